// dx_place_vote.hip -- from a unit's seeds to its place on the reference: a vote over diagonals.
//
//   dx_seeds_place   per unit the best band of diagonals, its votes and the extents of its seeds   (k_vote_keys, k_vote)
//
// A seed {unit, pos, gpos, strand} lies on the 32-bit diagonal  gpos - pos + 2^31  (strand 0)  or  gpos + pos  (strand 1) -- along
// either a read that matches the reference without indels keeps one value -- and in the bin  diag >> band_bits.  c(s, b) = the
// unit's seeds of strand s in bin b.  The best (s, b), among those with c(s, b) > 0, has the largest c(s, b) + c(s, b + 1) -- a band
// two bins wide, so that a place that straddles a bin's edge is not halved; a bin beyond the last counts 0 --, on a tie the smaller
// s, then the smaller b.  The voted seeds are those of strand s in bin b or b + 1; the answer is dx_place {seeds, votes, strand,
// diag = b << band_bits, rbeg, rend, gbeg, gend}: min pos and max pos + k, min gpos and max gpos + k over the voted seeds.  A unit
// without a seed gets {0, 0, 0, UINT32_MAX x 5}.
//
// The positions are GLOBAL: a band that runs from one target's end into the next target's start counts the seeds of both.
// Per-target bands are NOT built (toff on the host says which target gbeg lies in; dx_place_select cuts gend at that target's end).
// This is seed-and-vote placement and NOT alignment: no chaining, no base-level alignment, no CIGAR.
//
// k_vote_keys writes, a thread a seed, the key  unit << (33 - band_bits) | strand << (32 - band_bits) | bin  into scratch.
// dx_sort_u64 sorts the keys with exactly the bits in use, bits(n - 1) + 33 - band_bits; the unit is the top field, so unit j's sorted
// keys stand in [off[j], off[j + 1]) again.  k_vote<false> takes 64 units a round: a stretch of up to VT_LANE keys is its lane's, one
// of up to VT_GROUP goes four a step by 16 lanes each; the others go to the whole wave in a launch of their own, k_vote<true>, ONE
// unit a ticket -- measured: with 64 a ticket the few waves that drew the matching reads took 11 ms over 10^7 seeds while the device
// stood idle (vt_unit<1 / 16 / 64>, one body).  A lane looks at the keys i = first, first + width, ..: where key[i - 1] != key[i]
// a run (s, b) begins; its end and the end of the run (s, b + 1) behind it are found by doubling steps and a bisection over the sorted keys (vt_bound: 2 log2 of the run's length loads, from the
// L2 that the lane's neighbours have just filled), so the votes are a difference of two places and no run is walked.  A lane's
// candidates come in ascending (s, b), so keeping the first of the largest obeys the tie rule; across lanes the pair (votes, (s, b))
// is reduced by __shfl_xor.  The same lanes then walk the unit's UNSORTED seeds for the four extents, one 16-byte load a seed, and
// check every seed's unit against its stretch.
//
// Device memory per seed: 16 bytes for the seed, 8 for the key and 8 for the sort's second array (both made and freed here).
//
// ESTIMATE (before the first run; 10^5 reads x 10 kb at k = 21, every read matching once: 10^9 seeds).  Keys: 16 GB read, 8 written,
// 5 to 6 ms.  The sort: bits(10^5 - 1) + 33 - band_bits = 17 + 25 = 42 bits at band_bits 8, 6 passes of 16 bytes a key: 96 GB, 25 to
// 30 ms at HBM's rate -- the largest part.  k_vote: 8 + 16 GB read, few runs a unit when the reads match (one band holds nearly all
// seeds): 6 to 8 ms.  About 40 ms in all, 40 ns a read-kilobase.  With 1 % of the reads matching, 10^7 seeds: launches, under 1 ms.
// MEASURED (profiles/place_rate.txt, the same workload, medians of 5 after a warm-up).  10^9 seeds: 56 to 57 ms, of which the sort
// alone (dx_sort_u64 of as many 42-bit keys) 47 to 49 ms -- 8 ms a pass, not the 4 to 5 estimated -- and the rest, keys, vote and
// extents, 8 to 10 ms where 11 to 14 were estimated.  10^7 seeds: 2.4 to 2.6 ms, 0.65 of it the sort; the rest is two device arrays
// made and freed a call, three launches and three read-backs, not the 1 ms estimated.  The first call of a size pays the arrays'
// first allocation (2.4 s for 16 GB: the rounds' maximum).
//
// This file stands outside the evidence set of profiles/ (profiles/check.py hashes csrc/*.hip); its kernels have no entry in the
// profiler's name table and are timed with events on the context's stream (tools/place_rate.py).
#include "units/dx_units.hpp"

#define VT_LANE   4u                       // keys: a stretch of up to so many is its lane's
#define VT_GROUP  256u                     // keys: up to here 16 lanes take the stretch, beyond the wave
#define VT_ROUND  64u                      // units a ticket

// a seed's diagonal
__device__ __forceinline__ uint32_t vt_diag(const u32x4 &e) { return e.w ? e.z + e.y : e.z - e.y + 0x80000000u; }

// ---------------------------------------------------------------------------------------------
//  k_vote_keys
// ---------------------------------------------------------------------------------------------
// key[i] = seed[i]'s unit (its low `ubits` bits), strand and bin, one below the other
__global__ __launch_bounds__(DX_BLOCK)
void k_vote_keys(const u32x4_u *__restrict__ seed, uint64_t n, uint32_t band_bits, uint32_t ubits, uint64_t *__restrict__ key)
{ const uint64_t i = (uint64_t) blockIdx.x * DX_BLOCK + threadIdx.x;
  if (i >= n) return;
  const u32x4    e = seed[i];
  const uint64_t u = ubits ? (uint64_t) e.x & ((1ull << ubits) - 1u) : 0ull;
  key[i] = (u << (33u - band_bits)) | ((uint64_t) (e.w & 1u) << (32u - band_bits)) | (uint64_t) (vt_diag(e) >> band_bits);
}

// ---------------------------------------------------------------------------------------------
//  k_vote
// ---------------------------------------------------------------------------------------------
// the first place in (lo, hi) whose key's low field is above `top`, hi if there is none; key[lo]'s is not above it
__device__ __forceinline__ uint64_t vt_bound(const uint64_t *__restrict__ key, uint64_t lo, uint64_t hi, uint64_t mask, uint64_t top)
{ uint64_t step = 1u, up = lo + 1u;
  while (up < hi && (key[up] & mask) <= top) { lo = up; step *= 2u; up = lo + step; }      // key[lo] <= top; up: above, or beyond hi
  if (up > hi) up = hi;
  while (up - lo > 1u)                                     // key[lo] <= top < key[up] (or up == hi)
    { const uint64_t mid = lo + (up - lo) / 2u;
      if ((key[mid] & mask) <= top) lo = mid; else up = mid;
    }
  return up;
}

// One unit by WIDTH lanes (1, 16 or 64; `first` = this lane's number among them): its stretch [o0, o1) of the sorted keys and of the
// seeds, o1 > o0.  Every lane of the WIDTH gets the answer's two halves.
template <uint32_t WIDTH>
__device__ __forceinline__ void vt_unit(const u32x4_u *__restrict__ seed, const uint64_t *__restrict__ key, uint64_t o0, uint64_t o1,
                                        uint32_t first, uint32_t unit, uint32_t k, uint32_t band_bits, unsigned long long *bad_seed,
                                        u32x4 &e0, u32x4 &e1)
{ const uint64_t mask = (1ull << (33u - band_bits)) - 1u, last = (1ull << (32u - band_bits)) - 1u;      // the low field; the last bin
  uint32_t votes = 0u;
  uint64_t best = ~0ull;                                   // (s, b) as the key holds it
  for (uint64_t i = o0 + first; i < o1; i += WIDTH)
    { const uint64_t v = key[i] & mask;
      if (i != o0 && (key[i - 1u] & mask) == v) continue;  // (not a run's first key)
      const uint64_t top = (v & last) != last ? v + 1u : v;                   // the band's upper bin: b + 1, of the same strand
      const uint32_t c   = (uint32_t) (vt_bound(key, i, o1, mask, top) - i);
      if (c > votes) { votes = c; best = v; }
    }
  #pragma unroll
  for (int d = (int) WIDTH / 2; d > 0; d >>= 1)
    { const uint32_t ov = (uint32_t) __shfl_xor((int) votes, d);
      const uint64_t ob = (uint64_t) __shfl_xor((unsigned long long) best, d);
      if (ov > votes || (ov == votes && ob < best)) { votes = ov; best = ob; }
    }

  // the extents, over the unit's seeds as they were listed
  const uint32_t s = (uint32_t) (best >> (32u - band_bits)) & 1u, b = (uint32_t) (best & last);
  uint32_t rb = 0xffffffffu, re = 0u, gb = 0xffffffffu, ge = 0u;
  for (uint64_t i = o0 + first; i < o1; i += WIDTH)
    { const u32x4 e = seed[i];
      if (e.x != unit) atomicMin(bad_seed, (unsigned long long) i);
      const uint32_t bin = vt_diag(e) >> band_bits;
      if ((e.w & 1u) == s && (bin == b || (b != (uint32_t) last && bin == b + 1u)))
        { rb = min(rb, e.y); re = max(re, e.y + k); gb = min(gb, e.z); ge = max(ge, e.z + k); }
    }
  #pragma unroll
  for (int d = (int) WIDTH / 2; d > 0; d >>= 1)
    { rb = min(rb, (uint32_t) __shfl_xor((int) rb, d)); re = max(re, (uint32_t) __shfl_xor((int) re, d));
      gb = min(gb, (uint32_t) __shfl_xor((int) gb, d)); ge = max(ge, (uint32_t) __shfl_xor((int) ge, d));
    }
  e0.x = (uint32_t) (o1 - o0); e0.y = votes; e0.z = s; e0.w = band_bits < 32u ? b << band_bits : 0u;
  e1.x = rb; e1.y = re; e1.z = gb; e1.w = ge;
}

// off[0 .. n]: the units' stretches in seed and key (both begin at the arrays' first entry: off[0] has been taken off by the host),
// all: the entries there are.  A stretch that ends in front of its beginning, beyond `all`, or holds 2^32 entries or more counts as
// empty and goes to *bad_off.  total: seeds, votes, units placed.
// HEAVY false: the stretches of up to VT_GROUP keys, 64 units a ticket.  HEAVY true: the others, ONE unit a ticket -- a wave that
// drew 64 long stretches at once would work through them alone while the rest of the device waited.
template <bool HEAVY>
__global__ __launch_bounds__(DX_BLOCK)
void k_vote(const u32x4_u *__restrict__ seed, const uint64_t *__restrict__ key, const uint64_t *__restrict__ off, uint64_t n, uint64_t all,
            uint32_t k, uint32_t band_bits, u32x4_u *__restrict__ out, unsigned long long *__restrict__ total,
            unsigned long long *__restrict__ bad_off, unsigned long long *__restrict__ bad_seed, uint32_t *__restrict__ ticket)
{ __shared__ unsigned long long s_tot[3];
  if (threadIdx.x < 3u) s_tot[threadIdx.x] = 0ull;
  __syncthreads();

  const uint32_t lane = (uint32_t) lane_id(), sub = lane % UNITS_GROUP;
  const u32x4    none0 = { 0u, 0u, 0u, 0xffffffffu }, none1 = { 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu };
  uint64_t t_seed = 0, t_vote = 0, t_unit = 0;
  auto leave = [&](uint64_t unit, const u32x4 &e0, const u32x4 &e1)
    { t_seed += e0.x; t_vote += e0.y; t_unit += e0.x ? 1u : 0u;
      out[2u * unit] = e0; out[2u * unit + 1u] = e1;
    };
  if (HEAVY)
    { const uint64_t base = uniform64(off[0]);
      for (uint64_t j = next_unit(ticket); j < n; j = next_unit(ticket))
        { const uint64_t a = uniform64(off[j]), b = uniform64(off[j + 1u]);
          if (!(a >= base && b >= a && b - base <= all && b - a <= 0xffffffffull) || b - a <= VT_GROUP) continue;
          u32x4 e0 = none0, e1 = none1;
          vt_unit<64u>(seed, key, a - base, b - base, lane, (uint32_t) j, k, band_bits, bad_seed, e0, e1);
          if (lane == 0u) leave(j, e0, e1);
        }
    }
  else
    units_rounds<false>(ticket, VT_ROUND, n, [&](uint64_t u0, uint64_t r1)
      { const uint64_t i = u0 + lane, base = off[0];
        uint64_t o0 = 0, o1 = 0;                             // unit i's stretch
        bool     ok = false;
        if (i < r1)
          { const uint64_t a = off[i], b = off[i + 1u];
            ok = a >= base && b >= a && b - base <= all && b - a <= 0xffffffffull;
            if (ok) { o0 = a - base; o1 = b - base; }
            else atomicMin(bad_off, (unsigned long long) i);
          }
        const uint64_t w = o1 - o0;

        if (i < r1 && w <= VT_LANE)
          { u32x4 e0 = none0, e1 = none1;
            if (w) vt_unit<1u>(seed, key, o0, o1, 0u, (uint32_t) i, k, band_bits, bad_seed, e0, e1);
            leave(i, e0, e1);
          }

        units_by_fours(__ballot(w > VT_LANE && w <= VT_GROUP), [&](int from, bool mine)
          { const uint64_t g0 = __shfl(o0, from), s1 = __shfl(o1, from), g1 = mine ? s1 : g0;  // (not one of them: an empty stretch)
            u32x4 e0 = none0, e1 = none1;
            vt_unit<UNITS_GROUP>(seed, key, g0, g1, sub, (uint32_t) (u0 + (uint64_t) from), k, band_bits, bad_seed, e0, e1);
            if (mine && sub == 0u) leave(u0 + (uint64_t) from, e0, e1);
          });
      });

  if (t_seed) atomicAdd(&s_tot[0], (unsigned long long) t_seed);
  if (t_vote) atomicAdd(&s_tot[1], (unsigned long long) t_vote);
  if (t_unit) atomicAdd(&s_tot[2], (unsigned long long) t_unit);
  __syncthreads();
  if (threadIdx.x < 3u && s_tot[threadIdx.x] != 0ull) atomicAdd(total + threadIdx.x, s_tot[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------
//  the entry point
// ---------------------------------------------------------------------------------------------
static_assert(sizeof(dx_place) == 32 && sizeof(dx_place_report) == 80, "a place is two 16-byte stores");

extern "C" int dx_seeds_place(dx_ctx *ctx, const dx_seed *d_seeds, const uint64_t *d_off, uint64_t n, uint32_t k, uint32_t band_bits,
                              dx_place *d_out, uint64_t total[3])
{ const char *who = "dx_seeds_place";
  if (ctx == NULL) return DX_E_ARG;
  if (total) total[0] = total[1] = total[2] = 0;
  if (total == NULL || (n && (d_off == NULL || d_out == NULL))) return dx_fail(ctx, DX_E_ARG, "%s: NULL pointer", who);
  if (k < 1u || k > 32u) return dx_fail(ctx, DX_E_ARG, "%s: k = %u (1 to 32)", who, k);
  if (band_bits > 31u) return dx_fail(ctx, DX_E_ARG, "%s: band_bits = %u (0 to 31)", who, band_bits);
  if (((uintptr_t) d_seeds & 3u) != 0u || ((uintptr_t) d_off & 7u) != 0u || ((uintptr_t) d_out & 3u) != 0u)
    return dx_fail(ctx, DX_E_ARG, "%s: d_seeds, d_off or d_out is not aligned", who);
  if (n >= (1ull << 31)) return dx_fail(ctx, DX_E_ARG, "%s: more than 2^31 - 1 units in one batch", who);
  if (n == 0) return DX_OK;
  DX_HIP(ctx, hipSetDevice(ctx->device));

  // the stretches' two ends come down: how many seeds there are
  uint64_t ends[2] = { 0, 0 };
  int rc = dx_d2h(ctx, &ends[0], d_off, 8);
  if (rc == DX_OK) rc = dx_d2h(ctx, &ends[1], d_off + n, 8);
  if (rc != DX_OK) return rc;
  if (ends[1] < ends[0]) return dx_fail(ctx, DX_E_FORMAT, "%s: d_off decreases: %llu seeds in front of the first unit, %llu at the last one's end", who,
                                        (unsigned long long) ends[0], (unsigned long long) ends[1]);
  const uint64_t all = ends[1] - ends[0];
  if (all >= (1ull << 36)) return dx_fail(ctx, DX_E_ARG, "%s: %llu seeds (fewer than 2^36)", who, (unsigned long long) all);
  if (all && d_seeds == NULL) return dx_fail(ctx, DX_E_ARG, "%s: NULL pointer", who);
  const dx_seed *seeds = d_seeds + ends[0];

  uint32_t ubits = 0;
  while (ubits < 32u && ((n - 1u) >> ubits) != 0u) ubits++;
  uint64_t *d_key = NULL, *d_tmp = NULL;
  if (all)
    { if ((rc = dx_malloc(ctx, (size_t) all * 8u + 64u, (void **) &d_key)) != DX_OK) return rc;
      if ((rc = dx_malloc(ctx, (size_t) all * 8u + 64u, (void **) &d_tmp)) != DX_OK) { (void) dx_free(ctx, d_key); return rc; }
    }
  rc = [&]() -> int
    { if (all)
        { hipLaunchKernelGGL(k_vote_keys, dim3((unsigned) ((all + DX_BLOCK - 1u) / DX_BLOCK)), dim3(DX_BLOCK), 0, ctx->stream,
                             (const u32x4_u *) seeds, all, band_bits, ubits, d_key);
          DX_HIP(ctx, hipGetLastError());
          const int r = dx_sort_u64(ctx, d_key, d_tmp, all, ubits + 33u - band_bits);
          if (r != DX_OK) return r;
        }
      units_frame f;
      uint64_t    back[UF_OUT + 4];
      int r = units_begin(ctx, who, n, true, NULL, 4, 0, NULL, NULL, &f);
      if (r != DX_OK) return r;
      DX_HIP(ctx, hipMemsetAsync(f.out + 3, 0xff, 8, ctx->stream));
      hipLaunchKernelGGL(k_vote<false>, dim3(dx_grid_waves(ctx, (n + VT_ROUND - 1u) / VT_ROUND, 16)), dim3(DX_BLOCK), 0, ctx->stream,
                         (const u32x4_u *) seeds, (const uint64_t *) d_key, d_off, n, all, k, band_bits, (u32x4_u *) d_out, f.out, f.bad,
                         f.out + 3, f.ticket);
      if (all > VT_GROUP)                                  // (a stretch of more than VT_GROUP keys may exist)
        { DX_HIP(ctx, hipMemsetAsync(f.ticket, 0, 4, ctx->stream));
          hipLaunchKernelGGL(k_vote<true>, dim3(dx_grid_waves(ctx, n, 16)), dim3(DX_BLOCK), 0, ctx->stream,
                             (const u32x4_u *) seeds, (const uint64_t *) d_key, d_off, n, all, k, band_bits, (u32x4_u *) d_out, f.out, f.bad,
                             f.out + 3, f.ticket);
        }
      r = units_end(ctx, f, back, NULL, "%s: d_off decreases (or leaves 2^32 seeds or more, or more than there are) behind index %llu", 0);
      if (r == DX_OK || r == DX_E_FORMAT)
        for (int t = 0; t < 3; t++) total[t] = back[UF_OUT + t];
      if (r == DX_OK && back[UF_OUT + 3] != UINT64_MAX)
        r = dx_fail(ctx, DX_E_FORMAT, "%s: seed %llu does not name the unit in whose stretch it stands", who,
                    (unsigned long long) (back[UF_OUT + 3] + ends[0]));
      return r;
    }();
  if (d_key) (void) dx_free(ctx, d_key);
  if (d_tmp) (void) dx_free(ctx, d_tmp);
  return rc;
}
