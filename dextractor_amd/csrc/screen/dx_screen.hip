// dx_screen.hip -- which windows of packed reads are in a set of k-mers, and how much of each read they cover.
//
//   dx_code_kmer_screen   per unit of a .bps / .arw / .dexta / .dexar payload: {hits, covered, first, last} against a dx_kmer_set   (k_screen)
//
// A unit is what it is for dx_code_kmer_codes: symbols [beg, beg + len) of the packed read at in + boff, any byte offset, any phase.
// A window's code is made as k_kc_codes makes it (kmers/dx_kmer_windows.hpp: kc_take, kc_roll) with the set's k and canonical.  For a
// unit, hits = the windows whose code is in the set, covered = the symbols that lie in one such window at least, first / last = the
// smallest and the largest position of such a window (UINT32_MAX: none).
//
// The walk is the one kmers/dx_kmer_windows.hpp describes: tickets, 64 units a round, a lane reading one unit's parameters and checking
// its bounds; a unit of up to KC_LANE chunks (16 packed bytes = 64 positions on 16-byte boundaries of the buffer) is its lane's, one
// of up to 16 goes four a step by 16 lanes each -- one step: the group has a lane a chunk --, the others by the whole wave, 64 chunks
// a step.  The unit's extent and its way to the group and to the wave are that header's (kc_unit_of, kc_unit_from, kc_unit_uniform);
// the three tiers join a unit's chunks differently, so their bodies stand here.
//
// The look-up (sc_mask).  b = code >> (2 k - p) chooses the bucket; first[b] and first[b + 1] come from ONE 8-byte load at a 4-byte
// boundary (gfx950 runs with unaligned access); then codes[lo .. hi) is searched: by bisection while more than SC_LINEAR codes are
// left, then one after the other.  With the natural p a bucket holds half a code on the average: two DEPENDENT loads a window and
// seldom a third.  So a lane takes SC_BATCH = 8 positions at a time (as k_find holds 8 windows): their 8 codes first, then all 8
// first[] loads asked for before any is waited for, then the 8 first codes of the buckets, then the few that need more.  A
// position past the part's windows still makes a code of the words (zeros behind the buffer) and asks for a bucket that exists --
// b < 2^p whatever the code --; its answer is masked off.
//
// The coverage.  A lane's up to 64 positions give one hit mask M_c, bit j = the window that begins at position j of the chunk.  The
// symbols of the chunk that lie in a hit window are D_c = OR_{i < k} (M_c << i | M_{c-1} >> (64 - i)): the 128 bits (M_c, M_{c-1})
// smeared upwards over k places in log2 k steps (sc_cover), k <= 32 < 64 so only the one chunk in front matters.  M_{c-1} is 0 at the
// unit's first chunk, the lane's own last mask on the lane path, the lane before's on the other two (__shfl_up: ds_bpermute), and
// across the wave path's steps lane 63's, kept wave-uniform.  Only positions at which a window of the UNIT begins are ever set, so
// every covered symbol lies inside the unit by construction, and the unit's last chunk, in which no window may begin, gets its
// share from M_{c-1} alone.
//
// The totals (windows, hits, covered, units with a hit): four 64-bit registers a lane, added up in LDS at the kernel's end, then one
// vector atomicAdd a word and workgroup, as in k_code_counts.  Per unit one 16-byte store by the unit's leader; a unit that does not
// lie in the buffer gets {0, 0, UINT32_MAX, UINT32_MAX}, adds nothing, and the smallest such index goes back with DX_E_FORMAT.
//
// An LDS copy of a small set: not built -- the small-set case stands at 1.2 times the store-bound codes kernel without one.  Cost a
// window beside the walk's (about 10 vector instructions for the code): the bucket's address 3, the two loads, 2 compares, the mask 2.
// MEASURED (profiles/screen_rate.txt, 10^5 reads x 10 kb, k = 21 canonical, 10^9 windows; dx_code_kmer_codes over the same units
// 4.77 ms, dx_code_counts 0.27 ms): 5.75 ms against 4.8 x 10^4 codes (0.9 MB with the index: L2), 22.6 ms against 5 x 10^6 (107 MB:
// Infinity Cache), 40 ms against 10^8 (1 GB: HBM) with none or 1 % of the windows in the set; 8.5 / 36.0 / 45.6 ms with all of them.
// Bound by the rate of the gathers (45 to 55 G a second from the Infinity Cache), not by the walk.  Writing and sorting the reads'
// codes for a merge instead costs 4.77 + 49 ms before the merge: the look-up is under it at every size, by a quarter at 10^8 codes,
// where a partitioned look-up (the codes bucketed by their top bits, a bucket of the set staged in LDS) is the next step.
//
// This file stands outside the evidence set of profiles/ (profiles/check.py hashes csrc/*.hip); its kernels have no entry in the
// profiler's name table and are timed with events on the context's stream (tools/screen_rate.py).
#include "screen/dx_screen_look.hpp"

extern "C" {
#include "dx_host.h"
}

// ---------------------------------------------------------------------------------------------
//  k_screen  (sc_set, sc_mask, sc_cover, sc_chunk_mask: screen/dx_screen_look.hpp, which k_spans shares)
// ---------------------------------------------------------------------------------------------
// what a lane has gathered of a unit
struct sc_acc { uint32_t hits, covered, first, last; };

// ... added to the lane's account; base = 4 a - S0: the chunk's first position as a symbol of the unit (negative in the first chunk)
__device__ __forceinline__ void sc_add(sc_acc &x, uint64_t m, uint64_t prev, int64_t base, uint32_t k)
{ x.hits += (uint32_t) __popcll((unsigned long long) m);
  x.covered += (uint32_t) __popcll((unsigned long long) sc_cover(m, prev, k));
  if (m)
    { const uint32_t f = (uint32_t) (base + (int64_t) (__ffsll((unsigned long long) m) - 1)), l = (uint32_t) (base + 63 - (int64_t) __clzll((long long) m));
      if (x.first == SC_NONE || f < x.first) x.first = f;
      if (x.last == SC_NONE || l > x.last) x.last = l;
    }
}

// two lanes' accounts of one unit joined (o: the other's)
__device__ __forceinline__ void sc_join(sc_acc &x, uint32_t d)
{ const uint32_t oh = (uint32_t) __shfl_xor((int) x.hits, (int) d), oc = (uint32_t) __shfl_xor((int) x.covered, (int) d);
  const uint32_t of = (uint32_t) __shfl_xor((int) x.first, (int) d), ol = (uint32_t) __shfl_xor((int) x.last, (int) d);
  x.hits += oh; x.covered += oc;
  x.first = of < x.first ? of : x.first;                               // (SC_NONE is the largest value)
  x.last = ol != SC_NONE && (x.last == SC_NONE || ol > x.last) ? ol : x.last;
}

__device__ __forceinline__ void sc_store(dx_screen *out, uint64_t i, const sc_acc &x)
{ if (out == NULL) return;
  u32x4 e;
  e.x = x.hits; e.y = x.covered; e.z = x.first; e.w = x.last;
  *(u32x4_u *) (out + i) = e;                           // (one store at any 4-byte boundary: a driver's d_extra is 8-byte aligned)
}

// in holds in_bytes bytes and 16 at least; the units are checked against `bound` (as in k_kc_codes).  out: n entries or NULL;
// total: windows, hits, covered, units with a hit.
template <bool CANON>
__global__ __launch_bounds__(DX_BLOCK)
void k_screen(const uint8_t *__restrict__ in, uint64_t in_bytes, uint64_t bound, const uint64_t *__restrict__ boff,
              const uint32_t *__restrict__ beg, const uint32_t *__restrict__ len, uint64_t n, sc_set s,
              dx_screen *__restrict__ out, unsigned long long *__restrict__ total, unsigned long long *__restrict__ bad,
              uint32_t *__restrict__ ticket)
{ __shared__ unsigned long long s_tot[4];
  if (threadIdx.x < 4u) s_tot[threadIdx.x] = 0ull;
  __syncthreads();

  const uint32_t lane = (uint32_t) lane_id(), sub = lane % UNITS_GROUP, k = s.k;
  uint64_t t_win = 0, t_hit = 0, t_cov = 0, t_unit = 0;
  units_rounds<false>(ticket, ticket_units_of(ticket, KC_BATCH), n, [&](uint64_t u0, uint64_t r1)
    { // unit u0 + lane is this lane's to read and to check
      const uint64_t    i  = u0 + lane;
      const packed_unit pu = packed_unit_take(boff, beg, len, i, r1, bound, bad);
      const kc_unit     e  = kc_unit_of(pu, k);
      if (e.nch) t_win += pu.len - k + 1u;
      const sc_acc none = { 0u, 0u, SC_NONE, SC_NONE };

      // no window (too short, or not in the buffer), or up to KC_LANE chunks: the lane's own, chunk after chunk
      if (i < r1 && e.nch <= KC_LANE)
        { sc_acc   x = none;
          uint64_t prev = 0ull;
          for (uint32_t j = 0; j < e.nch; j++)
            { const uint64_t a = e.a0 + 16u * j, m = sc_chunk_mask<CANON>(in, in_bytes, a, e.S0, e.S1, s);
              sc_add(x, m, prev, (int64_t) (4u * a) - (int64_t) e.S0, k);
              prev = m;
            }
          t_hit += x.hits; t_cov += x.covered; t_unit += x.hits ? 1u : 0u;
          sc_store(out, i, x);
        }

      // up to 16 chunks: lanes 16 g .. 16 g + 15 take unit k + g, a chunk each
      units_by_fours(__ballot(e.nch > KC_LANE && e.nch <= KC_GROUP), [&](int from, bool mine)
        { const kc_unit  g   = kc_unit_from(e, from);
          const bool     on  = mine && sub < g.nch;
          const uint64_t a   = g.a0 + 16u * sub;
          const uint64_t m   = on ? sc_chunk_mask<CANON>(in, in_bytes, a, g.S0, g.S1, s) : 0ull;
          const uint64_t up  = (uint64_t) __shfl_up((unsigned long long) m, 1u);
          sc_acc x = none;
          if (on) sc_add(x, m, sub ? up : 0ull, (int64_t) (4u * a) - (int64_t) g.S0, k);
          t_hit += x.hits; t_cov += x.covered;
          #pragma unroll
          for (uint32_t d = 1; d < UNITS_GROUP; d <<= 1) sc_join(x, d);
          if (mine && sub == 0u)
            { t_unit += x.hits ? 1u : 0u;
              sc_store(out, u0 + (uint64_t) from, x);
            }
        });

      // the others: the whole wave, 64 chunks a step
      units_each(__ballot(e.nch > KC_GROUP), [&](int from)
        { const kc_unit w = kc_unit_uniform(e, from);
          sc_acc   x = none;
          uint64_t carry = 0ull;                                         // lane 63's mask of the step before (wave-uniform)
          for (uint32_t base = 0; base < w.nch; base += 64u)
            { const uint32_t j = base + lane;
              const uint64_t a = w.a0 + 16ull * j;
              const uint64_t m = j < w.nch ? sc_chunk_mask<CANON>(in, in_bytes, a, w.S0, w.S1, s) : 0ull;
              const uint64_t up = (uint64_t) __shfl_up((unsigned long long) m, 1u);
              if (j < w.nch) sc_add(x, m, lane ? up : carry, (int64_t) (4u * a) - (int64_t) w.S0, k);
              carry = uniform64((uint64_t) __shfl((unsigned long long) m, 63));
            }
          t_hit += x.hits; t_cov += x.covered;
          #pragma unroll
          for (uint32_t d = 1; d < 64u; d <<= 1) sc_join(x, d);
          if (lane == 0u)
            { t_unit += x.hits ? 1u : 0u;
              sc_store(out, u0 + (uint64_t) from, x);
            }
        });
    });

  if (t_win)  atomicAdd(&s_tot[0], (unsigned long long) t_win);
  if (t_hit)  atomicAdd(&s_tot[1], (unsigned long long) t_hit);
  if (t_cov)  atomicAdd(&s_tot[2], (unsigned long long) t_cov);
  if (t_unit) atomicAdd(&s_tot[3], (unsigned long long) t_unit);
  __syncthreads();
  if (threadIdx.x < 4u && s_tot[threadIdx.x] != 0ull) atomicAdd(total + threadIdx.x, s_tot[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------
//  the entry point
// ---------------------------------------------------------------------------------------------
static_assert(sizeof(dx_screen) == 16 && sizeof(dx_screen_report) == 56, "an entry is one 16-byte store");

extern "C" int dx_code_kmer_screen(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes,
                                   const uint64_t *d_boff, const uint32_t *d_beg, const uint32_t *d_len, uint64_t n,
                                   const dx_kmer_set *set, dx_screen *d_out, uint64_t total[4], uint64_t *bad_unit)
{ if (ctx == NULL) return DX_E_ARG;
  if (bad_unit) *bad_unit = UINT64_MAX;
  if (total) total[0] = total[1] = total[2] = total[3] = 0;
  if (set == NULL) return dx_fail(ctx, DX_E_ARG, "dx_code_kmer_screen: no set");
  if (total == NULL) return dx_fail(ctx, DX_E_ARG, "dx_code_kmer_screen: NULL pointer");
  if (((uintptr_t) d_out & 3u) != 0u) return dx_fail(ctx, DX_E_ARG, "dx_code_kmer_screen: d_out is not 4-byte aligned");
  if (n >= (1ull << 31)) return dx_fail(ctx, DX_E_ARG, "dx_code_kmer_screen: more than 2^31 - 1 units in one batch");
  if (n == 0) return DX_OK;

  units_frame    f;
  uint64_t       back[UF_OUT + 4];
  const uint64_t bound = in_bytes;
  int rc = units_begin(ctx, "dx_code_kmer_screen", n, d_boff && d_len && (d_in || !in_bytes), NULL, 4, 16, &d_in, &in_bytes, &f);
  if (rc != DX_OK) return rc;
  const sc_set s = sc_set_of(set);
  const int grid = dx_grid_waves(ctx, n, 16);
  kc_tickets(ctx, d_boff, n, f);
  if (set->canonical) hipLaunchKernelGGL(k_screen<true>, dim3(grid), dim3(DX_BLOCK), 0, ctx->stream, d_in, in_bytes, bound, d_boff, d_beg, d_len,
                                         n, s, d_out, f.out, f.bad, f.ticket);
  else                hipLaunchKernelGGL(k_screen<false>, dim3(grid), dim3(DX_BLOCK), 0, ctx->stream, d_in, in_bytes, bound, d_boff, d_beg, d_len,
                                         n, s, d_out, f.out, f.bad, f.ticket);
  rc = units_end(ctx, f, back, bad_unit, "%s: unit %llu does not lie inside the %llu packed bytes", bound);
  if (rc == DX_OK || rc == DX_E_FORMAT)
    for (int t = 0; t < 4; t++) total[t] = back[UF_OUT + t];
  return rc;
}

// dx_host.h: dx_file_screen.c's refusals, worded there
extern "C" int dx_screen_fail(dx_ctx *ctx, int code, const char *what)
{ if (ctx == NULL) return code;
  return dx_fail(ctx, code, "dx_file_screen: %s", what);
}
