// dx_kmer_codes_range.hip -- dx_code_kmer_codes for a range of the codes: only the windows whose code falls into bins
// [bin_lo, bin_hi) of its top `bits` bits are written, densely, in the order (unit, position).
//
//   dx_code_kmer_codes_range   bin_lo <= code >> (2 k - bits) < bin_hi  ->  codes[...]          (k_kc_range<CANON, false>, k_kc_range<CANON, true>)
//
// One pass of a wide count that does not fit the device at once (dx_files_kmers_wide, dx_file_kmers_files.c): the bins
// (dx_code_kmer_bins) say how many windows a range holds, this writes them out, dx_sort_u64 and dx_kmer_runs count them.  The range
// is stated in bins so that k = 32 needs no 2^64.
//
// The array is the same on every call, so nothing is placed by an atomic cursor; the places come as k_find's and k_spans' do:
//   1. a counting launch (LIST false) leaves every unit's kept windows in w[j] -- a lane's own sum for a unit of up to KC_LANE
//      chunks, the sum along the 16 lanes of a unit of up to 16 (row_sum), the wave's sum over its steps for the others;
//   2. dx_scan_u32 gives every unit's first place and the total, which the host holds against cap before anything is written;
//   3. a listing launch (LIST true) goes over the units that keep a window (off[j + 1] > off[j]; the others cost their three loads):
//      a lane carries its running place from chunk to chunk; on the 16-lane and the wave route a lane counts its chunk's kept
//      codes first, a scan over the lanes' counts (wave_incl_scan) places the chunk -- on the 16-lane route less what the rows in
//      front hold, on the wave route plus a carry across the wave's steps -- and the lane walks its chunk again and writes.
// The code is the shared one (kc_take, kc_roll), and so are the unit's extent and its way to a group's lanes and to the wave
// (kc_unit_of, kc_unit_from, kc_unit_uniform: kmers/dx_kmer_windows.hpp, which says how the walk goes); the three routes differ in how
// they sum and place, so their bodies stand here.
//
// Cost, ESTIMATE: the counting launch is dx_code_kmer_bins' walk without the LDS (the same order as k_kmers' LDS route, 0.5 to 0.8
// ms for 10^9 positions); the listing launch walks a chunk twice on two of its routes and stores what k_kc_codes stores for the
// kept share: bound by the stores as that kernel is (4.65 ms for 10^9 windows kept), the second walk cheap beside them
// (dx_code_counts walks 10^9 positions in 0.34 ms).  MEASURED (profiles/kmer_files_rate.txt, tools/kmer_files_rate.py; 10^9 windows,
// k = 21 canonical, the prefix sum and its read-back included): all 4096 bins kept 5.79 ms beside dx_code_kmer_codes' 4.77 in the
// same run -- the counting launch and the second walk cost 1.0 ms --, the quarter of the windows in bins [0, 549) 2.70 ms.
//
// A kernel beside k_kc_codes, not a template parameter of it: the two existing instances keep their code and their registers
// (DESIGN.md 4).  This file stands outside the evidence set of profiles/ (profiles/check.py hashes csrc/*.hip).
#include "kmers/dx_kmer_windows.hpp"

extern "C" {
#include "dx_host.h"
}

#define KR_BITS_MAX 12u                    // dx_code_kmer_bins' bound: the bins are its

// ---------------------------------------------------------------------------------------------
//  k_kc_range
// ---------------------------------------------------------------------------------------------
// what is kept: lo <= code >> down < lo + span
struct kr_keep { uint32_t down, lo, span; };

__device__ __forceinline__ bool kr_in(const kr_keep &K, uint64_t code) { return (uint32_t) (code >> K.down) - K.lo < K.span; }

// the part's kept windows
template <bool CANON>
__device__ __forceinline__ uint32_t kr_count(const kc_part &p, uint32_t k, const kr_keep &K)
{ uint32_t kept = 0;
  if (p.n == 0u) return kept;
  kc_roll<CANON> R(p, k);
  for (uint32_t i = 0; i < p.n; i++)
    { kept += kr_in(K, R.code()) ? 1u : 0u;
      R.step();
    }
  return kept;
}

// the part's kept codes, one behind the other from out[0] on; how many there were
template <bool CANON>
__device__ __forceinline__ uint32_t kr_write(const kc_part &p, uint32_t k, const kr_keep &K, uint64_t *out)
{ uint32_t kept = 0;
  if (p.n == 0u) return kept;
  kc_roll<CANON> R(p, k);
  for (uint32_t i = 0; i < p.n; i++)
    { const uint64_t cur = R.code();
      if (kr_in(K, cur)) out[kept++] = cur;
      R.step();
    }
  return kept;
}

// in holds in_bytes bytes and 16 at least; the units are checked against `bound`.  LIST false: w[j] = unit j's kept windows (0 for a
// unit without a window and one that does not lie inside `bound`); off and codes are not read.  LIST true: off = the exclusive
// sums of those counts (n + 1 of them), codes holds off[n] words at least; w is not read.
template <bool CANON, bool LIST>
__global__ __launch_bounds__(DX_BLOCK)
void k_kc_range(const uint8_t *__restrict__ in, uint64_t in_bytes, uint64_t bound, const uint64_t *__restrict__ boff,
                const uint32_t *__restrict__ beg, const uint32_t *__restrict__ len, uint64_t n, uint32_t k, kr_keep K,
                uint32_t *__restrict__ w, const uint64_t *__restrict__ off, uint64_t *__restrict__ codes,
                unsigned long long *__restrict__ bad, uint32_t *__restrict__ ticket)
{ const uint32_t lane = (uint32_t) lane_id(), sub = lane % UNITS_GROUP, grp = lane / UNITS_GROUP;
  units_rounds<false>(ticket, ticket_units_of(ticket, KC_BATCH), n, [&](uint64_t u0, uint64_t r1)
    { // unit u0 + lane is this lane's to read and to check
      const uint64_t    i  = u0 + lane;
      const packed_unit pu = packed_unit_take(boff, beg, len, i, r1, bound, bad);
      uint64_t to = 0;                                     // its first kept code's place
      bool     any = true;                                 // it keeps a window (LIST)
      if (LIST && pu.ok && pu.len >= k) { to = off[i]; any = off[i + 1u] > to; }
      const kc_unit e = kc_unit_of(pu, k, any);

      // up to KC_LANE chunks: the lane's own, chunk after chunk
      uint32_t own = 0;
      if (e.nch && e.nch <= KC_LANE)
        for (uint32_t j = 0; j < e.nch; j++)
          { const kc_part p = kc_take(in, in_bytes, e.a0 + 16u * j, e.S0, e.S1, k);
            if (LIST) to += kr_write<CANON>(p, k, K, codes + to);
            else      own += kr_count<CANON>(p, k, K);
          }
      if (!LIST && i < r1 && e.nch <= KC_LANE) w[i] = own; // (nch 0: no window, or no good unit)

      // up to 16 chunks: lanes 16 g .. 16 g + 15 take unit k + g, a chunk each
      units_by_fours(__ballot(e.nch > KC_LANE && e.nch <= KC_GROUP), [&](int from, bool mine)
        { const kc_unit  g   = kc_unit_from(e, from);
          const uint64_t gto = __shfl(to, from);
          const bool     on  = mine && sub < g.nch;
          kc_part p = { 0ull, 0ull, 0ull, 0u, 0u };
          if (on) p = kc_take(in, in_bytes, g.a0 + 16u * sub, g.S0, g.S1, k);
          const uint32_t kept = kr_count<CANON>(p, k, K);
          if (LIST)
            { const uint32_t incl  = wave_incl_scan(kept);
              const uint32_t front = __shfl(incl, (int) (grp ? UNITS_GROUP * grp - 1u : 0u));           // what the rows in front hold
              if (on && kept) kr_write<CANON>(p, k, K, codes + gto + (incl - kept - (grp ? front : 0u)));
            }
          else
            { const uint32_t all = row_sum(kept);
              if (mine && sub == UNITS_GROUP - 1u) w[u0 + (uint32_t) from] = all;
            }
        });

      // the others: the whole wave, 64 chunks a step
      units_each(__ballot(e.nch > KC_GROUP), [&](int from)
        { const kc_unit  u   = kc_unit_uniform(e, from);
          const uint64_t wto = uniform64(__shfl(to, from));
          uint64_t carry = 0;                              // the unit's kept codes in the steps before this one
          for (uint32_t base = 0; base < u.nch; base += 64u)
            { const uint32_t j = base + lane;
              kc_part p = { 0ull, 0ull, 0ull, 0u, 0u };
              if (j < u.nch) p = kc_take(in, in_bytes, u.a0 + 16ull * j, u.S0, u.S1, k);
              const uint32_t kept = kr_count<CANON>(p, k, K);
              const uint32_t incl = wave_incl_scan(kept);
              if (LIST && kept) kr_write<CANON>(p, k, K, codes + wto + carry + (incl - kept));
              carry += wave_total(incl);
            }
          if (!LIST && lane == 0u) w[u0 + (uint32_t) from] = (uint32_t) carry;
        });
    });
}

// ---------------------------------------------------------------------------------------------
//  the entry point
// ---------------------------------------------------------------------------------------------
template <bool LIST>
static void kr_launch(dx_ctx *ctx, int grid, int canonical, const uint8_t *d_in, uint64_t in_bytes, uint64_t bound, const uint64_t *d_boff,
                      const uint32_t *d_beg, const uint32_t *d_len, uint64_t n, uint32_t k, kr_keep K, uint32_t *d_w,
                      const uint64_t *d_off, uint64_t *d_codes, const units_frame &f)
{ if (canonical) hipLaunchKernelGGL((k_kc_range<true, LIST>), dim3(grid), dim3(DX_BLOCK), 0, ctx->stream, d_in, in_bytes, bound, d_boff, d_beg,
                                    d_len, n, k, K, d_w, d_off, d_codes, f.bad, f.ticket);
  else           hipLaunchKernelGGL((k_kc_range<false, LIST>), dim3(grid), dim3(DX_BLOCK), 0, ctx->stream, d_in, in_bytes, bound, d_boff, d_beg,
                                    d_len, n, k, K, d_w, d_off, d_codes, f.bad, f.ticket);
}

extern "C" int dx_code_kmer_codes_range(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes,
                                        const uint64_t *d_boff, const uint32_t *d_beg, const uint32_t *d_len, uint64_t n,
                                        uint32_t k, int canonical, uint32_t bits, uint32_t bin_lo, uint32_t bin_hi,
                                        uint64_t *d_codes, uint64_t cap, uint64_t *windows, uint64_t *bad_unit)
{ const char *who = "dx_code_kmer_codes_range";
  if (ctx == NULL) return DX_E_ARG;
  if (bad_unit) *bad_unit = UINT64_MAX;
  if (windows) *windows = 0;
  if (k < 1u || k > KC_KMAX) return dx_fail(ctx, DX_E_ARG, "%s: k = %u (1 to %u)", who, k, KC_KMAX);
  if (bits < 1u || bits > KR_BITS_MAX || bits > 2u * k)
    return dx_fail(ctx, DX_E_ARG, "%s: bits = %u (1 to %u)", who, bits, 2u * k < KR_BITS_MAX ? 2u * k : KR_BITS_MAX);
  if (bin_lo > bin_hi || bin_hi > (1u << bits))
    return dx_fail(ctx, DX_E_ARG, "%s: bins [%u, %u) of %u", who, bin_lo, bin_hi, 1u << bits);
  if (windows == NULL || (d_codes == NULL && cap)) return dx_fail(ctx, DX_E_ARG, "%s: NULL pointer", who);
  if (n >= (1ull << 31)) return dx_fail(ctx, DX_E_ARG, "%s: more than 2^31 - 1 units in one batch", who);
  if (n == 0) return DX_OK;

  // one scratch block: the frame, then every unit's first place (n + 1) and its kept windows (n)
  units_frame    f;
  uint64_t       back[UF_OUT + 1], *d_off = NULL, total = 0;
  uint32_t      *d_win = NULL;
  const uint64_t bound = in_bytes;
  int rc = units_list_begin(ctx, who, n, d_boff && d_len && (d_in || !in_bytes), 1, 16, true, &d_in, &in_bytes, &f, &d_off, &d_win);
  if (rc != DX_OK) return rc;
  const kr_keep K    = { 2u * k - bits, bin_lo, bin_hi - bin_lo };
  const int     grid = dx_grid_waves(ctx, n, 16);
  kc_tickets(ctx, d_boff, n, f);
  kr_launch<false>(ctx, grid, canonical, d_in, in_bytes, bound, d_boff, d_beg, d_len, n, k, K, d_win, (const uint64_t *) NULL, (uint64_t *) NULL, f);
  if ((rc = units_list_places(ctx, f, d_win, n, d_off, &total)) != DX_OK) return rc;
  *windows = total;
  if (total > cap)
    return dx_fail(ctx, DX_E_NOMEM, "%s: %llu windows in the range, and room for %llu codes", who, (unsigned long long) total, (unsigned long long) cap);

  if (total) kr_launch<true>(ctx, grid, canonical, d_in, in_bytes, bound, d_boff, d_beg, d_len, n, k, K, (uint32_t *) NULL, (const uint64_t *) d_off, d_codes, f);
  return units_end(ctx, f, back, bad_unit, "%s: unit %llu does not lie inside the %llu packed bytes", bound);
}
