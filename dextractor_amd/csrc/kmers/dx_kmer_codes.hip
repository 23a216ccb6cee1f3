// dx_kmer_codes.hip -- the k-mers of packed reads written out, 1 <= k <= 32: every window's code as a 64-bit word, at a fixed place.
//
//   dx_code_kmer_codes   per unit of a .bps / .arw / .dexta / .dexar payload: window p of unit j -> codes[off[j] + p]   (k_kc_windows, k_kc_codes)
//
// The first step of the wide route: beyond k = 14 a table of 4^k cells is out of the question and a hashed one would put
// every window on the path of the global atomic requests, which dx_kmers.hip measured as the slow one.  Here a window costs one plain
// store; dx_sort_u64 (sort/dx_sort.hip) and dx_kmer_runs (dx_kmer_runs.hip) make counts of the codes.
//
// A unit is what it is for dx_code_kmers: symbols [beg, beg + len) of the packed read at in + boff, any byte offset, any phase.  A
// window's code is its symbols as a base-4 number, the first on top, in the low 2 k bits of the word -- the top 2 k bits of the 64 bits
// that dx_find.hip holds for a position, moved down.  With `canonical` it is min(code, rc), compared unsigned (at k = 32 the top bit is
// in use).  Places: off = the exclusive sums of w_j = max(0, len_j - k + 1), a unit that does not lie inside the buffer counting 0:
// kc_windows_places (kmers/dx_kmer_windows.hpp: k_kc_windows, dx_scan_u32) leaves the w_j, the sums and the total, which the host holds
// against cap before anything is written.
//
// The walk is kc_walk (kmers/dx_kmer_windows.hpp, which says how it goes): tickets, 64 units a round, a unit of up to KC_LANE chunks by
// its lane, of up to 16 by 16 lanes, the others by the whole wave; what is done with a chunk stands here (kc_write), and the unit's
// first window's place travels with it.  A lane holds its chunk and the 8 bytes behind it (a window of
// up to 32 symbols that begins in the chunk ends there at the latest) as three 64-bit words in the read's bit order, moved up to the
// first position that is the unit's and at which a window begins (kc_take, as fd_take); a position's code is one shift of the upper
// word, and the words move up two bits a position.  The reverse strand rolls along in a second 64-bit register, as in k_kmers:
// rc(p + 1) = rc(p) >> 2 | (3 - s) << (2 k - 2) with s the symbol that entered; the first form (bit reversal, kc_rc) starts it, once a
// chunk.  Nothing outside [0, in_bytes) is read (last16_ask, units_begin's pad).
//
// Cost a window, counted from the source: the code 2 (v_lshrrev_b64), the words' move 3 shifts of 64 bits and 2 v_alignbit-like
// funnel shifts (about 8), canonical + 6 (v_lshrrev_b64, v_not / v_and, v_lshlrev_b64, 2 v_or, v_cmp + 2 v_cndmask), the store's address
// 2 and the global_store_dwordx2: about 15 to 20 vector instructions -- 10^9 windows in 0.5 ms on 39 T lane-instructions/s.  Bytes: 8
// written a window, 0.25 read.  A lane writes its up to 64 windows one behind the other, 512 bytes, so a store instruction of the wave
// touches 64 different 128-byte lines and a line is filled by 16 instructions of one lane; the lines are completed in the L2 before
// they leave.  ESTIMATE: the 8 GB of 10^9 windows at half the rate of a copy's writes, about 4 to 5 ms.  MEASURED
// (profiles/kmer_wide_rate.txt, 10^5 reads x 10 kb, the two small launches, the prefix sum and its read-back included): 4.65 ms
// at k = 14, 16, 21 and 32 alike, 1.7 TB/s of codes written, 1.4 times a device-to-device copy of the same 8 GB (3.3 ms, which
// moves 16 GB): bound by the stores, not by the walk (dx_code_counts reads the same units in 0.34 ms).  Stores of whole lines -- the
// wave's 64 x 64 codes turned in LDS -- are what would lift it; not built.
//
// This file stands outside the evidence set of profiles/ (profiles/check.py hashes csrc/*.hip); its kernels have no entry in the
// profiler's name table and are timed with events on the context's stream (tools/kmer_wide_rate.py).
#include "kmers/dx_kmer_windows.hpp"

extern "C" {
#include "dx_host.h"
}

// ---------------------------------------------------------------------------------------------
//  k_kc_codes
// ---------------------------------------------------------------------------------------------
// the part's codes, one behind the other from out[0] on
template <bool CANON>
__device__ __forceinline__ void kc_write(const kc_part &p, uint32_t k, uint64_t *out)
{ if (p.n == 0u) return;
  uint64_t w0 = p.w0, w1 = p.w1, w2 = p.w2;
  const uint32_t down = 64u - 2u * k, top = 2u * k - 2u;
  uint64_t rcw = CANON ? kc_rc(w0, k) << 2 : 0ull;         // (the first step moves it down again and sets the top symbol it has already)
  for (uint32_t i = 0; i < p.n; i++)
    { uint64_t cur = w0 >> down;
      if (CANON)
        { rcw = (rcw >> 2) | ((~cur & 3ull) << top);
          cur = cur < rcw ? cur : rcw;
        }
      out[i] = cur;
      w0 = (w0 << 2) | (w1 >> 62); w1 = (w1 << 2) | (w2 >> 62); w2 <<= 2;
    }
}

// in holds in_bytes bytes and 16 at least; the units are checked against `bound` (as in k_code_counts).  off: the exclusive sums of
// k_kc_windows' counts; codes holds off[n] words at least.
template <bool CANON>
__global__ __launch_bounds__(DX_BLOCK)
void k_kc_codes(const uint8_t *__restrict__ in, uint64_t in_bytes, uint64_t bound, const uint64_t *__restrict__ boff,
                const uint32_t *__restrict__ beg, const uint32_t *__restrict__ len, uint64_t n, uint32_t k,
                const uint64_t *__restrict__ off, uint64_t *__restrict__ codes, unsigned long long *__restrict__ bad,
                uint32_t *__restrict__ ticket)
{ const uint32_t lane = (uint32_t) lane_id();
  units_rounds<false>(ticket, ticket_units_of(ticket, KC_BATCH), n, [&](uint64_t u0, uint64_t r1)
    { // unit u0 + lane is this lane's to read and to check; its first window's place travels with it
      const uint64_t    i  = u0 + lane;
      const packed_unit pu = packed_unit_take(boff, beg, len, i, r1, bound, bad);
      const kc_unit     e  = kc_unit_of(pu, k);
      const kc_place    at = { e.nch ? off[i] : 0ull, 0u };
      kc_walk(e, at, [&](uint64_t a, const kc_unit &u, const kc_place &to)
        { const kc_part p = kc_take(in, in_bytes, a, u.S0, u.S1, k);
          kc_write<CANON>(p, k, codes + to.to + p.first);
        });
    });
}

// ---------------------------------------------------------------------------------------------
//  the entry point
// ---------------------------------------------------------------------------------------------
extern "C" int dx_code_kmer_codes(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes,
                                  const uint64_t *d_boff, const uint32_t *d_beg, const uint32_t *d_len, uint64_t n,
                                  uint32_t k, int canonical, uint64_t *d_codes, uint64_t cap, uint64_t *windows, uint64_t *bad_unit)
{ if (ctx == NULL) return DX_E_ARG;
  if (bad_unit) *bad_unit = UINT64_MAX;
  if (windows) *windows = 0;
  if (k < 1u || k > KC_KMAX) return dx_fail(ctx, DX_E_ARG, "dx_code_kmer_codes: k = %u (1 to %u)", k, KC_KMAX);
  if (windows == NULL || (d_codes == NULL && cap)) return dx_fail(ctx, DX_E_ARG, "dx_code_kmer_codes: NULL pointer");
  if (n >= (1ull << 31)) return dx_fail(ctx, DX_E_ARG, "dx_code_kmer_codes: more than 2^31 - 1 units in one batch");
  if (n == 0) return DX_OK;

  // one scratch block: the frame, then every unit's first place (n + 1) and its windows (n)
  units_frame    f;
  uint64_t       back[UF_OUT + 1], *d_off = NULL, total = 0;
  uint32_t      *d_win = NULL;
  const uint64_t bound = in_bytes;
  int rc = units_list_begin(ctx, "dx_code_kmer_codes", n, d_boff && d_len && (d_in || !in_bytes), 1, 16, true, &d_in, &in_bytes, &f, &d_off, &d_win);
  if (rc != DX_OK) return rc;
  if ((rc = kc_windows_places(ctx, d_boff, d_beg, d_len, n, bound, k, d_win, d_off, &total)) != DX_OK) return rc;
  *windows = total;
  if (total > cap)
    return dx_fail(ctx, DX_E_NOMEM, "dx_code_kmer_codes: %llu windows, and room for %llu codes", (unsigned long long) total, (unsigned long long) cap);

  const int grid = dx_grid_waves(ctx, n, 16);
  kc_tickets(ctx, d_boff, n, f);
  if (canonical) hipLaunchKernelGGL(k_kc_codes<true>, dim3(grid), dim3(DX_BLOCK), 0, ctx->stream, d_in, in_bytes, bound, d_boff, d_beg, d_len, n,
                                    k, (const uint64_t *) d_off, d_codes, f.bad, f.ticket);
  else           hipLaunchKernelGGL(k_kc_codes<false>, dim3(grid), dim3(DX_BLOCK), 0, ctx->stream, d_in, in_bytes, bound, d_boff, d_beg, d_len, n,
                                    k, (const uint64_t *) d_off, d_codes, f.bad, f.ticket);
  return units_end(ctx, f, back, bad_unit, "%s: unit %llu does not lie inside the %llu packed bytes", bound);
}
