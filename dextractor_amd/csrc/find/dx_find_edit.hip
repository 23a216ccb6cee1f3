// dx_find_edit.hip -- where given sequences occur in packed reads with insertions and deletions allowed, searched where they lie.
//
//   dx_code_find_edit   per unit of a .bps / .arw / .dexta / .dexar payload: the ends at which a query lies within max_err edits   (k_find_edit)
//
// Nothing is decoded.  A unit is what it is for dx_code_find: symbols [beg, beg + len) of the packed read at in + boff, any byte
// offset, any phase.  For a query P of m <= 64 symbols and a bound k < m,
//     D(e) = min over 0 <= s <= e of Levenshtein(P, U[s, e))      (1 <= e <= L; substitution, insertion and deletion cost one each)
//     c(e) = min(D(e), k + 1),   c(0) = c(L + 1) = k + 1
// and a HIT is an end e with c(e) <= k, c(e) < c(e - 1) and c(e) <= c(e + 1): one hit for each valley of the distance, at the
// leftmost end of its floor.  pos = e is the EXCLUSIVE END of the occurrence, not its start; mis = D(e).  The start lies in
// [e - m - D(e), e - m + D(e)]; dx_code_hit_starts (find/dx_find_span.hip: the reverse pattern run backwards from e) finds it exactly,
// and dx_file_find_edit_spans lists it beside every hit of a file.
//
// D is computed by the bit-vector algorithm of Myers (1999) in the formulation of Hyyro: a column of the DP matrix is one word of
// vertical deltas (Pv, Mv), a text symbol costs a fixed number of word operations, and the semi-global form (the start in the read is
// free) shifts NO carry of 1 into the horizontal deltas.  The queries arrive as a kernel argument and are read with uniform indices,
// so they stand in SGPRs.  A query of at most 32 symbols takes the 32-bit instance of the same body (fe_scan<uint32_t>), a longer
// one the 64-bit instance.
// The match mask Eq of a text symbol c (bit i set when symbol i of the query is c) is not looked up in four masks Peq[c]: c differs
// from lane to lane, the masks stand in SGPRs, and the selection compiled to a divergent branch with both sides run, 18 vector
// instructions a symbol in the 64-bit instance.  The host leaves the query's two bit planes instead, and Eq = ~((b0 ^ B0) | (b1 ^ B1))
// with B0, B1 the symbol's two bits spread over a word: 6 instructions (4 in the 32-bit instance).  The query stands at the word's
// TOP, its last symbol in the top bit, so the score's delta is a shift by a constant; the bits below the query are kept neutral
// (Eq 0 there -- `low` is ORed in front of the complement --, so Pv stays 1, Mv 0, and nothing but zeros is shifted into the query).
//
// Stretches.  The scan of a unit is cut into independent pieces: a lane takes the ends [e0, e1) of one stretch of DX_FIND_EDIT_STRETCH
// ends, begins the standard column (Pv all ones, Mv 0, score m) at symbol max(0, e0 - 1 - (m + k)) and steps through symbol e1 (one
// symbol of lookahead for the valley rule; none at the unit's end, where c(L + 1) = k + 1).  This is exact: an alignment with at most
// k errors consumes at most m + k symbols, so a column begun at least m + k symbols in front of an end has min(D, k + 1) there, and
// the warm-up reaches back far enough for end e0 - 1 too, which the rule at e0 needs.  Only the ends in [e0, e1) are classified.
//
// Cost, counted from the compiled code (hipcc -O3 --offload-arch=gfx950 -S; the loop of fe_scan, a symbol and query, warm-up or not):
//   32-bit instance (m <= 32): 32 vector instructions -- 2 for the symbol's bits (v_ashrrev, v_bfe_i32), 3 for Eq, 11 for the column (7
//     v_bitop3, v_or, the add, 2 shifts), 3 for the score (v_lshrrev, v_ashrrev, v_add3), v_min, 4 v_cmp and a v_addc for the valley rule, and
//     7 that step on: the word's shift, the two counters, their compares, two moves;
//   64-bit instance: 50 -- the column's operations twice (v_bitop3 is not formed there: v_or3, v_not, v_bfi) and 64-bit shifts and adds.
//   A first version that selected Eq from four masks took 56 in the 64-bit instance (above).  profiles/find_edit_rate.txt has what
//   this gives: 10^9 positions and 64 queries in 86 ms at m = 20, k = 4 and 172 ms at m = 45, k = 9, beside k_find's 23.5 ms.
// The stretch's size follows from it: a stretch of S ends costs (S + m + k + 1) / S of the plain scan:
//     S = 64 (one 16-byte chunk, as in k_find):  1.39 x at m = 20, k = 4;  1.86 x at m = 45, k = 9;  3 x at m = 64, k = 63
//     S = 128:                                   1.20 x                    1.43 x                    2 x
//     S = 256:                                   1.10 x                    1.21 x                    1.5 x
// 128 is taken: a read of 10 000 symbols is 79 stretches and occupies the wave (at 256 it would fill 40 lanes of one step), the
// listing launch's place words (below) are 64 KiB of LDS a workgroup, and beyond it the warm-up's share falls slowly.
//
// The walk is k_find's: the waves draw tickets and take a ticket's units 64 a round, a lane reading one unit's parameters and
// checking its bounds; a unit of up to FE_LANE stretches is its lane's, stretch after stretch; one of up to 16 goes FOUR A STEP,
// a group of 16 lanes each, a stretch a lane; the others go one after the other by the whole wave, 64 stretches a step.  A lane
// reads its symbols 8 bytes at a time, once for every query (the words stay in the caches); what lies behind the buffer's end reads
// as zero and is never stepped through, and nothing outside [0, in_bytes) is read.
//
// The list.  The order (unit, pos, query) must be the same on every call, so nothing is placed by an atomic cursor: the counting
// launch leaves min(count, cap) a unit, dx_scan_u32 turns them into every unit's first place, and a second launch
// (k_find_edit<true>) goes over the units that have a place below cap again.  There a lane counts its stretch's hits end by end
// into its column of the workgroup's place words in LDS (one 16-bit word an end), wave_incl_scan gives the lane its first place, the
// column's running sums give every end its first place within the lane's, and a second pass over the queries writes each hit at
// its end's place, which then moves on by one: the queries go by in rising order, so the hits of one end stand in query order.
// None is written at cap or beyond.  cap == 0 runs the counting launch alone.
//
// Totals: a lane adds a query's hits in its stretch to the workgroup's words in LDS, the workgroup adds them to the global words at
// the kernel's end.
//
// This file stands outside the evidence set of profiles/ (profiles/check.py hashes csrc/*.hip), like find/dx_find.hip; its kernels
// are timed with events on the context's stream (tools/find_edit_rate.py).
#include "units/dx_units.hpp"
#include "find/dx_find_edit.hpp"           // fe_query, fe_queries, FE_QMAX: the queries as the kernel reads them (dx_find_span.hip's too)

extern "C" {
#include "dx_host.h"
}

#define FE_BATCH   1u                     // units a ticket at least
#define FE_TARGET  (4u << 10)              // packed bytes a ticket and query (a symbol costs some three times k_find's): FE_FLOOR at least
#define FE_FLOOR   (1u << 10)
#define FE_STRETCH DX_FIND_EDIT_STRETCH    // ends a lane takes at a time (dexgpu.h; the size is argued above)
#define FE_LANE    4u                      // stretches: a unit of up to so many is its lane's
#define FE_GROUP   UNITS_GROUP             // stretches: up to here 16 lanes take the unit, beyond the wave

// What a lane has of a unit: the ends [e0, e1) of the unit whose first symbol is symbol U0 of the buffer and which has L symbols
// (1 <= e0, e1 <= L + 1; e1 <= e0: nothing of it)
struct fe_part { uint64_t U0; uint32_t L, e0, e1; };

__device__ __forceinline__ fe_part fe_take(uint64_t U0, uint32_t L, uint32_t j)           // stretch j of the unit
{ fe_part p;
  p.U0 = U0; p.L = L;
  p.e0 = 1u + j * FE_STRETCH;                                                             // (L < 2^31: no overflow)
  p.e1 = L + 1u - p.e0 < FE_STRETCH ? L + 1u : p.e0 + FE_STRETCH;
  return p;
}

// FE_COUNT: the part's hits of one query are counted.  FE_PLACE: ... and each adds one to its end's word of the lane's column `col`
// (word p of it at col[p * DX_BLOCK]).  FE_WRITE: each is written at hits[base + its end's word], none at cap or beyond, and the
// word moves on by one.
enum { FE_COUNT = 0, FE_PLACE = 1, FE_WRITE = 2 };

template <typename W, int MODE>
__device__ __forceinline__ uint32_t fe_scan(const uint8_t *in, uint64_t bytes, const fe_part &p, const fe_query &q, uint32_t k,
                                            uint16_t *col, uint64_t unit, u32x4_u *hits, uint64_t base, uint64_t cap)
{ if (p.e1 <= p.e0) return 0u;
  const uint32_t m = q.len, err = q.err, over = err + 1u, reach = m + err;
  constexpr uint32_t WB = 8u * sizeof(W);                                        // (the 32-bit instance takes the planes' upper halves)
  const W        b0 = (W) (q.b0 >> (64u - WB)), b1 = (W) (q.b1 >> (64u - WB)), low = (W) (q.low >> (64u - WB));
  const uint32_t s = p.e0 - 1u > reach ? p.e0 - 1u - reach : 0u;                 // the first symbol the column steps through
  const uint32_t t = p.e1 <= p.L ? p.e1 : p.L;                                   // ... and behind the last: symbol e1 - 1 is the lookahead
  W        Pv = ~(W) 0, Mv = (W) 0;
  uint32_t score = m, ca = over, cb = over, n = 0;                               // cb = c(i), ca = c(i - 1) in front of symbol i

  uint64_t A = p.U0 + s, o = A >> 2;                                             // symbol s of the unit in the buffer, its byte
  uint64_t w = be64_at(in, bytes, o) << (2u * (uint32_t) (A & 3u));
  uint32_t have = 32u - (uint32_t) (A & 3u);                                     // symbols left in w
  for (uint32_t i = s; i < t; i++)
    { if (have == 0u) { o += 8u; w = be64_at(in, bytes, o); have = 32u; }
      const int32_t top = (int32_t) (w >> 32);                                   // the symbol: bits 31, 30
      const W B1 = (W) (int64_t) (top >> 31), B0 = (W) (int64_t) ((int32_t) ((uint32_t) top << 1) >> 31);      // its two bits, each all over a word
      w <<= 2; have--;
      const W Eq = ~(((b0 ^ B0) | low) | (b1 ^ B1));                             // the query's symbols that are this one; 0 below the query
      const W Xv = Eq | Mv;
      const W Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
      W Ph = Mv | ~(Xh | Pv);
      W Mh = Pv & Xh;
      score += (uint32_t) (Ph >> (WB - 1u));
      score -= (uint32_t) (Mh >> (WB - 1u));
      Ph <<= 1; Mh <<= 1;                                                        // (semi-global: no 1 comes in)
      Pv = Mh | ~(Xv | Ph);
      Mv = Ph & Xv;
      const uint32_t cn = score < over ? score : over;                           // c(i + 1)
      if (cb <= err && cb < ca && cb <= cn && i >= p.e0)                         // end i is a hit (i < e1 by the loop's bound)
        { if (MODE == FE_PLACE) col[(i - p.e0) * DX_BLOCK]++;
          if (MODE == FE_WRITE)
            { const uint64_t at = base + col[(i - p.e0) * DX_BLOCK]++;
              if (at < cap)
                { u32x4 h;
                  h.x = (uint32_t) unit; h.y = (uint32_t) (unit >> 32); h.z = i; h.w = k | (cb << 24);
                  hits[at] = h;
                }
            }
          n++;
        }
      ca = cb; cb = cn;
    }
  if (p.e1 == p.L + 1u && cb <= err && cb < ca && p.L >= p.e0)                   // the unit's last end: c(L + 1) = k + 1
    { if (MODE == FE_PLACE) col[(p.L - p.e0) * DX_BLOCK]++;
      if (MODE == FE_WRITE)
        { const uint64_t at = base + col[(p.L - p.e0) * DX_BLOCK]++;
          if (at < cap)
            { u32x4 h;
              h.x = (uint32_t) unit; h.y = (uint32_t) (unit >> 32); h.z = p.L; h.w = k | (cb << 24);
              hits[at] = h;
            }
        }
      n++;
    }
  return n;
}

// the part's hits over all queries; FE_COUNT: s_tot gets every query's
template <int MODE>
__device__ __forceinline__ uint32_t fe_all(const uint8_t *in, uint64_t bytes, const fe_part &p, const fe_queries &Q, uint32_t nq,
                                           unsigned long long *s_tot, uint16_t *col, uint64_t unit, u32x4_u *hits, uint64_t base, uint64_t cap)
{ uint32_t c = 0;
  if (p.e1 <= p.e0) return 0u;
  for (uint32_t k = 0; k < nq; k++)
    { const fe_query &q = Q.q[k];
      const uint32_t ck = q.len <= 32u ? fe_scan<uint32_t, MODE>(in, bytes, p, q, k, col, unit, hits, base, cap)
                                       : fe_scan<uint64_t, MODE>(in, bytes, p, q, k, col, unit, hits, base, cap);
      if (MODE == FE_COUNT && ck) atomicAdd(s_tot + k, (unsigned long long) ck);
      c += ck;
    }
  return c;
}

// the listing launch's first pass over a part: the column's words of the part's ends emptied, then the hits counted into them
__device__ __forceinline__ uint32_t fe_places(const uint8_t *in, uint64_t bytes, const fe_part &p, const fe_queries &Q, uint32_t nq, uint16_t *col)
{ if (p.e1 <= p.e0) return 0u;
  for (uint32_t e = 0; e < p.e1 - p.e0; e++) col[e * DX_BLOCK] = 0u;
  return fe_all<FE_PLACE>(in, bytes, p, Q, nq, NULL, col, 0ull, NULL, 0ull, 0ull);
}

// ... and its second: the words become every end's first place within the part's hits, and the hits are written from `base` on
__device__ __forceinline__ void fe_write(const uint8_t *in, uint64_t bytes, const fe_part &p, const fe_queries &Q, uint32_t nq, uint16_t *col,
                                         uint64_t unit, u32x4_u *hits, uint64_t base, uint64_t cap)
{ uint32_t run = 0;
  for (uint32_t e = 0; e < p.e1 - p.e0; e++)                                     // (at most FE_STRETCH x FE_QMAX = 8192 hits: 16 bits hold them)
    { const uint32_t here = col[e * DX_BLOCK];
      col[e * DX_BLOCK] = (uint16_t) run;
      run += here;
    }
  (void) fe_all<FE_WRITE>(in, bytes, p, Q, nq, NULL, col, unit, hits, base, cap);
}

// in holds in_bytes bytes and 16 at least; the units are checked against `bound` (as in k_find).
// LIST false: count (n, or NULL) gets every unit's hits, saturated; room (n, or NULL) min(hits, cap); total: nq words the workgroups
//   add to.
// LIST true: room as the first launch left it, start its exclusive sums (n + 1); the hits of every unit that has room go to
//   hits[start[i] ..), none at cap or beyond.
template <bool LIST>
__global__ __launch_bounds__(DX_BLOCK)
void k_find_edit(const uint8_t *__restrict__ in, uint64_t in_bytes, uint64_t bound, const uint64_t *__restrict__ boff,
                 const uint32_t *__restrict__ beg, const uint32_t *__restrict__ len, uint64_t n, const fe_queries Q, uint32_t nq,
                 uint32_t *__restrict__ count, uint32_t *__restrict__ room, const uint64_t *__restrict__ start,
                 u32x4_u *__restrict__ hits, uint64_t cap, unsigned long long *__restrict__ total,
                 unsigned long long *__restrict__ bad, uint32_t *__restrict__ ticket)
{ // LIST: a column of FE_STRETCH place words a lane (64 KiB); else the totals, a word a query
  __shared__ unsigned long long s_mem[LIST ? FE_STRETCH * DX_BLOCK / 4u : FE_QMAX];
  unsigned long long *s_tot = s_mem;
  uint16_t           *col   = (uint16_t *) s_mem + (LIST ? threadIdx.x : 0u);
  if (!LIST)
    { if (threadIdx.x < FE_QMAX) s_tot[threadIdx.x] = 0ull;
      __syncthreads();
    }

  const uint32_t lane = (uint32_t) lane_id(), sub = lane % UNITS_GROUP, grp = lane / UNITS_GROUP;
  units_rounds<false>(ticket, ticket_units_of(ticket, FE_BATCH), n, [&](uint64_t u0, uint64_t r1)
    { // unit u0 + lane is this lane's to read and to check
      const uint64_t    i  = u0 + lane;
      const packed_unit pu = packed_unit_take(boff, beg, len, i, r1, bound, bad);
      uint64_t U0 = 0, st = 0;                             // its first symbol in the buffer; its first place in the list
      uint32_t L = 0, nst = 0;                             // its symbols, its stretches
      bool     act = pu.ok;                                // it is searched in this launch
      if (pu.ok)
        { U0 = 4u * pu.at + pu.beg; L = pu.len;
          nst = (L + FE_STRETCH - 1u) / FE_STRETCH;
        }
      if (LIST)
        { st  = i < r1 ? start[i] : 0ull;
          act = pu.ok && room[i < r1 ? i : 0u] != 0u && i < r1 && st < cap;
        }
      else if (i < r1 && !pu.ok)
        { if (count != NULL) count[i] = 0u;
          if (room != NULL) room[i] = 0u;
        }

      // no symbol, or up to FE_LANE stretches: the lane's own, stretch after stretch
      if (act && nst <= FE_LANE)
        { uint64_t at = st;
          uint32_t c = 0;
          for (uint32_t j = 0; j < nst && (!LIST || at < cap); j++)
            { const fe_part p = fe_take(U0, L, j);
              if (LIST)
                { const uint32_t cj = fe_places(in, in_bytes, p, Q, nq, col);
                  if (cj) fe_write(in, in_bytes, p, Q, nq, col, i, hits, at, cap);
                  at += cj;
                }
              else c += fe_all<FE_COUNT>(in, in_bytes, p, Q, nq, s_tot, col, 0ull, NULL, 0ull, 0ull);
            }
          if (!LIST)
            { if (count != NULL) count[i] = c;
              if (room != NULL) room[i] = (uint64_t) c < cap ? c : (uint32_t) cap;
            }
        }

      // up to 16 stretches: lanes 16 g .. 16 g + 15 take unit k + g, a stretch each
      units_by_fours(__ballot(act && nst > FE_LANE && nst <= FE_GROUP), [&](int from, bool mine)
        { const uint64_t gU0 = __shfl(U0, from), gst = __shfl(st, from);
          const uint32_t gL  = __shfl(L, from), gn = __shfl(nst, from);
          fe_part p = { 0ull, 0u, 1u, 0u };
          if (mine && sub < gn) p = fe_take(gU0, gL, sub);
          if (LIST)
            { const uint32_t c    = fe_places(in, in_bytes, p, Q, nq, col);
              const uint32_t incl = wave_incl_scan(c);
              const uint32_t low  = __shfl(incl, (int) (grp ? UNITS_GROUP * grp - 1u : 0u));           // what the groups below have
              if (c) fe_write(in, in_bytes, p, Q, nq, col, u0 + (uint64_t) from, hits, gst + (incl - c - (grp ? low : 0u)), cap);
            }
          else
            { const uint32_t all = row_sum(fe_all<FE_COUNT>(in, in_bytes, p, Q, nq, s_tot, col, 0ull, NULL, 0ull, 0ull));
              if (mine && sub == UNITS_GROUP - 1u)
                { if (count != NULL) count[u0 + (uint64_t) from] = all;
                  if (room != NULL) room[u0 + (uint64_t) from] = (uint64_t) all < cap ? all : (uint32_t) cap;
                }
            }
        });

      // the others: the whole wave, 64 stretches a step
      units_each(__ballot(act && nst > FE_GROUP), [&](int from)
        { const uint64_t wU0 = uniform64(__shfl(U0, from));
          const uint32_t wL  = uniform(__shfl(L, from)), wn = uniform(__shfl(nst, from));
          uint64_t run = uniform64(__shfl(st, from)), mine = 0;           // LIST: the step's first place; else: this lane's hits
          for (uint32_t base = 0; base < wn; base += 64u)
            { const uint32_t j = base + lane;
              fe_part p = { 0ull, 0u, 1u, 0u };
              if (j < wn) p = fe_take(wU0, wL, j);
              if (LIST)
                { const uint32_t c    = fe_places(in, in_bytes, p, Q, nq, col);
                  const uint32_t incl = wave_incl_scan(c);
                  if (c) fe_write(in, in_bytes, p, Q, nq, col, u0 + (uint64_t) from, hits, run + (incl - c), cap);
                  run += wave_total(incl);
                  if (run >= cap) break;
                }
              else mine += fe_all<FE_COUNT>(in, in_bytes, p, Q, nq, s_tot, col, 0ull, NULL, 0ull, 0ull);
            }
          if (!LIST)
            { const uint64_t all = wave_sum64(mine);
              if (lane == 0u)
                { if (count != NULL) count[u0 + (uint64_t) from] = all < 0xffffffffull ? (uint32_t) all : 0xffffffffu;
                  if (room != NULL) room[u0 + (uint64_t) from] = (uint32_t) (all < cap ? all : cap);
                }
            }
        });
    });

  if (!LIST)
    { __syncthreads();
      if (threadIdx.x < nq && s_tot[threadIdx.x] != 0ull) atomicAdd(total + threadIdx.x, s_tot[threadIdx.x]);
    }
}

// ---------------------------------------------------------------------------------------------
//  the entry point
// ---------------------------------------------------------------------------------------------
static_assert(sizeof(dx_hit) == 16, "a hit is one 16-byte store");
static_assert(FE_STRETCH * FE_QMAX <= 0xffffu + 1u && FE_STRETCH * DX_BLOCK * 2u <= (64u << 10), "the place words: 16 bits each, 64 KiB a workgroup");

extern "C" int dx_code_find_edit(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes,
                                 const uint64_t *d_boff, const uint32_t *d_beg, const uint32_t *d_len, uint64_t n,
                                 const dx_equery *q, uint32_t nq, uint32_t *d_count, dx_hit *d_hits, uint64_t cap,
                                 uint64_t total[], uint64_t *hits, uint64_t *bad_unit)
{ if (ctx == NULL) return DX_E_ARG;
  if (bad_unit) *bad_unit = UINT64_MAX;
  if (hits) *hits = 0;
  if (nq < 1u || nq > FE_QMAX) return dx_fail(ctx, DX_E_ARG, "dx_code_find_edit: %u queries (1 to %u)", nq, FE_QMAX);
  if (q == NULL || hits == NULL || (d_hits == NULL && cap)) return dx_fail(ctx, DX_E_ARG, "dx_code_find_edit: NULL pointer");
  if (cap > 0xffffffffull) return dx_fail(ctx, DX_E_ARG, "dx_code_find_edit: a list of more than 2^32 - 1 hits");
  if (total) memset(total, 0, (size_t) nq * 8u);
  fe_queries Q;
  int rq = fe_queries_make(ctx, "dx_code_find_edit", q, nq, false, &Q);
  if (rq != DX_OK) return rq;
  if (n >= (1ull << 31)) return dx_fail(ctx, DX_E_ARG, "dx_code_find_edit: more than 2^31 - 1 units in one batch");
  if (n == 0) return DX_OK;

  // one scratch block: the frame and the nq totals, then (with a list) every unit's first place and its room
  units_frame    f;
  uint64_t       back[UF_OUT + FE_QMAX], *d_start = NULL;
  uint32_t      *d_room = NULL;
  const uint64_t bound = in_bytes;
  int rc = units_list_begin(ctx, "dx_code_find_edit", n, d_boff && d_len && (d_in || !in_bytes), FE_QMAX, 16, cap != 0, &d_in, &in_bytes, &f, &d_start, &d_room);
  if (rc != DX_OK) return rc;
  const int      grid   = dx_grid_waves(ctx, n, 16);
  const uint32_t target = FE_TARGET / nq > FE_FLOOR ? FE_TARGET / nq : FE_FLOOR;
  hipLaunchKernelGGL(k_ticket_units, dim3(1), dim3(1), 0, ctx->stream, d_boff, d_boff + (n - 1), (const uint32_t *) NULL, n,
                     target, FE_BATCH, f.ticket);
  hipLaunchKernelGGL(k_find_edit<false>, dim3(grid), dim3(DX_BLOCK), 0, ctx->stream, d_in, in_bytes, bound, d_boff, d_beg, d_len, n, Q, nq,
                     d_count, d_room, (const uint64_t *) NULL, (u32x4_u *) NULL, cap, f.out, f.bad, f.ticket);
  if (cap)
    { uint64_t listed = 0;
      if ((rc = units_list_places(ctx, f, d_room, n, d_start, &listed)) != DX_OK) return rc;
      if (listed)
        hipLaunchKernelGGL(k_find_edit<true>, dim3(grid), dim3(DX_BLOCK), 0, ctx->stream, d_in, in_bytes, bound, d_boff, d_beg, d_len, n,
                           Q, nq, (uint32_t *) NULL, d_room, (const uint64_t *) d_start, (u32x4_u *) d_hits, cap,
                           (unsigned long long *) NULL, f.bad, f.ticket);
    }
  rc = units_end(ctx, f, back, bad_unit, "%s: unit %llu does not lie inside the %llu packed bytes", bound);
  for (uint32_t k = 0; k < nq; k++)
    { if (total) total[k] = back[UF_OUT + k];
      *hits += back[UF_OUT + k];
    }
  return rc;
}

// dx_host.h: dx_file_find_edit.c's refusals, worded there
extern "C" int dx_find_edit_fail(dx_ctx *ctx, int code, const char *what)
{ if (ctx == NULL) return code;
  return dx_fail(ctx, code, "dx_file_find_edit: %s", what);
}
