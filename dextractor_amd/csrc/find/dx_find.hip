// dx_find.hip -- where given short sequences occur in packed reads, searched where they lie.
//
//   dx_code_find   per unit of a .bps / .arw / .dexta / .dexar payload: the windows that are within max_mis symbols of a query   (k_find)
//
// Nothing is decoded.  A unit is what it is for dx_code_counts: symbols [beg, beg + len) of the packed read at in + boff, symbol i
// in byte i >> 2 at bits 7 - 2 (i & 3), 6 - 2 (i & 3) (DB.c:319-338), any byte offset, any phase.  A query of m <= 32 symbols is
// one 64-bit word, its first symbol on top as in a packed read, so a window of the read is too: position p is tested as
//     d = w(p) ^ code;   popc((d | d >> 1) & mask) <= max_mis
// with w(p) the 64 bits of the buffer that begin at symbol p, code the query moved to the word's top 2 m bits and mask the even
// bits of those.  Only positions p with beg <= p and p + m <= beg + len are tested, and only the top 2 m bits of w(p) pass the
// mask: the symbols in front of the unit, those behind it, the pad bits of a read's last byte and every byte that is not the
// unit's stand below the mask or in no tested window, whatever they hold.
//
// The walk is k_code_counts': the waves draw tickets (k_ticket_units) and take a ticket's units 64 a round, a lane reading one
// unit's parameters and checking its bounds; the unit is walked in chunks of 16 packed bytes = 64 positions that stand on 16-byte
// boundaries of the buffer, and
//   * a unit of up to four chunks is its lane's, chunk after chunk (FD_LANE: reads of up to some 200 symbols, 64 a round);
//   * one of up to 16 chunks (FD_GROUP) goes FOUR A STEP, a group of 16 lanes each, a chunk a lane;
//   * the others go one after the other by the whole wave, 64 chunks = FD_STEP positions a step.
// A lane holds its chunk and the 8 bytes behind it (a window that begins in the chunk ends there at the latest) as three 64-bit
// words in the read's own bit order.  It takes FD_BLOCK = 8 positions at a time: their windows are made once, two funnel shifts
// each, and stay in registers while the queries go by; a query's matches are gathered as bits and counted under the mask of the
// positions at which it may begin; then the words move up 16 bits.  Nothing outside [0, in_bytes) is read: the 16 bytes that
// would reach past the buffer's end are its last 16 (last16_ask) moved up, zeros behind them, and a buffer of fewer than 16 bytes
// is copied into the frame's pad first (units_begin).
// The queries arrive as a kernel argument and are read with uniform indices: they stand in SGPRs (s_load_dwordx4 + x2 a block
// and query), never fetched per position.
//
// Cost, counted from the compiled code (hipcc -O3 --offload-arch=gfx950 --save-temps; the unrolled blocks of fd_count):
//   word form, as built, vector instructions a position and query:
//     10 for a query of 17 to 32 symbols -- 2 v_xor, 2 v_lshrrev, 2 v_bitop3 ((d | d >> 1) & mask), 2 v_bcnt, v_cmp, and one of
//        v_cndmask / v_or3 / v_lshl_or that gathers the match bits -- and 6.3 for one of at most 16 (FD_NARROW: the upper word alone);
//     + 1.25: ten a block and query for the positions' mask and the count (v_sub, v_min3, v_bfe, 2 v_cmp, 2 v_cndmask, v_bitop3, v_bcnt, v_add);
//     + 2.75 / nq: 16 v_alignbit for the block's windows and 6 to move the words up, shared by the queries.
//     That is 11.3 (7.5) with many queries, 14 (10.3) with one.  A first version that moved the words up a position at a time inside
//     every query's loop took 18 + 3 scalar (13 + 3); measured 43.1 ms against 23.5 ms for 64 queries over 10^9 positions.
//   bit-sliced form, estimated, NOT built: with the chunk as four planes (is-a, is-c, is-g, is-t: 64 positions a register pair), an
//     exact query is one 64-bit AND a symbol of the plane its symbol names moved by its place -- but the moved planes must be made:
//     2 funnel shifts a plane, place and pair, 16 m a chunk, shared by the queries only if 4 x m pairs (256 registers for m = 32)
//     stay live; made again per query they cost 4 m + 2 m a chunk = 1.9 a position for m = 20, and exact queries would be about five
//     times cheaper than here.  With mismatches the ANDs become a bit-sliced counter (about 5 operations a symbol): 3.2 for m = 20,
//     still ahead.  It is the next step for this kernel; the word form was taken because one body serves every length and every
//     number of mismatches, and its order of hits is the list's.
//   profiles/find_rate.txt has what the word form gives.
//
// The list.  The order (unit, position, query) must be the same on every call, so nothing is placed by an atomic cursor: the
// counting launch leaves min(count, cap) a unit, dx_scan_u32 turns them into every unit's first place, and a second launch
// (k_find<true>) goes over the units that have a place below cap again: per step a lane counts its chunk's hits, wave_incl_scan
// gives it its first place, and it writes its hits position by position, query by query, none at cap or beyond.  cap == 0 runs
// the counting launch alone.  (With a list the scan's total is read back besides the frame: two waits for the stream a call.)
//
// Totals: a lane adds a query's hits in its chunk to the workgroup's words in LDS (only a chunk that has a hit costs anything),
// the workgroup adds them to the global words at the kernel's end.
//
// This file stands outside the evidence set of profiles/ (profiles/check.py hashes csrc/*.hip); its kernels have no entry in
// the profiler's name table and are timed with events on the context's stream (tools/find_rate.py).
#include "units/dx_units.hpp"

extern "C" {
#include "dx_host.h"
}

#define FD_QMAX    64u                     // queries a call
#define FD_BATCH   1u                      // units a ticket at least
#define FD_TARGET  (16u << 10)             // packed bytes a ticket and query: a ticket is about so many bytes / nq, FD_FLOOR at least
#define FD_FLOOR   (1u << 10)              // ... 64 chunks: a round of 64 one-chunk units, a step of four 16-chunk units, one longer unit
#define FD_CHUNK   64u                     // positions a chunk (16 packed bytes)
#define FD_LANE    4u                      // chunks: a unit of up to so many is its lane's
#define FD_GROUP   UNITS_GROUP             // chunks: up to here 16 lanes take the unit, beyond the wave
#define FD_STEP    (64u * FD_CHUNK)        // positions the wave takes a step
#define FD_BLOCK   8u                      // positions whose windows a lane holds while the queries go by (16 bits of the words)
#define FD_ALL     ((1u << FD_BLOCK) - 1u)
#define FD_NARROW  16u                     // symbols: a query up to here is decided by the window's upper word
#define FD_EVEN64  0x5555555555555555ull

struct fd_query   { uint64_t code, mask; uint32_t len, mis; };       // code and mask in the top 2 len bits of the word
struct fd_queries { fd_query q[FD_QMAX]; };

// What a lane has of a unit in one chunk: the chunk's positions [t0, t1) and the three words moved up to t0; `left`: the symbols
// from position t0 to the unit's end, so that query k may begin at t0 + d while d + len_k <= left.
struct fd_part { uint64_t w0, w1, w2; uint32_t t0, t1, left; };

// the chunk at byte a of the buffer against the unit that is symbols [S0, S1) of the buffer; t1 == t0: nothing of it
__device__ __forceinline__ fd_part fd_take(const uint8_t *in, uint64_t bytes, uint64_t a, uint64_t S0, uint64_t S1)
{ fd_part p = { 0ull, 0ull, 0ull, 0u, 0u, 0u };
  const uint64_t p0 = S0 > 4u * a ? S0 : 4u * a, p1 = S1 < 4u * a + FD_CHUNK ? S1 : 4u * a + FD_CHUNK;
  if (p1 <= p0) return p;
  p.t0 = (uint32_t) (p0 - 4u * a); p.t1 = (uint32_t) (p1 - 4u * a); p.left = (uint32_t) (S1 - p0);      // (a unit has fewer than 2^31 symbols)
  uint64_t w0, w1, w2;
  chunk_words(in, bytes, a, w0, w1, w2);
  uint32_t s = p.t0;
  if (s >= 32u) { w0 = w1; w1 = w2; w2 = 0ull; s -= 32u; }
  if (s)
    { w0 = (w0 << (2u * s)) | (w1 >> (64u - 2u * s));
      w1 = (w1 << (2u * s)) | (w2 >> (64u - 2u * s));
      w2 <<= 2u * s;
    }
  p.w0 = w0; p.w1 = w1; p.w2 = w2;
  return p;
}

// the positions of the part at which query q may begin: [t0, fd_upto)
__device__ __forceinline__ uint32_t fd_upto(const fd_part &p, uint32_t len)
{ if (p.left < len) return p.t0;
  const uint32_t most = p.left - len + 1u;                                     // so many positions from t0 on
  return most < p.t1 - p.t0 ? p.t0 + most : p.t1;
}

// The part's hits over all queries; s_tot (or NULL): the workgroup's word a query, which gets the query's.  FD_BLOCK positions at a
// time: their windows are made once (two funnel shifts each, the shifts constants) and stay in registers while the queries go by,
// a query's matches gathered as bits and counted under the mask of the positions at which it may begin.  A query of at most
// FD_NARROW symbols looks at the upper 32 bits alone.
__device__ __forceinline__ uint32_t fd_count(const fd_part &p, const fd_queries &Q, uint32_t nq, unsigned long long *s_tot)
{ uint32_t c = 0;
  if (p.t1 == p.t0) return 0u;
  uint32_t r0 = (uint32_t) (p.w0 >> 32), r1 = (uint32_t) p.w0, r2 = (uint32_t) (p.w1 >> 32), r3 = (uint32_t) p.w1;
  uint32_t r4 = (uint32_t) (p.w2 >> 32), r5 = (uint32_t) p.w2;
  for (uint32_t b0 = p.t0; b0 < p.t1; b0 += FD_BLOCK)
    { uint32_t hi[FD_BLOCK], lo[FD_BLOCK];
      hi[0] = r0; lo[0] = r1;
      #pragma unroll
      for (uint32_t s = 1; s < FD_BLOCK; s++)
        { hi[s] = (r0 << (2u * s)) | (r1 >> (32u - 2u * s)); lo[s] = (r1 << (2u * s)) | (r2 >> (32u - 2u * s)); }
      const uint32_t here = p.t1 - b0 < FD_BLOCK ? p.t1 - b0 : FD_BLOCK;      // the block's positions that are the part's
      const uint32_t rest = p.left - (b0 - p.t0);                               // symbols from b0 to the unit's end
      for (uint32_t k = 0; k < nq; k++)
        { const fd_query q = Q.q[k];
          uint32_t v = rest >= q.len ? rest - q.len + 1u : 0u;                  // at the first v of them query k may begin
          uint32_t m = 0;                                                       // matches, position s in bit FD_BLOCK - 1 - s
          v = v < here ? v : here;
          if (q.len <= FD_NARROW)
            { const uint32_t code = (uint32_t) (q.code >> 32), mask = (uint32_t) (q.mask >> 32);
              #pragma unroll
              for (uint32_t s = 0; s < FD_BLOCK; s++)
                { const uint32_t d = hi[s] ^ code;
                  m = (m << 1) | ((uint32_t) __popc((d | (d >> 1)) & mask) <= q.mis ? 1u : 0u);
                }
            }
          else                                                 // (bits 2 j and 2 j + 1 stand in one half: d | d >> 1 is taken half by half)
            { const uint32_t c1 = (uint32_t) (q.code >> 32), c0 = (uint32_t) q.code, m1 = (uint32_t) (q.mask >> 32), m0 = (uint32_t) q.mask;
              #pragma unroll
              for (uint32_t s = 0; s < FD_BLOCK; s++)
                { const uint32_t d1 = hi[s] ^ c1, d0 = lo[s] ^ c0;
                  m = (m << 1) | ((uint32_t) (__popc((d1 | (d1 >> 1)) & m1) + __popc((d0 | (d0 >> 1)) & m0)) <= q.mis ? 1u : 0u);
                }
            }
          const uint32_t ck = (uint32_t) __popc(m & ((FD_ALL << FD_BLOCK) >> v) & FD_ALL);
          if (s_tot != NULL && ck) atomicAdd(s_tot + k, (unsigned long long) ck);
          c += ck;
        }
      r0 = (r0 << 16) | (r1 >> 16); r1 = (r1 << 16) | (r2 >> 16); r2 = (r2 << 16) | (r3 >> 16);                  // FD_BLOCK positions up
      r3 = (r3 << 16) | (r4 >> 16); r4 = (r4 << 16) | (r5 >> 16); r5 <<= 16;
    }
  return c;
}

// ... and the same hits written, position by position and query by query, from place `at` of the list on; none at cap or beyond.
// A hit is 16 bytes: record (8), pos (4), query (2), strand (1: 0), mis (1).  pos0: the position of the part's t0 in its unit.
// What comes back is where the next part's hits go.
__device__ __forceinline__ uint64_t fd_list(const fd_part &p, const fd_queries &Q, uint32_t nq, uint64_t unit, uint32_t pos0,
                                            u32x4_u *hits, uint64_t at, uint64_t cap)
{ uint64_t w0 = p.w0, w1 = p.w1, w2 = p.w2;
  for (uint32_t t = p.t0; t < p.t1 && at < cap; t++)
    { for (uint32_t k = 0; k < nq; k++)
        { const fd_query q = Q.q[k];
          if (p.left - (t - p.t0) < q.len) continue;
          const uint64_t d   = w0 ^ q.code;
          const uint32_t mis = (uint32_t) __popcll((d | (d >> 1)) & q.mask);
          if (mis > q.mis) continue;
          if (at < cap)
            { u32x4 h;
              h.x = (uint32_t) unit; h.y = (uint32_t) (unit >> 32); h.z = pos0 + (t - p.t0); h.w = k | (mis << 24);
              hits[at] = h;
            }
          at++;
        }
      w0 = (w0 << 2) | (w1 >> 62); w1 = (w1 << 2) | (w2 >> 62); w2 <<= 2;
    }
  return at;                                               // (the place behind the part's hits, or some place at cap or beyond)
}

// in holds in_bytes bytes and 16 at least; the units are checked against `bound` (as in k_code_counts).
// LIST false: count (n, or NULL) gets every unit's hits, saturated; room (n, or NULL) min(hits, cap); total: nq words the workgroups
//   add to.
// LIST true: room as the first launch left it, start its exclusive sums (n + 1); the hits of every unit that has room go to
//   hits[start[i] ..), none at cap or beyond.
template <bool LIST>
__global__ __launch_bounds__(DX_BLOCK)
void k_find(const uint8_t *__restrict__ in, uint64_t in_bytes, uint64_t bound, const uint64_t *__restrict__ boff,
            const uint32_t *__restrict__ beg, const uint32_t *__restrict__ len, uint64_t n, const fd_queries Q, uint32_t nq,
            uint32_t *__restrict__ count, uint32_t *__restrict__ room, const uint64_t *__restrict__ start,
            u32x4_u *__restrict__ hits, uint64_t cap, unsigned long long *__restrict__ total,
            unsigned long long *__restrict__ bad, uint32_t *__restrict__ ticket)
{ __shared__ unsigned long long s_tot[FD_QMAX];
  if (!LIST)
    { if (threadIdx.x < FD_QMAX) s_tot[threadIdx.x] = 0ull;
      __syncthreads();
    }
  unsigned long long *tot = LIST ? NULL : s_tot;

  const uint32_t lane = (uint32_t) lane_id(), sub = lane % UNITS_GROUP, grp = lane / UNITS_GROUP;
  units_rounds<false>(ticket, ticket_units_of(ticket, FD_BATCH), n, [&](uint64_t u0, uint64_t r1)
    { // unit u0 + lane is this lane's to read and to check
      const uint64_t    i  = u0 + lane;
      const packed_unit pu = packed_unit_take(boff, beg, len, i, r1, bound, bad);
      uint64_t S0 = 0, S1 = 0, a0 = 0, st = 0;             // its symbols in the buffer; its first chunk's place; its first place in the list
      uint32_t nch = 0;                                    // its chunks
      bool     act = pu.ok;                                // it is searched in this launch
      if (pu.ok && pu.len != 0u)
        { S0 = 4u * pu.at + pu.beg; S1 = S0 + pu.len;
          a0 = (S0 >> 2) & ~15ull;
          nch = (uint32_t) ((((S1 - 1u) >> 2) - a0) >> 4) + 1u;
        }
      if (LIST)
        { st  = i < r1 ? start[i] : 0ull;
          act = pu.ok && room[i < r1 ? i : 0u] != 0u && i < r1 && st < cap;
        }
      else if (i < r1 && !pu.ok)
        { if (count != NULL) count[i] = 0u;
          if (room != NULL) room[i] = 0u;
        }

      // no symbol, or up to FD_LANE chunks: the lane's own, chunk after chunk (64 short units a round keep 64 lanes at work)
      if (act && nch <= FD_LANE)
        { uint64_t at = st;
          uint32_t c = 0;
          for (uint32_t j = 0; j < nch; j++)
            { const fd_part p = fd_take(in, in_bytes, a0 + 16u * j, S0, S1);
              if (LIST) at = fd_list(p, Q, nq, i, (uint32_t) (4u * (a0 + 16u * j) + p.t0 - S0), hits, at, cap);
              else      c += fd_count(p, Q, nq, tot);
            }
          if (!LIST)
            { if (count != NULL) count[i] = c;
              if (room != NULL) room[i] = (uint64_t) c < cap ? c : (uint32_t) cap;
            }
        }

      // up to 16 chunks: lanes 16 g .. 16 g + 15 take unit k + g, a chunk each
      units_by_fours(__ballot(act && nch > FD_LANE && nch <= FD_GROUP), [&](int from, bool mine)
        { const uint64_t gS0 = __shfl(S0, from), gS1 = __shfl(S1, from), ga0 = __shfl(a0, from), gst = __shfl(st, from);
          const uint32_t gn  = __shfl(nch, from);
          fd_part p = { 0ull, 0ull, 0ull, 0u, 0u, 0u };
          if (mine && sub < gn) p = fd_take(in, in_bytes, ga0 + 16u * sub, gS0, gS1);
          const uint32_t c = fd_count(p, Q, nq, tot);
          if (LIST)
            { const uint32_t incl = wave_incl_scan(c);
              const uint32_t low  = __shfl(incl, (int) (grp ? UNITS_GROUP * grp - 1u : 0u));           // what the groups below have
              if (c) fd_list(p, Q, nq, u0 + (uint64_t) from, (uint32_t) (4u * (ga0 + 16u * sub) + p.t0 - gS0), hits,
                             gst + (incl - c - (grp ? low : 0u)), cap);
            }
          else
            { const uint32_t all = row_sum(c);
              if (mine && sub == UNITS_GROUP - 1u)
                { if (count != NULL) count[u0 + (uint64_t) from] = all;
                  if (room != NULL) room[u0 + (uint64_t) from] = (uint64_t) all < cap ? all : (uint32_t) cap;
                }
            }
        });

      // the others: the whole wave, 64 chunks a step
      units_each(__ballot(act && nch > FD_GROUP), [&](int from)
        { const uint64_t wS0 = uniform64(__shfl(S0, from)), wS1 = uniform64(__shfl(S1, from)), wa0 = uniform64(__shfl(a0, from));
          const uint32_t wn  = uniform(__shfl(nch, from));
          uint64_t run = uniform64(__shfl(st, from)), mine = 0;           // LIST: the step's first place; else: this lane's hits
          for (uint32_t base = 0; base < wn; base += 64u)
            { const uint32_t j = base + lane;
              const uint64_t a = wa0 + 16ull * j;
              fd_part p = { 0ull, 0ull, 0ull, 0u, 0u, 0u };
              if (j < wn) p = fd_take(in, in_bytes, a, wS0, wS1);
              const uint32_t c = fd_count(p, Q, nq, tot);
              if (LIST)
                { const uint32_t incl = wave_incl_scan(c);
                  if (c) fd_list(p, Q, nq, u0 + (uint64_t) from, (uint32_t) (4u * a + p.t0 - wS0), hits, run + (incl - c), cap);
                  run += wave_total(incl);
                  if (run >= cap) break;
                }
              else mine += c;
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
static_assert(sizeof(dx_hit) == 16 && sizeof(dx_query) == 16, "a hit is one 16-byte store");

extern "C" int dx_code_find(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes,
                            const uint64_t *d_boff, const uint32_t *d_beg, const uint32_t *d_len, uint64_t n,
                            const dx_query *q, uint32_t nq, uint32_t *d_count, dx_hit *d_hits, uint64_t cap,
                            uint64_t total[], uint64_t *hits, uint64_t *bad_unit)
{ if (ctx == NULL) return DX_E_ARG;
  if (bad_unit) *bad_unit = UINT64_MAX;
  if (hits) *hits = 0;
  if (nq < 1u || nq > FD_QMAX) return dx_fail(ctx, DX_E_ARG, "dx_code_find: %u queries (1 to %u)", nq, FD_QMAX);
  if (q == NULL || hits == NULL || (d_hits == NULL && cap)) return dx_fail(ctx, DX_E_ARG, "dx_code_find: NULL pointer");
  if (cap > 0xffffffffull) return dx_fail(ctx, DX_E_ARG, "dx_code_find: a list of more than 2^32 - 1 hits");
  if (total) memset(total, 0, (size_t) nq * 8u);
  fd_queries Q;
  memset(&Q, 0, sizeof(Q));
  for (uint32_t k = 0; k < nq; k++)
    { if (q[k].len < 1u || q[k].len > 32u) return dx_fail(ctx, DX_E_ARG, "dx_code_find: query %u has %u symbols (1 to 32)", k, q[k].len);
      if (q[k].len < 32u && (q[k].code >> (2u * q[k].len)) != 0ull)
        return dx_fail(ctx, DX_E_ARG, "dx_code_find: query %u has bits above its %u symbols", k, q[k].len);
      Q.q[k].code = q[k].code << (64u - 2u * q[k].len);
      Q.q[k].mask = FD_EVEN64 << (64u - 2u * q[k].len);
      Q.q[k].len  = q[k].len; Q.q[k].mis = q[k].max_mis;
    }
  if (n >= (1ull << 31)) return dx_fail(ctx, DX_E_ARG, "dx_code_find: more than 2^31 - 1 units in one batch");
  if (n == 0) return DX_OK;

  // one scratch block: the frame and the nq totals, then (with a list) every unit's first place and its room
  units_frame    f;
  uint64_t       back[UF_OUT + FD_QMAX], *d_start = NULL;
  uint32_t      *d_room = NULL;
  const uint64_t bound = in_bytes;
  int rc = units_list_begin(ctx, "dx_code_find", n, d_boff && d_len && (d_in || !in_bytes), FD_QMAX, 16, cap != 0, &d_in, &in_bytes, &f, &d_start, &d_room);
  if (rc != DX_OK) return rc;
  // (the work of a ticket grows with the queries, so its bytes shrink with them: 100 000 reads of 10 000 symbols and 64 queries are one
  //  read a ticket, 43 ms of work beside 1 ms of draws; 16 reads a ticket left a third of the waves idle for the last quarter)
  const int      grid   = dx_grid_waves(ctx, n, 16);
  const uint32_t target = FD_TARGET / nq > FD_FLOOR ? FD_TARGET / nq : FD_FLOOR;
  hipLaunchKernelGGL(k_ticket_units, dim3(1), dim3(1), 0, ctx->stream, d_boff, d_boff + (n - 1), (const uint32_t *) NULL, n,
                     target, FD_BATCH, f.ticket);
  hipLaunchKernelGGL(k_find<false>, dim3(grid), dim3(DX_BLOCK), 0, ctx->stream, d_in, in_bytes, bound, d_boff, d_beg, d_len, n, Q, nq,
                     d_count, d_room, (const uint64_t *) NULL, (u32x4_u *) NULL, cap, f.out, f.bad, f.ticket);
  if (cap)
    { uint64_t listed = 0;
      if ((rc = units_list_places(ctx, f, d_room, n, d_start, &listed)) != DX_OK) return rc;
      if (listed)
        hipLaunchKernelGGL(k_find<true>, dim3(grid), dim3(DX_BLOCK), 0, ctx->stream, d_in, in_bytes, bound, d_boff, d_beg, d_len, n,
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

// dx_host.h: dx_file_find.c's refusals, worded there
extern "C" int dx_find_fail(dx_ctx *ctx, int code, const char *what)
{ if (ctx == NULL) return code;
  return dx_fail(ctx, code, "dx_file_find: %s", what);
}
