// dx_find_span.hip -- where the occurrences dx_code_find_edit found BEGIN.
//
//   dx_code_hit_starts   per hit of a list as dx_code_find_edit leaves it: the start of the occurrence that ends at the hit's pos   (k_hit_starts)
//
// dx_code_find_edit reports an occurrence by its exclusive end e and its distance d = D(e) = min over s of Levenshtein(P, U[s, e)), and
// says of the start only that it lies in [e - m - d, e - m + d].  Here, for a hit (unit j, e, query P of m symbols, d):
//     start = the LARGEST s, 0 <= s <= e, with Levenshtein(P, U_j[s, e)) == d
// -- the shortest stretch of the unit that ends at e and lies d edits from the pattern.  Such an s exists (D(e) is the minimum over s) and
// |(e - s) - m| <= d, so at most m + d <= 127 symbols in front of e matter, and never one in front of the unit's first.
//
// The distance is the same bit-vector recurrence (find/dx_find_edit.hip: Myers 1999 in Hyyro's formulation, the query at the word's TOP,
// the bits below it kept neutral) with two changes: the query is REVERSED (fe_queries_make: symbol i in bit 63 - i, so the pattern's last
// symbol is the column's first row), and a carry of 1 goes into the horizontal deltas, Ph = (Ph << 1) | one with `one` the query's lowest
// bit: the start is anchored at e and not free, row 0 of the matrix is 0, 1, 2 ...  The scan steps BACKWARDS from symbol e - 1, the score
// begins at m, and after t steps it is Levenshtein(P, U[e - t, e)); it stops at the first t where that equals d: start = e - t.  The
// first such t is the smallest, so the s is the largest.  A scan that reaches min(e, m + d) steps without meeting d says the hit is not
// one of this data.
//
// One lane a hit: the list is short beside the reads and a lane's work is at most 127 symbol steps of some 30 (32-bit instance, m <= 32)
// or 50 (64-bit) vector instructions (fe_scan's counts for the same column; this loop's were not counted).  The hit's query differs
// from lane to lane, so the planes are read from the kernel argument with a lane's index (vector loads from the constant segment, once
// a hit), and a wave whose hits have queries of both sizes runs both instances.
// The packed bytes are read backwards, 8 at a time, from any byte offset and phase: the 8 bytes that END at the symbol's byte, and when
// those would begin in front of the buffer its first 8 moved down (hs_be64_back, the mirror of be64_at): nothing outside [0, in_bytes)
// is read.  Hit i writes start[i] and nothing else; the smallest index of a bad hit is kept by an atomicMin as the units' kernels keep
// their bad unit's (units/dx_units.hpp), read back once a call.
//
// This file stands outside the evidence set of profiles/ (profiles/check.py hashes csrc/*.hip), like its neighbours in find/; its kernel
// is timed with events on the context's stream (tools/find_span_rate.py).
#include "units/dx_units.hpp"
#include "find/dx_find_edit.hpp"

extern "C" {
#include "dx_host.h"
}

// the 8 bytes that end with byte o of the buffer (o < bytes, bytes >= 8) as a word in the read's bit order: byte o at the bottom; the 8
// bytes that would begin in front of the buffer are its first 8, moved down (zeros on top)
__device__ __forceinline__ uint64_t hs_be64_back(const uint8_t *in, uint64_t o)
{ if (o >= 7u) return __builtin_bswap64(*(const u64_u *) (in + (o - 7u)));
  return __builtin_bswap64(*(const u64_u *) in) >> (8u * (7u - (uint32_t) o));
}

// the start of the occurrence of q that ends at end e (1 <= e <= the unit's symbols) with distance d, in the unit whose first symbol is
// symbol U0 of the buffer; UINT32_MAX when no stretch that ends at e lies d from the query
template <typename W>
__device__ __forceinline__ uint32_t hs_scan(const uint8_t *in, uint64_t U0, uint32_t e, const fe_query &q, uint32_t d)
{ constexpr uint32_t WB = 8u * sizeof(W);                                        // (the 32-bit instance takes the planes' upper halves)
  const uint32_t m = q.len, reach = m + d, steps = e < reach ? e : reach;
  const W        b0 = (W) (q.b0 >> (64u - WB)), b1 = (W) (q.b1 >> (64u - WB)), low = (W) (q.low >> (64u - WB));
  const W        one = (W) 1 << (WB - m);                                        // the query's lowest bit: where row 0's delta comes in
  W        Pv = ~(W) 0, Mv = (W) 0;
  uint32_t score = m;

  const uint64_t A = U0 + e - 1u;                                                // symbol e - 1 of the unit in the buffer
  uint64_t o = A >> 2;                                                           // ... its byte
  uint64_t w = hs_be64_back(in, o) >> (2u * (3u - (uint32_t) (A & 3u)));         // ... and the symbol in the word's two lowest bits
  uint32_t have = 29u + (uint32_t) (A & 3u);                                     // symbols left in w
  for (uint32_t t = 1; t <= steps; t++)
    { if (have == 0u) { o -= 8u; w = hs_be64_back(in, o); have = 32u; }         // (a symbol of the unit is wanted there: o >= 8)
      const uint32_t c = (uint32_t) w & 3u;
      const W B0 = (W) 0 - (W) (c & 1u), B1 = (W) 0 - (W) (c >> 1);              // its two bits, each all over a word
      w >>= 2; have--;
      const W Eq = ~(((b0 ^ B0) | low) | (b1 ^ B1));
      const W Xv = Eq | Mv;
      const W Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
      W Ph = Mv | ~(Xh | Pv);
      W Mh = Pv & Xh;
      score += (uint32_t) (Ph >> (WB - 1u));
      score -= (uint32_t) (Mh >> (WB - 1u));
      Ph = (Ph << 1) | one; Mh <<= 1;                                            // (anchored at e: a 1 comes in)
      Pv = Mh | ~(Xv | Ph);
      Mv = Ph & Xv;
      if (score == d) return e - t;
    }
  return UINT32_MAX;
}

// in holds in_bytes bytes and 8 at least; the units are checked against `bound`.  start[i] for every i < n_hits; *bad gets the smallest
// index of a bad hit.
__global__ __launch_bounds__(DX_BLOCK)
void k_hit_starts(const uint8_t *__restrict__ in, uint64_t bound, const uint64_t *__restrict__ boff, const uint32_t *__restrict__ beg,
                  const uint32_t *__restrict__ len, uint64_t n, const fe_queries Q, uint32_t nq,
                  const u32x4_u *__restrict__ hits, uint64_t n_hits, uint32_t *__restrict__ start, unsigned long long *__restrict__ bad)
{ const uint64_t i = (uint64_t) blockIdx.x * DX_BLOCK + threadIdx.x;
  if (i >= n_hits) return;
  const u32x4    h = hits[i];                                                    // record (x, y), pos (z), query | strand << 16 | mis << 24 (w)
  const uint64_t j = (uint64_t) h.x | ((uint64_t) h.y << 32);
  const uint32_t e = h.z, k = h.w & 0xffffu, d = h.w >> 24;
  uint32_t s = UINT32_MAX;
  if (j < n && k < nq)
    { const uint64_t at = boff[j];
      const uint32_t b = beg != NULL ? beg[j] : 0u, L = len[j];
      const fe_query q = Q.q[k];
      if (packed_unit_ok(at, b, L, bound) && e >= 1u && e <= L && d <= q.err)
        s = q.len <= 32u ? hs_scan<uint32_t>(in, 4u * at + b, e, q, d) : hs_scan<uint64_t>(in, 4u * at + b, e, q, d);
    }
  start[i] = s;
  if (s == UINT32_MAX) atomicMin(bad, (unsigned long long) i);
}

// ---------------------------------------------------------------------------------------------
//  the entry point
// ---------------------------------------------------------------------------------------------
static_assert(sizeof(dx_hit) == 16, "a hit is one 16-byte load");

extern "C" int dx_code_hit_starts(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes,
                                  const uint64_t *d_boff, const uint32_t *d_beg, const uint32_t *d_len, uint64_t n,
                                  const dx_equery *q, uint32_t nq, const dx_hit *d_hits, uint64_t n_hits, uint32_t *d_start,
                                  uint64_t *bad_hit)
{ if (ctx == NULL) return DX_E_ARG;
  if (bad_hit) *bad_hit = UINT64_MAX;
  fe_queries Q;
  int rc = fe_queries_make(ctx, "dx_code_hit_starts", q, nq, true, &Q);
  if (rc != DX_OK) return rc;
  if (n >= (1ull << 31)) return dx_fail(ctx, DX_E_ARG, "dx_code_hit_starts: more than 2^31 - 1 units in one batch");
  if (n_hits >= (1ull << 32)) return dx_fail(ctx, DX_E_ARG, "dx_code_hit_starts: a list of more than 2^32 - 1 hits");
  if (n_hits == 0) return DX_OK;
  units_frame    f;
  uint64_t       back[UF_OUT];
  const uint64_t bound = in_bytes;                         // (the kernel loads 8 bytes at a time: fewer are copied, zeros behind them)
  rc = units_begin(ctx, "dx_code_hit_starts", n, d_hits && d_start && ((d_boff && d_len) || !n) && (d_in || !in_bytes),
                   ctx->d_u64 + DXW_UNITS, 0, 8, &d_in, &in_bytes, &f);
  if (rc != DX_OK) return rc;
  const uint32_t grid = (uint32_t) ((n_hits + DX_BLOCK - 1u) / DX_BLOCK);
  hipLaunchKernelGGL(k_hit_starts, dim3(grid), dim3(DX_BLOCK), 0, ctx->stream, d_in, bound, d_boff, d_beg, d_len, n, Q, nq,
                     (const u32x4_u *) d_hits, n_hits, d_start, f.bad);
  return units_end(ctx, f, back, bad_hit,
                   "%s: hit %llu is none of these units and queries (its unit inside the %llu packed bytes, 1 <= pos <= its symbols, mis within the query's bound and met by a stretch that ends at pos)",
                   bound);
}

// dx_host.h: dx_file_cut.c's refusals, worded there
extern "C" int dx_cut_fail(dx_ctx *ctx, int code, const char *what)
{ if (ctx == NULL) return code;
  return dx_fail(ctx, code, "dx_file_cut: %s", what);
}
