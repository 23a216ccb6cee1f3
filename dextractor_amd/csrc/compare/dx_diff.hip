// dx_diff.hip -- how two buffers that should hold the same things differ, counted where they lie.
//
//   dx_diff_ranges  per unit a byte range of buffer a against one of the same length of buffer b            (k_diff<false>)
//   dx_code_diff    per unit the first d_len[j] symbols of a packed read of a against those of one of b     (k_diff<true>)
//
// dx_verify_ranges (verify/) answers "is there a difference, and where is the first"; it stops there, and dx_file_verify
// wants no more.  This file COUNTS: per unit the differing bytes (symbols) and the first of them, per kind of unit the
// differing bytes, the units that have one, the sum and the largest of |a - b|; and the first difference of the call.  Both
// sides are read once, nothing is written but two words a unit and the tallies: the roofline is HBM, what is read.
//
// One kernel body, two instances; only what a 16-byte chunk contributes differs between them (df_word).
//   * the waves draw tickets of consecutive units (k_ticket_units: about DF_TARGET bytes of side a ticket) and take a
//     ticket's units 64 a round, a lane reading one unit's parameters and checking its bounds (range_ok / packed_unit_ok);
//   * a unit of fewer than 16 bytes is its lane's, byte by byte;
//   * one below DF_LONG bytes goes FOUR A STEP, 16 lanes each, 256 bytes of either side a step;
//   * the others take the whole wave, 1 KiB of either side a step, the next step's bytes asked for before this step's are
//     counted.
// A unit's last, partial chunk is the 16 bytes that END at its end (dx_verify.hip's rule).  They overlap the chunk before,
// and a count must not see a byte twice: the bytes in front of the chunk's nominal place are cleared on both sides, so they
// are equal and add nothing.  A lane whose nominal place lies behind the unit asks for those same last 16 bytes and counts
// none of them.  Nothing outside a unit's two ranges is ever read, so no buffer needs padding.
// Packed codes (DB.c:319-338): symbol i of a read stands in byte i >> 2 at bits 7 - 2 (i & 3), 6 - 2 (i & 3), so a unit of
// len symbols is (len + 3) >> 2 bytes of which the last holds len & 3 symbols (0: four).  The bits behind them are pad: a
// foreign writer may leave anything there, and they are cleared on both sides like the bytes above.  Two symbols differ
// when either of their bits does: (d | d >> 1) on the even bits, one popcount a word.
// Side a's bytes are ANDed with the unit's kind's mask first (dx_diff_ranges: a_and): dexqv -l's rounding is 0xFE on the
// insertion line and 0xFC on the merge line (QV.c:1406-1415), so "b is what -l keeps of a" is a comparison with two masks.
//
// Tallies: a unit's leader adds its figures to the workgroup's words in LDS (only a unit that differs costs anything), the
// workgroup adds them to the global words at the kernel's end.
//
// This file stands outside the evidence set of profiles/ (profiles/check.py hashes csrc/*.hip); its kernels have no entry in
// the profiler's name table and are timed with synchronised host clocks (tools/compare_rate.py).
#include "units/dx_units.hpp"

extern "C" {
#include "dx_host.h"
}

#define DF_LONG    2048u                   // bytes: units from here on take the whole wave
#define DF_SHORT   16u                     // bytes: units below go byte by byte (a chunk is 16 bytes)
#define DF_LEAST   4u                      // units a ticket at least
#define DF_TARGET  (256u << 10)            // bytes of side a ticket
#define DF_KINDS   8
#define DF_NONE    0xffffffffu
#define DF_TALLY   4u                      // words a kind: differ, units, sum_abs, max_abs (dx_diff_tally)

struct df_acc { uint32_t differ, first, most; uint64_t sum; };

// One word of either side (x: side a, masked), whose byte 0 is byte `at` of the unit.
template <bool CODES>
__device__ __forceinline__ void df_word(df_acc &c, uint32_t x, uint32_t y, uint32_t at)
{ const uint32_t d = x ^ y;
  if (d == 0u) return;
  if (CODES)
    { const uint32_t e  = (d | (d >> 1)) & 0x55555555u;                      // a symbol differs: its even bit
      const uint32_t k  = (uint32_t) __builtin_ctz(e) >> 3;                   // the first byte that has one,
      const uint32_t eb = (e >> (8u * k)) & 0xffu;                           // ... and in it the pair nearest the top
      c.differ += (uint32_t) __popc(e);
      c.first   = min(c.first, 4u * (at + k) + 3u - ((31u - (uint32_t) __builtin_clz(eb)) >> 1));
    }
  else
    { const uint32_t nz = (((d & 0x7f7f7f7fu) + 0x7f7f7f7fu) | d) & 0x80808080u;      // a byte differs: its top bit
      c.differ += (uint32_t) __popc(nz);
      c.first   = min(c.first, at + ((uint32_t) __builtin_ctz(nz) >> 3));
      c.sum    += __builtin_amdgcn_sad_u8(x, y, 0u);
      #pragma unroll
      for (uint32_t k = 0; k < 4u; k++)
        c.most = max(c.most, __builtin_amdgcn_sad_u8(x & (0xffu << (8u * k)), y & (0xffu << (8u * k)), 0u));
    }
}

// bytes [lo, 4) of a word kept (lo <= 0: all, lo >= 4: none)
__device__ __forceinline__ uint32_t df_keep(int lo)
{ return lo <= 0 ? 0xffffffffu : (lo >= 4 ? 0u : 0xffffffffu << (8 * lo)); }

// The 16 bytes of both sides that begin at byte `from` of a unit of m bytes; those from byte lo of them on count.  and4: the
// kind's mask in all four bytes; pad: the bits of the unit's last byte that hold no symbol (CODES; 0: none).
template <bool CODES>
__device__ __forceinline__ void df_chunk(df_acc &c, u32x4 x, u32x4 y, uint32_t from, uint32_t lo, uint32_t m, uint32_t and4, uint32_t pad)
{ if (!CODES) { x.x &= and4; x.y &= and4; x.z &= and4; x.w &= and4; }
  if (lo)
    { const uint32_t k0 = df_keep((int) lo), k1 = df_keep((int) lo - 4), k2 = df_keep((int) lo - 8), k3 = df_keep((int) lo - 12);
      x.x &= k0; x.y &= k1; x.z &= k2; x.w &= k3;
      y.x &= k0; y.y &= k1; y.z &= k2; y.w &= k3;
    }
  if (CODES && pad && from + 16u == m)                     // (the unit's last byte is this chunk's)
    { x.w &= ~(pad << 24); y.w &= ~(pad << 24); }
  df_word<CODES>(c, x.x, y.x, from);
  df_word<CODES>(c, x.y, y.y, from + 4u);
  df_word<CODES>(c, x.z, y.z, from + 8u);
  df_word<CODES>(c, x.w, y.w, from + 12u);
}

// where a lane whose nominal place is byte pos of a unit of m >= 16 bytes loads from: there, or the unit's last 16 bytes when
// fewer are left (or none: asked for, never counted)
__device__ __forceinline__ uint32_t df_from(uint64_t pos, uint32_t m)
{ return pos + 16u <= (uint64_t) m ? (uint32_t) pos : m - 16u; }

// ... and what that lane counts of it
template <bool CODES>
__device__ __forceinline__ void df_lane(df_acc &c, const uint8_t *pa, const uint8_t *pb, uint64_t pos, uint32_t m, uint32_t and4, uint32_t pad)
{ if (pos >= (uint64_t) m) return;
  const uint32_t from = df_from(pos, m);
  df_chunk<CODES>(c, *(const u32x4_u *) (pa + from), *(const u32x4_u *) (pb + from), from, (uint32_t) pos - from, m, and4, pad);
}

// the figures of W lanes side by side, in all of them
template <int W>
__device__ __forceinline__ void df_join(df_acc &c)
{
  #pragma unroll
  for (int d = W / 2; d > 0; d >>= 1)
    { c.differ += (uint32_t) __shfl_xor((int) c.differ, d);
      c.first   = min(c.first, (uint32_t) __shfl_xor((int) c.first, d));
      c.most    = max(c.most, (uint32_t) __shfl_xor((int) c.most, d));
      c.sum    += (uint64_t) __shfl_xor((unsigned long long) c.sum, d);
    }
}

// a unit is done: its two words, and when it differs its share of the workgroup's tallies and of the call's first difference
__device__ __forceinline__ void df_done(const df_acc &c, uint64_t unit, uint32_t kind, uint32_t *differ, uint32_t *first,
                                        unsigned long long *s_tot, unsigned long long *out)
{ if (differ != NULL) differ[unit] = c.differ;
  if (first != NULL) first[unit] = c.first;
  if (c.differ == 0u) return;
  unsigned long long *t = s_tot + DF_TALLY * kind;
  atomicAdd(t, (unsigned long long) c.differ);
  atomicAdd(t + 1, 1ull);
  if (c.sum) atomicAdd(t + 2, (unsigned long long) c.sum);
  if (c.most) atomicMax(t + 3, (unsigned long long) c.most);
  atomicMin(out, (unsigned long long) ((unit << 32) | c.first));
}

// Unit j: a[a_off[j] ..) against b[b_off[j] ..), len[j] bytes -- CODES: symbols, (len[j] + 3) >> 2 bytes -- of each.
// kind: n, or NULL (all 0); and8: the kinds' masks, kind k's in byte k.  differ, first: n each, or NULL.
// out[0]: the smallest unit << 32 | place that differs (preset to all ones); out[1 + 4 k ..]: kind k's tally.
// bad: the smallest index of a unit that is refused (preset to all ones).
template <bool CODES>
__global__ __launch_bounds__(DX_BLOCK)
void k_diff(const uint8_t *__restrict__ a, uint64_t a_bytes, const uint64_t *__restrict__ a_off,
            const uint8_t *__restrict__ b, uint64_t b_bytes, const uint64_t *__restrict__ b_off,
            const uint32_t *__restrict__ len, const uint8_t *__restrict__ kind, uint32_t nkinds, uint64_t and8, uint64_t n,
            uint32_t *__restrict__ differ, uint32_t *__restrict__ first, unsigned long long *__restrict__ out,
            unsigned long long *__restrict__ bad, uint32_t *__restrict__ ticket)
{ __shared__ unsigned long long s_tot[DF_TALLY * DF_KINDS];
  if (threadIdx.x < DF_TALLY * DF_KINDS) s_tot[threadIdx.x] = 0ull;
  __syncthreads();

  const uint32_t lane = (uint32_t) lane_id(), sub = lane % UNITS_GROUP;
  units_rounds<false>(ticket, ticket_units_of(ticket, DF_LEAST), n, [&](uint64_t u0, uint64_t r1)
    { // unit u0 + lane is this lane's to read and to check
      const uint64_t i = u0 + lane;
      uint64_t ao = 0, bo = 0;
      uint32_t m = 0, kd = 0, pad = 0, and4 = 0xffffffffu;
      int      how = 0;                                    // 1: this lane's, 2: 16 lanes', 3: the wave's
      if (i < r1)
        { const uint32_t ln = len[i];
          ao = a_off[i]; bo = b_off[i];
          kd = kind != NULL ? kind[i] : 0u;
          const bool ok = CODES ? packed_unit_ok(ao, 0u, ln, a_bytes) && packed_unit_ok(bo, 0u, ln, b_bytes)
                                : range_ok(ao, ln, a_bytes) && range_ok(bo, ln, b_bytes) && kd < nkinds;
          if (ok)
            { m    = CODES ? (uint32_t) (((uint64_t) ln + 3u) >> 2) : ln;
              pad  = CODES && (ln & 3u) ? (1u << (8u - 2u * (ln & 3u))) - 1u : 0u;
              and4 = CODES ? 0xffffffffu : 0x01010101u * (uint32_t) ((and8 >> (8u * kd)) & 0xffu);
              how  = m < DF_SHORT ? 1 : (m < DF_LONG ? 2 : 3);
            }
          else atomicMin(bad, (unsigned long long) i);
        }

      // fewer than 16 bytes: the lane's own, byte by byte
      if (how == 1)
        { df_acc c = { 0u, DF_NONE, 0u, 0ull };
          for (uint32_t k = 0; k < m; k++)
            { uint32_t x = a[ao + k] & and4 & 0xffu, y = b[bo + k];
              if (CODES && k + 1u == m) { x &= ~pad; y &= ~pad; }
              df_word<CODES>(c, x, y, k);
            }
          df_done(c, i, kd, differ, first, s_tot, out);
        }

      // below DF_LONG: lanes 16 g .. 16 g + 15 take unit k + g, 256 bytes of either side a step
      units_by_fours(__ballot(how == 2), [&](int from, bool mine)
        { const uint8_t *pa = a + __shfl(ao, from), *pb = b + __shfl(bo, from);
          const uint32_t gm = __shfl(m, from), gand = __shfl(and4, from), gpad = __shfl(pad, from), gk = __shfl(kd, from);
          df_acc c = { 0u, DF_NONE, 0u, 0ull };
          if (mine)
            for (uint32_t base = 0; base < gm; base += 16u * UNITS_GROUP)
              df_lane<CODES>(c, pa, pb, (uint64_t) base + 16u * sub, gm, gand, gpad);
          df_join<(int) UNITS_GROUP>(c);
          if (mine && sub == 0u) df_done(c, u0 + (uint64_t) from, gk, differ, first, s_tot, out);
        });

      // the others: the whole wave, 1 KiB of either side a step.  A step's bytes are asked for a step before they are counted
      // (behind the unit's end df_from gives its last 16 bytes: asked for, never counted).
      units_each(__ballot(how == 3), [&](int from)
        { const uint8_t *pa = a + uniform64(__shfl(ao, from)), *pb = b + uniform64(__shfl(bo, from));
          const uint32_t wm = uniform(__shfl(m, from)), wand = uniform(__shfl(and4, from)), wpad = uniform(__shfl(pad, from));
          const uint32_t wk = uniform(__shfl(kd, from));
          df_acc c = { 0u, DF_NONE, 0u, 0ull };
          uint32_t at = df_from(16u * lane, wm);
          u32x4 x = *(const u32x4_u *) (pa + at), y = *(const u32x4_u *) (pb + at);
          for (uint64_t base = 0; base < (uint64_t) wm; base += DX_STEP)
            { const uint64_t pos = base + 16u * lane;
              const uint32_t nxt = df_from(pos + DX_STEP, wm);
              const u32x4 xn = *(const u32x4_u *) (pa + nxt), yn = *(const u32x4_u *) (pb + nxt);
              if (pos < (uint64_t) wm) df_chunk<CODES>(c, x, y, at, (uint32_t) pos - at, wm, wand, wpad);
              x = xn; y = yn; at = nxt;
            }
          df_join<64>(c);
          if (lane == 0u) df_done(c, u0 + (uint64_t) from, wk, differ, first, s_tot, out);
        });
    });

  __syncthreads();
  if (threadIdx.x < DF_TALLY * nkinds && s_tot[threadIdx.x] != 0ull)
    { if ((threadIdx.x & (DF_TALLY - 1u)) == 3u) atomicMax(out + 1u + threadIdx.x, s_tot[threadIdx.x]);
      else                                       atomicAdd(out + 1u + threadIdx.x, s_tot[threadIdx.x]);
    }
}

// ---------------------------------------------------------------------------------------------
//  the entry points
// ---------------------------------------------------------------------------------------------
static_assert(sizeof(dx_diff_tally) == DF_TALLY * 8u, "a tally is four words of the answer");

// one launch over n > 0 units; tally: nkinds of them, or NULL; *first: unit << 32 | place, or all ones
template <bool CODES>
static int diff_launch(dx_ctx *ctx, const char *who, const uint8_t *d_a, uint64_t a_bytes, const uint64_t *d_a_off,
                       const uint8_t *d_b, uint64_t b_bytes, const uint64_t *d_b_off, const uint32_t *d_len, const uint8_t *d_kind,
                       int nkinds, const uint8_t *a_and, uint64_t n, uint32_t *d_differ, uint32_t *d_first,
                       dx_diff_tally *tally, uint64_t *first, uint64_t *bad_unit)
{ units_frame f;
  uint64_t    back[UF_OUT + 1 + DF_TALLY * DF_KINDS], and8 = UINT64_MAX;
  const size_t words = 1u + DF_TALLY * (size_t) nkinds;     // (more than the context's frame holds: the frame heads a scratch block)
  int rc = units_begin(ctx, who, n, d_a_off && d_b_off && d_len && (d_a || !a_bytes) && (d_b || !b_bytes), NULL, words, 0, NULL, NULL, &f);
  if (rc != DX_OK) return rc;
  if (a_and != NULL)
    for (int k = 0; k < nkinds; k++) and8 = (and8 & ~(0xffull << (8 * k))) | ((uint64_t) a_and[k] << (8 * k));
  DX_HIP(ctx, hipMemsetAsync(f.out, 0xff, 8, ctx->stream));
  // (units a ticket from the extent of side a's offsets: units that do not stand in the buffer's order give a figure that means
  //  nothing, and the bounds of ticket_units_of hold)
  hipLaunchKernelGGL(k_ticket_units, dim3(1), dim3(1), 0, ctx->stream, d_a_off, d_a_off + (n - 1), d_len + (n - 1), n,
                     DF_TARGET, DF_LEAST, f.ticket);
  hipLaunchKernelGGL(k_diff<CODES>, dim3(dx_grid_waves(ctx, (n + DF_LEAST - 1) / DF_LEAST, 16)), dim3(DX_BLOCK), 0, ctx->stream,
                     d_a, a_bytes, d_a_off, d_b, b_bytes, d_b_off, d_len, d_kind, (uint32_t) nkinds, and8, n, d_differ, d_first,
                     f.out, f.bad, f.ticket);
  rc = units_end(ctx, f, back, bad_unit, CODES ? "%s: unit %llu does not lie inside the packed bytes of both sides (a: %llu)"
                                               : "%s: range %llu does not lie inside both buffers (a: %llu bytes), or its kind is not below %d",
                 a_bytes, nkinds);
  if (rc != DX_OK) return rc;
  if (first) *first = back[UF_OUT];
  if (tally) memcpy(tally, back + UF_OUT + 1, (size_t) nkinds * sizeof(*tally));
  return DX_OK;
}

extern "C" int dx_diff_ranges(dx_ctx *ctx, const uint8_t *d_a, uint64_t a_bytes, const uint64_t *d_a_off,
                              const uint8_t *d_b, uint64_t b_bytes, const uint64_t *d_b_off, const uint32_t *d_len,
                              const uint8_t *d_kind, int nkinds, const uint8_t *a_and, uint64_t n,
                              uint32_t *d_differ, uint32_t *d_first, dx_diff_tally *tally, uint64_t *first, uint64_t *bad_unit)
{ if (ctx == NULL) return DX_E_ARG;
  if (bad_unit) *bad_unit = UINT64_MAX;
  if (first) *first = UINT64_MAX;
  if (nkinds < 1 || nkinds > DF_KINDS)
    return dx_fail(ctx, DX_E_ARG, "dx_diff_ranges: %d kinds (1 to %d)", nkinds, DF_KINDS);
  if (tally) memset(tally, 0, (size_t) nkinds * sizeof(*tally));
  if (n == 0) return DX_OK;
  return diff_launch<false>(ctx, "dx_diff_ranges", d_a, a_bytes, d_a_off, d_b, b_bytes, d_b_off, d_len, d_kind, nkinds, a_and, n,
                            d_differ, d_first, tally, first, bad_unit);
}

extern "C" int dx_code_diff(dx_ctx *ctx, const uint8_t *d_a, uint64_t a_bytes, const uint64_t *d_a_boff,
                            const uint8_t *d_b, uint64_t b_bytes, const uint64_t *d_b_boff, const uint32_t *d_len, uint64_t n,
                            uint32_t *d_differ, uint32_t *d_first, uint64_t total[2], uint64_t *first, uint64_t *bad_unit)
{ if (ctx == NULL) return DX_E_ARG;
  if (bad_unit) *bad_unit = UINT64_MAX;
  if (first) *first = UINT64_MAX;
  if (total) total[0] = total[1] = 0;
  if (n == 0) return DX_OK;
  dx_diff_tally t;
  const int rc = diff_launch<true>(ctx, "dx_code_diff", d_a, a_bytes, d_a_boff, d_b, b_bytes, d_b_boff, d_len, NULL, 1, NULL, n,
                                   d_differ, d_first, &t, first, bad_unit);
  if (rc == DX_OK && total) { total[0] = t.differ; total[1] = t.units; }
  return rc;
}

// dx_host.h: the context's error text gets a side's letter in front ("a: ..."); side 0 empties the text, so that a host
// walk, which fails without words, is told from a device call, which has them
extern "C" int dx_side_fail(dx_ctx *ctx, int code, int side)
{ char was[480];
  if (ctx == NULL) return code;
  if (side == 0) { ctx->err[0] = '\0'; return code; }
  snprintf(was, sizeof(was), "%s", ctx->err);
  if (was[0] == '\0') snprintf(was, sizeof(was), "the image does not parse (error %d)", code);
  return dx_fail(ctx, code, "%c: %s", side, was);
}
