// dx_verify.hip -- dx_verify_ranges: is what a decoder made of an image the text the image was made from?
//
// n units, each a byte range of buffer a (the source text as it lies on the device) and one of buffer b (the decoder's
// output); the answer is the first unit, in unit order, whose ranges differ, the first differing byte in it, and how many
// units differ.  A pure stream: two bytes read per byte compared, nothing written but three words.
//
//   * the waves draw tickets of consecutive units from a counter (next_unit), about 256 KB of text a ticket
//     (k_ticket_units: the device knows the batch's bytes, the host does not);
//   * a unit of VF_LONG bytes and more is the whole wave's: 1 KiB a step (16 bytes a lane, one unaligned 16-byte load
//     from each side), four steps' loads issued before the first is looked at (8 KiB in flight a wave);
//   * shorter units go four at a time, 16 lanes each: 256 bytes a step, two steps in flight;
//   * a unit's last, partial chunk is the 16 bytes that END at its end (they overlap the chunk before: the same bytes
//     compared twice are the same answer); only units under 16 bytes are read byte by byte.  Nothing outside a unit's
//     two ranges is ever touched;
//   * a unit stops at its first difference; per differing unit one atomicMin on unit << 32 | position and one count.
//
// This file stands outside the evidence set of profiles/ (profiles/check.py hashes csrc/*.hip): its kernel has no entry
// in the profiler's name table and is timed with HIP events where a time is wanted (profiles/verify_rate.txt).
#include "units/dx_units.hpp"

#define VF_LONG   2048u                  // units from here on take the whole wave
#define VF_NONE   0xffffffffu
#define VF_TARGET (256u << 10)           // bytes of text a ticket
#define VF_LEAST  4u                     // units a ticket at least (the four sub-waves)

// first differing byte of two chunks (16: none)
__device__ __forceinline__ uint32_t chunk_diff(const u32x4 &x, const u32x4 &y)
{ const uint32_t d0 = x.x ^ y.x, d1 = x.y ^ y.y, d2 = x.z ^ y.z, d3 = x.w ^ y.w;
  if ((d0 | d1 | d2 | d3) == 0u) return 16u;
  if (d0) return (uint32_t) __builtin_ctz(d0) >> 3;
  if (d1) return 4u + ((uint32_t) __builtin_ctz(d1) >> 3);
  if (d2) return 8u + ((uint32_t) __builtin_ctz(d2) >> 3);
  return 12u + ((uint32_t) __builtin_ctz(d3) >> 3);
}

// This lane's chunk of a unit of m common bytes, nominally bytes [pos, pos + 16): where the two sides first differ in it
// (VF_NONE: nowhere, or the chunk lies behind the unit's end).
// (positions in 64 bits on the way: a unit may be close to 4 GiB long; an answer is below m and fits 32)
__device__ __forceinline__ uint32_t lane_diff(const uint8_t *a, const uint8_t *b, uint64_t pos, uint32_t m)
{ if (pos >= m) return VF_NONE;
  if (m - pos < 16u)
    { if (m >= 16u) pos = m - 16u;       // the 16 bytes that end where the unit ends
      else
        { for (uint32_t k = (uint32_t) pos; k < m; k++)
            if (a[k] != b[k]) return k;
          return VF_NONE;
        }
    }
  const u32x4 x = *(const u32x4_u *) (a + pos), y = *(const u32x4_u *) (b + pos);
  const uint32_t d = chunk_diff(x, y);
  return d < 16u ? (uint32_t) pos + d : VF_NONE;
}

__device__ __forceinline__ void report(unsigned long long *res, uint64_t unit, uint32_t pos)
{ atomicMin(res, (unsigned long long) ((unit << 32) | pos));
  atomicAdd(res + 1, 1ull);
}

// res[0]: the smallest unit << 32 | position that differs (preset to all ones), res[1]: differing units.
// skip: units behind a difference already found are not read (the count is then of no use).
__global__ __launch_bounds__(DX_BLOCK)
void k_verify_ranges(const uint8_t *__restrict__ a, const uint64_t *__restrict__ a_off, const uint32_t *__restrict__ a_len,
                     const uint8_t *__restrict__ b, const uint64_t *__restrict__ b_off, const uint32_t *__restrict__ b_len,
                     uint64_t n, int skip, unsigned long long *res, uint32_t *ticket)
{ const int      lane = lane_id(), sub = lane >> 4, sl = lane & 15;
  units_tickets<false>(ticket, ticket_units_of(ticket, VF_LEAST), n, [&](uint64_t t0, uint64_t t1)
    { if (skip && (uniform64(__hip_atomic_load(res, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) >> 32) < t0) return;
      for (uint64_t u0 = t0; u0 < t1; u0 += 4)
        { // four units, one to each 16 lanes
          const uint64_t u  = u0 + (uint64_t) sub;
          const bool     in = u < t1;
          const uint32_t al = in ? a_len[u] : 0u, bl = in ? b_len[u] : 0u, m = al < bl ? al : bl;
          const uint8_t *pa = a + (in ? a_off[u] : 0ull), *pb = b + (in ? b_off[u] : 0ull);
          const bool     small = in && m < VF_LONG;
          uint32_t found = VF_NONE;
          for (uint32_t base = 0; ; base += 512u)
            { const bool act = small && found == VF_NONE && base < m;
              if (!__any(act)) break;
              uint32_t f0 = VF_NONE, f1 = VF_NONE;
              if (act)
                { f0 = lane_diff(pa, pb, base + 16u * sl, m);
                  f1 = lane_diff(pa, pb, base + 256u + 16u * sl, m);
                }
              const uint32_t h0 = (uint32_t) (__ballot(f0 != VF_NONE) >> (16 * sub)) & 0xffffu;
              const uint32_t h1 = (uint32_t) (__ballot(f1 != VF_NONE) >> (16 * sub)) & 0xffffu;
              const uint32_t g0 = __shfl(f0, 16 * sub + (h0 ? __builtin_ctz(h0) : 0));
              const uint32_t g1 = __shfl(f1, 16 * sub + (h1 ? __builtin_ctz(h1) : 0));
              if (h0) found = g0; else if (h1) found = g1;
            }
          if (small && sl == 0 && (found != VF_NONE || al != bl))
            report(res, u, found != VF_NONE ? found : m);

          // the long ones among the four, one after the other, the whole wave each
          uint32_t todo = 0;
          #pragma unroll
          for (int g = 0; g < 4; g++)
            todo |= (uint32_t) (__shfl((int) (in && !small), 16 * g) != 0) << g;
          units_each(uniform(todo), [&](int g)
            { const uint64_t w   = u0 + (uint64_t) g;
              const uint32_t wal = uniform(__shfl(al, 16 * g)), wbl = uniform(__shfl(bl, 16 * g)), wm = wal < wbl ? wal : wbl;
              const uint8_t *wa  = a + uniform64(a_off[w]) + 16u * lane, *wb = b + uniform64(b_off[w]) + 16u * lane;
              uint64_t at = 0;
              uint32_t hit = VF_NONE;
              for (; at + 4u * DX_STEP <= wm && hit == VF_NONE; at += 4u * DX_STEP)
                { u32x4 x[4], y[4];
                  #pragma unroll
                  for (int k = 0; k < 4; k++) x[k] = *(const u32x4_u *) (wa + at + k * DX_STEP);
                  #pragma unroll
                  for (int k = 0; k < 4; k++) y[k] = *(const u32x4_u *) (wb + at + k * DX_STEP);
                  uint32_t any = 0;
                  #pragma unroll
                  for (int k = 0; k < 4; k++)
                    any |= (x[k].x ^ y[k].x) | (x[k].y ^ y[k].y) | (x[k].z ^ y[k].z) | (x[k].w ^ y[k].w);
                  if (__any(any != 0u))
                    {
                      #pragma unroll
                      for (int k = 3; k >= 0; k--)
                        { const uint32_t d = chunk_diff(x[k], y[k]);
                          const unsigned long long h = __ballot(d < 16u);
                          if (h)
                            { const int f = __builtin_ctzll(h);
                              hit = (uint32_t) at + k * DX_STEP + 16u * f + (uint32_t) __shfl((int) d, f);
                            }
                        }
                    }
                }
              for (; at < wm && hit == VF_NONE; at += DX_STEP)
                { const uint32_t f = lane_diff(wa - 16u * lane, wb - 16u * lane, at + 16u * lane, wm);
                  const unsigned long long h = __ballot(f != VF_NONE);
                  if (h) hit = (uint32_t) __shfl((int) f, __builtin_ctzll(h));
                }
              hit = uniform(hit);
              if (lane == 0 && (hit != VF_NONE || wal != wbl))
                report(res, w, hit != VF_NONE ? hit : wm);
            });
        }
    });
}

static_assert(DXW_COUNT == 64, "dx_ctx.hip allocates 64 words of d_u64");

// one launch over units [0, n), 0 < n < 2^31; first: unit << 32 | position, or all ones
static int verify_launch(dx_ctx *ctx, const uint8_t *d_a, const uint64_t *d_a_off, const uint32_t *d_a_len,
                         const uint8_t *d_b, const uint64_t *d_b_off, const uint32_t *d_b_len, uint64_t n, int skip,
                         uint64_t *first, uint64_t *differ)
{ units_frame f;
  uint64_t    back[UF_OUT + 2];
  int rc = units_begin(ctx, "dx_verify_ranges", n, d_a && d_a_off && d_a_len && d_b && d_b_off && d_b_len,
                       ctx->d_u64 + DXW_UNITS, 2, 0, NULL, NULL, &f);
  if (rc != DX_OK) return rc;
  DX_HIP(ctx, hipMemsetAsync(f.out, 0xff, 8, ctx->stream));
  hipLaunchKernelGGL(k_ticket_units, dim3(1), dim3(1), 0, ctx->stream, d_a_off, d_a_off + (n - 1), d_a_len + (n - 1), n,
                     VF_TARGET, VF_LEAST, f.ticket);
  hipLaunchKernelGGL(k_verify_ranges, dim3(dx_grid_waves(ctx, (n + VF_LEAST - 1) / VF_LEAST, 16)), dim3(DX_BLOCK), 0, ctx->stream,
                     d_a, d_a_off, d_a_len, d_b, d_b_off, d_b_len, n, skip, f.out, f.ticket);
  if ((rc = units_end(ctx, f, back, NULL, NULL, 0)) != DX_OK) return rc;   // (no unit is refused: nothing words one)
  *first = back[UF_OUT]; *differ = back[UF_OUT + 1];
  return DX_OK;
}

extern "C" int dx_verify_ranges(dx_ctx *ctx, const uint8_t *d_a, const uint64_t *d_a_off, const uint32_t *d_a_len,
                                const uint8_t *d_b, const uint64_t *d_b_off, const uint32_t *d_b_len, uint64_t n,
                                uint64_t *first_unit, uint32_t *first_pos, uint64_t *n_differ)
{ if (ctx == NULL) return DX_E_ARG;
  if (first_unit == NULL || first_pos == NULL)
    return dx_fail(ctx, DX_E_ARG, "dx_verify_ranges: nowhere to put the answer");
  *first_unit = UINT64_MAX; *first_pos = 0;
  if (n_differ) *n_differ = 0;
  const uint64_t piece = (1ull << 31) - 1u;                // (the key holds 32 bits of unit index; a launch takes fewer than 2^31 units)
  for (uint64_t at = 0; at < n; at += piece)
    { const uint64_t m = n - at < piece ? n - at : piece;
      uint64_t first = 0, differ = 0;
      const int rc = verify_launch(ctx, d_a, d_a_off + at, d_a_len + at, d_b, d_b_off + at, d_b_len + at, m, n_differ == NULL, &first, &differ);
      if (rc != DX_OK) return rc;
      if (n_differ) *n_differ += differ;
      if (first != UINT64_MAX && *first_unit == UINT64_MAX)
        { *first_unit = at + (first >> 32); *first_pos = (uint32_t) first;
          if (n_differ == NULL) break;                     // (nobody counts: what lies behind need not be read)
        }
    }
  return DX_OK;
}
