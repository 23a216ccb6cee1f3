// dx_crc.hip -- CRC-32 (zlib / gzip / PNG: polynomial 0xEDB88320 reflected, initial value and final xor 0xFFFFFFFF) of byte
// ranges of a device buffer, and of their concatenation from the ranges' CRCs and lengths alone.
//
//   dx_crc32_ranges   n units, each a byte range of one buffer -> n CRCs              (k_crc_ranges, k_crc_huge)
//   dx_crc32_fold     the CRC and length of the units' concatenation in index order   (k_crc_fold, twice)
//   dx_crc32_combine  zlib's crc32_combine, on the host
// and, for dx_file_digest alone (dx_host.h): the ranges with a stride through their arrays, and pairs folded two and two.
//
// The algebra (zlib's crc32_combine): a CRC is a polynomial over GF(2) modulo P, bit 31 the coefficient of x^0.  The
// register after bytes B from the state S is  S * x^(8 |B|)  +  raw(B),  raw(B) being the register that starts at 0: so the
// register of A || B is that of A times x^(8 |B|), plus raw(B), and the same holds of the finished CRCs, whose initial
// value and final xor cancel: crc(A || B) = crc(A) * x^(8 |B|) + crc(B).  That operator on (crc, length) pairs is associative,
// with (0, 0), the empty unit, as its identity.  gfx950 has no carry-less multiply: a product modulo P is 32 steps of shift
// and xor (crc_mul), x^(8 n) the product of the x^(2^k) of n's bits (crc_x2n; the 32 powers are constants of P, C_X2N).
//
// Where the bytes go (k_crc_ranges; the waves draw tickets of consecutive units, 64 units to a wave at a time, a lane
// reading one unit's offset and length and checking them against the buffer):
//   * a unit under CRC_WAVE_MIN bytes is ONE LANE's: 64 units a wave at once, 16 bytes a load, a byte a look-up.  A header
//     line or a 300-symbol entry costs a 64th of a wave, and no product at all;
//   * a longer one is the wave's: 64 chunks of equal length c (a multiple of 16; the first lanes' lie in front of the unit
//     and are empty, which a register that starts at 0 does not notice), a lane a chunk, then six steps of
//     "left half times x^(8 c 2^s), plus right half" -- equal chunks, so ONE factor a step for the whole wave, squared from
//     step to step, kept in scalar registers;
//   * a unit of `split` bytes and more (1 MiB; DEXGPU_TEST=crc_split=<bytes> lowers it) is set aside on a list, and
//     k_crc_huge deals its pieces of CRC_PIECE bytes out over all waves of a second launch: a piece's register times
//     x^(8 * the bytes behind the piece) is its share of the unit's, and the shares are xored into the unit's word in any
//     order (the word starts as the final xor).  A list of CRC_HUGE_MAX units; what it does not hold stays one wave's.
//
// Table look-ups.  The byte-at-a-time table (256 words) stands in LDS 32 times, entry e of copy c at word 32 e + c, and a
// lane reads copy lane & 31.  ds_read_b32 serves a wave as two halves of 32 lanes over 32 banks of 4 bytes (bank =
// word mod 32): here a lane's bank IS its copy, so every look-up is conflict-free whatever the 64 registers hold -- 2 LDS
// cycles for 64 bytes.  The alternative was a wider slice, by 4 or by 8 (4 or 8 KB): it has as many look-ups a byte, only
// a shorter dependency chain, and its tables cannot be given a copy per bank (128 or 256 KB of the CU's 160); 32 lanes
// that look up random entries of one copy put 3.5 on the busiest of 32 banks on average, so a look-up costs 7 cycles
// rather than 2 and a CU is held to 256 bytes in 28 LDS cycles, 9 B/clk -- under the 12 to 15 B/clk at which the vector
// ALU issues the byte-at-a-time loop (4.25 instructions a byte: xor of the word, then and, shift-or, shift, xor a byte).
// With conflict-free look-ups the kernel is bound by that issue rate, not by LDS.  The price is 32 KB of LDS a workgroup:
// five workgroups, 20 waves a CU (kernel_resources.txt: lds=32768; the registers would allow more), which is what the
// dependent chain look-up -> xor -> look-up needs to be hidden.  These are estimates from the guide's bank rules and the
// compiler's code: profiles/digest_rate.txt has the command that measures them (tools/digest_rate.py) and what it gave.
//
// Nothing outside a unit's range is read (16-byte loads while 16 bytes are left, then bytes), and a unit that does not
// lie inside [0, buf_bytes) is not read at all: the smallest such index goes back to the host, one read-back a call.
//
// This file stands outside the evidence set of profiles/ (profiles/check.py hashes csrc/*.hip); its kernels have no entry
// in the profiler's name table and are timed with events on the context's stream (tools/digest_rate.py).
#include "units/dx_units.hpp"
extern "C" {
#include "dx_host.h"              // dx_crc32_ranges_strided, dx_crc32_pairs
}

#define CRC_POLY      0xedb88320u
#define CRC_WAVE_MIN  4096u                  // units from here on take the whole wave
#define CRC_SPLIT     (1ull << 20)           // ... and from here on several waves of a second launch
#define CRC_PIECE     (256u << 10)           // bytes of a split unit a wave takes at a time
#define CRC_HUGE_MAX  16384u                 // split units a call (more of them: a wave each)
#define CRC_FOLD_BLKS 1024u                  // workgroups of the fold's first launch at most

// x^(2^k) mod P, k = 0 .. 31 (x^(2^32) = x again: the powers go round)
#define CRC_X2N_VALUES                                                                                        \
  { 0x40000000u, 0x20000000u, 0x08000000u, 0x00800000u, 0x00008000u, 0xedb88320u, 0xb1e6b092u, 0xa06a2517u,   \
    0xed627daeu, 0x88d14467u, 0xd7bbfe6au, 0xec447f11u, 0x8e7ea170u, 0x6427800eu, 0x4d47bae0u, 0x09fe548fu,   \
    0x83852d0fu, 0x30362f1au, 0x7b5a9cc3u, 0x31fec169u, 0x9fec022au, 0x6c8dedc4u, 0x15d6874du, 0x5fde7a4eu,   \
    0xbad90e37u, 0x2e4e5eefu, 0x4eaba214u, 0xa8a472c0u, 0x429a969eu, 0x148d302au, 0xc40ba6d0u, 0xc4e22c3cu }
__constant__ uint32_t C_X2N[32] = CRC_X2N_VALUES;
static const uint32_t H_X2N[32] __attribute__((unused)) = CRC_X2N_VALUES;   // (the host's copy: dx_crc32_combine)

// a * b mod P: a's coefficients from x^0 (bit 31) on, b times x from step to step
__host__ __device__ __forceinline__ uint32_t crc_mul(uint32_t a, uint32_t b)
{ uint32_t p = 0;
  #pragma unroll 8
  for (int i = 31; i >= 0; i--)
    { p ^= b & (0u - ((a >> i) & 1u));
      b  = (b >> 1) ^ (CRC_POLY & (0u - (b & 1u)));
    }
  return p;
}

// x^(8 n) mod P
__host__ __device__ __forceinline__ uint32_t crc_x2n(uint64_t n)
{
#ifdef __HIP_DEVICE_COMPILE__
  const uint32_t *pw = C_X2N;
#else
  const uint32_t *pw = H_X2N;
#endif
  uint32_t p = 0x80000000u;                  // x^0
  for (uint32_t k = 3; n != 0; n >>= 1, k++)
    if (n & 1u) p = crc_mul(pw[k & 31u], p);
  return p;
}

extern "C" uint32_t dx_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b)
{ return crc_mul(crc_x2n(len_b), crc_a) ^ crc_b; }

// ---------------------------------------------------------------------------------------------
//  the table, and a lane's bytes
// ---------------------------------------------------------------------------------------------
#define CRC_TAB_WORDS (256u * 32u)

// all 32 copies, by the 256 threads of a workgroup: thread e makes entry e (eight steps of the register) and writes it 32 times
__device__ __forceinline__ void crc_table(uint32_t *s_tab)
{ for (uint32_t e = threadIdx.x; e < 256u; e += DX_BLOCK)
    { uint32_t v = e;
      #pragma unroll
      for (int k = 0; k < 8; k++) v = (v >> 1) ^ (CRC_POLY & (0u - (v & 1u)));
      for (uint32_t c = 0; c < 32u; c++) s_tab[32u * e + c] = v;
    }
  __syncthreads();
}

// tab: the table from this lane's copy on (s_tab + (lane & 31)), entry e 32 words further on each
__device__ __forceinline__ uint32_t crc_word(const uint32_t *tab, uint32_t crc, uint32_t w)
{ crc ^= w;
  #pragma unroll
  for (int k = 0; k < 4; k++) crc = tab[(crc & 0xffu) << 5] ^ (crc >> 8);
  return crc;
}

// the register after bytes p[0 .. n), from `crc` on: nothing but those bytes is read
__device__ __forceinline__ uint32_t crc_run(const uint32_t *tab, const uint8_t *p, uint64_t n, uint32_t crc)
{ uint64_t at = 0;
  if (n >= 16u)
    { u32x4 v = *(const u32x4_u *) p;
      for (; at + 32u <= n; at += 16u)       // the next 16 bytes are asked for before these are gone through
        { const u32x4 nx = *(const u32x4_u *) (p + at + 16u);
          crc = crc_word(tab, crc, v.x); crc = crc_word(tab, crc, v.y); crc = crc_word(tab, crc, v.z); crc = crc_word(tab, crc, v.w);
          v = nx;
        }
      crc = crc_word(tab, crc, v.x); crc = crc_word(tab, crc, v.y); crc = crc_word(tab, crc, v.z); crc = crc_word(tab, crc, v.w);
      at += 16u;
    }
  for (; at < n; at++) crc = tab[((crc ^ p[at]) & 0xffu) << 5] ^ (crc >> 8);
  return crc;
}

// The register after bytes p[0 .. L) from `init` on, by the whole wave (p, L, init uniform; L > 0); every lane has the answer.
// Lane i's chunk ends at L - (63 - i) c and is c bytes long, less where it begins in front of the unit; the lane that holds
// byte 0 starts from init, the others from 0.
__device__ __forceinline__ uint32_t crc_wave(const uint32_t *tab, const uint8_t *p, uint64_t L, uint32_t init)
{ const uint32_t lane = (uint32_t) lane_id();
  const uint64_t c = (((L + 63u) >> 6) + 15u) & ~15ull;
  const int64_t  e = (int64_t) L - (int64_t) ((uint64_t) (63u - lane) * c);
  uint32_t st = 0;
  if (e > 0)
    { const int64_t s = e - (int64_t) c;
      st = s <= 0 ? crc_run(tab, p, (uint64_t) e, init) : crc_run(tab, p + s, c, 0u);
    }
  // lane 63 of step s holds chunks 64 - 2^(s+1) .. 63: the 2^s on its left, moved past the 2^s on its right, and those
  uint32_t f = crc_x2n(c);
  #pragma unroll
  for (int d = 1; d < 64; d += d)
    { const uint32_t left = (uint32_t) __shfl_up((int) st, d);
      st = crc_mul(left, f) ^ st;
      f  = crc_mul(f, f);
    }
  return (uint32_t) __builtin_amdgcn_readlane((int) st, 63);
}

// ---------------------------------------------------------------------------------------------
//  the units
// ---------------------------------------------------------------------------------------------
// Unit j: off[j * stride], len[j * stride] -> crc[j * stride].  bad: the smallest index of a unit that does not lie inside the
// buffer (preset to all ones).  ticket[0]: the units' counter.  huge / huge_n: the units set aside for k_crc_huge.
__global__ __launch_bounds__(DX_BLOCK)
void k_crc_ranges(const uint8_t *__restrict__ buf, uint64_t buf_bytes, const uint64_t *__restrict__ off, const uint64_t *__restrict__ len,
                  uint64_t n, uint64_t stride, uint32_t *__restrict__ crc, unsigned long long *__restrict__ bad,
                  uint32_t *__restrict__ ticket, uint32_t per_ticket, uint64_t split, uint32_t *__restrict__ huge, uint32_t *__restrict__ huge_n)
{ __shared__ uint32_t s_tab[CRC_TAB_WORDS];
  crc_table(s_tab);
  const uint32_t  lane = (uint32_t) lane_id();
  const uint32_t *tab  = s_tab + (lane & 31u);
  units_rounds<false>(ticket, per_ticket, n, [&](uint64_t u0, uint64_t r1)
    { const uint64_t i = u0 + lane;
      uint64_t at = 0, L = 0;
      int      kind = 0;                     // 1: this lane's, 2: the wave's, 3: set aside
      if (i < r1)
        { at = off[i * stride]; L = len[i * stride];
          if (range_ok(at, L, buf_bytes)) kind = L < CRC_WAVE_MIN ? 1 : (L < split ? 2 : 3);
          else atomicMin(bad, (unsigned long long) i);
        }
      if (kind == 3)
        { const uint32_t k = atomicAdd(huge_n, 1u);
          if (k < CRC_HUGE_MAX) { huge[k] = (uint32_t) i; crc[i * stride] = 0xffffffffu; }      // (the final xor; the pieces' shares follow)
          else kind = 2;
        }
      if (kind == 1) crc[i * stride] = ~crc_run(tab, buf + at, L, 0xffffffffu);
      units_each(__ballot(kind == 2), [&](int from)
        { const uint64_t wat = uniform64(__shfl(at, from)), wL = uniform64(__shfl(L, from));
          const uint32_t st  = crc_wave(tab, buf + wat, wL, 0xffffffffu);
          if (lane == 0) crc[(u0 + (uint64_t) from) * stride] = ~st;
        });
    });
}

// The units on the list, piece by piece: the pieces of all of them are numbered through, and wave w of W takes the numbers
// that are w modulo W.
__global__ __launch_bounds__(DX_BLOCK)
void k_crc_huge(const uint8_t *__restrict__ buf, const uint64_t *__restrict__ off, const uint64_t *__restrict__ len, uint64_t stride,
                uint32_t *__restrict__ crc, const uint32_t *__restrict__ huge, const uint32_t *__restrict__ huge_n)
{ __shared__ uint32_t s_tab[CRC_TAB_WORDS];
  const uint32_t listed = *huge_n, cnt = listed < CRC_HUGE_MAX ? listed : CRC_HUGE_MAX;
  if (cnt == 0u) return;
  crc_table(s_tab);
  const uint32_t  lane = (uint32_t) lane_id();
  const uint32_t *tab  = s_tab + (lane & 31u);
  const uint64_t  W = (uint64_t) gridDim.x * DX_WAVES_PER_BLK, w = uniform(blockIdx.x * DX_WAVES_PER_BLK + (threadIdx.x >> 6));
  uint64_t base = 0;
  for (uint32_t h = 0; h < cnt; h++)
    { const uint64_t j = huge[h], at = off[j * stride], L = len[j * stride], np = (L + CRC_PIECE - 1u) / CRC_PIECE;
      for (uint64_t q = (w + W - base % W) % W; q < np; q += W)
        { const uint64_t b0 = q * CRC_PIECE, bl = L - b0 < CRC_PIECE ? L - b0 : CRC_PIECE;
          const uint32_t st = crc_wave(tab, buf + at + b0, bl, q == 0 ? 0xffffffffu : 0u);
          const uint32_t sh = crc_mul(st, crc_x2n(L - b0 - bl));
          if (lane == 0) atomicXor(crc + j * stride, sh);
        }
      base += np;
    }
}

static int crc_ranges(dx_ctx *ctx, const char *who, const uint8_t *d_buf, uint64_t buf_bytes, const uint64_t *d_off, const uint64_t *d_len,
                      uint64_t n, uint64_t stride, uint32_t *d_crc, uint64_t *bad_unit)
{ if (ctx == NULL) return DX_E_ARG;
  if (bad_unit) *bad_unit = UINT64_MAX;
  if (n == 0) return DX_OK;
  units_frame f;                                           // (answer word 0: how many units are set aside)
  uint64_t    back[UF_OUT + 1];
  uint32_t   *d_huge;
  int rc = units_begin(ctx, who, n, d_off && d_len && d_crc && (d_buf || !buf_bytes) && stride != 0, ctx->d_u64 + DXW_UNITS, 1, 0, NULL, NULL, &f);
  if (rc != DX_OK) return rc;
  if ((rc = dx_scratch(ctx, CRC_HUGE_MAX * sizeof(uint32_t), (void **) &d_huge)) != DX_OK) return rc;
  long long split = dx_test_num("crc_split", (long long) CRC_SPLIT);                 // (tests: units split from this size on)
  if (split < (long long) CRC_WAVE_MIN) split = CRC_WAVE_MIN;
  // a ticket: 64 units at least; of many units more, so that the draws (an atomic on one address each) stay few beside the work
  const int grid = dx_grid_waves(ctx, (n + 63u) / 64u, 20);
  uint64_t  per  = n / ((uint64_t) grid * DX_WAVES_PER_BLK * 8u);
  per = per < 64u ? 64u : (per > 4096u ? 4096u : per & ~63ull);
  hipLaunchKernelGGL(k_crc_ranges, dim3(grid), dim3(DX_BLOCK), 0, ctx->stream, d_buf, buf_bytes, d_off, d_len, n, stride, d_crc,
                     f.bad, f.ticket, (uint32_t) per, (uint64_t) split, d_huge, (uint32_t *) f.out);
  DX_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_crc_huge, dim3(dx_grid_waves(ctx, UINT64_MAX, 20)), dim3(DX_BLOCK), 0, ctx->stream, d_buf, d_off, d_len, stride,
                     d_crc, d_huge, (const uint32_t *) f.out);
  return units_end(ctx, f, back, bad_unit, "%s: unit %llu does not lie inside the buffer's %llu bytes", buf_bytes);
}

extern "C" int dx_crc32_ranges(dx_ctx *ctx, const uint8_t *d_buf, uint64_t buf_bytes, const uint64_t *d_off, const uint64_t *d_len,
                               uint64_t n, uint32_t *d_crc, uint64_t *bad_unit)
{ return crc_ranges(ctx, "dx_crc32_ranges", d_buf, buf_bytes, d_off, d_len, n, 1, d_crc, bad_unit); }

extern "C" int dx_crc32_ranges_strided(dx_ctx *ctx, const uint8_t *d_buf, uint64_t buf_bytes, const uint64_t *d_off, const uint64_t *d_len,
                                       uint64_t n, uint64_t stride, uint32_t *d_crc, uint64_t *bad_unit)
{ return crc_ranges(ctx, "dx_crc32_ranges", d_buf, buf_bytes, d_off, d_len, n, stride, d_crc, bad_unit); }

// ---------------------------------------------------------------------------------------------
//  the fold
// ---------------------------------------------------------------------------------------------
// (a_crc, a_len) in front of (b_crc, b_len)
__device__ __forceinline__ void crc_join(uint32_t a_crc, uint64_t a_len, uint32_t &b_crc, uint64_t &b_len)
{ b_crc ^= crc_mul(a_crc, crc_x2n(b_len));
  b_len += a_len;
}

// Thread t folds units [t per, (t + 1) per) one after the other; the wave's 64 results are joined in six steps, the workgroup's
// four by its first thread: out[blockIdx.x].  A second launch of one workgroup folds the first one's results.
__global__ __launch_bounds__(DX_BLOCK)
void k_crc_fold(const uint32_t *__restrict__ crc, const uint64_t *__restrict__ len, uint64_t n, uint64_t per,
                uint32_t *__restrict__ out_crc, uint64_t *__restrict__ out_len)
{ __shared__ uint32_t s_crc[DX_WAVES_PER_BLK];
  __shared__ uint64_t s_len[DX_WAVES_PER_BLK];
  const uint32_t lane = (uint32_t) lane_id();
  const uint64_t t  = (uint64_t) blockIdx.x * DX_BLOCK + threadIdx.x;
  const uint64_t lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
  uint32_t c = 0;
  uint64_t l = 0;
  for (uint64_t u = lo; u < hi; u++)
    { uint32_t uc = crc[u];
      uint64_t ul = len[u];
      crc_join(c, l, uc, ul);
      c = uc; l = ul;
    }
  #pragma unroll
  for (int d = 1; d < 64; d += d)
    { const uint32_t lc = (uint32_t) __shfl_up((int) c, d);
      const uint64_t ll = (uint64_t) __shfl_up((unsigned long long) l, d);
      if (lane >= (uint32_t) d) crc_join(lc, ll, c, l);
    }
  if (lane == 63u) { s_crc[threadIdx.x >> 6] = c; s_len[threadIdx.x >> 6] = l; }
  __syncthreads();
  if (threadIdx.x == 0)
    { c = s_crc[0]; l = s_len[0];
      for (int k = 1; k < DX_WAVES_PER_BLK; k++)
        { uint32_t kc = s_crc[k];
          uint64_t kl = s_len[k];
          crc_join(c, l, kc, kl);
          c = kc; l = kl;
        }
      out_crc[blockIdx.x] = c; out_len[blockIdx.x] = l;
    }
}

extern "C" int dx_crc32_fold(dx_ctx *ctx, const uint32_t *d_crc, const uint64_t *d_len, uint64_t n, uint32_t *crc, uint64_t *bytes)
{ if (ctx == NULL) return DX_E_ARG;
  if (crc == NULL || bytes == NULL)
    return dx_fail(ctx, DX_E_ARG, "dx_crc32_fold: nowhere to put the answer");
  *crc = 0; *bytes = 0;
  if (n == 0) return DX_OK;
  if (!d_crc || !d_len)
    return dx_fail(ctx, DX_E_ARG, "dx_crc32_fold: NULL device pointer");
  DX_HIP(ctx, hipSetDevice(ctx->device));
  int rc = dx_after_pending(ctx);
  if (rc != DX_OK) return rc;

  uint64_t *d_res = ctx->d_u64 + DXW_UNITS + UF_OUT, back[2];   // the CRC's word, the length: the frame's answer words
  uint64_t  blocks = (n + 4u * DX_BLOCK - 1u) / (4u * DX_BLOCK);
  if (blocks > CRC_FOLD_BLKS) blocks = CRC_FOLD_BLKS;
  const uint64_t per = (n + blocks * DX_BLOCK - 1u) / (blocks * DX_BLOCK);
  DX_HIP(ctx, hipMemsetAsync(d_res, 0, 16, ctx->stream));
  if (blocks == 1u)
    hipLaunchKernelGGL(k_crc_fold, dim3(1), dim3(DX_BLOCK), 0, ctx->stream, d_crc, d_len, n, per, (uint32_t *) d_res, d_res + 1);
  else
    { uint64_t *d_part;                                    // the workgroups' lengths, their CRCs behind them
      if ((rc = dx_scratch(ctx, CRC_FOLD_BLKS * 12u, (void **) &d_part)) != DX_OK) return rc;
      uint32_t *d_pcrc = (uint32_t *) (d_part + CRC_FOLD_BLKS);
      hipLaunchKernelGGL(k_crc_fold, dim3((uint32_t) blocks), dim3(DX_BLOCK), 0, ctx->stream, d_crc, d_len, n, per, d_pcrc, d_part);
      DX_HIP(ctx, hipGetLastError());
      hipLaunchKernelGGL(k_crc_fold, dim3(1), dim3(DX_BLOCK), 0, ctx->stream, (const uint32_t *) d_pcrc, (const uint64_t *) d_part, blocks,
                         (blocks + DX_BLOCK - 1u) / DX_BLOCK, (uint32_t *) d_res, d_res + 1);
    }
  DX_HIP(ctx, hipGetLastError());
  DX_HIP(ctx, hipMemcpyAsync(back, d_res, 16, hipMemcpyDeviceToHost, ctx->stream));
  DX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *crc = (uint32_t) back[0]; *bytes = back[1];
  return DX_OK;
}

// units 2 k and 2 k + 1 joined: m pairs of units -> m units
__global__ __launch_bounds__(DX_BLOCK)
void k_crc_pairs(const uint32_t *__restrict__ crc, const uint64_t *__restrict__ len, uint64_t m,
                 uint32_t *__restrict__ out_crc, uint64_t *__restrict__ out_len)
{ for (uint64_t k = (uint64_t) blockIdx.x * DX_BLOCK + threadIdx.x; k < m; k += (uint64_t) gridDim.x * DX_BLOCK)
    { uint32_t c = crc[2u * k + 1u];
      uint64_t l = len[2u * k + 1u];
      crc_join(crc[2u * k], len[2u * k], c, l);
      out_crc[k] = c; out_len[k] = l;
    }
}

extern "C" int dx_crc32_pairs(dx_ctx *ctx, const uint32_t *d_crc, const uint64_t *d_len, uint64_t m, uint32_t *d_out_crc, uint64_t *d_out_len)
{ if (ctx == NULL) return DX_E_ARG;
  if (m == 0) return DX_OK;
  if (!d_crc || !d_len || !d_out_crc || !d_out_len)
    return dx_fail(ctx, DX_E_ARG, "dx_crc32_pairs: NULL device pointer");
  DX_HIP(ctx, hipSetDevice(ctx->device));
  int rc = dx_after_pending(ctx);
  if (rc != DX_OK) return rc;
  uint64_t blocks = (m + DX_BLOCK - 1u) / DX_BLOCK;
  if (blocks > 4096u) blocks = 4096u;
  hipLaunchKernelGGL(k_crc_pairs, dim3((uint32_t) blocks), dim3(DX_BLOCK), 0, ctx->stream, d_crc, d_len, m, d_out_crc, d_out_len);
  DX_HIP(ctx, hipGetLastError());
  return DX_OK;
}
