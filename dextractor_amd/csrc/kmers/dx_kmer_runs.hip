// dx_kmer_runs.hip -- what a sorted array of k-mer codes holds: dx_kmer_runs, the counts read off the runs of equal keys.
//
//   k_run_heads   tile t (KR_TILE = 2048 keys): the place of its first key that begins a run, or none
//   k_run_count   every run's length, where it begins: the spectrum, the runs, the longest and its smallest code, and a tile's runs
//                 that pass min_count
//   k_run_list    ... and those runs written, in the order of the codes, from the tile's first place on (dx_scan_u32 of the counts)
//
// The last step of the wide route.  The meanings are dx_kmer_spectrum's and dx_kmer_list's with a run in a cell's place:
// a run is a maximal stretch of equal keys, its length the code's count.  Key i begins a run if i == 0 or key[i] != key[i - 1]; the
// run's length is the distance to the next such key, or to n.  A tile works that out for the runs that BEGIN in it (kr_tile): a thread
// holds 8 consecutive keys, its first begin is handed down the workgroup as a suffix minimum, and behind the tile's last begin the
// workgroup looks through k_run_heads' words of the tiles that follow, 256 a step, for the first that has one -- a run of 10^5 equal
// keys (a homopolymer's) is 49 tiles, one step; all of 10^9 keys equal would be 1900 steps of one workgroup.
// Nothing is placed by an atomic cursor: the list's places come from the tiles' counts and a prefix sum, as in k_kmer_list.
// The spectrum's bins stand in LDS (KR_BINS at most; the few runs beyond go to the global words directly); the runs of length 1 --
// nearly all of them at a wide k -- are counted in a register and added once a thread, so that 64 lanes do not queue on bin 1.
// A workgroup's (runs, longest, its smallest code) go to a place of its own and the host folds them.  Read-backs: dx_scan_u32's
// total (the runs that pass), then one copy of the spectrum and the workgroups' words.
//
// Cost: 8 bytes read a key by k_run_heads and 8 by k_run_count, 8 more and 16 written an entry with a list; about 12 vector
// instructions a key (the compare with the key before, the flags, the walk back over 8 keys) and a few hundred a tile for the two
// scans.  ESTIMATE: bound by HBM, 16 GB for 10^9 keys, 3.5 to 4 ms.  MEASURED (profiles/kmer_wide_rate.txt, counting only, a
// spectrum of 256 bins, both read-backs included): 4.7 to 4.8 ms for 10^9 keys, 3.4 TB/s, whether 26 % of the keys begin a run
// (k = 14) or all of them (k = 32).
//
// This file stands outside the evidence set of profiles/ (profiles/check.py hashes csrc/*.hip); its kernels have no entry in the
// profiler's name table and are timed with events on the context's stream (tools/kmer_wide_rate.py).
#include "dx_internal.hpp"
#include "dx_device.hpp"

extern "C" {
#include "dx_host.h"
}

#define KR_ITEMS 8u                           // keys a thread
#define KR_TILE  (DX_BLOCK * KR_ITEMS)        // keys a workgroup
#define KR_BINS  4096u                        // bins of the spectrum that stand in LDS
#define KR_NONE  0xffffffffu
#define KR_NMAX  (1ull << 36)


struct kr_block_out { unsigned long long distinct, max_count, max_code; };       // a workgroup's: its runs, the longest, its smallest code

// the smallest value over the workgroup (every thread gets it); s_w: a word a wave
__device__ __forceinline__ uint32_t kr_block_min(uint32_t v, uint32_t *s_w)
{
  #pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = min(v, (uint32_t) __shfl_xor((int) v, d));
  __syncthreads();                                         // (s_w may still be read from its last use)
  if (lane_id() == 0) s_w[threadIdx.x / DX_WAVE] = v;
  __syncthreads();
  return min(min(s_w[0], s_w[1]), min(s_w[2], s_w[3]));
}

// first[t] = the place in tile t of its first key that begins a run, KR_NONE if it has none
__global__ __launch_bounds__(DX_BLOCK)
void k_run_heads(const uint64_t *__restrict__ key, uint64_t n, uint32_t *__restrict__ first)
{ __shared__ uint32_t s_w[DX_WAVES_PER_BLK];
  const uint64_t i0 = (uint64_t) blockIdx.x * KR_TILE + (uint64_t) KR_ITEMS * threadIdx.x;
  uint32_t mine = KR_NONE;
  if (i0 < n)
    { uint64_t prev = i0 ? key[i0 - 1u] : 0ull;
      #pragma unroll
      for (uint32_t j = 0; j < KR_ITEMS; j++)
        if (i0 + j < n)
          { const uint64_t v = key[i0 + j];
            if ((i0 + j == 0u || v != prev) && mine == KR_NONE) mine = KR_ITEMS * threadIdx.x + j;
            prev = v;
          }
    }
  const uint32_t all = kr_block_min(mine, s_w);
  if (threadIdx.x == 0u) first[blockIdx.x] = all;
}

// Tile t's keys, 8 a thread: v[j] = key KR_TILE t + 8 x + j, len[j] = the length of the run that begins there, 0 where none does.
// Uniform over the workgroup (it synchronises); s_f: a word a thread, s_w: a word a wave.
__device__ __forceinline__ void kr_tile(const uint64_t *__restrict__ key, uint64_t n, const uint32_t *__restrict__ first, uint64_t tiles,
                                        uint64_t t, uint32_t *s_f, uint32_t *s_w, uint64_t v[KR_ITEMS], uint64_t len[KR_ITEMS])
{ const uint64_t t0 = t * KR_TILE, i0 = t0 + (uint64_t) KR_ITEMS * threadIdx.x;
  bool     head[KR_ITEMS];
  uint32_t mine = KR_NONE;                                 // this thread's first begin, as a place in the tile
  uint64_t prev = i0 && i0 < n ? key[i0 - 1u] : 0ull;
  #pragma unroll
  for (uint32_t j = 0; j < KR_ITEMS; j++)
    { const bool have = i0 + j < n;
      v[j] = have ? key[i0 + j] : 0ull;
      head[j] = have && (i0 + j == 0u || v[j] != prev);
      if (head[j] && mine == KR_NONE) mine = KR_ITEMS * threadIdx.x + j;
      prev = v[j];
    }

  // the first begin behind the tile: in the tiles that follow, 256 of them a step; n if there is none
  uint64_t beyond = n;
  for (uint64_t b = t + 1u; b < tiles; b += DX_BLOCK)
    { const uint64_t u = b + threadIdx.x;
      const uint32_t f = u < tiles ? first[u] : KR_NONE;
      const uint32_t w = kr_block_min(f != KR_NONE ? threadIdx.x : KR_NONE, s_w);                  // the nearest such tile of the 256
      if (w != KR_NONE)
        { beyond = (b + w) * KR_TILE + first[b + w];
          break;                                                                                   // (uniform: w is the workgroup's)
        }
    }

  // the first begin behind this thread's keys: the smallest of the threads above it
  __syncthreads();
  s_f[threadIdx.x] = mine;
  __syncthreads();
  const uint32_t lane = (uint32_t) lane_id(), wave = threadIdx.x / DX_WAVE;
  uint32_t after = lane < 63u ? s_f[threadIdx.x + 1u] : KR_NONE;                                  // the wave's lanes above, suffix minimum
  #pragma unroll
  for (uint32_t d = 1; d < 64u; d <<= 1)
    { const uint32_t o = (uint32_t) __shfl_down((int) after, d);
      if (lane + d < 64u) after = min(after, o);
    }
  const uint32_t whole = min(after, mine);                                                       // the wave's first begin, in lane 0
  if (lane == 0u) s_w[wave] = whole;
  __syncthreads();
  for (uint32_t w = wave + 1u; w < DX_WAVES_PER_BLK; w++) after = min(after, s_w[w]);
  uint64_t next = after != KR_NONE ? t0 + after : beyond;
  #pragma unroll
  for (uint32_t jj = 0; jj < KR_ITEMS; jj++)
    { const uint32_t j = KR_ITEMS - 1u - jj;
      len[j] = 0ull;
      if (head[j]) { len[j] = next - (i0 + j); next = i0 + j; }
    }
  __syncthreads();                                         // (s_f, s_w: free for the next tile)
}

// spec: nspec words (nspec 0: none) the workgroups add their bins to; per: a kr_block_out a workgroup; pass[t]: tile t's runs of
// min_count keys at least
__global__ __launch_bounds__(DX_BLOCK)
void k_run_count(const uint64_t *__restrict__ key, uint64_t n, const uint32_t *__restrict__ first, uint64_t tiles, uint64_t min_count,
                 uint32_t nspec, unsigned long long *__restrict__ spec, kr_block_out *__restrict__ per, uint32_t *__restrict__ pass)
{ __shared__ uint32_t           s_bin[KR_BINS];
  __shared__ uint32_t           s_f[DX_BLOCK], s_w[DX_WAVES_PER_BLK], s_n[DX_WAVES_PER_BLK];
  __shared__ unsigned long long s_d[DX_WAVES_PER_BLK], s_m[DX_WAVES_PER_BLK], s_c[DX_WAVES_PER_BLK];
  const uint32_t inside = nspec < KR_BINS ? nspec : KR_BINS;
  for (uint32_t b = threadIdx.x; b < inside; b += DX_BLOCK) s_bin[b] = 0u;
  __syncthreads();

  unsigned long long d = 0, m = 0, mc = 0, ones = 0;
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x)
    { uint64_t v[KR_ITEMS], len[KR_ITEMS];
      kr_tile(key, n, first, tiles, t, s_f, s_w, v, len);
      uint32_t mine = 0;
      #pragma unroll
      for (uint32_t j = 0; j < KR_ITEMS; j++)
        if (len[j])
          { d++;
            if (len[j] > m) { m = len[j]; mc = v[j]; }       // (a thread's codes ascend, tile after tile: of equal lengths the first stays)
            if (len[j] >= min_count) mine++;
            if (len[j] == 1ull) ones++;
            else if (nspec)
              { const uint32_t b = len[j] < (uint64_t) (nspec - 1u) ? (uint32_t) len[j] : nspec - 1u;
                if (b < KR_BINS) atomicAdd(s_bin + b, 1u);
                else             atomicAdd(spec + b, 1ull);
              }
          }
      const uint32_t all = wave_sum(mine);
      if (lane_id() == 0) s_n[threadIdx.x / DX_WAVE] = all;
      __syncthreads();
      if (threadIdx.x == 0u) pass[t] = s_n[0] + s_n[1] + s_n[2] + s_n[3];
    }

  #pragma unroll
  for (int s = 32; s > 0; s >>= 1)
    { const unsigned long long om = __shfl_xor(m, s), oc = __shfl_xor(mc, s);
      d += __shfl_xor(d, s);
      ones += __shfl_xor(ones, s);
      if (om > m || (om == m && oc < mc)) { m = om; mc = oc; }
    }
  if (lane_id() == 0)
    { s_d[threadIdx.x / DX_WAVE] = d; s_m[threadIdx.x / DX_WAVE] = m; s_c[threadIdx.x / DX_WAVE] = mc;
      if (nspec && ones) atomicAdd(spec + 1, ones);          // (nspec >= 2: bin 1 is there, and with two bins it is the one that gathers)
    }
  __syncthreads();
  if (threadIdx.x == 0u)
    { for (uint32_t w = 1; w < DX_WAVES_PER_BLK; w++)
        { d += s_d[w];
          if (s_m[w] > m || (s_m[w] == m && s_c[w] < mc)) { m = s_m[w]; mc = s_c[w]; }
        }
      per[blockIdx.x].distinct = d; per[blockIdx.x].max_count = m; per[blockIdx.x].max_code = m ? mc : 0ull;
    }
  for (uint32_t b = threadIdx.x; b < inside; b += DX_BLOCK)
    if (s_bin[b]) atomicAdd(spec + b, (unsigned long long) s_bin[b]);
}

// start: every tile's first place in the list (dx_scan_u32 of k_run_count's counts); an entry is 16 bytes: code (8), count (8)
__global__ __launch_bounds__(DX_BLOCK)
void k_run_list(const uint64_t *__restrict__ key, uint64_t n, const uint32_t *__restrict__ first, uint64_t tiles, uint64_t min_count,
                const uint64_t *__restrict__ start, u32x4_u *__restrict__ out, uint64_t cap)
{ __shared__ uint32_t s_f[DX_BLOCK], s_w[DX_WAVES_PER_BLK], s_n[DX_WAVES_PER_BLK];
  const uint64_t from = start[blockIdx.x];
  if (from >= cap || start[blockIdx.x + 1u] == from) return;                 // (uniform: the whole workgroup leaves)
  uint64_t v[KR_ITEMS], len[KR_ITEMS];
  kr_tile(key, n, first, tiles, blockIdx.x, s_f, s_w, v, len);
  uint32_t mine = 0;
  #pragma unroll
  for (uint32_t j = 0; j < KR_ITEMS; j++)
    if (len[j] && len[j] >= min_count) mine++;
  const uint32_t incl = wave_incl_scan(mine), wave = threadIdx.x / DX_WAVE;
  if (lane_id() == 63) s_n[wave] = incl;
  __syncthreads();
  uint64_t at = from + (incl - mine);
  for (uint32_t w = 0; w < wave; w++) at += s_n[w];
  #pragma unroll
  for (uint32_t j = 0; j < KR_ITEMS; j++)
    if (len[j] && len[j] >= min_count)
      { if (at < cap)
          { u32x4 e;
            e.x = (uint32_t) v[j]; e.y = (uint32_t) (v[j] >> 32); e.z = (uint32_t) len[j]; e.w = (uint32_t) (len[j] >> 32);
            out[at] = e;
          }
        at++;
      }
}

// ---------------------------------------------------------------------------------------------
//  the entry point
// ---------------------------------------------------------------------------------------------
static_assert(sizeof(dx_kmer64) == 16 && sizeof(dx_kmers64) == 56 && sizeof(kr_block_out) == 24, "an entry of the list is one 16-byte store");

extern "C" int dx_kmer_runs(dx_ctx *ctx, const uint64_t *d_sorted, uint64_t n, uint64_t min_count, dx_kmer64 *d_out, uint64_t cap,
                            uint64_t *found, uint64_t *spectrum, uint32_t nspec, uint64_t *distinct, uint64_t *max_count, uint64_t *max_code)
{ if (ctx == NULL) return DX_E_ARG;
  if (found) *found = 0;
  if (found == NULL || (d_sorted == NULL && n) || (d_out == NULL && cap)) return dx_fail(ctx, DX_E_ARG, "dx_kmer_runs: NULL pointer");
  if (min_count < 1u) return dx_fail(ctx, DX_E_ARG, "dx_kmer_runs: min_count 0 (1 at least: the unseen codes are not listed)");
  if (spectrum != NULL && nspec < 2u) return dx_fail(ctx, DX_E_ARG, "dx_kmer_runs: a spectrum of %u bins (2 at least)", nspec);
  if (n >= KR_NMAX) return dx_fail(ctx, DX_E_ARG, "dx_kmer_runs: %llu keys (fewer than 2^36)", (unsigned long long) n);
  if (spectrum == NULL) nspec = 0;
  if (n == 0)
    { if (nspec) memset(spectrum, 0, (size_t) nspec * 8u);
      if (distinct) *distinct = 0;
      if (max_count) *max_count = 0;
      if (max_code) *max_code = 0;
      return DX_OK;
    }
  DX_HIP(ctx, hipSetDevice(ctx->device));
  int rc = dx_after_pending(ctx);
  if (rc != DX_OK) return rc;

  // one scratch block: the spectrum, the workgroups' words, every tile's first place in the list (tiles + 1), and behind them the
  // tiles' counts and first begins
  const uint64_t tiles = (n + KR_TILE - 1u) / KR_TILE;
  const int      grid  = dx_grid_waves(ctx, tiles * DX_WAVES_PER_BLK, 16);
  const size_t   words = (size_t) nspec + 3u * (size_t) grid;
  uint64_t      *d_w   = NULL;
  if ((rc = dx_scratch(ctx, (words + tiles + 1u + tiles + 1u) * 8u, (void **) &d_w)) != DX_OK) return rc;
  uint64_t *d_start = d_w + words;
  uint32_t *d_pass  = (uint32_t *) (d_start + tiles + 1u), *d_first = d_pass + tiles;
  if (nspec) DX_HIP(ctx, hipMemsetAsync(d_w, 0, (size_t) nspec * 8u, ctx->stream));
  hipLaunchKernelGGL(k_run_heads, dim3((unsigned) tiles), dim3(DX_BLOCK), 0, ctx->stream, d_sorted, n, d_first);
  hipLaunchKernelGGL(k_run_count, dim3(grid), dim3(DX_BLOCK), 0, ctx->stream, d_sorted, n, (const uint32_t *) d_first, tiles, min_count, nspec,
                     (unsigned long long *) d_w, (kr_block_out *) (d_w + nspec), d_pass);
  DX_HIP(ctx, hipGetLastError());
  if ((rc = dx_scan_u32(ctx, d_pass, tiles, d_start, found)) != DX_OK) return rc;
  if (cap && *found)
    { hipLaunchKernelGGL(k_run_list, dim3((unsigned) tiles), dim3(DX_BLOCK), 0, ctx->stream, d_sorted, n, (const uint32_t *) d_first, tiles,
                         min_count, (const uint64_t *) d_start, (u32x4_u *) d_out, cap);
      DX_HIP(ctx, hipGetLastError());
    }
  std::vector<uint64_t> back(words);
  DX_HIP(ctx, hipMemcpyAsync(back.data(), d_w, words * 8u, hipMemcpyDeviceToHost, ctx->stream));
  DX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  uint64_t d = 0, m = 0, mc = 0;
  for (int b = 0; b < grid; b++)
    { const uint64_t *o = back.data() + nspec + 3u * (size_t) b;
      d += o[0];
      if (o[1] > m || (o[1] == m && m && o[2] < mc)) { m = o[1]; mc = o[2]; }
    }
  if (nspec) memcpy(spectrum, back.data(), (size_t) nspec * 8u);
  if (distinct) *distinct = d;
  if (max_count) *max_count = m;
  if (max_code) *max_code = mc;
  return DX_OK;
}

// dx_host.h: dx_file_kmers_wide.c's refusals, worded there
extern "C" int dx_kmers_wide_fail(dx_ctx *ctx, int code, const char *what)
{ if (ctx == NULL) return code;
  return dx_fail(ctx, code, "dx_file_kmers_wide: %s", what);
}
