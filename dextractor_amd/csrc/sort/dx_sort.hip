// dx_sort.hip -- 64-bit keys sorted on the device: dx_sort_u64, a radix sort from the lowest digit up (k_sort_hist, k_sort_scatter).
//
// A pass takes SORT_BITS = 8 bits of the key, lowest first, and leaves the keys in the order of that digit, keys of one digit in the
// order they had (stable): after the last pass the keys stand in ascending order.  Only the digits that cover `bits` are passed over --
// 2 k bits of a k-mer's code are ceil(k / 4) passes.  A pass is three steps:
//   k_sort_hist     tile t (SORT_TILE = 4096 keys) counts its keys a digit: count[d * tiles + t], digit-major;
//   dx_scan_u32     the exclusive sums of the 256 x tiles counts: first[d * tiles + t], the place of tile t's first key of digit d;
//   k_sort_scatter  tile t ranks its keys -- digit, then place in the tile --, lays them out in LDS in that order and writes them,
//                   a thread the key at place p of the tile's order, to first[d * tiles + t] + (p - the tile's first place of d).
// The keys go to and fro between d_keys and d_tmp; an odd number of passes ends in d_tmp and is copied back.
//
// Ranks.  A wave takes 64 consecutive keys at a time (lane l the l-th), 16 times.  The lanes that hold the same digit find each other
// with eight ballots, a bit of the digit each (sort_peers): peers = AND over the bits of (ballot or its complement).  The lowest lane
// of a set of peers is its leader: it alone touches the digit's counter -- the wave's own row of 256 words in LDS --, reads what the
// wave's earlier keys left there and adds the set's size; a lane's rank among the wave's keys of its digit is that old value plus
// the peers below it.  No two leaders of a step share a digit, so no address is asked for twice in one instruction, and nothing is
// an atomic: 64 equal keys cost what 64 different ones cost, which is the point -- a read set is full of poly-A and poly-T, and one
// digit that holds a fifth (or all) of the keys is a normal input.
// The histogram kernel needs counts, not ranks, and counts with ds_add_u32 into one row of counters the workgroup shares: lanes that
// add to one address take an LDS cycle each, 64 at the worst, which is what the eight ballots and their selects would cost a wave
// anyway (some 40 vector instructions, 160 cycles of a SIMD, the LDS being shared by four) -- so the plain add is never dearer than
// the peers and on digits that differ far cheaper.  The one case that is looked for is a wave whose 64 keys all hold one digit: its
// first lane adds 64.
// The rows of the four waves become the tile's order digit by digit (thread d: its digit's four counts, a prefix sum over the
// digits), stable because wave w's keys stand before wave w + 1's and a wave's in the order it took them.
//
// Cost a key and pass, counted from the source (what hipcc -O3 --offload-arch=gfx950 makes of it was not gone through line by line):
//   bytes: 8 read by k_sort_hist, 8 read and 8 written by k_sort_scatter = 24 through HBM; the counts add 256 x (4 written + 2 x 4
//     read + 8 written + 8 read) a tile of 4096 keys = 1.75 bytes a key.  The keys written are 8-byte stores of consecutive lanes
//     to consecutive places within a digit: a tile of uniform keys has 16 of a digit, 128 bytes a stretch.
//   instructions, k_sort_scatter: the peers 8 x (v_bfe_i32, v_cmp into a pair of SGPRs, 2 three-input operations) = 32 vector; rank and counter
//     about 10 (2 v_mbcnt, 2 v_bcnt, s_ff1, ds_read, ds_write, ds_bpermute, v_add); then an LDS read of the wave's first place, an
//     LDS write of 8 bytes, an LDS read of 8 bytes, an LDS read of the digit's place and the global store: about 60 vector and 7 LDS a
//     key.  k_sort_hist: about 10 vector and one ds_add.
//   ESTIMATE: 10^9 keys, a pass: 26 GB at the 4.7 TB/s a plain copy reaches here = 5.5 ms, 1.6 times a device-to-device copy of the
//     8 GB of keys (which moves 16 GB); 70 vector instructions a key on 39 T lane-instructions/s = 1.8 ms, beside the traffic.
//   MEASURED (profiles/kmer_wide_rate.txt; 10^9 codes of uniform random reads, events on the context's stream): 8.1 to 8.4 ms a
//     pass, 2.5 times the copy's 3.3 ms, whatever the number of passes (4 at k = 14 and 16, 6 at k = 21, 8 at k = 32: 32, 33,
//     49, 67 ms); with every fifth key one value 8.1 ms a pass, every second 7.9, all keys one value 7.5 -- never more than on
//     uniform keys.  So a pass runs at 0.65 of the estimate's rate.  (An earlier run on another device gave 8.6 to 9.0 ms
//     beside a copy of 3.4; the comparisons that follow are from that run and its like.)
//   What binds it.  Not the counts: a form in which a workgroup took its tiles one after the other and carried the digits' places
//     along in LDS (256 counts a workgroup instead of a tile, 1000 times fewer) was built and took 10.6 ms a pass where the form
//     of that day took 9.3, its scatter kernel at 168 VGPRs and 3 waves a SIMD.  Not the peers' instructions alone: with 2
//     v_cndmask and 2 v_and a bit in the place of the two three-input operations, and the peers in the histogram kernel too, a
//     pass took 9.3 to 9.5 ms against 8.6 to 9.0.  What is left is k_sort_scatter's chain of five barriers a tile with 4 waves a
//     SIMD (100 VGPRs, 39 KiB of LDS) to hide it, and the stores' 128-byte stretches, of which a line's other half belongs to
//     another tile.  A wider tile a workgroup (longer stretches, fewer barriers a key) is the next thing to try.
//
// This file stands outside the evidence set of profiles/ (profiles/check.py hashes csrc/*.hip); its kernels have no entry in the
// profiler's name table and are timed with events on the context's stream (tools/kmer_wide_rate.py).
#include "dx_internal.hpp"
#include "dx_device.hpp"

extern "C" {
#include "dx_host.h"
}

#define SORT_BITS   8u
#define SORT_DIGITS (1u << SORT_BITS)
#define SORT_ITEMS  16u                               // keys a thread
#define SORT_WAVE   (64u * SORT_ITEMS)                // keys a wave: 1024 consecutive ones
#define SORT_TILE   (DX_BLOCK * SORT_ITEMS)           // keys a workgroup
#define SORT_NMAX   (1ull << 36)

static_assert(SORT_DIGITS == DX_BLOCK, "thread d of a workgroup owns digit d");

__device__ __forceinline__ uint32_t sort_digit(uint64_t key, uint32_t shift) { return (uint32_t) (key >> shift) & (SORT_DIGITS - 1u); }

// the lanes among `live` that hold the digit this lane holds (this lane among them, if it is live)
__device__ __forceinline__ uint64_t sort_peers(uint32_t d, uint64_t live)
{ uint32_t lo = (uint32_t) live, hi = (uint32_t) (live >> 32);
  #pragma unroll
  for (uint32_t b = 0; b < SORT_BITS; b++)
    { const uint32_t all = (uint32_t) ((int32_t) (d << (31u - b)) >> 31);         // bit b of the digit in every bit: v_bfe_i32
      const uint64_t has = __ballot(all != 0u);
      lo &= ~((uint32_t) has ^ all); hi &= ~((uint32_t) (has >> 32) ^ all);       // has where the bit is set, ~has where it is not: v_bitop3
    }
  return lo | ((uint64_t) hi << 32);
}

__device__ __forceinline__ uint32_t sort_below(uint64_t m)      // the set lanes of m below this one
{ return __builtin_amdgcn_mbcnt_hi((uint32_t) (m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m, 0u)); }

// count[d * tiles + t] = the keys of tile t whose digit is d
__global__ __launch_bounds__(DX_BLOCK)
void k_sort_hist(const uint64_t *__restrict__ keys, uint64_t n, uint32_t shift, uint64_t tiles, uint32_t *__restrict__ count)
{ __shared__ uint32_t s_cnt[SORT_DIGITS];
  s_cnt[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t lane = (uint32_t) lane_id(), wave = threadIdx.x / DX_WAVE;
  const uint64_t i0   = (uint64_t) blockIdx.x * SORT_TILE + (uint64_t) wave * SORT_WAVE + lane;
  #pragma unroll 4
  for (uint32_t j = 0; j < SORT_ITEMS; j++)
    { const uint64_t i    = i0 + 64u * j;
      const bool     have = i < n;
      const uint32_t d    = have ? sort_digit(keys[i], shift) : 0u;
      const uint64_t live = __ballot(have);
      if (live == 0ull) continue;                                          // (uniform)
      const uint32_t lead = (uint32_t) __ffsll((unsigned long long) live) - 1u, d0 = __builtin_amdgcn_readlane(d, lead);
      if (__ballot(have && d != d0) == 0ull)                               // one digit in all 64: one add of 64, not 64 adds that queue
        { if (lane == lead) atomicAdd(s_cnt + d0, (uint32_t) __popcll(live)); }
      else if (have) atomicAdd(s_cnt + d, 1u);
    }
  __syncthreads();
  count[(uint64_t) threadIdx.x * tiles + blockIdx.x] = s_cnt[threadIdx.x];
}

// first: dx_scan_u32 of the counts.  src and dst hold n keys each and are not the same array.
__global__ __launch_bounds__(DX_BLOCK)
void k_sort_scatter(const uint64_t *__restrict__ src, uint64_t *__restrict__ dst, uint64_t n, uint32_t shift, uint64_t tiles,
                    const uint64_t *__restrict__ first)
{ __shared__ uint64_t s_key[SORT_TILE];
  __shared__ uint64_t s_to[SORT_DIGITS];                                  // digit d's keys go to s_to[d] + their place in the tile
  __shared__ uint32_t s_cnt[DX_WAVES_PER_BLK][SORT_DIGITS];               // a wave's counts a digit; then what the waves before it hold
  __shared__ uint32_t s_wave[DX_WAVES_PER_BLK];
  const uint32_t lane = (uint32_t) lane_id(), wave = threadIdx.x / DX_WAVE;
  const uint64_t t0   = (uint64_t) blockIdx.x * SORT_TILE;
  const uint32_t here = n - t0 < SORT_TILE ? (uint32_t) (n - t0) : SORT_TILE;          // the tile's keys (the grid has no tile without one)
  #pragma unroll
  for (uint32_t w = 0; w < DX_WAVES_PER_BLK; w++) s_cnt[w][threadIdx.x] = 0u;
  __syncthreads();

  // the wave's keys, 64 at a time, and each one's rank among the wave's keys of its digit
  uint64_t key[SORT_ITEMS];
  uint32_t rank[SORT_ITEMS];
  uint32_t *mine = s_cnt[wave];
  #pragma unroll
  for (uint32_t j = 0; j < SORT_ITEMS; j++)
    { const uint32_t p    = wave * SORT_WAVE + 64u * j + lane;
      const bool     have = p < here;
      key[j] = have ? src[t0 + p] : 0ull;
      const uint32_t d     = sort_digit(key[j], shift);
      const uint64_t m     = sort_peers(d, __ballot(have));
      const uint32_t below = sort_below(m);
      uint32_t old = 0u;
      if (have && below == 0u)                                            // the leader: nobody else of this step asks for counter d
        { old = mine[d];
          mine[d] = old + (uint32_t) __popcll(m);
        }
      wave_sync();
      const int leader = have ? __ffsll((unsigned long long) m) - 1 : (int) lane;
      rank[j] = (uint32_t) __shfl((int) old, leader) + below;
    }
  __syncthreads();

  // thread d: digit d's keys a wave become the places of the waves' first keys of d in the tile's order
  { const uint32_t d = threadIdx.x;
    uint32_t c[DX_WAVES_PER_BLK], all = 0u;
    #pragma unroll
    for (uint32_t w = 0; w < DX_WAVES_PER_BLK; w++) { c[w] = s_cnt[w][d]; all += c[w]; }
    const uint32_t incl = wave_incl_scan(all);
    if (lane == 63u) s_wave[wave] = incl;
    __syncthreads();
    uint32_t at = incl - all;
    for (uint32_t w = 0; w < wave; w++) at += s_wave[w];
    s_to[d] = first[(uint64_t) d * tiles + blockIdx.x] - at;             // (modulo 2^64: the place p >= at is added again)
    #pragma unroll
    for (uint32_t w = 0; w < DX_WAVES_PER_BLK; w++) { s_cnt[w][d] = at; at += c[w]; }
  }
  __syncthreads();

  #pragma unroll
  for (uint32_t j = 0; j < SORT_ITEMS; j++)
    if (wave * SORT_WAVE + 64u * j + lane < here)
      s_key[s_cnt[wave][sort_digit(key[j], shift)] + rank[j]] = key[j];   // (below `here`: the ranks of `here` keys)
  __syncthreads();

  #pragma unroll
  for (uint32_t j = 0; j < SORT_ITEMS; j++)
    { const uint32_t p = j * DX_BLOCK + threadIdx.x;
      if (p < here)
        { const uint64_t v = s_key[p];
          dst[s_to[sort_digit(v, shift)] + p] = v;                        // (below n: the counts of all tiles sum to n)
        }
    }
}

extern "C" int dx_sort_u64(dx_ctx *ctx, uint64_t *d_keys, uint64_t *d_tmp, uint64_t n, uint32_t bits)
{ if (ctx == NULL) return DX_E_ARG;
  if (bits > 64u) return dx_fail(ctx, DX_E_ARG, "dx_sort_u64: keys of %u bits (0 to 64)", bits);
  if (n >= SORT_NMAX) return dx_fail(ctx, DX_E_ARG, "dx_sort_u64: %llu keys (fewer than 2^36)", (unsigned long long) n);
  if (n && (d_keys == NULL || d_tmp == NULL)) return dx_fail(ctx, DX_E_ARG, "dx_sort_u64: NULL device pointer");
  if (n == 0 || bits == 0u) return DX_OK;
  DX_HIP(ctx, hipSetDevice(ctx->device));
  int rc = dx_after_pending(ctx);
  if (rc != DX_OK) return rc;

  const uint64_t tiles = (n + SORT_TILE - 1u) / SORT_TILE, cells = tiles * SORT_DIGITS;
  uint64_t *d_first = NULL;                                // cells + 1 sums, and the cells' counts behind them
  if ((rc = dx_scratch(ctx, (cells + 1u) * 8u + cells * 4u, (void **) &d_first)) != DX_OK) return rc;
  uint32_t *d_count = (uint32_t *) (d_first + cells + 1u);
  uint64_t *src = d_keys, *dst = d_tmp;
  for (uint32_t shift = 0; shift < bits; shift += SORT_BITS)
    { hipLaunchKernelGGL(k_sort_hist, dim3((unsigned) tiles), dim3(DX_BLOCK), 0, ctx->stream, (const uint64_t *) src, n, shift, tiles, d_count);
      DX_HIP(ctx, hipGetLastError());
      if ((rc = dx_scan_u32(ctx, d_count, cells, d_first, NULL)) != DX_OK) return rc;
      hipLaunchKernelGGL(k_sort_scatter, dim3((unsigned) tiles), dim3(DX_BLOCK), 0, ctx->stream, (const uint64_t *) src, dst, n, shift, tiles,
                         (const uint64_t *) d_first);
      DX_HIP(ctx, hipGetLastError());
      uint64_t *t = src; src = dst; dst = t;
    }
  if (src != d_keys) DX_HIP(ctx, hipMemcpyAsync(d_keys, src, n * 8u, hipMemcpyDeviceToDevice, ctx->stream));
  DX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return DX_OK;
}
