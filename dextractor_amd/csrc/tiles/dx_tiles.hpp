// dx_tiles.hpp -- what the tile kernels share (kmers/dx_kmers, kmers/dx_kmer_runs, screen/dx_kmer_set; of screen/dx_screen_spans the
// host's side only: k_join's kernels measured slower on the shared device code and keep their own, profiles/tiles_refactor_rate.txt): a
// tile is TL_TILE consecutive items of a device array, TL_ITEMS a thread.  Three things stand here once:
//   * the tile compaction: a launch counts a tile's items that pass (tile_total), dx_scan_u32 gives every tile its first place
//     (tiles_places), a second launch writes them in order from there (tile_idle, tile_place, tile_put), none at cap or beyond and
//     nothing placed by an atomic cursor, so that a list is the same on every call;
//   * the run-head pattern: item i is a HEAD if it begins a run (the predicate is the kernel's), a heads kernel leaves every tile's
//     first head (tile_first_head), and a tile learns where the run of each of its heads ends -- at the next head, in the tile or in
//     one that follows, or at n (tile_run_ends);
//   * the figures: how many, the largest count and its smallest code (tile_figures), a spectrum whose bins stand in LDS, and the
//     host's fold of the workgroups' words (figures_read).
// What a kernel loads, which items pass and what it writes stay in its own file.  (Outside the evidence set of profiles/, as those
// files are.)
#pragma once

#include "dx_internal.hpp"
#include "dx_device.hpp"

extern "C" {
#include "dx_host.h"
}

#include <vector>

#define TL_ITEMS 8u                           // items a thread
#define TL_TILE  (DX_BLOCK * TL_ITEMS)        // items a workgroup
#define TL_NONE  0xffffffffu                  // no head
#define TL_NMAX  (1ull << 36)                 // items of an array (dx_sort_u64's bound; a tile's number fits 32 bits with room)

static_assert(DX_WAVES_PER_BLK == 4, "the sums over a workgroup's waves are written out");

// ---- the run-head pattern ------------------------------------------------------------------------------------------
// the smallest value over the workgroup (every thread gets it); s_w: a word a wave
__device__ __forceinline__ uint32_t tile_block_min(uint32_t v, uint32_t *s_w)
{
  #pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = min(v, (uint32_t) __shfl_xor((int) v, d));
  __syncthreads();                                         // (s_w may still be read from its last use)
  if (lane_id() == 0) s_w[threadIdx.x / DX_WAVE] = v;
  __syncthreads();
  return min(min(s_w[0], s_w[1]), min(s_w[2], s_w[3]));
}

// The body of a heads kernel, a workgroup a tile: first[t] = the place in tile t of its first head, TL_NONE if it has none.
// item(i) loads item i < n (the kernel's pointer keeps its type and alignment there); head(i, prev, v): item i (v; prev: item
// i - 1, zero for i == 0) is one -- asked of every item of the tile, in order.
template <typename L, typename H>
__device__ __forceinline__ void tile_first_head(uint64_t n, uint32_t *__restrict__ first, uint32_t *s_w, L &&item, H &&head)
{ typedef decltype(item(0ull)) T;
  const uint64_t i0 = (uint64_t) blockIdx.x * TL_TILE + (uint64_t) TL_ITEMS * threadIdx.x;
  const T  zero = {};
  uint32_t mine = TL_NONE;                                 // this thread's first head, as a place in the tile
  if (i0 < n)
    { T prev = i0 ? item(i0 - 1u) : zero;
      #pragma unroll
      for (uint32_t j = 0; j < TL_ITEMS; j++)
        if (i0 + j < n)
          { const T v = item(i0 + j);
            if (head(i0 + j, prev, v) && mine == TL_NONE) mine = TL_ITEMS * threadIdx.x + j;
            prev = v;
          }
    }
  const uint32_t all = tile_block_min(mine, s_w);
  if (threadIdx.x == 0u) first[blockIdx.x] = all;
}

// Tile t of n items, thread x holding items TL_TILE t + 8 x + j: head[j] says which of them are heads, mine is the first of them
// as a place in the tile (TL_NONE: none), first[] what the heads kernel left.  end(j, next) for every head, the highest j first:
// next is the index of the first head behind item j, n if there is none.  Uniform over the workgroup (it synchronises); s_f: a
// word a thread, s_w: a word a wave.
template <typename F>
__device__ __forceinline__ void tile_run_ends(uint64_t n, const uint32_t *__restrict__ first, uint64_t tiles, uint64_t t,
                                              const bool head[TL_ITEMS], uint32_t mine, uint32_t *s_f, uint32_t *s_w, F &&end)
{ const uint64_t t0 = t * TL_TILE, i0 = t0 + (uint64_t) TL_ITEMS * threadIdx.x;

  // the first head behind the tile: in the tiles that follow, 256 of them a step; n if there is none.  (A tile without a head has
  // nothing to end: first[t] is the workgroup's, so the branch is uniform.)
  uint64_t beyond = n;
  if (first[t] != TL_NONE)
    for (uint64_t b = t + 1u; b < tiles; b += DX_BLOCK)
      { const uint64_t u = b + threadIdx.x;
        const uint32_t f = u < tiles ? first[u] : TL_NONE;
        const uint32_t w = tile_block_min(f != TL_NONE ? threadIdx.x : TL_NONE, s_w);                // the nearest such tile of the 256
        if (w != TL_NONE)
          { beyond = (b + w) * TL_TILE + first[b + w];
            break;                                                                                   // (uniform: w is the workgroup's)
          }
      }

  // the first head behind this thread's items: the smallest of the threads above it
  __syncthreads();
  s_f[threadIdx.x] = mine;
  __syncthreads();
  const uint32_t lane = (uint32_t) lane_id(), wave = threadIdx.x / DX_WAVE;
  uint32_t after = lane < 63u ? s_f[threadIdx.x + 1u] : TL_NONE;                                  // the wave's lanes above, suffix minimum
  #pragma unroll
  for (uint32_t d = 1; d < 64u; d <<= 1)
    { const uint32_t o = (uint32_t) __shfl_down((int) after, d);
      if (lane + d < 64u) after = min(after, o);
    }
  const uint32_t whole = min(after, mine);                                                       // the wave's first head, in lane 0
  if (lane == 0u) s_w[wave] = whole;
  __syncthreads();
  for (uint32_t w = wave + 1u; w < DX_WAVES_PER_BLK; w++) after = min(after, s_w[w]);
  uint64_t next = after != TL_NONE ? t0 + after : beyond;
  #pragma unroll
  for (uint32_t jj = 0; jj < TL_ITEMS; jj++)
    { const uint32_t j = TL_ITEMS - 1u - jj;
      if (head[j]) { end(j, next); next = i0 + j; }
    }
  __syncthreads();                                         // (s_f, s_w: free for the next tile)
}

// ---- the tile compaction -------------------------------------------------------------------------------------------
// the workgroup's sum of the threads' counts -- thread 0 writes it to pass[t]; s_n: a word a wave
__device__ __forceinline__ uint32_t tile_total(uint32_t mine, uint32_t *s_n)
{ const uint32_t all = wave_sum(mine);
  if (lane_id() == 0) s_n[threadIdx.x / DX_WAVE] = all;
  __syncthreads();
  return s_n[0] + s_n[1] + s_n[2] + s_n[3];
}

// A listing workgroup's first place, from = start[t] (dx_scan_u32 of the tiles' counts), and whether it has nothing to write: no
// place below cap, or no item that passes.  (Uniform: the whole workgroup leaves.)
__device__ __forceinline__ bool tile_idle(const uint64_t *__restrict__ start, uint64_t t, uint64_t cap, uint64_t &from)
{ from = start[t];
  return from >= cap || start[t + 1u] == from;
}

// the place of a thread's first kept item: `from` and the kept items of the threads below it; s_n: a word a wave
__device__ __forceinline__ uint64_t tile_place(uint32_t mine, uint64_t from, uint32_t *s_n)
{ const uint32_t incl = wave_incl_scan(mine), wave = threadIdx.x / DX_WAVE;
  if (lane_id() == 63) s_n[wave] = incl;
  __syncthreads();
  uint64_t at = from + (incl - mine);
  for (uint32_t w = 0; w < wave; w++) at += s_n[w];
  return at;
}

// a kept item takes place `at`: put(at) writes it, and nothing is written at cap or beyond
template <typename P>
__device__ __forceinline__ void tile_put(uint64_t &at, uint64_t cap, P &&put)
{ if (at < cap) put(at);
  at++;
}

// ---- the figures ---------------------------------------------------------------------------------------------------
// how many counts there are (cells in use, runs), the largest, and the smallest code that has it: a thread's, then a workgroup's
struct tile_figures { unsigned long long distinct, max_count, max_code; };

// (a thread's codes ascend: of equal counts the first stays)
__device__ __forceinline__ void figures_note(tile_figures &g, unsigned long long count, unsigned long long code)
{ g.distinct++;
  if (count > g.max_count) { g.max_count = count; g.max_code = code; }
}

// the workgroup's figures, of equal counts the smaller code, to a place of its own: per[blockIdx.x]; s_g: a tile_figures a wave
__device__ __forceinline__ void figures_fold(tile_figures g, tile_figures *s_g, tile_figures *__restrict__ per)
{ unsigned long long d = g.distinct, m = g.max_count, mc = g.max_code;
  #pragma unroll
  for (int s = 32; s > 0; s >>= 1)
    { const unsigned long long om = __shfl_xor(m, s), oc = __shfl_xor(mc, s);
      d += __shfl_xor(d, s);
      if (om > m || (om == m && oc < mc)) { m = om; mc = oc; }
    }
  if (lane_id() == 0) { s_g[threadIdx.x / DX_WAVE].distinct = d; s_g[threadIdx.x / DX_WAVE].max_count = m; s_g[threadIdx.x / DX_WAVE].max_code = mc; }
  __syncthreads();
  if (threadIdx.x == 0u)
    { for (uint32_t w = 1; w < DX_WAVES_PER_BLK; w++)
        { d += s_g[w].distinct;
          if (s_g[w].max_count > m || (s_g[w].max_count == m && s_g[w].max_code < mc)) { m = s_g[w].max_count; mc = s_g[w].max_code; }
        }
      per[blockIdx.x].distinct = d; per[blockIdx.x].max_count = m; per[blockIdx.x].max_code = m ? mc : 0ull;
    }
}

// The spectrum: spec holds nspec words (nspec 0: none), the last of which gathers; its first `bins` stand in the workgroup's s_bin.
// spectrum_begin clears them, spectrum_bin adds one count (the few beyond the LDS bins go to the global words directly), and
// spectrum_flush adds the workgroup's bins to spec -- behind a barrier that follows the last spectrum_bin (figures_fold has one).
__device__ __forceinline__ void spectrum_begin(uint32_t nspec, uint32_t bins, uint32_t *s_bin)
{ const uint32_t inside = nspec < bins ? nspec : bins;
  for (uint32_t b = threadIdx.x; b < inside; b += DX_BLOCK) s_bin[b] = 0u;
  __syncthreads();
}

__device__ __forceinline__ void spectrum_bin(unsigned long long count, uint32_t nspec, uint32_t bins, uint32_t *s_bin,
                                             unsigned long long *__restrict__ spec)
{ if (nspec)
    { const uint32_t b = count < (unsigned long long) (nspec - 1u) ? (uint32_t) count : nspec - 1u;
      if (b < bins) atomicAdd(s_bin + b, 1u);
      else          atomicAdd(spec + b, 1ull);
    }
}

__device__ __forceinline__ void spectrum_flush(uint32_t nspec, uint32_t bins, const uint32_t *s_bin, unsigned long long *__restrict__ spec)
{ const uint32_t inside = nspec < bins ? nspec : bins;
  for (uint32_t b = threadIdx.x; b < inside; b += DX_BLOCK)
    if (s_bin[b]) atomicAdd(spec + b, (unsigned long long) s_bin[b]);
}

// ---- the host's side -----------------------------------------------------------------------------------------------
// One scratch block: head_words 64-bit words of the entry point's own in front, then every tile's first place in the list
// (tiles + 1), the tiles' counts and (with_first) their first heads.
struct tiles_layout
{ uint64_t *head, *start;
  uint32_t *pass, *first;
};

static int tiles_scratch(dx_ctx *ctx, size_t head_words, uint64_t tiles, bool with_first, tiles_layout *l)
{ uint64_t *d_w = NULL;
  const int rc = dx_scratch(ctx, (head_words + tiles + 1u + ((with_first ? 2u : 1u) * tiles + 1u) / 2u) * 8u, (void **) &d_w);
  if (rc != DX_OK) return rc;
  l->head = d_w; l->start = d_w + head_words;
  l->pass = (uint32_t *) (l->start + tiles + 1u); l->first = with_first ? l->pass + tiles : NULL;
  return DX_OK;
}

// Behind the counting launch: the counts summed to every tile's first place, *found what passed in all (one read-back), and *list
// whether a listing launch has anything to write.
static int tiles_places(dx_ctx *ctx, const tiles_layout &l, uint64_t tiles, uint64_t cap, uint64_t *found, bool *list)
{ DX_HIP(ctx, hipGetLastError());
  const int rc = dx_scan_u32(ctx, l.pass, tiles, l.start, found);
  *list = rc == DX_OK && cap && *found;
  return rc;
}

// the words a spectrum kernel leaves at d_w: the nspec bins, then a tile_figures a workgroup
static inline size_t figures_words(uint32_t nspec, int grid) { return (size_t) nspec + 3u * (size_t) grid; }

// ... read back in one copy (the stream synchronised) and the workgroups' figures folded (distinct, max_count, max_code: each may be NULL)
static int figures_read(dx_ctx *ctx, const uint64_t *d_w, uint32_t nspec, int grid, uint64_t *spectrum, uint64_t *distinct,
                        uint64_t *max_count, uint64_t *max_code)
{ std::vector<uint64_t> back(figures_words(nspec, grid));
  DX_HIP(ctx, hipMemcpyAsync(back.data(), d_w, back.size() * 8u, hipMemcpyDeviceToHost, ctx->stream));
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
