// dx_kmer_runs.hip -- what a sorted array of k-mer codes holds: dx_kmer_runs, the counts read off the runs of equal keys.
//
//   k_run_heads   tile t (TL_TILE = 2048 keys): the place of its first key that begins a run, or none
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
#include "tiles/dx_tiles.hpp"

#define KR_BINS  4096u                        // bins of the spectrum that stand in LDS

// first[t] = the place in tile t of its first key that begins a run, TL_NONE if it has none
__global__ __launch_bounds__(DX_BLOCK)
void k_run_heads(const uint64_t *__restrict__ key, uint64_t n, uint32_t *__restrict__ first)
{ __shared__ uint32_t s_w[DX_WAVES_PER_BLK];
  tile_first_head(n, first, s_w, [&](uint64_t i) { return key[i]; },
                  [](uint64_t i, uint64_t prev, uint64_t v) { return i == 0u || v != prev; });
}

// Tile t's keys, 8 a thread: v[j] = key TL_TILE t + 8 x + j, len[j] = the length of the run that begins there, 0 where none does.
// Uniform over the workgroup (it synchronises); s_f: a word a thread, s_w: a word a wave.
__device__ __forceinline__ void kr_tile(const uint64_t *__restrict__ key, uint64_t n, const uint32_t *__restrict__ first, uint64_t tiles,
                                        uint64_t t, uint32_t *s_f, uint32_t *s_w, uint64_t v[TL_ITEMS], uint64_t len[TL_ITEMS])
{ const uint64_t i0 = t * TL_TILE + (uint64_t) TL_ITEMS * threadIdx.x;
  bool     head[TL_ITEMS];
  uint32_t mine = TL_NONE;                                 // this thread's first begin, as a place in the tile
  uint64_t prev = i0 && i0 < n ? key[i0 - 1u] : 0ull;
  #pragma unroll
  for (uint32_t j = 0; j < TL_ITEMS; j++)
    { const bool have = i0 + j < n;
      v[j] = have ? key[i0 + j] : 0ull;
      head[j] = have && (i0 + j == 0u || v[j] != prev);
      if (head[j] && mine == TL_NONE) mine = TL_ITEMS * threadIdx.x + j;
      prev = v[j];
      len[j] = 0ull;
    }
  tile_run_ends(n, first, tiles, t, head, mine, s_f, s_w, [&](uint32_t j, uint64_t next) { len[j] = next - (i0 + j); });
}

// spec: nspec words (nspec 0: none) the workgroups add their bins to; per: a tile_figures a workgroup; pass[t]: tile t's runs of
// min_count keys at least
__global__ __launch_bounds__(DX_BLOCK)
void k_run_count(const uint64_t *__restrict__ key, uint64_t n, const uint32_t *__restrict__ first, uint64_t tiles, uint64_t min_count,
                 uint32_t nspec, unsigned long long *__restrict__ spec, tile_figures *__restrict__ per, uint32_t *__restrict__ pass)
{ __shared__ uint32_t     s_bin[KR_BINS];
  __shared__ uint32_t     s_f[DX_BLOCK], s_w[DX_WAVES_PER_BLK], s_n[DX_WAVES_PER_BLK];
  __shared__ tile_figures s_g[DX_WAVES_PER_BLK];
  spectrum_begin(nspec, KR_BINS, s_bin);

  tile_figures       g = { 0ull, 0ull, 0ull };
  unsigned long long ones = 0;
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x)
    { uint64_t v[TL_ITEMS], len[TL_ITEMS];
      kr_tile(key, n, first, tiles, t, s_f, s_w, v, len);
      uint32_t mine = 0;
      #pragma unroll
      for (uint32_t j = 0; j < TL_ITEMS; j++)
        if (len[j])
          { figures_note(g, len[j], v[j]);                   // (a thread's codes ascend, tile after tile)
            if (len[j] >= min_count) mine++;
            if (len[j] == 1ull) ones++;
            else spectrum_bin(len[j], nspec, KR_BINS, s_bin, spec);
          }
      const uint32_t all = tile_total(mine, s_n);
      if (threadIdx.x == 0u) pass[t] = all;
    }

  figures_fold(g, s_g, per);
  #pragma unroll
  for (int s = 32; s > 0; s >>= 1) ones += __shfl_xor(ones, s);
  if (lane_id() == 0 && nspec && ones) atomicAdd(spec + 1, ones);          // (nspec >= 2: bin 1 is there, and with two bins it is the one that gathers)
  spectrum_flush(nspec, KR_BINS, s_bin, spec);
}

// start: every tile's first place in the list (dx_scan_u32 of k_run_count's counts); an entry is 16 bytes: code (8), count (8)
__global__ __launch_bounds__(DX_BLOCK)
void k_run_list(const uint64_t *__restrict__ key, uint64_t n, const uint32_t *__restrict__ first, uint64_t tiles, uint64_t min_count,
                const uint64_t *__restrict__ start, u32x4_u *__restrict__ out, uint64_t cap)
{ __shared__ uint32_t s_f[DX_BLOCK], s_w[DX_WAVES_PER_BLK], s_n[DX_WAVES_PER_BLK];
  uint64_t from;
  if (tile_idle(start, blockIdx.x, cap, from)) return;
  uint64_t v[TL_ITEMS], len[TL_ITEMS];
  kr_tile(key, n, first, tiles, blockIdx.x, s_f, s_w, v, len);
  uint32_t mine = 0;
  #pragma unroll
  for (uint32_t j = 0; j < TL_ITEMS; j++)
    if (len[j] && len[j] >= min_count) mine++;
  uint64_t at = tile_place(mine, from, s_n);
  #pragma unroll
  for (uint32_t j = 0; j < TL_ITEMS; j++)
    if (len[j] && len[j] >= min_count)
      tile_put(at, cap, [&](uint64_t to)
        { u32x4 e;
          e.x = (uint32_t) v[j]; e.y = (uint32_t) (v[j] >> 32); e.z = (uint32_t) len[j]; e.w = (uint32_t) (len[j] >> 32);
          out[to] = e;
        });
}

// ---------------------------------------------------------------------------------------------
//  the entry point
// ---------------------------------------------------------------------------------------------
static_assert(sizeof(dx_kmer64) == 16 && sizeof(dx_kmers64) == 56 && sizeof(tile_figures) == 24, "an entry of the list is one 16-byte store");

extern "C" int dx_kmer_runs(dx_ctx *ctx, const uint64_t *d_sorted, uint64_t n, uint64_t min_count, dx_kmer64 *d_out, uint64_t cap,
                            uint64_t *found, uint64_t *spectrum, uint32_t nspec, uint64_t *distinct, uint64_t *max_count, uint64_t *max_code)
{ if (ctx == NULL) return DX_E_ARG;
  if (found) *found = 0;
  if (found == NULL || (d_sorted == NULL && n) || (d_out == NULL && cap)) return dx_fail(ctx, DX_E_ARG, "dx_kmer_runs: NULL pointer");
  if (min_count < 1u) return dx_fail(ctx, DX_E_ARG, "dx_kmer_runs: min_count 0 (1 at least: the unseen codes are not listed)");
  if (spectrum != NULL && nspec < 2u) return dx_fail(ctx, DX_E_ARG, "dx_kmer_runs: a spectrum of %u bins (2 at least)", nspec);
  if (n >= TL_NMAX) return dx_fail(ctx, DX_E_ARG, "dx_kmer_runs: %llu keys (fewer than 2^36)", (unsigned long long) n);
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

  // in front of the tiles' words: the spectrum and the workgroups' figures
  const uint64_t tiles = (n + TL_TILE - 1u) / TL_TILE;
  const int      grid  = dx_grid_waves(ctx, tiles * DX_WAVES_PER_BLK, 16);
  tiles_layout   l;
  bool           list  = false;
  if ((rc = tiles_scratch(ctx, figures_words(nspec, grid), tiles, true, &l)) != DX_OK) return rc;
  if (nspec) DX_HIP(ctx, hipMemsetAsync(l.head, 0, (size_t) nspec * 8u, ctx->stream));
  hipLaunchKernelGGL(k_run_heads, dim3((unsigned) tiles), dim3(DX_BLOCK), 0, ctx->stream, d_sorted, n, l.first);
  hipLaunchKernelGGL(k_run_count, dim3(grid), dim3(DX_BLOCK), 0, ctx->stream, d_sorted, n, (const uint32_t *) l.first, tiles, min_count, nspec,
                     (unsigned long long *) l.head, (tile_figures *) (l.head + nspec), l.pass);
  if ((rc = tiles_places(ctx, l, tiles, cap, found, &list)) != DX_OK) return rc;
  if (list)
    { hipLaunchKernelGGL(k_run_list, dim3((unsigned) tiles), dim3(DX_BLOCK), 0, ctx->stream, d_sorted, n, (const uint32_t *) l.first, tiles,
                         min_count, (const uint64_t *) l.start, (u32x4_u *) d_out, cap);
      DX_HIP(ctx, hipGetLastError());
    }
  return figures_read(ctx, l.head, nspec, grid, spectrum, distinct, max_count, max_code);
}

// dx_host.h: dx_file_kmers_wide.c's refusals, worded there
extern "C" int dx_kmers_wide_fail(dx_ctx *ctx, int code, const char *what)
{ if (ctx == NULL) return code;
  return dx_fail(ctx, code, "dx_file_kmers_wide: %s", what);
}
