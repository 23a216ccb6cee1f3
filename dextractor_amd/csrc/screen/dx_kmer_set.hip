// dx_kmer_set.hip -- a set of k-mers that stays on the device, 1 <= k <= 32, for dx_code_kmer_screen (dx_screen.hip) to ask.
//
//   dx_sorted_take            a SORTED device array (what dx_sort_u64 leaves) -> the first key of every run of min_count keys at least
//   dx_kmer_set_from_sorted   ... and those codes as a set: dx_sorted_take counts them, then fills an array of exactly that size
//   dx_kmer_set_from_codes    host codes, any order, repeats allowed: folded (canonical), uploaded, sorted, then the above
//   dx_kmer_set_info / _codes / _free
//   dx_kmer_set_from_sorted_counted   the same codes with each one's run length beside it: a COUNTED set (d_count)
//   dx_kmer_set_from_kmers            host (code, count) pairs, any order, equal codes adding: a counted set
//   dx_kmer_set_counted / _counts
//
//   k_set_take    tile t (TL_TILE = 2048 keys): the first key of every run of min_count keys at least -- counted (the tile's word),
//                 then, the places known from dx_scan_u32 of the counts, written to its place
//   k_set_index   one thread a bucket: first[b] = the lower bound of b << (2 k - p) in the codes
//   k_set_split   entry i of a list of (code, count) pairs -> codes[i] and count[i] = min(count, 2^32 - 1)
//
// The set is n distinct codes in ascending order and a bucket index over the top p bits of the 2 k-bit code: first[0 .. 2^p], 32-bit
// places, first[2^p] = n.  p is the smallest value with 2^p >= 2 n, so that a bucket holds half a code on the average and the
// screen's look-up is two dependent loads and one compare; it is clamped to [1, min(2 k, 26)] (26: 256 MiB of index), beyond which
// the buckets grow and the look-up searches them.  DEXGPU_TEST=set_bits=<p> forces p (clamped the same way) for a test.
//
// In a sorted array key i begins a run if i == 0 or key[i] != key[i - 1], and the run has min_count keys at least exactly if
// key[i + min_count - 1] is there and equal to key[i]: no run is measured, and a run may be longer than any tile.  Nothing is placed
// by an atomic cursor: the places come from the tiles' counts and a prefix sum, as in k_run_list, so the array is the same on every
// call.  k_set_index has a thread a bucket and a binary search each; nothing races.
//
// A counted set keeps n 32-bit counts beside the codes, count[i] of codes[i], saturated; the screen kernels never read them, the depth
// kernel (dx_screen_depth.hip) reads count[place] of a window that is in the set.  The runs of a sorted array are measured by nobody
// here: dx_kmer_runs (kmers/dx_kmer_runs.hip: tile_first_head, tile_run_ends, k_run_list) lists them as (code, count) pairs in
// ascending code order, the same bytes on every call, and k_set_split parts the pairs into the two arrays (ks_take_counted); the
// codes are the first keys of the runs of min_count keys at least, which is what k_set_take writes.  dx_kmer_set_from_kmers sorts
// and adds its pairs on the HOST (std::sort: the list is the host's, made once a set, and dx_sort_u64 moves keys alone), then
// uploads the two arrays.
//
// Cost: 8 bytes read a key twice (the count, the take), 8 written a code, 4 a bucket and log2 n dependent loads for it; all of it once a
// set, beside a sort of the same keys.  MEASURED with the codes and the sort of the sequence (profiles/screen_rate.txt, first call):
// 1.2 ms for 4.8 x 10^4 codes, 6.1 ms for 5 x 10^6, 116 ms for 10^8 (six sort passes and 2^26 binary searches).
//
// This file stands outside the evidence set of profiles/ (profiles/check.py hashes csrc/*.hip); its kernels have no entry in the
// profiler's name table and are timed with events on the context's stream (tools/screen_rate.py).
#include "tiles/dx_tiles.hpp"
#include "screen/dx_kmer_set.hpp"

#include <algorithm>
#include <new>

#define KS_KMAX       32u
#define KS_COUNT_MAX  0xffffffffu              // where a set's counts saturate

// ---------------------------------------------------------------------------------------------
//  k_set_take
// ---------------------------------------------------------------------------------------------
// WRITE false: pass[t] = the runs of min_count keys at least that begin in tile t.  WRITE true: their first keys to out, from
// start[t] on (the exclusive sums of the counts), in the order of the keys, none at cap or beyond.  (need = min_count - 1 < n.)
template <bool WRITE>
__global__ __launch_bounds__(DX_BLOCK)
void k_set_take(const uint64_t *__restrict__ key, uint64_t n, uint64_t need, uint32_t *__restrict__ pass,
                const uint64_t *__restrict__ start, uint64_t *__restrict__ out, uint64_t cap)
{ __shared__ uint32_t s_n[DX_WAVES_PER_BLK];
  const uint64_t i0 = (uint64_t) blockIdx.x * TL_TILE + (uint64_t) TL_ITEMS * threadIdx.x;
  uint64_t v[TL_ITEMS];
  bool     take[TL_ITEMS];
  uint32_t mine = 0;
  uint64_t prev = i0 && i0 < n ? key[i0 - 1u] : 0ull;
  #pragma unroll
  for (uint32_t j = 0; j < TL_ITEMS; j++)
    { const uint64_t i = i0 + j;
      const bool have = i < n;
      v[j] = have ? key[i] : 0ull;
      take[j] = have && (i == 0u || v[j] != prev) && need < n - i && (need == 0u || key[i + need] == v[j]);
      mine += take[j] ? 1u : 0u;
      prev = v[j];
    }
  if (!WRITE)
    { const uint32_t all = tile_total(mine, s_n);
      if (threadIdx.x == 0u) pass[blockIdx.x] = all;
      return;
    }
  uint64_t at = tile_place(mine, start[blockIdx.x], s_n);
  #pragma unroll
  for (uint32_t j = 0; j < TL_ITEMS; j++)
    if (take[j]) tile_put(at, cap, [&](uint64_t to) { out[to] = v[j]; });
}

// ---------------------------------------------------------------------------------------------
//  k_set_index
// ---------------------------------------------------------------------------------------------
// first[b], b = 0 .. 2^p: the codes in front of the first one >= b << shift (shift = 2 k - p < 64); first[2^p] = n
__global__ __launch_bounds__(DX_BLOCK)
void k_set_index(const uint64_t *__restrict__ code, uint32_t n, uint32_t bits, uint32_t shift, uint32_t *__restrict__ first)
{ const uint64_t b = (uint64_t) blockIdx.x * DX_BLOCK + threadIdx.x, buckets = 1ull << bits;
  if (b > buckets) return;
  uint32_t lo = 0, hi = n;
  if (b == buckets) lo = n;
  else
    { const uint64_t target = b << shift;
      while (lo < hi)
        { const uint32_t mid = lo + (hi - lo) / 2u;
          if (code[mid] < target) lo = mid + 1u; else hi = mid;
        }
    }
  first[b] = lo;
}

// ---------------------------------------------------------------------------------------------
//  k_set_split
// ---------------------------------------------------------------------------------------------
// list: n entries of 16 bytes as k_run_list leaves them, code (8), count (8); one 16-byte load, an 8-byte and a 4-byte store a thread
__global__ __launch_bounds__(DX_BLOCK)
void k_set_split(const u32x4_u *__restrict__ list, uint64_t n, uint64_t *__restrict__ code, uint32_t *__restrict__ count)
{ const uint64_t i = (uint64_t) blockIdx.x * DX_BLOCK + threadIdx.x;
  if (i >= n) return;
  const u32x4 e = list[i];
  code[i] = e.x | ((uint64_t) e.y << 32);
  count[i] = e.w ? KS_COUNT_MAX : e.z;
}

// ---------------------------------------------------------------------------------------------
//  the entry points
// ---------------------------------------------------------------------------------------------
static_assert(sizeof(dx_set_info) == 32, "dx_set_info is 32 bytes");
static_assert(sizeof(dx_kmer64) == 16, "k_set_split reads an entry of the list in one 16-byte load");

// what every maker asks of k, canonical and arrow: in dxf_kmers_args' words
static int ks_args(dx_ctx *ctx, const char *who, uint32_t k, int canonical, int arrow)
{ if (canonical && arrow) return dx_fail(ctx, DX_E_ARG, "%s: canonical: pulse widths have no complement (DX_KIND_FASTA only)", who);
  if (k < 1u || k > KS_KMAX) return dx_fail(ctx, DX_E_ARG, "%s: k = %u (1 to %u)", who, k, KS_KMAX);
  return DX_OK;
}

// p for a set of n codes of 2 k bits: the smallest with 2^p >= 2 n, or what DEXGPU_TEST=set_bits says, in [1, min(2 k, KS_BITS_MAX)]
static uint32_t ks_bits(uint64_t n, uint32_t k)
{ const uint32_t most = 2u * k < KS_BITS_MAX ? 2u * k : KS_BITS_MAX;
  long long p = 1;
  while (p < 40 && (1ull << p) < 2u * n) p++;
  p = dx_test_num("set_bits", p);
  return p < 1 ? 1u : (p > (long long) most ? most : (uint32_t) p);
}

extern "C" int dx_kmer_set_free(dx_ctx *ctx, dx_kmer_set *set)
{ if (ctx == NULL) return DX_E_ARG;
  if (set == NULL) return DX_OK;
  DX_HIP(ctx, hipSetDevice(ctx->device));
  if (set->d_codes) (void) hipFree(set->d_codes);
  if (set->d_first) (void) hipFree(set->d_first);
  if (set->d_count) (void) hipFree(set->d_count);
  delete set;
  return DX_OK;
}

extern "C" int dx_sorted_take(dx_ctx *ctx, const uint64_t *d_sorted, uint64_t n, uint64_t min_count, uint64_t *d_out, uint64_t cap,
                              uint64_t *found)
{ const char *who = "dx_sorted_take";
  if (ctx == NULL) return DX_E_ARG;
  if (found) *found = 0;
  if (found == NULL || (d_sorted == NULL && n) || (d_out == NULL && cap)) return dx_fail(ctx, DX_E_ARG, "%s: NULL pointer", who);
  if (min_count < 1u) return dx_fail(ctx, DX_E_ARG, "%s: min_count 0 (1 at least: the unseen codes are in no set)", who);
  if (n >= TL_NMAX) return dx_fail(ctx, DX_E_ARG, "%s: %llu keys (fewer than 2^36)", who, (unsigned long long) n);
  DX_HIP(ctx, hipSetDevice(ctx->device));
  int rc = dx_after_pending(ctx);
  if (rc != DX_OK) return rc;

  // the runs that pass, a tile: counted, and summed to every tile's first place
  const uint64_t tiles = (n + TL_TILE - 1u) / TL_TILE, need = min_count - 1u;
  tiles_layout   l;
  bool           list = false;
  if (n == 0 || need >= n) return DX_OK;
  if ((rc = tiles_scratch(ctx, 0, tiles, false, &l)) != DX_OK) return rc;
  hipLaunchKernelGGL(k_set_take<false>, dim3((unsigned) tiles), dim3(DX_BLOCK), 0, ctx->stream, d_sorted, n, need, l.pass,
                     (const uint64_t *) NULL, (uint64_t *) NULL, (uint64_t) 0);
  if ((rc = tiles_places(ctx, l, tiles, cap, found, &list)) != DX_OK) return rc;
  if (list)
    { hipLaunchKernelGGL(k_set_take<true>, dim3((unsigned) tiles), dim3(DX_BLOCK), 0, ctx->stream, d_sorted, n, need, (uint32_t *) NULL,
                         (const uint64_t *) l.start, d_out, cap);
      DX_HIP(ctx, hipGetLastError());
      DX_HIP(ctx, hipStreamSynchronize(ctx->stream));      // (the caller may free d_sorted; the scratch is free again)
    }
  return DX_OK;
}

// a set of `found` codes with its arrays made and nothing in them yet: *set, the caller's to fill, to index (ks_index) or to free
static int ks_new(dx_ctx *ctx, const char *who, uint64_t found, uint32_t k, int canonical, int arrow, bool counted, dx_kmer_set **set)
{ if (found >= KS_NMAX)
    return dx_fail(ctx, DX_E_ARG, "%s: %llu codes in the set (fewer than 2^32 - 1)", who, (unsigned long long) found);
  dx_kmer_set *s = new (std::nothrow) dx_kmer_set();
  if (s == NULL) return dx_fail(ctx, DX_E_NOMEM, "%s: out of memory", who);
  s->k = k; s->canonical = canonical ? 1u : 0u; s->arrow = arrow ? 1u : 0u; s->n = found;
  s->bits = ks_bits(found, k);
  const uint64_t buckets = 1ull << s->bits;
  s->device_bytes = found * (counted ? 12u : 8u) + (buckets + 1u) * 4u;
  int rc;
  if ((rc = dx_malloc(ctx, (size_t) found * 8u + 64u, (void **) &s->d_codes)) != DX_OK ||
      (rc = dx_malloc(ctx, (size_t) (buckets + 1u) * 4u + 64u, (void **) &s->d_first)) != DX_OK ||
      (counted && (rc = dx_malloc(ctx, (size_t) found * 4u + 64u, (void **) &s->d_count)) != DX_OK))
    { (void) dx_kmer_set_free(ctx, s);                     // (dx_malloc has left the words)
      return rc;
    }
  *set = s;
  return DX_OK;
}

// the bucket index over the set's codes, which are in place; the stream is waited for (the caller may free what the codes came from)
static int ks_index(dx_ctx *ctx, const char *who, dx_kmer_set *s)
{ const uint64_t buckets = 1ull << s->bits;
  hipLaunchKernelGGL(k_set_index, dim3((unsigned) ((buckets + 1u + DX_BLOCK - 1u) / DX_BLOCK)), dim3(DX_BLOCK), 0, ctx->stream,
                     (const uint64_t *) s->d_codes, (uint32_t) s->n, s->bits, 2u * s->k - s->bits, s->d_first);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  return e == hipSuccess ? DX_OK : dx_fail(ctx, DX_E_HIP, "%s: %s", who, hipGetErrorString(e));
}

// what dx_kmer_set_from_sorted and dx_kmer_set_from_sorted_counted ask of their arguments
static int ks_sorted_args(dx_ctx *ctx, const char *who, const uint64_t *d_sorted, uint64_t n, uint64_t min_count, uint32_t k, int canonical,
                          int arrow)
{ const int rc = ks_args(ctx, who, k, canonical, arrow);
  if (rc != DX_OK) return rc;
  if (d_sorted == NULL && n) return dx_fail(ctx, DX_E_ARG, "%s: NULL pointer", who);
  if (min_count < 1u) return dx_fail(ctx, DX_E_ARG, "%s: min_count 0 (1 at least: the unseen codes are in no set)", who);
  if (n >= TL_NMAX) return dx_fail(ctx, DX_E_ARG, "%s: %llu keys (fewer than 2^36)", who, (unsigned long long) n);
  return DX_OK;
}

// dx_host.h: dx_sorted_take with every kept run's length beside its first key.  The runs are dx_kmer_runs': listed as 16-byte pairs
// into d_tmp when the pairs fit its tmp_words words, into a block of their own otherwise, and parted by k_set_split.  cap == 0 counts.
extern "C" int dx_sorted_take_counted(dx_ctx *ctx, const uint64_t *d_sorted, uint64_t n, uint64_t min_count, void *d_tmp, uint64_t tmp_words,
                                      uint64_t *d_codes, uint32_t *d_count, uint64_t cap, uint64_t *found)
{ int rc = dx_kmer_runs(ctx, d_sorted, n, min_count, NULL, 0, found, NULL, 0, NULL, NULL, NULL);
  if (rc != DX_OK || cap == 0 || *found == 0) return rc;
  if (d_codes == NULL || d_count == NULL || cap < *found) return dx_fail(ctx, DX_E_ARG, "dx_sorted_take_counted: room for fewer than the runs");
  const uint64_t have = *found;
  void *d_own = NULL;
  if (d_tmp == NULL || 2u * have > tmp_words)
    { if ((rc = dx_malloc(ctx, (size_t) have * sizeof(dx_kmer64) + 64u, &d_own)) != DX_OK) return rc;
      d_tmp = d_own;
    }
  uint64_t again = 0;
  if ((rc = dx_kmer_runs(ctx, d_sorted, n, min_count, (dx_kmer64 *) d_tmp, have, &again, NULL, 0, NULL, NULL, NULL)) == DX_OK)
    { hipLaunchKernelGGL(k_set_split, dim3((unsigned) ((have + DX_BLOCK - 1u) / DX_BLOCK)), dim3(DX_BLOCK), 0, ctx->stream,
                         (const u32x4_u *) d_tmp, have, d_codes, d_count);
      hipError_t e = hipGetLastError();
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);          // (the pairs' block is freed; the caller may free d_sorted)
      if (e != hipSuccess) rc = dx_fail(ctx, DX_E_HIP, "dx_sorted_take_counted: %s", hipGetErrorString(e));
    }
  if (d_own) (void) dx_free(ctx, d_own);
  return rc;
}

// the two makers' one body: counted first, so that the set's arrays have exactly the size (the tiles are read once more when they
// are filled: 8 bytes a key, beside a sort)
static int ks_from_sorted(dx_ctx *ctx, const char *who, const uint64_t *d_sorted, uint64_t n, uint64_t min_count, uint32_t k, int canonical,
                          int arrow, bool counted, dx_kmer_set **set)
{ if (ctx == NULL) return DX_E_ARG;
  if (set == NULL) return dx_fail(ctx, DX_E_ARG, "%s: NULL pointer", who);
  *set = NULL;
  int rc = ks_sorted_args(ctx, who, d_sorted, n, min_count, k, canonical, arrow);
  if (rc != DX_OK) return rc;
  DX_HIP(ctx, hipSetDevice(ctx->device));

  uint64_t found = 0, again = 0;
  dx_kmer_set *s = NULL;
  if ((rc = dx_sorted_take(ctx, d_sorted, n, min_count, NULL, 0, &found)) != DX_OK) return rc;
  if ((rc = ks_new(ctx, who, found, k, canonical, arrow, counted, &s)) != DX_OK) return rc;
  if (found && counted) rc = dx_sorted_take_counted(ctx, d_sorted, n, min_count, NULL, 0, s->d_codes, s->d_count, found, &again);
  else if (found)       rc = dx_sorted_take(ctx, d_sorted, n, min_count, s->d_codes, found, &again);
  if (rc == DX_OK && again != found) rc = dx_fail(ctx, DX_E_HIP, "%s: the runs counted twice differ", who);
  if (rc == DX_OK) rc = ks_index(ctx, who, s);
  if (rc != DX_OK) { (void) dx_kmer_set_free(ctx, s); return rc; }
  *set = s;
  return DX_OK;
}

extern "C" int dx_kmer_set_from_sorted(dx_ctx *ctx, const uint64_t *d_sorted, uint64_t n, uint64_t min_count, uint32_t k, int canonical,
                                       int arrow, dx_kmer_set **set)
{ return ks_from_sorted(ctx, "dx_kmer_set_from_sorted", d_sorted, n, min_count, k, canonical, arrow, false, set); }

extern "C" int dx_kmer_set_from_sorted_counted(dx_ctx *ctx, const uint64_t *d_sorted, uint64_t n, uint64_t min_count, uint32_t k,
                                               int canonical, int arrow, dx_kmer_set **set)
{ return ks_from_sorted(ctx, "dx_kmer_set_from_sorted_counted", d_sorted, n, min_count, k, canonical, arrow, true, set); }

// dx_host.h: the counted set of n distinct ascending codes and their counts that stand on the device already (dx_files_kmer_set_counted's
// ranges, one behind the other): copied into arrays of the set's own, then indexed
extern "C" int dx_kmer_set_from_counted(dx_ctx *ctx, const uint64_t *d_codes, const uint32_t *d_count, uint64_t n, uint32_t k, int canonical,
                                        int arrow, dx_kmer_set **set)
{ const char *who = "dx_files_kmer_set_counted";
  dx_kmer_set *s = NULL;
  *set = NULL;
  int rc = ks_new(ctx, who, n, k, canonical, arrow, true, &s);
  if (rc != DX_OK) return rc;
  if (n && ((rc = dx_d2d(ctx, s->d_codes, d_codes, (size_t) n * 8u)) != DX_OK || (rc = dx_d2d(ctx, s->d_count, d_count, (size_t) n * 4u)) != DX_OK))
    { (void) dx_kmer_set_free(ctx, s); return rc; }
  if ((rc = ks_index(ctx, who, s)) != DX_OK) { (void) dx_kmer_set_free(ctx, s); return rc; }
  *set = s;
  return DX_OK;
}

// the code of the reverse complement of a code of k symbols (host)
static uint64_t ks_rc(uint64_t code, uint32_t k)
{ uint64_t out = 0;
  for (uint32_t i = 0; i < k; i++)
    out = (out << 2) | (3u - ((code >> (2u * i)) & 3u));
  return out;
}

extern "C" int dx_kmer_set_from_codes(dx_ctx *ctx, const uint64_t *codes, uint64_t n, uint32_t k, int canonical, int arrow,
                                      dx_kmer_set **set)
{ const char *who = "dx_kmer_set_from_codes";
  if (ctx == NULL) return DX_E_ARG;
  if (set == NULL) return dx_fail(ctx, DX_E_ARG, "%s: NULL pointer", who);
  *set = NULL;
  int rc = ks_args(ctx, who, k, canonical, arrow);
  if (rc != DX_OK) return rc;
  if (codes == NULL && n) return dx_fail(ctx, DX_E_ARG, "%s: NULL pointer", who);
  if (n >= TL_NMAX) return dx_fail(ctx, DX_E_ARG, "%s: %llu codes (fewer than 2^36)", who, (unsigned long long) n);
  if (n == 0) return dx_kmer_set_from_sorted(ctx, NULL, 0, 1, k, canonical, arrow, set);

  std::vector<uint64_t> own;
  if (k < KS_KMAX)
    for (uint64_t i = 0; i < n; i++)
      if (codes[i] >> (2u * k))
        return dx_fail(ctx, DX_E_ARG, "%s: code %llu has bits above its %u symbols", who, (unsigned long long) i, k);
  if (canonical)
    { own.assign(codes, codes + n);
      for (uint64_t i = 0; i < n; i++)
        { const uint64_t r = ks_rc(own[i], k);
          if (r < own[i]) own[i] = r;
        }
      codes = own.data();
    }
  void *d_keys = NULL, *d_tmp = NULL;
  if ((rc = dx_malloc(ctx, (size_t) n * 8u + 64u, &d_keys)) == DX_OK && (rc = dx_malloc(ctx, (size_t) n * 8u + 64u, &d_tmp)) == DX_OK &&
      (rc = dx_h2d(ctx, d_keys, codes, (size_t) n * 8u)) == DX_OK &&
      (rc = dx_sort_u64(ctx, (uint64_t *) d_keys, (uint64_t *) d_tmp, n, 2u * k)) == DX_OK)
    rc = dx_kmer_set_from_sorted(ctx, (const uint64_t *) d_keys, n, 1, k, canonical, arrow, set);
  if (d_keys) (void) dx_free(ctx, d_keys);
  if (d_tmp) (void) dx_free(ctx, d_tmp);
  return rc;
}

extern "C" int dx_kmer_set_from_kmers(dx_ctx *ctx, const dx_kmer64 *list, uint64_t n, uint32_t k, int canonical, int arrow, dx_kmer_set **set)
{ const char *who = "dx_kmer_set_from_kmers";
  if (ctx == NULL) return DX_E_ARG;
  if (set == NULL) return dx_fail(ctx, DX_E_ARG, "%s: NULL pointer", who);
  *set = NULL;
  int rc = ks_args(ctx, who, k, canonical, arrow);
  if (rc != DX_OK) return rc;
  if (list == NULL && n) return dx_fail(ctx, DX_E_ARG, "%s: NULL pointer", who);
  if (n >= TL_NMAX) return dx_fail(ctx, DX_E_ARG, "%s: %llu pairs (fewer than 2^36)", who, (unsigned long long) n);
  if (k < KS_KMAX)
    for (uint64_t i = 0; i < n; i++)
      if (list[i].code >> (2u * k))
        return dx_fail(ctx, DX_E_ARG, "%s: code %llu has bits above its %u symbols", who, (unsigned long long) i, k);
  DX_HIP(ctx, hipSetDevice(ctx->device));

  // the pairs that count, folded, in the order of their codes; then equal codes added up, in place
  std::vector<dx_kmer64> own;
  std::vector<uint64_t>  codes;
  std::vector<uint32_t>  counts;
  try
    { own.reserve((size_t) n);
      for (uint64_t i = 0; i < n; i++)
        if (list[i].count)
          { dx_kmer64 e = list[i];
            const uint64_t r = canonical ? ks_rc(e.code, k) : e.code;
            if (r < e.code) e.code = r;
            own.push_back(e);
          }
      std::sort(own.begin(), own.end(), [](const dx_kmer64 &a, const dx_kmer64 &b) { return a.code < b.code; });
      for (size_t i = 0; i < own.size(); )
        { uint64_t sum = 0;
          size_t   j = i;
          for (; j < own.size() && own[j].code == own[i].code; j++)
            sum = own[j].count >= KS_COUNT_MAX || sum + own[j].count >= KS_COUNT_MAX ? KS_COUNT_MAX : sum + own[j].count;
          codes.push_back(own[i].code); counts.push_back((uint32_t) sum);
          i = j;
        }
    }
  catch (const std::bad_alloc &) { return dx_fail(ctx, DX_E_NOMEM, "%s: out of memory", who); }

  dx_kmer_set *s = NULL;
  const uint64_t found = codes.size();
  if ((rc = ks_new(ctx, who, found, k, canonical, arrow, true, &s)) != DX_OK) return rc;
  if (found && ((rc = dx_h2d(ctx, s->d_codes, codes.data(), (size_t) found * 8u)) != DX_OK ||
                (rc = dx_h2d(ctx, s->d_count, counts.data(), (size_t) found * 4u)) != DX_OK))
    { (void) dx_kmer_set_free(ctx, s); return rc; }
  if ((rc = ks_index(ctx, who, s)) != DX_OK) { (void) dx_kmer_set_free(ctx, s); return rc; }
  *set = s;
  return DX_OK;
}

extern "C" int dx_kmer_set_info(const dx_kmer_set *set, dx_set_info *info)
{ if (set == NULL || info == NULL) return DX_E_ARG;
  info->codes = set->n; info->device_bytes = set->device_bytes;
  info->k = set->k; info->canonical = set->canonical; info->arrow = set->arrow; info->index_bits = set->bits;
  return DX_OK;
}

extern "C" int dx_kmer_set_codes(dx_ctx *ctx, const dx_kmer_set *set, uint64_t *out, uint64_t cap)
{ if (ctx == NULL) return DX_E_ARG;
  if (set == NULL || (out == NULL && cap)) return dx_fail(ctx, DX_E_ARG, "dx_kmer_set_codes: NULL pointer");
  if (cap < set->n)
    return dx_fail(ctx, DX_E_NOMEM, "dx_kmer_set_codes: %llu codes, and room for %llu", (unsigned long long) set->n, (unsigned long long) cap);
  return dx_d2h(ctx, out, set->d_codes, (size_t) set->n * 8u);
}

extern "C" int dx_kmer_set_counted(const dx_kmer_set *set)
{ return set == NULL ? DX_E_ARG : (set->d_count != NULL ? 1 : 0); }

extern "C" int dx_kmer_set_counts(dx_ctx *ctx, const dx_kmer_set *set, uint32_t *out, uint64_t cap)
{ if (ctx == NULL) return DX_E_ARG;
  if (set == NULL || (out == NULL && cap)) return dx_fail(ctx, DX_E_ARG, "dx_kmer_set_counts: NULL pointer");
  if (set->d_count == NULL) return dx_fail(ctx, DX_E_ARG, "dx_kmer_set_counts: the set is not counted (it holds codes alone)");
  if (cap < set->n)
    return dx_fail(ctx, DX_E_NOMEM, "dx_kmer_set_counts: %llu counts, and room for %llu", (unsigned long long) set->n, (unsigned long long) cap);
  return dx_d2h(ctx, out, set->d_count, (size_t) set->n * 4u);
}

// dx_host.h: dx_file_screen.c's refusals of dx_file_kmer_set, worded there
extern "C" int dx_kmer_set_fail(dx_ctx *ctx, int code, const char *what)
{ if (ctx == NULL) return code;
  return dx_fail(ctx, code, "dx_file_kmer_set: %s", what);
}
