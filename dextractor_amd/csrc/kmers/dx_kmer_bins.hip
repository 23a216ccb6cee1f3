// dx_kmer_bins.hip -- how the k-mers of packed reads spread over the top bits of their codes, 1 <= k <= 32, and the ranges of
// codes made of that: the first step of a wide count that goes in passes (dx_files_kmers_wide, dx_file_kmers_files.c).
//
//   dx_code_kmer_bins    per unit of a .bps / .arw / .dexta / .dexar payload: every window adds one to bin `code >> (2 k - bits)`   (k_kmer_bins)
//   dx_kmer_range_plan   host: the bins cut into ranges of consecutive bins whose windows fit a pass
//
// The answer of a range of codes depends on no other range, and the order of the sorted codes is the codes': so the windows may
// be counted range after range, each range's codes (dx_code_kmer_codes_range) sorted alone, and the answers concatenate.  What a
// range costs in device memory is its windows, 16 bytes each, and that is what the bins tell: 2^bits 64-bit words, ADDED to,
// 1 <= bits <= min(2 k, 12).
//
// Units, the bounds check, *windows and *bad_unit are dx_code_kmer_codes'.  The walk is kc_walk, the chunk's words and the windows'
// codes are kc_take's and kc_roll's (all in kmers/dx_kmer_windows.hpp), the canonical code the rolling one; what is done with a
// chunk stands here (kb_count), and the walk's hook after every step does the sweeps.  Nothing outside [0, in_bytes) is read.
//
// Counting is k_kmers' LDS route: the bins stand in LDS as 32-bit cells, 16 KiB at most; below 4096 cells a cell stands several
// times (4096 / 2^bits copies, 64 at most, side by side: copy lane & (copies - 1)); a lane merges equal consecutive bins into one
// add (a homopolymer, and at few bits any stretch of reads that begin alike); a wave that has taken KB_FLUSH windows since it last
// did so sweeps all the workgroup's cells into the global words (atomic exchange against zero, no barrier), so that no cell passes
// 2^32; the rest leaves at the kernel's end, zero cells skipped.  DEXGPU_TEST=bins_flush=<windows> lowers the figure for a test.
//
// Cost, ESTIMATE (made before anything was measured): a window is kc_roll's code and step (about 10 vector instructions, 16
// canonical), one shift for the bin, a compare and an add for the merge, and a ds_add_u32 where the bin changes -- what k_kmers'
// LDS route does a position, which takes 0.53 to 0.83 ms for 10^9 positions (profiles/kmer_rate.txt).  The same order is
// expected here, beside about 60 ms for the sort of as many codes.  MEASURED (profiles/kmer_files_rate.txt, tools/kmer_files_rate.py;
// 10^5 reads x 10 kb of uniform symbols, events on the context's stream): 0.76 ms at k = 6 and at k = 21 alike, 0.90 and 0.95
// canonical, beside dx_code_kmers' 0.50 (0.61 canonical) at k = 6 and dx_code_counts' 0.27 over the same units in the same run: the
// same order, 1.5 times the LDS route -- the words that move along are 64 bits wide here, 32 there -- and 1/50 of the sort.  In
// the driver the pass costs 8.8 ms for a 0.25 GB image, of which the upload is most.
//
// This file stands outside the evidence set of profiles/ (profiles/check.py hashes csrc/*.hip); its kernel has no entry in the
// profiler's name table and is timed with events on the context's stream.
#include "kmers/dx_kmer_windows.hpp"

extern "C" {
#include "dx_host.h"
#include "dx_env.h"
}

#define KB_BITS_MAX 12u                    // 4096 cells of 32 bits: 16 KiB of LDS
#define KB_WORDS    4096u                  // LDS words the bins take at least: 4096 / 2^bits copies of a cell ...
#define KB_COPIES   64u                    // ... and so many at most
#define KB_FLUSH    (1ull << 29)           // windows a wave takes between two sweeps of the workgroup's cells

// ---------------------------------------------------------------------------------------------
//  k_kmer_bins
// ---------------------------------------------------------------------------------------------
// the part's windows into this lane's copy of the cells: cell b is lds[b << shift]
template <bool CANON>
__device__ __forceinline__ void kb_count(const kc_part &p, uint32_t k, uint32_t down, uint32_t shift, uint32_t *lds)
{ if (p.n == 0u) return;
  kc_roll<CANON> R(p, k);
  uint32_t prev = (uint32_t) (R.code() >> down), run = 1u;
  for (uint32_t i = 1; i < p.n; i++)
    { R.step();
      const uint32_t cur = (uint32_t) (R.code() >> down);
      if (cur != prev)
        { atomicAdd(lds + (prev << shift), run);
          prev = cur; run = 0u;
        }
      run++;
    }
  atomicAdd(lds + (prev << shift), run);
}

// every cell of the workgroup taken (exchanged against zero) and added to the global words, by one wave
__device__ __forceinline__ void kb_sweep(uint32_t *s_bin, uint32_t cells, uint32_t shift, unsigned long long *bins, uint32_t lane)
{ for (uint32_t b = lane; b < cells; b += 64u)
    { unsigned long long s = 0;
      for (uint32_t c = 0; c < (1u << shift); c++) s += atomicExch(s_bin + ((b << shift) | c), 0u);
      if (s) atomicAdd(bins + b, s);
    }
}

// in holds in_bytes bytes and 16 at least; the units are checked against `bound`.  bins: 2^bits words the windows are added to;
// windows: one word, which gets sum max(0, len - k + 1) over the good units.  (2^bits << shift) words of dynamic LDS.
template <bool CANON>
__global__ __launch_bounds__(DX_BLOCK)
void k_kmer_bins(const uint8_t *__restrict__ in, uint64_t in_bytes, uint64_t bound, const uint64_t *__restrict__ boff,
                 const uint32_t *__restrict__ beg, const uint32_t *__restrict__ len, uint64_t n, uint32_t k, uint32_t bits,
                 uint32_t shift, uint64_t flush_at, unsigned long long *__restrict__ bins, unsigned long long *__restrict__ windows,
                 unsigned long long *__restrict__ bad, uint32_t *__restrict__ ticket)
{ extern __shared__ uint32_t s_bin[];
  const uint32_t cells = 1u << bits, down = 2u * k - bits;
  for (uint32_t c = threadIdx.x; c < (cells << shift); c += DX_BLOCK) s_bin[c] = 0u;
  __syncthreads();

  const uint32_t lane = (uint32_t) lane_id();
  uint32_t *mine_bins = s_bin + (lane & ((1u << shift) - 1u));
  uint64_t win = 0, counted = 0;           // the windows of the units this lane has read; an upper bound of what the wave has taken since its last sweep
  units_rounds<false>(ticket, ticket_units_of(ticket, KC_BATCH), n, [&](uint64_t u0, uint64_t r1)
    { // unit u0 + lane is this lane's to read and to check
      const packed_unit pu = packed_unit_take(boff, beg, len, u0 + lane, r1, bound, bad);
      const kc_unit     e  = kc_unit_of(pu, k);
      const kc_place    at = { 0ull, 0u };
      if (e.nch) win += pu.len - k + 1u;
      // The wave sweeps as soon as it has taken flush_at windows, and a step of the walk adds 64 KC_LANE KC_CHUNK = 2^14 at the most:
      // a wave adds fewer than KB_FLUSH + 2^14 between two sweeps of its own, and what a cell holds was added since the last
      // sweep of any wave, which is no earlier than any wave's own last -- below 4 (2^29 + 2^14) < 2^32 for the four waves.
      kc_walk(e, at, [&](uint64_t a, const kc_unit &u, const kc_place &)
        { kb_count<CANON>(kc_take(in, in_bytes, a, u.S0, u.S1, k), k, down, shift, mine_bins); },
        [&](uint32_t chunks)
        { counted += chunks * KC_CHUNK;
          if (counted >= flush_at)
            { kb_sweep(s_bin, cells, shift, bins, lane);
              counted = 0;
            }
        });
    });

  win = wave_sum64(win);
  if (lane == 0u && win) atomicAdd(windows, (unsigned long long) win);
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < cells; b += DX_BLOCK)
    { unsigned long long s = 0;
      for (uint32_t c = 0; c < (1u << shift); c++) s += s_bin[(b << shift) | c];
      if (s) atomicAdd(bins + b, s);
    }
}

// ---------------------------------------------------------------------------------------------
//  the entry points
// ---------------------------------------------------------------------------------------------
extern "C" int dx_code_kmer_bins(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes,
                                 const uint64_t *d_boff, const uint32_t *d_beg, const uint32_t *d_len, uint64_t n,
                                 uint32_t k, int canonical, uint32_t bits, uint64_t *d_bins, uint64_t *windows, uint64_t *bad_unit)
{ if (ctx == NULL) return DX_E_ARG;
  if (bad_unit) *bad_unit = UINT64_MAX;
  if (windows) *windows = 0;
  if (k < 1u || k > KC_KMAX) return dx_fail(ctx, DX_E_ARG, "dx_code_kmer_bins: k = %u (1 to %u)", k, KC_KMAX);
  if (bits < 1u || bits > KB_BITS_MAX || bits > 2u * k)
    return dx_fail(ctx, DX_E_ARG, "dx_code_kmer_bins: bits = %u (1 to %u)", bits, 2u * k < KB_BITS_MAX ? 2u * k : KB_BITS_MAX);
  if (d_bins == NULL) return dx_fail(ctx, DX_E_ARG, "dx_code_kmer_bins: NULL pointer");
  if (n >= (1ull << 31)) return dx_fail(ctx, DX_E_ARG, "dx_code_kmer_bins: more than 2^31 - 1 units in one batch");
  if (n == 0) return DX_OK;
  units_frame    f;
  uint64_t       back[UF_OUT + 4];
  const uint64_t bound = in_bytes;                         // (the kernel loads 16 bytes at a time: fewer are copied, zeros behind them)
  int rc = units_begin(ctx, "dx_code_kmer_bins", n, d_boff && d_len && (d_in || !in_bytes), ctx->d_u64 + DXW_UNITS, 4, 16, &d_in, &in_bytes, &f);
  if (rc != DX_OK) return rc;

  const uint32_t cells = 1u << bits;
  uint32_t       shift = 0;                                // log2 of the copies a cell has in LDS
  while ((cells << (shift + 1u)) <= KB_WORDS && (2u << shift) <= KB_COPIES) shift++;
  const size_t   bytes = (size_t) (cells << shift) * sizeof(uint32_t);
  long long      flush = dx_test_num("bins_flush", (long long) KB_FLUSH);    // (tests: the cells swept from this many windows on)
  if (flush < 1 || flush > (long long) KB_FLUSH) flush = (long long) KB_FLUSH;
  const int      grid  = dx_grid_waves(ctx, n, 16);
  kc_tickets(ctx, d_boff, n, f);
  if (canonical) hipLaunchKernelGGL(k_kmer_bins<true>, dim3(grid), dim3(DX_BLOCK), bytes, ctx->stream, d_in, in_bytes, bound, d_boff, d_beg,
                                    d_len, n, k, bits, shift, (uint64_t) flush, (unsigned long long *) d_bins, f.out, f.bad, f.ticket);
  else           hipLaunchKernelGGL(k_kmer_bins<false>, dim3(grid), dim3(DX_BLOCK), bytes, ctx->stream, d_in, in_bytes, bound, d_boff, d_beg,
                                    d_len, n, k, bits, shift, (uint64_t) flush, (unsigned long long *) d_bins, f.out, f.bad, f.ticket);
  rc = units_end(ctx, f, back, bad_unit, "%s: unit %llu does not lie inside the %llu packed bytes", bound);
  if (windows) *windows = back[UF_OUT];
  return rc;
}

// Greedy: a range takes bins while its sum stays <= room; an empty bin costs nothing, so it joins the range in front of it.
extern "C" int dx_kmer_range_plan(dx_ctx *ctx, const uint64_t *bins, uint32_t nbins, uint64_t room, uint32_t *cut, uint32_t *ranges)
{ if (ranges) *ranges = 0;
  if (bins == NULL || cut == NULL || ranges == NULL || nbins == 0u)
    return dx_fail(ctx, DX_E_ARG, "dx_kmer_range_plan: NULL pointer, or no bins");
  uint32_t r = 0;
  uint64_t sum = 0;
  cut[0] = 0u;
  for (uint32_t b = 0; b < nbins; b++)
    { if (room && bins[b] > room)
        return dx_fail(ctx, DX_E_NOMEM, "dx_kmer_range_plan: bin %u holds %llu windows, and a pass has room for %llu", b,
                       (unsigned long long) bins[b], (unsigned long long) room);
      if (room && bins[b] > room - sum) { cut[++r] = b; sum = 0; }          // (sum <= room always: no overflow)
      sum += bins[b];
    }
  cut[++r] = nbins;
  *ranges = r;
  return DX_OK;
}

// dx_host.h: dx_file_kmers_files.c's refusals, worded there
extern "C" int dx_kmers_files_fail(dx_ctx *ctx, int code, const char *who, const char *what)
{ if (ctx == NULL) return code;
  return dx_fail(ctx, code, "%s: %s", who, what);
}

// ... and the index of the image that did not open, in front of what the walk said of it; image < 0 empties the text (a host walk
// fails without words, and what an earlier call left must not pass for them)
extern "C" int dx_kmers_files_image_fail(dx_ctx *ctx, int code, const char *who, int64_t image)
{ char was[440];
  if (ctx == NULL) return code;
  if (image < 0) { ctx->err[0] = '\0'; return code; }
  snprintf(was, sizeof(was), "%s", ctx->err);
  if (was[0] == '\0') snprintf(was, sizeof(was), "the image does not parse (error %d)", code);
  return dx_fail(ctx, code, "%s: image %lld: %s", who, (long long) image, was);
}

// ... and bytes from one device array to another, behind everything on the context's stream; the stream is waited for
extern "C" int dx_d2d(dx_ctx *ctx, void *d_dst, const void *d_src, size_t bytes)
{ if (ctx == NULL) return DX_E_ARG;
  if (bytes == 0) return DX_OK;
  DX_HIP(ctx, hipSetDevice(ctx->device));
  int rc = dx_after_pending(ctx);
  if (rc != DX_OK) return rc;
  DX_HIP(ctx, hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  DX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return DX_OK;
}
