// dx_kmers.hip -- the k-mers of packed reads, counted where the reads lie, and what a table of such counts holds.
//
//   dx_code_kmers     per unit of a .bps / .arw / .dexta / .dexar payload: every window of k symbols adds one to its cell   (k_kmers)
//   dx_kmer_spectrum  how many cells hold 1, 2, 3 ... ; how many hold anything; the largest and its code                       (k_kmer_spectrum)
//   dx_kmer_list      the cells from a count on, in code order                                                                 (k_kmer_tiles, k_kmer_list)
//
// Nothing is decoded.  A unit is what it is for dx_code_counts and dx_code_find: symbols [beg, beg + len) of the packed read at
// in + boff, symbol i in byte i >> 2 at bits 7 - 2 (i & 3), 6 - 2 (i & 3) (DB.c:319-338), any byte offset, any phase.  The code of
// a k-mer is its symbols as a base-4 number, the first on top -- the top 2 k bits of the 64 bits that dx_find.hip holds for a
// position, and k <= 14 keeps it in the upper 32.  The table is addressed by it: 4^k cells of 64 bits, ADDED to.
//
// The walk is kc_walk (kmers/dx_kmer_windows.hpp, which says how it goes, with that header's geometry: KC_LANE, KC_GROUP, KC_CHUNK,
// KC_TARGET, KC_BATCH): the waves draw tickets and take a ticket's units 64 a round, a lane reading one unit's
// parameters and checking its bounds; a unit is walked in chunks of 16 packed bytes = 64 positions on 16-byte boundaries of the
// buffer -- up to KC_LANE chunks by its lane, up to UNITS_GROUP four units a step by 16 lanes each, the others by the whole wave.
// What is done with a chunk stands here (km_take, km_count: 32-bit words, k <= 14), and the walk's hook after every step does the
// sweeps.  A lane holds its chunk and the 4 bytes behind it (a window that begins in the chunk ends there at the latest) as five 32-bit
// words in the read's bit order, moved up to the first position that is the unit's.  It takes 8 positions at a time: a position's
// window is one funnel shift of the two upper words, its code one shift down, and after the eight the words move up 16 bits.
// Only positions p with beg <= p and p + k <= beg + len are taken, so the symbols in front of the unit, those behind it, the pad
// bits and every foreign byte are part of no window.  Nothing outside [0, in_bytes) is read (last16_ask, units_begin's pad).
//
// Canonical.  A window counts under min(code, rc), rc the codes 3 - c in reverse order.  Two forms were written down:
//   * from the window alone: v_bfrev, the two bits of every pair exchanged (2 shifts, v_bfi), complement and mask (v_bitop3 / v_not,
//     v_and): 6 to 7 instructions a position;
//   * a second register that rolls the reverse strand along: rc(p + 1) = rc(p) >> 2 | (3 - s) << (2 k - 2) with s the symbol that
//     entered, the code's two lowest bits: v_lshrrev, v_bitop3 ((~code) & 3), v_lshl_or: 3 a position, and v_min_u32 either way.
// The rolling form is built; the first form (km_rc) starts it, once a chunk.
//
// Counting.  A lane merges equal consecutive k-mers before it adds: a run of r >= k equal symbols gives r - k + 1 equal k-mers
// in a row (raw reads are full of homopolymers), one compare a position turns them into one add of r - k + 1.  Two routes:
//   1. k <= KM_LDS_K = 7: the table stands in LDS as 32-bit cells, counted into with ds_add_u32, and leaves at the kernel's end,
//      the non-zero cells as 64-bit global adds.  4^7 cells are 64 KiB: two workgroups a CU, eight waves, which this kernel --
//      bound by its own instructions and the LDS, not by waiting for HBM -- lives with; k = 7 on the global route would put every
//      add of the machine on the 2048 lines of a 128 KiB table, the contended shape (MI355X: every adder on few rows, 14 x
//      slower).  k = 8 would take 256 KiB.  Below k = 6 a cell stands several times (4096 / 4^k copies, 64 at most, side by side:
//      copy lane & (copies - 1)), as k_byte_hist's bins do, so that 64 lanes on 4 or 16 cells do not queue on one address.
//      A wave that has taken KM_FLUSH windows since it last did so empties all the workgroup's cells into the global ones
//      (atomic exchange against zero, no barrier): four waves add little more than 4 x 2^29 between two sweeps, so no cell passes
//      2^32.  DEXGPU_TEST=kmer_flush=<windows> lowers the figure for a test.
//   2. k >= 8: global_atomic_add_x2 without return, one a distinct consecutive k-mer, a lane a request.
//
// Cost, counted from the compiled code (hipcc -O3 --offload-arch=gfx950 --save-temps; the unrolled full block of km_count):
//   vector instructions a position, global route: 4.6 for a window that equals the one before it, 8.6 for one that is sent off;
//   canonical 8.6 and 12.6 --
//     the window and its code 2 (v_alignbit, v_lshrrev); canonical + 4 (v_lshrrev, v_bitop3 for (~code) & 3, v_lshl_or, v_min_u32);
//     the compare 1 (v_cmp_ne), the run count 1 (v_add); where it differs, the add: v_lshl_add_u64 for the cell's address, 3 v_mov
//     (the count's upper word, prev, run) and the global_atomic_add_x2 itself; + 0.6 for the 5 funnel shifts that move the words
//     up, a block of eight; and 4 to 6 scalar a position for the exec mask around the add (s_or, s_and_saveexec, s_cbranch_execz,
//     s_or exec).
//   LDS route: the same with v_lshlrev, v_lshl_add_u32 for the cell's word, 2 v_mov and ds_add_u32 in the atomic's place.
//   Atomic requests: one a distinct consecutive k-mer -- on uniform random symbols 1 - 4^-k of the windows, all of them in effect.
//   ESTIMATE for the global route, from the guide's figure for float atomics of the same shape (64 lanes in 64 different rows:
//   0.08 TB/s of added dwords = 20 G requests/s chip-wide): 10^9 windows at k = 14 in about 50 ms, 20 G windows/s; the
//   instructions alone (9 to 13 a position; 256 CUs x 4 SIMDs x 2.4 GHz x 16 lanes a cycle = 39 T lane-instructions/s) would
//   allow 0.3 ms, and the walk's bytes (0.25 GB) less.  So the estimate is: bound by the atomic requests, by two orders.
//   MEASURED (profiles/kmer_rate.txt; 10^5 reads x 10 kb of uniform symbols, events on the context's stream): 54.9 ms and 18.2 G
//   requests/s at k = 14, 42 ms and 23.7 G requests/s at k = 8 and 11, canonical the same -- the estimate holds within 10 to 20 %, and
//   the route is 120 to 160 times dx_code_counts' 0.34 ms over the same units.  The LDS route: 0.53 ms at k = 4, 0.73 ms at k = 7
//   (0.83 canonical), 1.6 to 2.4 times that floor.  The merge is worth 5 % at k = 14 on reads whose symbols repeat with p = 0.5 (a
//   window repeats only when k + 1 symbols in a row are equal); it is there for the homopolymers' hot cells.  What would lift the
//   global route is fewer, fuller requests -- partition the codes by their upper bits, then count a partition in LDS.
//
// The spectrum and the list are streaming passes over the table, 2 GiB at most, bound by HBM.  The spectrum's bins stand in LDS
// (KM_BINS at most; the few cells beyond go to the global words directly) and leave once a workgroup; a workgroup's (cells in use,
// largest count, its smallest code) go to a place of its own, and the host folds them: one read-back.  The list's order must be the
// same on every call, so nothing is placed by an atomic cursor: k_kmer_tiles counts a tile's cells that pass, dx_scan_u32 turns the
// counts into every tile's first place, k_kmer_list goes over the tiles again and writes, none at cap or beyond.
//
// This file stands outside the evidence set of profiles/ (profiles/check.py hashes csrc/*.hip); its kernels have no entry in
// the profiler's name table and are timed with events on the context's stream (tools/kmer_rate.py).
#include "kmers/dx_kmer_windows.hpp"
#include "tiles/dx_tiles.hpp"

#define KM_KMAX    14u                     // 4^14 cells of 8 bytes: 2 GiB
#define KM_LDS_K   7u                      // up to here the table stands in LDS
#define KM_WORDS   4096u                   // LDS words a table takes at least: 4096 / 4^k copies of a cell ...
#define KM_COPIES  64u                     // ... and so many at most
#define KM_BLOCK   8u                      // positions between two moves of the words
#define KM_FLUSH   (1ull << 29)            // windows a wave takes between two sweeps of the workgroup's cells
#define KM_BINS    4096u                   // bins of the spectrum that stand in LDS
#define KM_EVEN    0x55555555u


// ---------------------------------------------------------------------------------------------
//  k_kmers
// ---------------------------------------------------------------------------------------------
// the 4 bytes at byte o of the buffer as a word in the read's bit order; what lies behind the buffer's end reads as zero, and
// the 4 bytes that would reach past it are its last 4, moved up (bytes >= 16)
__device__ __forceinline__ uint32_t km_be32(const uint8_t *in, uint64_t bytes, uint64_t o)
{ if (o + 4u <= bytes) return __builtin_bswap32(*(const u32_u *) (in + o));
  if (o >= bytes) return 0u;
  return __builtin_bswap32(*(const u32_u *) (in + (bytes - 4u))) << (8u * (uint32_t) (o + 4u - bytes));
}

// What a lane has of a unit in one chunk: n windows begin in it, and the five words are the buffer from the first of them on
struct km_part { uint32_t r0, r1, r2, r3, r4, n; };

// the chunk at byte a < bytes of the buffer against the unit that is symbols [S0, S1) of the buffer; n == 0: no window begins here
__device__ __forceinline__ km_part km_take(const uint8_t *in, uint64_t bytes, uint64_t a, uint64_t S0, uint64_t S1, uint32_t k)
{ km_part p = { 0u, 0u, 0u, 0u, 0u, 0u };
  const uint64_t p0 = S0 > 4u * a ? S0 : 4u * a, p1 = S1 < 4u * a + KC_CHUNK ? S1 : 4u * a + KC_CHUNK;
  if (p1 <= p0 || S1 - p0 < k) return p;
  const uint32_t most = (uint32_t) (S1 - p0) - k + 1u;                        // windows from p0 on (a unit has fewer than 2^31 symbols)
  p.n = most < (uint32_t) (p1 - p0) ? most : (uint32_t) (p1 - p0);
  const u32x4    v    = last16_ask(in, bytes, a);
  const uint32_t back = (uint32_t) (a - last16_from(a, bytes));              // 0, or how many bytes in front of a the 16 begin
  uint64_t w0 = __builtin_bswap64(v.x | ((uint64_t) v.y << 32)), w1 = __builtin_bswap64(v.z | ((uint64_t) v.w << 32)), w2 = 0ull;
  if (back == 0u)      w2 = (uint64_t) km_be32(in, bytes, a + 16u) << 32;
  else if (back < 8u)  { w0 = (w0 << (8u * back)) | (w1 >> (64u - 8u * back)); w1 <<= 8u * back; }
  else                 { w0 = w1 << (8u * (back - 8u)); w1 = 0ull; }
  uint32_t s = (uint32_t) (p0 - 4u * a);                                       // the words move up to position p0
  if (s >= 32u) { w0 = w1; w1 = w2; w2 = 0ull; s -= 32u; }
  if (s)
    { w0 = (w0 << (2u * s)) | (w1 >> (64u - 2u * s));
      w1 = (w1 << (2u * s)) | (w2 >> (64u - 2u * s));
      w2 <<= 2u * s;
    }
  p.r0 = (uint32_t) (w0 >> 32); p.r1 = (uint32_t) w0; p.r2 = (uint32_t) (w1 >> 32); p.r3 = (uint32_t) w1; p.r4 = (uint32_t) (w2 >> 32);
  return p;
}

// the reverse complement's code of the window that stands in the top 2 k bits of w: the bits reversed put symbol i at bits
// 2 i + 1, 2 i with its two bits exchanged; they are exchanged back, complemented, and what stood below the window is masked off
__device__ __forceinline__ uint32_t km_rc(uint32_t w, uint32_t k)
{ const uint32_t y = __builtin_bitreverse32(w);
  return ~(((y >> 1) & KM_EVEN) | ((y & KM_EVEN) << 1)) & ((1u << (2u * k)) - 1u);
}

// where the counts go: cell `code` of the workgroup's table in LDS (this lane's copy of it: cell << shift from lds on), or of the
// global table
struct km_sink { uint32_t *lds; unsigned long long *table; uint32_t shift; bool each; };

template <bool LDS>
__device__ __forceinline__ void km_emit(const km_sink &S, uint32_t code, uint32_t run)
{ if (LDS) atomicAdd(S.lds + (code << S.shift), run);
  else     atomicAdd(S.table + code, (unsigned long long) run);
}

// one position: w has its window on top.  prev has been seen run times in a row; a code that differs sends them off
template <bool CANON, bool LDS>
__device__ __forceinline__ void km_step(const km_sink &S, uint32_t w, uint32_t down, uint32_t top, uint32_t &rcw, uint32_t &prev, uint32_t &run)
{ uint32_t cur = w >> down;
  if (CANON)
    { rcw = (rcw >> 2) | ((~cur & 3u) << top);
      cur = cur < rcw ? cur : rcw;
    }
  if (cur != prev || S.each)
    { km_emit<LDS>(S, prev, run);
      prev = cur; run = 0u;
    }
  run++;
}

// the part's windows, KM_BLOCK positions between two moves of the words
template <bool CANON, bool LDS>
__device__ __forceinline__ void km_count(const km_part &p, uint32_t k, const km_sink &S)
{ if (p.n == 0u) return;
  uint32_t r0 = p.r0, r1 = p.r1, r2 = p.r2, r3 = p.r3, r4 = p.r4;
  const uint32_t down = 32u - 2u * k, top = 2u * k - 2u;
  uint32_t prev = r0 >> down, run = 0u, rcw = 0u;          // (the first position finds its own code waiting: nothing is sent off for it)
  if (CANON)
    { const uint32_t rc = km_rc(r0, k);
      rcw = rc << 2;                                        // (the first step moves it down again and sets the top symbol it has already)
      prev = prev < rc ? prev : rc;
    }
  for (uint32_t b0 = 0; b0 < p.n; b0 += KM_BLOCK)
    { const uint32_t here = p.n - b0;
      if (here >= KM_BLOCK)
        { km_step<CANON, LDS>(S, r0, down, top, rcw, prev, run);
          #pragma unroll
          for (uint32_t s = 1; s < KM_BLOCK; s++)
            km_step<CANON, LDS>(S, (r0 << (2u * s)) | (r1 >> (32u - 2u * s)), down, top, rcw, prev, run);
        }
      else
        { km_step<CANON, LDS>(S, r0, down, top, rcw, prev, run);
          #pragma unroll
          for (uint32_t s = 1; s < KM_BLOCK - 1u; s++)
            if (s < here) km_step<CANON, LDS>(S, (r0 << (2u * s)) | (r1 >> (32u - 2u * s)), down, top, rcw, prev, run);
        }
      r0 = (r0 << 16) | (r1 >> 16); r1 = (r1 << 16) | (r2 >> 16); r2 = (r2 << 16) | (r3 >> 16);
      r3 = (r3 << 16) | (r4 >> 16); r4 <<= 16;
    }
  km_emit<LDS>(S, prev, run);
}

// every cell of the workgroup taken (exchanged against zero) and added to the global cells, by one wave
__device__ __forceinline__ void km_sweep(uint32_t *s_tab, uint32_t cells, uint32_t shift, unsigned long long *table, uint32_t lane)
{ for (uint32_t b = lane; b < cells; b += 64u)
    { unsigned long long s = 0;
      for (uint32_t c = 0; c < (1u << shift); c++) s += atomicExch(s_tab + ((b << shift) | c), 0u);
      if (s) atomicAdd(table + b, s);
    }
}

// in holds in_bytes bytes and 16 at least; the units are checked against `bound` (as in k_code_counts).  table: 4^k cells the
// windows are added to; windows: one word, which gets sum max(0, len - k + 1) over the good units.  LDS: 4^k << shift words of
// dynamic LDS; each: nothing is merged (a measurement's switch).
template <bool CANON, bool LDS>
__global__ __launch_bounds__(DX_BLOCK)
void k_kmers(const uint8_t *__restrict__ in, uint64_t in_bytes, uint64_t bound, const uint64_t *__restrict__ boff,
             const uint32_t *__restrict__ beg, const uint32_t *__restrict__ len, uint64_t n, uint32_t k, uint32_t shift,
             uint32_t each, uint64_t flush_at, unsigned long long *__restrict__ table, unsigned long long *__restrict__ windows,
             unsigned long long *__restrict__ bad, uint32_t *__restrict__ ticket)
{ extern __shared__ uint32_t s_tab[];
  const uint32_t cells = 1u << (2u * k);
  if (LDS)
    { for (uint32_t c = threadIdx.x; c < (cells << shift); c += DX_BLOCK) s_tab[c] = 0u;
      __syncthreads();
    }

  const uint32_t lane = (uint32_t) lane_id();
  km_sink S;
  S.lds = s_tab + (lane & ((1u << shift) - 1u)); S.table = table; S.shift = shift; S.each = each != 0u;
  uint64_t win = 0, counted = 0;           // the windows of the units this lane has read; (LDS) an upper bound of what the wave has taken since its last sweep
  units_rounds<false>(ticket, ticket_units_of(ticket, KC_BATCH), n, [&](uint64_t u0, uint64_t r1)
    { // unit u0 + lane is this lane's to read and to check
      const packed_unit pu = packed_unit_take(boff, beg, len, u0 + lane, r1, bound, bad);
      const kc_unit     e  = kc_unit_of(pu, k);
      const kc_place    at = { 0ull, 0u };
      if (e.nch) win += pu.len - k + 1u;
      // (LDS) the wave sweeps as soon as it has taken flush_at windows, and a step of the walk adds 64 KC_LANE KC_CHUNK = 2^14 at the
      // most: a wave adds fewer than KM_FLUSH + 2^14 between two sweeps of its own, and what a cell holds was added since the last
      // sweep of any wave, which is no earlier than any wave's own last -- below 4 (2^29 + 2^14) < 2^32 for the four waves.
      kc_walk(e, at, [&](uint64_t a, const kc_unit &u, const kc_place &)
        { km_count<CANON, LDS>(km_take(in, in_bytes, a, u.S0, u.S1, k), k, S); },
        [&](uint32_t chunks)
        { counted += chunks * KC_CHUNK;
          if (LDS && counted >= flush_at)
            { km_sweep(s_tab, cells, shift, table, lane);
              counted = 0;
            }
        });
    });

  win = wave_sum64(win);
  if (lane == 0u && win) atomicAdd(windows, (unsigned long long) win);
  if (LDS)
    { __syncthreads();
      for (uint32_t b = threadIdx.x; b < cells; b += DX_BLOCK)
        { unsigned long long s = 0;
          for (uint32_t c = 0; c < (1u << shift); c++) s += s_tab[(b << shift) | c];
          if (s) atomicAdd(table + b, s);
        }
    }
}

// ---------------------------------------------------------------------------------------------
//  k_kmer_spectrum
// ---------------------------------------------------------------------------------------------
// spec: nspec words (nspec 0: none) the workgroups add their bins to; per: a tile_figures a workgroup
__global__ __launch_bounds__(DX_BLOCK)
void k_kmer_spectrum(const unsigned long long *__restrict__ table, uint64_t cells, uint32_t nspec,
                     unsigned long long *__restrict__ spec, tile_figures *__restrict__ per)
{ __shared__ uint32_t     s_bin[KM_BINS];
  __shared__ tile_figures s_g[DX_WAVES_PER_BLK];
  spectrum_begin(nspec, KM_BINS, s_bin);

  tile_figures g = { 0ull, 0ull, 0ull };
  const uint64_t stride = (uint64_t) gridDim.x * DX_BLOCK;
  for (uint64_t c = (uint64_t) blockIdx.x * DX_BLOCK + threadIdx.x; c < cells; c += stride)
    { const unsigned long long v = table[c];
      if (v == 0ull) continue;
      figures_note(g, v, c);                               // (a lane's codes ascend)
      spectrum_bin(v, nspec, KM_BINS, s_bin, spec);
    }
  figures_fold(g, s_g, per);
  spectrum_flush(nspec, KM_BINS, s_bin, spec);
}

// ---------------------------------------------------------------------------------------------
//  k_kmer_tiles, k_kmer_list
// ---------------------------------------------------------------------------------------------
// tile t is cells [TL_TILE t, TL_TILE (t + 1)), thread x of its workgroup has cells 8 x .. 8 x + 7 of it
__global__ __launch_bounds__(DX_BLOCK)
void k_kmer_tiles(const unsigned long long *__restrict__ table, uint64_t cells, uint64_t min_count, uint32_t *__restrict__ count)
{ __shared__ uint32_t s_n[DX_WAVES_PER_BLK];
  const uint64_t c0 = (uint64_t) blockIdx.x * TL_TILE + TL_ITEMS * threadIdx.x;
  uint32_t mine = 0;
  #pragma unroll
  for (uint32_t j = 0; j < TL_ITEMS; j++)
    if (c0 + j < cells && table[c0 + j] >= min_count) mine++;
  const uint32_t all = tile_total(mine, s_n);
  if (threadIdx.x == 0u) count[blockIdx.x] = all;
}

// start: every tile's first place in the list (dx_scan_u32 of the counts); an entry is 16 bytes: count (8), code (4), 0 (4)
__global__ __launch_bounds__(DX_BLOCK)
void k_kmer_list(const unsigned long long *__restrict__ table, uint64_t cells, uint64_t min_count,
                 const uint64_t *__restrict__ start, u32x4_u *__restrict__ out, uint64_t cap)
{ __shared__ uint32_t s_n[DX_WAVES_PER_BLK];
  uint64_t first;
  if (tile_idle(start, blockIdx.x, cap, first)) return;
  const uint64_t c0 = (uint64_t) blockIdx.x * TL_TILE + TL_ITEMS * threadIdx.x;
  unsigned long long v[TL_ITEMS];
  uint32_t mine = 0;
  #pragma unroll
  for (uint32_t j = 0; j < TL_ITEMS; j++)
    { v[j] = c0 + j < cells ? table[c0 + j] : 0ull;
      if (c0 + j < cells && v[j] >= min_count) mine++;
    }
  uint64_t at = tile_place(mine, first, s_n);
  #pragma unroll
  for (uint32_t j = 0; j < TL_ITEMS; j++)
    if (c0 + j < cells && v[j] >= min_count)
      tile_put(at, cap, [&](uint64_t to)
        { u32x4 e;
          e.x = (uint32_t) v[j]; e.y = (uint32_t) (v[j] >> 32); e.z = (uint32_t) (c0 + j); e.w = 0u;
          out[to] = e;
        });
}

// ---------------------------------------------------------------------------------------------
//  the entry points
// ---------------------------------------------------------------------------------------------
static_assert(sizeof(dx_kmer) == 16 && sizeof(dx_kmers) == 48 && sizeof(tile_figures) == 24, "an entry of the list is one 16-byte store");

template <bool CANON, bool LDS>
static int km_launch(dx_ctx *ctx, int grid, size_t lds, const uint8_t *d_in, uint64_t in_bytes, uint64_t bound, const uint64_t *d_boff,
                     const uint32_t *d_beg, const uint32_t *d_len, uint64_t n, uint32_t k, uint32_t shift, uint32_t each,
                     uint64_t flush, uint64_t *d_table, const units_frame &f)
{ if (lds > (32u << 10))                                  // (64 KiB: k = 7)
    DX_HIP(ctx, hipFuncSetAttribute((const void *) k_kmers<CANON, LDS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
  hipLaunchKernelGGL((k_kmers<CANON, LDS>), dim3(grid), dim3(DX_BLOCK), lds, ctx->stream, d_in, in_bytes, bound, d_boff, d_beg, d_len, n,
                     k, shift, each, flush, (unsigned long long *) d_table, f.out, f.bad, f.ticket);
  return DX_OK;
}

extern "C" int dx_code_kmers(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes,
                             const uint64_t *d_boff, const uint32_t *d_beg, const uint32_t *d_len, uint64_t n,
                             uint32_t k, int canonical, uint64_t *d_table, uint64_t *windows, uint64_t *bad_unit)
{ if (ctx == NULL) return DX_E_ARG;
  if (bad_unit) *bad_unit = UINT64_MAX;
  if (windows) *windows = 0;
  if (k < 1u || k > KM_KMAX) return dx_fail(ctx, DX_E_ARG, "dx_code_kmers: k = %u (1 to %u)", k, KM_KMAX);
  if (d_table == NULL) return dx_fail(ctx, DX_E_ARG, "dx_code_kmers: NULL table");
  if (n >= (1ull << 31)) return dx_fail(ctx, DX_E_ARG, "dx_code_kmers: more than 2^31 - 1 units in one batch");
  if (n == 0) return DX_OK;
  units_frame    f;
  uint64_t       back[UF_OUT + 4];
  const uint64_t bound = in_bytes;                         // (the kernel loads 16 bytes at a time: fewer are copied, zeros behind them)
  int rc = units_begin(ctx, "dx_code_kmers", n, d_boff && d_len && (d_in || !in_bytes), ctx->d_u64 + DXW_UNITS, 4, 16, &d_in, &in_bytes, &f);
  if (rc != DX_OK) return rc;

  const bool     lds    = k <= KM_LDS_K;
  const uint32_t cells  = 1u << (2u * k);
  uint32_t       shift  = 0;                               // log2 of the copies a cell has in LDS
  while (lds && (cells << (shift + 1u)) <= KM_WORDS && (2u << shift) <= KM_COPIES) shift++;
  const size_t   bytes  = lds ? (size_t) (cells << shift) * sizeof(uint32_t) : 0;
  const uint32_t each   = dx_test_num("kmer_merge", 1) == 0;                 // (tools/kmer_rate.py: what the merge is worth)
  long long      flush  = dx_test_num("kmer_flush", (long long) KM_FLUSH);   // (tests: the cells swept from this many windows on)
  if (flush < 1 || flush > (long long) KM_FLUSH) flush = (long long) KM_FLUSH;
  const int      grid   = dx_grid_waves(ctx, n, bytes > (32u << 10) ? 8 : 16);
  kc_tickets(ctx, d_boff, n, f);
  if (canonical) rc = lds ? km_launch<true, true>(ctx, grid, bytes, d_in, in_bytes, bound, d_boff, d_beg, d_len, n, k, shift, each, (uint64_t) flush, d_table, f)
                          : km_launch<true, false>(ctx, grid, bytes, d_in, in_bytes, bound, d_boff, d_beg, d_len, n, k, shift, each, (uint64_t) flush, d_table, f);
  else           rc = lds ? km_launch<false, true>(ctx, grid, bytes, d_in, in_bytes, bound, d_boff, d_beg, d_len, n, k, shift, each, (uint64_t) flush, d_table, f)
                          : km_launch<false, false>(ctx, grid, bytes, d_in, in_bytes, bound, d_boff, d_beg, d_len, n, k, shift, each, (uint64_t) flush, d_table, f);
  if (rc != DX_OK) return rc;
  rc = units_end(ctx, f, back, bad_unit, "%s: unit %llu does not lie inside the %llu packed bytes", bound);
  if (windows) *windows = back[UF_OUT];
  return rc;
}

extern "C" int dx_kmer_spectrum(dx_ctx *ctx, const uint64_t *d_table, uint32_t k, uint64_t *spectrum, uint32_t nspec,
                                uint64_t *distinct, uint64_t *max_count, uint32_t *max_code)
{ if (ctx == NULL) return DX_E_ARG;
  if (k < 1u || k > KM_KMAX) return dx_fail(ctx, DX_E_ARG, "dx_kmer_spectrum: k = %u (1 to %u)", k, KM_KMAX);
  if (d_table == NULL) return dx_fail(ctx, DX_E_ARG, "dx_kmer_spectrum: NULL table");
  if (spectrum != NULL && nspec < 2u) return dx_fail(ctx, DX_E_ARG, "dx_kmer_spectrum: a spectrum of %u bins (2 at least)", nspec);
  if (spectrum == NULL) nspec = 0;
  DX_HIP(ctx, hipSetDevice(ctx->device));
  int rc = dx_after_pending(ctx);
  if (rc != DX_OK) return rc;
  const uint64_t cells = 1ull << (2u * k);
  const int      grid  = dx_grid_waves(ctx, (cells + 63u) / 64u, 8);
  uint64_t      *d_w   = NULL, mc = 0;
  if ((rc = dx_scratch(ctx, figures_words(nspec, grid) * 8u, (void **) &d_w)) != DX_OK) return rc;
  if (nspec) DX_HIP(ctx, hipMemsetAsync(d_w, 0, (size_t) nspec * 8u, ctx->stream));
  hipLaunchKernelGGL(k_kmer_spectrum, dim3(grid), dim3(DX_BLOCK), 0, ctx->stream, (const unsigned long long *) d_table, cells, nspec,
                     (unsigned long long *) d_w, (tile_figures *) (d_w + nspec));
  DX_HIP(ctx, hipGetLastError());
  if ((rc = figures_read(ctx, d_w, nspec, grid, spectrum, distinct, max_count, &mc)) != DX_OK) return rc;
  if (max_code) *max_code = (uint32_t) mc;
  return DX_OK;
}

extern "C" int dx_kmer_list(dx_ctx *ctx, const uint64_t *d_table, uint32_t k, uint64_t min_count, dx_kmer *d_out, uint64_t cap,
                            uint64_t *found)
{ if (ctx == NULL) return DX_E_ARG;
  if (found) *found = 0;
  if (k < 1u || k > KM_KMAX) return dx_fail(ctx, DX_E_ARG, "dx_kmer_list: k = %u (1 to %u)", k, KM_KMAX);
  if (d_table == NULL || found == NULL || (d_out == NULL && cap)) return dx_fail(ctx, DX_E_ARG, "dx_kmer_list: NULL pointer");
  if (min_count < 1u) return dx_fail(ctx, DX_E_ARG, "dx_kmer_list: min_count 0 (1 at least: the unseen codes are not listed)");
  DX_HIP(ctx, hipSetDevice(ctx->device));
  int rc = dx_after_pending(ctx);
  if (rc != DX_OK) return rc;
  const uint64_t cells = 1ull << (2u * k), tiles = (cells + TL_TILE - 1u) / TL_TILE;
  tiles_layout   l;
  bool           list = false;
  if ((rc = tiles_scratch(ctx, 0, tiles, false, &l)) != DX_OK) return rc;
  hipLaunchKernelGGL(k_kmer_tiles, dim3((unsigned) tiles), dim3(DX_BLOCK), 0, ctx->stream, (const unsigned long long *) d_table, cells,
                     min_count, l.pass);
  if ((rc = tiles_places(ctx, l, tiles, cap, found, &list)) != DX_OK) return rc;
  if (list)
    { hipLaunchKernelGGL(k_kmer_list, dim3((unsigned) tiles), dim3(DX_BLOCK), 0, ctx->stream, (const unsigned long long *) d_table, cells,
                         min_count, (const uint64_t *) l.start, (u32x4_u *) d_out, cap);
      DX_HIP(ctx, hipGetLastError());
      DX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
  return DX_OK;
}

// dx_host.h: dx_file_kmers.c's refusals, worded there
extern "C" int dx_kmers_fail(dx_ctx *ctx, int code, const char *what)
{ if (ctx == NULL) return code;
  return dx_fail(ctx, code, "dx_file_kmers: %s", what);
}
