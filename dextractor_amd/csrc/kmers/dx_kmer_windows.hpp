// dx_kmer_windows.hpp -- the windows of a packed unit, and the walk over them that nine kernels make: k_kc_codes, k_kc_range, k_kmer_bins,
// k_kmers (kmers/), k_screen, k_spans, k_depths (screen/), k_ix_keys and k_seeds (place/).
//
// The chunk.  A lane holds its chunk (16 packed bytes = 64 positions on a 16-byte boundary of the buffer) and the 8 bytes behind it
// as three 64-bit words in the read's bit order, moved up to the first position that is the unit's and at which a window begins
// (kc_take); a position's code is one shift of the upper word, the words move up two bits a position, and the reverse strand rolls
// along in a second register, started once a chunk by kc_rc (kc_roll).  Nothing outside [0, bytes) is read (last16_ask).
//
// The walk.  The waves draw tickets (kc_tickets: k_ticket_units over the units' byte offsets) and take a ticket's units 64 a round,
// a lane reading one unit's parameters and checking its bounds.  kc_unit_of makes the unit's extent in the buffer of them; a unit of
// up to KC_LANE chunks is its lane's, one of up to KC_GROUP goes four a step by 16 lanes each (kc_unit_from hands the extent to the
// group), the others go by the whole wave, 64 chunks a step (kc_unit_uniform hands it to the wave).  A kernel whose chunks do not
// depend on one another gives kc_walk what it does with a chunk; one that reduces or scans across a unit's chunks (k_kc_range,
// k_screen, k_spans, k_seeds) takes the three extent functions and keeps its own tiers.
//
// The host's side: kc_windows_places (k_kc_windows and the prefix sum: every unit's first window's place) and kc_tickets.
// (Outside the evidence set of profiles/, as the files that include it are.)
#pragma once

#include "units/dx_units.hpp"

#define KC_KMAX    32u
#define KC_BATCH   1u                      // units a ticket at least
#define KC_TARGET  (16u << 10)             // packed bytes a ticket
#define KC_CHUNK   64u                     // positions a chunk (16 packed bytes)
#define KC_LANE    4u                      // chunks: a unit of up to so many is its lane's
#define KC_GROUP   UNITS_GROUP             // chunks: up to here 16 lanes take the unit, beyond the wave
#define KC_EVEN64  0x5555555555555555ull

// ---- a unit's extent, and the walk over its chunks ---------------------------------------------------------------------
// A unit in the buffer: its symbols are [S0, S1) of the buffer's, its first chunk stands at byte a0, and it has nch chunks; all
// zero for a unit without a window
struct kc_unit { uint64_t S0, S1, a0; uint32_t nch; };

// the extent of a unit that has been taken; none for one that is not ok, is shorter than k, or is not `wanted`
__device__ __forceinline__ kc_unit kc_unit_of(const packed_unit &pu, uint32_t k, bool wanted = true)
{ kc_unit e = { 0ull, 0ull, 0ull, 0u };
  if (pu.ok && pu.len >= k && wanted)
    { const uint64_t S0 = 4u * pu.at + pu.beg, S1 = S0 + pu.len;
      const uint64_t a0 = (S0 >> 2) & ~15ull;
      e.S0 = S0; e.S1 = S1; e.a0 = a0;
      e.nch = (uint32_t) ((((S1 - 1u) >> 2) - a0) >> 4) + 1u;
    }
  return e;
}

// lane `from`'s extent, for the lanes of a group ...
__device__ __forceinline__ kc_unit kc_unit_from(const kc_unit &e, int from)
{ const kc_unit g = { __shfl(e.S0, from), __shfl(e.S1, from), __shfl(e.a0, from), __shfl(e.nch, from) };
  return g;
}

// ... and for the whole wave (from is uniform): wave-uniform values
__device__ __forceinline__ kc_unit kc_unit_uniform(const kc_unit &e, int from)
{ const kc_unit w = { uniform64(__shfl(e.S0, from)), uniform64(__shfl(e.S1, from)), uniform64(__shfl(e.a0, from)), uniform(__shfl(e.nch, from)) };
  return w;
}

// What travels with a unit: its first place in the output, and (k_ix_keys) its first symbol's global position
struct kc_place { uint64_t to; uint32_t g; };

// The walk of a round's units for a kernel whose chunks do not depend on one another.  e, at: the extent and the place of the
// unit that this lane has read.  body(a, unit, place) is called once for every chunk of every unit of the round, by the lane that
// takes the chunk at byte a; took(chunks) is called by the whole wave, in uniform control flow, after every step, with the chunks
// the wave has taken at the most (k_kmer_bins and k_kmers sweep their LDS cells by it).
template <typename F, typename G>
__device__ __forceinline__ void kc_walk(const kc_unit &e, const kc_place &at, F &&body, G &&took)
{ const uint32_t lane = (uint32_t) lane_id(), sub = lane % UNITS_GROUP;

  // up to KC_LANE chunks: the lane's own, chunk after chunk
  if (e.nch && e.nch <= KC_LANE)
    for (uint32_t j = 0; j < e.nch; j++) body(e.a0 + 16u * j, e, at);
  took(64u * KC_LANE);

  // up to 16 chunks: lanes 16 g .. 16 g + 15 take unit k + g, a chunk each
  units_by_fours(__ballot(e.nch > KC_LANE && e.nch <= KC_GROUP), [&](int from, bool mine)
    { const kc_unit  g  = kc_unit_from(e, from);
      const kc_place gp = { __shfl(at.to, from), __shfl(at.g, from) };
      if (mine && sub < g.nch) body(g.a0 + 16u * sub, g, gp);
      took(64u);
    });

  // the others: the whole wave, 64 chunks a step
  units_each(__ballot(e.nch > KC_GROUP), [&](int from)
    { const kc_unit  w  = kc_unit_uniform(e, from);
      const kc_place wp = { uniform64(__shfl(at.to, from)), uniform(__shfl(at.g, from)) };
      for (uint32_t base = 0; base < w.nch; base += 64u)
        { const uint32_t j = base + lane;
          if (j < w.nch) body(w.a0 + 16ull * j, w, wp);
          took(64u);
        }
    });
}

template <typename F>
__device__ __forceinline__ void kc_walk(const kc_unit &e, const kc_place &at, F &&body) { kc_walk(e, at, body, [](uint32_t) {}); }

// ---- the chunk -----------------------------------------------------------------------------------------------------
// What a lane has of a unit in one chunk: n windows begin in it, the first at symbol `first` of the unit, and the three words are the
// buffer from that window's first symbol on
struct kc_part { uint64_t w0, w1, w2; uint32_t n, first; };

// the chunk at byte a < bytes of the buffer against the unit that is symbols [S0, S1) of the buffer; n == 0: no window begins here
__device__ __forceinline__ kc_part kc_take(const uint8_t *in, uint64_t bytes, uint64_t a, uint64_t S0, uint64_t S1, uint32_t k)
{ kc_part p = { 0ull, 0ull, 0ull, 0u, 0u };
  const uint64_t p0 = S0 > 4u * a ? S0 : 4u * a, p1 = S1 < 4u * a + KC_CHUNK ? S1 : 4u * a + KC_CHUNK;
  if (p1 <= p0 || S1 - p0 < k) return p;
  const uint32_t most = (uint32_t) (S1 - p0) - k + 1u;                        // windows from p0 on (a unit has fewer than 2^31 symbols)
  p.n = most < (uint32_t) (p1 - p0) ? most : (uint32_t) (p1 - p0);
  p.first = (uint32_t) (p0 - S0);
  uint64_t w0, w1, w2;
  chunk_words(in, bytes, a, w0, w1, w2);
  uint32_t s = (uint32_t) (p0 - 4u * a);                                       // the words move up to position p0
  if (s >= 32u) { w0 = w1; w1 = w2; w2 = 0ull; s -= 32u; }
  if (s)
    { w0 = (w0 << (2u * s)) | (w1 >> (64u - 2u * s));
      w1 = (w1 << (2u * s)) | (w2 >> (64u - 2u * s));
      w2 <<= 2u * s;
    }
  p.w0 = w0; p.w1 = w1; p.w2 = w2;
  return p;
}

// the reverse complement's code of the window that stands in the top 2 k bits of w: the bits reversed put symbol i at bits
// 2 i + 1, 2 i with its two bits exchanged; they are exchanged back, complemented, and what stood below the window is masked off
__device__ __forceinline__ uint64_t kc_rc(uint64_t w, uint32_t k)
{ const uint64_t y = __builtin_bitreverse64(w);
  return ~(((y >> 1) & KC_EVEN64) | ((y & KC_EVEN64) << 1)) & (k < 32u ? (1ull << (2u * k)) - 1u : ~0ull);
}

// The windows of a part, one after the other: code() is the window's that stands on top, step() moves to the next.  CANON: the
// smaller of the code and its reverse complement's, compared unsigned.  (k_kc_codes' loop, kc_write, states the same steps itself.)
template <bool CANON>
struct kc_roll
{ uint64_t w0, w1, w2, rcw;
  uint32_t down, top;
  __device__ __forceinline__ kc_roll(const kc_part &p, uint32_t k) : w0(p.w0), w1(p.w1), w2(p.w2), down(64u - 2u * k), top(2u * k - 2u)
  { rcw = CANON ? kc_rc(w0, k) << 2 : 0ull; }              // (the first code() moves it down again and sets the top symbol it has already)
  __device__ __forceinline__ uint64_t code()
  { uint64_t cur = w0 >> down;
    if (CANON)
      { rcw = (rcw >> 2) | ((~cur & 3ull) << top);
        cur = cur < rcw ? cur : rcw;
      }
    return cur;
  }
  __device__ __forceinline__ void step() { w0 = (w0 << 2) | (w1 >> 62); w1 = (w1 << 2) | (w2 >> 62); w2 <<= 2; }
};

// ---- the host's side -----------------------------------------------------------------------------------------------
// w[j] = the windows of unit j: max(0, len - k + 1), 0 for a unit that does not lie inside `bound` bytes (the walk reports those)
static __global__ __launch_bounds__(DX_BLOCK)
void k_kc_windows(const uint64_t *__restrict__ boff, const uint32_t *__restrict__ beg, const uint32_t *__restrict__ len, uint64_t n,
                  uint64_t bound, uint32_t k, uint32_t *__restrict__ w)
{ const uint64_t j = (uint64_t) blockIdx.x * DX_BLOCK + threadIdx.x;
  if (j >= n) return;
  const uint32_t l = len[j];
  w[j] = packed_unit_ok(boff[j], beg != NULL ? beg[j] : 0u, l, bound) && l >= k ? l - k + 1u : 0u;
}

// every unit's windows into d_win[n], their exclusive sums -- every unit's first window's place -- into d_off[n + 1], the total
// read back.  (No ticket has been drawn yet: the first is, after the scan.)
static int kc_windows_places(dx_ctx *ctx, const uint64_t *d_boff, const uint32_t *d_beg, const uint32_t *d_len, uint64_t n, uint64_t bound,
                             uint32_t k, uint32_t *d_win, uint64_t *d_off, uint64_t *total)
{ hipLaunchKernelGGL(k_kc_windows, dim3((unsigned) ((n + DX_BLOCK - 1u) / DX_BLOCK)), dim3(DX_BLOCK), 0, ctx->stream, d_boff, d_beg, d_len, n,
                     bound, k, d_win);
  DX_HIP(ctx, hipGetLastError());
  return dx_scan_u32(ctx, d_win, n, d_off, total);
}

// the units a ticket of the walk, from the units' byte offsets, into the frame's ticket
static void kc_tickets(dx_ctx *ctx, const uint64_t *d_boff, uint64_t n, const units_frame &f)
{ hipLaunchKernelGGL(k_ticket_units, dim3(1), dim3(1), 0, ctx->stream, d_boff, d_boff + (n - 1), (const uint32_t *) NULL, n,
                     KC_TARGET, KC_BATCH, f.ticket);
}
