// dx_kmer_windows.hpp -- a chunk of a packed unit as the windows that begin in it: what k_kc_codes (dx_kmer_codes.hip) writes out and
// k_screen (screen/dx_screen.hip) looks up.  A lane holds its chunk (16 packed bytes = 64 positions on a 16-byte boundary of the
// buffer) and the 8 bytes behind it as three 64-bit words in the read's bit order, moved up to the first position that is the unit's
// and at which a window begins (kc_take); a position's code is one shift of the upper word, the words move up two bits a position,
// and the reverse strand rolls along in a second register, started once a chunk by kc_rc (kc_roll).  Nothing outside [0, bytes) is
// read (last16_ask).  (Outside the evidence set of profiles/, as the files that include it are.)
#pragma once

#include "units/dx_units.hpp"

#define KC_KMAX    32u
#define KC_BATCH   1u                      // units a ticket at least
#define KC_TARGET  (16u << 10)             // packed bytes a ticket
#define KC_CHUNK   64u                     // positions a chunk (16 packed bytes)
#define KC_LANE    4u                      // chunks: a unit of up to so many is its lane's
#define KC_GROUP   UNITS_GROUP             // chunks: up to here 16 lanes take the unit, beyond the wave
#define KC_EVEN64  0x5555555555555555ull

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
