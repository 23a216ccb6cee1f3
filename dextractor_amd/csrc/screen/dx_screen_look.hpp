// dx_screen_look.hpp -- the look-up of a chunk's windows in a dx_kmer_set and the cover mask of its hits: what k_screen
// (screen/dx_screen.hip) and k_spans (screen/dx_screen_spans.hip) share.  dx_screen.hip's header says how the look-up (sc_mask) and
// the coverage (sc_cover) work and what they cost; the walk over a unit's chunks is kmers/dx_kmer_windows.hpp's.  (Outside the evidence set of profiles/, as the files that include it are.)
#pragma once

#include "kmers/dx_kmer_windows.hpp"
#include "screen/dx_kmer_set.hpp"

#define SC_BATCH  8u                       // positions a lane asks for before it waits for any
#define SC_LINEAR 4u                       // codes of a bucket that are looked at one after the other; more are bisected first
#define SC_NONE   0xffffffffu

// what a kernel needs of a dx_kmer_set
struct sc_set { const uint64_t *code; const uint32_t *first; uint32_t k, shift; };     // shift = 2 k - p

static sc_set sc_set_of(const dx_kmer_set *set)
{ const sc_set s = { set->d_codes, set->d_first, set->k, 2u * set->k - set->bits };
  return s;
}

// the part's hit mask: bit bit0 + i = window i of the part is in the set (bit0 + p.n <= 64)
template <bool CANON>
__device__ __forceinline__ uint64_t sc_mask(const kc_part &p, uint32_t bit0, const sc_set &s)
{ uint64_t m = 0ull;
  if (p.n == 0u) return m;
  kc_roll<CANON> r(p, s.k);
  for (uint32_t i0 = 0; i0 < p.n; i0 += SC_BATCH)
    { uint64_t c[SC_BATCH], v[SC_BATCH];
      uint32_t lo[SC_BATCH], hi[SC_BATCH];
      #pragma unroll
      for (uint32_t t = 0; t < SC_BATCH; t++) { c[t] = r.code(); r.step(); }
      #pragma unroll
      for (uint32_t t = 0; t < SC_BATCH; t++)
        { const uint64_t two = *(const u64_u *) (s.first + (c[t] >> s.shift));
          lo[t] = (uint32_t) two; hi[t] = (uint32_t) (two >> 32);
        }
      #pragma unroll
      for (uint32_t t = 0; t < SC_BATCH; t++)
        { while (hi[t] - lo[t] > SC_LINEAR)                           // (a long bucket: a small p, or many codes that share their top bits)
            { const uint32_t mid = lo[t] + (hi[t] - lo[t]) / 2u;
              if (s.code[mid] <= c[t]) lo[t] = mid; else hi[t] = mid;
            }
          v[t] = lo[t] < hi[t] ? s.code[lo[t]] : ~c[t];
        }
      #pragma unroll
      for (uint32_t t = 0; t < SC_BATCH; t++)
        { bool hit = v[t] == c[t];
          for (uint32_t j = lo[t] + 1u; !hit && j < hi[t] && v[t] < c[t]; j++)
            { v[t] = s.code[j];
              hit = v[t] == c[t];
            }
          if (hit && i0 + t < p.n) m |= 1ull << (bit0 + i0 + t);
        }
    }
  return m;
}

// sc_mask's sibling for k_depths (screen/dx_screen_depth.hip): the same buckets, the same batches of SC_BATCH positions and the same
// search, but what is kept of a code that is found is its PLACE in the set, not a bit.  at[t] = the place of batch position t's code,
// SC_NONE when the set does not hold it; r stands at the batch's first window and is moved SC_BATCH windows on.  (A position past the
// part's windows makes a code of the words all the same and asks for a bucket that exists; its answer is the caller's to drop.)
template <bool CANON>
__device__ __forceinline__ void sc_places(kc_roll<CANON> &r, const sc_set &s, uint32_t at[SC_BATCH])
{ uint64_t c[SC_BATCH], v[SC_BATCH];
  uint32_t lo[SC_BATCH], hi[SC_BATCH];
  #pragma unroll
  for (uint32_t t = 0; t < SC_BATCH; t++) { c[t] = r.code(); r.step(); }
  #pragma unroll
  for (uint32_t t = 0; t < SC_BATCH; t++)
    { const uint64_t two = *(const u64_u *) (s.first + (c[t] >> s.shift));
      lo[t] = (uint32_t) two; hi[t] = (uint32_t) (two >> 32);
    }
  #pragma unroll
  for (uint32_t t = 0; t < SC_BATCH; t++)
    { while (hi[t] - lo[t] > SC_LINEAR)
        { const uint32_t mid = lo[t] + (hi[t] - lo[t]) / 2u;
          if (s.code[mid] <= c[t]) lo[t] = mid; else hi[t] = mid;
        }
      v[t] = lo[t] < hi[t] ? s.code[lo[t]] : ~c[t];
    }
  #pragma unroll
  for (uint32_t t = 0; t < SC_BATCH; t++)
    { uint32_t j = lo[t];
      bool hit = v[t] == c[t];
      for (; !hit && j + 1u < hi[t] && v[t] < c[t]; )
        { v[t] = s.code[++j];
          hit = v[t] == c[t];
        }
      at[t] = hit ? j : SC_NONE;
    }
}

// the positions of a chunk that lie in a hit window: the chunk's mask m and the mask of the chunk in front of it
__device__ __forceinline__ uint64_t sc_cover(uint64_t m, uint64_t prev, uint32_t k)
{ uint64_t hi = m, lo = prev;
  uint32_t w = 1;
  for (; 2u * w <= k; w *= 2u)                                         // (w < 64: k <= 32)
    { hi |= (hi << w) | (lo >> (64u - w));
      lo |= lo << w;
    }
  if (k > w)
    { const uint32_t d = k - w;
      hi |= (hi << d) | (lo >> (64u - d));
    }
  return hi;
}

// chunk `a` (its byte) of the unit that is symbols [S0, S1) of the buffer: its mask; prev: the mask of the chunk in front
template <bool CANON>
__device__ __forceinline__ uint64_t sc_chunk_mask(const uint8_t *in, uint64_t bytes, uint64_t a, uint64_t S0, uint64_t S1, const sc_set &s)
{ const kc_part p = kc_take(in, bytes, a, S0, S1, s.k);
  return p.n ? sc_mask<CANON>(p, (uint32_t) (S0 + p.first - 4u * a), s) : 0ull;
}
