// dx_kmer_set.hpp -- what a dx_kmer_set is for the two device files of screen/: dx_kmer_set.hip makes it, dx_screen.hip reads it.
// Opaque to everybody else (include/dexgpu.h).
#pragma once

#include <stdint.h>

#define KS_BITS_MAX 26u                    // the bucket index has 2^p + 1 words of 32 bits, p <= 26: 256 MiB at most
#define KS_NMAX     0xffffffffull          // codes a set: fewer than this (first[] holds their places as 32-bit words)

struct dx_kmer_set
{ uint32_t  k, canonical, arrow, bits;     // bits: p, the top bits of the 2 k-bit code that choose the bucket
  uint64_t  n;                             // distinct codes, ascending (compared unsigned)
  uint64_t *d_codes;                       // n of them (never NULL: an empty set has a block of its own too)
  uint32_t *d_first;                       // 2^p + 1: first[b] = the place of the first code whose top p bits are >= b; first[2^p] = n
  uint32_t *d_count;                       // NULL: an uncounted set; else n words, count[i] = how often codes[i] was seen, saturated at 2^32 - 1
  uint64_t  device_bytes;                  // what the arrays take
};
