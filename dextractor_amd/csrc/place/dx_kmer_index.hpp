// dx_kmer_index.hpp -- what a dx_kmer_index is for the device files of place/: dx_kmer_index.hip makes it, dx_place_seeds.hip reads it.
// Opaque to everybody else (include/dexgpu.h).  (Outside the evidence set of profiles/, as the files that include it are.)
#pragma once

#include <stdint.h>
#include "screen/dx_kmer_set.hpp"

#define KX_GMAX (1ull << 31)               // symbols a reference: fewer than this (a position and its flip are one 32-bit word)

struct dx_kmer_index
{ dx_kmer_set *set;                        // the COUNTED set of the reference's windows: codes ascending, count[i] = the occurrences of code i
  uint32_t    *d_start;                    // set->n + 1: the exclusive sums of the counts; start[n] = the windows
  uint32_t    *d_pos;                      // windows: pos[start[i] .. start[i + 1]) = code i's occurrences as g << 1 | flip, ascending in g
  uint64_t    *toff;                       // HOST, targets + 1: the exclusive sums of the targets' lengths; toff[targets] = the symbols
  uint64_t     targets, windows;
  uint64_t     device_bytes;               // the set's arrays, start and pos
};
