// dx_find_edit.hpp -- the queries of the edit-distance kernels as they stand in a kernel argument: what find/dx_find_edit.hip (the ends of
// the occurrences) and find/dx_find_span.hip (their starts) share.  (Outside the evidence set of profiles/, as those files are.)
#pragma once

#include <string.h>

#include "dx_internal.hpp"

#define FE_QMAX    64u                     // queries a call

// a query as the kernels read it: the two bit planes of its symbols (b0: the low bits, b1: the high) at the TOP of a 64-bit word, and
// `low`: the bits below the query, which the column keeps neutral.
//   forward (dx_find_edit.hip):  symbol i in bit 64 - len + i -- the query's LAST symbol in the word's top bit, where the score's delta is
//     read without a shift by len;
//   reversed (dx_find_span.hip): symbol i in bit 63 - i -- the query read backwards, so its FIRST symbol is in the top bit.
struct fe_query   { uint64_t b0, b1, low; uint32_t len, err; };     // 32 bytes
struct fe_queries { fe_query q[FE_QMAX]; };

static_assert(sizeof(dx_equery) == 24 && sizeof(fe_query) == 32, "64 queries fit a kernel argument");

// The checks both entry points make of q and nq (DX_E_ARG, worded for `who`), and the planes
static int fe_queries_make(dx_ctx *ctx, const char *who, const dx_equery *q, uint32_t nq, bool reversed, fe_queries *Q)
{ if (nq < 1u || nq > FE_QMAX) return dx_fail(ctx, DX_E_ARG, "%s: %u queries (1 to %u)", who, nq, FE_QMAX);
  if (q == NULL) return dx_fail(ctx, DX_E_ARG, "%s: NULL pointer", who);
  memset(Q, 0, sizeof(*Q));
  for (uint32_t k = 0; k < nq; k++)
    { const uint32_t m = q[k].len;
      if (m < 1u || m > 64u) return dx_fail(ctx, DX_E_ARG, "%s: query %u has %u symbols (1 to 64)", who, k, m);
      if (q[k].max_err >= m)
        return dx_fail(ctx, DX_E_ARG, "%s: query %u: %u errors are not below its %u symbols", who, k, q[k].max_err, m);
      for (uint32_t i = 0; i < 64u; i++)
        { const uint64_t c = (q[k].code[i >> 5] >> (2u * (31u - (i & 31u)))) & 3u;
          const uint32_t at = reversed ? 63u - i : 64u - m + i;
          if (i < m) { Q->q[k].b0 |= (c & 1u) << at; Q->q[k].b1 |= (c >> 1) << at; }
          else if (c) return dx_fail(ctx, DX_E_ARG, "%s: query %u has bits behind its %u symbols", who, k, m);
        }
      Q->q[k].low = m < 64u ? (1ull << (64u - m)) - 1u : 0ull;
      Q->q[k].len = m; Q->q[k].err = q[k].max_err;
    }
  return DX_OK;
}
