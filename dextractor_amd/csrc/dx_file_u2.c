/*
 * dx_file_u2.c -- the packed reads of a walked .dexta / .dexar image on the device, slice by slice of whole records: dxf_u2_slices,
 * the one loop under every driver that works on the reads where they lie (dx_file_census, dx_file_find / _find_edit / _cut,
 * dx_file_kmers_add, dx_file_kmers_wide, dx_files_kmers_wide); and what decides the slices, dxf_u2_cap and dxf_u2_slice_end.
 *
 * The decoded-text side has the same shape in dxf_unpack2_slices / dxf_undexqv_sliced and their slice_fn.  A slice here is the image's
 * bytes from its first record's packed read to its last one's end, every record's offset into them, and the lengths: what the unit
 * kernels (dx_code_counts, dx_code_find, dx_code_kmers, ...) take as in / boff / len.  What a driver wants per record beside them --
 * counts to bring back -- it asks for as `extra` bytes a record and finds at d_extra: nobody carves the arrays by hand.
 */
#include <stdlib.h>

#include "dexgpu.h"
#include "dx_host.h"
#include "dx_files.h"

/* how much of a 2-bit image of m bytes the device takes at once beside 48 bytes of arrays a record: 0 = all of it.  DEXGPU_TEXT_BUDGET
   counts bytes of image here (there is no text) */
size_t dxf_u2_cap(dx_ctx *ctx, size_t m, uint64_t units)
{ uint64_t fr = 0, all = 0;
  size_t   cap;
  if (dxf_budget_env(m, 4096u, &cap)) return cap;
  if (dx_mem_info(ctx, &fr, &all) != DX_OK || fr == 0) return 0;
  if ((double) m + 48.0 * (double) units <= 0.9 * (double) fr) return 0;
  { const double room = (0.9 * (double) fr) / 2.0;
    return room > (double) ((size_t) 4 << 20) ? (size_t) room : (size_t) 4 << 20;
  }
}

/* a slice of whole records from i0 on: as many as span at most `cap` bytes of image, and one at least; cap 0: all that are left */
uint64_t dxf_u2_slice_end(const u2_index *x, uint64_t i0, size_t cap)
{ uint64_t i1 = i0 + 1;
  if (cap == 0) return x->cnt;
  while (i1 < x->cnt && dxf_u2_end(x, i1) - x->ioff[i0] <= cap) i1++;
  return i1;
}

/* One allocation serves all slices: d_in for the largest slice's bytes, d_arr for the most records a slice has -- their offsets (8 a
   record), the hook's words (`extra` a record, the whole rounded up to 8 bytes), their lengths (4 a record), in this order.  Per slice
   the image's bytes go up, then the offsets, then the lengths; then the hook runs. */
int dxf_u2_slices(dx_ctx *ctx, const uint8_t *img, const u2_index *x, size_t cap, size_t extra, u2_slice_fn fn, void *arg)
{ const uint64_t cnt = x->cnt;
  uint64_t *rel = NULL, i, i0, i1, most = 0;
  size_t    smax = 0, ext;
  void     *d_in = NULL, *d_arr = NULL;
  u2_slice  s;
  int       rc = DX_OK;
  if (cnt == 0) return DX_OK;
  for (i0 = 0; i0 < cnt; i0 = i1)
    { i1 = dxf_u2_slice_end(x, i0, cap);
      if (dxf_u2_end(x, i1 - 1) - x->ioff[i0] > smax) smax = (size_t) (dxf_u2_end(x, i1 - 1) - x->ioff[i0]);
      if (i1 - i0 > most) most = i1 - i0;
    }
  ext = ((size_t) most * extra + 7) & ~(size_t) 7;
  if ((rel = malloc((size_t) most * sizeof(*rel))) == NULL) return DX_E_NOMEM;
  TRY(dx_malloc(ctx, smax + 64, &d_in));
  TRY(dx_malloc(ctx, (size_t) most * 12 + ext + 64, &d_arr));
  s.d_in    = d_in;
  s.d_boff  = d_arr;
  s.d_extra = (uint8_t *) d_arr + (size_t) most * 8;
  s.d_len   = (const uint32_t *) ((uint8_t *) s.d_extra + ext);
  for (i0 = 0; i0 < cnt; i0 = i1)
    { const uint64_t b0 = x->ioff[i0];
      i1 = dxf_u2_slice_end(x, i0, cap);
      s.i0 = i0; s.n = i1 - i0; s.bytes = dxf_u2_end(x, i1 - 1) - b0;
      for (i = i0; i < i1; i++) rel[i - i0] = x->ioff[i] - b0;
      TRY(dx_h2d(ctx, d_in, img + b0, (size_t) s.bytes));
      TRY(dx_h2d(ctx, (void *) s.d_boff, rel, (size_t) s.n * 8));
      TRY(dx_h2d(ctx, (void *) s.d_len, x->nsym + i0, (size_t) s.n * 4));
      TRY(fn(arg, &s));
    }
done:
  if (d_in) (void) dx_free(ctx, d_in);
  if (d_arr) (void) dx_free(ctx, d_arr);
  free(rel);
  return rc;
}
