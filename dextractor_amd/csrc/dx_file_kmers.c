/*
 * dx_file_kmers.c -- the k-mers of the reads of a .dexta / .dexar image, counted: dx_file_kmers_add, dx_file_kmers; and the two
 * host helpers that turn letters into a code and back, dx_kmer_code and dx_kmer_letters.
 *
 * Today the question takes undexta -U of the whole file and a counting loop on one core, or a k-mer counter fed with text.  Here
 * the image is walked on the host (dxf_image_open: any key, legacy layout or byte order) and uploaded, and the packed reads are
 * counted where they lie (dx_code_kmers, units ux.ioff / ux.nsym): no text is made and a quarter of its bytes is read.
 *
 * The count is over what the archive HOLDS: an N that dexta stored as a is an a (Number_Read, DB.c:393-416).  The k-mers are exactly
 * those of the letters undexta -U / undexar prints, record by record; a window never spans two records.
 * An image that does not fit the device, or exceeds DEXGPU_TEXT_BUDGET, goes in slices of whole records (dxf_u2_cap,
 * dxf_u2_slice_end), laid out as dxf_find_run lays them out: the table is added to, so the slices need nothing else.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dexgpu.h"
#include "dx_host.h"
#include "dx_files.h"

#define KMER_KMAX 14u

/* ---- the host helpers ------------------------------------------------------------------------------------------------ */
int dx_kmer_code(int arrow, const char *letters, uint32_t k, int canonical, uint32_t *code)
{ uint32_t c = 0, rev = 0, i;
  if (letters == NULL || code == NULL || k < 1 || k > KMER_KMAX) return DX_E_ARG;
  for (i = 0; i < k; i++)
    { const int s = dxf_find_letter(arrow, (unsigned char) letters[i]);      /* (the text's end is no letter: nothing behind it is read) */
      if (s < 0) return DX_E_ARG;
      c = (c << 2) | (uint32_t) s;
      rev |= (uint32_t) (3 - s) << (2 * i);                 /* letter i is letter k - 1 - i of the reverse: in the bits 2 i + 1, 2 i */
    }
  *code = canonical && rev < c ? rev : c;
  return DX_OK;
}

int dx_kmer_letters(int arrow, uint32_t code, uint32_t k, char *out)
{ uint32_t i;
  if (out == NULL || k < 1 || k > KMER_KMAX || (uint64_t) code >> (2 * k)) return DX_E_ARG;
  for (i = 0; i < k; i++)
    out[i] = (arrow ? "1234" : "ACGT")[(code >> (2 * (k - 1 - i))) & 3];
  out[k] = 0;
  return DX_OK;
}

/* ---- the drivers ----------------------------------------------------------------------------------------------------- */
static int kmers_args(dx_ctx *ctx, int kind, uint32_t k, int canonical)
{ char why[96];
  if (kind == DX_KIND_QUIVA)
    return dx_kmers_fail(ctx, DX_E_ARG, "a .dexqv image has no packed reads to count (DX_KIND_FASTA or DX_KIND_ARROW)");
  if (kind != DX_KIND_FASTA && kind != DX_KIND_ARROW) return dx_kmers_fail(ctx, DX_E_ARG, "unknown kind");
  if (canonical && kind == DX_KIND_ARROW)
    return dx_kmers_fail(ctx, DX_E_ARG, "canonical: pulse widths have no complement (DX_KIND_FASTA only)");
  if (k < 1 || k > KMER_KMAX)
    { snprintf(why, sizeof(why), "k = %u (1 to %u)", k, KMER_KMAX);
      return dx_kmers_fail(ctx, DX_E_ARG, why);
    }
  return DX_OK;
}

static uint64_t u2_end(const u2_index *x, uint64_t i) { return x->ioff[i] + (((uint64_t) x->nsym[i] + 3) >> 2); }

int dx_file_kmers_add(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, uint32_t k, int canonical,
                      uint64_t *d_table, uint64_t *records, uint64_t *symbols, uint64_t *windows)
{ image_text im;
  uint64_t  *rel = NULL, cnt, i, i0, i1, most = 0, sym = 0, win = 0;
  size_t     cap, smax = 0, in_cap = 0, arr_cap = 0;
  void      *d_in = NULL, *d_arr = NULL;
  const u2_index *x;
  int        rc;
  if (ctx == NULL || (img == NULL && m)) return DX_E_ARG;
  if ((rc = kmers_args(ctx, kind, k, canonical)) != DX_OK) return rc;
  if (d_table == NULL) return dx_kmers_fail(ctx, DX_E_ARG, "NULL table");

  TRY(dxf_image_open(ctx, kind, 0, 1, img, m, &im));       /* (the line width lays out a text nobody makes) */
  x = &im.ux; cnt = x->cnt;
  cap = cnt ? dxf_u2_cap(ctx, m, cnt) : 0;
  for (i0 = 0; i0 < cnt; i0 = i1)                          /* the largest slice: one allocation serves them all */
    { i1 = dxf_u2_slice_end(x, i0, cap);
      if (u2_end(x, i1 - 1) - x->ioff[i0] > smax) smax = (size_t) (u2_end(x, i1 - 1) - x->ioff[i0]);
      if (i1 - i0 > most) most = i1 - i0;
    }
  if (cnt)
    { if ((rel = malloc((most + 1) * sizeof(*rel))) == NULL) { rc = DX_E_NOMEM; goto done; }
      TRY(dgrow(ctx, &d_in, &in_cap, smax + 64));
      TRY(dgrow(ctx, &d_arr, &arr_cap, (size_t) most * 12 + 64));            /* offsets (8), symbols (4) */
    }
  for (i0 = 0; i0 < cnt; i0 = i1)
    { const uint64_t b0 = x->ioff[i0];
      uint64_t *d_boff = d_arr, n, bytes, w = 0;
      uint32_t *d_len;
      i1 = dxf_u2_slice_end(x, i0, cap); n = i1 - i0; bytes = u2_end(x, i1 - 1) - b0;
      d_len = (uint32_t *) (d_boff + most);
      for (i = i0; i < i1; i++) { rel[i - i0] = x->ioff[i] - b0; sym += x->nsym[i]; }
      TRY(dx_h2d(ctx, d_in, img + b0, (size_t) bytes));
      TRY(dx_h2d(ctx, d_boff, rel, (size_t) n * 8));
      TRY(dx_h2d(ctx, d_len, x->nsym + i0, (size_t) n * 4));
      TRY(dx_code_kmers(ctx, d_in, bytes, d_boff, NULL, d_len, n, k, canonical, d_table, &w, NULL));
      win += w;
    }
  if (records) *records = cnt;
  if (symbols) *symbols = sym;
  if (windows) *windows = win;
  rc = DX_OK;

done:
  if (d_in) (void) dx_free(ctx, d_in);
  if (d_arr) (void) dx_free(ctx, d_arr);
  dxf_image_close(&im);
  free(rel);
  return rc;
}

int dx_file_kmers(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, uint32_t k, int canonical,
                  uint64_t min_count, uint64_t max_list, dx_kmers *out, uint64_t *spectrum, uint32_t nspec,
                  dx_kmer **list, uint64_t *listed, uint64_t **table)
{ dx_kmers  km;
  dx_kmer  *lst = NULL;
  uint64_t *tab = NULL, found = 0, got = 0, *spec = NULL;
  void     *d_table = NULL, *d_list = NULL;
  size_t    cells;
  int       rc;
  if (ctx == NULL || out == NULL || (img == NULL && m)) return DX_E_ARG;
  if (list) *list = NULL;
  if (listed) *listed = 0;
  if (table) *table = NULL;
  if ((rc = kmers_args(ctx, kind, k, canonical)) != DX_OK) return rc;
  if (spectrum != NULL && nspec < 2) return dx_kmers_fail(ctx, DX_E_ARG, "a spectrum of fewer than 2 bins");
  if (list != NULL && listed == NULL) return dx_kmers_fail(ctx, DX_E_ARG, "a list without a place for its length");
  memset(&km, 0, sizeof(km));
  km.k = k;
  cells = (size_t) 1 << (2 * k);

  if (spectrum != NULL && (spec = malloc((size_t) nspec * sizeof(*spec))) == NULL) return DX_E_NOMEM;     /* (the caller's stays as it is on an error) */
  TRY(dx_malloc(ctx, cells * 8 + 64, &d_table));
  TRY(dx_memset(ctx, d_table, 0, cells * 8));
  TRY(dx_file_kmers_add(ctx, kind, img, m, k, canonical, d_table, &km.records, &km.symbols, &km.windows));
  TRY(dx_kmer_spectrum(ctx, d_table, k, spec, nspec, &km.distinct, &km.max_count, &km.max_code));
  if (list != NULL && min_count >= 1)
    { const uint64_t room = max_list < km.distinct ? max_list : km.distinct;          /* (no more than `distinct` can pass) */
      if (room) TRY(dx_malloc(ctx, (size_t) room * sizeof(dx_kmer) + 64, &d_list));
      if (min_count <= km.max_count) TRY(dx_kmer_list(ctx, d_table, k, min_count, d_list, room, &found));
      got = found < room ? found : room;
      if ((lst = malloc((size_t) (got ? got : 1) * sizeof(*lst))) == NULL) { rc = DX_E_NOMEM; goto done; }
      if (got) TRY(dx_d2h(ctx, lst, d_list, (size_t) got * sizeof(*lst)));
    }
  if (table != NULL)
    { if ((tab = malloc(cells * 8)) == NULL) { rc = DX_E_NOMEM; goto done; }
      TRY(dx_d2h(ctx, tab, d_table, cells * 8));
    }

  *out = km;
  if (spectrum) memcpy(spectrum, spec, (size_t) nspec * sizeof(*spec));
  if (list) { *list = lst; lst = NULL; *listed = got; }
  if (table) { *table = tab; tab = NULL; }
  rc = DX_OK;

done:
  if (d_table) (void) dx_free(ctx, d_table);
  if (d_list) (void) dx_free(ctx, d_list);
  free(lst); free(tab); free(spec);
  return rc;
}
