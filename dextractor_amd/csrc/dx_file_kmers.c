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
 * An image that does not fit the device, or exceeds DEXGPU_TEXT_BUDGET, goes in slices of whole records (dxf_u2_cap; dxf_u2_slices,
 * dx_file_u2.c): the table is added to, so the slices need nothing else.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dexgpu.h"
#include "dx_host.h"
#include "dx_files.h"

#define KMER_KMAX 14u

/* ---- the host helpers: the 64-bit ones (dx_file_kmers_wide.c) under this table's limit ------------------------------------ */
int dx_kmer_code(int arrow, const char *letters, uint32_t k, int canonical, uint32_t *code)
{ uint64_t c;
  int      rc;
  if (code == NULL || k > KMER_KMAX) return DX_E_ARG;
  if ((rc = dx_kmer_code64(arrow, letters, k, canonical, &c)) == DX_OK) *code = (uint32_t) c;
  return rc;
}

int dx_kmer_letters(int arrow, uint32_t code, uint32_t k, char *out)
{ if (k > KMER_KMAX) return DX_E_ARG;
  return dx_kmer_letters64(arrow, code, k, out);          /* (which refuses a code with bits above its 2 k) */
}

/* ---- the drivers ----------------------------------------------------------------------------------------------------- */
int dxf_kmers_args(dx_ctx *ctx, int kind, uint32_t k, uint32_t kmax, int canonical, int (*fail)(dx_ctx *, int, const char *))
{ char why[96];
  if (kind == DX_KIND_QUIVA)
    return fail(ctx, DX_E_ARG, "a .dexqv image has no packed reads to count (DX_KIND_FASTA or DX_KIND_ARROW)");
  if (kind != DX_KIND_FASTA && kind != DX_KIND_ARROW) return fail(ctx, DX_E_ARG, "unknown kind");
  if (canonical && kind == DX_KIND_ARROW)
    return fail(ctx, DX_E_ARG, "canonical: pulse widths have no complement (DX_KIND_FASTA only)");
  if (k < 1 || k > kmax)
    { snprintf(why, sizeof(why), "k = %u (1 to %u)", k, kmax);
      return fail(ctx, DX_E_ARG, why);
    }
  return DX_OK;
}

/* a slice of the image's packed reads (dxf_u2_slices): its k-mers added to the table, its symbols and windows to the sums */
typedef struct { dx_ctx *ctx; const uint32_t *nsym; uint32_t k; int canonical; uint64_t *d_table, sym, win; } kmers_job;

static int kmers_slice(void *arg, const u2_slice *s)
{ kmers_job *j = arg;
  uint64_t   i, w = 0;
  int        rc;
  for (i = 0; i < s->n; i++) j->sym += j->nsym[s->i0 + i];
  if ((rc = dx_code_kmers(j->ctx, s->d_in, s->bytes, s->d_boff, NULL, s->d_len, s->n, j->k, j->canonical, j->d_table, &w, NULL)) != DX_OK) return rc;
  j->win += w;
  return DX_OK;
}

int dx_file_kmers_add(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, uint32_t k, int canonical,
                      uint64_t *d_table, uint64_t *records, uint64_t *symbols, uint64_t *windows)
{ image_text im;
  kmers_job  j = { ctx, NULL, k, canonical, d_table, 0, 0 };
  uint64_t   cnt;
  int        rc;
  if (ctx == NULL || (img == NULL && m)) return DX_E_ARG;
  if ((rc = dxf_kmers_args(ctx, kind, k, KMER_KMAX, canonical, dx_kmers_fail)) != DX_OK) return rc;
  if (d_table == NULL) return dx_kmers_fail(ctx, DX_E_ARG, "NULL table");

  TRY(dxf_image_open(ctx, kind, 0, 1, img, m, &im));       /* (the line width lays out a text nobody makes) */
  cnt = im.ux.cnt; j.nsym = im.ux.nsym;
  TRY(dxf_u2_slices(ctx, img, &im.ux, cnt ? dxf_u2_cap(ctx, m, cnt) : 0, 0, kmers_slice, &j));
  if (records) *records = cnt;
  if (symbols) *symbols = j.sym;
  if (windows) *windows = j.win;
  rc = DX_OK;

done:
  dxf_image_close(&im);
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
  if ((rc = dxf_kmers_args(ctx, kind, k, KMER_KMAX, canonical, dx_kmers_fail)) != DX_OK) return rc;
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
