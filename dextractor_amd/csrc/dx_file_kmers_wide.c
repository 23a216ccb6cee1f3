/*
 * dx_file_kmers_wide.c -- the k-mers of the reads of a .dexta / .dexar image for 1 <= k <= 32, counted by sorting: dx_file_kmers_wide;
 * the same k-mers as a set that stays on the device (screen/dx_kmer_set.hip), by the same route up to the sorted array: dx_file_kmer_set,
 * and with every code's count beside it dx_file_kmer_set_counted (one body, a flag);
 * and the two host helpers that turn letters into a 64-bit code and back, dx_kmer_code64 and dx_kmer_letters64.
 *
 * dx_file_kmers (dx_file_kmers.c) counts into a table of 4^k cells and stops at k = 14.  Here every window's code is written into ONE
 * array on the device (dx_code_kmer_codes, units ux.ioff / ux.nsym, slice behind slice), the array is sorted (dx_sort_u64 with
 * bits = 2 k) and the counts are read off the runs of equal codes (dx_kmer_runs): streaming traffic throughout, no atomic request,
 * and the answer in ascending code order.  The meanings are dx_file_kmers': the count is over what the archive HOLDS, record by record.
 *
 * The image is opened and walked as dx_file_kmers_add walks it (dxf_image_open; slices of whole records under dxf_u2_cap /
 * DEXGPU_TEXT_BUDGET, handed over by dxf_u2_slices, dx_file_u2.c).  The windows are known from the lengths before anything is
 * allocated; the codes and the sort's second array stand on the device together, 16 bytes a window.  An image whose windows do not
 * fit that way is DX_E_NOMEM here: dx_files_kmers_wide (dx_file_kmers_files.c) counts such an image, and several images into one
 * answer, in passes over ranges of the codes.
 */
#include <stdlib.h>
#include <string.h>

#include "dexgpu.h"
#include "dx_host.h"
#include "dx_files.h"

#define KMER64_KMAX 32u

/* ---- the host helpers ------------------------------------------------------------------------------------------------ */
int dx_kmer_code64(int arrow, const char *letters, uint32_t k, int canonical, uint64_t *code)
{ uint64_t c = 0, rev = 0;
  uint32_t i;
  if (letters == NULL || code == NULL || k < 1 || k > KMER64_KMAX) return DX_E_ARG;
  for (i = 0; i < k; i++)
    { const int s = dxf_find_letter(arrow, (unsigned char) letters[i]);      /* (the text's end is no letter: nothing behind it is read) */
      if (s < 0) return DX_E_ARG;
      c = (c << 2) | (uint64_t) s;
      rev |= (uint64_t) (3 - s) << (2 * i);                 /* letter i is letter k - 1 - i of the reverse: in the bits 2 i + 1, 2 i */
    }
  *code = canonical && rev < c ? rev : c;
  return DX_OK;
}

int dx_kmer_letters64(int arrow, uint64_t code, uint32_t k, char *out)
{ uint32_t i;
  if (out == NULL || k < 1 || k > KMER64_KMAX || (k < KMER64_KMAX && code >> (2 * k))) return DX_E_ARG;
  for (i = 0; i < k; i++)
    out[i] = (arrow ? "1234" : "ACGT")[(code >> (2 * (k - 1 - i))) & 3];
  out[k] = 0;
  return DX_OK;
}

/* ---- the driver ------------------------------------------------------------------------------------------------------ */
/* DEXGPU_TIMING=1: where the driver spends its time (stderr) */
static void wmark(const char *what)
{ static double t0 = -1.0;
  dx_mark("kmers_wide", &t0, what);
}

/* a slice of the image's packed reads (dxf_u2_slices): its windows' codes written behind those of the slices before it */
typedef struct { dx_ctx *ctx; uint32_t k; int canonical; uint64_t *d_codes, windows, done; } wide_job;

static int wide_slice(void *arg, const u2_slice *s)
{ wide_job *j = arg;
  uint64_t  w = 0;
  int       rc;
  if ((rc = dx_code_kmer_codes(j->ctx, s->d_in, s->bytes, s->d_boff, NULL, s->d_len, s->n, j->k, j->canonical, j->d_codes + j->done,
                               j->windows - j->done, &w, NULL)) != DX_OK) return rc;
  j->done += w;
  return DX_OK;
}

/* The route up to the sorted array, which dx_file_kmers_wide and dx_file_kmer_set share: the image opened and walked, every window's
   code written (slice behind slice) and sorted.  *km: records, symbols, windows and k, the rest zero; *d_codes: the km->windows sorted
   codes, *d_tmp: as many words of room beside them -- both the caller's to dx_free, NULL when there is no window and on any error.
   The refusals are worded by `fail`. */
static int wide_sorted(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, uint32_t k, int canonical,
                       int (*fail)(dx_ctx *, int, const char *), dx_kmers64 *km, void **d_codes, void **d_tmp)
{ image_text im;
  wide_job   j;
  uint64_t   cnt, i;
  size_t     cap;
  const u2_index *x;
  int        rc;
  *d_codes = *d_tmp = NULL;
  memset(km, 0, sizeof(*km));
  km->k = k;
  TRY(dxf_image_open(ctx, kind, 0, 1, img, m, &im));       /* (the line width lays out a text nobody makes) */
  x = &im.ux; cnt = x->cnt;
  km->records = cnt;
  for (i = 0; i < cnt; i++)                                /* the windows, from the lengths: the codes' array is made once */
    { km->symbols += x->nsym[i];
      if (x->nsym[i] >= k) km->windows += x->nsym[i] - k + 1;
    }
  cap = cnt ? dxf_u2_cap(ctx, m, cnt) : 0;
  if (km->windows)
    { TRY(dx_malloc(ctx, (size_t) km->windows * 8 + 64, d_codes));           /* the codes and the sort's second array: 16 bytes a window */
      TRY(dx_malloc(ctx, (size_t) km->windows * 8 + 64, d_tmp));
    }
  wmark("the image walked, the device arrays made");
  j = (wide_job) { ctx, k, canonical, *d_codes, km->windows, 0 };
  if (km->windows) TRY(dxf_u2_slices(ctx, img, x, cap, 0, wide_slice, &j));  /* (the slices' arrays are gone when it returns: the sort has the room) */
  if (j.done != km->windows) { rc = fail(ctx, DX_E_FORMAT, "the slices' windows are not the image's"); goto done; }
  wmark("the slices up, their codes written");

  TRY(dx_sort_u64(ctx, *d_codes, *d_tmp, km->windows, 2 * k));
  wmark("the codes sorted");
  rc = DX_OK;

done:
  if (rc != DX_OK)
    { if (*d_codes) (void) dx_free(ctx, *d_codes);
      if (*d_tmp) (void) dx_free(ctx, *d_tmp);
      *d_codes = *d_tmp = NULL;
    }
  dxf_image_close(&im);
  return rc;
}

int dx_file_kmers_wide(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, uint32_t k, int canonical,
                       uint64_t min_count, uint64_t max_list, dx_kmers64 *out, uint64_t *spectrum, uint32_t nspec,
                       dx_kmer64 **list, uint64_t *listed)
{ dx_kmers64 km;
  dx_kmer64 *lst = NULL;
  uint64_t  *spec = NULL, found = 0, got = 0, room = 0;
  void      *d_codes = NULL, *d_tmp = NULL, *d_list = NULL;
  int        rc, want_list;
  if (ctx == NULL || out == NULL || (img == NULL && m)) return DX_E_ARG;
  if (list) *list = NULL;
  if (listed) *listed = 0;
  if ((rc = dxf_kmers_args(ctx, kind, k, KMER64_KMAX, canonical, dx_kmers_wide_fail)) != DX_OK) return rc;
  if (spectrum != NULL && nspec < 2) return dx_kmers_wide_fail(ctx, DX_E_ARG, "a spectrum of fewer than 2 bins");
  if (list != NULL && listed == NULL) return dx_kmers_wide_fail(ctx, DX_E_ARG, "a list without a place for its length");
  want_list = list != NULL && min_count >= 1;

  wmark(NULL);
  if (spectrum != NULL && (spec = calloc(nspec, sizeof(*spec))) == NULL) { rc = DX_E_NOMEM; goto done; }   /* (the caller's stays as it is on an error) */
  TRY(wide_sorted(ctx, kind, img, m, k, canonical, dx_kmers_wide_fail, &km, &d_codes, &d_tmp));
  if (want_list)
    { room = max_list < km.windows ? max_list : km.windows;                  /* (no more than `windows` runs can pass; d_tmp is free now) */
      if (room > km.windows / 2) TRY(dx_malloc(ctx, (size_t) room * sizeof(dx_kmer64) + 64, &d_list));
    }
  if (km.windows)
    TRY(dx_kmer_runs(ctx, d_codes, km.windows, min_count ? min_count : 1, d_list ? d_list : d_tmp, want_list ? room : 0, &found, spec, nspec,
                     &km.distinct, &km.max_count, &km.max_code));
  if (want_list)
    { got = found < room ? found : room;
      if ((lst = malloc((size_t) (got ? got : 1) * sizeof(*lst))) == NULL) { rc = DX_E_NOMEM; goto done; }
      if (got) TRY(dx_d2h(ctx, lst, d_list ? d_list : d_tmp, (size_t) got * sizeof(*lst)));
    }

  wmark("the runs counted, the list back");

  *out = km;
  if (spectrum) memcpy(spectrum, spec, (size_t) nspec * sizeof(*spec));
  if (list) { *list = lst; lst = NULL; *listed = got; }
  rc = DX_OK;

done:
  if (d_codes) (void) dx_free(ctx, d_codes);
  if (d_tmp) (void) dx_free(ctx, d_tmp);
  if (d_list) (void) dx_free(ctx, d_list);
  free(lst); free(spec);
  wmark("the device arrays freed");
  return rc;
}

/* ---- the same k-mers as a set on the device --------------------------------------------------------------------------- */
static int file_kmer_set(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, uint32_t k, int canonical, uint64_t min_count, int counted,
                         dx_kmer_set **set, dx_kmers64 *out)
{ dx_kmers64   km;
  dx_kmer_set *s = NULL;
  uint64_t     found = 0;
  void        *d_codes = NULL, *d_tmp = NULL;
  int          rc;
  if (ctx == NULL || set == NULL || (img == NULL && m)) return DX_E_ARG;
  *set = NULL;
  if ((rc = dxf_kmers_args(ctx, kind, k, KMER64_KMAX, canonical, dx_kmer_set_fail)) != DX_OK) return rc;
  if (min_count < 1) return dx_kmer_set_fail(ctx, DX_E_ARG, "min_count 0 (1 at least: the unseen codes are in no set)");

  wmark(NULL);
  TRY(wide_sorted(ctx, kind, img, m, k, canonical, dx_kmer_set_fail, &km, &d_codes, &d_tmp));
  if (out != NULL && km.windows)                           /* the report's other three figures, as dx_file_kmers_wide reads them off the runs */
    TRY(dx_kmer_runs(ctx, d_codes, km.windows, 1, NULL, 0, &found, NULL, 0, &km.distinct, &km.max_count, &km.max_code));
  TRY((counted ? dx_kmer_set_from_sorted_counted : dx_kmer_set_from_sorted)(ctx, d_codes, km.windows, min_count, k, canonical,
                                                                          kind == DX_KIND_ARROW, &s));
  wmark("the set made");
  if (out) *out = km;
  *set = s;
  rc = DX_OK;

done:
  if (d_codes) (void) dx_free(ctx, d_codes);
  if (d_tmp) (void) dx_free(ctx, d_tmp);
  wmark("the device arrays freed");
  return rc;
}

int dx_file_kmer_set(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, uint32_t k, int canonical, uint64_t min_count,
                     dx_kmer_set **set, dx_kmers64 *out)
{ return file_kmer_set(ctx, kind, img, m, k, canonical, min_count, 0, set, out); }

int dx_file_kmer_set_counted(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, uint32_t k, int canonical, uint64_t min_count,
                             dx_kmer_set **set, dx_kmers64 *out)
{ return file_kmer_set(ctx, kind, img, m, k, canonical, min_count, 1, set, out); }
