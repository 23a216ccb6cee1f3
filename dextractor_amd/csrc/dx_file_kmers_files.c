/*
 * dx_file_kmers_files.c -- the k-mers of the reads of SEVERAL .dexta / .dexar images, 1 <= k <= 32, counted into one answer, in as
 * many passes over ranges of the codes as the device's memory asks for: dx_files_kmers_wide; and the same k-mers as one set on the
 * device: dx_files_kmer_set, and with every code's count beside it dx_files_kmer_set_counted (one body, a flag).
 *
 * dx_file_kmers_wide (dx_file_kmers_wide.c) writes every window's code of ONE image into one array, sorts it and reads the counts off
 * the runs: 16 bytes of device memory a window.  The answer of a range of codes depends on no other range, and the order is the
 * codes': so here the windows are counted range after range, ascending, and the ranges' answers concatenate -- the spectra and
 * `distinct` add, the lists append, the largest count is replaced only by a strictly larger one.  Nothing is merged.
 *
 *   1. every image is opened (dxf_image_open); the windows are known from the lengths;
 *   2. room = the windows a pass may hold: the caller's, or 0.8 x free / 16 (dx_mem_info), 2^36 - 1 at most (the sort's bound);
 *   3. all windows fit: ONE pass, whose launches are dx_file_kmers_wide's, image after image -- dx_code_kmer_codes slice behind slice
 *      into the one array; no bins, no filter;
 *   4. otherwise a pass over all images counts the windows by the top min(2 k, 12) bits of their codes (dx_code_kmer_bins), and
 *      dx_kmer_range_plan cuts the bins into ranges of at most `room` windows; a single bin above `room` is DX_E_NOMEM (finer
 *      splitting is not built);
 *   5. a range: every image's slices again, dx_code_kmer_codes_range one behind the other into the one array -- what was written must be
 *      the bins' sum --, dx_sort_u64 (bits = 2 k), then what the caller of the passes wants of the sorted codes (dx_kmer_runs; dx_sorted_take).
 *
 * The images are walked on the host once and UPLOADED ONCE A PASS (dxf_u2_slices under dxf_u2_cap / DEXGPU_TEXT_BUDGET, as
 * dx_file_kmers_wide does it): p ranges cost p + 1 uploads of every image.  Keeping the packed images resident -- 1/64 of the codes'
 * bytes -- is the obvious next saving; not built.  DEXGPU_TIMING=1 marks every pass.
 */
#include <stdlib.h>
#include <string.h>

#include "dexgpu.h"
#include "dx_host.h"
#include "dx_files.h"

#define KMER64_KMAX 32u
#define BINS_BITS   12u                     /* dx_code_kmer_bins' most */
#define SORT_MAX    ((1ull << 36) - 1)      /* keys dx_sort_u64 and dx_kmer_runs take */

/* DEXGPU_TIMING=1: where the drivers spend their time (stderr) */
static void fmark(const char *what)
{ static double t0 = -1.0;
  dx_mark("kmers_files", &t0, what);
}

/* ---- the passes ------------------------------------------------------------------------------------------------------- */
/* what a slice of an image's packed reads (dxf_u2_slices) is asked for: its windows' codes behind those of the slices before it (all
   of them, or those of bins [lo, hi)), or its windows added to the bins */
enum { JOB_CODES, JOB_BINS, JOB_RANGE };
typedef struct { dx_ctx *ctx; uint32_t k; int canonical, what; uint32_t bits, lo, hi; uint64_t *d_codes, *d_bins, cap, done; } files_job;

static int files_slice(void *arg, const u2_slice *s)
{ files_job *j = arg;
  uint64_t   w = 0;
  int        rc;
  if (j->what == JOB_BINS)
    rc = dx_code_kmer_bins(j->ctx, s->d_in, s->bytes, s->d_boff, NULL, s->d_len, s->n, j->k, j->canonical, j->bits, j->d_bins, &w, NULL);
  else if (j->what == JOB_RANGE)
    rc = dx_code_kmer_codes_range(j->ctx, s->d_in, s->bytes, s->d_boff, NULL, s->d_len, s->n, j->k, j->canonical, j->bits, j->lo, j->hi,
                                  j->d_codes + j->done, j->cap - j->done, &w, NULL);
  else
    rc = dx_code_kmer_codes(j->ctx, s->d_in, s->bytes, s->d_boff, NULL, s->d_len, s->n, j->k, j->canonical, j->d_codes + j->done,
                            j->cap - j->done, &w, NULL);
  if (rc != DX_OK) return rc;
  j->done += w;
  return DX_OK;
}

/* every image's slices, one image behind the other, to the job */
static int files_walk(dx_ctx *ctx, const uint8_t *const *imgs, const size_t *bytes, const image_text *im, uint32_t nimg, files_job *j)
{ uint32_t i;
  int      rc;
  for (i = 0; i < nimg; i++)
    if (im[i].ux.cnt && (rc = dxf_u2_slices(ctx, imgs[i], &im[i].ux, dxf_u2_cap(ctx, bytes[i], im[i].ux.cnt), 0, files_slice, j)) != DX_OK)
      return rc;
  return DX_OK;
}

/* a range's n > 0 sorted codes at d_codes, and as many words of room at d_tmp, to who asked for the passes */
typedef int (*range_fn)(void *arg, uint64_t *d_codes, uint64_t *d_tmp, uint64_t n);

/* The passes that dx_files_kmers_wide and dx_files_kmer_set share.  *tot: records, symbols, windows summed and k, the rest zero (`fn`
   knows the rest); per_file (may be NULL): the same an image; *passes (may be NULL): the ranges that were sorted -- 0 when there is no
   window.  Every device array made here is freed here, whatever happens. */
static int files_passes(dx_ctx *ctx, const char *who, int kind, const uint8_t *const *imgs, const size_t *bytes, uint32_t nimg, uint32_t k,
                        int canonical, uint64_t room, dx_kmers64 *tot, dx_kmers64 *per_file, uint32_t *passes, range_fn fn, void *arg)
{ image_text *im = NULL;
  uint64_t   *bins = NULL, fr = 0, all = 0, most = 0, sum, i;
  uint32_t   *cut = NULL, opened = 0, ranges = 0, nbins = 0, r, b, f;
  void       *d_codes = NULL, *d_tmp = NULL, *d_bins = NULL;
  files_job   j;
  int         rc;
  memset(tot, 0, sizeof(*tot));
  tot->k = k;
  if (passes) *passes = 0;
  if (nimg && (im = calloc(nimg, sizeof(*im))) == NULL) return DX_E_NOMEM;
  for (f = 0; f < nimg; f++)
    { dx_kmers64 km;
      const u2_index *x = &im[f].ux;
      memset(&km, 0, sizeof(km));
      km.k = k;
      (void) dx_kmers_files_image_fail(ctx, DX_OK, who, -1);
      opened = f + 1;
      if ((rc = dxf_image_open(ctx, kind, 0, 1, imgs[f], bytes[f], &im[f])) != DX_OK)     /* (the line width lays out a text nobody makes) */
        { rc = dx_kmers_files_image_fail(ctx, rc, who, (int64_t) f); goto done; }
      km.records = x->cnt;
      for (i = 0; i < x->cnt; i++)                         /* the windows, from the lengths */
        { km.symbols += x->nsym[i];
          if (x->nsym[i] >= k) km.windows += x->nsym[i] - k + 1;
        }
      tot->records += km.records; tot->symbols += km.symbols; tot->windows += km.windows;
      if (per_file) per_file[f] = km;
    }
  fmark("the images walked");
  if (tot->windows == 0) { rc = DX_OK; goto done; }

  if (room == 0 && dx_mem_info(ctx, &fr, &all) == DX_OK) room = (uint64_t) (0.8 * (double) fr / 16.0);
  if (room == 0 || room > SORT_MAX) room = SORT_MAX;
  j = (files_job) { ctx, k, canonical, JOB_CODES, 0, 0, 0, NULL, NULL, 0, 0 };

  if (tot->windows <= room) { ranges = 1; most = tot->windows; }
  else
    { /* the bins of all images, the plan */
      j.bits = 2 * k < BINS_BITS ? 2 * k : BINS_BITS;
      nbins = 1u << j.bits;
      if ((bins = malloc((size_t) nbins * sizeof(*bins))) == NULL || (cut = malloc(((size_t) nbins + 1) * sizeof(*cut))) == NULL)
        { rc = DX_E_NOMEM; goto done; }
      memset(bins, 0, (size_t) nbins * sizeof(*bins));
      TRY(dx_malloc(ctx, (size_t) nbins * 8 + 64, &d_bins));
      TRY(dx_h2d(ctx, d_bins, bins, (size_t) nbins * 8));
      j.what = JOB_BINS; j.d_bins = d_bins;
      TRY(files_walk(ctx, imgs, bytes, im, nimg, &j));
      TRY(dx_d2h(ctx, bins, d_bins, (size_t) nbins * 8));
      (void) dx_free(ctx, d_bins); d_bins = NULL;
      for (sum = 0, b = 0; b < nbins; b++) sum += bins[b];
      if (j.done != tot->windows || sum != tot->windows)
        { rc = dx_kmers_files_fail(ctx, DX_E_FORMAT, who, "the bins' windows are not the images'"); goto done; }
      TRY(dx_kmer_range_plan(ctx, bins, nbins, room, cut, &ranges));
      for (r = 0; r < ranges; r++)
        { for (sum = 0, b = cut[r]; b < cut[r + 1]; b++) sum += bins[b];
          if (sum > most) most = sum;
        }
      fmark("the bins counted, the ranges planned");
    }

  TRY(dx_malloc(ctx, (size_t) most * 8 + 64, &d_codes));   /* the codes and the sort's second array: 16 bytes a window of the largest range */
  TRY(dx_malloc(ctx, (size_t) most * 8 + 64, &d_tmp));
  j.d_codes = d_codes;
  for (r = 0; r < ranges; r++)
    { uint64_t want = tot->windows;
      j.what = JOB_CODES; j.done = 0;
      if (bins)
        { for (want = 0, b = cut[r]; b < cut[r + 1]; b++) want += bins[b];
          j.what = JOB_RANGE; j.lo = cut[r]; j.hi = cut[r + 1];
        }
      j.cap = want;
      if (want == 0) continue;                             /* (a range of empty bins alone: bins that are all empty) */
      TRY(files_walk(ctx, imgs, bytes, im, nimg, &j));
      if (j.done != want)
        { rc = dx_kmers_files_fail(ctx, DX_E_FORMAT, who, bins ? "a range's windows are not its bins'" : "the slices' windows are not the images'"); goto done; }
      fmark("a pass: the images up, the codes written");
      TRY(dx_sort_u64(ctx, d_codes, d_tmp, want, 2 * k));
      fmark("a pass: the codes sorted");
      TRY(fn(arg, d_codes, d_tmp, want));
      fmark("a pass: the runs read");
      if (passes) ++*passes;
    }
  rc = DX_OK;

done:
  if (d_codes) (void) dx_free(ctx, d_codes);
  if (d_tmp) (void) dx_free(ctx, d_tmp);
  if (d_bins) (void) dx_free(ctx, d_bins);
  for (f = 0; f < opened; f++) dxf_image_close(&im[f]);
  free(im); free(bins); free(cut);
  return rc;
}

/* the refusals the two drivers share; `fail` words them */
static int wide_files_fail(dx_ctx *ctx, int code, const char *what) { return dx_kmers_files_fail(ctx, code, "dx_files_kmers_wide", what); }
static int set_files_fail(dx_ctx *ctx, int code, const char *what)  { return dx_kmers_files_fail(ctx, code, "dx_files_kmer_set", what); }

static int files_args(dx_ctx *ctx, int kind, const uint8_t *const *imgs, const size_t *bytes, uint32_t nimg, uint32_t k, int canonical,
                      int (*fail)(dx_ctx *, int, const char *))
{ uint32_t f;
  int      rc;
  if ((rc = dxf_kmers_args(ctx, kind, k, KMER64_KMAX, canonical, fail)) != DX_OK) return rc;
  if (nimg && (imgs == NULL || bytes == NULL)) return fail(ctx, DX_E_ARG, "NULL pointer");
  for (f = 0; f < nimg; f++)
    if (imgs[f] == NULL && bytes[f]) return fail(ctx, DX_E_ARG, "NULL image");
  return DX_OK;
}

/* ---- dx_files_kmers_wide ---------------------------------------------------------------------------------------------- */
typedef struct
  { dx_ctx *ctx; uint64_t min_count, max_list, *spec, *rspec, got; uint32_t nspec; int want_list; dx_kmers64 *km; dx_kmer64 *lst; } wide_fold;

/* a range's runs, folded into the answer so far: the ranges ascend */
static int wide_range(void *arg, uint64_t *d_codes, uint64_t *d_tmp, uint64_t n)
{ wide_fold *w = arg;
  uint64_t   found = 0, distinct = 0, mx = 0, mc = 0, room = 0, take;
  void      *d_list = NULL;
  uint32_t   c;
  int        rc;
  if (w->want_list)
    { room = w->max_list - w->got < n ? w->max_list - w->got : n;            /* (no more than n runs can pass; d_tmp is free now) */
      if (room > n / 2) TRY(dx_malloc(w->ctx, (size_t) room * sizeof(dx_kmer64) + 64, &d_list));
    }
  TRY(dx_kmer_runs(w->ctx, d_codes, n, w->min_count ? w->min_count : 1, d_list ? d_list : (void *) d_tmp, room, &found, w->rspec, w->nspec,
                   &distinct, &mx, &mc));
  for (c = 0; c < w->nspec; c++) w->spec[c] += w->rspec[c];
  w->km->distinct += distinct;
  if (mx > w->km->max_count) { w->km->max_count = mx; w->km->max_code = mc; }  /* (strictly: of equal counts the smallest code stays) */
  take = found < room ? found : room;
  if (take)
    { dx_kmer64 *more = realloc(w->lst, (size_t) (w->got + take) * sizeof(*more));
      if (more == NULL) { rc = DX_E_NOMEM; goto done; }
      w->lst = more;
      TRY(dx_d2h(w->ctx, w->lst + w->got, d_list ? d_list : (void *) d_tmp, (size_t) take * sizeof(*more)));
      w->got += take;
    }
  rc = DX_OK;
done:
  if (d_list) (void) dx_free(w->ctx, d_list);
  return rc;
}

int dx_files_kmers_wide(dx_ctx *ctx, int kind, const uint8_t *const *imgs, const size_t *bytes, uint32_t nimg, uint32_t k, int canonical,
                        uint64_t min_count, uint64_t max_list, uint64_t room, dx_kmers64 *out, uint64_t *spectrum, uint32_t nspec,
                        dx_kmer64 **list, uint64_t *listed, dx_kmers64 *per_file, uint32_t *passes)
{ dx_kmers64  km, *pf = NULL;
  wide_fold   w;
  uint32_t    np = 0;
  int         rc;
  if (ctx == NULL || out == NULL) return DX_E_ARG;
  if (list) *list = NULL;
  if (listed) *listed = 0;
  if ((rc = files_args(ctx, kind, imgs, bytes, nimg, k, canonical, wide_files_fail)) != DX_OK) return rc;
  if (spectrum != NULL && nspec < 2) return wide_files_fail(ctx, DX_E_ARG, "a spectrum of fewer than 2 bins");
  if (list != NULL && listed == NULL) return wide_files_fail(ctx, DX_E_ARG, "a list without a place for its length");
  if (spectrum == NULL) nspec = 0;

  fmark(NULL);
  memset(&w, 0, sizeof(w));
  w.ctx = ctx; w.min_count = min_count; w.max_list = max_list; w.nspec = nspec; w.km = &km;
  w.want_list = list != NULL && min_count >= 1;
  if (nspec && ((w.spec = calloc(nspec, sizeof(*w.spec))) == NULL || (w.rspec = calloc(nspec, sizeof(*w.rspec))) == NULL))
    { rc = DX_E_NOMEM; goto done; }                        /* (the caller's stays as it is on an error) */
  if (per_file && nimg && (pf = calloc(nimg, sizeof(*pf))) == NULL) { rc = DX_E_NOMEM; goto done; }
  if (w.want_list && (w.lst = malloc(sizeof(*w.lst))) == NULL) { rc = DX_E_NOMEM; goto done; }
  TRY(files_passes(ctx, "dx_files_kmers_wide", kind, imgs, bytes, nimg, k, canonical, room, &km, pf, &np, wide_range, &w));

  *out = km;
  if (spectrum) memcpy(spectrum, w.spec, (size_t) nspec * sizeof(*w.spec));
  if (list) { *list = w.lst; w.lst = NULL; *listed = w.got; }
  if (pf) memcpy(per_file, pf, (size_t) nimg * sizeof(*pf));
  if (passes) *passes = np;
  rc = DX_OK;

done:
  free(w.lst); free(w.spec); free(w.rspec); free(pf);
  fmark("the device arrays freed");
  return rc;
}

/* ---- dx_files_kmer_set ------------------------------------------------------------------------------------------------ */
typedef struct
  { dx_ctx *ctx; uint64_t min_count, total; int report, counted; dx_kmers64 *km; void **part, **cpart; uint64_t *len; uint32_t parts; } set_fold;

/* a range's kept codes, into a device array of exactly their size -- and, counted, their runs' lengths into a second one */
static int set_range(void *arg, uint64_t *d_codes, uint64_t *d_tmp, uint64_t n)
{ set_fold *s = arg;
  uint64_t  found = 0, again = 0, listed = 0, distinct = 0, mx = 0, mc = 0;
  int       rc;
  if (s->report)                                           /* the report's other three figures, as dx_file_kmer_set reads them off the runs */
    { if ((rc = dx_kmer_runs(s->ctx, d_codes, n, 1, NULL, 0, &listed, NULL, 0, &distinct, &mx, &mc)) != DX_OK) return rc;
      s->km->distinct += distinct;
      if (mx > s->km->max_count) { s->km->max_count = mx; s->km->max_code = mc; }
    }
  if ((rc = dx_sorted_take(s->ctx, d_codes, n, s->min_count, NULL, 0, &found)) != DX_OK || found == 0) return rc;
  if ((rc = dx_malloc(s->ctx, (size_t) found * 8 + 64, &s->part[s->parts])) != DX_OK) return rc;
  if (s->counted && (rc = dx_malloc(s->ctx, (size_t) found * 4 + 64, &s->cpart[s->parts])) != DX_OK) return rc;   /* (the caller frees the part) */
  s->len[s->parts++] = found;
  s->total += found;
  if (s->counted)
    return dx_sorted_take_counted(s->ctx, d_codes, n, s->min_count, d_tmp, n, s->part[s->parts - 1], s->cpart[s->parts - 1], found, &again);
  return dx_sorted_take(s->ctx, d_codes, n, s->min_count, s->part[s->parts - 1], found, &again);
}

static int files_kmer_set(dx_ctx *ctx, int kind, const uint8_t *const *imgs, const size_t *bytes, uint32_t nimg, uint32_t k, int canonical,
                          uint64_t min_count, uint64_t room, int counted, dx_kmer_set **set, dx_kmers64 *out, uint32_t *passes)
{ dx_kmers64   km;
  dx_kmer_set *made = NULL;
  set_fold     s;
  void        *d_all = NULL, *d_call = NULL;
  uint64_t     at = 0;
  uint32_t     np = 0, p;
  int          rc;
  if (ctx == NULL || set == NULL) return DX_E_ARG;
  *set = NULL;
  if ((rc = files_args(ctx, kind, imgs, bytes, nimg, k, canonical, set_files_fail)) != DX_OK) return rc;
  if (min_count < 1) return set_files_fail(ctx, DX_E_ARG, "min_count 0 (1 at least: the unseen codes are in no set)");

  fmark(NULL);
  memset(&s, 0, sizeof(s));
  s.ctx = ctx; s.min_count = min_count; s.report = out != NULL; s.counted = counted; s.km = &km;
  if ((s.part = calloc((1u << BINS_BITS) + 1, sizeof(*s.part))) == NULL || (s.len = calloc((1u << BINS_BITS) + 1, sizeof(*s.len))) == NULL ||
      (s.cpart = calloc((1u << BINS_BITS) + 1, sizeof(*s.cpart))) == NULL)
    { rc = DX_E_NOMEM; goto done; }                        /* (a range holds a bin at least) */
  TRY(files_passes(ctx, "dx_files_kmer_set", kind, imgs, bytes, nimg, k, canonical, room, &km, NULL, &np, set_range, &s));

  /* the ranges ascend: their arrays one behind the other are sorted and distinct */
  if (s.total) TRY(dx_malloc(ctx, (size_t) s.total * 8 + 64, &d_all));
  if (s.total && counted) TRY(dx_malloc(ctx, (size_t) s.total * 4 + 64, &d_call));
  for (p = 0; p < s.parts; p++)
    { TRY(dx_d2d(ctx, (uint64_t *) d_all + at, s.part[p], (size_t) s.len[p] * 8));
      if (counted) TRY(dx_d2d(ctx, (uint32_t *) d_call + at, s.cpart[p], (size_t) s.len[p] * 4));
      at += s.len[p];
      (void) dx_free(ctx, s.part[p]); s.part[p] = NULL;
      if (s.cpart[p]) { (void) dx_free(ctx, s.cpart[p]); s.cpart[p] = NULL; }
    }
  if (counted) TRY(dx_kmer_set_from_counted(ctx, d_all, d_call, s.total, k, canonical, kind == DX_KIND_ARROW, &made));
  else         TRY(dx_kmer_set_from_sorted(ctx, d_all, s.total, 1, k, canonical, kind == DX_KIND_ARROW, &made));
  fmark("the set made");
  if (out) *out = km;
  if (passes) *passes = np;
  *set = made;
  rc = DX_OK;

done:
  for (p = 0; s.part && s.cpart && p <= s.parts && p <= (1u << BINS_BITS); p++)      /* (a range that failed half made stands at s.parts) */
    { if (s.part[p]) (void) dx_free(ctx, s.part[p]);
      if (s.cpart[p]) (void) dx_free(ctx, s.cpart[p]);
    }
  if (d_all) (void) dx_free(ctx, d_all);
  if (d_call) (void) dx_free(ctx, d_call);
  free(s.part); free(s.cpart); free(s.len);
  fmark("the device arrays freed");
  return rc;
}

int dx_files_kmer_set(dx_ctx *ctx, int kind, const uint8_t *const *imgs, const size_t *bytes, uint32_t nimg, uint32_t k, int canonical,
                      uint64_t min_count, uint64_t room, dx_kmer_set **set, dx_kmers64 *out, uint32_t *passes)
{ return files_kmer_set(ctx, kind, imgs, bytes, nimg, k, canonical, min_count, room, 0, set, out, passes); }

int dx_files_kmer_set_counted(dx_ctx *ctx, int kind, const uint8_t *const *imgs, const size_t *bytes, uint32_t nimg, uint32_t k,
                              int canonical, uint64_t min_count, uint64_t room, dx_kmer_set **set, dx_kmers64 *out, uint32_t *passes)
{ return files_kmer_set(ctx, kind, imgs, bytes, nimg, k, canonical, min_count, room, 1, set, out, passes); }
