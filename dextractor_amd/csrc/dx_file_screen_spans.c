/*
 * dx_file_screen_spans.c -- WHERE the records of a .dexta / .dexar image match a set of k-mers on the device, as joined intervals:
 * dx_file_screen_spans; and the image with those intervals cut out of its records, or kept alone: dx_file_screen_cut.
 *
 * dx_file_screen says which records share k-mers with the set; what one does with a vector, a control or an organelle inside a
 * chimeric subread, with the repeats of a read, or with "the part that matches the target" needs the places.  The image is opened,
 * walked and sliced as dx_file_screen does it (dxf_image_open, dxf_u2_cap, dxf_u2_slices; 4 bytes a record of the hook's own: the
 * record's raw spans).  Per slice the raw spans are counted (dx_code_kmer_spans with no list), a device list of exactly that size
 * is taken, the list is made from the counts that are there (dx_spans_list_counted: the look-ups once more, not twice), the spans the
 * join and the filter keep are counted (dx_spans_join with no list), a second list of exactly that size is taken and filled, and only
 * the joined, kept spans come down, their record numbers moved by the slice's first record.  A record lies in one slice, so no join
 * crosses a slice and the answer does not depend on the slicing; the order and max_spans run across slices as max_hits does in
 * dx_file_find.
 *
 * dx_file_screen_cut is dx_file_screen_spans with every span listed, dx_spans_cut_plan (dx_file_cut.c) and dx_file_subset, as
 * dx_file_cut is for the occurrences of patterns.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dexgpu.h"
#include "dx_host.h"
#include "dx_files.h"

#define WHO_SPANS "dx_file_screen_spans"
#define WHO_CUT   "dx_file_screen_cut"

/* DEXGPU_TIMING=1: where the driver spends its time (stderr) */
static void smark(const char *what)
{ static double t0 = -1.0;
  dx_mark("screen_spans", &t0, what);
}

/* what the slices add up to, the list they fill and the two device lists of one slice: its raw spans, its joined and kept ones */
typedef struct
  { dx_ctx *ctx; const dx_kmer_set *set; const char *who;
    uint32_t max_gap, min_span;
    uint64_t keep;                /* spans the list is to hold */
    uint64_t covered, records_hit, raw, spans, symbols, listed;
    dx_span *list; uint64_t list_cap;
    uint32_t *rec;                /* kept spans a record, or NULL */
    void *d_list, *d_kept; size_t d_cap, d_kept_cap;
  } spans_job;

/* a device list of exactly n spans at *p (the one of the slice before serves when it is large enough); DX_E_NOMEM names the bytes */
static int spans_room(spans_job *j, void **p, size_t *cap, uint64_t n, const char *what)
{ char why[120];
  if (dgrow(j->ctx, p, cap, (size_t) n * sizeof(dx_span)) == DX_OK) return DX_OK;
  snprintf(why, sizeof(why), "no %llu bytes of device memory for %s", (unsigned long long) (n * sizeof(dx_span)), what);
  return dx_screen_spans_fail(j->ctx, DX_E_NOMEM, j->who, why);
}

/* a slice of the image's packed reads (dxf_u2_slices): its spans counted, listed, joined, and the kept ones brought down */
static int spans_slice(void *arg, const u2_slice *s)
{ spans_job *j = arg;
  dx_ctx    *ctx = j->ctx;
  uint64_t   t[3], jt[2], listed = 0, want;
  dx_span   *d_raw, *d_out;
  int        rc;
  if ((rc = dx_code_kmer_spans(ctx, s->d_in, s->bytes, s->d_boff, NULL, s->d_len, s->n, j->set, s->d_extra, NULL, 0, t, NULL)) != DX_OK) return rc;
  j->raw += t[0]; j->covered += t[1]; j->records_hit += t[2];
  if (t[0] == 0) return DX_OK;
  if (t[0] > 0xffffffffull)
    return dx_screen_spans_fail(ctx, DX_E_NOMEM, j->who, "more than 2^32 - 1 raw spans in one slice: lower DEXGPU_TEXT_BUDGET");
  if ((rc = spans_room(j, &j->d_list, &j->d_cap, t[0], "the raw spans of a slice")) != DX_OK) return rc;
  d_raw = j->d_list;
  if ((rc = dx_spans_list_counted(ctx, s->d_in, s->bytes, s->d_boff, s->d_len, s->n, j->set, s->d_extra, d_raw, t[0], &listed)) != DX_OK) return rc;
  if ((rc = dx_spans_join(ctx, d_raw, t[0], j->max_gap, j->min_span, NULL, 0, jt, NULL)) != DX_OK) return rc;      /* how many are kept */
  j->spans += jt[0]; j->symbols += jt[1];
  if (jt[0] == 0) return DX_OK;
  if ((rc = spans_room(j, &j->d_kept, &j->d_kept_cap, jt[0], "the joined spans of a slice")) != DX_OK) return rc;
  d_out = j->d_kept;
  if ((rc = dx_spans_join(ctx, d_raw, t[0], j->max_gap, j->min_span, d_out, jt[0], jt, NULL)) != DX_OK) return rc;

  /* down: all the slice's kept spans when somebody counts them by record, else what the list still takes */
  want = j->keep - j->listed < jt[0] ? j->keep - j->listed : jt[0];
  if (j->rec != NULL || want)
    { const uint64_t down = j->rec != NULL ? jt[0] : want;
      dx_span *h;
      uint64_t i;
      if (j->listed + down > j->list_cap)
        { const uint64_t cap = j->listed + down > 2 * j->list_cap ? j->listed + down : 2 * j->list_cap;
          dx_span *bigger = realloc(j->list, (size_t) cap * sizeof(*bigger));
          if (bigger == NULL) return DX_E_NOMEM;
          j->list = bigger; j->list_cap = cap;
        }
      h = j->list + j->listed;                             /* (what lies behind `want` is the next slice's to overwrite) */
      if (down && (rc = dx_d2h(ctx, h, d_out, (size_t) down * sizeof(*h))) != DX_OK) return rc;
      for (i = 0; i < down; i++)
        { if (j->rec != NULL) j->rec[s->i0 + h[i].record]++;
          h[i].record += s->i0;
        }
      j->listed += want;
    }
  return DX_OK;
}

int dx_file_screen_spans(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, const dx_kmer_set *set,
                         uint32_t max_gap, uint32_t min_span, uint64_t max_spans, dx_spans_report *out,
                         dx_span **spans, uint32_t **rec_spans, uint32_t **rec_len)
{ image_text       im;
  dx_set_info      si;
  dx_spans_report  rp;
  spans_job        j;
  uint32_t        *rl = NULL;
  uint64_t         cnt, i;
  size_t           cap;
  const u2_index  *x;
  int              rc;
  if (ctx == NULL || out == NULL || (img == NULL && m)) return DX_E_ARG;
  if (spans) *spans = NULL;
  if (rec_spans) *rec_spans = NULL;
  if (rec_len) *rec_len = NULL;
  if (kind == DX_KIND_QUIVA)
    return dx_screen_spans_fail(ctx, DX_E_ARG, WHO_SPANS, "a .dexqv image has no packed reads to screen (DX_KIND_FASTA or DX_KIND_ARROW)");
  if (kind != DX_KIND_FASTA && kind != DX_KIND_ARROW) return dx_screen_spans_fail(ctx, DX_E_ARG, WHO_SPANS, "unknown kind");
  if (dx_kmer_set_info(set, &si) != DX_OK) return dx_screen_spans_fail(ctx, DX_E_ARG, WHO_SPANS, "no set");
  if ((si.arrow != 0) != (kind == DX_KIND_ARROW))
    return dx_screen_spans_fail(ctx, DX_E_ARG, WHO_SPANS, si.arrow ? "a set of pulse widths against a .dexta image" : "a set of bases against a .dexar image");
  memset(&rp, 0, sizeof(rp));
  rp.k = si.k;
  memset(&j, 0, sizeof(j));

  smark(NULL);
  TRY(dxf_image_open(ctx, kind, 0, 1, img, m, &im));       /* (the line width lays out a text nobody makes) */
  x = &im.ux; cnt = x->cnt;
  rp.records = cnt;
  for (i = 0; i < cnt; i++) rp.symbols += x->nsym[i];
  cap = cnt ? dxf_u2_cap(ctx, m, cnt) : 0;
  if (rec_spans != NULL && (j.rec = calloc((size_t) (cnt ? cnt : 1), sizeof(*j.rec))) == NULL) { rc = DX_E_NOMEM; goto done; }
  if (rec_len != NULL)
    { if ((rl = malloc((size_t) (cnt ? cnt : 1) * sizeof(*rl))) == NULL) { rc = DX_E_NOMEM; goto done; }
      if (cnt) memcpy(rl, x->nsym, (size_t) cnt * sizeof(*rl));
    }
  smark("the image walked");
  j.ctx = ctx; j.set = set; j.who = WHO_SPANS; j.max_gap = max_gap; j.min_span = min_span;
  j.keep = spans != NULL ? max_spans : 0;                  /* spans the list is to hold (nobody takes it: none) */
  TRY(dxf_u2_slices(ctx, img, x, cap, sizeof(uint32_t), spans_slice, &j));
  smark("the slices up, their spans listed and joined, the kept ones back");
  rp.covered = j.covered; rp.records_hit = j.records_hit; rp.raw_spans = j.raw;
  rp.spans = j.spans; rp.span_symbols = j.symbols; rp.listed = j.listed;
  if (spans != NULL && j.list == NULL && (j.list = malloc(sizeof(*j.list))) == NULL) { rc = DX_E_NOMEM; goto done; }

  *out = rp;
  if (spans) { *spans = j.list; j.list = NULL; }
  if (rec_spans) { *rec_spans = j.rec; j.rec = NULL; }
  if (rec_len) { *rec_len = rl; rl = NULL; }
  rc = DX_OK;

done:
  dxf_image_close(&im);
  if (j.d_list) (void) dx_free(ctx, j.d_list);
  if (j.d_kept) (void) dx_free(ctx, j.d_kept);
  free(j.list); free(j.rec); free(rl);
  return rc;
}

int dx_file_screen_cut(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, const dx_kmer_set *set,
                       uint32_t max_gap, uint32_t min_span, uint32_t min_len, int mode,
                       uint8_t **out, size_t *out_len, dx_cut *report, uint64_t **ids, uint32_t **beg, uint32_t **end, uint64_t *n_ids)
{ dx_spans_report rp;
  dx_span  *sp = NULL;
  uint32_t *rlen = NULL, *sb = NULL, *se = NULL;
  uint64_t *si = NULL, n = 0;
  dx_cut    cut;
  int       rc;

  if (ctx == NULL || out == NULL || out_len == NULL || (img == NULL && m)) return DX_E_ARG;
  *out = NULL; *out_len = 0;
  if (ids) *ids = NULL;
  if (beg) *beg = NULL;
  if (end) *end = NULL;
  if (n_ids) *n_ids = 0;
  if (report) memset(report, 0, sizeof(*report));
  if (mode != DX_CUT_SPLIT && mode != DX_CUT_LONGEST && mode != DX_CUT_DROP) return dx_screen_spans_fail(ctx, DX_E_ARG, WHO_CUT, "unknown mode");
  if (kind == DX_KIND_QUIVA)
    return dx_screen_spans_fail(ctx, DX_E_ARG, WHO_CUT, "a .dexqv image has no packed reads to screen: cut the .dexta of the same records, then apply the selection with dx_file_subset");

  TRY(dx_file_screen_spans(ctx, kind, img, m, set, max_gap, min_span, UINT64_MAX, &rp, &sp, NULL, &rlen));
  if (rp.listed < rp.spans)
    { char why[160];
      snprintf(why, sizeof(why), "%llu of %llu spans were listed: nothing is cut from part of them", (unsigned long long) rp.listed,
               (unsigned long long) rp.spans);
      rc = dx_screen_spans_fail(ctx, DX_E_NOMEM, WHO_CUT, why);
      goto done;
    }
  rc = dx_spans_cut_plan(sp, rp.listed, rlen, rp.records, min_len, mode, &si, &sb, &se, &n, &cut);
  if (rc != DX_OK) { rc = dx_screen_spans_fail(ctx, rc, WHO_CUT, "the spans do not make a plan"); goto done; }
  if (n == 0)
    { rc = dx_screen_spans_fail(ctx, DX_E_DEGENERATE, WHO_CUT, rp.records ? "nothing is kept of any record" : "the image has no records");
      goto done;
    }
  TRY(dx_file_subset(ctx, kind, img, m, si, sb, se, n, 0, out, out_len));
  if (report) *report = cut;
  if (ids) { *ids = si; si = NULL; }
  if (beg) { *beg = sb; sb = NULL; }
  if (end) { *end = se; se = NULL; }
  if (n_ids) *n_ids = n;
  rc = DX_OK;

done:
  free(sp); free(rlen); free(si); free(sb); free(se);
  return rc;
}
