/*
 * dx_file_cut.c -- what is kept of the records of an image once the occurrences of given sequences are cut out of them, and the image of
 * it: dx_hits_cut_plan, dx_spans_cut_plan (host), dx_file_cut.
 *
 * Everything one does with a found adapter or primer needs both of its ends: cutting it out, splitting a chimeric subread at a missed
 * SMRTbell adapter, dropping the read.  dx_file_find_edit_spans has both ends (the starts by dx_code_hit_starts, on the device, while a
 * slice's hits are still there), and dx_file_subset writes, byte for byte, the file dexta / dexar / dexqv would write for a cut text, the
 * B_E of every header rewritten as dextract names the subreads of a well.  Between the two stands only a plan, and it is this file's:
 * per record the spans [start, pos) of all patterns and strands united, and the pieces between them chosen by the mode.  Today the
 * step takes undexta of the whole file, a text scan on one core and dexta again -- and the same for the .dexar and the .dexqv of the run,
 * for which dx_file_cut hands its selection back.
 *
 * The plan needs no device and no context (tools/cut_host_check.c runs it under the sanitizers).  It works on (record, beg, end) triples,
 * so the spans of a k-mer screen (dx_file_screen_spans.c) get the same plan through dx_spans_cut_plan (tools/spans_host_check.c).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dexgpu.h"
#include "dx_host.h"
#include "dx_env.h"
#include "dx_files.h"

static int by_record_beg(const void *a, const void *b)
{ const dx_span *x = a, *y = b;
  if (x->record != y->record) return x->record < y->record ? -1 : 1;
  if (x->beg != y->beg) return x->beg < y->beg ? -1 : 1;
  return x->end < y->end ? -1 : x->end > y->end;
}

/* one unit more, the arrays grown as need be */
static int keep(uint64_t **ids, uint32_t **beg, uint32_t **end, uint64_t *n, uint64_t *cap, uint64_t id, uint32_t b, uint32_t e)
{ if (*n == *cap)
    { const uint64_t want = *cap ? 2 * *cap : 256;
      uint64_t *i2 = realloc(*ids, (size_t) want * sizeof(**ids));
      uint32_t *b2, *e2;
      if (i2 == NULL) return DX_E_NOMEM;
      *ids = i2;
      if ((b2 = realloc(*beg, (size_t) want * sizeof(**beg))) == NULL) return DX_E_NOMEM;
      *beg = b2;
      if ((e2 = realloc(*end, (size_t) want * sizeof(**end))) == NULL) return DX_E_NOMEM;
      *end = e2;
      *cap = want;
    }
  (*ids)[*n] = id; (*beg)[*n] = b; (*end)[*n] = e; (*n)++;
  return DX_OK;
}

/* the plan of n spans (sp: the plan's own copy, sorted here; every one inside its record) over `records` records: what both entry points
   share.  The outputs are the caller's, emptied already; mode is one of the three */
static int plan_spans(dx_span *sp, uint64_t n_hits, const uint32_t *rec_len, uint64_t records, uint32_t min_len, int mode,
                      uint64_t **ids, uint32_t **beg, uint32_t **end, uint64_t *n_ids, dx_cut *report)
{ const uint32_t least = min_len ? min_len : 1;            /* a piece has one symbol at least */
  uint64_t *oi = NULL, n = 0, cap = 0, r, k = 0;
  uint32_t *ob = NULL, *oe = NULL;
  dx_cut    cut;
  int       rc;
  memset(&cut, 0, sizeof(cut));
  cut.records_in = records;
  qsort(sp, (size_t) n_hits, sizeof(*sp), by_record_beg);  /* (a list of hits comes by (record, pos): not by start) */

  for (r = 0; r < records; r++)
    { const uint32_t len = rec_len[r];
      uint32_t at = 0, best_b = 0, best_e = 0;             /* where the piece in the making begins; LONGEST: the best so far */
      uint64_t kept = 0;
      cut.symbols_in += len;
      if (k == n_hits || sp[k].record != r)                /* no occurrence: whole, whatever min_len is */
        { TRY(keep(&oi, &ob, &oe, &n, &cap, r, 0, len));
          cut.symbols_kept += len;
          continue;
        }
      while (k < n_hits && sp[k].record == r)
        { const uint32_t b = sp[k].beg;                    /* one united span [b, e): everything that overlaps or touches it */
          uint32_t e = sp[k].end;
          for (k++; k < n_hits && sp[k].record == r && sp[k].beg <= e; k++)
            if (sp[k].end > e) e = sp[k].end;
          cut.spans++;
          if (mode == DX_CUT_SPLIT && b - at >= least)
            { TRY(keep(&oi, &ob, &oe, &n, &cap, r, at, b)); kept++; cut.symbols_kept += b - at; }
          if (mode == DX_CUT_LONGEST && b - at >= least && b - at > best_e - best_b) { best_b = at; best_e = b; }
          at = e;
        }
      if (mode == DX_CUT_SPLIT && len - at >= least)
        { TRY(keep(&oi, &ob, &oe, &n, &cap, r, at, len)); kept++; cut.symbols_kept += len - at; }
      if (mode == DX_CUT_LONGEST)
        { if (len - at >= least && len - at > best_e - best_b) { best_b = at; best_e = len; }
          if (best_e > best_b) { TRY(keep(&oi, &ob, &oe, &n, &cap, r, best_b, best_e)); kept++; cut.symbols_kept += best_e - best_b; }
        }
      if (kept) cut.records_cut++; else cut.records_dropped++;
    }
  cut.pieces = n;
  if (oi == NULL)                                          /* (nothing kept: arrays all the same, for dx_file_free) */
    { oi = malloc(sizeof(*oi)); ob = malloc(sizeof(*ob)); oe = malloc(sizeof(*oe));
      if (oi == NULL || ob == NULL || oe == NULL) { rc = DX_E_NOMEM; goto done; }
    }
  *ids = oi; *beg = ob; *end = oe; *n_ids = n;
  oi = NULL; ob = NULL; oe = NULL;
  if (report) *report = cut;
  rc = DX_OK;

done:
  free(oi); free(ob); free(oe);
  return rc;
}

/* what both entry points ask of their arguments before they look at a span; the outputs emptied */
static int plan_args(const void *a, const void *b, uint64_t n, const uint32_t *rec_len, uint64_t records, int mode,
                     uint64_t **ids, uint32_t **beg, uint32_t **end, uint64_t *n_ids, dx_cut *report)
{ if (ids == NULL || beg == NULL || end == NULL || n_ids == NULL) return DX_E_ARG;
  *ids = NULL; *beg = NULL; *end = NULL; *n_ids = 0;
  if (report) memset(report, 0, sizeof(*report));
  if (mode != DX_CUT_SPLIT && mode != DX_CUT_LONGEST && mode != DX_CUT_DROP) return DX_E_ARG;
  if ((n && (a == NULL || b == NULL)) || (records && rec_len == NULL)) return DX_E_ARG;
  return DX_OK;
}

int dx_hits_cut_plan(const dx_hit *hits, const uint32_t *start, uint64_t n_hits, const uint32_t *rec_len, uint64_t records,
                     uint32_t min_len, int mode, uint64_t **ids, uint32_t **beg, uint32_t **end, uint64_t *n_ids, dx_cut *report)
{ dx_span *sp;
  uint64_t h;
  int      rc;
  if ((rc = plan_args(hits, start, n_hits, rec_len, records, mode, ids, beg, end, n_ids, report)) != DX_OK) return rc;
  if ((sp = malloc(((size_t) n_hits + 1) * sizeof(*sp))) == NULL) return DX_E_NOMEM;
  for (h = 0; h < n_hits; h++)
    { if (hits[h].record >= records || start[h] > hits[h].pos || hits[h].pos > rec_len[hits[h].record]) { rc = DX_E_ARG; goto done; }
      sp[h].record = hits[h].record; sp[h].beg = start[h]; sp[h].end = hits[h].pos;
    }
  rc = plan_spans(sp, n_hits, rec_len, records, min_len, mode, ids, beg, end, n_ids, report);

done:
  free(sp);
  return rc;
}

int dx_spans_cut_plan(const dx_span *spans, uint64_t n, const uint32_t *rec_len, uint64_t records, uint32_t min_len, int mode,
                      uint64_t **ids, uint32_t **beg, uint32_t **end, uint64_t *n_ids, dx_cut *report)
{ dx_span *sp;
  uint64_t h;
  int      rc;
  if ((rc = plan_args(spans, spans, n, rec_len, records, mode, ids, beg, end, n_ids, report)) != DX_OK) return rc;
  if ((sp = malloc(((size_t) n + 1) * sizeof(*sp))) == NULL) return DX_E_NOMEM;
  for (h = 0; h < n; h++)
    { if (spans[h].record >= records || spans[h].beg > spans[h].end || spans[h].end > rec_len[spans[h].record]) { rc = DX_E_ARG; goto done; }
      sp[h] = spans[h];
    }
  rc = plan_spans(sp, n, rec_len, records, min_len, mode, ids, beg, end, n_ids, report);

done:
  free(sp);
  return rc;
}

int dx_file_cut(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, const char *const *pattern, uint32_t npat, uint32_t max_err,
                int both_strands, uint32_t min_len, int mode, uint8_t **out, size_t *out_len, dx_cut *report,
                uint64_t **ids, uint32_t **beg, uint32_t **end, uint64_t *n_ids)
{ dx_find   fd;
  dx_hit   *hits = NULL;
  uint32_t *start = NULL, *rlen = NULL, *sb = NULL, *se = NULL;
  uint64_t *si = NULL, n = 0;
  dx_cut    cut;
  /* (DEXGPU_TEST cut_max_hits: a list that ends early, which no file small enough for a test gives) */
  const uint64_t most = (uint64_t) dx_test_num("cut_max_hits", -1);
  int       rc;

  if (ctx == NULL || out == NULL || out_len == NULL || (img == NULL && m)) return DX_E_ARG;
  *out = NULL; *out_len = 0;
  if (ids) *ids = NULL;
  if (beg) *beg = NULL;
  if (end) *end = NULL;
  if (n_ids) *n_ids = 0;
  if (report) memset(report, 0, sizeof(*report));
  if (mode != DX_CUT_SPLIT && mode != DX_CUT_LONGEST && mode != DX_CUT_DROP) return dx_cut_fail(ctx, DX_E_ARG, "unknown mode");
  if (kind == DX_KIND_QUIVA)
    return dx_cut_fail(ctx, DX_E_ARG, "a .dexqv image has no packed reads to search: cut the .dexta of the same records, then apply the selection with dx_file_subset");

  TRY(dx_file_find_edit_spans(ctx, kind, img, m, pattern, npat, max_err, both_strands, most, &fd, &hits, NULL, &start, &rlen));
  if (fd.listed < fd.hits)
    { char why[160];
      snprintf(why, sizeof(why), "%llu of %llu hits were listed: nothing is cut from part of them", (unsigned long long) fd.listed,
               (unsigned long long) fd.hits);
      rc = dx_cut_fail(ctx, DX_E_NOMEM, why);
      goto done;
    }
  rc = dx_hits_cut_plan(hits, start, fd.listed, rlen, fd.records, min_len, mode, &si, &sb, &se, &n, &cut);
  if (rc != DX_OK) { rc = dx_cut_fail(ctx, rc, "the hits do not make a plan"); goto done; }
  if (n == 0)
    { rc = dx_cut_fail(ctx, DX_E_DEGENERATE, fd.records ? "nothing is kept of any record" : "the image has no records");
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
  free(hits); free(start); free(rlen); free(si); free(sb); free(se);
  return rc;
}
