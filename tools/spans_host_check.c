/*
 * spans_host_check.c -- dx_spans_cut_plan (csrc/dx_file_cut.c) run alone, without a device, for a build under the sanitizers: cases made
 * by hand (touching and nested spans, a span over a whole record, spans at 0 and at the record's end, an empty span, records of length 0,
 * no spans, no records), the refusals, and random plans in the list's order (record, beg) and in any order, in all three modes with
 * min_len 0, 1, small and large.  Every plan is held against a second formulation that shares nothing with the first -- the record's
 * symbols marked one by one, the pieces read off as the runs of unmarked symbols -- and against dx_hits_cut_plan over the same triples.
 *
 *     spans_host_check [<random cases>]
 *
 * prints a line a group of cases; exits 1 when a plan differs, its ids decrease, a refusal is missing or a report figure is off.
 *
 * Build (csrc/dx_file_cut.c compiled here with the sanitizers; dx_file_cut's callees are taken from the library, which this program never
 * calls into):
 *     clang -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Idextractor_amd/csrc \
 *           tools/spans_host_check.c dextractor_amd/csrc/dx_file_cut.c -Ldextractor_amd -ldexgpu -Wl,-rpath,$PWD/dextractor_amd -o spans_host_check
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dexgpu.h"
#include "dx_host.h"

/* (find/dx_find_span.hip has it in the library, hidden: here no context has a text to keep) */
int dx_cut_fail(dx_ctx *ctx, int code, const char *what) { (void) ctx; (void) what; return code; }

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n)                            /* xorshift64*: 0 .. n - 1 */
{ rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return (uint32_t) (((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % n);
}

typedef struct { uint64_t id; uint32_t beg, end; } unit;

/* the plan by marking: per record every symbol of a span marked, the pieces the runs of unmarked symbols (the spans are not empty) */
static uint64_t marked_plan(const dx_span *s, uint64_t ns, const uint32_t *len, uint64_t records, uint32_t min_len, int mode, unit *out, dx_cut *cut)
{ uint64_t n = 0, r, k;
  memset(cut, 0, sizeof(*cut));
  cut->records_in = records;
  for (r = 0; r < records; r++)
    { uint8_t *mark = calloc((size_t) len[r] + 2, 1);
      uint32_t i, b, best_b = 0, best_e = 0, least = min_len ? min_len : 1;
      uint64_t first = n, hit = 0;
      if (mark == NULL) { fprintf(stderr, "out of memory\n"); exit(2); }
      cut->symbols_in += len[r];
      for (k = 0; k < ns; k++)
        if (s[k].record == r) { hit = 1; for (i = s[k].beg; i < s[k].end; i++) mark[i] = 1; }
      if (!hit) { out[n].id = r; out[n].beg = 0; out[n].end = len[r]; n++; cut->symbols_kept += len[r]; free(mark); continue; }
      for (i = 0; i < len[r]; i++) if (mark[i] && (i == 0 || !mark[i - 1])) cut->spans++;
      for (b = 0, i = 0; i <= len[r]; i++)
        if (i == len[r] || mark[i])
          { if (i > b && i - b >= least && mode != DX_CUT_DROP)
              { if (mode == DX_CUT_SPLIT) { out[n].id = r; out[n].beg = b; out[n].end = i; n++; }
                else if (i - b > best_e - best_b) { best_b = b; best_e = i; }
              }
            b = i + 1;
          }
      if (mode == DX_CUT_LONGEST && best_e > best_b) { out[n].id = r; out[n].beg = best_b; out[n].end = best_e; n++; }
      for (k = first; k < n; k++) cut->symbols_kept += out[k].end - out[k].beg;
      if (n > first) cut->records_cut++; else cut->records_dropped++;
      free(mark);
    }
  cut->pieces = n;
  return n;
}

static int same(const dx_span *s, uint64_t ns, const uint32_t *len, uint64_t records, uint32_t min_len, int mode)
{ uint64_t *ids, *hi, n, hn, k, total = records;
  uint32_t *beg, *end, *hb, *he, *st;
  dx_hit   *h;
  dx_cut    got, want, hcut;
  unit     *u;
  int       bad = 0, rc;
  for (k = 0; k < records; k++) total += len[k];
  u = malloc(((size_t) total + 1) * sizeof(*u)); h = malloc(((size_t) ns + 1) * sizeof(*h)); st = malloc(((size_t) ns + 1) * sizeof(*st));
  if (u == NULL || h == NULL || st == NULL) { fprintf(stderr, "out of memory\n"); exit(2); }
  for (k = 0; k < ns; k++) { memset(h + k, 0, sizeof(*h)); h[k].record = s[k].record; h[k].pos = s[k].end; st[k] = s[k].beg; }
  rc = dx_spans_cut_plan(s, ns, len, records, min_len, mode, &ids, &beg, &end, &n, &got);
  if (rc != DX_OK) { printf("  plan: error %d\n", rc); free(u); free(h); free(st); return 1; }
  if (n != marked_plan(s, ns, len, records, min_len, mode, u, &want)) bad = 1;
  for (k = 0; k < n && !bad; k++)
    { if (ids[k] != u[k].id || beg[k] != u[k].beg || end[k] != u[k].end) bad = 1;
      if (k && ids[k] < ids[k - 1]) bad = 1;
    }
  if (memcmp(&got, &want, sizeof(got))) bad = 1;
  /* the same triples as hits and starts: the same selection, the same report */
  if (dx_hits_cut_plan(h, st, ns, len, records, min_len, mode, &hi, &hb, &he, &hn, &hcut) != DX_OK || hn != n || memcmp(&hcut, &got, sizeof(got))) bad = 1;
  else if (n && (memcmp(hi, ids, (size_t) n * sizeof(*ids)) || memcmp(hb, beg, (size_t) n * sizeof(*beg)) || memcmp(he, end, (size_t) n * sizeof(*end)))) bad = 1;
  if (bad) printf("  DIFFERS: %" PRIu64 " spans, %" PRIu64 " records, min_len %u, mode %d\n", ns, records, min_len, mode);
  dx_file_free(ids); dx_file_free(beg); dx_file_free(end); dx_file_free(hi); dx_file_free(hb); dx_file_free(he);
  free(u); free(h); free(st);
  return bad;
}

static int all_modes(const dx_span *s, uint64_t ns, const uint32_t *len, uint64_t records)
{ static const uint32_t least[] = { 0, 1, 3, 9, 1000 };
  int bad = 0, mode;
  size_t i;
  for (mode = DX_CUT_SPLIT; mode <= DX_CUT_DROP; mode++)
    for (i = 0; i < sizeof(least) / sizeof(*least); i++) bad |= same(s, ns, len, records, least[i], mode);
  return bad;
}

static int by_hand(void)
{ static const uint32_t len[] = { 30, 0, 12, 40, 7, 20 };
  static const dx_span  sp[] = { { 0, 2, 8 }, { 0, 8, 12 }, { 0, 3, 5 }, { 0, 20, 25 }, { 2, 0, 12 }, { 3, 18, 22 }, { 3, 5, 23 }, { 3, 30, 31 },
                                 { 3, 10, 31 }, { 5, 0, 4 }, { 5, 15, 20 } };
  dx_span   e = { 0, 10, 10 };
  uint32_t *beg, *end;
  uint64_t *ids, n;
  dx_cut    cut;
  int       bad;
  bad = all_modes(sp, 11, len, 6);
  bad |= all_modes(NULL, 0, len, 6);                       /* no spans: every record whole */
  bad |= all_modes(NULL, 0, NULL, 0);                      /* no records */
  bad |= dx_spans_cut_plan(sp, 11, len, 6, 0, DX_CUT_SPLIT, &ids, &beg, &end, &n, &cut) != DX_OK;
  bad |= n != 8 || cut.records_cut != 3 || cut.records_dropped != 1 || cut.spans != 6 || cut.symbols_in != 109 || cut.symbols_kept != 47;
  dx_file_free(ids); dx_file_free(beg); dx_file_free(end);
  /* an empty span cuts nothing out and parts the record where it stands */
  bad |= dx_spans_cut_plan(&e, 1, len, 1, 0, DX_CUT_SPLIT, &ids, &beg, &end, &n, &cut) != DX_OK;
  bad |= n != 2 || beg[0] != 0 || end[0] != 10 || beg[1] != 10 || end[1] != 30 || cut.symbols_kept != 30;
  dx_file_free(ids); dx_file_free(beg); dx_file_free(end);
  /* ... and in a record of length 0 it leaves nothing */
  e.record = 1; e.beg = e.end = 0;
  bad |= dx_spans_cut_plan(&e, 1, len, 2, 0, DX_CUT_SPLIT, &ids, &beg, &end, &n, &cut) != DX_OK;
  bad |= n != 1 || ids[0] != 0 || cut.records_dropped != 1 || cut.spans != 1;
  dx_file_free(ids); dx_file_free(beg); dx_file_free(end);
  printf("by hand: %s\n", bad ? "BAD" : "ok");
  return bad;
}

static int refusals(void)
{ static const uint32_t len[] = { 10, 8 };
  dx_span   s[2] = { { 0, 2, 5 }, { 1, 3, 6 } };
  uint32_t *beg, *end;
  uint64_t *ids, n;
  int       bad = 0;
  bad |= dx_spans_cut_plan(s, 2, len, 2, 0, DX_CUT_SPLIT, &ids, &beg, &end, &n, NULL) != DX_OK || n != 4;
  dx_file_free(ids); dx_file_free(beg); dx_file_free(end);
  bad |= dx_spans_cut_plan(s, 2, len, 2, 0, 3, &ids, &beg, &end, &n, NULL) != DX_E_ARG;                 /* an unknown mode */
  bad |= dx_spans_cut_plan(s, 2, len, 2, 0, -1, &ids, &beg, &end, &n, NULL) != DX_E_ARG;
  bad |= dx_spans_cut_plan(s, 2, len, 1, 0, DX_CUT_SPLIT, &ids, &beg, &end, &n, NULL) != DX_E_ARG;      /* a record that is not there */
  s[0].beg = 6;
  bad |= dx_spans_cut_plan(s, 2, len, 2, 0, DX_CUT_SPLIT, &ids, &beg, &end, &n, NULL) != DX_E_ARG;      /* beg > end */
  s[0].beg = 2; s[1].end = 9;
  bad |= dx_spans_cut_plan(s, 2, len, 2, 0, DX_CUT_LONGEST, &ids, &beg, &end, &n, NULL) != DX_E_ARG;    /* end beyond the record */
  s[1].end = 6;
  bad |= dx_spans_cut_plan(NULL, 2, len, 2, 0, DX_CUT_SPLIT, &ids, &beg, &end, &n, NULL) != DX_E_ARG;
  bad |= dx_spans_cut_plan(s, 2, NULL, 2, 0, DX_CUT_SPLIT, &ids, &beg, &end, &n, NULL) != DX_E_ARG;
  bad |= dx_spans_cut_plan(s, 2, len, 2, 0, DX_CUT_SPLIT, NULL, &beg, &end, &n, NULL) != DX_E_ARG;
  bad |= dx_spans_cut_plan(s, 2, len, 2, 0, DX_CUT_SPLIT, &ids, &beg, &end, NULL, NULL) != DX_E_ARG;
  bad |= ids != NULL || beg != NULL || end != NULL;        /* a refusal hands nothing back */
  printf("refusals: %s\n", bad ? "BAD" : "ok");
  return bad;
}

static int by_record_beg(const void *a, const void *b)
{ const dx_span *x = a, *y = b;
  if (x->record != y->record) return x->record < y->record ? -1 : 1;
  return x->beg < y->beg ? -1 : x->beg > y->beg;
}

static int random_cases(uint32_t cases)
{ uint32_t c, k, bad = 0;
  for (c = 0; c < cases && !bad; c++)
    { const uint32_t records = 1 + rnd(12), ns = rnd(60);
      uint32_t len[12], n = 0;
      dx_span *s = malloc(((size_t) ns + 1) * sizeof(*s));
      if (s == NULL) { fprintf(stderr, "out of memory\n"); exit(2); }
      for (k = 0; k < records; k++) len[k] = rnd(4) ? rnd(80) : 0;
      for (k = 0; k < ns; k++)
        { const uint32_t r = rnd(records);
          if (len[r] == 0) continue;
          s[n].record = r; s[n].end = 1 + rnd(len[r]);     /* 1 <= end <= len */
          s[n].beg = s[n].end - 1 - rnd(s[n].end < 12 ? s[n].end : 12);      /* a span of 1 to 12 symbols */
          n++;
        }
      if (c & 1) qsort(s, n, sizeof(*s), by_record_beg);   /* the list's own order, or any */
      bad |= all_modes(s, n, len, records);
      free(s);
    }
  printf("random: %u cases: %s\n", c, bad ? "BAD" : "ok");
  return (int) bad;
}

int main(int argc, char **argv)
{ const uint32_t cases = argc > 1 ? (uint32_t) strtoul(argv[1], NULL, 10) : 2000;
  int bad = by_hand();
  bad |= refusals();
  bad |= random_cases(cases);
  return bad;
}
