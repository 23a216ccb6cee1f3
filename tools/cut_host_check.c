/*
 * cut_host_check.c -- the host part of dx_file_cut (csrc/dx_file_cut.c: dx_hits_cut_plan) run alone, without a device, for a build under
 * the sanitizers: cases made by hand (touching and nested spans, a span over a whole record, hits of two patterns interleaved, records
 * without hits, no hits, no records, an empty span), the refusals, and random inputs in the list's order (record, pos) and in any
 * order, in all three modes with min_len 0, 1, small and large.  Every plan is held against a second formulation that shares nothing
 * with the first: the record's symbols marked one by one, the pieces read off as the runs of unmarked symbols.
 *
 *     cut_host_check [<random cases>]
 *
 * prints a line a group of cases; exits 1 when a plan differs from the marked one, its ids decrease, a refusal is missing or a report
 * figure is off.
 *
 * Build (csrc/dx_file_cut.c compiled here with the sanitizers; dx_file_cut's callees are taken from the library, which this program never
 * calls into):
 *     clang -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Idextractor_amd/csrc \
 *           tools/cut_host_check.c dextractor_amd/csrc/dx_file_cut.c -Ldextractor_amd -ldexgpu -Wl,-rpath,$PWD/dextractor_amd -o cut_host_check
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
static uint64_t marked_plan(const dx_hit *h, const uint32_t *st, uint64_t nh, const uint32_t *len, uint64_t records, uint32_t min_len, int mode,
                            unit *out, dx_cut *cut)
{ uint64_t n = 0, r, k;
  memset(cut, 0, sizeof(*cut));
  cut->records_in = records;
  for (r = 0; r < records; r++)
    { uint8_t *mark = calloc((size_t) len[r] + 2, 1);
      uint32_t i, b, best_b = 0, best_e = 0, least = min_len ? min_len : 1;
      uint64_t first = n, hit = 0;
      if (mark == NULL) { fprintf(stderr, "out of memory\n"); exit(2); }
      cut->symbols_in += len[r];
      for (k = 0; k < nh; k++)
        if (h[k].record == r) { hit = 1; for (i = st[k]; i < h[k].pos; i++) mark[i] = 1; }
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

static int same(const dx_hit *h, const uint32_t *st, uint64_t nh, const uint32_t *len, uint64_t records, uint32_t min_len, int mode)
{ uint64_t *ids, n, k, total = records;
  uint32_t *beg, *end;
  dx_cut    got, want;
  unit     *u;
  int       bad = 0, rc;
  for (k = 0; k < records; k++) total += len[k];
  if ((u = malloc(((size_t) total + 1) * sizeof(*u))) == NULL) { fprintf(stderr, "out of memory\n"); exit(2); }
  rc = dx_hits_cut_plan(h, st, nh, len, records, min_len, mode, &ids, &beg, &end, &n, &got);
  if (rc != DX_OK) { printf("  plan: error %d\n", rc); free(u); return 1; }
  if (n != marked_plan(h, st, nh, len, records, min_len, mode, u, &want)) bad = 1;
  for (k = 0; k < n && !bad; k++)
    { if (ids[k] != u[k].id || beg[k] != u[k].beg || end[k] != u[k].end) bad = 1;
      if (k && ids[k] < ids[k - 1]) bad = 1;
    }
  if (memcmp(&got, &want, sizeof(got))) bad = 1;
  if (bad) printf("  DIFFERS: %" PRIu64 " hits, %" PRIu64 " records, min_len %u, mode %d\n", nh, records, min_len, mode);
  dx_file_free(ids); dx_file_free(beg); dx_file_free(end);
  free(u);
  return bad;
}

static int all_modes(const dx_hit *h, const uint32_t *st, uint64_t nh, const uint32_t *len, uint64_t records)
{ static const uint32_t least[] = { 0, 1, 3, 9, 1000 };
  int bad = 0, mode;
  size_t i;
  for (mode = DX_CUT_SPLIT; mode <= DX_CUT_DROP; mode++)
    for (i = 0; i < sizeof(least) / sizeof(*least); i++) bad |= same(h, st, nh, len, records, least[i], mode);
  return bad;
}

static dx_hit hit(uint64_t record, uint32_t pos) { dx_hit h = { record, pos, 0, 0, 0 }; return h; }

static int by_hand(void)
{ static const uint32_t len[] = { 30, 0, 12, 40, 7, 20 };
  static const uint32_t span[][3] = { { 0, 2, 8 }, { 0, 8, 12 }, { 0, 3, 5 }, { 0, 20, 25 }, { 2, 0, 12 }, { 3, 18, 22 }, { 3, 5, 23 }, { 3, 30, 31 },
                                      { 3, 10, 31 }, { 5, 0, 4 }, { 5, 15, 20 } };
  dx_hit    h[11];
  uint32_t  st[11], *beg, *end;
  uint64_t *ids, n, k;
  dx_cut    cut;
  int       bad;
  for (k = 0; k < 11; k++) { h[k] = hit(span[k][0], span[k][2]); st[k] = span[k][1]; }
  bad = all_modes(h, st, 11, len, 6);
  bad |= all_modes(NULL, NULL, 0, len, 6);                 /* no hits: every record whole */
  bad |= all_modes(NULL, NULL, 0, NULL, 0);                /* no records */
  bad |= dx_hits_cut_plan(h, st, 11, len, 6, 0, DX_CUT_SPLIT, &ids, &beg, &end, &n, &cut) != DX_OK;
  bad |= n != 8 || cut.records_cut != 3 || cut.records_dropped != 1 || cut.spans != 6 || cut.symbols_in != 109 || cut.symbols_kept != 47;
  dx_file_free(ids); dx_file_free(beg); dx_file_free(end);
  /* an empty span cuts nothing out and parts the record where it stands */
  h[0] = hit(0, 10); st[0] = 10;
  bad |= dx_hits_cut_plan(h, st, 1, len, 1, 0, DX_CUT_SPLIT, &ids, &beg, &end, &n, &cut) != DX_OK;
  bad |= n != 2 || beg[0] != 0 || end[0] != 10 || beg[1] != 10 || end[1] != 30 || cut.symbols_kept != 30;
  dx_file_free(ids); dx_file_free(beg); dx_file_free(end);
  printf("by hand: %s\n", bad ? "BAD" : "ok");
  return bad;
}

static int refusals(void)
{ static const uint32_t len[] = { 10, 8 };
  dx_hit    h[2];
  uint32_t  st[2] = { 2, 3 }, *beg, *end;
  uint64_t *ids, n;
  int       bad = 0;
  h[0] = hit(0, 5); h[1] = hit(1, 6);
  bad |= dx_hits_cut_plan(h, st, 2, len, 2, 0, DX_CUT_SPLIT, &ids, &beg, &end, &n, NULL) != DX_OK || n != 4;
  dx_file_free(ids); dx_file_free(beg); dx_file_free(end);
  bad |= dx_hits_cut_plan(h, st, 2, len, 2, 0, 3, &ids, &beg, &end, &n, NULL) != DX_E_ARG;               /* an unknown mode */
  bad |= dx_hits_cut_plan(h, st, 2, len, 2, 0, -1, &ids, &beg, &end, &n, NULL) != DX_E_ARG;
  bad |= dx_hits_cut_plan(h, st, 2, len, 1, 0, DX_CUT_SPLIT, &ids, &beg, &end, &n, NULL) != DX_E_ARG;    /* a record that is not there */
  st[0] = 6;
  bad |= dx_hits_cut_plan(h, st, 2, len, 2, 0, DX_CUT_SPLIT, &ids, &beg, &end, &n, NULL) != DX_E_ARG;    /* start > pos */
  st[0] = UINT32_MAX;
  bad |= dx_hits_cut_plan(h, st, 2, len, 2, 0, DX_CUT_DROP, &ids, &beg, &end, &n, NULL) != DX_E_ARG;     /* a bad hit's start */
  st[0] = 2; h[1].pos = 9;
  bad |= dx_hits_cut_plan(h, st, 2, len, 2, 0, DX_CUT_LONGEST, &ids, &beg, &end, &n, NULL) != DX_E_ARG;  /* pos beyond the record */
  h[1].pos = 6;
  bad |= dx_hits_cut_plan(NULL, st, 2, len, 2, 0, DX_CUT_SPLIT, &ids, &beg, &end, &n, NULL) != DX_E_ARG;
  bad |= dx_hits_cut_plan(h, NULL, 2, len, 2, 0, DX_CUT_SPLIT, &ids, &beg, &end, &n, NULL) != DX_E_ARG;
  bad |= dx_hits_cut_plan(h, st, 2, NULL, 2, 0, DX_CUT_SPLIT, &ids, &beg, &end, &n, NULL) != DX_E_ARG;
  bad |= dx_hits_cut_plan(h, st, 2, len, 2, 0, DX_CUT_SPLIT, NULL, &beg, &end, &n, NULL) != DX_E_ARG;
  bad |= dx_hits_cut_plan(h, st, 2, len, 2, 0, DX_CUT_SPLIT, &ids, &beg, &end, NULL, NULL) != DX_E_ARG;
  bad |= ids != NULL || beg != NULL || end != NULL;        /* a refusal hands nothing back */
  printf("refusals: %s\n", bad ? "BAD" : "ok");
  return bad;
}

static int by_record_pos(const void *a, const void *b)
{ const uint32_t *x = a, *y = b;                           /* (record, start, pos) triples */
  if (x[0] != y[0]) return x[0] < y[0] ? -1 : 1;
  return x[2] < y[2] ? -1 : x[2] > y[2];
}

static int random_cases(uint32_t cases)
{ uint32_t c, k, bad = 0;
  for (c = 0; c < cases && !bad; c++)
    { const uint32_t records = 1 + rnd(12), nh = rnd(60);
      uint32_t len[12], (*t)[3] = malloc(((size_t) nh + 1) * sizeof(*t)), *st = malloc(((size_t) nh + 1) * sizeof(*st));
      dx_hit  *h = malloc(((size_t) nh + 1) * sizeof(*h));
      uint32_t n = 0;
      if (t == NULL || st == NULL || h == NULL) { fprintf(stderr, "out of memory\n"); exit(2); }
      for (k = 0; k < records; k++) len[k] = rnd(4) ? rnd(80) : 0;
      for (k = 0; k < nh; k++)
        { const uint32_t r = rnd(records);
          if (len[r] == 0) continue;
          t[n][0] = r; t[n][2] = 1 + rnd(len[r]);          /* 1 <= pos <= len */
          t[n][1] = t[n][2] - 1 - rnd(t[n][2] < 12 ? t[n][2] : 12);      /* a span of 1 to 12 symbols */
          n++;
        }
      if (c & 1) qsort(t, n, sizeof(*t), by_record_pos);  /* the list's own order, or any */
      for (k = 0; k < n; k++) { h[k] = hit(t[k][0], t[k][2]); st[k] = t[k][1]; }
      bad |= all_modes(h, st, n, len, records);
      free(t); free(st); free(h);
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
