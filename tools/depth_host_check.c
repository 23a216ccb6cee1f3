/*
 * depth_host_check.c -- dx_depth_select (csrc/dx_file_depth.c) run alone, without a device, for a build under the sanitizers: random
 * records (a quarter of them without a window), every stat, both modes, bounds that cut through the values, min_windows 0, 1 and large;
 * no records; the refusals.  Every answer is held against a second loop that reads the fields by name, and the two modes against each
 * other: together they list every record once, ascending.
 *
 *     depth_host_check [<random cases>]
 *
 * prints a line a group of cases; exits 1 when a selection differs, its ids are not ascending or a refusal is missing.
 *
 * Build (csrc/dx_file_depth.c compiled here with the sanitizers; dx_file_depth itself, whose callees are the library's own, is not
 * called and is dropped by the linker, a section a function):
 *     clang -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffunction-sections -Iinclude -Idextractor_amd/csrc \
 *           tools/depth_host_check.c dextractor_amd/csrc/dx_file_depth.c -Wl,--gc-sections -o depth_host_check
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dexgpu.h"

/* (dx_files.c has it in the library, which this program does not link: what dx_depth_select hands out is malloc'd) */
void dx_file_free(void *p) { free(p); }

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n)                            /* xorshift64*: 0 .. n - 1 */
{ rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return (uint32_t) (((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % n);
}

static uint32_t stat_of(const dx_depth *e, int stat)
{ switch (stat)
    { case DX_DEPTH_MIN: return e->min;
      case DX_DEPTH_Q1: return e->q1;
      case DX_DEPTH_MEDIAN: return e->median;
      case DX_DEPTH_Q3: return e->q3;
      default: return e->max;
    }
}

static int fails = 0;
static void bad(const char *what, uint64_t a, uint64_t b)
{ fprintf(stderr, "FAIL: %s (%" PRIu64 ", %" PRIu64 ")\n", what, a, b);
  fails++;
}

static void one_case(uint64_t records)
{ dx_depth *rec = calloc((size_t) records + 1, sizeof(*rec));
  uint8_t  *seen = calloc((size_t) records + 1, 1);
  uint64_t  i;
  int       stat, mode;
  if (rec == NULL || seen == NULL) { fprintf(stderr, "out of memory\n"); exit(2); }
  for (i = 0; i < records; i++)
    { uint16_t v[5];
      int      a, b;
      if (rnd(4) == 0) continue;                           /* no window: all zeros */
      for (a = 0; a < 5; a++) v[a] = (uint16_t) (rnd(3) ? rnd(300) : rnd(65536));
      for (a = 0; a < 5; a++) for (b = a + 1; b < 5; b++) if (v[b] < v[a]) { uint16_t t = v[a]; v[a] = v[b]; v[b] = t; }
      rec[i].windows = 1 + rnd(2000);
      rec[i].min = v[0]; rec[i].q1 = v[1]; rec[i].median = v[2]; rec[i].q3 = v[3]; rec[i].max = v[4];
    }
  for (stat = DX_DEPTH_MIN; stat <= DX_DEPTH_MAX; stat++)
    { const uint32_t lo = rnd(2) ? rnd(200) : 0, hi = lo + (rnd(2) ? rnd(400) : 65535 - lo), mw = rnd(3) == 0 ? 0 : (rnd(2) ? 1 : rnd(1500));
      memset(seen, 0, (size_t) records + 1);
      for (mode = DX_SCREEN_KEEP; mode <= DX_SCREEN_DROP; mode++)
        { uint64_t *ids = NULL, n = 0, at = 0;
          if (dx_depth_select(rec, records, stat, lo, hi, mw, mode, &ids, &n) != DX_OK) { bad("a selection was refused", stat, mode); continue; }
          for (i = 0; i < records; i++)
            { const int match = rec[i].windows >= (mw ? mw : 1) && stat_of(rec + i, stat) >= lo && stat_of(rec + i, stat) <= hi;
              if (match == (mode == DX_SCREEN_KEEP))
                { if (at >= n || ids[at] != i) { bad("an id is missing or out of order", i, at); break; }
                  at++; seen[i]++;
                }
            }
          if (at != n) bad("more ids than records that match", at, n);
          dx_file_free(ids);
        }
      for (i = 0; i < records; i++) if (seen[i] != 1) { bad("the two modes do not part the records", i, seen[i]); break; }
    }
  free(rec); free(seen);
}

int main(int argc, char **argv)
{ const int cases = argc > 1 ? atoi(argv[1]) : 200;
  uint64_t *ids = NULL, n = 7;
  dx_depth  one;
  int       c;
  memset(&one, 0, sizeof(one));
  one.windows = 5; one.median = 3;
  for (c = 0; c < cases; c++) one_case(c < 3 ? (uint64_t) c : rnd(3000));
  printf("%d random cases, every stat, both modes\n", cases);
  if (dx_depth_select(NULL, 0, DX_DEPTH_MEDIAN, 0, 5, 1, DX_SCREEN_KEEP, &ids, &n) != DX_OK || n != 0) bad("no records is not DX_OK", n, 0);
  dx_file_free(ids);
  if (dx_depth_select(&one, 1, 5, 0, 9, 1, 0, &ids, &n) != DX_E_ARG) bad("stat 5 taken", 0, 0);
  if (dx_depth_select(&one, 1, -1, 0, 9, 1, 0, &ids, &n) != DX_E_ARG) bad("stat -1 taken", 0, 0);
  if (dx_depth_select(&one, 1, 2, 0, 9, 1, 2, &ids, &n) != DX_E_ARG) bad("mode 2 taken", 0, 0);
  if (dx_depth_select(&one, 1, 2, 9, 8, 1, 0, &ids, &n) != DX_E_ARG) bad("lo > hi taken", 0, 0);
  if (dx_depth_select(NULL, 1, 2, 0, 9, 1, 0, &ids, &n) != DX_E_ARG) bad("NULL records taken", 0, 0);
  if (dx_depth_select(&one, 1, 2, 0, 9, 1, 0, NULL, &n) != DX_E_ARG) bad("NULL ids taken", 0, 0);
  if (dx_depth_select(&one, 1, 2, 0, 9, 1, 0, &ids, NULL) != DX_E_ARG) bad("NULL n_ids taken", 0, 0);
  if (ids != NULL) bad("a refusal left ids", 0, 0);
  if (dx_depth_select(&one, 1, 2, 3, 3, 1, 0, &ids, &n) != DX_OK || n != 1 || ids[0] != 0) bad("the one record is not selected", n, 0);
  dx_file_free(ids);
  printf("the refusals\n");
  return fails ? 1 : 0;
}
