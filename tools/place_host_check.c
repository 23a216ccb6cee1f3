/*
 * place_host_check.c -- dx_place_select and dx_pack_letters (csrc/dx_file_place.c) run alone, without a device, for a build under the
 * sanitizers: random places over targets of which some are empty, every target and any, loci that cut through the intervals, both
 * modes, all three strand masks; no records; the refusals; and the packer at every length around a byte, its last byte's pad bits
 * zero, a foreign letter at every position.  Every selection is held against a second loop that finds the target by walking toff, and
 * the two modes against each other: together they list every record once, ascending.
 *
 *     place_host_check [<random cases>]
 *
 * prints a line a group of cases; exits 1 when a selection differs, its ids are not ascending, a packed byte differs or a refusal is
 * missing.
 *
 * Build (csrc/dx_file_place.c and csrc/dx_file_find.c, which has the letters, compiled here with the sanitizers; the drivers in them,
 * whose callees are the library's own, are not called and are dropped by the linker, a section a function):
 *     clang -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffunction-sections -Iinclude -Idextractor_amd/csrc \
 *           tools/place_host_check.c dextractor_amd/csrc/dx_file_place.c dextractor_amd/csrc/dx_file_find.c -Wl,--gc-sections \
 *           -o place_host_check
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dexgpu.h"

/* (dx_files.c has it in the library, which this program does not link: what dx_place_select hands out is malloc'd) */
void dx_file_free(void *p) { free(p); }

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n)                            /* xorshift64*: 0 .. n - 1 */
{ rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return (uint32_t) (((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % n);
}

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { printf("FAILED: " __VA_ARGS__); printf("\n"); fails++; } } while (0)

/* the statement once more: the target by a walk over toff */
static int matches(const dx_place *e, const uint64_t *toff, uint64_t T, uint32_t target, uint32_t lo, uint32_t hi, uint32_t min_votes, int strands)
{ uint64_t t, tb, te;
  if (e->votes < (min_votes ? min_votes : 1) || e->strand > 1 || !((strands >> e->strand) & 1) || e->gbeg >= toff[T]) return 0;
  for (t = 0; !(toff[t] <= e->gbeg && e->gbeg < toff[t + 1]); t++) ;
  if (target != UINT32_MAX && t != target) return 0;
  tb = e->gbeg - toff[t];
  te = (e->gend < toff[t + 1] ? e->gend : toff[t + 1]) - toff[t];
  return tb < hi && lo < te;
}

static void select_cases(int cases)
{ int c;
  for (c = 0; c < cases; c++)
    { const uint64_t T = 1 + rnd(6), records = rnd(400);
      uint64_t  *toff = malloc((size_t) (T + 1) * sizeof(*toff)), *keep = NULL, *drop = NULL, nk = 0, nd = 0, i, a, b;
      dx_place  *rec = malloc((size_t) (records ? records : 1) * sizeof(*rec));
      const uint32_t target = rnd(3) ? rnd((uint32_t) T) : UINT32_MAX, lo = rnd(500), hi = lo + rnd(600), min_votes = rnd(6);
      const int strands = 1 + (int) rnd(3);
      for (toff[0] = 0, i = 0; i < T; i++) toff[i + 1] = toff[i] + (rnd(4) ? rnd(700) : 0);
      for (i = 0; i < records; i++)
        { memset(&rec[i], 0xff, sizeof(rec[i]));
          rec[i].seeds = rec[i].votes = rec[i].strand = 0;
          if (rnd(4))
            { rec[i].votes = rnd(8); rec[i].seeds = rec[i].votes + rnd(3); rec[i].strand = rnd(2);
              rec[i].gbeg = rnd((uint32_t) toff[T] + 40); rec[i].gend = rec[i].gbeg + 1 + rnd(300);
            }
        }
      CHECK(dx_place_select(rec, records, toff, T, target, lo, hi, min_votes, strands, DX_SCREEN_KEEP, &keep, &nk) == DX_OK, "keep");
      CHECK(dx_place_select(rec, records, toff, T, target, lo, hi, min_votes, strands, DX_SCREEN_DROP, &drop, &nd) == DX_OK, "drop");
      CHECK(nk + nd == records, "the two modes list %" PRIu64 " + %" PRIu64 " of %" PRIu64, nk, nd, records);
      for (a = b = 0, i = 0; i < records; i++)
        { const int m = matches(&rec[i], toff, T, target, lo, hi, min_votes, strands);
          if (m) { CHECK(a < nk && keep[a] == i, "record %" PRIu64 " matches and is not kept", i); a++; }
          else   { CHECK(b < nd && drop[b] == i, "record %" PRIu64 " does not match and is not dropped", i); b++; }
        }
      dx_file_free(keep); dx_file_free(drop); free(rec); free(toff);
    }
  printf("select: %d random cases\n", cases);
}

static void select_refusals(void)
{ const uint64_t toff[3] = { 0, 10, 30 }, down[3] = { 0, 10, 5 }, late[2] = { 1, 9 };
  dx_place  rec[2];
  uint64_t *ids = NULL, n = 7;
  memset(rec, 0, sizeof(rec));
  CHECK(dx_place_select(NULL, 0, toff, 2, UINT32_MAX, 0, 9, 1, 3, DX_SCREEN_KEEP, &ids, &n) == DX_OK && n == 0 && ids != NULL, "no records");
  dx_file_free(ids);
  CHECK(dx_place_select(rec, 2, toff, 2, UINT32_MAX, 0, 9, 1, 0, DX_SCREEN_KEEP, &ids, &n) == DX_E_ARG && ids == NULL, "strands 0");
  CHECK(dx_place_select(rec, 2, toff, 2, UINT32_MAX, 0, 9, 1, 4, DX_SCREEN_KEEP, &ids, &n) == DX_E_ARG, "strands 4");
  CHECK(dx_place_select(rec, 2, toff, 2, UINT32_MAX, 9, 8, 1, 3, DX_SCREEN_KEEP, &ids, &n) == DX_E_ARG, "lo > hi");
  CHECK(dx_place_select(rec, 2, toff, 2, 2, 0, 9, 1, 3, DX_SCREEN_KEEP, &ids, &n) == DX_E_ARG, "a target that is not there");
  CHECK(dx_place_select(rec, 2, toff, 2, UINT32_MAX, 0, 9, 1, 3, 2, &ids, &n) == DX_E_ARG, "another mode");
  CHECK(dx_place_select(rec, 2, down, 2, UINT32_MAX, 0, 9, 1, 3, DX_SCREEN_KEEP, &ids, &n) == DX_E_ARG, "toff decreases");
  CHECK(dx_place_select(rec, 2, late, 1, UINT32_MAX, 0, 9, 1, 3, DX_SCREEN_KEEP, &ids, &n) == DX_E_ARG, "toff does not begin at 0");
  CHECK(dx_place_select(NULL, 2, toff, 2, UINT32_MAX, 0, 9, 1, 3, DX_SCREEN_KEEP, &ids, &n) == DX_E_ARG, "no records' array");
  CHECK(dx_place_select(rec, 2, NULL, 2, UINT32_MAX, 0, 9, 1, 3, DX_SCREEN_KEEP, &ids, &n) == DX_E_ARG, "no toff");
  CHECK(dx_place_select(rec, 2, toff, 2, UINT32_MAX, 0, 9, 1, 3, DX_SCREEN_KEEP, NULL, &n) == DX_E_ARG, "no ids");
  printf("select: the refusals\n");
}

static void packer(void)
{ uint32_t len, i, bad;
  int arrow;
  for (arrow = 0; arrow < 2; arrow++)
    for (len = 0; len <= 70; len++)
      { const char *letters = arrow ? "1234" : (len & 1 ? "acgt" : "ACGT");
        char    *seq = malloc(len ? len : 1);               /* exactly len letters: no terminator is looked for */
        uint8_t *out = malloc((len + 3) / 4 ? (len + 3) / 4 : 1), *sym = malloc(len ? len : 1);
        for (i = 0; i < len; i++) { sym[i] = (uint8_t) rnd(4); seq[i] = letters[sym[i]]; }
        memset(out, 0xa5, (len + 3) / 4 ? (len + 3) / 4 : 1);
        CHECK(dx_pack_letters(arrow, seq, len, out, &bad) == DX_OK && bad == UINT32_MAX, "%u letters do not pack", len);
        for (i = 0; i < 4 * ((len + 3) / 4); i++)
          CHECK(((out[i >> 2] >> (6 - 2 * (i & 3))) & 3) == (i < len ? sym[i] : 0), "symbol %u of %u", i, len);
        for (i = 0; i < len; i++)
          { const char was = seq[i];
            seq[i] = arrow ? 'A' : "N5 \n"[i & 3];
            CHECK(dx_pack_letters(arrow, seq, len, out, &bad) == DX_E_ARG && bad == i, "a foreign letter at %u of %u", i, len);
            seq[i] = was;
          }
        free(seq); free(out); free(sym);
      }
  CHECK(dx_pack_letters(0, NULL, 4, (uint8_t *) &len, NULL) == DX_E_ARG && dx_pack_letters(0, "ACGT", 4, NULL, NULL) == DX_E_ARG, "NULL pointers");
  CHECK(dx_pack_letters(0, NULL, 0, NULL, NULL) == DX_OK, "nothing to pack");
  printf("pack: every length up to 70, both kinds, a foreign letter at every position\n");
}

int main(int argc, char **argv)
{ select_cases(argc > 1 ? atoi(argv[1]) : 2000);
  select_refusals();
  packer();
  printf(fails ? "%d checks FAILED\n" : "all checks passed\n", fails);
  return fails ? 1 : 0;
}
