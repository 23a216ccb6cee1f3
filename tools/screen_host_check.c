/*
 * screen_host_check.c -- the host part of the screen (csrc/dx_file_screen.c: dx_screen_select) run alone, without a device, for a build
 * under the sanitizers: cases made by hand (equality at the permille threshold and one symbol fewer, a record of length 0, min_hits 0,
 * products that leave 32 bits, no records), the refusals, and random entries in both modes.  Every selection is held against a second
 * formulation that shares nothing with the first: the threshold as a quotient rounded up, the two modes as a mark a record.
 *
 *     screen_host_check [<random cases>]
 *
 * prints a line a group of cases; exits 1 when a selection differs, its ids do not ascend, the two modes do not partition the records
 * or a refusal is missing.
 *
 * Build (csrc/dx_file_screen.c compiled here with the sanitizers; dx_file_screen's callees are taken from the library, which this
 * program never calls into):
 *     cc -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Idextractor_amd/csrc \
 *        tools/screen_host_check.c dextractor_amd/csrc/dx_file_screen.c -Ldextractor_amd -ldexgpu -Wl,-rpath,$PWD/dextractor_amd -o screen_host_check
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dexgpu.h"
#include "dx_host.h"
#include "dx_files.h"

/* (the library has these hidden: here no context has a text to keep and no image is opened) */
int      dx_screen_fail(dx_ctx *ctx, int code, const char *what) { (void) ctx; (void) what; return code; }
int      dxf_image_open(dx_ctx *ctx, int kind, int upper, uint32_t width, const uint8_t *img, size_t n, image_text *im)
{ (void) ctx; (void) kind; (void) upper; (void) width; (void) img; (void) n; (void) im; return DX_E_UNSUPPORTED; }
void     dxf_image_close(image_text *im) { (void) im; }
size_t   dxf_u2_cap(dx_ctx *ctx, size_t m, uint64_t units) { (void) ctx; (void) m; (void) units; return 0; }
int      dxf_u2_slices(dx_ctx *ctx, const uint8_t *img, const u2_index *x, size_t cap, size_t extra, u2_slice_fn fn, void *arg)
{ (void) ctx; (void) img; (void) x; (void) cap; (void) extra; (void) fn; (void) arg; return DX_E_UNSUPPORTED; }

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n)                            /* xorshift64*: 0 .. n - 1 */
{ rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return (uint32_t) (((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % n);
}

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("  FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

/* does record i match?  The threshold as the fewest covered symbols that pass: ceil(min_permille * len / 1000) */
static int matches(const dx_screen *r, uint32_t len, uint32_t min_hits, uint32_t min_permille)
{ const uint64_t need = ((uint64_t) min_permille * len + 999) / 1000;
  return r->hits >= (min_hits > 1 ? min_hits : 1) && r->covered >= need;
}

/* both modes of one question against the marks; returns the records kept */
static uint64_t both(const dx_screen *rec, const uint32_t *len, uint64_t n, uint32_t min_hits, uint32_t min_permille)
{ uint64_t *keep = NULL, *drop = NULL, nk = 7, nd = 7, i, a = 0, b = 0;
  CHECK(dx_screen_select(rec, len, n, min_hits, min_permille, DX_SCREEN_KEEP, &keep, &nk) == DX_OK);
  CHECK(dx_screen_select(rec, len, n, min_hits, min_permille, DX_SCREEN_DROP, &drop, &nd) == DX_OK);
  CHECK(keep != NULL && drop != NULL && nk + nd == n);
  for (i = 0; i < n && keep && drop; i++)
    { if (matches(rec + i, len[i], min_hits, min_permille)) { CHECK(a < nk && keep[a] == i); a++; }
      else                                                  { CHECK(b < nd && drop[b] == i); b++; }
    }
  CHECK(a == nk && b == nd);
  dx_file_free(keep); dx_file_free(drop);
  return nk;
}

int main(int argc, char **argv)
{ const int cases = argc > 1 ? atoi(argv[1]) : 2000;
  int c;

  { /* by hand */
    const dx_screen rec[] = { { 5, 900, 0, 800 }, { 5, 899, 0, 800 }, { 1, 7, 0, 0 }, { 1, 6, 0, 0 }, { 2, 1000, 0, 0 },
                              { 0, 0, UINT32_MAX, UINT32_MAX }, { 0, 0, UINT32_MAX, UINT32_MAX }, { 1, 0x7fffffff, 0, 0 }, { 1, 0x7ffffffe, 0, 0 } };
    const uint32_t len[] = { 1000, 1000, 7, 7, 1000, 0, 50, 0x7fffffff, 0x7fffffff };
    uint64_t *ids = NULL, n = 0;
    CHECK(both(rec, len, 9, 1, 900) == 5);                 /* 0, 2, 4, 7, 8 */
    CHECK(both(rec, len, 9, 1, 1000) == 3);                /* 2, 4, 7 */
    CHECK(both(rec, len, 9, 0, 0) == 7 && both(rec, len, 9, 1, 0) == 7);            /* min_hits 0 acts as 1; length 0 never matches */
    CHECK(both(rec, len, 9, 3, 0) == 2);
    CHECK(both(rec, len, 0, 1, 0) == 0 && both(NULL, NULL, 0, 1, 500) == 0);
    CHECK(dx_screen_select(rec, len, 9, 1, 1001, DX_SCREEN_KEEP, &ids, &n) == DX_E_ARG && ids == NULL && n == 0);
    CHECK(dx_screen_select(rec, len, 9, 1, 0, 2, &ids, &n) == DX_E_ARG && dx_screen_select(rec, len, 9, 1, 0, -1, &ids, &n) == DX_E_ARG);
    CHECK(dx_screen_select(NULL, len, 9, 1, 0, 0, &ids, &n) == DX_E_ARG && dx_screen_select(rec, NULL, 9, 1, 0, 0, &ids, &n) == DX_E_ARG);
    CHECK(dx_screen_select(rec, len, 9, 1, 0, 0, NULL, &n) == DX_E_ARG && dx_screen_select(rec, len, 9, 1, 0, 0, &ids, NULL) == DX_E_ARG);
    printf("by hand: %s\n", failures ? "FAILED" : "ok");
  }

  for (c = 0; c < cases; c++)
    { const uint64_t n = rnd(200);
      dx_screen *rec = malloc((size_t) (n ? n : 1) * sizeof(*rec));
      uint32_t  *len = malloc((size_t) (n ? n : 1) * sizeof(*len));
      uint64_t   i;
      if (rec == NULL || len == NULL) { fprintf(stderr, "out of memory\n"); return 2; }
      for (i = 0; i < n; i++)
        { len[i] = rnd(4) ? rnd(3000) : 0x7fffffffu - rnd(1000);
          rec[i].hits = rnd(3) ? rnd(40) : 0;
          rec[i].covered = rec[i].hits ? (len[i] ? rnd(len[i]) + (rnd(5) == 0) : 0) : 0;
          rec[i].first = rec[i].last = rec[i].hits ? 0 : UINT32_MAX;
        }
      both(rec, len, n, rnd(6), rnd(1001));
      free(rec); free(len);
    }
  printf("%d random cases: %s\n", cases, failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
