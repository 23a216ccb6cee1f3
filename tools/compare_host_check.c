/*
 * compare_host_check.c -- the host part of dx_file_compare (csrc/dx_file_compare.c: dxf_compare_open, dxf_compare_slice_end) run alone,
 * without a device, for a build under the sanitizers: the two walks and their pairing, the prefix / header / length comparison, and the
 * slice plan for a list of budgets.  Every walk is the host's (ctx == NULL).
 *
 *     compare_host_check <fasta|arrow|quiva> <image a> <image b> [<budget> ...]
 *
 * prints the host fields of the report and, per budget, the slices; exits 1 when a plan is not a partition of the compared records into
 * non-empty ranges of which only a one-record range may exceed the budget.
 *
 * Build (the library's host C files compiled here with the sanitizers, the device files' entry points taken from the library, which this
 * program never calls into):
 *     clang -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Idextractor_amd/csrc \
 *           tools/compare_host_check.c $(for f in dx_file_compare dx_file_u2 dx_file_check dx_file_qv dx_file_pack2 dx_files dx_host dx_walk_host dx_crew; \
 *           do echo dextractor_amd/csrc/$f.c; done) -Ldextractor_amd -ldexgpu -Wl,-rpath,$PWD/dextractor_amd -lpthread -lm -o compare_host_check
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dexgpu.h"
#include "dx_host.h"
#include "dx_files.h"

/* (compare/dx_diff.hip has it in the library, hidden: here no context has a text to put a letter in front of) */
int dx_side_fail(dx_ctx *ctx, int code, int side) { (void) ctx; (void) side; return code; }

static uint8_t *slurp(const char *path, size_t *n)
{ FILE *f = fopen(path, "rb");
  uint8_t *p;
  long len;
  if (f == NULL) { perror(path); exit(2); }
  fseek(f, 0, SEEK_END); len = ftell(f); fseek(f, 0, SEEK_SET);
  p = malloc((size_t) len + 1);
  if (p == NULL || fread(p, 1, (size_t) len, f) != (size_t) len) { fprintf(stderr, "%s: cannot read\n", path); exit(2); }
  fclose(f);
  *n = (size_t) len;
  return p;
}

int main(int argc, char **argv)
{ cmp_pair   p;
  dx_compare c;
  uint8_t   *a, *b;
  size_t     na, nb;
  int        kind, rc, side = 0, k, bad = 0;

  if (argc < 4) { fprintf(stderr, "usage: %s <fasta|arrow|quiva> <image a> <image b> [<budget> ...]\n", argv[0]); return 2; }
  kind = !strcmp(argv[1], "fasta") ? DX_KIND_FASTA : !strcmp(argv[1], "arrow") ? DX_KIND_ARROW : DX_KIND_QUIVA;
  a = slurp(argv[2], &na); b = slurp(argv[3], &nb);
  memset(&p, 0, sizeof(p));
  rc = dxf_compare_open(NULL, kind, a, na, b, nb, &p, &c, &side);
  if (rc != DX_OK)
    { printf("%c: error %d\n", side, rc);
      dxf_compare_close(&p);
      free(a); free(b);
      return 0;                                           /* (an image that does not parse is an answer, not a failure of the check) */
    }
  printf("records %" PRIu64 " %" PRIu64 " both %" PRIu64 " prefix_differs %d headers_differ %" PRIu64 " first %" PRId64
         " lengths_differ %" PRIu64 " first %" PRId64 " measure %" PRIu64 " %" PRIu64 "\n",
         c.records_a, c.records_b, p.both, c.prefix_differs, c.headers_differ, (int64_t) c.first_header,
         c.lengths_differ, (int64_t) c.first_length, p.pa[p.both] - p.pa[0], p.pb[p.both] - p.pb[0]);
  for (k = 4; k < argc; k++)
    { const size_t cap = (size_t) strtoull(argv[k], NULL, 10);
      uint64_t i0, i1, slices = 0;
      for (i0 = 0; i0 < p.both; i0 = i1, slices++)
        { i1 = dxf_compare_slice_end(&p, i0, cap);
          if (i1 <= i0 || i1 > p.both) { bad = 1; break; }
          if (cap && i1 - i0 > 1 && (p.pa[i1] - p.pa[i0]) + (p.pb[i1] - p.pb[i0]) > cap) bad = 1;
        }
      printf("budget %zu: %" PRIu64 " slices%s\n", cap, slices, bad ? "  BAD PLAN" : "");
    }
  dxf_compare_close(&p);
  free(a); free(b);
  return bad;
}
