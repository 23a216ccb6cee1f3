/*
 * find_host_check.c -- the host part of dx_file_find (csrc/dx_file_find.c: dxf_find_plan, dxf_find_map; csrc/dx_file_u2.c:
 * dxf_u2_slice_end) run alone, without a device, for a build under the sanitizers: pattern parsing and its refusals, the reverse
 * complement, the query table, the slice plan for a list of budgets, and the mapping of a slice's hits to records, patterns and
 * strands.  The walk is the host's (ctx == NULL); what the device would list for a slice is made here by a plain search of the
 * image's packed reads, in the kernel's order (unit, pos, query).
 *
 *     find_host_check <fasta|arrow> <image> [<budget> ...]
 *
 * prints the query table, the hits per pattern and strand, and per budget the slices; exits 1 when a refusal is missing, a reverse
 * complement's reverse complement is not the pattern, a plan is not a partition of the records into non-empty ranges of which only
 * a one-record range may exceed the budget, the mapped list is not in the order (record, pos, pattern, strand), or the sliced
 * totals differ from the one-slice totals.
 *
 * Build (the library's host C files compiled here with the sanitizers, the device files' entry points taken from the library, which
 * this program never calls into):
 *     clang -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Idextractor_amd/csrc \
 *           tools/find_host_check.c $(for f in dx_file_find dx_file_u2 dx_file_check dx_file_qv dx_file_pack2 dx_files dx_host dx_walk_host dx_crew; \
 *           do echo dextractor_amd/csrc/$f.c; done) -Ldextractor_amd -ldexgpu -Wl,-rpath,$PWD/dextractor_amd -lpthread -lm -o find_host_check
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dexgpu.h"
#include "dx_host.h"
#include "dx_files.h"

/* (find/dx_find.hip has it in the library, hidden: here no context has a text to keep) */
int dx_find_fail(dx_ctx *ctx, int code, const char *what) { (void) ctx; (void) what; return code; }
int dx_find_edit_fail(dx_ctx *ctx, int code, const char *what) { (void) ctx; (void) what; return code; }      /* (dx_file_find.c's driver serves dx_file_find_edit too) */

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

static int code_at(const uint8_t *read, uint32_t i) { return (read[i >> 2] >> (6 - 2 * (i & 3))) & 3; }

/* records [i0, i1) searched as the kernel would: the hits in the order (unit, pos, query), the unit counted from i0 */
static uint64_t search(const uint8_t *img, const u2_index *x, uint64_t i0, uint64_t i1, const find_plan *fp, dx_hit **list, uint64_t *cap, uint64_t n)
{ uint64_t i;
  for (i = i0; i < i1; i++)
    { const uint8_t *read = img + x->ioff[i];
      uint32_t pos, k, j;
      for (pos = 0; pos < x->nsym[i]; pos++)
        for (k = 0; k < fp->nq; k++)
          { const dx_query *q = &fp->q[k];
            uint32_t mis = 0;
            if (x->nsym[i] - pos < q->len) continue;
            for (j = 0; j < q->len; j++) mis += code_at(read, pos + j) != (int) ((q->code >> (2 * (q->len - 1 - j))) & 3);
            if (mis > q->max_mis) continue;
            if (n == *cap)
              { *cap = *cap ? 2 * *cap : 256;
                if ((*list = realloc(*list, (size_t) *cap * sizeof(**list))) == NULL) { fprintf(stderr, "out of memory\n"); exit(2); }
              }
            (*list)[n].record = i - i0; (*list)[n].pos = pos; (*list)[n].query = (uint16_t) k; (*list)[n].strand = 0; (*list)[n].mis = (uint8_t) mis;
            n++;
          }
    }
  return n;
}

static int refusals(int kind)
{ static const char *long33 = "ACGTACGTACGTACGTACGTACGTACGTACGTA", *many[65];
  const char *one[2];
  find_plan fp;
  int bad = 0, k;
  for (k = 0; k < 65; k++) many[k] = kind == DX_KIND_ARROW ? "1234" : "ACGT";
  one[0] = kind == DX_KIND_ARROW ? "12a4" : "ACNT"; one[1] = NULL;
  bad |= dxf_find_plan(NULL, kind, one, 1, 0, 0, &fp) != DX_E_ARG;                     /* a letter that is not the kind's */
  one[0] = long33;
  bad |= dxf_find_plan(NULL, DX_KIND_FASTA, one, 1, 0, 0, &fp) != DX_E_ARG;            /* 33 letters */
  one[0] = "";
  bad |= dxf_find_plan(NULL, kind, one, 1, 0, 0, &fp) != DX_E_ARG;                     /* none */
  bad |= dxf_find_plan(NULL, kind, one, 0, 0, 0, &fp) != DX_E_ARG;
  bad |= dxf_find_plan(NULL, kind, NULL, 1, 0, 0, &fp) != DX_E_ARG;
  bad |= dxf_find_plan(NULL, kind, many, 65, 0, 0, &fp) != DX_E_ARG;
  bad |= dxf_find_plan(NULL, kind, many, 64, 0, 0, &fp) != DX_OK || fp.nq != 64;
  bad |= dxf_find_plan(NULL, kind, many, 2, 4, 0, &fp) != DX_E_ARG;                    /* max_mis not below the shortest pattern */
  bad |= dxf_find_plan(NULL, kind, many, 2, 3, 0, &fp) != DX_OK;
  bad |= dxf_find_plan(NULL, DX_KIND_QUIVA, many, 1, 0, 0, &fp) != DX_E_ARG;
  bad |= dxf_find_plan(NULL, DX_KIND_ARROW, many, 1, 0, 1, &fp) != DX_E_ARG;           /* both strands of pulse widths */
  bad |= dxf_find_plan(NULL, DX_KIND_FASTA, many, 33, 0, 1, &fp) != DX_E_ARG;
  if (kind == DX_KIND_FASTA)
    bad |= dxf_find_plan(NULL, kind, many, 32, 0, 1, &fp) != DX_OK || fp.nq != 32;     /* 32 palindromes: a query each */
  return bad;
}

int main(int argc, char **argv)
{ static const char *fasta[] = { "TACG", "ACGT", "a", "GGCCAATTGGCCAATTGGCCAATTGGCCAATT", "ttttcc" }, *arrow[] = { "1234", "4", "11", "32123" };
  image_text  im;
  find_plan   fp;
  dx_hit     *list = NULL;
  uint64_t    cap = 0, n, whole[64][2], k, i;
  uint8_t    *img;
  size_t      m;
  int         kind, rc, bad, a, both;
  uint32_t    npat;
  const char *const *pats;

  if (argc < 3) { fprintf(stderr, "usage: %s <fasta|arrow> <image> [<budget> ...]\n", argv[0]); return 2; }
  kind = !strcmp(argv[1], "arrow") ? DX_KIND_ARROW : DX_KIND_FASTA;
  both = kind == DX_KIND_FASTA;
  pats = kind == DX_KIND_FASTA ? fasta : arrow; npat = kind == DX_KIND_FASTA ? 5 : 4;
  bad = refusals(kind);
  if (bad) printf("a refusal is missing\n");

  if ((rc = dxf_find_plan(NULL, kind, pats, npat, 0, both, &fp)) != DX_OK) { printf("plan: error %d\n", rc); return 1; }
  for (k = 0; k < fp.nq; k++)
    { printf("query %2" PRIu64 ": pattern %u strand %u len %2u code %016" PRIx64 "\n", k, fp.pat[k], fp.strand[k], fp.q[k].len, fp.q[k].code);
      if (k && (fp.pat[k] < fp.pat[k - 1] || (fp.pat[k] == fp.pat[k - 1] && fp.strand[k] <= fp.strand[k - 1]))) bad = 1;
      if (fp.strand[k])                                    /* the reverse complement of the reverse complement is the pattern */
        { uint64_t back = 0;
          uint32_t j;
          for (j = 0; j < fp.q[k].len; j++) back |= (3 - ((fp.q[k].code >> (2 * j)) & 3)) << (2 * (fp.q[k].len - 1 - j));
          if (back != fp.q[k - 1].code || fp.pat[k - 1] != fp.pat[k] || back == fp.q[k].code) { printf("  BAD REVERSE COMPLEMENT\n"); bad = 1; }
        }
    }

  img = slurp(argv[2], &m);
  if ((rc = dxf_image_open(NULL, kind, 0, 1, img, m, &im)) != DX_OK)
    { printf("image: error %d\n", rc);                     /* (an image that does not parse is an answer, not a failure of the check) */
      dxf_image_close(&im);
      free(img);
      return bad;
    }
  memset(whole, 0, sizeof(whole));
  for (a = 2; a < (argc > 3 ? argc : 3); a++)              /* first the one-slice plan (budget 0), then every budget */
    { const size_t budget = a == 2 ? 0 : (size_t) strtoull(argv[a], NULL, 10);
      uint64_t i0, i1, slices = 0, per[64][2], listed = 0;
      dx_hit   last = { 0, 0, 0, 0, 0 };
      memset(per, 0, sizeof(per));
      for (i0 = 0; i0 < im.ux.cnt; i0 = i1, slices++)
        { i1 = dxf_u2_slice_end(&im.ux, i0, budget);
          if (i1 <= i0 || i1 > im.ux.cnt) { bad = 1; break; }
          if (budget && i1 - i0 > 1 && im.ux.ioff[i1 - 1] + ((im.ux.nsym[i1 - 1] + 3u) >> 2) - im.ux.ioff[i0] > budget) bad = 1;
          n = search(img, &im.ux, i0, i1, &fp, &list, &cap, 0);
          dxf_find_map(&fp, list, n, i0);
          for (i = 0; i < n; i++)
            { const dx_hit *h = &list[i];
              if (h->record < i0 || h->record >= i1 || h->query >= npat || h->strand > 1) { bad = 1; break; }
              if (listed && (h->record < last.record || (h->record == last.record && (h->pos < last.pos || (h->pos == last.pos &&
                  (h->query < last.query || (h->query == last.query && h->strand <= last.strand))))))) bad = 1;
              per[h->query][h->strand]++; last = *h; listed++;
            }
        }
      if (a == 2) memcpy(whole, per, sizeof(per));
      else if (memcmp(whole, per, sizeof(per))) bad = 1;
      printf("budget %zu: %" PRIu64 " slices, %" PRIu64 " hits%s\n", budget, slices, listed, bad ? "  BAD" : "");
      if (a == 2)
        for (k = 0; k < npat; k++) printf("  pattern %" PRIu64 " (%s): %" PRIu64 " + %" PRIu64 "\n", k, pats[k], per[k][0], per[k][1]);
    }
  free(list);
  dxf_image_close(&im);
  free(img);
  return bad;
}
