/* u2_slices_standin.c -- dxf_u2_slices (csrc/dx_file_u2.c), the loop that hands the packed reads of a walked .dexta / .dexar image to
   the drivers slice by slice, with the HOST standing in for the device, for tests/test_u2_slices_host.py: device memory is host
   memory, so that the loop's own work -- the slices, the bytes and offsets it uploads, how it carves the hook's words out of the
   record arrays, what it frees -- runs under the host's sanitizers and without a GPU.  Linked with the library's C files; what those
   name of the device side and never reach here stays unresolved.
   usage: u2_slices_standin fasta|arrow image   (prints the slices every cap gave; exits 1 on the first breach, with a line saying which) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "dexgpu.h"
#include "dx_host.h"              /* (the library's own declarations of what is defined here: a changed signature does not compile) */

struct dx_ctx { int x; };
static int mallocs, frees;
int dx_malloc(dx_ctx *c, size_t n, void **p) { (void) c; mallocs++; *p = malloc(n ? n : 1); return *p ? DX_OK : DX_E_NOMEM; }
int dx_free(dx_ctx *c, void *p) { (void) c; frees++; free(p); return DX_OK; }
int dx_h2d(dx_ctx *c, void *d, const void *s, size_t n) { (void) c; memcpy(d, s, n); return DX_OK; }
int dx_d2h(dx_ctx *c, void *d, const void *s, size_t n) { (void) c; memcpy(d, s, n); return DX_OK; }
int dx_mem_info(dx_ctx *c, uint64_t *f, uint64_t *a) { (void) c; *f = *a = 1ull << 34; return DX_OK; }
#include "dx_files.h"

#define FAIL(...) do { fprintf(stderr, "cap %zu, extra %zu, slice %llu: ", j->cap, j->extra, (unsigned long long) j->slices); \
                       fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); exit(1); } while (0)

typedef struct
  { const uint8_t *img; const u2_index *x;
    size_t    cap, extra;
    uint64_t  next, slices, fail_at;         /* the record the next slice must begin with; slices so far; the slice that is refused (0: none) */
    uint64_t  tot[4], *rec;                  /* the four codes counted over all records, and every record's own four */
  } job;

static int hook(void *arg, const u2_slice *s)
{ job *j = arg;
  const u2_index *x = j->x;
  uint64_t k, i;
  j->slices++;
  if (j->fail_at && j->slices == j->fail_at) return DX_E_FORMAT;
  if (s->n == 0 || s->i0 != j->next || s->i0 + s->n > x->cnt) FAIL("records [%llu, +%llu): not the next ones", (unsigned long long) s->i0, (unsigned long long) s->n);
  j->next = s->i0 + s->n;
  if (s->bytes != dxf_u2_end(x, j->next - 1) - x->ioff[s->i0]) FAIL("%llu bytes", (unsigned long long) s->bytes);
  if (j->cap == 0 && s->n != x->cnt) FAIL("cap 0 is one slice");
  if (j->cap != 0 && s->bytes > j->cap && s->n != 1) FAIL("%llu records span %llu bytes", (unsigned long long) s->n, (unsigned long long) s->bytes);
  if (memcmp(s->d_in, j->img + x->ioff[s->i0], (size_t) s->bytes)) FAIL("the image's bytes differ");
  if (((uintptr_t) s->d_extra & 7u) || ((uintptr_t) s->d_boff & 7u) || ((uintptr_t) s->d_len & 3u)) FAIL("an array is not aligned");
  memset(s->d_extra, 0xa5, j->extra * (size_t) s->n);       /* all of the hook's words: they overlie neither the offsets nor the lengths */
  for (k = 0; k < s->n; k++)
    { if (s->d_boff[k] != x->ioff[s->i0 + k] - x->ioff[s->i0]) FAIL("record %llu: offset", (unsigned long long) k);
      if (s->d_len[k] != x->nsym[s->i0 + k]) FAIL("record %llu: length", (unsigned long long) k);
      if (s->d_len[k] && s->d_boff[k] + ((s->d_len[k] + 3u) >> 2) > s->bytes) FAIL("record %llu ends outside the slice", (unsigned long long) k);
      for (i = 0; i < s->d_len[k]; i++)
        { const unsigned v = (s->d_in[s->d_boff[k] + (i >> 2)] >> (6 - 2 * (i & 3))) & 3u;
          j->tot[v]++; j->rec[4 * (s->i0 + k) + v]++;
        }
    }
  for (k = 0; k < j->extra * (size_t) s->n; k++)
    if (((const uint8_t *) s->d_extra)[k] != 0xa5) FAIL("the hook's words did not stay");
  return DX_OK;
}

static uint8_t *slurp(const char *p, size_t *n)
{ FILE *f = fopen(p, "rb"); uint8_t *b;
  if (f == NULL) { perror(p); exit(2); }
  fseek(f, 0, SEEK_END); *n = (size_t) ftell(f); fseek(f, 0, SEEK_SET);
  b = malloc(*n + 1); if (fread(b, 1, *n, f) != *n) exit(2); fclose(f); return b;
}

int main(int argc, char **argv)
{ static const size_t caps[] = { 0, 1, 5, 64, 4096 }, extras[] = { 0, 4, 16 };
  size_t m, c, e; uint8_t *img; u2_index x; dx_ctx ctx; job whole, jb, *j = &jb; uint64_t *rec[2]; int rc;
  if (argc < 3) return 2;
  img = slurp(argv[2], &m);
  if ((rc = dxf_u2_walk(strcmp(argv[1], "arrow") ? DX_LETTERS_LOWER : DX_LETTERS_ARROW, img, m, NULL, &x)) != DX_OK) { fprintf(stderr, "walk: rc %d\n", rc); return 1; }
  rec[0] = calloc(4 * x.cnt + 1, sizeof(uint64_t)); rec[1] = calloc(4 * x.cnt + 1, sizeof(uint64_t));
  printf("%llu records\n", (unsigned long long) x.cnt);
  for (c = 0; c < sizeof(caps) / sizeof(*caps); c++)
    for (e = 0; e < sizeof(extras) / sizeof(*extras); e++)
      { memset(&jb, 0, sizeof(jb)); memset(rec[c != 0], 0, (4 * x.cnt + 1) * sizeof(uint64_t));
        jb.img = img; jb.x = &x; jb.cap = caps[c]; jb.extra = extras[e]; jb.rec = rec[c != 0];
        mallocs = frees = 0;
        rc = dxf_u2_slices(&ctx, img, &x, caps[c], extras[e], hook, &jb);
        if (rc != DX_OK) FAIL("rc %d", rc);
        if (jb.next != x.cnt) FAIL("the slices end at record %llu", (unsigned long long) jb.next);
        if (mallocs != (x.cnt ? 2 : 0) || frees != mallocs) FAIL("%d device arrays made, %d freed", mallocs, frees);
        if (c == 0) whole = jb;                             /* (cap 0: the one-slice totals the others are held against) */
        else if (memcmp(jb.tot, whole.tot, sizeof(jb.tot)) || memcmp(rec[1], rec[0], 4 * x.cnt * sizeof(uint64_t))) FAIL("totals differ from the one slice's");
        if (e == 0) printf("cap %zu: %llu slices\n", caps[c], (unsigned long long) jb.slices);
      }
  for (c = 1; c < sizeof(caps) / sizeof(*caps); c++)        /* the hook refuses the second slice: its answer comes back, nothing is left behind */
    { memset(&jb, 0, sizeof(jb)); memset(rec[1], 0, (4 * x.cnt + 1) * sizeof(uint64_t));
      jb.img = img; jb.x = &x; jb.cap = caps[c]; jb.extra = 16; jb.rec = rec[1]; jb.fail_at = 2;
      mallocs = frees = 0;
      rc = dxf_u2_slices(&ctx, img, &x, caps[c], 16, hook, &jb);
      if (jb.slices < 2) { if (rc != DX_OK) FAIL("rc %d", rc); continue; }
      if (rc != DX_E_FORMAT || jb.slices != 2 || frees != mallocs) FAIL("a refused slice: rc %d, %llu slices, %d of %d arrays freed", rc, (unsigned long long) jb.slices, frees, mallocs);
    }
  free(rec[0]); free(rec[1]); dxf_u2_index_free(&x); free(img);
  return 0;
}
