/* extract_standin.c -- dx_file_extract's 2-bit driver (csrc/dx_file_extract.c, the loader of csrc/dx_select.c) with the HOST standing in
   for the device, for tests/test_extract_host.py: device memory is host memory, dx_reads_unpack_lines a plain loop over the symbols that
   writes a unit's text and not a byte more, so that the driver's own work -- the layout, the spans it sends, the slices of whole units,
   the offsets it hands the kernel, the header lines it lays in -- runs under the host's sanitizers and without a GPU.  Linked with the
   driver's C files; what those name of the device side and never reach here stays unresolved.
   usage: extract_standin image.dexta units.bin out.txt budget width   (units.bin: n x {u64 id, u32 beg, u32 end}; budget:
   DEXGPU_TEXT_BUDGET of the second of two runs, whose outputs must agree; prints how many dx_reads_unpack_lines calls each run made and
   how many packed bytes went up for them; out.txt is followed by out.txt.toff, the n + 1 offsets as u64) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "dexgpu.h"
#include "dx_host.h"              /* (the library's own declarations of what is defined here: a changed signature does not compile) */

struct dx_ctx { int x; };
int dx_malloc(dx_ctx *c, size_t n, void **p) { (void) c; *p = malloc(n ? n : 1); return *p ? DX_OK : DX_E_NOMEM; }
int dx_free(dx_ctx *c, void *p) { (void) c; free(p); return DX_OK; }
int dx_h2d(dx_ctx *c, void *d, const void *s, size_t n) { (void) c; memcpy(d, s, n); return DX_OK; }
int dx_d2h(dx_ctx *c, void *d, const void *s, size_t n) { (void) c; memcpy(d, s, n); return DX_OK; }
int dx_mem_info(dx_ctx *c, uint64_t *f, uint64_t *a) { (void) c; *f = *a = 1ull << 34; return DX_OK; }
int dx_unit_fail(dx_ctx *c, int code, const char *who, uint64_t j, const char *what)
{ (void) c; fprintf(stderr, "%s: unit %llu: %s\n", who, (unsigned long long) j, what); return code; }
int dx_entry_fail(dx_ctx *c, uint64_t id, uint64_t at, uint64_t nbytes)
{ (void) c; fprintf(stderr, "entry %llu at %llu of %llu\n", (unsigned long long) id, (unsigned long long) at, (unsigned long long) nbytes); return DX_E_FORMAT; }

#include "dx_files.h"
/* (the quiva drivers' helpers, which the linked files name: never reached here) */
int dxf_qv_header(tbuf *b, const char *p, const int32_t *h) { (void) b; (void) p; (void) h; abort(); }
int dxf_qv_head(const dx_qv_coding *cd, const uint8_t *t, size_t p, size_t more, uint8_t **img, size_t *head) { (void) cd; (void) t; (void) p; (void) more; (void) img; (void) head; abort(); }
dx_qv_batch dxf_qv_batch(const void *a, const void *b, const void *c, uint64_t m, uint64_t s, int l) { (void) a; (void) b; (void) c; (void) m; (void) s; (void) l; abort(); }
int dxf_qv_stage(dpool *pool, const int32_t *h, uint64_t m, int32_t *lw, const void *a, const void *b, const void *c, uint64_t s, int l, qv_staged *st) { (void) pool; (void) h; (void) m; (void) lw; (void) a; (void) b; (void) c; (void) s; (void) l; (void) st; abort(); }
int dxf_qv_encode_batch(dx_ctx *x, const qv_staged *s, const uint64_t (*h)[256], const dx_qv_coding *cd, int l, void **o, size_t *oc, uint64_t *t) { (void) x; (void) s; (void) h; (void) cd; (void) l; (void) o; (void) oc; (void) t; abort(); }
size_t dxf_undexqv_cap(dx_ctx *x, const dx_undexqv_plan *p, int *w) { (void) x; (void) p; (void) w; abort(); }
int dxf_undexqv_sliced(dx_ctx *x, const dx_undexqv_plan *p, int u, slice_fn d, void *a, size_t c, int w) { (void) x; (void) p; (void) u; (void) d; (void) a; (void) c; (void) w; abort(); }

static int      calls;
static uint64_t sent;
int dx_reads_unpack_lines(dx_ctx *c, int letters, const uint8_t *in, uint64_t in_bytes, const uint64_t *boff, const uint32_t *beg,
                          const uint32_t *len, uint64_t n, uint32_t width, uint8_t *out, const uint64_t *ooff, uint64_t *bad)
{ const char *abc = letters == DX_LETTERS_LOWER ? "acgt" : letters == DX_LETTERS_UPPER ? "ACGT" : "1234";
  uint64_t j, i;
  (void) c;
  calls++; sent += in_bytes;
  for (j = 0; j < n; j++)
    { uint8_t *o = out + ooff[j];
      if (len[j] && boff[j] + ((beg[j] + (uint64_t) len[j] - 1) >> 2) >= in_bytes) { *bad = j; return DX_E_FORMAT; }
      for (i = 0; i < len[j]; i++)
        { const uint64_t s = beg[j] + i;
          *o++ = (uint8_t) abc[(in[boff[j] + (s >> 2)] >> (6 - 2 * (s & 3))) & 3u];
          if ((i + 1) % width == 0 || i + 1 == len[j]) *o++ = '\n';
        }
    }
  return DX_OK;
}

static uint8_t *slurp(const char *p, size_t *n)
{ FILE *f = fopen(p, "rb"); uint8_t *b;
  if (f == NULL) exit(2);
  fseek(f, 0, SEEK_END); *n = (size_t) ftell(f); fseek(f, 0, SEEK_SET);
  b = malloc(*n + 1); if (fread(b, 1, *n, f) != *n) exit(2); fclose(f); return b;
}

int main(int argc, char **argv)
{ size_t m, un, k, n, ol[2]; uint8_t *img, *u, *out[2]; uint64_t *ids, *toff[2]; uint32_t *beg, *end; dx_ctx ctx; int pass, rc; char name[4096];
  if (argc < 6) return 2;
  img = slurp(argv[1], &m); u = slurp(argv[2], &un); n = un / 16;
  ids = malloc(n * 8 + 8); beg = malloc(n * 4 + 4); end = malloc(n * 4 + 4);
  for (k = 0; k < n; k++) { memcpy(ids + k, u + 16 * k, 8); memcpy(beg + k, u + 16 * k + 8, 4); memcpy(end + k, u + 16 * k + 12, 4); }
  for (pass = 0; pass < 2; pass++)
    { if (pass) setenv("DEXGPU_TEXT_BUDGET", argv[4], 1); else unsetenv("DEXGPU_TEXT_BUDGET");
      calls = 0; sent = 0;
      rc = dx_file_extract(&ctx, DX_KIND_FASTA, img, m, ids, beg, end, n, 1, (uint32_t) strtoul(argv[5], NULL, 10), &out[pass], &ol[pass], &toff[pass]);
      if (rc != DX_OK) { fprintf(stderr, "pass %d: rc %d\n", pass, rc); return 1; }
      printf("pass %d: %zu bytes, %d unpack calls, %llu packed bytes sent\n", pass, ol[pass], calls, (unsigned long long) sent);
    }
  if (ol[0] != ol[1] || memcmp(out[0], out[1], ol[0]) || memcmp(toff[0], toff[1], (n + 1) * 8)) { fprintf(stderr, "sliced differs\n"); return 1; }
  { FILE *f = fopen(argv[3], "wb"); fwrite(out[1], 1, ol[1], f); fclose(f); }
  snprintf(name, sizeof(name), "%s.toff", argv[3]);
  { FILE *f = fopen(name, "wb"); fwrite(toff[1], 8, n + 1, f); fclose(f); }
  dx_file_free(out[0]); dx_file_free(out[1]); dx_file_free(toff[0]); dx_file_free(toff[1]);
  free(img); free(u); free(ids); free(beg); free(end);
  return 0;
}
