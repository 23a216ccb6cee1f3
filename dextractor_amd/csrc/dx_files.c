/*
 * dx_files.c -- whole-file drivers: the host side of the six tools, above the kernel C-ABI.  This file has what all of them use; the
 * drivers themselves are in dx_file_pack2.c, dx_file_qv.c, dx_file_check.c and dx_select.c (dx_files.h).
 *
 * Each function takes a complete input file image in host memory and returns the complete output
 * image (malloc'd; release with dx_file_free), byte-identical to what the reference tool writes:
 *
 *     dx_file_pack2    dexta.c:104-205 / dexar.c:103-211
 *     dx_file_unpack2  undexta.c:131-271 / undexar.c:129-229
 *     dx_file_dexqv    dexqv.c:79-143 (QVcoding_Scan, Create_QVcoding, Write_QVcoding,
 *                      Compress_Next_QVentry per entry)
 *     dx_file_undexqv  undexqv.c:101-208
 *
 * The host does what is O(records) or pure text parsing (indexing lines, sscanf of the header
 * fields, sprintf of decoded headers, Huffman table construction); every per-symbol loop runs on
 * the GPU through the kernels of libdexgpu.  Plain C: only the public C-ABI is used.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dexgpu.h"
#include "dx_env.h"
#include "dx_host.h"
#include "dx_files.h"

void dx_file_free(void *p) { free(p); }

/* ---- what every driver uses (dx_files.h says what each of these is) ---------------------------------------------------- */
int dxf_budget_env(size_t whole, size_t floor, size_t *cap)
{ const char *e = getenv("DEXGPU_TEXT_BUDGET");
  unsigned long long v;
  if (e == NULL || !*e) return 0;
  v = strtoull(e, NULL, 10);
  *cap = v && v < whole ? (size_t) (v < floor ? floor : v) : 0;
  return 1;
}

int dxf_tb_room(tbuf *b, size_t more)
{ if (b->len + more > b->cap)
    { size_t nc = (b->len + more) * 2 + 4096;
      char  *np = realloc(b->p, nc);
      if (np == NULL) return DX_E_NOMEM;
      b->p = np; b->cap = nc;
    }
  return DX_OK;
}

/* ---- decoded text on its way out -------------------------------------------------------------------------------------- */
/* a chunk of it (dx_d2h_stream, at0 bytes into the streamed buffer): the header lines that fall into it are laid over it */
static int patch_and_pass(void *arg, uint8_t *data, size_t len, size_t at0)
{ hdr_patch *h = arg;
  const size_t at = at0 + h->base;
  uint64_t lo = 0, hi = h->n, i;
  while (lo < hi)                                         /* first entry whose text starts beyond `at` */
    { uint64_t mid = (lo + hi) / 2;
      if (h->ooff[mid] > at) hi = mid; else lo = mid + 1;
    }
  for (i = lo; i < h->n; i++)
    { const size_t hl = (size_t) (h->hat[i+1] - h->hat[i]), h0 = (size_t) h->ooff[i] - hl, h1 = (size_t) h->ooff[i];
      const size_t c0 = h0 > at ? h0 : at, c1 = h1 < at + len ? h1 : at + len;
      if (h0 >= at + len) break;
      if (c0 < c1)
        memcpy(data + (c0 - at), h->hd + h->hat[i] + (c0 - h0), c1 - c0);
    }
  return h->sink(h->user, data, len, at);
}

uint64_t dxf_text_slice_end(const hdr_patch *h, uint64_t i0, size_t cap)
{ uint64_t i1 = i0 + 1;
  if (cap == 0) return h->n;
  while (i1 < h->n && text_at(h, i1 + 1) - text_at(h, i0) <= cap) i1++;
  return i1;
}

size_t dxf_out_cap(dx_ctx *ctx, size_t n, size_t total, uint64_t units)
{ uint64_t fr = 0, all = 0;
  size_t   cap;
  if (dxf_budget_env(total, 65536u, &cap)) return cap;
  if (dx_mem_info(ctx, &fr, &all) != DX_OK || fr == 0) return 0;
  if ((double) n + (double) total + 48.0 * (double) units <= 0.9 * (double) fr) return 0;
  { const double room = 0.9 * (double) fr - (double) n - 48.0 * (double) units;
    return room > (double) ((size_t) 4 << 20) ? (size_t) room : (size_t) 4 << 20;
  }
}

int dxf_slice_deliver(void *arg, const void *d_out, uint64_t i0, uint64_t i1, size_t t0, size_t bytes)
{ slice_out *s = arg;
  hdr_patch *h = s->h;
  uint64_t   i;
  int        rc;
  if (s->res == NULL)
    { h->base = t0;
      return dx_d2h_stream(s->ctx, d_out, bytes, patch_and_pass, h);
    }
  rc = dx_d2h(s->ctx, s->res + t0, d_out, bytes);
  for (i = i0; i < i1 && rc == DX_OK; i++)
    memcpy(s->res + h->ooff[i] - (h->hat[i+1] - h->hat[i]), h->hd + h->hat[i], (size_t) (h->hat[i+1] - h->hat[i]));
  return rc;
}
