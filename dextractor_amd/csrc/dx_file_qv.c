/*
 * dx_file_qv.c -- the file drivers of .quiva / .dexqv: dexqv of a whole text and in slices; undexqv as a plan and its
 * run (dexqv on several GPUs: dx_file_qv_shard.c).  dx_files.h has what the other drivers take from here.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "dexgpu.h"
#include "dx_env.h"
#include "dx_host.h"
#include "dx_files.h"

/* DEXGPU_TIMING=1: where a file driver spends its time (stderr; the tools print their own marks beside these) */
static void fmark(const char *what)
{ static double t0 = -1.0;
  dx_mark("dx_file", &t0, what);
}

/* The encoder of the file drivers is dx_qv_encode_onepass (no size pass; the same bytes).  DEXGPU_TEST=twopass
 * selects dx_qv_sizes + dx_qv_encode instead (the two-pass API, kept as a cross-check). */
static int two_pass(void)
{ return dx_test_on("twopass"); }

/* ==========================================================================================
 *  dexqv
 * ========================================================================================== */
int dxf_quiva_index_host(quiva_index *qx, const uint8_t *text, size_t n, uint64_t *errline, int *errcode)
{ const int rc = dx_index_quiva(text, n, 0, NULL, NULL, NULL, &qx->cnt, &qx->plen, errline, errcode);
  if (rc != DX_OK) return rc;
  if (qx->cnt == 0) return DX_E_DEGENERATE;              /* empty file: the reference dereferences a NULL header (dexqv.c:94) */
  qx->off  = malloc((qx->cnt + 1) * sizeof(*qx->off));
  qx->len  = malloc((qx->cnt + 1) * sizeof(*qx->len));
  qx->hdr4 = malloc((qx->cnt + 1) * 4 * sizeof(*qx->hdr4));
  if (!qx->off || !qx->len || !qx->hdr4) return DX_E_NOMEM;
  return dx_index_quiva(text, n, qx->cnt, qx->off, qx->len, qx->hdr4, &qx->cnt, &qx->plen, errline, errcode);
}

void dxf_quiva_index_free(quiva_index *qx)
{ free(qx->off); free(qx->len); free(qx->hdr4); }

/* a slice of whole entries from e0 on: as many as make at most `cap` bytes of text (an entry larger than the cap is a slice of its own) */
static uint64_t quiva_slice_end(const quiva_index *qx, uint64_t e0, size_t cap)
{ const uint64_t s0 = e0 ? dxf_quiva_end(qx, e0 - 1) : 0;
  uint64_t e1 = e0 + 1;
  while (e1 < qx->cnt && dxf_quiva_end(qx, e1) - s0 <= cap) e1++;
  return e1;
}

dx_qv_batch dxf_qv_batch(const void *d_text, const void *d_off, const void *d_len, uint64_t m, uint64_t span, int line_pad)
{ dx_qv_batch b;
  memset(&b, 0, sizeof(b));
  b.d_text = d_text; b.d_off = d_off; b.d_len = d_len; b.n = m; b.line_pad = (uint32_t) line_pad; b.text_bytes = span;
  return b;
}

/* m entries whose text is on the device (span bytes at d_text) staged in `pool`: their header fields hdr4 framed from *lwell on (the well
   chain runs through a file's batches) and uploaded; hdr4 == NULL: no framing bytes */
int dxf_qv_stage(dpool *pool, const int32_t *hdr4, uint64_t m, int32_t *lwell, const void *d_text, const void *d_off, const void *d_len,
                    uint64_t span, int line_pad, qv_staged *s)
{ uint64_t *hoff = NULL;
  uint8_t  *blob = NULL;
  int       rc;
  memset(s, 0, sizeof(*s));
  s->b = dxf_qv_batch(d_text, d_off, d_len, m, span, line_pad);
  if (hdr4 != NULL)
    { hoff = malloc((m + 1) * sizeof(*hoff));
      blob = malloc(dx_frame_bound(hdr4, m, *lwell, 0) + 16);
      if (!hoff || !blob) { rc = DX_E_NOMEM; goto done; }
      TRY(dx_frame_headers(hdr4, NULL, m, 0, lwell, blob, hoff));
      TRY(dupload(pool, blob, (size_t) hoff[m], &s->d_hdr));
      TRY(dupload(pool, hoff, (m + 1) * 8, &s->d_hoff));
      s->hbytes = hoff[m];
    }
  TRY(dalloc(pool, (m + 1) * 8, &s->d_rec));
  TRY(dalloc(pool, m * 5 * 4, &s->d_seg));
done:
  free(hoff); free(blob);
  return rc;
}

/* Compress_Next_QVentry for a staged batch (dexqv.c:112-143) under the coding in force (cd): the records into *d_out, *total bytes of them.
   `hist` is what dx_qv_hist counted for THIS batch: it bounds the output.  *d_out holds *out_cap bytes (none yet: NULL, 0) and is made
   anew only when that is too few, so a caller with batch after batch keeps one buffer; it is the caller's to dx_free. */
int dxf_qv_encode_batch(dx_ctx *ctx, const qv_staged *s, const uint64_t (*hist)[256], const dx_qv_coding *cd, int lossy,
                           void **d_out, size_t *out_cap, uint64_t *total)
{ const int twice = two_pass();
  uint64_t  need;
  int       rc;
  if (twice) TRY(dx_qv_sizes(ctx, &s->b, s->d_hoff, s->d_seg, s->d_rec, &need));
  else       need = s->hbytes + dx_qv_out_bound(hist, s->b.n, cd, lossy);
  if (need > *out_cap || *d_out == NULL)
    { if (*d_out != NULL) { (void) dx_free(ctx, *d_out); *d_out = NULL; }
      *out_cap = 0;
      TRY(dx_malloc(ctx, (size_t) need + 64, d_out));
      *out_cap = (size_t) need;
    }
  if (twice)
    { TRY(dx_qv_encode(ctx, &s->b, s->d_hdr, s->d_hoff, s->d_rec, s->d_seg, *d_out));
      *total = need;
    }
  else
    TRY(dx_qv_encode_onepass(ctx, &s->b, s->d_hdr, s->d_hoff, s->d_seg, s->d_rec, *d_out, *out_cap, total));
done:
  return rc;
}

/* the head of a .dexqv image, dexqv.c:105-108: the key and the coding (Write_QVcoding; the prefix is the text's first plen bytes).
   *img: malloc'd, `head` bytes written, room for `more` behind them */
int dxf_qv_head(const dx_qv_coding *cd, const uint8_t *text, size_t plen, size_t more, uint8_t **img, size_t *head)
{ const uint16_t key = 0x55aa;
  size_t clen = 0;
  int    rc = dx_qv_write_coding(cd, (const char *) text, plen, NULL, 0, &clen);            /* size of Write_QVcoding */
  if (rc != DX_OK && rc != DX_E_SPACE) return rc;
  *head = 2 + clen;
  *img  = malloc(*head + more + 16);
  if (*img == NULL) return DX_E_NOMEM;
  memcpy(*img, &key, 2);
  return dx_qv_write_coding(cd, (const char *) text, plen, *img + 2, clen, &clen);
}

/* ---- a .quiva image larger than the device (or than DEXGPU_TEXT_BUDGET): slices of whole entries -------------------
 * The reference streams a file of any size through two passes (dexqv.c:81-82, 112-143).  Here: the host index of the
 * whole image (line structure, header fields), then per slice of at most `cap` bytes of text
 *   pass 1: upload, dx_qv_prescan (the scan state carried from slice to slice, entry0 = the slice's first entry),
 *           dx_qv_hist (adds into the file's histograms);
 *   tables, the file's head (key + coding) out;
 *   pass 2: upload again, dx_qv_hist once more (for the tokens of THIS slice under the final scan state; its counts go
 *           nowhere), the encoder (dxf_qv_encode_batch), the slice's records out behind the last slice's.
 * A slice is bound by the host link (two uploads of the text at ~50 GB/s against kernels at ~1.7 TB/s), so the second
 * histogram pass costs nothing that shows.  The well chain of the framing bytes runs through the slices.          */
typedef struct { uint8_t *p; size_t n, cap; } grow_sink;
static int grow_take(void *arg, uint8_t *data, size_t len, size_t at)
{ grow_sink *g = arg;
  if (at + len > g->cap)
    { size_t nc = 2 * g->cap + at + len + 4096;
      uint8_t *t = realloc(g->p, nc);
      if (t == NULL) return 1;
      g->p = t; g->cap = nc;
    }
  memcpy(g->p + at, data, len);
  if (at + len > g->n) g->n = at + len;
  return 0;
}

static int dexqv_sliced(dx_ctx *ctx, const uint8_t *text, size_t n, int lossy, size_t cap, uint8_t **out, dx_sink_fn sink, void *user,
                        size_t *out_len, uint64_t *errline, int *errcode)
{ dpool        pool = { {0}, 0, ctx }, spool = { {0}, 0, ctx };       /* spool: what lives for one slice */
  quiva_index  qx = { 0, NULL, NULL, NULL, 0 };
  uint64_t    *rel = NULL, tot = 0, e0, e1, at = 0;
  int32_t      lwell = 0;
  uint8_t     *head_img = NULL;
  size_t       head = 0, maxent = 0, slice_bytes = 0, out_cap = 0;
  dx_qv_params p = { -1, -1, -1, -1 };
  dx_qv_coding *cd = NULL;
  uint64_t   (*hist)[256] = NULL, (*junk)[256] = NULL;
  void        *d_text = NULL, *d_off = NULL, *d_len = NULL, *d_out = NULL;
  grow_sink    grow = { NULL, 0, 0 };
  int          rc, pass, was_threads = 0;

  if (out) { sink = grow_take; user = &grow; was_threads = dx_set_sink_threads(ctx, 1); }     /* (grow_take wants its chunks in order) */
  cd = malloc(sizeof(*cd)); hist = calloc(6, sizeof(*hist)); junk = calloc(6, sizeof(*junk));
  if (!cd || !hist || !junk) { rc = DX_E_NOMEM; goto done; }
  TRY(dxf_quiva_index_host(&qx, text, n, errline, errcode));
  for (e0 = 0; e0 < qx.cnt; e0 = e1)                      /* the widest slice in entries and bytes: one allocation serves them all */
    { const uint64_t s0 = e0 ? dxf_quiva_end(&qx, e0 - 1) : 0;
      e1 = quiva_slice_end(&qx, e0, cap);
      if (e1 - e0 > maxent) maxent = (size_t) (e1 - e0);
      if (dxf_quiva_end(&qx, e1 - 1) - s0 > slice_bytes) slice_bytes = (size_t) (dxf_quiva_end(&qx, e1 - 1) - s0);
    }
  rel = malloc((maxent + 1) * sizeof(*rel));
  if (!rel) { rc = DX_E_NOMEM; goto done; }
  TRY(dalloc(&pool, slice_bytes, &d_text));
  TRY(dalloc(&pool, (maxent + 1) * 8, &d_off));
  TRY(dalloc(&pool, (maxent + 1) * 4, &d_len));

  for (pass = 1; pass <= 2; pass++)
    { if (pass == 2)
        { TRY(dx_qv_build((const uint64_t (*)[256]) hist, tot, &p, lossy, cd));          /* Create_QVcoding, dexqv.c:86 */
          TRY(dx_qv_set_coding(ctx, cd, lossy));
          TRY(dxf_qv_head(cd, text, qx.plen, 0, &head_img, &head));
          if (sink(user, head_img, head, 0)) { rc = DX_E_IO; goto done; }
          at = head;
        }
      for (e0 = 0; e0 < qx.cnt; e0 = e1)
        { const uint64_t s0 = e0 ? dxf_quiva_end(&qx, e0 - 1) : 0;
          uint64_t s1, k, m, total = 0;
          dx_qv_batch b;
          e1 = quiva_slice_end(&qx, e0, cap);
          s1 = dxf_quiva_end(&qx, e1 - 1);
          m  = e1 - e0;
          for (k = 0; k < m; k++) rel[k] = qx.off[e0 + k] - s0;
          TRY(dx_h2d(ctx, d_text, text + s0, (size_t) (s1 - s0)));
          TRY(dx_h2d(ctx, d_off, rel, (size_t) m * 8));
          TRY(dx_h2d(ctx, d_len, qx.len + e0, (size_t) m * 4));
          b = dxf_qv_batch(d_text, d_off, d_len, m, s1 - s0, 1);
          if (pass == 1)
            TRY(dx_qv_scan(ctx, &b, e0, &p, hist, &tot));                               /* QV.c:993-1017, state carried along */
          else
            { uint64_t  t2 = 0;
              qv_staged st;
              shifted_sink h = { sink, user, (size_t) at };
              memset(junk, 0, 6 * sizeof(*junk));
              TRY(dx_qv_hist(ctx, &b, e0, &p, junk, &t2));                               /* this slice's tokens (and its own counts, for the bound) */
              TRY(dxf_qv_stage(&spool, qx.hdr4 + 4 * e0, m, &lwell, d_text, d_off, d_len, s1 - s0, 1, &st));
              TRY(dxf_qv_encode_batch(ctx, &st, (const uint64_t (*)[256]) junk, cd, lossy, &d_out, &out_cap, &total));
              TRY(dx_d2h_stream(ctx, d_out, total, pass_shifted, &h));
              at += total;
              dfree_all(&spool);
            }
        }
    }
  *out_len = (size_t) at;
  if (out) { *out = grow.p; grow.p = NULL; }
  rc = DX_OK;

done:
  if (was_threads) (void) dx_set_sink_threads(ctx, was_threads);
  if (d_out) dx_free(ctx, d_out);
  dfree_all(&spool);
  dfree_all(&pool);
  (void) dx_trim(ctx, DX_TRIM_TOKENS);                     /* (a slice's tokens must not meet another batch that looks like it) */
  dxf_quiva_index_free(&qx);
  free(rel); free(cd); free(hist); free(junk); free(head_img); free(grow.p);
  return rc;
}

/* how much text the device takes at once: DEXGPU_TEXT_BUDGET (bytes) when set, else what fits beside the tokens, the scratch
   regions and the output (about 2.5 bytes of device memory per byte of text), 0 = all of it */
static size_t text_cap(dx_ctx *ctx, size_t n)
{ uint64_t fr = 0, all = 0;
  size_t   cap;
  if (dxf_budget_env(n, (size_t) 4 << 20, &cap)) return cap;
  if (dx_mem_info(ctx, &fr, &all) != DX_OK || fr == 0) return 0;
  return (double) n * 2.5 > (double) fr ? (size_t) (fr / 3) : 0;
}

/* out != NULL: the image in memory; else through the sink, in order, nothing before all of it is known to exist */
/* text == NULL: the image is the first n bytes of the file behind fd (dx_file_dexqv_fd_to): uploaded by dx_h2d_fd, and whatever
   wants it in memory -- a small file, slices, the host indexer's words for a malformed one -- is DX_E_AGAIN */
static int dexqv_core(dx_ctx *ctx, const uint8_t *text, int fd, size_t n, int lossy, uint8_t **out, dx_sink_fn sink, void *user,
                      size_t *out_len, uint64_t *errline, int *errcode)
{ dpool        pool = { {0}, 0, ctx };
  uint8_t      headbuf[4096];
  quiva_index  qx = { 0, NULL, NULL, NULL, 0 };
  uint64_t     total = 0, tot = 0;
  int32_t      lwell = 0;
  uint8_t     *img = NULL;
  size_t       head = 0, out_cap = 0;
  qv_staged    st;
  dx_qv_params p = { -1, -1, -1, -1 };
  dx_qv_coding *cd = NULL;
  uint64_t   (*hist)[256] = NULL;
  void        *d_text, *d_off = NULL, *d_len = NULL, *d_out = NULL;
  int          rc;

  if (ctx == NULL || (out == NULL && sink == NULL) || out_len == NULL) return DX_E_ARG;
  if (out) *out = NULL;
  *out_len = 0;
  { const size_t cap = text_cap(ctx, n);
    if (cap)
      return text == NULL ? DX_E_AGAIN : dexqv_sliced(ctx, text, n, lossy, cap, out, sink, user, out_len, errline, errcode);
  }
  if (text == NULL && (n < DX_GPU_INDEX_MIN || dx_test_on("host_index"))) return DX_E_AGAIN;

  /* pass 1 of the reference (QVcoding_Scan, dexqv.c:81-82): validate + index.  Large images are
   * indexed on the GPU (newline scan + structure checks there, only the header lines come back);
   * small ones, and any image the GPU front end rejects (so that the message is exactly the
   * reference's first one), by the host indexer.                                               */
  cd   = malloc(sizeof(*cd));
  hist = calloc(6, sizeof(*hist));
  if (!cd || !hist) { rc = DX_E_NOMEM; goto done; }
  fmark("dexqv: begin");
  if (text != NULL) TRY(dupload(&pool, text, n, &d_text));
  else
    { size_t got = 0, want = n < sizeof(headbuf) ? n : sizeof(headbuf);
      TRY(dalloc(&pool, n, &d_text));
      TRY(dx_h2d_fd(ctx, d_text, fd, 0, n));
      while (got < want)                                  /* (the first header line, for the coding's prefix) */
        { const ssize_t k = pread(fd, headbuf + got, want - got, (off_t) got);
          if (k <= 0) { rc = DX_E_IO; goto done; }
          got += (size_t) k;
        }
    }
  fmark("dexqv: text on the device");
  if (n >= DX_GPU_INDEX_MIN && !dx_test_on("host_index"))
    { uint64_t *go = NULL; uint32_t *gl = NULL;
      rc = dx_index_quiva_device(ctx, d_text, n, &go, &gl, &qx.cnt, &qx.hdr4, &qx.plen, errline, errcode);
      if (rc == DX_OK && qx.cnt > 0)
        { if (dadopt(&pool, go) | dadopt(&pool, gl)) { rc = DX_E_NOMEM; goto done; }      /* (each of them, whatever becomes of the other) */
          d_off = go; d_len = gl;
        }
      else if (rc != DX_OK && rc != DX_E_FORMAT)
        goto done;
      else if (text == NULL)                              /* (malformed, or empty: the in-memory driver says what is wrong) */
        { rc = DX_E_AGAIN; goto done; }
      rc = DX_OK;
    }
  if (text == NULL)
    { if (qx.plen >= sizeof(headbuf)) { rc = DX_E_AGAIN; goto done; }
      text = headbuf;                                     /* (from here on only the prefix is looked at) */
    }
  if (d_off == NULL)
    { free(qx.hdr4); qx.hdr4 = NULL;
      TRY(dxf_quiva_index_host(&qx, text, n, errline, errcode));
      TRY(dupload(&pool, qx.off, qx.cnt * 8, &d_off));
      TRY(dupload(&pool, qx.len, qx.cnt * 4, &d_len));
    }
  fmark("dexqv: indexed");
  TRY(dxf_qv_stage(&pool, qx.hdr4, qx.cnt, &lwell, d_text, d_off, d_len, n, 1, &st));

  /* ... and histogram on the device (QV.c:988-1017) */
  TRY(dx_qv_scan(ctx, &st.b, 0, &p, hist, &tot));
  TRY(dx_qv_build((const uint64_t (*)[256]) hist, tot, &p, lossy, cd));   /* Create_QVcoding, dexqv.c:86 */
  TRY(dx_qv_set_coding(ctx, cd, lossy));
  fmark("dexqv: scanned, tables built");

  /* pass 2, dexqv.c:112-143: Compress_Next_QVentry for every entry */
  TRY(dxf_qv_encode_batch(ctx, &st, (const uint64_t (*)[256]) hist, cd, lossy, &d_out, &out_cap, &total));
  fmark("dexqv: encoded");
  TRY(dxf_qv_head(cd, text, qx.plen, out ? total : 0, &img, &head));
  if (out)
    { TRY(dx_d2h(ctx, img + head, d_out, total));
      *out = img; img = NULL;
    }
  else
    { shifted_sink h = { sink, user, head };
      if (sink(user, img, head, 0)) { rc = DX_E_IO; goto done; }
      TRY(dx_d2h_stream(ctx, d_out, total, pass_shifted, &h));
    }
  *out_len = head + total;
  rc = DX_OK;
  fmark("dexqv: output passed on");

done:
  if (d_out) (void) dx_free(ctx, d_out);
  dfree_all(&pool);
  dxf_quiva_index_free(&qx);
  free(cd); free(hist); free(img);
  fmark("dexqv: device memory released");
  return rc;
}

int dx_file_dexqv(dx_ctx *ctx, const uint8_t *text, size_t n, int lossy,
                  uint8_t **out, size_t *out_len, uint64_t *errline, int *errcode)
{ if (out == NULL || text == NULL) return DX_E_ARG;
  return dexqv_core(ctx, text, -1, n, lossy, out, NULL, NULL, out_len, errline, errcode);
}

int dx_file_dexqv_fd_to(dx_ctx *ctx, int fd, size_t n, int lossy, dx_sink_fn sink, void *user,
                        size_t *out_len, uint64_t *errline, int *errcode)
{ if (sink == NULL || fd < 0) return DX_E_ARG;
  return dexqv_core(ctx, NULL, fd, n, lossy, NULL, sink, user, out_len, errline, errcode);
}

int dx_file_dexqv_to(dx_ctx *ctx, const uint8_t *text, size_t n, int lossy, dx_sink_fn sink, void *user,
                     size_t *out_len, uint64_t *errline, int *errcode)
{ if (sink == NULL || text == NULL) return DX_E_ARG;
  return dexqv_core(ctx, text, -1, n, lossy, NULL, sink, user, out_len, errline, errcode);
}

/* ==========================================================================================
 *  undexqv
 * ========================================================================================== */
/* undexqv in two steps (dexgpu.h): the plan is host work only, the run is the GPU's.  The run has one path, dxf_undexqv_sliced: slices of
   whole entries, and the whole text is the case of one slice.  dx_file_undexqv_run, dx_file_verify and dx_file_digest all decode
   through it, so a check of an image takes the decoder kernels the tool's own run takes. */
void dx_file_undexqv_plan_free(dx_undexqv_plan *p)
{ if (p == NULL) return;
  dx_qv_index_free(&p->x);
  if (p->ctx != NULL)
    { dx_qv_dindex_free(p->ctx, &p->dix);
      if (p->d_in != NULL) (void) dx_free(p->ctx, p->d_in);
    }
  free(p->ooff); free(p->hat); free(p->hd.p);
  free(p);
}

int dxf_qv_header(tbuf *b, const char *prefix, const int32_t *h4)
{ int rc;
  if ((rc = dxf_tb_room(b, strlen(prefix) + 80)) != DX_OK) return rc;
  b->len += (size_t) sprintf(b->p + b->len, "%s/%d/%d_%d RQ=0.%d\n", prefix, h4[0], h4[1], h4[2], h4[3]);
  return DX_OK;
}

/* header lines (undexqv.c:182) and where every entry's lines go in the text, from p->x.n / len / hdr4 / prefix */
static int plan_layout(dx_undexqv_plan *p)
{ size_t   total = 0;
  uint64_t i;
  int      rc;
  p->ooff = malloc((p->x.n + 1) * sizeof(*p->ooff));
  p->hat  = malloc((p->x.n + 1) * sizeof(*p->hat));
  if (!p->ooff || !p->hat) return DX_E_NOMEM;
  for (i = 0; i < p->x.n; i++)
    { const int32_t *h = p->x.hdr4 + 4*i;
      p->hat[i]  = p->hd.len;
      if ((rc = dxf_qv_header(&p->hd, p->x.prefix, h)) != DX_OK) return rc;
      total     += p->hd.len - (size_t) p->hat[i];
      p->ooff[i] = total;
      total     += 5 * ((size_t) p->x.len[i] + 1);        /* undexqv.c:206-207 */
    }
  p->hat[p->x.n] = p->hd.len;
  p->ooff[p->x.n] = total;
  p->total = total;
  return DX_OK;
}

/* The plan of a large 0x55aa-keyed image with the GPU at hand: the image goes to the device (where the run wants it anyway),
   the records are walked THERE (dx_qv_walk_device: a lane per 32 KiB piece; 0.1 s for 14 GB of records where 32 host
   threads take 7.5 s), and only the entries' lengths and header fields come back for the header lines.  Whatever the device
   walk does not take -- small images (the host walk is over before the device's tables are up), 16-bit framing fields,
   walks that do not chain up, a damaged stream -- is planned on the host as before (dx_file_undexqv_plan), which also
   has the words for what is wrong with a file.  DEXGPU_TEST=host_walk: always on the host.                          */
#define DX_DEVICE_WALK_MIN ((size_t) 256 << 20)
int dx_file_undexqv_plan_on(dx_ctx *ctx, const uint8_t *img, size_t n, dx_undexqv_plan **plan, size_t *out_len)
{ dx_undexqv_plan *p;
  size_t   at = 0;
  int      rc, keep = 0;
  const size_t least = (size_t) dx_test_num("device_walk_min", (long long) DX_DEVICE_WALK_MIN);

  if (img == NULL || plan == NULL || out_len == NULL) return DX_E_ARG;
  if (ctx == NULL || n < least || n < 16 || dx_test_on("host_walk"))
    return dx_file_undexqv_plan(img, n, plan, out_len);
  *plan = NULL; *out_len = 0;
  p = calloc(1, sizeof(*p));
  if (p == NULL) return DX_E_NOMEM;
  if (dx_qv_read_head(img, n, &p->x, &at) != DX_OK || !p->x.newv) goto host;     /* the head, as dx_qv_walk reads it */
  { /* image, walk scratch (records 0.7, the lanes' words for the group index 1.1 of the image) and index (0.3) must fit together;
       asked before anything goes up (dx_qv_walk_device asks again, to the byte) */
    uint64_t fr = 0, all = 0;
    if (dx_mem_info(ctx, &fr, &all) == DX_OK && fr > 0 && 3.2 * (double) n + (double) (128 << 20) > 0.95 * (double) fr)
      goto host;
  }
  p->ctx = ctx;
  if ((rc = dx_malloc(ctx, n + 64, &p->d_in)) != DX_OK) { p->d_in = NULL; goto host; }
  if ((rc = dx_h2d(ctx, p->d_in, img, n)) != DX_OK) goto host;
  rc = dx_qv_walk_device(ctx, p->d_in, n, at, &p->x.coding, 1, p->x.flip, &p->dix);
  if (rc != DX_OK) { keep = rc != DX_E_NOMEM && rc != DX_E_HIP; goto host; }
  p->x.n    = p->dix.n;
  p->x.len  = malloc((p->x.n + 1) * sizeof(uint32_t));
  p->x.hdr4 = malloc((p->x.n + 1) * 4 * sizeof(int32_t));
  if (!p->x.len || !p->x.hdr4) { rc = DX_E_NOMEM; goto fail; }
  if (p->x.n > 0 && ((rc = dx_d2h(ctx, p->x.len, p->dix.d_len, p->x.n * 4)) != DX_OK ||
                     (rc = dx_d2h(ctx, p->x.hdr4, p->dix.d_hdr4, p->x.n * 16)) != DX_OK)) goto fail;
  p->img = img; p->n = n;
  if ((rc = plan_layout(p)) != DX_OK) goto fail;
  *plan = p; *out_len = p->total;
  return DX_OK;

host:                                                     /* not the device's: the host walk (and its verdict) */
  { void *d_in = keep ? p->d_in : NULL;                   /* an image that is up stays up: the run wants it there */
    if (d_in != NULL) p->d_in = NULL;
    dx_file_undexqv_plan_free(p);
    rc = dx_file_undexqv_plan(img, n, plan, out_len);
    if (d_in != NULL)
      { if (rc == DX_OK) { (*plan)->ctx = ctx; (*plan)->d_in = d_in; }
        else             (void) dx_free(ctx, d_in);
      }
    return rc;
  }
fail:
  dx_file_undexqv_plan_free(p);
  return rc;
}

int dx_file_undexqv_plan(const uint8_t *img, size_t n, dx_undexqv_plan **plan, size_t *out_len)
{ dx_undexqv_plan *p;
  int      rc;

  if (img == NULL || plan == NULL || out_len == NULL) return DX_E_ARG;
  *plan = NULL; *out_len = 0;
  p = calloc(1, sizeof(*p));
  if (p == NULL) return DX_E_NOMEM;
  /* boundary walk (host).  With DEXGPU_TEST=walk_index it also leaves the group index the wave-per-line decoders take
     (dx_qv_use_index below): 31 instead of 50 ms of kernels per 14 GB of records -- but the walk is 45 % longer with it
     and the index is another 30 % to upload, and from file to file that costs more than it saves (undexqv of a 1 GB
     .quiva: 0.54-0.59 s with, 0.44-0.48 s without; profiles/r03c_cli_timing.txt), so it is off unless asked for */
  rc = dx_qv_walk_indexed(img, n, &p->x, dx_test_on("walk_index"));
  if (rc != DX_OK) { free(p); return rc; }
  p->img = img; p->n = n;
  if ((rc = plan_layout(p)) != DX_OK) goto fail;
  *plan = p; *out_len = p->total;
  return DX_OK;

fail:
  dx_file_undexqv_plan_free(p);
  return rc;
}

/* The record index a plan holds, as host arrays of the caller's (dx_qv_index_free): n, rec_off, hdr_off, seg, len, hdr4, the
   coding, prefix, newv / flip -- copied from the host walk's, or downloaded when the plan was made on the device. */
int dx_file_undexqv_plan_index(const dx_undexqv_plan *p, dx_qv_index *x)
{ const uint64_t n = p ? p->x.n : 0;
  int rc = DX_OK;
  if (p == NULL || x == NULL) return DX_E_ARG;
  memset(x, 0, sizeof(*x));
  x->n = n; x->coding = p->x.coding; x->newv = p->x.newv; x->flip = p->x.flip;
  x->rec_off = malloc((n + 1) * sizeof(uint64_t));
  x->hdr_off = malloc((n + 1) * sizeof(uint64_t));
  x->seg     = malloc((n + 1) * 5 * sizeof(uint32_t));
  x->len     = malloc((n + 1) * sizeof(uint32_t));
  x->hdr4    = malloc((n + 1) * 4 * sizeof(int32_t));
  x->prefix  = malloc(strlen(p->x.prefix) + 1);
  if (!x->rec_off || !x->hdr_off || !x->seg || !x->len || !x->hdr4 || !x->prefix) { dx_qv_index_free(x); return DX_E_NOMEM; }
  strcpy(x->prefix, p->x.prefix);
  memcpy(x->len, p->x.len, n * sizeof(uint32_t));
  memcpy(x->hdr4, p->x.hdr4, n * 4 * sizeof(int32_t));
  if (PLAN_HAS_INDEX(p))
    { if ((rc = dx_d2h(p->ctx, x->rec_off, p->dix.d_rec_off, (n + 1) * 8)) == DX_OK &&
          (rc = dx_d2h(p->ctx, x->hdr_off, p->dix.d_hdr_off, (n + 1) * 8)) == DX_OK && n > 0)
        rc = dx_d2h(p->ctx, x->seg, p->dix.d_seg, n * 20);
    }
  else
    { memcpy(x->rec_off, p->x.rec_off, (n + 1) * 8);
      memcpy(x->hdr_off, p->x.hdr_off, (n + 1) * 8);
      memcpy(x->seg, p->x.seg, n * 20);
    }
  if (rc != DX_OK) dx_qv_index_free(x);
  return rc;
}

/* What a decode of a plan's records reads, on the device: the image and per record its offset, framing offset, segment sizes and length.
   What the plan has there already (dx_file_undexqv_plan_on) is taken as it is, the rest goes up into `pool`.  in_bytes > 0: the image stays
   down; d_in and d_rec are buffers for a slice's records, in_bytes of them at most in `most` records.  The coding is set, and the device
   walk's group index installed when there is one (*indexed: dx_qv_use_index takes it out again, before the plan's arrays go). */
typedef struct { void *d_in, *d_rec, *d_hoff, *d_seg, *d_len; } undexqv_staged;

static int undexqv_stage(dx_ctx *ctx, const dx_undexqv_plan *p, dpool *pool, size_t in_bytes, uint64_t most, undexqv_staged *s, int *indexed)
{ const uint64_t n = p->x.n;
  int rc;
  TRY(dx_qv_set_coding(ctx, &p->x.coding, 0));
  if (PLAN_HAS_IMAGE(p)) s->d_in = p->d_in;
  else if (!in_bytes)    TRY(dupload(pool, p->img, p->n, &s->d_in));
  else                   TRY(dalloc(pool, in_bytes, &s->d_in));
  if (PLAN_HAS_INDEX(p))
    { s->d_rec = p->dix.d_rec_off; s->d_hoff = p->dix.d_hdr_off; s->d_seg = p->dix.d_seg; s->d_len = p->dix.d_len; }
  else
    { if (!in_bytes) TRY(dupload(pool, p->x.rec_off, (n + 1) * 8, &s->d_rec));
      else           TRY(dalloc(pool, (most + 1) * 8, &s->d_rec));
      TRY(dupload(pool, p->x.hdr_off, (n + 1) * 8, &s->d_hoff));
      TRY(dupload(pool, p->x.seg, n * 5 * 4, &s->d_seg));
      TRY(dupload(pool, p->x.len, n * 4, &s->d_len));
    }
  if (PLAN_HAS_INDEX(p) && p->dix.d_gidx != NULL && !p->x.flip)     /* the run-coded lines' groups (a slice is a contiguous part of the index) */
    { TRY(dx_qv_use_dindex(ctx, s->d_in, &p->dix));
      *indexed = 1;
    }
done:
  return rc;
}

static int decode_flags(const dx_undexqv_plan *p, int upper)
{ return (upper ? DX_DECODE_UPPER : 0) | (p->x.flip ? DX_DECODE_FLIP : 0); }

/* ---- the decode of a plan's records: slices of whole entries ------------------------------------------------------------
 * The reference writes entry after entry (undexqv.c:182-207).  Here: per slice of at most `cap` bytes of text (0: the whole
 * text, one slice; else a text larger than the device, or than DEXGPU_TEXT_BUDGET), the slice's records -- the whole image
 * stays on the device when it is there already (a plan made there) or fits beside a slice's text, else the slice's bytes are
 * uploaded -- are decoded into one buffer that goes to `deliver` before the next slice comes in.  Same text; a file in several
 * slices is bound by the host link.
 * The host walk's group index (DEXGPU_TEST=walk_index: a wavefront per line, dx_qv_use_index) is for the whole image in one
 * slice; with several slices it stays out.
 * dxf_undexqv_range: the same for entries [r0, r1) alone -- who decodes two plans side by side (dx_file_compare.c) states the range
 * and gets it in slices that end at r1.                                                                                 */
int dxf_undexqv_sliced(dx_ctx *ctx, const dx_undexqv_plan *p, int upper, slice_fn deliver, void *arg, size_t cap, int whole_in_)
{ return dxf_undexqv_range(ctx, p, upper, 0, p->x.n, deliver, arg, cap, whole_in_); }

/* where the slice that begins with entry i0 ends: dxf_text_slice_end, and r1 at the latest */
static uint64_t range_slice_end(const hdr_patch *h, uint64_t i0, size_t cap, uint64_t r1)
{ const uint64_t i1 = dxf_text_slice_end(h, i0, cap);
  return i1 < r1 ? i1 : r1;
}

int dxf_undexqv_range(dx_ctx *ctx, const dx_undexqv_plan *p, int upper, uint64_t r0, uint64_t r1, slice_fn deliver, void *arg, size_t cap, int whole_in_)
{ const int whole_in = whole_in_ || PLAN_HAS_IMAGE(p);    /* (an image that is there is there whole) */
  dpool     pool = { {0}, 0, ctx };
  const uint64_t n = p->x.n;
  undexqv_staged s;
  void     *d_out = NULL, *d_ooff = NULL;
  uint64_t *rel = NULL, i0, i1, i, most = 0;
  size_t    tmax = 0, imax = 0;
  const hdr_patch h = { n, p->ooff, p->hat, p->hd.p, NULL, NULL, 0, p->total };      /* (the layout, for the slices' bounds) */
  int       rc = DX_OK, indexed = 0;
  if (r1 > n || r0 > r1) return DX_E_ARG;
  for (i0 = r0; i0 < r1; i0 = i1)                         /* the largest slice: one allocation serves them all */
    { i1 = range_slice_end(&h, i0, cap, r1);
      if (text_at(&h, i1) - text_at(&h, i0) > tmax) tmax = text_at(&h, i1) - text_at(&h, i0);
      if (i1 - i0 > most) most = i1 - i0;
      if (!whole_in && p->x.rec_off[i1] - p->x.rec_off[i0] > imax) imax = (size_t) (p->x.rec_off[i1] - p->x.rec_off[i0]);
    }
  rel = malloc((most + 1) * 2 * sizeof(*rel));
  if (rel == NULL) return DX_E_NOMEM;
  TRY(undexqv_stage(ctx, p, &pool, imax, most, &s, &indexed));
  TRY(dalloc(&pool, (most + 1) * 8, &d_ooff));
  TRY(dalloc(&pool, tmax, &d_out));
  if (p->x.gidx != NULL && !p->x.flip && whole_in && r0 == 0 && range_slice_end(&h, 0, cap, r1) == n)
    { void *d_gidx, *d_goff;
      TRY(dupload(&pool, p->x.gidx, (size_t) p->x.gidx_words * 4, &d_gidx));
      TRY(dupload(&pool, p->x.gidx_off, (n + 1) * 8, &d_goff));
      TRY(dx_qv_use_index(ctx, s.d_in, s.d_seg, n, d_gidx, d_goff, p->x.gidx_none));
      indexed = 1;
    }
  for (i0 = r0; i0 < r1; i0 = i1)
    { const size_t t0 = text_at(&h, i0);
      const uint64_t *rec = s.d_rec;
      i1 = range_slice_end(&h, i0, cap, r1);
      for (i = i0; i < i1; i++) rel[i - i0] = p->ooff[i] - t0;
      TRY(dx_h2d(ctx, d_ooff, rel, (i1 - i0) * 8));
      if (whole_in)
        rec = (const uint64_t *) s.d_rec + i0;
      else                                                /* this slice's records, their offsets from the slice's first byte */
        { const uint64_t b0 = p->x.rec_off[i0];
          for (i = i0; i <= i1; i++) rel[most + 1 + (i - i0)] = p->x.rec_off[i] - b0;
          TRY(dx_h2d(ctx, s.d_in, p->img + b0, (size_t) (p->x.rec_off[i1] - b0)));
          TRY(dx_h2d(ctx, s.d_rec, rel + most + 1, (i1 - i0 + 1) * 8));
        }
      fmark("undexqv: buffers ready");
      TRY(dx_qv_decode(ctx, s.d_in, rec, (const uint64_t *) s.d_hoff + i0, (const uint32_t *) s.d_seg + 5 * i0, (const uint32_t *) s.d_len + i0, i1 - i0,
                       decode_flags(p, upper), d_out, d_ooff));
      fmark("undexqv: decoded");
      TRY(deliver(arg, d_out, i0, i1, t0, text_at(&h, i1) - t0));
      fmark("undexqv: text passed on");
    }
done:
  if (indexed) (void) dx_qv_use_index(ctx, NULL, NULL, 0, NULL, NULL, 0);     /* (either index: the host walk's lives in the pool freed below) */
  dfree_all(&pool);
  free(rel);
  return rc == SLICE_STOP ? DX_OK : rc;
}

/* does the text fit beside the image?  DEXGPU_TEXT_BUDGET (bytes) says how much text the device takes at once; else what is free
   decides: the image (unless it is there already), the index and the text, and a tenth to spare.  0: all of it at once; else the
   bytes of text a slice may have, and *whole_in: the image goes up whole beside them */
size_t dxf_undexqv_cap(dx_ctx *ctx, const dx_undexqv_plan *p, int *whole_in)
{ uint64_t fr = 0, all = 0;
  size_t   cap = 0;
  *whole_in = 1;
  if (dxf_budget_env(p->total, 65536u, &cap)) return cap;
  if (dx_mem_info(ctx, &fr, &all) == DX_OK && fr > 0)
    { const double in = PLAN_HAS_IMAGE(p) ? 0.0 : (double) p->n;
      if (in + (double) p->total + 48.0 * (double) p->x.n > 0.9 * (double) fr)
        { *whole_in = in <= 0.4 * (double) fr;
          cap = (size_t) ((0.9 * (double) fr - (*whole_in ? in : 0.0) - 48.0 * (double) p->x.n) / (*whole_in ? 1.0 : 1.4));
          if (cap < ((size_t) 4 << 20)) cap = (size_t) 4 << 20;
        }
    }
  return cap;
}

int dx_file_undexqv_run(dx_ctx *ctx, const dx_undexqv_plan *p, int upper, dx_sink_fn sink, void *user)
{ size_t cap;
  int    whole_in;

  if (ctx == NULL || p == NULL || sink == NULL) return DX_E_ARG;
  if (p->ctx != NULL && p->ctx != ctx) return DX_E_ARG;   /* (a plan made on a device runs there) */
  if (p->x.n == 0) return DX_OK;
  cap = dxf_undexqv_cap(ctx, p, &whole_in);
  if (cap && dx_test_on("slice_input") && !PLAN_HAS_IMAGE(p)) whole_in = 0;      /* (DEXGPU_TEST=slice_input) */
  { hdr_patch h = { p->x.n, p->ooff, p->hat, p->hd.p, sink, user, 0, p->total };
    slice_out so = { ctx, &h, NULL };
    return dxf_undexqv_sliced(ctx, p, upper, dxf_slice_deliver, &so, cap, whole_in);
  }
}

typedef struct { uint8_t *res; } mem_sink;
static int to_memory(void *user, uint8_t *data, size_t len, size_t at)
{ memcpy(((mem_sink *) user)->res + at, data, len);
  return 0;
}

int dx_file_undexqv(dx_ctx *ctx, const uint8_t *img, size_t n, int upper, uint8_t **out, size_t *out_len)
{ dx_undexqv_plan *p = NULL;
  mem_sink m = { NULL };
  size_t   total = 0;
  int      rc;

  if (ctx == NULL || out == NULL || out_len == NULL || img == NULL) return DX_E_ARG;
  *out = NULL; *out_len = 0;
  rc = dx_file_undexqv_plan_on(ctx, img, n, &p, &total);
  if (rc != DX_OK) return rc;
  m.res = malloc(total + 16);
  if (m.res == NULL) rc = DX_E_NOMEM;
  else               rc = dx_file_undexqv_run(ctx, p, upper, to_memory, &m);
  if (rc == DX_OK) { *out = m.res; *out_len = total; }
  else             free(m.res);
  dx_file_undexqv_plan_free(p);
  return rc;
}
