/*
 * dx_file_subset.c -- a new .dexta / .dexar / .dexqv image cut out of an old one: a list of records, whole or an interval of each, becomes
 * the file dexta / dexar / dexqv [-l] writes for the text undexta / undexar / undexqv prints for those records alone -- and no text is made
 * on the way for the 2-bit kinds, none leaves the device for quiva.
 *
 *     dx_file_subset_layout   host only: the 2-bit kinds' new framing, and the units dx_reads_repack takes
 *     dx_file_subset          the layout, the packed reads re-packed where the framing left room for them (2-bit kinds); the selected
 *                             entries decoded, gathered, scanned and coded anew (quiva)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dexgpu.h"
#include "dx_env.h"
#include "dx_host.h"
#include "dx_files.h"

/* ==========================================================================================
 *  the selection (dx_files.h): unit j is record ids[j] (ids == NULL: j), all of it or its symbols [beg[j], end[j])
 * ========================================================================================== */
int dxf_sel_check(dx_ctx *ctx, const char *who, selection *s, uint64_t cnt, const uint32_t *rlen, int ordered)
{ uint64_t j, last = 0;
  if (s->ids == NULL && s->n == UINT64_MAX)               /* every record of the image */
    { if (cnt == 0) return DX_E_DEGENERATE;
      s->n = cnt;
    }
  for (j = 0; j < s->n; j++)
    { const uint64_t id = sel_id(s, j);
      if (ordered && id < last) return dx_unit_fail(ctx, DX_E_ARG, who, j, "its id is below the one in front of it");
      if (id >= cnt)  return dx_unit_fail(ctx, DX_E_ARG, who, j, "its id is not below the image's record count");
      if (s->beg != NULL && s->beg[j] > s->end[j]) return dx_unit_fail(ctx, DX_E_ARG, who, j, "beg > end");
      if (s->beg != NULL && s->end[j] > rlen[id])  return dx_unit_fail(ctx, DX_E_ARG, who, j, "end > the record's length");
      last = id;
    }
  return DX_OK;
}

int dxf_sel_args(dx_ctx *ctx, const char *who, const uint8_t *img, const uint64_t *ids, const uint32_t *beg, const uint32_t *end, uint64_t n_ids)
{ if (img == NULL) return DX_E_ARG;
  if ((beg == NULL) != (end == NULL))
    return dx_unit_fail(ctx, DX_E_ARG, who, 0, "beg and end are given together, or neither");
  if (n_ids == UINT64_MAX && (ids != NULL || beg != NULL))              /* (every record whole: no arrays to go with it) */
    return dx_unit_fail(ctx, DX_E_ARG, who, 0, "n_ids == UINT64_MAX (every record) goes with ids == beg == end == NULL");
  return n_ids == 0 ? DX_E_DEGENERATE : DX_OK;
}

/* dx_file_subset's own: its ids do not decrease (dexta's well-delta chain cannot say otherwise) */
static int sel_check(dx_ctx *ctx, selection *s, uint64_t cnt, const uint32_t *rlen) { return dxf_sel_check(ctx, "dx_file_subset", s, cnt, rlen, 1); }

static int sel_args(dx_ctx *ctx, const uint8_t *img, const uint64_t *ids, const uint32_t *beg, const uint32_t *end, uint64_t n_ids)
{ return dxf_sel_args(ctx, "dx_file_subset", img, ids, beg, end, n_ids); }

/* ==========================================================================================
 *  fasta / arrow: the framing anew (dexta.c:124-129, 187-198; dexar.c:193-204), the payload where it lies
 * ========================================================================================== */
typedef struct
  { u2_index  x;                                 /* the image's records */
    uint8_t  *frame;  size_t total;              /* the new image: every byte but the payload's (those are 0) */
    uint64_t *src_off, *dst_off;                 /* per unit: where its read begins in the image, where its payload goes in the new one */
    uint32_t *src_beg, *len;                     /* ... the symbols [src_beg, src_beg + len) of that read */
  } subset2;

static void subset2_free(subset2 *p)
{ dxf_u2_index_free(&p->x);
  free(p->frame); free(p->src_off); free(p->dst_off); free(p->src_beg); free(p->len);
  memset(p, 0, sizeof(*p));
}

/* an error leaves what there is to subset2_free */
static int subset2_plan(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, selection *s, subset2 *p)
{ const int arrow = kind == DX_KIND_ARROW;
  uint64_t  n;
  int32_t  *hdr4 = NULL, lwell = 0, plen;
  uint16_t *cnr4 = NULL, key;
  uint64_t *hoff = NULL, j;
  uint8_t  *blob = NULL;
  size_t    at;
  int       rc;

  TRY(dxf_u2_walk(arrow ? DX_LETTERS_ARROW : DX_LETTERS_LOWER, img, m, NULL, &p->x));
  TRY(sel_check(ctx, s, p->x.cnt, p->x.nsym));
  n = s->n;
  memcpy(&key, img, 2); memcpy(&plen, img + 2, 4);        /* (the walk has seen to it that both are there) */
  if (key == 0xaa55 || key == 0xcc33) plen = (int32_t) flip32((uint32_t) plen);

  hdr4 = malloc((n + 1) * 4 * sizeof(*hdr4)); cnr4 = malloc((n + 1) * 4 * sizeof(*cnr4)); hoff = malloc((n + 1) * sizeof(*hoff));
  p->src_off = malloc((n + 1) * sizeof(*p->src_off)); p->dst_off = malloc((n + 1) * sizeof(*p->dst_off));
  p->src_beg = malloc((n + 1) * sizeof(*p->src_beg)); p->len = malloc((n + 1) * sizeof(*p->len));
  if (!hdr4 || !cnr4 || !hoff || !p->src_off || !p->dst_off || !p->src_beg || !p->len) { rc = DX_E_NOMEM; goto done; }
  for (j = 0; j < n; j++)                                 /* well/B_E becomes well/(B + beg)_(B + end); qv and the SN words as they are */
    { const uint64_t id = sel_id(s, j);
      const int32_t *h  = p->x.hdr4 + 4 * id;
      const uint32_t b  = sel_beg(s, j), e = sel_end(s, j, p->x.nsym);
      hdr4[4*j] = h[0]; hdr4[4*j + 1] = h[1] + (int32_t) b; hdr4[4*j + 2] = h[1] + (int32_t) e; hdr4[4*j + 3] = h[3];
      memcpy(cnr4 + 4*j, p->x.cnr4 + 4 * id, 4 * sizeof(*cnr4));
      p->src_off[j] = p->x.ioff[id]; p->src_beg[j] = b; p->len[j] = e - b;
    }
  blob = malloc(dx_frame_bound(hdr4, n, 0, arrow) + 16);
  if (blob == NULL) { rc = DX_E_NOMEM; goto done; }
  TRY(dx_frame_headers(hdr4, cnr4, n, arrow, &lwell, blob, hoff));        /* the well chain from 0 on, over the selected records */

  at = 2 + 4 + (size_t) plen;
  for (j = 0; j < n; j++) at += (size_t) (hoff[j + 1] - hoff[j]) + (((size_t) p->len[j] + 3) >> 2);
  p->total = at;
  if ((p->frame = calloc(p->total + 16, 1)) == NULL) { rc = DX_E_NOMEM; goto done; }
  key = 0x55aa;                                           /* key, prefix length, prefix (dexta.c:124-129): the image's own prefix */
  memcpy(p->frame, &key, 2); memcpy(p->frame + 2, &plen, 4); memcpy(p->frame + 6, img + 6, (size_t) plen);
  at = 2 + 4 + (size_t) plen;
  for (j = 0; j < n; j++)
    { const size_t hl = (size_t) (hoff[j + 1] - hoff[j]);
      memcpy(p->frame + at, blob + hoff[j], hl);
      p->dst_off[j] = at + hl;
      at += hl + (((size_t) p->len[j] + 3) >> 2);
    }
  rc = DX_OK;
done:
  free(hdr4); free(cnr4); free(hoff); free(blob);
  return rc;
}

int dx_file_subset_layout(int kind, const uint8_t *img, size_t m,
                          const uint64_t *ids, const uint32_t *beg, const uint32_t *end, uint64_t n_ids,
                          uint8_t **frame, size_t *out_len,
                          uint64_t **src_off, uint32_t **src_beg, uint32_t **len, uint64_t **dst_off)
{ selection s = { ids, beg, end, n_ids };
  subset2 p;
  int     rc;
  if (frame == NULL || out_len == NULL || (kind != DX_KIND_FASTA && kind != DX_KIND_ARROW)) return DX_E_ARG;
  *frame = NULL; *out_len = 0;
  if (src_off) *src_off = NULL;
  if (src_beg) *src_beg = NULL;
  if (len)     *len = NULL;
  if (dst_off) *dst_off = NULL;
  if ((rc = sel_args(NULL, img, ids, beg, end, n_ids)) != DX_OK) return rc;
  if (n_ids == UINT64_MAX && (src_off || src_beg || len || dst_off))     /* (arrays of a length the call does not hand back) */
    return dx_unit_fail(NULL, DX_E_ARG, "dx_file_subset_layout", 0, "n_ids == UINT64_MAX (every record) gives the frame alone: name the units to have their arrays");
  memset(&p, 0, sizeof(p));
  if ((rc = subset2_plan(NULL, kind, img, m, &s, &p)) == DX_OK)
    { *frame = p.frame; *out_len = p.total; p.frame = NULL;
      if (src_off) { *src_off = p.src_off; p.src_off = NULL; }
      if (src_beg) { *src_beg = p.src_beg; p.src_beg = NULL; }
      if (len)     { *len = p.len; p.len = NULL; }
      if (dst_off) { *dst_off = p.dst_off; p.dst_off = NULL; }
    }
  subset2_free(&p);
  return rc;
}

/* how much of a 2-bit image of m bytes the device takes at once beside the new image and 32 bytes of arrays a unit: 0 = all of it.
   DEXGPU_TEXT_BUDGET counts bytes of image here, as for the census (there is no text) */
static size_t subset2_cap(dx_ctx *ctx, size_t m, size_t total, uint64_t units)
{ uint64_t fr = 0, all = 0;
  size_t   cap;
  if (dxf_budget_env(m, 4096u, &cap)) return cap;
  if (dx_mem_info(ctx, &fr, &all) != DX_OK || fr == 0) return 0;
  if ((double) m + (double) total + 32.0 * (double) units <= 0.9 * (double) fr) return 0;
  { const double room = (0.9 * (double) fr) / 3.0;
    return room > (double) ((size_t) 4 << 20) ? (size_t) room : (size_t) 4 << 20;
  }
}


/* where unit j's framing begins in the new image (j == n: where the image ends; unit 0 takes the file's head along) */
static size_t unit_at(const subset2 *p, uint64_t n, uint64_t j)
{ return j == 0 ? 0 : (j == n ? p->total : (size_t) p->dst_off[j - 1] + (((size_t) p->len[j - 1] + 3) >> 2)); }

/* The payload into the frame: slices of whole source records of at most `cap` bytes of image (0: in one), those without a selected record
   left out; a slice whose units would make more than `cap` bytes of the new image ends early, and the next one begins with the record it
   stopped in (one unit at least a slice).  A slice's part of the image goes up, and its part of the frame; dx_reads_repack writes the payload between the framing
   bytes there; the part comes back. */
static int subset2_run(dx_ctx *ctx, const uint8_t *img, const selection *s, subset2 *p, size_t cap)
{ const uint64_t n = s->n;
  uint64_t *rel = NULL, j, j0, j1;
  void     *d_in = NULL, *d_out = NULL, *d_arr = NULL;
  size_t    in_cap = 0, out_cap = 0, arr_cap = 0;
  int       rc = DX_OK;
  for (j0 = 0; j0 < n; j0 = j1)
    { const uint64_t i0 = sel_id(s, j0), b0 = p->x.ioff[i0];
      uint64_t i1 = i0 + 1, m, b1;
      size_t   o0, o1;
      while (cap != 0 && i1 < p->x.cnt && dxf_u2_end(&p->x, i1) - b0 <= cap) i1++;
      if (cap == 0) i1 = p->x.cnt;
      o0 = unit_at(p, n, j0);                              /* ... and of at most `cap` bytes of the new image: an id may repeat without end */
      for (j1 = j0; j1 < n && sel_id(s, j1) < i1 && (cap == 0 || j1 == j0 || unit_at(p, n, j1 + 1) - o0 <= cap); j1++) ;
      m  = j1 - j0;
      b1 = dxf_u2_end(&p->x, sel_id(s, j1 - 1));               /* (from the first selected record to the last: ids do not decrease) */
      o1 = unit_at(p, n, j1);
      { uint64_t *t = realloc(rel, (size_t) (2 * m + 1) * sizeof(*rel));
        if (t == NULL) { rc = DX_E_NOMEM; goto done; }
        rel = t;
      }
      for (j = 0; j < m; j++)
        { rel[j]     = p->src_off[j0 + j] - b0;
          rel[m + j] = p->dst_off[j0 + j] - o0;
        }
      TRY(dgrow(ctx, &d_in, &in_cap, (size_t) (b1 - b0) + 64));
      TRY(dgrow(ctx, &d_out, &out_cap, (o1 - o0) + 64));
      TRY(dgrow(ctx, &d_arr, &arr_cap, (size_t) m * 24 + 64));            /* source and destination offsets (8 each), first symbols, lengths (4 each) */
      { uint64_t *d_soff = d_arr, *d_doff = d_soff + m;
        uint32_t *d_beg = (uint32_t *) (d_doff + m), *d_len = d_beg + m;
        TRY(dx_h2d(ctx, d_in, img + b0, (size_t) (b1 - b0)));
        TRY(dx_h2d(ctx, d_out, p->frame + o0, o1 - o0));
        TRY(dx_h2d(ctx, d_soff, rel, (size_t) m * 16));
        TRY(dx_h2d(ctx, d_beg, p->src_beg + j0, (size_t) m * 4));
        TRY(dx_h2d(ctx, d_len, p->len + j0, (size_t) m * 4));
        TRY(dx_reads_repack(ctx, d_in, b1 - b0, d_soff, d_beg, d_len, m, d_out, d_doff, NULL));
        TRY(dx_d2h(ctx, p->frame + o0, d_out, o1 - o0));
      }
    }
done:
  if (d_in) (void) dx_free(ctx, d_in);
  if (d_out) (void) dx_free(ctx, d_out);
  if (d_arr) (void) dx_free(ctx, d_arr);
  free(rel);
  return rc;
}

/* ==========================================================================================
 *  quiva: the selected entries' text, decoded and cut on the device, is a .quiva of its own -- scanned, its coding built, its entries
 *  compressed as dexqv does it (dexqv.c:81-143), in the two passes of dexqv_sliced (dx_file_qv.c) with decoded slices
 *  (dxf_undexqv_sliced) in place of uploaded ones.  A dx_qv_batch fixes an entry's line stride at its length + line_pad, so the
 *  five intervals of an entry are gathered first (dx_copy_ranges, five units an entry; whole entries alike), a newline behind each.
 * ========================================================================================== */
typedef struct
  { dx_ctx                *ctx;
    const dx_undexqv_plan *p;
    const selection       *s;
    int                    lossy, pass;            /* pass: 1 scans, 2 codes */
    uint64_t               j;                      /* the units of the slices so far in this pass */
    dx_qv_params           par;
    dx_qv_coding          *cd;
    uint64_t             (*hist)[256], (*junk)[256], tot;
    int32_t                lwell;
    uint8_t               *img;   size_t at, cap;  /* the new image: `at` bytes of it so far */
    void                  *d_text, *d_arr, *d_bat, *d_enc;   /* device: a slice's gathered text; its ranges; its batch arrays; its records */
    size_t                 text_cap, arr_cap, bat_cap, enc_cap;
    dpool                  spool;                  /* what lives for one slice's encode */
    /* The scan's first batch when the text comes in several slices.  dx_qv_scan looks for the substitution run character among the
       entries of the batch with entry0 == 0, up to the one with which the symbols reach 100000 (QV.c:1006-1015), so units [0, first_n),
       the shortest such head of the selection, are gathered side by side from slice to slice and scanned together. */
    uint64_t               first_n, first_fill;    /* its units; the bytes gathered so far */
    void                  *d_first;
    uint64_t              *first_off;
    uint32_t              *first_len;
  } qsub_job;

#define QV_SUBCHAR_SYMBOLS 100000u                 /* QV.c:1006 */

static uint32_t qsub_len(const qsub_job *q, uint64_t j)
{ return sel_end(q->s, j, q->p->x.len) - sel_beg(q->s, j); }

/* the gathered text of units [ja, jb): five lines and five newlines each */
static uint64_t qsub_span(const qsub_job *q, uint64_t ja, uint64_t jb)
{ uint64_t j, span = 0;
  for (j = ja; j < jb; j++) span += 5 * ((uint64_t) qsub_len(q, j) + 1);
  return span;
}

/* the coding of the scanned selection and the new image's head (Create_QVcoding, Write_QVcoding: dexqv.c:86, 105-108) */
static int qsub_head(qsub_job *q)
{ size_t head = 0;
  int    rc;
  if ((rc = dx_qv_build((const uint64_t (*)[256]) q->hist, q->tot, &q->par, q->lossy, q->cd)) != DX_OK) return rc;
  if ((rc = dxf_qv_head(q->cd, (const uint8_t *) q->p->x.prefix, strlen(q->p->x.prefix), 0, &q->img, &head)) != DX_OK) return rc;
  q->at = q->cap = head;
  return DX_OK;
}

/* Units [ja, jb), whose entries stand in the slice of decoded text at d_out (`bytes` of it, the first at t0 in the whole text), gathered
   at d_dst from `base` on (newlines are there already).  off, len32: the units as a dx_qv_batch wants them; hdr4 (may be NULL): their
   header fields, well/B_E become well/(B + beg)_(B + end) */
static int qsub_gather(qsub_job *q, const void *d_out, size_t t0, size_t bytes, uint64_t ja, uint64_t jb, void *d_dst, uint64_t base,
                       uint64_t *off, uint32_t *len32, int32_t *hdr4)
{ const dx_undexqv_plan *p = q->p;
  const uint64_t m = jb - ja;
  uint64_t *soff, *ln, *doff, k, at = base;
  int       rc;
  if ((soff = malloc((size_t) m * 120 + 64)) == NULL) return DX_E_NOMEM;            /* five ranges a unit: source, length, destination */
  ln = soff + 5 * m; doff = ln + 5 * m;
  for (k = 0; k < m; k++)
    { const uint64_t id = sel_id(q->s, ja + k), L = p->x.len[id];
      const uint32_t b = sel_beg(q->s, ja + k), l = qsub_len(q, ja + k);
      const int32_t *ph = p->x.hdr4 + 4 * id;
      int line;
      for (line = 0; line < 5; line++)
        { soff[5*k + line] = p->ooff[id] - t0 + (uint64_t) line * (L + 1) + b;
          ln[5*k + line]   = l;
          doff[5*k + line] = at + (uint64_t) line * ((uint64_t) l + 1);
        }
      off[k] = at; len32[k] = l;
      if (hdr4 != NULL)
        { hdr4[4*k] = ph[0]; hdr4[4*k + 1] = ph[1] + (int32_t) b; hdr4[4*k + 2] = ph[1] + (int32_t) (b + l); hdr4[4*k + 3] = ph[3]; }
      at += 5 * ((uint64_t) l + 1);
    }
  TRY(dgrow(q->ctx, &q->d_arr, &q->arr_cap, (size_t) m * 120 + 64));
  TRY(dx_h2d(q->ctx, q->d_arr, soff, (size_t) m * 120));
  { const uint64_t *d_soff = q->d_arr, *d_ln = d_soff + 5 * m, *d_doff = d_ln + 5 * m;
    TRY(dx_copy_ranges(q->ctx, d_out, bytes, d_soff, d_ln, 5 * m, d_dst, d_doff, NULL));
  }
done:
  free(soff);
  return rc;
}

/* m units at d_text as a batch: their offsets and lengths up */
static int qsub_batch(qsub_job *q, const void *d_text, uint64_t span, const uint64_t *off, const uint32_t *len32, uint64_t m, dx_qv_batch *b)
{ int rc;
  if ((rc = dgrow(q->ctx, &q->d_bat, &q->bat_cap, (size_t) m * 12 + 64)) != DX_OK) return rc;
  if ((rc = dx_h2d(q->ctx, q->d_bat, off, (size_t) m * 8)) != DX_OK) return rc;
  if ((rc = dx_h2d(q->ctx, (uint64_t *) q->d_bat + m, len32, (size_t) m * 4)) != DX_OK) return rc;
  *b = dxf_qv_batch(d_text, q->d_bat, (uint64_t *) q->d_bat + m, m, span, 1);
  return DX_OK;
}

/* Compress_Next_QVentry for a slice's gathered units [j0, j0 + b->n) (dexqv.c:112-143), their records behind the image so far */
static int qsub_code(qsub_job *q, const dx_qv_batch *b, uint64_t j0, const int32_t *hdr4)
{ uint64_t  t2 = 0, total = 0;
  qv_staged st;
  int       rc;
  TRY(dx_qv_set_coding(q->ctx, q->cd, q->lossy));
  memset(q->junk, 0, 6 * sizeof(*q->junk));
  TRY(dx_qv_hist(q->ctx, b, j0, &q->par, q->junk, &t2));                  /* this slice's tokens (and its own counts, for the bound) */
  TRY(dxf_qv_stage(&q->spool, hdr4, b->n, &q->lwell, b->d_text, b->d_off, b->d_len, b->text_bytes, 1, &st));
  TRY(dxf_qv_encode_batch(q->ctx, &st, (const uint64_t (*)[256]) q->junk, q->cd, q->lossy, &q->d_enc, &q->enc_cap, &total));
  if (q->at + total > q->cap)
    { const size_t nc = 2 * q->cap + (size_t) total + 4096;
      uint8_t *t = realloc(q->img, nc + 16);
      if (t == NULL) { rc = DX_E_NOMEM; goto done; }
      q->img = t; q->cap = nc;
    }
  TRY(dx_d2h(q->ctx, q->img + q->at, q->d_enc, (size_t) total));
  q->at += (size_t) total;
done:
  dfree_all(&q->spool);
  return rc;
}

/* pass 1 of a text in several slices, the slice's units [ja, jb) that belong to the scan's first batch: gathered behind those that are
   there, and the batch scanned once it is complete */
static int qsub_first(qsub_job *q, const void *d_out, size_t t0, size_t bytes, uint64_t ja, uint64_t jb)
{ dx_qv_batch b;
  int rc;
  if ((rc = qsub_gather(q, d_out, t0, bytes, ja, jb, q->d_first, q->first_fill, q->first_off + ja, q->first_len + ja, NULL)) != DX_OK) return rc;
  q->first_fill += qsub_span(q, ja, jb);
  if (jb < q->first_n) return DX_OK;
  if ((rc = qsub_batch(q, q->d_first, q->first_fill, q->first_off, q->first_len, q->first_n, &b)) != DX_OK) return rc;
  return dx_qv_scan(q->ctx, &b, 0, &q->par, q->hist, &q->tot);             /* QV.c:993-1017 */
}

/* a slice of decoded text, entries [i0, i1): its selected units gathered, then scanned (pass 1) or coded (pass 2).  A slice that is the
   whole text is scanned and coded where it lies: the second pass is not made */
static int qsub_slice(void *arg, const void *d_out, uint64_t i0, uint64_t i1, size_t t0, size_t bytes)
{ qsub_job *q = arg;
  const selection *s = q->s;
  const int whole = i0 == 0 && i1 == q->p->x.n;
  uint64_t  ja = q->j, jb, m, span, *off = NULL;
  int       rc = DX_OK;
  for (jb = ja; jb < s->n && sel_id(s, jb) < i1; jb++) ;
  q->j = jb;
  if (q->pass == 1 && !whole && ja < q->first_n)          /* the head of the selection: the scan's first batch */
    { const uint64_t je = jb < q->first_n ? jb : q->first_n;
      if (je > ja && (rc = qsub_first(q, d_out, t0, bytes, ja, je)) != DX_OK) return rc;
      ja = je;
    }
  m = jb - ja;
  if (m > 0)
    { uint32_t   *len32;
      int32_t    *hdr4;
      dx_qv_batch b;
      if ((off = malloc((size_t) m * 28 + 64)) == NULL) return DX_E_NOMEM;          /* place (8), symbols a line (4), header fields (16) */
      len32 = (uint32_t *) (off + m); hdr4 = (int32_t *) (len32 + m);
      span  = qsub_span(q, ja, jb);
      TRY(dgrow(q->ctx, &q->d_text, &q->text_cap, (size_t) span + 64));
      TRY(dx_memset(q->ctx, q->d_text, '\n', (size_t) span));
      TRY(qsub_gather(q, d_out, t0, bytes, ja, jb, q->d_text, 0, off, len32, hdr4));
      TRY(qsub_batch(q, q->d_text, span, off, len32, m, &b));
      if (q->pass == 1)
        { TRY(dx_qv_scan(q->ctx, &b, ja, &q->par, q->hist, &q->tot));     /* QV.c:993-1017, state carried along */
          if (whole) TRY(qsub_head(q));
        }
      if (q->pass == 2 || whole)
        { TRY(qsub_code(q, &b, ja, hdr4));
          if (!whole) TRY(dx_qv_set_coding(q->ctx, &q->p->x.coding, 0));  /* (the next slice is decoded under the image's coding) */
        }
    }
  if (whole) q->pass = 2;
  if (whole || jb == s->n) rc = SLICE_STOP;
done:
  free(off);
  return rc;
}

static int subset_qv(dx_ctx *ctx, const uint8_t *img, size_t m, selection *s, int lossy, uint8_t **out, size_t *out_len)
{ dx_undexqv_plan *p = NULL;
  qsub_job q;
  size_t   total = 0, cap;
  int      rc, whole_in = 1;
  memset(&q, 0, sizeof(q));
  q.ctx = ctx; q.s = s; q.lossy = lossy; q.spool.ctx = ctx;
  q.par.delChar = q.par.subChar = -1; q.par.del_first = q.par.sub_first = -1;
  TRY(dx_file_undexqv_plan_on(ctx, img, m, &p, &total));
  q.p = p;
  TRY(sel_check(ctx, s, p->x.n, p->x.len));
  q.cd = malloc(sizeof(*q.cd)); q.hist = calloc(6, sizeof(*q.hist)); q.junk = calloc(6, sizeof(*q.junk));
  if (!q.cd || !q.hist || !q.junk) { rc = DX_E_NOMEM; goto done; }

  cap = dxf_undexqv_cap(ctx, p, &whole_in);
  if (cap == 0)                                           /* (the gathered text and its records stand beside the decoded text) */
    { uint64_t fr = 0, all = 0;
      const double in = PLAN_HAS_IMAGE(p) ? 0.0 : (double) m;
      if (dx_mem_info(ctx, &fr, &all) == DX_OK && fr > 0 && in + 3.0 * (double) total > 0.9 * (double) fr)
        { const double room = (0.9 * (double) fr - in) / 3.0;
          cap = room > (double) ((size_t) 4 << 20) ? (size_t) room : (size_t) 4 << 20;
        }
    }
  if (cap != 0)                                           /* (several slices, it may be: room for the scan's first batch) */
    { uint64_t sym = 0, span;
      while (q.first_n < s->n && sym < QV_SUBCHAR_SYMBOLS) sym += qsub_len(&q, q.first_n++);
      span = qsub_span(&q, 0, q.first_n);
      q.first_off = malloc((q.first_n + 1) * sizeof(*q.first_off)); q.first_len = malloc((q.first_n + 1) * sizeof(*q.first_len));
      if (!q.first_off || !q.first_len) { rc = DX_E_NOMEM; goto done; }
      TRY(dx_malloc(ctx, (size_t) span + 64, &q.d_first));
      TRY(dx_memset(ctx, q.d_first, '\n', (size_t) span));
    }
  q.pass = 1;
  TRY(dxf_undexqv_sliced(ctx, p, 0, qsub_slice, &q, cap, whole_in));
  if (q.pass == 1)                                        /* several slices: the coding, then the text once more */
    { TRY(qsub_head(&q));
      q.pass = 2; q.j = 0;
      TRY(dxf_undexqv_sliced(ctx, p, 0, qsub_slice, &q, cap, whole_in));
    }
  *out = q.img; *out_len = q.at; q.img = NULL;
  rc = DX_OK;
done:
  if (q.d_text) (void) dx_free(ctx, q.d_text);
  if (q.d_arr) (void) dx_free(ctx, q.d_arr);
  if (q.d_bat) (void) dx_free(ctx, q.d_bat);
  if (q.d_enc) (void) dx_free(ctx, q.d_enc);
  if (q.d_first) (void) dx_free(ctx, q.d_first);
  dfree_all(&q.spool);
  (void) dx_trim(ctx, DX_TRIM_TOKENS);                     /* (a slice's tokens must not meet another batch that looks like it) */
  dx_file_undexqv_plan_free(p);
  free(q.cd); free(q.hist); free(q.junk); free(q.img); free(q.first_off); free(q.first_len);
  return rc;
}

int dx_file_subset(dx_ctx *ctx, int kind, const uint8_t *img, size_t m,
                   const uint64_t *ids, const uint32_t *beg, const uint32_t *end, uint64_t n_ids,
                   int lossy, uint8_t **out, size_t *out_len)
{ selection s = { ids, beg, end, n_ids };
  int rc;
  if (ctx == NULL || out == NULL || out_len == NULL) return DX_E_ARG;
  if (kind != DX_KIND_FASTA && kind != DX_KIND_ARROW && kind != DX_KIND_QUIVA) return DX_E_ARG;
  *out = NULL; *out_len = 0;
  if ((rc = sel_args(ctx, img, ids, beg, end, n_ids)) != DX_OK) return rc;
  if (kind == DX_KIND_QUIVA) return subset_qv(ctx, img, m, &s, lossy, out, out_len);
  { subset2 p;
    memset(&p, 0, sizeof(p));
    rc = subset2_plan(ctx, kind, img, m, &s, &p);
    if (rc == DX_OK) rc = subset2_run(ctx, img, &s, &p, subset2_cap(ctx, m, p.total, s.n));
    if (rc == DX_OK) { *out = p.frame; *out_len = p.total; p.frame = NULL; }
    subset2_free(&p);
  }
  return rc;
}
