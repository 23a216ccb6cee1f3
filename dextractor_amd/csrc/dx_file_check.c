/*
 * dx_file_check.c -- an image of any of the three kinds and the text it decodes to, for who wants the text's slices where they are
 * made: the round-trip check (dx_file_verify), the digest (dx_file_digest) and the census (dx_file_census).
 */
#include <stdlib.h>
#include <string.h>

#include "dexgpu.h"
#include "dx_env.h"
#include "dx_host.h"
#include "dx_files.h"

/* ==========================================================================================
 *  An image of any of the three kinds and the text it decodes to, for who wants the text's slices where they are made
 *  (dx_file_verify, dx_file_digest): the image's records walked, the header lines the decoder prints, the text's layout.
 *  image_text is in dx_files.h: dx_file_compare.c opens two of them.
 * ========================================================================================== */
void dxf_image_close(image_text *im)
{ dx_file_undexqv_plan_free(im->plan);
  dxf_u2_index_free(&im->ux);
  if (im->kind != DX_KIND_QUIVA) free(im->ooff);
  memset(im, 0, sizeof(*im));
}

int dxf_image_open(dx_ctx *ctx, int kind, int upper, uint32_t width, const uint8_t *img, size_t n, image_text *im)
{ hdr_patch *h = &im->h;
  int rc;
  memset(im, 0, sizeof(*im));
  im->kind = kind; im->upper = upper; im->width = width; im->img = img; im->n = n;
  if (kind == DX_KIND_QUIVA)
    { if ((rc = dx_file_undexqv_plan_on(ctx, img, n, &im->plan, &h->total)) != DX_OK) return rc;
      h->n = im->plan->x.n; im->ooff = im->plan->ooff; h->hat = im->plan->hat; h->hd = im->plan->hd.p; im->hd_len = im->plan->hd.len;
    }
  else
    { im->mode = kind == DX_KIND_ARROW ? DX_LETTERS_ARROW : (upper ? DX_LETTERS_UPPER : DX_LETTERS_LOWER);
      if ((rc = dxf_u2_walk(im->mode, img, n, NULL, &im->ux)) != DX_OK) return rc;
      h->n = im->ux.cnt;
      if ((im->ooff = malloc((h->n + 1) * sizeof(*im->ooff))) == NULL) return DX_E_NOMEM;
      h->total = dxf_u2_layout(&im->ux, width, im->ooff);
      im->ooff[h->n] = h->total;
      h->hat = im->ux.hat; h->hd = im->ux.hd.p; im->hd_len = im->ux.hd.len;
    }
  h->ooff = im->ooff;
  return DX_OK;
}

/* the text in slices of at most `cap` bytes (0: in one), each to `fn`; whole_in: quiva's image goes up whole (dxf_undexqv_sliced) */
static int image_slices(dx_ctx *ctx, const image_text *im, size_t cap, int whole_in, slice_fn fn, void *arg)
{ if (im->kind == DX_KIND_QUIVA) return dxf_undexqv_sliced(ctx, im->plan, im->upper, fn, arg, cap, whole_in);
  return dxf_unpack2_slices(ctx, im->mode, im->img, im->n, im->width, &im->ux, &im->h, cap, fn, arg);
}

int dxf_image_range(dx_ctx *ctx, const image_text *im, uint64_t r0, uint64_t r1, int whole_in, slice_fn fn, void *arg)
{ if (im->kind != DX_KIND_QUIVA) return DX_E_ARG;
  return dxf_undexqv_range(ctx, im->plan, im->upper, r0, r1, fn, arg, 0, whole_in);
}

/* ==========================================================================================
 *  round-trip check (dx_file_verify): the tools remove their source (dexta.c:205), and nothing ever asked whether the image
 *  gives it back -- SURVEY.md 8(c) lists when it does not.  The text is indexed and the image walked as the drivers above do
 *  it, the image decoded by their kernels slice by slice, and every slice compared with its part of the text where it lies:
 *  on the device (dx_verify_ranges).  Only the verdict comes back.
 * ========================================================================================== */
/* one side of the comparison, record by record: where the record's header line and body begin in the host text and how long the
   body is.  The text side reads them off its index, the image side off the decoder's layout. */
typedef struct
  { dx_ctx           *ctx;
    dx_verify_report *rep;
    int               kind, lossy, failed;         /* failed: the device said no to a slice (an error, not a verdict) */
    const uint8_t    *text;
    size_t            n;
    uint64_t          cnt;                         /* the text's records */
    const uint64_t   *off;                         /* ... where each one's body begins */
    const uint32_t   *blen;                        /* fasta / arrow: its bytes (tlen); quiva: symbols a line (len) */
    const uint64_t   *ooff, *hat;                  /* the decoded text's layout (hdr_patch) */
    uint64_t          upto;                        /* records [0, upto) have bodies to compare: both sides have them, and no header before differs */
    uint64_t          hit, hit_pos;                /* the first record whose bodies differ (UINT64_MAX: none), and where */
    void             *d_src, *d_arr;               /* device: a slice of the text; its unit arrays */
    size_t            src_cap, arr_cap;
  } verify_job;

static uint64_t vj_body_bytes(const verify_job *v, uint64_t i)
{ uint64_t b = v->kind == DX_KIND_QUIVA ? 5 * ((uint64_t) v->blen[i] + 1) : v->blen[i];
  return v->off[i] + b > v->n ? v->n - v->off[i] : b;    /* (a .quiva whose last line has no newline) */
}
static uint64_t vj_head_at(const verify_job *v, uint64_t i)
{ return i ? v->off[i - 1] + vj_body_bytes(v, i - 1) : 0; }
/* the decoded body of record i: from ooff[i] to the next record's header line (ooff[records_img]: the decoded text's end) */
static uint64_t vj_dec_bytes(const verify_job *v, uint64_t i)
{ return (i + 1 < v->rep->records_img ? v->ooff[i + 1] - (v->hat[i + 2] - v->hat[i + 1]) : v->ooff[i + 1]) - v->ooff[i]; }

/* a slice of decoded text, records [i0, i1), against the same records of the text */
static int verify_slice(void *arg, const void *d_out, uint64_t i0, uint64_t i1, size_t t0, size_t bytes)
{ verify_job *v = arg;
  const uint64_t e1 = i1 < v->upto ? i1 : v->upto, m = e1 > i0 ? e1 - i0 : 0;
  uint64_t  s0, s1, k, unit = UINT64_MAX, *a_off, *b_off;
  uint32_t *a_len, *b_len, *q_len, pos = 0;
  uint8_t  *h = NULL;
  int       rc = DX_OK;
  (void) bytes;
  if (m == 0) return SLICE_STOP;
  s0 = v->off[i0]; s1 = v->off[e1 - 1] + vj_body_bytes(v, e1 - 1);
  if ((rc = dgrow(v->ctx, &v->d_src, &v->src_cap, (size_t) (s1 - s0) + 64)) != DX_OK) goto bad;
  if ((rc = dgrow(v->ctx, &v->d_arr, &v->arr_cap, (size_t) m * 28 + 64)) != DX_OK) goto bad;
  h = malloc((size_t) m * 28 + 64);                        /* a_off, b_off (8 each), a_len, b_len, the lines' symbols (4 each) */
  if (h == NULL) { rc = DX_E_NOMEM; goto bad; }
  a_off = (uint64_t *) h; b_off = a_off + m; a_len = (uint32_t *) (b_off + m); b_len = a_len + m; q_len = b_len + m;
  for (k = 0; k < m; k++)
    { const uint64_t i = i0 + k;
      a_off[k] = v->off[i] - s0;
      a_len[k] = (uint32_t) vj_body_bytes(v, i);
      b_off[k] = v->ooff[i] - t0;
      b_len[k] = (uint32_t) vj_dec_bytes(v, i);
      q_len[k] = v->blen[i];
    }
  if ((rc = dx_h2d(v->ctx, v->d_src, v->text + s0, (size_t) (s1 - s0))) != DX_OK) goto bad;
  if ((rc = dx_h2d(v->ctx, v->d_arr, h, (size_t) m * 28)) != DX_OK) goto bad;
  { const uint64_t *da_off = v->d_arr, *db_off = da_off + m;
    const uint32_t *da_len = (const uint32_t *) (db_off + m), *db_len = da_len + m, *dq_len = db_len + m;
    if (v->lossy && v->kind == DX_KIND_QUIVA)              /* what dexqv -l keeps of the text (QV.c:1355-1372) */
      { const dx_qv_batch b = dxf_qv_batch(v->d_src, da_off, dq_len, m, s1 - s0, 1);
        if ((rc = dx_qv_lossy_text(v->ctx, &b)) != DX_OK) goto bad;
      }
    rc = dx_verify_ranges(v->ctx, v->d_src, da_off, da_len, d_out, db_off, db_len, m, &unit, &pos, NULL);
    if (rc != DX_OK) goto bad;
  }
  free(h);
  if (unit != UINT64_MAX)
    { v->hit = i0 + unit; v->hit_pos = pos;
      return SLICE_STOP;
    }
  return e1 == v->upto ? SLICE_STOP : DX_OK;
bad:
  free(h);
  v->failed = 1;
  return rc;
}

/* how much decoded text a slice may have: the slice, its part of the text and the image are on the device together.  0: all at once */
static size_t verify_cap(dx_ctx *ctx, size_t resident, size_t total, uint64_t units)
{ uint64_t fr = 0, all = 0;
  size_t   cap;
  if (dxf_budget_env(2 * total, 131072u, &cap)) return cap / 2;
  if (dx_mem_info(ctx, &fr, &all) != DX_OK || fr == 0) return 0;
  if ((double) resident + 2.0 * (double) total + 80.0 * (double) units <= 0.9 * (double) fr) return 0;
  { const double room = (0.9 * (double) fr - (double) resident - 80.0 * (double) units) / 2.0;
    return room > (double) ((size_t) 4 << 20) ? (size_t) room : (size_t) 4 << 20;
  }
}

/* record r's place in the report: byte `pos` of its body in the text (line, column), or of its header line (body == 0) */
static void verify_place(const verify_job *v, uint64_t r, int body, uint64_t pos)
{ dx_verify_report *rep = v->rep;
  const uint64_t at = body ? v->off[r] : vj_head_at(v, r), lim = body ? vj_body_bytes(v, r) : v->off[r] - at;
  uint64_t k, line = body ? 1 : 0, col = 0;
  if (pos > lim) pos = lim;
  for (k = 0; k < pos; k++)
    if (v->text[at + k] == '\n') { line += 1; col = 0; } else col += 1;
  rep->record = r; rep->line = line; rep->column = col; rep->src_byte = at + pos;
}

/* The options that give an indexed text back (dexgpu.h: dx_file_verify, dx_file_text_options): the case of its letters, its line width
   (quiva: 0).  sx: the index of a .fasta / .arrow, qx: of a .quiva. */
static void text_options(int kind, const uint8_t *text, const seq_index *sx, const quiva_index *qx, int32_t *upper, uint32_t *width)
{ uint64_t i;
  *upper = 0; *width = 0;
  if (kind == DX_KIND_QUIVA)
    { for (i = 0; i < qx->cnt; i++)                       /* undexqv -U: the deletion tags' case (undexqv.c:198-204) */
        if (qx->len[i] > 0)
          { const uint8_t c = text[qx->off[i] + qx->len[i] + 1];
            *upper = c >= 'A' && c <= 'Z';
            break;
          }
    }
  else
    { uint32_t longest = 0;
      for (i = 0; i < sx->cnt && kind == DX_KIND_FASTA; i++)
        if (sx->nsym[i] > 0)
          { const uint8_t *q = text + sx->off[i];
            while (*q == '\n') q++;
            *upper = *q >= 'A' && *q <= 'Z';
            break;
          }
      for (i = 0; i < sx->cnt && *width == 0; i++)         /* -w: the first line that another line of its record follows */
        { const uint8_t *q = text + sx->off[i], *e = sx->tlen[i] ? memchr(q, '\n', sx->tlen[i]) : NULL;
          if (e != NULL && (size_t) (e - q) + 1 < sx->tlen[i] && e > q) *width = (uint32_t) (e - q);
          if (sx->nsym[i] > longest) longest = sx->nsym[i];
        }
      if (*width == 0) *width = longest ? longest : 1;
    }
}

int dx_file_text_options(int kind, const uint8_t *text, size_t n, int *upper, uint32_t *width)
{ seq_index   sx;
  quiva_index qx = { 0, NULL, NULL, NULL, 0 };
  uint64_t    el = 0;
  int32_t     up = 0;
  int         rc, ec = 0;
  if (upper == NULL || width == NULL || (text == NULL && n)) return DX_E_ARG;
  if (kind != DX_KIND_FASTA && kind != DX_KIND_ARROW && kind != DX_KIND_QUIVA) return DX_E_ARG;
  memset(&sx, 0, sizeof(sx));
  rc = kind == DX_KIND_QUIVA ? dxf_quiva_index_host(&qx, text, n, &el, &ec) : dxf_seq_index_host(&sx, kind == DX_KIND_ARROW, text, n, &el, &ec);
  if (rc == DX_OK)
    { text_options(kind, text, &sx, &qx, &up, width);
      *upper = up;
    }
  dxf_seq_index_free(&sx); dxf_quiva_index_free(&qx);
  return rc;
}

int dx_file_verify(dx_ctx *ctx, int kind, const uint8_t *text, size_t n, const uint8_t *img, size_t m, int lossy, dx_verify_report *rep)
{ seq_index        sx;
  quiva_index      qx = { 0, NULL, NULL, NULL, 0 };
  image_text       im;
  verify_job       v;
  uint64_t         el = 0, both, hfirst;
  const uint64_t  *hat;
  const char      *hd;
  int              rc, ec = 0;

  if (ctx == NULL || rep == NULL || (text == NULL && n) || (img == NULL && m)) return DX_E_ARG;
  if (kind != DX_KIND_FASTA && kind != DX_KIND_ARROW && kind != DX_KIND_QUIVA) return DX_E_ARG;
  memset(rep, 0, sizeof(*rep));
  memset(&sx, 0, sizeof(sx)); memset(&im, 0, sizeof(im)); memset(&v, 0, sizeof(v));
  v.ctx = ctx; v.rep = rep; v.kind = kind; v.lossy = lossy; v.text = text; v.n = n; v.hit = UINT64_MAX;

  /* the text: its records, and the options that would give it back */
  if (kind == DX_KIND_QUIVA)
    { TRY(dxf_quiva_index_host(&qx, text, n, &el, &ec));
      v.cnt = qx.cnt; v.off = qx.off; v.blen = qx.len;
    }
  else
    { TRY(dxf_seq_index_host(&sx, kind == DX_KIND_ARROW, text, n, &el, &ec));
      v.cnt = sx.cnt; v.off = sx.off; v.blen = sx.tlen;
    }
  text_options(kind, text, &sx, &qx, &rep->upper, &rep->width);
  rep->records_src = v.cnt;

  /* the image, decoded with those options */
  rc = m ? dxf_image_open(ctx, kind, rep->upper, rep->width, img, m, &im) : DX_E_FORMAT;
  if (rc == DX_E_FORMAT || rc == DX_E_UNSUPPORTED || rc == DX_E_DEGENERATE)
    { rep->where = DX_VERIFY_IMAGE;                        /* (no image of anything) */
      rc = DX_OK; goto done;
    }
  if (rc != DX_OK) goto done;
  rep->records_img = im.h.n; v.ooff = im.h.ooff; v.hat = hat = im.h.hat; hd = im.h.hd;

  /* header lines, here: the first record whose line is not the decoder's (O(records)) */
  both = v.cnt < rep->records_img ? v.cnt : rep->records_img;
  for (hfirst = 0; hfirst < both; hfirst++)
    { const uint64_t at = vj_head_at(&v, hfirst), hl = v.off[hfirst] - at;
      if (hl != hat[hfirst + 1] - hat[hfirst] || memcmp(text + at, hd + hat[hfirst], (size_t) hl) != 0) break;
    }

  /* bodies, there: of the records in front of that one */
  v.upto = hfirst;
  if (v.upto > 0)
    { const size_t cap = verify_cap(ctx, kind == DX_KIND_QUIVA && PLAN_HAS_IMAGE(im.plan) ? 0 : m, im.h.total, both);
      rc = image_slices(ctx, &im, cap, 1, verify_slice, &v);
      if (rc != DX_OK && !v.failed && (rc == DX_E_FORMAT || rc == DX_E_MISMATCH || rc == DX_E_UNSUPPORTED))
        { rep->where = DX_VERIFY_IMAGE;                    /* the decoder turned the records down */
          rc = DX_OK; goto done;
        }
      if (rc != DX_OK) goto done;
    }

  if (v.hit != UINT64_MAX)                                /* a body: a byte, or one side's end */
    { const uint64_t al = vj_body_bytes(&v, v.hit);
      const uint64_t bl = vj_dec_bytes(&v, v.hit);
      rep->where = v.hit_pos < al && v.hit_pos < bl ? DX_VERIFY_BODY : DX_VERIFY_LENGTH;
      verify_place(&v, v.hit, 1, v.hit_pos);
    }
  else if (hfirst < both)
    { uint64_t at = vj_head_at(&v, hfirst), hl = v.off[hfirst] - at, dl = hat[hfirst + 1] - hat[hfirst], k = 0;
      while (k < hl && k < dl && text[at + k] == (uint8_t) hd[hat[hfirst] + k]) k++;
      rep->where = DX_VERIFY_HEADER;
      verify_place(&v, hfirst, 0, k);
    }
  else if (v.cnt != rep->records_img)
    { rep->where = DX_VERIFY_COUNT;
      rep->record = both;
      rep->src_byte = both < v.cnt ? vj_head_at(&v, both) : n;
    }
  else
    rep->ok = 1;

  if (!rep->ok && rep->record < rep->records_img)          /* where that record stands in the image */
    { if (kind != DX_KIND_QUIVA)
        { uint64_t sym = 0, k;
          for (k = v.off[rep->record]; rep->where == DX_VERIFY_BODY && k < rep->src_byte; k++) sym += text[k] != '\n';
          rep->img_byte = im.ux.ioff[rep->record] + sym / 4;
        }
      else if (PLAN_HAS_INDEX(im.plan))
        TRY(dx_d2h(ctx, &rep->img_byte, im.plan->dix.d_rec_off + rep->record, 8));
      else
        rep->img_byte = im.plan->x.rec_off[rep->record];
    }
  rc = DX_OK;

done:
  if (v.d_src) (void) dx_free(ctx, v.d_src);
  if (v.d_arr) (void) dx_free(ctx, v.d_arr);
  dxf_image_close(&im);
  dxf_seq_index_free(&sx); dxf_quiva_index_free(&qx);
  return rc;
}

/* ==========================================================================================
 *  digest (dx_file_digest): the CRC-32 of the text an image decodes to, for the day the text is gone.  The image is walked and
 *  decoded as the drivers above do it, slice by slice; a slice of decoded bodies stays where it is made and is hashed there
 *  (dx_crc32_ranges), and so are the header lines, which the host prints and uploads once.  Per slice the device joins a record's
 *  two (crc, length) pairs and folds the records' (dx_crc32_fold); the host joins the slices.  Nothing of the text comes back.
 * ========================================================================================== */
typedef struct
  { dx_ctx          *ctx;
    const hdr_patch *h;                            /* the decoded text's layout */
    void            *d_hd;    size_t hd_bytes;     /* device: the header lines, one after the other */
    void            *d_arr;   size_t arr_cap;      /* ... a slice's unit arrays */
    uint32_t         crc;     uint64_t bytes;      /* of the slices so far */
    uint32_t        *rec;                          /* every record's CRC, when wanted */
  } digest_job;

/* a slice of decoded text, records [i0, i1): per record two units, its header line (in d_hd) and its body (in d_out) */
static int digest_slice(void *arg, const void *d_out, uint64_t i0, uint64_t i1, size_t t0, size_t bytes)
{ digest_job *g = arg;
  const hdr_patch *h = g->h;
  const uint64_t m = i1 - i0;
  uint64_t *off, *len, k, sbytes = 0;
  uint32_t  scrc = 0;
  int       rc;
  if ((rc = dgrow(g->ctx, &g->d_arr, &g->arr_cap, (size_t) m * 52 + 64)) != DX_OK) return rc;
  off = malloc((size_t) m * 32 + 64);                      /* off, len: 2 m each, a record's header line, then its body */
  if (off == NULL) return DX_E_NOMEM;
  len = off + 2 * m;
  for (k = 0; k < m; k++)
    { const uint64_t i = i0 + k;
      off[2*k]     = h->hat[i];
      len[2*k]     = h->hat[i + 1] - h->hat[i];
      off[2*k + 1] = h->ooff[i] - t0;
      len[2*k + 1] = text_at(h, i + 1) - h->ooff[i];
    }
  rc = dx_h2d(g->ctx, g->d_arr, off, (size_t) m * 32);
  free(off);
  if (rc != DX_OK) return rc;
  { uint64_t *d_off = g->d_arr, *d_len = d_off + 2 * m, *d_rlen = d_len + 2 * m;
    uint32_t *d_crc = (uint32_t *) (d_rlen + m), *d_rcrc = d_crc + 2 * m;
    if ((rc = dx_crc32_ranges_strided(g->ctx, g->d_hd, g->hd_bytes, d_off, d_len, m, 2, d_crc, NULL)) != DX_OK) return rc;
    if ((rc = dx_crc32_ranges_strided(g->ctx, d_out, bytes, d_off + 1, d_len + 1, m, 2, d_crc + 1, NULL)) != DX_OK) return rc;
    if ((rc = dx_crc32_pairs(g->ctx, d_crc, d_len, m, d_rcrc, d_rlen)) != DX_OK) return rc;
    if ((rc = dx_crc32_fold(g->ctx, d_rcrc, d_rlen, m, &scrc, &sbytes)) != DX_OK) return rc;
    if (g->rec != NULL && (rc = dx_d2h(g->ctx, g->rec + i0, d_rcrc, (size_t) m * 4)) != DX_OK) return rc;
  }
  g->crc    = dx_crc32_combine(g->crc, scrc, sbytes);
  g->bytes += sbytes;
  return DX_OK;
}

int dx_file_digest(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, int upper, uint32_t width, dx_digest *out, uint32_t **rec_crc)
{ image_text im;
  digest_job g;
  uint64_t   cnt;
  int        rc;

  if (ctx == NULL || img == NULL || out == NULL) return DX_E_ARG;
  if (kind != DX_KIND_FASTA && kind != DX_KIND_ARROW && kind != DX_KIND_QUIVA) return DX_E_ARG;
  if (kind != DX_KIND_QUIVA && width == 0) return DX_E_ARG;
  if (rec_crc) *rec_crc = NULL;
  memset(&g, 0, sizeof(g));
  g.ctx = ctx; g.h = &im.h;

  TRY(dxf_image_open(ctx, kind, upper, width, img, m, &im));
  cnt = im.h.n; g.hd_bytes = im.hd_len;
  if (rec_crc != NULL && (g.rec = malloc((cnt + 1) * sizeof(*g.rec))) == NULL) { rc = DX_E_NOMEM; goto done; }

  if (cnt > 0)
    { int whole_in = 1;
      const size_t cap = kind == DX_KIND_QUIVA ? dxf_undexqv_cap(ctx, im.plan, &whole_in) : dxf_out_cap(ctx, m, im.h.total, cnt);
      TRY(dx_malloc(ctx, g.hd_bytes + 64, &g.d_hd));
      TRY(dx_h2d(ctx, g.d_hd, im.h.hd, g.hd_bytes));
      TRY(image_slices(ctx, &im, cap, whole_in, digest_slice, &g));
      if (g.bytes != im.h.total) { rc = DX_E_MISMATCH; goto done; }     /* (the slices are the whole text) */
    }
  out->crc32 = g.crc; out->reserved = 0; out->bytes = g.bytes; out->records = cnt;
  if (rec_crc) { *rec_crc = g.rec; g.rec = NULL; }
  rc = DX_OK;

done:
  if (g.d_hd) (void) dx_free(ctx, g.d_hd);
  if (g.d_arr) (void) dx_free(ctx, g.d_arr);
  dxf_image_close(&im);
  free(g.rec);
  return rc;
}

/* ==========================================================================================
 *  census (dx_file_census): what an image holds -- records, symbols, the shortest and the longest read, N50, the composition of the
 *  2-bit kinds, the distribution of a .quiva's five lines -- for the day the text is gone.  dex2DB.c:587-595 / 793-797 count
 *  the same on one core as reads enter a database (DAZZ_DB.freq, totlen, maxlen: 896-913).  A .dexta / .dexar image is walked and
 *  uploaded slice by slice (dxf_u2_slices, dx_file_u2.c), and its packed reads are counted where they lie (dx_code_counts): no text
 *  is made.  A .dexqv image is planned and decoded as the digest does it, and a slice hook counts every entry's five lines where they
 *  are made (dx_byte_hist_ranges).
 * ========================================================================================== */
/* Two counting passes, the first over the lengths' high halves (how many, and their sum), the second over the low halves of the
   lengths in the bucket in which the running sum, from the longest down, reaches half of the total. */
int dx_census_lengths(const uint32_t *len, uint64_t n, dx_census *out)
{ uint64_t *sumh, *cntl, total = 0, run = 0, i;
  uint32_t  lo = UINT32_MAX, hi = 0, n50 = 0;
  int       h, l;
  if (out == NULL || (len == NULL && n)) return DX_E_ARG;
  if ((sumh = calloc(2 * 65536, sizeof(*sumh))) == NULL) return DX_E_NOMEM;
  cntl = sumh + 65536;
  for (i = 0; i < n; i++)
    { const uint32_t v = len[i];
      sumh[v >> 16] += v; total += v;
      if (v < lo) lo = v;
      if (v > hi) hi = v;
    }
  if (total > 0)
    { for (h = 65535; h > 0 && run + sumh[h] < total - (run + sumh[h]); h--) run += sumh[h];      /* (2 running >= total, without the doubling) */
      for (i = 0; i < n; i++)
        if ((len[i] >> 16) == (uint32_t) h) cntl[len[i] & 0xffffu] += 1;
      for (l = 65535; l >= 0; l--)                        /* the reads of one length together: the sum reaches half with one of them or with none */
        { const uint64_t v = ((uint64_t) h << 16) | (uint64_t) l;
          run += cntl[l] * v;
          if (cntl[l] != 0 && run >= total - run) { n50 = (uint32_t) v; break; }
        }
    }
  free(sumh);
  out->records = n; out->symbols = total;
  out->min_len = n ? lo : 0; out->max_len = hi; out->n50 = n50; out->reserved = 0;
  return DX_OK;
}

/* a slice of a walked image's packed reads (dxf_u2_slices, 16 bytes a record of its own): code[4] added to and, when wanted, every
   record's four counts */
typedef struct { dx_ctx *ctx; uint64_t *code; uint32_t *rec; } census2_job;

static int census_pack2_slice(void *arg, const u2_slice *s)
{ census2_job *c = arg;
  uint32_t *d_cnt = s->d_extra;
  uint64_t  tot[4];
  int       rc, q;
  if ((rc = dx_code_counts(c->ctx, s->d_in, s->bytes, s->d_boff, NULL, s->d_len, s->n, c->rec ? d_cnt : NULL, tot, NULL)) != DX_OK) return rc;
  if (c->rec != NULL && (rc = dx_d2h(c->ctx, c->rec + 4 * s->i0, d_cnt, (size_t) s->n * 16)) != DX_OK) return rc;
  for (q = 0; q < 4; q++) c->code[q] += tot[q];
  return DX_OK;
}

typedef struct
  { dx_ctx          *ctx;
    const hdr_patch *h;                            /* the decoded text's layout */
    const uint32_t  *len;                          /* every entry's symbols a line */
    void            *d_arr;   size_t arr_cap;      /* device: a slice's unit arrays */
    uint64_t       (*hist)[256];                   /* five tables, of the slices so far */
    uint64_t        *rec;                          /* every record's five sums, when wanted */
  } census_job;

/* a slice of decoded text, entries [i0, i1): per entry five ranges, its lines without their newlines, kinds 0 .. 4 */
static int census_slice(void *arg, const void *d_out, uint64_t i0, uint64_t i1, size_t t0, size_t bytes)
{ census_job *c = arg;
  const uint64_t m = i1 - i0;
  uint64_t *off, *ln, k, hs[5][256];
  uint8_t  *kd;
  int       rc, q;
  if ((rc = dgrow(c->ctx, &c->d_arr, &c->arr_cap, (size_t) m * 125 + 64)) != DX_OK) return rc;       /* off, len, sum (40 each), kind (5) */
  if ((off = malloc((size_t) m * 85 + 64)) == NULL) return DX_E_NOMEM;
  ln = off + 5 * m; kd = (uint8_t *) (ln + 5 * m);
  for (k = 0; k < m; k++)
    for (q = 0; q < 5; q++)
      { off[5*k + q] = c->h->ooff[i0 + k] - t0 + (uint64_t) q * ((uint64_t) c->len[i0 + k] + 1);
        ln[5*k + q]  = c->len[i0 + k];
        kd[5*k + q]  = (uint8_t) q;
      }
  { uint64_t *d_off = c->d_arr, *d_len = d_off + 5 * m, *d_sum = d_len + 5 * m;
    uint8_t  *d_kind = (uint8_t *) (d_sum + 5 * m);
    rc = dx_h2d(c->ctx, d_off, off, (size_t) m * 80);
    if (rc == DX_OK) rc = dx_h2d(c->ctx, d_kind, kd, (size_t) m * 5);
    free(off);
    if (rc != DX_OK) return rc;
    if ((rc = dx_byte_hist_ranges(c->ctx, d_out, bytes, d_off, d_len, d_kind, 5, 5 * m, c->rec ? d_sum : NULL, &hs[0][0], NULL)) != DX_OK) return rc;
    if (c->rec != NULL && (rc = dx_d2h(c->ctx, c->rec + 5 * i0, d_sum, (size_t) m * 40)) != DX_OK) return rc;
  }
  for (q = 0; q < 5; q++)
    for (k = 0; k < 256; k++) c->hist[q][k] += hs[q][k];
  return DX_OK;
}

int dx_file_census(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, dx_census *out, uint32_t **rec_len, uint32_t **rec_code, uint64_t **rec_sum)
{ image_text  im;
  dx_census  *cs = NULL;
  uint32_t   *rl = NULL, *rcode = NULL;
  uint64_t   *rsum = NULL, cnt;
  const uint32_t *lens;
  int         rc;

  if (ctx == NULL || img == NULL || out == NULL) return DX_E_ARG;
  if (kind != DX_KIND_FASTA && kind != DX_KIND_ARROW && kind != DX_KIND_QUIVA) return DX_E_ARG;
  if (rec_len) *rec_len = NULL;
  if (rec_code) *rec_code = NULL;
  if (rec_sum) *rec_sum = NULL;

  TRY(dxf_image_open(ctx, kind, 0, 1, img, m, &im));      /* (the tag line in lower case; the line width lays out a text nobody makes) */
  cnt  = im.h.n;
  lens = kind == DX_KIND_QUIVA ? im.plan->x.len : im.ux.nsym;
  if ((cs = calloc(1, sizeof(*cs))) == NULL) { rc = DX_E_NOMEM; goto done; }
  TRY(dx_census_lengths(lens, cnt, cs));
  if (rec_len != NULL)
    { if ((rl = malloc((cnt + 1) * sizeof(*rl))) == NULL) { rc = DX_E_NOMEM; goto done; }
      if (cnt) memcpy(rl, lens, cnt * sizeof(*rl));
    }
  if (kind != DX_KIND_QUIVA)
    { if (rec_code != NULL && (rcode = malloc((cnt + 1) * 4 * sizeof(*rcode))) == NULL) { rc = DX_E_NOMEM; goto done; }
      if (cnt > 0)
        { census2_job c = { ctx, cs->code, rcode };
          TRY(dxf_u2_slices(ctx, img, &im.ux, dxf_u2_cap(ctx, m, cnt), 16, census_pack2_slice, &c));
        }
    }
  else
    { census_job c;
      memset(&c, 0, sizeof(c));
      c.ctx = ctx; c.h = &im.h; c.len = lens; c.hist = cs->hist;
      if (rec_sum != NULL && (rsum = malloc((cnt + 1) * 5 * sizeof(*rsum))) == NULL) { rc = DX_E_NOMEM; goto done; }
      c.rec = rsum;
      if (cnt > 0)
        { int whole_in = 1;
          const size_t cap = dxf_undexqv_cap(ctx, im.plan, &whole_in);
          rc = image_slices(ctx, &im, cap, whole_in, census_slice, &c);
        }
      if (c.d_arr) (void) dx_free(ctx, c.d_arr);
      if (rc != DX_OK) goto done;
    }
  *out = *cs;
  if (rec_len)  { *rec_len = rl; rl = NULL; }
  if (rec_code) { *rec_code = rcode; rcode = NULL; }
  if (rec_sum)  { *rec_sum = rsum; rsum = NULL; }
  rc = DX_OK;

done:
  dxf_image_close(&im);
  free(cs); free(rl); free(rcode); free(rsum);
  return rc;
}
