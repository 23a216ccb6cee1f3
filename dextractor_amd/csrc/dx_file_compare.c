/*
 * dx_file_compare.c -- how two .dexta / .dexar / .dexqv images of the same records differ, for the day both texts are gone: a lossless
 * .dexqv and the -l one dx_file_subset made of it, a legacy or byte-swapped archive and its rewrite, the reference's image and this
 * library's.  The digests say "equal" or "not equal"; this says what differs, where and by how much -- without the round trip through
 * two texts and a text diff.
 *
 *     host            both images walked (dxf_image_open: the drivers' own walks), records paired by index; counts, prefixes, the
 *                     headers' fields and the lengths compared here, O(records)                              [dxf_compare_open]
 *     fasta / arrow   both images up (or a slice's bytes of each), the packed reads compared where they lie: dx_code_diff.  No text.
 *     quiva           both images decoded by dxf_undexqv_range, each with its own coding, a's slice hook decoding the same records of b
 *                     so that both texts stand on the device together; the five lines of every record compared there: dx_diff_ranges,
 *                     kinds 0 .. 4, side a masked for lossy (QV.c:1406-1415).  Nothing of either text comes back.
 *
 * A pair is cut into slices of whole records, the SAME record range on both sides (dxf_compare_slice_end), when its two texts (2-bit
 * kinds: images) do not fit the device together or exceed DEXGPU_TEXT_BUDGET; the report is the same.
 */
#include <stdlib.h>
#include <string.h>

#include "dexgpu.h"
#include "dx_host.h"
#include "dx_files.h"

/* ==========================================================================================
 *  the host part: two walks paired (tools/compare_host_check.c runs it alone, under the sanitizers)
 * ========================================================================================== */
/* the prefix of a walked 2-bit image (the walk has seen to it that it is there): undexta.c:161-169 */
static void u2_prefix(const uint8_t *img, const char **name, size_t *plen)
{ uint16_t key;
  int32_t  n;
  memcpy(&key, img, 2); memcpy(&n, img + 2, 4);
  if (key == 0xaa55 || key == 0xcc33) n = (int32_t) flip32((uint32_t) n);
  *name = (const char *) img + 6; *plen = (size_t) n;
}

/* what the walk of one side knows of record i, whichever the kind */
static const int32_t *side_hdr4(const image_text *im) { return im->kind == DX_KIND_QUIVA ? im->plan->x.hdr4 : im->ux.hdr4; }
static const uint32_t *side_len(const image_text *im) { return im->kind == DX_KIND_QUIVA ? im->plan->x.len : im->ux.nsym; }

void dxf_compare_close(cmp_pair *p)
{ dxf_image_close(&p->a); dxf_image_close(&p->b);
  free(p->pa); free(p->pb);
  memset(p, 0, sizeof(*p));
}

/* p is zeroed.  Both images opened (*side: 'a' or 'b', the one that was being opened when an error came), the record counts, prefixes,
   headers and lengths compared into *c, and the slices' measure laid out: record i of a side costs p[i + 1] - p[i] -- bytes of text
   (quiva) or of image (the 2-bit kinds: from its packed read to the next record's).  An error leaves what there is to dxf_compare_close. */
int dxf_compare_open(dx_ctx *ctx, int kind, const uint8_t *img_a, size_t m_a, const uint8_t *img_b, size_t m_b, cmp_pair *p, dx_compare *c, int *side)
{ const int32_t  *ha, *hb;
  const uint32_t *la, *lb;
  const char     *na, *nb;
  size_t          pla, plb;
  uint64_t        i;
  int             rc;

  memset(c, 0, sizeof(*c));
  c->lines = kind == DX_KIND_QUIVA ? 5 : 1;
  c->first_header = c->first_length = c->first_record = UINT64_MAX;
  *side = 'a';
  (void) dx_side_fail(ctx, DX_OK, 0);
  if ((rc = m_a ? dxf_image_open(ctx, kind, 0, 1, img_a, m_a, &p->a) : DX_E_FORMAT) != DX_OK) return rc;
  *side = 'b';
  (void) dx_side_fail(ctx, DX_OK, 0);
  if ((rc = m_b ? dxf_image_open(ctx, kind, 0, 1, img_b, m_b, &p->b) : DX_E_FORMAT) != DX_OK) return rc;
  c->records_a = p->a.h.n; c->records_b = p->b.h.n;
  p->both = c->records_a < c->records_b ? c->records_a : c->records_b;

  if (kind == DX_KIND_QUIVA)
    { na = p->a.plan->x.prefix; pla = strlen(na); nb = p->b.plan->x.prefix; plb = strlen(nb); }
  else
    { u2_prefix(img_a, &na, &pla); u2_prefix(img_b, &nb, &plb); }
  c->prefix_differs = pla != plb || memcmp(na, nb, pla) != 0;

  ha = side_hdr4(&p->a); hb = side_hdr4(&p->b); la = side_len(&p->a); lb = side_len(&p->b);
  for (i = 0; i < p->both; i++)
    { int differs = memcmp(ha + 4 * i, hb + 4 * i, 4 * sizeof(*ha)) != 0;
      if (kind == DX_KIND_ARROW && memcmp(p->a.ux.cnr4 + 4 * i, p->b.ux.cnr4 + 4 * i, 4 * sizeof(uint16_t)) != 0) differs = 1;
      if (differs && c->headers_differ++ == 0) c->first_header = i;
      if (la[i] != lb[i] && c->lengths_differ++ == 0) c->first_length = i;
    }

  p->pa = malloc((p->both + 1) * sizeof(*p->pa)); p->pb = malloc((p->both + 1) * sizeof(*p->pb));
  if (p->pa == NULL || p->pb == NULL) return DX_E_NOMEM;
  for (i = 0; i <= p->both; i++)
    if (kind == DX_KIND_QUIVA) { p->pa[i] = text_at(&p->a.h, i); p->pb[i] = text_at(&p->b.h, i); }
    else if (i < p->both)      { p->pa[i] = p->a.ux.ioff[i]; p->pb[i] = p->b.ux.ioff[i]; }
    else                       { p->pa[i] = i ? dxf_u2_end(&p->a.ux, i - 1) : 0; p->pb[i] = i ? dxf_u2_end(&p->b.ux, i - 1) : 0; }
  return DX_OK;
}

/* a slice of whole records from i0 on, the same on both sides: as many as cost at most `cap` bytes on the two sides together, and one at
   least; cap 0: all that are left */
uint64_t dxf_compare_slice_end(const cmp_pair *p, uint64_t i0, size_t cap)
{ uint64_t i1 = i0 + 1;
  if (cap == 0 || i0 >= p->both) return p->both;
  while (i1 < p->both && (p->pa[i1 + 1] - p->pa[i0]) + (p->pb[i1 + 1] - p->pb[i0]) <= cap) i1++;
  return i1;
}

/* ==========================================================================================
 *  the device part
 * ========================================================================================== */
typedef struct
  { dx_ctx         *ctx;
    const cmp_pair *p;
    dx_compare     *c;
    uint32_t       *rec;                           /* both x lines: every compared record's differing symbols, line by line */
    const uint8_t  *a_and;                         /* quiva, lossy: the five lines' masks for side a */
    int             whole_in, side;                /* side: whose decode an error is ('a', 'b'; 0: neither's) */
    void           *d_arr;   size_t arr_cap;       /* device: a slice's unit arrays */
    uint64_t       *h_arr;   size_t h_cap;         /* ... and their host copy */
    const void     *d_a;     size_t t0_a, bytes_a; /* quiva: a's slice of text, while b's is made */
  } cmp_job;

/* a slice's counts are down in j->rec: the records that differ, and the call's first difference, `first` = unit << 32 | place */
static void slice_account(cmp_job *j, uint64_t i0, uint64_t m, uint64_t first)
{ dx_compare *c = j->c;
  const uint32_t lines = (uint32_t) c->lines;
  uint64_t k, q;
  for (k = 0; k < m; k++)
    for (q = 0; q < lines; q++)
      if (j->rec[(i0 + k) * lines + q] != 0) { c->records_differ += 1; break; }
  if (first != UINT64_MAX && c->first_record == UINT64_MAX)
    { c->first_record = i0 + (first >> 32) / lines;
      c->first_line   = (uint32_t) ((first >> 32) % lines);
      c->first_column = (uint32_t) first;
    }
}

static int job_room(cmp_job *j, size_t bytes)
{ int rc = dgrow(j->ctx, &j->d_arr, &j->arr_cap, bytes + 64);
  if (rc == DX_OK && bytes + 64 > j->h_cap)
    { free(j->h_arr);
      j->h_arr = malloc(bytes + 64); j->h_cap = j->h_arr ? bytes + 64 : 0;
      if (j->h_arr == NULL) rc = DX_E_NOMEM;
    }
  return rc;
}

/* ---- fasta / arrow: records [i0, i1) of both images up, their packed reads compared where they lie ---- */
static int compare_pack2(cmp_job *j, size_t cap)
{ const cmp_pair *p = j->p;
  const u2_index *xa = &p->a.ux, *xb = &p->b.ux;
  uint64_t  i, i0, i1, most = 0;
  size_t    amax = 0, bmax = 0, a_cap = 0, b_cap = 0;
  void     *d_a = NULL, *d_b = NULL;
  int       rc = DX_OK;
  for (i0 = 0; i0 < p->both; i0 = i1)                     /* the largest slice: one allocation serves them all */
    { i1 = dxf_compare_slice_end(p, i0, cap);
      if (dxf_u2_end(xa, i1 - 1) - xa->ioff[i0] > amax) amax = (size_t) (dxf_u2_end(xa, i1 - 1) - xa->ioff[i0]);
      if (dxf_u2_end(xb, i1 - 1) - xb->ioff[i0] > bmax) bmax = (size_t) (dxf_u2_end(xb, i1 - 1) - xb->ioff[i0]);
      if (i1 - i0 > most) most = i1 - i0;
    }
  TRY(dgrow(j->ctx, &d_a, &a_cap, amax + 64));
  TRY(dgrow(j->ctx, &d_b, &b_cap, bmax + 64));
  TRY(job_room(j, (size_t) most * 24));                   /* offsets (8, 8), symbols (4), counts (4) */
  for (i0 = 0; i0 < p->both; i0 = i1)
    { const uint64_t a0 = xa->ioff[i0], b0 = xb->ioff[i0];
      uint64_t *aoff = j->h_arr, *boff, m, tot[2], first;
      uint32_t *len;
      i1 = dxf_compare_slice_end(p, i0, cap); m = i1 - i0;
      boff = aoff + m; len = (uint32_t *) (boff + m);
      for (i = i0; i < i1; i++)
        { aoff[i - i0] = xa->ioff[i] - a0; boff[i - i0] = xb->ioff[i] - b0;
          len[i - i0]  = xa->nsym[i] < xb->nsym[i] ? xa->nsym[i] : xb->nsym[i];
        }
      TRY(dx_h2d(j->ctx, d_a, p->a.img + a0, (size_t) (dxf_u2_end(xa, i1 - 1) - a0)));
      TRY(dx_h2d(j->ctx, d_b, p->b.img + b0, (size_t) (dxf_u2_end(xb, i1 - 1) - b0)));
      TRY(dx_h2d(j->ctx, j->d_arr, j->h_arr, (size_t) m * 20));
      { const uint64_t *da_off = j->d_arr, *db_off = da_off + m;
        const uint32_t *d_len = (const uint32_t *) (db_off + m);
        uint32_t *d_differ = (uint32_t *) d_len + m;
        TRY(dx_code_diff(j->ctx, d_a, dxf_u2_end(xa, i1 - 1) - a0, da_off, d_b, dxf_u2_end(xb, i1 - 1) - b0, db_off, d_len, m, d_differ, NULL,
                         tot, &first, NULL));
        TRY(dx_d2h(j->ctx, j->rec + i0, d_differ, (size_t) m * 4));
      }
      j->c->differ[0] += tot[0]; j->c->line_records[0] += tot[1];
      slice_account(j, i0, m, first);
    }
done:
  if (d_a) (void) dx_free(j->ctx, d_a);
  if (d_b) (void) dx_free(j->ctx, d_b);
  return rc;
}

/* ---- quiva: b's slice of text is made while a's stands; the records' five lines, without their newlines, are the units ---- */
static int compare_qv_b(void *arg, const void *d_out, uint64_t i0, uint64_t i1, size_t t0, size_t bytes)
{ cmp_job *j = arg;
  const cmp_pair *p = j->p;
  const uint32_t *la = side_len(&p->a), *lb = side_len(&p->b);
  const uint64_t  m = i1 - i0;
  uint64_t *aoff, *boff, k, first;
  uint32_t *len;
  uint8_t  *kd;
  dx_diff_tally t[5];
  int       rc, q;
  j->side = 0;                                            /* (both texts are made: what fails here is neither image's) */
  if ((rc = job_room(j, (size_t) m * 5 * 25)) != DX_OK) return rc;     /* offsets (8, 8), symbols (4), kind (1), counts (4) a line */
  aoff = j->h_arr; boff = aoff + 5 * m; len = (uint32_t *) (boff + 5 * m); kd = (uint8_t *) (len + 5 * m);
  for (k = 0; k < m; k++)
    for (q = 0; q < 5; q++)
      { const uint64_t i = i0 + k;
        aoff[5*k + q] = p->a.h.ooff[i] - j->t0_a + (uint64_t) q * ((uint64_t) la[i] + 1);
        boff[5*k + q] = p->b.h.ooff[i] - t0 + (uint64_t) q * ((uint64_t) lb[i] + 1);
        len[5*k + q]  = la[i] < lb[i] ? la[i] : lb[i];
        kd[5*k + q]   = (uint8_t) q;
      }
  if ((rc = dx_h2d(j->ctx, j->d_arr, j->h_arr, (size_t) m * 5 * 21)) != DX_OK) return rc;
  { const uint64_t *da_off = j->d_arr, *db_off = da_off + 5 * m;
    const uint32_t *d_len = (const uint32_t *) (db_off + 5 * m);
    const uint8_t  *d_kind = (const uint8_t *) (d_len + 5 * m);
    uint32_t *d_differ = (uint32_t *) ((uint8_t *) j->d_arr + (((size_t) m * 5 * 21 + 3) & ~(size_t) 3));
    if ((rc = dx_diff_ranges(j->ctx, j->d_a, j->bytes_a, da_off, d_out, bytes, db_off, d_len, d_kind, 5, j->a_and, 5 * m, d_differ, NULL,
                             t, &first, NULL)) != DX_OK) return rc;
    if ((rc = dx_d2h(j->ctx, j->rec + 5 * i0, d_differ, (size_t) m * 20)) != DX_OK) return rc;
  }
  for (q = 0; q < 5; q++)
    { dx_compare *c = j->c;
      c->differ[q] += t[q].differ; c->line_records[q] += t[q].units; c->sum_abs[q] += t[q].sum_abs;
      if (t[q].max_abs > c->max_abs[q]) c->max_abs[q] = t[q].max_abs;
    }
  slice_account(j, i0, m, first);
  j->side = 'a';                                          /* (b's part of this slice is done: what fails from here on is a's) */
  return DX_OK;
}

static int compare_qv_a(void *arg, const void *d_out, uint64_t i0, uint64_t i1, size_t t0, size_t bytes)
{ cmp_job *j = arg;
  int rc;
  j->d_a = d_out; j->t0_a = t0; j->bytes_a = bytes;
  if ((rc = dx_sync(j->ctx)) != DX_OK) return rc;          /* (a's text is made before b's coding takes the context's tables) */
  j->side = 'b';
  return dxf_image_range(j->ctx, &j->p->b, i0, i1, j->whole_in, compare_qv_b, j);
}

/* How much of the two texts the device takes at once (0: all of both, the images whole beside them).  A pair in slices sends a slice's
   records of each image with the slice (*whole_in 0; an image the plan has put on the device stays there): every slice is a decode of
   its own on either side, and the whole images would travel once a slice. */
static size_t compare_qv_cap(dx_ctx *ctx, const cmp_pair *p, int *whole_in)
{ const dx_undexqv_plan *a = p->a.plan, *b = p->b.plan;
  const double in = (PLAN_HAS_IMAGE(a) ? 0.0 : (double) a->n) + (PLAN_HAS_IMAGE(b) ? 0.0 : (double) b->n);
  const double text = (double) p->pa[p->both] + (double) p->pb[p->both], arrays = 96.0 * (double) (a->x.n + b->x.n) + 125.0 * (double) p->both;
  uint64_t fr = 0, all = 0;
  size_t   cap = 0;
  if (!dxf_budget_env((size_t) (p->pa[p->both] + p->pb[p->both]), 131072u, &cap) &&
      dx_mem_info(ctx, &fr, &all) == DX_OK && fr > 0 && in + text + arrays > 0.9 * (double) fr)
    { cap = (size_t) ((0.9 * (double) fr - arrays) / 1.4);    /* (a slice's records are about 0.3 of its text) */
      if (0.9 * (double) fr - arrays < (double) ((size_t) 8 << 20)) cap = (size_t) 8 << 20;
    }
  *whole_in = cap == 0;
  return cap;
}

int dx_file_compare(dx_ctx *ctx, int kind, const uint8_t *img_a, size_t m_a, const uint8_t *img_b, size_t m_b,
                    int lossy, dx_compare *out, uint32_t **rec_differ)
{ static const uint8_t lossy_and[5] = { 0xff, 0xff, 0xfe, 0xfc, 0xff };      /* QV.c:1406-1415: the insertion and the merge line */
  cmp_pair   p;
  cmp_job    j;
  dx_compare c;
  int        rc, side = 'a';

  if (ctx == NULL || out == NULL || (img_a == NULL && m_a) || (img_b == NULL && m_b)) return DX_E_ARG;
  if (kind != DX_KIND_FASTA && kind != DX_KIND_ARROW && kind != DX_KIND_QUIVA) return DX_E_ARG;
  if (lossy && kind != DX_KIND_QUIVA) return DX_E_ARG;
  if (rec_differ) *rec_differ = NULL;
  memset(&p, 0, sizeof(p)); memset(&j, 0, sizeof(j));
  j.ctx = ctx; j.p = &p; j.c = &c; j.a_and = lossy ? lossy_and : NULL; j.side = 'a';

  if ((rc = dxf_compare_open(ctx, kind, img_a, m_a, img_b, m_b, &p, &c, &side)) != DX_OK)
    { rc = dx_side_fail(ctx, rc, side); goto done; }
  if ((j.rec = calloc((size_t) (p.both + 1) * (size_t) c.lines, sizeof(*j.rec))) == NULL) { rc = DX_E_NOMEM; goto done; }

  if (p.both > 0 && kind != DX_KIND_QUIVA)
    TRY(compare_pack2(&j, dxf_u2_cap(ctx, (size_t) (p.pa[p.both] + p.pb[p.both]), p.both)));     /* (of the two images together) */
  else if (p.both > 0)
    { const size_t cap = compare_qv_cap(ctx, &p, &j.whole_in);
      uint64_t i0, i1;
      for (i0 = 0; i0 < p.both; i0 = i1)
        { i1 = dxf_compare_slice_end(&p, i0, cap);
          j.side = 'a';
          (void) dx_side_fail(ctx, DX_OK, 0);
          if ((rc = dxf_image_range(ctx, &p.a, i0, i1, j.whole_in, compare_qv_a, &j)) != DX_OK)
            { if (j.side) rc = dx_side_fail(ctx, rc, j.side);
              goto done;
            }
        }
    }

  c.same = c.records_a == c.records_b && !c.prefix_differs && c.headers_differ == 0 && c.lengths_differ == 0 && c.records_differ == 0;
  *out = c;
  if (rec_differ) { *rec_differ = j.rec; j.rec = NULL; }
  rc = DX_OK;

done:
  if (j.d_arr) (void) dx_free(ctx, j.d_arr);
  free(j.h_arr); free(j.rec);
  dxf_compare_close(&p);
  return rc;
}
