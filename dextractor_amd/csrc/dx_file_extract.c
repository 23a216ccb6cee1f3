/*
 * dx_file_extract.c -- chosen records of a .dexta / .dexar / .dexqv image as the text undexta / undexar / undexqv print for them alone: a
 * list of records in any order, whole or an interval of each, decoded and nothing else -- no image is made on the way (the route through
 * dx_file_subset and a decoder frames, for quiva even codes, an image that is thrown away).
 *
 *     fasta / arrow   the image walked (dxf_u2_walk), the selected reads' packed spans up (dxf_sel_slices), ONE dx_reads_unpack_lines a slice
 *                     straight into the text's layout
 *     quiva           the stream walked (dx_file_undexqv_plan_on: the format stores no lengths, so that cost stays), the selected records'
 *                     spans up unless the plan has the image on the device, dx_qv_decode on the gathered starts
 *
 * The header lines are printed by the decoders' own printers with B_E moved to (B + beg)_(B + end), and laid into the text on the host
 * once a slice's bytes are down, as dxf_slice_deliver does it.
 *
 * What an interval of a quiva entry costs: a Huffman stream has no way in at symbol `beg`, so the WHOLE entry is decoded, into scratch,
 * and dx_copy_ranges gathers the five line intervals from there -- an interval of a long entry costs the entry's decode and five lines of
 * scratch, and an entry selected k times is decoded k times.  Whole entries are decoded where they end up.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dexgpu.h"
#include "dx_host.h"
#include "dx_files.h"

#define WHO "dx_file_extract"

/* the text's layout, common to the kinds: unit j's header line is hd[hat[j] .. hat[j + 1]) and goes to to[j], its lines to body[j];
   to[n]: the text's end.  un, at: the unit's span of the image and its first byte, as dxf_sel_slices takes them */
typedef struct
  { uint64_t  n, *to, *body, *at, *hat;
    rspan    *un;
    tbuf      hd;
  } ext_layout;

static int layout_alloc(ext_layout *y, uint64_t n)
{ memset(y, 0, sizeof(*y));
  y->n  = n;
  y->to = malloc((n + 1) * sizeof(*y->to)); y->body = malloc((n + 1) * sizeof(*y->body)); y->at = malloc((n + 1) * sizeof(*y->at));
  y->hat = malloc((n + 1) * sizeof(*y->hat)); y->un = malloc((n + 1) * sizeof(*y->un));
  return y->to && y->body && y->at && y->hat && y->un ? DX_OK : DX_E_NOMEM;
}

static void layout_free(ext_layout *y)
{ free(y->to); free(y->body); free(y->at); free(y->hat); free(y->un); free(y->hd.p);
  memset(y, 0, sizeof(*y));
}

/* unit j, whose header line has just been printed behind hat[j], has `lines` bytes of lines and reaches bytes [lo, hi) of the image */
static void layout_unit(ext_layout *y, uint64_t j, size_t *total, size_t lines, uint64_t lo, uint64_t hi)
{ y->to[j]   = *total;
  y->body[j] = *total + (y->hd.len - (size_t) y->hat[j]);
  *total     = (size_t) y->body[j] + lines;
  y->un[j].lo = y->at[j] = lo; y->un[j].hi = hi; y->un[j].j = j;
}

/* the text is down: the header lines into it, and the results out */
static int layout_deliver(ext_layout *y, uint8_t *res, size_t total, uint8_t **text, size_t *text_bytes, uint64_t **toff)
{ uint64_t j;
  for (j = 0; j < y->n; j++)
    memcpy(res + y->to[j], y->hd.p + y->hat[j], (size_t) (y->body[j] - y->to[j]));
  y->to[y->n] = total;
  *text = res; *text_bytes = total;
  if (toff) { *toff = y->to; y->to = NULL; }
  return DX_OK;
}

/* where the units of a slice that begins with unit j0 go in the slice's text, on the device: body[j0 + k] - to[j0] */
static int slice_places(dpool *pool, const ext_layout *y, uint64_t j0, uint64_t m, void **d_place)
{ uint64_t *rel = malloc((size_t) (m + 1) * sizeof(*rel)), k;
  int rc;
  if (rel == NULL) return DX_E_NOMEM;
  for (k = 0; k < m; k++) rel[k] = y->body[j0 + k] - y->to[j0];
  rc = dupload(pool, rel, (size_t) m * 8, d_place);
  free(rel);
  return rc;
}

/* ==========================================================================================
 *  fasta / arrow: one dx_reads_unpack_lines a slice
 * ========================================================================================== */
typedef struct { dx_ctx *ctx; int letters; uint32_t width; const ext_layout *y; const uint32_t *ph, *len; } ext2_job;

static int ext2_slice(void *arg, dpool *pool, const void *d_in, uint64_t in_bytes, const uint64_t *d_start, const uint64_t *d_ooff,
                      uint64_t j0, uint64_t m, int packed, void *d_out, uint64_t *bad)
{ const ext2_job *e = arg;
  void *d_beg, *d_len, *d_place;
  int   rc;
  (void) packed; (void) d_ooff;                           /* (a unit's place is its header line's: the letters go behind it) */
  TRY(dupload(pool, e->ph + j0, (size_t) m * 4, &d_beg));
  TRY(dupload(pool, e->len + j0, (size_t) m * 4, &d_len));
  TRY(slice_places(pool, e->y, j0, m, &d_place));
  TRY(dx_reads_unpack_lines(e->ctx, e->letters, d_in, in_bytes, d_start, d_beg, d_len, m, e->width, d_out, d_place, bad));
done:
  return rc;
}

static int extract2(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, selection *s, int upper, uint32_t width,
                    uint8_t **text, size_t *text_bytes, uint64_t **toff)
{ const int arrow = kind == DX_KIND_ARROW, letters = arrow ? DX_LETTERS_ARROW : upper ? DX_LETTERS_UPPER : DX_LETTERS_LOWER;
  u2_index    x;
  ext_layout  y;
  uint32_t   *ph = NULL, *len = NULL;
  char       *name = NULL;
  uint8_t    *res = NULL;
  size_t      total = 0;
  uint64_t    j;
  uint16_t    key;
  int32_t     plen;
  int         rc;

  memset(&y, 0, sizeof(y));
  TRY(dxf_u2_walk(letters, img, m, NULL, &x));
  rc = dxf_sel_check(ctx, WHO, s, x.cnt, x.nsym, 0);
  if (rc == DX_E_DEGENERATE) { s->n = 0; rc = DX_OK; }    /* (every record of an image without records: undexta prints nothing) */
  if (rc != DX_OK) goto done;
  memcpy(&key, img, 2); memcpy(&plen, img + 2, 4);        /* (the walk has seen to it that both are there, and the prefix) */
  if (key == 0xaa55 || key == 0xcc33) plen = (int32_t) flip32((uint32_t) plen);
  name = malloc((size_t) plen + 1);
  ph = malloc((s->n + 1) * sizeof(*ph)); len = malloc((s->n + 1) * sizeof(*len));
  if ((rc = layout_alloc(&y, s->n)) != DX_OK) goto done;
  if (!name || !ph || !len) { rc = DX_E_NOMEM; goto done; }
  memcpy(name, img + 6, (size_t) plen); name[plen] = '\0';

  for (j = 0; j < s->n; j++)                              /* well/B_E becomes well/(B + beg)_(B + end) */
    { const uint64_t id = sel_id(s, j), b = sel_beg(s, j), e = sel_end(s, j, x.nsym), L = e - b;
      const int32_t *h  = x.hdr4 + 4 * id;
      y.hat[j] = y.hd.len;
      TRY(dxf_u2_header(&y.hd, arrow, name, h[0], h[1] + (int32_t) b, h[1] + (int32_t) e, h[3], x.cnr4 + 4 * id));
      layout_unit(&y, j, &total, (size_t) (L + (L + width - 1) / width), x.ioff[id] + b / 4, L ? x.ioff[id] + (e - 1) / 4 + 1 : x.ioff[id] + b / 4);
      ph[j] = (uint32_t) (b & 3); len[j] = (uint32_t) L;
    }
  y.hat[s->n] = y.hd.len; y.to[s->n] = total;
  if ((res = malloc(total + 16)) == NULL) { rc = DX_E_NOMEM; goto done; }
  if (s->n > 0)
    { ext2_job e = { ctx, letters, width, &y, ph, len };
      TRY(dxf_sel_slices(ctx, img, m, NULL, y.un, y.at, y.to, s->ids, s->n, x.ioff, "reads_packed", "reads_whole", ext2_slice, &e, res));
    }
  rc = layout_deliver(&y, res, total, text, text_bytes, toff);
  res = NULL;
done:
  dxf_u2_index_free(&x);
  layout_free(&y);
  free(ph); free(len); free(name); free(res);
  return rc;
}

/* ==========================================================================================
 *  quiva: dx_qv_decode on gathered starts, sizes and lengths; an interval by way of scratch
 * ========================================================================================== */
typedef struct
  { dx_ctx *ctx; const selection *s; const ext_layout *y; const dx_qv_index *x;
    int flags;
  } extq_job;

/* A slice's units in three sorts: whole entries, decoded where they end up; intervals, whose entries are decoded into scratch and gathered;
   and units without symbols, which are five line ends.  The slice's text is line ends to begin with when there is one of the last two. */
static int extq_slice(void *arg, dpool *pool, const void *d_in, uint64_t in_bytes, const uint64_t *d_start, const uint64_t *d_ooff,
                      uint64_t j0, uint64_t m, int packed, void *d_out, uint64_t *bad)
{ const extq_job *q = arg;
  const dx_qv_index *x = q->x;
  const size_t bytes = (size_t) (q->y->to[j0 + m] - q->y->to[j0]);
  uint64_t  nW = 0, nI = 0, k, iw = 0, ii = 0, scratch = 0;
  uint64_t *start = NULL, *h64 = NULL;
  void     *d_arr = NULL, *d_scr = NULL, *d_place;
  int       rc = DX_OK;
  (void) packed; (void) d_ooff; (void) bad; (void) in_bytes;

  for (k = 0; k < m; k++)
    { const uint64_t id = sel_id(q->s, j0 + k);
      const uint32_t b = sel_beg(q->s, j0 + k), e = sel_end(q->s, j0 + k, x->len);
      if (e == b) continue;
      if (b == 0 && e == x->len[id]) nW++; else nI++;
    }
  if (nW == m)                                            /* whole entries all: the slice's starts as they are */
    { uint32_t *h32 = malloc((size_t) m * 24 + 64);
      void     *d_seg;
      if (h32 == NULL) return DX_E_NOMEM;
      for (k = 0; k < m; k++)
        { const uint64_t id = sel_id(q->s, j0 + k);
          memcpy(h32 + 5 * k, x->seg + 5 * id, 20);
          h32[5 * m + k] = x->len[id];
        }
      rc = dupload(pool, h32, (size_t) m * 24, &d_seg);
      free(h32);
      if (rc != DX_OK) return rc;
      TRY(slice_places(pool, q->y, j0, m, &d_place));
      TRY(dx_qv_decode(q->ctx, d_in, d_start, NULL, d_seg, (const uint32_t *) d_seg + 5 * m, m, q->flags, d_out, d_place));
      return DX_OK;
    }

  /* per sort, in 64-bit words: the entries' starts and where their lines go (W: in the text; I: in scratch); five ranges an interval
     (source, length, destination); then in 32-bit words the segment sizes (5) and lengths of W, and of I */
  { const size_t w64 = (size_t) (2 * nW + 2 * nI + 15 * nI), w32 = (size_t) (6 * nW + 6 * nI);
    uint64_t *sW, *oW, *sI, *oI, *rs, *rl, *rd;
    uint32_t *gW, *lW, *gI, *lI;
    start = malloc((size_t) (m + 1) * 8); h64 = malloc(w64 * 8 + w32 * 4 + 64);
    if (!start || !h64) { rc = DX_E_NOMEM; goto done; }
    sW = h64; oW = sW + nW; sI = oW + nW; oI = sI + nI; rs = oI + nI; rl = rs + 5 * nI; rd = rl + 5 * nI;
    gW = (uint32_t *) (rd + 5 * nI); lW = gW + 5 * nW; gI = lW + nW; lI = gI + 5 * nI;
    TRY(dx_d2h(q->ctx, start, d_start, (size_t) m * 8));
    for (k = 0; k < m; k++)
      { const uint64_t id = sel_id(q->s, j0 + k), L = x->len[id], place = q->y->body[j0 + k] - q->y->to[j0];
        const uint32_t b = sel_beg(q->s, j0 + k), e = sel_end(q->s, j0 + k, x->len), l = e - b;
        int line;
        if (l == 0) continue;
        if (b == 0 && e == L)
          { sW[iw] = start[k]; oW[iw] = place; memcpy(gW + 5 * iw, x->seg + 5 * id, 20); lW[iw] = (uint32_t) L; iw++; }
        else
          { sI[ii] = start[k]; oI[ii] = scratch; memcpy(gI + 5 * ii, x->seg + 5 * id, 20); lI[ii] = (uint32_t) L;
            for (line = 0; line < 5; line++)
              { rs[5 * ii + line] = scratch + (uint64_t) line * (L + 1) + b;
                rl[5 * ii + line] = l;
                rd[5 * ii + line] = place + (uint64_t) line * ((uint64_t) l + 1);
              }
            scratch += 5 * (L + 1);
            ii++;
          }
      }
    TRY(dupload(pool, h64, w64 * 8 + w32 * 4, &d_arr));
    TRY(dx_memset(q->ctx, d_out, '\n', bytes));
    { const uint64_t *dsW = d_arr, *doW = dsW + nW, *dsI = doW + nW, *doI = dsI + nI, *drs = doI + nI, *drl = drs + 5 * nI, *drd = drl + 5 * nI;
      const uint32_t *dgW = (const uint32_t *) (drd + 5 * nI), *dlW = dgW + 5 * nW, *dgI = dlW + nW, *dlI = dgI + 5 * nI;
      if (nW > 0) TRY(dx_qv_decode(q->ctx, d_in, dsW, NULL, dgW, dlW, nW, q->flags, d_out, doW));
      if (nI > 0)
        { TRY(dalloc(pool, (size_t) scratch, &d_scr));
          TRY(dx_qv_decode(q->ctx, d_in, dsI, NULL, dgI, dlI, nI, q->flags, d_scr, doI));
          TRY(dx_copy_ranges(q->ctx, d_scr, scratch, drs, drl, 5 * nI, d_out, drd, NULL));
        }
    }
  }
done:
  free(start); free(h64);
  return rc;
}

static int extract_qv(dx_ctx *ctx, const uint8_t *img, size_t m, selection *s, int upper,
                      uint8_t **text, size_t *text_bytes, uint64_t **toff)
{ dx_undexqv_plan *p = NULL;
  dx_qv_index x;
  ext_layout  y;
  uint8_t    *res = NULL;
  size_t      total = 0, whole_text = 0;
  uint64_t    j;
  int         rc;

  memset(&y, 0, sizeof(y)); memset(&x, 0, sizeof(x));
  TRY(dx_file_undexqv_plan_on(ctx, img, m, &p, &whole_text));
  rc = dxf_sel_check(ctx, WHO, s, p->x.n, p->x.len, 0);
  if (rc == DX_E_DEGENERATE) { s->n = 0; rc = DX_OK; }
  if (rc != DX_OK) goto done;
  TRY(dx_file_undexqv_plan_index(p, &x));                 /* (the index on the host, wherever the walk was made: O(records)) */
  TRY(layout_alloc(&y, s->n));
  for (j = 0; j < s->n; j++)
    { const uint64_t id = sel_id(s, j), b = sel_beg(s, j), e = sel_end(s, j, x.len);
      const int32_t *h  = x.hdr4 + 4 * id;
      const int32_t  h4[4] = { h[0], h[1] + (int32_t) b, h[1] + (int32_t) e, h[3] };
      y.hat[j] = y.hd.len;
      TRY(dxf_qv_header(&y.hd, x.prefix, h4));
      layout_unit(&y, j, &total, (size_t) (5 * (e - b + 1)), x.rec_off[id] + (x.hdr_off[id + 1] - x.hdr_off[id]), x.rec_off[id + 1]);
    }
  y.hat[s->n] = y.hd.len; y.to[s->n] = total;
  if ((res = malloc(total + 16)) == NULL) { rc = DX_E_NOMEM; goto done; }
  if (s->n > 0)
    { extq_job q = { ctx, s, &y, &x, (upper ? DX_DECODE_UPPER : 0) | (x.flip ? DX_DECODE_FLIP : 0) };
      TRY(dx_qv_set_coding(ctx, &x.coding, 0));
      TRY(dxf_sel_slices(ctx, img, m, PLAN_HAS_IMAGE(p) ? p->d_in : NULL, y.un, y.at, y.to, s->ids, s->n, x.rec_off,
                         "entries_packed", "entries_whole", extq_slice, &q, res));
    }
  rc = layout_deliver(&y, res, total, text, text_bytes, toff);
  res = NULL;
done:
  dx_qv_index_free(&x);
  dx_file_undexqv_plan_free(p);
  layout_free(&y);
  free(res);
  return rc;
}

int dx_file_extract(dx_ctx *ctx, int kind, const uint8_t *img, size_t m,
                    const uint64_t *ids, const uint32_t *beg, const uint32_t *end, uint64_t n_ids,
                    int upper, uint32_t width, uint8_t **text, size_t *text_bytes, uint64_t **toff)
{ selection s = { ids, beg, end, n_ids };
  int rc;
  if (ctx == NULL || text == NULL || text_bytes == NULL) return DX_E_ARG;
  if (kind != DX_KIND_FASTA && kind != DX_KIND_ARROW && kind != DX_KIND_QUIVA) return DX_E_ARG;
  *text = NULL; *text_bytes = 0;
  if (toff) *toff = NULL;
  rc = dxf_sel_args(ctx, WHO, img, ids, beg, end, n_ids);
  if (rc != DX_OK && rc != DX_E_DEGENERATE) return rc;    /* (no units: an empty text, once the image has been looked at) */
  if (kind == DX_KIND_QUIVA) return extract_qv(ctx, img, m, &s, upper, text, text_bytes, toff);
  if (width == 0) return dx_unit_fail(ctx, DX_E_ARG, WHO, 0, "line width must be >= 1 (the reference loops forever on -w0, undexta.c:265)");
  return extract2(ctx, kind, img, m, &s, upper, width, text, text_bytes, toff);
}
