/*
 * dx_select.c -- units at known starts: the in-memory entry API of a .qvs track (dx_entries_*) and the read loader of a .bps / .arw
 * payload (dx_reads_uncompress), with the one loader that brings either selection to the device and its text back.
 */
#include <stdlib.h>
#include <string.h>

#include "dexgpu.h"
#include "dx_env.h"
#include "dx_host.h"
#include "dx_files.h"

/* ==========================================================================================
 *  in-memory entry API: the shape of QVcoding_Scan1 /
 *  Compress_Next_QVentry1 (QV.c:866-920, 1343-1379), i.e. what dex2DB.c:511-643 calls per entry
 *  to write a .qvs track -- as a batch: entries are gathered on the host, then scanned and
 *  compressed together on the GPU.  The output is the bare record stream (no framing bytes) and
 *  the offset of every entry in it (DAZZ_READ.coff, dex2DB.c:617-621).
 * ========================================================================================== */
struct dx_entries
  { uint8_t  *text;  size_t tlen, tcap;      /* five lines back to back per entry (line_pad 0) */
    uint64_t *off;   uint32_t *len;
    uint64_t  n, cap;
  };

dx_entries *dx_entries_new(void) { return calloc(1, sizeof(dx_entries)); }

void dx_entries_free(dx_entries *e)
{ if (e == NULL) return;
  free(e->text); free(e->off); free(e->len); free(e);
}

/* QVcoding_Scan1's / Compress_Next_QVentry1's argument list: one entry, five streams of rlen bytes */
int dx_entries_add(dx_entries *e, int rlen, const char *del, const char *tag, const char *ins,
                   const char *mrg, const char *sub)
{ const char *s[5];
  int k;
  if (e == NULL || rlen < 0 || (rlen > 0 && (!del || !tag || !ins || !mrg || !sub))) return DX_E_ARG;
  s[0] = del; s[1] = tag; s[2] = ins; s[3] = mrg; s[4] = sub;
  if (e->n == e->cap)
    { uint64_t nc = e->cap ? 2 * e->cap : 1024;
      uint64_t *no = realloc(e->off, nc * sizeof(*no));
      uint32_t *nl = realloc(e->len, nc * sizeof(*nl));
      if (no) e->off = no;
      if (nl) e->len = nl;
      if (!no || !nl) return DX_E_NOMEM;
      e->cap = nc;
    }
  if (e->tlen + 5 * (size_t) rlen + 16 > e->tcap)
    { size_t nc = 2 * e->tcap + 5 * (size_t) rlen + 4096;
      uint8_t *nt = realloc(e->text, nc);
      if (!nt) return DX_E_NOMEM;
      e->text = nt; e->tcap = nc;
    }
  e->off[e->n] = e->tlen;
  e->len[e->n] = (uint32_t) rlen;
  for (k = 0; k < 5; k++)
    { memcpy(e->text + e->tlen, s[k], (size_t) rlen);
      e->tlen += (size_t) rlen;
    }
  e->n += 1;
  return DX_OK;
}

int dx_entries_compress(dx_ctx *ctx, const dx_entries *e, int lossy, dx_qv_coding *coding,
                        uint8_t **records, size_t *nbytes, uint64_t **coff)
{ dpool        pool = { {0}, 0, ctx };
  qv_staged    st;
  dx_qv_params p = { -1, -1, -1, -1 };
  uint64_t   (*hist)[256] = NULL, tot = 0, total = 0;
  void        *d_text, *d_off, *d_len, *d_out = NULL;
  size_t       out_cap = 0;
  uint8_t     *res = NULL;
  uint64_t    *ro = NULL;
  int          rc;

  if (ctx == NULL || e == NULL || coding == NULL || records == NULL || nbytes == NULL) return DX_E_ARG;
  *records = NULL; *nbytes = 0;
  if (coff) *coff = NULL;
  if (e->n == 0) return DX_E_DEGENERATE;
  hist = calloc(6, sizeof(*hist));
  if (!hist) return DX_E_NOMEM;
  TRY(dupload(&pool, e->text, e->tlen, &d_text));
  TRY(dupload(&pool, e->off, e->n * 8, &d_off));
  TRY(dupload(&pool, e->len, e->n * 4, &d_len));
  TRY(dxf_qv_stage(&pool, NULL, e->n, NULL, d_text, d_off, d_len, e->tlen, 0, &st));      /* (line_pad 0, no framing bytes) */
  TRY(dx_qv_scan(ctx, &st.b, 0, &p, hist, &tot));          /* QVcoding_Scan1 over all entries */
  TRY(dx_qv_build((const uint64_t (*)[256]) hist, tot, &p, lossy, coding));   /* Create_QVcoding */
  TRY(dx_qv_set_coding(ctx, coding, lossy));
  TRY(dxf_qv_encode_batch(ctx, &st, (const uint64_t (*)[256]) hist, coding, lossy, &d_out, &out_cap, &total));     /* Compress_Next_QVentry1 x n */
  res = malloc(total + 16);
  ro  = malloc((e->n + 1) * sizeof(*ro));
  if (!res || !ro) { rc = DX_E_NOMEM; goto done; }
  TRY(dx_d2h(ctx, res, d_out, total));
  TRY(dx_d2h(ctx, ro, st.d_rec, (e->n + 1) * 8));
  *records = res; *nbytes = total; res = NULL;
  if (coff) { *coff = ro; ro = NULL; }
  rc = DX_OK;

done:
  if (d_out) (void) dx_free(ctx, d_out);
  dfree_all(&pool);
  free(hist); free(res); free(ro);
  return rc;
}

/* ==========================================================================================
 *  A selection of units at known starts -- records of a .qvs track, reads of a .bps / .arw payload,
 *  any of them in any order -- decoded as a batch.  What travels is decided here for both kinds: every
 *  unit has a span of the input that it can reach, and the selection's spans are merged; when they
 *  cover less than HALF of the input they go up packed side by side (a slice's own spans per slice),
 *  else the whole input goes up once -- unless the input, with a slice of 4 MB of text beside it, is
 *  more than the device has free: then the packed way is taken, since a slice's spans are what has to fit.
 * ========================================================================================== */
static int rspan_cmp(const void *a, const void *b)
{ const rspan *x = a, *y = b;
  return x->lo < y->lo ? -1 : x->lo > y->lo ? 1 : x->j < y->j ? -1 : x->j > y->j;
}

/* The spans of sp[0 .. m), sorted here, merged and laid side by side: rel[sp[k].j] = where span k begins in that layout; with dst the
   bytes are copied there.  Returns the layout's bytes. */
static uint64_t spans_pack(rspan *sp, uint64_t m, const uint8_t *records, uint8_t *dst, uint64_t *rel)
{ uint64_t k, base = 0, lo = 0, hi = 0;
  qsort(sp, (size_t) m, sizeof(*sp), rspan_cmp);
  for (k = 0; k < m; k++)
    { if (k == 0 || sp[k].lo > hi)                        /* a gap: the run of spans so far is complete */
        { if (dst != NULL && hi > lo) memcpy(dst + base, records + lo, (size_t) (hi - lo));
          base += hi - lo;
          lo = sp[k].lo; hi = sp[k].hi;
        }
      else if (sp[k].hi > hi) hi = sp[k].hi;
      if (rel != NULL) rel[sp[k].j] = base + (sp[k].lo - lo);
    }
  if (dst != NULL && hi > lo) memcpy(dst + base, records + lo, (size_t) (hi - lo));
  return base + (hi - lo);
}

/* Does a selection's stream go up whole?  When its merged spans cover half of it or more -- and the device has room for it beside a
   slice of text: else the packed way whatever is selected, since a slice's spans are what has to fit.  (Tests: packed_key /
   whole_key in DEXGPU_TEST decide.) */
static int sel_goes_whole(dx_ctx *ctx, uint64_t covered, size_t nbytes, const char *packed_key, const char *whole_key)
{ int whole = 2 * covered >= nbytes && !dx_test_on(packed_key);
  if (whole)
    { uint64_t fr = 0, all_b = 0;
      if (dx_mem_info(ctx, &fr, &all_b) == DX_OK && fr != 0 && (double) nbytes + (double) ((size_t) 4 << 20) > 0.9 * (double) fr) whole = 0;
    }
  if (dx_test_on(whole_key)) whole = 1;
  return whole;
}

/* a slice of whole units of a selection from j0 on, to[] their places in the text: at most cap bytes of it (0: all at once), one unit at least */
static uint64_t sel_slice_end(const uint64_t *to, uint64_t j0, uint64_t n_ids, size_t cap)
{ const uint64_t m_most = (uint64_t) 1 << 30;
  uint64_t j1;
  for (j1 = j0 + 1; j1 < n_ids && j1 - j0 < m_most && (cap == 0 || to[j1 + 1] - to[j0] <= cap); j1++) ;
  return j1;
}

/* The one loader of a selection (dx_files.h: the hook sel_fn, and what the arguments are): whole or packed by sel_goes_whole, unless the
   input is on the device already. */
int dxf_sel_slices(dx_ctx *ctx, const uint8_t *in, size_t nbytes, const void *d_have, const rspan *un, const uint64_t *at,
                   const uint64_t *to, const uint64_t *ids, uint64_t n_ids, const uint64_t *start, const char *packed_key,
                   const char *whole_key, sel_fn fn, void *arg, uint8_t *res)
{ dpool     all = { {0}, 0, ctx }, pool = { {0}, 0, ctx };
  rspan    *sp  = malloc((n_ids + 1) * sizeof(*sp));      /* a slice's spans, as spans_pack sorts them */
  uint64_t *rel = malloc((n_ids + 1) * sizeof(*rel)), j, j0, j1, covered;
  uint8_t  *stage = NULL;
  void     *d_whole = (void *) d_have;                    /* (there already: not this call's to bring up, or to free) */
  size_t    cap;
  int       rc = DX_OK, whole;

  if (!sp || !rel) { rc = DX_E_NOMEM; goto done; }
  memcpy(sp, un, (size_t) n_ids * sizeof(*sp));
  covered = spans_pack(sp, n_ids, in, NULL, NULL);
  whole   = d_have != NULL || sel_goes_whole(ctx, covered, nbytes, packed_key, whole_key);
  cap     = dxf_out_cap(ctx, d_have != NULL ? 0 : whole ? nbytes : (size_t) covered, (size_t) to[n_ids], n_ids);
  if (whole && d_have == NULL) TRY(dupload(&all, in, nbytes, &d_whole));
  if (!whole)                                             /* (no slice's spans are more than the selection's) */
    { stage = malloc((size_t) covered + 16);
      if (stage == NULL) { rc = DX_E_NOMEM; goto done; }
    }

  for (j0 = 0; j0 < n_ids; j0 = j1)                       /* slices of whole units: at most cap bytes of text each (0: all at once) */
    { void    *d_in = d_whole, *d_start, *d_ooff, *d_out;
      uint64_t m, in_bytes = nbytes, bad = UINT64_MAX;
      j1 = sel_slice_end(to, j0, n_ids, cap);
      m  = j1 - j0;
      if (whole)
        memcpy(rel, at + j0, (size_t) m * 8);
      else                                                /* this slice's spans, packed */
        { for (j = 0; j < m; j++) { sp[j] = un[j0 + j]; sp[j].j = j; }
          in_bytes = spans_pack(sp, m, in, stage, rel);
          TRY(dupload(&pool, stage, (size_t) in_bytes, &d_in));
        }
      TRY(dupload(&pool, rel, m * 8, &d_start));
      for (j = 0; j < m; j++) rel[j] = to[j0 + j] - to[j0];   /* the units' places in the slice's text */
      TRY(dupload(&pool, rel, m * 8, &d_ooff));
      TRY(dalloc(&pool, (size_t) (to[j1] - to[j0]), &d_out));
      rc = fn(arg, &pool, d_in, in_bytes, d_start, d_ooff, j0, m, !whole, d_out, &bad);
      if (rc == DX_E_FORMAT && bad != UINT64_MAX)         /* the caller's unit, not its place in the slice */
        { const uint64_t id = ids ? ids[j0 + bad] : j0 + bad;
          rc = dx_entry_fail(ctx, id, start[id], nbytes);
        }
      if (rc != DX_OK) goto done;
      TRY(dx_d2h(ctx, res + to[j0], d_out, (size_t) (to[j1] - to[j0])));
      dfree_all(&pool);
    }

done:
  dfree_all(&pool);
  dfree_all(&all);
  free(sp); free(rel); free(stage);
  return rc;
}

/* ==========================================================================================
 *  ... the read side of a .qvs track: Load_QVentry (DB.c:2575-2621) = a seek to DAZZ_READ.coff and
 *  Uncompress_Next_QVentry (QV.c:1428-1481) with the read's length, for any read in any order -- as
 *  a batch: the selected records' segment sizes by dx_qv_walk_records_device (a lane a record), then
 *  dx_qv_decode with the entries' starts as d_rec_off and no framing bytes.
 *
 *  A record's size is not stored, but it has a bound -- every line's symbols at the longest code of
 *  its scheme (a run-coded line: a token for every symbol), and the tags: its span is [coff, coff +
 *  bound).  A record must end inside its span: one that does not is DX_E_FORMAT, whole or packed.
 * ========================================================================================== */
/* bits a symbol of a line can take at most: the longest code, an escape's literal, and in a run-coded line a run code with its literal */
static uint32_t line_bits_most(const dx_qv_coding *cd, int sym, int run)
{ uint32_t m = 0, r = 0;
  int i;
  for (i = 0; i < 256; i++)
    { if (cd->s[sym].lens[i] > (int32_t) m) m = (uint32_t) cd->s[sym].lens[i];
      if (run >= 0 && cd->s[run].lens[i] > (int32_t) r) r = (uint32_t) cd->s[run].lens[i];
    }
  return m + (cd->s[sym].type == 2 ? 8u : 0u) + (run >= 0 ? r + 16u : 0u);
}

/* bytes a record of L symbols a line takes at most (bits: line_bits_most of its four coded lines), pad words and tags included */
static uint64_t record_bytes_most(uint64_t L, const uint32_t bits[4])
{ uint64_t most = (L + 3) >> 2;
  int k;
  for (k = 0; k < 4 && L > 0; k++) most += (L * bits[k] + 7) / 8 + 8;
  return most;
}

/* a slice of entries (sel_fn): their segment sizes walked, then decoded.  len, at: per selected entry; seg: the host's room for a slice's sizes */
typedef struct { dx_ctx *ctx; const dx_qv_coding *coding; int flip, flags; size_t nbytes; const uint32_t *len, *bits; const uint64_t *at; uint32_t *seg; } qvs_job;

static int qvs_slice(void *arg, dpool *pool, const void *d_in, uint64_t in_bytes, const uint64_t *d_start, const uint64_t *d_ooff,
                     uint64_t j0, uint64_t m, int packed, void *d_out, uint64_t *bad)
{ const qvs_job *q = arg;
  void    *d_len, *d_seg;
  uint64_t j;
  int      rc;
  TRY(dupload(pool, q->len + j0, m * 4, &d_len));
  TRY(dalloc(pool, m * 20, &d_seg));
  TRY(dx_qv_walk_records_device(q->ctx, d_in, in_bytes, d_start, d_len, m, q->coding, q->flip, d_seg, bad));
  if (packed)                                             /* a record ends inside its own span, not in a neighbour's bytes */
    { TRY(dx_d2h(q->ctx, q->seg, d_seg, m * 20));
      for (j = 0; j < m; j++)
        { const uint32_t *s = q->seg + 5 * j;
          const uint64_t used = (uint64_t) s[0] + s[1] + s[2] + s[3] + s[4];
          if (used > record_bytes_most(q->len[j0 + j], q->bits) || used > q->nbytes - q->at[j0 + j])
            { *bad = j; return DX_E_FORMAT; }
        }
    }
  TRY(dx_qv_decode(q->ctx, d_in, d_start, NULL, d_seg, d_len, m, q->flags, d_out, d_ooff));
done:
  return rc;
}

int dx_entries_uncompress(dx_ctx *ctx, const dx_qv_coding *coding, int flip,
                          const uint8_t *records, size_t nbytes, const uint64_t *coff, const uint32_t *rlen,
                          const uint64_t *ids, uint64_t n_ids,
                          int ascii, uint8_t **text, size_t *text_bytes, uint64_t **toff)
{ rspan    *un = NULL;                                    /* un[j]: the span of the stream that entry j of the selection can reach */
  uint64_t *to = NULL, *at = NULL, j;
  uint32_t *len = NULL, *seg = NULL, bits[4];
  uint8_t  *res = NULL;
  int       rc = DX_OK;

  if (ctx == NULL || coding == NULL || text == NULL || text_bytes == NULL || toff == NULL || ascii < 0 || ascii > 2) return DX_E_ARG;
  if (n_ids > 0 && (coff == NULL || rlen == NULL || (records == NULL && nbytes > 0))) return DX_E_ARG;
  *text = NULL; *text_bytes = 0; *toff = NULL;
  to  = malloc((n_ids + 1) * sizeof(*to));
  un  = malloc((n_ids + 1) * sizeof(*un));
  at  = malloc((n_ids + 1) * sizeof(*at));
  len = malloc((n_ids + 1) * sizeof(*len));
  seg = malloc((n_ids + 1) * 5 * sizeof(*seg));
  if (!to || !un || !at || !len || !seg) { rc = DX_E_NOMEM; goto done; }

  /* the text's layout, and every entry's span of the stream */
  bits[0] = line_bits_most(coding, DX_DEL, coding->delChar >= 0 ? DX_DRUN : -1);
  bits[1] = line_bits_most(coding, DX_INS, -1);
  bits[2] = line_bits_most(coding, DX_MRG, -1);
  bits[3] = line_bits_most(coding, DX_SUB, coding->subChar >= 0 ? DX_SRUN : -1);
  to[0] = 0;
  for (j = 0; j < n_ids; j++)
    { const uint64_t id = ids ? ids[j] : j, L = rlen[id], most = record_bytes_most(L, bits);
      if (L > 0x7fffffffu || coff[id] > nbytes)
        { rc = dx_entry_fail(ctx, id, coff[id], nbytes); goto done; }
      un[j].lo = at[j] = coff[id]; un[j].j = j;
      un[j].hi = nbytes - coff[id] < most ? nbytes : coff[id] + most;
      len[j] = (uint32_t) L;
      to[j + 1] = to[j] + 5 * (L + 1);
    }
  res = malloc((size_t) to[n_ids] + 16);
  if (res == NULL) { rc = DX_E_NOMEM; goto done; }
  if (n_ids == 0) goto deliver;

  TRY(dx_qv_set_coding(ctx, coding, 0));
  { qvs_job q = { ctx, coding, flip, (ascii == 2 ? DX_DECODE_UPPER : 0) | (flip ? DX_DECODE_FLIP : 0), nbytes, len, bits, at, seg };
    TRY(dxf_sel_slices(ctx, records, nbytes, NULL, un, at, to, ids, n_ids, coff, "entries_packed", "entries_whole", qvs_slice, &q, res));
  }
  if (ascii == 0)                                         /* DB.c:2605-2610: the tag line through Number_Read (DB.c:393-416) */
    for (j = 0; j < n_ids; j++)
      { uint8_t *t = res + to[j] + len[j] + 1;
        uint32_t k;
        for (k = 0; k < len[j]; k++)
          t[k] = t[k] == 'c' ? 1 : t[k] == 'g' ? 2 : t[k] == 't' ? 3 : 0;
      }

deliver:
  *text = res; *text_bytes = (size_t) to[n_ids]; *toff = to;
  res = NULL; to = NULL;
  rc = DX_OK;

done:
  free(un); free(at); free(len); free(seg); free(res); free(to);
  return rc;
}

/* ==========================================================================================
 *  The .bps / .arw read side: Load_Read (DB.c:1232-1298), Load_Subread (DB.c:1308-1381), Load_Arrow
 *  (DB.c:1508-1548) for a selection at once, in Load_All_Reads' layout (DB.c:1406-1433) -- dx_reads_unpack
 *  on the selected units.  A unit's span of the payload is exact: bytes [boff + beg / 4, boff +
 *  (end - 1) / 4 + 1), cut at the payload's end.  A span that is cut ends the packed layout as it ends
 *  the payload, so the unit reaches past the end of what the device has either way, and the kernel's
 *  own check finds it.
 * ========================================================================================== */
/* a slice of units (sel_fn); ph, len: per selected unit, the phase of its first base in its byte and its bases */
typedef struct { dx_ctx *ctx; int letters; const uint32_t *ph, *len; } reads_job;

static int reads_slice(void *arg, dpool *pool, const void *d_in, uint64_t in_bytes, const uint64_t *d_start, const uint64_t *d_ooff,
                       uint64_t j0, uint64_t m, int packed, void *d_out, uint64_t *bad)
{ const reads_job *r = arg;
  void *d_beg, *d_len;
  int   rc;
  (void) packed;
  TRY(dupload(pool, r->ph + j0, m * 4, &d_beg));
  TRY(dupload(pool, r->len + j0, m * 4, &d_len));
  TRY(dx_reads_unpack(r->ctx, r->letters, d_in, in_bytes, d_start, d_beg, d_len, m, d_out, d_ooff, bad));
done:
  return rc;
}

int dx_reads_uncompress(dx_ctx *ctx, int letters, const uint8_t *payload, size_t nbytes,
                        const uint64_t *boff, const uint32_t *rlen,
                        const uint64_t *ids, const uint32_t *beg, const uint32_t *end, uint64_t n_ids,
                        uint8_t **text, size_t *text_bytes, uint64_t **toff)
{ rspan    *un = NULL;                                    /* un[j]: unit j's span */
  uint64_t *to = NULL, *at = NULL, j;                     /* at[j]: where unit j's first byte is, cut or not */
  uint32_t *len = NULL, *ph = NULL;
  uint8_t  *res = NULL;
  int       rc = DX_OK;
  const uint8_t delim = letters == DX_LETTERS_NUMBERS ? 4 : 0;    /* DB.c:362 / DB.c:367-389 */

  if (ctx == NULL || text == NULL || text_bytes == NULL || toff == NULL || letters < DX_LETTERS_LOWER || letters > DX_LETTERS_NUMBERS)
    return DX_E_ARG;
  if ((beg == NULL) != (end == NULL)) return DX_E_ARG;
  if (n_ids > 0 && (boff == NULL || rlen == NULL || (payload == NULL && nbytes > 0))) return DX_E_ARG;
  *text = NULL; *text_bytes = 0; *toff = NULL;
  to  = malloc((n_ids + 1) * sizeof(*to));
  un  = malloc((n_ids + 1) * sizeof(*un));
  at  = malloc((n_ids + 1) * sizeof(*at));
  len = malloc((n_ids + 1) * sizeof(*len));
  ph  = malloc((n_ids + 1) * sizeof(*ph));
  if (!to || !un || !at || !len || !ph) { rc = DX_E_NOMEM; goto done; }

  /* the text's layout, and every unit's span of the payload */
  to[0] = 1;
  for (j = 0; j < n_ids; j++)
    { const uint64_t id = ids ? ids[j] : j, L = rlen[id];
      const uint64_t b = beg ? beg[j] : 0, e = end ? end[j] : L;
      uint64_t lo, hi;
      if (b > e || e > L || e - b > 0x7fffffffu) { rc = DX_E_ARG; goto done; }
      if (boff[id] > nbytes)
        { rc = dx_entry_fail(ctx, id, boff[id], nbytes); goto done; }
      lo = boff[id] + b / 4;
      hi = e > b ? boff[id] + (e - 1) / 4 + 1 : lo;
      un[j].lo = lo < nbytes ? lo : nbytes;
      un[j].hi = hi < nbytes ? hi : nbytes;
      un[j].j  = j;
      at[j]  = lo;
      len[j] = (uint32_t) (e - b);
      ph[j]  = (uint32_t) (b & 3);
      to[j + 1] = to[j] + (e - b) + 1;
    }
  res = malloc((size_t) to[n_ids] + 16);
  if (res == NULL) { rc = DX_E_NOMEM; goto done; }
  res[0] = delim;
  if (n_ids == 0) goto deliver;

  { reads_job r = { ctx, letters, ph, len };
    TRY(dxf_sel_slices(ctx, payload, nbytes, NULL, un, at, to, ids, n_ids, boff, "reads_packed", "reads_whole", reads_slice, &r, res));
  }

deliver:
  *text = res; *text_bytes = (size_t) to[n_ids]; *toff = to;
  res = NULL; to = NULL;
  rc = DX_OK;

done:
  free(un); free(at); free(len); free(ph); free(res); free(to);
  return rc;
}
