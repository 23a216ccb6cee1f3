/*
 * dx_walk_host.c -- bare-file index: walk a .dexqv image front to back (host)
 *
 *  The format stores no record or segment lengths (QV.c:1428-1481; undexqv.c:119-208), so the
 *  start of every segment is known only after the previous one has been walked code by code.
 *  This is that walk: it decodes code LENGTHS only (plus what it needs to count symbols) and
 *  yields the index dx_qv_decode takes.  Inherently sequential; everything that produces
 *  symbols runs on the GPU afterwards.
 */
#include <pthread.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "dexgpu.h"
#include "dx_env.h"
#include "dx_host.h"
#include "dx_layout.h"
#include "dx_walk.h"

/* ---- look-up tables ---------------------------------------------------------------------------------------------------- */

typedef struct { uint16_t e[0x10000]; } wlut;          /* len << 8 | symbol, by 16-bit window (QV.c:365-372) */

static void build_wlut(const dx_scheme *s, wlut *t)
{ int i;
  memset(t->e, 0, sizeof(t->e));
  for (i = 0; i < 256; i++)                             /* ascending: 255 wins shared escape codes */
    if (s->lens[i] > 0 && s->lens[i] <= 16)
      { uint32_t base = (s->bits[i] << (16 - s->lens[i])) & 0xffffu, cnt = 1u << (16 - s->lens[i]), j;
        for (j = 0; j < cnt; j++)
          t->e[(base + j) & 0xffffu] = (uint16_t) ((s->lens[i] << 8) | i);
      }
}

/* Several codes per look-up for the walk, which needs lengths only: for every 12-bit window, how
   many whole codes it holds, their total length and the length of the last one (escape codes end
   a group: the 8-bit literal that follows is not a code).  8 KB per scheme: stays in L1. */
#define MW_BITS 12
typedef struct { uint8_t nbits, nsym, last, pad; } mwent;
typedef struct { mwent e[1 << MW_BITS]; } mwlut;

static void build_mwlut(const wlut *t, int esc, mwlut *m)
{ uint32_t x;
  for (x = 0; x < (1u << MW_BITS); x++)
    { uint32_t pos = 0, cnt = 0, last = 0;
      for (;;)
        { uint32_t e = t->e[((x << (16 - MW_BITS)) << pos) & 0xffffu], l = e >> 8;
          if (l == 0 || pos + l > MW_BITS || (esc && (e & 0xff) == 255)) break;
          pos += l; cnt += 1; last = l;
        }
      m->e[x].nbits = (uint8_t) pos; m->e[x].nsym = (uint8_t) cnt; m->e[x].last = (uint8_t) last; m->e[x].pad = 0;
    }
}

/* The same for a run-coded stream: a (run code, symbol code) pair that fits the window whole and
   needs no literal (run < 255, symbol not escaped). */
typedef struct { uint8_t nbits, run, last, ok; } rwent;
typedef struct { rwent e[1 << MW_BITS]; } rwlut;

static void build_rwlut(const wlut *rt, const wlut *nt, int esc, rwlut *m)
{ uint32_t x;
  for (x = 0; x < (1u << MW_BITS); x++)
    { const uint32_t w  = x << (16 - MW_BITS);
      const uint32_t e1 = rt->e[w], l1 = e1 >> 8;
      rwent g = { 0, 0, 0, 0 };
      if (l1 > 0 && l1 < MW_BITS && (e1 & 0xff) != 255)
        { const uint32_t e2 = nt->e[(w << l1) & 0xffffu], l2 = e2 >> 8;
          if (l2 > 0 && l1 + l2 <= MW_BITS && !(esc && (e2 & 0xff) == 255))
            { g.nbits = (uint8_t) (l1 + l2); g.run = (uint8_t) (e1 & 0xff); g.last = (uint8_t) l2; g.ok = 1; }
        }
      m->e[x] = g;
    }
}

/* everything a walk needs besides the image */
typedef struct
  { wlut  *lut[6];                    /* DX_DEL .. DX_SRUN; a run scheme's only when the coding has the run character */
    mwlut *mlut[4];
    rwlut *rlut[2];                   /* del, sub: with lut[DX_DRUN] / lut[DX_SRUN] */
    int    esc[4];                    /* scheme DX_DEL .. DX_SUB is of the escape kind */
    int    newv, flip;
    int    want_index;                /* leave the group index too (dx_qv_walk_indexed) */
  } walk_tabs;

static void walk_tabs_free(walk_tabs *t)
{ int s;
  for (s = 0; s < 6; s++) free(t->lut[s]);
  for (s = 0; s < 4; s++) free(t->mlut[s]);
  free(t->rlut[0]); free(t->rlut[1]);
  memset(t, 0, sizeof(*t));
}

/* the tables of a coding into *t (anything else in it is zeroed); DX_E_NOMEM leaves what was built to walk_tabs_free */
static int walk_tabs_build(const dx_qv_coding *cd, walk_tabs *t)
{ int s;
  memset(t, 0, sizeof(*t));
  for (s = 0; s < 6; s++)
    { if ((s == DX_DRUN && cd->delChar < 0) || (s == DX_SRUN && cd->subChar < 0)) continue;
      if ((t->lut[s] = malloc(sizeof(wlut))) == NULL) return DX_E_NOMEM;
      build_wlut(&cd->s[s], t->lut[s]);
      if (s < 4)
        { t->esc[s] = cd->s[s].type == 2;
          if ((t->mlut[s] = malloc(sizeof(mwlut))) == NULL) return DX_E_NOMEM;
          build_mwlut(t->lut[s], t->esc[s], t->mlut[s]);
        }
    }
  for (s = 0; s < 2; s++)
    { const int sym = s ? DX_SUB : DX_DEL, run = s ? DX_SRUN : DX_DRUN;
      if (t->lut[run] == NULL) continue;
      if ((t->rlut[s] = malloc(sizeof(rwlut))) == NULL) return DX_E_NOMEM;
      build_rwlut(t->lut[run], t->lut[sym], t->esc[sym], t->rlut[s]);
    }
  return DX_OK;
}

/* The same tables for the device walk (dx_qv_walk.hip), 16 bits an entry: layout in dx_walk.h. */
int dx_walk_luts_build(const dx_qv_coding *cd, uint8_t *blob, int esc[4])
{ walk_tabs t;
  int       s, rc;
  uint32_t  x;
  if (cd == NULL || blob == NULL || esc == NULL) return DX_E_ARG;
  memset(blob, 0, WALK_BLOB_BYTES);
  rc = walk_tabs_build(cd, &t);
  for (s = 0; s < 6 && rc == DX_OK; s++)
    if (t.lut[s] != NULL) memcpy(blob + WALK_W16_OFF + (size_t) s * 65536u * 2u, t.lut[s]->e, 65536u * 2u);
  for (s = 0; s < 4 && rc == DX_OK; s++)
    { uint16_t *m16 = (uint16_t *) (blob + WALK_MW_OFF) + (size_t) s * 4096u;
      uint16_t *o16 = (uint16_t *) (blob + WALK_ONE_OFF) + (size_t) s * 4096u;
      esc[s] = t.esc[s];
      for (x = 0; x < 4096u; x++)
        { const mwent    g = t.mlut[s]->e[x];
          const uint32_t e = t.lut[s]->e[x << 4], l = e >> 8;
          const uint32_t first = (l > 0 && l <= WALK_WIN && !(esc[s] && (e & 0xff) == 255)) ? l : 0u;
          m16[x] = g.nsym ? (uint16_t) (g.nbits | (g.last << 4) | (g.nsym << 8)) : 0;
          o16[x] = first ? (uint16_t) (first | (first << 4) | (1u << 8)) : 0;
        }
    }
  for (s = 0; s < 2 && rc == DX_OK; s++)
    { const wlut *rt = t.lut[s ? DX_SRUN : DX_DRUN];
      uint16_t *r16 = (uint16_t *) (blob + WALK_RW_OFF) + (size_t) s * 4096u;
      uint16_t *o16 = (uint16_t *) (blob + WALK_R1_OFF) + (size_t) s * 4096u;
      if (rt == NULL) continue;
      for (x = 0; x < 4096u; x++)
        { const rwent    g  = t.rlut[s]->e[x];
          const uint32_t e1 = rt->e[x << 4], l1 = e1 >> 8;
          r16[x] = g.ok ? (uint16_t) (g.nbits | (g.last << 4) | (((uint32_t) g.run + 1u) << 8)) : 0;
          o16[x] = (l1 > 0 && l1 <= WALK_WIN && (e1 & 0xff) != 255) ? (uint16_t) (l1 | (l1 << 4) | ((e1 & 0xff) << 8)) : 0;
        }
    }
  walk_tabs_free(&t);
  return rc;
}

/* ---- one segment ------------------------------------------------------------------------------------------------------- */

typedef struct { const uint8_t *p, *end; uint64_t buf; int nb; uint64_t T; int flip; } wrd;

static void w_fill(wrd *r)
{ if (r->p + 4 <= r->end)                               /* (well predicted; the data-dependent part is branch-free) */
    { uint32_t w;
      const uint64_t take = (uint64_t) 0 - (uint64_t) (r->nb <= 32);      /* all ones: the buffer has room for a word */
      memcpy(&w, r->p, 4);
      if (r->flip) w = flip32(w);
      r->buf |= ((uint64_t) w << ((32 - r->nb) & 63)) & take;
      r->nb  += (int) (32 & take);
      r->p   += 4 & take;
    }
}
static uint32_t w_peek(wrd *r) { w_fill(r); return (uint32_t) (r->buf >> 48); }
static void w_skip(wrd *r, int n) { r->buf <<= n; r->nb -= n; r->T += (uint64_t) n; }

static uint32_t pad_words(uint64_t T, uint32_t last)    /* QV.c:436-442 */
{ uint32_t olen = (uint32_t) T & 31u, llen = (uint32_t) (T - last) & 31u;
  uint32_t w = (uint32_t) (T >> 5) + (olen ? 1u : 0u);
  if (olen > 0) return w + ((llen > 16u && olen > llen) ? 1u : 0u);
  return w + ((T > 0 && llen > 16u) ? 1u : 0u);
}

/* Bytes of a plain-coded segment of rlen symbols starting at p (QV.c:510-599); -1: it does not end inside the image.  Several
   codes per look-up (mwlut), one code where they would pass the segment's end.
   With `share` the walk also leaves the line's share of the GROUP INDEX the wave-per-line decoders take (dx_layout.h; device
   side: dx_device.hpp, k_qv_encode_fast writes it, k_qv_decode_sub reads it): one byte per group of 16 symbols = the group's
   code bits minus its symbols.  The several-codes look-ups then also stop at a group's boundary. */
static int64_t walk_plain(const uint8_t *p, const uint8_t *end, uint32_t rlen, const wlut *t, const mwlut *m,
                          int esc, int flip, uint8_t *share)
{ wrd r = { p, end, 0, 0, 0, flip };
  uint32_t j = 0, last = 0, gbits = 0, none = 0;
  int64_t bytes;
  while (j < rlen)
    { uint32_t w = w_peek(&r);
      const mwent g = m->e[w >> (16 - MW_BITS)];
      if (r.nb < 0) return -1;                           /* more bits consumed than the image holds */
      if (g.nsym && j + g.nsym <= rlen && (share == NULL || (j & 15u) + g.nsym <= 16u))
        { w_skip(&r, g.nbits);
          j += g.nsym; gbits += g.nbits; last = g.last;
        }
      else
        { uint32_t e = t->e[w];
          last = e >> 8;
          if (last == 0) return -1;                        /* no such code */
          w_skip(&r, (int) last);
          gbits += last;
          if (esc && (e & 0xff) == 255)
            { w_peek(&r); w_skip(&r, 8); last = 8; gbits += 8; }
          j += 1;
        }
      if (share != NULL && ((j & 15u) == 0 || j == rlen))
        { const uint32_t valid = (j & 15u) ? (j & 15u) : 16u;
          if (gbits - valid > 254u) none = 1;               /* does not fit the byte (escape schemes): no index for this line */
          share[(j - 1) >> 4] = (uint8_t) (gbits - valid);
          gbits = 0;
        }
    }
  if (share != NULL && (none || esc) && rlen) share[0] = (uint8_t) DXL_SUB_NONE;
  bytes = 4 * (int64_t) pad_words(r.T, last);
  return (p + bytes <= end) ? bytes : -1;
}

/* The same for a run-coded segment (QV.c:604-691); *nonrun receives the number of non-run symbols.  One look-up for a
   (run code, symbol code) pair that fits the window whole and needs no literal, else one code at a time.
   With tb / ts (room for rlen tokens) the walk also notes per token its bits and the positions it covers (run + 1). */
static int64_t walk_runs(const uint8_t *p, const uint8_t *end, uint32_t rlen, const wlut *nt, int esc,
                         const wlut *rt, const rwlut *pair, uint32_t *nonrun, int flip, uint16_t *tb, uint32_t *ts)
{ wrd r = { p, end, 0, 0, 0, flip };
  uint32_t j = 0, last = 0, nn = 0;
  int64_t bytes;
  while (j < rlen)
    { uint32_t w = w_peek(&r), e, c, bits;
      const rwent g = pair->e[w >> (16 - MW_BITS)];
      if (r.nb < 0) return -1;                           /* more bits consumed than the image holds */
      if (g.ok && j + g.run < rlen)                      /* run, then a symbol that exists */
        { w_skip(&r, g.nbits);
          if (tb != NULL) { tb[nn] = g.nbits; ts[nn] = (uint32_t) g.run + 1u; }
          j   += (uint32_t) g.run + 1u;
          nn  += 1;
          last = g.last;
          continue;
        }
      e = rt->e[w]; c = e & 0xff;
      last = e >> 8;
      if (last == 0) return -1;                            /* no such code */
      w_skip(&r, (int) last);
      bits = last;
      if (c == 255)
        { c = w_peek(&r); w_skip(&r, 16); last = 16; bits += 16; }
      if (c > rlen - j) return -1;
      j += c;
      if (j < rlen)
        { e = nt->e[w_peek(&r)];
          last = e >> 8;
          if (last == 0) return -1;
          w_skip(&r, (int) last);
          bits += last;
          if (esc && (e & 0xff) == 255)
            { w_peek(&r); w_skip(&r, 8); last = 8; bits += 8; }
          if (tb != NULL) { tb[nn] = (uint16_t) bits; ts[nn] = c + 1u; }
          j  += 1;
          nn += 1;
        }
    }
  *nonrun = nn;
  bytes = 4 * (int64_t) pad_words(r.T, last);
  return (p + bytes <= end) ? bytes : -1;
}

/* ---- one record -------------------------------------------------------------------------------------------------------- */

typedef struct { uint32_t hdr_bytes, len, seg[5]; int32_t dwell, beg, end, qv; uint64_t gx_at, gx_words; uint32_t gx_none; } walk_rec;

/* index words of the records a thread walks (in the order it walks them) + its token scratch */
typedef struct { uint32_t *w; uint64_t n, cap; uint16_t *tb; uint32_t *ts; uint32_t tcap; } gx_buf;

static void gx_free(gx_buf *g) { free(g->w); free(g->tb); free(g->ts); memset(g, 0, sizeof(*g)); }

static uint32_t *gx_room(gx_buf *g, uint64_t words)        /* `words` more zeroed words; NULL: out of memory */
{ if (g->n + words > g->cap)
    { uint64_t nc = g->cap ? g->cap : (1u << 16);
      uint32_t *q;
      while (nc < g->n + words) nc *= 2;
      q = realloc(g->w, nc * sizeof(*q));
      if (q == NULL) return NULL;
      g->w = q; g->cap = nc;
    }
  memset(g->w + g->n, 0, words * sizeof(uint32_t));
  g->n += words;
  return g->w + g->n - words;
}

/* token scratch for a line of rlen symbols, and an entry's first words: the four plain shares and the three header words
   (dx_layout.h), the run-coded lines' "no index" until gx_run_line says otherwise; 0: out of memory */
static int gx_open(gx_buf *g, uint32_t rlen)
{ const uint64_t at = g->n;
  const uint32_t rb = dxl_run_base(rlen);
  if (rlen > g->tcap)
    { uint16_t *tb = realloc(g->tb, ((size_t) rlen + 1) * sizeof(*tb));
      uint32_t *ts;
      if (tb == NULL) return 0;
      g->tb = tb;
      ts = realloc(g->ts, ((size_t) rlen + 1) * sizeof(*ts));
      if (ts == NULL) return 0;
      g->ts = ts; g->tcap = rlen;
    }
  if (gx_room(g, (uint64_t) rb + 3u) == NULL) return 0;
  g->w[at + rb + 0] = DXL_RUN_NONE; g->w[at + rb + 1] = DXL_RUN_NONE;
  return 1;
}

/* the group words of a run-coded line from its tokens, as k_qv_encode_fast cuts them: passes of 512 tokens, in a pass
   of m tokens lane l holds the (m + 63) / 64 tokens from l times that on; word = bits | positions << 16.  Returns the
   header word: the token count, or DXL_RUN_NONE when a group does not fit (positions > 65535, a pass > RUN_PASSBITS). */
static uint32_t run_groups(const uint16_t *tb, const uint32_t *ts, uint32_t cnt, uint32_t L, uint32_t *grp)
{ uint32_t k0, none = 0;
  if (cnt > dxl_tok_limit(L)) none = 1;    /* more tokens than the encoder's token slots hold: such a line never has an
                                                             index (k_qv_decode_runs refuses one), the lane-per-line kernel takes it */
  for (k0 = 0; k0 < cnt; k0 += DXL_RUN_PASS, grp += 64)
    { const uint32_t m = cnt - k0 < DXL_RUN_PASS ? cnt - k0 : DXL_RUN_PASS, T = (m + 63u) >> 6;
      uint32_t lane, total = 0;
      for (lane = 0; lane < 64; lane++)
        { const uint32_t first = lane * T, c = first < m ? (m - first < T ? m - first : T) : 0u;
          uint32_t nb = 0, span = 0, k;
          for (k = 0; k < c; k++) { nb += tb[k0 + first + k]; span += ts[k0 + first + k]; }
          if (span > 0xffffu || nb > 0xffffu) none = 1;
          grp[lane] = nb | (span << 16);
          total += nb;
        }
      if (total > DXL_RUN_PASSBITS) none = 1;
    }
  return none ? DXL_RUN_NONE : cnt;
}

/* The group words of the run-coded line just walked into g->tb / g->ts (cnt tokens, of an entry of L symbols whose header
   words stand at g->w[hdr]): 64 words a pass behind what the entry has so far, the line's header word (which: 0 deletion,
   1 substitution; 0 tokens -- a line of run characters only -- is an index too) and, for the deletion line, its passes in
   the third.  0: out of memory. */
static int gx_run_line(gx_buf *g, uint64_t hdr, int which, uint32_t cnt, uint32_t L, walk_rec *r)
{ const uint32_t passes = dxl_run_passes(cnt);
  uint32_t *grp = gx_room(g, 64ull * passes);
  if (grp == NULL) return 0;
  g->w[hdr + which] = run_groups(g->tb, g->ts, cnt, L, grp);
  if (g->w[hdr + which] == DXL_RUN_NONE) r->gx_none += 1;
  if (which == 0) g->w[hdr + 2] = passes;
  return 1;
}

/* beg, end and qv of a record's framing at p: 32-bit fields (0x55aa-keyed images) or 16-bit ones, byte-swapped or not
   (undexqv.c:140-179); returns their bytes */
static size_t framing_fields(const uint8_t *p, int newv, int flip, int32_t f[3])
{ int k;
  for (k = 0; k < 3; k++)
    if (newv) { uint32_t v; memcpy(&v, p + 4*k, 4); f[k] = (int32_t) (flip ? flip32(v) : v); }
    else      { uint16_t v; memcpy(&v, p + 2*k, 2); f[k] = flip ? flip16(v) : v; }
  return newv ? 12 : 6;
}

/* the framing of a record (undexqv.c:119-180); returns the offset of its first segment, 0: no plausible record here */
static size_t walk_framing(const walk_tabs *t, const uint8_t *img, size_t n, size_t at, walk_rec *r)
{ const size_t h0 = at;
  int32_t  f[3], dw = 0;
  uint32_t rlen;

  while (at < n && img[at] == 255) { dw += 255; at += 1; }
  if (at >= n) return 0;
  dw += img[at++];
  if (at + (t->newv ? 12 : 6) > n) return 0;
  at += framing_fields(img + at, t->newv, t->flip, f);
  if (f[1] < f[0] || (int64_t) f[1] - (int64_t) f[0] > 0x7fffffff) return 0;
  rlen = (uint32_t) ((int64_t) f[1] - (int64_t) f[0]);
  if ((uint64_t) rlen > 65536u * 8u * (uint64_t) (n - at) + 64u)      /* a token has >= 1 bit and covers <= 65536 symbols */
    return 0;
  r->hdr_bytes = (uint32_t) (at - h0);
  r->len = rlen; r->dwell = dw; r->beg = f[0]; r->end = f[1]; r->qv = f[2];
  return at;
}

/* One record at img + at (undexqv.c:119-208): the framing, then the five segments walked code by code (QV.c:1433-1478).
   Returns the offset behind the record; 0 if there is no well-formed record here.  With g the record's share of the group
   index is appended to it; on failure g is as it was. */
static size_t walk_record(const walk_tabs *t, const uint8_t *img, size_t n, size_t at, walk_rec *r, gx_buf *g)
{ static const struct { int sym, run, slot; } line[5] =    /* symbol scheme (-1: the deletion line's tags, 2 bits for every symbol
                                                              it spelt out), run scheme if the coding has the run character, plain share */
    { { DX_DEL, DX_DRUN, 0 }, { -1, -1, -1 }, { DX_INS, -1, 1 }, { DX_MRG, -1, 2 }, { DX_SUB, DX_SRUN, 3 } };
  const uint8_t *end = img + n;
  const uint64_t g0 = g != NULL ? g->n : 0;
  uint32_t rlen, clen, sw = 0, rb = 0;
  int      k;

  at = walk_framing(t, img, n, at, r);
  if (at == 0) return 0;
  rlen = clen = r->len;
  if (g != NULL)
    { if (!gx_open(g, rlen)) return 0;
      sw = dxl_sub_words(rlen); rb = dxl_run_base(rlen);
      r->gx_at = g0; r->gx_none = 0;
    }
  for (k = 0; k < 5; k++)
    { const int s = line[k].sym, run = line[k].run;
      int64_t   b;
      if (s < 0)
        b = at + ((clen + 3) >> 2) <= n ? (int64_t) ((clen + 3) >> 2) : -1;
      else if (run < 0 || t->lut[run] == NULL)
        b = walk_plain(img + at, end, rlen, t->lut[s], t->mlut[s], t->esc[s], t->flip,
                       g != NULL ? (uint8_t *) (g->w + g0 + (uint32_t) line[k].slot * sw) : NULL);
      else
        { uint32_t nn = 0;
          b = walk_runs(img + at, end, rlen, t->lut[s], t->esc[s], t->lut[run], t->rlut[run - DX_DRUN], &nn, t->flip,
                        g != NULL ? g->tb : NULL, g != NULL ? g->ts : NULL);
          if (b >= 0 && g != NULL && !gx_run_line(g, g0 + rb, run - DX_DRUN, nn, rlen, r)) b = -1;
          if (s == DX_DEL) clen = nn;
        }
      if (b < 0)
        { if (g != NULL) g->n = g0;
          return 0;
        }
      r->seg[k] = (uint32_t) b; at += (size_t) b;
    }
  if (g != NULL) r->gx_words = g->n - g0;
  return at;
}

/* ---- records at known starts ------------------------------------------------------------------------------------------- */

/* The five segments of a record without framing bytes (a .qvs track: dex2DB.c:617-621, read back by Load_QVentry,
   DB.c:2575-2621) at buf + at, rlen symbols a line: their sizes into seg.  0: a segment does not end inside the buffer. */
static int walk_segments(const walk_tabs *t, const uint8_t *buf, size_t n, size_t at, uint32_t rlen, uint32_t seg[5])
{ static const struct { int sym, run; } line[5] =
    { { DX_DEL, DX_DRUN }, { -1, -1 }, { DX_INS, -1 }, { DX_MRG, -1 }, { DX_SUB, DX_SRUN } };
  uint32_t clen = rlen;
  int      k;
  if (at > n) return 0;
  if (rlen == 0)                                          /* QV.c:436-442: nothing is written for an empty stream */
    { memset(seg, 0, 5 * sizeof(uint32_t)); return 1; }
  for (k = 0; k < 5; k++)
    { const int s = line[k].sym, run = line[k].run;
      int64_t   b;
      if (s < 0)
        b = at + ((clen + 3) >> 2) <= n ? (int64_t) ((clen + 3) >> 2) : -1;
      else if (run < 0 || t->lut[run] == NULL)
        b = walk_plain(buf + at, buf + n, rlen, t->lut[s], t->mlut[s], t->esc[s], t->flip, NULL);
      else
        { uint32_t nn = 0;
          b = walk_runs(buf + at, buf + n, rlen, t->lut[s], t->esc[s], t->lut[run], t->rlut[run - DX_DRUN], &nn, t->flip, NULL, NULL);
          if (s == DX_DEL) clen = nn;
        }
      if (b < 0) return 0;
      seg[k] = (uint32_t) b; at += (size_t) b;
    }
  return 1;
}

int dx_qv_walk_records(const uint8_t *buf, size_t nbytes, const uint64_t *start, const uint32_t *rlen, uint64_t n,
                       const dx_qv_coding *cd, int flip, uint32_t *seg, uint64_t *bad_entry)
{ walk_tabs t;
  uint64_t  i;
  int       rc;
  if (bad_entry) *bad_entry = UINT64_MAX;
  if (cd == NULL || (n > 0 && (start == NULL || rlen == NULL || seg == NULL)) || (buf == NULL && nbytes > 0)) return DX_E_ARG;
  if (n == 0) return DX_OK;
  rc = walk_tabs_build(cd, &t);
  t.flip = flip != 0;
  for (i = 0; i < n && rc == DX_OK; i++)
    if (rlen[i] > 0x7fffffffu || !walk_segments(&t, buf, nbytes, (size_t) start[i], rlen[i], seg + 5 * i))
      { if (bad_entry) *bad_entry = i;
        rc = DX_E_FORMAT;
      }
  walk_tabs_free(&t);
  return rc;
}

/* ---- the records of an image ------------------------------------------------------------------------------------------- */

/* records of img[from, to) appended to a growing list; stops at `to` exactly (returns it), behind it
   (a record straddles `to`: returns that offset) or 0 on a malformed record / out of memory (*rc says which) */
typedef struct { walk_rec *r; uint64_t n, cap; gx_buf gx; } rec_list;

static void rec_list_free(rec_list *L) { free(L->r); gx_free(&L->gx); memset(L, 0, sizeof(*L)); }

static size_t walk_span(const walk_tabs *t, const uint8_t *img, size_t n, size_t from, size_t to, rec_list *L, int *rc)
{ size_t at = from;
  while (at < to)
    { size_t nx;
      if (L->n == L->cap)
        { uint64_t  nc = L->cap ? 2 * L->cap : 1024;
          walk_rec *q  = realloc(L->r, nc * sizeof(*q));
          if (q == NULL) { *rc = DX_E_NOMEM; return 0; }
          L->r = q; L->cap = nc;
        }
      nx = walk_record(t, img, n, at, &L->r[L->n], t->want_index ? &L->gx : NULL);
      if (nx == 0) { *rc = DX_E_FORMAT; return 0; }
      L->n += 1;
      at = nx;
    }
  return at;
}

/* ---- the walk on several host threads ---------------------------------------------------------
 * Where a record starts is only known by walking from the file's first record -- but a guessed start can be
 * CHECKED: the image is cut into pieces, a thread per piece looks for the first offset in its piece at which
 * a plausible record header stands (0 <= beg <= end, a sane quality value) AND from which two consecutive
 * records walk cleanly, and then walks from there to the start the next thread found.  Arriving there
 * exactly proves both guesses (a walk from a wrong offset does not re-synchronise onto record boundaries:
 * framing fields and pad words are not self-delimiting); any thread that overshoots its neighbour's start
 * condemns the attempt, and the file is walked front to back as before.  Results are identical by
 * construction: only offsets verified by an unbroken chain of walks from the first record are kept.   */
typedef struct
  { const walk_tabs *t;
    const uint8_t   *img;
    size_t           n, lo, hi;       /* piece [lo, hi) */
    size_t           start, stop;     /* where this thread's records begin / must end */
    size_t           landed;
    rec_list         L;
    int              rc;
  } walk_job;

static int header_plausible(const walk_tabs *t, const uint8_t *img, size_t n, size_t at)
{ int32_t f[3];
  int k = 0;
  while (at < n && img[at] == 255 && k < 16) { at += 1; k += 1; }
  if (at + 13 > n) return 0;
  at += 1;
  framing_fields(img + at, 1, t->flip, f);              /* (guessed at in 0x55aa-keyed images only) */
  /* A guess that passes costs a walk of its (garbage) length: entries beyond 4 M symbols are left to be
     reached by the neighbouring thread's walk rather than guessed at (1 in ~10^7 offsets passes by chance). */
  return f[0] >= 0 && f[0] < (1 << 28) && f[1] >= f[0] && f[1] - f[0] <= (1 << 22) && f[2] >= 0 && f[2] < 1000000 &&
         (uint64_t) (f[1] - f[0]) <= 8u * (uint64_t) (n - at);
}

static void *walk_find(void *arg)                       /* first checked record start in the piece (0: none) */
{ walk_job *j = arg;
  size_t p;
  j->start = 0;
  for (p = j->lo; p < j->hi; p++)
    if (header_plausible(j->t, j->img, j->n, p))
      { walk_rec r;
        size_t a = walk_record(j->t, j->img, j->n, p, &r, NULL), b;
        if (a == 0) continue;
        if (a == j->n) { j->start = p; break; }         /* the file's last record */
        if (!header_plausible(j->t, j->img, j->n, a)) continue;
        b = walk_record(j->t, j->img, j->n, a, &r, NULL);
        if (b == 0) continue;
        j->start = p;
        break;
      }
  return NULL;
}

static void *walk_piece(void *arg)
{ walk_job *j = arg;
  j->rc = DX_OK;
  j->landed = walk_span(j->t, j->img, j->n, j->start, j->stop, &j->L, &j->rc);
  return NULL;
}

#define WALK_PIECE_MIN ((size_t) 2 << 20)               /* bytes of image a thread should at least have */
#define WALK_THREADS_MAX 64

static void walk_mark(const char *what)                  /* DEXGPU_TIMING=1: where the walk's time goes */
{ static double t0 = 0;
  dx_mark("walk", &t0, what);
}

/* records of img[first, n) into *out on up to `threads` threads; DX_E_MISMATCH: the guesses did not chain up */
static int walk_parallel(const walk_tabs *t, const uint8_t *img, size_t n, size_t first, int threads, rec_list *out)
{ walk_job  job[WALK_THREADS_MAX];
  pthread_t th[WALK_THREADS_MAX];
  int       T = threads, k, m, rc = DX_OK, made;
  size_t    piece;
  if (T > WALK_THREADS_MAX) T = WALK_THREADS_MAX;
  if ((size_t) T > (n - first) / WALK_PIECE_MIN) T = (int) ((n - first) / WALK_PIECE_MIN);
  if (T < 2) return DX_E_MISMATCH;
  piece = (n - first) / (size_t) T;
  memset(job, 0, sizeof(job));
  for (k = 0; k < T; k++)
    { job[k].t = t; job[k].img = img; job[k].n = n;
      job[k].lo = first + (size_t) k * piece;
      job[k].hi = k == T - 1 ? n : first + (size_t) (k + 1) * piece;
    }
  job[0].start = first;
  made = 0;                                             /* guesses: pieces 1 .. T-1 */
  for (k = 1; k < T; k++)
    { if (pthread_create(&th[k], NULL, walk_find, &job[k]) != 0) break;
      made = k;
    }
  for (k = 1; k <= made; k++) pthread_join(th[k], NULL);
  walk_mark("record starts guessed and checked");
  if (made < T - 1) return DX_E_MISMATCH;
  m = 0;                                                /* pieces without a start are walked by their predecessor */
  for (k = 1; k < T; k++)
    if (job[k].start != 0)
      { job[m].stop = job[k].start;
        m += 1;
        if (m != k) job[m] = job[k];
      }
  job[m].stop = n;
  T = m + 1;
  made = -1;
  for (k = 0; k < T; k++)
    { if (pthread_create(&th[k], NULL, walk_piece, &job[k]) != 0) break;
      made = k;
    }
  for (k = 0; k <= made; k++) pthread_join(th[k], NULL);
  walk_mark("pieces walked");
  if (made < T - 1) rc = DX_E_MISMATCH;
  for (k = 0; k < T && rc == DX_OK; k++)
    if (job[k].rc == DX_E_NOMEM) rc = DX_E_NOMEM;
    else if (job[k].rc != DX_OK || job[k].landed != job[k].stop) rc = DX_E_MISMATCH;   /* a wrong guess (or a damaged file): walk it front to back */
  if (rc == DX_OK)
    { uint64_t tot = 0, at = 0, gw = 0, gat = 0, i;
      for (k = 0; k < T; k++) { tot += job[k].L.n; gw += job[k].L.gx.n; }
      out->r = malloc((tot + 1) * sizeof(walk_rec));
      if (t->want_index) out->gx.w = malloc((gw + 1) * sizeof(uint32_t));
      if (out->r == NULL || (t->want_index && out->gx.w == NULL)) rc = DX_E_NOMEM;
      else
        { for (k = 0; k < T; k++)
            { memcpy(out->r + at, job[k].L.r, job[k].L.n * sizeof(walk_rec));
              if (t->want_index)
                { memcpy(out->gx.w + gat, job[k].L.gx.w, job[k].L.gx.n * sizeof(uint32_t));
                  for (i = 0; i < job[k].L.n; i++) out->r[at + i].gx_at += gat;    /* (offsets were into the thread's own words) */
                  gat += job[k].L.gx.n;
                }
              at += job[k].L.n;
            }
          out->n = out->cap = tot;
          out->gx.n = out->gx.cap = gw;
        }
    }
  for (k = 0; k < T; k++) rec_list_free(&job[k].L);
  return rc;
}

void dx_qv_index_free(dx_qv_index *x)
{ if (x == NULL) return;
  free(x->rec_off); free(x->hdr_off); free(x->seg); free(x->len); free(x->hdr4); free(x->prefix);
  free(x->gidx); free(x->gidx_off);
  memset(x, 0, sizeof(*x));
}

int dx_qv_walk(const uint8_t *img, size_t n, dx_qv_index *x) { return dx_qv_walk_indexed(img, n, x, 0); }

int dx_qv_walk_indexed(const uint8_t *img, size_t n, dx_qv_index *x, int want_index)
{ walk_tabs t;
  rec_list  L;
  size_t    at = 0;
  uint64_t  hat = 0, i;
  int       rc, well = 0, threads;

  if (img == NULL || x == NULL) return DX_E_ARG;
  memset(x, 0, sizeof(*x));
  memset(&t, 0, sizeof(t));
  memset(&L, 0, sizeof(L));
  if ((rc = dx_qv_read_head(img, n, x, &at)) != DX_OK) goto done;
  if ((rc = walk_tabs_build(&x->coding, &t)) != DX_OK) goto done;
  t.newv = x->newv; t.flip = x->flip; t.want_index = want_index != 0;

  /* the records: on several threads when the image is large (32-bit framing fields only: the older
     16-bit ones are too easily plausible), else -- and whenever the guesses do not chain up -- front to back */
  { const char *e = getenv("DEXGPU_WALK_THREADS");
    long cores = sysconf(_SC_NPROCESSORS_ONLN);
    threads = e ? atoi(e) : (int) (cores > 32 ? 32 : cores);
  }
  walk_mark(NULL);
  rc = DX_E_MISMATCH;
  if (threads > 1 && x->newv && n - at >= 4 * WALK_PIECE_MIN)
    rc = walk_parallel(&t, img, n, at, threads, &L);
  if (rc == DX_E_MISMATCH && dx_test_on("walk_require_parallel"))
    goto done;                                            /* (tests: no silent front-to-back walk) */
  if (rc == DX_E_MISMATCH)
    { rec_list_free(&L);
      rc = DX_OK;
      if (walk_span(&t, img, n, at, n, &L, &rc) == 0 && rc == DX_OK && at < n) rc = DX_E_FORMAT;
    }
  if (rc != DX_OK) goto done;

  x->n       = L.n;
  x->rec_off = malloc((L.n + 1) * sizeof(uint64_t));
  x->hdr_off = malloc((L.n + 1) * sizeof(uint64_t));
  x->seg     = malloc((L.n + 1) * 5 * sizeof(uint32_t));
  x->len     = malloc((L.n + 1) * sizeof(uint32_t));
  x->hdr4    = malloc((L.n + 1) * 4 * sizeof(int32_t));
  if (t.want_index) x->gidx_off = malloc((L.n + 1) * sizeof(uint64_t));
  if (!x->rec_off || !x->hdr_off || !x->seg || !x->len || !x->hdr4 || (t.want_index && !x->gidx_off)) { rc = DX_E_NOMEM; goto done; }
  if (t.want_index)                                       /* the group index: the threads' words are already in record order */
    { x->gidx = L.gx.w; L.gx.w = NULL;
      for (i = 0; i < L.n; i++)
        { x->gidx_off[i] = L.r[i].gx_at;
          x->gidx_none  += L.r[i].gx_none;
        }
      x->gidx_off[L.n] = L.gx.n;
      x->gidx_words    = L.gx.n;
    }
  for (i = 0; i < L.n; i++)
    { const walk_rec *r = &L.r[i];
      x->rec_off[i] = at;
      x->hdr_off[i] = hat;
      hat  += r->hdr_bytes;
      well += r->dwell;                                   /* undexqv.c:124-133: wells are a running sum */
      x->len[i] = r->len;
      x->hdr4[4*i] = well; x->hdr4[4*i+1] = r->beg; x->hdr4[4*i+2] = r->end; x->hdr4[4*i+3] = r->qv;
      memcpy(x->seg + 5*i, r->seg, sizeof(r->seg));
      at += (size_t) r->hdr_bytes + r->seg[0] + r->seg[1] + r->seg[2] + r->seg[3] + r->seg[4];
    }
  x->rec_off[L.n] = at;
  x->hdr_off[L.n] = hat;
  walk_mark("index assembled");

done:
  rec_list_free(&L);
  walk_tabs_free(&t);
  if (rc != DX_OK) dx_qv_index_free(x);
  return rc;
}
