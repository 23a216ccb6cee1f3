/*
 * dx_file_pack2.c -- the file drivers of the 2-bit kinds: dexta / dexar of a whole text, of one that arrives in pieces, and on several
 * GPUs; undexta / undexar of a whole image and of one that arrives in pieces.  dx_files.h has what the other drivers take from here.
 */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dexgpu.h"
#include "dx_env.h"
#include "dx_host.h"
#include "dx_crew.h"
#include "dx_files.h"

/* ==========================================================================================
 *  dexta / dexar
 * ========================================================================================== */

/* A header line with the end of the file right behind it is an error for the reference unless it is the file's only line
   (dx_index_seq has the story): such a text goes to the host index, which knows; the device front end takes the empty read. */
static int ends_with_a_header(const uint8_t *text, size_t n)
{ size_t at;
  if (n < 2 || text[n - 1] != '\n') return 0;
  for (at = n - 1; at > 0 && text[at - 1] != '\n'; at--) ;
  return at > 0 && text[at] == '>';
}

/* how much text the device packs at once: DEXGPU_TEXT_BUDGET (bytes) when set, else all of it (0) unless the text, its packed
   image and the index do not fit what is free */
static size_t pack2_cap(dx_ctx *ctx, size_t n)
{ uint64_t fr = 0, all = 0;
  size_t   cap;
  if (dxf_budget_env(n, 65536u, &cap)) return cap;
  if (dx_mem_info(ctx, &fr, &all) != DX_OK || fr == 0) return 0;
  return 1.35 * (double) n > 0.9 * (double) fr ? (size_t) (0.6 * (double) fr) : 0;
}

void dxf_seq_index_free(seq_index *ix)
{ free(ix->off); free(ix->hoff); free(ix->ooff); free(ix->tlen); free(ix->nsym); free(ix->hdr4); free(ix->cnr4); free(ix->blob); }

int dxf_seq_index_host(seq_index *ix, int arrow, const uint8_t *text, size_t n, uint64_t *errline, int *errcode)
{ const int rc = dx_index_seq(arrow, text, n, 0, NULL, NULL, NULL, NULL, NULL, &ix->cnt, &ix->plen, errline, errcode);
  if (rc != DX_OK) return rc;
  ix->off  = malloc((ix->cnt + 1) * sizeof(*ix->off));
  ix->tlen = malloc((ix->cnt + 1) * sizeof(*ix->tlen));
  ix->nsym = malloc((ix->cnt + 1) * sizeof(*ix->nsym));
  ix->hdr4 = malloc((ix->cnt + 1) * 4 * sizeof(*ix->hdr4));
  ix->cnr4 = malloc((ix->cnt + 1) * 4 * sizeof(*ix->cnr4));
  if (!ix->off || !ix->tlen || !ix->nsym || !ix->hdr4 || !ix->cnr4) return DX_E_NOMEM;
  return dx_index_seq(arrow, text, n, ix->cnt, ix->off, ix->tlen, ix->nsym, ix->hdr4, ix->cnr4, &ix->cnt, &ix->plen, errline, errcode);
}

/* the framing bytes of every header, *well the last record's well before and after (the record framing codes differences,
   dexta.c:187-193), and the records' places in an image whose first record stands at `at` */
static int seq_index_frame(seq_index *ix, int arrow, int32_t *well, size_t at)
{ uint64_t i;
  int      rc;
  ix->hoff = malloc((ix->cnt + 1) * sizeof(*ix->hoff));
  ix->ooff = malloc((ix->cnt + 1) * sizeof(*ix->ooff));
  ix->blob = malloc(dx_frame_bound(ix->hdr4, ix->cnt, 0, arrow) + 16);
  if (!ix->hoff || !ix->ooff || !ix->blob) return DX_E_NOMEM;
  rc = dx_frame_headers(ix->hdr4, ix->cnr4, ix->cnt, arrow, well, ix->blob, ix->hoff);
  if (rc != DX_OK) return rc;
  for (i = 0; i < ix->cnt; i++)
    { ix->ooff[i] = at;
      at += (size_t) (ix->hoff[i+1] - ix->hoff[i]) + (((size_t) ix->nsym[i] + 3) >> 2);
    }
  ix->ooff[ix->cnt] = ix->total = at;
  return DX_OK;
}

/* key, prefix length, prefix (2 + 4 + plen bytes): dexta.c:124-129 */
static void pack2_head(uint8_t *img, const uint8_t *text, size_t plen)
{ const uint16_t key = 0x55aa;
  const int32_t  pl  = (int32_t) plen;
  memcpy(img, &key, 2);
  memcpy(img + 2, &pl, 4);
  memcpy(img + 6, text, plen);
}

/* Reads [i0, i1) of a host index: their text up, with offsets counted from the range's first byte; packed; the records down to their
   places in img.  The device buffers live for the call. */
static int pack2_range(dx_ctx *ctx, int arrow, const uint8_t *text, const seq_index *ix, uint64_t i0, uint64_t i1, uint8_t *img)
{ dpool     pool = { {0}, 0, ctx };
  const uint64_t m = i1 - i0;
  uint64_t  i, *roff, *rhoff, *rooff;
  void     *d_text, *d_off, *d_tlen, *d_nsym, *d_hdr, *d_hoff, *d_out, *d_ooff;
  int       rc;
  if (m == 0) return DX_OK;
  roff = malloc((3 * m + 1) * sizeof(*roff));
  if (roff == NULL) return DX_E_NOMEM;
  rooff = roff + m; rhoff = rooff + m;
  { const uint64_t t0 = ix->off[i0], t1 = ix->off[i1 - 1] + ix->tlen[i1 - 1];
    const uint64_t h0 = ix->hoff[i0], o0 = ix->ooff[i0], obytes = ix->ooff[i1] - o0;
    for (i = 0; i < m; i++)
      { roff[i]  = ix->off[i0 + i] - t0;
        rhoff[i] = ix->hoff[i0 + i] - h0;
        rooff[i] = ix->ooff[i0 + i] - o0;
      }
    rhoff[m] = ix->hoff[i1] - h0;
    TRY(dupload(&pool, text + t0, (size_t) (t1 - t0), &d_text));
    TRY(dupload(&pool, roff, m * 8, &d_off));
    TRY(dupload(&pool, ix->tlen + i0, m * 4, &d_tlen));
    TRY(dupload(&pool, ix->nsym + i0, m * 4, &d_nsym));
    TRY(dupload(&pool, ix->blob + h0, (size_t) rhoff[m], &d_hdr));
    TRY(dupload(&pool, rhoff, (m + 1) * 8, &d_hoff));
    TRY(dupload(&pool, rooff, m * 8, &d_ooff));
    TRY(dalloc(&pool, (size_t) obytes, &d_out));
    TRY(dx_pack2_encode(ctx, arrow ? DX_ALPHA_ARROW : DX_ALPHA_BASES, d_text, d_off, d_tlen, d_nsym, m,
                        d_hdr, d_hoff, d_out, d_ooff));
    TRY(dx_d2h(ctx, img + o0, d_out, (size_t) obytes));
  }
done:
  dfree_all(&pool);
  free(roff);
  return rc;
}

/* a slice of whole reads from i0 on: as many as make at most `cap` bytes of text, and one at least */
static uint64_t pack2_slice_end(const seq_index *ix, uint64_t i0, size_t cap)
{ uint64_t i1 = i0 + 1;
  while (i1 < ix->cnt && (size_t) ix->off[i1] + ix->tlen[i1] - (size_t) ix->off[i0] <= cap) i1++;
  return i1;
}

/* One piece of a .fasta / .arrow text -- whole records, the first of them the file's first (`first`: the image then begins with the
   key and the name prefix, dexta.c:124-129) or a later one; *well: the last record's well before and after (the record framing
   codes differences, dexta.c:187-193). */
static int pack2_piece(dx_ctx *ctx, int arrow, const uint8_t *text, size_t n, int first, int32_t *well,
                       uint8_t **out, size_t *out_len, uint64_t *errline, int *errcode)
{ dpool     pool = { {0}, 0, ctx };
  seq_index ix;
  int32_t   lwell = *well;
  uint8_t  *img = NULL;
  void     *d_text, *d_off = NULL, *d_tlen = NULL, *d_nsym = NULL, *d_hdr, *d_hoff, *d_out, *d_ooff;
  uint64_t  i0, i1;
  size_t    sliced;
  int       rc;

  if (ctx == NULL || out == NULL || out_len == NULL) return DX_E_ARG;
  *out = NULL; *out_len = 0;
  memset(&ix, 0, sizeof(ix));

  /* A text that does not fit the device beside its packed image (or DEXGPU_TEXT_BUDGET): indexed on the host, then slices of
     whole reads -- upload, pack, the slice's records into the image (the reference reads record after record,
     dexta.c:104-205). */
  sliced = pack2_cap(ctx, n);
  /* index: on the GPU for large images (newline scan, record extents there; only header lines come
     back), on the host for small ones and for anything the GPU front end rejects (exact message) */
  if (!sliced && n >= DX_GPU_INDEX_MIN && !dx_test_on("host_index") && !ends_with_a_header(text, n))
    { uint64_t *go = NULL; uint32_t *gt = NULL, *gs = NULL;
      TRY(dupload(&pool, text, n, &d_text));
      rc = dx_index_seq_device(ctx, arrow, d_text, n, &go, &gt, &gs, &ix.cnt, &ix.hdr4, &ix.cnr4, &ix.plen, errline, errcode);
      if (rc == DX_OK)
        { if (dadopt(&pool, go) | dadopt(&pool, gt) | dadopt(&pool, gs)) { rc = DX_E_NOMEM; goto done; }      /* (each of them, whatever becomes of the others) */
          d_off = go; d_tlen = gt; d_nsym = gs;
          ix.nsym = malloc((ix.cnt + 1) * sizeof(*ix.nsym));
          if (!ix.nsym) { rc = DX_E_NOMEM; goto done; }
          TRY(dx_d2h(ctx, ix.nsym, d_nsym, ix.cnt * 4));
        }
      else if (rc != DX_E_FORMAT)
        goto done;
    }
  if (d_off == NULL) TRY(dxf_seq_index_host(&ix, arrow, text, n, errline, errcode));
  TRY(seq_index_frame(&ix, arrow, &lwell, first ? 2 + 4 + ix.plen : 0));

  img = malloc(ix.total + 16);
  if (!img) { rc = DX_E_NOMEM; goto done; }
  if (first) pack2_head(img, text, ix.plen);

  if (d_off != NULL && ix.cnt > 0)                       /* indexed on the device: text and index are there, nothing to rebase */
    { TRY(dupload(&pool, ix.blob, (size_t) ix.hoff[ix.cnt], &d_hdr));
      TRY(dupload(&pool, ix.hoff, (ix.cnt + 1) * 8, &d_hoff));
      TRY(dupload(&pool, ix.ooff, ix.cnt * 8, &d_ooff));
      TRY(dalloc(&pool, ix.total, &d_out));
      TRY(dx_pack2_encode(ctx, arrow ? DX_ALPHA_ARROW : DX_ALPHA_BASES, d_text, d_off, d_tlen, d_nsym, ix.cnt,
                          d_hdr, d_hoff, d_out, d_ooff));
      TRY(dx_d2h(ctx, img + ix.ooff[0], (uint8_t *) d_out + ix.ooff[0], ix.total - (size_t) ix.ooff[0]));
    }
  else if (d_off == NULL)
    for (i0 = 0; i0 < ix.cnt; i0 = i1)                   /* indexed here: all reads at once, or slice after slice */
      { i1 = sliced ? pack2_slice_end(&ix, i0, sliced) : ix.cnt;
        TRY(pack2_range(ctx, arrow, text, &ix, i0, i1, img));
      }
  *out = img; *out_len = ix.total; img = NULL;
  *well = lwell;
  rc = DX_OK;

done:
  dfree_all(&pool);
  dxf_seq_index_free(&ix);
  free(img);
  return rc;
}

int dx_file_pack2(dx_ctx *ctx, int arrow, const uint8_t *text, size_t n,
                  uint8_t **out, size_t *out_len, uint64_t *errline, int *errcode)
{ int32_t well = 0;
  if (ctx == NULL || out == NULL || out_len == NULL) return DX_E_ARG;
  return pack2_piece(ctx, arrow, text, n, 1, &well, out, out_len, errline, errcode);
}

/* dexta / dexar of a text that arrives in pieces -- a pipe, or a file too large to hold: the reference reads record after record
   (dexta.c:104-205, dexar.c:103-211) and never holds more than one.  Here: `chunk` bytes at a time from rd(); a piece is cut in
   front of the buffer's last header but one (so that what stays behind begins with a header and holds another: the last piece,
   which the end of the input makes, then tells a lone last header -- the reference's "too long" -- from a file of one header), the
   piece's records packed on the device like a whole file's, its bytes handed to the sink in file order, the rest moved to the
   buffer's front.  Memory: the buffer (chunk + a record or two) and a piece's image. */
/* line ends in n bytes, eight at a time (a text of gigabytes byte by byte is seconds) */
static uint64_t count_newlines(const uint8_t *p, size_t n)
{ uint64_t c = 0;
  size_t   i = 0;
  for (; i + 8 <= n; i += 8)
    { uint64_t w, x, t;
      memcpy(&w, p + i, 8);
      x = w ^ 0x0a0a0a0a0a0a0a0aull;
      t = (((x & 0x7f7f7f7f7f7f7f7full) + 0x7f7f7f7f7f7f7f7full) | x) & 0x8080808080808080ull;     /* 0x80 in every byte that is no line end */
      c += 8u - (uint64_t) __builtin_popcountll(t);
    }
  for (; i < n; i++) c += p[i] == '\n';
  return c;
}

/* Reading ahead: a helper thread takes the next block from the caller's read function while the last one is on the device -- a pipe
   hands over 2 GB/s at best, and a chunk's packing is no faster than that: one after the other they add up (dexta -i of 4 GB: 3.1 s),
   side by side the slower one counts.  Two blocks of RA_BLOCK bytes; ra_read() gives their bytes out in order. */
#define RA_BLOCK ((size_t) 32 << 20)
typedef struct
  { dx_read_fn      rd;
    void           *user;
    uint8_t        *blk[2];
    size_t          len[2], pos;
    int             full[2], cur, eof, err, stop, threaded;
    pthread_mutex_t mx;
    pthread_cond_t  cv;
    pthread_t       th;
  } readahead;

static void *ra_main(void *arg)
{ readahead *r = arg;
  int slot = 0;
  for (;;)
    { size_t n = 0;
      int    bad = 0;
      pthread_mutex_lock(&r->mx);
      while (r->full[slot] && !r->stop) pthread_cond_wait(&r->cv, &r->mx);
      if (r->stop) { pthread_mutex_unlock(&r->mx); break; }
      pthread_mutex_unlock(&r->mx);
      while (n < RA_BLOCK)
        { const long k = r->rd(r->user, r->blk[slot] + n, RA_BLOCK - n);
          if (k < 0) { bad = 1; break; }
          if (k == 0) break;
          n += (size_t) k;
        }
      pthread_mutex_lock(&r->mx);
      r->len[slot] = n; r->full[slot] = 1;
      if (bad) r->err = 1;
      if (n < RA_BLOCK) r->eof = 1;
      pthread_cond_broadcast(&r->cv);
      pthread_mutex_unlock(&r->mx);
      if (n < RA_BLOCK) break;
      slot ^= 1;
    }
  return NULL;
}

static void ra_begin(readahead *r, dx_read_fn rd, void *user)
{ memset(r, 0, sizeof(*r));
  r->rd = rd; r->user = user;
  r->blk[0] = malloc(RA_BLOCK); r->blk[1] = malloc(RA_BLOCK);
  if (r->blk[0] != NULL && r->blk[1] != NULL && !dx_test_on("no_readahead"))
    { pthread_mutex_init(&r->mx, NULL);
      pthread_cond_init(&r->cv, NULL);
      r->threaded = pthread_create(&r->th, NULL, ra_main, r) == 0;
    }
}

static long ra_read(void *arg, void *buf, size_t want)
{ readahead *r = arg;
  size_t got = 0;
  if (!r->threaded) return r->rd(r->user, buf, want);
  while (got < want)
    { int have, err;
      pthread_mutex_lock(&r->mx);
      while (!r->full[r->cur] && !r->eof && !r->err) pthread_cond_wait(&r->cv, &r->mx);
      have = r->full[r->cur]; err = r->err;
      pthread_mutex_unlock(&r->mx);
      if (err) return -1;
      if (!have) break;                                /* the input's end, and nothing left in this block (blocks come in turn) */
      { const size_t k = r->len[r->cur] - r->pos < want - got ? r->len[r->cur] - r->pos : want - got;
        memcpy((uint8_t *) buf + got, r->blk[r->cur] + r->pos, k);
        got += k; r->pos += k;
      }
      if (r->pos == r->len[r->cur])
        { const int last = r->len[r->cur] < RA_BLOCK;
          pthread_mutex_lock(&r->mx);
          r->full[r->cur] = 0;
          pthread_cond_broadcast(&r->cv);
          pthread_mutex_unlock(&r->mx);
          r->cur ^= 1; r->pos = 0;
          if (last) break;
        }
    }
  return (long) got;
}

static void ra_end(readahead *r)
{ if (r->threaded)
    { pthread_mutex_lock(&r->mx);
      r->stop = 1;
      pthread_cond_broadcast(&r->cv);
      pthread_mutex_unlock(&r->mx);
      pthread_join(r->th, NULL);
      pthread_cond_destroy(&r->cv);
      pthread_mutex_destroy(&r->mx);
    }
  free(r->blk[0]); free(r->blk[1]);
}

int dx_file_pack2_stream(dx_ctx *ctx, int arrow, dx_read_fn rd_, void *ruser_, size_t chunk,
                         dx_sink_fn sink, void *suser, size_t *out_len, uint64_t *errline, int *errcode)
{ uint8_t *buf = NULL;
  readahead ra;
  dx_read_fn rd = ra_read;
  void      *ruser = &ra;
  size_t   cap, have = 0, total = 0;
  uint64_t lines = 0;
  int32_t  well = 0;
  int      eof = 0, first = 1, rc = DX_OK;

  if (ctx == NULL || rd_ == NULL || sink == NULL) return DX_E_ARG;
  if (chunk == 0) chunk = (size_t) dx_test_num("stream_chunk", (long long) 256 << 20);
  if (chunk < 4096) chunk = 4096;
  cap = chunk + 65536;
  buf = malloc(cap);
  if (buf == NULL) return DX_E_NOMEM;
  ra_begin(&ra, rd_, ruser_);
  if (out_len) *out_len = 0;
  for (;;)
    { size_t cut, k, heads = 0;
      while (!eof && have < chunk)
        { const long got = rd(ruser, buf + have, chunk - have);
          if (got < 0) { rc = DX_E_IO; goto done; }
          if (got == 0) eof = 1;
          have += (size_t) got;
        }
      cut = have;
      if (!eof)                                        /* the last header line but one that is not the buffer's first line -- nor stands */
        { int good = 0;                                /* behind another header line: a piece that ENDS in a header reads like a file that does */
          for (k = have; k > 1 && !good; k--)
            if (buf[k - 1] == '>' && buf[k - 2] == '\n')
              { size_t q = k - 2;                       /* the line in front of this header begins at q */
                while (q > 0 && buf[q - 1] != '\n') q--;
                heads++;
                if (heads >= 2 && buf[q] != '>') { cut = k - 1; good = 1; }
              }
          if (!good)                                   /* a record (or two) larger than the chunk: more of it */
            { uint8_t *nb;
              chunk += chunk;
              nb = realloc(buf, chunk + 65536);
              if (nb == NULL) { rc = DX_E_NOMEM; goto done; }
              buf = nb; cap = chunk + 65536;
              continue;
            }
        }
      if (cut > 0 || first)
        { uint8_t *img = NULL;
          size_t   il = 0;
          uint64_t el = 0;
          rc = pack2_piece(ctx, arrow, buf, cut, first, &well, &img, &il, &el, errcode);
          if (rc != DX_OK)
            { if (errline) *errline = el ? lines + el : 0;
              goto done;
            }
          if (il > 0 && sink(suser, img, il, total)) { free(img); rc = DX_E_IO; goto done; }
          free(img);
          total += il;
          lines += count_newlines(buf, cut);
          first = 0;
        }
      memmove(buf, buf + cut, have - cut);
      have -= cut;
      if (eof && have == 0) break;
    }
  if (out_len) *out_len = total;
done:
  ra_end(&ra);
  free(buf);
  return rc;
}

/* ==========================================================================================
 *  dexta / dexar of one file on several GPUs: reads are independent, so contiguous read ranges
 *  (balanced by text bytes) go to one host thread per context; nothing is exchanged -- the only
 *  cross-record datum, the previous well of a range's first read, is known from the host index.
 *  The threads are a crew of one phase (dx_crew.h): all of them exist, or no range is packed.
 * ========================================================================================== */
typedef struct
  { dx_ctx          *ctx;
    int              arrow, rc;
    const uint8_t   *text;
    const seq_index *ix;
    uint8_t         *img;
    uint64_t         lo, hi;                  /* reads [lo, hi) */
  } p2_job;

static void p2_range(void *arg)
{ p2_job *j = arg;
  j->rc = pack2_range(j->ctx, j->arrow, j->text, j->ix, j->lo, j->hi, j->img);
}

static const dx_crew_phase p2_phases[] = { { p2_range, NULL } };

int dx_file_pack2_sharded(dx_ctx **ctxs, int nctx, int arrow, const uint8_t *text, size_t n,
                          uint8_t **out, size_t *out_len, uint64_t *errline, int *errcode)
{ seq_index ix;
  int32_t   lwell = 0;
  uint8_t  *img = NULL;
  p2_job   *jobs = NULL;
  int       rc, k;

  if (ctxs == NULL || nctx < 1 || out == NULL || out_len == NULL) return DX_E_ARG;
  if (nctx == 1) return dx_file_pack2(ctxs[0], arrow, text, n, out, out_len, errline, errcode);
  *out = NULL; *out_len = 0;
  memset(&ix, 0, sizeof(ix));

  TRY(dxf_seq_index_host(&ix, arrow, text, n, errline, errcode));
  TRY(seq_index_frame(&ix, arrow, &lwell, 2 + 4 + ix.plen));             /* one pass: well deltas chain over the whole file */
  img = malloc(ix.total + 16);
  if (!img) { rc = DX_E_NOMEM; goto done; }
  pack2_head(img, text, ix.plen);

  jobs = calloc((size_t) nctx, sizeof(*jobs));
  if (!jobs) { rc = DX_E_NOMEM; goto done; }
  { uint64_t lo = 0;
    const uint64_t tbytes = ix.cnt ? ix.off[ix.cnt - 1] + ix.tlen[ix.cnt - 1] - ix.off[0] : 0;
    for (k = 0; k < nctx; k++)
      { uint64_t hi = lo;
        const uint64_t want = ix.off[0] + tbytes / (uint64_t) nctx * (uint64_t) (k + 1);
        if (k == nctx - 1) hi = ix.cnt;
        else while (hi < ix.cnt && ix.off[hi] < want) hi++;
        jobs[k].ctx = ctxs[k]; jobs[k].arrow = arrow; jobs[k].text = text; jobs[k].ix = &ix; jobs[k].img = img;
        jobs[k].lo = lo; jobs[k].hi = hi;
        lo = hi;
      }
  }
  if (dx_crew_run(nctx, p2_phases, 1, jobs, sizeof(*jobs), NULL)) { rc = DX_E_NOMEM; goto done; }      /* (all the ranges, or none) */
  rc = DX_OK;
  for (k = 0; k < nctx; k++)
    if (jobs[k].rc != DX_OK) { rc = jobs[k].rc; break; }
  if (rc == DX_OK)
    { *out = img; *out_len = ix.total; img = NULL; }

done:
  dxf_seq_index_free(&ix);
  free(img); free(jobs);
  return rc;
}

/* ==========================================================================================
 *  undexta / undexar
 * ========================================================================================== */
/* One path: the image is walked on the host (dxf_u2_walk), the text laid out (dxf_u2_layout), and dxf_unpack2_slices decodes it slice by slice
   of whole reads -- the whole text is the case of one slice.  What becomes of a slice is its hook's business (slice_fn): out to the
   caller (dxf_slice_deliver), compared (verify_slice), hashed (digest_slice). */
typedef struct { const uint8_t *p; size_t n, at; int bad; } rsrc;

static void rd(rsrc *r, void *dst, size_t k)
{ if (r->at + k > r->n) { r->bad = 1; memset(dst, 0, k); r->at = r->n; return; }
  memcpy(dst, r->p + r->at, k);
  r->at += k;
}
static int32_t  rd_i32(rsrc *r, int flip) { uint32_t v; rd(r, &v, 4); return (int32_t) (flip ? flip32(v) : v); }
static uint16_t rd_u16(rsrc *r, int flip) { uint16_t v; rd(r, &v, 2); return flip ? flip16(v) : v; }

void dxf_u2_index_free(u2_index *x)
{ free(x->ioff); free(x->hat); free(x->nsym); free(x->hd.p); free(x->hdr4); free(x->cnr4); }

int dxf_u2_header(tbuf *b, int arrow, const char *name, int well, int beg, int end, int qv, const uint16_t *cnr)
{ int rc, k;
  if ((rc = dxf_tb_room(b, strlen(name) + 160)) != DX_OK) return rc;
  if (arrow)                                              /* undexar.c:199-203 */
    { float snr[4];
      for (k = 0; k < 4; k++) snr[k] = (float) (cnr[k] / 100.);
      b->len += (size_t) sprintf(b->p + b->len, "%s/%d/%d_%d SN=%.2f,%.2f,%.2f,%.2f\n", name, well, beg, end, snr[0], snr[1], snr[2], snr[3]);
    }
  else                                                    /* undexta.c:242 */
    b->len += (size_t) sprintf(b->p + b->len, "%s/%d/%d_%d RQ=0.%d\n", name, well, beg, end, qv);
  return DX_OK;
}

#define U2_NOT_YET 1               /* (a piece of an image that arrives in pieces: its head is not all here yet; nothing consumed) */

/* mode: DX_LETTERS_LOWER / _UPPER (dexta images) or _ARROW (dexar images); st: the image arrives in pieces (else NULL) */
int dxf_u2_walk(int mode, const uint8_t *img, size_t n, u2_state *st, u2_index *x)
{ rsrc      r = { img, n, 0, 0 };
  uint64_t  cnt = 0, cap = 0;
  uint16_t  key;
  int       flip, newv, well = 0, rc = DX_OK, arrow = (mode == DX_LETTERS_ARROW);
  int32_t   plen;
  char     *name = NULL;

  memset(x, 0, sizeof(*x));
  if (st != NULL) st->consumed = 0;
  if (st != NULL && st->started)                          /* a later piece: records from its first byte on */
    { flip = st->flip; newv = st->newv; plen = st->plen; well = st->well;
      name = malloc((size_t) plen + 1);
      if (!name) return DX_E_NOMEM;
      memcpy(name, st->name, (size_t) plen + 1);
    }
  else
    { rd(&r, &key, 2);                                    /* undexta.c:138-159, undexar.c:136-145 */
      if (r.bad) return st != NULL && st->more ? U2_NOT_YET : DX_E_FORMAT;
      if (key == 0x55aa)               { flip = 0; newv = 1; }
      else if (key == 0xaa55)          { flip = 1; newv = 1; }
      else if (!arrow && key == 0x33cc) { flip = 0; newv = 0; }
      else if (!arrow && key == 0xcc33) { flip = 1; newv = 0; }
      else return DX_E_FORMAT;

      plen = rd_i32(&r, flip);                            /* undexta.c:161-169 */
      if (r.bad) return st != NULL && st->more ? U2_NOT_YET : DX_E_FORMAT;
      if (plen < 0) return DX_E_FORMAT;
      if ((size_t) plen > n - r.at) return st != NULL && st->more && plen < (1 << 24) ? U2_NOT_YET : DX_E_FORMAT;
      name = malloc((size_t) plen + 1);
      if (!name) return DX_E_NOMEM;
      rd(&r, name, (size_t) plen);
      name[plen] = '\0';
      if (st != NULL)
        { st->name = malloc((size_t) plen + 1);
          if (st->name == NULL) { free(name); return DX_E_NOMEM; }
          memcpy(st->name, name, (size_t) plen + 1);
          st->started = 1; st->flip = flip; st->newv = newv; st->plen = plen;
          st->consumed = r.at;
        }
    }

  while (r.at < r.n)                                      /* undexta.c:175-271: walk the records */
    { uint8_t  byte;
      int      beg, end, qv = 0, k;
      uint16_t cnr[4] = { 0, 0, 0, 0 };
      uint32_t rlen;
      size_t   clen;
      const size_t rec_at = r.at;
      const int    well_was = well;

      rd(&r, &byte, 1);
      while (byte == 255 && !r.bad)
        { well += 255;
          rd(&r, &byte, 1);
        }
      well += byte;
      if (newv)
        { beg = rd_i32(&r, flip);
          end = rd_i32(&r, flip);
          if (arrow) for (k = 0; k < 4; k++) cnr[k] = rd_u16(&r, flip);
          else       qv = rd_i32(&r, flip);
        }
      else
        { beg = rd_u16(&r, flip); end = rd_u16(&r, flip); qv = rd_u16(&r, flip); }
      if (r.bad && st != NULL && st->more)                /* the piece ends inside this record's head: the next piece has it whole */
        { r.at = rec_at; r.bad = 0; well = well_was; break; }
      if (r.bad || end < beg || (int64_t) end - (int64_t) beg > 0x7fffffff)   /* (hostile headers: no int overflow) */
        { rc = DX_E_FORMAT; goto done; }
      rlen = (uint32_t) ((int64_t) end - (int64_t) beg);
      clen = ((size_t) rlen + 3) >> 2;
      if (r.at + clen > r.n)
        { if (st != NULL && st->more) { r.at = rec_at; well = well_was; break; }     /* ... or inside its bases */
          rc = DX_E_FORMAT; goto done;
        }

      if (cnt == cap)
        { void *t;                                        /* a failed realloc leaves the old block to the caller's dxf_u2_index_free */
          cap  = cap ? 2 * cap : 1024;
          if ((t = realloc(x->ioff, cap * sizeof(*x->ioff))) == NULL) { rc = DX_E_NOMEM; goto done; }
          x->ioff = t;
          if ((t = realloc(x->hat, (cap + 1) * sizeof(*x->hat))) == NULL) { rc = DX_E_NOMEM; goto done; }
          x->hat = t;
          if ((t = realloc(x->nsym, cap * sizeof(*x->nsym))) == NULL) { rc = DX_E_NOMEM; goto done; }
          x->nsym = t;
          if ((t = realloc(x->hdr4, cap * 4 * sizeof(*x->hdr4))) == NULL) { rc = DX_E_NOMEM; goto done; }
          x->hdr4 = t;
          if ((t = realloc(x->cnr4, cap * 4 * sizeof(*x->cnr4))) == NULL) { rc = DX_E_NOMEM; goto done; }
          x->cnr4 = t;
        }
      x->hat[cnt] = x->hd.len;
      if ((rc = dxf_u2_header(&x->hd, arrow, name, well, beg, end, qv, cnr)) != DX_OK) goto done;

      x->ioff[cnt] = r.at;
      x->nsym[cnt] = rlen;
      x->hdr4[4*cnt] = well; x->hdr4[4*cnt + 1] = beg; x->hdr4[4*cnt + 2] = end; x->hdr4[4*cnt + 3] = qv;
      memcpy(x->cnr4 + 4*cnt, cnr, sizeof(cnr));
      r.at += clen;
      cnt  += 1;
    }
  if (cnt) x->hat[cnt] = x->hd.len;
  x->cnt = cnt; x->at = r.at; x->well = well;
done:
  free(name);
  return rc;
}

/* the text's layout for a line width: header line, wrapped letters, read after read; ooff[i]: where read i's letters begin */
size_t dxf_u2_layout(const u2_index *x, uint32_t width, uint64_t *ooff)
{ size_t   total = 0;
  uint64_t i;
  for (i = 0; i < x->cnt; i++)
    { const size_t L = x->nsym[i];
      total  += (size_t) (x->hat[i+1] - x->hat[i]);
      ooff[i] = total;
      total  += L + (L + width - 1) / width;
    }
  return total;
}

/* A walked image's text made in slices of whole reads, at most `cap` bytes of text each (0: the whole text, one slice), the image resident
   (a quarter of the text); every slice goes to `deliver` before the next one is made (the reference writes read after read,
   undexta.c:175-271).  The only decode of a .dexta / .dexar image in this file. */
int dxf_unpack2_slices(dx_ctx *ctx, int mode, const uint8_t *img, size_t n, uint32_t width, const u2_index *x, const hdr_patch *h,
                          size_t cap, slice_fn deliver, void *arg)
{ dpool     pool = { {0}, 0, ctx };
  const uint64_t cnt = x->cnt;
  uint64_t *rel = NULL, i, i0, i1, most = 0;
  size_t    tmax = 0;
  void     *d_in, *d_ioff, *d_nsym, *d_out, *d_ooff;
  int       rc;
  for (i0 = 0; i0 < cnt; i0 = i1)
    { i1 = dxf_text_slice_end(h, i0, cap);
      if (text_at(h, i1) - text_at(h, i0) > tmax) tmax = text_at(h, i1) - text_at(h, i0);
      if (i1 - i0 > most) most = i1 - i0;
    }
  rel = malloc((most + 1) * sizeof(*rel));
  if (rel == NULL) return DX_E_NOMEM;
  rc = dupload(&pool, img, n, &d_in);
  if (rc == DX_OK) rc = dupload(&pool, x->ioff, cnt * 8, &d_ioff);
  if (rc == DX_OK) rc = dupload(&pool, x->nsym, cnt * 4, &d_nsym);
  if (rc == DX_OK) rc = dalloc(&pool, (most + 1) * 8, &d_ooff);
  if (rc == DX_OK) rc = dalloc(&pool, tmax, &d_out);
  for (i0 = 0; i0 < cnt && rc == DX_OK; i0 = i1)
    { const size_t t0 = text_at(h, i0);
      i1 = dxf_text_slice_end(h, i0, cap);
      for (i = i0; i < i1; i++) rel[i - i0] = h->ooff[i] - t0;
      rc = dx_h2d(ctx, d_ooff, rel, (i1 - i0) * 8);
      if (rc == DX_OK)
        rc = dx_pack2_decode(ctx, mode, d_in, (const uint64_t *) d_ioff + i0, (const uint32_t *) d_nsym + i0, i1 - i0, width, d_out, d_ooff);
      if (rc == DX_OK)
        rc = deliver(arg, d_out, i0, i1, t0, text_at(h, i1) - t0);
    }
  dfree_all(&pool);
  free(rel);
  return rc == SLICE_STOP ? DX_OK : rc;
}

/* out != NULL: the text in memory, else through the sink */
static int unpack2_core(dx_ctx *ctx, int mode, const uint8_t *img, size_t n, uint32_t width,
                        uint8_t **out, dx_sink_fn sink, void *user, size_t *out_len, u2_state *st)
{ u2_index  x;
  uint64_t  cnt, *ooff = NULL;
  int       rc;
  uint8_t  *res = NULL;
  size_t    total = 0;

  if (ctx == NULL || (out == NULL && sink == NULL) || out_len == NULL || img == NULL) return DX_E_ARG;
  if (width == 0) return DX_E_ARG;
  if (out) *out = NULL;
  *out_len = 0;

  rc = dxf_u2_walk(mode, img, n, st, &x);
  if (rc == U2_NOT_YET) { dxf_u2_index_free(&x); return DX_OK; }
  if (rc != DX_OK) goto done;
  cnt = x.cnt;
  ooff = malloc((cnt + 1) * sizeof(*ooff));
  if (ooff == NULL) { rc = DX_E_NOMEM; goto done; }
  total = dxf_u2_layout(&x, width, ooff);                     /* output layout: header line, wrapped text */
  if (out)
    { res = malloc(total + 16);
      if (!res) { rc = DX_E_NOMEM; goto done; }
    }

  if (cnt > 0)                                            /* (an image without records: nothing for the device) */
    { /* All of the text at once, or, when it does not fit the device beside the image (or DEXGPU_TEXT_BUDGET says so), in slices
         of whole reads, every slice's text out before the next one's is made. */
      hdr_patch h = { cnt, ooff, x.hat, x.hd.p, sink, user, 0, total };
      slice_out so = { ctx, &h, res };
      TRY(dxf_unpack2_slices(ctx, mode, img, n, width, &x, &h, dxf_out_cap(ctx, n, total, cnt), dxf_slice_deliver, &so));
    }
  if (out) { *out = res; res = NULL; }
  *out_len = total;
  if (st != NULL) { st->well = x.well; st->consumed = x.at; }
  rc = DX_OK;

done:
  dxf_u2_index_free(&x);
  free(ooff); free(res);
  return rc;
}

int dx_file_unpack2(dx_ctx *ctx, int mode, const uint8_t *img, size_t n, uint32_t width, uint8_t **out, size_t *out_len)
{ if (out == NULL) return DX_E_ARG;
  return unpack2_core(ctx, mode, img, n, width, out, NULL, NULL, out_len, NULL);
}

int dx_file_unpack2_to(dx_ctx *ctx, int mode, const uint8_t *img, size_t n, uint32_t width,
                       dx_sink_fn sink, void *user, size_t *out_len)
{ if (sink == NULL) return DX_E_ARG;
  return unpack2_core(ctx, mode, img, n, width, NULL, sink, user, out_len, NULL);
}

/* undexta / undexar of an image that arrives in pieces (a pipe: undexta -i, undexta.c:175-271 reads record after record): `chunk`
   bytes at a time from rd(), the whole records among them unpacked on the device, their text handed to the sink in file order, the
   rest (a record the chunk cuts) moved to the buffer's front.  The same bytes as dx_file_unpack2 of the whole image. */

int dx_file_unpack2_stream(dx_ctx *ctx, int mode, dx_read_fn rd_, void *ruser, size_t chunk, uint32_t width,
                           dx_sink_fn sink, void *suser, size_t *out_len)
{ uint8_t *buf = NULL;
  size_t   have = 0, total = 0;
  u2_state st;
  int      eof = 0, rc = DX_OK;

  if (ctx == NULL || rd_ == NULL || sink == NULL || width == 0) return DX_E_ARG;
  memset(&st, 0, sizeof(st));
  if (chunk == 0) chunk = (size_t) dx_test_num("stream_chunk", (long long) 128 << 20);
  if (chunk < 4096) chunk = 4096;
  buf = malloc(chunk + 16);
  if (buf == NULL) return DX_E_NOMEM;
  if (out_len) *out_len = 0;
  for (;;)
    { size_t piece = 0;
      shifted_sink h = { sink, suser, total };
      while (!eof && have < chunk)
        { const long got = rd_(ruser, buf + have, chunk - have);
          if (got < 0) { rc = DX_E_IO; goto done; }
          if (got == 0) eof = 1;
          have += (size_t) got;
        }
      st.more = !eof;
      rc = unpack2_core(ctx, mode, buf, have, width, NULL, pass_shifted, &h, &piece, &st);
      if (rc != DX_OK) goto done;
      total += piece;
      if (eof) break;                                    /* (the last piece: whole, or the core has said DX_E_FORMAT) */
      if (st.consumed == 0)                              /* not one whole record in the buffer: a larger one */
        { uint8_t *nb;
          chunk += chunk;
          nb = realloc(buf, chunk + 16);
          if (nb == NULL) { rc = DX_E_NOMEM; goto done; }
          buf = nb;
          continue;
        }
      memmove(buf, buf + st.consumed, have - st.consumed);
      have -= st.consumed;
    }
  if (out_len) *out_len = total;
done:
  free(st.name);
  free(buf);
  return rc;
}
