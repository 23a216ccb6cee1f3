/*
 * dx_files.c -- whole-file drivers: the host side of the six tools, above the kernel C-ABI.
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
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "dexgpu.h"
#include "dx_env.h"
#include "dx_host.h"
#include "dx_walk.h"

void dx_file_free(void *p) { free(p); }

/* DEXGPU_TIMING=1: where a file driver spends its time (stderr; the tools print their own marks beside these) */
static void fmark(const char *what)
{ static double t0 = -1.0;
  dx_mark("dx_file", &t0, what);
}

#define TRY(x) do { rc = (x); if (rc != DX_OK) goto done; } while (0)

#define DX_GPU_INDEX_MIN (1u << 20)      /* .quiva images from 1 MiB on are indexed on the GPU */

typedef struct { void *p[24]; int n; dx_ctx *ctx; } dpool;

static int dalloc(dpool *pool, size_t bytes, void **out)
{ int rc;
  if (pool->n >= (int) (sizeof(pool->p) / sizeof(pool->p[0])) - 2) return DX_E_NOMEM;   /* pool slots exhausted */
  rc = dx_malloc(pool->ctx, bytes + 64, out);
  if (rc == DX_OK) pool->p[pool->n++] = *out;
  return rc;
}

static int dupload(dpool *pool, const void *src, size_t bytes, void **out)
{ int rc = dalloc(pool, bytes, out);
  if (rc == DX_OK && bytes) rc = dx_h2d(pool->ctx, *out, src, bytes);
  return rc;
}

/* a device array of the caller's (*p, *cap bytes of it; none yet: NULL, 0) that is to hold `need` bytes: made anew when it is too small,
   and what it held is gone then */
static int dgrow(dx_ctx *ctx, void **p, size_t *cap, size_t need)
{ int rc;
  if (need <= *cap) return DX_OK;
  if (*p) (void) dx_free(ctx, *p);
  *p = NULL; *cap = 0;
  if ((rc = dx_malloc(ctx, need, p)) != DX_OK) { *p = NULL; return rc; }
  *cap = need;
  return DX_OK;
}

/* The encoder of the file drivers is dx_qv_encode_onepass (no size pass; the same bytes).  DEXGPU_TEST=twopass
 * selects dx_qv_sizes + dx_qv_encode instead (the two-pass API, kept as a cross-check). */
static int two_pass(void)
{ return dx_test_on("twopass"); }

static void dfree_all(dpool *pool)
{ int i;
  for (i = 0; i < pool->n; i++)
    dx_free(pool->ctx, pool->p[i]);
  pool->n = 0;
}

/* DEXGPU_TEXT_BUDGET (bytes): how much of `whole` bytes the device is to take at once.  1: the variable is set and has decided -- *cap is
   its figure (`floor` at least), or 0 for all at once (no figure, or one the whole stays under); 0: it is not set, what is free decides */
static int budget_env(size_t whole, size_t floor, size_t *cap)
{ const char *e = getenv("DEXGPU_TEXT_BUDGET");
  unsigned long long v;
  if (e == NULL || !*e) return 0;
  v = strtoull(e, NULL, 10);
  *cap = v && v < whole ? (size_t) (v < floor ? floor : v) : 0;
  return 1;
}

/* a sink that sees its chunks `shift` bytes further on (the record stream follows the file's head; a piece follows the pieces before it) */
typedef struct { dx_sink_fn sink; void *user; size_t shift; } shifted_sink;
static int pass_shifted(void *arg, uint8_t *data, size_t len, size_t at)
{ shifted_sink *h = arg;
  return h->sink(h->user, data, len, at + h->shift);
}

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
  if (budget_env(n, 65536u, &cap)) return cap;
  if (dx_mem_info(ctx, &fr, &all) != DX_OK || fr == 0) return 0;
  return 1.35 * (double) n > 0.9 * (double) fr ? (size_t) (0.6 * (double) fr) : 0;
}

/* The index of a .fasta / .arrow text and the layout of its image.  Per read: where its lines begin in the text and how long they are
   (off, tlen: host index only), its symbols (nsym), the header's fields (hdr4, cnr4); then the framed header bytes (blob, hoff[cnt + 1])
   and the record's place in the image (ooff[cnt + 1]; ooff[cnt] == total). */
typedef struct
  { uint64_t  cnt, *off, *hoff, *ooff;
    uint32_t *tlen, *nsym;
    int32_t  *hdr4;
    uint16_t *cnr4;
    uint8_t  *blob;
    size_t    plen, total;
  } seq_index;

static void seq_index_free(seq_index *ix)
{ free(ix->off); free(ix->hoff); free(ix->ooff); free(ix->tlen); free(ix->nsym); free(ix->hdr4); free(ix->cnr4); free(ix->blob); }

static int seq_index_host(seq_index *ix, int arrow, const uint8_t *text, size_t n, uint64_t *errline, int *errcode)
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
        { d_off = go; d_tlen = gt; d_nsym = gs;
          pool.p[pool.n++] = go; pool.p[pool.n++] = gt; pool.p[pool.n++] = gs;
          ix.nsym = malloc((ix.cnt + 1) * sizeof(*ix.nsym));
          if (!ix.nsym) { rc = DX_E_NOMEM; goto done; }
          TRY(dx_d2h(ctx, ix.nsym, d_nsym, ix.cnt * 4));
        }
      else if (rc != DX_E_FORMAT)
        goto done;
    }
  if (d_off == NULL) TRY(seq_index_host(&ix, arrow, text, n, errline, errcode));
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
  seq_index_free(&ix);
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
 * ========================================================================================== */
typedef struct
  { dx_ctx          *ctx;
    int              arrow, rc;
    const uint8_t   *text;
    const seq_index *ix;
    uint8_t         *img;
    uint64_t         lo, hi;                  /* reads [lo, hi) */
  } p2_job;

static void *p2_main(void *arg)
{ p2_job *j = (p2_job *) arg;
  j->rc = pack2_range(j->ctx, j->arrow, j->text, j->ix, j->lo, j->hi, j->img);
  return NULL;
}

int dx_file_pack2_sharded(dx_ctx **ctxs, int nctx, int arrow, const uint8_t *text, size_t n,
                          uint8_t **out, size_t *out_len, uint64_t *errline, int *errcode)
{ seq_index ix;
  int32_t   lwell = 0;
  uint8_t  *img = NULL;
  p2_job   *jobs = NULL;
  pthread_t *th = NULL;
  int       rc, k, started = 0;

  if (ctxs == NULL || nctx < 1 || out == NULL || out_len == NULL) return DX_E_ARG;
  if (nctx == 1) return dx_file_pack2(ctxs[0], arrow, text, n, out, out_len, errline, errcode);
  *out = NULL; *out_len = 0;
  memset(&ix, 0, sizeof(ix));

  TRY(seq_index_host(&ix, arrow, text, n, errline, errcode));
  TRY(seq_index_frame(&ix, arrow, &lwell, 2 + 4 + ix.plen));             /* one pass: well deltas chain over the whole file */
  img = malloc(ix.total + 16);
  if (!img) { rc = DX_E_NOMEM; goto done; }
  pack2_head(img, text, ix.plen);

  jobs = calloc((size_t) nctx, sizeof(*jobs));
  th   = calloc((size_t) nctx, sizeof(*th));
  if (!jobs || !th) { rc = DX_E_NOMEM; goto done; }
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
  for (k = 0; k < nctx; k++)
    { if (pthread_create(&th[k], NULL, p2_main, &jobs[k]) != 0) { rc = DX_E_NOMEM; break; }
      started++;
    }
  for (k = 0; k < started; k++)
    pthread_join(th[k], NULL);
  if (started < nctx) goto done;
  rc = DX_OK;
  for (k = 0; k < nctx; k++)
    if (jobs[k].rc != DX_OK) { rc = jobs[k].rc; break; }
  if (rc == DX_OK)
    { *out = img; *out_len = ix.total; img = NULL; }

done:
  seq_index_free(&ix);
  free(img); free(jobs); free(th);
  return rc;
}

/* ==========================================================================================
 *  undexta / undexar
 * ========================================================================================== */
/* One path: the image is walked on the host (u2_walk), the text laid out (u2_layout), and unpack2_slices decodes it slice by slice
   of whole reads -- the whole text is the case of one slice.  What becomes of a slice is its hook's business (slice_fn): out to the
   caller (slice_deliver), compared (verify_slice), hashed (digest_slice). */
typedef struct { const uint8_t *p; size_t n, at; int bad; } rsrc;

static void rd(rsrc *r, void *dst, size_t k)
{ if (r->at + k > r->n) { r->bad = 1; memset(dst, 0, k); r->at = r->n; return; }
  memcpy(dst, r->p + r->at, k);
  r->at += k;
}
static int32_t  rd_i32(rsrc *r, int flip) { uint32_t v; rd(r, &v, 4); return (int32_t) (flip ? flip32(v) : v); }
static uint16_t rd_u16(rsrc *r, int flip) { uint16_t v; rd(r, &v, 2); return flip ? flip16(v) : v; }

typedef struct { char *p; size_t len, cap; } tbuf;

static int tb_room(tbuf *b, size_t more)
{ if (b->len + more > b->cap)
    { size_t nc = (b->len + more) * 2 + 4096;
      char  *np = realloc(b->p, nc);
      if (np == NULL) return DX_E_NOMEM;
      b->p = np; b->cap = nc;
    }
  return DX_OK;
}

/* A chunk of decoded text on its way out (dx_d2h_stream): the header lines that fall into it are laid over it.
   Entry i's text starts at ooff[i]; its header line, hd[hat[i] .. hat[i+1]), ends there.                 */
typedef struct
  { uint64_t n; const uint64_t *ooff, *hat; const char *hd;
    dx_sink_fn sink; void *user;
    size_t base;                  /* where in the text the streamed buffer starts (a slice of the entries; else 0) */
    size_t total;                 /* the whole text's bytes */
  } hdr_patch;

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

/* where entry i's header line starts in the text (i == n: where the text ends) */
static size_t text_at(const hdr_patch *h, uint64_t i)
{ return i < h->n ? (size_t) h->ooff[i] - (size_t) (h->hat[i + 1] - h->hat[i]) : h->total; }

/* a slice of whole entries from i0 on: as many as make at most `cap` bytes of text, and one at least; cap 0: all that are left */
static uint64_t text_slice_end(const hdr_patch *h, uint64_t i0, size_t cap)
{ uint64_t i1 = i0 + 1;
  if (cap == 0) return h->n;
  while (i1 < h->n && text_at(h, i1 + 1) - text_at(h, i0) <= cap) i1++;
  return i1;
}

/* how much of an output of `total` bytes the device makes at once beside an input of n bytes (and 48 bytes of index a unit): 0 = all
   of it; DEXGPU_TEXT_BUDGET (bytes) when set, else what is free decides */
static size_t out_cap(dx_ctx *ctx, size_t n, size_t total, uint64_t units)
{ uint64_t fr = 0, all = 0;
  size_t   cap;
  if (budget_env(total, 65536u, &cap)) return cap;
  if (dx_mem_info(ctx, &fr, &all) != DX_OK || fr == 0) return 0;
  if ((double) n + (double) total + 48.0 * (double) units <= 0.9 * (double) fr) return 0;
  { const double room = 0.9 * (double) fr - (double) n - 48.0 * (double) units;
    return room > (double) ((size_t) 4 << 20) ? (size_t) room : (size_t) 4 << 20;
  }
}

/* What becomes of a slice of decoded text -- entries [i0, i1), `bytes` of them at d_out, the first at t0 in the whole text: DX_OK
   (the next slice), SLICE_STOP (no more slices are wanted: not an error), or an error */
typedef int (*slice_fn)(void *arg, const void *d_out, uint64_t i0, uint64_t i1, size_t t0, size_t bytes);
#define SLICE_STOP 1

/* ... out to the caller: into the text in memory (res), or through the sink of h; header lines in place either way */
typedef struct { dx_ctx *ctx; hdr_patch *h; uint8_t *res; } slice_out;
static int slice_deliver(void *arg, const void *d_out, uint64_t i0, uint64_t i1, size_t t0, size_t bytes)
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

/* an image that arrives in pieces (dx_file_unpack2_stream): what the file's head said, the well the last record stood at, and
   how far into this piece the whole records reached (a piece may end inside a record: `more` says that more is coming) */
typedef struct { int started, flip, newv, well, more; int32_t plen; char *name; size_t consumed; } u2_state;

/* The records of a .dexta / .dexar image, walked (undexta.c:138-271, undexar.c:136-229): per read where its packed bases stand in the
   image (ioff) and how many there are (nsym), and its header line as the tool prints it (hd, from hat[i] on; hat[cnt]: their end);
   `at`: how far the whole records reached, `well`: the last one's well. */
typedef struct { uint64_t cnt, *ioff, *hat; uint32_t *nsym; tbuf hd; size_t at; int well; } u2_index;

static void u2_index_free(u2_index *x)
{ free(x->ioff); free(x->hat); free(x->nsym); free(x->hd.p); }

#define U2_NOT_YET 1                /* (a piece of an image that arrives in pieces: its head is not all here yet; nothing consumed) */

/* mode: DX_LETTERS_LOWER / _UPPER (dexta images) or _ARROW (dexar images); st: the image arrives in pieces (else NULL) */
static int u2_walk(int mode, const uint8_t *img, size_t n, u2_state *st, u2_index *x)
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
        { void *t;                                        /* a failed realloc leaves the old block to the caller's u2_index_free */
          cap  = cap ? 2 * cap : 1024;
          if ((t = realloc(x->ioff, cap * sizeof(*x->ioff))) == NULL) { rc = DX_E_NOMEM; goto done; }
          x->ioff = t;
          if ((t = realloc(x->hat, (cap + 1) * sizeof(*x->hat))) == NULL) { rc = DX_E_NOMEM; goto done; }
          x->hat = t;
          if ((t = realloc(x->nsym, cap * sizeof(*x->nsym))) == NULL) { rc = DX_E_NOMEM; goto done; }
          x->nsym = t;
        }
      if ((rc = tb_room(&x->hd, (size_t) plen + 160)) != DX_OK) goto done;
      x->hat[cnt] = x->hd.len;
      if (arrow)                                          /* undexar.c:199-203 */
        { float snr[4];
          for (k = 0; k < 4; k++) snr[k] = (float) (cnr[k] / 100.);
          x->hd.len += (size_t) sprintf(x->hd.p + x->hd.len, "%s/%d/%d_%d SN=%.2f,%.2f,%.2f,%.2f\n", name, well, beg, end,
                                        snr[0], snr[1], snr[2], snr[3]);
        }
      else                                                /* undexta.c:242 */
        x->hd.len += (size_t) sprintf(x->hd.p + x->hd.len, "%s/%d/%d_%d RQ=0.%d\n", name, well, beg, end, qv);

      x->ioff[cnt] = r.at;
      x->nsym[cnt] = rlen;
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
static size_t u2_layout(const u2_index *x, uint32_t width, uint64_t *ooff)
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
static int unpack2_slices(dx_ctx *ctx, int mode, const uint8_t *img, size_t n, uint32_t width, const u2_index *x, const hdr_patch *h,
                          size_t cap, slice_fn deliver, void *arg)
{ dpool     pool = { {0}, 0, ctx };
  const uint64_t cnt = x->cnt;
  uint64_t *rel = NULL, i, i0, i1, most = 0;
  size_t    tmax = 0;
  void     *d_in, *d_ioff, *d_nsym, *d_out, *d_ooff;
  int       rc;
  for (i0 = 0; i0 < cnt; i0 = i1)
    { i1 = text_slice_end(h, i0, cap);
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
      i1 = text_slice_end(h, i0, cap);
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

  rc = u2_walk(mode, img, n, st, &x);
  if (rc == U2_NOT_YET) { u2_index_free(&x); return DX_OK; }
  if (rc != DX_OK) goto done;
  cnt = x.cnt;
  ooff = malloc((cnt + 1) * sizeof(*ooff));
  if (ooff == NULL) { rc = DX_E_NOMEM; goto done; }
  total = u2_layout(&x, width, ooff);                     /* output layout: header line, wrapped text */
  if (out)
    { res = malloc(total + 16);
      if (!res) { rc = DX_E_NOMEM; goto done; }
    }

  if (cnt > 0)                                            /* (an image without records: nothing for the device) */
    { /* All of the text at once, or, when it does not fit the device beside the image (or DEXGPU_TEXT_BUDGET says so), in slices
         of whole reads, every slice's text out before the next one's is made. */
      hdr_patch h = { cnt, ooff, x.hat, x.hd.p, sink, user, 0, total };
      slice_out so = { ctx, &h, res };
      TRY(unpack2_slices(ctx, mode, img, n, width, &x, &h, out_cap(ctx, n, total, cnt), slice_deliver, &so));
    }
  if (out) { *out = res; res = NULL; }
  *out_len = total;
  if (st != NULL) { st->well = x.well; st->consumed = x.at; }
  rc = DX_OK;

done:
  u2_index_free(&x);
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

/* ==========================================================================================
 *  dexqv
 * ========================================================================================== */
/* The host's index of a .quiva text (dx_index_quiva): per entry where its five lines begin, how long they are, the header's four fields */
typedef struct { uint64_t cnt, *off; uint32_t *len; int32_t *hdr4; size_t plen; } quiva_index;

static int quiva_index_host(quiva_index *qx, const uint8_t *text, size_t n, uint64_t *errline, int *errcode)
{ const int rc = dx_index_quiva(text, n, 0, NULL, NULL, NULL, &qx->cnt, &qx->plen, errline, errcode);
  if (rc != DX_OK) return rc;
  if (qx->cnt == 0) return DX_E_DEGENERATE;              /* empty file: the reference dereferences a NULL header (dexqv.c:94) */
  qx->off  = malloc((qx->cnt + 1) * sizeof(*qx->off));
  qx->len  = malloc((qx->cnt + 1) * sizeof(*qx->len));
  qx->hdr4 = malloc((qx->cnt + 1) * 4 * sizeof(*qx->hdr4));
  if (!qx->off || !qx->len || !qx->hdr4) return DX_E_NOMEM;
  return dx_index_quiva(text, n, qx->cnt, qx->off, qx->len, qx->hdr4, &qx->cnt, &qx->plen, errline, errcode);
}

static void quiva_index_free(quiva_index *qx)
{ free(qx->off); free(qx->len); free(qx->hdr4); }

/* where entry e's five lines end in the text */
static uint64_t quiva_end(const quiva_index *qx, uint64_t e)
{ return qx->off[e] + 5 * ((uint64_t) qx->len[e] + 1); }

/* a slice of whole entries from e0 on: as many as make at most `cap` bytes of text (an entry larger than the cap is a slice of its own) */
static uint64_t quiva_slice_end(const quiva_index *qx, uint64_t e0, size_t cap)
{ const uint64_t s0 = e0 ? quiva_end(qx, e0 - 1) : 0;
  uint64_t e1 = e0 + 1;
  while (e1 < qx->cnt && quiva_end(qx, e1) - s0 <= cap) e1++;
  return e1;
}

static dx_qv_batch qv_batch(const void *d_text, const void *d_off, const void *d_len, uint64_t m, uint64_t span, int line_pad)
{ dx_qv_batch b;
  memset(&b, 0, sizeof(b));
  b.d_text = d_text; b.d_off = d_off; b.d_len = d_len; b.n = m; b.line_pad = (uint32_t) line_pad; b.text_bytes = span;
  return b;
}

/* A batch of entries as the encoder wants it: the text (b), the framing bytes of the headers and their offsets (none of either for the bare
   record stream of the entry API), and the per-entry record offsets and segment sizes the encoder fills */
typedef struct { dx_qv_batch b; void *d_hdr, *d_hoff, *d_rec, *d_seg; uint64_t hbytes; } qv_staged;

/* m entries whose text is on the device (span bytes at d_text) staged in `pool`: their header fields hdr4 framed from *lwell on (the well
   chain runs through a file's batches) and uploaded; hdr4 == NULL: no framing bytes */
static int qv_stage(dpool *pool, const int32_t *hdr4, uint64_t m, int32_t *lwell, const void *d_text, const void *d_off, const void *d_len,
                    uint64_t span, int line_pad, qv_staged *s)
{ uint64_t *hoff = NULL;
  uint8_t  *blob = NULL;
  int       rc;
  memset(s, 0, sizeof(*s));
  s->b = qv_batch(d_text, d_off, d_len, m, span, line_pad);
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
static int qv_encode_batch(dx_ctx *ctx, const qv_staged *s, const uint64_t (*hist)[256], const dx_qv_coding *cd, int lossy,
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
static int qv_head(const dx_qv_coding *cd, const uint8_t *text, size_t plen, size_t more, uint8_t **img, size_t *head)
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
 *           nowhere), the encoder (qv_encode_batch), the slice's records out behind the last slice's.
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
  TRY(quiva_index_host(&qx, text, n, errline, errcode));
  for (e0 = 0; e0 < qx.cnt; e0 = e1)                      /* the widest slice in entries and bytes: one allocation serves them all */
    { const uint64_t s0 = e0 ? quiva_end(&qx, e0 - 1) : 0;
      e1 = quiva_slice_end(&qx, e0, cap);
      if (e1 - e0 > maxent) maxent = (size_t) (e1 - e0);
      if (quiva_end(&qx, e1 - 1) - s0 > slice_bytes) slice_bytes = (size_t) (quiva_end(&qx, e1 - 1) - s0);
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
          TRY(qv_head(cd, text, qx.plen, 0, &head_img, &head));
          if (sink(user, head_img, head, 0)) { rc = DX_E_IO; goto done; }
          at = head;
        }
      for (e0 = 0; e0 < qx.cnt; e0 = e1)
        { const uint64_t s0 = e0 ? quiva_end(&qx, e0 - 1) : 0;
          uint64_t s1, k, m, total = 0;
          dx_qv_batch b;
          e1 = quiva_slice_end(&qx, e0, cap);
          s1 = quiva_end(&qx, e1 - 1);
          m  = e1 - e0;
          for (k = 0; k < m; k++) rel[k] = qx.off[e0 + k] - s0;
          TRY(dx_h2d(ctx, d_text, text + s0, (size_t) (s1 - s0)));
          TRY(dx_h2d(ctx, d_off, rel, (size_t) m * 8));
          TRY(dx_h2d(ctx, d_len, qx.len + e0, (size_t) m * 4));
          b = qv_batch(d_text, d_off, d_len, m, s1 - s0, 1);
          if (pass == 1)
            TRY(dx_qv_scan(ctx, &b, e0, &p, hist, &tot));                               /* QV.c:993-1017, state carried along */
          else
            { uint64_t  t2 = 0;
              qv_staged st;
              shifted_sink h = { sink, user, (size_t) at };
              memset(junk, 0, 6 * sizeof(*junk));
              TRY(dx_qv_hist(ctx, &b, e0, &p, junk, &t2));                               /* this slice's tokens (and its own counts, for the bound) */
              TRY(qv_stage(&spool, qx.hdr4 + 4 * e0, m, &lwell, d_text, d_off, d_len, s1 - s0, 1, &st));
              TRY(qv_encode_batch(ctx, &st, (const uint64_t (*)[256]) junk, cd, lossy, &d_out, &out_cap, &total));
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
  quiva_index_free(&qx);
  free(rel); free(cd); free(hist); free(junk); free(head_img); free(grow.p);
  return rc;
}

/* how much text the device takes at once: DEXGPU_TEXT_BUDGET (bytes) when set, else what fits beside the tokens, the scratch
   regions and the output (about 2.5 bytes of device memory per byte of text), 0 = all of it */
static size_t text_cap(dx_ctx *ctx, size_t n)
{ uint64_t fr = 0, all = 0;
  size_t   cap;
  if (budget_env(n, (size_t) 4 << 20, &cap)) return cap;
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
        { d_off = go; d_len = gl;
          pool.p[pool.n++] = go; pool.p[pool.n++] = gl;
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
      TRY(quiva_index_host(&qx, text, n, errline, errcode));
      TRY(dupload(&pool, qx.off, qx.cnt * 8, &d_off));
      TRY(dupload(&pool, qx.len, qx.cnt * 4, &d_len));
    }
  fmark("dexqv: indexed");
  TRY(qv_stage(&pool, qx.hdr4, qx.cnt, &lwell, d_text, d_off, d_len, n, 1, &st));

  /* ... and histogram on the device (QV.c:988-1017) */
  TRY(dx_qv_scan(ctx, &st.b, 0, &p, hist, &tot));
  TRY(dx_qv_build((const uint64_t (*)[256]) hist, tot, &p, lossy, cd));   /* Create_QVcoding, dexqv.c:86 */
  TRY(dx_qv_set_coding(ctx, cd, lossy));
  fmark("dexqv: scanned, tables built");

  /* pass 2, dexqv.c:112-143: Compress_Next_QVentry for every entry */
  TRY(qv_encode_batch(ctx, &st, (const uint64_t (*)[256]) hist, cd, lossy, &d_out, &out_cap, &total));
  fmark("dexqv: encoded");
  TRY(qv_head(cd, text, qx.plen, out ? total : 0, &img, &head));
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
  quiva_index_free(&qx);
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
/* undexqv in two steps (dexgpu.h): the plan is host work only, the run is the GPU's.  The run has one path, undexqv_sliced: slices of
   whole entries, and the whole text is the case of one slice.  dx_file_undexqv_run, dx_file_verify and dx_file_digest all decode
   through it, so a check of an image takes the decoder kernels the tool's own run takes. */
struct dx_undexqv_plan
  { const uint8_t *img;
    size_t         n, total;
    dx_qv_index    x;
    tbuf           hd;            /* the header lines, one after the other */
    uint64_t      *ooff, *hat;    /* per entry: where its five data lines start in the text; where its header line starts in hd */
    /* a plan made on the device (dx_file_undexqv_plan_on): the image is there already, and so is the index */
    dx_ctx        *ctx;
    void          *d_in;          /* the image, when it is on ctx's device already */
    dx_qv_dindex   dix;           /* the index, when it was made there (d_rec_off != NULL) */
  };
#define PLAN_HAS_IMAGE(p) ((p)->ctx != NULL && (p)->d_in != NULL)
#define PLAN_HAS_INDEX(p) ((p)->ctx != NULL && (p)->dix.d_rec_off != NULL)

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

/* header lines (undexqv.c:182) and where every entry's lines go in the text, from p->x.n / len / hdr4 / prefix */
static int plan_layout(dx_undexqv_plan *p)
{ const size_t plen = strlen(p->x.prefix);
  size_t   total = 0;
  uint64_t i;
  int      rc;
  p->ooff = malloc((p->x.n + 1) * sizeof(*p->ooff));
  p->hat  = malloc((p->x.n + 1) * sizeof(*p->hat));
  if (!p->ooff || !p->hat) return DX_E_NOMEM;
  for (i = 0; i < p->x.n; i++)
    { const int32_t *h = p->x.hdr4 + 4*i;
      if ((rc = tb_room(&p->hd, plen + 80)) != DX_OK) return rc;
      p->hat[i]  = p->hd.len;
      p->hd.len += (size_t) sprintf(p->hd.p + p->hd.len, "%s/%d/%d_%d RQ=0.%d\n", p->x.prefix, h[0], h[1], h[2], h[3]);
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
 * slice; with several slices it stays out.                                                                          */
static int undexqv_sliced(dx_ctx *ctx, const dx_undexqv_plan *p, int upper, slice_fn deliver, void *arg, size_t cap, int whole_in_)
{ const int whole_in = whole_in_ || PLAN_HAS_IMAGE(p);    /* (an image that is there is there whole) */
  dpool     pool = { {0}, 0, ctx };
  const uint64_t n = p->x.n;
  undexqv_staged s;
  void     *d_out = NULL, *d_ooff = NULL;
  uint64_t *rel = NULL, i0, i1, i, most = 0;
  size_t    tmax = 0, imax = 0;
  const hdr_patch h = { n, p->ooff, p->hat, p->hd.p, NULL, NULL, 0, p->total };      /* (the layout, for the slices' bounds) */
  int       rc = DX_OK, indexed = 0;
  for (i0 = 0; i0 < n; i0 = i1)                           /* the largest slice: one allocation serves them all */
    { i1 = text_slice_end(&h, i0, cap);
      if (text_at(&h, i1) - text_at(&h, i0) > tmax) tmax = text_at(&h, i1) - text_at(&h, i0);
      if (i1 - i0 > most) most = i1 - i0;
      if (!whole_in && p->x.rec_off[i1] - p->x.rec_off[i0] > imax) imax = (size_t) (p->x.rec_off[i1] - p->x.rec_off[i0]);
    }
  rel = malloc((most + 1) * 2 * sizeof(*rel));
  if (rel == NULL) return DX_E_NOMEM;
  TRY(undexqv_stage(ctx, p, &pool, imax, most, &s, &indexed));
  TRY(dalloc(&pool, (most + 1) * 8, &d_ooff));
  TRY(dalloc(&pool, tmax, &d_out));
  if (p->x.gidx != NULL && !p->x.flip && whole_in && text_slice_end(&h, 0, cap) == n)
    { void *d_gidx, *d_goff;
      TRY(dupload(&pool, p->x.gidx, (size_t) p->x.gidx_words * 4, &d_gidx));
      TRY(dupload(&pool, p->x.gidx_off, (n + 1) * 8, &d_goff));
      TRY(dx_qv_use_index(ctx, s.d_in, s.d_seg, n, d_gidx, d_goff, p->x.gidx_none));
      indexed = 1;
    }
  for (i0 = 0; i0 < n; i0 = i1)
    { const size_t t0 = text_at(&h, i0);
      const uint64_t *rec = s.d_rec;
      i1 = text_slice_end(&h, i0, cap);
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
static size_t undexqv_cap(dx_ctx *ctx, const dx_undexqv_plan *p, int *whole_in)
{ uint64_t fr = 0, all = 0;
  size_t   cap = 0;
  *whole_in = 1;
  if (budget_env(p->total, 65536u, &cap)) return cap;
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
  cap = undexqv_cap(ctx, p, &whole_in);
  if (cap && dx_test_on("slice_input") && !PLAN_HAS_IMAGE(p)) whole_in = 0;      /* (DEXGPU_TEST=slice_input) */
  { hdr_patch h = { p->x.n, p->ooff, p->hat, p->hd.p, sink, user, 0, p->total };
    slice_out so = { ctx, &h, NULL };
    return undexqv_sliced(ctx, p, upper, slice_deliver, &so, cap, whole_in);
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

/* ==========================================================================================
 *  An image of any of the three kinds and the text it decodes to, for who wants the text's slices where they are made
 *  (dx_file_verify, dx_file_digest): the image's records walked, the header lines the decoder prints, the text's layout.
 * ========================================================================================== */
typedef struct
  { int              kind, mode, upper;            /* DX_KIND_*; the 2-bit kinds' DX_LETTERS_*; quiva: undexqv -U */
    uint32_t         width;                        /* the 2-bit kinds' line width */
    const uint8_t   *img;
    size_t           n;
    u2_index         ux;                           /* the 2-bit kinds' records */
    dx_undexqv_plan *plan;                         /* quiva's */
    uint64_t        *ooff;                         /* h.n + 1 (the last: h.total); owned for the 2-bit kinds, the plan's for quiva */
    hdr_patch        h;                            /* the layout as the slice loops and their hooks read it (no sink): h.n records, h.total
                                                      bytes of text, the header lines h.hd one after the other, hd_len bytes of them */
    size_t           hd_len;
  } image_text;

static void image_close(image_text *im)
{ dx_file_undexqv_plan_free(im->plan);
  u2_index_free(&im->ux);
  if (im->kind != DX_KIND_QUIVA) free(im->ooff);
  memset(im, 0, sizeof(*im));
}

/* an error leaves what there is to image_close */
static int image_open(dx_ctx *ctx, int kind, int upper, uint32_t width, const uint8_t *img, size_t n, image_text *im)
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
      if ((rc = u2_walk(im->mode, img, n, NULL, &im->ux)) != DX_OK) return rc;
      h->n = im->ux.cnt;
      if ((im->ooff = malloc((h->n + 1) * sizeof(*im->ooff))) == NULL) return DX_E_NOMEM;
      h->total = u2_layout(&im->ux, width, im->ooff);
      im->ooff[h->n] = h->total;
      h->hat = im->ux.hat; h->hd = im->ux.hd.p; im->hd_len = im->ux.hd.len;
    }
  h->ooff = im->ooff;
  return DX_OK;
}

/* the text in slices of at most `cap` bytes (0: in one), each to `fn`; whole_in: quiva's image goes up whole (undexqv_sliced) */
static int image_slices(dx_ctx *ctx, const image_text *im, size_t cap, int whole_in, slice_fn fn, void *arg)
{ if (im->kind == DX_KIND_QUIVA) return undexqv_sliced(ctx, im->plan, im->upper, fn, arg, cap, whole_in);
  return unpack2_slices(ctx, im->mode, im->img, im->n, im->width, &im->ux, &im->h, cap, fn, arg);
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
      { const dx_qv_batch b = qv_batch(v->d_src, da_off, dq_len, m, s1 - s0, 1);
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
  if (budget_env(2 * total, 131072u, &cap)) return cap / 2;
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
  rc = kind == DX_KIND_QUIVA ? quiva_index_host(&qx, text, n, &el, &ec) : seq_index_host(&sx, kind == DX_KIND_ARROW, text, n, &el, &ec);
  if (rc == DX_OK)
    { text_options(kind, text, &sx, &qx, &up, width);
      *upper = up;
    }
  seq_index_free(&sx); quiva_index_free(&qx);
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
    { TRY(quiva_index_host(&qx, text, n, &el, &ec));
      v.cnt = qx.cnt; v.off = qx.off; v.blen = qx.len;
    }
  else
    { TRY(seq_index_host(&sx, kind == DX_KIND_ARROW, text, n, &el, &ec));
      v.cnt = sx.cnt; v.off = sx.off; v.blen = sx.tlen;
    }
  text_options(kind, text, &sx, &qx, &rep->upper, &rep->width);
  rep->records_src = v.cnt;

  /* the image, decoded with those options */
  rc = m ? image_open(ctx, kind, rep->upper, rep->width, img, m, &im) : DX_E_FORMAT;
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
  image_close(&im);
  seq_index_free(&sx); quiva_index_free(&qx);
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

  TRY(image_open(ctx, kind, upper, width, img, m, &im));
  cnt = im.h.n; g.hd_bytes = im.hd_len;
  if (rec_crc != NULL && (g.rec = malloc((cnt + 1) * sizeof(*g.rec))) == NULL) { rc = DX_E_NOMEM; goto done; }

  if (cnt > 0)
    { int whole_in = 1;
      const size_t cap = kind == DX_KIND_QUIVA ? undexqv_cap(ctx, im.plan, &whole_in) : out_cap(ctx, m, im.h.total, cnt);
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
  image_close(&im);
  free(g.rec);
  return rc;
}

/* ==========================================================================================
 *  dexqv of one file on several GPUs: contiguous entry ranges, one host thread
 *  per context; the only exchange is on the host -- the merged scan state (32 bytes) and the sum
 *  of the 12 KB histograms -- after which every shard is encoded with identical tables and the
 *  record streams are concatenated in order.  No RCCL.
 * ========================================================================================== */

typedef struct shard_job shard_job;

typedef struct
  { int               nsh, lossy, rc;
    int               ok;                    /* written by shard 0 in its merge steps only, read by all after the next barrier */
    int               go;                    /* start gate: 0 wait, 1 run, -1 a thread could not be created: leave */
    pthread_mutex_t   gate_mx;
    pthread_cond_t    gate_cv;
    pthread_barrier_t bar;
    const uint8_t    *text;
    const uint64_t   *off;
    const uint32_t   *len;
    const int32_t    *hdr4;
    uint64_t          cnt, cut;              /* cut: entry at which the running symbol count reaches 100000 */
    dx_qv_params      p;
    dx_qv_coding      cd;
    uint64_t          hist[6][256], tot;
    uint8_t          *img;
    size_t            head, total;
    shard_job        *jobs;
    /* by bytes (large files): no index of the whole file exists; every shard finds and indexes its own records (shard_slice) */
    int               by_bytes, again;       /* again: something is not as it should be -- the whole file once more, the serial way */
    size_t            n, plen;
  } shard_all;

struct shard_job
  { shard_all   *all;
    dx_ctx      *ctx;
    int          id, rc;
    uint64_t     lo, hi;                      /* entries [lo, hi) */
    dx_qv_params p;
    uint64_t     hist[6][256], tot, bytes, at;
    /* by bytes: the shard's byte range as dealt, the newlines in it, where its first record begins and the line that is, its own
       index (hdr4 / len: host, the shard's entries; the offsets stay on the device) */
    size_t       p0, p1, start;
    uint64_t     nl, line0;
    int32_t     *hdr4;
    uint32_t    *len;
  };

/* Steps alternate between "every shard works and sets its own rc" and "shard 0 folds the results",
 * with a barrier after each: shard 0 reads the others' rc only in its folding steps (nobody writes
 * then) and publishes the verdict in a->ok, which the working steps read (nobody writes it then).   */
static int all_ok(shard_all *a)
{ int k;
  for (k = 0; k < a->nsh; k++)
    if (a->jobs[k].rc != DX_OK) return 0;
  return a->rc == DX_OK;
}

static int shard_slice(shard_job *j, dpool *pool, void **d_text, void **d_off, void **d_len, uint64_t *span);

/* The shard's entries staged on its device and prescanned (QV.c:993-1015, per shard).  By bytes, shard_slice has put text and index
   there (d_text, d_off, d_len, span); else they are cut from the file's host index here. */
static int shard_stage(shard_job *j, dpool *pool, void *d_text, void *d_off, void *d_len, uint64_t span, qv_staged *st)
{ shard_all     *a = j->all;
  const uint64_t m = j->hi - j->lo;
  const int32_t *hdr4 = j->hdr4;
  uint64_t      *roff = NULL, i;
  int32_t        lwell;
  int            rc;
  if (a->by_bytes)
    { const shard_job *prev = &a->jobs[j->id ? j->id - 1 : 0];
      lwell = j->id ? prev->hdr4[4 * (prev->hi - prev->lo - 1)] : 0;
    }
  else                                                   /* this shard's slice of the text image */
    { const uint64_t base = a->off[j->lo];
      hdr4  = a->hdr4 + 4 * j->lo;
      lwell = j->lo ? a->hdr4[4 * (j->lo - 1)] : 0;
      span  = a->off[j->hi - 1] + 5 * ((uint64_t) a->len[j->hi - 1] + 1) - base;
      roff  = malloc(m * sizeof(*roff));
      if (!roff) return DX_E_NOMEM;
      for (i = 0; i < m; i++) roff[i] = a->off[j->lo + i] - base;
      TRY(dupload(pool, a->text + base, span, &d_text));
      TRY(dupload(pool, roff, m * 8, &d_off));
      TRY(dupload(pool, a->len + j->lo, m * 4, &d_len));
    }
  TRY(qv_stage(pool, hdr4, m, &lwell, d_text, d_off, d_len, span, 1, st));
  TRY(dx_qv_prescan(j->ctx, &st->b, j->lo, &j->p));
done:
  free(roff);
  return rc;
}

/* the file's first 100000 symbols (QV.c:1006-1015) reach beyond shard 0: the provisional subChar from a prefix batch of
   entries [0, cut] instead */
static int shard_prefix_sub(shard_job *j, dpool *pool)
{ shard_all   *a = j->all;
  const uint64_t mp = a->cut + 1, sp = a->off[a->cut] + 5 * ((uint64_t) a->len[a->cut] + 1) - a->off[0];
  uint64_t    *po = malloc(mp * sizeof(*po)), i;
  void        *pt = NULL, *pd_off = NULL, *pd_len = NULL;
  dx_qv_batch  pb;
  dx_qv_params pp = { 0, -1, 0, -1 };                     /* delChar "set": only the sub search runs */
  int          rc;
  if (po == NULL) return DX_E_NOMEM;
  for (i = 0; i < mp; i++) po[i] = a->off[i] - a->off[0];
  TRY(dupload(pool, a->text + a->off[0], sp, &pt));
  TRY(dupload(pool, po, mp * 8, &pd_off));
  TRY(dupload(pool, a->len, mp * 4, &pd_len));
  pb = qv_batch(pt, pd_off, pd_len, mp, sp, 1);
  TRY(dx_qv_prescan(j->ctx, &pb, 0, &pp));
done:
  j->p.subChar = pp.subChar; j->p.sub_first = pp.sub_first;
  free(po);
  return rc;
}

static void *shard_main(void *arg)
{ shard_job  *j = arg;
  shard_all  *a = j->all;
  dpool       pool = { {0}, 0, j->ctx };
  uint64_t    m = j->hi - j->lo, span = 0, total = 0;
  void       *d_text = NULL, *d_off = NULL, *d_len = NULL, *d_out = NULL;
  size_t      out_cap = 0;
  qv_staged   st;
  int         rc = DX_OK, k;

  pthread_mutex_lock(&a->gate_mx);                        /* all threads exist, or none runs */
  while (a->go == 0) pthread_cond_wait(&a->gate_cv, &a->gate_mx);
  k = a->go;
  pthread_mutex_unlock(&a->gate_mx);
  if (k < 0) return NULL;

  memset(&st, 0, sizeof(st));
  j->p.delChar = j->p.subChar = -1; j->p.del_first = j->p.sub_first = -1;
  memset(j->hist, 0, sizeof(j->hist)); j->tot = 0; j->bytes = 0;

  if (a->by_bytes)
    { rc = shard_slice(j, &pool, &d_text, &d_off, &d_len, &span);        /* (five barriers inside, whatever becomes of it) */
      m = j->hi - j->lo;
    }
  if (rc == DX_OK && m > 0)
    rc = shard_stage(j, &pool, d_text, d_off, d_len, span, &st);
  if (rc == DX_OK && j->id == 0 && a->cut >= j->hi && !a->by_bytes)      /* (by bytes: shard_slice has seen to it that this is not so) */
    rc = shard_prefix_sub(j, &pool);
  j->rc = rc;
  pthread_barrier_wait(&a->bar);

  if (j->id == 0 && (a->ok = all_ok(a)))                 /* merge the scan state (lowest entry wins) */
    { a->p.delChar = a->p.subChar = -1; a->p.del_first = a->p.sub_first = -1;
      for (k = 0; k < a->nsh; k++)
        if (a->jobs[k].p.delChar >= 0 && (a->p.delChar < 0 || a->jobs[k].p.del_first < a->p.del_first))
          { a->p.delChar = a->jobs[k].p.delChar; a->p.del_first = a->jobs[k].p.del_first; }
      for (k = 0; k < a->nsh; k++)
        if (a->jobs[k].lo == 0 && a->jobs[k].hi > 0)
          { a->p.subChar = a->jobs[k].p.subChar; a->p.sub_first = a->jobs[k].p.sub_first; }
    }
  pthread_barrier_wait(&a->bar);

  if (a->ok && m > 0)
    j->rc = dx_qv_hist(j->ctx, &st.b, j->lo, &a->p, j->hist, &j->tot);     /* QV.c:988-1017, per shard */
  pthread_barrier_wait(&a->bar);

  if (j->id == 0 && (a->ok = all_ok(a)))                 /* host-side sum + Create_QVcoding */
    { int s, x;
      memset(a->hist, 0, sizeof(a->hist)); a->tot = 0;
      for (k = 0; k < a->nsh; k++)
        { for (s = 0; s < 6; s++)
            for (x = 0; x < 256; x++)
              a->hist[s][x] += a->jobs[k].hist[s][x];
          a->tot += a->jobs[k].tot;
        }
      a->rc = dx_qv_build((const uint64_t (*)[256]) a->hist, a->tot, &a->p, a->lossy, &a->cd);
      a->ok = a->rc == DX_OK;
    }
  pthread_barrier_wait(&a->bar);

  if (a->ok && m > 0)                                    /* Compress_Next_QVentry for the shard's entries */
    { rc = dx_qv_set_coding(j->ctx, &a->cd, a->lossy);
      if (rc == DX_OK) rc = qv_encode_batch(j->ctx, &st, (const uint64_t (*)[256]) j->hist, &a->cd, a->lossy, &d_out, &out_cap, &total);
      j->bytes = total;
      j->rc = rc;
    }
  pthread_barrier_wait(&a->bar);

  if (j->id == 0 && (a->ok = all_ok(a)))                 /* layout of the final image */
    { size_t plen = a->plen, records = 0;
      if (!a->by_bytes)
        { const uint8_t *h = a->text, *slash = memchr(h + 1, '/', (size_t) (a->off[0] - 1));
          plen = slash ? (size_t) (slash - h) : 0;
        }
      for (k = 0; k < a->nsh; k++)
        { a->jobs[k].at = records;                        /* (behind the head, once that is known) */
          records += a->jobs[k].bytes;
        }
      a->rc = qv_head(&a->cd, a->text, plen, records, &a->img, &a->head);
      for (k = 0; k < a->nsh; k++) a->jobs[k].at += a->head;
      a->total = a->head + records;
      a->ok = a->rc == DX_OK;
    }
  pthread_barrier_wait(&a->bar);

  if (a->ok && m > 0)
    j->rc = dx_d2h(j->ctx, a->img + j->at, d_out, total);
  if (d_out) (void) dx_free(j->ctx, d_out);
  dfree_all(&pool);
  return NULL;
}

/* A file too large to be indexed by one thread first (a terabyte over eight GPUs): the bytes are dealt evenly, and
 * every shard finds the records that BEGIN in its range -- a record is six lines (QV.c:948-978), so all it needs of the others is
 * how many newlines stand in front of its range --, uploads exactly those and has its own device index them (dx_index_quiva_device:
 * structure checks and all).  Anything out of the ordinary (a line count that is no multiple of six, an indexer that says no, the
 * first 100000 symbols reaching beyond shard 0) sets a->again: dx_file_dexqv_sharded then does the file the serial way, which also has
 * the reference's words for a malformed file.  Every thread passes the same five barriers.                                     */
static int shard_slice(shard_job *j, dpool *pool, void **d_text, void **d_off, void **d_len, uint64_t *span)
{ shard_all *a = j->all;
  int rc = DX_OK, k;
  { const uint8_t *q = a->text + j->p0, *e = a->text + j->p1;            /* 1: the newlines of the range as dealt */
    uint64_t c = 0;
    while (q < e && (q = memchr(q, '\n', (size_t) (e - q))) != NULL) { c += 1; q += 1; }
    j->nl = c;
  }
  pthread_barrier_wait(&a->bar);
  if (j->id == 0)                                        /* 2: the lines in front of every range; six lines a record, the last one whole */
    { uint64_t before = 0;
      for (k = 0; k < a->nsh; k++) { a->jobs[k].line0 = before; before += a->jobs[k].nl; }
      if (before % 6 != 0 || before == 0 || a->text[a->n - 1] != '\n') a->again = 1;
      a->cnt = before / 6;
    }
  pthread_barrier_wait(&a->bar);
  if (!a->again)                                         /* 3: the first record that begins in the range */
    { const uint8_t *q = a->text + j->p0, *e = a->text + a->n;
      uint64_t line = j->line0;                            /* (the line p0 stands in) */
      if (j->p0 > 0 && q[-1] != '\n')                       /* ... which began in front of the range: the next one */
        { q = memchr(q, '\n', (size_t) (e - q)); q = q ? q + 1 : e; line += 1; }
      while (line % 6 != 0 && q < e)
        { q = memchr(q, '\n', (size_t) (e - q)); q = q ? q + 1 : e; line += 1; }
      j->start = (size_t) (q - a->text);
      j->lo = line / 6;
    }
  pthread_barrier_wait(&a->bar);
  if (!a->again)                                         /* 4: the shard's records, to its device, indexed there */
    { const size_t end = j->id + 1 < a->nsh ? a->jobs[j->id + 1].start : a->n;
      uint64_t cnt = 0, el = 0;
      int      ec = 0;
      j->hi = j->id + 1 < a->nsh ? a->jobs[j->id + 1].lo : a->cnt;
      *span = end - j->start;
      if (j->hi > j->lo)
        { uint64_t *go = NULL; uint32_t *gl = NULL;
          size_t plen = 0;
          rc = dupload(pool, a->text + j->start, (size_t) *span, d_text);
          if (rc == DX_OK) rc = dx_index_quiva_device(j->ctx, *d_text, *span, &go, &gl, &cnt, &j->hdr4, &plen, &el, &ec);
          if (rc == DX_OK && cnt > 0) { pool->p[pool->n++] = go; pool->p[pool->n++] = gl; *d_off = go; *d_len = gl; }
          if (rc == DX_OK && cnt != j->hi - j->lo) rc = DX_E_FORMAT;
          if (rc == DX_OK && (j->len = malloc((size_t) cnt * 4)) == NULL) rc = DX_E_NOMEM;
          if (rc == DX_OK) rc = dx_d2h(j->ctx, j->len, gl, (size_t) cnt * 4);
          if (j->id == 0) a->plen = plen;
        }
      else if (j->hi < j->lo) rc = DX_E_FORMAT;
      if (rc != DX_OK) { j->rc = rc; }
    }
  pthread_barrier_wait(&a->bar);
  if (j->id == 0 && !a->again)                           /* the entry at which the running symbol count reaches 100000 (QV.c:1006-1015) */
    { uint64_t run = 0, e2 = 0, m0 = a->jobs[0].hi - a->jobs[0].lo;
      for (k = 0; k < a->nsh; k++) if (a->jobs[k].rc != DX_OK || a->jobs[k].hi <= a->jobs[k].lo) a->again = 1;
      for (e2 = 0; !a->again && e2 < m0; e2++)
        { run += a->jobs[0].len[e2];
          if (run >= 100000) break;
        }
      if (!a->again && e2 >= m0) a->again = 1;             /* (not within shard 0: a small file, the serial way knows what to do) */
      a->cut = e2;
    }
  pthread_barrier_wait(&a->bar);
  if (a->again) { j->hi = j->lo; return DX_E_FORMAT; }
  return rc;
}

#define DX_SHARD_BYTES_MIN ((size_t) 64 << 20)           /* per shard: from here on the shards index their own byte ranges */
int dx_file_dexqv_sharded(dx_ctx **ctxs, int nctx, const uint8_t *text, size_t n, int lossy,
                          uint8_t **out, size_t *out_len, uint64_t *errline, int *errcode)
{ shard_all  a;
  pthread_t *th = NULL;
  quiva_index qx = { 0, NULL, NULL, NULL, 0 };
  int        rc, k, started = 0, by_bytes;

  if (ctxs == NULL || nctx < 1 || out == NULL || out_len == NULL) return DX_E_ARG;
  if (nctx == 1) return dx_file_dexqv(ctxs[0], text, n, lossy, out, out_len, errline, errcode);
  *out = NULL; *out_len = 0;
  { const size_t least = (size_t) dx_test_num("shard_bytes_min", (long long) DX_SHARD_BYTES_MIN);     /* (tests: the by-bytes way on small files) */
    by_bytes = n / (size_t) nctx >= least && n / (size_t) nctx >= 4096 && !dx_test_on("host_index");
  }
again:
  memset(&a, 0, sizeof(a));
  started = 0;
  a.jobs = calloc((size_t) nctx, sizeof(*a.jobs));
  th = calloc((size_t) nctx, sizeof(*th));
  if (!a.jobs || !th) { rc = DX_E_NOMEM; goto done; }
  a.nsh = nctx; a.lossy = lossy; a.text = text; a.n = n; a.rc = DX_OK; a.by_bytes = by_bytes;

  if (!by_bytes)                                          /* the whole file indexed here first (small files; what the shards turn down) */
    { TRY(quiva_index_host(&qx, text, n, errline, errcode));
      a.off = qx.off; a.len = qx.len; a.hdr4 = qx.hdr4; a.cnt = qx.cnt;
      { uint64_t run = 0, e;
        a.cut = 0;
        for (e = 0; e < qx.cnt; e++)
          { run += qx.len[e];
            if (run >= 100000) break;
          }
        a.cut = e < qx.cnt ? e : 0;             /* never reached: no subChar at all, shard 0 finds that too */
      }
    }
  pthread_barrier_init(&a.bar, NULL, (unsigned) nctx);
  pthread_mutex_init(&a.gate_mx, NULL);
  pthread_cond_init(&a.gate_cv, NULL);
  a.go = 0; a.ok = 1;
  { uint64_t per = qx.cnt / (uint64_t) nctx, extra = qx.cnt % (uint64_t) nctx, lo = 0;
    for (k = 0; k < nctx; k++)
      { uint64_t m = per + ((uint64_t) k < extra ? 1 : 0);
        a.jobs[k].all = &a; a.jobs[k].ctx = ctxs[k]; a.jobs[k].id = k;
        a.jobs[k].lo = lo; a.jobs[k].hi = lo + m; a.jobs[k].rc = DX_OK;
        lo += m;
        a.jobs[k].p0 = (size_t) ((unsigned __int128) n * (unsigned) k / (unsigned) nctx);        /* (by bytes: the range as dealt) */
        a.jobs[k].p1 = (size_t) ((unsigned __int128) n * (unsigned) (k + 1) / (unsigned) nctx);
      }
  }
  for (k = 0; k < nctx; k++)                              /* the barriers count nctx threads: all of them or none */
    { if (pthread_create(&th[k], NULL, shard_main, &a.jobs[k]) != 0) break;
      started += 1;
    }
  pthread_mutex_lock(&a.gate_mx);
  a.go = started == nctx ? 1 : -1;
  pthread_cond_broadcast(&a.gate_cv);
  pthread_mutex_unlock(&a.gate_mx);
  for (k = 0; k < started; k++)
    pthread_join(th[k], NULL);
  if (started < nctx)
    rc = DX_E_NOMEM;
  else
    { rc = a.rc;
      for (k = 0; k < nctx && rc == DX_OK; k++)
        rc = a.jobs[k].rc;
    }
  if (rc == DX_OK && !a.again)
    { *out = a.img; *out_len = a.total; a.img = NULL; }

  pthread_barrier_destroy(&a.bar);
  pthread_mutex_destroy(&a.gate_mx);
  pthread_cond_destroy(&a.gate_cv);
done:
  for (k = 0; a.jobs != NULL && k < nctx; k++) { free(a.jobs[k].hdr4); free(a.jobs[k].len); }
  quiva_index_free(&qx);
  memset(&qx, 0, sizeof(qx));
  free(a.jobs); free(th); free(a.img);
  th = NULL;
  if (by_bytes && a.again && started == nctx)            /* the shards turned the file down: the serial way (and its words for what is wrong) */
    { by_bytes = 0;
      goto again;
    }
  return rc;
}

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
  TRY(qv_stage(&pool, NULL, e->n, NULL, d_text, d_off, d_len, e->tlen, 0, &st));      /* (line_pad 0, no framing bytes) */
  TRY(dx_qv_scan(ctx, &st.b, 0, &p, hist, &tot));          /* QVcoding_Scan1 over all entries */
  TRY(dx_qv_build((const uint64_t (*)[256]) hist, tot, &p, lossy, coding));   /* Create_QVcoding */
  TRY(dx_qv_set_coding(ctx, coding, lossy));
  TRY(qv_encode_batch(ctx, &st, (const uint64_t (*)[256]) hist, coding, lossy, &d_out, &out_cap, &total));     /* Compress_Next_QVentry1 x n */
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
 *  ... and the read side: Load_QVentry (DB.c:2575-2621) = a seek to DAZZ_READ.coff and
 *  Uncompress_Next_QVentry (QV.c:1428-1481) with the read's length, for any read in any order -- as
 *  a batch: the selected records' segment sizes by dx_qv_walk_records_device (a lane a record), then
 *  dx_qv_decode with the entries' starts as d_rec_off and no framing bytes.
 *
 *  What travels: a record's size is not stored, but it has a bound -- every line's symbols at the
 *  longest code of its scheme (a run-coded line: a token for every symbol), and the tags.  The
 *  selection's spans [coff, coff + bound) are merged; when they cover less than HALF of the stream
 *  they go up packed side by side (a slice's own spans per slice), else the whole stream goes up
 *  once -- unless the stream, with a slice of 4 MB of text beside it, is more than the device has
 *  free: then the packed way is taken whatever is selected, since a slice's spans are what has to
 *  fit.  A record must end inside its span: one that does not is DX_E_FORMAT in either case.
 * ========================================================================================== */
typedef struct { uint64_t lo, hi, j; } rspan;

static int rspan_cmp(const void *a, const void *b)
{ const rspan *x = a, *y = b;
  return x->lo < y->lo ? -1 : x->lo > y->lo ? 1 : x->j < y->j ? -1 : x->j > y->j;
}

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

/* sp[0 .. m): the spans of the stream that entries j0 .. j0 + m - 1 of the selection can reach, sp[k].j = k */
static void spans_of(rspan *sp, uint64_t j0, uint64_t m, const uint64_t *ids, const uint64_t *coff, const uint32_t *len,
                     const uint32_t bits[4], uint64_t nbytes)
{ uint64_t k;
  for (k = 0; k < m; k++)
    { const uint64_t lo = coff[ids ? ids[j0 + k] : j0 + k], most = record_bytes_most(len[j0 + k], bits);
      sp[k].lo = lo; sp[k].j = k;
      sp[k].hi = nbytes - lo < most ? nbytes : lo + most;
    }
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

int dx_entries_uncompress(dx_ctx *ctx, const dx_qv_coding *coding, int flip,
                          const uint8_t *records, size_t nbytes, const uint64_t *coff, const uint32_t *rlen,
                          const uint64_t *ids, uint64_t n_ids,
                          int ascii, uint8_t **text, size_t *text_bytes, uint64_t **toff)
{ dpool     all = { {0}, 0, ctx }, pool = { {0}, 0, ctx };
  rspan    *sp = NULL;
  uint64_t *to = NULL, *rel = NULL, j, j0, j1, covered;
  uint32_t *len = NULL, *seg = NULL, bits[4];
  uint8_t  *res = NULL, *stage = NULL;
  void     *d_whole = NULL;
  size_t    cap;
  int       rc = DX_OK, whole;

  if (ctx == NULL || coding == NULL || text == NULL || text_bytes == NULL || toff == NULL || ascii < 0 || ascii > 2) return DX_E_ARG;
  if (n_ids > 0 && (coff == NULL || rlen == NULL || (records == NULL && nbytes > 0))) return DX_E_ARG;
  *text = NULL; *text_bytes = 0; *toff = NULL;
  to  = malloc((n_ids + 1) * sizeof(*to));
  sp  = malloc((n_ids + 1) * sizeof(*sp));
  rel = malloc((n_ids + 1) * sizeof(*rel));
  len = malloc((n_ids + 1) * sizeof(*len));
  seg = malloc((n_ids + 1) * 5 * sizeof(*seg));
  if (!to || !sp || !rel || !len || !seg) { rc = DX_E_NOMEM; goto done; }

  /* the text's layout, and every entry's span of the stream */
  bits[0] = line_bits_most(coding, DX_DEL, coding->delChar >= 0 ? DX_DRUN : -1);
  bits[1] = line_bits_most(coding, DX_INS, -1);
  bits[2] = line_bits_most(coding, DX_MRG, -1);
  bits[3] = line_bits_most(coding, DX_SUB, coding->subChar >= 0 ? DX_SRUN : -1);
  to[0] = 0;
  for (j = 0; j < n_ids; j++)
    { const uint64_t id = ids ? ids[j] : j, L = rlen[id];
      if (L > 0x7fffffffu || coff[id] > nbytes)
        { rc = dx_entry_fail(ctx, id, coff[id], nbytes); goto done; }
      len[j] = (uint32_t) L;
      to[j + 1] = to[j] + 5 * (L + 1);
    }
  res = malloc((size_t) to[n_ids] + 16);
  if (res == NULL) { rc = DX_E_NOMEM; goto done; }
  if (n_ids == 0) goto deliver;

  spans_of(sp, 0, n_ids, ids, coff, len, bits, nbytes);
  covered = spans_pack(sp, n_ids, records, NULL, NULL);
  whole   = sel_goes_whole(ctx, covered, nbytes, "entries_packed", "entries_whole");
  cap = out_cap(ctx, whole ? nbytes : (size_t) covered, (size_t) to[n_ids], n_ids);
  TRY(dx_qv_set_coding(ctx, coding, 0));
  if (whole) TRY(dupload(&all, records, nbytes, &d_whole));
  else                                                    /* (no slice's spans are more than the selection's) */
    { stage = malloc((size_t) covered + 16);
      if (stage == NULL) { rc = DX_E_NOMEM; goto done; }
    }

  for (j0 = 0; j0 < n_ids; j0 = j1)                       /* slices of whole entries: at most cap bytes of text each (0: all at once) */
    { void    *d_in = d_whole, *d_start, *d_len, *d_seg, *d_ooff, *d_out;
      uint64_t m, in_bytes = nbytes, bad = UINT64_MAX;
      j1 = sel_slice_end(to, j0, n_ids, cap);
      m  = j1 - j0;
      if (whole)
        for (j = 0; j < m; j++) rel[j] = coff[ids ? ids[j0 + j] : j0 + j];
      else                                                /* this slice's spans, packed */
        { spans_of(sp, j0, m, ids, coff, len, bits, nbytes);
          in_bytes = spans_pack(sp, m, records, stage, rel);
          TRY(dupload(&pool, stage, (size_t) in_bytes, &d_in));
        }
      TRY(dupload(&pool, rel, m * 8, &d_start));
      TRY(dupload(&pool, len + j0, m * 4, &d_len));
      TRY(dalloc(&pool, m * 20, &d_seg));
      TRY(dalloc(&pool, m * 8, &d_ooff));
      for (j = 0; j < m; j++) rel[j] = to[j0 + j] - to[j0];   /* the entries' places in the slice's text */
      TRY(dx_h2d(ctx, d_ooff, rel, m * 8));
      TRY(dalloc(&pool, (size_t) (to[j1] - to[j0]), &d_out));
      rc = dx_qv_walk_records_device(ctx, d_in, in_bytes, d_start, d_len, m, coding, flip, d_seg, &bad);
      if (rc == DX_E_FORMAT && bad != UINT64_MAX)
        { const uint64_t id = ids ? ids[j0 + bad] : j0 + bad;
          rc = dx_entry_fail(ctx, id, coff[id], nbytes);
        }
      if (rc != DX_OK) goto done;
      if (!whole)                                         /* a record ends inside its own span, not in a neighbour's bytes */
        { TRY(dx_d2h(ctx, seg, d_seg, m * 20));
          for (j = 0; j < m; j++)
            { const uint64_t id = ids ? ids[j0 + j] : j0 + j;
              uint64_t used = 0;
              int k;
              for (k = 0; k < 5; k++) used += seg[5 * j + k];
              if (used > record_bytes_most(len[j0 + j], bits) || used > nbytes - coff[id])
                { rc = dx_entry_fail(ctx, id, coff[id], nbytes); goto done; }
            }
        }
      TRY(dx_qv_decode(ctx, d_in, d_start, NULL, d_seg, d_len, m, (ascii == 2 ? DX_DECODE_UPPER : 0) | (flip ? DX_DECODE_FLIP : 0), d_out, d_ooff));
      TRY(dx_d2h(ctx, res + to[j0], d_out, (size_t) (to[j1] - to[j0])));
      dfree_all(&pool);
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
  dfree_all(&pool);
  dfree_all(&all);
  free(sp); free(rel); free(len); free(seg); free(stage); free(res); free(to);
  return rc;
}

/* ==========================================================================================
 *  The .bps / .arw read side: Load_Read (DB.c:1232-1298), Load_Subread (DB.c:1308-1381), Load_Arrow
 *  (DB.c:1508-1548) for a selection at once, in Load_All_Reads' layout (DB.c:1406-1433) -- dx_reads_unpack
 *  on the selected units.  What travels is decided as for a .qvs track above, but a unit's span of the
 *  payload is exact: bytes [boff + beg / 4, boff + (end - 1) / 4 + 1), cut at the payload's end.  A
 *  span that is cut ends the packed layout as it ends the payload, so the unit reaches past the end of
 *  what the device has either way, and the kernel's own check finds it.
 * ========================================================================================== */
int dx_reads_uncompress(dx_ctx *ctx, int letters, const uint8_t *payload, size_t nbytes,
                        const uint64_t *boff, const uint32_t *rlen,
                        const uint64_t *ids, const uint32_t *beg, const uint32_t *end, uint64_t n_ids,
                        uint8_t **text, size_t *text_bytes, uint64_t **toff)
{ dpool     all = { {0}, 0, ctx }, pool = { {0}, 0, ctx };
  rspan    *sp = NULL, *un = NULL;                        /* un[j]: unit j's span; sp: a slice's, as spans_pack sorts them */
  uint64_t *to = NULL, *rel = NULL, *at = NULL, j, j0, j1, covered;   /* at[j]: where unit j's first byte is, cut or not */
  uint32_t *len = NULL, *ph = NULL;
  uint8_t  *res = NULL, *stage = NULL;
  void     *d_whole = NULL;
  size_t    cap;
  int       rc = DX_OK, whole;
  const uint8_t delim = letters == DX_LETTERS_NUMBERS ? 4 : 0;    /* DB.c:362 / DB.c:367-389 */

  if (ctx == NULL || text == NULL || text_bytes == NULL || toff == NULL || letters < DX_LETTERS_LOWER || letters > DX_LETTERS_NUMBERS)
    return DX_E_ARG;
  if ((beg == NULL) != (end == NULL)) return DX_E_ARG;
  if (n_ids > 0 && (boff == NULL || rlen == NULL || (payload == NULL && nbytes > 0))) return DX_E_ARG;
  *text = NULL; *text_bytes = 0; *toff = NULL;
  to  = malloc((n_ids + 1) * sizeof(*to));
  sp  = malloc((n_ids + 1) * sizeof(*sp));
  un  = malloc((n_ids + 1) * sizeof(*un));
  rel = malloc((n_ids + 1) * sizeof(*rel));
  at  = malloc((n_ids + 1) * sizeof(*at));
  len = malloc((n_ids + 1) * sizeof(*len));
  ph  = malloc((n_ids + 1) * sizeof(*ph));
  if (!to || !sp || !un || !rel || !at || !len || !ph) { rc = DX_E_NOMEM; goto done; }

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

  memcpy(sp, un, (size_t) n_ids * sizeof(*sp));
  covered = spans_pack(sp, n_ids, payload, NULL, NULL);
  whole   = sel_goes_whole(ctx, covered, nbytes, "reads_packed", "reads_whole");
  cap     = out_cap(ctx, whole ? nbytes : (size_t) covered, (size_t) to[n_ids], n_ids);
  if (whole) TRY(dupload(&all, payload, nbytes, &d_whole));
  else                                                    /* (no slice's spans are more than the selection's) */
    { stage = malloc((size_t) covered + 16);
      if (stage == NULL) { rc = DX_E_NOMEM; goto done; }
    }

  for (j0 = 0; j0 < n_ids; j0 = j1)                       /* slices of whole units: at most cap bytes of text each (0: all at once) */
    { void    *d_in = d_whole, *d_boff, *d_beg, *d_len, *d_ooff, *d_out;
      uint64_t m, in_bytes = nbytes, bad = UINT64_MAX;
      j1 = sel_slice_end(to, j0, n_ids, cap);
      m  = j1 - j0;
      if (whole)
        memcpy(rel, at + j0, (size_t) m * 8);
      else                                                /* this slice's spans, packed */
        { for (j = 0; j < m; j++) { sp[j] = un[j0 + j]; sp[j].j = j; }
          in_bytes = spans_pack(sp, m, payload, stage, rel);
          TRY(dupload(&pool, stage, (size_t) in_bytes, &d_in));
        }
      TRY(dupload(&pool, rel, m * 8, &d_boff));
      TRY(dupload(&pool, ph + j0, m * 4, &d_beg));
      TRY(dupload(&pool, len + j0, m * 4, &d_len));
      for (j = 0; j < m; j++) rel[j] = to[j0 + j] - to[j0];   /* the units' places in the slice's text */
      TRY(dupload(&pool, rel, m * 8, &d_ooff));
      TRY(dalloc(&pool, (size_t) (to[j1] - to[j0]), &d_out));
      rc = dx_reads_unpack(ctx, letters, d_in, in_bytes, d_boff, d_beg, d_len, m, d_out, d_ooff, &bad);
      if (rc == DX_E_FORMAT && bad != UINT64_MAX)         /* the caller's read, not its place in the slice */
        { const uint64_t id = ids ? ids[j0 + bad] : j0 + bad;
          rc = dx_entry_fail(ctx, id, boff[id], nbytes);
        }
      if (rc != DX_OK) goto done;
      TRY(dx_d2h(ctx, res + to[j0], d_out, (size_t) (to[j1] - to[j0])));
      dfree_all(&pool);
    }

deliver:
  *text = res; *text_bytes = (size_t) to[n_ids]; *toff = to;
  res = NULL; to = NULL;
  rc = DX_OK;

done:
  dfree_all(&pool);
  dfree_all(&all);
  free(sp); free(un); free(rel); free(at); free(len); free(ph); free(stage); free(res); free(to);
  return rc;
}
