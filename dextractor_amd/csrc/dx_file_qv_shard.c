/*
 * dx_file_qv_shard.c -- dexqv of one file on several GPUs: contiguous entry ranges, one host thread per context;
 * the only exchange is on the host -- the merged scan state (32 bytes) and the sum of the 12 KB histograms -- after which every
 * shard is encoded with identical tables and the record streams are concatenated in order.  No RCCL.
 *
 * The threads are a crew (dx_crew.h) and a run is a table of phases: what every shard does on its own device is a phase's work,
 * what shard 0 folds from the shards' results is its fold.  No function in this file waits at a barrier.
 */
#include <stdlib.h>
#include <string.h>

#include "dexgpu.h"
#include "dx_env.h"
#include "dx_crew.h"
#include "dx_files.h"

typedef struct shard_job shard_job;

typedef struct
  { int               nsh, lossy, rc;
    int               ok;                    /* the verdict: written by shard 0 in a fold, read by all in the work phases behind it */
    const uint8_t    *text;
    size_t            n;
    quiva_index       qx;                    /* by entries: the file's host index; by bytes: cnt alone, from the shards' line counts */
    uint64_t          cut;                   /* by entries: the entry at which the running symbol count reaches QV_SUB_SYMBOLS */
    dx_qv_params      p;
    dx_qv_coding      cd;
    uint64_t          hist[6][256], tot;
    uint8_t          *img;
    size_t            head, total;
    shard_job        *jobs;
    /* by bytes (large files): no index of the whole file exists; every shard finds and indexes its own records (the slice_ phases) */
    int               by_bytes, again;       /* again: something is not as it should be -- the whole file once more, the serial way */
  } shard_all;

struct shard_job
  { shard_all   *all;
    dx_ctx      *ctx;
    int          id, rc;
    uint64_t     lo, hi;                      /* entries [lo, hi) */
    dx_qv_params p;
    uint64_t     hist[6][256], tot, bytes, at;
    /* on the shard's device from phase to phase, released in the last one: its entries' text and index (in), what the encoder wants
       beside them (st), the records (d_out) */
    dpool        pool;
    dx_qv_batch  in;
    qv_staged    st;
    void        *d_out;
    size_t       out_cap;
    /* by bytes: the shard's byte range as dealt, the newlines in it, where its first record begins and the line that is, its own
       index (hdr4 / len: host, the shard's entries; the offsets stay on the device), the length of the prefix it found there */
    size_t       p0, p1, start, plen;
    uint64_t     nl, line0;
    int32_t     *hdr4;
    uint32_t    *len;
  };

/* shard 0 reads the others' rc only in a fold (nobody writes then) */
static int all_ok(shard_all *a)
{ int k;
  for (k = 0; k < a->nsh; k++)
    if (a->jobs[k].rc != DX_OK) return 0;
  return a->rc == DX_OK;
}

/* The file's first QV_SUB_SYMBOLS symbols decide its subChar (QV.c:1006-1015): the entry of len[0 .. m) at which the running symbol
   count reaches that many; m: it never does */
#define QV_SUB_SYMBOLS 100000
static uint64_t sub_cut(const uint32_t *len, uint64_t m)
{ uint64_t run = 0, e;
  for (e = 0; e < m; e++)
    { run += len[e];
      if (run >= QV_SUB_SYMBOLS) break;
    }
  return e;
}

/* entries [e0, e1) of a host-indexed text cut out into `pool`: their text, where each begins in it, their lengths */
static int quiva_cut(dpool *pool, const uint8_t *text, const quiva_index *qx, uint64_t e0, uint64_t e1, dx_qv_batch *b)
{ const uint64_t m = e1 - e0, base = qx->off[e0], span = dxf_quiva_end(qx, e1 - 1) - base;
  uint64_t *rel = malloc(m * sizeof(*rel)), i;
  void     *d_text, *d_off, *d_len;
  int       rc;
  if (rel == NULL) return DX_E_NOMEM;
  for (i = 0; i < m; i++) rel[i] = qx->off[e0 + i] - base;
  TRY(dupload(pool, text + base, span, &d_text));
  TRY(dupload(pool, rel, m * 8, &d_off));
  TRY(dupload(pool, qx->len + e0, m * 4, &d_len));
  *b = dxf_qv_batch(d_text, d_off, d_len, m, span, 1);
done:
  free(rel);
  return rc;
}

/* ---- by bytes: every shard finds, uploads and indexes its own records ---------------------------------------------------------
 * A file too large to be indexed by one thread first (a terabyte over eight GPUs): the bytes are dealt evenly, and
 * every shard finds the records that BEGIN in its range -- a record is six lines (QV.c:948-978), so all it needs of the others is
 * how many newlines stand in front of its range --, uploads exactly those and has its own device index them (dx_index_quiva_device:
 * structure checks and all).  Anything out of the ordinary (a line count that is no multiple of six, an indexer that says no, a
 * range in which no record begins, the first QV_SUB_SYMBOLS symbols reaching beyond shard 0) sets a->again: dx_file_dexqv_sharded
 * then does the file the serial way, which also has the reference's words for a malformed file.                              */

/* the newlines of the range as dealt */
static void slice_newlines(void *arg)
{ shard_job *j = arg;
  const uint8_t *q = j->all->text + j->p0, *e = j->all->text + j->p1;
  uint64_t c = 0;
  while (q < e && (q = memchr(q, '\n', (size_t) (e - q))) != NULL) { c += 1; q += 1; }
  j->nl = c;
}

/* the lines in front of every range; six lines a record, the last one whole */
static void slice_lines(void *arg)
{ shard_all *a = arg;
  uint64_t before = 0;
  int k;
  for (k = 0; k < a->nsh; k++) { a->jobs[k].line0 = before; before += a->jobs[k].nl; }
  if (before % 6 != 0 || before == 0 || a->text[a->n - 1] != '\n') a->again = 1;
  a->qx.cnt = before / 6;
}

/* the first record that begins in the range */
static void slice_start(void *arg)
{ shard_job *j = arg;
  shard_all *a = j->all;
  const uint8_t *q = a->text + j->p0, *e = a->text + a->n;
  uint64_t line = j->line0;                               /* (the line p0 stands in) */
  if (a->again) return;
  if (j->p0 > 0 && q[-1] != '\n')                          /* ... which began in front of the range: the next one */
    { q = memchr(q, '\n', (size_t) (e - q)); q = q ? q + 1 : e; line += 1; }
  while (line % 6 != 0 && q < e)
    { q = memchr(q, '\n', (size_t) (e - q)); q = q ? q + 1 : e; line += 1; }
  j->start = (size_t) (q - a->text);
  j->lo = line / 6;
}

/* the shard's records, to its device, indexed there */
static void slice_index(void *arg)
{ shard_job *j = arg;
  shard_all *a = j->all;
  const shard_job *next = j->id + 1 < a->nsh ? &a->jobs[j->id + 1] : NULL;
  const uint64_t span = (next ? next->start : a->n) - j->start;
  uint64_t *go = NULL, cnt = 0, el = 0;
  uint32_t *gl = NULL;
  void     *d_text;
  size_t    plen = 0;
  int       rc, ec = 0;
  if (a->again) return;
  j->hi = next ? next->lo : a->qx.cnt;
  if (j->hi < j->lo) { j->rc = DX_E_FORMAT; return; }
  if (j->hi == j->lo) return;
  TRY(dupload(&j->pool, a->text + j->start, (size_t) span, &d_text));
  TRY(dx_index_quiva_device(j->ctx, d_text, span, &go, &gl, &cnt, &j->hdr4, &plen, &el, &ec));
  if (cnt > 0 && (dadopt(&j->pool, go) | dadopt(&j->pool, gl))) { rc = DX_E_NOMEM; goto done; }      /* (each of them, whatever becomes of the other) */
  if (cnt != j->hi - j->lo) { rc = DX_E_FORMAT; goto done; }
  if ((j->len = malloc((size_t) cnt * 4)) == NULL) { rc = DX_E_NOMEM; goto done; }
  TRY(dx_d2h(j->ctx, j->len, gl, (size_t) cnt * 4));
  j->in = dxf_qv_batch(d_text, go, gl, cnt, span, 1);
  j->plen = plen;
done:
  j->rc = rc;
}

/* every range has its records, and the running symbol count reaches QV_SUB_SYMBOLS within shard 0's (else: a small file, the serial
   way knows what to do) */
static void slice_verdict(void *arg)
{ shard_all *a = arg;
  const shard_job *j0 = &a->jobs[0];
  int k;
  if (a->again) return;
  for (k = 0; k < a->nsh; k++)
    if (a->jobs[k].rc != DX_OK || a->jobs[k].hi <= a->jobs[k].lo) a->again = 1;
  if (!a->again && sub_cut(j0->len, j0->hi - j0->lo) >= j0->hi - j0->lo) a->again = 1;
}

/* ---- the phases both ways share ------------------------------------------------------------------------------------------- */

/* the file's first QV_SUB_SYMBOLS symbols reach beyond shard 0: the provisional subChar from a prefix batch of entries [0, cut]
   instead */
static int shard_prefix_sub(shard_job *j)
{ shard_all   *a = j->all;
  dx_qv_batch  pb;
  dx_qv_params pp = { 0, -1, 0, -1 };                     /* delChar "set": only the sub search runs */
  int          rc;
  TRY(quiva_cut(&j->pool, a->text, &a->qx, 0, a->cut + 1, &pb));
  TRY(dx_qv_prescan(j->ctx, &pb, 0, &pp));
done:
  j->p.subChar = pp.subChar; j->p.sub_first = pp.sub_first;
  return rc;
}

/* The shard's entries staged on its device and prescanned (QV.c:993-1015, per shard).  By bytes, slice_index has put text and index
   there; else they are cut from the file's host index here. */
static void shard_stage(void *arg)
{ shard_job *j = arg;
  shard_all *a = j->all;
  const int32_t *hdr4 = j->hdr4;
  int32_t    lwell;
  int        rc = DX_OK;
  if (a->again) { j->hi = j->lo; j->rc = DX_E_FORMAT; return; }
  if (j->hi > j->lo)
    { if (a->by_bytes)
        { const shard_job *prev = &a->jobs[j->id ? j->id - 1 : 0];
          lwell = j->id ? prev->hdr4[4 * (prev->hi - prev->lo - 1)] : 0;
        }
      else                                                /* this shard's slice of the text image */
        { hdr4  = a->qx.hdr4 + 4 * j->lo;
          lwell = j->lo ? a->qx.hdr4[4 * (j->lo - 1)] : 0;
          TRY(quiva_cut(&j->pool, a->text, &a->qx, j->lo, j->hi, &j->in));
        }
      TRY(dxf_qv_stage(&j->pool, hdr4, j->hi - j->lo, &lwell, j->in.d_text, j->in.d_off, j->in.d_len, j->in.text_bytes, 1, &j->st));
      TRY(dx_qv_prescan(j->ctx, &j->st.b, j->lo, &j->p));
    }
  if (j->id == 0 && !a->by_bytes && a->cut >= j->hi)      /* (by bytes: slice_verdict has seen to it that this is not so) */
    TRY(shard_prefix_sub(j));
done:
  j->rc = rc;
}

/* merge the scan state (lowest entry wins) */
static void fold_scan(void *arg)
{ shard_all *a = arg;
  int k;
  if (!(a->ok = all_ok(a))) return;
  a->p.delChar = a->p.subChar = -1; a->p.del_first = a->p.sub_first = -1;
  for (k = 0; k < a->nsh; k++)
    if (a->jobs[k].p.delChar >= 0 && (a->p.delChar < 0 || a->jobs[k].p.del_first < a->p.del_first))
      { a->p.delChar = a->jobs[k].p.delChar; a->p.del_first = a->jobs[k].p.del_first; }
  for (k = 0; k < a->nsh; k++)
    if (a->jobs[k].lo == 0 && a->jobs[k].hi > 0)
      { a->p.subChar = a->jobs[k].p.subChar; a->p.sub_first = a->jobs[k].p.sub_first; }
}

/* QV.c:988-1017, per shard */
static void shard_hist(void *arg)
{ shard_job *j = arg;
  if (j->all->ok && j->hi > j->lo)
    j->rc = dx_qv_hist(j->ctx, &j->st.b, j->lo, &j->all->p, j->hist, &j->tot);
}

/* host-side sum + Create_QVcoding */
static void fold_hist(void *arg)
{ shard_all *a = arg;
  int k, s, x;
  if (!(a->ok = all_ok(a))) return;
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

/* Compress_Next_QVentry for the shard's entries */
static void shard_encode(void *arg)
{ shard_job *j = arg;
  shard_all *a = j->all;
  uint64_t   total = 0;
  int        rc;
  if (!a->ok || j->hi <= j->lo) return;
  rc = dx_qv_set_coding(j->ctx, &a->cd, a->lossy);
  if (rc == DX_OK) rc = dxf_qv_encode_batch(j->ctx, &j->st, (const uint64_t (*)[256]) j->hist, &a->cd, a->lossy, &j->d_out, &j->out_cap, &total);
  j->bytes = total;
  j->rc = rc;
}

/* layout of the final image */
static void fold_layout(void *arg)
{ shard_all *a = arg;
  size_t plen = a->jobs[0].plen, records = 0;
  int k;
  if (!(a->ok = all_ok(a))) return;
  if (!a->by_bytes)
    { const uint8_t *h = a->text, *slash = memchr(h + 1, '/', (size_t) (a->qx.off[0] - 1));
      plen = slash ? (size_t) (slash - h) : 0;
    }
  for (k = 0; k < a->nsh; k++)
    { a->jobs[k].at = records;                            /* (behind the head, once that is known) */
      records += a->jobs[k].bytes;
    }
  a->rc = dxf_qv_head(&a->cd, a->text, plen, records, &a->img, &a->head);
  for (k = 0; k < a->nsh; k++) a->jobs[k].at += a->head;
  a->total = a->head + records;
  a->ok = a->rc == DX_OK;
}

/* the shard's records to their place in the image; what the shard holds on its device released, whatever the verdict */
static void shard_download(void *arg)
{ shard_job *j = arg;
  if (j->all->ok && j->hi > j->lo)
    j->rc = dx_d2h(j->ctx, j->all->img + j->at, j->d_out, j->bytes);
  if (j->d_out) (void) dx_free(j->ctx, j->d_out);
  dfree_all(&j->pool);
}

static const dx_crew_phase shard_phases[] =
  { { slice_newlines, slice_lines   },                    /* by bytes: from here */
    { slice_start,    NULL          },
    { slice_index,    slice_verdict },
#define SHARD_BY_ENTRIES 3                                /* by entries: from here */
    { shard_stage,    fold_scan     },
    { shard_hist,     fold_hist     },
    { shard_encode,   fold_layout   },
    { shard_download, NULL          }
  };

/* one run over the contexts, by bytes or by entries; *again: the by-bytes run has turned the file down (and nothing else is to be
   made of its result) */
static int run_once(dx_ctx **ctxs, int nctx, const uint8_t *text, size_t n, int lossy, int by_bytes, int *again,
                    uint8_t **out, size_t *out_len, uint64_t *errline, int *errcode)
{ const int from = by_bytes ? 0 : SHARD_BY_ENTRIES;
  shard_all a;
  int rc, k;

  *again = 0;
  memset(&a, 0, sizeof(a));
  a.jobs = calloc((size_t) nctx, sizeof(*a.jobs));
  if (!a.jobs) return DX_E_NOMEM;
  a.nsh = nctx; a.lossy = lossy; a.text = text; a.n = n; a.rc = DX_OK; a.by_bytes = by_bytes; a.ok = 1;

  if (!by_bytes)                                          /* the whole file indexed here first (small files; what the shards turn down) */
    { TRY(dxf_quiva_index_host(&a.qx, text, n, errline, errcode));
      a.cut = sub_cut(a.qx.len, a.qx.cnt);
      if (a.cut >= a.qx.cnt) a.cut = 0;                   /* never reached: no subChar at all, shard 0 finds that too */
    }
  { uint64_t per = a.qx.cnt / (uint64_t) nctx, extra = a.qx.cnt % (uint64_t) nctx, lo = 0;
    for (k = 0; k < nctx; k++)
      { shard_job *j = &a.jobs[k];
        uint64_t m = per + ((uint64_t) k < extra ? 1 : 0);
        j->all = &a; j->ctx = ctxs[k]; j->id = k; j->rc = DX_OK;
        j->lo = lo; j->hi = lo + m;
        lo += m;
        j->p.delChar = j->p.subChar = -1; j->p.del_first = j->p.sub_first = -1;
        j->pool.ctx = ctxs[k];
        j->p0 = (size_t) ((unsigned __int128) n * (unsigned) k / (unsigned) nctx);               /* (by bytes: the range as dealt) */
        j->p1 = (size_t) ((unsigned __int128) n * (unsigned) (k + 1) / (unsigned) nctx);
      }
  }
  if (dx_crew_run(nctx, shard_phases + from, (int) (sizeof(shard_phases) / sizeof(shard_phases[0])) - from, a.jobs, sizeof(*a.jobs), &a))
    { rc = DX_E_NOMEM; goto done; }
  rc = a.rc;
  for (k = 0; k < nctx && rc == DX_OK; k++)
    rc = a.jobs[k].rc;
  *again = a.again;
  if (rc == DX_OK && !a.again)
    { *out = a.img; *out_len = a.total; a.img = NULL; }

done:
  for (k = 0; k < nctx; k++) { free(a.jobs[k].hdr4); free(a.jobs[k].len); }
  dxf_quiva_index_free(&a.qx);
  free(a.jobs); free(a.img);
  return rc;
}

#define DX_SHARD_BYTES_MIN ((size_t) 64 << 20)           /* per shard: from here on the shards index their own byte ranges */
int dx_file_dexqv_sharded(dx_ctx **ctxs, int nctx, const uint8_t *text, size_t n, int lossy,
                          uint8_t **out, size_t *out_len, uint64_t *errline, int *errcode)
{ int rc, by_bytes, again;

  if (ctxs == NULL || nctx < 1 || out == NULL || out_len == NULL) return DX_E_ARG;
  if (nctx == 1) return dx_file_dexqv(ctxs[0], text, n, lossy, out, out_len, errline, errcode);
  *out = NULL; *out_len = 0;
  { const size_t least = (size_t) dx_test_num("shard_bytes_min", (long long) DX_SHARD_BYTES_MIN);     /* (tests: the by-bytes way on small files) */
    by_bytes = n / (size_t) nctx >= least && n / (size_t) nctx >= 4096 && !dx_test_on("host_index");
  }
  rc = run_once(ctxs, nctx, text, n, lossy, by_bytes, &again, out, out_len, errline, errcode);
  if (by_bytes && again)                                  /* the shards turned the file down: the serial way (and its words for what is wrong) */
    rc = run_once(ctxs, nctx, text, n, lossy, 0, &again, out, out_len, errline, errcode);
  return rc;
}
