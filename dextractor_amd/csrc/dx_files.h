/*
 * dx_files.h -- what the file drivers share among themselves; no part of the C-ABI.
 *
 *     dx_files.c       what every driver uses, and the decoded text on its way out (header lines laid over it, slices of it)
 *     dx_file_pack2.c  dexta / dexar (whole, streamed, sharded), undexta / undexar
 *     dx_file_qv.c     dexqv (whole, sliced), undexqv plan / run
 *     dx_file_qv_shard.c  dexqv sharded: a table of phases that a crew of threads walks, one per context
 *     dx_crew.c        that crew (dx_crew.h; dx_file_pack2_sharded is a crew of one phase): the library's only barrier wait
 *     dx_file_check.c  an image of any kind and its text where it is made: dx_file_verify, dx_file_digest, dx_file_census
 *     dx_file_u2.c     the packed reads of a walked 2-bit image on the device, slice by slice: dxf_u2_slices and what decides the slices
 *     dx_select.c      the .qvs entry API, the .bps / .arw read loader
 *     dx_file_subset.c a new image cut out of an old one: dx_file_subset_layout (host), dx_file_subset
 *     dx_file_extract.c chosen records as text: dx_file_extract
 *     dx_file_compare.c how two images of the same records differ: dx_file_compare
 *     dx_file_find.c   where given sequences occur in an image's reads: dx_file_find
 *     dx_file_find_edit.c  ... within an edit distance: dx_file_find_edit, dx_file_find_edit_spans
 *     dx_file_kmers.c  the k-mers of an image's reads, counted: dx_file_kmers_add, dx_file_kmers; dx_kmer_code, dx_kmer_letters (host)
 *     dx_file_kmers_wide.c  ... for k up to 32, counted by sorting: dx_file_kmers_wide; the same k-mers as a set on the device: dx_file_kmer_set;
 *                      dx_kmer_code64, dx_kmer_letters64 (host)
 *     dx_file_kmers_files.c  ... of several images into one answer, in passes over ranges of the codes: dx_files_kmers_wide, dx_files_kmer_set
 *     dx_file_screen.c the records that share k-mers with a set: dx_file_screen; dx_screen_select (host)
 *     dx_file_screen_spans.c  WHERE a record matches the set, as joined intervals, and the image cut there: dx_file_screen_spans, dx_file_screen_cut
 *     dx_file_cut.c    what is kept of the records once the occurrences are cut out, and the image of it: dx_hits_cut_plan, dx_spans_cut_plan
 *                      (host), dx_file_cut
 *
 * A function that one of these files has for another carries the prefix dxf_ and is hidden: the library exports none of them.
 */
#ifndef DX_FILES_H
#define DX_FILES_H
#include <stddef.h>
#include <stdint.h>
#include "dexgpu.h"

#define DXF_HIDDEN __attribute__((visibility("hidden")))

#define TRY(x) do { rc = (x); if (rc != DX_OK) goto done; } while (0)

#define DX_GPU_INDEX_MIN (1u << 20)      /* .quiva images from 1 MiB on are indexed on the GPU */

/* ---- device arrays that are freed together -------------------------------------------------------------------------- */
#define DPOOL_SLOTS 24
typedef struct { void *p[DPOOL_SLOTS]; int n; dx_ctx *ctx; } dpool;

static inline int dalloc(dpool *pool, size_t bytes, void **out)
{ int rc;
  if (pool->n >= DPOOL_SLOTS) return DX_E_NOMEM;         /* pool slots exhausted */
  rc = dx_malloc(pool->ctx, bytes + 64, out);
  if (rc == DX_OK) pool->p[pool->n++] = *out;
  return rc;
}

/* a device array made elsewhere (an indexer's) joins the pool: the pool's to free from here on, or freed at once when no slot is left
   (DX_E_NOMEM, nothing else) -- never the caller's again */
static inline int dadopt(dpool *pool, void *p)
{ if (pool->n >= DPOOL_SLOTS)
    { (void) dx_free(pool->ctx, p);
      return DX_E_NOMEM;
    }
  pool->p[pool->n++] = p;
  return DX_OK;
}

static inline int dupload(dpool *pool, const void *src, size_t bytes, void **out)
{ int rc = dalloc(pool, bytes, out);
  if (rc == DX_OK && bytes) rc = dx_h2d(pool->ctx, *out, src, bytes);
  return rc;
}

/* a device array of the caller's (*p, *cap bytes of it; none yet: NULL, 0) that is to hold `need` bytes: made anew when it is too small,
   and what it held is gone then */
static inline int dgrow(dx_ctx *ctx, void **p, size_t *cap, size_t need)
{ int rc;
  if (need <= *cap) return DX_OK;
  if (*p) (void) dx_free(ctx, *p);
  *p = NULL; *cap = 0;
  if ((rc = dx_malloc(ctx, need, p)) != DX_OK) { *p = NULL; return rc; }
  *cap = need;
  return DX_OK;
}

static inline void dfree_all(dpool *pool)
{ int i;
  for (i = 0; i < pool->n; i++)
    dx_free(pool->ctx, pool->p[i]);
  pool->n = 0;
}

/* ---- dx_files.c ------------------------------------------------------------------------------------------------------ */
/* DEXGPU_TEXT_BUDGET (bytes): how much of `whole` bytes the device is to take at once.  1: the variable is set and has decided -- *cap is
   its figure (`floor` at least), or 0 for all at once (no figure, or one the whole stays under); 0: it is not set, what is free decides */
DXF_HIDDEN int dxf_budget_env(size_t whole, size_t floor, size_t *cap);

/* a sink that sees its chunks `shift` bytes further on (the record stream follows the file's head; a piece follows the pieces before it) */
typedef struct { dx_sink_fn sink; void *user; size_t shift; } shifted_sink;
static inline int pass_shifted(void *arg, uint8_t *data, size_t len, size_t at)
{ shifted_sink *h = arg;
  return h->sink(h->user, data, len, at + h->shift);
}

/* text that grows (the header lines a decoder prints): room for `more` bytes behind the len that are there */
typedef struct { char *p; size_t len, cap; } tbuf;
DXF_HIDDEN int dxf_tb_room(tbuf *b, size_t more);

/* A chunk of decoded text on its way out (dx_d2h_stream): the header lines that fall into it are laid over it.
   Entry i's text starts at ooff[i]; its header line, hd[hat[i] .. hat[i+1]), ends there.                 */
typedef struct
  { uint64_t n; const uint64_t *ooff, *hat; const char *hd;
    dx_sink_fn sink; void *user;
    size_t base;                  /* where in the text the streamed buffer starts (a slice of the entries; else 0) */
    size_t total;                 /* the whole text's bytes */
  } hdr_patch;

/* where entry i's header line starts in the text (i == n: where the text ends) */
static inline size_t text_at(const hdr_patch *h, uint64_t i)
{ return i < h->n ? (size_t) h->ooff[i] - (size_t) (h->hat[i + 1] - h->hat[i]) : h->total; }

/* a slice of whole entries from i0 on: as many as make at most `cap` bytes of text, and one at least; cap 0: all that are left */
DXF_HIDDEN uint64_t dxf_text_slice_end(const hdr_patch *h, uint64_t i0, size_t cap);

/* how much of an output of `total` bytes the device makes at once beside an input of n bytes (and 48 bytes of index a unit): 0 = all
   of it; DEXGPU_TEXT_BUDGET (bytes) when set, else what is free decides */
DXF_HIDDEN size_t dxf_out_cap(dx_ctx *ctx, size_t n, size_t total, uint64_t units);

/* What becomes of a slice of decoded text -- entries [i0, i1), `bytes` of them at d_out, the first at t0 in the whole text: DX_OK
   (the next slice), SLICE_STOP (no more slices are wanted: not an error), or an error */
typedef int (*slice_fn)(void *arg, const void *d_out, uint64_t i0, uint64_t i1, size_t t0, size_t bytes);
#define SLICE_STOP 1

/* ... out to the caller: into the text in memory (res), or through the sink of h; header lines in place either way */
typedef struct { dx_ctx *ctx; hdr_patch *h; uint8_t *res; } slice_out;
DXF_HIDDEN int dxf_slice_deliver(void *arg, const void *d_out, uint64_t i0, uint64_t i1, size_t t0, size_t bytes);

/* ---- dx_file_pack2.c ------------------------------------------------------------------------------------------------- */
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

DXF_HIDDEN int  dxf_seq_index_host(seq_index *ix, int arrow, const uint8_t *text, size_t n, uint64_t *errline, int *errcode);
DXF_HIDDEN void dxf_seq_index_free(seq_index *ix);

/* an image that arrives in pieces (dx_file_unpack2_stream): what the file's head said, the well the last record stood at, and
   how far into this piece the whole records reached (a piece may end inside a record: `more` says that more is coming) */
typedef struct { int started, flip, newv, well, more; int32_t plen; char *name; size_t consumed; } u2_state;

/* The records of a .dexta / .dexar image, walked (undexta.c:138-271, undexar.c:136-229): per read where its packed bases stand in the
   image (ioff) and how many there are (nsym), and its header line as the tool prints it (hd, from hat[i] on; hat[cnt]: their end);
   `at`: how far the whole records reached, `well`: the last one's well.  And the header's fields as the image has them, for who frames
   records anew (dx_file_subset.c): hdr4[4 i ..] = well, beg, end, qv (dexar images: 0), cnr4[4 i ..] = the four SN words (dexta: 0). */
typedef struct { uint64_t cnt, *ioff, *hat; uint32_t *nsym; tbuf hd; size_t at; int well; int32_t *hdr4; uint16_t *cnr4; } u2_index;

/* mode: DX_LETTERS_LOWER / _UPPER (dexta images) or _ARROW (dexar images); st: the image arrives in pieces (else NULL) */
DXF_HIDDEN int    dxf_u2_walk(int mode, const uint8_t *img, size_t n, u2_state *st, u2_index *x);
DXF_HIDDEN void   dxf_u2_index_free(u2_index *x);
/* the text's layout for a line width: header line, wrapped letters, read after read; ooff[i]: where read i's letters begin */
DXF_HIDDEN size_t dxf_u2_layout(const u2_index *x, uint32_t width, uint64_t *ooff);
/* a walked image's text in slices of whole reads, at most `cap` bytes of text each (0: the whole text, one slice), each to `deliver` */
DXF_HIDDEN int    dxf_unpack2_slices(dx_ctx *ctx, int mode, const uint8_t *img, size_t n, uint32_t width, const u2_index *x, const hdr_patch *h,
                                     size_t cap, slice_fn deliver, void *arg);

/* a read's header line as undexta / undexar print it (undexta.c:242, undexar.c:199-203) behind what b holds; the walk's own printer */
DXF_HIDDEN int    dxf_u2_header(tbuf *b, int arrow, const char *name, int well, int beg, int end, int qv, const uint16_t *cnr);

/* ---- dx_file_qv.c ---------------------------------------------------------------------------------------------------- */
/* The host's index of a .quiva text (dx_index_quiva): per entry where its five lines begin, how long they are, the header's four fields */
typedef struct { uint64_t cnt, *off; uint32_t *len; int32_t *hdr4; size_t plen; } quiva_index;

DXF_HIDDEN int  dxf_quiva_index_host(quiva_index *qx, const uint8_t *text, size_t n, uint64_t *errline, int *errcode);
DXF_HIDDEN void dxf_quiva_index_free(quiva_index *qx);

/* where entry e's five lines end in the text */
static inline uint64_t dxf_quiva_end(const quiva_index *qx, uint64_t e)
{ return qx->off[e] + 5 * ((uint64_t) qx->len[e] + 1); }

DXF_HIDDEN dx_qv_batch dxf_qv_batch(const void *d_text, const void *d_off, const void *d_len, uint64_t m, uint64_t span, int line_pad);

/* A batch of entries as the encoder wants it: the text (b), the framing bytes of the headers and their offsets (none of either for the bare
   record stream of the entry API), and the per-entry record offsets and segment sizes the encoder fills */
typedef struct { dx_qv_batch b; void *d_hdr, *d_hoff, *d_rec, *d_seg; uint64_t hbytes; } qv_staged;

/* m entries whose text is on the device staged in `pool` (hdr4 == NULL: no framing bytes); Compress_Next_QVentry for a staged batch */
DXF_HIDDEN int dxf_qv_stage(dpool *pool, const int32_t *hdr4, uint64_t m, int32_t *lwell, const void *d_text, const void *d_off, const void *d_len,
                            uint64_t span, int line_pad, qv_staged *s);
DXF_HIDDEN int dxf_qv_encode_batch(dx_ctx *ctx, const qv_staged *s, const uint64_t (*hist)[256], const dx_qv_coding *cd, int lossy,
                                   void **d_out, size_t *out_cap, uint64_t *total);

/* the head of a .dexqv image: the key and the coding, the prefix being the text's first plen bytes.  *img: malloc'd, `head` bytes written,
   room for `more` behind them */
DXF_HIDDEN int dxf_qv_head(const dx_qv_coding *cd, const uint8_t *text, size_t plen, size_t more, uint8_t **img, size_t *head);

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

/* an entry's header line as undexqv prints it (undexqv.c:182) behind what b holds: h4 = well, beg, end, qv; the plan's own printer */
DXF_HIDDEN int    dxf_qv_header(tbuf *b, const char *prefix, const int32_t *h4);

/* a plan's text in slices of whole entries, at most `cap` bytes of text each (0: in one), each to `deliver`; and the cap the device asks for */
DXF_HIDDEN int    dxf_undexqv_sliced(dx_ctx *ctx, const dx_undexqv_plan *p, int upper, slice_fn deliver, void *arg, size_t cap, int whole_in_);
DXF_HIDDEN size_t dxf_undexqv_cap(dx_ctx *ctx, const dx_undexqv_plan *p, int *whole_in);
/* ... and entries [r0, r1) of it alone, in slices that end at r1 (dxf_undexqv_sliced is the range of all entries) */
DXF_HIDDEN int    dxf_undexqv_range(dx_ctx *ctx, const dx_undexqv_plan *p, int upper, uint64_t r0, uint64_t r1, slice_fn deliver, void *arg,
                                    size_t cap, int whole_in_);

/* ---- dx_file_check.c ------------------------------------------------------------------------------------------------- */
/* An image of any of the three kinds and the text it decodes to, for who wants the text's slices where they are made (dx_file_verify,
   dx_file_digest, dx_file_census, dx_file_compare): the image's records walked, the header lines the decoder prints, the text's layout. */
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

/* an error leaves what there is to dxf_image_close */
DXF_HIDDEN int  dxf_image_open(dx_ctx *ctx, int kind, int upper, uint32_t width, const uint8_t *img, size_t n, image_text *im);
DXF_HIDDEN void dxf_image_close(image_text *im);
/* records [r0, r1) of a quiva image decoded in one slice, to `fn`: for who holds two images' texts side by side and so states the
   range himself (the 2-bit kinds' reads are compared where they lie: nobody asks for a range of their text, and it is DX_E_ARG) */
DXF_HIDDEN int  dxf_image_range(dx_ctx *ctx, const image_text *im, uint64_t r0, uint64_t r1, int whole_in, slice_fn fn, void *arg);

/* ---- dx_file_u2.c ---------------------------------------------------------------------------------------------------- */
/* where record i's packed read ends in the image */
static inline uint64_t dxf_u2_end(const u2_index *x, uint64_t i) { return x->ioff[i] + (((uint64_t) x->nsym[i] + 3) >> 2); }

/* how much of a 2-bit image of m bytes the device takes at once beside 48 bytes of arrays a record: 0 = all of it (DEXGPU_TEXT_BUDGET counts
   bytes of image here); and a slice of whole records from i0 on: as many as span at most `cap` bytes of image, and one at least */
DXF_HIDDEN size_t   dxf_u2_cap(dx_ctx *ctx, size_t m, uint64_t units);
DXF_HIDDEN uint64_t dxf_u2_slice_end(const u2_index *x, uint64_t i0, size_t cap);

/* a slice of a walked 2-bit image on the device: records [i0, i0 + n), `bytes` of image at d_in, record i0 + k's packed read at
   d_boff[k] of it with d_len[k] symbols; d_extra: `extra` bytes a record of the hook's own, 8-byte aligned, not initialised */
typedef struct { const uint8_t *d_in; uint64_t bytes; const uint64_t *d_boff; const uint32_t *d_len; void *d_extra; uint64_t i0, n; } u2_slice;
typedef int (*u2_slice_fn)(void *arg, const u2_slice *s);
/* the image's packed reads in slices of whole records, at most `cap` bytes of image each (0: in one), each to `fn`; the first answer
   that is not DX_OK ends the loop and is returned.  No records: nothing is allocated and `fn` is not called */
DXF_HIDDEN int dxf_u2_slices(dx_ctx *ctx, const uint8_t *img, const u2_index *x, size_t cap, size_t extra, u2_slice_fn fn, void *arg);

/* ---- dx_file_find.c -------------------------------------------------------------------------------------------------- */
/* The host part of dx_file_find, apart so that it can run without a device (ctx == NULL: no error text is kept).  The patterns as the
   queries of dx_code_find: query k is pattern pat[k] on strand strand[k], the queries in the order (pattern, strand), so that the
   kernel's order (unit, pos, query) is the file's (record, pos, pattern, strand).  eq: the same patterns as the queries of
   dx_code_find_edit, which dxf_find_edit_plan leaves in q's stead. */
typedef struct { dx_query q[64]; uint16_t pat[64]; uint8_t strand[64]; uint32_t nq; dx_equery eq[64]; } find_plan;

DXF_HIDDEN int  dxf_find_plan(dx_ctx *ctx, int kind, const char *const *pattern, uint32_t npat, uint32_t max_mis, int both_strands,
                              find_plan *fp);
/* a slice's hits as dx_code_find listed them -- record: the unit in the slice, query: the query -- become the file's: record + i0, the
   pattern's index, the strand */
DXF_HIDDEN void dxf_find_map(const find_plan *fp, dx_hit *h, uint64_t cnt, uint64_t i0);
/* a letter's code (Number_Read / Number_Arrow, DB.c:393-441), or -1 when it is none of the kind's */
DXF_HIDDEN int  dxf_find_letter(int arrow, int c);
/* what dx_file_find does once its patterns are a plan: the image walked, its slices searched, the report and the lists made.  edit 0:
   the queries are fp->q, searched by dx_code_find; 1: fp->eq, by dx_code_find_edit (dx_file_find_edit.c).  start (edit alone; NULL:
   nothing is launched for it) gets the listed hits' starts, one dx_code_hit_starts a slice behind its listing; rec_len (may be NULL)
   every record's symbols */
DXF_HIDDEN int  dxf_find_run(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, const find_plan *fp, int edit, uint64_t max_hits, dx_find *out,
                             dx_hit **hits, uint32_t **rec_hits, uint32_t **start, uint32_t **rec_len);

/* ---- dx_file_find_edit.c --------------------------------------------------------------------------------------------- */
/* The host part of dx_file_find_edit, apart so that it can run without a device (ctx == NULL: no error text is kept): the patterns as
   the queries of dx_code_find_edit in fp->eq, with pat, strand and nq as dxf_find_plan leaves them (fp->q stays empty). */
DXF_HIDDEN int  dxf_find_edit_plan(dx_ctx *ctx, int kind, const char *const *pattern, uint32_t npat, uint32_t max_err, int both_strands,
                                   find_plan *fp);

/* ---- dx_file_kmers.c ------------------------------------------------------------------------------------------------- */
/* what dx_file_kmers (kmax 14, dx_kmers_fail) and dx_file_kmers_wide (32, dx_kmers_wide_fail) ask of kind, k and canonical: DX_E_ARG in
   `fail`'s words */
DXF_HIDDEN int  dxf_kmers_args(dx_ctx *ctx, int kind, uint32_t k, uint32_t kmax, int canonical, int (*fail)(dx_ctx *, int, const char *));

/* ---- dx_file_compare.c ----------------------------------------------------------------------------------------------- */
/* Two images of one kind, walked and paired by index: the first `both` records of each are compared.  pa / pb (both + 1 each): what the
   slices are measured by -- records [i0, i1) of a side cost p[i1] - p[i0] bytes of text (quiva) or of image (the 2-bit kinds).
   The host part of dx_file_compare, apart so that it can run without a device (ctx == NULL: every walk on the host). */
typedef struct { image_text a, b; uint64_t both, *pa, *pb; } cmp_pair;

DXF_HIDDEN int      dxf_compare_open(dx_ctx *ctx, int kind, const uint8_t *img_a, size_t m_a, const uint8_t *img_b, size_t m_b,
                                     cmp_pair *p, dx_compare *c, int *side);
DXF_HIDDEN uint64_t dxf_compare_slice_end(const cmp_pair *p, uint64_t i0, size_t cap);
DXF_HIDDEN void     dxf_compare_close(cmp_pair *p);

/* ---- dx_select.c ----------------------------------------------------------------------------------------------------- */
/* the span of the input that a unit of a selection can reach, and the unit it belongs to */
typedef struct { uint64_t lo, hi, j; } rspan;

/* What decodes a slice -- units [j0, j0 + m) of the selection.  Their input is at d_in, in_bytes of it: the whole input, or (packed) the
   slice's own spans side by side; unit j0 + k begins at d_start[k] of it, and its text goes to d_out + d_ooff[k].  `pool` lives as long as
   the slice: for the hook's own arrays.  DX_E_FORMAT with *bad = k: unit j0 + k does not end inside the input. */
typedef int (*sel_fn)(void *arg, dpool *pool, const void *d_in, uint64_t in_bytes, const uint64_t *d_start, const uint64_t *d_ooff,
                      uint64_t j0, uint64_t m, int packed, void *d_out, uint64_t *bad);

/* The one loader of a selection: n_ids units of the nbytes at `in`.  Unit j can reach the span un[j] of them, its first byte is at at[j]
   (cut at the input's end or not), and its text goes to res + to[j] (to[n_ids]: the text's end).  The input goes up whole or packed
   (packed_key / whole_key of DEXGPU_TEST decide for a test) -- or is taken where it is: d_have, the whole input on ctx's device
   already --, the text is made in slices of whole units that fit the device (dxf_out_cap), every slice by `fn` and down to its place in
   res.  A unit that `fn` turns down is named as the caller knows it: ids[j] (ids == NULL: j), which starts at start[id] (dx_entry_fail). */
DXF_HIDDEN int dxf_sel_slices(dx_ctx *ctx, const uint8_t *in, size_t nbytes, const void *d_have, const rspan *un, const uint64_t *at,
                              const uint64_t *to, const uint64_t *ids, uint64_t n_ids, const uint64_t *start, const char *packed_key,
                              const char *whole_key, sel_fn fn, void *arg, uint8_t *res);

/* ---- dx_file_subset.c ------------------------------------------------------------------------------------------------ */
/* the selection of dx_file_subset and dx_file_extract: unit j is record ids[j] (ids == NULL: j), all of it or its symbols [beg[j], end[j]) */
typedef struct { const uint64_t *ids; const uint32_t *beg, *end; uint64_t n; } selection;

static inline uint64_t sel_id(const selection *s, uint64_t j)                      { return s->ids ? s->ids[j] : j; }
static inline uint32_t sel_beg(const selection *s, uint64_t j)                     { return s->beg ? s->beg[j] : 0; }
static inline uint32_t sel_end(const selection *s, uint64_t j, const uint32_t *rl) { return s->end ? s->end[j] : rl[sel_id(s, j)]; }

/* what an entry point (`who`) asks of its arguments before it looks at the image: DX_E_DEGENERATE for n_ids == 0 */
DXF_HIDDEN int dxf_sel_args(dx_ctx *ctx, const char *who, const uint8_t *img, const uint64_t *ids, const uint32_t *beg, const uint32_t *end,
                            uint64_t n_ids);
/* ... and of the selection once the image's cnt records and their lengths are known: DX_E_ARG with the unit named (dx_last_error) unless the
   ids are below cnt -- and, `ordered`, do not decrease -- and every interval lies in its record.  n == UINT64_MAX becomes cnt
   (DX_E_DEGENERATE when that is 0) */
DXF_HIDDEN int dxf_sel_check(dx_ctx *ctx, const char *who, selection *s, uint64_t cnt, const uint32_t *rlen, int ordered);

#endif
