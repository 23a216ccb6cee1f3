/*
 * dexgpu.h -- C-ABI of libdexgpu: MI355X (gfx950) kernels for DEXTRACTOR's three codecs.
 *
 * The reference (thegenemyers/DEXTRACTOR) has no plugin/FFI interface; its boundary is the C API
 * of QV.h:48-97 + DB.h:255-267 (per-entry, FILE*-streaming, static state) under six CLI tools.
 * A GPU cannot be fed one entry at a time through FILE*, so this library exposes the SAME
 * operations batch-wise over device-resident buffers.  Each entry point names the reference
 * function(s) it replaces.  Plain pointers and sizes only; no HIP or torch types.
 *
 * Conventions
 *   - `d_` pointers are DEVICE pointers (from dx_malloc, hipMalloc, or a torch tensor's
 *     data_ptr()); everything else is host memory.
 *   - every function returns DX_OK (0) or a negative DX_E_* code; dx_last_error() gives a
 *     message.  Nothing here ever calls exit() (the reference's batch error model, DB.h:45-47,
 *     is reproduced by the CLI front-ends, not the library).
 *   - one dx_ctx per GPU and per host thread; all work of a context is issued on one HIP
 *     stream (dx_set_stream lets a caller supply its own, e.g. torch's current stream).
 *   - multi-byte integers in all produced file images are little-endian, as the reference
 *     writes them on x86-64 hosts (endian key 0x55aa / 0x33cc).
 */
#ifndef DEXGPU_H
#define DEXGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DX_OK              0
#define DX_E_ARG         (-1)   /* bad argument */
#define DX_E_HIP         (-2)   /* HIP runtime error (message has hipGetErrorString) */
#define DX_E_FORMAT      (-3)   /* malformed input image */
#define DX_E_DEGENERATE  (-4)   /* a stream that needs a scheme has an empty histogram (reference: UB, QV.c:201) */
#define DX_E_UNSUPPORTED (-5)   /* a final code longer than 16 bits (the reference's own decoder cannot read it) */
#define DX_E_NOMEM       (-6)
#define DX_E_MISMATCH    (-7)   /* device-side consistency check failed (e.g. symbol count != expected) */
#define DX_E_SPACE       (-8)   /* output buffer too small */
#define DX_E_IO          (-9)   /* a caller's sink refused data (dx_d2h_stream); a file could not be read (dx_h2d_fd) */
#define DX_E_AGAIN       (-10)  /* not this way: an entry point that takes a file descriptor wants the image in memory after all
                                   (a small or malformed file, one that does not fit the device): call its in-memory twin */

typedef struct dx_ctx dx_ctx;

/* ------------------------------------------------------------------------------------------
 *  context, memory, profiling
 * ------------------------------------------------------------------------------------------ */
int         dx_device_count(void);
int         dx_open(int device, dx_ctx **ctx);
void        dx_close(dx_ctx *ctx);
const char *dx_last_error(const dx_ctx *ctx);      /* ctx may be NULL: last error of dx_open */
int         dx_set_stream(dx_ctx *ctx, void *hip_stream);   /* issue on this hipStream_t; NULL = the default (null) stream,
                                                               e.g. torch's current stream when it is the default one */
int         dx_reset_stream(dx_ctx *ctx);                   /* back to the context's own non-blocking stream */
int         dx_sync(dx_ctx *ctx);

int dx_malloc(dx_ctx *ctx, size_t bytes, void **d_ptr);
int dx_free  (dx_ctx *ctx, void *d_ptr);
int dx_h2d   (dx_ctx *ctx, void *d_dst, const void *src, size_t bytes);   /* synchronous */
int dx_d2h   (dx_ctx *ctx, void *dst, const void *d_src, size_t bytes);   /* synchronous */
/* bytes [foff, foff + bytes) of the file behind fd to device memory, read (pread) by several threads straight into pinned buffers
 * that leave as they fill: no mapping of the file in the caller's address space (a large dx_h2d from memory goes through the same
 * threads).  DX_E_IO: the file could not be read.                                                                       */
int dx_h2d_fd(dx_ctx *ctx, void *d_dst, int fd, uint64_t foff, size_t bytes);
/* Device memory to a consumer on the host, in order, in chunks (32 MiB) through two pinned staging buffers the
 * context owns: sink(user, data, len, at) is called on a helper thread for the bytes [at, at + len) while the
 * next chunk is in flight; it may modify data[0 .. len) and returns 0, or nonzero to stop (DX_E_IO comes back).
 * For outputs headed to a file: a pwrite per chunk costs no page fault in the caller's address space, where
 * dx_d2h into fresh memory pays one per 4 KiB (0.25 s per GiB, single-threaded).                             */
typedef int (*dx_sink_fn)(void *user, uint8_t *data, size_t len, size_t at);
int dx_d2h_stream(dx_ctx *ctx, const void *d_src, size_t bytes, dx_sink_fn sink, void *user);
/* A sink that is positional -- it takes chunk [at, at + len) whatever came before, from whichever thread (a pwrite per chunk) --
 * may be fed by several threads: from 128 MiB on dx_d2h_stream (and every file driver that delivers through a sink) then keeps up
 * to eight 16 MiB copies in flight and calls the sink from `threads` helper threads, chunks in any order (one thread writing into
 * a file's pages is slower than the link brings them).  Default 1: in order, one thread.  Returns the value in force before.     */
int dx_set_sink_threads(dx_ctx *ctx, int threads);
int dx_memset(dx_ctx *ctx, void *d_dst, int value, size_t bytes);

/* Per-kernel device time, measured with HIP events on the context's stream around every launch
 * while profiling is enabled.  Kernel ids: */
enum { DX_K_PACK2_ENC = 0, DX_K_PACK2_DEC, DX_K_QV_PRESCAN, DX_K_QV_HIST, DX_K_QV_SIZES, DX_K_SCAN,
       DX_K_QV_ENCODE, DX_K_QV_DECODE, DX_K_SYNTH, DX_K_INDEX, DX_K_QV_COMPACT,
       DX_K_QV_ENCODE_TEXT,                       /* the encoder that reads the text (two-pass path; entries without usable tokens) */
       DX_K_QV_DEC_SUB, DX_K_QV_DEC_RUNS, DX_K_QV_DEC_PLAIN, DX_K_QV_DEC_TAGS,   /* DX_K_QV_DECODE: the generic lane-per-line decoder */
       DX_K_QV_WALK,                              /* the record walk of a bare stream (dx_qv_walk_device) */
       DX_K_COUNT };
int         dx_profile(dx_ctx *ctx, int enable);                  /* enabling resets the counters */
int         dx_profile_get(dx_ctx *ctx, int kernel, double *ms_total, uint64_t *launches);  /* syncs */
const char *dx_kernel_name(int kernel);

/* ------------------------------------------------------------------------------------------
 *  2-bit packers: dexta/undexta, dexar/undexar
 * ------------------------------------------------------------------------------------------ */
enum { DX_ALPHA_BASES = 0,    /* Number_Read  DB.c:393: c/C->1 g/G->2 t/T->3, everything else 0   */
       DX_ALPHA_ARROW = 1,    /* Number_Arrow DB.c:418: '1'->0 '2'->1 '3','G'->2, everything else 3 */
       DX_ALPHA_NUMBERS = 2 };/* already numbers 0..3 (what Compress_Read DB.c:319 takes): the low two bits */
enum { DX_LETTERS_LOWER = 0,  /* Lower_Read  DB.c:367 acgt */
       DX_LETTERS_UPPER = 1,  /* Upper_Read  DB.c:375 ACGT */
       DX_LETTERS_ARROW = 2,  /* Letter_Arrow DB.c:383 1234 */
       DX_LETTERS_NUMBERS = 3 };/* the numbers 0..3 themselves (what Uncompress_Read DB.c:342 leaves) */

/* Replaces, for n reads at once: the line-gathering loop dexta.c:161-183 (newlines are skipped on
 * the device), Number_Read/Number_Arrow (DB.c:393-441), Compress_Read (DB.c:319-338) and the
 * record writes dexta.c:187-204 / dexar.c:193-210.
 *   read i's sequence text = d_text[d_off[i] .. d_off[i]+d_tlen[i]) : any number of lines, '\n'
 *   bytes are dropped, all other bytes are symbols; it must hold exactly d_nsym[i] symbols.
 *   Output record i is written at d_out + d_out_off[i]: first the framing bytes
 *   d_hdr[d_hdr_off[i] .. d_hdr_off[i+1]) (may be NULL: no framing), then (nsym+3)>>2 packed
 *   bytes, first symbol in the top two bits, missing symbols 0.
 * Returns DX_E_MISMATCH if some read's symbol count differs from d_nsym[i].                     */
int dx_pack2_encode(dx_ctx *ctx, int alphabet,
                    const uint8_t *d_text, const uint64_t *d_off, const uint32_t *d_tlen,
                    const uint32_t *d_nsym, uint64_t n,
                    const uint8_t *d_hdr, const uint64_t *d_hdr_off,
                    uint8_t *d_out, const uint64_t *d_out_off);

/* Replaces Uncompress_Read (DB.c:342-363) + Lower_Read/Upper_Read/Letter_Arrow (DB.c:367-389)
 * + the line wrapping of undexta.c:263-270 / undexar.c:221-228.
 *   read i's packed bytes start at d_in + d_in_off[i]; its text (d_nsym[i] letters, a '\n'
 *   after every `width` letters and after the last partial line; nothing for an empty read) is
 *   written at d_out + d_out_off[i].  width >= 1.                                               */
int dx_pack2_decode(dx_ctx *ctx, int letters,
                    const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_nsym, uint64_t n,
                    uint32_t width, uint8_t *d_out, const uint64_t *d_out_off);

/* Host helpers for the record framing of all three formats (dexta.c:187-198, dexar.c:159-163 +
 * 193-204, dexqv.c:128-139): well-delta chain, int32 beg, end, then int32 qv (kind 0) or four
 * uint16 cnr (kind 1, values already converted with dx_snr_to_cnr).  `field[i]` points at the
 * 4 int32 {well,beg,end,qv} (kind 0) or {well,beg,end,-} followed in `cnr` by 4 uint16 (kind 1).
 * blob must hold dx_frame_bound(...) bytes; off gets n+1 entries.  *lwell carries the previous
 * well across calls (starts at 0, dexta.c:137).                                                 */
size_t   dx_frame_bound(const int32_t *hdr4, uint64_t n, int32_t lwell, int kind);
int      dx_frame_headers(const int32_t *hdr4, const uint16_t *cnr4, uint64_t n, int kind,
                          int32_t *lwell, uint8_t *blob, uint64_t *off);
uint16_t dx_snr_to_cnr(float snr);                 /* dexar.c:159-163 */

/* ------------------------------------------------------------------------------------------
 *  text front end (host): index a file image so the kernels can read it in place
 * ------------------------------------------------------------------------------------------ */
/* why an image was rejected (*errcode), with the 1-based line number in *errline */
enum { DX_IDX_NO_NEWLINE = 1,   /* last line does not end with a newline   (QV.c:779) */
       DX_IDX_NO_HEADER  = 2,   /* header line missing                     (QV.c:954, dexta.c:113) */
       DX_IDX_BAD_HEADER = 3,   /* header line incorrectly formatted       (QV.c:958-968, dexta.c:146-155) */
       DX_IDX_INCOMPLETE = 4,   /* incomplete last entry of .quiva file    (QV.c:789) */
       DX_IDX_RAGGED     = 5,   /* lines for an entry are not the same length (QV.c:793) */
       DX_IDX_TOO_LONG   = 6,   /* fasta/arrow line longer than 99998 chars (dexta.c:165-172) */
       DX_IDX_EMPTY      = 7 }; /* empty input (the reference reads an uninitialised buffer, dexta.c:108) */

/* .quiva: replaces the Read_Lines loops and header validation of QVcoding_Scan (QV.c:751-798,
 * 948-978).  Fills (up to cap entries of) off[i] = offset of entry i's first data line, len[i] =
 * symbols per line, hdr4[4i..] = well, beg, end, qv; *count = entries found (call with cap 0 to
 * count); *prefix_len = bytes of the first header before its first '/' after position 0.      */
int dx_index_quiva(const uint8_t *text, size_t n, uint64_t cap,
                   uint64_t *off, uint32_t *len, int32_t *hdr4,
                   uint64_t *count, size_t *prefix_len, uint64_t *errline, int *errcode);

/* .fasta (arrow = 0) / .arrow (arrow = 1): replaces dexta.c:104-183 / dexar.c:103-188.  off[i] =
 * offset of read i's first sequence line, tlen[i] = its text bytes up to the next header or the
 * end (newlines included), nsym[i] = symbols (tlen - lines), hdr4 = well, beg, end, qv (qv = 0
 * when "RQ=" is missing), cnr4 (arrow) = the four SN values converted by dx_snr_to_cnr.        */
int dx_index_seq(int arrow, const uint8_t *text, size_t n, uint64_t cap,
                 uint64_t *off, uint32_t *tlen, uint32_t *nsym, int32_t *hdr4, uint16_t *cnr4,
                 uint64_t *count, size_t *prefix_len, uint64_t *errline, int *errcode);

/* GPU text front end for a .quiva image already in device memory: newline scan, structure checks
 * and entry index on the device; only the header lines come back to the host, where sscanf parses
 * them as QV.c:964 does.  Same results as dx_index_quiva.  *d_off / *d_len are device arrays
 * (release with dx_free), *hdr4 a host array (free()).  On DX_E_FORMAT *errline / *errcode name an
 * offending line, found in three steps.  (1) The text's last byte is looked at first and on its own: a
 * header or a first data line without its newline is DX_IDX_NO_NEWLINE at the last line, whatever stands
 * in front of it; where that is the text's one defect, line and code are dx_index_quiva's.  (2) Then the
 * kernels check every entry for no '@', an empty header, no '/', ragged and missing data lines: of these
 * the lowest line is named, in whichever workgroup it lies, with dx_index_quiva's line and code where
 * the text has no defect of another step.  (3) The header fields are parsed only once (2) has passed: a
 * header whose fields do not parse, standing in front of a defect of (1) or (2), is refused too, but at
 * the later line.  (The sentence "the lowest offending line number wins" at the top of
 * csrc/dx_index.hip is to be read with these limits: it holds within step (2).)  Callers that need the
 * reference's exact first message re-run dx_index_quiva on the host copy (the error path is not
 * performance relevant).  d_text needs no alignment.                                              */
int dx_index_quiva_device(dx_ctx *ctx, const uint8_t *d_text, uint64_t nbytes,
                          uint64_t **d_off, uint32_t **d_len, uint64_t *count,
                          int32_t **hdr4, size_t *prefix_len, uint64_t *errline, int *errcode);
int dx_parse_quiva_headers(const uint8_t *blob, const uint64_t *pos, uint64_t n, int32_t *hdr4,
                           size_t *prefix_len, uint64_t *bad_entry);

/* The same for a .fasta (arrow = 0) / .arrow (arrow = 1) image: records are delimited on the device by
 * their header lines ('>' first); results as dx_index_seq.  On DX_E_FORMAT a text whose one defect is a line that
 * is too long, a first line that is no header or a missing final newline is refused with dx_index_seq's line
 * and code.  With several defects the order is the device's: the last byte is looked at first (a missing final
 * newline is named whatever stands in front of it), then the lines, then the headers' fields; a header that
 * does not parse is DX_IDX_BAD_HEADER at *errline = 0.  Re-run dx_index_seq on the host copy for the
 * reference's exact first message.  d_text needs no alignment.                                   */
int dx_index_seq_device(dx_ctx *ctx, int arrow, const uint8_t *d_text, uint64_t nbytes,
                        uint64_t **d_off, uint32_t **d_tlen, uint32_t **d_nsym, uint64_t *count,
                        int32_t **hdr4, uint16_t **cnr4, size_t *prefix_len,
                        uint64_t *errline, int *errcode);
int dx_parse_seq_headers(int arrow, const uint8_t *blob, const uint64_t *pos, uint64_t n,
                         int32_t *hdr4, uint16_t *cnr4, size_t *prefix_len, uint64_t *bad_entry);

/* ------------------------------------------------------------------------------------------
 *  5-stream QV coder: dexqv/undexqv (QV.c)
 * ------------------------------------------------------------------------------------------ */
enum { DX_DEL = 0, DX_INS = 1, DX_MRG = 2, DX_SUB = 3, DX_DRUN = 4, DX_SRUN = 5 };

/* A batch of .quiva entries resident on the device.  Entry i's five streams (deletion QV,
 * deletion tag, insertion QV, merge QV, substitution QV -- the line order of QV.c:973-991) are
 * d_len[i] bytes each; stream k starts at d_text + d_off[i] + k*(d_len[i] + line_pad).  For a
 * .quiva file image line_pad = 1 (the '\n').                                                    */
typedef struct
  { const uint8_t  *d_text;
    const uint64_t *d_off;
    const uint32_t *d_len;
    uint64_t        n;
    uint64_t        text_bytes;   /* readable bytes at d_text (the whole image).  With it the kernels
                                     may load a line's last, partial 16-byte chunk in one piece;
                                     0 = unknown: nothing beyond a line's end is ever read        */
    uint32_t        line_pad;
  } dx_qv_batch;

/* The order-dependent scan state of QVcoding_Scan (QV.c:993-1017): run characters (-1 none) and
 * the GLOBAL entry index from which each run-length histogram starts counting.                  */
typedef struct
  { int32_t delChar, subChar;
    int64_t del_first, sub_first;
  } dx_qv_params;

/* The lossy rounding of Compress_Next_QVentry (QV.c:1355-1372: insertion QVs >> 1 << 1, merge QVs >> 2 << 2) applied IN PLACE
 * to the batch's text on the device: the text a lossy .dexqv decodes back to (what a lossy round trip is compared with). */
int dx_qv_lossy_text(dx_ctx *ctx, const dx_qv_batch *b);

/* Finds delChar (deletion QV under the first 'n'/'N' tag, QV.c:993-1002) and the provisional
 * subChar (argmax of the substitution histogram of the entries up to the one where the running
 * symbol count first reaches 100000, ties to the smallest value, QV.c:1006-1015), on the device.
 * entry0 = global index of the batch's first entry.  Fields of *p that are already set (>= 0)
 * are kept; initialise *p to {-1,-1,-1,-1}.  The subChar search needs the file's first entries,
 * so it only runs for the batch with entry0 == 0 (a shard holding the first 100000 symbols).   */
int dx_qv_prescan(dx_ctx *ctx, const dx_qv_batch *b, uint64_t entry0, dx_qv_params *p);

/* Histogram_Seqs x4 + Histogram_Runs x2 (QV.c:702-724, 988-1017) over the batch: ADDS the
 * batch's counts into hist (host, 6x256, order DX_DEL..DX_SRUN) and its symbol count into
 * *totChar.  Run histograms are raw counts: the reference's start value of 1 per bin
 * (QV.c:934-935) is added once by dx_qv_build.  Shards of one file: call per shard (any GPU),
 * add the arrays on the host.                                                                   */
int dx_qv_hist(dx_ctx *ctx, const dx_qv_batch *b, uint64_t entry0, const dx_qv_params *p,
               uint64_t hist[6][256], uint64_t *totChar);

/* QVcoding_Scan (QV.c:922-1023) over one batch in one call: dx_qv_prescan followed by dx_qv_hist -- the same *p, hist and
 * *totChar as the two calls leave -- with ONE wait on the device instead of three.  The scan state stays on the device
 * between the kernels; the two things the host has to decide before it knows that state (which of its histogram kernels
 * fits the batch's run density, whether the token buffers it holds are large enough) it takes from the context's last
 * scan, and the device checks them: a context's first batch, or a batch unlike the last one, simply goes through the
 * two calls.  Nothing of one batch's RESULTS is carried to the next.  DEXGPU_TEST=no_scan_guess: always the two calls.   */
int dx_qv_scan(dx_ctx *ctx, const dx_qv_batch *b, uint64_t entry0, dx_qv_params *p,
               uint64_t hist[6][256], uint64_t *totChar);

typedef struct
  { int32_t  type;              /* 0 normal, 2 truncated with escape code (QV.c:76-81) */
    uint32_t bits[256];
    int32_t  lens[256];
  } dx_scheme;

typedef struct
  { dx_scheme s[6];             /* DX_DEL..DX_SRUN; run schemes valid iff the run char is >= 0 */
    int32_t   delChar, subChar; /* final values (subChar may have been dropped, QV.c:1044-1045) */
  } dx_qv_coding;

/* Create_QVcoding (QV.c:1029-1169) incl. Huffman/Reheap/Build_Table (QV.c:91-220): host only. */
int dx_qv_build(const uint64_t hist[6][256], uint64_t totChar, const dx_qv_params *p, int lossy,
                dx_qv_coding *out);

/* Write_QVcoding (QV.c:1173-1210) / Read_QVcoding (QV.c:1214-1320) on memory images.  The
 * image starts at the 0x33cc key (dexqv's own 0x55aa key, dexqv.c:105, is not included).       */
int dx_qv_write_coding(const dx_qv_coding *c, const char *prefix, size_t plen,
                       uint8_t *buf, size_t cap, size_t *written);
int dx_qv_read_coding(const uint8_t *buf, size_t n, dx_qv_coding *c, int *flip,
                      char *prefix, size_t pcap, size_t *consumed);

/* Uploads the code tables for the kernels below (and remembers `lossy`, QV.c:1406-1415). */
int dx_qv_set_coding(dx_ctx *ctx, const dx_qv_coding *c, int lossy);

/* Record sizes: for each entry the bytes Compress_Next_QVentry (QV.c:1381-1426) would write
 * (bit totals, pad rule QV.c:436-442 / 499-505, Pack_Tag length): d_seg[5*i+k] = bytes of entry
 * i's del / tag / ins / mrg / sub segment -- the index the format itself does not store and a
 * parallel decoder needs.  Adding the framing bytes d_hdr_off[i+1]-d_hdr_off[i] (NULL: none) and
 * an exclusive scan in file order gives d_rec_off[0..n] (device, n+1 entries); *total =
 * d_rec_off[n].                                                                                */
int dx_qv_sizes(dx_ctx *ctx, const dx_qv_batch *b, const uint64_t *d_hdr_off,
                uint32_t *d_seg, uint64_t *d_rec_off, uint64_t *total);

/* Compress_Next_QVentry for the whole batch: record i = framing bytes, then the del words, tag
 * bytes, ins words, mrg words, sub words (Encode / Encode_Run / Pack_Tag+Number_Read+
 * Compress_Read, QV.c:386-506, 810-819, 1393-1423) at d_out + d_rec_off[i].  d_seg and
 * d_rec_off are the outputs of dx_qv_sizes for the same batch and coding (the deletion QVs and
 * their tags are written in one sweep, which needs the deletion segment's size up front); the
 * kernel re-derives every segment size and returns DX_E_MISMATCH if one disagrees.              */
int dx_qv_encode(dx_ctx *ctx, const dx_qv_batch *b, const uint8_t *d_hdr, const uint64_t *d_hdr_off,
                 const uint64_t *d_rec_off, const uint32_t *d_seg, uint8_t *d_out);

/* Compress_Next_QVentry x n (QV.c:1381-1426) in one call: the five segment sizes of every entry (d_seg, n x 5: the same index
 * dx_qv_sizes produces), a scan that turns them into d_rec_off (n + 1), and every record -- framing bytes and segments -- written
 * where it belongs in d_out.  *total receives the stream's size; DX_E_SPACE if it exceeds out_cap (nothing useful is in d_out
 * then).  The bytes are those of dx_qv_sizes + dx_qv_encode.  Which kernels run depends on what this context's dx_qv_hist (or
 * dx_qv_scan) of the same batch has left: tokens and every entry's own histograms (the usual case: sizes by a dot product,
 * k_qv_encode_fast), tokens alone (sizes from tokens and plain lines), nothing (sizes and records from the text); a batch of
 * short entries goes a lane an entry, one with long entries among the short ones is dealt between the two kinds of kernel
 * (dx_qv_onepass_info tells).  No scratch beyond O(n) bookkeeping: rounds 2-3's slots and their compaction are gone (round 6). */
int dx_qv_encode_onepass(dx_ctx *ctx, const dx_qv_batch *b, const uint8_t *d_hdr, const uint64_t *d_hdr_off,
                         uint32_t *d_seg, uint64_t *d_rec_off, uint8_t *d_out, uint64_t out_cap, uint64_t *total);
/* The same in two halves (kept from the rounds in which a compaction ran behind the encoder: a caller written for them works
 * unchanged): _begin does the encode and keeps the answer, _end hands back the stream's size and the verdict (DX_E_SPACE, ...).
 * Between the two, the NEXT batch's dx_qv_prescan, dx_qv_hist, dx_qv_build and dx_qv_set_coding may run; dx_qv_sizes,
 * dx_qv_encode, dx_qv_decode and a second dx_qv_encode_onepass[_begin] are refused (DX_E_ARG) until _end has been called.  A
 * dx_qv_set_coding in between leaves the group index (dx_qv_subindex) of the ended encode unarmed.  One encode at a time per
 * context.                                                                                                              */
int dx_qv_encode_onepass_begin(dx_ctx *ctx, const dx_qv_batch *b, const uint8_t *d_hdr, const uint64_t *d_hdr_off,
                               uint32_t *d_seg, uint64_t *d_rec_off, uint8_t *d_out, uint64_t out_cap);
int dx_qv_encode_onepass_end(dx_ctx *ctx, uint64_t *total);

/* Which way the last dx_qv_encode_onepass / _begin of this context took, for logs and benchmarks: direct (below), tokens = 1 when
 * the histogram pass's tokens fed the encoder, scratch_bytes = the context's scratch allocation after the call, token_bytes =
 * the token slots, text_entries = entries the text-reading kernels took (no tokens, or tokens that could not be used: a byte
 * >= 128 in a run-coded line, more tokens than the slot or the list holds; the short entries of routes 3 and 5).  groups,
 * region_bytes and avail_bytes are of the scratch-slot route, which is gone: always 0 (kept for the layout).            */
typedef struct
  { int32_t  groups, direct, tokens, reserved;        /* direct: 1 sizes by k_qv_sizes_fast (tokens and plain lines read again), 2 sizes from the
                                                         entries' own histograms (k_qv_sizes_hist): the product route, 3 a batch of short entries: a
                                                         lane per entry (k_qs_entries: sizes, then records), 4 no tokens of this batch: sizes and records
                                                         from the text, 5 short entries by the lanes and the long ones among them as a batch of their
                                                         own through the wave-per-entry kernels */
    uint64_t region_bytes, scratch_bytes, avail_bytes, token_bytes, text_entries;
    uint64_t chain_waits[3];                          /* always 0 (the routes that reported here are gone; kept for the layout) */
  } dx_onepass_info;
int dx_qv_onepass_info(const dx_ctx *ctx, dx_onepass_info *out);

/* An upper bound on one scratch request of the context (0, the default: none; requests of up to 64 MB always pass).  Rounds
 * 2-3's encoder sized its scratch regions by it; since round 6 no route needs scratch beyond O(n) bookkeeping, and the call
 * only bounds that.  The environment variable DEXGPU_SCRATCH_BUDGET (bytes) overrides it.                              */
int dx_set_scratch_budget(dx_ctx *ctx, uint64_t bytes);

/* Device memory free / in all on the context's GPU right now (hipMemGetInfo). */
int dx_mem_info(dx_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes);

/* Gives device memory the context keeps between calls back to the device (it is allocated again when next needed):
 * DX_TRIM_SCRATCH the scratch regions of dx_qv_encode_onepass and dx_qv_hist, DX_TRIM_TOKENS the token slots the
 * histogram pass leaves for the encoder (the next encode without a fresh dx_qv_hist then reads the text),
 * DX_TRIM_INDEX the group index of dx_qv_subindex (the next decode then takes the lane-per-line kernels).       */
#define DX_TRIM_SCRATCH 1
#define DX_TRIM_TOKENS  2
#define DX_TRIM_INDEX   4
#define DX_TRIM_ALL     7
int dx_trim(dx_ctx *ctx, int what);

/* Host helper sizing d_out for dx_qv_encode_onepass: an upper bound of the bytes the batch's n entries
 * encode to (framing bytes not included), from the batch's own raw histograms (what dx_qv_hist added
 * for it) and the coding in force -- every symbol priced at its code (QV.c:427-434), run tokens at
 * theirs (QV.c:475-497), partial / pad words (QV.c:436-442) and tag bytes (QV.c:810-819) per entry.
 * Within a few percent of the real size once the file is much longer than the 100000 symbols after which
 * the run histograms start (the runs before are priced at the dearest run token).                    */
uint64_t dx_qv_out_bound(const uint64_t hist[6][256], uint64_t n, const dx_qv_coding *c, int lossy);

/* Uncompress_Next_QVentry (QV.c:1428-1481: Decode, Decode_Run, Unpack_Tag) for n records whose
 * segment starts are known: record i starts at d_in + d_rec_off[i] with d_hdr_off[i+1] -
 * d_hdr_off[i] framing bytes (NULL: none) followed by segments of d_seg[5*i+k] bytes -- exactly
 * the arrays dx_qv_sizes produces, or dx_qv_walk for a bare file.  The five decoded lines
 * (d_len[i] symbols each, every line followed by '\n') are written at d_out + d_out_off[i].
 * flags: DX_DECODE_UPPER applies undexqv's -U (undexqv.c:198-204); DX_DECODE_FLIP reads the code
 * words byte-swapped (a file written on a host of the other endianness: GETFLIP, QV.c:553-568).
 * Uses the tables of dx_qv_set_coding.                                                          */
#define DX_DECODE_UPPER 1
#define DX_DECODE_FLIP  2
int dx_qv_decode(dx_ctx *ctx, const uint8_t *d_in, const uint64_t *d_rec_off, const uint64_t *d_hdr_off,
                 const uint32_t *d_seg, const uint32_t *d_len, uint64_t n, int flags,
                 uint8_t *d_out, const uint64_t *d_out_off);

/* Host walk of a bare .dexqv image (undexqv.c:101-208 and the bit-level structure of QV.c:510-691):
 * the format stores no lengths, so the start of every segment is only known after walking the one
 * before it, code by code.  Fills the index dx_qv_decode needs (arrays are malloc'd; release with
 * dx_qv_index_free).  Sequential by nature of the format.                                        */
typedef struct
  { uint64_t      n;            /* records */
    uint64_t     *rec_off;      /* n+1: offset of each record in the image */
    uint64_t     *hdr_off;      /* n+1: running sum of the records' framing bytes */
    uint32_t     *seg;          /* n x 5 segment byte sizes */
    uint32_t     *len;          /* n: symbols per entry (end - beg, undexqv.c:186) */
    int32_t      *hdr4;         /* n x 4: well, beg, end, qv */
    dx_qv_coding  coding;
    char         *prefix;       /* header prefix (QV.c:1256-1265) */
    int           newv, flip;   /* 0x55aa-keyed file (int32 fields) / byte-swapped writer */
    /* dx_qv_walk_indexed(want_index != 0): the group index of dx_qv_subindex, made by the walk (it passes every code anyway) */
    uint32_t     *gidx;         /* gidx_words words: per entry the plain lines' group bytes, three header words, the run lines' group words */
    uint64_t     *gidx_off;     /* n+1: where each entry's words start */
    uint64_t      gidx_words;
    uint64_t      gidx_none;    /* run-coded lines left without an index (a group that does not fit its word) */
  } dx_qv_index;
int  dx_qv_walk(const uint8_t *img, size_t n, dx_qv_index *idx);
/* The same, and with want_index != 0 also the group index (layout: csrc/dx_layout.h) that lets dx_qv_decode take a
 * wavefront per line instead of a lane: hand it over with dx_qv_use_index.  The walk then takes one table look-up per
 * symbol instead of one per several.                                                                         */
int  dx_qv_walk_indexed(const uint8_t *img, size_t n, dx_qv_index *idx, int want_index);
/* A group index for the stream at d_in with the segment index d_seg (n entries), uploaded by the caller (d_gidx: the
 * words, d_gidx_off: n + 1 offsets; none: dx_qv_index.gidx_none).  dx_qv_decode of that stream -- all of it or a
 * contiguous part, same d_in and d_seg -- then decodes with it.  The memory stays the caller's and must outlive the
 * decodes; d_gidx == NULL takes the index back.  An index the context made itself (dx_qv_subindex) is dropped.   */
int  dx_qv_use_index(dx_ctx *ctx, const uint8_t *d_in, const uint32_t *d_seg, uint64_t n,
                     const uint32_t *d_gidx, const uint64_t *d_gidx_off, uint64_t none);
void dx_qv_index_free(dx_qv_index *idx);

/* The same walk on the device, for a record stream already there (undexqv.c:119-208, QV.c:1428-1481): d_img[0, n) is the
 * file image, `first` the offset of its first record (behind the 0x55aa key and the coding, which the caller has read on
 * the host: dx_qv_read_coding), cd that coding, newv / flip as dx_qv_index has them.  The stream is cut into pieces of
 * 32 KiB (more of a stream beyond 16 GB); a lane per piece finds a record start in its piece, checks it by walking, and walks on to the next piece's
 * start; only offsets on an unbroken chain of such walks from the first record are kept, so the index is the host
 * walk's (csrc/dx_qv_walk.hip).  The arrays are device memory of the library's (dx_qv_dindex_free): what dx_qv_decode
 * takes, and d_hdr4 (n x 4: well, beg, end, qv) for the header lines.  DX_E_MISMATCH: the walks did not chain up, a record
 * did not walk, 16-bit framing fields -- the caller then walks on the host (dx_qv_walk), which also names what is wrong
 * with a damaged file.  The run-coded lines' groups of the group index are noted on the way (dx_qv_use_dindex).               */
typedef struct
  { uint64_t  n;                /* records */
    uint64_t *d_rec_off;        /* n + 1 */
    uint64_t *d_hdr_off;        /* n + 1 */
    uint32_t *d_seg;            /* n x 5 */
    uint32_t *d_len;            /* n */
    int32_t  *d_hdr4;           /* n x 4 */
    uint64_t  pieces, piece_bytes;      /* how the stream was cut (for logs) */
    /* the run-coded lines' share of the group index (NULL: none made -- neither line run-coded, a byte-swapped stream):
       gidx_words words, gidx_off[n + 1] where each entry's begin, gidx_none run-coded lines without (dx_qv_use_dindex) */
    uint32_t *d_gidx;
    uint64_t *d_gidx_off;
    uint64_t  gidx_words, gidx_none;
    uint64_t  gidx_nosync;      /* plain lines without their words (where every 64th symbol is) */
    uint32_t  sync_kinds;       /* bit q: the plain lines of kind q (0 del, 1 ins, 2 mrg, 3 sub) have such words */
  } dx_qv_dindex;
int  dx_qv_walk_device(dx_ctx *ctx, const uint8_t *d_img, uint64_t n, uint64_t first, const dx_qv_coding *cd, int newv, int flip,
                       dx_qv_dindex *out);
void dx_qv_dindex_free(dx_ctx *ctx, dx_qv_dindex *x);
/* Hands the index a device walk has left to the decoder: a dx_qv_decode of the stream at d_in with x's arrays (the whole of
 * it or a contiguous part) then decodes every run-coded line -- and the tag line with the deletion line -- a wavefront at a
 * time (k_qv_decode_runs; QV.c:604-691, 823-847) instead of a lane; the plain lines have no groups in this index and stay with
 * the lane-per-line kernel.  x == NULL or x->d_gidx == NULL: takes it back.  x must outlive the decodes.                  */
int  dx_qv_use_dindex(dx_ctx *ctx, const uint8_t *d_in, const dx_qv_dindex *x);

/* Group index (on = 1): dx_qv_encode_onepass also leaves, in the context, where the codes are: one byte per group of
 * 16 symbols of each plain line (the group's code bits), one word per group of <= 8 (run, symbol) tokens of each
 * run-coded line (bits and positions covered) -- about 4.5 KB per 10 kb entry.  A dx_qv_decode of that record stream
 * (same d_in / d_seg, the whole batch or a contiguous part of it) in the same context then decodes each line with a
 * whole wavefront, 64 consecutive groups at a time, instead of a lane (k_qv_decode_sub, k_qv_decode_runs).  The .dexqv
 * bytes do not change; a stream decoded without the index (a bare file, another context) takes the lane-per-line
 * kernels, as do the lines of entries the fast encoder does not handle (runs of 127 and more, bytes >= 128).  Off by
 * default.                                                                                                       */
int  dx_qv_subindex(dx_ctx *ctx, int on);

/* ------------------------------------------------------------------------------------------
 *  whole-file drivers (host images in, host images out): what the six CLI tools call
 * ------------------------------------------------------------------------------------------ */
/* Each takes a complete input file image and returns the complete output image (malloc'd, free
 * with dx_file_free), byte-identical to the file the reference tool writes.  On DX_E_FORMAT from
 * the text front end, *errline / *errcode say where and why (DX_IDX_*).
 *   dx_file_pack2    dexta.c:104-205 (arrow = 0) / dexar.c:103-211 (arrow = 1)
 *   dx_file_unpack2  undexta.c:131-271 (mode DX_LETTERS_LOWER / _UPPER) / undexar.c:129-229 (_ARROW)
 *   dx_file_dexqv    dexqv.c:79-143                                                             */
int  dx_file_pack2  (dx_ctx *ctx, int arrow, const uint8_t *text, size_t n,
                     uint8_t **out, size_t *out_len, uint64_t *errline, int *errcode);
/* The same for a text that arrives in pieces (a pipe: dexta -i, dexta.c:55-58; a file too large to hold): rd(user, buf, want)
 * returns the bytes it put into buf (fewer than want only at the end, 0 at the end, < 0: an error); `chunk` bytes are read at a time
 * (0: 256 MiB), whole records of them packed, the image's bytes handed to the sink in file order (at = their place in the
 * image).  The same bytes as dx_file_pack2 of the whole text; memory: about 1.3 x chunk whatever the text's size.           */
typedef long (*dx_read_fn)(void *user, void *buf, size_t want);
int  dx_file_pack2_stream(dx_ctx *ctx, int arrow, dx_read_fn rd, void *ruser, size_t chunk,
                          dx_sink_fn sink, void *suser, size_t *out_len, uint64_t *errline, int *errcode);
/* ... and the other way (undexta -i / undexar -i, undexta.c:175-271): the image in pieces of `chunk` bytes (0: 128 MiB), the text of
 * the whole records among them to the sink in file order; mode and width as for dx_file_unpack2.                              */
int  dx_file_unpack2_stream(dx_ctx *ctx, int mode, dx_read_fn rd, void *ruser, size_t chunk, uint32_t width,
                            dx_sink_fn sink, void *suser, size_t *out_len);
int  dx_file_unpack2(dx_ctx *ctx, int mode, const uint8_t *img, size_t n, uint32_t width,
                     uint8_t **out, size_t *out_len);
int  dx_file_dexqv  (dx_ctx *ctx, const uint8_t *text, size_t n, int lossy,
                     uint8_t **out, size_t *out_len, uint64_t *errline, int *errcode);
/* dx_file_unpack2 with the text delivered through a sink, in order (dx_d2h_stream), header lines in place */
int  dx_file_unpack2_to(dx_ctx *ctx, int mode, const uint8_t *img, size_t n, uint32_t width,
                        dx_sink_fn sink, void *user, size_t *out_len);
/* dx_file_dexqv with the .dexqv image delivered through a sink instead (the file's head, then the record stream
 * in chunks: dx_d2h_stream), for a caller that writes it straight to a file.  The sink sees nothing unless the
 * whole input was valid and encoded.                                                                       */
/* (dx_file_dexqv / _to: a .quiva image that does not fit the device beside its tokens, scratch and output -- or is larger than
 *  DEXGPU_TEXT_BUDGET bytes when that is set -- is worked through in SLICES of whole entries, like the reference streams a
 *  file of any size (dexqv.c:112-143): the scan pass over every slice (histograms added up on the host, the scan state
 *  carried along), the tables, then slice by slice again -- upload, tokens, encode, records out.  Same bytes.)          */
/* ... and with the .quiva read from a file descriptor (dx_h2d_fd: no image of it in the caller's memory at all): n bytes from
 * offset 0.  DX_E_AGAIN -- nothing has been passed to the sink -- when the file has to be handed over in memory after all (below
 * 1 MiB, larger than the device takes at once, or malformed: the in-memory driver has the reference's words for that).   */
int  dx_file_dexqv_fd_to(dx_ctx *ctx, int fd, size_t n, int lossy, dx_sink_fn sink, void *user,
                         size_t *out_len, uint64_t *errline, int *errcode);
int  dx_file_dexqv_to(dx_ctx *ctx, const uint8_t *text, size_t n, int lossy, dx_sink_fn sink, void *user,
                      size_t *out_len, uint64_t *errline, int *errcode);
/* dexqv of ONE file on several GPUs (one context each; contiguous entry ranges, one host thread per
 * context, scan state and 12 KB histograms merged on the host, outputs concatenated): identical
 * bytes to dx_file_dexqv.  nctx == 1 is dx_file_dexqv.                                          */
int  dx_file_dexqv_sharded(dx_ctx **ctxs, int nctx, const uint8_t *text, size_t n, int lossy,
                           uint8_t **out, size_t *out_len, uint64_t *errline, int *errcode);
/* dexta / dexar of ONE file on several GPUs: contiguous read ranges balanced by text bytes, one host
 * thread per context, no exchange at all; identical bytes to dx_file_pack2.        */
int  dx_file_pack2_sharded(dx_ctx **ctxs, int nctx, int arrow, const uint8_t *text, size_t n,
                           uint8_t **out, size_t *out_len, uint64_t *errline, int *errcode);
int  dx_file_undexqv(dx_ctx *ctx, const uint8_t *img, size_t n, int upper,
                     uint8_t **out, size_t *out_len);                       /* undexqv.c:101-208 */
/* The same in two steps, for a caller that wants the text somewhere else than in a malloc'd image (the CLI
 * streams it into the output file).  The plan -- the host walk over the record stream (dx_qv_walk) and the
 * header lines, undexqv.c:182 -- needs no GPU (it can run while a context is still being opened) and tells
 * the output's size; the run decodes on the GPU and delivers the text through the sink, in order
 * (dx_d2h_stream).  img must stay valid until the run is over.                                           */
typedef struct dx_undexqv_plan dx_undexqv_plan;
int  dx_file_undexqv_plan(const uint8_t *img, size_t n, dx_undexqv_plan **plan, size_t *out_len);
/* The plan with the GPU at hand: a large 0x55aa-keyed image is uploaded and its records are walked on the device
 * (dx_qv_walk_device), anything else -- and anything the device walk turns down -- is planned on the host as above.  Such a
 * plan holds device memory of ctx until it is freed, and runs on ctx only.  dx_file_undexqv plans this way.
 * A text that does not fit the device beside the image (or DEXGPU_TEXT_BUDGET bytes) comes out in slices of whole entries. */
int  dx_file_undexqv_plan_on(dx_ctx *ctx, const uint8_t *img, size_t n, dx_undexqv_plan **plan, size_t *out_len);
int  dx_file_undexqv_run (dx_ctx *ctx, const dx_undexqv_plan *plan, int upper, dx_sink_fn sink, void *user);
/* The record index the plan holds, as host arrays of the caller's (release with dx_qv_index_free; no group index): where every
 * record and segment of the image stands -- what the walk found, wherever it ran.                                       */
int  dx_file_undexqv_plan_index(const dx_undexqv_plan *plan, dx_qv_index *idx);
void dx_file_undexqv_plan_free(dx_undexqv_plan *plan);
void dx_file_free(void *p);

/* ------------------------------------------------------------------------------------------
 *  round-trip check: does the image give the text back?  (neither the reference nor its tools ever ask)
 * ------------------------------------------------------------------------------------------ */
/* Compares n units of two device buffers: unit i is d_a[d_a_off[i] .. + d_a_len[i]) against d_b[d_b_off[i] .. + d_b_len[i]),
 * offsets of any alignment, lengths from 0 up.  *first_unit = the smallest index whose two ranges differ (UINT64_MAX: none
 * does), *first_pos = the first differing byte in it -- min(a_len, b_len) when one range is the other's beginning --,
 * *n_differ = how many units differ.  n_differ == NULL: not counted, and units behind a difference already found are not
 * read.  One read of the answer per call (it waits for the context's stream).  Reads 2 bytes per byte compared, writes nothing
 * else (csrc/verify/dx_verify.hip).                                                                                  */
int dx_verify_ranges(dx_ctx *ctx, const uint8_t *d_a, const uint64_t *d_a_off, const uint32_t *d_a_len,
                     const uint8_t *d_b, const uint64_t *d_b_off, const uint32_t *d_b_len, uint64_t n,
                     uint64_t *first_unit, uint32_t *first_pos, uint64_t *n_differ);

enum { DX_KIND_FASTA = 0, DX_KIND_ARROW = 1, DX_KIND_QUIVA = 2 };
enum { DX_VERIFY_NONE = 0,      /* nothing differs */
       DX_VERIFY_HEADER = 1,    /* a header line is not the one the decoder prints */
       DX_VERIFY_BODY = 2,      /* a byte of a record's sequence / QV lines differs */
       DX_VERIFY_LENGTH = 3,    /* the lines of one side end where the other's go on */
       DX_VERIFY_COUNT = 4,     /* one side has more records */
       DX_VERIFY_IMAGE = 5 };   /* the image does not parse or decode (dx_last_error has the library's words) */
typedef struct
  { int32_t  ok;                /* 1: decoding the image with the options below gives the text back, byte for byte */
    int32_t  upper;             /* the case the text wants: undexta / undexqv -U (arrow: 0) */
    uint32_t width;             /* the line width the text wants: undexta / undexar -w (quiva: 0) */
    int32_t  where;             /* DX_VERIFY_*; what follows describes the FIRST record, in file order, that differs in any way */
    uint64_t records_src, records_img;
    uint64_t record;            /* 0-based (COUNT: the first record only one side has; IMAGE: 0) */
    uint64_t line;              /* 0-based line of the record in the text, 0 = its header line */
    uint64_t column;            /* 0-based byte in that line */
    uint64_t src_byte;          /* where that is in the text */
    uint64_t img_byte;          /* where the record begins in the image (fasta / arrow BODY: the byte that holds the symbol) */
  } dx_verify_report;

/* Is `img` (a .dexta / .dexar / .dexqv image, kind DX_KIND_*) the text it was made from?  The decode options are read off the
 * text: upper = its first sequence (quiva: deletion tag) letter is upper case; width = the length of the first sequence line
 * that another line of the same record follows, else the longest sequence, 1 at least.  The text is indexed and the image
 * walked by the drivers' own code, the image decoded on the device by the decoders' own kernels, the bodies compared THERE
 * (dx_verify_ranges: the decoded text is never downloaded), the header lines here against what the decoders print.  lossy
 * (quiva): the text is compared after dx_qv_lossy_text -- what dexqv -l promises to keep.  A text that does not fit the device
 * beside image and decoded text (or DEXGPU_TEXT_BUDGET) goes in slices of whole records.  DX_OK whenever there is an answer:
 * it stands in *rep.  A text that does not index is the error it is for dx_file_pack2 / dx_file_dexqv.                 */
int  dx_file_verify(dx_ctx *ctx, int kind, const uint8_t *text, size_t n, const uint8_t *img, size_t m, int lossy,
                    dx_verify_report *rep);

/* ------------------------------------------------------------------------------------------
 *  digest: the CRC-32 of what an image decodes to, once the text is gone  (none of the three formats carries a checksum)
 * ------------------------------------------------------------------------------------------ */
/* CRC-32 (zlib: polynomial 0xEDB88320 reflected, initial value and final xor 0xFFFFFFFF) of n byte ranges of a device buffer:
 * d_crc[j] = crc32(d_buf[d_off[j] .. d_off[j] + d_len[j])), any offset, any length from 0 (crc 0) up, ranges may overlap or repeat.
 * Nothing outside [0, buf_bytes) is read; DX_E_FORMAT with *bad_unit = the smallest j whose range does not lie inside it
 * (UINT64_MAX otherwise; may be NULL), checked by the kernel, one read-back a call (the convention of dx_reads_unpack).
 * n < 2^31.  Short units go a lane each, long ones a wave each, those of 1 MiB and more over many waves (csrc/digest/dx_crc.hip). */
int dx_crc32_ranges(dx_ctx *ctx, const uint8_t *d_buf, uint64_t buf_bytes, const uint64_t *d_off, const uint64_t *d_len,
                    uint64_t n, uint32_t *d_crc, uint64_t *bad_unit);

/* The CRC-32 of the units' concatenation in index order, from their CRCs and lengths alone (device arrays), and its length:
 * n == 0 gives 0 and 0.  One read-back.                                                                                    */
int dx_crc32_fold(dx_ctx *ctx, const uint32_t *d_crc, const uint64_t *d_len, uint64_t n, uint32_t *crc, uint64_t *bytes);

/* host: zlib's crc32_combine -- crc(A || B) from crc(A), crc(B) and B's length */
uint32_t dx_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

typedef struct { uint32_t crc32, reserved; uint64_t bytes, records; } dx_digest;
/* The CRC-32 and the size of the text undexta [-U] [-w<width>] / undexar [-w<width>] / undexqv [-U] writes for img (kind
 * DX_KIND_FASTA / _ARROW / _QUIVA; arrow ignores upper, quiva ignores width): header lines included, byte for byte the output of
 * dx_file_unpack2 / dx_file_undexqv -- which is never assembled or downloaded.  rec_crc != NULL: also *rec_crc[i] = the CRC-32
 * of record i's text, its header line included (malloc'd, dx_file_free), to find WHICH records of two files differ.
 * Errors are those of dx_file_unpack2 / dx_file_undexqv for the same image; *out is then untouched.
 * The image is walked and decoded by the drivers' own code, slice by slice when the text does not fit the device (or
 * DEXGPU_TEXT_BUDGET); the header lines, printed on the host, are hashed on the device like the bodies.               */
int dx_file_digest(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, int upper, uint32_t width,
                   dx_digest *out, uint32_t **rec_crc);

/* The options that give a text back, read off it as dx_file_verify reads them (see there): *upper, *width (quiva: 0).  A text that
 * does not index is the error it is for dx_file_pack2 / dx_file_dexqv.  Host only.                                      */
int dx_file_text_options(int kind, const uint8_t *text, size_t n, int *upper, uint32_t *width);

/* ------------------------------------------------------------------------------------------
 *  census: what an archive holds, counted where it lies  (dex2DB.c:587-595, 793-797, 896-913 count this on one core)
 * ------------------------------------------------------------------------------------------ */
/* The composition of packed reads (csrc/census/dx_census.hip).  Unit j is what it is for dx_reads_unpack: symbols [d_beg[j], d_beg[j] +
 * d_len[j]) of the packed read that starts at d_in + d_boff[j], any byte offset, any phase, d_beg == NULL: all 0.  d_counts[4 j + c]
 * (may be NULL) = how many of the unit's symbols have code c, total[c] (host; may be NULL) = the sum over the call's units.  The pad
 * bits of a read's last byte and the symbols in front of d_beg[j] are not counted; units may overlap or repeat; nothing is decoded,
 * and nothing outside [0, in_bytes) is read.  Bad units are dx_reads_unpack's: DX_E_FORMAT with *bad_unit = the smallest such j
 * (UINT64_MAX otherwise; may be NULL), checked by the kernel, one read-back a call (the totals come with it).  n < 2^31.
 * On a .bps / .arw payload with DAZZ_READ.boff / .rlen the totals are DAZZ_DB.freq (times totlen), for any selection of reads.   */
int dx_code_counts(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes,
                   const uint64_t *d_boff, const uint32_t *d_beg /* NULL: all 0 */, const uint32_t *d_len, uint64_t n,
                   uint32_t *d_counts /* n x 4, may be NULL */, uint64_t total[4] /* host */, uint64_t *bad_unit /* may be NULL */);

/* Byte-value histograms and byte sums of n ranges of a device buffer: range j = d_buf[d_off[j] .. d_off[j] + d_len[j]) adds its
 * bytes' values to table d_kind[j] (d_kind == NULL: all 0) of the nkinds (1 to 8) tables of hist (host, nkinds x 256; may be
 * NULL), and d_sum[j] (may be NULL) = the sum of its bytes.  Offsets of any alignment, lengths from 0 up, ranges may overlap or
 * repeat (dx_crc32_ranges' conventions).  DX_E_FORMAT with *bad_unit = the smallest j whose range does not lie inside
 * [0, buf_bytes) or whose kind is not below nkinds (UINT64_MAX otherwise; may be NULL); one read-back a call.  n < 2^31.       */
int dx_byte_hist_ranges(dx_ctx *ctx, const uint8_t *d_buf, uint64_t buf_bytes, const uint64_t *d_off, const uint64_t *d_len,
                        const uint8_t *d_kind /* NULL: all 0 */, int nkinds /* 1..8 */, uint64_t n,
                        uint64_t *d_sum /* n, may be NULL */, uint64_t *hist /* host, nkinds x 256 */, uint64_t *bad_unit);

typedef struct
  { uint64_t records, symbols;
    uint32_t min_len, max_len, n50, reserved;    /* all 0 for an image without records */
    uint64_t code[4];                            /* fasta: a c g t; arrow: 1 2 3 4; quiva: zeros */
    uint64_t hist[5][256];                       /* quiva: byte values of the del, tag, ins, mrg, sub lines as undexqv (no -U) writes them, newlines not counted; 2-bit kinds: zeros */
  } dx_census;

/* host only: records, symbols, min_len, max_len and n50 of n lengths (the other fields of *out are left as they are).  N50: over the
 * lengths sorted downward, the length at which the running sum first reaches half of the total (2 * running >= symbols); 0 without
 * symbols.  Two counting passes, no sort.                                                                                       */
int dx_census_lengths(const uint32_t *len, uint64_t n, dx_census *out);

/* The census of a .dexta / .dexar / .dexqv image (kind DX_KIND_*).  fasta / arrow: the image is walked as dx_file_unpack2 walks it,
 * uploaded, and the packed reads counted where they lie (dx_code_counts): no text is made.  quiva: the image is planned and decoded
 * as dx_file_digest does it, slice by slice, and every entry's five lines are counted where they are made (dx_byte_hist_ranges,
 * kinds 0..4; the tag line in lower case): the text is never downloaded.  An image that does not fit the device (or exceeds
 * DEXGPU_TEXT_BUDGET: bytes of image for the 2-bit kinds, bytes of text for quiva) goes in slices of whole records.
 * The optional results are malloc'd (dx_file_free): *rec_len = every record's symbols; *rec_code (2-bit kinds; n x 4) = its symbols
 * code by code; *rec_sum (quiva; n x 5) = the byte sums of its five lines.  One that does not apply to the kind comes back NULL.
 * Errors are those of dx_file_unpack2 / dx_file_undexqv for the same image; *out is then untouched.                             */
int dx_file_census(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, dx_census *out,
                   uint32_t **rec_len, uint32_t **rec_code /* n x 4; 2-bit kinds */, uint64_t **rec_sum /* n x 5; quiva */);

/* ------------------------------------------------------------------------------------------
 *  subset: a new archive cut out of an old one, without the round trip through text  (undexta | a text filter | dexta today)
 * ------------------------------------------------------------------------------------------ */
/* dx_reads_repack (device in, device out; csrc/reads/dx_repack.hip), the packed-to-packed sibling of dx_reads_unpack: unit j is
 * what it is there -- symbols [d_beg[j], d_beg[j] + d_len[j]) of the packed read that starts at d_in + d_boff[j], any byte offset,
 * any phase, d_beg == NULL: all 0 -- and leaves as Compress_Read's bytes of those symbols (DB.c:319-338): (d_len[j] + 3) >> 2
 * bytes at d_out + d_out_off[j] (any alignment), symbol i in bits 7 - 2 (i & 3), 6 - 2 (i & 3) of byte i >> 2, the symbols the
 * last byte lacks 0 (DB.c:329-334).  NOT ONE BYTE outside those is written: in a .dexta / .dexar image the bytes on both sides of
 * a record's payload are other records' framing.  d_len[j] == 0 writes nothing.  Units may overlap or repeat in the input; the
 * outputs are the caller's to keep disjoint.  Nothing outside [0, in_bytes) is read.  Bad units are dx_reads_unpack's: DX_E_FORMAT
 * with *bad_unit = the smallest such j (UINT64_MAX otherwise; may be NULL), checked by the kernel, one read-back a call.  n < 2^31. */
int dx_reads_repack(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes,
                    const uint64_t *d_boff, const uint32_t *d_beg /* NULL: all 0 */, const uint32_t *d_len,
                    uint64_t n, uint8_t *d_out, const uint64_t *d_out_off, uint64_t *bad_unit /* may be NULL */);

/* n byte ranges copied on the device (the same kernel at phase 0): d_dst[d_dst_off[j] .. + d_len[j]) = d_src[d_src_off[j] .. + d_len[j]),
 * any alignment on both sides, lengths from 0 up, nothing written outside them; sources may overlap or repeat, the destinations are
 * the caller's to keep disjoint, and d_src and d_dst do not overlap.  dx_crc32_ranges' conventions: DX_E_FORMAT with *bad_unit = the
 * smallest j whose source does not lie inside [0, src_bytes) (UINT64_MAX otherwise; may be NULL), one read-back a call.  n < 2^31.
 * NOT A GENERAL COPY: a range is ONE wavefront's however long it is (16 bytes a lane a step), which suits many ranges of a line's or a
 * read's size -- a batch of few, long ranges (from a MiB on) keeps a few of the device's wavefronts busy and the rest idle, and is
 * hipMemcpyAsync's business, not this call's.  dx_file_subset gathers the five lines of a .quiva entry's interval with it: a dx_qv_batch
 * fixes an entry's line stride at d_len + line_pad, so an interval of a decoded entry cannot be coded where it lies.          */
int dx_copy_ranges(dx_ctx *ctx, const uint8_t *d_src, uint64_t src_bytes,
                   const uint64_t *d_src_off, const uint64_t *d_len, uint64_t n,
                   uint8_t *d_dst, const uint64_t *d_dst_off, uint64_t *bad_unit /* may be NULL */);

/* Host only, no GPU: the framing of the image dx_file_subset makes of a .dexta / .dexar image (kind DX_KIND_FASTA / _ARROW), and
 * the units dx_reads_repack fills it with.  The selection is dx_file_subset's (see there).  The image is walked as dx_file_unpack2
 * walks it (legacy and byte-swapped layouts too); *frame (malloc'd, dx_file_free; *out_len bytes) is the finished image in the
 * current native layout with every payload byte 0: key, prefix length and the IMAGE's prefix (dexta.c:124-129), then per unit the
 * well-delta chain, restarted at 0 and run over the selected records (dexta.c:187-193), beg and end moved to B + beg[j], B + end[j],
 * and qv (dexta.c:194-198) or the four SN words as the image has them (dexar.c:204: copied, not derived from printed text).
 * Unit j of dx_reads_repack: the read at img + (*src_off)[j], its symbols [(*src_beg)[j], .. + (*len)[j]), to *frame + (*dst_off)[j].
 * The four arrays (n_ids values each; malloc'd, dx_file_free) are optional: NULL leaves one out.  With n_ids == UINT64_MAX (every
 * record) the call gives the frame alone: the arrays would have a length it does not hand back, and asking for one is DX_E_ARG.
 * Errors are dx_file_subset's.                                                                                              */
int dx_file_subset_layout(int kind, const uint8_t *img, size_t m,
                          const uint64_t *ids, const uint32_t *beg, const uint32_t *end, uint64_t n_ids,
                          uint8_t **frame, size_t *out_len,
                          uint64_t **src_off, uint32_t **src_beg, uint32_t **len, uint64_t **dst_off);

/* A new image cut out of img (a .dexta / .dexar / .dexqv image, kind DX_KIND_*; legacy and byte-swapped layouts as the decoders
 * take them).  Unit j is record ids[j] (ids == NULL: records 0 .. n_ids - 1; with beg == end == NULL as well, n_ids == UINT64_MAX
 * stands for the image's record count -- every record whole, for a caller that has not walked the image; with an array it is
 * DX_E_ARG, and an image without records DX_E_DEGENERATE): all of it when beg == NULL (then end == NULL too),
 * else its symbols [beg[j], end[j]), beg[j] <= end[j] <= its length; beg[j] == end[j] gives an empty record.  ids must not
 * decrease; an id may repeat (several subreads of one well, as dextract writes them).  *out (malloc'd, dx_file_free) is BYTE FOR
 * BYTE the file dexta / dexar / dexqv [-l] writes (dexta.c:104-205, dexar.c:103-211, dexqv.c:81-143) for the text undexta /
 * undexar / undexqv prints for img with only the selected records kept, in that order, each record's sequence (quiva: each of
 * its five lines) cut to [beg, end) and the well/B_E of its header line rewritten to well/(B + beg)_(B + end) -- always in the
 * current native layout.  Neither format stores the decode options (-U, -w), and neither encoder's output depends on them.
 * fasta / arrow: dx_file_subset_layout, then the packed reads re-packed on the device straight into the framed image
 * (dx_reads_repack); no text is made.  quiva: the selection gets its OWN coding -- the entries are decoded as dx_file_undexqv
 * decodes them, the selected intervals gathered on the device (dx_copy_ranges), and scan, histograms, dx_qv_build and the
 * encode run over that text exactly as dx_file_dexqv would treat it (lossy: dexqv -l); a text dexqv refuses is dx_file_dexqv's
 * error for it.  An image that does not fit the device (or exceeds DEXGPU_TEXT_BUDGET: bytes of image for the 2-bit kinds, of
 * text for quiva) goes in slices of whole source records; the quiva text is then decoded twice, once for each of dexqv's passes.
 * What a slice MAKES is bounded too for the 2-bit kinds: with ids that repeat, a slice ends once its units' part of the new image
 * would pass the same figure (one unit at least), and the next slice takes the record up again.  For quiva it is not: a slice's
 * gathered text holds every selected interval of the slice's entries, so a selection that repeats an entry k times needs k times
 * that entry's text on the device at once (DX_E_NOMEM when it is not there).
 * DX_E_ARG (dx_last_error names the unit j) for a decreasing id, an id that is not below the record count, beg[j] > end[j],
 * end[j] > the record's length, or only one of beg / end; DX_E_DEGENERATE for n_ids == 0; else the decoders' errors for img.  */
int dx_file_subset(dx_ctx *ctx, int kind, const uint8_t *img, size_t m,
                   const uint64_t *ids, const uint32_t *beg, const uint32_t *end, uint64_t n_ids,
                   int lossy /* quiva */, uint8_t **out, size_t *out_len);

/* ------------------------------------------------------------------------------------------
 *  extract: chosen records as text  (undexta | a text filter today; dx_file_subset + a decoder through this library)
 * ------------------------------------------------------------------------------------------ */
/* dx_reads_unpack_lines (device in, device out; csrc/reads/dx_lines.hip), dx_reads_unpack with k_pack2_decode's line ends: unit j is
 * what it is there -- symbols [d_beg[j], d_beg[j] + d_len[j]) of the packed read that starts at d_in + d_boff[j], any byte offset,
 * any phase, d_beg == NULL: all 0 -- and leaves as T = d_len[j] + (d_len[j] + width - 1) / width bytes at d_out + d_out_off[j]
 * (any alignment): the letters with '\n' behind every width-th one and behind the last one (undexta.c:263-270).  NOT ONE BYTE
 * outside those T is written, and there is no delimiter: in dx_file_extract's layout the neighbours are header lines.  d_len[j] ==
 * 0 writes nothing.  letters: DX_LETTERS_LOWER, _UPPER or _ARROW (numbers have no lines: DX_E_ARG); width >= 1 (0: DX_E_ARG, as
 * for dx_pack2_decode), and a width beyond every length is one line a unit.  Units may overlap or repeat in the input; the outputs
 * are the caller's to keep disjoint.  Nothing outside [0, in_bytes) is read.  Bad units are dx_reads_unpack's: DX_E_FORMAT with
 * *bad_unit = the smallest such j (UINT64_MAX otherwise; may be NULL), checked by the kernel, one read-back a call.  n < 2^31.  */
int dx_reads_unpack_lines(dx_ctx *ctx, int letters, const uint8_t *d_in, uint64_t in_bytes,
                          const uint64_t *d_boff, const uint32_t *d_beg /* NULL: all 0 */, const uint32_t *d_len,
                          uint64_t n, uint32_t width, uint8_t *d_out, const uint64_t *d_out_off, uint64_t *bad_unit /* may be NULL */);

/* The text undexta [-U] [-w<width>] / undexar [-w<width>] / undexqv [-U] prints for chosen records of img alone (a .dexta / .dexar /
 * .dexqv image, kind DX_KIND_*; legacy and byte-swapped layouts as the decoders take them; arrow ignores upper, quiva ignores
 * width).  The selection is dx_file_subset's -- unit j is record ids[j], whole or its symbols [beg[j], end[j]); ids == NULL: records
 * 0 .. n_ids - 1; n_ids == UINT64_MAX with no array: every record -- but the ids may come in ANY order (a text has no well-delta
 * chain), and may repeat.  *text (malloc'd, dx_file_free; *text_bytes of it) has the units in the selection's order: the header line
 * with well/B_E rewritten to well/(B + beg)_(B + end), then the sequence (quiva: each of the five lines) cut to [beg, end); a unit
 * with beg == end is its header line alone for the 2-bit kinds, its header line and five empty lines for quiva.  (*toff)[j] (n_ids
 * + 1 values, malloc'd; toff may be NULL) is where unit j's header line begins, (*toff)[n_ids] = *text_bytes.  For a selection
 * dx_file_subset accepts the text is, byte for byte, dx_file_unpack2 / dx_file_undexqv of dx_file_subset's image -- without
 * that image: nothing is framed, no coding is built, nothing is encoded.
 * fasta / arrow: the image is walked on the host, only the selected reads' packed spans travel (dx_reads_uncompress's loader and
 * its rule), and one dx_reads_unpack_lines a slice writes the lines where they belong.  quiva: the stream is walked as
 * dx_file_undexqv walks it (the format stores no lengths: that cost stays), only the selected records' bytes travel unless the
 * walk has left the image on the device, and dx_qv_decode runs on the gathered starts.  A whole entry is decoded where it ends
 * up; for an interval the WHOLE entry is decoded into scratch first -- a Huffman stream has no way in at symbol beg -- and
 * dx_copy_ranges gathers the five line intervals, so an interval costs its entry's decode, and an entry selected k times is
 * decoded k times.  A selection whose text exceeds DEXGPU_TEXT_BUDGET bytes, or what is free on the device, goes in slices of whole
 * units; the text is the same.
 * n_ids == 0: DX_OK and an empty text.  DX_E_ARG (dx_last_error names the unit j) for an id that is not below the record count,
 * beg[j] > end[j], end[j] > the record's length, only one of beg / end, or width == 0 for a 2-bit kind; else the decoders' errors
 * for img.                                                                                                                    */
int dx_file_extract(dx_ctx *ctx, int kind, const uint8_t *img, size_t m,
                    const uint64_t *ids, const uint32_t *beg, const uint32_t *end, uint64_t n_ids,
                    int upper, uint32_t width, uint8_t **text, size_t *text_bytes, uint64_t **toff /* n_ids + 1, may be NULL */);

/* ------------------------------------------------------------------------------------------
 *  compare: how two archives of the same records differ, without either text  (undexqv of both and a text diff today)
 * ------------------------------------------------------------------------------------------ */
typedef struct { uint64_t differ, units, sum_abs, max_abs; } dx_diff_tally;

/* n byte ranges of device buffer a against n of device buffer b, counted (csrc/compare/dx_diff.hip): unit j is d_a[d_a_off[j] .. +
 * d_len[j]) against d_b[d_b_off[j] .. + d_len[j]), offsets of any alignment on either side, lengths from 0 up, ranges may overlap
 * or repeat.  d_kind[j] (NULL: all 0) names one of nkinds (1 to 8) tallies, and a_and[kind] (host, nkinds bytes; NULL: all 0xff) is
 * ANDed onto side a's bytes before they are compared: dexqv -l's rounding is 0xFE on the insertion and 0xFC on the merge line
 * (QV.c:1406-1415).  d_differ[j] (may be NULL) = the unit's differing bytes, d_first[j] (may be NULL) = the first of them, UINT32_MAX
 * if none.  tally[k] (host, nkinds; may be NULL): kind k's differing bytes, its units with at least one, the sum and the largest of
 * |a - b| after the mask.  *first (may be NULL) = the smallest unit << 32 | position that differs, all ones if none does.  Where
 * dx_verify_ranges stops at the first difference, this reads everything, and every byte once: nothing outside a unit's two ranges
 * is read.  DX_E_FORMAT with *bad_unit = the smallest j whose range does not lie inside a_bytes / b_bytes or whose kind is not below
 * nkinds (UINT64_MAX otherwise; may be NULL); one read-back a call.  n < 2^31; n == 0 gives zeros.                             */
int dx_diff_ranges(dx_ctx *ctx, const uint8_t *d_a, uint64_t a_bytes, const uint64_t *d_a_off,
                   const uint8_t *d_b, uint64_t b_bytes, const uint64_t *d_b_off, const uint32_t *d_len,
                   const uint8_t *d_kind /* NULL: all 0 */, int nkinds /* 1..8 */, const uint8_t *a_and /* host; NULL: all 0xff */,
                   uint64_t n, uint32_t *d_differ /* may be NULL */, uint32_t *d_first /* may be NULL */,
                   dx_diff_tally *tally /* host, nkinds */, uint64_t *first, uint64_t *bad_unit);

/* The same for packed reads where they lie, nothing decoded: unit j is symbols [0, d_len[j]) of the packed read at d_a + d_a_boff[j]
 * against those of the one at d_b + d_b_boff[j] (four symbols a byte, the first in the top two bits: DB.c:319-338).  d_differ[j] =
 * the symbols that differ, d_first[j] = the first of them (UINT32_MAX: none); total[0] (host; may be NULL) = the differing symbols
 * of the call, total[1] = the units that have one; *first = the smallest unit << 32 | symbol.  The pad bits of a read's last byte
 * are NOT compared: a foreign writer may leave anything there.  Bad units are dx_code_counts' on either side.  n < 2^31.          */
int dx_code_diff(dx_ctx *ctx, const uint8_t *d_a, uint64_t a_bytes, const uint64_t *d_a_boff,
                 const uint8_t *d_b, uint64_t b_bytes, const uint64_t *d_b_boff, const uint32_t *d_len, uint64_t n,
                 uint32_t *d_differ /* may be NULL */, uint32_t *d_first /* may be NULL */, uint64_t total[2] /* host */,
                 uint64_t *first, uint64_t *bad_unit);

typedef struct
  { int32_t  same;                               /* 1: the counts, the prefixes, every header, every length and every symbol (after the mask) are equal */
    int32_t  lines;                              /* lines a record compared: 1 for the 2-bit kinds, 5 for quiva */
    int32_t  prefix_differs, reserved;
    uint64_t records_a, records_b;               /* the first min of them are compared */
    uint64_t headers_differ, first_header;       /* records whose well, beg, end or qv / four SN words differ; the first (UINT64_MAX: none) */
    uint64_t lengths_differ, first_length;       /* records whose symbol counts differ (compared over the shorter one); the first */
    uint64_t records_differ, first_record;       /* records with a differing symbol; the first difference in file order: its record */
    uint32_t first_line, first_column;           /* ... (UINT64_MAX: none), line and column */
    uint64_t differ[5], line_records[5];         /* per line: differing symbols, records that have one */
    uint64_t sum_abs[5], max_abs[5];             /* quiva: the sum and the largest of |a - b| (2-bit kinds: 0) */
  } dx_compare;

/* How two images of one kind (DX_KIND_*) differ: any key, legacy layout, byte order or coding on either side, as dx_file_unpack2 /
 * dx_file_undexqv accept them; records are paired by index.  Quiva lines are del, tag, ins, mrg, sub; the tag line is compared in
 * lower case on both sides; newlines and header lines are not compared (the headers' FIELDS are, as the host walks decode them).
 * lossy (quiva only; DX_E_ARG else): side a's insertion and merge lines are masked as dexqv -l rounds them before the comparison,
 * so same == 1 says "b is exactly what dexqv -l keeps of a".  *rec_differ (may be NULL; malloc'd, dx_file_free): min(records) x
 * lines counts, the differing symbols of every compared record line by line.
 * fasta / arrow: both images are walked on the host and uploaded, and the packed reads compared where they lie (dx_code_diff): no
 * text is made.  quiva: both images are planned and decoded by the drivers' own code, each with its own coding, and the line ranges
 * compared where they are made (dx_diff_ranges, kinds 0..4): nothing of either text comes back.  A pair that does not fit the
 * device beside its two texts, or whose texts together exceed DEXGPU_TEXT_BUDGET (2-bit kinds: bytes of image), goes in slices of
 * whole records, the same record range on both sides; the report is the same.
 * An image that does not parse or decode is the error it is for its own driver, dx_last_error begins with "a:" or "b:", and *out
 * is untouched.                                                                                                                 */
int dx_file_compare(dx_ctx *ctx, int kind, const uint8_t *img_a, size_t m_a, const uint8_t *img_b, size_t m_b,
                    int lossy, dx_compare *out, uint32_t **rec_differ /* may be NULL */);

/* ------------------------------------------------------------------------------------------
 *  find: where given sequences occur in an archive, without its text  (undexta -U of the whole file and a text search today)
 * ------------------------------------------------------------------------------------------ */
typedef struct { uint64_t code; uint32_t len, max_mis; } dx_query;      /* symbol i of the query in bits 2 (len - 1 - i) + 1, 2 (len - 1 - i) of
                                                                            code: the first symbol on top, as in a packed read; bits above 2 len are 0 */
typedef struct { uint64_t record; uint32_t pos; uint16_t query; uint8_t strand, mis; } dx_hit;   /* 16 bytes */

/* Up to 64 queries of 1 to 32 symbols searched in n packed reads where they lie, nothing decoded (csrc/find/dx_find.hip; a text
 * search of the decoded reads on one core today).  Unit j is what it is for dx_code_counts: symbols [d_beg[j], d_beg[j] + d_len[j])
 * of the packed read at d_in + d_boff[j], any byte offset, any phase, units may overlap or repeat.  Query k hits unit j at pos when
 * 0 <= pos <= d_len[j] - q[k].len and the unit's symbols [pos, pos + q[k].len) differ from the query's in at most q[k].max_mis
 * places; overlapping hits all count, a unit shorter than a query has no hit of it, duplicate queries each report.  The symbols in
 * front of d_beg[j], those behind the unit's end, the pad bits of a read's last byte and every byte that is not the unit's are part
 * of no window, and nothing outside [0, in_bytes) is read.
 * d_count[j] (may be NULL) = the unit's hits over all queries, UINT32_MAX when there are more; total[k] (host, nq; may be NULL) =
 * query k's hits over the call; *hits = their sum, listed or not.  d_hits (cap entries; may be NULL when cap == 0) gets the first
 * min(cap, *hits) hits in the order (unit, pos, query) -- record = j, strand = 0, mis = the distance --, the same on every call:
 * places come from counts and prefix sums, no atomic cursor.  Not one byte behind d_hits[min(cap, *hits)] is written; cap == 0 runs
 * the counting pass alone.  cap < 2^32.
 * DX_E_FORMAT with *bad_unit = the smallest j that does not lie inside the in_bytes (UINT64_MAX otherwise; may be NULL); such units
 * are not searched; checked by the kernel, one read-back a call (with a list: two).  DX_E_ARG for nq outside 1..64, a len outside
 * 1..32, bits of code above 2 len, a NULL pointer that is needed, n >= 2^31.  n == 0 gives zeros.                               */
int dx_code_find(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes,
                 const uint64_t *d_boff, const uint32_t *d_beg /* NULL: all 0 */, const uint32_t *d_len, uint64_t n,
                 const dx_query *q /* host */, uint32_t nq /* 1..64 */,
                 uint32_t *d_count /* n, may be NULL */, dx_hit *d_hits /* cap, may be NULL when cap == 0 */, uint64_t cap,
                 uint64_t total[] /* host, nq; may be NULL */, uint64_t *hits /* host: all of them, listed or not */,
                 uint64_t *bad_unit /* may be NULL */);

typedef struct { uint64_t records, records_hit, hits, listed; uint64_t per_pattern[64][2]; } dx_find;

/* Which records of a .dexta / .dexar image (kind DX_KIND_FASTA or DX_KIND_ARROW; any key, legacy layout or byte order, as
 * dx_file_unpack2 takes them) contain the given patterns, and where (undexta -U | a text search today).  A pattern is 1 to 32
 * letters, acgtACGT for fasta, 1234 for arrow; npat is 1 to 64, with both_strands 1 to 32.  max_mis (one figure for all patterns,
 * below the shortest pattern's length) is the Hamming distance a window may have.  both_strands (fasta only): every pattern is
 * also searched as its reverse complement; such a hit has strand 1 and pos = the leftmost symbol of the window on the read as
 * stored; a pattern that is its own reverse complement is searched once and reports strand 0 only.
 * The search is over what the archive HOLDS: an N that dexta stored as a is an a.  The hits are exactly those a search of the letters
 * undexta -U / undexar prints, record by record, would find; a window never spans two records.
 * out->records = the image's records, records_hit those with a hit, hits all hits, listed = min(hits, max_hits),
 * per_pattern[p][s] the hits of pattern p on strand s.  *hits (may be NULL; malloc'd, dx_file_free) has `listed` entries in the
 * order (record, pos, pattern, strand), query = the pattern's index; *rec_hits (may be NULL; malloc'd) one count a record,
 * UINT32_MAX when there are more.
 * The image is walked on the host and uploaded, and the reads are searched where they lie (dx_code_find): no text is made.  An
 * image that does not fit the device, or exceeds DEXGPU_TEXT_BUDGET (bytes of image, as for dx_file_census), goes in slices of
 * whole records; record numbers, the order and max_hits run across the slices as if there were none.
 * DX_E_ARG (dx_last_error says why; for a letter the pattern's index and the column) for DX_KIND_QUIVA, a pattern of 0 or more
 * than 32 letters or with a letter that is not the kind's, npat out of range, max_mis not below the shortest pattern,
 * both_strands for arrow; else dx_file_unpack2's errors for the image, and *out is untouched.                                    */
int dx_file_find(dx_ctx *ctx, int kind, const uint8_t *img, size_t m,
                 const char *const *pattern, uint32_t npat, uint32_t max_mis, int both_strands,
                 uint64_t max_hits, dx_find *out, dx_hit **hits /* may be NULL */, uint32_t **rec_hits /* may be NULL */);

/* ------------------------------------------------------------------------------------------
 *  find with indels: where given sequences occur within an edit distance  (raw reads err by insertion and deletion, which the
 *  Hamming distance of find does not see: an adapter with one inserted base is half its length away from the pattern)
 * ------------------------------------------------------------------------------------------ */
typedef struct { uint64_t code[2]; uint32_t len, max_err; } dx_equery;  /* symbol i of the query in bits 2 (31 - (i & 31)) + 1, 2 (31 - (i & 31))
                                                                           of code[i >> 5]: the first symbol on top of code[0]; unused bits are 0 */
#define DX_FIND_EDIT_STRETCH 128u       /* the ends a lane of the kernel takes at a time (csrc/find/dx_find_edit.hip says why): no part of the
                                           answer, which is the same for any value; here for the tests, which lay hits across its multiples */

/* Up to 64 queries of 1 to 64 symbols searched in n packed reads where they lie, nothing decoded, by Myers' bit-vector algorithm
 * (csrc/find/dx_find_edit.hip).  Unit j is what it is for dx_code_find.  For a unit U of L symbols and a query P of m symbols with the
 * error bound k = max_err, 0 <= k < m:
 *     D(e) = min over 0 <= s <= e of Levenshtein(P, U[s, e)) for 1 <= e <= L; substitution, insertion and deletion each cost one; the
 *            alignment is semi-global: the start in the read is free;
 *     c(e) = min(D(e), k + 1), and c(0) = c(L + 1) = k + 1.
 * A hit of the query in the unit is an end e with c(e) <= k, c(e) < c(e - 1) and c(e) <= c(e + 1): one hit for each valley of the
 * distance, at the leftmost end of its floor.  The hit reports pos = e, the EXCLUSIVE END of the occurrence, not its start, and
 * mis = D(e).  The start lies in [e - m - D(e), e - m + D(e)]; dx_code_hit_starts finds it exactly.  A unit shorter than m - k has no
 * hit; duplicate queries each report.  The symbols in front of d_beg[j], those behind the unit's end, the pad bits of a read's last
 * byte and every byte that is not the unit's take part in nothing, and nothing outside [0, in_bytes) is read.
 * d_count, total, *hits, d_hits, cap and the list's order (unit, pos, query) are dx_code_find's: d_count[j] saturated at UINT32_MAX,
 * a total a query, *hits all hits listed or not, the first min(cap, *hits) in d_hits, the same on every call (places come from
 * counts and prefix sums, no atomic cursor), not one byte written at cap or beyond, cap == 0 runs the counting pass alone.
 * DX_E_FORMAT with *bad_unit as for dx_code_find.  DX_E_ARG for nq outside 1..64, a len outside 1..64, max_err >= len, bits of code
 * behind the len symbols, a NULL pointer that is needed, n >= 2^31, cap >= 2^32.  n == 0 gives zeros.                              */
int dx_code_find_edit(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes,
                      const uint64_t *d_boff, const uint32_t *d_beg /* NULL: all 0 */, const uint32_t *d_len, uint64_t n,
                      const dx_equery *q /* host */, uint32_t nq /* 1..64 */,
                      uint32_t *d_count /* n, may be NULL */, dx_hit *d_hits /* cap, may be NULL when cap == 0 */, uint64_t cap,
                      uint64_t total[] /* host, nq; may be NULL */, uint64_t *hits /* host: all of them, listed or not */,
                      uint64_t *bad_unit /* may be NULL */);

/* dx_file_find with that distance: which records of a .dexta / .dexar image contain the patterns within max_err edits, and where
 * they END.  A pattern is 1 to 64 letters; npat is 1 to 64, with both_strands 1 to 32; max_err (one figure for all patterns) is
 * below the shortest pattern's length.  A hit is what it is for dx_code_find_edit -- one for each valley of the distance, pos = the
 * exclusive end of the occurrence on the read as stored, mis = the distance --; a reverse complement's hit has strand 1 and its pos
 * is the end of the reverse complement's occurrence on the read as stored.  Everything else is dx_file_find's: the letters, the
 * kinds, both_strands (a pattern that is its own reverse complement is searched once), what *out, *hits and *rec_hits hold, their
 * order (record, pos, pattern, strand), the slices of whole records with record numbers, order and max_hits running across them,
 * and the errors (DX_E_ARG for DX_KIND_QUIVA, a pattern of 0 or more than 64 letters or with a letter that is not the kind's --
 * dx_last_error names the pattern's index and the column --, npat out of range, max_err not below the shortest pattern,
 * both_strands for arrow).                                                                                                       */
int dx_file_find_edit(dx_ctx *ctx, int kind, const uint8_t *img, size_t m,
                      const char *const *pattern, uint32_t npat, uint32_t max_err, int both_strands,
                      uint64_t max_hits, dx_find *out, dx_hit **hits /* may be NULL */, uint32_t **rec_hits /* may be NULL */);

/* ------------------------------------------------------------------------------------------
 *  cut: where the occurrences start, and an archive cut at them  (undexta of the whole file, a text scan on one core and dexta again
 *  today -- and the same once more for the .dexar and the .dexqv of the same run)
 * ------------------------------------------------------------------------------------------ */
/* The starts of the occurrences dx_code_find_edit found (csrc/find/dx_find_span.hip).  Units and queries are dx_code_find_edit's, and
 * d_hits is a list exactly as that call leaves it: record = the unit j, pos = the end e, query = the index into q, mis = the distance
 * d (strand is not read).  For every hit
 *     d_start[i] = the LARGEST s, 0 <= s <= e, with Levenshtein(P, U_j[s, e)) == d
 * -- the shortest stretch of the unit that ends at e and lies d edits from the pattern; |(e - s) - m| <= d.  It is found by the
 * bit-vector recurrence with the query reversed and the start anchored at e, stepped backwards from symbol e - 1 for at most m + d
 * symbols, one lane a hit.  No symbol in front of d_beg[j] is read, and nothing outside [0, in_bytes).  Hit i writes d_start[i] and
 * nothing else; n_hits == 0 launches nothing.
 * A hit is BAD when record >= n, its unit does not lie inside the in_bytes (the unit is not read), pos == 0 or pos > d_len[record],
 * query >= nq, mis > q[query].max_err, or no stretch that ends at pos lies mis from the query (the hit is not one of this data): its
 * d_start is UINT32_MAX, the good hits' starts are written all the same, and the call returns DX_E_FORMAT with *bad_hit = the
 * smallest such index (UINT64_MAX otherwise; may be NULL), one read-back a call.  DX_E_ARG for what dx_code_find_edit refuses in q and
 * nq, a NULL pointer that is needed, n >= 2^31, n_hits >= 2^32.                                                                    */
int dx_code_hit_starts(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes,
                       const uint64_t *d_boff, const uint32_t *d_beg /* NULL: all 0 */, const uint32_t *d_len, uint64_t n,
                       const dx_equery *q /* host */, uint32_t nq /* 1..64 */,
                       const dx_hit *d_hits, uint64_t n_hits, uint32_t *d_start /* n_hits */, uint64_t *bad_hit /* may be NULL */);

/* dx_file_find_edit with both ends of every listed occurrence: the same arguments, the same *out, *hits and *rec_hits, and beside them
 * *start (malloc'd, dx_file_free): `listed` values, (*start)[i] the first symbol of hit i's occurrence on the read as stored, so that
 * the occurrence is the record's symbols [(*start)[i], (*hits)[i].pos) -- for a strand-1 hit the leftmost symbol of the reverse
 * complement's occurrence.  The start is dx_code_hit_starts': the shortest stretch that ends at pos and lies mis edits from the
 * pattern.  *rec_len (may be NULL; malloc'd) = every record's symbols, from the walk the driver makes anyway.  The starts of a slice are
 * computed while its image and its hits are still on the device, one launch a slice behind the listing; record numbers, the order and
 * max_hits run across slices as for dx_file_find_edit.  start != NULL wants hits != NULL (DX_E_ARG); start == NULL is
 * dx_file_find_edit.                                                                                                              */
int dx_file_find_edit_spans(dx_ctx *ctx, int kind, const uint8_t *img, size_t m,
                            const char *const *pattern, uint32_t npat, uint32_t max_err, int both_strands,
                            uint64_t max_hits, dx_find *out, dx_hit **hits, uint32_t **rec_hits /* may be NULL */,
                            uint32_t **start, uint32_t **rec_len /* may be NULL */);

#define DX_CUT_SPLIT   0                /* every piece between the occurrences, in order */
#define DX_CUT_LONGEST 1                /* the longest piece of a record; on a tie the first */
#define DX_CUT_DROP    2                /* only the records without an occurrence, whole */
typedef struct
  { uint64_t records_in;                /* the records the plan was made for */
    uint64_t records_cut;               /* records with an occurrence of which something is kept */
    uint64_t records_dropped;           /* records with an occurrence of which nothing is kept */
    uint64_t pieces;                    /* units of the selection: the kept pieces and the untouched records */
    uint64_t symbols_in, symbols_kept;
    uint64_t spans;                     /* occurrences after the union of those that overlap or touch */
  } dx_cut;

/* Host only, no GPU: what is kept of every record once the occurrences are cut out, as a selection dx_file_subset accepts.  hits and
 * start are n_hits values as dx_file_find_edit_spans leaves them (record, pos and the start beside it; any order: they are sorted
 * here); rec_len has `records` lengths.  Within a record the spans [start, pos) of all patterns and strands are united -- spans that
 * overlap or touch become one --, and the PIECES are what lies between the united spans, in front of the first and behind the last;
 * a piece has one symbol at least.  (An empty span, start == pos, which the search never reports, cuts nothing out and parts the
 * record where it stands.)
 *   DX_CUT_SPLIT:   every piece of at least min_len symbols, in order; the id repeats, as dextract writes several subreads of a well;
 *   DX_CUT_LONGEST: the longest such piece of a record, on a tie the first;
 *   DX_CUT_DROP:    nothing of a record with an occurrence.
 * A record without an occurrence is kept whole, [0, its length), in every mode and whatever min_len is.  *ids, *beg, *end (malloc'd,
 * dx_file_free; *n_ids values each) come out with the ids not decreasing and the pieces of a record in order; *n_ids == 0 is DX_OK
 * here (dx_file_subset refuses it).  *report may be NULL.  DX_E_ARG for a hit with start > pos (a bad hit's UINT32_MAX among them),
 * pos > its record's length, record >= records, an unknown mode, a NULL pointer that is needed; nothing is handed back then.    */
int dx_hits_cut_plan(const dx_hit *hits, const uint32_t *start, uint64_t n_hits, const uint32_t *rec_len, uint64_t records,
                     uint32_t min_len, int mode, uint64_t **ids, uint32_t **beg, uint32_t **end, uint64_t *n_ids,
                     dx_cut *report /* may be NULL */);

/* A .dexta / .dexar image with the occurrences of the patterns cut out: dx_file_find_edit_spans with max_hits unlimited (patterns,
 * max_err, both_strands and their refusals are dx_file_find_edit's), dx_hits_cut_plan, dx_file_subset.  *out (malloc'd, dx_file_free;
 * *out_len bytes) is BYTE FOR BYTE the file dexta / dexar writes for the text of img with every record cut as the plan says and the
 * well/B_E of its header lines rewritten, as for dx_file_subset.  The selection comes back too (*ids, *beg, *end: malloc'd, *n_ids
 * values each; each may be NULL), so that the caller can apply it with dx_file_subset to the .dexar and the .dexqv of the same
 * records (INTEGRATION.md shows the three calls).  *report may be NULL.
 * It never cuts from part of the hits: a list that came back shorter than the hits is DX_E_NOMEM.  A selection without a unit (every
 * record dropped, or no record) is DX_E_DEGENERATE, as for dx_file_subset, and hands nothing back.  DX_E_ARG for DX_KIND_QUIVA (a
 * .dexqv has no reads to search: cut its .dexta, then apply the selection), an unknown mode, and what dx_file_find_edit refuses.  */
int dx_file_cut(dx_ctx *ctx, int kind, const uint8_t *img, size_t m,
                const char *const *pattern, uint32_t npat, uint32_t max_err, int both_strands,
                uint32_t min_len, int mode, uint8_t **out, size_t *out_len, dx_cut *report /* may be NULL */,
                uint64_t **ids /* may be NULL */, uint32_t **beg /* may be NULL */, uint32_t **end /* may be NULL */, uint64_t *n_ids /* may be NULL */);

/* ------------------------------------------------------------------------------------------
 *  k-mers: what is in the reads that nobody thought to ask for  (undexta -U of the whole file and a counting loop on one core today)
 * ------------------------------------------------------------------------------------------ */
typedef struct { uint64_t count; uint32_t code, reserved; } dx_kmer;          /* 16 bytes */
typedef struct { uint64_t records, symbols, windows, distinct, max_count; uint32_t max_code, k; } dx_kmers;   /* 48 bytes */

/* Exact counts of all k-mers, 1 <= k <= 14, of n packed reads in a direct-addressed table of 4^k 64-bit counters on the device
 * (csrc/kmers/dx_kmers.hip; 2 GiB at k = 14).  The code of a k-mer is its symbols as a base-4 number, the first on top:
 * code = sum s_i 4^(k - 1 - i), the order of a packed read and of dx_query.code.  With canonical a window counts under
 * min(code, rc(code)), rc being the codes 3 - c in reverse order; a k-mer that is its own reverse complement counts once a window.
 * Unit j is what it is for dx_code_counts and dx_code_find: symbols [d_beg[j], d_beg[j] + d_len[j]) of the packed read at
 * d_in + d_boff[j], any byte offset, any phase; units may overlap or repeat, and their windows add.  A window never spans two units,
 * a unit shorter than k has none; the symbols in front of d_beg[j], those behind the unit's end, the pad bits of a read's last byte
 * and every byte that is not the unit's are part of no window, and nothing outside [0, in_bytes) is read.
 * d_table is ADDED to: the caller zeroes it, and two calls over disjoint halves of the units leave what one call over all of them
 * leaves.  *windows (may be NULL) = sum max(0, d_len[j] - k + 1) over this call's good units.
 * DX_E_FORMAT with *bad_unit = the smallest j that does not lie inside the in_bytes (UINT64_MAX otherwise; may be NULL); such units
 * add nothing; checked by the kernel, one read-back a call.  DX_E_ARG for k outside 1..14, a NULL pointer that is needed,
 * n >= 2^31.  n == 0 changes nothing.  (canonical is a property of the codes here; dx_file_kmers refuses it for arrow.)          */
int dx_code_kmers(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes,
                  const uint64_t *d_boff, const uint32_t *d_beg /* NULL: all 0 */, const uint32_t *d_len, uint64_t n,
                  uint32_t k /* 1..14 */, int canonical,
                  uint64_t *d_table /* 4^k counters, ADDED to */, uint64_t *windows /* host, may be NULL: this call's */,
                  uint64_t *bad_unit /* may be NULL */);

/* What a table of 4^k counters holds.  spectrum[c] (host, nspec >= 2 values; may be NULL), 1 <= c < nspec - 1, = the codes whose
 * counter is c; spectrum[nspec - 1] gathers every counter >= nspec - 1; spectrum[0] is 0 always (the unseen codes are
 * 4^k - *distinct, and in canonical mode half the cells are never used).  *distinct = the counters >= 1, *max_count the largest,
 * *max_code the smallest code that has it (both 0 for an empty table); each may be NULL.  One read-back a call.                  */
int dx_kmer_spectrum(dx_ctx *ctx, const uint64_t *d_table, uint32_t k,
                     uint64_t *spectrum /* host, nspec; may be NULL */, uint32_t nspec,
                     uint64_t *distinct, uint64_t *max_count, uint32_t *max_code);

/* The codes whose counter is >= min_count (>= 1), in ascending code order, the same on every call: places come from counts and a
 * prefix sum, no atomic cursor.  *found counts all of them, listed or not; d_out gets the first min(cap, *found), and nothing is
 * written at cap or beyond; cap == 0 counts only.                                                                               */
int dx_kmer_list(dx_ctx *ctx, const uint64_t *d_table, uint32_t k, uint64_t min_count /* >= 1 */,
                 dx_kmer *d_out /* cap; may be NULL when cap == 0 */, uint64_t cap, uint64_t *found);

/* The k-mers of the reads of a .dexta / .dexar image (kind DX_KIND_FASTA or DX_KIND_ARROW; any key, legacy layout or byte order, as
 * dx_file_unpack2 takes them) added to the caller's table, so that several files can be counted into one.  The count is over what
 * the archive HOLDS (an N that dexta stored as a is an a): exactly the k-mers of the letters undexta -U / undexar prints, record by
 * record; a window never spans two records.  The image is walked on the host and uploaded, and the reads are counted where they lie
 * (dx_code_kmers); an image that does not fit the device, or exceeds DEXGPU_TEXT_BUDGET (bytes of image), goes in slices of whole
 * records.  *records, *symbols, *windows (each may be NULL) = this image's.  canonical: fasta only.  The refusals are
 * dx_file_kmers'; an image that is refused has added nothing.                                                                   */
int dx_file_kmers_add(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, uint32_t k, int canonical,
                      uint64_t *d_table, uint64_t *records, uint64_t *symbols, uint64_t *windows);

/* ... with a table of its own, zeroed, and then the spectrum and the list of it: *out = the image's records, symbols and windows,
 * the table's distinct, max_count and max_code, and k.  With min_count >= 1 and list != NULL, *list (malloc'd, dx_file_free) has
 * *listed = min(found, max_list) entries in ascending code order (reserved = 0); with min_count == 0 or list == NULL there is no
 * list.  *table (may be NULL; malloc'd, dx_file_free) = the 4^k counters.
 * DX_E_ARG (dx_last_error says why) for DX_KIND_QUIVA, an unknown kind, canonical with arrow, k outside 1..14, nspec < 2 with a
 * spectrum; else dx_file_unpack2's errors for the image, and *out is untouched.                                                  */
int dx_file_kmers(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, uint32_t k, int canonical,
                  uint64_t min_count, uint64_t max_list, dx_kmers *out,
                  uint64_t *spectrum /* host, nspec; may be NULL */, uint32_t nspec,
                  dx_kmer **list /* may be NULL */, uint64_t *listed, uint64_t **table /* may be NULL: 4^k, malloc'd */);

/* Host only, no GPU: k letters (acgtACGT, or 1234 with arrow) -> their code, with canonical min(code, rc); and a code -> its k
 * letters, upper case or 1234, and a NUL (out: k + 1 bytes).  DX_E_ARG for k outside 1..14, a letter that is not the kind's (the
 * text's end among them), a code of more than 2 k bits, a NULL pointer.                                                          */
int dx_kmer_code(int arrow, const char *letters, uint32_t k, int canonical, uint32_t *code);
int dx_kmer_letters(int arrow, uint32_t code, uint32_t k, char *out /* k + 1 */);

/* ------------------------------------------------------------------------------------------
 *  k-mers up to k = 32: every window's code written out, sorted on the device, counted off the runs  (csrc/sort/, csrc/kmers/)
 * ------------------------------------------------------------------------------------------ */
typedef struct { uint64_t code, count; } dx_kmer64;                                                      /* 16 bytes */
typedef struct { uint64_t records, symbols, windows, distinct, max_count, max_code; uint32_t k, reserved; } dx_kmers64;   /* 56 bytes */

/* d_keys[0 .. n) sorted ascending as unsigned numbers, on the device: a radix sort of 8 bits a pass from the lowest digit up
 * (csrc/sort/dx_sort.hip; no device library).  The caller promises that every key is < 2^bits (bits < 64): only the ceil(bits / 8)
 * digits that cover `bits` are passed over.  d_tmp: n keys of room, not d_keys; its contents are lost.  The sorted keys end in d_keys
 * whatever the number of passes.  The cost does not depend on how the keys are distributed.  n == 0 or bits == 0 does nothing.
 * DX_E_ARG for bits > 64, a NULL pointer with n > 0, n >= 2^36.                                                                    */
int dx_sort_u64(dx_ctx *ctx, uint64_t *d_keys, uint64_t *d_tmp /* n keys of room */, uint64_t n, uint32_t bits /* 0..64 */);

/* The codes of all windows of k symbols, 1 <= k <= 32, of n packed reads, written out (csrc/kmers/dx_kmer_codes.hip).  Unit j is what
 * it is for dx_code_kmers: symbols [d_beg[j], d_beg[j] + d_len[j]) of the packed read at d_in + d_boff[j], any byte offset, any phase;
 * units may overlap or repeat; pad bits and foreign symbols are part of no window, and nothing outside [0, in_bytes) is read.  A
 * window's code is its symbols as a base-4 number, the first on top, in the low 2 k bits of the word, zeros above; with canonical it
 * is min(code, rc(code)), compared unsigned.  Window p of unit j goes to d_codes[off[j] + p], off = the exclusive sums of
 * w_j = max(0, d_len[j] - k + 1), a unit that does not lie inside the in_bytes counting w_j = 0: the same array on every call.
 * *windows = sum w_j.  If that exceeds cap nothing is written and the call is DX_E_NOMEM, *windows still set.  DX_E_FORMAT with
 * *bad_unit = the smallest j that does not lie inside the in_bytes (UINT64_MAX otherwise; may be NULL): the good units' codes are
 * written all the same.  DX_E_ARG for k outside 1..32, a NULL pointer that is needed (d_codes may be NULL when cap == 0), n >= 2^31.   */
int dx_code_kmer_codes(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes,
                       const uint64_t *d_boff, const uint32_t *d_beg /* NULL: all 0 */, const uint32_t *d_len, uint64_t n,
                       uint32_t k /* 1..32 */, int canonical,
                       uint64_t *d_codes, uint64_t cap /* keys of room */, uint64_t *windows /* host */, uint64_t *bad_unit /* may be NULL */);

/* What a SORTED array of n codes holds (csrc/kmers/dx_kmer_runs.hip): a run is a maximal stretch of equal keys, its length the code's
 * count.  The meanings are dx_kmer_spectrum's and dx_kmer_list's, read off runs instead of cells: *distinct = the runs, *max_count the
 * longest, *max_code the smallest code that has it (both 0 for n == 0); spectrum[c] (host, nspec >= 2 values; may be NULL) = the runs
 * of length c, the last bin everything >= nspec - 1, spectrum[0] = 0; *found = the runs of min_count (>= 1) keys at least, listed or
 * not; d_out gets the first min(cap, *found) of them in ascending code order, nothing at cap or beyond; cap == 0 counts only.  Places
 * come from counts and a prefix sum, no atomic cursor; a run may be longer than any tile.  distinct, max_count, max_code may be NULL.
 * Two waits for the stream: the prefix sum's total, then one read-back of everything else.  DX_E_ARG for a NULL pointer that is
 * needed, min_count 0, nspec < 2 with a spectrum, n >= 2^36.                                                                      */
int dx_kmer_runs(dx_ctx *ctx, const uint64_t *d_sorted, uint64_t n, uint64_t min_count /* >= 1 */,
                 dx_kmer64 *d_out /* cap; may be NULL when cap == 0 */, uint64_t cap, uint64_t *found,
                 uint64_t *spectrum /* host, nspec; may be NULL */, uint32_t nspec,
                 uint64_t *distinct, uint64_t *max_count, uint64_t *max_code);

/* dx_file_kmers for 1 <= k <= 32, by another route: every window's code is written into ONE array on the device (dx_code_kmer_codes,
 * slice behind slice), the array is sorted (dx_sort_u64 with bits = 2 k) and the counts are read off the runs (dx_kmer_runs).  The
 * meaning of every argument and of *out is dx_file_kmers': the count is over what the archive HOLDS, a window never spans two records,
 * the list (malloc'd, dx_file_free) has min(found, max_list) entries in ascending code order when min_count >= 1 and list != NULL.
 * There is no table.  The codes and the sort's second array stand on the device together, 16 bytes a window: if dx_malloc cannot
 * give them the call is DX_E_NOMEM and dx_last_error names the bytes asked for.  DX_E_ARG (dx_last_error says why) for DX_KIND_QUIVA,
 * an unknown kind, canonical with arrow, k outside 1..32, nspec < 2 with a spectrum, a list without `listed`; else dx_file_unpack2's
 * errors for the image.  *out and the caller's spectrum are untouched on any error.                                               */
int dx_file_kmers_wide(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, uint32_t k /* 1..32 */, int canonical,
                       uint64_t min_count, uint64_t max_list, dx_kmers64 *out,
                       uint64_t *spectrum /* host, nspec; may be NULL */, uint32_t nspec,
                       dx_kmer64 **list /* may be NULL; malloc'd, dx_file_free */, uint64_t *listed);

/* How the windows of dx_code_kmer_codes spread over the top `bits` bits of their codes (csrc/kmers/dx_kmer_bins.hip): every window adds
 * one to d_bins[code >> (2 k - bits)], the canonical code's with canonical; d_bins: 2^bits 64-bit words on the device, ADDED to;
 * 1 <= bits <= min(2 k, 12).  Units, the bounds check, *windows (may be NULL) and *bad_unit are dx_code_kmer_codes': a unit that does
 * not lie inside the in_bytes adds nothing and is DX_E_FORMAT, the good units counted all the same.  DX_E_ARG for k outside 1..32,
 * bits out of range, a NULL pointer that is needed, n >= 2^31.  n == 0 changes nothing.                                              */
int dx_code_kmer_bins(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes,
                      const uint64_t *d_boff, const uint32_t *d_beg /* NULL: all 0 */, const uint32_t *d_len, uint64_t n,
                      uint32_t k /* 1..32 */, int canonical, uint32_t bits /* 1..min(2 k, 12) */,
                      uint64_t *d_bins /* 2^bits, added to */, uint64_t *windows /* host; may be NULL */, uint64_t *bad_unit /* may be NULL */);

/* dx_code_kmer_codes for a range of the codes (csrc/kmers/dx_kmer_codes_range.hip): only the windows with
 * bin_lo <= code >> (2 k - bits) < bin_hi are written, densely, in the order (unit, position) -- the same array on every call; the
 * places come from a counting launch and a prefix sum, no atomic cursor.  bits as for dx_code_kmer_bins, 0 <= bin_lo <= bin_hi <=
 * 2^bits (bins state the range so that k = 32 needs no 2^64).  *windows = the windows KEPT.  If that exceeds cap nothing is written
 * and the call is DX_E_NOMEM, *windows still set.  *bad_unit, DX_E_FORMAT and DX_E_ARG as for dx_code_kmer_codes, and DX_E_ARG for
 * bits or the bins out of range.                                                                                                     */
int dx_code_kmer_codes_range(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes,
                             const uint64_t *d_boff, const uint32_t *d_beg /* NULL: all 0 */, const uint32_t *d_len, uint64_t n,
                             uint32_t k /* 1..32 */, int canonical, uint32_t bits, uint32_t bin_lo, uint32_t bin_hi,
                             uint64_t *d_codes, uint64_t cap /* keys of room */, uint64_t *windows /* host */, uint64_t *bad_unit /* may be NULL */);

/* Host only (ctx may be NULL: it is where the error text goes).  bins[0 .. nbins) cut into ranges of consecutive bins: cut[0] = 0 <
 * ... < cut[*ranges] = nbins (cut has room for nbins + 1), range r = bins [cut[r], cut[r + 1]).  Greedy: a range takes bins while its
 * sum stays <= room; an empty bin costs nothing and never begins a range.  room == 0, or everything fitting, gives one range.  A
 * single bin above room is DX_E_NOMEM, and dx_last_error names the bin and its windows.  DX_E_ARG for a NULL pointer, nbins == 0.    */
int dx_kmer_range_plan(dx_ctx *ctx, const uint64_t *bins, uint32_t nbins, uint64_t room, uint32_t *cut /* nbins + 1 */, uint32_t *ranges);

/* dx_file_kmers_wide over SEVERAL images of one kind, counted into one answer, in passes over ranges of the codes when the windows do
 * not fit the device at once (csrc/dx_file_kmers_files.c).  room: the windows a pass may hold, 16 bytes of device memory each; 0: chosen
 * -- 0.8 x the free memory / 16 --; 2^36 - 1 at most.  All windows within room: ONE pass, whose launches are dx_file_kmers_wide's,
 * image after image.  Otherwise the windows are counted by the top min(2 k, 12) bits of their codes (dx_code_kmer_bins),
 * dx_kmer_range_plan cuts the bins into ranges, and every range, ascending, is written (dx_code_kmer_codes_range over all images),
 * sorted and read off its runs; a single bin above room is DX_E_NOMEM (dx_last_error names it).  The ranges' answers concatenate:
 * spectra and distinct add, the list takes the ranges' entries one behind the other up to max_list, max_code is the smallest code
 * with the largest count.  The images are uploaded once a pass.  The meaning of every argument that dx_file_kmers_wide has, and of
 * *out, is its own, summed over the images; per_file[i] (nimg of them; may be NULL): image i's records, symbols, windows and k, the
 * rest zero; *passes (may be NULL): the ranges that were sorted, 0 when there is no window.  nimg == 0 is the empty answer.  The
 * refusals are dx_file_kmers_wide's; an image that does not open is dx_file_unpack2's error, and dx_last_error names it ("image 1").
 * On any error *out, the caller's spectrum, per_file and *passes are untouched, *list is NULL and no device memory stays behind.    */
int dx_files_kmers_wide(dx_ctx *ctx, int kind, const uint8_t *const *imgs, const size_t *bytes, uint32_t nimg, uint32_t k /* 1..32 */,
                        int canonical, uint64_t min_count, uint64_t max_list, uint64_t room /* windows a pass; 0: chosen */,
                        dx_kmers64 *out, uint64_t *spectrum /* host, nspec; may be NULL */, uint32_t nspec,
                        dx_kmer64 **list /* may be NULL; malloc'd, dx_file_free */, uint64_t *listed,
                        dx_kmers64 *per_file /* nimg; may be NULL */, uint32_t *passes /* may be NULL */);

/* dx_kmer_code and dx_kmer_letters for 1 <= k <= 32.  Host only.  DX_E_ARG for k outside 1..32, a letter that is not the kind's (the
 * text's end among them), a code of more than 2 k bits (k < 32), a NULL pointer.                                                  */
int dx_kmer_code64(int arrow, const char *letters, uint32_t k, int canonical, uint64_t *code);
int dx_kmer_letters64(int arrow, uint64_t code, uint32_t k, char *out /* k + 1 */);

/* ------------------------------------------------------------------------------------------
 *  screen: which reads share k-mers with a given sequence set  (undexta -U, a k-mer index on one core, dexta again today)
 *          (csrc/screen/, csrc/dx_file_screen.c)
 * ------------------------------------------------------------------------------------------ */
/* A set of k-mers, 1 <= k <= 32, that stays on the device: its distinct codes in ascending order (compared unsigned) as 64-bit words
 * and a bucket index over the top p bits of the 2 k-bit code, first[0 .. 2^p] of 32-bit places.  p (index_bits) is the smallest value
 * with 2^p >= 2 codes, clamped to [1, min(2 k, 26)].  A set remembers k, canonical and arrow; it belongs to the context's device and
 * is freed with dx_kmer_set_free before the context is closed.                                                                    */
typedef struct dx_kmer_set dx_kmer_set;
typedef struct { uint64_t codes, device_bytes; uint32_t k, canonical, arrow, index_bits; } dx_set_info;   /* 32 bytes; (dx_kmer_set_info is the call, as dx_qv_onepass_info is dx_onepass_info's) */

/* The set of the n host codes, in any order, repeats allowed; n == 0 is the empty set.  With canonical every code is replaced by
 * min(code, rc(code)) first, so the letters of either strand may be given (dx_kmer_code64 makes a code of letters).  The codes are
 * uploaded, sorted (dx_sort_u64, bits = 2 k) and the distinct ones taken.  DX_E_ARG (dx_last_error says why) for k outside 1..32,
 * canonical with arrow, a code with bits above 2 k (k < 32; the index is named), a NULL pointer that is needed, a set of 2^32 - 1 or
 * more distinct codes (the count is named).  *set is NULL on any error.                                                          */
int dx_kmer_set_from_codes(dx_ctx *ctx, const uint64_t *codes, uint64_t n, uint32_t k, int canonical, int arrow, dx_kmer_set **set);

/* The set of the codes whose run in a SORTED device array of n keys (what dx_sort_u64 leaves) has min_count (>= 1) keys at least.
 * The array is only read; places come from counts and a prefix sum, the same array on every call.  The refusals are the above and
 * min_count 0, n >= 2^36.                                                                                                         */
int dx_kmer_set_from_sorted(dx_ctx *ctx, const uint64_t *d_sorted, uint64_t n, uint64_t min_count, uint32_t k, int canonical, int arrow,
                            dx_kmer_set **set);

/* The set of the distinct k-mers of a .dexta / .dexar image that are counted min_count (>= 1) times at least: dx_file_kmers_wide's
 * route up to the sorted array, then dx_kmer_set_from_sorted (arrow = the image's kind).  *out (may be NULL) is what
 * dx_file_kmers_wide reports for the image.  The refusals and errors are dx_file_kmers_wide's, and min_count 0.                   */
int dx_file_kmer_set(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, uint32_t k, int canonical, uint64_t min_count,
                     dx_kmer_set **set, dx_kmers64 *out /* may be NULL */);

/* The first key of every run of min_count (>= 1) keys at least of a SORTED device array of n keys, in the order of the keys:
 * *found = how many there are, d_out gets the first min(cap, *found) of them, nothing at cap or beyond; cap == 0 counts only.  What
 * dx_kmer_set_from_sorted makes its codes with.  The array is only read; places come from counts and a prefix sum, the same array on
 * every call.  DX_E_ARG for a NULL pointer that is needed (d_out may be NULL when cap == 0), min_count 0, n >= 2^36.                */
int dx_sorted_take(dx_ctx *ctx, const uint64_t *d_sorted, uint64_t n, uint64_t min_count /* >= 1 */,
                   uint64_t *d_out /* cap; may be NULL when cap == 0 */, uint64_t cap, uint64_t *found);

/* dx_file_kmer_set over SEVERAL images of one kind: dx_files_kmers_wide's passes; after each range's sort dx_sorted_take counts the
 * kept codes and writes them into a device array of exactly that size, and at the end the arrays are copied one behind the other on
 * the device -- the ranges ascend, so the result is sorted and distinct -- and handed to dx_kmer_set_from_sorted (min_count 1).
 * *out (may be NULL) is what dx_files_kmers_wide reports; room and *passes (may be NULL) are its own.  The refusals and errors are
 * dx_files_kmers_wide's, and min_count 0.  *set is NULL on any error, and no device memory stays behind.                             */
int dx_files_kmer_set(dx_ctx *ctx, int kind, const uint8_t *const *imgs, const size_t *bytes, uint32_t nimg, uint32_t k, int canonical,
                      uint64_t min_count, uint64_t room /* windows a pass; 0: chosen */, dx_kmer_set **set, dx_kmers64 *out /* may be NULL */,
                      uint32_t *passes /* may be NULL */);

int dx_kmer_set_info(const dx_kmer_set *set, dx_set_info *info);
/* the codes back, ascending: out (host) has room for cap of them; DX_E_NOMEM when that is fewer than the set holds */
int dx_kmer_set_codes(dx_ctx *ctx, const dx_kmer_set *set, uint64_t *out /* host */, uint64_t cap);
int dx_kmer_set_free(dx_ctx *ctx, dx_kmer_set *set /* may be NULL */);

/* Per unit: how many of its windows are in the set, and how much of it they cover.  16 bytes a unit.                              */
typedef struct { uint32_t hits, covered, first, last; } dx_screen;

/* Units are dx_code_kmer_codes' own: symbols [d_beg[j], d_beg[j] + d_len[j]) of the packed read at d_in + d_boff[j], any byte offset,
 * any phase; they may overlap or repeat; pad bits and foreign symbols are part of no window, and nothing outside [0, in_bytes) is
 * read.  A window's code is made as dx_code_kmer_codes makes it, with the set's k and canonical.  For unit j: hits = the windows
 * whose code is in the set; covered = the symbols of the unit that lie in one such window at least (the size of the union of the
 * [p, p + k)); first and last = the smallest and the largest such p, UINT32_MAX when there is none.  d_out (n entries, 4-byte aligned;
 * may be NULL) gets them; total[0 .. 4) (host) = the windows, the hits, the covered symbols and the units with a hit, over the good
 * units.  A unit that does not lie inside the in_bytes gets {0, 0, UINT32_MAX, UINT32_MAX} and adds nothing; the smallest such j
 * goes back in *bad_unit (UINT64_MAX otherwise; may be NULL) with DX_E_FORMAT, the others' entries and the totals are made all the
 * same.  One read-back a call; the same bytes on every call.  DX_E_ARG for a NULL set or another pointer that is needed, n >= 2^31.  */
int dx_code_kmer_screen(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes,
                        const uint64_t *d_boff, const uint32_t *d_beg /* NULL: all 0 */, const uint32_t *d_len, uint64_t n,
                        const dx_kmer_set *set,
                        dx_screen *d_out /* n entries; may be NULL */,
                        uint64_t total[4] /* host: windows, hits, covered, units with a hit */,
                        uint64_t *bad_unit /* may be NULL */);

typedef struct { uint64_t records, symbols, windows, hits, covered, records_hit; uint32_t k, reserved; } dx_screen_report;   /* 56 bytes */

/* The records of a .dexta / .dexar image (kind DX_KIND_FASTA or DX_KIND_ARROW; any key, legacy layout or byte order) screened against
 * the set, where they lie: the image is walked on the host and goes up whole or, when it does not fit the device or exceeds
 * DEXGPU_TEXT_BUDGET (bytes of image), in slices of whole records; the answer does not depend on the slicing.  *out = the sums;
 * *rec (may be NULL; malloc'd, dx_file_free) one dx_screen a record, *rec_len (may be NULL; malloc'd) every record's symbols.
 * DX_E_ARG (dx_last_error says why) for DX_KIND_QUIVA, an unknown kind, a set whose arrow is not the image's kind, a NULL pointer
 * that is needed; else dx_file_unpack2's errors for the image.  *out is untouched on any error.                                   */
int dx_file_screen(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, const dx_kmer_set *set, dx_screen_report *out,
                   dx_screen **rec /* may be NULL; malloc'd, dx_file_free; one a record */, uint32_t **rec_len /* may be NULL */);

#define DX_SCREEN_KEEP 0   /* ids = the records that match */
#define DX_SCREEN_DROP 1   /* ids = the others */
/* Host only, no GPU: the records that dx_file_screen's answer selects.  A record matches when hits >= max(min_hits, 1) and
 * covered * 1000 >= min_permille * len (64-bit products; a record of length 0 has no hit and never matches).  *ids (malloc'd,
 * dx_file_free; *n_ids of them, ascending) goes to dx_file_subset unchanged -- for the .dexta, the .dexar and the .dexqv of the same
 * records.  *n_ids == 0 is DX_OK here (dx_file_subset refuses it).  DX_E_ARG for min_permille > 1000, another mode, a NULL pointer.  */
int dx_screen_select(const dx_screen *rec, const uint32_t *rec_len, uint64_t records, uint32_t min_hits, uint32_t min_permille,
                     int mode, uint64_t **ids, uint64_t *n_ids);

/* ------------------------------------------------------------------------------------------
 *  depth: HOW OFTEN the k-mers of a read were seen -- counted sets, a depth profile, per-read quantiles
 *         (csrc/screen/dx_kmer_set.hip, csrc/screen/dx_screen_depth.hip, csrc/dx_file_depth.c)
 * ------------------------------------------------------------------------------------------ */
/* A COUNTED set keeps a 32-bit count beside every code, saturated at 2^32 - 1; dx_set_info.device_bytes includes the counts.
 * dx_code_kmer_screen and dx_code_kmer_spans take a counted set and ignore its counts; every set made by the calls above is
 * uncounted and behaves as before.  dx_kmer_set_counted: 1 or 0, DX_E_ARG for NULL.  dx_kmer_set_counts: the counts in the order
 * of dx_kmer_set_codes; DX_E_NOMEM when cap is fewer than the set holds, DX_E_ARG (dx_last_error says so) for an uncounted set.   */
int dx_kmer_set_counted(const dx_kmer_set *set);
int dx_kmer_set_counts(dx_ctx *ctx, const dx_kmer_set *set, uint32_t *out /* host */, uint64_t cap);

/* dx_kmer_set_from_sorted with every kept code's count = min(the length of its run, 2^32 - 1).  The codes are byte for byte
 * dx_kmer_set_from_sorted's of the same input; a run may be longer than any tile (dx_kmer_runs measures it); places come from
 * counts and a prefix sum, the same bytes on every call.  The refusals are dx_kmer_set_from_sorted's.                              */
int dx_kmer_set_from_sorted_counted(dx_ctx *ctx, const uint64_t *d_sorted, uint64_t n, uint64_t min_count, uint32_t k, int canonical,
                                    int arrow, dx_kmer_set **set);

/* The counted set of n host (code, count) pairs in any order -- the lists dx_file_kmers_wide and dx_files_kmers_wide hand out, or a
 * table from elsewhere.  With canonical every code is replaced by min(code, rc(code)) first; entries with equal codes ADD; a sum,
 * and a single count, saturates at 2^32 - 1; a pair with count 0 is dropped.  The pairs are sorted and added on the host, the two
 * arrays uploaded and indexed.  The refusals are dx_kmer_set_from_codes', the index named.                                          */
int dx_kmer_set_from_kmers(dx_ctx *ctx, const dx_kmer64 *list /* host */, uint64_t n, uint32_t k, int canonical, int arrow,
                           dx_kmer_set **set);

/* dx_file_kmer_set and dx_files_kmer_set with the runs' lengths kept beside the codes: the same arguments, the same route and passes
 * (in the multi-pass route a range's counts are gathered and concatenated as its codes are), the same refusals and errors.        */
int dx_file_kmer_set_counted(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, uint32_t k, int canonical, uint64_t min_count,
                             dx_kmer_set **set, dx_kmers64 *out /* may be NULL */);
int dx_files_kmer_set_counted(dx_ctx *ctx, int kind, const uint8_t *const *imgs, const size_t *bytes, uint32_t nimg, uint32_t k,
                              int canonical, uint64_t min_count, uint64_t room /* windows a pass; 0: chosen */, dx_kmer_set **set,
                              dx_kmers64 *out /* may be NULL */, uint32_t *passes /* may be NULL */);

/* The depth profile.  Units, windows, codes and bounds are dx_code_kmer_codes', with the set's k and canonical.  Window p of unit j
 * goes to d_depth[off[j] + p], off = the exclusive sums of w_j = max(0, d_len[j] - k + 1), a unit that does not lie inside the
 * in_bytes counting 0; d_off[0 .. n] (device, 8-byte aligned; may be NULL) gets off, d_off[n] = the windows.  The value is
 * min(count of the window's code, 65535), 0 for a code that is not in the set; an uncounted set counts 1 for every code it holds.
 * *windows = sum w_j.  If that exceeds cap nothing is written (d_off neither) and the call is DX_E_NOMEM, *windows still set.
 * DX_E_FORMAT, *bad_unit and DX_E_ARG are dx_code_kmer_codes' (the good units' depths are written all the same), and DX_E_ARG for a
 * NULL set.  The same bytes on every call; nothing behind d_depth[*windows] is touched.  n == 0 writes d_off[0] = 0 alone.          */
int dx_code_kmer_depths(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes,
                        const uint64_t *d_boff, const uint32_t *d_beg /* NULL: all 0 */, const uint32_t *d_len, uint64_t n,
                        const dx_kmer_set *set,
                        uint16_t *d_depth, uint64_t cap /* words of room */,
                        uint64_t *d_off /* n + 1, device; may be NULL */,
                        uint64_t *windows /* host */, uint64_t *bad_unit /* may be NULL */);

typedef struct { uint32_t windows, hits; uint64_t sum; uint16_t min, q1, median, q3, max, reserved[3]; } dx_depth;   /* 32 bytes */

/* Per unit j the statistics of v = d_depth[d_off[j] .. d_off[j + 1]), w values: windows = w; hits = the values that are not 0; sum =
 * their 64-bit sum (of the clamped values, as stored); min and max over all w; with s = v sorted ascending q1 = s[(w - 1) / 4],
 * median = s[2 (w - 1) / 4], q3 = s[3 (w - 1) / 4] (integer divisions, 64-bit products: values that occur; exact); w == 0 gives all
 * zeros; reserved is 0.  d_out (n entries, 4-byte aligned; may be NULL) gets them; total[0 .. 4) (host) = the windows, the hits, the
 * sum and the units with a hit.  DX_E_FORMAT if d_off decreases (or a unit has 2^32 values or more), the smallest index in
 * dx_last_error: that unit gets zeros, the others and the totals are made all the same.  DX_E_ARG for a NULL pointer that is needed
 * (d_depth, d_off, total), an array that is not aligned, n >= 2^31.  n == 0 launches nothing.                                         */
int dx_depth_stats(dx_ctx *ctx, const uint16_t *d_depth, const uint64_t *d_off /* n + 1 */, uint64_t n,
                   dx_depth *d_out /* n; may be NULL */, uint64_t total[4] /* host: windows, hits, sum, units with a hit */);

typedef struct { uint64_t records, symbols, windows, hits, sum, records_hit; uint32_t k, reserved; } dx_depth_report;   /* 56 bytes */

/* The records of a .dexta / .dexar image against a (counted) set, where they lie: walked and sliced as dx_file_screen does it, 32
 * bytes of entries a record; per slice a device profile of exactly the slice's windows (known from the lengths; the slices are
 * narrowed so that a slice and its profile fit together, and DX_E_NOMEM names the bytes if one record's do not), dx_code_kmer_depths,
 * dx_depth_stats, and the entries brought down.  *rec (may be NULL; malloc'd, dx_file_free) one dx_depth a record, *rec_len (may
 * be NULL; malloc'd) every record's symbols; *profile (may be NULL; malloc'd) the whole profile, brought down only when it is asked
 * for, and *rec_off (may be NULL; malloc'd) every record's place in it, records + 1 words, the last the windows.  A record lies in
 * one slice: the answer does not depend on the slicing.  The refusals are dx_file_screen's.  *out is untouched on any error.        */
int dx_file_depth(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, const dx_kmer_set *set, dx_depth_report *out,
                  dx_depth **rec /* may be NULL */, uint32_t **rec_len /* may be NULL */,
                  uint16_t **profile /* may be NULL */, uint64_t **rec_off /* may be NULL; records + 1 */);

#define DX_DEPTH_MIN    0
#define DX_DEPTH_Q1     1
#define DX_DEPTH_MEDIAN 2
#define DX_DEPTH_Q3     3
#define DX_DEPTH_MAX    4
/* Host only, no GPU: the records that dx_file_depth's answer selects.  A record matches when windows >= max(min_windows, 1) and
 * lo <= stat <= hi, stat one of DX_DEPTH_*; mode DX_SCREEN_KEEP: the records that match, DX_SCREEN_DROP: the others.  *ids (malloc'd,
 * dx_file_free; *n_ids of them, ascending) goes to dx_file_subset unchanged -- for the .dexta, the .dexar and the .dexqv of the same
 * records.  *n_ids == 0 is DX_OK.  DX_E_ARG for an unknown stat or mode, lo > hi, a NULL pointer that is needed.                     */
int dx_depth_select(const dx_depth *rec, uint64_t records, int stat, uint32_t lo, uint32_t hi, uint32_t min_windows, int mode,
                    uint64_t **ids, uint64_t *n_ids);

/* ------------------------------------------------------------------------------------------
 *  screen spans: WHERE a read matches the set, and the archive cut there  (csrc/screen/dx_screen_spans.hip, csrc/dx_file_screen_spans.c)
 * ------------------------------------------------------------------------------------------ */
typedef struct { uint64_t record; uint32_t beg, end; } dx_span;     /* 16 bytes: symbols [beg, end) of unit / record `record` */

/* Units, windows and codes are dx_code_kmer_screen's: any byte offset and phase, d_beg in front of the unit, pad bits and foreign
 * symbols part of no window, nothing outside [0, in_bytes) read, the set's k and canonical.  The SPANS of unit j are the maximal runs
 * of symbols that lie in at least one window whose code is in the set -- the union of the [p, p + k) that dx_screen.covered counts,
 * written out as intervals.  So every span has k symbols at least, two spans of a unit are one symbol apart at least, the lengths
 * sum to dx_screen.covered, the first beg is dx_screen.first and the last end dx_screen.last + k.
 * The list is in the order (unit, beg), the same bytes on every call (places come from counts and a prefix sum, no atomic cursor):
 * d_spans (8-byte aligned) gets the first min(cap, spans) of them, each one complete, nothing at cap or beyond; cap == 0 counts only.
 * d_count[j] (may be NULL) = unit j's spans, all of them (at most len / (k + 1) + 1: it does not saturate).  total[0 .. 3) (host) =
 * the spans, listed or not, the covered symbols and the units with a span, over the good units.  A unit that does not lie inside
 * the in_bytes has no spans, count 0, adds nothing; the smallest such j goes back in *bad_unit (UINT64_MAX otherwise; may be NULL)
 * with DX_E_FORMAT, the other units' spans are made all the same.  One read-back a call, and with a list the prefix sum's besides.
 * DX_E_ARG for a NULL set or another pointer that is needed, n >= 2^31, cap >= 2^32, a list or counts that are not aligned.        */
int dx_code_kmer_spans(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes,
                       const uint64_t *d_boff, const uint32_t *d_beg /* NULL: all 0 */, const uint32_t *d_len, uint64_t n,
                       const dx_kmer_set *set,
                       uint32_t *d_count /* n; may be NULL: every unit's spans */,
                       dx_span *d_spans /* cap entries; may be NULL when cap == 0 */, uint64_t cap,
                       uint64_t total[3] /* host: spans, covered symbols, units with a span */,
                       uint64_t *bad_unit /* may be NULL */);

/* A list as dx_code_kmer_spans leaves it -- beg < end for every entry, the records not decreasing, end[i] <= beg[i + 1] within a
 * record -- joined and filtered on the device: (1) consecutive spans of one record are joined while beg[i + 1] - end[i] <= max_gap,
 * a joined span running from the first one's beg to the last one's end; (2) a joined span is kept if end - beg >= min_span.  The
 * join comes first and the filter does not influence it; max_gap UINT32_MAX leaves one span a record.  d_out (8-byte aligned, not
 * overlapping d_in) gets the first min(cap, kept) in the input's order, the same bytes on every call, nothing at cap or beyond;
 * cap == 0 counts only.  total[0 .. 2) (host) = the spans kept, listed or not, and their symbols.  A joined span may take in any
 * number of entries.  DX_E_FORMAT with *bad (may be NULL; UINT64_MAX otherwise) = the smallest index that breaks the input's
 * order; the totals are 0 then and what d_out holds means nothing.  n == 0 launches nothing.  DX_E_ARG for a NULL pointer that is
 * needed, a list that is not aligned, d_out overlapping d_in, cap >= 2^32, n >= 2^36.                                              */
int dx_spans_join(dx_ctx *ctx, const dx_span *d_in, uint64_t n, uint32_t max_gap, uint32_t min_span,
                  dx_span *d_out /* cap entries; not overlapping d_in */, uint64_t cap,
                  uint64_t total[2] /* host: spans kept, their symbols */, uint64_t *bad /* may be NULL */);

typedef struct { uint64_t records, symbols, covered, records_hit, raw_spans, spans, span_symbols, listed; uint32_t k, reserved; } dx_spans_report;   /* 72 bytes */

/* The records of a .dexta / .dexar image screened against the set as dx_file_screen screens them (the same walk, the same slices, the
 * same refusals), and per slice the raw spans counted, listed into a device list of exactly that size (DX_E_NOMEM, dx_last_error
 * naming the bytes, if it cannot be had), joined and filtered (dx_spans_join: max_gap, min_span); only the joined, kept spans come
 * down.  *spans (may be NULL; malloc'd, dx_file_free) has out->listed = min(out->spans, max_spans) of them in the order (record,
 * beg), `record` being the image's record number; *rec_spans (may be NULL; malloc'd) = the kept spans of every record, listed or
 * not; *rec_len (may be NULL; malloc'd) = every record's symbols.  out->covered, records_hit (dx_file_screen's) and raw_spans
 * describe the raw spans, out->spans and span_symbols what the join and the filter keep.  A record lies in one slice: the answer
 * does not depend on the slicing.  *out is untouched on any error.                                                               */
int dx_file_screen_spans(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, const dx_kmer_set *set,
                         uint32_t max_gap, uint32_t min_span, uint64_t max_spans, dx_spans_report *out,
                         dx_span **spans /* may be NULL; malloc'd, dx_file_free */,
                         uint32_t **rec_spans /* may be NULL: kept spans a record */, uint32_t **rec_len /* may be NULL */);

/* Host only, no GPU: dx_hits_cut_plan's plan over spans given directly -- symbols [beg, end) of record `record`, in any order; the
 * modes, min_len, the union of spans that overlap or touch, the outputs and *report are dx_hits_cut_plan's.  DX_E_ARG for a span with
 * beg > end, end > its record's length, record >= records, an unknown mode, a NULL pointer that is needed.                        */
int dx_spans_cut_plan(const dx_span *spans, uint64_t n, const uint32_t *rec_len, uint64_t records, uint32_t min_len, int mode,
                      uint64_t **ids, uint32_t **beg, uint32_t **end, uint64_t *n_ids, dx_cut *report /* may be NULL */);

/* A .dexta / .dexar image with what matches the set cut out of its records: dx_file_screen_spans with every span listed,
 * dx_spans_cut_plan, dx_file_subset.  Outputs, the selection handed back for the .dexar and the .dexqv of the same records, the
 * modes and DX_E_DEGENERATE for a selection without a unit are dx_file_cut's; it never cuts from part of the spans (DX_E_NOMEM).
 * DX_E_ARG for DX_KIND_QUIVA (cut its .dexta, then apply the selection), an unknown mode, and what dx_file_screen refuses.         */
int dx_file_screen_cut(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, const dx_kmer_set *set,
                       uint32_t max_gap, uint32_t min_span, uint32_t min_len, int mode,
                       uint8_t **out, size_t *out_len, dx_cut *report /* may be NULL */,
                       uint64_t **ids /* may be NULL */, uint32_t **beg /* may be NULL */, uint32_t **end /* may be NULL */, uint64_t *n_ids /* may be NULL */);

/* ------------------------------------------------------------------------------------------
 *  place: WHERE ON A REFERENCE each read lies, and on which strand -- an index that keeps positions, seeds, a vote over diagonals
 *         (csrc/place/, csrc/dx_file_place.c).  Seed-and-vote placement, not alignment: no chaining, no base-level alignment, no CIGAR.
 * ------------------------------------------------------------------------------------------ */
/* The reference is T targets of l_t symbols one behind the other: toff[0 .. T] = the exclusive sums of the lengths, G = toff[T] < 2^31.
 * The window at global position g = toff[t] + p exists for 0 <= p <= l_t - k; a window never spans two targets.  Its code is
 * dx_code_kmer_codes'; with canonical the code kept is min(fwd, rc) and flip = (rc < fwd), without canonical and for a k-mer that is
 * its own reverse complement flip = 0.  A dx_kmer_index (opaque, on the device, the context's; freed with dx_kmer_index_free before
 * the context is closed) holds a COUNTED dx_kmer_set of those windows -- codes ascending, count[i] = the occurrences --, start[0 .. n]
 * (32-bit) = the exclusive sums of the counts, and pos[start[i] .. start[i + 1]) = the occurrences of code i as g << 1 | flip,
 * ascending in g.  An index over 2^31 symbols or more is not built.                                                                 */
typedef struct dx_kmer_index dx_kmer_index;
typedef struct { uint64_t codes, windows, targets, symbols, device_bytes; uint32_t k, canonical, arrow, reserved; } dx_index_info;   /* 56 bytes */

/* The targets are the units of a packed buffer, which are dx_code_kmer_codes' own (any byte offset and phase, d_beg in front).  The
 * counted set is made by dx_code_kmer_codes, dx_sort_u64 and dx_kmer_set_from_sorted_counted (min_count 1); one kernel then writes a
 * key place << 32 | g << 1 | flip a window, dx_sort_u64 orders them and the low words are kept: the same bytes on every call.  While
 * it is built the index takes 16 bytes a window beside itself.  DX_E_ARG (dx_last_error says why) for k outside 1..32, canonical with
 * arrow, n >= 2^31, a NULL pointer that is needed, G >= 2^31 (the size and the target are named); DX_E_FORMAT for a target that does
 * not lie inside the in_bytes.  *index is NULL on any error, and no device memory stays behind.                                      */
int dx_code_kmer_index(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes,
                       const uint64_t *d_boff, const uint32_t *d_beg /* NULL: all 0 */, const uint32_t *d_len, uint64_t n,
                       uint32_t k /* 1..32 */, int canonical, int arrow, dx_kmer_index **index);

/* The records of a .dexta / .dexar image are the targets (arrow = the image's kind): a read set, or an assembly written in the
 * archive's header form, serves as the reference.  The image goes up whole.  The refusals are dx_file_kmer_set's and the above.     */
int dx_file_kmer_index(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, uint32_t k, int canonical, dx_kmer_index **index);

/* A plain reference: T sequences of lens[t] letters (acgtACGT, or 1234 with arrow; no terminator is looked for).  They are packed
 * on the host, four symbols a byte with the first on top, every target at a byte of its own, and go through dx_code_kmer_index.
 * DX_E_ARG for a letter that is not the kind's: dx_last_error names the target and the position.                                    */
int dx_kmer_index_from_letters(dx_ctx *ctx, int arrow, const char *const *seqs, const uint32_t *lens, uint64_t T, uint32_t k, int canonical,
                               dx_kmer_index **index);
/* Host only, its packer: len letters into (len + 3) / 4 bytes at out, four symbols a byte, the first on top, the last byte's pad bits
 * zero.  DX_E_ARG for a letter that is not the kind's, *bad_pos (may be NULL) = its position; out is then written up to there.        */
int dx_pack_letters(int arrow, const char *seq, uint32_t len, uint8_t *out, uint32_t *bad_pos /* may be NULL */);

int dx_kmer_index_info(const dx_kmer_index *index, dx_index_info *info);
/* the counted set inside, the index's own (not to be freed): dx_code_kmer_screen, _spans and _depths and their file drivers take it  */
const dx_kmer_set *dx_kmer_index_set(const dx_kmer_index *index);
/* toff[0 .. *targets] (host, the index's own: valid until dx_kmer_index_free); *targets may be NULL                                 */
const uint64_t *dx_kmer_index_targets(const dx_kmer_index *index, uint64_t *targets);
/* start (codes + 1 words) and pos (windows words) back to the host; either may be NULL with its cap 0; DX_E_NOMEM when a cap is
 * fewer than the index holds                                                                                                         */
int dx_kmer_index_positions(dx_ctx *ctx, const dx_kmer_index *index, uint32_t *start /* host */, uint64_t start_cap,
                            uint32_t *pos /* host */, uint64_t pos_cap);
int dx_kmer_index_free(dx_ctx *ctx, dx_kmer_index *index /* may be NULL */);

typedef struct { uint32_t unit, pos, gpos, strand; } dx_seed;       /* 16 bytes */

/* The SEEDS of unit j.  Units are dx_code_kmer_codes' own: any byte offset and phase, d_beg in front of the unit, pad bits and
 * foreign symbols part of no window, nothing outside [0, in_bytes) read.  The windows are taken with p ascending; a window's code is
 * made with the index's k and canonical, f being its own flip.  If the index holds the code at place i and count[i] <= max_occ
 * (>= 1), every r in [start[i], start[i + 1]), ascending, gives the seed {j, p, pos[r] >> 1, (pos[r] & 1) ^ f}; a code above max_occ
 * gives none.  The list is in the order (unit, pos, gpos), the same bytes on every call: a counting launch, a prefix sum, a listing
 * launch, no atomic cursor.  d_count[j] (may be NULL) = unit j's seeds; d_off[0 .. n] (device, 8-byte aligned; may be NULL) = their
 * exclusive sums, unit j's seeds standing in d_seeds[d_off[j] .. d_off[j + 1]).  cap == 0 counts only; cap below the seeds is
 * DX_E_NOMEM with nothing written (d_off neither), total still set.  total[0 .. 4) (host) = the windows, the windows with a seed, the
 * seeds and the units with a seed, over the good units.  A unit of 2^32 seeds or more is DX_E_NOMEM, dx_last_error naming the
 * smallest.  A unit that does not lie inside the in_bytes has no seed; the smallest such j goes back in *bad_unit (UINT64_MAX
 * otherwise; may be NULL) with DX_E_FORMAT, the others' seeds are made all the same.  DX_E_ARG for a NULL index or another pointer
 * that is needed, max_occ 0, n >= 2^31, an array that is not aligned.  n == 0 writes d_off[0] = 0 alone.                            */
int dx_code_kmer_seeds(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes,
                       const uint64_t *d_boff, const uint32_t *d_beg /* NULL: all 0 */, const uint32_t *d_len, uint64_t n,
                       const dx_kmer_index *index, uint32_t max_occ /* >= 1 */,
                       uint32_t *d_count /* n; may be NULL */, uint64_t *d_off /* n + 1, device; may be NULL */,
                       dx_seed *d_seeds /* cap entries; may be NULL when cap == 0 */, uint64_t cap,
                       uint64_t total[4] /* host: windows, windows with a seed, seeds, units with a seed */, uint64_t *bad_unit /* may be NULL */);

typedef struct { uint32_t seeds, votes, strand, diag, rbeg, rend, gbeg, gend; } dx_place;   /* 32 bytes */

/* The placement of unit j from its seeds d_seeds[d_off[j] .. d_off[j + 1]).  A seed's diagonal is 32 bits: gpos - pos + 2^31 for
 * strand 0, gpos + pos for strand 1 (both modulo 2^32); its bin = diag >> band_bits, 0 <= band_bits <= 31.  With c(s, b) = the unit's
 * seeds of strand s in bin b, the best (s, b), among those with c(s, b) > 0, has the largest c(s, b) + c(s, b + 1), a bin beyond the
 * last counting 0; on a tie the smaller s wins, then the smaller b.  The voted seeds are those of strand s in bin b or b + 1.
 * d_out[j] = {seeds: all the unit's; votes: the best sum; strand: s; diag: b << band_bits; rbeg / rend: min pos and max pos + k
 * over the voted seeds, read coordinates as stored; gbeg / gend: min gpos and max gpos + k over them, global}; a unit without a seed
 * gets {0, 0, 0, UINT32_MAX x 5}.  The positions are global: a band that runs from one target's end into the next target's start
 * counts the seeds of both -- per-target bands are not built.  total[0 .. 3) (host) = the seeds, the votes and the units placed.
 * The keys (8 bytes a seed) and the sort's second array (8 more) are made and freed here.  DX_E_FORMAT if d_off decreases or a
 * seed's `unit` is not its stretch's: the smallest index goes into dx_last_error, and what d_out holds means nothing.  DX_E_ARG for
 * k outside 1..32, band_bits > 31, a NULL pointer that is needed, an array that is not aligned, n >= 2^31, 2^36 seeds or more.
 * n == 0 launches nothing.                                                                                                           */
int dx_seeds_place(dx_ctx *ctx, const dx_seed *d_seeds, const uint64_t *d_off /* n + 1 */, uint64_t n, uint32_t k, uint32_t band_bits,
                   dx_place *d_out /* n */, uint64_t total[3] /* host: seeds, votes, units placed */);

typedef struct { uint64_t records, symbols, windows, hits, seeds, votes, records_placed, groups, reserved; uint32_t k, band_bits; } dx_place_report;   /* 80 bytes */

/* The records of a .dexta / .dexar image placed on the index's reference, where they lie: walked and sliced as dx_file_screen_spans
 * does it.  Per slice the seeds are counted and the per-record counts brought down; consecutive records are grouped greedily so that
 * a group's seeds stay at or below seed_room (0: 0.8 x the free memory / 32 bytes); every group is listed (dx_code_kmer_seeds' list
 * from the counts that are there), placed (dx_seeds_place), and 32 bytes a record come down.  A single record above the room is
 * DX_E_NOMEM, dx_last_error naming it.  A record lies in one slice and one group: the answer depends neither on the slicing nor on
 * the room.  *rec (may be NULL; malloc'd, dx_file_free) one dx_place a record, *rec_len (may be NULL; malloc'd) every record's
 * symbols; out->hits = the windows with a seed, out->groups = the groups that were listed.  The refusals are dx_file_screen's:
 * DX_KIND_QUIVA, an unknown kind, an index whose arrow is not the image's kind, a NULL pointer that is needed; and max_occ 0,
 * band_bits > 31.  *out is untouched on any error, and no device memory stays behind.                                               */
int dx_file_place(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, const dx_kmer_index *index, uint32_t max_occ, uint32_t band_bits,
                  uint64_t seed_room /* seeds a group; 0: chosen */, dx_place_report *out,
                  dx_place **rec /* may be NULL; malloc'd, dx_file_free; one a record */, uint32_t **rec_len /* may be NULL */);

/* Host only, no GPU: the records of dx_file_place's answer that lie on a locus.  A record's target t is the one that holds gbeg
 * (toff[t] <= gbeg < toff[t + 1]; toff: T + 1 words, dx_kmer_index_targets').  The record matches when votes >= max(min_votes, 1), its
 * strand is allowed (strands: 1 = strand 0, 2 = strand 1, 3 = both), target == UINT32_MAX or t == target, and
 * [gbeg - toff[t], min(gend, toff[t + 1]) - toff[t]) meets [lo, hi).  mode DX_SCREEN_KEEP: the records that match, DX_SCREEN_DROP:
 * the others.  *ids (malloc'd, dx_file_free; *n_ids of them, ascending) goes to dx_file_subset unchanged -- for the .dexta, the
 * .dexar and the .dexqv of the same records.  *n_ids == 0 is DX_OK.  DX_E_ARG for strands outside 1..3, another mode, lo > hi, a
 * target that is neither UINT32_MAX nor below T, a toff that decreases or does not begin at 0, a NULL pointer that is needed.         */
int dx_place_select(const dx_place *rec, uint64_t records, const uint64_t *toff, uint64_t T, uint32_t target /* UINT32_MAX: any */,
                    uint32_t lo, uint32_t hi, uint32_t min_votes, int strands /* 1, 2 or 3 */, int mode, uint64_t **ids, uint64_t *n_ids);

/* ------------------------------------------------------------------------------------------
 *  in-memory entry API: QVcoding_Scan1 / Compress_Next_QVentry1 (QV.c:866-920, 1343-1379) as a batch
 * ------------------------------------------------------------------------------------------ */
/* dex2DB.c:511-643 feeds entries one at a time through the *1 functions and writes the compressed
 * bytes of each to a .qvs file, remembering its offset (DAZZ_READ.coff).  Here the entries are
 * gathered first (dx_entries_add has the *1 functions' argument list), then scanned and compressed
 * together on the GPU: *records = the bare record stream (no framing bytes), coff[i] = offset of
 * entry i in it (n+1 values), *coding = the tables to write with dx_qv_write_coding.  records / coff
 * are malloc'd (dx_file_free).  The streams are copied; the caller's buffers are not modified
 * (the reference mutates them in place).                                                        */
typedef struct dx_entries dx_entries;
dx_entries *dx_entries_new(void);
void        dx_entries_free(dx_entries *e);
int         dx_entries_add(dx_entries *e, int rlen, const char *del, const char *tag, const char *ins,
                           const char *mrg, const char *sub);
int         dx_entries_compress(dx_ctx *ctx, const dx_entries *e, int lossy, dx_qv_coding *coding,
                                uint8_t **records, size_t *nbytes, uint64_t **coff);

/* The read side: Load_QVentry (DB.c:2575-2621) seeks to reads[i].coff and calls Uncompress_Next_QVentry(..., rlen)
 * (QV.c:1428-1481) for any i, in any order.  A .qvs record has no framing bytes and the format stores no segment sizes, but with
 * every record's start and length known the records are independent: one record is one unit of work.
 *
 * dx_qv_walk_records (host, no GPU) / dx_qv_walk_records_device: record i's deletion segment starts at buf + start[i] and every
 * line of it has rlen[i] symbols; seg[5i ..] receives the byte sizes of its del, tag, ins, mrg and sub segments (code lengths
 * only are decoded; each segment ends by the pad rule, QV.c:436-442).  Starts may come in any order, may repeat and need not
 * tile the buffer; rlen 0 gives five zeros.  DX_E_FORMAT with *bad_entry = the first such i (UINT64_MAX otherwise; may be NULL)
 * when a segment does not end inside [0, nbytes).  flip: the code words were written byte-swapped (DX_DECODE_FLIP).
 * The device form (csrc/records/dx_qv_records.hip) walks a record a lane and never reads outside [0, nbytes); d_start (as
 * d_rec_off), d_seg and d_len are what dx_qv_decode takes with d_hdr_off = NULL.  Entries of more than 4 M symbols are walked by
 * the host function on a copy of their bytes.                                                                            */
int dx_qv_walk_records(const uint8_t *buf, size_t nbytes, const uint64_t *start, const uint32_t *rlen, uint64_t n,
                       const dx_qv_coding *cd, int flip, uint32_t *seg /* n x 5 */, uint64_t *bad_entry);
int dx_qv_walk_records_device(dx_ctx *ctx, const uint8_t *d_buf, uint64_t nbytes, const uint64_t *d_start,
                              const uint32_t *d_len, uint64_t n, const dx_qv_coding *cd, int flip,
                              uint32_t *d_seg, uint64_t *bad_entry);

/* Load_QVentry for a selection of entries at once: entry ids[j] (ids == NULL: entries 0 .. n_ids - 1) starts at records +
 * coff[ids[j]] and has rlen[ids[j]] symbols a line; its five lines, each followed by '\n' (dx_qv_decode's layout), stand at
 * *text + toff[j], toff[n_ids] = *text_bytes (both malloc'd: dx_file_free).  ids may come in any order and may repeat.
 * ascii as Load_QVentry's (DB.c:2602-2618): 1 the tag line in lower case, 2 in upper case, 0 as numbers 0..3 (Number_Read).
 * coding / flip: what dx_qv_read_coding gave for the track.  ONE coding per call: a .qvs made of several files has one coding
 * per file (DB.c:2485-2508), and the caller groups its reads by coding.
 * Only the selected records' bytes travel: when they make up less than half of the stream they are uploaded packed side by
 * side, else the whole stream goes up once (a stream the device has no room for goes up packed, slice by slice, whatever
 * is selected).  A selection whose text exceeds DEXGPU_TEXT_BUDGET bytes, or what is free on the device, is decoded in slices
 * of whole entries.  n_ids == 0: DX_OK and an empty text.  DX_E_FORMAT: an entry does not lie inside the stream
 * (dx_last_error names it).                                                                                              */
int dx_entries_uncompress(dx_ctx *ctx, const dx_qv_coding *coding, int flip,
                          const uint8_t *records, size_t nbytes, const uint64_t *coff, const uint32_t *rlen,
                          const uint64_t *ids, uint64_t n_ids,
                          int ascii, uint8_t **text, size_t *text_bytes, uint64_t **toff /* n_ids + 1 */);

/* ------------------------------------------------------------------------------------------
 *  .bps / .arw read side: Load_Read, Load_Subread, Load_All_Reads, Load_Arrow as a batch
 * ------------------------------------------------------------------------------------------ */
/* A .bps / .arw payload is dx_pack2_encode's output with d_hdr = NULL: Compress_Read's bytes (DB.c:319-338) of every read, one
 * behind the other, found through DAZZ_READ.boff and .rlen.  Load_Read (DB.c:1232-1298) reads COMPRESSED_LEN(rlen) bytes at
 * boff, Load_Subread (DB.c:1308-1381) bytes [beg / 4, (end - 1) / 4 + 1) of them -- the string it returns begins beg % 4
 * symbols into what it uncompressed (DB.c:1351-1367) --, Load_Arrow (DB.c:1508-1548) does the same on the .arw track; all
 * leave a delimiter on both sides of the string, Load_All_Reads (DB.c:1389-1441) one between any two reads.
 *
 * dx_reads_unpack (device in, device out; csrc/reads/dx_reads.hip): unit j is symbols [d_beg[j], d_beg[j] + d_len[j]) of the
 * packed read that starts at d_in + d_boff[j] -- any byte offset, any phase; symbol i of a read is bits 7 - 2 (i & 3),
 * 6 - 2 (i & 3) of its byte i >> 2; d_beg == NULL: all 0.  It writes d_len[j] bytes at d_out + d_out_off[j] (any alignment)
 * and ONE delimiter byte behind them, nothing else: 4 for DX_LETTERS_NUMBERS (Uncompress_Read, DB.c:362), '\0' for the
 * letter sets (Lower_Read & co., DB.c:367-389); d_len[j] == 0 writes the delimiter only.  Units may overlap or repeat in the
 * input; the outputs are the caller's to keep disjoint.  Nothing outside [0, in_bytes) is read.  DX_E_FORMAT with *bad_unit =
 * the smallest such j (UINT64_MAX otherwise; may be NULL) when a unit's last packed byte d_boff[j] + ((d_beg[j] + d_len[j] - 1)
 * >> 2) is not below in_bytes (d_len[j] > 0), when d_boff[j] > in_bytes, or when d_len[j] > 2^31 - 1 (DAZZ_READ.rlen is an int);
 * nothing is promised about d_out then.  The check is the kernel's own: one read-back of the verdict a call.            */
int dx_reads_unpack(dx_ctx *ctx, int letters, const uint8_t *d_in, uint64_t in_bytes,
                    const uint64_t *d_boff, const uint32_t *d_beg /* NULL: all 0 */, const uint32_t *d_len,
                    uint64_t n, uint8_t *d_out, const uint64_t *d_out_off, uint64_t *bad_unit /* may be NULL */);

/* Load_Read / Load_Subread / Load_Arrow for a selection at once (host in, host out): unit j is read ids[j] (ids == NULL: reads
 * 0 .. n_ids - 1), which starts at payload + boff[ids[j]] and has rlen[ids[j]] symbols -- all of it when beg == NULL, else its
 * symbols [beg[j], end[j]) (beg and end are given together; beg[j] <= end[j] <= rlen[ids[j]], else DX_E_ARG).  ids may come in
 * any order and may repeat.  The layout is Load_All_Reads' (DB.c:1406-1433): (*text)[0] is a delimiter, toff[0] = 1,
 * toff[j + 1] = toff[j] + len_j + 1, *text_bytes = toff[n_ids]; unit j is (*text)[toff[j] .. toff[j] + len_j), with a
 * delimiter in front of it and behind it -- Load_Read's "the byte before read will be set to a delimiter".  The one difference
 * from Load_All_Reads: its first byte is 4 whatever ascii is (DB.c:1406); here it is the letter set's delimiter, as Load_Read
 * leaves it.  text and toff are malloc'd (dx_file_free).
 * What travels, as for dx_entries_uncompress: a unit's span of the payload is exact, [boff + beg / 4, boff + (end - 1) / 4 + 1);
 * the spans are merged, and when they cover less than half of the payload they go up packed side by side, else the payload
 * goes up once (one the device has no room for goes up packed, slice by slice, whatever is selected).  A selection whose
 * text exceeds DEXGPU_TEXT_BUDGET bytes, or what is free on the device, is decoded in slices of whole units.  n_ids == 0:
 * DX_OK, and the text is one delimiter byte.  DX_E_FORMAT: a read does not lie inside [0, nbytes) (dx_last_error names the
 * caller's read id).                                                                                                    */
int dx_reads_uncompress(dx_ctx *ctx, int letters, const uint8_t *payload, size_t nbytes,
                        const uint64_t *boff, const uint32_t *rlen,
                        const uint64_t *ids, const uint32_t *beg, const uint32_t *end, uint64_t n_ids,
                        uint8_t **text, size_t *text_bytes, uint64_t **toff /* n_ids + 1 */);

/* ------------------------------------------------------------------------------------------
 *  seeded synthetic corpora on the device (benchmark/test plumbing; mirrors dextractor_amd/synth.py)
 * ------------------------------------------------------------------------------------------ */
/* Writes entries [entry0, entry0+n) of the .quiva corpus `seed`: for each entry the header line
 * "@<movie>/WWWWWWWW/BBBBBBB_EEEEEEE RQ=0.QQQ\n" (fixed width, from d_hdr4 = well,beg,end,qv)
 * ending right before d_off[i], then the five lines.  d_lut = 5 x 4096 symbol tables (del, tag,
 * ins, mrg, sub); del_run = value under which the tag is 'N' (-1 never).                        */
int dx_synth_quiva(dx_ctx *ctx, uint32_t seed, uint64_t entry0, uint64_t n,
                   const uint64_t *d_off, const uint32_t *d_len, const int32_t *d_hdr4,
                   const uint8_t *d_lut, int del_run, const char *movie, uint8_t *d_text);

#ifdef __cplusplus
}
#endif
#endif
