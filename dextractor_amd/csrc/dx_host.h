/*
 * dx_host.h -- what the library's host C files (dx_host.c, dx_walk_host.c, the file drivers of dx_files.h) share among themselves; no part of the C-ABI.
 */
#ifndef DX_HOST_H
#define DX_HOST_H
#include <stddef.h>
#include <stdint.h>
#include "dexgpu.h"

static inline uint16_t flip16(uint16_t v) { return (uint16_t) ((v << 8) | (v >> 8)); }
static inline uint32_t flip32(uint32_t v)
{ return (v << 24) | ((v & 0xff00u) << 8) | ((v >> 8) & 0xff00u) | (v >> 24); }

/* DEXGPU_TIMING=1: "[tag  12.3 ms] what" on stderr, the time since the watch *t0 was started: by its first mark when it
   is set to a negative value beforehand, or anew by a mark with what == NULL (which prints nothing) */
void dx_mark(const char *tag, double *t0, const char *what);

/* The head of a .dexqv image (undexqv.c:103-110, QV.c:1222-1256): the 0x55aa key of the newer layout when it is there, then
   the coding with the prefix in front of it.  Fills newv, flip, coding and prefix (malloc'd, also when the coding behind it
   does not read: dx_qv_index_free) of *x, which the caller has zeroed; *first = the offset of the first record. */
int dx_qv_read_head(const uint8_t *img, size_t n, dx_qv_index *x, size_t *first);

/* DX_E_FORMAT with the words for it (dx_last_error): entry `id` of a record stream of nbytes bytes, which starts at byte `at`, does
   not end inside the stream.  Defined beside dx_qv_walk_records_device (records/dx_qv_records.hip: a context's error text is
   written by the device files' dx_fail); dx_entries_uncompress names the caller's entry with it, not its place in a slice. */
int dx_entry_fail(dx_ctx *ctx, uint64_t id, uint64_t at, uint64_t nbytes);

/* `code` with the words for it (dx_last_error; ctx NULL: the text dx_last_error(NULL) gives): "<who>: unit <j>: <what>".  Defined beside
   dx_entry_fail, for the host files that check a selection's units (dx_file_subset.c); the library does not export it. */
__attribute__((visibility("hidden"))) int dx_unit_fail(dx_ctx *ctx, int code, const char *who, uint64_t j, const char *what);

/* `code`, with the letter of the image it is about ('a', 'b') in front of the context's error text: "a: <the words>".  side 0 empties the
   text and changes nothing else: a host walk fails without words, and what an earlier call left must not pass for them.  Defined in
   compare/dx_diff.hip, for dx_file_compare.c. */
__attribute__((visibility("hidden"))) int dx_side_fail(dx_ctx *ctx, int code, int side);

/* `code` with the words for it (dx_last_error; ctx NULL: nothing is kept): "dx_file_find: <what>".  Defined in find/dx_find.hip, for
   dx_file_find.c, which words its refusals itself (the pattern's index and the column). */
__attribute__((visibility("hidden"))) int dx_find_fail(dx_ctx *ctx, int code, const char *what);
/* ... and "dx_file_find_edit: <what>", defined in find/dx_find_edit.hip, for dx_file_find_edit.c */
__attribute__((visibility("hidden"))) int dx_find_edit_fail(dx_ctx *ctx, int code, const char *what);
/* ... and "dx_file_cut: <what>", defined in find/dx_find_span.hip, for dx_file_cut.c */
__attribute__((visibility("hidden"))) int dx_cut_fail(dx_ctx *ctx, int code, const char *what);
/* ... and "dx_file_kmers: <what>", defined in kmers/dx_kmers.hip, for dx_file_kmers.c */
__attribute__((visibility("hidden"))) int dx_kmers_fail(dx_ctx *ctx, int code, const char *what);
/* ... and "dx_file_kmers_wide: <what>", defined in kmers/dx_kmer_runs.hip, for dx_file_kmers_wide.c */
__attribute__((visibility("hidden"))) int dx_kmers_wide_fail(dx_ctx *ctx, int code, const char *what);
/* ... and "<who>: <what>", defined in kmers/dx_kmer_bins.hip, for the two drivers of dx_file_kmers_files.c; "<who>: image <i>: <the words
   the walk left>" for an image that does not open (image < 0 empties the text and changes nothing else); and what they copy from one
   device array to another, behind everything on the context's stream, which is waited for */
__attribute__((visibility("hidden"))) int dx_kmers_files_fail(dx_ctx *ctx, int code, const char *who, const char *what);
__attribute__((visibility("hidden"))) int dx_kmers_files_image_fail(dx_ctx *ctx, int code, const char *who, int64_t image);
__attribute__((visibility("hidden"))) int dx_d2d(dx_ctx *ctx, void *d_dst, const void *d_src, size_t bytes);
/* ... and "dx_file_kmer_set: <what>", defined in screen/dx_kmer_set.hip, for dx_file_kmers_wide.c, and "dx_file_screen: <what>", in
   screen/dx_screen.hip, for dx_file_screen.c */
__attribute__((visibility("hidden"))) int dx_kmer_set_fail(dx_ctx *ctx, int code, const char *what);
__attribute__((visibility("hidden"))) int dx_screen_fail(dx_ctx *ctx, int code, const char *what);
/* ... and "dx_file_depth: <what>", defined in screen/dx_screen_depth.hip, for dx_file_depth.c */
__attribute__((visibility("hidden"))) int dx_depth_fail(dx_ctx *ctx, int code, const char *what);

/* What dx_files_kmer_set_counted wants of screen/dx_kmer_set.hip beyond the C-ABI.  dx_sorted_take_counted: dx_sorted_take with every kept
   run's length, saturated at 2^32 - 1, in d_count beside its first key in d_codes (cap of each; cap == 0 counts only, cap < *found is
   DX_E_ARG); the runs are listed by dx_kmer_runs as 16-byte pairs, into d_tmp when 2 *found <= tmp_words (d_tmp may be NULL), else into a
   block made and freed there.  dx_kmer_set_from_counted: the counted set of n distinct ascending codes and their counts on the device,
   which are copied. */
__attribute__((visibility("hidden"))) int dx_sorted_take_counted(dx_ctx *ctx, const uint64_t *d_sorted, uint64_t n, uint64_t min_count,
                                                                 void *d_tmp, uint64_t tmp_words, uint64_t *d_codes, uint32_t *d_count,
                                                                 uint64_t cap, uint64_t *found);
__attribute__((visibility("hidden"))) int dx_kmer_set_from_counted(dx_ctx *ctx, const uint64_t *d_codes, const uint32_t *d_count, uint64_t n,
                                                                   uint32_t k, int canonical, int arrow, dx_kmer_set **set);
/* ... and "<who>: <what>", defined in screen/dx_screen_spans.hip, for the two drivers of dx_file_screen_spans.c */
__attribute__((visibility("hidden"))) int dx_screen_spans_fail(dx_ctx *ctx, int code, const char *who, const char *what);

/* What dx_file_screen_spans wants of dx_code_kmer_spans beyond the C-ABI (screen/dx_screen_spans.hip): the list alone, for units whose
   counts a counting call over the same arguments (d_beg NULL) has left in d_count -- the driver counts a slice first, to size the
   list, and the look-ups are made once more, not twice.  *listed (may be NULL) = the counts' sum. */
__attribute__((visibility("hidden"))) int dx_spans_list_counted(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_boff,
                                                                const uint32_t *d_len, uint64_t n, const dx_kmer_set *set, uint32_t *d_count,
                                                                dx_span *d_spans, uint64_t cap, uint64_t *listed);

/* "<who>: <what>", defined in place/dx_kmer_index.hip, for the drivers of dx_file_place.c */
__attribute__((visibility("hidden"))) int dx_place_fail(dx_ctx *ctx, int code, const char *who, const char *what);

/* What dx_file_place wants of dx_code_kmer_seeds beyond the C-ABI (place/dx_place_seeds.hip): the list alone, for units whose counts a
   counting call over the same arguments (d_beg NULL) has left in d_count -- the driver counts a slice first, to form its groups.
   d_off (n + 1, may be NULL) gets the units' places; *listed (may be NULL) = the counts' sum. */
__attribute__((visibility("hidden"))) int dx_seeds_list_counted(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_boff,
                                                                const uint32_t *d_len, uint64_t n, const dx_kmer_index *index, uint32_t max_occ,
                                                                uint32_t *d_count, uint64_t *d_off, dx_seed *d_seeds, uint64_t cap,
                                                                uint64_t *listed);

/* What dx_file_digest wants of the CRC kernels beyond the C-ABI (digest/dx_crc.hip).  dx_crc32_ranges with a stride through its three
   arrays: unit j is d_off[j * stride], d_len[j * stride] -> d_crc[j * stride] -- header lines and bodies lie in two buffers, and their
   (crc, length) pairs are wanted side by side in record order.  dx_crc32_pairs: units 2 k and 2 k + 1 joined into unit k of the
   output arrays (a record's header line and its body -> the record), m of them, on the device; nothing comes back. */
int dx_crc32_ranges_strided(dx_ctx *ctx, const uint8_t *d_buf, uint64_t buf_bytes, const uint64_t *d_off, const uint64_t *d_len,
                            uint64_t n, uint64_t stride, uint32_t *d_crc, uint64_t *bad_unit);
int dx_crc32_pairs(dx_ctx *ctx, const uint32_t *d_crc, const uint64_t *d_len, uint64_t m, uint32_t *d_out_crc, uint64_t *d_out_len);

#ifdef __cplusplus
/* For the device files alone (dx_qv.hip defines it with C++ linkage, whatever block this header is included in): the exclusive sums
   of n counts on the device, d_out[0 .. n] with the total last; the total also comes back (`total` may be NULL) */
extern "C++" int dx_scan_u32(dx_ctx *ctx, const uint32_t *d_in, uint64_t n, uint64_t *d_out, uint64_t *total);
#endif

#endif
