/*
 * dx_file_place.c -- where on a reference every record of a .dexta / .dexar image lies, and on which strand: the index made of an
 * image's records (dx_file_kmer_index) or of plain letters (dx_kmer_index_from_letters, dx_pack_letters), the placement of an
 * image's records (dx_file_place), and the host step from that answer to a list of records that dx_file_subset takes
 * (dx_place_select).
 *
 * The index, the seeds and the vote are device code (csrc/place/).  dx_file_kmer_index opens the image as dx_file_kmer_set does and
 * sends it up WHOLE, in one slice of dxf_u2_slices: the records are the targets, and the builder wants them all.
 * dx_kmer_index_from_letters packs the letters on the host, every target at a byte of its own, and uploads the bytes with the
 * targets' places and lengths.
 *
 * dx_file_place walks and slices the image as dx_file_screen_spans does (dxf_image_open, dxf_u2_cap, dxf_u2_slices; 36 bytes a
 * record of the hook's own: the record's dx_place and its seed count).  Per slice the seeds are counted (dx_code_kmer_seeds with no
 * list) and the counts come down; consecutive records are grouped greedily so that a group's seeds stay at or below seed_room; a
 * group's seeds are listed from the counts that are there (dx_seeds_list_counted) into a device list that grows to the largest
 * group, dx_seeds_place votes, and the group's 32 bytes a record come down.  A group without a seed is answered on the host.  A
 * record lies in one slice and one group and no vote looks beyond its record, so the answer depends neither on the slicing nor on
 * the room.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dexgpu.h"
#include "dx_host.h"
#include "dx_files.h"

#define WHO_INDEX   "dx_file_kmer_index"
#define WHO_LETTERS "dx_kmer_index_from_letters"
#define WHO_PLACE   "dx_file_place"

/* DEXGPU_TIMING=1: where the driver spends its time (stderr) */
static void pmark(const char *what)
{ static double t0 = -1.0;
  dx_mark("place", &t0, what);
}

static int index_fail(dx_ctx *ctx, int code, const char *what) { return dx_place_fail(ctx, code, WHO_INDEX, what); }

/* ---- the index of an image's records ---------------------------------------------------------------------------------- */
typedef struct { dx_ctx *ctx; uint32_t k; int canonical, arrow; dx_kmer_index *x; } index_job;

static int index_slice(void *arg, const u2_slice *s)
{ index_job *j = arg;
  return dx_code_kmer_index(j->ctx, s->d_in, s->bytes, s->d_boff, NULL, s->d_len, s->n, j->k, j->canonical, j->arrow, &j->x);
}

int dx_file_kmer_index(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, uint32_t k, int canonical, dx_kmer_index **index)
{ image_text im;
  index_job  j;
  int        rc;
  if (ctx == NULL || index == NULL || (img == NULL && m)) return DX_E_ARG;
  *index = NULL;
  if ((rc = dxf_kmers_args(ctx, kind, k, 32, canonical, index_fail)) != DX_OK) return rc;
  memset(&j, 0, sizeof(j));
  j.ctx = ctx; j.k = k; j.canonical = canonical; j.arrow = kind == DX_KIND_ARROW;
  pmark(NULL);
  TRY(dxf_image_open(ctx, kind, 0, 1, img, m, &im));       /* (the line width lays out a text nobody makes) */
  pmark("the image walked");
  if (im.ux.cnt) TRY(dxf_u2_slices(ctx, img, &im.ux, 0, 0, index_slice, &j));             /* (cap 0: one slice, the whole image) */
  else TRY(dx_code_kmer_index(ctx, NULL, 0, NULL, NULL, NULL, 0, k, canonical, j.arrow, &j.x));
  pmark("the index made");
  *index = j.x; j.x = NULL;
  rc = DX_OK;

done:
  dxf_image_close(&im);
  if (j.x) (void) dx_kmer_index_free(ctx, j.x);
  return rc;
}

/* ---- the index of plain letters ---------------------------------------------------------------------------------------- */
int dx_pack_letters(int arrow, const char *seq, uint32_t len, uint8_t *out, uint32_t *bad_pos)
{ uint32_t i;
  if (bad_pos) *bad_pos = UINT32_MAX;
  if ((seq == NULL || out == NULL) && len) return DX_E_ARG;
  for (i = 0; i < len; i++)
    { const int s = dxf_find_letter(arrow, (unsigned char) seq[i]);
      if (s < 0)
        { if (bad_pos) *bad_pos = i;
          return DX_E_ARG;
        }
      if ((i & 3) == 0) out[i >> 2] = 0;
      out[i >> 2] |= (uint8_t) (s << (6 - 2 * (i & 3)));
    }
  return DX_OK;
}

int dx_kmer_index_from_letters(dx_ctx *ctx, int arrow, const char *const *seqs, const uint32_t *lens, uint64_t T, uint32_t k, int canonical,
                               dx_kmer_index **index)
{ uint8_t  *buf = NULL;
  uint64_t *boff = NULL, t, bytes = 0;
  void     *d = NULL;
  size_t    at_off, at_len;
  int       rc;
  if (ctx == NULL || index == NULL) return DX_E_ARG;
  *index = NULL;
  if ((seqs == NULL || lens == NULL) && T) return dx_place_fail(ctx, DX_E_ARG, WHO_LETTERS, "NULL pointer");
  if (T >= (1ull << 31)) return dx_place_fail(ctx, DX_E_ARG, WHO_LETTERS, "more than 2^31 - 1 targets");
  if (T == 0) return dx_code_kmer_index(ctx, NULL, 0, NULL, NULL, NULL, 0, k, canonical, arrow, index);
  if ((boff = malloc((size_t) T * sizeof(*boff))) == NULL) return DX_E_NOMEM;
  for (t = 0; t < T; t++)
    { boff[t] = bytes;
      bytes += ((uint64_t) lens[t] + 3) >> 2;
    }
  if ((buf = malloc((size_t) bytes + 16)) == NULL) { rc = DX_E_NOMEM; goto done; }
  for (t = 0; t < T; t++)
    { uint32_t bad = 0;
      if (dx_pack_letters(arrow, seqs[t], lens[t], buf + boff[t], &bad) != DX_OK)
        { char why[120];
          snprintf(why, sizeof(why), "target %llu, position %u: not a letter of the kind (%s)", (unsigned long long) t, bad, arrow ? "1234" : "acgtACGT");
          rc = dx_place_fail(ctx, DX_E_ARG, WHO_LETTERS, why);
          goto done;
        }
    }
  /* one block: the packed bytes, the targets' places, their lengths */
  at_off = ((size_t) bytes + 15) & ~(size_t) 7;
  at_len = at_off + (size_t) T * 8;
  TRY(dx_malloc(ctx, at_len + (size_t) T * 4 + 64, &d));
  if (bytes) TRY(dx_h2d(ctx, d, buf, (size_t) bytes));
  TRY(dx_h2d(ctx, (uint8_t *) d + at_off, boff, (size_t) T * 8));
  TRY(dx_h2d(ctx, (uint8_t *) d + at_len, lens, (size_t) T * 4));
  rc = dx_code_kmer_index(ctx, d, bytes, (const uint64_t *) ((uint8_t *) d + at_off), NULL, (const uint32_t *) ((uint8_t *) d + at_len), T, k, canonical,
                          arrow, index);

done:
  if (d) (void) dx_free(ctx, d);
  free(buf); free(boff);
  return rc;
}

/* ---- the placement of an image's records ------------------------------------------------------------------------------- */
typedef struct
  { dx_ctx *ctx; const dx_kmer_index *x;
    uint32_t k, max_occ, band_bits;
    uint64_t room;                /* seeds a group; 0: chosen, slice by slice */
    uint64_t windows, hits, seeds, votes, placed, groups;
    dx_place *rec;                /* one a record, or NULL */
    uint32_t *cnt; size_t cnt_cap;            /* a slice's counts on the host */
    void *d_seeds, *d_off; size_t d_seeds_cap, d_off_cap;
  } place_job;

static int place_slice(void *arg, const u2_slice *s)
{ place_job *j = arg;
  dx_ctx    *ctx = j->ctx;
  dx_place  *d_place = s->d_extra;
  uint32_t  *d_cnt = (uint32_t *) ((uint8_t *) s->d_extra + (size_t) s->n * sizeof(dx_place));
  uint64_t   t[4], pt[3], room = j->room, i, listed = 0;
  int        rc;
  if ((rc = dx_code_kmer_seeds(ctx, s->d_in, s->bytes, s->d_boff, NULL, s->d_len, s->n, j->x, j->max_occ, d_cnt, NULL, NULL, 0, t, NULL)) != DX_OK)
    return rc;
  j->windows += t[0]; j->hits += t[1]; j->seeds += t[2];
  if (s->n > j->cnt_cap)
    { uint32_t *bigger = realloc(j->cnt, (size_t) s->n * sizeof(*bigger));
      if (bigger == NULL) return DX_E_NOMEM;
      j->cnt = bigger; j->cnt_cap = s->n;
    }
  if ((rc = dx_d2h(ctx, j->cnt, d_cnt, (size_t) s->n * sizeof(*j->cnt))) != DX_OK) return rc;
  if (room == 0)
    { uint64_t fr = 0, all = 0;
      if (dx_mem_info(ctx, &fr, &all) == DX_OK) room = (uint64_t) (0.8 * (double) fr / 32.0);
      if (room == 0) room = 1;
    }

  for (i = 0; i < s->n; )
    { const uint64_t g0 = i;
      uint64_t sum = 0, r;
      for (; i < s->n && (i == g0 || sum + j->cnt[i] <= room); i++)
        { if (j->cnt[i] > room)
            { char why[160];
              snprintf(why, sizeof(why), "record %llu has %u seeds, and a group has room for %llu: raise seed_room or lower max_occ",
                       (unsigned long long) (s->i0 + i), j->cnt[i], (unsigned long long) room);
              return dx_place_fail(ctx, DX_E_NOMEM, WHO_PLACE, why);
            }
          sum += j->cnt[i];
        }
      if (sum == 0)                                        /* nobody has a seed: answered here */
        { if (j->rec != NULL)
            for (r = g0; r < i; r++)
              { memset(&j->rec[s->i0 + r], 0xff, sizeof(dx_place));
                j->rec[s->i0 + r].seeds = j->rec[s->i0 + r].votes = j->rec[s->i0 + r].strand = 0;
              }
          continue;
        }
      if (dgrow(ctx, &j->d_seeds, &j->d_seeds_cap, (size_t) sum * sizeof(dx_seed)) != DX_OK ||
          dgrow(ctx, &j->d_off, &j->d_off_cap, (size_t) (i - g0 + 1) * 8) != DX_OK)
        { char why[120];
          snprintf(why, sizeof(why), "no %llu bytes of device memory for a group's seeds: lower seed_room", (unsigned long long) (sum * sizeof(dx_seed)));
          return dx_place_fail(ctx, DX_E_NOMEM, WHO_PLACE, why);
        }
      if ((rc = dx_seeds_list_counted(ctx, s->d_in, s->bytes, s->d_boff + g0, s->d_len + g0, i - g0, j->x, j->max_occ, d_cnt + g0, j->d_off,
                                      j->d_seeds, sum, &listed)) != DX_OK) return rc;
      if (listed != sum) return dx_place_fail(ctx, DX_E_FORMAT, WHO_PLACE, "a group's seeds are not its records'");
      if ((rc = dx_seeds_place(ctx, j->d_seeds, j->d_off, i - g0, j->k, j->band_bits, d_place + g0, pt)) != DX_OK) return rc;
      j->votes += pt[1]; j->placed += pt[2]; j->groups++;
      if (j->rec != NULL && (rc = dx_d2h(ctx, j->rec + s->i0 + g0, d_place + g0, (size_t) (i - g0) * sizeof(dx_place))) != DX_OK) return rc;
    }
  return DX_OK;
}

int dx_file_place(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, const dx_kmer_index *index, uint32_t max_occ, uint32_t band_bits,
                  uint64_t seed_room, dx_place_report *out, dx_place **rec, uint32_t **rec_len)
{ image_text      im;
  dx_index_info   xi;
  dx_place_report rp;
  place_job       j;
  dx_place       *r = NULL;
  uint32_t       *rl = NULL;
  uint64_t        cnt, i;
  size_t          cap;
  const u2_index *x;
  int             rc;
  if (ctx == NULL || out == NULL || (img == NULL && m)) return DX_E_ARG;
  if (rec) *rec = NULL;
  if (rec_len) *rec_len = NULL;
  if (kind == DX_KIND_QUIVA)
    return dx_place_fail(ctx, DX_E_ARG, WHO_PLACE, "a .dexqv image has no packed reads to place (DX_KIND_FASTA or DX_KIND_ARROW)");
  if (kind != DX_KIND_FASTA && kind != DX_KIND_ARROW) return dx_place_fail(ctx, DX_E_ARG, WHO_PLACE, "unknown kind");
  if (dx_kmer_index_info(index, &xi) != DX_OK) return dx_place_fail(ctx, DX_E_ARG, WHO_PLACE, "no index");
  if ((xi.arrow != 0) != (kind == DX_KIND_ARROW))
    return dx_place_fail(ctx, DX_E_ARG, WHO_PLACE, xi.arrow ? "an index of pulse widths against a .dexta image" : "an index of bases against a .dexar image");
  if (max_occ < 1) return dx_place_fail(ctx, DX_E_ARG, WHO_PLACE, "max_occ 0 (1 at least)");
  if (band_bits > 31) return dx_place_fail(ctx, DX_E_ARG, WHO_PLACE, "band_bits above 31");
  memset(&rp, 0, sizeof(rp));
  rp.k = xi.k; rp.band_bits = band_bits;
  memset(&j, 0, sizeof(j));

  pmark(NULL);
  TRY(dxf_image_open(ctx, kind, 0, 1, img, m, &im));       /* (the line width lays out a text nobody makes) */
  x = &im.ux; cnt = x->cnt;
  rp.records = cnt;
  for (i = 0; i < cnt; i++) rp.symbols += x->nsym[i];
  cap = cnt ? dxf_u2_cap(ctx, m, cnt) : 0;
  if (rec != NULL && (r = malloc((size_t) (cnt ? cnt : 1) * sizeof(*r))) == NULL) { rc = DX_E_NOMEM; goto done; }
  if (rec_len != NULL)
    { if ((rl = malloc((size_t) (cnt ? cnt : 1) * sizeof(*rl))) == NULL) { rc = DX_E_NOMEM; goto done; }
      if (cnt) memcpy(rl, x->nsym, (size_t) cnt * sizeof(*rl));
    }
  pmark("the image walked");
  j.ctx = ctx; j.x = index; j.k = xi.k; j.max_occ = max_occ; j.band_bits = band_bits; j.room = seed_room; j.rec = r;
  TRY(dxf_u2_slices(ctx, img, x, cap, sizeof(dx_place) + sizeof(uint32_t), place_slice, &j));
  pmark("the slices up, their seeds counted, listed and voted on, the places back");
  rp.windows = j.windows; rp.hits = j.hits; rp.seeds = j.seeds; rp.votes = j.votes; rp.records_placed = j.placed; rp.groups = j.groups;

  *out = rp;
  if (rec) { *rec = r; r = NULL; }
  if (rec_len) { *rec_len = rl; rl = NULL; }
  rc = DX_OK;

done:
  dxf_image_close(&im);
  if (j.d_seeds) (void) dx_free(ctx, j.d_seeds);
  if (j.d_off) (void) dx_free(ctx, j.d_off);
  free(j.cnt); free(r); free(rl);
  return rc;
}

/* ---- the selection (host) ---------------------------------------------------------------------------------------------- */
int dx_place_select(const dx_place *rec, uint64_t records, const uint64_t *toff, uint64_t T, uint32_t target, uint32_t lo, uint32_t hi,
                    uint32_t min_votes, int strands, int mode, uint64_t **ids, uint64_t *n_ids)
{ uint64_t *out, i, n = 0, t;
  const uint32_t least = min_votes ? min_votes : 1;
  if (ids) *ids = NULL;
  if (n_ids) *n_ids = 0;
  if (ids == NULL || n_ids == NULL || toff == NULL || (rec == NULL && records)) return DX_E_ARG;
  if (strands < 1 || strands > 3 || lo > hi || (mode != DX_SCREEN_KEEP && mode != DX_SCREEN_DROP)) return DX_E_ARG;
  if (target != UINT32_MAX && target >= T) return DX_E_ARG;
  if (toff[0] != 0) return DX_E_ARG;
  for (t = 0; t < T; t++)
    if (toff[t + 1] < toff[t]) return DX_E_ARG;
  if ((out = malloc((size_t) (records ? records : 1) * sizeof(*out))) == NULL) return DX_E_NOMEM;
  for (i = 0; i < records; i++)
    { int match = 0;
      if (rec[i].votes >= least && rec[i].strand <= 1 && ((strands >> rec[i].strand) & 1) && rec[i].gbeg < toff[T])
        { uint64_t a = 0, b = T;                           /* toff[a] <= gbeg < toff[b] */
          while (b - a > 1)
            { const uint64_t mid = a + (b - a) / 2;
              if (toff[mid] <= rec[i].gbeg) a = mid; else b = mid;
            }
          if (target == UINT32_MAX || a == target)
            { const uint64_t tb = rec[i].gbeg - toff[a], te = (rec[i].gend < toff[a + 1] ? rec[i].gend : toff[a + 1]) - toff[a];
              match = tb < hi && lo < te;
            }
        }
      if (match == (mode == DX_SCREEN_KEEP)) out[n++] = i;
    }
  *ids = out; *n_ids = n;
  return DX_OK;
}
