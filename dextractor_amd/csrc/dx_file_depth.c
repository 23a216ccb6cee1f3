/*
 * dx_file_depth.c -- how often the k-mers of every record of a .dexta / .dexar image were seen, against a counted set on the device:
 * dx_file_depth (per record the windows, the hits, the sum and the quantiles of its depths; on request the whole profile); and the host
 * step from that answer to a list of records that dx_file_subset takes: dx_depth_select.
 *
 * The set is made elsewhere (dx_file_kmer_set_counted, dx_files_kmer_set_counted, dx_kmer_set_from_kmers: screen/dx_kmer_set.hip) and
 * stays on the device; an uncounted set gives the membership.  The image is opened and walked as dx_file_screen walks it
 * (dxf_image_open; slices of whole records under dxf_u2_cap / DEXGPU_TEXT_BUDGET, handed over by dxf_u2_slices with 32 bytes a record
 * for the entries).  A slice's windows are known from its records' lengths: the slice takes one device block of exactly its size --
 * the records' places (8 a record and 8) and the profile (2 a window) --, dx_code_kmer_depths fills it, dx_depth_stats reads it, the
 * entries come down behind those of the slices before, the profile too when it is asked for, and the block is freed.  A byte of
 * image holds 4 symbols, so a slice's profile takes up to 8 times the slice: the slice cap is narrowed to a tenth of the free memory
 * where the image and its profile do not fit together, and a record whose own block cannot be had is DX_E_NOMEM, dx_malloc naming
 * the bytes.  A window never spans two records and every record is in one slice, so the answer does not depend on the slicing.
 */
#include <stdlib.h>
#include <string.h>

#include "dexgpu.h"
#include "dx_host.h"
#include "dx_files.h"

/* DEXGPU_TIMING=1: where the driver spends its time (stderr) */
static void dmark(const char *what)
{ static double t0 = -1.0;
  dx_mark("depth", &t0, what);
}

/* a slice of the image's packed reads (dxf_u2_slices): its profile made and read, its records' entries made at d_extra and brought
   down, its totals added; roff: every record's place in the image's profile (cnt + 1) */
typedef struct { dx_ctx *ctx; const dx_kmer_set *set; dx_depth *rec; uint16_t *prof; const uint64_t *roff; uint64_t total[4]; } depth_job;

static int depth_slice(void *arg, const u2_slice *s)
{ depth_job     *j = arg;
  const uint64_t w0 = j->roff[s->i0], w = j->roff[s->i0 + s->n] - w0;
  const size_t   offs = ((size_t) s->n + 1) * 8;
  uint64_t       t[4], got = 0;
  void          *d = NULL;
  int            rc, i;
  TRY(dx_malloc(j->ctx, offs + (size_t) w * 2 + 64, &d));
  TRY(dx_code_kmer_depths(j->ctx, s->d_in, s->bytes, s->d_boff, NULL, s->d_len, s->n, j->set, (uint16_t *) ((uint8_t *) d + offs), w, d, &got,
                          NULL));
  if (got != w) { rc = dx_depth_fail(j->ctx, DX_E_FORMAT, "a slice's windows are not its records'"); goto done; }
  TRY(dx_depth_stats(j->ctx, (const uint16_t *) ((uint8_t *) d + offs), d, s->n, j->rec ? s->d_extra : NULL, t));
  for (i = 0; i < 4; i++) j->total[i] += t[i];
  if (j->rec) TRY(dx_d2h(j->ctx, j->rec + s->i0, s->d_extra, (size_t) s->n * sizeof(dx_depth)));
  if (j->prof && w) TRY(dx_d2h(j->ctx, j->prof + w0, (uint8_t *) d + offs, (size_t) w * 2));
  rc = DX_OK;
done:
  if (d) (void) dx_free(j->ctx, d);
  return rc;
}

int dx_file_depth(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, const dx_kmer_set *set, dx_depth_report *out,
                  dx_depth **rec, uint32_t **rec_len, uint16_t **profile, uint64_t **rec_off)
{ image_text      im;
  dx_set_info     si;
  dx_depth_report rp;
  depth_job       j;
  dx_depth       *r = NULL;
  uint32_t       *rl = NULL;
  uint16_t       *pf = NULL;
  uint64_t       *ro = NULL, cnt, i, fr = 0, all = 0;
  size_t          cap;
  const u2_index *x;
  int             rc;
  if (ctx == NULL || out == NULL || (img == NULL && m)) return DX_E_ARG;
  if (rec) *rec = NULL;
  if (rec_len) *rec_len = NULL;
  if (profile) *profile = NULL;
  if (rec_off) *rec_off = NULL;
  if (kind == DX_KIND_QUIVA)
    return dx_depth_fail(ctx, DX_E_ARG, "a .dexqv image has no packed reads to look up (DX_KIND_FASTA or DX_KIND_ARROW)");
  if (kind != DX_KIND_FASTA && kind != DX_KIND_ARROW) return dx_depth_fail(ctx, DX_E_ARG, "unknown kind");
  if (dx_kmer_set_info(set, &si) != DX_OK) return dx_depth_fail(ctx, DX_E_ARG, "no set");
  if ((si.arrow != 0) != (kind == DX_KIND_ARROW))
    return dx_depth_fail(ctx, DX_E_ARG, si.arrow ? "a set of pulse widths against a .dexta image" : "a set of bases against a .dexar image");
  memset(&rp, 0, sizeof(rp));
  rp.k = si.k;

  dmark(NULL);
  TRY(dxf_image_open(ctx, kind, 0, 1, img, m, &im));       /* (the line width lays out a text nobody makes) */
  x = &im.ux; cnt = x->cnt;
  rp.records = cnt;
  if ((ro = malloc(((size_t) cnt + 1) * sizeof(*ro))) == NULL) { rc = DX_E_NOMEM; goto done; }
  for (ro[0] = 0, i = 0; i < cnt; i++)                     /* the windows, from the lengths: every record's place in the profile */
    { rp.symbols += x->nsym[i];
      ro[i + 1] = ro[i] + (x->nsym[i] >= si.k ? x->nsym[i] - si.k + 1 : 0);
    }
  cap = cnt ? dxf_u2_cap(ctx, m, cnt) : 0;
  if (cnt && dx_mem_info(ctx, &fr, &all) == DX_OK && fr &&
      (double) m + 96.0 * (double) cnt + 2.0 * (double) ro[cnt] > 0.9 * (double) fr)       /* the image and its profile do not fit together */
    { const size_t tenth = (size_t) (0.9 * (double) fr / 10.0);
      if (cap == 0 || cap > tenth) cap = tenth ? tenth : 1;
    }
  if (rec != NULL && (r = malloc((size_t) (cnt ? cnt : 1) * sizeof(*r))) == NULL) { rc = DX_E_NOMEM; goto done; }
  if (rec_len != NULL)
    { if ((rl = malloc((size_t) (cnt ? cnt : 1) * sizeof(*rl))) == NULL) { rc = DX_E_NOMEM; goto done; }
      if (cnt) memcpy(rl, x->nsym, (size_t) cnt * sizeof(*rl));
    }
  if (profile != NULL && (pf = malloc((size_t) (ro[cnt] ? ro[cnt] : 1) * sizeof(*pf))) == NULL) { rc = DX_E_NOMEM; goto done; }
  dmark("the image walked");
  memset(&j, 0, sizeof(j));
  j.ctx = ctx; j.set = set; j.rec = r; j.prof = pf; j.roff = ro;
  TRY(dxf_u2_slices(ctx, img, x, cap, sizeof(dx_depth), depth_slice, &j));
  dmark("the slices up, their profiles made and read, their entries back");
  if (j.total[0] != ro[cnt]) { rc = dx_depth_fail(ctx, DX_E_FORMAT, "the slices' windows are not the image's"); goto done; }
  rp.windows = j.total[0]; rp.hits = j.total[1]; rp.sum = j.total[2]; rp.records_hit = j.total[3];

  *out = rp;
  if (rec) { *rec = r; r = NULL; }
  if (rec_len) { *rec_len = rl; rl = NULL; }
  if (profile) { *profile = pf; pf = NULL; }
  if (rec_off) { *rec_off = ro; ro = NULL; }
  rc = DX_OK;

done:
  dxf_image_close(&im);
  free(r); free(rl); free(pf); free(ro);
  return rc;
}

/* ---- the selection (host) -------------------------------------------------------------------------------------------- */
int dx_depth_select(const dx_depth *rec, uint64_t records, int stat, uint32_t lo, uint32_t hi, uint32_t min_windows, int mode,
                    uint64_t **ids, uint64_t *n_ids)
{ uint64_t *out, i, n = 0;
  const uint32_t least = min_windows ? min_windows : 1;
  if (ids) *ids = NULL;
  if (n_ids) *n_ids = 0;
  if (ids == NULL || n_ids == NULL || (rec == NULL && records)) return DX_E_ARG;
  if (stat < DX_DEPTH_MIN || stat > DX_DEPTH_MAX || lo > hi || (mode != DX_SCREEN_KEEP && mode != DX_SCREEN_DROP)) return DX_E_ARG;
  if ((out = malloc((size_t) (records ? records : 1) * sizeof(*out))) == NULL) return DX_E_NOMEM;
  for (i = 0; i < records; i++)
    { const uint16_t five[5] = { rec[i].min, rec[i].q1, rec[i].median, rec[i].q3, rec[i].max };
      const int match = rec[i].windows >= least && lo <= five[stat] && five[stat] <= hi;
      if (match == (mode == DX_SCREEN_KEEP)) out[n++] = i;
    }
  *ids = out; *n_ids = n;
  return DX_OK;
}
