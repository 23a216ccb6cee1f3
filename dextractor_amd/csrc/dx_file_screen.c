/*
 * dx_file_screen.c -- which records of a .dexta / .dexar image share k-mers with a set on the device, and how much of each they cover:
 * dx_file_screen; and the host step from that answer to a list of records that dx_file_subset takes: dx_screen_select.
 *
 * The set is made elsewhere (dx_kmer_set_from_codes, dx_file_kmer_set: screen/dx_kmer_set.hip, dx_file_kmers_wide.c) and stays on the
 * device; the reads are screened where they lie.  The image is opened and walked as dx_file_kmers_wide walks it (dxf_image_open;
 * slices of whole records under dxf_u2_cap / DEXGPU_TEXT_BUDGET, handed over by dxf_u2_slices with 16 bytes a record for the
 * kernel's entries); a slice's entries come down behind those of the slices before it, and its totals add.  A window never spans
 * two records and every record is in one slice, so the answer does not depend on the slicing.
 */
#include <stdlib.h>
#include <string.h>

#include "dexgpu.h"
#include "dx_host.h"
#include "dx_files.h"

/* DEXGPU_TIMING=1: where the driver spends its time (stderr) */
static void smark(const char *what)
{ static double t0 = -1.0;
  dx_mark("screen", &t0, what);
}

/* a slice of the image's packed reads (dxf_u2_slices): its records' entries made at d_extra and brought down, its totals added */
typedef struct { dx_ctx *ctx; const dx_kmer_set *set; dx_screen *rec; uint64_t total[4]; } screen_job;

static int screen_slice(void *arg, const u2_slice *s)
{ screen_job *j = arg;
  uint64_t    t[4];
  int         rc, i;
  if ((rc = dx_code_kmer_screen(j->ctx, s->d_in, s->bytes, s->d_boff, NULL, s->d_len, s->n, j->set, j->rec ? s->d_extra : NULL, t,
                                NULL)) != DX_OK) return rc;
  for (i = 0; i < 4; i++) j->total[i] += t[i];
  if (j->rec) return dx_d2h(j->ctx, j->rec + s->i0, s->d_extra, (size_t) s->n * sizeof(dx_screen));
  return DX_OK;
}

int dx_file_screen(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, const dx_kmer_set *set, dx_screen_report *out,
                   dx_screen **rec, uint32_t **rec_len)
{ image_text       im;
  dx_set_info      si;
  dx_screen_report rp;
  screen_job       j;
  dx_screen       *r = NULL;
  uint32_t        *rl = NULL;
  uint64_t         cnt, i;
  size_t           cap;
  const u2_index  *x;
  int              rc;
  if (ctx == NULL || out == NULL || (img == NULL && m)) return DX_E_ARG;
  if (rec) *rec = NULL;
  if (rec_len) *rec_len = NULL;
  if (kind == DX_KIND_QUIVA)
    return dx_screen_fail(ctx, DX_E_ARG, "a .dexqv image has no packed reads to screen (DX_KIND_FASTA or DX_KIND_ARROW)");
  if (kind != DX_KIND_FASTA && kind != DX_KIND_ARROW) return dx_screen_fail(ctx, DX_E_ARG, "unknown kind");
  if (dx_kmer_set_info(set, &si) != DX_OK) return dx_screen_fail(ctx, DX_E_ARG, "no set");
  if ((si.arrow != 0) != (kind == DX_KIND_ARROW))
    return dx_screen_fail(ctx, DX_E_ARG, si.arrow ? "a set of pulse widths against a .dexta image" : "a set of bases against a .dexar image");
  memset(&rp, 0, sizeof(rp));
  rp.k = si.k;

  smark(NULL);
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
  smark("the image walked");
  memset(&j, 0, sizeof(j));
  j.ctx = ctx; j.set = set; j.rec = r;
  TRY(dxf_u2_slices(ctx, img, x, cap, sizeof(dx_screen), screen_slice, &j));
  smark("the slices up and screened, their entries back");
  rp.windows = j.total[0]; rp.hits = j.total[1]; rp.covered = j.total[2]; rp.records_hit = j.total[3];

  *out = rp;
  if (rec) { *rec = r; r = NULL; }
  if (rec_len) { *rec_len = rl; rl = NULL; }
  rc = DX_OK;

done:
  dxf_image_close(&im);
  free(r); free(rl);
  return rc;
}

/* ---- the selection (host) -------------------------------------------------------------------------------------------- */
int dx_screen_select(const dx_screen *rec, const uint32_t *rec_len, uint64_t records, uint32_t min_hits, uint32_t min_permille,
                     int mode, uint64_t **ids, uint64_t *n_ids)
{ uint64_t *out, i, n = 0;
  const uint32_t least = min_hits ? min_hits : 1;
  if (ids) *ids = NULL;
  if (n_ids) *n_ids = 0;
  if (ids == NULL || n_ids == NULL || ((rec == NULL || rec_len == NULL) && records)) return DX_E_ARG;
  if (min_permille > 1000 || (mode != DX_SCREEN_KEEP && mode != DX_SCREEN_DROP)) return DX_E_ARG;
  if ((out = malloc((size_t) (records ? records : 1) * sizeof(*out))) == NULL) return DX_E_NOMEM;
  for (i = 0; i < records; i++)
    { const int match = rec[i].hits >= least && (uint64_t) rec[i].covered * 1000 >= (uint64_t) min_permille * rec_len[i];
      if (match == (mode == DX_SCREEN_KEEP)) out[n++] = i;
    }
  *ids = out; *n_ids = n;
  return DX_OK;
}
