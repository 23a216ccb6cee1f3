/*
 * dx_file_find.c -- where given sequences occur in the reads of a .dexta / .dexar image: dx_file_find.
 *
 * Today the question takes undexta -U of the whole file and a text search on one core.  Here the image is walked on the host
 * (dxf_image_open: any key, legacy layout or byte order) and uploaded, and the packed reads are searched where they lie
 * (dx_code_find, units ux.ioff / ux.nsym): no text is made, a quarter of its bytes is read, and there are no header lines or line
 * wraps to step over.
 *
 * The search is over what the archive HOLDS: an N that dexta stored as a is an a (Number_Read, DB.c:393-416, codes every letter that is not
 * c, g or t as 0).  The hits are exactly those a search of the letters undexta -U / undexar prints, record by record, would find.
 *
 * A pattern becomes one query, or two with both_strands: the reverse complement is the codes 3 - c in reverse order, and a pattern
 * that equals its own is searched once.  The queries stand in the order (pattern, strand), so that the kernel's order (unit, pos,
 * query) is the file's (record, pos, pattern, strand); dxf_find_map then names every hit by its pattern and strand.
 * An image that does not fit the device, or exceeds DEXGPU_TEXT_BUDGET, goes in slices of whole records (dxf_u2_slices, dx_file_u2.c): a
 * slice's hits are listed into what max_hits has left, its record numbers moved by the slice's first record.
 *
 * Everything behind the plan is dxf_find_run, which dx_file_find_edit.c calls with its own plan and kernel (edit = 1) -- and, for
 * dx_file_find_edit_spans, with a place for the occurrences' starts: dx_code_hit_starts then runs once a slice behind its listing.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dexgpu.h"
#include "dx_host.h"
#include "dx_files.h"

#define FIND_ROOM ((uint64_t) 1 << 20)       /* hits a slice is listed into at first; one with more is searched again into enough */

/* a letter's code (Number_Read / Number_Arrow, DB.c:393-441), or -1 when it is none of the kind's */
int dxf_find_letter(int arrow, int c)
{ if (arrow) return c >= '1' && c <= '4' ? c - '1' : -1;
  switch (c)
    { case 'a': case 'A': return 0;
      case 'c': case 'C': return 1;
      case 'g': case 'G': return 2;
      case 't': case 'T': return 3;
      default:            return -1;
    }
}

int dxf_find_plan(dx_ctx *ctx, int kind, const char *const *pattern, uint32_t npat, uint32_t max_mis, int both_strands, find_plan *fp)
{ char     why[160];
  uint32_t p, least = UINT32_MAX;
  memset(fp, 0, sizeof(*fp));
  if (kind == DX_KIND_QUIVA)
    return dx_find_fail(ctx, DX_E_ARG, "a .dexqv image has no packed reads to search (DX_KIND_FASTA or DX_KIND_ARROW)");
  if (kind != DX_KIND_FASTA && kind != DX_KIND_ARROW) return dx_find_fail(ctx, DX_E_ARG, "unknown kind");
  if (both_strands && kind == DX_KIND_ARROW)
    return dx_find_fail(ctx, DX_E_ARG, "both_strands: pulse widths have no complement (DX_KIND_FASTA only)");
  if (pattern == NULL || npat < 1 || npat > (both_strands ? 32u : 64u))
    { snprintf(why, sizeof(why), "%u patterns (1 to %u%s)", npat, both_strands ? 32u : 64u, both_strands ? " with both_strands" : "");
      return dx_find_fail(ctx, DX_E_ARG, why);
    }
  for (p = 0; p < npat; p++)
    { const char *s = pattern[p];
      const size_t len = s ? strlen(s) : 0;
      uint64_t code = 0, rev = 0;
      size_t   i;
      if (len < 1 || len > 32)
        { snprintf(why, sizeof(why), "pattern %u has %zu letters (1 to 32)", p, len);
          return dx_find_fail(ctx, DX_E_ARG, why);
        }
      for (i = 0; i < len; i++)
        { const int c = dxf_find_letter(kind == DX_KIND_ARROW, (unsigned char) s[i]);
          if (c < 0)
            { snprintf(why, sizeof(why), "pattern %u, column %zu: not one of %s", p, i + 1, kind == DX_KIND_ARROW ? "1234" : "acgtACGT");
              return dx_find_fail(ctx, DX_E_ARG, why);
            }
          code = (code << 2) | (uint64_t) c;
          rev |= (uint64_t) (3 - c) << (2 * i);            /* letter i is letter len - 1 - i of the reverse: in the bits 2 i + 1, 2 i */
        }
      if (len < least) least = (uint32_t) len;
      fp->q[fp->nq].code = code; fp->q[fp->nq].len = (uint32_t) len; fp->q[fp->nq].max_mis = max_mis;
      fp->pat[fp->nq] = (uint16_t) p; fp->strand[fp->nq] = 0; fp->nq++;
      if (both_strands && rev != code)
        { fp->q[fp->nq].code = rev; fp->q[fp->nq].len = (uint32_t) len; fp->q[fp->nq].max_mis = max_mis;
          fp->pat[fp->nq] = (uint16_t) p; fp->strand[fp->nq] = 1; fp->nq++;
        }
    }
  if (max_mis >= least)
    { snprintf(why, sizeof(why), "%u mismatches: not below the shortest pattern's %u letters", max_mis, least);
      return dx_find_fail(ctx, DX_E_ARG, why);
    }
  return DX_OK;
}

void dxf_find_map(const find_plan *fp, dx_hit *h, uint64_t cnt, uint64_t i0)
{ uint64_t k;
  for (k = 0; k < cnt; k++)
    { const uint16_t q = h[k].query;
      h[k].record += i0; h[k].query = fp->pat[q]; h[k].strand = fp->strand[q];
    }
}

int dx_file_find(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, const char *const *pattern, uint32_t npat, uint32_t max_mis,
                 int both_strands, uint64_t max_hits, dx_find *out, dx_hit **hits, uint32_t **rec_hits)
{ find_plan fp;
  int       rc;
  if (ctx == NULL || out == NULL || (img == NULL && m)) return DX_E_ARG;
  if (hits) *hits = NULL;
  if (rec_hits) *rec_hits = NULL;
  if ((rc = dxf_find_plan(ctx, kind, pattern, npat, max_mis, both_strands, &fp)) != DX_OK) return rc;
  return dxf_find_run(ctx, kind, img, m, &fp, 0, max_hits, out, hits, rec_hits, NULL, NULL);
}

/* what dxf_find_run holds across the slices: the plan, the report so far, every record's count, the hits kept and (start wanted) their
   starts, and the device arrays a slice's hits and starts are listed into */
typedef struct
  { dx_ctx *ctx; const find_plan *fp; int edit, starts;
    dx_find  *fd;
    uint32_t *rec, *st;
    dx_hit   *list;
    uint64_t  keep, kept, list_cap;
    void     *d_hits, *d_st;
    size_t    hit_cap, st_cap;
  } find_job;

/* a slice of the image's packed reads (dxf_u2_slices, 4 bytes a record of its own: the record's count) searched, its hits listed into
   what `keep` has left */
static int find_slice(void *arg, const u2_slice *s)
{ find_job *j = arg;
  dx_ctx   *ctx = j->ctx;
  const find_plan *fp = j->fp;
  uint32_t *d_cnt = s->d_extra;
  uint64_t  i, found = 0, room, tot[64];
  int       rc;
  room = j->keep - j->kept < FIND_ROOM ? j->keep - j->kept : FIND_ROOM;
  for (;;)                                                  /* (a second time only for a slice with more hits than FIND_ROOM that are wanted) */
    { TRY(dgrow(ctx, &j->d_hits, &j->hit_cap, (size_t) room * sizeof(dx_hit) + 64));
      if (j->edit) TRY(dx_code_find_edit(ctx, s->d_in, s->bytes, s->d_boff, NULL, s->d_len, s->n, fp->eq, fp->nq, d_cnt, j->d_hits, room, tot, &found, NULL));
      else         TRY(dx_code_find(ctx, s->d_in, s->bytes, s->d_boff, NULL, s->d_len, s->n, fp->q, fp->nq, d_cnt, j->d_hits, room, tot, &found, NULL));
      if (found <= room || room == j->keep - j->kept) break;
      room = found < j->keep - j->kept ? found : j->keep - j->kept;
      if (room > UINT32_MAX)
        return (j->edit ? dx_find_edit_fail : dx_find_fail)(ctx, DX_E_NOMEM, "more than 2^32 - 1 hits of one slice to list: lower max_hits");
    }
  TRY(dx_d2h(ctx, j->rec + s->i0, d_cnt, (size_t) s->n * 4));
  for (i = 0; i < fp->nq; i++) j->fd->per_pattern[fp->pat[i]][fp->strand[i]] += tot[i];
  j->fd->hits += found;
  { const uint64_t got = found < room ? found : room;
    if (got)
      { if (j->kept + got > j->list_cap)
          { const uint64_t want = j->kept + got > 2 * j->list_cap ? j->kept + got : 2 * j->list_cap;
            dx_hit *bigger = realloc(j->list, (size_t) want * sizeof(*j->list));
            if (bigger == NULL) return DX_E_NOMEM;
            j->list = bigger; j->list_cap = want;
            if (j->starts)
              { uint32_t *more = realloc(j->st, (size_t) want * sizeof(*j->st));
                if (more == NULL) return DX_E_NOMEM;
                j->st = more;
              }
          }
        if (j->starts)                                      /* the slice's image and its unit-relative hits are still on the device */
          { TRY(dgrow(ctx, &j->d_st, &j->st_cap, (size_t) got * sizeof(*j->st) + 64));
            TRY(dx_code_hit_starts(ctx, s->d_in, s->bytes, s->d_boff, NULL, s->d_len, s->n, fp->eq, fp->nq, j->d_hits, got, j->d_st, NULL));
            TRY(dx_d2h(ctx, j->st + j->kept, j->d_st, (size_t) got * sizeof(*j->st)));
          }
        TRY(dx_d2h(ctx, j->list + j->kept, j->d_hits, (size_t) got * sizeof(*j->list)));
        dxf_find_map(fp, j->list + j->kept, got, s->i0);
        j->kept += got;
      }
  }
done:
  return rc;
}

int dxf_find_run(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, const find_plan *fp, int edit, uint64_t max_hits, dx_find *out,
                 dx_hit **hits, uint32_t **rec_hits, uint32_t **start, uint32_t **rec_len)
{ image_text im;
  find_job   j;
  uint32_t  *rlen = NULL;
  uint64_t   cnt, i;
  int        rc;

  memset(&j, 0, sizeof(j));
  j.ctx = ctx; j.fp = fp; j.edit = edit; j.starts = start != NULL;
  j.keep = hits != NULL ? max_hits : 0;                    /* hits the list is to hold (nobody takes it: none) */
  TRY(dxf_image_open(ctx, kind, 0, 1, img, m, &im));       /* (the line width lays out a text nobody makes) */
  cnt = im.ux.cnt;
  if ((j.fd = calloc(1, sizeof(*j.fd))) == NULL || (j.rec = malloc((cnt + 1) * sizeof(*j.rec))) == NULL) { rc = DX_E_NOMEM; goto done; }
  j.fd->records = cnt;
  if (rec_len)
    { if ((rlen = malloc((cnt + 1) * sizeof(*rlen))) == NULL) { rc = DX_E_NOMEM; goto done; }
      if (cnt) memcpy(rlen, im.ux.nsym, (size_t) cnt * sizeof(*rlen));
    }

  TRY(dxf_u2_slices(ctx, img, &im.ux, cnt ? dxf_u2_cap(ctx, m, cnt) : 0, 4, find_slice, &j));
  for (i = 0; i < cnt; i++) j.fd->records_hit += j.rec[i] != 0;
  j.fd->listed = j.fd->hits < max_hits ? j.fd->hits : max_hits;
  if (hits != NULL && j.list == NULL && (j.list = malloc(sizeof(*j.list))) == NULL) { rc = DX_E_NOMEM; goto done; }
  if (start != NULL && j.st == NULL && (j.st = malloc(sizeof(*j.st))) == NULL) { rc = DX_E_NOMEM; goto done; }

  *out = *j.fd;
  if (hits) { *hits = j.list; j.list = NULL; }
  if (rec_hits) { *rec_hits = j.rec; j.rec = NULL; }
  if (start) { *start = j.st; j.st = NULL; }
  if (rec_len) { *rec_len = rlen; rlen = NULL; }
  rc = DX_OK;

done:
  if (j.d_hits) (void) dx_free(ctx, j.d_hits);
  if (j.d_st) (void) dx_free(ctx, j.d_st);
  dxf_image_close(&im);
  free(j.fd); free(j.list); free(j.rec); free(j.st); free(rlen);
  return rc;
}
