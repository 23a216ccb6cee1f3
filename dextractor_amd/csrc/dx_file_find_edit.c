/*
 * dx_file_find_edit.c -- where given sequences occur in the reads of a .dexta / .dexar image with insertions and deletions allowed:
 * dx_file_find_edit, and dx_file_find_edit_spans, which lists where every occurrence BEGINS beside where it ends.
 *
 * dx_file_find's distance is Hamming's, and the reads these archives hold err by insertion and deletion: an adapter with one inserted
 * base is half its length away from the pattern.  Here the distance is Levenshtein's, the alignment semi-global (the start in the read
 * is free), and a hit is one valley of the distance, reported at its END (dx_code_find_edit, include/dexgpu.h).
 *
 * Only the plan is this file's: a pattern of up to 64 letters becomes one dx_equery, or two with both_strands -- the reverse
 * complement is the codes 3 - c in reverse order, and a pattern that equals its own is searched once --, in the order (pattern,
 * strand).  Everything else is dx_file_find.c's (dxf_find_run): the image's walk, the slices of whole records, the FIND_ROOM retry,
 * the record numbers, the order and max_hits across slices, dxf_find_map.  A strand-1 hit's pos is the end of the reverse complement's
 * occurrence on the read as stored, and its start (dx_file_find_edit_spans) the leftmost symbol of that occurrence.
 */
#include <stdio.h>
#include <string.h>

#include "dexgpu.h"
#include "dx_host.h"
#include "dx_files.h"

/* symbol i of a query: bits 2 (31 - (i & 31)) + 1, 2 (31 - (i & 31)) of code[i >> 5] */
static void put(dx_equery *q, size_t i, int c) { q->code[i >> 5] |= (uint64_t) c << (2 * (31 - (i & 31))); }

int dxf_find_edit_plan(dx_ctx *ctx, int kind, const char *const *pattern, uint32_t npat, uint32_t max_err, int both_strands, find_plan *fp)
{ char     why[160];
  uint32_t p, least = UINT32_MAX;
  memset(fp, 0, sizeof(*fp));
  if (kind == DX_KIND_QUIVA)
    return dx_find_edit_fail(ctx, DX_E_ARG, "a .dexqv image has no packed reads to search (DX_KIND_FASTA or DX_KIND_ARROW)");
  if (kind != DX_KIND_FASTA && kind != DX_KIND_ARROW) return dx_find_edit_fail(ctx, DX_E_ARG, "unknown kind");
  if (both_strands && kind == DX_KIND_ARROW)
    return dx_find_edit_fail(ctx, DX_E_ARG, "both_strands: pulse widths have no complement (DX_KIND_FASTA only)");
  if (pattern == NULL || npat < 1 || npat > (both_strands ? 32u : 64u))
    { snprintf(why, sizeof(why), "%u patterns (1 to %u%s)", npat, both_strands ? 32u : 64u, both_strands ? " with both_strands" : "");
      return dx_find_edit_fail(ctx, DX_E_ARG, why);
    }
  for (p = 0; p < npat; p++)
    { const char *s = pattern[p];
      const size_t len = s ? strlen(s) : 0;
      dx_equery fwd, rev;
      size_t    i;
      if (len < 1 || len > 64)
        { snprintf(why, sizeof(why), "pattern %u has %zu letters (1 to 64)", p, len);
          return dx_find_edit_fail(ctx, DX_E_ARG, why);
        }
      memset(&fwd, 0, sizeof(fwd)); memset(&rev, 0, sizeof(rev));
      fwd.len = rev.len = (uint32_t) len; fwd.max_err = rev.max_err = max_err;
      for (i = 0; i < len; i++)
        { const int c = dxf_find_letter(kind == DX_KIND_ARROW, (unsigned char) s[i]);
          if (c < 0)
            { snprintf(why, sizeof(why), "pattern %u, column %zu: not one of %s", p, i + 1, kind == DX_KIND_ARROW ? "1234" : "acgtACGT");
              return dx_find_edit_fail(ctx, DX_E_ARG, why);
            }
          put(&fwd, i, c);
          put(&rev, len - 1 - i, 3 - c);                     /* letter i is letter len - 1 - i of the reverse */
        }
      if (len < least) least = (uint32_t) len;
      fp->eq[fp->nq] = fwd; fp->pat[fp->nq] = (uint16_t) p; fp->strand[fp->nq] = 0; fp->nq++;
      if (both_strands && (rev.code[0] != fwd.code[0] || rev.code[1] != fwd.code[1]))
        { fp->eq[fp->nq] = rev; fp->pat[fp->nq] = (uint16_t) p; fp->strand[fp->nq] = 1; fp->nq++; }
    }
  if (max_err >= least)
    { snprintf(why, sizeof(why), "%u errors: not below the shortest pattern's %u letters", max_err, least);
      return dx_find_edit_fail(ctx, DX_E_ARG, why);
    }
  return DX_OK;
}

int dx_file_find_edit(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, const char *const *pattern, uint32_t npat, uint32_t max_err,
                      int both_strands, uint64_t max_hits, dx_find *out, dx_hit **hits, uint32_t **rec_hits)
{ find_plan fp;
  int       rc;
  if (ctx == NULL || out == NULL || (img == NULL && m)) return DX_E_ARG;
  if (hits) *hits = NULL;
  if (rec_hits) *rec_hits = NULL;
  if ((rc = dxf_find_edit_plan(ctx, kind, pattern, npat, max_err, both_strands, &fp)) != DX_OK) return rc;
  return dxf_find_run(ctx, kind, img, m, &fp, 1, max_hits, out, hits, rec_hits, NULL, NULL);
}

int dx_file_find_edit_spans(dx_ctx *ctx, int kind, const uint8_t *img, size_t m, const char *const *pattern, uint32_t npat, uint32_t max_err,
                            int both_strands, uint64_t max_hits, dx_find *out, dx_hit **hits, uint32_t **rec_hits, uint32_t **start,
                            uint32_t **rec_len)
{ find_plan fp;
  int       rc;
  if (ctx == NULL || out == NULL || (img == NULL && m)) return DX_E_ARG;
  if (hits) *hits = NULL;
  if (rec_hits) *rec_hits = NULL;
  if (start) *start = NULL;
  if (rec_len) *rec_len = NULL;
  if (start != NULL && hits == NULL) return dx_find_edit_fail(ctx, DX_E_ARG, "the starts stand beside the hits: start without hits");
  if ((rc = dxf_find_edit_plan(ctx, kind, pattern, npat, max_err, both_strands, &fp)) != DX_OK) return rc;
  return dxf_find_run(ctx, kind, img, m, &fp, 1, max_hits, out, hits, rec_hits, start, rec_len);
}
