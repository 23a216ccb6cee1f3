/*
 * find_edit_scan.c -- what answers "where does this pattern END in the reads, within k edits" without dx_file_find_edit: a plain C
 * bit-vector scan (Myers 1999, the semi-global form) of the TEXT undexta -U prints, on one core.  tools/find_edit_rate.py compiles it
 * with -O2 into a shared object and times it behind the GPU unpack of the same image: the baseline the new call is held against.
 *
 *     uint64_t find_edit_scan(const uint8_t *text, size_t n, const char *pattern, uint32_t k, uint64_t *records_hit)
 *
 * text: header lines begin with '>', every other line holds letters of the record (acgtACGT; anything else counts as a).  Returns
 * the hits by the valley rule of include/dexgpu.h (c(e) <= k, c(e) < c(e - 1), c(e) <= c(e + 1), c = min(D, k + 1) and k + 1 at
 * both ends of a record), *records_hit = the records with one.  pattern: 1 to 64 letters.
 */
#include <stddef.h>
#include <stdint.h>
#include <string.h>

uint64_t find_edit_scan(const uint8_t *text, size_t n, const char *pattern, uint32_t k, uint64_t *records_hit)
{ uint64_t peq[256], hits = 0, recs = 0, pv = ~0ull, mv = 0, here = 0;
  const uint32_t m = (uint32_t) strlen(pattern), over = k + 1;
  uint32_t score = m, ca = over, cb = over, i;
  size_t   at = 0;
  static const char low[] = "acgt", up[] = "ACGT";
  uint64_t by_code[4] = { 0, 0, 0, 0 };
  if (m < 1 || m > 64) return 0;
  for (i = 0; i < m; i++)
    { const char *l = strchr(low, pattern[i]), *u = strchr(up, pattern[i]);
      by_code[l && pattern[i] ? l - low : u && pattern[i] ? u - up : 0] |= 1ull << i;
    }
  for (i = 0; i < 256; i++) peq[i] = by_code[0];
  for (i = 0; i < 4; i++) peq[(uint8_t) low[i]] = peq[(uint8_t) up[i]] = by_code[i];

  while (at <= n)
    { if (at == n || text[at] == '>')                      /* a record ends: its last end is a hit if it is the floor of a valley */
        { if (cb <= k && cb < ca) { hits++; here++; }
          recs += here != 0; here = 0;
          pv = ~0ull; mv = 0; score = m; ca = cb = over;
          if (at == n) break;
          while (at < n && text[at] != '\n') at++;
          at++;
          continue;
        }
      if (text[at] == '\n') { at++; continue; }
      { const uint64_t eq = peq[text[at++]], xv = eq | mv, xh = (((eq & pv) + pv) ^ pv) | eq;
        uint64_t ph = mv | ~(xh | pv), mh = pv & xh;
        uint32_t cn;
        score += (uint32_t) ((ph >> (m - 1)) & 1);
        score -= (uint32_t) ((mh >> (m - 1)) & 1);
        ph <<= 1; mh <<= 1;
        pv = mh | ~(xv | ph);
        mv = ph & xv;
        cn = score < over ? score : over;
        if (cb <= k && cb < ca && cb <= cn) { hits++; here++; }
        ca = cb; cb = cn;
      }
    }
  if (records_hit) *records_hit = recs;
  return hits;
}
