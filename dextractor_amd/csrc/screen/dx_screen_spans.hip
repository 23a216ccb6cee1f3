// dx_screen_spans.hip -- WHERE in packed reads the windows that are in a set of k-mers lie, as intervals, and those intervals joined.
//
//   dx_code_kmer_spans   per unit the maximal runs of symbols that lie in a window whose code is in a dx_kmer_set   (k_spans)
//   dx_spans_join        consecutive spans of a record joined across gaps of at most max_gap, the short ones dropped
//                        (k_join_heads, k_join)
//
// Units, windows, codes and the three paths are k_screen's (screen/dx_screen.hip; the unit's extent and its way to a group's lanes
// and to the wave are kc_unit_of, kc_unit_from and kc_unit_uniform of kmers/dx_kmer_windows.hpp); the look-up and the cover word of a chunk are its
// own functions (screen/dx_screen_look.hpp).  What is new is the step from a chunk's cover word D_c (bit j: position j of the chunk
// lies in a hit window) to intervals.  With t = the top bit of D_{c-1} (0 at the unit's first chunk):
//     the begins          B_c = D_c & ~(D_c << 1 | t)
//     the exclusive ends  E_c = ~D_c & (D_c << 1 | t)
// Only symbols of the unit are ever covered, so an end never lies behind the unit's end; the end AT the unit's end is bit S1 - 4 a
// of E_c when the unit ends inside its last chunk, and one end more (sp_edges.last) when it ends with the chunk and bit 63 is set.
// The r-th begin and the r-th end of a unit are one span.  A chunk's first begin has the rank of the begins in the chunks in front
// of it, its first end that rank minus t (the span that is open at the seam ends here first), so a lane writes the begins and the
// ends of ITS chunk without knowing who writes the other half: {record, beg} by one 8-byte and one 4-byte store, end by a 4-byte
// one.  D_{c-1}'s top bit travels as M_{c-1} does: the lane's own word on the lane path, __shfl_up on the other two, a wave-uniform
// carry across the wave path's steps.
//
// The list is in the order (unit, beg) and the same on every call; nothing is placed by an atomic cursor.  The counting launch
// (k_spans<.., false>) leaves every unit's full count (at most len / (k + 1) + 1: it does not saturate), dx_scan_u32 turns the
// counts into every unit's first place, and the listing launch (k_spans<.., true>) goes over the units that have a span and a place
// below cap again, a wave_incl_scan of the chunks' begins giving each lane its first place.  Nothing is written at cap or beyond, and
// a span below cap gets both its halves: the wave path stops only when the places are used up AND no span is open at the seam.
// cap == 0 runs the counting launch alone: one read-back; with a list the scan's total is read back besides, as for dx_code_find.
//
// Which of the two designs: the listing launch REPEATS the look-ups of the units that have a span (k_find's way).  MEASURED
// (profiles/screen_spans_rate.txt, 10^5 reads x 10 kb, k = 21 canonical, 10^9 windows, beside dx_code_kmer_screen in the same run):
// the count alone costs the screen's time at every set size (5.8 / 22.9 / 40.0 ms against 4.8 x 10^4 / 5 x 10^6 / 10^8 codes, 1.00 to
// 1.01 times); with the list 6.8 / 24.7 / 52.9 ms (1.18 / 1.09 / 1.33 times) when 1 % of the reads come from the set's sequence, and
// 16.9 / 71.8 / 90.5 ms when ALL do -- 2.00 times the screen, one whole screen more, as the code says: every unit has a span and
// every look-up is made twice.  A list that MORE than doubled the screen at the 10^8-code set would call for the other form; it
// doubles it and no more (2.0003, inside the rounds' spread).  The other form -- the counting launch leaves the cover words in
// scratch, 8 bytes a chunk, and the listing launch reads them -- is NOT built, so there is no second figure: its scratch cannot be
// kept by buffer position, because units may overlap and repeat, so it wants a scan of the units' chunks in front of the first
// launch and 1/8 of the image's bytes again in scratch; what it could save is the second half of the all-reads-match case.
// dx_spans_join: 0.09 ms up to 10^5 spans (launches and two read-backs), 0.46 ms for 10^7 and 3.7 ms for 10^8 synthetic spans.
//
// dx_spans_join is the run-head pattern of dx_kmer_runs / k_set_take.  Entry i is a HEAD if i == 0, its record is not its
// predecessor's, or beg[i] - end[i - 1] > max_gap; a joined span runs from a head's beg to the end of the entry in front of the next
// head.  k_join_heads checks every entry against its predecessor (beg < end, records not decreasing, end[i - 1] <= beg[i] within a
// record: the smallest index that fails goes back with DX_E_FORMAT) and leaves every tile's first head; k_join works a tile's heads
// out (sj_tile: a thread holds SJ_ITEMS entries, the next head is handed down the workgroup as a suffix minimum, and behind the
// tile's last head the workgroup looks through k_join_heads' words of the tiles that follow, 256 a step -- no lane walks forward
// without bound), counts those with end - beg >= min_span (the filter comes after the join and does not influence it), and, the
// places known from dx_scan_u32 of the tiles' counts, writes them.  Cost: 16 bytes read an entry by each of the three launches and
// one 4-byte gather a head.
//
// This file stands outside the evidence set of profiles/ (profiles/check.py hashes csrc/*.hip); its kernels have no entry in the
// profiler's name table and are timed with events on the context's stream (tools/screen_spans_rate.py).
#include "screen/dx_screen_look.hpp"
#include "tiles/dx_tiles.hpp"

// ---------------------------------------------------------------------------------------------
//  k_spans
// ---------------------------------------------------------------------------------------------
// a chunk's edges: the positions at which a span begins, those that are a span's exclusive end, and (last) one end more at the unit's end
struct sp_edges { uint64_t B, E; uint32_t last; };

// D: the chunk's cover word, t: the top bit of the cover word in front, lim: the unit's end as a position of the chunk (> 64: not here)
__device__ __forceinline__ sp_edges sp_take(uint64_t D, uint32_t t, uint64_t lim)
{ const uint64_t up = (D << 1) | (uint64_t) t;
  sp_edges e;
  e.B = D & ~up; e.E = ~D & up;
  e.last = lim == 64u && (D >> 63) != 0ull ? 1u : 0u;
  return e;
}

// the chunk's halves of the unit's spans: its begins from place `at` on, its ends from at - t on; base = 4 a - S0, none at cap or beyond
__device__ __forceinline__ void sp_list(const sp_edges &e, uint32_t t, uint64_t unit, int64_t base, uint32_t len, dx_span *out,
                                        uint64_t at, uint64_t cap)
{ uint64_t p = at;
  for (uint64_t b = e.B; b; b &= b - 1u, p++)
    if (p < cap)
      { out[p].record = unit;
        out[p].beg = (uint32_t) (base + (int64_t) (__ffsll((unsigned long long) b) - 1));
      }
  p = at - t;                                              // (t == 1: a span began in front of this chunk, at >= 1)
  for (uint64_t x = e.E; x; x &= x - 1u, p++)
    if (p < cap) out[p].end = (uint32_t) (base + (int64_t) (__ffsll((unsigned long long) x) - 1));
  if (e.last && p < cap) out[p].end = len;
}

// in holds in_bytes bytes and 16 at least; the units are checked against `bound` (as in k_screen).
// LIST false: count (n, or NULL) gets every unit's spans; total: spans, covered symbols, units with a span.
// LIST true: count as the first launch left it, start its exclusive sums (n + 1): the spans of every unit that has one and a place
//   below cap go to out[start[i] ..), none at cap or beyond.
template <bool CANON, bool LIST>
__global__ __launch_bounds__(DX_BLOCK)
void k_spans(const uint8_t *__restrict__ in, uint64_t in_bytes, uint64_t bound, const uint64_t *__restrict__ boff,
             const uint32_t *__restrict__ beg, const uint32_t *__restrict__ len, uint64_t n, sc_set s,
             uint32_t *__restrict__ count, const uint64_t *__restrict__ start, dx_span *__restrict__ out, uint64_t cap,
             unsigned long long *__restrict__ total, unsigned long long *__restrict__ bad, uint32_t *__restrict__ ticket)
{ __shared__ unsigned long long s_tot[3];
  if (!LIST)
    { if (threadIdx.x < 3u) s_tot[threadIdx.x] = 0ull;
      __syncthreads();
    }

  const uint32_t lane = (uint32_t) lane_id(), sub = lane % UNITS_GROUP, grp = lane / UNITS_GROUP, k = s.k;
  const sp_edges none = { 0ull, 0ull, 0u };
  uint64_t t_span = 0, t_cov = 0, t_unit = 0;
  units_rounds<false>(ticket, ticket_units_of(ticket, KC_BATCH), n, [&](uint64_t u0, uint64_t r1)
    { // unit u0 + lane is this lane's to read and to check
      const uint64_t    i  = u0 + lane;
      const packed_unit pu = packed_unit_take(boff, beg, len, i, r1, bound, bad);
      const kc_unit     U  = kc_unit_of(pu, k);
      uint64_t st = 0;                                     // its first place in the list
      bool     act = i < r1;                               // it is this launch's
      if (LIST)
        { st  = i < r1 ? start[i] : 0ull;
          act = i < r1 && U.nch != 0u && count[i] != 0u && st < cap;
        }

      // no window (too short, or not in the buffer), or up to KC_LANE chunks: the lane's own, chunk after chunk
      if (act && U.nch <= KC_LANE)
        { uint64_t prev = 0ull, at = st;
          uint32_t t = 0u, c = 0u, cov = 0u;
          for (uint32_t j = 0; j < U.nch; j++)
            { const uint64_t a = U.a0 + 16u * j, m = sc_chunk_mask<CANON>(in, in_bytes, a, U.S0, U.S1, s);
              const uint64_t D = sc_cover(m, prev, k);
              const sp_edges e = sp_take(D, t, U.S1 - 4u * a);
              const uint32_t nb = (uint32_t) __popcll((unsigned long long) e.B);
              if (LIST)
                { sp_list(e, t, i, (int64_t) (4u * a) - (int64_t) U.S0, (uint32_t) (U.S1 - U.S0), out, at, cap);
                  at += nb;
                }
              else { c += nb; cov += (uint32_t) __popcll((unsigned long long) D); }
              prev = m; t = (uint32_t) (D >> 63);
            }
          if (!LIST)
            { t_span += c; t_cov += cov; t_unit += c ? 1u : 0u;
              if (count != NULL) count[i] = c;
            }
        }

      // up to 16 chunks: lanes 16 g .. 16 g + 15 take unit k + g, a chunk each
      units_by_fours(__ballot(act && U.nch > KC_LANE && U.nch <= KC_GROUP), [&](int from, bool mine)
        { const kc_unit  g   = kc_unit_from(U, from);
          const uint64_t gst = __shfl(st, from);
          const bool     on  = mine && sub < g.nch;
          const uint64_t a   = g.a0 + 16u * sub;
          const uint64_t m   = on ? sc_chunk_mask<CANON>(in, in_bytes, a, g.S0, g.S1, s) : 0ull;
          const uint64_t upm = (uint64_t) __shfl_up((unsigned long long) m, 1u);
          const uint64_t D   = on ? sc_cover(m, sub ? upm : 0ull, k) : 0ull;
          const uint64_t upd = (uint64_t) __shfl_up((unsigned long long) D, 1u);
          const uint32_t t   = sub ? (uint32_t) (upd >> 63) : 0u;
          const sp_edges e   = on ? sp_take(D, t, g.S1 - 4u * a) : none;
          const uint32_t nb  = (uint32_t) __popcll((unsigned long long) e.B);
          if (LIST)
            { const uint32_t incl = wave_incl_scan(nb);
              const uint32_t low  = __shfl(incl, (int) (grp ? UNITS_GROUP * grp - 1u : 0u));           // what the groups below have
              if (on) sp_list(e, t, u0 + (uint64_t) from, (int64_t) (4u * a) - (int64_t) g.S0, (uint32_t) (g.S1 - g.S0), out,
                              gst + (incl - nb - (grp ? low : 0u)), cap);
            }
          else
            { const uint32_t all = row_sum(nb);
              t_span += nb; t_cov += (uint32_t) __popcll((unsigned long long) D);
              if (mine && sub == UNITS_GROUP - 1u)
                { t_unit += all ? 1u : 0u;
                  if (count != NULL) count[u0 + (uint64_t) from] = all;
                }
            }
        });

      // the others: the whole wave, 64 chunks a step
      units_each(__ballot(act && U.nch > KC_GROUP), [&](int from)
        { const kc_unit  w   = kc_unit_uniform(U, from);
          uint64_t run = uniform64(__shfl(st, from)), mine = 0;           // LIST: the step's first place; else: this lane's spans
          uint64_t carry = 0ull;                                         // lane 63's mask of the step before (wave-uniform)
          uint32_t open = 0u;                                            // ... and the top bit of its cover word
          for (uint32_t base = 0; base < w.nch; base += 64u)
            { const uint32_t j  = base + lane;
              const bool     on = j < w.nch;
              const uint64_t a   = w.a0 + 16ull * j;
              const uint64_t m   = on ? sc_chunk_mask<CANON>(in, in_bytes, a, w.S0, w.S1, s) : 0ull;
              const uint64_t upm = (uint64_t) __shfl_up((unsigned long long) m, 1u);
              const uint64_t D   = on ? sc_cover(m, lane ? upm : carry, k) : 0ull;
              const uint64_t upd = (uint64_t) __shfl_up((unsigned long long) D, 1u);
              const uint32_t t   = lane ? (uint32_t) (upd >> 63) : open;
              const sp_edges e   = on ? sp_take(D, t, w.S1 - 4u * a) : none;
              const uint32_t nb  = (uint32_t) __popcll((unsigned long long) e.B);
              carry = uniform64((uint64_t) __shfl((unsigned long long) m, 63));
              open  = uniform((uint32_t) __shfl((int) (uint32_t) (D >> 63), 63));
              if (LIST)
                { const uint32_t incl = wave_incl_scan(nb);
                  if (on) sp_list(e, t, u0 + (uint64_t) from, (int64_t) (4u * a) - (int64_t) w.S0, (uint32_t) (w.S1 - w.S0), out,
                                  run + (incl - nb), cap);
                  run += wave_total(incl);
                  if (run >= cap + open) break;                          // (a span that is open at the seam still wants its end)
                }
              else { mine += nb; t_cov += (uint32_t) __popcll((unsigned long long) D); }
            }
          if (!LIST)
            { const uint64_t all = wave_sum64(mine);
              t_span += mine;
              if (lane == 0u)
                { t_unit += all ? 1u : 0u;
                  if (count != NULL) count[u0 + (uint64_t) from] = (uint32_t) all;
                }
            }
        });
    });

  if (!LIST)
    { if (t_span) atomicAdd(&s_tot[0], (unsigned long long) t_span);
      if (t_cov)  atomicAdd(&s_tot[1], (unsigned long long) t_cov);
      if (t_unit) atomicAdd(&s_tot[2], (unsigned long long) t_unit);
      __syncthreads();
      if (threadIdx.x < 3u && s_tot[threadIdx.x] != 0ull) atomicAdd(total + threadIdx.x, s_tot[threadIdx.x]);
    }
}

// ---------------------------------------------------------------------------------------------
//  the entry point
// ---------------------------------------------------------------------------------------------
static_assert(sizeof(dx_span) == 16 && sizeof(dx_spans_report) == 72, "a span is 16 bytes: the join loads it whole");

// counted: d_count holds what a counting call over the same arguments left, and only the list is made (total[0] alone is set)
static int spans_run(dx_ctx *ctx, const char *who, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_boff, const uint32_t *d_beg,
                     const uint32_t *d_len, uint64_t n, const dx_kmer_set *set, uint32_t *d_count, bool counted, dx_span *d_spans,
                     uint64_t cap, uint64_t total[3], uint64_t *bad_unit)
{ if (ctx == NULL) return DX_E_ARG;
  if (bad_unit) *bad_unit = UINT64_MAX;
  if (total) total[0] = total[1] = total[2] = 0;
  if (set == NULL) return dx_fail(ctx, DX_E_ARG, "%s: no set", who);
  if (total == NULL || (d_spans == NULL && cap)) return dx_fail(ctx, DX_E_ARG, "%s: NULL pointer", who);
  if (((uintptr_t) d_spans & 7u) != 0u) return dx_fail(ctx, DX_E_ARG, "%s: d_spans is not 8-byte aligned", who);
  if (((uintptr_t) d_count & 3u) != 0u) return dx_fail(ctx, DX_E_ARG, "%s: d_count is not 4-byte aligned", who);
  if (cap > 0xffffffffull) return dx_fail(ctx, DX_E_ARG, "%s: a list of more than 2^32 - 1 spans", who);
  if (n >= (1ull << 31)) return dx_fail(ctx, DX_E_ARG, "%s: more than 2^31 - 1 units in one batch", who);
  if (n == 0) return DX_OK;

  // one scratch block: the frame and the three totals, then (with a list) every unit's first place, and the counts nobody asked for
  units_frame    f;
  uint64_t       back[UF_OUT + 3], *d_start = NULL;
  const uint64_t bound = in_bytes;
  int rc = units_list_begin(ctx, who, n, d_boff && d_len && (d_in || !in_bytes), 3, 16, cap != 0, &d_in, &in_bytes, &f, &d_start, &d_count);
  if (rc != DX_OK) return rc;
  const sc_set s = sc_set_of(set);
  const int grid = dx_grid_waves(ctx, n, 16);
  kc_tickets(ctx, d_boff, n, f);
  if (!counted)
    { if (set->canonical) hipLaunchKernelGGL((k_spans<true, false>), dim3(grid), dim3(DX_BLOCK), 0, ctx->stream, d_in, in_bytes, bound, d_boff,
                                             d_beg, d_len, n, s, d_count, (const uint64_t *) NULL, (dx_span *) NULL, cap, f.out, f.bad, f.ticket);
      else                hipLaunchKernelGGL((k_spans<false, false>), dim3(grid), dim3(DX_BLOCK), 0, ctx->stream, d_in, in_bytes, bound, d_boff,
                                             d_beg, d_len, n, s, d_count, (const uint64_t *) NULL, (dx_span *) NULL, cap, f.out, f.bad, f.ticket);
    }
  uint64_t spans = 0;
  if (cap)
    { if ((rc = units_list_places(ctx, f, d_count, n, d_start, &spans)) != DX_OK) return rc;
      if (spans)
        { if (set->canonical) hipLaunchKernelGGL((k_spans<true, true>), dim3(grid), dim3(DX_BLOCK), 0, ctx->stream, d_in, in_bytes, bound,
                                                 d_boff, d_beg, d_len, n, s, d_count, (const uint64_t *) d_start, d_spans, cap,
                                                 (unsigned long long *) NULL, f.bad, f.ticket);
          else                hipLaunchKernelGGL((k_spans<false, true>), dim3(grid), dim3(DX_BLOCK), 0, ctx->stream, d_in, in_bytes, bound,
                                                 d_boff, d_beg, d_len, n, s, d_count, (const uint64_t *) d_start, d_spans, cap,
                                                 (unsigned long long *) NULL, f.bad, f.ticket);
        }
    }
  rc = units_end(ctx, f, back, bad_unit, "%s: unit %llu does not lie inside the %llu packed bytes", bound);
  if (rc == DX_OK || rc == DX_E_FORMAT)
    { for (int t = 0; t < 3; t++) total[t] = back[UF_OUT + t];
      if (counted) total[0] = spans;
    }
  return rc;
}

extern "C" int dx_code_kmer_spans(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes,
                                  const uint64_t *d_boff, const uint32_t *d_beg, const uint32_t *d_len, uint64_t n,
                                  const dx_kmer_set *set, uint32_t *d_count, dx_span *d_spans, uint64_t cap, uint64_t total[3],
                                  uint64_t *bad_unit)
{ return spans_run(ctx, "dx_code_kmer_spans", d_in, in_bytes, d_boff, d_beg, d_len, n, set, d_count, false, d_spans, cap, total, bad_unit);
}

// dx_host.h: the list alone, for dx_file_screen_spans.c, which has counted the slice already (to size the list) and kept the counts
extern "C" int dx_spans_list_counted(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_boff, const uint32_t *d_len,
                                     uint64_t n, const dx_kmer_set *set, uint32_t *d_count, dx_span *d_spans, uint64_t cap, uint64_t *listed)
{ uint64_t t[3];
  if (d_count == NULL || cap == 0) return ctx ? dx_fail(ctx, DX_E_ARG, "dx_spans_list_counted: no counts, or no list") : DX_E_ARG;
  const int rc = spans_run(ctx, "dx_code_kmer_spans", d_in, in_bytes, d_boff, NULL, d_len, n, set, d_count, true, d_spans, cap, t, NULL);
  if (listed) *listed = t[0];
  return rc;
}

// ---------------------------------------------------------------------------------------------
//  k_join_heads, k_join
// ---------------------------------------------------------------------------------------------
#define SJ_ITEMS 8u                           // entries a thread
#define SJ_TILE  (DX_BLOCK * SJ_ITEMS)        // entries a workgroup
#define SJ_NONE  0xffffffffu
#define SJ_NMAX  (1ull << 36)

// an entry as it is loaded: x, y = the record, z = beg, w = end
__device__ __forceinline__ uint64_t sj_record(const u32x4 &v) { return (uint64_t) v.x | ((uint64_t) v.y << 32); }
// entry v behind entry p begins a joined span
__device__ __forceinline__ bool sj_head(const u32x4 &p, const u32x4 &v, uint32_t max_gap)
{ return sj_record(v) != sj_record(p) || v.z - p.w > max_gap; }

// the smallest value over the workgroup (every thread gets it); s_w: a word a wave
__device__ __forceinline__ uint32_t sj_block_min(uint32_t v, uint32_t *s_w)
{
  #pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = min(v, (uint32_t) __shfl_xor((int) v, d));
  __syncthreads();                                         // (s_w may still be read from its last use)
  if (lane_id() == 0) s_w[threadIdx.x / DX_WAVE] = v;
  __syncthreads();
  return min(min(s_w[0], s_w[1]), min(s_w[2], s_w[3]));
}

// first[t] = the place in tile t of its first head, SJ_NONE if it has none; bad: the smallest index of an entry that breaks the order
__global__ __launch_bounds__(DX_BLOCK)
void k_join_heads(const u32x4_u *__restrict__ in, uint64_t n, uint32_t max_gap, uint32_t *__restrict__ first,
                  unsigned long long *__restrict__ bad)
{ __shared__ uint32_t s_w[DX_WAVES_PER_BLK];
  const uint64_t i0 = (uint64_t) blockIdx.x * SJ_TILE + (uint64_t) SJ_ITEMS * threadIdx.x;
  uint32_t mine = SJ_NONE;
  if (i0 < n)
    { u32x4 prev = in[i0 ? i0 - 1u : 0u];
      #pragma unroll
      for (uint32_t j = 0; j < SJ_ITEMS; j++)
        if (i0 + j < n)
          { const u32x4 v = in[i0 + j];
            const bool  f = i0 + j != 0u;                  // it has a predecessor
            if (v.z >= v.w || (f && (sj_record(v) < sj_record(prev) || (sj_record(v) == sj_record(prev) && v.z < prev.w))))
              atomicMin(bad, (unsigned long long) (i0 + j));
            if ((!f || sj_head(prev, v, max_gap)) && mine == SJ_NONE) mine = SJ_ITEMS * threadIdx.x + j;
            prev = v;
          }
    }
  const uint32_t all = sj_block_min(mine, s_w);
  if (threadIdx.x == 0u) first[blockIdx.x] = all;
}

// Tile t's entries, 8 a thread: v[j] = entry SJ_TILE t + 8 x + j, end[j] = where the joined span that begins there ends, 0 where none
// does (a span has a symbol at least: its end is not 0).  Uniform over the workgroup (it synchronises); s_f: a word a thread, s_w: a
// word a wave.
__device__ __forceinline__ void sj_tile(const u32x4_u *__restrict__ in, uint64_t n, const uint32_t *__restrict__ first, uint64_t tiles,
                                        uint64_t t, uint32_t max_gap, uint32_t *s_f, uint32_t *s_w, u32x4 v[SJ_ITEMS], uint32_t end[SJ_ITEMS])
{ const uint64_t t0 = t * SJ_TILE, i0 = t0 + (uint64_t) SJ_ITEMS * threadIdx.x;
  const u32x4 zero = { 0u, 0u, 0u, 0u };
  bool     head[SJ_ITEMS];
  uint32_t mine = SJ_NONE;                                 // this thread's first head, as a place in the tile
  u32x4    prev = i0 && i0 < n ? in[i0 - 1u] : zero;
  #pragma unroll
  for (uint32_t j = 0; j < SJ_ITEMS; j++)
    { const bool have = i0 + j < n;
      v[j] = have ? in[i0 + j] : zero;
      head[j] = have && (i0 + j == 0u || sj_head(prev, v[j], max_gap));
      if (head[j] && mine == SJ_NONE) mine = SJ_ITEMS * threadIdx.x + j;
      prev = v[j];
    }

  // the first head behind the tile: in the tiles that follow, 256 of them a step; n if there is none.  (A tile without a head has
  // nothing to end: first[t] is the workgroup's, so the branch is uniform.)
  uint64_t beyond = n;
  if (first[t] != SJ_NONE)
    for (uint64_t b = t + 1u; b < tiles; b += DX_BLOCK)
      { const uint64_t u = b + threadIdx.x;
        const uint32_t f = u < tiles ? first[u] : SJ_NONE;
        const uint32_t w = sj_block_min(f != SJ_NONE ? threadIdx.x : SJ_NONE, s_w);                  // the nearest such tile of the 256
        if (w != SJ_NONE)
          { beyond = (b + w) * SJ_TILE + first[b + w];
            break;                                                                                   // (uniform: w is the workgroup's)
          }
      }

  // the first head behind this thread's entries: the smallest of the threads above it
  __syncthreads();
  s_f[threadIdx.x] = mine;
  __syncthreads();
  const uint32_t lane = (uint32_t) lane_id(), wave = threadIdx.x / DX_WAVE;
  uint32_t after = lane < 63u ? s_f[threadIdx.x + 1u] : SJ_NONE;                                  // the wave's lanes above, suffix minimum
  #pragma unroll
  for (uint32_t d = 1; d < 64u; d <<= 1)
    { const uint32_t o = (uint32_t) __shfl_down((int) after, d);
      if (lane + d < 64u) after = min(after, o);
    }
  const uint32_t whole = min(after, mine);                                                       // the wave's first head, in lane 0
  if (lane == 0u) s_w[wave] = whole;
  __syncthreads();
  for (uint32_t w = wave + 1u; w < DX_WAVES_PER_BLK; w++) after = min(after, s_w[w]);
  uint64_t next = after != SJ_NONE ? t0 + after : beyond;
  #pragma unroll
  for (uint32_t jj = 0; jj < SJ_ITEMS; jj++)
    { const uint32_t j = SJ_ITEMS - 1u - jj;
      end[j] = 0u;
      if (head[j])
        { end[j] = next == i0 + j + 1u ? v[j].w : ((const uint32_t *) in)[4u * (next - 1u) + 3u];             // (next - 1 < n: an entry of the list)
          next = i0 + j;
        }
    }
  __syncthreads();                                         // (s_f, s_w: free again)
}

// LIST false: pass[t] = tile t's joined spans of min_span symbols at least; total: those, their symbols.
// LIST true: start = the exclusive sums of pass; they are written from out[start[t]] on, none at cap or beyond.
template <bool LIST>
__global__ __launch_bounds__(DX_BLOCK)
void k_join(const u32x4_u *__restrict__ in, uint64_t n, const uint32_t *__restrict__ first, uint64_t tiles, uint32_t max_gap,
            uint32_t min_span, uint32_t *__restrict__ pass, const uint64_t *__restrict__ start, u32x4_u *__restrict__ out, uint64_t cap,
            unsigned long long *__restrict__ total)
{ __shared__ uint32_t           s_f[DX_BLOCK], s_w[DX_WAVES_PER_BLK], s_n[DX_WAVES_PER_BLK];
  __shared__ unsigned long long s_s[DX_WAVES_PER_BLK];
  const uint64_t t = blockIdx.x;
  uint64_t from = 0;
  if (LIST)
    { from = start[t];
      if (from >= cap || start[t + 1u] == from) return;                        // (uniform: the whole workgroup leaves)
    }
  u32x4    v[SJ_ITEMS];
  uint32_t end[SJ_ITEMS];
  sj_tile(in, n, first, tiles, t, max_gap, s_f, s_w, v, end);
  uint32_t mine = 0;
  uint64_t sym = 0;
  #pragma unroll
  for (uint32_t j = 0; j < SJ_ITEMS; j++)
    if (end[j] && end[j] - v[j].z >= min_span) { mine++; sym += end[j] - v[j].z; }
  const uint32_t incl = wave_incl_scan(mine), wave = threadIdx.x / DX_WAVE;
  if (LIST)
    { if (lane_id() == 63) s_n[wave] = incl;
      __syncthreads();
      uint64_t at = from + (incl - mine);
      for (uint32_t w = 0; w < wave; w++) at += s_n[w];
      #pragma unroll
      for (uint32_t j = 0; j < SJ_ITEMS; j++)
        if (end[j] && end[j] - v[j].z >= min_span)
          { if (at < cap)
              { u32x4 e = v[j];
                e.w = end[j];
                out[at] = e;
              }
            at++;
          }
    }
  else
    { const uint64_t all = wave_sum64(sym);
      if (lane_id() == 63) { s_n[wave] = incl; s_s[wave] = all; }
      __syncthreads();
      if (threadIdx.x == 0u)
        { const uint32_t c = s_n[0] + s_n[1] + s_n[2] + s_n[3];
          pass[t] = c;
          if (c)
            { atomicAdd(total, (unsigned long long) c);
              atomicAdd(total + 1, s_s[0] + s_s[1] + s_s[2] + s_s[3]);
            }
        }
    }
}

extern "C" int dx_spans_join(dx_ctx *ctx, const dx_span *d_in, uint64_t n, uint32_t max_gap, uint32_t min_span,
                             dx_span *d_out, uint64_t cap, uint64_t total[2], uint64_t *bad)
{ if (ctx == NULL) return DX_E_ARG;
  if (bad) *bad = UINT64_MAX;
  if (total) total[0] = total[1] = 0;
  if (total == NULL || (d_in == NULL && n) || (d_out == NULL && cap)) return dx_fail(ctx, DX_E_ARG, "dx_spans_join: NULL pointer");
  if ((((uintptr_t) d_in | (uintptr_t) d_out) & 7u) != 0u) return dx_fail(ctx, DX_E_ARG, "dx_spans_join: a list is not 8-byte aligned");
  if (cap > 0xffffffffull) return dx_fail(ctx, DX_E_ARG, "dx_spans_join: a list of more than 2^32 - 1 spans");
  if (n >= SJ_NMAX) return dx_fail(ctx, DX_E_ARG, "dx_spans_join: %llu spans (fewer than 2^36)", (unsigned long long) n);
  if (n && cap && (uintptr_t) d_out < (uintptr_t) (d_in + n) && (uintptr_t) d_in < (uintptr_t) (d_out + cap))
    return dx_fail(ctx, DX_E_ARG, "dx_spans_join: d_out overlaps d_in");
  if (n == 0) return DX_OK;
  DX_HIP(ctx, hipSetDevice(ctx->device));
  int rc = dx_after_pending(ctx);
  if (rc != DX_OK) return rc;

  // in front of the tiles' words: the smallest bad index and the two totals
  const uint64_t tiles = (n + SJ_TILE - 1u) / SJ_TILE;
  uint64_t       back[3], found = 0;
  tiles_layout   l;
  bool           list = false;
  if ((rc = tiles_scratch(ctx, 3, tiles, true, &l)) != DX_OK) return rc;
  DX_HIP(ctx, hipMemsetAsync(l.head, 0xff, 8, ctx->stream));
  DX_HIP(ctx, hipMemsetAsync(l.head + 1, 0, 16, ctx->stream));
  hipLaunchKernelGGL(k_join_heads, dim3((unsigned) tiles), dim3(DX_BLOCK), 0, ctx->stream, (const u32x4_u *) d_in, n, max_gap, l.first,
                     (unsigned long long *) l.head);
  hipLaunchKernelGGL(k_join<false>, dim3((unsigned) tiles), dim3(DX_BLOCK), 0, ctx->stream, (const u32x4_u *) d_in, n,
                     (const uint32_t *) l.first, tiles, max_gap, min_span, l.pass, (const uint64_t *) NULL, (u32x4_u *) NULL, cap,
                     (unsigned long long *) (l.head + 1));
  if ((rc = tiles_places(ctx, l, tiles, cap, &found, &list)) != DX_OK) return rc;
  if (list)
    { hipLaunchKernelGGL(k_join<true>, dim3((unsigned) tiles), dim3(DX_BLOCK), 0, ctx->stream, (const u32x4_u *) d_in, n,
                         (const uint32_t *) l.first, tiles, max_gap, min_span, (uint32_t *) NULL, (const uint64_t *) l.start,
                         (u32x4_u *) d_out, cap, (unsigned long long *) NULL);
      DX_HIP(ctx, hipGetLastError());
    }
  DX_HIP(ctx, hipMemcpyAsync(back, l.head, 24, hipMemcpyDeviceToHost, ctx->stream));
  DX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (back[0] != UINT64_MAX)
    { if (bad) *bad = back[0];
      return dx_fail(ctx, DX_E_FORMAT, "dx_spans_join: span %llu has no symbol, or does not follow the span in front of it", (unsigned long long) back[0]);
    }
  total[0] = back[1]; total[1] = back[2];
  return DX_OK;
}

// dx_host.h: dx_file_screen_spans.c's refusals, worded there
extern "C" int dx_screen_spans_fail(dx_ctx *ctx, int code, const char *who, const char *what)
{ if (ctx == NULL) return code;
  return dx_fail(ctx, code, "%s: %s", who, what);
}
