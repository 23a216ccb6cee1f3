// dx_place_seeds.hip -- the windows of packed reads looked up in a dx_kmer_index (place/dx_kmer_index.hip), every occurrence on the
// reference written out as a SEED: where in the read, where on the reference, which strand.
//
//   dx_code_kmer_seeds   per unit the seeds {unit, pos, gpos, strand}, 16 bytes each, in the order (unit, pos, gpos)   (k_seeds)
//
// Units, windows and codes are dx_code_kmer_codes' with the index's k and canonical; the walk and its three paths are k_screen's
// (screen/dx_screen.hip; the unit's extent and its way to a group's lanes and to the wave are kc_unit_of, kc_unit_from and
// kc_unit_uniform of kmers/dx_kmer_windows.hpp), the look-up is sc_places (screen/dx_screen_look.hpp): SC_BATCH = 8 positions a lane in flight.  A window
// p of unit j whose code stands at place i of the index with count[i] <= max_occ gives, for every r in [start[i], start[i + 1])
// ascending, the seed {j, p, pos[r] >> 1, (pos[r] & 1) ^ f}, f the window's own flip (the code that was looked up is the reverse
// strand's; a second kc_roll over the part gives it, as in k_ix_keys).  A code above max_occ gives none: repeats are dropped by a
// count, not looked at.
//
// The list is made as dx_code_kmer_spans makes its list: the counting launch (k_seeds<.., false>) leaves every unit's seeds (one
// dependent 4-byte load, count[i], a hit), dx_scan_u32 turns the counts into every unit's first place, and the listing launch
// (k_seeds<.., true>) goes over the units that have a seed again.  A lane knows its chunk's seed count, so on the 16-lane and the
// wave path a wave_incl_scan of the chunks' counts inside the unit gives each lane its first place; on the lane path the chunks
// follow each other and nothing is scanned.  Nothing is placed by an atomic cursor: the same bytes on every call.  A seed leaves in
// one 16-byte store.  cap below the seeds writes nothing (DX_E_NOMEM, the totals set all the same): the listing launch never checks
// a place against cap.  A unit of 2^32 seeds or more does not fit its 32-bit count: DX_E_NOMEM names the smallest such unit.
//
// The listing launch REPEATS the look-ups, as k_spans does: once more to count a chunk (16-lane and wave path), and once to write
// it, for the chunks that have a seed.  NOT built: the chunks' counts kept in scratch by the counting launch (units may overlap and
// repeat, so the scratch cannot be kept by buffer position), and per-lane balancing of the writes -- a window whose code occurs
// max_occ times makes its lane write max_occ seeds while its neighbours wait.
//
// ESTIMATE (before the first run; the workload of profiles/screen_rate.txt: 10^5 reads x 10 kb, k = 21 canonical, 10^9 windows).
// The count = dx_code_kmer_depths' gathers without its stores: the screen's time with 1 % of the reads matching (5.8 / 22.9 / 40 ms
// against 4.8 x 10^4 / 5 x 10^6 / 10^8 codes), 1.4 to 1.6 times it when all match (a count gather a hit).  The list with 1 % matching:
// the look-ups of 10^3 reads twice more and 10^7 seeds of 16 bytes, under 1 ms: 1.0 to 1.1 times the screen.  With all matching:
// two more rounds of look-ups, per seed two dependent gathers (start, pos) and one 16-byte store, 10^9 seeds = 16 GB written,
// 4 to 5 ms at HBM's rate but issue-bound at a store a seed as k_kc_codes is (4.65 ms for 10^9 8-byte stores): 3 to 3.5 times
// the screen of the same run, 30 / 110 / 140 ms.
// MEASURED (profiles/place_rate.txt, the same workload, medians of 5 after a warm-up, beside dx_code_kmer_screen against the set
// inside the index in the same run: 5.8 / 22.8 / 41.3 ms with 1 % of the reads matching, 8.5 / 36.9 / 46.7 ms with all).  The count:
// 1.01 to 1.02 times the screen with 1 %, 1.38 to 1.44 times with all, as estimated.  The list (count, prefix sum and listing launch):
// 8.9 / 28.3 / 60.3 ms with 1 %, 1.24 to 1.53 times the screen where 1.0 to 1.1 were estimated -- the look-ups of the matching reads
// are not 1 % of the time, they are the ones that hit; 41.3 / 188.6 / 234.6 ms with all, 4.85 to 5.12 times the screen where 3 to 3.5
// were estimated: three rounds of look-ups in all and two dependent gathers a seed.  Keeping the chunks' counts would take one
// round away.
//
// This file stands outside the evidence set of profiles/ (profiles/check.py hashes csrc/*.hip); its kernels have no entry in the
// profiler's name table and are timed with events on the context's stream (tools/place_rate.py).
#include "screen/dx_screen_look.hpp"
#include "place/dx_kmer_index.hpp"

// what the kernel needs of a dx_kmer_index beside its set
struct ps_index { const uint32_t *count, *start, *pos; uint32_t max_occ; };

// the part's seeds, counted; wins: its windows that give one at least
template <bool CANON>
__device__ __forceinline__ uint64_t ps_count(const kc_part &p, const sc_set &s, const ps_index &x, uint32_t &wins)
{ uint64_t seeds = 0ull;
  wins = 0u;
  if (p.n == 0u) return seeds;
  kc_roll<CANON> r(p, s.k);
  for (uint32_t i0 = 0; i0 < p.n; i0 += SC_BATCH)
    { uint32_t at[SC_BATCH], c[SC_BATCH];
      sc_places<CANON>(r, s, at);
      #pragma unroll
      for (uint32_t t = 0; t < SC_BATCH; t++)
        { c[t] = 0u;
          if (at[t] != SC_NONE && i0 + t < p.n) c[t] = x.count[at[t]];
        }
      #pragma unroll
      for (uint32_t t = 0; t < SC_BATCH; t++)
        if (c[t] != 0u && c[t] <= x.max_occ) { seeds += c[t]; wins++; }
    }
  return seeds;
}

// the part's seeds, written one behind the other from out[0] on; how many there were
template <bool CANON>
__device__ __forceinline__ uint64_t ps_list(const kc_part &p, const sc_set &s, const ps_index &x, uint32_t unit, u32x4_u *out)
{ uint64_t n = 0ull;
  if (p.n == 0u) return n;
  kc_roll<CANON> r(p, s.k), q(p, s.k);                     // r: the look-ups'; q: the same windows once more, for the flip
  for (uint32_t i0 = 0; i0 < p.n; i0 += SC_BATCH)
    { uint32_t at[SC_BATCH], lo[SC_BATCH], hi[SC_BATCH];
      sc_places<CANON>(r, s, at);
      #pragma unroll
      for (uint32_t t = 0; t < SC_BATCH; t++)
        { lo[t] = hi[t] = 0u;
          if (at[t] != SC_NONE && i0 + t < p.n)
            { const uint64_t two = *(const u64_u *) (x.start + at[t]);
              lo[t] = (uint32_t) two; hi[t] = (uint32_t) (two >> 32);
            }
        }
      #pragma unroll
      for (uint32_t t = 0; t < SC_BATCH; t++)
        { uint32_t f = 0u;
          if (CANON)
            { (void) q.code();
              f = q.rcw < (q.w0 >> q.down) ? 1u : 0u;
              q.step();
            }
          if (hi[t] - lo[t] > x.max_occ) continue;
          for (uint32_t at_r = lo[t]; at_r < hi[t]; at_r++)
            { const uint32_t v = x.pos[at_r];
              const u32x4    e = { unit, p.first + i0 + t, v >> 1, (v & 1u) ^ f };
              out[n++] = e;
            }
        }
    }
  return n;
}

// in holds in_bytes bytes and 16 at least; the units are checked against `bound` (as in k_screen).
// LIST false: count (n, or NULL) gets every unit's seeds, saturated at 2^32 - 1 with the unit's number to *big; total: windows,
//   windows with a seed, seeds, units with a seed.
// LIST true: count as the first launch left it, start its exclusive sums (n + 1): the seeds of every unit that has one go to
//   out[start[i] ..).
template <bool CANON, bool LIST>
__global__ __launch_bounds__(DX_BLOCK)
void k_seeds(const uint8_t *__restrict__ in, uint64_t in_bytes, uint64_t bound, const uint64_t *__restrict__ boff,
             const uint32_t *__restrict__ beg, const uint32_t *__restrict__ len, uint64_t n, sc_set s, ps_index x,
             uint32_t *__restrict__ count, const uint64_t *__restrict__ start, u32x4_u *__restrict__ out,
             unsigned long long *__restrict__ total, unsigned long long *__restrict__ big, unsigned long long *__restrict__ bad,
             uint32_t *__restrict__ ticket)
{ __shared__ unsigned long long s_tot[4];
  if (!LIST)
    { if (threadIdx.x < 4u) s_tot[threadIdx.x] = 0ull;
      __syncthreads();
    }

  const uint32_t lane = (uint32_t) lane_id(), sub = lane % UNITS_GROUP, grp = lane / UNITS_GROUP, k = s.k;
  uint64_t t_win = 0, t_hit = 0, t_seed = 0, t_unit = 0;
  // a unit's count leaves: what the list holds of it, the totals, and the unit's number when the count does not fit
  auto leave = [&](uint64_t unit, uint64_t all)
    { t_unit += all ? 1u : 0u;
      if (all > 0xffffffffull) atomicMin(big, (unsigned long long) unit);
      if (count != NULL) count[unit] = all > 0xffffffffull ? 0xffffffffu : (uint32_t) all;
    };
  units_rounds<false>(ticket, ticket_units_of(ticket, KC_BATCH), n, [&](uint64_t u0, uint64_t r1)
    { const uint64_t    i  = u0 + lane;
      const packed_unit pu = packed_unit_take(boff, beg, len, i, r1, bound, bad);
      const kc_unit     e  = kc_unit_of(pu, k);
      uint64_t st = 0;                                     // its first place in the list
      bool     act = i < r1;                               // it is this launch's
      if (!LIST && e.nch) t_win += pu.len - k + 1u;
      if (LIST)
        { st  = i < r1 ? start[i] : 0ull;
          act = i < r1 && e.nch != 0u && count[i] != 0u;
        }

      // no window, or up to KC_LANE chunks: the lane's own, chunk after chunk
      if (act && e.nch <= KC_LANE)
        { uint64_t c = 0;
          for (uint32_t j = 0; j < e.nch; j++)
            { const kc_part p = kc_take(in, in_bytes, e.a0 + 16u * j, e.S0, e.S1, k);
              if (LIST) c += ps_list<CANON>(p, s, x, (uint32_t) i, out + st + c);
              else
                { uint32_t w;
                  c += ps_count<CANON>(p, s, x, w);
                  t_hit += w;
                }
            }
          if (!LIST) { t_seed += c; leave(i, c); }
        }

      // up to 16 chunks: lanes 16 g .. 16 g + 15 take unit k + g, a chunk each
      units_by_fours(__ballot(act && e.nch > KC_LANE && e.nch <= KC_GROUP), [&](int from, bool mine)
        { const kc_unit  g   = kc_unit_from(e, from);
          const uint64_t gst = __shfl(st, from);
          const bool     on  = mine && sub < g.nch;
          kc_part  p = { 0ull, 0ull, 0ull, 0u, 0u };
          uint32_t w = 0u;
          if (on) p = kc_take(in, in_bytes, g.a0 + 16u * sub, g.S0, g.S1, k);
          const uint64_t c = on ? ps_count<CANON>(p, s, x, w) : 0ull;
          if (LIST)
            { const uint32_t incl = wave_incl_scan((uint32_t) c);              // (the unit's seeds fit 32 bits: the host has seen to it)
              const uint32_t low  = __shfl(incl, (int) (grp ? UNITS_GROUP * grp - 1u : 0u));           // what the groups below have
              if (on && c) (void) ps_list<CANON>(p, s, x, (uint32_t) (u0 + (uint64_t) from), out + gst + (incl - (uint32_t) c - (grp ? low : 0u)));
            }
          else
            { const uint64_t all = row_sum64(c);
              t_hit += w; t_seed += c;
              if (mine && sub == 0u) leave(u0 + (uint64_t) from, all);
            }
        });

      // the others: the whole wave, 64 chunks a step
      units_each(__ballot(act && e.nch > KC_GROUP), [&](int from)
        { const kc_unit u = kc_unit_uniform(e, from);
          uint64_t run = uniform64(__shfl(st, from)), mine = 0;           // LIST: the step's first place; else: this lane's seeds
          for (uint32_t base = 0; base < u.nch; base += 64u)
            { const uint32_t j  = base + lane;
              const bool     on = j < u.nch;
              kc_part  p = { 0ull, 0ull, 0ull, 0u, 0u };
              uint32_t w = 0u;
              if (on) p = kc_take(in, in_bytes, u.a0 + 16ull * j, u.S0, u.S1, k);
              const uint64_t c = on ? ps_count<CANON>(p, s, x, w) : 0ull;
              if (LIST)
                { const uint32_t incl = wave_incl_scan((uint32_t) c);
                  if (on && c) (void) ps_list<CANON>(p, s, x, (uint32_t) (u0 + (uint64_t) from), out + run + (incl - (uint32_t) c));
                  run += wave_total(incl);
                }
              else { mine += c; t_hit += w; }
            }
          if (!LIST)
            { const uint64_t all = wave_sum64(mine);
              t_seed += mine;
              if (lane == 0u) leave(u0 + (uint64_t) from, all);
            }
        });
    });

  if (!LIST)
    { if (t_win)  atomicAdd(&s_tot[0], (unsigned long long) t_win);
      if (t_hit)  atomicAdd(&s_tot[1], (unsigned long long) t_hit);
      if (t_seed) atomicAdd(&s_tot[2], (unsigned long long) t_seed);
      if (t_unit) atomicAdd(&s_tot[3], (unsigned long long) t_unit);
      __syncthreads();
      if (threadIdx.x < 4u && s_tot[threadIdx.x] != 0ull) atomicAdd(total + threadIdx.x, s_tot[threadIdx.x]);
    }
}

// ---------------------------------------------------------------------------------------------
//  the entry point
// ---------------------------------------------------------------------------------------------
static_assert(sizeof(dx_seed) == 16, "a seed leaves in one 16-byte store");

#define PS_LAUNCH(CANON, LIST, ...) \
  hipLaunchKernelGGL((k_seeds<CANON, LIST>), dim3(grid), dim3(DX_BLOCK), 0, ctx->stream, d_in, in_bytes, bound, d_boff, d_beg, d_len, n, s, \
                     x, __VA_ARGS__, f.out, f.out + 4, f.bad, f.ticket)

// counted: d_count holds what a counting call over the same arguments left, and only the list is made (total[2] alone is set)
static int seeds_run(dx_ctx *ctx, const char *who, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_boff, const uint32_t *d_beg,
                     const uint32_t *d_len, uint64_t n, const dx_kmer_index *index, uint32_t max_occ, uint32_t *d_count, bool counted,
                     uint64_t *d_off, dx_seed *d_seeds, uint64_t cap, uint64_t total[4], uint64_t *bad_unit)
{ if (ctx == NULL) return DX_E_ARG;
  if (bad_unit) *bad_unit = UINT64_MAX;
  if (total) total[0] = total[1] = total[2] = total[3] = 0;
  if (index == NULL) return dx_fail(ctx, DX_E_ARG, "%s: no index", who);
  if (total == NULL || (d_seeds == NULL && cap)) return dx_fail(ctx, DX_E_ARG, "%s: NULL pointer", who);
  if (max_occ < 1u) return dx_fail(ctx, DX_E_ARG, "%s: max_occ 0 (1 at least: a code that occurs nowhere is in no index)", who);
  if (((uintptr_t) d_seeds & 3u) != 0u || ((uintptr_t) d_count & 3u) != 0u || ((uintptr_t) d_off & 7u) != 0u)
    return dx_fail(ctx, DX_E_ARG, "%s: d_seeds, d_count or d_off is not aligned", who);
  if (n >= (1ull << 31)) return dx_fail(ctx, DX_E_ARG, "%s: more than 2^31 - 1 units in one batch", who);
  if (n == 0)
    { if (d_off == NULL) return DX_OK;
      DX_HIP(ctx, hipSetDevice(ctx->device));
      DX_HIP(ctx, hipMemsetAsync(d_off, 0, 8, ctx->stream));
      DX_HIP(ctx, hipStreamSynchronize(ctx->stream));
      return DX_OK;
    }

  // one scratch block: the frame, the four totals and the unit that is too large, then every unit's first place and the counts
  const dx_kmer_set *set = index->set;
  units_frame    f;
  uint64_t       back[UF_OUT + 5], *d_start = NULL, seeds = 0, large = UINT64_MAX;
  const uint64_t bound = in_bytes;
  const bool     places = cap != 0 || d_off != NULL;
  int rc = units_list_begin(ctx, who, n, d_boff && d_len && (d_in || !in_bytes), 5, 16, places, &d_in, &in_bytes, &f, &d_start, &d_count);
  if (rc != DX_OK) return rc;
  DX_HIP(ctx, hipMemsetAsync(f.out + 4, 0xff, 8, ctx->stream));
  const sc_set   s = sc_set_of(set);
  const ps_index x = { set->d_count, index->d_start, index->d_pos, max_occ };
  const int grid = dx_grid_waves(ctx, n, 16);
  kc_tickets(ctx, d_boff, n, f);
  if (!counted)
    { if (set->canonical) PS_LAUNCH(true, false, d_count, (const uint64_t *) NULL, (u32x4_u *) NULL);
      else                PS_LAUNCH(false, false, d_count, (const uint64_t *) NULL, (u32x4_u *) NULL);
    }
  if (places)
    { if ((rc = units_list_places(ctx, f, d_count, n, d_start, &seeds)) != DX_OK) return rc;
      DX_HIP(ctx, hipMemcpyAsync(&large, f.out + 4, 8, hipMemcpyDeviceToHost, ctx->stream));           // (a count that does not fit: nothing is listed)
      DX_HIP(ctx, hipStreamSynchronize(ctx->stream));
      if (large == UINT64_MAX && (cap == 0 || seeds <= cap))
        { if (d_off) DX_HIP(ctx, hipMemcpyAsync(d_off, d_start, (size_t) (n + 1u) * 8u, hipMemcpyDeviceToDevice, ctx->stream));
          if (cap && seeds)
            { if (set->canonical) PS_LAUNCH(true, true, d_count, (const uint64_t *) d_start, (u32x4_u *) d_seeds);
              else                PS_LAUNCH(false, true, d_count, (const uint64_t *) d_start, (u32x4_u *) d_seeds);
            }
        }
    }
  rc = units_end(ctx, f, back, bad_unit, "%s: unit %llu does not lie inside the %llu packed bytes", bound);
  if (rc != DX_OK && rc != DX_E_FORMAT) return rc;
  for (int t = 0; t < 4; t++) total[t] = back[UF_OUT + t];
  if (counted) total[2] = seeds;
  if (back[UF_OUT + 4] != UINT64_MAX)
    return dx_fail(ctx, DX_E_NOMEM, "%s: unit %llu has 2^32 seeds or more: lower max_occ", who, (unsigned long long) back[UF_OUT + 4]);
  if (cap && total[2] > cap)
    return dx_fail(ctx, DX_E_NOMEM, "%s: %llu seeds, and room for %llu", who, (unsigned long long) total[2], (unsigned long long) cap);
  return rc;
}

extern "C" int dx_code_kmer_seeds(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes,
                                  const uint64_t *d_boff, const uint32_t *d_beg, const uint32_t *d_len, uint64_t n,
                                  const dx_kmer_index *index, uint32_t max_occ, uint32_t *d_count, uint64_t *d_off,
                                  dx_seed *d_seeds, uint64_t cap, uint64_t total[4], uint64_t *bad_unit)
{ return seeds_run(ctx, "dx_code_kmer_seeds", d_in, in_bytes, d_boff, d_beg, d_len, n, index, max_occ, d_count, false, d_off, d_seeds, cap,
                   total, bad_unit);
}

// dx_host.h: the list alone, for dx_file_place.c, which has counted the slice already (to form its groups) and kept the counts
extern "C" int dx_seeds_list_counted(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_boff, const uint32_t *d_len,
                                     uint64_t n, const dx_kmer_index *index, uint32_t max_occ, uint32_t *d_count, uint64_t *d_off,
                                     dx_seed *d_seeds, uint64_t cap, uint64_t *listed)
{ uint64_t t[4];
  if (d_count == NULL || cap == 0) return ctx ? dx_fail(ctx, DX_E_ARG, "dx_seeds_list_counted: no counts, or no list") : DX_E_ARG;
  const int rc = seeds_run(ctx, "dx_code_kmer_seeds", d_in, in_bytes, d_boff, NULL, d_len, n, index, max_occ, d_count, true, d_off, d_seeds, cap,
                           t, NULL);
  if (listed) *listed = t[2];
  return rc;
}
