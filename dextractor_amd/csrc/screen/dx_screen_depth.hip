// dx_screen_depth.hip -- how often the k-mers of packed reads were seen: every window's count in a COUNTED dx_kmer_set, written out, and
// per read the quantiles of those counts.
//
//   dx_code_kmer_depths   per unit of a .bps / .arw / .dexta / .dexar payload: window p of unit j -> depth[off[j] + p]        (k_depths)
//   dx_depth_stats        per stretch [off[j], off[j + 1]) of such a profile: windows, hits, sum, min, q1, median, q3, max     (k_depth_stats)
//
// A unit, a window and its code are what they are for dx_code_kmer_screen (screen/dx_screen.hip), the places are dx_code_kmer_codes'
// (kmers/dx_kmer_codes.hip): off = the exclusive sums of w_j = max(0, len_j - k + 1), a unit outside the buffer counting 0;
// kc_windows_places (kmers/dx_kmer_windows.hpp: k_kc_windows, dx_scan_u32) states and sums the w_j, and the host holds the total
// against cap before anything is written.  A depth is min(count, 65535) of the window's code, 0 for a code the set does not hold,
// and 1 for every code of an uncounted set.
//
// k_depths.  The walk is kc_walk (kmers/dx_kmer_windows.hpp, which says how it goes): tickets, 64 units a round, a unit of up to
// KC_LANE chunks by its lane, of up to 16 by 16 lanes, the others by the whole wave; what is done with a chunk stands here
// (sd_write), and the unit's first window's place travels with it; kc_take and kc_roll make the codes.  The look-up is sc_places (screen/dx_screen_look.hpp), sc_mask's sibling: SC_BATCH = 8
// positions in flight, the 8 first[] loads asked for before any is waited for, then the buckets' first codes, then the few that need
// more -- and for a code that is found ONE more dependent 4-byte load, count[place], asked for under the lane's own condition so that
// a miss costs no request.
//
// The stores.  A lane's up to 64 windows are up to 128 consecutive bytes of the profile at a 2-byte boundary.  Chosen: the 8 depths
// of a batch are packed into four 32-bit registers (a v_perm or v_lshl_or a pair) and leave in ONE 16-byte store at whatever 2-byte
// boundary they fall (global_store_dwordx4; gfx950 runs with unaligned access), 8 stores a full chunk instead of 64.  The stores of
// a kernel like this one are bound by their ISSUE, not by bytes (k_kc_codes stands at 1.4 times a copy with 8-byte stores), and a
// 16-byte store costs what a 2-byte one does.  The last batch of a part holds p.n mod 8 windows: it leaves as an 8-, a 4- and a 2-byte
// store as the bits of that number say, so that no byte beyond the part's windows is written -- the words behind belong to the next
// chunk's lane, to the next unit, or to nobody (nothing behind depth[windows] is touched).  Turning a wave's 64 x 64 depths in LDS
// for whole 128-byte lines: not built; a line is completed in the L2 by 8 stores of one lane.
//
// Cost a window, counted from the source: the walk's about 10 vector instructions (the code 2, the words' move about 8; canonical + 6),
// the look-up's 9 (the bucket's address 3, the two loads, 2 compares, the place 2), the count's 4 (v_cmp, address 2, the load), the
// clamp 1, the packing 0.5, the store 0.25 with its address: about 25, 31 canonical.
//
// k_depth_stats.  A wave a stretch, drawn by ticket.  The quantiles are EXACT, by two rounds of 256-bin histograms in LDS: the high
// bytes of all values first -- the bins are summed across the wave (4 bins a lane, wave_incl_scan) and each of the three ranks
// (w - 1) / 4, 2 (w - 1) / 4, 3 (w - 1) / 4 finds the bin that holds it and its rank inside --, then the low bytes of the values whose
// high byte is one of those up to three bins, a histogram a DISTINCT bin, all three ranks in the same two sweeps.  3 KiB a wave (the
// round of the high bytes uses the first): one 1-KiB histogram would serve only when the three ranks share their high byte, and a
// third sweep costs more than 2 KiB.  A sweep reads 4 values a lane in one 8-byte load at the stretch's 2-byte boundary, 256 values a
// step, the last few one by one; any w < 2^32.  windows, hits, sum, min and max ride along in the first sweep's registers.  The second
// sweep reads what the first has left in the L2.  Every value is one ds_add; values that share a bin -- a profile whose depths all
// lie below 256 has ONE high byte -- queue on it, 64 lanes deep at the worst.  Short stretches sharing a wave in groups of 16 lanes:
// not built; a stretch of fewer than 256 values leaves lanes idle.  The totals are added up as k_screen adds them: registers, LDS,
// one atomic add a word and workgroup.
//
// ESTIMATE (before the first run; the workload of profiles/screen_rate.txt: 10^5 reads x 10 kb, k = 21 canonical, 10^9 windows).
// dx_code_kmer_depths = dx_code_kmer_screen's gathers + one dependent 4-byte gather a HIT + 2 GB of stores.  The stores: 1.25 x 10^8
// store instructions of 16 bytes against k_kc_codes' 10^9 of 8 bytes in 4.65 ms: 1 to 1.5 ms if issue-bound, hidden in part behind the
// gathers.  With 1 % of the windows in the set the count loads are nothing: 5.75 + 1 = 7 ms against 4.8 x 10^4 codes, 22.6 + 1 = 24 ms
// against 5 x 10^6, 40 + 1 = 41 ms against 10^8.  With all of them in the set there are 10^9 more gathers, from the L2 for the small
// set (+ 2 ms: 10.5 ms), at the Infinity Cache's 45 to 55 G a second for the middle one (+ 20 ms: 56 ms), and from HBM for the large
// one (+ 25 ms: 70 ms): below twice the screen at every size.  dx_depth_stats: 2 x 2 GB read, 1 ms at HBM's rate, but 2 x 10^9 ds_add
// on 256 CUs, and with all depths below 256 every add of the first round on one bin: 64 cycles a wave instruction, 10^9 / 64 x 64 / 256
// CUs = 4 x 10^6 cycles = 1.7 ms, so 3 to 4 ms in all.
// MEASURED (profiles/depth_rate.txt, the same workload, medians of 5 after a warm-up; a device-to-device copy of the profile's 2 GB
// takes 0.79 ms).  dx_code_kmer_depths with 1 % of the windows in the set: 6.45 ms against 4.8 x 10^4 codes (the screen of the same
// run: 5.77), 24.5 ms against 5 x 10^6 (22.8), 42.6 ms against 10^8 (40.0): 1.06 to 1.12 times the screen, the stores and the three
// small launches in front.  With all of them in the set: 12.2 ms (8.43), 55.7 ms (36.0), 73.4 ms (45.5): 1.45, 1.55 and 1.61 times the
// screen, never twice; what is added is the 10^9 dependent count gathers, 20 to 28 ms from the Infinity Cache and from HBM, as
// estimated (the small set's 3.8 ms is above the 2 estimated).  dx_depth_stats: 6.62 ms whatever the set, 0.6 TB/s of its 4 GB -- the
// estimate had 3 to 4.  The depths of this workload are 0 and 1 alone, so in BOTH rounds every ds_add of a wave lands on one or two
// bins: what is measured is the queue on a bin, the worst case, not memory; a profile spread over many bins has not been measured.
// Context.depth of the 1 GB .fasta's image (0.25 GB) against the middle set: 55.8 ms beside Context.screen's 45.9 ms in the same
// run, 14.5 ms of it the host's walk of the image.
//
// This file stands outside the evidence set of profiles/ (profiles/check.py hashes csrc/*.hip); its kernels have no entry in the
// profiler's name table and are timed with events on the context's stream (tools/depth_rate.py).
#include "screen/dx_screen_look.hpp"

extern "C" {
#include "dx_host.h"
}

#define SD_DEPTH_MAX 65535u                   // where a profile's depths saturate
#define SD_BINS      256u                     // bins of a histogram: a byte of the value
#define SD_STEP      256u                     // values a wave takes a step of a sweep: 4 a lane

typedef uint16_t u16_u __attribute__((aligned(1)));

// ---------------------------------------------------------------------------------------------
//  k_depths
// ---------------------------------------------------------------------------------------------
// the part's depths, one behind the other from out[0] on (a 2-byte boundary); count NULL: an uncounted set, 1 a code it holds
template <bool CANON>
__device__ __forceinline__ void sd_write(const kc_part &p, const sc_set &s, const uint32_t *__restrict__ count, uint16_t *out)
{ if (p.n == 0u) return;
  kc_roll<CANON> r(p, s.k);
  for (uint32_t i0 = 0; i0 < p.n; i0 += SC_BATCH)
    { uint32_t at[SC_BATCH], d[SC_BATCH];
      sc_places<CANON>(r, s, at);
      #pragma unroll
      for (uint32_t t = 0; t < SC_BATCH; t++)
        { d[t] = at[t] != SC_NONE ? 1u : 0u;
          if (count != NULL && at[t] != SC_NONE) d[t] = count[at[t]];
        }
      #pragma unroll
      for (uint32_t t = 0; t < SC_BATCH; t++) d[t] = d[t] < SD_DEPTH_MAX ? d[t] : SD_DEPTH_MAX;
      u32x4 e;
      e.x = d[0] | (d[1] << 16); e.y = d[2] | (d[3] << 16); e.z = d[4] | (d[5] << 16); e.w = d[6] | (d[7] << 16);
      uint16_t      *o    = out + i0;
      const uint32_t left = p.n - i0;
      if (left >= SC_BATCH) *(u32x4_u *) o = e;
      else
        { if (left & 4u) { *(u64_u *) o = e.x | ((uint64_t) e.y << 32); o += 4; e.x = e.z; e.y = e.w; }
          if (left & 2u) { *(u32_u *) o = e.x; o += 2; e.x = e.y; }
          if (left & 1u) *(u16_u *) o = (uint16_t) e.x;
        }
    }
}

// in holds in_bytes bytes and 16 at least; the units are checked against `bound` (as in k_kc_codes).  off: the exclusive sums of
// k_kc_windows' counts; depth holds off[n] words at least.
template <bool CANON>
__global__ __launch_bounds__(DX_BLOCK)
void k_depths(const uint8_t *__restrict__ in, uint64_t in_bytes, uint64_t bound, const uint64_t *__restrict__ boff,
              const uint32_t *__restrict__ beg, const uint32_t *__restrict__ len, uint64_t n, sc_set s, const uint32_t *__restrict__ count,
              const uint64_t *__restrict__ off, uint16_t *__restrict__ depth, unsigned long long *__restrict__ bad,
              uint32_t *__restrict__ ticket)
{ const uint32_t lane = (uint32_t) lane_id();
  units_rounds<false>(ticket, ticket_units_of(ticket, KC_BATCH), n, [&](uint64_t u0, uint64_t r1)
    { // unit u0 + lane is this lane's to read and to check; its first window's place travels with it
      const uint64_t    i  = u0 + lane;
      const packed_unit pu = packed_unit_take(boff, beg, len, i, r1, bound, bad);
      const kc_unit     e  = kc_unit_of(pu, s.k);
      const kc_place    at = { e.nch ? off[i] : 0ull, 0u };
      kc_walk(e, at, [&](uint64_t a, const kc_unit &u, const kc_place &to)
        { const kc_part p = kc_take(in, in_bytes, a, u.S0, u.S1, s.k);
          sd_write<CANON>(p, s, count, depth + to.to + p.first);
        });
    });
}

// ---------------------------------------------------------------------------------------------
//  k_depth_stats
// ---------------------------------------------------------------------------------------------
// One sweep of the wave over the w values at v (a 2-byte boundary): take(x) for each, in no order.  A lane's 4 values are one 8-byte
// load where all 4 are the stretch's; the stretch's last few are read one by one, so that nothing behind it is.
template <typename F>
__device__ __forceinline__ void sd_sweep(const uint16_t *__restrict__ v, uint64_t w, uint32_t lane, F &&take)
{ for (uint64_t base = 0; base < w; base += SD_STEP)
    { const uint64_t i = base + 4u * lane;
      if (i + 4u <= w)
        { const uint64_t four = *(const u64_u *) (v + i);
          take((uint32_t) four & 0xffffu); take((uint32_t) (four >> 16) & 0xffffu);
          take((uint32_t) (four >> 32) & 0xffffu); take((uint32_t) (four >> 48));
        }
      else
        for (uint64_t j = i; j < w; j++) take((uint32_t) v[j]);
    }
}

// The bins that hold ranks rank[0 .. 3) of the values counted in h[0 .. 256) (a rank is below their number), and each rank inside
// its bin: every lane gets all six.  A lane sums 4 consecutive bins, the sums are scanned across the wave.
__device__ __forceinline__ void sd_ranks(const uint32_t *h, uint32_t lane, const uint32_t rank[3], uint32_t bin[3], uint32_t inside[3])
{ const u32x4    c    = *(const u32x4 *) (h + 4u * lane);
  const uint32_t sum  = c.x + c.y + c.z + c.w, incl = wave_incl_scan(sum), excl = incl - sum;
  #pragma unroll
  for (uint32_t t = 0; t < 3u; t++)
    { const uint32_t r = rank[t];
      const bool     mine = excl <= r && r < incl;         // (one lane exactly)
      uint32_t b = 0, in = 0;
      if (mine)
        { uint32_t e = excl;
          b = 4u * lane; in = r - e;
          if (in >= c.x) { e += c.x; b++; in = r - e;
            if (in >= c.y) { e += c.y; b++; in = r - e;
              if (in >= c.z) { e += c.z; b++; in = r - e; } } }
        }
      const int from = __ffsll((unsigned long long) __ballot(mine)) - 1;
      bin[t] = uniform((uint32_t) __shfl((int) b, from)); inside[t] = uniform((uint32_t) __shfl((int) in, from));
    }
}

// depth: the profile; off[0 .. n]: the stretches' places, which do not decrease; out: n entries or NULL; total: windows, hits, sum,
// units with a hit.  A stretch that ends in front of its beginning, or holds 2^32 values or more, gets zeros and goes to *bad.
__global__ __launch_bounds__(DX_BLOCK)
void k_depth_stats(const uint16_t *__restrict__ depth, const uint64_t *__restrict__ off, uint64_t n, dx_depth *__restrict__ out,
                   unsigned long long *__restrict__ total, unsigned long long *__restrict__ bad, uint32_t *__restrict__ ticket)
{ __shared__ __attribute__((aligned(16))) uint32_t s_h[DX_WAVES_PER_BLK][3][SD_BINS];
  __shared__ unsigned long long s_tot[4];
  if (threadIdx.x < 4u) s_tot[threadIdx.x] = 0ull;
  __syncthreads();

  const uint32_t lane = (uint32_t) lane_id();
  uint32_t (*h)[SD_BINS] = s_h[threadIdx.x / DX_WAVE];
  uint64_t t_win = 0, t_hit = 0, t_sum = 0, t_unit = 0;    // (the wave's, kept by every lane alike; lane 0 adds them up)
  for (uint64_t j = next_unit(ticket); j < n; j = next_unit(ticket))
    { const uint64_t o0 = uniform64(off[j]), o1 = uniform64(off[j + 1u]);
      const bool     ok = o1 >= o0 && o1 - o0 <= 0xffffffffull;
      const uint64_t w  = ok ? o1 - o0 : 0ull;
      const uint16_t *v = depth + o0;
      if (!ok && lane == 0u) atomicMin(bad, (unsigned long long) j);
      u32x4 e0 = { (uint32_t) w, 0u, 0u, 0u }, e1 = { 0u, 0u, 0u, 0u };
      if (w)
        { // the high bytes, and what rides along
          const u32x4 zero = { 0u, 0u, 0u, 0u };
          *(u32x4 *) (h[0] + 4u * lane) = zero;
          wave_sync();
          uint64_t sum = 0;
          uint32_t hits = 0, mn = SD_DEPTH_MAX, mx = 0;
          sd_sweep(v, w, lane, [&](uint32_t x)
            { atomicAdd(h[0] + (x >> 8), 1u);
              sum += x; hits += x ? 1u : 0u;
              mn = x < mn ? x : mn; mx = x > mx ? x : mx;
            });
          wave_sync();
          sum = wave_sum64(sum); hits = wave_sum(hits);
          #pragma unroll
          for (int d = 32; d > 0; d >>= 1)
            { mn = min(mn, (uint32_t) __shfl_xor((int) mn, d)); mx = max(mx, (uint32_t) __shfl_xor((int) mx, d)); }
          const uint32_t rank[3] = { (uint32_t) ((w - 1u) / 4u), (uint32_t) (2u * (w - 1u) / 4u), (uint32_t) (3u * (w - 1u) / 4u) };
          uint32_t hb[3], in[3], lb[3], rest[3];
          sd_ranks(h[0], lane, rank, hb, in);

          // the low bytes of the values in those bins: a histogram a distinct bin
          wave_sync();                                     // (the bins have been read)
          #pragma unroll
          for (uint32_t t = 0; t < 3u; t++) *(u32x4 *) (h[t] + 4u * lane) = zero;
          wave_sync();
          sd_sweep(v, w, lane, [&](uint32_t x)
            { const uint32_t top = x >> 8;
              if (top == hb[0])      atomicAdd(h[0] + (x & 255u), 1u);
              else if (top == hb[1]) atomicAdd(h[1] + (x & 255u), 1u);
              else if (top == hb[2]) atomicAdd(h[2] + (x & 255u), 1u);
            });
          wave_sync();
          uint32_t q[3];
          #pragma unroll
          for (uint32_t t = 0; t < 3u; t++)
            { const uint32_t slot = hb[t] == hb[0] ? 0u : (hb[t] == hb[1] ? 1u : 2u);
              const uint32_t one[3] = { in[t], in[t], in[t] };
              sd_ranks(h[slot], lane, one, lb, rest);
              q[t] = (hb[t] << 8) | lb[0];
            }
          wave_sync();                                     // (the bins have been read: the next stretch clears them)
          e0.y = hits; e0.z = (uint32_t) sum; e0.w = (uint32_t) (sum >> 32);
          e1.x = mn | (q[0] << 16); e1.y = q[1] | (q[2] << 16); e1.z = mx;
          t_win += w; t_hit += hits; t_sum += sum; t_unit += hits ? 1u : 0u;
        }
      if (out != NULL && lane == 0u)
        { u32x4_u *o = (u32x4_u *) (out + j);                // (two stores at any 4-byte boundary: a driver's d_extra is 8-byte aligned)
          o[0] = e0; o[1] = e1;
        }
    }

  if (lane == 0u)
    { if (t_win)  atomicAdd(&s_tot[0], (unsigned long long) t_win);
      if (t_hit)  atomicAdd(&s_tot[1], (unsigned long long) t_hit);
      if (t_sum)  atomicAdd(&s_tot[2], (unsigned long long) t_sum);
      if (t_unit) atomicAdd(&s_tot[3], (unsigned long long) t_unit);
    }
  __syncthreads();
  if (threadIdx.x < 4u && s_tot[threadIdx.x] != 0ull) atomicAdd(total + threadIdx.x, s_tot[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------
//  the entry points
// ---------------------------------------------------------------------------------------------
static_assert(sizeof(dx_depth) == 32 && sizeof(dx_depth_report) == 56, "an entry is two 16-byte stores");

extern "C" int dx_code_kmer_depths(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes,
                                   const uint64_t *d_boff, const uint32_t *d_beg, const uint32_t *d_len, uint64_t n,
                                   const dx_kmer_set *set, uint16_t *d_depth, uint64_t cap, uint64_t *d_off, uint64_t *windows,
                                   uint64_t *bad_unit)
{ const char *who = "dx_code_kmer_depths";
  if (ctx == NULL) return DX_E_ARG;
  if (bad_unit) *bad_unit = UINT64_MAX;
  if (windows) *windows = 0;
  if (set == NULL) return dx_fail(ctx, DX_E_ARG, "%s: no set", who);
  if (windows == NULL || (d_depth == NULL && cap)) return dx_fail(ctx, DX_E_ARG, "%s: NULL pointer", who);
  if (((uintptr_t) d_depth & 1u) != 0u || ((uintptr_t) d_off & 7u) != 0u) return dx_fail(ctx, DX_E_ARG, "%s: d_depth or d_off is not aligned", who);
  if (n >= (1ull << 31)) return dx_fail(ctx, DX_E_ARG, "%s: more than 2^31 - 1 units in one batch", who);
  if (n == 0)
    { if (d_off == NULL) return DX_OK;
      DX_HIP(ctx, hipSetDevice(ctx->device));
      DX_HIP(ctx, hipMemsetAsync(d_off, 0, 8, ctx->stream));               // (off[0] = the windows = 0)
      DX_HIP(ctx, hipStreamSynchronize(ctx->stream));
      return DX_OK;
    }

  // one scratch block: the frame, then every unit's first place (n + 1) and its windows (n)
  units_frame    f;
  uint64_t       back[UF_OUT + 1], *d_start = NULL, total = 0;
  uint32_t      *d_win = NULL;
  const uint64_t bound = in_bytes;
  int rc = units_list_begin(ctx, who, n, d_boff && d_len && (d_in || !in_bytes), 1, 16, true, &d_in, &in_bytes, &f, &d_start, &d_win);
  if (rc != DX_OK) return rc;
  if ((rc = kc_windows_places(ctx, d_boff, d_beg, d_len, n, bound, set->k, d_win, d_start, &total)) != DX_OK) return rc;
  *windows = total;
  if (total > cap)
    return dx_fail(ctx, DX_E_NOMEM, "%s: %llu windows, and room for %llu depths", who, (unsigned long long) total, (unsigned long long) cap);
  if (d_off) DX_HIP(ctx, hipMemcpyAsync(d_off, d_start, (size_t) (n + 1u) * 8u, hipMemcpyDeviceToDevice, ctx->stream));

  const sc_set s = sc_set_of(set);
  const int grid = dx_grid_waves(ctx, n, 16);
  kc_tickets(ctx, d_boff, n, f);
  if (set->canonical) hipLaunchKernelGGL(k_depths<true>, dim3(grid), dim3(DX_BLOCK), 0, ctx->stream, d_in, in_bytes, bound, d_boff, d_beg, d_len,
                                         n, s, (const uint32_t *) set->d_count, (const uint64_t *) d_start, d_depth, f.bad, f.ticket);
  else                hipLaunchKernelGGL(k_depths<false>, dim3(grid), dim3(DX_BLOCK), 0, ctx->stream, d_in, in_bytes, bound, d_boff, d_beg, d_len,
                                         n, s, (const uint32_t *) set->d_count, (const uint64_t *) d_start, d_depth, f.bad, f.ticket);
  return units_end(ctx, f, back, bad_unit, "%s: unit %llu does not lie inside the %llu packed bytes", bound);
}

extern "C" int dx_depth_stats(dx_ctx *ctx, const uint16_t *d_depth, const uint64_t *d_off, uint64_t n, dx_depth *d_out, uint64_t total[4])
{ const char *who = "dx_depth_stats";
  if (ctx == NULL) return DX_E_ARG;
  if (total) total[0] = total[1] = total[2] = total[3] = 0;
  if (total == NULL) return dx_fail(ctx, DX_E_ARG, "%s: NULL pointer", who);
  if ((((uintptr_t) d_depth) & 1u) != 0u || ((uintptr_t) d_off & 7u) != 0u || ((uintptr_t) d_out & 3u) != 0u)
    return dx_fail(ctx, DX_E_ARG, "%s: d_depth, d_off or d_out is not aligned", who);
  if (n >= (1ull << 31)) return dx_fail(ctx, DX_E_ARG, "%s: more than 2^31 - 1 units in one batch", who);
  if (n == 0) return DX_OK;

  units_frame f;
  uint64_t    back[UF_OUT + 4];
  int rc = units_begin(ctx, who, n, d_depth && d_off, NULL, 4, 0, NULL, NULL, &f);
  if (rc != DX_OK) return rc;
  hipLaunchKernelGGL(k_depth_stats, dim3(dx_grid_waves(ctx, n, 16)), dim3(DX_BLOCK), 0, ctx->stream, d_depth, d_off, n, d_out, f.out, f.bad,
                     f.ticket);
  rc = units_end(ctx, f, back, NULL, "%s: d_off decreases (or leaves 2^32 values or more) behind index %llu", 0);
  if (rc == DX_OK || rc == DX_E_FORMAT)
    for (int t = 0; t < 4; t++) total[t] = back[UF_OUT + t];
  return rc;
}

// dx_host.h: dx_file_depth.c's refusals, worded there
extern "C" int dx_depth_fail(dx_ctx *ctx, int code, const char *what)
{ if (ctx == NULL) return code;
  return dx_fail(ctx, code, "dx_file_depth: %s", what);
}
