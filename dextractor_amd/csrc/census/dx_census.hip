// dx_census.hip -- what a batch of packed reads or of decoded lines holds, counted where it lies.
//
//   dx_code_counts       per unit of a .bps / .arw / .dexta / .dexar payload: how many symbols have code 0, 1, 2, 3  (k_code_counts)
//   dx_byte_hist_ranges  byte-value histograms (one table a kind) and byte sums of ranges of a buffer               (k_byte_hist)
//
// The reference counts on one core as it adds reads to a database: dex2DB.c:587-595 and :793-797 (count[4], totlen, maxlen),
// folded into DAZZ_DB.freq / .totlen / .maxlen at :896-913.  Nothing is decoded here, and nothing is written but the counts.
// Roofline of both kernels: HBM, what they read.
//
// k_code_counts.  A unit is what it is for dx_reads_unpack: symbols [beg, beg + len) of the packed read at in + boff, symbol i in
// byte i >> 2 at bits 7 - 2 (i & 3), 6 - 2 (i & 3).  The waves draw tickets (k_ticket_units) and take a ticket's units 64 at a
// time, a lane reading one unit's parameters and checking its bounds.  The unit is then walked in chunks of 16 packed bytes that
// stand on 16-byte boundaries of the buffer (the first may begin in front of the unit, the last end behind it), and
//   * a unit that has one chunk is its lane's;
//   * one of up to 16 chunks goes FOUR A STEP, a group of 16 lanes each, the group's counts summed along its row;
//   * the others go one after the other by the whole wave, 1 KiB a step, the next step's bytes asked for before this step's are
//     counted, wave_sum at the unit's end.
// A chunk's counts are popcounts of bit planes: with h the words' odd bits moved onto the even ones and l the even ones, under
// the mask m of the even bits whose symbol is the unit's, popc(h & m), popc(l & m) and popc(h & l & m) give the four codes'
// counts (3: both, 2: h alone, 1: l alone, 0: the rest of popc(m)); no loop goes round per symbol.  The pad bits behind a
// read's last symbol and the symbols in front of beg lie outside m.  A chunk inside the unit (all but two) needs no mask and no
// byte swap, and its four words are counted as two of 64 bits.
// Nothing outside [0, in_bytes) is read: the 16 bytes that would reach past the buffer's end are its last 16, and the mask is
// moved with them (a buffer of fewer than 16 bytes is copied into 16 first).  A unit that does not lie inside the buffer is not
// counted; the smallest such index goes back to the host with the totals, one read-back a call.
// Totals: a lane keeps what it has stored in four 64-bit registers, the workgroup adds them up in LDS at the kernel's end and
// adds its four sums to the global words, one vector atomicAdd each.
//
// k_byte_hist.  Range j's bytes are counted in table kind[j] (of nkinds <= 8 tables of 256), their sum goes to sum[j].  As in
// k_crc_ranges a range under HS_WAVE_MIN bytes is one lane's, a longer one the wave's (a lane 16 bytes a step, the chunks on
// 16-byte boundaries, the next step asked for ahead).  A word's four bytes are summed by v_sad_u8 against zero.
// The tables stand in LDS and are counted into with ds_add_u32.  Lanes of a wave that add to ONE address take an LDS cycle
// each, and QV lines are the known bad case: a quarter of an insertion line is one value, and a line of one
// repeated value puts all 64 lanes on one counter.  So every bin stands HS_COPIES = 8 times, copy c of bin b at word 8 b + c,
// and a lane counts in copy lane & 7: eight copies are eight banks side by side, a value every lane has costs 4 cycles a
// 32-lane half instead of 32, and random values spread over 2048 words a table as they would over 256.  8 is where k_qv_hist
// ended for its busiest table, the insertion line's (PPC_INS in dx_qv.hip; profiles/r06_hist_lds.txt); 16 would halve the repeated value's cost once more, and
// with 5 tables (a .quiva entry's lines) take 80 KB a workgroup, one workgroup a CU less than two; 8 takes 40 KB, three or
// four workgroups a CU, which a kernel that waits for HBM needs more than the cycles.  These are estimates from the guide's bank
// rules: tools/census_rate.py measures, profiles/census_rate.txt has what it gave.
// The counters are 32 bits wide.  A wave that has counted HS_FLUSH bytes (2^29; DEXGPU_TEST=hist_flush=<bytes> lowers it)
// since it last did so empties ALL the workgroup's counters into the global 64-bit words: it takes each with an atomic
// exchange against zero, so nothing another wave adds meanwhile is lost, and no barrier is needed.  Between two such sweeps
// each of the four waves adds little more than 2^29 bytes (a step, or 64 short ranges), so no counter passes 2^32.  The rest leaves at the kernel's end.
//
// This file stands outside the evidence set of profiles/ (profiles/check.py hashes csrc/*.hip); its kernels have no entry in
// the profiler's name table and are timed with events on the context's stream (tools/census_rate.py).
#include "units/dx_units.hpp"

#define CC_BATCH    16u                    // units a ticket at least (k_ticket_units: more of short ones)
#define CC_EVEN     0x55555555u
#define CC_EVEN64   0x5555555555555555ull

#define HS_COPIES   8u                     // copies of every bin
#define HS_WAVE_MIN 512u                   // ranges from here on take the whole wave
#define HS_FLUSH    (1ull << 29)           // bytes a wave counts between two sweeps of the workgroup's counters
#define HS_KINDS    8

// ---------------------------------------------------------------------------------------------
//  k_code_counts
// ---------------------------------------------------------------------------------------------
struct cc_acc { uint32_t nh, nl, nb, nv; };          // symbols with the high bit, the low bit, both; symbols

// one word whose symbol t stands at bits 31 - 2t, 30 - 2t: symbols [lo, hi) of it, 0 <= lo, hi <= 16
__device__ __forceinline__ void cc_word(cc_acc &c, uint32_t w, int lo, int hi)
{ lo = lo < 0 ? 0 : (lo > 16 ? 16 : lo);
  hi = hi < 0 ? 0 : (hi > 16 ? 16 : hi);
  if (hi <= lo) return;
  const uint32_t m = CC_EVEN & (uint32_t) (0xffffffffull >> (2 * lo)) & ~(uint32_t) (0xffffffffull >> (2 * hi));
  const uint32_t h = (w >> 1) & m, l = w & m;
  c.nh += __popc(h); c.nl += __popc(l); c.nb += __popc(h & l); c.nv += __popc(m);
}

// The chunk whose place is byte `a` of the buffer (v: what last16_ask gave for it): its symbols that are symbols [S0, S1) of the
// buffer (symbol 4 x + t: byte x, bits 7 - 2t, 6 - 2t).
__device__ __forceinline__ void cc_chunk(cc_acc &c, const u32x4 &v, uint64_t bytes, uint64_t a, uint64_t S0, uint64_t S1)
{ const uint64_t from = last16_from(a, bytes);
  if (from == a && S0 <= 4u * a && 4u * a + 64u <= S1)
    { const uint64_t x = v.x | ((uint64_t) v.y << 32), y = v.z | ((uint64_t) v.w << 32);
      const uint64_t hx = (x >> 1) & CC_EVEN64, lx = x & CC_EVEN64, hy = (y >> 1) & CC_EVEN64, ly = y & CC_EVEN64;
      c.nh += __popcll(hx) + __popcll(hy); c.nl += __popcll(lx) + __popcll(ly); c.nb += __popcll(hx & lx) + __popcll(hy & ly);
      c.nv += 64u;
      return;
    }
  const uint64_t s0 = S0 > 4u * a ? S0 : 4u * a, s1 = S1 < 4u * a + 64u ? S1 : 4u * a + 64u;
  if (s1 <= s0) return;
  const int lo = (int) (s0 - 4u * from), hi = (int) (s1 - 4u * from);        // 0 <= lo < hi <= 64: S1 <= 4 bytes
  cc_word(c, __builtin_bswap32(v.x), lo, hi);
  cc_word(c, __builtin_bswap32(v.y), lo - 16, hi - 16);
  cc_word(c, __builtin_bswap32(v.z), lo - 32, hi - 32);
  cc_word(c, __builtin_bswap32(v.w), lo - 48, hi - 48);
}

__device__ __forceinline__ u32x4 cc_codes(uint32_t nh, uint32_t nl, uint32_t nb, uint32_t nv)
{ u32x4 r;
  r.x = nv - nh - nl + nb; r.y = nl - nb; r.z = nh - nb; r.w = nb;
  return r;
}

// in holds in_bytes bytes and 16 at least: the units are checked against `bound`, which is less only for a buffer of fewer than 16
// bytes (the host's padded copy of it).  bad: the smallest index of a unit that does not lie inside the buffer (preset to all ones).
// counts: n x 4, or NULL; total: four words the workgroups add to.
__global__ __launch_bounds__(DX_BLOCK)
void k_code_counts(const uint8_t *__restrict__ in, uint64_t in_bytes, uint64_t bound, const uint64_t *__restrict__ boff,
                   const uint32_t *__restrict__ beg, const uint32_t *__restrict__ len, uint64_t n,
                   uint32_t *__restrict__ counts, unsigned long long *__restrict__ total,
                   unsigned long long *__restrict__ bad, uint32_t *__restrict__ ticket)
{ __shared__ unsigned long long s_tot[4];
  if (threadIdx.x < 4u) s_tot[threadIdx.x] = 0ull;
  __syncthreads();

  const uint32_t lane = (uint32_t) lane_id(), sub = lane % UNITS_GROUP;
  uint64_t t0 = 0, t1 = 0, t2 = 0, t3 = 0;                 // what this lane has stored, code by code
  units_rounds<true>(ticket, ticket_units_of(ticket, CC_BATCH), n, [&](uint64_t u0, uint64_t r1)
    { // unit u0 + lane is this lane's to read and to check
      const uint64_t    i  = u0 + lane;
      const packed_unit pu = packed_unit_take(boff, beg, len, i, r1, bound, bad);
      uint64_t S0 = 0, S1 = 0, a0 = 0;                     // its symbols in the buffer; its first chunk's place
      uint32_t nch = 0;                                    // its chunks
      if (pu.ok && pu.len != 0u)
        { S0 = 4u * pu.at + pu.beg; S1 = S0 + pu.len;
          a0 = (S0 >> 2) & ~15ull;
          nch = (uint32_t) ((((S1 - 1u) >> 2) - a0) >> 4) + 1u;
        }

      // no symbol, or one chunk: the lane's own
      if (pu.ok && nch <= 1u)
        { cc_acc c = { 0u, 0u, 0u, 0u };
          if (nch) cc_chunk(c, last16_ask(in, in_bytes, a0), in_bytes, a0, S0, S1);
          const u32x4 r = cc_codes(c.nh, c.nl, c.nb, c.nv);
          if (counts != NULL) *(u32x4_u *) (counts + 4u * i) = r;
          t0 += r.x; t1 += r.y; t2 += r.z; t3 += r.w;
        }

      // up to 16 chunks: lanes 16 g .. 16 g + 15 take unit k + g, a chunk each, the group's counts summed along its row
      units_by_fours(__ballot(pu.ok && nch > 1u && nch <= UNITS_GROUP), [&](int from, bool mine)
        { const uint64_t gS0 = __shfl(S0, from), gS1 = __shfl(S1, from), ga0 = __shfl(a0, from);
          const uint32_t gn  = __shfl(nch, from);
          cc_acc c = { 0u, 0u, 0u, 0u };
          if (mine && sub < gn)
            { const uint64_t a = ga0 + 16u * sub;
              cc_chunk(c, last16_ask(in, in_bytes, a), in_bytes, a, gS0, gS1);
            }
          const uint32_t nh = row_sum(c.nh), nl = row_sum(c.nl), nb = row_sum(c.nb), nv = row_sum(c.nv);
          if (mine && sub == UNITS_GROUP - 1u)
            { const u32x4 r = cc_codes(nh, nl, nb, nv);
              if (counts != NULL) *(u32x4_u *) (counts + 4u * (u0 + (uint64_t) from)) = r;
              t0 += r.x; t1 += r.y; t2 += r.z; t3 += r.w;
            }
        });

      // the others: the whole wave, 1 KiB a step.  A step's bytes are asked for a step before they are counted (behind the
      // unit last16_ask gives the buffer's last 16 bytes: asked for, never counted), in a register of their own: nothing but the
      // loads is under way, so the wait in front of the counting is for all but the youngest of them.
      units_each(__ballot(pu.ok && nch > UNITS_GROUP), [&](int from)
        { const uint64_t wS0 = uniform64(__shfl(S0, from)), wS1 = uniform64(__shfl(S1, from)), wa0 = uniform64(__shfl(a0, from));
          const uint32_t wn  = uniform(__shfl(nch, from));
          cc_acc c = { 0u, 0u, 0u, 0u };
          u32x4 cur = last16_ask(in, in_bytes, wa0 + 16u * lane);
          for (uint32_t base = 0; base < wn; base += 64u)
            { const uint32_t j = base + lane;
              const u32x4 ahead = last16_ask(in, in_bytes, wa0 + 16ull * (j + 64u));
              if (j < wn) cc_chunk(c, cur, in_bytes, wa0 + 16ull * j, wS0, wS1);
              cur = ahead;
            }
          const uint32_t nh = wave_sum(c.nh), nl = wave_sum(c.nl), nb = wave_sum(c.nb), nv = wave_sum(c.nv);
          if (lane == 0u)
            { const u32x4 r = cc_codes(nh, nl, nb, nv);
              if (counts != NULL) *(u32x4_u *) (counts + 4u * (u0 + (uint64_t) from)) = r;
              t0 += r.x; t1 += r.y; t2 += r.z; t3 += r.w;
            }
        });
    });

  if (t0) atomicAdd(&s_tot[0], (unsigned long long) t0);
  if (t1) atomicAdd(&s_tot[1], (unsigned long long) t1);
  if (t2) atomicAdd(&s_tot[2], (unsigned long long) t2);
  if (t3) atomicAdd(&s_tot[3], (unsigned long long) t3);
  __syncthreads();
  if (threadIdx.x < 4u && s_tot[threadIdx.x] != 0ull) atomicAdd(total + threadIdx.x, s_tot[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------
//  k_byte_hist
// ---------------------------------------------------------------------------------------------
// tab: the range's table from this lane's copy on (s_bins + 2048 kind + (lane & 7)), bin b 8 words further on each
__device__ __forceinline__ void hs_word(uint32_t *tab, uint32_t w)
{ atomicAdd(tab + HS_COPIES * (w & 0xffu), 1u);
  atomicAdd(tab + HS_COPIES * ((w >> 8) & 0xffu), 1u);
  atomicAdd(tab + HS_COPIES * ((w >> 16) & 0xffu), 1u);
  atomicAdd(tab + HS_COPIES * (w >> 24), 1u);
}

// bytes [lo, hi) of a word, 0 <= lo, hi <= 4 after clamping: counted, and what is left of the word when the others are zeroed
__device__ __forceinline__ uint32_t hs_part(uint32_t *tab, uint32_t w, int lo, int hi)
{ lo = lo < 0 ? 0 : (lo > 4 ? 4 : lo);
  hi = hi < 0 ? 0 : (hi > 4 ? 4 : hi);
  if (hi <= lo) return 0u;
  for (int k = lo; k < hi; k++) atomicAdd(tab + HS_COPIES * ((w >> (8 * k)) & 0xffu), 1u);
  return w & (uint32_t) (((1ull << (8 * hi)) - 1u) & ~((1ull << (8 * lo)) - 1u));
}

// The chunk whose place is byte `a` of the buffer (v: what last16_ask gave for it): its bytes that are bytes [B0, B1) of the buffer are
// counted; their sum comes back.
__device__ __forceinline__ uint32_t hs_chunk(uint32_t *tab, u32x4 v, uint64_t bytes, uint64_t a, uint64_t B0, uint64_t B1)
{ const uint64_t from = last16_from(a, bytes);
  if (!(from == a && B0 <= a && a + 16u <= B1))
    { const uint64_t b0 = B0 > a ? B0 : a, b1 = B1 < a + 16u ? B1 : a + 16u;
      if (b1 <= b0) return 0u;
      const int lo = (int) (b0 - from), hi = (int) (b1 - from);              // 0 <= lo < hi <= 16: B1 <= bytes
      v.x = hs_part(tab, v.x, lo, hi);
      v.y = hs_part(tab, v.y, lo - 4, hi - 4);
      v.z = hs_part(tab, v.z, lo - 8, hi - 8);
      v.w = hs_part(tab, v.w, lo - 12, hi - 12);
    }
  else
    { hs_word(tab, v.x); hs_word(tab, v.y); hs_word(tab, v.z); hs_word(tab, v.w); }
  uint32_t s = __builtin_amdgcn_sad_u8(v.x, 0u, 0u);
  s = __builtin_amdgcn_sad_u8(v.y, 0u, s);
  s = __builtin_amdgcn_sad_u8(v.z, 0u, s);
  return __builtin_amdgcn_sad_u8(v.w, 0u, s);
}

// every counter of the workgroup taken (exchanged against zero) and added to the global words, by one wave
__device__ __forceinline__ void hs_sweep(uint32_t *s_bins, uint32_t nbins, unsigned long long *hist, uint32_t lane)
{ for (uint32_t b = lane; b < nbins; b += 64u)
    { unsigned long long s = 0;
      #pragma unroll
      for (uint32_t c = 0; c < HS_COPIES; c++) s += atomicExch(s_bins + HS_COPIES * b + c, 0u);
      if (s) atomicAdd(hist + b, s);
    }
}

// buf holds buf_bytes bytes and 16 at least; the ranges are checked against `bound` (as in k_code_counts).  hist: nkinds x 256 words
// the workgroups add to; sum: n, or NULL; kind: n, or NULL (all 0).  Dynamic LDS: nkinds x 256 x HS_COPIES counters.
__global__ __launch_bounds__(DX_BLOCK)
void k_byte_hist(const uint8_t *__restrict__ buf, uint64_t buf_bytes, uint64_t bound, const uint64_t *__restrict__ off,
                 const uint64_t *__restrict__ len, const uint8_t *__restrict__ kind, uint32_t nkinds, uint64_t n,
                 unsigned long long *__restrict__ sum, unsigned long long *__restrict__ hist, unsigned long long *__restrict__ bad,
                 uint32_t *__restrict__ ticket, uint32_t per_ticket, uint64_t flush_at)
{ extern __shared__ uint32_t s_bins[];
  const uint32_t nbins = 256u * nkinds;
  for (uint32_t k = threadIdx.x; k < nbins * HS_COPIES; k += DX_BLOCK) s_bins[k] = 0u;
  __syncthreads();

  const uint32_t lane = (uint32_t) lane_id();
  uint32_t *copy = s_bins + (lane & (HS_COPIES - 1u));
  uint64_t  counted = 0;                                   // bytes this wave has counted since it last swept
  units_rounds<false>(ticket, per_ticket, n, [&](uint64_t u0, uint64_t r1)
    { const uint64_t i = u0 + lane;
      uint64_t B0 = 0, L = 0;
      uint32_t kd = 0;
      int      how = 0;                      // 1: this lane's, 2: the wave's
      if (i < r1)
        { B0 = off[i]; L = len[i];
          kd = kind != NULL ? kind[i] : 0u;
          if (range_ok(B0, L, bound) && kd < nkinds) how = L < HS_WAVE_MIN ? 1 : 2;
          else atomicMin(bad, (unsigned long long) i);
        }
      // the short ones: chunk after chunk from the boundary in front of the range on, the lanes side by side
      { const uint64_t a0 = B0 & ~15ull;
        const uint32_t nch = how == 1 && L ? (uint32_t) (((B0 + L - 1u - a0) >> 4) + 1u) : 0u;
        uint32_t *tab = copy + 256u * HS_COPIES * kd;
        uint32_t  s = 0;
        for (uint32_t j = 0; j < nch; j++)
          s += hs_chunk(tab, last16_ask(buf, buf_bytes, a0 + 16u * j), buf_bytes, a0 + 16u * j, B0, B0 + L);
        if (how == 1 && sum != NULL) sum[i] = s;
        counted += wave_sum(how == 1 ? (uint32_t) L : 0u);
      }
      // the others: the whole wave, 1 KiB a step, the next step's bytes asked for before this step's are counted
      units_each(__ballot(how == 2), [&](int from)
        { const uint64_t wB0 = uniform64(__shfl(B0, from)), wL = uniform64(__shfl(L, from));
          const uint32_t wk  = uniform(__shfl(kd, from));
          const uint64_t wa0 = wB0 & ~15ull, wn = ((wB0 + wL - 1u - wa0) >> 4) + 1u;
          uint32_t *tab = copy + 256u * HS_COPIES * wk;
          uint64_t  s = 0;
          u32x4 cur = last16_ask(buf, buf_bytes, wa0 + 16u * lane);
          for (uint64_t base = 0; base < wn; base += 64u)
            { const uint64_t j = base + lane;
              const u32x4 ahead = last16_ask(buf, buf_bytes, wa0 + 16u * (j + 64u));
              if (j < wn) s += hs_chunk(tab, cur, buf_bytes, wa0 + 16u * j, wB0, wB0 + wL);
              cur = ahead;
              counted += DX_STEP;
              if (counted >= flush_at)
                { hs_sweep(s_bins, nbins, hist, lane);
                  counted = 0;
                }
            }
          #pragma unroll
          for (int d = 32; d > 0; d >>= 1) s += __shfl_xor((unsigned long long) s, d);
          if (lane == 0u && sum != NULL) sum[u0 + (uint64_t) from] = s;
        });
      if (counted >= flush_at)
        { hs_sweep(s_bins, nbins, hist, lane);
          counted = 0;
        }
    });

  __syncthreads();
  for (uint32_t b = threadIdx.x; b < nbins; b += DX_BLOCK)
    { unsigned long long s = 0;
      #pragma unroll
      for (uint32_t c = 0; c < HS_COPIES; c++) s += s_bins[HS_COPIES * b + c];
      if (s) atomicAdd(hist + b, s);
    }
}

// ---------------------------------------------------------------------------------------------
//  the entry points
// ---------------------------------------------------------------------------------------------
extern "C" int dx_code_counts(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes,
                              const uint64_t *d_boff, const uint32_t *d_beg, const uint32_t *d_len, uint64_t n,
                              uint32_t *d_counts, uint64_t total[4], uint64_t *bad_unit)
{ if (ctx == NULL) return DX_E_ARG;
  if (bad_unit) *bad_unit = UINT64_MAX;
  if (total) total[0] = total[1] = total[2] = total[3] = 0;
  if (n == 0) return DX_OK;
  units_frame    f;
  uint64_t       back[UF_OUT + 4];
  const uint64_t bound = in_bytes;                         // (the kernel loads 16 bytes at a time: fewer are copied, zeros behind them)
  int rc = units_begin(ctx, "dx_code_counts", n, d_boff && d_len && (d_in || !in_bytes), ctx->d_u64 + DXW_UNITS, 4, 16, &d_in, &in_bytes, &f);
  if (rc != DX_OK) return rc;
  // (units per ticket from the packed bytes' extent, about 40 kB a ticket: units that do not stand in the buffer's order give a
  //  figure that means nothing, and the bounds of ticket_units_of hold)
  hipLaunchKernelGGL(k_ticket_units, dim3(1), dim3(1), 0, ctx->stream, d_boff, d_boff + (n - 1), (const uint32_t *) NULL, n,
                     CC_BATCH * 2500u, CC_BATCH, f.ticket);
  hipLaunchKernelGGL(k_code_counts, dim3(dx_grid_waves(ctx, n, 32)), dim3(DX_BLOCK), 0, ctx->stream, d_in, in_bytes, bound,
                     d_boff, d_beg, d_len, n, d_counts, f.out, f.bad, f.ticket);
  rc = units_end(ctx, f, back, bad_unit, "%s: unit %llu does not lie inside the %llu packed bytes", bound);
  if (rc == DX_OK && total) memcpy(total, back + UF_OUT, 32);
  return rc;
}

extern "C" int dx_byte_hist_ranges(dx_ctx *ctx, const uint8_t *d_buf, uint64_t buf_bytes, const uint64_t *d_off, const uint64_t *d_len,
                                   const uint8_t *d_kind, int nkinds, uint64_t n, uint64_t *d_sum, uint64_t *hist, uint64_t *bad_unit)
{ if (ctx == NULL) return DX_E_ARG;
  if (bad_unit) *bad_unit = UINT64_MAX;
  if (nkinds < 1 || nkinds > HS_KINDS)
    return dx_fail(ctx, DX_E_ARG, "dx_byte_hist_ranges: %d tables (1 to %d)", nkinds, HS_KINDS);
  if (hist) memset(hist, 0, (size_t) nkinds * 256u * 8u);
  if (n == 0) return DX_OK;
  const size_t   words = (size_t) nkinds * 256u;           // (more than the context's frame holds: the frame heads a scratch block,
  units_frame    f;                                        //  so that the tables still come back with it in one copy)
  const uint64_t bound = buf_bytes;
  int rc = units_begin(ctx, "dx_byte_hist_ranges", n, d_off && d_len && (d_buf || !buf_bytes), NULL, words, 16, &d_buf, &buf_bytes, &f);
  if (rc != DX_OK) return rc;
  std::vector<uint64_t> back(UF_OUT + words);
  long long flush = dx_test_num("hist_flush", (long long) HS_FLUSH);               // (tests: the counters swept from this many bytes on)
  if (flush < (long long) DX_STEP || flush > (long long) HS_FLUSH) flush = (long long) HS_FLUSH;
  // a ticket: 64 units at least; of many units more, so that the draws stay few beside the work (as dx_crc32_ranges)
  const size_t lds  = words * HS_COPIES * sizeof(uint32_t);
  const int    grid = dx_grid_waves(ctx, (n + 63u) / 64u, (int) (4u * ((160u << 10) / lds > 4u ? 4u : (160u << 10) / lds)));
  uint64_t     per  = n / ((uint64_t) grid * DX_WAVES_PER_BLK * 8u);
  per = per < 64u ? 64u : (per > 4096u ? 4096u : per & ~63ull);
  if (lds > (32u << 10))                                  // (up to 64 KB: eight tables)
    DX_HIP(ctx, hipFuncSetAttribute((const void *) k_byte_hist, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
  hipLaunchKernelGGL(k_byte_hist, dim3(grid), dim3(DX_BLOCK), lds, ctx->stream, d_buf, buf_bytes, bound, d_off, d_len, d_kind,
                     (uint32_t) nkinds, n, (unsigned long long *) d_sum, f.out, f.bad, f.ticket, (uint32_t) per, (uint64_t) flush);
  rc = units_end(ctx, f, back.data(), bad_unit, "%s: range %llu does not lie inside the buffer's %llu bytes, or its kind is not below %d", bound, nkinds);
  if (rc == DX_OK && hist) memcpy(hist, back.data() + UF_OUT, words * 8u);
  return rc;
}
