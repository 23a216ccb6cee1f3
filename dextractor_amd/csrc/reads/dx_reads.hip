// dx_reads.hip -- dx_reads_unpack: reads and subreads out of a .bps / .arw payload, as the DB runtime hands them to its callers.
//
// Reference behaviour reproduced (bit-exact):
//   Load_Read        DB.c:1274-1297   COMPRESSED_LEN(rlen) bytes at boff, Uncompress_Read, the letters, a delimiter on both sides
//   Load_Subread     DB.c:1351-1378   bytes [beg / 4, (end - 1) / 4 + 1) of the read, the string begins beg % 4 symbols into them
//   Load_All_Reads   DB.c:1406-1433   the reads one behind the other, one delimiter between two of them
//   Load_Arrow       DB.c:1508-1548   the same for the .arw track
//   Uncompress_Read  DB.c:342-363     symbol i = bits 7 - 2 (i & 3), 6 - 2 (i & 3) of byte i >> 2; 4 behind the last one
//   Lower_Read & co. DB.c:367-389     the letters, '\0' behind the last one
//
// A unit is symbols [beg, beg + len) of the packed read that starts at in + boff -- boff any byte, beg any phase -- and leaves as
// len bytes and ONE delimiter behind them at out + out_off: nothing in front, nothing behind that.  The units are independent:
// any order, overlapping or repeated in the input.  Roofline: HBM, 0.25 bytes read and 1 written a symbol.
//
// Layout: the waves draw units from a ticket counter (k_ticket_units: about 160 kB of output a ticket, 16 units at least) and
// take a ticket's units 64 at a time, a lane reading one unit's four parameters and checking its bounds.  Then
//   * the units whose bytes fit 256 (from the 16-byte boundary in front of them) go FOUR A STEP, a group of 16 lanes each --
//     a batch of subreads of a few dozen symbols costs a quarter of a wave-step a unit, not a whole one;
//   * the others one after the other by the whole wave, 1 KiB a step, the packed bytes of the next step asked for before
//     the letters of this one are made.
// Either way a lane's share is 16 output bytes from 8 packed ones (5 are needed: 16 symbols at any phase), the phase beg & 3
// folded into the shift that lines the symbols up, four look-ups in a 256-entry table of a byte's four letters, and one
// 16-byte store.  As in k_pack2_decode (profiles/r06_pack2_align.txt) the stores stand on 16-byte boundaries of the OUTPUT:
// the unit is walked as if it began at the boundary in front of it.  There are no line ends, so nothing is moved inside a
// chunk: the chunk in front of the boundary and the last, partial one are whole chunks too, slid to the unit's first and
// last 16 bytes (two stores off a boundary a unit; the neighbours write the bytes they share again, with the same values),
// and the delimiter is the last byte of the last one.  Units of fewer than 16 bytes go byte by byte, by one lane.
//
// Nothing outside [0, in_bytes) is read: 8 bytes that would reach past the buffer's end are its last 8, shifted (a buffer of
// fewer than 8 bytes is copied into 8 first).  A unit that does not lie inside the buffer is not decoded; the smallest such index
// goes back to the host, one read-back a call.
//
// This file stands outside the evidence set of profiles/ (profiles/check.py hashes csrc/*.hip), and the kernel has no entry in
// the profiler's name table: tools/reads_rate.py times it with events on the context's stream, beside k_pack2_decode.
#include "units/dx_units.hpp"

#define RD_BATCH   16u                   // units a ticket at least (k_ticket_units: more of short ones)
#define RD_SHORT   (16u * UNITS_GROUP)   // a short unit (16 lanes'): its bytes, from the 16-byte boundary in front of them on, are no more than this

template <int LETTERS>
__device__ __forceinline__ uint32_t rd_letter(uint32_t code)
{ if (LETTERS == DX_LETTERS_LOWER) return (0x74676361u >> (8 * code)) & 0xffu;       // "acgt"
  if (LETTERS == DX_LETTERS_UPPER) return (0x54474341u >> (8 * code)) & 0xffu;       // "ACGT"
  if (LETTERS == DX_LETTERS_ARROW) return '1' + code;
  return code;                                       // DX_LETTERS_NUMBERS
}

// one unit: N = len + 1 bytes (the delimiter is one of them) at out + to, which stands adj bytes behind a 16-byte boundary
struct rd_unit
{ uint64_t at, to;              // boff, out_off
  uint32_t beg, N, adj;
};

// The chunk at position q of the unit's frame (the output from the boundary in front of dst on; q a multiple of 16) begins with
// output byte q - adj: slid to 0 in front of the unit and to N - 16 behind it, so that it is 16 bytes of the unit wherever q
// is (N >= 16).  A q behind the frame gives the unit's last chunk once more.
__device__ __forceinline__ uint32_t rd_first(const rd_unit &u, uint32_t q)
{ const uint32_t o = q < u.adj ? 0u : q - u.adj;
  return o > u.N - 16u ? u.N - 16u : o;
}

// The 8 packed bytes from the one that holds the chunk's first symbol on (N >= 16: that symbol is one of the unit's, so its
// byte lies inside the buffer) -- the buffer's last 8 bytes instead when they would reach past its end (in_bytes >= 8: the
// host sees to that).  rd_ask only asks: what came is put right by rd_got, where it is used, so that nothing waits here.
__device__ __forceinline__ uint64_t rd_byte(const rd_unit &u, uint32_t q)
{ return u.at + (((uint64_t) u.beg + rd_first(u, q)) >> 2); }

__device__ __forceinline__ uint64_t rd_ask(const uint8_t *in, uint64_t in_bytes, const rd_unit &u, uint32_t q)
{ const uint64_t a = rd_byte(u, q);
  return *(const u64_u *) (in + (a + 8u > in_bytes ? in_bytes - 8u : a));
}

// ... first in the low byte, what lay in front of the chunk's byte shifted out
__device__ __forceinline__ uint64_t rd_got(uint64_t raw, uint64_t in_bytes, const rd_unit &u, uint32_t q)
{ const uint64_t a = rd_byte(u, q);
  return a + 8u > in_bytes ? raw >> (8u * (uint32_t) ((a + 8u - in_bytes) & 7u)) : raw;
}

// 16 symbols from 8 packed bytes: symbol j of the chunk in bits 31 - 2j, 30 - 2j
__device__ __forceinline__ uint32_t rd_codes(uint64_t raw, uint32_t phase)
{ const uint64_t be = ((uint64_t) __builtin_bswap32((uint32_t) raw) << 32) | __builtin_bswap32((uint32_t) (raw >> 32));
  return (uint32_t) ((be << (2u * phase)) >> 32);
}

template <int LETTERS>
__device__ __forceinline__ void rd_put(const uint32_t *quad, uint64_t in_bytes, uint8_t *out, const rd_unit &u, uint32_t q, uint64_t raw)
{ const uint32_t delim = LETTERS == DX_LETTERS_NUMBERS ? 4u : 0u;                    // DB.c:362 / DB.c:367-389
  const uint32_t o  = rd_first(u, q);
  const uint32_t cw = rd_codes(rd_got(raw, in_bytes, u, q), (u.beg + o) & 3u);
  u32x4 v;
  v.x = quad[cw >> 24];
  v.y = quad[(cw >> 16) & 0xffu];
  v.z = quad[(cw >> 8) & 0xffu];
  v.w = quad[cw & 0xffu];
  if (o + 16u == u.N) v.w = (v.w & 0x00ffffffu) | (delim << 24);                     // the unit's last chunk ends with the delimiter
  *(u32x4_u *) (out + u.to + o) = v;
}

// a unit of fewer than 16 bytes (at most 14 symbols in 5 packed bytes), by one lane
template <int LETTERS>
__device__ __forceinline__ void rd_small(const uint8_t *in, const uint32_t *quad, uint8_t *out, const rd_unit &u)
{ const uint32_t delim = LETTERS == DX_LETTERS_NUMBERS ? 4u : 0u;
  const uint32_t len = u.N - 1u, nb = len ? ((u.beg & 3u) + len + 3u) >> 2 : 0u;
  const uint64_t a = u.at + (u.beg >> 2);
  uint64_t raw = 0;
  for (uint32_t k = 0; k < nb; k++)
    raw |= (uint64_t) in[a + k] << (8u * k);
  const uint32_t cw = rd_codes(raw, u.beg & 3u);
  const uint32_t w0 = quad[cw >> 24], w1 = quad[(cw >> 16) & 0xffu], w2 = quad[(cw >> 8) & 0xffu], w3 = quad[cw & 0xffu];
  for (uint32_t b = 0; b < u.N; b++)
    { const uint32_t w = b < 4u ? w0 : b < 8u ? w1 : b < 12u ? w2 : w3;
      out[u.to + b] = (uint8_t) (b == len ? delim : w >> (8u * (b & 3u)));
    }
}

// bad: the smallest index of a unit that does not lie inside the buffer (preset to all ones).  in holds in_bytes bytes and 8 at least:
// the units are checked against `bound`, which is less only for a buffer of fewer than 8 bytes (the host's padded copy of it).
template <int LETTERS>
__global__ __launch_bounds__(DX_BLOCK)
void k_reads_unpack(const uint8_t *__restrict__ in, uint64_t in_bytes, uint64_t bound, const uint64_t *__restrict__ boff,
                    const uint32_t *__restrict__ beg, const uint32_t *__restrict__ len, uint64_t n,
                    uint8_t *__restrict__ out, const uint64_t *__restrict__ out_off,
                    unsigned long long *__restrict__ bad, uint32_t *__restrict__ ticket)
{ __shared__ uint32_t s_quad[256];       // packed byte -> its four letters
  for (uint32_t k = threadIdx.x; k < 256u; k += DX_BLOCK)
    s_quad[k] = rd_letter<LETTERS>(k >> 6) | (rd_letter<LETTERS>((k >> 4) & 3u) << 8)
              | (rd_letter<LETTERS>((k >> 2) & 3u) << 16) | (rd_letter<LETTERS>(k & 3u) << 24);
  __syncthreads();

  const uint32_t lane = (uint32_t) lane_id(), q_grp = 16u * (lane % UNITS_GROUP);
  units_rounds<true>(ticket, ticket_units_of(ticket, RD_BATCH), n, [&](uint64_t u0, uint64_t r1)
    { // unit u0 + lane is this lane's to read and to check
      const uint64_t    i  = u0 + lane;
      const packed_unit pu = packed_unit_take(boff, beg, len, i, r1, bound, bad);
      rd_unit mine = { pu.at, 0ull, pu.beg, pu.len + 1u, 0u };
      if (i < r1)
        { mine.to  = out_off[i];
          mine.adj = (uint32_t) ((uintptr_t) (out + mine.to) & 15u);
        }
      const bool brief = pu.ok && mine.N + mine.adj <= RD_SHORT;

      // the short ones: lanes 16 g .. 16 g + 15 take unit k + g
      units_by_fours(__ballot(brief), [&](int from, bool its)
        { rd_unit u;
          u.at  = __shfl(mine.at, from);
          u.beg = __shfl(mine.beg, from);
          u.N   = __shfl(mine.N, from);
          u.adj = __shfl(mine.adj, from);
          u.to  = __shfl(mine.to, from);
          if (its && q_grp < u.N + u.adj)
            { if (u.N >= 16u) rd_put<LETTERS>(s_quad, in_bytes, out, u, q_grp, rd_ask(in, in_bytes, u, q_grp));
              else if (q_grp == 0u) rd_small<LETTERS>(in, s_quad, out, u);
            }
        });

      // the others: the whole wave, 1 KiB of the frame a step
      units_each(__ballot(pu.ok && !brief), [&](int from)
        { rd_unit u;
          u.at  = uniform64(__shfl(mine.at, from));
          u.beg = uniform(__shfl(mine.beg, from));
          u.N   = uniform(__shfl(mine.N, from));
          u.adj = uniform(__shfl(mine.adj, from));
          u.to  = uniform64(__shfl(mine.to, from));
          const uint32_t TS = u.N + u.adj;                 // the frame's bytes
          // A step's packed bytes are asked for a step before its letters are made and stored, in two registers that take
          // turns (a copy of a requested register would wait for it).  A wave's loads and stores are counted together and
          // retire in order, so a wait for a load is a wait for every older store as well.  In the steps in which every lane
          // has a chunk (all but a unit's last) each step issues exactly one load and one store, and behind "ask for the
          // next step" the wait is for all but the two youngest operations -- that request and the store of the step
          // before, which so has a whole step to be acknowledged in.  The first of these steps stands in front of the loop,
          // so that the loop is entered as it is gone round: one request and one store under way (where paths with other
          // counts meet the compiler waits for the shortest).  The waits written here only say what the compiler could
          // count itself (as in k_pack2_decode); its own stay sufficient whatever these say.  Behind the frame rd_ask gives
          // the last chunk's bytes once more: asked for, never used.
          const uint32_t full = TS & ~(DX_STEP - 1u);      // the frame's bytes in whole steps
          uint32_t q = 16u * lane, base = 0;
          uint64_t rawA = rd_ask(in, in_bytes, u, q), rawB = rd_ask(in, in_bytes, u, q + DX_STEP);
          if (full != 0u)
            { rd_put<LETTERS>(s_quad, in_bytes, out, u, q, rawA);
              for (base = DX_STEP; base + 2u * DX_STEP <= full; base += 2u * DX_STEP)
                { rawA = rd_ask(in, in_bytes, u, q + base + DX_STEP);
                  __builtin_amdgcn_s_waitcnt(0x0F72);      // vmcnt(2)
                  rd_put<LETTERS>(s_quad, in_bytes, out, u, q + base, rawB);
                  rawB = rd_ask(in, in_bytes, u, q + base + 2u * DX_STEP);
                  __builtin_amdgcn_s_waitcnt(0x0F72);
                  rd_put<LETTERS>(s_quad, in_bytes, out, u, q + base + DX_STEP, rawA);
                }
              rawA = rawB;
            }
          // what is left: a whole step at most, and the last, partial one (rawA: the bytes of the step at base)
          for (; base < TS; base += DX_STEP)
            { const uint64_t ahead = rd_ask(in, in_bytes, u, q + base + DX_STEP);
              if (q + base < TS) rd_put<LETTERS>(s_quad, in_bytes, out, u, q + base, rawA);
              rawA = ahead;
            }
        });
    });
}

extern "C" int dx_reads_unpack(dx_ctx *ctx, int letters, const uint8_t *d_in, uint64_t in_bytes,
                               const uint64_t *d_boff, const uint32_t *d_beg, const uint32_t *d_len,
                               uint64_t n, uint8_t *d_out, const uint64_t *d_out_off, uint64_t *bad_unit)
{ if (ctx == NULL) return DX_E_ARG;
  if (bad_unit) *bad_unit = UINT64_MAX;
  if (letters < DX_LETTERS_LOWER || letters > DX_LETTERS_NUMBERS)
    return dx_fail(ctx, DX_E_ARG, "dx_reads_unpack: unknown letter set %d", letters);
  if (n == 0) return DX_OK;
  units_frame    f;
  uint64_t       back[UF_OUT];
  const uint64_t bound = in_bytes;                         // (the kernel loads 8 bytes at a time: fewer are copied, zeros behind them)
  int rc = units_begin(ctx, "dx_reads_unpack", n, d_boff && d_len && d_out && d_out_off && (d_in || !in_bytes),
                       ctx->d_u64 + DXW_UNITS, 0, 8, &d_in, &in_bytes, &f);
  if (rc != DX_OK) return rc;
  // (units per ticket from the output's extent: outputs that do not stand in the units' order give a figure that means
  //  nothing, and the bounds of ticket_units_of hold)
  hipLaunchKernelGGL(k_ticket_units, dim3(1), dim3(1), 0, ctx->stream, d_out_off, d_out_off + (n - 1), d_len + (n - 1), n,
                     RD_BATCH * 10000u, RD_BATCH, f.ticket);
  const int grid = dx_grid_waves(ctx, n, 32);
  switch (letters)
    { case DX_LETTERS_LOWER:
        hipLaunchKernelGGL(k_reads_unpack<DX_LETTERS_LOWER>, dim3(grid), dim3(DX_BLOCK), 0, ctx->stream,
                           d_in, in_bytes, bound, d_boff, d_beg, d_len, n, d_out, d_out_off, f.bad, f.ticket);
        break;
      case DX_LETTERS_UPPER:
        hipLaunchKernelGGL(k_reads_unpack<DX_LETTERS_UPPER>, dim3(grid), dim3(DX_BLOCK), 0, ctx->stream,
                           d_in, in_bytes, bound, d_boff, d_beg, d_len, n, d_out, d_out_off, f.bad, f.ticket);
        break;
      case DX_LETTERS_ARROW:
        hipLaunchKernelGGL(k_reads_unpack<DX_LETTERS_ARROW>, dim3(grid), dim3(DX_BLOCK), 0, ctx->stream,
                           d_in, in_bytes, bound, d_boff, d_beg, d_len, n, d_out, d_out_off, f.bad, f.ticket);
        break;
      default:
        hipLaunchKernelGGL(k_reads_unpack<DX_LETTERS_NUMBERS>, dim3(grid), dim3(DX_BLOCK), 0, ctx->stream,
                           d_in, in_bytes, bound, d_boff, d_beg, d_len, n, d_out, d_out_off, f.bad, f.ticket);
        break;
    }
  return units_end(ctx, f, back, bad_unit, "%s: unit %llu does not lie inside the %llu packed bytes", bound);
}
