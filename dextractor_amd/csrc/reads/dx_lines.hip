// dx_lines.hip -- dx_reads_unpack_lines: an interval of a packed read as the lines undexta / undexar print for it.
//
// Reference behaviour reproduced (bit-exact):
//   undexta.c:263-270  the letters `width` a line, '\n' behind every line and behind the last, shorter one
//   Uncompress_Read    DB.c:342-363   symbol i = bits 7 - 2 (i & 3), 6 - 2 (i & 3) of byte i >> 2
//   Lower_Read & co.   DB.c:367-389   the letters
//
// A unit is what it is for dx_reads_unpack (dx_reads.hip) -- symbols [beg, beg + len) of the packed read that starts at in +
// boff, boff any byte, beg any phase -- and leaves as T = len + (len + width - 1) / width bytes at out + out_off: k_pack2_decode's
// text of those symbols.  NOT ONE BYTE outside those T is written: in dx_file_extract's layout the neighbours are header
// lines.  There is no delimiter; len == 0 writes nothing.  Roofline: HBM, 0.25 bytes read and 1 + 1 / width written a symbol.
//
// Layout: k_reads_unpack's.  The waves draw units from a ticket counter and take a ticket's units 64 at a time, a lane reading
// one unit's parameters and checking its bounds; units whose text fits 256 bytes (from the 16-byte boundary in front of it) go
// FOUR A STEP, a group of 16 lanes each, the others one after the other by the whole wave, 1 KiB a step, the packed bytes of
// the next step asked for before the letters of this one are made.  A lane's share is a CHUNK: 16 bytes of text from 8 packed
// ones.  The stores stand on 16-byte boundaries of the OUTPUT (profiles/r06_pack2_align.txt): the text is walked as if it began
// at the boundary in front of it, and the chunk in front of that boundary and the last, partial one are whole chunks too, slid
// to the text's first and last 16 bytes (two stores off a boundary a unit; the neighbours write the bytes they share again,
// with the same values).  Texts of fewer than 16 bytes go byte by byte, by one lane.
//
// What is new here is where a chunk stands in the text.  Text byte o lies in line o / (width + 1) at column o % (width + 1),
// column `width` being the line's end; `line` line ends stand in front of it, so the chunk's first symbol is o - line.
//   * width >= 16: one line end a chunk at most, but for the text's last byte, which is a line end wherever it falls.  The 16
//     codes are made as if there were none, a 2-bit hole is opened where the line end goes (k_pack2_decode's), and the
//     last chunk's last byte is set.  (line, column) are kept per lane and moved on by a step's worth, as k_pack2_decode does
//     it: no division but one a unit, for the last chunk's place.
//   * width < 16: several line ends a chunk.  A kernel of its own (NARROW) places a chunk by division and makes it byte by byte.
//
// Nothing outside [0, in_bytes) is read: 8 bytes that would reach past the buffer's end are its last 8, shifted (a buffer of
// fewer than 8 bytes is copied into 8 first).  A unit that does not lie inside the buffer is not decoded; the smallest such
// index goes back to the host, one read-back a call.
//
// This file stands outside the evidence set of profiles/ (profiles/check.py hashes csrc/*.hip), and the kernel has no entry in
// the profiler's name table: tools/reads_rate.py times it with events on the context's stream, beside k_reads_unpack.
#include "units/dx_units.hpp"

#define LN_BATCH   16u                   // units a ticket at least (k_ticket_units: more of short ones)
#define LN_SHORT   (16u * UNITS_GROUP)   // a short unit (16 lanes'): its text, from the 16-byte boundary in front of it on, is no more than this
#define LN_WIDTH_MOST 0x80000000u        // a line never has more than UNITS_LEN_MAX symbols: wider than this is as wide as this

template <int LETTERS>
__device__ __forceinline__ uint32_t ln_letter(uint32_t code)
{ if (LETTERS == DX_LETTERS_LOWER) return (0x74676361u >> (8 * code)) & 0xffu;       // "acgt"
  if (LETTERS == DX_LETTERS_UPPER) return (0x54474341u >> (8 * code)) & 0xffu;       // "ACGT"
  return '1' + code;                                                                 // DX_LETTERS_ARROW
}

// one unit: T bytes of text at out + to, which stands adj bytes behind a 16-byte boundary; its last chunk (text byte T - 16 on,
// T >= 16) begins in line endl at column endc
struct ln_unit
{ uint64_t at, to;              // boff, out_off
  uint32_t beg, len, T, adj, endl, endc;
};

// a place in the text as (line, column): text byte line * (width + 1) + column
struct ln_pos { uint32_t line, col; };

__device__ __forceinline__ ln_pos ln_moved(ln_pos p, uint32_t dline, uint32_t dcol, uint32_t W1)
{ p.line += dline; p.col += dcol;
  if (p.col >= W1) { p.col -= W1; p.line += 1u; }
  return p;
}

// The place adj bytes in front of p (adj < 16 <= width: one borrow at most).  In front of the text it is line -1, and comes
// right again when ln_moved carries it over the text's begin.
__device__ __forceinline__ ln_pos ln_back(ln_pos p, uint32_t adj, uint32_t W1)
{ if (p.col < adj) { p.col += W1; p.line -= 1u; }
  p.col -= adj;
  return p;
}

__device__ __forceinline__ uint32_t ln_text_bytes(uint32_t len, uint32_t width)
{ return len + (uint32_t) (((uint64_t) len + width - 1u) / width); }

// a chunk: text bytes [o, o + 16), the first at column col; its first symbol's packed byte and phase
struct ln_chunk { uint64_t a; uint32_t o, col, ph; };

// The chunk at position q of the unit's frame (the output from the boundary in front of it on; q a multiple of 16) begins with
// text byte q - adj: slid to 0 in front of the text and to T - 16 behind it, so that it is 16 bytes of the text wherever q is
// (T >= 16).  A q behind the frame gives the last chunk once more.  p: the place of text byte q - adj (!NARROW).
template <bool NARROW>
__device__ __forceinline__ ln_chunk ln_where(const ln_unit &u, uint32_t q, ln_pos p, uint32_t W1)
{ ln_chunk c;
  uint32_t line;
  if (q < u.adj)               { c.o = 0u;         line = 0u;     c.col = 0u; }
  else if (q - u.adj > u.T - 16u) { c.o = u.T - 16u;  line = u.endl; c.col = u.endc; }
  else                         { c.o = q - u.adj;  line = p.line; c.col = p.col; }
  if (NARROW)
    { line  = c.o / W1;
      c.col = c.o - line * W1;
    }
  const uint64_t s = (uint64_t) u.beg + (c.o - line);        // the read's symbol the chunk begins with: one of the unit's
  c.a = u.at + (s >> 2); c.ph = (uint32_t) s & 3u;
  return c;
}

// The 8 packed bytes from byte a on -- the buffer's last 8 bytes instead when they would reach past its end (in_bytes >= 8: the
// host sees to that).  ln_ask only asks: what came is put right by ln_got, where it is used, so that nothing waits here.
__device__ __forceinline__ uint64_t ln_ask(const uint8_t *in, uint64_t in_bytes, uint64_t a)
{ return *(const u64_u *) (in + (a + 8u > in_bytes ? in_bytes - 8u : a)); }

// ... first in the low byte, what lay in front of byte a shifted out
__device__ __forceinline__ uint64_t ln_got(uint64_t raw, uint64_t in_bytes, uint64_t a)
{ return a + 8u > in_bytes ? raw >> (8u * (uint32_t) ((a + 8u - in_bytes) & 7u)) : raw; }

// 16 symbols from 8 packed bytes: symbol j in bits 31 - 2j, 30 - 2j
__device__ __forceinline__ uint32_t ln_codes(uint64_t raw, uint32_t phase)
{ const uint64_t be = ((uint64_t) __builtin_bswap32((uint32_t) raw) << 32) | __builtin_bswap32((uint32_t) (raw >> 32));
  return (uint32_t) ((be << (2u * phase)) >> 32);
}

// 16 bytes of text byte by byte, any width: the first at column col, byte endb the text's last (16: it is not among them)
template <int LETTERS>
__device__ __forceinline__ u32x4 ln_bytes(uint32_t cw, uint32_t col, uint32_t width, uint32_t endb)
{ uint32_t w[4] = { 0u, 0u, 0u, 0u };
  #pragma unroll
  for (uint32_t b = 0; b < 16u; b++)
    { uint32_t ch;
      if (col == width || b == endb) { ch = '\n'; col = 0u; }
      else                           { ch = ln_letter<LETTERS>(cw >> 30); cw <<= 2; col += 1u; }
      w[b >> 2] |= ch << (8u * (b & 3u));
    }
  const u32x4 v = { w[0], w[1], w[2], w[3] };
  return v;
}

template <int LETTERS, bool NARROW>
__device__ __forceinline__ void ln_put(const uint32_t *quad, uint64_t in_bytes, uint8_t *out, const ln_unit &u, const ln_chunk &c,
                                       uint64_t raw, uint32_t width)
{ uint32_t   cw   = ln_codes(ln_got(raw, in_bytes, c.a), c.ph);
  const bool last = c.o + 16u == u.T;
  u32x4 v;
  if (NARROW)
    v = ln_bytes<LETTERS>(cw, c.col, width, last ? 15u : 16u);
  else
    { const uint32_t nlpos = width - c.col;                  // where this line ends, from the chunk's first byte on
      if (nlpos < 16u)
        { const uint32_t K = 30u - 2u * nlpos;               // open a 2-bit hole at slot nlpos
          const uint32_t keep = ~((4u << K) - 1u);           // slots before it
          cw = (cw & keep) | ((cw & ~keep) >> 2);
        }
      v.x = quad[cw >> 24];
      v.y = quad[(cw >> 16) & 0xffu];
      v.z = quad[(cw >> 8) & 0xffu];
      v.w = quad[cw & 0xffu];
      if (nlpos < 16u)
        { const uint32_t m = 0xffu << (8u * (nlpos & 3u)), j = nlpos >> 2;
          const uint32_t nl4 = 0x0a0a0a0au;
          v.x = j == 0u ? (v.x & ~m) | (nl4 & m) : v.x;
          v.y = j == 1u ? (v.y & ~m) | (nl4 & m) : v.y;
          v.z = j == 2u ? (v.z & ~m) | (nl4 & m) : v.z;
          v.w = j == 3u ? (v.w & ~m) | (nl4 & m) : v.w;
        }
      if (last) v.w = (v.w & 0x00ffffffu) | ((uint32_t) '\n' << 24);     // the text's last byte, wherever its line ends
    }
  *(u32x4_u *) (out + u.to + c.o) = v;
}

// a text of fewer than 16 bytes (at most 14 symbols in 5 packed bytes), by one lane
template <int LETTERS>
__device__ __forceinline__ void ln_small(const uint8_t *in, uint8_t *out, const ln_unit &u, uint32_t width)
{ const uint32_t nb = u.len ? ((u.beg & 3u) + u.len + 3u) >> 2 : 0u;
  const uint64_t a  = u.at + (u.beg >> 2);
  uint64_t raw = 0;
  for (uint32_t k = 0; k < nb; k++)
    raw |= (uint64_t) in[a + k] << (8u * k);
  const u32x4 v = ln_bytes<LETTERS>(ln_codes(raw, u.beg & 3u), 0u, width, u.T - 1u);
  for (uint32_t b = 0; b < u.T; b++)
    { const uint32_t w = b < 4u ? v.x : b < 8u ? v.y : b < 12u ? v.z : v.w;
      out[u.to + b] = (uint8_t) (w >> (8u * (b & 3u)));
    }
}

// bad: the smallest index of a unit that does not lie inside the buffer (preset to all ones).  in holds in_bytes bytes and 8 at least:
// the units are checked against `bound`, which is less only for a buffer of fewer than 8 bytes (the host's padded copy of it).
// width: 1 .. LN_WIDTH_MOST, and NARROW says that it is below 16.
template <int LETTERS, bool NARROW>
__global__ __launch_bounds__(DX_BLOCK)
void k_reads_unpack_lines(const uint8_t *__restrict__ in, uint64_t in_bytes, uint64_t bound, const uint64_t *__restrict__ boff,
                          const uint32_t *__restrict__ beg, const uint32_t *__restrict__ len, uint64_t n, uint32_t width,
                          uint8_t *__restrict__ out, const uint64_t *__restrict__ out_off,
                          unsigned long long *__restrict__ bad, uint32_t *__restrict__ ticket)
{ __shared__ uint32_t s_quad[256];       // packed byte -> its four letters
  for (uint32_t k = threadIdx.x; k < 256u; k += DX_BLOCK)
    s_quad[k] = ln_letter<LETTERS>(k >> 6) | (ln_letter<LETTERS>((k >> 4) & 3u) << 8)
              | (ln_letter<LETTERS>((k >> 2) & 3u) << 16) | (ln_letter<LETTERS>(k & 3u) << 24);
  __syncthreads();

  // the places of frame bytes 16 lane (the wave's) and 16 (lane % 16) (a group's) of a text that begins on a boundary, and a step's worth
  const uint32_t W1   = width + 1u;
  const uint32_t lane = (uint32_t) lane_id(), q_grp = 16u * (lane % UNITS_GROUP);
  const ln_pos   at_wave = { (16u * lane) / W1, (16u * lane) % W1 }, at_grp = { q_grp / W1, q_grp % W1 };
  const uint32_t dline = DX_STEP / W1, dcol = DX_STEP % W1;

  units_rounds<true>(ticket, ticket_units_of(ticket, LN_BATCH), n, [&](uint64_t u0, uint64_t r1)
    { // unit u0 + lane is this lane's to read and to check
      const uint64_t    i  = u0 + lane;
      const packed_unit pu = packed_unit_take(boff, beg, len, i, r1, bound, bad);
      ln_unit mine = { pu.at, 0ull, pu.beg, pu.len, pu.ok ? ln_text_bytes(pu.len, width) : 0u, 0u, 0u, 0u };
      if (i < r1)
        { mine.to  = out_off[i];
          mine.adj = (uint32_t) ((uintptr_t) (out + mine.to) & 15u);
        }
      if (!NARROW && mine.T >= 16u)
        { mine.endl = (mine.T - 16u) / W1;
          mine.endc = (mine.T - 16u) - mine.endl * W1;
        }
      const bool brief = pu.ok && mine.T + mine.adj <= LN_SHORT;

      // the short ones: lanes 16 g .. 16 g + 15 take unit k + g
      units_by_fours(__ballot(brief), [&](int from, bool its)
        { ln_unit u;
          u.at   = __shfl(mine.at, from);
          u.to   = __shfl(mine.to, from);
          u.beg  = __shfl(mine.beg, from);
          u.len  = __shfl(mine.len, from);
          u.T    = __shfl(mine.T, from);
          u.adj  = __shfl(mine.adj, from);
          u.endl = __shfl(mine.endl, from);
          u.endc = __shfl(mine.endc, from);
          if (its && q_grp < u.T + u.adj)
            { if (u.T >= 16u)
                { const ln_chunk c = ln_where<NARROW>(u, q_grp, ln_back(at_grp, u.adj, W1), W1);
                  ln_put<LETTERS, NARROW>(s_quad, in_bytes, out, u, c, ln_ask(in, in_bytes, c.a), width);
                }
              else if (q_grp == 0u) ln_small<LETTERS>(in, out, u, width);
            }
        });

      // the others: the whole wave, 1 KiB of the frame a step
      units_each(__ballot(pu.ok && !brief), [&](int from)
        { ln_unit u;
          u.at   = uniform64(__shfl(mine.at, from));
          u.to   = uniform64(__shfl(mine.to, from));
          u.beg  = uniform(__shfl(mine.beg, from));
          u.len  = uniform(__shfl(mine.len, from));
          u.T    = uniform(__shfl(mine.T, from));
          u.adj  = uniform(__shfl(mine.adj, from));
          u.endl = uniform(__shfl(mine.endl, from));
          u.endc = uniform(__shfl(mine.endc, from));
          const uint32_t TS = u.T + u.adj;                 // the frame's bytes
          // As in k_reads_unpack: a step's packed bytes are asked for a step before its letters are made and stored, in two
          // registers that take turns.  A wave's loads and stores are counted together and retire in order; in the steps in which
          // every lane has a chunk (all but a unit's last) each step issues exactly one load and one store, and behind "ask for
          // the next step" the wait is for all but the two youngest operations -- that request and the store of the step before.
          // The first of these steps stands in front of the loop, so that the loop is entered as it is gone round.  The waits
          // written here only say what the compiler could count itself; its own stay sufficient whatever these say.  Behind the
          // frame ln_where gives the last chunk once more: asked for, never used.
          // p: the place of this lane's chunk in the step that is asked for next.
          const uint32_t full = TS & ~(DX_STEP - 1u);      // the frame's bytes in whole steps
          uint32_t q = 16u * lane, base = 0;
          ln_pos   p = ln_back(at_wave, u.adj, W1);
          ln_chunk cA = ln_where<NARROW>(u, q, p, W1), cB = cA;
          uint64_t rawA = ln_ask(in, in_bytes, cA.a), rawB = 0;
          p = ln_moved(p, dline, dcol, W1);
          if (full != 0u)
            { cB = ln_where<NARROW>(u, q + DX_STEP, p, W1); rawB = ln_ask(in, in_bytes, cB.a);
              p  = ln_moved(p, dline, dcol, W1);
              ln_put<LETTERS, NARROW>(s_quad, in_bytes, out, u, cA, rawA, width);
              for (base = DX_STEP; base + 2u * DX_STEP <= full; base += 2u * DX_STEP)
                { cA = ln_where<NARROW>(u, q + base + DX_STEP, p, W1); rawA = ln_ask(in, in_bytes, cA.a);
                  p  = ln_moved(p, dline, dcol, W1);
                  __builtin_amdgcn_s_waitcnt(0x0F72);      // vmcnt(2)
                  ln_put<LETTERS, NARROW>(s_quad, in_bytes, out, u, cB, rawB, width);
                  cB = ln_where<NARROW>(u, q + base + 2u * DX_STEP, p, W1); rawB = ln_ask(in, in_bytes, cB.a);
                  p  = ln_moved(p, dline, dcol, W1);
                  __builtin_amdgcn_s_waitcnt(0x0F72);
                  ln_put<LETTERS, NARROW>(s_quad, in_bytes, out, u, cA, rawA, width);
                }
              cA = cB; rawA = rawB;
            }
          // what is left: a whole step at most, and the last, partial one (cA, rawA: the step at base)
          for (; base < TS; base += DX_STEP)
            { const ln_chunk cN = ln_where<NARROW>(u, q + base + DX_STEP, p, W1);
              const uint64_t ahead = ln_ask(in, in_bytes, cN.a);
              p = ln_moved(p, dline, dcol, W1);
              if (q + base < TS) ln_put<LETTERS, NARROW>(s_quad, in_bytes, out, u, cA, rawA, width);
              cA = cN; rawA = ahead;
            }
        });
    });
}

template <int LETTERS>
static void lines_launch(dx_ctx *ctx, int grid, const uint8_t *d_in, uint64_t in_bytes, uint64_t bound, const uint64_t *d_boff,
                         const uint32_t *d_beg, const uint32_t *d_len, uint64_t n, uint32_t width, uint8_t *d_out,
                         const uint64_t *d_out_off, const units_frame &f)
{ if (width < 16u)
    hipLaunchKernelGGL((k_reads_unpack_lines<LETTERS, true>), dim3(grid), dim3(DX_BLOCK), 0, ctx->stream,
                       d_in, in_bytes, bound, d_boff, d_beg, d_len, n, width, d_out, d_out_off, f.bad, f.ticket);
  else
    hipLaunchKernelGGL((k_reads_unpack_lines<LETTERS, false>), dim3(grid), dim3(DX_BLOCK), 0, ctx->stream,
                       d_in, in_bytes, bound, d_boff, d_beg, d_len, n, width, d_out, d_out_off, f.bad, f.ticket);
}

extern "C" int dx_reads_unpack_lines(dx_ctx *ctx, int letters, const uint8_t *d_in, uint64_t in_bytes,
                                     const uint64_t *d_boff, const uint32_t *d_beg, const uint32_t *d_len,
                                     uint64_t n, uint32_t width, uint8_t *d_out, const uint64_t *d_out_off, uint64_t *bad_unit)
{ if (ctx == NULL) return DX_E_ARG;
  if (bad_unit) *bad_unit = UINT64_MAX;
  if (letters < DX_LETTERS_LOWER || letters > DX_LETTERS_ARROW)
    return dx_fail(ctx, DX_E_ARG, "dx_reads_unpack_lines: letter set %d has no lines (lower, upper or arrow letters)", letters);
  if (width == 0)
    return dx_fail(ctx, DX_E_ARG, "dx_reads_unpack_lines: line width must be >= 1 "
                                  "(the reference loops forever on -w0, undexta.c:265)");
  if (n == 0) return DX_OK;
  if (width > LN_WIDTH_MOST) width = LN_WIDTH_MOST;          // (the same text: no unit has that many symbols)
  units_frame    f;
  uint64_t       back[UF_OUT];
  const uint64_t bound = in_bytes;                         // (the kernel loads 8 bytes at a time: fewer are copied, zeros behind them)
  int rc = units_begin(ctx, "dx_reads_unpack_lines", n, d_boff && d_len && d_out && d_out_off && (d_in || !in_bytes),
                       ctx->d_u64 + DXW_UNITS, 0, 8, &d_in, &in_bytes, &f);
  if (rc != DX_OK) return rc;
  // (units per ticket from the output's extent: outputs that do not stand in the units' order give a figure that means
  //  nothing, and the bounds of ticket_units_of hold)
  hipLaunchKernelGGL(k_ticket_units, dim3(1), dim3(1), 0, ctx->stream, d_out_off, d_out_off + (n - 1), d_len + (n - 1), n,
                     LN_BATCH * 10000u, LN_BATCH, f.ticket);
  const int grid = dx_grid_waves(ctx, n, 32);
  switch (letters)
    { case DX_LETTERS_LOWER:
        lines_launch<DX_LETTERS_LOWER>(ctx, grid, d_in, in_bytes, bound, d_boff, d_beg, d_len, n, width, d_out, d_out_off, f);
        break;
      case DX_LETTERS_UPPER:
        lines_launch<DX_LETTERS_UPPER>(ctx, grid, d_in, in_bytes, bound, d_boff, d_beg, d_len, n, width, d_out, d_out_off, f);
        break;
      default:
        lines_launch<DX_LETTERS_ARROW>(ctx, grid, d_in, in_bytes, bound, d_boff, d_beg, d_len, n, width, d_out, d_out_off, f);
        break;
    }
  return units_end(ctx, f, back, bad_unit, "%s: unit %llu does not lie inside the %llu packed bytes", bound);
}
