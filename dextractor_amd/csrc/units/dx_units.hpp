// dx_units.hpp -- what the range kernels share (verify/, reads/, digest/, census/): n units of a device buffer, drawn by ticket,
// checked, dealt to a lane, to 16 lanes or to the wave; and the one frame of device words and host calls around such a kernel.
// What a kernel does with a unit's chunks stays in its own file.  (Outside the evidence set of profiles/, as those files are.)
#pragma once

#include "dx_internal.hpp"
#include "dx_device.hpp"
#include "dx_words.h"

extern "C" {
#include "dx_host.h"
}

#define UNITS_GROUP   16u                  // lanes that take a short unit together
#define UNITS_LEN_MAX 0x7fffffffu          // symbols a packed unit (DAZZ_READ.rlen is an int); more are refused like a unit out of bounds

// ---- the loops -----------------------------------------------------------------------------------------------------
// Tickets of `per` consecutive units until the n are gone: body(r0, r1) a ticket.  AHEAD: the next ticket is drawn before the
// body, hidden behind its units.
template <bool AHEAD, typename F>
__device__ __forceinline__ void units_tickets(uint32_t *ticket, uint32_t per, uint64_t n, F &&body)
{ for (uint64_t r0 = next_unit(ticket, per), nxt = 0; r0 < n; r0 = nxt)
    { if (AHEAD) nxt = next_unit(ticket, per);
      body(r0, r0 + per < n ? r0 + per : n);
      if (!AHEAD) nxt = next_unit(ticket, per);
    }
}

// ... a ticket's units 64 a round, unit u0 + lane the lane's to read and to check while it is below r1: body(u0, r1)
template <bool AHEAD, typename F>
__device__ __forceinline__ void units_rounds(uint32_t *ticket, uint32_t per, uint64_t n, F &&body)
{ units_tickets<AHEAD>(ticket, per, n, [&](uint64_t r0, uint64_t r1)
    { for (uint64_t u0 = r0; u0 < r1; u0 += 64u) body(u0, r1); });
}

// the set bits of a (uniform) mask, lowest first: body(from) -- a round's long units, one after the other by the whole wave
template <typename F>
__device__ __forceinline__ void units_each(uint64_t mask, F &&body)
{ while (mask)
    { const int from = __ffsll((unsigned long long) mask) - 1;
      mask &= mask - 1u;
      body(from);
    }
}

// a round's short units FOUR A STEP: lanes 16 g .. 16 g + 15 get unit k + g.  body(from, mine) -- mine: that unit is one of them
template <typename F>
__device__ __forceinline__ void units_by_fours(uint64_t briefs, F &&body)
{ const uint32_t grp = (uint32_t) lane_id() / UNITS_GROUP;
  for (uint32_t k = 0; k < 64u; k += 64u / UNITS_GROUP)
    if ((briefs >> k) & ((1ull << (64u / UNITS_GROUP)) - 1u))
      { const int from = (int) (k + grp);
        body(from, ((briefs >> from) & 1ull) != 0ull);
      }
}

// ---- the bounds rules, and a packed unit's intake ------------------------------------------------------------------
// symbols [beg, beg + len) of the packed read at byte `at` (four a byte) lie inside `bound` bytes
__device__ __forceinline__ bool packed_unit_ok(uint64_t at, uint32_t beg, uint32_t len, uint64_t bound)
{ return at <= bound && len <= UNITS_LEN_MAX && (len == 0u || (((uint64_t) beg + len - 1u) >> 2) < bound - at); }

// bytes [off, off + len) lie inside `bound` bytes
__device__ __forceinline__ bool range_ok(uint64_t off, uint64_t len, uint64_t bound)
{ return off <= bound && len <= bound - off; }

struct packed_unit { uint64_t at; uint32_t beg, len; bool ok; };

// unit i of a round that ends at r1 (beg NULL: from symbol 0); the smallest index that is refused goes to *bad
__device__ __forceinline__ packed_unit packed_unit_take(const uint64_t *boff, const uint32_t *beg, const uint32_t *len,
                                                        uint64_t i, uint64_t r1, uint64_t bound, unsigned long long *bad)
{ packed_unit u = { 0ull, 0u, 0u, false };
  if (i < r1)
    { u.at = boff[i]; u.beg = beg != NULL ? beg[i] : 0u; u.len = len[i];
      u.ok = packed_unit_ok(u.at, u.beg, u.len, bound);
      if (!u.ok) atomicMin(bad, (unsigned long long) i);
    }
  return u;
}

// the sum along a row of 16 lanes, in the row's last lane (the first four steps of wave_incl_scan)
__device__ __forceinline__ uint32_t row_sum(uint32_t v)
{ v += __builtin_amdgcn_update_dpp(0u, v, 0x111, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0u, v, 0x112, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0u, v, 0x114, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0u, v, 0x118, 0xf, 0xf, true);
  return v;
}

// 16 bytes at byte `a` of a buffer of `bytes` >= 16: its last 16 when they would reach past its end
__device__ __forceinline__ uint64_t last16_from(uint64_t a, uint64_t bytes) { return a + 16u > bytes ? bytes - 16u : a; }
__device__ __forceinline__ u32x4 last16_ask(const uint8_t *in, uint64_t bytes, uint64_t a)
{ return *(const u32x4_u *) (in + last16_from(a, bytes)); }

// the 8 bytes at byte o of the buffer (bytes >= 8) as a word in the read's bit order (the first symbol on top); what lies behind the
// buffer's end reads as zero, and the 8 bytes that would reach past it are its last 8, moved up
__device__ __forceinline__ uint64_t be64_at(const uint8_t *in, uint64_t bytes, uint64_t o)
{ if (o + 8u <= bytes) return __builtin_bswap64(*(const u64_u *) (in + o));
  if (o >= bytes) return 0ull;
  return __builtin_bswap64(*(const u64_u *) (in + (bytes - 8u))) << (8u * (uint32_t) (o + 8u - bytes));
}

// the chunk whose place is byte a < bytes of the buffer (bytes >= 16) and the 8 bytes behind it, as three such words
__device__ __forceinline__ void chunk_words(const uint8_t *in, uint64_t bytes, uint64_t a, uint64_t &w0, uint64_t &w1, uint64_t &w2)
{ const u32x4    v    = last16_ask(in, bytes, a);
  const uint32_t back = (uint32_t) (a - last16_from(a, bytes));              // 0, or how many bytes in front of a the 16 begin
  const uint64_t h = __builtin_bswap64(v.x | ((uint64_t) v.y << 32)), l = __builtin_bswap64(v.z | ((uint64_t) v.w << 32));
  if (back == 0u)      { w0 = h; w1 = l; w2 = be64_at(in, bytes, a + 16u); }
  else if (back < 8u)  { w0 = (h << (8u * back)) | (l >> (64u - 8u * back)); w1 = l << (8u * back); w2 = 0ull; }
  else                 { w0 = l << (8u * (back - 8u)); w1 = 0ull; w2 = 0ull; }
}

// the sum along a row of 16 lanes of a 64-bit value, in every lane of the row
__device__ __forceinline__ uint64_t row_sum64(uint64_t v)
{
  #pragma unroll
  for (int d = 8; d > 0; d >>= 1) v += (uint64_t) __shfl_xor((unsigned long long) v, d);
  return v;
}

// the sum of a 64-bit value over the wave, in every lane
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v)
{
  #pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += (uint64_t) __shfl_xor((unsigned long long) v, d);
  return v;
}

// ---- the call frame ------------------------------------------------------------------------------------------------
// A frame's 64-bit words on the device: the ticket (2 x 32 bits: the counter, k_ticket_units' units a ticket), the smallest
// index of a refused unit, 16 bytes for an input shorter than the kernel's loads, and the call's answer words behind them.
enum { UF_TICKET = 0, UF_BAD = 1, UF_PAD = 2, UF_OUT = 4 };

struct units_frame
{ uint32_t           *ticket;
  unsigned long long *bad, *out;
  size_t              words;               // UF_OUT + the answer's
  const char         *who;
};

// The checks every entry point makes of n > 0 units (have: none of its pointers is missing), then the frame at d_w -- NULL: at
// the head of a dx_scratch block, for an answer the context's own frame (out_words <= 4) does not hold -- zeroed, its bad-unit
// word all ones, and an input of fewer than `least` bytes (0, 8 or 16: what the kernel loads at a time) moved into the pad
// (least 0: d_in and in_bytes may be NULL).
static int units_begin(dx_ctx *ctx, const char *who, uint64_t n, bool have, uint64_t *d_w, size_t out_words, uint32_t least,
                       const uint8_t **d_in, uint64_t *in_bytes, units_frame *f)
{ if (n >= (1ull << 31)) return dx_fail(ctx, DX_E_ARG, "%s: more than 2^31 - 1 units in one batch", who);
  if (!have) return dx_fail(ctx, DX_E_ARG, "%s: NULL device pointer", who);
  DX_HIP(ctx, hipSetDevice(ctx->device));
  int rc = dx_after_pending(ctx);
  if (rc != DX_OK) return rc;
  f->words = UF_OUT + out_words; f->who = who;
  if (d_w == NULL && (rc = dx_scratch(ctx, f->words * 8u, (void **) &d_w)) != DX_OK) return rc;
  f->ticket = (uint32_t *) (d_w + UF_TICKET);
  f->bad = (unsigned long long *) (d_w + UF_BAD); f->out = (unsigned long long *) (d_w + UF_OUT);
  DX_HIP(ctx, hipMemsetAsync(d_w, 0, f->words * 8u, ctx->stream));
  DX_HIP(ctx, hipMemsetAsync(f->bad, 0xff, 8, ctx->stream));
  if (least && *in_bytes < least)
    { if (*in_bytes) DX_HIP(ctx, hipMemcpyAsync(d_w + UF_PAD, *d_in, *in_bytes, hipMemcpyDeviceToDevice, ctx->stream));
      *d_in = (const uint8_t *) (d_w + UF_PAD); *in_bytes = least;
    }
  return DX_OK;
}

// The same for an entry point that may list: ONE scratch block with the frame and out_words answer words in front and, when
// `places`, every unit's first place in the list behind them (*d_start: n + 1 words; NULL without) and, when the caller brings no
// counts (*d_room == NULL), a room[n] of its own, which *d_room then names.
static int units_list_begin(dx_ctx *ctx, const char *who, uint64_t n, bool have, size_t out_words, uint32_t least, bool places,
                            const uint8_t **d_in, uint64_t *in_bytes, units_frame *f, uint64_t **d_start, uint32_t **d_room)
{ uint64_t    *d_w   = NULL;
  const size_t words = UF_OUT + out_words;
  const bool   own   = places && *d_room == NULL;
  DX_HIP(ctx, hipSetDevice(ctx->device));
  const int rc = dx_scratch(ctx, (words + (places ? n + 1u : 0u) + (own ? (n + 1u) / 2u : 0u)) * 8u, (void **) &d_w);
  if (rc != DX_OK) return rc;
  *d_start = places ? d_w + words : NULL;
  if (own) *d_room = (uint32_t *) (*d_start + n + 1u);
  return units_begin(ctx, who, n, have, d_w, out_words, least, d_in, in_bytes, f);
}

// Between the counting launch and the listing launch: d_room[n] summed to every unit's first place, *listed what the list holds
// (one read-back), and, when it holds anything, the ticket counter back at 0 for the second walk over the units.
static int units_list_places(dx_ctx *ctx, const units_frame &f, const uint32_t *d_room, uint64_t n, uint64_t *d_start, uint64_t *listed)
{ DX_HIP(ctx, hipGetLastError());
  const int rc = dx_scan_u32(ctx, d_room, n, d_start, listed);
  if (rc != DX_OK) return rc;
  if (*listed) DX_HIP(ctx, hipMemsetAsync(f.ticket, 0, 4, ctx->stream));     // (the counter; the units a ticket stay)
  return DX_OK;
}

// Behind the launches: the frame and the answer read back into back[0 .. f.words) in one copy, the stream synchronised, and a
// refused unit turned into DX_E_FORMAT -- fmt words it, from (who, unit, bound, extra).
static int units_end(dx_ctx *ctx, const units_frame &f, uint64_t *back, uint64_t *bad_unit, const char *fmt, uint64_t bound, int extra = 0)
{ DX_HIP(ctx, hipGetLastError());
  DX_HIP(ctx, hipMemcpyAsync(back, f.ticket, f.words * 8u, hipMemcpyDeviceToHost, ctx->stream));
  DX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (back[UF_BAD] == UINT64_MAX) return DX_OK;
  if (bad_unit) *bad_unit = back[UF_BAD];
  return dx_fail(ctx, DX_E_FORMAT, fmt, f.who, (unsigned long long) back[UF_BAD], (unsigned long long) bound, extra);
}
