// dx_kmer_index.hip -- a set of k-mers that remembers WHERE on the reference each k-mer stands: the index that dx_code_kmer_seeds
// (place/dx_place_seeds.hip) turns the windows of packed reads into seeds with.
//
//   dx_code_kmer_index    the units of a packed buffer are the targets                                        (k_ix_keys, k_ix_narrow)
//   dx_kmer_index_info / _set / _targets / _positions / _free
//
// The reference is T targets one behind the other: toff = the exclusive sums of their lengths, G = toff[T] < 2^31, the window at
// g = toff[t] + p exists for 0 <= p <= l_t - k and never spans two targets.  The index is a COUNTED dx_kmer_set of those windows
// (screen/dx_kmer_set.hip: codes ascending, count[i] = the occurrences, the bucket index as it is), start[0 .. n] = the exclusive sums
// of the counts as 32-bit words, and pos[start[i] .. start[i + 1]) = the occurrences of code i as g << 1 | flip, ascending in g.
// flip = (rc < fwd) with canonical -- the code kept is the reverse strand's --, 0 without and for a k-mer that is its own reverse
// complement.
//
// The build, all by calls that exist: dx_code_kmer_codes writes every window's code, dx_sort_u64 (2 k bits) sorts them,
// dx_kmer_set_from_sorted_counted (min_count 1) makes the set, dx_scan_u32 sums its counts and k_ix_narrow keeps the low words as
// start.  New is k_ix_keys: kc_walk over the targets (kmers/dx_kmer_windows.hpp, as k_depths; a unit's first
// window's place and its first symbol's global position travel with it), sc_places for the place of every window's
// code in the set that was just made, and one 8-byte store a window at off[t] + p -- the place where dx_code_kmer_codes put its code,
// the array is used again -- of the key  place << 32 | g << 1 | flip.  A second kc_roll over the same part gives the flip: after
// code() kc_roll<true> holds the reverse strand's code in rcw and the forward one in w0 >> down (kmers/dx_kmer_windows.hpp is not
// changed).  The kernel's units are pieces of the targets, 4096 windows each, made on the host (kx_keys): the walk gives a unit to
// one wave at the most, and a reference is a few long targets.  dx_sort_u64 over 32 + bits(n - 1) bits orders the keys by place
// and, inside a place, by g; the sort has no payload and needs none.  k_ix_narrow keeps the low words as pos.  The codes' array and the sort's second one are freed: while it is built an
// index takes 16 bytes a window beside itself, afterwards 12 a distinct code, 4 a window and the bucket index.
//
// NOT built: an index over 2^31 symbols or more (DX_E_ARG names the size: g << 1 | flip is one 32-bit word, and a seed's gpos too);
// per-target anything -- the positions are global, toff on the host says which target one lies in.
//
// ESTIMATE (before the first run; the references of tools/screen_rate.py).  Per window: the codes 8 bytes written, the first sort
// ceil(2 k / 8) = 6 passes of 16 bytes read and written at k = 21, the keys one look-up and 8 bytes, the second sort 4 + ceil(bits(n -
// 1) / 8) = 7 or 8 passes.  The sorts dominate: 14 passes against dx_file_kmer_set_counted's 6, so 2.3 to 2.5 times that call's
// time; with dx_sort_u64 at about 1 ms a pass for 10^8 keys (profiles/kmers_wide_rate.txt's order), 15 to 20 ms for the 10^8-code
// reference, and launches alone (under 1 ms) for the phage.
// MEASURED (profiles/place_rate.txt, the fastest of two builds after a warm-up): 1.6 ms for the phage (4.8 x 10^4 symbols), 9.1 ms
// for 5 x 10^6, 135 ms for 10^8: 7 to 9 times the estimate.  The passes were costed at 1 ms for 10^8 keys; the vote's sort of the
// same run takes 8 ms a pass for 10^9 keys, and beside the 14 passes stand the set's two counting passes and its run list.  The
// first run took 2971 ms for the 10^8-symbol reference: its one target was one wave's; that is what the pieces are for.
//
// This file stands outside the evidence set of profiles/ (profiles/check.py hashes csrc/*.hip); its kernels have no entry in the
// profiler's name table and are timed with events on the context's stream (tools/place_rate.py).
#include "screen/dx_screen_look.hpp"
#include "place/dx_kmer_index.hpp"

#include <stdlib.h>
#include <string.h>
#include <new>

#define KX_KMAX 32u

// ---------------------------------------------------------------------------------------------
//  k_ix_keys, k_ix_narrow
// ---------------------------------------------------------------------------------------------
// the part's keys, one behind the other from out[0] on; g0: the global position of the part's first window
template <bool CANON>
__device__ __forceinline__ void ix_write(const kc_part &p, const sc_set &s, uint32_t g0, uint64_t *out)
{ if (p.n == 0u) return;
  kc_roll<CANON> r(p, s.k), q(p, s.k);                     // r: the look-ups'; q: the same windows once more, for the flip
  for (uint32_t i0 = 0; i0 < p.n; i0 += SC_BATCH)
    { uint32_t at[SC_BATCH];
      sc_places<CANON>(r, s, at);
      #pragma unroll
      for (uint32_t t = 0; t < SC_BATCH; t++)
        { uint32_t flip = 0u;
          if (CANON)
            { (void) q.code();
              flip = q.rcw < (q.w0 >> q.down) ? 1u : 0u;
              q.step();
            }
          if (i0 + t < p.n) out[i0 + t] = ((uint64_t) at[t] << 32) | (uint64_t) (((g0 + i0 + t) << 1) | flip);
        }
    }
}

// in holds in_bytes bytes and 16 at least; the units are checked against `bound`.  off: every target's first window's place (the
// exclusive sums of max(0, len - k + 1)), toff: its first symbol's global position; key holds off[n] words at least.
template <bool CANON>
__global__ __launch_bounds__(DX_BLOCK)
void k_ix_keys(const uint8_t *__restrict__ in, uint64_t in_bytes, uint64_t bound, const uint64_t *__restrict__ boff,
               const uint32_t *__restrict__ beg, const uint32_t *__restrict__ len, uint64_t n, sc_set s,
               const uint64_t *__restrict__ off, const uint64_t *__restrict__ toff, uint64_t *__restrict__ key,
               unsigned long long *__restrict__ bad, uint32_t *__restrict__ ticket)
{ const uint32_t lane = (uint32_t) lane_id();
  units_rounds<false>(ticket, ticket_units_of(ticket, KC_BATCH), n, [&](uint64_t u0, uint64_t r1)
    { // unit u0 + lane is this lane's to read and to check; its first window's place and its first symbol's global position travel with it
      const uint64_t    i  = u0 + lane;
      const packed_unit pu = packed_unit_take(boff, beg, len, i, r1, bound, bad);
      const kc_unit     e  = kc_unit_of(pu, s.k);
      const kc_place    at = { e.nch ? off[i] : 0ull, e.nch ? (uint32_t) toff[i] : 0u };
      kc_walk(e, at, [&](uint64_t a, const kc_unit &u, const kc_place &to)
        { const kc_part p = kc_take(in, in_bytes, a, u.S0, u.S1, s.k);
          ix_write<CANON>(p, s, to.g + p.first, key + to.to + p.first);
        });
    });
}

// out[i] = the low word of in[i]
__global__ __launch_bounds__(DX_BLOCK)
void k_ix_narrow(const uint64_t *__restrict__ in, uint64_t n, uint32_t *__restrict__ out)
{ const uint64_t i = (uint64_t) blockIdx.x * DX_BLOCK + threadIdx.x;
  if (i < n) out[i] = (uint32_t) in[i];
}

// ---------------------------------------------------------------------------------------------
//  the entry points
// ---------------------------------------------------------------------------------------------
static_assert(sizeof(dx_index_info) == 56, "dx_index_info is 56 bytes");

extern "C" int dx_kmer_index_free(dx_ctx *ctx, dx_kmer_index *x)
{ if (ctx == NULL) return DX_E_ARG;
  if (x == NULL) return DX_OK;
  if (x->set) (void) dx_kmer_set_free(ctx, x->set);
  if (x->d_start) (void) dx_free(ctx, x->d_start);
  if (x->d_pos) (void) dx_free(ctx, x->d_pos);
  free(x->toff);
  delete x;
  return DX_OK;
}

static int kx_narrow(dx_ctx *ctx, const uint64_t *d_in, uint64_t n, uint32_t *d_out)
{ if (n == 0) return DX_OK;
  hipLaunchKernelGGL(k_ix_narrow, dim3((unsigned) ((n + DX_BLOCK - 1u) / DX_BLOCK)), dim3(DX_BLOCK), 0, ctx->stream, d_in, n, d_out);
  DX_HIP(ctx, hipGetLastError());
  return DX_OK;
}

#define KX_PIECE 4096u                     // windows a piece: a long target is dealt to the waves in pieces of so many (one step of the wave path)

// The keys of every window into d_key (the codes' array, used again).  h_off, h_toff: the host's sums, n + 1 each; h_boff, h_beg (NULL:
// all 0), h_len: the targets as the host has read them.  k_ix_keys deals a unit to ONE wave at the most, and a reference is a few
// long targets, not many short ones: so the kernel's units are PIECES of the targets, KX_PIECE windows each (the last one of a target
// fewer), piece j of target t being symbols [j KX_PIECE, j KX_PIECE + KX_PIECE + k - 1) of it with its own first window's place and
// global position; the whole bytes of a piece's first symbol go into its byte offset, so that d_beg stays below 4.
static int kx_keys(dx_ctx *ctx, const char *who, const uint8_t *d_in, uint64_t in_bytes, uint64_t n, const dx_kmer_set *set,
                   const uint64_t *h_off, const uint64_t *h_toff, const uint64_t *h_boff, const uint32_t *h_beg, const uint32_t *h_len,
                   uint64_t *d_key)
{ const uint32_t k = set->k;
  uint64_t pieces = 0;
  for (uint64_t t = 0; t < n; t++) pieces += (h_off[t + 1u] - h_off[t] + KX_PIECE - 1u) / KX_PIECE;
  if (pieces == 0) return DX_OK;
  if (pieces >= (1ull << 31)) return dx_fail(ctx, DX_E_ARG, "%s: %llu pieces of targets (fewer than 2^31)", who, (unsigned long long) pieces);
  // one host block and one device block: off, toff, boff (8 bytes a piece each), then beg and len (4 each)
  uint64_t *h = (uint64_t *) malloc((size_t) pieces * 32u);
  if (h == NULL) return dx_fail(ctx, DX_E_NOMEM, "%s: out of memory", who);
  uint64_t *p_off = h, *p_toff = h + pieces, *p_boff = h + 2u * pieces;
  uint32_t *p_beg = (uint32_t *) (h + 3u * pieces), *p_len = p_beg + pieces;
  uint64_t at = 0;
  for (uint64_t t = 0; t < n; t++)
    { const uint64_t w = h_off[t + 1u] - h_off[t];
      for (uint64_t w0 = 0; w0 < w; w0 += KX_PIECE, at++)
        { const uint64_t first = (uint64_t) (h_beg ? h_beg[t] : 0u) + w0, take = w - w0 < KX_PIECE ? w - w0 : KX_PIECE;
          p_off[at] = h_off[t] + w0; p_toff[at] = h_toff[t] + w0;
          p_boff[at] = h_boff[t] + (first >> 2); p_beg[at] = (uint32_t) (first & 3u);
          p_len[at] = (uint32_t) (take + k - 1u);
        }
    }
  uint64_t *d = NULL;
  int rc = dx_malloc(ctx, (size_t) pieces * 32u + 64u, (void **) &d);
  if (rc == DX_OK) rc = dx_h2d(ctx, d, h, (size_t) pieces * 32u);
  free(h);
  if (rc == DX_OK)
    rc = [&]() -> int
      { const uint64_t *d_off = d, *d_toff = d + pieces, *d_boff = d + 2u * pieces;
        const uint32_t *d_beg = (const uint32_t *) (d + 3u * pieces), *d_len = d_beg + pieces;
        units_frame    f;
        uint64_t       back[UF_OUT];
        const uint64_t bound = in_bytes;
        int r = units_begin(ctx, who, pieces, true, NULL, 0, 16, &d_in, &in_bytes, &f);
        if (r != DX_OK) return r;
        const sc_set s = sc_set_of(set);
        const int grid = dx_grid_waves(ctx, pieces, 16);
        kc_tickets(ctx, d_boff, pieces, f);
        if (set->canonical) hipLaunchKernelGGL(k_ix_keys<true>, dim3(grid), dim3(DX_BLOCK), 0, ctx->stream, d_in, in_bytes, bound, d_boff, d_beg,
                                               d_len, pieces, s, d_off, d_toff, d_key, f.bad, f.ticket);
        else                hipLaunchKernelGGL(k_ix_keys<false>, dim3(grid), dim3(DX_BLOCK), 0, ctx->stream, d_in, in_bytes, bound, d_boff, d_beg,
                                               d_len, pieces, s, d_off, d_toff, d_key, f.bad, f.ticket);
        return units_end(ctx, f, back, NULL, "%s: piece %llu of the targets does not lie inside the %llu packed bytes", bound);
      }();
  if (d) (void) dx_free(ctx, d);
  return rc;
}

extern "C" int dx_code_kmer_index(dx_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes,
                                  const uint64_t *d_boff, const uint32_t *d_beg, const uint32_t *d_len, uint64_t n,
                                  uint32_t k, int canonical, int arrow, dx_kmer_index **index)
{ const char *who = "dx_code_kmer_index";
  if (ctx == NULL) return DX_E_ARG;
  if (index == NULL) return dx_fail(ctx, DX_E_ARG, "%s: NULL pointer", who);
  *index = NULL;
  if (canonical && arrow) return dx_fail(ctx, DX_E_ARG, "%s: canonical: pulse widths have no complement (DX_KIND_FASTA only)", who);
  if (k < 1u || k > KX_KMAX) return dx_fail(ctx, DX_E_ARG, "%s: k = %u (1 to %u)", who, k, KX_KMAX);
  if (n >= (1ull << 31)) return dx_fail(ctx, DX_E_ARG, "%s: more than 2^31 - 1 targets", who);
  if (n && (d_boff == NULL || d_len == NULL || (d_in == NULL && in_bytes))) return dx_fail(ctx, DX_E_ARG, "%s: NULL device pointer", who);
  DX_HIP(ctx, hipSetDevice(ctx->device));

  // the targets' lengths come down: toff stays on the host, and the windows are known before anything is allocated
  uint64_t *h = (uint64_t *) malloc((size_t) (n + 1u) * 24u + (size_t) n * 8u + 16u);
  if (h == NULL) return dx_fail(ctx, DX_E_NOMEM, "%s: out of memory", who);
  uint64_t *h_toff = h, *h_off = h + n + 1u, *h_boff = h + 2u * (n + 1u);
  uint32_t *h_len = (uint32_t *) (h + 3u * (n + 1u)), *h_beg = d_beg != NULL ? h_len + n : NULL;
  dx_kmer_index *x = NULL;
  uint64_t *d_codes = NULL, *d_tmp = NULL, W = 0, got = 0, bad = UINT64_MAX, sum = 0;
  int rc = n ? dx_d2h(ctx, h_len, d_len, (size_t) n * 4u) : DX_OK;
  if (rc == DX_OK && n) rc = dx_d2h(ctx, h_boff, d_boff, (size_t) n * 8u);
  if (rc == DX_OK && n && h_beg) rc = dx_d2h(ctx, h_beg, d_beg, (size_t) n * 4u);
  if (rc != DX_OK) goto done;
  h_toff[0] = h_off[0] = 0;
  for (uint64_t t = 0; t < n; t++)
    { h_toff[t + 1u] = h_toff[t] + h_len[t];
      h_off[t + 1u] = h_off[t] + (h_len[t] >= k ? h_len[t] - k + 1u : 0u);
      if (h_toff[t + 1u] >= KX_GMAX)
        { rc = dx_fail(ctx, DX_E_ARG, "%s: a reference of %llu symbols and more by target %llu (fewer than 2^31: an index over more is not built)",
                       who, (unsigned long long) h_toff[t + 1u], (unsigned long long) t);
          goto done;
        }
    }
  W = h_off[n];

  x = new (std::nothrow) dx_kmer_index();
  if (x == NULL) { rc = dx_fail(ctx, DX_E_NOMEM, "%s: out of memory", who); goto done; }
  x->targets = n; x->windows = W;
  if ((x->toff = (uint64_t *) malloc((size_t) (n + 1u) * 8u)) == NULL) { rc = dx_fail(ctx, DX_E_NOMEM, "%s: out of memory", who); goto done; }
  memcpy(x->toff, h_toff, (size_t) (n + 1u) * 8u);

  // the counted set by the existing route
  if (W)
    { if ((rc = dx_malloc(ctx, (size_t) W * 8u + 64u, (void **) &d_codes)) != DX_OK) goto done;
      if ((rc = dx_malloc(ctx, (size_t) W * 8u + 64u, (void **) &d_tmp)) != DX_OK) goto done;
      if ((rc = dx_code_kmer_codes(ctx, d_in, in_bytes, d_boff, d_beg, d_len, n, k, canonical, d_codes, W, &got, &bad)) != DX_OK) goto done;
      if (got != W) { rc = dx_fail(ctx, DX_E_FORMAT, "%s: the targets' windows are not their lengths'", who); goto done; }
      if ((rc = dx_sort_u64(ctx, d_codes, d_tmp, W, 2u * k)) != DX_OK) goto done;
    }
  if ((rc = dx_kmer_set_from_sorted_counted(ctx, d_codes, W, 1, k, canonical, arrow, &x->set)) != DX_OK) goto done;

  // start: the counts' exclusive sums, narrowed (the sort's second array holds the 64-bit sums meanwhile: n + 1 <= W + 1 words)
  { const uint64_t nc = x->set->n;
    if ((rc = dx_malloc(ctx, (size_t) (nc + 1u) * 4u + 64u, (void **) &x->d_start)) != DX_OK) goto done;
    if ((rc = dx_malloc(ctx, (size_t) W * 4u + 64u, (void **) &x->d_pos)) != DX_OK) goto done;
    x->device_bytes = x->set->device_bytes + (nc + 1u) * 4u + W * 4u;
    if (nc == 0) { if ((rc = dx_memset(ctx, x->d_start, 0, 4)) != DX_OK) goto done; }
    else
      { if ((rc = dx_scan_u32(ctx, x->set->d_count, nc, d_tmp, &sum)) != DX_OK) goto done;
        if (sum != W) { rc = dx_fail(ctx, DX_E_HIP, "%s: the counts do not sum to the windows", who); goto done; }
        if ((rc = kx_narrow(ctx, d_tmp, nc + 1u, x->d_start)) != DX_OK) goto done;

        // pos: a key a window, sorted by place and position, the low words kept
        uint32_t bits = 0;
        while (bits < 32u && ((nc - 1u) >> bits) != 0u) bits++;
        if ((rc = kx_keys(ctx, who, d_in, in_bytes, n, x->set, h_off, h_toff, h_boff, h_beg, h_len, d_codes)) != DX_OK) goto done;
        if ((rc = dx_sort_u64(ctx, d_codes, d_tmp, W, 32u + bits)) != DX_OK) goto done;
        if ((rc = kx_narrow(ctx, d_codes, W, x->d_pos)) != DX_OK) goto done;
      }
    hipError_t e = hipStreamSynchronize(ctx->stream);      // (the two arrays are freed)
    if (e != hipSuccess) { rc = dx_fail(ctx, DX_E_HIP, "%s: %s", who, hipGetErrorString(e)); goto done; }
  }
  rc = DX_OK;

done:
  if (d_codes) (void) dx_free(ctx, d_codes);
  if (d_tmp) (void) dx_free(ctx, d_tmp);
  free(h);
  if (rc != DX_OK) { if (x) (void) dx_kmer_index_free(ctx, x); }
  else *index = x;
  return rc;
}

extern "C" int dx_kmer_index_info(const dx_kmer_index *x, dx_index_info *info)
{ if (x == NULL || info == NULL) return DX_E_ARG;
  info->codes = x->set->n; info->windows = x->windows; info->targets = x->targets; info->symbols = x->toff[x->targets];
  info->device_bytes = x->device_bytes;
  info->k = x->set->k; info->canonical = x->set->canonical; info->arrow = x->set->arrow; info->reserved = 0;
  return DX_OK;
}

extern "C" const dx_kmer_set *dx_kmer_index_set(const dx_kmer_index *x) { return x ? x->set : NULL; }

extern "C" const uint64_t *dx_kmer_index_targets(const dx_kmer_index *x, uint64_t *targets)
{ if (targets) *targets = x ? x->targets : 0;
  return x ? x->toff : NULL;
}

extern "C" int dx_kmer_index_positions(dx_ctx *ctx, const dx_kmer_index *x, uint32_t *start, uint64_t start_cap, uint32_t *pos, uint64_t pos_cap)
{ if (ctx == NULL) return DX_E_ARG;
  if (x == NULL || (start == NULL && start_cap) || (pos == NULL && pos_cap)) return dx_fail(ctx, DX_E_ARG, "dx_kmer_index_positions: NULL pointer");
  if ((start != NULL && start_cap < x->set->n + 1u) || (pos != NULL && pos_cap < x->windows))
    return dx_fail(ctx, DX_E_NOMEM, "dx_kmer_index_positions: %llu codes and %llu positions, and room for %llu and %llu",
                   (unsigned long long) x->set->n, (unsigned long long) x->windows, (unsigned long long) start_cap, (unsigned long long) pos_cap);
  int rc = DX_OK;
  if (start != NULL) rc = dx_d2h(ctx, start, x->d_start, (size_t) (x->set->n + 1u) * 4u);
  if (rc == DX_OK && pos != NULL && x->windows) rc = dx_d2h(ctx, pos, x->d_pos, (size_t) x->windows * 4u);
  return rc;
}

// dx_host.h: dx_file_place.c's refusals, worded there
extern "C" int dx_place_fail(dx_ctx *ctx, int code, const char *who, const char *what)
{ if (ctx == NULL) return code;
  return dx_fail(ctx, code, "%s: %s", who, what);
}
