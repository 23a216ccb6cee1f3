// dx_words.h -- the 64 words of ctx->d_u64 (dx_ctx.hip allocates them), every one with its owner.
//
// This is where to look for a free word.  The files in the evidence set of profiles/ (csrc/*.hip, csrc/*.hpp) still address
// their words by the bare numbers given here and keep them until that set is next re-made: change a number here and there
// together.  The files under verify/, reads/, digest/ and census/ use the names.
#pragma once

enum
{ DXW_QV_KEY      = 0,     // dx_qv.hip: k_qv_prescan_del's key (dx_qv_prescan, dx_qv_scan)                      1: free
  DXW_QV_SUB      = 2,     // dx_qv.hip: k_qv_prescan_sub's two words, 2 and 3                                   4 .. 7: free
  DXW_INDEX_ERR   = 8,     // dx_index.hip: the first line that is malformed                                     9 .. 15: free
  DXW_DEC_NEXT    = 16,    // dx_qv_decode.hip: task counter
  DXW_HIST_TICKET = 17,    // dx_qv.hip: dx_qv_hist, dx_qv_scan
  DXW_SIZE_TICKET = 18,    // dx_qv.hip: dx_qv_sizes
  DXW_ENC_TICKET  = 19,    // dx_qv.hip: encode_text, onepass_direct; dx_qv_short.hpp
  DXW_PACK_TICKET = 20,    // dx_pack2.hip: dx_pack2_encode
  DXW_UNPK_TICKET = 21,    // dx_pack2.hip: dx_pack2_decode
  DXW_SIZE_TICK2  = 22,    // dx_qv.hip: onepass_direct; dx_qv_short.hpp                                         23: free
  DXW_REC_BASE    = 24,    // dx_qv.hip: onepass_direct's running record offset, 24 and 25                       26 .. 28: free
  DXW_DEC_NEXT4   = 29,    // dx_qv_decode.hip: task counters
  DXW_DEC_NEXT3   = 30,
  DXW_DEC_NEXT2   = 31,
  DXW_UNITS       = 32,    // units/dx_units.hpp: the range kernels' frame, 32 .. 39 (ticket, bad unit, 16 bytes of padded input, four
                           //   answer words), shared by verify/, reads/, digest/ and census/: each call synchronises before it returns
  DXW_QS_WORK     = 40,    // dx_qv_short.hpp: the survey's eight 32-bit figures, 40 .. 43                       44 .. 47: free
  DXW_DENSITY     = 48,    // dx_qv.hip: k_qv_density's four words and the share chosen, 48 .. 52                53 .. 55: free
  DXW_SCAN_DEV    = 56,    // dx_qv.hip: scan_dev, 56 .. 59                                                      60 .. 63: free
  DXW_COUNT       = 64
};
