// What more than one of the split-operand convolution units needs (conv_bf.hip: forward / data gradient, conv_up2.hip: the fused
// decoder operator, conv_wgrad.hip: the weight gradient).  Anything only one of them uses stays in that file.
#pragma once
#include "common.h"

namespace {
typedef kmh_f32x16 f32x16;
typedef kmh_bf16x8 bf16x8;     // 8 x 16-bit fragment (bf16 or fp16 bits; see common.h for the split arithmetic)
typedef __attribute__((address_space(3))) void* kmh_lds_ptr;           // operands of __builtin_amdgcn_global_load_lds (LDS-DMA)
typedef const __attribute__((address_space(1))) void* kmh_glb_ptr;

constexpr int KC = 8;              // channels per LDS refill (= half of the MFMA K)

// padded width of the packed filters' cout axis (whole 64- or 128-wide N tiles)
static inline int cout_pad(int Cout) { return Cout > 64 ? (Cout + 127) & ~127 : (Cout + 63) & ~63; }
}  // namespace
