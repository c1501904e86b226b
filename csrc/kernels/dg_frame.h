// The vocabulary of the board-resident 3x3 kernels (conv_stack2.hip, conv_layer2.hip,
// conv_stack_f8.hip, head_body.h): the 21x21 zero-bordered frame of a 19x19 board, its swizzled
// LDS image and the packed-bf16 epilogue arithmetic.  The one-letter names are the ones those
// kernels' index math is written in, so only they include this: the kernels of any frame size
// (conv_board.hip, conv_mfma.hip, head.hip) compute F from their padding, and the epilogue
// kinds EPI_* they share with these are in dg_common.h.
#pragma once
#include "dg_common.h"

namespace dg {

constexpr int F = 21;           // frame side: 19 + 2 * pad(1)
constexpr int FF = F * F;       // 441 frame rows (pixels)
constexpr int HROWS = 448;      // frame rows padded to whole 8-wave DMA rounds
constexpr int T = 9;            // taps of a 3x3 kernel

// swizzle signature of frame row f = 21 y + x: 16-B slot g of the row's 128 B lives at
// g ^ ((x + 3y) & 7)
DG_DEV int fsig(int f) { return ((f % F) + 3 * (f / F)) & 7; }
// frame-row offset of tap t = 3 ky + kx
DG_DEV int toff_of(int t) { return (t / 3 - 1) * F + (t % 3 - 1); }

// s_waitcnt lgkmcnt(0) (LDS writes of this wave done), vmcnt/expcnt untouched, then barrier:
// unlike __syncthreads() this does not drain the weight loads already in flight
DG_DEV void lds_barrier() {
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_s_barrier();
}

// two fp32 -> packed bf16 (RNE, v_cvt_pk_bf16_f32)
DG_DEV uint32_t bf16x2_bits(f32x2 v) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2v));
}
// ... then ReLU as a packed int16 max with 0 (v_pk_max_i16)
DG_DEV uint32_t relu_bf16x2(f32x2 v) {
  const s16x2 h = __builtin_bit_cast(s16x2, __builtin_convertvector(v, bf16x2v));
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(h, s16x2{0, 0}));
}
// packed bf16 pair -> two fp32
DG_DEV f32x2 bf16x2_f32(uint32_t u) {
  return f32x2{__uint_as_float(u << 16), __uint_as_float(u & 0xFFFF0000u)};
}
// bits 0 / 1 of nib -> 0xffff / 0xffff0000 halves (v_bfe_i32 x 2 + v_perm_b32)
DG_DEV uint32_t pair_mask(uint32_t nib) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_sbfe((int)nib, 0, 1);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_sbfe((int)nib, 1, 1);
  return __builtin_amdgcn_perm(hi, lo, 0x07060100u);
}

}  // namespace dg
