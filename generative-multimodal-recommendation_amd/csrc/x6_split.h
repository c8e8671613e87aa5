// Exact three-way bf16 split of fp32 values, two at a time, as hand-placed single-issue VALU instructions
// (gemm_x6.hip's operand staging and the split-bf16 InfoNCE passes of diffmm.hip).
//
// x = hi + mid + lo with hi = bf16(clamp(x)), mid = bf16(x - hi), lo = bf16(x - hi - mid), every conversion
// round-to-nearest-even and both subtractions exact (see gemm_x6.hip).  Written in C++ the compiler's SLP
// vectoriser pairs the subtractions of neighbouring elements into v_pk_add_f32 (and the InfoNCE passes' scale /
// weight arithmetic into v_pk_mul_f32 / v_pk_fma_f32) at plain -O3, and a packed fp32 instruction costs ~13 cycles
// more than two scalar ones when it issues beside v_mfma_f32_32x32x16_bf16.  Making the differences opaque to the
// vectoriser (an empty asm on the register) removes the packed forms but leaves an s_nop before each conversion
// that reads such a register (the hazard recogniser assumes the worst of an asm's results).  So the 13 instructions
// of a pair are spelled out, in three pieces of 4 + 4 + 5 that a pipelined loop can drop into successive MFMA gaps
// (a 32-cycle gap hides five 4-cycle fillers), or as one block where the split has a phase of its own: the same
// instructions the compiler chose around its packed subtractions (v_med3_f32, v_cvt_pk_bf16_f32, v_lshlrev_b32 /
// v_and_b32 to read a bf16 half back as fp32), the same roundings, the same bits.  None of these instructions
// needs a wait state before the next reads its result.
#pragma once
#include <hip/hip_runtime.h>

namespace gmr_x6 {

struct Pair {  // one pair in flight: packed hi and mid, hi[0] as fp32, and the two remainders
  unsigned h, m;
  float a, r0, r1;
};

// piece 0 (4 VALU): h = bf16 pair of the values clamped into bf16's range; a = h[0] as fp32
__device__ __forceinline__ void split_p0(float x0, float x1, Pair& s) {
  float t0, t1;
  asm("v_med3_f32 %2, %4, %6, %7\n\t"
      "v_med3_f32 %3, %5, %6, %7\n\t"
      "v_cvt_pk_bf16_f32 %0, %2, %3\n\t"
      "v_lshlrev_b32_e32 %1, 16, %0"
      : "=&v"(s.h), "=&v"(s.a), "=&v"(t0), "=&v"(t1)
      : "v"(x0), "v"(x1), "s"(-0x1.fep127f), "v"(0x1.fep127f));
}

// piece 1 (4 VALU): r = x - hi (exact), m = bf16 pair of r
__device__ __forceinline__ void split_p1(float x0, float x1, Pair& s) {
  float b;
  asm("v_and_b32_e32 %3, 0xffff0000, %6\n\t"
      "v_sub_f32_e32 %0, %4, %7\n\t"
      "v_sub_f32_e32 %1, %5, %3\n\t"
      "v_cvt_pk_bf16_f32 %2, %0, %1"
      : "=&v"(s.r0), "=&v"(s.r1), "=&v"(s.m), "=&v"(b)
      : "v"(x0), "v"(x1), "v"(s.h), "v"(s.a));
}

// piece 2 (5 VALU): lo = bf16 pair of r - mid (exact: at most 8 significand bits remain)
__device__ __forceinline__ unsigned split_p2(const Pair& s) {
  unsigned l;
  float a, b;
  asm("v_lshlrev_b32_e32 %1, 16, %5\n\t"
      "v_and_b32_e32 %2, 0xffff0000, %5\n\t"
      "v_sub_f32_e32 %1, %3, %1\n\t"
      "v_sub_f32_e32 %2, %4, %2\n\t"
      "v_cvt_pk_bf16_f32 %0, %1, %2"
      : "=&v"(l), "=&v"(a), "=&v"(b)
      : "v"(s.r0), "v"(s.r1), "v"(s.m));
  return l;
}

// A whole pair at once (13 VALU): packed hi, mid, lo.  One asm statement, not the three pieces in a row: between
// two asm statements the hazard recogniser puts an s_nop wherever the second reads a result of the first.
__device__ __forceinline__ void split_pair(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
  float a, b, r0, r1;
  asm("v_med3_f32 %3, %7, %9, %10\n\t"
      "v_med3_f32 %4, %8, %9, %10\n\t"
      "v_cvt_pk_bf16_f32 %0, %3, %4\n\t"
      "v_lshlrev_b32_e32 %3, 16, %0\n\t"
      "v_and_b32_e32 %4, 0xffff0000, %0\n\t"
      "v_sub_f32_e32 %5, %7, %3\n\t"
      "v_sub_f32_e32 %6, %8, %4\n\t"
      "v_cvt_pk_bf16_f32 %1, %5, %6\n\t"
      "v_lshlrev_b32_e32 %3, 16, %1\n\t"
      "v_and_b32_e32 %4, 0xffff0000, %1\n\t"
      "v_sub_f32_e32 %3, %5, %3\n\t"
      "v_sub_f32_e32 %4, %6, %4\n\t"
      "v_cvt_pk_bf16_f32 %2, %3, %4"
      : "=&v"(h), "=&v"(m), "=&v"(l), "=&v"(a), "=&v"(b), "=&v"(r0), "=&v"(r1)
      : "v"(x0), "v"(x1), "s"(-0x1.fep127f), "v"(0x1.fep127f));
}

// hi and mid only (8 VALU): the operands of the three-product Y accumulation of the InfoNCE passes
__device__ __forceinline__ void split_pair2(float x0, float x1, unsigned& h, unsigned& m) {
  float a, b;
  asm("v_med3_f32 %2, %4, %6, %7\n\t"
      "v_med3_f32 %3, %5, %6, %7\n\t"
      "v_cvt_pk_bf16_f32 %0, %2, %3\n\t"
      "v_lshlrev_b32_e32 %2, 16, %0\n\t"
      "v_and_b32_e32 %3, 0xffff0000, %0\n\t"
      "v_sub_f32_e32 %2, %4, %2\n\t"
      "v_sub_f32_e32 %3, %5, %3\n\t"
      "v_cvt_pk_bf16_f32 %1, %2, %3"
      : "=&v"(h), "=&v"(m), "=&v"(a), "=&v"(b)
      : "v"(x0), "v"(x1), "s"(-0x1.fep127f), "v"(0x1.fep127f));
}

// the same of x = w * e (x0, x1: the rounded products): mid = bf16(fma(w, e, -hi)), the
// contraction the compiler makes of (w * e) - hi where the product feeds the subtraction directly
__device__ __forceinline__ void split_pair2_fma(float x0, float x1, float w0, float e0, float w1, float e1,
                                                unsigned& h, unsigned& m) {
  float a, b;
  asm("v_med3_f32 %2, %4, %10, %11\n\t"
      "v_med3_f32 %3, %5, %10, %11\n\t"
      "v_cvt_pk_bf16_f32 %0, %2, %3\n\t"
      "v_lshlrev_b32_e32 %2, 16, %0\n\t"
      "v_and_b32_e32 %3, 0xffff0000, %0\n\t"
      "v_fma_f32 %2, %6, %7, -%2\n\t"
      "v_fma_f32 %3, %8, %9, -%3\n\t"
      "v_cvt_pk_bf16_f32 %1, %2, %3"
      : "=&v"(h), "=&v"(m), "=&v"(a), "=&v"(b)
      : "v"(x0), "v"(x1), "v"(w0), "v"(e0), "v"(w1), "v"(e1), "s"(-0x1.fep127f), "v"(0x1.fep127f));
}

}  // namespace gmr_x6
