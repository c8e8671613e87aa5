// The 16-row tile scheme of the row-local fused kernels (csrc/mgcn.hip, csrc/smore.hip): 64-column rows, a workgroup
// of four waves, weights and row tiles in LDS with row stride 68.  In the element phases thread tid owns row tid >> 4,
// columns 4 (tid & 15) .. + 3 of the tile; in the MFMA phases (v_mfma_f32_16x16x4_f32) wave w computes the output
// columns 16 w .. 16 w + 15 of every product and hands them back through the row tiles.  One fixed MFMA k order and one
// butterfly per row sum: a row's result depends on its own inputs and the weights only.
#pragma once
#include <math.h>

#include "gemm_impl.h"

namespace gmr_row {

constexpr int D = 64, TR = 16, LDX = D + 4;

using gmr::ld4, gmr::st4, gmr::mul4;
// one fixed fma chain: two rows with the same values give the same bits wherever the compiler places the call
__device__ __forceinline__ float dot4(float4 a, float4 b) {
  return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)));
}
__device__ __forceinline__ float row16_sum(float v) {
#pragma unroll
  for (int m = 8; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }  // +-inf arguments give 1 / 0
__device__ __forceinline__ float4 sigm4(float4 x) { return make_float4(sigm(x.x), sigm(x.y), sigm(x.z), sigm(x.w)); }
__device__ __forceinline__ float4 tanh4(float4 x) { return make_float4(tanhf(x.x), tanhf(x.y), tanhf(x.z), tanhf(x.w)); }
// g (1 - g) and 1 - h^2
__device__ __forceinline__ float4 dsig4(float4 g) {
  return make_float4(g.x * (1.f - g.x), g.y * (1.f - g.y), g.z * (1.f - g.z), g.w * (1.f - g.w));
}
__device__ __forceinline__ float4 dtanh4(float4 h) {
  return make_float4(1.f - h.x * h.x, 1.f - h.y * h.y, 1.f - h.z * h.z, 1.f - h.w * h.w);
}

// acc (16 rows x columns 16 ct .. 16 ct + 15) += A[16][64] . Bt[col][0..63]^T, both in LDS with row stride LDX.
// Lane l feeds row / column l & 15 and, per float4, the k values 16 (l >> 4) + 4 s .. + 3 (the same on both sides).
// acc element e of lane l: row 4 (l >> 4) + e, column 16 ct + (l & 15).
__device__ __forceinline__ void mm16c(const float* sA, const float* sBt, int ct, floatx4& acc) {
  const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const float4 a = ld4(sA + r * LDX + 16 * q + 4 * s);
    const float4 b = ld4(sBt + (16 * ct + r) * LDX + 16 * q + 4 * s);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
  }
}
// the wave's 16 x 16 block into a row tile (+ bias[column], bias may be null)
__device__ __forceinline__ void put16c(float* sX, int ct, const floatx4& acc, const float* bias) {
  const int lane = threadIdx.x & 63, col = 16 * ct + (lane & 15), r0 = 4 * (lane >> 4);
  const float b = bias ? bias[col] : 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) sX[(r0 + e) * LDX + col] = acc[e] + b;
}
// s[j][k] = W[j][k] (x W^T: the product of the forward) or s[k][j] = W[j][k] (z W: the backward), 256 threads
__device__ __forceinline__ void stage_w(float* s, const float* __restrict__ W, int64_t ldw, bool transposed) {
  const int tid = threadIdx.x;
  if (!transposed) {
    for (int i = tid; i < D * 16; i += 256) {
      const int j = i >> 4, k = (i & 15) * 4;
      st4(s + j * LDX + k, ld4(W + j * ldw + k));
    }
  } else {
    const int k = tid & 63, jg = tid >> 6;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int j0 = 16 * it + 4 * jg;
      st4(s + k * LDX + j0,
          make_float4(W[(j0 + 0) * ldw + k], W[(j0 + 1) * ldw + k], W[(j0 + 2) * ldw + k], W[(j0 + 3) * ldw + k]));
    }
  }
}

__device__ __forceinline__ floatx4 zero4() { return floatx4{0.f, 0.f, 0.f, 0.f}; }

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool rows16(const float* p, int64_t ld, int cols = D) { return p && ld >= cols && ld % 4 == 0 && al16(p); }

}  // namespace gmr_row
