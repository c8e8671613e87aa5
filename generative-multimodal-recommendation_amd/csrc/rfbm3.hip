// RFBM3's inputs of the rectified-flow step (models/rfbm3.py:107-175 of the reference) from BM3's projected item
// tables T = text_trs(text), V = image_trs(image) (I x 64 each, either may be absent):
//
//   gmr_rf_item_inputs   item rows of the N x C condition table = [V | T] (one modality: that block alone) and item
//                        rows of the N x 64 prior table = Z - mean_items(Z), Z = V + T.  The user rows of both tables
//                        are zero in the reference (BM3 has no R); they are zeroed once by the caller and never
//                        touched here.
//
// Three small kernels behind the one entry point: per-block column sums of Z (and the condition rows, since V and T
// are in registers), the sum of the block partials in one fixed order, Z - mean.  No float atomics: two runs are
// bit-identical.  16 lanes hold a 64-column row as one float4 each, so a wave moves four rows per access.
#include "gmr_common.h"

namespace {

constexpr int D = 64;
constexpr int RB = 128;  // rows per block: 16 row groups of 16 lanes, 8 rows each

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// parts[block][64] = column sums of Z over the block's rows (row group rg adds its rows i = 0..7 in order, the 16
// groups are added in order); cond item rows written on the way
__global__ __launch_bounds__(256) void rf_inputs_sum_kernel(int64_t I, const float* __restrict__ T, int64_t ldt,
                                                            const float* __restrict__ V, int64_t ldv,
                                                            float* __restrict__ cond, int64_t ldc,
                                                            float* __restrict__ parts) {
  __shared__ float4 red[16][16];
  const int rg = threadIdx.x >> 4, c = (threadIdx.x & 15) * 4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int i = 0; i < RB / 16; ++i) {
    const int64_t row = (int64_t)blockIdx.x * RB + i * 16 + rg;
    if (row < I) {
      float4 z;
      if (V && T) {
        const float4 v = ld4(V + row * ldv + c), t = ld4(T + row * ldt + c);
        st4(cond + row * ldc + c, v);
        st4(cond + row * ldc + D + c, t);
        z = gmr::f4_add(v, t);
      } else {
        z = V ? ld4(V + row * ldv + c) : ld4(T + row * ldt + c);
        st4(cond + row * ldc + c, z);
      }
      acc = gmr::f4_add(acc, z);
    }
  }
  red[rg][threadIdx.x & 15] = acc;
  __syncthreads();
  if (threadIdx.x < 16) {
    float4 s = red[0][threadIdx.x];
#pragma unroll
    for (int g = 1; g < 16; ++g) s = gmr::f4_add(s, red[g][threadIdx.x]);
    st4(parts + (int64_t)blockIdx.x * D + c, s);
  }
}

// mean[c] = (sum of the block partials of column c) / I: thread (part, c) adds the blocks part, part + 4, ... in
// order, the four parts are added in order
__global__ __launch_bounds__(256) void rf_inputs_mean_kernel(int nblk, int64_t I, const float* __restrict__ parts,
                                                             float* __restrict__ mean) {
  __shared__ float red[4][D];
  const int c = threadIdx.x & 63, part = threadIdx.x >> 6;
  float a = 0.f;
  for (int i = part; i < nblk; i += 4) a += parts[(int64_t)i * D + c];
  red[part][c] = a;
  __syncthreads();
  if (part == 0) mean[c] = (((red[0][c] + red[1][c]) + red[2][c]) + red[3][c]) / (float)I;
}

__global__ __launch_bounds__(256) void rf_inputs_prior_kernel(int64_t I, const float* __restrict__ T, int64_t ldt,
                                                              const float* __restrict__ V, int64_t ldv,
                                                              const float* __restrict__ mean,
                                                              float* __restrict__ prior, int64_t ldp) {
  const int rg = threadIdx.x >> 4, c = (threadIdx.x & 15) * 4;
  const float4 m = ld4(mean + c);
#pragma unroll
  for (int i = 0; i < RB / 16; ++i) {
    const int64_t row = (int64_t)blockIdx.x * RB + i * 16 + rg;
    if (row < I) {
      float4 z;
      if (V && T) z = gmr::f4_add(ld4(V + row * ldv + c), ld4(T + row * ldt + c));
      else z = V ? ld4(V + row * ldv + c) : ld4(T + row * ldt + c);
      st4(prior + row * ldp + c, make_float4(z.x - m.x, z.y - m.y, z.z - m.z, z.w - m.w));
    }
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// ==================================================================================================== C ABI
extern "C" int64_t gmr_rf_item_inputs_ws_floats(int64_t I) { return ((I + RB - 1) / RB + 1) * D; }

extern "C" int gmr_rf_item_inputs(int64_t I, int64_t U, const float* T, int64_t ldt, const float* V, int64_t ldv,
                                  float* cond, int64_t ldc, float* prior, int64_t ldp, float* ws, void* stream) {
  GMR_ARG(I >= 1 && I <= ((int64_t)1 << 31) - RB && U >= 0, "I >= 1 and U >= 0");
  GMR_ARG(T || V, "at least one of the projected tables T, V");
  const int64_t C = T && V ? 2 * D : D;
  GMR_ARG(cond && prior && ws && ldc >= C && ldp >= D && (!T || ldt >= D) && (!V || ldv >= D),
          "bad pointers or strides");
  GMR_ARG(aligned16(T) && aligned16(V) && aligned16(cond) && aligned16(prior) && aligned16(ws) && ldt % 4 == 0 &&
              ldv % 4 == 0 && ldc % 4 == 0 && ldp % 4 == 0,
          "rows must be 16-byte aligned");
  const int nblk = gmr::grid_for(I, RB);
  float* mean = ws + (int64_t)nblk * D;
  float* ci = cond + U * ldc;  // the item rows
  float* pi = prior + U * ldp;
  hipLaunchKernelGGL(rf_inputs_sum_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, I, T, ldt, V, ldv, ci, ldc, ws);
  GMR_LAUNCHED();
  hipLaunchKernelGGL(rf_inputs_mean_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, nblk, I, ws, mean);
  GMR_LAUNCHED();
  hipLaunchKernelGGL(rf_inputs_prior_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, I, T, ldt, V, ldv, mean, pi,
                     ldp);
  GMR_LAUNCHED();
  return GMR_OK;
}
