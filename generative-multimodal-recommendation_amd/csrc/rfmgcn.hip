// RFMGCN's prior of the rectified-flow step (models/rfmgcn.py:156-172 of the reference) from MGCN's two modal views
// a = [R Hv; Hv], b = [R Ht; Ht] (N x 64 each, N = U + I; in the model both are column blocks of the one table ab):
//
//   gmr_rf_view_prior   prior[r] = Z[r] - mean_seg(r)(Z), Z = 0.5 (a + b); the mean is over the U user rows for r < U and
//                       over the I item rows otherwise.  MGCN carries both views to the users over R, so unlike RFBM3's
//                       prior (csrc/rfbm3.hip) the user half is not zero and has a mean of its own.
//
// Three small kernels behind the one entry point, as in csrc/rfbm3.hip: per-block column sums of Z, the sum of a
// segment's block partials in one fixed order (one workgroup per segment), Z - mean.  The grid is ceil(U / 128) user
// blocks followed by ceil(I / 128) item blocks, so no block holds rows of both segments and the item segment starts at
// row U whatever U mod 128 is.  No float atomics: two runs are bit-identical.  16 lanes hold a 64-column row as one
// float4 each, so a wave moves four rows per access.
#include "gmr_common.h"

namespace {

constexpr int D = 64;
constexpr int RB = 128;  // rows per block: 16 row groups of 16 lanes, 8 rows each

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// rows [lo, hi) of the block: user block k < nbu covers [128 k, min(U, 128 k + 128)), item block k - nbu covers
// [U + 128 (k - nbu), min(N, ...))
__device__ __forceinline__ void block_rows(int nbu, int64_t U, int64_t N, int64_t& lo, int64_t& hi) {
  const int k = blockIdx.x;
  const bool user = k < nbu;
  lo = user ? (int64_t)k * RB : U + (int64_t)(k - nbu) * RB;
  const int64_t end = user ? U : N;
  hi = lo + RB < end ? lo + RB : end;
}

__device__ __forceinline__ float4 view_z(const float* __restrict__ a, int64_t lda, const float* __restrict__ b,
                                         int64_t ldb, int64_t row, int c) {
  return gmr::f4_scale(0.5f, gmr::f4_add(ld4(a + row * lda + c), ld4(b + row * ldb + c)));
}

// parts[block][64] = column sums of Z over the block's rows (row group rg adds its rows i = 0..7 in order, the 16
// groups are added in order)
__global__ __launch_bounds__(256) void rf_view_sum_kernel(int nbu, int64_t U, int64_t N, const float* __restrict__ a,
                                                          int64_t lda, const float* __restrict__ b, int64_t ldb,
                                                          float* __restrict__ parts) {
  __shared__ float4 red[16][16];
  const int rg = threadIdx.x >> 4, c = (threadIdx.x & 15) * 4;
  int64_t lo, hi;
  block_rows(nbu, U, N, lo, hi);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int i = 0; i < RB / 16; ++i) {
    const int64_t row = lo + i * 16 + rg;
    if (row < hi) acc = gmr::f4_add(acc, view_z(a, lda, b, ldb, row, c));
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

// mean[seg][c] = (sum of the segment's block partials of column c) / rows(seg), one workgroup per segment: thread
// (part, c) adds the segment's blocks part, part + 16, ... in order, the sixteen parts are added in order (sixteen
// chains of dependent loads instead of four: at 152 user blocks the four-chain form took longer than either row pass)
constexpr int MP = 16;
__global__ __launch_bounds__(MP * D) void rf_view_mean_kernel(int nbu, int nbi, int64_t U, int64_t I,
                                                              const float* __restrict__ parts,
                                                              float* __restrict__ mean) {
  __shared__ float red[MP][D];
  const int seg = blockIdx.x, c = threadIdx.x & 63, part = threadIdx.x >> 6;
  const int nblk = seg ? nbi : nbu;
  const float* p = parts + (int64_t)(seg ? nbu : 0) * D;
  float s = 0.f;
  for (int i = part; i < nblk; i += MP) s += p[(int64_t)i * D + c];
  red[part][c] = s;
  __syncthreads();
  if (part == 0) {
    float t = red[0][c];
#pragma unroll
    for (int k = 1; k < MP; ++k) t += red[k][c];
    mean[seg * D + c] = t / (float)(seg ? I : U);
  }
}

__global__ __launch_bounds__(256) void rf_view_prior_kernel(int nbu, int64_t U, int64_t N, const float* __restrict__ a,
                                                            int64_t lda, const float* __restrict__ b, int64_t ldb,
                                                            const float* __restrict__ mean, float* __restrict__ prior,
                                                            int64_t ldp) {
  const int rg = threadIdx.x >> 4, c = (threadIdx.x & 15) * 4;
  int64_t lo, hi;
  block_rows(nbu, U, N, lo, hi);
  const float4 m = ld4(mean + ((int)blockIdx.x < nbu ? 0 : D) + c);
#pragma unroll
  for (int i = 0; i < RB / 16; ++i) {
    const int64_t row = lo + i * 16 + rg;
    if (row < hi) {
      const float4 z = view_z(a, lda, b, ldb, row, c);
      st4(prior + row * ldp + c, make_float4(z.x - m.x, z.y - m.y, z.z - m.z, z.w - m.w));
    }
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
constexpr int64_t MAX_ROWS = ((int64_t)1 << 31) - RB;

}  // namespace

// ==================================================================================================== C ABI
extern "C" int64_t gmr_rf_view_prior_ws_floats(int64_t U, int64_t I) {
  if (U < 1 || I < 1 || U > MAX_ROWS || I > MAX_ROWS) return -1;
  return ((U + RB - 1) / RB + (I + RB - 1) / RB + 2) * D;
}

extern "C" int gmr_rf_view_prior(int64_t U, int64_t I, const float* a, int64_t lda, const float* b, int64_t ldb,
                                 float* prior, int64_t ldp, float* ws, void* stream) {
  GMR_ARG(U >= 1 && I >= 1 && U <= MAX_ROWS && I <= MAX_ROWS, "1 <= U, I <= 2^31 - 128 (a mean over no rows is NaN)");
  GMR_ARG(a && b && prior && ws && lda >= D && ldb >= D && ldp >= D, "bad pointers or strides");
  GMR_ARG(aligned16(a) && aligned16(b) && aligned16(prior) && aligned16(ws) && lda % 4 == 0 && ldb % 4 == 0 &&
              ldp % 4 == 0,
          "rows must be 16-byte aligned");
  const int nbu = gmr::grid_for(U, RB), nbi = gmr::grid_for(I, RB);
  float* mean = ws + (int64_t)(nbu + nbi) * D;  // [users | items]
  hipLaunchKernelGGL(rf_view_sum_kernel, dim3(nbu + nbi), dim3(256), 0, (hipStream_t)stream, nbu, U, U + I, a, lda, b,
                     ldb, ws);
  GMR_LAUNCHED();
  hipLaunchKernelGGL(rf_view_mean_kernel, dim3(2), dim3(MP * D), 0, (hipStream_t)stream, nbu, nbi, U, I, ws, mean);
  GMR_LAUNCHED();
  hipLaunchKernelGGL(rf_view_prior_kernel, dim3(nbu + nbi), dim3(256), 0, (hipStream_t)stream, nbu, U, U + I, a, lda,
                     b, ldb, mean, prior, ldp);
  GMR_LAUNCHED();
  return GMR_OK;
}
