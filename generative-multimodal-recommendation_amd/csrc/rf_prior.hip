// The centred priors of the rectified-flow step, prior[r] = Z[r] - mean_seg(r)(Z), for the backbones that pass one:
//
//   gmr_rf_item_inputs   RFBM3 (models/rfbm3.py:107-175 of the reference), from BM3's projected item tables T =
//                        text_trs(text), V = image_trs(image) (I x 64 each, either may be absent): Z = V + T, the mean
//                        over the I items.  Writes the item rows of the N x 64 prior table and, on the way, the item rows
//                        of the N x C condition table = [V | T] (one modality: that block alone).  The user rows of both
//                        tables are zero in the reference (BM3 has no R); they are zeroed once by the caller and never
//                        touched here.
//   gmr_rf_view_prior    RFMGCN (models/rfmgcn.py:156-172), from MGCN's two modal views a = [R Hv; Hv], b = [R Ht; Ht]
//                        (N x 64 each, N = U + I; in the model both are column blocks of the one table ab): Z =
//                        0.5 (a + b); the mean is over the U user rows for r < U and over the I item rows otherwise.
//                        MGCN carries both views to the users over R, so the user half has a mean of its own.
//   gmr_rf_view3_inputs  RFSMORE (models/rfsmore.py:165-195), from SMORE's three views a, b, f and the fusion
//                        preference gate g of the step (with that step's dropout mask and scale; N x 64 each, every
//                        one with a row stride of its own: column blocks of abf and of saved in the model): Z =
//                        (a + b + g f) / 3, the two segment means as for RFMGCN.  Writes the N x 64 prior and, on the
//                        way, the N x 192 condition table [a | b | g f].
//   gmr_rf_view_sum_prior  RFLGMRec (models/rflgmrec.py:125-143), from LGMRec's two propagated modal views mge_v, mge_t
//                        (the column blocks of the one N x 128 table mge): Z = a + b, a sum and no mean of the views;
//                        the segments, the grid and the fixed-order means as gmr_rf_view_prior.
//   gmr_rf_center_segments  RFGRCN (models/rfgrcn.py:171-190), from GRCN's concatenated table [id_rep | rep_v | rep_t]
//                        (N x W, W = 64, 128 or 192): every 64-wide block centred per segment, which is the whole
//                        W-wide row minus its segment's column means.  The same three kernels at row width W (a lane
//                        holds W / 64 float4 of a row), so the table is read once per pass, not once per block.
//
// Three small kernels behind every entry point, each a template over the functor that forms Z for a row: per-block
// column sums of Z, the sum of a segment's block partials in one fixed order (one workgroup per segment), Z - mean.
// The grid is ceil(U / 128) blocks of the first segment followed by ceil(I / 128) of the second, so no block holds
// rows of both and the second segment starts at row U whatever U mod 128 is; gmr_rf_item_inputs has the first segment
// alone, on tables that start at the item rows.  No float atomics: two runs are bit-identical.  16 lanes hold a
// 64-column row as one float4 each, so a wave moves four rows per access.
#include "gmr_common.h"

namespace {

using gmr::ld4, gmr::st4, gmr::aligned16;

constexpr int D = 64;
constexpr int RB = 128;  // rows per block: 16 row groups of 16 lanes, 8 rows each
constexpr int64_t MAX_ROWS = ((int64_t)1 << 31) - RB;

// Z = V + T, or the one table present; STORE: the row of the condition table written on the way, since V and T are in
// registers
template <bool STORE>
struct ItemZ {
  const float* __restrict__ T;
  int64_t ldt;
  const float* __restrict__ V;
  int64_t ldv;
  float* __restrict__ cond;
  int64_t ldc;
  __device__ __forceinline__ float4 operator()(int64_t row, int c) const {
    float4 z;
    if (V && T) {
      const float4 v = ld4(V + row * ldv + c), t = ld4(T + row * ldt + c);
      if (STORE) {
        st4(cond + row * ldc + c, v);
        st4(cond + row * ldc + D + c, t);
      }
      z = gmr::f4_add(v, t);
    } else {
      z = V ? ld4(V + row * ldv + c) : ld4(T + row * ldt + c);
      if (STORE) st4(cond + row * ldc + c, z);
    }
    return z;
  }
};

struct ViewZ {
  const float* __restrict__ a;
  int64_t lda;
  const float* __restrict__ b;
  int64_t ldb;
  __device__ __forceinline__ float4 operator()(int64_t row, int c) const {
    return gmr::f4_scale(0.5f, gmr::f4_add(ld4(a + row * lda + c), ld4(b + row * ldb + c)));
  }
};

struct ViewSumZ {
  const float* __restrict__ a;
  int64_t lda;
  const float* __restrict__ b;
  int64_t ldb;
  __device__ __forceinline__ float4 operator()(int64_t row, int c) const {
    return gmr::f4_add(ld4(a + row * lda + c), ld4(b + row * ldb + c));
  }
};

// Z = (a + b + g f) / 3; STORE: the condition row [a | b | g f] written on the way.  g f is one rounded product in
// both passes (no contraction with the sum), so the condition's third block and the prior see the same number.
template <bool STORE>
struct View3Z {
  const float* __restrict__ a;
  int64_t lda;
  const float* __restrict__ b;
  int64_t ldb;
  const float* __restrict__ f;
  int64_t ldf;
  const float* __restrict__ g;
  int64_t ldg;
  float* __restrict__ cond;
  int64_t ldc;
  __device__ __forceinline__ float4 operator()(int64_t row, int c) const {
#pragma clang fp contract(off)
    const float4 av = ld4(a + row * lda + c), bv = ld4(b + row * ldb + c);
    const float4 fv = ld4(f + row * ldf + c), gv = ld4(g + row * ldg + c);
    const float4 gf = make_float4(gv.x * fv.x, gv.y * fv.y, gv.z * fv.z, gv.w * fv.w);
    if (STORE) {
      st4(cond + row * ldc + c, av);
      st4(cond + row * ldc + D + c, bv);
      st4(cond + row * ldc + 2 * D + c, gf);
    }
    const float4 s = gmr::f4_add(gmr::f4_add(av, bv), gf);
    return make_float4(s.x / 3.f, s.y / 3.f, s.z / 3.f, s.w / 3.f);
  }
};

// rows [lo, hi) of the block and its segment: block k < nbu of the first covers [128 k, min(U, 128 k + 128)), block
// k - nbu of the second covers [U + 128 (k - nbu), min(N, ...))
__device__ __forceinline__ int block_rows(int nbu, int64_t U, int64_t N, int64_t& lo, int64_t& hi) {
  const int k = blockIdx.x;
  const bool first = k < nbu;
  lo = first ? (int64_t)k * RB : U + (int64_t)(k - nbu) * RB;
  const int64_t end = first ? U : N;
  hi = lo + RB < end ? lo + RB : end;
  return first ? 0 : 1;
}

// parts[block][64] = column sums of Z over the block's rows (row group rg adds its rows i = 0..7 in order, the 16
// groups are added in order)
template <class Z>
__global__ __launch_bounds__(256) void rf_prior_sum_kernel(int nbu, int64_t U, int64_t N, Z z,
                                                           float* __restrict__ parts) {
  __shared__ float4 red[16][16];
  const int rg = threadIdx.x >> 4, c = (threadIdx.x & 15) * 4;
  int64_t lo, hi;
  block_rows(nbu, U, N, lo, hi);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int i = 0; i < RB / 16; ++i) {
    const int64_t row = lo + i * 16 + rg;
    if (row < hi) acc = gmr::f4_add(acc, z(row, c));
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
// (part, c) adds the segment's blocks part, part + MP, ... in order, the MP parts are added in order.  MP is the
// entry point's own and part of its result: 4 for gmr_rf_item_inputs, 16 for gmr_rf_view_prior (sixteen chains of
// dependent loads instead of four: at 152 user blocks the four-chain form took longer than either row pass)
template <int MP>
__global__ __launch_bounds__(MP * D) void rf_prior_mean_kernel(int nbu, int nbi, int64_t U, int64_t I,
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

template <class Z>
__global__ __launch_bounds__(256) void rf_prior_sub_kernel(int nbu, int64_t U, int64_t N, Z z,
                                                           const float* __restrict__ mean, float* __restrict__ prior,
                                                           int64_t ldp) {
  const int rg = threadIdx.x >> 4, c = (threadIdx.x & 15) * 4;
  int64_t lo, hi;
  const float4 m = ld4(mean + block_rows(nbu, U, N, lo, hi) * D + c);
#pragma unroll
  for (int i = 0; i < RB / 16; ++i) {
    const int64_t row = lo + i * 16 + rg;
    if (row < hi) {
      const float4 v = z(row, c);
      st4(prior + row * ldp + c, make_float4(v.x - m.x, v.y - m.y, v.z - m.z, v.w - m.w));
    }
  }
}

// ------------------------------------------------------------------------------------------------ W-wide rows
// The three kernels above at row width W = 64 NJ for a plain table: 16 lanes hold a row as NJ float4 each (columns
// 4 (lane & 15) + 64 j), the grid and the block's row order are the same, parts and mean rows are W wide.
template <int NJ>
__global__ __launch_bounds__(256) void rf_center_sum_kernel(int nbu, int64_t U, int64_t N,
                                                            const float* __restrict__ src, int64_t lds,
                                                            float* __restrict__ parts) {
  __shared__ float4 red[16][NJ][16];
  const int rg = threadIdx.x >> 4, l = threadIdx.x & 15, c = l * 4;
  int64_t lo, hi;
  block_rows(nbu, U, N, lo, hi);
  float4 acc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int i = 0; i < RB / 16; ++i) {
    const int64_t row = lo + i * 16 + rg;
    if (row < hi) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[j] = gmr::f4_add(acc[j], ld4(src + row * lds + c + D * j));
    }
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) red[rg][j][l] = acc[j];
  __syncthreads();
  if (threadIdx.x < 16 * NJ) {  // thread (j, l) adds the 16 row groups in order
    const int j = threadIdx.x >> 4;
    float4 s = red[0][j][l];
#pragma unroll
    for (int g = 1; g < 16; ++g) s = gmr::f4_add(s, red[g][j][l]);
    st4(parts + (int64_t)blockIdx.x * (D * NJ) + D * j + c, s);
  }
}

// mean[seg][c] over W = 64 NJ columns by one workgroup of 1024 threads per segment: thread (part, c), part < MP =
// 1024 / W, adds the segment's blocks part, part + MP, ... in order, the MP parts are added in order
template <int NJ>
__global__ __launch_bounds__(1024) void rf_center_mean_kernel(int nbu, int nbi, int64_t U, int64_t I,
                                                              const float* __restrict__ parts,
                                                              float* __restrict__ mean) {
  constexpr int W = D * NJ, MP = 1024 / W;
  __shared__ float red[MP][W];
  const int seg = blockIdx.x, c = threadIdx.x % W, part = threadIdx.x / W;
  const int nblk = seg ? nbi : nbu;
  const float* p = parts + (int64_t)(seg ? nbu : 0) * W;
  if (part < MP) {
    float s = 0.f;
    for (int i = part; i < nblk; i += MP) s += p[(int64_t)i * W + c];
    red[part][c] = s;
  }
  __syncthreads();
  if (part == 0) {
    float t = red[0][c];
#pragma unroll
    for (int k = 1; k < MP; ++k) t += red[k][c];
    mean[seg * W + c] = t / (float)(seg ? I : U);
  }
}

template <int NJ>
__global__ __launch_bounds__(256) void rf_center_sub_kernel(int nbu, int64_t U, int64_t N,
                                                            const float* __restrict__ src, int64_t lds,
                                                            const float* __restrict__ mean, float* __restrict__ prior,
                                                            int64_t ldp) {
  const int rg = threadIdx.x >> 4, c = (threadIdx.x & 15) * 4;
  int64_t lo, hi;
  const int seg = block_rows(nbu, U, N, lo, hi);
  float4 m[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) m[j] = ld4(mean + seg * (D * NJ) + D * j + c);
#pragma unroll
  for (int i = 0; i < RB / 16; ++i) {
    const int64_t row = lo + i * 16 + rg;
    if (row < hi) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const float4 v = ld4(src + row * lds + c + D * j);
        st4(prior + row * ldp + c + D * j, make_float4(v.x - m[j].x, v.y - m[j].y, v.z - m[j].z, v.w - m[j].w));
      }
    }
  }
}

template <int NJ>
hipError_t center_launch(int nbu, int nbi, int64_t U, int64_t I, const float* src, int64_t lds, float* prior,
                         int64_t ldp, float* ws, hipStream_t st) {
  float* mean = ws + (int64_t)(nbu + nbi) * (D * NJ);  // [users | items]
  hipLaunchKernelGGL(rf_center_sum_kernel<NJ>, dim3(nbu + nbi), dim3(256), 0, st, nbu, U, U + I, src, lds, ws);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(rf_center_mean_kernel<NJ>, dim3(2), dim3(1024), 0, st, nbu, nbi, U, I, ws, mean);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(rf_center_sub_kernel<NJ>, dim3(nbu + nbi), dim3(256), 0, st, nbu, U, U + I, src, lds, mean, prior,
                     ldp);
  return hipGetLastError();
}

}  // namespace

// ==================================================================================================== C ABI
extern "C" int64_t gmr_rf_item_inputs_ws_floats(int64_t I) { return ((I + RB - 1) / RB + 1) * D; }

extern "C" int gmr_rf_item_inputs(int64_t I, int64_t U, const float* T, int64_t ldt, const float* V, int64_t ldv,
                                  float* cond, int64_t ldc, float* prior, int64_t ldp, float* ws, void* stream) {
  GMR_ARG(I >= 1 && I <= MAX_ROWS && U >= 0, "I >= 1 and U >= 0");
  GMR_ARG(T || V, "at least one of the projected tables T, V");
  const int64_t C = T && V ? 2 * D : D;
  GMR_ARG(cond && prior && ws && ldc >= C && ldp >= D && (!T || ldt >= D) && (!V || ldv >= D),
          "bad pointers or strides");
  GMR_ARG(aligned16(T) && aligned16(V) && aligned16(cond) && aligned16(prior) && aligned16(ws) && ldt % 4 == 0 &&
              ldv % 4 == 0 && ldc % 4 == 0 && ldp % 4 == 0,
          "rows must be 16-byte aligned");
  const int nblk = gmr::grid_for(I, RB);
  float* mean = ws + (int64_t)nblk * D;
  float* ci = cond + U * ldc;  // the item rows: the I rows are the first segment, the second is empty
  float* pi = prior + U * ldp;
  hipLaunchKernelGGL(rf_prior_sum_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, nblk, I, I,
                     ItemZ<true>{T, ldt, V, ldv, ci, ldc}, ws);
  GMR_LAUNCHED();
  hipLaunchKernelGGL(rf_prior_mean_kernel<4>, dim3(1), dim3(4 * D), 0, (hipStream_t)stream, nblk, 0, I, (int64_t)0, ws,
                     mean);
  GMR_LAUNCHED();
  hipLaunchKernelGGL(rf_prior_sub_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, nblk, I, I,
                     ItemZ<false>{T, ldt, V, ldv, nullptr, 0}, mean, pi, ldp);
  GMR_LAUNCHED();
  return GMR_OK;
}

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
  const ViewZ z{a, lda, b, ldb};
  hipLaunchKernelGGL(rf_prior_sum_kernel, dim3(nbu + nbi), dim3(256), 0, (hipStream_t)stream, nbu, U, U + I, z, ws);
  GMR_LAUNCHED();
  hipLaunchKernelGGL(rf_prior_mean_kernel<16>, dim3(2), dim3(16 * D), 0, (hipStream_t)stream, nbu, nbi, U, I, ws, mean);
  GMR_LAUNCHED();
  hipLaunchKernelGGL(rf_prior_sub_kernel, dim3(nbu + nbi), dim3(256), 0, (hipStream_t)stream, nbu, U, U + I, z, mean,
                     prior, ldp);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int64_t gmr_rf_view_sum_prior_ws_floats(int64_t U, int64_t I) { return gmr_rf_view_prior_ws_floats(U, I); }

extern "C" int gmr_rf_view_sum_prior(int64_t U, int64_t I, const float* a, int64_t lda, const float* b, int64_t ldb,
                                     float* prior, int64_t ldp, float* ws, void* stream) {
  GMR_ARG(U >= 1 && I >= 1 && U <= MAX_ROWS && I <= MAX_ROWS, "1 <= U, I <= 2^31 - 128 (a mean over no rows is NaN)");
  GMR_ARG(a && b && prior && ws && lda >= D && ldb >= D && ldp >= D, "bad pointers or strides");
  GMR_ARG(aligned16(a) && aligned16(b) && aligned16(prior) && aligned16(ws) && lda % 4 == 0 && ldb % 4 == 0 &&
              ldp % 4 == 0,
          "rows must be 16-byte aligned");
  const int nbu = gmr::grid_for(U, RB), nbi = gmr::grid_for(I, RB);
  float* mean = ws + (int64_t)(nbu + nbi) * D;  // [users | items]
  const ViewSumZ z{a, lda, b, ldb};
  hipLaunchKernelGGL(rf_prior_sum_kernel, dim3(nbu + nbi), dim3(256), 0, (hipStream_t)stream, nbu, U, U + I, z, ws);
  GMR_LAUNCHED();
  hipLaunchKernelGGL(rf_prior_mean_kernel<16>, dim3(2), dim3(16 * D), 0, (hipStream_t)stream, nbu, nbi, U, I, ws, mean);
  GMR_LAUNCHED();
  hipLaunchKernelGGL(rf_prior_sub_kernel, dim3(nbu + nbi), dim3(256), 0, (hipStream_t)stream, nbu, U, U + I, z, mean,
                     prior, ldp);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int64_t gmr_rf_view3_inputs_ws_floats(int64_t U, int64_t I) { return gmr_rf_view_prior_ws_floats(U, I); }

extern "C" int gmr_rf_view3_inputs(int64_t U, int64_t I, const float* a, int64_t lda, const float* b, int64_t ldb,
                                   const float* f, int64_t ldf, const float* g, int64_t ldg, float* cond, int64_t ldc,
                                   float* prior, int64_t ldp, float* ws, void* stream) {
  GMR_ARG(U >= 1 && I >= 1 && U <= MAX_ROWS && I <= MAX_ROWS, "1 <= U, I <= 2^31 - 128 (a mean over no rows is NaN)");
  GMR_ARG(a && b && f && g && cond && prior && ws && lda >= D && ldb >= D && ldf >= D && ldg >= D && ldc >= 3 * D &&
              ldp >= D,
          "bad pointers or strides");
  GMR_ARG(aligned16(a) && aligned16(b) && aligned16(f) && aligned16(g) && aligned16(cond) && aligned16(prior) &&
              aligned16(ws) && lda % 4 == 0 && ldb % 4 == 0 && ldf % 4 == 0 && ldg % 4 == 0 && ldc % 4 == 0 &&
              ldp % 4 == 0,
          "rows must be 16-byte aligned");
  const int nbu = gmr::grid_for(U, RB), nbi = gmr::grid_for(I, RB);
  float* mean = ws + (int64_t)(nbu + nbi) * D;  // [users | items]
  hipLaunchKernelGGL(rf_prior_sum_kernel, dim3(nbu + nbi), dim3(256), 0, (hipStream_t)stream, nbu, U, U + I,
                     View3Z<true>{a, lda, b, ldb, f, ldf, g, ldg, cond, ldc}, ws);
  GMR_LAUNCHED();
  hipLaunchKernelGGL(rf_prior_mean_kernel<16>, dim3(2), dim3(16 * D), 0, (hipStream_t)stream, nbu, nbi, U, I, ws, mean);
  GMR_LAUNCHED();
  hipLaunchKernelGGL(rf_prior_sub_kernel, dim3(nbu + nbi), dim3(256), 0, (hipStream_t)stream, nbu, U, U + I,
                     View3Z<false>{a, lda, b, ldb, f, ldf, g, ldg, nullptr, 0}, mean, prior, ldp);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int64_t gmr_rf_center_segments_ws_floats(int64_t U, int64_t I, int32_t W) {
  if (U < 1 || I < 1 || U > MAX_ROWS || I > MAX_ROWS || (W != D && W != 2 * D && W != 3 * D)) return -1;
  return ((U + RB - 1) / RB + (I + RB - 1) / RB + 2) * W;
}

extern "C" int gmr_rf_center_segments(int64_t U, int64_t I, int32_t W, const float* src, int64_t lds, float* prior,
                                      int64_t ldp, float* ws, void* stream) {
  GMR_ARG(U >= 1 && I >= 1 && U <= MAX_ROWS && I <= MAX_ROWS, "1 <= U, I <= 2^31 - 128 (a mean over no rows is NaN)");
  GMR_ARG(W == D || W == 2 * D || W == 3 * D, "the row width W must be 64, 128 or 192");
  GMR_ARG(src && prior && ws && lds >= W && ldp >= W, "bad pointers or strides");
  GMR_ARG(aligned16(src) && aligned16(prior) && aligned16(ws) && lds % 4 == 0 && ldp % 4 == 0,
          "rows must be 16-byte aligned");
  const int nbu = gmr::grid_for(U, RB), nbi = gmr::grid_for(I, RB);
  const hipStream_t st = (hipStream_t)stream;
  const hipError_t e = W == D       ? center_launch<1>(nbu, nbi, U, I, src, lds, prior, ldp, ws, st)
                       : W == 2 * D ? center_launch<2>(nbu, nbi, U, I, src, lds, prior, ldp, ws, st)
                                    : center_launch<3>(nbu, nbi, U, I, src, lds, prior, ldp, ws, st);
  if (e != hipSuccess) return gmr::hip_status(__func__, e);
  return GMR_OK;
}
