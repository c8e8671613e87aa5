// LATTICE (models/lattice.py of the reference): the learned kNN item graph and its backward on slot lists.
//
// Per modality m (M <= 2) the projected features are row-normalised (n_m, I x 64) and idx_m (I x k) holds each row's
// top-k of n_m n_m^T.  Edge e = (i, m, slot) sits at position q = m k + slot of row i; everything per edge is an
// I x (M k) array.  A column may occur in several slots of a row: every sum below is linear in the slots, so the
// duplicates add and no union is formed.
//   v_e   = <n_i, n_j>                        j = idx_m[i, slot]
//   a_e   = w_m v_e                           w = softmax(modal_weight) (M = 1: w = 1)
//   r_i   = sum_q a_(i,q);  s_i = r_i^-1/2 (0 where r_i = 0)
//   L_e   = s_i a_e s_j
//   item_adj row i (R = 2 M k slots) = [(1 - lambda) L_(i,.) | lambda w_m O_m[i,.]]   O_m the frozen original lists
// Backward from dA (I x R, the sampled product sum_l <g_l[i], h_(l-1)[col]>):
//   p_e   = (1 - lambda) dA_e a_e             (dL_e a_e)
//   ds_i  = sum_q p_(i,q) s_col + sum_{e -> i} p_e s_row(e);   dr_i = -1/2 ds_i s_i^3 (0 where r_i = 0)
//   da_e  = (1 - lambda) dA_e s_i s_j + dr_i; dv_e = w_m da_e; dw_m = sum_e da_e v_e + lambda sum O_m dA_orig
//   dn_m[i] = sum_slot dv_(i,m,slot) n_j + sum_{e -> i} dv_e n_row(e)
// The incoming lists (e -> i) come from the caller: in_ptr (M I + 1) and in_edge, the edge ids (i M k + q) sorted
// stably by the key m I + col.
//
//   gmr_lat_edge_fwd    v, the learned columns, r, s         a quarter-wave per row, one 256-byte row per float4 x 16
//   gmr_lat_adj_fwd     the I x R values                     a thread per slot
//   gmr_lat_sddmm       dA (+)= <g[i], h[col]>               a quarter-wave per row
//   gmr_lat_bwd_ds      dr                                   a wave per item, a lane per edge
//   gmr_lat_bwd_da      dv and the per-row parts of dw       a wave per row, a lane per slot
//   gmr_lat_dw_reduce   the 2-element softmax backward       one workgroup, fp64 tree
//   gmr_lat_bwd_dn      dn_m                                 a wave per (item, modality), a quarter-wave per edge
//
// No float atomics: every sum is a per-lane chain in list order followed by one xor butterfly, so two runs give the
// same bits.  A list longer than a wave's trip (a hub that every row lists) is a longer loop of the same wave.
#include <math.h>

#include "gmr_common.h"

namespace {

constexpr int D = 64;

using gmr::ld4, gmr::st4;
// one fixed fma chain
__device__ __forceinline__ float dot4(float4 a, float4 b) {
  return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)));
}
__device__ __forceinline__ float row16_sum(float v) {
#pragma unroll
  for (int m = 8; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
// softmax over the two modal weights; equal entries give (0.5, 0.5) exactly
__device__ __forceinline__ void modal_w(const float* __restrict__ mw, int M, float& w0, float& w1) {
  if (M == 2) {
    const float a = mw[0], b = mw[1];
    w0 = 1.f / (1.f + expf(b - a));
    w1 = 1.f / (1.f + expf(a - b));
  } else {
    w0 = 1.f;
    w1 = 0.f;
  }
}

struct EdgeArgs {
  int64_t n;
  int k, M;
  const float* nv[2];
  int64_t ldn[2];
  const int* idx[2];
  int64_t ldi[2];
  const float* mw;
  float* v;   // n x (M k)
  int* col;   // n x ldc, the first M k columns written
  int64_t ldc;
  float *r, *s;
};

__global__ __launch_bounds__(256) void lat_edge_fwd_kernel(EdgeArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (i >= a.n) return;  // the 16 lanes of a row leave together
  const int l = threadIdx.x & 15, c = l * 4;
  float w[2];
  modal_w(a.mw, a.M, w[0], w[1]);
  const int Mk = a.M * a.k;
  float rs = 0.f;
  for (int m = 0; m < a.M; ++m) {
    const float* nv = a.nv[m];
    const int64_t ld = a.ldn[m];
    const float4 ni = ld4(nv + i * ld + c);
    const int* row = a.idx[m] + i * a.ldi[m];
    for (int sl = 0; sl < a.k; ++sl) {
      const int j = row[sl];
      const float d = row16_sum(dot4(ni, ld4(nv + (int64_t)j * ld + c)));
      rs += w[m] * d;
      if (l == 0) {
        a.v[i * Mk + m * a.k + sl] = d;
        a.col[i * a.ldc + m * a.k + sl] = j;
      }
    }
  }
  if (l == 0) {
    a.r[i] = rs;
    a.s[i] = rs == 0.f ? 0.f : 1.f / sqrtf(rs);
  }
}

__global__ __launch_bounds__(256) void lat_adj_fwd_kernel(int64_t n, int k, int M, const float* __restrict__ v,
                                                          const float* __restrict__ s, const int* __restrict__ col,
                                                          int64_t ldc, const float* __restrict__ oval,
                                                          const float* __restrict__ mw, float lambda,
                                                          float* __restrict__ val) {
  const int Mk = M * k, R = 2 * Mk;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= n * R) return;
  const int64_t i = gid / R;
  const int q = (int)(gid - i * R);
  float w[2];
  modal_w(mw, M, w[0], w[1]);
  if (q < Mk) {
    const int j = col[i * ldc + q];
    val[gid] = (1.f - lambda) * ((s[i] * (w[q / k] * v[i * Mk + q])) * s[j]);
  } else {
    const int q2 = q - Mk;
    val[gid] = lambda * (w[q2 / k] * oval[i * Mk + q2]);
  }
}

__global__ __launch_bounds__(256) void lat_sddmm_kernel(int64_t n, int R, const int* __restrict__ col, int64_t ldc,
                                                        const float* __restrict__ g, int64_t ldg,
                                                        const float* __restrict__ h, int64_t ldh, int accumulate,
                                                        float* __restrict__ dA) {
  const int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (i >= n) return;
  const int l = threadIdx.x & 15, c = l * 4;
  const float4 gi = ld4(g + i * ldg + c);
  const int* row = col + i * ldc;
  for (int q = 0; q < R; ++q) {
    const float d = row16_sum(dot4(gi, ld4(h + (int64_t)row[q] * ldh + c)));
    if (l == 0) dA[i * R + q] = accumulate ? dA[i * R + q] + d : d;
  }
}

// a wave per item
__global__ __launch_bounds__(256) void lat_bwd_ds_kernel(int64_t n, int k, int M, const float* __restrict__ dA,
                                                         const float* __restrict__ v, const float* __restrict__ r,
                                                         const float* __restrict__ s, const int* __restrict__ col,
                                                         int64_t ldc, const int* __restrict__ in_ptr,
                                                         const int* __restrict__ in_edge,
                                                         const float* __restrict__ mw, float lambda,
                                                         float* __restrict__ dr) {
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int lane = threadIdx.x & 63;
  const int Mk = M * k, R = 2 * Mk;
  float w[2];
  modal_w(mw, M, w[0], w[1]);
  const float c1 = 1.f - lambda;
  float acc = 0.f;
  for (int q = lane; q < Mk; q += 64)
    acc += (c1 * dA[i * R + q]) * (w[q / k] * v[i * Mk + q]) * s[col[i * ldc + q]];
  for (int m = 0; m < M; ++m) {
    const int end = in_ptr[(int64_t)m * n + i + 1];
    for (int t = in_ptr[(int64_t)m * n + i] + lane; t < end; t += 64) {
      const int64_t e = in_edge[t];
      const int64_t row = e / Mk;
      const int q = (int)(e - row * Mk);
      acc += (c1 * dA[row * R + q]) * (w[m] * v[e]) * s[row];
    }
  }
  const float ds = gmr::wave_sum(acc);
  if (lane == 0) {
    const float si = s[i];
    dr[i] = r[i] == 0.f ? 0.f : -0.5f * ds * (si * si * si);
  }
}

// a wave per row
__global__ __launch_bounds__(256) void lat_bwd_da_kernel(int64_t n, int k, int M, const float* __restrict__ dA,
                                                         const float* __restrict__ v, const float* __restrict__ s,
                                                         const float* __restrict__ dr, const int* __restrict__ col,
                                                         int64_t ldc, const float* __restrict__ oval,
                                                         const float* __restrict__ mw, float lambda,
                                                         float* __restrict__ dv, float* __restrict__ parts) {
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int lane = threadIdx.x & 63;
  const int Mk = M * k, R = 2 * Mk;
  float w[2];
  modal_w(mw, M, w[0], w[1]);
  const float c1 = 1.f - lambda, si = s[i], dri = dr[i];
  float dw[2] = {0.f, 0.f};
  for (int q = lane; q < R; q += 64) {
    const float g = dA[i * R + q];
    if (q < Mk) {
      const int m = q / k;
      const float da = (c1 * g) * si * s[col[i * ldc + q]] + dri;
      dv[i * Mk + q] = w[m] * da;
      const float t = da * v[i * Mk + q];
      if (m == 0) dw[0] += t; else dw[1] += t;
    } else {
      const int q2 = q - Mk;
      const float t = lambda * (oval[i * Mk + q2] * g);
      if (q2 / k == 0) dw[0] += t; else dw[1] += t;
    }
  }
  const float d0 = gmr::wave_sum(dw[0]), d1 = gmr::wave_sum(dw[1]);
  if (lane == 0) {
    parts[2 * i] = d0;
    parts[2 * i + 1] = d1;
  }
}

// dmw = softmax backward of (dw_0, dw_1) = the column sums of parts (n x 2); fixed-order fp64 tree
__global__ void __launch_bounds__(1024) lat_dw_reduce_kernel(int64_t n, const float* __restrict__ parts,
                                                             const float* __restrict__ mw, float* __restrict__ dmw) {
  __shared__ double sh[2][1024];
  const int t = threadIdx.x;
  double a0 = 0.0, a1 = 0.0;
  for (int64_t i = t; i < n; i += 1024) {
    a0 += (double)parts[2 * i];
    a1 += (double)parts[2 * i + 1];
  }
  sh[0][t] = a0;
  sh[1][t] = a1;
  __syncthreads();
  for (int off = 512; off > 0; off >>= 1) {
    if (t < off) {
      sh[0][t] += sh[0][t + off];
      sh[1][t] += sh[1][t + off];
    }
    __syncthreads();
  }
  if (t == 0) {
    float w0, w1;
    modal_w(mw, 2, w0, w1);
    const double d0 = sh[0][0], d1 = sh[1][0];
    const double dot = (double)w0 * d0 + (double)w1 * d1;
    dmw[0] = (float)((double)w0 * (d0 - dot));
    dmw[1] = (float)((double)w1 * (d1 - dot));
  }
}

// a wave per (item, modality); quarter-wave qw takes the edges qw, qw + 4, ... of each list
__global__ __launch_bounds__(256) void lat_bwd_dn_kernel(int64_t n, int k, int M, const float* __restrict__ dv,
                                                         const float* __restrict__ nv0, int64_t ldn0,
                                                         const float* __restrict__ nv1, int64_t ldn1,
                                                         const int* __restrict__ col, int64_t ldc,
                                                         const int* __restrict__ in_ptr,
                                                         const int* __restrict__ in_edge, float* __restrict__ dn0,
                                                         int64_t ldd0, float* __restrict__ dn1, int64_t ldd1) {
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int m = blockIdx.y;
  const int lane = threadIdx.x & 63, qw = lane >> 4, c = (lane & 15) * 4;
  const int Mk = M * k;
  const float* nv = m ? nv1 : nv0;
  const int64_t ld = m ? ldn1 : ldn0;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int sl = qw; sl < k; sl += 4) {
    const int q = m * k + sl;
    acc = gmr::f4_fma(dv[i * Mk + q], ld4(nv + (int64_t)col[i * ldc + q] * ld + c), acc);
  }
  const int end = in_ptr[(int64_t)m * n + i + 1];
  for (int t = in_ptr[(int64_t)m * n + i] + qw; t < end; t += 4) {
    const int64_t e = in_edge[t];
    acc = gmr::f4_fma(dv[e], ld4(nv + (e / Mk) * ld + c), acc);
  }
  acc = gmr::f4_add(acc, gmr::shfl_xor_f4(acc, 16));
  acc = gmr::f4_add(acc, gmr::shfl_xor_f4(acc, 32));
  if (qw == 0) st4((m ? dn1 : dn0) + i * (m ? ldd1 : ldd0) + c, acc);
}

inline bool rows16(const float* p, int64_t ld) { return p && ld >= D && ld % 4 == 0 && gmr::aligned16(p); }
inline bool sizes_ok(int64_t n, int k, int M) {
  return n >= 1 && k >= 1 && k <= 64 && (M == 1 || M == 2) && n * 2 * M * k < (1ll << 31);
}

}  // namespace

// ==================================================================================================== C ABI
extern "C" int gmr_lat_edge_fwd(int64_t n, int32_t k, int32_t M, const float* n0, int64_t ldn0, const int32_t* idx0,
                                int64_t ldi0, const float* n1, int64_t ldn1, const int32_t* idx1, int64_t ldi1,
                                const float* mw, float* v, int32_t* col, int64_t ldc, float* r, float* s,
                                void* stream) {
  GMR_ARG(sizes_ok(n, k, M), "n >= 1, 1 <= k <= 64, M in {1, 2}, n 2 M k < 2^31");
  GMR_ARG(v && col && r && s && idx0 && ldi0 >= k && ldc >= (int64_t)M * k, "null pointer or short row stride");
  GMR_ARG(rows16(n0, ldn0), "rows must be 16-byte aligned with ld >= 64, ld % 4 == 0");
  GMR_ARG(M == 1 || (rows16(n1, ldn1) && idx1 && ldi1 >= k && mw), "the second modality's rows, lists and the weights");
  EdgeArgs a{n, (int)k, (int)M, {n0, n1}, {ldn0, ldn1}, {idx0, idx1}, {ldi0, ldi1}, mw, v, col, ldc, r, s};
  hipLaunchKernelGGL(lat_edge_fwd_kernel, dim3(gmr::grid_for(n, 16)), dim3(256), 0, (hipStream_t)stream, a);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_lat_adj_fwd(int64_t n, int32_t k, int32_t M, const float* v, const float* s, const int32_t* col,
                               int64_t ldc, const float* oval, const float* mw, float lambda, float* val,
                               void* stream) {
  GMR_ARG(sizes_ok(n, k, M), "n >= 1, 1 <= k <= 64, M in {1, 2}, n 2 M k < 2^31");
  GMR_ARG(v && s && col && oval && val && ldc >= (int64_t)M * k && (M == 1 || mw), "null pointer or short row stride");
  hipLaunchKernelGGL(lat_adj_fwd_kernel, dim3(gmr::grid_for(n * 2 * M * k, 256)), dim3(256), 0, (hipStream_t)stream, n,
                     (int)k, (int)M, v, s, col, ldc, oval, mw, lambda, val);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_lat_sddmm(int64_t n, int32_t R, const int32_t* col, int64_t ldc, const float* g, int64_t ldg,
                             const float* h, int64_t ldh, int32_t accumulate, float* dA, void* stream) {
  GMR_ARG(n >= 1 && R >= 1 && n * R < (1ll << 31), "bad sizes");
  GMR_ARG(col && dA && ldc >= R, "null pointer or short row stride");
  GMR_ARG(rows16(g, ldg) && rows16(h, ldh), "rows must be 16-byte aligned with ld >= 64, ld % 4 == 0");
  hipLaunchKernelGGL(lat_sddmm_kernel, dim3(gmr::grid_for(n, 16)), dim3(256), 0, (hipStream_t)stream, n, (int)R, col,
                     ldc, g, ldg, h, ldh, (int)accumulate, dA);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_lat_bwd_ds(int64_t n, int32_t k, int32_t M, const float* dA, const float* v, const float* r,
                              const float* s, const int32_t* col, int64_t ldc, const int32_t* in_ptr,
                              const int32_t* in_edge, const float* mw, float lambda, float* dr, void* stream) {
  GMR_ARG(sizes_ok(n, k, M), "n >= 1, 1 <= k <= 64, M in {1, 2}, n 2 M k < 2^31");
  GMR_ARG(dA && v && r && s && col && in_ptr && in_edge && dr && ldc >= (int64_t)M * k && (M == 1 || mw),
          "null pointer or short row stride");
  hipLaunchKernelGGL(lat_bwd_ds_kernel, dim3(gmr::grid_for(n, 4)), dim3(256), 0, (hipStream_t)stream, n, (int)k, (int)M,
                     dA, v, r, s, col, ldc, in_ptr, in_edge, mw, lambda, dr);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_lat_bwd_da(int64_t n, int32_t k, int32_t M, const float* dA, const float* v, const float* s,
                              const float* dr, const int32_t* col, int64_t ldc, const float* oval, const float* mw,
                              float lambda, float* dv, float* parts, void* stream) {
  GMR_ARG(sizes_ok(n, k, M), "n >= 1, 1 <= k <= 64, M in {1, 2}, n 2 M k < 2^31");
  GMR_ARG(dA && v && s && dr && col && oval && dv && parts && ldc >= (int64_t)M * k && (M == 1 || mw),
          "null pointer or short row stride");
  hipLaunchKernelGGL(lat_bwd_da_kernel, dim3(gmr::grid_for(n, 4)), dim3(256), 0, (hipStream_t)stream, n, (int)k, (int)M,
                     dA, v, s, dr, col, ldc, oval, mw, lambda, dv, parts);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_lat_dw_reduce(int64_t n, const float* parts, const float* mw, float* dmw, void* stream) {
  GMR_ARG(n >= 1 && parts && mw && dmw, "bad args");
  hipLaunchKernelGGL(lat_dw_reduce_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, n, parts, mw, dmw);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_lat_bwd_dn(int64_t n, int32_t k, int32_t M, const float* dv, const float* n0, int64_t ldn0,
                              const float* n1, int64_t ldn1, const int32_t* col, int64_t ldc, const int32_t* in_ptr,
                              const int32_t* in_edge, float* dn0, int64_t ldd0, float* dn1, int64_t ldd1,
                              void* stream) {
  GMR_ARG(sizes_ok(n, k, M), "n >= 1, 1 <= k <= 64, M in {1, 2}, n 2 M k < 2^31");
  GMR_ARG(dv && col && in_ptr && in_edge && ldc >= (int64_t)M * k, "null pointer or short row stride");
  GMR_ARG(rows16(n0, ldn0) && rows16(dn0, ldd0) && (M == 1 || (rows16(n1, ldn1) && rows16(dn1, ldd1))),
          "rows must be 16-byte aligned with ld >= 64, ld % 4 == 0");
  hipLaunchKernelGGL(lat_bwd_dn_kernel, dim3(gmr::grid_for(n, 4), (unsigned)M), dim3(256), 0, (hipStream_t)stream, n,
                     (int)k, (int)M, dv, n0, ldn0, n1, ldn1, col, ldc, in_ptr, in_edge, dn0, ldd0, dn1, ldd1);
  GMR_LAUNCHED();
  return GMR_OK;
}
