// BM3 (models/bm3.py of the reference): the bootstrap loss in one launch.  Four gathered row streams
//   u = ua[users], i = ib[items], t = T[items], v = V[items]           (64 wide; T / V may be absent)
// go through the shared predictor P(x) = x Wp^T + bp; the targets are the dropped-out inputs themselves (no gradient):
//   ui = cos(P(u), drop(i))   iu = cos(P(i), drop(u))
//   t  = cos(P(t), drop(i))   tv = cos(P(t), drop(t))   v = cos(P(v), drop(i))   vt = cos(P(v), drop(v))
//   cos(a, b) = <a, b> / (max(|a|, 1e-8) max(|b|, 1e-8))
//
//   gmr_bm3_loss_fwd_bwd   a workgroup owns 16 batch rows: gather, P on v_mfma_f32_16x16x4_f32 (wave w = stream w, Wp
//                          and Wp^T staged in LDS), targets, the six cosines, the gradient rows d_on of the four online
//                          rows, dx = d_on Wp on the MFMA again, the contribution rows of [users | items]
//   gmr_bm3_loss_reduce    loss[] = [total, ui, iu, t, v, tv, vt, reg] from the cosines and the two squared table
//                          norms, and the two coefficients of the dense reg gradient (all on the device)
//   gmr_bm3_reg_bwd        dG += coef[side] G over the rows of [ua; ib]
//
// Drawn keep masks belong to a TABLE row, not a batch row: stream s (0 u, 1 i, 2 t, 3 v) of table row id (the user id
// for u, the item id for the others) draws
//   r = Philox(key = seed + (site + s) * 0x9E3779B97F4A7C15, subsequence = step, offset = id * 16 + c / 4)
// for its columns c..c+3 (c a multiple of 4; words x, y, z, w in column order) and keeps a column when
//   (float)(word >> 8) * 2^-24 < 1.f - p,
// so an id that occurs twice in a batch (or in two batches of one step) has one mask.
//
// No float atomics; a row's result depends on its own inputs only (one fixed MFMA k order, one butterfly per row sum).
#include <math.h>

#include "gemm_impl.h"

namespace {

constexpr int D = 64, TR = 16, LDX = D + 4, NS = 4;
constexpr uint64_t SITE_MIX = 0x9E3779B97F4A7C15ull;
constexpr float COS_EPS = 1e-8f;

using gmr::ld4, gmr::st4, gmr::dot4;
__device__ __forceinline__ float row16_sum(float v) {
#pragma unroll
  for (int m = 8; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// acc[ct] (16 rows x columns 16 ct .. 16 ct + 15) += A[16][64] . Bt[col][0..63]^T, both in LDS with row stride LDX.
// Lane l feeds row / column l & 15 and, per float4, the k values 16 (l >> 4) + 4 s .. + 3 (the same on both sides).
// acc element e of lane l: row 4 (l >> 4) + e, column 16 ct + (l & 15).
__device__ __forceinline__ void mm16(const float* sA, const float* sBt, floatx4 (&acc)[4]) {
  const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const float4 a = ld4(sA + r * LDX + 16 * q + 4 * s);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const float4 b = ld4(sBt + (16 * ct + r) * LDX + 16 * q + 4 * s);
      acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc[ct], 0, 0, 0);
      acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc[ct], 0, 0, 0);
      acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc[ct], 0, 0, 0);
      acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc[ct], 0, 0, 0);
    }
  }
}

struct Bm3Args {
  int B;
  int64_t U;
  const float* G;
  int64_t ldg;
  const float* T;
  int64_t ldt;
  const float* V;
  int64_t ldv;
  const int32_t* users;
  const int32_t* items;
  const float* Wp;
  int64_t ldw;
  const float* bp;
  float p, cl_weight, inv_norm;
  int drop;  // 0 none, 1 keep bytes given, 2 drawn (and written to keep_out)
  const uint8_t* keep[NS];
  int64_t ldk;
  uint64_t seed, step, site;
  uint8_t* keep_out[NS];
  int64_t ldko;
  float* terms;
  float* contrib;
  int64_t ldc;
  float* xg;
  float* don;
};

// one cosine against a target: the value, and the two coefficients of its gradient d cos / d a = cb b - ca a
struct Cos {
  float c, cb, ca;
};
__device__ __forceinline__ Cos cosine(float ab, float aa, float bb) {
  const float ra = sqrtf(aa), na = fmaxf(ra, COS_EPS), nb = fmaxf(sqrtf(bb), COS_EPS);
  Cos o;
  o.cb = 1.f / (na * nb);
  o.c = ab * o.cb;
  o.ca = ra > COS_EPS ? o.c / (na * na) : 0.f;  // a clamped norm is a constant
  return o;
}
__device__ __forceinline__ float4 axpby(float a, float4 x, float b, float4 y) {
  return make_float4(a * x.x + b * y.x, a * x.y + b * y.y, a * x.z + b * y.z, a * x.w + b * y.w);
}

// In the element phases thread tid owns row tid >> 4, columns 4 (tid & 15) .. + 3 of the tile, in all four streams.
__global__ __launch_bounds__(256) void bm3_loss_kernel(Bm3Args a) {
  __shared__ __attribute__((aligned(16))) float sW[D * LDX];        // Wp[j][k]
  __shared__ __attribute__((aligned(16))) float sWt[D * LDX];       // Wp^T[k][j]
  // the gathered rows by stream, then the online rows, then d_on, each in place of the last: wave w alone reads and
  // writes stream w in the MFMA phases (its stores depend on all its loads), a thread its own four floats in between
  __shared__ __attribute__((aligned(16))) float sR[NS * TR * LDX];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  for (int i = tid; i < D * 16; i += 256) {
    const int j = i >> 4, k = (i & 15) * 4;
    st4(sW + j * LDX + k, ld4(a.Wp + j * a.ldw + k));
  }
  {
    const int k = tid & 63, jg = tid >> 6;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int j0 = 16 * it + 4 * jg;
      st4(sWt + k * LDX + j0, make_float4(a.Wp[(j0 + 0) * a.ldw + k], a.Wp[(j0 + 1) * a.ldw + k],
                                          a.Wp[(j0 + 2) * a.ldw + k], a.Wp[(j0 + 3) * a.ldw + k]));
    }
  }
  const int row = tid >> 4, c = (tid & 15) * 4;
  const int64_t b = (int64_t)blockIdx.x * TR + row;
  const bool ok = b < a.B;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 x[NS] = {z, z, z, z};
  int64_t id[NS] = {0, 0, 0, 0};
  if (ok) {
    id[0] = a.users[b];
    id[1] = id[2] = id[3] = a.items[b];
    x[0] = ld4(a.G + id[0] * a.ldg + c);
    x[1] = ld4(a.G + (a.U + id[1]) * a.ldg + c);
    if (a.T) x[2] = ld4(a.T + id[2] * a.ldt + c);
    if (a.V) x[3] = ld4(a.V + id[3] * a.ldv + c);
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    st4(sR + (s * TR + row) * LDX + c, x[s]);  // tail rows: zeros, never stored
    if (ok) st4(a.xg + ((int64_t)s * a.B + b) * D + c, x[s]);
  }
  __syncthreads();
  {  // the online rows of stream w
    floatx4 acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    mm16(sR + w * TR * LDX, sW, acc);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const int col = 16 * ct + (lane & 15);
      const float bias = a.bp[col];
#pragma unroll
      for (int e = 0; e < 4; ++e) sR[(w * TR + 4 * (lane >> 4) + e) * LDX + col] = acc[ct][e] + bias;
    }
  }
  __syncthreads();
  // targets: the gathered rows through their table row's keep mask
  const float p_keep = 1.f - a.p, scale = 1.f / (1.f - a.p);
  float4 tg[NS], on[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    on[s] = ld4(sR + (s * TR + row) * LDX + c);
    uint32_t bits = 0xFu;
    const bool has = s < 2 || (s == 2 ? a.T != nullptr : a.V != nullptr);
    if (ok && has && a.drop == 1) {
      const uint8_t* kp = a.keep[s] + b * a.ldk + c;
      bits = (kp[0] ? 1u : 0u) | (kp[1] ? 2u : 0u) | (kp[2] ? 4u : 0u) | (kp[3] ? 8u : 0u);
    } else if (ok && has && a.drop == 2) {
      const uint4 r = gmr::Philox::gen(a.seed + (a.site + (uint64_t)s) * SITE_MIX, a.step,
                                       (uint64_t)id[s] * 16 + (uint64_t)(c >> 2));
      const float k24 = 1.0f / 16777216.0f;
      bits = ((float)(r.x >> 8) * k24 < p_keep ? 1u : 0u) | ((float)(r.y >> 8) * k24 < p_keep ? 2u : 0u) |
             ((float)(r.z >> 8) * k24 < p_keep ? 4u : 0u) | ((float)(r.w >> 8) * k24 < p_keep ? 8u : 0u);
      if (a.keep_out[s]) {
        uint8_t* ko = a.keep_out[s] + b * a.ldko + c;
        ko[0] = bits & 1u, ko[1] = (bits >> 1) & 1u, ko[2] = (bits >> 2) & 1u, ko[3] = (bits >> 3) & 1u;
      }
    }
    const float m = a.drop ? scale : 1.f;
    tg[s] = make_float4(bits & 1u ? x[s].x * m : 0.f, bits & 2u ? x[s].y * m : 0.f, bits & 4u ? x[s].z * m : 0.f,
                        bits & 8u ? x[s].w * m : 0.f);
  }
  float oo[NS], tt[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    oo[s] = row16_sum(dot4(on[s], on[s]));
    tt[s] = row16_sum(dot4(tg[s], tg[s]));
  }
  const Cos ui = cosine(row16_sum(dot4(on[0], tg[1])), oo[0], tt[1]);
  const Cos iu = cosine(row16_sum(dot4(on[1], tg[0])), oo[1], tt[0]);
  const Cos c_t = cosine(row16_sum(dot4(on[2], tg[1])), oo[2], tt[1]);
  const Cos c_tv = cosine(row16_sum(dot4(on[2], tg[2])), oo[2], tt[2]);
  const Cos c_v = cosine(row16_sum(dot4(on[3], tg[1])), oo[3], tt[1]);
  const Cos c_vt = cosine(row16_sum(dot4(on[3], tg[3])), oo[3], tt[3]);
  const bool hasT = a.T != nullptr, hasV = a.V != nullptr;
  // d loss / d online row: every term is 1 - mean cos, the modal ones weighted by cl_weight
  const float wg = -a.inv_norm, wm = -a.inv_norm * a.cl_weight;
  float4 d[NS];
  d[0] = axpby(wg * ui.cb, tg[1], -wg * ui.ca, on[0]);
  d[1] = axpby(wg * iu.cb, tg[0], -wg * iu.ca, on[1]);
  d[2] = gmr::f4_add(axpby(wm * c_t.cb, tg[1], -wm * (c_t.ca + c_tv.ca), on[2]), gmr::f4_scale(wm * c_tv.cb, tg[2]));
  d[3] = gmr::f4_add(axpby(wm * c_v.cb, tg[1], -wm * (c_v.ca + c_vt.ca), on[3]), gmr::f4_scale(wm * c_vt.cb, tg[3]));
  if (!hasT) d[2] = z;
  if (!hasV) d[3] = z;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    st4(sR + (s * TR + row) * LDX + c, d[s]);  // the same thread read these four floats
    if (ok) st4(a.don + ((int64_t)s * a.B + b) * D + c, d[s]);
  }
  if (ok) {
    if ((tid & 15) == 0) {
      const int64_t B = a.B;
      a.terms[b] = ui.c;
      a.terms[B + b] = iu.c;
      a.terms[2 * B + b] = hasT ? c_t.c : 0.f;
      a.terms[3 * B + b] = hasV ? c_v.c : 0.f;
      a.terms[4 * B + b] = hasT ? c_tv.c : 0.f;
      a.terms[5 * B + b] = hasV ? c_vt.c : 0.f;
    }
    st4(a.contrib + b * a.ldc + D + c, z);  // a user row has no modal columns
    st4(a.contrib + b * a.ldc + 2 * D + c, z);
  }
  __syncthreads();
  {  // dx of stream w = d_on Wp: [dx_u | 0 | 0] on the user rows, [dx_i | dx_t | dx_v] on the item rows
    floatx4 acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    if (w < 2 || (w == 2 ? hasT : hasV)) mm16(sR + w * TR * LDX, sWt, acc);  // wave-uniform
    const int64_t r0 = (int64_t)blockIdx.x * TR + 4 * (lane >> 4);
    const int64_t rbase = w == 0 ? 0 : (int64_t)a.B;
    const int cbase = w < 2 ? 0 : (w - 1) * D;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (r0 + e < a.B) {
        float* dst = a.contrib + (rbase + r0 + e) * a.ldc + cbase + (lane & 15);
#pragma unroll
        for (int q = 0; q < 4; ++q) dst[16 * q] = acc[q][e];
      }
    }
  }
}

// loss[0..7] = [total, ui, iu, t, v, tv, vt, reg], loss[8], loss[9] = reg_weight / (I |ua|_F), reg_weight / (I |ib|_F);
// fixed-order fp64 tree
__global__ void __launch_bounds__(1024) bm3_loss_reduce_kernel(int B, const float* __restrict__ terms,
                                                               const float* __restrict__ sq, int has_t, int has_v,
                                                               float reg_weight, float cl_weight, float inv_norm,
                                                               float inv_items, float* __restrict__ loss) {
  __shared__ double s[6][1024];
  const int t = threadIdx.x;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int b = t; b < B; b += 1024)
    for (int k = 0; k < 6; ++k) acc[k] += (double)terms[(int64_t)k * B + b];
  for (int k = 0; k < 6; ++k) s[k][t] = acc[k];
  __syncthreads();
  for (int off = 512; off > 0; off >>= 1) {
    if (t < off)
      for (int k = 0; k < 6; ++k) s[k][t] += s[k][t + off];
    __syncthreads();
  }
  if (t == 0) {
    float m[6];
    for (int k = 0; k < 6; ++k) {
      const bool has = k < 2 || ((k & 1) ? has_v : has_t);  // order ui, iu, t, v, tv, vt
      m[k] = has ? (float)(1.0 - s[k][0] * (double)inv_norm) : 0.f;
    }
    const float nu = sqrtf(sq[0]), ni = sqrtf(sq[1]);
    const float reg = (nu + ni) * inv_items;
    loss[0] = (m[0] + m[1]) + reg_weight * reg + cl_weight * (m[2] + m[3] + m[4] + m[5]);
    for (int k = 0; k < 6; ++k) loss[1 + k] = m[k];
    loss[7] = reg;
    loss[8] = nu > 0.f ? reg_weight * inv_items / nu : 0.f;
    loss[9] = ni > 0.f ? reg_weight * inv_items / ni : 0.f;
  }
}

// dG[r] += coef[r < n_users ? 0 : 1] G[r]: 16 lanes per row, 4 columns per lane
__global__ void __launch_bounds__(256) bm3_reg_bwd_kernel(int64_t n_rows, int64_t n_users,
                                                          const float* __restrict__ coef, const float* __restrict__ G,
                                                          int64_t ldg, float* __restrict__ dG, int64_t ldd) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t r = gid >> 4;
  if (r >= n_rows) return;
  const int c = (int)(gid & 15) * 4;
  const float k = coef[r < n_users ? 0 : 1];
  st4(dG + r * ldd + c, gmr::f4_fma(k, ld4(G + r * ldg + c), ld4(dG + r * ldd + c)));
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool rows16(const float* p, int64_t ld) { return ld >= D && ld % 4 == 0 && al16(p); }

}  // namespace

// ==================================================================================================== C ABI
extern "C" int32_t gmr_bm3_tile_rows(void) { return TR; }

extern "C" int gmr_bm3_loss_fwd_bwd(int32_t B, int64_t n_users, const float* G, int64_t ldg, const float* T,
                                    int64_t ldt, const float* V, int64_t ldv, const int32_t* users,
                                    const int32_t* items, const float* Wp, int64_t ldw, const float* bp, float p,
                                    float cl_weight, float inv_norm, int32_t drop_mode, const uint8_t* keep_u,
                                    const uint8_t* keep_i, const uint8_t* keep_t, const uint8_t* keep_v, int64_t ldk,
                                    uint64_t seed, uint64_t step, uint64_t site, uint8_t* keep_out_u,
                                    uint8_t* keep_out_i, uint8_t* keep_out_t, uint8_t* keep_out_v, int64_t ldko,
                                    float* terms, float* contrib, int64_t ldc, float* xg, float* don, void* stream) {
  GMR_ARG(B >= 1 && n_users >= 0, "bad sizes");
  GMR_ARG(G && users && items && Wp && bp && terms && contrib && xg && don, "null pointer");
  GMR_ARG(p >= 0.f && p < 1.f, "dropout must be in [0, 1)");
  GMR_ARG(rows16(G, ldg) && rows16(Wp, ldw) && (!T || rows16(T, ldt)) && (!V || rows16(V, ldv)),
          "table rows must be 16-byte aligned with ld >= 64");
  GMR_ARG(ldc >= 3 * D && ldc % 4 == 0 && al16(contrib) && al16(xg) && al16(don),
          "contrib / xg / don rows must be 16-byte aligned (ldc >= 192)");
  GMR_ARG(drop_mode >= 0 && drop_mode <= 2, "bad dropout mode");
  GMR_ARG(drop_mode != 1 || (ldk >= D && keep_u && keep_i && (!T || keep_t) && (!V || keep_v)),
          "given keep bytes: one array per present stream, ldk >= 64");
  GMR_ARG((T || (!keep_t && !keep_out_t)) && (V || (!keep_v && !keep_out_v)),
          "keep bytes of a modality whose table is null");
  GMR_ARG(!(keep_out_u || keep_out_i || keep_out_t || keep_out_v) || ldko >= D, "bad keep_out stride");
  Bm3Args a{B, n_users, G, ldg, T, ldt, V, ldv, users, items, Wp, ldw, bp, p, cl_weight, inv_norm, drop_mode,
            {keep_u, keep_i, keep_t, keep_v}, ldk, seed, step, site, {keep_out_u, keep_out_i, keep_out_t, keep_out_v},
            ldko, terms, contrib, ldc, xg, don};
  hipLaunchKernelGGL(bm3_loss_kernel, dim3((unsigned)((B + TR - 1) / TR)), dim3(256), 0, (hipStream_t)stream, a);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_bm3_loss_reduce(int32_t B, const float* terms, const float* sqnorms, int32_t has_t, int32_t has_v,
                                   float reg_weight, float cl_weight, float inv_norm, int64_t n_items, float* loss,
                                   void* stream) {
  GMR_ARG(B >= 1 && n_items >= 1 && terms && sqnorms && loss, "bad args");
  hipLaunchKernelGGL(bm3_loss_reduce_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, B, terms, sqnorms,
                     (int)has_t, (int)has_v, reg_weight, cl_weight, inv_norm, 1.f / (float)n_items, loss);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_bm3_reg_bwd(int64_t n_rows, int64_t n_users, const float* coef, const float* G, int64_t ldg,
                               float* dG, int64_t ldd, void* stream) {
  GMR_ARG(n_rows >= 1 && n_users >= 0 && n_users <= n_rows && coef && G && dG, "bad args");
  GMR_ARG(rows16(G, ldg) && rows16(dG, ldd), "rows must be 16-byte aligned with ld >= 64");
  hipLaunchKernelGGL(bm3_reg_bwd_kernel, dim3(gmr::grid_for(n_rows * 16, 256)), dim3(256), 0, (hipStream_t)stream,
                     n_rows, n_users, coef, G, ldg, dG, ldd);
  GMR_LAUNCHED();
  return GMR_OK;
}
