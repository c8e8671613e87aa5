// DDRM (models/ddrm.py of the reference): diffusion on 64-wide LightGCN embedding rows with two conditional
// denoisers  out = W2 tanh(W1 [x | emb(t) | cond] + b1) + b2  (hidden width H, any multiple of 4 in 4..1024).
//
//   gmr_ddrm_denoise_fwd   gather x0 / cond rows, q_sample, dropout, both layers and the row's mean (x0 - out)^2 in
//                          one launch: a workgroup owns 32 rows, activations stay in LDS, products on
//                          v_mfma_f32_32x32x2_f32.  The time columns of W1 are folded by the caller into a T x H table
//                          TB[t] = W1[:, 64:128] emb_layer(temb(t)) + b1, so the first layer has K = 128 + one gathered
//                          row.  H is walked in chunks of 128 columns: columns past H are masked (layer 1's N, layer
//                          2's K).
//   gmr_ddrm_chain         the reverse chain of full_sort_predict, x <- c1[i] net(x, cond, i) + c2[i] x (+ sigma[i]
//                          noise where i != 0) for i = S-1..0, in one launch on the same tile code
//   gmr_ddrm_loss_fwd_bwd  the weighted row loss with its gradient rows
//   gmr_ddrm_input_bwd     d loss / d (gathered x0, cond rows) from the first layer's input gradients
//
// No float atomics; every sum has one fixed order per row, whatever tile the row falls in: a row's result depends
// on its own inputs and its global row number (Philox keys) only.
#include <math.h>

#include "gemm_impl.h"

namespace {

constexpr int D = 64, TR = 32, LDX = D + 4, HC = 128, LDHC = HC + 4;
constexpr int LDW1 = 3 * D;  // in_layers.0.weight rows: [x | time | cond]
constexpr uint64_t SITE_MIX = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ floatx16 zero16() {
  floatx16 z;
#pragma unroll
  for (int e = 0; e < 16; ++e) z[e] = 0.f;
  return z;
}

// acc (32 rows x 32 columns col0..) += A[32][64] (LDS, row stride LDX) . W[col][0..63]^T (global, row stride ldw).
// Lane l feeds row / column l & 31 and the k half l >> 5.  Columns past H read row H - 1 (the caller drops them).
__device__ __forceinline__ void mm_in(const float* sA, const float* __restrict__ W, int ldw, int col0, int H,
                                      floatx16& acc) {
  const int lane = threadIdx.x & 63, h = lane >> 5, r = lane & 31;
  const int wr = min(col0 + r, H - 1);
  const float* wp = W + (size_t)wr * ldw + h * (D / 2);
  const float* sp = sA + r * LDX + h * (D / 2);
#pragma unroll 4
  for (int s = 0; s < D / 2; s += 4) {
    const float4 a = *reinterpret_cast<const float4*>(sp + s);
    const float4 b = *reinterpret_cast<const float4*>(wp + s);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
  }
}

// acc (32 rows x output columns 32 ct..) += sH[32][64 kh .. 64 kh + 63] . W2[col][hc0 + 64 kh ..]^T; k past H is
// zero on both sides (H is a multiple of 4, so a float4 of k lies wholly inside or outside)
__device__ __forceinline__ void mm_out(const float* sHc, const float* __restrict__ W2, int H, int hc0, int ct, int kh,
                                       floatx16& acc) {
  const int lane = threadIdx.x & 63, h = lane >> 5, r = lane & 31;
  const int kg = hc0 + 64 * kh + 32 * h;
  const float* wp = W2 + (size_t)(32 * ct + r) * H + kg;
  const float* sp = sHc + r * LDHC + 64 * kh + 32 * h;
#pragma unroll 4
  for (int s = 0; s < 32; s += 4) {
    const float4 a = *reinterpret_cast<const float4*>(sp + s);
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (kg + s < H) b = *reinterpret_cast<const float4*>(wp + s);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
  }
}

// sO[32][64] = W2 tanh(W1x sX + W1c sC + TB[sT]) + b2 for the tile's 32 rows.  The caller has synchronised after
// filling sX, sC, sT; ends with a barrier.  hout: the hidden rows (N x H, row stride ldh) or NULL.
// acc element e of lane l: row (e & 3) + 8 (e >> 2) + 4 (l >> 5), column col0 + (l & 31).
__device__ __forceinline__ void net_tile(const float* sX, const float* sC, const int* sT, float* sHc, float* sO,
                                         const float* __restrict__ W1, const float* __restrict__ TB,
                                         const float* __restrict__ W2, const float* __restrict__ b2, int H,
                                         float* __restrict__ hout, int64_t ldh, int64_t r0, int64_t N) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, hh = lane >> 5, lc = lane & 31;
  const int ct = w & 1, kh = w >> 1;
  floatx16 acc2 = zero16();
  for (int hc0 = 0; hc0 < H; hc0 += HC) {
    const int col0 = hc0 + 32 * w;
    if (col0 < H) {  // wave-uniform
      floatx16 acc = zero16();
      mm_in(sX, W1, LDW1, col0, H, acc);
      mm_in(sC, W1 + 2 * D, LDW1, col0, H, acc);
      const int c = col0 + lc;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int r = (e & 3) + 8 * (e >> 2) + 4 * hh;
        float v = 0.f;
        if (c < H) {
          v = tanhf(acc[e] + TB[(size_t)sT[r] * H + c]);
          if (hout && r0 + r < N) hout[(r0 + r) * ldh + c] = v;
        }
        sHc[r * LDHC + 32 * w + lc] = v;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e) sHc[((e & 3) + 8 * (e >> 2) + 4 * hh) * LDHC + 32 * w + lc] = 0.f;
    }
    __syncthreads();
    if (hc0 + 64 * kh < H) mm_out(sHc, W2, H, hc0, ct, kh, acc2);  // wave-uniform
    __syncthreads();  // every wave has read the chunk before the next one overwrites it
  }
  // the two k halves of an output tile are added in one order: half 0 + half 1, then the bias
  if (kh == 1) {
#pragma unroll
    for (int e = 0; e < 16; ++e) sO[((e & 3) + 8 * (e >> 2) + 4 * hh) * LDX + 32 * ct + lc] = acc2[e];
  }
  __syncthreads();
  if (kh == 0) {
    const float b = b2[32 * ct + lc];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int o = ((e & 3) + 8 * (e >> 2) + 4 * hh) * LDX + 32 * ct + lc;
      sO[o] = (acc2[e] + sO[o]) + b;
    }
  }
  __syncthreads();
}

// eight N(0, 1) values of row `row`, columns c0..c0+7 (c0 a multiple of 8): Philox counter row * 16 + column / 4
__device__ __forceinline__ void randn8(uint64_t key, uint64_t step, uint64_t row, int c0, float* v) {
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const uint4 r = gmr::Philox::gen(key, step, row * 16 + (uint64_t)(c0 / 4 + q));
    const float2 a = gmr::box_muller(r.x, r.y), b = gmr::box_muller(r.z, r.w);
    v[4 * q] = a.x, v[4 * q + 1] = a.y, v[4 * q + 2] = b.x, v[4 * q + 3] = b.y;
  }
}

// In the element phases thread tid owns row tid >> 3, columns 8 (tid & 7) .. + 7 of the tile.
struct FwdArgs {
  int64_t N, row_off;
  int H, T;
  const float* X;
  int64_t ldx;
  const int32_t* idx_x;
  const float* C;
  int64_t ldc;
  const int32_t* idx_c;
  const int32_t* t;
  const float* sqrt_ac;
  const float* sqrt_1mac;
  const float* noise;
  int64_t ldn;
  int drop;  // 0 none, 1 keep bytes given, 2 drawn (and written to keep_out)
  const uint8_t* keep;
  int64_t ldk;
  uint64_t seed, step, site;
  const float *W1, *TB, *W2, *b2;
  float* out;
  int64_t ldo;
  float* xd;
  int64_t ldxd;
  uint8_t* keep_out;
  int64_t ldko;
  float* h;
  int64_t ldh;
  float* rowmse;
};

__global__ __launch_bounds__(256) void ddrm_fwd_kernel(FwdArgs a) {
  __shared__ __attribute__((aligned(16))) float sX[TR * LDX];
  __shared__ __attribute__((aligned(16))) float sC[TR * LDX];
  __shared__ __attribute__((aligned(16))) float sX0[TR * LDX];
  __shared__ __attribute__((aligned(16))) float sO[TR * LDX];
  __shared__ __attribute__((aligned(16))) float sHc[TR * LDHC];
  __shared__ int sT[TR];
  const int tid = threadIdx.x, row = tid >> 3, c0 = (tid & 7) * 8;
  const int64_t r0 = (int64_t)blockIdx.x * TR, gr = r0 + row;
  const bool ok = gr < a.N;
  float x0[8], xv[8], cv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) x0[j] = xv[j] = cv[j] = 0.f;
  int tt = 0;
  if (ok) {
    tt = min(max(a.t[gr], 0), a.T - 1);  // a timestep outside the tables never becomes an address
    const int64_t ix = a.idx_x ? (int64_t)a.idx_x[gr] : gr, ic = a.idx_c ? (int64_t)a.idx_c[gr] : gr;
    const float* xp = a.X + ix * a.ldx + c0;
    const float* cp = a.C + ic * a.ldc + c0;
    float nz[8];
    if (a.noise) {
#pragma unroll
      for (int j = 0; j < 8; ++j) nz[j] = a.noise[gr * a.ldn + c0 + j];
    } else {
      randn8(a.seed + a.site * SITE_MIX, a.step, (uint64_t)(a.row_off + gr), c0, nz);
    }
    uint32_t bits = 0xFFu;
    if (a.drop == 1) {
      bits = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) bits |= (a.keep[gr * a.ldk + c0 + j] ? 1u : 0u) << j;
    } else if (a.drop == 2) {
      // one Philox word per 32 columns of the row: p = 1/2, a keep bit per column
      const uint4 r = gmr::Philox::gen(a.seed + (a.site + 1) * SITE_MIX, a.step, (uint64_t)(a.row_off + gr));
      bits = ((c0 < 32 ? r.x : r.y) >> (c0 & 31)) & 0xFFu;
    }
    const float sa = a.sqrt_ac[tt], s1 = a.sqrt_1mac[tt];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      x0[j] = xp[j];
      cv[j] = cp[j];
      const float xn = sa * x0[j] + s1 * nz[j];
      xv[j] = a.drop == 0 ? xn : ((bits >> j) & 1u) ? xn * 2.f : 0.f;  // nn.Dropout(0.5): kept values / 0.5
      if (a.xd) a.xd[gr * a.ldxd + c0 + j] = xv[j];
      if (a.drop == 2 && a.keep_out) a.keep_out[gr * a.ldko + c0 + j] = (uint8_t)((bits >> j) & 1u);
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sX[row * LDX + c0 + j] = xv[j];  // tail rows: zeros, never stored
    sC[row * LDX + c0 + j] = cv[j];
    sX0[row * LDX + c0 + j] = x0[j];
  }
  if ((tid & 7) == 0) sT[row] = tt;
  __syncthreads();
  net_tile(sX, sC, sT, sHc, sO, a.W1, a.TB, a.W2, a.b2, a.H, a.h, a.ldh, r0, a.N);
  float sq = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float o = sO[row * LDX + c0 + j];
    if (ok) a.out[gr * a.ldo + c0 + j] = o;
    const float d = x0[j] - o;
    sq = fmaf(d, d, sq);
  }
  // the row's eight partial sums, one butterfly order
  sq += __shfl_xor(sq, 1);
  sq += __shfl_xor(sq, 2);
  sq += __shfl_xor(sq, 4);
  if (ok && (tid & 7) == 0 && a.rowmse) a.rowmse[gr] = sq * (1.f / D);
}

struct ChainArgs {
  int64_t N, row_off;
  int H, S, T;
  const float* xs;
  int64_t ldx;
  const float* noise0;
  int64_t ldn0;
  float qa, qb;
  const float* C;
  int64_t ldc;
  const int32_t* idx_c;
  const float *W1, *TB, *W2, *b2, *c1, *c2, *sigma;
  const float* step_noise;  // [S][N][64] indexed by timestep, or NULL: Philox when sigma is given
  uint64_t seed, step, site;
  float* out;
  int64_t ldo;
};

__global__ __launch_bounds__(256) void ddrm_chain_kernel(ChainArgs a) {
  __shared__ __attribute__((aligned(16))) float sX[TR * LDX];
  __shared__ __attribute__((aligned(16))) float sC[TR * LDX];
  __shared__ __attribute__((aligned(16))) float sO[TR * LDX];
  __shared__ __attribute__((aligned(16))) float sHc[TR * LDHC];
  __shared__ int sT[TR];
  const int tid = threadIdx.x, row = tid >> 3, c0 = (tid & 7) * 8;
  const int64_t r0 = (int64_t)blockIdx.x * TR, gr = r0 + row;
  const bool ok = gr < a.N;
  float x[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = 0.f;
  if (ok) {
    const int64_t ic = a.idx_c ? (int64_t)a.idx_c[gr] : gr;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float xs = a.xs[gr * a.ldx + c0 + j];
      x[j] = a.noise0 ? a.qa * xs + a.qb * a.noise0[gr * a.ldn0 + c0 + j] : xs;
      sC[row * LDX + c0 + j] = a.C[ic * a.ldc + c0 + j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) sC[row * LDX + c0 + j] = 0.f;
  }
  for (int i = a.S - 1; i >= 0; --i) {
#pragma unroll
    for (int j = 0; j < 8; ++j) sX[row * LDX + c0 + j] = x[j];
    if ((tid & 7) == 0) sT[row] = i;
    __syncthreads();
    net_tile(sX, sC, sT, sHc, sO, a.W1, a.TB, a.W2, a.b2, a.H, nullptr, 0, r0, a.N);
    const float k1 = a.c1[i], k2 = a.c2[i];
    float nz[8];
    const bool noisy = a.sigma && i != 0 && ok;
    if (noisy) {
      if (a.step_noise) {
#pragma unroll
        for (int j = 0; j < 8; ++j) nz[j] = a.step_noise[((int64_t)i * a.N + gr) * D + c0 + j];
      } else {
        randn8(a.seed + a.site * SITE_MIX, a.step, (uint64_t)(a.row_off + gr) * (uint64_t)a.T + (uint64_t)i, c0, nz);
      }
    }
    const float sg = noisy ? a.sigma[i] : 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = k1 * sO[row * LDX + c0 + j] + k2 * x[j];
      if (noisy) v = v + sg * nz[j];
      x[j] = v;
    }
    // the next step's barrier (after sX is rewritten) orders these sO reads before the next net_tile's writes
  }
  if (ok) {
#pragma unroll
    for (int j = 0; j < 8; ++j) a.out[gr * a.ldo + c0 + j] = x[j];
  }
}

// ------------------------------------------------------------------------------------------------ row loss
using gmr::ld4, gmr::st4, gmr::dot4;
__device__ __forceinline__ float row16_sum(float v) {
#pragma unroll
  for (int m = 8; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
// F.softplus (beta 1, threshold 20), its small branch as max(x, 0) + log1p(exp(-|x|))
__device__ __forceinline__ float softplus(float x) {
  return x > 20.f ? x : fmaxf(x, 0.f) + log1pf(expf(-fabsf(x)));
}
__device__ __forceinline__ float sigmoid(float x) {
  const float e = expf(-fabsf(x));
  return x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}
__device__ __forceinline__ float log_sigmoid(float x) { return fminf(x, 0.f) - log1pf(expf(-fabsf(x))); }

// 16 lanes per batch row, 4 columns per lane.  terms: [w | softplus | recon | loss_b] (4 x B)
__global__ void __launch_bounds__(256) ddrm_loss_rows_kernel(
    int B, int64_t U, const float* __restrict__ G, int64_t ldg, const int* __restrict__ users,
    const int* __restrict__ pos, const int* __restrict__ neg, const float* __restrict__ out_u, int64_t ldou,
    const float* __restrict__ out_i, int64_t ldoi, const float* __restrict__ mse_u, const float* __restrict__ mse_i,
    const float* __restrict__ reg, float alpha, float beta, float reg_weight, float inv_norm,
    float* __restrict__ terms, float* __restrict__ contrib, int64_t ldc, float* __restrict__ dout_u,
    float* __restrict__ dout_i) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int b = (int)(gid >> 4);
  const bool ok = b < B;
  const int c = (int)(gid & 15) * 4;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 u = z, p = z, n = z, ou = z, oi = z;
  if (ok) {
    u = ld4(G + (int64_t)users[b] * ldg + c);
    p = ld4(G + (U + pos[b]) * ldg + c);
    n = ld4(G + (U + neg[b]) * ldg + c);
    ou = ld4(out_u + (int64_t)b * ldou + c);
    oi = ld4(out_i + (int64_t)b * ldoi + c);
  }
  const float ps = row16_sum(dot4(u, p)), ns = row16_sum(dot4(u, n));
  if (!ok) return;
  const float x = ns - ps;
  const float w = expf(beta * log_sigmoid(ps));  // sigmoid(pos)^beta, detached
  const float sp = softplus(x);
  const float rec = 0.5f * (mse_u[b] + mse_i[b]);
  if ((gid & 15) == 0) {
    terms[b] = w;
    terms[(int64_t)B + b] = sp;
    terms[2 * (int64_t)B + b] = rec;
    terms[3 * (int64_t)B + b] = w * ((1.f - alpha) * (sp + reg_weight * reg[0]) + alpha * rec);
  }
  const float cs = w * (1.f - alpha) * sigmoid(x) * inv_norm;  // d loss / d (neg - pos)
  const float kr = w * alpha * inv_norm * (0.5f * 2.f / D);    // d loss / d (x0 - out), per unit difference
  const float4 du = make_float4(u.x - ou.x, u.y - ou.y, u.z - ou.z, u.w - ou.w);
  const float4 dp = make_float4(p.x - oi.x, p.y - oi.y, p.z - oi.z, p.w - oi.w);
  st4(contrib + (int64_t)b * ldc + c, make_float4(cs * (n.x - p.x) + kr * du.x, cs * (n.y - p.y) + kr * du.y,
                                                  cs * (n.z - p.z) + kr * du.z, cs * (n.w - p.w) + kr * du.w));
  st4(contrib + ((int64_t)B + b) * ldc + c, make_float4(kr * dp.x - cs * u.x, kr * dp.y - cs * u.y,
                                                        kr * dp.z - cs * u.z, kr * dp.w - cs * u.w));
  st4(contrib + (2 * (int64_t)B + b) * ldc + c, make_float4(cs * u.x, cs * u.y, cs * u.z, cs * u.w));
  st4(dout_u + (int64_t)b * D + c, make_float4(-kr * du.x, -kr * du.y, -kr * du.z, -kr * du.w));
  st4(dout_i + (int64_t)b * D + c, make_float4(-kr * dp.x, -kr * dp.y, -kr * dp.z, -kr * dp.w));
}

// loss[0] = sum(loss_b) inv_norm, loss[1] = (1 - alpha) reg_weight mean(w), loss[2] = loss[1] inv_norm: fixed-order
// fp64 tree
__global__ void __launch_bounds__(1024) ddrm_loss_reduce_kernel(int B, const float* __restrict__ terms, float alpha,
                                                                float reg_weight, float inv_norm,
                                                                float* __restrict__ loss) {
  __shared__ double s[2][1024];
  const int t = threadIdx.x;
  double a0 = 0.0, a1 = 0.0;
  for (int b = t; b < B; b += 1024) a0 += (double)terms[3 * (int64_t)B + b], a1 += (double)terms[b];
  s[0][t] = a0, s[1][t] = a1;
  __syncthreads();
  for (int off = 512; off > 0; off >>= 1) {
    if (t < off) s[0][t] += s[0][t + off], s[1][t] += s[1][t + off];
    __syncthreads();
  }
  if (t == 0) {
    loss[0] = (float)(s[0][0] * (double)inv_norm);
    const float coef = (float)((double)(1.f - alpha) * (double)reg_weight * (s[1][0] * (double)inv_norm));
    loss[1] = coef;
    loss[2] = coef * inv_norm;  // d loss / d |E0 row|^2 x 2: reg = sum |row|^2 inv_norm / 2
  }
}

// dst[b] += sqrt_ac[t_b] (keep ? 2 : 0) dxd[b] + dcond[b]: the q_sample input (through the dropout) and the other
// model's cond columns
__global__ void __launch_bounds__(256) ddrm_input_bwd_kernel(int64_t N, const float* __restrict__ dxd,
                                                             const uint8_t* __restrict__ keep, int64_t ldk,
                                                             const int32_t* __restrict__ t,
                                                             const float* __restrict__ sqrt_ac,
                                                             const float* __restrict__ dcond, float* __restrict__ dst,
                                                             int64_t ldd) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * D) return;
  const int64_t row = i >> 6;
  const int c = (int)(i & 63);
  float g = sqrt_ac[t[row]] * dxd[i];
  if (keep) g = keep[row * ldk + c] ? g * 2.f : 0.f;
  dst[row * ldd + c] = (dst[row * ldd + c] + g) + dcond[i];
}

}  // namespace

// ==================================================================================================== C ABI
extern "C" int32_t gmr_ddrm_tile_rows(void) { return TR; }

static bool ddrm_h_ok(int32_t H) { return H >= 4 && H <= 1024 && H % 4 == 0; }
static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int gmr_ddrm_denoise_fwd(int64_t N, int32_t H, int32_t T, int64_t row_off, const float* X, int64_t ldx,
                                    const int32_t* idx_x, const float* C, int64_t ldc, const int32_t* idx_c,
                                    const int32_t* t, const float* sqrt_ac, const float* sqrt_1mac, const float* noise,
                                    int64_t ldn, int32_t drop_mode, const uint8_t* keep, int64_t ldk, uint64_t seed,
                                    uint64_t step, uint64_t site, const float* W1, const float* TB, const float* W2,
                                    const float* b2, float* out, int64_t ldo, float* xd, int64_t ldxd,
                                    uint8_t* keep_out, int64_t ldko, float* h, int64_t ldh, float* rowmse,
                                    void* stream) {
  GMR_ARG(ddrm_h_ok(H), "hidden width: a multiple of 4 in 4..1024");
  GMR_ARG(N >= 1 && N <= ((int64_t)1 << 31) * TR - TR && T >= 1 && row_off >= 0, "bad sizes");
  GMR_ARG(X && C && t && sqrt_ac && sqrt_1mac && W1 && TB && W2 && b2 && out, "null pointer");
  GMR_ARG(ldx >= D && ldc >= D && ldo >= D && (!noise || ldn >= D) && (!xd || ldxd >= D) && (!h || ldh >= H),
          "bad strides");
  GMR_ARG(drop_mode >= 0 && drop_mode <= 2 && (drop_mode != 1 || (keep && ldk >= D)) && (!keep_out || ldko >= D),
          "bad dropout arguments");
  GMR_ARG(al16(W1) && al16(W2), "weights must be 16-byte aligned");
  FwdArgs a{N, row_off, H, T, X, ldx, idx_x, C, ldc, idx_c, t, sqrt_ac, sqrt_1mac, noise, ldn, drop_mode, keep, ldk,
            seed, step, site, W1, TB, W2, b2, out, ldo, xd, ldxd, keep_out, ldko, h, ldh, rowmse};
  hipLaunchKernelGGL(ddrm_fwd_kernel, dim3((unsigned)((N + TR - 1) / TR)), dim3(256), 0, (hipStream_t)stream, a);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_ddrm_chain(int64_t N, int32_t H, int32_t T, int32_t S, int64_t row_off, const float* xs,
                              int64_t ldx, const float* noise0, int64_t ldn0, float qa, float qb, const float* C,
                              int64_t ldc, const int32_t* idx_c, const float* W1, const float* TB, const float* W2,
                              const float* b2, const float* c1, const float* c2, const float* sigma,
                              const float* step_noise, uint64_t seed, uint64_t step, uint64_t site, float* out,
                              int64_t ldo, void* stream) {
  GMR_ARG(ddrm_h_ok(H), "hidden width: a multiple of 4 in 4..1024");
  GMR_ARG(N >= 1 && N <= ((int64_t)1 << 31) * TR - TR && T >= 1 && S >= 0 && S <= T && row_off >= 0, "bad sizes");
  GMR_ARG(xs && out && ldx >= D && ldo >= D && (!noise0 || ldn0 >= D), "bad pointers or strides");
  GMR_ARG(S == 0 || (C && ldc >= D && W1 && TB && W2 && b2 && c1 && c2), "a chain of S >= 1 steps needs the model");
  GMR_ARG(S == 0 || (al16(W1) && al16(W2)), "weights must be 16-byte aligned");
  ChainArgs a{N, row_off, H, S, T, xs, ldx, noise0, ldn0, qa, qb, C, ldc, idx_c, W1, TB, W2, b2, c1, c2, sigma,
              step_noise, seed, step, site, out, ldo};
  hipLaunchKernelGGL(ddrm_chain_kernel, dim3((unsigned)((N + TR - 1) / TR)), dim3(256), 0, (hipStream_t)stream, a);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_ddrm_loss_fwd_bwd(int32_t B, int64_t n_users, const float* G, int64_t ldg, const int32_t* users,
                                     const int32_t* pos, const int32_t* neg, const float* out_u, int64_t ldou,
                                     const float* out_i, int64_t ldoi, const float* mse_u, const float* mse_i,
                                     const float* reg, float alpha, float beta, float reg_weight, float inv_norm,
                                     float* terms, float* loss, float* contrib, int64_t ldc, float* dout_u,
                                     float* dout_i, void* stream) {
  GMR_ARG(B >= 1 && n_users >= 0, "bad sizes");
  GMR_ARG(G && users && pos && neg && out_u && out_i && mse_u && mse_i && reg && terms && loss && contrib && dout_u &&
              dout_i,
          "null pointer");
  GMR_ARG(ldg >= D && ldou >= D && ldoi >= D && ldc >= D && ldg % 4 == 0 && ldou % 4 == 0 && ldoi % 4 == 0 &&
              ldc % 4 == 0 && al16(G) && al16(out_u) && al16(out_i) && al16(contrib) && al16(dout_u) && al16(dout_i),
          "rows must be 16-byte aligned");
  hipLaunchKernelGGL(ddrm_loss_rows_kernel, dim3(gmr::grid_for((int64_t)B * 16, 256)), dim3(256), 0,
                     (hipStream_t)stream, B, n_users, G, ldg, users, pos, neg, out_u, ldou, out_i, ldoi, mse_u, mse_i,
                     reg, alpha, beta, reg_weight, inv_norm, terms, contrib, ldc, dout_u, dout_i);
  GMR_LAUNCHED();
  hipLaunchKernelGGL(ddrm_loss_reduce_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, B, terms, alpha, reg_weight,
                     inv_norm, loss);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_ddrm_input_bwd(int64_t N, const float* dxd, const uint8_t* keep, int64_t ldk, const int32_t* t,
                                  const float* sqrt_ac, const float* dcond, float* dst, int64_t ldd, void* stream) {
  GMR_ARG(N >= 1 && dxd && t && sqrt_ac && dcond && dst && ldd >= D && (!keep || ldk >= D), "bad args");
  hipLaunchKernelGGL(ddrm_input_bwd_kernel, dim3(gmr::grid_for(N * D, 256)), dim3(256), 0, (hipStream_t)stream, N, dxd,
                     keep, ldk, t, sqrt_ac, dcond, dst, ldd);
  GMR_LAUNCHED();
  return GMR_OK;
}
