// Rectified-flow embedding generator (models/rf_modules.py of the reference: SimpleVelocityNet,
// RFEmbeddingGenerator) for hidden_dim 128 and (embedding_dim, condition_dim) = (64, 64 | 128 | 192), (128, 128) or
// (192, 192).  The entry points without a suffix are the embedding_dim 64 ones; the _w ones take the width DW as an
// argument (the concat-fusion backbones generate rows as wide as their conditions) and are the same kernels
// instantiated at DW: at DW = 64 both names reach the same code.
//
//   gmr_rf_sample                    the whole Euler integration of generate() in one launch: a workgroup owns
//                                    32 rows, activations stay in LDS, weights are read through L2, products on
//                                    v_mfma_f32_32x32x2_f32; the condition product in K chunks of at most 128 columns
//   gmr_rf_sample_mix                the same launch with the evaluation's mix as its epilogue: the final store of a
//                                    tile writes base + ratio z (ratio a device scalar) instead of z
//   gmr_rf_act_fwd / gmr_rf_act_bwd  [LayerNorm] + SiLU [+ dropout mask] [+ residual] rows of the training step,
//                                    LN weight / bias gradients as fixed-order column reductions (no float atomics)
//   gmr_rf_time_embed, gmr_rf_interp, gmr_rf_head_fwd / _prior_fwd / _bwd, gmr_rf_losses
//   gmr_rf_infonce_sampled_fwd_bwd   sampled InfoNCE of the predicted end points against the detached targets
//   gmr_adamw_f32                    Adam with decoupled decay (torch.optim.AdamW)
//   gmr_rf_randn / gmr_rf_rand       Philox draws keyed on (seed, step, site)
//
// The packed parameters are the reference's velocity_net.named_parameters() order, every tensor dense and row-major
// (all sizes are multiples of 64 floats, so a gmr Slab holds exactly this layout).
#include "gemm_impl.h"

namespace {
using gmr::wave_sum;

constexpr int H = 128, D = 64, TR = 32, LDH = H + 4;
constexpr int MAX_DW = 192;  // widest generated row
constexpr int MAX_L = 4;
constexpr float LN_EPS = 1e-5f;

struct RfOff {
  int tw, tb, cw, cb, cg, cbe, iw, ib, ig, ibe;
  int blk[MAX_L][8];  // W1 b1 g1 be1 W2 b2 g2 be2
  int ow, ob, og, obe, pw, pb, total;
};

RfOff rf_offsets(int DW, int C, int L) {
  RfOff o{};
  int p = 0;
  auto take = [&](int n) { int at = p; p += n; return at; };
  o.tw = take(H * 64), o.tb = take(H);
  o.cw = take(H * C), o.cb = take(H), o.cg = take(H), o.cbe = take(H);
  o.iw = take(H * DW), o.ib = take(H), o.ig = take(H), o.ibe = take(H);
  for (int l = 0; l < L; ++l) {
    o.blk[l][0] = take(H * H), o.blk[l][1] = take(H), o.blk[l][2] = take(H), o.blk[l][3] = take(H);
    o.blk[l][4] = take(H * H), o.blk[l][5] = take(H), o.blk[l][6] = take(H), o.blk[l][7] = take(H);
  }
  o.ow = take(H * H), o.ob = take(H), o.og = take(H), o.obe = take(H);
  o.pw = take(DW * H), o.pb = take(DW);
  o.total = p;
  return o;
}

// the (embedding_dim, condition_dim) pairs the kernels are instantiated for
bool rf_widths_ok(int DW, int C) {
  return (DW == 64 && (C == 64 || C == 128 || C == 192)) || (DW == 128 && C == 128) || (DW == 192 && C == 192);
}

__device__ __forceinline__ float silu(float x) { return x / (1.f + expf(-x)); }

// ------------------------------------------------------------------------------------------------ fused sampler
// acc (32 rows x 32 columns col0..) += src[32][K] (LDS, row stride ld) . W[col][K]^T (global, k contiguous).  Lane l
// feeds row / column l & 31 and the k half l >> 5: step s of the half multiplies k = (K / 2) (l >> 5) + s, so both
// operands are float4 reads; every row's sum has one fixed order, whatever tile the row falls in.
// tile_mm_ld: the same over the K columns of a wider weight that start at W (row stride ldw >= K floats, ldw % 4 == 0),
// one K chunk of a product whose operand does not fit the LDS tile at once.
template <int K>
__device__ __forceinline__ void tile_mm_ld(const float* __restrict__ src, int ld, const float* __restrict__ W, int ldw,
                                           int col0, floatx16& acc) {
  const int lane = threadIdx.x & 63, h = lane >> 5, r = lane & 31;
  const float* wp = W + (size_t)(col0 + r) * ldw + h * (K / 2);
  const float* sp = src + r * ld + h * (K / 2);
#pragma unroll 4
  for (int s = 0; s < K / 2; s += 4) {
    const float4 a = *reinterpret_cast<const float4*>(sp + s);
    const float4 b = *reinterpret_cast<const float4*>(wp + s);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
  }
}

template <int K>
__device__ __forceinline__ void tile_mm(const float* __restrict__ src, int ld, const float* __restrict__ W, int col0,
                                        floatx16& acc) {
  tile_mm_ld<K>(src, ld, W, K, col0, acc);
}

__device__ __forceinline__ floatx16 zero16() {
  floatx16 z;
#pragma unroll
  for (int e = 0; e < 16; ++e) z[e] = 0.f;
  return z;
}

// acc element e of lane l: row (e & 3) + 8 (e >> 2) + 4 (l >> 5), column col0 + (l & 31)
__device__ __forceinline__ void tile_store(float* dst, int col0, const floatx16& acc, const float* __restrict__ bias) {
  const int lane = threadIdx.x & 63, h = lane >> 5, c = col0 + (lane & 31);
  const float b = bias[c];
#pragma unroll
  for (int e = 0; e < 16; ++e) dst[((e & 3) + 8 * (e >> 2) + 4 * h) * LDH + c] = acc[e] + b;
}

// out = silu(LN(buf) [+ res]) [+ addv[c] + addm]; wave w takes rows 8w .. 8w + 7, a lane columns l and l + 64.
// Ends with a barrier.
__device__ __forceinline__ void tile_ln_silu(const float* buf, const float* __restrict__ g, const float* __restrict__ b,
                                             const float* res, const float* addv, const float* addm, float* out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float g0 = g[lane], g1 = g[lane + 64], b0 = b[lane], b1 = b[lane + 64];
#pragma unroll 2
  for (int i = 0; i < TR / 4; ++i) {
    const int o = (w * (TR / 4) + i) * LDH + lane;
    const float x0 = buf[o], x1 = buf[o + 64];
    const float mean = wave_sum(x0 + x1) * (1.f / H);
    const float d0 = x0 - mean, d1 = x1 - mean;
    const float rstd = 1.f / sqrtf(wave_sum(d0 * d0 + d1 * d1) * (1.f / H) + LN_EPS);
    float y0 = d0 * rstd * g0 + b0, y1 = d1 * rstd * g1 + b1;
    if (res) y0 += res[o], y1 += res[o + 64];
    y0 = silu(y0), y1 = silu(y1);
    if (addv) {
      y0 = y0 + addv[lane] + addm[o];
      y1 = y1 + addv[lane + 64] + addm[o + 64];
    }
    out[o] = y0, out[o + 64] = y1;
  }
  __syncthreads();
}

// One K chunk of the condition encoder: columns [K0, K0 + CK) of the tile's condition rows into sT (tail rows: zeros,
// never stored), then acc += sT . W[:, K0 .. K0 + CK)^T with W at row stride C.  Before a later chunk is staged, a
// barrier: every wave has read the one before.  The barrier after staging also covers the z0 tile on the first call.
template <int K0, int CK, int C>
__device__ __forceinline__ void cond_chunk(int64_t N, int64_t r0, const float* __restrict__ cond, int64_t ldc,
                                           float* sT, const float* __restrict__ W, floatx16& acc) {
  static_assert(CK <= H && CK % 8 == 0 && K0 % 4 == 0 && K0 + CK <= C, "a chunk fits the LDS tile; float4 reads");
  const int tid = threadIdx.x;
  if (K0 > 0) __syncthreads();
  for (int idx = tid; idx < TR * CK; idx += 256) {
    const int r = idx / CK, c = idx % CK;
    sT[r * LDH + c] = r0 + r < N ? cond[(r0 + r) * ldc + K0 + c] : 0.f;
  }
  __syncthreads();
  tile_mm_ld<CK>(sT, LDH, W + K0, C, (tid >> 6) * 32, acc);
}

// LDS of one workgroup at generated width DW: three 32 x 132 activation tiles, the 32 x (DW + 4) z tile (row stride
// mod 32 banks = 4 at every DW), the time embedding and its sinusoid: 58.75 KB at DW = 64 (static), 66.75 KB at 128 and
// 74.75 KB at 192 (dynamic: past the 64 KB static limit; two workgroups still fit the 160 KB of a CU)
constexpr int rf_sample_lds_floats(int DW) { return 3 * TR * LDH + TR * (DW + 4) + H + 64; }

// MIX: the evaluation's mix as the epilogue (base != nullptr at the entry); the plain instantiation reads none of
// base, ldb, ratio and is the code it was before the mix existed.  DW: the width of z0, out and base.
template <int DW, int C, bool MIX>
__global__ __launch_bounds__(256) void rf_sample_kernel(int64_t N, const float* __restrict__ z0, int64_t ldz,
                                                        const float* __restrict__ cond, int64_t ldc,
                                                        const float* __restrict__ P, RfOff o, int L, int n_steps,
                                                        double dt_d, float* __restrict__ out, int64_t ldo,
                                                        const float* __restrict__ base, int64_t ldb,
                                                        const float* __restrict__ ratio) {
  static_assert(DW % 64 == 0 && DW <= MAX_DW, "whole 32-column output tiles, float4 rows");
  constexpr int LDZ = DW + 4;
  float *sH, *sT, *sC, *sZ, *sE, *sS;
  if constexpr (DW == D) {
    __shared__ __attribute__((aligned(16))) float aH[TR * LDH];
    __shared__ __attribute__((aligned(16))) float aT[TR * LDH];
    __shared__ __attribute__((aligned(16))) float aC[TR * LDH];
    __shared__ __attribute__((aligned(16))) float aZ[TR * LDZ];
    __shared__ float aE[H], aS[64];
    sH = aH, sT = aT, sC = aC, sZ = aZ, sE = aE, sS = aS;
  } else {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    sH = lds, sT = sH + TR * LDH, sC = sT + TR * LDH, sZ = sC + TR * LDH, sE = sZ + TR * LDZ, sS = sE + H;
  }
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int64_t r0 = (int64_t)blockIdx.x * TR;
  for (int idx = tid; idx < TR * DW; idx += 256) {
    const int r = idx / DW, c = idx % DW;
    sZ[r * LDZ + c] = r0 + r < N ? z0[(r0 + r) * ldz + c] : 0.f;
  }
  // condition encoder, once per tile.  sT holds at most H condition columns, so the product runs in K chunks of
  // H (then the rest) into one accumulator: columns [0, 128) and [128, 192) at C = 192.  One chunk at C <= 128.
  floatx16 acc = zero16();
  constexpr int C0 = C < H ? C : H;
  cond_chunk<0, C0, C>(N, r0, cond, ldc, sT, P + o.cw, acc);
  if constexpr (C > H) cond_chunk<H, C - H, C>(N, r0, cond, ldc, sT, P + o.cw, acc);
  tile_store(sC, w * 32, acc, P + o.cb);
  __syncthreads();
  tile_ln_silu(sC, P + o.cg, P + o.cbe, nullptr, nullptr, nullptr, sC);
  const float dt = (float)dt_d;
  for (int step = 0; step < n_steps; ++step) {
    // time embedding of this step: one H-vector for all rows
    const float t = (float)((double)step * dt_d);
    if (tid < 32) {
      const float f = expf((float)tid * -(logf(10000.f) / 31.f));
      sS[tid] = sinf(t * f), sS[tid + 32] = cosf(t * f);
    }
    __syncthreads();
    if (tid < H) {
      const float* wr = P + o.tw + tid * 64;
      float s = 0.f;
      for (int k = 0; k < 64; ++k) s = fmaf(wr[k], sS[k], s);
      sE[tid] = silu(s + P[o.tb + tid]);
    }
    // input projection; h = input + time + condition
    acc = zero16();
    tile_mm<DW>(sZ, LDZ, P + o.iw, w * 32, acc);
    tile_store(sT, w * 32, acc, P + o.ib);
    __syncthreads();
    tile_ln_silu(sT, P + o.ig, P + o.ibe, nullptr, sE, sC, sH);
    for (int l = 0; l < L; ++l) {
      const int* b = o.blk[l];
      acc = zero16();
      tile_mm<H>(sH, LDH, P + b[0], w * 32, acc);
      tile_store(sT, w * 32, acc, P + b[1]);
      __syncthreads();
      tile_ln_silu(sT, P + b[2], P + b[3], nullptr, nullptr, nullptr, sT);
      acc = zero16();
      tile_mm<H>(sT, LDH, P + b[4], w * 32, acc);
      __syncthreads();  // every wave has read sT before it is overwritten
      tile_store(sT, w * 32, acc, P + b[5]);
      __syncthreads();
      tile_ln_silu(sT, P + b[6], P + b[7], sH, nullptr, nullptr, sH);
    }
    acc = zero16();
    tile_mm<H>(sH, LDH, P + o.ow, w * 32, acc);
    tile_store(sT, w * 32, acc, P + o.ob);
    __syncthreads();
    tile_ln_silu(sT, P + o.og, P + o.obe, nullptr, nullptr, nullptr, sT);
    // DW output columns in DW / 32 column tiles, tile ct on wave ct & 3 (waves 0, 1 alone at DW = 64): z += v dt.
    // sZ is written here and read by the next step's input projection, behind the barrier that ends the step
    for (int ct = w; ct < DW / 32; ct += 4) {
      acc = zero16();
      tile_mm<H>(sT, LDH, P + o.pw, ct * 32, acc);
      const int hh = lane >> 5, c = ct * 32 + (lane & 31);
      const float pb = P[o.pb + c];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int r = (e & 3) + 8 * (e >> 2) + 4 * hh;
        const float v = acc[e] + pb;
        sZ[r * LDZ + c] = sZ[r * LDZ + c] + v * dt;
      }
    }
    __syncthreads();
  }
  if constexpr (!MIX) {  // plain: the integrated rows
    for (int idx = tid; idx < TR * DW; idx += 256) {
      const int r = idx / DW, c = idx % DW;
      if (r0 + r < N) out[(r0 + r) * ldo + c] = sZ[r * LDZ + c];
    }
  } else {
    // the mix as the epilogue: out = base + ratio z, one fused multiply-add per element; z itself is not written.
    // DW / 4 lanes hold a row as one float4 each (sZ's rows are 16-byte aligned: LDZ % 4 == 0)
    const float rt = ratio[0];
    for (int idx = tid; idx < TR * (DW / 4); idx += 256) {
      const int r = idx / (DW / 4), c = (idx % (DW / 4)) * 4;
      if (r0 + r < N) {
        const float4 z = *reinterpret_cast<const float4*>(sZ + r * LDZ + c);
        const float4 b = *reinterpret_cast<const float4*>(base + (r0 + r) * ldb + c);
        *reinterpret_cast<float4*>(out + (r0 + r) * ldo + c) =
            make_float4(fmaf(rt, z.x, b.x), fmaf(rt, z.y, b.y), fmaf(rt, z.z, b.z), fmaf(rt, z.w, b.w));
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ row kernels
// out = drop(silu(LN(y) [+ res])) [+ add1] [+ add2] over N x 128 contiguous rows; g == NULL: no LayerNorm
__global__ __launch_bounds__(256) void rf_act_fwd_kernel(int64_t N, const float* __restrict__ y,
                                                         const float* __restrict__ g, const float* __restrict__ b,
                                                         const float* __restrict__ res,
                                                         const uint8_t* __restrict__ mask, float scale,
                                                         const float* __restrict__ add1,
                                                         const float* __restrict__ add2, float* __restrict__ out) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const int lane = threadIdx.x & 63;
  const int64_t o = row * H + lane;
  float x0 = y[o], x1 = y[o + 64];
  if (g) {
    const float mean = wave_sum(x0 + x1) * (1.f / H);
    const float d0 = x0 - mean, d1 = x1 - mean;
    const float rstd = 1.f / sqrtf(wave_sum(d0 * d0 + d1 * d1) * (1.f / H) + LN_EPS);
    x0 = d0 * rstd * g[lane] + b[lane], x1 = d1 * rstd * g[lane + 64] + b[lane + 64];
  }
  if (res) x0 += res[o], x1 += res[o + 64];
  x0 = silu(x0), x1 = silu(x1);
  if (mask) x0 = mask[o] ? x0 * scale : 0.f, x1 = mask[o + 64] ? x1 * scale : 0.f;
  if (add1) x0 = x0 + add1[o], x1 = x1 + add1[o + 64];
  if (add2) x0 = x0 + add2[o], x1 = x1 + add2[o + 64];
  out[o] = x0, out[o + 64] = x1;
}

constexpr int BWD_ROWS = 64;  // rows per block of the backward: 4 waves x 16 rows

// dy = d loss / d y from dout = d loss / d out; dres = the gradient of the pre-activation (the residual input's
// share); parts[block][2][128]: this block's sums of dpre * xhat and dpre
__global__ __launch_bounds__(256) void rf_act_bwd_kernel(int64_t N, const float* __restrict__ y,
                                                         const float* __restrict__ g, const float* __restrict__ b,
                                                         const float* __restrict__ res,
                                                         const uint8_t* __restrict__ mask, float scale,
                                                         const float* __restrict__ dout, float* __restrict__ dy,
                                                         float* __restrict__ dres, float* __restrict__ parts) {
  __shared__ float red[4][2][H];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float ag[2] = {0.f, 0.f}, ab[2] = {0.f, 0.f};
  float gv[2] = {1.f, 1.f}, bv[2] = {0.f, 0.f};
  if (g) gv[0] = g[lane], gv[1] = g[lane + 64], bv[0] = b[lane], bv[1] = b[lane + 64];
  for (int i = 0; i < BWD_ROWS / 4; ++i) {
    const int64_t row = (int64_t)blockIdx.x * BWD_ROWS + w * (BWD_ROWS / 4) + i;
    if (row >= N) break;  // wave-uniform
    const int64_t o = row * H + lane;
    float xh[2] = {y[o], y[o + 64]}, pre[2], rstd = 1.f;
    if (g) {
      const float mean = wave_sum(xh[0] + xh[1]) * (1.f / H);
      xh[0] -= mean, xh[1] -= mean;
      rstd = 1.f / sqrtf(wave_sum(xh[0] * xh[0] + xh[1] * xh[1]) * (1.f / H) + LN_EPS);
      xh[0] *= rstd, xh[1] *= rstd;
    }
    float dp[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      pre[j] = g ? xh[j] * gv[j] + bv[j] : xh[j];
      if (res) pre[j] += res[o + 64 * j];
      float da = dout[o + 64 * j];
      if (mask) da = mask[o + 64 * j] ? da * scale : 0.f;
      const float s = 1.f / (1.f + expf(-pre[j]));
      dp[j] = da * (s * (1.f + pre[j] * (1.f - s)));
      if (dres) dres[o + 64 * j] = dp[j];
    }
    if (g) {
      ag[0] += dp[0] * xh[0], ag[1] += dp[1] * xh[1], ab[0] += dp[0], ab[1] += dp[1];
      const float q0 = dp[0] * gv[0], q1 = dp[1] * gv[1];
      const float m1 = wave_sum(q0 + q1) * (1.f / H);
      const float m2 = wave_sum(q0 * xh[0] + q1 * xh[1]) * (1.f / H);
      dy[o] = rstd * (q0 - m1 - xh[0] * m2);
      dy[o + 64] = rstd * (q1 - m1 - xh[1] * m2);
    } else {
      dy[o] = dp[0], dy[o + 64] = dp[1];
    }
  }
  if (!g) return;
  red[w][0][lane] = ag[0], red[w][0][lane + 64] = ag[1], red[w][1][lane] = ab[0], red[w][1][lane + 64] = ab[1];
  __syncthreads();
  const int which = threadIdx.x >> 7, c = threadIdx.x & 127;
  parts[(int64_t)blockIdx.x * 256 + threadIdx.x] =
      ((red[0][which][c] + red[1][which][c]) + red[2][which][c]) + red[3][which][c];
}

// column sums of the per-block partials in one fixed order: thread (part, j) adds the blocks part, part + 4, ...
// of column j into four interleaved accumulators (independent loads in flight), the four parts are added in order
__global__ __launch_bounds__(1024) void rf_parts_reduce_kernel(int nblk, const float* __restrict__ parts,
                                                               float* __restrict__ dg, float* __restrict__ db) {
  __shared__ float red[4][256];
  const int j = threadIdx.x & 255, part = threadIdx.x >> 8;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int i = part;
  for (; i + 12 < nblk; i += 16) {
    a0 += parts[(int64_t)i * 256 + j];
    a1 += parts[(int64_t)(i + 4) * 256 + j];
    a2 += parts[(int64_t)(i + 8) * 256 + j];
    a3 += parts[(int64_t)(i + 12) * 256 + j];
  }
  for (; i < nblk; i += 4) a0 += parts[(int64_t)i * 256 + j];
  red[part][j] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (part != 0) return;
  const float s = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
  if (j < H) dg[j] = s;
  else db[j - H] = s;
}

__global__ void rf_time_embed_kernel(int64_t N, const float* __restrict__ t, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * 32) return;
  const int64_t row = i >> 5;
  const int k = (int)(i & 31);
  const float a = t[row] * expf((float)k * -(logf(10000.f) / 31.f));
  out[row * 64 + k] = sinf(a), out[row * 64 + 32 + k] = cosf(a);
}

// the row kernels below take the generated width DW as a template argument; DW = 64 is the code behind the entry
// points without a suffix
template <int DW>
__global__ void rf_interp_kernel(int64_t N, const float* __restrict__ X1, int64_t ld1, const float* __restrict__ X0,
                                 const float* __restrict__ t, float* __restrict__ Xt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * DW) return;
  const int64_t row = i / DW;
  const int c = (int)(i % DW);
  const float tt = t[row];
  Xt[i] = tt * X1[row * ld1 + c] + (1.f - tt) * X0[i];
}

// one wave per row, lane = column: v += (1 - t)^2 scale cos_grad(Xt, X1); squared error to parts; pred.  PRIOR: the
// user-prior term (1 - t)^2 pscale prior is added first, as the reference orders the two guidance terms.  The 64-wide
// head: the code behind gmr_rf_head_fwd / _prior_fwd, and behind the _w entries at DW = 64
template <bool PRIOR>
__global__ __launch_bounds__(256) void rf_head_fwd_kernel(int64_t N, float* __restrict__ V,
                                                          const float* __restrict__ Xt, const float* __restrict__ X1,
                                                          int64_t ld1, const float* __restrict__ X0,
                                                          const float* __restrict__ t,
                                                          const float* __restrict__ prior, int64_t ldp, float pscale,
                                                          float gscale, float* __restrict__ pred,
                                                          double* __restrict__ parts) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const int lane = threadIdx.x & 63;
  const int64_t o = row * D + lane;
  const float xt = Xt[o], x1 = X1[row * ld1 + lane], x0 = X0[o], tt = t[row];
  const float nt = sqrtf(wave_sum(xt * xt)), n1 = sqrtf(wave_sum(x1 * x1));
  const float dot = wave_sum(xt * x1);
  const float cs = dot / sqrtf(fmaxf((nt * nt) * (n1 * n1), 1e-16f));  // F.cosine_similarity, eps 1e-8
  const float ntc = fmaxf(nt, 1e-8f);
  const float grad = (x1 / fmaxf(n1, 1e-12f)) / ntc - (xt / fmaxf(nt, 1e-12f)) * cs / ntc;
  const float lam = (1.f - tt) * (1.f - tt);
  float v = V[o];
  if (PRIOR) v = v + lam * pscale * prior[row * ldp + lane];
  v = v + lam * gscale * grad;
  V[o] = v;
  const float e = v - (x1 - x0);
  const double sq = gmr::wave_sum_d((double)e * (double)e);
  if (lane == 0) parts[row] = sq;
  pred[o] = xt + (1.f - tt) * v;
}

// The head at DW = 128 or 192: one wave per row, a lane holds the DW / 64 columns lane + 64 j.  Norms and dots are wave
// sums over the whole row (a lane adds its columns in order first).  Every operation is rounded on its own (no
// contraction), so the result does not depend on how an instantiation is compiled: with an all-zero prior the PRIOR
// instantiation adds an exact zero and gives the plain one's bits.
template <int DW, bool PRIOR>
__global__ __launch_bounds__(256) void rf_head_fwd_w_kernel(int64_t N, float* __restrict__ V,
                                                            const float* __restrict__ Xt,
                                                            const float* __restrict__ X1, int64_t ld1,
                                                            const float* __restrict__ X0, const float* __restrict__ t,
                                                            const float* __restrict__ prior, int64_t ldp,
                                                            float pscale, float gscale, float* __restrict__ pred,
                                                            double* __restrict__ parts) {
#pragma clang fp contract(off)
  constexpr int NJ = DW / 64;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const int lane = threadIdx.x & 63;
  const int64_t o = row * DW + lane;
  const float tt = t[row];
  float xt[NJ], x1[NJ], x0[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) xt[j] = Xt[o + 64 * j], x1[j] = X1[row * ld1 + lane + 64 * j], x0[j] = X0[o + 64 * j];
  float st = xt[0] * xt[0], s1 = x1[0] * x1[0], sd = xt[0] * x1[0];
#pragma unroll
  for (int j = 1; j < NJ; ++j) st += xt[j] * xt[j], s1 += x1[j] * x1[j], sd += xt[j] * x1[j];
  const float nt = sqrtf(wave_sum(st)), n1 = sqrtf(wave_sum(s1));
  const float dot = wave_sum(sd);
  const float cs = dot / sqrtf(fmaxf((nt * nt) * (n1 * n1), 1e-16f));  // F.cosine_similarity, eps 1e-8
  const float ntc = fmaxf(nt, 1e-8f);
  const float lam = (1.f - tt) * (1.f - tt);
  double sq = 0.0;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const float grad = (x1[j] / fmaxf(n1, 1e-12f)) / ntc - (xt[j] / fmaxf(nt, 1e-12f)) * cs / ntc;
    float v = V[o + 64 * j];
    if (PRIOR) v = v + lam * pscale * prior[row * ldp + lane + 64 * j];
    v = v + lam * gscale * grad;
    V[o + 64 * j] = v;
    const float e = v - (x1[j] - x0[j]);
    sq = j == 0 ? (double)e * (double)e : sq + (double)e * (double)e;
    pred[o + 64 * j] = xt[j] + (1.f - tt) * v;
  }
  sq = gmr::wave_sum_d(sq);
  if (lane == 0) parts[row] = sq;
}

template <int DW>
__global__ void rf_head_bwd_kernel(int64_t N, const float* __restrict__ V, const float* __restrict__ X1, int64_t ld1,
                                   const float* __restrict__ X0, const float* __restrict__ t,
                                   const float* __restrict__ dpred, float inv, float* __restrict__ dV) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * DW) return;
  const int64_t row = i / DW;
  const int c = (int)(i % DW);
  const float vt = X1[row * ld1 + c] - X0[i];
  dV[i] = 2.f * (V[i] - vt) * inv + (1.f - t[row]) * dpred[i];
}

// [rf_loss, cl_loss, total]: fixed-order fp64 sums by one block; rf_loss is the mean over the N x DW entries
__global__ __launch_bounds__(256) void rf_losses_kernel(int64_t N, int DW, const double* __restrict__ rowparts,
                                                        int64_t B, const double* __restrict__ clparts, float weight,
                                                        float* __restrict__ out) {
  __shared__ double red[2][4];
  double a = 0.0, c = 0.0;
  for (int64_t i = threadIdx.x; i < N; i += 256) a += rowparts[i];
  for (int64_t i = threadIdx.x; i < 2 * B; i += 256) c += clparts[i];
  a = gmr::wave_sum_d(a), c = gmr::wave_sum_d(c);
  if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = a, red[1][threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float rf = (float)(((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) / (double)(N * DW));
    const float cl = B > 0 ? (float)(((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) / (double)B) : 0.f;
    out[0] = rf, out[1] = cl, out[2] = rf + weight * cl;
  }
}

// ------------------------------------------------------------------------------------------------ sampled InfoNCE
constexpr uint64_t SITE_MIX = 0x9E3779B97F4A7C15ull;

using gmr::mul4, gmr::dot4;
__device__ __forceinline__ float group16_sum(float v) {  // over the 16 lanes of a row group
#pragma unroll
  for (int m = 8; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ float4 across_groups(float4 v) {  // over the four 16-lane groups of a wave
  v = gmr::f4_add(v, gmr::shfl_xor_f4(v, 16));
  return gmr::f4_add(v, gmr::shfl_xor_f4(v, 32));
}

// one block per anchor.  16 lanes hold a DW-column row as NJ = DW / 64 float4 each (columns 4 (lane & 15) + 64 j), so a
// wave reads four negatives at a time (and draws four indices, not one index 64 times): slot s = 16 i + 4 w + q
// belongs to group q = lane >> 4 of wave w.  A lane adds its NJ chunks in order, group sums are butterflies, the four
// groups and then the four waves are added in order: one fixed order.
template <int NJ>
__global__ __launch_bounds__(256) void rf_infonce_kernel(int64_t n, const float* __restrict__ pred, int64_t ldp,
                                                         const float* __restrict__ T, int64_t ldt, int64_t row_off,
                                                         const int32_t* __restrict__ idx, int n_neg,
                                                         const int32_t* __restrict__ neg, uint64_t seed,
                                                         uint64_t step, uint64_t site, float inv_temp, float coef,
                                                         double* __restrict__ parts, float* __restrict__ contrib,
                                                         int64_t ldc) {
  __shared__ float4 rg[4][NJ][16], rq[4][NJ][16];
  __shared__ float rs[4];
  const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6, q = lane >> 4, c = (lane & 15) * 4;
  const int64_t p = idx[b];
  auto dotj = [](const float4* x, const float4* y) {  // a lane's share of a row dot product
    float d = dot4(x[0], y[0]);
#pragma unroll
    for (int j = 1; j < NJ; ++j) d += dot4(x[j], y[j]);
    return d;
  };
  float4 a[NJ], an[NJ], tp[NJ], tpn[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    a[j] = *reinterpret_cast<const float4*>(pred + (row_off + p) * ldp + c + 64 * j);
    tp[j] = *reinterpret_cast<const float4*>(T + (row_off + p) * ldt + c + 64 * j);
  }
  const float na = fmaxf(sqrtf(group16_sum(dotj(a, a))), 1e-12f);
  const float ntp = fmaxf(sqrtf(group16_sum(dotj(tp, tp))), 1e-12f);
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    an[j] = make_float4(a[j].x / na, a[j].y / na, a[j].z / na, a[j].w / na);
    tpn[j] = make_float4(tp[j].x / ntp, tp[j].y / ntp, tp[j].z / ntp, tp[j].w / ntp);
  }
  const float pos = expf(group16_sum(dotj(an, tpn)) * inv_temp);
  auto row_of = [&](int s) -> const float* {
    int64_t j;
    if (neg) {
      j = neg[(int64_t)b * n_neg + s];
    } else {
      const uint64_t k = (uint64_t)b * (uint64_t)n_neg + (uint64_t)s;
      const uint4 r = gmr::Philox::gen(seed + site * SITE_MIX, step, k >> 2);
      const uint32_t x = (k & 3) == 0 ? r.x : (k & 3) == 1 ? r.y : (k & 3) == 2 ? r.z : r.w;
      j = (int64_t)(((uint64_t)x * (uint64_t)n) >> 32);
    }
    if (j == p) j = (j + 1) % n;  // a negative equal to the positive: the next row
    return T + (row_off + j) * ldt + c;
  };
  // the reference normalises the gathered negatives (B, n_neg, DW) over dim 1, the n_neg axis (:762): column c of
  // every negative of this anchor is divided by the norm of that column over the anchor's negatives
  float4 sq[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) sq[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  const int iters = (n_neg + 15) / 16;
  for (int i = 0; i < iters; ++i) {
    const int s = 16 * i + 4 * w + q;
    if (s < n_neg) {
      const float* tr = row_of(s);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const float4 tv = *reinterpret_cast<const float4*>(tr + 64 * j);
        sq[j] = gmr::f4_add(sq[j], mul4(tv, tv));
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    sq[j] = across_groups(sq[j]);
    if (lane < 16) rq[w][j][lane] = sq[j];
  }
  __syncthreads();
  float4 icn[NJ], gv[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const float4 cn = gmr::f4_add(
        gmr::f4_add(gmr::f4_add(rq[0][j][lane & 15], rq[1][j][lane & 15]), rq[2][j][lane & 15]), rq[3][j][lane & 15]);
    icn[j] = make_float4(1.f / fmaxf(sqrtf(cn.x), 1e-12f), 1.f / fmaxf(sqrtf(cn.y), 1e-12f),
                         1.f / fmaxf(sqrtf(cn.z), 1e-12f), 1.f / fmaxf(sqrtf(cn.w), 1e-12f));
    gv[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float se = 0.f;
  // every lane takes every iteration: the group sums are wave-wide shuffles
  for (int i = 0; i < iters; ++i) {
    const int s = 16 * i + 4 * w + q;
    const bool valid = s < n_neg;
    float4 tn[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) tn[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (valid) {
      const float* tr = row_of(s);
#pragma unroll
      for (int j = 0; j < NJ; ++j) tn[j] = mul4(*reinterpret_cast<const float4*>(tr + 64 * j), icn[j]);
    }
    const float d = group16_sum(dotj(an, tn));
    const float e = valid ? expf(d * inv_temp) : 0.f;
    se += e;
#pragma unroll
    for (int j = 0; j < NJ; ++j) gv[j] = gmr::f4_fma(e, tn[j], gv[j]);
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    gv[j] = across_groups(gv[j]);
    if (lane < 16) rg[w][j][lane] = gv[j];
  }
  se += __shfl_xor(se, 16);
  se += __shfl_xor(se, 32);
  if (lane == 0) rs[w] = se;
  __syncthreads();
  if (w != 0) return;
  // -log(pos / ttl) as log1p(sum / pos) and pos / ttl - 1 as -sum / ttl: with few or far negatives the sum is small
  // against pos, and pos / ttl rounded next to 1 keeps only four digits of a loss of 1e-3 (and of k1)
  const float nsum = ((rs[0] + rs[1]) + rs[2]) + rs[3];
  const float ttl = pos + nsum;
  if (lane == 0) parts[b] = (double)log1pf(nsum / pos);
  // d loss / d an = ((pos / ttl - 1) tp + sum_s (e_s / ttl) t_s) / temp, then through the normalisation
  const float k1 = -nsum / ttl, k2 = 1.f / ttl;
  float4 gn[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const float4 gs = gmr::f4_add(
        gmr::f4_add(gmr::f4_add(rg[0][j][lane & 15], rg[1][j][lane & 15]), rg[2][j][lane & 15]), rg[3][j][lane & 15]);
    gn[j] = make_float4((k1 * tpn[j].x + gs.x * k2) * inv_temp, (k1 * tpn[j].y + gs.y * k2) * inv_temp,
                        (k1 * tpn[j].z + gs.z * k2) * inv_temp, (k1 * tpn[j].w + gs.w * k2) * inv_temp);
  }
  const float proj = group16_sum(dotj(an, gn));
  const float sc = coef / na;
  if (lane < 16) {
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      *reinterpret_cast<float4*>(contrib + (int64_t)b * ldc + c + 64 * j) =
          make_float4(sc * (gn[j].x - an[j].x * proj), sc * (gn[j].y - an[j].y * proj),
                      sc * (gn[j].z - an[j].z * proj), sc * (gn[j].w - an[j].w * proj));
  }
}

// ------------------------------------------------------------------------------------------------ optimiser, draws
__global__ void adamw_kernel(int64_t n, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                             float* __restrict__ v, float b1, float b2, float eps, float decay, float step_size,
                             float bc2_sqrt) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float gi = g[i];
  const float pi = p[i] * decay;  // decoupled decay first: p <- p (1 - lr wd)
  const float mi = m[i] + (1.f - b1) * (gi - m[i]);
  const float vi = v[i] * b2 + (1.f - b2) * gi * gi;
  m[i] = mi, v[i] = vi;
  p[i] = pi - step_size * (mi / (sqrtf(vi) / bc2_sqrt + eps));
}

__global__ void rf_randn_kernel(int64_t n, uint64_t seed, uint64_t step, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // four values per thread
  if (4 * i >= n) return;
  const uint4 r = gmr::Philox::gen(seed, step, (uint64_t)i);
  const float2 a = gmr::box_muller(r.x, r.y), b = gmr::box_muller(r.z, r.w);
  const float v[4] = {a.x, a.y, b.x, b.y};
  for (int q = 0; q < 4 && 4 * i + q < n; ++q) out[4 * i + q] = v[q];
}

__global__ void rf_rand_kernel(int64_t n, uint64_t seed, uint64_t step, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (4 * i >= n) return;
  const uint4 r = gmr::Philox::gen(seed, step, (uint64_t)i);
  const uint32_t x[4] = {r.x, r.y, r.z, r.w};
  for (int q = 0; q < 4 && 4 * i + q < n; ++q) out[4 * i + q] = (float)(x[q] >> 8) * (1.0f / 16777216.0f);  // [0, 1)
}

}  // namespace

// ==================================================================================================== C ABI
extern "C" int32_t gmr_rf_tile_rows(void) { return TR; }

extern "C" int64_t gmr_rf_param_floats_w(int32_t DW, int32_t C, int32_t L) {
  if (!rf_widths_ok(DW, C) || L < 1 || L > MAX_L) return -1;
  return rf_offsets(DW, C, L).total;
}

extern "C" int64_t gmr_rf_param_floats(int32_t C, int32_t L) { return gmr_rf_param_floats_w(D, C, L); }

// the argument checks the sampler entries share, reported under the entry's own name; DW is the entry's width
#define RF_SAMPLE_ARGS()                                                                                   \
  GMR_ARG(hidden == H, "rf_hidden_dim must be 128");                                                       \
  GMR_ARG(rf_widths_ok(DW, C),                                                                             \
          "(embedding_dim, condition_dim) must be (64, 64 | 128 | 192), (128, 128) or (192, 192)");        \
  GMR_ARG(L >= 1 && L <= MAX_L, "rf_n_layers must be in 1..4");                                            \
  GMR_ARG(N >= 1 && N <= ((int64_t)1 << 31) * TR - TR && n_steps >= 1, "N >= 1 and n_steps >= 1");         \
  GMR_ARG(z0 && cond && params && out && ldz >= DW && ldc >= C && ldo >= DW, "bad pointers or strides");   \
  GMR_ARG(((uintptr_t)params & 15) == 0, "params must be 16-byte aligned")

#define RF_MIX_ARGS()                                                                                               \
  GMR_ARG(base != nullptr, "base must not be null");                                                                \
  GMR_ARG(ratio != nullptr, "ratio must not be null (a device scalar)");                                            \
  GMR_ARG(ldb >= DW && ldb % 4 == 0, "the row stride of base must be >= the row width and a multiple of 4");        \
  GMR_ARG(ldo >= DW && ldo % 4 == 0, "the row stride of out must be >= the row width and a multiple of 4");         \
  GMR_ARG(((uintptr_t)base & 15) == 0 && ((uintptr_t)out & 15) == 0, "base and out must be 16-byte aligned");       \
  GMR_ARG(base != out, "base must not alias out")

// one instantiation: the wide ones take their LDS as dynamic (past the 64 KB static limit), which the runtime grants
// per kernel and device on request; the request is a host call without a launch, made before every wide launch
template <int DW, int C, bool MIX>
static hipError_t rf_sample_one(dim3 grid, hipStream_t st, int64_t N, const float* z0, int64_t ldz, const float* cond,
                                int64_t ldc, const float* params, const RfOff& o, int L, int n_steps, double dt,
                                float* out, int64_t ldo, const float* base, int64_t ldb, const float* ratio) {
  int lds = 0;
  if (DW != D) {
    lds = rf_sample_lds_floats(DW) * (int)sizeof(float);
    const hipError_t e = hipFuncSetAttribute((const void*)rf_sample_kernel<DW, C, MIX>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((rf_sample_kernel<DW, C, MIX>), grid, dim3(256), lds, st, N, z0, ldz, cond, ldc, params, o, L,
                     n_steps, dt, out, ldo, base, ldb, ratio);
  return hipGetLastError();
}

// the plain (base == nullptr) and the mixed sampler of every width behind one launch
static int rf_sample_launch(int64_t N, int32_t DW, int32_t C, int32_t L, int32_t n_steps, const float* z0, int64_t ldz,
                            const float* cond, int64_t ldc, const float* params, float* out, int64_t ldo,
                            const float* base, int64_t ldb, const float* ratio, void* stream) {
  const RfOff o = rf_offsets(DW, C, L);
  const dim3 grid((unsigned)((N + TR - 1) / TR));
  const double dt = 1.0 / (double)n_steps;
  hipError_t e;
#define RF_SAMPLE_LAUNCH(DWW, CW, MIXED)                                                                          \
  e = rf_sample_one<DWW, CW, MIXED>(grid, (hipStream_t)stream, N, z0, ldz, cond, ldc, params, o, L, n_steps, dt, \
                                    out, ldo, base, ldb, ratio)
  if (base == nullptr) {
    if (DW == 128) RF_SAMPLE_LAUNCH(128, 128, false);
    else if (DW == 192) RF_SAMPLE_LAUNCH(192, 192, false);
    else if (C == 64) RF_SAMPLE_LAUNCH(64, 64, false);
    else if (C == 128) RF_SAMPLE_LAUNCH(64, 128, false);
    else RF_SAMPLE_LAUNCH(64, 192, false);
  } else {
    if (DW == 128) RF_SAMPLE_LAUNCH(128, 128, true);
    else if (DW == 192) RF_SAMPLE_LAUNCH(192, 192, true);
    else if (C == 64) RF_SAMPLE_LAUNCH(64, 64, true);
    else if (C == 128) RF_SAMPLE_LAUNCH(64, 128, true);
    else RF_SAMPLE_LAUNCH(64, 192, true);
  }
#undef RF_SAMPLE_LAUNCH
  if (e != hipSuccess) return gmr::hip_status(__func__, e);
  return GMR_OK;
}

extern "C" int gmr_rf_sample(int64_t N, int32_t hidden, int32_t C, int32_t L, int32_t n_steps, const float* z0,
                             int64_t ldz, const float* cond, int64_t ldc, const float* params, float* out, int64_t ldo,
                             void* stream) {
  constexpr int DW = D;
  RF_SAMPLE_ARGS();
  return rf_sample_launch(N, DW, C, L, n_steps, z0, ldz, cond, ldc, params, out, ldo, nullptr, 0, nullptr, stream);
}

extern "C" int gmr_rf_sample_w(int64_t N, int32_t hidden, int32_t DW, int32_t C, int32_t L, int32_t n_steps,
                               const float* z0, int64_t ldz, const float* cond, int64_t ldc, const float* params,
                               float* out, int64_t ldo, void* stream) {
  RF_SAMPLE_ARGS();
  return rf_sample_launch(N, DW, C, L, n_steps, z0, ldz, cond, ldc, params, out, ldo, nullptr, 0, nullptr, stream);
}

// out[r] = base[r] + ratio[0] * z[r] with z the rows gmr_rf_sample would write; base must not alias out (a tile's
// rows are read as they are written, but nothing orders two calls' views of one table)
extern "C" int gmr_rf_sample_mix(int64_t N, int32_t hidden, int32_t C, int32_t L, int32_t n_steps, const float* z0,
                                 int64_t ldz, const float* cond, int64_t ldc, const float* params, const float* base,
                                 int64_t ldb, const float* ratio, float* out, int64_t ldo, void* stream) {
  constexpr int DW = D;
  RF_SAMPLE_ARGS();
  RF_MIX_ARGS();
  return rf_sample_launch(N, DW, C, L, n_steps, z0, ldz, cond, ldc, params, out, ldo, base, ldb, ratio, stream);
}

extern "C" int gmr_rf_sample_mix_w(int64_t N, int32_t hidden, int32_t DW, int32_t C, int32_t L, int32_t n_steps,
                                   const float* z0, int64_t ldz, const float* cond, int64_t ldc, const float* params,
                                   const float* base, int64_t ldb, const float* ratio, float* out, int64_t ldo,
                                   void* stream) {
  RF_SAMPLE_ARGS();
  RF_MIX_ARGS();
  return rf_sample_launch(N, DW, C, L, n_steps, z0, ldz, cond, ldc, params, out, ldo, base, ldb, ratio, stream);
}

extern "C" int gmr_rf_act_fwd(int64_t N, const float* y, const float* ln_w, const float* ln_b, const float* res,
                              const uint8_t* mask, float keep_scale, const float* add1, const float* add2, float* out,
                              void* stream) {
  GMR_ARG(N >= 1 && y && out && (!ln_w == !ln_b), "bad args");
  hipLaunchKernelGGL(rf_act_fwd_kernel, dim3(gmr::grid_for(N, 4)), dim3(256), 0, (hipStream_t)stream, N, y, ln_w, ln_b,
                     res, mask, keep_scale, add1, add2, out);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int64_t gmr_rf_act_parts_floats(int64_t N) { return (N + BWD_ROWS - 1) / BWD_ROWS * 256; }

extern "C" int gmr_rf_act_bwd(int64_t N, const float* y, const float* ln_w, const float* ln_b, const float* res,
                              const uint8_t* mask, float keep_scale, const float* dout, float* dy, float* dres,
                              float* parts, float* d_ln_w, float* d_ln_b, void* stream) {
  GMR_ARG(N >= 1 && y && dout && dy && (!ln_w == !ln_b), "bad args");
  GMR_ARG(!ln_w || (parts && d_ln_w && d_ln_b), "LayerNorm gradients need parts, d_ln_w and d_ln_b");
  const int nblk = gmr::grid_for(N, BWD_ROWS);
  hipLaunchKernelGGL(rf_act_bwd_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, N, y, ln_w, ln_b, res, mask,
                     keep_scale, dout, dy, dres, parts);
  GMR_LAUNCHED();
  if (ln_w) {
    hipLaunchKernelGGL(rf_parts_reduce_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, nblk, parts, d_ln_w, d_ln_b);
    GMR_LAUNCHED();
  }
  return GMR_OK;
}

extern "C" int gmr_rf_time_embed(int64_t N, const float* t, float* out, void* stream) {
  GMR_ARG(N >= 1 && t && out, "bad args");
  hipLaunchKernelGGL(rf_time_embed_kernel, dim3(gmr::grid_for(N * 32, 256)), dim3(256), 0, (hipStream_t)stream, N, t,
                     out);
  GMR_LAUNCHED();
  return GMR_OK;
}

// the row entries of every width: DISPATCH_DW(launch) instantiates at the three widths
#define RF_DW_OK(DW) ((DW) == 64 || (DW) == 128 || (DW) == 192)
#define RF_DISPATCH_DW(DW, LAUNCH) \
  do {                             \
    if ((DW) == 64) {              \
      LAUNCH(64);                  \
    } else if ((DW) == 128) {      \
      LAUNCH(128);                 \
    } else {                       \
      LAUNCH(192);                 \
    }                              \
  } while (0)

extern "C" int gmr_rf_interp_w(int64_t N, int32_t DW, const float* X1, int64_t ld1, const float* X0, const float* t,
                               float* Xt, void* stream) {
  GMR_ARG(RF_DW_OK(DW), "the row width must be 64, 128 or 192");
  GMR_ARG(N >= 1 && X1 && X0 && t && Xt && ld1 >= DW, "bad args");
#define LAUNCH(W)                                                                                                      \
  hipLaunchKernelGGL(rf_interp_kernel<W>, dim3(gmr::grid_for(N * W, 256)), dim3(256), 0, (hipStream_t)stream, N, X1, \
                     ld1, X0, t, Xt)
  RF_DISPATCH_DW(DW, LAUNCH);
#undef LAUNCH
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_rf_interp(int64_t N, const float* X1, int64_t ld1, const float* X0, const float* t, float* Xt,
                             void* stream) {
  return gmr_rf_interp_w(N, D, X1, ld1, X0, t, Xt, stream);
}

extern "C" int gmr_rf_head_fwd_w(int64_t N, int32_t DW, float* V, const float* Xt, const float* X1, int64_t ld1,
                                 const float* X0, const float* t, float guidance_scale, float* pred, double* row_parts,
                                 void* stream) {
  GMR_ARG(RF_DW_OK(DW), "the row width must be 64, 128 or 192");
  GMR_ARG(N >= 1 && V && Xt && X1 && X0 && t && pred && row_parts && ld1 >= DW, "bad args");
#define LAUNCH(KERNEL)                                                                                           \
  hipLaunchKernelGGL((KERNEL), dim3(gmr::grid_for(N, 4)), dim3(256), 0, (hipStream_t)stream, N, V, Xt, X1, ld1, X0, t, \
                     (const float*)nullptr, (int64_t)0, 0.f, guidance_scale, pred, row_parts)
  if (DW == D) LAUNCH(rf_head_fwd_kernel<false>);
  else if (DW == 128) LAUNCH((rf_head_fwd_w_kernel<128, false>));
  else LAUNCH((rf_head_fwd_w_kernel<192, false>));
#undef LAUNCH
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_rf_head_fwd(int64_t N, float* V, const float* Xt, const float* X1, int64_t ld1, const float* X0,
                               const float* t, float guidance_scale, float* pred, double* row_parts, void* stream) {
  return gmr_rf_head_fwd_w(N, D, V, Xt, X1, ld1, X0, t, guidance_scale, pred, row_parts, stream);
}

extern "C" int gmr_rf_head_prior_fwd_w(int64_t N, int32_t DW, float* V, const float* Xt, const float* X1, int64_t ld1,
                                       const float* X0, const float* t, const float* prior, int64_t ldp,
                                       float prior_scale, float cos_scale, float* pred, double* row_parts,
                                       void* stream) {
  GMR_ARG(RF_DW_OK(DW), "the row width must be 64, 128 or 192");
  GMR_ARG(N >= 1 && V && Xt && X1 && X0 && t && pred && row_parts && ld1 >= DW, "bad args");
  GMR_ARG(prior && ldp >= DW, "prior must be a table as wide as the rows with a row stride >= that width");
#define LAUNCH(KERNEL)                                                                                           \
  hipLaunchKernelGGL((KERNEL), dim3(gmr::grid_for(N, 4)), dim3(256), 0, (hipStream_t)stream, N, V, Xt, X1, ld1, X0, t, \
                     prior, ldp, prior_scale, cos_scale, pred, row_parts)
  if (DW == D) LAUNCH(rf_head_fwd_kernel<true>);
  else if (DW == 128) LAUNCH((rf_head_fwd_w_kernel<128, true>));
  else LAUNCH((rf_head_fwd_w_kernel<192, true>));
#undef LAUNCH
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_rf_head_prior_fwd(int64_t N, float* V, const float* Xt, const float* X1, int64_t ld1,
                                     const float* X0, const float* t, const float* prior, int64_t ldp,
                                     float prior_scale, float cos_scale, float* pred, double* row_parts,
                                     void* stream) {
  return gmr_rf_head_prior_fwd_w(N, D, V, Xt, X1, ld1, X0, t, prior, ldp, prior_scale, cos_scale, pred, row_parts,
                                 stream);
}

extern "C" int gmr_rf_head_bwd_w(int64_t N, int32_t DW, const float* V, const float* X1, int64_t ld1, const float* X0,
                                 const float* t, const float* dpred, float* dV, void* stream) {
  GMR_ARG(RF_DW_OK(DW), "the row width must be 64, 128 or 192");
  GMR_ARG(N >= 1 && V && X1 && X0 && t && dpred && dV && ld1 >= DW, "bad args");
#define LAUNCH(W)                                                                                                      \
  hipLaunchKernelGGL(rf_head_bwd_kernel<W>, dim3(gmr::grid_for(N * W, 256)), dim3(256), 0, (hipStream_t)stream, N, V, \
                     X1, ld1, X0, t, dpred, (float)(1.0 / ((double)N * W)), dV)
  RF_DISPATCH_DW(DW, LAUNCH);
#undef LAUNCH
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_rf_head_bwd(int64_t N, const float* V, const float* X1, int64_t ld1, const float* X0, const float* t,
                               const float* dpred, float* dV, void* stream) {
  return gmr_rf_head_bwd_w(N, D, V, X1, ld1, X0, t, dpred, dV, stream);
}

extern "C" int gmr_rf_losses_w(int64_t N, int32_t DW, const double* row_parts, int64_t B, const double* cl_parts,
                               float weight, float* out3, void* stream) {
  GMR_ARG(RF_DW_OK(DW), "the row width must be 64, 128 or 192");
  GMR_ARG(N >= 1 && row_parts && B >= 0 && (B == 0 || cl_parts) && out3, "bad args");
  hipLaunchKernelGGL(rf_losses_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, N, (int)DW, row_parts, B, cl_parts,
                     weight, out3);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_rf_losses(int64_t N, const double* row_parts, int64_t B, const double* cl_parts, float weight,
                             float* out3, void* stream) {
  return gmr_rf_losses_w(N, D, row_parts, B, cl_parts, weight, out3, stream);
}

extern "C" int gmr_rf_infonce_sampled_fwd_bwd_w(int32_t B, int64_t n, int32_t DW, const float* pred, int64_t ldp,
                                                const float* target, int64_t ldt, int64_t row_off, const int32_t* idx,
                                                int32_t n_neg, const int32_t* neg, uint64_t seed, uint64_t step,
                                                uint64_t site, float inv_temp, float coef, double* parts,
                                                float* contrib, int64_t ldc, void* stream) {
  GMR_ARG(RF_DW_OK(DW), "the row width must be 64, 128 or 192");
  GMR_ARG(B >= 1 && n >= 1 && n < ((int64_t)1 << 31) && n_neg >= 0 && row_off >= 0, "bad sizes");
  GMR_ARG(pred && target && idx && parts && contrib && ldp >= DW && ldt >= DW && ldc >= DW, "bad pointers or strides");
  GMR_ARG((((uintptr_t)pred | (uintptr_t)target | (uintptr_t)contrib) & 15) == 0 && ldp % 4 == 0 && ldt % 4 == 0 &&
              ldc % 4 == 0,
          "rows must be 16-byte aligned");
#define LAUNCH(W)                                                                                                   \
  hipLaunchKernelGGL(rf_infonce_kernel<W / 64>, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, n, pred, ldp, \
                     target, ldt, row_off, idx, n_neg, neg, seed, step, site, inv_temp, coef, parts, contrib, ldc)
  RF_DISPATCH_DW(DW, LAUNCH);
#undef LAUNCH
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_rf_infonce_sampled_fwd_bwd(int32_t B, int64_t n, const float* pred, int64_t ldp, const float* target,
                                              int64_t ldt, int64_t row_off, const int32_t* idx, int32_t n_neg,
                                              const int32_t* neg, uint64_t seed, uint64_t step, uint64_t site,
                                              float inv_temp, float coef, double* parts, float* contrib, int64_t ldc,
                                              void* stream) {
  return gmr_rf_infonce_sampled_fwd_bwd_w(B, n, D, pred, ldp, target, ldt, row_off, idx, n_neg, neg, seed, step, site,
                                          inv_temp, coef, parts, contrib, ldc, stream);
}

extern "C" int gmr_adamw_f32(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float beta1,
                             float beta2, float eps, float decay_factor, float step_size, float bias_correction2_sqrt,
                             void* stream) {
  GMR_ARG(param && grad && exp_avg && exp_avg_sq && n >= 0, "bad args");
  if (n == 0) return GMR_OK;
  hipLaunchKernelGGL(adamw_kernel, dim3(gmr::grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, n, param, grad,
                     exp_avg, exp_avg_sq, beta1, beta2, eps, decay_factor, step_size, bias_correction2_sqrt);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_rf_randn(int64_t n, uint64_t seed, uint64_t step, uint64_t site, float* out, void* stream) {
  GMR_ARG(n >= 1 && out, "bad args");
  hipLaunchKernelGGL(rf_randn_kernel, dim3(gmr::grid_for((n + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream, n,
                     seed + site * SITE_MIX, step, out);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_rf_rand(int64_t n, uint64_t seed, uint64_t step, uint64_t site, float* out, void* stream) {
  GMR_ARG(n >= 1 && out, "bad args");
  hipLaunchKernelGGL(rf_rand_kernel, dim3(gmr::grid_for((n + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream, n,
                     seed + site * SITE_MIX, step, out);
  GMR_LAUNCHED();
  return GMR_OK;
}
