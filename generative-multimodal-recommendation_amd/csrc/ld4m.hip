// LD4MRec C-Net row kernels (gfx950): FiLM-modulated LayerNorm, exact GELU with inverted dropout, the
// smoothed-target MSE rows, the loss-history moving average and the importance draw of t.
//
// C-Net block (gmr/ld4mrec.py): n = LN(h) w + b;  z = n (1 + s) + sh;  h' = h + W2 drop(gelu(W1 z + b1)) + b2.
// The products run in gemm.hip; this file holds what sits between them.  Row kernels take one 64-lane wave
// per row and 16-byte loads: H is a multiple of 64 in 64..1024, so a lane owns up to four float4 of a row.
// Nothing here accumulates floating-point values with atomics: column sums go through per-block partials that
// a second kernel adds in block order, the history update walks the batch in order.
#include "gmr_common.h"

namespace {

constexpr int kRowsPerBlock = 8;  // film_bwd: rows per workgroup = one row of dw/db partials
constexpr int kMaxQ = 4;          // float4 per lane at H = 1024

using gmr::ld4, gmr::st4;
__device__ __forceinline__ float4 f4_mul(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float f4_hsum(float4 a) { return (a.x + a.y) + (a.z + a.w); }

// z = (LN(h) w + b) (1 + s) + sh; mean / rstd saved.  One wave per row, four rows per workgroup.
__global__ void __launch_bounds__(256) film_fwd_kernel(int64_t rows, int H, const float* __restrict__ h, int64_t ldh,
                                                       const float* __restrict__ w, const float* __restrict__ b,
                                                       const float* __restrict__ s, int64_t lds,
                                                       const float* __restrict__ sh, int64_t ldsh, float eps,
                                                       float* __restrict__ z, int64_t ldz, float* __restrict__ mean_out,
                                                       float* __restrict__ rstd_out) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int lane = threadIdx.x & 63;
  const int nq = H >> 2;
  float4 v[kMaxQ];
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < kMaxQ; ++j) {
    const int q = j * 64 + lane;
    v[j] = q < nq ? ld4(h + r * ldh + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
    sum += f4_hsum(v[j]);
  }
  const float mean = gmr::wave_sum(sum) / (float)H;
  float sq = 0.f;
#pragma unroll
  for (int j = 0; j < kMaxQ; ++j) {
    if (j * 64 + lane >= nq) continue;
    const float4 d = make_float4(v[j].x - mean, v[j].y - mean, v[j].z - mean, v[j].w - mean);
    sq += f4_hsum(f4_mul(d, d));
  }
  const float rstd = 1.f / sqrtf(gmr::wave_sum(sq) / (float)H + eps);
#pragma unroll
  for (int j = 0; j < kMaxQ; ++j) {
    const int q = j * 64 + lane;
    if (q >= nq) continue;
    const int c = 4 * q;
    const float4 ww = ld4(w + c), bb = ld4(b + c), ss = ld4(s + r * lds + c), hh = ld4(sh + r * ldsh + c);
    float4 o;
    o.x = ((v[j].x - mean) * rstd * ww.x + bb.x) * (1.f + ss.x) + hh.x;
    o.y = ((v[j].y - mean) * rstd * ww.y + bb.y) * (1.f + ss.y) + hh.y;
    o.z = ((v[j].z - mean) * rstd * ww.z + bb.z) * (1.f + ss.z) + hh.z;
    o.w = ((v[j].w - mean) * rstd * ww.w + bb.w) * (1.f + ss.w) + hh.w;
    st4(z + r * ldz + c, o);
  }
  if (lane == 0) {
    mean_out[r] = mean;
    rstd_out[r] = rstd;
  }
}

// From dz: ds = dz n, dsh = dz (skipped when it aliases dz), dn = dz (1 + s), dh (+)= LN backward of dn,
// dw / db column partials of the workgroup's rows -> part[blk][2 H] = [dw | db].
__global__ void __launch_bounds__(256) film_bwd_kernel(int64_t rows, int H, const float* __restrict__ h, int64_t ldh,
                                                       const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       const float* __restrict__ w, const float* __restrict__ b,
                                                       const float* __restrict__ s, int64_t lds, const float* dz,
                                                       int64_t lddz, float* __restrict__ ds, int64_t ldds, float* dsh,
                                                       int64_t lddsh, float* __restrict__ dh, int64_t lddh,
                                                       int accumulate, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float red[];  // [4][2 H]
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nq = H >> 2;
  float4 pw[kMaxQ], pb[kMaxQ];
#pragma unroll
  for (int j = 0; j < kMaxQ; ++j) pw[j] = pb[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  const int64_t r0 = (int64_t)blockIdx.x * kRowsPerBlock;
  for (int64_t r = r0 + wv; r < rows && r < r0 + kRowsPerBlock; r += 4) {
    const float mu = mean[r], rs = rstd[r];
    float4 xh[kMaxQ], g[kMaxQ];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < kMaxQ; ++j) {
      const int q = j * 64 + lane;
      xh[j] = g[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (q >= nq) continue;
      const int c = 4 * q;
      const float4 hv = ld4(h + r * ldh + c), ww = ld4(w + c), bb = ld4(b + c), ss = ld4(s + r * lds + c);
      const float4 d = ld4(dz + r * lddz + c);
      xh[j] = make_float4((hv.x - mu) * rs, (hv.y - mu) * rs, (hv.z - mu) * rs, (hv.w - mu) * rs);
      const float4 n = make_float4(xh[j].x * ww.x + bb.x, xh[j].y * ww.y + bb.y, xh[j].z * ww.z + bb.z,
                                   xh[j].w * ww.w + bb.w);
      st4(ds + r * ldds + c, f4_mul(d, n));
      if (dsh && dsh != dz) st4(dsh + r * lddsh + c, d);
      const float4 dn = make_float4(d.x * (1.f + ss.x), d.y * (1.f + ss.y), d.z * (1.f + ss.z), d.w * (1.f + ss.w));
      pw[j] = gmr::f4_add(pw[j], f4_mul(dn, xh[j]));
      pb[j] = gmr::f4_add(pb[j], dn);
      g[j] = f4_mul(dn, ww);
      s1 += f4_hsum(g[j]);
      s2 += f4_hsum(f4_mul(g[j], xh[j]));
    }
    s1 = gmr::wave_sum(s1) / (float)H;
    s2 = gmr::wave_sum(s2) / (float)H;
#pragma unroll
    for (int j = 0; j < kMaxQ; ++j) {
      const int q = j * 64 + lane;
      if (q >= nq) continue;
      const int c = 4 * q;
      float4 o = make_float4(rs * (g[j].x - s1 - xh[j].x * s2), rs * (g[j].y - s1 - xh[j].y * s2),
                             rs * (g[j].z - s1 - xh[j].z * s2), rs * (g[j].w - s1 - xh[j].w * s2));
      if (accumulate) o = gmr::f4_add(o, ld4(dh + r * lddh + c));
      st4(dh + r * lddh + c, o);
    }
  }
#pragma unroll
  for (int j = 0; j < kMaxQ; ++j) {
    const int q = j * 64 + lane;
    if (q >= nq) continue;
    st4(red + (size_t)wv * 2 * H + 4 * q, pw[j]);
    st4(red + (size_t)wv * 2 * H + H + 4 * q, pb[j]);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < 2 * H; c += 256)
    part[(int64_t)blockIdx.x * 2 * H + c] = (red[c] + red[2 * H + c]) + (red[4 * H + c] + red[6 * H + c]);
}

// column c of the P x 2H partials, added in block order (16 interleaved groups, then the groups in order)
__global__ void __launch_bounds__(1024) film_param_reduce_kernel(int P, int H, const float* __restrict__ part,
                                                                 float* __restrict__ dw, float* __restrict__ db,
                                                                 int accumulate) {
  __shared__ double red[16][64];
  const int cl = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  double s = 0.0;
  if (c < 2 * H)
    for (int p = g; p < P; p += 16) s += part[(int64_t)p * 2 * H + c];
  red[g][cl] = s;
  __syncthreads();
  if (g != 0 || c >= 2 * H) return;
  s = 0.0;
  for (int j = 0; j < 16; ++j) s += red[j][cl];
  float* o = c < H ? dw + c : db + (c - H);
  *o = (float)s + (accumulate ? *o : 0.f);
}

__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float dgelu_f(float x) {
  const float cdf = 0.5f * (1.f + erff(x * 0.70710678118654752f));
  const float pdf = 0.3989422804014327f * expf(-0.5f * x * x);
  return cdf + x * pdf;
}
__device__ __forceinline__ uint8_t keep_byte(uint64_t seed, uint64_t step, uint64_t ctr, float p_keep) {
  const uint4 q = gmr::Philox::gen(seed, step, ctr);  // gmr_keep_mask_u8's draw
  return (float)(q.x >> 8) * (1.0f / 16777216.0f) < p_keep ? 1 : 0;
}

// y = gelu(x) keep / p_keep.  mode 0: p_keep = 1 (no mask), 1: replay mask_in, 2: draw (and record to mask_out)
__global__ void __launch_bounds__(256) gelu_drop_fwd_kernel(int64_t rows, int H, const float* __restrict__ x,
                                                            int64_t ldx, float p_keep, int mode,
                                                            const uint8_t* __restrict__ mask_in,
                                                            uint8_t* __restrict__ mask_out, int64_t ldm, uint64_t seed,
                                                            uint64_t step, uint64_t ctr0, float* __restrict__ y,
                                                            int64_t ldy) {
  const int nq = H >> 2;
  const float scale = 1.f / p_keep;
  for (int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gi < rows * nq;
       gi += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = gi / nq;
    const int c = (int)(gi % nq) * 4;
    const float4 v = ld4(x + r * ldx + c);
    float o[4] = {gelu_f(v.x), gelu_f(v.y), gelu_f(v.z), gelu_f(v.w)};
    if (mode != 0) {
      uint8_t k[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        k[j] = mode == 1 ? (mask_in[r * ldm + c + j] != 0) : keep_byte(seed, step, ctr0 + (uint64_t)(r * H + c + j), p_keep);
      if (mode == 2 && mask_out) {
#pragma unroll
        for (int j = 0; j < 4; ++j) mask_out[r * ldm + c + j] = k[j];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = k[j] ? o[j] * scale : 0.f;
    }
    st4(y + r * ldy + c, make_float4(o[0], o[1], o[2], o[3]));
  }
}

// dx = dy keep / p_keep gelu'(x)   (mask NULL: p_keep = 1)
__global__ void __launch_bounds__(256) gelu_drop_bwd_kernel(int64_t rows, int H, const float* __restrict__ x,
                                                            int64_t ldx, const uint8_t* __restrict__ mask, int64_t ldm,
                                                            float p_keep, const float* dy, int64_t lddy, float* dx,
                                                            int64_t lddx) {
  const int nq = H >> 2;
  const float scale = 1.f / p_keep;
  for (int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gi < rows * nq;
       gi += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = gi / nq;
    const int c = (int)(gi % nq) * 4;
    const float4 v = ld4(x + r * ldx + c), d = ld4(dy + r * lddy + c);
    float o[4] = {d.x * dgelu_f(v.x), d.y * dgelu_f(v.y), d.z * dgelu_f(v.z), d.w * dgelu_f(v.w)};
    if (mask) {
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = mask[r * ldm + c + j] ? o[j] * scale : 0.f;
    }
    st4(dx + r * lddx + c, make_float4(o[0], o[1], o[2], o[3]));
  }
}

// y = x + bias (rows x H; y may be x)
__global__ void __launch_bounds__(256) add_bias_kernel(int64_t rows, int H, const float* x, int64_t ldx,
                                                       const float* __restrict__ bias, float* y, int64_t ldy) {
  const int nq = H >> 2;
  for (int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gi < rows * nq;
       gi += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = gi / nq;
    const int c = (int)(gi % nq) * 4;
    st4(y + r * ldy + c, gmr::f4_add(ld4(x + r * ldx + c), ld4(bias + c)));
  }
}

// One workgroup per row: target = x0 (1 - gamma) + (1 - x0) gamma with x0 the user's train row (LDS bitmap);
// loss_b = mean_I (pred - target)^2 (fp64);  pred <- ca (pred - target), ca = 2 / I * grad_scale.
__global__ void __launch_bounds__(256) ld4_loss_rows_kernel(int B, int I, const int* __restrict__ users,
                                                            const int* __restrict__ uptr, const int* __restrict__ uitems,
                                                            float gamma, float* __restrict__ pred, int64_t ld,
                                                            float grad_scale, double* __restrict__ loss_out,
                                                            int write_grad) {
  extern __shared__ __attribute__((aligned(16))) uint32_t bits[];
  const int b = blockIdx.x;
  const int u = users[b];
  const int nw = (I + 31) / 32;
  for (int i = threadIdx.x; i < nw; i += 256) bits[i] = 0u;
  __syncthreads();
  for (int e = uptr[u] + threadIdx.x; e < uptr[u + 1]; e += 256) {
    const int c = uitems[e];
    atomicOr(&bits[c >> 5], 1u << (c & 31));  // integer bit set, order-free
  }
  __syncthreads();
  const float hi = 1.f - gamma, lo = gamma;
  const float ca = (float)(2.0 / (double)I) * grad_scale;
  float* row = pred + (int64_t)b * ld;
  float s = 0.f;
  for (int i = threadIdx.x; i < I; i += 256) {
    const float tg = (bits[i >> 5] >> (i & 31)) & 1u ? hi : lo;
    const float d = row[i] - tg;
    s = fmaf(d, d, s);
    if (write_grad) row[i] = ca * d;
  }
  __shared__ double redd[4];
  const double sd = gmr::wave_sum_d((double)s);
  if ((threadIdx.x & 63) == 0) redd[threadIdx.x >> 6] = sd;
  __syncthreads();
  if (threadIdx.x == 0) loss_out[b] = ((redd[0] + redd[1]) + (redd[2] + redd[3])) / (double)I;
}

// hist[t_b] <- 0.9 hist[t_b] + 0.1 loss_b, rows in batch order: work-item k owns timestep k and walks the
// batch.  fp32 as the reference evaluates it: fl(0.9f * h) + fl32(0.1 * (double)fl32(loss_b)).
__global__ void __launch_bounds__(1024) history_ema_kernel(int B, int T, const int* __restrict__ t,
                                                           const double* __restrict__ loss, float* __restrict__ hist) {
#pragma clang fp contract(off)  // the product and the sum round separately, as the reference's two torch ops do
  constexpr int kChunk = 2048;  // batch rows staged in LDS at a time (t and the 0.1 loss term)
  __shared__ int ts[kChunk];
  __shared__ float ls[kChunk];
  const int k = threadIdx.x;
  float hv = k < T ? hist[k] : 0.f;
  bool hit = false;
  for (int base = 0; base < B; base += kChunk) {
    const int n = B - base < kChunk ? B - base : kChunk;
    for (int i = k; i < n; i += 1024) {
      ts[i] = t[base + i];
      ls[i] = (float)(0.1 * (double)(float)loss[base + i]);
    }
    __syncthreads();
    if (k < T)
      for (int i = 0; i < n; ++i)
        if (ts[i] == k) {
          const float prod = 0.9f * hv;
          hv = prod + ls[i];
          hit = true;
        }
    __syncthreads();
  }
  if (k < T && hit) hist[k] = hv;
}

// t_b = #{k : cdf_k <= u_b} clamped to T - 1; cdf = fp64 running sum of |hist| / sum |hist|
__global__ void __launch_bounds__(256) ld4_sample_t_kernel(int B, int T, const float* __restrict__ hist,
                                                           const float* __restrict__ u_in, uint64_t seed, uint64_t step,
                                                           int64_t row0, int* __restrict__ t) {
  __shared__ double cdf[1024];
  for (int k = threadIdx.x; k < T; k += 256) cdf[k] = fabs((double)hist[k]);
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int k = 0; k < T; ++k) tot += cdf[k];
    double run = 0.0;
    for (int k = 0; k < T; ++k) {
      run += cdf[k] / tot;
      cdf[k] = run;
    }
  }
  __syncthreads();
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  double u;
  if (u_in) {
    u = (double)u_in[b];
  } else {
    const uint4 q = gmr::Philox::gen(seed ^ 0xA5A5A5A5ull, step, (uint64_t)(row0 + b));
    u = (double)(q.x >> 8) * (1.0 / 16777216.0);  // [0, 1)
  }
  int lo = 0, hi = T;  // first k with cdf_k > u
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cdf[mid] <= u) lo = mid + 1;
    else hi = mid;
  }
  t[b] = lo < T ? lo : T - 1;
}

bool width_ok(int32_t H) { return H >= 64 && H <= 1024 && H % 64 == 0; }
bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

#define LD4_WIDTH(H) GMR_ARG(width_ok(H), "H must be a multiple of 64 in 64..1024")

extern "C" int gmr_ld4_film_fwd(int64_t rows, int32_t H, const float* h, int64_t ldh, const float* w, const float* b,
                                const float* s, int64_t lds, const float* sh, int64_t ldsh, float eps, float* z,
                                int64_t ldz, float* mean, float* rstd, void* stream) {
  GMR_ARG(h && w && b && s && sh && z && mean && rstd && rows > 0, "bad args");
  LD4_WIDTH(H);
  GMR_ARG(ldh >= H && lds >= H && ldsh >= H && ldz >= H && ldh % 4 == 0 && lds % 4 == 0 && ldsh % 4 == 0 && ldz % 4 == 0,
          "row strides must be >= H and multiples of 4");
  GMR_ARG(al16(h) && al16(w) && al16(b) && al16(s) && al16(sh) && al16(z), "16-byte alignment");
  hipLaunchKernelGGL(film_fwd_kernel, dim3(gmr::grid_for(rows, 4)), dim3(256), 0, (hipStream_t)stream, rows, (int)H, h,
                     ldh, w, b, s, lds, sh, ldsh, eps, z, ldz, mean, rstd);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int64_t gmr_ld4_film_parts_floats(int64_t rows, int32_t H) {
  return ((rows + kRowsPerBlock - 1) / kRowsPerBlock) * 2 * (int64_t)H;
}

extern "C" int gmr_ld4_film_bwd(int64_t rows, int32_t H, const float* h, int64_t ldh, const float* mean,
                                const float* rstd, const float* w, const float* b, const float* s, int64_t lds,
                                const float* dz, int64_t lddz, float* ds, int64_t ldds, float* dsh, int64_t lddsh,
                                float* dh, int64_t lddh, int32_t accumulate_dh, float* parts, float* dw, float* db,
                                int32_t accumulate_params, void* stream) {
  GMR_ARG(h && mean && rstd && w && b && s && dz && ds && dh && parts && dw && db && rows > 0, "bad args");
  LD4_WIDTH(H);
  GMR_ARG(ldh >= H && lds >= H && lddz >= H && ldds >= H && lddh >= H && (!dsh || lddsh >= H),
          "row strides must be >= H");
  GMR_ARG(ldh % 4 == 0 && lds % 4 == 0 && lddz % 4 == 0 && ldds % 4 == 0 && lddh % 4 == 0 && (!dsh || lddsh % 4 == 0),
          "row strides must be multiples of 4");
  GMR_ARG(al16(h) && al16(w) && al16(b) && al16(s) && al16(dz) && al16(ds) && al16(dsh) && al16(dh), "16-byte alignment");
  GMR_ARG(ds != dz && dh != dz, "ds and dh must not alias dz (dsh may)");
  hipStream_t st = (hipStream_t)stream;
  const int P = (int)((rows + kRowsPerBlock - 1) / kRowsPerBlock);
  hipLaunchKernelGGL(film_bwd_kernel, dim3(P), dim3(256), sizeof(float) * 8 * (size_t)H, st, rows, (int)H, h, ldh, mean,
                     rstd, w, b, s, lds, dz, lddz, ds, ldds, dsh, lddsh, dh, lddh, (int)accumulate_dh, parts);
  GMR_LAUNCHED();
  hipLaunchKernelGGL(film_param_reduce_kernel, dim3(gmr::grid_for(2 * H, 64)), dim3(1024), 0, st, P, (int)H, parts, dw,
                     db, (int)accumulate_params);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_ld4_gelu_drop_fwd(int64_t rows, int32_t H, const float* x, int64_t ldx, float p_keep,
                                     const uint8_t* mask_in, uint8_t* mask_out, int64_t ldm, uint64_t seed,
                                     uint64_t step, uint64_t ctr0, float* y, int64_t ldy, void* stream) {
  GMR_ARG(x && y && rows > 0, "bad args");
  LD4_WIDTH(H);
  GMR_ARG(p_keep > 0.f && p_keep <= 1.f, "p_keep in (0, 1]");
  GMR_ARG(ldx >= H && ldy >= H && ldx % 4 == 0 && ldy % 4 == 0 && al16(x) && al16(y),
          "row strides must be >= H and multiples of 4, 16-byte alignment");
  const int mode = p_keep >= 1.f ? 0 : (mask_in ? 1 : 2);
  GMR_ARG(mode == 0 || ldm >= H, "mask row stride must be >= H");
  hipLaunchKernelGGL(gelu_drop_fwd_kernel, dim3(gmr::grid_for(rows * (H / 4), 256, 16384)), dim3(256), 0,
                     (hipStream_t)stream, rows, (int)H, x, ldx, p_keep, mode, mask_in, mask_out, ldm, seed, step, ctr0, y,
                     ldy);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_ld4_gelu_drop_bwd(int64_t rows, int32_t H, const float* x, int64_t ldx, const uint8_t* mask,
                                     int64_t ldm, float p_keep, const float* dy, int64_t lddy, float* dx, int64_t lddx,
                                     void* stream) {
  GMR_ARG(x && dy && dx && rows > 0, "bad args");
  LD4_WIDTH(H);
  GMR_ARG(p_keep > 0.f && p_keep <= 1.f, "p_keep in (0, 1]");
  GMR_ARG(p_keep >= 1.f || (mask && ldm >= H), "p_keep < 1 needs the recorded mask");
  GMR_ARG(ldx >= H && lddy >= H && lddx >= H && ldx % 4 == 0 && lddy % 4 == 0 && lddx % 4 == 0 && al16(x) && al16(dy) &&
              al16(dx),
          "row strides must be >= H and multiples of 4, 16-byte alignment");
  hipLaunchKernelGGL(gelu_drop_bwd_kernel, dim3(gmr::grid_for(rows * (H / 4), 256, 16384)), dim3(256), 0,
                     (hipStream_t)stream, rows, (int)H, x, ldx, p_keep >= 1.f ? nullptr : mask, ldm, p_keep, dy, lddy, dx,
                     lddx);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_ld4_add_bias(int64_t rows, int32_t H, const float* x, int64_t ldx, const float* bias, float* y,
                                int64_t ldy, void* stream) {
  GMR_ARG(x && bias && y && rows > 0, "bad args");
  LD4_WIDTH(H);
  GMR_ARG(ldx >= H && ldy >= H && ldx % 4 == 0 && ldy % 4 == 0 && al16(x) && al16(bias) && al16(y),
          "row strides must be >= H and multiples of 4, 16-byte alignment");
  hipLaunchKernelGGL(add_bias_kernel, dim3(gmr::grid_for(rows * (H / 4), 256, 16384)), dim3(256), 0,
                     (hipStream_t)stream, rows, (int)H, x, ldx, bias, y, ldy);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_ld4_loss_rows(int32_t B, int32_t I, const int32_t* users, const int32_t* user_ptr,
                                 const int32_t* user_items, float gamma, float* pred, int64_t ld, float grad_scale,
                                 double* loss_out, int32_t write_grad, void* stream) {
  GMR_ARG(users && user_ptr && user_items && pred && loss_out && B > 0 && I > 0 && ld >= I, "bad args");
  const size_t dyn = sizeof(uint32_t) * (size_t)((I + 31) / 32);
  GMR_ARG(dyn <= 60000, "item count too large for the LDS bitmap");
  hipLaunchKernelGGL(ld4_loss_rows_kernel, dim3(B), dim3(256), dyn, (hipStream_t)stream, B, I, users, user_ptr,
                     user_items, gamma, pred, ld, grad_scale, loss_out, (int)write_grad);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_ld4_history_ema(int32_t B, int32_t T, const int32_t* t, const double* loss, float* hist,
                                   void* stream) {
  GMR_ARG(t && loss && hist && B > 0 && T > 0 && T <= 1024, "bad args (T <= 1024)");
  hipLaunchKernelGGL(history_ema_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, B, T, t, loss, hist);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_ld4_sample_t(int32_t B, int32_t T, const float* hist, const float* u, uint64_t seed, uint64_t step,
                                int64_t row0, int32_t* t, void* stream) {
  GMR_ARG(hist && t && B > 0 && T > 0 && T <= 1024 && row0 >= 0, "bad args (T <= 1024)");
  hipLaunchKernelGGL(ld4_sample_t_kernel, dim3(gmr::grid_for(B, 256)), dim3(256), 0, (hipStream_t)stream, B, T, hist, u,
                     seed, step, row0, t);
  GMR_LAUNCHED();
  return GMR_OK;
}
