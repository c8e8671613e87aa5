// LGMRec (models/lgmrec.py of the reference): the global hypergraph embedding block as fp32 row kernels with their
// backward.  Per modality m in {v, t}, with H = hyper_num <= 64 hyperedges:
//   Li_m = X_m Hy_m (I x H, a column block of the projection GEMM's output),  Lu_m = adj Li_m (a sum over the user's items)
//   S = softmax((L + g) / tau) per row, g Gumbel(0, 1);  h = dropout(S, 1 - keep_rate)
//   lat_m = hi_m^T E (H x 64);  x_m = h_m lat_m on all N = U + I rows
//   all = cge + n(mge_v) + n(mge_t) + alpha n(x_v + x_t),  n(x) = x / max(|x|, 1e-12)
//
//   gmr_lgm_hyper_fwd    one wave per row: the user rows' CSR sums, the draws, the softmax and the dropout
//   gmr_lgm_lat          A^T X per modality over n rows: per-tile partials, then a fixed-order fp64 sum
//   gmr_lgm_apply        Y = A_m M_m rows
//   gmr_lgm_combine_fwd  x_v, x_t, the five norms, all and the [n(x_v) | n(x_t)] table in one launch
//   gmr_lgm_combine_bwd  the three normalise backwards of all
//   gmr_lgm_dh           dh = X M^T rows (+ acc), optionally through the dropout and softmax backward to d L
//   gmr_lgm_logit_bwd    d Li += the users' d Lu through the transposed CSR, in gather form
//   gmr_lgm_reg          the Frobenius-norm regulariser of the three batch row sets and its rows
//
// Layouts: S, h, d h, d L are n x 2H tables [v | t]; lat and d lat are [2][H][64].  Every H is HBM-bound (2 H 64 flop
// per 64-float row), so the products run on the vector ALU from LDS-staged matrices.  No float atomics: a row's result
// depends on its own inputs only, a sum over rows goes through per-tile partials that a second pass adds in tile order
// (sixteen fp64 slices, one fixed tree), so no result depends on the grid.
#include <math.h>

#include "row_tile.h"

namespace {

using namespace gmr_row;  // D, LDX, ld4 / st4, dot4, row16_sum, rows16 (csrc/row_tile.h)
using gmr::f4_add;
using gmr::f4_scale;
constexpr int MAXH = 64;
constexpr int MAX_BLOCKS = 1024;
constexpr int LT = 32;  // rows of a reduction tile
constexpr int RED_SLICES = 16;
constexpr int LDM = D + 1;  // row stride of a staged [2H][64] matrix read by column index per lane
constexpr float EPS = 1e-12f;
constexpr uint64_t SITE_MIX = 0x9E3779B97F4A7C15ull;
constexpr uint64_t SITE_LGM = 0x4C474D52ull;  // sites SITE_LGM + 4 m + 2 (item row) + (dropout)

__device__ __forceinline__ float4 zero_f4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 fma4(float s, float4 a, float4 acc) {
  return make_float4(fmaf(s, a.x, acc.x), fmaf(s, a.y, acc.y), fmaf(s, a.z, acc.z), fmaf(s, a.w, acc.w));
}
__device__ __forceinline__ float4 div4(float4 a, float s) { return make_float4(a.x / s, a.y / s, a.z / s, a.w / s); }
__device__ __forceinline__ float4 sub4(float4 a, float4 b) {
  return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
}
__device__ __forceinline__ float norm16(float4 x) { return fmaxf(sqrtf(row16_sum(dot4(x, x))), EPS); }
// d x of y = x / max(|x|, eps) from d y: (d y - y <y, d y>) / nrm; a clamped norm has no projection term
__device__ __forceinline__ float4 nbwd16(float4 y, float nrm, float4 dy) {
  float dp = row16_sum(dot4(y, dy));
  if (nrm <= EPS) dp = 0.f;
  return div4(sub4(dy, f4_scale(dp, y)), nrm);
}

// the 32 random bits of (site, step, row, column): a row's draws do not depend on the tiling or on the row count
__device__ __forceinline__ uint32_t draw_bits(uint64_t seed, uint64_t step, int site, int64_t row, int k) {
  const uint4 q = gmr::Philox::gen(seed + (SITE_LGM + (uint64_t)site) * SITE_MIX, step, (uint64_t)row * 16 + (k >> 2));
  const int e = k & 3;
  return e == 0 ? q.x : e == 1 ? q.y : e == 2 ? q.z : q.w;
}
// u in (0, 1) on 23 bits, both ends excluded: g = -log(-log(u)) is finite
__device__ __forceinline__ float gumbel_of(uint32_t bits) {
  const float u = ((float)(bits >> 9) + 0.5f) * (1.0f / 8388608.0f);
  return -logf(-logf(u));
}
__device__ __forceinline__ bool keep_of(uint32_t bits, float p_keep) {
  return (float)(bits >> 8) * (1.0f / 16777216.0f) < p_keep;
}

// ------------------------------------------------------------------------------------------------ hyperedge rows
struct HyperArgs {
  int64_t U, I;
  int H;
  const float* L[2];
  int64_t ldl[2];
  const int32_t *rowptr, *col;
  const float* g[2];  // given Gumbel draws (N x H each), or null
  int64_t ldg;
  const uint8_t* keep[2];  // given keep bytes (N x H each), or null
  int64_t ldk;
  float tau, p_keep;
  int drop;  // 0 none, 1 keep bytes given, 2 drawn
  uint64_t seed, step;
  float *S, *h;
  int64_t ldh;
};

// One wave per row.  HP = H rounded up to a power of two; lane = grp HP + k.  A user row's entry e (in column order)
// goes to group (e - row start) mod (64 / HP); the groups' sums meet in one xor butterfly, which leaves the same bits
// in every group.
__global__ __launch_bounds__(256) void lgm_hyper_fwd_kernel(HyperArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int HP = 1;
  while (HP < a.H) HP <<= 1;
  const int k = lane & (HP - 1), grp = lane / HP, G = 64 / HP;
  const bool kin = k < a.H;
  const int64_t N = a.U + a.I;
  const float scale = 1.f / a.p_keep;
  for (int64_t r = (int64_t)blockIdx.x * 4 + wv; r < N; r += (int64_t)gridDim.x * 4) {
    const bool user = r < a.U;
    const int64_t lr = user ? r : r - a.U;
    int e0 = 0, e1 = 0;
    if (user) {
      e0 = a.rowptr[r];
      e1 = a.rowptr[r + 1];
    }
    for (int m = 0; m < 2; ++m) {
      const float* L = a.L[m];
      const int64_t ld = a.ldl[m];
      float x = 0.f;
      if (user) {
        if (kin)
          for (int e = e0 + grp; e < e1; e += G) x += L[(int64_t)a.col[e] * ld + k];
        for (int mk = HP; mk < 64; mk <<= 1) x += __shfl_xor(x, mk);
      } else if (kin) {
        x = L[lr * ld + k];
      }
      const int site = 4 * m + (user ? 0 : 2);
      float gum = 0.f;
      if (kin) gum = a.g[m] ? a.g[m][r * a.ldg + k] : gumbel_of(draw_bits(a.seed, a.step, site, lr, k));
      const float z = kin ? (x + gum) / a.tau : -INFINITY;
      float mx = z;
      for (int mk = HP >> 1; mk >= 1; mk >>= 1) mx = fmaxf(mx, __shfl_xor(mx, mk));
      const float ex = kin ? expf(z - mx) : 0.f;
      float sm = ex;
      for (int mk = HP >> 1; mk >= 1; mk >>= 1) sm += __shfl_xor(sm, mk);
      const float s = ex / sm;
      float hv = s;
      if (a.drop && kin) {
        const bool kp = a.drop == 1 ? a.keep[m][r * a.ldk + k] != 0
                                    : keep_of(draw_bits(a.seed, a.step, site + 1, lr, k), a.p_keep);
        hv = kp ? s * scale : 0.f;
      }
      if (grp == 0 && kin) {
        a.S[r * a.ldh + m * a.H + k] = s;
        a.h[r * a.ldh + m * a.H + k] = hv;
      }
    }
  }
}

// the draws of one site as the row kernel makes them: g (n x H) and keep bytes (n x H), either may be null
__global__ void lgm_draws_kernel(int64_t n, int H, int site, uint64_t seed, uint64_t step, float p_keep, float* g,
                                 uint8_t* keep) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * H) return;
  const int64_t r = i / H;
  const int k = (int)(i - r * H);
  if (g) g[i] = gumbel_of(draw_bits(seed, step, site, r, k));
  if (keep) keep[i] = keep_of(draw_bits(seed, step, site + 1, r, k), p_keep) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ A^T X over rows
struct LatArgs {
  int64_t n;
  const float* A;
  int64_t lda;
  int H;
  const float* X[2];
  int64_t ldx;
  float* ws;  // [tile][2H][64]
};

__global__ __launch_bounds__(256) void lgm_lat_part_kernel(LatArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, c = tid & 63, w = tid >> 6, H2 = 2 * a.H;
  float* sX = lds;                // [2][LT][64]
  float* sA = lds + 2 * LT * D;   // [LT][2H]
  const int64_t ntiles = (a.n + LT - 1) / LT;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t r0 = t * LT;
    for (int i = tid; i < LT * H2; i += 256) {
      const int r = i / H2, kk = i - r * H2;
      sA[i] = r0 + r < a.n ? a.A[(r0 + r) * a.lda + kk] : 0.f;
    }
    for (int i = tid; i < 2 * LT * 16; i += 256) {
      const int m = i / (LT * 16), rem = i - m * LT * 16, r = rem >> 4, cc = (rem & 15) * 4;
      st4(sX + (m * LT + r) * D + cc, r0 + r < a.n ? ld4(a.X[m] + (r0 + r) * a.ldx + cc) : zero_f4());
    }
    __syncthreads();
    for (int kk = w; kk < H2; kk += 4) {
      const float* x = sX + (kk >= a.H ? LT * D : 0);
      float acc = 0.f;
#pragma unroll 8
      for (int r = 0; r < LT; ++r) acc = fmaf(sA[r * H2 + kk], x[r * D + c], acc);
      a.ws[(t * H2 + kk) * D + c] = acc;
    }
    __syncthreads();
  }
}

// one workgroup per (modality, hyperedge): sixteen slices of tiles (tile mod 16) summed in tile order in fp64, then one
// fixed tree; a tile of zeros leaves the bits as they are
__global__ __launch_bounds__(RED_SLICES * D) void lgm_lat_reduce_kernel(int64_t ntiles, int H2,
                                                                        const float* __restrict__ ws,
                                                                        float* __restrict__ out) {
  __shared__ double s[RED_SLICES][D];
  const int kk = blockIdx.x, j = threadIdx.x & 63, sl = threadIdx.x >> 6;
  double acc = 0.0;
  for (int64_t i = sl; i < ntiles; i += RED_SLICES) acc += (double)ws[(i * H2 + kk) * D + j];
  s[sl][j] = acc;
  __syncthreads();
  for (int off = RED_SLICES / 2; off >= 1; off >>= 1) {
    if (sl < off) s[sl][j] += s[sl + off][j];
    __syncthreads();
  }
  if (sl == 0) out[kk * D + j] = (float)s[0][j];
}

// ------------------------------------------------------------------------------------------------ rows of A M
__device__ __forceinline__ void stage_m(float* sM, const float* __restrict__ M, int H2, int ld) {
  for (int i = threadIdx.x; i < H2 * D; i += 256) sM[(i >> 6) * ld + (i & 63)] = M[i];
}
// x_v, x_t of one row on this thread's four columns: sM is [2H][64] with stride 64
__device__ __forceinline__ void apply_row(const float* arow, int H, const float* sM, int c, float4& xv, float4& xt) {
  xv = zero_f4();
  xt = zero_f4();
  for (int k = 0; k < H; ++k) {
    xv = fma4(arow[k], ld4(sM + k * D + c), xv);
    xt = fma4(arow[H + k], ld4(sM + (H + k) * D + c), xt);
  }
}

__global__ __launch_bounds__(256) void lgm_apply_kernel(int64_t n, const float* __restrict__ A, int64_t lda, int H,
                                                        const float* __restrict__ M, float* Y, int64_t ldy, int mode) {
  extern __shared__ __attribute__((aligned(16))) float sM[];
  stage_m(sM, M, 2 * H, D);
  __syncthreads();
  const int row = threadIdx.x >> 4, c = (threadIdx.x & 15) * 4;
  const int64_t ntiles = (n + 15) / 16;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t gr = t * 16 + row;
    if (gr >= n) continue;
    float4 xv, xt;
    apply_row(A + gr * lda, H, sM, c, xv, xt);
    if (mode == 0) {
      st4(Y + gr * ldy + c, xv);
      st4(Y + gr * ldy + D + c, xt);
    } else {
      st4(Y + gr * ldy + c, f4_add(ld4(Y + gr * ldy + c), f4_add(xv, xt)));
    }
  }
}

struct CombArgs {
  int64_t n;
  const float* cge;
  int64_t ldc;
  const float* mge;  // [mge_v | mge_t]
  int64_t ldm;
  const float* h;
  int64_t ldh;
  int H;
  const float* lat;
  float alpha;
  float* all;
  int64_t ldo;
  float* CLN;    // n x 128: [n(x_v) | n(x_t)]
  float* nrmCL;  // [2][n]
  float* nrm3;   // [3][n]: |mge_v|, |mge_t|, |x_v + x_t| (clamped)
};

__global__ __launch_bounds__(256) void lgm_combine_fwd_kernel(CombArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sM[];
  stage_m(sM, a.lat, 2 * a.H, D);
  __syncthreads();
  const int row = threadIdx.x >> 4, c = (threadIdx.x & 15) * 4;
  const int64_t ntiles = (a.n + 15) / 16;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t gr = t * 16 + row;
    const bool ok = gr < a.n;
    float4 xv = zero_f4(), xt = zero_f4(), mv = zero_f4(), mt = zero_f4();
    if (ok) {
      apply_row(a.h + gr * a.ldh, a.H, sM, c, xv, xt);
      mv = ld4(a.mge + gr * a.ldm + c);
      mt = ld4(a.mge + gr * a.ldm + D + c);
    }
    const float4 g = f4_add(xv, xt);
    const float nxv = norm16(xv), nxt = norm16(xt), ng = norm16(g), nmv = norm16(mv), nmt = norm16(mt);
    if (!ok) continue;
    const float4 loc = f4_add(f4_add(ld4(a.cge + gr * a.ldc + c), div4(mv, nmv)), div4(mt, nmt));
    st4(a.all + gr * a.ldo + c, f4_add(loc, f4_scale(a.alpha, div4(g, ng))));
    st4(a.CLN + gr * 128 + c, div4(xv, nxv));
    st4(a.CLN + gr * 128 + D + c, div4(xt, nxt));
    if ((threadIdx.x & 15) == 0) {
      a.nrmCL[gr] = nxv;
      a.nrmCL[a.n + gr] = nxt;
      a.nrm3[gr] = nmv;
      a.nrm3[a.n + gr] = nmt;
      a.nrm3[2 * a.n + gr] = ng;
    }
  }
}

struct CombBwdArgs {
  int64_t n;
  const float* dall;
  int64_t ldda;
  const float* mge;
  int64_t ldm;
  const float *CLN, *nrmCL, *nrm3;
  float alpha;
  float* dmge;
  int64_t lddm;
  float* dK;  // n x 128, added to: [d x_v | d x_t]
};

__global__ __launch_bounds__(256) void lgm_combine_bwd_kernel(CombBwdArgs a) {
  const int row = threadIdx.x >> 4, c = (threadIdx.x & 15) * 4;
  const int64_t ntiles = (a.n + 15) / 16;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t gr = t * 16 + row;
    const bool ok = gr < a.n;
    float4 da = zero_f4(), mv = zero_f4(), mt = zero_f4(), g = zero_f4();
    float nmv = 1.f, nmt = 1.f, ng = 1.f;
    if (ok) {
      da = ld4(a.dall + gr * a.ldda + c);
      mv = ld4(a.mge + gr * a.ldm + c);
      mt = ld4(a.mge + gr * a.ldm + D + c);
      nmv = a.nrm3[gr];
      nmt = a.nrm3[a.n + gr];
      ng = a.nrm3[2 * a.n + gr];
      g = f4_add(f4_scale(a.nrmCL[gr], ld4(a.CLN + gr * 128 + c)),
                 f4_scale(a.nrmCL[a.n + gr], ld4(a.CLN + gr * 128 + D + c)));
    }
    const float4 dmv = nbwd16(div4(mv, nmv), nmv, da), dmt = nbwd16(div4(mt, nmt), nmt, da);
    const float4 dg = nbwd16(div4(g, ng), ng, f4_scale(a.alpha, da));
    if (!ok) continue;
    st4(a.dmge + gr * a.lddm + c, dmv);
    st4(a.dmge + gr * a.lddm + D + c, dmt);
    float* k = a.dK + gr * 128 + c;
    st4(k, f4_add(ld4(k), dg));
    st4(k + D, f4_add(ld4(k + D), dg));
  }
}

// ------------------------------------------------------------------------------------------------ rows of X M^T
struct DhArgs {
  int64_t n;
  const float* X[2];
  int64_t ldx;
  const float* M;  // [2][H][64]
  int H;
  const float* acc;  // n x 2H added to the products, or null
  int64_t ldacc;
  const float *S, *h;  // both given: the dropout and softmax backward, out = d L
  int64_t ldh;
  float p_keep, tau;
  float* out;
  int64_t ldo;
};

// 16 rows per pass; thread (row, j) owns the outputs kk = j, j + 16, .. < 2H of its row.  Every 64-term product is one
// fma chain in fp64, rounded once (the kernel is bound by its rows' bytes, not by 2 H 64 fp64 fma per row): fp32
// torch's products are within an ulp of exact, and the softmax backward multiplies their error by up to 1 / (tau
// keep_rate).  <d S, S> and the last line run in fp64 as well.
__global__ __launch_bounds__(256) void lgm_dh_kernel(DhArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int H2 = 2 * a.H;
  float* sX = lds;                                                  // [2][16][LDX]
  float* sD = lds + 2 * 16 * LDX;                                   // [16][2H]
  double* sI = reinterpret_cast<double*>(sD + 16 * H2);             // [16][2]
  float* sM = sD + 16 * H2 + 64;                                    // [2H][LDM]
  stage_m(sM, a.M, H2, LDM);
  const int tid = threadIdx.x, row = tid >> 4, j = tid & 15, c = j * 4;
  const bool sbwd = a.S != nullptr;
  const double scale = 1.0 / (double)a.p_keep;
  const int64_t ntiles = (a.n + 15) / 16;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t gr = t * 16 + row;
    const bool ok = gr < a.n;
    st4(sX + row * LDX + c, ok ? ld4(a.X[0] + gr * a.ldx + c) : zero_f4());
    st4(sX + (16 + row) * LDX + c, ok ? ld4(a.X[1] + gr * a.ldx + c) : zero_f4());
    __syncthreads();
    for (int kk = j; kk < H2; kk += 16) {
      const float* x = sX + ((kk >= a.H ? 16 : 0) + row) * LDX;
      const float* mr = sM + kk * LDM;
      double acc = 0.0;
#pragma unroll 8
      for (int d = 0; d < D; ++d) acc = fma((double)x[d], (double)mr[d], acc);
      float v = (float)acc;
      if (a.acc && ok) v += a.acc[gr * a.ldacc + kk];
      if (sbwd)
        sD[row * H2 + kk] = v;
      else if (ok)
        a.out[gr * a.ldo + kk] = v;
    }
    if (sbwd) {
      __syncthreads();
      if (j < 2 && ok) {  // <d S, S> of (row, modality j), hyperedges in order
        const float *hr = a.h + gr * a.ldh + j * a.H, *sr = a.S + gr * a.ldh + j * a.H, *dr = sD + row * H2 + j * a.H;
        double inner = 0.0;
        for (int k = 0; k < a.H; ++k) inner = fma(hr[k] != 0.f ? (double)dr[k] * scale : 0.0, (double)sr[k], inner);
        sI[row * 2 + j] = inner;
      }
      __syncthreads();
      if (ok)
        for (int kk = j; kk < H2; kk += 16) {
          // a dropped entry has h = 0; an entry whose probability underflowed to 0 has S = 0 and gets 0 either way
          const double ds = a.h[gr * a.ldh + kk] != 0.f ? (double)sD[row * H2 + kk] * scale : 0.0;
          a.out[gr * a.ldo + kk] =
              (float)((double)a.S[gr * a.ldh + kk] * (ds - sI[row * 2 + (kk >= a.H ? 1 : 0)]) / (double)a.tau);
        }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ d Lu to the items
struct LogitBwdArgs {
  int64_t U, I;
  int H;
  const float* dL;
  int64_t lddl;
  const int32_t *trp, *tcol;  // the I x U transpose of the interaction CSR
  float* out[2];
  int64_t ldo[2];
};

__global__ __launch_bounds__(256) void lgm_logit_bwd_kernel(LogitBwdArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int HP = 1;
  while (HP < a.H) HP <<= 1;
  const int k = lane & (HP - 1), grp = lane / HP, G = 64 / HP;
  const bool kin = k < a.H;
  for (int64_t i = (int64_t)blockIdx.x * 4 + wv; i < a.I; i += (int64_t)gridDim.x * 4) {
    const int e0 = a.trp[i], e1 = a.trp[i + 1];
    for (int m = 0; m < 2; ++m) {
      float x = 0.f;
      if (kin) {
        if (grp == 0) x = a.dL[(a.U + i) * a.lddl + m * a.H + k];
        for (int e = e0 + grp; e < e1; e += G) x += a.dL[(int64_t)a.tcol[e] * a.lddl + m * a.H + k];
      }
      for (int mk = HP; mk < 64; mk <<= 1) x += __shfl_xor(x, mk);
      if (grp == 0 && kin) a.out[m][i * a.ldo[m] + k] = x;
    }
  }
}

// ------------------------------------------------------------------------------------------------ regulariser
// reg = coef (|all[users]|_F + |all[U + pos]|_F + |all[U + neg]|_F); contrib (3B x 64: [du; dp; dn]) += its rows.
// One workgroup: thread t sums the squares of elements t, t + 1024, .. in fp64, one fixed tree per set.
__global__ __launch_bounds__(1024) void lgm_reg_kernel(int B, int64_t U, const float* __restrict__ all, int64_t lda,
                                                       const int32_t* users, const int32_t* pos, const int32_t* neg,
                                                       float coef, float* contrib, int64_t ldc, float* out) {
  __shared__ double s[1024];
  __shared__ float nrm[3];
  const int tid = threadIdx.x;
  const int32_t* idx[3] = {users, pos, neg};
  for (int q = 0; q < 3; ++q) {
    double acc = 0.0;
    for (int64_t e = tid; e < (int64_t)B * D; e += 1024) {
      const float v = all[((q ? U : 0) + idx[q][e >> 6]) * lda + (e & 63)];
      acc += (double)v * (double)v;
    }
    s[tid] = acc;
    __syncthreads();
    for (int off = 512; off >= 1; off >>= 1) {
      if (tid < off) s[tid] += s[tid + off];
      __syncthreads();
    }
    if (tid == 0) nrm[q] = (float)sqrt(s[0]);
    __syncthreads();
  }
  if (tid == 0) out[0] = coef * (nrm[0] + nrm[1] + nrm[2]);
  for (int q = 0; q < 3; ++q) {
    const float sc = nrm[q] > 0.f ? coef / nrm[q] : 0.f;
    for (int64_t e = tid; e < (int64_t)B * D; e += 1024) {
      float* o = contrib + ((int64_t)q * B + (e >> 6)) * ldc + (e & 63);
      *o += sc * all[((q ? U : 0) + idx[q][e >> 6]) * lda + (e & 63)];
    }
  }
}

inline unsigned cap_grid(int64_t units, int32_t max_blocks) {
  return (unsigned)gmr::grid_for(units, 1, max_blocks > 0 ? max_blocks : MAX_BLOCKS);
}
inline bool h_ok(int32_t H) { return H >= 1 && H <= MAXH; }

}  // namespace

// ==================================================================================================== C ABI
#define LGM_H(H) GMR_ARG(h_ok(H), "hyper_num: 1..64")

extern "C" int32_t gmr_lgm_tile_rows(void) { return LT; }
extern "C" int32_t gmr_lgm_max_blocks(void) { return MAX_BLOCKS; }
extern "C" int64_t gmr_lgm_lat_ws_floats(int64_t n, int32_t H) {
  return n < 1 || !h_ok(H) ? 0 : (n + LT - 1) / LT * 2 * H * D;
}

extern "C" int gmr_lgm_hyper_fwd(int64_t U, int64_t I, int32_t H, const float* Lv, int64_t ldlv, const float* Lt,
                                 int64_t ldlt, const int32_t* rowptr, const int32_t* col, const float* gv,
                                 const float* gt, int64_t ldg, const uint8_t* keepv, const uint8_t* keept, int64_t ldk,
                                 float tau, float p_keep, int32_t drop_mode, uint64_t seed, uint64_t step, float* S,
                                 float* h, int64_t ldh, int32_t max_blocks, void* stream) {
  LGM_H(H);
  GMR_ARG(U >= 0 && I >= 1 && U + I < (1ll << 31), "bad row counts");
  GMR_ARG(Lv && Lt && ldlv >= H && ldlt >= H && S && h && ldh >= 2 * H, "logits: ld >= H; S, h: ld >= 2 H");
  GMR_ARG(U == 0 || (rowptr && col), "user rows need the interaction CSR");
  GMR_ARG((gv == nullptr) == (gt == nullptr) && (!gv || ldg >= H), "given Gumbel draws: both modalities, ld >= H");
  GMR_ARG(tau > 0.f && p_keep > 0.f && p_keep <= 1.f && drop_mode >= 0 && drop_mode <= 2,
          "tau > 0, 0 < keep_rate <= 1, mode 0, 1 or 2");
  GMR_ARG(drop_mode != 1 || (keepv && keept && ldk >= H), "given keep bytes: both modalities, ld >= H");
  HyperArgs a{U, I, (int)H, {Lv, Lt}, {ldlv, ldlt}, rowptr, col, {gv, gt}, ldg, {keepv, keept}, ldk, tau, p_keep,
              p_keep < 1.f ? (int)drop_mode : 0, seed, step, S, h, ldh};
  hipLaunchKernelGGL(lgm_hyper_fwd_kernel, dim3(cap_grid((U + I + 3) / 4, max_blocks)), dim3(256), 0,
                     (hipStream_t)stream, a);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_lgm_draws(int64_t n, int32_t H, int32_t site, uint64_t seed, uint64_t step, float p_keep, float* g,
                             uint8_t* keep, void* stream) {
  LGM_H(H);
  GMR_ARG(n >= 1 && n < (1ll << 31) && site >= 0 && site < 8 && site % 2 == 0, "rows >= 1; site 0, 2, 4 or 6");
  hipLaunchKernelGGL(lgm_draws_kernel, dim3(gmr::grid_for(n * H, 256)), dim3(256), 0, (hipStream_t)stream, n, (int)H,
                     (int)site, seed, step, p_keep, g, keep);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_lgm_lat(int64_t n, const float* A, int64_t lda, int32_t H, const float* Xv, const float* Xt,
                           int64_t ldx, float* ws, int64_t ws_floats, int32_t max_blocks, float* lat, void* stream) {
  LGM_H(H);
  GMR_ARG(n >= 1 && n < (1ll << 31), "bad row count");
  GMR_ARG(A && lda >= 2 * H && lat, "A: n x 2H, ld >= 2 H");
  GMR_ARG(rows16(Xv, ldx) && rows16(Xt, ldx), "X rows must be 16-byte aligned with ld >= 64, ld % 4 == 0");
  GMR_ARG(ws && ws_floats >= gmr_lgm_lat_ws_floats(n, H), "workspace: gmr_lgm_lat_ws_floats(n, H) floats");
  const int64_t ntiles = (n + LT - 1) / LT;
  LatArgs a{n, A, lda, (int)H, {Xv, Xt}, ldx, ws};
  hipLaunchKernelGGL(lgm_lat_part_kernel, dim3(cap_grid(ntiles, max_blocks)), dim3(256),
                     (2 * LT * D + LT * 2 * H) * sizeof(float), (hipStream_t)stream, a);
  GMR_LAUNCHED();
  hipLaunchKernelGGL(lgm_lat_reduce_kernel, dim3(2 * H), dim3(RED_SLICES * D), 0, (hipStream_t)stream, ntiles,
                     (int)(2 * H), ws, lat);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_lgm_apply(int64_t n, const float* A, int64_t lda, int32_t H, const float* M, float* Y, int64_t ldy,
                             int32_t mode, int32_t max_blocks, void* stream) {
  LGM_H(H);
  GMR_ARG(n >= 1 && n < (1ll << 31), "bad row count");
  GMR_ARG(A && lda >= 2 * H && M && (mode == 0 || mode == 1), "A: n x 2H, ld >= 2 H; mode 0 or 1");
  GMR_ARG(rows16(Y, ldy, mode == 0 ? 2 * D : D), "Y rows must be 16-byte aligned (mode 0: ld >= 128, 1: ld >= 64)");
  hipLaunchKernelGGL(lgm_apply_kernel, dim3(cap_grid((n + 15) / 16, max_blocks)), dim3(256), 2 * H * D * sizeof(float),
                     (hipStream_t)stream, n, A, lda, (int)H, M, Y, ldy, (int)mode);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_lgm_combine_fwd(int64_t n, const float* cge, int64_t ldc, const float* mge, int64_t ldm,
                                   const float* h, int64_t ldh, int32_t H, const float* lat, float alpha, float* all,
                                   int64_t ldo, float* CLN, float* nrmCL, float* nrm3, int32_t max_blocks,
                                   void* stream) {
  LGM_H(H);
  GMR_ARG(n >= 1 && n < (1ll << 31), "bad row count");
  GMR_ARG(h && ldh >= 2 * H && lat && nrmCL && nrm3, "h: n x 2H, ld >= 2 H");
  GMR_ARG(rows16(cge, ldc) && rows16(mge, ldm, 2 * D) && rows16(all, ldo) && rows16(CLN, 2 * D, 2 * D),
          "rows must be 16-byte aligned (mge: ld >= 128, cge, all: ld >= 64), ld % 4 == 0");
  CombArgs a{n, cge, ldc, mge, ldm, h, ldh, (int)H, lat, alpha, all, ldo, CLN, nrmCL, nrm3};
  hipLaunchKernelGGL(lgm_combine_fwd_kernel, dim3(cap_grid((n + 15) / 16, max_blocks)), dim3(256),
                     2 * H * D * sizeof(float), (hipStream_t)stream, a);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_lgm_combine_bwd(int64_t n, const float* dall, int64_t ldda, const float* mge, int64_t ldm,
                                   const float* CLN, const float* nrmCL, const float* nrm3, float alpha, float* dmge,
                                   int64_t lddm, float* dK, int32_t max_blocks, void* stream) {
  GMR_ARG(n >= 1 && n < (1ll << 31), "bad row count");
  GMR_ARG(nrmCL && nrm3, "null pointer");
  GMR_ARG(rows16(dall, ldda) && rows16(mge, ldm, 2 * D) && rows16(CLN, 2 * D, 2 * D) && rows16(dmge, lddm, 2 * D) &&
              rows16(dK, 2 * D, 2 * D),
          "rows must be 16-byte aligned (mge, dmge: ld >= 128, dall: ld >= 64), ld % 4 == 0");
  CombBwdArgs a{n, dall, ldda, mge, ldm, CLN, nrmCL, nrm3, alpha, dmge, lddm, dK};
  hipLaunchKernelGGL(lgm_combine_bwd_kernel, dim3(cap_grid((n + 15) / 16, max_blocks)), dim3(256), 0,
                     (hipStream_t)stream, a);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_lgm_dh(int64_t n, const float* Xv, const float* Xt, int64_t ldx, const float* M, int32_t H,
                          const float* acc, int64_t ldacc, const float* S, const float* h, int64_t ldh, float p_keep,
                          float tau, float* out, int64_t ldo, int32_t max_blocks, void* stream) {
  LGM_H(H);
  GMR_ARG(n >= 1 && n < (1ll << 31), "bad row count");
  GMR_ARG(rows16(Xv, ldx) && rows16(Xt, ldx), "X rows must be 16-byte aligned with ld >= 64, ld % 4 == 0");
  GMR_ARG(M && out && ldo >= 2 * H && (!acc || ldacc >= 2 * H), "out, acc: n x 2H, ld >= 2 H");
  GMR_ARG((S == nullptr) == (h == nullptr) && (!S || (ldh >= 2 * H && tau > 0.f && p_keep > 0.f && p_keep <= 1.f)),
          "S and h together: ld >= 2 H, tau > 0, 0 < keep_rate <= 1");
  DhArgs a{n, {Xv, Xt}, ldx, M, (int)H, acc, ldacc, S, h, ldh, p_keep, tau, out, ldo};
  const size_t lds = (2 * 16 * LDX + 16 * 2 * H + 64 + 2 * H * LDM) * sizeof(float);
  hipLaunchKernelGGL(lgm_dh_kernel, dim3(cap_grid((n + 15) / 16, max_blocks)), dim3(256), lds, (hipStream_t)stream,
                     a);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_lgm_logit_bwd(int64_t U, int64_t I, int32_t H, const float* dL, int64_t lddl, const int32_t* trp,
                                 const int32_t* tcol, float* outv, int64_t ldov, float* outt, int64_t ldot,
                                 int32_t max_blocks, void* stream) {
  LGM_H(H);
  GMR_ARG(U >= 0 && I >= 1 && U + I < (1ll << 31), "bad row counts");
  GMR_ARG(dL && lddl >= 2 * H && trp && (U == 0 || tcol) && outv && outt && ldov >= H && ldot >= H,
          "dL: ld >= 2 H; outputs: ld >= H");
  LogitBwdArgs a{U, I, (int)H, dL, lddl, trp, tcol, {outv, outt}, {ldov, ldot}};
  hipLaunchKernelGGL(lgm_logit_bwd_kernel, dim3(cap_grid((I + 3) / 4, max_blocks)), dim3(256), 0, (hipStream_t)stream, a);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_lgm_reg(int32_t B, int64_t U, const float* all, int64_t lda, const int32_t* users,
                           const int32_t* pos, const int32_t* neg, float coef, float* contrib, int64_t ldc, float* out,
                           void* stream) {
  GMR_ARG(B >= 1 && U >= 0, "bad row counts");
  GMR_ARG(all && lda >= D && users && pos && neg && contrib && ldc >= D && out, "null pointer or ld < 64");
  hipLaunchKernelGGL(lgm_reg_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (int)B, U, all, lda, users, pos, neg,
                     coef, contrib, ldc, out);
  GMR_LAUNCHED();
  return GMR_OK;
}
