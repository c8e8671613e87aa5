// SMORE (models/smore.py of the reference): the spectrum step with its three purifier gates, and the fuser, as
// row-local launches on the fp32 MFMA, with their backward.
//   spectrum   A = rfft(V), B = rfft(T) (norm 'ortho', 33 bins);  image_conv = irfft(A Wi), text_conv = irfft(B Wt),
//              fusion_conv = irfft(A B Wf);  Pv = E_i * sigmoid(gate_v(image_conv)), Pt, Pf likewise
//   fuser      sv = softmax_64(Wv2 tanh(Wv1 f + bv1)), st likewise;  gi, gt, gf = dropout(sigmoid(W. c + b.))
//              side = (gi sv a + gt st b + gf f) / 3;  all = c + side
//
// The 64-real layout of a spectrum row: column j <= 32 holds Re X_j, column j >= 33 holds Im X_(j - 32).  Im X_0 and
// Im X_32 of a real row's spectrum are zero and irfft ignores them, so they have no column: the forward transform
// S = x F^T (F[j][n] = cos(theta j n) / 8, -sin(theta (j - 32) n) / 8) and the inverse x = Y Gt^T (Gt[n][j] =
// c_j F[j][n], c = 1 for bins 0 and 32, else 2) are each one 64 x 64 real product, and a complex multiply is an
// element phase that reads a column's partner at j +- 32.  The backward runs on the same two matrices: the spectrum of
// an output gradient is g F^T, and c_k moves from Ybar = c_k G_k into the inverse product.  Im W_0 and Im W_32 of a
// filter are never read; their gradients are written as 0.
//
//   gmr_smore_spectrum_fwd / _bwd   two transforms + three inverses + three gates per row (backward: the same eight)
//   gmr_smore_fuse_fwd / _bwd       seven 64 x 64 products per row
//
// The scheme is csrc/row_tile.h's, shared with csrc/mgcn.hip: a workgroup of four waves stages the weights in LDS once
// (stride 68) and loops over 16-row tiles with a capped grid; in the element phases thread tid owns row tid >> 4,
// columns 4 (tid & 15) .. + 3; in the MFMA phases (v_mfma_f32_16x16x4_f32) wave w computes the output columns
// 16 w .. 16 w + 15.  Five (spectrum) or seven (fuser) staged matrices are 87 KB / 122 KB, over the 64 KB static limit
// and inside the 160 KiB of a CU: the kernels take dynamic LDS (hipFuncSetAttribute) and run one workgroup per CU.
//
// No float atomics; a row's result depends on its own inputs and the weights only.  The complex-weight gradients are
// per-tile column sums in a workspace (row order), summed by a second pass (a workgroup per filter) in a fixed fp64
// order that does not depend on the grid.
#include <mutex>

#include "row_tile.h"

namespace {

using namespace gmr_row;  // D, TR, LDX, the element helpers, mm16c / put16c / stage_w (csrc/row_tile.h)
using gmr::f4_add;
constexpr int MAX_BLOCKS = 256;  // one workgroup per CU
constexpr int WMAT = D * LDX, TILE = TR * LDX;
constexpr int SPEC_FWD_LDS = (5 * WMAT + 3 * TILE + 6 * D) * 4;
constexpr int SPEC_BWD_LDS = (5 * WMAT + 8 * TILE + 6 * D) * 4;
constexpr int FUSE_LDS = (7 * WMAT + 5 * TILE) * 4;
constexpr uint64_t SITE_MIX = 0x9E3779B97F4A7C15ull;
constexpr uint64_t SITE_GATES = 0x534D4F52ull;  // the three preference gates: sites SITE_GATES + 0, 1, 2

__device__ __forceinline__ float row16_max(float v) {
#pragma unroll
  for (int m = 8; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
  return v;
}
__device__ __forceinline__ float4 zero_f4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// ------------------------------------------------------------------------------------------------ twiddles
// [0]: F[j][n], the forward transform; [1]: Gt[n][j] = c_j F[j][n], the inverse.  Written once per device by
// twiddle_kernel (cospi / sinpi in double on the reduced angle index, rounded once).
__device__ __attribute__((aligned(16))) float g_tw[2][D * D];

__global__ void twiddle_kernel() {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D * D) return;
  const int j = i >> 6, n = i & 63;
  const int k = j <= 32 ? j : j - 32;
  const int m = (k * n) & 63;  // theta k n = 2 pi m / 64
  const double v = j <= 32 ? cospi(m / 32.0) : -sinpi(m / 32.0);
  const float f = (float)(v * 0.125);
  g_tw[0][j * D + n] = f;
  g_tw[1][n * D + j] = (k == 0 || k == 32) ? f : 2.f * f;
}

// bin k(j) of a spectrum row in the 64-real layout
__device__ __forceinline__ void bin(const float* row, int j, float& re, float& im) {
  const int k = j <= 32 ? j : j - 32;
  re = row[k];
  im = (k == 0 || k == 32) ? 0.f : row[k + 32];
}
// column j of x w and of g conj(x)
__device__ __forceinline__ float cmul_col(int j, float xr, float xi, float wr, float wi) {
  return j <= 32 ? xr * wr - xi * wi : xr * wi + xi * wr;
}
__device__ __forceinline__ float cconj_col(int j, float gr, float gi, float xr, float xi) {
  return j <= 32 ? gr * xr + gi * xi : gi * xr - gr * xi;
}
// the three filters by column: sC[2 f][j] = Re W_k, sC[2 f + 1][j] = Im W_k (0 for k = 0, 32)
__device__ __forceinline__ void stage_filters(float* sC, const float* Wi, const float* Wt, const float* Wf) {
  const int tid = threadIdx.x;
  if (tid < 3 * D) {
    const int f = tid >> 6, j = tid & 63, k = j <= 32 ? j : j - 32;
    const float* W = f == 0 ? Wi : f == 1 ? Wt : Wf;
    sC[(2 * f) * D + j] = W[2 * k];
    sC[(2 * f + 1) * D + j] = (k == 0 || k == 32) ? 0.f : W[2 * k + 1];
  }
}

// ------------------------------------------------------------------------------------------------ spectrum
struct SpecArgs {
  int64_t n;
  const float *V, *T, *E;
  int64_t ldv, ldt, lde;
  const float *Wi, *Wt, *Wf;  // 33 x 2 each
  const float *Wgv, *bgv, *Wgt, *bgt, *Wgf, *bgf;
  int64_t ldw;
  float* S;  // [A | B]
  int64_t ldsp;
  float* conv;  // [image_conv | text_conv | fusion_conv]
  int64_t ldcv;
  float* g;  // the three gate rows
  int64_t ldg;
  float* P;  // [Pv | Pt | Pf]
  int64_t ldp;
};

__global__ __launch_bounds__(256) void smore_spectrum_fwd_kernel(SpecArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *sF = lds, *sG = lds + WMAT;
  float* sW[3] = {lds + 2 * WMAT, lds + 3 * WMAT, lds + 4 * WMAT};
  float* sX[3] = {lds + 5 * WMAT, lds + 5 * WMAT + TILE, lds + 5 * WMAT + 2 * TILE};
  float* sC = lds + 5 * WMAT + 3 * TILE;
  const int tid = threadIdx.x, w = tid >> 6;
  stage_w(sF, g_tw[0], D, false);
  stage_w(sG, g_tw[1], D, false);
  stage_w(sW[0], a.Wgv, a.ldw, false);
  stage_w(sW[1], a.Wgt, a.ldw, false);
  stage_w(sW[2], a.Wgf, a.ldw, false);
  stage_filters(sC, a.Wi, a.Wt, a.Wf);
  const int row = tid >> 4, c = (tid & 15) * 4;
  float* mine[3] = {sX[0] + row * LDX + c, sX[1] + row * LDX + c, sX[2] + row * LDX + c};
  const float* bias[3] = {a.bgv, a.bgt, a.bgf};
  const int64_t ntiles = (a.n + TR - 1) / TR;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t gr = t * TR + row;
    const bool ok = gr < a.n;
    st4(mine[0], ok ? ld4(a.V + gr * a.ldv + c) : zero_f4());  // tail rows: zeros, never stored
    st4(mine[1], ok ? ld4(a.T + gr * a.ldt + c) : zero_f4());
    __syncthreads();
    floatx4 p0 = zero4(), p1 = zero4(), p2 = zero4();
    mm16c(sX[0], sF, w, p0);
    mm16c(sX[1], sF, w, p1);
    __syncthreads();
    put16c(sX[0], w, p0, nullptr);
    put16c(sX[1], w, p1, nullptr);
    __syncthreads();
    // the three spectral products on this thread's four columns
    const float *ra = sX[0] + row * LDX, *rb = sX[1] + row * LDX;
    float y[3][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = c + e;
      float ar, ai, br, bi;
      bin(ra, j, ar, ai);
      bin(rb, j, br, bi);
      y[0][e] = cmul_col(j, ar, ai, sC[j], sC[D + j]);
      y[1][e] = cmul_col(j, br, bi, sC[2 * D + j], sC[3 * D + j]);
      const float pr = ar * br - ai * bi, pi = ar * bi + ai * br;
      y[2][e] = cmul_col(j, pr, pi, sC[4 * D + j], sC[5 * D + j]);
    }
    if (ok) {
      st4(a.S + gr * a.ldsp + c, ld4(mine[0]));
      st4(a.S + gr * a.ldsp + D + c, ld4(mine[1]));
    }
    __syncthreads();
#pragma unroll
    for (int f = 0; f < 3; ++f) st4(mine[f], make_float4(y[f][0], y[f][1], y[f][2], y[f][3]));
    __syncthreads();
    p0 = zero4(), p1 = zero4(), p2 = zero4();
    mm16c(sX[0], sG, w, p0);
    mm16c(sX[1], sG, w, p1);
    mm16c(sX[2], sG, w, p2);
    __syncthreads();
    put16c(sX[0], w, p0, nullptr);
    put16c(sX[1], w, p1, nullptr);
    put16c(sX[2], w, p2, nullptr);
    __syncthreads();
    if (ok) {
#pragma unroll
      for (int f = 0; f < 3; ++f) st4(a.conv + gr * a.ldcv + f * D + c, ld4(mine[f]));
    }
    p0 = zero4(), p1 = zero4(), p2 = zero4();
    mm16c(sX[0], sW[0], w, p0);
    mm16c(sX[1], sW[1], w, p1);
    mm16c(sX[2], sW[2], w, p2);
    __syncthreads();
    put16c(sX[0], w, p0, bias[0]);
    put16c(sX[1], w, p1, bias[1]);
    put16c(sX[2], w, p2, bias[2]);
    __syncthreads();
    if (ok) {
      const float4 e = ld4(a.E + gr * a.lde + c);
#pragma unroll
      for (int f = 0; f < 3; ++f) {
        const float4 g = sigm4(ld4(mine[f]));
        st4(a.g + gr * a.ldg + f * D + c, g);
        st4(a.P + gr * a.ldp + f * D + c, mul4(e, g));
      }
    }
    // the next tile's staging writes the floats this thread just read
  }
}

struct SpecBwdArgs {
  int64_t n;
  const float* dP;
  int64_t lddp;
  const float* g;
  int64_t ldg;
  const float* E;
  int64_t lde;
  const float* S;
  int64_t ldsp;
  const float *Wi, *Wt, *Wf;
  const float *Wgv, *Wgt, *Wgf;
  int64_t ldw;
  float* dE;
  int64_t ldde;
  int accumulate;
  float* z;  // [zv | zt | zf]
  int64_t ldz;
  float *dV, *dT;
  int64_t lddv;
  float* ws;  // [tile][3][64]
};

__global__ __launch_bounds__(256) void smore_spectrum_bwd_kernel(SpecBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *sF = lds, *sG = lds + WMAT;
  float* sW[3] = {lds + 2 * WMAT, lds + 3 * WMAT, lds + 4 * WMAT};
  float* base = lds + 5 * WMAT;
  float* sX[3] = {base, base + TILE, base + 2 * TILE};
  float* sP[3] = {base + 3 * TILE, base + 4 * TILE, base + 5 * TILE};  // the rows' shares of the filter gradients
  float* sS[2] = {base + 6 * TILE, base + 7 * TILE};                   // the saved spectra A, B
  float* sC = base + 8 * TILE;
  const int tid = threadIdx.x, w = tid >> 6;
  stage_w(sF, g_tw[0], D, false);
  stage_w(sG, g_tw[1], D, false);
  stage_w(sW[0], a.Wgv, a.ldw, true);
  stage_w(sW[1], a.Wgt, a.ldw, true);
  stage_w(sW[2], a.Wgf, a.ldw, true);
  stage_filters(sC, a.Wi, a.Wt, a.Wf);
  const int row = tid >> 4, c = (tid & 15) * 4;
  const int off = row * LDX + c;
  const int64_t ntiles = (a.n + TR - 1) / TR;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t gr = t * TR + row;
    const bool ok = gr < a.n;
    float4 zz[3] = {zero_f4(), zero_f4(), zero_f4()};
    float4 sa = zero_f4(), sb = zero_f4();
    if (ok) {
      const float4 e = ld4(a.E + gr * a.lde + c);
      float4 de = a.accumulate ? ld4(a.dE + gr * a.ldde + c) : zero_f4();
      float4 sum = zero_f4();
#pragma unroll
      for (int f = 0; f < 3; ++f) {
        const float4 dp = ld4(a.dP + gr * a.lddp + f * D + c), g = ld4(a.g + gr * a.ldg + f * D + c);
        sum = f == 0 ? mul4(dp, g) : f4_add(sum, mul4(dp, g));
        zz[f] = mul4(mul4(dp, e), dsig4(g));
        st4(a.z + gr * a.ldz + f * D + c, zz[f]);
      }
      st4(a.dE + gr * a.ldde + c, a.accumulate ? f4_add(sum, de) : sum);
      sa = ld4(a.S + gr * a.ldsp + c);
      sb = ld4(a.S + gr * a.ldsp + D + c);
    }
#pragma unroll
    for (int f = 0; f < 3; ++f) st4(sX[f] + off, zz[f]);
    st4(sS[0] + off, sa);
    st4(sS[1] + off, sb);
    __syncthreads();
    floatx4 p0 = zero4(), p1 = zero4(), p2 = zero4();
    mm16c(sX[0], sW[0], w, p0);  // d conv = z Wg
    mm16c(sX[1], sW[1], w, p1);
    mm16c(sX[2], sW[2], w, p2);
    __syncthreads();
    put16c(sX[0], w, p0, nullptr);
    put16c(sX[1], w, p1, nullptr);
    put16c(sX[2], w, p2, nullptr);
    __syncthreads();
    p0 = zero4(), p1 = zero4(), p2 = zero4();
    mm16c(sX[0], sF, w, p0);  // G = rfft(d conv)
    mm16c(sX[1], sF, w, p1);
    mm16c(sX[2], sF, w, p2);
    __syncthreads();
    put16c(sX[0], w, p0, nullptr);
    put16c(sX[1], w, p1, nullptr);
    put16c(sX[2], w, p2, nullptr);
    __syncthreads();
    const float *gi_ = sX[0] + row * LDX, *gt_ = sX[1] + row * LDX, *gf_ = sX[2] + row * LDX;
    const float *ra = sS[0] + row * LDX, *rb = sS[1] + row * LDX;
    float xa[4], xb[4], ci[4], ct[4], cf[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = c + e;
      float gir, gii, gtr, gti, gfr, gfi, ar, ai, br, bi;
      bin(gi_, j, gir, gii);
      bin(gt_, j, gtr, gti);
      bin(gf_, j, gfr, gfi);
      bin(ra, j, ar, ai);
      bin(rb, j, br, bi);
      const float wfr = sC[4 * D + j], wfi = sC[5 * D + j];
      const float qbr = br * wfr - bi * wfi, qbi = br * wfi + bi * wfr;  // B Wf
      const float qar = ar * wfr - ai * wfi, qai = ar * wfi + ai * wfr;  // A Wf
      const float pr = ar * br - ai * bi, pi = ar * bi + ai * br;        // A B
      xa[e] = cconj_col(j, gir, gii, sC[j], sC[D + j]) + cconj_col(j, gfr, gfi, qbr, qbi);
      xb[e] = cconj_col(j, gtr, gti, sC[2 * D + j], sC[3 * D + j]) + cconj_col(j, gfr, gfi, qar, qai);
      ci[e] = cconj_col(j, gir, gii, ar, ai);
      ct[e] = cconj_col(j, gtr, gti, br, bi);
      cf[e] = cconj_col(j, gfr, gfi, pr, pi);
    }
    __syncthreads();
    st4(sX[0] + off, make_float4(xa[0], xa[1], xa[2], xa[3]));
    st4(sX[1] + off, make_float4(xb[0], xb[1], xb[2], xb[3]));
    st4(sP[0] + off, make_float4(ci[0], ci[1], ci[2], ci[3]));
    st4(sP[1] + off, make_float4(ct[0], ct[1], ct[2], ct[3]));
    st4(sP[2] + off, make_float4(cf[0], cf[1], cf[2], cf[3]));
    __syncthreads();
    p0 = zero4(), p1 = zero4();
    mm16c(sX[0], sG, w, p0);  // dV, dT: the inverse product carries c_k
    mm16c(sX[1], sG, w, p1);
    if (tid < 3 * D) {  // the tile's column sums, rows in order
      const int f = tid >> 6, j = tid & 63;
      float s = 0.f;
#pragma unroll
      for (int r = 0; r < TR; ++r) s += sP[f][r * LDX + j];
      a.ws[(t * 3 + f) * D + j] = s;
    }
    __syncthreads();
    put16c(sX[0], w, p0, nullptr);
    put16c(sX[1], w, p1, nullptr);
    __syncthreads();
    if (ok) {
      st4(a.dV + gr * a.lddv + c, ld4(sX[0] + off));
      st4(a.dT + gr * a.lddv + c, ld4(sX[1] + off));
    }
  }
}

// dW (3 x 33 x 2) from the per-tile column sums, one workgroup per filter: sixteen slices of tiles (tile mod 16) summed
// in tile order in fp64, then one fixed tree over the slices; a tile of zeros leaves the bits as they are.  c_k is
// applied here; Im dW_0 = Im dW_32 = 0.
constexpr int RED_SLICES = 16;
__global__ __launch_bounds__(RED_SLICES * D) void smore_dw_reduce_kernel(int64_t ntiles, const float* __restrict__ ws,
                                                                         float* __restrict__ dWi,
                                                                         float* __restrict__ dWt,
                                                                         float* __restrict__ dWf) {
  __shared__ double s[RED_SLICES][D];
  const int f = blockIdx.x, j = threadIdx.x & 63, sl = threadIdx.x >> 6;
  double acc = 0.0;
#pragma unroll 4
  for (int64_t i = sl; i < ntiles; i += RED_SLICES) acc += (double)ws[(i * 3 + f) * D + j];
  s[sl][j] = acc;
  __syncthreads();
  for (int off = RED_SLICES / 2; off >= 1; off >>= 1) {
    if (sl < off) s[sl][j] += s[sl + off][j];
    __syncthreads();
  }
  if (sl == 0) {
    const int k = j <= 32 ? j : j - 32;
    float* out = f == 0 ? dWi : f == 1 ? dWt : dWf;
    const double ck = (k == 0 || k == 32) ? 1.0 : 2.0;
    out[2 * k + (j <= 32 ? 0 : 1)] = (float)(ck * s[0][j]);
    if (j == 0 || j == 32) out[2 * j + 1] = 0.f;
  }
}

// ------------------------------------------------------------------------------------------------ fuser
struct FuseArgs {
  int64_t n;
  const float* abf;  // [a | b | f]
  int64_t ldabf;
  const float* c;
  int64_t ldc;
  const float *Wv1, *bv1, *Wv2, *Wt1, *bt1, *Wt2, *Wi, *bi, *Wt, *bt, *Wf, *bf;
  int64_t ldw;
  float p;
  int drop;             // 0 none, 1 keep bytes given, 2 drawn
  const uint8_t* keep;  // n x 192 bytes [image | text | fusion]
  int64_t ldk;
  uint64_t seed, step;
  float *side, *all;
  int64_t ldo;
  float* saved;  // [hv | ht | sv | st | gi | gt | gf]
  int64_t lds;
};

__device__ __forceinline__ float4 softmax_row(float4 x) {
  const float mx = row16_max(fmaxf(fmaxf(x.x, x.y), fmaxf(x.z, x.w)));
  const float4 e = make_float4(expf(x.x - mx), expf(x.y - mx), expf(x.z - mx), expf(x.w - mx));
  const float s = row16_sum((e.x + e.y) + (e.z + e.w));
  return make_float4(e.x / s, e.y / s, e.z / s, e.w / s);
}

__global__ __launch_bounds__(256) void smore_fuse_fwd_kernel(FuseArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* sW[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) sW[i] = lds + i * WMAT;
  float* sX[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) sX[i] = lds + 7 * WMAT + i * TILE;
  const int tid = threadIdx.x, w = tid >> 6;
  stage_w(sW[0], a.Wv1, a.ldw, false);
  stage_w(sW[1], a.Wv2, a.ldw, false);
  stage_w(sW[2], a.Wt1, a.ldw, false);
  stage_w(sW[3], a.Wt2, a.ldw, false);
  stage_w(sW[4], a.Wi, a.ldw, false);
  stage_w(sW[5], a.Wt, a.ldw, false);
  stage_w(sW[6], a.Wf, a.ldw, false);
  const int row = tid >> 4, c = (tid & 15) * 4;
  const int off = row * LDX + c;
  const float p_keep = 1.f - a.p, scale = 1.f / (1.f - a.p);
  const int64_t ntiles = (a.n + TR - 1) / TR;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t gr = t * TR + row;
    const bool ok = gr < a.n;
    float4 xa = zero_f4(), xb = zero_f4(), xf = zero_f4(), xc = zero_f4();
    if (ok) {
      xa = ld4(a.abf + gr * a.ldabf + c);
      xb = ld4(a.abf + gr * a.ldabf + D + c);
      xf = ld4(a.abf + gr * a.ldabf + 2 * D + c);
      xc = ld4(a.c + gr * a.ldc + c);
    }
    st4(sX[0] + off, xf);
    st4(sX[1] + off, xc);
    __syncthreads();
    floatx4 p0 = zero4(), p1 = zero4(), p2 = zero4(), p3 = zero4(), p4 = zero4();
    mm16c(sX[0], sW[0], w, p0);
    mm16c(sX[0], sW[2], w, p1);
    mm16c(sX[1], sW[4], w, p2);
    mm16c(sX[1], sW[5], w, p3);
    mm16c(sX[1], sW[6], w, p4);
    __syncthreads();
    put16c(sX[0], w, p0, a.bv1);
    put16c(sX[1], w, p1, a.bt1);
    put16c(sX[2], w, p2, a.bi);
    put16c(sX[3], w, p3, a.bt);
    put16c(sX[4], w, p4, a.bf);
    __syncthreads();
    const float4 hv = tanh4(ld4(sX[0] + off)), ht = tanh4(ld4(sX[1] + off));
    float4 g[3] = {sigm4(ld4(sX[2] + off)), sigm4(ld4(sX[3] + off)), sigm4(ld4(sX[4] + off))};
    st4(sX[0] + off, hv);  // this thread's own floats: nobody else reads them before the barrier
    st4(sX[1] + off, ht);
    __syncthreads();
    p0 = zero4(), p1 = zero4();
    mm16c(sX[0], sW[1], w, p0);
    mm16c(sX[1], sW[3], w, p1);
    __syncthreads();
    put16c(sX[0], w, p0, nullptr);
    put16c(sX[1], w, p1, nullptr);
    __syncthreads();
    const float4 sv = softmax_row(ld4(sX[0] + off)), st = softmax_row(ld4(sX[1] + off));
    if (ok) {
      if (a.drop) {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          uint32_t bits;
          if (a.drop == 1) {
            const uint8_t* kp = a.keep + gr * a.ldk + s * D + c;
            bits = (kp[0] ? 1u : 0u) | (kp[1] ? 2u : 0u) | (kp[2] ? 4u : 0u) | (kp[3] ? 8u : 0u);
          } else {
            const uint4 r = gmr::Philox::gen(a.seed + (SITE_GATES + (uint64_t)s) * SITE_MIX, a.step,
                                             (uint64_t)gr * 16 + (uint64_t)(c >> 2));
            const float k24 = 1.0f / 16777216.0f;
            bits = ((float)(r.x >> 8) * k24 < p_keep ? 1u : 0u) | ((float)(r.y >> 8) * k24 < p_keep ? 2u : 0u) |
                   ((float)(r.z >> 8) * k24 < p_keep ? 4u : 0u) | ((float)(r.w >> 8) * k24 < p_keep ? 8u : 0u);
          }
          g[s] = make_float4(bits & 1u ? g[s].x * scale : 0.f, bits & 2u ? g[s].y * scale : 0.f,
                             bits & 4u ? g[s].z * scale : 0.f, bits & 8u ? g[s].w * scale : 0.f);
        }
      }
      const float4 s3 = f4_add(f4_add(mul4(mul4(g[0], sv), xa), mul4(mul4(g[1], st), xb)), mul4(g[2], xf));
      const float4 side = make_float4(s3.x / 3.f, s3.y / 3.f, s3.z / 3.f, s3.w / 3.f);
      st4(a.side + gr * a.ldo + c, side);
      st4(a.all + gr * a.ldo + c, f4_add(xc, side));
      float* sv_ = a.saved + gr * a.lds + c;
      st4(sv_, hv);
      st4(sv_ + D, ht);
      st4(sv_ + 2 * D, sv);
      st4(sv_ + 3 * D, st);
      st4(sv_ + 4 * D, g[0]);
      st4(sv_ + 5 * D, g[1]);
      st4(sv_ + 6 * D, g[2]);
    }
  }
}

struct FuseBwdArgs {
  int64_t n;
  const float* dall;
  int64_t ldda;
  const float *dside, *dcin;  // either may be null (zero)
  int64_t ldds;
  const float* abf;
  int64_t ldabf;
  const float* saved;
  int64_t lds;
  float p;
  const float *Wv1, *Wv2, *Wt1, *Wt2, *Wi, *Wt, *Wf;
  int64_t ldw;
  float* dabf;  // [da | db | df]
  int64_t lddabf;
  float* dc;
  int64_t lddc;
  float* z;  // [z1v | z2v | z1t | z2t | zi | zt | zf]
  int64_t ldz;
};

// the gradient of a masked gate row m = keep sigmoid(y) / (1 - p) with respect to y, times dm: a dropped entry has
// m = 0 and gets 0; a kept one has sigmoid = m (1 - p)
__device__ __forceinline__ float4 dgate4(float4 dm, float4 m, float p_keep, float scale) {
  const float4 s = gmr::f4_scale(p_keep, m);
  return gmr::f4_scale(scale, mul4(dm, dsig4(s)));
}

__global__ __launch_bounds__(256) void smore_fuse_bwd_kernel(FuseBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* sW[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) sW[i] = lds + i * WMAT;
  float* sX[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) sX[i] = lds + 7 * WMAT + i * TILE;
  const int tid = threadIdx.x, w = tid >> 6;
  stage_w(sW[0], a.Wv1, a.ldw, true);
  stage_w(sW[1], a.Wv2, a.ldw, true);
  stage_w(sW[2], a.Wt1, a.ldw, true);
  stage_w(sW[3], a.Wt2, a.ldw, true);
  stage_w(sW[4], a.Wi, a.ldw, true);
  stage_w(sW[5], a.Wt, a.ldw, true);
  stage_w(sW[6], a.Wf, a.ldw, true);
  const int row = tid >> 4, c = (tid & 15) * 4;
  const int off = row * LDX + c;
  const float p_keep = 1.f - a.p, scale = 1.f / (1.f - a.p);
  const int64_t ntiles = (a.n + TR - 1) / TR;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t gr = t * TR + row;
    const bool ok = gr < a.n;
    const float4 z0 = zero_f4();
    float4 da = z0, db = z0, df = z0, dc = z0, zi = z0, zt = z0, zf = z0, dsv = z0, dst = z0, sv = z0, st = z0;
    float4 hv = z0, ht = z0;
    if (ok) {
      const float4 g = ld4(a.dall + gr * a.ldda + c);
      const float4 ds = a.dside ? f4_add(g, ld4(a.dside + gr * a.ldds + c)) : g;
      dc = a.dcin ? f4_add(g, ld4(a.dcin + gr * a.ldds + c)) : g;
      const float4 s3 = make_float4(ds.x / 3.f, ds.y / 3.f, ds.z / 3.f, ds.w / 3.f);
      const float4 xa = ld4(a.abf + gr * a.ldabf + c), xb = ld4(a.abf + gr * a.ldabf + D + c);
      const float4 xf = ld4(a.abf + gr * a.ldabf + 2 * D + c);
      const float* sv_ = a.saved + gr * a.lds + c;
      hv = ld4(sv_);
      ht = ld4(sv_ + D);
      sv = ld4(sv_ + 2 * D);
      st = ld4(sv_ + 3 * D);
      const float4 mi = ld4(sv_ + 4 * D), mt = ld4(sv_ + 5 * D), mf = ld4(sv_ + 6 * D);
      da = mul4(s3, mul4(mi, sv));
      db = mul4(s3, mul4(mt, st));
      df = mul4(s3, mf);
      zi = dgate4(mul4(s3, mul4(sv, xa)), mi, p_keep, scale);
      zt = dgate4(mul4(s3, mul4(st, xb)), mt, p_keep, scale);
      zf = dgate4(mul4(s3, xf), mf, p_keep, scale);
      dsv = mul4(s3, mul4(mi, xa));
      dst = mul4(s3, mul4(mt, xb));
    }
    // softmax backward: z2 = s (ds - <ds, s>)
    const float iv = row16_sum(dot4(dsv, sv)), it = row16_sum(dot4(dst, st));
    const float4 z2v = mul4(sv, make_float4(dsv.x - iv, dsv.y - iv, dsv.z - iv, dsv.w - iv));
    const float4 z2t = mul4(st, make_float4(dst.x - it, dst.y - it, dst.z - it, dst.w - it));
    float* z_ = a.z + gr * a.ldz + c;
    if (ok) {
      st4(z_ + D, z2v);
      st4(z_ + 3 * D, z2t);
      st4(z_ + 4 * D, zi);
      st4(z_ + 5 * D, zt);
      st4(z_ + 6 * D, zf);
    }
    st4(sX[0] + off, z2v);
    st4(sX[1] + off, z2t);
    st4(sX[2] + off, zi);
    st4(sX[3] + off, zt);
    st4(sX[4] + off, zf);
    __syncthreads();
    floatx4 p0 = zero4(), p1 = zero4(), p2 = zero4();
    mm16c(sX[0], sW[1], w, p0);  // d hv = z2v Wv2
    mm16c(sX[1], sW[3], w, p1);
    mm16c(sX[2], sW[4], w, p2);  // d c += zi Wi + zt Wt + zf Wf
    mm16c(sX[3], sW[5], w, p2);
    mm16c(sX[4], sW[6], w, p2);
    __syncthreads();
    put16c(sX[0], w, p0, nullptr);
    put16c(sX[1], w, p1, nullptr);
    put16c(sX[2], w, p2, nullptr);
    __syncthreads();
    const float4 z1v = mul4(ld4(sX[0] + off), dtanh4(hv)), z1t = mul4(ld4(sX[1] + off), dtanh4(ht));
    if (ok) {
      st4(z_, z1v);
      st4(z_ + 2 * D, z1t);
      st4(a.dc + gr * a.lddc + c, f4_add(dc, ld4(sX[2] + off)));
    }
    st4(sX[0] + off, z1v);  // this thread's own floats
    st4(sX[1] + off, z1t);
    __syncthreads();
    p0 = zero4();
    mm16c(sX[0], sW[0], w, p0);  // d f += z1v Wv1 + z1t Wt1
    mm16c(sX[1], sW[2], w, p0);
    put16c(sX[3], w, p0, nullptr);  // a tile every wave has read before the last barrier
    __syncthreads();
    if (ok) {
      float* d_ = a.dabf + gr * a.lddabf + c;
      st4(d_, da);
      st4(d_ + D, db);
      st4(d_ + 2 * D, f4_add(df, ld4(sX[3] + off)));
    }
  }
}

inline unsigned tiles_grid(int64_t n) { return (unsigned)gmr::grid_for(n, TR, MAX_BLOCKS); }

// the twiddle matrices of the current device, written on first use; the kernels' LDS attributes are set with them
int prepare(const char* fn, hipStream_t st) {
  static std::mutex mu;
  static bool ready[64] = {};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return gmr::hip_status(fn, e);
  std::lock_guard<std::mutex> lock(mu);
  if (dev < 0 || dev >= 64) {
    gmr::set_error(fn, "device index out of range");
    return GMR_ERR_ARG;
  }
  if (ready[dev]) return GMR_OK;
  const struct {
    const void* f;
    int bytes;
  } attrs[] = {{(const void*)smore_spectrum_fwd_kernel, SPEC_FWD_LDS},
               {(const void*)smore_spectrum_bwd_kernel, SPEC_BWD_LDS},
               {(const void*)smore_fuse_fwd_kernel, FUSE_LDS},
               {(const void*)smore_fuse_bwd_kernel, FUSE_LDS}};
  for (const auto& at : attrs) {
    e = hipFuncSetAttribute(at.f, hipFuncAttributeMaxDynamicSharedMemorySize, at.bytes);
    if (e != hipSuccess) return gmr::hip_status(fn, e);
  }
  hipLaunchKernelGGL(twiddle_kernel, dim3(D * D / 256), dim3(256), 0, st);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // once: later calls may come on another stream
  if (e != hipSuccess) return gmr::hip_status(fn, e);
  ready[dev] = true;
  return GMR_OK;
}

}  // namespace

// ==================================================================================================== C ABI
extern "C" int32_t gmr_smore_tile_rows(void) { return TR; }
extern "C" int32_t gmr_smore_max_blocks(void) { return MAX_BLOCKS; }
extern "C" int64_t gmr_smore_spectrum_ws_floats(int64_t n) { return n < 1 ? 0 : (n + TR - 1) / TR * 3 * D; }

extern "C" int gmr_smore_twiddles(float* fwd, float* inv, void* stream) {
  GMR_ARG(fwd && inv, "null pointer");
  const int rc = prepare(__func__, (hipStream_t)stream);
  if (rc != GMR_OK) return rc;
  float* tw = nullptr;
  hipError_t e = hipGetSymbolAddress((void**)&tw, HIP_SYMBOL(g_tw));
  if (e == hipSuccess)
    e = hipMemcpyAsync(fwd, tw, sizeof(float) * D * D, hipMemcpyDeviceToDevice, (hipStream_t)stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(inv, tw + D * D, sizeof(float) * D * D, hipMemcpyDeviceToDevice, (hipStream_t)stream);
  if (e != hipSuccess) return gmr::hip_status(__func__, e);
  return GMR_OK;
}

extern "C" int gmr_smore_spectrum_fwd(int64_t n, const float* V, int64_t ldv, const float* T, int64_t ldt,
                                      const float* E, int64_t lde, const float* Wi, const float* Wt, const float* Wf,
                                      const float* Wgv, const float* bgv, const float* Wgt, const float* bgt,
                                      const float* Wgf, const float* bgf, int64_t ldw, float* S, int64_t ldsp,
                                      float* conv, int64_t ldcv, float* g, int64_t ldg, float* P, int64_t ldp,
                                      void* stream) {
  GMR_ARG(n >= 1 && n < (1ll << 31), "bad row count");
  GMR_ARG(Wi && Wt && Wf && bgv && bgt && bgf, "null pointer");
  GMR_ARG(rows16(V, ldv) && rows16(T, ldt) && rows16(E, lde) && rows16(Wgv, ldw) && rows16(Wgt, ldw) &&
              rows16(Wgf, ldw),
          "input rows must be 16-byte aligned with ld >= 64, ld % 4 == 0");
  GMR_ARG(rows16(S, ldsp, 2 * D) && rows16(conv, ldcv, 3 * D) && rows16(g, ldg, 3 * D) && rows16(P, ldp, 3 * D),
          "output rows must be 16-byte aligned (S: ld >= 128, conv, g, P: ld >= 192), ld % 4 == 0");
  const int rc = prepare(__func__, (hipStream_t)stream);
  if (rc != GMR_OK) return rc;
  SpecArgs a{n, V, T, E, ldv, ldt, lde, Wi, Wt, Wf, Wgv, bgv, Wgt, bgt, Wgf, bgf, ldw, S, ldsp, conv, ldcv, g, ldg,
             P, ldp};
  hipLaunchKernelGGL(smore_spectrum_fwd_kernel, dim3(tiles_grid(n)), dim3(256), SPEC_FWD_LDS, (hipStream_t)stream, a);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_smore_spectrum_bwd(int64_t n, const float* dP, int64_t lddp, const float* g, int64_t ldg,
                                      const float* E, int64_t lde, const float* S, int64_t ldsp, const float* Wi,
                                      const float* Wt, const float* Wf, const float* Wgv, const float* Wgt,
                                      const float* Wgf, int64_t ldw, float* dE, int64_t ldde, int32_t accumulate,
                                      float* z, int64_t ldz, float* dV, float* dT, int64_t lddv, float* ws,
                                      int64_t ws_floats, float* dWi, float* dWt, float* dWf, void* stream) {
  GMR_ARG(n >= 1 && n < (1ll << 31), "bad row count");
  GMR_ARG(Wi && Wt && Wf && dWi && dWt && dWf, "null pointer");
  GMR_ARG(ws && ws_floats >= gmr_smore_spectrum_ws_floats(n), "workspace: gmr_smore_spectrum_ws_floats(n) floats");
  GMR_ARG(rows16(dP, lddp, 3 * D) && rows16(g, ldg, 3 * D) && rows16(E, lde) && rows16(S, ldsp, 2 * D) &&
              rows16(Wgv, ldw) && rows16(Wgt, ldw) && rows16(Wgf, ldw),
          "input rows must be 16-byte aligned (dP, g: ld >= 192, S: ld >= 128, the others ld >= 64), ld % 4 == 0");
  GMR_ARG(rows16(dE, ldde) && rows16(z, ldz, 3 * D) && rows16(dV, lddv) && rows16(dT, lddv),
          "output rows must be 16-byte aligned (z: ld >= 192, the others ld >= 64), ld % 4 == 0");
  const int rc = prepare(__func__, (hipStream_t)stream);
  if (rc != GMR_OK) return rc;
  SpecBwdArgs a{n, dP, lddp, g, ldg, E, lde, S, ldsp, Wi, Wt, Wf, Wgv, Wgt, Wgf, ldw, dE, ldde, (int)accumulate, z,
                ldz, dV, dT, lddv, ws};
  hipLaunchKernelGGL(smore_spectrum_bwd_kernel, dim3(tiles_grid(n)), dim3(256), SPEC_BWD_LDS, (hipStream_t)stream, a);
  GMR_LAUNCHED();
  hipLaunchKernelGGL(smore_dw_reduce_kernel, dim3(3), dim3(RED_SLICES * D), 0, (hipStream_t)stream, (n + TR - 1) / TR,
                     ws, dWi, dWt, dWf);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_smore_fuse_fwd(int64_t n, const float* abf, int64_t ldabf, const float* c, int64_t ldc,
                                  const float* Wv1, const float* bv1, const float* Wv2, const float* Wt1,
                                  const float* bt1, const float* Wt2, const float* Wi, const float* bi, const float* Wt,
                                  const float* bt, const float* Wf, const float* bf, int64_t ldw, float p,
                                  int32_t drop_mode, const uint8_t* keep, int64_t ldk, uint64_t seed, uint64_t step,
                                  float* side, float* all, int64_t ldo, float* saved, int64_t lds, void* stream) {
  GMR_ARG(n >= 1 && n < (1ll << 31), "bad row count");
  GMR_ARG(bv1 && bt1 && bi && bt && bf, "null pointer");
  GMR_ARG(p >= 0.f && p < 1.f && drop_mode >= 0 && drop_mode <= 2, "dropout: 0 <= p < 1, mode 0, 1 or 2");
  GMR_ARG(drop_mode != 1 || (keep && ldk >= 3 * D), "given keep bytes: n x 192, ldk >= 192");
  GMR_ARG(rows16(abf, ldabf, 3 * D) && rows16(c, ldc) && rows16(Wv1, ldw) && rows16(Wv2, ldw) && rows16(Wt1, ldw) &&
              rows16(Wt2, ldw) && rows16(Wi, ldw) && rows16(Wt, ldw) && rows16(Wf, ldw),
          "input rows must be 16-byte aligned (abf: ld >= 192, the others ld >= 64), ld % 4 == 0");
  GMR_ARG(rows16(side, ldo) && rows16(all, ldo) && rows16(saved, lds, 7 * D),
          "output rows must be 16-byte aligned (saved: ld >= 448, the others ld >= 64), ld % 4 == 0");
  const int rc = prepare(__func__, (hipStream_t)stream);
  if (rc != GMR_OK) return rc;
  FuseArgs a{n, abf, ldabf, c, ldc, Wv1, bv1, Wv2, Wt1, bt1, Wt2, Wi, bi, Wt, bt, Wf, bf, ldw, p,
             p > 0.f ? (int)drop_mode : 0, keep, ldk, seed, step, side, all, ldo, saved, lds};
  hipLaunchKernelGGL(smore_fuse_fwd_kernel, dim3(tiles_grid(n)), dim3(256), FUSE_LDS, (hipStream_t)stream, a);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_smore_fuse_bwd(int64_t n, const float* dall, int64_t ldda, const float* dside, const float* dcin,
                                  int64_t ldds, const float* abf, int64_t ldabf, const float* saved, int64_t lds,
                                  float p, const float* Wv1, const float* Wv2, const float* Wt1, const float* Wt2,
                                  const float* Wi, const float* Wt, const float* Wf, int64_t ldw, float* dabf,
                                  int64_t lddabf, float* dc, int64_t lddc, float* z, int64_t ldz, void* stream) {
  GMR_ARG(n >= 1 && n < (1ll << 31), "bad row count");
  GMR_ARG(p >= 0.f && p < 1.f, "dropout: 0 <= p < 1");
  GMR_ARG(rows16(dall, ldda) && (!dside || rows16(dside, ldds)) && (!dcin || rows16(dcin, ldds)) &&
              rows16(abf, ldabf, 3 * D) && rows16(saved, lds, 7 * D) && rows16(Wv1, ldw) && rows16(Wv2, ldw) &&
              rows16(Wt1, ldw) && rows16(Wt2, ldw) && rows16(Wi, ldw) && rows16(Wt, ldw) && rows16(Wf, ldw),
          "input rows must be 16-byte aligned (abf: ld >= 192, saved: ld >= 448, the others ld >= 64), ld % 4 == 0");
  GMR_ARG(rows16(dabf, lddabf, 3 * D) && rows16(dc, lddc) && rows16(z, ldz, 7 * D),
          "output rows must be 16-byte aligned (dabf: ld >= 192, z: ld >= 448, dc: ld >= 64), ld % 4 == 0");
  const int rc = prepare(__func__, (hipStream_t)stream);
  if (rc != GMR_OK) return rc;
  FuseBwdArgs a{n, dall, ldda, dside, dcin, ldds, abf, ldabf, saved, lds, p, Wv1, Wv2, Wt1, Wt2, Wi, Wt, Wf, ldw,
                dabf, lddabf, dc, lddc, z, ldz};
  hipLaunchKernelGGL(smore_fuse_bwd_kernel, dim3(tiles_grid(n)), dim3(256), FUSE_LDS, (hipStream_t)stream, a);
  GMR_LAUNCHED();
  return GMR_OK;
}
