// GRCN (models/grcn.py of the reference): edge-softmax routing and graph refining on the user-item lists.
//
// Per modality m (M <= 2): f (I x 64) the normalised item rows, p^r (U x 64) the user preference rows after r routing
// rounds.  The train graph comes as the users' CSR (rowptr, col: items) and the items' CSC (trp, tcol: users) with the
// position maps csr2csc / csc2csr between the two list orders.  An attention row of destination x_d over its list:
//   s_k = <x_d, x_k>, alpha = softmax_k(s) (the maximum subtracted), h = sum_k alpha_k x_k
// and its backward from dh and dalpha: t_k = dalpha_k + <dh, x_k>, ds_k = alpha_k (t_k - sum_l alpha_l t_l),
//   dx_d += sum_k ds_k x_k  (the destination pass),  dx_k += alpha_k dh + ds_k x_d  (the source pass, over the
//   transposed list, a gather through the position map).
// Per-edge arrays of the 2E directed edges are laid out [user-destination, CSR order | item-destination, CSC order],
// one such array per modality (stride 2E).
//
//   gmr_grcn_route_fwd      p^1 .. p^R of all users, both modalities     a wave per user, the row in registers
//   gmr_grcn_attn_fwd       rep = x + h and alpha, both sides            a wave per destination row
//   gmr_grcn_refine_fwd     w = relu(max_m alpha_m conf[src, m]), arg    a thread per directed edge
//   gmr_grcn_dw             dw_e = <x[s], dx1[d]> + <x1[s], g[d]>        a wave per destination row
//   gmr_grcn_refine_bwd     dalpha and dconf                             a wave per source node, its own edge list
//   gmr_grcn_attn_bwd_dst   ds and dx_d of the final layer               a wave per destination row
//   gmr_grcn_route_bwd_dst  the R rounds in reverse: alpha^r, ds^r, dy^r, d preference     a wave per user
//   gmr_grcn_bwd_src        dx_k summed over a node's transposed list and over up to 8 (alpha, ds) terms
//   gmr_grcn_loss_rows      the BPR and regulariser rows at 128 / 192 columns
//
// A wave holds a destination row four times (a float4 per lane, 16 lanes per copy); quarter q takes the neighbours q,
// q + 4, ... of the list, so a 256-byte neighbour row is one float4 load per lane.  No float atomics: every sum is a
// per-quarter chain in list order followed by two xor steps, so the result depends on the row's own list only and any
// grid gives the same bits.  A list longer than a wave's trip (a hub item) is a longer loop of the same wave.
#include <math.h>

#include "gmr_common.h"

namespace {

constexpr int D = 64, MAXR = 7, MAXT = 8, MAX_BLOCKS = 4096;

using gmr::ld4, gmr::st4, gmr::f4_fma, gmr::f4_add, gmr::f4_scale, gmr::shfl_xor_f4;
// one fixed fma chain
__device__ __forceinline__ float dot4(float4 a, float4 b) {
  return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)));
}
__device__ __forceinline__ float row16_sum(float v) {
#pragma unroll
  for (int m = 8; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
// across the four quarters of a wave: the same bits in every lane
__device__ __forceinline__ float q4_sum(float v) {
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}
__device__ __forceinline__ float q4_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16));
  return fmaxf(v, __shfl_xor(v, 32));
}
__device__ __forceinline__ float4 q4_sum4(float4 v) {
  v = f4_add(v, shfl_xor_f4(v, 16));
  return f4_add(v, shfl_xor_f4(v, 32));
}
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 div4(float4 a, float d) { return make_float4(a.x / d, a.y / d, a.z / d, a.w / d); }
__device__ __forceinline__ float4 sub4(float4 a, float4 b) {
  return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
}

// The loops over a list run the same trips in every quarter (k0 = 0, 4, ...); a quarter past the end reads the last
// entry again and drops the result, so the shuffles inside always see whole waves.
#define GRCN_FOR_LIST(deg)                   \
  for (int k0 = 0; k0 < (deg); k0 += 4) {    \
    const int k = k0 + qw;                   \
    const bool ok = k < (deg);               \
    const int kk = ok ? k : (deg) - 1;
#define GRCN_END }

// the largest score of the row over its list (deg >= 1)
__device__ __forceinline__ float score_max(float4 xd, const float* __restrict__ Xs, int64_t lds,
                                           const int32_t* __restrict__ list, int deg, int qw, int c) {
  float mx = -INFINITY;
  GRCN_FOR_LIST(deg)
    const float s = row16_sum(dot4(xd, ld4(Xs + (int64_t)list[kk] * lds + c)));
    if (ok) mx = fmaxf(mx, s);
  GRCN_END
  return q4_max(mx);
}

// ------------------------------------------------------------------------------------------------ routing forward
struct RouteFwdArgs {
  int64_t U;
  int R, M, messages;
  const int32_t *rowptr, *col;
  const float* F;
  int64_t ldf;
  float* P;  // (R + 1) tables of U x 64 M, table stride pstride; table 0 is read
  int64_t ldp, pstride;
  float* nrmY;  // R x M x U
};

__global__ __launch_bounds__(256) void grcn_route_fwd_kernel(RouteFwdArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, qw = lane >> 4, c = (lane & 15) * 4;
  for (int64_t u = (int64_t)blockIdx.x * 4 + wv; u < a.U; u += (int64_t)gridDim.x * 4) {
    const int e0 = a.rowptr[u], deg = a.messages ? a.rowptr[u + 1] - e0 : 0;
    const int32_t* list = a.col + e0;
    for (int m = 0; m < a.M; ++m) {
      const float* Fm = a.F + D * m;
      float4 p = ld4(a.P + u * a.ldp + D * m + c);
      for (int r = 0; r < a.R; ++r) {
        float4 y = p;
        if (deg > 0) {
          const float mx = score_max(p, Fm, a.ldf, list, deg, qw, c);
          float den = 0.f;
          float4 acc = zero4();
          GRCN_FOR_LIST(deg)
            const float4 xk = ld4(Fm + (int64_t)list[kk] * a.ldf + c);
            const float e = ok ? expf(row16_sum(dot4(p, xk)) - mx) : 0.f;
            den += e;
            acc = f4_fma(e, xk, acc);
          GRCN_END
          den = q4_sum(den);
          y = f4_add(p, div4(q4_sum4(acc), den));
        }
        const float nv = fmaxf(sqrtf(row16_sum(dot4(y, y))), 1e-12f);
        p = f4_scale(1.f / nv, y);
        if (qw == 0) st4(a.P + (int64_t)(r + 1) * a.pstride + u * a.ldp + D * m + c, p);
        if (lane == 0) a.nrmY[((int64_t)r * a.M + m) * a.U + u] = nv;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ final attention
struct Graph {
  int64_t U, I, E;
  const int32_t *rowptr, *col, *trp, *tcol;
};

struct AttnFwdArgs {
  Graph g;
  int M;
  const float* P;
  int64_t ldp;
  const float* F;
  int64_t ldf;
  float* rep;
  int64_t ldr;
  float* alpha;  // M x 2E
};

__global__ __launch_bounds__(256) void grcn_attn_fwd_kernel(AttnFwdArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, qw = lane >> 4, c = (lane & 15) * 4;
  const bool lead = (lane & 15) == 0;
  const int64_t N = a.g.U + a.g.I;
  for (int64_t w = (int64_t)blockIdx.x * 4 + wv; w < N; w += (int64_t)gridDim.x * 4) {
    const bool user = w < a.g.U;
    const int64_t i = w - a.g.U;
    const int e0 = user ? a.g.rowptr[w] : a.g.trp[i], deg = (user ? a.g.rowptr[w + 1] : a.g.trp[i + 1]) - e0;
    const int32_t* list = (user ? a.g.col : a.g.tcol) + e0;
    const float* Xd = user ? a.P + w * a.ldp : a.F + i * a.ldf;
    const float* Xs = user ? a.F : a.P;
    const int64_t lds = user ? a.ldf : a.ldp;
    for (int m = 0; m < a.M; ++m) {
      const float4 xd = ld4(Xd + D * m + c);
      float4 out = xd;
      if (deg > 0) {
        const float* Xm = Xs + D * m;
        float* al = a.alpha + (int64_t)m * 2 * a.g.E + (user ? 0 : a.g.E) + e0;
        const float mx = score_max(xd, Xm, lds, list, deg, qw, c);
        float den = 0.f;
        float4 acc = zero4();
        GRCN_FOR_LIST(deg)
          const float4 xk = ld4(Xm + (int64_t)list[kk] * lds + c);
          const float e = ok ? expf(row16_sum(dot4(xd, xk)) - mx) : 0.f;
          den += e;
          acc = f4_fma(e, xk, acc);
          if (ok && lead) al[k] = e;
        GRCN_END
        den = q4_sum(den);
        out = f4_add(xd, div4(q4_sum4(acc), den));
        if (lead)
          for (int k = qw; k < deg; k += 4) al[k] = al[k] / den;  // the lane's own writes
      }
      if (qw == 0) st4(a.rep + w * a.ldr + D * m + c, out);
    }
  }
}

// ------------------------------------------------------------------------------------------------ refine
// arg[q] = the winning modality, + 2 where the ReLU pruned the edge
__global__ __launch_bounds__(256) void grcn_refine_fwd_kernel(Graph g, int M, const int32_t* __restrict__ csr2csc,
                                                              const int32_t* __restrict__ csc2csr,
                                                              const float* __restrict__ alpha,
                                                              const float* __restrict__ conf, int64_t ldc,
                                                              float* __restrict__ W, float* __restrict__ WT,
                                                              int32_t* __restrict__ arg) {
  const int64_t E = g.E;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < 2 * E; q += (int64_t)gridDim.x * 256) {
    const bool aside = q < E;
    const int64_t s = aside ? g.U + g.col[q] : g.tcol[q - E];
    float best = alpha[q] * conf[s * ldc];
    int bm = 0;
    if (M == 2) {
      const float v1 = alpha[2 * E + q] * conf[s * ldc + 1];
      if (v1 > best) {
        best = v1;
        bm = 1;
      }
    }
    const bool live = best > 0.f;
    const float w = live ? best : 0.f;
    W[q] = w;
    WT[aside ? E + csr2csc[q] : csc2csr[q - E]] = w;
    arg[q] = bm + (live ? 0 : 2);
  }
}

struct DwArgs {
  Graph g;
  const float *x, *x1, *dx1, *gr;
  int64_t ldx, ldx1, lddx1, ldg;
  float* dw;
};

__global__ __launch_bounds__(256) void grcn_dw_kernel(DwArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, qw = lane >> 4, c = (lane & 15) * 4;
  const bool lead = (lane & 15) == 0;
  const int64_t N = a.g.U + a.g.I;
  for (int64_t w = (int64_t)blockIdx.x * 4 + wv; w < N; w += (int64_t)gridDim.x * 4) {
    const bool user = w < a.g.U;
    const int64_t i = w - a.g.U;
    const int e0 = user ? a.g.rowptr[w] : a.g.trp[i], deg = (user ? a.g.rowptr[w + 1] : a.g.trp[i + 1]) - e0;
    const int32_t* list = (user ? a.g.col : a.g.tcol) + e0;
    const int64_t off = user ? a.g.U : 0;
    float* dw = a.dw + (user ? 0 : a.g.E) + e0;
    const float4 d1 = ld4(a.dx1 + w * a.lddx1 + c), gg = ld4(a.gr + w * a.ldg + c);
    GRCN_FOR_LIST(deg)
      const int64_t s = off + list[kk];
      const float v = row16_sum(dot4(ld4(a.x + s * a.ldx + c), d1) + dot4(ld4(a.x1 + s * a.ldx1 + c), gg));
      if (ok && lead) dw[k] = v;
    GRCN_END
  }
}

struct RefBwdArgs {
  Graph g;
  int M;
  const int32_t *csr2csc, *csc2csr;
  const float *alpha, *conf;
  int64_t ldc;
  const int32_t* arg;
  const float* dw;
  float *dalpha, *dconf;
  int64_t lddc;
};

// a wave per source node: a user is the source of the item-destination edges of its own CSR row, an item of the
// user-destination edges of its CSC row
__global__ __launch_bounds__(256) void grcn_refine_bwd_kernel(RefBwdArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t N = a.g.U + a.g.I, E = a.g.E;
  for (int64_t w = (int64_t)blockIdx.x * 4 + wv; w < N; w += (int64_t)gridDim.x * 4) {
    const bool user = w < a.g.U;
    const int64_t i = w - a.g.U;
    const int e0 = user ? a.g.rowptr[w] : a.g.trp[i], e1 = user ? a.g.rowptr[w + 1] : a.g.trp[i + 1];
    const float c0 = a.conf[w * a.ldc], c1 = a.M == 2 ? a.conf[w * a.ldc + 1] : 0.f;
    float acc0 = 0.f, acc1 = 0.f;
    for (int e = e0 + lane; e < e1; e += 64) {
      const int64_t q = user ? E + a.csr2csc[e] : a.csc2csr[e];
      const int ar = a.arg[q];
      const float d = a.dw[q];
      const float v0 = ar == 0 ? d : 0.f, v1 = ar == 1 ? d : 0.f;
      a.dalpha[q] = v0 * c0;
      acc0 += v0 * a.alpha[q];
      if (a.M == 2) {
        a.dalpha[2 * E + q] = v1 * c1;
        acc1 += v1 * a.alpha[2 * E + q];
      }
    }
    acc0 = gmr::wave_sum(acc0);
    acc1 = gmr::wave_sum(acc1);
    if (lane == 0) {
      a.dconf[w * a.lddc] = acc0;
      if (a.M == 2) a.dconf[w * a.lddc + 1] = acc1;
    }
  }
}

// ------------------------------------------------------------------------------------------------ attention backward
struct AttnBwdArgs {
  Graph g;
  int M;
  const float* P;
  int64_t ldp;
  const float* F;
  int64_t ldf;
  const float *alpha, *dalpha;  // M x 2E
  const float* drep;            // N x 64 M
  int64_t lddr;
  float* ds;   // M x 2E
  float* dxd;  // N x 64 M: drep + sum_k ds_k x_k
  int64_t lddx;
};

__global__ __launch_bounds__(256) void grcn_attn_bwd_dst_kernel(AttnBwdArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, qw = lane >> 4, c = (lane & 15) * 4;
  const bool lead = (lane & 15) == 0;
  const int64_t N = a.g.U + a.g.I;
  for (int64_t w = (int64_t)blockIdx.x * 4 + wv; w < N; w += (int64_t)gridDim.x * 4) {
    const bool user = w < a.g.U;
    const int64_t i = w - a.g.U;
    const int e0 = user ? a.g.rowptr[w] : a.g.trp[i], deg = (user ? a.g.rowptr[w + 1] : a.g.trp[i + 1]) - e0;
    const int32_t* list = (user ? a.g.col : a.g.tcol) + e0;
    const float* Xs = user ? a.F : a.P;
    const int64_t lds = user ? a.ldf : a.ldp;
    for (int m = 0; m < a.M; ++m) {
      const float4 dh = ld4(a.drep + w * a.lddr + D * m + c);
      float4 out = dh;
      if (deg > 0) {
        const float* Xm = Xs + D * m;
        const int64_t eoff = (int64_t)m * 2 * a.g.E + (user ? 0 : a.g.E) + e0;
        const float *al = a.alpha + eoff, *dal = a.dalpha + eoff;
        float* dsv = a.ds + eoff;
        float tbar = 0.f;
        GRCN_FOR_LIST(deg)
          const float t = row16_sum(dot4(dh, ld4(Xm + (int64_t)list[kk] * lds + c))) + dal[kk];
          if (ok) tbar = fmaf(al[kk], t, tbar);
        GRCN_END
        tbar = q4_sum(tbar);
        float4 acc = zero4();
        GRCN_FOR_LIST(deg)
          const float4 xk = ld4(Xm + (int64_t)list[kk] * lds + c);
          const float t = row16_sum(dot4(dh, xk)) + dal[kk];
          const float d = ok ? al[kk] * (t - tbar) : 0.f;
          if (ok && lead) dsv[k] = d;
          acc = f4_fma(d, xk, acc);
        GRCN_END
        out = f4_add(dh, q4_sum4(acc));
      }
      if (qw == 0) st4(a.dxd + w * a.lddx + D * m + c, out);
    }
  }
}

struct RouteBwdArgs {
  int64_t U, E;
  int R, M, messages;
  const int32_t *rowptr, *col;
  const float* F;
  int64_t ldf;
  const float* P;
  int64_t ldp, pstride;
  const float* nrmY;
  const float* dpR;  // U x 64 M: d loss / d p^R
  int64_t lddp;
  float *RA, *RD;  // R x M x E: alpha^r and ds^r in CSR order
  float* DY;       // R x U x 64 M (packed): d loss / d (p^r + h^r)
  const float* pref[2];
  int64_t ldpref;
  const float* nrm0;  // M x U
  const float* regtab;  // U x 64 M or null: added to d preference
  int64_t ldreg;
  float dense[2];  // d preference += dense[m] preference
  float* dpref[2];
  int64_t lddpref;
};

__global__ __launch_bounds__(256) void grcn_route_bwd_dst_kernel(RouteBwdArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, qw = lane >> 4, c = (lane & 15) * 4;
  const bool lead = (lane & 15) == 0;
  for (int64_t u = (int64_t)blockIdx.x * 4 + wv; u < a.U; u += (int64_t)gridDim.x * 4) {
    const int e0 = a.rowptr[u], deg = a.messages ? a.rowptr[u + 1] - e0 : 0;
    const int32_t* list = a.col + e0;
    for (int m = 0; m < a.M; ++m) {
      const float* Fm = a.F + D * m;
      float4 dp = ld4(a.dpR + u * a.lddp + D * m + c);
      for (int r = a.R - 1; r >= 0; --r) {
        const float4 pn = ld4(a.P + (int64_t)(r + 1) * a.pstride + u * a.ldp + D * m + c);
        const float nv = a.nrmY[((int64_t)r * a.M + m) * a.U + u];
        float pd = row16_sum(dot4(pn, dp));
        if (nv <= 1e-12f) pd = 0.f;
        const float4 dy = f4_scale(1.f / nv, sub4(dp, f4_scale(pd, pn)));
        if (qw == 0) st4(a.DY + ((int64_t)r * a.U + u) * (D * a.M) + D * m + c, dy);
        dp = dy;
        if (deg > 0) {
          const float4 pr = ld4(a.P + (int64_t)r * a.pstride + u * a.ldp + D * m + c);
          const int64_t eoff = ((int64_t)r * a.M + m) * a.E + e0;
          const float mx = score_max(pr, Fm, a.ldf, list, deg, qw, c);
          float den = 0.f, tsum = 0.f;
          GRCN_FOR_LIST(deg)
            const float4 xk = ld4(Fm + (int64_t)list[kk] * a.ldf + c);
            const float e = ok ? expf(row16_sum(dot4(pr, xk)) - mx) : 0.f;
            den += e;
            tsum = fmaf(e, row16_sum(dot4(dy, xk)), tsum);
          GRCN_END
          den = q4_sum(den);
          const float tbar = q4_sum(tsum) / den;
          float4 acc = zero4();
          GRCN_FOR_LIST(deg)
            const float4 xk = ld4(Fm + (int64_t)list[kk] * a.ldf + c);
            const float al = expf(row16_sum(dot4(pr, xk)) - mx) / den;
            const float d = ok ? al * (row16_sum(dot4(dy, xk)) - tbar) : 0.f;
            if (ok && lead) {
              a.RA[eoff + k] = al;
              a.RD[eoff + k] = d;
            }
            acc = f4_fma(d, xk, acc);
          GRCN_END
          dp = f4_add(dy, q4_sum4(acc));
        }
      }
      const float4 p0 = ld4(a.P + u * a.ldp + D * m + c);
      const float nv = a.nrm0[(int64_t)m * a.U + u];
      float pd = row16_sum(dot4(p0, dp));
      if (nv <= 1e-12f) pd = 0.f;
      float4 out = f4_scale(1.f / nv, sub4(dp, f4_scale(pd, p0)));
      if (a.dense[m] != 0.f) out = f4_fma(a.dense[m], ld4(a.pref[m] + u * a.ldpref + c), out);
      if (a.regtab) out = f4_add(out, ld4(a.regtab + u * a.ldreg + D * m + c));
      if (qw == 0) st4(a.dpref[m] + u * a.lddpref + c, out);
    }
  }
}

struct SrcTerm {
  const float *A, *DS;  // M arrays with stride estride, indexed by the position map
  int64_t estride;
  const float* DH;  // the destinations' dh rows, n_dst x 64 M
  int64_t lddh;
  const float* XD;  // the destinations' own rows
  int64_t ldxd;
};

struct SrcArgs {
  int64_t n;
  int M, T;
  const int32_t *ptr, *idx, *pos;
  SrcTerm t[MAXT];
  float* out;  // n x 64 M, added to
  int64_t ldo;
};

__global__ __launch_bounds__(256) void grcn_bwd_src_kernel(SrcArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, qw = lane >> 4, c = (lane & 15) * 4;
  for (int64_t s = (int64_t)blockIdx.x * 4 + wv; s < a.n; s += (int64_t)gridDim.x * 4) {
    const int e0 = a.ptr[s], deg = a.ptr[s + 1] - e0;
    if (deg == 0) continue;  // the whole wave
    const int32_t *idx = a.idx + e0, *pos = a.pos + e0;
    for (int m = 0; m < a.M; ++m) {
      float4 acc = zero4();
      for (int t = 0; t < a.T; ++t) {
        const SrcTerm& tm = a.t[t];
        const float *A = tm.A + (int64_t)m * tm.estride, *DS = tm.DS + (int64_t)m * tm.estride;
        GRCN_FOR_LIST(deg)
          const int64_t d = idx[kk], q = pos[kk];
          const float al = ok ? A[q] : 0.f, dsv = ok ? DS[q] : 0.f;
          acc = f4_fma(al, ld4(tm.DH + d * tm.lddh + D * m + c), acc);
          acc = f4_fma(dsv, ld4(tm.XD + d * tm.ldxd + D * m + c), acc);
        GRCN_END
      }
      acc = q4_sum4(acc);
      if (qw == 0) {
        float* o = a.out + s * a.ldo + D * m + c;
        st4(o, f4_add(ld4(o), acc));
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ loss rows
struct LossArgs {
  int B;
  int64_t U;
  int M;
  const float* res;  // N x 64 (1 + M)
  int64_t ldr;
  const float* E;  // N x 64 id embedding
  int64_t lde;
  const float* pref[2];
  int64_t ldpref;
  const int32_t *users, *pos, *neg;
  float inv_norm, reg_weight;
  float* terms;    // 2B: -log sigmoid(s_b); the batch rows' share of the regulariser
  float* contrib;  // 3B x (64 (1 + M) + 64 + 64 M): [d result | d id (reg) | d preference (reg)], rows [u; p; n]
  int64_t ldc;
};

// a wave per batch row; lane l holds columns 4 l .. 4 l + 3 of a result row (l < 16 (1 + M)).  The row's scalars (the
// score, the softplus and its derivative, the sums of squares and the coefficients) are formed in fp64 and rounded
// once: B rows only, and fp32 chains of 128 - 192 products miss the bar of twice fp32 torch's error on a single row
__device__ __forceinline__ double dot4d(float4 a, float4 b) {
  return fma((double)a.w, (double)b.w, fma((double)a.z, (double)b.z, fma((double)a.y, (double)b.y, (double)a.x * (double)b.x)));
}
__global__ __launch_bounds__(256) void grcn_loss_rows_kernel(LossArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = lane * 4;
  const int W = D * (1 + a.M);
  for (int b = blockIdx.x * 4 + wv; b < a.B; b += gridDim.x * 4) {
    const int64_t u = a.users[b], p = a.U + a.pos[b], n = a.U + a.neg[b];
    const bool in = c < W;
    const float4 ru = in ? ld4(a.res + u * a.ldr + c) : zero4(), rp = in ? ld4(a.res + p * a.ldr + c) : zero4(),
                 rn = in ? ld4(a.res + n * a.ldr + c) : zero4();
    const float4 diff = sub4(rp, rn);
    const double s = gmr::wave_sum_d(dot4d(ru, diff));
    // -log sigmoid(s) = softplus(-s), and its derivative -sigmoid(-s)
    const float sp = (float)(fmax(-s, 0.0) + log1p(exp(-fabs(s))));
    const float cf = (float)(-(double)a.inv_norm / (1.0 + exp(s)));
    float* cu = a.contrib + (int64_t)b * a.ldc;
    float* cp = a.contrib + ((int64_t)a.B + b) * a.ldc;
    float* cn = a.contrib + (2 * (int64_t)a.B + b) * a.ldc;
    if (in) {
      st4(cu + c, f4_scale(cf, diff));
      st4(cp + c, f4_scale(cf, ru));
      st4(cn + c, f4_scale(-cf, ru));
    }
    // the regulariser's batch rows: mean(id[users]^2 + id[items]^2) over 2B x 64 and mean(pref_m[users]^2) likewise
    const double k1 = 1.0 / (128.0 * (double)a.B);
    const float k4 = (float)(4.0 * k1 * (double)a.reg_weight), k2 = (float)(2.0 * k1 * (double)a.reg_weight);
    const int part = lane >> 4, cc = (lane & 15) * 4;
    double sq = 0.0;
    if (part == 0) {
      const float4 eu = ld4(a.E + u * a.lde + cc), ep = ld4(a.E + p * a.lde + cc), en = ld4(a.E + n * a.lde + cc);
      sq = 2.0 * dot4d(eu, eu) + dot4d(ep, ep) + dot4d(en, en);
      st4(cu + W + cc, f4_scale(k4, eu));
      st4(cp + W + cc, f4_scale(k2, ep));
      st4(cn + W + cc, f4_scale(k2, en));
    } else if (part <= a.M) {
      const float4 pu = ld4(a.pref[part - 1] + u * a.ldpref + cc);
      sq = 2.0 * dot4d(pu, pu);
      st4(cu + W + D * part + cc, f4_scale(k4, pu));
      st4(cp + W + D * part + cc, zero4());
      st4(cn + W + D * part + cc, zero4());
    }
    sq = gmr::wave_sum_d(sq);
    if (lane == 0) {
      a.terms[b] = sp;
      a.terms[a.B + b] = (float)(k1 * sq);
    }
  }
}

inline unsigned cap_grid(int64_t units, int32_t max_blocks) {
  return (unsigned)gmr::grid_for(units, 1, max_blocks > 0 ? max_blocks : MAX_BLOCKS);
}
inline bool rows16(const float* p, int64_t ld, int cols) { return p && ld >= cols && ld % 4 == 0 && gmr::aligned16(p); }
inline bool graph_ok(int64_t U, int64_t I, int64_t E, const int32_t* rowptr, const int32_t* col, const int32_t* trp,
                     const int32_t* tcol) {
  return U >= 0 && I >= 0 && U + I >= 1 && U + I < (1ll << 31) && E >= 0 && 4 * E < (1ll << 31) && rowptr && trp &&
         (E == 0 || (col && tcol));
}

}  // namespace

// ==================================================================================================== C ABI
#define GRCN_M(M) GMR_ARG((M) == 1 || (M) == 2, "modalities: 1 or 2")
#define GRCN_GRAPH() \
  GMR_ARG(graph_ok(U, I, E, rowptr, col, trp, tcol), "graph: U + I in 1..2^31 - 1, 4 E < 2^31, both lists given")

extern "C" int32_t gmr_grcn_max_blocks(void) { return MAX_BLOCKS; }
extern "C" int32_t gmr_grcn_max_layers(void) { return MAXR; }

extern "C" int gmr_grcn_route_fwd(int64_t U, int32_t R, int32_t M, int32_t messages, const int32_t* rowptr,
                                  const int32_t* col,
                                  const float* F, int64_t ldf, float* P, int64_t ldp, int64_t pstride, float* nrmY,
                                  int32_t max_blocks, void* stream) {
  GRCN_M(M);
  GMR_ARG(U >= 0 && U < (1ll << 31) && R >= 0 && R <= MAXR, "users >= 0, n_layers 0..7");
  if (U == 0) return GMR_OK;
  GMR_ARG(rowptr && (col || R == 0 || !messages), "the users' CSR");
  GMR_ARG(rows16(P, ldp, D * M) && pstride >= (U - 1) * ldp + D * M && pstride % 4 == 0,
          "P: R + 1 tables of U x 64 M, 16-byte aligned rows");
  GMR_ARG(R == 0 || ((!messages || rows16(F, ldf, D * M)) && nrmY),
          "F: I x 64 M, 16-byte aligned rows; nrmY: R x M x U");
  if (R == 0) return GMR_OK;
  RouteFwdArgs a{U, (int)R, (int)M, messages ? 1 : 0, rowptr, col, F, ldf, P, ldp, pstride, nrmY};
  hipLaunchKernelGGL(grcn_route_fwd_kernel, dim3(cap_grid((U + 3) / 4, max_blocks)), dim3(256), 0, (hipStream_t)stream,
                     a);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_grcn_attn_fwd(int64_t U, int64_t I, int64_t E, int32_t M, const int32_t* rowptr,
                                 const int32_t* col, const int32_t* trp, const int32_t* tcol, const float* P,
                                 int64_t ldp, const float* F, int64_t ldf, float* rep, int64_t ldr, float* alpha,
                                 int32_t max_blocks, void* stream) {
  GRCN_M(M);
  GRCN_GRAPH();
  GMR_ARG((U == 0 || rows16(P, ldp, D * M)) && (I == 0 || rows16(F, ldf, D * M)) && rows16(rep, ldr, D * M),
          "P, F, rep: 64 M columns, 16-byte aligned rows");
  GMR_ARG(alpha || E == 0, "alpha: M x 2E");
  AttnFwdArgs a{{U, I, E, rowptr, col, trp, tcol}, (int)M, P, ldp, F, ldf, rep, ldr, alpha};
  hipLaunchKernelGGL(grcn_attn_fwd_kernel, dim3(cap_grid((U + I + 3) / 4, max_blocks)), dim3(256), 0,
                     (hipStream_t)stream, a);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_grcn_refine_fwd(int64_t U, int64_t I, int64_t E, int32_t M, const int32_t* rowptr,
                                   const int32_t* col, const int32_t* trp, const int32_t* tcol,
                                   const int32_t* csr2csc, const int32_t* csc2csr, const float* alpha,
                                   const float* conf, int64_t ldc, float* W, float* WT, int32_t* arg,
                                   int32_t max_blocks, void* stream) {
  GRCN_M(M);
  GRCN_GRAPH();
  if (E == 0) return GMR_OK;
  GMR_ARG(csr2csc && csc2csr && alpha && conf && ldc >= M && W && WT && arg, "null pointer or conf ld < M");
  Graph g{U, I, E, rowptr, col, trp, tcol};
  hipLaunchKernelGGL(grcn_refine_fwd_kernel, dim3(cap_grid((2 * E + 255) / 256, max_blocks)), dim3(256), 0,
                     (hipStream_t)stream, g, (int)M, csr2csc, csc2csr, alpha, conf, ldc, W, WT, arg);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_grcn_dw(int64_t U, int64_t I, int64_t E, const int32_t* rowptr, const int32_t* col,
                           const int32_t* trp, const int32_t* tcol, const float* x, int64_t ldx, const float* x1,
                           int64_t ldx1, const float* dx1, int64_t lddx1, const float* g, int64_t ldg, float* dw,
                           int32_t max_blocks, void* stream) {
  GRCN_GRAPH();
  if (E == 0) return GMR_OK;
  GMR_ARG(rows16(x, ldx, D) && rows16(x1, ldx1, D) && rows16(dx1, lddx1, D) && rows16(g, ldg, D) && dw,
          "x, x1, dx1, g: N x 64, 16-byte aligned rows");
  DwArgs a{{U, I, E, rowptr, col, trp, tcol}, x, x1, dx1, g, ldx, ldx1, lddx1, ldg, dw};
  hipLaunchKernelGGL(grcn_dw_kernel, dim3(cap_grid((U + I + 3) / 4, max_blocks)), dim3(256), 0, (hipStream_t)stream, a);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_grcn_refine_bwd(int64_t U, int64_t I, int64_t E, int32_t M, const int32_t* rowptr,
                                   const int32_t* col, const int32_t* trp, const int32_t* tcol,
                                   const int32_t* csr2csc, const int32_t* csc2csr, const float* alpha,
                                   const float* conf, int64_t ldc, const int32_t* arg, const float* dw, float* dalpha,
                                   float* dconf, int64_t lddc, int32_t max_blocks, void* stream) {
  GRCN_M(M);
  GRCN_GRAPH();
  GMR_ARG(conf && ldc >= M && dconf && lddc >= M, "conf, dconf: N x M");
  GMR_ARG(E == 0 || (csr2csc && csc2csr && alpha && arg && dw && dalpha), "null pointer");
  RefBwdArgs a{{U, I, E, rowptr, col, trp, tcol}, (int)M, csr2csc, csc2csr, alpha, conf, ldc, arg, dw, dalpha, dconf,
               lddc};
  hipLaunchKernelGGL(grcn_refine_bwd_kernel, dim3(cap_grid((U + I + 3) / 4, max_blocks)), dim3(256), 0,
                     (hipStream_t)stream, a);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_grcn_attn_bwd_dst(int64_t U, int64_t I, int64_t E, int32_t M, const int32_t* rowptr,
                                     const int32_t* col, const int32_t* trp, const int32_t* tcol, const float* P,
                                     int64_t ldp, const float* F, int64_t ldf, const float* alpha,
                                     const float* dalpha, const float* drep, int64_t lddr, float* ds, float* dxd,
                                     int64_t lddx, int32_t max_blocks, void* stream) {
  GRCN_M(M);
  GRCN_GRAPH();
  GMR_ARG((U == 0 || rows16(P, ldp, D * M)) && (I == 0 || rows16(F, ldf, D * M)) && rows16(drep, lddr, D * M) &&
              rows16(dxd, lddx, D * M),
          "P, F, drep, dxd: 64 M columns, 16-byte aligned rows");
  GMR_ARG(E == 0 || (alpha && dalpha && ds), "alpha, dalpha, ds: M x 2E");
  AttnBwdArgs a{{U, I, E, rowptr, col, trp, tcol}, (int)M, P, ldp, F, ldf, alpha, dalpha, drep, lddr, ds, dxd, lddx};
  hipLaunchKernelGGL(grcn_attn_bwd_dst_kernel, dim3(cap_grid((U + I + 3) / 4, max_blocks)), dim3(256), 0,
                     (hipStream_t)stream, a);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_grcn_route_bwd_dst(int64_t U, int64_t E, int32_t R, int32_t M, int32_t messages,
                                      const int32_t* rowptr, const int32_t* col, const float* F, int64_t ldf, const float* P, int64_t ldp,
                                      int64_t pstride, const float* nrmY, const float* dpR, int64_t lddp, float* RA,
                                      float* RD, float* DY, const float* pref0, const float* pref1, int64_t ldpref,
                                      const float* nrm0, const float* regtab, int64_t ldreg, float dense0, float dense1,
                                      float* dpref0, float* dpref1, int64_t lddpref, int32_t max_blocks,
                                      void* stream) {
  GRCN_M(M);
  GMR_ARG(U >= 0 && U < (1ll << 31) && E >= 0 && R >= 0 && R <= MAXR && (int64_t)R * M * E < (1ll << 31),
          "users >= 0, n_layers 0..7, R M E < 2^31");
  if (U == 0) return GMR_OK;
  GMR_ARG(rowptr && (col || E == 0), "the users' CSR");
  GMR_ARG(rows16(P, ldp, D * M) && pstride >= (U - 1) * ldp + D * M && rows16(dpR, lddp, D * M) && nrm0,
          "P, dpR: U x 64 M, 16-byte aligned rows; nrm0: M x U");
  GMR_ARG(R == 0 || (nrmY && DY && gmr::aligned16(DY) && (!messages || (rows16(F, ldf, D * M) && (E == 0 || (RA && RD))))),
          "F, nrmY, DY, RA, RD of the routing rounds");
  GMR_ARG(rows16(dpref0, lddpref, D) && (M == 1 || rows16(dpref1, lddpref, D)), "d preference: U x 64 per modality");
  GMR_ARG((dense0 == 0.f || rows16(pref0, ldpref, D)) && (M == 1 || dense1 == 0.f || rows16(pref1, ldpref, D)),
          "a dense term needs the preference rows");
  GMR_ARG(!regtab || rows16(regtab, ldreg, D * M), "regtab: U x 64 M, 16-byte aligned rows");
  RouteBwdArgs a{U, E, (int)R, (int)M, messages ? 1 : 0, rowptr, col, F, ldf, P, ldp, pstride, nrmY, dpR, lddp, RA, RD, DY,
                 {pref0, pref1}, ldpref, nrm0, regtab, ldreg, {dense0, M == 2 ? dense1 : 0.f}, {dpref0, dpref1},
                 lddpref};
  hipLaunchKernelGGL(grcn_route_bwd_dst_kernel, dim3(cap_grid((U + 3) / 4, max_blocks)), dim3(256), 0,
                     (hipStream_t)stream, a);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_grcn_bwd_src(int64_t n, int32_t M, int32_t T, const int32_t* ptr, const int32_t* idx,
                                const int32_t* pos, const float* const* A, const float* const* DS,
                                const int64_t* estride, const float* const* DH, const int64_t* lddh,
                                const float* const* XD, const int64_t* ldxd, float* out, int64_t ldo,
                                int32_t max_blocks, void* stream) {
  GRCN_M(M);
  GMR_ARG(n >= 1 && n < (1ll << 31) && T >= 0 && T <= MAXT, "rows >= 1, 0..8 terms");
  GMR_ARG(ptr && rows16(out, ldo, D * M), "out: n x 64 M, 16-byte aligned rows");
  if (T == 0) return GMR_OK;
  GMR_ARG(idx && pos && A && DS && estride && DH && lddh && XD && ldxd, "null pointer");
  SrcArgs a{n, (int)M, (int)T, ptr, idx, pos, {}, out, ldo};
  for (int t = 0; t < T; ++t) {
    GMR_ARG(A[t] && DS[t] && rows16(DH[t], lddh[t], D * M) && rows16(XD[t], ldxd[t], D * M),
            "a term's arrays and its 64 M-column tables");
    a.t[t] = SrcTerm{A[t], DS[t], estride[t], DH[t], lddh[t], XD[t], ldxd[t]};
  }
  hipLaunchKernelGGL(grcn_bwd_src_kernel, dim3(cap_grid((n + 3) / 4, max_blocks)), dim3(256), 0, (hipStream_t)stream, a);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_grcn_loss_rows(int32_t B, int64_t U, int32_t M, const float* res, int64_t ldr, const float* E,
                                  int64_t lde, const float* pref0, const float* pref1, int64_t ldpref,
                                  const int32_t* users, const int32_t* pos, const int32_t* neg, float inv_norm,
                                  float reg_weight, float* terms, float* contrib, int64_t ldc, int32_t max_blocks,
                                  void* stream) {
  GRCN_M(M);
  GMR_ARG(B >= 1 && U >= 1, "bad row counts");
  GMR_ARG(rows16(res, ldr, D * (1 + M)) && rows16(E, lde, D) && rows16(pref0, ldpref, D) &&
              (M == 1 || rows16(pref1, ldpref, D)),
          "result: 64 (1 + M) columns; id, preference: 64 columns; 16-byte aligned rows");
  GMR_ARG(users && pos && neg && terms && rows16(contrib, ldc, D * (2 + 2 * M)), "contrib: 3B x (128 + 128 M)");
  LossArgs a{(int)B, U, (int)M, res, ldr, E, lde, {pref0, pref1}, ldpref, users, pos, neg, inv_norm, reg_weight, terms,
             contrib, ldc};
  hipLaunchKernelGGL(grcn_loss_rows_kernel, dim3(cap_grid((B + 3) / 4, max_blocks)), dim3(256), 0, (hipStream_t)stream,
                     a);
  GMR_LAUNCHED();
  return GMR_OK;
}
