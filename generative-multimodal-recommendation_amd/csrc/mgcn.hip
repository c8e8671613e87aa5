// MGCN (models/mgcn.py of the reference): the two dense per-row blocks of the forward and their backward, and the
// BPR + L2 rows of the loss.
//   purifier   Pv = E_i * sigmoid(V Wgv^T + bgv),  Pt = E_i * sigmoid(T Wgt^T + bgt)                (item rows)
//   fuser      q(x) = w2 . tanh(W1 x + b1);  (wa, wb) = softmax(q(a), q(b));  m = wa a + wb b
//              side = (sigmoid(Wi c + bi) * (a - m) + sigmoid(Wt c + bt) * (b - m) + m) / 3;  all = c + side
//
//   gmr_mgcn_purify_fwd / _bwd   two 64 x 64 products per row, both modalities in one launch
//   gmr_mgcn_fuse_fwd / _bwd     four 64 x 64 products per row (W1 on a and b, Wi and Wt on c; backward: z . W)
//   gmr_mgcn_bpr_reg_fwd_bwd     -logsigmoid(<u,p> - <u,n>), 0.5 (|u|^2 + |p|^2 + |n|^2) and the rows [du; dp; dn]
//   gmr_mgcn_loss_reduce         loss[] = [total, bpr, reg, nce_items, nce_users] (fixed-order fp64 tree)
//
// The row kernels (the tile scheme of csrc/row_tile.h, shared with csrc/smore.hip): a workgroup of four waves stages
// the weights in LDS once (stride 68) and loops over 16-row tiles with a capped grid.  In the element phases thread tid owns row tid >> 4, columns 4 (tid & 15) .. + 3 of the tile
// (float4 global loads and stores); in the MFMA phases (v_mfma_f32_16x16x4_f32) wave w computes the output columns
// 16 w .. 16 w + 15 of every product and hands them back through the row tiles.  Three weights and three row tiles are
// 65,280 bytes of static LDS, so the fuser passes its fourth product through a tile that has been read already.
// The forward saves tanh(.), the two gate rows and (wa, wb); the backward recomputes nothing.  Every weight gradient
// is a GEMM / column sum on the z rows the backward writes (the host side).
//
// No float atomics; a row's result depends on its own inputs and the weights only (one fixed MFMA k order, one
// butterfly per row sum).
#include "row_tile.h"

namespace {

using namespace gmr_row;  // D, TR, LDX, the element helpers, mm16c / put16c / stage_w (csrc/row_tile.h)
constexpr int MAX_BLOCKS = 256;  // one workgroup per CU; each stages the weights once and loops over tiles

__device__ __forceinline__ float4 sub4(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }

// ------------------------------------------------------------------------------------------------ purifier
struct PurArgs {
  int64_t n;
  const float *E, *V, *T;
  int64_t lde, ldv, ldt;
  const float *Wgv, *bgv, *Wgt, *bgt;
  int64_t ldw;
  float *Pv, *Pt;
  int64_t ldp;
  float *gv, *gt;
  int64_t ldg;
};

__global__ __launch_bounds__(256) void mgcn_purify_fwd_kernel(PurArgs a) {
  __shared__ __attribute__((aligned(16))) float sW[2][D * LDX];
  __shared__ __attribute__((aligned(16))) float sX[2][TR * LDX];
  const int tid = threadIdx.x, w = tid >> 6;
  stage_w(sW[0], a.Wgv, a.ldw, false);
  stage_w(sW[1], a.Wgt, a.ldw, false);
  const int row = tid >> 4, c = (tid & 15) * 4;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  const int64_t ntiles = (a.n + TR - 1) / TR;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t gr = t * TR + row;
    const bool ok = gr < a.n;
    st4(sX[0] + row * LDX + c, ok ? ld4(a.V + gr * a.ldv + c) : z);  // tail rows: zeros, never stored
    st4(sX[1] + row * LDX + c, ok ? ld4(a.T + gr * a.ldt + c) : z);
    __syncthreads();
    floatx4 av = zero4(), at = zero4();
    mm16c(sX[0], sW[0], w, av);
    mm16c(sX[1], sW[1], w, at);
    __syncthreads();
    put16c(sX[0], w, av, a.bgv);
    put16c(sX[1], w, at, a.bgt);
    __syncthreads();
    if (ok) {
      const float4 e = ld4(a.E + gr * a.lde + c);
      const float4 g_v = sigm4(ld4(sX[0] + row * LDX + c)), g_t = sigm4(ld4(sX[1] + row * LDX + c));
      st4(a.gv + gr * a.ldg + c, g_v);
      st4(a.gt + gr * a.ldg + c, g_t);
      st4(a.Pv + gr * a.ldp + c, mul4(e, g_v));
      st4(a.Pt + gr * a.ldp + c, mul4(e, g_t));
    }
    // the next tile's staging writes the four floats this thread just read
  }
}

struct PurBwdArgs {
  int64_t n;
  const float *dPv, *dPt;
  int64_t lddp;
  const float *gv, *gt;
  int64_t ldg;
  const float* E;
  int64_t lde;
  const float *Wgv, *Wgt;
  int64_t ldw;
  float* dE;
  int64_t ldde;
  int accumulate;
  float* z;  // [zv | zt]
  int64_t ldz;
  float *dV, *dT;
  int64_t lddv;
};

__global__ __launch_bounds__(256) void mgcn_purify_bwd_kernel(PurBwdArgs a) {
  __shared__ __attribute__((aligned(16))) float sW[2][D * LDX];
  __shared__ __attribute__((aligned(16))) float sX[2][TR * LDX];
  const int tid = threadIdx.x, w = tid >> 6;
  stage_w(sW[0], a.Wgv, a.ldw, true);
  stage_w(sW[1], a.Wgt, a.ldw, true);
  const int row = tid >> 4, c = (tid & 15) * 4;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  const int64_t ntiles = (a.n + TR - 1) / TR;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t gr = t * TR + row;
    const bool ok = gr < a.n;
    float4 zv = z, zt = z;
    if (ok) {
      const float4 dpv = ld4(a.dPv + gr * a.lddp + c), dpt = ld4(a.dPt + gr * a.lddp + c);
      const float4 g_v = ld4(a.gv + gr * a.ldg + c), g_t = ld4(a.gt + gr * a.ldg + c);
      const float4 e = ld4(a.E + gr * a.lde + c);
      float4 de = gmr::f4_add(mul4(dpv, g_v), mul4(dpt, g_t));
      if (a.accumulate) de = gmr::f4_add(de, ld4(a.dE + gr * a.ldde + c));
      st4(a.dE + gr * a.ldde + c, de);
      zv = mul4(mul4(dpv, e), dsig4(g_v));
      zt = mul4(mul4(dpt, e), dsig4(g_t));
      st4(a.z + gr * a.ldz + c, zv);
      st4(a.z + gr * a.ldz + D + c, zt);
    }
    st4(sX[0] + row * LDX + c, zv);
    st4(sX[1] + row * LDX + c, zt);
    __syncthreads();
    floatx4 av = zero4(), at = zero4();
    mm16c(sX[0], sW[0], w, av);
    mm16c(sX[1], sW[1], w, at);
    __syncthreads();
    put16c(sX[0], w, av, nullptr);
    put16c(sX[1], w, at, nullptr);
    __syncthreads();
    if (ok) {
      st4(a.dV + gr * a.lddv + c, ld4(sX[0] + row * LDX + c));
      st4(a.dT + gr * a.lddv + c, ld4(sX[1] + row * LDX + c));
    }
  }
}

// ------------------------------------------------------------------------------------------------ fuser
struct FuseArgs {
  int64_t n;
  const float *a, *b;
  int64_t ldab;
  const float* c;
  int64_t ldc;
  const float *W1, *b1, *w2, *Wi, *bi, *Wt, *bt;
  int64_t ldw;
  float *side, *all;
  int64_t ldo;
  float *ha, *hb, *gi, *gt;  // saved for the backward
  int64_t lds;
  float* wab;  // n x 2: (wa, wb)
};

__global__ __launch_bounds__(256) void mgcn_fuse_fwd_kernel(FuseArgs a) {
  __shared__ __attribute__((aligned(16))) float sW[3][D * LDX];  // W1, Wi, Wt as [j][k]
  __shared__ __attribute__((aligned(16))) float sX[3][TR * LDX];
  const int tid = threadIdx.x, w = tid >> 6;
  stage_w(sW[0], a.W1, a.ldw, false);
  stage_w(sW[1], a.Wi, a.ldw, false);
  stage_w(sW[2], a.Wt, a.ldw, false);
  const int row = tid >> 4, c = (tid & 15) * 4;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 w2 = ld4(a.w2 + c);
  const int64_t ntiles = (a.n + TR - 1) / TR;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t gr = t * TR + row;
    const bool ok = gr < a.n;
    const float4 xa = ok ? ld4(a.a + gr * a.ldab + c) : z, xb = ok ? ld4(a.b + gr * a.ldab + c) : z;
    const float4 xc = ok ? ld4(a.c + gr * a.ldc + c) : z;
    float* mine[3] = {sX[0] + row * LDX + c, sX[1] + row * LDX + c, sX[2] + row * LDX + c};
    st4(mine[0], xa);
    st4(mine[1], xb);
    st4(mine[2], xc);
    __syncthreads();
    floatx4 p1a = zero4(), p1b = zero4(), pi = zero4(), pt = zero4();
    mm16c(sX[0], sW[0], w, p1a);
    mm16c(sX[1], sW[0], w, p1b);
    mm16c(sX[2], sW[1], w, pi);
    mm16c(sX[2], sW[2], w, pt);
    __syncthreads();
    put16c(sX[0], w, p1a, a.b1);
    put16c(sX[1], w, p1b, a.b1);
    put16c(sX[2], w, pi, a.bi);
    __syncthreads();
    const float4 ha = tanh4(ld4(mine[0])), hb = tanh4(ld4(mine[1])), gi = sigm4(ld4(mine[2]));
    __syncthreads();
    put16c(sX[0], w, pt, a.bt);  // the fourth product, through a tile every thread has read
    __syncthreads();
    const float4 gt = sigm4(ld4(mine[0]));
    const float qa = row16_sum(dot4(w2, ha)), qb = row16_sum(dot4(w2, hb));
    const float wa = 1.f / (1.f + expf(qb - qa)), wb = 1.f / (1.f + expf(qa - qb));  // equal logits: 0.5, 0.5
    if (ok) {
      const float4 m = make_float4(wa * xa.x + wb * xb.x, wa * xa.y + wb * xb.y, wa * xa.z + wb * xb.z,
                                   wa * xa.w + wb * xb.w);
      const float4 s = gmr::f4_add(gmr::f4_add(mul4(gi, sub4(xa, m)), mul4(gt, sub4(xb, m))), m);
      const float4 side = make_float4(s.x / 3.f, s.y / 3.f, s.z / 3.f, s.w / 3.f);
      st4(a.side + gr * a.ldo + c, side);
      st4(a.all + gr * a.ldo + c, gmr::f4_add(xc, side));
      st4(a.ha + gr * a.lds + c, ha);
      st4(a.hb + gr * a.lds + c, hb);
      st4(a.gi + gr * a.lds + c, gi);
      st4(a.gt + gr * a.lds + c, gt);
      if ((tid & 15) == 0) {
        a.wab[2 * gr] = wa;
        a.wab[2 * gr + 1] = wb;
      }
    }
  }
}

struct FuseBwdArgs {
  int64_t n;
  const float* dall;
  int64_t ldda;
  const float *dside, *dcin;  // either may be null (zero)
  int64_t ldds;
  const float *a, *b;
  int64_t ldab;
  const float *ha, *hb, *gi, *gt;
  int64_t lds;
  const float* wab;
  const float *w2, *W1, *Wi, *Wt;
  int64_t ldw;
  float *da, *db;
  int64_t lddab;
  float* dc;
  int64_t lddc;
  float *z1a, *z1b, *zi, *zt;
  int64_t ldz;
  float* r;
  int64_t ldr;
};

__global__ __launch_bounds__(256) void mgcn_fuse_bwd_kernel(FuseBwdArgs a) {
  __shared__ __attribute__((aligned(16))) float sW[3][D * LDX];  // W1, Wi, Wt as [k][j]
  __shared__ __attribute__((aligned(16))) float sX[3][TR * LDX];
  const int tid = threadIdx.x, w = tid >> 6;
  stage_w(sW[0], a.W1, a.ldw, true);
  stage_w(sW[1], a.Wi, a.ldw, true);
  stage_w(sW[2], a.Wt, a.ldw, true);
  const int row = tid >> 4, c = (tid & 15) * 4;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 w2 = ld4(a.w2 + c);
  const int64_t ntiles = (a.n + TR - 1) / TR;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t gr = t * TR + row;
    const bool ok = gr < a.n;
    float4 z1a = z, z1b = z, zi = z, zt = z, da = z, db = z, dc = z, dm = z, ab = z, ha = z, hb = z;
    float wa = 0.f, wb = 0.f;
    if (ok) {
      const float4 g = ld4(a.dall + gr * a.ldda + c);
      const float4 ds = a.dside ? gmr::f4_add(g, ld4(a.dside + gr * a.ldds + c)) : g;
      dc = a.dcin ? gmr::f4_add(g, ld4(a.dcin + gr * a.ldds + c)) : g;
      const float4 s3 = make_float4(ds.x / 3.f, ds.y / 3.f, ds.z / 3.f, ds.w / 3.f);
      const float4 xa = ld4(a.a + gr * a.ldab + c), xb = ld4(a.b + gr * a.ldab + c);
      const float4 gi = ld4(a.gi + gr * a.lds + c), gt = ld4(a.gt + gr * a.lds + c);
      ha = ld4(a.ha + gr * a.lds + c);
      hb = ld4(a.hb + gr * a.lds + c);
      wa = a.wab[2 * gr];
      wb = a.wab[2 * gr + 1];
      const float4 m = make_float4(wa * xa.x + wb * xb.x, wa * xa.y + wb * xb.y, wa * xa.z + wb * xb.z,
                                   wa * xa.w + wb * xb.w);
      zi = mul4(mul4(s3, sub4(xa, m)), dsig4(gi));
      zt = mul4(mul4(s3, sub4(xb, m)), dsig4(gt));
      dm = make_float4(s3.x * (1.f - gi.x - gt.x), s3.y * (1.f - gi.y - gt.y), s3.z * (1.f - gi.z - gt.z),
                       s3.w * (1.f - gi.w - gt.w));
      ab = sub4(xa, xb);
      da = gmr::f4_fma(wa, dm, mul4(s3, gi));
      db = gmr::f4_fma(wb, dm, mul4(s3, gt));
    }
    // softmax over two logits: dqa = wa wb <dm, a - b>, dqb = -dqa
    const float dqa = wa * wb * row16_sum(dot4(dm, ab));
    if (ok) {
      z1a = gmr::f4_scale(dqa, mul4(w2, dtanh4(ha)));
      z1b = gmr::f4_scale(-dqa, mul4(w2, dtanh4(hb)));
      st4(a.z1a + gr * a.ldz + c, z1a);
      st4(a.z1b + gr * a.ldz + c, z1b);
      st4(a.zi + gr * a.ldz + c, zi);
      st4(a.zt + gr * a.ldz + c, zt);
      st4(a.r + gr * a.ldr + c, gmr::f4_scale(dqa, sub4(ha, hb)));
    }
    float* mine[3] = {sX[0] + row * LDX + c, sX[1] + row * LDX + c, sX[2] + row * LDX + c};
    st4(mine[0], z1a);
    st4(mine[1], z1b);
    st4(mine[2], zi);
    __syncthreads();
    floatx4 pa = zero4(), pb = zero4(), pc = zero4();
    mm16c(sX[0], sW[0], w, pa);
    mm16c(sX[1], sW[0], w, pb);
    mm16c(sX[2], sW[1], w, pc);
    __syncthreads();
    st4(mine[2], zt);  // the fourth product's rows, in the tile every wave has read
    __syncthreads();
    mm16c(sX[2], sW[2], w, pc);
    __syncthreads();
    put16c(sX[0], w, pa, nullptr);
    put16c(sX[1], w, pb, nullptr);
    put16c(sX[2], w, pc, nullptr);
    __syncthreads();
    if (ok) {
      st4(a.da + gr * a.lddab + c, gmr::f4_add(da, ld4(mine[0])));
      st4(a.db + gr * a.lddab + c, gmr::f4_add(db, ld4(mine[1])));
      st4(a.dc + gr * a.lddc + c, gmr::f4_add(dc, ld4(mine[2])));
    }
  }
}

// ------------------------------------------------------------------------------------------------ loss rows
// 16 lanes per batch row, 4 columns per lane
__global__ __launch_bounds__(256) void mgcn_bpr_reg_kernel(int B, int64_t U, const float* __restrict__ A, int64_t lda,
                                                           const int* __restrict__ users, const int* __restrict__ pos,
                                                           const int* __restrict__ neg, float inv_norm, float reg_coef,
                                                           float* __restrict__ terms, float* __restrict__ contrib,
                                                           int64_t ldc) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t b = gid >> 4;
  const bool ok = b < B;
  const int c = (int)(gid & 15) * 4;
  float4 u = make_float4(0.f, 0.f, 0.f, 0.f), p = u, q = u;
  if (ok) {
    u = ld4(A + (int64_t)users[b] * lda + c);
    p = ld4(A + (U + pos[b]) * lda + c);
    q = ld4(A + (U + neg[b]) * lda + c);
  }
  const float x = row16_sum(dot4(u, p) - dot4(u, q));
  const float sq = row16_sum(dot4(u, u) + dot4(p, p) + dot4(q, q));
  if (!ok) return;
  if ((gid & 15) == 0) {
    terms[b] = fmaxf(-x, 0.f) + log1pf(expf(-fabsf(x)));  // -F.logsigmoid(x)
    terms[(int64_t)B + b] = 0.5f * sq;
  }
  const float dx = -inv_norm / (1.f + expf(x));
  st4(contrib + b * ldc + c, gmr::f4_fma(reg_coef, u, gmr::f4_scale(dx, sub4(p, q))));
  st4(contrib + ((int64_t)B + b) * ldc + c, gmr::f4_fma(reg_coef, p, gmr::f4_scale(dx, u)));
  st4(contrib + (2 * (int64_t)B + b) * ldc + c, gmr::f4_fma(reg_coef, q, gmr::f4_scale(-dx, u)));
}

// loss[0..4] = [total, bpr, reg, nce_items, nce_users] from terms [4][B]; fixed-order fp64 tree
__global__ void __launch_bounds__(1024) mgcn_loss_reduce_kernel(int B, const float* __restrict__ terms, float inv_norm,
                                                                float reg_coef, float cl_loss,
                                                                float* __restrict__ loss) {
  __shared__ double s[4][1024];
  const int t = threadIdx.x;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = t; b < B; b += 1024)
    for (int k = 0; k < 4; ++k) acc[k] += (double)terms[(int64_t)k * B + b];
  for (int k = 0; k < 4; ++k) s[k][t] = acc[k];
  __syncthreads();
  for (int off = 512; off > 0; off >>= 1) {
    if (t < off)
      for (int k = 0; k < 4; ++k) s[k][t] += s[k][t + off];
    __syncthreads();
  }
  if (t == 0) {
    const float bpr = (float)(s[0][0] * (double)inv_norm), reg = (float)(s[1][0] * (double)reg_coef);
    const float ni = (float)(s[2][0] * (double)inv_norm), nu = (float)(s[3][0] * (double)inv_norm);
    loss[0] = bpr + reg + cl_loss * (ni + nu);
    loss[1] = bpr;
    loss[2] = reg;
    loss[3] = ni;
    loss[4] = nu;
  }
}

inline unsigned tiles_grid(int64_t n) { return (unsigned)gmr::grid_for(n, TR, MAX_BLOCKS); }

}  // namespace

// ==================================================================================================== C ABI
extern "C" int32_t gmr_mgcn_tile_rows(void) { return TR; }
extern "C" int32_t gmr_mgcn_max_blocks(void) { return MAX_BLOCKS; }

extern "C" int gmr_mgcn_purify_fwd(int64_t n, const float* E, int64_t lde, const float* V, int64_t ldv, const float* T,
                                   int64_t ldt, const float* Wgv, const float* bgv, const float* Wgt, const float* bgt,
                                   int64_t ldw, float* Pv, float* Pt, int64_t ldp, float* gv, float* gt, int64_t ldg,
                                   void* stream) {
  GMR_ARG(n >= 1 && n < (1ll << 31), "bad row count");
  GMR_ARG(bgv && bgt, "null pointer");
  GMR_ARG(rows16(E, lde) && rows16(V, ldv) && rows16(T, ldt) && rows16(Wgv, ldw) && rows16(Wgt, ldw),
          "input rows must be 16-byte aligned with ld >= 64, ld % 4 == 0");
  GMR_ARG(rows16(Pv, ldp) && rows16(Pt, ldp) && rows16(gv, ldg) && rows16(gt, ldg),
          "output rows must be 16-byte aligned with ld >= 64, ld % 4 == 0");
  PurArgs a{n, E, V, T, lde, ldv, ldt, Wgv, bgv, Wgt, bgt, ldw, Pv, Pt, ldp, gv, gt, ldg};
  hipLaunchKernelGGL(mgcn_purify_fwd_kernel, dim3(tiles_grid(n)), dim3(256), 0, (hipStream_t)stream, a);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_mgcn_purify_bwd(int64_t n, const float* dPv, const float* dPt, int64_t lddp, const float* gv,
                                   const float* gt, int64_t ldg, const float* E, int64_t lde, const float* Wgv,
                                   const float* Wgt, int64_t ldw, float* dE, int64_t ldde, int32_t accumulate, float* z,
                                   int64_t ldz, float* dV, float* dT, int64_t lddv, void* stream) {
  GMR_ARG(n >= 1 && n < (1ll << 31), "bad row count");
  GMR_ARG(rows16(dPv, lddp) && rows16(dPt, lddp) && rows16(gv, ldg) && rows16(gt, ldg) && rows16(E, lde) &&
              rows16(Wgv, ldw) && rows16(Wgt, ldw),
          "input rows must be 16-byte aligned with ld >= 64, ld % 4 == 0");
  GMR_ARG(rows16(dE, ldde) && rows16(z, ldz, 2 * D) && rows16(dV, lddv) && rows16(dT, lddv),
          "output rows must be 16-byte aligned (z: ld >= 128, the others ld >= 64), ld % 4 == 0");
  PurBwdArgs a{n, dPv, dPt, lddp, gv, gt, ldg, E, lde, Wgv, Wgt, ldw, dE, ldde, (int)accumulate, z, ldz, dV, dT, lddv};
  hipLaunchKernelGGL(mgcn_purify_bwd_kernel, dim3(tiles_grid(n)), dim3(256), 0, (hipStream_t)stream, a);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_mgcn_fuse_fwd(int64_t n, const float* a, const float* b, int64_t ldab, const float* c, int64_t ldc,
                                 const float* W1, const float* b1, const float* w2, const float* Wi, const float* bi,
                                 const float* Wt, const float* bt, int64_t ldw, float* side, float* all, int64_t ldo,
                                 float* ha, float* hb, float* gi, float* gt, int64_t lds, float* wab, void* stream) {
  GMR_ARG(n >= 1 && n < (1ll << 31), "bad row count");
  GMR_ARG(b1 && w2 && bi && bt && wab && al16(w2), "null pointer (w2: 16-byte aligned)");
  GMR_ARG(rows16(a, ldab) && rows16(b, ldab) && rows16(c, ldc) && rows16(W1, ldw) && rows16(Wi, ldw) && rows16(Wt, ldw),
          "input rows must be 16-byte aligned with ld >= 64, ld % 4 == 0");
  GMR_ARG(rows16(side, ldo) && rows16(all, ldo) && rows16(ha, lds) && rows16(hb, lds) && rows16(gi, lds) &&
              rows16(gt, lds),
          "output rows must be 16-byte aligned with ld >= 64, ld % 4 == 0");
  FuseArgs g{n, a, b, ldab, c, ldc, W1, b1, w2, Wi, bi, Wt, bt, ldw, side, all, ldo, ha, hb, gi, gt, lds, wab};
  hipLaunchKernelGGL(mgcn_fuse_fwd_kernel, dim3(tiles_grid(n)), dim3(256), 0, (hipStream_t)stream, g);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_mgcn_fuse_bwd(int64_t n, const float* dall, int64_t ldda, const float* dside, const float* dcin,
                                 int64_t ldds, const float* a, const float* b, int64_t ldab, const float* ha,
                                 const float* hb, const float* gi, const float* gt, int64_t lds, const float* wab,
                                 const float* w2, const float* W1, const float* Wi, const float* Wt, int64_t ldw,
                                 float* da, float* db, int64_t lddab, float* dc, int64_t lddc, float* z1a, float* z1b,
                                 float* zi, float* zt, int64_t ldz, float* r, int64_t ldr, void* stream) {
  GMR_ARG(n >= 1 && n < (1ll << 31), "bad row count");
  GMR_ARG(wab && w2 && al16(w2), "null pointer (w2: 16-byte aligned)");
  GMR_ARG(rows16(dall, ldda) && (!dside || rows16(dside, ldds)) && (!dcin || rows16(dcin, ldds)) && rows16(a, ldab) &&
              rows16(b, ldab) && rows16(ha, lds) && rows16(hb, lds) && rows16(gi, lds) && rows16(gt, lds) &&
              rows16(W1, ldw) && rows16(Wi, ldw) && rows16(Wt, ldw),
          "input rows must be 16-byte aligned with ld >= 64, ld % 4 == 0");
  GMR_ARG(rows16(da, lddab) && rows16(db, lddab) && rows16(dc, lddc) && rows16(z1a, ldz) && rows16(z1b, ldz) &&
              rows16(zi, ldz) && rows16(zt, ldz) && rows16(r, ldr),
          "output rows must be 16-byte aligned with ld >= 64, ld % 4 == 0");
  FuseBwdArgs g{n, dall, ldda, dside, dcin, ldds, a, b, ldab, ha, hb, gi, gt, lds, wab, w2, W1, Wi, Wt, ldw,
                da, db, lddab, dc, lddc, z1a, z1b, zi, zt, ldz, r, ldr};
  hipLaunchKernelGGL(mgcn_fuse_bwd_kernel, dim3(tiles_grid(n)), dim3(256), 0, (hipStream_t)stream, g);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_mgcn_bpr_reg_fwd_bwd(int32_t B, int64_t n_users, const float* all, int64_t lda, const int32_t* users,
                                        const int32_t* pos, const int32_t* neg, float inv_norm, float reg_weight,
                                        float reg_div, float* terms, float* contrib, int64_t ldc, void* stream) {
  GMR_ARG(B >= 1 && n_users >= 0 && reg_div > 0.f, "bad sizes");
  GMR_ARG(users && pos && neg && terms, "null pointer");
  GMR_ARG(rows16(all, lda) && rows16(contrib, ldc), "rows must be 16-byte aligned with ld >= 64, ld % 4 == 0");
  hipLaunchKernelGGL(mgcn_bpr_reg_kernel, dim3(gmr::grid_for((int64_t)B * 16, 256)), dim3(256), 0, (hipStream_t)stream,
                     (int)B, n_users, all, lda, users, pos, neg, inv_norm, reg_weight / reg_div, terms, contrib, ldc);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_mgcn_loss_reduce(int32_t B, const float* terms, float inv_norm, float reg_weight, float reg_div,
                                    float cl_loss, float* loss, void* stream) {
  GMR_ARG(B >= 1 && terms && loss && reg_div > 0.f, "bad args");
  hipLaunchKernelGGL(mgcn_loss_reduce_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (int)B, terms, inv_norm,
                     reg_weight / reg_div, cl_loss, loss);
  GMR_LAUNCHED();
  return GMR_OK;
}
