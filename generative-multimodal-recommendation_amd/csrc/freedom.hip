// FREEDOM (models/freedom.py): the fused three-term BPR loss with its backward, the degree-sensitive
// edge pruning (weighted sampling without replacement over all train edges), the weighted union of
// the two modal kNN graphs, and the layer mean of the LightGCN propagation.
#include <math.h>

#include "gmr_common.h"

namespace {

using gmr::ld4, gmr::st4, gmr::dot4;
__device__ __forceinline__ float4 f4(float a, float b, float c, float d) { return make_float4(a, b, c, d); }
__device__ __forceinline__ float4 sub4(float4 a, float4 b) { return f4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }

__device__ __forceinline__ float row16_sum(float v) {
#pragma unroll
  for (int m = 8; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// ----------------------------------------------------------------- fused three-term BPR
// -logsigmoid(x) (the exact F.logsigmoid) and inv_norm * d/dx of it
__device__ __forceinline__ float neg_logsigmoid(float x) { return fmaxf(-x, 0.f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float neg_logsigmoid_dx(float x, float inv_norm) { return -inv_norm / (1.f + expf(x)); }

// 16 lanes per batch row, 4 columns per lane.  The user row is read once for the three terms; the
// per-row loss terms go to fp64 partials [3][B] that frd_loss_reduce_kernel sums in a fixed order.
// contrib rows [users | pos | neg] (3B), columns [graph | text | image] (192).
__global__ void __launch_bounds__(256) frd_loss_rows_kernel(
    int B, int64_t U, const float* __restrict__ G, int64_t ldg, const float* __restrict__ T, int64_t ldt,
    const float* __restrict__ V, int64_t ldv, const int* __restrict__ users, const int* __restrict__ pos,
    const int* __restrict__ neg, float reg, float inv_norm, double* __restrict__ parts, float* __restrict__ contrib,
    int64_t ldc) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int b = (int)(gid >> 4);
  const bool ok = b < B;
  const int c = (int)(gid & 15) * 4;
  const float4 z = f4(0, 0, 0, 0);
  float4 u = z, pg = z, ng = z, pt = z, nt = z, pv = z, nv = z;
  if (ok) {
    const int64_t p = pos[b], n = neg[b];
    u = ld4(G + (int64_t)users[b] * ldg + c);
    pg = ld4(G + (U + p) * ldg + c);
    ng = ld4(G + (U + n) * ldg + c);
    if (T) {
      pt = ld4(T + p * ldt + c);
      nt = ld4(T + n * ldt + c);
    }
    if (V) {
      pv = ld4(V + p * ldv + c);
      nv = ld4(V + n * ldv + c);
    }
  }
  // pos_scores - neg_scores, each a row sum (freedom.py:181-184)
  const float xg = row16_sum(dot4(u, pg)) - row16_sum(dot4(u, ng));
  const float xt = row16_sum(dot4(u, pt)) - row16_sum(dot4(u, nt));
  const float xv = row16_sum(dot4(u, pv)) - row16_sum(dot4(u, nv));
  if (!ok) return;
  if ((gid & 15) == 0) {
    parts[b] = (double)neg_logsigmoid(xg);
    parts[(int64_t)B + b] = T ? (double)neg_logsigmoid(xt) : 0.0;
    parts[2 * (int64_t)B + b] = V ? (double)neg_logsigmoid(xv) : 0.0;
  }
  const float cg = neg_logsigmoid_dx(xg, inv_norm);
  const float ct = T ? reg * neg_logsigmoid_dx(xt, inv_norm) : 0.f;
  const float cv = V ? reg * neg_logsigmoid_dx(xv, inv_norm) : 0.f;
  const float4 dg = sub4(pg, ng), dt = sub4(pt, nt), dv = sub4(pv, nv);
  float* du = contrib + (int64_t)b * ldc + c;
  float* dp = contrib + ((int64_t)B + b) * ldc + c;
  float* dn = contrib + (2 * (int64_t)B + b) * ldc + c;
  st4(du, f4(cg * dg.x + ct * dt.x + cv * dv.x, cg * dg.y + ct * dt.y + cv * dv.y, cg * dg.z + ct * dt.z + cv * dv.z,
             cg * dg.w + ct * dt.w + cv * dv.w));
  st4(du + 64, z);
  st4(du + 128, z);
  st4(dp, f4(cg * u.x, cg * u.y, cg * u.z, cg * u.w));
  st4(dp + 64, f4(ct * u.x, ct * u.y, ct * u.z, ct * u.w));
  st4(dp + 128, f4(cv * u.x, cv * u.y, cv * u.z, cv * u.w));
  st4(dn, f4(-cg * u.x, -cg * u.y, -cg * u.z, -cg * u.w));
  st4(dn + 64, f4(-ct * u.x, -ct * u.y, -ct * u.z, -ct * u.w));
  st4(dn + 128, f4(-cv * u.x, -cv * u.y, -cv * u.z, -cv * u.w));
}

// loss[1..3] = the three means, loss[0] = graph + reg * (text + image); fixed-order fp64 tree
__global__ void __launch_bounds__(1024) frd_loss_reduce_kernel(int B, const double* __restrict__ parts, float reg,
                                                               float inv_norm, float* __restrict__ loss) {
  __shared__ double s[3][1024];
  const int t = threadIdx.x;
  double a[3] = {0.0, 0.0, 0.0};
  for (int b = t; b < B; b += 1024)
    for (int k = 0; k < 3; ++k) a[k] += parts[(int64_t)k * B + b];
  for (int k = 0; k < 3; ++k) s[k][t] = a[k];
  __syncthreads();
  for (int off = 512; off > 0; off >>= 1) {
    if (t < off)
      for (int k = 0; k < 3; ++k) s[k][t] += s[k][t + off];
    __syncthreads();
  }
  if (t == 0) {
    const float lg = (float)(s[0][0] * (double)inv_norm), lt = (float)(s[1][0] * (double)inv_norm),
                lv = (float)(s[2][0] * (double)inv_norm);
    loss[0] = lg + reg * (lt + lv);
    loss[1] = lg;
    loss[2] = lt;
    loss[3] = lv;
  }
}

// ----------------------------------------------------------------- degree-sensitive pruning
// key_e = w_e / (-log u_e): the m largest keys are a draw of m edges without replacement with
// probability proportional to w (Efraimidis-Spirakis), which is what torch.multinomial(w, m) draws.
__global__ void __launch_bounds__(256) frd_keys_kernel(int64_t E, const float* __restrict__ w,
                                                       const float* __restrict__ u_in, uint64_t seed, uint64_t step,
                                                       float* __restrict__ keys) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  float u;
  if (u_in) {
    u = u_in[e];
  } else {
    const uint4 r = gmr::Philox::gen(seed ^ 0xF2EED0F2EED0ull, step, (uint64_t)e);
    u = gmr::u32_to_unit(r.x);  // (0, 1]
  }
  // fp64 log and division, one rounding to fp32; -log u is kept away from 0 (u = 1) so keys stay finite
  const double nl = fmax(-log((double)u), 2.9802322387695312e-08);
  const float k = (float)((double)w[e] / nl);
  keys[e] = k > 0.f ? k : 0.f;  // non-negative floats: their bit patterns order like the values
}

constexpr int kSelState = 4;           // [threshold prefix, remaining rank, -, -]
constexpr int kSelHist = 4 * 256;      // one 256-bin histogram per radix pass
constexpr int kSelBlocks = 1024;       // chunks of the tie-rank pass
constexpr int kSelWords = kSelState + kSelHist + kSelBlocks + 1;

// histogram of byte `pass` (from the top) over the keys whose higher bytes equal the prefix
__global__ void __launch_bounds__(256) frd_hist_kernel(int64_t E, const unsigned* __restrict__ keys, int pass,
                                                       const unsigned* __restrict__ state, unsigned* __restrict__ hist) {
  __shared__ unsigned h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int shift = 24 - 8 * pass;
  const unsigned prefix = state[0];
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    const unsigned k = keys[e];
    if (pass == 0 || (k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&h[(k >> shift) & 255u], 1u);
  }
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

// the bin that holds the element of the remaining rank (counted from the largest key)
__global__ void __launch_bounds__(256) frd_pick_kernel(int pass, unsigned m, const unsigned* __restrict__ hist,
                                                       unsigned* __restrict__ state) {
  __shared__ unsigned h[256];
  h[threadIdx.x] = hist[threadIdx.x];
  __syncthreads();
  if (threadIdx.x != 0) return;
  unsigned rem = pass == 0 ? m : state[1], above = 0;
  int bin = 255;
  for (; bin > 0; --bin) {
    if (above + h[bin] >= rem) break;
    above += h[bin];
  }
  state[0] |= (unsigned)bin << (24 - 8 * pass);
  state[1] = rem - above;
}

// keys equal to the threshold, per chunk of the edge list
__global__ void __launch_bounds__(256) frd_tie_count_kernel(int64_t E, int64_t chunk, const unsigned* __restrict__ keys,
                                                            const unsigned* __restrict__ state,
                                                            unsigned* __restrict__ cnt) {
  __shared__ unsigned s;
  if (threadIdx.x == 0) s = 0;
  __syncthreads();
  const unsigned thr = state[0];
  const int64_t lo = blockIdx.x * chunk, hi = lo + chunk < E ? lo + chunk : E;
  unsigned c = 0;
  for (int64_t e = lo + threadIdx.x; e < hi; e += 256) c += keys[e] == thr ? 1u : 0u;
  if (c) atomicAdd(&s, c);
  __syncthreads();
  if (threadIdx.x == 0) cnt[blockIdx.x] = s;
}

// exclusive scan of n <= 1024 counts, in place (+ the total at [n])
__global__ void __launch_bounds__(1024) frd_scan1024_kernel(int n, unsigned* __restrict__ cnt) {
  __shared__ unsigned s[1024];
  const int t = threadIdx.x;
  const unsigned own = t < n ? cnt[t] : 0u;
  s[t] = own;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const unsigned v = t >= off ? s[t - off] : 0u;
    __syncthreads();
    s[t] += v;
    __syncthreads();
  }
  if (t < n) cnt[t] = s[t] - own;
  if (t == n - 1) cnt[n] = s[t];
}

// keep[e] = key above the threshold, or equal to it and among the first `remaining` such edges
__global__ void __launch_bounds__(256) frd_keep_kernel(int64_t E, int64_t chunk, const unsigned* __restrict__ keys,
                                                       const unsigned* __restrict__ state,
                                                       const unsigned* __restrict__ tie_base,
                                                       uint8_t* __restrict__ keep) {
  __shared__ unsigned wave_cnt[4];
  const unsigned thr = state[0], rem = state[1];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t lo = blockIdx.x * chunk, hi = lo + chunk < E ? lo + chunk : E;
  unsigned base = tie_base[blockIdx.x];
  for (int64_t e0 = lo; e0 < hi; e0 += 256) {  // chunk is a multiple of 256: every thread runs every round
    const int64_t e = e0 + threadIdx.x;
    const unsigned k = e < hi ? keys[e] : 0u;
    const bool tie = e < hi && k == thr;
    const unsigned long long m = __ballot(tie);
    if (lane == 0) wave_cnt[wv] = (unsigned)__popcll(m);
    __syncthreads();
    unsigned before = base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    for (int q = 0; q < wv; ++q) before += wave_cnt[q];
    if (e < hi) keep[e] = (k > thr || (tie && before < rem)) ? 1 : 0;
    base += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    __syncthreads();
  }
}

// ----------------------------------------------------------------- weighted kNN union
// one thread per row: both lists into the row's 2k staging slots, sorted by column, equal columns
// summed (a's value first)
__global__ void __launch_bounds__(128) frd_union_stage_kernel(int n, int k, const int* __restrict__ ia, int64_t lda,
                                                              const int* __restrict__ ib, int64_t ldb, float va,
                                                              float vb, int* __restrict__ scol, float* __restrict__ sval,
                                                              int* __restrict__ cnt) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  int* c = scol + (int64_t)r * 2 * k;
  float* v = sval + (int64_t)r * 2 * k;
  int m = 0;
  for (int list = 0; list < (ib ? 2 : 1); ++list) {
    const int* src = list ? ib + (int64_t)r * ldb : ia + (int64_t)r * lda;
    const float val = list ? vb : va;
    for (int j = 0; j < k; ++j) {
      const int x = src[j];
      int p = m;  // insertion sort over <= 2k entries
      while (p > 0 && c[p - 1] > x) --p;
      if (p > 0 && c[p - 1] == x) {
        v[p - 1] += val;
        continue;
      }
      for (int q = m; q > p; --q) {
        c[q] = c[q - 1];
        v[q] = v[q - 1];
      }
      c[p] = x;
      v[p] = val;
      ++m;
    }
  }
  cnt[r] = m;
}

// rowptr = exclusive scan of cnt (one workgroup, fixed order)
__global__ void __launch_bounds__(1024) frd_rowptr_kernel(int n, const int* __restrict__ cnt, int* __restrict__ rowptr) {
  __shared__ int s[1024];
  __shared__ int carry;
  const int t = threadIdx.x;
  if (t == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < n; base += 1024) {
    const int own = base + t < n ? cnt[base + t] : 0;
    s[t] = own;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      const int x = t >= off ? s[t - off] : 0;
      __syncthreads();
      s[t] += x;
      __syncthreads();
    }
    if (base + t < n) rowptr[base + t] = carry + s[t] - own;
    __syncthreads();
    if (t == 1023) carry += s[t];
    __syncthreads();
  }
  if (t == 0) rowptr[n] = carry;
}

__global__ void __launch_bounds__(256) frd_union_write_kernel(int n, int k, const int* __restrict__ scol,
                                                              const float* __restrict__ sval,
                                                              const int* __restrict__ rowptr, int* __restrict__ col,
                                                              float* __restrict__ val) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int r = (int)(i / (2 * k)), j = (int)(i % (2 * k));
  if (r >= n) return;
  const int lo = rowptr[r];
  if (j >= rowptr[r + 1] - lo) return;
  col[lo + j] = scol[i];
  val[lo + j] = sval[i];
}

// ----------------------------------------------------------------- layer mean
struct FrdLayers {
  const float* p[GMR_FRD_MAX_LAYERS];
  int64_t ld[GMR_FRD_MAX_LAYERS];
};

// out[r] = (E_0[r] + ... + E_{n-1}[r]) / n, + h[r - n_users] on the item rows (freedom.py:175-178)
__global__ void __launch_bounds__(256) frd_mean_kernel(int64_t n_rows, int64_t n_users, int n_layers, FrdLayers L,
                                                       const float* __restrict__ h, int64_t ldh,
                                                       float* __restrict__ out, int64_t ldo) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t r = gid >> 4;
  if (r >= n_rows) return;
  const int c = (int)(gid & 15) * 4;
  float4 s = ld4(L.p[0] + r * L.ld[0] + c);
  for (int k = 1; k < n_layers; ++k) s = gmr::f4_add(s, ld4(L.p[k] + r * L.ld[k] + c));
  const float d = (float)n_layers;
  s = f4(s.x / d, s.y / d, s.z / d, s.w / d);
  if (h && r >= n_users) s = gmr::f4_add(s, ld4(h + (r - n_users) * ldh + c));
  st4(out + r * ldo + c, s);
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int gmr_frd_loss_fwd_bwd(int32_t B, int64_t n_users, const float* G, int64_t ldg, const float* T,
                                    int64_t ldt, const float* V, int64_t ldv, const int32_t* users,
                                    const int32_t* pos, const int32_t* neg, float reg_weight, float inv_norm,
                                    double* parts_ws, float* loss, float* contrib, int64_t ldc, void* stream) {
  GMR_ARG(G && users && pos && neg && parts_ws && loss && contrib && B > 0 && n_users >= 0, "bad args");
  GMR_ARG(ldg >= 64 && ldg % 4 == 0 && al16(G) && ldc >= 192 && ldc % 4 == 0 && al16(contrib),
          "G / contrib rows must be 16-byte aligned (ldg >= 64, ldc >= 192)");
  GMR_ARG((!T || (ldt >= 64 && ldt % 4 == 0 && al16(T))) && (!V || (ldv >= 64 && ldv % 4 == 0 && al16(V))),
          "T / V rows must be 16-byte aligned with ld >= 64");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(frd_loss_rows_kernel, dim3(gmr::grid_for((int64_t)B * 16, 256)), dim3(256), 0, st, B, n_users, G,
                     ldg, T, ldt, V, ldv, users, pos, neg, reg_weight, inv_norm, parts_ws, contrib, ldc);
  GMR_LAUNCHED();
  hipLaunchKernelGGL(frd_loss_reduce_kernel, dim3(1), dim3(1024), 0, st, B, parts_ws, reg_weight, inv_norm, loss);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_frd_prune_keys(int64_t n_edges, const float* w, const float* u, uint64_t seed, uint64_t step,
                                  float* keys, void* stream) {
  GMR_ARG(w && keys && n_edges > 0, "bad args");
  hipLaunchKernelGGL(frd_keys_kernel, dim3(gmr::grid_for(n_edges, 256)), dim3(256), 0, (hipStream_t)stream, n_edges, w,
                     u, seed, step, keys);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int64_t gmr_frd_prune_workspace_ints(void) { return kSelWords; }

extern "C" int gmr_frd_prune_select(int64_t n_edges, int64_t m, const float* keys, int32_t* workspace, uint8_t* keep,
                                    void* stream) {
  GMR_ARG(keys && workspace && keep && n_edges > 0 && n_edges < (1ll << 31), "bad args");
  GMR_ARG(m >= 0 && m <= n_edges, "m must be in [0, n_edges]");
  hipStream_t st = (hipStream_t)stream;
  if (m == 0) {
    hipError_t e = hipMemsetAsync(keep, 0, (size_t)n_edges, st);
    return e == hipSuccess ? GMR_OK : gmr::hip_status(__func__, e);
  }
  unsigned* state = (unsigned*)workspace;
  unsigned* hist = state + kSelState;
  unsigned* ties = hist + kSelHist;
  hipError_t e = hipMemsetAsync(workspace, 0, sizeof(int32_t) * kSelWords, st);
  if (e != hipSuccess) return gmr::hip_status(__func__, e);
  const unsigned* kb = (const unsigned*)keys;
  const int hg = gmr::grid_for(n_edges, 256 * 8, 1024);
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(frd_hist_kernel, dim3(hg), dim3(256), 0, st, n_edges, kb, pass, state, hist + 256 * pass);
    GMR_LAUNCHED();
    hipLaunchKernelGGL(frd_pick_kernel, dim3(1), dim3(256), 0, st, pass, (unsigned)m, hist + 256 * pass,
                       state);
    GMR_LAUNCHED();
  }
  int64_t chunk = (n_edges + kSelBlocks - 1) / kSelBlocks;
  chunk = (chunk + 255) / 256 * 256;
  const int nb = (int)((n_edges + chunk - 1) / chunk);
  hipLaunchKernelGGL(frd_tie_count_kernel, dim3(nb), dim3(256), 0, st, n_edges, chunk, kb, state, ties);
  GMR_LAUNCHED();
  hipLaunchKernelGGL(frd_scan1024_kernel, dim3(1), dim3(1024), 0, st, nb, ties);
  GMR_LAUNCHED();
  hipLaunchKernelGGL(frd_keep_kernel, dim3(nb), dim3(256), 0, st, n_edges, chunk, kb, state, ties, keep);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_frd_knn_union_csr(int64_t n, int32_t k, const int32_t* idx_a, int64_t lda, float w_a,
                                     const int32_t* idx_b, int64_t ldb, float w_b, int32_t* stage_col,
                                     float* stage_val, int32_t* count_ws, int32_t* rowptr, int32_t* col, float* val,
                                     void* stream) {
  GMR_ARG(idx_a && stage_col && stage_val && count_ws && rowptr && col && val, "bad args");
  GMR_ARG(n > 0 && k > 0 && lda >= k && (!idx_b || ldb >= k) && n * 2 * (int64_t)k < (1ll << 31), "bad shape");
  hipStream_t st = (hipStream_t)stream;
  // the reference's values (freedom.py:93-100): r = pow(k + 1e-7, -0.5) in fp32, value r * r, times the weight
  const float r = powf((float)k + 1e-7f, -0.5f);
  const float v = r * r;
  hipLaunchKernelGGL(frd_union_stage_kernel, dim3(gmr::grid_for(n, 128)), dim3(128), 0, st, (int)n, (int)k, idx_a, lda,
                     idx_b, ldb, w_a * v, w_b * v, stage_col, stage_val, count_ws);
  GMR_LAUNCHED();
  hipLaunchKernelGGL(frd_rowptr_kernel, dim3(1), dim3(1024), 0, st, (int)n, count_ws, rowptr);
  GMR_LAUNCHED();
  hipLaunchKernelGGL(frd_union_write_kernel, dim3(gmr::grid_for(n * 2 * k, 256)), dim3(256), 0, st, (int)n, (int)k,
                     stage_col, stage_val, rowptr, col, val);
  GMR_LAUNCHED();
  return GMR_OK;
}

extern "C" int gmr_frd_mean_fwd(int64_t n_rows, int64_t n_users, int32_t n_layers, const float* const* layers,
                                const int64_t* ld_layers, const float* h, int64_t ldh, float* out, int64_t ldo,
                                void* stream) {
  GMR_ARG(layers && ld_layers && out && n_rows > 0 && n_users >= 0 && n_users <= n_rows, "bad args");
  GMR_ARG(n_layers >= 1 && n_layers <= GMR_FRD_MAX_LAYERS, "1 to GMR_FRD_MAX_LAYERS layers");
  GMR_ARG(ldo >= 64 && ldo % 4 == 0 && al16(out) && (!h || (ldh >= 64 && ldh % 4 == 0 && al16(h))),
          "rows must be 16-byte aligned with ld >= 64");
  FrdLayers L{};
  for (int k = 0; k < n_layers; ++k) {
    GMR_ARG(layers[k] && ld_layers[k] >= 64 && ld_layers[k] % 4 == 0 && al16(layers[k]), "bad layer table");
    L.p[k] = layers[k];
    L.ld[k] = ld_layers[k];
  }
  hipLaunchKernelGGL(frd_mean_kernel, dim3(gmr::grid_for(n_rows * 16, 256)), dim3(256), 0, (hipStream_t)stream, n_rows,
                     n_users, (int)n_layers, L, h, ldh, out, ldo);
  GMR_LAUNCHED();
  return GMR_OK;
}
