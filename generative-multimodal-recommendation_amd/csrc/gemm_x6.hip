// K3/K4 — fp32 GEMM on the bf16 matrix cores by exact operand splitting (GMR_GEMM_X6).
// Same operand, epilogue, split-K and tile-order conventions as gemm.hip (gemm_impl.h).
#include <stdlib.h>

#include <type_traits>

#include "gemm_impl.h"
#include "x6_split.h"

namespace {
using namespace gmr_gemm;

// ---------------------------------------------------------------------------------------------
// Split-bf16 variant (GMR_GEMM_X6): fp32 operands on the bf16 matrix cores.  Each fp32 x is split
// on its way into LDS into three bf16 terms x = hi + mid + lo, EXACTLY (round-to-nearest splits:
// 3 x 8 significand bits hold fp32's 24), and a product a*b is accumulated as the six bf16 MFMA
// products hi*hi + hi*mid + mid*hi + hi*lo + lo*hi + mid*mid (v_mfma_f32_32x32x16_bf16: bf16
// products are exact in fp32, fp32 accumulation).  The three dropped terms (mid*lo, lo*mid,
// lo*lo) are below 2^-23 |a b|, i.e. at the rounding of an fp32 product, so the sums carry fp32
// accuracy (tests/test_kernels_gpu.py checks the error against fp64 next to the fp32-MFMA kernel's).
// Six 32x32x16 bf16 MFMAs (6 x 32 cycles) replace eight 32x32x2 f32 ones (8 x 64 cycles) per
// 32x32x16 block: 2.7x the fp32 MFMA rate at the instruction level.
// LDS: per stage and operand three planes [rows][32 k] of bf16 (64-byte rows); the 16-byte k
// chunk c of row r sits at chunk c ^ ((r >> 2) & 3), so the 16 lanes of a fragment read hit 16
// distinct bank groups (m- / n-contiguous operands read in place: [32 k][rows] planes, TrTile).  Register staging (the split needs the values in VGPRs anyway); NBUF = 2
// double-buffers LDS (one barrier per k tile), NBUF = 1 for the 256^2 tile (2 barriers).
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int x6_swz(int r) { return (r >> 2) & 3; }

// Edge values: rounding a finite |x| above bf16's largest value (0x1.fep127) to bf16 gives
// inf and then NaN terms, so x is clamped into bf16's range first (one v_med3_f32): hi = +-0x1.fep127
// exactly and x - hi (same binade, Sterbenz) is exact, so the split stays exact up to FLT_MAX.  An inf
// operand still splits into hi = 0x1.fep127, mid = inf, lo = NaN: its products come out non-finite
// (NaN where fp32 gives inf), as an inf input to the fp32 kernel does.
__device__ __forceinline__ void split3(float x, __bf16& h, __bf16& m, __bf16& l) {
  h = (__bf16)__builtin_amdgcn_fmed3f(x, -0x1.fep127f, 0x1.fep127f);
  const float r1 = x - (float)h;  // exact
  m = (__bf16)r1;
  l = (__bf16)(r1 - (float)m);    // exact: at most 8 significand bits remain
}

// N (even) consecutive elements -> their three bf16 vectors, pair by pair as single-issue instructions (x6_split.h:
// split3's values and roundings; written in C++ the subtractions of neighbours compile to v_pk_add_f32)
template <int N, typename V>
__device__ __forceinline__ void split3n(const float* v, V& h, V& m, V& l) {
  typedef unsigned U __attribute__((ext_vector_type(N / 2)));
  U hh, mm, ll;
#pragma unroll
  for (int e = 0; e < N / 2; ++e) {
    unsigned a, b, c;
    gmr_x6::split_pair(v[2 * e], v[2 * e + 1], a, b, c);
    hh[e] = a, mm[e] = b, ll[e] = c;
  }
  h = __builtin_bit_cast(V, hh);
  m = __builtin_bit_cast(V, mm);
  l = __builtin_bit_cast(V, ll);
}

// register tile -> the three bf16 planes of one LDS stage (plane stride PL elements)
template <int R, bool KC, int NT, int N4>
__device__ __forceinline__ void x6_store(const float4 (&r)[N4], __bf16* s) {
  constexpr int PL = R * BK;
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < N4; ++i) {
    const int idx = t + NT * i;
    const float v[4] = {r[i].x, r[i].y, r[i].z, r[i].w};
    if (KC) {  // 4 consecutive k of one row: 8 bytes per plane
      const int rr = idx / (BK / 4), k4 = (idx % (BK / 4)) * 4;
      bf16x4 h, m, l;
      split3n<4>(v, h, m, l);
      const int off = rr * BK + (((k4 >> 3) ^ x6_swz(rr)) << 3) + (k4 & 7);
      *reinterpret_cast<bf16x4*>(s + off) = h;
      *reinterpret_cast<bf16x4*>(s + PL + off) = m;
      *reinterpret_cast<bf16x4*>(s + 2 * PL + off) = l;
    } else {  // 4 consecutive rows at one k: one element per row and plane
      const int kk = idx / (R / 4), m4 = (idx % (R / 4)) * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int rr = m4 + e;
        const int off = rr * BK + (((kk >> 3) ^ x6_swz(rr)) << 3) + (kk & 7);
        __bf16 a, b, c;
        split3(v[e], a, b, c);
        s[off] = a;
        s[PL + off] = b;
        s[2 * PL + off] = c;
      }
    }
  }
}

// k-contiguous operand tile [R rows][BK k] in registers, loaded through per-granule element offsets
// computed once per workgroup: rows past the operand's end are clamped onto its last row (their
// products only reach C rows / columns the epilogue discards), so a full k tile loads with no
// bounds test at all; only the last, partial k tile zeroes k >= K (lda >= K rounded up to 4, so
// its float4 granules that start below K stay inside the row).
template <int R, int NT>
struct KcTile {
  static constexpr int N4 = R * BK / 4 / NT;
  static_assert(N4 * NT * 4 == R * BK, "tile rows x BK must split evenly over the block");
  int off[N4];
  float4 r[N4];

  __device__ __forceinline__ void init(int64_t r0, int64_t nrows, int64_t ld) {
#pragma unroll
    for (int i = 0; i < N4; ++i) {
      const int idx = threadIdx.x + NT * i;
      const int rr = idx / (BK / 4), k4 = (idx % (BK / 4)) * 4;
      const int64_t row = min(r0 + rr, nrows - 1) - r0;
      off[i] = (int)(row * ld) + k4;
    }
  }
  __device__ __forceinline__ void load(const float* __restrict__ base) {  // base = tile row 0, k0
#pragma unroll
    for (int i = 0; i < N4; ++i) r[i] = *reinterpret_cast<const float4*>(base + off[i]);
  }
  __device__ __forceinline__ void load_tail(const float* __restrict__ base, int kleft) {
#pragma unroll
    for (int i = 0; i < N4; ++i) {
      const int k4 = ((threadIdx.x + NT * i) % (BK / 4)) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k4 < kleft) {
        v = *reinterpret_cast<const float4*>(base + off[i]);
        if (k4 + 1 >= kleft) v.y = 0.f;
        if (k4 + 2 >= kleft) v.z = 0.f;
        if (k4 + 3 >= kleft) v.w = 0.f;
      }
      r[i] = v;
    }
  }
};

// m- / n-contiguous operand tile (A stored K x M of a TN call, B stored K x N of an NN / TN call) read in place:
// float4 granules of 4 consecutive rows at one k (a wave loads whole 512-byte or 1-KiB row segments of the operand
// as it lies), split per granule and stored as 8 bytes per plane into [k][row] planes: the transpose of KcTile's
// image, the same bytes per plane.  mstep reads its fragments from them with ds_read_b64_tr_b16 (x6_tr_frag), which
// hands each lane 4 consecutive k of its own row: two of them are the bf16x8 one ds_read_b128 takes from a [row][k]
// image, so the MFMA inputs, and every output bit, are those of the k-contiguous path.
// Swizzle: the 8-byte unit u = row / 4 of k row k sits at unit u ^ ((k & 3) << 3) of that row (R / 4 units, 256 or
// 512 bytes).  A transposed read's 32-lane half takes 4 k rows x 8 units (2 x 16 rows); all k rows start on bank 0,
// so unswizzled the 4 rows of a block collide 4-way; the XOR puts them in the 4 different 64-byte quarters of the
// 256 bytes: 64 distinct banks.  The stores' 16-lane groups write 16 consecutive units of one k row, XOR-ed by one
// constant: 32 distinct banks.
// Rows: granules that start past the operand's last row are clamped onto its last in-bounds granule, and that one
// may straddle the end (the caller guarantees ld >= rows rounded up to 4, a 16-byte aligned base and ld % 4 == 0):
// such values only reach C rows / columns the epilogue discards.  k past the slab's end is zeroed, never loaded.
template <int R, int NT>
struct TrTile {
  static constexpr int N4 = R * BK / 4 / NT;
  static constexpr int GR = R / 4;  // granules per k row
  static_assert(N4 * NT * 4 == R * BK && NT % (4 * GR) == 0, "whole k rows per pass, k & 3 fixed per thread");
  static_assert(R % 128 == 0, "the swizzle moves a unit by up to 24 within its k row, a 32-row block by up to 3");
  int off[N4];
  float4 r[N4];

  __device__ __forceinline__ void init(int64_t r0, int64_t nrows, int64_t ld) {
    const int last = (int)(((nrows - 1) & ~(int64_t)3) - r0);  // first row of the last in-bounds granule
#pragma unroll
    for (int i = 0; i < N4; ++i) {
      const int idx = threadIdx.x + NT * i;
      const int kk = idx / GR, m4 = (idx % GR) * 4;
      off[i] = (int)(kk * ld) + min(m4, last);
    }
  }
  // base = element (k0, row r0); kleft = valid k of this tile (BK for a full one)
  __device__ __forceinline__ void load(const float* __restrict__ base, int kleft) {
    if (kleft == BK) {
#pragma unroll
      for (int i = 0; i < N4; ++i) r[i] = *reinterpret_cast<const float4*>(base + off[i]);
    } else {
#pragma unroll
      for (int i = 0; i < N4; ++i) {
        const int kk = (threadIdx.x + NT * i) / GR;
        r[i] = kk < kleft ? *reinterpret_cast<const float4*>(base + off[i]) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  }
  // the three [k][row] bf16 planes of one LDS stage (plane stride R * BK elements)
  __device__ __forceinline__ void store(__bf16* s) const {
    constexpr int PL = R * BK;
#pragma unroll
    for (int i = 0; i < N4; ++i) {
      const int idx = threadIdx.x + NT * i;
      const int kk = idx / GR, u = idx % GR;
      const float v[4] = {r[i].x, r[i].y, r[i].z, r[i].w};
      bf16x4 h, m, l;
      split3n<4>(v, h, m, l);
      const int o = kk * R + ((u ^ ((kk & 3) << 3)) << 2);
      *reinterpret_cast<bf16x4*>(s + o) = h;
      *reinterpret_cast<bf16x4*>(s + PL + o) = m;
      *reinterpret_cast<bf16x4*>(s + 2 * PL + o) = l;
    }
  }
};

// Per-lane element offset into a TrTile plane for the fragment of rows 32 J + l32 (J: the 32-row block of the tile):
// within its 16-lane group, lane 4 q + p supplies the address of k row q, rows 4 p .. 4 p + 3 of the group's 16
// (ds_read_b64_tr_b16's address map), the groups being (h, row half) = (0, 0), (0, 1), (1, 0), (1, 1) as the MFMA
// operand wants them; k = 8 h + q here, x6_tr_frag adds 16 s (+ 4).
template <int R>
__device__ __forceinline__ int x6_tr_lane_off(int J) {
  const int lane = threadIdx.x & 63;
  const int q = (lane & 15) >> 2, p = lane & 3, gs = (lane >> 4) & 1, h = lane >> 5;
  return (8 * h + q) * R + ((((J ^ q) << 3) + 4 * gs + p) << 2);  // unit (8 J + 4 gs + p) ^ (q << 3)
}

// the bf16x8 fragment (k = 16 s + 8 h + 0..7 of the lane's row) of one TrTile plane: two transposed reads, 4 k each.
// EXEC must be all ones here (the gather crosses lanes): every caller is in wave-uniform control flow.
template <int R>
__device__ __forceinline__ bf16x8 x6_tr_frag(const __bf16* pl, int o, int s) {
  typedef __attribute__((address_space(3))) bf16x4* lds4;
  const bf16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds4)(pl + o + 16 * s * R));
  const bf16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds4)(pl + o + (16 * s + 4) * R));
  return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}

// one k tile of a k-contiguous operand straight into ring registers d (KcTile's offsets; full tile or the
// zero-padded last one): the loads of later ring slots stay in flight while earlier slots are split
template <int R, int NT, int N4>
__device__ __forceinline__ void kc_fetch(float4 (&d)[N4], const KcTile<R, NT>& tl, const float* __restrict__ base,
                                         bool full, int kleft) {
  if (full) {
#pragma unroll
    for (int i = 0; i < N4; ++i) d[i] = *reinterpret_cast<const float4*>(base + tl.off[i]);
  } else {
#pragma unroll
    for (int i = 0; i < N4; ++i) {
      const int k4 = ((threadIdx.x + NT * i) % (BK / 4)) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k4 < kleft) {
        v = *reinterpret_cast<const float4*>(base + tl.off[i]);
        if (k4 + 1 >= kleft) v.y = 0.f;
        if (k4 + 2 >= kleft) v.z = 0.f;
        if (k4 + 3 >= kleft) v.w = 0.f;
      }
      d[i] = v;
    }
  }
}

template <int BM, int BN, int WGM, int WGN, int NBUF, int OCC, int PIPE, bool AKC = true, bool BKC = true>
__global__ void __launch_bounds__(64 * WGM * WGN, OCC) gemm_x6_kernel(int64_t M, int64_t N, int64_t K,
                                                                const float* __restrict__ A, int64_t lda,
                                                                const float* __restrict__ B, int64_t ldb,
                                                                float* __restrict__ C, int64_t ldc, Epi epi,
                                                                int tiles_n, int64_t k_per_split,
                                                                float* __restrict__ ws) {
  constexpr int NT = 64 * WGM * WGN;
  constexpr int WTM = BM / WGM, WTN = BN / WGN;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int APL = BM * BK, BPL = BN * BK;  // bf16 elements per plane
  constexpr int STAGE = 3 * (APL + BPL);
  __shared__ __attribute__((aligned(16))) __bf16 smem[NBUF * STAGE];

  const int nwg = gridDim.x;
  const int b = blockIdx.x;
  const int xcd = b & 7, q = nwg >> 3, r = nwg & 7;
  const int tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
  int tmi, tni;
  tile_mn(tile, tiles_n, (int)((M + BM - 1) / BM), tmi, tni);
  const int64_t m0 = (int64_t)tmi * BM;
  const int64_t n0 = (int64_t)tni * BN;
  const int64_t kbeg = (int64_t)blockIdx.z * k_per_split;
  const int64_t kend = min(K, kbeg + k_per_split);

  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int wm = w / WGN, wn = w % WGN;
  const int h = lane >> 5, l32 = lane & 31;

  // Two accumulators per output tile (round 6): hi * hi alone into acc, the five small products into sml, added
  // once after the k loop.  The bf16 MFMA's fp32 accumulation is not unbiased when it adds products far below
  // the accumulator (it rounds toward -inf by ~0.03 ulp per x6 k step, both signs of the result alike:
  // scripts/micro/mfma_round.hip, profiles/r06j_mfma_rounding.txt); with the small products summed apart, at
  // 2^-8 of the magnitude, that bias shrinks 13x on one-sign sums (-0.185 -> -0.014 ulp of scale over 64 steps)
  // and the mean |error| halves (the gc term's Z = out @ feats sums the denoiser output's errors over 7,050 items,
  // where a bias adds up linearly: gc rows 1.1e-5 -> 1.5e-6 off fp64 at baby, profiles/r06j_*).  Cost: +4-7 % on
  // the p_sample products (the 128^2 three-blocks-per-CU tile no longer fits its registers), ~1 ms per epoch.
  floatx16 acc[TM][TN], sml[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = sml[i][j][e] = 0.f;

  // m- / n-contiguous operands (TrTile planes): the lane's offsets for its row blocks' transposed reads
  [[maybe_unused]] int tra[TM], trb[TN];
#pragma unroll
  for (int i = 0; i < TM; ++i) tra[i] = AKC ? 0 : x6_tr_lane_off<BM>(wm * (WTM / 32) + i);
#pragma unroll
  for (int j = 0; j < TN; ++j) trb[j] = BKC ? 0 : x6_tr_lane_off<BN>(wn * (WTN / 32) + j);

  // one 16-deep MFMA step s (k = 16 s + 8 h + j: chunk 2 s + h of the 32-deep rows) of a stage; gap(g) is called
  // after the step's g-th MFMA (the pipelined loop puts a piece of the next tile's split there)
  auto mstep = [&](const __bf16* a_s, int s, auto&& gap) {
    const __bf16* b_s = a_s + 3 * APL;
    bf16x8 fb[3][TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      if constexpr (BKC) {
        const int row = wn * WTN + j * 32 + l32;
        const int off = row * BK + (((2 * s + h) ^ x6_swz(row)) << 3);
#pragma unroll
        for (int p = 0; p < 3; ++p) fb[p][j] = *reinterpret_cast<const bf16x8*>(b_s + p * BPL + off);
      } else {
#pragma unroll
        for (int p = 0; p < 3; ++p) fb[p][j] = x6_tr_frag<BN>(b_s + p * BPL, trb[j], s);
      }
    }
    // A fragments read per row block: 12 live registers, not 12 TM; the pipelined loop (one block per CU) reads
    // them all ahead of the step's first MFMA, since nothing moves across its gaps
    bf16x8 fa_[TM][3];
    auto read_a = [&](int i) {
      if constexpr (AKC) {
        const int row = wm * WTM + i * 32 + l32;
        const int off = row * BK + (((2 * s + h) ^ x6_swz(row)) << 3);
#pragma unroll
        for (int p = 0; p < 3; ++p) fa_[i][p] = *reinterpret_cast<const bf16x8*>(a_s + p * APL + off);
      } else {
#pragma unroll
        for (int p = 0; p < 3; ++p) fa_[i][p] = x6_tr_frag<BM>(a_s + p * APL, tra[i], s);
      }
    };
    if constexpr (PIPE == 1) {
#pragma unroll
      for (int i = 0; i < TM; ++i) read_a(i);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      if constexpr (PIPE != 1) read_a(i);
      const bf16x8(&fa)[3] = fa_[i];
#pragma unroll
      for (int j = 0; j < TN; ++j) {  // small terms first
        const int g = 6 * (i * TN + j);
        sml[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1], fb[1][j], sml[i][j], 0, 0, 0);
        gap(g);
        sml[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0], fb[2][j], sml[i][j], 0, 0, 0);
        gap(g + 1);
        sml[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[2], fb[0][j], sml[i][j], 0, 0, 0);
        gap(g + 2);
        sml[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0], fb[1][j], sml[i][j], 0, 0, 0);
        gap(g + 3);
        sml[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1], fb[0][j], sml[i][j], 0, 0, 0);
        gap(g + 4);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0], fb[0][j], acc[i][j], 0, 0, 0);
        gap(g + 5);
      }
    }
  };

  auto nogap = [](int) {};
  static_assert((AKC && BKC) || PIPE == 0, "m- / n-contiguous operands: the PIPE 0 loop only");
  std::conditional_t<AKC, KcTile<BM, NT>, TrTile<BM, NT>> ra;
  std::conditional_t<BKC, KcTile<BN, NT>, TrTile<BN, NT>> rb;
  ra.init(m0, M, lda);
  rb.init(n0, N, ldb);
  const float* a0 = AKC ? A + m0 * lda : A + m0;
  const float* b0 = BKC ? B + n0 * ldb : B + n0;
  const int nk = kend > kbeg ? (int)((kend - kbeg + BK - 1) / BK) : 0;
  const int kl = (int)(kend - kbeg - (int64_t)(nk - 1) * BK);  // k in the last tile (1..32)
  auto fetch = [&](int t) {
    const int64_t k0 = kbeg + (int64_t)t * BK;
    if constexpr (AKC && BKC) {
      if (t + 1 < nk || kl == BK) {
        ra.load(a0 + k0);
        rb.load(b0 + k0);
      } else {
        ra.load_tail(a0 + k0, kl);
        rb.load_tail(b0 + k0, kl);
      }
    } else {
      const int kleft = t + 1 < nk ? BK : kl;
      if constexpr (AKC) {
        if (kleft == BK) ra.load(a0 + k0);
        else ra.load_tail(a0 + k0, kleft);
      } else {
        ra.load(a0 + k0 * lda, kleft);
      }
      if constexpr (BKC) {
        if (kleft == BK) rb.load(b0 + k0);
        else rb.load_tail(b0 + k0, kleft);
      } else {
        rb.load(b0 + k0 * ldb, kleft);
      }
    }
  };
  auto store = [&](__bf16* s) {  // the registers of one k tile -> the planes of one LDS stage
    if constexpr (AKC) x6_store<BM, true, NT>(ra.r, s);
    else ra.store(s);
    if constexpr (BKC) x6_store<BN, true, NT>(rb.r, s + 3 * APL);
    else rb.store(s + 3 * APL);
  };
  if constexpr (PIPE == 2) {
    // register ring of PF k tiles (the small 64^2 tiles: one 4-wave block per CU at the 2,048-row GenRecV1
    // products, 12 MFMAs per wave per k tile - one tile of prefetch left every k step waiting on its loads):
    // tile t is split into LDS buffer t & 1, then the slot refills with tile t + PF while t is computed.
    // One barrier per tile: a wave storing tile t has passed tile t - 1's barrier, which every wave reaches
    // only after its compute of tile t - 2 (the previous user of buffer t & 1).
    constexpr int PF = 4;
    constexpr int NA = KcTile<BM, NT>::N4, NB = KcTile<BN, NT>::N4;
    float4 qa[PF][NA], qb[PF][NB];
    auto fetch_slot = [&](float4 (&da)[NA], float4 (&db)[NB], int t) {
      if (t < nk) {
        const int64_t k0 = kbeg + (int64_t)t * BK;
        const bool full = t + 1 < nk || kl == BK;
        kc_fetch<BM, NT, NA>(da, ra, a0 + k0, full, kl);
        kc_fetch<BN, NT, NB>(db, rb, b0 + k0, full, kl);
      }
    };
#pragma unroll
    for (int q = 0; q < PF; ++q) fetch_slot(qa[q], qb[q], q);
    for (int t0 = 0; t0 < nk; t0 += PF) {
#pragma unroll
      for (int q = 0; q < PF; ++q) {
        const int t = t0 + q;
        if (t < nk) {
          __bf16* buf = smem + (t & 1) * STAGE;
          x6_store<BM, true, NT>(qa[q], buf);
          x6_store<BN, true, NT>(qb[q], buf + 3 * APL);
          __syncthreads();
          fetch_slot(qa[q], qb[q], t + PF);
          mstep(buf, 0, nogap);
          mstep(buf, 1, nogap);
        }
      }
    }
    __syncthreads();  // every wave is done with the buffers before an LDS epilogue reuses them
  } else if constexpr (PIPE == 0) {
  int cur = 0;
  if (nk > 0) {
    fetch(0);
    store(smem);
  }
  __syncthreads();
  for (int t = 0; t < nk; ++t) {
    const bool more = t + 1 < nk;
    if (more) fetch(t + 1);
    const __bf16* a_s = smem + cur * STAGE;
    mstep(a_s, 0, nogap);
    mstep(a_s, 1, nogap);
    if constexpr (NBUF == 2) {
      if (more) store(smem + (cur ^ 1) * STAGE);
      __syncthreads();
      cur ^= 1;
    } else {
      __syncthreads();
      if (more) store(smem);
      __syncthreads();
    }
  }
  } else {
    // PIPE = 1 (NBUF = 2): registers double-buffered; tile t+2 loads while tile t is computed and tile t+1
    // (landed during t-1) is split into the free LDS buffer BETWEEN the MFMAs of tile t.  The placement is by
    // hand: the split of a pair of elements is three pieces of 4 + 4 + 5 single-issue VALU instructions
    // (x6_split.h), piece after piece goes behind successive MFMAs, and a sched_barrier after every gap keeps the
    // compiler from moving anything across (it ignored sched_group_barrier pipelines here and left the whole
    // split in one burst between the two steps: profiles/x6_split_listing_counts.txt).  A 32-cycle
    // v_mfma_f32_32x32x16_bf16 gap hides five 4-cycle fillers, so at most one piece (and one LDS write) per gap
    // where the tile has the gaps for it: 128^2, 48 pieces in 48 gaps; 256 x 128, 36 in 48.  The split runs
    // unconditionally: on the last tile it fills the idle buffer with stale registers that are never read.
    static_assert(NBUF == 2, "the pipelined loop double-buffers LDS");
    constexpr int NA = KcTile<BM, NT>::N4, NB = KcTile<BN, NT>::N4, NF = NA + NB;
    constexpr int NM = 6 * TM * TN;                        // MFMAs (gaps) per step
    constexpr int NPC = 6 * NF;                            // pieces per k tile: 2 pairs per float4 granule
    constexpr int PPG = (NPC + 2 * NM - 1) / (2 * NM);     // pieces per gap
    float4 qa[NA], qb[NB];  // tile t+1 while ra / rb take tile t+2
    auto fetch_next = [&](int t) {  // registers of tile t (clamped: past the end a tile is re-read)
      fetch(min(t, nk - 1));
    };
    if (nk > 0) {
      fetch(0);
      x6_store<BM, true, NT>(ra.r, smem);
      x6_store<BN, true, NT>(rb.r, smem + 3 * APL);
      fetch_next(1);
    }
    __syncthreads();
    for (int t = 0; t < nk; ++t) {
#pragma unroll
      for (int i = 0; i < NA; ++i) qa[i] = ra.r[i];
#pragma unroll
      for (int i = 0; i < NB; ++i) qb[i] = rb.r[i];
      if (t + 2 < nk) fetch_next(t + 2);
      const __bf16* a_s = smem + (t & 1) * STAGE;
      __bf16* nxt = smem + ((t & 1) ^ 1) * STAGE;
      gmr_x6::Pair ps[2 * NF];
      unsigned lo[2 * NF];
      // piece c of the tile: pair c / 3 (granule c / 6 of the A | B register list, its .xy or .zw), phase c % 3;
      // the second pair of a granule writes plane (phase) of the granule once both pairs have it
      auto piece = [&](int c) {
        const int p = c / 3, ph = c % 3, gr = p >> 1;
        const float4 v = gr < NA ? qa[gr < NA ? gr : 0] : qb[gr < NA ? 0 : gr - NA];
        const float x0 = (p & 1) ? v.z : v.x, x1 = (p & 1) ? v.w : v.y;
        if (ph == 0) gmr_x6::split_p0(x0, x1, ps[p]);
        else if (ph == 1) gmr_x6::split_p1(x0, x1, ps[p]);
        else lo[p] = gmr_x6::split_p2(ps[p]);
        if (p & 1) {
          const bool isa = gr < NA;
          const int idx = threadIdx.x + NT * (isa ? gr : gr - NA);
          const int rr = idx / (BK / 4), k4 = (idx % (BK / 4)) * 4;
          const int off = rr * BK + (((k4 >> 3) ^ x6_swz(rr)) << 3) + (k4 & 7);
          __bf16* pl = nxt + (isa ? 0 : 3 * APL) + ph * (isa ? APL : BPL) + off;
          const uint2 w = ph == 0   ? make_uint2(ps[p - 1].h, ps[p].h)
                          : ph == 1 ? make_uint2(ps[p - 1].m, ps[p].m)
                                    : make_uint2(lo[p - 1], lo[p]);
          *reinterpret_cast<uint2*>(pl) = w;
        }
      };
      auto gap0 = [&](int g) {
#pragma unroll
        for (int c = g * PPG; c < (g + 1) * PPG; ++c)
          if (c < NPC) piece(c);
        __builtin_amdgcn_sched_barrier(0);
      };
      auto gap1 = [&](int g) { gap0(NM + g); };
      mstep(a_s, 0, gap0);
      mstep(a_s, 1, gap1);
      __syncthreads();
    }
  }

#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] += sml[i][j];

  // epilogues that read an aux / C element per output leave through LDS as float4 row chunks (coalesced
  // C / aux traffic: the p_sample posterior product 870 -> 726 us at 8192 rows); the others store the
  // accumulator fragments directly (the row passes of the LDS epilogue cost the bias-only products)
  if (!ws && epi_reads_x(epi))
    gemm_epilogue_lds<BM, BN, WGM, WGN, NBUF * 3 * (BM + BN) * BK / 2>(acc, reinterpret_cast<float*>(smem), M, N, C,
                                                                     ldc, epi, m0, n0, ws);
  else
    gemm_epilogue<BM, BN, WGM, WGN, 32>(acc, M, N, C, ldc, epi, m0, n0, ws);
}

// 64 x 64 tiles through LDS (row pad 1: conflict-free column reads), 256 threads, 16 elements each;
// reads and writes are 256-byte row segments
__global__ void __launch_bounds__(256) x6_transpose_kernel(const float* __restrict__ src, int64_t ld_src,
                                                           int64_t rows, int64_t cols, float* __restrict__ dst,
                                                           int64_t ld_dst, int64_t tiles_c) {
  __shared__ float t[64][65];
  const int64_t tr = blockIdx.x / tiles_c, tc = blockIdx.x % tiles_c;
  const int64_t r0 = tr * 64, c0 = tc * 64;
  const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int64_t r = r0 + y + 4 * i, c = c0 + x;
    t[y + 4 * i][x] = (r < rows && c < cols) ? src[r * ld_src + c] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int64_t c = c0 + y + 4 * i, r = r0 + x;
    if (c < cols && r < rows) dst[c * ld_dst + r] = t[x][y + 4 * i];
  }
}

}  // namespace

namespace gmr_gemm {

void x6_transpose(const float* src, int64_t ld_src, int64_t rows, int64_t cols, float* dst, int64_t ld_dst,
                  hipStream_t st) {
  const int64_t tr = (rows + 63) / 64, tc = (cols + 63) / 64;
  hipLaunchKernelGGL(x6_transpose_kernel, dim3((unsigned)(tr * tc)), dim3(256), 0, st, src, ld_src, rows, cols, dst,
                     ld_dst, tc);
}

// GMR_GEMM_X6_PIPE = 1 / 0 (read once): every call / no call takes the pipelined loop, whatever its plan or
// GMR_GEMM_X6_PIPE1 flag says; = 2: the 256 x 128 and 128 x 256 tiles take it, the others follow their plan (the
// one form that won standalone, for epoch A/B runs); unset (-1): the plan decides
static int x6_pipe() {
  static const int v = [] {
    const char* e = getenv("GMR_GEMM_X6_PIPE");
    return e ? atoi(e) : -1;
  }();
  return v;
}

// GMR_X6_RING = 0 turns off the register-ring 64^2 kernel (PIPE 2) and its unsplit plans (A/B)
int x6_ring() {
  static const int v = [] {
    const char* e = getenv("GMR_X6_RING");
    return e ? atoi(e) : 1;
  }();
  return v;
}

static int x6_nb128() {
  static const int v = [] {
    const char* e = getenv("GMR_GEMM_X6_NB128");
    return e ? atoi(e) : 0;
  }();
  return v;
}

// GMR_X6_INPLACE (read once; A/B runs): unset (-1): the plan's default (gemm.hip: eligible m- / n-contiguous operands
// of TN / NN split-bf16 calls are read in place, TrTile); 0: always copy them k-contiguous first; 1: only B in place,
// the m-contiguous A of TN calls copied; 2: both in place
int x6_inplace() {
  static const int v = [] {
    const char* e = getenv("GMR_X6_INPLACE");
    return e ? atoi(e) : -1;
  }();
  return v;
}

// the plain loop on m- / n-contiguous operands read in place (TrTile: whole 128-row operand tiles only)
template <int BM, int BN, int WGM, int WGN, int NBUF, int OCC>
static int x6_launch_tr(bool akc, bool bkc, dim3 grid, hipStream_t st, int64_t M, int64_t N, int64_t K, const float* A,
                        int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, const Epi& epi, int tiles_n,
                        int64_t kps, float* ws) {
  if constexpr (BM % 128 == 0 && BN % 128 == 0) {
    const dim3 blk(64 * WGM * WGN);
    if (akc)
      hipLaunchKernelGGL((gemm_x6_kernel<BM, BN, WGM, WGN, NBUF, OCC, 0, true, false>), grid, blk, 0, st, M, N, K, A, lda,
                         B, ldb, C, ldc, epi, tiles_n, kps, ws);
    else if (!bkc)
      hipLaunchKernelGGL((gemm_x6_kernel<BM, BN, WGM, WGN, NBUF, OCC, 0, false, false>), grid, blk, 0, st, M, N, K, A, lda,
                         B, ldb, C, ldc, epi, tiles_n, kps, ws);
    else
      hipLaunchKernelGGL((gemm_x6_kernel<BM, BN, WGM, WGN, NBUF, OCC, 0, false, true>), grid, blk, 0, st, M, N, K, A, lda,
                         B, ldb, C, ldc, epi, tiles_n, kps, ws);
    return 0;
  } else {
    return -1;
  }
}

int x6_launch(int bm, int bn, dim3 grid, hipStream_t st, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
              const float* B, int64_t ldb, float* C, int64_t ldc, const Epi& epi, int tiles_n, int64_t kps, float* ws,
              bool akc, bool bkc, bool pipe) {
  if (x6_pipe() == 0 || x6_pipe() == 1) pipe = x6_pipe() == 1;
  if (x6_pipe() == 2) pipe = pipe || bm * bn == 256 * 128;
#define GMR_X6(BM_, BN_, WGM_, WGN_, NBUF_, OCC_)                                                                \
  {                                                                                                                \
    if (!akc || !bkc)                                                                                              \
      return x6_launch_tr<BM_, BN_, WGM_, WGN_, NBUF_, OCC_>(akc, bkc, grid, st, M, N, K, A, lda, B, ldb, C, ldc, epi, \
                                                             tiles_n, kps, ws);                                   \
    if (NBUF_ == 2 && pipe)                                                                                        \
      hipLaunchKernelGGL((gemm_x6_kernel<BM_, BN_, WGM_, WGN_, NBUF_, OCC_, NBUF_ - 1>), grid, dim3(64 * WGM_ * WGN_), \
                         0, st, M, N, K, A, lda, B, ldb, C, ldc, epi, tiles_n, kps, ws);                           \
    else                                                                                                           \
      hipLaunchKernelGGL((gemm_x6_kernel<BM_, BN_, WGM_, WGN_, NBUF_, OCC_, 0>), grid, dim3(64 * WGM_ * WGN_), 0,   \
                         st, M, N, K, A, lda, B, ldb, C, ldc, epi, tiles_n, kps, ws);                              \
    return 0;                                                                                                      \
  }
  // 256 x 128 / 128 x 256: one 8-wave block per CU, LDS double-buffered (144 KiB); 128^2: two or three
  // 4-wave blocks per CU, single-buffered (48 KiB each), so one block's split / barrier phase overlaps
  // the others' MFMA steps (GMR_GEMM_X6_NB128 = 1 / 3: always two / three single-buffered blocks,
  // = 2: one double-buffered block per CU; for A/B runs)
  // 64^2 (4 waves of 32^2, LDS double-buffered, 48 KiB: three blocks per CU) for the small products
  if (bm == 64 && bn == 64 && (!akc || !bkc)) return -1;  // 64^2 split tiles: NT calls only (make_plan)
  if (bm == 64 && bn == 64 && x6_ring()) {
    hipLaunchKernelGGL((gemm_x6_kernel<64, 64, 2, 2, 2, 3, 2>), grid, dim3(256), 0, st, M, N, K, A, lda, B, ldb, C,
                       ldc, epi, tiles_n, kps, ws);
    return 0;
  }
  if (bm == 64 && bn == 64) GMR_X6(64, 64, 2, 2, 2, 3)
  if (bm == 256 && bn == 128) GMR_X6(256, 128, 4, 2, 2, 1)
  if (bm == 128 && bn == 256) GMR_X6(128, 256, 2, 4, 2, 1)
  if (bm == 128 && bn == 128) {
    // two blocks per CU.  (Three (168 VGPRs) won 4-8 % on the 19445-row p_sample products with one accumulator
    // set (profiles/r02x6_study.txt); with the two sets of round 6 it spills 392 bytes per lane, so it is
    // opt-in, GMR_GEMM_X6_NB128 = 3.)
    const int nb = x6_nb128();
    if (nb == 2 || (pipe && akc && bkc && nb == 0)) GMR_X6(128, 128, 2, 2, 2, 1)  // the pipelined loop double-buffers
    if (nb == 3) GMR_X6(128, 128, 2, 2, 1, 3)
    GMR_X6(128, 128, 2, 2, 1, 2)
  }
#undef GMR_X6
  return -1;
}

}  // namespace gmr_gemm
