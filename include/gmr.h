/* libgmr_hip.so — C-ABI of the MI355X-native GenMMRec hot path (gfx950).
 *
 * The reference (orangeai-research/Generative-Multimodal-Recommendation, GenMMRec/src) is pure
 * PyTorch: its hot path has no FFI.  The boundary it exposes is the Python module API
 * (GeneralRecommender.calculate_loss / full_sort_predict, the trainers' diffusion hooks);
 * every entry point below replaces the torch/ATen call sites named in its comment, and the
 * Python package `gmr` (generative-multimodal-recommendation_amd/gmr) binds them with ctypes.
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless the comment says "host"; the caller owns every
 *     buffer (no allocation inside); workspaces are sized by the *_words and *_floats helpers;
 *   - matrices are row-major with an explicit leading dimension (elements);
 *   - every call is asynchronous on `stream` (a hipStream_t; NULL = legacy default stream);
 *   - return 0 on success, GMR_ERR_ARG for a rejected argument, or -(hipError_t);
 *     gmr_last_error_string() describes the last failure of the calling thread;
 *   - calls are stateless and re-entrant (safe from several threads on different streams).
 */
#ifndef GMR_H_
#define GMR_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GMR_ABI_VERSION 2
#define GMR_OK 0
#define GMR_ERR_ARG (-1000)

/* GEMM epilogues (gmr_gemm_f32) */
#define GMR_EPI_NONE 0         /* C = alpha*acc + beta*C                                  */
#define GMR_EPI_BIAS 1         /* C = alpha*acc + bias + beta*C                           */
#define GMR_EPI_BIAS_TANH 2    /* C = tanh(alpha*acc + bias)            Denoise in_layers */
#define GMR_EPI_LEAKY 3        /* C = leaky_relu(alpha*acc + bias, slope)  modal projection */
#define GMR_EPI_POSTERIOR 4    /* C = c1*(alpha*acc + bias) + c2*aux[m,n], c1 = rv1 ? rv1[m] : slope,
                                  c2 = rv2 ? rv2[m] : beta            p_sample posterior mean */
#define GMR_EPI_DTANH 5        /* C = alpha*acc * (1 - aux[m,n]^2)      tanh backward      */
#define GMR_EPI_ROWSCALE_AUX 6 /* C = alpha*acc + bias + rv1[m]*aux[m,n]                  */
#define GMR_EPI_BIAS_RELU 7    /* C = relu(alpha*acc + bias)        TransformerDecoderLayer FF */
/* split-K workspaces start with this many int32 tile counters: zero them once when the buffer is
 * allocated (every gmr_gemm_f32 call leaves them zero); the partial slabs follow */
#define GMR_GEMM_COUNTER_WORDS 16384
#define GMR_GEMM_GLDS (1 << 22)      /* tile flag: stage operands by global_load_lds (the default) */
#define GMR_GEMM_REGSTAGE (1 << 23)  /* tile flag: stage operands through registers + ds_write */
#define GMR_GEMM_MFMA16 (1 << 24)
#define GMR_GEMM_MFMA32 (1 << 25)
#define GMR_GEMM_X6 (1 << 26)        /* tile flag: split-bf16 operands on the bf16 MFMA (six products, fp32-accurate) */
#define GMR_GEMM_F32 (1 << 27)       /* tile flag: force the fp32-input MFMA (overrides GMR_GEMM_X6=1 in the environment) */
#define GMR_GEMM_X6_PIPE1 (1 << 28)  /* tile flag: a split-bf16 call on a >= 128^2 tile runs the pipelined k loop (the next
                                        tile's split between this tile's MFMAs; 128^2: one double-buffered block per CU).
                                        Same plan, same sums, bit for bit; no effect on any other call */
#define GMR_GEMM_X6_COPY (1 << 29)   /* tile flag: a TN / NN split-bf16 call copies its m- / n-contiguous operands k-contiguous
                                        into the workspace instead of reading them in place.  Same sums, bit for bit */
#define GMR_EPI_DRELU 8        /* C = aux[m,n] > 0 ? alpha*acc : 0  ReLU (+ dropout) backward  */
#define GMR_EPI_LEAKY_NORM 9   /* C = leaky_relu(alpha*acc + bias, slope) and its row normalisation in the split-K
                                  reduce: aux (WRITTEN, ld_aux) = C[m] / max(|C[m]|, 1e-12), rowvec1 (WRITTEN) = that
                                  norm; N = 64 plans with split-K only (DiffMM modality projection + F.normalize,
                                  models/diffmm.py:115-127, 138-149) */
#define GMR_EPI_SCALE_BIAS 10  /* C = slope*(alpha*acc + bias): POSTERIOR with c2 = 0 without reading aux, bit for
                                  bit (the last p_sample step, t = 0, whose posterior mean is the x0 prediction) */

const char* gmr_last_error_string(void);
int gmr_version(void);
int gmr_device_name(char* buf /* host */, int32_t len);
int gmr_zero(void* ptr, int64_t bytes, void* stream);
/* host-layer stream plumbing: an event (timing disabled) and "record ev on from, make to wait" */
int gmr_event_create(void** ev /* host */);
int gmr_event_destroy(void* ev);
int gmr_stream_fork(void* from, void* to, void* ev);
/* test probe (no reference counterpart): a one-wave kernel that sleeps ~us microseconds on `stream`, used to
 * perturb side-stream timing in the stream-ordering tests */
int gmr_delay(int32_t us, void* stream);

/* ---------------------------------------------------------------- K1 graph convolution
 * Y = alpha * A * X + beta * Y for CSR A (int32 rowptr/col, fp32 val).
 * Replaces torch.spmm / torch.sparse.mm: models/diffmm.py:136,139,142,146,149,152,176,179,285;
 * lightgcn.py:120.  X is n_blocks (1,2,4) column blocks of 64 floats; block b reads source
 * row s from x_lo[b] + s*ld_lo[b] when s < split, else x_hi[b] + (s-split)*ld_hi[b]
 * (x_lo/x_hi/ld_* are HOST arrays of device pointers / strides).  A plan is built once per
 * matrix by gmr_spmm_plan_build; seg_nnz selects the schedule:
 *   64..448 (multiple of 64): segment plan — rows cut into <= seg_nnz segments, one wave per
 *            segment, hub rows combined in segment order by a second pass that reads
 *            `partial` (gmr_spmm_partial_rows(...) x (64*n_blocks) floats);
 *   512..8192: blocked plan — whole rows packed into ~seg_nnz-nnz blocks, one 1024-thread
 *            workgroup per block and XCD-pinned 32-column slice, rows cut by the in-block
 *            nnz split combined in LDS (no second pass, `partial` unused).
 *   GMR_SPMM_LANE_PLAN | L (L = 32, 64 or 128): lane plan — X cut into 16- or 32-column
 *            slices pinned one per XCD (L2-resident), one lane group per row of degree <= L
 *            (rows ordered by degree), one workgroup per hub row (degree > L); one launch,
 *            `partial` unused.
 *   GMR_SPMM_LANE_PLAN | GMR_SPMM_PACKED | 32: packed lane plan — as the lane plan, with the
 *            short rows' col/val copied into plan order by gmr_spmm_plan_pack (call it after
 *            gmr_spmm_plan_build, and again whenever col/val change): a row's entries are found
 *            from a degree-bucket table, so no descriptor load sits on the gather chain and the
 *            next rows' entries load while the current gathers land.  Same sums, bit for bit.
 *   GMR_SPMM_CHUNK_PLAN: chunk plan — rows of degree 1..128 cut in row order into tasks of whole
 *            rows holding <= 128 entries; a wave gathers a task's entries in one round whatever
 *            rows they belong to (no idle gather slots on short rows), row sums crossing lane
 *            groups meet in LDS in a fixed order; rows of degree > 128 take a workgroup each;
 *            X sliced per XCD as in the lane plan.  Needs gmr_spmm_plan_pack after the build.
 * All are deterministic.  flags: GMR_SPMM_NO_SPLIT_ROWS when the segment plan has no row
 * longer than seg_nnz (gmr_spmm_plan_info header word 1 == 0): the combine pass is skipped. */
#define GMR_SPMM_NO_SPLIT_ROWS 1
/* lane plans whose hub rows were split into segments (plan header word 2 >> 1 > 0): the launch
 * adds the segment partials (partial buffer of gmr_spmm_partial_rows x 256 floats) in order. */
#define GMR_SPMM_HUB_FIXUP 2
#define GMR_SPMM_LANE_PLAN (1 << 16)
#define GMR_SPMM_PACKED (1 << 17)
#define GMR_SPMM_CHUNK_PLAN (1 << 18)
int64_t gmr_spmm_plan_words(int64_t n_rows, int64_t nnz, int32_t seg_nnz);
int64_t gmr_spmm_partial_rows(int64_t n_rows, int64_t nnz, int32_t seg_nnz);
/* gmr_spmm_plan_build with row classes (non-packed lane plans): the short rows >= class_split are
 * scheduled before the rows < class_split, each class by descending degree (the item rows, then
 * the user rows of a bipartite graph: each phase gathers one side's X rows); 0 = one class.
 * Same sums as the one-class plan. */
int gmr_spmm_plan_build_split(const int32_t* rowptr, int64_t n_rows, int64_t nnz, int32_t seg_nnz,
                              int64_t class_split, int32_t* plan, void* stream);
int gmr_spmm_plan_build(const int32_t* rowptr, int64_t n_rows, int64_t nnz, int32_t seg_nnz, int32_t* plan,
                        void* stream);
/* Copies the 4-word plan header to the host (synchronises the stream): segment plan
 * {n_segments, n_split_rows, n_partials, 0}; blocked plan {n_blocks, 0, 0, seg_nnz};
 * lane plan {n_hub_descriptors, n_short_rows, packed | n_split_hub_rows << 1, L}; chunk plan
 * {n_hub_rows, n_tasks, n_empty_rows, n_packed_entries}. */
int gmr_spmm_plan_pack(const int32_t* rowptr, const int32_t* col, const float* val, int64_t n_rows, int64_t nnz,
                       int32_t seg_nnz, int32_t* plan, void* stream);
/* Lane-plan SpMM with X in column-panel layout: S contiguous panels of panel_rows x W floats
 * (W = 16 for n_blocks 1 and 2, 32 for 4; S = 64 * n_blocks / W), panel s holding columns
 * [s*W, (s+1)*W) of X, so each XCD's slice occupies whole cache lines.  Same sums as
 * gmr_spmm_csr_f32 on the row-major X. */
int gmr_spmm_panel_f32(const int32_t* col, const float* val, int64_t n_rows, int64_t nnz, const int32_t* plan,
                       int32_t seg_nnz, int32_t n_blocks, const float* x_panel, int64_t panel_rows, float alpha,
                       float beta, float* y, int64_t ldy, float* partial, int32_t flags, void* stream);
/* Lane-plan SpMM with one output per 64-column block: block b goes to y_blocks[b] (row stride
 * ld_y[b]; host arrays of device pointers / strides).  Fuses independent products of one matrix
 * (DiffMM's H and K2) into one launch; same sums as the separate gmr_spmm_csr_f32 calls. */
int gmr_spmm_multi_f32(const int32_t* col, const float* val, int64_t n_rows, int64_t nnz, const int32_t* plan,
                       int32_t seg_nnz, int32_t n_blocks, const float* const* x_lo, const int64_t* ld_lo,
                       const float* const* x_hi, const int64_t* ld_hi, int64_t split, float alpha, float beta,
                       float* const* y_blocks, const int64_t* ld_y, float* partial, int32_t flags, void* stream);
/* One launch for up to 4 independent lane-plan products, of one or several matrices (DiffMM's
 * Qi = iadj.[E0|nimg], Qt = tadj.[E0|ntxt] and G = adj.[nimg|ntxt] of forward_MM, models/diffmm.py:
 * 135-149; the backward's adj^T products of the contrastive and BPR gradients, and the UI-graph
 * transposes beside adj^T dE).  Job q is gmr_spmm_multi_f32's argument list; every job keeps its
 * own plan, sources, outputs, alpha/beta, partial buffer and flags, and its sums are exactly the
 * single-job call's.  All jobs of a launch need n_blocks in {1, 2} or all 4.  Hub-row fixups of
 * the jobs that need one (GMR_SPMM_HUB_FIXUP) follow in one second launch. */
typedef struct gmr_spmm_job {
  const int32_t* col;
  const float* val;
  const int32_t* plan;
  float* partial;
  int64_t n_rows, nnz;
  int32_t seg_nnz, n_blocks, flags, reserved;
  const float* x_lo[4];
  int64_t ld_lo[4];
  const float* x_hi[4];
  int64_t ld_hi[4];
  int64_t split;
  float alpha, beta;
  float* y[4];
  int64_t ld_y[4];
} gmr_spmm_job;
int gmr_spmm_jobs_f32(int32_t n_jobs, const gmr_spmm_job* jobs, void* stream);
int gmr_spmm_plan_info(const int32_t* plan, int32_t* host_hdr, void* stream);

/* Side-split SpMM (csrc/spmm_side.hip; the graph-conv products of models/diffmm.py:136-191, 285 and
 * common/trainer.py:464-485).  Rows [0, split) and [split, n) are the two sides of a bipartite
 * adjacency; each XCD serves one (side, 32-column slice) group, lane groups stream tasks of <= T
 * CSR entries (whole rows; hub rows cut into pieces whose partial rows the last-arriving piece adds
 * in order, in-launch).  Plan: built on the HOST from a host copy of rowptr (words from
 * gmr_spmm_side_plan_words), copied to the device, then gmr_spmm_side_pack writes the packed
 * (col, val) entries into it (packed_off = plan word 14).  scratch: gmr_spmm_side_scratch_floats
 * floats, zero before the first call (its counters re-arm themselves); two launches that may run
 * concurrently need separate scratch.  Y = alpha A X + beta Y with X / Y as gmr_spmm_multi_f32's
 * per-block split sources / outputs (16-byte aligned, strides multiples of 4).  A short row's sum
 * is its entries in CSR order; a hub row adds its pieces in piece order: deterministic. */
/* T: bits 0-15 = entries per short-row task (rows of degree > T are hub rows), bits 16-23 = entries
 * per lane group of a hub block (blocks of 8 x that; 0 = 32); | GMR_SIDE_CLASSES: degree-class plan —
 * rows of degree 1 .. 16 are grouped by degree (a wave takes 8 tasks of 16 / d whole rows of one degree
 * d, so every lane group's row ends fall on the same entry slots: full-width row stores), their
 * (col, val) copied in class order by gmr_spmm_side_pack_classes (after gmr_spmm_side_pack, with the
 * host plan); rows above 16 entries are hub rows.  Short-row sums keep CSR order from zero. */
#define GMR_SIDE_CLASSES (1 << 24)
int64_t gmr_spmm_side_plan_words(const int32_t* rowptr_host, int64_t n_rows, int64_t split, int32_t T);
int gmr_spmm_side_plan_build(const int32_t* rowptr_host, int64_t n_rows, int64_t split, int32_t T, int32_t* plan_host,
                             int64_t words);
int64_t gmr_spmm_side_scratch_floats(const int32_t* plan_host);
int gmr_spmm_side_pack(const int32_t* rowptr, const int32_t* col, const float* val, int64_t n_rows, int64_t nnz,
                       int64_t packed_off, int32_t* plan, void* stream);
int gmr_spmm_side_pack_classes(const int32_t* rowptr, const int32_t* col, const float* val, const int32_t* plan_host,
                               int32_t* plan, void* stream);
/* launch shape for tuning sweeps: workgroups per XCD and entries in flight per lane group (8 / 16);
 * defaults GMR_SPMM_SIDE_WPX / GMR_SPMM_SIDE_EB (64 / 16) */
int gmr_spmm_side_tune(int32_t wpx, int32_t eb);
/* wpx: workgroups per XCD of the launch (0 = GMR_SPMM_SIDE_WPX or 64); gmr_spmm_side_tune overrides it */
int gmr_spmm_side_f32(const int32_t* plan, int32_t n_blocks, const float* const* x_lo, const int64_t* ld_lo,
                      const float* const* x_hi, const int64_t* ld_hi, int64_t split, float alpha, float beta,
                      float* const* y_blocks, const int64_t* ld_y, float* scratch, int32_t wpx, void* stream);
/* The same product as Y = alpha A X + beta Z: z_blocks / ld_z (NULL: Z = Y) give the beta term's source, and
 * only_side 0 / 1 computes only the rows < split / >= split (the other rows of Y are left untouched; -1: all),
 * with all eight XCDs on that side.  DiffMM's backward (round 6, models/diffmm.py:141-195): Tcl and the
 * contrastive views' dC = dK + adj^T dK in one pass, and the second GCN hop's item rows T3i = T2i + adj^T T2u. */
int gmr_spmm_side2_f32(const int32_t* plan, int32_t n_blocks, const float* const* x_lo, const int64_t* ld_lo,
                       const float* const* x_hi, const int64_t* ld_hi, int64_t split, float alpha, float beta,
                       const float* const* z_blocks, const int64_t* ld_z, float* const* y_blocks, const int64_t* ld_y,
                       int32_t only_side, float* scratch, int32_t wpx, void* stream);
/* Up to 4 independent side-split products of the same width (n_blocks) in ONE launch (round 5; the forward's
 * Qi / Qt / G and the backward's UI-graph transposes, models/diffmm.py:129-195): job q has its own plan,
 * hub scratch, split and block arrays at entries [4 q, 4 q + n_blocks) of x_lo / ld_lo / x_hi / ld_hi / y /
 * ld_y.  Each job's sums are those of its own gmr_spmm_side_f32 call, bit for bit. */
int gmr_spmm_side_jobs_f32(int32_t njobs, const int32_t* const* plans, float* const* scratch, int32_t n_blocks,
                           const float* const* x_lo, const int64_t* ld_lo, const float* const* x_hi,
                           const int64_t* ld_hi, const int64_t* split, float alpha, float beta, float* const* y,
                           const int64_t* ld_y, int32_t wpx, void* stream);

int gmr_spmm_csr_f32(const int32_t* rowptr, const int32_t* col, const float* val, int64_t n_rows, int64_t nnz,
                     const int32_t* plan, int32_t seg_nnz, float* partial, int32_t n_blocks,
                     const float* const* x_lo, const int64_t* ld_lo, const float* const* x_hi, const int64_t* ld_hi,
                     int64_t split, float alpha, float beta, float* y, int64_t ldy, int32_t flags, void* stream);

/* ---------------------------------------------------------------- K9b fp16 scoring (opt-in)
 * C (E x I, fp32) = fp16(A) (E x 64) . fp16(B)^T, fp32 accumulation on v_mfma_f32_32x32x16_f16;
 * the fp16 MFMA scoring GEMM of BASELINE config 5, replacing the fp32 product of
 * GenRecV1.full_sort_predict (models/genrecv1.py:419-427) when scoring_dtype = fp16.  A and B
 * are fp32 and rounded on load.  d must be 64. */
int gmr_score_f16(int64_t E, int64_t I, int64_t d, const float* A, int64_t lda, const float* B, int64_t ldb,
                  float* C, int64_t ldc, void* stream);

/* ---------------------------------------------------------------- K11 graph construction
 * Symmetric-normalised bipartite adjacency (N = U + I) in CSR from a user->items CSR
 * (items ascending and distinct per user).  Replaces DiffMM.get_norm_adj_mat
 * (models/diffmm.py:88-107: self_loops=0, deg_eps=1e-7) and DiffMMTrainer.buildUIMatrix +
 * normalizeAdj (common/trainer.py:464-485: self_loops=1, deg_eps=0).  rowptr: N+1, col/val:
 * gmr_bipartite_nnz(...) entries, workspace: gmr_bipartite_workspace_ints(...) ints. */
int64_t gmr_bipartite_nnz(int64_t n_users, int64_t n_items, int64_t n_user_items, int32_t self_loops);
int64_t gmr_bipartite_workspace_ints(int64_t n_users, int64_t n_items);
int gmr_bipartite_symnorm_build(int64_t n_users, int64_t n_items, const int32_t* user_ptr, const int32_t* user_items,
                                int64_t n_user_items, int32_t self_loops, double deg_eps, int32_t* workspace,
                                int32_t* rowptr, int32_t* col, float* val, void* stream);
/* per-user top-k item lists (n_users x k, ld) -> user CSR with items sorted (trainer.py:545-562) */
int gmr_topk_to_user_csr(int64_t n_users, int32_t k, const int32_t* topk, int64_t ld, int32_t* user_ptr,
                         int32_t* user_items, void* stream);

/* ---------------------------------------------------------------- K3/K4/K6/K9 dense GEMM (fp32 operands)
 * C[M,N] = epilogue(alpha * op(A) op(B)); op(A) = A (M x K, lda) or A^T (A stored K x M);
 * op(B) = B (K x N, ldb) or B^T (B stored N x K).  bias[(bias_row ? bias_row[m] : 0)*ld_bias + n].
 * Replaces nn.Linear / torch.mm / matmul: diffmm.py:117,124,277,352-358,472-473; vbpr.py:70,105.
 * tile: 0 auto, 64, 128, 256, 256128 (256 x 128), 128256 or 12864 (128 x 64, fp32 kernel only), optionally | GMR_GEMM_MFMA16 (v_mfma_f32_16x16x4_f32)
 * or | GMR_GEMM_MFMA32 (v_mfma_f32_32x32x2_f32) to force the matrix instruction, | GMR_GEMM_REGSTAGE /
 * GMR_GEMM_GLDS to force register or global_load_lds operand staging (same sums, bit for bit);
 * split_k: 0 auto, else >= 1.
 * gmr_gemm_workspace_floats returns the exact scratch the same call needs (GMR_GEMM_COUNTER_WORDS
 * tile counters + splits*M*N floats of split-K partials, 0 when it does not split); the counter
 * words must be zero before the first call (they are left zero).  The split slabs are summed in
 * slab order by a reduce pass; the environment switch GMR_GEMM_FIXUP=1 instead has the last slice
 * of each tile sum them in-launch (same order and bits; slower on gfx950).
 * GMR_GEMM_GROUP=G (tuning) walks G tile rows per column inside each XCD's tile range.
 * Split-bf16 products (gemm_x6.hip): NT calls (trans_a = 0, trans_b = 1) with 16-byte aligned A / B and
 * lda, ldb multiples of 4 on a >= 128^2 tile run on the bf16 matrix cores with every fp32 operand split
 * exactly into three bf16 terms and six products accumulated in fp32 (fp32-accurate: error vs fp64 within
 * the fp32-MFMA kernel's bound, tests/test_kernels_gpu.py); | GMR_GEMM_X6 forces it, | GMR_GEMM_F32 (or
 * any staging / MFMA-shape flag) keeps the fp32-input MFMA, and the environment variable GMR_GEMM_X6=0
 * turns it off for every call.  | GMR_GEMM_X6_PIPE1 picks the pipelined k loop of such a call (the environment
 * variable GMR_GEMM_X6_PIPE = 1 / 0, read once, forces it on / off for every call, = 2 on for the 256 x 128
 * tiles).  TN / NN calls whose NT form qualifies run on it as well: an m- / n-contiguous operand that is 16-byte
 * aligned, with a leading dimension that is a multiple of 4 and >= its rows rounded up to 4 (up to 3 floats past
 * the last row of each k line are read, never used), is read in place; any other, and every one under
 * | GMR_GEMM_X6_COPY or GMR_X6_INPLACE=0, is first copied k-contiguous into the workspace (same sums, bit for
 * bit; gmr_gemm_workspace_floats counts the copies either way).  gmr_gemm_kernel_kind returns the matrix path a call with these
 * arguments takes: 6 (split-bf16), 32 (v_mfma_f32_32x32x2_f32) or 16 (v_mfma_f32_16x16x4_f32). */
int32_t gmr_gemm_kernel_kind(int32_t trans_a, int32_t trans_b, int64_t M, int64_t N, int64_t K, int32_t tile,
                             int32_t split_k, int32_t aligned);
int64_t gmr_gemm_workspace_floats(int32_t trans_a, int32_t trans_b, int64_t M, int64_t N, int64_t K, int32_t tile,
                                  int32_t split_k);
int gmr_gemm_f32(int32_t trans_a, int32_t trans_b, int64_t M, int64_t N, int64_t K, float alpha, const float* A,
                 int64_t lda, const float* B, int64_t ldb, float beta, float* C, int64_t ldc, int32_t epilogue,
                 const float* bias, const int32_t* bias_row, int64_t ld_bias, const float* aux, int64_t ld_aux,
                 const float* rowvec1, const float* rowvec2, float slope, int32_t tile, int32_t split_k,
                 float* workspace, int64_t workspace_floats, void* stream);

/* bf16 plane sets (csrc/planes.hip): an fp32 matrix as three bf16 matrices (uint16 storage) [3][rows][ld]
 * with plane stride ps, x = hi + mid + lo exactly for every fp32 x (the split of GMR_GEMM_X6); ld is a
 * multiple of 32 and the columns [cols, ld) are zero.  gmr_split3_planes writes one from an fp32 matrix
 * (the item table of gmr_score_topk_x6).  (Round 4's pre-split GEMM gmr_gemm_p3_f32 was removed in round 5:
 * slower in the epoch and less accurate at K = 7,050 than the on-the-fly split of gmr_gemm_f32.) */
int gmr_split3_planes(int64_t rows, int64_t cols, const float* src, int64_t ld_src, uint16_t* dst, int64_t ld_dst,
                      int64_t plane_stride, void* stream);

/* ---------------------------------------------------------------- DiffMM rec step (diffmm.py:129-258)
 * Fused row kernels of forward_MM / forward_cl_MM / calculate_loss and their backward
 * (layouts in csrc/diffmm.hip). */
int gmr_dmm_combine_fwd(int64_t n, float* G, const float* H, const float* Qi, const float* Qt, const float* mw,
                        float lam, float* M, void* stream);
int gmr_dmm_final_fwd(int64_t n, const float* M, const float* L, float ris, float* Emb, float* nrm, void* stream);
int gmr_dmm_cl_fwd(int64_t n, const float* Qi, const float* Qt, const float* K2, float* CLN, float* nrm,
                   void* stream);
int gmr_dmm_final_bwd(int64_t n, const float* dEmb, const float* T1, const float* M, const float* nrmM, float ris,
                      const float* E, const float* mw, float* dE, float* partials, void* stream);
int64_t gmr_dmm_final_bwd_partials(int64_t n);
int gmr_dmm_mw_grad(int64_t nparts, const float* partials, const float* mw, float* dmw, int32_t accumulate,
                    void* stream);
int gmr_dmm_dg(int64_t n, int64_t U, const float* dE, const float* T2, float* dG, void* stream);
int gmr_dmm_cl_bwd(int64_t n, const float* dK, const float* T, const float* dE, float lam, float* Ri, float* Rt,
                   void* stream);
int gmr_dmm_assemble(int64_t n, int64_t U, const float* T2, const float* T3, const float* Ri, const float* Rt,
                     const float* E0, float reg2, float* dE0, float* dNF, void* stream);
/* Round 6: the rec step's small passes folded into their neighbours (same reference lines).
 * final_bwd2: clear != 0 zeroes dEmb after reading it (its last reader; the next step's sorted scatter adds onto
 *   zeros, so no fill pass); Ri / Rt (both or neither): also write lam * dE_img / lam * dE_txt into their left
 *   halves (what gmr_dmm_cl_bwd writes there).
 * cl_bwd2: clear != 0 zeroes dK[:, :64] after reading it; left = 0 leaves Ri / Rt's left halves alone.
 * assemble2: dNF leaves through the modality projections' normalize + leaky-ReLU backward (NF = the normalised
 *   projections I x 128, nrmF = their norms [2][I], slope) - gmr_normalize_rows_bwd_f32 on each half, same bits;
 *   dK_clear (N x 128, optional): its [:, :64] half is zeroed (the contrastive view gradient's last reader);
 *   t3u_from_t2: T3's user rows are read from T2 (they are equal: adj is bipartite) - T3 holds item rows only.
 * bpr_sqnorm: gmr_bpr_fwd_bwd and gmr_sqnorm_part_f32(n_sq, x, sq_parts) in one launch (same bits).
 * loss_mw: gmr_dmm_loss_total (+ acc[0] += loss when acc is not NULL: the trainer's epoch-loss sum) and
 *   gmr_dmm_mw_grad (accumulate 0) in one two-block launch. */
int gmr_dmm_final_bwd2(int64_t n, float* dEmb, const float* T1, const float* M, const float* nrmM, float ris,
                       const float* E, const float* mw, float* dE, float* partials, int32_t clear, float lam, float* Ri,
                       float* Rt, void* stream);
int gmr_dmm_cl_bwd2(int64_t n, float* dK, const float* T, const float* dE, float lam, float* Ri, float* Rt,
                    int32_t clear, int32_t left, void* stream);
int gmr_dmm_assemble2(int64_t n, int64_t U, const float* T2, const float* T3, const float* Ri, const float* Rt,
                      const float* E0, float reg2, float* dE0, float* dNF, const float* NF, const float* nrmF,
                      float slope, float* dK_clear, int32_t t3u_from_t2, void* stream);
int gmr_dmm_bpr_sqnorm(int32_t B, int64_t U, const float* Emb, const int32_t* users, const int32_t* pos,
                       const int32_t* neg, float* loss, float* contrib, float inv_norm, int64_t n_sq, const float* x,
                       double* sq_parts, void* stream);
int gmr_dmm_loss_mw(int64_t B, const float* loss_bpr, float inv_nr, const double* parts, int64_t nparts,
                    float reg_scale, const float* loss_cu, const float* loss_ci, float ssl_scale, float* out,
                    float* acc, int64_t n_mw_parts, const float* mw_parts, const float* mw, float* dmw, void* stream);

/* F.normalize (p=2, eps=1e-12) over rows and its backward (optionally fused with leaky-ReLU backward) */
int gmr_normalize_rows_f32(int64_t n, int32_t cols, const float* x, int64_t ldx, float* y, int64_t ldy, float* nrm,
                           void* stream);
int gmr_normalize_rows_bwd_f32(int64_t n, int32_t cols, const float* y, int64_t ldy, const float* nrm, const float* dy,
                               int64_t lddy, float* dx, int64_t lddx, float slope, int32_t accumulate, void* stream);

/* K7 BPR: -log(1e-10 + sigmoid(<a,p> - <a,n>)) with gathers; per-row loss + 3B contribution rows
 * (diffmm.py:220-227, common/loss.py:33-37) */
int gmr_bpr_fwd_bwd(int32_t B, int64_t U, const float* Emb, const int32_t* users, const int32_t* pos,
                    const int32_t* neg, float* loss, float* contrib, float inv_norm, void* stream);
/* K8 InfoNCE pieces (diffmm.py:251-258): in-place row softmax of logits with log-sum-exp out,
 * and the per-row terms of the gathered batch */
/* VBPR calculate_loss (models/vbpr.py:76-97; common/loss.py BPRLoss + EmbLoss): rows of one
 * (U + I) x D table (items at item_off); loss = mean -log(1e-10 + sigmoid(<u,p> - <u,n>)) +
 * reg_weight * (||U||_F + ||P||_F + ||N||_F) / B; contrib = [dU; dP; dN] (3B x D) for
 * gmr_scatter_sorted_f32.  Workspaces: x_ws B floats, sq_ws 3B doubles, coef_ws 3 floats. */
int gmr_vbpr_loss_fwd_bwd(int32_t B, int32_t D, const float* table, int64_t ldt, const int32_t* users,
                          const int32_t* pos, const int32_t* neg, int64_t item_off, float reg_weight, float* x_ws,
                          double* sq_ws, float* coef_ws, float* loss, float* contrib, int64_t ldc, void* stream);
int gmr_fill2d_f32(int64_t rows, int64_t cols, float* p, int64_t ld, float value, void* stream);
int gmr_row_softmax_f32(int64_t rows, int64_t cols, float* L, int64_t ld, float coef, float* lse, void* stream);
int gmr_contrast_rows(int32_t B, const float* CLN, const int32_t* nodes, int64_t node_off, const float* lse,
                      float inv_temp, float coef, float* loss, float* contrib, int64_t ld_contrib, void* stream);
/* K8 fused InfoNCE: forward + backward of DiffMM.contrastLoss (models/diffmm.py:251-258) for one
 * gathered batch, replacing the logits GEMM + row softmax + two gradient GEMMs.  P = view-1 rows of
 * the batch (B x 64, ldp; P_i = CLN[node_off + nodes[i], 0:64]), T = the view-2 table (n x 64, ldt),
 * CLN = the N x 128 [view 1 | view 2] table.  Writes loss[i] = log sum_j exp(<P_i,T_j>/temp) -
 * <P_i,T_node(i)>/temp; contrib[i, 0:64] = dL/dP_i and contrib[i, 64:128] = -coef/temp P_i (the
 * T_node(i) term, for the caller's scatter); dT (n x 64, ld_dt, overwritten) = the dense table
 * gradient; gradients scaled by coef.  No B x n matrix in HBM; f32 MFMA; deterministic.
 * P = NULL (round 6): the passes read P_i = CLN[node_off + nodes[i], 0:64] in place, ldp = CLN's leading
 * dimension (no gathered copy; the default pipelined split-bf16 passes only, else an argument error).
 * workspace: gmr_contrast_workspace_floats(B, n) floats. */
int64_t gmr_contrast_workspace_floats(int32_t B, int64_t n);
int gmr_contrast_fused_f32(int32_t B, int64_t n, const float* P, int64_t ldp, const float* T, int64_t ldt,
                           const float* CLN, const int32_t* nodes, int64_t node_off, float inv_temp, float coef,
                           float* loss, float* contrib, int64_t ld_contrib, float* dT, int64_t ld_dt, float* workspace,
                           int64_t workspace_floats, void* stream);
/* The same with dT taken through the normalize backward of the table's view in the reduce pass (y = the
 * normalised table rows n x 64, ldy; nrm = their norms): dT = nbwd(dense gradient).  DiffMM: the dense part of
 * dK[:, 64:] (contrastLoss's F.normalize, diffmm.py:252-253); the sparse part goes through
 * gmr_scatter_sorted_nbwd_f32 (the normalize backward is linear in its input). */
int gmr_contrast_fused_nbwd_f32(int32_t B, int64_t n, const float* P, int64_t ldp, const float* T, int64_t ldt,
                                const float* CLN, const int32_t* nodes, int64_t node_off, float inv_temp, float coef,
                                float* loss, float* contrib, int64_t ld_contrib, float* dT, int64_t ld_dt,
                                const float* y, int64_t ldy, const float* nrm, float* workspace,
                                int64_t workspace_floats, void* stream);
/* K2 gather / deterministic scatter-add through a sorted (key << 32 | slot) plan */
int gmr_gather_rows_f32(int32_t B, int32_t cols, const float* src, int64_t lds, const int32_t* idx, int64_t off,
                        float* out, int64_t ldo, void* stream);
int gmr_scatter_sorted_f32(int32_t n, int32_t cols, const uint64_t* plan, const float* contrib, int64_t ldc,
                           float* dst, int64_t ldd, void* stream);
/* 128-wide contribution rows through the plan, each 64-column half taken through the normalize backward of the
 * contrastive view it belongs to (y = CLN, N x 128; nrm = [2][n_nodes] norms) and ADDED to dK (N x 128):
 * dK[key] += [nbwd(s[:64]) | nbwd(s[64:])]  (DiffMM contrastLoss's sparse terms, diffmm.py:252-258) */
int gmr_scatter_sorted_nbwd_f32(int32_t n, const uint64_t* plan, const float* contrib, int64_t ldc, const float* y,
                                const float* nrm, int64_t n_nodes, float* dK, void* stream);
int gmr_sort_batch_keys(int64_t n_batches, const int32_t* keys, const int64_t* offsets, const int32_t* key_add,
                        int32_t n_keysets, int64_t key_stride, uint64_t* out, int64_t out_stride, int32_t pow2,
                        void* stream);
/* deterministic reductions */
int gmr_sum_f32(int64_t n, const float* x, float scale, float* out, int32_t accumulate, void* stream);
#define GMR_SQNORM_PARTS 1024 /* workspace doubles of gmr_sqnorm_f32 */
int gmr_sqnorm_f32(int64_t n, const float* x, float scale, float* out, int32_t accumulate, double* workspace,
                   void* stream);
/* The same as two steps: per-block fp64 partials (gmr_sqnorm_nparts(n) of them) into workspace,
 * then gmr_dmm_loss_total sums them in order with the other loss terms of DiffMM.calculate_loss
 * (models/diffmm.py:203-249): out = sum(bpr)*inv_nr + reg*|x|^2 + ssl*(sum(cu) + sum(ci)), one
 * launch and the same float value as the four separate reductions. */
int64_t gmr_sqnorm_nparts(int64_t n);
int gmr_sqnorm_part_f32(int64_t n, const float* x, double* workspace, void* stream);
int gmr_dmm_loss_total(int64_t B, const float* loss_bpr, float inv_nr, const double* parts, int64_t nparts,
                       float reg_scale, const float* loss_cu, const float* loss_ci, float ssl_scale, float* out,
                       void* stream);
int gmr_sum_f64(int64_t n, const double* x, double scale, double* out, int32_t accumulate, void* stream);
int gmr_colsum_f32(int64_t rows, int64_t cols, const float* x, int64_t ld, const int32_t* group, int32_t n_groups,
                   float* out, int32_t accumulate, void* stream);

/* column sums over few columns with the rows split 32 ways (fixed-order partials; workspace
 * gmr_colsum_split_floats(cols) floats) — bias gradients of the B x 512 transformer products */
int64_t gmr_colsum_split_floats(int64_t cols);
int gmr_colsum_split_f32(int64_t rows, int64_t cols, const float* x, int64_t ld, float* out, int32_t accumulate,
                         float* workspace, int64_t workspace_floats, void* stream);

/* ---------------------------------------------------------------- BPR epoch sampler (dataloader.py:218-275)
 * shuffled interactions + one rejection-sampled negative from `all_items` per interaction (redrawn while
 * in the user's history); rows still without a true negative after 4096 draws are added to
 * *n_fallback (may be NULL; the caller zeroes it) and keep their last draw. */
int gmr_sample_epoch(int64_t n_inter, const int32_t* inter_user, const int32_t* inter_item, const int32_t* user_rowptr,
                     const int32_t* user_items, const int32_t* all_items, int64_t n_all_items, uint64_t seed,
                     uint64_t epoch, int32_t* out_users, int32_t* out_pos, int32_t* out_neg, int32_t* n_fallback,
                     void* stream);
/* random permutation of [0, n) (DataLoader(shuffle=True) over users, trainer.py:462) */
int gmr_permutation(int64_t n, uint64_t seed, uint64_t epoch, int32_t* out, void* stream);

/* ---------------------------------------------------------------- K5/K6 diffusion (diffmm.py:408-484, diffrec.py:182-310)
 * x_t = sqrt_ac[t]*x0 + sqrt_1mac[t]*eps, times the Denoise input dropout keep/keep_prob when
 * dropout != 0; x0 rows come from the user's train items.  noise/keep may be NULL (Philox).
 * row0: index of row 0 inside the global batch — the Philox draws of a row depend on
 * (seed, step, row0 + b) only, so a batch split over data-parallel ranks draws what one
 * process drawing the whole batch would (trainer.py:491-527).
 * Row strides (ldx, ld_noise / ld_keep of a non-NULL buffer, ld of the loss rows, the three of gc_rows) below the
 * row width are rejected when B > 1; every argument check returns before the first launch. */
int gmr_diff_sample_t(int32_t B, int32_t T, uint64_t seed, uint64_t step, int64_t row0, int32_t* t, void* stream);
int gmr_diff_qsample(int32_t B, int32_t I, const int32_t* users, const int32_t* user_ptr, const int32_t* user_items,
                     const int32_t* t, const float* sqrt_ac, const float* sqrt_1mac, const float* noise,
                     int64_t ld_noise, const float* keep, int64_t ld_keep, float keep_prob, int32_t dropout,
                     uint64_t seed, uint64_t step, int64_t row0, float* x, int64_t ldx, void* stream);
int gmr_diff_densify(int32_t B, int32_t I, const int32_t* users, const int32_t* user_ptr, const int32_t* user_items,
                     float* x, int64_t ldx, void* stream);
int gmr_diff_time_bias(int32_t T, int32_t E, const float* emb_W, const float* emb_b, const float* W1, int64_t ld_w1,
                       int64_t col_off, const float* b1, int32_t H, float* EB, float* temb_out, float* emb_out,
                       void* stream);
int gmr_diff_loss_rows(int32_t B, int32_t I, const int32_t* users, const int32_t* user_ptr, const int32_t* user_items,
                       const int32_t* t, const double* wtab, const float* pt, float* out, int64_t ld, float grad_scale,
                       double* mse_out, double* diff_out, double* loss_out, int32_t write_grad, void* stream);
/* out[c][r] = in[r][c] for a rows x cols fp32 matrix. */
int gmr_transpose_f32(int64_t rows, int64_t cols, const float* in, int64_t ldi, float* out, int64_t ldo,
                      void* stream);
/* First p_sample step on binary x0 rows (models/diffmm.py:408-426 with steps = 0, the loop's
 * first model call): h[b] = tanh(sum over the user's items i of W1T[i, :] + eb), W1T = W1[:, :I]^T
 * (I x H) — the sparse form of the hidden GEMM. */
int gmr_diff_sparse_hidden(int32_t B, int32_t H, const int32_t* users, const int32_t* user_ptr,
                           const int32_t* user_items, const float* W1T, int64_t ldw, const float* eb, float* h,
                           int64_t ldh, void* stream);
/* Folded p_sample chain (round 5; the same p_sample, models/diffmm.py:408-451 and models/diffrec.py:291-310,
 * carried as the hidden pre-activation a = x_t W1[:, :I]^T instead of x_t: a_i = c1_i (h_i P^T + v) +
 * c2_i a_{i+1} with P = W1[:, :I] W2 (H x H), v = W1[:, :I] b2; gmr/denoise.py p_sample_fold).
 * gmr_diff_sparse_pre: the first step from binary x0 rows, a[b] = sum over the user's items of W1T[i, :]
 * and h[b] = tanh(a[b] + eb) (h bit-identical to gmr_diff_sparse_hidden).
 * gmr_tanh_bias_f32: h = tanh(a + bias) per row (rows x cols, cols % 4 == 0, 16-byte aligned). */
int gmr_diff_sparse_pre(int32_t B, int32_t H, const int32_t* users, const int32_t* user_ptr, const int32_t* user_items,
                        const float* W1T, int64_t ldw, const float* eb, float* a, int64_t lda, float* h, int64_t ldh,
                        void* stream);
int gmr_tanh_bias_f32(int64_t rows, int32_t cols, const float* a, int64_t lda, const float* bias, float* h,
                      int64_t ldh, void* stream);
/* DiffRec importance sampling of t (models/diffrec.py:234-250): uniform t and pt = 1 until every
 * t has hist_len recorded losses, then t ~ (1-up) sqrt(mean(hist^2))/sum + up/T, pt = p[t]*T. */
int gmr_diff_sample_t_importance(int32_t B, int32_t T, int32_t hist_len, const double* hist, const int32_t* count,
                                 double uniform_prob, uint64_t seed, uint64_t step, int64_t row0, int32_t* t,
                                 float* pt, void* stream);
/* Lt_history / Lt_count update (models/diffrec.py:279-286), rows applied in batch order; t < 0 skips. */
int gmr_diff_history_update(int32_t B, int32_t T, int32_t hist_len, const int32_t* t, const double* loss,
                            double* hist, int32_t* count, void* stream);
int gmr_diff_gc_rows(int32_t B, const int32_t* users, const int32_t* user_ptr, const int32_t* user_items,
                     const float* item_embeds, int64_t ld_ie, const float* Z, int64_t ldz, float gscale, float* G,
                     int64_t ldg, double* gc_out, void* stream);
int gmr_diff_time_bwd(int32_t T, int32_t E, int32_t H, const float* S, const float* temb, const float* emb,
                      const float* W1, int64_t ld_w1, int64_t col_off, float* dW1, float* db1, float* d_emb_W,
                      float* d_emb_b, int32_t accumulate, void* stream);

/* ---------------------------------------------------------------- K10/K12 eval tail (trainer.py:369-388)
 * ties -> lowest index; k <= 64 */
int gmr_mask_scores_f32(int64_t n, const int32_t* rows, const int32_t* cols, float* scores, int64_t ld, float fill,
                        void* stream);
int gmr_topk_rows_f32(int64_t n_rows, int64_t n_cols, const float* scores, int64_t ld, int32_t k, int32_t* out_idx,
                      int64_t ld_idx, float* out_val, void* stream);
/* K9 + K10 fused (common/trainer.py:379-386 with models/diffmm.py:276-277): per eval row r,
 * scores = user_table[users[r]] . item_table^T (users NULL: row r is user r), the row's train positives
 * mask_cols[mask_ptr[r] .. mask_ptr[r+1]) (sorted ascending within a row) set to `fill` (-1e10), then
 * the top-k item indices (score desc, ties -> lowest index) into out_idx[r * ld_idx + j] and,
 * if out_val is not NULL, their scores.  No n_rows x n_items buffer; dim 64 or 128; k <= 64.
 * mask_ptr holds n_rows + 1 absolute offsets into mask_cols (pass &ptr[first row] for a slice). */
int gmr_score_topk_f32(int64_t n_rows, const int32_t* users, const float* user_table, int64_t ld_user, int64_t n_items,
                       const float* item_table, int64_t ld_item, int64_t dim, const int64_t* mask_ptr,
                       const int32_t* mask_cols, float fill, int32_t k, int32_t* out_idx, int64_t ld_idx,
                       float* out_val, void* stream);
/* The same with the scores on the bf16 matrix cores (round 4): the item table as a plane set
 * (gmr_split3_planes: item_planes[p * plane_stride + i * ld_plane + c], x = hi + mid + lo exactly) and
 * the six-product split of GMR_GEMM_X6 (fp32-accurate sums, 2.7x the fp32 MFMA rate); the user
 * table stays fp32 and is split in registers.  dim 64; ld_plane a multiple of 8. */
int gmr_score_topk_x6(int64_t n_rows, const int32_t* users, const float* user_table, int64_t ld_user, int64_t n_items,
                      const uint16_t* item_planes, int64_t ld_plane, int64_t plane_stride, int64_t dim,
                      const int64_t* mask_ptr, const int32_t* mask_cols, float fill, int32_t k, int32_t* out_idx,
                      int64_t ld_idx, float* out_val, void* stream);
/* Recall/NDCG/Precision/MAP sums over users at ks (topk_evaluator.py:107-120, metrics.py):
 * out_sums[metric*8 + j], metric 0 recall 1 ndcg 2 precision 3 map, j < n_ks (fp64). */
int64_t gmr_eval_metrics_partials(int64_t n_users);
int gmr_eval_metrics(int64_t n_users, const int32_t* topk, int64_t ld_topk, int32_t K, const int64_t* pos_ptr,
                     const int32_t* pos_items, int32_t n_ks, const int32_t* ks, double* partials, double* out_sums,
                     void* stream);
/* The same sums over the eval-user rows sel[0 .. n_sel) only, each scored against its own row of
 * (pos_ptr, pos_items): the test-time group metrics (Pop/Niche positives, Cold/Warm users,
 * topk_evaluator.py:122-200).  partials: gmr_eval_metrics_partials(n_sel) doubles. */
int gmr_eval_metrics_sel(int64_t n_sel, const int32_t* sel, const int32_t* topk, int64_t ld_topk, int32_t K,
                         const int64_t* pos_ptr, const int32_t* pos_items, int32_t n_ks, const int32_t* ks,
                         double* partials, double* out_sums, void* stream);
/* counts[j * n_items + i] = times item i appears in the first ks[j] columns of topk (ks ascending, <= 64, n_ks <= 8):
 * Coverage / Gini / Tail% (topk_evaluator.py:212-270). */
int gmr_topk_item_counts(int64_t n_users, const int32_t* topk, int64_t ld_topk, int32_t n_ks, const int32_t* ks,
                         int64_t n_items, int32_t* counts, void* stream);

/* ---------------------------------------------------------------- GenRecV1 rec step (models/genrecv1.py:225-427)
 * Tables are rows x 64 fp32.  BatchNorm1d(64) (eps, momentum as nn.BatchNorm1d): train mode uses
 * batch statistics and updates run_mean/run_var (unbiased var); eval mode uses them.  Fused:
 * y = act(BN(z)) [* keep * keep_scale] (act 0 none, 1 leaky(slope), 2 sigmoid, 3 tanh) and the
 * post op: 0 none, 1 out2 = rs[0]*aux + y (res_scale residual, :229), 2 out2 = aux*y (gate product,
 * :268), 3 rowdot[r] = <y_r, aux[0:64]> (Linear(64, 1, bias=False), :88).
 * Replaces nn.BatchNorm1d + activation + Dropout chains at genrecv1.py:84-89,155-164,166-222.
 * parts: gmr_bn_parts_doubles(rows) doubles; mean/invstd: 64 floats each (saved for backward). */
int64_t gmr_bn_parts_doubles(int64_t rows);
int gmr_bn_fwd_f32(int64_t rows, const float* z, int64_t ldz, int32_t train, float eps, float momentum, float* run_mean,
                   float* run_var, double* parts, float* mean, float* invstd, const float* w, const float* b,
                   int32_t act, float slope, const uint8_t* keep, int64_t ld_keep, float keep_scale, float* y,
                   int64_t ldy, int32_t post, const float* aux, int64_t ld_aux, const float* rs, float* out2,
                   int64_t ld2, float* rowdot, void* stream);
/* backward of the above (train mode): upstream = dy (* mul) or, for post 3, da[r] * v[c]; writes
 * dz (accumulated if asked), dw/db (and dv for post 3, of the kept and scaled activation; accumulated if asked);
 * sums: 128 floats.  Forward and backward read and write rows as float4: every ld a multiple of 4, at least 64. */
int gmr_bn_bwd_f32(int64_t rows, const float* z, int64_t ldz, const float* mean, const float* invstd, const float* w,
                   const float* b, int32_t act, float slope, const uint8_t* keep, int64_t ld_keep, float keep_scale,
                   const float* dy, int64_t lddy, const float* mul, int64_t ld_mul, const float* da, const float* v,
                   double* parts, float* sums, float* dw, float* db, float* dv, int32_t accumulate_params, float* dz,
                   int64_t lddz, int32_t accumulate_dz, void* stream);
/* content = w0 (E + A1)/2 + w1 (E + A2)/2, w = softmax(origin_weight, generation_weight) (:255-264,:332-336)
 * and its backward (T_k = A_k^T dC; dE += ... + reg2 E; d(ow, gw) accumulated); parts: gmr_gr_parts doubles */
int64_t gmr_gr_parts(int64_t n);
int gmr_gr_content_fwd(int64_t n, const float* E, const float* A1, const float* A2, const float* ow, const float* gw,
                       float* C, void* stream);
int gmr_gr_content_bwd(int64_t n, const float* E, const float* A1, const float* A2, const float* dC, const float* T1,
                       const float* T2, const float* ow, const float* gw, float reg2, double* parts, float* dE,
                       float* dow, float* dgw, void* stream);
/* gate_attention_fusion + prefer gates (:309-353): SIDE = (PI (IMG-COM) + PT (TXT-COM) + COM)/4 */
int gmr_gr_fusion_fwd(int64_t n, const float* IMG, const float* TXT, const float* aI, const float* aT,
                      const float* PI, const float* PT, float* SIDE, float* alpha, void* stream);
int gmr_gr_fusion_bwd(int64_t n, const float* IMG, const float* TXT, const float* alpha, const float* PI,
                      const float* PT, const float* dSIDE, float* dIMG, float* dTXT, float* daI, float* daT,
                      float* dPI, float* dPT, void* stream);
/* out (+)= scale * a * b (rows x 64); out = sum(a * b) * scale (+ out), deterministic (parts >= 1024 doubles) */
int gmr_mul64_f32(int64_t rows, const float* a, int64_t lda, const float* b, int64_t ldb, float* out, int64_t ldo,
                  float scale, int32_t accumulate, void* stream);
int gmr_dot64_f32(int64_t rows, const float* a, int64_t lda, const float* b, int64_t ldb, double* parts, float scale,
                  float* out, int32_t accumulate, void* stream);
/* InfoNCE rows on L = v1 v2^T / temp (B x B, in place; :407-414): loss[r] = lse(L_r) - L_rr and
 * L <- coef (softmax - I) for the two gradient GEMMs (coef 0: loss only) */
int gmr_nce_rows_f32(int64_t B, float* L, int64_t ld, float coef, float* loss, void* stream);
/* the same for a data-parallel rank's block: rows [diag_off, diag_off + rows) of the global batch
 * against all cols keys (row r's positive at column diag_off + r; genrecv1.py:407-414 over the
 * global batch) */
int gmr_nce_rows_off_f32(int64_t rows, int64_t cols, float* L, int64_t ld, int64_t diag_off, float coef, float* loss,
                         void* stream);
/* GenRecV1's in-batch InfoNCE terms through gmr_contrast_fused_f32 (round 4; genrecv1.py:389-397): term k
 * pairs the normalised query table i1[k] with key table i2[k] of nv [4][tab][64] (i1 / i2: host arrays of
 * nterms <= 4 entries; Bg rows used per table).  gmr_nce_pairs_f32 writes the (query, positive) pair rows
 * CLN [nterms][ct][128] of the rank's rows [row0, row0 + B); after one contrast call per term (contrib
 * [nterms][ct][128], dT [nterms][dts][64]) gmr_nce_combine_f32 writes every nv row's gradient g [4][tab][64],
 * summed in term order. */
int gmr_nce_pairs_f32(int32_t nterms, int64_t B, int64_t Bg, int64_t row0, const int32_t* i1, const int32_t* i2,
                      const float* nv, int64_t tab, float* cln, int64_t ct, void* stream);
int gmr_nce_combine_f32(int32_t nterms, int64_t B, int64_t Bg, int64_t row0, const int32_t* i1, const int32_t* i2,
                        const float* contrib, int64_t ct, const float* dT, int64_t dts, float* g, int64_t tab,
                        void* stream);
/* BPR with log-sigmoid (:377-380) over one (U + I) x 64 table; contrib = [dU; dP; dN] */
int gmr_bpr_logsigmoid_f32(int32_t B, int64_t U, const float* C, const int32_t* users, const int32_t* pos,
                           const int32_t* neg, float* loss, float* contrib, float inv_norm, void* stream);

/* y += alpha[0] x (device scalar); out = a * b (flat); Bernoulli(p_keep) keep bytes (nn.Dropout masks) */
int gmr_axpy_dev_f32(int64_t n, const float* alpha, const float* x, float* y, void* stream);
int gmr_mul_f32(int64_t n, const float* a, const float* b, float* out, void* stream);
/* keep byte i uses Philox counter ctr0 + i (a data-parallel rank's rows: ctr0 = first global row x row length) */
int gmr_keep_mask_u8(int64_t n, float p_keep, uint64_t seed, uint64_t step, uint64_t ctr0, uint8_t* out, void* stream);

/* ---------------------------------------------------------------- GenRecV1 graphs (§8a G2, G6)
 * CSR transpose (columns ascending in every output row, values carried); workspace 2*n_cols ints,
 * stage_col/stage_val nnz entries.  Backward of the non-symmetric SpMMs (dropped UI graph, kNN, R). */
int gmr_csr_transpose(int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t* rowptr, const int32_t* col,
                      const float* val, int32_t* workspace, int32_t* t_rowptr, int32_t* t_col, float* t_val,
                      int32_t* stage_col, float* stage_val, void* stream);
/* SpAdjDropEdge (:443-457): keep e iff floor(u_e + keep_rate) >= 1 (Philox u, or keep[e]); values / keep_rate.
 * Two calls: counts + out_rowptr (workspace n_rows ints), then the compaction.  transposed = 1 on a
 * structurally symmetric matrix gives (dropped A)^T directly (entry (r, c) takes the flag of (c, r)). */
int gmr_csr_drop_count(int64_t n_rows, const int32_t* rowptr, const int32_t* col, int32_t transposed,
                       const uint8_t* keep, float keep_rate, uint64_t seed, uint64_t step, int32_t* workspace,
                       int32_t* out_rowptr, void* stream);
int gmr_csr_drop_write(int64_t n_rows, const int32_t* rowptr, const int32_t* col, const float* val,
                       int32_t transposed, const uint8_t* keep, float keep_rate, uint64_t seed, uint64_t step,
                       const int32_t* out_rowptr, int32_t* out_col, float* out_val, void* stream);
/* kNN graph from per-row top-k (idx, sim) (utils/utils.py:184-197, 'sym'): deg = row sums of the
 * kept sims (top-k order), w = d_r v d_c, d = deg^-1/2 (inf -> 0); rowptr n+1, col/val n*k */
int gmr_knn_symnorm_csr(int64_t n, int32_t k, const int32_t* topi, int64_t ldi, const float* topv, int64_t ldv,
                        float* dis_ws, int32_t* rowptr, int32_t* col, float* val, void* stream);
/* rebuild (common/trainer.py:752-754): den = x0 with the gen_topk positions taken from xs */
int gmr_gen_mask(int32_t B, int32_t I, int32_t k, const int32_t* topi, int64_t ldt, const float* x0, const float* xs,
                 int64_t ld, float* den, void* stream);
/* InterestDebiase (interest_cluster.py:186-332): exact-n uniform picks of 0->1 / 1->0 flips among the
 * gen_topk positions (n = int(count * ratio)); picks[type][max_picks][2] = (row, item), n_picks[2];
 * then the cluster rules (labels < 64) applied to den in place */
int gmr_debias_select(int32_t B, int32_t k, const int32_t* topi, int64_t ldt, const float* x0, const float* xs,
                      int64_t ld, float ratio, uint64_t seed, uint64_t step, uint64_t* keys_ws /* 2*B*k */,
                      int32_t* picks, int32_t max_picks, int32_t* n_picks, void* stream);
int gmr_debias_apply(int32_t type, const int32_t* picks, const int32_t* n_picks, int32_t max_picks, const float* x0,
                     int64_t ld0, int32_t I, const int32_t* labels, float* den, int64_t ldd, void* stream);
/* K-means pieces (interest_cluster.py:60-79 — StandardScaler + KMeans): distances and centroid sums
 * are GEMMs (gmr_gemm_f32) between these calls */
int gmr_kmeans_standardize(int64_t n, int32_t d, const float* X, int64_t ldx, float* mean, float* scale, float* Y,
                           int64_t ldy, float* sq, void* stream);
int gmr_kmeans_pp_pick(int64_t n, const float* mind, uint64_t seed, uint64_t step, int32_t* out, void* stream);
int gmr_kmeans_take_center(int32_t d, const float* X, int64_t ldx, const int32_t* idx, float* C, int64_t ldc,
                           int32_t j, const float* xsq, float* csq, void* stream);
/* greedy k-means++ step (sklearn's default seeding: L = 2 + floor(ln k) candidates, round 4): given dots =
 * X . Cc^T (n x L) of the candidate rows Cc and their squared norms ccsq, picks the candidate of the lowest
 * potential sum_r min(mind[r], |x_r - c|^2) (fixed-order sums, ties -> lowest), copies it to C[j], sets
 * csq[j] and lowers mind. */
int gmr_kmeans_pp_greedy(int64_t n, int32_t L, const float* xsq, const float* dots, int64_t ldd, const float* ccsq,
                         float* mind, const float* Cc, int64_t ldcc, int32_t d, float* C, int64_t ldc, int32_t j,
                         float* csq, void* stream);
int gmr_kmeans_min_dist(int64_t n, const float* xsq, const float* dots, int64_t ld_dots, const float* csq, int32_t j,
                        float* mind, int32_t first, void* stream);
int64_t gmr_kmeans_parts(int64_t n);
int gmr_kmeans_assign(int64_t n, int32_t k, const float* dots, int64_t ldd, const float* csq, const float* xsq,
                      int32_t* label, float* onehot_t, int64_t ldo, int32_t* changed, double* inertia_parts,
                      void* stream);
int gmr_kmeans_centroids(int32_t k, int32_t d, const float* sums, int64_t lds, const float* onehot_t, int64_t ldo,
                         int64_t n, float* C, int64_t ldc, float* csq, void* stream);

/* ---------------------------------------------------------------- GenRecV1 generation (§8a G4, G5)
 * FlipInterestDiffusion (models/genrecv1.py:460-648).  tables = [gamma_cum (T) | eps_cum (T) |
 * pos_weight | sparsity] from the batch users' history sizes (get_cum, :480-498). */
int gmr_flip_schedule(int32_t B, const int32_t* users, const int32_t* user_ptr, int32_t I, int32_t T, float* tables,
                      void* stream);
/* q_sample (:512-526): x_t = x0 xor Bernoulli(sigmoid((a_t - u) temp)); flip (0/1 bytes) replaces the draws.
 * Draws are keyed by (step, global row row0 + b, item), so a data-parallel rank holding rows
 * [row0, row0 + B) of a batch draws what one process holding the whole batch draws. */
int gmr_flip_qsample(int32_t B, int32_t I, const float* x0, int64_t ld0, const int32_t* t, int32_t t_const,
                     const float* tables, int32_t T, float temp, const uint8_t* flip, int64_t ld_flip, uint64_t seed,
                     uint64_t step, int64_t row0, float* xt, int64_t ldt, void* stream);
/* one p_sample step on the model logits (:536-548); probs may be NULL; draws keyed as gmr_flip_qsample */
int gmr_flip_step(int32_t B, int32_t I, const float* z, int64_t ldz, const float* tables, int32_t T, int32_t qi,
                  int32_t last,
                  const uint8_t* draws, int64_t ldd, uint64_t seed, uint64_t step, int64_t row0, float* x, int64_t ldx,
                  float* probs, int64_t ldp, void* stream);
/* BCE(pos_weight) + curriculum KL rows (:550-627); dz = grad_scale * dBCE/dz (may alias z) */
int gmr_flip_loss_rows(int32_t B, int32_t I, const float* x0, int64_t ld0, const float* z, int64_t ldz,
                       const int32_t* t, const float* tables, int32_t T, float grad_scale, float* dz, int64_t lddz,
                       double* bce_row, double* kl_row, void* stream);
/* [bce, kl, cl, bce + kl + w_cl cl] (training_losses total, :604) */
int gmr_flip_total(const double* bce_kl, const float* cl, float w_cl, float* out4, void* stream);
/* ModalDenoiseTransformer rows (:650-710).  LayerNorm over D (64..1024) of s = a + keep*scale*b
 * (b a matrix, or a broadcast row when ldb == 0; keep may be NULL), optional exact GELU after;
 * saves s, mean, rstd.  Backward: dx (+)=, dw/db (+)= through parts (gmr_layernorm_parts_floats). */
int gmr_layernorm_fwd(int64_t rows, int32_t D, const float* a, int64_t lda, const float* b, int64_t ldb,
                      const uint8_t* keep, int64_t ld_keep, float keep_scale, const float* w, const float* bias,
                      float eps, int32_t gelu, float* y, int64_t ldy, float* s_out, int64_t lds, float* mean,
                      float* rstd, void* stream);
/* The same with the residual-branch dropout drawn in the kernel (nn.Dropout on the decoder layer's branch,
 * :650-710): keep_out[r][c] = (Philox(seed, step, ctr0 + r D + c).x >> 8) / 2^24 < p_keep (gmr_keep_mask_u8's
 * key, so the bytes equal a gmr_keep_mask_u8 draw of rows x D at ctr0) is stored and applied; one launch
 * instead of the mask launch + gmr_layernorm_fwd.  b must be a matrix (ldb > 0). */
int gmr_layernorm_drop_fwd(int64_t rows, int32_t D, const float* a, int64_t lda, const float* b, int64_t ldb,
                           float p_keep, uint64_t seed, uint64_t step, uint64_t ctr0, uint8_t* keep_out,
                           int64_t ld_keep, float keep_scale, const float* w, const float* bias, float eps,
                           int32_t gelu, float* y, int64_t ldy, float* s_out, int64_t lds, float* mean, float* rstd,
                           void* stream);
int64_t gmr_layernorm_parts_floats(int64_t rows, int32_t D);
int gmr_layernorm_bwd(int64_t rows, int32_t D, const float* s, int64_t lds, const float* mean, const float* rstd,
                      const float* w, const float* bias, int32_t gelu, const float* dy, int64_t lddy, float* dx,
                      int64_t lddx, int32_t accumulate_dx, float* parts, float* dw, float* db,
                      int32_t accumulate_params, void* stream);
/* adaLN (:702-703): h1 = h0 (1 + scale[t]) + shift[t], S = T x 2D [shift | scale]; backward writes
 * dh0 and prod = dh1 * h0 (grouped column sums give dscale / dshift, gmr_colsum_f32) */
int gmr_adaln_fwd(int64_t rows, int32_t D, const float* h0, int64_t ld0, const int32_t* t, int32_t t_const,
                  const float* S, int64_t lds, float* h1, int64_t ld1, void* stream);
int gmr_adaln_bwd(int64_t rows, int32_t D, const float* h0, int64_t ld0, const float* dh1, int64_t ldd,
                  const int32_t* t, const float* S, int64_t lds, float* dh0, int64_t ldo, float* prod, int64_t ldp,
                  void* stream);
/* dropout with keep probability p_keep, one draw per (row, column / group) (group = head size for
 * the attention-weight dropout of a length-1 sequence); mask_in replays a mask, mask_out records it */
int gmr_dropout_f32(int64_t rows, int32_t D, int32_t group, const float* x, int64_t ldx, float p_keep,
                    const uint8_t* mask_in, uint8_t* mask_out, int64_t ldm, uint64_t seed, uint64_t step, int64_t row0,
                    float* y, int64_t ldy, void* stream);
/* Cross-attention of the decoder layers on their all-zero memory (models/genrecv1.py:650-710): head h
 * outputs the value bias bv'_h on every row, so with head dropout the block is, per row, a mixture of
 * nhead fixed vectors.  gmr_xattn_table_f32: P[l][h][j] = sum_{c in head h} Wo_l[j][c] bv'_l[c] / p_keep
 * for the L layers (layer l's tensors at woc0 / bvc0 + l * layer_stride floats; Wo row-major, ld D).
 * gmr_xattn_fwd_f32: CA[r] = b_o + sum_h keep[r][h] P[h] (keep drawn as gmr_dropout_f32 with group
 * D / nhead draws it, or read from mask_in; mask_out records it).  gmr_xattn_bwd_f32: from dCA (B x D)
 * and the masks, dWo += Gs[h(c)][j] bv'[c] / p_keep and dbv' += sum_j Wo[j][c] Gs[h(c)][j] / p_keep,
 * Gs[h][j] = sum_r keep[r][h] dCA[r][j]; nhead <= 16; ws of gmr_xattn_bwd_workspace_floats floats.
 * They replace the B x D x D out-projection GEMM, its transposed-operand gradient and dBc products. */
int gmr_xattn_table_f32(int32_t L, int32_t D, int32_t nhead, const float* woc0, const float* bvc0,
                        int64_t layer_stride, float p_keep, float* P, void* stream);
int gmr_xattn_fwd_f32(int64_t rows, int32_t D, int32_t nhead, const float* P, const float* bo, float p_keep,
                      const uint8_t* mask_in, uint8_t* mask_out, int64_t ldm, uint64_t seed, uint64_t step, int64_t row0,
                      float* CA, int64_t ldc, void* stream);
int64_t gmr_xattn_bwd_workspace_floats(int64_t rows, int32_t D, int32_t nhead);
int gmr_xattn_bwd_f32(int64_t rows, int32_t D, int32_t nhead, const float* dCA, int64_t ld, const uint8_t* mask,
                      int64_t ldm, const float* wo, const float* bv, float p_keep, float* g_wo, float* g_bv, float* ws,
                      int64_t ws_floats, void* stream);
/* (Round 4's one-launch decoder stack, gmr_decoder_fwd_f32 / _masks_u8 / _split_f32, was removed in round 6:
 * opt-in, slower than the layer-by-layer path at the GenRecV1 batch in every round it was measured.) */
/* The same L decoder layers layer by layer, issued from C++ (csrc/decoder_host.hip, round 5): the kernels and
 * arguments of gmr/transformer.py's Python layer loop (gmr_gemm_f32 NT products with `tile`, gmr_dropout_f32,
 * gmr_layernorm_[drop_]fwd, gmr_xattn_fwd_f32 in train mode; the constant cross-attention row cav = b_v' Wo^T +
 * b_o, recomputed unless reuse_cav, in eval mode), bit-identical to it, without its per-launch Python cost.
 * offsets: 17 slab offsets of layer 0 (Wv = in_proj rows 2D..3D, bv, Wo, bo, norm1 w/b, b_v' = cross in_proj
 * bias + 2D, Wo', bo', norm2 w/b, W1, b1, W2, b2, norm3 w/b), layer l at + l * layer_stride.  bufs: 22 device
 * pointers of the activation workspace with Bmax rows per layer (h [L+1], V, SAin, SA, s1, h1, LN1 stats
 * [L][3][Bmax], CA, s2, h2, F1, F2, s3, LN2 / LN3 stats, cav [L][D], masks a / c [L][Bmax][nhead], masks
 * 1 / 2 / 3 / f [L][Bmax][D]; SAin, CA and the masks may be NULL in eval mode); h[0] is the input, h[L] the
 * output.  gemm_ws: >= gmr_gemm_workspace_floats of the B x D x D and 1 x D x D products (zeroed counters). */
int gmr_decoder_layers_fwd_f32(int64_t B, int64_t Bmax, int32_t L, int32_t D, int32_t nhead, const float* slab,
                               const int64_t* offsets, int64_t layer_stride, int32_t train_drop, float p_keep,
                               uint64_t seed, uint64_t step, int64_t row0, int32_t reuse_cav, const float* xP,
                               void* const* bufs, int32_t tile, float* gemm_ws, int64_t gemm_ws_floats, void* stream);
/* sinusoidal time embedding table T x E (:692-696); SiLU (dy == NULL) or its backward */
int gmr_time_embedding(int32_t T, int32_t E, float* out, void* stream);
int gmr_silu_f32(int64_t n, const float* x, const float* dy, float* y, void* stream);

/* ---------------------------------------------------------------- optimizer (torch.optim.Adam, trainer.py:125-142)
 * flat fp32 slabs; step_size = lr / (1 - b1^t), bias_correction2_sqrt = sqrt(1 - b2^t) */
int gmr_adam_f32(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float beta1,
                 float beta2, float eps, float weight_decay, float step_size, float bias_correction2_sqrt,
                 void* stream);

/* ---------------------------------------------------------------- FREEDOM (models/freedom.py)
 * calculate_loss (:189-210) in one call: loss = bpr(G) + reg_weight * (bpr(T) + bpr(V)) with
 * bpr = -sum(logsigmoid(<u,p> - <u,n>)) * inv_norm over the B rows (the exact F.logsigmoid).  G is the
 * propagated (n_users + I) x 64 table [ua; ia]; T / V are the I x 64 projected text / image tables (either may
 * be NULL: that term and its columns are 0); the user row of all three terms is G[users[b]].  loss = [total,
 * graph, text, image].  contrib (3B x 192, ldc): rows [users | pos | neg], columns [graph | text | image]; a user
 * row carries the three terms' d/du in columns 0:64 and zeros after, so one gmr_scatter_sorted_f32 through the
 * loader's BPR plan (key offsets [0, U, U]) gives the gradient of a (U + I) x 192 table [G | T | V].
 * parts_ws: 3B doubles (per-row terms, summed in a fixed order).  All rows 16-byte aligned. */
int gmr_frd_loss_fwd_bwd(int32_t B, int64_t n_users, const float* G, int64_t ldg, const float* T, int64_t ldt,
                         const float* V, int64_t ldv, const int32_t* users, const int32_t* pos, const int32_t* neg,
                         float reg_weight, float inv_norm, double* parts_ws, float* loss, float* contrib,
                         int64_t ldc, void* stream);
/* Degree-sensitive edge pruning (pre_epoch_processing, :128-143): torch.multinomial(w, m) without replacement
 * as the m largest keys w_e / (-log u_e), u_e = Philox(seed, step, e) in (0, 1] or u[e] when u is given.
 * gmr_frd_prune_select marks the m largest of the n_edges non-negative keys in keep (one byte per edge, exactly
 * m set): radix histogram passes over the key bits find the m-th largest key, ties at it go to the lower edge
 * index.  workspace: gmr_frd_prune_workspace_ints() ints.  m outside [0, n_edges] is an argument error. */
int gmr_frd_prune_keys(int64_t n_edges, const float* w, const float* u, uint64_t seed, uint64_t step, float* keys,
                       void* stream);
int64_t gmr_frd_prune_workspace_ints(void);
int gmr_frd_prune_select(int64_t n_edges, int64_t m, const float* keys, int32_t* workspace, uint8_t* keep,
                         void* stream);
/* mm_adj (:64-100): CSR of w_a A + w_b B for the binary top-k adjacencies A, B (n x k index lists, distinct per
 * row), every entry weight / (k + 1e-7) evaluated as the reference does (pow(k + 1e-7, -0.5) squared, fp32).
 * Columns ascending and distinct per row, an index in both lists gets the summed value; idx_b = NULL: w_a A
 * alone.  stage_col / stage_val: n * 2k entries, count_ws: n ints; rowptr n + 1; col / val up to n * 2k entries
 * (rowptr[n] are used). */
int gmr_frd_knn_union_csr(int64_t n, int32_t k, const int32_t* idx_a, int64_t lda, float w_a, const int32_t* idx_b,
                          int64_t ldb, float w_b, int32_t* stage_col, float* stage_val, int32_t* count_ws,
                          int32_t* rowptr, int32_t* col, float* val, void* stream);
/* forward (:164-178): out = (E_0 + ... + E_{n_layers-1}) / n_layers over n_rows x 64 tables (layers / ld_layers:
 * host arrays), + h[r - n_users] on the rows from n_users (h may be NULL).  With one layer and no h it is a
 * strided 64-column copy (the pre-fill of the backward's Horner chain). */
#define GMR_FRD_MAX_LAYERS 8
int gmr_frd_mean_fwd(int64_t n_rows, int64_t n_users, int32_t n_layers, const float* const* layers,
                     const int64_t* ld_layers, const float* h, int64_t ldh, float* out, int64_t ldo, void* stream);

/* ---------------------------------------------------------------- rectified-flow generator (models/rf_modules.py)
 * SimpleVelocityNet with embedding_dim 64 and hidden_dim 128, condition_dim C in {64, 128, 192}, L = rf_n_layers in 1..4.
 * params: the net's named_parameters() order, every tensor dense and row-major (gmr_rf_param_floats(C, L) floats,
 * 16-byte aligned): time_embed.1 {W 128x64, b}; condition_encoder {W 128xC, b, LN w, LN b}; input_proj {W 128x64, b,
 * LN w, LN b}; L x res_blocks {W, b, LN w, LN b, W, b, LN w, LN b}; output_proj {W 128x128, b, LN w, LN b, W 64x128,
 * b 64}.  LayerNorm: eps 1e-5, biased variance. */
int64_t gmr_rf_param_floats(int32_t C, int32_t L); /* -1 outside the supported range */
int32_t gmr_rf_tile_rows(void);                    /* rows a workgroup of gmr_rf_sample owns */
/* generate() (:896-975): z <- z + net(z, i / n_steps, cond) / n_steps for i = 0 .. n_steps - 1 from z0, dropout and
 * guidance off, the whole loop in one launch.  z0 N x 64 (ldz), cond N x C (ldc), out N x 64 (ldo); any N >= 1 (tail
 * rows are masked).  A row's result does not depend on N or on the rows around it.  The condition product runs in K
 * chunks of at most 128 columns into one accumulator (two chunks at C = 192), in one fixed order per row.  hidden != 128, C or L outside
 * the range: GMR_ERR_ARG. */
int gmr_rf_sample(int64_t N, int32_t hidden, int32_t C, int32_t L, int32_t n_steps, const float* z0, int64_t ldz,
                  const float* cond, int64_t ldc, const float* params, float* out, int64_t ldo, void* stream);
/* The same launch with the evaluation's mix as its epilogue: out[r] = base[r] + ratio[0] * z[r] with z the rows
 * gmr_rf_sample writes from the same arguments, one fused multiply-add per element; z itself is not written.  base
 * N x 64 with a row stride ldb of its own, ratio a device scalar (read by the kernel, so a captured graph sees a
 * changed ratio), out N x 64 (ldo); columns of out beyond 64 are not written.  base must not alias out.  A NULL base
 * or ratio, ldb or ldo below 64 or no multiple of 4, base or out not 16-byte aligned: GMR_ERR_ARG, next to
 * gmr_rf_sample's own. */
int gmr_rf_sample_mix(int64_t N, int32_t hidden, int32_t C, int32_t L, int32_t n_steps, const float* z0, int64_t ldz,
                      const float* cond, int64_t ldc, const float* params, const float* base, int64_t ldb,
                      const float* ratio, float* out, int64_t ldo, void* stream);
/* Rows of the training step over N x 128 contiguous tables:
 *   out = drop(silu(LN(y) [+ res])) [+ add1] [+ add2],  drop(x) = mask ? x * keep_scale : 0
 * ln_w == ln_b == NULL: no LayerNorm; res, mask, add1, add2 may be NULL.  Backward from dout = dL/dout: dy = dL/dy,
 * dres (may be NULL) = the gradient of the pre-activation, which is the residual input's share; d_ln_w / d_ln_b are
 * per-block partial sums (parts: gmr_rf_act_parts_floats(N) floats) added up in one fixed order. */
int gmr_rf_act_fwd(int64_t N, const float* y, const float* ln_w, const float* ln_b, const float* res,
                   const uint8_t* mask, float keep_scale, const float* add1, const float* add2, float* out,
                   void* stream);
int64_t gmr_rf_act_parts_floats(int64_t N);
int gmr_rf_act_bwd(int64_t N, const float* y, const float* ln_w, const float* ln_b, const float* res,
                   const uint8_t* mask, float keep_scale, const float* dout, float* dy, float* dres, float* parts,
                   float* d_ln_w, float* d_ln_b, void* stream);
/* SinusoidalPositionEmbedding(64) of t (N) -> N x 64 (:296-320) */
int gmr_rf_time_embed(int64_t N, const float* t, float* out, void* stream);
/* X_t = t X1 + (1 - t) X0 (:855); X1 N x 64 with ld1, the rest contiguous */
int gmr_rf_interp(int64_t N, const float* X1, int64_t ld1, const float* X0, const float* t, float* Xt, void* stream);
/* Head (:859-869): V (the net's output, in place) += (1 - t)^2 guidance_scale cosine_similarity_gradient(X_t, X1);
 * row_parts[r] = sum_c (V - (X1 - X0))^2 in fp64; pred = X_t + (1 - t) V.
 * Backward: dV = 2 (V - (X1 - X0)) / (64 N) + (1 - t) dpred. */
int gmr_rf_head_fwd(int64_t N, float* V, const float* Xt, const float* X1, int64_t ld1, const float* X0,
                    const float* t, float guidance_scale, float* pred, double* row_parts, void* stream);
/* The head with the user-prior guidance term (:457-476, the backbones that pass user_prior): with lam = (1 - t)^2,
 * V <- (V + lam prior_scale prior) + lam cos_scale cosine_similarity_gradient(X_t, X1), the two terms added in the
 * reference's order; prior N x 64 with row stride ldp >= 64.  row_parts, pred and the backward (which reads the
 * updated V; both terms are constants of the parameters) are gmr_rf_head_fwd's.  An all-zero prior gives
 * gmr_rf_head_fwd's result bit for bit. */
int gmr_rf_head_prior_fwd(int64_t N, float* V, const float* Xt, const float* X1, int64_t ld1, const float* X0,
                          const float* t, const float* prior, int64_t ldp, float prior_scale, float cos_scale,
                          float* pred, double* row_parts, void* stream);
int gmr_rf_head_bwd(int64_t N, const float* V, const float* X1, int64_t ld1, const float* X0, const float* t,
                    const float* dpred, float* dV, void* stream);
/* RFBM3's RF inputs (models/rfbm3.py:107-175) from BM3's projected item tables T = text_trs(text), V =
 * image_trs(image) (I x 64, strides ldt / ldv; either may be NULL): the item rows U .. U + I - 1 of cond ((U + I) x
 * C, ldc) = [V | T] (C = 128; one table: that block alone, C = 64) and of prior ((U + I) x 64, ldp) = Z - mean over
 * the items of Z, Z = V + T.  The user rows are never touched (zero in the reference; the caller zeroes them
 * once).  The column means are block partials added in one fixed order: no float atomics, two runs are
 * bit-identical.  ws: gmr_rf_item_inputs_ws_floats(I) floats.  All pointers 16-byte aligned, strides multiples of
 * 4 floats. */
int64_t gmr_rf_item_inputs_ws_floats(int64_t I);
int gmr_rf_item_inputs(int64_t I, int64_t U, const float* T, int64_t ldt, const float* V, int64_t ldv, float* cond,
                       int64_t ldc, float* prior, int64_t ldp, float* ws, void* stream);
/* RFMGCN's prior (models/rfmgcn.py:156-172) from MGCN's two modal views a, b ((U + I) x 64, strides lda / ldb; in the
 * model both are column blocks of one 128-wide table): prior[r] = Z[r] - mean_seg(r)(Z), Z = 0.5 (a + b), the mean
 * over the U user rows for r < U and over the I item rows otherwise.  prior is (U + I) x 64 with stride ldp; nothing
 * outside that block is written.  The grid is the user blocks followed by the item blocks (128 rows each), so the
 * item segment starts at row U for every U; the column means are block partials added in one fixed order by one
 * workgroup per segment: no float atomics, two runs are bit-identical.  1 <= U, I <= 2^31 - 128 (GMR_ERR_ARG
 * otherwise: the mean over an empty segment is NaN in the reference; _ws_floats returns -1).  ws:
 * gmr_rf_view_prior_ws_floats(U, I) floats.  All pointers 16-byte aligned, strides multiples of 4 floats. */
int64_t gmr_rf_view_prior_ws_floats(int64_t U, int64_t I);
int gmr_rf_view_prior(int64_t U, int64_t I, const float* a, int64_t lda, const float* b, int64_t ldb, float* prior,
                      int64_t ldp, float* ws, void* stream);
/* RFLGMRec's prior (models/rflgmrec.py:125-143) from LGMRec's two propagated modal views a, b (the column blocks of
 * the (U + I) x 128 table mge): Z = a + b, a sum and no mean of the views; the arguments, the segments, the grid,
 * the fixed-order means, the limits and the workspace are gmr_rf_view_prior's. */
int64_t gmr_rf_view_sum_prior_ws_floats(int64_t U, int64_t I);
int gmr_rf_view_sum_prior(int64_t U, int64_t I, const float* a, int64_t lda, const float* b, int64_t ldb, float* prior,
                          int64_t ldp, float* ws, void* stream);
/* RFSMORE's RF inputs (models/rfsmore.py:165-195) from SMORE's three views a, b, f and the fusion preference gate g
 * of the step, dropout mask and scale included ((U + I) x 64 each, every one with a stride of its own: column blocks
 * of a 192-wide and a 448-wide table in the model): cond ((U + I) x 192, ldc) = [a | b | g f], the first two blocks
 * copies and the third the rounded fp32 product; prior ((U + I) x 64, ldp) = Z - mean_seg(Z), Z = (a + b + g f) / 3
 * with that same product, the segments, the grid and the fixed-order means as gmr_rf_view_prior.  Nothing outside
 * the two blocks is written.  1 <= U, I <= 2^31 - 128 (GMR_ERR_ARG otherwise; _ws_floats returns -1).  ws:
 * gmr_rf_view3_inputs_ws_floats(U, I) floats.  All pointers 16-byte aligned, strides multiples of 4 floats. */
int64_t gmr_rf_view3_inputs_ws_floats(int64_t U, int64_t I);
int gmr_rf_view3_inputs(int64_t U, int64_t I, const float* a, int64_t lda, const float* b, int64_t ldb, const float* f,
                        int64_t ldf, const float* g, int64_t ldg, float* cond, int64_t ldc, float* prior, int64_t ldp,
                        float* ws, void* stream);
/* out3 = [rf_loss = sum(row_parts) / (64 N), cl_loss = sum(cl_parts[0 : 2B]) / B, rf_loss + weight cl_loss] */
int gmr_rf_losses(int64_t N, const double* row_parts, int64_t B, const double* cl_parts, float weight, float* out3,
                  void* stream);
/* _infonce_loss_interaction_based (:717-777) for B anchors idx[b] of one side (rows row_off + idx of pred and
 * target, n rows on that side): n_neg negatives per anchor from neg (B x n_neg, side-relative) or, neg == NULL,
 * drawn uniformly by Philox (seed, step, site; counter b n_neg + slot); a negative equal to the positive becomes
 * (neg + 1) % n.  As the reference (:762, F.normalize over dim 1 of the (B, n_neg, 64) gather), a negative's column c
 * is divided by the norm of column c over the anchor's n_neg negatives; the anchor and the positive are
 * row-normalised.  parts[b] = -log(pos / (pos + sum neg)) in fp64; contrib[b] = coef * dloss_b / dpred[idx[b]] through
 * the normalisation (the target side is constant), for gmr_scatter_sorted_f32. */
int gmr_rf_infonce_sampled_fwd_bwd(int32_t B, int64_t n, const float* pred, int64_t ldp, const float* target,
                                   int64_t ldt, int64_t row_off, const int32_t* idx, int32_t n_neg, const int32_t* neg,
                                   uint64_t seed, uint64_t step, uint64_t site, float inv_temp, float coef,
                                   double* parts, float* contrib, int64_t ldc, void* stream);
/* ---- the generator at row width DW (the _w entry points).  The concat-fusion backbones generate rows as wide as
 * their conditions: embedding_dim DW with condition_dim C, (DW, C) in {(64, 64), (64, 128), (64, 192), (128, 128),
 * (192, 192)}.  The packed parameters are the same order with input_proj W 128 x DW and output_proj {W DW x 128,
 * b DW}; the sinusoidal time embedding stays 64 wide.  Every _w entry at DW = 64 is the entry without the suffix,
 * bit for bit (one kernel behind both names); every table that was N x 64 is N x DW, with the same stride and
 * alignment rules.  Any other width: GMR_ERR_ARG (gmr_rf_param_floats_w: -1). */
int64_t gmr_rf_param_floats_w(int32_t DW, int32_t C, int32_t L);
/* gmr_rf_sample / gmr_rf_sample_mix with z0, out and base N x DW.  A workgroup still owns 32 rows; its z tile is
 * 32 x (DW + 4) floats and the output projection runs over DW / 32 column tiles shared among the four waves, every
 * element's sum in one fixed order.  The wide instantiations take 66.75 KB (DW = 128) / 74.75 KB (DW = 192) of
 * dynamic LDS, so two workgroups share a CU. */
int gmr_rf_sample_w(int64_t N, int32_t hidden, int32_t DW, int32_t C, int32_t L, int32_t n_steps, const float* z0,
                    int64_t ldz, const float* cond, int64_t ldc, const float* params, float* out, int64_t ldo,
                    void* stream);
int gmr_rf_sample_mix_w(int64_t N, int32_t hidden, int32_t DW, int32_t C, int32_t L, int32_t n_steps, const float* z0,
                        int64_t ldz, const float* cond, int64_t ldc, const float* params, const float* base,
                        int64_t ldb, const float* ratio, float* out, int64_t ldo, void* stream);
/* The row kernels over N x DW tables, DW in {64, 128, 192}: X1 (ld1) and prior (ldp) keep row strides of their own,
 * the rest are contiguous.  The head is one wave per row with DW / 64 columns per lane; norms, dots and the fp64
 * squared error run over the whole row.  gmr_rf_head_bwd_w and gmr_rf_losses_w divide by DW N. */
int gmr_rf_interp_w(int64_t N, int32_t DW, const float* X1, int64_t ld1, const float* X0, const float* t, float* Xt,
                    void* stream);
int gmr_rf_head_fwd_w(int64_t N, int32_t DW, float* V, const float* Xt, const float* X1, int64_t ld1, const float* X0,
                      const float* t, float guidance_scale, float* pred, double* row_parts, void* stream);
int gmr_rf_head_prior_fwd_w(int64_t N, int32_t DW, float* V, const float* Xt, const float* X1, int64_t ld1,
                            const float* X0, const float* t, const float* prior, int64_t ldp, float prior_scale,
                            float cos_scale, float* pred, double* row_parts, void* stream);
int gmr_rf_head_bwd_w(int64_t N, int32_t DW, const float* V, const float* X1, int64_t ld1, const float* X0,
                      const float* t, const float* dpred, float* dV, void* stream);
int gmr_rf_losses_w(int64_t N, int32_t DW, const double* row_parts, int64_t B, const double* cl_parts, float weight,
                    float* out3, void* stream);
/* gmr_rf_infonce_sampled_fwd_bwd over DW-wide rows: a 16-lane group holds a row as DW / 64 float4 per lane, four
 * negatives per wave; the Philox indexing (so the drawn indices for one key are those of every width), the collision
 * rule and the per-column normalisation over the anchor's negatives are unchanged.  contrib rows are DW wide. */
int gmr_rf_infonce_sampled_fwd_bwd_w(int32_t B, int64_t n, int32_t DW, const float* pred, int64_t ldp,
                                     const float* target, int64_t ldt, int64_t row_off, const int32_t* idx,
                                     int32_t n_neg, const int32_t* neg, uint64_t seed, uint64_t step, uint64_t site,
                                     float inv_temp, float coef, double* parts, float* contrib, int64_t ldc,
                                     void* stream);
/* RFGRCN's prior (models/rfgrcn.py:171-190): prior[r, :W] = src[r, :W] - the column means of r's segment (the U user
 * rows, then the I item rows), W in {64, 128, 192}; src ((U + I) x W, lds) and prior (ldp) may be column blocks of
 * wider tables, nothing outside the block is written.  Centring every 64-wide block on its own, as the reference
 * does, is centring the whole row.  The grid, the block partials and the fixed-order means are gmr_rf_view_prior's at
 * row width W: no float atomics, two runs are bit-identical.  1 <= U, I <= 2^31 - 128.  ws:
 * gmr_rf_center_segments_ws_floats(U, I, W) floats (-1 outside the range).  All pointers 16-byte aligned, strides
 * multiples of 4 floats. */
int64_t gmr_rf_center_segments_ws_floats(int64_t U, int64_t I, int32_t W);
int gmr_rf_center_segments(int64_t U, int64_t I, int32_t W, const float* src, int64_t lds, float* prior, int64_t ldp,
                           float* ws, void* stream);
/* torch.optim.AdamW: p <- p * decay_factor (= 1 - lr wd) first, then gmr_adam_f32's update without its L2 term */
int gmr_adamw_f32(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float beta1,
                  float beta2, float eps, float decay_factor, float step_size, float bias_correction2_sqrt,
                  void* stream);
/* N(0, 1) / U[0, 1) draws from Philox (seed, step, site) */
int gmr_rf_randn(int64_t n, uint64_t seed, uint64_t step, uint64_t site, float* out, void* stream);
int gmr_rf_rand(int64_t n, uint64_t seed, uint64_t step, uint64_t site, float* out, void* stream);

/* ---------------------------------------------------------------- LD4MRec C-Net rows (csrc/ld4m.hip)
 * ConditionalBlock (models/ld4mrec.py:57-87): n = LN(h) w + b, z = n (1 + s) + sh, h' = h + linear2(drop(gelu(
 * linear1(z)))).  H: a multiple of 64 in 64..1024; every matrix has unit column stride, a row stride that is a
 * multiple of 4 and a 16-byte aligned base (float4 loads, one 64-lane wave per row).
 * film_fwd: z from h and the B x H modulation matrices s, sh (own strides); mean / rstd (rows each) saved.
 * film_bwd, from dz: ds = dz n;  dsh = dz (dsh may be NULL or alias dz: no write);  dh (+)= LayerNorm backward of
 * dz (1 + s);  dw / db (+)= through parts (gmr_ld4_film_parts_floats floats), added in block order. */
int gmr_ld4_film_fwd(int64_t rows, int32_t H, const float* h, int64_t ldh, const float* w, const float* b,
                     const float* s, int64_t lds, const float* sh, int64_t ldsh, float eps, float* z, int64_t ldz,
                     float* mean, float* rstd, void* stream);
int64_t gmr_ld4_film_parts_floats(int64_t rows, int32_t H);
int gmr_ld4_film_bwd(int64_t rows, int32_t H, const float* h, int64_t ldh, const float* mean, const float* rstd,
                     const float* w, const float* b, const float* s, int64_t lds, const float* dz, int64_t lddz,
                     float* ds, int64_t ldds, float* dsh, int64_t lddsh, float* dh, int64_t lddh,
                     int32_t accumulate_dh, float* parts, float* dw, float* db, int32_t accumulate_params,
                     void* stream);
/* y = gelu(x) keep / p_keep (exact erf GELU, inverted dropout).  keep[r][c] = mask_in[r][c] when mask_in is given,
 * else drawn with gmr_keep_mask_u8's key (seed, step, ctr0 + r H + c) and recorded in mask_out (may be NULL);
 * p_keep = 1 draws nothing and touches no mask.  Backward: dx = dy keep / p_keep gelu'(x) from the
 * pre-activation x and the recorded mask (NULL at p_keep = 1); dx may alias dy. */
int gmr_ld4_gelu_drop_fwd(int64_t rows, int32_t H, const float* x, int64_t ldx, float p_keep, const uint8_t* mask_in,
                          uint8_t* mask_out, int64_t ldm, uint64_t seed, uint64_t step, uint64_t ctr0, float* y,
                          int64_t ldy, void* stream);
int gmr_ld4_gelu_drop_bwd(int64_t rows, int32_t H, const float* x, int64_t ldx, const uint8_t* mask, int64_t ldm,
                          float p_keep, const float* dy, int64_t lddy, float* dx, int64_t lddx, void* stream);
/* y = x + bias over rows x H (y may be x): the bias of item_proj after gmr_diff_sparse_pre's sum of weight rows */
int gmr_ld4_add_bias(int64_t rows, int32_t H, const float* x, int64_t ldx, const float* bias, float* y, int64_t ldy,
                     void* stream);
/* loss_b = mean_I (pred_b - target_b)^2 (fp64), target = x0 (1 - gamma) + (1 - x0) gamma with x0 the train row of
 * users[b] (user CSR); write_grad: pred <- 2 (pred - target) / I * grad_scale in place (ld4mrec.py:299-335). */
int gmr_ld4_loss_rows(int32_t B, int32_t I, const int32_t* users, const int32_t* user_ptr, const int32_t* user_items,
                      float gamma, float* pred, int64_t ld, float grad_scale, double* loss_out, int32_t write_grad,
                      void* stream);
/* hist[t_b] <- 0.9 hist[t_b] + 0.1 loss_b for b = 0 .. B-1 in that order, in the reference's fp32 arithmetic
 * (ld4mrec.py:340-342); t_b < 0 skips the row.  T <= 1024. */
int gmr_ld4_history_ema(int32_t B, int32_t T, const int32_t* t, const double* loss, float* hist, void* stream);
/* t_b = searchsorted(cumsum(|hist| / sum |hist|), u_b, side = right) clamped to T - 1, the running sum in fp64
 * (np.random.choice(T, B, p), ld4mrec.py:307-312).  u: B uniforms in [0, 1), or NULL: drawn from Philox keyed on
 * (seed, step, row0 + b). */
int gmr_ld4_sample_t(int32_t B, int32_t T, const float* hist, const float* u, uint64_t seed, uint64_t step,
                     int64_t row0, int32_t* t, void* stream);

/* ---------------------------------------------------------------- DDRM (models/ddrm.py; csrc/ddrm.hip)
 * The conditional denoiser out = W2 tanh(W1 [x | emb_layer(temb(t)) | cond] + b1) + b2 on 64-wide rows, hidden width
 * H (a multiple of 4 in 4..1024).  W1: H x 192 (row stride 192), W2: 64 x H (row stride H), both 16-byte aligned.
 * TB (T x H, row stride H) is the folded time table TB[t] = W1[:, 64:128] emb_layer(temb(t)) + b1, built by the caller.
 * A row's result depends on its inputs and its global row number row_off + r only (not on N or its neighbours). */
int32_t gmr_ddrm_tile_rows(void);
/* One training forward of one denoiser over N rows: x0 = X[idx_x[r]] and cond = C[idx_c[r]] (idx NULL: row r),
 * x_t = sqrt_ac[t_r] x0 + sqrt_1mac[t_r] noise_r, xd = dropout_0.5(x_t), h = tanh(.), out, rowmse_r = mean_64 (x0 -
 * out)^2.  noise (N x 64, ldn) or NULL: Philox (seed, step, site; row row_off + r).  drop_mode 0: no dropout; 1: the
 * keep bytes `keep` (N x 64, ldk); 2: drawn from Philox (site + 1) and written to keep_out.  xd, keep_out, h, rowmse
 * may be NULL. */
int gmr_ddrm_denoise_fwd(int64_t N, int32_t H, int32_t T, int64_t row_off, const float* X, int64_t ldx,
                         const int32_t* idx_x, const float* C, int64_t ldc, const int32_t* idx_c, const int32_t* t,
                         const float* sqrt_ac, const float* sqrt_1mac, const float* noise, int64_t ldn,
                         int32_t drop_mode, const uint8_t* keep, int64_t ldk, uint64_t seed, uint64_t step,
                         uint64_t site, const float* W1, const float* TB, const float* W2, const float* b2, float* out,
                         int64_t ldo, float* xd, int64_t ldxd, uint8_t* keep_out, int64_t ldko, float* h, int64_t ldh,
                         float* rowmse, void* stream);
/* The reverse chain of full_sort_predict in one launch, eval mode: x = xs (noise0 != NULL: qa xs + qb noise0), then
 * for i = S-1..0: x <- c1[i] net(x, cond, i) + c2[i] x, + sigma[i] noise_i where i != 0 when sigma != NULL (noise_i =
 * step_noise[i] of an S x N x 64 array, or Philox keyed on (seed, step, site; (row_off + r) T + i)).  S = 0 copies. */
int gmr_ddrm_chain(int64_t N, int32_t H, int32_t T, int32_t S, int64_t row_off, const float* xs, int64_t ldx,
                   const float* noise0, int64_t ldn0, float qa, float qb, const float* C, int64_t ldc,
                   const int32_t* idx_c, const float* W1, const float* TB, const float* W2, const float* b2,
                   const float* c1, const float* c2, const float* sigma, const float* step_noise, uint64_t seed,
                   uint64_t step, uint64_t site, float* out, int64_t ldo, void* stream);
/* calculate_loss's row loss (:405-433) with its backward.  G: the propagated (n_users + I) x 64 table; with u, p, n
 * the rows of users / pos / neg: w = sigmoid(<u,p>)^beta (no gradient), sp = softplus(<u,n> - <u,p>), rec = (mse_u +
 * mse_i) / 2, loss_b = w ((1 - alpha) (sp + reg_weight reg[0]) + alpha rec).  terms (4 x B): [w | sp | rec | loss_b];
 * loss[0] = sum(loss_b) inv_norm (fp64, fixed order), loss[1] = (1 - alpha) reg_weight sum(w) inv_norm, the
 * coefficient of reg, loss[2] = loss[1] inv_norm (3 floats).  contrib (3B x 64, ldc): rows [users | pos | neg] for gmr_scatter_sorted_f32 (scores and the
 * recon targets); dout_u, dout_i (B x 64 dense): d loss / d the denoiser outputs. */
int gmr_ddrm_loss_fwd_bwd(int32_t B, int64_t n_users, const float* G, int64_t ldg, const int32_t* users,
                          const int32_t* pos, const int32_t* neg, const float* out_u, int64_t ldou, const float* out_i,
                          int64_t ldoi, const float* mse_u, const float* mse_i, const float* reg, float alpha,
                          float beta, float reg_weight, float inv_norm, float* terms, float* loss, float* contrib,
                          int64_t ldc, float* dout_u, float* dout_i, void* stream);
/* dst[r] += sqrt_ac[t_r] (keep ? 2 : 0) dxd[r] + dcond[r] over N x 64 rows (dxd, dcond dense; keep NULL: no
 * dropout): the gradient of a gathered row through q_sample and through the other model's cond columns */
int gmr_ddrm_input_bwd(int64_t N, const float* dxd, const uint8_t* keep, int64_t ldk, const int32_t* t,
                       const float* sqrt_ac, const float* dcond, float* dst, int64_t ldd, void* stream);

/* ---------------------------------------------------------------- BM3 (models/bm3.py; csrc/bm3.hip)
 * calculate_loss's six cosine terms (:121-147) with their backward in one launch.  G: the (n_users + I) x 64 table
 * [ua; ib]; T / V: the I x 64 projected text / image tables (either may be NULL: its stream's outputs are 0); every
 * table has its own row stride (16-byte aligned rows).  Streams u = G[users], i = G[n_users + items], t = T[items],
 * v = V[items]; P(x) = x Wp^T + bp (Wp 64 x 64, row stride ldw); targets drop(x) = keep x / (1 - p), no gradient.
 * drop_mode 0: no dropout; 1: the keep bytes of the batch rows (B x 64 per present stream, ldk); 2: drawn by Philox
 * keyed on (seed + (site + stream) 0x9E3779B97F4A7C15, step, table row id * 16 + column / 4), a column kept when
 * (word >> 8) 2^-24 < 1 - p, and written to the keep_out arrays that are not NULL (ldko).
 *   terms   (6 x B)      the cosines [ui | iu | t | v | tv | vt]
 *   contrib (2B x 192)   rows 0..B-1 [dx_u | 0 | 0], rows B..2B-1 [dx_i | dx_t | dx_v], dx = d_on Wp, every element
 *                        written: one gmr_scatter_sorted_f32 through the plan of keys [users | n_users + items]
 *   xg, don (4B x 64)    the gathered inputs and d loss / d P(x), stacked by stream: dWp = don^T xg, dbp = colsum(don)
 * d_on carries inv_norm (the modal streams also cl_weight, their two terms summed). */
int32_t gmr_bm3_tile_rows(void);
int gmr_bm3_loss_fwd_bwd(int32_t B, int64_t n_users, const float* G, int64_t ldg, const float* T, int64_t ldt,
                         const float* V, int64_t ldv, const int32_t* users, const int32_t* items, const float* Wp,
                         int64_t ldw, const float* bp, float p, float cl_weight, float inv_norm, int32_t drop_mode,
                         const uint8_t* keep_u, const uint8_t* keep_i, const uint8_t* keep_t, const uint8_t* keep_v,
                         int64_t ldk, uint64_t seed, uint64_t step, uint64_t site, uint8_t* keep_out_u,
                         uint8_t* keep_out_i, uint8_t* keep_out_t, uint8_t* keep_out_v, int64_t ldko, float* terms,
                         float* contrib, int64_t ldc, float* xg, float* don, void* stream);
/* loss (10 floats) = [total, ui, iu, t, v, tv, vt, reg, cu, ci]: term = 1 - sum(cos) inv_norm (0 for an absent
 * modality), reg = (sqrt(sqnorms[0]) + sqrt(sqnorms[1])) / n_items, total = ui + iu + reg_weight reg + cl_weight (t +
 * v + tv + vt); cu, ci = reg_weight / (n_items sqrt(sqnorms[k])) (0 for a zero norm), the coefficients of
 * gmr_bm3_reg_bwd.  Fixed-order fp64 sums; sqnorms: the squared Frobenius norms of ua and ib on the device. */
int gmr_bm3_loss_reduce(int32_t B, const float* terms, const float* sqnorms, int32_t has_t, int32_t has_v,
                        float reg_weight, float cl_weight, float inv_norm, int64_t n_items, float* loss, void* stream);
/* dG[r] += coef[r < n_users ? 0 : 1] G[r] over n_rows x 64 (coef: two device floats) */
int gmr_bm3_reg_bwd(int64_t n_rows, int64_t n_users, const float* coef, const float* G, int64_t ldg, float* dG,
                    int64_t ldd, void* stream);

/* ---------------------------------------------------------------- MGCN (models/mgcn.py; csrc/mgcn.hip)
 * Row-local fused blocks on the fp32 MFMA: a row's outputs depend on that row's inputs and the weights only, no float
 * atomics.  Every row array is 64 columns wide with 16-byte aligned rows and its own leading dimension (>= 64,
 * % 4 == 0); weights are 64 x 64 [out][in] with row stride ldw, biases and w2 64 floats (w2 16-byte aligned).  The
 * grid is capped at gmr_mgcn_max_blocks() workgroups of gmr_mgcn_tile_rows() rows per trip.
 *
 * Purifier (:152-154) over the n item rows, both modalities in one launch:
 *   gv = sigmoid(V Wgv^T + bgv), gt = sigmoid(T Wgt^T + bgt);  Pv = E * gv, Pt = E * gt
 * gv, gt (n x 64, ldg) are what the backward reads.  Backward: dE (+)= dPv * gv + dPt * gt (accumulate = 1 adds to
 * dE); z (n x 128, ldz >= 128) = [zv | zt], zv = dPv * E * gv (1 - gv), the pre-activation rows (dWgv = zv^T V,
 * dbgv = colsum(zv) on the host side; V and T themselves are not read); dV = zv Wgv, dT = zt Wgt (ld lddv). */
int32_t gmr_mgcn_tile_rows(void);
int32_t gmr_mgcn_max_blocks(void);
int gmr_mgcn_purify_fwd(int64_t n, const float* E, int64_t lde, const float* V, int64_t ldv, const float* T,
                        int64_t ldt, const float* Wgv, const float* bgv, const float* Wgt, const float* bgt,
                        int64_t ldw, float* Pv, float* Pt, int64_t ldp, float* gv, float* gt, int64_t ldg,
                        void* stream);
int gmr_mgcn_purify_bwd(int64_t n, const float* dPv, const float* dPt, int64_t lddp, const float* gv, const float* gt,
                        int64_t ldg, const float* E, int64_t lde, const float* Wgv, const float* Wgt, int64_t ldw,
                        float* dE, int64_t ldde, int32_t accumulate, float* z, int64_t ldz, float* dV, float* dT,
                        int64_t lddv, void* stream);
/* Fuser (:187-201) over the n = U + I rows of a, b (ldab) and c (ldc):
 *   ha = tanh(W1 a + b1), hb = tanh(W1 b + b1);  (wa, wb) = softmax(w2 . ha, w2 . hb);  m = wa a + wb b
 *   gi = sigmoid(Wi c + bi), gt = sigmoid(Wt c + bt);  side = (gi * (a - m) + gt * (b - m) + m) / 3;  all = c + side
 * side, all (ldo) and the saved rows ha, hb, gi, gt (lds) and wab (n x 2: wa, wb) are written; equal logits give
 * wa = wb = 0.5 exactly.  Backward from dall (d loss / d all, ldda) and dside, dcin (the direct gradients of side and
 * c, ldds; either may be NULL = zero): da, db (lddab), dc (lddc), the pre-activation rows z1a, z1b (of W1 a + b1 and
 * W1 b + b1), zi, zt (of the two gates; ldz) and r = dq_a ha + dq_b hb (ldr).  Host side: dW1 = z1a^T a + z1b^T b,
 * db1 = colsum(z1a) + colsum(z1b), dWi = zi^T c, dbi = colsum(zi), the same for Wt, dw2 = colsum(r). */
int gmr_mgcn_fuse_fwd(int64_t n, const float* a, const float* b, int64_t ldab, const float* c, int64_t ldc,
                      const float* W1, const float* b1, const float* w2, const float* Wi, const float* bi,
                      const float* Wt, const float* bt, int64_t ldw, float* side, float* all, int64_t ldo, float* ha,
                      float* hb, float* gi, float* gt, int64_t lds, float* wab, void* stream);
int gmr_mgcn_fuse_bwd(int64_t n, const float* dall, int64_t ldda, const float* dside, const float* dcin, int64_t ldds,
                      const float* a, const float* b, int64_t ldab, const float* ha, const float* hb, const float* gi,
                      const float* gt, int64_t lds, const float* wab, const float* w2, const float* W1,
                      const float* Wi, const float* Wt, int64_t ldw, float* da, float* db, int64_t lddab, float* dc,
                      int64_t lddc, float* z1a, float* z1b, float* zi, float* zt, int64_t ldz, float* r, int64_t ldr,
                      void* stream);
/* bpr_loss (:210-222) on rows gathered from all ((n_users + I) x 64, lda): terms[b] = -logsigmoid(<u,p> - <u,n>)
 * (exact, as gmr_bpr_logsigmoid_f32), terms[B + b] = 0.5 (|u|^2 + |p|^2 + |n|^2); contrib (3B x 64, ldc) =
 * [du; dp; dn] of inv_norm sum(terms[:B]) + reg_weight / reg_div sum(terms[B:]) for gmr_scatter_sorted_f32 through
 * the plan of keys [users | n_users + pos | n_users + neg]. */
int gmr_mgcn_bpr_reg_fwd_bwd(int32_t B, int64_t n_users, const float* all, int64_t lda, const int32_t* users,
                             const int32_t* pos, const int32_t* neg, float inv_norm, float reg_weight, float reg_div,
                             float* terms, float* contrib, int64_t ldc, void* stream);
/* loss (5 floats) = [total, bpr, reg, nce_items, nce_users] from terms (4 x B: the two rows above, then the per-row
 * InfoNCE values of the item and the user term): bpr = inv_norm sum, reg = reg_weight / reg_div sum, nce = inv_norm
 * sum, total = bpr + reg + cl_loss (nce_items + nce_users).  Fixed-order fp64 sums. */
int gmr_mgcn_loss_reduce(int32_t B, const float* terms, float inv_norm, float reg_weight, float reg_div, float cl_loss,
                         float* loss, void* stream);

/* ---------------------------------------------------------------- LATTICE (models/lattice.py): the learned item graph
 * n items, M <= 2 modalities, k <= 64 neighbours; n_m: the row-normalised projected features (n x 64, ldn), idx_m
 * (n x k, ldi): each row's top-k of n_m n_m^T.  Edge (i, m, slot) is position q = m k + slot of row i in the n x (M k)
 * edge arrays (v, dv, oval) and in the first M k of the R = 2 M k columns of item_adj's rows (col: ldc, val: n x R
 * dense).  mw: the two modal_weight floats on the device, w = softmax(mw) (equal entries: exactly 0.5; M = 1: w = 1,
 * mw may be NULL).  A column may occur in several slots of a row; all sums are linear in the slots.
 * edge_fwd:  v = <n_i, n_j> (fixed fma chain + butterfly), col[:, :M k] = idx, r_i = sum_q w_m v, s = r^-1/2
 *            (0 where r = 0).
 * adj_fwd:   val[i, q] = (1 - lambda) s_i w_m v s_col for q < M k, lambda w_m oval[i, q - M k] after (oval: the frozen
 *            original lists' normalised values; their columns are col[:, M k:], written once by the caller).
 * sddmm:     dA[i, q] (+)= <g[i], h[col[i, q]]> over R columns (the graph's gradient on its pattern).
 * The backward takes the incoming lists of the learned edges: in_edge = the edge ids i M k + q sorted stably by the
 * key m n + col, in_ptr (M n + 1) the row pointer over the keys.
 * bwd_ds:    dr_i = -1/2 s_i^3 (sum_q p_(i,q) s_col + sum_{e -> i} p_e s_row(e)), p = (1 - lambda) dA w_m v; 0 where
 *            r_i = 0.
 * bwd_da:    dv = w_m ((1 - lambda) dA s_i s_col + dr_i); parts (n x 2) = the row's share of dw_m = sum da v +
 *            lambda sum oval dA.
 * dw_reduce: dmw (2) = the softmax backward of the column sums of parts (fixed-order fp64 tree).
 * bwd_dn:    dn_m[i] = sum_slot dv n_col + sum_{e -> i} dv_e n_row(e)  (n x 64, ldd).
 * No float atomics; two runs give the same bits. */
int gmr_lat_edge_fwd(int64_t n, int32_t k, int32_t M, const float* n0, int64_t ldn0, const int32_t* idx0, int64_t ldi0,
                     const float* n1, int64_t ldn1, const int32_t* idx1, int64_t ldi1, const float* mw, float* v,
                     int32_t* col, int64_t ldc, float* r, float* s, void* stream);
int gmr_lat_adj_fwd(int64_t n, int32_t k, int32_t M, const float* v, const float* s, const int32_t* col, int64_t ldc,
                    const float* oval, const float* mw, float lambda, float* val, void* stream);
int gmr_lat_sddmm(int64_t n, int32_t R, const int32_t* col, int64_t ldc, const float* g, int64_t ldg, const float* h,
                  int64_t ldh, int32_t accumulate, float* dA, void* stream);
int gmr_lat_bwd_ds(int64_t n, int32_t k, int32_t M, const float* dA, const float* v, const float* r, const float* s,
                   const int32_t* col, int64_t ldc, const int32_t* in_ptr, const int32_t* in_edge, const float* mw,
                   float lambda, float* dr, void* stream);
int gmr_lat_bwd_da(int64_t n, int32_t k, int32_t M, const float* dA, const float* v, const float* s, const float* dr,
                   const int32_t* col, int64_t ldc, const float* oval, const float* mw, float lambda, float* dv,
                   float* parts, void* stream);
int gmr_lat_dw_reduce(int64_t n, const float* parts, const float* mw, float* dmw, void* stream);
int gmr_lat_bwd_dn(int64_t n, int32_t k, int32_t M, const float* dv, const float* n0, int64_t ldn0, const float* n1,
                   int64_t ldn1, const int32_t* col, int64_t ldc, const int32_t* in_ptr, const int32_t* in_edge,
                   float* dn0, int64_t ldd0, float* dn1, int64_t ldd1, void* stream);

/* ---------------------------------------------------------------- SMORE (models/smore.py; csrc/smore.hip)
 * Row-local fused blocks in mgcn.hip's scheme (fp32 MFMA, 16-row tiles, a grid capped at gmr_smore_max_blocks()
 * workgroups, no float atomics).  Rows are 16-byte aligned with ld % 4 == 0; packed arrays hold 64-column blocks side
 * by side.  Weights are 64 x 64 [out][in] with row stride ldw, biases 64 floats.  The kernels take 87 - 143 KB of
 * dynamic LDS: one workgroup per CU.
 *
 * A spectrum row lives in the 64-real layout: column j <= 32 is Re X_j, column j >= 33 is Im X_(j - 32) (Im X_0 and
 * Im X_32 have no column).  The complex filters Wi, Wt, Wf are 33 x 2 floats (re, im); Im W_0 and Im W_32 are never
 * read and their gradients are written as 0.  gmr_smore_twiddles copies the two 64 x 64 transform matrices (forward
 * F[j][n], inverse Gt[n][j] = c_j F[j][n], built once per device in double and rounded) for tests.
 *
 * spectrum_fwd over the n item rows of V, T (the projected features) and E (the item id rows):
 *   A = rfft(V), B = rfft(T) (norm 'ortho');  conv = [irfft(A Wi) | irfft(B Wt) | irfft(A B Wf)]  (n x 192, ldcv)
 *   g = sigmoid(conv_m Wg_m^T + bg_m) (n x 192, ldg);  P = [E * g_v | E * g_t | E * g_f]  (n x 192, ldp)
 *   S = [A | B] (n x 128, ldsp) is what the backward reads.
 * spectrum_bwd from dP (n x 192): dE (+)= sum_m dP_m * g_m (accumulate = 1 adds to dE); z (n x 192) = dP_m * E * g_m
 * (1 - g_m), the gate pre-activation rows (host side: dWg_m = z_m^T conv_m, dbg_m = colsum(z_m)); dV, dT (lddv); and
 * the filter gradients dWi, dWt, dWf (33 x 2 each): per-tile column sums go to ws (gmr_smore_spectrum_ws_floats(n)
 * floats) and a second pass (a workgroup per filter) adds them in a fixed fp64 order that does not depend on the grid. */
int32_t gmr_smore_tile_rows(void);
int32_t gmr_smore_max_blocks(void);
int64_t gmr_smore_spectrum_ws_floats(int64_t n);
int gmr_smore_twiddles(float* fwd, float* inv, void* stream);
int gmr_smore_spectrum_fwd(int64_t n, const float* V, int64_t ldv, const float* T, int64_t ldt, const float* E,
                           int64_t lde, const float* Wi, const float* Wt, const float* Wf, const float* Wgv,
                           const float* bgv, const float* Wgt, const float* bgt, const float* Wgf, const float* bgf,
                           int64_t ldw, float* S, int64_t ldsp, float* conv, int64_t ldcv, float* g, int64_t ldg,
                           float* P, int64_t ldp, void* stream);
int gmr_smore_spectrum_bwd(int64_t n, const float* dP, int64_t lddp, const float* g, int64_t ldg, const float* E,
                           int64_t lde, const float* S, int64_t ldsp, const float* Wi, const float* Wt,
                           const float* Wf, const float* Wgv, const float* Wgt, const float* Wgf, int64_t ldw,
                           float* dE, int64_t ldde, int32_t accumulate, float* z, int64_t ldz, float* dV, float* dT,
                           int64_t lddv, float* ws, int64_t ws_floats, float* dWi, float* dWt, float* dWf,
                           void* stream);
/* Fuser over the n = U + I rows of abf = [a | b | f] (n x 192, ldabf) and c (ldc):
 *   hv = tanh(Wv1 f + bv1), sv = softmax_64(Wv2 hv);  ht, st the same from Wt1, bt1, Wt2
 *   gi, gt, gf = keep * sigmoid(W. c + b.) / (1 - p);  side = (gi sv a + gt st b + gf f) / 3;  all = c + side
 * drop_mode 0: no dropout (also whenever p = 0); 1: keep (n x 192 bytes, ldk, [image | text | fusion], non-zero =
 * kept) is given; 2: drawn from Philox keyed on (seed, the gate's site, step, row, column group), so a row's mask does
 * not depend on the tiling.  saved (n x 448, lds) = [hv | ht | sv | st | gi | gt | gf] with the masked gate rows.
 * Backward from dall, dside, dcin as gmr_mgcn_fuse_bwd (p: the forward's, 0 where it dropped nothing): dabf =
 * [da | db | df] (n x 192), dc, and z (n x 448, ldz) = [z1v | z2v | z1t | z2t | zi | zt | zf], the pre-activation rows
 * of the seven products.  Host side: dWv1 = z1v^T f, dbv1 = colsum(z1v), dWv2 = z2v^T hv, the same for t;
 * dWi = zi^T c, dbi = colsum(zi), the same for Wt, Wf. */
int gmr_smore_fuse_fwd(int64_t n, const float* abf, int64_t ldabf, const float* c, int64_t ldc, const float* Wv1,
                       const float* bv1, const float* Wv2, const float* Wt1, const float* bt1, const float* Wt2,
                       const float* Wi, const float* bi, const float* Wt, const float* bt, const float* Wf,
                       const float* bf, int64_t ldw, float p, int32_t drop_mode, const uint8_t* keep, int64_t ldk,
                       uint64_t seed, uint64_t step, float* side, float* all, int64_t ldo, float* saved, int64_t lds,
                       void* stream);
int gmr_smore_fuse_bwd(int64_t n, const float* dall, int64_t ldda, const float* dside, const float* dcin, int64_t ldds,
                       const float* abf, int64_t ldabf, const float* saved, int64_t lds, float p, const float* Wv1,
                       const float* Wv2, const float* Wt1, const float* Wt2, const float* Wi, const float* Wt,
                       const float* Wf, int64_t ldw, float* dabf, int64_t lddabf, float* dc, int64_t lddc, float* z,
                       int64_t ldz, void* stream);

/* ---------------------------------------------------------------- LGMRec (models/lgmrec.py; csrc/lgmrec.hip)
 * The global hypergraph embedding block, fp32, deterministic (no float atomics; no result depends on the grid).
 * H = hyper_num, 1..64 (anything else is an argument error).  Tables S, h, d h, d L are n x 2H, [v | t]; lat and
 * d lat are [2][H][64].  max_blocks caps a launch's grid (0: gmr_lgm_max_blocks()); every row kernel loops over its
 * rows with that grid, and a row's result does not depend on it.
 * hyper_fwd: the N = U + I rows, users first.  An item row i reads its logits Lv[i], Lt[i] (H columns of the
 *   projection product, ldlv / ldlt); a user row sums its items' logit rows over the interaction CSR in column order.
 *   S = softmax((L + g) / tau), h = keep S / p_keep.  gv, gt (N x H, ldg): given Gumbel draws, else drawn from Philox
 *   keyed on (seed, site, step, row within users / items, column); site = 4 m + 2 (item row) + (dropout).  drop_mode
 *   0: no dropout (also whenever p_keep = 1); 1: keepv, keept (N x H bytes, ldk) given; 2: drawn.
 * draws: the draws of an even site as hyper_fwd makes them, g (n x H) and keep (n x H bytes) of site + 1; either NULL.
 * lat: lat[m] = A[:, m H : m H + H]^T X_m over n rows (Xv, Xt: n x 64, ldx).  32-row tiles write partials to ws
 *   (gmr_lgm_lat_ws_floats(n, H) floats); a second pass adds them in tile order (sixteen fp64 slices, one tree).
 * apply: mode 0: Y (n x 128) = [A_v M_v | A_t M_t]; mode 1: Y (n x 64) += A_v M_v + A_t M_t.
 * combine_fwd: x_m = h_m lat_m; all = cge + n(mge_v) + n(mge_t) + alpha n(x_v + x_t) with n(x) = x / max(|x|, 1e-12);
 *   CLN (n x 128, packed) = [n(x_v) | n(x_t)], nrmCL [2][n] their clamped norms (the layout of
 *   gmr_contrast_fused_nbwd_f32 and gmr_scatter_sorted_nbwd_f32), nrm3 [3][n] = |mge_v|, |mge_t|, |x_v + x_t| clamped.
 * combine_bwd: from dall: dmge (n x 128) and dK (n x 128, packed) += [d | d], d = alpha nbwd(x_v + x_t)(dall).
 * dh: out[r, m H + k] = <X_m[r], M[m][k]> (+ acc[r, m H + k]); with S and h given the result is taken through the
 *   dropout and softmax backward: out = S (d S - <d S, S>) / tau, d S = d h / p_keep where h != 0, else 0 (finite
 *   where a probability underflowed to 0).
 * logit_bwd: outm[i, k] = dL[U + i, m H + k] + sum over the users u of item i (trp, tcol: the I x U transposed CSR,
 *   users ascending) of dL[u, m H + k].
 * reg: out[0] = coef (|all[users]|_F + |all[U + pos]|_F + |all[U + neg]|_F); contrib (3B x 64) += its rows. */
int32_t gmr_lgm_tile_rows(void);
int32_t gmr_lgm_max_blocks(void);
int64_t gmr_lgm_lat_ws_floats(int64_t n, int32_t H);
int gmr_lgm_hyper_fwd(int64_t U, int64_t I, int32_t H, const float* Lv, int64_t ldlv, const float* Lt, int64_t ldlt,
                      const int32_t* rowptr, const int32_t* col, const float* gv, const float* gt, int64_t ldg,
                      const uint8_t* keepv, const uint8_t* keept, int64_t ldk, float tau, float p_keep,
                      int32_t drop_mode, uint64_t seed, uint64_t step, float* S, float* h, int64_t ldh,
                      int32_t max_blocks, void* stream);
int gmr_lgm_draws(int64_t n, int32_t H, int32_t site, uint64_t seed, uint64_t step, float p_keep, float* g,
                  uint8_t* keep, void* stream);
int gmr_lgm_lat(int64_t n, const float* A, int64_t lda, int32_t H, const float* Xv, const float* Xt, int64_t ldx,
                float* ws, int64_t ws_floats, int32_t max_blocks, float* lat, void* stream);
int gmr_lgm_apply(int64_t n, const float* A, int64_t lda, int32_t H, const float* M, float* Y, int64_t ldy,
                  int32_t mode, int32_t max_blocks, void* stream);
int gmr_lgm_combine_fwd(int64_t n, const float* cge, int64_t ldc, const float* mge, int64_t ldm, const float* h,
                        int64_t ldh, int32_t H, const float* lat, float alpha, float* all, int64_t ldo, float* CLN,
                        float* nrmCL, float* nrm3, int32_t max_blocks, void* stream);
int gmr_lgm_combine_bwd(int64_t n, const float* dall, int64_t ldda, const float* mge, int64_t ldm, const float* CLN,
                        const float* nrmCL, const float* nrm3, float alpha, float* dmge, int64_t lddm, float* dK,
                        int32_t max_blocks, void* stream);
int gmr_lgm_dh(int64_t n, const float* Xv, const float* Xt, int64_t ldx, const float* M, int32_t H, const float* acc,
               int64_t ldacc, const float* S, const float* h, int64_t ldh, float p_keep, float tau, float* out,
               int64_t ldo, int32_t max_blocks, void* stream);
int gmr_lgm_logit_bwd(int64_t U, int64_t I, int32_t H, const float* dL, int64_t lddl, const int32_t* trp,
                      const int32_t* tcol, float* outv, int64_t ldov, float* outt, int64_t ldot, int32_t max_blocks,
                      void* stream);
int gmr_lgm_reg(int32_t B, int64_t U, const float* all, int64_t lda, const int32_t* users, const int32_t* pos,
                const int32_t* neg, float coef, float* contrib, int64_t ldc, float* out, void* stream);

/* ---------------------------------------------------------------- GRCN (models/grcn.py; csrc/grcn.hip)
 * The train graph: the users' CSR (rowptr U + 1, col: items, E entries) and the items' CSC (trp I + 1, tcol: users) with
 * the position maps csr2csc[e] / csc2csr[t] between the two list orders.  M (1 or 2) modalities sit side by side in
 * 64-column blocks of every table: F (I x 64 M) the normalised item rows, P (U x 64 M) the preference rows.  Per-edge
 * arrays of the 2E directed edges are [user-destination in CSR order | item-destination in CSC order], one per modality
 * (stride 2E).  All rows 16-byte aligned, ld % 4 == 0.  Every kernel takes max_blocks (0: the default cap,
 * gmr_grcn_max_blocks()) and gives the same bits under any grid; no float atomics.
 * route_fwd: P holds R + 1 tables (stride pstride floats); table 0 = n(preference) is read, tables 1..R written,
 *   p^(r+1)_u = n(p^r_u + sum_j softmax_j(<p^r_u, f_j>) f_j) over the user's items; nrmY (R x M x U) the clamped norms.
 *   messages = 0: the users receive no message (the reference's routing edges point from the users to the items,
 *   grcn.py:149-156), a round is p <- n(p); the same flag in route_bwd_dst, which then leaves RA / RD alone.
 * attn_fwd: rep (N x 64 M) = x + h for user rows (over the CSR, sources F) and item rows (over the CSC, sources P),
 *   alpha (M x 2E) the softmax values.
 * refine_fwd: W[q] = relu(max_m alpha_m[q] conf[source(q), m]) (conf N x M, ld ldc), WT the same values at the
 *   transposed edge's position, arg[q] = the winning modality + 2 where the ReLU pruned the edge.
 * dw: dw[q] = <x[source], dx1[dest]> + <x1[source], g[dest]> over N x 64 tables (the sampled product of the two
 *   weighted hops' backward).
 * refine_bwd: dalpha (M x 2E) and dconf (N x M, every row written) from dw through the ReLU and the recorded argmax; a
 *   node sums over its own edge list.
 * attn_bwd_dst: t_k = dalpha_k + <drep_d, x_k>, ds_k = alpha_k (t_k - sum alpha t) into ds (M x 2E), dxd (N x 64 M) =
 *   drep + sum_k ds_k x_k.
 * route_bwd_dst: from dpR = d loss / d p^R, the R rounds in reverse with alpha recomputed from p^r: RA, RD (R x M x E,
 *   CSR order) = alpha^r, ds^r; DY (R x U x 64 M packed) = d loss / d (p^r + h^r); dpref_m (U x 64) = the normalise
 *   backward of d p^0 (nrm0: M x U clamped norms of the preference rows) + dense_m preference_m + regtab (U x 64 M,
 *   may be NULL).
 * bwd_src: out[s] (n x 64 M) += sum over T <= 8 terms and the entries k of row s of (ptr, idx, pos) of
 *   A_t[m][pos_k] DH_t[idx_k] + DS_t[m][pos_k] XD_t[idx_k]  (per-modality array stride estride_t).
 * loss_rows: terms[b] = -log sigmoid(<r_u, r_p - r_n>), terms[B + b] = the batch rows' share of the regulariser means;
 *   contrib (3B x (128 + 128 M), rows [users | pos | neg]) = [d result (inv_norm) | reg_weight d id rows | reg_weight d
 *   preference rows] for gmr_scatter_sorted_f32 through the plan of keys [users | U + pos | U + neg]. */
int32_t gmr_grcn_max_blocks(void);
int32_t gmr_grcn_max_layers(void);
int gmr_grcn_route_fwd(int64_t U, int32_t R, int32_t M, int32_t messages, const int32_t* rowptr, const int32_t* col,
                       const float* F, int64_t ldf, float* P, int64_t ldp, int64_t pstride, float* nrmY, int32_t max_blocks,
                       void* stream);
int gmr_grcn_attn_fwd(int64_t U, int64_t I, int64_t E, int32_t M, const int32_t* rowptr, const int32_t* col,
                      const int32_t* trp, const int32_t* tcol, const float* P, int64_t ldp, const float* F, int64_t ldf,
                      float* rep, int64_t ldr, float* alpha, int32_t max_blocks, void* stream);
int gmr_grcn_refine_fwd(int64_t U, int64_t I, int64_t E, int32_t M, const int32_t* rowptr, const int32_t* col,
                        const int32_t* trp, const int32_t* tcol, const int32_t* csr2csc, const int32_t* csc2csr,
                        const float* alpha, const float* conf, int64_t ldc, float* W, float* WT, int32_t* arg,
                        int32_t max_blocks, void* stream);
int gmr_grcn_dw(int64_t U, int64_t I, int64_t E, const int32_t* rowptr, const int32_t* col, const int32_t* trp,
                const int32_t* tcol, const float* x, int64_t ldx, const float* x1, int64_t ldx1, const float* dx1,
                int64_t lddx1, const float* g, int64_t ldg, float* dw, int32_t max_blocks, void* stream);
int gmr_grcn_refine_bwd(int64_t U, int64_t I, int64_t E, int32_t M, const int32_t* rowptr, const int32_t* col,
                        const int32_t* trp, const int32_t* tcol, const int32_t* csr2csc, const int32_t* csc2csr,
                        const float* alpha, const float* conf, int64_t ldc, const int32_t* arg, const float* dw,
                        float* dalpha, float* dconf, int64_t lddc, int32_t max_blocks, void* stream);
int gmr_grcn_attn_bwd_dst(int64_t U, int64_t I, int64_t E, int32_t M, const int32_t* rowptr, const int32_t* col,
                          const int32_t* trp, const int32_t* tcol, const float* P, int64_t ldp, const float* F,
                          int64_t ldf, const float* alpha, const float* dalpha, const float* drep, int64_t lddr,
                          float* ds, float* dxd, int64_t lddx, int32_t max_blocks, void* stream);
int gmr_grcn_route_bwd_dst(int64_t U, int64_t E, int32_t R, int32_t M, int32_t messages, const int32_t* rowptr,
                           const int32_t* col,
                           const float* F, int64_t ldf, const float* P, int64_t ldp, int64_t pstride,
                           const float* nrmY, const float* dpR, int64_t lddp, float* RA, float* RD, float* DY,
                           const float* pref0, const float* pref1, int64_t ldpref, const float* nrm0,
                           const float* regtab, int64_t ldreg, float dense0, float dense1, float* dpref0, float* dpref1,
                           int64_t lddpref, int32_t max_blocks, void* stream);
int gmr_grcn_bwd_src(int64_t n, int32_t M, int32_t T, const int32_t* ptr, const int32_t* idx, const int32_t* pos,
                     const float* const* A, const float* const* DS, const int64_t* estride, const float* const* DH,
                     const int64_t* lddh, const float* const* XD, const int64_t* ldxd, float* out, int64_t ldo,
                     int32_t max_blocks, void* stream);
int gmr_grcn_loss_rows(int32_t B, int64_t U, int32_t M, const float* res, int64_t ldr, const float* E, int64_t lde,
                       const float* pref0, const float* pref1, int64_t ldpref, const int32_t* users, const int32_t* pos,
                       const int32_t* neg, float inv_norm, float reg_weight, float* terms, float* contrib, int64_t ldc,
                       int32_t max_blocks, void* stream);

/* (Round 5's native executor of a captured HIP graph, gmr_graph_exec_*, was removed in round 6: its replayed
 * step ran slower on the GPU than eager issue; the host tape of gmr/tape.py removes the Python issue cost and
 * keeps the eager streams and order.) */

#ifdef __cplusplus
}
#endif
#endif /* GMR_H_ */
