/*
 * include/mms.h -- C ABI of libmms_hip.so: the MI355X (gfx950) implementation
 * of the MMS metric-learning inner loop of lxmeng/mms_answer_selection.
 *
 * This is the drop-in boundary.  Each entry point replaces the body of one
 * Caffe virtual of the reference (the file:line it replaces is cited per
 * function; paths relative to the reference checkout).  A Caffe build binds
 * them from Forward_gpu/Backward_gpu with blob->gpu_data()/mutable_gpu_diff()
 * pointers (INTEGRATION.md shows the stub); tests bind them with ctypes.
 *
 * Conventions
 *  - Plain pointers and sizes only.  Every data pointer is DEVICE memory
 *    (hipMalloc / torch.cuda tensor), row-major contiguous, laid out exactly
 *    like the reference's blobs.  No allocation, no host synchronisation, no
 *    stream other than `stream` (a hipStream_t passed as void*; NULL = the
 *    null stream, which is what Caffe uses).  Safe to capture in a hipGraph.
 *  - Return value: MMS_OK or an MMS_ERR_* code; nothing is launched on error.
 *    (The C++ Layer mirror turns a non-zero code into the reference's
 *    CHECK/LOG(FATAL) abort.)
 *  - Deterministic: the same inputs give the same bits every run.  No floating-point atomics anywhere; the only
 *    atomics in the library are the INTEGER arrival words of the fused steps' in-launch loss sum (order-free:
 *    integer addition commutes), which live in the caller's workspace (mms_triplet_workspace_init).
 *  - Numerics: results whose summation order the reference's
 *    own source fixes (Euclidean SimCross forward/backward, PairRankLoss
 *    per-element terms and gradients) are BIT-IDENTICAL to the reference CPU
 *    code.  Results that pass through CBLAS in the reference (cosine,
 *    bilinear, SimMatrix) or a long scalar sum (the loss value) agree to
 *    1e-5 relative.
 *  - dist_mode: 0 cosine, 1 Euclidean 1/(1+||q-a||), 2 bilinear q W a^T
 *    (src/caffe/proto/caffe.proto:471-477; default 1).
 */
#ifndef MMS_H_
#define MMS_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 0.2.0: mms_embed_simcross_forward_f32 gained `embed_bias`, mms_rank_workspace_bytes and the mms_layer_t option
 * table changed (round 2), the triplet workspace carries the arrival words and must be initialised (round 3).
 * A host built against another header must refuse to run: compare mms_version() with MMS_VERSION at start-up. */
#define MMS_VERSION 212

enum {
  MMS_OK = 0,
  MMS_ERR_INVALID_ARG = 1,   /* null pointer, negative size, unknown mode     */
  MMS_ERR_UNSUPPORTED = 2,   /* valid request this build cannot run           */
  MMS_ERR_WORKSPACE = 3,     /* workspace missing or too small                */
  MMS_ERR_LAUNCH = 4         /* hipGetLastError() != hipSuccess after launch  */
};

int mms_version(void);
const char* mms_error_string(int code);

/* ------------------------------------------------------------------------- *
 * Arithmetic of the Euclidean backward term  tt = dT*T*T*T*(q-a)/(T-1+1e-9)
 * (sim_cross_layer.cpp:214-216: float products divided by a DOUBLE, rounded once
 * to float).  The forward value T is bit-identical to the CPU code in both modes.
 *   MMS_EUCLID_BWD_FP32 (default): fp32 throughout, tt = (c*(q-a)) * fl32(1/den);
 *       at most 2 ulp from the reference's value (<= 1.2e-7 relative; the bar is
 *       1e-5).  Used by the kernels specialised for D = 100 / 200 / 300 in the
 *       one-word geometry (SimCross and the fused triplet step) and by the tiled
 *       word-grid backward; every other kernel always runs the reference mode.
 *       For batches of >= 512 narrow word grids (D <= 64) the word-grid backward also
 *       sums da over the rows j in two halves (two waves per pair) and adds the halves:
 *       one association away from the reference's j-ascending sum, within the same bar.
 *   MMS_EUCLID_BWD_REFERENCE: the reference's bits, everywhere.
 * The mode belongs to the CALLING THREAD (a Caffe host drives each GPU from its own thread, and so does its
 * `Caffe` singleton, src/caffe/common.cpp:13-15): mms_set_euclid_backward_mode changes it for the calling
 * thread only and is read when a call is issued.  A thread that never set it uses the process default, the
 * environment variable MMS_EUCLID_BWD=reference|fp32 (fp32 when unset).  The Layer mirror can pin a mode per
 * layer (include/mms_layer.h: mms_layer_set_euclid_backward_mode).
 * ------------------------------------------------------------------------- */
#define MMS_EUCLID_BWD_FP32 0
#define MMS_EUCLID_BWD_REFERENCE 1
int mms_set_euclid_backward_mode(int mode);
int mms_get_euclid_backward_mode(void);

/* Which comparison gates the hinge term in the PairRankLoss BACKWARD (the standalone entry point and the
 * fused triplet step).  The reference's two implementations disagree where margin - y*(a-b) is exactly 0:
 *   MMS_PAIRRANK_HINGE_CPU (default): `ordered > 0`,  PairRankLossLayer::Backward_cpu
 *                                     (src/caffe/layers/pair_rank_loss_layer.cpp:76) -- the parity target;
 *   MMS_PAIRRANK_HINGE_GPU:           `ordered >= 0`, the PairRankLossBackward kernel that Backward_gpu
 *                                     launches (src/caffe/layers/pair_rank_loss_layer.cu:51).
 * Set per calling thread, like the Euclidean mode above. */
/* Measurement aid (no reference counterpart): launches an EMPTY kernel of `workgroups` x 512 threads on
 * `stream`.  bench.py replays it under the same hipGraph protocol as the Layer-API sequence to report what a
 * launch costs by itself on this box (about 2.0 us per graph kernel node on MI355X), i.e. how much of a
 * two-launch step no kernel can remove. */
int mms_null_launch(int workgroups, void* stream);

/* out[0] = sum_i x[i]*y[i], all three on the device (one workgroup, fixed summation tree).  The Layer mirror's
 * Forward uses it for loss tops in GPU mode where the reference calls caffe_gpu_dot
 * (include/caffe/layer.hpp:469-481, src/caffe/util/math_functions.cu caffe_gpu_dot). */
int mms_dot_f32(int n, const float* x, const float* y, float* out, void* stream);

/* SplitLayer::Backward (src/caffe/layers/split_layer.cpp:38-57, split_layer.cu:19-34): the gradient of a blob that
 * feeds `ntop` consumers is the sum of their gradients, formed in consumer order: bottom = top_0 (ntop == 1: a copy),
 * (top_0 + top_1), then + top_2, ... -- the reference's caffe_gpu_add followed by caffe_gpu_axpy(1, ...), same
 * association, hence the same bits.  `top_diffs`: a HOST array of ntop DEVICE pointers; bottom_diff may be top_diffs[0]. */
int mms_split_backward_f32(int count, int ntop, const float* const* top_diffs, float* bottom_diff, void* stream);
int mms_dot_f64(int n, const double* x, const double* y, double* out, void* stream);

#define MMS_PAIRRANK_HINGE_CPU 0
#define MMS_PAIRRANK_HINGE_GPU 1
int mms_set_pairrank_hinge_mode(int mode);
int mms_get_pairrank_hinge_mode(void);

/* How PairRankLoss's loss scalar is summed (mms_pairrank_forward_f32 and the fused triplet step; per calling
 * thread, like the modes above).
 *   MMS_LOSS_SUM_FAST (default): an order-free sum of the bit-exact per-element terms (fixed-shape tree, or integer
 *       arithmetic inside the fused step): within 2e-6 of the exact mean, hence within 1e-5 of the reference's value
 *       wherever that value is itself within 1e-5 of the exact mean.
 *   MMS_LOSS_SUM_REFERENCE: Forward_cpu's own sum, ONE running fp32 accumulator over the terms in index order
 *       (pair_rank_loss_layer.cpp:41-49): the CPU code's bits, including its drift for thousands of near-constant
 *       terms (every add of ~2 to a partial sum in [4096, 8192) rounds the same way: 1-2e-5 relative at N = 4096).
 *       A dependent chain of `count` adds by one lane, ~3 ns each, in one extra one-workgroup launch; the fused
 *       step then sums by a second launch whatever its finish mode. */
#define MMS_LOSS_SUM_FAST 0
#define MMS_LOSS_SUM_REFERENCE 1
int mms_set_loss_sum_mode(int mode);
int mms_get_loss_sum_mode(void);

/* ------------------------------------------------------------------------- *
 * SimCross  (q (N,W1,D), a (N,W2,D) -> top (N, M|1, W1, W2))
 * ------------------------------------------------------------------------- */

/* Replaces SimCrossLayer<float>::Forward_cpu / Forward_gpu
 *   src/caffe/layers/sim_cross_layer.cpp:83-163, sim_cross_layer.cu:128-194.
 * W (M,D,D) and bias (M,W1,W2) are read for dist_mode 2 only (bias may be NULL
 * = bias_term false).  norm0 (N,W1) / norm1 (N,W2) are the layer's
 * data{0,1}_norm_ blobs: written for dist_mode 0 (they hold the NORM, like the
 * CPU code, :118,:126 -- not the squared norm the reference .cu caches),
 * ignored otherwise.  M is mesure_count (dist_mode 2) and must be 1 otherwise.
 * workspace: mms_simcross_workspace_bytes(...) bytes of device scratch. */
int mms_simcross_forward_f32(int dist_mode, int N, int W1, int W2, int D, int M,
                             const float* q, const float* a, const float* W,
                             const float* bias, float* top, float* norm0,
                             float* norm1, void* workspace,
                             size_t workspace_bytes, void* stream);

/* Replaces SimCrossLayer<float>::Backward_cpu / Backward_gpu
 *   src/caffe/layers/sim_cross_layer.cpp:166-307, sim_cross_layer.cu:197-243.
 * Reference-visible behaviour kept: dq and da are ALWAYS overwritten (zeroed
 * first, :176-177); if neither propagate_down flag is set they stay zero, if
 * either is set BOTH are computed (:201).  dist_mode 2: dW (M,D,D) is
 * overwritten (the reference zeroes W.diff itself, :256); dbias (M,W1,W2) is
 * ACCUMULATED into (:301-304) when bias_term != 0. */
int mms_simcross_backward_f32(int dist_mode, int N, int W1, int W2, int D, int M,
                              const float* q, const float* a, const float* W,
                              int bias_term, const float* top,
                              const float* top_diff, const float* norm0,
                              const float* norm1, int propagate_down0,
                              int propagate_down1, float* dq, float* da,
                              float* dW, float* dbias, void* workspace,
                              size_t workspace_bytes, void* stream);

/* The two calls above with their arguments in ONE block (same meaning, same checks, same results): for hosts
 * whose foreign-function calls cost per argument -- ctypes, JNI, cgo -- so that launching kernel by kernel keeps
 * ahead of the device without a hipGraph (a 21-argument ctypes call costs ~4 us of host time, one with a block
 * pointer ~1.3 us; a kernel of this path runs 3-5 us).  The block may be reused and edited between calls. */
typedef struct mms_simcross_args_f32 {
  int dist_mode, N, W1, W2, D, M;
  const float* q; const float* a; const float* W; const float* bias;   /* bias: forward only */
  float* top;                                                          /* forward: written; backward: read */
  float* norm0; float* norm1;
  /* backward only */
  int bias_term, propagate_down0, propagate_down1;
  const float* top_diff; float* dq; float* da; float* dW; float* dbias;
  void* workspace; size_t workspace_bytes;
} mms_simcross_args_f32;
int mms_simcross_forward_block_f32(const mms_simcross_args_f32* args, void* stream);
int mms_simcross_backward_block_f32(const mms_simcross_args_f32* args, void* stream);

/* Forward and Backward in ONE launch, for hosts that hold top_diff BEFORE the forward runs
 * (dist_mode 0/1: q and a are read once, top/dq/da written once; dist_mode 2 runs the two passes
 * back to back on `stream`).  Results are identical to the two calls above.  NOT reachable from
 * the reference's callers: a Caffe Net and `caffe time` alike run every layer's Forward, then every
 * layer's Backward (net.cpp:535-546, 581-591; tools/caffe.cpp:349-361), so a Layer binds the two
 * calls above -- that pair of launches is what bench.py reports; this entry point is a labelled
 * variant there. */
int mms_simcross_forward_backward_f32(int dist_mode, int N, int W1, int W2,
                                      int D, int M, const float* q,
                                      const float* a, const float* W,
                                      const float* bias, const float* top_diff,
                                      float* top, float* norm0, float* norm1,
                                      float* dq, float* da, float* dW,
                                      float* dbias, void* workspace,
                                      size_t workspace_bytes, void* stream);

/* fp16-STORAGE variants of the Euclidean sentence-vector path (W1 = W2 = 1,
 * dist_mode 1; BASELINE cfg 5): q, a, dq, da are IEEE half in HBM, the scores
 * and top_diff stay fp32, and all arithmetic is the fp32 reference arithmetic on
 * the exactly-widened inputs -- top equals the fp32 result on those inputs bit
 * for bit and dq/da are its correctly rounded (RNE) halves.  D % 8 == 0,
 * D <= 2048.  The reference has no fp16 instantiation (common.hpp:41-44). */
/* How the fp16-storage entry points sum the D squares of a pair (per calling thread):
 *   MMS_F16_DISTANCE_ORDERED (default): d-ascending fp32 sum, the order of sim_cross_layer.cpp:100-105 -- scores
 *       bit-identical to the fp32 layer run on the fp16-rounded inputs (and so is any ranking);
 *   MMS_F16_DISTANCE_TREE: a fixed tree sum (deterministic, ~1e-6 relative from the ordered sum; SURVEY 8(d) holds
 *       this configuration to 1e-3 against the fp32 oracle because the reference has no fp16 instantiation to
 *       reproduce).  2.3x faster at D = 1024: the ordered chain is 55 % of the ordered kernel. */
#define MMS_F16_DISTANCE_ORDERED 0
#define MMS_F16_DISTANCE_TREE 1
int mms_set_f16_distance_mode(int mode);
int mms_get_f16_distance_mode(void);
int mms_simcross_euclid_forward_f16(int N, int D, const void* q_f16, const void* a_f16,
                                    float* top, void* stream);
int mms_simcross_euclid_forward_backward_f16(int N, int D, const void* q_f16,
                                             const void* a_f16, const float* top_diff,
                                             float* top, void* dq_f16, void* da_f16,
                                             void* stream);
/* fp16-STORAGE cosine (dist_mode 0), W1 = W2 = 1 (round 3): q, a, dq, da IEEE half in HBM, scores / norms / top_diff fp32,
 * fp32 arithmetic on the exactly-widened inputs in the reference's form (sim_cross_layer.cpp:112-139, 226-250: norms
 * cached, T = q.a / nq / na).  Inputs whose dot products are exact in fp32 give the bits of mms_simcross_forward_f32 on the
 * widened inputs for top and the norms; otherwise those are within a few 2^-24 of fp64 (tree sums).  dq / da are the RNE
 * halves of a value within 5 x 2^-24 of (|t1| + |t2|) per (j, k) term pair of the fp64 gradient from the stored top and norms.
 * norm0 / norm1 may be NULL.  D % 8 == 0, D <= 2048, 16-byte aligned operands, else MMS_ERR_UNSUPPORTED. */
int mms_simcross_cosine_forward_f16(int N, int D, const void* q_f16, const void* a_f16, float* top, float* norm0,
                                    float* norm1, void* stream);
int mms_simcross_cosine_forward_backward_f16(int N, int D, const void* q_f16, const void* a_f16, const float* top_diff,
                                             float* top, float* norm0, float* norm1, void* dq_f16, void* da_f16,
                                             void* stream);

/* fp16-STORAGE SimCross on W1 x W2 WORD GRIDS, dist_mode 0 (cosine) and 1 (Euclid): q (N,W1,D), a (N,W2,D), dq, da IEEE
 * half in HBM; top, top_diff (N,1,W1,W2) and norm0 (N,W1), norm1 (N,W2) fp32.  No workspace.
 *   Arithmetic: every half is widened exactly and everything is the fp32 arithmetic of mms_simcross_forward_f32 /
 *       mms_simcross_backward_f32 on the widened inputs, all sums fp32 in the reference's order: the forward sums d
 *       ascending per output, dq[j,d] sums over k ascending from 0, da[k,d] over j ascending from 0
 *       (sim_cross_layer.cpp:96-139, 208-250).  Euclid: top carries the bits of the fp32 call.  Cosine: top and the norms
 *       carry its bits too (same kernels' order).  mms_set_f16_distance_mode is NOT consulted: the tree sum belongs to
 *       the rows family (W1 = W2 = 1) above only; here every dist_mode sums in order whatever that mode says.
 *   Gradients: accumulated in fp32, each element rounded ONCE (RNE) to half when stored; overflow gives +-Inf as RNE does.
 *   Norms: dist_mode 0: required, written by the forward, read by the backward (as mms_simcross_forward_f32);
 *       dist_mode 1: ignored, may be NULL.
 *   Euclid backward: mms_set_euclid_backward_mode is honoured as in mms_simcross_backward_f32 (reference: the fp32
 *       gradient is the reference's bit for bit before its one rounding to half), read once per call.
 *   Any D >= 1 and any 2-byte aligned operands: alignment only selects between kernels, never refuses.
 *   MMS_ERR_UNSUPPORTED: dist_mode 2 (use mms_simcross_bilinear_*_f16 below); W1 == 1 && W2 == 1 (use the rows family:
 *       mms_simcross_euclid_*_f16 / mms_simcross_cosine_*_f16).  MMS_ERR_INVALID_ARG: bad sizes, a NULL required pointer,
 *       as in the fp32 calls.  N == 0: MMS_OK.  A call that does not return MMS_OK, and N == 0, write nothing.
 *   mms_simcross_forward_backward_f16: the forward, then the backward, on `stream`; the same bits as the two calls. */
int mms_simcross_forward_f16(int dist_mode, int N, int W1, int W2, int D, const void* q_f16, const void* a_f16,
                             float* top, float* norm0, float* norm1, void* stream);
int mms_simcross_backward_f16(int dist_mode, int N, int W1, int W2, int D, const void* q_f16, const void* a_f16,
                              const float* top, const float* top_diff, const float* norm0, const float* norm1,
                              void* dq_f16, void* da_f16, void* stream);
int mms_simcross_forward_backward_f16(int dist_mode, int N, int W1, int W2, int D, const void* q_f16,
                                      const void* a_f16, const float* top_diff, float* top, float* norm0,
                                      float* norm1, void* dq_f16, void* da_f16, void* stream);

/* fp16-STORAGE SimCross dist_mode 2 (bilinear, T[n,m] = Q_n W_m A_n^T + bias_m) on W1 x W2 WORD GRIDS, the mode network_v4
 * scores and trains with (sim_cross_layer.cpp:140-161, 251-305): q (N,W1,D), a (N,W2,D), dq, da IEEE half in HBM; W (M,D,D),
 * bias and dbias (M,W1,W2), top and top_diff (N,M,W1,W2) and dW (M,D,D) fp32.  bias NULL = no bias term.
 *   Arithmetic: every half is widened exactly and everything after that is the fp32 arithmetic of mms_simcross_forward_f32 /
 *       mms_simcross_backward_f32 at dist_mode 2 on the widened inputs (the same kernels, instantiated for half storage, where
 *       the word grids fit them; otherwise those calls themselves on a widened copy in the workspace).  The sums the
 *       reference takes in place keep their ascending order: dq, da over m; dW over pairs; dbias over n.  dW is OVERWRITTEN;
 *       dbias is ACCUMULATED into when bias_term != 0 (the fused call: when bias != NULL) and untouched otherwise.
 *   Bits: top, dW and dbias carry the bits of the fp32 calls run on 16-byte-aligned fp32 copies of the widened operands; dq
 *       and da are those calls' dq and da, each element rounded ONCE (RNE) to half when stored; overflow gives +-Inf as RNE
 *       does.  There are no propagate-down flags: both gradients are always computed.  mms_set_matrix_mode is NOT consulted
 *       (dist_mode 2 on word grids is fp32 MFMA in the fp32 call too).
 *   workspace: mms_simcross_bilinear_workspace_bytes_f16 bytes (never 0 for a valid shape; it covers the forward and the
 *       backward of the shape), no initialisation needed, nothing past that size is written.  A missing or short workspace:
 *       MMS_ERR_WORKSPACE.
 *   Any D >= 1 and any 2-byte aligned operands: alignment (and D) only select how wide the staging loads are, never refuse.
 *   MMS_ERR_UNSUPPORTED: W1 == 1 && W2 == 1 (the rows family of the learned metric: mms_simmatrix_forward_f16,
 *       mms_simmatrix_forward_train_f16, mms_simmatrix_backward_f16).  MMS_ERR_INVALID_ARG: bad sizes (as
 *       mms_simcross_forward_f32 at dist_mode 2: N < 0, W1, W2, D or M <= 0, more than 2^31 - 1 elements in q, a or top), a
 *       NULL required pointer -- q, a, W, top; in the backward also top_diff, dq, da, dW, and dbias with a bias term.
 *       N == 0: MMS_OK.  A call that does not return MMS_OK, and N == 0, write nothing.
 *   mms_simcross_bilinear_forward_backward_f16: the forward, then the backward, on `stream`; the same bits as the two calls. */
size_t mms_simcross_bilinear_workspace_bytes_f16(int N, int W1, int W2, int D, int M);
int mms_simcross_bilinear_forward_f16(int N, int W1, int W2, int D, int M, const void* q_f16, const void* a_f16,
                                      const float* W, const float* bias, float* top, void* workspace,
                                      size_t workspace_bytes, void* stream);
int mms_simcross_bilinear_backward_f16(int N, int W1, int W2, int D, int M, const void* q_f16, const void* a_f16,
                                       const float* W, int bias_term, const float* top_diff, void* dq_f16, void* da_f16,
                                       float* dW, float* dbias, void* workspace, size_t workspace_bytes, void* stream);
int mms_simcross_bilinear_forward_backward_f16(int N, int W1, int W2, int D, int M, const void* q_f16, const void* a_f16,
                                               const float* W, const float* bias, const float* top_diff, float* top,
                                               void* dq_f16, void* da_f16, float* dW, float* dbias, void* workspace,
                                               size_t workspace_bytes, void* stream);
/* The scoring forward of the same family straight from word ids and a HALF embedding table (K,D): the twin of
 * mms_embed_simcross_bilinear_forward_f32 (below), the gather done by the staging loads, no workspace.  Row value =
 * embed_bias[d] + widen(table[id][d]) in fp32 (embed_bias: D floats or NULL), ids clamped to [0, K - 1] as there; top
 * carries the bits of that call on the widened table -- and, with embed_bias NULL, of mms_simcross_bilinear_forward_f16 on
 * the gathered rows.  K > 0, K * D <= 2^31 - 1, else MMS_ERR_INVALID_ARG; MMS_ERR_UNSUPPORTED outside the geometries the
 * _f32 twin covers (W1, W2 <= 48, D <= 64, not W1 == W2 == 1, and N >= 512 or N <= 256 with N * M <= 65535). */
int mms_embed_simcross_bilinear_forward_f16(int N, int W1, int W2, int D, int M, int K, const float* index_q,
                                            const float* index_a, const void* table_f16, const float* embed_bias,
                                            const float* W, const float* bias, float* top, void* stream);
/* The scoring forward of dist_mode 0 (cosine) and 1 (Euclid) straight from word ids and a HALF embedding table (K,D):
 * top == SimCross(Embed(index_q), Embed(index_a)), the twin of mms_embed_simcross_forward_f32 (below), the gather done
 * by the staging loads of the word-grid kernels of mms_simcross_forward_f16.
 *   Operands: index_q (N,W1), index_a (N,W2) word ids as floats, converted with (int) and clamped to [0, K - 1] as there;
 *       table_f16 (K,D) IEEE halves; embed_bias D floats or NULL; top (N,1,W1,W2) fp32; norm0 (N,W1), norm1 (N,W2) fp32,
 *       written in dist_mode 0 (required), ignored in dist_mode 1 (may be NULL).
 *   Row value: embed_bias[d] + widen(table[id][d]), one fp32 add -- the widened half alone when embed_bias is NULL.
 *       Everything after that is the fp32 arithmetic of mms_embed_simcross_forward_f32: the forward sums d ascending
 *       per output, the norms use that call's lane order and wave sum.
 *   Bits: top, and in dist_mode 0 the norms, carry the bits of mms_embed_simcross_forward_f32 run on the table widened
 *       to fp32 -- and, with embed_bias NULL, of mms_simcross_forward_f16 on the gathered rows.  Euclid top is therefore
 *       the reference CPU code's on the widened gathered rows.
 *   No workspace, no allocation, no host synchronisation; safe to capture in a hipGraph.  One launch in dist_mode 1,
 *       three in dist_mode 0 (two norm launches, then the forward), as the twin.
 *   Any D >= 1 and any 2-byte aligned table: alignment and D only select how wide the loads are, never refuse.
 *       W1 == 1 && W2 == 1 is served (by the word-grid kernels, as in the twin).
 *   MMS_ERR_UNSUPPORTED: dist_mode 2 (use mms_embed_simcross_bilinear_forward_f16 above), and any other dist_mode that is
 *       not 0 or 1, answered before the sizes are looked at, as by the twin.  MMS_ERR_INVALID_ARG: whatever
 *       mms_embed_simcross_forward_f32 rejects -- bad sizes, K <= 0, K * D > 2^31 - 1, a NULL required pointer (index_q,
 *       index_a, table_f16, top; the norms in dist_mode 0).  N == 0: MMS_OK.  A call that does not return MMS_OK, and
 *       N == 0, write nothing. */
int mms_embed_simcross_forward_f16(int dist_mode, int N, int W1, int W2, int D, int K, const float* index_q,
                                   const float* index_a, const void* table_f16, const float* embed_bias, float* top,
                                   float* norm0, float* norm1, void* stream);

/* Device scratch needed by the three fp32 calls above (0 is possible). */
size_t mms_simcross_workspace_bytes(int dist_mode, int N, int W1, int W2, int D,
                                    int M);

/* ------------------------------------------------------------------------- *
 * SimMatrix  (q (N,K1), a (N,K2), W (K1,K2) -> top (N,1), s_i = q_i^T W a_i)
 * ------------------------------------------------------------------------- */

/* Replaces SimMatrixLayer<float>::Forward_cpu / Forward_gpu
 *   src/caffe/layers/sim_matrix_layer.cpp:53-65, sim_matrix_layer.cu:21-41.
 * qw_scratch (N,K2) receives Q*W.  The reference uses bottom[1]'s diff buffer
 * for it (:58); pass a_blob->mutable_gpu_diff() to reproduce that side effect. */
int mms_simmatrix_forward_f32(int N, int K1, int K2, const float* q,
                              const float* a, const float* W, float* top,
                              float* qw_scratch, void* stream);

/* The same forward for a caller that owns a workspace (mms_simmatrix_workspace_bytes, the backward's; no
 * initialisation needed): with it, and N >= 2048 pairs, Q*W runs on the BF16 matrix pipe at fp32 accuracy -- every
 * fp32 operand is the exact sum of three bf16 values, the six partial products of weight >= 2^-16 are accumulated in
 * fp32 (csrc/bx3_gemm.h; the three dropped are <= 2^-24 relative) -- 16 x the fp32 pipe's rate per instruction for 6 x
 * the instructions.  Results agree with the fp32-MFMA product of mms_simmatrix_forward_f32 to fp32 rounding (both are
 * inside the 1e-5 contract of this BLAS-backed layer: the reference calls cblas_sgemm, no defined order); an input
 * holding an infinity yields NaN where the fp32 product yields inf.  The three planes hold an operand exactly while its
 * last mantissa bit is at least 2^-133, bf16's smallest subnormal, i.e. for magnitudes from 2^-110 up; a smaller element
 * enters the product rounded to a multiple of 2^-133 (nothing is flushed to zero: absolute error <= 2^-134 per element,
 * relative 2^-24 at 2^-110 growing to 2^-8 at 2^-126); a magnitude of 2^128 - 2^119 (3.3962e38) or more rounds the
 * first plane to infinity and, like an infinity, makes its row NaN (tests/test_gpu_matrix_pipe_accuracy.py holds each
 * kept plane product to a componentwise 2^-20 against fp64).  The backward calls below take the same route for
 * dq (and da) when handed this workspace.  mms_set_matrix_mode(1) pins every product to the fp32 pipe (process-wide;
 * 0 = default), mms_get_matrix_mode() reads it. */
int mms_simmatrix_forward_ws_f32(int N, int K1, int K2, const float* q,
                                 const float* a, const float* W, float* top,
                                 float* qw_scratch, void* workspace,
                                 size_t workspace_bytes, void* stream);
int mms_set_matrix_mode(int mode);
int mms_get_matrix_mode(void);

/* fp16-STORAGE SimMatrix scoring (no reference instantiation: common.hpp:41-44; cfg 5's "fp16 embeddings" with a learned
 * metric): q (N,K1) and a (N,K2) IEEE half in HBM, W (K1,K2) and top (N) fp32; top_i = a_i . (q_i W), the forward of
 * sim_matrix_layer.cpp:53-65 without its Q*W output.  Runs on the bf16 matrix pipe whatever the matrix mode: a half is
 * the exact sum of two bf16 values, so the products are formed exactly and accumulated in fp32 -- the fp32 layer's
 * result on the widened inputs to fp32 rounding (1e-5).  K1 % 8 == 0 (any length), K2 % 4 == 0, K2 <= 320, q 16-byte and a
 * 8-byte aligned, else MMS_ERR_UNSUPPORTED (there is no fp32 fallback).  workspace: mms_simmatrix_workspace_bytes. */
int mms_simmatrix_forward_f16(int N, int K1, int K2, const void* q_f16, const void* a_f16,
                              const float* W, float* top, void* workspace,
                              size_t workspace_bytes, void* stream);
/* The TRAINING pair of the same family: the forward also leaves Q*W (fp32, (N,K2)) in qw_scratch; the backward
 * (sim_matrix_layer.cpp:68-95) takes it back and writes dq (N,K1) and da (N,K2) as halves (rounded RNE from the fp32
 * values; either may be NULL = not propagated) and ACCUMULATES dW (K1,K2) in fp32 (NULL = not propagated).  K1 % 8 == 0
 * and K2 % 8 == 0 (both products take a half operand along their inner dimension), K1, K2 <= 320.  Against the fp32
 * layer on the widened inputs: scores and dW at 1e-5, dq / da at half precision (1e-3). */
int mms_simmatrix_forward_train_f16(int N, int K1, int K2, const void* q_f16, const void* a_f16,
                                    const float* W, float* top, float* qw_scratch, void* workspace,
                                    size_t workspace_bytes, void* stream);
int mms_simmatrix_backward_f16(int N, int K1, int K2, const void* q_f16, const void* a_f16,
                               const float* W, const float* qw, const float* top_diff,
                               void* dq_f16, void* da_f16, float* dW, void* workspace,
                               size_t workspace_bytes, void* stream);

/* Replaces SimMatrixLayer<float>::Backward_cpu / Backward_gpu
 *   src/caffe/layers/sim_matrix_layer.cpp:68-95, sim_matrix_layer.cu:43-46.
 * dW (K1,K2) is ACCUMULATED into when param_propagate_down (:73-80);
 * dq / da are overwritten when their propagate_down flag is set (:81-93) and
 * left untouched otherwise. */
int mms_simmatrix_backward_f32(int N, int K1, int K2, const float* q,
                               const float* a, const float* W,
                               const float* top_diff, int param_propagate_down,
                               int propagate_down0, int propagate_down1,
                               float* dq, float* da, float* dW, void* workspace,
                               size_t workspace_bytes, void* stream);

/* Same call for a caller that kept the forward's product: qw (N,K2) is what
 * mms_simmatrix_forward_f32 wrote to qw_scratch for the SAME q and W, unchanged
 * since.  da_j = dT_j * (W^T q_j) (:88) is row j of that product times dT_j, so
 * the call scales it instead of recomputing it -- same bits as the call above,
 * one GEMM fewer.  qw may be the da buffer itself (in place), which is where the
 * reference's forward leaves it (bottom[1]'s diff, :58). */
int mms_simmatrix_backward_cached_f32(int N, int K1, int K2, const float* q,
                                      const float* a, const float* W,
                                      const float* qw, const float* top_diff,
                                      int param_propagate_down,
                                      int propagate_down0, int propagate_down1,
                                      float* dq, float* da, float* dW,
                                      void* workspace, size_t workspace_bytes,
                                      void* stream);

size_t mms_simmatrix_workspace_bytes(int N, int K1, int K2);

/* ------------------------------------------------------------------------- *
 * PairRankLoss  (a, b, y of `count` = N*C elements -> scalar loss)
 * ------------------------------------------------------------------------- */

/* Replaces PairRankLossLayer<float>::Forward_cpu / Forward_gpu
 *   src/caffe/layers/pair_rank_loss_layer.cpp:26-52, pair_rank_loss_layer.cu:10-43.
 * ordered / similar are the layer's cached ordered_diff_ / similar_diff_ blobs
 * (count floats each, outputs).  loss is ONE device float. */
int mms_pairrank_forward_f32(int count, float margin, const float* a,
                             const float* b, const float* y, float* ordered,
                             float* similar, float* loss, void* workspace,
                             size_t workspace_bytes, void* stream);

/* Replaces PairRankLossLayer<float>::Backward_cpu / Backward_gpu
 *   src/caffe/layers/pair_rank_loss_layer.cpp:55-84, pair_rank_loss_layer.cu:45-83.
 * top_diff = top[0]->cpu_diff()[0] (the loss weight).  Uses the CPU code's
 * strict `ordered > 0` (:76), not the .cu's `>=`.  da / db are overwritten
 * when their flag is set.  (propagate_down[2] is a LOG(FATAL) in the
 * reference and is rejected one level up, in the Layer mirror.) */
int mms_pairrank_backward_f32(int count, float top_diff, const float* y,
                              const float* ordered, const float* similar,
                              int propagate_down0, int propagate_down1,
                              float* da, float* db, void* stream);

size_t mms_pairrank_workspace_bytes(int count);

/* ------------------------------------------------------------------------- *
 * Fused training step of the metric-learning inner loop (one launch, see below):
 *   s_pos = SimCross_euclid(q, a_pos), s_neg = SimCross_euclid(q, a_neg)   (N,1,1,1)
 *   loss  = PairRankLoss(s_pos, s_neg, y)                 (margin, loss_weight)
 *   backward through PairRankLoss and both SimCross layers:
 *   dq = dq(from pos) + dq(from neg)  (Caffe's Split layer sum), da_pos, da_neg.
 * Equivalent net: two SimCross layers sharing bottom q (sim_cross_layer.cpp)
 * feeding PairRankLoss (pair_rank_loss_layer.cpp), geometry W1 = W2 = 1.
 * Outputs equal the layer-by-layer result bitwise, except the loss scalar: it is within 2e-6 of the exact mean of
 * the (bit-exact) per-triplet terms, hence within 1e-5 of the reference's value wherever the reference's fp32
 * running sum is itself that close to the exact mean (for thousands of near-constant terms it drifts by 1-2e-5:
 * DESIGN.md 5); bit-identical to the reference's in MMS_LOSS_SUM_REFERENCE mode (above).
 * `loss` may be NULL: the scalar (a display value: no gradient depends on it) is then not reduced at all -- 7.6
 * instead of 9.6 us of kernel time at 4096 x 300.
 * workspace: mms_triplet_workspace_bytes(N) bytes of 8-byte-aligned device memory that belongs to this call
 * sequence alone: its head holds the arrival words of the in-launch loss sum (zero between launches), the rest one
 * term per triplet.  Call mms_triplet_workspace_init ONCE after allocating it (it zeroes the words, asynchronously
 * on `stream`) -- and again if a launch that used it died mid-way; a workspace sized for a larger N serves any
 * smaller one.  Launches that may be in flight together -- two streams, two captured graphs replayed
 * concurrently -- need a workspace each; nothing about the words is chosen by host state at call or capture time.
 * ------------------------------------------------------------------------- */
/* How the loss scalar of the fused step is summed (per calling thread):
 *   MMS_TRIPLET_FINISH_INLAUNCH (default): the step is ONE launch.  The per-triplet terms are added as integers in
 *       units of 2^-S (S = 42 - ceil(log2 N): 2^-30 at N = 4096), so the sum does not depend on the order in which
 *       workgroups finish, and the arrival count travels in the same 64-bit word as the sum (waves -> workgroup
 *       word in LDS -> one word per 16 workgroups -> top word; the wave that completes the top word writes the
 *       loss).  10.3 us per 4096 x 300 step HBM-cold against 11.2 for the second launch.  Domain: every term
 *       max(0, margin - y*(s_pos - s_neg)) + |(1 - y)*(s_pos - s_neg)| must be below 2^10 -- any margin and labels
 *       below a few hundred.  A term outside it makes the loss NaN (never a wrong number); scores and gradients do
 *       not depend on the mode.  Batches of more than 131072 triplets, and widths other than 100 / 200 / 300, use
 *       the second launch whatever the mode.
 *   MMS_TRIPLET_FINISH_LAUNCH: a second, one-workgroup launch adds the N per-triplet terms in a fixed order (no
 *       limit on the terms). */
#define MMS_TRIPLET_FINISH_LAUNCH 0
#define MMS_TRIPLET_FINISH_INLAUNCH 1
int mms_set_triplet_finish_mode(int mode);
int mms_get_triplet_finish_mode(void);
int mms_triplet_euclid_step_f32(int N, int D, float margin, float loss_weight,
                                const float* q, const float* a_pos,
                                const float* a_neg, const float* y,
                                float* s_pos, float* s_neg, float* loss,
                                float* dq, float* da_pos, float* da_neg,
                                void* workspace, size_t workspace_bytes,
                                void* stream);

size_t mms_triplet_workspace_bytes(int N);
int mms_triplet_workspace_init(void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Fused training step of the COSINE metric (dist_mode 0), one launch:
 *   s_pos = SimCross_cosine(q, a_pos), s_neg = SimCross_cosine(q, a_neg)   (N,1,1,1)
 *   loss  = PairRankLoss(s_pos, s_neg, y)                 (margin, loss_weight)
 *   backward through PairRankLoss and both SimCross layers:
 *   dq = dq(pos) + dq(neg) (Net::Init's Split sum, in that order: one fp32 add of the two rounded values),
 *   da_pos, da_neg.
 * Equivalent net: two SimCross layers with `dist_mode: 0` sharing bottom q (sim_cross_layer.cpp:112-139 forward,
 * :226-250 backward) feeding PairRankLoss (pair_rank_loss_layer.cpp:26-84), geometry W1 = W2 = 1.  It replaces
 * seven launches (two mms_simcross_forward_f32, mms_pairrank_forward_f32 / _backward_f32, two
 * mms_simcross_backward_f32, mms_split_backward_f32) and reads q, a_pos, a_neg once and writes dq, da_pos, da_neg
 * once: 6*N*D*4 bytes.  ||q|| is computed once and serves both branches.
 * Numerics:
 *   - s_pos, s_neg, norm_q, norm_pos, norm_neg equal what mms_simcross_forward_f32(0, ...) writes for the same rows
 *     BIT FOR BIT (same per-lane accumulation order and reduction as the unfused kernel that serves the width: one
 *     definition of the device code, csrc/cosine_math.h), so a ranking of training-time scores is the ranking a
 *     scoring call gives.  Against the reference they are within 1e-5 (its dot products are cblas_sdot: no order).
 *   - dq, da_pos, da_neg equal mms_simcross_backward_f32(0, ...) twice + mms_split_backward_f32 given those scores,
 *     bit for bit: per-pair factors 1/n0/n1, T/n0^2, T/n1^2 and 0 + g*(...) per element at D = 100 / 200 / 300 with
 *     16-byte-aligned arrays, the reference's expression written out elsewhere, as in the unfused kernels.  g+ / g-
 *     are PairRankLoss's (strict `ordered > 0` unless mms_set_pairrank_hinge_mode says otherwise).
 *     The unfused calls choose their kernel per call from D and the 16-byte alignment of the arrays they are given;
 *     this step chooses once, from q, a_pos, a_neg (sum order) and dq, da_pos, da_neg (backward expression).  The
 *     two agree bitwise whenever the unfused calls of both branches would take the same kernel -- always, except
 *     when exactly one of a_pos / a_neg (or of the gradient arrays) breaks 16-byte alignment; then the step uses
 *     the scalar order for both branches and the 1e-5 contract holds.
 *   - loss: as for mms_triplet_euclid_step_f32 -- within 2e-6 of the exact mean of the bit-exact per-triplet terms
 *     (hence within 1e-5 of the reference's value); in MMS_LOSS_SUM_REFERENCE mode the reference-order fp32 running
 *     sum of the terms formed from this step's own scores.  `loss` may be NULL (no reduction).
 *   - a zero q or answer row gives the reference's 0/0: NaN exactly where the unfused chain gives NaN.
 *   - deterministic: no atomics on floats, two calls give identical bits.
 * norm_q / norm_pos / norm_neg: (N) each, what the layers cache as norm0 / norm1; any of them may be NULL.
 * workspace: the Euclid step's -- mms_triplet_workspace_bytes(N), mms_triplet_workspace_init, same ownership rules,
 * same finish modes (mms_set_triplet_finish_mode; in-launch at D = 100 / 200 / 300 with aligned inputs and at most
 * 131072 triplets, second launch otherwise).  A cosine term is at most margin + 2, so the in-launch domain (terms
 * below 2^10) admits the same margins.  N == 0 is a no-op; a workspace that is too small, NULL or not 8-byte aligned
 * returns MMS_ERR_WORKSPACE.
 * Measured (tools/triplet_cosine_probe.py, HBM-cold ring, graph-replayed, profiles/triplet_cosine_probe.txt): 8.45 us
 * per 4096 x 300 step (0.44 of 8 TB/s on 6*N*D*4 bytes) against 26.7 us for the seven launches and 9.47 us for the
 * Euclid step in the same run; 16384 x 300: 26.7 against 64.2 and 29.8 us.
 * ------------------------------------------------------------------------- */
int mms_triplet_cosine_step_f32(int N, int D, float margin, float loss_weight,
                                const float* q, const float* a_pos,
                                const float* a_neg, const float* y,
                                float* s_pos, float* s_neg,
                                float* norm_q, float* norm_pos, float* norm_neg,
                                float* loss,
                                float* dq, float* da_pos, float* da_neg,
                                void* workspace, size_t workspace_bytes,
                                void* stream);

/* ------------------------------------------------------------------------- *
 * Fused training step of the LEARNED metric (cfg 3's arithmetic):
 *   s_pos_i = q_i^T W a_pos_i, s_neg_i = q_i^T W a_neg_i          SimMatrix x 2, W shared (sim_matrix_layer.cpp:53-65)
 *   loss = PairRankLoss(s_pos, s_neg, y)                            (pair_rank_loss_layer.cpp:26-52)
 *   backward through PairRankLoss (:55-84) and both SimMatrix layers (sim_matrix_layer.cpp:68-95):
 *   dq = dq(pos) + dq(neg) (Net::Init's Split sum), da_pos, da_neg, dW += both branches' q_i a_i^T terms (param
 *   diffs accumulate, as in the layers).
 * Equivalent net: two SimMatrix layers with bottom q in common and `param { name }` in common, feeding PairRankLoss.
 * Three products instead of the layers' six: Q W once for both branches -- its epilogue forms both scores, the hinge
 * term and its gradients g+, g- per row, and writes da_pos = g+ (W^T q), da_neg = g- (W^T q) and B = g+ a_pos + g- a_neg;
 * then dq = B W^T and dW += Q^T B.  Neither Q W nor the (N, 1) score gradients reach HBM.  Scores, loss terms and
 * hinge decisions follow the reference's operation order given the scores; everything that passes through a product
 * agrees with the layer-by-layer result to 1e-5 (the reference's own products go through CBLAS).
 * Shapes the panel kernel does not serve (K1 or K2 > 304, K1 or K2 not a multiple of 4, fewer than 6081 triplets --
 * 96 panels of 64 rows -- or N not a multiple of 4) run the layers one by one
 * inside the call: same results, no fusion.  `loss` may be NULL.  dW is accumulated into (zero it like
 * Net::ClearParamDiffs does).  workspace: mms_triplet_simmatrix_workspace_bytes(N, K1, K2), no initialisation needed.
 * ------------------------------------------------------------------------- */
size_t mms_triplet_simmatrix_workspace_bytes(int N, int K1, int K2);
int mms_triplet_simmatrix_step_f32(int N, int K1, int K2, float margin, float loss_weight,
                                   const float* q, const float* a_pos, const float* a_neg, const float* y,
                                   const float* W, float* s_pos, float* s_neg, float* loss,
                                   float* dq, float* da_pos, float* da_neg, float* dW,
                                   void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Ranking metrics over the scores (forward only).  These
 * define "ranking output": with the Euclidean scores bit-identical to the CPU
 * code, MAP/MRR/AUC computed here are bit-identical too wherever the sort order
 * is defined (ties between EQUAL scores are implementation-defined in the
 * reference's unstable std::sort; here they keep original order -- which is also what
 * libstdc++'s std::sort does for a bucket of at most 16 items, its stable insertion sort:
 * MAP / MRR over candidate groups that small match a libstdc++ build of the reference bit
 * for bit even when tied scores carry different labels).
 * Labels and group ids are taken as int(x), as the reference stores them: labels are not
 * limited to {0, 1} (MAP counts a bucket with a label 1 and any label != 1, MRR one with a
 * label 1 and a label 0; 0.7 -> 0, 1.9 -> 1), and -0.5 / 0.5 are both group 0.
 * -0.0 and +0.0 are EQUAL scores, as under the reference's `lhs.first > rhs.first`.
 * NaN scores: the reference's comparator is then no strict weak order and its result is
 * undefined; so is the result here.
 * ------------------------------------------------------------------------- */

/* Order of EQUAL scores that carry different labels (MAP / MRR / AUC; per calling thread).
 *   MMS_RANK_TIES_INPUT_ORDER (default): ties keep the input order -- also what libstdc++ does in buckets of at
 *       most 16 items.
 *   MMS_RANK_TIES_LIBSTDCXX: the order a libstdc++ build of the reference leaves them in -- buckets of more than
 *       16 items that contain such a tie are re-sorted by a step-by-step restatement of libstdc++'s std::sort
 *       (csrc/libstdcxx_sort.h: introsort with median-of-three partitioning, heap-sort fallback, final insertion
 *       sort; checked against the real std::sort by tests/test_libstdcxx_sort.py) on the bucket's items in their
 *       original order.  Sequential, one lane per bucket, hence opt-in (tools/rank_ties_probe.py, heavily tied
 *       scores): MAP + MRR over 1,517 candidates in groups of ~22: 147 instead of 91 us; AUC, whose one bucket is
 *       the whole input: 4.4 ms instead of 60 us at 1,517 items, 117 ms at 20,000.  Without such a tie the mode
 *       costs its detection pass only. */
#define MMS_RANK_TIES_INPUT_ORDER 0
#define MMS_RANK_TIES_LIBSTDCXX 1
int mms_set_rank_tie_mode(int mode);
int mms_get_rank_tie_mode(void);

/* Replaces MAPLayer<float>::Forward_cpu (src/caffe/layers/map_layer.cpp:41-100) and
 * MRRLayer<float>::Forward_cpu (src/caffe/layers/mrr_layer.cpp:38-79).
 * prob (n, fixed_axis+1): the score of item i is prob[i*(fixed_axis+1)+fixed_axis];
 * label (n), taken as int(label[i]); group (n): items are bucketed by int(group[i]).
 * map_out / mrr_out / effective_out (device scalars) may each be NULL. */
int mms_rank_map_mrr_f32(int n, int fixed_axis, const float* prob, const float* label,
                         const float* group, float* map_out, float* mrr_out,
                         int* effective_out, void* workspace, size_t workspace_bytes,
                         void* stream);

/* Replaces AUCLayer<float>::Forward_cpu (src/caffe/layers/auc_layer.cpp:47-136) for
 * inner_num = 1: prob (n, dim), score = prob[i*dim + fixed_axis]. */
int mms_rank_auc_f32(int n, int dim, int fixed_axis, const float* prob, const float* label,
                     int has_ignore_label, int ignore_label, float* auc_out,
                     void* workspace, size_t workspace_bytes, void* stream);

/* The same layer for any label axis: prob (outer, channels, inner) -- bottom[0] with `axis` as its label axis,
 * outer = count(0, axis), inner = count(axis + 1) -- and label (outer, inner); item (o, j) scores
 * prob[o*channels*inner + fixed_axis*inner + j] (auc_layer.cpp:66-77).  Items whose label equals ignore_label are
 * skipped when has_ignore_label (:69-71).  Workspace: mms_rank_workspace_bytes(outer * inner). */
int mms_rank_auc_nd_f32(int outer, int channels, int inner, int fixed_axis, const float* prob,
                        const float* label, int has_ignore_label, int ignore_label, float* auc_out,
                        void* workspace, size_t workspace_bytes, void* stream);

/* Replaces RankAccuracyLayer<float>::Forward_cpu
 * (src/caffe/layers/rank_accuracy_layer.cpp:36-50): mean of [label*(a-b) > 0]. */
int mms_rank_accuracy_f32(int count, const float* a, const float* b, const float* label,
                          float* acc_out, void* workspace, size_t workspace_bytes,
                          void* stream);

size_t mms_rank_workspace_bytes(int n);

/* ------------------------------------------------------------------------- *
 * Embed -- the layer that produces SimCross's bottoms.
 * index (M) holds word ids as floats (Caffe feeds them as Dtype), weight (K,N),
 * bias (N) or NULL, top (M,N).
 * ------------------------------------------------------------------------- */

/* Replaces EmbedLayer<float>::Forward_cpu / Forward_gpu
 *   src/caffe/layers/embed_layer.cpp:135-152, embed_layer.cu:42-62. */
int mms_embed_forward_f32(int M, int N, int K, const float* index, const float* weight,
                          const float* bias, float* top, void* stream);

/* Replaces EmbedLayer<float>::Backward_cpu / Backward_gpu
 *   src/caffe/layers/embed_layer.cpp:155-180, embed_layer.cu:64-88.
 * weight_diff (K,N) is ACCUMULATED into in the CPU code's n-ascending order
 * (bit-identical; the reference's .cu uses atomicAdd).  bias_diff (N) likewise
 * accumulated (BLAS-ordered in the reference: 1e-5).  Either may be NULL
 * (= param_propagate_down false). */
int mms_embed_backward_f32(int M, int N, int K, const float* index, const float* top_diff,
                           float* weight_diff, float* bias_diff, void* workspace,
                           size_t workspace_bytes, void* stream);
/* Two Embed layers that share ONE table (and bias) -- network_v4's w2v_q / w2v_a, do_trec_qa_clean.py:452-467 --
 * back-propagated in one pass: exactly mms_embed_backward_f32(layer 0) followed by mms_embed_backward_f32(layer 1) into
 * the same weight_diff / bias_diff (pass the layer whose Backward the net runs first -- the LATER layer of the file --
 * as layer 0), with the same bits in weight_diff (a table row's additions keep the order "layer 0's rows ascending,
 * then layer 1's"), but the inverted index is built once over M0 + M1 indices, every touched table row is read and
 * written once, and the bias gradient is one column sum.  workspace: mms_embed_workspace_bytes(M0 + M1, N). */
int mms_embed_backward_pair_f32(int M0, int M1, int N, int K, const float* index0, const float* top_diff0,
                                const float* index1, const float* top_diff1, float* weight_diff, float* bias_diff,
                                void* workspace, size_t workspace_bytes, void* stream);
/* The same pair with the inverted index built in the FORWARD pass: it depends on the word ids alone, the one-workgroup
 * sort that builds it takes ~14 us, and beside the forward's gathers it costs nothing.
 *   mms_embed_forward_pair_f32: top0 = Embed(index0), top1 = Embed(index1) (embed_layer.cpp:135-152 twice) in ONE
 *       launch; with index_workspace != NULL (mms_embed_workspace_bytes(M0 + M1, N)) and
 *       mms_embed_pair_index_supported(M0, M1, K) it also writes the index of the ids in the order (index0, index1).
 *   mms_embed_backward_pair_indexed_f32: mms_embed_backward_pair_f32 minus the index build; index0 / index1 and the
 *       workspace must be the ones the forward call was given, in the same order, and the workspace untouched since.
 *       (For the reference's nets pass the LATER layer of the file as layer 0 in BOTH calls: Net::Backward reaches it first.) */
int mms_embed_pair_index_supported(int M0, int M1, int K);
int mms_embed_forward_pair_f32(int M0, int M1, int N, int K, const float* index0, const float* index1,
                               const float* weight, const float* bias, float* top0, float* top1, void* index_workspace,
                               size_t index_workspace_bytes, void* stream);
int mms_embed_backward_pair_indexed_f32(int M0, int M1, int N, int K, const float* index0, const float* top_diff0,
                                        const float* index1, const float* top_diff1, float* weight_diff, float* bias_diff,
                                        void* index_workspace, size_t index_workspace_bytes, void* stream);

size_t mms_embed_workspace_bytes(int M, int N);

/* fp16-STORAGE Embed (no reference instantiation: common.hpp:41-44): the Embed ends of the fp16-storage word-grid family
 * (mms_simcross_*_f16, mms_simcross_bilinear_*_f16 above).  The forwards gather a HALF table into the half (N,W,D) grids
 * those calls read; the backwards take the half dq / da those calls leave and add them into the fp32 master gradient of
 * the table in the reference's order.  Each call is the twin of the _f32 call of the same name, above.
 *   Operands: index* word ids as floats, converted with (int) and clamped to [0, K - 1] exactly as the twins do;
 *       table_f16 (K,N), top*_f16 (M,N), top_diff*_f16 (M,N) IEEE halves; bias (N) fp32 or NULL; weight_diff (K,N) and
 *       bias_diff (N) fp32, accumulated into as in the twin, either may be NULL.
 *   Forward: with bias NULL, top[n,d] is the table's half copied bit for bit (NaN payloads, +-Inf, subnormals pass
 *       through).  With a bias, top[n,d] = RNE_half(bias[d] + widen(table[id][d])): the one fp32 add of the twin, then one
 *       rounding to nearest even (overflow gives +-Inf) -- mms_embed_forward_f32 on the widened table, rounded once.  With
 *       bias NULL, mms_simcross_forward_f16 on these grids carries the bits of mms_embed_simcross_forward_f16 from the
 *       same ids.
 *   Backward: every half of top_diff is widened exactly; everything after that is the fp32 arithmetic of the twin.
 *       weight_diff[id,:] receives its rows one by one, n ascending, on top of the value already there
 *       (embed_layer.cpp:155-180); for the pair calls layer 0's rows, then layer 1's.  weight_diff AND bias_diff carry
 *       the bits of the _f32 twin run on the widened top_diff -- weight_diff therefore the reference CPU code's bits on
 *       those values.
 *   Workspace: mms_embed_workspace_bytes(M, N) (M0 + M1 for the pair calls) serves the _f16 calls unchanged: the layout
 *       holds ids, row numbers and fp32 partial sums, nothing of the storage type.
 *   Inverted index: it depends on the ids alone.  mms_embed_forward_pair_f16 writes the same workspace contents as
 *       mms_embed_forward_pair_f32 for the same ids, under the same mms_embed_pair_index_supported rule; an index built by
 *       either forward serves either indexed backward.
 *   Any N >= 1 and any 2-byte aligned half operands: alignment and N only select how wide the loads and stores are,
 *       never refuse.
 *   No allocation, no host synchronisation; safe to capture in a hipGraph.  No floating-point atomics: the results are
 *       deterministic.  None of the per-thread arithmetic modes is consulted.
 *   Errors: argument tuple for argument tuple those of the _f32 twins.  M == 0 (single-layer calls): MMS_OK.
 *       weight_diff == bias_diff == NULL: MMS_OK.  The indexed call with sizes mms_embed_pair_index_supported refuses:
 *       MMS_ERR_UNSUPPORTED.  A missing or short workspace: MMS_ERR_WORKSPACE.  Bad sizes (M < 0, M0 or M1 <= 0, N <= 0,
 *       K <= 0, M * N > 2^31 - 1) or a NULL required pointer: MMS_ERR_INVALID_ARG.  A call that does not return MMS_OK
 *       writes nothing, and nothing past an output's last element is ever written. */
int mms_embed_forward_f16(int M, int N, int K, const float* index, const void* table_f16,
                          const float* bias, void* top_f16, void* stream);
int mms_embed_forward_pair_f16(int M0, int M1, int N, int K, const float* index0, const float* index1,
                               const void* table_f16, const float* bias, void* top0_f16, void* top1_f16,
                               void* index_workspace, size_t index_workspace_bytes, void* stream);
int mms_embed_backward_f16(int M, int N, int K, const float* index, const void* top_diff_f16,
                           float* weight_diff, float* bias_diff, void* workspace,
                           size_t workspace_bytes, void* stream);
int mms_embed_backward_pair_f16(int M0, int M1, int N, int K, const float* index0, const void* top_diff0_f16,
                                const float* index1, const void* top_diff1_f16, float* weight_diff,
                                float* bias_diff, void* workspace, size_t workspace_bytes, void* stream);
int mms_embed_backward_pair_indexed_f16(int M0, int M1, int N, int K, const float* index0, const void* top_diff0_f16,
                                        const float* index1, const void* top_diff1_f16, float* weight_diff,
                                        float* bias_diff, void* index_workspace, size_t index_workspace_bytes,
                                        void* stream);

/* Embed fused into SimCross's loads (forward / scoring; dist_mode 0 or 1):
 *   top == SimCross(Embed(index_q), Embed(index_a))
 * i.e. embed_layer.cpp:135-152 followed by sim_cross_layer.cpp:96-139, without the (N,W,D) blobs in
 * between.  index_q (N,W1) and index_a (N,W2) hold word ids as floats, clamped into [0,K) like
 * mms_embed_forward_f32; weight (K,D) is the table BOTH Embed layers read (the driver shares it by
 * parameter name, do_trec_qa_clean.py:462-467); embed_bias (D) is their shared bias blob or NULL
 * (bias_term false) -- the driver's Embed layers DO carry one (`bias_term` is left at its default,
 * the `#bias_term=False` of :462 is commented out), so a row is bias[d] + weight[id][d], one
 * rounding, as the layer's gemm gives it (:146-151); top (N,1,W1,W2); norm0 (N,W1) / norm1 (N,W2)
 * receive the row norms in dist_mode 0 (NULL otherwise).  Results are the bits of the two separate
 * calls (Euclid: the reference's CPU bits).  dist_mode 2 has its own entry point below (it needs
 * W and bias). */
int mms_embed_simcross_forward_f32(int dist_mode, int N, int W1, int W2, int D, int K,
                                   const float* index_q, const float* index_a,
                                   const float* weight, const float* embed_bias, float* top,
                                   float* norm0, float* norm1, void* stream);

/* The same fusion for dist_mode 2, the mode network_v4 scores with (do_trec_qa_clean.py:468):
 *   top (N,M,W1,W2) == SimCross_bilinear(Embed(index_q), Embed(index_a); W (M,D,D), bias (M,W1,W2) or NULL)
 * embed_layer.cpp:135-152 (embed_bias as above) followed by sim_cross_layer.cpp:140-161, ONE launch: the word-grid
 * forward kernels gather their q / a images from the table themselves.  Same kernels and operand values as
 * mms_embed_forward_f32 x2 + mms_simcross_forward_f32, hence the same bits (1e-5 vs the reference: BLAS order).
 * Covers the word-grid geometries of the fused forward (W1, W2 <= 48, D <= 64, and either N >= 512 or
 * N <= 256 with N*M <= 65535); anything else returns MMS_ERR_UNSUPPORTED -- run the two layers separately. */
int mms_embed_simcross_bilinear_forward_f32(int N, int W1, int W2, int D, int M, int K,
                                            const float* index_q, const float* index_a,
                                            const float* weight, const float* embed_bias,
                                            const float* W, const float* bias, float* top, void* stream);

/* ------------------------------------------------------------------------- *
 * FM: second-order factorization-machine pooling over the channels of a blob
 * (src/caffe/layers/fm_layer.cpp, fm_param { bias_term }, caffe.proto:415-420).
 * x is contiguous (N, C, dim): element (i, k, j) at i*C*dim + k*dim + j, which is
 * what the reference reads (channels() and height(); width() is ignored, so a
 * blob with width > 1 is NOT this layout).  Column 0 of a channel is its linear
 * term, columns 1..dim-1 its latent factors:
 *   top[i] = 1/2 sum_{j>=1} [ (sum_k x_ikj)^2 - sum_k x_ikj^2 ] + sum_k x_ik0 + bias
 * top is (N, 1), the shape PairRankLoss consumes.  Any C >= 1, dim >= 1, N >= 0;
 * MMS_ERR_INVALID_ARG for N < 0, C <= 0, dim <= 0, N*C*dim > INT_MAX (the
 * reference indexes with int) or a NULL required array with N > 0; N == 0
 * launches nothing.  One launch per call, no workspace, no atomics.  All results
 * are BIT-IDENTICAL to the reference CPU code: its loop order fixes them
 * (one ordered chain of (dim-1)(C+1) + C + 1 adds per sample).
 * ------------------------------------------------------------------------- */

/* Replaces FMLayer<float>::Forward_cpu / Forward_gpu
 *   src/caffe/layers/fm_layer.cpp:33-62, fm_layer.cu:12-15 (which calls the CPU code).
 * bias: blobs_[0], ONE device float; NULL = bias_term false.  top: N floats. */
int mms_fm_forward_f32(int N, int C, int dim, const float* x, const float* bias, float* top, void* stream);

/* Replaces FMLayer<float>::Backward_cpu / Backward_gpu
 *   src/caffe/layers/fm_layer.cpp:65-99, fm_layer.cu:17-21.
 * bottom_diff (N*C*dim floats; NULL = propagate_down[0] false): every element is
 * OVERWRITTEN; it must not alias x.  bias_diff (ONE device float; NULL = no bias
 * term, or param_propagate_down_[0] false) is OVERWRITTEN with the ascending sum
 * of top_diff, as the reference zeroes it itself (:77) -- it is not accumulated
 * into.  x and top_diff are required even when bottom_diff is NULL. */
int mms_fm_backward_f32(int N, int C, int dim, const float* x, const float* top_diff, float* bottom_diff,
                        float* bias_diff, void* stream);

/* Both of the above in one launch, for a host that knows top_diff up front (as
 * mms_simcross_forward_backward_f32): x is read from HBM once; top, bottom_diff
 * and bias_diff hold the same bits as after the two separate calls.  bottom_diff
 * is required (and must not alias x); bias and bias_diff are each optional. */
int mms_fm_forward_backward_f32(int N, int C, int dim, const float* x, const float* bias, const float* top_diff,
                                float* top, float* bottom_diff, float* bias_diff, void* stream);

/* ------------------------------------------------------------------------- *
 * BN: the fork's batch normalisation (include/caffe/layers/batch_norm_v0_layer.hpp,
 * src/caffe/layers/bn_layer.cpp / .cu, bn_param { scale_filler shift_filler
 * bn_memory = 0.9 }, caffe.proto:484-488).  x and top are contiguous (N, C, S)
 * with S = H*W: element (n, c, s) at (n*C + c)*S + s.  Per channel c, over its
 * N*S elements:
 *   TRAIN (phase 0)  mean = (1/N)(1/S) sum x;  var = (1/N)(1/S) sum x*x - mean*mean
 *                    running_mean = (1 - bn_memory)*mean + bn_memory*running_mean
 *                    running_var  = (1 - bn_memory)*var  + bn_memory*running_var
 *   TEST  (phase 1)  mean = running_mean, var = running_var (both only read)
 *   std = sqrt(var + 1e-9);  xn = (x + (-mean)) / std;  top = xn*scale + shift
 *   backward: shift_diff = sum dy;  scale_diff = sum xn*dy;  g = dy*scale;
 *             bottom_diff = (g - (xn * sum xn*g + sum g) / (N*S)) / std
 * scale, shift, running_mean, running_var are the layer's blobs_[0..3], C
 * elements each; save_mean / save_std (C each) are its batch_mean_ /
 * batch_variance_ after Forward (the latter holds the standard deviation), which
 * Backward reads -- whichever phase the last forward ran in.  xn is not stored:
 * backward recomputes it from x with the forward's two operations.  var is not
 * clamped (as in the reference, a channel whose var rounds below -1e-9 is NaN).
 * The reference's sums are BLAS gemv's (1e-5 class); the order
 * here is fixed: no atomics, the same words on every run, on either side of the
 * routing threshold and whether or not the arrays allow 16-byte accesses.
 *
 * Any S >= 1, C >= 1, N >= 0 and any element-aligned arrays.  Host-side, before
 * anything is enqueued: MMS_ERR_INVALID_ARG for N < 0, C <= 0, S <= 0,
 * N*C*S > INT_MAX, a phase other than 0 / 1 or, with N > 0, a NULL required array
 * or top == x (the reference's CHECK_NE: no in-place); N == 0 launches nothing;
 * MMS_ERR_WORKSPACE when the workspace is NULL or smaller than the query and the
 * call needs it (TRAIN forward and backward; TEST forward never does).
 *
 * workspace: mms_bn_workspace_bytes(N, C, S), 0 where one workgroup per channel
 * serves (one launch per pass).  Otherwise a channel's 16-byte groups are cut
 * into K = bytes / (C * 4 * sizeof(element)) chunks; launch 1 leaves the sums of
 * chunk k of channel c in words (c*K + k)*4 + {0..3} of the workspace (forward:
 * sum x, sum x*x; backward: sum dy, sum xn*dy, sum g, sum xn*g) and launch 2 adds
 * them in ascending k, starting from chunk 0's.
 * ------------------------------------------------------------------------- */
size_t mms_bn_workspace_bytes(int N, int C, int S);

/* Replaces BNLayer<float>::Forward_cpu / Forward_gpu
 *   src/caffe/layers/bn_layer.cpp:122-257, bn_layer.cu.
 * All arrays are required; top must not be x.  TRAIN updates running_mean and
 * running_var in place; TEST reads them. */
int mms_bn_forward_f32(int phase, int N, int C, int S, float bn_memory, const float* x, const float* scale,
                       const float* shift, float* running_mean, float* running_var, float* top, float* save_mean,
                       float* save_std, void* workspace, size_t workspace_bytes, void* stream);

/* Replaces BNLayer<float>::Backward_cpu / Backward_gpu
 *   src/caffe/layers/bn_layer.cpp:262-383, bn_layer.cu.
 * bottom_diff (N*C*S), scale_diff (C) and shift_diff (C) may each be NULL, which
 * skips that output; at least one must be given.  Each one given is OVERWRITTEN
 * -- the reference's gemv's run with beta = 0, so the two parameter diffs are not
 * accumulated into.  bottom_diff must not alias x or top_diff. */
int mms_bn_backward_f32(int N, int C, int S, const float* x, const float* top_diff, const float* scale,
                        const float* save_mean, const float* save_std, float* bottom_diff, float* scale_diff,
                        float* shift_diff, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * BN -> AvePool -> TanH in one call: what network_v4 does with both of its BN
 * outputs (do_trec_qa_clean.py:472-477).  Replaces, in sequence,
 *   BNLayer (bn_layer.cpp), PoolingLayer AVE (pooling_layer.cpp:197-212,
 *   :291-317) and the in-place TanHLayer (tanh_layer.cpp:13-33)
 * for poolings whose windows TILE the map: kernel (kh, kw) with H % kh == 0 and
 * W % kw == 0, stride == kernel, no padding -- or ONE window that is the whole
 * map, whatever stride it declares.  Every window then has pool_size = kh*kw.
 * Any other pooling is MMS_ERR_INVALID_ARG here: call mms_bn_forward and pool in
 * the host.  x and bottom_diff are (N, C, H, W); top, top_diff and save_pool
 * are (N, C, H/kh, W/kw); every other array has C elements.
 *   mean, var, std = sqrt(var + 1e-9), running blobs: as mms_bn_forward
 *   m = window_mean(x): the window's elements added in (h, w) order, / (kh*kw)
 *   save_pool = (m + (-mean)) / std        (the pooled normalised map)
 *   top = tanh(save_pool*scale + shift)    (the TanH's blob: it runs in place)
 *   backward: gp = top_diff*(1 - top*top);  shift_diff = sum gp;
 *             scale_diff = sum gp*save_pool;  a = scale*scale_diff;
 *             b = scale*shift_diff;  xn = (x + (-mean)) / std;
 *             bottom_diff = (gp/(kh*kw)*scale + (-1/(N*H*W))*(xn*a + b)) / std
 * The BN output itself is never formed: a host that needs it calls
 * mms_bn_forward.  x is read once per pass and bottom_diff written once; the
 * rest of the traffic is pooled-size.  Sums have a fixed order (no atomics;
 * DESIGN.md 4.12a): the same words on every run, on either route, whatever the
 * arrays' alignment and whatever the workspace held.
 *
 * Host-side, before anything is enqueued: MMS_ERR_INVALID_ARG for N < 0, C, H, W,
 * kh or kw below 1, windows that do not tile the map, N*C*H*W > INT_MAX, a
 * phase other than 0 / 1 or, with N > 0, a NULL required array, top or save_pool
 * equal to an input or to each other, bottom_diff equal to an input; N == 0
 * launches nothing; then MMS_ERR_WORKSPACE when the workspace is NULL or
 * smaller than the query and the call needs it (TRAIN forward and backward).
 *
 * workspace: 0 where one workgroup per channel serves (at most 64 KB of x per
 * channel: one launch per pass); otherwise two launches per pass (TEST forward:
 * always one).  Backward: bottom_diff, scale_diff, shift_diff may each be NULL
 * (skipped), at least one is required; those given are overwritten.
 * ------------------------------------------------------------------------- */
size_t mms_bn_pool_tanh_workspace_bytes(int N, int C, int H, int W, int kh, int kw);
int mms_bn_pool_tanh_forward_f32(int phase, int N, int C, int H, int W, int kh, int kw, float bn_memory,
                                 const float* x, const float* scale, const float* shift, float* running_mean,
                                 float* running_var, float* top, float* save_pool, float* save_mean, float* save_std,
                                 void* workspace, size_t workspace_bytes, void* stream);
int mms_bn_pool_tanh_backward_f32(int N, int C, int H, int W, int kh, int kw, const float* x, const float* top,
                                  const float* top_diff, const float* save_pool, const float* scale,
                                  const float* save_mean, const float* save_std, float* bottom_diff, float* scale_diff,
                                  float* shift_diff, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Batch feed: dst[i,:] = src[perm[first+i],:], i < rows,
 * for a dataset (src_rows, row_elems) resident in HBM; perm (src_rows ints on
 * the device) or NULL for the identity; first + rows <= src_rows.
 * A perm entry outside [0, src_rows) reads the nearest valid row (0 or src_rows - 1).
 * Replaces the per-row caffe_copy loop of HDF5DataLayer<float>::Forward_cpu/_gpu
 *   src/caffe/layers/hdf5_data_layer.cpp:124-151, hdf5_data_layer.cu:19-51.
 * ------------------------------------------------------------------------- */
int mms_feed_gather_rows_f32(int rows, int row_elems, int src_rows, const float* src, const int* perm,
                             int first, float* dst, void* stream);

/* ------------------------------------------------------------------------- *
 * double instantiation.  The reference instantiates every layer for float and
 * double (INSTANTIATE_CLASS, include/caffe/common.hpp:41-44); these are what a
 * Layer<double>::Forward_gpu / Backward_gpu binds.  Same argument meaning and
 * error behaviour as the _f32 functions above (no norm / workspace differences
 * except that SimMatrix backward and PairRankLoss need no workspace).  The
 * kernels are functional rather than tuned (csrc/f64_paths.hip); Euclidean
 * results, PairRankLoss (loss included) and dbias are bit-identical to the CPU
 * code, BLAS-backed results agree to ~1e-12.
 * ------------------------------------------------------------------------- */
size_t mms_simcross_workspace_bytes_f64(int dist_mode, int N, int W1, int W2, int D, int M);
int mms_simcross_forward_f64(int dist_mode, int N, int W1, int W2, int D, int M, const double* q,
                             const double* a, const double* W, const double* bias, double* top,
                             double* norm0, double* norm1, void* workspace, size_t workspace_bytes,
                             void* stream);
int mms_simcross_backward_f64(int dist_mode, int N, int W1, int W2, int D, int M, const double* q,
                              const double* a, const double* W, int bias_term, const double* top,
                              const double* top_diff, const double* norm0, const double* norm1,
                              int propagate_down0, int propagate_down1, double* dq, double* da,
                              double* dW, double* dbias, void* workspace, size_t workspace_bytes,
                              void* stream);
int mms_simmatrix_forward_f64(int N, int K1, int K2, const double* q, const double* a,
                              const double* W, double* top, double* qw_scratch, void* stream);
int mms_simmatrix_backward_f64(int N, int K1, int K2, const double* q, const double* a,
                               const double* W, const double* top_diff, int param_propagate_down,
                               int propagate_down0, int propagate_down1, double* dq, double* da,
                               double* dW, void* stream);
int mms_pairrank_forward_f64(int count, double margin, const double* a, const double* b,
                             const double* y, double* ordered, double* similar, double* loss,
                             void* stream);
int mms_pairrank_backward_f64(int count, double top_diff, const double* y, const double* ordered,
                              const double* similar, int propagate_down0, int propagate_down1,
                              double* da, double* db, void* stream);
/* FMLayer<double>: same arguments and errors as mms_fm_forward_f32 / mms_fm_backward_f32, same loop order, the
 * bits of the reference's double instantiation (one thread per output; csrc/fm.hip). */
int mms_fm_forward_f64(int N, int C, int dim, const double* x, const double* bias, double* top, void* stream);
int mms_fm_backward_f64(int N, int C, int dim, const double* x, const double* top_diff, double* bottom_diff,
                        double* bias_diff, void* stream);
/* BNLayer<double>: the arguments, errors, routes and fixed order of mms_bn_forward_f32 / mms_bn_backward_f32 with
 * every float a double (16-byte groups are 2 elements; var_eps_ is the double 1e-9); ~1e-12 vs the reference. */
size_t mms_bn_workspace_bytes_f64(int N, int C, int S);
int mms_bn_forward_f64(int phase, int N, int C, int S, double bn_memory, const double* x, const double* scale,
                       const double* shift, double* running_mean, double* running_var, double* top,
                       double* save_mean, double* save_std, void* workspace, size_t workspace_bytes, void* stream);
int mms_bn_backward_f64(int N, int C, int S, const double* x, const double* top_diff, const double* scale,
                        const double* save_mean, const double* save_std, double* bottom_diff, double* scale_diff,
                        double* shift_diff, void* workspace, size_t workspace_bytes, void* stream);
/* mms_bn_pool_tanh_* with every float a double: the same arguments, errors, routes and fixed order (a 16-byte access
 * is 2 elements); ~1e-12 vs the three reference layers in sequence. */
size_t mms_bn_pool_tanh_workspace_bytes_f64(int N, int C, int H, int W, int kh, int kw);
int mms_bn_pool_tanh_forward_f64(int phase, int N, int C, int H, int W, int kh, int kw, double bn_memory,
                                 const double* x, const double* scale, const double* shift, double* running_mean,
                                 double* running_var, double* top, double* save_pool, double* save_mean,
                                 double* save_std, void* workspace, size_t workspace_bytes, void* stream);
int mms_bn_pool_tanh_backward_f64(int N, int C, int H, int W, int kh, int kw, const double* x, const double* top,
                                  const double* top_diff, const double* save_pool, const double* scale,
                                  const double* save_mean, const double* save_std, double* bottom_diff,
                                  double* scale_diff, double* shift_diff, void* workspace, size_t workspace_bytes,
                                  void* stream);

/* EmbedLayer<double> (embed_layer.cpp:135-180): the arguments, errors and M == 0 behaviour of mms_embed_forward_f32 /
 * mms_embed_backward_f32 with every float* a double* (word ids are doubles: Caffe feeds them as Dtype).  top and
 * weight_diff carry the bits of the reference's double instantiation (same inverted index, the per-row sums in n
 * order), bias_diff is BLAS-ordered there: ~1e-12.  Rows move in 16-byte accesses in the forward when N is even and
 * weight / bias / top are 16-byte aligned.  workspace: mms_embed_workspace_bytes_f64(M, N).  The pair and the fused
 * Embed calls exist for float only. */
size_t mms_embed_workspace_bytes_f64(int M, int N);
int mms_embed_forward_f64(int M, int N, int K, const double* index, const double* weight,
                          const double* bias, double* top, void* stream);
int mms_embed_backward_f64(int M, int N, int K, const double* index, const double* top_diff,
                           double* weight_diff, double* bias_diff, void* workspace,
                           size_t workspace_bytes, void* stream);
/* MAPLayer / MRRLayer / AUCLayer / RankAccuracyLayer<double>: the arguments and errors of the _f32 calls.  The
 * reference's comparators take std::pair<float, int> for every Dtype (map_layer.cpp:34, mrr_layer.cpp:33,
 * auc_layer.cpp:42 -- AUC's vector holds pair<Dtype, int>, std::sort converts its elements for the comparator), so
 * items are ORDERED by their scores narrowed to float: two doubles that differ below float precision are a tie, to
 * which mms_set_rank_tie_mode applies as it does to float ties.  Labels and groups are int(x).  The folds
 * (ap += ++rank / (Dtype)(i + 1), map += ap / rank, mrr += 1.0 / (rank + 1), AUC's sum of integers, the final
 * divisions) run in double: the bits of the reference's double instantiation.  workspace:
 * mms_rank_workspace_bytes_f64(n). */
size_t mms_rank_workspace_bytes_f64(int n);
int mms_rank_map_mrr_f64(int n, int fixed_axis, const double* prob, const double* label,
                         const double* group, double* map_out, double* mrr_out,
                         int* effective_out, void* workspace, size_t workspace_bytes,
                         void* stream);
int mms_rank_auc_f64(int n, int dim, int fixed_axis, const double* prob, const double* label,
                     int has_ignore_label, int ignore_label, double* auc_out,
                     void* workspace, size_t workspace_bytes, void* stream);
int mms_rank_auc_nd_f64(int outer, int channels, int inner, int fixed_axis, const double* prob,
                        const double* label, int has_ignore_label, int ignore_label, double* auc_out,
                        void* workspace, size_t workspace_bytes, void* stream);
int mms_rank_accuracy_f64(int count, const double* a, const double* b, const double* label,
                          double* acc_out, void* workspace, size_t workspace_bytes,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MMS_H_ */
