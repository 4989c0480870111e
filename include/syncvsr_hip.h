/* libsyncvsr_hip.so — C ABI of the MI355X (gfx950) SyncVSR training hot path.
 *
 * The reference (KAIST-AILab/SyncVSR) has no native/FFI layer: its hot path is reached through torch.nn modules
 * (SURVEY.md §8b).  Each entry point below therefore names the reference *module call* it replaces.
 *
 * Conventions (all entry points):
 *   - arguments are raw device pointers + explicit sizes; `void*` activations are bf16 unless stated; parameters,
 *     statistics and gradients are fp32.  The caller owns every buffer, including workspaces.
 *   - asynchronous: work is enqueued on `stream`; the call returns 0, SVSR_ERR_ARG (1001) for an unsupported
 *     shape/argument, or a hipError_t value if the launch failed.  Nothing throws; the only global mutable state is the
 *     table of result-preserving tuning knobs behind svsr_tune() (the library never reads the environment).
 *   - activations are NHWC ("pixels x channels"); a frame index is just the leading pixel index.
 *   - REPRODUCIBLE: no kernel accumulates floating-point values with atomics.  Grid-wide sums (BatchNorm statistics, split-K
 *     weight gradients, bias / LayerNorm gradients, losses, the gradient norm) are written as one partial row per workgroup
 *     into a caller-owned workspace and added in a fixed order by a second small launch (svsr_colsum_rows or a specialised
 *     finaliser), so two identical calls give bit-identical results.  Entry points named *_rows / *_plan are HOST-side
 *     queries (no launch) that tell the caller how large such a workspace must be for a shape.
 *
 * The declarations are kept one per statement in a regular form because syncvsr_amd/_lib.py derives its ctypes
 * signatures from this file.
 */
#ifndef SYNCVSR_HIP_H
#define SYNCVSR_HIP_H

#include <stdint.h>

#ifndef __HIP_PLATFORM_AMD__
typedef void* hipStream_t;
#else
#include <hip/hip_runtime_api.h>
#endif

#define SVSR_OK 0
#define SVSR_ERR_ARG 1001
/* Store / add mode of the entry points that write a parameter gradient (the *_v2 forms; the older symbols add to both destinations).
 * A set bit: the destination is loaded and added to.  A clear bit: the launch is the FIRST writer of that range in this step and stores
 * 0.f + sum without loading the destination — bit for bit what the add onto a zero-filled buffer left (-0 becomes +0), without the fill
 * and without the read.  Every element of a destination is written in either mode. */
#define SVSR_GRAD_ADD_DW 1
#define SVSR_GRAD_ADD_DB 2
/* step-list groups (svsr_steplist_push_group): a group is open where none may be (a nested group, a break or a copy inside a group) */
#define SVSR_ERR_GROUP_OPEN 1003
/* step-list groups: a group index the list does not have (a copy naming it, closing with no group open) */
#define SVSR_ERR_NO_GROUP 1004
/* step-list groups: a skip mask whose length is not the list's group count */
#define SVSR_ERR_MASK_SIZE 1005

/* one problem of svsr_igemm_wgrad_group: the arguments of a svsr_igemm_wgrad call (device pointers; meta = the HOST meta[8] of the plan) */
typedef struct svsr_wgrad_problem {
    const void* x; const void* dy; float* dw; float* dbias; const int* plan_dev; const int* meta;
    int Nimg; int in_pix; int Ci; int in_pitch; int Co; int out_pix; int out_pitch; int wt_taps;
} svsr_wgrad_problem;

/* one encoder layer of svsr_enc_fwd: DEVICE pointers.  Weights: the bf16 shadows [out][in] of query|key|value (adjacent: [1536][512]),
 * attention.output.dense [512][512], intermediate.dense [2048][512], output.dense [512][2048]; biases and LayerNorm parameters fp32.
 * Written by the launch (what the backward reads): qkv bf16 [R][1536], probs bf16 [B*8][S][ldp = ceil8(S)], ctx / ao / x1 / f / xout bf16
 * [R][512], z / hg bf16 [R][2048], LayerNorm statistics m1 r1 m2 r2 fp32 [R].  site_*: dropout sites of the attention probabilities,
 * BertSelfOutput's and BertOutput's dropout. */
typedef struct svsr_enc_layer {
    const void* wqkv; const void* wo; const void* w1; const void* w2;
    const float* bqkv; const float* bo; const float* b1; const float* b2; const float* g1; const float* be1; const float* g2; const float* be2;
    void* qkv; void* probs; void* ctx; void* ao; void* x1; void* z; void* hg; void* f; void* xout;
    float* m1; float* r1; float* m2; float* r2;
    unsigned site_probs; unsigned site_ao; unsigned site_fo; unsigned pad_;
} svsr_enc_layer;

/* one encoder layer of svsr_enc_bwd (the backward of svsr_enc_fwd: autograd of HF BertLayer, reference LRW/video/src/lightning.py:92,152-156):
 * DEVICE pointers.  Weights: the TRANSPOSED bf16 shadows [in][out] the data-gradient launches read — output.dense [2048][512],
 * intermediate.dense [512][2048], attention.output.dense [512][512], query|key|value [512][1536]; g1 / g2: LayerNorm weights.  Read: what
 * the forward kept (f, x1, ao, the layer input xin, z, qkv, probs, LayerNorm statistics).  Written: see svsr_enc_bwd. */
typedef struct svsr_enc_bwd_layer {
    const void* w2t; const void* w1t; const void* wot; const void* wqkvt;
    const float* g1; const float* g2;
    const void* f; const void* x1; const void* ao; const void* xin; const void* z; const void* qkv; const void* probs;
    const float* m1; const float* r1; const float* m2; const float* r2;
    void* ds2; void* df; void* dz; void* dx1; void* ds1; void* dao; void* dqkv; void* dx;
    float* part1; float* part2;
    unsigned site_probs; unsigned site_ao; unsigned site_fo; unsigned pad_;
} svsr_enc_bwd_layer;

#ifdef __cplusplus
extern "C" {
#endif

/* ---- plumbing (runtime.hip) ------------------------------------------------------------------------------------
 * svsr_tune: sets a result-preserving tuning knob ("igemm_tile", "igemm_m128", "wg_blocks", "w3_blocks", "ln_rpb",
 * "igemm_bn64_below", "wg_short_k", "igemm_ksplit", "igemm_lin_bn64", "p8", "p8_grid", "p8_min_items", "p8_stagger", "wg_imgmajor",
 * "wg_units", "wg_unit_max", "wg_unit_min", "igemm_ksplit128", "w3_waves", "reduce_cus", "w3_dense": tile shapes, split counts, kernel-variant switches — documented at the table in
 * runtime.hip; never read from the environment); unknown key -> SVSR_ERR_ARG.  svsr_tune_value reads a knob back.  The knobs that decide
 * the ORDER in which a weight gradient's or a BatchNorm statistic's partial sums are added (reduce_cus — the compute-unit count the splits
 * are planned for: a fixed 256, not the device's —, wg_blocks, wg_units, wg_unit_max, wg_unit_min, wg_short_k, w3_blocks, w3_waves, w3_dense) are what a
 * bit-identical resume depends on: engine.TrainStep.state_dict() records them, load_state_dict() warns when they differ.
 * svsr_colsum_rows: out[c] (+)= scale * sum_{r<nrows} ws[r*ld + c], rows added in a fixed order; columns [0,n0) go to out0,
 * [n0,n0+n1) to out1 (may be null when n1 = 0); accumulate != 0 adds to the existing values. */
int svsr_tune(const char* key, int value);
int svsr_tune_value(const char* key, int* value);
int svsr_colsum_rows(const float* ws, int nrows, int64_t ld, float* out0, int64_t n0, float* out1, int64_t n1, int accumulate, float scale, hipStream_t stream);
/* (accumulate: 0 stores, 1 adds to both outputs; 4 | SVSR_GRAD_ADD_* bits (bit 0: out0, bit 1: out1) adds where the bit is set and stores
 * 0.f + sum elsewhere — the split-K tail of svsr_igemm_wgrad_v2) */
/* up to any number of svsr_colsum_rows problems, 16 per launch (the postponed parameter-gradient reductions of a layer's backward: LayerNorm
 * weight / bias, linear biases — autograd's accumulation into .grad of lightning.py's modules).  entries: n records of 64 bytes in HOST memory,
 * {const float* ws; float* out0; float* out1; int64_t ld, n0, n1; int32_t nrows, accumulate; float scale; int32_t reserved}; the outputs of
 * different records must not overlap.  Same additions in the same order as n separate calls. */
int svsr_colsum_rows_multi(const void* entries, int n, hipStream_t stream);

/* ---- implicit-GEMM contractions (igemm_fwd.hip) -------------------------------------------------------------------
 * svsr_igemm_fwd replaces: nn.Conv2d forward of resnet.layer{1..4} (reference LRW/video/src/tcn/models/resnet.py:8-16,
 *   59-72 / timm resnet18 via lightning.py:55,114-117), their input-gradient (autograd), and every nn.Linear forward /
 *   input-gradient of the BERT encoder and heads (lightning.py:92,107,82,161,168).
 * The rows of the contraction come from a PLAN built on the host once per shape (svsr_conv_plan / svsr_rows_plan) and kept
 *   on the device: output positions are grouped into classes that share the same set of in-grid taps, so the kernel never
 *   multiplies by a convolution's zero padding and a stride-2 input-gradient (four output-parity classes) is one launch.
 *   svsr_*_plan(words = null) returns the number of int32 words; a second call fills `words` (host) and meta[8] =
 *   {bm, bn, ns, tiles, grid_y, classes, max taps, rows}: the kernel instantiation k_igemm_fwd_glds<bm,bn,ns> the launch will
 *   use and `tiles` = rows of BatchNorm partials it writes.  Negative return = -SVSR_ERR_ARG.
 *   svsr_conv_plan: k x k / stride / pad convolution over Nimg images whose FORWARD input is H x W; mode 0 forward
 *   (in = x [H][W] -> out = y [Ho][Wo], wt [Co][k*k][Ci]), mode 1 input-gradient (in = dy [Ho][Wo] -> out = dx [H][W], wt =
 *   transposed weights [Ci][k*k][Co]; pixels no tap reaches are written as 0 (+ bias / addend)), mode 2 the same for an
 *   in-place accumulation (addend aliases out): pixels no tap reaches are left alone; mode 3 (3x3 / stride 2 / pad 1 only) mode 1 with
 *   the 1x1 / stride 2 input-gradient of the same input folded in as one more tap of the (even, even) pixels (svsr_igemm_dgrad2).
 *   svsr_rows_plan: dense layer over Nimg sequences, row (n, j < P) reads source row n*in_pix + src0 + j and writes target row
 *   n*out_pix + dst0 + j (plain linear: P = 1, in_pix = out_pix = 1).
 * svsr_igemm_fwd(plan_dev = device copy of the words, meta = the host meta): in [Nimg][in_pix] pixels of pitch in_pitch with
 *   Ci channels per tap, out [Nimg][out_pix] pixels of pitch out_pitch with Co channels; wt bf16 [Co][wt_taps][Ci].
 *   Optional epilogues: +bias, +addend (bf16 pixels laid out like `out`: residual-gradient merge; may alias `out`),
 *   out = alpha * dropout(act(acc + bias)) + addend with act 0 none / 1 exact GELU (pre-activation saved to out_pre) / 2 ReLU
 *   (LRS PositionwiseFeedForward, transformer/positionwise_feed_forward.py:28-30; alpha carries the Conformer's 0.5 macaron
 *   scale and the sqrt(d) embedding scale, encoder_layer.py:97,131, embedding.py:208); dropout(p) with the keep decision
 *   hash(*drop_seed, drop_site, output element index) (drop_seed null or p = 0: off; see svsr_scale_bf16), fp32 output,
 *   per-channel BatchNorm partial sums stats[tiles][2][Co] (plain stores; reduced by svsr_bn_finalize). */
int svsr_conv_plan(int mode, int Nimg, int H, int W, int Co_out, int k, int stride, int pad, int* words, int cap_words, int* meta);
int svsr_rows_plan(int Nimg, int P, int src0, int dst0, int Co_out, int* words, int cap_words, int* meta);
int svsr_igemm_fwd_kgroups(const int* meta, int Ci, int Co, int bn_epilogue);   /* host query: 2 when the launch splits K over two wave groups (k_igemm_fwd_glds<64,64,4,2>) */
int svsr_igemm_fwd(const void* in, const void* wt, void* out, void* out_pre, const float* bias, const void* addend, float* stats, const int* plan_dev, const int* meta, int Nimg, int in_pix, int Ci, int in_pitch, int Co, int out_pix, int out_pitch, int wt_taps, int act, int out_f32, float alpha, const unsigned* drop_seed, unsigned drop_site, float drop_p, hipStream_t stream);

/* svsr_igemm_wgrad replaces: the weight-gradient of the same Conv2d / Linear layers (torch autograd).
 * dw fp32 [Co][wt_taps][Ci] is ACCUMULATED (dw += ...).  x = forward input pixels [Nimg][in_pix] (pitch in_pitch, Ci channels),
 * dyp = output-gradient pixels [Nimg][out_pix] (pitch out_pitch, Co channels).  dbias (optional, fp32 [Co]) += column sums of
 * dyp = the bias gradient of an nn.Linear, from the tiles the kernel stages anyway (one MFMA against a fragment of ones).
 * Rows come from a host-built plan, per tap the (source pixel, target pixel) pairs whose source lies inside the grid (no products
 * with the zero padding): svsr_wgrad_plan for a k x k / stride / pad convolution of Nimg images [H][W], svsr_wgrad_rows_plan for
 * a dense layer over Nimg sequences (row (n, j < P): source row n*in_pix + src0 + j, target row n*out_pix + dst0 + j).  Both
 * return the number of int32 words (words = null: count only; negative = error), meta[8] = {tile edge, ring depth, K splits,
 * chunks per split, tasks, taps, max positions per tap} and *part_floats = the workspace svsr_igemm_wgrad needs for its split-K
 * slabs (any contents; added into dw / dbias in a fixed order; 0 when a single split writes dw directly). */
int svsr_wgrad_plan(int Nimg, int H, int W, int Ci, int Co, int k, int stride, int pad, int* words, int cap_words, int* meta, int64_t* part_floats);
int svsr_wgrad_rows_plan(int Nimg, int P, int src0, int dst0, int Ci, int Co, int has_bias, int* words, int cap_words, int* meta, int64_t* part_floats);
int svsr_igemm_wgrad(const void* x, const void* dyp, float* dw, float* dbias, const int* plan_dev, const int* meta, int Nimg, int in_pix, int Ci, int in_pitch, int Co, int out_pix, int out_pitch, int wt_taps, float* part, int64_t part_floats, hipStream_t stream);
/* svsr_wgrad_rows_plan_tile: svsr_wgrad_rows_plan with the tile edge given (bc = 64 or 128; anything else is -SVSR_ERR_ARG) and no K split:
 * meta = {bc, ring depth (3 / 2), 1, all chunks, tasks, 1, P, 0}, *part_floats = 0.  For the problems of a grouped launch, which fills the
 * chip with many problems at once and so needs neither the narrow tile nor the split that svsr_wgrad_rows_plan picks for one problem alone. */
int svsr_wgrad_rows_plan_tile(int Nimg, int P, int src0, int dst0, int Ci, int Co, int has_bias, int bc, int* words, int cap_words, int* meta, int64_t* part_floats);
/* svsr_igemm_wgrad_group: n independent svsr_igemm_wgrad problems in ONE launch — the weight gradients of the encoder's and the heads'
 * nn.Linear layers (reference lightning.py:82,92,107: 26 short contractions of a backward pass; as launches of their own each is 7-17 us
 * of latency for ~1 us of work).  Every problem must carry a plain plan without K split, and all problems of a launch the same tile:
 * meta[0..2] = {64, 3, 1} or {128, 2, 1} (svsr_wgrad_rows_plan_tile); anything else — a mix of the two, a split or unit-list plan, n < 1,
 * n > 256 — returns SVSR_ERR_ARG before anything is launched.  table_dev: caller-owned device buffer of >= svsr_igemm_wgrad_group_bytes(n) bytes.  Results are identical
 * to n separate svsr_igemm_wgrad calls (same workgroup code, one writer per element). */
int64_t svsr_igemm_wgrad_group_bytes(int n);
int svsr_igemm_wgrad_group(const svsr_wgrad_problem* problems, int n, void* table_dev, int64_t table_bytes, hipStream_t stream);
/* the two above with the store / add mode of dw and dbias (SVSR_GRAD_ADD_DW | SVSR_GRAD_ADD_DB; the group: one HOST int per problem, null = all add) */
int svsr_igemm_wgrad_v2(const void* x, const void* dyp, float* dw, float* dbias, const int* plan_dev, const int* meta, int Nimg, int in_pix, int Ci, int in_pitch, int Co, int out_pix, int out_pitch, int wt_taps, float* part, int64_t part_floats, int mode, hipStream_t stream);
int svsr_igemm_wgrad_group_v2(const svsr_wgrad_problem* problems, const int* modes, int n, void* table_dev, int64_t table_bytes, hipStream_t stream);

/* svsr_conv3x3_c64: conv3x3(64, 64), stride 1, pad 1 (layer1 of the trunk, resnet.py:8-10,36,53) forward and, with the
 * transposed weights and mirrored taps, its input-gradient; persistent workgroups, weights resident in LDS
 * (conv3x3_c64.hip).  in/out/addend bf16 [Nimg][H][W][64]; wt bf16 [64][9][64]; tap t reads pixel (y+dy[t], x+dx[t]) with
 * weight tap tw[t] (HOST arrays of 9 ints); out = conv (+ addend); stats [rows][2][64] with rows =
 * svsr_conv3x3_c64_stat_rows(Nimg, H, W) (one per persistent workgroup).  Requires W <= 29. */
int svsr_conv3x3_c64_stat_rows(int Nimg, int H, int W);
/* pixtab (both launches below): device copy of svsr_conv3x3_c64_pixtab's table for (Nimg, H, W) — pixel index or -1 per padded
 * coordinate — or null (the kernel then derives the source pixel of every staged row by arithmetic: ~500 instructions per chunk and thread).
 * svsr_conv3x3_c64_pixtab(..., out = null) returns the entry count. */
int64_t svsr_conv3x3_c64_pixtab(int Nimg, int H, int W, int* out, int64_t cap);
int svsr_conv3x3_c64(const void* in, const void* wt, void* out, const void* addend, float* stats, int Nimg, int H, int W, const int* dy, const int* dx, const int* tw, const int* pixtab, hipStream_t stream);

/* Data-gradient launches with the FIRST PASS OF THE BATCHNORM BACKWARD in their epilogue (replaces the separate reduce pass of
 * svsr_bn_act_bwd for the ReLU trunk; reference backward of tcn/models/resnet.py:59-72 = autograd of bn -> relu).  The launch computes
 * dL/dy (+ addend, which may alias out) for a tensor y = relu(bn(x) [+ residual]) that has the geometry of `out`, and while the tile
 * is in registers stores g = (y > 0 ? dL/dy : 0) INSTEAD of dL/dy and writes, per row tile / persistent workgroup, the column sums
 * of g and of g * (x - mean) * rstd into stats[rows][2][Co] (rows = meta[3] of the plan, resp. svsr_conv3x3_c64_stat_rows).
 * y == NULL (allowed only when y has no residual branch): the mask is recomputed from x as bn(x) > 0 with gamma / beta in the forward
 * pass's own arithmetic (svsr_bn_act_fwd) and y is not read; otherwise gamma / beta may be NULL.
 * act = 1: ReLU as described.  act = 2: Swish (LRS trunk, Conformer convolution module): g = dL/dy * swish'(bn(x) + r), where `y` is the
 * residual INPUT r of the output (NULL: none) and gamma / beta are required.
 * svsr_igemm_dgrad_bn needs a plan that visits every target pixel once (svsr_conv_plan mode 1), Co % 8 == 0, out_pitch % 8 == 0.
 * svsr_bn_bwd_from_stats then adds the rows in a fixed order (dgamma +=, dbeta +=, coef[3][C] scratch) and writes
 * dx = gamma * rstd * (g - mean(g) - xhat * mean(g * xhat)). */
int svsr_igemm_dgrad_bn(const void* in, const void* wt, void* out, const void* addend, float* stats, const int* plan_dev, const int* meta, int Nimg, int in_pix, int Ci, int in_pitch, int Co, int out_pix, int out_pitch, int wt_taps, const void* y, const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta, int act, hipStream_t stream);
/* The same epilogue for a linear layer / convolution whose INPUT was y = dropout(relu(z)) (positionwise_feed_forward.py:28-30): stores
 * dz = (y > 0 ? gscale * dL/dy : 0) (gscale = 1 / (1 - p): y is zero where ReLU or the dropout mask cut) and writes the column sums of dz per row tile
 * into the first half of stats[meta[3]][2][Co] — the partial rows of the bias gradient of the layer in front (svsr_colsum_rows adds them).
 * zeros / ones: device vectors of Co floats holding 0 / 1.  4-wave plans only (not the persistent 3x3 kernel). */
int svsr_igemm_dgrad_relu(const void* in, const void* wt, void* out, float* stats, const int* plan_dev, const int* meta, int Nimg, int in_pix, int Ci, int in_pitch, int Co, int out_pix, int out_pitch, int wt_taps, const void* y, const float* zeros, const float* ones, float gscale, hipStream_t stream);
/* The input gradient of a downsample block (reference tcn/models/resnet.py:36-53,59-72: conv1 3x3 / stride 2 and downsample 1x1 / stride 2
 * read the same input) in ONE launch: plan = svsr_conv_plan mode 3 (3x3 / stride 2 / pad 1 only), whose (even, even) pixels carry one more tap read
 * from the second operand pair: in2 = the 1x1 branch's dy (geometry and pitch of `in`), wt2 = its transposed weight [Co][Ci].  Both branches
 * meet in the fp32 accumulator and are rounded once.  Other arguments: svsr_igemm_fwd / svsr_igemm_dgrad_bn without the addend. */
int svsr_igemm_dgrad2(const void* in, const void* wt, const void* in2, const void* wt2, void* out, void* out_pre, const float* bias, float* stats, const int* plan_dev, const int* meta, int Nimg, int in_pix, int Ci, int in_pitch, int Co, int out_pix, int out_pitch, int wt_taps, int act, int out_f32, float alpha, const unsigned* drop_seed, unsigned drop_site, float drop_p, hipStream_t stream);
int svsr_igemm_dgrad2_bn(const void* in, const void* wt, const void* in2, const void* wt2, void* out, float* stats, const int* plan_dev, const int* meta, int Nimg, int in_pix, int Ci, int in_pitch, int Co, int out_pix, int out_pitch, int wt_taps, const void* y, const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta, int act, hipStream_t stream);
int svsr_conv3x3_c64_dgrad_bn(const void* in, const void* wt, void* out, const void* addend, float* stats, int Nimg, int H, int W, const int* dy, const int* dx, const int* tw, const void* y, const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta, int act, const int* pixtab, hipStream_t stream);
int svsr_bn_bwd_from_stats(const void* g, const void* x, const float* mean, const float* rstd, const float* gamma, const float* stats, int nrows, float* coef, float* dgamma, float* dbeta, void* dx, int64_t npix, int C, hipStream_t stream);
/* The same for bn2 of a downsample block (resnet.py:36-53,69-72: out += downsample(x)), where g is the gradient of the 1x1 branch's BatchNorm
 * output too: the apply pass reads that BatchNorm's input xd along and writes the first pass of ITS backward, the column sums of g and of
 * g * (xd - mean_d) * rstd_d, into rows_d[svsr_bn_act_bwd_rows(npix, C)][2][C] — bit for bit the rows svsr_bn_act_bwd(g, NULL, xd, ..., act 0)
 * forms.  svsr_bn_bwd_from_stats(g, xd, mean_d, rstd_d, gamma_d, rows_d, svsr_bn_act_bwd_rows(npix, C), ...) then finishes that branch.
 * dx as svsr_bn_bwd_from_stats writes it.  rows_d may reuse the memory of `stats`.  Null pointers: SVSR_ERR_ARG. */
int svsr_bn_bwd_from_stats_ds(const void* g, const void* x, const float* mean, const float* rstd, const float* gamma, const float* stats, int nrows, float* coef, float* dgamma, float* dbeta, void* dx, const void* xd, const float* mean_d, const float* rstd_d, float* rows_d, int64_t npix, int C, hipStream_t stream);


/* svsr_conv3x3_wgrad: weight gradient of a 3x3 / stride-1 / pad-1 Conv2d (resnet.py:8-10) with all nine taps sharing one
 * pass over x [Nimg][H][W][Ci] and dy [Nimg][H][W][Co] (zero-padded coordinates, wgrad3x3.hip).  dw fp32 [Co][9][Ci] is
 * ACCUMULATED; split-K slabs go through `part` (size from svsr_conv3x3_wgrad_plan) and are added in a fixed order.
 * Requires Ci, Co multiples of 64 and W <= 29; other shapes go through svsr_igemm_wgrad. */
int svsr_conv3x3_wgrad_plan(int Nimg, int H, int W, int Ci, int Co, int* splits, int64_t* part_floats);
int svsr_conv3x3_wgrad(const void* x, const void* dy, float* dw, int Nimg, int H, int W, int Ci, int Co, float* part, int64_t part_floats, hipStream_t stream);
/* the same with the store / add mode of dw (0 or SVSR_GRAD_ADD_DW) */
int svsr_conv3x3_wgrad_v2(const void* x, const void* dy, float* dw, int Nimg, int H, int W, int Ci, int Co, float* part, int64_t part_floats, int mode, hipStream_t stream);
/* The chained form.  defer != 0: the launch leaves its split-K slabs in `part` un-added (nothing is deferred where the plan has one split: dw
 * is written directly); the caller hands them on as the PENDING slabs of a later svsr_conv3x3_wgrad_chain on the same stream, or to
 * svsr_conv3x3_wgrad_reduce.  pend_part != NULL: pend_splits (>= 2, from svsr_conv3x3_wgrad_plan of that convolution) slabs per 64 x 64
 * tile of an earlier deferred launch — any geometry, pend_Ci / pend_Co its channel counts — which this launch's workgroups add into
 * pend_dw (pend_mode: that convolution's store / add mode) before their own work, in the order of the stand-alone reduce: the same bits.
 * Stream order is the only synchronisation, so the pending slabs must not overlap the range [part, part + part_floats needed) this launch
 * writes: SVSR_ERR_ARG, nothing launched (keep two slab sets and alternate).  pend_part == NULL and defer == 0: svsr_conv3x3_wgrad_v2. */
int svsr_conv3x3_wgrad_chain(const void* x, const void* dy, float* dw, int Nimg, int H, int W, int Ci, int Co, float* part, int64_t part_floats, int mode, int defer, const float* pend_part, float* pend_dw, int pend_splits, int pend_Ci, int pend_Co, int pend_mode, hipStream_t stream);
int svsr_conv3x3_wgrad_reduce(const float* part, float* dw, int splits, int Ci, int Co, int mode, hipStream_t stream);

/* ---- 3-D stem (stem.hip) --------------------------------------------------------------------------------------
 * svsr_stem_conv_fwd replaces stem3d[0] = nn.Conv3d(1,64,(5,7,7),(1,2,2),(2,3,3),bias=False) (lightning.py:50).
 * vid fp32 [B][1][T][H][W]; w fp32 [64][1][5][7][7]; out bf16 [B*T][H/2][W/2][64]; stats [rows][2][64] with rows =
 * svsr_stem_conv_fwd_stat_rows(B, T, H, W).  H and W even and >= 8.  ws: svsr_stem_conv_fwd_ws_bytes(B, T, H, W) bytes (non-zero where
 * W % 8 == 0) for the DMA-fed kernel; NULL or too small: the direct kernel, at any even W.  A shape whose tile does not fit the LDS of
 * the kernel chosen (W >= 1394 direct, W >= 1392 DMA-fed) returns SVSR_ERR_ARG before anything is launched. */
int svsr_stem_conv_fwd_stat_rows(int B, int T, int H, int W);
int64_t svsr_stem_conv_fwd_ws_bytes(int B, int T, int H, int W);
int svsr_stem_conv_fwd(const float* vid, const float* w, void* out, float* stats, int B, int T, int H, int W, void* ws, int64_t ws_bytes, hipStream_t stream);

/* weight gradient of the stem conv (autograd of lightning.py:50); dw fp32 [64][245] accumulated (per-workgroup slabs in
 * `part`, size from svsr_stem_conv_wgrad_plan, added in a fixed order). */
int svsr_stem_conv_wgrad_plan(int B, int T, int H, int W, int* splits, int64_t* part_floats);
int svsr_stem_conv_wgrad(const float* vid, const void* dy, float* dw, int B, int T, int H, int W, int use_tr, float* part, int64_t part_floats, hipStream_t stream);

/* The apply pass of svsr_stem_bn_act_pool_bwd and svsr_stem_conv_wgrad as ONE pass (autograd of lightning.py:49-54's stem3d[1..3] into
 * stem3d[0].weight): the gradient of the convolution output is made tile by tile in LDS and contracted at once, never written.  Call
 * svsr_stem_bn_act_pool_bwd first with dx = NULL and xwin / gpool given (it then runs its reduce pass and the finalisation only and
 * leaves gpool and coef); x = the convolution output, amax / mean / rstd as there.  dw bit-identical to the two-launch form.
 * svsr_stem_bwd_wgrad_ok: 1 when the shape is covered (W % 4 == 0 and W <= 96; else use the two launches). */
int svsr_stem_bwd_wgrad_ok(int B, int T, int H, int W);
int svsr_stem_bwd_wgrad(const float* vid, const void* gpool, const void* amax, const void* x, const float* mean, const float* rstd, const float* coef, float* dw, int B, int T, int H, int W, float* part, int64_t part_floats, hipStream_t stream);

/* ---- BatchNorm / activation / pooling passes (norm_act.hip) ---------------------------------------------------
 * svsr_bn_finalize: train-mode statistics of nn.BatchNorm2d/3d (lightning.py:51; resnet.py:37,54,14): adds the nrows
 * partial rows part[nrows][2][C] written by the producing convolution in a fixed order (double accumulation), writes
 * mean/rstd, updates running_mean/var (momentum, unbiased var) and num_batches_tracked. */
int svsr_bn_finalize(const float* part, int nrows, int C, float count, float eps, float momentum, float* mean, float* rstd, float* running_mean, float* running_var, int64_t* num_batches_tracked, hipStream_t stream);

/* eval-mode statistics: mean = running_mean, rstd = rsqrt(running_var + eps). */
int svsr_bn_eval_prepare(const float* running_mean, const float* running_var, int C, float eps, float* mean, float* rstd, hipStream_t stream);

/* y = act(gamma*(x-mean)*rstd + beta [+ res]); act 0 none, 1 ReLU, 2 Swish (LRS backbones/modules/resnet.py:90-107,
 * transformer/convolution.py:69); any C % 8 == 0 up to 2048.  Replaces bn1/relu1, bn2/+residual/relu2 and the
 * downsample BatchNorm of BasicBlock.forward (resnet.py:59-72). */
int svsr_bn_act_fwd(const void* x, const void* res, void* y, const float* mean, const float* rstd, const float* gamma, const float* beta, int64_t npix, int C, int act, hipStream_t stream);
/* The block-end pass of a downsample block in the ReLU trunk (resnet.py:65-72), both BatchNorms in one launch:
 * y = relu(bn(x) + bf16(bn_d(xd))), the downsample term rounded to bf16 as the stored tensor was — the bits of
 * svsr_bn_act_fwd(x, res = svsr_bn_act_fwd(xd, NULL, act 0), act 1) without writing that tensor.  Null x / xd / y: SVSR_ERR_ARG. */
int svsr_bn_act_fwd2(const void* x, const void* xd, void* y, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* mean_d, const float* rstd_d, const float* gamma_d, const float* beta_d, int64_t npix, int C, hipStream_t stream);

/* backward of the above: dgamma/dbeta accumulated; dx (grad of the conv output) and optional dres (= masked dy).
 * slots: workspace of svsr_bn_act_bwd_rows(npix, C) rows of [2][C] floats (any contents); coef [3][C] scratch.  Swish recomputes its
 * pre-activation and therefore needs beta and the forward's residual input `res` (null if there was none). */
int svsr_bn_act_bwd_rows(int64_t npix, int C);
int svsr_bn_act_bwd(const void* dy, const void* y, const void* x, const float* mean, const float* rstd, const float* gamma, float* slots, float* coef, float* dgamma, float* dbeta, void* dx, void* dres, int64_t npix, int C, int act, const float* beta, const void* res, hipStream_t stream);

/* stem3d[1..3]: BatchNorm3d -> activation -> MaxPool3d((1,3,3),(1,2,2),(0,1,1)) fused; act 1 = exact nn.GELU()
 * (LRW lightning.py:51-53), act 2 = Swish (LRS backbones/conv3d_extractor.py:30-36).
 * x [N][Hc][Wc][C] -> y [N][Hp][Wp][C], amax uint8 [N][Hp][Wp][C] = window-local argmax (first max wins).
 * Hp = (Hc - 1) / 2 + 1 and Wp = (Wc - 1) / 2 + 1: anything else is SVSR_ERR_ARG, in the forward and in every form of the backward. */
int svsr_stem_bn_act_pool_fwd(const void* x, void* y, void* amax, const float* mean, const float* rstd, const float* gamma, const float* beta, int N, int Hc, int Wc, int Hp, int Wp, int C, int act, void* xwin, hipStream_t stream);

/* backward of the fused stem pass: dx = gradient of the stem conv output; slots: workspace of
 * svsr_stem_bn_act_pool_bwd_rows(N, Hc, Wc, C) rows of [2][C] floats. */
int svsr_stem_bn_act_pool_bwd_rows(int N, int Hc, int Wc, int C);
/* xwin (forward: optional output, backward: optional input), gpool (backward: optional workspace), both bf16 [N][Hp][Wp][C] like y:
 * the convolution output at every window's arg-max, kept by the forward so that the backward's reduce pass streams pooled-size tensors
 * (one activation derivative per pooled output, g = dpool * act' written to gpool) instead of gathering from the 4x larger
 * convolution output, and its apply pass evaluates no activation derivative at all.  Null: the gather form. */
int svsr_stem_bn_act_pool_bwd(const void* dpool, const void* amax, const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta, float* slots, float* coef, float* dgamma, float* dbeta, void* dx, int N, int Hc, int Wc, int Hp, int Wp, int C, int act, const void* xwin, void* gpool, hipStream_t stream);

/* hidden.mean((2,3)) (lightning.py:118) and its backward: [N][HW][C] <-> [N][C]. */
int svsr_avgpool_fwd(const void* x, void* y, int64_t N, int HW, int C, hipStream_t stream);
int svsr_avgpool_bwd(const void* dy, void* dx, int64_t N, int HW, int C, hipStream_t stream);

/* ---- transformer encoder passes (bert.hip) --------------------------------------------------------------------
 * y = LayerNorm(a + r) (BertSelfOutput / BertOutput, reached from lightning.py:152-156; LRS transformer/layer_norm.py);
 * r may be null; any D % 8 == 0 up to 2048.  The backward returns ds = dLN/d(a+r) (+ addend: the skip-path gradient of a
 * pre-LN residual block, encoder_layer.py:93-137); dgamma/dbeta are accumulated from per-workgroup partial rows in `part`
 * (svsr_add_ln_bwd_rows(R) rows of [2][D] floats). */
int svsr_add_ln_fwd(const void* a, const void* r, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int R, int D, float eps, hipStream_t stream);
int svsr_add_ln_bwd_rows(int R);
int svsr_add_ln_bwd(const void* dy, const void* a, const void* r, const float* gamma, const float* mean, const float* rstd, void* ds, float* dgamma, float* dbeta, int R, int D, const void* addend, float* part, hipStream_t stream);
/* svsr_add_ln_bwd / svsr_bias_act_bwd WITHOUT their fixed-order reduction: the partial rows stay in `part` (a buffer of the caller's that must live until
 * it has added them with svsr_colsum_rows on a stream of its choice — parameter-gradient sums the backward chain never waits for) */
int svsr_add_ln_bwd_partials(const void* dy, const void* a, const void* r, const float* gamma, const float* mean, const float* rstd, void* ds, int R, int D, const void* addend, float* part, hipStream_t stream);
/* svsr_add_ln_bwd_partials with a second output for the residual branch that ends in this sum (x' = x + alpha * dropout(branch), the LRS
 * encoder / decoder layers, encoder_layer.py:93-150): ds2 = alpha2 * mask / (1 - p) * ds, computed from the bf16-rounded ds with the element
 * indices svsr_scale_bf16 uses, i.e. bit for bit what svsr_scale_bf16(ds) would write (ds2 null: exactly svsr_add_ln_bwd_partials) */
int svsr_add_ln_bwd_branch(const void* dy, const void* a, const void* r, const float* gamma, const float* mean, const float* rstd, void* ds, int R, int D, const void* addend, float* part, void* ds2, float alpha2, const unsigned* drop_seed, unsigned drop_site, float drop_p, hipStream_t stream);
int svsr_bias_act_bwd_partials(const void* dy, const void* z, void* dz, float* db, int R, int N, int n_valid, int ld, int act, float gscale, float* part, hipStream_t stream);

/* BertEmbeddings on inputs_embeds = emb_dropout(cat(cls_token, feats)) (lightning.py:149-156):
 * y = dropout_out(LN(dropout_in(e) + pos[s] + type[0])); dropout_in = the module's emb_dropout (site_in, p_in), dropout_out =
 * BertEmbeddings' hidden dropout (site_out, p_out); both off when drop_seed is null or p = 0 (mask semantics: svsr_scale_bf16,
 * element index = position in the [B*S][D] tensor).  feats bf16 [B][S-1][D]; sum_out bf16 [B*S][D] keeps the pre-norm sum for the
 * backward.  svsr_embed_bwd_scatter takes ds = gradient of that sum and regenerates the dropout_in mask for dfeats / dcls
 * (part: [S][D] float workspace). */
int svsr_embed_ln_fwd(const void* feats, const float* cls, const float* pos, const float* type0, const float* gamma, const float* beta, void* sum_out, void* y, float* mean, float* rstd, int B, int S, int D, float eps, const unsigned* drop_seed, unsigned site_in, float p_in, unsigned site_out, float p_out, hipStream_t stream);
int svsr_embed_bwd_scatter(const void* ds, void* dfeats, float* dcls, float* dpos, float* dtype0, int B, int S, int D, float* part, const unsigned* drop_seed, unsigned site_in, float p_in, hipStream_t stream);

/* ---- `model.bert.type: x-transformers` encoder passes (csrc/xt.hip) ----------------------------------------------------
 * The reference instantiates x_transformers.Encoder(dim, depth, heads, attn_dropout, layer_dropout, ff_dropout, use_rmsnorm,
 * ff_glu, rotary_pos_emb) (lightning.py:93-105) — a third-party package absent from the reference tree, so these restate its
 * published algorithm (parity unpinned).  Activations are bf16 [R][ld] with ld = D rounded up to 64 and pad columns zero.
 *
 * RMSNorm: y = x / max(||x||_2 * D^-0.5, eps) * g; inv [R] keeps 1 / max(...) for the backward.  The backward returns
 * dx (+ addend, the gradient that bypasses the block through the residual connection) and accumulates dg from
 * svsr_rmsnorm_bwd_rows(R) partial rows of [ld] floats in `part`. */
int svsr_rmsnorm_fwd(const void* x, const float* g, void* y, float* inv, int R, int D, int ld, float eps, hipStream_t stream);
int svsr_rmsnorm_bwd_rows(int R);
int svsr_rmsnorm_bwd(const void* dy, const void* x, const float* g, const float* inv, const void* addend, void* dx, float* dg, float* part, int R, int D, int ld, hipStream_t stream);

/* Rotary embedding, in place, on the first 32 dims of `heads_total` consecutive 64-wide heads per row (q | k | v of the fused
 * projection); position = row % S; tab fp32 [S][32] = 16 cosines then 16 sines of position * 10000^(-j/16); sign -1 = backward. */
int svsr_rotary(void* qkv, const float* tab, int R, int S, int heads_total, int ld, int sign, hipStream_t stream);

/* GEGLU: u = [value | gate] bf16 [R][ldu] (halves I wide, I % 4 == 0); y [R][ldy] = dropout(value * gelu(gate)), zero for columns
 * >= I.  Backward: du [R][ldu] from dy [R][ldy] (mask regenerated), zero for columns >= 2I.  Dropout index = r * ldy + column. */
int svsr_geglu_fwd(const void* u, void* y, int R, int I, int ldu, int ldy, const unsigned* drop_seed, unsigned drop_site, float drop_p, hipStream_t stream);
int svsr_geglu_bwd(const void* dy, const void* u, void* du, int R, int I, int ldu, int ldy, const unsigned* drop_seed, unsigned drop_site, float drop_p, hipStream_t stream);

/* x0 = emb_dropout(cat(cls_token, cat(feats, word_mask[..., None], -1), 1)) (lightning.py:145-150): feats bf16 [B][S-1][F],
 * wmask fp32 [B][S-1] (D = F + 1) or null (D = F), cls fp32 [>= D], x0 bf16 [B*S][ld].  The backward writes dfeats bf16
 * [B][S-1][F] and adds the batch sum of row 0 into dcls (batch order fixed).  Dropout index = row * ld + column. */
int svsr_xt_embed_fwd(const void* feats, const float* wmask, const float* cls, void* x0, int B, int S, int F, int D, int ld, const unsigned* drop_seed, unsigned drop_site, float drop_p, hipStream_t stream);
int svsr_xt_embed_bwd(const void* dx0, void* dfeats, float* dcls, int B, int S, int F, int D, int ld, const unsigned* drop_seed, unsigned drop_site, float drop_p, hipStream_t stream);

/* dz = dy * act'(z) when z != null: act 1 = GELU from the saved pre-activation (BertIntermediate), act 2 = ReLU from the
 * saved output (PositionwiseFeedForward; gscale = 1/(1-p) when that output went through dropout — dropped elements are
 * exactly the zeros of the saved output); db[n] += column sums (bias gradient of any nn.Linear; db may be null), via
 * svsr_bias_act_bwd_rows(R, N) partial rows of [N] floats in `part` (0 rows: a single row slab adds into db directly). */
int svsr_bias_act_bwd_rows(int R, int N);
int svsr_bias_act_bwd(const void* dy, const void* z, void* dz, float* db, int R, int N, int n_valid, int ld, int act, float gscale, float* part, hipStream_t stream);

/* ---- losses / metric / optimiser (loss_optim.hip) --------------------------------------------------------------
 * F.cross_entropy(logits.float(), target, label_smoothing) mean over R rows (lightning.py:163-165,171): exactly one of
 * target_idx (int64 [R]) / target_prob (fp32 [R][V], pitch ldt) is non-null.  *loss = mean loss (row losses land in
 * row_loss [R] and are added in a fixed order).  A target index outside [0, V) yields NaN (torch raises a device assert). */
int svsr_ce_fwd(const void* logits, int logits_f32, int ld, const int64_t* target_idx, const float* target_prob, int ldt, int R, int V, float smoothing, float* loss, float* lse, float* row_loss, hipStream_t stream);
/* svsr_ce_bwd: dlogits bf16 [R][ldo] = gout / R * d loss / d logits; columns V .. ldo - 1 of every row are written as zeros. */
int svsr_ce_bwd(const void* logits, int logits_f32, int ld, const int64_t* target_idx, const float* target_prob, int ldt, int R, int V, float smoothing, const float* lse, const float* gout, void* dlogits, int ldo, hipStream_t stream);

/* ---- the SyncVSR audio-token head (audio_head.hip) ----------------------------------------------------------------------
 * svsr_linear_ce_fwd: loss = F.cross_entropy((h W^T + bias).reshape(-1, V), tok) of lightning.py:168-171 as ONE contraction whose
 * accumulators never leave the registers: h bf16 rows of pitch K (row r = hidden row (r / seq_T) * seq_S + seq_s0 + r % seq_T, or row r
 * when seq_T = 0), W bf16 [G*V][K] (nn.Linear layout), bias fp32 [G*V] or null, tok int64 [R*G] (row r, group g -> tok[r*G + g]: the
 * reference's logits.reshape(-1, V) order).  Writes lse [R*G], row_loss [R*G] (workspace) and *loss = their mean (fixed order).  A target
 * outside [0, V) yields NaN.  svsr_linear_ce_ok: 1 when the shape is taken (V a multiple of 320 — both codecs —, K a multiple of 64 up to 576).
 * svsr_linear_ce_bwd: the contraction again, then dlogits [R][G*V] bf16 = gout[0] / (R*G) * (softmax - onehot) for the projection's
 * data- and weight-gradient launches (svsr_igemm_fwd on the transposed weight, svsr_igemm_wgrad): no logits tensor is ever stored. */
int svsr_linear_ce_ok(int R, int K, int G, int V);
int svsr_linear_ce_fwd(const void* h, const void* w, const float* bias, const int64_t* tok, int R, int K, int G, int V, int seq_S, int seq_s0, int seq_T, float* loss, float* lse, float* row_loss, hipStream_t stream);
int svsr_linear_ce_bwd(const void* h, const void* w, const float* bias, const int64_t* tok, int R, int K, int G, int V, int seq_S, int seq_s0, int seq_T, const float* lse, const float* gout, void* dlogits, hipStream_t stream);

/* ---- the wav2vec2 audio tokeniser (w2v_codec.hip) ------------------------------------------------------------------------
 * Replaces forward_audios of the `wav2vec2` codec (LRS e2e_asr_transformer.py:167-180, LRW lightning.py:121-131): HF Wav2Vec2FeatureEncoder
 * (7 Conv1d of 512 channels, kernels 10,3,3,3,3,2,2, strides 5,2,2,2,2,2,2, exact GELU), feature_projection.layer_norm and the quantiser's
 * weight_proj + argmax (eval) / argmax of logits + Gumbel noise (training).  Activations: channels-last bf16 rows [B][rows][512].
 * svsr_w2v_conv0: layer 0 in fp32 over wave fp32 [B][L_in] followed by `pad` zeros per row: F0 = (L_in + pad - 10) / 5 + 1 frames into
 *   out [B][out_rows][512] (out_rows >= F0).  mode 0 ("layer" models): + bias, LayerNorm(512; gamma, beta, eps), GELU.  mode 1 ("group"):
 *   the pre-norm conv output (bias may be null) and, in stats (svsr_w2v_stats_floats(B, F0) floats), per 64-frame block the per-channel
 *   sums / sums of squares (plain stores) that svsr_w2v_norm_gelu mode 1 reduces in a fixed order.
 * svsr_w2v_norm_gelu: in place over the F valid rows of every clip of x [B][rows][512]: mode 0 GELU(LayerNorm(512)), mode 1 GELU(GroupNorm)
 *   with the statistics of the clip's F0 = F frames (GroupNorm(512 groups): each channel over the whole time axis, padding included).
 * Layers 1-6 are svsr_igemm_fwd over svsr_rows_plan(B, F_out, 0, 0, 512): a stride-2 kernel-k convolution reads frames 2t .. 2t+k-1, i.e.
 *   the contiguous k*512 values of source row t when rows overlap with pitch 1024 (Ci = k*512, in_pitch = 1024, in_pix = rows / 2).
 * svsr_w2v_quantize: feat bf16 [R][512] (R / F clips of F frames) -> LayerNorm(512) -> logits = . W^T + bias (W bf16 [640][512]) ->
 *   tok int64 [R / F][keep][2] = (argmax of columns 0..319, 320 + argmax of columns 320..639) of frames t < keep, ties to the lowest index:
 *   the cropped tokens[:, :T*A] of the LRS forward, contiguous, in the layout svsr_linear_ce_fwd / svsr_ce_fwd read.  seed != null: argmax of logits + g, g = -log(-log u),
 *   u = (hash(*seed, site, r * 640 + column) + 0.5) 2^-32 (the dropout hash of csrc/common.h).  logits_out (fp32 [R][640], optional): the logits. */
int64_t svsr_w2v_stats_floats(int B, int F0);
int svsr_w2v_conv0(const float* wave, int B, int L_in, int pad, const float* w, const float* bias, const float* gamma, const float* beta, float eps, void* out, int out_rows, float* stats, int mode, hipStream_t stream);
int svsr_w2v_norm_gelu(void* x, int B, int F, int rows, const float* gamma, const float* beta, float eps, float* stats, int F0, int mode, hipStream_t stream);
int svsr_w2v_quantize(const void* feat, int R, int F, int keep, const float* gamma, const float* beta, float eps, const void* w, const float* bias, const unsigned* seed, unsigned site, int64_t* tok, float* logits_out, hipStream_t stream);

/* ---- the vq-wav2vec k-means audio tokeniser (vq_codec.hip) ---------------------------------------------------------------
 * Replaces forward_audios of the `vq` codec (LRW lightning.py:121-131): fairseq ConvFeatureExtractionModel (8 Conv1d of 512 channels without
 * bias, kernels 10,8,4,4,4,1,1,1, strides 5,4,2,2,2,1,1,1, each followed by GroupNorm(1, 512) + ReLU; log(|x| + 1) at the end) and
 * KmeansVectorQuantizer (grouped 1x1 projection, GroupNorm(2, 512), nearest of 320 centroids per group).  Activations: channels-last bf16 rows
 * [B][rows][512].  Every GroupNorm takes its statistics over all frames of a clip: producers store per-(clip, block) partial {sum, sum of
 * squares} pairs, consumers add them in block order in double.  svsr_vq_part_floats(B, F, kind): floats of such a partial buffer for clips of
 *   F frames: kind 0 = [B][ceil(F / 64)][2] (svsr_vq_conv0_*, svsr_vq_gn_*), kind 1 = [B][2][ceil(F / 32)][2] (svsr_vq_project / svsr_vq_assign).
 * svsr_vq_conv0_stats: layer 0 (w fp32 [512][10]) in fp32 over wave fp32 [B][L_in] followed by `pad` zeros per row, F0 = (L_in + pad - 10) / 5 + 1
 *   frames; stores only the partial sums (kind 0) of the F0 x 512 pre-norm values.
 * svsr_vq_conv0_apply: the same convolution again, then relu(GroupNorm(1, 512) * gamma + beta) into out [B][out_rows][512] (out_rows >= F0).
 * Layers 1-7 are svsr_igemm_fwd over svsr_rows_plan(B, F_out, 0, 0, 512): a stride-s kernel-k convolution reads the contiguous k*512 values of
 *   source row t when rows overlap with pitch s*512 (Ci = k*512, in_pitch = s*512, in_pix = rows / s), followed by
 * svsr_vq_gn_partial: partial sums (kind 0) of the F valid rows of every clip of x [B][rows][512], and
 * svsr_vq_gn_relu: in place over those rows relu(GroupNorm(1, 512) * gamma + beta), mode 1: log(. + 1) on top.  Rows F .. rows - 1 are not touched.
 * svsr_vq_project: x bf16 [B * F][512], w bf16 [512][256] (output channel o of group o / 256 reads input channels (o / 256) * 256 ..) ->
 *   ze fp32 [B * F][512] and the partial sums (kind 1) of each group's F x 256 values.
 * svsr_vq_assign: z = GroupNorm(2, 512)(ze) * gamma + beta, score[v] = e2[g][v] - 2 z_g . emb[g][v] (emb bf16 [2][320][256], e2 fp32 [2][320]),
 *   tok int64 [B][keep][2] = per-group argmin of frames t < keep, ties to the lowest index, in the layout svsr_linear_ce_fwd / svsr_ce_fwd read
 *   (no + 320 offset).  A row with a NaN score in either group gets token 0 in both.  scores_out (fp32 [B * F][2][320], optional): the scores. */
int64_t svsr_vq_part_floats(int B, int F, int kind);
int svsr_vq_conv0_stats(const float* wave, int B, int L_in, int pad, const float* w, float* part, hipStream_t stream);
int svsr_vq_conv0_apply(const float* wave, int B, int L_in, int pad, const float* w, const float* gamma, const float* beta, float eps, const float* part, void* out, int out_rows, hipStream_t stream);
int svsr_vq_gn_partial(const void* x, int B, int F, int rows, float* part, hipStream_t stream);
int svsr_vq_gn_relu(void* x, int B, int F, int rows, const float* gamma, const float* beta, float eps, const float* part, int mode, hipStream_t stream);
int svsr_vq_project(const void* x, int B, int F, const void* w, float* ze, float* part, hipStream_t stream);
int svsr_vq_assign(const float* ze, int B, int F, int keep, const float* gamma, const float* beta, float eps, const float* part, const void* emb, const float* e2, int64_t* tok, float* scores_out, hipStream_t stream);

/* top-1 / top-5 accuracy (lightning.py:177-183); out2 = {top1, top5}; rows2: [B][2] float workspace. */
int svsr_topk_acc(const float* logits, const int64_t* labels, const float* soft_labels, int B, int C, float* out2, float* rows2, hipStream_t stream);

/* clip_grad_norm_ + AdamW + HF cosine-with-warm-up (lightning.py:216-223; Lightning gradient_clip_val).
 * opt_state: device struct {int step; int skipped; float lr_last; float gnorm_last; float part[1024]} (4112 bytes),
 * zero-initialised; svsr_grad_sumsq writes the 1024 partial sums of squares, svsr_adamw_step adds them in a fixed order.
 * A step whose gradient norm is NOT FINITE is skipped: parameters, moments and `step` stay as they are, `skipped` counts it and
 * gnorm_last shows the value (the reference would train on with NaN parameters; a poisoned fused-encoder launch — svsr_enc_gave_up —
 * is the case this exists for). */
int svsr_grad_sumsq(const float* g, int64_t n, void* opt_state, hipStream_t stream);
/* one range of the gradient into partial sums [part0, part0 + nparts): a step's ranges cover the buffer and the 1024 partials once each
 * (the clip of lightning's `gradient_clip_val` needs the whole norm; most of it can be summed before the last weight gradient is done) */
int svsr_grad_sumsq_parts(const float* g, int64_t n, void* opt_state, int part0, int nparts, hipStream_t stream);
int svsr_adamw_step(float* p, const float* g, float* m, float* v, void* shadow, int64_t n, int64_t decay_end, float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm, int warmup, int total_steps, void* opt_state, hipStream_t stream);
/* the same over one RANGE of the flat buffers (pointers offset by the caller, decay_end relative to the range); the step counter advances only
 * with advance != 0 — the last range of a step.  Lets a step update what the next forward needs first and the rest on another stream. */
int svsr_adamw_range(float* p, const float* g, float* m, float* v, void* shadow, int64_t n, int64_t decay_end, float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm, int warmup, int total_steps, void* opt_state, int advance, hipStream_t stream);

/* AdamW under torch.optim.lr_scheduler.OneCycleLR stepped per batch with cycle_momentum (the DC-TCN recipe, lightning.py:314-334): the
 * learning rate AND beta1 of a step are computed on the device from the step counter, with torch's phase arithmetic in double (phase ends
 * pct_start * total_steps - 1, [2 * pct_start * total_steps - 2,] total_steps - 1; a phase starts where the one before it ended), and the
 * bias correction 1 - beta1 ** step takes the step's own beta1.  No learning rate crosses the bus and nothing is read back.
 * schedule: HOST record {double max_lr, initial_lr, min_lr, base_momentum, max_momentum, pct_start; int32 three_phase, cos_anneal,
 * total_steps, reserved} (64 bytes), read during the call.
 * opt_state: the struct of svsr_adamw_step followed by {float beta1_last; int error; int reserved[2]} (4128 bytes), zero-initialised;
 * lr_last / beta1_last hold what the last counted step used.  The clip (max_norm > 0) reads svsr_grad_sumsq's partial sums; a step whose
 * gradient norm is not finite is skipped as svsr_adamw_step skips it.  A launch whose counter is already total_steps (torch raises there)
 * writes NOTHING, and the advancing launch sets `error` to 1001 instead of counting: the counter lives on the device, so that is where
 * the error code is returned; the call itself returns 1001 for a schedule no step can be taken from (total_steps < 1, pct_start outside
 * [0, 1], pct_start * total_steps == 1: torch divides by zero at step 0).  No atomics: a step's bits depend on its inputs only.
 * _range: svsr_adamw_range's contract (pointers offset by the caller, decay_end relative to the range, advance != 0 on the last range). */
int svsr_adamw_onecycle_step(float* p, const float* g, float* m, float* v, void* shadow, int64_t n, int64_t decay_end, float beta2, float eps, float weight_decay, float max_norm, const void* schedule, void* opt_state, hipStream_t stream);
int svsr_adamw_onecycle_range(float* p, const float* g, float* m, float* v, void* shadow, int64_t n, int64_t decay_end, float beta2, float eps, float weight_decay, float max_norm, const void* schedule, void* opt_state, int advance, hipStream_t stream);

/* bf16 shadows of fp32 parameters: plain cast, and a table-driven [A][T][B] -> [B][T][Apad] transpose-cast.
 * table: device array of {int64 src_off, dst_off; int32 A, T, Bd, Apad} (elements). */
int svsr_cast_bf16(const float* src, void* dst, int64_t n, hipStream_t stream);
int svsr_transpose_cast_multi(const float* src, void* dst, const void* table, int n_entries, hipStream_t stream);
/* the same from the bf16 shadow (src16: bf16 copy of the parameter buffer, same offsets): half the bytes read, identical result */
int svsr_transpose_bf16_multi(const void* src16, void* dst, const void* table, int n_entries, hipStream_t stream);
int svsr_fill_f32(float* p, int64_t n, float v, hipStream_t stream);
/* svsr_fill_ranges: base[begin, end) = the 32-bit pattern `bits` for n ranges (ranges: 2 n HOST int64 {begin, end} in floats, begin and end
 * multiples of 4, inside [0, limit)), 16 ranges per launch: the per-step fill of the parts of the flat gradient buffer no store-mode writer
 * covers (pads, 1-D tensors, tensors whose writers only add), as ONE launch instead of a memset of the whole buffer.  bits = 0 in a training
 * step; a NaN pattern in the tests that prove no writer reads what it should have stored. */
int svsr_fill_ranges(float* base, int64_t limit, const int64_t* ranges, int n, unsigned bits, hipStream_t stream);
/* scalars on the device, so that a step never depends on a host value: *word += delta (the dropout seed word, advanced once per
 * training forward: lightning.py:150 draws fresh masks every step);  *out = *a + wb * *b  (loss_total = loss_category +
 * lambda_audio * loss_audio, lightning.py:187). */
/* ---- fused encoder forward (enc_fused.hip) -----------------------------------------------------------------------
 * svsr_enc_fwd replaces the forward of `n_layers` (<= 8 per call) consecutive HF BertLayers of the word-level model's encoder
 * (reference LRW/video/src/lightning.py:92,152-156: BertSelfAttention, BertSelfOutput, BertIntermediate, BertOutput) for width 512,
 * 8 heads of 64, FFN 2048 and sequences of S <= 32 rows: ONE launch per 32 sequences instead of seven per layer.  Eight workgroups
 * per sequence (one per head / column eighth) exchange ctx, ao, hg and f through memory between arrival counters (write-through
 * stores, relaxed agent-scope counter, L1-bypassing loads; all eight must be resident together, which the 32-sequence launches
 * guarantee on 256 CUs).  x0 bf16 [B*S][512]; `layers`: HOST array of records (copied by value into the launch); every tensor a
 * layer writes has the contents the unfused launches (svsr_igemm_fwd, svsr_mha_fwd, svsr_add_ln_fwd) give it, dropout masks included.
 * ws: svsr_enc_fwd_ws_bytes(B) bytes of device workspace (arrival counters, zeroed here; word B = error flag, non-zero if a bounded
 * wait gave up; the layer records). */
/* A bounded cluster wait that gives up is LOUD: the launch's error word (word B of ws) is set, the giving-up workgroup overwrites its slice
 * of the launch's final output with NaN (the step's loss / gradient norm turn NaN without a host synchronisation), and a sticky
 * process-wide flag is set that svsr_enc_gave_up(reset) returns (1 / 0; it synchronises: call it where the host waits anyway;
 * -1 if the flag cannot be read).  svsr_enc_gave_up_peek() reads a copy of the flag that the giving-up workgroup stores into pinned host
 * memory: no synchronisation, so engine.TrainStep looks at it before every step and, when set, re-routes the encoder to the per-layer launch
 * chain for the rest of the run (the poisoned step itself is skipped by svsr_adamw_step's non-finite guard).  A launch holds at most
 * svsr_device_cus() / 8 sequences. */
int svsr_enc_gave_up(int reset);
int svsr_enc_gave_up_peek(void);
int svsr_debug_enc_spin_limit(unsigned limit);     /* test aid: polls before a cluster wait gives up (0 = default 2^20; 1 provokes the give-up path) */
int64_t svsr_enc_fwd_ws_bytes(int B);
int svsr_debug_enc_trace(int64_t* out, int n);     /* debug: out == null arms s_memtime stamps of workgroup 0 at the phase boundaries of the next launches; else copies n stamps out */
int svsr_enc_fwd(const void* x0, const svsr_enc_layer* layers, int n_layers, int B, int S, float ln_eps, const unsigned* drop_seed, float p_hidden, float p_attn, void* ws, int64_t ws_bytes, hipStream_t stream);

/* Backward of the same layers in one launch per 32 sequences (enc_fused.hip, k_enc_bwd): replaces, per layer, two svsr_add_ln_bwd, four
 * svsr_igemm_fwd data-gradient launches, svsr_bias_act_bwd, svsr_mha_bwd and the dropout re-scalings between them.  dy bf16 [B*S][512] =
 * gradient of the last layer's output; layers = HOST array in forward order.  Per layer it writes ds2 / df / dx1 / ds1 / dao / dx bf16
 * [R][512], dz bf16 [R][2048], dqkv bf16 [R][1536] — (hg, df), (x1, dz), (ctx, dao), (xin, dqkv) are the operand pairs of the layer's four weight
 * gradients; df may alias ds2 and dao ds1 without hidden dropout — and part1 / part2 fp32 [B][2][512], one row of {sum dy*xhat | sum dy} per
 * sequence and LayerNorm (svsr_colsum_rows over B rows of 1024 gives gamma | beta gradients).  layers[0].dx = gradient of the first input. */
int64_t svsr_enc_bwd_ws_bytes(int B);
int svsr_enc_bwd(const void* dy, const svsr_enc_bwd_layer* layers, int n_layers, int B, int S, const unsigned* drop_seed, float p_hidden, float p_attn, void* ws, int64_t ws_bytes, hipStream_t stream);

int svsr_word_add(int* word, int delta, hipStream_t stream);
int svsr_lincomb2(const float* a, const float* b, float wb, float* out, hipStream_t stream);
/* out0 = (wa*a + wb*b) + wc*c with one rounding per product and per sum (what `mtlalpha * loss_ctc + (1 - mtlalpha) * loss_att + w * loss_audio` gives
 * in torch, reference LRS e2e_asr_transformer.py:217-224), and out1 = num / den (the token accuracy) when out1 is not null: 0-d device values */
int svsr_lincomb3_ratio(const float* a, float wa, const float* b, float wb, const float* c, float wc, float* out0, const float* num, const float* den, float* out1, hipStream_t stream);

/* Device-side input pipeline (reference LRW/video/src/data.py:150,157-171: x/255 -> RandomHorizontalFlip ->
 * RandomResizedCrop | CenterCrop -> Normalize(0.421, 0.165)): stored uint8 clips [B][T][Hs][Ws] -> fp32 model input
 * [B][1][T][H][W].  params: device int32 [B][5] = {top, left, h, w, flip} chosen by the host per clip; the window is resized to
 * H x W with bilinear sampling (align_corners = False, no antialias; a window of exactly H x W is a plain crop). */
int svsr_clip_prep(const void* src_u8, const int* params, float* dst, int B, int T, int Hs, int Ws, int H, int W, float mean, float std, hipStream_t stream);

/* Device-side input pipeline of the LRS path (csrc/lrs_prep.hip), what the reference runs per sample in dataloader workers
 * (LRS/video/datamodule/transforms.py:89-135, av_dataset.py:30-41) and pads on the host (data_module.py:12-43).
 *
 * svsr_lrs_clip_prep: VideoTransform("train") (x / 255 -> RandomResizedCrop(96) -> RandomHorizontalFlip -> Grayscale -> Normalize(0.421,
 * 0.165)) and the val / test pipelines (Resize(96) | CenterCrop(96)) over a batch of clips of DIFFERENT lengths in one launch.
 * src_u8: packed uint8 frames [total_frames][Hs][Ws], one channel (AVDataset decodes with TJPF_GRAY, so Grayscale() is the identity);
 * off: device int32 [B + 1], clip b holds frames off[b] .. off[b + 1] - 1; params: device int32 [B][5] = {top, left, h, w, flip} as in
 * svsr_clip_prep; dst: fp32 [B][Tpad][1][H][W], the layout E2E.forward takes.  Frame t < T_b = off[b + 1] - off[b] of clip b is
 * Normalize(flip(resize(window(x / 255)))) with svsr_clip_prep's sampling formulas (the same formulas, not bit-identical results: the compiler contracts them differently in the two
 * kernels, measured difference at most 9.5e-7): bilinear, align_corners = False, NO
 * antialias, a window of exactly H x W is a plain crop.  (torchvision's resize of a tensor antialiases only when it shrinks.  The LRS crops
 * are stored at 96 x 96 and RandomResizedCrop(96) never draws a window larger than the stored frame, so it only enlarges and antialias
 * never acts; a larger stored frame with a window above H x W is sampled WITHOUT antialias here, which is then not what torchvision
 * computes.)  Frames T_b .. Tpad - 1 are written as 0.0 — what collate_pad pads the normalised clips with — and so is any frame that
 * would lie outside [0, total_frames); a window is clamped into the stored frame: nothing outside src is read whatever off and params hold.
 * tmask: device uint8 [B][Tpad] or null; a real frame with tmask != 0 is written as (0 - mean) / std, a frame zeroed in front of Normalize
 * (AdaptiveTimeMask(10, 25), transforms.py:101, commented out in the reference: null by default).  Every element of dst is written: no
 * zero-fill beside the launch.  Grid: one workgroup per (clip, frame, block of 32 rows) up to 16384, the rest in a stride loop; 16-byte
 * stores where W % 4 == 0 and dst is 16-byte aligned.  max_blocks > 0 caps the grid instead (a test aid: the result does not depend on it).
 * Moves total_frames * Hs * Ws bytes in (the window's share of them) and B * Tpad * H * W * 4 bytes out: HBM-bound on the write.
 *
 * svsr_wave_prep: AudioTransform (AddNoise = torchaudio.functional.add_noise at a drawn SNR, then F.layer_norm(x, x.shape, eps = 1e-8)).
 * wave: fp32 [B][Spad], or int16 [B][Spad] with wave_i16 != 0 (a sample counts as v / 32768, pydub_to_np's scale); len: device int32 [B] real
 * samples per clip (clamped to [0, Spad]); noise: device fp32 noise bank [Nn] or null; nstart: device int32 [B], clip b mixes noise[nstart[b]
 * .. nstart[b] + len[b]); snr_db: device fp32 [B]; out: fp32 [B][Spad].  Per clip over its real samples
 *     Ex = sum x^2, En = sum n^2, scale = sqrt(Ex / En) * 10^(-snr_db / 20), y = x + scale * n,
 *     out = (y - mean(y)) / sqrt(var_biased(y) + eps),            samples >= len: 0.0
 * scale is DEFINED as 0 — the noise-free normalisation, no NaN — where Ex == 0 or En == 0, where noise is null (the val / test transform
 * without snr_target) and where the clip's noise segment would leave the bank (nothing outside it is read).  snr_db = 999999, the
 * reference's "clean" level, underflows the power to 0: scale is an exact 0 and the output is bit-identical to noise = null.  A clip of
 * length 0 is all padding.  Reductions: the first launch writes, per 4096 samples of a clip, one row of the five sums {x, n, x^2, n^2, x n}
 * in DOUBLE into ws (caller-owned, svsr_wave_prep_ws_bytes(B, Spad) bytes, 8-byte aligned); the second adds a clip's rows in index order,
 * derives scale, mean and variance from them in double (sum y = Sx + scale Sn, sum y^2 = Sxx + 2 scale Sxn + scale^2 Snn: a DC offset
 * costs the variance no digits that matter) and writes out, each element evaluated in double and rounded once.  No atomics, a fixed
 * order, a partition that depends on the lengths alone: bit-identical from run to run and under any max_blocks (as above: a test aid,
 * 0 = one workgroup per 4096 samples up to 16384).  Bounds (SVSR_ERR_ARG): B >= 1, 1 <= Spad <= 2^30, eps >= 0, ws large enough. */
int svsr_lrs_clip_prep(const void* src_u8, int64_t total_frames, const int* off, const int* params, const void* tmask, float* dst, int B, int Tpad, int Hs, int Ws, int H, int W, float mean, float std, int max_blocks, hipStream_t stream);
int64_t svsr_wave_prep_ws_bytes(int B, int Spad);
int svsr_wave_prep(const void* wave, int wave_i16, const int* len, const float* noise, int64_t Nn, const int* nstart, const float* snr_db, float* out, int B, int Spad, float eps, void* ws, int64_t ws_bytes, int max_blocks, hipStream_t stream);

/* Device-side training inputs of the LRW path (csrc/lrw_prep.hip): the reference's per-clip chain x / 255 -> RandomHorizontalFlip ->
 * RandomResizedCrop | Identity -> Grayscale -> TimeMask -> Normalize (LRW/video/src/data.py:157-164) and the frame splice of its sequential
 * CutMix (LRW/video/src/augment.py:27-118) in two launches per batch.  src_u8: uint8 clips [B][T][Hs][Ws]; params: device int32 [B][5] =
 * {top, left, h, w, flip} as in svsr_clip_prep, sampled by the SAME device function (csrc/clip_sample.h): x_s[t], frame t of clip s in front
 * of Normalize, is what svsr_clip_prep samples, and a frame that is neither masked nor spliced has svsr_clip_prep's bits.
 *
 * svsr_lrw_clip_sums: frame_sums fp32 [B][T], the sum of x_s[t] over the frame's H * W pixels.  One workgroup per (clip, frame) up to 16384,
 * the rest in a stride loop; thread i of 256 adds pixels i, i + 256, ... in index order, the 64 lanes in a butterfly, the 4 waves in wave
 * order: the partition depends on H * W alone.  No atomics; bit-identical from run to run and under any max_blocks (> 0 caps the grid: a
 * test aid).  Reads the windows' share of B * T * Hs * Ws bytes, writes B * T * 4.
 *
 * svsr_lrw_clip_mix: dst fp32 [B][1][T][H][W], dst[b][0][t] = Normalize(TimeMask(x_s))[t] with s = frame_src[b][t] — the ORIGINAL clip that
 * frame t of sample b comes from once the reference's in-place chain is resolved (augment.make_plan); crop, flip and mask are clip s's.
 * frame_src: device int32 [B][T], clamped into [0, B).  runs: device int32 [B][n_mask][2] = (start, length) of clip s's masked runs in the
 * order TimeMask draws them, clamped into [0, T] (a length of 0 masks nothing); n_mask = 0: no mask, runs may be null.  The fill of run j is
 * the mean over all T * H * W values of the clip AS MASKED SO FAR, derived per workgroup from the clip's T frame sums:
 *     S = sum_t fs[t];   per run: m = S / (T H W), for t in the run: S += H W m - cur[t], cur[t] = H W m
 * (fp32, a fixed order) and a masked frame is written as the constant (fill - mean) / std; with replace_with_zero the fill is 0 and
 * frame_sums may be null.  Any other frame is sampled and normalised as svsr_clip_prep does.  Nothing outside src_u8 is read whatever
 * params, frame_src and runs hold.  One workgroup per (sample, frame, block of 32 rows) up to 16384, the rest in a stride loop; 16-byte
 * stores where W % 4 == 0 and dst is 16-byte aligned; max_blocks as above.  Every element of dst is written once.  Together the two
 * launches read the clips twice (uint8) and write B * T * H * W * 4 bytes: HBM-bound on the write.
 * Bounds (SVSR_ERR_ARG): B, T, Hs, Ws, H, W >= 1, T <= 256, Hs * Ws, H * W and B * T <= 2^24, std > 0, 0 <= n_mask <= 65536, max_blocks >= 0. */
int svsr_lrw_clip_sums(const void* src_u8, const int* params, float* frame_sums, int B, int T, int Hs, int Ws, int H, int W, int max_blocks, hipStream_t stream);
int svsr_lrw_clip_mix(const void* src_u8, const int* params, const int* frame_src, const int* runs, const float* frame_sums, float* dst, int B, int T, int Hs, int Ws, int H, int W, int n_mask, int replace_with_zero, float mean, float std, int max_blocks, hipStream_t stream);

/* Device-side training inputs of the DC-TCN word-level path (csrc/dctcn_prep.hip): the reference's LRWDatasetForDCTCN per clip
 * (LRW/video/src/data.py:70-139: videos = 2 x / 255 - 1, _mask_frames, _trim_frames, then the transform chain, which divides by 255 a
 * second time in front of Normalize) and the clip mixup of its module (lightning.py:264-270), in at most three launches per batch.
 * src_u8: uint8 clips [B][T][Hs][Ws].
 *
 * svsr_dctcn_clip_sums: frame_sums uint32 [B][T], the exact integer sum of every STORED frame (Hs * Ws <= 2^24 keeps it in range).  One
 * workgroup per frame up to 16384, the rest in a stride loop.  Needed only when some clip masks a run of positive length.
 *
 * svsr_dctcn_clip_mix: dst fp32 [B][1][T][H][W].  table: device int32 [B][9] = {top, left, h, w, flip, shift, trunc, mask_off, mask_len}
 * per clip; the window as in svsr_clip_prep.  val(s, t), frame t of clip s in front of Normalize:
 *     t >= trunc_s                                  0
 *     ts = (t - shift_s) mod T in [mask_off_s, mask_off_s + mask_len_s)      m_s / 255, m_s = 2 S_s / (255 T Hs Ws) - 1, S_s the clip's T
 *                                                   frame sums added in 64-bit integer (m_s in double, rounded once)
 *     otherwise                                     (2 u / 255 - 1) / 255, u = stored frame ts sampled by csrc/clip_sample.h with clip s's
 *                                                   window and flip
 * dst[b][0][t] = (x - mean) / std with x = val(b, t) for lam == 0 and x = val(b, t) + lam (val(b', t) - val(b, t)), b' = (b - 1 + B) mod B,
 * otherwise (torch.lerp(v, v.roll(1, 0), lam) for lam < 0.5).  frame_sums null: no frame is masked (every mask_len counts as 0).  trunc
 * and mask_off are clamped into [0, T], mask_len into [0, T - mask_off], shift is reduced mod T: nothing outside src_u8 is read whatever the
 * table holds.  Masked and trimmed frames are written without sampling.  One workgroup per (sample, frame, block of 32 rows) up to 16384,
 * the rest in a stride loop; 16-byte stores where W % 4 == 0 and dst is 16-byte aligned.  Every element of dst is written once: the launch
 * reads the clips once (twice with lam != 0) as uint8 and writes B * T * H * W * 4 bytes, HBM-bound on the write.
 *
 * svsr_dctcn_wave_trim: wave fp32 [B][L] -> out fp32 [B][L], table device int32 [B][2] = {ashift, azero}:
 * out[b][i] = i < azero_b ? wave[b][(i - ashift_b) mod L] : 0; azero clamped into [0, L].  Out of place: out == wave is refused.
 *
 * No atomics; bit-identical from run to run and under any max_blocks (> 0 caps the grid: a test aid, 0 = the default grid).
 * Bounds (SVSR_ERR_ARG): B, T, Hs, Ws, H, W >= 1, T <= 256, Hs * Ws, H * W and B * T <= 2^24, std > 0, 0 <= lam <= 0.5, 1 <= L <= 2^30,
 * max_blocks >= 0, no null buffer but frame_sums of svsr_dctcn_clip_mix. */
int svsr_dctcn_clip_sums(const void* src_u8, unsigned* frame_sums, int B, int T, int Hs, int Ws, int max_blocks, hipStream_t stream);
int svsr_dctcn_clip_mix(const void* src_u8, const int* table, const unsigned* frame_sums, float* dst, int B, int T, int Hs, int Ws, int H, int W, float lam, float mean, float std, int max_blocks, hipStream_t stream);
int svsr_dctcn_wave_trim(const float* wave, const int* table, float* out, int B, int L, int max_blocks, hipStream_t stream);

/* ---- LRS (E2E: Conformer encoder + CTC / attention decoder) -----------------------------------------------------
 * Multi-head attention with 64-wide heads (mha.hip).  q rows [B*Lq] with pitch q_pitch (head h at column h*64), k/v rows
 * [B*Lk] with pitch kv_pitch; klen[b] = number of valid keys (null: all), causal != 0 masks j > i.  With pe != null the
 * Conformer's relative-position scores are used: ((q+u)·k_j + (q+v)·pe[Lq-1+j-i]) * scale, pe = linear_pos(pos_emb)
 * [2*Lq-1][pe_pitch] (reference LRS/video/espnet/nets/pytorch_backend/transformer/attention.py:191-278 incl. rel_shift
 * :216-236; plain MHA :38-108; mask semantics :71-78).  probs [B*H][Lq][ldp] bf16 (before dropout) is kept for the backward;
 * attention dropout (attention.py:80) uses the keep decision hash(*drop_seed, drop_site, index into probs). */
int svsr_mha_fwd(const void* q, int q_pitch, const void* k, const void* v, int kv_pitch, const void* pe, int pe_pitch, const float* bias_u, const float* bias_v, const int* klen, int causal, int B, int H, int dh, int Lq, int Lk, int ldp, float scale, void* ctx, int ctx_pitch, void* probs, const unsigned* drop_seed, unsigned drop_site, float drop_p, hipStream_t stream);

/* backward of svsr_mha_fwd: ds [B*H][Lq][ldp] workspace (score gradients); dq/dk/dv written (not accumulated); for the
 * relative-position form also dq_ac / dq_bd (the two summands of dq, whose column sums are the pos_bias_u / pos_bias_v
 * gradients) and dpe [2*Lq-1][dpe_pitch] (gradient of the projected position table, feeds linear_pos's weight gradient);
 * pe_part: fp32 workspace [B][2*Lq-1][dpe_pitch] (per-batch-item partials of dpe; dpe_pitch must equal H*64). */
int svsr_mha_bwd(const void* dctx, int dctx_pitch, const void* q, int q_pitch, const void* k, const void* v, int kv_pitch, const void* pe, int pe_pitch, const float* bias_u, const float* bias_v, const void* probs, void* ds, int B, int H, int dh, int Lq, int Lk, int ldp, float scale, void* dq, int dq_pitch, void* dq_ac, void* dq_bd, int aux_pitch, void* dk, void* dv, int dkv_pitch, void* dpe, int dpe_pitch, float* pe_part, const unsigned* drop_seed, unsigned drop_site, float drop_p, hipStream_t stream);

/* The same attention without the probability matrix on the way forward (mha_flash.h; attention.py:38-108,191-278 as above): keys streamed in
 * blocks of 32 with an online softmax, one wave per 32-query tile, up to eight tiles of one (clip, head) per workgroup.  The forward keeps
 * lse [B*H][Lq] fp32 (log-sum-exp of a query's scaled, masked scores; +inf when every key is masked) instead of probs; dropout decisions are
 * the same hash(*drop_seed, drop_site, (bh * Lq + i) * ldp + j) as svsr_mha_fwd's.  The backward recomputes P from lse and takes
 * rowsum(P o dP) as dctx_i . ctx_i (ctx: the forward's output); its query pass writes probs / ds [B*H][Lq][ldp] bf16 (ldp % 8 == 0) as
 * WORKSPACE for the key and position-table passes, which are svsr_mha_bwd's.  ws: svsr_mha_flash_ws_bytes(H, Lq) bytes (the transposed
 * position table; rel-pos only).  klen / causal must be the forward's. */
int64_t svsr_mha_flash_ws_bytes(int H, int Lq);
int svsr_mha_flash_fwd(const void* q, int q_pitch, const void* k, const void* v, int kv_pitch, const void* pe, int pe_pitch, const float* bias_u, const float* bias_v, const int* klen, int causal, int B, int H, int dh, int Lq, int Lk, int ldp, float scale, void* ctx, int ctx_pitch, float* lse, const unsigned* drop_seed, unsigned drop_site, float drop_p, hipStream_t stream);
int svsr_mha_flash_bwd(const void* dctx, int dctx_pitch, const void* ctx, int ctx_pitch, const float* lse, const void* q, int q_pitch, const void* k, const void* v, int kv_pitch, const void* pe, int pe_pitch, const float* bias_u, const float* bias_v, const int* klen, int causal, void* probs, void* ds, int B, int H, int dh, int Lq, int Lk, int ldp, float scale, void* dq, int dq_pitch, void* dq_ac, void* dq_bd, int aux_pitch, void* dk, void* dv, int dkv_pitch, void* dpe, int dpe_pitch, float* pe_part, void* ws, int64_t ws_bytes, const unsigned* drop_seed, unsigned drop_site, float drop_p, hipStream_t stream);
/* the same in two parts (parts bit 0: query + key passes — dq, dq_ac, dq_bd, dk, dv; bit 1: the position-table pass — dpe, which only the weight
 * gradient of linear_pos reads, so it may be issued on another stream behind bit 0's launches; 3 = svsr_mha_flash_bwd; bit 2, with bit 0: ws already
 * holds the transposed position table, made by svsr_mha_pe_transpose — it depends on pe alone, so the forward or another stream can make it) */
int svsr_mha_pe_transpose(const void* pe, int pe_pitch, int H, int Lq, void* ws, int64_t ws_bytes, hipStream_t stream);
int svsr_mha_flash_bwd_parts(const void* dctx, int dctx_pitch, const void* ctx, int ctx_pitch, const float* lse, const void* q, int q_pitch, const void* k, const void* v, int kv_pitch, const void* pe, int pe_pitch, const float* bias_u, const float* bias_v, const int* klen, int causal, void* probs, void* ds, int B, int H, int dh, int Lq, int Lk, int ldp, float scale, void* dq, int dq_pitch, void* dq_ac, void* dq_bd, int aux_pitch, void* dk, void* dv, int dkv_pitch, void* dpe, int dpe_pitch, float* pe_part, void* ws, int64_t ws_bytes, const unsigned* drop_seed, unsigned drop_site, float drop_p, int parts, hipStream_t stream);

/* Conformer convolution module core (transformer/convolution.py:56-75): u [B*T][2D] = pointwise_cov1 output ->
 * GLU -> depthwise Conv1d(K odd <= 31, pad (K-1)/2, weight [D][K], bias) -> c [B*T][D] bf16 + BatchNorm1d partial sums
 * stats[rows][2][D], rows = svsr_glu_dwconv_fwd_stat_rows(B, T) (finalised by svsr_bn_finalize; BN+Swish itself is svsr_bn_act_fwd act 2). */
int svsr_glu_dwconv_fwd_stat_rows(int B, int T);
int svsr_glu_dwconv_fwd(const void* u, const float* w, const float* bias, void* c, float* stats, int B, int T, int D, int K, hipStream_t stream);

/* backward: dc = gradient of c -> du [B*T][2D]; dw [D][K] and dbias [D] accumulated.  part: fp32 workspace of
 * nsplit * D * (K+1) floats. */
int svsr_glu_dwconv_bwd(const void* dc, const void* u, const float* w, void* du, float* dw, float* dbias, float* part, int nsplit, int B, int T, int D, int K, hipStream_t stream);
/* the same in two parts (bit 0: du and the partial rows; bit 1: the fixed-order sum of the rows into dw / dbias, which nothing in the backward
 * chain waits for — another stream may take it; part must then be a buffer of its own until that launch is done) */
int svsr_glu_dwconv_bwd_parts(const void* dc, const void* u, const float* w, void* du, float* dw, float* dbias, float* part, int nsplit, int B, int T, int D, int K, int parts, hipStream_t stream);

/* CTC loss as the reference calls it (ctc.py:44-74,83-151): log_softmax over V, torch.nn.CTCLoss(reduction="sum",
 * zero_infinity=True), blank 0, divided by the batch size.  logits fp32 [B*T][ld]; labels int64 [B][Lmax] padded with -1
 * at the tail; ilen int32 [B].  Workspaces: lse [B*T], ab [B][T][2*Lmax+1], nll [B].  *loss = sum_b nll_b / B.
 * ilen is not trusted: an item with ilen[b] < 1 or ilen[b] > T contributes 0 to the loss (B still divides), gets zero rows from
 * svsr_ctc_grad, and no logit, lse or ab row is read or written for it. */
int svsr_ctc_fwd(const float* logits, int ld, const int64_t* labels, int Lmax, const int* ilen, int B, int T, int V, float* lse, float* ab, float* nll, float* loss, hipStream_t stream);

/* dlogits [B*T][ldo] bf16 = gout/B * (softmax - label occupancy) for t < ilen[b], 0 elsewhere (and for infeasible targets and
 * items whose ilen[b] is outside [1, T]); all ldo columns of every row are written (columns V.. with 0). */
int svsr_ctc_grad(const float* logits, int ld, const int64_t* labels, int Lmax, const int* ilen, int B, int T, int V, const float* lse, const float* ab, const float* nll, const float* gout, void* dlogits, int ldo, hipStream_t stream);

/* CTC prefix scores of beam-search extensions (espnet/nets/ctc_prefix_score.py:11-165 `CTCPrefixScoreTH.__call__`, driven by
 * scorers/ctc.py:87-127 from LRS/video/lightning.py:237-279).  logp fp32 [T][ldp] = log-softmax of ctc_lo over the clip;
 * r_prev fp32 [n][T][2] = (non-blank, blank) forward log-probabilities of each hypothesis' prefix; last int64 [n] = last label
 * of each prefix; ids int64 [n][S] = candidate labels per hypothesis (null: all V labels, S = V); out_len = labels in the
 * prefixes without <sos>.  Writes r_new fp32 [n][S][T][2] (state of every extension) and psi fp32 [n][S] (log prefix
 * probability; eos -> total probability of the prefix, blank -> -1e10).  A candidate outside [0, V) is an impossible extension: its
 * r_new and psi are -1e10 and logp is not read for it.  Ids and last labels are compared as the int64 values they are (2^32 + 5 is not
 * label 5; a last label outside [0, V) equals no candidate).  Defined in lrs_search.hip: the kernel of svsr_ctc_prefix_score_clips with one
 * clip of T frames. */
int svsr_ctc_prefix_score(const float* logp, int ldp, const float* r_prev, const int64_t* last, const int64_t* ids, float* r_new, float* psi, int T, int V, int n, int S, int out_len, int blank, int eos, hipStream_t stream);

/* Decoder input: x[r] = emb[tok[r]] * scale + pe[r % L]  (torch.nn.Embedding + PositionalEncoding, decoder.py:80-84,
 * embedding.py:78-89); backward scatter-adds scale * dx into demb. */
/* add_sos_eos (reference add_sos_eos.py:10-31, e2e_asr_transformer.py:203-215) + the CTC label form, one launch: label [B][L] int64 with
 * ignore_id padding (dropped wherever it sits in a row, as the reference's `y[y != ignore_id]`) -> labels [B][L] (live tokens, -1 padded),
 * ys_in / ys_out [B][L+1] (sos = eos; ys_out padded with ignore_id).  A live token outside [1, odim) — torch's Embedding / CTCLoss stop on it
 * with a device-side assert — is replaced by eos and reported through svsr_lrs_target_errors (nothing traps). */
int svsr_lrs_targets(const int64_t* label, int B, int L, int odim, int64_t ignore_id, int64_t eos, int64_t* labels, int64_t* ys_in, int64_t* ys_out, hipStream_t stream);
/* sticky error word of svsr_lrs_targets: 1 if a label outside [1, odim) was met since the last reset (it was replaced by eos so that no
 * later kernel leaves its tables; ignore_id entries anywhere in a row are dropped as the reference's add_sos_eos drops them), else 0; -1 if
 * the word cannot be read.  Synchronises. */
int svsr_lrs_target_errors(int reset);
int svsr_embed_pos_fwd(const int64_t* tok, const float* emb, const float* pe, void* x, int R, int L, int D, float scale, hipStream_t stream);
int svsr_embed_pos_bwd(const int64_t* tok, const void* dx, float* demb, int R, int D, float scale, hipStream_t stream);

/* ESPnet LabelSmoothingLoss (label_smoothing_loss.py:41-63): KL(true || softmax(logits)) summed over rows whose target
 * is not -1, times inv_denom (1/batch, or 1/#tokens with length normalisation); true = 1-smoothing at the target and
 * smoothing/(V-1) elsewhere.  counts[0] = rows whose argmax equals the target, counts[1] = live rows (th_accuracy,
 * nets_utils.py:303-323).  logits fp32 [R][ld]; lse [R] saved for the backward; rows3: [R][3] float workspace. */
int svsr_ls_loss_fwd(const float* logits, int ld, const int64_t* target, int R, int V, float smoothing, float inv_denom, float* loss, float* lse, float* counts, float* rows3, hipStream_t stream);
int svsr_ls_loss_bwd(const float* logits, int ld, const int64_t* target, int R, int V, float smoothing, float inv_denom, const float* lse, const float* gout, void* dlogits, int ldo, hipStream_t stream);

/* y = alpha * dropout_p(x) over n (multiple of 8) contiguous bf16 elements (y may alias x).  Dropout everywhere in this
 * library is counter based: element i of a tensor is kept iff mix(i * 2654435761 + key) >= p * 2^32 with
 * key = mix(*drop_seed * 0x9E3779B9 + drop_site * 0x7F4A7C15 + 0x165667B1) and mix = the murmur3 finaliser; kept values are
 * scaled by 1/(1-p).  The backward passes regenerate the mask from (seed, site); drop_seed is a device word the caller
 * advances once per step.  drop_seed == null or p == 0 disables it. */
int svsr_scale_bf16(const void* x, void* y, int64_t n, float alpha, const unsigned* drop_seed, unsigned drop_site, float drop_p, hipStream_t stream);

/* ---- Transformer language-model scorer of the beam search (lrs_lm.hip) -----------------------------------------------
 * Replaces the cached self-attention of TransformerLM.score / batch_score (reference LRS/video/espnet/nets/pytorch_backend/lm/
 * transformer.py:176-250 -> transformer/encoder.py:291-319 -> encoder_layer.py:98-120 -> attention.py:38-108), whose cache is
 * re-stacked per hypothesis and re-projected over the whole prefix every step.  Here the state of a search is, per layer, an
 * APPEND-ONLY pool of bf16 rows q | k | v (pitch elements per row, >= 3 * H * 64) shared by all hypotheses, plus ONE int32 row table
 * [n][table_pitch]: entry p of row b names the pool row of position p of hypothesis b.
 *   e >= 0: row e, visible as a key;  e == -1: no row (never a key; as a query: zeros);  e <= -2: row -e - 2, a query but never a key
 *   (the reference's key mask `ys != 0`, lm/transformer.py:135-138).  Rows outside [0, pool_rows) count as e == -1.
 * svsr_mha_table_fwd: for hypothesis b and query position j in [L - Lq, L): q of row table[b][j] against the keys / values of rows
 * table[b][0..j] (causal by construction), softmax in fp32 (scores * scale), ctx bf16 [n * Lq][ctx_pitch] (H * 64 written per row).
 * Lq = 1 is a beam step, Lq = L the prefix pass.  A query without a visible key writes zeros.  One wave per (b, j, head); it gathers
 * (j + 1) * 256 bytes: n * Lq * H * L * 256 at most per launch, no contraction — latency / gather bound by construction.
 * svsr_lm_embed_fwd: the tail of the LM's input layer (encoder.py:143-150 after Embedding + Linear): out bf16 [R][D] =
 * relu(LayerNorm(x[r]; gamma, beta, eps)) * scale + pe[pos[r]], x bf16 rows of pitch x_pitch, pe fp32 [pe_rows][D], pos int32 [R]
 * (clamped into the table), D % 8 == 0 up to 2048. */
int svsr_mha_table_fwd(const void* pool, int pool_rows, int64_t pitch, const int* table, int table_pitch, int n, int Lq, int L, int H, float scale, void* ctx, int64_t ctx_pitch, hipStream_t stream);
int svsr_lm_embed_fwd(const void* x, int64_t x_pitch, const float* gamma, const float* beta, const float* pe, int pe_rows, const int* pos, int R, int D, float eps, float scale, void* out, hipStream_t stream);

/* ---- Recurrent language-model scorer of the beam search (lrs_rnnlm.hip) ------------------------------------------------
 * Replaces one nn.LSTMCell / nn.GRUCell of DefaultRNNLM (reference LRS/video/espnet/nets/pytorch_backend/lm/default.py:396-429) together
 * with the embedding lookup in front of layer 0 and the per-hypothesis state gather the search does between two steps
 * (default.py:193-213: a dict of lists of rows, re-stacked every step).
 * svsr_rnn_cell_step: ONE layer of ONE step for R hypotheses.  gru = 0: LSTM (gates i, f, g, o), 1: GRU (r, z, n) — torch's orders.
 *   x_r  = x[xidx ? xidx[r * xidx_stride] : r]       x bf16 [x_rows][x_pitch >= Ep]: the embedding table (xidx = the tokens) or the bf16
 *                                                    output rows of the layer below (xidx = NULL); an index outside [0, x_rows): zeros
 *   hp_r, cp_r = h_prev[src[r]], c_prev[src[r]]      fp32 [prev_rows][Up], rounded to bf16 for the contraction only; src = NULL, or
 *                                                    src[r] outside [0, prev_rows): zeros (the first step)
 *   LSTM: c = sig(f) cp + sig(i) tanh(g), h = sig(o) tanh(c);  GRU: n = tanh(W_in x + b_in + r (W_hn hp + b_hn)), h = (1 - z) n + z hp
 *   h_out, c_out fp32 [R][Up] (c_out / c_prev unused by the GRU), h16_out bf16 [R][Up] or NULL: the same h, the next layer's / the output
 *   projection's input.  Units u >= U (the padding) are written as exact zeros.  h_out must not be h_prev (nor c_out c_prev): a step
 *   reads one buffer of a ping-pong pair and writes the other, which is what folds the search's select_states into the next step.
 * wpk: bf16 [Up / 16][(Ep + Up) / 32][G][64][8] (G = 4 | 3), the MFMA B fragments in the order the lanes read them: entry (t, s, g, l, j) =
 *   W_g[16 t + (l & 15)][32 s + 8 (l >> 4) + j] with W_g = [W_ih,g | W_hh,g] zero-padded to [Up][Ep + Up].  bias: fp32 [Up / 16][4][16]:
 *   LSTM b_ih + b_hh per gate; GRU r, z (summed), b_in, b_hn.  (syncvsr_amd.lrs_lm.pack_rnn_cell / unpack_rnn_cell.)
 * Grid: one workgroup per 16 units; its four waves share the row tiles, so the weights are streamed once per 320 rows.  No LDS, no
 * atomics: a pure function of the inputs.  Bounds (SVSR_ERR_ARG): Ep, Up multiples of 64 in [64, 4096]; 1 <= U <= Up; 1 <= R <= 65536;
 * x_pitch >= Ep and a multiple of 8; wpk, x, h_prev 16-byte aligned. */
int svsr_rnn_cell_step(int gru, const void* wpk, const float* bias, const void* x, int64_t x_pitch, int x_rows, const int64_t* xidx, int64_t xidx_stride, const float* h_prev, const float* c_prev, const int64_t* src, int prev_rows, float* h_out, float* c_out, void* h16_out, int R, int Ep, int Up, int U, hipStream_t stream);

/* ---- dense temporal back-end of the DC-TCN word-level model (dctcn.hip; syncvsr_amd/dctcn.py, eval path) ---------------------
 * Replaces DenseTemporalConvNet.forward (reference LRW/video/src/tcn/models/densetcn.py:38-192, se_module.py:8-23) and the consensus of
 * DCTCNLightningModule.forward (lightning.py:278-279).  Activations are channels-last bf16 rows [B*T][pitch]; a layer reads the first n_in
 * channels of a row and writes its channels at an offset, so a dense block's `torch.cat(features, 1)` is one buffer and never a copy.
 *
 * svsr_tconv_fwd: nb (1..3) dilated temporal convolutions of the same rows in one launch.  `branches` is a HOST table of nb x 8 64-bit
 * words, read during the call only: {k, w, gate, scale, shift, slope, out_off, res_off} — k odd in 1..7; w bf16 [co][k][n_in] (tap-major
 * within an output channel); gate fp32 [B][n_in] or 0; scale / shift fp32 [co] (BatchNorm(eval) and the conv bias folded: the bf16
 * weights stay unscaled); slope fp32 [co] (act 3 only).  For branch i, row (b, t), channel c < co:
 *   y = act(scale[c] * sum_{j < k} sum_{ci < n_in} bf16(gate[b][ci] * x[b][t + (j - (k-1)/2) * d][ci]) * w[c][j][ci] + shift[c])
 *   out[b*T + t][out_off + c] = bf16(res ? res_act(y + res[b*T + t][res_off + c]) : y)
 * with rows outside [0, T) of the SAME clip contributing zero ("same" padding per clip: Conv1d(padding = (k-1)d) + symmetric Chomp1d);
 * fp32 accumulation on MFMA; act: 0 none, 1 ReLU, 2 Swish, 3 PReLU; res_act: 0 none, 2 Swish; res bf16 rows of res_pitch.  out may be the
 * buffer x points into when the written channels lie behind n_in.  Taken: any B, T >= 1; n_in a multiple of 64 (>= 64); co a multiple of
 * 64; d >= 1 with (k - 1) * d / 2 <= 16; x and w 16-byte aligned, x_pitch a multiple of 8.  Anything else: SVSR_ERR_ARG.
 *
 * svsr_tcn_se_fwd: the nb squeeze-and-excitation gates of a layer: m = mean over t of x[b][t][:n_in] (computed once), gate[i][b] =
 * sigmoid(W2_i swish(W1_i m)); w1 bf16 [nb][R][n_in], w2 bf16 [nb][n_in][R], gate fp32 [nb][B][n_in]; R a multiple of 4, n_in a multiple
 * of 64 up to 8192.
 *
 * svsr_tcn_norm_pool_fwd: h bf16 [B*T][C] = x * scale + shift (norm5); pooled bf16 [B][C] = sum_t h * mask[b][t] / (sum_t mask[b][t] + 1e-6)
 * over the stored h, mask fp32 [B][T]; C a multiple of 8. */
int svsr_tconv_fwd(const void* x, int64_t x_pitch, int B, int T, int n_in, int d, int nb, const int64_t* branches, int co, int act, void* out, int64_t out_pitch, const void* res, int64_t res_pitch, int res_act, hipStream_t stream);
int svsr_tcn_se_fwd(const void* x, int64_t x_pitch, int B, int T, int n_in, int R, int nb, const void* w1, const void* w2, float* gate, hipStream_t stream);
int svsr_tcn_norm_pool_fwd(const void* x, int64_t x_pitch, int B, int T, int C, const float* scale, const float* shift, const float* mask, void* h, void* pooled, hipStream_t stream);

/* ---- backward of the dense temporal back-end (dctcn.hip; DCTCNLightningModule.loss_and_backend_grads) ------------------------
 * The statistics mode of the forward: running-statistic BatchNorm, no dropout.  Gradient rows are channels-last bf16 [B*T][pitch]; parameter
 * gradients and per-channel sums are fp32.  No atomics: one writer per element and launch, every sum in one fixed order (two runs: same bits).
 *
 * svsr_tconv_fwd_save: svsr_tconv_fwd (same arguments, same output bits) that also stores the fp32 accumulator of every written element:
 * acc[b*T + t][i * co + c] for branch i, acc_pitch >= nb * co.  The backward recomputes z = scale * acc + shift from it with the forward's fma;
 * nothing is recovered by dividing by scale and no activation is inverted.
 *
 * svsr_tconv_epi_bwd: the epilogue's backward over C channels (a multiple of 64) of `rows` rows.  z = scale[c] * acc + shift[c], y = act(z);
 * with res: u = y + res, du = dy * res_act'(u), dres = bf16(du); without: du = dy.  g = du * act'(z); dacc = bf16(g * scale[c]).
 * sums fp32 [4][C] = per channel the sums over the rows of g, g * acc, du * min(z, 0) (PReLU slope gradient; 0 otherwise) and du (0 without
 * res): first per block of 64 rows into part (fp32, 4 * C * ceil(rows / 64)), then folded in block order.  dy, dacc, dres, res are passed
 * at their first channel, with their pitches.  The host turns the sums into d bn.weight, d bn.bias, d conv.bias with O(C) operations.
 *
 * svsr_tconv_dgrad: data gradient of nb (1..3) branches in one launch, on MFMA with the forward's staged slab.  `branches` is a HOST table of
 * nb x 4 64-bit words {k, wt, gate, dy_off}: wt bf16 [n_out][k][co] with wt[ci][j][c] = w[c][k-1-j][ci] (transposed, taps flipped); gate fp32
 * [B][n_out] or 0; dy_off the first channel of the branch's dacc in a dy row.
 *   dxg_i[b][t][ci] = sum_j sum_c dy[b][t + (j - (k-1)/2) d][dy_off + c] * wt[ci][j][c]      (rows outside the clip contribute zero)
 *   out[b*T + t][ci] = bf16(addend + cadd[b][ci] * cadd_scale + sum_i (gate_i ? gate_i[b][ci] : 1) * dxg_i)     (one write; addend, cadd optional;
 *   addend may be out itself)
 *   gpart[i][b][tile][ci] = sum over the 32-row time tile of x[b][t][ci] * dxg_i   (gated branches only; x bf16 rows of x_pitch)
 * Same shape domain as svsr_tconv_fwd with co and n_out exchanged for n_in and co; anything else SVSR_ERR_ARG.
 *
 * svsr_tconv_wgrad: one branch's weight gradient dw[c][ci][j] (the parameter's own [co][n_valid][k] layout, ci < n_valid <= n_in)
 *   = (add ? dw : 0) + sum_{b,t} dy[b][t][c] * bf16(x * gate)[b][t + (j - (k-1)/2) d][ci], fp32 on MFMA over the rows; gate fp32 [B][n_in] or
 * null; the rows are split `splits` ways (1 .. ceil(B * ceil(T/32) / 2)), part fp32 [splits][co][k][n_in] is folded in split order.
 *
 * svsr_tcn_se_bwd: from the gate partials of svsr_tconv_dgrad through sigmoid(W2 swish(W1 m)): dm fp32 [B][n_in] (gradient of the time mean,
 * summed over the branches; dm / T belongs to every row: svsr_tconv_dgrad's cadd) and the weight gradients, written (or added, `add`) to the
 * 2 * nb fp32 pointers of the HOST table dw = {dW1_0 .. , dW2_0 ..} ([R][n_in] and [n_in][R]); sums over clips in clip order.  work: fp32
 * scratch of nb*B*n_in + 2*nb*B*R + B*n_in floats.  n_in up to (64 KiB - 8 R) / 24 channels.
 *
 * svsr_tcn_norm_pool_bwd: g = dh[b][t][c] + dpooled[b][c] * mask[b][t] / (sum_t mask + 1e-6); dx = bf16(g * scale[c]) (rows of dx_pitch);
 * sums fp32 [2][C] = the sums over all rows of g and g * x (x: the forward's input), per clip into part (fp32 [B][2][C]) then in clip order.
 *
 * svsr_tcn_fold: out[i] = (add ? out[i] : 0) + sum_r part[r * n + i], r ascending. */
int svsr_tconv_fwd_save(const void* x, int64_t x_pitch, int B, int T, int n_in, int d, int nb, const int64_t* branches, int co, int act, void* out, int64_t out_pitch, const void* res, int64_t res_pitch, int res_act, float* acc, int64_t acc_pitch, hipStream_t stream);
int svsr_tconv_epi_bwd(const void* dy, int64_t dy_pitch, const float* acc, int64_t acc_pitch, int64_t rows, int C, int act, const float* scale, const float* shift, const float* slope, const void* res, int64_t res_pitch, int res_act, void* dacc, int64_t dacc_pitch, void* dres, int64_t dres_pitch, float* part, float* sums, hipStream_t stream);
int svsr_tconv_dgrad(const void* dy, int64_t dy_pitch, int B, int T, int co, int d, int nb, const int64_t* branches, int n_out, const void* x, int64_t x_pitch, const void* addend, int64_t add_pitch, const float* cadd, float cadd_scale, void* out, int64_t out_pitch, float* gpart, hipStream_t stream);
int svsr_tconv_wgrad(const void* x, int64_t x_pitch, const float* gate, const void* dy, int64_t dy_pitch, int B, int T, int n_in, int co, int k, int d, int splits, float* part, float* dw, int n_valid, int add, hipStream_t stream);
int svsr_tcn_se_bwd(const void* x, int64_t x_pitch, int B, int T, int n_in, int R, int nb, const void* w1, const void* w2, const float* gate, const float* gpart, float* work, float* dm, const int64_t* dw, int add, hipStream_t stream);
int svsr_tcn_norm_pool_bwd(const void* dh, const void* dpooled, const void* x, int64_t x_pitch, int B, int T, int C, const float* scale, const float* mask, void* dx, int64_t dx_pitch, float* part, float* sums, hipStream_t stream);
int svsr_tcn_fold(const float* part, int rows, int64_t n, float* out, int add, hipStream_t stream);

/* ---- batch-statistic stages of the dense temporal back-end (dctcn.hip; loss_and_backend_grads(train_stats=True)) --------------
 * The reference's TemporalConvLayer is Conv1d(padding = (k-1)d) -> BatchNorm1d -> symmetric chomp -> activation: in training mode a
 * branch's statistics run over T + (k-1)d positions a clip.  A stage is convolution -> statistics -> apply on the EXTENDED axis: with
 * h_i = (k_i - 1) d / 2 <= hmax <= 16 a clip owns T + 2 hmax rows, time t is row t + hmax, branch i owns rows [hmax - h_i, hmax + h_i + T).
 * `h` is a HOST table of nb ints (the h_i); C = nb * co; channels [i * co, (i + 1) * co) are branch i's.
 *
 * svsr_tconv_fwd_ext: svsr_tconv_fwd's convolution (same table; k, w, gate are read) at every own row of every branch: fp32 accumulators
 *   acc [B * (T + 2 hmax)][acc_pitch], no activation row.  Rows outside a branch's extent are neither written nor read by anything.
 * svsr_tcn_colstats: stats fp32 [2][C] = per channel (mean, sum (x - mean)^2) over the B * (T + 2 h_i) own rows of x (fp32, or bf16 with
 *   is_bf16): per clip a mean and the squares against it, clips merged in order with Chan's update.  part: fp32 scratch [B][2][C].
 * svsr_tconv_apply: k_tconv's epilogue on the T interior rows: z = fma(acc, scale, shift), activation, dropout (drop_p > 0: element
 *   row * C + c kept iff drop_keep(drop_key, p * 2^32, .), kept values times 1 / (1 - p); B * T * C <= 2^32 with drop_p > 0, the index being a
 *   32-bit counter), + res, res_act -> out bf16 [B * T][out_pitch].
 * svsr_tconv_epi_bwd_bs: pass 1 of the backward, svsr_tconv_epi_bwd's sums [4][C] and dres over the interior rows with the mask in the chain
 *   (no dacc).  part: fp32 scratch [ceil(B T / 64)][4][C].
 * svsr_tconv_bn_bwd: pass 2, dacc bf16 [B * (T + 2 hmax)][dacc_pitch] = scale * (g - ca - xhat * cb) on a branch's own rows (g recomputed on
 *   interior rows, 0 on chomped ones; xhat = (acc - mean) * invstd), zeros on the others.
 * svsr_tconv_dgrad_ext / svsr_tconv_wgrad_ext: svsr_tconv_dgrad / svsr_tconv_wgrad over such gradient rows (hmax = 0: the same launch).
 * svsr_tcn_norm_pool_bwd_bs: svsr_tcn_norm_pool_bwd's dx with norm5's batch statistics in the chain (no sums). */
int svsr_tconv_fwd_ext(const void* x, int64_t x_pitch, int B, int T, int n_in, int d, int nb, const int64_t* branches, int co, int hmax, float* acc, int64_t acc_pitch, hipStream_t stream);
int svsr_tcn_colstats(const void* x, int64_t pitch, int is_bf16, int B, int T, int C, int co, int hmax, int nb, const int* h, float* part, float* stats, hipStream_t stream);
int svsr_tconv_apply(const float* acc, int64_t acc_pitch, int B, int T, int C, int co, int hmax, int nb, const int* h, int act, const float* scale, const float* shift, const float* slope, const void* res, int64_t res_pitch, int res_act, unsigned drop_key, float drop_p, void* out, int64_t out_pitch, hipStream_t stream);
int svsr_tconv_epi_bwd_bs(const void* dy, int64_t dy_pitch, const float* acc, int64_t acc_pitch, int B, int T, int C, int co, int hmax, int nb, const int* h, int act, const float* scale, const float* shift, const float* slope, const void* res, int64_t res_pitch, int res_act, unsigned drop_key, float drop_p, void* dres, int64_t dres_pitch, float* part, float* sums, hipStream_t stream);
int svsr_tconv_bn_bwd(const void* dy, int64_t dy_pitch, const float* acc, int64_t acc_pitch, int B, int T, int C, int co, int hmax, int nb, const int* h, int act, const float* scale, const float* shift, const float* slope, const void* res, int64_t res_pitch, int res_act, unsigned drop_key, float drop_p, const float* mean, const float* invstd, const float* ca, const float* cb, void* dacc, int64_t dacc_pitch, hipStream_t stream);
int svsr_tconv_dgrad_ext(const void* dy, int64_t dy_pitch, int B, int T, int co, int d, int nb, const int64_t* branches, int n_out, const void* x, int64_t x_pitch, const void* addend, int64_t add_pitch, const float* cadd, float cadd_scale, void* out, int64_t out_pitch, float* gpart, int hmax, hipStream_t stream);
int svsr_tconv_wgrad_ext(const void* x, int64_t x_pitch, const float* gate, const void* dy, int64_t dy_pitch, int B, int T, int n_in, int co, int k, int d, int splits, float* part, float* dw, int n_valid, int add, int hmax, hipStream_t stream);
int svsr_tcn_norm_pool_bwd_bs(const void* dh, const void* dpooled, const void* x, int64_t x_pitch, int B, int T, int C, const float* scale, const float* mean, const float* invstd, const float* ca, const float* cb, const float* mask, void* dx, int64_t dx_pitch, hipStream_t stream);

/* ---- multi-clip beam search (lrs_search.hip; BatchBeamSearch.forward_clips of syncvsr_amd/lrs_infer.py) -----------------
 * C clips advance through one search in lock step.  The n live hypotheses are rows grouped by clip: clip_of int32 [n] is non-decreasing,
 * clip c owns rows row_lo[c] .. row_lo[c + 1] - 1 (row_lo int32 [C + 1]; an empty range: the clip has finished).
 *
 * svsr_beam_select: the selection of one search position (batch_beam_search.py:146-158 per clip), two launches.  Planes s0 .. s(nplanes-1)
 * fp32 [n][ldv] with weights w0 .., run fp32 [n].  total[r][v] = ((((0 + w0 * s0[r][v]) + w1 * s1[r][v]) + ...) + run[r]), every product
 * and sum rounded on its own (no FMA): bit for bit what `weighted = zeros; weighted += w_k * s_k; ...; weighted += run[:, None]` gives.
 * Per clip the k_c = min(beam, rows_c * V) best (r, v) are written, best first, at output rows out_off[c] .. out_off[c] + k_c - 1
 * (out_off int32 [C]; the caller knows rows_c and lays the outputs out compactly): prev int64 (global row r), tok int64 (v), total fp32,
 * vals fp32 [nplanes][out_rows] (each plane's value at the winner), clip_out int32 (= clip_of[r]); count int32 [C] = k_c.  Order: higher
 * total first, ties to the lower (row, token); NaN sorts above everything (torch.topk's rule).  The result is a pure function of the
 * inputs: no atomics, no dependence on arrival.  max_rows >= the rows of the largest clip.  cand: workspace of
 * C * svsr_beam_select_slices(V, beam, max_rows) * beam 64-bit words.  Bounds (SVSR_ERR_ARG; svsr_beam_select_slices returns 0):
 * nplanes <= 4, beam <= 256, max_rows * V <= 2^20, and slices * beam <= 4096 with slices = ceil(max_rows * V / 4096) — beam 40 over 5,049
 * units holds up to 82 rows per clip, the search never has more than `beam`.
 *
 * svsr_ctc_prefix_score_clips: svsr_ctc_prefix_score (the same kernel) with logp fp32 [C][Tmax][ldp], tlen int32 [C], r_prev fp32 [n][Tmax][2]: hypothesis r
 * walks the tlen[clip_of[r]] frames of its clip's posteriors, eos takes logaddexp of r_prev at that clip's last frame, frames
 * tlen .. Tmax - 1 of r_new [n][S][Tmax][2] are -1e10, and nothing reads logp or r_prev beyond a clip's length.  A row whose clip is
 * outside [0, C) or has no frame, and a candidate outside [0, V), score -1e10.
 *
 * svsr_mha_src_step_fwd: source attention of one query row per hypothesis: q bf16 [n] rows of q_pitch (H * 64 read), kv bf16
 * [C * Tmax] rows of kv_pitch = k | v (2 * H * 64 read) projected once per clip; row r attends to rows clip_of[r] * Tmax + [0, tlen[clip]);
 * softmax in fp32 (scores * scale); ctx bf16 [n] rows of ctx_pitch.  One wave per (row, head); it gathers tlen * 256 bytes.
 *
 * svsr_ctc_align: CTC forced alignment (Viterbi) of B clips, what `CTC.forced_align_batch` (ctc.py:246-328) computes, one workgroup per
 * clip.  logp fp32 log-probabilities [B][Tmax][ldp] (ldp >= V; columns >= V and rows >= tlen[b] are never read), tlen int32 [B], labels
 * int64 [B][Lmax] padded with -1 at the tail (as for svsr_ctc_fwd; anything else in front of the tail is a label).  States
 * ext = [blank, y1, blank, ..., yL, blank]; d[0][0] = logp[0][blank], d[0][1] = logp[0][y1];
 * d[t][s] = best(d[t-1][s], d[t-1][s-1], d[t-1][s-2]) + logp[t][ext[s]] with s-2 only for odd s >= 3 with ext[s] != ext[s-2], the
 * candidates compared in that order with strict > (the first maximum wins), one fp32 add per cell; the end state is the larger of
 * d[tlen-1][S-2] and d[tlen-1][S-1], S-2 on a tie.  Outputs: frames int32 [B][Tmax] the token of every frame (blank for blank states, -1
 * for t >= tlen[b]); spans int32 [B][Lmax][2] first and last frame of every label's state (-1, -1 for l >= L_b); score fp32 [B] the d of
 * the end state.  bp: workspace of B * Tmax * (2 Lmax + 1) bytes (one back-pointer per cell).  A clip without a path — tlen < L + (adjacent
 * equal labels), tlen <= 0, L = 0, a label outside [0, V) (as the 64-bit value it is) or equal to blank, a best path of -inf — gets score
 * -inf and frames = spans = -1, and nothing of logp is read through such a label.  No atomics; the result is a pure function of the inputs
 * and equals the reference's, value for value.  Bounds (SVSR_ERR_ARG): 2 Lmax + 1 <= 2048 and 12 (2 Lmax + 1) + 2 Tmax <= 65536 bytes of
 * LDS.  A chain of tlen dependent steps per clip: latency, not throughput.
 *
 * svsr_ctc_frame_best + svsr_ctc_collapse: CTC best-path (greedy) decoding of C clips, what `CTC.argmax` (ctc.py:172) and the host
 * `groupby` that follows it compute, from the LOGITS of ctc_lo: no [C][Tmax][V] log-softmax is ever stored.
 * svsr_ctc_frame_best: logits fp32 [C * Tmax][ldp] (ldp >= V; what svsr_linear_fwd writes with an fp32 output of that pitch), tlen int32
 * [C].  Row (c, t) with t < tlen[c]: best int32 = the column of the largest logit, the lowest column on a tie, the first NaN if there is
 * one (torch.argmax's rule); best_logp fp32 = logits[best] - logsumexp(logits[0 .. V)), the logsumexp in fp32 around the row maximum (NaN
 * for a row that holds a NaN or nothing but -inf).  Rows t >= tlen[c] get best = -1 and best_logp = 0.  Columns >= V and rows t >= tlen[c]
 * are never read.  One wave per row, one pass carrying (max, column, rescaled sum), 16-byte loads where the rows are 16-byte aligned (logits
 * aligned and ldp % 4 == 0; single loads otherwise), a fixed butterfly over the 64 lanes: no atomics, a pure function of the inputs.
 * HBM-bound by construction: it reads rows * V * 4 bytes once and writes 8 bytes per row, about 1.25 exp per element and no contraction.
 * Bounds (SVSR_ERR_ARG): V >= 1, ldp >= V, C >= 1, Tmax >= 1, C * Tmax < 2^31.
 * svsr_ctc_collapse: best / best_logp [C][Tmax] as written above (any int32 winners), blank any id.  A run is a maximal stretch of equal
 * best over frames 0 .. tlen[c] - 1; every run whose value is not blank is one token, in frame order: tokens int64 [C][Lcap] its id, spans
 * int32 [C][Lcap][2] its first and last frame, token_logp fp32 [C][Lcap] the fp32 sum of best_logp over the run in frame order divided by
 * the run length (one correctly rounded division).  ntok int32 [C] = the number of tokens (0: an all-blank clip is an empty transcript);
 * rows l >= ntok[c] hold tokens -1, spans (-1, -1), token_logp 0.  score fp32 [C] = the fp32 sum of best_logp over the clip's frames in
 * frame order, the log-probability of the best path.  tlen[c] <= 0: ntok = 0, score = 0.  Lcap is the row capacity of the three token
 * outputs (Tmax always suffices); no row l >= Lcap is written, ntok counts them all the same.  One workgroup per clip, token positions
 * from a flag per frame and a workgroup prefix sum: no atomics, nothing depends on arrival.  Bounds (SVSR_ERR_ARG): Tmax <= 4096 (the
 * clip's winners and log-probabilities live in 8 Tmax bytes of LDS), Lcap >= 1, C >= 1.  A few short dependent chains per clip: latency,
 * not throughput. */
int svsr_beam_select_slices(int V, int beam, int max_rows);
int svsr_beam_select(const float* s0, const float* s1, const float* s2, const float* s3, float w0, float w1, float w2, float w3, int nplanes, int64_t ldv, const float* run, const int* clip_of, const int* row_lo, const int* out_off, int n, int C, int V, int beam, int max_rows, int out_rows, void* cand, int64_t* prev, int64_t* tok, float* total, float* vals, int* clip_out, int* count, hipStream_t stream);
int svsr_ctc_prefix_score_clips(const float* logp, int ldp, const float* r_prev, const int64_t* last, const int64_t* ids, const int* clip_of, const int* tlen, float* r_new, float* psi, int C, int Tmax, int V, int n, int S, int out_len, int blank, int eos, hipStream_t stream);
int svsr_ctc_align(const float* logp, int ldp, const int* tlen, const int64_t* labels, int Lmax, int B, int Tmax, int V, int blank, unsigned char* bp, int* frames, int* spans, float* score, hipStream_t stream);
int svsr_ctc_frame_best(const float* logits, int64_t ldp, const int* tlen, int C, int Tmax, int V, int* best, float* best_logp, hipStream_t stream);
int svsr_ctc_collapse(const int* best, const float* best_logp, const int* tlen, int C, int Tmax, int Lcap, int blank, int64_t* tokens, int* spans, float* token_logp, int* ntok, float* score, hipStream_t stream);
int svsr_mha_src_step_fwd(const void* q, int64_t q_pitch, const void* kv, int64_t kv_pitch, const int* clip_of, const int* tlen, int C, int Tmax, int n, int H, float scale, void* ctx, int64_t ctx_pitch, hipStream_t stream);

/* ---- scoring of decoded transcripts (lrs_eval.hip) -----------------------------------------------------------------
 * svsr_edit_distance: Levenshtein distance of N (hypothesis, reference) pairs and its split into substitutions, deletions and insertions:
 * what the reference's test_step asks of torchaudio.functional.edit_distance (LRS/video/lightning.py:17-20,127), for a whole batch, an
 * n-best list or a validation step at once.  hyp int64 [N] rows of ldh ids, ref int64 [N] rows of ldr ids (row strides in ids), hyp_len /
 * ref_len int32 [N]; out int32 [N][4] = distance, substitutions, deletions, insertions.  Ids are compared on all 64 bits and may be
 * anything (token ids, interned words, code points).  A length is cut to [0, min(row stride, 1024)] and nothing behind it is read.
 * Definition: a cell holds (cost, S, D, I); cell(0,0) is all zero; cell(i,0) is i insertions (hypothesis ids with nothing to match);
 * cell(0,j) is j deletions; for i, j >= 1 the candidates are, in priority order, (1) the diagonal cell(i-1,j-1) plus one substitution unless
 * hyp[i-1] == ref[j-1], (2) a deletion from cell(i,j-1), (3) an insertion from cell(i-1,j); the smallest cost wins, a tie goes to the earlier
 * candidate, and the counts travel with the chosen predecessor.  out is cell(hyp_len, ref_len).  So cost is the textbook distance,
 * S + D + I == cost and hyp_len == ref_len - D + I, with no back-pointer matrix and nothing that depends on arrival: integer arithmetic, no
 * atomics, no LDS.  One wave per pair: lane l keeps K = ceil(ref_len / 64) consecutive columns (ids and the cells above) in registers, the
 * lanes sweep the rows skewed by one row per lane and hand the strip's last cell and the row's hypothesis id one lane up, so a pair takes
 * hyp_len + (ref_len - 1) / K <= hyp_len + 63 steps of K cells.  Bounds (SVSR_ERR_ARG): N >= 1, ldh, ldr >= 0.  A dependent chain per pair:
 * latency, not throughput. */
int svsr_edit_distance(const int64_t* hyp, int64_t ldh, const int* hyp_len, const int64_t* ref, int64_t ldr, const int* ref_len, int N, int* out, hipStream_t stream);

/* ---- native step enqueuer (steplist.hip; host code, launches nothing of its own) -----------------------------------
 * Stands where the reference's per-step host loop stands (pl.Trainer.fit -> training_step, LRW/video/src/train.py:23-45,
 * lightning.py:194-202): ONE host call per optimisation step instead of one per launch.  A list records, once, the launch
 * sequence of a training step: CALL = one stream-taking entry point of this header with its arguments frozen (arguments are
 * passed as 64-bit slots: integers sign-extended, floats as the bits of a double, pointers as they are), WAIT = `waiter`
 * waits for everything enqueued so far on `signaller`, MEMSET = hipMemsetAsync, BREAK = segment boundary (the host may issue
 * a collective between two segments).  svsr_steplist_run(list, k, &failed) re-issues segment k (k < 0: every segment) on the
 * recorded streams and returns 0 or the first failing call's code with its op index in *failed.  Every buffer a recorded call
 * points to (device and host) must stay alive and in place while the list exists.  svsr_steplist_knows(name): 1 if the
 * entry point can be recorded.  svsr_stream_wait / svsr_memset_async / svsr_memcpy_async are the eager twins of WAIT / MEMSET / COPY.
 *
 * Op groups (layer drop: whole encoder blocks left out of some replays).  svsr_steplist_push_group(list, n >= 0) opens group n and
 * (list, -1) closes it; every CALL and MEMSET pushed in between belongs to group n (a group may be opened again later: the forward
 * and the backward half of one block).  Groups do not nest (SVSR_ERR_GROUP_OPEN) and hold no BREAK (push_break returns
 * -SVSR_ERR_GROUP_OPEN); a WAIT inside a group is issued whatever is skipped.  svsr_steplist_push_copy(list, dst, src, bytes, stream, g)
 * appends a device-to-device hipMemcpyAsync on `stream` that is issued only in a replay where group g is skipped (g must exist:
 * SVSR_ERR_NO_GROUP; not inside a group).  svsr_steplist_set_skips(list, mask, ngroups): mask[g] != 0 leaves group g out of every
 * following svsr_steplist_run until it is set again; the list keeps a copy; ngroups must be svsr_steplist_groups(list)
 * (SVSR_ERR_MASK_SIZE).  svsr_steplist_calls(list, g): CALL ops of group g (g < 0: of the whole list).  svsr_steplist_last_issued:
 * CALL ops issued since segment 0 (or the whole list) was last run.
 *
 * Gradient accumulation (engine.TrainStep(accumulate = N)) keeps ONE list per batch shape for the three kinds of micro-step: the zero-fill
 * of the gradient buffer and the optimiser tail (sums of squares, AdamW ranges, shadow transposes) are two more groups, numbered behind
 * the layer-drop groups, and the mask of a replay names the skipped groups of both kinds.  The tail group is opened several times (around
 * the early sum of squares inside the backward, and behind the reducer's BREAK).
 * svsr_steplist_dry_run(list, segment, counts): what svsr_steplist_run(list, segment, ..) would issue under the current mask, without
 * issuing anything — counts[4] = {CALL, WAIT, MEMSET, COPY} ops (WAITs are counted, as they are issued, whatever is skipped).  The walk
 * is the one svsr_steplist_run takes; it needs no device (svsr_steplist_push_wait defers making its event to the first run where no
 * device is present). */
void* svsr_steplist_create(void);
int svsr_steplist_destroy(void* list);
int svsr_steplist_knows(const char* name);
int svsr_steplist_push_call(void* list, const char* name, const int64_t* slots, int nslots);
int svsr_steplist_push_wait(void* list, hipStream_t waiter, hipStream_t signaller);
int svsr_steplist_push_memset(void* list, void* ptr, int value, int64_t bytes, hipStream_t stream);
int svsr_steplist_push_break(void* list);
int svsr_steplist_segments(void* list);
int64_t svsr_steplist_size(void* list);
int svsr_steplist_run(void* list, int segment, int* failed);
int svsr_steplist_dry_run(void* list, int segment, int64_t* counts);
int svsr_steplist_push_group(void* list, int group);
int svsr_steplist_push_copy(void* list, void* dst, const void* src, int64_t bytes, hipStream_t stream, int when_skipped);
int svsr_steplist_set_skips(void* list, const uint8_t* mask, int ngroups);
int svsr_steplist_groups(void* list);
int64_t svsr_steplist_calls(void* list, int group);
int64_t svsr_steplist_last_issued(void* list);
int svsr_stream_wait(hipStream_t waiter, hipStream_t signaller);
int svsr_memset_async(void* ptr, int value, int64_t bytes, hipStream_t stream);
int svsr_memcpy_async(void* dst, const void* src, int64_t bytes, hipStream_t stream);

/* Compute units of the current device (persistent kernels size their grids, static tile lists and cluster counts by it). */
int svsr_device_cus(void);

/* Measurement aid: the effective shader clock.  `blocks` workgroups run iters x 4 MFMAs per wave and write {shader cycles (s_memtime),
 * 100 MHz ticks (s_memrealtime)} of that block to out[b][2] (device int64, blocks * 2 + 1 words): MHz = 100 * sum(cycles) / sum(ticks).
 * bench.py reads it before and after its sustained leg (the `sustained` object of its line). */
int svsr_clock_probe(int64_t* out, int blocks, int iters, hipStream_t stream);

/* Test aid (csrc/runtime.hip): a foreign resident kernel — `workgroups` workgroups x 256 threads, each holding lds_bytes of LDS, that sleep
 * until svsr_debug_occupy_stop() (or ~4 s).  Stands in for a peer-waiting collective kernel beside a training step of the reference's
 * strategy="ddp" loop (LRW/video/src/train.py:28): tests/test_gpu_cotenant.py runs steps beside it. */
int svsr_debug_occupy_start(int workgroups, int lds_bytes, hipStream_t stream);
int svsr_debug_occupy_stop(void);

#ifdef __cplusplus
}
#endif
#endif /* SYNCVSR_HIP_H */
