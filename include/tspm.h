/*
 * tspm.h — C ABI of the MI355X-native AVMNIST late-fusion training path (libtspm.so, gfx950).
 *
 * Drop-in boundary for the reference's hot path (TArsenii/task-specific-pretraining-multimodal,
 * MML_Suite; paths below are relative to MML_Suite/).  The reference is pure Python/PyTorch: each
 * entry point here replaces the ATen op family that the cited reference line dispatches.  The
 * Python host side (task-specific-pretraining-multimodal_amd/_lib.py) binds these with ctypes —
 * the stub a maintainer adds to the reference is shown in INTEGRATION.md.
 *
 * Conventions
 *   - Every pointer is a DEVICE pointer unless stated otherwise; sizes are element counts.
 *   - Activations are "HWNC": rows ordered (h, w, n), C contiguous fp32 per row.
 *   - Conv weights are OHWI fp32 (the channels_last view of the reference's OIHW nn.Conv2d weight;
 *     the state_dict keeps shape [O, I, H, W]).
 *   - No entry point allocates, synchronises the host, reads the environment or keeps mutable global state
 *     (ABI 21; tspm_flag_create / _destroy below are the one documented allocating pair); workspace is
 *     caller-provided (size queries provided).  Every call is enqueued on `stream` (a hipStream_t),
 *     so calls are capturable into a hipGraph.
 *   - Return value: TSPM_OK (0) or a TSPM_ERR_* code; nothing is launched on error.
 */
#ifndef TSPM_H_
#define TSPM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* tspm_stream_t; /* hipStream_t */

enum {
  TSPM_OK = 0,
  TSPM_ERR_INVALID = 1,   /* bad shape / null pointer / unsupported configuration */
  TSPM_ERR_LAUNCH = 2,    /* the HIP launch failed (hipGetLastError != hipSuccess) */
  TSPM_ERR_WORKSPACE = 3, /* caller-provided workspace too small */
};

/* Version of this ABI (bumped on any signature change; 18 = round 5: the entry points no step calls removed —
 * tspm_conv_fwd_bnin, tspm_conv_wgrad_t, tspm_conv_dgrad_bnfuse / _bwd_bnfuse / _dgrad_bn_tiles,
 * tspm_bn_bwd_apply / _max_tiles, tspm_debug_barrier_timeouts, tspm_bn1d_bwd_maxout — and the 2x2 LDS tiles;
 * 19 = tspm_bn_bwd_src, the BN backward reading its gradient through a pooling layer's backward, and
 * tspm_bn_apply_maxpool, the stem's apply + ReLU + max pool in one launch, and tspm_set_conv_lds_floor (gone in 21);
 * 20 = tspm_conv_bwd_adam, the fused backward launch carrying an Adam update over earlier-finished parameters,
 * and tspm_head_desc.adam_step; 21 = round 6: no mutable global state and no environment reads inside the library —
 * tspm_set_conv_lds_floor removed, the floor and the hand-off mode are per-call tspm_conv_algo fields, and the
 * head's row block is tspm_head_desc.rows_per_block); 22 = round 6: tspm_conv_algo.variant 4, the LDS-staged kernels with
 * every fp32 product formed from an exact three-piece bf16 split on the bf16 MFMA (same structs and entry points);
 * 23 = tspm_mono_head_step, the monomodal pre-training head (classifier, cross-entropy, predictions, backward) in
 * one launch.  Added under 23 with no existing signature or struct changed (callers built against 23 keep working):
 * tspm_mono_head_bce_step / tspm_mono_head_bce_workspace, the multi-label (BCEWithLogits, F1 counts) form of that
 * head for the MMIMDb encoder pre-training step; tspm_regress_head_step, the scalar-output head of the MOSI / MOSEI
 * sentiment regression (L1 / MSE, backward, epoch accumulators, loss log) in one launch; tspm_lstm_fwd_w /
 * tspm_lstm_bwd_w, the LSTM recurrences at any hidden width that is a multiple of 4 up to 128 (same descriptors);
 * tspm_lstm_fwd_t16 / tspm_lstm_bwd_t16, those recurrences with a 16-bit "maxpool" time index (up to 65535 steps);
 * tspm_lstm_fwd_len / tspm_lstm_bwd_len, the recurrences with per-sample sequence lengths read on the device
 * (pack_padded_sequence semantics; their own descriptors); tspm_textcnn_pool_fwd_len, the TextCNN pooling over each
 * row's own windows (per-sample text lengths read on the device); tspm_adam_begin_multi / tspm_adam_step_multi /
 * tspm_grad_clip_coef_multi, the optimizer phase of a step with up to 8 FusedAdam groups in the launches one group
 * takes; tspm_lstm_bwd_seq, the backward recurrence with a gradient at every step, and tspm_attn_pool_fwd /
 * tspm_attn_pool_bwd, the attention pooling of LSTMEncoder(embd_method="attention"); tspm_pattern_head_train_step /
 * tspm_pattern_head_train_workspace, the AVMNIST fusion head's train step (forward, dropout, cross-entropy, weight
 * backward) over every missing-modality pattern of a batch whose encoders are frozen, in two launches;
 * tspm_embed_gather and tspm_cached_head_train_step / tspm_cached_head_train_workspace, that head stage on a cache of
 * the frozen encoders' embeddings (rows gathered by index; every pattern of the batch or one pattern per sample);
 * tspm_cached_head_train_steps, up to 64 consecutive steps of that stage per host call with Adam applied in the
 * weight-gradient launch; tspm_utt_cache_rows, the UTT-Fusion encoder half read from a cache of the frozen encoders'
 * embeddings and pooled TextCNN features. */
#define TSPM_ABI_VERSION 23
int tspm_abi_version(void);  /* returns TSPM_ABI_VERSION */
/* Static string for a status code. */
const char* tspm_status_string(int status);

/* ------------------------------------------------------------------------------------------------
 * Convolution (implicit GEMM on v_mfma_f32_32x32x2_f32, exact fp32)
 * Replaces nn.Conv2d forward / input-grad / weight-grad at models/msa/networks/resnet.py:25,30
 * (3x3 s1/s2 p1), :137 (7x7 s2 p3 stem, Cin=1) and :176 (1x1 s2 downsample); no bias.
 * ----------------------------------------------------------------------------------------------*/
typedef struct tspm_conv_shape {
  int32_t n, h, w, c;  /* input batch, height, width, channels */
  int32_t k, r, s;     /* output channels, kernel height, kernel width */
  int32_t stride, pad; /* symmetric stride / zero padding */
  int32_t p, q;        /* output height, width (= (h + 2 pad - r) / stride + 1, ...) */
} tspm_conv_shape;

/* Tile / split configuration.  tm, tn: 32x32 MFMA tiles per wave along M (rows) and N (columns).
 * variant 0 — register-direct kernels (operands loaded straight into MFMA fragments): a workgroup
 *   holds wn x wk waves: wn neighbouring column tiles of the same rows and wk waves that split the
 *   reduction of one tile and combine through LDS in fixed order (deterministic, no workspace);
 *   splits: additional split of the wgrad reduction over workgroups (fp32 slabs, summed in slab
 *   order).  Supported: (tm,tn) in {(1,1),(1,2),(2,2)}, wn in {1,2,4}, wk in {1,2,4,8,16},
 *   wn*wk <= 8 when wn > 1, wk == 16 only with wn == 1, at most 160 KiB of LDS for the combine.
 *   All-zero fields select the built-in heuristic.
 * variant 1 — LDS-staged kernels (operand stages fetched in full 128-B lines, double-buffered in
 *   LDS): a workgroup is 4 waves = wm x wn x wk with wm = 4 / (wn*wk); tile (wm*tm*32) x (wn*tn*32);
 *   wk waves split every 32-deep reduction stage; splits: split-K over workgroups for fwd, dgrad
 *   and wgrad (fp32 slabs in the workspace, reduced in slab order in-launch).  tm, tn in {1,2}.
 *   Needs HWNC operands, n % (wm*tm*32) == 0 (fwd/dgrad), c % 32 == 0 (fwd), k % 32 == 0 (dgrad),
 *   n % 32 == 0 and c % (wn*tn*32) == 0 (wgrad); otherwise the call returns TSPM_ERR_INVALID.
 *   The workgroup also carries 4 loader waves that stage each operand stage through registers (3 stages
 *   of loads in flight) into two LDS slots.
 * variant 2 — the same tiles and rules with single-role waves: the 4 waves issue the operand loads
 *   themselves as LDS-DMA into a 2-4-slot ring (faster for the batch-256 / 1024 grids; ABI 15).
 * variant 4 — variant 1's kernels (same tiles, splits, epilogues, fused launches) with every fp32 product formed on
 *   the bf16 matrix cores: the loader waves split each fp32 operand exactly into three bf16 pieces (x = h + m + l,
 *   h = x truncated to bf16, m the remainder truncated, l what is left: at most 8 significant bits each, so exact) and
 *   each 16-deep step of a 32x32 tile is the 9 v_mfma_f32_32x32x16_bf16 of the piece pairs — each product x*w is formed
 *   exactly as the sum of its 9 exact parts in the fp32 accumulator; the sign of the staged A operand and of the
 *   accumulator alternates per stage so the bf16 MFMA's truncating accumulation does not bias long reductions.
 *   wk <= 2 (the waves take whole 16-deep steps).  Round 6, ABI 22.
 * variant 3 — the ResNet stems only (c == 1, 7x7, stride 2, pad 3, k == 64; forward and weight
 *   gradient; the other fields are ignored): a workgroup owns one image and a band of output rows,
 *   stages the band's input rows (and, for the weight gradient, its dy rows) in LDS and runs the band
 *   on MFMA.  The forward's BN partial statistics are per band (tspm_conv_fwd_tiles /
 *   _tile_rows report the band count and rows); the weight gradient reduces per-workgroup slabs in
 *   the workspace after its TSPM_COUNTER_BYTES header (tspm_conv_wgrad_workspace).  Round 4.
 * lds_floor (ABI 21; variants 1 and 2): minimum dynamic LDS in bytes (<= 160 KiB; 0 = none) of this launch — a
 *   floor caps how many of the launch's workgroups share a CU, so a concurrent stream keeps CU room (the step sets
 *   it on the encoder with slack).  Scheduling only: results are bitwise the same.  For tspm_conv_bwd[_adam] the
 *   larger of the two algos' floors applies.  (Replaces ABI 19-20's process-wide tspm_set_conv_lds_floor.)
 * flags (ABI 21): TSPM_ALGO_HANDOFF_ACQUIRE — the split-K / BN-merge last arrivers take an agent-scope acquire
 *   before plain loads instead of reading the write-through payload with sc1 loads (bitwise the same; the
 *   reference side of tests/test_gpu_handoff.py, not a performance option). */
#define TSPM_ALGO_HANDOFF_ACQUIRE 1
typedef struct tspm_conv_algo {
  int32_t tm, tn, wn, wk, splits;
  int32_t variant;
  int32_t lds_floor;
  int32_t flags;
} tspm_conv_algo;

/* Element strides (n, h, w, c) of a conv input tensor.  HWNC tensors: {c, w*n*c, n*c, 1}.
 * The reference's NCHW stem input [N,1,H,W] / [N,H,W]: {h*w, w, 1, 0}. */
typedef struct tspm_strides4 {
  int64_t sn, sh, sw, sc;
} tspm_strides4;

/* BatchNorm statistics produced by the convolution epilogue (BatchNorm2d after every conv,
 * resnet.py:25-26,30-31,137-138,176-177).  partial: 3 planes of [tiles][K] floats (tile shift K,
 * mean offset, M2; tiles and rows per tile from the two queries below).  If counters != NULL the
 * last workgroup to finish each column block merges the partials in-launch (no tspm_bn_finalize
 * launch) and writes save_mean / save_invstd and the running statistics: counters = one uint32 per
 * 32 output channels, zero before first use (left zero after every launch).  With counters == NULL
 * only the partials are written (merge them with tspm_bn_finalize).
 * counters_len / partial_floats (ABI 10; 0 = the sizes above): when they reach
 * tspm_conv_fwd_bn_counters / tspm_conv_fwd_bn_partial_floats, a layer with too many tiles for one
 * merging workgroup is merged in two levels inside the launch (groups of tiles by their group's
 * last workgroup into a second partial array after the first, then the groups by the last group)
 * instead of by a tspm_bn_finalize launch. */
typedef struct tspm_bn_fuse {
  float* partial;
  uint32_t* counters;
  float* running_mean; /* nullable */
  float* running_var;  /* nullable */
  float momentum, eps;
  float* save_mean;
  float* save_invstd;
  int32_t counters_len;
  int32_t reserved_;
  int64_t partial_floats;
} tspm_bn_fuse;

/* y[P,Q,N,K] = conv(x, w).  y is HWNC.  bn: NULL, or the BatchNorm statistics to produce from the
 * epilogue (see tspm_bn_fuse) — the conv output is never re-read for them.  Workspace
 * (tspm_conv_fwd_workspace; nonzero only for variant-1 split-K): TSPM_COUNTER_BYTES of arrival
 * counters, zero before first use and left zero, followed by the fp32 slabs. */
int tspm_conv_fwd(const tspm_conv_shape* shape, const tspm_conv_algo* algo, const float* x,
                  const tspm_strides4* x_strides, const float* w, float* y, const tspm_bn_fuse* bn,
                  void* workspace, size_t workspace_bytes, tspm_stream_t stream);
int32_t tspm_conv_fwd_tiles(const tspm_conv_shape* shape, const tspm_conv_algo* algo);
int32_t tspm_conv_fwd_tile_rows(const tspm_conv_shape* shape, const tspm_conv_algo* algo);
/* Buffer sizes that enable the two-level in-launch BN merge (tspm_bn_fuse.counters_len /
 * partial_floats) for this shape and algo. */
int32_t tspm_conv_fwd_bn_counters(const tspm_conv_shape* shape, const tspm_conv_algo* algo);
int64_t tspm_conv_fwd_bn_partial_floats(const tspm_conv_shape* shape, const tspm_conv_algo* algo);
size_t tspm_conv_fwd_workspace(const tspm_conv_shape* shape, const tspm_conv_algo* algo);

/* Round 6 (ABI 21): two independent LDS-staged forwards in ONE launch — the first 3x3 conv of a downsampling
 * BasicBlock and its 1x1 downsample, which read the same block input (resnet.py:41,50-51).  Each half is exactly
 * tspm_conv_fwd with its own shape, algo, operands, BN fuse and workspace (outputs, BN statistics and running stats
 * bitwise those of the two separate calls); the algos must share (tm, tn, wn, wk, variant) — splits and lds_floor
 * may differ (the launch takes the larger floor).  The two BN fuses need distinct partial / counter buffers and two
 * split-K halves distinct workspaces.  TSPM_ERR_INVALID (nothing launched) when the pair is not supported. */
int32_t tspm_conv_fwd_pair_supported(const tspm_conv_shape* s1, const tspm_conv_algo* a1, const tspm_strides4* xs1,
                                     const tspm_conv_shape* s2, const tspm_conv_algo* a2, const tspm_strides4* xs2);
int tspm_conv_fwd_pair(const tspm_conv_shape* s1, const tspm_conv_algo* a1, const float* x1,
                       const tspm_strides4* xs1, const float* w1, float* y1, const tspm_bn_fuse* bn1, void* ws1,
                       size_t ws1_bytes, const tspm_conv_shape* s2, const tspm_conv_algo* a2, const float* x2,
                       const tspm_strides4* xs2, const float* w2, float* y2, const tspm_bn_fuse* bn2, void* ws2,
                       size_t ws2_bytes, tspm_stream_t stream);

/* dx[H,W,N,C] (HWNC) = beta * dx + conv_input_grad(dy[P,Q,N,K], w), beta in {0, 1}.  Workspace
 * (tspm_conv_dgrad_workspace) only for variant-1 split-K, laid out as for the forward. */
int tspm_conv_dgrad(const tspm_conv_shape* shape, const tspm_conv_algo* algo, const float* dy,
                    const float* w, float* dx, int32_t beta, void* workspace, size_t workspace_bytes,
                    tspm_stream_t stream);
size_t tspm_conv_dgrad_workspace(const tspm_conv_shape* shape, const tspm_conv_algo* algo);

/* dw[K,R,S,C] (OHWI) = conv_weight_grad(x, dy[P,Q,N,K]); overwritten (zero_grad semantics).
 * With splits > 1 the workspace holds TSPM_COUNTER_BYTES of arrival counters followed by the fp32
 * slabs; the last workgroup of each tile sums the slabs in slab order in-launch.  The counter
 * header must be zero before the first call (it is left zero after every call), so one zeroed
 * workspace can serve every wgrad shape. */
#define TSPM_COUNTER_BYTES 65536
int tspm_conv_wgrad(const tspm_conv_shape* shape, const tspm_conv_algo* algo, const float* x,
                    const tspm_strides4* x_strides, const float* dy, float* dw, void* workspace,
                    size_t workspace_bytes, tspm_stream_t stream);
size_t tspm_conv_wgrad_workspace(const tspm_conv_shape* shape, const tspm_conv_algo* algo);

/* Input AND weight gradient of one convolution in ONE launch (both algos variant 1): the dgrad and
 * wgrad implicit GEMMs read the same dy and are independent, and at batch 128 either alone leaves
 * most of the 256 CUs idle, so their workgroups share one grid.  Results are bitwise those of
 * tspm_conv_dgrad(algo_dgrad, beta) + tspm_conv_wgrad(algo_wgrad).  Workspaces as for those two
 * calls, one each (not the same buffer when both algos split).  Only the (dgrad, wgrad) tile pairs
 * built into the library run fused: tspm_conv_bwd_supported() returns 1 for those, 0 otherwise
 * (then call the two entry points; tspm_conv_bwd returns TSPM_ERR_INVALID). */
int32_t tspm_conv_bwd_supported(const tspm_conv_shape* shape, const tspm_conv_algo* algo_dgrad,
                                const tspm_conv_algo* algo_wgrad, const tspm_strides4* x_strides);
int tspm_conv_bwd(const tspm_conv_shape* shape, const tspm_conv_algo* algo_dgrad,
                  const tspm_conv_algo* algo_wgrad, const float* x, const tspm_strides4* x_strides,
                  const float* dy, const float* w, float* dx, int32_t beta, float* dw, void* ws_dgrad,
                  size_t ws_dgrad_bytes, void* ws_wgrad, size_t ws_wgrad_bytes, tspm_stream_t stream);
/* ------------------------------------------------------------------------------------------------
 * BatchNorm2d, training mode (batch statistics over N*H*W, biased variance for normalisation,
 * unbiased for running_var, momentum 0.1, eps 1e-5) — resnet.py:26,31,138,177.
 * ----------------------------------------------------------------------------------------------*/
/* Batch statistics of y[M,C] (M = N*H*W rows).  If nslab > 1, y holds nslab partial slabs
 * (slab_stride elements apart) that are summed in slab order and written to y_out (the conv output
 * used downstream); with nslab == 1, y_out may be NULL or == y.  Writes save_mean / save_invstd [C]
 * and updates running_mean / running_var in place (if non-NULL).  Workspace: tspm_bn_stats_workspace. */
int tspm_bn_stats(int64_t m, int32_t c, const float* y, int32_t nslab, int64_t slab_stride,
                  float* y_out, float* running_mean, float* running_var, float momentum, float eps,
                  float* save_mean, float* save_invstd, void* workspace, size_t workspace_bytes,
                  tspm_stream_t stream);
size_t tspm_bn_stats_workspace(int64_t m, int32_t c);

/* Merge per-tile partial statistics (3 planes of [ntiles][c]: tile shift K, mean-K, M2; tile t
 * holds min(rows_per_tile, m - t*rows_per_tile) rows) into save_mean / save_invstd and the running
 * statistics — the tail of tspm_bn_stats, and the consumer of tspm_conv_fwd's partials when no
 * counters are given. */
int tspm_bn_finalize(int64_t m, int32_t c, int32_t ntiles, int64_t rows_per_tile, const float* partial,
                     float* running_mean, float* running_var, float momentum, float eps, float* save_mean,
                     float* save_invstd, tspm_stream_t stream);

/* out = act( gamma*(y-mean)*invstd + beta  [+ residual] ), act = ReLU if relu != 0.
 * res_mode 0: no residual; 1: residual = res (raw tensor, same [M,C]); 2: residual =
 * BN(res; res_mean, res_invstd, res_gamma, res_beta) — the downsample branch (resnet.py:47-52). */
int tspm_bn_apply(int64_t m, int32_t c, const float* y, const float* mean, const float* invstd,
                  const float* gamma, const float* beta, int32_t res_mode, const float* res,
                  const float* res_mean, const float* res_invstd, const float* res_gamma,
                  const float* res_beta, int32_t relu, float* out, float* out_t, int64_t ld_t,
                  tspm_stream_t stream);

/* Eval-mode BN (running statistics) with the same fusion options. */
int tspm_bn_apply_eval(int64_t m, int32_t c, const float* y, const float* running_mean,
                       const float* running_var, float eps, const float* gamma, const float* beta,
                       int32_t res_mode, const float* res, const float* res_rmean, const float* res_rvar,
                       const float* res_gamma, const float* res_beta, int32_t relu, float* out,
                       tspm_stream_t stream);

/* ABI 17: the encoder's last block apply with the adaptive average pool folded in.  Rows are
 * position-major (row = p*n + sample, npos positions): out = tspm_bn_apply's result over the npos*n rows
 * (tspm_bn_apply_eval's when eval != 0: mean / inv are then the running mean / variance and eps applies),
 * and pooled[n][c] = (sum over p of out) / npos — tspm_avgpool_fwd of out — in the same launch. */
int tspm_bn_apply_pool(int32_t npos, int32_t n, int32_t c, const float* y, const float* mean, const float* inv,
                       const float* gamma, const float* beta, int32_t res_mode, const float* res,
                       const float* res_mean, const float* res_inv, const float* res_gamma, const float* res_beta,
                       int32_t relu, int32_t eval, float eps, float* out, float* pooled, tspm_stream_t stream);

/* Round 6 (ABI 21): the training-mode apply (as tspm_bn_apply) with the statistics merge of tspm_bn_finalize folded
 * into its prologue, for convs whose forward cannot merge its partials in-launch (tspm_conv_fwd_bn_inlaunch == 0;
 * the caller then passes a tspm_bn_fuse without counters so the conv only writes the partials): every workgroup
 * merges the `tiles` (<= 256) partial tiles of its 16 channels in double in a fixed order, row block 0 writes
 * save_mean / save_invstd and updates the running statistics (momentum, unbiased variance), and its rows are
 * normalised.  One launch instead of tspm_bn_finalize + tspm_bn_apply.  c % 16 == 0. */
int32_t tspm_conv_fwd_bn_inlaunch(const tspm_conv_shape* shape, const tspm_conv_algo* algo);
int tspm_bn_apply_merge(int64_t m, int32_t c, int32_t tiles, int64_t rows_per_tile, const float* partial,
                        float* running_mean, float* running_var, float momentum, float eps, float* save_mean,
                        float* save_invstd, const float* y, const float* gamma, const float* beta, int32_t res_mode,
                        const float* res, const float* res_mean, const float* res_invstd, const float* res_gamma,
                        const float* res_beta, int32_t relu, float* out, tspm_stream_t stream);

/* ABI 19: the stem's BN apply + ReLU with the following MaxPool2d(3, 2, 1) in the same launch (resnet.py:138-140):
 * pooled [p][q][n][c] and its argmax taps idx exactly as tspm_maxpool_fwd over tspm_bn_apply's output, and that
 * output out [h][w][n][c] (nullable; the BN backward's ReLU mask) — bitwise the two launches.  eval != 0: inv is
 * the running variance and eps applies (tspm_bn_apply_eval's arithmetic).  p = (h-1)/2+1, q = (w-1)/2+1. */
int tspm_bn_apply_maxpool(int32_t n, int32_t h, int32_t w, int32_t c, const float* y, const float* mean,
                          const float* inv, const float* gamma, const float* beta, int32_t eval, float eps, float* out,
                          float* pooled, uint8_t* idx, int32_t p, int32_t q, tspm_stream_t stream);

/* BN backward through  out = relu(BN(y) [+ BN2(y2)])  (y2 / second BN optional, may be NULL):
 *   g' = g * (out > 0)  (out may be NULL: no ReLU)
 *   dgamma = sum(g' * xhat), dbeta = sum(g')          (written, not accumulated)
 *   dy  = gamma*invstd*(g' - dbeta/M - xhat*dgamma/M)
 *   dy2 likewise for the second BN; if dres != NULL it receives g' (identity residual grad).
 * dy_t / dy2_t (nullable): also write dy / dy2 transposed, [c][ld_t] with the m = (h*W + w)*N + n rows of
 * channel c contiguous (ld_t >= m, ld_t % 4 == 0, 16-byte aligned); no step uses them.
 * Workspace: tspm_bn_bwd_workspace bytes (per-tile partial sums); one workspace must not be used by two
 * launches in flight at once. */
int tspm_bn_bwd(int64_t m, int32_t c, const float* g, const float* out, const float* y,
                const float* mean, const float* invstd, const float* gamma, float* dgamma, float* dbeta,
                float* dy, const float* y2, const float* mean2, const float* invstd2,
                const float* gamma2, float* dgamma2, float* dbeta2, float* dy2, float* dres,
                float* dy_t, float* dy2_t, int64_t ld_t, void* workspace, size_t workspace_bytes,
                tspm_stream_t stream);
size_t tspm_bn_bwd_workspace(int64_t m, int32_t c);
/* ABI 19: the same BN backward with its incoming gradient g formed on the fly from a pooling layer's output
 * gradient instead of read from a materialised [m, c] tensor (one launch and the g tensor's write + reads fewer):
 *   kind TSPM_GSRC_AVGPOOL — the encoder's AdaptiveAvgPool2d(1) + flatten (resnet.py:59-60): g[(pos, n)] =
 *     gp[n * ldg + c] / npos, exactly tspm_avgpool_bwd's value (npos = h * w);
 *   kind TSPM_GSRC_MAXPOOL — the stem's MaxPool2d(3, 2, 1) (resnet.py:140): g = tspm_maxpool_bwd's dx from gp
 *     [p][q][n][c] and its argmax taps idx (same window order, bitwise).
 * Rows m = h * w * n (HWNC) < 2^24.  Otherwise as tspm_bn_bwd without the transposed copies. */
enum { TSPM_GSRC_AVGPOOL = 1, TSPM_GSRC_MAXPOOL = 2 };
typedef struct tspm_bn_gsrc {
  int32_t kind;
  int32_t n, h, w;     /* the BN input map: m = h * w * n rows */
  int32_t p, q;        /* maxpool: the pooled map */
  int32_t npos, ldg;   /* avgpool: positions (= h * w) and the row stride of gp [n][ldg] */
  const float* gp;     /* the pooling layer's output gradient */
  const uint8_t* idx;  /* maxpool: argmax taps [p][q][n][c] (tspm_maxpool_fwd) */
} tspm_bn_gsrc;
int tspm_bn_bwd_src(int64_t m, int32_t c, const tspm_bn_gsrc* src, const float* out, const float* y,
                    const float* mean, const float* invstd, const float* gamma, float* dgamma, float* dbeta,
                    float* dy, const float* y2, const float* mean2, const float* invstd2, const float* gamma2,
                    float* dgamma2, float* dbeta2, float* dy2, float* dres, void* workspace, size_t workspace_bytes,
                    tspm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Pooling — nn.MaxPool2d(3, 2, 1) (resnet.py:140,208) and AdaptiveAvgPool2d(1)+flatten (:149,215-216)
 * ----------------------------------------------------------------------------------------------*/
/* y[P,Q,N,C] = maxpool(x[H,W,N,C]); argmax tap (0..k*k-1, first max in row-major window order,
 * as ATen's CPU kernel) stored in idx (uint8, same shape as y). */
int tspm_maxpool_fwd(int32_t n, int32_t h, int32_t w, int32_t c, int32_t k, int32_t stride, int32_t pad,
                     int32_t p, int32_t q, const float* x, float* y, uint8_t* idx, float* y_t, int64_t ld_t,
                     tspm_stream_t stream);
/* dx = scatter of dy to the argmax positions (gather form, deterministic); dx overwritten. */
int tspm_maxpool_bwd(int32_t n, int32_t h, int32_t w, int32_t c, int32_t k, int32_t stride, int32_t pad,
                     int32_t p, int32_t q, const float* dy, const uint8_t* idx, float* dx,
                     tspm_stream_t stream);
/* y[N,C] = mean over the npos positions of x[npos,N,C] (HWNC). */
int tspm_avgpool_fwd(int32_t npos, int32_t n, int32_t c, const float* x, float* y, tspm_stream_t stream);
/* dx[npos,N,C] = dy[N,C] / npos (dy row stride ldy). */
int tspm_avgpool_bwd(int32_t npos, int32_t n, int32_t c, const float* dy, int32_t ldy, float* dx,
                     tspm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Linear layers — encoder fc (resnet.py:150,217) and the fusion head (models/avmnist.py:219-230,267)
 * w is [out, in] row-major (nn.Linear layout).  ld* are row strides (elements).
 * ----------------------------------------------------------------------------------------------*/
/* y = act(x @ w^T + b) [* keep*scale]; relu != 0 applies ReLU; keep (uint8 [n,out], may be NULL)
 * applies the dropout mask with scale 1/(1-p) (models/avmnist.py:219-230). */
int tspm_linear_fwd(int32_t n, int32_t in, int32_t out, const float* x, int32_t ldx, const float* w,
                    const float* b, int32_t relu, const uint8_t* keep, float keep_scale, float* y,
                    int32_t ldy, tspm_stream_t stream);
/* tspm_linear_fwd with the reduction split over `splits` workgroup slices (ABI 11): for long inputs
 * with few output tiles (the MMIMDb image encoder, 4096 -> 512 at batch 256: 128 tiles for 256 CUs).
 * Partial products go to the workspace (tspm_linear_fwd_splitk_workspace bytes; 0 = no split needed)
 * and a second launch sums the slices in order and applies the epilogue.  Same results as
 * tspm_linear_fwd up to summation order. */
int tspm_linear_fwd_splitk(int32_t n, int32_t in, int32_t out, const float* x, int32_t ldx, const float* w,
                           const float* b, int32_t relu, const uint8_t* keep, float keep_scale, float* y,
                           int32_t ldy, int32_t splits, void* workspace, size_t workspace_bytes,
                           tspm_stream_t stream);
size_t tspm_linear_fwd_splitk_workspace(int32_t n, int32_t in, int32_t out, int32_t splits);
/* Two bias-free Linear forwards of the same shape in one launch (the GMU's fc_one / fc_two,
 * models/gates/gated_bimodal.py; ABI 11): y0 = x0 @ w0^T, y1 = x1 @ w1^T, bitwise tspm_linear_fwd. */
int tspm_linear_fwd_pair(int32_t n, int32_t in, int32_t out, const float* x0, int32_t ldx0, const float* w0,
                         float* y0, int32_t ldy0, const float* x1, int32_t ldx1, const float* w1, float* y1,
                         int32_t ldy1, tspm_stream_t stream);
/* dx = dy @ w  (dx overwritten). */
int tspm_linear_bwd_data(int32_t n, int32_t in, int32_t out, const float* dy, int32_t ldy, const float* w,
                         float* dx, int32_t ldx, tspm_stream_t stream);
/* dw = dy^T @ x, db = sum_n dy (both overwritten). */
int tspm_linear_bwd_weight(int32_t n, int32_t in, int32_t out, const float* x, int32_t ldx,
                           const float* dy, int32_t ldy, float* dw, float* db, tspm_stream_t stream);
/* tspm_linear_bwd_weight with the reduction over the n rows split into `splits` workgroup slices
 * (ABI 13): for very long reductions with few output tiles (the LSTM weight gradients of the MOSI
 * step, n = T*B = 6400 rows into 256 x 64 / 256 x 5 / 256 x 20 outputs).  Per-slice partial products
 * and row sums go to the workspace (tspm_linear_bwd_weight_splitk_workspace bytes; 0 = no split), a
 * second launch sums the slices in order.  Same results as tspm_linear_bwd_weight up to summation
 * order; dw and db from the same call share one split (an LSTM's db_ih / db_hh stay bitwise equal). */
int tspm_linear_bwd_weight_splitk(int32_t n, int32_t in, int32_t out, const float* x, int32_t ldx, const float* dy,
                                  int32_t ldy, float* dw, float* db, int32_t splits, void* workspace,
                                  size_t workspace_bytes, tspm_stream_t stream);
size_t tspm_linear_bwd_weight_splitk_workspace(int32_t n, int32_t in, int32_t out, int32_t splits);
/* Both backward products of one nn.Linear in ONE launch (ABI 11): dw = dy^T @ x, db = sum_n dy
 * (db nullable), and, if dx != NULL, dx = dy @ w (row stride lddx) — bitwise the results of
 * tspm_linear_bwd_weight + tspm_linear_bwd_data (same per-product reduction split). */
int tspm_linear_bwd(int32_t n, int32_t in, int32_t out, const float* x, int32_t ldx, const float* dy, int32_t ldy,
                    const float* w, float* dw, float* db, float* dx, int32_t lddx, tspm_stream_t stream);
/* Backward of up to 2 independent nn.Linear layers in ONE launch (ABI 11; e.g. the GMU's fc_one and
 * fc_two, or the MMIMDb image and text encoder Linears): each descriptor as tspm_linear_bwd (dx
 * nullable), bitwise its results.  descs is a host array read at launch time. */
typedef struct tspm_linear_bwd_desc {
  int32_t n, in, out, ldx, ldy, lddx;
  const float* x;
  const float* dy;
  const float* w;
  float* dw;
  float* db;
  float* dx;
} tspm_linear_bwd_desc;
int tspm_linear_bwd_multi(int32_t count, const tspm_linear_bwd_desc* descs, tspm_stream_t stream);
/* In-place gradient masking through a ReLU(+dropout) output y: g = (y > 0) ? g * scale : 0
 * (scale = 1/(1-p) when y is the post-dropout output — y > 0 implies the unit was kept). */
int tspm_act_bwd(int32_t n, int32_t cols, float* g, int32_t ldg, const float* y, int32_t ldy, float scale,
                 tspm_stream_t stream);

/* Dropout keep mask (uint8) from a counter-based hash RNG: keep[i] = u(seed, ctr, i) >= p, where
 * ctr is read from device memory (*counter) so graph replays draw fresh masks. */
int tspm_dropout_mask(int64_t count, float p, uint64_t seed, const uint64_t* counter, uint8_t* keep,
                      tspm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Loss — LossFunctionGroup{cross_entropy: 1.0} (experiment_utils/loss.py:123-148,
 * models/avmnist.py:301) + on-device accuracy counters (avmnist.py:305-309)
 * ----------------------------------------------------------------------------------------------*/
/* loss[0] = grad_scale * mean_i CE(logits_i, labels_i) (the group's total: weight × CE, grad_scale =
 * the term's weight); dlogits = (softmax - onehot)/n * grad_scale;
 * if stats != NULL: stats[0] += loss*n, stats[1] += #correct (argmax == label, first maximum), stats[2] += n.
 * A label outside [0, classes) gives a NaN loss and a NaN dlogits row (no out-of-bounds read) and never counts
 * as correct, whatever the row's argmax. */
int tspm_cross_entropy(int32_t n, int32_t classes, const float* logits, const int64_t* labels, float* loss,
                       float* dlogits, float grad_scale, float* stats, tspm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Fusion head train step (ABI 16) — AVMNIST's classifier `net` = Linear(in, hidden) → ReLU →
 * Dropout(p) → Linear(hidden, hidden2) → ReLU → Linear(hidden2, classes) (models/avmnist.py:219-230,
 * forward :267), the LossFunctionGroup's weighted cross-entropy (experiment_utils/loss.py:98-148) and
 * the head's whole backward, in TWO launches instead of ten:
 *   (1) one sample per workgroup (512 threads; round 5 — rows_per_block = 4 selects round 4's blocks of 4
 *       samples on 256 threads), the three weight matrices staged in LDS: dropout keep
 *       mask (same counter-hash bits as
 *       tspm_dropout_mask, or read from `keep` when gen_keep == 0), h1, hh, logits, per-row CE,
 *       dlogits, dz3 = (dlogits @ w5) * (hh > 0), dz0 = (dz3 @ w3) * (h1 > 0 ? 1/(1-p) : 0) and
 *       dx = dz0 @ w0 (the gradient flowing into the two encoders' embeddings);
 *   (2) the three weight / bias gradients (dw = dz^T @ input, db = column sums; overwritten) on the
 *       small-GEMM tiles, plus one workgroup that reduces the per-row losses in a fixed order:
 *       loss[0] = weight * mean CE, stats[0] += sum CE, stats[1] += #(argmax == label), stats[2] += n.
 * Every buffer below is caller-owned device memory; row_ws holds 2*n floats.  Same semantics as
 * tspm_linear_fwd/_bwd + tspm_act_bwd + tspm_dropout_mask + tspm_cross_entropy (out-of-range label →
 * NaN loss and gradients, never counted in stats[1]), up to summation order.  Limits: in <= 256, hidden <= 256, hidden2 <= 128,
 * classes <= 16; in, hidden, hidden2 multiples of 4; w0 / w3 / x rows 16-byte aligned; the three
 * weight matrices plus the row blocks within 160 KiB of LDS (floats, RB = rows per workgroup, logits rows
 * padded to a multiple of 4: hidden*(in+4) + hidden2*(hidden+4) + classes*(hidden2+4)
 * + RB*(in+hidden+hidden2+12+round_up4(classes)) + hidden+hidden2+classes+RB); otherwise TSPM_ERR_INVALID. */
typedef struct tspm_head_desc {
  int32_t n, in, hidden, hidden2, classes, ldx, lddx, gen_keep;
  const float* x;                  /* [n, ldx] the fused embeddings (concat of the two encoders) */
  const float *w0, *b0, *w3, *b3, *w5, *b5;
  float p;                         /* dropout probability (0: no mask) */
  float loss_weight;               /* the cross-entropy term's weight */
  uint64_t seed;
  const uint64_t* counter;         /* device step counter (fresh masks per graph replay) */
  uint8_t* keep;                   /* [n, hidden] */
  const int64_t* labels;           /* [n] */
  float *h1, *hh, *logits, *dlogits, *dz3, *dz0, *dx, *row_ws;
  float *gw0, *gb0, *gw3, *gb3, *gw5, *gb5;
  float *loss, *stats;             /* stats nullable */
  int64_t* adam_step;              /* nullable (ABI 20): the optimizer's tspm_adam_hyper.step, incremented once by
                                    * launch 2 after launch 1 read `counter` (tspm_adam_begin's job, one launch fewer
                                    * between the forward and the backward) */
  int32_t rows_per_block;          /* ABI 21: samples per workgroup of launch 1 — 0 = the default (1 up to 256
                                    * rows, else 4), or 1 / 4 (A/B; was the TSPM_HEAD_RB environment read) */
  int32_t reserved_;
} tspm_head_desc;
int tspm_head_train_step(const tspm_head_desc* desc, tspm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Adam — torch.optim.Adam (L2 weight decay folded into the gradient) as instantiated by
 * config/optimizer_config.py:199-226 with lr 5e-4, wd 1e-4 (train_avmnist_resnet.yaml)
 * ----------------------------------------------------------------------------------------------*/
typedef struct tspm_adam_hyper {
  /* doubles, like torch.optim.Adam's Python-float hyper-parameters: 1-beta2 and the bias
   * corrections are formed in double and rounded to fp32 once, as ATen does */
  double lr, beta1, beta2, eps, weight_decay, grad_scale; /* grad_scale multiplies g (e.g. 1/world) */
  int64_t step;                                          /* incremented on device by tspm_adam_begin */
  int64_t pad_;                                          /* device scratch: tspm_cached_head_train_steps keeps the step
                                                          * in flight here; nothing else reads or writes it */
} tspm_adam_hyper;
/* hyper->step += 1 (device-side, so a captured graph advances the bias correction per replay). */
int tspm_adam_begin(tspm_adam_hyper* hyper, tspm_stream_t stream);
/* counters[i] += value for i < count (ABI 13): every BatchNorm's num_batches_tracked (one shared
 * int64 vector) advanced once per training step inside the captured step. */
int tspm_counters_add(int64_t* counters, int64_t count, int64_t value, tspm_stream_t stream);

/* Step flags (ABI 15) for the DP step's exchange ordering across a graph boundary.  A flag is a device
 * counter plus a word of coherent pinned host memory.  tspm_flag_bump enqueues a one-thread kernel that
 * increments the counter and stores the new value to the host word (system-scope release) — capturable, so
 * it marks a point INSIDE a captured step graph; tspm_flag_host_wait spins on the host until the word is
 * >= value (0 = TSPM_OK; TSPM_ERR_LAUNCH after timeout_ms).  The host then launches work that depends on
 * that point.  (ROCm 7 refuses graph-external event records; a hipStreamWaitValue64 on another stream
 * cost 0.21 ms per step — the waiting queue stalls the graph's.) */
typedef struct tspm_flag tspm_flag;
int tspm_flag_create(tspm_flag** flag);
int tspm_flag_destroy(tspm_flag* flag);
int tspm_flag_bump(tspm_flag* flag, tspm_stream_t stream);
int tspm_flag_host_wait(tspm_flag* flag, uint64_t value, int32_t timeout_ms);
/* One fused Adam update over `count` contiguous fp32 elements (the flat parameter buffer). */
int tspm_adam_step(int64_t count, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                   const tspm_adam_hyper* hyper, tspm_stream_t stream);
/* tspm_adam_step with the gradient also multiplied by the device scalar *clip_coef (ABI 12: the
 * coefficient tspm_grad_clip_coef wrote — torch.nn.utils.clip_grad_norm_ before optimizer.step(),
 * MML_Suite/models/msa/utt_fusion.py:188-190).  g' = (g * grad_scale) * clip_coef. */
int tspm_adam_step_clip(int64_t count, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                        const tspm_adam_hyper* hyper, const float* clip_coef, tspm_stream_t stream);
/* Several FusedAdam groups in one launch each (added under ABI 23): `segs` is a HOST array of `count` segments,
 * 1 <= count <= TSPM_ADAM_MAX_SEGMENTS, copied into the kernel arguments (nothing of it is read after the call
 * returns).  A segment is one group's flat buffers with its own device tspm_adam_hyper (lr, betas, eps, weight decay,
 * grad_scale and step all per segment); a segment with count 0 is empty: its buffers are never touched and may be
 * NULL.  Every non-empty segment needs non-NULL, 16-byte-aligned param / grad / exp_avg / exp_avg_sq and a non-NULL
 * hyper; any violation, a negative count or a count outside 1..8 is TSPM_ERR_INVALID before any launch.
 * tspm_adam_begin_multi: hyper->step += 1 for every segment whose hyper is non-NULL (an empty segment's too), one
 * launch of one thread that takes the segments in order (a hyper named by two segments advances twice).
 * tspm_adam_step_multi: every non-empty segment updated in ONE launch.  Each workgroup belongs to exactly one
 * segment: the host gives a segment cdiv(count/4 + 1, 256) workgroups (tspm_adam_step's grid), scaled down
 * proportionally to about 2048 in total with at least one per non-empty segment, and passes the prefix of that
 * partition in the kernel arguments; a workgroup finds its segment by scanning those <= 8 entries and runs
 * tspm_adam_step's element loop (f32x4 body, scalar tail for count & 3) with that segment's constants.  No atomics,
 * no communication between workgroups, no table in memory.  Adam is element-wise, so each segment's param / exp_avg /
 * exp_avg_sq are bitwise those of tspm_adam_step on it alone — with clip_coef (device scalar, nullable) those of
 * tspm_adam_step_clip.  Segments must not overlap.  With every segment empty the call launches nothing. */
#define TSPM_ADAM_MAX_SEGMENTS 8
typedef struct tspm_adam_seg {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t count;           /* >= 0; 0 = an empty segment, skipped */
  tspm_adam_hyper* hyper;  /* device */
} tspm_adam_seg;
int tspm_adam_begin_multi(int32_t count, const tspm_adam_seg* segs, tspm_stream_t stream);
int tspm_adam_step_multi(int32_t count, const tspm_adam_seg* segs, const float* clip_coef, tspm_stream_t stream);

/* ABI 20: tspm_conv_bwd that also carries an Adam update: `blocks` extra workgroups of the same grid run
 * tspm_adam_step's element loop over `count` elements starting at param / grad / exp_avg / exp_avg_sq (a range of
 * the optimizer's flat buffers whose gradients an EARLIER launch on the stream finished and which no later launch
 * reads), bitwise tspm_adam_step over that range (hyper->step must already be advanced by tspm_adam_begin).  The
 * optimizer pass that follows the backward (MML_Suite train loop: loss.backward(); optimizer.step(),
 * train_multimodal.py) is thereby spread over the backward's latency-bound launches instead of following them.
 * count = 0: plain tspm_conv_bwd. */
typedef struct tspm_adam_job {
  float* param;
  const float* grad;
  float *exp_avg, *exp_avg_sq;
  int64_t count;
  const tspm_adam_hyper* hyper;
  int32_t blocks, pad_;
} tspm_adam_job;
int tspm_conv_bwd_adam(const tspm_conv_shape* s, const tspm_conv_algo* dgrad_algo, const tspm_conv_algo* wgrad_algo,
                       const float* x, const tspm_strides4* x_strides, const float* dy, const float* w, float* dx,
                       int32_t beta, float* dw, const tspm_adam_job* job, void* ws_d, size_t ws_d_bytes, void* ws_w,
                       size_t ws_w_bytes, tspm_stream_t stream);

/* Round 6 (ABI 21): the BatchNorm backward's partial sums formed by the dgrad epilogue that writes its incoming
 * gradient.  In the ResNet backward (resnet.py:37-54 under autograd) the gradient of bn1's output is conv2's input
 * gradient, and the gradient of bn2's output (through the block's ReLU) is the next block's conv1 input gradient
 * accumulated onto the residual branch; the last-arriving workgroup of each dgrad tile holds those values in
 * registers.  With bnp set, tspm_conv_bwd_ex's dgrad epilogue also writes, per 32-row tile t and channel c of dx
 * (after the beta accumulate — dx itself bitwise as without bnp), with g' = dx * [out > 0]:
 *   part[0][t][c] = sum g',  part[1][t][c] = sum g' (y - mean[c]),  part[2][t][c] = sum g' (y2 - mean2[c]) (y2 set)
 * — exactly what tspm_bn_bwd's partial pass computes over its own row tiles, so tspm_bn_bwd_apply_part can run the
 * BN backward's apply (merge + dy) without that pass: one launch fewer per BatchNorm backward.  Needs
 * (h*w*n) % 32 == 0; out, y, y2 are [h*w*n][c] HWNC like dx. */
typedef struct tspm_bn_bwd_part {
  const float* out;    /* the ReLU output that gates the gradient */
  const float* y;      /* the BN's input (its conv output) */
  const float* mean;   /* its save_mean [c] */
  const float* y2;     /* nullable: a second BN fed by the same gradient (the block's downsample branch) */
  const float* mean2;  /* its save_mean [c] */
  float* part;         /* [2 or 3][(h*w*n)/32][c] */
  /* Max-pool gather (nullable idx): dx is the gradient of a MaxPool2d(3, 2, 1) output whose argmax taps are idx
   * ([h][w][n][c] uint8, tspm_bn_apply_maxpool's), and the BN sits before that pool on a pool_h x pool_w map (the
   * ResNet stem, resnet.py:138-140): out / y are read at each pooled element's argmax position, so the sums are the
   * BN backward's over the pool's input-gradient (sum over the map of maxpool_bwd(dx) * [out > 0] ...) formed in
   * the pooled domain — one gathered read per pooled element instead of a pass over the pool's input. */
  const uint8_t* idx;
  int32_t pool_h, pool_w;
  /* Whole BN backward in the same launch (round 6; dy non-null, no idx): the last dgrad tile of each column block
   * to finish (a ticket on counters[column block]: one uint32 per (c / tile columns), zero before first use, left
   * zero) merges that block's partial tiles in tspm_bn_bwd_apply_part's order, writes dgamma / dbeta and applies
   * dy [, dy2] [, dres = g'] over all rows of its channels — tspm_bn_bwd_apply_part's values, no apply launch.
   * dx and the partials are then published write-through (sc1) for it.  Meant for short maps (the tail is one
   * workgroup per column block). */
  const float *invstd, *gamma;
  float *dgamma, *dbeta, *dy;
  const float *invstd2, *gamma2;
  float *dgamma2, *dbeta2, *dy2, *dres;
  uint32_t* counters;
} tspm_bn_bwd_part;
/* tspm_conv_bwd with an optional carried Adam job (as tspm_conv_bwd_adam; nullable) and optional BN-backward
 * partial sums of dx (bnp; nullable). */
int tspm_conv_bwd_ex(const tspm_conv_shape* s, const tspm_conv_algo* dgrad_algo, const tspm_conv_algo* wgrad_algo,
                     const float* x, const tspm_strides4* x_strides, const float* dy, const float* w, float* dx,
                     int32_t beta, float* dw, const tspm_adam_job* job, const tspm_bn_bwd_part* bnp, void* ws_d,
                     size_t ws_d_bytes, void* ws_w, size_t ws_w_bytes, tspm_stream_t stream);
/* Round 6: the backward of a downsampling block's second conv (s, dg, wg: its dgrad + wgrad exactly as
 * tspm_conv_bwd_ex, with the optional bnp) and of the block's 1x1 downsample (s2, dg2, wg2: dgrad with beta 0 into
 * dx2 + wgrad into dw2) in ONE launch — both read gradients the block's bn2 backward has just written and write
 * disjoint tensors (resnet.py:41-51 under autograd).  dg2 / wg2 must have dg / wg's (tm, tn, wn, wk, variant);
 * splits may differ; split-K halves need pairwise distinct workspaces.  job (nullable) as tspm_conv_bwd_adam. */
int32_t tspm_conv_bwd_quad_supported(const tspm_conv_shape* s, const tspm_conv_algo* dg, const tspm_conv_algo* wg,
                                     const tspm_strides4* xs, const tspm_conv_shape* s2, const tspm_conv_algo* dg2,
                                     const tspm_conv_algo* wg2, const tspm_strides4* xs2);
int tspm_conv_bwd_quad(const tspm_conv_shape* s, const tspm_conv_algo* dg, const tspm_conv_algo* wg, const float* x,
                       const tspm_strides4* xs, const float* dy, const float* w, float* dx, int32_t beta, float* dw,
                       const tspm_bn_bwd_part* bnp, void* ws_d, size_t ws_d_bytes, void* ws_w, size_t ws_w_bytes,
                       const tspm_conv_shape* s2, const tspm_conv_algo* dg2, const tspm_conv_algo* wg2,
                       const float* x2, const tspm_strides4* xs2, const float* dy2, const float* w2, float* dx2,
                       float* dw2, void* ws_d2, size_t ws_d2_bytes, void* ws_w2, size_t ws_w2_bytes,
                       const tspm_adam_job* job, tspm_stream_t stream);
/* The BN backward's second launch alone (tspm_bn_bwd's k_bn_bwd_apply_m) over partial sums `part` of `tiles` row
 * tiles ([2 or 3][tiles][c], e.g. from tspm_conv_bwd_ex's bnp; tiles <= 128): every workgroup merges the tiles in
 * double in a fixed order, writes dgamma / dbeta (first row block) and dy = gamma*invstd*(g' - mean(g') -
 * xhat*mean(g' xhat)) [dy2 likewise for y2], dres = g' (nullable).  Arguments otherwise as tspm_bn_bwd with g dense
 * (out required). */
/* tspm_bn_bwd_apply_part with the gradient read through a pooling layer's backward (the stem BN under the max pool:
 * src->kind TSPM_GSRC_MAXPOOL, as tspm_bn_bwd_src), its partial sums from tspm_conv_bwd_ex's max-pool gather mode
 * (tspm_bn_bwd_part.idx); single BN, no dres. */
int tspm_bn_bwd_apply_part_src(int64_t m, int32_t c, int32_t tiles, const float* part, const tspm_bn_gsrc* src,
                               const float* out, const float* y, const float* mean, const float* invstd,
                               const float* gamma, float* dgamma, float* dbeta, float* dy, tspm_stream_t stream);
int tspm_bn_bwd_apply_part(int64_t m, int32_t c, int32_t tiles, const float* part, const float* g, const float* out,
                           const float* y, const float* mean, const float* invstd, const float* gamma, float* dgamma,
                           float* dbeta, float* dy, const float* y2, const float* mean2, const float* invstd2,
                           const float* gamma2, float* dgamma2, float* dbeta2, float* dy2, float* dres,
                           tspm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Layout / data-stage helpers (collate → device, MML_Suite/data/avmnist.py:186-191,248-277)
 * ----------------------------------------------------------------------------------------------*/
/* image_f32[i] = lut[u8[i]] * (1/255)  (gist_earth→L colormap LUT, torchvision ToDtype(scale)). */
int tspm_image_lut(int64_t count, const uint8_t* u8, const uint8_t* lut, float* out, tspm_stream_t stream);
/* Batch assembly from an HBM-resident AVMNIST corpus (replaces, per batch, AVMNIST.__getitem__ +
 * _load_audio/_load_image + get_samples + collate_fn: MML_Suite/data/avmnist.py:164-224,248-277,
 * data/base_dataset.py:61-74).  For r < count, s = index[r]:
 *   audio_out[r,:]  = audio[s,:] * audio_mask[r]                       (audio_elems floats/row)
 *   image_out[r,:]  = (float)lut[image[s,:]] * fp32(1/255) * image_mask[r]  (image_elems bytes/row)
 *   labels_out[r]   = labels[s]
 * A null mask means "no multiply"; a null lut means the identity map; a null output skips that
 * modality (target_modality audio / image only).  An index outside [0, n_samples) writes NaN rows
 * and label -1 (tspm_cross_entropy then yields NaN) instead of reading out of bounds.
 * Fast path (16-byte audio, 4-byte image accesses) when both element counts are multiples of 4 and
 * audio/audio_out/image_out are 16-byte and image/lut 4-byte aligned; otherwise per element. */
int tspm_avmnist_gather(int64_t count, const int64_t* index, int64_t n_samples, const float* audio,
                        int32_t audio_elems, const uint8_t* image, int32_t image_elems, const int64_t* labels,
                        const uint8_t* lut, const float* audio_mask, const float* image_mask, float* audio_out,
                        float* image_out, int64_t* labels_out, tspm_stream_t stream);
/* Classification bookkeeping for one batch, on device (replaces the per-batch softmax → argmax →
 * .cpu() → MetricRecorder.update_group_all of models/avmnist.py:305-309,345-350 and
 * experiment_utils/metric_recorder.py:96-145, and the epoch loops' per-batch loss lists,
 * train_multimodal.py:478-491,525-541).  For r < n:
 *   pred = first argmax of softmax(logits[r,:classes]);  pred_out[r] = pred  (if pred_out)
 *   confusion[g][labels[r]][pred] += 1  with g = groups ? groups[r] : 0  (int64 counts,
 *   [n_groups][classes][classes]; rows whose label or group is out of range are not counted)
 * and once per call, when counters is given: loss_log[counters[0]] = *loss (if loss_log and
 * counters[0] < log_capacity), counters[0] += 1, counters[1] += n.  Graph-capturable. */
int tspm_classify_update(int32_t n, int32_t classes, const float* logits, const int64_t* labels,
                         const int32_t* groups, int32_t n_groups, int64_t* confusion, int64_t* pred_out,
                         const float* loss, float* loss_log, int64_t* counters, int64_t log_capacity,
                         tspm_stream_t stream);
/* Argmax conventions: the fusion model predicts argmax(softmax(logits)) (models/avmnist.py:305-306),
 * the monomodal pre-training step argmax(logits) (train_monomodal.py:236,394); they differ only when
 * two logits round to one probability. */
#define TSPM_ARGMAX_SOFTMAX 0
#define TSPM_ARGMAX_LOGITS 1
/* tspm_classify_update with an explicit convention (argmax_of: TSPM_ARGMAX_*). */
int tspm_classify_update_ex(int32_t n, int32_t classes, const float* logits, const int64_t* labels,
                            const int32_t* groups, int32_t n_groups, int64_t* confusion, int64_t* pred_out,
                            const float* loss, float* loss_log, int64_t* counters, int64_t log_capacity,
                            int32_t argmax_of, tspm_stream_t stream);
/* Sum `nslab` slabs of `count` floats (slab_stride apart) into out (deterministic slab order). */
int tspm_reduce_slabs(int64_t count, int32_t nslab, int64_t slab_stride, const float* slabs, float* out,
                      tspm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * MMIMDb late-fusion path (BASELINE configs[3]; ABI 11).  The encoders (BatchNorm1d + Linear,
 * models/mmimdb.py:63-93) and the MaxOut / output projections reuse tspm_bn_* (m = batch rows, HW = 1)
 * and tspm_linear_*; these entry points add the pieces around them.
 * ----------------------------------------------------------------------------------------------*/
/* GatedBiModalNetwork.forward (models/gates/gated_bimodal.py): u[n,2d] holds fc_one(x1) in columns
 * [0,d) and fc_two(x2) in [d,2d).  h = tanh(u) (the concatenated features, [n,2d], kept for the
 * backward), gate[r] = sigmoid(sum_j wz[j]*h[r,j]) (hidden_sigmoid, no bias),
 * z[r,j] = gate*h[r,j] + (1-gate)*h[r,d+j]. */
int tspm_gmu_fwd(int32_t n, int32_t d, const float* u, int32_t ldu, const float* wz, float* h, int32_t ldh,
                 float* gate, float* z, int32_t ldz, tspm_stream_t stream);
/* Backward of tspm_gmu_fwd: du[n,2d] (gradient of both projections' outputs) and ds[n] (gradient of
 * the gate pre-activation; hidden_sigmoid.weight.grad = ds^T @ h via tspm_linear_bwd_weight). */
int tspm_gmu_bwd(int32_t n, int32_t d, const float* dz, int32_t lddz, const float* h, int32_t ldh,
                 const float* gate, const float* wz, float* du, int32_t lddu, float* ds, tspm_stream_t stream);
/* MultimodalPooling (ABI 13; models/pooling.py:6-127), the MMIMDb `multimodal_pooling` fusion.
 * u = [proj_a(x_a) | proj_b(x_b)] [n, 2d] from the small GEMM (with biases).
 * tspm_pool_act_fwd: tu = tanh(u), ab = tu * keep * keep_scale ([n, 2d] contiguous; keep nullable =
 *   no dropout; the module's one Dropout draws a and b independently).
 * tspm_pool_mix_fwd: z = max(a, b) (kind 0, NaN-propagating) / (a + b) / 2 (1) / a + b (2) /
 *   attention (3: w = softmax(W2 tanh(hpre) + b2), z = w0 a + w1 b) / gated (4: g = sigmoid(W2
 *   tanh(hpre) + b2), z = g a + (1 - g) b); hpre [n, hd] = the scoring MLP's first Linear (+ bias) of
 *   [a | b] (small GEMM); hh receives tanh(hpre), wts [n][2] the mixing weights (kinds 3-4).
 * tspm_pool_mix_bwd: dab [n, 2d] through the mix (max: ties split the gradient in half, as torch.maximum);
 *   kinds 3-4 also ds [n, 2 | 1] (scores' gradient: W2 grad = ds^T hh, b2 grad = column sums) and
 *   dhpre [n, hd] (through W2 and the tanh).
 * tspm_pool_act_bwd: du = (dab + dab2) * keep * keep_scale * (1 - tu^2) (dab2 nullable: the scoring
 *   MLP's input gradient). */
int tspm_pool_act_fwd(int32_t n, int32_t d, const float* u, int32_t ldu, const uint8_t* keep, float keep_scale,
                      float* tu, float* ab, tspm_stream_t stream);
int tspm_pool_mix_fwd(int32_t n, int32_t d, int32_t hd, int32_t kind, const float* ab, const float* hpre, float* hh,
                      const float* w2, const float* b2, float* wts, float* z, int32_t ldz, tspm_stream_t stream);
int tspm_pool_mix_bwd(int32_t n, int32_t d, int32_t hd, int32_t kind, const float* dz, int32_t lddz, const float* ab,
                      const float* hh, const float* w2, const float* wts, float* dab, float* ds, float* dhpre,
                      tspm_stream_t stream);
int tspm_pool_act_bwd(int32_t n, int32_t d, const float* dab, const float* dab2, const float* tu, const uint8_t* keep,
                      float keep_scale, float* du, tspm_stream_t stream);
/* MaxOut(num_units=2) (models/maxout.py) + the Dropout after it (models/mmimdb.py:40-45): a[n,2d] is
 * the product with both units' weights stacked ([2d, in] — layers.0.weight then layers.1.weight);
 * y = max(a[:, :d], a[:, d:]) * (keep ? keep_scale : 0)  (keep NULL: no dropout). */
int tspm_maxout_fwd(int32_t n, int32_t d, const float* a, int32_t lda, const uint8_t* keep, float keep_scale,
                    float* y, int32_t ldy, tspm_stream_t stream);
/* tspm_maxout_fwd with the dropout mask drawn in-launch (ABI 11): keep[t] = the bit tspm_dropout_mask(
 * count, p, seed, counter) writes at index index_offset + t (stored for the backward), y as tspm_maxout_fwd
 * with that mask — one launch instead of mask + MaxOut. */
int tspm_maxout_fwd_rng(int32_t n, int32_t d, const float* a, int32_t lda, float p, uint64_t seed,
                        const uint64_t* counter, int64_t index_offset, uint8_t* keep, float keep_scale, float* y,
                        int32_t ldy, tspm_stream_t stream);
/* da[n,2d] from dy: the unit holding the max receives the (dropout-masked) gradient; ties split it in
 * half (ATen's derivative of torch.maximum). */
int tspm_maxout_bwd(int32_t n, int32_t d, const float* dy, int32_t lddy, const float* a, int32_t lda,
                    const uint8_t* keep, float keep_scale, float* da, int32_t ldda, tspm_stream_t stream);
/* BatchNorm1d, training mode, over x[m, c] (m = batch rows; models/mmimdb.py:78,38-46), in one launch:
 * batch mean / biased variance for y = gamma*(x-mean)*invstd + beta, running statistics updated with
 * the unbiased variance (momentum, eps as nn.BatchNorm1d; NULL running buffers skip the update),
 * save_mean / save_invstd [c] kept for the backward.  No workspace. */
int tspm_bn1d_fwd(int32_t m, int32_t c, const float* x, const float* gamma, const float* beta,
                  float* running_mean, float* running_var, float momentum, float eps, float* save_mean,
                  float* save_invstd, float* y, tspm_stream_t stream);
/* Its backward in one launch: dgamma = sum(g*xhat), dbeta = sum(g) (written), and (dx nullable)
 * dx = gamma*invstd*(g - dbeta/m - xhat*dgamma/m). */
int tspm_bn1d_bwd(int32_t m, int32_t c, const float* g, const float* x, const float* mean, const float* invstd,
                  const float* gamma, float* dgamma, float* dbeta, float* dx, tspm_stream_t stream);
/* BatchNorm1d followed by Dropout (FcClassifier(use_bn=True): Linear -> ReLU -> BatchNorm1d -> Dropout,
 * models/msa/networks/classifier.py:98-104; ABI 14): tspm_bn1d_fwd, then y *= keep ? keep_scale : 0
 * (keep uint8 [m, c], nullable = no dropout). */
int tspm_bn1d_fwd_drop(int32_t m, int32_t c, const float* x, const float* gamma, const float* beta,
                       float* running_mean, float* running_var, float momentum, float eps, float* save_mean,
                       float* save_invstd, const uint8_t* keep, float keep_scale, float* y, tspm_stream_t stream);
/* Its backward (ABI 14): g is the gradient of the Dropout output (g_keep nullable), x the BatchNorm input =
 * a ReLU output; dgamma / dbeta as tspm_bn1d_bwd on g*keep*g_scale, dx (nullable) = the BN input gradient
 * with the ReLU's mask applied (0 where x <= 0) — the gradient of the Linear that fed the ReLU. */
int tspm_bn1d_bwd_drop_relu(int32_t m, int32_t c, const float* g, const uint8_t* g_keep, float g_scale,
                            const float* x, const float* mean, const float* invstd, const float* gamma,
                            float* dgamma, float* dbeta, float* dx, tspm_stream_t stream);
/* Two independent BatchNorm1d layers over the same m rows in one launch (the MMIMDb image and text
 * encoders' input BNs; ABI 11): each half exactly as tspm_bn1d_fwd / tspm_bn1d_bwd (bitwise). */
int tspm_bn1d_fwd_pair(int32_t m, int32_t c0, const float* x0, const float* gamma0, const float* beta0,
                       float* running_mean0, float* running_var0, float momentum0, float eps0, float* save_mean0,
                       float* save_invstd0, float* y0, int32_t c1, const float* x1, const float* gamma1,
                       const float* beta1, float* running_mean1, float* running_var1, float momentum1, float eps1,
                       float* save_mean1, float* save_invstd1, float* y1, tspm_stream_t stream);
int tspm_bn1d_bwd_pair(int32_t m, int32_t c0, const float* g0, const float* x0, const float* mean0,
                       const float* invstd0, const float* gamma0, float* dgamma0, float* dbeta0, float* dx0,
                       int32_t c1, const float* g1, const float* x1, const float* mean1, const float* invstd1,
                       const float* gamma1, float* dgamma1, float* dbeta1, float* dx1, tspm_stream_t stream);
/* tspm_bn1d_fwd over a REPLICATED batch, from its m distinct rows (added under ABI 23) — the input BatchNorm1d of an
 * encoder when every missing-modality pattern of a batch trains in one step: the batch the layer sees holds each row of
 * x [m, c] `reps` times (the patterns that keep the modality, reps >= 1) and, per row of x, `zero_rows_per_row`
 * all-zero rows (the patterns that drop it, >= 0), N = m*(reps + zero_rows_per_row) rows in all.  Per channel, with
 * S = sum_r x[r]:
 *   mean   = reps*S / N
 *   M2     = reps*sum_r (x[r] - mean)^2 + zero_rows_per_row*m*mean^2
 *   invstd = 1/sqrt(M2/N + eps)           (the biased variance normalises)
 *   running_mean <- (1 - momentum)*running_mean + momentum*mean,  running_var likewise with M2/(N - 1)  (NULL: skipped)
 *   y[r]   = gamma*(x[r] - mean)*invstd + beta   for r < m
 *   y[m]   = gamma*(0 - mean)*invstd + beta      — the row every all-zero row normalises to
 * so y has m + 1 rows ([m + 1, c]; x is read over m rows only) and save_mean / save_invstd [c] hold the replicated
 * batch's statistics: tspm_bn1d_bwd at m + 1 rows over an input whose row m is zero, with the gradients folded onto
 * those rows, then gives the replicated batch's dgamma / dbeta.  tspm_bn1d_fwd's kernel structure (one launch, lane =
 * channel, 32 row groups, two-pass statistics in double, row groups combined in a fixed order, no atomics, no
 * workspace).  With reps = 1 and zero_rows_per_row = 0, rows [0, m) of y, the saved and the running statistics are
 * BITWISE tspm_bn1d_fwd's.  The pair form takes two layers over the same m rows in one launch, each half with its own
 * reps / zero_rows_per_row and bitwise the single call.  TSPM_ERR_INVALID before any launch: m <= 0, c <= 0,
 * reps < 1, zero_rows_per_row < 0, m*(reps + zero_rows_per_row) < 2, a NULL among x, gamma, beta, save_mean,
 * save_invstd, y. */
int tspm_bn1d_fwd_rep(int32_t m, int32_t c, const float* x, const float* gamma, const float* beta,
                      float* running_mean, float* running_var, float momentum, float eps, float* save_mean,
                      float* save_invstd, float* y, int32_t reps, int32_t zero_rows_per_row, tspm_stream_t stream);
int tspm_bn1d_fwd_rep_pair(int32_t m, int32_t c0, const float* x0, const float* gamma0, const float* beta0,
                           float* running_mean0, float* running_var0, float momentum0, float eps0, float* save_mean0,
                           float* save_invstd0, float* y0, int32_t reps0, int32_t zero_rows_per_row0, int32_t c1,
                           const float* x1, const float* gamma1, const float* beta1, float* running_mean1,
                           float* running_var1, float momentum1, float eps1, float* save_mean1, float* save_invstd1,
                           float* y1, int32_t reps1, int32_t zero_rows_per_row1, tspm_stream_t stream);
/* BCEWithLogitsLoss (mean) — LossFunctionGroup{bce_with_logits: w} (experiment_utils/loss.py:52,
 * configs/mmimdb/centralised/mmimdb_baseline.yaml): loss[0] = grad_scale * mean((1-t)*x - logsigmoid(x)),
 * dlogits = (sigmoid(x) - t) * grad_scale / (n*classes) (nullable).  If stats != NULL (3 + 3*classes
 * floats, accumulated): [0] += loss*n, [1] += n, [2] += sum of per-sample F1 (zero_division 0),
 * [3+3k .. 5+3k] += tp, fp, fn of class k, with prediction = sigmoid(x) > threshold
 * (models/mmimdb.py:236-237). */
int tspm_bce_logits(int32_t n, int32_t classes, const float* logits, const float* targets, float* loss,
                    float* dlogits, float grad_scale, float threshold, float* stats, tspm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * MOSI UTT-Fusion (BASELINE configs[4]; ABI 12) — MML_Suite/models/msa/utt_fusion.py:25-200 with
 * configs/mosi/centralised/utt_fusion_base_training.yaml.  Sequences are time-major on the device:
 * row (t, b) of a [T][B][F] tensor.
 * ----------------------------------------------------------------------------------------------*/
/* nn.LSTM(input, hidden, batch_first=True), one layer, zero initial state, embd_method "last" or
 * "maxpool" (models/msa/networks/lstm.py:8-67; the reference runs the padded length, no packing).
 * xg = x W_ih^T + b_ih for all steps (a tspm_linear_fwd over the T*B rows); the recurrence adds
 * h W_hh^T + b_hh.  Saved for the backward: activated gates i,f,g,o [T][B][4H], c_t [T][B][H], h_t
 * [T+1][B][H] (hs[0] = h0 = 0).  argmax NULL ("last"): h_T goes to h_out (row stride ld_out); argmax
 * non-NULL ("maxpool", ABI 14; lstm.py:47-52 F.max_pool1d over r_out): max over t of h_t goes to h_out
 * and its time index (first maximum, NaN wins) to argmax uint8 [batch][hidden] (steps <= 256).  hidden
 * must be 64; any batch >= 1 (an odd batch leaves the last 2-row workgroup one ghost row, which reads the
 * last real row and writes nothing). */
typedef struct tspm_lstm_fwd_desc {
  int32_t batch, steps, hidden, ld_out;
  const float* xg;
  const float* w_hh;
  const float* b_hh; /* nullable */
  float* gates;
  float* cs;
  float* hs;
  float* h_out;
  uint8_t* argmax; /* nullable; ABI 14 */
} tspm_lstm_fwd_desc;
/* 1 or 2 independent LSTMs (the audio and video encoders) in one launch. */
int tspm_lstm_fwd(int32_t count, const tspm_lstm_fwd_desc* descs, tspm_stream_t stream);
/* Backward through time from dh (the gradient of the embedding, row stride ld_dh: of h_T, or with
 * argmax (ABI 14) of h_{argmax} per unit, the max-pool backward): writes the pre-activation
 * gate gradients dgates [T][B][4H].  The weight gradients are then GEMMs over the T*B rows:
 * dW_hh = dgates^T hs[0:T], dW_ih = dgates^T x, db_hh = db_ih = column sums of dgates. */
typedef struct tspm_lstm_bwd_desc {
  int32_t batch, steps, hidden, ld_dh;
  const float* w_hh;
  const float* gates;
  const float* cs;
  const float* dh;
  float* dgates;
  const uint8_t* argmax; /* nullable; ABI 14 */
} tspm_lstm_bwd_desc;
int tspm_lstm_bwd(int32_t count, const tspm_lstm_bwd_desc* descs, tspm_stream_t stream);
/* The same recurrences at any hidden width (added under ABI 23; tspm_lstm_fwd / _bwd above keep refusing every width
 * but 64): hidden a multiple of 4 with 4 <= hidden <= 128 — one thread per gate column with its row (column quarter)
 * of W_hh in registers, 512 threads at most — anything else is TSPM_ERR_INVALID.  Same descriptors, semantics and
 * memory layouts, with the real hidden as the width of every tensor (no padding in memory).  count is 1 or 2 and each
 * descriptor has its own hidden / batch / steps; widths are served by three kernel tiers (32 / 64 / 128 lanes per
 * gate, lanes past hidden idle) and the compile-time 64-wide kernels, two descriptors of one kind share a launch and
 * two of different kinds take one launch each; either way the results are bitwise those of two count-1 calls, and at
 * hidden = 64 bitwise those of tspm_lstm_fwd / tspm_lstm_bwd.  Every descriptor is validated before the first launch. */
int tspm_lstm_fwd_w(int32_t count, const tspm_lstm_fwd_desc* descs, tspm_stream_t stream);
int tspm_lstm_bwd_w(int32_t count, const tspm_lstm_bwd_desc* descs, tspm_stream_t stream);
/* tspm_lstm_fwd_w / tspm_lstm_bwd_w with a 16-bit time index (added under ABI 23, no existing signature changed): the
 * "maxpool" embedding past 256 steps (the unaligned CMU-MOSI / CMU-MOSEI audio and video sequences).  Same descriptors,
 * widths, tiers, launch sharing and semantics (first maximum, NaN wins; h_out is the kernel's own h at its own index; a
 * ghost row writes nothing), with ONE difference: a non-NULL `argmax` field is read as `uint16_t*` — the caller casts
 * its `uint16_t [batch][hidden]` buffer (2-byte aligned) to the field's declared `uint8_t*`, and must pass the same
 * buffer to the backward.  With an index 1 <= steps <= 65535; with argmax NULL steps is unlimited, as in _w; anything
 * else is TSPM_ERR_INVALID.  With argmax NULL the results are bitwise those of _w; with an index and steps <= 256 every
 * float output is bitwise _w's and the index values are equal as integers. */
int tspm_lstm_fwd_t16(int32_t count, const tspm_lstm_fwd_desc* descs, tspm_stream_t stream);
int tspm_lstm_bwd_t16(int32_t count, const tspm_lstm_bwd_desc* descs, tspm_stream_t stream);
/* The recurrences with per-sample sequence lengths (added under ABI 23, no existing signature changed):
 * pack_padded_sequence semantics over a padded batch.  The descriptors are tspm_lstm_fwd_desc / tspm_lstm_bwd_desc plus
 *   lengths     int32 [batch] in DEVICE memory, required (NULL is TSPM_ERR_INVALID).  The host never reads the values; the
 *               kernel runs row b for L_b = min(max(lengths[b], 1), steps) steps, so no value moves an access outside
 *               the buffers, and a captured graph may be replayed after the buffer's contents change;
 *   index_bits  the width of the `argmax` buffer: 8 (uint8 [batch][hidden], steps <= 256) or 16 (uint16 [batch][hidden],
 *               2-byte aligned, steps <= 65535); with an index anything else is TSPM_ERR_INVALID, with argmax NULL the
 *               field is ignored and steps is unlimited.  One pair of entry points covers what _w and _t16 cover.
 * hidden: a multiple of 4 in 4..128, served by the tiers and kinds of tspm_lstm_fwd_w.  count is 1 or 2, each descriptor
 * with its own batch / steps / hidden / lengths / index_bits; two descriptors of one kernel kind (and, where both carry
 * an index, one index width) share a launch, otherwise one launch each, and the results are bitwise those of two
 * count-1 calls.  Every descriptor is validated before the first launch.
 * Forward, row b: for t < L_b the arithmetic of tspm_lstm_fwd_w unchanged (gates, cs, hs[t+1] saved as there).  argmax
 * NULL ("last"): h_out[b] = h at step L_b - 1.  argmax non-NULL ("maxpool"): h_out[b] = max over t < L_b of h_t (first
 * maximum, NaN wins) and the index written is < L_b.  hs[t+1][b] for L_b <= t < steps is written as +0.0 (what
 * pad_packed_sequence returns; the dW_hh GEMM multiplies these rows by zero gate gradients, so they must be finite);
 * gates and cs rows at t >= L_b are NOT written and nothing may read them.  With every length >= steps all outputs are
 * bitwise those of tspm_lstm_fwd_w (index_bits 8) / tspm_lstm_fwd_t16 (16).
 * Backward, row b: the embedding gradient dh enters at t = L_b - 1 ("last") or at the saved index ("maxpool"); for
 * t < L_b the arithmetic of tspm_lstm_bwd_w unchanged; dgates[t][b] for L_b <= t < steps is written as +0.0, so the
 * weight-gradient GEMMs over all steps * batch rows stay as they are.  Pass the forward's lengths.
 * A 2-row workgroup runs max(L_b) over its rows (the ghost row of an odd batch takes the length of the row it clamps
 * to), so a launch lasts as long as the batch's longest sequence, not the padded length. */
typedef struct tspm_lstm_fwd_len_desc {
  int32_t batch, steps, hidden, ld_out;
  const float* xg;
  const float* w_hh;
  const float* b_hh; /* nullable */
  float* gates;
  float* cs;
  float* hs;
  float* h_out;
  void* argmax; /* nullable; uint8 or uint16 by index_bits */
  const int32_t* lengths;
  int32_t index_bits;
  int32_t reserved_; /* 0 */
} tspm_lstm_fwd_len_desc;
typedef struct tspm_lstm_bwd_len_desc {
  int32_t batch, steps, hidden, ld_dh;
  const float* w_hh;
  const float* gates;
  const float* cs;
  const float* dh;
  float* dgates;
  const void* argmax; /* nullable; the forward's buffer */
  const int32_t* lengths;
  int32_t index_bits;
  int32_t reserved_; /* 0 */
} tspm_lstm_bwd_len_desc;
int tspm_lstm_fwd_len(int32_t count, const tspm_lstm_fwd_len_desc* descs, tspm_stream_t stream);
int tspm_lstm_bwd_len(int32_t count, const tspm_lstm_bwd_len_desc* descs, tspm_stream_t stream);
/* The backward recurrence with a gradient at EVERY step (added under ABI 23, no existing signature changed): what an
 * embedding that weights all of r_out — LSTMEncoder(embd_method="attention") — hands to the recurrence.  The descriptor
 * is tspm_lstm_bwd_len_desc without the index fields, plus
 *   dseq  [steps][batch][hidden], nullable: added to dh_t at every t < L_b;
 *   wt    [steps][batch], nullable: with dh non-NULL, dh_t += wt[t][b] * dh[b] at every t < L_b (the alpha_t g term of
 *         the attention pooling without another pass over [steps][batch][hidden]); with wt NULL dh enters at L_b - 1,
 *         exactly as tspm_lstm_bwd_len's "last" does; with dh NULL wt is not read;
 *   dh    nullable; at least one of dh / dseq must be given (else TSPM_ERR_INVALID).
 * lengths (device int32 [batch]) is required and clamped on the device as in tspm_lstm_bwd_len; nothing at t >= L_b is
 * read from dseq / wt (the padding may hold anything), and dgates[t][b] for L_b <= t < steps is written as +0.0.
 * hidden, count, tiers, kinds and launch sharing are those of tspm_lstm_bwd_w; every descriptor is validated before
 * the first launch.  Per step: dh_t = (the recurrent term) [+ wt * dh] [+ dseq], in that order; with dseq and wt NULL
 * the results are bitwise those of tspm_lstm_bwd_len without an index. */
typedef struct tspm_lstm_bwd_seq_desc {
  int32_t batch, steps, hidden, ld_dh;
  const float* w_hh;
  const float* gates;
  const float* cs;
  const float* dh;   /* nullable */
  float* dgates;
  const float* dseq; /* nullable */
  const float* wt;   /* nullable */
  const int32_t* lengths;
} tspm_lstm_bwd_seq_desc;
int tspm_lstm_bwd_seq(int32_t count, const tspm_lstm_bwd_seq_desc* descs, tspm_stream_t stream);
/* Attention pooling over the LSTM outputs (added under ABI 23) — LSTMEncoder(embd_method="attention"), the
 * Hierarchical-Attention embedding of models/msa/networks/lstm.py:21-44.  Row b, L_b = min(max(lengths[b], 1), steps),
 * r_t = r[t][b] (the recurrence's hs + batch * hidden):
 *   norm 0 ("time"): s_t = tanh(p_t) . u for t < L_b, alpha_t = exp(s_t - max s) / sum_{tau < L_b} exp(s_tau - max s);
 *   norm 1 ("unit"): alpha_t = 1 for t < L_b (a softmax over a trailing axis of size 1);
 *   alpha_t = +0.0 for t >= L_b;  h_out[b] = sum_{t < L_b} alpha_t r_t (row stride ld_out).
 * p [steps][batch][hidden] comes in as the pre-activation W r_t + c (a tspm_linear_fwd over the steps * batch rows) and
 * leaves as z = tanh(p) for t < L_b (rows past the length are neither read nor written); with norm 1, p and u are not
 * read and may be NULL.  alpha is [steps][batch].  One workgroup per batch row; every reduction runs in an order that
 * depends on L_b (and hidden) alone, so a row's alpha and h_out are bitwise the same whatever the padding and whatever
 * else is in the batch.  hidden: a multiple of 4 in 4..128; r and p 16-byte aligned; steps * batch within int32; norm
 * other than 0 / 1, a NULL lengths, count outside 1..2: TSPM_ERR_INVALID before any launch.  Two descriptors share the
 * one launch. */
typedef struct tspm_attn_pool_fwd_desc {
  int32_t batch, steps, hidden, ld_out;
  int32_t norm, reserved_; /* reserved_: 0 */
  const float* r;
  float* p;       /* in: W r + c; out: tanh of it (norm 0; nullable with norm 1) */
  const float* u; /* [hidden] (norm 0; nullable with norm 1) */
  float* alpha;
  float* h_out;
  const int32_t* lengths;
} tspm_attn_pool_fwd_desc;
int tspm_attn_pool_fwd(int32_t count, const tspm_attn_pool_fwd_desc* descs, tspm_stream_t stream);
/* Its backward for norm 0 (norm 1 has no gradient through the scores: the caller launches nothing and the recurrence
 * takes wt = alpha, dh = g).  From g = dloss/dh_out (row stride ld_g), alpha, z (the forward's p buffer), r and u:
 * a_t = g . r_t, D = sum_{t < L_b} alpha_t a_t, ds_t = alpha_t (a_t - D),
 *   dp[t][b] = ds_t * u * (1 - z_t^2) for t < L_b and +0.0 for t >= L_b ([steps][batch][hidden]: the GEMMs that follow
 *   — dW = dp^T r, dseq = dp W — read all steps * batch rows);
 *   du[h] = sum_{b, t < L_b} ds_t z_t[h];
 *   dc[h] = -u[h] sum_{b, t < L_b} ds_t z_t[h]^2 — the bias gradient sum_{b,t} dp[t][b][h] with its cancelling part
 *   (sum_t ds_t = 0 in every row) taken out; the column sums of dp in float32 lose 1e-5 .. 1e-4 of it to that part;
 *   du and dc: per-row sums into rows [batch][2 * hidden] (caller-provided scratch), then a second launch adds the rows
 *   in index order.  No floating-point atomics: the same inputs give the same bits.
 * Shapes, alignment (r, z, dp 16-byte aligned), lengths and count as in the forward; norm must be 0. */
typedef struct tspm_attn_pool_bwd_desc {
  int32_t batch, steps, hidden, ld_g;
  int32_t norm, reserved_; /* norm: 0 */
  const float* g;
  const float* alpha;
  const float* z;
  const float* r;
  const float* u;
  float* dp;
  float* du;
  float* dc;
  float* rows;
  const int32_t* lengths;
} tspm_attn_pool_bwd_desc;
int tspm_attn_pool_bwd(int32_t count, const tspm_attn_pool_bwd_desc* descs, tspm_stream_t stream);
/* TextCNN pooling (models/msa/networks/textcnn.py:56-67): for conv i (kernel height heights[i], output
 * conv_out[i] time-major [steps-heights[i]+1][batch][channels] without bias), bias[i] added, ReLU,
 * max over time (first maximum, F.max_pool1d), concatenated over convs: pooled[b][i*C+c] and the
 * argmax time index; out[b*ld_out + i*C+c] = pooled * (keep ? keep*keep_scale : 1) — the dropout before
 * the embedding Linear (keep uint8 [batch][nconv*C], nullable).  nconv <= 4, steps <= 256. */
int tspm_textcnn_pool_fwd(int32_t batch, int32_t steps, int32_t nconv, const int32_t* heights,
                          int32_t channels, const float* const* conv_out, const float* const* bias,
                          const uint8_t* keep, float keep_scale, float* pooled, uint8_t* argmax,
                          float* out, int32_t ld_out, tspm_stream_t stream);
/* The same pooling with per-sample text lengths (added under ABI 23): the arguments of tspm_textcnn_pool_fwd in their
 * order plus lengths, int32 [batch] in device memory (required: NULL is TSPM_ERR_INVALID).  The host never reads a
 * length; the kernel clamps L_b = min(max(lengths[b], 1), steps), so no value moves an access outside the buffers and a
 * captured graph may be replayed after the buffer's contents change.  Row b of conv i has
 * n_i(b) = max(L_b - heights[i] + 1, 1) windows: bias, ReLU and the first maximum (NaN wins) run over t < n_i(b), and the
 * index written is < n_i(b); pooled, argmax, the dropout and out are as in tspm_textcnn_pool_fwd.  That is the TextCNN
 * applied to the row's own first L_b steps, zero-padded to max(L_b, heights[i]).  PRECONDITION: for a row shorter than a
 * kernel height the single window reads the input's padding rows [L_b, heights[i]), which must be zero (what
 * pad_sequence and tspm_seq_gather write) — the one place where the padding's content, not its extent, still matters.
 * With every length >= steps the outputs are bitwise those of tspm_textcnn_pool_fwd.  tspm_textcnn_bwd takes the indices
 * written here unchanged: it reads x only at argmax + dt, dt < heights[i], which stays below max(L_b, heights[i]). */
int tspm_textcnn_pool_fwd_len(int32_t batch, int32_t steps, int32_t nconv, const int32_t* heights,
                              int32_t channels, const float* const* conv_out, const float* const* bias,
                              const uint8_t* keep, float keep_scale, float* pooled, uint8_t* argmax,
                              float* out, int32_t ld_out, const int32_t* lengths, tspm_stream_t stream);
/* TextCNN backward from dout (gradient of the embedding Linear's input, row stride ld_dout): through the
 * dropout and the ReLU at the argmax; conv weight gradients dw[i] ([C][heights[i]][feat], the
 * nn.Conv2d(1, C, (h, feat)) weight layout) and bias gradients db[i] (nullable) from the argmax rows
 * only (the time-max passes gradient to one position per (b, c)): dw[c][dt][f] = sum_b g[b][c]
 * x[arg[b][c] + dt][b][f].  x is the time-major text input [steps][batch][feat] (feat <= 1024,
 * heights <= 5); g_work holds batch*nconv*channels floats. */
int tspm_textcnn_bwd(int32_t batch, int32_t steps, int32_t feat, int32_t nconv, const int32_t* heights,
                     int32_t channels, const float* x, const float* dout, int32_t ld_dout, const uint8_t* keep,
                     float keep_scale, const float* pooled, const uint8_t* argmax, float* const* dw,
                     float* const* db, float* g_work, tspm_stream_t stream);
/* clip_grad_norm_(parameters, max_norm) coefficient (utt_fusion.py:189): total = ||grad * grad_scale||_2
 * (squares summed in double, fixed order), *coef = min(1, max_norm / (total + 1e-6)) for
 * tspm_adam_step_clip, as torch.clamp(max=1): a NaN total gives a NaN coefficient (an inf total gives 0);
 * *total_norm (nullable) = total.  workspace: tspm_grad_clip_workspace() bytes (a missing or shorter one, with
 * the other arguments valid, is TSPM_ERR_WORKSPACE). */
size_t tspm_grad_clip_workspace(void);
int tspm_grad_clip_coef(int64_t count, const float* grad, float grad_scale, float max_norm, float* coef,
                        float* total_norm, void* workspace, size_t workspace_bytes, tspm_stream_t stream);
/* clip_grad_norm_ over several gradient buffers (added under ABI 23): total = the 2-norm of all `ranges` together (a
 * HOST array of `count` ranges, 1 <= count <= TSPM_ADAM_MAX_SEGMENTS, copied into the kernel arguments; a range with
 * count 0 is skipped and may have a NULL grad), in the two launches of tspm_grad_clip_coef: one sum-of-squares launch
 * of 512 workgroups writing double partials, each workgroup summing a slice of ONE range, then the same coefficient
 * kernel.  A non-empty range gets 1 + floor((512 - n) * count / total) workgroups (n = the number of non-empty
 * ranges, total = the sum of their counts); workgroups left over write a zero partial.  The partition depends on the
 * counts alone, so equal inputs give equal bits; with count == 1 it is tspm_grad_clip_coef's and *coef and
 * *total_norm are bitwise that call's.  Otherwise the squares are summed in another order: in double, so only the
 * final rounding to float can differ.  coef, total_norm, workspace and the status codes as tspm_grad_clip_coef
 * (TSPM_ERR_INVALID also for a negative count, a NULL grad of a non-empty range, or no element at all). */
typedef struct tspm_grad_range {
  const float* grad;
  int64_t count;
} tspm_grad_range;
int tspm_grad_clip_coef_multi(int32_t count, const tspm_grad_range* ranges, float grad_scale, float max_norm,
                              float* coef, float* total_norm, void* workspace, size_t workspace_bytes,
                              tspm_stream_t stream);
/* Padded batch assembly (data/mosi.py:202-232 pad_sequence + the step's .to(device)) from a ragged
 * corpus data[rows][feat] (sample s = rows offsets[s] .. offsets[s]+lengths[s]-1): out[t*stride_t +
 * b*stride_b + f] = sample index[b]'s row t (0 past its length) * row_mask[b] (nullable), for
 * t < steps_pad; labels_out[b] = labels[index[b]] (both nullable).  Out-of-range indices write NaN
 * rows and label -1. */
int tspm_seq_gather(int32_t count, const int64_t* index, int64_t n_samples, const float* data,
                    const int64_t* offsets, const int32_t* lengths, int32_t feat, int32_t steps_pad, float* out,
                    int64_t stride_t, int64_t stride_b, const float* row_mask, const int64_t* labels,
                    int64_t* labels_out, tspm_stream_t stream);
/* Missing-modality pattern expansion (added under ABI 23) — every pattern of a batch from ONE encoder pass over 2*batch
 * rows.  emb [2*batch][ld_emb]: rows [0, batch) are the embeddings cat(audio, video, text) of the real inputs, rows
 * [batch, 2*batch) those of the zeroed inputs of the same rows (a zeroed tensor through the encoder, not a zero
 * embedding).  In one launch, for p < npat and b < batch, with row = p*batch + b:
 *   out[row*ld_out + c]  = emb[(keep[3p + m] ? b : batch + b)*ld_emb + c]  for every column c of modality m
 *   labels_out[row]      = labels[b]         (label_bytes = 8: int64 class labels, 4: float32 scores; copied as bytes)
 *   groups_out[row]      = group_id[p]       (int32)
 * keep ([npat][3], the (audio, video, text) flags of a pattern, non-zero = kept) and group_id ([npat]) are HOST
 * arrays copied into the kernel arguments (nothing of them is read after the call returns).  Plain loads and stores,
 * 16 bytes wide for a modality whose width and column offset are multiples of 4 when ld_emb and ld_out are too and
 * emb / out are 16-byte aligned, else one float each; no atomics; nothing but the elements named above is written
 * (padding columns of out keep their content).  TSPM_ERR_INVALID before any launch: batch <= 0, npat outside
 * 1..TSPM_MAX_PATTERNS, a non-positive width, ld_emb or ld_out below the width sum, a pattern that keeps nothing, a
 * NULL pointer, label_bytes other than 4 or 8. */
#define TSPM_MAX_PATTERNS 7
int tspm_pattern_expand(int32_t batch, int32_t npat, const int32_t* keep, const int32_t* group_id, int32_t w_audio,
                        int32_t w_video, int32_t w_text, const float* emb, int64_t ld_emb, float* out, int64_t ld_out,
                        const void* labels, void* labels_out, int32_t label_bytes, int32_t* groups_out,
                        tspm_stream_t stream);
/* The adjoint of tspm_pattern_expand (added under ABI 23), for training every pattern of a batch in one step: folds
 * the classifier-input gradient dout [npat*batch][ld_dout] (row p*batch + b) back onto the 2*batch encoder rows.  For
 * each modality m whose bit is set in modalities (bit 0 audio, 1 video, 2 text), b < batch and column c of m:
 *   demb[b*ld_demb + c]           = sum over the p with keep[3p + m] != 0 of dout[(p*batch + b)*ld_dout + c]
 *   demb[(batch + b)*ld_demb + c] = sum over the p with keep[3p + m] == 0 of the same
 * Each sum starts from +0.0 and adds in ascending p with plain fp32 adds (nothing to contract, no atomics: one thread
 * owns one output unit), so it is deterministic and a host loop restates it bit for bit; a slot no pattern uses is
 * written +0.0.  Columns of a modality whose bit is clear (a frozen encoder, whose gradient nobody reads) and padding
 * columns keep their content.  keep is a HOST array as above.  16 bytes per thread under tspm_pattern_expand's rule
 * (applied to dout / ld_dout and demb / ld_demb), else one float.  TSPM_ERR_INVALID before any launch: everything
 * tspm_pattern_expand refuses (batch <= 0, npat outside 1..TSPM_MAX_PATTERNS, a non-positive width, ld_dout or
 * ld_demb below the width sum, a pattern that keeps nothing, a NULL pointer) and modalities outside 1..7. */
int tspm_pattern_expand_bwd(int32_t batch, int32_t npat, const int32_t* keep, int32_t w_audio, int32_t w_video,
                            int32_t w_text, const float* dout, int64_t ld_dout, float* demb, int64_t ld_demb,
                            int32_t modalities, tspm_stream_t stream);

/* The UTT-Fusion encoder half read from a cache (added under ABI 23) — the head stage on frozen encoders without the
 * encoders.  With all three encoders frozen, everything up to the TextCNN's dropout is a per-sample constant: cache
 * row i of emb [n_rows][ld_cache] is [ eA(i) | eV(i) | pooled(i) ] (w_audio + w_video + w_pool fp32 columns: the two
 * LSTM embeddings and the TextCNN's time-max output BEFORE its dropout), and zero [n_zero][ld_cache] holds the same
 * for the zeroed inputs — one row for the whole split (n_zero == 1) or one per sample (n_zero == n_rows: with
 * per-sample lengths a zero row's embedding depends on its own lengths).  One launch; with R = halves*batch, for
 * r < R, b = r mod batch and each modality m (audio, video, text):
 *   source row = emb[rows[b]]                       when r < batch and (row_keep == NULL or row_keep[3b + m] != 0)
 *              = zero[n_zero == 1 ? 0 : rows[b]]    otherwise
 *   av_out[r*ld_av + c]     = source[c]                                  for c < w_audio + w_video (m by column)
 *   pool_out[r*ld_pool + j] = keep ? v * (keep[r*w_pool + j] ? scale : 0.f) : v,   v = source[w_audio + w_video + j]
 *   labels_out[b]           = labels_all[rows[b]]                        for r < batch only
 * halves == 2 is the all-pattern layout tspm_pattern_expand reads (the batch in rows [0, batch), its zero rows in
 * [batch, 2*batch)); halves == 1 with row_keep (uint8 [batch][3] on the DEVICE) gives each row its own pattern.  The
 * pool_out expression is tspm_textcnn_pool_fwd's store: with the same mask bytes the output is bitwise the fc_in the
 * TextCNN would have written from those pooled values.  keep (uint8 [R][w_pool], nullable) is read, never drawn here.
 * label_bytes = 8: int64 labels, 4: float32 scores.  An index outside [0, n_rows) gives a NaN row and label -1 (NaN
 * for float32 labels) and reads nothing out of bounds.  Every load and store of a float is a float4; no LDS, no
 * atomics; padding columns of av_out / pool_out keep their content.  TSPM_ERR_INVALID, nothing launched: a NULL among
 * emb, zero, rows, av_out, pool_out; a width or leading dimension that is not a positive multiple of 4, or a leading
 * dimension below its width (ld_cache below the width sum); emb, zero, av_out, pool_out or keep not 16-byte aligned;
 * halves outside {1, 2}; row_keep with halves == 2; n_zero not in {1, n_rows}; label_bytes not in {4, 8}; only one of
 * labels_all / labels_out; batch < 1 or n_rows < 1. */
typedef struct tspm_utt_cache_rows_desc {
  int32_t batch, halves, w_audio, w_video, w_pool, ld_cache, ld_av, ld_pool;
  int64_t n_rows, n_zero;
  const float* emb;            /* [n_rows, ld_cache] */
  const float* zero;           /* [n_zero, ld_cache] */
  const int64_t* rows;         /* [batch] */
  const uint8_t* row_keep;     /* DEVICE [batch][3] (audio, video, text); nullable, halves == 1 only */
  const void* labels_all;      /* [n_rows] int64 or float32; nullable with labels_out */
  void* labels_out;            /* [batch] */
  int32_t label_bytes;         /* 8 or 4 */
  float scale;                 /* the dropout's 1 / (1 - p) */
  const uint8_t* keep;         /* [R, w_pool]; nullable */
  float* av_out;               /* [R, ld_av] */
  float* pool_out;             /* [R, ld_pool] */
} tspm_utt_cache_rows_desc;
int tspm_utt_cache_rows(const tspm_utt_cache_rows_desc* desc, tspm_stream_t stream);

/* All-pattern evaluation head (added under ABI 23) — AVMNIST's classifier `net` (tspm_head_train_step's three Linears,
 * no dropout), the loss group's weighted cross-entropy and tspm_classify_update's bookkeeping for EVERY missing-modality
 * pattern of a batch in one call.  In eval mode an encoder's output row depends on that row's input and the weights
 * only, so the embedding of a zeroed modality is one constant row: x0 [in] holds both encoders' zero-input embeddings
 * (columns [0, w_audio) the audio encoder's, [w_audio, in) the image encoder's) and x [batch][ldx] the embeddings of the
 * real inputs.  For p < npat and b < batch, row = p*batch + b:
 *   input  = per modality m (0 audio, 1 image) x[b]'s columns when keep[2p + m] != 0, else x0's
 *   logits[row] = Linear(w5,b5)(relu(Linear(w3,b3)(relu(Linear(w0,b0)(input)))))
 *   preds[row]  = first argmax of softmax(logits[row])            (TSPM_ARGMAX_SOFTMAX; preds nullable)
 *   confusion[group_id[p]][labels[b]][pred] += 1                  (integer atomics; a row whose label is outside
 *                                                                   [0, classes) or whose group is outside
 *                                                                   [0, n_groups) is not counted; confusion nullable)
 *   loss[p] = loss_weight * mean_b CE(logits[p*batch + b], labels[b])   (an out-of-range label: NaN, nothing read out of
 *                                                                   bounds)
 * and once per call, when counters is given: loss_log[counters[0] + p] = loss[p] for every p with that index below
 * log_capacity (loss_log nullable), then counters[0] += npat, counters[1] += npat*batch — what npat calls of
 * tspm_cross_entropy + tspm_classify_update on the row slices leave behind, in pattern order.
 * keep ([npat][2]) and group_id ([npat]) are HOST arrays copied into the launch arguments, as in tspm_pattern_expand.
 * Two launches.  (1) One workgroup of 512 threads per sample (at most 256 workgroups, each walking its samples), the
 * three weight matrices staged in LDS as tspm_head_train_step stages them.  fc0 is linear in the concatenated input, so
 * the workgroup forms the audio-half and the image-half product of x0 once and of each sample once and adds the two
 * halves a pattern selects; fc3, fc5, the row's cross-entropy term, its prediction and its confusion count follow
 * per (pattern, sample) row.  A row's logits depend on x[b], x0, the weights and keep[p] only — not on batch, npat or
 * the other rows (bitwise).  (2) One workgroup adds each pattern's per-row terms from the workspace in a fixed order
 * (tspm_cross_entropy's: strided partial sums and a tree, in double) and writes loss, the log entries and the counters.
 * No floating-point atomics; two calls on the same inputs are bitwise equal.
 * Limits (tspm_head_train_step's): in <= 256, hidden <= 256, hidden2 <= 128, classes <= 16; in, w_audio, hidden,
 * hidden2 multiples of 4, 0 < w_audio < in; ldx >= in and a multiple of 4; x, x0, w0, w3, w5 16-byte aligned; 1 <= npat
 * <= TSPM_PATTERN_HEAD_MAX_PATTERNS; weights plus row buffers within 160 KiB of LDS.  x0 may be NULL when every pattern
 * keeps both modalities.  loss_log needs counters; confusion needs n_groups >= 1; log_capacity >= 0.  Anything else, or
 * a NULL among x, keep, group_id, the six weights, labels, logits, loss: TSPM_ERR_INVALID; a missing or short workspace
 * with the other arguments valid: TSPM_ERR_WORKSPACE.  Nothing is launched on error. */
#define TSPM_PATTERN_HEAD_MAX_PATTERNS 8
typedef struct tspm_pattern_head_eval_desc {
  int32_t batch, npat, in, w_audio, hidden, hidden2, classes, ldx;
  const float* x;           /* [batch, ldx] */
  const float* x0;          /* [in] */
  const int32_t* keep;      /* HOST [npat][2]: (audio, image), non-zero = the real input */
  const int32_t* group_id;  /* HOST [npat] */
  const float *w0, *b0, *w3, *b3, *w5, *b5;
  const int64_t* labels;    /* [batch] */
  float loss_weight;        /* the cross-entropy term's weight */
  int32_t n_groups;
  float* logits;            /* [npat*batch, classes] */
  int64_t* preds;           /* nullable: [npat*batch] */
  float* loss;              /* [npat] */
  int64_t* confusion;       /* nullable: [n_groups][classes][classes] */
  float* loss_log;          /* nullable */
  int64_t* counters;        /* nullable: {entries, samples} */
  int64_t log_capacity;
  void* workspace;          /* tspm_pattern_head_eval_workspace(batch, npat) bytes, 16-byte aligned */
  size_t workspace_bytes;
} tspm_pattern_head_eval_desc;
size_t tspm_pattern_head_eval_workspace(int32_t batch, int32_t npat);
int tspm_pattern_head_eval(const tspm_pattern_head_eval_desc* desc, tspm_stream_t stream);

/* All-pattern head TRAIN step (added under ABI 23) — tspm_head_train_step (forward, dropout, weighted cross-entropy,
 * the head's whole weight backward) for EVERY missing-modality pattern of a batch in one call, for the head stage on
 * frozen encoders: an encoder on its running statistics is a per-row function, so the embedding of a zeroed modality
 * is the constant row x0 and never changes while only the head trains.  Inputs as in tspm_pattern_head_eval (x, x0,
 * HOST keep [npat][2], the six weights, labels [batch]) plus tspm_head_desc's dropout fields.  For p < npat and
 * b < batch, row = p*batch + b, the head's input is x[b]'s columns per kept modality, else x0's:
 *   logits[row]                  [npat*batch][classes]
 *   loss[0]                      = loss_weight * mean over ALL npat*batch rows of CE(logits[row], labels[b])
 *   stats (nullable)             stats[0] += sum CE, stats[1] += #(argmax == label), stats[2] += npat*batch
 *   adam_step (nullable)         += 1 by launch 2, after launch 1 read `counter` (as tspm_head_desc.adam_step)
 *   gw0 gb0 gw3 gb3 gw5 gb5      overwritten with the gradients of loss[0]
 * There is no dx: the encoders are frozen and nobody reads it.  The per-row h1, hh, dlogits and dz3 that the
 * weight-gradient launch reads live in the workspace.  Dropout: the mask of row p*batch + b is drawn per (pattern,
 * sample) row; with gen_keep = 1 the bytes written to keep_mask [npat*batch][hidden] are those of
 * tspm_dropout_mask(npat*batch*hidden, p, seed, counter); with gen_keep = 0 keep_mask is read.  Semantics: those of
 * tspm_pattern_expand followed by tspm_head_train_step with n = npat*batch, up to summation order; an out-of-range
 * label gives a NaN loss and NaN gradients (nothing read out of bounds) and never counts as correct.
 * Two launches.  (1) One workgroup of 512 threads per sample (at most 256 workgroups, each walking its samples),
 * weights staged in LDS as tspm_head_train_step stages them.  fc0 is linear in the concatenated input: the audio-half
 * and image-half products of x0 are formed once per workgroup and those of a sample once (2 half products per sample
 * instead of npat full ones); fc3, fc5, the cross-entropy and the backward down to dz0 run on the sample's npat rows.
 * The same algebra runs backwards: per modality m the workgroup writes fold_m[b] = sum over the p that keep m of
 * dz0[p*batch + b] (ascending p) and accumulates zsum_m = sum over the p that drop m and its samples b of the same (its
 * samples in ascending b, p ascending inside), one partial row per workgroup.  (2) The weight gradients on the
 * small-GEMM tiles — gw5 / gw3 over the npat*batch rows, and gw0[:, cols_m] = sum_b fold_m[b]^T (x) x[b, cols_m]
 * + sum_g zsum_m[g]^T (x) x0[cols_m] as ONE product per modality whose K is batch + workgroups (not npat*batch),
 * gb0 its row sums — plus the loss workgroup (tspm_head_train_step's fixed-order sums, in double).  No floating-point
 * atomics; every sum has a fixed order; eager, captured and replayed calls are bitwise equal.  A sample's npat logits
 * rows depend on x[b], x0, the weights, keep and the rows' masks only.
 * Limits: tspm_head_train_step's (in <= 256, hidden <= 256, hidden2 <= 128, classes <= 16; in, hidden, hidden2
 * multiples of 4; ldx >= in and a multiple of 4; x, x0, w0, w3, w5 16-byte aligned; 0 <= p < 1, keep_mask required when
 * p > 0) plus 0 < w_audio < in, w_audio % 4 == 0, 1 <= npat <= TSPM_PATTERN_HEAD_MAX_PATTERNS; weights plus the npat
 * row buffers within 160 KiB of LDS (tspm_pattern_head_eval's formula).  x0 may be NULL when every pattern keeps both
 * modalities.  Anything else, or a NULL among x, keep, the six weights, labels, logits, the six gradients, loss:
 * TSPM_ERR_INVALID; a missing, misaligned or short workspace with the other arguments valid: TSPM_ERR_WORKSPACE.
 * Nothing is launched on error. */
typedef struct tspm_pattern_head_train_desc {
  int32_t batch, npat, in, w_audio, hidden, hidden2, classes, ldx;
  int32_t gen_keep, reserved_;
  const float* x;           /* [batch, ldx] */
  const float* x0;          /* [in] */
  const int32_t* keep;      /* HOST [npat][2]: (audio, image), non-zero = the real input */
  const float *w0, *b0, *w3, *b3, *w5, *b5;
  const int64_t* labels;    /* [batch] */
  float p;                  /* dropout probability (0: no mask) */
  float loss_weight;        /* the cross-entropy term's weight */
  uint64_t seed;
  const uint64_t* counter;  /* device step counter (fresh masks per graph replay) */
  uint8_t* keep_mask;       /* [npat*batch, hidden] */
  float* logits;            /* [npat*batch, classes] */
  float *gw0, *gb0, *gw3, *gb3, *gw5, *gb5;
  float *loss, *stats;      /* stats nullable */
  int64_t* adam_step;       /* nullable */
  void* workspace;          /* tspm_pattern_head_train_workspace(batch, npat) bytes, 16-byte aligned */
  size_t workspace_bytes;
} tspm_pattern_head_train_desc;
size_t tspm_pattern_head_train_workspace(int32_t batch, int32_t npat);
int tspm_pattern_head_train_step(const tspm_pattern_head_train_desc* desc, tspm_stream_t stream);

/* Cached embeddings (added under ABI 23) — the head stage without the encoders.  A frozen encoder on its running
 * statistics is a per-row function whose weights never move, so the embedding of every corpus sample is a constant of
 * the whole head stage: emb [n_rows][ld_emb] holds them (columns [0, w_audio) the audio encoder's, the rest the image
 * encoder's), labels_all [n_rows] the samples' labels, x0 [in] the embeddings of zeroed inputs, and a batch is the
 * index vector rows [batch] (int64, the loader's index dtype).
 *
 * tspm_embed_gather — one launch:
 *   out[b][0:in]  = emb[rows[b]][0:in]        for b < batch
 *   labels_out[b] = labels_all[rows[b]]       (labels_all / labels_out: both given or both NULL)
 * With row_keep ([batch][2] uint8 on the DEVICE, audio then image) the columns of a modality whose flag is 0 come from
 * x0 instead (w_audio splits the columns; x0 is required with row_keep).  ld_emb and ld_out are multiples of 4 and at
 * least in; in (and w_audio with row_keep, 0 < w_audio < in) a multiple of 4; emb, x0, out 16-byte aligned: every load
 * and store is a float4.  The padding columns of out keep their content.  An index outside [0, n_rows) writes a NaN row
 * and label -1 and reads nothing out of bounds.  batch >= 1, n_rows >= 1; anything else, or a NULL among emb, rows,
 * out: TSPM_ERR_INVALID, nothing launched. */
int tspm_embed_gather(int32_t batch, int32_t in, const float* emb, int64_t n_rows, int32_t ld_emb, const int64_t* rows,
                      const int64_t* labels_all, const uint8_t* row_keep, int32_t w_audio, const float* x0, float* out,
                      int32_t ld_out, int64_t* labels_out, tspm_stream_t stream);

/* tspm_cached_head_train_step — tspm_pattern_head_train_step reading its samples straight from the cache, with
 * tspm_classify_update's bookkeeping folded in.  Two launches, the semantics, sums (order included), limits and status
 * codes of tspm_pattern_head_train_step — the text above applies word for word — except:
 *   - sample b's input row is emb[rows[b]] and its label labels_all[rows[b]]; no [batch][in] input is ever formed;
 *   - two modes.  EVERY PATTERN OF THE BATCH: HOST keep [npat][2] as above, and HOST group_id [npat] (required when
 *     confusion is given).  ONE PATTERN PER SAMPLE (what the default train loader draws): npat == 1, DEVICE row_keep
 *     [batch][2] uint8 (audio, image) and DEVICE row_group [batch] int32, both given; HOST keep must be NULL, group_id
 *     is not read and x0 is required.  Sample b's one row takes each modality from emb or from x0 by its own flags;
 *     fold_m[b] is zero for a sample whose flag drops modality m, and the workgroup's zsum_m row accumulates those
 *     samples' dz0 (ascending b);
 *   - the bookkeeping of a tspm_classify_update call over the npat*batch rows (TSPM_ARGMAX_SOFTMAX: the first maximum
 *     of the softmax values): confusion[group][label][pred] += 1 with integer atomics (a row whose label or group is out
 *     of range is not counted), and once per call, when counters is given: loss_log[counters[0]] = loss[0] when that
 *     index is below log_capacity (loss_log nullable), then counters[0] += 1, counters[1] += npat*batch.  confusion,
 *     loss_log and counters are nullable; loss_log needs counters, confusion needs n_groups >= 1, log_capacity >= 0;
 *   - an index outside [0, n_rows) behaves like an out-of-range label: NaN loss and gradients, the row is not counted,
 *     nothing is read out of bounds (the sample's input row reads as zeros, its label as -1).
 * Every-pattern mode is bitwise tspm_pattern_head_train_step on the explicitly gathered rows.  No floating-point
 * atomics; eager, captured and replayed calls are bitwise equal.  In addition to tspm_pattern_head_train_step's
 * limits: n_rows >= 1; ld_emb >= in and a multiple of 4; emb 16-byte aligned; rows, emb, labels_all given; row_keep and
 * row_group both given or both NULL.  The workspace is tspm_cached_head_train_workspace(batch, npat) bytes. */
typedef struct tspm_cached_head_train_desc {
  int32_t batch, npat, in, w_audio, hidden, hidden2, classes, ld_emb;
  int32_t gen_keep, n_groups;
  int64_t n_rows;
  const float* emb;            /* [n_rows, ld_emb] */
  const float* x0;             /* [in] */
  const int64_t* rows;         /* [batch] */
  const int64_t* labels_all;   /* [n_rows] */
  const int32_t* keep;         /* HOST [npat][2], every-pattern mode; NULL in per-sample mode */
  const int32_t* group_id;     /* HOST [npat], every-pattern mode */
  const uint8_t* row_keep;     /* DEVICE [batch][2], per-sample mode */
  const int32_t* row_group;    /* DEVICE [batch], per-sample mode */
  const float *w0, *b0, *w3, *b3, *w5, *b5;
  float p;                     /* dropout probability (0: no mask) */
  float loss_weight;
  uint64_t seed;
  const uint64_t* counter;
  uint8_t* keep_mask;          /* [npat*batch, hidden] */
  float* logits;               /* [npat*batch, classes] */
  float *gw0, *gb0, *gw3, *gb3, *gw5, *gb5;
  float *loss, *stats;         /* stats nullable */
  int64_t* adam_step;          /* nullable */
  int64_t* confusion;          /* nullable: [n_groups][classes][classes] */
  float* loss_log;             /* nullable */
  int64_t* counters;           /* nullable: {entries, samples} */
  int64_t log_capacity;
  void* workspace;             /* tspm_cached_head_train_workspace(batch, npat) bytes, 16-byte aligned */
  size_t workspace_bytes;
} tspm_cached_head_train_desc;
size_t tspm_cached_head_train_workspace(int32_t batch, int32_t npat);
int tspm_cached_head_train_step(const tspm_cached_head_train_desc* desc, tspm_stream_t stream);

/* tspm_cached_head_train_steps (added under ABI 23) — `steps` consecutive head-stage steps of a cached epoch in one
 * host call, Adam applied inside each step's weight-gradient launch.  For k = 0 .. steps-1 it enqueues one step that is
 * BITWISE tspm_cached_head_train_step followed by tspm_adam_step over the head's parameters, where step k reads
 *   rows + k*batch, and in per-sample mode row_keep + 2*k*batch and row_group + k*batch
 * (rows [steps*batch], row_keep [steps*batch][2], row_group [steps*batch]: an epoch's device-resident order, sliced on
 * the device) and every other field of desc is shared by all steps.  logits, loss, keep_mask and the six gradient
 * buffers hold the last step's values afterwards; stats, confusion, loss_log and counters accumulate one entry per
 * step, as `steps` single calls would.  The workspace is tspm_cached_head_train_workspace(batch, npat) bytes, reused
 * step after step.
 *
 * Two launches per step.  Launch 1 is tspm_cached_head_train_step's, in which one thread also stores the step in
 * flight, hyper->step + 1, to hyper->pad_ (a word nothing else in that launch touches).  Launch 2 walks the same four
 * weight-gradient products, one 32x32 tile per workgroup; the wave that stores a tile's gradients applies Adam — the
 * arithmetic of tspm_adam_step with the bias corrections of step hyper->pad_, formed once per workgroup — to the
 * parameter, exp_avg and exp_avg_sq at the gradient's flat offset, bias gradients included.  The gradient is still
 * stored.  Every element has one owner, nothing in launch 2 reads a weight or hyper->step, and the loss workgroup stores
 * hyper->pad_ to hyper->step at its end: hyper->step == old + steps after the call, and step k's dropout counter is
 * old + k when desc->counter is that word.  No clip coefficient.  No floating-point atomics; eager, captured and
 * replayed calls are bitwise equal.
 *
 * adam names the head's one flat Adam group: the six gradients desc->gw0 .. gb5 each lie inside [grad, grad + count),
 * and the matching desc->w0 .. b5 is param plus the same offset; desc->adam_step == &adam->hyper->step.  Refused with
 * TSPM_ERR_INVALID before any launch, nothing written: desc or adam NULL; steps < 1 or > TSPM_CACHED_HEAD_MAX_STEPS;
 * whatever tspm_cached_head_train_step refuses (TSPM_ERR_WORKSPACE for the workspace, as there); a NULL or
 * 16-byte-unaligned param, grad, exp_avg or exp_avg_sq; hyper NULL; count < 1; a gradient outside the range or a weight
 * at another offset; another adam_step. */
typedef struct tspm_head_adam_desc {
  float* param;
  float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t count;
  tspm_adam_hyper* hyper;      /* device; pad_ is written (the step in flight) */
} tspm_head_adam_desc;
#define TSPM_CACHED_HEAD_MAX_STEPS 64
int tspm_cached_head_train_steps(const tspm_cached_head_train_desc* desc, const tspm_head_adam_desc* adam,
                                 int32_t steps, tspm_stream_t stream);

/* All-pattern MMIMDb fusion (added under ABI 23) — tspm_gmu_fwd for EVERY missing-modality pattern of a batch in one
 * launch.  In eval mode an encoder's output row depends on that row's input and the weights only, and fc_one / fc_two
 * each act on one modality, so a zeroed modality is one constant half of the projection buffer: u [batch][ldu] holds
 * [fc_one(image) | fc_two(text)] of the real inputs, u0 [2d] that of an all-zero input.  For p < npat and b < batch,
 * row = p*batch + b:
 *   input[row]  = columns [0, d) of u[b] when keep[2p] != 0, else of u0; columns [d, 2d) by keep[2p + 1] likewise
 *   h[row], gate[row], z[row] = tspm_gmu_fwd's of that input row  (h [npat*batch][ldh] and gate [npat*batch] nullable:
 *                               evaluation needs neither and h is three quarters of the writes)
 * BITWISE what tspm_gmu_fwd writes for the explicitly expanded rows: one 256-thread workgroup per sample (at most 1024
 * workgroups, each walking its samples) forms tanh(u[b]) and tanh(u0) once in LDS (4d + 4 floats), then runs, per
 * pattern, tspm_gmu_fwd's own per-thread fmaf chain, block sum and mix.  A row depends on u[b], u0, wz and keep[p]
 * only — not on batch, npat or the other rows.  Plain loads and stores, no atomics; nothing but the named elements is
 * written (padding columns keep their content).  keep ([npat][2], the (image, text) flags, non-zero = the real input)
 * is a HOST array copied into the launch arguments, as in tspm_pattern_expand.  u0 may be NULL when every pattern
 * keeps both modalities.  TSPM_ERR_INVALID before any launch: batch <= 0, npat outside 1..TSPM_MAX_PATTERNS, a pattern
 * that keeps nothing, d outside 1..TSPM_GMU_PATTERN_MAX_D (the 64 KiB LDS carve: (4d + 4) floats), ldu < 2d, ldz < d,
 * ldh < 2d with h given, a NULL among keep / u / wz / z, a NULL u0 with a dropped modality. */
#define TSPM_GMU_PATTERN_MAX_D 4095
int tspm_gmu_pattern_fwd(int32_t batch, int32_t npat, const int32_t* keep, int32_t d, const float* u, int32_t ldu,
                         const float* u0, const float* wz, float* h, int32_t ldh, float* gate, float* z, int32_t ldz,
                         tspm_stream_t stream);
/* The adjoint of tspm_gmu_pattern_fwd (added under ABI 23), for training every pattern of a batch in one step: the
 * gradient of the P*batch fusion rows folded onto batch + 1 projection rows.  dz [npat*batch][lddz] is the gradient of
 * z; h [npat*batch][ldh] and gate [npat*batch] are what tspm_gmu_pattern_fwd wrote (both required here).  Per row
 * r = p*batch + b, with (ds_r, du_r[2d]) = what tspm_gmu_bwd computes for that row:
 *   ds[r]                  = ds_r   (the gate weight gradient stays tspm_linear_bwd_weight over the npat*batch rows)
 *   du[b][half]            = sum over the p that keep the half's modality of du_r[half]          (b < batch)
 *   du[batch][half]        = sum over every b and every p that drops the half's modality of du_r[half]
 * half = columns [0, d) (image, keep[2p]) or [d, 2d) (text, keep[2p + 1]); du [batch + 1][lddu].  Row batch is the
 * gradient of the one projection row every all-zero input shares (tspm_gmu_pattern_fwd's u0).  A slot no pattern uses
 * is written +0.0 (every pattern keeps both modalities: row batch is all +0.0).
 * Two launches.  (1) One 256-thread workgroup per sample (G = min(batch, 1024) workgroups, workgroup g walking samples
 * g, g + G, ...): per pattern tspm_gmu_bwd's per-thread fmaf chain, block sum and element expressions; a thread owns
 * columns tid, tid + 256, ... of both halves and keeps their sums in registers.  Order of every sum, all plain fp32 adds
 * from +0.0: du[b] over p ascending; workgroup g's zero-row partial over its samples b ascending and, within a sample,
 * p ascending.  The partials go to workspace [G][2d].  (2) Column c of du[batch] = ((s0 + s1) + s2) + s3 with s_q the
 * sum over g = q, q + 4, q + 8, ... ascending of partial g.  No floating-point atomics, no inter-workgroup hand-off
 * inside a launch; two calls on the same inputs are bitwise equal; rows b < batch depend on sample b's rows, wz and
 * keep only.  Nothing but the named elements is written (padding columns keep their content).  keep is a HOST array as
 * in tspm_gmu_pattern_fwd.  workspace: tspm_gmu_pattern_bwd_workspace(batch, d) bytes (0 for a refused shape), fully
 * overwritten by every call (no initialisation needed).  TSPM_ERR_INVALID before any launch: batch <= 0, npat outside
 * 1..TSPM_MAX_PATTERNS, a pattern that keeps nothing, d outside 1..TSPM_GMU_PATTERN_MAX_D, lddz < d, ldh < 2d,
 * lddu < 2d, a NULL among keep / dz / h / gate / wz / du / ds; a missing or short workspace with the other arguments
 * valid: TSPM_ERR_WORKSPACE. */
size_t tspm_gmu_pattern_bwd_workspace(int32_t batch, int32_t d);
int tspm_gmu_pattern_bwd(int32_t batch, int32_t npat, const int32_t* keep, int32_t d, const float* dz, int32_t lddz,
                         const float* h, int32_t ldh, const float* gate, const float* wz, float* du, int32_t lddu,
                         float* ds, void* workspace, size_t workspace_bytes, tspm_stream_t stream);
/* tspm_bce_logits for every pattern of a batch in one call (added under ABI 23; no gradient): logits
 * [npat*batch][classes] (row p*batch + b), targets [batch][classes] shared by the patterns (not replicated).  Workgroup
 * p runs tspm_bce_logits' code on its row slice: loss[p] and stats[p] (stats [npat][3 + 3*classes], tspm_bce_logits'
 * layout, ACCUMULATED into; nullable) are BITWISE what npat calls of tspm_bce_logits on the slices leave.  Then, once
 * per call and when counters (int64 {entries, samples}) is given, a one-thread launch writes
 * loss_log[counters[0] + p] = loss[p] for every p with that index below log_capacity (loss_log nullable) and adds
 * npat to counters[0] and npat*batch to counters[1] — tspm_pattern_head_eval's log semantics.  No floating-point
 * atomics; two calls on the same inputs are bitwise equal.  TSPM_ERR_INVALID before any launch: batch <= 0, npat
 * outside 1..TSPM_MAX_PATTERNS, classes <= 0, a NULL among logits / targets / loss, loss_log without counters,
 * log_capacity < 0. */
int tspm_bce_logits_patterns(int32_t batch, int32_t npat, int32_t classes, const float* logits, const float* targets,
                             float grad_scale, float threshold, float* loss, float* stats, float* loss_log,
                             int64_t* counters, int64_t log_capacity, tspm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Monomodal pre-training head (ABI 23) — train_monomodal.MonomodalEncoder's `classifier = nn.Linear(hid,
 * classes)` forward, the loss group's weighted cross-entropy, the argmax(logits, 1) predictions
 * (train_monomodal.py:236,394) and the Linear's whole backward in ONE launch, for the launch-bound MOSI / MOSEI
 * encoder pre-training step ([128,64] x [64,3]).  Semantics of tspm_linear_fwd + tspm_cross_entropy +
 * tspm_linear_bwd up to summation order: logits = emb w^T + b; loss[0] = loss_weight * mean CE;
 * dlogits = (softmax - onehot)/n * loss_weight; dw = dlogits^T emb, db = column sums of dlogits,
 * demb = dlogits w (all overwritten); an out-of-range label gives NaN loss and gradients (no out-of-bounds read)
 * and is never counted in stats[1].
 * One workgroup walks the rows in chunks of 64 with the embeddings staged in LDS and reduces in a fixed order:
 * no atomics, no workspace, two runs on the same input are bitwise equal; forward-only mode (dw, db and demb all
 * NULL) gives bitwise the training mode's logits, loss and preds.
 * Limits: 1 <= n <= 1024; hid <= 128 and a multiple of 4; classes <= 16; ld_emb, ld_demb >= hid and multiples of
 * 4 with emb / demb 16-byte aligned; dw, db, demb all given or all NULL; otherwise TSPM_ERR_INVALID. */
typedef struct tspm_mono_head_desc {
  int32_t n, hid, classes, ld_emb, ld_demb;
  float loss_weight;     /* the cross-entropy term's weight (tspm_cross_entropy's grad_scale) */
  const float* emb;      /* [n, ld_emb] */
  const float* w;        /* [classes, hid] */
  const float* b;        /* [classes] */
  const int64_t* labels; /* [n] */
  float* logits;         /* [n, classes] */
  float* loss;           /* loss[0] */
  int64_t* preds;        /* nullable: first maximum of the logits (TSPM_ARGMAX_LOGITS) */
  float* dw;             /* [classes, hid] */
  float* db;             /* [classes] */
  float* demb;           /* [n, ld_demb] */
  float* stats;          /* nullable: the three accumulators of tspm_cross_entropy */
} tspm_mono_head_desc;
int tspm_mono_head_step(const tspm_mono_head_desc* desc, tspm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Multi-label monomodal head (added under ABI 23) — the same head around an MMIMDbModalityEncoder (hid 512, 23 genres,
 * float multi-hot targets): `classifier` forward, the loss group's weighted BCEWithLogits, the predictions
 * sigmoid(x) > threshold, the F1 accumulators and the Linear's whole backward in ONE launch.  Semantics of
 * tspm_linear_fwd + tspm_bce_logits + tspm_linear_bwd up to summation order: logits = emb w^T + b;
 * loss[0] = loss_weight * mean((1-t)*x - logsigmoid(x)); dlogits = (sigmoid(x) - t) * loss_weight / (n*classes);
 * dw = dlogits^T emb, db = column sums of dlogits, demb = dlogits w (all overwritten; padding columns of demb
 * untouched).  stats (nullable) has tspm_bce_logits' layout and accumulate-into semantics (3 + 3*classes floats).
 * Rows are spread over up to 16 workgroups (chunks of up to 16 rows staged in LDS); each publishes its partial dw / db /
 * loss / counts in the workspace and the last arriver adds them in workgroup order: no float atomics, every sum
 * in a fixed order, two runs on the same input are bitwise equal; forward-only mode (dw, db and demb all NULL)
 * gives bitwise the training mode's logits, loss, preds and stats.
 * workspace: tspm_mono_head_bce_workspace(n, hid, classes) bytes, 16-byte aligned, its first 64 bytes (the arrival
 * counter) zero before the first launch that uses it (the kernel re-arms it); one workspace serves one stream.
 * Limits: 1 <= n <= 1024; hid <= 512 and a multiple of 4; 1 <= classes <= 32; ld_emb, ld_demb >= hid and multiples
 * of 4 with emb / demb 16-byte aligned; dw, db, demb all given or all NULL; otherwise TSPM_ERR_INVALID (a missing or
 * short workspace with the other arguments valid: TSPM_ERR_WORKSPACE) with nothing written. */
typedef struct tspm_mono_head_bce_desc {
  int32_t n, hid, classes, ld_emb, ld_demb;
  float loss_weight;    /* the bce_with_logits term's weight (tspm_bce_logits' grad_scale) */
  float threshold;      /* prediction = sigmoid(x) > threshold */
  const float* emb;     /* [n, ld_emb] */
  const float* w;       /* [classes, hid] */
  const float* b;       /* [classes] */
  const float* targets; /* [n, classes] multi-hot */
  float* logits;        /* [n, classes] */
  float* loss;          /* loss[0] */
  uint8_t* preds;       /* nullable: [n, classes] */
  float* dw;            /* [classes, hid] */
  float* db;            /* [classes] */
  float* demb;          /* [n, ld_demb] */
  float* stats;         /* nullable: tspm_bce_logits' accumulators */
  void* workspace;
  size_t workspace_bytes;
} tspm_mono_head_bce_desc;
size_t tspm_mono_head_bce_workspace(int32_t n, int32_t hid, int32_t classes);
int tspm_mono_head_bce_step(const tspm_mono_head_bce_desc* desc, tspm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Regression head (added under ABI 23) — the scalar-output head Linear(hid, 1) of the CMU-MOSI / CMU-MOSEI sentiment
 * regression (continuous score in [-3, 3]): FcClassifier.fc_out of the fusion model (hid 32 / 48) or the
 * MonomodalEncoder's classifier (hid 64), with a float32 label per row, in ONE launch of ONE workgroup:
 *   pred[r] = emb[r] . w + b;  e_r = pred[r] - labels[r];  loss[0] = loss_weight * mean_r l(e_r)
 *   kind TSPM_REGRESS_L1:  l = |e|,  dpred = loss_weight * sign(e) / n   (sign(0) = 0, as torch)
 *   kind TSPM_REGRESS_MSE: l = e^2,  dpred = loss_weight * 2 e / n
 *   dw = sum_r dpred_r emb[r],  db = sum_r dpred_r,  demb[r] = dpred_r w   (all overwritten; padding columns of demb
 *   untouched).  Forward-only mode (dw, db and demb all NULL) gives bitwise the training mode's pred and loss.
 * stats (nullable): one tspm_regress_stats record per pattern group, g = groups ? groups[r] : 0; the call ADDS to
 * every field over its rows.  e for the sums is (double)pred - (double)label.  conf7 is indexed
 * [rintf(clip(y,-3,3)) + 3][rintf(clip(p,-3,3)) + 3] (half-to-even, numpy's round); sign3 by the sign of y and of p
 * (0 negative, 1 zero, 2 positive; compared in fp32).  Acc-7 / Acc-5 / Acc-3 follow from conf7 (clipping to +-2 or
 * +-1 after rounding equals rounding after that clip), both binary tasks from sign3, MAE and Pearson's r from the
 * sums.  A row whose label or prediction is NaN, or whose group is outside [0, n_groups), is left out of every
 * field (it still makes the loss NaN), as tspm_classify_update leaves out an out-of-range label.
 * counters (nullable), once per call: loss_log[counters[0]] = loss[0] (if loss_log and counters[0] < log_capacity),
 * counters[0] += 1, counters[1] += n — tspm_classify_update's log.
 * The rows are walked in chunks of 64 staged in LDS; the loss and the seven sums run in double in a fixed order: no
 * atomics, no workspace, two runs on the same input are bitwise equal and k calls add the same bits to the
 * accumulators in every run.
 * Limits: 1 <= n <= 1024; hid <= 128 and a multiple of 4; ld_emb, ld_demb >= hid and multiples of 4 with emb / demb
 * 16-byte aligned; dw, db, demb all given or all NULL; kind 0 or 1; with stats 1 <= n_groups <= 16; loss_log needs
 * counters; otherwise TSPM_ERR_INVALID before any launch. */
#define TSPM_REGRESS_L1 0
#define TSPM_REGRESS_MSE 1
typedef struct tspm_regress_stats { /* 66 8-byte words */
  int64_t n;                                                     /* rows counted */
  double sum_abs, sum_sq, sum_p, sum_y, sum_pp, sum_yy, sum_py;  /* sum |e|, e^2, p, y, p^2, y^2, p y */
  int64_t conf7[7][7];                                           /* [rounded clipped label + 3][... prediction + 3] */
  int64_t sign3[3][3];                                           /* [sign of label][sign of prediction] */
} tspm_regress_stats;
typedef struct tspm_regress_head_desc {
  int32_t n, hid, ld_emb, ld_demb, kind, n_groups;
  float loss_weight;         /* the loss term's weight */
  int32_t reserved_;
  const float* emb;          /* [n, ld_emb] */
  const float* w;            /* [1, hid] */
  const float* b;            /* [1] */
  const float* labels;       /* [n] */
  const int32_t* groups;     /* nullable: [n] */
  float* pred;               /* [n] (= logits [n, 1]) */
  float* loss;               /* loss[0] */
  float* dw;                 /* [1, hid] */
  float* db;                 /* [1] */
  float* demb;               /* [n, ld_demb] */
  tspm_regress_stats* stats; /* nullable: [n_groups] */
  float* loss_log;           /* nullable: [log_capacity] */
  int64_t* counters;         /* nullable: {batches, samples} */
  int64_t log_capacity;
} tspm_regress_head_desc;
int tspm_regress_head_step(const tspm_regress_head_desc* desc, tspm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TSPM_H_ */
