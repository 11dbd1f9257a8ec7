// MMIMDb late-fusion path (BASELINE configs[3]): the element-wise and row-reduction
// pieces around the small GEMMs —
//   * GatedBiModalNetwork (MML_Suite/models/gates/gated_bimodal.py): tanh of both projections, the
//     scalar gate sigmoid(w_z · [h1, h2]) per row, and z = g*h1 + (1-g)*h2, plus its backward;
//   * MaxOut(num_units=2, no bias) (models/maxout.py) fused with the Dropout(0.5) that follows it in
//     MLPGenreClassifier (models/mmimdb.py:38-47), plus the backward of torch.maximum (ties split the
//     gradient in half, as ATen's derivative of maximum does);
//   * BCEWithLogitsLoss(mean) (experiment_utils/loss.py:52) with on-device multilabel counts for the
//     f1_{samples,macro,weighted,micro} metrics of configs/mmimdb/centralised/mmimdb_baseline.yaml
//     (prediction = sigmoid(x) > threshold, models/mmimdb.py:236-237);
//   * the GMU forward and that loss for every missing-modality pattern of a batch in one call each
//     (k_gmu_pattern_fwd, k_bce_logits_patterns: bitwise the per-row / per-pattern kernels above);
//   * training every pattern of a batch in one step: the encoders' input BatchNorm1d over the replicated batch from its
//     distinct rows (k_bn1d_fwd_rep*), and the GMU backward folded onto batch + 1 projection rows (k_gmu_pattern_bwd*).
// Every kernel is HBM/latency bound (a few hundred KB per launch); rows map to workgroups so the
// row reductions are wave shuffles + one LDS step in a fixed order (deterministic).
#include "common.h"

namespace {

constexpr int kRowThreads = 256;
constexpr int kLossThreads = 1024;
constexpr int kGmuPatternGrid = 1024;  // k_gmu_pattern_fwd: at most this many workgroups, each walking its samples

// Block-wide sum in a fixed order: wave shuffle tree, then wave 0 adds the 4 wave totals.
template <int NT = kRowThreads>
TSPM_DEV float block_sum(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) t += red[w];
  return t;
}

// One workgroup per row.  u: [n, 2d] (fc_one output in columns [0,d), fc_two output in [d,2d)).
__global__ __launch_bounds__(kRowThreads) void k_gmu_fwd(int d, const float* __restrict__ u, int ldu,
                                                         const float* __restrict__ wz, float* __restrict__ h,
                                                         int ldh, float* __restrict__ gate, float* __restrict__ z,
                                                         int ldz) {
  __shared__ float red[kRowThreads / 64];
  const long long r = blockIdx.x;
  const float* ur = u + r * ldu;
  float* hr = h + r * ldh;
  float s = 0.f;
  for (int j = threadIdx.x; j < 2 * d; j += kRowThreads) {
    const float t = tanhf(ur[j]);
    hr[j] = t;
    s = fmaf(wz[j], t, s);
  }
  s = block_sum(s, red);
  const float g = 1.f / (1.f + expf(-s));
  if (threadIdx.x == 0) gate[r] = g;
  const float g1 = 1.f - g;
  float* zr = z + r * ldz;
  for (int j = threadIdx.x; j < d; j += kRowThreads) zr[j] = g * hr[j] + g1 * hr[d + j];
}

// dz -> du [n,2d] (through gate and tanh) and ds[n] = d(loss)/d(gate pre-activation) (the weight
// gradient of hidden_sigmoid is then ds^T @ h, a small GEMM).
__global__ __launch_bounds__(kRowThreads) void k_gmu_bwd(int d, const float* __restrict__ dz, int lddz,
                                                         const float* __restrict__ h, int ldh,
                                                         const float* __restrict__ gate,
                                                         const float* __restrict__ wz, float* __restrict__ du,
                                                         int lddu, float* __restrict__ ds) {
  __shared__ float red[kRowThreads / 64];
  const long long r = blockIdx.x;
  const float* hr = h + r * ldh;
  const float* dzr = dz + r * lddz;
  float a = 0.f;
  for (int j = threadIdx.x; j < d; j += kRowThreads) a = fmaf(dzr[j], hr[j] - hr[d + j], a);
  a = block_sum(a, red);
  const float g = gate[r];
  const float dsv = a * g * (1.f - g);
  if (threadIdx.x == 0) ds[r] = dsv;
  float* dur = du + r * lddu;
  for (int j = threadIdx.x; j < d; j += kRowThreads) {
    const float h1 = hr[j], h2 = hr[d + j];
    const float d1 = fmaf(dsv, wz[j], g * dzr[j]);
    const float d2 = fmaf(dsv, wz[d + j], (1.f - g) * dzr[j]);
    dur[j] = d1 * (1.f - h1 * h1);
    dur[d + j] = d2 * (1.f - h2 * h2);
  }
}

// y[r,j] = max(a[r,j], a[r,d+j]) [* (keep ? scale : 0)]
__global__ __launch_bounds__(256) void k_maxout_fwd(int n, int d, const float* __restrict__ a, int lda,
                                                    const uint8_t* __restrict__ keep, float scale,
                                                    float* __restrict__ y, int ldy) {
  const long long total = (long long)n * d;
  for (long long t = blockIdx.x * 256LL + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
    const long long r = t / d;
    const int j = (int)(t - r * d);
    const float a0 = a[r * lda + j], a1 = a[r * lda + d + j];
    float v = (a1 > a0 || a1 != a1) ? a1 : a0;  // NaN in either unit propagates (torch.max)
    if (keep) v = v * (keep[t] ? scale : 0.f);
    y[r * ldy + j] = v;
  }
}

// MaxOut forward that draws its dropout mask in-launch (the bits tspm_dropout_mask would write for
// elements index_offset + t) and stores it for the backward.
__global__ __launch_bounds__(256) void k_maxout_fwd_rng(int n, int d, const float* __restrict__ a, int lda, float p,
                                                        uint64_t seed, const uint64_t* __restrict__ ctr,
                                                        long long index_offset, uint8_t* __restrict__ keep,
                                                        float scale, float* __restrict__ y, int ldy) {
  const uint64_t base = tspm_dropout_base(seed, ctr ? *ctr : 0ULL);
  const long long total = (long long)n * d;
  for (long long t = blockIdx.x * 256LL + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
    const long long r = t / d;
    const int j = (int)(t - r * d);
    const float a0 = a[r * lda + j], a1 = a[r * lda + d + j];
    const bool k = tspm_dropout_keep(base, index_offset + t, p);
    keep[t] = k ? 1 : 0;
    const float v = (a1 > a0 || a1 != a1) ? a1 : a0;  // NaN in either unit propagates (torch.max)
    y[r * ldy + j] = v * (k ? scale : 0.f);
  }
}

__global__ __launch_bounds__(256) void k_maxout_bwd(int n, int d, const float* __restrict__ dy, int lddy,
                                                    const float* __restrict__ a, int lda,
                                                    const uint8_t* __restrict__ keep, float scale,
                                                    float* __restrict__ da, int ldda) {
  const long long total = (long long)n * d;
  for (long long t = blockIdx.x * 256LL + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
    const long long r = t / d;
    const int j = (int)(t - r * d);
    float g = dy[r * lddy + j];
    if (keep) g = g * (keep[t] ? scale : 0.f);
    const float a0 = a[r * lda + j], a1 = a[r * lda + d + j];
    const float half = 0.5f * g;
    // torch.maximum's derivative: where(a0 == a1, g/2, g) masked to 0 where the unit is the smaller one
    // (so a NaN in either unit sends the full gradient to both, as ATen does)
    da[r * ldda + j] = a0 == a1 ? half : (a0 < a1 ? 0.f : g);
    da[r * ldda + d + j] = a0 == a1 ? half : (a1 < a0 ? 0.f : g);
  }
}

// One workgroup's BCEWithLogits over n rows: loss (mean over n*c), dlogits, and the metric counts.  The body of
// k_bce_logits (the whole batch) and of k_bce_logits_patterns (one pattern's row slice per workgroup): one
// statement list, so both sum and contract alike.
TSPM_DEV void bce_logits_rows(int n, int c, const float* __restrict__ x, const float* __restrict__ t,
                              float* __restrict__ loss, float* __restrict__ dx, float grad_scale, float threshold,
                              float* __restrict__ stats, float* red) {
  const long long total = (long long)n * c;
  const float inv = 1.f / (float)total;
  float acc = 0.f;
  for (long long i = threadIdx.x; i < total; i += kLossThreads) {
    const float xv = x[i], tv = t[i];
    // ATen: (1 - t) * x - log_sigmoid(x),  log_sigmoid(x) = min(x, 0) - log1p(exp(-|x|))
    const float ls = fminf(xv, 0.f) - log1pf(expf(-fabsf(xv)));
    acc += (1.f - tv) * xv - ls;
    if (dx) dx[i] = (1.f / (1.f + expf(-xv)) - tv) * inv * grad_scale;
  }
  const float sum = block_sum<kLossThreads>(acc, red);
  const float mean = sum * inv * grad_scale;
  if (threadIdx.x == 0) {
    loss[0] = mean;
    if (stats) {
      stats[0] += mean * (float)n;
      stats[1] += (float)n;
    }
  }
  if (!stats) return;
  // stats[2] += sum over rows of the per-sample F1 (zero_division = 0); per class k:
  // stats[3+3k+{0,1,2}] += tp, fp, fn.  Thread-exclusive slots, so plain read-modify-write.
  float f1 = 0.f;
  for (int r = threadIdx.x; r < n; r += kLossThreads) {
    int tp = 0, fp = 0, fn = 0;
    for (int k = 0; k < c; ++k) {
      const bool p = 1.f / (1.f + expf(-x[(long long)r * c + k])) > threshold;
      const bool y = t[(long long)r * c + k] > 0.5f;
      tp += p && y;
      fp += p && !y;
      fn += !p && y;
    }
    const int den = 2 * tp + fp + fn;
    f1 += den > 0 ? (2.f * tp) / (float)den : 0.f;
  }
  const float f1s = block_sum<kLossThreads>(f1, red);
  if (threadIdx.x == 0) stats[2] += f1s;
  for (int k = threadIdx.x; k < c; k += kLossThreads) {
    float tp = 0.f, fp = 0.f, fn = 0.f;
    for (int r = 0; r < n; ++r) {
      const bool p = 1.f / (1.f + expf(-x[(long long)r * c + k])) > threshold;
      const bool y = t[(long long)r * c + k] > 0.5f;
      tp += (p && y) ? 1.f : 0.f;
      fp += (p && !y) ? 1.f : 0.f;
      fn += (!p && y) ? 1.f : 0.f;
    }
    stats[3 + 3 * k] += tp;
    stats[4 + 3 * k] += fp;
    stats[5 + 3 * k] += fn;
  }
}

// Single workgroup: the whole batch.
__global__ __launch_bounds__(kLossThreads) void k_bce_logits(int n, int c, const float* __restrict__ x,
                                                            const float* __restrict__ t, float* __restrict__ loss,
                                                            float* __restrict__ dx, float grad_scale, float threshold,
                                                            float* __restrict__ stats) {
  __shared__ float red[kLossThreads / 64];
  bce_logits_rows(n, c, x, t, loss, dx, grad_scale, threshold, stats, red);
}

// Every missing-modality pattern of a batch: workgroup p runs k_bce_logits' code on rows [p*n, (p+1)*n) of x against
// the n target rows all patterns share, into loss[p] and stats[p] (3 + 3c floats each).
__global__ __launch_bounds__(kLossThreads) void k_bce_logits_patterns(int n, int c, const float* __restrict__ x,
                                                                     const float* __restrict__ t,
                                                                     float* __restrict__ loss, float grad_scale,
                                                                     float threshold, float* __restrict__ stats) {
  __shared__ float red[kLossThreads / 64];
  const long long p = blockIdx.x;
  bce_logits_rows(n, c, x + p * n * c, t, loss + p, nullptr, grad_scale, threshold,
                  stats ? stats + p * (3 + 3 * c) : nullptr, red);
}

// The loss log of one all-pattern call (tspm_pattern_head_eval's semantics): P entries in pattern order, then the
// counters.  One thread; runs after k_bce_logits_patterns in the same stream.
__global__ __launch_bounds__(64) void k_pattern_loss_log(int npat, long long rows, const float* __restrict__ loss,
                                                         float* __restrict__ loss_log, long long* __restrict__ counters,
                                                         long long cap) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const long long base = counters[0];
  if (loss_log)
    for (int p = 0; p < npat; ++p)
      if (base + p >= 0 && base + p < cap) loss_log[base + p] = loss[p];
  counters[0] = base + npat;
  counters[1] += rows;
}

// tspm_gmu_fwd for every missing-modality pattern of a batch.  u [batch, ldu] holds the projections of the real
// inputs, u0 [2d] those of an all-zero input (one constant row in eval mode); row p*batch + b takes its image half
// (columns [0, d)) from u[b] or u0 and its text half likewise.  One workgroup per sample (walking samples above the
// grid cap): tanh(u[b]) and tanh(u0) once into LDS, then per pattern k_gmu_fwd's own fmaf chain over
// j = tid, tid + 256, ..., its block_sum and its mix line — so every row is bitwise what k_gmu_fwd writes for the
// explicitly expanded row.  LDS: 4d + 4 floats.
struct GmuPatternSet {
  int keep[TSPM_MAX_PATTERNS];  // bit 0: the image half comes from u[b], bit 1: the text half
};

__global__ __launch_bounds__(kRowThreads) void k_gmu_pattern_fwd(int batch, int npat, GmuPatternSet ps, int d,
                                                                 const float* __restrict__ u, int ldu,
                                                                 const float* __restrict__ u0,
                                                                 const float* __restrict__ wz, float* __restrict__ h,
                                                                 int ldh, float* __restrict__ gate,
                                                                 float* __restrict__ z, int ldz) {
  extern __shared__ __attribute__((aligned(16))) float gmu_lds[];  // no static LDS in this kernel: the base stays aligned
  float* th = gmu_lds;           // tanh(u[b])  [2d]
  float* th0 = gmu_lds + 2 * d;  // tanh(u0)    [2d]
  float* red = gmu_lds + 4 * d;  // block_sum's wave totals
  for (int j = threadIdx.x; j < 2 * d; j += kRowThreads) th0[j] = u0 ? tanhf(u0[j]) : 0.f;
  for (int b = blockIdx.x; b < batch; b += gridDim.x) {
    const float* ur = u + (long long)b * ldu;
    for (int j = threadIdx.x; j < 2 * d; j += kRowThreads) th[j] = tanhf(ur[j]);
    __syncthreads();
    for (int p = 0; p < npat; ++p) {
      const float* h1 = (ps.keep[p] & 1) ? th : th0;
      const float* h2 = ((ps.keep[p] & 2) ? th : th0) + d;
      const long long r = (long long)p * batch + b;
      float s = 0.f;
      for (int j = threadIdx.x; j < 2 * d; j += kRowThreads) {
        const float t = j < d ? h1[j] : h2[j - d];
        if (h) h[r * ldh + j] = t;
        s = fmaf(wz[j], t, s);
      }
      s = block_sum(s, red);
      const float g = 1.f / (1.f + expf(-s));
      if (gate && threadIdx.x == 0) gate[r] = g;
      const float g1 = 1.f - g;
      float* zr = z + r * ldz;
      for (int j = threadIdx.x; j < d; j += kRowThreads) zr[j] = g * h1[j] + g1 * h2[j];
    }
    __syncthreads();  // every wave is done with th before the next sample overwrites it
  }
}

// The adjoint of k_gmu_pattern_fwd, folded onto batch + 1 rows.  One workgroup per sample (walking samples above the
// grid cap, like the forward): per pattern p it runs k_gmu_bwd's statement list on row p*batch + b — the same fmaf
// chain over j = tid, tid + 256, ..., the same block_sum — writes ds[row], and adds the row's two du halves to the
// sample's register accumulators (a half the pattern keeps) or to the workgroup's zero-row accumulators (a half it
// drops), in ascending p from +0.0.  TRIPS = ceil(d / 256) elements per thread and half, a template parameter so the
// accumulators stay in registers.  The sample's sums go to du[b]; the zero-row sums, carried across the workgroup's
// samples b = g, g + G, ... in ascending order, go to part[g][2d] for k_gmu_pattern_bwd_zero.  No LDS beyond block_sum's.
template <int TRIPS>
__global__ __launch_bounds__(kRowThreads) void k_gmu_pattern_bwd(int batch, int npat, GmuPatternSet ps, int d,
                                                                 const float* __restrict__ dz, int lddz,
                                                                 const float* __restrict__ h, int ldh,
                                                                 const float* __restrict__ gate,
                                                                 const float* __restrict__ wz, float* __restrict__ du,
                                                                 int lddu, float* __restrict__ ds,
                                                                 float* __restrict__ part) {
  __shared__ float red[kRowThreads / 64];
  float zi[TRIPS], zt[TRIPS];
#pragma unroll
  for (int t = 0; t < TRIPS; ++t) zi[t] = zt[t] = 0.f;
  for (int b = blockIdx.x; b < batch; b += gridDim.x) {
    float ai[TRIPS], at[TRIPS];
#pragma unroll
    for (int t = 0; t < TRIPS; ++t) ai[t] = at[t] = 0.f;
    for (int p = 0; p < npat; ++p) {
      const long long r = (long long)p * batch + b;
      const float* hr = h + r * ldh;
      const float* dzr = dz + r * lddz;
      float a = 0.f;
#pragma unroll
      for (int t = 0; t < TRIPS; ++t) {
        const int j = threadIdx.x + t * kRowThreads;
        if (j < d) a = fmaf(dzr[j], hr[j] - hr[d + j], a);
      }
      a = block_sum(a, red);
      const float g = gate[r];
      const float dsv = a * g * (1.f - g);
      if (threadIdx.x == 0) ds[r] = dsv;
      const bool ki = ps.keep[p] & 1, kt = ps.keep[p] & 2;  // uniform: kernel arguments
#pragma unroll
      for (int t = 0; t < TRIPS; ++t) {
        const int j = threadIdx.x + t * kRowThreads;
        if (j < d) {
          const float h1 = hr[j], h2 = hr[d + j];
          const float d1 = fmaf(dsv, wz[j], g * dzr[j]);
          const float d2 = fmaf(dsv, wz[d + j], (1.f - g) * dzr[j]);
          const float v1 = d1 * (1.f - h1 * h1), v2 = d2 * (1.f - h2 * h2);
          if (ki) ai[t] += v1; else zi[t] += v1;
          if (kt) at[t] += v2; else zt[t] += v2;
        }
      }
    }
    float* dur = du + (long long)b * lddu;
#pragma unroll
    for (int t = 0; t < TRIPS; ++t) {
      const int j = threadIdx.x + t * kRowThreads;
      if (j < d) {
        dur[j] = ai[t];
        dur[d + j] = at[t];
      }
    }
  }
  float* pr = part + (long long)blockIdx.x * 2 * d;
#pragma unroll
  for (int t = 0; t < TRIPS; ++t) {
    const int j = threadIdx.x + t * kRowThreads;
    if (j < d) {
      pr[j] = zi[t];
      pr[d + j] = zt[t];
    }
  }
}

// The zero row of tspm_gmu_pattern_bwd: column c of out = ((s0 + s1) + s2) + s3, s_q = the sum from +0.0 over the
// workgroup partials g = q, q + 4, q + 8, ... (ascending) of part[g][c].  64 columns x 4 partial groups per workgroup;
// a launch of its own, after k_gmu_pattern_bwd in the same stream, so it reads finished partials.
constexpr int kGmuZeroCols = 64, kGmuZeroGroups = 4;
__global__ __launch_bounds__(kGmuZeroCols * kGmuZeroGroups) void k_gmu_pattern_bwd_zero(int nparts, int width,
                                                                                      const float* __restrict__ part,
                                                                                      float* __restrict__ out) {
  __shared__ float s[kGmuZeroGroups][kGmuZeroCols];
  const int cl = threadIdx.x % kGmuZeroCols, q = threadIdx.x / kGmuZeroCols;
  const int c = blockIdx.x * kGmuZeroCols + cl;
  float v = 0.f;
  if (c < width)
    for (int g = q; g < nparts; g += kGmuZeroGroups) v += part[(long long)g * width + c];
  s[q][cl] = v;
  __syncthreads();
  if (q == 0 && c < width) out[c] = ((s[0][cl] + s[1][cl]) + s[2][cl]) + s[3][cl];
}

// BatchNorm1d over [m, c] rows in ONE launch each way (m = the batch, at most a few thousand rows on
// this path): one workgroup per kBnCh channels, kBnGroups row groups — lane = channel, so every row
// read is one coalesced segment; two-pass statistics (sum, then centred squares), row groups
// combined through LDS in a fixed order (deterministic).  Replaces the stats/finalize/apply triple
// (forward) and the partial/apply pair (backward) used for BatchNorm2d, whose launch overhead
// dominates at these sizes.
#ifndef TSPM_BN1D_CH
#define TSPM_BN1D_CH 32
#endif
// 1024 threads: 32 channels (one 128-byte line per row) x 32 row groups keep the per-lane row chain
// short and put c/32 workgroups on the chip (64 channels x 16 groups: 6.2-6.8 us per launch at c=512)
constexpr int kBnCh = TSPM_BN1D_CH, kBnGroups = 1024 / TSPM_BN1D_CH;

// Per-channel sums of the row groups, in double and in fixed group order.  BatchNorm1d runs over as
// few as 4 rows here, where the backward's projection (g - mean(g) - xhat * mean(g xhat)) cancels
// most of g: the statistics and sums are formed in double (as ATen's CPU kernels accumulate) so the
// cancellation does not amplify fp32 rounding.
TSPM_DEV double bn_group_sum(double v, double* red) {
  const int ch = threadIdx.x % kBnCh, grp = threadIdx.x / kBnCh;
  __syncthreads();
  red[grp * kBnCh + ch] = v;
  __syncthreads();
  // one row group forms each channel's total (same order as before) and publishes it: every thread
  // summing all kBnGroups doubles itself read 256 KB of LDS per call (≈ 1 µs at these sizes)
  if (grp == 0) {
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < kBnGroups; ++q) t += red[q * kBnCh + ch];
    red[ch] = t;
  }
  __syncthreads();
  return red[ch];
}

struct Bn1dFwd {
  int c;
  const float* x;
  const float* gamma;
  const float* beta;
  float* rmean;
  float* rvar;
  float momentum, eps;
  float* smean;
  float* sinvstd;
  float* y;
  const uint8_t* keep;  // optional Dropout after the BN (tspm_bn1d_fwd_drop): y *= keep ? keep_scale : 0
  float keep_scale;
};

// DROP: the Dropout-after-BN variant (tspm_bn1d_fwd_drop) — a template parameter so the plain
// BatchNorm1d launches compile exactly as before (a runtime branch in the row loop cost them 1-2 us).
template <bool DROP = false>
TSPM_DEV void bn1d_fwd_body(int m, const Bn1dFwd& p, int bid, double* red);

template <bool DROP>
__global__ __launch_bounds__(kBnCh * kBnGroups) void k_bn1d_fwd(int m, Bn1dFwd p) {
  __shared__ double red[kBnCh * kBnGroups];
  bn1d_fwd_body<DROP>(m, p, blockIdx.x, red);
}

// Two independent BatchNorm1d layers over the same rows (the MMIMDb image and text encoders' input
// BNs) in one launch: blocks [0, nb0) take p0.
__global__ __launch_bounds__(kBnCh * kBnGroups) void k_bn1d_fwd2(int m, Bn1dFwd p0, Bn1dFwd p1, int nb0) {
  __shared__ double red[kBnCh * kBnGroups];
  if ((int)blockIdx.x < nb0)
    bn1d_fwd_body(m, p0, blockIdx.x, red);
  else
    bn1d_fwd_body(m, p1, blockIdx.x - nb0, red);
}

template <bool DROP>
TSPM_DEV void bn1d_fwd_body(int m, const Bn1dFwd& p, int bid, double* red) {
  const int c = p.c;
  const float* __restrict__ x = p.x;
  const float momentum = p.momentum, eps = p.eps;
  float* __restrict__ rmean = p.rmean;
  float* __restrict__ rvar = p.rvar;
  const int ch = bid * kBnCh + threadIdx.x % kBnCh, grp = threadIdx.x / kBnCh;
  const bool ok = ch < c;
  double s = 0.0;
  if (ok)
#pragma unroll 4
    for (int r = grp; r < m; r += kBnGroups) s += (double)x[(long long)r * c + ch];
  const double meand = bn_group_sum(s, red) / (double)m;
  double q = 0.0;
  if (ok)
#pragma unroll 4
    for (int r = grp; r < m; r += kBnGroups) {
      const double d = (double)x[(long long)r * c + ch] - meand;
      q = fma(d, d, q);
    }
  const double m2 = bn_group_sum(q, red);
  const float mean = (float)meand;
  const float invstd = (float)(1.0 / sqrt(m2 / (double)m + (double)eps));
  if (!ok) return;
  if (grp == 0) {
    p.smean[ch] = mean;
    p.sinvstd[ch] = invstd;
    if (rmean) rmean[ch] = (1.f - momentum) * rmean[ch] + momentum * mean;
    if (rvar) rvar[ch] = (1.f - momentum) * rvar[ch] + momentum * (float)(m > 1 ? m2 / (double)(m - 1) : m2);
  }
  const float ga = p.gamma[ch], be = p.beta[ch];
  for (int r = grp; r < m; r += kBnGroups) {
    const long long i = (long long)r * c + ch;
    const float v = (x[i] - mean) * invstd * ga + be;
    p.y[i] = (DROP && p.keep) ? v * (p.keep[i] ? p.keep_scale : 0.f) : v;
  }
}

// BatchNorm1d over a batch that holds each of the m rows of x `reps` times and, per row of x, `zrows` all-zero rows
// (every missing-modality pattern of a batch in one train step: the patterns that keep the modality, the patterns that
// drop it) — the statistics of those N = m*(reps + zrows) rows from the m real rows alone, per channel with S = sum x:
//   mean = reps*S / N,  M2 = reps*sum (x - mean)^2 + zrows*m*mean^2,  invstd = 1/sqrt(M2/N + eps),  running var <- M2/(N-1)
// bn1d_fwd_body's structure (lane = channel, kBnGroups row groups, two passes in double, bn_group_sum's fixed order, no
// atomics) as a body of its own, so the plain kernels compile as before.  y has m + 1 rows: row m is what every
// all-zero row normalises to.  reps = 1, zrows = 0 forms bn1d_fwd_body's values bit for bit (1.0*S, Q + 0.0): the
// compiler contracts nothing here, and the fmaf calls below are the contractions it makes in bn1d_fwd_body (the running
// variance's blend and y's scale-and-shift; the running mean's blend is two products and an add there).
TSPM_DEV void bn1d_fwd_rep_body(int m, const Bn1dFwd& p, int reps, int zrows, int bid, double* red) {
#pragma clang fp contract(off)
  const int c = p.c;
  const float* __restrict__ x = p.x;
  const float momentum = p.momentum, eps = p.eps;
  float* __restrict__ rmean = p.rmean;
  float* __restrict__ rvar = p.rvar;
  const int ch = bid * kBnCh + threadIdx.x % kBnCh, grp = threadIdx.x / kBnCh;
  const bool ok = ch < c;
  const double nrep = (double)m * (double)(reps + zrows);
  double s = 0.0;
  if (ok)
#pragma unroll 4
    for (int r = grp; r < m; r += kBnGroups) s += (double)x[(long long)r * c + ch];
  const double meand = (double)reps * bn_group_sum(s, red) / nrep;
  double q = 0.0;
  if (ok)
#pragma unroll 4
    for (int r = grp; r < m; r += kBnGroups) {
      const double d = (double)x[(long long)r * c + ch] - meand;
      q = fma(d, d, q);
    }
  const double m2 = (double)reps * bn_group_sum(q, red) + (double)zrows * (double)m * (meand * meand);
  const float mean = (float)meand;
  const float invstd = (float)(1.0 / sqrt(m2 / nrep + (double)eps));
  if (!ok) return;
  const float ga = p.gamma[ch], be = p.beta[ch];
  if (grp == 0) {
    p.smean[ch] = mean;
    p.sinvstd[ch] = invstd;
    if (rmean) rmean[ch] = (1.f - momentum) * rmean[ch] + momentum * mean;
    if (rvar) rvar[ch] = fmaf(1.f - momentum, rvar[ch], momentum * (float)(m2 / (nrep - 1.0)));
    p.y[(long long)m * c + ch] = fmaf(ga, (0.f - mean) * invstd, be);
  }
  for (int r = grp; r < m; r += kBnGroups) {
    const long long i = (long long)r * c + ch;
    p.y[i] = fmaf(ga, (x[i] - mean) * invstd, be);
  }
}

__global__ __launch_bounds__(kBnCh * kBnGroups) void k_bn1d_fwd_rep(int m, Bn1dFwd p, int reps, int zrows) {
  __shared__ double red[kBnCh * kBnGroups];
  bn1d_fwd_rep_body(m, p, reps, zrows, blockIdx.x, red);
}

// Two such layers over the same m rows in one launch (k_bn1d_fwd2's split): blocks [0, nb0) take p0.
__global__ __launch_bounds__(kBnCh * kBnGroups) void k_bn1d_fwd_rep2(int m, Bn1dFwd p0, int reps0, int zrows0,
                                                                     Bn1dFwd p1, int reps1, int zrows1, int nb0) {
  __shared__ double red[kBnCh * kBnGroups];
  if ((int)blockIdx.x < nb0)
    bn1d_fwd_rep_body(m, p0, reps0, zrows0, blockIdx.x, red);
  else
    bn1d_fwd_rep_body(m, p1, reps1, zrows1, blockIdx.x - nb0, red);
}

struct Bn1dBwd {
  int c;
  const float* g;
  const float* x;
  const float* mean;
  const float* invstd;
  const float* gamma;
  float* dgamma;
  float* dbeta;
  float* dx;
  const uint8_t* g_keep;  // tspm_bn1d_bwd_drop_relu: g is the gradient of Dropout(BN(x)) -> g*keep*g_scale,
  float g_scale;          // and x is a ReLU output: dx = 0 where x <= 0
  int relu_x;
};

// DR: the Dropout-gradient-in / ReLU-mask-out variant (tspm_bn1d_bwd_drop_relu), compiled separately.
template <bool DR = false>
TSPM_DEV void bn1d_bwd_body(int m, const Bn1dBwd& p, int bid, double* red);

template <bool DR>
__global__ __launch_bounds__(kBnCh * kBnGroups) void k_bn1d_bwd(int m, Bn1dBwd p) {
  __shared__ double red[kBnCh * kBnGroups];
  bn1d_bwd_body<DR>(m, p, blockIdx.x, red);
}

__global__ __launch_bounds__(kBnCh * kBnGroups) void k_bn1d_bwd2(int m, Bn1dBwd p0, Bn1dBwd p1, int nb0) {
  __shared__ double red[kBnCh * kBnGroups];
  if ((int)blockIdx.x < nb0)
    bn1d_bwd_body(m, p0, blockIdx.x, red);
  else
    bn1d_bwd_body(m, p1, blockIdx.x - nb0, red);
}

template <bool DR>
TSPM_DEV void bn1d_bwd_body(int m, const Bn1dBwd& p, int bid, double* red) {
  const int c = p.c;
  const float* __restrict__ g = p.g;
  const float* __restrict__ x = p.x;
  const float* __restrict__ mean_ = p.mean;
  const float* __restrict__ invstd_ = p.invstd;
  const float* __restrict__ gamma = p.gamma;
  float* __restrict__ dgamma = p.dgamma;
  float* __restrict__ dbeta = p.dbeta;
  float* __restrict__ dx = p.dx;
  const int ch = bid * kBnCh + threadIdx.x % kBnCh, grp = threadIdx.x / kBnCh;
  const bool ok = ch < c;
  const float mean = ok ? mean_[ch] : 0.f, invstd = ok ? invstd_[ch] : 0.f;
  const uint8_t* __restrict__ gk = p.g_keep;
  const float gs = p.g_scale;
  auto gval = [&](long long i) -> float { return (DR && gk) ? g[i] * (gk[i] ? gs : 0.f) : g[i]; };
  double sg = 0.0, sgx = 0.0;
  if (ok)
#pragma unroll 4
    for (int r = grp; r < m; r += kBnGroups) {
      const long long i = (long long)r * c + ch;
      const double gv = (double)gval(i);
      sg += gv;
      sgx = fma(gv, ((double)x[i] - (double)mean) * (double)invstd, sgx);
    }
  const double tg = bn_group_sum(sg, red);
  const double tgx = bn_group_sum(sgx, red);
  if (!ok) return;
  if (grp == 0) {
    dgamma[ch] = (float)tgx;
    dbeta[ch] = (float)tg;
  }
  if (!dx) return;
  const double k = (double)gamma[ch] * (double)invstd, mg = tg / (double)m, mgx = tgx / (double)m;
  for (int r = grp; r < m; r += kBnGroups) {
    const long long i = (long long)r * c + ch;
    float v = (float)(k * ((double)gval(i) - mg - ((double)x[i] - (double)mean) * (double)invstd * mgx));
    if (DR && p.relu_x && !(x[i] > 0.f)) v = 0.f;
    dx[i] = v;
  }
}

int ew_grid(long long work) {
  long long b = cdiv64(work, 256);
  if (b > 4096) b = 4096;
  return (int)(b < 1 ? 1 : b);
}

// ------------------------------------------------------------------------------------------------
// MultimodalPooling (models/pooling.py:6-127): u = [proj_a(x_a) | proj_b(x_b)] [n, 2d] (+ bias, from
// the small GEMM), a | b = dropout(tanh(u)) (one Dropout module, two draws: keep [n, 2d]), then
// kind 0 max / 1 avg / 2 sum / 3 attention / 4 gated.  Attention and gated run their scoring MLP's
// first Linear (+ bias) on the small GEMM into hpre [n, hd]; tanh, the second Linear (hd -> 2 / 1 +
// bias), softmax / sigmoid and the mix run here, one workgroup per row, fixed-order block sums.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pool_act_fwd(long long total, int d2, const float* __restrict__ u, int ldu,
                                                      const uint8_t* __restrict__ keep, float scale,
                                                      float* __restrict__ tu, float* __restrict__ ab) {
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const long long r = e / d2;
    const int j = (int)(e - r * d2);
    const float t = tanhf(u[r * ldu + j]);
    tu[e] = t;
    ab[e] = keep ? t * (keep[e] ? scale : 0.f) : t;
  }
}

__global__ __launch_bounds__(kRowThreads) void k_pool_mix_fwd(int d, int hd, int kind, const float* __restrict__ ab,
                                                              const float* __restrict__ hpre, float* __restrict__ hh,
                                                              const float* __restrict__ w2, const float* __restrict__ b2,
                                                              float* __restrict__ wts, float* __restrict__ z, int ldz) {
  __shared__ float red[kRowThreads / 64];
  const long long r = blockIdx.x;
  const float* a = ab + r * 2 * d;
  const float* b = a + d;
  float* zr = z + r * ldz;
  if (kind <= 2) {
    for (int j = threadIdx.x; j < d; j += kRowThreads) {
      const float x = a[j], y = b[j];
      zr[j] = kind == 0 ? ((x > y || x != x) ? x : y) : (kind == 1 ? (x + y) / 2.f : x + y);
    }
    return;
  }
  const float* hp = hpre + r * hd;
  float* hr = hh + r * hd;
  float s0 = 0.f, s1 = 0.f;
  for (int j = threadIdx.x; j < hd; j += kRowThreads) {
    const float t = tanhf(hp[j]);
    hr[j] = t;
    s0 = fmaf(w2[j], t, s0);
    if (kind == 3) s1 = fmaf(w2[hd + j], t, s1);
  }
  s0 = block_sum(s0, red) + b2[0];
  float wa, wb;
  if (kind == 3) {
    s1 = block_sum(s1, red) + b2[1];
    const float m = fmaxf(s0, s1);
    const float e0 = expf(s0 - m), e1 = expf(s1 - m);
    const float inv = 1.f / (e0 + e1);
    wa = e0 * inv;
    wb = e1 * inv;
  } else {
    wa = 1.f / (1.f + expf(-s0));
    wb = 1.f - wa;
  }
  if (threadIdx.x == 0) {
    wts[2 * r] = wa;
    wts[2 * r + 1] = wb;
  }
  for (int j = threadIdx.x; j < d; j += kRowThreads) zr[j] = wa * a[j] + wb * b[j];
}

// dz -> dab [n, 2d] through the mix; attention / gated also: ds [n, k] (scores' gradient, for the
// second Linear's weight gradient ds^T @ hh) and dhpre [n, hd] (through that Linear and the tanh).
__global__ __launch_bounds__(kRowThreads) void k_pool_mix_bwd(int d, int hd, int kind, const float* __restrict__ dz,
                                                              int lddz, const float* __restrict__ ab,
                                                              const float* __restrict__ hh, const float* __restrict__ w2,
                                                              const float* __restrict__ wts, float* __restrict__ dab,
                                                              float* __restrict__ ds, float* __restrict__ dhpre) {
  __shared__ float red[kRowThreads / 64];
  const long long r = blockIdx.x;
  const float* a = ab + r * 2 * d;
  const float* b = a + d;
  const float* g = dz + r * lddz;
  float* da = dab + r * 2 * d;
  float* db = da + d;
  if (kind <= 2) {
    for (int j = threadIdx.x; j < d; j += kRowThreads) {
      const float gv = g[j];
      if (kind == 0) {  // torch.maximum's derivative: ties split the gradient in half
        const float x = a[j], y = b[j];
        const float h = gv / 2.f;
        da[j] = x == y ? h : (x > y ? gv : 0.f);
        db[j] = x == y ? h : (y > x ? gv : 0.f);
      } else {
        const float v = kind == 1 ? gv / 2.f : gv;
        da[j] = v;
        db[j] = v;
      }
    }
    return;
  }
  const float wa = wts[2 * r], wb = wts[2 * r + 1];
  float pa = 0.f, pb = 0.f;
  for (int j = threadIdx.x; j < d; j += kRowThreads) {
    const float gv = g[j];
    pa = fmaf(gv, a[j], pa);
    pb = fmaf(gv, b[j], pb);
    da[j] = wa * gv;
    db[j] = wb * gv;
  }
  pa = block_sum(pa, red);
  pb = block_sum(pb, red);
  float d0, d1 = 0.f;
  if (kind == 3) {  // softmax backward over the two scores
    const float dot = wa * pa + wb * pb;
    d0 = wa * (pa - dot);
    d1 = wb * (pb - dot);
  } else {          // z = g a + (1 - g) b: dg = sum dz (a - b); sigmoid backward
    d0 = (pa - pb) * wa * (1.f - wa);
  }
  if (threadIdx.x == 0) {
    ds[r * (kind == 3 ? 2 : 1)] = d0;
    if (kind == 3) ds[r * 2 + 1] = d1;
  }
  const float* hr = hh + r * hd;
  float* dh = dhpre + r * hd;
  for (int j = threadIdx.x; j < hd; j += kRowThreads) {
    float v = d0 * w2[j];
    if (kind == 3) v = fmaf(d1, w2[hd + j], v);
    const float t = hr[j];
    dh[j] = v * (1.f - t * t);
  }
}

// du = (dab [+ dab2]) * keep * scale * (1 - tanh(u)^2)
__global__ __launch_bounds__(256) void k_pool_act_bwd(long long total, const float* __restrict__ dab,
                                                      const float* __restrict__ dab2, const float* __restrict__ tu,
                                                      const uint8_t* __restrict__ keep, float scale,
                                                      float* __restrict__ du) {
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    float v = dab[e];
    if (dab2) v += dab2[e];
    if (keep) v = v * (keep[e] ? scale : 0.f);
    const float t = tu[e];
    du[e] = v * (1.f - t * t);
  }
}

// ------------------------------------------------------------------------------------------------
// Multi-label monomodal head (added under ABI 23): classifier Linear forward, weighted BCEWithLogits, predictions, F1 counts
// and the Linear's whole backward in ONE launch.  At hid 512 x 23 classes the three products are too much for one
// workgroup (≈ 1.5 M multiply-adds each at n = 128, 64 per clock and CU), so the ROWS are spread: workgroup g takes
// rows [g*rpw, (g+1)*rpw) (at most HB_MAXG workgroups) in chunks of HB_CH rows staged in LDS next to the whole weight, computes their logits,
// loss terms, predictions, dlogits and demb, and keeps its partial dw in registers across its chunks.  Each
// workgroup publishes its partial dw / db / loss / counts in its own workspace record (write-through stores) and the
// last arriver (common.h last_arriver: agent-scope acquire, counter re-armed) adds the records in workgroup order —
// no float atomics, every sum in a fixed order, the same grid in forward-only mode.
// ------------------------------------------------------------------------------------------------
constexpr int HB_THREADS = 256, HB_CH = 16, HB_MAXH = 512, HB_MAXC = 32, HB_MAXN = 1024, HB_MAXG = 16;
constexpr int HB_LDZ = HB_MAXC + 1;          // LDS row stride of the chunk's logits / dlogits
constexpr int HB_SL = HB_THREADS / (HB_CH / 2);  // logits: threads that share two rows (half a wave)
constexpr int HB_QPT = HB_MAXH / 4 / HB_SL;  // logits: column quads per thread
static_assert(HB_SL <= 64 && (HB_SL & (HB_SL - 1)) == 0, "the logits' lane reduction is an xor butterfly in a wave");
// rows per workgroup come in steps of HB_RG: 8 rows each up to n = 128 (16 workgroups; a half-filled chunk), which
// measured 3 us per step faster at n = 128 than 16 rows in 8 workgroups, and one full 16-row chunk each at n = 256
// (6 us faster than two 8-row chunks) — scripts/bench_mmimdb_mono.py
constexpr int HB_RG = 8;
constexpr int HB_CU = 4;                     // logits: classes whose lane reductions run together
constexpr int HB_CPT = 16;                   // dw: classes per thread (hid/4 = 128 columns x 2 class groups)
constexpr int HB_HDR = 16;                   // workspace floats ahead of the records (the arrival counter)

struct HbPlan {
  int rpw, groups, rec;  // rows per workgroup, workgroups, floats per workspace record
};
inline HbPlan hb_plan(int n, int hid, int classes) {
  HbPlan p;
  p.rpw = HB_RG * cdiv(n, HB_RG * HB_MAXG);
  p.groups = cdiv(n, p.rpw);
  // record: loss sum, F1 sum (two doubles) | db[classes] | tp, fp, fn [classes][3] | dw[classes][hid]
  p.rec = (4 + 4 * classes + classes * hid + 3) & ~3;
  return p;
}

TSPM_DEV void st_sc1_f64(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
TSPM_DEV double ld_sc1_f64(const double* p) {
  return __hip_atomic_load((__attribute__((address_space(1))) double*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Sum of v over the workgroup's HB_THREADS threads in a fixed order (xor butterfly per wave, waves in index order).
TSPM_DEV double hb_block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int w = 1; w < HB_THREADS / 64; ++w) s += red[w];
  return s;
}

__global__ __launch_bounds__(HB_THREADS) void k_mono_head_bce(tspm_mono_head_bce_desc d, int rpw, int rec) {
  extern __shared__ float lds[];
  const int t = threadIdx.x, N = d.n, H = d.hid, K = d.classes, H4 = H >> 2, LDE = H + 4;
  float* w_s = lds;                                  // [K][LDE]
  float* emb_s = w_s + K * LDE;                      // [HB_CH][LDE]
  float* z_s = emb_s + HB_CH * LDE;                  // [HB_CH][HB_LDZ] logits, then dlogits
  float* b_s = z_s + HB_CH * HB_LDZ;                 // [HB_MAXC]
  double* red = reinterpret_cast<double*>(b_s + HB_MAXC);  // [4] (8-byte aligned: every size above is even)
  int* flag = reinterpret_cast<int*>(red + 4);
  uint8_t* p_s = reinterpret_cast<uint8_t*>(flag + 4);     // [HB_CH][HB_MAXC] predictions
  uint8_t* y_s = p_s + HB_CH * HB_MAXC;                    // [HB_CH][HB_MAXC] targets > 0.5
  const bool train = d.dw != nullptr;
  if ((reinterpret_cast<uintptr_t>(d.w) & 15) == 0) {  // uniform; a parameter view need not be 16-byte aligned
    for (int e = t; e < K * H4; e += HB_THREADS) st4(w_s + (e / H4) * LDE + (e % H4) * 4, ld4(d.w + 4 * e));
  } else {
    for (int e = t; e < K * H; e += HB_THREADS) w_s[(e / H) * LDE + e % H] = d.w[e];
  }
  if (t < K) b_s[t] = d.b[t];
  // dw: thread (cg, q) owns column quad q of classes cg, cg + CG, ... (HB_CPT of them at most: CG >= 2)
  const int CG = HB_THREADS / H4, dq = t % H4, dcg = t / H4;
  const bool dw_thread = dcg < CG;
  f32x4 acc[HB_CPT];
#pragma unroll
  for (int u = 0; u < HB_CPT; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  float dbacc = 0.f;              // thread c < K: db[c]
  int tp = 0, fp = 0, fn = 0;     // thread 64 + c: the counts of class c
  double lsum = 0.0, f1sum = 0.0;
  const float inv = 1.f / (float)((long long)N * K);
  const int g = blockIdx.x, r_end = min(N, (g + 1) * rpw);
  for (int r0 = g * rpw; r0 < r_end; r0 += HB_CH) {
    const int rows = min(HB_CH, r_end - r0);
    __syncthreads();  // the previous chunk's readers are done (and w_s / b_s are written)
    for (int i = t; i < HB_CH * H4; i += HB_THREADS) {
      const int r = i / H4, j = (i % H4) * 4;
      st4(emb_s + r * LDE + j,
          r < rows ? ld4(d.emb + (long long)(r0 + r) * d.ld_emb + j) : f32x4{0.f, 0.f, 0.f, 0.f});
    }
    __syncthreads();
    {  // logits: HB_SL lanes share rows 2rp and 2rp + 1, each over column quads s, s + HB_SL, ...; xor butterfly
      const int rp = t / HB_SL, s = t % HB_SL;
      f32x4 e0[HB_QPT], e1[HB_QPT];
#pragma unroll
      for (int i = 0; i < HB_QPT; ++i) {
        const int q = s + HB_SL * i;
        const bool ok = q < H4;
        e0[i] = ok ? ld4(emb_s + (2 * rp) * LDE + 4 * q) : f32x4{0.f, 0.f, 0.f, 0.f};
        e1[i] = ok ? ld4(emb_s + (2 * rp + 1) * LDE + 4 * q) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
      for (int c0 = 0; c0 < K; c0 += HB_CU) {  // HB_CU classes at a time: their butterflies overlap
        float p0[HB_CU], p1[HB_CU];
#pragma unroll
        for (int u = 0; u < HB_CU; ++u) {
          const int c = min(c0 + u, K - 1);  // a class past the last repeats it (never stored)
          float a0 = 0.f, a1 = 0.f;
#pragma unroll
          for (int i = 0; i < HB_QPT; ++i) {
            const int q = s + HB_SL * i;
            if (q < H4) {
              const f32x4 wv = ld4(w_s + c * LDE + 4 * q);
              a0 += e0[i][0] * wv[0]; a0 += e0[i][1] * wv[1]; a0 += e0[i][2] * wv[2]; a0 += e0[i][3] * wv[3];
              a1 += e1[i][0] * wv[0]; a1 += e1[i][1] * wv[1]; a1 += e1[i][2] * wv[2]; a1 += e1[i][3] * wv[3];
            }
          }
          p0[u] = a0;
          p1[u] = a1;
        }
#pragma unroll
        for (int o = HB_SL / 2; o > 0; o >>= 1) {
#pragma unroll
          for (int u = 0; u < HB_CU; ++u) {
            p0[u] += __shfl_xor(p0[u], o, 64);
            p1[u] += __shfl_xor(p1[u], o, 64);
          }
        }
#pragma unroll
        for (int u = 0; u < HB_CU; ++u) {
          const int c = c0 + u;
          if (s == c && c < K) {  // K <= 32
            z_s[(2 * rp) * HB_LDZ + c] = p0[u] + b_s[c];
            z_s[(2 * rp + 1) * HB_LDZ + c] = p1[u] + b_s[c];
          }
        }
      }
    }
    __syncthreads();
    // BCEWithLogits per element (k_bce_logits' arithmetic); dlogits overwrite the logits in LDS
    for (int p = t; p < rows * K; p += HB_THREADS) {
      const int r = p / K, c = p % K;
      const long long gi = (long long)(r0 + r) * K + c;
      const float xv = z_s[r * HB_LDZ + c], tv = d.targets[gi];
      d.logits[gi] = xv;
      const float ls = fminf(xv, 0.f) - log1pf(expf(-fabsf(xv)));
      lsum += (double)((1.f - tv) * xv - ls);
      const float sg = 1.f / (1.f + expf(-xv));
      const bool pr = sg > d.threshold;
      if (d.preds) d.preds[gi] = pr ? 1 : 0;
      p_s[r * HB_MAXC + c] = pr ? 1 : 0;
      y_s[r * HB_MAXC + c] = tv > 0.5f ? 1 : 0;
      z_s[r * HB_LDZ + c] = (sg - tv) * inv * d.loss_weight;
    }
    __syncthreads();
    if (d.stats) {
      if (t < rows) {  // per-sample F1 (zero_division = 0)
        int a = 0, b = 0, c2 = 0;
        for (int k = 0; k < K; ++k) {
          const int p = p_s[t * HB_MAXC + k], y = y_s[t * HB_MAXC + k];
          a += p & y;
          b += p & (y ^ 1);
          c2 += (p ^ 1) & y;
        }
        const int den = 2 * a + b + c2;
        f1sum += den > 0 ? (double)((2.f * a) / (float)den) : 0.0;
      } else if (t >= 64 && t < 64 + K) {  // per-class counts
        const int k = t - 64;
        for (int r = 0; r < rows; ++r) {
          const int p = p_s[r * HB_MAXC + k], y = y_s[r * HB_MAXC + k];
          tp += p & y;
          fp += p & (y ^ 1);
          fn += (p ^ 1) & y;
        }
      }
    }
    if (!train) continue;  // uniform: forward only
    // demb = dlogits @ w for the chunk's rows
    for (int i = t; i < rows * H4; i += HB_THREADS) {
      const int r = i / H4, j = (i % H4) * 4;
      f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int c = 0; c < K; ++c) s4 += z_s[r * HB_LDZ + c] * ld4(w_s + c * LDE + j);
      st4(d.demb + (long long)(r0 + r) * d.ld_demb + j, s4);
    }
    // dw[c][4q..] += sum_r dlogits[r][c] emb[r][4q..] (rows in order), db[c] += sum_r dlogits[r][c]
    if (dw_thread)
      for (int r = 0; r < rows; ++r) {
        const f32x4 ev = ld4(emb_s + r * LDE + 4 * dq);
#pragma unroll
        for (int u = 0; u < HB_CPT; ++u) {
          const int c = dcg + u * CG;
          if (c < K) acc[u] += z_s[r * HB_LDZ + c] * ev;
        }
      }
    if (t < K)
      for (int r = 0; r < rows; ++r) dbacc += z_s[r * HB_LDZ + t];
  }
  // publish this workgroup's record (write-through), then the last arriver adds the records in workgroup order
  float* ws = static_cast<float*>(d.workspace);
  float* my = ws + HB_HDR + (long long)g * rec;
  const double lwg = hb_block_sum(lsum, red);
  const double fwg = hb_block_sum(f1sum, red);
  if (t == 0) {
    st_sc1_f64(reinterpret_cast<double*>(my), lwg);
    st_sc1_f64(reinterpret_cast<double*>(my) + 1, fwg);
  }
  if (t < K) st_sc1(my + 4 + t, dbacc);
  if (t >= 64 && t < 64 + K) {
    float* cnt = my + 4 + K + 3 * (t - 64);
    st_sc1(cnt, (float)tp);
    st_sc1(cnt + 1, (float)fp);
    st_sc1(cnt + 2, (float)fn);
  }
  const int dw0 = 4 + 4 * K;
  if (train && dw_thread) {
#pragma unroll
    for (int u = 0; u < HB_CPT; ++u) {
      const int c = dcg + u * CG;
      if (c < K) {
        float* p = my + dw0 + c * H + 4 * dq;
        st_sc1(p, acc[u][0]);
        st_sc1(p + 1, acc[u][1]);
        st_sc1(p + 2, acc[u][2]);
        st_sc1(p + 3, acc[u][3]);
      }
    }
  }
  const int G = gridDim.x;
  if (!last_arriver(reinterpret_cast<unsigned*>(ws), (unsigned)G, flag)) return;
  const float* recs = ws + HB_HDR;
  if (train) {
    // behind last_arriver's agent-scope acquire: plain 16-byte loads, G of them in flight per column quad (one
    // sc1 load per element left the last workgroup waiting on K*H/256 round trips in a row)
    // two column quads per pass, so 2 G loads are in flight
    for (int e = t; e < K * H4; e += 2 * HB_THREADS) {
      const int e2 = e + HB_THREADS;
      const bool two = e2 < K * H4;
      f32x4 v[HB_MAXG], v2[HB_MAXG];
#pragma unroll
      for (int q = 0; q < HB_MAXG; ++q) {
        const float* rq = recs + (long long)q * rec + dw0;
        v[q] = q < G ? ld4(rq + 4 * e) : f32x4{0.f, 0.f, 0.f, 0.f};
        v2[q] = q < G && two ? ld4(rq + 4 * e2) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
      f32x4 s4 = v[0], s42 = v2[0];
#pragma unroll
      for (int q = 1; q < HB_MAXG; ++q)
        if (q < G) {
          s4 += v[q];
          s42 += v2[q];
        }
      float* o = d.dw + 4 * e;
      o[0] = s4[0]; o[1] = s4[1]; o[2] = s4[2]; o[3] = s4[3];
      if (two) {
        float* o2 = d.dw + 4 * e2;
        o2[0] = s42[0]; o2[1] = s42[1]; o2[2] = s42[2]; o2[3] = s42[3];
      }
    }
    if (t < K) {
      float s = 0.f;
      for (int q = 0; q < G; ++q) s += ld_sc1(recs + (long long)q * rec + 4 + t);
      d.db[t] = s;
    }
  }
  if (t == 0) {
    double l = 0.0, f = 0.0;
    for (int q = 0; q < G; ++q) {
      const double* rq = reinterpret_cast<const double*>(recs + (long long)q * rec);
      l += ld_sc1_f64(rq);
      f += ld_sc1_f64(rq + 1);
    }
    const float mean = (float)(l / ((double)N * (double)K)) * d.loss_weight;
    d.loss[0] = mean;
    if (d.stats) {
      d.stats[0] += mean * (float)N;
      d.stats[1] += (float)N;
      d.stats[2] += (float)f;
    }
  }
  if (d.stats && t >= 64 && t < 64 + K) {
    float a = 0.f, b = 0.f, c2 = 0.f;
    for (int q = 0; q < G; ++q) {
      const float* cnt = recs + (long long)q * rec + 4 + K + 3 * (t - 64);
      a += ld_sc1(cnt);
      b += ld_sc1(cnt + 1);
      c2 += ld_sc1(cnt + 2);
    }
    float* out = d.stats + 3 + 3 * (t - 64);
    out[0] += a;
    out[1] += b;
    out[2] += c2;
  }
}

}  // namespace

extern "C" size_t tspm_mono_head_bce_workspace(int32_t n, int32_t hid, int32_t classes) {
  if (n < 1 || n > HB_MAXN || hid < 4 || hid > HB_MAXH || hid % 4 || classes < 1 || classes > HB_MAXC) return 0;
  const HbPlan p = hb_plan(n, hid, classes);
  return ((size_t)HB_HDR + (size_t)p.groups * p.rec) * sizeof(float);
}

extern "C" int tspm_mono_head_bce_step(const tspm_mono_head_bce_desc* desc, tspm_stream_t stream) {
  if (!desc) return TSPM_ERR_INVALID;
  const tspm_mono_head_bce_desc& d = *desc;
  if (d.n < 1 || d.n > HB_MAXN || d.hid < 4 || d.hid > HB_MAXH || d.hid % 4 || d.classes < 1 || d.classes > HB_MAXC)
    return TSPM_ERR_INVALID;
  if (!d.emb || !d.w || !d.b || !d.targets || !d.logits || !d.loss) return TSPM_ERR_INVALID;
  const auto aligned16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  if (d.ld_emb < d.hid || d.ld_emb % 4 || !aligned16(d.emb)) return TSPM_ERR_INVALID;
  const bool train = d.dw || d.db || d.demb;
  if (train) {  // the whole backward or none of it
    if (!d.dw || !d.db || !d.demb) return TSPM_ERR_INVALID;
    if (d.ld_demb < d.hid || d.ld_demb % 4 || !aligned16(d.demb)) return TSPM_ERR_INVALID;
  }
  const HbPlan p = hb_plan(d.n, d.hid, d.classes);
  if (d.workspace && !aligned16(d.workspace)) return TSPM_ERR_INVALID;
  if (!d.workspace || d.workspace_bytes < ((size_t)HB_HDR + (size_t)p.groups * p.rec) * sizeof(float))
    return TSPM_ERR_WORKSPACE;
  const int LDE = d.hid + 4;
  const size_t lds = (size_t)(d.classes * LDE + HB_CH * LDE + HB_CH * HB_LDZ + HB_MAXC) * sizeof(float) +
                     4 * sizeof(double) + 4 * sizeof(int) + 2 * HB_CH * HB_MAXC;
  hipLaunchKernelGGL(k_mono_head_bce, dim3(p.groups), dim3(HB_THREADS), lds, static_cast<hipStream_t>(stream), d, p.rpw,
                     p.rec);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}

extern "C" int tspm_gmu_fwd(int32_t n, int32_t d, const float* u, int32_t ldu, const float* wz, float* h,
                            int32_t ldh, float* gate, float* z, int32_t ldz, tspm_stream_t stream) {
  if (n <= 0 || d <= 0 || ldu < 2 * d || ldh < 2 * d || ldz < d || !u || !wz || !h || !gate || !z)
    return TSPM_ERR_INVALID;
  hipLaunchKernelGGL(k_gmu_fwd, dim3(n), dim3(kRowThreads), 0, static_cast<hipStream_t>(stream), d, u, ldu, wz, h,
                     ldh, gate, z, ldz);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}

extern "C" int tspm_gmu_bwd(int32_t n, int32_t d, const float* dz, int32_t lddz, const float* h, int32_t ldh,
                            const float* gate, const float* wz, float* du, int32_t lddu, float* ds,
                            tspm_stream_t stream) {
  if (n <= 0 || d <= 0 || lddz < d || ldh < 2 * d || lddu < 2 * d || !dz || !h || !gate || !wz || !du || !ds)
    return TSPM_ERR_INVALID;
  hipLaunchKernelGGL(k_gmu_bwd, dim3(n), dim3(kRowThreads), 0, static_cast<hipStream_t>(stream), d, dz, lddz, h, ldh,
                     gate, wz, du, lddu, ds);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}

extern "C" int tspm_maxout_fwd(int32_t n, int32_t d, const float* a, int32_t lda, const uint8_t* keep,
                               float keep_scale, float* y, int32_t ldy, tspm_stream_t stream) {
  if (n <= 0 || d <= 0 || lda < 2 * d || ldy < d || !a || !y) return TSPM_ERR_INVALID;
  hipLaunchKernelGGL(k_maxout_fwd, dim3(ew_grid((long long)n * d)), dim3(256), 0, static_cast<hipStream_t>(stream), n,
                     d, a, lda, keep, keep_scale, y, ldy);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}

extern "C" int tspm_maxout_bwd(int32_t n, int32_t d, const float* dy, int32_t lddy, const float* a, int32_t lda,
                               const uint8_t* keep, float keep_scale, float* da, int32_t ldda, tspm_stream_t stream) {
  if (n <= 0 || d <= 0 || lddy < d || lda < 2 * d || ldda < 2 * d || !dy || !a || !da) return TSPM_ERR_INVALID;
  hipLaunchKernelGGL(k_maxout_bwd, dim3(ew_grid((long long)n * d)), dim3(256), 0, static_cast<hipStream_t>(stream), n,
                     d, dy, lddy, a, lda, keep, keep_scale, da, ldda);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}

extern "C" int tspm_bce_logits(int32_t n, int32_t classes, const float* logits, const float* targets, float* loss,
                               float* dlogits, float grad_scale, float threshold, float* stats, tspm_stream_t stream) {
  if (n <= 0 || classes <= 0 || !logits || !targets || !loss) return TSPM_ERR_INVALID;
  hipLaunchKernelGGL(k_bce_logits, dim3(1), dim3(kLossThreads), 0, static_cast<hipStream_t>(stream), n, classes, logits,
                     targets, loss, dlogits, grad_scale, threshold, stats);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}

extern "C" int tspm_bce_logits_patterns(int32_t batch, int32_t npat, int32_t classes, const float* logits,
                                        const float* targets, float grad_scale, float threshold, float* loss,
                                        float* stats, float* loss_log, int64_t* counters, int64_t log_capacity,
                                        tspm_stream_t stream) {
  if (batch <= 0 || npat < 1 || npat > TSPM_MAX_PATTERNS || classes <= 0 || !logits || !targets || !loss)
    return TSPM_ERR_INVALID;
  if (log_capacity < 0 || (loss_log && !counters)) return TSPM_ERR_INVALID;
  hipLaunchKernelGGL(k_bce_logits_patterns, dim3(npat), dim3(kLossThreads), 0, static_cast<hipStream_t>(stream), batch,
                     classes, logits, targets, loss, grad_scale, threshold, stats);
  TSPM_LAUNCH_CHECK();
  if (counters) {
    hipLaunchKernelGGL(k_pattern_loss_log, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), npat,
                       (long long)npat * batch, loss, loss_log, reinterpret_cast<long long*>(counters),
                       (long long)log_capacity);
    TSPM_LAUNCH_CHECK();
  }
  return TSPM_OK;
}

extern "C" int tspm_gmu_pattern_fwd(int32_t batch, int32_t npat, const int32_t* keep, int32_t d, const float* u,
                                    int32_t ldu, const float* u0, const float* wz, float* h, int32_t ldh, float* gate,
                                    float* z, int32_t ldz, tspm_stream_t stream) {
  if (batch <= 0 || npat < 1 || npat > TSPM_MAX_PATTERNS || d <= 0 || d > TSPM_GMU_PATTERN_MAX_D)
    return TSPM_ERR_INVALID;
  if (!keep || !u || !wz || !z || ldu < 2 * d || ldz < d || (h && ldh < 2 * d)) return TSPM_ERR_INVALID;
  GmuPatternSet ps{};
  for (int p = 0; p < npat; ++p) {
    ps.keep[p] = (keep[2 * p] ? 1 : 0) | (keep[2 * p + 1] ? 2 : 0);
    if (ps.keep[p] == 0 || (ps.keep[p] != 3 && !u0)) return TSPM_ERR_INVALID;
  }
  const size_t lds = (size_t)(4 * d + 4) * sizeof(float);
  hipLaunchKernelGGL(k_gmu_pattern_fwd, dim3(batch < kGmuPatternGrid ? batch : kGmuPatternGrid), dim3(kRowThreads), lds,
                     static_cast<hipStream_t>(stream), batch, npat, ps, d, u, ldu, u0, wz, h, ldh, gate, z, ldz);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}

extern "C" size_t tspm_gmu_pattern_bwd_workspace(int32_t batch, int32_t d) {
  if (batch <= 0 || d <= 0 || d > TSPM_GMU_PATTERN_MAX_D) return 0;
  return (size_t)(batch < kGmuPatternGrid ? batch : kGmuPatternGrid) * 2 * (size_t)d * sizeof(float);
}

extern "C" int tspm_gmu_pattern_bwd(int32_t batch, int32_t npat, const int32_t* keep, int32_t d, const float* dz,
                                    int32_t lddz, const float* h, int32_t ldh, const float* gate, const float* wz,
                                    float* du, int32_t lddu, float* ds, void* workspace, size_t workspace_bytes,
                                    tspm_stream_t stream) {
  if (batch <= 0 || npat < 1 || npat > TSPM_MAX_PATTERNS || d <= 0 || d > TSPM_GMU_PATTERN_MAX_D)
    return TSPM_ERR_INVALID;
  if (!keep || !dz || !h || !gate || !wz || !du || !ds || lddz < d || ldh < 2 * d || lddu < 2 * d)
    return TSPM_ERR_INVALID;
  GmuPatternSet ps{};
  for (int p = 0; p < npat; ++p) {
    ps.keep[p] = (keep[2 * p] ? 1 : 0) | (keep[2 * p + 1] ? 2 : 0);
    if (ps.keep[p] == 0) return TSPM_ERR_INVALID;
  }
  if (!workspace || workspace_bytes < tspm_gmu_pattern_bwd_workspace(batch, d)) return TSPM_ERR_WORKSPACE;
  const int grid = batch < kGmuPatternGrid ? batch : kGmuPatternGrid;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
#define TSPM_GMU_PBWD(TRIPS)                                                                                          \
  hipLaunchKernelGGL(k_gmu_pattern_bwd<TRIPS>, dim3(grid), dim3(kRowThreads), 0, st, batch, npat, ps, d, dz, lddz, h, \
                     ldh, gate, wz, du, lddu, ds, part)
  const int trips = cdiv(d, kRowThreads);  // 1..16 (d <= 4095)
  if (trips <= 1) TSPM_GMU_PBWD(1);
  else if (trips <= 2) TSPM_GMU_PBWD(2);
  else if (trips <= 4) TSPM_GMU_PBWD(4);
  else if (trips <= 8) TSPM_GMU_PBWD(8);
  else TSPM_GMU_PBWD(16);
#undef TSPM_GMU_PBWD
  TSPM_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_gmu_pattern_bwd_zero, dim3(cdiv(2 * d, kGmuZeroCols)), dim3(kGmuZeroCols * kGmuZeroGroups), 0,
                     st, grid, 2 * d, part, du + (long long)batch * lddu);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}

extern "C" int tspm_bn1d_fwd_rep(int32_t m, int32_t c, const float* x, const float* gamma, const float* beta,
                                 float* running_mean, float* running_var, float momentum, float eps, float* save_mean,
                                 float* save_invstd, float* y, int32_t reps, int32_t zero_rows_per_row,
                                 tspm_stream_t stream) {
  if (m <= 0 || c <= 0 || reps < 1 || zero_rows_per_row < 0 || (long long)m * (reps + (long long)zero_rows_per_row) < 2 ||
      !x || !gamma || !beta || !save_mean || !save_invstd || !y)
    return TSPM_ERR_INVALID;
  const Bn1dFwd p{c, x, gamma, beta, running_mean, running_var, momentum, eps, save_mean, save_invstd, y};
  hipLaunchKernelGGL(k_bn1d_fwd_rep, dim3(cdiv(c, kBnCh)), dim3(kBnCh * kBnGroups), 0, static_cast<hipStream_t>(stream),
                     m, p, reps, zero_rows_per_row);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}

extern "C" int tspm_bn1d_fwd_rep_pair(int32_t m, int32_t c0, const float* x0, const float* gamma0, const float* beta0,
                                      float* running_mean0, float* running_var0, float momentum0, float eps0,
                                      float* save_mean0, float* save_invstd0, float* y0, int32_t reps0,
                                      int32_t zero_rows_per_row0, int32_t c1, const float* x1, const float* gamma1,
                                      const float* beta1, float* running_mean1, float* running_var1, float momentum1,
                                      float eps1, float* save_mean1, float* save_invstd1, float* y1, int32_t reps1,
                                      int32_t zero_rows_per_row1, tspm_stream_t stream) {
  if (m <= 0 || c0 <= 0 || c1 <= 0 || reps0 < 1 || reps1 < 1 || zero_rows_per_row0 < 0 || zero_rows_per_row1 < 0 ||
      (long long)m * (reps0 + (long long)zero_rows_per_row0) < 2 ||
      (long long)m * (reps1 + (long long)zero_rows_per_row1) < 2 || !x0 || !gamma0 || !beta0 || !save_mean0 ||
      !save_invstd0 || !y0 || !x1 || !gamma1 || !beta1 || !save_mean1 || !save_invstd1 || !y1)
    return TSPM_ERR_INVALID;
  const Bn1dFwd p0{c0, x0, gamma0, beta0, running_mean0, running_var0, momentum0, eps0, save_mean0, save_invstd0, y0};
  const Bn1dFwd p1{c1, x1, gamma1, beta1, running_mean1, running_var1, momentum1, eps1, save_mean1, save_invstd1, y1};
  const int nb0 = cdiv(c0, kBnCh);
  hipLaunchKernelGGL(k_bn1d_fwd_rep2, dim3(nb0 + cdiv(c1, kBnCh)), dim3(kBnCh * kBnGroups), 0,
                     static_cast<hipStream_t>(stream), m, p0, reps0, zero_rows_per_row0, p1, reps1, zero_rows_per_row1,
                     nb0);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}

extern "C" int tspm_bn1d_fwd(int32_t m, int32_t c, const float* x, const float* gamma, const float* beta,
                             float* running_mean, float* running_var, float momentum, float eps, float* save_mean,
                             float* save_invstd, float* y, tspm_stream_t stream) {
  if (m <= 0 || c <= 0 || !x || !gamma || !beta || !save_mean || !save_invstd || !y) return TSPM_ERR_INVALID;
  const Bn1dFwd p{c, x, gamma, beta, running_mean, running_var, momentum, eps, save_mean, save_invstd, y};
  hipLaunchKernelGGL(k_bn1d_fwd<false>, dim3(cdiv(c, kBnCh)), dim3(kBnCh * kBnGroups), 0, static_cast<hipStream_t>(stream),
                     m, p);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}

extern "C" int tspm_bn1d_bwd(int32_t m, int32_t c, const float* g, const float* x, const float* mean,
                             const float* invstd, const float* gamma, float* dgamma, float* dbeta, float* dx,
                             tspm_stream_t stream) {
  if (m <= 0 || c <= 0 || !g || !x || !mean || !invstd || !gamma || !dgamma || !dbeta) return TSPM_ERR_INVALID;
  const Bn1dBwd p{c, g, x, mean, invstd, gamma, dgamma, dbeta, dx};
  hipLaunchKernelGGL(k_bn1d_bwd<false>, dim3(cdiv(c, kBnCh)), dim3(kBnCh * kBnGroups), 0, static_cast<hipStream_t>(stream),
                     m, p);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}

extern "C" int tspm_bn1d_fwd_drop(int32_t m, int32_t c, const float* x, const float* gamma, const float* beta,
                                  float* running_mean, float* running_var, float momentum, float eps, float* save_mean,
                                  float* save_invstd, const uint8_t* keep, float keep_scale, float* y,
                                  tspm_stream_t stream) {
  if (m <= 0 || c <= 0 || !x || !gamma || !beta || !save_mean || !save_invstd || !y) return TSPM_ERR_INVALID;
  const Bn1dFwd p{c, x, gamma, beta, running_mean, running_var, momentum, eps, save_mean, save_invstd, y, keep, keep_scale};
  hipLaunchKernelGGL(k_bn1d_fwd<true>, dim3(cdiv(c, kBnCh)), dim3(kBnCh * kBnGroups), 0, static_cast<hipStream_t>(stream),
                     m, p);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}

extern "C" int tspm_bn1d_bwd_drop_relu(int32_t m, int32_t c, const float* g, const uint8_t* g_keep, float g_scale,
                                       const float* x, const float* mean, const float* invstd, const float* gamma,
                                       float* dgamma, float* dbeta, float* dx, tspm_stream_t stream) {
  if (m <= 0 || c <= 0 || !g || !x || !mean || !invstd || !gamma || !dgamma || !dbeta) return TSPM_ERR_INVALID;
  const Bn1dBwd p{c, g, x, mean, invstd, gamma, dgamma, dbeta, dx, g_keep, g_scale, 1};
  hipLaunchKernelGGL(k_bn1d_bwd<true>, dim3(cdiv(c, kBnCh)), dim3(kBnCh * kBnGroups), 0, static_cast<hipStream_t>(stream),
                     m, p);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}

extern "C" int tspm_bn1d_fwd_pair(int32_t m, int32_t c0, const float* x0, const float* gamma0, const float* beta0,
                                  float* running_mean0, float* running_var0, float momentum0, float eps0,
                                  float* save_mean0, float* save_invstd0, float* y0, int32_t c1, const float* x1,
                                  const float* gamma1, const float* beta1, float* running_mean1, float* running_var1,
                                  float momentum1, float eps1, float* save_mean1, float* save_invstd1, float* y1,
                                  tspm_stream_t stream) {
  if (m <= 0 || c0 <= 0 || c1 <= 0 || !x0 || !gamma0 || !beta0 || !save_mean0 || !save_invstd0 || !y0 || !x1 ||
      !gamma1 || !beta1 || !save_mean1 || !save_invstd1 || !y1)
    return TSPM_ERR_INVALID;
  const Bn1dFwd p0{c0, x0, gamma0, beta0, running_mean0, running_var0, momentum0, eps0, save_mean0, save_invstd0, y0};
  const Bn1dFwd p1{c1, x1, gamma1, beta1, running_mean1, running_var1, momentum1, eps1, save_mean1, save_invstd1, y1};
  const int nb0 = cdiv(c0, kBnCh);
  hipLaunchKernelGGL(k_bn1d_fwd2, dim3(nb0 + cdiv(c1, kBnCh)), dim3(kBnCh * kBnGroups), 0,
                     static_cast<hipStream_t>(stream), m, p0, p1, nb0);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}

extern "C" int tspm_bn1d_bwd_pair(int32_t m, int32_t c0, const float* g0, const float* x0, const float* mean0,
                                  const float* invstd0, const float* gamma0, float* dgamma0, float* dbeta0, float* dx0,
                                  int32_t c1, const float* g1, const float* x1, const float* mean1,
                                  const float* invstd1, const float* gamma1, float* dgamma1, float* dbeta1, float* dx1,
                                  tspm_stream_t stream) {
  if (m <= 0 || c0 <= 0 || c1 <= 0 || !g0 || !x0 || !mean0 || !invstd0 || !gamma0 || !dgamma0 || !dbeta0 || !g1 ||
      !x1 || !mean1 || !invstd1 || !gamma1 || !dgamma1 || !dbeta1)
    return TSPM_ERR_INVALID;
  const Bn1dBwd p0{c0, g0, x0, mean0, invstd0, gamma0, dgamma0, dbeta0, dx0};
  const Bn1dBwd p1{c1, g1, x1, mean1, invstd1, gamma1, dgamma1, dbeta1, dx1};
  const int nb0 = cdiv(c0, kBnCh);
  hipLaunchKernelGGL(k_bn1d_bwd2, dim3(nb0 + cdiv(c1, kBnCh)), dim3(kBnCh * kBnGroups), 0,
                     static_cast<hipStream_t>(stream), m, p0, p1, nb0);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}

extern "C" int tspm_maxout_fwd_rng(int32_t n, int32_t d, const float* a, int32_t lda, float p, uint64_t seed,
                                   const uint64_t* counter, int64_t index_offset, uint8_t* keep, float keep_scale,
                                   float* y, int32_t ldy, tspm_stream_t stream) {
  if (n <= 0 || d <= 0 || lda < 2 * d || ldy < d || !a || !keep || !y || p < 0.f || p >= 1.f || index_offset < 0)
    return TSPM_ERR_INVALID;
  hipLaunchKernelGGL(k_maxout_fwd_rng, dim3(ew_grid((long long)n * d)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     n, d, a, lda, p, (unsigned long long)seed, counter, (long long)index_offset, keep, keep_scale, y,
                     ldy);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}

extern "C" int tspm_pool_act_fwd(int32_t n, int32_t d, const float* u, int32_t ldu, const uint8_t* keep, float keep_scale,
                                 float* tu, float* ab, tspm_stream_t stream) {
  if (n <= 0 || d <= 0 || ldu < 2 * d || !u || !tu || !ab) return TSPM_ERR_INVALID;
  const long long total = (long long)n * 2 * d;
  hipLaunchKernelGGL(k_pool_act_fwd, dim3(ew_grid(total)), dim3(256), 0, static_cast<hipStream_t>(stream), total, 2 * d,
                     u, ldu, keep, keep_scale, tu, ab);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}

extern "C" int tspm_pool_mix_fwd(int32_t n, int32_t d, int32_t hd, int32_t kind, const float* ab, const float* hpre,
                                 float* hh, const float* w2, const float* b2, float* wts, float* z, int32_t ldz,
                                 tspm_stream_t stream) {
  if (n <= 0 || d <= 0 || kind < 0 || kind > 4 || ldz < d || !ab || !z) return TSPM_ERR_INVALID;
  if (kind >= 3 && (hd <= 0 || !hpre || !hh || !w2 || !b2 || !wts)) return TSPM_ERR_INVALID;
  hipLaunchKernelGGL(k_pool_mix_fwd, dim3(n), dim3(kRowThreads), 0, static_cast<hipStream_t>(stream), d, hd, kind, ab,
                     hpre, hh, w2, b2, wts, z, ldz);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}

extern "C" int tspm_pool_mix_bwd(int32_t n, int32_t d, int32_t hd, int32_t kind, const float* dz, int32_t lddz,
                                 const float* ab, const float* hh, const float* w2, const float* wts, float* dab,
                                 float* ds, float* dhpre, tspm_stream_t stream) {
  if (n <= 0 || d <= 0 || kind < 0 || kind > 4 || lddz < d || !dz || !ab || !dab) return TSPM_ERR_INVALID;
  if (kind >= 3 && (hd <= 0 || !hh || !w2 || !wts || !ds || !dhpre)) return TSPM_ERR_INVALID;
  hipLaunchKernelGGL(k_pool_mix_bwd, dim3(n), dim3(kRowThreads), 0, static_cast<hipStream_t>(stream), d, hd, kind, dz,
                     lddz, ab, hh, w2, wts, dab, ds, dhpre);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}

extern "C" int tspm_pool_act_bwd(int32_t n, int32_t d, const float* dab, const float* dab2, const float* tu,
                                 const uint8_t* keep, float keep_scale, float* du, tspm_stream_t stream) {
  if (n <= 0 || d <= 0 || !dab || !tu || !du) return TSPM_ERR_INVALID;
  const long long total = (long long)n * 2 * d;
  hipLaunchKernelGGL(k_pool_act_bwd, dim3(ew_grid(total)), dim3(256), 0, static_cast<hipStream_t>(stream), total, dab,
                     dab2, tu, keep, keep_scale, du);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}
