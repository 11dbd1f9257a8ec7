// Attention pooling over the LSTM outputs — LSTMEncoder(embd_method="attention"), the Hierarchical-Attention embedding
// of models/msa/networks/lstm.py:21-44 (tspm_attn_pool_fwd / tspm_attn_pool_bwd, include/tspm.h).  Row b of a padded
// batch pools over its own L_b = min(max(lengths[b], 1), T) steps:
//   p_t = W r_t + c (a GEMM over the T*B rows, before this kernel)   z_t = tanh(p_t)   s_t = z_t . u
//   "time": alpha_t = softmax over t < L_b of s_t        "unit": alpha_t = 1        e = sum_{t < L_b} alpha_t r_t
// Layout: time-major, row (t, b) of [T][B][H]; alpha is [T][B].
//
// One workgroup of 256 threads per batch row.  Every reduction runs in an order fixed by L_b and H alone — waves stride
// over t, a wave's dot product is the xor butterfly, partial sums meet in LDS in index order — so a row's results do not
// depend on the padding, the batch size or its neighbours, and there is no floating-point atomic anywhere.
#include "common.h"

namespace {

constexpr int kAttnThreads = 256;
constexpr int kAttnWaves = kAttnThreads / 64;
constexpr int kAttnSlices = kAttnThreads / 32;  // time slices of the weighted sum: 32 lanes x float4 cover H <= 128

struct AttnFwdDesc {
  int B, T, H, ldo, norm;
  const float* r;      // [T][B][H]
  float* p;            // [T][B][H] in: W r + c, out: tanh ("time")
  const float* u;      // [H]
  float* alpha;        // [T][B]
  float* hout;         // [B] rows of stride ldo
  const int32_t* lens;
};

// max / sum over the workgroup's 256 values in a fixed tree; every thread gets the result
template <bool Max>
TSPM_DEV float attn_block_reduce(float v, float* red) {
  const int tid = threadIdx.x;
  __syncthreads();  // red may still be read from the previous reduction
  red[tid] = v;
  __syncthreads();
  for (int o = kAttnThreads / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] = Max ? fmaxf(red[tid], red[tid + o]) : red[tid] + red[tid + o];
    __syncthreads();
  }
  return red[0];
}

TSPM_DEV void attn_fwd_body(const AttnFwdDesc& d, int b) {
  __shared__ float red[kAttnThreads];
  __shared__ f32x4 acc_sh[kAttnSlices][32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int B = d.B, T = d.T, H = d.H;
  const int L = min(max(d.lens[b], 1), T);
  if (d.norm == 0) {
    // scores: wave w takes t = w, w + 4, ...; lane l the units l and l + 64
    const float u0 = lane < H ? d.u[lane] : 0.f, u1 = lane + 64 < H ? d.u[lane + 64] : 0.f;
    for (int t = wave; t < L; t += kAttnWaves) {
      float* pr = d.p + ((long long)t * B + b) * H;
      float s = 0.f;
      if (lane < H) {
        const float z = tanhf(pr[lane]);
        pr[lane] = z;
        s = z * u0;
      }
      if (lane + 64 < H) {
        const float z = tanhf(pr[lane + 64]);
        pr[lane + 64] = z;
        s = fmaf(z, u1, s);
      }
      s = wave_sum(s);
      if (lane == 0) d.alpha[(long long)t * B + b] = s;  // the score waits in alpha's slot
    }
    __syncthreads();  // the scores, written by other waves of this workgroup, are visible
    float m = -INFINITY;
    for (int t = tid; t < L; t += kAttnThreads) m = fmaxf(m, d.alpha[(long long)t * B + b]);
    m = attn_block_reduce<true>(m, red);
    float sum = 0.f;
    for (int t = tid; t < L; t += kAttnThreads) {
      const float e = expf(d.alpha[(long long)t * B + b] - m);
      d.alpha[(long long)t * B + b] = e;  // this thread reads it back below
      sum += e;
    }
    sum = attn_block_reduce<false>(sum, red);
    for (int t = tid; t < L; t += kAttnThreads) d.alpha[(long long)t * B + b] = d.alpha[(long long)t * B + b] / sum;
  } else {
    for (int t = tid; t < L; t += kAttnThreads) d.alpha[(long long)t * B + b] = 1.f;
  }
  for (int t = L + tid; t < T; t += kAttnThreads) d.alpha[(long long)t * B + b] = 0.f;
  __syncthreads();
  // e = sum_t alpha_t r_t: slice s takes t = s, s + 8, ... in ascending order, lane q the units 4q .. 4q + 3
  const int slice = tid >> 5, q = tid & 31;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (4 * q < H) {
    for (int t = slice; t < L; t += kAttnSlices) {
      const float a = d.alpha[(long long)t * B + b];
      const f32x4 v = ld4(d.r + ((long long)t * B + b) * H + 4 * q);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = fmaf(a, v[i], acc[i]);
    }
  }
  acc_sh[slice][q] = acc;
  __syncthreads();
  if (slice == 0 && 4 * q < H) {
    f32x4 e = acc_sh[0][q];
#pragma unroll
    for (int s = 1; s < kAttnSlices; ++s) {
      const f32x4 v = acc_sh[s][q];
#pragma unroll
      for (int i = 0; i < 4; ++i) e[i] += v[i];
    }
    float* o = d.hout + (long long)b * d.ldo + 4 * q;  // ld_out need not keep the rows 16-byte aligned
    o[0] = e[0]; o[1] = e[1]; o[2] = e[2]; o[3] = e[3];
  }
}

// Workgroups [0, nb0) run problem 0's rows, the rest problem 1's (a count-1 launch passes its problem twice).
__global__ __launch_bounds__(kAttnThreads) void k_attn_pool_fwd(AttnFwdDesc d0, AttnFwdDesc d1, int nb0) {
  if ((int)blockIdx.x < nb0)
    attn_fwd_body(d0, blockIdx.x);
  else
    attn_fwd_body(d1, blockIdx.x - nb0);
}

// ------------------------------------------------------------------------------------------------
// Backward ("time"): a_t = g . r_t, D = sum_t alpha_t a_t, ds_t = alpha_t (a_t - D), dp_t = ds_t u (1 - z_t^2) (zeros
// past the length: the GEMMs that follow read all T*B rows), du = sum_{b,t} ds_t z_t — per wave in registers over its
// steps, the four waves added in order into du_rows[b], the rows added in order by k_attn_du.  Two passes over r: D
// first, from the very a_t the second pass forms again (the same instructions on the same data: the same bits), so
// sum_t ds_t cancels as it does in the softmax's own backward (D taken from the forward's output g . e instead is
// rounded differently from the a_t and leaves a residue of 1e-7 |a| in every ds_t).
// dc = sum_{b,t} dp_t is NOT left to the GEMM that forms dW: sum_t ds_t = 0 for every row, so dc_h = u_h sum ds_t
// (1 - z_th^2) is a sum whose leading part cancels — with |z| ~ 0.1 what is left is 1e-2 of the terms, and float32
// summation of the terms (the GEMM's column sums; torch's own backward too) lost 1e-5 .. 1e-4 of the result on the MOSI
// shapes.  The kernel forms what is left directly, dc_h = -u_h sum_{b,t} ds_t z_th^2, beside du.
// ------------------------------------------------------------------------------------------------
struct AttnBwdDesc {
  int B, T, H, ldg;
  const float* g;      // [B] rows of stride ldg
  const float* alpha;  // [T][B]
  const float* z;      // [T][B][H]
  const float* r;      // [T][B][H]
  const float* u;      // [H]
  float* dp;           // [T][B][H]
  float* du;           // [H]
  float* dc;           // [H]
  float* rows;         // [B][2H] scratch: each row's du, then its dc
  const int32_t* lens;
};

TSPM_DEV void attn_bwd_body(const AttnBwdDesc& d, int b) {
  __shared__ float dus[kAttnWaves][128];
  __shared__ float dcs[kAttnWaves][128];
  __shared__ float dsh[kAttnWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int B = d.B, T = d.T, H = d.H;
  const int L = min(max(d.lens[b], 1), T);
  const bool h0 = lane < H, h1 = lane + 64 < H;
  const float g0 = h0 ? d.g[(long long)b * d.ldg + lane] : 0.f, g1 = h1 ? d.g[(long long)b * d.ldg + lane + 64] : 0.f;
  const float u0 = h0 ? d.u[lane] : 0.f, u1 = h1 ? d.u[lane + 64] : 0.f;
  float dw = 0.f;  // this wave's share of D, over its steps in ascending order
  for (int t = wave; t < L; t += kAttnWaves) {
    const long long row = (long long)t * B + b;
    const float* rr = d.r + row * H;
    const float r0 = h0 ? rr[lane] : 0.f, r1 = h1 ? rr[lane + 64] : 0.f;
    dw = fmaf(d.alpha[row], wave_sum(fmaf(g1, r1, g0 * r0)), dw);
  }
  if (lane == 0) dsh[wave] = dw;
  __syncthreads();
  const float D = ((dsh[0] + dsh[1]) + dsh[2]) + dsh[3];
  float du0 = 0.f, du1 = 0.f, dc0 = 0.f, dc1 = 0.f;
  for (int t = wave; t < L; t += kAttnWaves) {
    const long long row = (long long)t * B + b;
    const float* rr = d.r + row * H;
    const float* zr = d.z + row * H;
    float* dpr = d.dp + row * H;
    const float r0 = h0 ? rr[lane] : 0.f, r1 = h1 ? rr[lane + 64] : 0.f;
    const float z0 = h0 ? zr[lane] : 0.f, z1 = h1 ? zr[lane + 64] : 0.f;
    const float a = wave_sum(fmaf(g1, r1, g0 * r0));
    const float ds = d.alpha[row] * (a - D);
    if (h0) dpr[lane] = ds * u0 * (1.f - z0 * z0);
    if (h1) dpr[lane + 64] = ds * u1 * (1.f - z1 * z1);
    du0 = fmaf(ds, z0, du0);
    du1 = fmaf(ds, z1, du1);
    dc0 = fmaf(ds * z0, z0, dc0);
    dc1 = fmaf(ds * z1, z1, dc1);
  }
  for (int t = L + wave; t < T; t += kAttnWaves) {
    float* dpr = d.dp + ((long long)t * B + b) * H;
    if (h0) dpr[lane] = 0.f;
    if (h1) dpr[lane + 64] = 0.f;
  }
  dus[wave][lane] = du0;
  dus[wave][lane + 64] = du1;
  dcs[wave][lane] = dc0;
  dcs[wave][lane + 64] = dc1;
  __syncthreads();
  if (tid < H) {
    float* row = d.rows + (long long)b * 2 * H;
    row[tid] = ((dus[0][tid] + dus[1][tid]) + dus[2][tid]) + dus[3][tid];
    row[H + tid] = -d.u[tid] * (((dcs[0][tid] + dcs[1][tid]) + dcs[2][tid]) + dcs[3][tid]);
  }
}

__global__ __launch_bounds__(kAttnThreads) void k_attn_pool_bwd(AttnBwdDesc d0, AttnBwdDesc d1, int nb0) {
  if ((int)blockIdx.x < nb0)
    attn_bwd_body(d0, blockIdx.x);
  else
    attn_bwd_body(d1, blockIdx.x - nb0);
}

// du[h] = sum_b rows[b][h], dc[h] = sum_b rows[b][H + h] in index order: one workgroup per problem, thread h
__global__ __launch_bounds__(128) void k_attn_du(AttnBwdDesc d0, AttnBwdDesc d1) {
  const AttnBwdDesc& d = blockIdx.x == 0 ? d0 : d1;
  const int h = threadIdx.x;
  if (h >= d.H) return;
  float su = 0.f, sc = 0.f;
  for (int b = 0; b < d.B; ++b) {
    su += d.rows[(long long)b * 2 * d.H + h];
    sc += d.rows[(long long)b * 2 * d.H + d.H + h];
  }
  d.du[h] = su;
  d.dc[h] = sc;
}

bool attn_shape_ok(int B, int T, int H, const int32_t* lens) {
  return B > 0 && T > 0 && H >= 4 && H <= 128 && (H & 3) == 0 && lens && (long long)T * B <= 0x7fffffffLL;
}
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int tspm_attn_pool_fwd(int32_t count, const tspm_attn_pool_fwd_desc* descs, tspm_stream_t stream) {
  if (count < 1 || count > 2 || !descs) return TSPM_ERR_INVALID;
  AttnFwdDesc d[2];
  for (int i = 0; i < count; ++i) {  // every descriptor before the launch
    const tspm_attn_pool_fwd_desc& s = descs[i];
    if (!attn_shape_ok(s.batch, s.steps, s.hidden, s.lengths) || s.ld_out < s.hidden || (s.norm != 0 && s.norm != 1) ||
        !s.r || !aligned16(s.r) || !s.alpha || !s.h_out || (s.norm == 0 && (!s.p || !s.u || !aligned16(s.p))))
      return TSPM_ERR_INVALID;
    d[i] = {s.batch, s.steps, s.hidden, s.ld_out, s.norm, s.r, s.p, s.u, s.alpha, s.h_out, s.lengths};
  }
  const int nb0 = d[0].B, nb1 = count > 1 ? d[1].B : 0;
  hipLaunchKernelGGL(k_attn_pool_fwd, dim3(nb0 + nb1), dim3(kAttnThreads), 0, static_cast<hipStream_t>(stream), d[0],
                     d[count - 1], nb0);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}

extern "C" int tspm_attn_pool_bwd(int32_t count, const tspm_attn_pool_bwd_desc* descs, tspm_stream_t stream) {
  if (count < 1 || count > 2 || !descs) return TSPM_ERR_INVALID;
  AttnBwdDesc d[2];
  for (int i = 0; i < count; ++i) {
    const tspm_attn_pool_bwd_desc& s = descs[i];
    if (!attn_shape_ok(s.batch, s.steps, s.hidden, s.lengths) || s.ld_g < s.hidden || s.norm != 0 || !s.g || !s.alpha || !s.z || !s.r || !s.u || !s.dp || !s.du || !s.dc || !s.rows ||
        !aligned16(s.r) || !aligned16(s.z) || !aligned16(s.dp))
      return TSPM_ERR_INVALID;
    d[i] = {s.batch, s.steps, s.hidden, s.ld_g, s.g, s.alpha, s.z, s.r, s.u, s.dp, s.du, s.dc, s.rows, s.lengths};
  }
  const int nb0 = d[0].B, nb1 = count > 1 ? d[1].B : 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_attn_pool_bwd, dim3(nb0 + nb1), dim3(kAttnThreads), 0, st, d[0], d[count - 1], nb0);
  TSPM_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_attn_du, dim3(count), dim3(128), 0, st, d[0], d[count - 1]);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}
