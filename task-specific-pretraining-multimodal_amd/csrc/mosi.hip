// MOSI UTT-Fusion (BASELINE configs[4]; MML_Suite/models/msa/utt_fusion.py:25-200 with
// configs/mosi/centralised/utt_fusion_base_training.yaml): the recurrent LSTM encoders
// (models/msa/networks/lstm.py:8-67, nn.LSTM(batch_first) + "last" embedding), the TextCNN time-max
// pooling and its sparse weight gradient (models/msa/networks/textcnn.py:10-69), the global-norm
// gradient clip of train_step (utt_fusion.py:189, torch.nn.utils.clip_grad_norm_) and the padded
// sequence gather (data/mosi.py:202-232, pad_sequence).  The dense products around them (the LSTM
// input projection and weight gradients, the TextCNN convolutions, every Linear) run on the shared
// MFMA GEMM / implicit-GEMM conv kernels.
//
// Layout: sequences are TIME-MAJOR on the device — row (t, b) of a [T][B][F] tensor — so every
// step's rows are contiguous, the LSTM weight gradients are plain GEMMs over the T*B rows, and the
// text input is an HWNC tensor (H = T, W = 1, N = B, C = 768) for the LDS-staged conv kernel.
#include <type_traits>

#include "common.h"

namespace {

TSPM_DEV float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// ------------------------------------------------------------------------------------------------
// LSTM forward: one workgroup per RB batch rows runs all T steps; thread j (of 4H) owns gate column
// j and keeps row j of W_hh in registers; h_{t-1} is broadcast from LDS.  ATen's LSTMCell order:
// gates = (h W_hh^T + b_hh) + (x W_ih^T + b_ih); i,f,o = sigmoid, g = tanh; c = f*c + i*g;
// h = o * tanh(c).  Saved for the backward: activated gates, c_t, h_t.
// ------------------------------------------------------------------------------------------------
// Per-sample lengths (tspm_lstm_fwd_len / tspm_lstm_bwd_len): row b runs L_b = min(max(lens[b], 1), T) steps and its
// state freezes there (pack_padded_sequence).  Every thread of a workgroup reads the lengths of ALL the workgroup's RB
// rows (the ghost row of an odd batch through its clamped index) from the same addresses, so `bound`, the trip count
// of the time loop that holds the barriers, is the same in every thread; a thread's own row (`mine`) only masks work
// between barriers.  The general template (Len false) is empty and folds to the unmasked code.
template <int RB, bool Len>
struct LstmLens {
  static constexpr int mine = 0;
  TSPM_DEV LstmLens(const int32_t*, const int*, int, int) {}
  TSPM_DEV LstmLens(const int32_t*, int, int, int, int) {}
  TSPM_DEV int bound(int T) const { return T; }
  TSPM_DEV bool row_runs(int, int) const { return true; }
  TSPM_DEV bool mine_runs(int) const { return true; }
};
template <int RB>
struct LstmLens<RB, true> {
  int len[RB];  // the workgroup's rows' clamped lengths (uniform)
  int mine;     // the length of this thread's cell row (0 for a thread that owns no cell)
  TSPM_DEV LstmLens(const int32_t* lens, const int* rowc, int T, int cr) {
    mine = 0;
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      len[r] = min(max(lens[rowc[r]], 1), T);
      if (r == cr) mine = len[r];
    }
  }
  TSPM_DEV LstmLens(const int32_t* lens, int b0, int B, int T, int cr) {  // the backward: rows clamped here
    mine = 0;
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      len[r] = min(max(lens[min(b0 + r, B - 1)], 1), T);
      if (r == cr) mine = len[r];
    }
  }
  TSPM_DEV int bound(int) const {
    int m = len[0];
#pragma unroll
    for (int r = 1; r < RB; ++r) m = max(m, len[r]);
    return m;
  }
  TSPM_DEV bool row_runs(int r, int t) const { return t < len[r]; }
  TSPM_DEV bool mine_runs(int t) const { return t < mine; }
};

// One problem of a launch.  The "maxpool" time index `arg` is untyped here: the kernels' template parameter Ix says
// whether it is uint8_t (steps <= 256) or uint16_t (steps <= 65535), and the bodies cast it where they use it.
struct LstmFwdDesc {
  int B, T;
  const float* xg;   // [T][B][4H]: x W_ih^T + b_ih
  const float* whh;  // [4H][H]
  const float* bhh;  // [4H] or null
  float* gates;      // [T][B][4H] activated i, f, g, o
  float* cs;         // [T][B][H]
  float* hs;         // [T+1][B][H], hs[0] = 0
  float* hout;       // h_T rows (embd "last") or max_t h_t (embd "maxpool"), stride ldh
  int ldh;
  void* arg;         // embd "maxpool": Ix [B][H] time index of the maximum (F.max_pool1d), else null
};

// What a kernel takes per problem after the descriptor, as a pack X of plain kernel arguments: `int` — the run-time
// width, absent when the width is the compile-time HP (Fixed) — then `const int32_t*` — the lengths, present with Len.
// A kernel so carries only what it reads, and its argument list is (d0, x0..., d1, x1..., nb0).
struct LstmExtra {
  int H;  // unused when Fixed
  const int32_t* lens;
};
TSPM_DEV LstmExtra lstm_extra() { return {0, nullptr}; }
TSPM_DEV LstmExtra lstm_extra(int H) { return {H, nullptr}; }
TSPM_DEV LstmExtra lstm_extra(const int32_t* lens) { return {0, lens}; }
TSPM_DEV LstmExtra lstm_extra(int H, const int32_t* lens) { return {H, lens}; }
template <typename... X> constexpr bool kLstmFixed = !(std::is_same_v<X, int> || ...);
template <typename... X> constexpr bool kLstmLen = (std::is_same_v<X, const int32_t*> || ...);

// The reductions are guarded per chunk of this many lanes, not per float4 group: one wave-uniform branch per chunk (at
// most 4; 32 per-group guards hoisted out of the time loop as scalar masks spilled 55 / 113 SGPRs in the 128 tier) and
// the chunk's LDS reads in flight together.  Inside a chunk that straddles the width the padded products are 0 x 0: a
// padded weight is zero and a padded h / gate-gradient slot of LDS is zero from the start and never written, so no NaN
// of a real unit can meet a padded zero.
constexpr int kLstmChunk = 32;

// The forward recurrence on HP lanes per gate.  Thread (q, u) = (gate, unit) of 4 * HP owns gate column q * H + u when
// u < H.  Width policy: Fixed — H is HP itself, every guard on H folds away and the k loop is one straight unrolled
// chain; otherwise H (a multiple of 4, 4 <= H <= HP) comes with the problem: a padded lane (u >= H) holds zero weights,
// reads and writes no global memory and never writes h (its LDS slot stays the initial zero), a chunk of the k loop
// wholly past H is skipped, and at H = HP the fmaf sequence is the fixed one's.  Memory layouts carry the real H: xg /
// gates [T][B][4H], cs [T][B][H], hs [T+1][B][H].  Len: per-row lengths, see "Per-sample lengths" above.
template <int HP, int RB, typename Ix, bool Fixed, bool Len>
TSPM_DEV void lstm_fwd_body(const LstmFwdDesc& d, const LstmExtra x, int chunk) {
  const int H = Fixed ? HP : x.H;
  const int32_t* lens = x.lens;
  constexpr int GP = 4 * HP;
  __shared__ __attribute__((aligned(16))) float hsh[RB][HP];
  __shared__ float gsh[RB][GP];
  const int tid = threadIdx.x;
  const int q = tid / HP, u = tid - (tid / HP) * HP;
  const bool live = u < H;
  const int G = 4 * H;
  const int j = q * H + u;  // the gate column in memory (live lanes)
  const int b0 = chunk * RB;
  const int B = d.B, T = d.T;
  float w[HP];
#pragma unroll
  for (int k = 0; k < HP; k += 4) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (live && k < H) v = ld4(d.whh + (long long)j * H + k);
    w[k] = v[0]; w[k + 1] = v[1]; w[k + 2] = v[2]; w[k + 3] = v[3];
  }
  const float bh = (live && d.bhh) ? d.bhh[j] : 0.f;
  // cell threads: (row cr, unit cu) = (q, u) of the first RB gate blocks; the ghost row of an odd batch reads the
  // last real row's inputs (clamped index) and writes nothing
  const int cr = q, cu = u;
  const bool upd = tid < RB * HP && live;
  const bool cell = upd && b0 + cr < B;
  float c = 0.f, h = 0.f;
  float mx = -INFINITY;  // embd "maxpool": running max over t of h_t and its first index (NaN wins, as
  int am = 0;            // max_pool2d_with_indices: val > max || isnan(val))
  if (tid < RB * HP) hsh[cr][cu] = 0.f;
  if (cell) d.hs[(long long)(b0 + cr) * H + cu] = 0.f;
  // i, f, o = sigmoid, g = tanh.  The fixed spelling is kept as it is: `q != 2` gives the fixed-width kernels another
  // register assignment.
  const bool sig = Fixed ? (tid < 2 * HP || tid >= 3 * HP) : q != 2;
  int rowc[RB];  // clamped row of each of the workgroup's rows
#pragma unroll
  for (int r = 0; r < RB; ++r) rowc[r] = min(b0 + r, B - 1);
  float xn[RB];
#pragma unroll
  for (int r = 0; r < RB; ++r) xn[r] = live ? d.xg[(long long)rowc[r] * G + j] : 0.f;
  const LstmLens<RB, Len> ln(lens, rowc, T, cr);
  const int TL = ln.bound(T);
  __syncthreads();
  for (int t = 0; t < TL; ++t) {
    float xc[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) xc[r] = xn[r];
    if (t + 1 < TL && live) {
#pragma unroll
      for (int r = 0; r < RB; ++r) xn[r] = d.xg[((long long)(t + 1) * B + rowc[r]) * G + j];
    }
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      if (!ln.row_runs(r, t)) continue;  // workgroup-uniform: a finished row's gates are not formed
      float a4[4] = {0.f, 0.f, 0.f, 0.f};  // four interleaved partial sums (k mod 4): an H/4-deep chain, not H
#pragma unroll
      for (int k0 = 0; k0 < HP; k0 += kLstmChunk) {
        if (k0 < H) {  // wave-uniform: a chunk wholly past the width is skipped
#pragma unroll
          for (int k = k0; k < k0 + kLstmChunk; k += 4) {
            const f32x4 hv = *reinterpret_cast<const f32x4*>(&hsh[r][k]);
#pragma unroll
            for (int v = 0; v < 4; ++v) a4[v] = fmaf(hv[v], w[k + v], a4[v]);
          }
        }
      }
      const float acc = (a4[0] + a4[1]) + (a4[2] + a4[3]);
      const float pre = (acc + bh) + xc[r];
      const float a = sig ? sigmoidf_(pre) : tanhf(pre);
      gsh[r][tid] = a;
      if (live && b0 + r < B) d.gates[((long long)t * B + b0 + r) * G + j] = a;
    }
    __syncthreads();
    if (upd && ln.mine_runs(t)) {
      const float ig = gsh[cr][cu], fg = gsh[cr][HP + cu], gg = gsh[cr][2 * HP + cu], og = gsh[cr][3 * HP + cu];
      c = fg * c + ig * gg;
      h = og * tanhf(c);
      hsh[cr][cu] = h;
    }
    if (cell && ln.mine_runs(t)) {
      const long long o = ((long long)t * B + b0 + cr) * H + cu;
      d.cs[o] = c;
      d.hs[o + (long long)B * H] = h;
      if (d.arg && (h > mx || h != h)) {
        mx = h;
        am = t;
      }
    }
    __syncthreads();
  }
  if (cell) {
    d.hout[(long long)(b0 + cr) * d.ldh + cu] = d.arg ? mx : h;
    if (d.arg) static_cast<Ix*>(d.arg)[(long long)(b0 + cr) * H + cu] = (Ix)am;
    if constexpr (Len) {  // hs past the row's length: zeros (pad_packed_sequence; dW_hh's GEMM reads these rows)
      for (int t = ln.mine; t < T; ++t) d.hs[((long long)(t + 1) * B + b0 + cr) * H + cu] = 0.f;
    }
  }
}

// Both problems of a launch: workgroups [0, nb0) run problem 0, the rest problem 1 (a count-1 launch passes its
// problem twice and nb0 = the grid).
template <int HP, int RB, typename Ix, typename... X>
__global__ __launch_bounds__(4 * HP) void k_lstm_fwd(LstmFwdDesc d0, X... x0, LstmFwdDesc d1, X... x1, int nb0) {
  static_assert(RB <= 4, "cell threads are the first RB gate blocks");
  if ((int)blockIdx.x < nb0)
    lstm_fwd_body<HP, RB, Ix, kLstmFixed<X...>, kLstmLen<X...>>(d0, lstm_extra(x0...), blockIdx.x);
  else
    lstm_fwd_body<HP, RB, Ix, kLstmFixed<X...>, kLstmLen<X...>>(d1, lstm_extra(x1...), blockIdx.x - nb0);
}

// ------------------------------------------------------------------------------------------------
// LSTM backward through time: thread (q, k) = (gate quarter, hidden unit) keeps column k of the
// quarter-q rows of W_hh in registers for dh_{t-1} = dgates_t @ W_hh (4 partial sums combined in
// fixed order through LDS); threads (r, u) carry dc and form the pre-activation gate gradients
// (written time-major for the weight-gradient GEMMs that follow).
// ------------------------------------------------------------------------------------------------
struct LstmBwdDesc {
  int B, T;
  const float* whh;    // [4H][H]
  const float* gates;  // [T][B][4H]
  const float* cs;     // [T][B][H]
  const float* dh;     // gradient of the embedding rows (h_T, or max_t h_t at arg), stride lddh
  int lddh;
  float* dgates;       // [T][B][4H] out
  const void* arg;     // embd "maxpool": Ix [B][H] time index that received the embedding (null: T-1)
};

// On HP lanes per gate quarter, with the forward's width policy: a padded lane (k >= H) keeps zeros for its column of
// W_hh, the unrolled jj loop runs in guarded chunks of kLstmChunk as the forward's k loop, padded lanes read and write
// no global memory, and only units < H are ever read back from LDS.  The step bounds are spelled with compile-time
// ternaries on Len (not through LstmLens), which the front end folds before any pass sees them.
template <int HP, int RB, typename Ix, bool Fixed, bool Len>
TSPM_DEV void lstm_bwd_body(const LstmBwdDesc& d, const LstmExtra x, int chunk) {
  const int H = Fixed ? HP : x.H;
  const int32_t* lens = x.lens;
  constexpr int GP = 4 * HP;
  __shared__ __attribute__((aligned(16))) float dgs[RB][GP];
  __shared__ float part[4][RB][HP];
  const int tid = threadIdx.x;
  const int q = tid / HP, k = tid - (tid / HP) * HP;
  const bool live = k < H;
  const int G = 4 * H;
  const int b0 = chunk * RB;
  const int B = d.B, T = d.T;
  float wc[HP];
#pragma unroll
  for (int jj = 0; jj < HP; ++jj) wc[jj] = (live && jj < H) ? d.whh[(long long)(q * H + jj) * H + k] : 0.f;
  const int cr = q, cu = k;
  const bool cell = tid < RB * HP && live && b0 + cr < B;  // ghost rows and padded lanes compute zeros, write nothing
  float dc = 0.f, dh = 0.f, gin = 0.f;
  const LstmLens<RB, Len> ln(lens, b0, B, T, cr);
  int am = (Len ? ln.mine : T) - 1;  // the step whose h received the embedding gradient: the row's last step
  if (cell) {
    gin = d.dh[(long long)(b0 + cr) * d.lddh + cu];
    if (d.arg) am = static_cast<const Ix*>(d.arg)[(long long)(b0 + cr) * H + cu];
  }
  if (tid < RB * HP && !cell) {
    dgs[cr][cu] = 0.f; dgs[cr][HP + cu] = 0.f; dgs[cr][2 * HP + cu] = 0.f; dgs[cr][3 * HP + cu] = 0.f;
  }
  for (int t = (Len ? ln.bound(T) : T) - 1; t >= 0; --t) {
    if (cell && (!Len || t < ln.mine)) {
      if (t < (Len ? ln.mine : T) - 1) {
        dh = ((part[0][cr][cu] + part[1][cr][cu]) + part[2][cr][cu]) + part[3][cr][cu];
        if (t == am) dh += gin;  // max-pooled embedding: its gradient joins the recurrent one at the argmax
      } else {
        dh = am == (Len ? ln.mine : T) - 1 ? gin : 0.f;
      }
      const long long go = ((long long)t * B + b0 + cr) * G + cu;
      const float ig = d.gates[go], fg = d.gates[go + H], gg = d.gates[go + 2 * H], og = d.gates[go + 3 * H];
      const long long co = ((long long)t * B + b0 + cr) * H + cu;
      const float c = d.cs[co];
      const float cp = t > 0 ? d.cs[co - (long long)B * H] : 0.f;
      const float tc = tanhf(c);
      const float dog = dh * tc;
      const float dcc = dc + dh * og * (1.f - tc * tc);
      const float dig = dcc * gg, dgg = dcc * ig, dfg = dcc * cp;
      dc = dcc * fg;
      const float ai = dig * ig * (1.f - ig), af = dfg * fg * (1.f - fg);
      const float ag = dgg * (1.f - gg * gg), ao = dog * og * (1.f - og);
      dgs[cr][cu] = ai; dgs[cr][HP + cu] = af; dgs[cr][2 * HP + cu] = ag; dgs[cr][3 * HP + cu] = ao;
      d.dgates[go] = ai; d.dgates[go + H] = af; d.dgates[go + 2 * H] = ag; d.dgates[go + 3 * H] = ao;
    }
    __syncthreads();
    if (t > 0) {
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        if constexpr (Len) {
          if (!ln.row_runs(r, t)) continue;  // workgroup-uniform: the row has not started yet
        }
        float a4[4] = {0.f, 0.f, 0.f, 0.f};  // interleaved partial sums, as in the forward
#pragma unroll
        for (int j0 = 0; j0 < HP; j0 += kLstmChunk) {
          if (j0 < H) {  // wave-uniform: a chunk wholly past the width is skipped
#pragma unroll
            for (int jj = j0; jj < j0 + kLstmChunk; jj += 4) {
              const f32x4 dv = *reinterpret_cast<const f32x4*>(&dgs[r][q * HP + jj]);
#pragma unroll
              for (int v = 0; v < 4; ++v) a4[v] = fmaf(dv[v], wc[jj + v], a4[v]);
            }
          }
        }
        part[q][r][k] = (a4[0] + a4[1]) + (a4[2] + a4[3]);
      }
    }
    __syncthreads();
  }
  if constexpr (Len) {  // gate gradients past the row's length: zeros, so the weight-gradient GEMMs keep all T*B rows
    if (cell) {
      for (int t = ln.mine; t < T; ++t) {
        const long long go = ((long long)t * B + b0 + cr) * G + cu;
        d.dgates[go] = 0.f; d.dgates[go + H] = 0.f; d.dgates[go + 2 * H] = 0.f; d.dgates[go + 3 * H] = 0.f;
      }
    }
  }
}

template <int HP, int RB, typename Ix, typename... X>
__global__ __launch_bounds__(4 * HP) void k_lstm_bwd(LstmBwdDesc d0, X... x0, LstmBwdDesc d1, X... x1, int nb0) {
  static_assert(RB <= 4, "cell threads are the first RB gate quarters");
  if ((int)blockIdx.x < nb0)
    lstm_bwd_body<HP, RB, Ix, kLstmFixed<X...>, kLstmLen<X...>>(d0, lstm_extra(x0...), blockIdx.x);
  else
    lstm_bwd_body<HP, RB, Ix, kLstmFixed<X...>, kLstmLen<X...>>(d1, lstm_extra(x1...), blockIdx.x - nb0);
}

// ------------------------------------------------------------------------------------------------
// The same backward with a gradient at EVERY step (tspm_lstm_bwd_seq; the "attention" embedding weights all of r_out):
// dh_t = (the recurrent term) [+ wt[t][b] * dh[b]] [+ dseq[t][b]] for t < L_b.  It exists with lengths only and needs
// no time index.  A body and a descriptor of its own, not one more mode of lstm_bwd_body: the two extra pointers would
// change LstmBwdDesc, the argument list of every existing backward kernel, and those kernels stay instruction for
// instruction what they were.  The loop is lstm_bwd_body's with Len; with dseq and wt null the arithmetic is the same.
// ------------------------------------------------------------------------------------------------
struct LstmBwdSeqDesc {
  int B, T;
  const float* whh;    // [4H][H]
  const float* gates;  // [T][B][4H]
  const float* cs;     // [T][B][H]
  const float* dh;     // [B] rows of stride lddh, or null
  int lddh;
  float* dgates;       // [T][B][4H] out
  const float* dseq;   // [T][B][H] or null
  const float* wt;     // [T][B] or null: dh enters every step with this weight (null: at the row's last step)
};

template <int HP, int RB, bool Fixed>
TSPM_DEV void lstm_bwd_seq_body(const LstmBwdSeqDesc& d, const LstmExtra x, int chunk) {
  const int H = Fixed ? HP : x.H;
  constexpr int GP = 4 * HP;
  __shared__ __attribute__((aligned(16))) float dgs[RB][GP];
  __shared__ float part[4][RB][HP];
  const int tid = threadIdx.x;
  const int q = tid / HP, k = tid - (tid / HP) * HP;
  const bool live = k < H;
  const int G = 4 * H;
  const int b0 = chunk * RB;
  const int B = d.B, T = d.T;
  float wc[HP];
#pragma unroll
  for (int jj = 0; jj < HP; ++jj) wc[jj] = (live && jj < H) ? d.whh[(long long)(q * H + jj) * H + k] : 0.f;
  const int cr = q, cu = k;
  const bool cell = tid < RB * HP && live && b0 + cr < B;  // ghost rows and padded lanes compute zeros, write nothing
  float dc = 0.f, dh = 0.f, gin = 0.f;
  const LstmLens<RB, true> ln(x.lens, b0, B, T, cr);
  const int last = ln.mine - 1;
  const float* wt = d.dh ? d.wt : nullptr;  // without dh there is nothing to weight
  if (cell && d.dh) gin = d.dh[(long long)(b0 + cr) * d.lddh + cu];
  if (tid < RB * HP && !cell) {
    dgs[cr][cu] = 0.f; dgs[cr][HP + cu] = 0.f; dgs[cr][2 * HP + cu] = 0.f; dgs[cr][3 * HP + cu] = 0.f;
  }
  // A step's operands — its gates, c_{t-1}, wt and dseq — are fetched one step ahead, after the previous step's stores:
  // they arrive while the recurrent product below runs instead of standing between the barrier and the cell arithmetic
  // (fetched at the step itself, behind their own branches, wt and dseq each cost the loop one more memory round trip
  // per step).  c_t is the previous step's c_{t-1}.  The arithmetic is untouched.
  float nig = 0.f, nfg = 0.f, ngg = 0.f, nog = 0.f, ncc = 0.f, ncp = 0.f, nwt = 0.f, nds = 0.f;
  auto fetch = [&](int t) {
    const long long row = (long long)t * B + b0 + cr;
    const long long go = row * G + cu;
    nig = d.gates[go]; nfg = d.gates[go + H]; ngg = d.gates[go + 2 * H]; nog = d.gates[go + 3 * H];
    ncp = t > 0 ? d.cs[row * H + cu - (long long)B * H] : 0.f;
    if (wt) nwt = wt[row];
    if (d.dseq) nds = d.dseq[row * H + cu];
  };
  if (cell) {  // the row's first step, L_b - 1: nothing of dseq / wt at t >= L_b is ever read
    ncc = d.cs[((long long)last * B + b0 + cr) * H + cu];
    fetch(last);
  }
  for (int t = ln.bound(T) - 1; t >= 0; --t) {
    if (cell && t < ln.mine) {
      if (t < last)
        dh = ((part[0][cr][cu] + part[1][cr][cu]) + part[2][cr][cu]) + part[3][cr][cu];
      else
        dh = wt ? 0.f : gin;  // the row's last step: where "last" puts the embedding gradient
      if (wt) dh = fmaf(nwt, gin, dh);
      if (d.dseq) dh += nds;
      const long long go = ((long long)t * B + b0 + cr) * G + cu;
      const float ig = nig, fg = nfg, gg = ngg, og = nog, c = ncc, cp = ncp;
      const float tc = tanhf(c);
      const float dog = dh * tc;
      const float dcc = dc + dh * og * (1.f - tc * tc);
      const float dig = dcc * gg, dgg = dcc * ig, dfg = dcc * cp;
      dc = dcc * fg;
      const float ai = dig * ig * (1.f - ig), af = dfg * fg * (1.f - fg);
      const float ag = dgg * (1.f - gg * gg), ao = dog * og * (1.f - og);
      dgs[cr][cu] = ai; dgs[cr][HP + cu] = af; dgs[cr][2 * HP + cu] = ag; dgs[cr][3 * HP + cu] = ao;
      d.dgates[go] = ai; d.dgates[go + H] = af; d.dgates[go + 2 * H] = ag; d.dgates[go + 3 * H] = ao;
      if (t > 0) {
        ncc = cp;
        fetch(t - 1);
      }
    }
    __syncthreads();
    if (t > 0) {
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        if (!ln.row_runs(r, t)) continue;  // workgroup-uniform: the row has not started yet
        float a4[4] = {0.f, 0.f, 0.f, 0.f};  // interleaved partial sums, as in the forward
#pragma unroll
        for (int j0 = 0; j0 < HP; j0 += kLstmChunk) {
          if (j0 < H) {  // wave-uniform: a chunk wholly past the width is skipped
#pragma unroll
            for (int jj = j0; jj < j0 + kLstmChunk; jj += 4) {
              const f32x4 dv = *reinterpret_cast<const f32x4*>(&dgs[r][q * HP + jj]);
#pragma unroll
              for (int v = 0; v < 4; ++v) a4[v] = fmaf(dv[v], wc[jj + v], a4[v]);
            }
          }
        }
        part[q][r][k] = (a4[0] + a4[1]) + (a4[2] + a4[3]);
      }
    }
    __syncthreads();
  }
  if (cell) {  // gate gradients past the row's length: zeros, so the weight-gradient GEMMs keep all T*B rows
    for (int t = ln.mine; t < T; ++t) {
      const long long go = ((long long)t * B + b0 + cr) * G + cu;
      d.dgates[go] = 0.f; d.dgates[go + H] = 0.f; d.dgates[go + 2 * H] = 0.f; d.dgates[go + 3 * H] = 0.f;
    }
  }
}

template <int HP, int RB, typename... X>
__global__ __launch_bounds__(4 * HP) void k_lstm_bwd_seq(LstmBwdSeqDesc d0, X... x0, LstmBwdSeqDesc d1, X... x1, int nb0) {
  static_assert(RB <= 4 && kLstmLen<X...>, "cell threads are the first RB gate quarters; the lengths are required");
  if ((int)blockIdx.x < nb0)
    lstm_bwd_seq_body<HP, RB, kLstmFixed<X...>>(d0, lstm_extra(x0...), blockIdx.x);
  else
    lstm_bwd_seq_body<HP, RB, kLstmFixed<X...>>(d1, lstm_extra(x1...), blockIdx.x - nb0);
}

// ------------------------------------------------------------------------------------------------
// TextCNN pooling: conv_i [Tout_i][B][C] (+ bias) -> ReLU -> max over time (first maximum, as
// F.max_pool1d) for every (b, conv i, channel); the result (and its dropout, textcnn.py:66) goes to
// the embedding Linear's input.  The argmax time index and the pooled value are kept for the backward.
// ------------------------------------------------------------------------------------------------
struct PoolSet {
  const float* y[4];
  const float* bias[4];
  int kh[4];
};

__global__ __launch_bounds__(256) void k_textcnn_pool(int B, int T, int nconv, int C, PoolSet ps,
                                                      const uint8_t* __restrict__ keep, float scale,
                                                      float* __restrict__ pre, uint8_t* __restrict__ arg,
                                                      float* __restrict__ out, int ldo) {
  const int nc = nconv * C;
  const long long total = (long long)B * nc;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int b = (int)(e / nc), ci = (int)(e - (long long)b * nc);
    const int i = ci / C, c = ci - i * C;
    const int tout = T - ps.kh[i] + 1;
    const float* y = ps.y[i];
    const float bv = ps.bias[i] ? ps.bias[i][c] : 0.f;
    float best = -1.f;
    int bi = 0;
    for (int t = 0; t < tout; ++t) {
      float v = y[((long long)t * B + b) * C + c] + bv;
      v = v > 0.f ? v : (v != v ? v : 0.f);  // ReLU (NaN propagates)
      if (v > best || v != v) { best = v; bi = t; }
    }
    pre[e] = best;
    arg[e] = (uint8_t)bi;
    out[(long long)b * ldo + ci] = keep ? best * (keep[e] ? scale : 0.f) : best;
  }
}

// The same pooling over each row's own windows (tspm_textcnn_pool_fwd_len): row b has max(L_b - kh_i + 1, 1) of them, L_b =
// lengths[b] clamped to 1..T here.  A kernel of its own, not a template parameter of k_textcnn_pool: sharing the loop
// body through a device function changed the unmasked kernel's instructions, and that kernel stays as it was.
__global__ __launch_bounds__(256) void k_textcnn_pool_len(int B, int T, int nconv, int C, PoolSet ps,
                                                          const uint8_t* __restrict__ keep, float scale,
                                                          float* __restrict__ pre, uint8_t* __restrict__ arg,
                                                          float* __restrict__ out, int ldo,
                                                          const int32_t* __restrict__ lengths) {
  const int nc = nconv * C;
  const long long total = (long long)B * nc;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int b = (int)(e / nc), ci = (int)(e - (long long)b * nc);
    const int i = ci / C, c = ci - i * C;
    const int lb = min(max(lengths[b], 1), T);
    const int tout = max(lb - ps.kh[i] + 1, 1);  // <= T - kh + 1: no length moves a read outside conv_out
    const float* y = ps.y[i];
    const float bv = ps.bias[i] ? ps.bias[i][c] : 0.f;
    float best = -1.f;
    int bi = 0;
    for (int t = 0; t < tout; ++t) {
      float v = y[((long long)t * B + b) * C + c] + bv;
      v = v > 0.f ? v : (v != v ? v : 0.f);  // ReLU (NaN propagates)
      if (v > best || v != v) { best = v; bi = t; }
    }
    pre[e] = best;
    arg[e] = (uint8_t)bi;
    out[(long long)b * ldo + ci] = keep ? best * (keep[e] ? scale : 0.f) : best;
  }
}

// grad of the pooled features: through the dropout (keep * scale) and the ReLU at the argmax.
__global__ __launch_bounds__(256) void k_textcnn_pool_grad(long long total, int nc, const float* __restrict__ dout,
                                                           int ldd, const uint8_t* __restrict__ keep, float scale,
                                                           const float* __restrict__ pre, float* __restrict__ g) {
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const long long b = e / nc, ci = e - b * nc;
    float v = dout[b * ldd + ci];
    if (keep) v = v * (keep[e] ? scale : 0.f);
    g[e] = pre[e] > 0.f ? v : 0.f;
  }
}

// Sparse weight gradient of conv i: dW[c][dt][f] = sum_b g[b][c] x[arg[b][c] + dt][b][f] (only the
// argmax position of each (b, c) carries gradient after the time-max), db[c] = sum_b g[b][c].
// One workgroup per (conv, channel); threads over f; the kh rows of a window accumulate in registers.
struct WgradSet {
  float* dw[4];
  float* db[4];
  int kh[4];
};

template <int KMAX, int FPT>
__global__ __launch_bounds__(256) void k_textcnn_wgrad(int B, int F, int C, WgradSet ws, const float* __restrict__ x,
                                                       const float* __restrict__ g, const uint8_t* __restrict__ arg,
                                                       int nc) {
  const int i = blockIdx.x / C, c = blockIdx.x - (blockIdx.x / C) * C;
  const int kh = ws.kh[i];
  const int ci = i * C + c;
  float acc[KMAX][FPT];
#pragma unroll
  for (int dt = 0; dt < KMAX; ++dt)
#pragma unroll
    for (int u = 0; u < FPT; ++u) acc[dt][u] = 0.f;
  for (int b = 0; b < B; ++b) {
    const float gv = g[(long long)b * nc + ci];
    if (gv == 0.f) continue;  // workgroup-uniform
    const int t0 = arg[(long long)b * nc + ci];
#pragma unroll
    for (int dt = 0; dt < KMAX; ++dt) {
      if (dt >= kh) break;
      const float* row = x + ((long long)(t0 + dt) * B + b) * F;
#pragma unroll
      for (int u = 0; u < FPT; ++u) {
        const int f = threadIdx.x + 256 * u;
        if (f < F) acc[dt][u] = fmaf(gv, row[f], acc[dt][u]);
      }
    }
  }
  float* dw = ws.dw[i] + (long long)c * kh * F;
#pragma unroll
  for (int dt = 0; dt < KMAX; ++dt) {
    if (dt >= kh) break;
#pragma unroll
    for (int u = 0; u < FPT; ++u) {
      const int f = threadIdx.x + 256 * u;
      if (f < F) dw[(long long)dt * F + f] = acc[dt][u];
    }
  }
  if (threadIdx.x == 0 && ws.db[i]) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += g[(long long)b * nc + ci];
    ws.db[i][c] = s;
  }
}

// Same gradient, organised for HBM reuse (C = 128 channels): one workgroup per (conv, 8-float slice of
// the 768 features).  Each step stages NBS batch rows' [T][8] input slices, the g and argmax of those
// rows in LDS; thread (c = tid / 2, 4 features) accumulates dW[c][0..kh)[4] over b in ascending order —
// the same fmaf sequence as k_textcnn_wgrad, so the two are bitwise identical — while the input is read
// from HBM once per conv (T*B*F*4 bytes) instead of once per (channel, batch row) window.
constexpr int kWgFB = 8;    // features per workgroup
constexpr int kWgNBS = 8;   // batch rows staged per LDS round
constexpr int kWgC = 128;   // channels (2 threads each)

template <int KMAX>
__global__ __launch_bounds__(256) void k_textcnn_wgrad_slab(int B, int T, int F, WgradSet ws, const float* __restrict__ x,
                                                            const float* __restrict__ g,
                                                            const uint8_t* __restrict__ arg, int nc, int nfb) {
  __shared__ float4 xs[kWgNBS][256][kWgFB / 4];  // [row][t][8 floats]; T <= 256
  __shared__ float gs[kWgNBS][kWgC];
  __shared__ int as_[kWgNBS][kWgC];
  const int i = blockIdx.x / nfb, fb = blockIdx.x - (blockIdx.x / nfb) * nfb;
  const int kh = ws.kh[i], f0 = fb * kWgFB;
  const int tid = threadIdx.x, c = tid >> 1, half = tid & 1;
  const int ci = i * kWgC + c;
  float4 acc[KMAX];
#pragma unroll
  for (int dt = 0; dt < KMAX; ++dt) acc[dt] = make_float4(0.f, 0.f, 0.f, 0.f);
  float dbs = 0.f;
  for (int b0 = 0; b0 < B; b0 += kWgNBS) {
    const int nb = B - b0 < kWgNBS ? B - b0 : kWgNBS;
    __syncthreads();
    for (int e = tid; e < nb * T * 2; e += 256) {  // 2 float4 per (row, t)
      const int q = e & 1, rt = e >> 1, r = rt / T, t = rt - r * T;
      xs[r][t][q] = *reinterpret_cast<const float4*>(x + ((long long)t * B + b0 + r) * F + f0 + 4 * q);
    }
    for (int e = tid; e < nb * kWgC; e += 256) {
      const int r = e / kWgC, cc = e - r * kWgC;
      gs[r][cc] = g[(long long)(b0 + r) * nc + i * kWgC + cc];
      as_[r][cc] = arg[(long long)(b0 + r) * nc + i * kWgC + cc];
    }
    __syncthreads();
    for (int r = 0; r < nb; ++r) {
      const float gv = gs[r][c];
      if (half == 0) dbs += gv;
      if (gv == 0.f) continue;
      const int t0 = as_[r][c];
#pragma unroll
      for (int dt = 0; dt < KMAX; ++dt) {
        if (dt >= kh) break;
        const float4 v = xs[r][t0 + dt][half];
        acc[dt].x = fmaf(gv, v.x, acc[dt].x);
        acc[dt].y = fmaf(gv, v.y, acc[dt].y);
        acc[dt].z = fmaf(gv, v.z, acc[dt].z);
        acc[dt].w = fmaf(gv, v.w, acc[dt].w);
      }
    }
  }
  float* dw = ws.dw[i] + (long long)c * kh * F;
#pragma unroll
  for (int dt = 0; dt < KMAX; ++dt) {
    if (dt >= kh) break;
    *reinterpret_cast<float4*>(dw + (long long)dt * F + f0 + 4 * half) = acc[dt];
  }
  if (fb == 0 && half == 0 && ws.db[i]) ws.db[i][c] = dbs;
  (void)ci;
}

// ------------------------------------------------------------------------------------------------
// Global-norm gradient clip (torch.nn.utils.clip_grad_norm_, norm 2): sum of squares of
// (grad * grad_scale) in double per workgroup, then one workgroup sums the partials in index order
// and writes coef = min(1, max_norm / (total_norm + 1e-6)) for the Adam launch that follows.
// ------------------------------------------------------------------------------------------------
constexpr int kClipBlocks = 512;

__global__ __launch_bounds__(256) void k_sumsq(long long count, const float* __restrict__ g, float gs,
                                               double* __restrict__ partial) {
  __shared__ double red[256];
  double s = 0.0;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
    const double v = (double)(g[i] * gs);
    s += v * v;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// k_sumsq over several buffers (tspm_grad_clip_coef_multi): workgroups first[r] .. first[r+1]-1 sum range r with
// k_sumsq's loop and tree (one range over all kClipBlocks workgroups is k_sumsq bit for bit); the workgroups past
// first[nrange] write a zero partial, so k_clip_coef always reads kClipBlocks of them.
struct GradRanges {
  const float* g[TSPM_ADAM_MAX_SEGMENTS];
  long long count[TSPM_ADAM_MAX_SEGMENTS];
  int first[TSPM_ADAM_MAX_SEGMENTS + 1];
  int nrange;
};

__global__ __launch_bounds__(256) void k_sumsq_multi(GradRanges a, float gs, double* __restrict__ partial) {
  __shared__ double red[256];
  int r = 0;  // the last range whose first workgroup is <= this one (empty ranges share the next one's start)
#pragma unroll
  for (int i = 1; i < TSPM_ADAM_MAX_SEGMENTS; ++i)
    if (i < a.nrange && (int)blockIdx.x >= a.first[i]) r = i;
  const int blk = (int)blockIdx.x - a.first[r], nblk = a.first[r + 1] - a.first[r];
  const long long count = blk < nblk ? a.count[r] : 0;  // a left-over workgroup sums nothing
  const float* __restrict__ g = a.g[r];
  double s = 0.0;
  for (long long i = blk * 256LL + threadIdx.x; i < count; i += (long long)nblk * 256) {
    const double v = (double)(g[i] * gs);
    s += v * v;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// one workgroup: strided partial sums then a fixed-order LDS tree (deterministic; all loads in flight
// together instead of one thread's dependent chain)
__global__ __launch_bounds__(256) void k_clip_coef(int nparts, const double* __restrict__ partial, float max_norm,
                                                   float* __restrict__ coef, float* __restrict__ norm_out) {
  __shared__ double red[256];
  double a = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) a += partial[i];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double s = red[0];
  const float total = (float)sqrt(s);
  const float cf = max_norm / (total + 1e-6f);
  coef[0] = cf > 1.f ? 1.f : cf;  // torch.clamp(max=1): a NaN total gives a NaN coefficient (inf gives 0)
  if (norm_out) norm_out[0] = total;
}

// ------------------------------------------------------------------------------------------------
// Padded sequence gather (pad_sequence(batch_first) of data/mosi.py:225-230 + the step's .to(device)):
// out[t][b][:] (time-major, strides st / sb) = row offset[idx_b] + t of the ragged corpus if
// t < length[idx_b], else 0; times the per-row modality mask; labels gathered alongside.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_seq_gather(int nb, const int64_t* __restrict__ index, long long nsamp,
                                                    const float* __restrict__ data, const int64_t* __restrict__ offs,
                                                    const int32_t* __restrict__ lens, int F, int Tpad,
                                                    float* __restrict__ out, long long st, long long sb,
                                                    const float* __restrict__ mask, const int64_t* __restrict__ lab_in,
                                                    int64_t* __restrict__ lab_out) {
  const long long total = (long long)Tpad * nb * F;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int f = (int)(e % F);
    const long long tb = e / F;
    const int b = (int)(tb % nb), t = (int)(tb / nb);
    const long long s = index[b];
    float v;
    if (s < 0 || s >= nsamp) {
      v = __builtin_nanf("");
    } else {
      v = t < lens[s] ? data[(offs[s] + t) * (long long)F + f] : 0.f;
      if (mask) v = v * mask[b];
    }
    out[(long long)t * st + (long long)b * sb + f] = v;
    if (lab_out && t == 0 && f == 0) lab_out[b] = (s < 0 || s >= nsamp) ? -1 : lab_in[s];
  }
}

int grid_for(long long work) {
  long long b = cdiv64(work, 256);
  if (b > 4096) b = 4096;
  return (int)(b < 1 ? 1 : b);
}

// ------------------------------------------------------------------------------------------------
// Missing-modality pattern expansion: emb [2B][ld_emb] holds the embeddings of the real inputs (rows [0, B)) and of
// the zeroed inputs (rows [B, 2B)) as cat(audio, video, text); row (p, b) of out takes each modality's columns from
// row b when pattern p keeps it, else from row B + b.  A thread moves one unit of a row: a float4 of a segment whose
// width, column offset and both row strides are multiples of 4 (both bases 16-byte aligned), else one float.  Unit 0
// of a row also copies the row's label (4 or 8 bytes) and writes its group id.  The per-pattern tables ride in the
// kernel's arguments (as PoolSet does).
// ------------------------------------------------------------------------------------------------
struct PatternSet {
  int keep[TSPM_MAX_PATTERNS];   // bit m: modality m (audio, video, text) comes from the real row
  int group[TSPM_MAX_PATTERNS];
  int width[3], col[3], units[3], vec[3];
};

__global__ __launch_bounds__(256) void k_pattern_expand(int B, int npat, PatternSet ps, const float* __restrict__ emb,
                                                        long long ld_emb, float* __restrict__ out, long long ld_out,
                                                        const void* __restrict__ lab_in, void* __restrict__ lab_out,
                                                        int lab_bytes, int32_t* __restrict__ groups_out) {
  const int u0 = ps.units[0], u01 = u0 + ps.units[1], upr = u01 + ps.units[2];
  const long long total = (long long)npat * B * upr;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int u = (int)(e % upr);
    const long long row = e / upr;  // p * B + b
    const int b = (int)(row % B), p = (int)(row / B);
    const int m = u < u0 ? 0 : (u < u01 ? 1 : 2);
    const int uu = u - (m == 0 ? 0 : (m == 1 ? u0 : u01));
    const long long src = ((ps.keep[p] >> m) & 1) ? b : (long long)B + b;
    const float* s = emb + src * ld_emb + ps.col[m];
    float* d = out + row * ld_out + ps.col[m];
    if (ps.vec[m]) {
      reinterpret_cast<float4*>(d)[uu] = reinterpret_cast<const float4*>(s)[uu];
    } else {
      d[uu] = s[uu];
    }
    if (u == 0) {
      if (lab_bytes == 8) {
        static_cast<unsigned long long*>(lab_out)[row] = static_cast<const unsigned long long*>(lab_in)[b];
      } else {
        static_cast<unsigned*>(lab_out)[row] = static_cast<const unsigned*>(lab_in)[b];
      }
      groups_out[row] = ps.group[p];
    }
  }
}

// The adjoint of k_pattern_expand: demb [2B][ld_demb] row b takes, per modality, the sum of dout's rows (p, b) over the
// patterns that keep the modality, row B + b the sum over those that drop it.  One thread owns one unit of demb (the
// unit rule above) and adds the patterns in ascending p from +0.0 — plain fp32 adds, no atomics, so the host can
// restate it bit for bit; a slot no pattern uses is written +0.0.  Units of a modality whose bit in mods is clear are
// skipped: their columns keep their content.
__global__ __launch_bounds__(256) void k_pattern_expand_bwd(int B, int npat, PatternSet ps,
                                                            const float* __restrict__ dout, long long ld_dout,
                                                            float* __restrict__ demb, long long ld_demb, int mods) {
  const int u0 = ps.units[0], u01 = u0 + ps.units[1], upr = u01 + ps.units[2];
  const long long total = 2LL * B * upr;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int u = (int)(e % upr);
    const long long row = e / upr;  // half * B + b
    const int b = (int)(row % B), want = row < B ? 1 : 0;
    const int m = u < u0 ? 0 : (u < u01 ? 1 : 2);
    if (!((mods >> m) & 1)) continue;
    const int uu = u - (m == 0 ? 0 : (m == 1 ? u0 : u01));
    const float* s = dout + b * ld_dout + ps.col[m];
    float* d = demb + row * ld_demb + ps.col[m];
    if (ps.vec[m]) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int p = 0; p < npat; ++p) {
        if (((ps.keep[p] >> m) & 1) != want) continue;
        const float4 g = reinterpret_cast<const float4*>(s + (long long)p * B * ld_dout)[uu];
        acc.x += g.x;
        acc.y += g.y;
        acc.z += g.z;
        acc.w += g.w;
      }
      reinterpret_cast<float4*>(d)[uu] = acc;
    } else {
      float acc = 0.f;
      for (int p = 0; p < npat; ++p) {
        if (((ps.keep[p] >> m) & 1) != want) continue;
        acc += s[(long long)p * B * ld_dout + uu];
      }
      d[uu] = acc;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// The encoder half of the UTT-Fusion head stage read from a cache (tspm_utt_cache_rows): cache row i is
// [eA(i) | eV(i) | pooled(i)], `zero` the same for the zeroed inputs (one row, or one per sample).  Output row r < R =
// halves*B serves sample rows[r mod B]: a modality comes from emb when r < B and the row keeps it (row_keep NULL: every
// modality), else from zero.  A thread moves one float4: an audio / video unit to av_out, a pooled unit through the
// dropout of k_textcnn_pool's store (the same expression, so the same mask bytes give the same fc_in bits) to pool_out.
// The first unit of a row r < B carries the row's label.  Memory bound: no LDS, no atomics.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_utt_cache_rows(tspm_utt_cache_rows_desc d) {
  const int B = d.batch, R = d.halves * d.batch;
  const int uav = (d.w_audio + d.w_video) / 4, ua = d.w_audio / 4, upr = uav + d.w_pool / 4;
  const float4* __restrict__ emb = static_cast<const float4*>(static_cast<const void*>(d.emb));
  const float4* __restrict__ zero = static_cast<const float4*>(static_cast<const void*>(d.zero));
  const long long ldc = d.ld_cache / 4, total = (long long)R * upr;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int u = (int)(e % upr), r = (int)(e / upr);
    const int b = r % B;
    const long long s = d.rows[b];
    const bool valid = s >= 0 && s < d.n_rows;
    const int m = u < ua ? 0 : (u < uav ? 1 : 2);
    const bool real = r < B && (!d.row_keep || d.row_keep[3 * b + m] != 0);
    float4 v;
    if (!valid) {
      const float q = __builtin_nanf("");
      v = make_float4(q, q, q, q);
    } else {
      v = real ? emb[s * ldc + u] : zero[(d.n_zero == 1 ? 0 : s) * ldc + u];
    }
    if (m < 2) {
      reinterpret_cast<float4*>(d.av_out + (long long)r * d.ld_av)[u] = v;
    } else {
      const int j = (u - uav) * 4;
      if (d.keep) {
        const uchar4 k = *reinterpret_cast<const uchar4*>(d.keep + (long long)r * d.w_pool + j);
        const float sc = d.scale;
        v.x = v.x * (k.x ? sc : 0.f);
        v.y = v.y * (k.y ? sc : 0.f);
        v.z = v.z * (k.z ? sc : 0.f);
        v.w = v.w * (k.w ? sc : 0.f);
      }
      *reinterpret_cast<float4*>(d.pool_out + (long long)r * d.ld_pool + j) = v;
    }
    if (u == 0 && r < B && d.labels_out) {
      if (d.label_bytes == 8) {
        static_cast<long long*>(d.labels_out)[b] = valid ? static_cast<const long long*>(d.labels_all)[s] : -1LL;
      } else {
        static_cast<float*>(d.labels_out)[b] = valid ? static_cast<const float*>(d.labels_all)[s] : __builtin_nanf("");
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// LSTM host path: each of the nine entry points fills one LstmProb per descriptor, validates it against the entry
// point's rules and hands the problems to lstm_dispatch.
// ------------------------------------------------------------------------------------------------
constexpr int kLstmRB = 2;  // batch rows per workgroup (B = 128: 64 workgroups per LSTM)

// The widths of the recurrences: 4 <= H <= 128, a multiple of 4 (float4 rows of W_hh; one gate column per thread, at
// most 512 threads with W_hh's row in registers).  kind: 0 = the compile-time 64-wide kernels, else the tier.
bool lstm_width_ok(int H) { return H >= 4 && H <= 128 && (H & 3) == 0; }
int lstm_kind(int H) { return H == 64 ? 0 : H <= 32 ? 32 : H <= 64 ? 64 : 128; }

// One problem of a call: the descriptor (index pointer untyped), the hidden width, the lengths or null (which picks
// the Len kernels), and the width of the time index — 8 or 16 as the entry point (or a _len descriptor's index_bits)
// says, 0 for a _len problem without an index, which either instantiation serves.
template <typename Desc>
struct LstmProb {
  Desc d;
  int H, bits;
  const int32_t* lens;
};
using LstmFwdProb = LstmProb<LstmFwdDesc>;
using LstmBwdProb = LstmProb<LstmBwdDesc>;
using LstmBwdSeqProb = LstmProb<LstmBwdSeqDesc>;

// tspm_lstm_fwd_desc / _fwd_len_desc and the two backward descriptors agree on these fields.
template <typename S>
LstmFwdProb lstm_fwd_prob(const S& s, int bits, const int32_t* lens) {
  return {{s.batch, s.steps, s.xg, s.w_hh, s.b_hh, s.gates, s.cs, s.hs, s.h_out, s.ld_out, s.argmax}, s.hidden, bits, lens};
}
template <typename S>
LstmBwdProb lstm_bwd_prob(const S& s, int bits, const int32_t* lens) {
  return {{s.batch, s.steps, s.w_hh, s.gates, s.cs, s.dh, s.ld_dh, s.dgates, s.argmax}, s.hidden, bits, lens};
}

// What differs between the entry points: tspm_lstm_fwd / _bwd take width 64 only, the _len pair needs lengths.  The
// index width is in the problem (8: at most 256 steps with an index; 16: at most 65535, indices 0..65534, and a
// 2-byte aligned buffer); without an index steps is unlimited and bits is not looked at.
struct LstmRules {
  bool any_width, lens;
};

bool lstm_shape_ok(int B, int T, int H, int ld, const void* arg, int bits, const int32_t* lens, LstmRules r) {
  if (B <= 0 || T <= 0 || ld < H || (r.any_width ? !lstm_width_ok(H) : H != 64) || (r.lens && !lens)) return false;
  if (!arg) return true;
  if (bits == 8) return T <= 256;
  return bits == 16 && T <= 65535 && !(reinterpret_cast<uintptr_t>(arg) & 1);
}
bool lstm_valid(const LstmFwdProb& p, LstmRules r) {  // the forward reads W_hh's rows as float4
  const LstmFwdDesc& d = p.d;
  return lstm_shape_ok(d.B, d.T, p.H, d.ldh, d.arg, p.bits, p.lens, r) && d.xg && d.whh && d.gates && d.cs && d.hs &&
         d.hout && !(reinterpret_cast<uintptr_t>(d.whh) & 15);
}
bool lstm_valid(const LstmBwdProb& p, LstmRules r) {
  const LstmBwdDesc& d = p.d;
  return lstm_shape_ok(d.B, d.T, p.H, d.lddh, d.arg, p.bits, p.lens, r) && d.whh && d.gates && d.cs && d.dh && d.dgates;
}

bool lstm_valid(const LstmBwdSeqProb& p, LstmRules r) {  // dh or dseq (or both); no index
  const LstmBwdSeqDesc& d = p.d;
  return lstm_shape_ok(d.B, d.T, p.H, d.dh ? d.lddh : p.H, nullptr, 0, p.lens, r) && d.whh && d.gates && d.cs &&
         d.dgates && (d.dh || d.dseq);
}

// The one place that names the kernels: X is the kernel's pack of per-problem extras, A the arguments after d0.
template <int HP, typename Ix, typename... X, typename... A>
void lstm_kernel(dim3 grid, hipStream_t st, const LstmFwdDesc& d0, A... rest) {
  hipLaunchKernelGGL((k_lstm_fwd<HP, kLstmRB, Ix, X...>), grid, dim3(4 * HP), 0, st, d0, rest...);
}
template <int HP, typename Ix, typename... X, typename... A>
void lstm_kernel(dim3 grid, hipStream_t st, const LstmBwdDesc& d0, A... rest) {
  hipLaunchKernelGGL((k_lstm_bwd<HP, kLstmRB, Ix, X...>), grid, dim3(4 * HP), 0, st, d0, rest...);
}

template <int HP, typename Ix, typename... X, typename... A>
void lstm_kernel(dim3 grid, hipStream_t st, const LstmBwdSeqDesc& d0, A... rest) {
  if constexpr (kLstmLen<X...>)  // the per-step form exists with lengths only (and has no index: Ix is not used)
    hipLaunchKernelGGL((k_lstm_bwd_seq<HP, kLstmRB, X...>), grid, dim3(4 * HP), 0, st, d0, rest...);
}

template <int HP, bool Fixed, typename Ix, bool Len, typename Desc>
int lstm_launch(const LstmProb<Desc>& a, const LstmProb<Desc>* b, hipStream_t st) {
  const int na = cdiv(a.d.B, kLstmRB), nbb = b ? cdiv(b->d.B, kLstmRB) : 0;
  const dim3 grid(na + nbb);
  const LstmProb<Desc>& b_ = b ? *b : a;
  if constexpr (Fixed && !Len)
    lstm_kernel<HP, Ix>(grid, st, a.d, b_.d, na);
  else if constexpr (Fixed)
    lstm_kernel<HP, Ix, const int32_t*>(grid, st, a.d, a.lens, b_.d, b_.lens, na);
  else if constexpr (!Len)
    lstm_kernel<HP, Ix, int>(grid, st, a.d, a.H, b_.d, b_.H, na);
  else
    lstm_kernel<HP, Ix, int, const int32_t*>(grid, st, a.d, a.H, a.lens, b_.d, b_.H, b_.lens, na);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}

// One launch of one kernel kind (a's; b, if any, is of the same kind): width 64 on the compile-time kernels, every
// other width on its tier.
template <typename Ix, bool Len, typename Desc>
int lstm_launch_kind(const LstmProb<Desc>& a, const LstmProb<Desc>* b, hipStream_t st) {
  switch (lstm_kind(a.H)) {
    case 0: return lstm_launch<64, true, Ix, Len>(a, b, st);
    case 32: return lstm_launch<32, false, Ix, Len>(a, b, st);
    case 64: return lstm_launch<64, false, Ix, Len>(a, b, st);
    default: return lstm_launch<128, false, Ix, Len>(a, b, st);
  }
}

// Validated problems to launches.  Two problems share a launch when they are of one kernel kind and their index widths
// agree (a problem without an index width goes with either, and alone takes the 8-bit kernels); otherwise one launch
// each.  A workgroup's arithmetic does not depend on its neighbours, so either way the results are those of two
// count-1 calls.  All problems of a call have lengths or none has.
template <typename Desc>
int lstm_dispatch(int count, const LstmProb<Desc>* p, tspm_stream_t stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  auto run = [&](const LstmProb<Desc>& a, const LstmProb<Desc>* b) {
    const bool wide = (a.bits ? a.bits : (b ? b->bits : 0)) == 16;
    if (a.lens) return wide ? lstm_launch_kind<uint16_t, true>(a, b, st) : lstm_launch_kind<uint8_t, true>(a, b, st);
    return wide ? lstm_launch_kind<uint16_t, false>(a, b, st) : lstm_launch_kind<uint8_t, false>(a, b, st);
  };
  const bool together = count == 2 && lstm_kind(p[0].H) == lstm_kind(p[1].H) &&
                        (p[0].bits == p[1].bits || !p[0].bits || !p[1].bits);
  if (count == 1 || together) return run(p[0], count > 1 ? &p[1] : nullptr);
  const int rc = run(p[0], nullptr);
  return rc != TSPM_OK ? rc : run(p[1], nullptr);
}

// An entry point: every descriptor filled and validated before the first launch.
template <typename Desc, typename S, typename Fill>
int lstm_entry(int32_t count, const S* descs, tspm_stream_t stream, LstmRules rules, Fill fill) {
  if (count < 1 || count > 2 || !descs) return TSPM_ERR_INVALID;
  LstmProb<Desc> p[2];
  for (int i = 0; i < count; ++i) {
    p[i] = fill(descs[i]);
    if (!lstm_valid(p[i], rules)) return TSPM_ERR_INVALID;
  }
  return lstm_dispatch(count, p, stream);
}

constexpr LstmRules kRules64{false, false}, kRulesAnyWidth{true, false}, kRulesLen{true, true};

}  // namespace

extern "C" int tspm_lstm_fwd(int32_t count, const tspm_lstm_fwd_desc* descs, tspm_stream_t stream) {
  return lstm_entry<LstmFwdDesc>(count, descs, stream, kRules64,
                                 [](const tspm_lstm_fwd_desc& s) { return lstm_fwd_prob(s, 8, nullptr); });
}

extern "C" int tspm_lstm_bwd(int32_t count, const tspm_lstm_bwd_desc* descs, tspm_stream_t stream) {
  return lstm_entry<LstmBwdDesc>(count, descs, stream, kRules64,
                                 [](const tspm_lstm_bwd_desc& s) { return lstm_bwd_prob(s, 8, nullptr); });
}

extern "C" int tspm_lstm_fwd_w(int32_t count, const tspm_lstm_fwd_desc* descs, tspm_stream_t stream) {
  return lstm_entry<LstmFwdDesc>(count, descs, stream, kRulesAnyWidth,
                                 [](const tspm_lstm_fwd_desc& s) { return lstm_fwd_prob(s, 8, nullptr); });
}

extern "C" int tspm_lstm_bwd_w(int32_t count, const tspm_lstm_bwd_desc* descs, tspm_stream_t stream) {
  return lstm_entry<LstmBwdDesc>(count, descs, stream, kRulesAnyWidth,
                                 [](const tspm_lstm_bwd_desc& s) { return lstm_bwd_prob(s, 8, nullptr); });
}

// The same launches with a 16-bit time index: argmax points to uint16_t [batch][hidden], 1 <= steps <= 65535 with it.
extern "C" int tspm_lstm_fwd_t16(int32_t count, const tspm_lstm_fwd_desc* descs, tspm_stream_t stream) {
  return lstm_entry<LstmFwdDesc>(count, descs, stream, kRulesAnyWidth,
                                 [](const tspm_lstm_fwd_desc& s) { return lstm_fwd_prob(s, 16, nullptr); });
}

extern "C" int tspm_lstm_bwd_t16(int32_t count, const tspm_lstm_bwd_desc* descs, tspm_stream_t stream) {
  return lstm_entry<LstmBwdDesc>(count, descs, stream, kRulesAnyWidth,
                                 [](const tspm_lstm_bwd_desc& s) { return lstm_bwd_prob(s, 16, nullptr); });
}

// Per-sample lengths: each descriptor with its own `lengths` [batch] in device memory.  The host never reads them: a
// row's length is clamped to 1..steps in the kernel, so no value moves an access outside the buffers.
extern "C" int tspm_lstm_fwd_len(int32_t count, const tspm_lstm_fwd_len_desc* descs, tspm_stream_t stream) {
  return lstm_entry<LstmFwdDesc>(count, descs, stream, kRulesLen, [](const tspm_lstm_fwd_len_desc& s) {
    return lstm_fwd_prob(s, s.argmax ? s.index_bits : 0, s.lengths);
  });
}

extern "C" int tspm_lstm_bwd_len(int32_t count, const tspm_lstm_bwd_len_desc* descs, tspm_stream_t stream) {
  return lstm_entry<LstmBwdDesc>(count, descs, stream, kRulesLen, [](const tspm_lstm_bwd_len_desc& s) {
    return lstm_bwd_prob(s, s.argmax ? s.index_bits : 0, s.lengths);
  });
}

extern "C" int tspm_lstm_bwd_seq(int32_t count, const tspm_lstm_bwd_seq_desc* descs, tspm_stream_t stream) {
  return lstm_entry<LstmBwdSeqDesc>(count, descs, stream, kRulesLen, [](const tspm_lstm_bwd_seq_desc& s) {
    return LstmBwdSeqProb{{s.batch, s.steps, s.w_hh, s.gates, s.cs, s.dh, s.ld_dh, s.dgates, s.dseq, s.wt},
                          s.hidden, 0, s.lengths};
  });
}

namespace {
// One host path behind tspm_textcnn_pool_fwd and tspm_textcnn_pool_fwd_len (`lengths`: device memory, never read here).
int textcnn_pool_launch(int32_t batch, int32_t steps, int32_t nconv, const int32_t* heights, int32_t channels,
                        const float* const* conv_out, const float* const* bias, const uint8_t* keep, float keep_scale,
                        float* pooled, uint8_t* argmax, float* out, int32_t ld_out, const int32_t* lengths,
                        tspm_stream_t stream) {
  if (batch <= 0 || steps <= 0 || nconv < 1 || nconv > 4 || !heights || channels <= 0 || !conv_out || !pooled ||
      !argmax || !out || ld_out < nconv * channels || steps > 256)
    return TSPM_ERR_INVALID;
  PoolSet ps{};
  for (int i = 0; i < nconv; ++i) {
    if (heights[i] < 1 || heights[i] > steps || !conv_out[i]) return TSPM_ERR_INVALID;
    ps.y[i] = conv_out[i];
    ps.bias[i] = bias ? bias[i] : nullptr;
    ps.kh[i] = heights[i];
  }
  const dim3 grid(grid_for((long long)batch * nconv * channels));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (lengths)
    hipLaunchKernelGGL(k_textcnn_pool_len, grid, dim3(256), 0, st, batch, steps, nconv, channels, ps, keep, keep_scale,
                       pooled, argmax, out, ld_out, lengths);
  else
    hipLaunchKernelGGL(k_textcnn_pool, grid, dim3(256), 0, st, batch, steps, nconv, channels, ps, keep, keep_scale,
                       pooled, argmax, out, ld_out);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}
}  // namespace

extern "C" int tspm_textcnn_pool_fwd(int32_t batch, int32_t steps, int32_t nconv, const int32_t* heights,
                                     int32_t channels, const float* const* conv_out, const float* const* bias,
                                     const uint8_t* keep, float keep_scale, float* pooled, uint8_t* argmax,
                                     float* out, int32_t ld_out, tspm_stream_t stream) {
  return textcnn_pool_launch(batch, steps, nconv, heights, channels, conv_out, bias, keep, keep_scale, pooled, argmax,
                             out, ld_out, nullptr, stream);
}

// Per-sample text lengths: row b pools over its own max(L_b - kh_i + 1, 1) windows, L_b = lengths[b] clamped to
// 1..steps in the kernel.  The host checks `lengths` for non-NULL only: no value moves an access outside the buffers.
extern "C" int tspm_textcnn_pool_fwd_len(int32_t batch, int32_t steps, int32_t nconv, const int32_t* heights,
                                         int32_t channels, const float* const* conv_out, const float* const* bias,
                                         const uint8_t* keep, float keep_scale, float* pooled, uint8_t* argmax,
                                         float* out, int32_t ld_out, const int32_t* lengths, tspm_stream_t stream) {
  if (!lengths) return TSPM_ERR_INVALID;
  return textcnn_pool_launch(batch, steps, nconv, heights, channels, conv_out, bias, keep, keep_scale, pooled, argmax,
                             out, ld_out, lengths, stream);
}

extern "C" int tspm_textcnn_bwd(int32_t batch, int32_t steps, int32_t feat, int32_t nconv, const int32_t* heights,
                                int32_t channels, const float* x, const float* dout, int32_t ld_dout,
                                const uint8_t* keep, float keep_scale, const float* pooled, const uint8_t* argmax,
                                float* const* dw, float* const* db, float* g_work, tspm_stream_t stream) {
  if (batch <= 0 || steps <= 0 || feat <= 0 || feat > 1024 || nconv < 1 || nconv > 4 || !heights || channels <= 0 ||
      !x || !dout || !pooled || !argmax || !dw || !g_work || ld_dout < nconv * channels)
    return TSPM_ERR_INVALID;
  WgradSet ws{};
  for (int i = 0; i < nconv; ++i) {
    if (heights[i] < 1 || heights[i] > 5 || heights[i] > steps || !dw[i]) return TSPM_ERR_INVALID;
    ws.dw[i] = dw[i];
    ws.db[i] = db ? db[i] : nullptr;
    ws.kh[i] = heights[i];
  }
  const int nc = nconv * channels;
  const long long total = (long long)batch * nc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_textcnn_pool_grad, dim3(grid_for(total)), dim3(256), 0, st, total, nc, dout, ld_dout, keep,
                     keep_scale, pooled, g_work);
  TSPM_LAUNCH_CHECK();
  const bool slab = channels == kWgC && feat % kWgFB == 0 && steps <= 256 &&
                    (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  if (slab) {
    for (int i = 0; i < nconv; ++i)
      if (reinterpret_cast<uintptr_t>(dw[i]) & 15) return TSPM_ERR_INVALID;
    const int nfb = feat / kWgFB;
    hipLaunchKernelGGL((k_textcnn_wgrad_slab<5>), dim3(nconv * nfb), dim3(256), 0, st, batch, steps, feat, ws, x, g_work,
                       argmax, nc, nfb);
  } else {
    hipLaunchKernelGGL((k_textcnn_wgrad<5, 4>), dim3(nc), dim3(256), 0, st, batch, feat, channels, ws, x, g_work,
                       argmax, nc);
  }
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}

extern "C" size_t tspm_grad_clip_workspace(void) { return (size_t)kClipBlocks * sizeof(double); }

extern "C" int tspm_grad_clip_coef(int64_t count, const float* grad, float grad_scale, float max_norm, float* coef,
                                   float* total_norm, void* workspace, size_t workspace_bytes, tspm_stream_t stream) {
  if (count <= 0 || !grad || !coef || !(max_norm > 0.f)) return TSPM_ERR_INVALID;
  if (!workspace || workspace_bytes < tspm_grad_clip_workspace()) return TSPM_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* part = static_cast<double*>(workspace);
  hipLaunchKernelGGL(k_sumsq, dim3(kClipBlocks), dim3(256), 0, st, (long long)count, grad, grad_scale, part);
  TSPM_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_clip_coef, dim3(1), dim3(256), 0, st, kClipBlocks, part, max_norm, coef, total_norm);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}

extern "C" int tspm_grad_clip_coef_multi(int32_t count, const tspm_grad_range* ranges, float grad_scale, float max_norm,
                                         float* coef, float* total_norm, void* workspace, size_t workspace_bytes,
                                         tspm_stream_t stream) {
  if (count < 1 || count > TSPM_ADAM_MAX_SEGMENTS || !ranges || !coef || !(max_norm > 0.f)) return TSPM_ERR_INVALID;
  int nonempty = 0;
  unsigned long long total = 0;
  for (int r = 0; r < count; ++r) {
    if (ranges[r].count < 0 || (ranges[r].count > 0 && !ranges[r].grad)) return TSPM_ERR_INVALID;
    if (ranges[r].count > 0) { ++nonempty; total += (unsigned long long)ranges[r].count; }
  }
  if (nonempty == 0) return TSPM_ERR_INVALID;
  if (!workspace || workspace_bytes < tspm_grad_clip_workspace()) return TSPM_ERR_WORKSPACE;
  // the partition, from the counts alone: one workgroup per non-empty range, the rest in proportion (rounded down)
  GradRanges a{};
  a.nrange = count;
  int at = 0;
  for (int r = 0; r < count; ++r) {
    a.g[r] = ranges[r].grad;
    a.count[r] = ranges[r].count;
    a.first[r] = at;
    if (ranges[r].count > 0)  // exact: the shares sum to at most kClipBlocks - nonempty
      at += 1 + (int)((unsigned __int128)(kClipBlocks - nonempty) * (unsigned long long)ranges[r].count / total);
  }
  for (int r = count; r <= TSPM_ADAM_MAX_SEGMENTS; ++r) a.first[r] = at;
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* part = static_cast<double*>(workspace);
  hipLaunchKernelGGL(k_sumsq_multi, dim3(kClipBlocks), dim3(256), 0, st, a, grad_scale, part);
  TSPM_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_clip_coef, dim3(1), dim3(256), 0, st, kClipBlocks, part, max_norm, coef, total_norm);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}

extern "C" int tspm_seq_gather(int32_t count, const int64_t* index, int64_t n_samples, const float* data,
                               const int64_t* offsets, const int32_t* lengths, int32_t feat, int32_t steps_pad,
                               float* out, int64_t stride_t, int64_t stride_b, const float* row_mask,
                               const int64_t* labels, int64_t* labels_out, tspm_stream_t stream) {
  if (count <= 0 || !index || n_samples <= 0 || !data || !offsets || !lengths || feat <= 0 || steps_pad <= 0 || !out)
    return TSPM_ERR_INVALID;
  if ((labels == nullptr) != (labels_out == nullptr)) return TSPM_ERR_INVALID;
  hipLaunchKernelGGL(k_seq_gather, dim3(grid_for((long long)steps_pad * count * feat)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), count, index, (long long)n_samples, data, offsets, lengths, feat,
                     steps_pad, out, (long long)stride_t, (long long)stride_b, row_mask, labels, labels_out);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}

// Fills ps from the host tables (group_id may be null) and picks each modality's unit: a float4 where strides4 holds
// (both row strides multiples of 4), both bases are 16-byte aligned and the width and column offset are multiples of 4.
// False for a pattern that keeps nothing.
static bool pattern_set_fill(PatternSet& ps, int npat, const int32_t* keep, const int32_t* group_id, int w_audio,
                             int w_video, int w_text, bool strides4, const void* base_a, const void* base_b) {
  for (int p = 0; p < npat; ++p) {
    const int bits = (keep[3 * p] ? 1 : 0) | (keep[3 * p + 1] ? 2 : 0) | (keep[3 * p + 2] ? 4 : 0);
    if (bits == 0) return false;  // a pattern keeps at least one modality
    ps.keep[p] = bits;
    ps.group[p] = group_id ? group_id[p] : 0;
  }
  const int w[3] = {w_audio, w_video, w_text};
  const bool wide_ok =
      strides4 && ((reinterpret_cast<uintptr_t>(base_a) | reinterpret_cast<uintptr_t>(base_b)) & 15) == 0;
  int col = 0;
  for (int m = 0; m < 3; ++m) {
    ps.width[m] = w[m];
    ps.col[m] = col;
    ps.vec[m] = (wide_ok && w[m] % 4 == 0 && col % 4 == 0) ? 1 : 0;
    ps.units[m] = ps.vec[m] ? w[m] / 4 : w[m];
    col += w[m];
  }
  return true;
}

extern "C" int tspm_pattern_expand(int32_t batch, int32_t npat, const int32_t* keep, const int32_t* group_id,
                                   int32_t w_audio, int32_t w_video, int32_t w_text, const float* emb, int64_t ld_emb,
                                   float* out, int64_t ld_out, const void* labels, void* labels_out,
                                   int32_t label_bytes, int32_t* groups_out, tspm_stream_t stream) {
  if (batch <= 0 || npat < 1 || npat > TSPM_MAX_PATTERNS || w_audio <= 0 || w_video <= 0 || w_text <= 0)
    return TSPM_ERR_INVALID;
  if (!keep || !group_id || !emb || !out || !labels || !labels_out || !groups_out) return TSPM_ERR_INVALID;
  if (label_bytes != 4 && label_bytes != 8) return TSPM_ERR_INVALID;
  const long long sum = (long long)w_audio + w_video + w_text;
  if (ld_emb < sum || ld_out < sum || sum > INT32_MAX / 2) return TSPM_ERR_INVALID;
  PatternSet ps{};
  if (!pattern_set_fill(ps, npat, keep, group_id, w_audio, w_video, w_text, ld_emb % 4 == 0 && ld_out % 4 == 0, emb, out))
    return TSPM_ERR_INVALID;
  const long long upr = (long long)ps.units[0] + ps.units[1] + ps.units[2];
  hipLaunchKernelGGL(k_pattern_expand, dim3(grid_for((long long)npat * batch * upr)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), batch, npat, ps, emb, (long long)ld_emb, out, (long long)ld_out,
                     labels, labels_out, label_bytes, groups_out);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}

extern "C" int tspm_pattern_expand_bwd(int32_t batch, int32_t npat, const int32_t* keep, int32_t w_audio,
                                       int32_t w_video, int32_t w_text, const float* dout, int64_t ld_dout,
                                       float* demb, int64_t ld_demb, int32_t modalities, tspm_stream_t stream) {
  if (batch <= 0 || npat < 1 || npat > TSPM_MAX_PATTERNS || w_audio <= 0 || w_video <= 0 || w_text <= 0)
    return TSPM_ERR_INVALID;
  if (!keep || !dout || !demb || modalities < 1 || modalities > 7) return TSPM_ERR_INVALID;
  const long long sum = (long long)w_audio + w_video + w_text;
  if (ld_dout < sum || ld_demb < sum || sum > INT32_MAX / 2) return TSPM_ERR_INVALID;
  PatternSet ps{};
  if (!pattern_set_fill(ps, npat, keep, nullptr, w_audio, w_video, w_text, ld_dout % 4 == 0 && ld_demb % 4 == 0, dout,
                        demb))
    return TSPM_ERR_INVALID;
  const long long upr = (long long)ps.units[0] + ps.units[1] + ps.units[2];
  hipLaunchKernelGGL(k_pattern_expand_bwd, dim3(grid_for(2LL * batch * upr)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), batch, npat, ps, dout, (long long)ld_dout, demb,
                     (long long)ld_demb, modalities);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}

extern "C" int tspm_utt_cache_rows(const tspm_utt_cache_rows_desc* desc, tspm_stream_t stream) {
  if (!desc) return TSPM_ERR_INVALID;
  const tspm_utt_cache_rows_desc& d = *desc;
  if (d.batch < 1 || d.n_rows < 1 || (d.halves != 1 && d.halves != 2)) return TSPM_ERR_INVALID;
  if (!d.emb || !d.zero || !d.rows || !d.av_out || !d.pool_out) return TSPM_ERR_INVALID;
  const int dims[6] = {d.w_audio, d.w_video, d.w_pool, d.ld_cache, d.ld_av, d.ld_pool};
  for (int v : dims)
    if (v < 4 || v % 4 != 0) return TSPM_ERR_INVALID;
  const long long wav = (long long)d.w_audio + d.w_video;
  if (d.ld_cache < wav + d.w_pool || d.ld_av < wav || d.ld_pool < d.w_pool) return TSPM_ERR_INVALID;
  const void* aligned[5] = {d.emb, d.zero, d.av_out, d.pool_out, d.keep};
  for (const void* p : aligned)
    if (reinterpret_cast<uintptr_t>(p) & 15) return TSPM_ERR_INVALID;
  if (d.row_keep && d.halves == 2) return TSPM_ERR_INVALID;
  if (d.n_zero != 1 && d.n_zero != d.n_rows) return TSPM_ERR_INVALID;
  if ((d.labels_all == nullptr) != (d.labels_out == nullptr)) return TSPM_ERR_INVALID;
  if (d.label_bytes != 4 && d.label_bytes != 8) return TSPM_ERR_INVALID;
  if ((long long)d.halves * d.batch > INT32_MAX) return TSPM_ERR_INVALID;
  const long long units = (long long)d.halves * d.batch * ((wav + d.w_pool) / 4);
  hipLaunchKernelGGL(k_utt_cache_rows, dim3(grid_for(units)), dim3(256), 0, static_cast<hipStream_t>(stream), d);
  TSPM_LAUNCH_CHECK();
  return TSPM_OK;
}
