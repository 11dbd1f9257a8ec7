"""The attention embedding of ``LSTMEncoder(embd_method="attention", attention_norm=...)``, restated for the tests in
plain torch (differentiable, any dtype; run in float32 and float64, gradients by autograd).  This file is the definition
the kernels are held to — the reference's lstm.py is not available to the tests:

    row b, L = L_b = min(max(lengths[b], 1), T) (T without lengths), r_t = the LSTM output at step t
    p_t = W r_t + c      z_t = tanh(p_t)      s_t = z_t . u                                   (t < L)
    "time": alpha_t = exp(s_t - max) / sum_{tau < L} exp(s_tau - max)        "unit": alpha_t = 1
    alpha_t = 0 for t >= L            e = sum_{t < L} alpha_t r_t

``attn_pool`` is the pooling alone on a time-major r [T, B, H] (what tspm_attn_pool_fwd computes); ``AttnEncoderRef`` is
the plain-torch module with the reference's attribute names and construction order; ``encode`` runs such a module (or
any module with the same attributes) on a batch-first input with lengths.  test_mosi_attention_cpu.py holds ``encode`` to
an independent composition (nn.LSTM over pack_padded_sequence, nn.Linear, tanh, softmax over the valid steps) in float64.
"""
import torch
import torch.nn as nn

NORMS = ("time", "unit")


def clamp_lengths(lengths, T):
    return [min(max(int(v), 1), int(T)) for v in lengths]


def attn_pool(r, W, c, u, lengths, norm, p=None):
    """r [T, B, H] time-major, W [H, H], c [H], u [H] (or [H, 1]) -> (e [B, H], alpha [T, B], z [T, B, H]); z is zero
    past a row's length (the kernel leaves those rows unwritten).  ``p`` [T, B, H]: the pre-activation given instead of
    W r + c (the op-level tests hand the kernel and this function the same one)."""
    assert norm in NORMS
    T, B, H = r.shape
    lens = clamp_lengths(lengths, T) if lengths is not None else [T] * B
    u = u.reshape(-1)
    es, alphas, zs = [], [], []
    for b in range(B):
        Lb = lens[b]
        rb = r[:Lb, b]                                     # [L, H]
        z = torch.tanh(rb @ W.T + c if p is None else p[:Lb, b])
        if norm == "time":
            s = z @ u
            ex = torch.exp(s - s.max())
            a = ex / ex.sum()
        else:  # the softmax over a trailing axis of size 1, literally: every weight 1, zero gradient to the scores
            a = torch.softmax((z @ u).unsqueeze(1), dim=-1).squeeze(1)
        es.append((a.unsqueeze(1) * rb).sum(0))
        alphas.append(torch.cat([a, a.new_zeros(T - Lb)]))
        zs.append(torch.cat([z, z.new_zeros(T - Lb, H)]))
    return torch.stack(es), torch.stack(alphas, 1), torch.stack(zs, 1)


class AttnEncoderRef(nn.Module):
    """The reference's construction restated: ``rnn``, then for "attention" ``attention_vector_weight`` =
    Parameter(Tensor(H, 1)), ``attention_layer`` = Sequential(Linear(H, H), Tanh()), ``softmax`` = Softmax(dim=-1).  The
    vector is left as allocated (the reference never initialises it): the tests fill or load it."""

    def __init__(self, input_size, hidden_size, embd_method="attention", attention_norm=None):
        super().__init__()
        self.attention_norm = attention_norm
        self.input_size, self.hidden_size = input_size, hidden_size
        self.rnn = nn.LSTM(input_size, hidden_size, batch_first=True)
        if embd_method == "attention":
            self.attention_vector_weight = nn.Parameter(torch.zeros(hidden_size, 1))
            self.attention_layer = nn.Sequential(nn.Linear(hidden_size, hidden_size), nn.Tanh())
            self.softmax = nn.Softmax(dim=-1)
        self.embd_method = embd_method


def lstm_outputs(rnn, x, lengths=None):
    """r_out [B, T, H] of nn.LSTM(batch_first) with each row run over its own first L_b steps (zeros after): a per-row
    loop over the unpadded row — ``pack_padded_sequence`` semantics without packing."""
    B, T, _ = x.shape
    lens = clamp_lengths(lengths, T) if lengths is not None else [T] * B
    rows = []
    for b in range(B):
        out, _ = rnn(x[b:b + 1, :lens[b]])
        rows.append(torch.cat([out[0], out.new_zeros(T - lens[b], out.shape[2])]))
    return torch.stack(rows)


def encode(enc, x, lengths=None, norm=None):
    """The embedding [B, H] of x [B, T, F] under a module with ``rnn`` / ``attention_layer`` / ``attention_vector_weight``
    (AttnEncoderRef, or a copy of the package's LSTMEncoder on the CPU); ``norm``: default the module's
    ``attention_norm``."""
    norm = enc.attention_norm if norm is None else norm
    r = lstm_outputs(enc.rnn, x, lengths).transpose(0, 1)  # [T, B, H]
    lin = enc.attention_layer[0]
    return attn_pool(r, lin.weight, lin.bias, enc.attention_vector_weight, lengths, norm)[0]


class AttnOracle:
    """Replacement of oracle.mosi_ref.lstm_forward (monkeypatched in): an "attention" encoder through ``encode`` under a
    fixed length dict {"audio": [...], "video": [...]} (a missing name: the padded length), any other encoder through
    ``other`` (the oracle's own function, or the length-aware one of test_gpu_mosi_lengths)."""

    def __init__(self, other, lengths=None):
        self.other, self.lengths = other, lengths or {}

    def __call__(self, enc, x, trace=None, site="lstm"):
        if getattr(enc, "embd_method", None) != "attention":
            return self.other(enc, x, trace, site)
        return encode(enc, x, self.lengths.get("audio" if ".a." in site else "video"))
