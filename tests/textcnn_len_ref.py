"""The TextCNN forward with per-sample text lengths, restated for the tests (``text_lengths`` /
``tspm_textcnn_pool_fwd_len``): per row b and conv i of height kh_i the row's own first L_b steps, zero-padded to
max(L_b, kh_i), then conv, ReLU and the first maximum over time — the row has n_i(b) = max(L_b - kh_i + 1, 1) windows.
L_b is the given length clamped to 1..steps.  Differentiable, any dtype; with a ``MosiTrace`` it records and forces the
time index as ``MosiTrace.time_max`` does (sites ``text.pool{i}`` / ``text.relu{i}``; the recorded pre-activation is
[B, C, Tout] with -inf at the windows a row does not have, so no comparison can pick one).

test_mosi_text_lengths_cpu.py holds it to oracle.mosi_ref.textcnn_forward run on each row alone.
"""
import torch
import torch.nn.functional as F


def clamp_len(length: int, steps: int) -> int:
    return min(max(int(length), 1), int(steps))


def n_windows(length: int, kh: int, steps: int) -> int:
    return max(clamp_len(length, steps) - kh + 1, 1)


def own_row(x_row: torch.Tensor, length: int, kh: int) -> torch.Tensor:
    """x_row [steps, F] -> the row's first L_b steps zero-padded to max(L_b, kh)."""
    lb = clamp_len(length, x_row.shape[0])
    row = x_row[:lb]
    if lb < kh:
        row = torch.cat([row, row.new_zeros(kh - lb, row.shape[1])], 0)
    return row


def pooled_len(net, x: torch.Tensor, lengths, trace=None) -> torch.Tensor:
    """The pooled features [B, 3C] (before the dropout) of x [B, steps, F] under ``lengths`` (a sequence of B ints)."""
    b, steps, f = x.shape
    outs = []
    for i, conv in enumerate((net.conv1, net.conv2, net.conv3)):
        kh = conv.weight.shape[2]
        ys = [F.conv2d(own_row(x[r], lengths[r], kh).view(1, 1, -1, f), conv.weight, conv.bias)[0, :, :, 0]
              for r in range(b)]  # per row [C, n_i(b)]
        if trace is None:
            outs.append(torch.stack([F.relu(y).max(1).values for y in ys]))
            continue
        site_p, site_r = f"text.pool{i}", f"text.relu{i}"
        pre = x.new_full((b, conv.weight.shape[0], steps - kh + 1), float("-inf"))
        idx = []
        for r, y in enumerate(ys):
            pre[r, :, :y.shape[1]] = y.detach()
            act = F.relu(y).unsqueeze(0)
            idx.append(F.max_pool1d(act, act.size(2), return_indices=True)[1][0, :, 0])  # the first maximum
        trace.pre[site_p], trace.idx[site_p] = pre, torch.stack(idx)
        if trace.force is None or site_p not in trace.force:
            outs.append(torch.stack([F.relu(y).gather(1, k.unsqueeze(1)).squeeze(1) for y, k in zip(ys, idx)]))
            continue
        forced = trace.force[site_p].to(x.device)
        assert all(int(forced[r].max()) < ys[r].shape[1] for r in range(b)), "a forced index outside the row's windows"
        at = torch.stack([y.gather(1, forced[r].unsqueeze(1)).squeeze(1) for r, y in enumerate(ys)])
        trace.pre[site_r] = at.detach()
        outs.append(at * trace.force[site_r].to(device=at.device, dtype=at.dtype))
    return torch.cat(outs, 1)


def textcnn_forward_len(net, x, training, keep, trace=None, lengths=None):
    """oracle.mosi_ref.textcnn_forward with ``lengths`` (None: every row at the full length)."""
    lengths = [x.shape[1]] * x.shape[0] if lengths is None else lengths
    h = pooled_len(net, x, lengths, trace)
    if training and net.p > 0:
        h = h * (keep.to(h.dtype) / (1.0 - net.p)) if keep is not None else F.dropout(h, net.p, True)
    z = F.linear(h, net.embd[0].weight, net.embd[0].bias)
    return F.relu(z) if trace is None else trace.relu("text.embd", z)


class TextLenOracle:
    """Replacement of oracle.mosi_ref.textcnn_forward (monkeypatched in): the restatement under a fixed length vector."""

    def __init__(self, lengths):
        self.lengths = lengths

    def __call__(self, net, x, training, keep, trace=None):
        return textcnn_forward_len(net, x, training, keep, trace, self.lengths)
