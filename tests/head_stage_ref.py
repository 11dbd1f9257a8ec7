"""Plain-torch restatement of the AVMNIST head stage over every missing-modality pattern of a batch: the chain
``tspm_pattern_expand`` -> ``tspm_head_train_step`` with ``n = P*B`` (what ``tspm_pattern_head_train_step`` must equal
up to summation order), run in any dtype through autograd on the REPLICATED batch, and the folding identity the kernel
uses for fc0's weight gradient, restated on the dz0 rows.  Shared by test_head_stage_cpu.py (the identity, in fp64) and
the GPU tests (fp64 truth and the fp32 yardstick)."""
from typing import Dict, Optional, Sequence, Tuple

import torch

KEEP = {"a": (1, 0), "ai": (1, 1), "i": (0, 1)}


def keep_of(patterns: Sequence[str]) -> Tuple[Tuple[int, int], ...]:
    return tuple(KEEP[p] for p in patterns)


def make_head(F: int, H: int, H2: int, C: int, seed: int) -> Dict[str, torch.Tensor]:
    """nn.Linear-scaled weights of the three Linears (fp32, CPU)."""
    g = torch.Generator().manual_seed(seed)

    def lin(o, i):
        b = 1.0 / i ** 0.5
        return (torch.rand(o, i, generator=g) * 2 - 1) * b, (torch.rand(o, generator=g) * 2 - 1) * b
    w0, b0 = lin(H, F)
    w3, b3 = lin(H2, H)
    w5, b5 = lin(C, H2)
    return {"w0": w0, "b0": b0, "w3": w3, "b3": b3, "w5": w5, "b5": b5}


def expand(x: torch.Tensor, x0: torch.Tensor, keep, w_audio: int) -> torch.Tensor:
    """[P*B, F]: row p*B + b holds x[b]'s columns per kept modality, else x0's."""
    rows = []
    for ka, ki in keep:
        r = x.clone()
        if not ka:
            r[:, :w_audio] = x0[:w_audio]
        if not ki:
            r[:, w_audio:] = x0[w_audio:]
        rows.append(r)
    return torch.cat(rows, 0)


def chain(x, x0, keep, w_audio: int, W: Dict[str, torch.Tensor], labels, loss_weight: float = 1.0, p: float = 0.0,
          mask: Optional[torch.Tensor] = None, dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """Forward, weighted mean cross-entropy over ALL P*B rows and autograd's gradients of the six head parameters.
    ``mask`` [P*B, H] (uint8 keep mask) with ``p > 0``: h1 = relu(.) * mask / (1 - p)."""
    P = len(keep)
    Wd = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in W.items()}
    X = expand(x.to(dtype), x0.to(dtype), keep, w_audio)
    z0 = X @ Wd["w0"].T + Wd["b0"]
    z0.retain_grad()
    h1 = torch.relu(z0)
    if p > 0:
        h1 = h1 * (mask.to(dtype) * (1.0 / (1.0 - p)))
    hh = torch.relu(h1 @ Wd["w3"].T + Wd["b3"])
    logits = hh @ Wd["w5"].T + Wd["b5"]
    lab = labels.repeat(P)
    ce = torch.nn.functional.cross_entropy(logits, lab, reduction="none")
    loss = loss_weight * ce.mean()
    loss.backward()
    out = {"logits": logits.detach(), "loss": loss.detach(), "ce_sum": ce.detach().sum(),
           "correct": (logits.detach().argmax(1) == lab).sum(), "dz0": z0.grad.detach(), "X": X.detach()}
    for k in W:
        out["g" + k] = Wd[k].grad.detach()
    return out


def folded_fc0_grads(dz0: torch.Tensor, x: torch.Tensor, x0: torch.Tensor, keep, w_audio: int):
    """gw0 / gb0 from the dz0 rows by the kernel's algebra — K is B, not P*B.  For modality m with columns cols_m:
        fold_m[b] = sum over the p that keep m of dz0[p*B + b]
        zsum_m    = sum over the p that drop m and every b of dz0[p*B + b]
        gw0[:, cols_m] = sum_b fold_m[b]^T (x) x[b, cols_m] + zsum_m^T (x) x0[cols_m]
        gb0 = sum_b fold_m[b] + zsum_m   (either m)"""
    P, B = len(keep), x.shape[0]
    H, F = dz0.shape[1], x.shape[1]
    d = dz0.view(P, B, H)
    gw0 = torch.zeros(H, F, dtype=dz0.dtype)
    gb0 = []
    for m, cols in enumerate((slice(0, w_audio), slice(w_audio, F))):
        fold = torch.zeros(B, H, dtype=dz0.dtype)
        zsum = torch.zeros(H, dtype=dz0.dtype)
        for p in range(P):
            if keep[p][m]:
                fold = fold + d[p]
            else:
                zsum = zsum + d[p].sum(0)
        gw0[:, cols] = fold.T @ x[:, cols].to(dz0.dtype) + torch.outer(zsum, x0[cols].to(dz0.dtype))
        gb0.append(fold.sum(0) + zsum)
    return gw0, gb0[0], gb0[1]


def inputs(B: int, F: int, C: int, seed: int):
    """x [B, F], x0 [F] (fp32, CPU) and labels [B]."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, F, generator=g)
    x0 = torch.randn(F, generator=g)
    labels = torch.randint(0, C, (B,), generator=g)
    return x, x0, labels
