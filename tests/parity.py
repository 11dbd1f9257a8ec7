"""Model-level parity criterion shared by the GPU tests.

Ground truth is the CPU oracle run in fp64 with the HIP step's own ReLU masks and max-pool argmax
indices FORCED into it (oracle.avmnist_ref.MaskTrace).  Every output / gradient is then held to the
§8(c) bounds with no relaxed branch:

* logits and loss: rel-L2 <= 1e-4 against fp64;
* every parameter gradient and BN running statistic: rel-L2 <= 1e-3 and cosine >= 0.9999 against
  fp64, and in addition within 4x the error the fp32 reference makes on the same forced decisions
  (+2e-6 / 2e-5 floors) — the tighter of the two is what catches a kernel regression.

Forcing is what makes the bound honest at batch 128: an element whose pre-activation sits within
rounding of zero (or a max-pool window with a near-tie) is decided differently by ANY two fp32
implementations, and one such flip moves every upstream gradient by ~1e-3.  Each forced decision
that differs from fp64's own is a *flip*; the tests must show every flip is such a near-tie
(|pre-activation| <= NEAR x rms of its tensor, or pool candidates within NEAR x rms of each other)
and that flips are rare (``MAX_FLIP_FRAC`` of the decisions).  The counts are logged and asserted.
"""
from __future__ import annotations

import copy
from typing import Dict, Optional, Tuple

import torch

from oracle import avmnist_ref as orc

LOGITS_REL = 1e-4     # §8(c) end-to-end logits
GRAD_REL = 1e-3       # §8(c) gradients
GRAD_COS = 0.9999     # §8(c) gradients
FACTOR = 4.0          # vs the fp32 reference on the same forced decisions
FLOOR_OUT = 2e-6
FLOOR_GRAD = 2e-5
NEAR = 1e-4           # a flip must sit within NEAR x rms(tensor) of the threshold / of the tie
MAX_FLIP_FRAC = 1e-4  # at most this fraction of the decisions of one site may flip


def rel_l2(a, b) -> float:
    a = torch.as_tensor(a).detach().double().cpu().reshape(-1)
    b = torch.as_tensor(b).detach().double().cpu().reshape(-1)
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def cosine(a, b) -> float:
    a = torch.as_tensor(a).detach().double().cpu().reshape(-1)
    b = torch.as_tensor(b).detach().double().cpu().reshape(-1)
    if a.norm() == 0 and b.norm() == 0:
        return 1.0
    return (a @ b / (a.norm() * b.norm()).clamp_min(1e-300)).item()


# ------------------------------------------------------------------------------------------------
# The HIP step's decisions, in the oracle's NCHW layout
# ------------------------------------------------------------------------------------------------
def _hwnc_to_nchw(t: torch.Tensor, h: int, w: int, n: int) -> torch.Tensor:
    c = t.numel() // (h * w * n)
    return t.detach().reshape(h, w, n, c).permute(2, 3, 0, 1).cpu()


def engine_decisions(eng, prefix: str) -> Dict[str, torch.Tensor]:
    """ReLU masks (bool) and max-pool flat argmax (int64, torch's return_indices convention) of the
    last training forward of an ``engine.EncoderEngine``: stem = a0 > 0, mp from mp_idx (window tap
    kh*3+kw), blk{i}.a1 / blk{i}.out from the post-ReLU buffers."""
    n = eng.N
    p1, q1, p2, q2 = eng.mp_shape
    out = {prefix + "stem": _hwnc_to_nchw(eng.a0, p1, q1, n) > 0}
    tap = _hwnc_to_nchw(eng.mp_idx, p2, q2, n).long()
    kh, kw = tap // 3, tap % 3
    pp = torch.arange(p2).view(1, 1, p2, 1)
    qq = torch.arange(q2).view(1, 1, 1, q2)
    hh, ww = pp * 2 - 1 + kh, qq * 2 - 1 + kw
    if not ((hh >= 0) & (hh < p1) & (ww >= 0) & (ww < q1)).all():
        raise AssertionError("max-pool index outside its window")
    out[prefix + "mp"] = hh * q1 + ww
    for i, bp in enumerate(eng.blocks):
        s = bp.conv1.shape
        out[f"{prefix}blk{i}.a1"] = _hwnc_to_nchw(bp.a1, s.p, s.q, n) > 0
        out[f"{prefix}blk{i}.out"] = _hwnc_to_nchw(bp.out, s.p, s.q, n) > 0
    return out


def head_decisions(h1: torch.Tensor, hh: torch.Tensor) -> Dict[str, torch.Tensor]:
    """Fusion-head ReLU masks from the head's saved activations (h1 already carries the dropout
    keep-mask: dropped units are 0 there, and their decision is irrelevant — gradient 0 either way)."""
    return {"head.h1": h1.detach().cpu() > 0, "head.hh": hh.detach().cpu() > 0}


def step_decisions(step) -> Dict[str, torch.Tensor]:
    d = engine_decisions(step.eng_a, "audio.")
    d.update(engine_decisions(step.eng_i, "image."))
    d.update(head_decisions(step.h1, step.hh))
    return d


# ------------------------------------------------------------------------------------------------
# Flips: forced decisions that differ from fp64's own, each proven to be a near-tie
# ------------------------------------------------------------------------------------------------
def flip_report(trace64: "orc.MaskTrace", forced: Dict[str, torch.Tensor],
                keep: Optional[torch.Tensor] = None) -> Dict[str, Tuple[int, int, float]]:
    """site -> (flips, decisions, worst |distance to the threshold or tie| / rms).  Asserts that every
    flip is a near-tie and that flips are rare."""
    rep = {}
    for site, f in forced.items():
        x = trace64.pre[site].detach().cpu()
        rms = x.double().pow(2).mean().sqrt().item() or 1.0
        if f.dtype == torch.bool:
            nat = x > 0
            flip = f != nat
            if site == "head.h1" and keep is not None:  # dropped units: decision irrelevant
                flip &= keep.detach().cpu().reshape(flip.shape).bool()
            dist = x.double().abs()[flip]
            n_dec = f.numel()
        else:
            nat = trace64.idx[site].cpu()
            flip = f != nat
            flat = x.double().flatten(2)
            v_ours = flat.gather(2, f.flatten(2)).reshape(f.shape)
            v_nat = flat.gather(2, nat.flatten(2)).reshape(f.shape)
            dist = (v_ours - v_nat).abs()[flip]
            n_dec = f.numel()
        nf = int(flip.sum())
        worst = (dist.max().item() / rms) if nf else 0.0
        rep[site] = (nf, n_dec, worst)
        assert worst <= NEAR, f"{site}: a flipped decision is {worst:.2e} x rms from its threshold/tie (> {NEAR})"
        assert nf <= max(1, MAX_FLIP_FRAC * n_dec), f"{site}: {nf} of {n_dec} decisions flipped"
    return rep


def flips_summary(rep) -> str:
    tot = sum(v[0] for v in rep.values())
    sites = {k: v for k, v in rep.items() if v[0]}
    return f"{tot} flips " + ", ".join(f"{k}:{v[0]}({v[2]:.1e})" for k, v in sites.items())


# ------------------------------------------------------------------------------------------------
# Comparisons (no relaxed branch)
# ------------------------------------------------------------------------------------------------
class Tally:
    """Counts the comparisons made and the worst ratios seen (printed by the tests)."""

    def __init__(self):
        self.n = 0
        self.worst_rel = 0.0
        self.worst_name = ""

    def note(self, name, e):
        self.n += 1
        if e > self.worst_rel:
            self.worst_rel, self.worst_name = e, name

    def __str__(self):
        return f"{self.n} tensors compared, worst rel-L2 {self.worst_rel:.2e} ({self.worst_name})"


def check_out(name, ours, ref32, ref64, tally: Optional[Tally] = None, bound: float = LOGITS_REL):
    e_ours = rel_l2(ours, ref64)
    e_ref = rel_l2(ref32, ref64) if ref32 is not None else 0.0
    assert e_ours <= bound, f"{name}: rel-L2 {e_ours:.3e} > {bound:g} (fp64 truth)"
    if ref32 is not None:
        assert e_ours <= FACTOR * e_ref + FLOOR_OUT, f"{name}: ours {e_ours:.3e} vs fp32 reference {e_ref:.3e}"
    if tally is not None:
        tally.note(name, e_ours)
    return e_ours


def check_grad(name, ours, ref32, ref64, tally: Optional[Tally] = None):
    e_ours = rel_l2(ours, ref64)
    cos = cosine(ours, ref64)
    assert e_ours <= GRAD_REL and cos >= GRAD_COS, f"{name}: rel-L2 {e_ours:.3e}, cosine {cos:.7f} (fp64 truth)"
    if ref32 is not None:
        e_ref = rel_l2(ref32, ref64)
        assert e_ours <= FACTOR * e_ref + FLOOR_GRAD, f"{name}: ours {e_ours:.3e} vs fp32 reference {e_ref:.3e}"
    if tally is not None:
        tally.note(name, e_ours)
    return e_ours


def adam_fp64(p0, g, step, lr=5e-4, wd=1e-4, b1=0.9, b2=0.999, eps=1e-8, m=None, v=None):
    """torch.optim.Adam's single-tensor update in fp64 (L2 weight decay folded into the gradient)."""
    p0, g = p0.double(), g.double()
    g = g + wd * p0
    m = (1 - b1) * g if m is None else b1 * m.double() + (1 - b1) * g
    v = (1 - b2) * g * g if v is None else b2 * v.double() + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    return p0 - (lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps), m, v


def adam_tolerance(p0, g, step, exp_v, lr, wd, b1=0.9, b2=0.999, eps=1e-8):
    """Per-element bound for an fp32 Adam update against fp64: 1e-6 relative + 2e-9, plus the first-order
    effect of rounding g' = g + wd*p in fp32 (4 ulps of |g| + |wd*p|) through the update
    lr/bc1 * (1-b1) * dg' / (sqrt(v)/sqrt(bc2) + eps) — large only where g and wd*p nearly cancel, which
    torch's fp32 Adam computes the same way (the value is ill-conditioned, not a kernel error)."""
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    dg = 4 * 2.0 ** -23 * (g.abs() + wd * p0.abs())
    denom = exp_v.sqrt() / bc2 ** 0.5 + eps
    return 2e-9 + lr / bc1 * (1 - b1) * dg / denom


def check_adam(model, opt, p_before, m_before, v_before, step, lr=5e-4, wd=1e-4, coef=1.0):
    """The optimizer exactly: fp64 Adam applied to OUR gradient (times the clip coefficient) and OUR
    moments reproduces OUR update (adam_tolerance)."""
    for n, p in model.named_parameters():
        g = p.grad.detach().cpu().double() * coef
        exp, _, v = adam_fp64(p_before[n], g, step, lr=lr, wd=wd,
                              m=None if m_before is None else m_before[n], v=None if v_before is None else v_before[n])
        got = p.detach().cpu().double()
        tol = 1e-6 * exp.abs() + adam_tolerance(p_before[n], g, step, v, lr, wd)
        bad = (got - exp).abs() > tol
        assert not bad.any(), (n, step, int(bad.sum()), ((got - exp).abs() / tol).max().item())


def snapshot(model, opt=None):
    p = {n: q.detach().cpu().double().clone() for n, q in model.named_parameters()}
    if opt is None:
        return p, None, None
    m = {n: opt.state[q]["exp_avg"].detach().cpu().double().clone() for n, q in model.named_parameters()}
    v = {n: opt.state[q]["exp_avg_sq"].detach().cpu().double().clone() for n, q in model.named_parameters()}
    return p, m, v


def anchor(oracle_model: torch.nn.Module, ours: torch.nn.Module) -> None:
    """Load our current parameters and BatchNorm buffers into an oracle model (same state_dict keys)
    so the next step is checked from OUR state (re-anchoring: Adam's first updates are ~lr x sign(g),
    so free-running trajectories of two correct implementations separate; each step is checked
    from the same starting point instead)."""
    sd = oracle_model.state_dict()
    with torch.no_grad():
        for k, v in ours.state_dict().items():
            sd[k].copy_(v.detach().cpu().to(sd[k].dtype))


def pair_from(ours: torch.nn.Module, builder) -> Tuple[torch.nn.Module, torch.nn.Module]:
    """(fp32, fp64) oracle models holding our current state."""
    o32 = builder()
    anchor(o32, ours)
    return o32, copy.deepcopy(o32).double()


# ------------------------------------------------------------------------------------------------
# Op-level tests (test_gpu_seq_ops.py, test_gpu_loss_ops.py): one entry point against a plain-torch
# restatement in fp64, with the fp32 run of the same restatement as the yardstick
# ------------------------------------------------------------------------------------------------
GUARD = 64                    # sentinel elements after every guarded output
_SENTINEL = {torch.float32: 0x7FA5A5A5, torch.uint8: 0xA5, torch.int64: 0x7FA5A5A5A5A5A5A5}  # fp32: a NaN pattern
_BITS = {torch.float32: torch.int32, torch.uint8: torch.uint8, torch.int64: torch.int64}


class Guarded:
    """A device output of `rows` x `width` elements with row stride `ld`, followed by GUARD elements.  The whole
    allocation starts as a sentinel bit pattern; ``intact()`` asserts that the tail and the padding columns
    (ld > width) still hold it, i.e. the kernel wrote only its own elements."""

    def __init__(self, dev, rows, width, ld=None, dtype=torch.float32):
        self.rows, self.width, self.ld = rows, width, ld or width
        assert self.ld >= width
        self.flat = torch.empty(rows * self.ld + GUARD, dtype=dtype, device=dev)
        self.flat.view(_BITS[dtype]).fill_(_SENTINEL[dtype])

    @property
    def t(self) -> torch.Tensor:
        """[rows, width] view of the kernel's own elements."""
        return self.flat[:self.rows * self.ld].view(self.rows, self.ld)[:, :self.width]

    def ptr(self) -> int:
        return self.flat.data_ptr()

    def cpu(self) -> torch.Tensor:
        return self.t.cpu().contiguous()

    def intact(self, name="output"):
        bits = self.flat.cpu().view(_BITS[self.flat.dtype])
        s = _SENTINEL[self.flat.dtype]
        assert bool((bits[self.rows * self.ld:] == s).all()), f"{name}: wrote past its last element"
        pad = bits[:self.rows * self.ld].view(self.rows, self.ld)[:, self.width:]
        assert bool((pad == s).all()), f"{name}: wrote into the padding columns of its rows"


class Ratios:
    """Worst err_ours / err_ref32 per name (printed by the tests; the bound is FACTOR with the floors above)."""

    def __init__(self):
        self.worst = {}

    def note(self, name, e_ours, e_ref):
        r = e_ours / e_ref if e_ref > 0 else (0.0 if e_ours == 0 else float("inf"))
        if name not in self.worst or r > self.worst[name][0]:
            self.worst[name] = (r, e_ours, e_ref)

    def __str__(self):
        return "; ".join(f"{k} {v[0]:.2f} ({v[1]:.1e}/{v[2]:.1e})" for k, v in self.worst.items())


def op_check(name, ours, ref32, ref64, grad=False, ratios: Optional[Ratios] = None):
    """err_ours <= FACTOR * err_ref32 + floor against fp64 (FLOOR_OUT, or FLOOR_GRAD and cosine >= GRAD_COS for a
    gradient); both errors are printed before the assertion."""
    e_ours, e_ref = rel_l2(ours, ref64), rel_l2(ref32, ref64)
    floor = FLOOR_GRAD if grad else FLOOR_OUT
    print(f"{name}: err_ours {e_ours:.3e} err_ref32 {e_ref:.3e}")
    if ratios is not None:
        ratios.note(name.split("[")[0], e_ours, e_ref)
    assert e_ours <= FACTOR * e_ref + floor, f"{name}: ours {e_ours:.3e} vs fp32 reference {e_ref:.3e} (fp64 truth)"
    if grad:
        cos = cosine(ours, ref64)
        assert cos >= GRAD_COS, f"{name}: cosine {cos:.7f}"
    return e_ours, e_ref


def near_tie_flips(name, ours_idx, ref_idx, values64, dim):
    """Argmax decisions against the fp64 reference's own: a disagreement must be a near-tie (the two fp64 candidates
    within NEAR x rms of the tensor) and rare (at most max(1, MAX_FLIP_FRAC x numel)).  Returns the flip count."""
    flip = ours_idx != ref_idx
    nf = int(flip.sum())
    if nf:
        v = values64.double()
        rms = v.pow(2).mean().sqrt().item() or 1.0
        dist = (v.gather(dim, ours_idx.unsqueeze(dim)) - v.gather(dim, ref_idx.unsqueeze(dim))).squeeze(dim).abs()[flip]
        worst = dist.max().item() / rms
        assert worst <= NEAR, f"{name}: a flipped decision is {worst:.2e} x rms from its tie"
    assert nf <= max(1, MAX_FLIP_FRAC * ours_idx.numel()), f"{name}: {nf} of {ours_idx.numel()} decisions flipped"
    return nf
