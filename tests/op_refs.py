"""Plain CPU references and per-element error bounds for the op-level tests of the small GEMM (csrc/misc.hip),
the one-launch BatchNorm1d and its fused variants (csrc/mmimdb.hip) and the slab reduction (csrc/conv.hip).

Nothing here touches the GPU or libtspm: tests/test_op_refs_cpu.py checks these references against torch's own
float64 operators, the test_gpu_* files hold the kernels to them ("Op-level bounds of the glue
kernels").

Small GEMM, two data regimes:
  E (exact)   every input an integer in {+-1, +-2, +-3} stored as fp32, keep scale 2: each product is an integer of
              magnitude <= 9 and every partial sum, in any order, an integer below 2^24 (exact_regime_ok asserts
              9*K + 3 < 2^24), so fp32 arithmetic is exact and the kernel must EQUAL the int64 reference.  A dropped,
              doubled or mis-paired index cannot hide in a tolerance, whatever the wave split.
  R (rounding) randn inputs, weights x 0.05, fp64 reference, |err| <= 64 * 2^-23 * sum|a||b| (+ 2^-23 |bias|) per
              element: the bound the convolution tests use (tests/test_gpu_ops.py::_check).
"""
from __future__ import annotations

import torch

EPS32 = 2.0 ** -23
EPS_DSUM = 2.0 ** -40   # a double sum of <= 2^12 fp32-sized terms, as a fraction of sum|terms| (2^-53 per add)
GEMM_FACTOR = 64        # the convolution tests' factor on 2^-23 * sum|a||b|
KEEP_SCALE = 2.0        # dropout p = 0.5: a power of two, so x * scale is exact in both regimes


# ------------------------------------------------------------------------------------------------
# data
# ------------------------------------------------------------------------------------------------
def exact_regime_ok(k: int) -> bool:
    """Regime E's premise for a reduction over k terms (+ a bias of magnitude <= 3)."""
    return k <= 4100 and 9 * k + 3 < 2 ** 24


def exact_ints(gen: torch.Generator, *shape) -> torch.Tensor:
    """Integers drawn from {+-1, +-2, +-3}, as fp32."""
    mag = torch.randint(1, 4, shape, generator=gen)
    sign = torch.randint(0, 2, shape, generator=gen) * 2 - 1
    return (mag * sign).float()


def gemm_inputs(gen: torch.Generator, regime: str, n: int, fin: int, fout: int):
    """x [n, fin], w [fout, fin], b [fout], dy [n, fout] and a keep mask [n, fout] of one regime."""
    if regime == "E":
        assert exact_regime_ok(max(n, fin, fout)), "regime E needs every partial sum below 2^24"
        x, w, b, dy = (exact_ints(gen, *s) for s in ((n, fin), (fout, fin), (fout,), (n, fout)))
    else:
        x, w = torch.randn(n, fin, generator=gen), torch.randn(fout, fin, generator=gen) * 0.05
        b, dy = torch.randn(fout, generator=gen), torch.randn(n, fout, generator=gen)
    keep = (torch.rand(n, fout, generator=gen) > 0.5).to(torch.uint8)
    return x, w, b, dy, keep


def padded(t: torch.Tensor, ld: int, lead: int = 0, fill: float = 1e30) -> torch.Tensor:
    """t's rows laid out `ld` apart after `lead` floats, in a flat buffer whose other elements are `fill` (not data:
    a kernel that reads them shows it)."""
    rows, width = t.shape
    assert ld >= width
    flat = torch.full((lead + rows * ld,), fill, dtype=t.dtype)
    flat[lead:].view(rows, ld)[:, :width] = t
    return flat


# ------------------------------------------------------------------------------------------------
# nn.Linear's three products
# ------------------------------------------------------------------------------------------------
def _acc(regime: str):
    return torch.int64 if regime == "E" else torch.float64


def linear_fwd_ref(regime, x, w, b=None, relu=False, keep=None, scale=KEEP_SCALE):
    """(y, tol): y = relu(x w^T + b) * keep * scale in int64 (E) or fp64 (R); tol None in E, else the per-element
    bound.  ReLU does not grow the error; the keep mask scales it (a dropped element must be exactly 0)."""
    dt = _acc(regime)
    y = x.to(dt) @ w.to(dt).T
    tol = None if regime == "E" else GEMM_FACTOR * EPS32 * (x.double().abs() @ w.double().abs().T)
    if b is not None:
        y = y + b.to(dt)
        if tol is not None:
            tol = tol + EPS32 * b.double().abs()
    if relu:
        y = y.clamp_min(0)
    if keep is not None:
        s = int(scale) if regime == "E" else float(scale)
        assert s == scale
        y = y * keep.to(dt) * s
        if tol is not None:
            tol = tol * keep.double() * s
    return y, tol


def linear_bwd_data_ref(regime, dy, w):
    dt = _acc(regime)
    dx = dy.to(dt) @ w.to(dt)
    return dx, (None if regime == "E" else GEMM_FACTOR * EPS32 * (dy.double().abs() @ w.double().abs()))


def linear_bwd_weight_ref(regime, x, dy):
    """(dw, db, tol_dw, tol_db): dw = dy^T x, db = column sums of dy (bound 64 * 2^-23 * sum|dy|)."""
    dt = _acc(regime)
    dw, db = dy.to(dt).T @ x.to(dt), dy.to(dt).sum(0)
    if regime == "E":
        return dw, db, None, None
    return dw, db, GEMM_FACTOR * EPS32 * (dy.double().abs().T @ x.double().abs()), \
        GEMM_FACTOR * EPS32 * dy.double().abs().sum(0)


WORST = {}  # name -> worst err / tol seen (printed by the tests; DESIGN §4 quotes the MI355X figures)


def check(name: str, out: torch.Tensor, ref: torch.Tensor, tol=None):
    """tol None: out must equal ref exactly (regime E; -0.0, a dropped negative value, equals the integer 0).
    Otherwise |out - ref| <= tol per element; the worst err / tol is printed, recorded and reported on failure."""
    out = out.detach().cpu()
    assert out.shape == ref.shape, f"{name}: shape {tuple(out.shape)} vs {tuple(ref.shape)}"
    if tol is None:
        want = ref.to(torch.float32)
        assert bool((want.to(ref.dtype) == ref).all()), f"{name}: the reference is not exact in fp32"
        bad = out != want
        assert not bool(bad.any()), f"{name}: {int(bad.sum())} of {bad.numel()} elements differ from the exact " \
                                    f"result; first at {tuple(bad.nonzero()[0].tolist())}"
        return 0.0
    err = (out.double() - ref.double()).abs()
    tol = tol.double().expand_as(err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol.clamp_min(1e-300))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    key = name.split("[")[0]
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print(f"RATIO {name} {worst:.4f}")
    bad = ~(err <= tol)  # a NaN is out of tolerance
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} elements out of tolerance; max err {err.max().item():.3e}, " \
                                f"max ratio {worst:.2f}"
    return worst


# ------------------------------------------------------------------------------------------------
# BatchNorm1d (training mode) and its fused variants
# ------------------------------------------------------------------------------------------------
def bn1d_fwd_ref(x, gamma, beta, rmean=None, rvar=None, momentum=0.1, eps=1e-5, keep=None, scale=1.0):
    """fp64 batch statistics of the fp32 input; y = (x - mean) * invstd * gamma + beta, then * keep * scale (the
    Dropout after the BN); running statistics as nn.BatchNorm1d (unbiased variance).  Returns a dict of fp64
    tensors, with the per-element tolerance of every output under "tol_*"."""
    x64, ga, be = x.double(), gamma.double(), beta.double()
    m = x64.shape[0]
    mean = x64.mean(0)
    var = (x64 - mean).pow(2).mean(0)
    invstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x64 - mean) * invstd
    y = xhat * ga + be
    # fp32 evaluation of (x - mean32) * invstd32 * gamma + beta: a few roundings of xhat*gamma and of y, plus the
    # fp32 rounding of the mean (2^-24 |mean|, scaled by invstd * |gamma|)
    tol_y = EPS32 * (8 * (xhat * ga).abs() + 2 * y.abs() + mean.abs() * invstd * ga.abs())
    if keep is not None:
        y = y * keep.double() * scale
        tol_y = tol_y * keep.double() * scale
    r = dict(mean=mean, invstd=invstd, xhat=xhat, y=y, tol_y=tol_y,
             tol_mean=EPS32 * mean.abs(), tol_invstd=EPS32 * invstd.abs())
    if rmean is not None:
        r["rmean"] = (1 - momentum) * rmean.double() + momentum * mean
        r["tol_rmean"] = 4 * EPS32 * (rmean.double().abs() + r["rmean"].abs())
    if rvar is not None:
        r["rvar"] = (1 - momentum) * rvar.double() + momentum * var * (m / (m - 1))
        r["tol_rvar"] = 4 * EPS32 * (rvar.double().abs() + r["rvar"].abs())
    return r


def bn1d_bwd_ref(g, x, mean_saved, invstd_saved, gamma, keep=None, scale=1.0, relu_x=False):
    """The backward from the SAVED mean / invstd (the fp32 values handed to the kernel, promoted to fp64):
    g_eff = g * keep * scale, dbeta = sum g_eff, dgamma = sum g_eff * xhat,
    dx = gamma * invstd * (g_eff - mean(g_eff) - xhat * mean(g_eff * xhat)), zero where x <= 0 with relu_x.
    The sums are double sums rounded once to fp32; dx is a double expression rounded once."""
    g64, x64, ga = g.double(), x.double(), gamma.double()
    mean, invstd = mean_saved.double(), invstd_saved.double()
    m = x64.shape[0]
    geff = g64 if keep is None else g64 * keep.double() * scale
    xhat = (x64 - mean) * invstd
    dbeta, dgamma = geff.sum(0), (geff * xhat).sum(0)
    mg, mgx = dbeta / m, dgamma / m
    k = ga * invstd
    dx = k * (geff - mg - xhat * mgx)
    tol_dx = EPS32 * dx.abs() + EPS_DSUM * k.abs() * (geff.abs() + mg.abs() + xhat.abs() * mgx.abs())
    if relu_x:
        live = (x64 > 0).double()
        dx, tol_dx = dx * live, tol_dx * live
    return dict(dgamma=dgamma, dbeta=dbeta, dx=dx, tol_dx=tol_dx,
                tol_dgamma=EPS32 * dgamma.abs() + EPS_DSUM * (geff * xhat).abs().sum(0),
                tol_dbeta=EPS32 * dbeta.abs() + EPS_DSUM * geff.abs().sum(0))


# ------------------------------------------------------------------------------------------------
# slab reduction
# ------------------------------------------------------------------------------------------------
WIDE_GROUPS = 8
WIDE_MIN_SLABS, WIDE_MAX_COUNT = 16, 1 << 18


def reduce_slabs_is_wide(count: int, nslab: int) -> bool:
    return nslab >= WIDE_MIN_SLABS and count <= WIDE_MAX_COUNT


def reduce_slabs_emul(slabs: torch.Tensor, wide: bool) -> torch.Tensor:
    """fp32 emulation of tspm_reduce_slabs' documented order over slabs [nslab, count] (torch's elementwise fp32
    add is the IEEE add).  Narrow: 0 + slab 0 + slab 1 + ...  Wide: group q sums slabs q, q+8, q+16, ... in order
    from 0, then the 8 partial sums are added in group order from 0."""
    assert slabs.dtype == torch.float32
    nslab, count = slabs.shape
    zero = torch.zeros(count, dtype=torch.float32)
    if not wide:
        s = zero.clone()
        for z in range(nslab):
            s = s + slabs[z]
        return s
    t = zero.clone()
    for q in range(WIDE_GROUPS):
        p = zero.clone()
        for z in range(q, nslab, WIDE_GROUPS):
            p = p + slabs[z]
        t = t + p
    return t


def reduce_slabs_tol(slabs: torch.Tensor) -> torch.Tensor:
    """nslab * 2^-23 * sum|slab| per element: at most nslab fp32 adds, each within 2^-24 of a partial sum that is
    itself at most sum|slab|."""
    return slabs.shape[0] * EPS32 * slabs.double().abs().sum(0)


# ------------------------------------------------------------------------------------------------
# argmax conventions of tspm_classify_update_ex
# ------------------------------------------------------------------------------------------------
def softmax_tie_rows(classes: int = 5):
    """(logits [4, classes] fp32, first index, larger index): rows whose two largest logits are 1 ulp apart at
    magnitude 1e-3 (2^-33 apart: exp(-2^-33) rounds to 1.0f, so both have the same fp32 softmax value).  In rows
    0-1 the smaller comes first (argmax of the softmax picks it, argmax of the logits the larger); in rows 2-3 the
    larger comes first (both pick it)."""
    a = torch.tensor(1e-3, dtype=torch.float32)
    b = torch.nextafter(a, torch.tensor(1.0))
    z = torch.full((4, classes), -2.0)
    z[:, 0] = -1.0
    first = torch.tensor([1, 2, 1, 3])
    second = torch.tensor([3, 4, 2, 4])
    for r in range(4):
        lo, hi = (a, b) if r < 2 else (b, a)
        z[r, first[r]], z[r, second[r]] = lo, hi
    larger = torch.where(torch.arange(4) < 2, second, first)
    return z, first, larger
