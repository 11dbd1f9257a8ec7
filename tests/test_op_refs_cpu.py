"""The op-level references of tests/op_refs.py, checked on the CPU against torch's own float64 operators: the
GPU tests (test_gpu_gemm_paths.py, test_gpu_bn1d_variants.py, test_gpu_reduce_slabs.py) hold the HIP kernels to
these references, so the references themselves must be right without a GPU."""
import numpy as np
import pytest
import torch

import op_refs as R


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------
# small GEMM
# ------------------------------------------------------------------------------------------------
def test_exact_regime_data_and_bound():
    v = R.exact_ints(_gen(1), 1000, 7)
    assert v.dtype == torch.float32
    assert set(v.unique().tolist()) == {-3.0, -2.0, -1.0, 1.0, 2.0, 3.0}
    assert R.exact_regime_ok(4100) and not R.exact_regime_ok(4101)
    with pytest.raises(AssertionError):
        R.gemm_inputs(_gen(2), "E", 4, 4101, 3)


@pytest.mark.parametrize("n,fin,fout", [(5, 300, 33), (33, 7, 65), (257, 33, 40)])
def test_exact_regime_is_exact_in_fp32_in_any_order(n, fin, fout):
    """The premise of regime E: fp32 arithmetic on this data, forwards, backwards or in halves, gives the int64
    result; and the int64 and fp64 references are the same numbers."""
    x, w, b, dy, keep = R.gemm_inputs(_gen(n + fin), "E", n, fin, fout)
    y, tol = R.linear_fwd_ref("E", x, w, b, True, keep)
    assert tol is None and y.dtype == torch.int64
    y32 = torch.relu(x @ w.T + b) * keep.float() * 2.0
    assert torch.equal(y32, y.float())
    rev = torch.arange(fin - 1, -1, -1)
    h = fin // 2
    assert torch.equal(torch.relu(x[:, rev] @ w[:, rev].T + b) * keep.float() * 2.0, y.float())
    assert torch.equal(torch.relu((x[:, h:] @ w[:, h:].T + x[:, :h] @ w[:, :h].T) + b) * keep.float() * 2.0, y.float())
    dx, _ = R.linear_bwd_data_ref("E", dy, w)
    dw, db, _, _ = R.linear_bwd_weight_ref("E", x, dy)
    assert torch.equal(dy @ w, dx.float()) and torch.equal(dy.T @ x, dw.float()) and torch.equal(dy.sum(0), db.float())
    y64, _ = R.linear_fwd_ref("R", x, w, b, True, keep)
    assert torch.equal(y64, y.double())
    assert int(y.abs().max()) < 2 ** 24 and int(dw.abs().max()) < 2 ** 24


@pytest.mark.parametrize("relu,use_keep,use_bias", [(0, 0, 0), (1, 1, 1), (0, 1, 1), (1, 0, 0)])
def test_linear_refs_match_double_autograd(relu, use_keep, use_bias):
    n, fin, fout = 9, 130, 40
    x, w, b, dy, keep = R.gemm_inputs(_gen(7), "R", n, fin, fout)
    lin = torch.nn.Linear(fin, fout, bias=bool(use_bias)).double()
    with torch.no_grad():
        lin.weight.copy_(w.double())
        if use_bias:
            lin.bias.copy_(b.double())
    xr = x.double().requires_grad_(True)
    z = lin(xr)
    z.retain_grad()
    out = torch.relu(z) if relu else z
    if use_keep:
        out = out * keep.double() * R.KEEP_SCALE
    out.backward(dy.double())
    y, tol = R.linear_fwd_ref("R", x, w, b if use_bias else None, relu, keep if use_keep else None)
    assert (y - out.detach()).abs().max() <= 1e-10
    assert tol.shape == y.shape and bool((tol >= 0).all())
    if use_keep:
        assert bool((tol[keep == 0] == 0).all())  # a dropped element must be exactly zero
    gz = z.grad.float()  # the gradient that reaches the Linear: the products' dy
    dx, tdx = R.linear_bwd_data_ref("R", gz, w)
    dw, db, tdw, tdb = R.linear_bwd_weight_ref("R", x, gz)
    assert (dx - xr.grad).abs().max() <= 1e-6 * xr.grad.abs().max()  # gz was rounded to fp32
    assert (dw - lin.weight.grad).abs().max() <= 1e-6 * lin.weight.grad.abs().max()
    dx, _ = R.linear_bwd_data_ref("R", z.grad, w)
    dw, db, _, _ = R.linear_bwd_weight_ref("R", x, z.grad)
    assert (dx - xr.grad).abs().max() <= 1e-10 and (dw - lin.weight.grad).abs().max() <= 1e-10
    if use_bias:
        assert (db - lin.bias.grad).abs().max() <= 1e-10


def test_check_sees_one_wrong_element_and_nan():
    x, w, b, dy, keep = R.gemm_inputs(_gen(3), "E", 33, 64, 40)
    y, _ = R.linear_fwd_ref("E", x, w, b)
    good = y.float()
    R.check("exact", good, y)
    bad = good.clone()
    bad[17, 5] += 1.0
    with pytest.raises(AssertionError, match="1 of"):
        R.check("exact", bad, y)
    x, w, b, dy, keep = R.gemm_inputs(_gen(4), "R", 33, 128, 40)
    y, tol = R.linear_fwd_ref("R", x, w, b)
    good = (x @ w.T + b)
    assert R.check("fp32[cpu]", good, y, tol) < 1.0  # torch's own fp32 product sits inside the bound
    bad = good.clone()
    bad[3, 2] += 3 * tol[3, 2].float() + 1e-6
    with pytest.raises(AssertionError, match="max ratio"):
        R.check("fp32[cpu]", bad, y, tol)
    bad = good.clone()
    bad[0, 0] = float("nan")
    with pytest.raises(AssertionError):
        R.check("fp32[cpu]", bad, y, tol)
    # a dropped k (the last one) is outside the bound for almost every element
    short = x[:, :-1] @ w[:, :-1].T + b
    with pytest.raises(AssertionError):
        R.check("fp32[cpu]", short, y, tol)


def test_padded_layout():
    t = torch.arange(6.0).view(2, 3)
    f = R.padded(t, 5, lead=1)
    assert f.numel() == 11 and f[0] == 1e30
    assert torch.equal(f[1:].view(2, 5)[:, :3], t) and bool((f[1:].view(2, 5)[:, 3:] == 1e30).all())


# ------------------------------------------------------------------------------------------------
# BatchNorm1d
# ------------------------------------------------------------------------------------------------
def _bn_data(m, c, kind, seed=0):
    g = _gen(seed + 13 * m + c)
    x = torch.randn(m, c, generator=g) * 3 + 1 if kind == "a" else 1000 + torch.randn(m, c, generator=g)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    rm, rv = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    gy = torch.randn(m, c, generator=g)
    keep = (torch.rand(m, c, generator=g) > 0.5).to(torch.uint8)
    return x, gamma, beta, rm, rv, gy, keep


@pytest.mark.parametrize("m,c,kind", [(2, 1, "a"), (4, 33, "a"), (31, 32, "b"), (65, 68, "a"), (33, 31, "b")])
@pytest.mark.parametrize("variant", ["plain", "drop", "drop_relu"])
def test_bn1d_refs_match_double_autograd(m, c, kind, variant):
    """nn.BatchNorm1d in float64 (chained with ReLU before it and dropout-by-mask after it for the fused
    variants) gives the references' y, running statistics, dgamma, dbeta and dx to 1e-10."""
    x, gamma, beta, rm, rv, gy, keep = _bn_data(m, c, kind)
    mom, eps = 0.1, 1e-5
    bn = torch.nn.BatchNorm1d(c, eps=eps, momentum=mom).double()
    with torch.no_grad():
        bn.weight.copy_(gamma.double()); bn.bias.copy_(beta.double())
        bn.running_mean.copy_(rm.double()); bn.running_var.copy_(rv.double())
    scale = 2.0
    if variant == "drop_relu":
        z = (x - (1.0 if kind == "a" else 1000.0)).double().requires_grad_(True)
        h = torch.relu(z)
        xin = h.detach().float()
        assert bool((xin == 0).any())
    else:
        z = x.double().requires_grad_(True)
        h = z
        xin = x
    y = bn(h)
    kp = None if variant == "plain" else keep
    out = y if kp is None else y * kp.double() * scale
    out.backward(gy.double())
    f = R.bn1d_fwd_ref(xin, gamma, beta, rm, rv, mom, eps, kp, scale)
    tol = 1e-10
    assert (f["y"] - out.detach()).abs().max() <= tol
    assert (f["rmean"] - bn.running_mean).abs().max() <= tol and (f["rvar"] - bn.running_var).abs().max() <= tol
    b = R.bn1d_bwd_ref(gy, xin, f["mean"], f["invstd"], gamma, kp, scale, relu_x=variant == "drop_relu")
    assert (b["dgamma"] - bn.weight.grad).abs().max() <= tol
    assert (b["dbeta"] - bn.bias.grad).abs().max() <= tol
    assert (b["dx"] - z.grad).abs().max() <= tol
    for k, v in list(f.items()) + list(b.items()):
        if k.startswith("tol_"):
            assert bool((v >= 0).all()) and bool(torch.isfinite(v).all())


def test_bn1d_refs_constant_and_dead_channels():
    """A constant channel has variance 0: xhat = 0, y = beta, dgamma = 0; an all-zero ("dead ReLU") channel of the
    drop_relu variant also has dx = 0.  The tolerances there are exactly 0 where the result is exactly known."""
    m, c = 33, 4
    x, gamma, beta, rm, rv, gy, keep = _bn_data(m, c, "a", seed=5)
    x = torch.relu(x)
    x[:, 1] = 1234.5
    x[:, 2] = 0.0
    f = R.bn1d_fwd_ref(x, gamma, beta, rm, rv, 0.1, 1e-5)
    for ch in (1, 2):
        assert bool((f["xhat"][:, ch] == 0).all()) and bool((f["y"][:, ch] == beta[ch].double()).all())
        assert f["invstd"][ch] == 1.0 / np.sqrt(1e-5)
    b = R.bn1d_bwd_ref(gy, x, f["mean"].float(), f["invstd"].float(), gamma, keep, 2.0, relu_x=True)
    assert b["dgamma"][1] == 0 and b["dgamma"][2] == 0 and b["tol_dgamma"][2] == 0
    assert bool((b["dx"][:, 2] == 0).all()) and bool((b["tol_dx"][:, 2] == 0).all())
    assert b["dbeta"][2] == (gy[:, 2].double() * keep[:, 2].double() * 2).sum()


# ------------------------------------------------------------------------------------------------
# slab reduction
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count,nslab", [(7, 3), (50, 15), (50, 16), (50, 17), (50, 37), (1, 1)])
def test_reduce_slabs_emulation_order(count, nslab):
    slabs = torch.randn(nslab, count, generator=_gen(nslab)) * 10.0 ** torch.randint(-3, 4, (nslab, 1), generator=_gen(1))
    s = slabs.numpy()
    narrow = np.zeros(count, np.float32)
    for z in range(nslab):
        narrow = (narrow + s[z]).astype(np.float32)
    wide = np.zeros(count, np.float32)
    for q in range(8):
        p = np.float32(0) * np.zeros(count, np.float32)
        z = q
        while z < nslab:
            p = (p + s[z]).astype(np.float32)
            z += 8
        wide = (wide + p).astype(np.float32)
    assert torch.equal(R.reduce_slabs_emul(slabs, False), torch.from_numpy(narrow))
    assert torch.equal(R.reduce_slabs_emul(slabs, True), torch.from_numpy(wide))
    ref, tol = slabs.double().sum(0), R.reduce_slabs_tol(slabs)
    for wide_ in (False, True):
        assert bool(((R.reduce_slabs_emul(slabs, wide_).double() - ref).abs() <= tol).all())
    assert R.reduce_slabs_is_wide(count, nslab) == (nslab >= 16)
    assert not R.reduce_slabs_is_wide((1 << 18) + 1, 64)


def test_reduce_slabs_orders_differ():
    """The two orders are different fp32 results on ordinary data, so the bitwise comparison tells them apart (and
    a swap of two group partials from the documented order)."""
    slabs = torch.randn(37, 4000, generator=_gen(9))
    a, b = R.reduce_slabs_emul(slabs, False), R.reduce_slabs_emul(slabs, True)
    assert int((a != b).sum()) > 100
    perm = list(range(37))
    for z in range(1, 36, 8):  # groups 1 and 2 exchanged: the same partials added in the order 0, 2, 1, 3, ...
        perm[z], perm[z + 1] = z + 1, z
    assert int((R.reduce_slabs_emul(slabs[perm], True) != b).sum()) > 100


# ------------------------------------------------------------------------------------------------
# argmax conventions
# ------------------------------------------------------------------------------------------------
def test_softmax_tie_rows():
    z, first, larger = R.softmax_tie_rows()
    assert z.dtype == torch.float32
    for r in range(z.shape[0]):
        top = torch.topk(z[r].double(), 2)
        assert top.values[0] > top.values[1] and int(top.indices[0]) == int(larger[r])
        # same fp32 probability: exp(z - max) is 1.0f for both
        e = torch.exp(z[r] - z[r].max())
        assert e[first[r]] == 1.0 and e[larger[r]] == 1.0
        p = torch.softmax(z[r], 0)
        assert int((p == p.max()).nonzero()[0]) == int(first[r])
        assert int(torch.argmax(z[r])) == int(larger[r])
    assert bool((first[:2] != larger[:2]).all()) and bool((first[2:] == larger[2:]).all())
