"""The loss and mix entry points one at a time against plain-torch restatements in float64 on the CPU:
tspm_bce_logits (loss, gradient, the F1 / tp / fp / fn accumulators), tspm_cross_entropy (class counts, ties, large
logits, out-of-range labels) and the four tspm_pool_* calls of the MultimodalPooling fusion (all five kinds).

Criterion as tests/test_gpu_seq_ops.py (tests/parity.py): err_ours <= FACTOR x err_ref32 + floor against fp64 with
the fp32 CPU run of the same restatement as the yardstick; exact operations and integer counts are held to equality;
every output carries a sentinel guard region (and guard padding columns); every kernel runs twice for bitwise
determinism."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from parity import Guarded, Ratios, op_check
from tspm_amd import _lib as L

pytestmark = pytest.mark.gpu
RATIOS = Ratios()


def _sync():
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# BCEWithLogits + the multilabel metric accumulators
# ------------------------------------------------------------------------------------------------
def _bce_inputs(n, c):
    g = torch.Generator().manual_seed(n * 31 + c)
    x = torch.randn(n, c, generator=g) * 3
    t = (torch.rand(n, c, generator=g) > 0.6).float()
    flat_x, flat_t = x.view(-1), t.view(-1)
    plant = [(100.0, 1.0), (100.0, 0.0), (-100.0, 1.0), (-100.0, 0.0), (20.0, 0.0), (-20.0, 1.0), (0.0, 1.0), (0.0, 0.0)]
    if n * c == 1:
        flat_x[0], flat_t[0] = 0.0, 1.0   # sigmoid(0) == 0.5 is not > 0.5: predicted false, a false negative
    elif n * c >= 2 * len(plant):
        for k, (xv, tv) in enumerate(plant):
            flat_x[k], flat_t[k] = xv, tv
    if n >= 4:  # a row with no positive target and no positive prediction: F1 = 0 by zero_division
        x[n - 1], t[n - 1] = -x[n - 1].abs() - 0.5, 0.0
    return x, t


def _bce_metrics(x, t, thr, dtype):
    """Per-sample F1 (zero_division 0) summed over rows, and per-class tp / fp / fn, from sigmoid(x) > thr."""
    p = (torch.sigmoid(x.to(dtype)) > thr).numpy()
    y = (t > 0.5).numpy()
    tp, fp, fn = (p & y), (p & ~y), (~p & y)
    den = 2 * tp.sum(1) + fp.sum(1) + fn.sum(1)
    npdt = np.float32 if dtype == torch.float32 else np.float64
    f1 = np.where(den > 0, (2 * tp.sum(1)).astype(npdt) / np.maximum(den, 1).astype(npdt), npdt(0))
    return f1.sum(dtype=npdt), np.stack([tp.sum(0), fp.sum(0), fn.sum(0)], 1).reshape(-1), p


def _bce_ref(x, t, gs, dtype):
    xx = x.detach().clone().to(dtype).requires_grad_(True)
    loss = gs * F.binary_cross_entropy_with_logits(xx, t.to(dtype))
    loss.backward()
    return loss.detach().reshape(1), xx.grad


@pytest.mark.parametrize("n,c", [(1, 1), (4, 23), (257, 23), (1000, 3)])
def test_bce_logits_vs_fp64(gpu, n, c):
    x, t = _bce_inputs(n, c)
    xd, td = x.to(gpu), t.to(gpu)
    thr = 0.5
    f1_64, counts, p64 = _bce_metrics(x, t, thr, torch.float64)
    f1_32, counts32, p32 = _bce_metrics(x, t, thr, torch.float32)
    assert (p32 == p64).all(), "the seed must leave no prediction within fp32 rounding of the threshold"
    assert not p64[x.numpy() == 0].any()   # the compare is strict

    def run(gs, with_dx=True, with_stats=True, stats=None):
        loss, dx = Guarded(gpu, 1, 1), Guarded(gpu, n, c)
        if stats is None:
            stats = Guarded(gpu, 1, 3 + 3 * c)
            stats.t.zero_()
        L.check(L.lib().tspm_bce_logits(n, c, xd.data_ptr(), td.data_ptr(), loss.ptr(), dx.ptr() if with_dx else None, gs,
                                        thr, stats.ptr() if with_stats else None, L.stream_handle()), "bce_logits")
        _sync()
        loss.intact("bce loss"); dx.intact("bce dlogits"); stats.intact("bce stats")
        return loss.cpu().view(1), dx, stats
    for gs in (1.0, 0.5):
        tag = f"n{n} c{c} gs{gs}"
        l32, d32 = _bce_ref(x, t, gs, torch.float32)
        l64, d64 = _bce_ref(x, t, gs, torch.float64)
        loss, dx, stats = run(gs)
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dx.cpu()).all())
        op_check(f"bce_logits.loss[{tag}]", loss, l32, l64, ratios=RATIOS)
        op_check(f"bce_logits.dlogits[{tag}]", dx.cpu(), d32, d64, grad=True, ratios=RATIOS)
        s1 = stats.cpu().view(-1)
        op_check(f"bce_logits.stats0[{tag}]", s1[0:1], l32 * n, l64 * n, ratios=RATIOS)
        assert s1[1].item() == float(n)
        op_check(f"bce_logits.f1[{tag}]", s1[2:3], torch.tensor([f1_32]), torch.tensor([f1_64]), ratios=RATIOS)
        assert np.array_equal(s1[3:].numpy(), counts.astype(np.float32)), "tp / fp / fn are exact integer counts"
        if n >= 4:
            assert counts.reshape(c, 3)[:, :2].sum() > 0 and not p64[n - 1].any()   # the empty row is really empty
        # a second call on the same accumulators doubles every one of them exactly
        loss2, dx2, _ = run(gs, stats=stats)
        assert torch.equal(loss, loss2) and torch.equal(dx.cpu(), dx2.cpu()), "not deterministic"
        assert torch.equal(stats.cpu().view(-1), 2 * s1)
        # dlogits == NULL, stats == NULL: same loss, nothing else written
        loss3, dx3, st3 = run(gs, with_dx=False, with_stats=False)
        assert torch.equal(loss3, loss) and bool(dx3.flat.cpu().isnan().all()) and bool((st3.cpu() == 0).all())
    print("worst ratios:", RATIOS)


# ------------------------------------------------------------------------------------------------
# Cross-entropy
# ------------------------------------------------------------------------------------------------
def _ce(gpu, z, lab, gs=1.0):
    n, k = z.shape
    zd, ld = z.to(gpu), lab.to(gpu)
    loss, dz, stats = Guarded(gpu, 1, 1), Guarded(gpu, n, k), Guarded(gpu, 1, 3)
    stats.t.zero_()
    L.check(L.lib().tspm_cross_entropy(n, k, zd.data_ptr(), ld.data_ptr(), loss.ptr(), dz.ptr(), gs, stats.ptr(),
                                       L.stream_handle()), "cross_entropy")
    _sync()
    loss.intact("ce loss"); dz.intact("ce dlogits"); stats.intact("ce stats")
    return loss.cpu().view(1), dz.cpu(), stats.cpu().view(3)


def _ce_ref(z, lab, gs, dtype):
    zz = z.detach().clone().to(dtype).requires_grad_(True)
    loss = gs * F.cross_entropy(zz, lab)
    loss.backward()
    return loss.detach().reshape(1), zz.grad


def _ce_inputs(n, k):
    g = torch.Generator().manual_seed(n * 17 + k)
    z = torch.randn(n, k, generator=g) * 3
    lab = torch.randint(0, k, (n,), generator=g)
    first = z.argmax(1)
    if k >= 3:
        # equal maxima: the first index is the prediction.  Row 0: maxima at 0 and 2 (label 0: correct; the
        # last-maximum rule would miss it); row 1: maxima at 1 and k-1, label k-1 (the first-maximum rule misses it)
        z[0] = -1.0; z[0, 0] = z[0, 2] = 4.0; lab[0] = 0
        z[1] = -1.0; z[1, 1] = z[1, k - 1] = 4.0; lab[1] = k - 1
        # +-1e4: no overflow, the softmax is exactly one-hot
        z[2] = 0.0; z[2, 0], z[2, 1] = 1e4, -1e4; lab[2] = 0
        z[3] = 0.0; z[3, 0], z[3, 1] = 1e4, -1e4; lab[3] = 1
        first = z.argmax(1)
        first[0], first[1] = 0, 1
    return z, lab, first


@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("n", [7, 300])
def test_cross_entropy_classes_ties_and_large_logits(gpu, n, k):
    z, lab, first = _ce_inputs(n, k)
    for gs in (1.0, 0.25):
        tag = f"n{n} k{k} gs{gs}"
        loss, dz, stats = _ce(gpu, z, lab, gs)
        loss2, dz2, stats2 = _ce(gpu, z, lab, gs)
        assert torch.equal(loss, loss2) and torch.equal(dz, dz2) and torch.equal(stats, stats2), "not deterministic"
        l32, d32 = _ce_ref(z, lab, gs, torch.float32)
        l64, d64 = _ce_ref(z, lab, gs, torch.float64)
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dz).all())
        op_check(f"cross_entropy.loss[{tag}]", loss, l32, l64, ratios=RATIOS)
        op_check(f"cross_entropy.dlogits[{tag}]", dz, d32, d64, grad=True, ratios=RATIOS)
        op_check(f"cross_entropy.stats0[{tag}]", stats[0:1], l32 / gs * n, l64 / gs * n, ratios=RATIOS)
        assert stats[1].item() == float((first == lab).sum()) and stats[2].item() == float(n)
        if k == 1:
            assert loss.item() == 0.0 and bool((dz == 0).all()) and stats[1].item() == float(n)
    print("worst ratios:", RATIOS)


@pytest.mark.parametrize("k", [3, 16])
def test_cross_entropy_out_of_range_label_is_never_correct(gpu, k):
    """A label outside [0, classes) gives a NaN loss and a NaN gradient row (no out-of-bounds read) and is never
    counted in stats[1] = #(argmax == label) — also when the row's argmax is 0, the class the bounds-safe read
    falls back to."""
    n = 9
    z, lab, first = _ce_inputs(n, k)
    z[5] = -1.0; z[5, 0] = 3.0; lab[5] = -1
    z[6] = -1.0; z[6, 0] = 3.0; lab[6] = k
    first = z.argmax(1)
    first[0], first[1] = 0, 1
    valid = torch.ones(n, dtype=torch.bool)
    valid[5] = valid[6] = False
    loss, dz, stats = _ce(gpu, z, lab)
    want = int(((first == lab) & valid).sum())
    print(f"cross_entropy bad labels[k{k}]: stats[1] {stats[1].item()} expected {want}")
    assert loss.isnan().all() and stats[0].isnan() and stats[2].item() == float(n)
    assert bool(dz[~valid].isnan().all()) and bool(torch.isfinite(dz[valid]).all())
    # the valid rows' gradients: (softmax - onehot) / n, n counting every row
    zz = z.double()
    ref = (torch.softmax(zz, 1) - F.one_hot(lab.clamp(0, k - 1), k).double()) / n
    ref32 = (torch.softmax(z, 1) - F.one_hot(lab.clamp(0, k - 1), k).float()) / n
    op_check(f"cross_entropy.dlogits[bad labels k{k}]", dz[valid], ref32[valid], ref[valid], grad=True)
    assert stats[1].item() == float(want)


# ------------------------------------------------------------------------------------------------
# MultimodalPooling: act_fwd -> mix_fwd -> mix_bwd -> act_bwd, all five kinds
# ------------------------------------------------------------------------------------------------
def _pool_inputs(n, d, hd, kind, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    u = r(n, 2 * d)
    keep = (torch.rand(n, 2 * d, generator=g) > 0.3).to(torch.uint8)
    nk = 2 if kind == 3 else 1
    w2, b2 = r(nk, hd), r(nk) * 0.1
    hpre = r(n, hd) * 0.03
    if kind >= 3:
        # rows 0 (and 1 when n > 2): tanh(hpre) = +-1 exactly, aligned with the score direction, and w2 scaled so the
        # score difference (kind 3) / the score (kind 4) is +-80: the weights saturate without NaN
        dirn = w2[0] - w2[1] if kind == 3 else w2[0]
        w2 = w2 * (80.0 / dirn.abs().sum())
        dirn = w2[0] - w2[1] if kind == 3 else w2[0]
        b2 = b2 * 0
        hpre[0] = 20.0 * dirn.sign()
        if n > 2:
            hpre[1] = -20.0 * dirn.sign()
    if kind == 0:  # exact ties between a and b (u equal and kept alike): the gradient splits in half
        u[0, d:d + 3] = u[0, 0:3]
        keep[0, 0:3] = keep[0, d:d + 3] = 1
        u[n - 1, 2 * d - 1] = u[n - 1, d - 1]
        keep[n - 1, d - 1] = keep[n - 1, 2 * d - 1] = 0   # both dropped: 0 == 0 is a tie too
    dz, dab2 = r(n, d), r(n, 2 * d) * 0.5
    return dict(u=u, keep=keep, w2=w2, b2=b2, hpre=hpre, dz=dz, dab2=dab2)


def _pool_ref(inp, n, d, hd, kind, use_keep, use_dab2, scale, dtype):
    """Autograd through the header's formulas.  hpre is an input here (the scoring MLP's first Linear is a GEMM
    outside these kernels), so its gradient is dhpre and the gradient of [a | b] through it arrives as dab2."""
    c = lambda k: inp[k].detach().clone().to(dtype)
    u = c("u").requires_grad_(True)
    tu = torch.tanh(u)
    ab = tu * (c("keep") * scale) if use_keep else tu * 1
    a, b = ab[:, :d], ab[:, d:]
    out = dict(tu=tu, ab=ab)
    if kind == 0:
        z = torch.maximum(a, b)
    elif kind == 1:
        z = (a + b) / 2
    elif kind == 2:
        z = a + b
    else:
        hpre = c("hpre").requires_grad_(True)
        hh = torch.tanh(hpre)
        s = hh @ c("w2").T + c("b2")
        if kind == 3:
            wts = torch.softmax(s, 1)
        else:
            gate = torch.sigmoid(s)
            wts = torch.cat([gate, 1 - gate], 1)
        z = wts[:, 0:1] * a + wts[:, 1:2] * b
        out.update(hh=hh, wts=wts)
    loss = (z * c("dz")).sum()
    dab, = torch.autograd.grad(loss, ab, retain_graph=True)   # the mix's own part, as tspm_pool_mix_bwd writes it
    if use_dab2:
        loss = loss + (ab * c("dab2")).sum()
    if kind >= 3:
        du, ds, dhpre = torch.autograd.grad(loss, [u, s, hpre])
        out.update(ds=ds, dhpre=dhpre)
    else:
        du, = torch.autograd.grad(loss, u)
    out.update(z=z, dab=dab, du=du)
    return {k: v.detach() for k, v in out.items()}


@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("n,d,hd", [(3, 5, 7), (2, 300, 130)])
def test_pool_kernels_vs_fp64(gpu, n, d, hd, kind):
    inp = _pool_inputs(n, d, hd, kind, seed=kind * 10 + n)
    dev = {k: v.to(gpu) for k, v in inp.items()}
    lib, sh, scale = L.lib(), L.stream_handle(), 1.0 / 0.7
    nk = 2 if kind == 3 else 1

    def run(use_keep, use_dab2, ldz):
        o = dict(tu=Guarded(gpu, n, 2 * d), ab=Guarded(gpu, n, 2 * d), hh=Guarded(gpu, n, hd), wts=Guarded(gpu, n, 2),
                 z=Guarded(gpu, n, d, ldz), dab=Guarded(gpu, n, 2 * d), ds=Guarded(gpu, n, nk), dhpre=Guarded(gpu, n, hd),
                 du=Guarded(gpu, n, 2 * d))
        kp = dev["keep"].data_ptr() if use_keep else None
        L.check(lib.tspm_pool_act_fwd(n, d, dev["u"].data_ptr(), 2 * d, kp, scale, o["tu"].ptr(), o["ab"].ptr(), sh), "act_fwd")
        L.check(lib.tspm_pool_mix_fwd(n, d, hd, kind, o["ab"].ptr(), dev["hpre"].data_ptr(), o["hh"].ptr(),
                                      dev["w2"].data_ptr(), dev["b2"].data_ptr(), o["wts"].ptr(), o["z"].ptr(), ldz, sh),
                "mix_fwd")
        dzp = torch.full((n, ldz), 1e30, device=gpu)   # lddz == ldz: the padding columns are not gradients
        dzp[:, :d] = dev["dz"]
        L.check(lib.tspm_pool_mix_bwd(n, d, hd, kind, dzp.data_ptr(), ldz, o["ab"].ptr(), o["hh"].ptr(),
                                      dev["w2"].data_ptr(), o["wts"].ptr(), o["dab"].ptr(), o["ds"].ptr(), o["dhpre"].ptr(),
                                      sh), "mix_bwd")
        L.check(lib.tspm_pool_act_bwd(n, d, o["dab"].ptr(), dev["dab2"].data_ptr() if use_dab2 else None, o["tu"].ptr(), kp,
                                      scale, o["du"].ptr(), sh), "act_bwd")
        _sync()
        for k, gd in o.items():
            gd.intact("pool " + k)
        return o
    for use_keep in (True, False):
        for use_dab2 in (True, False):
            for ldz in (d, d + 3):
                tag = f"kind{kind} n{n} d{d} keep{int(use_keep)} dab2{int(use_dab2)} ldz{ldz}"
                o = run(use_keep, use_dab2, ldz)
                o2 = run(use_keep, use_dab2, ldz)
                names = ["tu", "ab", "z", "dab", "du"] + (["hh", "wts", "ds", "dhpre"] if kind >= 3 else [])
                for k in names:
                    assert torch.equal(o[k].cpu(), o2[k].cpu()), f"{k}: not deterministic"
                for k in set(o) - set(names):   # kinds 0-2 have no scoring MLP: its buffers stay untouched
                    assert bool(o[k].flat.cpu().isnan().all()), k
                r32 = _pool_ref(inp, n, d, hd, kind, use_keep, use_dab2, scale, torch.float32)
                r64 = _pool_ref(inp, n, d, hd, kind, use_keep, use_dab2, scale, torch.float64)
                for k in names:
                    got = o[k].cpu()
                    assert bool(torch.isfinite(got).all()), k
                    op_check(f"pool.{k}[{tag}]", got, r32[k], r64[k], grad=k in ("dab", "du", "ds", "dhpre"), ratios=RATIOS)
                # exact in fp32: the keep-mask scale, and for kinds 0-2 the mix and its backward on our own ab
                tu, ab = o["tu"].cpu(), o["ab"].cpu()
                mask = torch.where(inp["keep"].bool(), torch.tensor(scale), torch.tensor(0.0)) if use_keep else None
                assert torch.equal(ab, tu * mask if use_keep else tu)
                a, b, dz = ab[:, :d], ab[:, d:], inp["dz"]
                if kind <= 2:
                    z = torch.maximum(a, b) if kind == 0 else ((a + b) / 2 if kind == 1 else a + b)
                    assert torch.equal(o["z"].cpu(), z)
                    if kind == 0:
                        da = torch.where(a == b, dz / 2, torch.where(a > b, dz, torch.zeros(())))
                        db = torch.where(a == b, dz / 2, torch.where(b > a, dz, torch.zeros(())))
                        assert int((a == b).sum()) >= 4, "the planted ties are there"
                    else:
                        da = db = dz / 2 if kind == 1 else dz
                    assert torch.equal(o["dab"].cpu(), torch.cat([da, db], 1))
                else:   # the planted rows saturate: the dominant weight is exactly 1, the other vanishes
                    w = o["wts"].cpu()
                    assert w[0].max().item() == 1.0 and w[0].min().item() < 1e-30
                    if n > 2:
                        assert w[1].max().item() == 1.0 and w[1].min().item() < 1e-30 and w[0].argmax() != w[1].argmax()
    print("worst ratios:", RATIOS)
