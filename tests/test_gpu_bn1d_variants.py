"""The one-launch BatchNorm1d of csrc/mmimdb.hip through all six entry points (tspm_bn1d_fwd / _bwd, _fwd_drop,
_bwd_drop_relu, _fwd_pair, _bwd_pair) against the fp64 references of op_refs.py, per element.

The kernel gives a workgroup 32 channels and 32 row groups (row r belongs to group r % 32), sums in double and
stores / uses the mean and invstd in fp32.  The bounds (op_refs.bn1d_fwd_ref / bn1d_bwd_ref) follow from that
arithmetic; the backward reference takes the fp32 mean / invstd handed to the kernel.  Dropout scale 2 (p = 0.5):
g * scale is then exact in fp32, as the bounds on dgamma / dbeta / dx assume.

Shapes: m in {2, 4, 31, 32, 33, 65} (fewer rows than groups, exactly 32, one and two extra rounds), c in
{1, 31, 32, 33, 68} (a partly filled workgroup, exactly one, one channel into the next, three workgroups).
Data: (a) randn*3 + 1; (b) 1000 + randn (cancellation in the statistics and in x - mean); (c) as (a) with one
constant channel (variance 0, xhat = 0, dgamma = 0) and, for drop_relu, one all-zero "dead ReLU" channel (dx = 0).
"""
import pytest
import torch

import op_refs as R
from parity import Guarded
from tspm_amd import _lib as L

pytestmark = pytest.mark.gpu
INVALID = 1
MOM = torch.tensor(0.1, dtype=torch.float32).item()   # the fp32 values the kernel receives
EPS = torch.tensor(1e-5, dtype=torch.float32).item()
SCALE = 2.0
SHAPES = [(2, 33), (4, 1), (31, 68), (32, 31), (33, 32), (65, 33)]  # every m and every c once


def _sync():
    torch.cuda.synchronize()


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _data(m, c, kind, relu_input=False, seed=0):
    """x, gamma, beta, running mean / var, the output gradient and a keep mask.  relu_input: x is a ReLU output
    (exact zeros in (a) and (c); at (b)'s offset every element stays positive)."""
    g = torch.Generator().manual_seed(seed + 131 * m + c + {"a": 0, "b": 5000, "c": 9000}[kind])
    x = 1000 + torch.randn(m, c, generator=g) if kind == "b" else torch.randn(m, c, generator=g) * 3 + 1
    if relu_input:
        x = torch.relu(x)
    if kind == "c":
        x[:, c // 2] = 1234.5           # constant channel
        if relu_input:
            x[:, 0] = 0.0               # dead ReLU channel (with c == 1 it replaces the constant one)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    gamma[::3] *= -1
    rm, rv = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    gy = torch.randn(m, c, generator=g)
    keep = (torch.rand(m, c, generator=g) > 0.5).to(torch.uint8)
    return x, gamma, beta, rm, rv, gy, keep


def _vec(gpu, t):
    """A [c] in/out vector in a guarded buffer."""
    g = Guarded(gpu, 1, t.numel())
    g.t.copy_(t.view(1, -1))
    return g


class FwdOut:
    def __init__(self, gpu, m, c, rm, rv):
        self.y, self.mean, self.inv = Guarded(gpu, m, c), Guarded(gpu, 1, c), Guarded(gpu, 1, c)
        self.rm = _vec(gpu, rm) if rm is not None else None
        self.rv = _vec(gpu, rv) if rv is not None else None

    def args(self):
        return (self.rm.ptr() if self.rm else None, self.rv.ptr() if self.rv else None)

    def done(self, what):
        for n in ("y", "mean", "inv", "rm", "rv"):
            g = getattr(self, n)
            if g is not None:
                g.intact(f"{what} {n}")

    def cpu(self, n):
        g = getattr(self, n)
        return g.cpu() if n == "y" else g.cpu().view(-1)


def _fwd(gpu, x, gamma, beta, rm, rv, entry="fwd", keep=None, mom=MOM, eps=EPS):
    m, c = x.shape
    xd, gd, bd = x.to(gpu), gamma.to(gpu), beta.to(gpu)
    o = FwdOut(gpu, m, c, rm, rv)
    lib, sh = L.lib(), L.stream_handle()
    if entry == "fwd":
        st = lib.tspm_bn1d_fwd(m, c, xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), *o.args(), mom, eps, o.mean.ptr(),
                               o.inv.ptr(), o.y.ptr(), sh)
    else:
        kd = keep.to(gpu) if keep is not None else None
        st = lib.tspm_bn1d_fwd_drop(m, c, xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), *o.args(), mom, eps, o.mean.ptr(),
                                    o.inv.ptr(), L.ptr(kd), SCALE, o.y.ptr(), sh)
    L.check(st, "bn1d_" + entry)
    _sync()
    o.done("bn1d_" + entry)
    return o


def _check_fwd(name, tag, o, f):
    R.check(f"{name}.y[{tag}]", o.cpu("y"), f["y"], f["tol_y"])
    R.check(f"{name}.save_mean[{tag}]", o.cpu("mean"), f["mean"], f["tol_mean"])
    R.check(f"{name}.save_invstd[{tag}]", o.cpu("inv"), f["invstd"], f["tol_invstd"])
    if o.rm is not None:
        R.check(f"{name}.running_mean[{tag}]", o.cpu("rm"), f["rmean"], f["tol_rmean"])
    if o.rv is not None:
        R.check(f"{name}.running_var[{tag}]", o.cpu("rv"), f["rvar"], f["tol_rvar"])


@pytest.mark.parametrize("m,c", SHAPES)
@pytest.mark.parametrize("kind", ["a", "b", "c"])
def test_bn1d_fwd_and_fwd_drop(gpu, m, c, kind):
    x, gamma, beta, rm, rv, gy, keep = _data(m, c, kind)
    tag = f"m{m} c{c} {kind}"
    f = R.bn1d_fwd_ref(x, gamma, beta, rm, rv, MOM, EPS)
    plain = _fwd(gpu, x, gamma, beta, rm, rv)
    _check_fwd("bn1d_fwd", tag, plain, f)
    if kind == "c":  # the constant channel: variance 0, y = beta exactly
        ch = c // 2
        assert torch.equal(plain.cpu("y")[:, ch], beta[ch].expand(m))
        assert plain.cpu("mean")[ch] == 1234.5
    # NULL running statistics (the monomodal path): the same y and saved statistics
    bare = _fwd(gpu, x, gamma, beta, None, None)
    for n in ("y", "mean", "inv"):
        assert _bits_equal(bare.cpu(n), plain.cpu(n)), f"NULL running stats changed {n}"
    # Dropout after the BN
    fd = R.bn1d_fwd_ref(x, gamma, beta, rm, rv, MOM, EPS, keep, SCALE)
    drop = _fwd(gpu, x, gamma, beta, rm, rv, "fwd_drop", keep)
    _check_fwd("bn1d_fwd_drop", tag, drop, fd)
    assert bool((drop.cpu("y")[keep == 0] == 0).all())
    # keep NULL: bitwise tspm_bn1d_fwd
    nodrop = _fwd(gpu, x, gamma, beta, rm, rv, "fwd_drop", None)
    for n in ("y", "mean", "inv", "rm", "rv"):
        assert _bits_equal(nodrop.cpu(n), plain.cpu(n)), f"fwd_drop with keep NULL differs from bn1d_fwd in {n}"


# ------------------------------------------------------------------------------------------------
# backward
# ------------------------------------------------------------------------------------------------
class BwdOut:
    def __init__(self, gpu, m, c, with_dx=True):
        self.dg, self.db, self.dx = Guarded(gpu, 1, c), Guarded(gpu, 1, c), Guarded(gpu, m, c)
        self.with_dx = with_dx

    def dx_ptr(self):
        return self.dx.ptr() if self.with_dx else None

    def done(self, what):
        for n in ("dg", "db", "dx"):
            getattr(self, n).intact(f"{what} {n}")
        if not self.with_dx:
            assert bool(self.dx.cpu().isnan().all()), f"{what}: dx written although NULL was passed"

    def cpu(self, n):
        g = getattr(self, n)
        return g.cpu() if n == "dx" else g.cpu().view(-1)


def _bwd(gpu, gy, x, mean32, inv32, gamma, entry="bwd", keep=None, with_dx=True):
    m, c = x.shape
    t = [v.to(gpu) for v in (gy, x, mean32, inv32, gamma)]
    o = BwdOut(gpu, m, c, with_dx)
    lib, sh = L.lib(), L.stream_handle()
    if entry == "bwd":
        st = lib.tspm_bn1d_bwd(m, c, *[v.data_ptr() for v in t], o.dg.ptr(), o.db.ptr(), o.dx_ptr(), sh)
    else:
        kd = keep.to(gpu) if keep is not None else None
        st = lib.tspm_bn1d_bwd_drop_relu(m, c, t[0].data_ptr(), L.ptr(kd), SCALE, *[v.data_ptr() for v in t[1:]],
                                         o.dg.ptr(), o.db.ptr(), o.dx_ptr(), sh)
    L.check(st, "bn1d_" + entry)
    _sync()
    o.done("bn1d_" + entry)
    return o


def _check_bwd(name, tag, o, b):
    R.check(f"{name}.dgamma[{tag}]", o.cpu("dg"), b["dgamma"], b["tol_dgamma"])
    R.check(f"{name}.dbeta[{tag}]", o.cpu("db"), b["dbeta"], b["tol_dbeta"])
    if o.with_dx:
        R.check(f"{name}.dx[{tag}]", o.cpu("dx"), b["dx"], b["tol_dx"])


@pytest.mark.parametrize("m,c", SHAPES)
@pytest.mark.parametrize("kind", ["a", "b", "c"])
def test_bn1d_bwd(gpu, m, c, kind):
    x, gamma, beta, rm, rv, gy, keep = _data(m, c, kind)
    tag = f"m{m} c{c} {kind}"
    f = R.bn1d_fwd_ref(x, gamma, beta, None, None, MOM, EPS)
    mean32, inv32 = f["mean"].float(), f["invstd"].float()
    b = R.bn1d_bwd_ref(gy, x, mean32, inv32, gamma)
    full = _bwd(gpu, gy, x, mean32, inv32, gamma)
    _check_bwd("bn1d_bwd", tag, full, b)
    if kind == "c":
        assert full.cpu("dg")[c // 2] == 0
    # dx NULL (the monomodal path: the input needs no gradient): dgamma / dbeta are still written, the same bits
    nodx = _bwd(gpu, gy, x, mean32, inv32, gamma, with_dx=False)
    assert _bits_equal(nodx.cpu("dg"), full.cpu("dg")) and _bits_equal(nodx.cpu("db"), full.cpu("db"))


@pytest.mark.parametrize("m,c", SHAPES)
@pytest.mark.parametrize("kind", ["a", "b", "c"])
def test_bn1d_bwd_drop_relu(gpu, m, c, kind):
    x, gamma, beta, rm, rv, gy, keep = _data(m, c, kind, relu_input=True)
    if (kind == "a" or (kind == "c" and c > 1)) and m * c >= 32:
        assert bool((x == 0).any()) and bool((x > 0).any())
    tag = f"m{m} c{c} {kind}"
    f = R.bn1d_fwd_ref(x, gamma, beta, None, None, MOM, EPS)
    mean32, inv32 = f["mean"].float(), f["invstd"].float()
    for kp in (keep, None):
        b = R.bn1d_bwd_ref(gy, x, mean32, inv32, gamma, kp, SCALE, relu_x=True)
        o = _bwd(gpu, gy, x, mean32, inv32, gamma, "bwd_drop_relu", kp)
        _check_bwd("bn1d_bwd_drop_relu", f"{tag} keep{int(kp is not None)}", o, b)
        assert bool((o.cpu("dx")[x <= 0] == 0).all())
        if kind == "c":  # the dead channel: dgamma = 0, dx = 0, dbeta still the sum of the incoming gradient
            assert o.cpu("dg")[0] == 0 and bool((o.cpu("dx")[:, 0] == 0).all())
        nodx = _bwd(gpu, gy, x, mean32, inv32, gamma, "bwd_drop_relu", kp, with_dx=False)
        assert _bits_equal(nodx.cpu("dg"), o.cpu("dg")) and _bits_equal(nodx.cpu("db"), o.cpu("db"))


# ------------------------------------------------------------------------------------------------
# two BatchNorm1d layers over the same rows in one launch
# ------------------------------------------------------------------------------------------------
PAIR_C = [(33, 1), (32, 68), (1, 33)]
MOM1 = torch.tensor(0.25, dtype=torch.float32).item()
EPS1 = torch.tensor(1e-3, dtype=torch.float32).item()   # the halves' eps and momentum differ


@pytest.mark.parametrize("c0,c1", PAIR_C)
@pytest.mark.parametrize("m,kind", [(33, "a"), (4, "b"), (65, "c")])
def test_bn1d_fwd_pair(gpu, m, c0, c1, kind):
    d0, d1 = _data(m, c0, kind, seed=1), _data(m, c1, kind, seed=2)
    run1 = c0 > c1  # running statistics on both halves, or (second case) on the first half only
    halves = [(d0, MOM, EPS, True), (d1, MOM1, EPS1, run1)]
    single = [_fwd(gpu, d[0], d[1], d[2], d[3] if run else None, d[4] if run else None, mom=mo, eps=ep)
              for d, mo, ep, run in halves]
    outs = [FwdOut(gpu, m, d[0].shape[1], d[3] if run else None, d[4] if run else None) for d, mo, ep, run in halves]
    dev = [[t.to(gpu) for t in d[:3]] for d, _, _, _ in halves]
    args = []
    for (d, mo, ep, run), o, t in zip(halves, outs, dev):
        args += [d[0].shape[1], t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), *o.args(), mo, ep, o.mean.ptr(),
                 o.inv.ptr(), o.y.ptr()]
    L.check(L.lib().tspm_bn1d_fwd_pair(m, *args, L.stream_handle()), "bn1d_fwd_pair")
    _sync()
    for i, ((d, mo, ep, run), o, s) in enumerate(zip(halves, outs, single)):
        o.done(f"bn1d_fwd_pair half {i}")
        for n in ("y", "mean", "inv") + (("rm", "rv") if run else ()):
            assert _bits_equal(o.cpu(n), s.cpu(n)), f"half {i}: {n} differs from the single launch"
        f = R.bn1d_fwd_ref(d[0], d[1], d[2], d[3] if run else None, d[4] if run else None, mo, ep)
        _check_fwd("bn1d_fwd_pair", f"m{m} c{d[0].shape[1]} {kind} half{i}", o, f)


@pytest.mark.parametrize("c0,c1", PAIR_C)
@pytest.mark.parametrize("m,kind,dx_given", [(33, "a", (True, True)), (4, "b", (False, True)), (65, "c", (True, False)),
                                             (2, "a", (False, False))])
def test_bn1d_bwd_pair(gpu, m, c0, c1, kind, dx_given):
    ds = [_data(m, c0, kind, seed=3), _data(m, c1, kind, seed=4)]
    stats = []
    for d, ep in zip(ds, (EPS, EPS1)):
        f = R.bn1d_fwd_ref(d[0], d[1], d[2], None, None, MOM, ep)
        stats.append((f["mean"].float(), f["invstd"].float()))
    single = [_bwd(gpu, d[5], d[0], mu, iv, d[1], with_dx=dx) for d, (mu, iv), dx in zip(ds, stats, dx_given)]
    outs = [BwdOut(gpu, m, d[0].shape[1], dx) for d, dx in zip(ds, dx_given)]
    dev = [[t.to(gpu) for t in (d[5], d[0], mu, iv, d[1])] for d, (mu, iv) in zip(ds, stats)]
    args = []
    for d, o, t in zip(ds, outs, dev):
        args += [d[0].shape[1], *[v.data_ptr() for v in t], o.dg.ptr(), o.db.ptr(), o.dx_ptr()]
    L.check(L.lib().tspm_bn1d_bwd_pair(m, *args, L.stream_handle()), "bn1d_bwd_pair")
    _sync()
    for i, (d, (mu, iv), o, s) in enumerate(zip(ds, stats, outs, single)):
        o.done(f"bn1d_bwd_pair half {i}")
        for n in ("dg", "db") + (("dx",) if o.with_dx else ()):
            assert _bits_equal(o.cpu(n), s.cpu(n)), f"half {i}: {n} differs from the single launch"
        _check_bwd("bn1d_bwd_pair", f"m{m} c{d[0].shape[1]} {kind} half{i}", o, R.bn1d_bwd_ref(d[5], d[0], mu, iv, d[1]))


def test_bn1d_refusals(gpu):
    """m or c of 0 and a missing required pointer are refused before any launch."""
    x, gamma, beta, rm, rv, gy, keep = _data(4, 3, "a")
    t = [v.to(gpu) for v in (x, gamma, beta, gy)]
    o, b = FwdOut(gpu, 4, 3, rm, rv), BwdOut(gpu, 4, 3)
    lib, sh = L.lib(), L.stream_handle()
    xp, gp, bp, gyp = (v.data_ptr() for v in t)
    assert lib.tspm_bn1d_fwd(0, 3, xp, gp, bp, *o.args(), MOM, EPS, o.mean.ptr(), o.inv.ptr(), o.y.ptr(), sh) == INVALID
    assert lib.tspm_bn1d_fwd(4, 3, xp, gp, bp, *o.args(), MOM, EPS, None, o.inv.ptr(), o.y.ptr(), sh) == INVALID
    assert lib.tspm_bn1d_fwd_drop(4, 0, xp, gp, bp, *o.args(), MOM, EPS, o.mean.ptr(), o.inv.ptr(), None, SCALE,
                                  o.y.ptr(), sh) == INVALID
    assert lib.tspm_bn1d_bwd(4, 3, gyp, xp, gp, gp, gp, None, b.db.ptr(), b.dx.ptr(), sh) == INVALID
    assert lib.tspm_bn1d_bwd_drop_relu(4, 3, gyp, None, SCALE, xp, gp, gp, gp, b.dg.ptr(), None, b.dx.ptr(), sh) == INVALID
    _sync()
    o.done("refused bn1d_fwd"); b.done("refused bn1d_bwd")
    assert bool(o.cpu("y").isnan().all()) and bool(b.cpu("dx").isnan().all()) and bool(b.cpu("dg").isnan().all())
