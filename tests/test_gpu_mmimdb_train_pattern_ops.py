"""The entry points of the all-pattern MMIMDb train step through the C ABI, each against a plain-torch restatement in
fp64 with the fp32 run of the same restatement as the yardstick (tests/parity.py ``op_check``), outputs in guarded
buffers.

``tspm_bn1d_fwd_rep`` / ``_pair``: BatchNorm1d over the explicitly replicated batch (each row ``reps`` times,
``zero_rows_per_row`` all-zero rows per row) restated with ``torch.mean`` / ``torch.var`` — y including the zero row's
row m, the saved and the running statistics; with (1, 0) bitwise ``tspm_bn1d_fwd``; the pair bitwise the two single
calls.  Shapes: fewer rows than the 32 row groups (1, 2), one more than them (33), two per group (64); c below one
workgroup's 32 channels (4), no multiple of 32 (36, 300: a ragged last workgroup), 128 workgroups (4096).

``tspm_gmu_pattern_bwd``: ds bitwise ``tspm_gmu_bwd``'s on the expanded rows; du against the fp64 restatement (autograd
through the fusion on the expanded rows, folded on the host) with ``tspm_gmu_bwd`` + the same host fold as the fp32
yardstick; a slot no pattern uses exactly +0.0; two calls bitwise equal; rows b < B independent of the rest of the
batch.  Widths: the forward's trip-count set (one trip per thread: 4, 68; one or two: 260; exactly two: 512)."""
import ctypes

import pytest
import torch

from parity import Guarded, Ratios, op_check
from tspm_amd import _lib as L

pytestmark = pytest.mark.gpu

RATIOS = Ratios()
KEEP = {"it": (1, 1), "i": (1, 0), "t": (0, 1)}
PATTERN_SETS = [("it", "i", "t"), ("t", "it"), ("it",)]
MOM, EPS = 0.1, 1e-5


def _same(a, b):
    return torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------
# tspm_bn1d_fwd_rep
# ------------------------------------------------------------------------------------------------
BN_SHAPES = [(1, 4), (2, 36), (33, 300), (64, 4096)]
BN_REPS = [(1, 0), (2, 1), (1, 2), (1, 1)]
BN_CASES = [(m, c, k, z) for m, c in BN_SHAPES for k, z in BN_REPS if (m, k, z) != (1, 1, 0)]  # one row in all: refused


def _bn_inputs(m, c, dev, seed=0):
    g = torch.Generator().manual_seed(m * 7919 + c + seed)
    x = torch.relu(torch.randn(m, c, generator=g)) + 0.25 * torch.randn(m, c, generator=g)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.2
    rm, rv = torch.randn(c, generator=g) * 0.3, torch.rand(c, generator=g) + 0.5
    return tuple(t.to(dev) for t in (x, gamma, beta, rm, rv))


def _bn_restate(x, gamma, beta, rm, rv, reps, zr, dtype):
    """BatchNorm1d in train mode over the replicated batch, built explicitly: (y [m + 1, c], mean, invstd, rm, rv)."""
    x, gamma, beta, rm, rv = (t.cpu().to(dtype) for t in (x, gamma, beta, rm, rv))
    m = x.shape[0]
    full = torch.cat([x] * reps + [torch.zeros(zr * m, x.shape[1], dtype=dtype)])
    mean, var = full.mean(0), full.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + EPS)
    y = (torch.cat([x, torch.zeros(1, x.shape[1], dtype=dtype)]) - mean) * invstd * gamma + beta
    return y, mean, invstd, (1 - MOM) * rm + MOM * mean, (1 - MOM) * rv + MOM * full.var(0, unbiased=True)


def _bn_rep_args(dev, m, c, x, gamma, beta, rm, rv, reps, zr):
    out = dict(rm=Guarded(dev, 1, c), rv=Guarded(dev, 1, c), mean=Guarded(dev, 1, c), inv=Guarded(dev, 1, c),
               y=Guarded(dev, m + 1, c))
    out["rm"].t.copy_(rm.view(1, c))
    out["rv"].t.copy_(rv.view(1, c))
    args = [c, x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out["rm"].ptr(), out["rv"].ptr(), MOM, EPS,
            out["mean"].ptr(), out["inv"].ptr(), out["y"].ptr(), reps, zr]
    return out, args


def _bn_rep(dev, m, c, x, gamma, beta, rm, rv, reps, zr):
    out, args = _bn_rep_args(dev, m, c, x, gamma, beta, rm, rv, reps, zr)
    L.check(L.lib().tspm_bn1d_fwd_rep(m, *args, L.stream_handle()), "bn1d_fwd_rep")
    torch.cuda.synchronize()
    for k, v in out.items():
        v.intact(f"bn1d_fwd_rep {k}")
    return out


@pytest.mark.parametrize("m,c,reps,zr", BN_CASES)
def test_bn1d_fwd_rep_vs_fp64(gpu, m, c, reps, zr):
    inp = _bn_inputs(m, c, gpu)
    out = _bn_rep(gpu, m, c, *inp, reps, zr)
    r32, r64 = _bn_restate(*inp, reps, zr, torch.float32), _bn_restate(*inp, reps, zr, torch.float64)
    tag = f"m{m} c{c} k{reps} z{zr}"
    for i, (name, key) in enumerate((("y", "y"), ("save_mean", "mean"), ("save_invstd", "inv"), ("running_mean", "rm"),
                                     ("running_var", "rv"))):
        ours = out[key].cpu() if key == "y" else out[key].cpu().reshape(-1)
        op_check(f"bn1d_fwd_rep.{name}[{tag}]", ours, r32[i], r64[i], ratios=RATIOS)
    op_check(f"bn1d_fwd_rep.zero_row[{tag}]", out["y"].cpu()[m], r32[0][m], r64[0][m], ratios=RATIOS)


@pytest.mark.parametrize("m,c", BN_SHAPES[1:])
def test_bn1d_fwd_rep_once_is_bn1d_fwd_bitwise(gpu, m, c):
    """reps = 1 and no zero rows: rows [0, m), the saved and the running statistics are tspm_bn1d_fwd's, bit for bit."""
    x, gamma, beta, rm, rv = _bn_inputs(m, c, gpu)
    out = _bn_rep(gpu, m, c, x, gamma, beta, rm, rv, 1, 0)
    rm2, rv2 = rm.clone(), rv.clone()
    mean, inv, y = torch.empty(c, device=gpu), torch.empty(c, device=gpu), torch.empty(m, c, device=gpu)
    L.check(L.lib().tspm_bn1d_fwd(m, c, x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rm2.data_ptr(), rv2.data_ptr(),
                                  MOM, EPS, mean.data_ptr(), inv.data_ptr(), y.data_ptr(), L.stream_handle()),
            "bn1d_fwd")
    torch.cuda.synchronize()
    assert _same(out["y"].t[:m], y)
    assert _same(out["mean"].t.reshape(-1), mean) and _same(out["inv"].t.reshape(-1), inv)
    assert _same(out["rm"].t.reshape(-1), rm2) and _same(out["rv"].t.reshape(-1), rv2)


@pytest.mark.parametrize("m,c,reps,zr", [(1, 4, 1, 2), (2, 36, 2, 1), (33, 300, 1, 1), (64, 4096, 2, 1)])
def test_bn1d_fwd_rep_pair_is_two_calls_bitwise(gpu, m, c, reps, zr):
    """The pair form: each half with its own width and replication, bitwise the single call (the other half: 300
    channels kept by every one of two patterns)."""
    a = _bn_inputs(m, c, gpu)
    b = _bn_inputs(m, 300, gpu, seed=5)
    one_a, one_b = _bn_rep(gpu, m, c, *a, reps, zr), _bn_rep(gpu, m, 300, *b, 2, 0)
    out_a, args_a = _bn_rep_args(gpu, m, c, *a, reps, zr)
    out_b, args_b = _bn_rep_args(gpu, m, 300, *b, 2, 0)
    L.check(L.lib().tspm_bn1d_fwd_rep_pair(m, *args_a, *args_b, L.stream_handle()), "bn1d_fwd_rep_pair")
    torch.cuda.synchronize()
    for one, two in ((one_a, out_a), (one_b, out_b)):
        for k in one:
            two[k].intact(f"bn1d_fwd_rep_pair {k}")
            assert _same(one[k].t, two[k].t), k


# ------------------------------------------------------------------------------------------------
# tspm_gmu_pattern_bwd
# ------------------------------------------------------------------------------------------------
def _keep_arr(pats):
    return (ctypes.c_int32 * (2 * len(pats)))(*[k for p in pats for k in KEEP[p]])


def _gmu_inputs(B, d, P, dev):
    g = torch.Generator().manual_seed(B * 1009 + d * 3 + P)
    u = torch.randn(B, 2 * d, generator=g) * 1.5
    u0 = torch.randn(2 * d, generator=g) * 1.5
    wz = torch.randn(2 * d, generator=g) * (0.5 / d ** 0.5)
    dz = torch.randn(P * B, d, generator=g)
    return u.to(dev), u0.to(dev), wz.to(dev), dz.to(dev)


def _expand(u, u0, pats):
    """[P*B, 2d]: row p*B + b takes each half from u[b] or u0 (torch indexing)."""
    B, d = u.shape[0], u.shape[1] // 2
    rows = []
    for p in pats:
        ki, kt = KEEP[p]
        rows.append(torch.cat([u[:, :d] if ki else u0[:d].expand(B, d), u[:, d:] if kt else u0[d:].expand(B, d)], dim=1))
    return torch.cat(rows).contiguous()


def _fold(du_rows, B, pats):
    """[P*B, 2d] -> [B + 1, 2d]: per half, row b sums the patterns that keep it in ascending p from +0.0, row B every
    sample under every pattern that drops it (torch's sum: the order is the kernel's own business)."""
    d = du_rows.shape[1] // 2
    out = torch.zeros(B + 1, 2 * d, dtype=du_rows.dtype)
    for pi, p in enumerate(pats):
        gp = du_rows[pi * B:(pi + 1) * B]
        for half, kept in ((slice(0, d), KEEP[p][0]), (slice(d, 2 * d), KEEP[p][1])):
            if kept:
                out[:B, half] += gp[:, half]
            else:
                out[B, half] += gp[:, half].sum(0)
    return out


def _pattern_fwd(dev, u, u0, wz, pats):
    """h, gate as the step's forward leaves them (tspm_gmu_pattern_fwd with h and gate given)."""
    B, d, P = u.shape[0], u.shape[1] // 2, len(pats)
    h, gate, z = torch.empty(P * B, 2 * d, device=dev), torch.empty(P * B, device=dev), torch.empty(P * B, d, device=dev)
    L.check(L.lib().tspm_gmu_pattern_fwd(B, P, _keep_arr(pats), d, u.data_ptr(), 2 * d, u0.data_ptr(), wz.data_ptr(),
                                         h.data_ptr(), 2 * d, gate.data_ptr(), z.data_ptr(), d, L.stream_handle()),
            "gmu_pattern_fwd")
    return h, gate


def _pattern_bwd(dev, B, d, pats, dz, h, gate, wz, pad_dz=0, pad_du=0):
    P = len(pats)
    if pad_dz:
        wide = torch.full((P * B, d + pad_dz), float("nan"), device=dev)
        wide[:, :d] = dz
        dz_arg, lddz = wide, d + pad_dz
    else:
        dz_arg, lddz = dz, d
    du, ds = Guarded(dev, B + 1, 2 * d, 2 * d + pad_du), Guarded(dev, P * B, 1)
    wsb = int(L.lib().tspm_gmu_pattern_bwd_workspace(B, d))
    ws = Guarded(dev, 1, wsb // 4)
    L.check(L.lib().tspm_gmu_pattern_bwd(B, P, _keep_arr(pats), d, dz_arg.data_ptr(), lddz, h.data_ptr(), 2 * d,
                                         gate.data_ptr(), wz.data_ptr(), du.ptr(), du.ld, ds.ptr(), ws.ptr(), wsb,
                                         L.stream_handle()), "gmu_pattern_bwd")
    torch.cuda.synchronize()
    du.intact("gmu_pattern_bwd du"); ds.intact("gmu_pattern_bwd ds"); ws.intact("gmu_pattern_bwd workspace")
    return du, ds


def _gmu_bwd_rows(dev, dz, h, gate, wz):
    n, d = dz.shape
    du, ds = torch.empty(n, 2 * d, device=dev), torch.empty(n, device=dev)
    L.check(L.lib().tspm_gmu_bwd(n, d, dz.data_ptr(), d, h.data_ptr(), 2 * d, gate.data_ptr(), wz.data_ptr(),
                                 du.data_ptr(), 2 * d, ds.data_ptr(), L.stream_handle()), "gmu_bwd")
    torch.cuda.synchronize()
    return du, ds


def _restate64(x, wz, dz):
    """(du_rows, ds) of the fusion on the expanded rows by autograd, in fp64."""
    x = x.cpu().double().requires_grad_(True)
    wz, dz = wz.cpu().double(), dz.cpu().double()
    d = dz.shape[1]
    h = torch.tanh(x)
    s = h @ wz
    s.retain_grad()
    g = torch.sigmoid(s)
    z = g[:, None] * h[:, :d] + (1 - g[:, None]) * h[:, d:]
    z.backward(dz)
    return x.grad, s.grad


@pytest.mark.parametrize("pats", PATTERN_SETS, ids=["+".join(p) for p in PATTERN_SETS])
@pytest.mark.parametrize("B", [1, 5, 64])
@pytest.mark.parametrize("d", [4, 68, 260, 512])
def test_gmu_pattern_bwd_vs_fp64(gpu, d, B, pats):
    P = len(pats)
    u, u0, wz, dz = _gmu_inputs(B, d, P, gpu)
    h, gate = _pattern_fwd(gpu, u, u0, wz, pats)
    du, ds = _pattern_bwd(gpu, B, d, pats, dz, h, gate, wz, pad_dz=4, pad_du=8)
    du_rows32, ds32 = _gmu_bwd_rows(gpu, dz, h, gate, wz)
    du_rows64, ds64 = _restate64(_expand(u, u0, pats), wz, dz)
    tag = f"B{B} d{d} {'+'.join(pats)}"
    assert _same(ds.t.reshape(-1), ds32), "ds differs from tspm_gmu_bwd on the expanded rows"
    op_check(f"gmu_pattern_bwd.ds[{tag}]", ds.cpu().reshape(-1), ds32.cpu(), ds64, grad=True, ratios=RATIOS)
    op_check(f"gmu_pattern_bwd.du[{tag}]", du.cpu(), _fold(du_rows32.cpu(), B, pats), _fold(du_rows64, B, pats),
             grad=True, ratios=RATIOS)
    # a slot no pattern uses is +0.0, bit for bit
    bits = du.t.cpu().contiguous().view(torch.int32)
    if all(KEEP[p][0] for p in pats):
        assert not bits[B, :d].any(), "the image half of the zero row: no pattern drops it"
    if all(KEEP[p][1] for p in pats):
        assert not bits[B, d:].any(), "the text half of the zero row: no pattern drops it"
    assert bool(du.t[B].abs().sum() > 0) == (pats != ("it",))
    # the same inputs again: the same bits
    du2, ds2 = _pattern_bwd(gpu, B, d, pats, dz, h, gate, wz)
    assert _same(du2.t, du.t) and _same(ds2.t, ds.t)


@pytest.mark.parametrize("pats", PATTERN_SETS[:2], ids=["+".join(p) for p in PATTERN_SETS[:2]])
@pytest.mark.parametrize("d", [4, 68, 260, 512])
def test_gmu_pattern_bwd_real_rows_are_independent(gpu, d, pats):
    """Rows b < B depend on sample b's rows only: B = 5 against its first 2 samples, bitwise (ds too)."""
    B, P = 5, len(pats)
    u, u0, wz, dz = _gmu_inputs(B, d, P, gpu)
    h, gate = _pattern_fwd(gpu, u, u0, wz, pats)
    du, ds = _pattern_bwd(gpu, B, d, pats, dz, h, gate, wz)
    sub = lambda t: t.view(P, B, -1)[:, :2].reshape(P * 2, -1).contiguous()  # noqa: E731
    du_s, ds_s = _pattern_bwd(gpu, 2, d, pats, sub(dz), sub(h), sub(gate).reshape(-1), wz)
    assert _same(du_s.t[:2], du.t[:2])
    assert _same(ds_s.t.reshape(P, 2), ds.t.reshape(P, B)[:, :2])


def test_zz_ratios(gpu):
    print("worst err_ours / err_ref32:", RATIOS)
