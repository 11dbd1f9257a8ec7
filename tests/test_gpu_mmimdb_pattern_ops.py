"""The two entry points of the all-pattern MMIMDb eval pass through the C ABI.

``tspm_gmu_pattern_fwd``: bitwise ``tspm_gmu_fwd`` on the rows expanded with torch indexing (gate, z and h), the fp64
restatement with its fp32 run as yardstick (tests/parity.py ``op_check``), bitwise row independence (a row's z from a
sub-batch, a permuted batch and another pattern set), wide leading dimensions on guarded outputs, NULL h / gate / u0.
The widths cover every path of the mix loop, which the compiler unrolls by two with a one-trip remainder: one trip per
thread (d = 4, 68), one or two (260), exactly two (512), three or four (772).

``tspm_bce_logits_patterns``: bitwise P calls of ``tspm_bce_logits`` (loss and stats, accumulated over two calls), the
log entries and counters with ``log_capacity`` cutting the second call's entries, and two calls bitwise equal."""
import ctypes

import pytest
import torch

from parity import Guarded, Ratios, op_check
from tspm_amd import _lib as L

pytestmark = pytest.mark.gpu

RATIOS = Ratios()
KEEP = {"it": (1, 1), "i": (1, 0), "t": (0, 1)}
GRID_CAP = 1024  # csrc/mmimdb.hip kGmuPatternGrid: above it a workgroup walks several samples
SHAPES = [(1, 4), (3, 68), (5, 260), (8, 512), (2, 772), (GRID_CAP + 6, 4)]
PATTERN_SETS = [("it", "i", "t"), ("t",), ("i", "it")]


def _same(a, b):
    return torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


def _inputs(B, d, dev):
    g = torch.Generator().manual_seed(B * 1009 + d)
    u = torch.randn(B, 2 * d, generator=g) * 1.5
    u0 = torch.randn(2 * d, generator=g) * 1.5
    wz = torch.randn(2 * d, generator=g) * (0.5 / d ** 0.5)
    return u.to(dev), u0.to(dev), wz.to(dev)


def _expand(u, u0, pats):
    """[P*B, 2d]: row p*B + b takes each half from u[b] or u0 (torch indexing)."""
    B, d = u.shape[0], u.shape[1] // 2
    rows = []
    for p in pats:
        ki, kt = KEEP[p]
        rows.append(torch.cat([u[:, :d] if ki else u0[:d].expand(B, d), u[:, d:] if kt else u0[d:].expand(B, d)], dim=1))
    return torch.cat(rows).contiguous()


def _keep_arr(pats):
    return (ctypes.c_int32 * (2 * len(pats)))(*[k for p in pats for k in KEEP[p]])


def _pattern_fwd(dev, u, u0, wz, pats, ldu=None, pad_h=0, pad_z=0, with_h=True, with_gate=True):
    B, d, P = u.shape[0], u.shape[1] // 2, len(pats)
    if ldu is not None:
        wide = torch.full((B, ldu), float("nan"), device=dev)
        wide[:, :2 * d] = u
        u_arg, ldu_arg = wide, ldu
    else:
        u_arg, ldu_arg = u, 2 * d
    h = Guarded(dev, P * B, 2 * d, 2 * d + pad_h)
    gate = Guarded(dev, P * B, 1)
    z = Guarded(dev, P * B, d, d + pad_z)
    L.check(L.lib().tspm_gmu_pattern_fwd(B, P, _keep_arr(pats), d, u_arg.data_ptr(), ldu_arg,
                                         u0.data_ptr() if u0 is not None else None, wz.data_ptr(),
                                         h.ptr() if with_h else None, h.ld, gate.ptr() if with_gate else None, z.ptr(),
                                         z.ld, L.stream_handle()), "gmu_pattern_fwd")
    torch.cuda.synchronize()
    h.intact("gmu_pattern h"); gate.intact("gmu_pattern gate"); z.intact("gmu_pattern z")
    return h, gate, z


def _gmu_fwd(dev, x, wz):
    n, d = x.shape[0], x.shape[1] // 2
    h, gate, z = torch.empty(n, 2 * d, device=dev), torch.empty(n, device=dev), torch.empty(n, d, device=dev)
    L.check(L.lib().tspm_gmu_fwd(n, d, x.data_ptr(), 2 * d, wz.data_ptr(), h.data_ptr(), 2 * d, gate.data_ptr(),
                                 z.data_ptr(), d, L.stream_handle()), "gmu_fwd")
    torch.cuda.synchronize()
    return h, gate, z


def _restate(x, wz, dtype):
    x, wz = x.cpu().to(dtype), wz.cpu().to(dtype)
    d = x.shape[1] // 2
    h = torch.tanh(x)
    g = torch.sigmoid(h @ wz)
    return h, g, g[:, None] * h[:, :d] + (1 - g[:, None]) * h[:, d:]


@pytest.mark.parametrize("pats", PATTERN_SETS, ids=["+".join(p) for p in PATTERN_SETS])
@pytest.mark.parametrize("B,d", SHAPES)
def test_gmu_pattern_fwd_bitwise_and_vs_fp64(gpu, B, d, pats):
    u, u0, wz = _inputs(B, d, gpu)
    h, gate, z = _pattern_fwd(gpu, u, u0, wz, pats, ldu=2 * d + 12, pad_h=8, pad_z=4)
    x = _expand(u, u0, pats)
    h_ref, gate_ref, z_ref = _gmu_fwd(gpu, x, wz)
    assert _same(z.t, z_ref), "z differs from tspm_gmu_fwd on the expanded rows"
    assert _same(gate.t.reshape(-1), gate_ref) and _same(h.t, h_ref)
    tag = f"B{B} d{d} {'+'.join(pats)}"
    (h32, g32, z32), (h64, g64, z64) = _restate(x, wz, torch.float32), _restate(x, wz, torch.float64)
    op_check(f"gmu_pattern.z[{tag}]", z.cpu(), z32, z64, ratios=RATIOS)
    op_check(f"gmu_pattern.gate[{tag}]", gate.cpu().reshape(-1), g32, g64, ratios=RATIOS)
    op_check(f"gmu_pattern.h[{tag}]", h.cpu(), h32, h64, ratios=RATIOS)
    # eval's form: no h, no gate — the same z, the guarded h / gate buffers untouched
    h2, gate2, z2 = _pattern_fwd(gpu, u, u0, wz, pats, with_h=False, with_gate=False)
    assert _same(z2.t, z_ref)
    sentinel = Guarded(gpu, 1, 1).flat[:1].view(torch.int32).item()
    assert bool((h2.flat.view(torch.int32) == sentinel).all()) and bool((gate2.flat.view(torch.int32) == sentinel).all())


@pytest.mark.parametrize("B,d", SHAPES[:5])
def test_gmu_pattern_fwd_every_pattern_kept_needs_no_zero_row(gpu, B, d):
    u, u0, wz = _inputs(B, d, gpu)
    _, gate, z = _pattern_fwd(gpu, u, None, wz, ("it",))
    _, gate_ref, z_ref = _gmu_fwd(gpu, u, wz)
    assert _same(z.t, z_ref) and _same(gate.t.reshape(-1), gate_ref)


@pytest.mark.parametrize("B,d", [(5, 260), (8, 512), (GRID_CAP + 6, 4)])
def test_gmu_pattern_fwd_rows_are_independent(gpu, B, d):
    """A row's z depends on u[b], u0, wz and keep[p] only: the same bits from a sub-batch, a permuted batch and another
    pattern set."""
    u, u0, wz = _inputs(B, d, gpu)
    pats = ("it", "i", "t")
    z = _pattern_fwd(gpu, u, u0, wz, pats)[2].t.reshape(3, B, d)
    sub = _pattern_fwd(gpu, u[1:3].contiguous(), u0, wz, pats)[2].t.reshape(3, 2, d)
    assert _same(sub, z[:, 1:3])
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(B))
    zp = _pattern_fwd(gpu, u[perm.to(gpu)].contiguous(), u0, wz, pats)[2].t.reshape(3, B, d)
    assert _same(zp, z[:, perm.to(gpu)])
    other = _pattern_fwd(gpu, u, u0, wz, ("t", "it"))[2].t.reshape(2, B, d)
    assert _same(other[0], z[2]) and _same(other[1], z[0])


# ------------------------------------------------------------------------------------------------
# tspm_bce_logits_patterns
# ------------------------------------------------------------------------------------------------
def _bce_inputs(B, C, P, seed=0):
    g = torch.Generator().manual_seed(B * 131 + C * 7 + P + seed)
    x = torch.randn(P * B, C, generator=g) * 3
    t = (torch.rand(B, C, generator=g) > 0.6).float()
    return x, t


def _bce_each(dev, x, t, P, gs, thr, stats):
    """P calls of tspm_bce_logits on the row slices; stats [P, 3+3C] accumulated into."""
    B, C = t.shape
    loss = torch.zeros(P, device=dev)
    for p in range(P):
        L.check(L.lib().tspm_bce_logits(B, C, x[p * B:(p + 1) * B].data_ptr(), t.data_ptr(), loss[p:p + 1].data_ptr(),
                                        None, gs, thr, stats[p].data_ptr(), L.stream_handle()), "bce_logits")
    torch.cuda.synchronize()
    return loss


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("B,C", [(1, 1), (3, 23), (64, 23), (1030, 5)])
def test_bce_logits_patterns_bitwise_and_log(gpu, B, C, P):
    gs, thr, W = 0.5, 0.5, 3 + 3 * C
    cap = 2 * P - 1 if P > 1 else 1  # cuts the second call's entries (P = 1: all of them)
    stats = Guarded(gpu, P, W)
    stats.t.zero_()
    stats_ref = torch.zeros(P, W, device=gpu)
    log = Guarded(gpu, 1, cap)
    counters = torch.tensor([0, 0], dtype=torch.int64, device=gpu)
    losses = []
    for call in range(2):  # stats accumulate over two calls on different logits
        x, t = _bce_inputs(B, C, P, seed=call)
        xd, td = x.to(gpu), t.to(gpu)
        loss = Guarded(gpu, 1, P)
        args = (B, P, C, xd.data_ptr(), td.data_ptr(), gs, thr, loss.ptr(), stats.ptr(), log.ptr(), counters.data_ptr(),
                cap, L.stream_handle())
        L.check(L.lib().tspm_bce_logits_patterns(*args), "bce_logits_patterns")
        torch.cuda.synchronize()
        loss.intact("bce_patterns loss")
        want = _bce_each(gpu, xd, td, P, gs, thr, stats_ref)
        assert _same(loss.t.reshape(-1), want), "loss differs from P calls of tspm_bce_logits"
        assert _same(stats.flat[:P * W].view(P, W), stats_ref), "stats differ from P calls of tspm_bce_logits"
        losses.append(loss.t.reshape(-1).clone())
        if call == 1:  # the same inputs again, into fresh outputs: bitwise the same loss
            again = Guarded(gpu, 1, P)
            L.check(L.lib().tspm_bce_logits_patterns(B, P, C, xd.data_ptr(), td.data_ptr(), gs, thr, again.ptr(), None,
                                                     None, None, 0, L.stream_handle()), "bce_logits_patterns")
            torch.cuda.synchronize()
            assert _same(again.t, loss.t)
    log.intact("bce_patterns loss log"); stats.intact("bce_patterns stats")
    assert counters.cpu().tolist() == [2 * P, 2 * P * B]
    entries = torch.cat(losses)[:cap]  # entry k = call k // P, pattern k % P, for every index below the capacity
    assert _same(log.t.reshape(-1), entries)
    assert float(stats_ref[:, 1].min()) == 2 * B


def test_bce_logits_patterns_without_counters_or_stats(gpu):
    B, C, P = 3, 23, 3
    x, t = _bce_inputs(B, C, P)
    xd, td = x.to(gpu), t.to(gpu)
    loss = Guarded(gpu, 1, P)
    L.check(L.lib().tspm_bce_logits_patterns(B, P, C, xd.data_ptr(), td.data_ptr(), 1.0, 0.5, loss.ptr(), None, None,
                                             None, 0, L.stream_handle()), "bce_logits_patterns")
    torch.cuda.synchronize()
    loss.intact("bce_patterns loss")
    want = _bce_each(gpu, xd, td, P, 1.0, 0.5, torch.zeros(P, 3 + 3 * C, device=gpu))
    assert _same(loss.t.reshape(-1), want)
    l64 = torch.stack([torch.nn.functional.binary_cross_entropy_with_logits(x[p * B:(p + 1) * B].double(), t.double())
                       for p in range(P)])
    l32 = torch.stack([torch.nn.functional.binary_cross_entropy_with_logits(x[p * B:(p + 1) * B], t) for p in range(P)])
    op_check("bce_patterns.loss", loss.cpu().reshape(-1), l32, l64, ratios=RATIOS)


def test_zz_ratios(gpu):
    print("worst err_ours / err_ref32:", RATIOS)
