"""tspm_attn_pool_fwd / tspm_attn_pool_bwd — the attention pooling of LSTMEncoder(embd_method="attention") — and
tspm_lstm_bwd_seq — the backward recurrence with a gradient at every step — through the C ABI.

Reference: tests/attn_ref.py (``attn_pool`` on the same float32 pre-activation the kernel is handed) in float32 and
float64, gradients by autograd; for the recurrence ``test_gpu_lstm_len.len_cell_loop`` with
loss = sum(dseq * h) + sum(wt * (dh . h)).  Criterion (tests/parity.py): err_ours <= FACTOR x err_ref32 + floor against
float64; what is stated exact (the +0.0 tails, "unit" weights of exactly 1, padding independence, two descriptors against
single calls, determinism, the recurrence without dseq / wt against tspm_lstm_bwd_len) by torch.equal.  Every output is a
parity.Guarded buffer that starts as a NaN sentinel: required writes are proven written, stray writes are caught.

Shapes: H in {4, 36, 64, 128} (one per recurrence tier plus the compile-time kind; below, at and above one wave of
units), B = 5, T = 9, lengths (9, 1, 4, 4, 7) (a length-1 row, mixed lengths); T = 300 (more steps than a workgroup has
threads) with lengths (300, 257, 64).  Regime "wide" scales u until the scores span more than +-100: exp overflows
float32 without the max subtraction.
"""
import functools

import pytest
import torch

import attn_ref as R
from parity import Guarded, Ratios, op_check
from test_gpu_lstm_len import (LENS, B5, T9, WIDTHS, _is_pos_zero, _run_bwd_len, _run_fwd_len, clamp_lengths, last_of,
                               len_cell_loop)
from test_gpu_lstm_widths import _lstm_case
from test_gpu_seq_ops import _same, _sync
from tspm_amd import _lib as L

pytestmark = pytest.mark.gpu
RATIOS = Ratios()
LONG = (36, 3, 300, (300, 257, 64))  # H, B, T, lengths


# ------------------------------------------------------------------------------------------------
# cases and references
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pool_case(H, B, T, lengths, regime="a", seed=0):
    g = torch.Generator().manual_seed(seed + H)
    k = 1.0 / H ** 0.5
    r = torch.tanh(torch.randn(T, B, H, generator=g))                      # LSTM outputs lie in (-1, 1)
    W, c = (torch.rand(H, H, generator=g) * 2 - 1) * k, (torch.rand(H, generator=g) * 2 - 1) * k
    u = (torch.rand(H, generator=g) * 2 - 1) * k
    if regime == "wide":
        W, u = W * 4, u * 400 * H ** 0.5
    p = (r.double().reshape(T * B, H) @ W.double().T + c.double()).float().reshape(T, B, H).contiguous()
    gout = torch.randn(B, H, generator=g)
    ref = {}
    for norm in R.NORMS:
        for dt in (torch.float32, torch.float64):
            pl = p.to(dt).clone().requires_grad_(True)
            ul = u.to(dt).clone().requires_grad_(True)
            e, a, z = R.attn_pool(r.to(dt), None, None, ul, lengths, norm, p=pl)
            if e.requires_grad:  # "unit": nothing reaches p or u
                (gout.to(dt) * e).sum().backward()
            dp = pl.grad if pl.grad is not None else torch.zeros_like(pl)
            du = ul.grad if ul.grad is not None else torch.zeros_like(ul)
            r2, Wd = r.to(dt).reshape(T * B, H), W.to(dt)
            dp2 = dp.reshape(T * B, H)
            ref[norm, dt] = dict(e=e.detach(), alpha=a.detach(), z=z.detach(), dp=dp, du=du, dW=dp2.T @ r2,
                                 dc=dp2.sum(0), dseq=(dp2 @ Wd).reshape(T, B, H))
    if regime == "wide":
        s = ref["time", torch.float64]["z"] @ u.double()
        assert s.max().item() > 100 and s.min().item() < -100
    return dict(H=H, B=B, T=T, lengths=tuple(lengths), r=r, p=p, W=W, c=c, u=u, g=gout, ref=ref)


class _Pool:
    """Device buffers of one forward descriptor (guarded outputs); ``poison``: NaN in r and p past each row's length."""

    def __init__(self, gpu, case, norm, ld=None, poison=False, rows=None, steps=None):
        B, T, H = case["B"], case["T"], case["H"]
        r, p, lens = case["r"], case["p"], list(case["lengths"])
        if rows is not None:  # one row alone at its own length
            r, p, lens, B, T = r[:steps, rows:rows + 1].contiguous(), p[:steps, rows:rows + 1].contiguous(), [steps], 1, steps
        self.B, self.T, self.H, self.norm, self.ld = B, T, H, norm, ld or H
        r, p = r.clone(), p.clone()
        self.valid = (torch.arange(T).view(T, 1) < torch.tensor(clamp_lengths(lens, T)).view(1, B)).unsqueeze(2)
        if poison:
            r, p = r.masked_fill(~self.valid, float("nan")), p.masked_fill(~self.valid, float("nan"))
        self.r, self.p, self.u = r.to(gpu), p.to(gpu), case["u"].to(gpu)
        self.p_in = p
        self.lens = torch.tensor(lens, dtype=torch.int32, device=gpu)
        self.alpha, self.hout = Guarded(gpu, T, B), Guarded(gpu, B, H, self.ld)

    def desc(self):
        d = L.AttnPoolFwdDesc(self.B, self.T, self.H, self.ld, L.ATTN_NORMS[self.norm], 0)
        d.r, d.p, d.u = self.r.data_ptr(), self.p.data_ptr(), self.u.data_ptr()
        d.alpha, d.h_out, d.lengths = self.alpha.ptr(), self.hout.ptr(), self.lens.data_ptr()
        return d

    def outputs(self):
        self.alpha.intact("alpha"), self.hout.intact("h_out")
        return dict(alpha=self.alpha.cpu(), e=self.hout.cpu(), z=self.p.cpu())


def _run_pool(pools):
    descs = (L.AttnPoolFwdDesc * len(pools))(*[f.desc() for f in pools])
    L.check(L.lib().tspm_attn_pool_fwd(len(pools), descs, L.stream_handle()), "attn_pool_fwd")
    _sync()
    return [f.outputs() for f in pools]


def _check_pool(tag, case, f, o, norm):
    r32, r64 = case["ref"][norm, torch.float32], case["ref"][norm, torch.float64]
    lens = clamp_lengths(case["lengths"], case["T"])
    assert bool(o["alpha"].isfinite().all()) and bool(o["e"].isfinite().all()), tag
    op_check(f"attn_pool_fwd.e[{tag}]", o["e"], r32["e"], r64["e"], ratios=RATIOS)
    for b, Lb in enumerate(lens):
        assert _is_pos_zero(o["alpha"][Lb:, b]), f"{tag}: alpha tail of row {b}"
    if norm == "unit":
        assert torch.equal(o["alpha"], r64["alpha"].float()), f"{tag}: unit weights are exactly 1 on valid steps"
        assert _same(o["z"], f.p_in), f"{tag}: unit mode must not touch p"
        return
    op_check(f"attn_pool_fwd.alpha[{tag}]", o["alpha"], r32["alpha"], r64["alpha"], ratios=RATIOS)
    zero = torch.zeros(())
    op_check(f"attn_pool_fwd.z[{tag}]", torch.where(f.valid, o["z"], zero), r32["z"], r64["z"], ratios=RATIOS)
    assert _same(torch.where(f.valid, zero, o["z"]), torch.where(f.valid, zero, f.p_in)), f"{tag}: p past a length was written"


# ------------------------------------------------------------------------------------------------
# 1. forward against fp64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["a", "wide"])
@pytest.mark.parametrize("norm", R.NORMS)
@pytest.mark.parametrize("H", WIDTHS)
def test_pool_forward_vs_fp64(gpu, H, norm, regime):
    case = _pool_case(H, B5, T9, LENS, regime)
    tag = f"H{H} {norm} {regime}"
    f = _Pool(gpu, case, norm, ld=H + 12, poison=True)  # NaN past every length in r and p: never read
    o, = _run_pool([f])
    _check_pool(tag, case, f, o, norm)
    o2, = _run_pool([_Pool(gpu, case, norm, ld=H + 12, poison=True)])
    assert all(_same(o[k], o2[k]) for k in o), "attn_pool_fwd is not deterministic"
    print("worst ratios:", RATIOS)


# ------------------------------------------------------------------------------------------------
# 2. padding independence: a row is bitwise a B = 1, T = L_b call on that row alone
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", R.NORMS)
@pytest.mark.parametrize("shape", [(h, B5, T9, LENS) for h in WIDTHS] + [LONG], ids=lambda s: f"H{s[0]}T{s[2]}")
def test_rows_are_bitwise_their_own_unpadded_call(gpu, shape, norm):
    H, B, T, lens = shape
    case = _pool_case(H, B, T, lens)
    f = _Pool(gpu, case, norm)
    o, = _run_pool([f])
    if T > 256:
        _check_pool(f"H{H} T{T} {norm}", case, f, o, norm)
    for b, Lb in enumerate(lens):
        ob, = _run_pool([_Pool(gpu, case, norm, rows=b, steps=Lb)])
        assert torch.equal(o["alpha"][:Lb, b], ob["alpha"][:, 0]), (b, Lb)
        assert torch.equal(o["e"][b], ob["e"][0]), (b, Lb)
        if norm == "time":
            assert torch.equal(o["z"][:Lb, b], ob["z"][:, 0]), (b, Lb)


# ------------------------------------------------------------------------------------------------
# 3. backward against fp64 autograd, the GEMM that follows through the real tspm_linear_bwd call
# ------------------------------------------------------------------------------------------------
def _run_pool_bwd(gpu, case, f, o, ld_g):
    B, T, H = case["B"], case["T"], case["H"]
    g = torch.full((B, ld_g), float("nan"), device=gpu)
    g[:, :H] = case["g"].to(gpu)
    dp, du, dck = Guarded(gpu, T * B, H), Guarded(gpu, 1, H), Guarded(gpu, 1, H)
    rows = Guarded(gpu, B, 2 * H)
    d = L.AttnPoolBwdDesc(B, T, H, ld_g, 0, 0)
    d.g, d.alpha, d.z, d.r, d.u = g.data_ptr(), f.alpha.ptr(), f.p.data_ptr(), f.r.data_ptr(), f.u.data_ptr()
    d.dp, d.du, d.dc, d.rows, d.lengths = dp.ptr(), du.ptr(), dck.ptr(), rows.ptr(), f.lens.data_ptr()
    L.check(L.lib().tspm_attn_pool_bwd(1, (L.AttnPoolBwdDesc * 1)(d), L.stream_handle()), "attn_pool_bwd")
    W = case["W"].to(gpu)
    dW, dc, dseq = Guarded(gpu, H, H), Guarded(gpu, 1, H), Guarded(gpu, T * B, H)
    rz = torch.where(f.valid.to(gpu), f.r, torch.zeros((), device=gpu))  # the engine's hs rows past a length are +0.0
    L.check(L.lib().tspm_linear_bwd(T * B, H, H, rz.data_ptr(), H, dp.ptr(), H, W.data_ptr(), dW.ptr(), dc.ptr(), dseq.ptr(),
                                    H, L.stream_handle()), "linear_bwd")
    _sync()
    for n, b in (("dp", dp), ("du", du), ("dc", dck), ("rows", rows), ("dW", dW), ("gemm dc", dc), ("dseq", dseq)):
        b.intact(n)
    return dict(dp=dp.cpu().view(T, B, H), du=du.cpu().view(H), dc=dck.cpu().view(H), dW=dW.cpu(), dc_gemm=dc.cpu().view(H),
                dseq=dseq.cpu().view(T, B, H))


@pytest.mark.parametrize("shape", [(h, B5, T9, LENS) for h in WIDTHS] + [LONG], ids=lambda s: f"H{s[0]}T{s[2]}")
def test_pool_backward_vs_fp64_autograd(gpu, shape):
    """Regime "a" only: the backward takes alpha as an input and has no exponential to overflow, and under "wide" alpha
    is one-hot to rounding, where ds = alpha (a - D) is a difference of equal numbers in any float32 evaluation."""
    H, B, T, lens = shape
    case = _pool_case(H, B, T, lens)
    tag = f"H{H} T{T}"
    res = []
    for _ in range(2):
        f = _Pool(gpu, case, "time", ld=H + 4, poison=True)
        o, = _run_pool([f])
        res.append(_run_pool_bwd(gpu, case, f, o, H + 8))
    got, again = res
    assert all(torch.equal(got[k], again[k]) for k in got), "attn_pool_bwd is not deterministic"
    r32, r64 = case["ref"]["time", torch.float32], case["ref"]["time", torch.float64]
    for b, Lb in enumerate(clamp_lengths(lens, T)):
        assert _is_pos_zero(got["dp"][Lb:, b]), f"{tag}: dp tail of row {b}"
    for k in ("dp", "du", "dc", "dW", "dc_gemm", "dseq"):  # dc: the kernel's; dc_gemm: the column sums of dp
        op_check(f"attn_pool_bwd.{k}[{tag}]", got[k], r32[k.split("_")[0]], r64[k.split("_")[0]], grad=True, ratios=RATIOS)
    print("worst ratios:", RATIOS)


# ------------------------------------------------------------------------------------------------
# 4. tspm_lstm_bwd_seq
# ------------------------------------------------------------------------------------------------
class _BwdSeq:
    def __init__(self, gpu, f, dh, ld, dseq, wt):
        self.f, self.ld = f, ld
        self.dh = None
        if dh is not None:
            self.dh = torch.full((f.B, ld), float("nan"), device=gpu)  # the padding columns must never be read
            self.dh[:, :f.H] = dh.to(gpu)
        self.dseq = None if dseq is None else dseq.to(gpu).contiguous()
        self.wt = None if wt is None else wt.to(gpu).contiguous()
        self.dgates = Guarded(gpu, f.T * f.B, 4 * f.H)

    def desc(self):
        f = self.f
        return L.LstmBwdSeqDesc(f.B, f.T, f.H, self.ld, f.whh.data_ptr(), f.gates.ptr(), f.cs.ptr(), L.ptr(self.dh),
                                self.dgates.ptr(), L.ptr(self.dseq), L.ptr(self.wt), f.lengths.data_ptr())


def _run_bwd_seq(gpu, specs):
    """specs: list of (_FwdLen, dh [B,H] cpu or None, ld_dh, dseq [T,B,H] or None, wt [T,B] or None) -> dgates from ONE call."""
    bs = [_BwdSeq(gpu, *s) for s in specs]
    descs = (L.LstmBwdSeqDesc * len(bs))(*[b.desc() for b in bs])
    L.check(L.lib().tspm_lstm_bwd_seq(len(bs), descs, L.stream_handle()), "lstm_bwd_seq")
    _sync()
    for b in bs:
        b.dgates.intact(f"lstm_bwd_seq H{b.f.H} dgates")
    return [b.dgates.cpu().view(b.f.T, b.f.B, 4 * b.f.H) for b in bs]


def _seq_inputs(H, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, H, generator=g), torch.randn(T, B, H, generator=g), torch.rand(T, B, generator=g)


def _seq_ref(case, lengths, dh, dseq, wt, dtype):
    _, _, hs, leaf = len_cell_loop(case["xg"], case["whh"], case["bhh"], lengths, dtype, grad=True)
    h = hs[1:]  # zeros (constants) past each length
    loss = (dseq.to(dtype) * h).sum() if dseq is not None else 0.0
    if dh is not None and wt is not None:
        loss = loss + (wt.to(dtype).unsqueeze(2) * dh.to(dtype).unsqueeze(0) * h).sum()
    elif dh is not None:
        loss = loss + (dh.to(dtype) * last_of(hs, lengths)).sum()
    loss.backward()
    return leaf.grad


def _poison(t, T, lengths):
    valid = torch.arange(T).view(T, 1) < torch.tensor(clamp_lengths(lengths, T)).view(1, -1)
    return t.masked_fill(~(valid if t.dim() == 2 else valid.unsqueeze(2)), float("nan"))


@pytest.mark.parametrize("H", WIDTHS)
def test_bwd_seq_without_dseq_and_wt_is_bitwise_bwd_len(gpu, H):
    case = _lstm_case(H, B5, T9, "a", True)
    dh = _seq_inputs(H, B5, T9, H)[0]
    (f, _), = _run_fwd_len(gpu, [(case["xg"], case["whh"], case["bhh"], False, H, LENS)])
    want, = _run_bwd_len(gpu, [(f, dh, H + 12)])
    got, = _run_bwd_seq(gpu, [(f, dh, H + 12, None, None)])
    assert got.view(torch.int32).equal(want.view(torch.int32))


@pytest.mark.parametrize("mode", ["dseq+wt+dh", "dseq", "wt+dh", "dseq+dh"])
@pytest.mark.parametrize("H", WIDTHS)
def test_bwd_seq_vs_fp64_autograd(gpu, H, mode):
    """Random dseq, wt and dh against autograd through the cell loop; dseq / wt are NaN past each length on the device
    (never read), dgates are finite with +0.0 tails."""
    case = _lstm_case(H, B5, T9, "a", True)
    dh, dseq, wt = _seq_inputs(H, B5, T9, 100 + H)
    dh, dseq, wt = (dh if "dh" in mode else None, dseq if "dseq" in mode else None, wt if "wt" in mode else None)
    (f, _), = _run_fwd_len(gpu, [(case["xg"], case["whh"], case["bhh"], False, H, LENS)])
    spec = (f, dh, H + 4, None if dseq is None else _poison(dseq, T9, LENS), None if wt is None else _poison(wt, T9, LENS))
    got, = _run_bwd_seq(gpu, [spec])
    again, = _run_bwd_seq(gpu, [spec])
    assert torch.equal(got, again), "lstm_bwd_seq is not deterministic"
    assert bool(got.isfinite().all())
    for b, Lb in enumerate(clamp_lengths(LENS, T9)):
        assert _is_pos_zero(got[Lb:, b]), f"dgates tail of row {b}"
    r32, r64 = (_seq_ref(case, LENS, dh, dseq, wt, dt) for dt in (torch.float32, torch.float64))
    op_check(f"lstm_bwd_seq.dgates[H{H} {mode}]", got, r32, r64, grad=True, ratios=RATIOS)
    print("worst ratios:", RATIOS)


@pytest.mark.parametrize("ha,hb", [(36, 60), (64, 36), (128, 100)])
def test_bwd_seq_two_descriptors_equal_single_calls_in_both_orders(gpu, ha, hb):
    a, b = _lstm_case(ha, 5, 9, "a", True, seed=1), _lstm_case(hb, 3, 14, "a", True, seed=2)
    la, lb = (9, 1, 4, 4, 7), (2, 14, 5)
    fs = [_run_fwd_len(gpu, [(c["xg"], c["whh"], c["bhh"], False, h, ln)])[0][0] for c, h, ln in ((a, ha, la), (b, hb, lb))]
    ins = [_seq_inputs(ha, 5, 9, 7), _seq_inputs(hb, 3, 14, 8)]
    specs = [(fs[0], ins[0][0], ha + 12, ins[0][1], ins[0][2]), (fs[1], ins[1][0], hb, ins[1][1], None)]
    single = [_run_bwd_seq(gpu, [s])[0] for s in specs]
    for order in ((0, 1), (1, 0)):
        pair = _run_bwd_seq(gpu, [specs[i] for i in order])
        for g, i in zip(pair, order):
            assert torch.equal(g, single[i]), (order, i)


# ------------------------------------------------------------------------------------------------
# 5. two pool descriptors equal the single calls
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norms", [("time", "time"), ("time", "unit"), ("unit", "time")])
def test_two_pool_descriptors_equal_single_calls(gpu, norms):
    cases = [_pool_case(64, B5, T9, LENS), _pool_case(36, 3, 14, (2, 14, 5), seed=3)]
    single = [_run_pool([_Pool(gpu, c, n, ld=c["H"] + 4 * i)])[0] for i, (c, n) in enumerate(zip(cases, norms))]
    for order in ((0, 1), (1, 0)):
        pair = _run_pool([_Pool(gpu, cases[i], norms[i], ld=cases[i]["H"] + 4 * i) for i in order])
        for o, i in zip(pair, order):
            assert all(_same(o[k], single[i][k]) for k in o), (order, i)
