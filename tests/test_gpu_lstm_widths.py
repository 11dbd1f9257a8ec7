"""tspm_lstm_fwd_w / tspm_lstm_bwd_w — the LSTM recurrences at any hidden width — through the C ABI against plain-torch
restatements in float64 on the CPU, structured as test_gpu_seq_ops.py with the width H as a parameter.

Criterion (tests/parity.py): err_ours = rel-L2(ours, fp64) <= FACTOR x err_ref32 + floor, ref32 the same restatement
in float32; exact operations (the select of h_out, the first-maximum index of our own h, the zero initial state, the
zero steps of the backward) by torch.equal; argmax decisions against fp64's own, a disagreement allowed only as a rare
near-tie (near_tie_flips).  Every output is followed by a sentinel guard region and its padding columns are guards;
every kernel runs twice for bitwise determinism.

Widths: 4 (one float4 of W_hh), 32 (edge of the first tier), 36 (the first width with idle lanes, 28 of 64), 100 (idle
lanes in the top tier: 400 live gate columns of 512) and 128.  Shapes: one row, an odd batch (ghost row of the 2-row
workgroup), T = 1, the uint8 index limit T = 256 with the maximum planted at the last step of unit H-1 (the last live
lane), T = 300 without an index.

The flip cap of near_tie_flips is max(1, 1e-4 x numel).  With this generator and seed the fp32 restatement makes at
most 1 flip against fp64 on every combination below, each a near-tie <= 2e-7 x rms, except width 4 in regime "b" at
(5, 37) and (2, 256), where the fp32 reference itself flips 3 of 20 and 2 of 8 decisions (saturated h ties over many
steps): there the values and the self-consistency are checked and the flip count is left out.

One deviation from test_gpu_seq_ops.py's backward check, which takes its worst-step comparison over every live step:
here the worst-step and the step-by-step comparisons cover the steps whose fp64 gradient has rms >= 1e-30 (that
file's own threshold for its step-by-step check), and a live step below it is held to the same per-step bound plus an
absolute allowance of 2^-126 (fp32's smallest normal) x sqrt(numel).  Without it the criterion fails for correct fp32
arithmetic: at width 32, T = 300, regime "b" the first 130 steps have fp64 gradients of 1e-45 to 1e-79, the fp32
reference returns exact zeros there (relative error 1, so the bound is 4) and a result of one subnormal ulp, 1.4e-45,
against a true 1.6e-46 is a relative error of 8.  At width 64 that case happens not to arise.
"""
import functools

import pytest
import torch

from parity import FACTOR, FLOOR_GRAD, Guarded, Ratios, near_tie_flips, op_check, rel_l2
from test_gpu_seq_ops import _pool_time, _same, _sync
from tspm_amd import _lib as L

pytestmark = pytest.mark.gpu
RATIOS = Ratios()
WIDTHS = [4, 32, 36, 100, 128]
SHAPES = [(1, 1, "last"), (1, 1, "maxpool"), (3, 5, "maxpool"), (5, 37, "last"), (5, 37, "maxpool"),
          (2, 256, "maxpool"), (2, 300, "last")]
NO_FLIP_COUNT = {(4, "b", 5, 37), (4, "b", 2, 256)}  # the fp32 reference itself exceeds the cap (module docstring)


def _cell_loop(xg, whh, bhh, dtype, grad=False):
    """nn.LSTM's cell in ATen's order on the projected input (test_gpu_seq_ops._cell_loop at the width of `whh`)."""
    xg, whh = xg.to(dtype), whh.to(dtype)
    bhh = None if bhh is None else bhh.to(dtype)
    if grad:
        xg = xg.clone().requires_grad_(True)
    T, B, _ = xg.shape
    H = whh.shape[1]
    h, c = torch.zeros(B, H, dtype=dtype), torch.zeros(B, H, dtype=dtype)
    gates, cs, hs, pres = [], [], [h], []
    for t in range(T):
        rec = h @ whh.T
        if bhh is not None:
            rec = rec + bhh
        pre = rec + xg[t]
        if grad:
            pre.retain_grad()
        i, f, g, o = pre.chunk(4, 1)
        i, f, g, o = i.sigmoid(), f.sigmoid(), g.tanh(), o.sigmoid()
        c = f * c + i * g
        h = o * c.tanh()
        gates.append(torch.cat([i, f, g, o], 1)); cs.append(c); hs.append(h); pres.append(pre)
    return torch.stack(gates), torch.stack(cs), torch.stack(hs), pres


@functools.lru_cache(maxsize=None)
def _lstm_case(H, B, T, regime, with_bhh, seed=0, plant_last=False):
    """test_gpu_seq_ops._lstm_case at width H: regime 'a' nn.LSTM's default initialisation and a randn input, 'b'
    weights x8 and input x6 (saturating gates); `plant_last` shuts the output gate of unit H-1 of the last row until
    the last step, which then holds the maximum."""
    g = torch.Generator().manual_seed(seed)
    feat, G = 20, 4 * H
    k = 1.0 / H ** 0.5
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * k
    wih, whh, bih, bhh = u(G, feat), u(G, H), u(G), u(G)
    x = torch.randn(T, B, feat, generator=g)
    if regime == "b":
        wih, whh, bih, bhh, x = wih * 8, whh * 8, bih * 8, bhh * 8, x * 6
    xg = (x.reshape(T * B, feat) @ wih.T + bih).reshape(T, B, G).contiguous()
    if plant_last:
        b, un = B - 1, H - 1
        xg[:, b, 3 * H + un] = -20.0
        xg[T - 1, b, [un, H + un, 2 * H + un, 3 * H + un]] = torch.tensor([20.0, -20.0, 20.0, 20.0])
    bh = bhh if with_bhh else None
    r32 = _cell_loop(xg, whh, bh, torch.float32)[:3]
    r64 = _cell_loop(xg, whh, bh, torch.float64)[:3]
    return dict(xg=xg, whh=whh, bhh=bh, r32=r32, r64=r64, B=B, T=T, H=H)


class _Fwd:
    """Device buffers of one forward descriptor of width H (guarded outputs)."""

    def __init__(self, gpu, xg, whh, bhh, maxpool, ld):
        T, B, G = xg.shape
        H = G // 4
        self.T, self.B, self.H, self.ld, self.maxpool = T, B, H, ld, maxpool
        self.xg, self.whh = xg.to(gpu), whh.to(gpu)
        self.bhh = None if bhh is None else bhh.to(gpu)
        self.gates, self.cs = Guarded(gpu, T * B, G), Guarded(gpu, T * B, H)
        self.hs, self.hout = Guarded(gpu, (T + 1) * B, H), Guarded(gpu, B, H, ld)
        self.arg = Guarded(gpu, B, H, dtype=torch.uint8) if maxpool else None

    def desc(self):
        return L.LstmFwdDesc(self.B, self.T, self.H, self.ld, self.xg.data_ptr(), self.whh.data_ptr(), L.ptr(self.bhh),
                             self.gates.ptr(), self.cs.ptr(), self.hs.ptr(), self.hout.ptr(),
                             self.arg.ptr() if self.arg else None)

    def outputs(self):
        T, B, H = self.T, self.B, self.H
        o = dict(gates=self.gates.cpu().view(T, B, 4 * H), cs=self.cs.cpu().view(T, B, H),
                 hs=self.hs.cpu().view(T + 1, B, H), hout=self.hout.cpu())
        if self.arg:
            o["arg"] = self.arg.cpu()
        return o

    def intact(self):
        for n in ("gates", "cs", "hs", "hout", "arg"):
            if getattr(self, n) is not None:
                getattr(self, n).intact(f"lstm_fwd_w H{self.H} {n}")


def _run_fwd(gpu, specs, entry="tspm_lstm_fwd_w"):
    """specs: list of (xg, whh, bhh, maxpool, ld) -> list of (_Fwd, outputs) from ONE call."""
    fs = [_Fwd(gpu, *s) for s in specs]
    descs = (L.LstmFwdDesc * len(fs))(*[f.desc() for f in fs])
    L.check(getattr(L.lib(), entry)(len(fs), descs, L.stream_handle()), entry)
    _sync()
    for f in fs:
        f.intact()
    return [(f, f.outputs()) for f in fs]


class _Bwd:
    def __init__(self, gpu, f, dh, ld):
        self.f, self.ld = f, ld
        self.dh = torch.full((f.B, ld), float("nan"), device=gpu)  # the padding columns must never be read
        self.dh[:, :f.H] = dh.to(gpu)
        self.dgates = Guarded(gpu, f.T * f.B, 4 * f.H)

    def desc(self):
        f = self.f
        return L.LstmBwdDesc(f.B, f.T, f.H, self.ld, f.whh.data_ptr(), f.gates.ptr(), f.cs.ptr(), self.dh.data_ptr(),
                             self.dgates.ptr(), f.arg.ptr() if f.arg else None)


def _run_bwd(gpu, specs, entry="tspm_lstm_bwd_w"):
    """specs: list of (_Fwd, dh [B,H] cpu, ld_dh) -> list of dgates [T,B,4H] (cpu) from ONE call."""
    bs = [_Bwd(gpu, *s) for s in specs]
    descs = (L.LstmBwdDesc * len(bs))(*[b.desc() for b in bs])
    L.check(getattr(L.lib(), entry)(len(bs), descs, L.stream_handle()), entry)
    _sync()
    for b in bs:
        b.dgates.intact(f"lstm_bwd_w H{b.f.H} dgates")
    return [b.dgates.cpu().view(b.f.T, b.f.B, 4 * b.f.H) for b in bs]


def _bwd_ref(case, dh, arg, dtype):
    """Autograd through the cell loop from loss = sum(dh * emb), emb = h_T or h gathered at the KERNEL's argmax."""
    _, _, hs, pres = _cell_loop(case["xg"], case["whh"], case["bhh"], dtype, grad=True)
    emb = hs[-1] if arg is None else hs[1:].gather(0, arg.long().unsqueeze(0)).squeeze(0)
    (dh.to(dtype) * emb).sum().backward()
    return torch.stack([torch.zeros_like(p) if p.grad is None else p.grad for p in pres])


def _check_fwd(tag, case, o, maxpool, count_flips=True):
    g32, c32, h32 = case["r32"]
    g64, c64, h64 = case["r64"]
    op_check(f"lstm_fwd_w.gates[{tag}]", o["gates"], g32, g64, ratios=RATIOS)
    op_check(f"lstm_fwd_w.cs[{tag}]", o["cs"], c32, c64, ratios=RATIOS)
    op_check(f"lstm_fwd_w.hs[{tag}]", o["hs"], h32, h64, ratios=RATIOS)
    assert bool((o["hs"][0] == 0).all()), "hs[0] must be the zero initial state"
    if maxpool:
        v32, _ = _pool_time(h32)
        v64, i64 = _pool_time(h64)
        op_check(f"lstm_fwd_w.h_out[{tag}]", o["hout"], v32, v64, ratios=RATIOS)
        arg = o["arg"].long()
        if count_flips:
            nf = near_tie_flips(f"lstm_fwd_w.argmax[{tag}]", arg, i64, h64[1:].permute(1, 2, 0), 2)
            print(f"lstm_fwd_w.argmax[{tag}]: {nf} flips of {arg.numel()}")
        else:
            print(f"lstm_fwd_w.argmax[{tag}]: {int((arg != i64).sum())} flips of {arg.numel()} (not asserted)")
        # the select is exact: h_out is our own h at our own index, which is the first maximum of our own h
        assert torch.equal(o["hout"], o["hs"][1:].gather(0, arg.unsqueeze(0)).squeeze(0))
        assert torch.equal(arg, _pool_time(o["hs"])[1])
    else:
        op_check(f"lstm_fwd_w.h_out[{tag}]", o["hout"], h32[-1], h64[-1], ratios=RATIOS)
        assert torch.equal(o["hout"], o["hs"][-1])


@pytest.mark.parametrize("regime", ["a", "b"])
@pytest.mark.parametrize("B,T,mode", SHAPES)
@pytest.mark.parametrize("H", WIDTHS)
def test_lstm_fwd_w_vs_fp64(gpu, H, B, T, mode, regime):
    maxpool = mode == "maxpool"
    plant = (B, T) == (2, 256)
    for with_bhh in (True, False):
        case = _lstm_case(H, B, T, regime, with_bhh, plant_last=plant)
        for ld in (H, H + 12):
            tag = f"H{H} B{B} T{T} {mode} {regime} bhh{int(with_bhh)} ld{ld}"
            spec = (case["xg"], case["whh"], case["bhh"], maxpool, ld)
            (_, o), = _run_fwd(gpu, [spec])
            (_, o2), = _run_fwd(gpu, [spec])
            assert all(_same(o[k], o2[k]) for k in o), "lstm_fwd_w is not deterministic"
            _check_fwd(tag, case, o, maxpool, count_flips=(H, regime, B, T) not in NO_FLIP_COUNT)
            if plant:
                assert o["arg"][B - 1, H - 1].item() == 255
                assert _pool_time(case["r64"][2])[1][B - 1, H - 1].item() == 255
    print("worst ratios:", RATIOS)


@pytest.mark.parametrize("regime", ["a", "b"])
@pytest.mark.parametrize("B,T,mode", SHAPES)
@pytest.mark.parametrize("H", WIDTHS)
def test_lstm_bwd_w_vs_fp64(gpu, H, B, T, mode, regime):
    maxpool = mode == "maxpool"
    dh = torch.randn(B, H, generator=torch.Generator().manual_seed(B * 1000 + T))
    for with_bhh, ld in ((True, H), (False, H + 12)):
        case = _lstm_case(H, B, T, regime, with_bhh, plant_last=(B, T) == (2, 256))
        tag = f"H{H} B{B} T{T} {mode} {regime} bhh{int(with_bhh)} ld{ld}"
        (f, o), = _run_fwd(gpu, [(case["xg"], case["whh"], case["bhh"], maxpool, H)])
        dg, = _run_bwd(gpu, [(f, dh, ld)])
        dg2, = _run_bwd(gpu, [(f, dh, ld)])
        assert torch.equal(dg, dg2), "lstm_bwd_w is not deterministic"
        arg = o["arg"] if maxpool else None
        r32, r64 = _bwd_ref(case, dh, arg, torch.float32), _bwd_ref(case, dh, arg, torch.float64)
        op_check(f"lstm_bwd_w.dgates[{tag}]", dg, r32, r64, grad=True, ratios=RATIOS)
        # per time step: an error confined to one step cannot hide in the whole-tensor norm
        eo = [rel_l2(dg[t], r64[t]) for t in range(T)]
        er = [rel_l2(r32[t], r64[t]) for t in range(T)]
        live = [t for t in range(T) if r64[t].abs().max() > 0]
        for t in range(T):
            if t not in live:
                assert bool((dg[t] == 0).all()), f"{tag}: step {t} has no gradient and must be exact zeros"
        # where fp32 still carries its full precision (test_gpu_seq_ops: 1e-30 rms keeps every product of two factors
        # normal): the worst step, and step by step.  Below that the gradient has decayed through the forget gates out
        # of fp32's normal range — at width 32, T = 300, regime "b" the fp64 gradient of the first 130 steps is 1e-45
        # to 1e-79, under fp32's smallest subnormal, where the fp32 reference itself returns exact zeros (relative
        # error 1) and one subnormal ulp is a relative error of 8 — so there the same per-step criterion gets an
        # absolute allowance of fp32's smallest normal number per element (2^-126: nothing next to a gradient of
        # 1e-31, everything next to one of 1e-46, and still far below any value a wrong kernel would write).
        full = [t for t in live if r64[t].pow(2).mean().sqrt() >= 1e-30]
        assert full, tag
        mo, mr = max(eo[t] for t in full), max(er[t] for t in full)
        print(f"lstm_bwd_w.dgates per step[{tag}]: max err_ours {mo:.3e} max err_ref32 {mr:.3e} ({len(full)} of "
              f"{len(live)} live steps at full precision)")
        RATIOS.note("lstm_bwd_w.dgates/step", mo, mr)
        assert mo <= FACTOR * mr + FLOOR_GRAD, (tag, mo, mr)
        for t in full:
            assert eo[t] <= FACTOR * er[t] + FLOOR_GRAD, (tag, t, eo[t], er[t])
        for t in live:
            if t not in full:
                ao, n64 = float((dg[t].double() - r64[t]).norm()), float(r64[t].norm())
                assert ao <= (FACTOR * er[t] + FLOOR_GRAD) * n64 + 2.0 ** -126 * dg[t].numel() ** 0.5, (tag, t, ao, n64, er[t])
    print("worst ratios:", RATIOS)


@pytest.mark.parametrize("mode", ["last", "maxpool"])
def test_width_64_is_bitwise_the_fixed_width_entry_points(gpu, mode):
    """hidden = 64 through tspm_lstm_fwd_w / _bwd_w gives bitwise what tspm_lstm_fwd / _bwd give on the same inputs,
    one and two descriptors."""
    maxpool = mode == "maxpool"
    a, b = _lstm_case(64, 5, 37, "a", True, seed=1), _lstm_case(64, 2, 19, "b", False, seed=2)
    specs = [(a["xg"], a["whh"], a["bhh"], maxpool, 64 + 12), (b["xg"], b["whh"], b["bhh"], maxpool, 64)]
    dhs = [torch.randn(5, 64, generator=torch.Generator().manual_seed(5)),
           torch.randn(2, 64, generator=torch.Generator().manual_seed(6))]
    for sel in ([0], [1], [0, 1]):
        new = _run_fwd(gpu, [specs[i] for i in sel])
        old = _run_fwd(gpu, [specs[i] for i in sel], entry="tspm_lstm_fwd")
        for (_, on), (_, oo) in zip(new, old):
            assert on.keys() == oo.keys() and all(torch.equal(on[k], oo[k]) for k in on)
        gn = _run_bwd(gpu, [(new[n][0], dhs[i], 64 + 4 * n) for n, i in enumerate(sel)])
        go = _run_bwd(gpu, [(old[n][0], dhs[i], 64 + 4 * n) for n, i in enumerate(sel)], entry="tspm_lstm_bwd")
        assert all(torch.equal(x, y) for x, y in zip(gn, go))


@pytest.mark.parametrize("ha,hb", [(36, 128), (128, 36), (128, 4), (4, 128), (36, 60), (100, 128), (64, 36)])
def test_two_widths_in_one_call_equal_single_calls(gpu, ha, hb):
    """Two LSTMs of different widths, shapes and embedding modes in one call — two launches when their kernel tiers
    differ, one when they share a tier (each half of the grid then runs at its own width) — are bitwise what two
    count-1 calls give, forward and backward."""
    a, b = _lstm_case(ha, 5, 7, "a", True, seed=1), _lstm_case(hb, 2, 19, "a", False, seed=2)
    specs = [(a["xg"], a["whh"], a["bhh"], True, ha + 12), (b["xg"], b["whh"], b["bhh"], False, hb)]
    dhs = [torch.randn(5, ha, generator=torch.Generator().manual_seed(5)),
           torch.randn(2, hb, generator=torch.Generator().manual_seed(6))]
    pair = _run_fwd(gpu, specs)
    single = [_run_fwd(gpu, [s])[0] for s in specs]
    for (_, op), (_, os_) in zip(pair, single):
        assert op.keys() == os_.keys() and all(torch.equal(op[k], os_[k]) for k in op)
    _check_fwd(f"pair H{ha}", a, pair[0][1], True)
    _check_fwd(f"pair H{hb}", b, pair[1][1], False)
    gp = _run_bwd(gpu, [(pair[0][0], dhs[0], ha), (pair[1][0], dhs[1], hb + 12)])
    gs = [_run_bwd(gpu, [(single[0][0], dhs[0], ha)])[0], _run_bwd(gpu, [(single[1][0], dhs[1], hb + 12)])[0]]
    assert torch.equal(gp[0], gs[0]) and torch.equal(gp[1], gs[1])


@pytest.mark.parametrize("H", [36, 100])
def test_nan_stays_in_its_row_with_idle_lanes(gpu, H):
    """One NaN in xg at (t = 4, b = 1) at a width with idle lanes: every unit of row 1 ends NaN with the last step as
    its index; every other row — row 0 shares row 1's workgroup and its idle lanes — is bitwise the run without the
    NaN, forward and backward, and nothing is written outside the H real columns (guards)."""
    B, T = 4, 9
    case = _lstm_case(H, B, T, "a", True, seed=7)
    xg = case["xg"].clone()
    xg[4, 1, 2 * H + 9] = float("nan")
    (fc, clean), = _run_fwd(gpu, [(case["xg"], case["whh"], case["bhh"], True, H + 12)])
    (fn, o), = _run_fwd(gpu, [(xg, case["whh"], case["bhh"], True, H + 12)])
    others = [0, 2, 3]
    for k in ("gates", "cs", "hs"):
        assert torch.equal(o[k][:, others], clean[k][:, others]), k
        assert torch.equal(o[k][:4, 1], clean[k][:4, 1]), k  # row 1 before the NaN (hs[4] = h after step 3)
    assert torch.equal(o["hout"][others], clean["hout"][others]) and torch.equal(o["arg"][others], clean["arg"][others])
    assert bool(o["hs"][1:, 1].isnan().any(0).all()), "the NaN reaches every unit of its row through the recurrence"
    assert bool(o["hout"][1].isnan().all()) and bool((o["arg"][1] == T - 1).all())
    _, _, h32, _ = _cell_loop(xg, case["whh"], case["bhh"], torch.float32)
    assert torch.equal(_pool_time(h32)[1][1], o["arg"][1].long())  # F.max_pool1d agrees: last NaN
    dh = torch.randn(B, H, generator=torch.Generator().manual_seed(11))
    dgc, = _run_bwd(gpu, [(fc, dh, H + 12)])
    dgn, = _run_bwd(gpu, [(fn, dh, H + 12)])
    assert torch.equal(dgn[:, others], dgc[:, others])
    assert not bool(dgc.isnan().any())
