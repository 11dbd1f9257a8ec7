"""The sequence-path entry points one at a time against plain-torch restatements in float64 on the CPU:
tspm_lstm_fwd / _bwd, tspm_textcnn_pool_fwd, tspm_textcnn_bwd (per-channel rows kernel), tspm_grad_clip_coef,
tspm_adam_step_clip and tspm_linear_bwd_weight_splitk, through the C ABI.

Criterion (tests/parity.py): err_ours = rel-L2(ours, fp64) <= FACTOR x err_ref32 + floor, where ref32 is the same
restatement run in float32 on the CPU (gradients: FLOOR_GRAD and cosine >= GRAD_COS); exact operations (add, compare,
select, mask scale, copy, counts) are held to torch.equal with the fp32 CPU result; argmax decisions to the fp64
reference's own, a disagreement being allowed only as a rare near-tie.  Every output is followed by a sentinel guard
region (and its padding columns are guards), and every kernel runs twice for bitwise determinism.  The shapes are
the smallest at which each kernel can go wrong: a one-row and an odd batch (ghost row of the 2-row LSTM workgroup),
T = 1, the uint8 time-index limit T = 256, T > 256 without an index, row strides above the width.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from parity import (FACTOR, FLOOR_GRAD, Guarded, Ratios, adam_fp64, adam_tolerance, near_tie_flips, op_check, rel_l2)
from tspm_amd import _lib as L

pytestmark = pytest.mark.gpu
H, G = 64, 256
RATIOS = Ratios()


def _sync():
    torch.cuda.synchronize()


def _same(a, b):
    """torch.equal that takes NaN == NaN (payloads are not compared)."""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


# ------------------------------------------------------------------------------------------------
# LSTM
# ------------------------------------------------------------------------------------------------
def _cell_loop(xg, whh, bhh, dtype, grad=False):
    """nn.LSTM's cell in ATen's order on the projected input: gates = (h W_hh^T + b_hh) + xg_t; i, f, g, o;
    c = f*c + i*g; h = o*tanh(c).  Returns activated gates [T,B,4H], cs [T,B,H], hs [T+1,B,H] and the list of
    pre-activations (with retain_grad when `grad`)."""
    xg, whh = xg.to(dtype), whh.to(dtype)
    bhh = None if bhh is None else bhh.to(dtype)
    if grad:
        xg = xg.clone().requires_grad_(True)
    T, B, _ = xg.shape
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


def _pool_time(hs):
    """F.max_pool1d over time of r_out = hs[1:] -> (values [B,H], first-maximum index [B,H])."""
    r = hs[1:].permute(1, 2, 0).contiguous()  # [B, H, T]
    v, i = F.max_pool1d(r, r.shape[2], return_indices=True)
    return v.squeeze(2), i.squeeze(2)


@functools.lru_cache(maxsize=None)
def _lstm_case(B, T, regime, with_bhh, seed=0, plant_last=False):
    """Inputs (xg computed once on the CPU in fp32, so the projection GEMM is not part of the test) and the fp32 /
    fp64 forward references.  regime 'a': nn.LSTM default initialisation, randn input; 'b': weights x8, input x6
    (saturating gates)."""
    g = torch.Generator().manual_seed(seed)
    feat = 20
    k = 1.0 / H ** 0.5
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * k
    wih, whh, bih, bhh = u(G, feat), u(G, H), u(G), u(G)
    x = torch.randn(T, B, feat, generator=g)
    if regime == "b":
        wih, whh, bih, bhh, x = wih * 8, whh * 8, bih * 8, bhh * 8, x * 6
    xg = (x.reshape(T * B, feat) @ wih.T + bih).reshape(T, B, G).contiguous()
    if plant_last:  # unit 5 of the last row: output gate shut until the last step, which then holds the maximum
        b, un = B - 1, 5
        xg[:, b, 3 * H + un] = -20.0
        xg[T - 1, b, [un, H + un, 2 * H + un, 3 * H + un]] = torch.tensor([20.0, -20.0, 20.0, 20.0])
    bh = bhh if with_bhh else None
    r32 = _cell_loop(xg, whh, bh, torch.float32)[:3]
    r64 = _cell_loop(xg, whh, bh, torch.float64)[:3]
    return dict(xg=xg, whh=whh, bhh=bh, r32=r32, r64=r64, B=B, T=T)


class _Fwd:
    """Device buffers of one forward descriptor (guarded outputs)."""

    def __init__(self, gpu, xg, whh, bhh, maxpool, ld):
        T, B, _ = xg.shape
        self.T, self.B, self.ld, self.maxpool = T, B, ld, maxpool
        self.xg, self.whh = xg.to(gpu), whh.to(gpu)
        self.bhh = None if bhh is None else bhh.to(gpu)
        self.gates, self.cs = Guarded(gpu, T * B, G), Guarded(gpu, T * B, H)
        self.hs, self.hout = Guarded(gpu, (T + 1) * B, H), Guarded(gpu, B, H, ld)
        self.arg = Guarded(gpu, B, H, dtype=torch.uint8) if maxpool else None

    def desc(self):
        return L.LstmFwdDesc(self.B, self.T, H, self.ld, self.xg.data_ptr(), self.whh.data_ptr(), L.ptr(self.bhh),
                             self.gates.ptr(), self.cs.ptr(), self.hs.ptr(), self.hout.ptr(),
                             self.arg.ptr() if self.arg else None)

    def outputs(self):
        T, B = self.T, self.B
        o = dict(gates=self.gates.cpu().view(T, B, G), cs=self.cs.cpu().view(T, B, H),
                 hs=self.hs.cpu().view(T + 1, B, H), hout=self.hout.cpu())
        if self.arg:
            o["arg"] = self.arg.cpu()
        return o

    def intact(self):
        for n in ("gates", "cs", "hs", "hout", "arg"):
            if getattr(self, n) is not None:
                getattr(self, n).intact("lstm_fwd " + n)


def _run_fwd(gpu, specs):
    """specs: list of (xg, whh, bhh, maxpool, ld) -> list of (_Fwd, outputs) from ONE launch."""
    fs = [_Fwd(gpu, *s) for s in specs]
    descs = (L.LstmFwdDesc * len(fs))(*[f.desc() for f in fs])
    L.check(L.lib().tspm_lstm_fwd(len(fs), descs, L.stream_handle()), "lstm_fwd")
    _sync()
    for f in fs:
        f.intact()
    return [(f, f.outputs()) for f in fs]


class _Bwd:
    def __init__(self, gpu, f, dh, ld):
        self.f, self.ld = f, ld
        self.dh = torch.full((f.B, ld), float("nan"), device=gpu)  # the padding columns must never be read
        self.dh[:, :H] = dh.to(gpu)
        self.dgates = Guarded(gpu, f.T * f.B, G)

    def desc(self):
        f = self.f
        return L.LstmBwdDesc(f.B, f.T, H, self.ld, f.whh.data_ptr(), f.gates.ptr(), f.cs.ptr(), self.dh.data_ptr(),
                             self.dgates.ptr(), f.arg.ptr() if f.arg else None)


def _run_bwd(gpu, specs):
    """specs: list of (_Fwd, dh [B,H] cpu, ld_dh) -> list of dgates [T,B,4H] (cpu) from ONE launch."""
    bs = [_Bwd(gpu, *s) for s in specs]
    descs = (L.LstmBwdDesc * len(bs))(*[b.desc() for b in bs])
    L.check(L.lib().tspm_lstm_bwd(len(bs), descs, L.stream_handle()), "lstm_bwd")
    _sync()
    for b in bs:
        b.dgates.intact("lstm_bwd dgates")
    return [b.dgates.cpu().view(b.f.T, b.f.B, G) for b in bs]


def _bwd_ref(case, dh, arg, dtype):
    """Autograd through the cell loop from loss = sum(dh * emb), emb = h_T or h gathered at the KERNEL's argmax."""
    _, _, hs, pres = _cell_loop(case["xg"], case["whh"], case["bhh"], dtype, grad=True)
    emb = hs[-1] if arg is None else hs[1:].gather(0, arg.long().unsqueeze(0)).squeeze(0)
    (dh.to(dtype) * emb).sum().backward()
    return torch.stack([torch.zeros_like(p) if p.grad is None else p.grad for p in pres])


LSTM_SHAPES = [(1, 1, "maxpool"), (1, 1, "last"), (2, 3, "maxpool"), (2, 3, "last"), (5, 37, "maxpool"),
               (5, 37, "last"), (3, 256, "maxpool"), (2, 300, "last")]


def _check_fwd(tag, case, o, maxpool):
    g32, c32, h32 = case["r32"]
    g64, c64, h64 = case["r64"]
    op_check(f"lstm_fwd.gates[{tag}]", o["gates"], g32, g64, ratios=RATIOS)
    op_check(f"lstm_fwd.cs[{tag}]", o["cs"], c32, c64, ratios=RATIOS)
    op_check(f"lstm_fwd.hs[{tag}]", o["hs"], h32, h64, ratios=RATIOS)
    assert bool((o["hs"][0] == 0).all()), "hs[0] must be the zero initial state"
    if maxpool:
        v32, _ = _pool_time(h32)
        v64, i64 = _pool_time(h64)
        op_check(f"lstm_fwd.h_out[{tag}]", o["hout"], v32, v64, ratios=RATIOS)
        arg = o["arg"].long()
        nf = near_tie_flips(f"lstm_fwd.argmax[{tag}]", arg, i64, h64[1:].permute(1, 2, 0), 2)
        print(f"lstm_fwd.argmax[{tag}]: {nf} flips of {arg.numel()}")
        # the select is exact: h_out is our own h at our own index, which is the first maximum of our own h
        assert torch.equal(o["hout"], o["hs"][1:].gather(0, arg.unsqueeze(0)).squeeze(0))
        assert torch.equal(arg, _pool_time(o["hs"])[1])
    else:
        op_check(f"lstm_fwd.h_out[{tag}]", o["hout"], h32[-1], h64[-1], ratios=RATIOS)
        assert torch.equal(o["hout"], o["hs"][-1])


@pytest.mark.parametrize("regime", ["a", "b"])
@pytest.mark.parametrize("B,T,mode", LSTM_SHAPES)
def test_lstm_fwd_vs_fp64(gpu, B, T, mode, regime):
    maxpool = mode == "maxpool"
    plant = (B, T) == (3, 256)
    for with_bhh in (True, False):
        case = _lstm_case(B, T, regime, with_bhh, plant_last=plant)
        for ld in (H, H + 12):
            tag = f"B{B} T{T} {mode} {regime} bhh{int(with_bhh)} ld{ld}"
            spec = (case["xg"], case["whh"], case["bhh"], maxpool, ld)
            (_, o), = _run_fwd(gpu, [spec])
            (_, o2), = _run_fwd(gpu, [spec])
            assert all(_same(o[k], o2[k]) for k in o), "lstm_fwd is not deterministic"
            _check_fwd(tag, case, o, maxpool)
            if plant:
                assert o["arg"][B - 1, 5].item() == 255 and _pool_time(case["r64"][2])[1][B - 1, 5].item() == 255
    print("worst ratios:", RATIOS)


@pytest.mark.parametrize("regime", ["a", "b"])
@pytest.mark.parametrize("B,T,mode", LSTM_SHAPES)
def test_lstm_bwd_vs_fp64(gpu, B, T, mode, regime):
    maxpool = mode == "maxpool"
    dh = torch.randn(B, H, generator=torch.Generator().manual_seed(B * 1000 + T))
    for with_bhh, ld in ((True, H), (False, H + 12)):
        case = _lstm_case(B, T, regime, with_bhh, plant_last=(B, T) == (3, 256))
        tag = f"B{B} T{T} {mode} {regime} bhh{int(with_bhh)} ld{ld}"
        (f, o), = _run_fwd(gpu, [(case["xg"], case["whh"], case["bhh"], maxpool, H)])
        dg, = _run_bwd(gpu, [(f, dh, ld)])
        dg2, = _run_bwd(gpu, [(f, dh, ld)])
        assert torch.equal(dg, dg2), "lstm_bwd is not deterministic"
        arg = o["arg"] if maxpool else None
        r32, r64 = _bwd_ref(case, dh, arg, torch.float32), _bwd_ref(case, dh, arg, torch.float64)
        op_check(f"lstm_bwd.dgates[{tag}]", dg, r32, r64, grad=True, ratios=RATIOS)
        # per time step: an error confined to one step cannot hide in the whole-tensor norm
        eo = [rel_l2(dg[t], r64[t]) for t in range(T)]
        er = [rel_l2(r32[t], r64[t]) for t in range(T)]
        live = [t for t in range(T) if r64[t].abs().max() > 0]
        for t in range(T):
            if t not in live:
                assert bool((dg[t] == 0).all()), f"{tag}: step {t} has no gradient and must be exact zeros"
        mo, mr = max(eo[t] for t in live), max(er[t] for t in live)
        print(f"lstm_bwd.dgates per step[{tag}]: max err_ours {mo:.3e} max err_ref32 {mr:.3e} ({len(live)} live steps)")
        RATIOS.note("lstm_bwd.dgates/step", mo, mr)
        assert mo <= FACTOR * mr + FLOOR_GRAD, (tag, mo, mr)
        # step by step where fp32 still carries its full precision (the gradient decays through the forget gates
        # and leaves fp32's normal range on the long sequences; 1e-30 rms keeps every product of two factors normal)
        for t in live:
            if r64[t].pow(2).mean().sqrt() >= 1e-30:
                assert eo[t] <= FACTOR * er[t] + FLOOR_GRAD, (tag, t, eo[t], er[t])
    print("worst ratios:", RATIOS)


@pytest.mark.parametrize("order", [0, 1])
def test_lstm_two_descriptors_equal_single_launches(gpu, order):
    """Two LSTMs of different shapes and embedding modes in one launch (the nb0 block split, with an odd first batch
    in one order): each half is bitwise what its own one-descriptor call gives, forward and backward."""
    a, b = _lstm_case(5, 7, "a", True, seed=1), _lstm_case(2, 19, "a", False, seed=2)
    specs = [(a["xg"], a["whh"], a["bhh"], True, H + 12), (b["xg"], b["whh"], b["bhh"], False, H)]
    dhs = [torch.randn(5, H, generator=torch.Generator().manual_seed(5)),
           torch.randn(2, H, generator=torch.Generator().manual_seed(6))]
    if order:
        specs, dhs = specs[::-1], dhs[::-1]
    pair = _run_fwd(gpu, specs)
    single = [_run_fwd(gpu, [s])[0] for s in specs]
    for (fp, op), (fs, os_) in zip(pair, single):
        assert op.keys() == os_.keys() and all(torch.equal(op[k], os_[k]) for k in op)
    gp = _run_bwd(gpu, [(pair[0][0], dhs[0], H), (pair[1][0], dhs[1], H + 12)])
    gs = [_run_bwd(gpu, [(single[0][0], dhs[0], H)])[0], _run_bwd(gpu, [(single[1][0], dhs[1], H + 12)])[0]]
    assert torch.equal(gp[0], gs[0]) and torch.equal(gp[1], gs[1])


def test_lstm_exact_ties(gpu):
    """First maximum on exact ties, forward and backward."""
    # (i) everything zero: h == 0 at every step, the first step holds the (tied) maximum
    B, T = 3, 6
    z = torch.zeros
    (f, o), = _run_fwd(gpu, [(z(T, B, G), z(G, H), z(G), True, H)])
    assert bool((o["hs"] == 0).all()) and bool((o["hout"] == 0).all()) and bool((o["arg"] == 0).all())
    # the embedding gradient enters only at t = 0 and, with w_hh == 0, reaches no other step
    dh = torch.randn(B, H, generator=torch.Generator().manual_seed(3))
    dg, = _run_bwd(gpu, [(f, dh, H)])
    assert bool((dg[1:] == 0).all())
    case = dict(xg=z(T, B, G), whh=z(G, H), bhh=z(G))
    r64 = _bwd_ref(case, dh, o["arg"], torch.float64)
    op_check("lstm_bwd.dgates[all-zero tie]", dg, _bwd_ref(case, dh, o["arg"], torch.float32), r64, grad=True)
    assert bool((r64[1:] == 0).all())
    # (ii) w_hh == 0 and f == 0 exactly (pre-activation -200): h_t depends on xg[t] alone; steps 2 and 5 get the
    # same dominant row, so h_2 == h_5 bitwise and the first of them wins
    T = 7
    g = torch.Generator().manual_seed(4)
    xg = torch.rand(T, B, G, generator=g) * 2 - 1
    xg[:, :, H:2 * H] = -200.0
    xg[2] = xg[5] = 5.0
    xg[2, :, H:2 * H] = xg[5, :, H:2 * H] = -200.0
    (f, o), = _run_fwd(gpu, [(xg, z(G, H), None, True, H)])
    assert bool((o["gates"][:, :, H:2 * H] == 0).all()), "sigmoid(-200) must be exactly 0 in fp32"
    assert torch.equal(o["hs"][3], o["hs"][6]) and bool((o["arg"] == 2).all()) and torch.equal(o["hout"], o["hs"][3])
    _, i64 = _pool_time(_cell_loop(xg, z(G, H), None, torch.float64)[2])
    assert bool((i64 == 2).all())


def test_lstm_nan_wins_and_stays_in_its_row(gpu):
    """One NaN in xg at (t = 4, b = 1): every unit of row 1 ends NaN with the LAST step as its index (each NaN step
    replaces the running maximum, as max_pool2d_with_indices); every other row — row 0 shares row 1's workgroup —
    is bitwise the run without the NaN."""
    B, T = 4, 9
    case = _lstm_case(B, T, "a", True, seed=7)
    xg = case["xg"].clone()
    xg[4, 1, 2 * H + 9] = float("nan")
    (_, clean), = _run_fwd(gpu, [(case["xg"], case["whh"], case["bhh"], True, H)])
    (_, o), = _run_fwd(gpu, [(xg, case["whh"], case["bhh"], True, H)])
    others = [0, 2, 3]
    for k in ("gates", "cs", "hs"):
        assert torch.equal(o[k][:, others], clean[k][:, others]), k
        assert torch.equal(o[k][:4, 1], clean[k][:4, 1]), k  # row 1 before the NaN (hs[4] = h after step 3)
    assert torch.equal(o["hout"][others], clean["hout"][others]) and torch.equal(o["arg"][others], clean["arg"][others])
    nan_unit = o["hs"][1:, 1].isnan().any(0)
    assert bool(nan_unit.all()), "the NaN reaches every unit of its row through the recurrence"
    assert bool(o["hout"][1].isnan().all()) and bool((o["arg"][1] == T - 1).all())
    _, _, h32, _ = _cell_loop(xg, case["whh"], case["bhh"], torch.float32)
    assert torch.equal(_pool_time(h32)[1][1], o["arg"][1].long())  # F.max_pool1d agrees: last NaN


# ------------------------------------------------------------------------------------------------
# TextCNN pooling (every operation exact in fp32)
# ------------------------------------------------------------------------------------------------
def _pool_fwd(gpu, B, T, heights, C, convs, biases, keep, scale, ld):
    n, nc = len(heights), len(heights) * C
    cd = [c.to(gpu) for c in convs]
    bd = None if biases is None else [None if b is None else b.to(gpu) for b in biases]
    kd = None if keep is None else keep.to(gpu)
    pooled, arg, out = Guarded(gpu, B, nc), Guarded(gpu, B, nc, dtype=torch.uint8), Guarded(gpu, B, nc, ld)
    bp = None if bd is None else (ctypes.c_void_p * n)(*[L.ptr(b) for b in bd])
    L.check(L.lib().tspm_textcnn_pool_fwd(B, T, n, (ctypes.c_int32 * n)(*heights), C,
                                          (ctypes.c_void_p * n)(*[c.data_ptr() for c in cd]), bp, L.ptr(kd), scale,
                                          pooled.ptr(), arg.ptr(), out.ptr(), ld, L.stream_handle()), "textcnn_pool_fwd")
    _sync()
    for nme, gd in (("pooled", pooled), ("argmax", arg), ("out", out)):
        gd.intact("textcnn_pool_fwd " + nme)
    return pooled.cpu(), arg.cpu(), out.cpu()


def _pool_ref(B, T, heights, C, convs, biases, keep, scale):
    ps, idx = [], []
    for i, h in enumerate(heights):
        y = convs[i].permute(1, 2, 0)  # [B, C, Tout]
        if biases is not None and biases[i] is not None:
            y = y + biases[i][None, :, None]
        v, ix = F.max_pool1d(torch.relu(y), T - h + 1, return_indices=True)
        ps.append(v.squeeze(2)); idx.append(ix.squeeze(2))
    pooled, arg = torch.cat(ps, 1), torch.cat(idx, 1)
    out = pooled if keep is None else pooled * torch.where(keep.bool(), torch.tensor(scale), torch.tensor(0.0))
    return pooled, arg, out


@pytest.mark.parametrize("B,T,heights,C", [(1, 5, (5,), 5), (6, 9, (1, 2, 3, 5), 7), (3, 256, (3, 4, 5), 128)])
def test_textcnn_pool_fwd_exact(gpu, B, T, heights, C):
    g = torch.Generator().manual_seed(T)
    n, nc = len(heights), len(heights) * C
    convs = [torch.randn(T - h + 1, B, C, generator=g) for h in heights]
    bias = [torch.randn(C, generator=g) for _ in heights]
    keep = (torch.rand(B, nc, generator=g) > 0.5).to(torch.uint8)
    planted = {}
    if T == 256:  # the maximum at the last position of one channel (index T - h, up to 253)
        for i, h in enumerate(heights):
            convs[i][T - h, 1, 17] = 100.0
            planted[(1, i * C + 17)] = T - h
    if T == 9:
        i, ci = n - 1, (n - 1) * C
        convs[i][:, 0, 0] = -convs[i][:, 0, 0].abs() - bias[i][0].abs() - 1   # a channel never positive: 0 at index 0
        convs[i][1, 2, 1] = convs[i][3, 2, 1] = 50.0                           # equal maxima: the first wins
        convs[i][2, 4, 2] = float("nan")                                       # NaN wins
        planted.update({(0, ci): 0, (2, ci + 1): 1, (4, ci + 2): 2})
    nulled = list(bias); nulled[0] = None
    for biases in (bias, None, nulled):
        for kp in (keep, None):
            for ld in (nc, nc + 4):
                got = _pool_fwd(gpu, B, T, heights, C, convs, biases, kp, 2.0, ld)
                again = _pool_fwd(gpu, B, T, heights, C, convs, biases, kp, 2.0, ld)
                ref = _pool_ref(B, T, heights, C, convs, biases, kp, 2.0)
                assert _same(got[0], ref[0]), "pooled"
                assert torch.equal(got[1].long(), ref[1]), "argmax"
                assert _same(got[2], ref[2]), "out"
                assert all(_same(a, b) for a, b in zip(got, again)), "not deterministic"
                for (b, c), t in planted.items():
                    assert got[1][b, c].item() == t, (b, c, t)
    if T == 9:
        assert got[0][0, ci].item() == 0.0 and got[0][4, ci + 2].isnan()


# ------------------------------------------------------------------------------------------------
# TextCNN backward, per-channel rows kernel (channels != 128)
# ------------------------------------------------------------------------------------------------
def _textcnn_bwd_ref(B, T, Fe, heights, C, x, dout, keep, scale, pooled, arg, dtype):
    gw = dout.to(dtype)
    if keep is not None:
        gw = gw * keep.to(dtype) * scale
    gw = gw * (pooled > 0).to(dtype)
    xx = x.to(dtype).view(T, B, Fe)
    dws, dbs = [], []
    for i, h in enumerate(heights):
        a = arg.long()[:, i * C:(i + 1) * C]
        gi = gw[:, i * C:(i + 1) * C]
        ref = torch.zeros(C, h, Fe, dtype=dtype)
        for dt in range(h):
            ref[:, dt] = (gi[:, :, None] * xx[a + dt, torch.arange(B)[:, None]]).sum(0)
        dws.append(ref); dbs.append(gi.sum(0))
    return dws, dbs


@pytest.mark.parametrize("B,T,Fe,heights,C", [(5, 9, 33, (2, 5), 5), (3, 6, 1024, (3,), 4)])
def test_textcnn_bwd_rows_kernel_vs_fp64(gpu, B, T, Fe, heights, C):
    g = torch.Generator().manual_seed(Fe)
    n, nc = len(heights), len(heights) * C
    x = torch.randn(T, B, Fe, generator=g)
    x[:, 1] = 1e30   # batch row 1 is pooled to 0 everywhere below: it must contribute nothing
    dout = torch.randn(B, nc + 3, generator=g)
    dout[:, nc:] = 1e30   # the padding columns of ld_dout are not gradients
    keep = (torch.rand(B, nc, generator=g) > 0.3).to(torch.uint8)
    pooled = torch.randn(B, nc, generator=g).relu()
    pooled[1] = 0.0
    arg = torch.stack([torch.randint(0, T - h + 1, (B, C), generator=g) for h in heights], 1).reshape(B, nc)
    for i, h in enumerate(heights):   # a window that ends on the last row of the sequence
        arg[0, i * C] = T - h
        pooled[0, i * C], keep[0, i * C] = 1.5, 1
    arg = arg.to(torch.uint8)
    xd, dd, pd, ad = x.to(gpu), dout.to(gpu), pooled.to(gpu), arg.to(gpu)
    hs = (ctypes.c_int32 * n)(*heights)
    for kp in (keep, None):
        kd = None if kp is None else kp.to(gpu)
        r64 = _textcnn_bwd_ref(B, T, Fe, heights, C, x, dout[:, :nc], kp, 2.0, pooled, arg, torch.float64)
        r32 = _textcnn_bwd_ref(B, T, Fe, heights, C, x, dout[:, :nc], kp, 2.0, pooled, arg, torch.float32)
        for with_db in (True, False):
            def run():
                dws = [Guarded(gpu, C * h, Fe) for h in heights]
                dbs = [Guarded(gpu, 1, C) for _ in heights]
                work = Guarded(gpu, B, nc)
                dbp = (ctypes.c_void_p * n)(*[d.ptr() for d in dbs]) if with_db else None
                L.check(L.lib().tspm_textcnn_bwd(B, T, Fe, n, hs, C, xd.data_ptr(), dd.data_ptr(), nc + 3, L.ptr(kd), 2.0,
                                                 pd.data_ptr(), ad.data_ptr(),
                                                 (ctypes.c_void_p * n)(*[d.ptr() for d in dws]), dbp, work.ptr(),
                                                 L.stream_handle()), "textcnn_bwd")
                _sync()
                for d in dws + dbs + [work]:
                    d.intact("textcnn_bwd")
                return [d.cpu() for d in dws], [d.cpu() for d in dbs], dbs
            dws, dbs, raw = run()
            dws2, dbs2, _ = run()
            assert all(torch.equal(a, b) for a, b in zip(dws, dws2)), "not deterministic"
            for i, h in enumerate(heights):
                tag = f"B{B} F{Fe} conv{i} keep{int(kp is not None)}"
                op_check(f"textcnn_bwd.dw[{tag}]", dws[i].view(C, h, Fe), r32[0][i], r64[0][i], grad=True, ratios=RATIOS)
                if with_db:
                    op_check(f"textcnn_bwd.db[{tag}]", dbs[i].view(C), r32[1][i], r64[1][i], grad=True, ratios=RATIOS)
                    assert torch.equal(dbs[i], dbs2[i])
                else:  # db == NULL: nothing may be written anywhere near
                    assert bool(raw[i].flat.cpu().isnan().all())
    print("worst ratios:", RATIOS)


# ------------------------------------------------------------------------------------------------
# Global-norm clip coefficient and the clipped Adam
# ------------------------------------------------------------------------------------------------
def _clip(gpu, g, gs, max_norm, with_total=True, ws_bytes=None):
    gd = g.to(gpu)
    need = L.lib().tspm_grad_clip_workspace()
    ws = Guarded(gpu, 1, need, dtype=torch.uint8)
    coef, total = Guarded(gpu, 1, 1), Guarded(gpu, 1, 1)
    st = L.lib().tspm_grad_clip_coef(g.numel(), gd.data_ptr(), gs, max_norm, coef.ptr(), total.ptr() if with_total else None,
                                     ws.ptr(), need if ws_bytes is None else ws_bytes, L.stream_handle())
    _sync()
    ws.intact("clip workspace"); coef.intact("clip coef"); total.intact("clip total")
    return st, coef.cpu().reshape(()), total.flat[:1].cpu().reshape(())


def _neighbours(v):
    v = np.float32(v)
    return {float(np.nextafter(v, np.float32(-np.inf))), float(v), float(np.nextafter(v, np.float32(np.inf)))}


@pytest.mark.parametrize("count", [1, 3, 257, 512 * 256 + 1, 4 * 512 * 256 + 3])
def test_grad_clip_coef_vs_fp64(gpu, count):
    gen = torch.Generator().manual_seed(count)
    wide = 10.0 ** (torch.rand(count, generator=gen, dtype=torch.float64) * 38 - 20)   # 1e-20 .. 1e18
    wide = (wide * (torch.randint(0, 2, (count,), generator=gen) * 2 - 1)).float()
    values = {"randn": torch.randn(count, generator=gen), "wide": wide, "zeros": torch.zeros(count)}
    for name, g in values.items():
        for gs in (1.0, 1.0 / 3.0):
            gs32 = torch.tensor(gs, dtype=torch.float32)
            ref = np.float32(np.sqrt((g * gs32).double().pow(2).sum().item()))
            for max_norm in (1.0, 0.5):
                for with_total in (True, False):
                    st, coef, total = _clip(gpu, g, float(gs32), max_norm, with_total)
                    assert st == 0
                    _, coef2, _ = _clip(gpu, g, float(gs32), max_norm, with_total)
                    assert coef.item() == coef2.item(), "not deterministic"
                    cands = {float(min(np.float32(1.0), np.float32(max_norm) / (np.float32(t) + np.float32(1e-6))))
                             for t in _neighbours(ref)}
                    assert coef.item() in cands, (name, gs, max_norm, coef.item(), cands)
                    if with_total:
                        shown = total.item()
                        assert total.item() in _neighbours(ref), (name, gs, total.item(), float(ref))
                    else:  # total_norm == NULL: its sentinel is untouched
                        assert total.isnan()
                    if name == "zeros":
                        assert coef.item() == 1.0 and (not with_total or total.item() == 0.0)
            print(f"grad_clip_coef[{count} {name} gs {gs:.3f}]: total {shown:.9e} reference {float(ref):.9e}")


def test_grad_clip_coef_non_finite_follows_clip_grad_norm(gpu):
    """torch.nn.utils.clip_grad_norm_ clamps with torch.clamp(max=1.0), which propagates NaN: a NaN gradient
    element makes the total and the coefficient NaN (every gradient then turns NaN); an inf element gives an inf
    total and a coefficient of 0."""
    for count, at in ((4, 1), (512 * 256 + 1, 512 * 256)):
        g = torch.arange(1, count + 1, dtype=torch.float32) / count
        for bad in (float("nan"), float("inf"), float("-inf")):
            gb = g.clone()
            gb[at] = bad
            p = gb.clone().requires_grad_(True)
            p.grad = gb.clone()
            tref = torch.nn.utils.clip_grad_norm_([p], 1.0)
            st, coef, total = _clip(gpu, gb, 1.0, 1.0)
            print(f"grad_clip_coef[{count}, {bad}]: coef {coef.item()} total {total.item()} (torch total {tref.item()})")
            assert st == 0
            if bad != bad:
                assert tref.isnan() and bool(p.grad.isnan().all())
                assert total.isnan() and coef.isnan(), (coef.item(), total.item())
            else:
                assert tref.isinf() and total.item() == float("inf") and coef.item() == 0.0


def test_grad_clip_coef_short_workspace_status(gpu):
    g = torch.ones(8)
    need = L.lib().tspm_grad_clip_workspace()
    st, coef, _ = _clip(gpu, g, 1.0, 1.0, ws_bytes=need - 1)
    assert st == 3 and L.lib().tspm_status_string(st) == b"workspace too small"   # TSPM_ERR_WORKSPACE
    assert coef.isnan()  # nothing was launched
    gd = g.to(gpu)
    assert L.lib().tspm_grad_clip_coef(8, gd.data_ptr(), 1.0, 1.0, gd.data_ptr(), None, None, need, L.stream_handle()) == 3


def test_adam_step_clip_is_adam_on_scaled_gradients(gpu):
    """g' = (g * grad_scale) * coef: with grad_scale 1 the clipped update is bitwise tspm_adam_step on gradients
    pre-multiplied by the coefficient in fp32, and it is Adam in fp64 within adam_tolerance."""
    n, lr, wd = 1027, 1e-3, 1e-3
    gen = torch.Generator().manual_seed(11)
    p0, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 3
    m0, v0 = torch.randn(n, generator=gen) * 0.1, torch.rand(n, generator=gen) * 0.01
    st, coef, total = _clip(gpu, g, 1.0, 1.0)
    assert st == 0 and 0 < coef.item() < 1
    coef_d = coef.reshape(1).to(gpu)
    hyper = torch.tensor([lr, 0.9, 0.999, 1e-8, wd, 1.0, 0.0, 0.0], dtype=torch.float64)
    hyper.view(torch.int64)[6] = 3

    def run(clip):
        bufs = [Guarded(gpu, 1, n) for _ in range(3)]
        for b, src in zip(bufs, (p0, m0, v0)):
            b.t.copy_(src.view(1, n))
        gd = (g if clip else g * coef).to(gpu)
        hd = hyper.to(gpu)
        args = (n, bufs[0].ptr(), gd.data_ptr(), bufs[1].ptr(), bufs[2].ptr(), hd.data_ptr())
        if clip:
            L.check(L.lib().tspm_adam_step_clip(*args, coef_d.data_ptr(), L.stream_handle()), "adam_step_clip")
        else:
            L.check(L.lib().tspm_adam_step(*args, L.stream_handle()), "adam_step")
        _sync()
        for b in bufs:
            b.intact("adam")
        return [b.cpu().view(n) for b in bufs]
    clipped, plain = run(True), run(False)
    assert all(torch.equal(a, b) for a, b in zip(clipped, plain))
    assert all(torch.equal(a, b) for a, b in zip(clipped, run(True)))
    gc = g.double() * coef.double()
    exp, m, v = adam_fp64(p0, gc, 3, lr=lr, wd=wd, m=m0, v=v0)
    tol = 1e-6 * exp.abs() + adam_tolerance(p0.double(), gc, 3, v, lr, wd)
    err = (clipped[0].double() - exp).abs()
    print(f"adam_step_clip: worst |err| / tolerance {(err / tol).max().item():.3f}")
    assert bool((err <= tol).all())
    assert rel_l2(clipped[1], m) < 1e-6 and rel_l2(clipped[2], v) < 1e-6


# ------------------------------------------------------------------------------------------------
# Split weight gradient of a Linear (the LSTM weight gradients over the T*B rows)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,fin,fout,splits", [(33, 64, 256, 2), (80, 20, 256, 3), (736, 5, 256, 8), (100, 70, 30, 1)])
def test_linear_bwd_weight_splitk_vs_fp64(gpu, n, fin, fout, splits):
    gen = torch.Generator().manual_seed(n + fin)
    lib = L.lib()
    need = lib.tspm_linear_bwd_weight_splitk_workspace(n, fin, fout, splits)
    assert (need > 0) == (splits > 1)
    for ldx, ldy in ((fin, fout), (fin + 5, fout + 3)):
        x = torch.full((n, ldx), 1e30); dy = torch.full((n, ldy), 1e30)   # the padding columns are not data
        x[:, :fin] = torch.randn(n, fin, generator=gen); dy[:, :fout] = torch.randn(n, fout, generator=gen)
        xd, dyd = x.to(gpu), dy.to(gpu)

        def run(ws_bytes=need):
            dw, db = Guarded(gpu, fout, fin), Guarded(gpu, 1, fout)
            ws = Guarded(gpu, 1, max(need, 4), dtype=torch.uint8)
            st = lib.tspm_linear_bwd_weight_splitk(n, fin, fout, xd.data_ptr(), ldx, dyd.data_ptr(), ldy, dw.ptr(), db.ptr(),
                                                   splits, ws.ptr(), ws_bytes, L.stream_handle())
            _sync()
            dw.intact("splitk dw"); db.intact("splitk db"); ws.intact("splitk workspace")
            return st, dw.cpu(), db.cpu().view(fout)
        st, dw, db = run()
        assert st == 0
        st2, dw2, db2 = run()
        assert torch.equal(dw, dw2) and torch.equal(db, db2)   # the b_ih / b_hh property: same dy, same db bits
        xs, ds = x[:, :fin], dy[:, :fout]
        tag = f"n{n} in{fin} out{fout} s{splits} ld{ldx}"
        op_check(f"linear_bwd_weight_splitk.dw[{tag}]", dw, ds.T @ xs, ds.double().T @ xs.double(), grad=True, ratios=RATIOS)
        op_check(f"linear_bwd_weight_splitk.db[{tag}]", db, ds.sum(0), ds.double().sum(0), grad=True, ratios=RATIOS)
        if need:
            st, dw, _ = run(need - 4)
            assert st == 3 and bool(dw.isnan().all())   # TSPM_ERR_WORKSPACE, nothing launched
    print("worst ratios:", RATIOS)
