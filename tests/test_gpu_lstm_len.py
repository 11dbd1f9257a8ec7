"""tspm_lstm_fwd_len / tspm_lstm_bwd_len — the LSTM recurrences with per-sample sequence lengths — through the C ABI.

Reference: ``len_cell_loop`` below, a per-row loop of the LSTM cell (test_gpu_lstm_widths._cell_loop, ATen's order) over
each row's own L_b = min(max(length, 1), T) steps, zeros after, and a maximum over t < L_b; run in float32 and float64.
``test_restatement_is_pack_padded_sequence`` (CPU) holds that restatement to torch.nn.LSTM over
pack_padded_sequence(enforce_sorted=False) in float64, to 1e-12.

Criterion (tests/parity.py, as test_gpu_seq_ops.py uses it for the unmasked kernels): err_ours = rel-L2(ours, fp64) <=
FACTOR x err_ref32 + floor; exact operations (the select of h_out, the first-maximum index of our own h, the zero tails)
by torch.equal; index decisions against fp64's own through near_tie_flips with its cap.  ``gates`` and ``cs`` past a row's
length are unspecified by the ABI: both sides are masked to zero there before they are compared.  Every output is a
parity.Guarded buffer that starts as a NaN sentinel, so the tails that must be written are proven written and a stray
write is caught.

Cases (test 1): H in {4, 36, 64, 128} (one per tier plus the compile-time 64 kind), B = 5 (odd batch: a ghost row; one
workgroup with two different lengths, one with equal lengths), T = 9, lengths [9, 1, 4, 4, 7], "last" and "maxpool",
regimes "a" and "b" of the generator of test_gpu_seq_ops.py (test_gpu_lstm_widths._lstm_case, the same generator at width
H).  Row 2 (L = 4) has an exact tie planted across its length boundary: unit H-1's output gate is shut everywhere except
t = 3 and t = 4, where i = g = o = 1 and f = 0 exactly, so h = tanh(1) at both — the masked step t = 4 must not win and
the index must be 3.  ``test_fp32_restatement_stays_within_the_flip_cap`` (CPU) shows that the float32 restatement alone
makes at most max(1, 1e-4 x numel) = 1 index flip against float64 on each of these cases, so the cap is fair to the kernel.
"""
import functools

import pytest
import torch

from parity import Guarded, Ratios, near_tie_flips, op_check
from test_gpu_lstm_t16 import Guarded16
from test_gpu_lstm_widths import _Bwd, _Fwd, _cell_loop, _lstm_case, _run_bwd, _run_fwd
from test_gpu_seq_ops import _same, _sync
from tspm_amd import _lib as L

gpu_test = pytest.mark.gpu
RATIOS = Ratios()
WIDTHS = [4, 36, 64, 128]
B5, T9, LENS = 5, 9, (9, 1, 4, 4, 7)
INVALID = 1


# ------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------
def clamp_lengths(lengths, T):
    return [min(max(int(v), 1), T) for v in lengths]


def len_cell_loop(xg, whh, bhh, lengths, dtype, grad=False):
    """Row b runs the cell over its own first L_b steps (state frozen afterwards: nothing is computed).  Returns gates
    [T,B,4H] and cs [T,B,H] (zeros past L_b: unspecified by the ABI), hs [T+1,B,H] (zeros past L_b: what
    pad_packed_sequence returns) and, with ``grad``, the projected input as a leaf whose gradient is dgates (the
    pre-activation is rec + xg[t], so the two gradients are equal; zero past L_b)."""
    T, B, G = xg.shape
    H = G // 4
    lens = clamp_lengths(lengths, T)
    leaf = xg.to(dtype).clone().requires_grad_(True) if grad else xg.to(dtype)
    gates, cs, hs = [], [], []
    for b in range(B):
        Lb = lens[b]
        g, c, h, _ = _cell_loop(leaf[:Lb, b:b + 1], whh, bhh, dtype)
        gates.append(torch.cat([g[:, 0], torch.zeros(T - Lb, G, dtype=dtype)]))
        cs.append(torch.cat([c[:, 0], torch.zeros(T - Lb, H, dtype=dtype)]))
        hs.append(torch.cat([h[:, 0], torch.zeros(T - Lb, H, dtype=dtype)]))
    return torch.stack(gates, 1), torch.stack(cs, 1), torch.stack(hs, 1), leaf


def masked_pool(hs, lengths):
    """max over t < L_b of h_t and its first index -> ([B,H], [B,H]); h = hs[1:] (NaN-free inputs)."""
    T = hs.shape[0] - 1
    lens = torch.tensor(clamp_lengths(lengths, T))
    t = torch.arange(T).view(T, 1, 1)
    r = hs[1:].masked_fill(t >= lens.view(1, -1, 1), float("-inf"))
    v = r.max(0).values
    first = torch.where(r == v.unsqueeze(0), t, T).min(0).values  # the FIRST maximum (torch.max does not promise it)
    return v, first


def last_of(hs, lengths):
    T = hs.shape[0] - 1
    lens = torch.tensor(clamp_lengths(lengths, T))
    return hs[lens, torch.arange(hs.shape[1])]


def len_embedding(hs, lengths, arg=None):
    """The embedding of the restatement: h at L_b - 1 ("last") or h gathered at the given index ("maxpool")."""
    return last_of(hs, lengths) if arg is None else hs[1:].gather(0, arg.long().unsqueeze(0)).squeeze(0)


def len_bwd_ref(xg, whh, bhh, lengths, dh, arg, dtype):
    """Autograd through the restatement from loss = sum(dh * emb) -> dgates [T,B,4H] (zeros past L_b)."""
    _, _, hs, leaf = len_cell_loop(xg, whh, bhh, lengths, dtype, grad=True)
    (dh.to(dtype) * len_embedding(hs, lengths, arg)).sum().backward()
    return leaf.grad


def _valid(T, lengths):
    """[T, B, 1] mask of the (t, b) a row really runs."""
    lens = torch.tensor(clamp_lengths(lengths, T))
    return (torch.arange(T).view(T, 1) < lens.view(1, -1)).unsqueeze(2)


@functools.lru_cache(maxsize=None)
def _len_case(H, B, T, regime, lengths, seed=0, tie_row=None, plant_row=None):
    """The generator's case with the references of the restatement.  ``tie_row``: the exact tie across that row's length
    boundary (module docstring).  ``plant_row``: unit H-1 of that row has its output gate shut until the row's own last
    step, which then holds its maximum."""
    base = _lstm_case(H, B, T, regime, True, seed=seed)
    xg = base["xg"].clone()  # the cached case is shared with other test files: never written
    lens = clamp_lengths(lengths, T)
    un = H - 1
    cols = [un, H + un, 2 * H + un, 3 * H + un]
    if tie_row is not None:
        Lb = lens[tie_row]
        assert Lb < T
        xg[:, tie_row, 3 * H + un] = -40.0
        for t in (Lb - 1, Lb):
            xg[t, tie_row, cols] = torch.tensor([40.0, -40.0, 40.0, 40.0])
    if plant_row is not None:
        Lb = lens[plant_row]
        xg[:, plant_row, 3 * H + un] = -20.0
        xg[Lb - 1, plant_row, cols] = torch.tensor([20.0, -20.0, 20.0, 20.0])
    whh, bhh = base["whh"], base["bhh"]
    r32 = len_cell_loop(xg, whh, bhh, lengths, torch.float32)[:3]
    r64 = len_cell_loop(xg, whh, bhh, lengths, torch.float64)[:3]
    return dict(xg=xg, whh=whh, bhh=bhh, r32=r32, r64=r64, B=B, T=T, H=H, lengths=tuple(lengths))


def _case1(H, regime):
    return _len_case(H, B5, T9, regime, LENS, tie_row=2)


# ------------------------------------------------------------------------------------------------
# CPU checks of the reference itself (not marked gpu)
# ------------------------------------------------------------------------------------------------
def test_restatement_is_pack_padded_sequence():
    """The restatement against torch.nn.LSTM over pack_padded_sequence(enforce_sorted=False) in float64: the padded
    output (zeros past each length), h_n ("last") and the masked maximum, forward and gradient, to 1e-12."""
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    torch.manual_seed(0)
    for H in (4, 36):
        feat = 7
        rnn = torch.nn.LSTM(feat, H, batch_first=True).double()
        x = torch.randn(B5, T9, feat, dtype=torch.float64)
        lens = torch.tensor(LENS)
        packed = pack_padded_sequence(x, lens, batch_first=True, enforce_sorted=False)
        out, (hn, _) = rnn(packed)
        r_out, _ = pad_packed_sequence(out, batch_first=True, total_length=T9)  # [B, T, H]
        xg = (x.transpose(0, 1).reshape(T9 * B5, feat) @ rnn.weight_ih_l0.T + rnn.bias_ih_l0).reshape(T9, B5, 4 * H)
        xg = xg.detach()
        whh, bhh = rnn.weight_hh_l0.detach(), rnn.bias_hh_l0.detach()
        _, _, hs, _ = len_cell_loop(xg, whh, bhh, LENS, torch.float64)
        assert (hs[1:].transpose(0, 1) - r_out).abs().max().item() <= 1e-12
        assert (last_of(hs, LENS) - hn[0]).abs().max().item() <= 1e-12
        # the masked maximum: over the packed steps only
        want = torch.stack([r_out[b, :LENS[b]].max(0).values for b in range(B5)])
        got, idx = masked_pool(hs, LENS)
        assert (got - want).abs().max().item() <= 1e-12 and bool((idx < lens.view(-1, 1)).all())
        # gradient of sum(dh * h_n) with respect to the projected input
        dh = torch.randn(B5, H, dtype=torch.float64)
        xl = x.clone().requires_grad_(True)
        _, (hn2, _) = rnn(pack_padded_sequence(xl, lens, batch_first=True, enforce_sorted=False))
        (dh * hn2[0]).sum().backward()
        dg = len_bwd_ref(xg, whh, bhh, LENS, dh, None, torch.float64)  # [T, B, 4H]
        dx = (dg.reshape(T9 * B5, 4 * H) @ rnn.weight_ih_l0.detach()).reshape(T9, B5, feat).transpose(0, 1)
        assert (dx - xl.grad).abs().max().item() <= 1e-12


@pytest.mark.parametrize("regime", ["a", "b"])
@pytest.mark.parametrize("H", WIDTHS)
def test_fp32_restatement_stays_within_the_flip_cap(H, regime):
    """On the cases of test 1 the float32 restatement alone stays within near_tie_flips' cap against float64, and the
    planted tie resolves to the step before the boundary in both."""
    case = _case1(H, regime)
    _, i32 = masked_pool(case["r32"][2], LENS)
    _, i64 = masked_pool(case["r64"][2], LENS)
    near_tie_flips(f"fp32 restatement H{H} {regime}", i32, i64, case["r64"][2][1:].permute(1, 2, 0), 2)
    assert i32[2, H - 1].item() == 3 and i64[2, H - 1].item() == 3
    # the planted values are equal on both sides of the boundary in an unmasked run of the same cell
    full = _cell_loop(case["xg"], case["whh"], case["bhh"], torch.float32)[2]
    assert full[4, 2, H - 1].item() == full[5, 2, H - 1].item() > 0


# ------------------------------------------------------------------------------------------------
# device buffers
# ------------------------------------------------------------------------------------------------
class _FwdLen(_Fwd):
    """test_gpu_lstm_widths._Fwd plus the device lengths and the index width (8: uint8 buffer, 16: int16 storage)."""

    def __init__(self, gpu, xg, whh, bhh, maxpool, ld, lengths, bits=8):
        super().__init__(gpu, xg, whh, bhh, maxpool and bits == 8, ld)
        self.maxpool, self.bits = maxpool, bits
        if maxpool and bits != 8:
            self.arg = Guarded16(gpu, self.B, self.H)
        self.lengths = None if lengths is None else torch.tensor(list(lengths), dtype=torch.int32, device=gpu)

    def desc(self):
        d = L.LstmFwdLenDesc(self.B, self.T, self.H, self.ld, self.xg.data_ptr(), self.whh.data_ptr(), L.ptr(self.bhh),
                             self.gates.ptr(), self.cs.ptr(), self.hs.ptr(), self.hout.ptr(),
                             self.arg.ptr() if self.arg else None)
        d.lengths, d.index_bits = L.ptr(self.lengths), self.bits
        return d

    def outputs(self):
        o = super().outputs()
        if self.arg:
            o["arg"] = o["arg"].long()
        return o


def _run_fwd_len(gpu, specs, expect=0):
    """specs: list of (xg, whh, bhh, maxpool, ld, lengths[, bits]) -> list of (_FwdLen, outputs) from ONE call."""
    fs = [_FwdLen(gpu, *s) for s in specs]
    descs = (L.LstmFwdLenDesc * len(fs))(*[f.desc() for f in fs])
    rc = L.lib().tspm_lstm_fwd_len(len(fs), descs, L.stream_handle())
    _sync()
    assert rc == expect, f"tspm_lstm_fwd_len returned {rc}, expected {expect}"
    for f in fs:
        f.intact()
    return [(f, f.outputs()) for f in fs]


class _BwdLen(_Bwd):
    def desc(self):
        f = self.f
        d = L.LstmBwdLenDesc(f.B, f.T, f.H, self.ld, f.whh.data_ptr(), f.gates.ptr(), f.cs.ptr(), self.dh.data_ptr(),
                             self.dgates.ptr(), f.arg.ptr() if f.arg else None)
        d.lengths, d.index_bits = L.ptr(f.lengths), f.bits
        return d


def _run_bwd_len(gpu, specs, expect=0):
    """specs: list of (_FwdLen, dh [B,H] cpu, ld_dh) -> list of dgates [T,B,4H] (cpu) from ONE call."""
    bs = [_BwdLen(gpu, *s) for s in specs]
    descs = (L.LstmBwdLenDesc * len(bs))(*[b.desc() for b in bs])
    rc = L.lib().tspm_lstm_bwd_len(len(bs), descs, L.stream_handle())
    _sync()
    assert rc == expect, f"tspm_lstm_bwd_len returned {rc}, expected {expect}"
    for b in bs:
        b.dgates.intact(f"lstm_bwd_len H{b.f.H} dgates")
    return [b.dgates.cpu().view(b.f.T, b.f.B, 4 * b.f.H) for b in bs]


def _is_pos_zero(t):
    return bool(((t == 0) & ~torch.signbit(t)).all())


def _check_tails(o, dg, lengths):
    """hs[t+1][b] and dgates[t][b] are exactly +0.0 for t >= L_b (the buffers started as the NaN sentinel)."""
    T = o["hs"].shape[0] - 1
    for b, Lb in enumerate(clamp_lengths(lengths, T)):
        assert _is_pos_zero(o["hs"][Lb + 1:, b]), f"hs tail of row {b}"
        if dg is not None:
            assert _is_pos_zero(dg[Lb:, b]), f"dgates tail of row {b}"
        assert not bool(o["hs"][1:Lb + 1, b].isnan().any()) and not bool(o["gates"][:Lb, b].isnan().any())


def _check_fwd_len(tag, case, o, maxpool, lengths, count_flips=True):
    g32, c32, h32 = case["r32"]
    g64, c64, h64 = case["r64"]
    T = case["T"]
    ok = _valid(T, lengths)
    zero = torch.zeros(())
    op_check(f"lstm_fwd_len.gates[{tag}]", torch.where(ok, o["gates"], zero), g32, g64, ratios=RATIOS)
    op_check(f"lstm_fwd_len.cs[{tag}]", torch.where(ok, o["cs"], zero), c32, c64, ratios=RATIOS)
    op_check(f"lstm_fwd_len.hs[{tag}]", o["hs"], h32, h64, ratios=RATIOS)
    assert bool((o["hs"][0] == 0).all()), "hs[0] must be the zero initial state"
    lens = torch.tensor(clamp_lengths(lengths, T))
    if maxpool:
        v32, _ = masked_pool(h32, lengths)
        v64, i64 = masked_pool(h64, lengths)
        op_check(f"lstm_fwd_len.h_out[{tag}]", o["hout"], v32, v64, ratios=RATIOS)
        arg = o["arg"]
        assert bool((arg < lens.view(-1, 1)).all()), f"{tag}: an index at or past its row's length"
        if count_flips:
            nf = near_tie_flips(f"lstm_fwd_len.argmax[{tag}]", arg, i64, h64[1:].permute(1, 2, 0), 2)
            print(f"lstm_fwd_len.argmax[{tag}]: {nf} flips of {arg.numel()}")
        # exact: h_out is our own h at our own index, which is the first maximum of our own h over t < L_b
        assert torch.equal(o["hout"], o["hs"][1:].gather(0, arg.unsqueeze(0)).squeeze(0))
        assert torch.equal(arg, masked_pool(o["hs"], lengths)[1])
    else:
        op_check(f"lstm_fwd_len.h_out[{tag}]", o["hout"], last_of(h32, lengths), last_of(h64, lengths), ratios=RATIOS)
        assert torch.equal(o["hout"], last_of(o["hs"], lengths))


def _check_bwd_len(tag, case, dg, dh, arg, lengths):
    a = (case["xg"], case["whh"], case["bhh"], lengths, dh, arg)
    r32, r64 = len_bwd_ref(*a, torch.float32), len_bwd_ref(*a, torch.float64)
    op_check(f"lstm_bwd_len.dgates[{tag}]", dg, r32, r64, grad=True, ratios=RATIOS)


# ------------------------------------------------------------------------------------------------
# 1. against fp64 (tails and guards, test 4, are checked on the same runs)
# ------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("regime", ["a", "b"])
@pytest.mark.parametrize("mode", ["last", "maxpool"])
@pytest.mark.parametrize("H", WIDTHS)
def test_lstm_len_vs_fp64(gpu, H, mode, regime):
    maxpool = mode == "maxpool"
    case = _case1(H, regime)
    tag = f"H{H} {mode} {regime}"
    spec = (case["xg"], case["whh"], case["bhh"], maxpool, H + 12, LENS)
    (f, o), = _run_fwd_len(gpu, [spec])
    (_, o2), = _run_fwd_len(gpu, [spec])
    assert all(_same(o[k], o2[k]) for k in o), "lstm_fwd_len is not deterministic"
    _check_fwd_len(tag, case, o, maxpool, LENS)
    if maxpool:  # the planted tie: the step before the boundary, never the masked one
        assert o["arg"][2, H - 1].item() == 3
    dh = torch.randn(B5, H, generator=torch.Generator().manual_seed(H))
    dg, = _run_bwd_len(gpu, [(f, dh, H + 12)])
    dg2, = _run_bwd_len(gpu, [(f, dh, H + 12)])
    assert torch.equal(dg, dg2), "lstm_bwd_len is not deterministic"
    _check_bwd_len(tag, case, dg, dh, o.get("arg"), LENS)
    _check_tails(o, dg, LENS)  # 4. the tails are +0.0, written over the NaN sentinel; guards checked by the runners
    print("worst ratios:", RATIOS)


# ------------------------------------------------------------------------------------------------
# 2. all lengths equal to steps: bitwise the unmasked entry points
# ------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("T,bits,mode", [(9, 8, "last"), (9, 8, "maxpool"), (300, 16, "maxpool"), (300, 16, "last")])
@pytest.mark.parametrize("H", WIDTHS)
def test_full_lengths_are_bitwise_the_unmasked_entry_points(gpu, H, T, bits, mode):
    from test_gpu_lstm_t16 import _run_bwd16, _run_fwd16
    maxpool = mode == "maxpool"
    B = 5
    case = _lstm_case(H, B, T, "a", True)
    spec = (case["xg"], case["whh"], case["bhh"], maxpool, H + 12)
    dh = torch.randn(B, H, generator=torch.Generator().manual_seed(T))
    (fl, ol), = _run_fwd_len(gpu, [spec + ((T,) * B, bits)])
    gl, = _run_bwd_len(gpu, [(fl, dh, H + 4)])
    if bits == 16:
        (fu, ou), = _run_fwd16(gpu, [spec])
        gu, = _run_bwd16(gpu, [(fu, dh, H + 4)])
    else:
        (fu, ou), = _run_fwd(gpu, [spec])
        gu, = _run_bwd(gpu, [(fu, dh, H + 4)])
    assert ol.keys() == ou.keys()
    for k in ("gates", "cs", "hs", "hout"):
        assert torch.equal(ol[k], ou[k]), k
    if maxpool:
        assert torch.equal(ol["arg"], ou["arg"].long())
    assert torch.equal(gl, gu)


# ------------------------------------------------------------------------------------------------
# 3. row independence: a row of length L is bitwise that row of an unmasked run of L steps
# ------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("mode", ["last", "maxpool"])
@pytest.mark.parametrize("H", WIDTHS)
def test_rows_equal_unmasked_runs_of_their_own_length(gpu, H, mode):
    maxpool = mode == "maxpool"
    case = _case1(H, "a")
    dh = torch.randn(B5, H, generator=torch.Generator().manual_seed(H + 1))
    (f, o), = _run_fwd_len(gpu, [(case["xg"], case["whh"], case["bhh"], maxpool, H, LENS)])
    dg, = _run_bwd_len(gpu, [(f, dh, H)])
    for Lv in sorted(set(LENS)):
        (fu, ou), = _run_fwd(gpu, [(case["xg"][:Lv].contiguous(), case["whh"], case["bhh"], maxpool, H)])
        gu, = _run_bwd(gpu, [(fu, dh, H)])
        rows = [b for b in range(B5) if LENS[b] == Lv]
        assert rows
        for b in rows:
            assert torch.equal(o["hout"][b], ou["hout"][b]), (Lv, b)
            assert torch.equal(o["gates"][:Lv, b], ou["gates"][:, b]) and torch.equal(o["cs"][:Lv, b], ou["cs"][:, b])
            assert torch.equal(o["hs"][:Lv + 1, b], ou["hs"][:, b])
            if maxpool:
                assert torch.equal(o["arg"][b], ou["arg"][b].long())
            assert torch.equal(dg[:Lv, b], gu[:, b]), (Lv, b)


# ------------------------------------------------------------------------------------------------
# 5. clamping
# ------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("mode", ["last", "maxpool"])
@pytest.mark.parametrize("H", [4, 64, 100])
def test_lengths_are_clamped_to_1_steps(gpu, H, mode):
    maxpool = mode == "maxpool"
    T = T9
    case = _lstm_case(H, B5, T, "a", True)
    dh = torch.randn(B5, H, generator=torch.Generator().manual_seed(3))
    res = []
    for lens in ((0, -3, T + 3, T, 1), (1, 1, T, T, 1)):
        (f, o), = _run_fwd_len(gpu, [(case["xg"], case["whh"], case["bhh"], maxpool, H, lens)])
        dg, = _run_bwd_len(gpu, [(f, dh, H)])
        _check_tails(o, dg, lens)
        res.append((o, dg))
    (oa, ga), (ob, gb) = res
    assert all(_same(oa[k], ob[k]) for k in oa)  # the unspecified rows stay the NaN sentinel on both sides
    assert torch.equal(ga, gb)


# ------------------------------------------------------------------------------------------------
# 6. wide index
# ------------------------------------------------------------------------------------------------
@gpu_test
def test_wide_index_with_lengths_vs_fp64(gpu):
    H, B, T = 8, 5, 300
    lens = (300, 257, 1, 256, 130)
    case = _len_case(H, B, T, "a", lens, plant_row=1)  # row 1's unit H-1 peaks at its own last step: index 256
    assert masked_pool(case["r64"][2], lens)[1][1, H - 1].item() == 256
    (f, o), = _run_fwd_len(gpu, [(case["xg"], case["whh"], case["bhh"], True, H + 12, lens, 16)])
    _check_fwd_len("wide", case, o, True, lens)
    assert o["arg"][1, H - 1].item() == 256 and int((o["arg"] > 255).sum()) >= 1
    dh = torch.randn(B, H, generator=torch.Generator().manual_seed(6))
    dg, = _run_bwd_len(gpu, [(f, dh, H + 12)])
    _check_bwd_len("wide", case, dg, dh, o["arg"], lens)
    _check_tails(o, dg, lens)


# ------------------------------------------------------------------------------------------------
# 7. two descriptors
# ------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("ha,hb", [(36, 60), (64, 36), (128, 100), (4, 64)])
def test_two_descriptors_equal_single_calls_in_both_orders(gpu, ha, hb):
    """Different T, H and lengths; (36, 60) and (128, 100) share a kernel kind and a launch, (64, 36) and (4, 64) take one
    launch each."""
    a, b = _lstm_case(ha, 5, 9, "a", True, seed=1), _lstm_case(hb, 3, 14, "a", True, seed=2)
    la, lb = (9, 1, 4, 4, 7), (2, 14, 5)
    specs = [(a["xg"], a["whh"], a["bhh"], True, ha + 12, la), (b["xg"], b["whh"], b["bhh"], False, hb, lb)]
    dhs = [torch.randn(5, ha, generator=torch.Generator().manual_seed(5)),
           torch.randn(3, hb, generator=torch.Generator().manual_seed(6))]
    single = [_run_fwd_len(gpu, [s])[0] for s in specs]
    gs = [_run_bwd_len(gpu, [(single[i][0], dhs[i], (ha, hb + 12)[i])])[0] for i in range(2)]
    for order in ((0, 1), (1, 0)):
        pair = _run_fwd_len(gpu, [specs[i] for i in order])
        for (_, op), i in zip(pair, order):
            os_ = single[i][1]
            assert op.keys() == os_.keys() and all(_same(op[k], os_[k]) for k in op), (order, i)
        gp = _run_bwd_len(gpu, [(pair[j][0], dhs[i], (ha, hb + 12)[i]) for j, i in enumerate(order)])
        for g, i in zip(gp, order):
            assert torch.equal(g, gs[i]), (order, i)


# ------------------------------------------------------------------------------------------------
# 8. status codes
# ------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("what", ["null_lengths", "bits8_257_steps", "bits12", "hidden130"])
def test_invalid_descriptors_are_refused_before_any_launch(gpu, what):
    H, B, T, bits, lens = 36, 2, 9, 8, (9, 4)
    if what == "bits8_257_steps":
        T, lens = 257, (257, 4)
    if what == "bits12":
        bits = 12
    if what == "hidden130":
        H = 132  # a multiple of 4 for the generator; the descriptor says 130 below
    case = _lstm_case(H, B, T, "a", True)
    f = _FwdLen(gpu, case["xg"], case["whh"], case["bhh"], True, H, None if what == "null_lengths" else lens,
                8 if bits == 12 else bits)
    d = f.desc()
    d.index_bits = bits
    if what == "hidden130":
        d.hidden = 130
    good = _FwdLen(gpu, case["xg"], case["whh"], case["bhh"], True, H, lens) if what != "hidden130" else None
    for descs in ([d], [good.desc(), d] if good is not None and what != "bits8_257_steps" else []):
        if not descs:
            continue
        arr = (L.LstmFwdLenDesc * len(descs))(*descs)
        assert L.lib().tspm_lstm_fwd_len(len(descs), arr, L.stream_handle()) == INVALID, what
    _sync()
    f.intact()
    for n in ("gates", "cs", "hs", "hout", "arg"):  # nothing launched: every output is still the sentinel
        g = getattr(f, n)
        bits_ = g.flat.cpu()
        assert bool((bits_ != bits_).all()) if bits_.is_floating_point() else bool((bits_ == 0xA5).all()), n
    if good is not None:  # ... including the valid descriptor that came first in the same call
        assert bool(good.hout.flat.cpu().isnan().all())
    dh = torch.zeros(B, H, device=gpu)
    dg = Guarded(gpu, T * B, 4 * H)
    b = L.LstmBwdLenDesc(B, T, d.hidden, H, f.whh.data_ptr(), f.gates.ptr(), f.cs.ptr(), dh.data_ptr(), dg.ptr(),
                         f.arg.ptr())
    b.lengths, b.index_bits = L.ptr(f.lengths), bits
    assert L.lib().tspm_lstm_bwd_len(1, (L.LstmBwdLenDesc * 1)(b), L.stream_handle()) == INVALID, what
    _sync()
    assert bool(dg.flat.cpu().isnan().all())
