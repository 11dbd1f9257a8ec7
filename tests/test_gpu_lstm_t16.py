"""tspm_lstm_fwd_t16 / tspm_lstm_bwd_t16 — the LSTM recurrences with a 16-bit "maxpool" time index — through the C ABI
against the plain-torch float64 restatement of test_gpu_lstm_widths.py, whose cases, buffers and checks are reused.

Criterion (tests/parity.py): err_ours = rel-L2(ours, fp64) <= FACTOR x err_ref32 + floor, ref32 the same restatement in
float32 — it adapts to the sequence length by itself; exact operations (the select of h_out, the first-maximum index of our
own h) by torch.equal; index decisions against fp64's own through near_tie_flips with its cap.  Every output is followed
by a sentinel guard region (the 16-bit index buffer too) and every call runs twice for bitwise determinism.

Widths 4 (one float4), 36 (idle lanes), 64 (the compile-time kernels), 128 (the top tier); regimes "a" and "b".
(B=2, T=257) has the maximum of unit H-1 of the last row planted at the last step: its index is exactly 256, which an
8-bit index would store as 0.  (B=3, T=300) is an odd batch (a ghost row); there the inputs are first shown, on the fp64
restatement alone, to put at least 8 maxima at steps >= 256 at widths 36 / 64 / 128 (seed 0, with b_hh: 18 / 11, 25 / 32,
73 / 68 in regimes a / b on the CPU; 1 / 1 at width 4, which relies on the planted case).  With this generator the fp32
restatement makes at most one flip against fp64 on every case below, each a near-tie, except width 4 in regime "b" at
(2, 257), where the fp32 reference itself flips 2 of 8 decisions (saturated h ties over many steps, as at (2, 256) in
test_gpu_lstm_widths.py): there the values, the planted index and the self-consistency are checked and the flip count is
left out, as that file does.

The 16-bit index buffer is int16 storage holding the unsigned pattern, as the engine allocates it; it is read through
``_lib.index_to_int64``.  An index past that storage's sign bit (32769, at T = 32770) is checked without a CPU recurrence,
which would take minutes: by the kernel's self-consistency and by the backward, which must be bitwise the "last"
backward when the only gradient enters at the planted last step.
"""
import pytest
import torch

from parity import FACTOR, FLOOR_GRAD, GUARD, Guarded, Ratios, op_check, rel_l2
from test_gpu_lstm_widths import _Fwd, _bwd_ref, _check_fwd, _lstm_case, _run_bwd, _run_fwd
from test_gpu_seq_ops import _pool_time, _same, _sync
from tspm_amd import _lib as L

pytestmark = pytest.mark.gpu
RATIOS = Ratios()
WIDTHS = [4, 36, 64, 128]
INVALID = 1
NO_FLIP_COUNT = {(4, "b", 2, 257)}  # the fp32 reference itself exceeds the cap (module docstring)
SENTINEL16 = 0xA5A5 - 0x10000  # the guard pattern as an int16 value


class Guarded16:
    """parity.Guarded for the 16-bit index: int16 storage (the unsigned pattern), the same guard region."""

    def __init__(self, dev, rows, width):
        self.rows, self.width = rows, width
        self.flat = torch.full((rows * width + GUARD,), SENTINEL16, dtype=torch.int16, device=dev)

    def ptr(self):
        return self.flat.data_ptr()

    def cpu(self):
        """The index values as int64 (widened without sign extension)."""
        return L.index_to_int64(self.flat[:self.rows * self.width].view(self.rows, self.width).cpu()).contiguous()

    def intact(self, name="index"):
        assert bool((self.flat[self.rows * self.width:].cpu() == SENTINEL16).all()), f"{name}: wrote past its last element"


class _Fwd16(_Fwd):
    """test_gpu_lstm_widths._Fwd with a 16-bit index buffer."""

    def __init__(self, gpu, xg, whh, bhh, maxpool, ld):
        super().__init__(gpu, xg, whh, bhh, False, ld)
        self.maxpool = maxpool
        self.arg = Guarded16(gpu, self.B, self.H) if maxpool else None


def _run_fwd16(gpu, specs, entry="tspm_lstm_fwd_t16"):
    """specs: list of (xg, whh, bhh, maxpool, ld) -> list of (_Fwd16, outputs) from ONE call."""
    fs = [_Fwd16(gpu, *s) for s in specs]
    descs = (L.LstmFwdDesc * len(fs))(*[f.desc() for f in fs])
    L.check(getattr(L.lib(), entry)(len(fs), descs, L.stream_handle()), entry)
    _sync()
    for f in fs:
        f.intact()
    return [(f, f.outputs()) for f in fs]


def _run_bwd16(gpu, specs):
    return _run_bwd(gpu, specs, entry="tspm_lstm_bwd_t16")


def _check_bwd(tag, case, dg, dh, arg):
    """The backward checks of test_gpu_lstm_widths.test_lstm_bwd_w_vs_fp64: the whole tensor, then step by step (an
    error confined to one step cannot hide in the whole-tensor norm) with that file's stated sub-normal allowance — a
    live step whose fp64 gradient has rms < 1e-30 is held to the same per-step bound plus 2^-126 x sqrt(numel)."""
    T = case["T"]
    r32, r64 = _bwd_ref(case, dh, arg, torch.float32), _bwd_ref(case, dh, arg, torch.float64)
    op_check(f"lstm_bwd_t16.dgates[{tag}]", dg, r32, r64, grad=True, ratios=RATIOS)
    eo = [rel_l2(dg[t], r64[t]) for t in range(T)]
    er = [rel_l2(r32[t], r64[t]) for t in range(T)]
    live = [t for t in range(T) if r64[t].abs().max() > 0]
    for t in range(T):
        if t not in live:
            assert bool((dg[t] == 0).all()), f"{tag}: step {t} has no gradient and must be exact zeros"
    full = [t for t in live if r64[t].pow(2).mean().sqrt() >= 1e-30]
    assert full, tag
    mo, mr = max(eo[t] for t in full), max(er[t] for t in full)
    print(f"lstm_bwd_t16.dgates per step[{tag}]: max err_ours {mo:.3e} max err_ref32 {mr:.3e} ({len(full)} of "
          f"{len(live)} live steps at full precision)")
    RATIOS.note("lstm_bwd_t16.dgates/step", mo, mr)
    assert mo <= FACTOR * mr + FLOOR_GRAD, (tag, mo, mr)
    for t in full:
        assert eo[t] <= FACTOR * er[t] + FLOOR_GRAD, (tag, t, eo[t], er[t])
    for t in live:
        if t not in full:
            ao, n64 = float((dg[t].double() - r64[t]).norm()), float(r64[t].norm())
            assert ao <= (FACTOR * er[t] + FLOOR_GRAD) * n64 + 2.0 ** -126 * dg[t].numel() ** 0.5, (tag, t, ao, n64, er[t])


@pytest.mark.parametrize("regime", ["a", "b"])
@pytest.mark.parametrize("B,T", [(2, 257), (3, 300)])
@pytest.mark.parametrize("H", WIDTHS)
def test_lstm_t16_vs_fp64(gpu, H, B, T, regime):
    """Forward and backward past 256 steps with the "maxpool" embedding against fp64."""
    plant = (B, T) == (2, 257)
    case = _lstm_case(H, B, T, regime, True, plant_last=plant)
    i64 = _pool_time(case["r64"][2])[1]
    # conditions on the inputs, on the fp64 restatement alone, before the kernel is looked at
    if plant:
        assert i64[B - 1, H - 1].item() == 256
    elif H != 4:
        assert int((i64 >= 256).sum()) >= 8, f"H{H} {regime}: only {int((i64 >= 256).sum())} reference indices >= 256"
    tag = f"H{H} B{B} T{T} maxpool {regime}"
    spec = (case["xg"], case["whh"], case["bhh"], True, H + 12)
    (f, o), = _run_fwd16(gpu, [spec])
    (_, o2), = _run_fwd16(gpu, [spec])
    assert all(_same(o[k], o2[k]) for k in o), "lstm_fwd_t16 is not deterministic"
    # values against fp64, flips through near_tie_flips with its cap, h_out = our own h at our own index, the index =
    # the first maximum of our own h
    _check_fwd(tag, case, o, True, count_flips=(H, regime, B, T) not in NO_FLIP_COUNT)
    print(f"lstm_fwd_t16.argmax[{tag}]: {int((o['arg'] >= 256).sum())} of {o['arg'].numel()} indices >= 256")
    if plant:
        assert o["arg"][B - 1, H - 1].item() == 256
        assert o["arg"][B - 1, H - 1].item() & 0xFF == 0  # what an 8-bit index would have read
    dh = torch.randn(B, H, generator=torch.Generator().manual_seed(B * 1000 + T))
    dg, = _run_bwd16(gpu, [(f, dh, H + 12)])
    dg2, = _run_bwd16(gpu, [(f, dh, H + 12)])
    assert torch.equal(dg, dg2), "lstm_bwd_t16 is not deterministic"
    _check_bwd(tag, case, dg, dh, o["arg"])  # the gradient enters at the kernel's own index
    print("worst ratios:", RATIOS)


@pytest.mark.parametrize("B,T,mode", [(5, 37, "maxpool"), (2, 256, "maxpool"), (2, 300, "last")])
@pytest.mark.parametrize("H", WIDTHS)
def test_t16_is_bitwise_the_8_bit_path_where_both_apply(gpu, H, B, T, mode):
    """With an index and steps <= 256, and without an index at any length, tspm_lstm_fwd_t16 / _bwd_t16 give bitwise
    tspm_lstm_fwd_w / _bwd_w's gates, cs, hs, h_out and dgates, and index values equal as integers; at width 64 also
    tspm_lstm_fwd / _bwd's."""
    maxpool = mode == "maxpool"
    case = _lstm_case(H, B, T, "a", True, plant_last=(B, T) == (2, 256))
    spec = (case["xg"], case["whh"], case["bhh"], maxpool, H + 12)
    dh = torch.randn(B, H, generator=torch.Generator().manual_seed(T))
    (f16, o16), = _run_fwd16(gpu, [spec])
    g16, = _run_bwd16(gpu, [(f16, dh, H + 4)])
    for fwd, bwd in ([("tspm_lstm_fwd_w", "tspm_lstm_bwd_w")] + ([("tspm_lstm_fwd", "tspm_lstm_bwd")] if H == 64 else [])):
        (f8, o8), = _run_fwd(gpu, [spec], entry=fwd)
        assert o8.keys() == o16.keys()
        for k in ("gates", "cs", "hs", "hout"):
            assert torch.equal(o16[k], o8[k]), (fwd, k)
        if maxpool:
            assert o8["arg"].dtype == torch.uint8 and torch.equal(o16["arg"], o8["arg"].long()), fwd
        g8, = _run_bwd(gpu, [(f8, dh, H + 4)], entry=bwd)
        assert torch.equal(g16, g8), bwd
    if (B, T) == (2, 256):
        assert o16["arg"][B - 1, H - 1].item() == 255


@pytest.mark.parametrize("ha,hb", [(36, 128), (36, 60), (128, 100), (64, 36), (4, 64)])
def test_two_descriptors_of_different_steps_equal_single_calls(gpu, ha, hb):
    """5 steps and 300 steps, different widths and batches, in one call — one launch when the kernel tiers agree, two
    otherwise — are bitwise two count-1 calls, forward and backward."""
    a, b = _lstm_case(ha, 5, 5, "a", True, seed=1), _lstm_case(hb, 3, 300, "a", True, seed=0)
    specs = [(a["xg"], a["whh"], a["bhh"], True, ha + 12), (b["xg"], b["whh"], b["bhh"], True, hb)]
    dhs = [torch.randn(5, ha, generator=torch.Generator().manual_seed(5)),
           torch.randn(3, hb, generator=torch.Generator().manual_seed(6))]
    pair = _run_fwd16(gpu, specs)
    single = [_run_fwd16(gpu, [s])[0] for s in specs]
    for (_, op), (_, os_) in zip(pair, single):
        assert op.keys() == os_.keys() and all(torch.equal(op[k], os_[k]) for k in op)
    _check_fwd(f"pair H{ha} T5", a, pair[0][1], True)
    _check_fwd(f"pair H{hb} T300", b, pair[1][1], True)
    gp = _run_bwd16(gpu, [(pair[0][0], dhs[0], ha), (pair[1][0], dhs[1], hb + 12)])
    gs = [_run_bwd16(gpu, [(single[0][0], dhs[0], ha)])[0], _run_bwd16(gpu, [(single[1][0], dhs[1], hb + 12)])[0]]
    assert torch.equal(gp[0], gs[0]) and torch.equal(gp[1], gs[1])


def test_the_8_bit_entry_points_still_refuse_257_indexed_steps(gpu):
    case = _lstm_case(36, 2, 257, "a", True, plant_last=True)
    f = _Fwd(gpu, case["xg"], case["whh"], case["bhh"], True, 36)
    d = (L.LstmFwdDesc * 1)(f.desc())
    assert L.lib().tspm_lstm_fwd_w(1, d, L.stream_handle()) == INVALID
    dh = torch.zeros(2, 36, device=gpu)
    dg = Guarded(gpu, 257 * 2, 4 * 36)
    b = (L.LstmBwdDesc * 1)(L.LstmBwdDesc(2, 257, 36, 36, f.whh.data_ptr(), f.gates.ptr(), f.cs.ptr(), dh.data_ptr(),
                                          dg.ptr(), f.arg.ptr()))
    assert L.lib().tspm_lstm_bwd_w(1, b, L.stream_handle()) == INVALID
    _sync()
    f.intact()  # a refused call wrote nothing
    dg.intact("refused lstm_bwd_w dgates")


def test_index_past_the_sign_bit_of_the_int16_storage(gpu):
    """T = 32770, width 4, the maximum of unit H-1 of the last row planted at the last step: the stored index is 32769
    (0x8001: negative as int16, widened by index_to_int64), every index is the first maximum of the kernel's own h,
    h_out is that h, and a gradient that enters only at the planted unit gives bitwise the "last" backward (whose
    gradient enters at step T-1) — an index read as anything but 32769 would put it elsewhere."""
    H, B, T = 4, 2, 32770
    g = torch.Generator().manual_seed(0)
    k = 1.0 / H ** 0.5
    whh, bhh = (torch.rand(4 * H, H, generator=g) * 2 - 1) * k, (torch.rand(4 * H, generator=g) * 2 - 1) * k
    xg = torch.randn(T, B, 4 * H, generator=g)
    xg[:, B - 1, 3 * H + H - 1] = -20.0  # the output gate of the planted unit stays shut ...
    xg[T - 1, B - 1, [H - 1, 2 * H - 1, 3 * H - 1, 4 * H - 1]] = torch.tensor([20.0, -20.0, 20.0, 20.0])  # ... until the end
    (f, o), = _run_fwd16(gpu, [(xg, whh, bhh, True, H)])
    assert int(f.arg.flat[(B - 1) * H + H - 1].item()) == 32769 - 65536  # the raw int16 pattern
    assert o["arg"][B - 1, H - 1].item() == 32769
    assert torch.equal(o["arg"], _pool_time(o["hs"])[1])
    assert torch.equal(o["hout"], o["hs"][1:].gather(0, o["arg"].unsqueeze(0)).squeeze(0))
    dh = torch.zeros(B, H)
    dh[B - 1, H - 1] = 1.5
    dg, = _run_bwd16(gpu, [(f, dh, H)])
    (fl, _), = _run_fwd16(gpu, [(xg, whh, bhh, False, H)])
    dgl, = _run_bwd16(gpu, [(fl, dh, H)])
    assert bool(dg[T - 1, B - 1].abs().sum() > 0) and torch.equal(dg, dgl)
