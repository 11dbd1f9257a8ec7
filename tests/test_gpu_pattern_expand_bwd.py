"""``tspm_pattern_expand_bwd`` on the device, through ctypes into guarded outputs, against a host restatement: a float32
loop that adds the patterns in ascending order from +0.0 - plain fp32 adds, which is all the kernel does, so the
comparison is bitwise.  Widths (8, 12, 8) with ld = E run the 16-byte path; (8, 12, 7) and (4, 4, 5) with padded, odd
leading dimensions the one-float path.  One adjoint identity in fp64 ties it to ``tspm_pattern_expand``."""
import ctypes

import pytest
import torch

from parity import Guarded
from tspm_amd import _lib as L
from tspm_amd.mosi_data import PATTERNS

pytestmark = pytest.mark.gpu
LETTERS = "avt"  # the column order of the embeddings: cat(audio, video, text)


def _cols(widths):
    return [0, widths[0], widths[0] + widths[1], sum(widths)]


def _restate(dout, B, patterns, widths, mods=7):
    """(demb [2B, E] float32 with NaN where nothing is written, used [2B, 3] bool) on the host: ascending p, fp32 adds."""
    c = _cols(widths)
    demb = torch.full((2 * B, sum(widths)), float("nan"), dtype=torch.float32)
    used = torch.zeros(2 * B, 3, dtype=torch.bool)
    for m, ch in enumerate(LETTERS):
        if not (mods >> m) & 1:
            continue
        for half in (0, 1):
            acc = torch.zeros(B, widths[m], dtype=torch.float32)  # +0.0
            for p, name in enumerate(patterns):
                if (ch in name) == (half == 0):
                    acc = acc + dout[p * B:(p + 1) * B, c[m]:c[m + 1]]
                    used[half * B:(half + 1) * B, m] = True
            demb[half * B:(half + 1) * B, c[m]:c[m + 1]] = acc
    return demb, used


def _run(gpu, B, patterns, widths, ld_dout, ld_demb, dout_full, mods=7):
    P, E = len(patterns), sum(widths)
    demb = Guarded(gpu, 2 * B, E, ld_demb)
    keep = (ctypes.c_int32 * (3 * P))(*[int(ch in name) for name in patterns for ch in LETTERS])
    d = dout_full.to(gpu)
    assert d.stride(0) == ld_dout
    L.check(L.lib().tspm_pattern_expand_bwd(B, P, keep, *widths, d.data_ptr(), ld_dout, demb.ptr(), ld_demb, mods,
                                            L.stream_handle()), "pattern_expand_bwd")
    torch.cuda.synchronize()
    return demb


def _bits(t):
    return t.contiguous().view(torch.int32)


SUBSET = ("tv", "atv", "v")  # non-canonical order; no pattern drops video, so its zero rows are an unused slot
CASES = [(B, pats, widths, pad_out, pad_emb)
         for B in (1, 5)
         for pats in (tuple(PATTERNS), ("atv",), SUBSET)
         for widths, pad_out, pad_emb in (((8, 12, 8), 0, 0), ((8, 12, 7), 2, 4), ((4, 4, 5), 0, 2))]


@pytest.mark.parametrize("B,pats,widths,pad_out,pad_emb", CASES,
                         ids=[f"B{c[0]}-P{len(c[1])}-w{'.'.join(map(str, c[2]))}-ld+{c[3]}+{c[4]}" for c in CASES])
def test_expand_bwd_is_the_host_sum_bitwise(gpu, B, pats, widths, pad_out, pad_emb):
    E = sum(widths)
    ld_dout, ld_demb = E + pad_out, E + pad_emb  # (8,12,8): 28, 28 -> float4; 27+2 = 29 / 27+4 = 31, 13 / 15: odd -> scalar
    assert (ld_dout % 4 == 0 and ld_demb % 4 == 0) == (widths == (8, 12, 8))
    g = torch.Generator().manual_seed(B * 100 + len(pats) + E)
    full = torch.randn(len(pats) * B, ld_dout, generator=g)
    full[0, 0] = -0.0  # a negative zero in a kept slot: +0.0 + -0.0 = +0.0 on both sides
    want, used = _restate(full[:, :E], B, pats, widths)
    runs = []
    for _ in range(2):
        out = _run(gpu, B, pats, widths, ld_dout, ld_demb, full)
        out.intact("demb")
        runs.append(out.cpu())
    assert not bool(torch.isnan(want).any())
    assert torch.equal(_bits(runs[0]), _bits(want)) and torch.equal(_bits(runs[0]), _bits(runs[1]))
    c = _cols(widths)
    for m in range(3):  # a slot no pattern uses is +0.0 exactly (bit pattern 0)
        for r in range(2 * B):
            if not used[r, m]:
                assert bool((_bits(runs[0][r, c[m]:c[m + 1]]) == 0).all()), (r, m)
    if pats == ("atv",):
        assert not bool(used[B:].any()) and bool((_bits(runs[0][B:]) == 0).all())  # the zero rows are all +0.0
        assert torch.equal(_bits(runs[0][:B]), _bits(full[:, :E] + 0.0))
    if pats == SUBSET:
        assert not bool(used[B:, 1].any()) and bool(used[B:, 0].all()) and bool(used[B:, 2].all())


@pytest.mark.parametrize("widths,pad", [((8, 12, 8), 0), ((8, 12, 7), 2)])
def test_a_clear_modality_bit_leaves_its_columns_alone(gpu, widths, pad):
    """modalities = 0b101: the video columns of every row keep their guard pattern, audio and text are the host sums."""
    B, pats, E = 5, tuple(PATTERNS), sum(widths)
    ld = E + pad
    g = torch.Generator().manual_seed(9)
    full = torch.randn(len(pats) * B, ld, generator=g)
    want, _ = _restate(full[:, :E], B, pats, widths, mods=0b101)
    out = _run(gpu, B, pats, widths, ld, ld, full, mods=0b101)
    out.intact("demb")
    got, c = out.cpu(), _cols(widths)
    sentinel = _bits(Guarded(gpu, 1, 1).cpu())[0, 0]
    assert bool((_bits(got[:, c[1]:c[2]]) == sentinel).all()), "the video columns were written"
    for m in (0, 2):
        assert torch.equal(_bits(got[:, c[m]:c[m + 1]]), _bits(want[:, c[m]:c[m + 1]]))
    for mods in (0b010, 0b110):  # and the other way round
        out = _run(gpu, B, pats, widths, ld, ld, full, mods=mods)
        got = out.cpu()
        assert bool((_bits(got[:, c[0]:c[1]]) == sentinel).all())
        assert bool((_bits(got[:, c[2]:c[3]]) == sentinel).all()) == (mods == 0b010)


def test_more_than_one_block_and_the_grid_stride(gpu):
    """2 x 800 rows x 48 float4 units = 76,800 units: 300 blocks; 2 x 3000 x 198 one-float units = 1,188,000, past the
    4096-block cap (1,048,576 units per sweep), so the grid-stride loop runs a second sweep.  Every element lands."""
    for B, widths in ((800, (64, 64, 64)), (3000, (65, 66, 67))):
        E = sum(widths)
        g = torch.Generator().manual_seed(E)
        full = torch.randn(7 * B, E, generator=g)
        want, _ = _restate(full, B, tuple(PATTERNS), widths)
        out = _run(gpu, B, tuple(PATTERNS), widths, E, E, full)
        out.intact("demb")
        assert torch.equal(_bits(out.cpu()), _bits(want))


def test_adjoint_of_pattern_expand(gpu):
    """<expand(x), y> == <x, expand_bwd(y)> for random x [2B, E], y [P*B, E]: both sides in fp64 on the host from the
    device results.  expand is a copy (exact); expand_bwd adds at most P = 7 fp32 terms per element, so each element is
    within (P - 1) roundings of the exact sum: |lhs - rhs| <= (P - 1) * 2^-24 * sum |x| * (sum_p |y|)."""
    B, pats, widths = 5, tuple(PATTERNS), (8, 12, 7)
    P, E = len(pats), sum(widths)
    g = torch.Generator().manual_seed(31)
    x, y = torch.randn(2 * B, E, generator=g), torch.randn(P * B, E, generator=g)
    keep = (ctypes.c_int32 * (3 * P))(*[int(ch in name) for name in pats for ch in LETTERS])
    gid = (ctypes.c_int32 * P)(*range(P))
    out = Guarded(gpu, P * B, E)
    lab, lab_out = torch.zeros(B, dtype=torch.int64, device=gpu), torch.zeros(P * B, dtype=torch.int64, device=gpu)
    grp = torch.zeros(P * B, dtype=torch.int32, device=gpu)
    x_d = x.to(gpu)
    L.check(L.lib().tspm_pattern_expand(B, P, keep, gid, *widths, x_d.data_ptr(), E, out.ptr(), E, lab.data_ptr(),
                                        lab_out.data_ptr(), 8, grp.data_ptr(), L.stream_handle()), "pattern_expand")
    bwd = _run(gpu, B, pats, widths, E, E, y)
    lhs = (out.cpu().double() * y.double()).sum().item()
    rhs = (x.double() * bwd.cpu().double()).sum().item()
    abs_sum, _ = _restate(y.abs(), B, pats, widths)
    bound = (P - 1) * 2.0 ** -24 * (x.abs().double() * abs_sum.double()).sum().item()
    print(f"adjoint: lhs {lhs:.12e} rhs {rhs:.12e} diff {abs(lhs - rhs):.3e} bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound
