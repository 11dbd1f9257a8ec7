"""``tspm_pattern_expand`` on the device, through ctypes into guarded outputs, against a host restatement: a pure copy, so
the comparison is bitwise.  Widths (8, 12, 5) with row strides wider than their sum run the 16-byte path (audio, video)
and the one-float path (text, 5 wide) in one launch; with an odd input stride every segment takes the one-float path;
(64, 64, 64) is the YAMLs' layout, all 16-byte."""
import ctypes

import pytest
import torch

from parity import Guarded
from tspm_amd import _lib as L
from tspm_amd.mosi_data import PATTERNS

pytestmark = pytest.mark.gpu
LETTERS = "avt"  # the column order of the embeddings: cat(audio, video, text)


def _restate(emb, B, patterns, widths, labels, group_of):
    """out [P*B, sum(widths)], labels [P*B], groups [P*B] on the host."""
    cols = [0, widths[0], widths[0] + widths[1], sum(widths)]
    out = torch.empty(len(patterns) * B, sum(widths), dtype=emb.dtype)
    for p, name in enumerate(patterns):
        for m, ch in enumerate(LETTERS):
            src = emb[:B] if ch in name else emb[B:2 * B]
            out[p * B:(p + 1) * B, cols[m]:cols[m + 1]] = src[:, cols[m]:cols[m + 1]]
    groups = torch.tensor([group_of[name] for name in patterns for _ in range(B)], dtype=torch.int32)
    return out, labels.repeat(len(patterns)), groups


def _run(gpu, B, patterns, widths, ld_emb, ld_out, labels, group_of, emb):
    P, E = len(patterns), sum(widths)
    out = Guarded(gpu, P * B, E, ld_out)
    lab = Guarded(gpu, P * B, 1, dtype=labels.dtype if labels.dtype == torch.int64 else torch.float32)
    grp = torch.full((P * B + 64,), -77, dtype=torch.int32, device=gpu)
    keep = (ctypes.c_int32 * (3 * P))(*[int(ch in name) for name in patterns for ch in LETTERS])
    gid = (ctypes.c_int32 * P)(*[group_of[name] for name in patterns])
    emb_d, lab_d = emb.to(gpu), labels.to(gpu)
    assert emb_d.stride(0) == ld_emb
    L.check(L.lib().tspm_pattern_expand(B, P, keep, gid, *widths, emb_d.data_ptr(), ld_emb, out.ptr(), ld_out,
                                        lab_d.data_ptr(), lab.ptr(), labels.element_size(), grp.data_ptr(),
                                        L.stream_handle()), "pattern_expand")
    torch.cuda.synchronize()
    out.intact("out")
    lab.intact("labels_out")
    assert bool((grp[P * B:] == -77).all()), "groups_out: wrote past its last element"
    return out.cpu(), lab.cpu().reshape(-1), grp[:P * B].cpu()


CASES = [(B, pats, widths, pad_in, pad_out, ldt)
         for B in (1, 5)
         for pats in (tuple(PATTERNS), ("v", "at"))
         for widths, pad_in, pad_out in (((8, 12, 5), 7, 3), ((8, 12, 5), 4, 0), ((8, 12, 5), 0, 7), ((64, 64, 64), 0, 0))
         for ldt in (torch.int64, torch.float32)]


@pytest.mark.parametrize("B,pats,widths,pad_in,pad_out,ldt", CASES,
                         ids=[f"B{c[0]}-P{len(c[1])}-w{c[2][0]}.{c[2][2]}-ld+{c[3]}+{c[4]}-{str(c[5])[6:]}" for c in CASES])
def test_expand_is_the_host_copy_bitwise(gpu, B, pats, widths, pad_in, pad_out, ldt):
    E = sum(widths)
    ld_emb, ld_out = E + pad_in, E + pad_out  # 25 + (7, 3) = (32, 28): both multiples of 4 -> 16-byte audio / video
    g = torch.Generator().manual_seed(B * 100 + len(pats) + E)
    full = torch.randn(2 * B, ld_emb, generator=g)
    emb = full[:, :E]  # a strided view: the padding columns of the input exist and are never read into out
    if ldt == torch.int64:
        labels = torch.randint(0, 3, (B,), generator=g) + (1 << 40)  # the high word travels too
    else:
        labels = (torch.randint(-15, 16, (B,), generator=g).double() / 5).float()
    group_of = {name: 6 - i for i, name in enumerate(PATTERNS)}  # ids the patterns' order does not give away
    want = _restate(emb, B, pats, widths, labels, group_of)
    runs = [_run(gpu, B, pats, widths, ld_emb, ld_out, labels, group_of, full) for _ in range(2)]
    for got in runs:
        for name, a, b in zip(("out", "labels_out", "groups_out"), got, want):
            assert a.dtype == b.dtype and torch.equal(a, b), name
    for a, b in zip(*runs):
        assert torch.equal(a, b)  # two runs: bitwise


def test_more_than_one_block_and_the_grid_stride(gpu):
    """The grid is capped at 4096 blocks of 256 threads (1,048,576 units per sweep).  7 patterns x 800 rows x 48 float4
    units = 268,800: about a thousand blocks, one sweep; with (65, 66, 67) on the one-float path 7 x 800 x 198 =
    1,108,800 units: past the cap, so the grid-stride loop runs a second sweep.  Every element still lands."""
    group_of = {name: i for i, name in enumerate(PATTERNS)}
    for B, widths in ((800, (64, 64, 64)), (800, (65, 66, 67))):
        E = sum(widths)
        g = torch.Generator().manual_seed(E)
        full = torch.randn(2 * B, E, generator=g)
        labels = torch.randint(0, 3, (B,), generator=g)
        want = _restate(full, B, tuple(PATTERNS), widths, labels, group_of)
        got = _run(gpu, B, tuple(PATTERNS), widths, E, E, labels, group_of, full)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
