"""Op-level tests of the multi-group optimizer entry points (added under ABI 23): tspm_adam_begin_multi,
tspm_adam_step_multi and tspm_grad_clip_coef_multi, through ctypes on NaN-sentinel guarded buffers.

* tspm_adam_step_multi is held BITWISE to tspm_adam_step / tspm_adam_step_clip run on each segment alone (Adam is
  element-wise, so the partition of the work cannot show), and each segment to parity.adam_fp64 within
  parity.adam_tolerance at its own hyper-parameters.  Segment sizes: vector tails of 1, 2 and 3 elements, an empty
  segment, a segment smaller than one f32x4, and a segment longer than one workgroup's stride; and three segments of
  4.2 M elements together, past the 2048 workgroups of one launch, where the host scales the partition down.
* tspm_grad_clip_coef_multi with one range is BITWISE tspm_grad_clip_coef; with several ranges the squares are summed
  in another order, but in double, so the bound of test_gpu_seq_ops.test_grad_clip_coef_vs_fp64 carries over unchanged:
  the total within one float32 neighbour of sqrt(fp64 sum), the coefficient in the candidate set that follows from it.
"""
import ctypes

import numpy as np
import pytest
import torch

from parity import Guarded, adam_fp64, adam_tolerance
from test_gpu_seq_ops import _clip, _neighbours, _sync
from tspm_amd import _lib as L

pytestmark = pytest.mark.gpu

SEG_COUNTS = [1, 3, 4, 5, 0, 1027, 2, 256 * 4 + 1]


def _hyper(i):
    """Segment i's own (lr, beta1, beta2, eps, weight_decay, step)."""
    return (1e-3 / (i + 1), 0.9 - 0.02 * i, 0.999 - 0.003 * i, 1e-8 * (i + 1), 1e-3 * (i % 3), 1 + 2 * i)


def _hyper_tensor(i, gpu, step=None):
    lr, b1, b2, eps, wd, st = _hyper(i)
    h = torch.tensor([lr, b1, b2, eps, wd, 1.0, 0.0, 0.0], dtype=torch.float64)
    h.view(torch.int64)[6] = st if step is None else step
    return h.to(gpu)


def _data(counts, seed):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for n in counts:
        out.append(dict(p=torch.randn(n, generator=gen), g=torch.randn(n, generator=gen) * 3,
                        m=torch.randn(n, generator=gen) * 0.1, v=torch.rand(n, generator=gen) * 0.01))
    return out


def _buffers(gpu, d):
    n = d["p"].numel()
    bufs = [Guarded(gpu, 1, n) for _ in range(3)]
    for b, k in zip(bufs, "pmv"):
        b.t.copy_(d[k].view(1, n))
    return bufs


def _run_multi(gpu, data, coef):
    segs = (L.AdamSeg * len(data))()
    keep = []
    for i, (sg, d) in enumerate(zip(segs, data)):
        n = d["p"].numel()
        bufs, gd, hd = _buffers(gpu, d), d["g"].to(gpu), _hyper_tensor(i, gpu)
        keep.append((bufs, gd, hd))
        if n:
            sg.param, sg.grad, sg.exp_avg, sg.exp_avg_sq = bufs[0].ptr(), gd.data_ptr(), bufs[1].ptr(), bufs[2].ptr()
        sg.count, sg.hyper = n, hd.data_ptr()
    cd = None if coef is None else coef.to(gpu)
    L.check(L.lib().tspm_adam_step_multi(len(data), segs, L.ptr(cd), L.stream_handle()), "adam_step_multi")
    _sync()
    for bufs, _, _ in keep:
        for b in bufs:
            b.intact("adam_step_multi")
    return [[b.cpu().view(-1) for b in bufs] for bufs, _, _ in keep]


def _run_single(gpu, data, coef):
    out = []
    cd = None if coef is None else coef.to(gpu)
    for i, d in enumerate(data):
        n = d["p"].numel()
        bufs, gd, hd = _buffers(gpu, d), d["g"].to(gpu), _hyper_tensor(i, gpu)
        if n:
            args = (n, bufs[0].ptr(), gd.data_ptr(), bufs[1].ptr(), bufs[2].ptr(), hd.data_ptr())
            if cd is not None:
                L.check(L.lib().tspm_adam_step_clip(*args, cd.data_ptr(), L.stream_handle()), "adam_step_clip")
            else:
                L.check(L.lib().tspm_adam_step(*args, L.stream_handle()), "adam_step")
        _sync()
        out.append([b.cpu().view(-1) for b in bufs])
    return out


# segments that together ask for more workgroups than one launch takes (cdiv(count/4 + 1, 256): 2930 + 1 + 1172 > 2048),
# the size at which the host scales the partition down in proportion — a fault there can show at no smaller size
SCALED_COUNTS = [3_000_001, 5, 1_200_003]


@pytest.mark.parametrize("counts", [SEG_COUNTS, [1027], SCALED_COUNTS], ids=["eight", "one", "scaled"])
@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip"])
def test_adam_step_multi_is_adam_step_per_segment(gpu, counts, clip):
    data = _data(counts, seed=len(counts))
    coef = torch.tensor([0.37], dtype=torch.float32) if clip else None
    multi, single = _run_multi(gpu, data, coef), _run_single(gpu, data, coef)
    worst = 0.0
    for i, (d, got, ref) in enumerate(zip(data, multi, single)):
        for a, b, nm in zip(got, ref, ("param", "exp_avg", "exp_avg_sq")):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (i, counts[i], nm)
        if not counts[i]:
            continue
        lr, b1, b2, eps, wd, st = _hyper(i)
        gc = d["g"].double() * (float(coef) if clip else 1.0)
        exp, m, v = adam_fp64(d["p"], gc, st, lr=lr, wd=wd, b1=b1, b2=b2, eps=eps, m=d["m"], v=d["v"])
        tol = 1e-6 * exp.abs() + adam_tolerance(d["p"].double(), gc, st, v, lr, wd, b1=b1, b2=b2, eps=eps)
        err = (got[0].double() - exp).abs()
        worst = max(worst, (err / tol).max().item())
        assert bool((err <= tol).all()), (i, counts[i], (err / tol).max().item())
    print(f"adam_step_multi[{len(counts)} segments, clip {clip}]: worst |err| / tolerance {worst:.3f}")
    again = _run_multi(gpu, data, coef)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for x, y in zip(multi, again) for a, b in zip(x, y))


def test_adam_begin_multi_advances_every_step_and_nothing_else(gpu):
    n = len(SEG_COUNTS)
    segs = (L.AdamSeg * n)()
    hypers = [Guarded(gpu, 1, 16) for _ in range(n)]  # 8 doubles as 16 float32 words
    before = []
    dummy = torch.zeros(2048, device=gpu)
    for i, (sg, h) in enumerate(zip(segs, hypers)):
        h.t.view(-1).view(torch.float64).copy_(_hyper_tensor(i, gpu))
        before.append(h.cpu().view(-1).view(torch.int64).clone())
        if SEG_COUNTS[i]:
            sg.param = sg.grad = sg.exp_avg = sg.exp_avg_sq = dummy.data_ptr()
        sg.count, sg.hyper = SEG_COUNTS[i], h.ptr()
    for rep in (1, 2):
        L.check(L.lib().tspm_adam_begin_multi(n, segs, L.stream_handle()), "adam_begin_multi")
        _sync()
        for i, h in enumerate(hypers):
            h.intact("hyper")
            now = h.cpu().view(-1).view(torch.int64)
            want = before[i].clone()
            want[6] += rep
            assert torch.equal(now, want), (i, rep)
    assert not bool(dummy.any())  # no buffer of a segment is touched


def _clip_multi(gpu, gs_list, gs, max_norm, with_total=True, ws_bytes=None):
    gds = [g.to(gpu) for g in gs_list]
    ranges = (L.GradRange * len(gds))(*[L.GradRange(g.data_ptr() if g.numel() else None, g.numel()) for g in gds])
    need = L.lib().tspm_grad_clip_workspace()
    ws = Guarded(gpu, 1, need, dtype=torch.uint8)
    coef, total = Guarded(gpu, 1, 1), Guarded(gpu, 1, 1)
    st = L.lib().tspm_grad_clip_coef_multi(len(gds), ranges, gs, max_norm, coef.ptr(), total.ptr() if with_total else None,
                                           ws.ptr(), need if ws_bytes is None else ws_bytes, L.stream_handle())
    _sync()
    ws.intact("clip workspace"); coef.intact("clip coef"); total.intact("clip total")
    return st, coef.cpu().reshape(()), total.flat[:1].cpu().reshape(())


def _bits(t):
    return t.reshape(1).view(torch.int32).item()


@pytest.mark.parametrize("count", [1, 257, 512 * 256 + 1])
def test_grad_clip_coef_multi_one_range_is_the_single_call(gpu, count):
    g = torch.randn(count, generator=torch.Generator().manual_seed(count)) * 2
    for gs in (1.0, float(torch.tensor(1.0 / 3.0, dtype=torch.float32))):
        for max_norm in (1.0, 0.5):
            st1, c1, t1 = _clip(gpu, g, gs, max_norm)
            st2, c2, t2 = _clip_multi(gpu, [g], gs, max_norm)
            assert st1 == st2 == 0
            assert _bits(c1) == _bits(c2) and _bits(t1) == _bits(t2), (count, gs, max_norm, c1.item(), c2.item())


RANGES = [3, 512 * 256 + 1, 1, 1027]


def test_grad_clip_coef_multi_vs_fp64(gpu):
    """The data and the bound of test_gpu_seq_ops.test_grad_clip_coef_vs_fp64 over four ranges."""
    gen = torch.Generator().manual_seed(7)
    n = sum(RANGES)
    wide = 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 38 - 20)   # 1e-20 .. 1e18
    wide = (wide * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1)).float()
    values = {"randn": torch.randn(n, generator=gen), "wide": wide, "zeros": torch.zeros(n)}
    for name, g in values.items():
        parts = list(torch.split(g, RANGES))
        for gs in (1.0, 1.0 / 3.0):
            gs32 = torch.tensor(gs, dtype=torch.float32)
            ref = np.float32(np.sqrt((g * gs32).double().pow(2).sum().item()))
            for max_norm in (1.0, 0.5):
                st, coef, total = _clip_multi(gpu, parts, float(gs32), max_norm)
                assert st == 0
                _, coef2, total2 = _clip_multi(gpu, parts, float(gs32), max_norm)
                assert _bits(coef) == _bits(coef2) and _bits(total) == _bits(total2), "not deterministic"
                cands = {float(min(np.float32(1.0), np.float32(max_norm) / (np.float32(t) + np.float32(1e-6))))
                         for t in _neighbours(ref)}
                print(f"grad_clip_coef_multi[{name} gs {gs:.3f} max {max_norm}]: total {total.item():.9e} reference "
                      f"{float(ref):.9e} coef {coef.item():.9e}")
                assert total.item() in _neighbours(ref), (name, gs, total.item(), float(ref))
                assert coef.item() in cands, (name, gs, max_norm, coef.item(), cands)
                if name == "zeros":
                    assert coef.item() == 1.0 and total.item() == 0.0
    # an empty range between the others changes nothing; total_norm is optional
    parts = list(torch.split(values["randn"], RANGES))
    _, c0, t0 = _clip_multi(gpu, parts, 1.0, 1.0)
    _, c1, t1 = _clip_multi(gpu, parts[:2] + [torch.zeros(0)] + parts[2:], 1.0, 1.0)
    assert _bits(c0) == _bits(c1) and _bits(t0) == _bits(t1)  # the partition follows the non-empty counts alone
    st, c2, t2 = _clip_multi(gpu, parts, 1.0, 1.0, with_total=False)
    assert st == 0 and _bits(c2) == _bits(c0) and t2.isnan()


def test_grad_clip_coef_multi_non_finite_follows_clip_grad_norm(gpu):
    """A NaN in one range: NaN total and coefficient; an inf: an inf total and a coefficient of 0 (torch.clamp(max=1))."""
    base = [torch.arange(1, n + 1, dtype=torch.float32) / n for n in RANGES]
    for r, at in ((0, 1), (1, 512 * 256), (3, 1026)):
        for bad in (float("nan"), float("inf"), float("-inf")):
            parts = [b.clone() for b in base]
            parts[r][at] = bad
            st, coef, total = _clip_multi(gpu, parts, 1.0, 1.0)
            assert st == 0
            if bad != bad:
                assert total.isnan() and coef.isnan(), (r, coef.item(), total.item())
            else:
                assert total.item() == float("inf") and coef.item() == 0.0, (r, bad, coef.item(), total.item())


def test_grad_clip_coef_multi_short_workspace_status(gpu):
    need = L.lib().tspm_grad_clip_workspace()
    st, coef, _ = _clip_multi(gpu, [torch.ones(8), torch.ones(5)], 1.0, 1.0, ws_bytes=need - 1)
    assert st == 3 and coef.isnan()  # TSPM_ERR_WORKSPACE, nothing launched
