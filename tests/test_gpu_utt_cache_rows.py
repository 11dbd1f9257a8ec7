"""tspm_utt_cache_rows (the UTT-Fusion encoder half read from a cache) at op level: bitwise against torch indexing.

The kernel only moves floats and multiplies the pooled ones by the dropout factor, so every check is ``torch.equal``:
``pool_out`` against ``v * torch.where(keep, scale, 0)`` bit for bit (``torch.where(keep, v * scale, 0)`` but for the
sign of the zero a dropped negative value leaves), the audio / video columns and the labels against plain
indexing, a captured replay against the eager call, sentinel padding columns untouched, and an out-of-range index giving
a NaN row and label -1 with its neighbours intact.  Each refusal of the header returns TSPM_ERR_INVALID."""
import ctypes

import pytest
import torch

from tspm_amd import _lib as L

pytestmark = pytest.mark.gpu
ERR_INVALID = 1
SENTINEL = -777.0


def _case(gpu, B, N, widths, halves, n_zero, *, keep=True, scale=1.0, float_labels=False, row_keep=None, pad=(0, 0, 0),
          rows=None, seed=0):
    """The launch's tensors and its descriptor; ``pad`` = extra columns of (ld_cache, ld_av, ld_pool)."""
    g = torch.Generator().manual_seed(seed)
    wa, wv, wp = widths
    W, R = wa + wv + wp, halves * B
    t = dict(emb=torch.randn(N, W + pad[0], generator=g), zero=torch.randn(n_zero, W + pad[0], generator=g),
             rows=torch.randint(0, N, (B,), generator=g) if rows is None else torch.tensor(rows, dtype=torch.int64),
             labels_all=(torch.randn(N, generator=g) if float_labels else torch.randint(0, 3, (N,), generator=g)),
             keep=(torch.rand(R, wp, generator=g) < 0.5).to(torch.uint8) if keep else None,
             row_keep=None if row_keep is None else torch.tensor(row_keep, dtype=torch.uint8),
             av_out=torch.full((R, wa + wv + pad[1]), SENTINEL), pool_out=torch.full((R, wp + pad[2]), SENTINEL))
    t["labels_out"] = torch.full((B,), 7, dtype=t["labels_all"].dtype)
    t = {k: (v.to(gpu) if v is not None else None) for k, v in t.items()}
    d = L.UttCacheRowsDesc(batch=B, halves=halves, w_audio=wa, w_video=wv, w_pool=wp, ld_cache=W + pad[0],
                           ld_av=wa + wv + pad[1], ld_pool=wp + pad[2], n_rows=N, n_zero=n_zero,
                           label_bytes=4 if float_labels else 8, scale=scale)
    for k in ("emb", "zero", "rows", "row_keep", "labels_all", "labels_out", "keep", "av_out", "pool_out"):
        setattr(d, k, L.ptr(t[k]))
    return t, d


def _launch(d):
    return L.lib().tspm_utt_cache_rows(ctypes.byref(d), L.stream_handle())


def _want(t, B, N, widths, halves, n_zero, scale):
    """(av, pool, labels) by torch indexing; an out-of-range index: NaN row, label -1 (NaN for float labels)."""
    wa, wv, wp = widths
    hav, R = wa + wv, halves * B
    rows = t["rows"].repeat(halves)
    ok = (rows >= 0) & (rows < N)
    safe = rows.clamp(0, N - 1)
    real = torch.zeros(R, 3, dtype=torch.bool, device=rows.device)
    real[:B] = True if t["row_keep"] is None else t["row_keep"] != 0
    zrow = t["zero"][torch.zeros_like(safe) if n_zero == 1 else safe]
    src = t["emb"][safe]
    col_mod = torch.tensor([0] * wa + [1] * wv + [2] * wp, device=rows.device)
    v = torch.where(real[:, col_mod], src[:, :hav + wp], zrow[:, :hav + wp])
    v = torch.where(ok[:, None], v, torch.full_like(v, float("nan")))
    pool = v[:, hav:]
    if t["keep"] is not None:
        # the kernel's own expression, v * (keep ? scale : 0): torch.where(keep, v * scale, 0) up to the sign of a
        # dropped negative value's zero (and NaN * 0 stays NaN), so the comparison below can be on the bits
        pool = pool * torch.where(t["keep"] != 0, torch.full_like(pool, scale), torch.zeros_like(pool))
    lab = t["labels_all"][safe[:B]]
    bad = float("nan") if lab.is_floating_point() else -1
    lab = torch.where(ok[:B], lab, torch.full_like(lab, bad))
    return v[:, :hav], pool, lab


def _same(a, b):
    """NaN in the same places, every other element equal as a bit pattern (the sign of a zero included)."""
    if a.shape != b.shape or a.dtype != b.dtype or not torch.equal(torch.isnan(a), torch.isnan(b)):
        return False
    a, b = (torch.where(torch.isnan(x), torch.zeros_like(x), x).contiguous() for x in (a, b))
    return torch.equal(a.view(torch.int64 if a.dtype == torch.float64 else torch.int32),
                       b.view(torch.int64 if b.dtype == torch.float64 else torch.int32))


def _check(t, B, N, widths, halves, n_zero, scale, pad=(0, 0, 0)):
    wa, wv, wp = widths
    av, pool, lab = _want(t, B, N, widths, halves, n_zero, scale)
    assert _same(t["av_out"][:, :wa + wv], av)
    assert _same(t["pool_out"][:, :wp], pool)
    assert _same(t["labels_out"].double(), lab.double())
    if pad[1]:
        assert bool((t["av_out"][:, wa + wv:] == SENTINEL).all())
    if pad[2]:
        assert bool((t["pool_out"][:, wp:] == SENTINEL).all())


def test_all_pattern_layout_with_dropout_and_per_sample_zero_rows(gpu):
    """Case 1: B=5, N=11, widths (8, 12, 384), halves 2, n_zero N, keep with scale 2, int64 labels; a repeat, index 0
    and index N-1 among the rows; larger leading dimensions with sentinel padding."""
    B, N, widths, pad = 5, 11, (8, 12, 384), (4, 8, 4)
    t, d = _case(gpu, B, N, widths, 2, N, scale=2.0, rows=[3, 0, N - 1, 3, 7], pad=pad)
    assert _launch(d) == 0
    torch.cuda.synchronize()
    _check(t, B, N, widths, 2, N, 2.0, pad)
    assert torch.equal(t["av_out"][B:, :20], t["zero"][t["rows"], :20])  # the zero rows of the same samples
    eager = {k: t[k].clone() for k in ("av_out", "pool_out", "labels_out")}
    for k in ("av_out", "pool_out"):
        t[k].fill_(SENTINEL)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with L.graph_capture(g):
        assert _launch(d) == 0
    g.replay()
    torch.cuda.synchronize()
    for k, v in eager.items():
        assert _same(t[k], v), k


def test_per_row_patterns_single_zero_row_and_float_labels(gpu):
    """Case 2: B=7, N=9, widths (4, 4, 12), halves 1, n_zero 1, a mixed row_keep with a row that keeps nothing."""
    B, N, widths = 7, 9, (4, 4, 12)
    rk = [[1, 1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 0], [1, 1, 0], [0, 1, 1]]
    t, d = _case(gpu, B, N, widths, 1, 1, scale=1.0 / 0.3, float_labels=True, row_keep=rk, seed=1)
    assert _launch(d) == 0
    torch.cuda.synchronize()
    _check(t, B, N, widths, 1, 1, d.scale)
    assert torch.equal(t["av_out"][4], t["zero"][0, :8]) and t["labels_out"].dtype == torch.float32


@pytest.mark.parametrize("halves", [1, 2])
def test_one_row_without_a_mask(gpu, halves):
    """Case 3: B = N = 1, keep NULL: the pooled values pass unscaled whatever ``scale`` says."""
    t, d = _case(gpu, 1, 1, (4, 8, 12), halves, 1, keep=False, scale=5.0, seed=2)
    assert _launch(d) == 0
    torch.cuda.synchronize()
    _check(t, 1, 1, (4, 8, 12), halves, 1, 5.0)
    assert torch.equal(t["pool_out"][0], t["emb"][0, 12:])


@pytest.mark.parametrize("float_labels", [False, True])
def test_out_of_range_index_gives_a_nan_row(gpu, float_labels):
    B, N, widths = 4, 6, (4, 4, 12)
    for bad in (N, -1):
        t, d = _case(gpu, B, N, widths, 2, N, scale=2.0, rows=[1, bad, 5, 0], float_labels=float_labels, seed=3)
        assert _launch(d) == 0
        torch.cuda.synchronize()
        _check(t, B, N, widths, 2, N, 2.0)
        for r in (1, B + 1):
            assert bool(torch.isnan(t["av_out"][r]).all()) and bool(torch.isnan(t["pool_out"][r]).all())
        ok = [r for r in range(2 * B) if r % B != 1]
        assert not bool(torch.isnan(t["av_out"][ok]).any()) and not bool(torch.isnan(t["pool_out"][ok]).any())
        lab = t["labels_out"]
        assert bool(torch.isnan(lab[1])) if float_labels else int(lab[1]) == -1
        assert torch.equal(lab[[0, 2, 3]], t["labels_all"][[1, 5, 0]])


def test_refusals(gpu):
    B, N, widths = 4, 6, (4, 8, 12)

    def refused(**change):
        kw = dict(halves=1, n_zero=1)
        kw.update({k: change.pop(k) for k in list(change) if k in ("halves", "n_zero", "row_keep")})
        t, d = _case(gpu, B, N, widths, kw["halves"], kw["n_zero"], row_keep=kw.get("row_keep"))
        for k, v in change.items():
            setattr(d, k, v(d, t) if callable(v) else v)
        before = t["av_out"].clone()
        rc = _launch(d)
        torch.cuda.synchronize()
        assert rc in (0, ERR_INVALID) and (rc == 0 or torch.equal(t["av_out"], before)), "a refusal launched something"
        return rc == ERR_INVALID

    assert not refused()
    for name in ("emb", "zero", "rows", "av_out", "pool_out"):
        assert refused(**{name: None}), name
    for name in ("w_audio", "w_video", "w_pool", "ld_cache", "ld_av", "ld_pool"):
        assert refused(**{name: 0}), name
        assert refused(**{name: lambda d, t, n=name: getattr(d, n) + 2}), name  # not a multiple of 4
    assert refused(ld_cache=20) and refused(ld_av=8) and refused(ld_pool=8)  # below the widths
    for name in ("emb", "zero", "av_out", "pool_out", "keep"):
        assert refused(**{name: lambda d, t, n=name: t[n].data_ptr() + 4}), name  # not 16-byte aligned
    assert refused(batch=0) and refused(n_rows=0)
    t, d = _case(gpu, B, N, widths, 1, 1)
    for h in (0, 3):
        d.halves = h
        assert _launch(d) == ERR_INVALID
    assert refused(halves=2, row_keep=[[1, 1, 1]] * B)
    t, d = _case(gpu, B, N, widths, 1, 1)
    d.n_zero = 2
    assert _launch(d) == ERR_INVALID
    assert refused(label_bytes=2) and refused(labels_all=None) and refused(labels_out=None)
    assert not refused(labels_all=None, labels_out=None)  # neither: no labels travel
    assert L.lib().tspm_utt_cache_rows(None, L.stream_handle()) == ERR_INVALID
