"""tspm_embed_gather and tspm_cached_head_train_step alone: the head stage reading its samples from a cache of embeddings
by index.  The cache has 300 rows; every index vector holds a repeat, row 0 and row 299.  Every-pattern mode is held
BITWISE to tspm_pattern_head_train_step on the explicitly gathered rows (test_gpu_pattern_head_train.run, same shapes and
pattern sets); per-sample mode bitwise to the every-pattern mode when every row carries the same flags, and with mixed
flags to the fp64 chain of tests/head_stage_ref.py on rows built with torch.where (parity.op_check, the fp32 CPU run as
yardstick, gradients with grad=True); the folded bookkeeping integer- and bit-equal to tspm_classify_update on the call's
own logits."""
import ctypes

import pytest
import torch

import head_stage_ref as R
import parity
import test_gpu_pattern_head_train as T
from tspm_amd import _lib as L

pytestmark = pytest.mark.gpu

SHAPES, PATSETS, GRADS, LOSS_WEIGHT, bits = T.SHAPES, T.PATSETS, T.GRADS, T.LOSS_WEIGHT, T.bits
N_ROWS = 300
INVALID, WORKSPACE = 1, 3
_CACHE = {}


def cache_case(shape):
    """The cache (emb [300, F], labels_all [300]), the index vector [B] and, from test_gpu_pattern_head_train.case, x0
    and the head's weights for a shape (fp32 / int64, CPU), built once per shape and never modified."""
    if shape not in _CACHE:
        B, F, wa, H, H2, C = shape
        g = torch.Generator().manual_seed(500 + B + F)
        emb = torch.randn(N_ROWS, F, generator=g)
        labels_all = torch.randint(0, C, (N_ROWS,), generator=g)
        idx = torch.randint(0, N_ROWS, (B,), generator=g)
        idx[0] = N_ROWS - 1
        if B > 1:
            idx[-1] = 0
        if B > 3:
            idx[2] = idx[1]
        _, x0, _, W = T.case(shape)
        _CACHE[shape] = (emb, labels_all, idx, x0, W)
    return _CACHE[shape]


def untouched(gd) -> bool:
    return bool((gd.flat.view(parity._BITS[gd.flat.dtype]) == parity._SENTINEL[gd.flat.dtype]).all())


def run_cached(dev, shape, pats, emb_t, labels_t, idx, x0_t, W, p=0.0, mask=None, gen_keep=0, seed=0, counter=None,
               adam_step=None, stats0=(0.0, 0.0, 0.0), lde=None, rk=None, rg=None, gids=None, log=None, expect=0,
               **over):
    """One tspm_cached_head_train_step call with every output in a parity.Guarded buffer.  ``pats`` = pattern names
    (every-pattern mode) or None with ``rk`` [B, 2] / ``rg`` [B], the rows' keep flags and groups (per-sample mode).  ``log`` = (conf,
    loss_log, counters, capacity, n_groups) device tensors.  ``over`` overrides descriptor fields; with ``expect`` != 0
    the status is asserted, nothing may have been written, and None is returned."""
    B, F, wa, H, H2, C = shape
    P = 1 if pats is None else len(pats)
    n = P * B
    ld_emb = lde or F
    d = {k: v.to(dev).contiguous() for k, v in W.items()}
    eg = torch.full((emb_t.shape[0], ld_emb), 7.0, device=dev)
    eg[:, :F] = emb_t.to(dev)
    x0d, lab, rows = x0_t.to(dev).contiguous(), labels_t.to(dev), idx.to(dev)
    out = {"logits": parity.Guarded(dev, n, C), "loss": parity.Guarded(dev, 1, 1), "gw0": parity.Guarded(dev, H, F),
           "gb0": parity.Guarded(dev, 1, H), "gw3": parity.Guarded(dev, H2, H), "gb3": parity.Guarded(dev, 1, H2),
           "gw5": parity.Guarded(dev, C, H2), "gb5": parity.Guarded(dev, 1, C),
           "mask": parity.Guarded(dev, n, H, dtype=torch.uint8)}
    if mask is not None:
        out["mask"].t.copy_(mask.to(dev))
    stats = torch.tensor(list(stats0) + [0.0], device=dev)
    need = int(L.lib().tspm_cached_head_train_workspace(B, P))
    assert need == int(L.lib().tspm_pattern_head_train_workspace(B, P))
    ws = parity.Guarded(dev, need, 1, dtype=torch.uint8)
    keep = gid = None
    if pats is not None:
        keep = (ctypes.c_int32 * (2 * P))(*[k for pt in pats for k in R.KEEP[pt]])
        gid = (ctypes.c_int32 * P)(*(gids if gids is not None else range(P)))
    rk = None if rk is None else rk.to(dev).to(torch.uint8).contiguous()
    rg = None if rg is None else rg.to(dev).to(torch.int32).contiguous()
    conf, loss_log, counters, cap, n_groups = log if log is not None else (None, None, None, 0, 1)
    f = dict(
        batch=B, npat=P, in_=F, w_audio=wa, hidden=H, hidden2=H2, classes=C, ld_emb=ld_emb, gen_keep=gen_keep,
        n_groups=n_groups, n_rows=emb_t.shape[0], emb=eg.data_ptr(), x0=x0d.data_ptr(), rows=rows.data_ptr(),
        labels_all=lab.data_ptr(), keep=keep, group_id=gid, row_keep=L.ptr(rk), row_group=L.ptr(rg),
        w0=d["w0"].data_ptr(), b0=d["b0"].data_ptr(), w3=d["w3"].data_ptr(), b3=d["b3"].data_ptr(),
        w5=d["w5"].data_ptr(), b5=d["b5"].data_ptr(), p=p, loss_weight=LOSS_WEIGHT, seed=seed,
        counter=None if counter is None else counter.data_ptr(), keep_mask=out["mask"].ptr() if p > 0 else None,
        logits=out["logits"].ptr(), **{g: out[g].ptr() for g in GRADS}, loss=out["loss"].ptr(), stats=stats.data_ptr(),
        adam_step=None if adam_step is None else adam_step.data_ptr(), confusion=L.ptr(conf), loss_log=L.ptr(loss_log),
        counters=L.ptr(counters), log_capacity=cap, workspace=ws.ptr(), workspace_bytes=need)
    f.update(over)
    status = L.lib().tspm_cached_head_train_step(L.CachedHeadTrainDesc(**f), L.stream_handle())
    torch.cuda.synchronize()
    if expect:
        assert status == expect, (status, over)
        for name, gd in out.items():
            if mask is None or name != "mask":
                assert untouched(gd), f"{name} written by a refused call {over}"
        assert untouched(ws) and stats.tolist() == list(stats0) + [0.0]
        return None
    L.check(status, "cached_head_train_step")
    for name, gd in out.items():
        if name == "mask" and p == 0:
            assert untouched(gd), "keep_mask touched without dropout"
            continue
        gd.intact(name)
    ws.intact("workspace")
    res = {k: v.cpu() for k, v in out.items()}
    for g in ("gb0", "gb3", "gb5", "loss"):
        res[g] = res[g].reshape(-1)
    res["stats"] = stats.cpu()
    return res


def same(a, b, keys=("logits", "loss", "stats") + GRADS):
    for k in keys:
        assert torch.equal(bits(a[k]), bits(b[k])), k


# ------------------------------------------------------------------------------------------------
# tspm_embed_gather
# ------------------------------------------------------------------------------------------------
def gather(dev, emb_t, labels_t, idx, F, lde=None, ldo=None, rk=None, wa=0, x0_t=None, expect=0, **over):
    B = idx.numel()
    ld_emb, ld_out = lde or F, ldo or F
    eg = torch.full((emb_t.shape[0], ld_emb), 7.0, device=dev)
    eg[:, :F] = emb_t.to(dev)
    out = parity.Guarded(dev, B, F, ld=ld_out)
    lab_out = parity.Guarded(dev, B, 1, dtype=torch.int64)
    rows, lab = idx.to(dev), labels_t.to(dev)
    rk = None if rk is None else rk.to(dev).to(torch.uint8).contiguous()
    x0d = None if x0_t is None else x0_t.to(dev).contiguous()
    a = dict(batch=B, in_=F, emb=eg.data_ptr(), n_rows=emb_t.shape[0], ld_emb=ld_emb, rows=rows.data_ptr(),
             labels_all=lab.data_ptr(), row_keep=L.ptr(rk), w_audio=wa, x0=L.ptr(x0d), out=out.ptr(), ld_out=ld_out,
             labels_out=lab_out.ptr())
    a.update(over)
    status = L.lib().tspm_embed_gather(*a.values(), L.stream_handle())
    torch.cuda.synchronize()
    if expect:
        assert status == expect, (status, over)
        assert untouched(out) and untouched(lab_out), over
        return None
    L.check(status, "embed_gather")
    out.intact("out")            # the tail and the padding columns (ld_out > in) keep their content
    lab_out.intact("labels_out")
    return out.cpu(), lab_out.cpu().reshape(-1)


@pytest.mark.parametrize("flags", [False, True], ids=["plain", "row_keep"])
@pytest.mark.parametrize("shape", SHAPES, ids=T._ids(SHAPES))
def test_embed_gather(gpu, shape, flags):
    B, F, wa = shape[:3]
    emb, labels_all, idx, x0, _ = cache_case(shape)
    rk = None
    want = emb[idx]
    if flags:
        rk = torch.tensor([(1, 0), (1, 1), (0, 1)], dtype=torch.uint8)[torch.arange(B) % 3]
        cols_a = torch.arange(F) < wa
        real = torch.where(cols_a.unsqueeze(0), rk[:, :1].bool(), rk[:, 1:].bool())
        want = torch.where(real, emb[idx], x0.unsqueeze(0).expand(B, F))
    for ld_emb, ld_out in ((F, F), (F + 8, F + 4)):
        got, lab = gather(gpu, emb, labels_all, idx, F, ld_emb, ld_out, rk, wa if flags else 0, x0 if flags else None)
        assert torch.equal(bits(got), bits(want))
        assert torch.equal(lab, labels_all[idx])


@pytest.mark.parametrize("bad", [N_ROWS, -1, 1 << 40])
def test_embed_gather_out_of_range_index(gpu, bad):
    shape = SHAPES[2]
    B, F, wa = shape[:3]
    emb, labels_all, idx, x0, _ = cache_case(shape)
    bad_idx = idx.clone()
    bad_idx[4] = bad
    rk = torch.tensor([(0, 1)] * B, dtype=torch.uint8)
    for flags in (None, rk):
        got, lab = gather(gpu, emb, labels_all, bad_idx, F, rk=flags, wa=wa, x0_t=x0)
        good, glab = gather(gpu, emb, labels_all, idx, F, rk=flags, wa=wa, x0_t=x0)
        ok = torch.arange(B) != 4
        assert torch.isnan(got[4]).all() and lab[4].item() == -1
        assert torch.equal(bits(got[ok]), bits(good[ok])) and torch.equal(lab[ok], glab[ok])


def test_embed_gather_refusals(gpu):
    shape = SHAPES[0]
    B, F, wa = shape[:3]
    emb, labels_all, idx, x0, _ = cache_case(shape)
    rk = torch.ones(B, 2, dtype=torch.uint8)
    for over in (dict(batch=0), dict(in_=0), dict(in_=F - 2), dict(n_rows=0), dict(ld_emb=F - 4), dict(ld_emb=F + 2),
                 dict(ld_out=F - 4), dict(ld_out=F + 2), dict(emb=None), dict(rows=None), dict(out=None),
                 dict(labels_out=None), dict(labels_all=None)):
        gather(gpu, emb, labels_all, idx, F, expect=INVALID, **over)
    for over in (dict(x0=None), dict(w_audio=0), dict(w_audio=F), dict(w_audio=wa + 2)):
        gather(gpu, emb, labels_all, idx, F, rk=rk, wa=wa, x0_t=x0, expect=INVALID, **over)
    gather(gpu, emb, labels_all, idx, F, expect=INVALID, emb=16 + 4)  # misaligned


# ------------------------------------------------------------------------------------------------
# every pattern of the batch: bitwise tspm_pattern_head_train_step on the gathered rows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["p0", "p0.5mask", "gen"])
@pytest.mark.parametrize("pats", PATSETS, ids=T._ids(PATSETS))
@pytest.mark.parametrize("shape", SHAPES, ids=T._ids(SHAPES))
def test_every_pattern_mode_is_bitwise_the_uncached_call_on_gathered_rows(gpu, shape, pats, mode):
    B, F, wa, H, H2, C = shape
    P = len(pats)
    emb, labels_all, idx, x0, W = cache_case(shape)
    x, labels = emb[idx].clone(), labels_all[idx].clone()
    kw = dict(stats0=(1.5, 2.0, 3.0))
    if mode == "p0.5mask":
        kw.update(p=0.5, mask=T.mask_for(shape, P))
    ctr = lambda: torch.tensor([41], dtype=torch.int64, device=gpu)  # noqa: E731
    if mode == "gen":
        c_ref, c_got = ctr(), ctr()
        ref = T.run(gpu, shape, pats, x, x0, labels, W, p=0.5, gen_keep=1, seed=0x1234_5678_9ABC, counter=c_ref,
                    adam_step=c_ref, **kw)
        got = run_cached(gpu, shape, pats, emb, labels_all, idx, x0, W, p=0.5, gen_keep=1, seed=0x1234_5678_9ABC,
                         counter=c_got, adam_step=c_got, **kw)
        assert c_ref.item() == 42 and c_got.item() == 42  # bumped once, by launch 2
    else:
        ref = T.run(gpu, shape, pats, x, x0, labels, W, **kw)
        got = run_cached(gpu, shape, pats, emb, labels_all, idx, x0, W, lde=F + 8 if shape == SHAPES[0] else None,
                         **kw)
    same(got, ref)
    if mode != "p0":
        assert torch.equal(got["mask"], ref["mask"])
    # a second call on the same inputs is bitwise equal
    if mode == "gen":
        c2 = ctr()
        again = run_cached(gpu, shape, pats, emb, labels_all, idx, x0, W, p=0.5, gen_keep=1, seed=0x1234_5678_9ABC,
                           counter=c2, adam_step=c2, **kw)
        assert torch.equal(again["mask"], got["mask"])
    else:
        again = run_cached(gpu, shape, pats, emb, labels_all, idx, x0, W, **kw)
    same(again, got)


# ------------------------------------------------------------------------------------------------
# one pattern per sample
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pat", ["a", "ai", "i"])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[3]], ids=T._ids([SHAPES[0], SHAPES[2], SHAPES[3]]))
def test_per_sample_mode_with_one_flag_pair_is_bitwise_the_every_pattern_mode(gpu, shape, pat):
    B = shape[0]
    emb, labels_all, idx, x0, W = cache_case(shape)
    mask = T.mask_for(shape, 1)
    every = run_cached(gpu, shape, (pat,), emb, labels_all, idx, x0, W, p=0.5, mask=mask)
    rk = torch.tensor([R.KEEP[pat]] * B, dtype=torch.uint8)
    per = run_cached(gpu, shape, None, emb, labels_all, idx, x0, W, p=0.5, mask=mask, rk=rk,
                     rg=torch.zeros(B, dtype=torch.int32))
    same(per, every)


def mixed_flags(B, kind):
    if kind == "no_audio":
        return torch.tensor([(0, 1)] * B, dtype=torch.uint8)
    return torch.tensor([(1, 0), (0, 1), (1, 1), (0, 1), (1, 1), (1, 0), (1, 0)], dtype=torch.uint8)[torch.arange(B) % 7]


@pytest.mark.parametrize("p", [0.0, 0.5], ids=["p0", "p0.5"])
@pytest.mark.parametrize("kind", ["mixed", "no_audio"])
@pytest.mark.parametrize("shape", SHAPES, ids=T._ids(SHAPES))
def test_per_sample_mode_against_the_fp64_chain(gpu, shape, kind, p):
    B, F, wa, H, H2, C = shape
    emb, labels_all, idx, x0, W = cache_case(shape)
    rk = mixed_flags(B, kind)
    mask = T.mask_for(shape, 1) if p else None
    out = run_cached(gpu, shape, None, emb, labels_all, idx, x0, W, p=p, mask=mask, rk=rk,
                     rg=torch.zeros(B, dtype=torch.int32), stats0=(1.5, 2.0, 3.0))
    real = torch.where((torch.arange(F) < wa).unsqueeze(0), rk[:, :1].bool(), rk[:, 1:].bool())
    X = torch.where(real, emb[idx], x0.unsqueeze(0).expand(B, F))
    labels = labels_all[idx]
    full = ((1, 1),)
    r64 = R.chain(X, x0, full, wa, W, labels, LOSS_WEIGHT, p, mask, torch.float64)
    r32 = R.chain(X, x0, full, wa, W, labels, LOSS_WEIGHT, p, mask, torch.float32)
    ratios = parity.Ratios()
    tag = f"[{shape},{kind},p={p}]"
    parity.op_check("logits" + tag, out["logits"], r32["logits"], r64["logits"], ratios=ratios)
    parity.op_check("loss" + tag, out["loss"], r32["loss"], r64["loss"], ratios=ratios)
    for g in GRADS:
        parity.op_check(g + tag, out[g], r32["g" + g[1:]], r64["g" + g[1:]], grad=True, ratios=ratios)
    print("worst ratios:", ratios)
    own_correct = int((out["logits"].argmax(1) == labels).sum())
    assert out["stats"][1].item() == 2.0 + own_correct and out["stats"][2].item() == 3.0 + B


# ------------------------------------------------------------------------------------------------
# the folded bookkeeping
# ------------------------------------------------------------------------------------------------
def classify_ref(dev, logits, labels, groups, n_groups, loss, entries, samples, cap, C):
    """tspm_classify_update on given logits -> (confusion, loss_log, counters) on the CPU."""
    conf = torch.zeros(n_groups, C, C, dtype=torch.int64, device=dev)
    loss_log = torch.full((cap + 2,), -1.0, device=dev)
    counters = torch.tensor([entries, samples], dtype=torch.int64, device=dev)
    lg, lb, gr, ls = logits.to(dev).contiguous(), labels.to(dev), groups.to(dev).to(torch.int32), loss.to(dev)
    L.check(L.lib().tspm_classify_update(lg.shape[0], C, lg.data_ptr(), lb.data_ptr(), gr.data_ptr(), n_groups,
                                         conf.data_ptr(), None, ls.data_ptr(), loss_log.data_ptr(), counters.data_ptr(),
                                         cap, L.stream_handle()), "classify_update")
    torch.cuda.synchronize()
    return conf.cpu(), loss_log.cpu(), counters.cpu()


@pytest.mark.parametrize("entries", [0, 4, 5, 9], ids=lambda e: f"entries{e}")
@pytest.mark.parametrize("per_sample", [False, True], ids=["every", "per_sample"])
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3]], ids=T._ids([SHAPES[2], SHAPES[3]]))
def test_folded_bookkeeping_is_tspm_classify_update_on_the_calls_own_logits(gpu, shape, per_sample, entries):
    """log_capacity 5: entries 0 and 4 are written, 5 and 9 are not; group 3 of 3 and group -1 are out of range."""
    B, C = shape[0], shape[-1]
    emb, labels_all, idx, x0, W = cache_case(shape)
    cap, n_groups = 5, 3
    conf = torch.zeros(n_groups, C, C, dtype=torch.int64, device=gpu)
    loss_log = torch.full((cap + 2,), -1.0, device=gpu)
    counters = torch.tensor([entries, 1000], dtype=torch.int64, device=gpu)
    log = (conf, loss_log, counters, cap, n_groups)
    if per_sample:
        rk = mixed_flags(B, "mixed")
        rg = torch.tensor([2, 0, 1, 3, -1, 1, 0], dtype=torch.int32)[torch.arange(B) % 7]
        out = run_cached(gpu, shape, None, emb, labels_all, idx, x0, W, rk=rk, rg=rg, log=log)
        groups, labels = rg, labels_all[idx]
    else:
        pats, gids = ("a", "ai", "i"), (2, 3, 0)
        out = run_cached(gpu, shape, pats, emb, labels_all, idx, x0, W, gids=gids, log=log)
        groups = torch.tensor(gids, dtype=torch.int32).repeat_interleave(B)
        labels = labels_all[idx].repeat(3)
    want = classify_ref(gpu, out["logits"], labels, groups, n_groups, out["loss"], entries, 1000, cap, C)
    assert torch.equal(conf.cpu(), want[0])
    assert torch.equal(bits(loss_log.cpu()), bits(want[1]))
    assert torch.equal(counters.cpu(), want[2])
    counted = int(((groups >= 0) & (groups < n_groups)).sum())
    assert int(conf.sum()) == counted < groups.numel()            # the out-of-range groups' rows are not counted
    assert counters.tolist() == [entries + 1, 1000 + groups.numel()]
    assert (loss_log[entries].item() == out["loss"].item()) if entries < cap else bool((loss_log == -1.0).all())
    # without the log nothing else changes; counters without loss_log only count
    plain = run_cached(gpu, shape, None, emb, labels_all, idx, x0, W, rk=rk, rg=rg) if per_sample else \
        run_cached(gpu, shape, pats, emb, labels_all, idx, x0, W, gids=gids)
    same(plain, out)
    c2 = torch.tensor([entries, 7], dtype=torch.int64, device=gpu)
    run_cached(gpu, shape, ("ai",), emb, labels_all, idx, x0, W, log=(None, None, c2, 0, 1))
    assert c2.tolist() == [entries + 1, 7 + B]


# ------------------------------------------------------------------------------------------------
# bad inputs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_sample", [False, True], ids=["every", "per_sample"])
@pytest.mark.parametrize("what,bad", [("index", N_ROWS), ("index", -1), ("index", 1 << 40), ("label", 10),
                                      ("label", -1), ("label", 1 << 40)])
def test_out_of_range_index_or_label(gpu, what, bad, per_sample):
    shape, pats = SHAPES[2], (None if per_sample else PATSETS[0])
    B, C = shape[0], shape[-1]
    P = 1 if per_sample else len(PATSETS[0])
    emb, labels_all, idx, x0, W = cache_case(shape)
    kw = dict(rk=mixed_flags(B, "mixed"), rg=torch.zeros(B, dtype=torch.int32)) if per_sample else {}
    conf = torch.zeros(3, C, C, dtype=torch.int64, device=gpu)
    good = run_cached(gpu, shape, pats, emb, labels_all, idx, x0, W, **kw)
    bad_idx, bad_labels = idx.clone(), labels_all.clone()
    if what == "index":
        bad_idx[4] = bad
    else:
        free = next(r for r in range(N_ROWS) if r not in set(idx.tolist()))  # a row nobody else of this batch reads
        bad_idx[4] = free
        bad_labels[free] = bad
    out = run_cached(gpu, shape, pats, emb, bad_labels, bad_idx, x0, W, log=(conf, None, None, 0, 3), **kw)
    assert torch.isnan(out["loss"]).all() and torch.isnan(out["stats"][0])
    ok = (torch.arange(B) != 4).repeat(P)
    assert torch.equal(bits(out["logits"][ok]), bits(good["logits"][ok]))
    assert torch.isnan(out["gw5"]).all() and torch.isnan(out["gb5"]).all()
    for g in ("gw3", "gb3", "gw0", "gb0"):
        assert torch.isnan(out[g]).any(), g
    assert int(conf.sum()) == (B - 1) * P                        # the bad sample's rows are not counted
    want = int((out["logits"].argmax(1) == labels_all[idx].repeat(P))[ok].sum())
    assert out["stats"][1].item() == want and out["stats"][2].item() == P * B


def test_refusals_launch_nothing(gpu):
    shape, pats = SHAPES[0], PATSETS[0]
    B, F, wa, H, H2, C = shape
    emb, labels_all, idx, x0, W = cache_case(shape)
    args = (gpu, shape, pats, emb, labels_all, idx, x0, W)
    some = torch.zeros(64, dtype=torch.int64, device=gpu)
    sp = some.data_ptr()
    invalid = [dict(batch=0), dict(npat=0), dict(npat=9), dict(in_=0), dict(in_=260), dict(hidden=260), dict(hidden2=132),
               dict(classes=17), dict(hidden=H + 2), dict(w_audio=0), dict(w_audio=F), dict(w_audio=wa + 2),
               dict(n_rows=0), dict(ld_emb=F - 4), dict(ld_emb=F + 2), dict(emb=None), dict(rows=None),
               dict(labels_all=None), dict(keep=None), dict(w0=None), dict(b5=None), dict(logits=None), dict(gw0=None),
               dict(gb5=None), dict(loss=None), dict(p=1.0), dict(p=-0.1), dict(p=0.5, keep_mask=None), dict(x0=None),
               dict(log_capacity=-1), dict(loss_log=sp), dict(confusion=sp, n_groups=0),
               dict(confusion=sp, group_id=None), dict(row_keep=sp), dict(row_group=sp),
               dict(row_keep=sp, row_group=sp),               # per-sample mode with npat = 3 and a host keep
               dict(emb=16 + 4), dict(w3=16 + 4)]
    for over in invalid:
        run_cached(*args, expect=INVALID, **over)
    # per-sample mode: npat must be 1, host keep NULL, x0 given
    rk, rg = torch.ones(B, 2, dtype=torch.uint8), torch.zeros(B, dtype=torch.int32)
    keep1 = (ctypes.c_int32 * 2)(1, 1)
    per = (gpu, shape, None, emb, labels_all, idx, x0, W)
    for over in (dict(keep=keep1), dict(x0=None), dict(row_group=None), dict(row_keep=None)):
        run_cached(*per, rk=rk, rg=rg, expect=INVALID, **over)
    for over in (dict(workspace=None), dict(workspace_bytes=15), dict(workspace_bytes=0)):
        run_cached(*args, expect=WORKSPACE, **over)
    need = int(L.lib().tspm_cached_head_train_workspace(B, len(pats)))
    run_cached(*args, expect=WORKSPACE, workspace_bytes=need - 1)
    assert L.lib().tspm_cached_head_train_workspace(0, 1) == 0 and L.lib().tspm_cached_head_train_workspace(4, 9) == 0
    assert L.lib().tspm_cached_head_train_step(None, L.stream_handle()) == INVALID
