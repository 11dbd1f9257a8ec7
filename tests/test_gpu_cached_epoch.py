"""Several cached head steps per host call, on the device: ``FusedCachedHeadStep(steps=K)`` and
``FusedCachedEvalStep(steps=K)`` against K runs of the ``steps=1`` steps, ``EpochRunner.train_epoch`` / ``validate_epoch``
with ``steps_per_call`` against the per-batch epochs, and ``fit(cache_embeddings=True, steps_per_call=K)``.  Everything is
compared bitwise: a K-step call is K single steps.  43 synthetic samples at B = 8 (5 full batches and a tail of 3),
test_gpu_avmnist_head_stage's model."""
import random

import numpy as np
import pytest
import torch

import head_stage_ref as R
import test_gpu_avmnist_head_stage as HS
from tspm_amd import _lib as L

pytestmark = pytest.mark.gpu

ALL, N, B, K = HS.ALL, 43, 8, 4
FLAGS = torch.tensor([R.KEEP[p] for p in ALL], dtype=torch.uint8)  # by group id


def _ds(gpu, split="train", n=N, seed=5, **kw):
    from tspm_amd.data import AVMNIST, synthetic_corpus
    return AVMNIST(None, split, "multimodal", corpus=synthetic_corpus(n, seed), device=gpu, **kw)


def _batches(gpu, calls, per):
    """``calls`` x (ids [K*B], keep [K*B, 2], groups [K*B]): every batch its own rows, with repeats, row 0 and row 42."""
    out = []
    for c in range(calls):
        g = torch.Generator().manual_seed(300 + c)
        ids = torch.randint(0, N, (K * B,), generator=g)
        ids[0], ids[-1], ids[B + 2] = N - 1, 0, ids[B + 1]
        gid = torch.randint(0, 3, (K * B,), generator=g).to(torch.int32)
        if c == 1:
            gid[B:2 * B] = 2                                    # a batch in which no row keeps audio
        out.append((ids.to(gpu),) + ((FLAGS[gid.long()].to(gpu), gid.to(gpu)) if per else ()))
    return out


def _head_state(model, opt):
    fg = opt.flat_groups()[0]
    return {"param": fg.param.clone(), "exp_avg": fg.exp_avg.clone(), "exp_avg_sq": fg.exp_avg_sq.clone(),
            "grad": fg.grad.clone(), "step": int(fg.hyper.view(torch.int64)[6]),
            "state_step": [float(opt.state[p]["step"]) for p in fg.params],
            **{"net." + n: p.detach().clone() for n, p in model.net.named_parameters()}}


def _same_state(a, b):
    for k, v in a.items():
        if torch.is_tensor(v):
            assert torch.equal(v.view(torch.int32) if v.dtype == torch.float32 else v,
                               b[k].view(torch.int32) if v.dtype == torch.float32 else b[k]), k
        else:
            assert v == b[k], (k, v, b[k])


@pytest.mark.parametrize("kind", ["every", "per_sample"])
def test_four_steps_per_call_are_twelve_single_steps(gpu, monkeypatch, kind):
    from tspm_amd.metrics import ClassificationLog
    from tspm_amd.step import FusedCachedHeadStep
    per = kind == "per_sample"
    ds = _ds(gpu)
    model, twin = HS._model(gpu), HS._model(gpu)
    opt, topt = HS._opt(model), HS._opt(twin)
    enc0 = HS._encoder_state(model)
    cache, tcache = ds.embedding_cache(model), ds.embedding_cache(twin)
    log, tlog = ClassificationLog(gpu), ClassificationLog(gpu)
    st = FusedCachedHeadStep(model, opt, None, B, cache, per_sample=per, log=log, steps=K)
    one = FusedCachedHeadStep(twin, topt, None, B, tcache, per_sample=per, log=tlog)
    assert st.steps == K and st.rows.shape == (K * B,) and st.row_keep.shape == (K * B, 2) and one.rows.shape == (B,)
    P = 1 if per else 3
    for c, args in enumerate(_batches(gpu, 3, per)):            # eager, capture, replay
        if c == 0:
            rec = HS._Recorder(L.lib())
            monkeypatch.setattr(L, "lib", lambda: rec)
        out = st.step(*args)
        if c == 0:
            monkeypatch.undo()
            assert [x for x in rec.calls if "adam" in x or "head" in x or "gather" in x or "classify" in x] == \
                ["tspm_cached_head_train_steps"], rec.calls     # no separate Adam launch
        for k in range(K):
            tout = one.step(*[a[k * B:(k + 1) * B] for a in args])
        assert out["logits"].shape == ((B, 10) if per else (3, B, 10))
        assert torch.equal(out["logits"], tout["logits"]) and torch.equal(out["loss"], tout["loss"]), c
        assert torch.equal(st.keep, one.keep) and 0.3 < st.keep.float().mean().item() < 0.7
        _same_state(_head_state(model, opt), _head_state(twin, topt))
        assert int(opt.flat_groups()[0].hyper.view(torch.int64)[6]) == (c + 1) * K
    assert st.graph is not None and st.calls == 3 and one.calls == 3 * K
    conf, ll, rows = log.fetch()
    tconf, tll, trows = tlog.fetch()
    assert len(ll) == 3 * K and rows == trows == 3 * K * P * B and np.array_equal(conf, tconf)
    assert ll.tolist() == tll.tolist() and len(set(ll.tolist())) == 3 * K
    HS._assert_encoders_untouched(model, enc0)


def test_multi_step_refusals(gpu):
    from tspm_amd.step import FusedCachedEvalStep, FusedCachedHeadStep
    ds = _ds(gpu)
    model = HS._model(gpu)
    opt = HS._opt(model)
    cache = ds.embedding_cache(model)
    mk = lambda **kw: FusedCachedHeadStep(model, opt, None, B, cache, **kw)  # noqa: E731
    with pytest.raises(L.TspmError, match='head="launches" has no multi-step form'):
        mk(steps=2, head="launches")
    with pytest.raises(L.TspmError, match="steps must be 1 .. 64"):
        mk(steps=0)
    with pytest.raises(L.TspmError, match="steps must be 1 .. 64"):
        mk(steps=65)
    with pytest.raises(L.TspmError, match="steps must be 1 .. 64"):
        FusedCachedEvalStep(model, None, B, cache, steps=65)
    st = mk(steps=2)
    with pytest.raises(L.TspmError, match="built for 16 samples, got 8 ids"):
        st.step(torch.arange(8, device=gpu))
    st.keep_override = st.keep.clone()
    with pytest.raises(L.TspmError, match="keep_override holds one step's mask"):
        st.step(torch.arange(16, device=gpu))
    st.keep_override = None
    opt.clip_coef = torch.ones(1, device=gpu)
    try:
        with pytest.raises(L.TspmError, match="no clip coefficient"):
            st.step(torch.arange(16, device=gpu))
        with pytest.raises(L.TspmError, match="no clip coefficient"):
            mk(steps=2)
    finally:
        opt.clip_coef = None
    # what the runner asks before it builds a multi-step step (else the epoch runs per batch, without raising)
    from tspm_amd.harness import EpochRunner
    runner = EpochRunner(model, opt, None)
    assert runner._multi_step_ok(3) and runner._multi_step_ok(1) and not runner._multi_step_ok(9)
    opt.clip_coef = torch.ones(1, device=gpu)
    try:
        assert not runner._multi_step_ok(3)
    finally:
        opt.clip_coef = None


@pytest.mark.parametrize("per", [False, True], ids=["fused_patterns", "per_pattern"])
def test_three_eval_batches_per_call_are_three_single_replays(gpu, per):
    from tspm_amd.metrics import ClassificationLog
    from tspm_amd.step import FusedCachedEvalStep
    model = HS._model(gpu)
    ds = _ds(gpu, "valid")
    cache = ds.embedding_cache(model)
    log, tlog = ClassificationLog(gpu), ClassificationLog(gpu)
    st = FusedCachedEvalStep(model, None, B, cache, log, per_sample=per, steps=3)
    one = FusedCachedEvalStep(model, None, B, cache, tlog, per_sample=per)
    for c in range(2):                                          # capture, replay
        g = torch.Generator().manual_seed(40 + c)
        ids = torch.randint(0, N, (3 * B,), generator=g).to(gpu)
        gid = torch.randint(0, 3, (3 * B,), generator=g).to(torch.int32)
        args = (ids,) + ((FLAGS[gid.long()].to(gpu), gid.to(gpu)) if per else ())
        out = st.step(*args)
        for k in range(3):
            tout = one.step(*[a[k * B:(k + 1) * B] for a in args])
        for key in ("logits", "loss", "preds"):
            assert torch.equal(out[key], tout[key]), (key, c)
    conf, ll, rows = log.fetch()
    tconf, tll, trows = tlog.fetch()
    assert len(ll) == (6 if per else 18) and rows == trows and np.array_equal(conf, tconf) and ll.tolist() == tll.tolist()


def _epoch_pair(gpu, train, kw, split):
    """The same epoch twice — per batch and with steps_per_call=4 — on twin loaders, models and optimizers."""
    from tspm_amd.harness import EpochRunner
    res = []
    for spc in (None, K):
        model = HS._model(gpu)
        opt = HS._opt(model)
        ds = _ds(gpu, split)
        runner = EpochRunner(model, opt, None)
        loader = ds.device_loader(B, generator=torch.Generator().manual_seed(3), ids_only=True, **kw)
        epoch = runner.train_epoch if train else runner.validate_epoch
        random.seed(12)
        loss, _, metrics, n = epoch(loader) if spc is None else epoch(loader, steps_per_call=spc)
        conf, ll, rows = runner.log.fetch()
        res.append(dict(loss=loss, metrics=metrics, n=n, conf=conf, ll=ll.tolist(), rows=rows,
                        state=_head_state(model, opt), keys=list(runner.train_steps)))
    return res


@pytest.mark.parametrize("kw", [dict(shuffle=True), dict(shuffle=True, all_patterns=True)], ids=["plain", "all_patterns"])
def test_train_epoch_with_steps_per_call_is_the_per_batch_epoch(gpu, kw):
    a, b = _epoch_pair(gpu, True, kw, "train")
    assert a["n"] == b["n"] == 6 and a["ll"] == b["ll"] and a["loss"] == b["loss"] and a["rows"] == b["rows"]
    assert np.array_equal(a["conf"], b["conf"]) and set(a["metrics"]) == set(b["metrics"])
    for k in a["metrics"]:
        assert np.array_equal(np.asarray(a["metrics"][k]), np.asarray(b["metrics"][k])), k
    _same_state(a["state"], b["state"])
    assert a["state"]["step"] == 6
    # 5 full batches at K = 4: one call of 4, the remaining full batch and the tail of 3 on single steps
    assert sorted(k[-1][1] if k[-1][0] == "steps" else 1 for k in b["keys"]) == [1, 1, 4], b["keys"]
    assert sorted(k[-1][1] if k[-1][0] == "steps" else 1 for k in a["keys"]) == [1, 1], a["keys"]


@pytest.mark.parametrize("kw", [dict(), dict(fuse_patterns=True)], ids=["per_pattern", "fused_patterns"])
def test_validate_epoch_with_steps_per_call_is_the_per_batch_epoch(gpu, kw):
    a, b = _epoch_pair(gpu, False, kw, "valid")
    assert a["n"] == b["n"] and a["ll"] == b["ll"] and a["loss"] == b["loss"] and a["rows"] == b["rows"]
    assert np.array_equal(a["conf"], b["conf"])
    for k in a["metrics"]:
        assert np.array_equal(np.asarray(a["metrics"][k]), np.asarray(b["metrics"][k])), k


def test_steps_per_call_needs_an_ids_only_device_loader(gpu):
    from tspm_amd.harness import EpochRunner
    model = HS._model(gpu)
    runner = EpochRunner(model, HS._opt(model), None)
    ds = _ds(gpu)
    with pytest.raises(L.TspmError, match="ids_only"):
        runner.train_epoch(ds.device_loader(B), steps_per_call=K)
    with pytest.raises(L.TspmError, match="ids_only"):
        runner.validate_epoch([{"cached": True}], steps_per_call=K)


def test_fit_with_steps_per_call_gives_the_same_history(gpu):
    from tspm_amd import harness

    def run(spc):
        model = HS._model(gpu)
        opt = HS._opt(model)
        tr, va = _ds(gpu), _ds(gpu, "valid", 21, 6)
        loaders = {"train": tr.device_loader(B, shuffle=True, generator=torch.Generator().manual_seed(3),
                                             all_patterns=True),
                   "validation": va.device_loader(B, fuse_patterns=True), "test": va.device_loader(B, fuse_patterns=True)}
        kw = {} if spc is None else dict(steps_per_call=spc)
        h = harness.fit(model, opt, None, loaders, epochs=2, early_stopping=False, cache_embeddings=True, **kw)
        return h, _head_state(model, opt)

    (ha, sa), (hb, sb) = run(None), run(K)
    _same_state(sa, sb)

    def strip(o):
        if isinstance(o, dict):
            return {k: strip(v) for k, v in o.items() if "tim" not in k and "seconds" not in k}
        if isinstance(o, (list, tuple)):
            return [strip(v) for v in o]
        return np.asarray(o).tolist()
    assert strip(ha) == strip(hb)
    assert len(ha["train"]) == 2 and "test" in ha and np.isfinite(ha["test"]["loss"])
