"""The AVMNIST head stage on cached embeddings, on the device: ``data.AVMNIST.embedding_cache`` (the fill and its guards),
``step.FusedCachedHeadStep`` (every pattern of the batch and one pattern per sample, both head legs),
``step.FusedCachedEvalStep`` and ``fit(cache_embeddings=True)``.  A synthetic corpus of 37 samples with B = 8 (a short last
batch), default encoders on non-default running statistics (test_gpu_avmnist_head_stage's model)."""
import types

import numpy as np
import pytest
import torch

import head_stage_ref as R
import parity
import test_gpu_avmnist_head_stage as HS
from oracle import avmnist_ref as orc
from tspm_amd import _lib as L

pytestmark = pytest.mark.gpu

ALL, N, B = HS.ALL, 37, 8
FLAGS = torch.tensor([R.KEEP[p] for p in ALL], dtype=torch.uint8)  # by group id, ("a", "ai", "i") order


def _ds(gpu, split="train", n=N, seed=5, **kw):
    from tspm_amd.data import AVMNIST, synthetic_corpus
    return AVMNIST(None, split, "multimodal", corpus=synthetic_corpus(n, seed), device=gpu, **kw)


def _ids(k, gpu):
    """Three batches of 8 indices: two runs of the corpus and one with a repeat, row 0 and the last row."""
    return [torch.arange(0, 8), torch.arange(20, 28), torch.tensor([36, 3, 3, 0, 17, 36, 9, 30])][k].to(gpu)


def test_cache_rows_are_the_encoders_eval_embeddings(gpu):
    model = HS._model(gpu)
    enc0 = HS._encoder_state(model)
    ds = _ds(gpu)
    cache = ds.embedding_cache(model, chunk=16)            # chunks of 16, 16 and 5 rows
    assert ds.embedding_cache(model) is cache and cache.fills == 1 and cache.stale_reason() is None
    assert cache.emb.shape == (N, 192) and cache.emb.dtype == torch.float32 and cache.emb.is_contiguous()
    assert cache.labels_all.dtype == torch.int64 and np.array_equal(cache.labels_all.cpu().numpy(), ds.corpus.labels)
    # x0 is zero_embeddings()' buffer and value
    assert cache.x0.data_ptr() == model.zero_embeddings(refresh=False).data_ptr()
    x0 = cache.x0.clone()
    assert torch.equal(model.zero_embeddings(refresh=True), x0)
    # the rows against the oracle encoders' eval forward on the very inputs the gather assembles, in fp64, with the fp32
    # CPU oracle as yardstick
    a, i, lab = ds.device_corpus.gather(torch.arange(N, device=gpu))
    o32, o64 = parity.pair_from(model, lambda: orc.build_oracle_avmnist(0))
    with torch.no_grad():
        for name, enc32, enc64, x, cols in (("audio", o32.audio_encoder, o64.audio_encoder, a.cpu(), slice(0, 64)),
                                            ("image", o32.image_encoder, o64.image_encoder, i.cpu(), slice(64, 192))):
            r32 = orc.encoder_forward(enc32, x, False)
            r64 = orc.encoder_forward(enc64, x.double(), False)
            parity.op_check(f"cache rows ({name})", cache.emb[:, cols], r32, r64)
        z32 = torch.cat([orc.encoder_forward(o32.audio_encoder, torch.zeros(1, 32, 94), False),
                         orc.encoder_forward(o32.image_encoder, torch.zeros(1, 1, 28, 28), False)], 1)
        z64 = torch.cat([orc.encoder_forward(o64.audio_encoder, torch.zeros(1, 32, 94).double(), False),
                         orc.encoder_forward(o64.image_encoder, torch.zeros(1, 1, 28, 28).double(), False)], 1)
        parity.op_check("x0", x0, z32, z64)
    # a second fill is bitwise the first; the fill changes nothing in the encoders
    first = cache.emb.clone()
    assert ds.embedding_cache(model, refresh=True) is cache and cache.fills == 2
    assert torch.equal(cache.emb, first)
    HS._assert_encoders_untouched(model, enc0)


def _uncached(kind, model, opt, use_graph=False):
    """The uncached head-stage step of ``kind`` with its encoder leg disabled: it trains on whatever ``fused`` holds."""
    from tspm_amd.step import FusedHeadStagePatternStep, FusedHeadStageStep
    st = FusedHeadStageStep(model, opt, None, B, use_graph=use_graph) if kind == "per_sample" else \
        FusedHeadStagePatternStep(model, opt, None, B, head="kernel", use_graph=use_graph)
    st._encoders = lambda fused: torch.cuda.current_stream().cuda_stream
    return st


@pytest.mark.parametrize("head", ["kernel", "launches"])
@pytest.mark.parametrize("kind", ["every", "per_sample"])
def test_three_cached_steps_on_one_graph_vs_fp64_eager_and_the_uncached_head(gpu, monkeypatch, kind, head):
    from tspm_amd.metrics import ClassificationLog
    from tspm_amd.step import FusedCachedHeadStep
    ds = _ds(gpu)
    twin, model, um = HS._model(gpu), HS._model(gpu), HS._model(gpu)
    topt, opt, uopt = HS._opt(twin), HS._opt(model), HS._opt(um)
    enc0 = HS._encoder_state(model)
    tcache, cache = ds.embedding_cache(twin), ds.embedding_cache(model)
    assert tcache is not cache and torch.equal(tcache.emb, cache.emb)
    tlog, log, ulog = ClassificationLog(gpu), ClassificationLog(gpu), ClassificationLog(gpu)
    per = kind == "per_sample"
    kw = dict(per_sample=per, head=head)
    tst = FusedCachedHeadStep(twin, topt, None, B, tcache, log=tlog, use_graph=False, **kw)
    st = FusedCachedHeadStep(model, opt, None, B, cache, log=log, use_graph=True, **kw)
    assert st.head == head and not hasattr(st, "eng_a") and not hasattr(st, "A")
    ust = _uncached(kind, um, uopt)
    ust.log = ulog
    ratios = parity.Ratios()
    P = 1 if per else 3
    zA, zI = torch.zeros(B, 32, 94, device=gpu), torch.zeros(B, 1, 28, 28, device=gpu)
    for k in range(3):  # eager, capture, replay: three different batches
        ids = _ids(k, gpu)
        gid = torch.randint(0, 3, (B,), generator=torch.Generator().manual_seed(70 + k)).to(torch.int32)
        if k == 2 and per:
            gid[:] = 2                                  # a batch in which no row keeps audio
        keep = FLAGS[gid.long()].to(gpu)
        args = (ids, keep, gid.to(gpu)) if per else (ids,)
        if k == 0:
            rec = HS._Recorder(L.lib())
            monkeypatch.setattr(L, "lib", lambda: rec)
        tout = {kk: v.clone() for kk, v in tst.step(*args).items()}
        if k == 0:
            monkeypatch.undo()
            calls = rec.calls
            assert not [c for c in calls if c.startswith(("tspm_conv", "tspm_stem", "tspm_bn", "tspm_avmnist_gather",
                                                          "tspm_maxpool", "tspm_linear"))], calls
            assert [c for c in calls if "adam" in c] == ["tspm_adam_step"]  # the head launch advanced the step counter
            legs = ("tspm_cached_head_train_step", "tspm_embed_gather", "tspm_head_train_step",
                    "tspm_pattern_head_train_step", "tspm_classify_update", "tspm_pattern_expand")
            got = [c for c in calls if c in legs]
            if head == "kernel":
                assert got == ["tspm_cached_head_train_step"], calls
            else:
                inner = "tspm_head_train_step" if per else "tspm_pattern_head_train_step"
                assert got == ["tspm_embed_gather", inner, "tspm_classify_update"], calls
        before = HS._snap(model, opt)
        out = st.step(*args)
        assert out["logits"].shape == ((B, 10) if per else (3, B, 10)) and out["loss"].shape == (1,)
        # capture (k = 1) and replay (k = 2) are bitwise the eager twin's
        assert torch.equal(out["logits"], tout["logits"]) and torch.equal(out["loss"], tout["loss"]), k
        for (n, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
            assert torch.equal(p, q), (k, n)
        assert torch.equal(st.keep, tst.keep) and 0.3 < st.keep.float().mean().item() < 0.7
        # the uncached head fed cache.emb[ids] (rows built with torch.where for per-sample flags)
        x, lab = cache.emb[ids], cache.labels_all[ids]
        if per:
            real = torch.where((torch.arange(192, device=gpu) < 64).unsqueeze(0), keep[:, :1].bool(), keep[:, 1:].bool())
            x = torch.where(real, x, cache.x0.unsqueeze(0).expand(B, 192))
        if head == "launches" or not per:  # (per-sample "kernel" is another kernel than tspm_head_train_step's: fp64 only)
            ust.fused.copy_(x)
            uout = ust.step(zA, zI, lab, gid.to(gpu)) if per else ust.step(zA, zI, lab)
            assert torch.equal(out["logits"], uout["logits"]) and torch.equal(out["loss"], uout["loss"]), k
            assert torch.equal(st.keep, ust.keep)
            for (n, p), (_, q) in zip(model.named_parameters(), um.named_parameters()):
                assert torch.equal(p, q), (k, n)
        # against the fp64 chain: test_gpu_avmnist_head_stage's yardstick
        shim = types.SimpleNamespace(fused=x, x0=cache.x0, keep=st.keep, patterns=ALL, ea=64, logits=st.logits,
                                     loss=st.loss)
        HS._check_step("plain" if per else "kernel", model, opt, shim, lab, before, k + 1, ratios)
        HS._assert_encoders_untouched(model, enc0)
    print("worst ratios:", ratios)
    assert st.graph is not None and tst.graph is None and st.calls == 3
    assert int(opt.flat_groups()[0].hyper.view(torch.int64)[6]) == 3
    conf, ll, rows = log.fetch()
    tconf, tll, _ = tlog.fetch()
    assert len(ll) == 3 and rows == 3 * P * B and conf.sum() == rows and np.array_equal(conf, tconf)
    assert ll.tolist() == tll.tolist()
    if head == "launches" or not per:
        uconf, ull, _ = ulog.fetch()
        assert np.array_equal(conf, uconf) and ll.tolist() == ull.tolist()
    if not per:
        assert [int(c.sum()) for c in conf] == [3 * B] * 3


def test_cached_eval_step_is_the_pattern_eval_head_on_the_cache_rows(gpu):
    from tspm_amd.metrics import ClassificationLog
    from tspm_amd.step import FusedCachedEvalStep, FusedPatternEvalStep
    model = HS._model(gpu)
    ds = _ds(gpu, "valid")
    cache = ds.embedding_cache(model)
    log, ulog = ClassificationLog(gpu), ClassificationLog(gpu)
    st = FusedCachedEvalStep(model, None, B, cache, log)
    ust = FusedPatternEvalStep(model, None, B, ulog, use_graph=False)
    a, i, lab = ds.device_corpus.gather(torch.arange(N, device=gpu))
    for k in range(3):
        ids = _ids(k, gpu)
        out = {kk: v.clone() for kk, v in st.step(ids).items()}
        # the uncached step's head on the same rows: its encoders run on the real inputs, then the rows are the cache's
        ust.load_batch(a[ids], i[ids], lab[ids])
        ust.model.eval()
        ust._bind_log()
        ust.fused.copy_(cache.emb[ids])
        ust._head_kernel(torch.cuda.current_stream().cuda_stream)
        assert torch.equal(out["logits"].reshape(-1, 10), ust.logits) and torch.equal(out["loss"], ust.loss)
        assert torch.equal(out["preds"].reshape(-1), ust.preds)
    conf, ll, rows = log.fetch()
    uconf, ull, urows = ulog.fetch()
    assert len(ll) == 9 and rows == urows == 9 * B and np.array_equal(conf, uconf) and ll.tolist() == ull.tolist()
    # a per-pattern batch: each row under its own flags, one loss entry
    pst = FusedCachedEvalStep(model, None, B, cache, log, per_sample=True)
    gid = torch.tensor([0, 1, 2, 2, 1, 0, 0, 1], dtype=torch.int32)
    out = pst.step(_ids(2, gpu), FLAGS[gid.long()].to(gpu), gid.to(gpu))
    full = st.step(_ids(2, gpu))["logits"]
    want = torch.stack([full[int(g), r] for r, g in enumerate(gid.tolist())])
    parity.op_check("per-pattern eval logits", out["logits"], want, want.double())  # another GEMM path than the kernel's
    assert out["loss"].shape == (1,) and log.fetch()[1].shape[0] == 9 + 1 + 3


def test_fit_two_epochs_on_cached_embeddings(gpu, monkeypatch):
    from tspm_amd import harness
    from tspm_amd.engine import EncoderEngine

    entries = []
    orig_finish = harness.EpochRunner._finish

    def finish(self, t0, loss=None):
        out = orig_finish(self, t0, loss)
        entries.append(out[3])
        return out
    monkeypatch.setattr(harness.EpochRunner, "_finish", finish)

    def run(cached):
        model = HS._model(gpu)
        enc0 = HS._encoder_state(model)
        opt = HS._opt(model)
        tr, va = _ds(gpu), _ds(gpu, "valid", 21, 6)
        g = torch.Generator().manual_seed(3)
        loaders = {"train": tr.device_loader(B, shuffle=True, generator=g, all_patterns=True),
                   "validation": va.device_loader(B, fuse_patterns=True)}
        forwards = []
        if cached:
            for d in (tr, va):
                d.embedding_cache(model)             # the fill
            orig = EncoderEngine.forward
            monkeypatch.setattr(EncoderEngine, "forward",
                                lambda self, *a, **k: (forwards.append(1), orig(self, *a, **k))[1])
        del entries[:]
        h = harness.fit(model, opt, None, loaders, epochs=2, early_stopping=False, cache_embeddings=cached)
        if cached:
            monkeypatch.setattr(EncoderEngine, "forward", orig)
            assert forwards == [], f"{len(forwards)} encoder forwards after the fill"
            assert set(h["embedding_cache"]["fill_seconds"]) == {"train", "validation"}
            assert h["embedding_cache"]["rows"] == {"train": N, "validation": 21}
        HS._assert_encoders_untouched(model, enc0)
        assert all(np.isfinite(e["loss"]) for e in h["train"] + h["validation"])
        return h, list(entries)

    hc, nc = run(True)
    hu, nu = run(False)
    assert nc == nu == [5, 9, 5, 9]                   # ceil(37/8) train entries; 3 patterns x ceil(21/8) validation entries
    for split in ("train", "validation"):
        assert [set(e) for e in hc[split]] == [set(e) for e in hu[split]]
    assert set(hc) - {"embedding_cache"} == set(hu)


def test_plain_cached_loaders_through_train_step_and_the_runner(gpu):
    """The default train loader's draw (one pattern per sample) and the plain valid loader, as ``ids_only`` batches."""
    from tspm_amd.harness import AVMNIST_METRICS, EpochRunner
    from tspm_amd.metrics import ClassificationLog, DeviceMetricRecorder
    model = HS._model(gpu)
    opt = HS._opt(model)
    tr, va = _ds(gpu), _ds(gpu, "valid", 21, 6)
    runner = EpochRunner(model, opt, None)
    loss, _, metrics, n = runner.train_epoch(tr.device_loader(B, shuffle=True, ids_only=True))
    fr = ("frozen", ("audio_encoder", "image_encoder"))
    assert n == 5 and np.isfinite(loss) and set(runner.train_steps) == {(8, fr, ("cached",)), (5, fr, ("cached",))}
    assert runner.log.fetch()[2] == N
    loss, _, vmetrics, n = runner.validate_epoch(va.device_loader(B, ids_only=True))
    assert n == 8 and np.isfinite(loss)               # ceil(63 / 8) per-pattern batches
    conf = runner.log.fetch()[0]
    assert [int(c.sum()) for c in conf] == [21, 21, 21]
    # ... against the uncached validation of the same model: the same rows per group, the loss within parity's bound
    uloss, _, umetrics, un = runner.validate_epoch(va.device_loader(B))
    assert un == 8 and [int(c.sum()) for c in runner.log.fetch()[0]] == [21, 21, 21]
    assert abs(uloss - loss) <= parity.LOGITS_REL * abs(uloss)
    assert set(vmetrics) == set(umetrics)
    # model.train_step / validation_step route a "cached" batch too
    rec = DeviceMetricRecorder(AVMNIST_METRICS, ClassificationLog(gpu))
    b = next(iter(tr.device_loader(B, ids_only=True)))
    assert b["cached"] and "audio" not in b and b["keep"].shape == (B, 2) and b["sample_ids"].dtype == torch.int64
    assert np.isfinite(model.train_step(b, opt, None, gpu, rec)["loss"])
    vb = next(iter(va.device_loader(B, fuse_patterns=True, ids_only=True)))
    assert np.isfinite(model.validation_step(vb, None, gpu, rec)["loss"])
    assert len(rec.log.fetch()[1]) == 1 + 3


def test_refusals(gpu):
    import tspm_amd
    from tspm_amd import harness
    from tspm_amd.data import DeviceLoader
    from tspm_amd.step import FusedCachedEvalStep, FusedCachedHeadStep
    ds = _ds(gpu)
    # an unfrozen model: the fill, the step and fit
    model = HS._model(gpu, frozen=False)
    with pytest.raises(L.TspmError, match="not frozen"):
        ds.embedding_cache(model)
    with pytest.raises(L.TspmError, match="frozen encoders"):
        harness.fit(model, HS._opt(model), None, {"train": ds.device_loader(B), "validation": ds.device_loader(B)},
                    epochs=1, cache_embeddings=True)
    # a single-modality target; fractional presence probabilities; out= together with ids_only
    with pytest.raises(L.TspmError, match="multimodal target"):
        tspm_amd.data.AVMNIST(None, "train", "audio", corpus=ds.corpus, device=gpu).embedding_cache(model)
    frac = tspm_amd.data.AVMNIST(None, "train", "multimodal", corpus=ds.corpus, device=gpu, missing_patterns={
        "ai": {"audio": 1.0, "image": 1.0}, "a": {"audio": 1.0, "image": 0.3}, "i": {"audio": 0.0, "image": 1.0}})
    with pytest.raises(L.TspmError, match="0 / 1 presence probabilities"):
        frac.device_loader(B, ids_only=True)
    with pytest.raises(L.TspmError, match="excludes out="):
        DeviceLoader(ds, B, ids_only=True, out=(None, None, None))
    # a stale cache: load_state_dict on the model or an encoder, unfreeze_encoders(), .to()
    model.freeze_encoders()
    opt = HS._opt(model)
    cache = ds.embedding_cache(model)
    st = FusedCachedHeadStep(model, opt, None, B, cache)
    ids = _ids(0, gpu)
    st.step(ids)
    for how in ("model", "encoder", "unfreeze", "to"):
        if how == "model":
            model.load_state_dict(model.state_dict())
        elif how == "encoder":
            model.image_encoder.load_state_dict(model.image_encoder.state_dict())
        elif how == "unfreeze":
            model.unfreeze_encoders()
            model.freeze_encoders()
        else:
            model.to(gpu, torch.float32)
        assert cache.stale_reason() is not None, how
        with pytest.raises(L.TspmError, match=r"stale EmbeddingCache.*refresh\(\)"):
            st.step(ids)
        with pytest.raises(L.TspmError, match=r"stale EmbeddingCache.*refresh\(\)"):
            FusedCachedEvalStep(model, None, B, cache)
        cache.refresh()
        assert cache.stale_reason() is None
        st.step(ids)                                   # ... and after refresh() the same step runs again
    # unfrozen at the time of use
    model.unfreeze_encoders()
    with pytest.raises(L.TspmError):
        st.step(ids)
    with pytest.raises(L.TspmError, match="not frozen"):
        cache.refresh()
    model.freeze_encoders()
    cache.refresh()
    # another model's cache
    other = HS._model(gpu)
    with pytest.raises(L.TspmError, match="built for another model"):
        FusedCachedHeadStep(other, HS._opt(other), None, B, cache)
    with pytest.raises(L.TspmError, match="built for another model"):
        FusedCachedEvalStep(other, None, B, cache)
    # allreduce; several Adam groups; keep flags handed to an every-pattern step
    with pytest.raises(L.TspmError, match="allreduce"):
        FusedCachedHeadStep(model, opt, None, B, cache, allreduce=object())
    two = tspm_amd.FusedAdam([{"params": list(model.net[0].parameters())},
                              {"params": list(model.net[3].parameters()) + list(model.net[5].parameters())}], lr=1e-3)
    with pytest.raises(L.TspmError, match="one FusedAdam group"):
        FusedCachedHeadStep(model, two, None, B, cache)
    with pytest.raises(L.TspmError, match="per-sample inputs"):
        FusedCachedHeadStep(model, opt, None, B, cache).step(ids, torch.ones(B, 2, dtype=torch.uint8, device=gpu))
    with pytest.raises(L.TspmError, match="built for 8 samples"):
        st.step(ids[:5])


def test_existing_steps_are_bitwise_what_they_were_before_the_cached_paths_ran(gpu):
    """FusedTrainStep on an all-trainable model and the uncached head-stage steps: the same keys and bits whether or
    not the cached code ran in the process."""
    import tspm_amd
    from tspm_amd.harness import EpochRunner

    def unfrozen():
        model = HS._model(gpu, frozen=False)
        opt = HS._opt(model)
        st = tspm_amd.FusedTrainStep(model, opt, None, 4)
        assert st._sig == (id(opt), id(None), 4)
        outs = []
        for k in range(2):
            a, i, lab, gid = HS._batch(4, 400 + k, gpu, masked=True)
            out = st.step(a, i, lab, gid)
            outs += [out["logits"].clone(), out["loss"].clone()]
        runner = EpochRunner(model, opt, None)
        assert runner._train_step(4).__class__ is tspm_amd.FusedTrainStep and set(runner.train_steps) == {4}
        return outs + [p.detach().clone() for p in model.parameters()] + [b.detach().clone() for b in model.buffers()]

    def head_stage():
        outs = []
        for kind in ("plain", "kernel", "launches"):
            model = HS._model(gpu)
            opt = HS._opt(model)
            st = HS._build(kind, model, opt, 4, True)
            fr = ("frozen", ("audio_encoder", "image_encoder"))
            assert st._sig[:4] == (id(opt), id(None), 4, fr) and st.eng_a is model.audio_encoder.engine_for(st.A)
            for k in range(3):
                a, i, lab, gid = HS._batch(4, 600 + k, gpu, masked=(kind == "plain"))
                out = st.step(a, i, lab, gid) if kind == "plain" else st.step(a, i, lab)
                outs += [out["logits"].clone(), out["loss"].clone(), st.keep.clone()]
            outs += [p.detach().clone() for p in model.parameters()]
        return outs

    first = unfrozen() + head_stage()
    frozen = HS._model(gpu)
    fopt = HS._opt(frozen)
    ds = _ds(gpu)
    cache = ds.embedding_cache(frozen)
    for kw in (dict(), dict(head="launches"), dict(per_sample=True), dict(per_sample=True, head="launches")):
        st = tspm_amd.FusedCachedHeadStep(frozen, fopt, None, B, cache, **kw)
        st.step(_ids(2, gpu), *((FLAGS[torch.arange(B) % 3].to(gpu),) if kw.get("per_sample") else ()))
    tspm_amd.FusedCachedEvalStep(frozen, None, B, cache).step(_ids(0, gpu))
    second = unfrozen() + head_stage()
    assert len(first) == len(second) and all(torch.equal(x, y) for x, y in zip(first, second))


def test_fallback_legs_for_a_head_outside_the_fused_kernels_limits(gpu, monkeypatch):
    """A head the fused kernels refuse: the cached train step gathers and runs the uncached step's expand +
    ``tspm_head_train_step`` leg, the cached eval step the uncached eval step's launches — bitwise those steps fed
    ``cache.emb[ids]``."""
    from tspm_amd.metrics import ClassificationLog
    from tspm_amd.step import FusedCachedEvalStep, FusedCachedHeadStep, FusedHeadStagePatternStep, FusedPatternEvalStep
    for name in ("pattern_head_train_supported", "cached_head_train_supported", "pattern_head_eval_supported"):
        monkeypatch.setattr(L, name, lambda *a: False)
    ds = _ds(gpu)
    model, um = HS._model(gpu), HS._model(gpu)
    opt, uopt = HS._opt(model), HS._opt(um)
    cache = ds.embedding_cache(model)
    log, ulog = ClassificationLog(gpu), ClassificationLog(gpu)
    st = FusedCachedHeadStep(model, opt, None, B, cache, head="kernel", log=log)
    assert st.head == "launches" and st._inner == "launches"
    ust = FusedHeadStagePatternStep(um, uopt, None, B, head="kernel", log=ulog, use_graph=False)
    assert ust.head == "launches"
    ust._encoders = lambda fused: torch.cuda.current_stream().cuda_stream
    zA, zI = torch.zeros(B, 32, 94, device=gpu), torch.zeros(B, 1, 28, 28, device=gpu)
    for k in range(3):
        ids = _ids(k, gpu)
        out = st.step(ids)
        ust.fused.copy_(cache.emb[ids])
        uout = ust.step(zA, zI, cache.labels_all[ids])
        assert torch.equal(out["logits"], uout["logits"]) and torch.equal(out["loss"], uout["loss"]), k
        assert torch.equal(st.keep, ust.keep)
        for (n, p), (_, q) in zip(model.named_parameters(), um.named_parameters()):
            assert torch.equal(p, q), (k, n)
    conf, ll, rows = log.fetch()
    uconf, ull, urows = ulog.fetch()
    assert st.graph is not None and len(ll) == 3 and rows == urows == 9 * B
    assert np.array_equal(conf, uconf) and ll.tolist() == ull.tolist() and [int(c.sum()) for c in conf] == [3 * B] * 3
    # evaluation, on the trained head
    elog, uelog = ClassificationLog(gpu), ClassificationLog(gpu)
    est = FusedCachedEvalStep(model, None, B, cache, elog)
    uest = FusedPatternEvalStep(model, None, B, uelog, use_graph=False)
    assert est.head == "launches" and uest.head == "launches"
    model.eval()
    for k in range(3):
        ids = _ids(k, gpu)
        out = {kk: v.clone() for kk, v in est.step(ids).items()}
        uest.labels.copy_(cache.labels_all[ids])
        uest._bind_log()
        uest.fused.copy_(cache.emb[ids])
        uest._head_launches(torch.cuda.current_stream().cuda_stream)
        assert torch.equal(out["logits"].reshape(-1, 10), uest.logits) and torch.equal(out["loss"], uest.loss), k
        assert torch.equal(out["preds"].reshape(-1), uest.preds)
    conf, ll, rows = elog.fetch()
    uconf, ull, urows = uelog.fetch()
    assert est.graph is not None and len(ll) == 9 and rows == urows == 9 * B
    assert np.array_equal(conf, uconf) and ll.tolist() == ull.tolist()
