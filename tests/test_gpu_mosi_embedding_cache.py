"""The UTT-Fusion head stage on cached encoder features: ``UttEmbeddingCache``, the ``ids_only`` loader,
``FusedMosiCachedStep`` / ``FusedMosiCachedEvalStep``, the runner and ``fit(cache_embeddings=True)``.

Shapes are test_gpu_mosi_patterns.py's (B = 5, steps (7, 9, 6) - reached as the ``pad_to`` of a 6-step corpus - widths
(8, 12, 8)); the corpus has 13 samples, so the last batch is short.  Three kinds of check:

* the cache's rows against ``oracle.mosi_ref``'s encoders in fp64 on the very inputs the gather assembles (``op_check``);
* BITWISE against the uncached step whose encoder leg is replaced by a stub that copies the cache's rows with torch
  indexing (``torch.where`` on the masks) and calls the embedding-Linear helper: everything behind the encoders is the
  same code on the same bits, so logits, loss, parameters, Adam moments, masks and logs are ``torch.equal``;
* one cached step against fp64 on the replicated REAL inputs (``test_gpu_mosi_train_patterns._check``), which validates
  the cache end to end and not only against itself.

The ``fit`` comparison: the cached and the uncached run (a covering ``pad_to``) compute the same fp32 function and
differ only by the encoder engines' batch shape, so each epoch's loss is held to twice ``op_check``'s loss bound with
one fp32 ulp in the place of the fp32 reference's error: 2 (FACTOR x 2^-24 + FLOOR_OUT)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import parity
import test_gpu_mosi_finetune as tf
import test_gpu_mosi_patterns as tp
import test_gpu_mosi_regress as tr
import test_gpu_mosi_train_patterns as tt
import tspm_amd
from oracle import mosi_ref as orc
from parity import op_check, pair_from
from tspm_amd import _lib as L
from tspm_amd import harness
from tspm_amd import mosi as M
from tspm_amd.metrics import ClassificationLog, RegressionLog
from tspm_amd.mosi_data import MOSI, PATTERNS, synthetic_mosi_corpus

pytestmark = pytest.mark.gpu
B, STEPS, WIDTHS, PATS = tp.B, tp.STEPS, tp.WIDTHS, tp.PATS
N, T0, ALL = 13, 6, ("audio", "video", "text")
HAV, NC = WIDTHS[0] + WIDTHS[1], 3 * 128
ROWS = [[0, 5, 12, 5, 3], [12, 11, 10, 9, 8], [1, 2, 3, 4, 6]]  # a repeat, index 0 and index N - 1
ENCODER_CALLS = ("tspm_lstm", "tspm_conv", "tspm_textcnn", "tspm_seq_gather", "tspm_attn")
FIT_BOUND = 2 * (parity.FACTOR * 2.0 ** -24 + parity.FLOOR_OUT)
CASES = dict(tt.CASES)  # "attn-time" included: an attention encoder keeps its own length buffers without lengths


def _corpus(c, seed=21):
    cfg = tp._cfg(c["name"])
    return synthetic_mosi_corpus(N, seed=seed, steps=T0, min_len=1 if c.get("lengths") else None,
                                 feats=(cfg.audio_dim, cfg.video_dim, cfg.text_dim), regression=c.get("output_dim") == 1)


def _ds(gpu, c, corpus=None, split="train", sel=None):
    use_len = bool(c.get("lengths"))
    return MOSI(split=split, corpus=corpus or _corpus(c), device=gpu, seed=4, use_lengths=use_len, text_lengths=use_len,
                selected_patterns=sel, labels_key="regression_labels" if c.get("output_dim") == 1 else
                "classification_labels")


def _frozen(c, gpu):
    """(cfg, model with all three encoders frozen, its one-group FusedAdam)."""
    return tt._setup(c, gpu, frozen=ALL)


def _dense(corpus, rows):
    """The padded batch-first inputs of ``rows`` as the gather assembles them, their lengths and labels (CPU)."""
    out, lens = [], {}
    for m, tpad in zip(ALL, STEPS):
        x = torch.zeros(len(rows), tpad, corpus.feat[m])
        for i, r in enumerate(rows):
            o, n = int(corpus.offsets[m][r]), int(corpus.lengths[m][r])
            x[i, :n] = torch.from_numpy(corpus.data[m][o:o + n])
        out.append(x)
        lens[m] = [int(corpus.lengths[m][r]) for r in rows]
    return out[0], out[1], out[2], torch.from_numpy(corpus.labels[rows]), lens


def _group(c):
    return tr.Group("l1", tt.L1_WEIGHT) if c.get("output_dim") == 1 else None


def _log(gpu, c):
    return RegressionLog(gpu, groups=PATTERNS) if c.get("output_dim") == 1 else \
        ClassificationLog(gpu, groups=PATTERNS, classes=3)


def _record(monkeypatch):
    rec = tf._Recorder(L.lib())
    monkeypatch.setattr(L, "lib", lambda: rec)
    return rec


def _encoder_calls(calls):
    return [n for n in calls if n.startswith(ENCODER_CALLS)]


# ------------------------------------------------------------------------------------------------
# the cache's contents
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["mosi", "mosei", "lengths", "attn-time"])
def test_cache_rows_against_the_oracle_encoders(gpu, key):
    c = CASES[key]
    cfg, ours, _ = _frozen(c, gpu)
    state = {k: v.detach().clone() for k, v in ours.state_dict().items()}
    ds = _ds(gpu, c)
    cache = ds.embedding_cache(ours, pad_to=STEPS, chunk=5)  # chunks of 5, 5 and 3 rows
    use_len = bool(c.get("lengths"))
    assert cache.steps == M.norm_steps(STEPS) == ds.corpus_steps(STEPS) and cache.n == N and cache.fills == 1
    assert tuple(cache.emb.shape) == (N, HAV + NC) and tuple(cache.zero.shape) == (N if use_len else 1, HAV + NC)
    assert cache.n_zero == (N if use_len else 1) and cache.labels_all is ds.device_corpus.labels
    assert ds.embedding_cache(ours, pad_to=STEPS) is cache and cache.fill_seconds > 0
    o32, o64 = pair_from(ours, tp._oracle_builder(**tt._model_args(c)))
    A, V, T, _, lens = _dense(ds.corpus, list(range(N)))
    for tag, (a, v, t), got in (("emb", (A, V, T), cache.emb), ("zero", (A * 0, V * 0, T * 0), cache.zero)):
        if tag == "zero" and not use_len:
            a, v, t = a[:1], v[:1], t[:1]
        ref = []
        for o, dt in ((o32, torch.float32), (o64, torch.float64)):
            with torch.no_grad(), tp._oracle_mode(c.get("method"), lens if use_len else None):
                trace = orc.MosiTrace()
                orc.textcnn_forward(o.netT.eval(), t.to(dt), False, None, trace)
                pooled = torch.cat([F.relu(trace.pre[f"text.pool{i}"]).amax(2) for i in range(3)], 1)
                ref.append((orc.lstm_forward(o.netA, a.to(dt), None, "lstm.a.pool"),
                            orc.lstm_forward(o.netV, v.to(dt), None, "lstm.v.pool"), pooled))
        for j, (nm, cols) in enumerate((("eA", slice(0, WIDTHS[0])), ("eV", slice(WIDTHS[0], HAV)),
                                        ("pooled", slice(HAV, None)))):
            op_check(f"{key} {tag} {nm}", got[:, cols].cpu(), ref[0][j], ref[1][j])
    first = (cache.emb.clone(), cache.zero.clone())
    ptrs = (cache.emb.data_ptr(), cache.zero.data_ptr())
    assert cache.refresh() is cache and cache.fills == 2 and ptrs == (cache.emb.data_ptr(), cache.zero.data_ptr())
    assert torch.equal(cache.emb, first[0]) and torch.equal(cache.zero, first[1])  # a second fill is bitwise the first
    for k, v in ours.state_dict().items():  # the fill leaves every parameter and buffer untouched
        assert torch.equal(v, state[k]), k


# ------------------------------------------------------------------------------------------------
# bitwise against the uncached step with its encoder leg replaced
# ------------------------------------------------------------------------------------------------
def _stub(eng_half, labels_dst, cache, model, rows_buf, row_keep=None):
    """``_forward_encoders`` of an uncached engine (half) replaced: the cache's rows by torch indexing."""
    tp_ = float(model.netT.dropout.p)

    def fwd(sh, train):
        e = eng_half
        idx = rows_buf
        zidx = idx if cache.n_zero > 1 else torch.zeros_like(idx)
        real, zero = cache.emb[idx], cache.zero[zidx]
        if row_keep is None:  # rows [0, B) the batch, rows [B, 2B) its zero rows
            src = torch.cat([real, zero])
        else:
            k = row_keep != 0
            cols = torch.cat([k[:, 0:1].expand(-1, WIDTHS[0]), k[:, 1:2].expand(-1, WIDTHS[1]), k[:, 2:3].expand(-1, NC)], 1)
            src = torch.where(cols, real, zero)
        e.fused[:, :HAV].copy_(src[:, :HAV])
        pooled = src[:, HAV:]
        if train and tp_ > 0:
            # the kernel's expression v * (keep ? scale : 0) - torch.where(keep, v * scale, 0) but for the sign of a
            # dropped value's zero; the pooled values are ReLU outputs, so here the two agree on the bits too
            pooled = pooled * torch.where(e.keeps[0] != 0, 1.0 / (1.0 - tp_), 0.0)
        e.fc_in.copy_(pooled)
        labels_dst.copy_(cache.labels_all.reshape(-1)[idx])
        M._text_embed(e, model.netT, sh, e.fused.data_ptr() + HAV * 4, e.E)
    return fwd


def _state(model, opt, log, eng_keeps):
    out = {f"p.{n}": p.detach().clone() for n, p in model.named_parameters()}
    out.update({f"b.{n}": b.detach().clone() for n, b in model.named_buffers()})
    for n, p in model.named_parameters():
        if p.requires_grad and p in opt.state:
            out[f"m.{n}"], out[f"v.{n}"] = opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()
    out.update({f"keep{i}": k.clone() for i, k in enumerate(eng_keeps)})
    conf, losses, samples = log.fetch()
    if hasattr(log, "records"):  # a RegressionLog: the raw per-group accumulators
        out["log.records"] = log.records.detach().cpu().clone()
    else:
        out["log.conf"] = torch.as_tensor(np.asarray(conf, dtype=np.float64))
    out["losses"] = torch.as_tensor(np.asarray(losses))
    out["samples"] = torch.tensor(samples)
    return out


def _assert_same(a, b, tag):
    assert a.keys() == b.keys(), tag
    for k in a:
        assert torch.equal(a[k], b[k]), f"{tag}: {k}"


@pytest.mark.parametrize("key", list(CASES) + ["per-sample"])
def test_cached_train_step_is_bitwise_the_uncached_step_behind_the_encoders(gpu, key, monkeypatch):
    per = key == "per-sample"
    c = CASES["mosi" if per else key]
    pats = None if per else c.get("patterns", PATS)
    use_len = bool(c.get("lengths"))
    (cfg, twin, topt), (_, ours, opt) = _frozen(c, gpu), _frozen(c, gpu)
    enc0 = {f"{net}.{n}": p.detach().clone() for net in ("netA", "netV", "netT")
            for n, p in getattr(ours, net).named_parameters()}
    ds = _ds(gpu, c)
    tcache, cache = ds.embedding_cache(twin, pad_to=STEPS), ds.embedding_cache(ours, pad_to=STEPS)
    assert tcache is not cache and torch.equal(tcache.emb, cache.emb) and torch.equal(tcache.zero, cache.zero)
    group, tlog, log = _group(c), _log(gpu, c), _log(gpu, c)
    rows_buf = torch.zeros(B, dtype=torch.int64, device=gpu)
    rk_buf = torch.ones(B, 3, dtype=torch.uint8, device=gpu)
    st = M.FusedMosiCachedStep(ours, opt, group, B, cache, patterns=pats, per_sample=per)
    if per:
        tst = M.FusedMosiStep(twin, topt, group, B, STEPS)
        te = tst.eng
        te._forward_encoders = _stub(te, te.labels, tcache, twin, rows_buf, rk_buf)
        tkeeps, keeps = te.keeps, st.eng.keeps
        assert not hasattr(st.eng, "lstm") and not hasattr(st.eng, "conv_out") and not hasattr(st.eng, "A")
    else:
        tst = M.FusedMosiPatternStep(twin, topt, group, B, STEPS, patterns=pats, ragged=use_len, text_lengths=use_len)
        te = tst.eng
        te.enc._forward_encoders = _stub(te.enc, te.labels_f if group else te.labels, tcache, twin, rows_buf)
        tkeeps, keeps = [te.enc.keeps[0]] + te.cls.keeps[1:], [st.eng.enc.keeps[0]] + st.eng.cls.keeps[1:]
        e = st.eng.enc
        assert not any(hasattr(e, a) for a in ("lstm", "conv_out", "A", "V", "X", "pooled", "dfused"))
        assert tuple(e.fused.shape) == (2 * B, sum(WIDTHS)) and tuple(e.keeps[0].shape) == (2 * B, NC)
    st.log, tst.log = log, tlog
    # per-sample: pattern ids per row; the second batch has no row that keeps audio
    pid = [[0, 1, 2, 3, 4], [3, 5, 6, 3, 5], [6, 0, 4, 2, 1]]
    for s, rows in enumerate(ROWS):
        r = torch.tensor(rows, device=gpu)
        rows_buf.copy_(r)
        args = (r,)
        if per:
            flags = torch.tensor([[int(ch in PATTERNS[p]) for ch in "avt"] for p in pid[s]], dtype=torch.uint8, device=gpu)
            groups = torch.tensor(pid[s], dtype=torch.int32, device=gpu)
            assert s != 1 or not bool(flags[:, 0].any())
            rk_buf.copy_(flags)
            te.groups.copy_(groups)
            args = (r, flags, groups)
        tst.run()
        tout = {"loss": (te.loss if per else te.cls.loss).clone(), "logits": te.logits.clone()}
        rec = _record(monkeypatch) if s == 0 else None  # the launch record, on the eager step
        out = st.step(*args)
        if rec is not None:
            monkeypatch.undo()
            assert rec.calls.count("tspm_utt_cache_rows") == 1 and not _encoder_calls(rec.calls), rec.calls
            print(f"[{key}] cached train step: {len(rec.calls)} library calls: {rec.calls}")
        torch.cuda.synchronize()
        assert tuple(out["logits"].shape) == ((B, 3) if per else (len(pats), B, 1 if group else 3))
        assert torch.equal(out["logits"], tout["logits"]) and torch.equal(out["loss"], tout["loss"]), f"step {s}"
        _assert_same(_state(ours, opt, log, keeps), _state(twin, topt, tlog, tkeeps), f"{key} step {s}")
        if s == 1:
            assert st.graph is not None and tst.graph is not None  # captured on the second call
    assert st.calls == 3 and not torch.equal(keeps[0], torch.ones_like(keeps[0]))
    for net in ("netA", "netV", "netT"):  # the encoders are bitwise unchanged, and have no gradient
        for n, p in getattr(ours, net).named_parameters():
            assert torch.equal(p, enc0[f"{net}.{n}"]) and p.grad is None, n


# ------------------------------------------------------------------------------------------------
# one cached step against fp64 on the replicated real inputs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["mosi", "lengths"])
def test_cached_step_vs_fp64_on_the_real_inputs(gpu, key):
    c = CASES[key]
    use_len = bool(c.get("lengths"))
    cfg, ours, opt = _frozen(c, gpu)
    ds = _ds(gpu, c)
    cache = ds.embedding_cache(ours, pad_to=STEPS)
    rows = ROWS[0]
    A, V, T, y, lens = _dense(ds.corpus, rows)
    lens = lens if use_len else None
    # the encoders' decisions (time-max indices, ReLU masks) from a real eval-mode encoder pass over the same rows
    real = M.MosiPatternEngine(ours, B, STEPS, gpu, PATS, ragged=use_len, text_lengths=use_len)
    real.load(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
    real.set_lengths(tp._dev(lens, gpu))
    real.forward(L.stream_handle())
    forced = tt._decisions(real, PATS)
    o32, o64 = tt._oracles(ours, c, frozen=ALL)
    st = M.FusedMosiCachedStep(ours, opt, None, B, cache)
    keeps = tt._our_keeps(cfg, PATS, 50)
    st.keep_override = {k: v.to(gpu) for k, v in keeps.items()}
    out = st.step(torch.tensor(rows, device=gpu))
    torch.cuda.synchronize()
    e, cl = st.eng.enc, st.eng.cls
    forced["text.embd"] = (e.fused[:, HAV:] > 0).cpu()[tt._rows(PATS, "t")]
    for j, h in enumerate(cl.r if cl.use_bn else cl.h):
        forced[f"cls.relu{j}"] = (h > 0).cpu()
    assert torch.equal(cl.labels.cpu(), y.repeat(len(PATS)))
    tt._check(f"cached {key}", ours, forced, out["logits"], out["loss"], o32, o64, tt._replicate(A, V, T, y, PATS, lens),
              tt._oracle_keeps(keeps, PATS))


# ------------------------------------------------------------------------------------------------
# eval
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", [False, True])
def test_cached_eval_step_is_bitwise_the_uncached_one_behind_the_encoders(gpu, per, monkeypatch):
    c = CASES["mosei"]
    _, ours, _ = _frozen(c, gpu)
    ds = _ds(gpu, c, split="valid")
    cache = ds.embedding_cache(ours, pad_to=STEPS)
    tlog, log = _log(gpu, c), _log(gpu, c)
    rows_buf = torch.zeros(B, dtype=torch.int64, device=gpu)
    rk_buf = torch.ones(B, 3, dtype=torch.uint8, device=gpu)
    st = M.FusedMosiCachedEvalStep(ours, None, B, cache, log, per_sample=per)
    if per:
        tst = M.FusedMosiEvalStep(ours, None, B, STEPS, tlog)
        te = tst.eng
        te._forward_encoders = _stub(te, te.labels, cache, ours, rows_buf, rk_buf)
    else:
        tst = M.FusedMosiPatternEvalStep(ours, None, B, STEPS, tlog)
        te = tst.eng
        te.enc._forward_encoders = _stub(te.enc, te.labels, cache, ours, rows_buf)
    try:
        for s, rows in enumerate(ROWS):
            r = torch.tensor(rows, device=gpu)
            rows_buf.copy_(r)
            args = (r,)
            if per:
                p = PATTERNS[(2 * s + 1) % 7]  # a grouped valid batch: one pattern for all rows
                flags = torch.tensor([[int(ch in p) for ch in "avt"]] * B, dtype=torch.uint8, device=gpu)
                groups = log.group_ids([p] * B)
                rk_buf.copy_(flags)
                te.groups.copy_(groups)
                args = (r, flags, groups)
            tst.run()
            want = te.logits.clone()
            rec = _record(monkeypatch) if s == 0 else None
            out = st.step(*args)
            if rec is not None:
                monkeypatch.undo()
                assert rec.calls.count("tspm_utt_cache_rows") == 1 and not _encoder_calls(rec.calls), rec.calls
            torch.cuda.synchronize()
            assert torch.equal(out["logits"], want) and torch.equal(out["loss"], te.loss if per else te.losses)
        a, b = log.fetch(), tlog.fetch()
        assert np.array_equal(a[0], b[0]) and a[1].tolist() == b[1].tolist() and a[2] == b[2]
        assert len(a[1]) == (3 if per else 3 * 7) and st.graph is not None and ours.training is False
    finally:
        ours._engines = {}  # the stubbed engines live in the model's table


# ------------------------------------------------------------------------------------------------
# the ids_only loader, the runner and fit
# ------------------------------------------------------------------------------------------------
def test_ids_only_loader_matches_the_tensor_loader(gpu):
    """Same order, pattern draws, ``len`` and batch keys under the same seeds, in all four loader forms."""
    c = CASES["mosi"]
    corpus = _corpus(c)
    dense = torch.from_numpy(corpus.data["audio"]).reshape(N, T0, -1)

    def rows_of(b):  # the sample of every row of a tensor batch, found by its content
        a = b["audio"][:, :T0].cpu()
        nz = a.flatten(1).any(1)
        return [int(np.flatnonzero((dense == a[i]).flatten(1).all(1))[0]) if nz[i] else -1 for i in range(a.shape[0])]

    forms = [("train", dict(shuffle=True, seed=7)), ("train", dict(shuffle=True, seed=7, all_patterns=True)),
             ("valid", dict()), ("valid", dict(fuse_patterns=True))]
    for split, kw in forms:
        full, ids = _ds(gpu, c, corpus, split), _ds(gpu, c, corpus, split)
        lf, li = full.loader(B, pad_to=STEPS, **kw), ids.loader(B, pad_to=STEPS, ids_only=True, **kw)
        assert len(lf) == len(li) and li.ids_only and not lf.ids_only
        for epoch in range(2):
            bf, bi = list(lf), list(li)
            assert len(bf) == len(bi) == len(lf)
            for x, y in zip(bf, bi):
                groups = [(None, x, y)] if "label" in x else [(p, x[p], y[p]) for p in x]
                assert "label" in x or list(x) == list(y)
                for p, gx, gy in groups:
                    assert gy["ids_only"] is True and gy["steps"] == M.norm_steps(STEPS) == gx["steps"]
                    assert gy["rows"].dtype == torch.int64 and gy["rows"].device.type == "cuda"
                    assert not any(k in gy for k in ("audio", "video", "text", "label"))
                    r = gy["rows"].cpu().tolist()
                    assert len(r) == gx["label"].numel()
                    assert torch.equal(gx["label"].cpu(), torch.from_numpy(corpus.labels[r]))
                    if kw.get("all_patterns") or kw.get("fuse_patterns"):
                        flag = "all_patterns" if kw.get("all_patterns") else "fused_patterns"
                        assert gy[flag] is True and gy["patterns"] == gx["patterns"] and "row_keep" not in gy
                        assert rows_of(gx) == r
                    else:
                        assert gy["pattern_name"] == gx["pattern_name"]
                        assert gy["row_keep"].cpu().tolist() == [[int(ch in q) for ch in "avt"] for q in gy["pattern_name"]]
                        assert [a for a, q in zip(rows_of(gx), gx["pattern_name"]) if "a" in q] == \
                            [a for a, q in zip(r, gy["pattern_name"]) if "a" in q]
    mono = MOSI(split="train", corpus=corpus, device=gpu, target_modality="audio")
    with pytest.raises(tspm_amd.TspmError, match="multimodal target"):
        mono.loader(B, ids_only=True)


def _fit(gpu, cached, forms, monkeypatch, tmp_path):
    c = CASES["mosi"]
    _, ours, opt = _frozen(c, gpu)
    corpus, vcorpus = _corpus(c), _corpus(c, seed=22)
    tr_ds, va = _ds(gpu, c, corpus), _ds(gpu, c, vcorpus, "valid")
    kw_t, kw_v = (dict(all_patterns=True), dict(fuse_patterns=True)) if forms == "fused" else ({}, {})
    loaders = {"train": tr_ds.loader(B, shuffle=True, seed=3, pad_to=STEPS, **kw_t),
               "validation": va.loader(B, pad_to=STEPS, **kw_v), "test": va.loader(B, pad_to=STEPS, **kw_v)}
    if cached:  # filled beforehand: no encoder call may then appear in the record
        tr_ds.embedding_cache(ours, pad_to=STEPS), va.embedding_cache(ours, pad_to=STEPS)
    rec = _record(monkeypatch)
    hist = harness.fit(ours, opt, None, loaders, epochs=2, early_stopping=False, cache_embeddings=cached,
                       checkpoint_dir=tmp_path / f"ck{int(cached)}")
    monkeypatch.undo()
    return hist, rec.calls, (tr_ds, va, ours)


@pytest.mark.parametrize("forms", ["fused", "plain"])
def test_fit_on_the_cache_matches_the_uncached_run(gpu, forms, monkeypatch, tmp_path):
    plain, pcalls, _ = _fit(gpu, False, forms, monkeypatch, tmp_path)
    hist, calls, (tr_ds, va, ours) = _fit(gpu, True, forms, monkeypatch, tmp_path)
    # the only encoder work of the cached run is the ONE refill for the test split, after the last optimizer launch
    # (the best checkpoint was reloaded): one chunk, hence one gather per modality
    at = [i for i, n in enumerate(calls) if n.startswith(ENCODER_CALLS)]
    assert _encoder_calls(pcalls) and at and min(at) > max(i for i, n in enumerate(calls) if "adam" in n)
    assert calls.count("tspm_seq_gather") == 3 and calls.count("tspm_utt_cache_rows") > 0
    assert "embedding_cache" not in plain
    assert set(hist["embedding_cache"]["rows"]) == {"train", "validation", "test"}
    assert hist["embedding_cache"]["rows"]["train"] == N
    # the best checkpoint was reloaded for the test split and the test cache refreshed
    assert va.embedding_cache(ours, pad_to=STEPS).fills == 2 and tr_ds.embedding_cache(ours, pad_to=STEPS).fills == 1
    for split in ("train", "validation"):
        for e in range(2):
            a, b = hist[split][e], plain[split][e]
            assert list(a) == list(b)  # the same metric keys
            ta, tb = hist["epoch_metrics"][e][split]["timing"], plain["epoch_metrics"][e][split]["timing"]
            na, nb = round(ta["total_time"] / ta["avg_batch_time"]), round(tb["total_time"] / tb["avg_batch_time"])
            assert na == nb, "the number of loss entries per epoch"
            for k in a:
                if isinstance(a[k], (int, float)):
                    print(f"[{forms}] {split} epoch {e + 1} {k}: cached {a[k]!r} uncached {b[k]!r}")
                    both_nan = a[k] != a[k] and b[k] != b[k]  # a score of a pattern without rows of that kind
                    assert both_nan or abs(a[k] - b[k]) <= FIT_BOUND * max(abs(a[k]), abs(b[k]), 1e-30), (split, e, k)
    assert list(hist["test"]) == list(plain["test"])
    assert abs(hist["test"]["loss"] - plain["test"]["loss"]) <= FIT_BOUND * abs(plain["test"]["loss"])


# ------------------------------------------------------------------------------------------------
# refusals and staleness
# ------------------------------------------------------------------------------------------------
def test_refusals_and_staleness(gpu):
    c = CASES["mosi"]
    cfg, ours, opt = _frozen(c, gpu)
    ds = _ds(gpu, c)
    cache = ds.embedding_cache(ours, pad_to=STEPS)
    rows = torch.tensor(ROWS[0], device=gpu)
    # a trainable encoder
    _, free, fopt = tt._setup(c, gpu)
    with pytest.raises(tspm_amd.TspmError, match="frozen encoders"):
        ds.embedding_cache(free, pad_to=STEPS)
    with pytest.raises(tspm_amd.TspmError, match="frozen encoders"):
        M.FusedMosiCachedStep(free, fopt, None, B, cache)
    loaders = {"train": ds.loader(B, pad_to=STEPS), "validation": ds.loader(B, pad_to=STEPS)}
    with pytest.raises(tspm_amd.TspmError, match="frozen encoders"):
        harness.fit(free, fopt, None, loaders, epochs=1, cache_embeddings=True)
    with pytest.raises(tspm_amd.TspmError, match="not built"):
        harness.fit(ours, opt, None, loaders, epochs=1, cache_embeddings=True, steps_per_call=2)
    # the optimizer
    with pytest.raises(tspm_amd.TspmError, match="FusedAdam"):
        M.FusedMosiCachedStep(ours, torch.optim.Adam(ours.netC.parameters()), None, B, cache)
    m2 = tp._ours("mosi").to(gpu)
    M.finetune_param_groups(m2, lr=1e-3, weight_decay=0.0, freeze=ALL)
    lins = list(m2.netC.parameters())
    two = tspm_amd.FusedAdam([dict(params=lins[:2], lr=1e-3), dict(params=lins[2:], lr=1e-4)])
    with pytest.raises(tspm_amd.TspmError, match="one FusedAdam parameter group"):
        M.FusedMosiCachedStep(m2, two, None, B, cache)
    with pytest.raises(tspm_amd.TspmError, match="allreduce"):
        M.FusedMosiCachedStep(ours, opt, None, B, cache, allreduce=lambda: None)
    # another model's cache; the wrong labels for the head
    _, other, oopt = _frozen(c, gpu)
    with pytest.raises(tspm_amd.TspmError, match="another model"):
        M.FusedMosiCachedStep(other, oopt, None, B, cache)
    reg = dict(c, output_dim=1)
    _, rmodel, ropt = _frozen(reg, gpu)
    with pytest.raises(tspm_amd.TspmError, match="float32 labels"):
        M.FusedMosiCachedStep(rmodel, ropt, _group(reg), B, ds.embedding_cache(rmodel, pad_to=STEPS))
    # another steps value is another cache
    assert ds.embedding_cache(ours, pad_to=(8, 9, 6)) is not cache
    assert ds.embedding_cache(ours, pad_to=(8, 9, 6)).steps == (8, 9, 6)
    st = M.FusedMosiCachedStep(ours, opt, None, B, cache)
    ev = M.FusedMosiCachedEvalStep(ours, None, B, cache, _log(gpu, c))
    st.step(rows)
    with pytest.raises(tspm_amd.TspmError, match="per_sample=True"):
        st.step(rows, torch.ones(B, 3, dtype=torch.uint8, device=gpu), torch.zeros(B, dtype=torch.int32, device=gpu))
    with pytest.raises(tspm_amd.TspmError, match="sample indices"):
        st.step(rows[:3])
    sd = {k: v.clone() for k, v in ours.state_dict().items()}

    def stale(step=st):
        with pytest.raises(tspm_amd.TspmError, match=r"stale UttEmbeddingCache.*refresh\(\)"):
            step.step(rows)
        assert cache.stale_reason() is not None
        cache.refresh()
        assert cache.stale_reason() is None

    ours.load_state_dict(sd)
    stale()
    st.step(rows)  # refresh() restores use
    ours.netV.load_state_dict(ours.netV.state_dict())
    stale(ev)
    ev.step(rows)
    ours.netT.requires_grad_(True)
    with pytest.raises(tspm_amd.TspmError, match="stale UttEmbeddingCache"):
        cache.check(ours)
    with pytest.raises(tspm_amd.TspmError, match="frozen encoders"):
        cache.refresh()
    ours.netT.requires_grad_(False)
    cache.check(ours)  # the flags are what they were at the fill
    ours.to(gpu)  # drops the engines
    with pytest.raises(tspm_amd.TspmError, match="stale UttEmbeddingCache"):
        cache.check(ours)
    cache.refresh().check(ours)


# ------------------------------------------------------------------------------------------------
# the existing steps are what they were
# ------------------------------------------------------------------------------------------------
def _existing(gpu):
    c = CASES["mosei"]
    cfg, ours, opt = _frozen(c, gpu)
    A, V, T, y = tp._batch("mosei", 0)
    out = M.FusedMosiStep(ours, opt, None, B, STEPS).step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
    res = [out["logits"].clone(), out["loss"].clone()] + [p.detach().clone() for p in ours.parameters()]
    log = _log(gpu, c)
    ev = M.FusedMosiPatternEvalStep(ours, None, B, STEPS, log)
    ev.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
    return res + [ev.eng.logits.clone(), ev.eng.losses.clone(), torch.as_tensor(log.fetch()[0].astype(np.float64))]


def test_existing_steps_are_bitwise_what_they_were_before_the_cached_paths_ran(gpu):
    before = _existing(gpu)
    c = CASES["mosei"]
    _, ours, opt = _frozen(c, gpu)
    ds = _ds(gpu, c)
    cache = ds.embedding_cache(ours, pad_to=STEPS)
    rows = torch.tensor(ROWS[0], device=gpu)
    for _ in range(3):
        M.FusedMosiCachedStep(ours, opt, None, B, cache).step(rows)
    M.FusedMosiCachedEvalStep(ours, None, B, cache, _log(gpu, c)).step(rows)
    after = _existing(gpu)
    assert len(before) == len(after)
    for a, b in zip(before, after):
        assert torch.equal(a, b)
