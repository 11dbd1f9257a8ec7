"""The AVMNIST head stage on the device: ``AVMNIST.freeze_encoders`` + ``step.FusedHeadStageStep`` (one random pattern per
sample) and ``step.FusedHeadStagePatternStep`` (every pattern of the batch, both heads), at B = 4 and B = 1 with the
default encoders.  The fp64 truth is tests/head_stage_ref.py's chain on the REPLICATED rows, fed with the device's own
embeddings, zero-input row and dropout mask: the encoders are frozen, so everything the step trains is the head."""
import json

import numpy as np
import pytest
import torch

import head_stage_ref as R
import parity
from oracle import avmnist_ref as orc
from tspm_amd import _lib as L

pytestmark = pytest.mark.gpu

ALL = ("a", "ai", "i")
LR, WD = 5e-4, 1e-4
HEAD = ("net.0.weight", "net.0.bias", "net.3.weight", "net.3.bias", "net.5.weight", "net.5.bias")
REF_KEY = dict(zip(HEAD, ("w0", "b0", "w3", "b3", "w5", "b5")))


class _Recorder:
    """``L.lib()`` with every tspm_* call noted by name (the step's launch record, taken on an eager step)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("tspm_"):
            return fn

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call


def _running_stats(model):
    """Non-trivial running statistics (a pre-trained encoder's are not 0 / 1)."""
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            gg = torch.Generator().manual_seed(m.num_features)
            rm, rv = torch.randn(m.num_features, generator=gg) * 0.1, torch.rand(m.num_features, generator=gg) + 0.5
            with torch.no_grad():
                m.running_mean.copy_(rm)
                m.running_var.copy_(rv)


def _model(dev, frozen=True, dropout=0.5):
    import tspm_amd
    torch.manual_seed(0)
    m = tspm_amd.AVMNIST(tspm_amd.ResNet18(1, 64), tspm_amd.ResNet34(1, 128), 128, dropout=dropout).to(dev)
    _running_stats(m)
    return m.freeze_encoders() if frozen else m


def _opt(model):
    import tspm_amd
    return tspm_amd.FusedAdam(model.parameters(), lr=LR, weight_decay=WD)


def _batch(B, seed, dev, masked):
    """A synthetic batch on the device; ``masked``: one random pattern per sample applied to the inputs, as the train
    loader does (group ids in ("a", "ai", "i") order)."""
    audio, image, labels, _ = orc.synthetic_batch(B, seed=seed)
    gid = torch.zeros(B, dtype=torch.int32)
    if masked:
        gid = torch.randint(0, 3, (B,), generator=torch.Generator().manual_seed(seed)).to(torch.int32)
        ka = torch.tensor([R.KEEP[ALL[g]][0] for g in gid.tolist()], dtype=torch.float32)
        ki = torch.tensor([R.KEEP[ALL[g]][1] for g in gid.tolist()], dtype=torch.float32)
        audio, image = audio * ka.view(B, 1, 1), image * ki.view(B, 1, 1, 1)
    return audio.to(dev), image.to(dev), labels.to(dev), gid.to(dev)


def _encoder_state(model):
    out = {}
    for name in ("audio_encoder", "image_encoder"):
        enc = getattr(model, name)
        out.update({f"{name}.{n}": t.detach().clone() for n, t in list(enc.named_parameters()) + list(enc.named_buffers())})
    return out


def _assert_encoders_untouched(model, before):
    now = _encoder_state(model)
    assert set(now) == set(before) and any(k.endswith("num_batches_tracked") for k in now)
    for k, t in now.items():
        assert torch.equal(t, before[k]), k
    for name in ("audio_encoder", "image_encoder"):
        assert all(p.grad is None and not p.requires_grad for p in getattr(model, name).parameters())


def _build(kind, model, opt, B, use_graph, log=None):
    from tspm_amd.step import FusedHeadStagePatternStep, FusedHeadStageStep
    if kind == "plain":
        st = FusedHeadStageStep(model, opt, None, B, use_graph=use_graph)
        st.log = log
        return st
    st = FusedHeadStagePatternStep(model, opt, None, B, head=kind, log=log, use_graph=use_graph)
    assert st.head == kind and st.patterns == ALL
    return st


def _snap(model, opt):
    ps = dict(model.named_parameters())
    return ({n: ps[n].detach().cpu().double().clone() for n in HEAD},
            {n: opt.state[ps[n]]["exp_avg"].detach().cpu().double().clone() for n in HEAD},
            {n: opt.state[ps[n]]["exp_avg_sq"].detach().cpu().double().clone() for n in HEAD})


def _check_step(kind, model, opt, st, labels, before, step, ratios):
    """The step just run against fp64: the reference chain on the device's own embeddings / zero row / keep mask with the
    head's parameters from before the step; logits, loss and the six gradients under parity.op_check (fp32 CPU run of the
    same chain as the yardstick); the parameters against parity.adam_fp64 — fed with OUR gradient within
    parity.adam_tolerance (the optimizer exactly), and fed with the fp64 gradient within that tolerance plus the
    first-order effect of the two gradients' difference on the update (twice the first-moment term: the second moment's
    term is of the same size at most), the gradient's own error being bounded by the op_check above."""
    pb, mb, vb = before
    W = {REF_KEY[n]: pb[n].float() for n in HEAD}
    x = st.fused.detach().cpu()
    B = x.shape[0]
    p = float(model.dropout_p)
    if kind == "plain":
        keep, x0 = ((1, 1),), torch.zeros(x.shape[1])
    else:
        keep, x0 = R.keep_of(st.patterns), st.x0.detach().cpu()
    mask = st.keep.detach().cpu() if p > 0 else None
    r64 = R.chain(x, x0, keep, st.ea, W, labels.cpu(), 1.0, p, mask, torch.float64)
    r32 = R.chain(x, x0, keep, st.ea, W, labels.cpu(), 1.0, p, mask, torch.float32)
    tag = f"[{kind},B={B},step {step}]"
    parity.op_check("logits" + tag, st.logits.reshape(-1, 10), r32["logits"], r64["logits"], ratios=ratios)
    parity.op_check("loss" + tag, st.loss, r32["loss"], r64["loss"], ratios=ratios)
    ps = dict(model.named_parameters())
    b1, b2, eps = 0.9, 0.999, 1e-8
    for n in HEAD:
        g_ours = ps[n].grad.detach().cpu().double()
        g64 = r64["g" + REF_KEY[n]]
        parity.op_check(f"grad {n}" + tag, g_ours, r32["g" + REF_KEY[n]], g64, grad=True, ratios=ratios)
        got = ps[n].detach().cpu().double()
        m0, v0 = (None, None) if step == 1 else (mb[n], vb[n])
        exp, _, v = parity.adam_fp64(pb[n], g_ours, step, lr=LR, wd=WD, m=m0, v=v0)
        tol = 1e-6 * exp.abs() + parity.adam_tolerance(pb[n], g_ours, step, v, LR, WD)
        assert bool(((got - exp).abs() <= tol).all()), (n, step, "Adam on our gradient")
        exp64, _, v64 = parity.adam_fp64(pb[n], g64, step, lr=LR, wd=WD, m=m0, v=v0)
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        denom = torch.minimum(v, v64).sqrt() / bc2 ** 0.5 + eps
        tol64 = 1e-6 * exp64.abs() + parity.adam_tolerance(pb[n], g64, step, v64, LR, WD) + \
            2 * LR / bc1 * (1 - b1) * (g_ours - g64).abs() / denom
        assert bool(((got - exp64).abs() <= tol64).all()), (n, step, "Adam on the fp64 gradient")


@pytest.mark.parametrize("B", [4, 1])
@pytest.mark.parametrize("kind", ["plain", "kernel", "launches"])
def test_three_steps_on_one_graph_vs_fp64_and_eager(gpu, monkeypatch, kind, B):
    from tspm_amd.metrics import ClassificationLog
    # the eager twin: the same model, optimizer and batches, every step enqueued eagerly, the first with a launch record
    twin, model = _model(gpu), _model(gpu)
    topt, opt = _opt(twin), _opt(model)
    assert [id(p) for p in opt.flat_groups()[0].params] == [id(p) for p in model.net.parameters()]
    enc0 = _encoder_state(model)
    tlog, log = ClassificationLog(gpu), ClassificationLog(gpu)
    tst, st = _build(kind, twin, topt, B, False, tlog), _build(kind, model, opt, B, True, log)
    ratios = parity.Ratios()
    P = 1 if kind == "plain" else 3
    for k in range(3):  # eager, capture, replay: three different batches
        a, i, lab, gid = _batch(B, 300 + k, gpu, masked=(kind == "plain"))
        args = (a, i, lab, gid) if kind == "plain" else (a, i, lab)
        if k == 0:
            rec = _Recorder(L.lib())
            monkeypatch.setattr(L, "lib", lambda: rec)
        tout = {kk: v.clone() for kk, v in tst.step(*args).items()}
        if k == 0:
            monkeypatch.undo()
            calls = rec.calls
            assert not [c for c in calls if c.startswith("tspm_conv_bwd") or c.startswith("tspm_bn_bwd")], calls
            assert any(c.startswith("tspm_conv_fwd") or c.startswith("tspm_stem") for c in calls)  # the encoders did run
            want_head = {"plain": "tspm_head_train_step", "kernel": "tspm_pattern_head_train_step",
                         "launches": "tspm_head_train_step"}[kind]
            assert calls.count(want_head) == 1 and calls.count("tspm_classify_update") == 1
            assert ("tspm_pattern_expand" in calls) == (kind == "launches")
            assert [c for c in calls if "adam" in c] == ["tspm_adam_step"]  # the head launch advanced the step counter
            assert "tspm_counters_add" not in calls                          # no num_batches_tracked bump
        before = _snap(model, opt)
        out = st.step(*args)
        assert out["logits"].shape == ((B, 10) if kind == "plain" else (3, B, 10)) and out["loss"].shape == (1,)
        # replay (k = 2) and capture (k = 1) are bitwise the eager twin's
        assert torch.equal(out["logits"], tout["logits"]) and torch.equal(out["loss"], tout["loss"]), k
        for (n, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
            assert torch.equal(p, q), (k, n)
        assert torch.equal(st.keep, tst.keep) and 0.3 < st.keep.float().mean().item() < 0.7
        _check_step(kind, model, opt, st, lab, before, k + 1, ratios)
        _assert_encoders_untouched(model, enc0)
    print("worst ratios:", ratios)
    assert st.graph is not None and tst.graph is None and st.calls == 3
    assert int(opt.flat_groups()[0].hyper.view(torch.int64)[6]) == 3      # one Adam step count per step
    # the log: ONE loss entry per step (the P*B-row mean), every row under its pattern's group
    conf, ll, rows = log.fetch()
    tconf, tll, _ = tlog.fetch()
    assert len(ll) == 3 and rows == 3 * P * B and conf.sum() == rows and np.array_equal(conf, tconf)
    assert ll.tolist() == tll.tolist()
    if kind != "plain":
        assert [int(c.sum()) for c in conf] == [3 * B] * 3
    assert model.training and model.net.training and not model.audio_encoder.training


def test_refusals_on_the_device_and_training_again(gpu):
    import tspm_amd
    from tspm_amd.harness import AVMNIST_METRICS
    from tspm_amd.metrics import ClassificationLog, DeviceMetricRecorder
    rec = DeviceMetricRecorder(AVMNIST_METRICS, ClassificationLog(gpu))
    a, i, lab, gid = _batch(4, 11, gpu, masked=True)
    batch = {"audio": a, "image": i, "labels": lab, "pattern_ids": gid}
    allb = {"audio": a, "image": i, "labels": lab, "patterns": list(ALL), "all_patterns": True}
    # an all_patterns batch on an unfrozen model: refused, and the message says why
    model = _model(gpu, frozen=False)
    opt = _opt(model)                                   # built BEFORE freezing
    with pytest.raises(L.TspmError, match="BatchNorm on batch statistics"):
        model.train_step(allb, opt, None, gpu, rec)
    # exactly one encoder frozen
    for p in model.image_encoder.parameters():
        p.requires_grad_(False)
    with pytest.raises(L.TspmError, match="exactly one encoder is frozen"):
        model.train_step(batch, opt, None, gpu, rec)
    for p in model.image_encoder.parameters():
        p.requires_grad_(True)
    # the optimizer built before freeze_encoders()
    model.freeze_encoders()
    for b in (batch, allb):
        with pytest.raises(L.TspmError, match="built before freeze_encoders"):
            model.train_step(b, opt, None, gpu, rec)
    with pytest.raises(L.TspmError, match="built before freeze_encoders"):
        tspm_amd.harness.EpochRunner(model, opt, None)._train_step(4)
    # ... and, with a rebuilt one, training again: both kinds of batch, through train_step
    enc0 = _encoder_state(model)
    opt = _opt(model)
    head0 = [p.detach().clone() for p in model.net.parameters()]
    r1 = model.train_step(batch, opt, None, gpu, rec)
    assert type(model._fused_step).__name__ == "FusedHeadStageStep"
    r2 = model.train_step(allb, opt, None, gpu, rec)
    assert np.isfinite(r1["loss"]) and np.isfinite(r2["loss"])
    assert all(not torch.equal(p, q) for p, q in zip(model.net.parameters(), head0))
    _assert_encoders_untouched(model, enc0)
    conf, ll, rows = rec.log.fetch()
    assert len(ll) == 2 and rows == 4 + 12
    # unfreezing leaves the head-stage step behind: the optimizer does not hold the encoders
    model.unfreeze_encoders()
    with pytest.raises(L.TspmError, match="is trainable but not in the FusedAdam's flat buffers|not frozen"):
        tspm_amd.step.FusedHeadStageStep(model, opt, None, 4)


def test_autograd_branch_on_a_frozen_model(gpu):
    """A loss group / optimizer the fused step does not take keeps going to the autograd path, which works on a frozen
    model: frozen parameters get ``grad is None`` and the encoders run on their running statistics."""
    model = _model(gpu)
    enc0 = _encoder_state(model)
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=LR)

    def loss_functions(logits, labels):
        return {"total_loss": torch.nn.functional.cross_entropy(logits, labels)}
    a, i, lab, _ = _batch(4, 21, gpu, masked=True)
    head0 = [p.detach().clone() for p in model.net.parameters()]
    r = model.train_step({"audio": a, "image": i, "labels": lab, "pattern_name": ["ai"] * 4}, opt, loss_functions, gpu, None)
    assert np.isfinite(r["loss"]) and model._fused_step is None
    assert all(p.grad is not None and not torch.equal(p, q) for p, q in zip(model.net.parameters(), head0))
    _assert_encoders_untouched(model, enc0)
    # the autograd gradients of the head are those of the fp64 chain on the same embeddings (no dropout mask: p = 0)
    m0 = _model(gpu, dropout=0.0)
    opt0 = torch.optim.SGD([p for p in m0.parameters() if p.requires_grad], lr=0.0)
    W = {REF_KEY[n]: p.detach().cpu() for n, p in m0.named_parameters() if n in HEAD}
    m0.train_step({"audio": a, "image": i, "labels": lab}, opt0, loss_functions, gpu, None)
    with torch.no_grad():
        m0.eval()
        x = torch.cat([m0.audio_encoder(a), m0.image_encoder(i)], 1).cpu()
    r64 = R.chain(x, torch.zeros(192), ((1, 1),), 64, W, lab.cpu(), dtype=torch.float64)
    r32 = R.chain(x, torch.zeros(192), ((1, 1),), 64, W, lab.cpu(), dtype=torch.float32)
    for n, p in m0.named_parameters():
        if n in HEAD:
            parity.op_check(f"autograd {n}", p.grad, r32["g" + REF_KEY[n]], r64["g" + REF_KEY[n]], grad=True)


def _datasets(gpu, n_train=40, n_val=24):
    from tspm_amd.data import AVMNIST, synthetic_corpus
    tr = AVMNIST(None, "train", "multimodal", corpus=synthetic_corpus(n_train, 5), device=gpu)
    va = AVMNIST(None, "valid", "multimodal", corpus=synthetic_corpus(n_val, 6), device=gpu)
    return tr, va


def test_fit_one_epoch_with_all_pattern_and_fused_loaders(gpu, tmp_path):
    from tspm_amd.harness import CheckpointManager, EpochRunner, fit
    from tspm_amd.step import FusedHeadStagePatternStep, FusedHeadStageStep

    def run(all_patterns, sub):
        model = _model(gpu)
        enc0 = _encoder_state(model)
        opt = _opt(model)
        tr, va = _datasets(gpu)
        g = torch.Generator().manual_seed(3)
        loaders = {"train": tr.device_loader(16, shuffle=True, generator=g, all_patterns=all_patterns),
                   "validation": va.device_loader(16, fuse_patterns=True), "test": va.device_loader(16, fuse_patterns=True)}
        h = fit(model, opt, None, loaders, epochs=1, metrics_path=tmp_path / sub, checkpoint_dir=tmp_path / sub / "ck")
        _assert_encoders_untouched(model, enc0)       # through the train epoch, the validation and the best.pth reload
        em = json.load(open(tmp_path / sub / "epoch_metrics.json"))

        def walk(d, pre=""):
            return {pre + k for k in d} | {x for k, v in d.items() if isinstance(v, dict) for x in walk(v, pre + k + ".")}
        assert np.isfinite(h["train"][0]["loss"]) and np.isfinite(h["test"]["loss"])
        return model, opt, (walk(em[0]), set(h["test"]), set(h["validation"][0]), set(h["train"][0])), tmp_path / sub / "ck"

    model, opt, keys_all, ck = run(True, "all")
    _, _, keys_plain, _ = run(False, "plain")
    assert keys_all == keys_plain and "accuracy_AI" in keys_all[3] and "train.AI.f1_macro" in keys_all[0]
    # best.pth reloads on the frozen model and leaves it frozen
    head = [p.detach().clone() for p in model.net.parameters()]
    with torch.no_grad():
        model.net[5].bias.add_(1.0)
    CheckpointManager(ck).load_checkpoint(model, load_best=True)
    assert all(torch.equal(p, q) for p, q in zip(model.net.parameters(), head))
    assert model.frozen_encoders() and not any(p.requires_grad for p in model.audio_encoder.parameters())
    # the runner's steps: keyed with the trailing ("frozen", names); the zero embeddings refreshed on the epoch's first
    # all-pattern batch only
    runner = EpochRunner(model, opt, None)
    tr, _ = _datasets(gpu)
    refreshes = []
    orig = FusedHeadStagePatternStep.run
    try:
        FusedHeadStagePatternStep.run = lambda self, refresh_zero=False: (refreshes.append(refresh_zero), orig(self, refresh_zero))[1]
        loss, _, metrics, n = runner.train_epoch(tr.device_loader(16, all_patterns=True))
    finally:
        FusedHeadStagePatternStep.run = orig
    fr = ("frozen", ("audio_encoder", "image_encoder"))
    assert n == 3 and refreshes == [True, False, False] and np.isfinite(loss)
    assert set(runner.train_steps) == {(("patterns", ALL), 16, fr), (("patterns", ALL), 8, fr)}
    conf, ll, rows = runner.log.fetch()
    assert rows == 3 * 40 and [int(c.sum()) for c in conf] == [40, 40, 40] and len(ll) == 3
    runner.train_epoch(tr.device_loader(16))
    assert {(16, fr), (8, fr)} <= set(runner.train_steps)
    assert isinstance(runner.train_steps[(16, fr)], FusedHeadStageStep)


def test_unfrozen_step_is_bitwise_what_it_was_before_the_new_paths_ran(gpu):
    """FusedTrainStep on an all-trainable model: the same launches, keys and bits whether or not the head-stage code
    ran in the process (and the runner's key for it is still the batch size)."""
    import tspm_amd
    from tspm_amd.harness import EpochRunner

    def two_steps():
        model = _model(gpu, frozen=False)
        opt = _opt(model)
        st = tspm_amd.FusedTrainStep(model, opt, None, 4)
        assert st._sig == (id(opt), id(None), 4)          # no ("frozen", ...) element for an all-trainable model
        outs = []
        for k in range(2):
            a, i, lab, gid = _batch(4, 400 + k, gpu, masked=True)
            out = st.step(a, i, lab, gid)
            outs += [out["logits"].clone(), out["loss"].clone()]
        runner = EpochRunner(model, opt, None)
        assert runner._train_step(4).__class__ is tspm_amd.FusedTrainStep and set(runner.train_steps) == {4}
        return outs + [p.detach().clone() for p in model.parameters()] + [b.detach().clone() for b in model.buffers()]

    first = two_steps()
    # the new code paths, on another model
    frozen = _model(gpu)
    fopt = _opt(frozen)
    a, i, lab, gid = _batch(4, 500, gpu, masked=True)
    tspm_amd.FusedHeadStageStep(frozen, fopt, None, 4).step(a, i, lab, gid)
    for head in ("kernel", "launches"):
        tspm_amd.FusedHeadStagePatternStep(frozen, fopt, None, 4, head=head).step(a, i, lab)
    second = two_steps()
    assert len(first) == len(second) and all(torch.equal(x, y) for x, y in zip(first, second))
