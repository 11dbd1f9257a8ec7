"""Every missing-modality pattern of an AVMNIST batch from one encoder pass: ``AVMNIST.forward_patterns`` /
``zero_embeddings``, ``step.FusedPatternEvalStep`` (both heads), the fused loader through ``EpochRunner`` and ``fit``,
against the CPU oracle's per-pattern ``validation_step`` on the masked inputs (the bound of
test_gpu_harness.test_fused_eval_step_vs_oracle: rel-L2 1e-4 on the logits, 1e-4 relative on the loss)."""
import json

import numpy as np
import pytest
import torch

from oracle import avmnist_eval_ref as eref
from oracle import avmnist_ref as orc

pytestmark = pytest.mark.gpu

BOUND = 1e-4
KEEP = {"a": (1, 0), "ai": (1, 1), "i": (0, 1)}
GID = {"a": 0, "ai": 1, "i": 2}
ALL = ("a", "ai", "i")


def rel(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return ((a - b).norm() / b.norm()).item()


def _running_stats(*models):
    """Non-trivial running statistics, as test_fused_eval_step_vs_oracle sets them."""
    for model in models:
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                gg = torch.Generator().manual_seed(m.num_features)
                rm, rv = torch.randn(m.num_features, generator=gg) * 0.1, torch.rand(m.num_features, generator=gg) + 0.5
                with torch.no_grad():
                    m.running_mean.copy_(rm)
                    m.running_var.copy_(rv)


def _models(dev, dropout=0.5):
    import tspm_amd
    torch.manual_seed(0)
    m = tspm_amd.AVMNIST(tspm_amd.ResNet18(1, 64), tspm_amd.ResNet34(1, 128), 128, dropout=dropout).to(dev)
    ref = orc.build_oracle_avmnist(0)
    _running_stats(m, ref)
    return m, ref


def _oracle(ref, audio, image, labels, pats):
    """Per pattern the oracle's validation_step on the masked inputs: logits [P, B, C], losses [P]."""
    outs = [eref.validation_step(ref, audio * KEEP[p][0], image * KEEP[p][1], labels) for p in pats]
    return torch.stack([o["logits"] for o in outs]), torch.stack([o["loss"] for o in outs])


def _check(name, out_logits, out_loss, ref_logits, ref_loss):
    for p in range(ref_logits.shape[0]):
        e = rel(out_logits[p], ref_logits[p])
        dl = abs(out_loss[p].item() - ref_loss[p].item()) / abs(ref_loss[p].item())
        print(f"{name}[{p}]: logits rel-L2 {e:.2e}, loss rel {dl:.2e}")
        assert e < BOUND and dl <= BOUND


def test_forward_patterns_vs_oracle(gpu):
    model, ref = _models(gpu)
    audio, image, labels, _ = orc.synthetic_batch(6, seed=99)
    want, _ = _oracle(ref, audio, image, labels, ALL)
    got = model.forward_patterns(audio.to(gpu), image.to(gpu))
    assert got.shape == (3, 6, 10) and not got.requires_grad
    for p, name in enumerate(ALL):
        e = rel(got[p], want[p])
        print(f"forward_patterns[{name}]: rel-L2 {e:.2e}")
        assert e < BOUND
    sub = model.forward_patterns(audio.to(gpu), image.to(gpu), patterns=("i", "ai"))  # a subset, in the given order
    assert sub.shape == (2, 6, 10) and rel(sub[0], want[2]) < BOUND and rel(sub[1], want[1]) < BOUND
    with pytest.raises(ValueError):
        model.forward_patterns(audio.to(gpu), image.to(gpu), patterns=("a", "x"))
    # the zero embeddings: one row per encoder, the embedding of a zeroed input under the oracle
    z = model.zero_embeddings(refresh=False)
    with torch.no_grad():
        ref.eval()
        za = orc.encoder_forward(ref.audio_encoder, torch.zeros(1, 32, 94), False)
        zi = orc.encoder_forward(ref.image_encoder, torch.zeros(1, 1, 28, 28), False)
    assert z.shape == (192,) and rel(z[:64], za) < BOUND and rel(z[64:], zi) < BOUND
    assert model.zero_embeddings(refresh=True).data_ptr() == z.data_ptr()  # a stable address


@pytest.mark.parametrize("pats", [ALL, ("i", "ai")], ids=["all", "i+ai"])
@pytest.mark.parametrize("head", ["kernel", "launches"])
def test_fused_pattern_eval_step_vs_oracle(gpu, head, pats):
    from tspm_amd.metrics import ClassificationLog
    from tspm_amd.step import FusedPatternEvalStep
    model, ref = _models(gpu)
    log = ClassificationLog(gpu)
    st = FusedPatternEvalStep(model, None, 6, log, patterns=pats, head=head)
    assert st.head == head and st.patterns == tuple(pats)
    P = len(pats)
    losses, conf = [], np.zeros((3, 10, 10), np.int64)
    for k in range(3):  # eager, capture, replay: three different batches
        audio, image, labels, _ = orc.synthetic_batch(6, seed=200 + k)
        out = st.step(audio.to(gpu), image.to(gpu), labels.to(gpu))
        assert out["logits"].shape == (P, 6, 10) and out["preds"].shape == (P, 6) and out["loss"].shape == (P,)
        want, want_loss = _oracle(ref, audio, image, labels, pats)
        _check(f"{head} call {k}", out["logits"], out["loss"], want, want_loss)
        losses += out["loss"].cpu().tolist()
        own = eref.predictions(out["logits"].cpu().reshape(P * 6, 10))
        assert torch.equal(out["preds"].cpu().reshape(-1), own)
        conf += eref.confusion(np.tile(labels.numpy(), P), own.numpy(), np.repeat([GID[p] for p in pats], 6), 3)
    got_conf, ll, n = log.fetch()
    assert n == 3 * P * 6 and ll.tolist() == losses            # 3·P entries, in pattern order within each batch
    assert np.array_equal(got_conf, conf)                       # each row under its pattern's group


def test_heads_agree_and_replays_are_bitwise(gpu):
    from tspm_amd.step import FusedPatternEvalStep
    model, _ = _models(gpu)
    audio, image, labels, _ = orc.synthetic_batch(6, seed=77)
    a, i, lab = audio.to(gpu), image.to(gpu), labels.to(gpu)
    outs = {}
    for head in ("kernel", "launches"):
        st = FusedPatternEvalStep(model, None, 6, None, head=head)
        runs = [{k: v.clone() for k, v in st.step(a, i, lab).items()} for _ in range(3)]  # eager, captured, replayed
        for r in runs[1:]:
            assert all(torch.equal(r[k], runs[0][k]) for k in r), head
        outs[head] = runs[0]
    e = rel(outs["kernel"]["logits"], outs["launches"]["logits"])
    dl = ((outs["kernel"]["loss"] - outs["launches"]["loss"]).abs() / outs["launches"]["loss"].abs()).max().item()
    print(f"kernel vs launches: logits rel-L2 {e:.2e}, loss rel {dl:.2e}")
    assert e < BOUND and dl <= BOUND


def test_loss_group_must_be_one_cross_entropy_term(gpu):
    from tspm_amd import _lib as L
    from tspm_amd.step import FusedPatternEvalStep
    model, _ = _models(gpu)

    class Group(dict):
        pass

    with pytest.raises(L.TspmError, match="single cross-entropy"):
        FusedPatternEvalStep(model, Group(a=object(), b=object()), 6)
    with pytest.raises(ValueError):
        FusedPatternEvalStep(model, None, 6, head="triton")


def test_zero_embeddings_follow_a_train_step(gpu):
    """FusedAdam writes the parameters through raw pointers: forward_patterns refreshes the zero embeddings itself."""
    import tspm_amd
    model, ref = _models(gpu)
    opt = tspm_amd.FusedAdam(model.parameters(), lr=5e-4, weight_decay=1e-4)
    ref_opt = orc.OracleAdam(list(ref.parameters()), lr=5e-4, weight_decay=1e-4)
    audio, image, labels, _ = orc.synthetic_batch(6, seed=99)
    a, i = audio.to(gpu), image.to(gpu)
    first = model.forward_patterns(a, i)
    z_first = model.zero_embeddings(refresh=False).clone()
    ta, ti, tl, _ = orc.synthetic_batch(8, seed=1234)
    keep = (torch.rand(8, 128, generator=torch.Generator().manual_seed(1)) > 0.5).to(torch.uint8)
    st = tspm_amd.FusedTrainStep(model, opt, None, 8)
    st.keep_override = keep.to(gpu)
    st.step(ta.to(gpu), ti.to(gpu), tl.to(gpu))
    orc.train_step(ref, ref_opt, ta, ti, tl, keep)
    second = model.forward_patterns(a, i)
    want, _ = _oracle(ref, audio, image, labels, ALL)
    for p, name in enumerate(ALL):
        e = rel(second[p], want[p])
        print(f"after one train step, forward_patterns[{name}]: rel-L2 {e:.2e}")
        assert e < BOUND
    assert not torch.equal(model.zero_embeddings(refresh=False), z_first)
    assert not torch.equal(second[0], first[0]) and not torch.equal(second[2], first[2])  # the a / i logits moved


def _datasets(gpu, n_val, n_train=64):
    from tspm_amd.data import AVMNIST, synthetic_corpus
    tr = AVMNIST(None, "train", "multimodal", selected_patterns=["ai"], corpus=synthetic_corpus(n_train, 5), device=gpu)
    va = AVMNIST(None, "valid", "multimodal", corpus=synthetic_corpus(n_val, 6), device=gpu)
    return tr, va


def test_runner_refreshes_the_zero_embeddings_each_epoch(gpu):
    import tspm_amd
    from tspm_amd.harness import EpochRunner
    model, _ = _models(gpu)
    opt = tspm_amd.FusedAdam(model.parameters(), lr=5e-4, weight_decay=1e-4)
    tr, va = _datasets(gpu, 64)
    runner = EpochRunner(model, opt, None)
    zs = []
    for _ in range(2):
        runner.train_epoch(tr.device_loader(32, shuffle=True, generator=torch.Generator().manual_seed(1)))
        runner.validate_epoch(va.device_loader(32, fuse_patterns=True))
        zs.append(model.zero_embeddings(refresh=False).clone())
    assert not torch.equal(zs[0], zs[1])
    # ... and what the second epoch used is what the weights give now
    assert torch.equal(model.zero_embeddings(refresh=True), zs[1])


def test_runner_fused_loader_equals_the_default_loader(gpu, lut):
    from tspm_amd.harness import EpochRunner
    model, ref = _models(gpu)
    _, va = _datasets(gpu, 64)
    runner = EpochRunner(model, None, None)
    fl = va.device_loader(32, fuse_patterns=True)
    loss_f, _, met_f, n_f = runner.validate_epoch(fl)
    conf_f, ll_f, rows_f = runner.log.fetch()
    loss_d, _, met_d, n_d = runner.validate_epoch(va.device_loader(32))
    conf_d, ll_d, rows_d = runner.log.fetch()
    print(f"validate_epoch: fused loss {loss_f!r} ({n_f} entries), default loss {loss_d!r} ({n_d} entries)")
    assert n_f == n_d == 6 and rows_f == rows_d == 192 and len(fl) == 2
    assert abs(loss_f - loss_d) <= BOUND * abs(loss_d)
    assert list(met_f.keys()) == list(met_d.keys()) and "accuracy_AI" in met_f
    # batch size divides N: the same per-(batch, pattern) losses in another order
    assert np.allclose(np.sort(ll_f), np.sort(ll_d), rtol=BOUND, atol=0)
    # per-row predictions: the fused step's against the per-pattern path's, on the rows the oracle calls clear
    c = va.corpus
    audio, labels = torch.from_numpy(c.audio), torch.from_numpy(c.labels)
    image = (lut[torch.from_numpy(c.image).long()].float() * (1.0 / 255.0)).unsqueeze(1)
    want, _ = _oracle(ref, audio, image, labels, ALL)
    top2 = want.reshape(192, 10).topk(2, dim=1).values
    clear = ((top2[:, 0] - top2[:, 1]) > 1e-3 * top2[:, 0].abs().clamp_min(1)).reshape(3, 64)
    assert int((~clear).sum()) <= 0.05 * 192
    pf = torch.empty(3, 64, dtype=torch.int64)
    for k, b in enumerate(fl):
        assert b["fused_patterns"] and b["patterns"] == list(ALL) and "pattern_name" not in b and "pattern_ids" not in b
        st = runner.pattern_eval_step_for(32, b["patterns"])
        pf[:, 32 * k:32 * (k + 1)] = st.step(b["audio"], b["image"], b["labels"])["preds"].cpu()
    pd = torch.empty(3, 64, dtype=torch.int64)
    for k, b in enumerate(va.device_loader(32)):  # items p·N + s in order: batch k is pattern k // 2, samples 32·(k % 2)...
        r = model.validation_step(b, None, gpu, None, return_test_info=True)
        assert set(b["pattern_name"]) == {ALL[k // 2]}
        pd[k // 2, 32 * (k % 2):32 * (k % 2 + 1)] = torch.from_numpy(r["predictions"])
    assert torch.equal(pf[clear], pd[clear]) and torch.equal(pf[clear], eref.predictions(want.reshape(192, 10)).reshape(3, 64)[clear])
    if bool(clear.all()):
        assert np.array_equal(conf_f, conf_d)


def test_runner_partial_last_batch(gpu):
    from tspm_amd.harness import EpochRunner
    model, _ = _models(gpu)
    _, va = _datasets(gpu, 40)
    runner = EpochRunner(model, None, None)
    loss, _, metrics, n = runner.validate_epoch(va.device_loader(32, fuse_patterns=True))
    conf, ll, rows = runner.log.fetch()
    assert n == 6 and rows == 3 * 40 and conf.sum() == 3 * 40 and [int(c.sum()) for c in conf] == [40, 40, 40]
    assert np.isfinite(loss) and set(runner.pattern_eval_steps) == {(ALL, 32), (ALL, 8)}
    assert not runner.eval_steps  # kept apart from the FusedEvalStep cache


def test_validation_step_on_a_fused_batch(gpu):
    from tspm_amd import _lib as L
    from tspm_amd.harness import AVMNIST_METRICS
    from tspm_amd.metrics import ClassificationLog, DeviceMetricRecorder
    model, _ = _models(gpu)
    _, va = _datasets(gpu, 8)
    batch = next(iter(va.device_loader(8, fuse_patterns=True)))
    log = ClassificationLog(gpu)
    r = model.validation_step(batch, None, gpu, DeviceMetricRecorder(AVMNIST_METRICS, log))
    conf, ll, rows = log.fetch()
    assert rows == 24 and len(ll) == 3 and r["loss"] == pytest.approx(float(np.mean(ll)), rel=1e-6)
    with pytest.raises(L.TspmError, match="DeviceMetricRecorder"):
        model.validation_step(batch, None, gpu, None)


def test_fit_with_fused_loaders_writes_the_same_keys(gpu, tmp_path):
    import tspm_amd
    from tspm_amd.harness import fit

    def keys_of(fused, sub):
        model, _ = _models(gpu)
        opt = tspm_amd.FusedAdam(model.parameters(), lr=5e-4, weight_decay=1e-4)
        tr, va = _datasets(gpu, 40)
        loaders = {"train": tr.device_loader(32, shuffle=True, generator=torch.Generator().manual_seed(3)),
                   "validation": va.device_loader(32, fuse_patterns=fused),
                   "test": va.device_loader(32, fuse_patterns=fused)}
        h = fit(model, opt, None, loaders, epochs=1, metrics_path=tmp_path / sub)
        em = json.load(open(tmp_path / sub / "epoch_metrics.json"))

        def walk(d, pre=""):
            return {pre + k for k in d} | {x for k, v in d.items() if isinstance(v, dict) for x in walk(v, pre + k + ".")}
        return walk(em[0]), set(h["test"]), set(h["validation"][0])

    fused, default = keys_of(True, "fused"), keys_of(False, "default")
    assert fused == default and "validation.AI.f1_macro" in fused[0] and "accuracy_AI" in fused[1]
