"""Every missing-modality pattern of an MMIMDb batch from one encoder pass: ``MMIMDb.forward_patterns`` /
``zero_projections``, ``FusedMMIMDbPatternEvalStep`` (both fusion legs, GMU and the five pooling kinds),
``evaluate_patterns`` and ``fit_mmimdb(fuse_patterns=True)`` — against the CPU oracle's eval forward on the masked inputs in
fp64, with the per-pattern path of the same build on the masked inputs as the fp32 yardstick (tests/parity.py
``check_out``: 1e-4 against fp64, and 4x the yardstick's error + 2e-6).  The models carry non-trivial BatchNorm running
statistics and affine parameters: a fresh model's zero row would be the biases alone."""
import numpy as np
import pytest
import torch

import tspm_amd
from oracle import mmimdb_ref as orc
from parity import Tally, anchor, check_out, pair_from
from test_mmimdb_cpu import POOL_KINDS, dropin, pool_cfg
from tspm_amd import _lib as L
from tspm_amd import mmimdb as M

pytestmark = pytest.mark.gpu

ALL = ("it", "i", "t")
TALLY = Tally()


def _model(gpu, seed=1, pooling=None):
    """(ours on the device, fp32 oracle, fp64 oracle) holding one state with non-trivial BatchNorm1d statistics."""
    ours = dropin(seed, pooling)
    g = torch.Generator().manual_seed(100 + seed)
    with torch.no_grad():
        for mod in ours.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                c = mod.num_features
                mod.running_mean.copy_(torch.randn(c, generator=g) * 0.3)
                mod.running_var.copy_(torch.rand(c, generator=g) + 0.5)
                mod.weight.copy_(torch.rand(c, generator=g) + 0.5)
                mod.bias.copy_(torch.randn(c, generator=g) * 0.2)
    ours = ours.to(gpu)
    o32, o64 = pair_from(ours, lambda: orc.build_oracle_mmimdb(seed, pooling=pooling))
    return ours, o32, o64


def _oracle(o64, I, T, y, pats):
    """Per pattern the fp64 eval forward on the masked inputs: logits [P, B, C], BCE losses [P]."""
    lg = [orc.eval_forward(o64, I.double() * M.PATTERNS[p][0], T.double() * M.PATTERNS[p][1]) for p in pats]
    return torch.stack(lg), torch.stack([orc.bce_loss(x, y.double()) for x in lg])


def _per_pattern(ours, gpu, I, T, y, pats):
    """The per-pattern path of the same build (MMIMDbEngine's eval forward + tspm_bce_logits on the masked inputs), or
    (None, None) at batch 1, which that engine refuses."""
    B = I.shape[0]
    if B < 2:
        return None, None
    eng, sh = ours._engine(B, gpu), L.stream_handle()
    logits, losses = [], []
    for p in pats:
        ip, tp = M.PATTERNS[p]
        eng.I.copy_(I * ip); eng.T.copy_(T * tp); eng.labels.copy_(y)
        eng.forward(sh, False)
        eng.loss_fn(sh, 1.0, False, False)
        logits.append(eng.logits.cpu().clone()); losses.append(eng.loss.cpu().clone().reshape(()))
    return torch.stack(logits), torch.stack(losses)


def _check(name, logits, loss, ref32, ref64, pats):
    for p, pat in enumerate(pats):
        check_out(f"{name}.logits[{pat}]", logits[p], None if ref32[0] is None else ref32[0][p], ref64[0][p], TALLY)
        if loss is not None:
            check_out(f"{name}.loss[{pat}]", loss[p], None if ref32[1] is None else ref32[1][p], ref64[1][p], TALLY)


@pytest.mark.parametrize("pats", [ALL, ("t", "it")], ids=["all", "t+it"])
@pytest.mark.parametrize("B", [1, 5, 64])
def test_forward_patterns_vs_oracle(gpu, B, pats):
    ours, _, o64 = _model(gpu)
    I, T, y = orc.synthetic_batch(B, seed=300 + B)
    ref64, ref32 = _oracle(o64, I, T, y, pats), _per_pattern(ours, gpu, I, T, y, pats)
    ours.train()  # whatever the mode flag: the pass runs on the running statistics and leaves the flag alone
    got = ours.forward_patterns(I.to(gpu), T.to(gpu), None if pats == ALL else pats)
    assert got.shape == (len(pats), B, 23) and not got.requires_grad and ours.training
    _check(f"forward_patterns B{B}", got, None, ref32, ref64, pats)
    with pytest.raises(ValueError):
        ours.forward_patterns(I.to(gpu), T.to(gpu), patterns=("it", "x"))
    # the zero projections: one row, the fusion's projections of a zeroed input under the oracle; a stable address
    z = ours.zero_projections(refresh=False)
    with torch.no_grad():
        f = o64.fusion_module
        want = torch.cat([f.fc_one(o64.image_model(torch.zeros(1, 4096, dtype=torch.float64))),
                          f.fc_two(o64.text_model(torch.zeros(1, 300, dtype=torch.float64)))], dim=1)[0]
    assert z.shape == (1024,)
    check_out("zero_projections", z, None, want, TALLY)
    assert ours.zero_projections(refresh=True).data_ptr() == z.data_ptr()


@pytest.mark.parametrize("fusion", ["kernel", "launches"])
@pytest.mark.parametrize("pats", [ALL, ("t", "it")], ids=["all", "t+it"])
@pytest.mark.parametrize("B", [1, 5, 64])
def test_fused_pattern_eval_step_vs_oracle(gpu, B, pats, fusion):
    ours, _, o64 = _model(gpu)
    st = M.FusedMMIMDbPatternEvalStep(ours, None, B, patterns=pats, fusion=fusion)
    assert st.fusion == fusion and st.patterns == tuple(pats)
    P = len(pats)
    logged, counts = [], np.zeros((P, 1 + 3 * 23))
    for k in range(3):  # eager, capture, replay: three different batches
        I, T, y = orc.synthetic_batch(B, seed=400 + 10 * B + k)
        ref64 = _oracle(o64, I, T, y, pats)
        ref32 = _per_pattern(ours, gpu, I, T, y, pats) if k == 0 else (None, None)
        out = st.step(I.to(gpu), T.to(gpu), y.to(gpu))
        assert out["logits"].shape == (P, B, 23) and out["loss"].shape == (P,)
        _check(f"{fusion} B{B} call {k}", out["logits"], out["loss"], ref32, ref64, pats)
        logged += out["loss"].cpu().tolist()
        for p in range(P):  # the counts of the step's OWN logits
            counts[p] += np.array(orc.f1_counts(out["logits"][p].cpu(), y))
    assert st.graph is not None
    s = st.stats.cpu()
    assert s[:, 1].tolist() == [3.0 * B] * P
    np.testing.assert_allclose(s[:, 2:].numpy(), counts.astype(np.float32), rtol=1e-6, atol=1e-4)
    assert st.counters.cpu().tolist() == [3 * P, 3 * P * B]
    assert st.loss_log[:3 * P].cpu().tolist() == logged  # P entries per step, in pattern order
    st.reset_log()
    assert st.counters.cpu().tolist() == [0, 0] and float(st.stats.abs().sum()) == 0.0


def test_legs_agree_bitwise_and_replays_are_bitwise(gpu):
    ours, _, _ = _model(gpu)
    I, T, y = orc.synthetic_batch(5, seed=77)
    Id, Td, yd = I.to(gpu), T.to(gpu), y.to(gpu)
    outs = {}
    for fusion in ("kernel", "launches"):
        st = M.FusedMMIMDbPatternEvalStep(ours, None, 5, fusion=fusion)
        runs = []
        for _ in range(4):  # eager, the capture run, two replays
            out = st.step(Id, Td, yd)
            runs.append({k: v.clone() for k, v in out.items()})
        assert st.graph is not None and st.calls == 4
        for r in runs[1:]:
            assert all(torch.equal(r[k], runs[0][k]) for k in r), fusion
        outs[fusion] = dict(runs[0], stats=st.stats.clone(), log=st.loss_log[:12].clone(), counters=st.counters.clone())
    for k in outs["kernel"]:
        assert torch.equal(outs["kernel"][k], outs["launches"][k]), k
    assert outs["kernel"]["counters"].cpu().tolist() == [12, 60]
    with pytest.raises(ValueError):
        M.FusedMMIMDbPatternEvalStep(ours, None, 5, fusion="triton")


@pytest.mark.parametrize("kind", POOL_KINDS)
def test_pooling_models_take_the_launches_leg(gpu, kind):
    ours, _, o64 = _model(gpu, seed=0, pooling=pool_cfg(kind))
    B = 16
    I, T, y = orc.synthetic_batch(B, seed=500)
    st = M.FusedMMIMDbPatternEvalStep(ours, None, B)  # the default leg falls back: no pattern kernel for the pooling
    assert st.fusion == "launches"
    ref64, ref32 = _oracle(o64, I, T, y, ALL), _per_pattern(ours, gpu, I, T, y, ALL)
    for k in range(3):
        out = st.step(I.to(gpu), T.to(gpu), y.to(gpu))
        _check(f"pooling {kind} call {k}", out["logits"], out["loss"], ref32, ref64, ALL)


def test_zero_projections_follow_a_train_step(gpu):
    """FusedAdam writes the parameters through raw pointers: forward_patterns refreshes the zero projections itself."""
    ours, _, o64 = _model(gpu)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=1e-3, weight_decay=1e-3)
    I, T, y = orc.synthetic_batch(5, seed=99)
    Id, Td = I.to(gpu), T.to(gpu)
    first = ours.forward_patterns(Id, Td)
    z_first = ours.zero_projections(refresh=False).clone()
    tI, tT, ty = orc.synthetic_batch(8, seed=1234)
    M.FusedMMIMDbStep(ours, opt, None, 8).step(tI.to(gpu), tT.to(gpu), ty.to(gpu))
    second = ours.forward_patterns(Id, Td)
    anchor(o64, ours)  # the oracle at OUR updated state (parameters and running statistics)
    _check("after one train step", second, None, (None, None), _oracle(o64, I, T, y, ALL), ALL)
    assert not torch.equal(ours.zero_projections(refresh=False), z_first)
    assert not torch.equal(second[1], first[1]) and not torch.equal(second[2], first[2])  # the i / t logits moved


def _oracle_evaluation(o64, Iv, Tv, yv, B, pats):
    """evaluate_patterns restated on the fp64 oracle: the mean of the per-(batch, pattern) losses and, per pattern,
    f1_metrics of the counts over the whole corpus."""
    n, entries, out = Iv.shape[0], [], {}
    for pat in pats:
        ip, tp = M.PATTERNS[pat]
        logits, loss_sum = [], 0.0
        for s in range(0, n, B):
            sl = slice(s, min(s + B, n))
            lg = orc.eval_forward(o64, Iv[sl].double() * ip, Tv[sl].double() * tp)
            logits.append(lg)
            bl = orc.bce_loss(lg, yv[sl].double()).item()
            entries.append(bl)
            loss_sum += bl * lg.shape[0]
        c = orc.f1_counts(torch.cat(logits), yv)
        out[pat] = M.f1_metrics(torch.tensor([loss_sum, float(n)] + c, dtype=torch.float64), 23)
    out["val_loss"] = float(np.mean(entries))
    return out


def _close(got, ref, pats):
    """The slacks of test_gpu_mmimdb.test_fit_loop_metrics_match_oracle: losses 1e-4 relative, F1 figures 2e-2."""
    assert abs(got["val_loss"] - ref["val_loss"]) <= 1e-4 * abs(ref["val_loss"]), (got["val_loss"], ref["val_loss"])
    for pat in pats:
        assert abs(got[pat]["loss"] - ref[pat]["loss"]) <= 1e-4 * abs(ref[pat]["loss"]), pat
        for k in ("f1_samples", "f1_macro", "f1_weighted", "f1_micro"):
            assert abs(got[pat][k] - ref[pat][k]) <= 2e-2, (pat, k, got[pat][k], ref[pat][k])


@pytest.mark.parametrize("fusion", [None, "launches"])
def test_evaluate_patterns_equals_the_per_pattern_loops(gpu, fusion):
    ours, _, _ = _model(gpu, seed=2)
    N, B = 192, 64
    Iv, Tv, yv = orc.synthetic_batch(N, seed=42)
    corpus = M.MMIMDbCorpus(Iv, Tv, yv, gpu)
    got = M.evaluate_patterns(ours, corpus, B, fusion=fusion)
    assert list(got) == ["val_loss", "it", "i", "t"]
    ref = {p: M._evaluate(ours, corpus, B, 1.0, p) for p in ALL}
    # the batch divides N: the default path's monitored loss is the same mean, shuffled or not
    for gen in (None, torch.Generator().manual_seed(7)):
        ref["val_loss"] = M.validation_loss(ours, corpus, B, 1.0, ALL, gen)
        _close(got, ref, ALL)
    sub = M.evaluate_patterns(ours, corpus, B, patterns=("t", "it"), fusion=fusion)
    assert list(sub) == ["val_loss", "t", "it"]
    _close(dict(sub, val_loss=1.0), dict(got, val_loss=1.0), ("t", "it"))  # the same patterns from another step


def test_evaluate_patterns_with_a_one_row_last_batch(gpu):
    ours, _, o64 = _model(gpu, seed=2)
    N, B = 193, 64
    Iv, Tv, yv = orc.synthetic_batch(N, seed=43)
    got = M.evaluate_patterns(ours, M.MMIMDbCorpus(Iv, Tv, yv, gpu), B)
    _close(got, _oracle_evaluation(o64, Iv, Tv, yv, B, ALL), ALL)
    steps = ours.__dict__["_pattern_steps"]
    assert sorted(k[-1] for k in steps) == [1, 64]
    assert steps[(ALL, M.DEFAULT_PATTERN_FUSION, 1.0, 64)].counters.cpu().tolist() == [9, 9 * 64]
    assert steps[(ALL, M.DEFAULT_PATTERN_FUSION, 1.0, 1)].counters.cpu().tolist() == [3, 3]


def test_fit_with_fused_patterns_returns_the_same_keys(gpu, tmp_path):
    def run(fused, sub):
        ours = dropin(2).to(gpu)
        opt = tspm_amd.FusedAdam(ours.parameters(), lr=1e-4, weight_decay=1e-3)
        I, T, y = orc.synthetic_batch(136, seed=41)
        Iv, Tv, yv = orc.synthetic_batch(128, seed=42)  # the batch divides it: both paths monitor the same mean
        return M.fit_mmimdb(ours, opt, M.MMIMDbCorpus(I, T, y, gpu), M.MMIMDbCorpus(Iv, Tv, yv, gpu), 64, epochs=2,
                            checkpoint_dir=tmp_path / sub, fuse_patterns=fused)
    fused, default = run(True, "fused"), run(False, "default")
    assert len(fused) == len(default) == 2
    for a, b in zip(fused, default):
        assert list(a) == list(b) and all(list(a[k]) == list(b[k]) for k in a if isinstance(a[k], dict))
        assert np.isfinite(a["val_loss"]) and abs(a["val_loss"] - b["val_loss"]) <= 1e-4 * abs(b["val_loss"])
    assert (tmp_path / "fused" / "best.pth").exists() and (tmp_path / "fused" / "epoch_1.pth").exists()


def test_zz_tally(gpu):
    print(TALLY)
