"""UTT-Fusion on unaligned MOSI / MOSEI batches — audio, video and text each at its own length (Ta, Tv, Tt) — on the HIP
path against the CPU oracle (oracle/mosi_ref.py accepts three lengths as it is).

Inputs are three tensors of their own lengths from one generator, in the scales of ``oracle.synthetic_batch``.  Criterion
and helpers are those of tests/test_gpu_mosi.py / test_gpu_mosi_widths.py / test_gpu_mosi_regress.py (tests/parity.py):
the oracle in fp64 with our decisions forced into it is the truth; a forced decision that differs from fp64's own must be
a near-tie and rare; logits / loss rel-L2 <= 1e-4, every gradient rel-L2 <= 1e-3, cosine >= 0.9999 and within 4x the fp32
reference's error; the clip coefficient against our total norm; Adam exactly; every step from our own state.

MOSI config at (7, 9, 6); MOSEI config ("maxpool", BatchNorm classifier) at (260, 5, 6), where the audio encoder needs
the 16-bit time index and the launch it shares with the video encoder takes tspm_lstm_fwd_t16 / _bwd_t16.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tspm_amd
from oracle import mosi_ref as orc
from parity import Tally, check_out, pair_from, rel_l2, snapshot
from test_gpu_mosi import _check_adam, _check_step, _corpus_from, _masked
from test_gpu_mosi_regress import Group, _scores
from test_gpu_mosi_regress import _check_step as _check_regress_step
from test_gpu_mosi_widths import _dropin, _mono, _oracle
from tspm_amd import _lib as L
from tspm_amd import harness
from tspm_amd import mosi as M
from tspm_amd.monomodal import fit_monomodal
from tspm_amd.mosi_data import MOSI, PATTERNS, MosiCorpus

pytestmark = pytest.mark.gpu
W64 = (64, 64, 64)
MOSI_TS, MOSEI_TS = (7, 9, 6), (260, 5, 6)


def _batch(B, Ts, seed, cfg=orc.MOSI):
    """orc.synthetic_batch's scales with each modality at its own length, from one generator."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(B, Ts[0], cfg.audio_dim, generator=g)
    V = 0.5 * torch.randn(B, Ts[1], cfg.video_dim, generator=g)
    T = 0.3 * torch.randn(B, Ts[2], cfg.text_dim, generator=g)
    return A, V, T, torch.randint(0, 3, (B,), generator=g)


def _steps_vs_oracle(gpu, cfg, widths, B, Ts, n_steps, seed=3):
    ours = _dropin(seed, cfg, widths).to(gpu)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
    A, V, T, y = _batch(B, Ts, 1234 + B, cfg)
    st = M.FusedMosiStep(ours, opt, None, B, Ts)
    e = st.eng
    assert st.T == Ts and e.T == Ts and e.Ts == Ts
    assert tuple(e.A.shape) == (Ts[0], B, cfg.audio_dim) and tuple(e.V.shape) == (Ts[1], B, cfg.video_dim)
    assert tuple(e.X.shape) == (Ts[2], B, cfg.text_dim)
    tally = Tally()
    for s in range(n_steps):
        keeps = orc.keep_masks(B, 50 + s, cfg=cfg)
        o32, o64 = pair_from(ours, lambda: _oracle(seed, cfg, widths))
        before = snapshot(ours, opt if s else None)
        st.keep_override = {k: v.to(gpu) for k, v in keeps.items()}
        out = st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        rep = _check_step(ours, st, o32, o64, A, V, T, y, keeps, out, tally)
        coef = float(e.clip_coef.item())
        exp = min(1.0, cfg.clip / (e.total_norm.item() + 1e-6))
        assert abs(coef - exp) <= 1e-6 * exp
        _check_adam(ours, opt, before, s + 1, coef, cfg)
        for enc in (ours.netA, ours.netV):  # one split per encoder: the two bias gradients stay bitwise equal
            assert torch.equal(enc.rnn.bias_ih_l0.grad, enc.rnn.bias_hh_l0.grad)
        print(f"[{widths} B={B} T={Ts} step {s + 1}] flips {rep} norm {e.total_norm.item():.3f} clip coef {coef:.4f}")
    print(tally)
    return ours, st, (A, V, T, y)


@pytest.mark.parametrize("B,widths", [(4, W64), (3, W64), (4, (36, 64, 64))], ids=["b4", "b3_odd", "b4_widths_36_64_64"])
def test_mosi_unaligned_step_vs_oracle(gpu, B, widths):
    """Three steps (eager, captured, replayed) at (Ta, Tv, Tt) = (7, 9, 6): logits, loss, every gradient, the clip norm
    and Adam."""
    cfg = orc.UttConfig() if widths == W64 else orc.UttConfig(cls_layers=(64, 32))
    _, st, _ = _steps_vs_oracle(gpu, cfg, widths, B, MOSI_TS, 3)
    assert st.graph is not None and not st.eng.wide
    assert st.eng.lstm["a"]["arg"] is None  # embd "last": no index at all


def test_unaligned_graph_replay_equals_eager(gpu):
    cfg, res = orc.MOSI, []
    for use_graph in (False, True):
        ours = _dropin(7, cfg, W64).to(gpu)
        opt = tspm_amd.FusedAdam(ours.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
        st = M.FusedMosiStep(ours, opt, None, 4, MOSI_TS, use_graph=use_graph)
        A, V, T, y = _batch(4, MOSI_TS, 5)
        for s in range(4):  # eager, capture, two replays
            st.keep_override = {k: v.to(gpu) for k, v in orc.keep_masks(4, 90 + s).items()}
            st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        assert (st.graph is not None) == use_graph
        res.append(torch.cat([p.detach().reshape(-1) for p in ours.parameters()] + [st.eng.loss.reshape(-1)]).cpu())
    assert torch.equal(res[0], res[1])


@pytest.mark.parametrize("pattern", ["atv", "a", "tv"])
def test_unaligned_missing_patterns_through_the_masks(gpu, pattern):
    """Patterns "avt", "a" and "vt" (PATTERNS spells them "atv", "a", "tv"): the loader gathers the batch with the
    pattern's modality masks straight into the step's three buffers — the host-masked batch, bitwise — and the step is
    held to the criterion against the oracle fed the same zeroed modalities."""
    B, cfg = 4, orc.MOSI
    A, V, T, y = _batch(B, MOSI_TS, 777)
    Am, Vm, Tm = _masked(A, V, T, pattern)
    ours = _dropin(3, cfg, W64).to(gpu)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
    ds = MOSI(split="train", corpus=_corpus_from(A, V, T, y), device=gpu, selected_patterns=[pattern])
    seen = []
    b = next(iter(ds.device_loader(B, shuffle=False,
                                   step_for=lambda n, t: seen.append((n, t)) or ours.fused_step(opt, None, n, t))))
    assert seen == [(B, MOSI_TS)] and b["steps"] == MOSI_TS and b["time_major"]
    st = ours.fused_step(opt, None, B, MOSI_TS)
    assert b["audio"] is st.eng.A and b["video"] is st.eng.V and b["text"] is st.eng.X
    for buf, ref in ((st.eng.A, Am), (st.eng.V, Vm), (st.eng.X, Tm)):
        assert torch.equal(buf.transpose(0, 1).cpu(), ref)
    keeps = orc.keep_masks(B, 61)
    o32, o64 = pair_from(ours, lambda: _oracle(3, cfg, W64))
    before = snapshot(ours)
    st.keep_override = {k: v.to(gpu) for k, v in keeps.items()}
    st.run()
    torch.cuda.synchronize()
    tally = Tally()
    rep = _check_step(ours, st, o32, o64, Am, Vm, Tm, y, keeps, {"loss": st.eng.loss, "logits": st.eng.logits}, tally)
    _check_adam(ours, opt, before, 1, float(st.eng.clip_coef.item()))
    print(f"[pattern {pattern}] flips {rep}; {tally}")


def _oracle_audio_indices(o, A):
    """The fp64 oracle's own "maxpool" time indices of the audio encoder (nothing forced)."""
    tr = orc.MosiTrace()
    with torch.no_grad():
        orc.lstm_forward(o.netA, A.double(), tr, "lstm.a.pool")
    return tr.idx["lstm.a.pool"]


def test_mosei_wide_index_step_vs_oracle(gpu):
    """MOSEI config at (260, 5, 6), B = 3 (a ghost row): the audio recurrence is "maxpool" past 256 steps, so the launch
    takes the 16-bit index for both encoders.  Two steps (eager, captured)."""
    cfg, B = orc.MOSEI, 3
    A = _batch(B, MOSEI_TS, 1234 + B, cfg)[0]
    # on the oracle alone: at least one audio maximum falls at a step >= 256
    i64 = _oracle_audio_indices(_oracle(3, cfg, W64).double(), A)
    assert int((i64 >= 256).sum()) >= 1
    ours, st, _ = _steps_vs_oracle(gpu, cfg, W64, B, MOSEI_TS, 2)
    e = st.eng
    assert e.wide and e.lstm["a"]["arg"].dtype == torch.int16 and e.lstm["v"]["arg"].dtype == torch.int16
    arg = L.index_to_int64(e.lstm["a"]["arg"]).cpu()
    assert int(arg.max()) < 260 and int((arg >= 256).sum()) >= 1, "the step itself stored indices past 8 bits"
    assert int(L.index_to_int64(e.lstm["v"]["arg"]).max()) < 5
    assert e.wg_splits == {"a": max(1, min(32, 260 * B // 128)), "v": 1}  # each encoder's own T_m * B
    print(f"audio indices >= 256: {int((arg >= 256).sum())} of {arg.numel()} (oracle alone: {int((i64 >= 256).sum())})")


def test_mosei_wide_index_eval_step_vs_oracle(gpu):
    cfg, B = orc.MOSEI, 3
    ours = _dropin(6, cfg, W64).to(gpu)
    o = _oracle(6, cfg, W64)
    o.load_state_dict({k: v.cpu() for k, v in ours.state_dict().items()})
    A, V, T, y = _batch(B, MOSEI_TS, 31, cfg)
    from tspm_amd.metrics import ClassificationLog
    log = ClassificationLog(gpu, groups=PATTERNS, classes=3)
    st = M.FusedMosiEvalStep(ours, None, B, MOSEI_TS, log)
    assert st.eng.wide and st.eng is ours._engine(B, MOSEI_TS, gpu)
    st.eng.groups.copy_(log.group_ids(["atv"] * B))
    outs = []
    for _ in range(3):  # eager, capture, replay
        st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        outs.append((st.eng.logits.cpu().clone(), st.eng.loss.cpu().clone()))
    assert all(torch.equal(a[0], outs[0][0]) and torch.equal(a[1], outs[0][1]) for a in outs[1:])
    r = orc.validation_step(o.double(), A.double(), V.double(), T.double(), y)
    check_out("mosei unaligned eval logits", outs[0][0], None, r["logits"])
    assert abs(outs[0][1].item() - r["loss"].item()) <= 1e-4 * abs(r["loss"].item())
    batch = {"audio": A, "video": V, "text": T, "label": y, "pattern_name": ["atv"] * B}
    v = ours.validation_step(batch, None, gpu, None)  # each modality's length read from its own tensor
    assert v["loss"] == outs[0][1].item()
    with torch.no_grad():  # the inference helper takes the wide index under the same rule
        ours.eval()
        assert torch.equal(ours.netA(A.to(gpu)), st.eng.fused[:, :64])


def test_mosei_wide_index_regression_step_vs_oracle(gpu):
    """output_dim = 1 with the one-launch L1 head at (260, 5, 6)."""
    cfg, B, seed = orc.MOSEI, 3, 3
    ours = _dropin(seed, cfg, W64, output_dim=1).to(gpu)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
    A, V, T, _ = _batch(B, MOSEI_TS, 1234 + B, cfg)
    y = _scores(B, 77 + B)
    st = M.FusedMosiStep(ours, opt, Group("l1", 1.0), B, MOSEI_TS)
    assert st.regress == (L.REGRESS_L1, 1.0) and st.eng.wide
    keeps = orc.keep_masks(B, 50, cfg=cfg)
    o32, o64 = pair_from(ours, lambda: _oracle(seed, cfg, W64, output_dim=1))
    before = snapshot(ours, None)
    st.keep_override = {k: v.to(gpu) for k, v in keeps.items()}
    out = st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
    torch.cuda.synchronize()
    tally = Tally()
    rep = _check_regress_step(ours, st, o32, o64, A, V, T, y, keeps, out, tally, "l1", 1.0)
    coef = float(st.eng.clip_coef.item())
    exp = min(1.0, cfg.clip / (st.eng.total_norm.item() + 1e-6))
    assert abs(coef - exp) <= 1e-6 * exp
    _check_adam(ours, opt, before, 1, coef, cfg)
    print(f"[regression {MOSEI_TS}] flips {rep}; {tally}")


def test_int_and_equal_triple_are_the_same_step(gpu):
    """fused_step(..., 8) and fused_step(..., (8, 8, 8)) are one object (and one engine); a step planned at 8 gives
    bitwise the outputs and updated parameters of a fresh model stepped through the triple form."""
    cfg, B = orc.MOSI, 4
    A, V, T, y = _batch(B, (8, 8, 8), 11)
    got = []
    for form in (8, (8, 8, 8)):
        ours = _dropin(5, cfg, W64).to(gpu)
        opt = tspm_amd.FusedAdam(ours.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
        st = ours.fused_step(opt, None, B, form)
        assert st is ours.fused_step(opt, None, B, 8) and st is ours.fused_step(opt, None, B, (8, 8, 8))
        assert st is ours.fused_step(opt, None, B, [8, 8, 8]) and st.T == 8 and st.eng.T == 8
        assert ours._engine(B, (8, 8, 8), gpu) is ours._engine(B, 8, gpu) and len(ours._steps) == 1
        assert not st.eng.wide and len(st.eng._lens) == 1
        for s in range(3):
            st.keep_override = {k: v.to(gpu) for k, v in orc.keep_masks(B, 20 + s).items()}
            out = st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        got.append(torch.cat([out["logits"].reshape(-1), out["loss"].reshape(-1)] +
                             [p.detach().reshape(-1) for p in ours.parameters()]).cpu())
    assert torch.equal(got[0], got[1])


def test_autograd_node_gradients_equal_the_fused_steps(gpu):
    """The autograd fallback (_UttFn: torch optimizer / another loss) at (7, 9, 6), dropout off: its gradients are the
    fused step's (the two differ only in where cross-entropy's gradient is formed)."""
    cfg, B = orc.MOSI, 4
    A, V, T, y = _batch(B, MOSI_TS, 21)
    grads = {}
    for kind in ("fused", "autograd"):
        ours = _dropin(4, cfg, W64, clip=1e9).to(gpu)
        ours.netT.dropout.p = 0.0
        ours.netC.dropout_p = 0.0
        if kind == "fused":
            opt = tspm_amd.FusedAdam(ours.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
            ours.fused_step(opt, None, B, MOSI_TS).step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
        else:
            ours.train()
            logits = ours(A.to(gpu), V.to(gpu), T.to(gpu))
            assert ours._engine(B, MOSI_TS, gpu).Ts == MOSI_TS
            F.cross_entropy(logits, y.to(gpu)).backward()
        torch.cuda.synchronize()
        grads[kind] = torch.cat([p.grad.detach().reshape(-1) for p in ours.parameters()]).cpu()
    assert bool(grads["fused"].abs().sum() > 0)
    assert rel_l2(grads["autograd"], grads["fused"]) < 1e-6


def _ragged_corpus(n, seed, regression=False, la=(5, 12), lv=(4, 10), lt=(5, 8)):
    """A corpus whose modalities differ in length sample by sample (audio 5..12, video 4..10, text 5..8 steps)."""
    g = np.random.default_rng(seed)
    lens = {"audio": g.integers(la[0], la[1] + 1, n), "video": g.integers(lv[0], lv[1] + 1, n),
            "text": g.integers(lt[0], lt[1] + 1, n)}
    seqs = {m: [(s * g.standard_normal((int(l), f))).astype(np.float32) for l in lens[m]]
            for m, f, s in (("audio", 5, 1.0), ("video", 20, 0.5), ("text", 768, 0.3))}
    lab = (g.integers(-15, 16, n) / 5.0).astype(np.float32) if regression else g.integers(0, 3, n).astype(np.int64)
    return MosiCorpus(seqs, lab)


def _pad_np(corpus, m, rows, tpad):
    """pad_sequence(batch_first) of one modality in numpy."""
    out = np.zeros((len(rows), tpad, corpus.feat[m]), np.float32)
    for j, i in enumerate(rows):
        o, l = int(corpus.offsets[m][i]), int(corpus.lengths[m][i])
        out[j, :l] = corpus.data[m][o:o + l]
    return out


def test_loader_gathers_unaligned_batches_into_the_steps_buffers(gpu):
    corpus = _ragged_corpus(12, seed=3)
    ours = _dropin(0, orc.MOSI, W64).to(gpu)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=1e-3, weight_decay=1e-3)
    tr = MOSI(split="train", corpus=corpus, device=gpu, selected_patterns=["atv"])
    seen = []
    step_for = lambda n, t: seen.append((n, t)) or ours.fused_step(opt, None, n, t)  # noqa: E731
    for k, b in enumerate(tr.loader(4, step_for=step_for)):
        rows = list(range(4 * k, 4 * k + 4))
        want = tuple(int(corpus.lengths[m][rows].max()) for m in ("audio", "video", "text"))
        assert seen[-1] == (4, M.norm_steps(want)) and b["steps"] == M.norm_steps(want) and b["time_major"]
        e = ours.fused_step(opt, None, 4, want).eng
        assert b["audio"] is e.A and b["video"] is e.V and b["text"] is e.X
        for m, buf, tp in (("audio", e.A, want[0]), ("video", e.V, want[1]), ("text", e.X, want[2])):
            assert tuple(buf.shape) == (tp, 4, corpus.feat[m])
            assert np.array_equal(buf.transpose(0, 1).cpu().numpy(), _pad_np(corpus, m, rows, tp)), (k, m)
        assert torch.equal(e.labels.cpu(), torch.from_numpy(corpus.labels[rows]))
    assert len(seen) == 3 and len({t for _, t in seen}) > 1  # ragged: pad_sequence's per-batch lengths
    # the collate without a step: batch-first tensors, each modality its own T_m
    b = tr.collate_fn(tr.__getitems__([0, 1, 2, 3]))
    want = tuple(int(corpus.lengths[m][[0, 1, 2, 3]].max()) for m in ("audio", "video", "text"))
    for m, tp in zip(("audio", "video", "text"), want):
        assert np.array_equal(b[m].cpu().numpy(), _pad_np(corpus, m, [0, 1, 2, 3], tp))
    # a per-modality pad_to that covers the corpus: one step shape for the epoch
    seen.clear()
    for b in tr.loader(4, step_for=step_for, pad_to=(12, 10, 8)):
        assert b["steps"] == (12, 10, 8)
    assert seen == [(4, (12, 10, 8))] * 3
    seen.clear()
    for b in tr.loader(4, step_for=step_for, pad_to={"audio": 12, "video": 12, "text": 12}):
        assert b["steps"] == 12  # entries that agree are the aligned int
    assert seen == [(4, 12)] * 3
    # the valid split groups by pattern; every group is gathered at its own per-modality lengths with its mask
    va = MOSI(split="valid", corpus=corpus, device=gpu, selected_patterns=["atv", "a"])
    runner = harness.MosiEpochRunner(ours, opt, None)
    for b in va.loader(8, shuffle=True, seed=2, step_for=runner.eval_step_for):
        (p, sub), = b.items()
        assert set(sub["pattern_name"]) == {p}
        e = runner.eval_step_for(len(sub["pattern_name"]), sub["steps"]).eng
        assert sub["audio"] is e.A and tuple(e.Ts) == M.steps_triple(sub["steps"])
        if p == "a":
            assert bool((e.V == 0).all()) and bool((e.X == 0).all()) and bool((e.A != 0).any())


def _fit_loaders(corpus_tr, corpus_va, gpu, key="classification_labels", pad_to=(12, 10, 8)):
    tr = MOSI(split="train", corpus=corpus_tr, device=gpu, seed=4, labels_key=key)
    va = MOSI(split="valid", corpus=corpus_va, device=gpu, labels_key=key)
    return va, {"train": tr.loader(4, shuffle=True, seed=1, pad_to=pad_to), "validation": va.loader(4, pad_to=pad_to),
                "test": va.loader(4, pad_to=pad_to)}


def test_harness_fit_on_an_unaligned_corpus(gpu, tmp_path):
    """harness.fit, two epochs, batch 4, lengths <= 12: trains, validates by pattern and tests; the test epoch's loss
    and per-pattern confusion counts equal a loop calling validation_step by hand on the same batches."""
    from sklearn.metrics import confusion_matrix
    ours = _dropin(8, orc.MOSI, W64).to(gpu)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=1e-3, weight_decay=1e-3)
    va, loaders = _fit_loaders(_ragged_corpus(16, seed=1), _ragged_corpus(4, seed=2), gpu)
    hist = harness.fit(ours, opt, None, loaders, epochs=2, early_stopping=False, checkpoint_dir=tmp_path / "ck")
    assert len(hist["train"]) == 2 and np.isfinite(hist["train"][-1]["loss"]) and np.isfinite(hist["validation"][-1]["loss"])
    assert {k[3] for k in ours._steps} == {(12, 10, 8)}  # one train step shape, one graph, for the epochs
    losses, preds, labels = [], {p: [] for p in PATTERNS}, {p: [] for p in PATTERNS}

    class Rec:
        def update_group_all(self, group, predictions, targets, m_types):
            for pr, t, m in zip(np.atleast_1d(predictions), np.atleast_1d(targets), m_types):
                preds[m].append(int(pr))
                labels[m].append(int(t))
    for b in va.device_loader(4, pad_to=(12, 10, 8)):
        for p, sub in b.items():
            assert tuple(sub["audio"].shape[1:]) == (12, 5) and tuple(sub["text"].shape[1:]) == (8, 768)
            losses.append(ours.validation_step(sub, None, gpu, Rec())["loss"])
    te = hist["test"]
    assert abs(te["loss"] - float(np.mean(losses))) <= 1e-6 * abs(te["loss"])
    for p in PATTERNS:
        conf = confusion_matrix(np.asarray(labels[p]), np.asarray(preds[p]), labels=[0, 1, 2])
        assert np.array_equal(np.asarray(te[f"ConfusionMatrix_{p.upper()}"]), conf), p


def test_harness_fit_regression_on_an_unaligned_corpus(gpu):
    ours = _dropin(8, orc.MOSI, W64, output_dim=1).to(gpu)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=1e-3, weight_decay=1e-3)
    group = Group("l1")
    va, loaders = _fit_loaders(_ragged_corpus(8, seed=1, regression=True), _ragged_corpus(4, seed=2, regression=True), gpu,
                               key="regression_labels", pad_to=0)  # pad_sequence's own lengths: several step shapes
    hist = harness.fit(ours, opt, group, loaders, epochs=1, early_stopping=False)
    assert any(isinstance(k[3], tuple) for k in ours._steps)
    losses = [ours.validation_step(sub, group, gpu, None)["loss"] for b in va.device_loader(4) for sub in b.values()]
    assert np.isfinite(hist["train"][-1]["loss"])
    assert abs(hist["test"]["loss"] - float(np.mean(losses))) <= 1e-6 * abs(hist["test"]["loss"])
    assert any(k.startswith("MSA_MAE_") for k in hist["test"])


def test_fit_monomodal_maxpool_past_256_steps_hands_over_to_utt_fusion(gpu, tmp_path):
    """Audio alone, "maxpool", T = 260: the pre-training step takes the wide index; encoder_audio_best.pth loads into
    UttFusionModel.netA, whose embedding then equals the pre-trained encoder's."""
    cfg = orc.UttConfig(embd_method="maxpool")
    ours = _mono(5, 64, "maxpool", gpu, 0)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=1e-3, weight_decay=1e-3)

    def corpus(n, seed):
        g = np.random.default_rng(seed)
        seqs = {"audio": [g.standard_normal((260, 5)).astype(np.float32) for _ in range(n)],
                "video": [np.zeros((1, 20), np.float32)] * n, "text": [np.zeros((5, 768), np.float32)] * n}
        return MosiCorpus(seqs, g.integers(0, 3, n).astype(np.int64))
    tr = MOSI(corpus=corpus(8, 5), split="train", target_modality="audio", selected_patterns=["a"], device=gpu)
    va = MOSI(corpus=corpus(4, 6), split="valid", target_modality="audio", selected_patterns=["a"], device=gpu)
    loaders = {"train": tr.loader(4, shuffle=True, seed=0), "validation": va.loader(4), "test": va.loader(4)}
    h = fit_monomodal(ours, opt, None, loaders, 1, experiment_name="MOSI_Audio_Encoder_Pretrain",
                      model_output_path=tmp_path)
    assert h["encoder_path"] and (tmp_path / "encoder_audio_best.pth").exists()
    engines = list(ours._mosi_engines.values()) if hasattr(ours, "_mosi_engines") else []
    assert all(e.wide and e.bufs["arg"].dtype == torch.int16 for e in engines)
    enc_sd = torch.load(tmp_path / "encoder_audio_best.pth", weights_only=True)
    fusion = _dropin(1, cfg, W64)
    fusion.netA.load_state_dict(enc_sd)
    assert list(enc_sd) == list(fusion.netA.state_dict())
    fusion = fusion.to(gpu).eval()
    A, V, T, _ = _batch(3, MOSEI_TS, 9, cfg)
    eng = fusion._engine(3, MOSEI_TS, gpu)
    eng.load(A.to(gpu), V.to(gpu), T.to(gpu))
    eng.forward(L.stream_handle(), False)
    torch.cuda.synchronize()
    assert eng.wide
    with torch.no_grad():
        ours.eval()
        assert torch.equal(ours.encoder(A.to(gpu)), eng.fused[:, :64])


def test_wrong_length_names_the_modality(gpu):
    ours = _dropin(0, orc.MOSI, W64).to(gpu).eval()
    eng = ours._engine(4, MOSI_TS, gpu)
    A, V, T, _ = _batch(4, MOSI_TS, 1)
    eng.load(A.to(gpu), V.to(gpu), T.to(gpu))
    A8 = _batch(4, (8, 9, 6), 1)[0]
    with pytest.raises(L.TspmError, match="audio"):
        eng.load(A8.to(gpu), V.to(gpu), T.to(gpu))
    with pytest.raises(L.TspmError, match="video"):
        eng.load(A.to(gpu), V[:, :8].contiguous().to(gpu), T.to(gpu))
    with pytest.raises(L.TspmError, match="text"):
        eng.load(A.to(gpu), V.to(gpu), T[:, :5].contiguous().to(gpu))
    with pytest.raises(L.TspmError, match="text length is 256"):
        ours._engine(2, (300, 300, 256), gpu)
