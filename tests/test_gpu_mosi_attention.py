"""LSTMEncoder(embd_method="attention", attention_norm="time" | "unit") on the UTT-Fusion HIP path, model level: the fused
step, ragged mode, frozen encoders, mixed methods, the autograd node, regression mode, the standalone encoder, the
encoder pre-training step and the epoch harness.

The oracle is oracle/mosi_ref.py around tests/attn_ref.py's restatement of the embedding (``AttnEncoderRef`` modules in
the oracle model, ``orc.lstm_forward`` replaced by ``AttnOracle``); the checks, tolerances, forced decisions and
dropout-mask injection are those of test_gpu_mosi.py (``_check_step``) on the shapes of test_gpu_mosi_text_lengths.py
(B = 6, steps (9, 11, 8)), MOSI and MOSEI configs with the method overridden.  Every test but the last constructs an
attention encoder and so fails without the feature.
"""
import numpy as np
import pytest
import torch

import attn_ref as R
import test_gpu_mosi as tm
import test_gpu_mosi_finetune as tf
import test_gpu_mosi_lengths as tl
import test_gpu_mosi_mono as tmm
import test_gpu_mosi_regress as tr
import test_gpu_mosi_text_lengths as tx
import tspm_amd
from oracle import mosi_ref as orc
from parity import Tally, check_adam, check_grad, check_out, pair_from, snapshot
from tspm_amd import _lib as L
from tspm_amd import mosi as M
from tspm_amd.monomodal import FusedMosiMonoStep, MonomodalEncoder, fit_monomodal
from tspm_amd.mosi_data import MOSI, synthetic_mosi_corpus

pytestmark = pytest.mark.gpu
B, STEPS = tx.B, tx.STEPS
FULL = {"audio": [STEPS[0]] * B, "video": [STEPS[1]] * B, "text": [STEPS[2]] * B}
LENS = tl.LENS[0]  # audio (9, 1, 4, 4, 7, 2), video (11, 3, 3, 8, 1, 6)
ATTN = ("attention_vector_weight", "attention_layer.0.weight", "attention_layer.0.bias")
NEW = ("tspm_attn_pool_fwd", "tspm_attn_pool_bwd", "tspm_lstm_bwd_seq")


def _cfg(name):
    return orc.MOSI if name == "mosi" else orc.MOSEI


def _ours(name, norm, seed=3, methods=("attention", "attention"), output_dim=3, clip=None):
    cfg = _cfg(name)
    torch.manual_seed(seed)
    mk = lambda dim, m: M.LSTMEncoder(dim, 64, embd_method=m, **(dict(attention_norm=norm) if m == "attention" else {}))  # noqa: E731
    a, v = mk(cfg.audio_dim, methods[0]), mk(cfg.video_dim, methods[1])
    t = M.TextCNN(input_size=768, embd_size=64, dropout=cfg.text_dropout, in_channels=1, out_channels=128,
                  kernel_heights=[3, 4, 5])
    c = M.FcClassifier(input_dim=192, layers=list(cfg.cls_layers), output_dim=output_dim, dropout=cfg.cls_dropout,
                       use_bn=cfg.use_bn)
    return M.UttFusionModel(a, v, t, c, clip=cfg.clip if clip is None else clip)


def _oracle(name, norm, seed=3, methods=("attention", "attention"), output_dim=3):
    """The oracle model of the same construction order (its values are then overwritten by ours: parity.anchor)."""
    cfg = _cfg(name)

    def build():
        torch.manual_seed(seed)
        mk = lambda dim, m: (R.AttnEncoderRef(dim, 64, "attention", norm) if m == "attention"  # noqa: E731
                             else orc.OracleLSTMEncoder(dim, 64, m))
        a, v = mk(cfg.audio_dim, methods[0]), mk(cfg.video_dim, methods[1])
        t = orc.OracleTextCNN(768, embd_size=64, dropout=cfg.text_dropout, in_channels=1, out_channels=128,
                              kernel_heights=[3, 4, 5])
        c = orc.OracleFcClassifier(192, list(cfg.cls_layers), output_dim, dropout=cfg.cls_dropout, use_bn=cfg.use_bn)
        return orc.OracleUttFusion(a, v, t, c, clip=cfg.clip)
    return build


def _patch(monkeypatch, lengths=None):
    other = tl.LenOracle(lengths) if lengths else orc.lstm_forward
    monkeypatch.setattr(orc, "lstm_forward", R.AttnOracle(other, lengths))
    if lengths:
        monkeypatch.setattr(tm, "_flips", tl._flips_len)


class _Recorder(tf._Recorder):
    """The launch record with each call's first argument (the descriptor count of the LSTM / attention entry points)."""

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("tspm_"):
            return fn

        def call(*args):
            self.calls.append(name)
            self.counts.append((name, args[0] if args else None))
            return fn(*args)
        return call


def _record(monkeypatch):
    rec = _Recorder(L.lib())
    rec.counts = []
    monkeypatch.setattr(L, "lib", lambda: rec)
    return rec


def _attn_params(model):
    return [(f"{net}.{n}", getattr(model, net).get_parameter(n)) for net in ("netA", "netV") for n in ATTN
            if M._is_attention(getattr(model, net))]


# ------------------------------------------------------------------------------------------------
# fused training against fp64, one graph
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", R.NORMS)
@pytest.mark.parametrize("name", ["mosi", "mosei"])
def test_fused_steps_vs_fp64_on_one_graph(gpu, monkeypatch, name, norm):
    """Three fused steps (eager, captured, replayed): logits, loss, every parameter gradient, the clip total, Adam.  "unit":
    the three attention parameters' gradients are exact zeros written every step (the update is then weight decay alone,
    which the Adam check holds them to) and the launch record has no attention backward call."""
    cfg = _cfg(name)
    _patch(monkeypatch)
    ours = _ours(name, norm).to(gpu)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
    rec = _record(monkeypatch)
    st = ours.fused_step(opt, None, B, STEPS)
    assert list(ours._steps) == [(id(opt), id(None), B, M.norm_steps(STEPS))]  # no key element for the method
    assert list(ours._engines) == [] and st.eng.lens is not None and not st.eng.ragged
    tally = Tally()
    for s in range(3):
        A, V, T, y = tx._batch(cfg, FULL, seed=100 + s)
        keeps = orc.keep_masks(B, 50 + s, cfg=cfg)
        o32, o64 = pair_from(ours, _oracle(name, norm))
        before = snapshot(ours, opt if s else None)
        st.keep_override = {k: v.to(gpu) for k, v in keeps.items()}
        for _, p in _attn_params(ours):  # stale values: "unit" must overwrite them with zeros, "time" with gradients
            p.grad.fill_(float("nan"))
        out = st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        if s == 0:  # the eager step's record: both encoders share every new call
            got = {n: [c for m, c in rec.counts if m == n] for n in NEW}
            want_bwd = [2] if norm == "time" else []
            assert got == {"tspm_attn_pool_fwd": [2], "tspm_attn_pool_bwd": want_bwd, "tspm_lstm_bwd_seq": [2]}, got
            assert rec.calls.count("tspm_lstm_fwd_len") == 1 and "tspm_lstm_bwd_len" not in rec.calls
            assert "tspm_lstm_fwd" not in rec.calls and "tspm_lstm_bwd" not in rec.calls
        rep = tm._check_step(ours, st, o32, o64, A, V, T, y, keeps, out, tally)
        coef = float(st.eng.clip_coef.item())
        exp = min(1.0, ours.clip / (st.eng.total_norm.item() + 1e-6))
        assert abs(coef - exp) <= 1e-6 * exp
        tm._check_adam(ours, opt, before, s + 1, coef, cfg)
        if norm == "unit":
            for n, p in _attn_params(ours):
                assert bool((p.grad == 0).all()), n  # exact zeros, not the NaN left there, not None
                assert not torch.equal(p.detach().cpu().double(), before[0][n]) or cfg.weight_decay == 0, n
        print(f"[{name} {norm} step {s + 1}] flips {rep} clip coef {coef:.4f}")
    assert st.graph is not None and st.calls == 3
    print(tally)


@pytest.mark.parametrize("norm", R.NORMS)
def test_graph_replay_is_bitwise_eager(gpu, norm):
    res = []
    for use_graph in (False, True):
        m = _ours("mosei", norm, seed=4).to(gpu)
        opt = tspm_amd.FusedAdam(m.parameters(), lr=1e-3, weight_decay=1e-3)
        st = M.FusedMosiStep(m, opt, None, B, STEPS, use_graph=use_graph, ragged=True)
        for s in range(4):
            A, V, T, y = tl._batch(orc.MOSEI, tl.LENS[s % 3], steps=STEPS, seed=20 + s)
            st.keep_override = {k: v.to(gpu) for k, v in orc.keep_masks(B, 60 + s, cfg=orc.MOSEI).items()}
            st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu), tl._dev_lengths(tl.LENS[s % 3], gpu))
        torch.cuda.synchronize()
        assert (st.graph is not None) == use_graph
        res.append([p.detach().clone() for p in m.parameters()] + [p.grad.clone() for p in m.parameters()] +
                   [b.clone() for b in m.buffers()] + [st.eng.logits.clone(), st.eng.loss.clone()])
    for p, q in zip(*res):
        assert torch.equal(p, q)


# ------------------------------------------------------------------------------------------------
# ragged mode
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", R.NORMS)
def test_ragged_fused_step_vs_fp64_and_padding_independence(gpu, monkeypatch, norm):
    """One ragged step against the oracle under the same lengths; the logits and both embeddings of the same batch
    zero-padded to (12, 14, 8) with the same lengths are bitwise the same."""
    cfg = orc.MOSI
    _patch(monkeypatch, LENS)
    A, V, T, y = tl._batch(cfg, LENS, steps=STEPS, seed=77)
    wide = (12, 14, 8)
    A2, V2 = torch.zeros(B, wide[0], A.shape[2]), torch.zeros(B, wide[1], V.shape[2])
    A2[:, :STEPS[0]], V2[:, :STEPS[1]] = A, V
    keeps = orc.keep_masks(B, 50, cfg=cfg)
    outs = []
    for steps, (a, v) in ((STEPS, (A, V)), (wide, (A2, V2))):
        ours = _ours("mosi", norm).to(gpu)
        opt = tspm_amd.FusedAdam(ours.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
        st = ours.fused_step(opt, None, B, steps, ragged=True)
        o32, o64 = pair_from(ours, _oracle("mosi", norm))
        st.keep_override = {k: m.to(gpu) for k, m in keeps.items()}
        out = st.step(a.to(gpu), v.to(gpu), T.to(gpu), y.to(gpu), tl._dev_lengths(LENS, gpu))
        torch.cuda.synchronize()
        if steps == STEPS:
            print(tm._check_step(ours, st, o32, o64, A, V, T, y, keeps, out, Tally()))
        outs.append((out["logits"].clone(), st.eng.fused.clone(), out["loss"].clone()))
    for x, z in zip(*outs):
        assert torch.equal(x, z)


# ------------------------------------------------------------------------------------------------
# frozen encoder, mixed methods
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", R.NORMS)
def test_frozen_attention_encoder(gpu, monkeypatch, norm):
    """A frozen attention netA beside a trainable attention netV: its parameters are bitwise unchanged, ``.grad is None``,
    no backward problem of its own in the record (the calls carry netV's descriptor only), no backward buffers, and
    the rest meets the oracle with the same flags."""
    cfg = orc.MOSI
    _patch(monkeypatch)
    ours = _ours("mosi", norm).to(gpu)
    ours.netA.requires_grad_(False)
    frozen0 = {n: p.detach().clone() for n, p in ours.netA.named_parameters()}
    opt = tspm_amd.FusedAdam([p for p in ours.parameters() if p.requires_grad], lr=cfg.lr, weight_decay=cfg.weight_decay)
    rec = _record(monkeypatch)
    st = ours.fused_step(opt, None, B, STEPS)
    assert st.frozen == ("audio",) and list(ours._steps)[0][-1] == ("frozen", ("audio",))
    bufs = st.eng.lstm["a"]
    assert bufs["dg"] is None and "dp" not in bufs and "dseq" not in bufs and bufs["alpha"] is not None
    tally = Tally()
    for s in range(2):
        A, V, T, y = tx._batch(cfg, FULL, seed=100 + s)
        keeps = orc.keep_masks(B, 50 + s, cfg=cfg)
        o32, o64 = tf._oracles(ours, ("audio",), _oracle("mosi", norm))
        st.keep_override = {k: v.to(gpu) for k, v in keeps.items()}
        out = st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        tf._check(ours, st, o32, o64, A, V, T, y, keeps, out, tally)
        if s == 0:  # the eager step's record (the capture of the second step makes the same calls again)
            got = {n: [c for m, c in rec.counts if m == n] for n in NEW}
            assert got == {"tspm_attn_pool_fwd": [2], "tspm_attn_pool_bwd": [1] if norm == "time" else [],
                           "tspm_lstm_bwd_seq": [1]}, got
    for n, p in ours.netA.named_parameters():
        assert p.grad is None and torch.equal(p.detach(), frozen0[n]), n
    print(tally)


@pytest.mark.parametrize("methods", [("attention", "maxpool"), ("last", "attention")])
def test_mixed_methods_train_a_step_vs_fp64(gpu, monkeypatch, methods):
    cfg = orc.MOSEI
    _patch(monkeypatch)
    ours = _ours("mosei", "time", methods=methods).to(gpu)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
    rec = _record(monkeypatch)
    st = ours.fused_step(opt, None, B, STEPS)
    A, V, T, y = tx._batch(cfg, FULL, seed=100)
    keeps = orc.keep_masks(B, 50, cfg=cfg)
    o32, o64 = pair_from(ours, _oracle("mosei", "time", methods=methods))
    before = snapshot(ours, None)
    st.keep_override = {k: v.to(gpu) for k, v in keeps.items()}
    out = st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
    torch.cuda.synchronize()
    print(tm._check_step(ours, st, o32, o64, A, V, T, y, keeps, out, Tally()))
    tm._check_adam(ours, opt, before, 1, float(st.eng.clip_coef.item()), cfg)
    got = {n: [c for m, c in rec.counts if m == n] for n in NEW + ("tspm_lstm_fwd_len", "tspm_lstm_bwd_len")}
    assert got == {"tspm_attn_pool_fwd": [1], "tspm_attn_pool_bwd": [1], "tspm_lstm_bwd_seq": [1],
                   "tspm_lstm_fwd_len": [2], "tspm_lstm_bwd_len": [1]}, got


# ------------------------------------------------------------------------------------------------
# the other entry points
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", R.NORMS)
def test_autograd_node_inference_and_validation_paths(gpu, norm):
    cfg = orc.MOSI
    A, V, T, y = tl._batch(cfg, LENS, steps=STEPS, seed=78)
    keeps = {k: v.to(gpu) for k, v in orc.keep_masks(B, 9, cfg=cfg).items()}
    dl = tl._dev_lengths(LENS, gpu)
    fused = _ours("mosi", norm, seed=6).to(gpu)
    opt = tspm_amd.FusedAdam(fused.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
    st = fused.fused_step(opt, None, B, STEPS, ragged=True)
    st.keep_override = keeps
    auto = _ours("mosi", norm, seed=6).to(gpu).train()
    auto._engine(B, STEPS, gpu, True).keep_override = keeps
    logits = auto(A.to(gpu), V.to(gpu), T.to(gpu), lengths=dl)  # the autograd node, before the fused step moves anything
    st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu), dl)
    assert torch.equal(logits, st.eng.logits)
    logits.backward(st.eng.dlogits.clone())  # the fused step's own loss gradient: the same launches on the same inputs
    torch.cuda.synchronize()
    for (n, p), (_, q) in zip(auto.named_parameters(), fused.named_parameters()):
        assert torch.equal(p.grad, q.grad), n
    # train_step reads batch["lengths"]: the cached ragged step
    batch = {"audio": A, "video": V, "text": T, "label": y, "lengths": dl}
    assert np.isfinite(fused.train_step(batch, opt, None, gpu, None)["loss"])
    assert st.calls == 2 and len(fused._steps) == 1
    # inference: the standalone encoder equals the engine's embedding, with and without lengths
    auto.eval()
    for lengths in (dl, None):
        with torch.no_grad():
            ref = auto(A.to(gpu), V.to(gpu), T.to(gpu), lengths=lengths).clone()
        eng = auto._engine(B, STEPS, gpu, lengths is not None)
        assert torch.equal(auto.netA(A.to(gpu), None if lengths is None else dl["audio"]), eng.fused[:, :64])
        assert torch.equal(auto.netV(V.to(gpu), None if lengths is None else dl["video"]), eng.fused[:, 64:128])
        sub = {k: v for k, v in batch.items() if k != "lengths" or lengths is not None}
        out = auto.validation_step(sub, None, gpu, None)
        assert torch.equal(eng.logits, ref)
        assert abs(out["loss"] - float(torch.nn.functional.cross_entropy(ref, y.to(gpu)))) <= 1e-5
        emb = auto.get_embeddings([sub], gpu)
        assert np.array_equal(emb["audio"][0], eng.fused[:, :64].cpu().numpy())
    from tspm_amd.metrics import ClassificationLog
    from tspm_amd.mosi_data import PATTERNS
    ev = M.FusedMosiEvalStep(auto, None, B, STEPS, ClassificationLog(gpu, groups=PATTERNS, classes=3), ragged=True)
    ev.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu), dl)
    with torch.no_grad():
        assert torch.equal(ev.eng.logits, auto(A.to(gpu), V.to(gpu), T.to(gpu), lengths=dl))
    # finetune_param_groups takes the model as it is: the attention parameters are the encoder group's
    groups = M.finetune_param_groups(auto, lr=1e-3, weight_decay=0.0, encoder_lr=1e-4)
    assert {id(p) for p in groups[1]["params"]} >= {id(p) for _, p in _attn_params(auto)}


def test_regression_step_vs_fp64(gpu, monkeypatch):
    cfg = orc.MOSI
    _patch(monkeypatch)
    ours = _ours("mosi", "time", output_dim=1).to(gpu)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
    st = ours.fused_step(opt, tr.Group("l1"), B, STEPS)
    assert st.regress is not None
    A, V, T, _ = tx._batch(cfg, FULL, seed=100)
    y = tr._scores(B, 1)
    keeps = orc.keep_masks(B, 50, cfg=cfg)
    o32, o64 = pair_from(ours, _oracle("mosi", "time", output_dim=1))
    st.keep_override = {k: v.to(gpu) for k, v in keeps.items()}
    out = st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
    torch.cuda.synchronize()
    tally = Tally()
    tr._check_step(ours, st, o32, o64, A, V, T, y, keeps, out, tally, "l1", 1.0)
    print(tally)


@pytest.mark.parametrize("norm", R.NORMS)
def test_monomodal_pretraining_step_vs_fp64_and_its_checkpoint(gpu, monkeypatch, tmp_path, norm):
    _patch(monkeypatch)
    feat, T = 5, 9
    torch.manual_seed(3)
    ours = MonomodalEncoder(M.LSTMEncoder(feat, 64, "attention", attention_norm=norm), 64, 3).to(gpu)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=tmm.LR, weight_decay=tmm.WD)
    x, y = tmm._batch("lstm_last", feat, B, T, 1234)
    st = FusedMosiMonoStep(ours, opt, None, (B, T, feat))
    tally = Tally()
    for s in range(3):  # eager, capture, replay
        o32, o64 = pair_from(ours, lambda: tmm.OracleMono(R.AttnEncoderRef(feat, 64, "attention", norm)))
        before = snapshot(ours, opt if s else None)
        out = st.step(x.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        r32 = tmm._oracle_step(o32, x, y, None, orc.MosiTrace({}))
        r64 = tmm._oracle_step(o64, x.double(), y, None, orc.MosiTrace({}))
        check_out("logits", out["logits"], r32["logits"], r64["logits"], tally)
        check_out("loss", out["loss"], r32["loss"].reshape(1), r64["loss"].reshape(1), tally)
        p32, p64 = dict(o32.named_parameters()), dict(o64.named_parameters())
        for n, p in ours.named_parameters():
            check_grad(f"grad {n}", p.grad, p32[n].grad, p64[n].grad, tally)
        check_adam(ours, opt, *before, s + 1, lr=tmm.LR, wd=tmm.WD)
    assert st.graph is not None
    print(tally)
    # fit_monomodal writes encoder_audio_best.pth; UttFusionModel.netA loads it
    kw = dict(target_modality="audio", selected_patterns=["a"], device=gpu)
    tr_ = MOSI(corpus=synthetic_mosi_corpus(24, seed=5, steps=12), split="train", **kw)
    va = MOSI(corpus=synthetic_mosi_corpus(8, seed=6, steps=12), split="valid", **kw)
    loaders = {"train": tr_.loader(8, shuffle=True, seed=0), "validation": va.loader(8)}
    h = fit_monomodal(ours, opt, None, loaders, 1, experiment_name="MOSI_Audio_Encoder_Pretrain", model_output_path=tmp_path)
    assert np.isfinite(h["metrics_history"]["train"][0]["loss"])
    paths = list(tmp_path.rglob("encoder_audio_best.pth"))
    assert len(paths) == 1
    sd = torch.load(paths[0], map_location="cpu", weights_only=True)
    model = _ours("mosi", norm, seed=9)
    assert list(sd) == list(model.netA.state_dict())
    model.netA.load_state_dict(sd)
    for k, v in ours.encoder.state_dict().items():
        assert torch.equal(model.netA.state_dict()[k], v.cpu()), k


def test_fit_runs_an_epoch_and_best_reloads(gpu, tmp_path):
    from tspm_amd import harness
    torch.manual_seed(8)
    ours = M.build_utt_fusion("mosi", embd_method="attention", attention_norm="time").to(gpu)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=1e-3, weight_decay=1e-3)
    tr_ = MOSI(split="train", corpus=synthetic_mosi_corpus(48, seed=1, steps=12), device=gpu, seed=4)
    va = MOSI(split="valid", corpus=synthetic_mosi_corpus(16, seed=2, steps=12), device=gpu)
    loaders = {"train": tr_.loader(16, shuffle=True, seed=1), "validation": va.loader(16)}
    hist = harness.fit(ours, opt, None, loaders, epochs=1, early_stopping=False, checkpoint_dir=tmp_path / "ck",
                       metrics_path=tmp_path / "m")
    assert np.isfinite(hist["train"][-1]["loss"]) and np.isfinite(hist["validation"][-1]["loss"])
    best = list((tmp_path / "ck").rglob("best.pth"))
    assert len(best) == 1
    sd = torch.load(best[0], map_location="cpu", weights_only=True)["model_state_dict"]
    assert "netA.attention_vector_weight" in sd and "netV.attention_layer.0.weight" in sd
    torch.manual_seed(0)
    again = M.build_utt_fusion("mosi", embd_method="attention", attention_norm="time")
    again.load_state_dict(sd)


# ------------------------------------------------------------------------------------------------
# the off path
# ------------------------------------------------------------------------------------------------
MOSI_CALLS = (["tspm_seq_gather"] * 3 + ["tspm_dropout_mask"] * 2 + ["tspm_linear_fwd"] * 2 + ["tspm_lstm_fwd"] + ["tspm_conv_fwd"] * 3 +
              ["tspm_textcnn_pool_fwd"] + ["tspm_linear_fwd"] * 5 + ["tspm_cross_entropy"] + ["tspm_linear_bwd"] +
              ["tspm_act_bwd", "tspm_linear_bwd"] * 3 + ["tspm_lstm_bwd"] + ["tspm_linear_bwd_weight_splitk"] * 4 +
              ["tspm_act_bwd", "tspm_linear_bwd", "tspm_textcnn_bwd"] +
              ["tspm_grad_clip_coef", "tspm_adam_begin", "tspm_adam_step_clip"])


MOSEI_CALLS = (MOSI_CALLS[:13] + ["tspm_linear_fwd", "tspm_bn1d_fwd_drop"] * 2 + ["tspm_counters_add", "tspm_linear_fwd",
                                                                                    "tspm_cross_entropy", "tspm_linear_bwd"] +
               ["tspm_bn1d_bwd_drop_relu", "tspm_linear_bwd"] * 2 + MOSI_CALLS[25:])


def test_default_models_keep_their_launch_record_and_keys(gpu, monkeypatch):
    """The default models' eager step is the call list recorded on the parent commit: three input gathers and the 33
    launches of the step (two dropout draws, 13 forward, 15 backward, three of the optimizer for MOSI), none of them
    new; the keys carry no new element and neither engine keeps a length buffer."""
    for name in ("mosi", "mosei"):
        cfg = _cfg(name)
        torch.manual_seed(1)
        ours = M.build_utt_fusion(name).to(gpu)
        opt = tspm_amd.FusedAdam(ours.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
        rec = _record(monkeypatch)
        st = ours.fused_step(opt, None, B, STEPS)
        assert list(ours._steps) == [(id(opt), id(None), B, M.norm_steps(STEPS))] and st.eng.lens is None
        A, V, T, y = tx._batch(cfg, FULL, seed=100)
        st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        calls = [c for c in rec.calls if not c.endswith("_workspace")]
        assert not set(calls) & set(NEW) and "tspm_lstm_fwd_len" not in calls
        assert len(MOSI_CALLS) == len(MOSEI_CALLS) == 36 and calls == (MOSI_CALLS if name == "mosi" else MOSEI_CALLS), calls
        with torch.no_grad():
            ours.eval()
            ours(A.to(gpu), V.to(gpu), T.to(gpu))
        assert list(ours._engines) == [(B, M.norm_steps(STEPS), A.to(gpu).device)]
