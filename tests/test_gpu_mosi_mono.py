"""MOSI / MOSEI encoder pre-training (MonomodalEncoder around mosi.LSTMEncoder / mosi.TextCNN) on the HIP path
against the CPU oracle's encoders (oracle/mosi_ref.py) under a Linear(64, 3) classifier.

Criterion as tests/test_gpu_mono.py and tests/test_gpu_mosi.py (tests/parity.py): the oracle in fp64 with our
decisions forced into it — the "maxpool" LSTM's time argmax, the TextCNN's time-max argmax and the ReLU at it, the
embedding ReLU mask, the dropout mask — is the truth; every forced decision that differs from fp64's own must be a
near-tie (and rare); logits / loss rel-L2 <= 1e-4, every gradient rel-L2 <= 1e-3 and cosine >= 0.9999 and within
4x the fp32 reference's error on the same decisions; Adam exactly; every step checked from our own state."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import tspm_amd
from oracle import mosi_ref as orc
from parity import Tally, check_adam, check_grad, check_out, pair_from, rel_l2, snapshot
from test_gpu_mono import _clear
from test_gpu_mosi import _flips
from tspm_amd import _lib as L
from tspm_amd import mosi as M
from tspm_amd.monomodal import FusedMosiMonoEvalStep, FusedMosiMonoStep, MonomodalEncoder, fit_monomodal
from tspm_amd.mosi_data import MOSI, synthetic_mosi_corpus

pytestmark = pytest.mark.gpu
LR, WD = 1e-3, 1e-3  # the caller's optimizer arguments (the mosi/mono YAMLs set them; none is built in)
CASES = {  # kind -> (encoder factory, oracle encoder factory, input scale)
    "lstm_last": (lambda f: M.LSTMEncoder(f, 64, "last"), lambda f: orc.OracleLSTMEncoder(f, 64, "last"), 1.0),
    "lstm_maxpool": (lambda f: M.LSTMEncoder(f, 64, "maxpool"), lambda f: orc.OracleLSTMEncoder(f, 64, "maxpool"), 0.5),
    "textcnn": (lambda f: M.TextCNN(f, 64, dropout=0.5), lambda f: orc.OracleTextCNN(f, embd_size=64, dropout=0.5), 0.3),
}


class OracleMono(nn.Module):
    """train_monomodal.MonomodalEncoder's two attributes around an oracle MOSI encoder."""

    def __init__(self, encoder):
        super().__init__()
        self.encoder = encoder
        self.classifier = nn.Linear(64, 3)


def _oracle_forward(o, x, training, keep=None, trace=None):
    if isinstance(o.encoder, orc.OracleTextCNN):
        emb = orc.textcnn_forward(o.encoder, x, training, keep, trace)
    else:
        emb = orc.lstm_forward(o.encoder, x, trace, "lstm.a.pool")
    return emb, o.classifier(emb)


def _oracle_step(o, x, y, keep, trace):
    """MonomodalEncoder.train_step up to the optimizer (oracle/monomodal_ref.py: CE * 1.0, no clip)."""
    o.train()
    for p in o.parameters():
        p.grad = None
    _, logits = _oracle_forward(o, x, True, keep, trace)
    loss = 0.0 + 1.0 * F.cross_entropy(logits, y)
    loss.backward()
    return {"logits": logits.detach(), "loss": loss.detach(), "preds": logits.detach().argmax(1)}


def _ours(kind, feat, dev, seed, fused_head=True):
    torch.manual_seed(seed)
    return MonomodalEncoder(CASES[kind][0](feat), 64, 3, fused_head=fused_head).to(dev)


def _batch(kind, feat, b, t, seed):
    g = torch.Generator().manual_seed(seed)
    x = CASES[kind][2] * torch.randn(b, t, feat, generator=g)
    return x, torch.randint(0, 3, (b,), generator=g)


def _keep(kind, b, seed):
    if kind != "textcnn":
        return None
    return (torch.rand(b, 384, generator=torch.Generator().manual_seed(seed)) >= 0.5).to(torch.uint8)


def _decisions(eng):
    d = {}
    if eng.is_text:
        C = eng.C
        for i in range(3):
            d[f"text.pool{i}"] = eng.argmax[:, i * C:(i + 1) * C].long().cpu()
            d[f"text.relu{i}"] = (eng.pooled[:, i * C:(i + 1) * C] > 0).cpu()
        d["text.embd"] = (eng.emb > 0).cpu()
    elif eng.bufs["arg"] is not None:
        d["lstm.a.pool"] = eng.bufs["arg"].long().cpu()
    return d


STEP_CASES = [("lstm_last", 5, 3, 5), ("lstm_last", 5, 128, 50), ("lstm_maxpool", 35, 33, 12),
              ("textcnn", 768, 6, 5), ("textcnn", 768, 64, 8)]


@pytest.mark.parametrize("kind,feat,batch,steps", STEP_CASES)
def test_fused_mosi_mono_step_vs_oracle(gpu, kind, feat, batch, steps):
    ours = _ours(kind, feat, gpu, 3)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=LR, weight_decay=WD)
    x, y = _batch(kind, feat, batch, steps, 1234 + batch)
    st = FusedMosiMonoStep(ours, opt, None, (batch, steps, feat))
    assert st.fused_head
    tally = Tally()
    for s in range(3):  # eager, capture, replay
        keep = _keep(kind, batch, 50 + s)
        o32, o64 = pair_from(ours, lambda: OracleMono(CASES[kind][1](feat)))
        before = snapshot(ours, opt if s else None)
        if keep is not None:
            st.keep_override = {"text": keep.to(gpu)}
        out = st.step(x.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        forced = _decisions(st.eng)
        t32, t64 = orc.MosiTrace(forced), orc.MosiTrace(forced)
        r32 = _oracle_step(o32, x, y, keep, t32)
        r64 = _oracle_step(o64, x.double(), y, keep, t64)
        rep = _flips(t64, forced, {})
        check_out("logits", out["logits"], r32["logits"], r64["logits"], tally)
        check_out("loss", out["loss"], r32["loss"].reshape(1), r64["loss"].reshape(1), tally)
        p32, p64 = dict(o32.named_parameters()), dict(o64.named_parameters())
        for n, p in ours.named_parameters():
            check_grad(f"grad {n}", p.grad, p32[n].grad, p64[n].grad, tally)
        if kind != "textcnn":  # the same column sums of the gate gradients (as in ATen): bitwise
            assert torch.equal(ours.encoder.rnn.bias_ih_l0.grad, ours.encoder.rnn.bias_hh_l0.grad)
        check_adam(ours, opt, *before, s + 1, lr=LR, wd=WD)
        clear = _clear(r64["logits"])
        assert torch.equal(out["preds"].cpu()[clear], r64["preds"][clear])
        print(f"[{kind} B={batch} T={steps} step {s + 1}] flips {rep}")
    assert st.graph is not None
    print(tally)


@pytest.mark.parametrize("fused_head", [True, False])
@pytest.mark.parametrize("kind,feat,batch,steps", [("lstm_maxpool", 35, 33, 12), ("textcnn", 768, 64, 8)])
def test_mosi_mono_graph_replay_equals_eager(gpu, kind, feat, batch, steps, fused_head):
    res = []
    for use_graph in (False, True):
        ours = _ours(kind, feat, gpu, 7, fused_head)
        opt = tspm_amd.FusedAdam(ours.parameters(), lr=LR, weight_decay=WD)
        x, y = _batch(kind, feat, batch, steps, 5)
        st = FusedMosiMonoStep(ours, opt, None, (batch, steps, feat), use_graph=use_graph)
        for s in range(4):
            keep = _keep(kind, batch, 90 + s)
            if keep is not None:
                st.keep_override = {"text": keep.to(gpu)}
            st.step(x.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        res.append(torch.cat([p.detach().reshape(-1) for p in ours.parameters()] + [st.loss.reshape(-1)]).cpu())
    assert torch.equal(res[0], res[1])


@pytest.mark.parametrize("kind,feat,batch,steps", [("lstm_last", 5, 128, 50), ("lstm_maxpool", 35, 33, 12),
                                                   ("textcnn", 768, 64, 8)])
def test_fused_head_and_separate_launches_agree(gpu, kind, feat, batch, steps):
    """fused_head=True (tspm_mono_head_step) against False (linear_fwd, cross_entropy, classify_update_ex,
    linear_bwd): the same loss, parameters within Adam's sign-amplified rounding, the same predictions."""
    got = {}
    for fh in (True, False):
        ours = _ours(kind, feat, gpu, 11, fh)
        opt = tspm_amd.FusedAdam(ours.parameters(), lr=LR, weight_decay=WD)
        x, y = _batch(kind, feat, batch, steps, 77)
        st = FusedMosiMonoStep(ours, opt, None, (batch, steps, feat))
        assert st.fused_head is fh
        keep = _keep(kind, batch, 3)
        if keep is not None:
            st.keep_override = {"text": keep.to(gpu)}
        out = st.step(x.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        got[fh] = (out["loss"].item(), torch.cat([p.detach().reshape(-1) for p in ours.parameters()]).cpu(),
                   out["logits"].cpu().clone(), out["preds"].cpu().clone())
    assert abs(got[True][0] - got[False][0]) <= 1e-6 * abs(got[False][0])
    assert rel_l2(got[True][1], got[False][1]) < 1e-4
    clear = _clear(got[False][2].double())
    assert torch.equal(got[True][3][clear], got[False][3][clear])


@pytest.mark.parametrize("fused_head", [True, False])
@pytest.mark.parametrize("kind,feat,batch,steps", [("lstm_last", 5, 33, 12), ("lstm_maxpool", 35, 33, 12),
                                                   ("textcnn", 768, 6, 5)])
def test_mosi_mono_eval_step_vs_oracle(gpu, kind, feat, batch, steps, fused_head):
    ours = _ours(kind, feat, gpu, 4, fused_head)
    ref = OracleMono(CASES[kind][1](feat))
    ref.load_state_dict({k: v.cpu() for k, v in ours.state_dict().items()})
    x, y = _batch(kind, feat, batch, steps, 31)
    st = FusedMosiMonoEvalStep(ours, None, (batch, steps, feat))
    outs = []
    for _ in range(3):  # eager, capture, replay
        o = st.step(x.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        outs.append((o["loss"].cpu().clone(), o["logits"].cpu().clone(), o["preds"].cpu().clone()))
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(o, outs[0]))
    with torch.no_grad():
        ref.eval()
        _, logits = _oracle_forward(ref, x, False)
        loss = F.cross_entropy(logits, y)
    assert rel_l2(outs[0][1], logits) < 1e-4
    assert abs(outs[0][0].item() - loss.item()) <= 1e-4 * abs(loss.item())
    clear = _clear(logits.double())
    assert torch.equal(outs[0][2][clear], logits.argmax(1)[clear])


class _Rec:
    def __init__(self):
        self.config = SimpleNamespace(groups={"classification": ["accuracy"]})
        self.calls = []

    def update_group(self, group_name, predictions, targets, modality):
        self.calls.append((group_name, modality, predictions.detach().cpu().numpy().copy()))


@pytest.mark.parametrize("kind,feat,key", [("lstm_last", 5, "audio"), ("lstm_maxpool", 35, "video"),
                                           ("textcnn", 768, "text")])
def test_train_and_validation_step_api(gpu, kind, feat, key):
    """The reference's call signatures and return dicts on the fused (FusedAdam) and autograd (torch.optim.Adam)
    paths; on the autograd path the ENCODER must train too (one autograd node over encoder + classifier)."""
    x, y = _batch(kind, feat, 16, 9, 77)
    cfg = SimpleNamespace(experiment=SimpleNamespace(name=f"MOSI_{key.capitalize()}_Encoder_Pretrain"))
    batch = {key: x, "label": y, "pattern_name": [key[0]] * 16}
    results = {}
    for path in ("fused", "autograd"):
        ours = _ours(kind, feat, gpu, 11)
        if kind == "textcnn":
            ours.encoder.dropout.p = 0.0  # no dropout: the two paths are compared
        opt = (tspm_amd.FusedAdam(ours.parameters(), lr=LR, weight_decay=WD) if path == "fused"
               else torch.optim.Adam(ours.parameters(), lr=LR, weight_decay=WD))
        loss_fns = None if path == "fused" else (lambda lg, lb: {"total_loss": F.cross_entropy(lg, lb)})
        before = {n: p.detach().cpu().clone() for n, p in ours.named_parameters()}
        rec = _Rec()
        ours.train()
        r = ours.train_step(batch, opt, loss_fns, gpu, rec, cfg)
        torch.cuda.synchronize()
        assert set(r) == {"loss", "metrics"} and set(r["metrics"]) == {"loss", "accuracy"}
        assert rec.calls[0][:2] == ("classification", key)
        assert (path == "fused") == (ours._fused is not None)
        for n, p in ours.named_parameters():  # every tensor moved: encoder as well as classifier
            assert not torch.equal(p.detach().cpu(), before[n]), f"{path}: {n} did not change"
        ours.eval()
        v = ours.validation_step(batch, loss_fns, gpu, rec, cfg)
        assert set(v) == {"loss", "metrics"} and rec.calls[-1][:2] == ("classification", key)
        results[path] = (r, v, torch.cat([p.detach().reshape(-1) for p in ours.parameters()]).cpu())
    o = OracleMono(CASES[kind][1](feat))
    torch.manual_seed(11)
    o.load_state_dict(_ours(kind, feat, "cpu", 11).state_dict())
    if kind == "textcnn":
        o.encoder.p = 0.0
    r32 = _oracle_step(o, x, y, None, None)
    for path, (r, v, _) in results.items():
        assert abs(r["loss"] - r32["loss"].item()) <= 1e-4 * abs(r32["loss"].item()), path
    assert abs(results["fused"][0]["loss"] - results["autograd"][0]["loss"]) <= 1e-6
    assert rel_l2(results["fused"][2], results["autograd"][2]) < 1e-4
    assert abs(results["fused"][1]["loss"] - results["autograd"][1]["loss"]) <= 1e-4 * abs(results["fused"][1]["loss"])


def test_autograd_path_draws_fresh_textcnn_masks(gpu):
    ours = _ours("textcnn", 768, gpu, 2).train()
    x, _ = _batch("textcnn", 768, 16, 6, 5)
    masks = []
    for _ in range(2):
        ours(x.to(gpu)).sum().backward()
        masks.append(ours._mosi_engine(16, 6, gpu).keep.clone())
    torch.cuda.synchronize()
    assert not torch.equal(masks[0], masks[1])
    assert abs(masks[0].float().mean().item() - 0.5) < 0.05
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in ours.parameters())


def test_fused_step_draws_fresh_textcnn_masks(gpu):
    ours = _ours("textcnn", 768, gpu, 2)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=LR, weight_decay=WD)
    x, y = _batch("textcnn", 768, 64, 8, 5)
    st = FusedMosiMonoStep(ours, opt, None, (64, 8, 768))
    masks = []
    for _ in range(3):
        st.step(x.to(gpu), y.to(gpu))
        masks.append(st.eng.keep.clone())
    torch.cuda.synchronize()
    assert not torch.equal(masks[0], masks[1]) and not torch.equal(masks[1], masks[2])
    assert all(abs(m.float().mean().item() - 0.5) < 0.03 for m in masks)


def test_textcnn_standalone_forward_equals_the_fusion_model_columns(gpu):
    torch.manual_seed(5)
    fusion = M.build_utt_fusion("mosi").to(gpu).eval()
    A, V, T, _ = orc.synthetic_batch(6, 9, seed=3)
    eng = fusion._engine(6, 9, gpu)
    eng.load(A.to(gpu), V.to(gpu), T.to(gpu))
    eng.forward(L.stream_handle(), False)
    with torch.no_grad():
        emb = fusion.netT(T.to(gpu))
    torch.cuda.synchronize()
    assert torch.equal(emb, eng.fused[:, 128:])
    with pytest.raises(L.TspmError):
        fusion.netT(T)  # a CPU tensor: the device-only rule


@pytest.mark.parametrize("m", ["audio", "video", "text"])
def test_single_modality_batches(gpu, m):
    corpus = synthetic_mosi_corpus(24, seed=2, steps=7)
    ds = MOSI(corpus=corpus, split="train", target_modality=m, selected_patterns=[m[0]], device=gpu)
    feat = corpus.feat[m]
    b = ds.collate_fn([ds.__getitems__(list(range(8)))[0]])
    assert list(b) == [m, "label", "pattern_name"] and tuple(b[m].shape) == (8, 7, feat)
    dense = torch.from_numpy(corpus.data[m]).reshape(24, 7, feat)
    assert torch.equal(b[m].cpu(), dense[:8]) and torch.equal(b["label"].cpu(), torch.from_numpy(corpus.labels[:8]))
    # gathered time-major straight into a step's input buffer
    enc = M.TextCNN(feat, 64) if m == "text" else M.LSTMEncoder(feat, 64)
    model = MonomodalEncoder(enc, 64, 3).to(gpu)
    st = FusedMosiMonoEvalStep(model, None, (8, 7, feat))
    for got in ds.device_loader(8, step_for=lambda bb, tt: st):
        assert list(got) == [m, "label", "pattern_name"] and got[m].data_ptr() == st.X.data_ptr()
        break
    assert torch.equal(st.X.cpu(), dense[:8].transpose(0, 1)) and torch.equal(st.labels.cpu(), b["label"].cpu())
    # valid split, single modality: flat batches (no per-pattern dict)
    va = MOSI(corpus=corpus, split="valid", target_modality=m, selected_patterns=[m[0]], device=gpu)
    assert list(next(iter(va.device_loader(8)))) == [m, "label", "pattern_name"]


def test_fit_monomodal_hands_encoder_to_utt_fusion(gpu, tmp_path):
    ours = _ours("lstm_last", 5, gpu, 0)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=LR, weight_decay=WD)
    tr = MOSI(corpus=synthetic_mosi_corpus(96, seed=5, steps=12), split="train", target_modality="audio",
              selected_patterns=["a"], device=gpu)
    va = MOSI(corpus=synthetic_mosi_corpus(40, seed=6, steps=12), split="valid", target_modality="audio",
              selected_patterns=["a"], device=gpu)
    loaders = {"train": tr.loader(32, shuffle=True, seed=0), "validation": va.loader(32), "test": va.loader(32)}
    w0 = ours.encoder.rnn.weight_hh_l0.detach().cpu().clone()
    h = fit_monomodal(ours, opt, None, loaders, 2, experiment_name="MOSI_Audio_Encoder_Pretrain",
                      model_output_path=tmp_path)
    assert len(h["metrics_history"]["train"]) == 2 and {"loss", "accuracy"} <= set(h["metrics_history"]["train"][0])
    assert {"loss", "accuracy"} <= set(h["metrics_history"]["validation"][0]) and "loss" in h["metrics_history"]["test"]
    assert all(np.isfinite(e["loss"]) for e in h["metrics_history"]["train"])
    assert not torch.equal(ours.encoder.rnn.weight_hh_l0.detach().cpu(), w0)
    # the loader gathered into the steps' own buffers (no batch copy): one train step for the one shape
    assert loaders["train"].step_for is not None and len(ours._by_buffer) >= 2
    assert h["encoder_path"] and (tmp_path / "encoder_audio_best.pth").exists() and (tmp_path / "best.pth").exists()
    enc_sd = torch.load(tmp_path / "encoder_audio_best.pth", weights_only=True)
    torch.manual_seed(1)
    fusion = M.build_utt_fusion("mosi")
    fusion.netA.load_state_dict(enc_sd)
    assert list(enc_sd) == list(fusion.netA.state_dict())
    fusion = fusion.to(gpu).eval()
    A, V, T, _ = orc.synthetic_batch(8, 12, seed=9)
    eng = fusion._engine(8, 12, gpu)
    eng.load(A.to(gpu), V.to(gpu), T.to(gpu))
    eng.forward(L.stream_handle(), False)
    mono = MonomodalEncoder(M.LSTMEncoder(5, 64), 64, 3)
    mono.encoder.load_state_dict(enc_sd)
    mono = mono.to(gpu).eval()
    est = FusedMosiMonoEvalStep(mono, None, (8, 12, 5))
    est.step(A.to(gpu), torch.zeros(8, dtype=torch.int64, device=gpu))
    torch.cuda.synchronize()
    assert torch.equal(est.emb, eng.fused[:, :64])
    assert torch.equal(mono.encoder(A.to(gpu)), eng.fused[:, :64])
