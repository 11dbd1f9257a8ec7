"""MOSI / MOSEI encoder pre-training on the sentiment score (MonomodalEncoder around mosi.LSTMEncoder / mosi.TextCNN
under a Linear(64, 1) classifier, float32 labels, a single mean L1 term) on the HIP path against the fp64 oracle encoder
+ Linear(64, 1) + L1, under tests/test_gpu_mosi_mono.py's criterion (tests/parity.py); Adam exactly; graph replay =
eager bitwise; and the hand-off of the pre-trained encoder to UttFusionModel."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import tspm_amd
from oracle import mosi_ref as orc
from parity import Tally, check_adam, check_grad, check_out, pair_from, rel_l2, snapshot
from test_gpu_mosi import _flips
from test_gpu_mosi_mono import CASES, _batch, _decisions, _keep, _oracle_forward
from test_gpu_mosi_regress import Group, _scores
from tspm_amd import _lib as L
from tspm_amd import mosi as M
from tspm_amd import msa_metrics as MM
from tspm_amd.metrics import RegressionLog
from tspm_amd.monomodal import FusedMosiMonoEvalStep, FusedMosiMonoStep, MonomodalEncoder, fit_monomodal
from tspm_amd.mosi_data import MOSI, synthetic_mosi_corpus

pytestmark = pytest.mark.gpu
LR, WD = 1e-3, 1e-3
STEP_CASES = [("lstm_last", 5, 3, 5), ("lstm_maxpool", 35, 33, 12), ("textcnn", 768, 6, 5)]


class OracleMono(nn.Module):
    def __init__(self, encoder):
        super().__init__()
        self.encoder = encoder
        self.classifier = nn.Linear(64, 1)


def _ours(kind, feat, dev, seed):
    torch.manual_seed(seed)
    return MonomodalEncoder(CASES[kind][0](feat), 64, 1).to(dev)


def _oracle_step(o, x, y, keep, trace):
    o.train()
    for p in o.parameters():
        p.grad = None
    _, logits = _oracle_forward(o, x, True, keep, trace)
    loss = 0.0 + 1.0 * F.l1_loss(logits.squeeze(-1), y.to(logits.dtype))
    loss.backward()
    return {"logits": logits.detach(), "loss": loss.detach()}


@pytest.mark.parametrize("kind,feat,batch,steps", STEP_CASES)
def test_fused_mono_regression_step_vs_oracle(gpu, kind, feat, batch, steps):
    ours = _ours(kind, feat, gpu, 3)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=LR, weight_decay=WD)
    x, _ = _batch(kind, feat, batch, steps, 1234 + batch)
    y = _scores(batch, 40 + batch)
    st = FusedMosiMonoStep(ours, opt, Group("l1"), (batch, steps, feat))
    assert st.regress == (L.REGRESS_L1, 1.0)
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
        e64 = r64["logits"].squeeze(-1) - y.double()
        assert torch.equal(torch.sign(out["logits"].cpu().squeeze(-1) - y).double(), torch.sign(e64))
        check_out("predictions", out["logits"], r32["logits"], r64["logits"], tally)
        check_out("loss", out["loss"], r32["loss"].reshape(1), r64["loss"].reshape(1), tally)
        assert out["preds"].dtype == torch.float32 and torch.equal(out["preds"], out["logits"].reshape(-1))
        p32, p64 = dict(o32.named_parameters()), dict(o64.named_parameters())
        for n, p in ours.named_parameters():
            check_grad(f"grad {n}", p.grad, p32[n].grad, p64[n].grad, tally)
        check_adam(ours, opt, *before, s + 1, lr=LR, wd=WD)
        print(f"[{kind} B={batch} T={steps} step {s + 1}] flips {rep}")
        assert not rep, f"forced decisions differ from fp64's own: {rep}"
    assert st.graph is not None
    print(tally)


@pytest.mark.parametrize("kind,feat,batch,steps", STEP_CASES)
def test_mono_regression_graph_replay_equals_eager(gpu, kind, feat, batch, steps):
    res = []
    for use_graph in (False, True):
        ours = _ours(kind, feat, gpu, 7)
        opt = tspm_amd.FusedAdam(ours.parameters(), lr=LR, weight_decay=WD)
        x, _ = _batch(kind, feat, batch, steps, 5)
        y = _scores(batch, 8)
        log = RegressionLog(gpu, groups=("m",))
        st = FusedMosiMonoStep(ours, opt, Group("l1"), (batch, steps, feat), use_graph=use_graph, log=log)
        for s in range(4):
            keep = _keep(kind, batch, 90 + s)
            if keep is not None:
                st.keep_override = {"text": keep.to(gpu)}
            st.step(x.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        res.append((torch.cat([p.detach().reshape(-1) for p in ours.parameters()] + [st.loss.reshape(-1)]).cpu(),
                    log.records.cpu(), log.loss_log[:4].cpu(), log.counters.cpu()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert res[0][3].tolist() == [4, 4 * batch]


@pytest.mark.parametrize("kind,feat,batch,steps", STEP_CASES)
def test_mono_regression_eval_step_vs_oracle(gpu, kind, feat, batch, steps):
    ours = _ours(kind, feat, gpu, 4)
    ref = OracleMono(CASES[kind][1](feat))
    ref.load_state_dict({k: v.cpu() for k, v in ours.state_dict().items()})
    ref = ref.double().eval()
    x, _ = _batch(kind, feat, batch, steps, 31)
    y = _scores(batch, 12)
    log = RegressionLog(gpu, groups=("m",))
    st = FusedMosiMonoEvalStep(ours, Group("l1"), (batch, steps, feat), log)
    outs = []
    for _ in range(3):  # eager, capture, replay
        o = st.step(x.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        outs.append((o["loss"].cpu().clone(), o["logits"].cpu().clone()))
    assert all(torch.equal(a[0], outs[0][0]) and torch.equal(a[1], outs[0][1]) for a in outs[1:])
    with torch.no_grad():
        _, logits = _oracle_forward(ref, x.double(), False)
        loss = F.l1_loss(logits.squeeze(-1), y.double())
    check_out("eval predictions", outs[0][1], None, logits)
    assert abs(outs[0][0].item() - loss.item()) <= 1e-4 * abs(loss.item())
    recs, losses, samples = log.fetch()
    want = MM.regression_record(np.tile(outs[0][1].numpy().reshape(-1), 3), np.tile(y.numpy(), 3))
    assert samples == 3 * batch and recs[0]["n"] == 3 * batch and np.array_equal(recs[0]["conf7"], want["conf7"])
    assert losses.tolist() == [outs[0][0].item()] * 3


def test_train_and_validation_step_api_in_regression_mode(gpu):
    """The reference's call signatures on the fused (FusedAdam) and autograd (torch.optim.Adam) paths: no accuracy in
    the returned metrics, float predictions to the recorder, both paths train the encoder and agree."""
    kind, feat, key = "lstm_last", 5, "audio"
    x, _ = _batch(kind, feat, 16, 9, 77)
    y = _scores(16, 3)
    cfg = SimpleNamespace(experiment=SimpleNamespace(name="MOSI_Audio_Encoder_Pretrain"))
    batch = {key: x, "label": y.reshape(-1, 1), "pattern_name": ["a"] * 16}
    group = Group("l1")
    results = {}
    for path in ("fused", "autograd"):
        ours = _ours(kind, feat, gpu, 11)
        opt = (tspm_amd.FusedAdam(ours.parameters(), lr=LR, weight_decay=WD) if path == "fused"
               else torch.optim.Adam(ours.parameters(), lr=LR, weight_decay=WD))
        calls = []
        rec = SimpleNamespace(config=SimpleNamespace(groups={"regression": ["MSA"]}),
                              update_group=lambda group_name, predictions, targets, modality:
                              calls.append((group_name, modality, predictions.detach().cpu().clone())))
        before = {n: p.detach().cpu().clone() for n, p in ours.named_parameters()}
        ours.train()
        r = ours.train_step(batch, opt, group, gpu, rec, cfg)
        torch.cuda.synchronize()
        assert set(r) == {"loss", "metrics"} and set(r["metrics"]) == {"loss"}
        assert calls[0][:2] == ("regression", key) and calls[0][2].dtype == torch.float32
        assert (path == "fused") == (ours._fused is not None)
        for n, p in ours.named_parameters():
            assert not torch.equal(p.detach().cpu(), before[n]), f"{path}: {n} did not change"
        ours.eval()
        v = ours.validation_step(batch, group, gpu, rec, cfg)
        assert set(v["metrics"]) == {"loss"}
        results[path] = (r, v, torch.cat([p.detach().reshape(-1) for p in ours.parameters()]).cpu())
    assert abs(results["fused"][0]["loss"] - results["autograd"][0]["loss"]) <= 1e-5 * abs(results["fused"][0]["loss"])
    assert rel_l2(results["fused"][2], results["autograd"][2]) < 1e-4
    assert abs(results["fused"][1]["loss"] - results["autograd"][1]["loss"]) <= 1e-4 * abs(results["fused"][1]["loss"])


def test_fit_monomodal_on_regression_labels_hands_the_encoder_to_utt_fusion(gpu, tmp_path):
    ours = _ours("lstm_last", 5, gpu, 0)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=LR, weight_decay=WD)
    group = Group("l1")
    tr = MOSI(corpus=synthetic_mosi_corpus(96, seed=5, steps=12, regression=True), split="train",
              target_modality="audio", selected_patterns=["a"], device=gpu, labels_key="regression_labels")
    va = MOSI(corpus=synthetic_mosi_corpus(40, seed=6, steps=12, regression=True), split="valid",
              target_modality="audio", selected_patterns=["a"], device=gpu, labels_key="regression_labels")
    loaders = {"train": tr.loader(32, shuffle=True, seed=0), "validation": va.loader(32), "test": va.loader(32)}
    w0 = ours.encoder.rnn.weight_hh_l0.detach().cpu().clone()
    with pytest.raises(ValueError):
        fit_monomodal(ours, opt, group, loaders, 1, experiment_name="MOSI_Audio_Encoder_Pretrain",
                      save_metric="accuracy")
    h = fit_monomodal(ours, opt, group, loaders, 2, experiment_name="MOSI_Audio_Encoder_Pretrain",
                      model_output_path=tmp_path)
    tr0, va0 = h["metrics_history"]["train"][0], h["metrics_history"]["validation"][0]
    assert len(h["metrics_history"]["train"]) == 2 and "accuracy" not in tr0 and "accuracy" not in va0
    assert [k for k in va0 if k != "loss"] == [f"MSA_{k}_AUDIO" for k in MM.REGRESSION_KEYS]
    assert all(np.isfinite(e["loss"]) for e in h["metrics_history"]["train"]) and "loss" in h["metrics_history"]["test"]
    assert not torch.equal(ours.encoder.rnn.weight_hh_l0.detach().cpu(), w0)
    assert loaders["train"].step_for is not None and len(ours._by_buffer) >= 2
    # the validation MAE is the L1 loss of the epoch's rows (40 rows: batches of 32 and 8)
    st = ours._eval_step_of(torch.zeros(32, 12, 5, device=gpu), group, None)
    assert isinstance(st, FusedMosiMonoEvalStep) and st.regress is not None
    assert (tmp_path / "encoder_audio_best.pth").exists() and (tmp_path / "best.pth").exists()
    enc_sd = torch.load(tmp_path / "encoder_audio_best.pth", weights_only=True)
    torch.manual_seed(1)
    fusion = M.build_utt_fusion("mosi", output_dim=1)
    fusion.netA.load_state_dict(enc_sd, strict=True)
    assert list(enc_sd) == list(fusion.netA.state_dict())
    fusion = fusion.to(gpu).eval()
    A, V, T, _ = orc.synthetic_batch(8, 12, seed=9)
    eng = fusion._engine(8, 12, gpu)
    eng.load(A.to(gpu), V.to(gpu), T.to(gpu))
    eng.forward(L.stream_handle(), False)
    torch.cuda.synchronize()
    assert torch.equal(ours.encoder(A.to(gpu)), eng.fused[:, :64])
