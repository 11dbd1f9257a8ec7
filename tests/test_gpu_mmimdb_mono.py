"""MMIMDb encoder pre-training (MonomodalEncoder around mmimdb.MMIMDbModalityEncoder) on the HIP path against the CPU
oracle's encoder (oracle.mmimdb_ref.OracleEncoder) under a Linear(out, classes) classifier and bce_loss.

Criterion as tests/test_gpu_mosi_mono.py and tests/test_gpu_mmimdb.py (tests/parity.py): the oracle in fp64 is the
truth and its fp32 run the yardstick; logits / loss rel-L2 <= 1e-4, every gradient rel-L2 <= 1e-3 and cosine >=
0.9999 and within 4x the fp32 reference's error, BatchNorm running statistics rel-L2 <= 1e-3; Adam exactly; every
step checked from our own state.  This path has no ReLU, max or dropout, so no decision is forced."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import tspm_amd
from oracle import mmimdb_ref as orc
from parity import GRAD_REL, Tally, check_adam, check_grad, check_out, pair_from, snapshot
from test_mmimdb_cpu import dropin
from tspm_amd import _lib as L
from tspm_amd import mmimdb as M
from tspm_amd.monomodal import (FusedMMIMDbMonoEvalStep, FusedMMIMDbMonoStep, MonomodalEncoder, fit_monomodal)

pytestmark = pytest.mark.gpu
LR, WD = 1e-3, 1e-3  # the caller's optimizer arguments (none is built in)
STEP_CASES = [(300, 512, 23, 33), (4096, 512, 23, 128), (20, 8, 3, 2), (300, 512, 23, 3)]  # (in, out, classes, n)


class OracleMono(nn.Module):
    """train_monomodal.MonomodalEncoder's two attributes around the oracle's MMIMDb encoder."""

    def __init__(self, fin, out, classes):
        super().__init__()
        self.encoder = orc.OracleEncoder(fin, out)
        self.classifier = nn.Linear(out, classes)

    def forward(self, x):
        return self.classifier(self.encoder(x))


def _oracle_step(o, x, y):
    """MonomodalEncoder.train_step up to the optimizer: zero_grad, forward (training-mode BatchNorm), BCE, backward."""
    o.train()
    for p in o.parameters():
        p.grad = None
    logits = o(x)
    loss = orc.bce_loss(logits, y)
    loss.backward()
    return {"logits": logits.detach(), "loss": loss.detach().reshape(1)}


def _ours(fin, out, classes, dev, seed, fused_head=True):
    torch.manual_seed(seed)
    return MonomodalEncoder(M.MMIMDbModalityEncoder(fin, out), out, classes, fused_head=fused_head).to(dev)


_FEATURES = {}


def _batch(fin, classes, n):
    """mmimdb.synthetic_features, sliced: the image features for a wide input, the text features otherwise."""
    if "f" not in _FEATURES:
        _FEATURES["f"] = M.synthetic_features(128, seed=77)
    image, text, labels = _FEATURES["f"]
    src = image if fin > text.shape[1] else text
    return src[:n, :fin].contiguous(), labels[:n, :classes].contiguous()


def _check_step(name, ours, out, o32, o64, x, y, tally):
    r32, r64 = _oracle_step(o32, x, y), _oracle_step(o64, x.double(), y.double())
    check_out(f"logits {name}", out["logits"], r32["logits"], r64["logits"], tally)
    check_out(f"loss {name}", out["loss"], r32["loss"], r64["loss"], tally)
    p32, p64 = dict(o32.named_parameters()), dict(o64.named_parameters())
    for pname, p in ours.named_parameters():
        check_grad(f"grad {pname} {name}", p.grad, p32[pname].grad, p64[pname].grad, tally)
    s32, s64 = o32.state_dict(), o64.state_dict()
    for k, v in ours.state_dict().items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            check_out(f"{k} {name}", v, s32[k], s64[k], tally, bound=GRAD_REL)
        elif k.endswith("num_batches_tracked"):
            assert int(v) == int(s64[k]), k
    cut = (r64["logits"].abs() > 1e-3)
    assert torch.equal(out["preds"].cpu()[cut], (r64["logits"] > 0)[cut])


def _run_three_steps(gpu, fin, out_dim, classes, n, fused_head):
    ours = _ours(fin, out_dim, classes, gpu, 3, fused_head)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=LR, weight_decay=WD)
    x, y = _batch(fin, classes, n)
    st = FusedMMIMDbMonoStep(ours, opt, None, (n, fin))
    assert st.fused_head is fused_head
    tally = Tally()
    for s in range(3):  # eager, capture, replay
        o32, o64 = pair_from(ours, lambda: OracleMono(fin, out_dim, classes))
        before = snapshot(ours, opt if s else None)
        out = st.step(x.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        _check_step(f"s{s}", ours, out, o32, o64, x, y, tally)
        check_adam(ours, opt, *before, s + 1, lr=LR, wd=WD)
    assert st.graph is not None
    assert int(ours.encoder.net[0].num_batches_tracked) == 3
    print(f"[in={fin} out={out_dim} classes={classes} n={n} fused_head={fused_head}] {tally}")


@pytest.mark.parametrize("fin,out_dim,classes,n", STEP_CASES)
def test_fused_mmimdb_mono_step_vs_oracle(gpu, fin, out_dim, classes, n):
    _run_three_steps(gpu, fin, out_dim, classes, n, True)


def test_separate_launch_head_is_held_to_the_same_checks(gpu):
    _run_three_steps(gpu, 300, 512, 23, 33, False)


@pytest.mark.parametrize("fused_head", [True, False])
@pytest.mark.parametrize("fin,n", [(300, 33), (4096, 128)])
def test_mmimdb_mono_graph_replay_equals_eager(gpu, fin, n, fused_head):
    res = []
    for use_graph in (False, True):
        ours = _ours(fin, 512, 23, gpu, 7, fused_head)
        opt = tspm_amd.FusedAdam(ours.parameters(), lr=LR, weight_decay=WD)
        x, y = _batch(fin, 23, n)
        st = FusedMMIMDbMonoStep(ours, opt, None, (n, fin), use_graph=use_graph)
        for _ in range(4):
            st.step(x.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        assert (st.graph is not None) == use_graph
        res.append(torch.cat([p.detach().reshape(-1) for p in ours.parameters()] +
                             [st.loss.reshape(-1), st.stats.reshape(-1)]).cpu())
    assert torch.equal(res[0], res[1])


def _randomise_running_stats(bn, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        bn.running_mean.copy_(0.1 * torch.randn(bn.num_features, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(bn.num_features, generator=g))


@pytest.mark.parametrize("fused_head", [True, False])
@pytest.mark.parametrize("fin,n", [(300, 33), (4096, 128), (300, 1)])
def test_mmimdb_mono_eval_step_vs_fp64(gpu, fin, n, fused_head):
    ours = _ours(fin, 512, 23, gpu, 4, fused_head)
    _randomise_running_stats(ours.encoder.net[0], 9)
    o32, o64 = pair_from(ours, lambda: OracleMono(fin, 512, 23))
    x, y = _batch(fin, 23, n)
    st = FusedMMIMDbMonoEvalStep(ours, None, (n, fin))
    assert st.fused_head is fused_head
    outs = []
    for _ in range(3):  # eager, capture, replay
        o = st.step(x.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        outs.append((o["loss"].cpu().clone(), o["logits"].cpu().clone(), o["preds"].cpu().clone()))
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(o, outs[0]))
    with torch.no_grad():
        l32, l64 = o32.eval()(x), o64.eval()(x.double())
        check_out("eval logits", outs[0][1], l32, l64)
        check_out("eval loss", outs[0][0], orc.bce_loss(l32, y).reshape(1), orc.bce_loss(l64, y.double()).reshape(1))
    cut = l64.abs() > 1e-3
    assert torch.equal(outs[0][2][cut], (l64 > 0)[cut])
    # three launches accumulated the counts of the kernel's own predictions
    p, t = outs[0][2], y > 0.5
    counts = torch.stack([(p & t).sum(0), (p & ~t).sum(0), (~p & t).sum(0)], 1).reshape(-1).float()
    assert torch.equal(st.stats.cpu()[3:], 3 * counts) and st.stats[1].item() == 3.0 * n
    if not fused_head:
        return
    # the forward-only head is bitwise the training head on the same embedding
    cls = ours.classifier
    f32 = dict(device=gpu, dtype=torch.float32)
    logits, loss, preds = torch.zeros(n, 23, **f32), torch.zeros(1, **f32), torch.zeros(n, 23, dtype=torch.uint8, device=gpu)
    dw, db, demb = torch.zeros(23, 512, **f32), torch.zeros(23, **f32), torch.zeros(n, 512, **f32)
    wsb = int(L.lib().tspm_mono_head_bce_workspace(n, 512, 23))
    ws = torch.zeros(wsb // 4, **f32)
    d = L.MonoHeadBceDesc(n=n, hid=512, classes=23, ld_emb=512, ld_demb=512, loss_weight=1.0, threshold=0.5)
    d.emb, d.w, d.b, d.targets = st.emb.data_ptr(), cls.weight.data_ptr(), cls.bias.data_ptr(), st.labels.data_ptr()
    d.logits, d.loss, d.preds = logits.data_ptr(), loss.data_ptr(), preds.data_ptr()
    d.dw, d.db, d.demb, d.workspace, d.workspace_bytes = dw.data_ptr(), db.data_ptr(), demb.data_ptr(), ws.data_ptr(), wsb
    L.check(L.lib().tspm_mono_head_bce_step(ctypes.byref(d), L.stream_handle()), "training head")
    torch.cuda.synchronize()
    assert torch.equal(logits, st.logits) and torch.equal(loss, st.loss) and torch.equal(preds.bool(), st.preds)


@pytest.mark.parametrize("fin,n", [(4096, 16), (300, 5)])
def test_encoder_inference_forward_equals_fp64_eval(gpu, fin, n):
    torch.manual_seed(6)
    enc = M.MMIMDbModalityEncoder(fin, 512).to(gpu).eval()
    _randomise_running_stats(enc.net[0], 2)
    o32 = orc.OracleEncoder(fin, 512)
    o32.load_state_dict({k: v.cpu() for k, v in enc.state_dict().items()})
    o64 = orc.OracleEncoder(fin, 512).double()
    o64.load_state_dict({k: v.cpu().double() if v.is_floating_point() else v.cpu() for k, v in enc.state_dict().items()})
    x, _ = _batch(fin, 23, n)
    emb = enc(x.to(gpu))
    with torch.no_grad():
        check_out("encoder embedding", emb, o32.eval()(x), o64.eval()(x.double()))
    enc.train()
    with torch.no_grad():  # no-grad: still the inference embedding
        assert torch.equal(enc(x.to(gpu)), emb)
    with pytest.raises(L.TspmError, match="MMIMDb.*MonomodalEncoder"):
        enc(x.to(gpu))  # training mode with grad enabled would need an autograd node
    with pytest.raises(L.TspmError):
        enc.eval()(x)  # a CPU tensor: the device-only rule


def test_train_and_validation_step_api(gpu):
    ours = _ours(300, 512, 23, gpu, 11, True)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=LR, weight_decay=WD)
    x, y = _batch(300, 23, 16)
    batch = {"text": x, "label": y}
    before = {n: p.detach().cpu().clone() for n, p in ours.named_parameters()}
    ours.train()
    r = ours.train_step(batch, opt, None, gpu, None, "MMIMDb_Text_Encoder_Pretrain")
    assert set(r) == {"loss", "metrics"} and set(r["metrics"]) == {"loss"} and np.isfinite(r["loss"])
    assert isinstance(ours._fused, FusedMMIMDbMonoStep)
    for n, p in ours.named_parameters():
        assert not torch.equal(p.detach().cpu(), before[n]), f"{n} did not change"
    ours.eval()
    v = ours.validation_step(batch, None, gpu, None, "MMIMDb_Text_Encoder_Pretrain")
    assert set(v) == {"loss", "metrics"} and set(v["metrics"]) == {"loss"}
    with pytest.raises(L.TspmError, match="FusedAdam"):
        ours.train_step(batch, torch.optim.Adam(ours.parameters()), None, gpu, None)


def test_fit_monomodal_hands_encoder_to_mmimdb(gpu, tmp_path):
    ours = _ours(300, 512, 23, gpu, 0, True)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=LR, weight_decay=WD)
    tr = M.MMIMDbCorpus(*M.synthetic_features(96, seed=5), gpu)
    va = M.MMIMDbCorpus(*M.synthetic_features(40, seed=6), gpu)
    loaders = {"train": tr.mono_loader("text", 32, shuffle=True, seed=0), "validation": va.mono_loader("text", 32),
               "test": va.mono_loader("text", 32)}
    with pytest.raises(ValueError, match="save_metric"):
        fit_monomodal(ours, opt, None, loaders, 2, experiment_name="MMIMDb_Text_Encoder_Pretrain",
                      model_output_path=tmp_path, save_metric="accuracy")
    w0 = ours.encoder.net[1].weight.detach().cpu().clone()
    h = fit_monomodal(ours, opt, None, loaders, 2, experiment_name="MMIMDb_Text_Encoder_Pretrain",
                      model_output_path=tmp_path)
    keys = {"loss", "f1_samples_TEXT", "f1_macro_TEXT", "f1_weighted_TEXT", "f1_micro_TEXT"}
    for split in ("train", "validation"):
        assert len(h["metrics_history"][split]) == 2
        for e in h["metrics_history"][split]:
            assert set(e) == keys and all(np.isfinite(v) for v in e.values()) and 0.0 <= e["f1_micro_TEXT"] <= 1.0
    assert set(h["metrics_history"]["test"]) == keys
    assert not torch.equal(ours.encoder.net[1].weight.detach().cpu(), w0)
    assert int(ours.encoder.net[0].num_batches_tracked) in (3, 6)  # 3 batches per epoch; the best checkpoint is loaded
    assert h["encoder_path"] and (tmp_path / "encoder_text_best.pth").exists() and (tmp_path / "best.pth").exists()
    # the best validation epoch's loss is the mean of the per-batch BCE of the fp64 oracle holding the best state
    # (fit_monomodal loads best.pth before the test pass)
    _, o64 = pair_from(ours, lambda: OracleMono(300, 512, 23))
    with torch.no_grad():
        o64.eval()
        want = np.mean([orc.bce_loss(o64(va.text[s:s + 32].cpu().double()), va.labels[s:s + 32].cpu().double()).item()
                        for s in range(0, 40, 32)])
    best = min(e["loss"] for e in h["metrics_history"]["validation"])
    assert abs(h["metrics_history"]["test"]["loss"] - best) <= 1e-6 * best
    assert abs(best - want) <= 1e-4 * abs(want)
    # hand-off: the file loads strictly into the fusion model's text encoder and moves its eval logits
    enc_sd = torch.load(tmp_path / "encoder_text_best.pth", weights_only=True)
    fusion = dropin(1)
    assert list(enc_sd) == list(fusion.get_encoder("text").state_dict())
    fusion = fusion.to(gpu).eval()
    I, T = va.image[:8].clone(), va.text[:8].clone()
    logits0 = fusion(I, T).clone()
    fusion.get_encoder("text").load_state_dict(enc_sd, strict=True)
    logits1 = fusion(I, T).clone()
    torch.cuda.synchronize()
    assert not torch.equal(logits0, logits1)
    mono = MonomodalEncoder(M.MMIMDbModalityEncoder(300, 512), 512, 23)
    mono.encoder.load_state_dict(enc_sd)
    mono = mono.to(gpu).eval()
    assert torch.equal(mono.encoder(T), fusion._engine(8, gpu).ET)  # the fusion engine's text embedding, bitwise
