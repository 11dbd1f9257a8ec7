"""MOSI / MOSEI sentiment regression (a one-output ``netC.fc_out``, float32 ``regression_labels``, a single mean L1 /
MSE term) on the fused HIP step against the fp64 oracle, under tests/test_gpu_mosi.py's criterion (tests/parity.py):
the oracle — built here from oracle/mosi_ref.py's parts with ``OracleFcClassifier(..., 1)``, ``F.l1_loss`` /
``F.mse_loss``, ``clip_grad_norm_`` and the oracle Adam — runs in fp64 with our decisions forced into it; predictions
and loss rel-L2 <= 1e-4, every gradient rel-L2 <= 1e-3 and cosine >= 0.9999 and within 4x the fp32 reference's error;
the clip coefficient against our total norm and Adam exactly; every step checked from our own state."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import tspm_amd
from oracle import mosi_ref as orc
from parity import Tally, check_grad, check_out, pair_from, rel_l2, snapshot
from test_gpu_mosi import _check_adam, _corpus_from, _decisions, _flips, _masked
from tspm_amd import _lib as L
from tspm_amd import mosi as M
from tspm_amd import msa_metrics as MM
from tspm_amd.metrics import RegressionLog

pytestmark = pytest.mark.gpu
LOSSES = {"l1": (nn.L1Loss, F.l1_loss), "mse": (nn.MSELoss, F.mse_loss)}


class Group(dict):
    """A LossFunctionGroup of one weighted term (items() -> terms with .loss_fn / .weight; call -> total_loss)."""

    def __init__(self, kind="l1", weight=1.0):
        super().__init__(term=SimpleNamespace(loss_fn=LOSSES[kind][0](), weight=weight))
        self.kind, self.weight = kind, weight

    def __call__(self, x, y):
        return {"total_loss": 0.0 + self.weight * LOSSES[self.kind][1](x, y)}


def _dropin(seed, cfg=orc.MOSI, clip=None, output_dim=1):
    torch.manual_seed(seed)
    a = M.LSTMEncoder(input_size=cfg.audio_dim, hidden_size=64, embd_method=cfg.embd_method)
    v = M.LSTMEncoder(input_size=cfg.video_dim, hidden_size=64, embd_method=cfg.embd_method)
    t = M.TextCNN(input_size=768, embd_size=64, dropout=cfg.text_dropout, in_channels=1, out_channels=128,
                  kernel_heights=[3, 4, 5])
    c = M.FcClassifier(input_dim=192, layers=list(cfg.cls_layers), output_dim=output_dim, dropout=cfg.cls_dropout,
                       use_bn=cfg.use_bn)
    return M.UttFusionModel(a, v, t, c, clip=cfg.clip if clip is None else clip)


def _oracle(seed, cfg=orc.MOSI):
    o = orc.build_oracle_utt(seed, cfg=cfg)
    o.netC = orc.OracleFcClassifier(3 * orc.HIDDEN, list(cfg.cls_layers), 1, dropout=cfg.cls_dropout, use_bn=cfg.use_bn)
    return o


def _scores(n, seed):
    """Sentiment scores on the 0.2 grid of the real labels."""
    return (torch.randint(-15, 16, (n,), generator=torch.Generator().manual_seed(seed)).double() / 5).float()


def _oracle_step(o, A, V, T, y, keeps, trace, kind, weight):
    """utt_fusion.py's train_step up to the optimizer with the regression loss (clip off: raw gradients)."""
    o.train()
    logits = orc.forward(o, A, V, T, True, keeps, trace)
    for p in o.parameters():
        p.grad = None
    loss = 0.0 + weight * LOSSES[kind][1](logits.squeeze(-1), y.to(logits.dtype))
    loss.backward()
    return {"loss": loss.detach(), "logits": logits.detach()}


def _check_step(ours, st, o32, o64, A, V, T, y, keeps, out, tally, kind, weight):
    eng = st.eng
    forced = _decisions(eng)
    t32, t64 = orc.MosiTrace(forced), orc.MosiTrace(forced)
    r32 = _oracle_step(o32, A, V, T, y, keeps, t32, kind, weight)
    r64 = _oracle_step(o64, A.double(), V.double(), T.double(), y, keeps, t64, kind, weight)
    rep = _flips(t64, forced, keeps, eng.use_bn)
    if kind == "l1":  # the sign of every residual is the fp64 oracle's own (no decision of the loss flipped)
        e64 = r64["logits"].squeeze(-1) - y.double()
        e = out["logits"].detach().cpu().squeeze(-1) - y
        assert torch.equal(torch.sign(e).double(), torch.sign(e64)), "an L1 residual changed sign"
    assert tuple(out["logits"].shape) == (y.numel(), 1)
    check_out("predictions", out["logits"], r32["logits"], r64["logits"], tally)
    check_out("loss", out["loss"], r32["loss"].reshape(1), r64["loss"].reshape(1), tally)
    p32, p64 = dict(o32.named_parameters()), dict(o64.named_parameters())
    for n, p in ours.named_parameters():
        check_grad(f"grad {n}", p.grad, p32[n].grad, p64[n].grad, tally)
    norm64 = torch.sqrt(sum((q.grad.double() ** 2).sum() for q in o64.parameters()))
    norm32 = torch.sqrt(sum((q.grad.double() ** 2).sum() for q in o32.parameters()))
    check_out("total grad norm", eng.total_norm, norm32.reshape(1), norm64.reshape(1), tally)
    if eng.use_bn:
        b32, b64 = dict(o32.named_buffers()), dict(o64.named_buffers())
        for n, b in ours.named_buffers():
            if n.endswith("num_batches_tracked"):
                assert int(b) == int(b64[n]), n
            else:
                check_out(n, b, b32[n], b64[n], tally)
    return rep


CASES = [("mosi", 33, 12, "l1", 1.0), ("mosi", 128, 50, "l1", 1.0), ("mosi", 33, 12, "mse", 0.5),
         ("mosei", 32, 9, "l1", 1.0)]


@pytest.mark.parametrize("name,batch,steps,kind,weight", CASES)
def test_fused_regression_step_vs_oracle(gpu, name, batch, steps, kind, weight):
    """Three steps (eager, captured, replayed) with injected dropout masks."""
    cfg = orc.MOSI if name == "mosi" else orc.MOSEI
    seed = 3
    ours = _dropin(seed, cfg).to(gpu)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
    lengths = [steps - (i * 7) % (steps // 2) for i in range(batch)]
    A, V, T, _ = orc.synthetic_batch(batch, steps, seed=1234 + batch, lengths=lengths, cfg=cfg)
    y = _scores(batch, 77 + batch)
    group = Group(kind, weight)
    st = M.FusedMosiStep(ours, opt, group, batch, steps)
    assert st.regress == (L.REGRESS_L1 if kind == "l1" else L.REGRESS_MSE, weight)
    tally = Tally()
    for s in range(3):
        keeps = orc.keep_masks(batch, 50 + s, cfg=cfg)
        o32, o64 = pair_from(ours, lambda: _oracle(seed, cfg))
        before = snapshot(ours, opt if s else None)
        st.keep_override = {k: v.to(gpu) for k, v in keeps.items()}
        out = st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        assert set(out) == {"loss", "logits"}
        rep = _check_step(ours, st, o32, o64, A, V, T, y, keeps, out, tally, kind, weight)
        coef = float(st.eng.clip_coef.item())
        exp = min(1.0, cfg.clip / (st.eng.total_norm.item() + 1e-6))
        assert abs(coef - exp) <= 1e-6 * exp
        _check_adam(ours, opt, before, s + 1, coef, cfg)
        print(f"[{name} B={batch} T={steps} {kind} step {s + 1}] flips {rep} clip coef {coef:.4f}")
        assert not rep, f"forced decisions differ from fp64's own: {rep}"
    assert st.graph is not None
    print(tally)


@pytest.mark.parametrize("name,batch,steps,kind,weight", CASES)
def test_regression_graph_replay_equals_eager(gpu, name, batch, steps, kind, weight):
    """Every case of the oracle test: four steps eager against eager, capture, two replays — parameters, buffers,
    the log's records, loss log and counters bitwise ((128, 50) is the case whose head walks two row chunks)."""
    cfg = orc.MOSI if name == "mosi" else orc.MOSEI
    res = []
    for use_graph in (False, True):
        ours = _dropin(7, cfg).to(gpu)
        opt = tspm_amd.FusedAdam(ours.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
        log = RegressionLog(gpu, groups=M.PATTERNS)
        st = M.FusedMosiStep(ours, opt, Group(kind, weight), batch, steps, use_graph=use_graph)
        st.log = log
        A, V, T, _ = orc.synthetic_batch(batch, steps, seed=5, cfg=cfg)
        y = _scores(batch, 6)
        for s in range(4):
            st.keep_override = {k: v.to(gpu) for k, v in orc.keep_masks(batch, 90 + s, cfg=cfg).items()}
            st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        res.append((torch.cat([t.detach().reshape(-1).double() for t in ours.state_dict().values()]).cpu(),
                    log.records.cpu(), log.loss_log[:4].cpu(), log.counters.cpu()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert res[0][3].tolist() == [4, 4 * batch] and int(res[0][1][0, 0]) == 4 * batch  # every row under "atv"


@pytest.mark.parametrize("pattern", ["atv", "a", "t"])
def test_regression_eval_step_vs_oracle(gpu, pattern):
    B, S = 33, 12
    ours = _dropin(6).to(gpu)
    o = _oracle(6)
    o.load_state_dict({k: v.cpu() for k, v in ours.state_dict().items()})
    o = o.double().eval()
    A, V, T, _ = orc.synthetic_batch(B, S, seed=31)
    Am, Vm, Tm = _masked(A, V, T, pattern)
    y = _scores(B, 9)
    log = RegressionLog(gpu, groups=M.PATTERNS)
    st = M.FusedMosiEvalStep(ours, Group("l1", 0.5), B, S, log)
    st.eng.groups.copy_(log.group_ids([pattern] * B))
    outs = []
    for _ in range(3):  # eager, capture, replay
        st.step(Am.to(gpu), Vm.to(gpu), Tm.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        outs.append((st.eng.logits.cpu().clone(), st.eng.loss.cpu().clone()))
    assert all(torch.equal(a[0], outs[0][0]) and torch.equal(a[1], outs[0][1]) for a in outs[1:])
    with torch.no_grad():
        ref = orc.forward(o, Am.double(), Vm.double(), Tm.double(), False)
        loss = 0.5 * F.l1_loss(ref.squeeze(-1), y.double())
    check_out(f"eval predictions [{pattern}]", outs[0][0], None, ref)
    assert abs(outs[0][1].item() - loss.item()) <= 1e-4 * abs(loss.item())
    recs, losses, samples = log.fetch()
    gi = M.PATTERNS.index(pattern) if isinstance(M.PATTERNS, list) else list(M.PATTERNS).index(pattern)
    want = MM.regression_record(np.tile(outs[0][0].numpy().reshape(-1), 3), np.tile(y.numpy(), 3))
    assert samples == 3 * B and len(losses) == 3 and recs[gi]["n"] == 3 * B
    assert np.array_equal(recs[gi]["conf7"], want["conf7"]) and np.array_equal(recs[gi]["sign3"], want["sign3"])
    assert all(r["n"] == 0 for i, r in enumerate(recs) if i != gi)
    # validation_step: the same engine and head, float predictions under the "regression" group
    calls = []
    rec = SimpleNamespace(update_group_all=lambda group, predictions, targets, m_types:
                          calls.append((group, predictions, targets, m_types)))
    batch = {"audio": Am, "video": Vm, "text": Tm, "label": y, "pattern_name": [pattern] * B}
    v = ours.validation_step(batch, Group("l1", 0.5), gpu, rec, return_test_info=True)
    assert v["loss"] == outs[0][1].item() and calls[0][0] == "regression"
    assert calls[0][1].dtype == np.float32 and np.array_equal(calls[0][1], outs[0][0].numpy().reshape(-1))
    assert np.array_equal(v["predictions"][0], calls[0][1]) and np.array_equal(calls[0][2], y.numpy())


def test_regression_epoch_harness_per_pattern_metrics(gpu):
    """A MosiEpochRunner epoch on a 40-sample corpus with float labels (zeros included): MSA_<key>_<PATTERN> equal
    msa_regression on the predictions read back per batch; the epoch reads the device once."""
    from tspm_amd import harness
    from tspm_amd.metrics import RegressionMetricRecorder
    from tspm_amd.mosi_data import MOSI, PATTERNS, synthetic_mosi_corpus
    ours = _dropin(8).to(gpu)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=1e-3, weight_decay=1e-3)
    group = Group("l1")
    corpus = synthetic_mosi_corpus(40, seed=2, steps=12, regression=True)
    assert (corpus.labels == 0).any()
    tr = MOSI(split="train", corpus=corpus, device=gpu, seed=4, labels_key="regression_labels")
    va = MOSI(split="valid", corpus=corpus, device=gpu, labels_key="regression_labels")
    runner = harness.runner_for(ours, opt, group)
    assert isinstance(runner, harness.MosiEpochRunner) and runner.regression
    assert isinstance(runner.log, RegressionLog) and isinstance(runner.recorder, RegressionMetricRecorder)
    fetches = []
    fetch = runner.log.fetch
    runner.log.fetch = lambda: (fetches.append(1), fetch())[1]
    tr_loss, _, tr_metrics, tr_n = runner.train_epoch(tr.loader(20, shuffle=True, seed=1))
    assert tr_n == 2 and np.isfinite(tr_loss) and len(fetches) == 1
    assert any(k.startswith("MSA_MAE_") for k in tr_metrics)
    va_loss, _, vm, va_n = runner.validate_epoch(va.loader(32))
    assert len(fetches) == 2
    # host replay of the validation epoch through validation_step, per pattern group
    losses, preds, labels = [], {p: [] for p in PATTERNS}, {p: [] for p in PATTERNS}

    class Rec:
        def update_group_all(self, group, predictions, targets, m_types):
            assert group == "regression"
            for pr, t, m in zip(predictions, targets, m_types):
                preds[m].append(pr)
                labels[m].append(t)
    for b in va.device_loader(32):
        for p, sub in b.items():
            losses.append(ours.validation_step(sub, group, gpu, Rec())["loss"])
    assert va_n == len(losses) and abs(va_loss - float(np.mean(losses))) <= 1e-6 * abs(va_loss)
    keys = [k for k in vm if k != "loss"]
    assert keys == [f"MSA_{k}_{p.upper()}" for p in sorted(PATTERNS) for k in MM.REGRESSION_KEYS]
    for p in PATTERNS:
        assert len(preds[p]) == 40
        want = MM.msa_regression(MM.regression_record(np.asarray(preds[p], np.float32), np.asarray(labels[p], np.float32)))
        for k, val in want.items():
            got = vm[f"MSA_{k}_{p.upper()}"]
            assert (np.isnan(val) and np.isnan(got)) or got == val, (p, k, got, val)
    print({p: vm[f"MSA_MAE_{p.upper()}"] for p in PATTERNS})
    with pytest.raises(ValueError):
        harness.fit(ours, opt, group, {"train": [], "validation": []}, 1, save_metric="MSA_MAE_ATV")


def test_loader_gathers_float_labels_into_the_step(gpu):
    from tspm_amd.mosi_data import MOSI, synthetic_mosi_corpus
    B, S = 16, 9
    corpus = synthetic_mosi_corpus(24, seed=5, steps=S, regression=True)
    ours = _dropin(3).to(gpu)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=1e-3, weight_decay=1e-3)
    group = Group("mse")
    ds = MOSI(split="train", corpus=corpus, device=gpu, selected_patterns=["atv"], labels_key="regression_labels")
    b = next(iter(ds.device_loader(B, shuffle=False, step_for=lambda n, t: ours.fused_step(opt, group, n, t))))
    st = ours.fused_step(opt, group, B, S)
    assert b["audio"] is st.eng.A and b["label"] is st.eng.labels_f and b["label"].dtype == torch.float32
    assert torch.equal(st.eng.labels_f.cpu(), torch.from_numpy(corpus.labels[:B]))
    st.run()
    torch.cuda.synchronize()
    assert np.isfinite(st.eng.loss.item())
    # the batch-first form: a float32 [B] tensor
    flat = ds.collate_fn(ds.__getitems__(list(range(8, 24))))
    assert flat["label"].dtype == torch.float32 and tuple(flat["label"].shape) == (16,)
    assert torch.equal(flat["label"].cpu(), torch.from_numpy(corpus.labels[8:24]))
    # [n, 1] labels are taken as well; an out-of-range index gives a NaN label
    from tspm_amd.mosi_data import DeviceMosiCorpus
    corpus.labels = corpus.labels.reshape(-1, 1)
    dc = DeviceMosiCorpus(corpus, gpu)
    out = {"audio": torch.empty(3, S, 5, device=gpu)}
    lab = torch.empty(3, device=gpu)
    dc.gather(torch.tensor([2, 99, 0], device=gpu), S, out, False, None, lab)
    got = lab.cpu()
    assert got[0].item() == corpus.labels[2, 0] and got[2].item() == corpus.labels[0, 0] and torch.isnan(got[1])


def test_train_step_api_fused_and_autograd_fallback(gpu):
    """UttFusionModel.train_step in regression mode: FusedAdam -> the fused step; torch.optim.Adam -> the autograd
    node with the same loss group (dropout off so the two can be compared)."""
    A, V, T, _ = orc.synthetic_batch(16, 12, seed=21)
    y = _scores(16, 4)
    batch = {"audio": A, "video": V, "text": T, "label": y.reshape(-1, 1), "pattern_name": ["atv"] * 16}
    group = Group("l1", 0.5)
    res = {}
    for kind in ("fused", "autograd"):
        ours = _dropin(4).to(gpu)
        ours.netT.dropout.p = 0.0
        ours.netC.dropout_p = 0.0
        opt = (tspm_amd.FusedAdam(ours.parameters(), lr=1e-3, weight_decay=1e-3) if kind == "fused"
               else torch.optim.Adam(ours.parameters(), lr=1e-3, weight_decay=1e-3))
        calls = []
        rec = SimpleNamespace(update_group_all=lambda group, predictions, targets, m_types:
                              calls.append((group, predictions, targets)))
        r = ours.train_step(batch, opt, group, gpu, rec)
        torch.cuda.synchronize()
        assert set(r) == {"loss"} and (kind == "fused") == bool(ours._steps)
        assert calls[0][0] == "regression" and calls[0][1].dtype == np.float32 and calls[0][1].shape == (16,)
        assert np.array_equal(calls[0][2], y.numpy())
        res[kind] = (r["loss"], torch.cat([p.detach().reshape(-1) for p in ours.parameters()]).cpu(), calls[0][1])
    assert abs(res["fused"][0] - res["autograd"][0]) <= 1e-5 * abs(res["fused"][0])
    assert rel_l2(res["fused"][2], res["autograd"][2]) < 1e-5
    assert rel_l2(res["fused"][1], res["autograd"][1]) < 1e-4
    # a head outside the kernel's limits: the fused step refuses at construction, train_step takes the autograd path
    torch.manual_seed(0)
    wide = M.UttFusionModel(M.LSTMEncoder(5, 64), M.LSTMEncoder(20, 64), M.TextCNN(768, 64),
                            M.FcClassifier(192, [64, 132], 1, dropout=0.0), clip=1.0).to(gpu)
    wopt = tspm_amd.FusedAdam(wide.parameters(), lr=1e-3)
    with pytest.raises(L.TspmError):
        M.FusedMosiStep(wide, wopt, group, 16, 12)
    topt = torch.optim.Adam(wide.parameters(), lr=1e-3)
    before = wide.netC.fc_out.weight.detach().clone()
    assert np.isfinite(wide.train_step(batch, topt, group, gpu, None)["loss"]) and not wide._steps
    assert not torch.equal(before, wide.netC.fc_out.weight.detach())
    with pytest.raises(L.TspmError):  # two terms: neither the regression head nor the cross-entropy step
        M.FusedMosiStep(_dropin(4).to(gpu), wopt, Group("l1", 1.0) | {"second": group["term"]}, 16, 12)


def test_classification_step_is_unchanged_by_a_regression_step(gpu):
    """The classification step of a model built before a regression step ran and of the same model built after it
    are bitwise the same (parameters after two steps, logits, loss)."""
    from test_mosi_cpu import _dropin as dropin3

    def classify():
        ours = dropin3(5).to(gpu)
        opt = tspm_amd.FusedAdam(ours.parameters(), lr=1e-3, weight_decay=1e-3)
        st = M.FusedMosiStep(ours, opt, None, 33, 12)
        assert st.regress is None
        A, V, T, y = orc.synthetic_batch(33, 12, seed=5)
        for s in range(3):
            st.keep_override = {k: v.to(gpu) for k, v in orc.keep_masks(33, 90 + s).items()}
            out = st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        return torch.cat([p.detach().reshape(-1) for p in ours.parameters()] +
                         [out["logits"].reshape(-1), out["loss"].reshape(-1)]).cpu()

    first = classify()
    reg = _dropin(5).to(gpu)
    ropt = tspm_amd.FusedAdam(reg.parameters(), lr=1e-3, weight_decay=1e-3)
    rst = M.FusedMosiStep(reg, ropt, Group("l1"), 33, 12)
    A, V, T, _ = orc.synthetic_batch(33, 12, seed=5)
    for _ in range(3):
        rst.step(A.to(gpu), V.to(gpu), T.to(gpu), _scores(33, 1).to(gpu))
    torch.cuda.synchronize()
    assert torch.equal(first, classify())


def test_labels_go_to_the_buffer_of_the_steps_mode(gpu):
    """``step()`` / ``load()`` route labels by the step's mode, not by the tensor's dtype: int64 scores given to a
    regression step are cast into ``labels_f``; float class labels given to a classification step are cast into
    ``labels`` (as before this mode existed) and ``labels_f`` stays untouched."""
    from test_mosi_cpu import _dropin as dropin3
    A, V, T, yc = orc.synthetic_batch(8, 9, seed=2)
    A, V, T = A.to(gpu), V.to(gpu), T.to(gpu)
    reg = _dropin(2).to(gpu)
    rst = M.FusedMosiStep(reg, tspm_amd.FusedAdam(reg.parameters(), lr=1e-3), Group("l1"), 8, 9)
    ints = torch.tensor([-3, -2, -1, 0, 0, 1, 2, 3])
    rst.step(A, V, T, ints.to(gpu))
    torch.cuda.synchronize()
    assert torch.equal(rst.eng.labels_f.cpu(), ints.float()) and not bool(rst.eng.labels.any())
    as_float = rst.eng.loss.item()
    cls = dropin3(2).to(gpu)
    cst = M.FusedMosiStep(cls, tspm_amd.FusedAdam(cls.parameters(), lr=1e-3), None, 8, 9)
    cst.step(A, V, T, yc.float().to(gpu))
    torch.cuda.synchronize()
    assert torch.equal(cst.eng.labels.cpu(), yc) and not bool(cst.eng.labels_f.any())
    assert np.isfinite(as_float) and np.isfinite(cst.eng.loss.item())
    # the pre-training step the same way
    from tspm_amd.monomodal import FusedMosiMonoStep, MonomodalEncoder
    torch.manual_seed(1)
    mono = MonomodalEncoder(M.LSTMEncoder(5, 64), 64, 1).to(gpu)
    mst = FusedMosiMonoStep(mono, tspm_amd.FusedAdam(mono.parameters(), lr=1e-3), Group("mse"), (8, 9, 5))
    mst.step(A, ints.to(gpu))
    torch.cuda.synchronize()
    assert torch.equal(mst.labels_f.cpu(), ints.float()) and not bool(mst.labels.any())
