"""Every missing-modality pattern of a batch from one encoder pass, model level: ``UttFusionModel.forward_patterns``,
``FusedMosiPatternEvalStep`` (MOSI and MOSEI classifiers, per-sample lengths, the attention embedding, regression mode),
the zero rows of the 2B-row inputs, and the ``fuse_patterns`` loader through ``MosiEpochRunner`` and ``fit``.

Shapes: B = 5 (odd: the recurrences' two-row workgroups see a ghost row at B and none at 2B), steps (7, 9, 6), embedding
widths (8, 12, 8), the YAMLs' feature dims.  The reference is oracle/mosi_ref.py in fp64 on the masked inputs (a missing
modality is the zeroed tensor through its encoder), with the length-aware and attention restatements the other model
tests use; the criterion is parity.op_check's (err_ours <= FACTOR x err_ref32 + FLOOR_OUT, the fp32 run of the same oracle
as the yardstick).  Argmax decisions against fp64 go through parity.near_tie_flips with its own cap.  With the seeds
below the fp32 oracle alone makes no flip against fp64 on any batch of any configuration (``oracle32_flips``, computed
on the CPU when the seeds were chosen and asserted again in every test), so a flip of ours would be ours.
"""
from contextlib import contextmanager

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attn_ref as R
import test_gpu_mosi_lengths as tl
import tspm_amd
from oracle import mosi_ref as orc
from parity import NEAR, near_tie_flips, op_check, pair_from, rel_l2
from textcnn_len_ref import TextLenOracle
from tspm_amd import harness
from tspm_amd import mosi as M
from tspm_amd import msa_metrics as MM
from tspm_amd.metrics import ClassificationLog, RegressionLog
from tspm_amd.mosi_data import MOSI, PATTERNS, synthetic_mosi_corpus

pytestmark = pytest.mark.gpu
B, STEPS, WIDTHS = 5, (7, 9, 6), (8, 12, 8)
PATS = tuple(PATTERNS)
SEED_MODEL, SEED_BATCH = 3, 200
# three batches' lengths: every vector holds a 1 and the full length
LENS = [{"audio": [7, 1, 4, 4, 2], "video": [9, 3, 1, 8, 6], "text": [6, 1, 4, 5, 2]},
        {"audio": [2, 7, 5, 1, 6], "video": [4, 9, 1, 7, 2], "text": [3, 6, 6, 1, 4]},
        {"audio": [6, 6, 3, 7, 1], "video": [1, 2, 9, 5, 9], "text": [5, 2, 6, 3, 1]}]
CONFIGS = {
    "mosi": dict(name="mosi"),
    "mosei": dict(name="mosei"),  # BatchNorm1d classifier with non-trivial running statistics, "maxpool"
    "lengths": dict(name="mosi", lengths=True),
    "attn-time": dict(name="mosi", method="attention", norm="time"),
    "attn-unit": dict(name="mosei", method="attention", norm="unit"),
}


def _cfg(name):
    return orc.MOSI if name == "mosi" else orc.MOSEI


def _ours(name="mosi", method=None, norm=None, output_dim=3, lengths=False, seed=SEED_MODEL):
    """The model on the CPU (the tests move it): the YAML's model at the small embedding widths; a BatchNorm classifier
    gets running statistics away from (0, 1) and an affine away from (1, 0)."""
    torch.manual_seed(seed)
    m = M.build_utt_fusion(name, output_dim=output_dim, embd_sizes=WIDTHS, embd_method=method, attention_norm=norm)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for bn in m.netC.bns():
            bn.running_mean.copy_(0.3 * torch.randn(bn.num_features, generator=g))
            bn.running_var.copy_(0.5 + torch.rand(bn.num_features, generator=g))
            bn.weight.copy_(1 + 0.2 * torch.randn(bn.num_features, generator=g))
            bn.bias.copy_(0.1 * torch.randn(bn.num_features, generator=g))
    return m


def _oracle_builder(name="mosi", method=None, norm=None, output_dim=3, lengths=False):
    cfg = _cfg(name)
    method = method or cfg.embd_method

    def build():
        mk = lambda dim, h: (R.AttnEncoderRef(dim, h, "attention", norm) if method == "attention"  # noqa: E731
                             else orc.OracleLSTMEncoder(dim, h, method))
        a, v = mk(cfg.audio_dim, WIDTHS[0]), mk(cfg.video_dim, WIDTHS[1])
        t = orc.OracleTextCNN(768, embd_size=WIDTHS[2], dropout=cfg.text_dropout, in_channels=1, out_channels=128,
                              kernel_heights=[3, 4, 5])
        c = orc.OracleFcClassifier(sum(WIDTHS), list(cfg.cls_layers), output_dim, dropout=cfg.cls_dropout,
                                   use_bn=cfg.use_bn)
        return orc.OracleUttFusion(a, v, t, c, clip=cfg.clip)
    return build


def _batch(name, s, lengths=None, regression=False):
    cfg = _cfg(name)
    g = torch.Generator().manual_seed(SEED_BATCH + s)
    A = torch.randn(B, STEPS[0], cfg.audio_dim, generator=g)
    V = 0.5 * torch.randn(B, STEPS[1], cfg.video_dim, generator=g)
    T = 0.3 * torch.randn(B, STEPS[2], cfg.text_dim, generator=g)
    if lengths is not None:  # zero padding past each sample's length, as pad_sequence leaves it
        for i in range(B):
            A[i, lengths["audio"][i]:] = 0
            V[i, lengths["video"][i]:] = 0
            T[i, lengths["text"][i]:] = 0
    if regression:
        return A, V, T, (torch.randint(-15, 16, (B,), generator=g).double() / 5).float()
    return A, V, T, torch.randint(0, 3, (B,), generator=g)


def _masked(A, V, T, pattern):
    """The batch as the per-pattern loader delivers it: a missing modality is the zeroed tensor."""
    k = [1.0 if ch in pattern else 0.0 for ch in "avt"]
    return A * k[0], V * k[1], T * k[2]


@contextmanager
def _oracle_mode(method, lengths):
    """oracle.mosi_ref with the restatements the configuration needs swapped in (and put back)."""
    saved = orc.lstm_forward, orc.textcnn_forward
    try:
        other = tl.LenOracle(lengths) if lengths else orc.lstm_forward
        orc.lstm_forward = R.AttnOracle(other, lengths) if method == "attention" else other
        if lengths:
            orc.textcnn_forward = TextLenOracle(lengths["text"])
        yield
    finally:
        orc.lstm_forward, orc.textcnn_forward = saved


def _reference(o32, o64, A, V, T, y, patterns, method=None, lengths=None, regress=None):
    """{pattern: (logits32, logits64, loss32, loss64)} of the two oracles in eval mode on the masked inputs."""
    out = {}
    with torch.no_grad(), _oracle_mode(method, lengths):
        for p in patterns:
            Am, Vm, Tm = _masked(A, V, T, p)
            row = []
            for o, dt in ((o32.eval(), torch.float32), (o64.eval(), torch.float64)):
                lg = orc.forward(o, Am.to(dt), Vm.to(dt), Tm.to(dt), False)
                if regress is not None:
                    loss = regress * F.l1_loss(lg.squeeze(-1), y.to(dt))
                else:
                    loss = F.cross_entropy(lg, y)
                row.append((lg, loss.reshape(1)))
            out[p] = (row[0][0], row[1][0], row[0][1], row[1][1])
    return out


def oracle32_flips(ref):
    """Argmax disagreements of the fp32 oracle with the fp64 oracle over a reference (the seeds keep it at 0)."""
    return sum(int((r[0].argmax(1) != r[1].argmax(1)).sum()) for r in ref.values())


def _dev(lengths, dev):
    return None if lengths is None else {k: torch.tensor(v, dtype=torch.int32, device=dev) for k, v in lengths.items()}


_REFS = {}


def _setup(key):
    """(model on the CPU, [(batch, lengths, reference)] x 3) of a configuration, computed once per session."""
    if key not in _REFS:
        c = CONFIGS[key]
        ours = _ours(**c)
        o32, o64 = pair_from(ours, _oracle_builder(**c))
        items = []
        for s in range(3):
            lengths = LENS[s] if c.get("lengths") else None
            A, V, T, y = _batch(c["name"], s, lengths)
            ref = _reference(o32, o64, A, V, T, y, PATS, c.get("method"), lengths)
            assert oracle32_flips(ref) == 0, f"{key}: choose another seed (the fp32 oracle flips on batch {s})"
            items.append(((A, V, T, y), lengths, ref))
        _REFS[key] = (ours, items)
    return _REFS[key]


# ------------------------------------------------------------------------------------------------
# forward_patterns
# ------------------------------------------------------------------------------------------------
def test_forward_patterns_vs_fp64(gpu):
    """[P, B, C] logits per pattern against fp64, and the existing path ``model.eval()(A ka, V kv, T kt)`` under the same
    criterion; the rel-L2 between the two paths is printed (not bitwise: the dense kernels' path depends on the rows).
    A subset in another order gives those patterns' rows."""
    cpu_model, items = _setup("mosi")
    ours = cpu_model.to(gpu).train()  # forward_patterns is eval-mode whatever the flag, and leaves the flag alone
    (A, V, T, _), _, ref = items[0]
    out = ours.forward_patterns(A.to(gpu), V.to(gpu), T.to(gpu))
    assert tuple(out.shape) == (7, B, 3) and ours.training and not out.requires_grad
    ours.eval()
    for i, p in enumerate(PATS):
        op_check(f"forward_patterns[{p}]", out[i], ref[p][0], ref[p][1])
        with torch.no_grad():
            plain = ours(*[x.to(gpu) for x in _masked(A, V, T, p)])
        op_check(f"per-pattern forward[{p}]", plain, ref[p][0], ref[p][1])
        print(f"fused vs per-pattern [{p}]: rel-L2 {rel_l2(out[i], plain):.3e}")
    sub = ours.forward_patterns(A.to(gpu), V.to(gpu), T.to(gpu), patterns=("v", "at"))
    assert tuple(sub.shape) == (2, B, 3)
    for i, p in enumerate(("v", "at")):
        op_check(f"forward_patterns subset[{p}]", sub[i], ref[p][0], ref[p][1])
    keys = [k for k in ours._engines if k[0] == ("patterns", PATS) or k[0] == ("patterns", ("v", "at"))]
    assert len(keys) == 2 and (B, M.norm_steps(STEPS), gpu) in ours._engines  # the plain engine keeps its key
    eng = ours._pattern_engine(B, STEPS, gpu)
    assert eng.enc.B == 2 * B and eng.cls.B == 7 * B and not hasattr(eng.cls, "lstm") and not hasattr(eng.cls, "conv_out")
    assert not hasattr(eng.enc, "h") and eng.enc.lstm["a"]["dg"] is None  # no classifier, no backward buffers
    with pytest.raises(ValueError):
        ours.forward_patterns(A.to(gpu), V.to(gpu), T.to(gpu), patterns=("atv", "x"))


# ------------------------------------------------------------------------------------------------
# the step: eager, capture, replay
# ------------------------------------------------------------------------------------------------
def _zero_rows(eng):
    for nm, buf in (("audio", eng.A), ("video", eng.V), ("text", eng.X)):
        assert buf.shape[1] == 2 * B and not bool(buf[:, B:].any()), f"{nm}: the zero rows were written"
        assert bool(buf[:, :B].any())


@pytest.mark.parametrize("key", list(CONFIGS))
def test_pattern_eval_step_three_batches(gpu, key):
    c = CONFIGS[key]
    cpu_model, items = _setup(key)
    ours = cpu_model.to(gpu)
    log = ClassificationLog(gpu, groups=PATTERNS, classes=3)
    use_len = bool(c.get("lengths"))
    st = M.FusedMosiPatternEvalStep(ours, None, B, STEPS, log, ragged=use_len, text_lengths=use_len)
    assert st.eng is ours._pattern_engine(B, STEPS, gpu, None, use_len, use_len) and st.patterns == PATS
    want_conf = np.zeros((7, 3, 3), dtype=np.int64)
    want_losses, graph = [], None
    for s, ((A, V, T, y), lengths, ref) in enumerate(items):
        st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu), _dev(lengths, gpu))
        torch.cuda.synchronize()
        logits, losses = st.eng.logits.cpu().clone(), st.eng.losses.cpu().clone()
        assert torch.equal(st.eng.cls.labels.cpu(), y.repeat(7))
        assert st.eng.cls.groups.cpu().tolist() == [g for g in range(7) for _ in range(B)]
        pred = torch.softmax(logits, dim=-1).argmax(dim=-1)
        for i, p in enumerate(PATS):
            for b in range(B):
                want_conf[i, int(y[b]), int(pred[i, b])] += 1
            nf = near_tie_flips(f"{key} batch {s} [{p}]", pred[i], ref[p][1].argmax(1), ref[p][1], 1)
            op_check(f"{key} batch {s} logits[{p}]", logits[i], ref[p][0], ref[p][1])
            op_check(f"{key} batch {s} loss[{p}]", losses[i:i + 1], ref[p][2], ref[p][3])
            if nf:
                print(f"{key} batch {s} [{p}]: {nf} near-tie flip")
        want_losses += losses.tolist()
        if use_len:  # the second half of every length buffer mirrors the first
            e = st.eng.enc
            for buf, nm in ((e.lens["a"], "audio"), (e.lens["v"], "video"), (e.text_lens, "text")):
                assert buf.numel() == 2 * B and buf[:B].cpu().tolist() == lengths[nm] == buf[B:].cpu().tolist()
        if s == 1:
            graph = st.graph
            assert graph is not None  # captured on the second call
        if s == 2:
            assert st.graph is graph  # replayed
    conf, loss_log, samples = log.fetch()
    assert np.array_equal(conf, want_conf)  # exactly the counts of the step's own logits
    assert samples == 3 * 7 * B and len(loss_log) == 3 * 7  # P entries per batch, in pattern order
    assert loss_log.tolist() == want_losses
    _zero_rows(st.eng)
    assert st.calls == 3


def test_step_refusals_and_group_order(gpu):
    cpu_model, items = _setup("mosi")
    ours = cpu_model.to(gpu)
    log = ClassificationLog(gpu, groups=PATTERNS, classes=3)
    two = type("Two", (dict,), {})(a=1, b=2)
    with pytest.raises(tspm_amd.TspmError, match="single cross-entropy"):
        M.FusedMosiPatternEvalStep(ours, two, B, STEPS, log)
    with pytest.raises(ValueError, match="Invalid patterns"):
        M.FusedMosiPatternEvalStep(ours, None, B, STEPS, log, patterns=["q"])
    # a subset out of order: rows, labels and group ids follow the given order, the ids the log's group order
    st = M.FusedMosiPatternEvalStep(ours, None, B, STEPS, log, patterns=("v", "at"))
    (A, V, T, y), _, ref = items[0]
    st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
    with pytest.raises(tspm_amd.TspmError):  # not a ragged step
        st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu), _dev(LENS[0], gpu))
    conf, losses, samples = log.fetch()
    assert samples == 2 * B and len(losses) == 2
    assert st.eng.cls.groups.cpu().tolist() == [6] * B + [1] * B
    assert conf.sum(axis=(1, 2)).tolist() == [0, B, 0, 0, 0, 0, B]
    for i, p in enumerate(("v", "at")):
        op_check(f"subset logits[{p}]", st.eng.logits[i], ref[p][0], ref[p][1])


# ------------------------------------------------------------------------------------------------
# regression mode
# ------------------------------------------------------------------------------------------------
def _record_vector(rec):
    return torch.tensor([rec[k] for k in ("sum_abs", "sum_sq", "sum_p", "sum_y", "sum_pp", "sum_yy", "sum_py")],
                        dtype=torch.float64)


def test_regression_records_and_losses(gpu):
    """``output_dim=1`` with a mean L1 term of weight 0.5: the RegressionLog of the fused step and the one of the
    per-pattern path (``FusedMosiEvalStep`` on the masked inputs) both within op_check's bound of the records of the
    fp64 oracle's predictions, pattern by pattern; the integer fields equal the host's records of each path's own
    predictions; 3 x P loss entries in pattern order."""
    import test_gpu_mosi_regress as tr
    group, w = tr.Group("l1", 0.5), 0.5
    ours = _ours("mosi", output_dim=1).to(gpu)
    o32, o64 = pair_from(ours, _oracle_builder("mosi", output_dim=1))
    log_f, log_p = RegressionLog(gpu, groups=PATTERNS), RegressionLog(gpu, groups=PATTERNS)
    st = M.FusedMosiPatternEvalStep(ours, group, B, STEPS, log_f)
    per = M.FusedMosiEvalStep(ours, group, B, STEPS, log_p)
    preds = {k: {p: [] for p in PATS} for k in ("fused", "per", "o32", "o64")}
    labels, want_losses = [], []
    for s in range(3):
        A, V, T, y = _batch("mosi", s, regression=True)
        ref = _reference(o32, o64, A, V, T, y, PATS, regress=w)
        st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        got, losses = st.eng.logits.cpu().clone(), st.eng.losses.cpu().clone()
        assert tuple(got.shape) == (7, B, 1) and torch.equal(st.eng.cls.labels_f.cpu(), y.repeat(7))
        want_losses += losses.tolist()
        labels.append(y.numpy())
        for i, p in enumerate(PATS):
            per.eng.groups.copy_(log_p.group_ids([p] * B))
            per.step(*[x.to(gpu) for x in _masked(A, V, T, p)], y.to(gpu))
            torch.cuda.synchronize()
            op_check(f"batch {s} predictions[{p}]", got[i], ref[p][0], ref[p][1])
            op_check(f"batch {s} loss[{p}]", losses[i:i + 1], ref[p][2], ref[p][3])
            op_check(f"batch {s} per-pattern loss[{p}]", per.eng.loss.cpu(), ref[p][2], ref[p][3])
            preds["fused"][p].append(got[i].reshape(-1).numpy())
            preds["per"][p].append(per.eng.logits.cpu().reshape(-1).numpy())
            preds["o32"][p].append(ref[p][0].reshape(-1).numpy())
            preds["o64"][p].append(ref[p][1].reshape(-1).numpy())
    rec_f, loss_log, samples = log_f.fetch()
    rec_p, loss_log_p, _ = log_p.fetch()
    assert samples == 3 * 7 * B and loss_log.tolist() == want_losses and len(loss_log_p) == 21
    yy = np.concatenate(labels)
    for i, p in enumerate(PATS):
        host = {k: MM.regression_record(np.concatenate(v[p]).astype(np.float32 if k != "o64" else np.float64), yy)
                for k, v in preds.items()}
        v32, v64 = _record_vector(host["o32"]), _record_vector(host["o64"])
        op_check(f"fused record[{p}]", _record_vector(rec_f[i]), v32, v64)
        op_check(f"per-pattern record[{p}]", _record_vector(rec_p[i]), v32, v64)
        print(f"records fused vs per-pattern [{p}]: rel-L2 {rel_l2(_record_vector(rec_f[i]), _record_vector(rec_p[i])):.3e}")
        for rec, k in ((rec_f[i], "fused"), (rec_p[i], "per")):
            assert rec["n"] == 3 * B and np.array_equal(rec["conf7"], host[k]["conf7"])
            assert np.array_equal(rec["sign3"], host[k]["sign3"])
    _zero_rows(st.eng)


# ------------------------------------------------------------------------------------------------
# loader, runner, fit
# ------------------------------------------------------------------------------------------------
def test_fused_loader_runner_and_fit(gpu, tmp_path):
    """20 samples at batch 5 (the batch divides the split): ``validate_epoch`` on the fused loader and on the per-pattern
    loader — the same metric keys, confusion counts equal except where a printed near-tie explains a row, mean losses
    both within op_check's bound of the fp64 oracle's mean; one ``fit`` epoch with fused valid and test loaders."""
    N, S = 20, 6
    ours = _ours("mosi").to(gpu)
    o32, o64 = pair_from(ours, _oracle_builder("mosi"))
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=1e-3, weight_decay=1e-3)
    corpus = synthetic_mosi_corpus(N, seed=11, steps=S)
    va = MOSI(split="valid", corpus=corpus, device=gpu)
    runner = harness.runner_for(ours, opt, None)
    fused_loader, plain_loader = va.loader(B, fuse_patterns=True), va.loader(B)
    assert len(fused_loader) == 4 and len(plain_loader) == 28
    # the fused batches: gathered once, unmasked, into rows [0, B) of the step's inputs
    runner.loader_for(fused_loader, False)
    dense = {m: torch.from_numpy(corpus.data[m]).reshape(N, S, -1) for m in ("audio", "video", "text")}
    for i, b in enumerate(fused_loader):
        st = runner.pattern_eval_step_for(B, S)
        assert b["fused_patterns"] is True and b["patterns"] == list(PATTERNS) and "pattern_name" not in b
        assert b["audio"] is st.eng.A and b["label"] is st.eng.labels and b["time_major"] and b["steps"] == S
        rows = slice(i * B, (i + 1) * B)
        for m, buf in (("audio", st.eng.A), ("video", st.eng.V), ("text", st.eng.X)):
            assert torch.equal(buf[:, :B].cpu().transpose(0, 1), dense[m][rows]) and not bool(buf[:, B:].any())
        assert np.array_equal(b["label"].cpu().numpy(), corpus.labels[rows])
    loss_f, _, met_f, n_f = runner.validate_epoch(fused_loader)
    conf_f, losses_f, samples_f = runner.log.fetch()
    loss_p, _, met_p, n_p = runner.validate_epoch(plain_loader)
    conf_p, losses_p, samples_p = runner.log.fetch()
    assert list(met_f) == list(met_p) and n_f == n_p == 28 and samples_f == samples_p == 7 * N
    assert len(runner.eval_steps) == 2 and (("patterns", PATS), B, S) in runner.eval_steps and (B, S) in runner.eval_steps
    # the reference: every (batch, pattern) entry of the epoch in fp32 and fp64, and each path's own logits
    y = torch.from_numpy(corpus.labels)
    l32, l64, want_f, want_p, explained = [], [], np.zeros_like(conf_f), np.zeros_like(conf_p), 0
    ours.eval()
    for i in range(N // B):
        rows = slice(i * B, (i + 1) * B)
        A, V, T = (dense[m][rows] for m in ("audio", "video", "text"))
        ref = _reference(o32, o64, A, V, T, y[rows], PATS)
        lf = ours.forward_patterns(A.to(gpu), V.to(gpu), T.to(gpu)).cpu()
        for j, p in enumerate(PATS):
            with torch.no_grad():
                lp = ours(*[x.to(gpu) for x in _masked(A, V, T, p)]).cpu()
            l32.append(ref[p][2])
            l64.append(ref[p][3])
            pf, pp = torch.softmax(lf[j], -1).argmax(-1), torch.softmax(lp, -1).argmax(-1)
            for b in range(B):
                want_f[j, int(y[rows][b]), int(pf[b])] += 1
                want_p[j, int(y[rows][b]), int(pp[b])] += 1
            if bool((pf != pp).any()):  # a row the two paths decide differently must be a near-tie in fp64
                explained += near_tie_flips(f"batch {i} [{p}] fused vs per-pattern", pf, pp, ref[p][1], 1)
                print(f"batch {i} [{p}]: fused {pf.tolist()} per-pattern {pp.tolist()} (near-tie)")
    assert np.array_equal(conf_f, want_f) and np.array_equal(conf_p, want_p)
    assert int(np.abs(conf_f - conf_p).sum()) == 2 * explained  # equal, but for the near-ties printed above
    m32, m64 = torch.cat(l32).mean().reshape(1), torch.cat(l64).mean().reshape(1)
    op_check("fused epoch loss", torch.tensor([loss_f]), m32, m64)
    op_check("per-pattern epoch loss", torch.tensor([loss_p]), m32, m64)
    print(f"epoch loss fused {loss_f:.7f} per-pattern {loss_p:.7f}")
    # fit: fused valid and test loaders, the usual epoch_metrics block
    tr_ds = MOSI(split="train", corpus=corpus, device=gpu, seed=4)
    te = MOSI(split="test", corpus=synthetic_mosi_corpus(10, seed=12, steps=S), device=gpu)
    loaders = {"train": tr_ds.loader(B, shuffle=True, seed=1), "validation": va.loader(B, fuse_patterns=True),
               "test": te.loader(B, fuse_patterns=True)}
    hist = harness.fit(ours, opt, None, loaders, epochs=1, early_stopping=False, metrics_path=tmp_path)
    block = hist["epoch_metrics"][0]
    assert block["epoch"] == 1 and set(block) == {"epoch", "train", "validation"}
    assert np.isfinite(block["validation"]["loss"]) and "timing" in block["validation"]
    assert any(k.startswith("MSA_") and k.endswith("_ATV") for k in block["validation"]["metrics"])
    assert (tmp_path / "epoch_metrics.json").exists() and np.isfinite(hist["test"]["loss"])
    assert list(hist["validation"][0]) == list(dict(met_p, loss=0.0))
