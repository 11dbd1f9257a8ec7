"""Training every missing-modality pattern of a batch in one step, model level: ``FusedMosiPatternStep`` /
``MosiPatternEngine(backward=True)`` (MOSI and MOSEI classifiers, per-sample lengths, the attention embedding, L1
regression, a pattern subset, frozen encoders, two Adam groups) and the ``all_patterns`` loader through
``MosiEpochRunner`` and ``fit``.

Shapes as test_gpu_mosi_patterns.py: B = 5, steps (7, 9, 6), embedding widths (8, 12, 8).  The yardstick is
oracle/mosi_ref.py (fp32 and fp64, driven as test_gpu_mosi.py drives it: our decisions forced into it, every forced
decision that differs from fp64's own a rare near-tie) on the REPLICATED batch: inputs cat_p(A*ka_p, V*kv_p, T*kt_p),
labels and lengths tiled P times, one mean loss over the P*B rows.  Dropout is on: the masks are injected on our side
through ``keep_override`` ("text" [2B, nc] per encoder row, "cls{j}" [P*B, w_j]) and mapped onto the oracle - replicated
row (p, b) takes the text mask of encoder row b when p keeps text, else of row B + b; the classifier masks row for row.
Bounds: parity.op_check (FACTOR, FLOOR_OUT / FLOOR_GRAD, gradient cosine) for loss, logits, every parameter gradient and
the BatchNorm running statistics; parity.near_tie_flips for the argmax.  Each of the three steps (eager, capture,
replay) is checked from our own state before that step.
"""
import numpy as np
import pytest
import torch

import test_gpu_mosi as tm
import test_gpu_mosi_finetune as tf
import test_gpu_mosi_lengths as tl
import test_gpu_mosi_patterns as tp
import test_gpu_mosi_regress as tr
import tspm_amd
from oracle import mosi_ref as orc
from parity import near_tie_flips, op_check, pair_from
from tspm_amd import harness
from tspm_amd import mosi as M
from tspm_amd.mosi_data import MOSI, PATTERNS, synthetic_mosi_corpus

pytestmark = pytest.mark.gpu
B, STEPS, WIDTHS, PATS, LENS = tp.B, tp.STEPS, tp.WIDTHS, tp.PATS, tp.LENS
SUBSET = ("tv", "atv", "v")  # non-canonical order; no pattern drops video
NC = 3 * 128
CASES = {
    "mosi": dict(name="mosi"),                                     # "last"
    "mosei": dict(name="mosei"),                                   # "maxpool", BatchNorm1d classifier
    "lengths": dict(name="mosi", lengths=True),                    # ragged + text_lengths
    "attn-time": dict(name="mosi", method="attention", norm="time"),
    "l1": dict(name="mosi", output_dim=1),                         # P*B = 35 <= 1024
    "subset": dict(name="mosi", patterns=SUBSET),
}
L1_WEIGHT = 0.5


def _rows(pats, ch):
    """The encoder row (of 2B) each replicated row (p, b) reads for modality ``ch``."""
    return torch.cat([torch.arange(B) + (0 if ch in p else B) for p in pats])


def _our_keeps(cfg, pats, seed):
    """Masks in OUR layout: "text" per encoder row [2B, nc], "cls{j}" per classifier row [P*B, w_j]."""
    g = torch.Generator().manual_seed(seed)
    out = {"text": (torch.rand(2 * B, NC, generator=g) >= cfg.text_dropout).to(torch.uint8)}
    for j, w in enumerate(cfg.cls_layers):
        out[f"cls{j}"] = (torch.rand(len(pats) * B, w, generator=g) >= cfg.cls_dropout).to(torch.uint8)
    return out


def _oracle_keeps(keeps, pats):
    """... mapped onto the replicated batch: the text mask of the encoder row each replicated row reads."""
    return dict(keeps, text=keeps["text"][_rows(pats, "t")])


def _replicate(A, V, T, y, pats, lengths):
    parts = [tp._masked(A, V, T, p) for p in pats]
    Ar, Vr, Tr = (torch.cat([q[i] for q in parts]) for i in range(3))
    lens = None if lengths is None else {k: list(v) * len(pats) for k, v in lengths.items()}
    return Ar, Vr, Tr, y.repeat(len(pats)), lens


def _decisions(eng, pats):
    """test_gpu_mosi._decisions for the replicated batch, read from the two halves of a MosiPatternEngine."""
    e, c, d = eng.enc, eng.cls, {}
    rt, C = _rows(pats, "t"), eng.enc.C
    for i in range(3):
        d[f"text.pool{i}"] = e.argmax[:, i * C:(i + 1) * C].long().cpu()[rt]
        d[f"text.relu{i}"] = (e.pooled[:, i * C:(i + 1) * C] > 0).cpu()[rt]
    col = eng.m.netA.hidden_size + eng.m.netV.hidden_size
    d["text.embd"] = (e.fused[:, col:] > 0).cpu()[rt]
    for j, h in enumerate(c.r if c.use_bn else c.h):
        d[f"cls.relu{j}"] = (h > 0).cpu()
    for name in ("a", "v"):
        if e.lstm[name]["arg"] is not None:
            d[f"lstm.{name}.pool"] = e.lstm[name]["arg"].long().cpu()[_rows(pats, name)]
    return d


def _oracle_run(o32, o64, rep, okeeps, forced, method, regress):
    """(r32, r64, t64): both oracles' train step (no optimizer, raw gradients) on the replicated batch."""
    Ar, Vr, Tr, yr, lens = rep
    t32, t64 = orc.MosiTrace(forced), orc.MosiTrace(forced)
    with tp._oracle_mode(method, lens):
        if regress is not None:
            r32 = tr._oracle_step(o32, Ar, Vr, Tr, yr, okeeps, t32, *regress)
            r64 = tr._oracle_step(o64, Ar.double(), Vr.double(), Tr.double(), yr, okeeps, t64, *regress)
        else:
            o32.clip = o64.clip = None
            r32 = orc.train_step(o32, None, Ar, Vr, Tr, yr, okeeps, t32)
            r64 = orc.train_step(o64, None, Ar.double(), Vr.double(), Tr.double(), yr, okeeps, t64)
    return r32, r64, t64


def _check(tag, ours, forced, logits, loss, o32, o64, rep, okeeps, method=None, regress=None):
    """The bounds of the module docstring for one step of ``ours`` (gradients in ``p.grad``), whichever engine ran it."""
    use_bn = ours.netC.use_bn
    r32, r64, t64 = _oracle_run(o32, o64, rep, okeeps, forced, method, regress)
    flips = (tl._flips_len if rep[4] is not None else tm._flips)(t64, forced, okeeps, use_bn)
    n = rep[3].numel()
    logits = logits.detach().cpu().reshape(n, -1)
    op_check(f"{tag} logits", logits, r32["logits"].reshape(n, -1), r64["logits"].reshape(n, -1))
    op_check(f"{tag} loss", loss.detach().cpu().reshape(1), r32["loss"].reshape(1), r64["loss"].reshape(1))
    if regress is None:
        nf = near_tie_flips(f"{tag} argmax", logits.argmax(1), r64["logits"].argmax(1), r64["logits"], 1)
        assert int((r32["logits"].argmax(1) != r64["logits"].argmax(1)).sum()) == 0, "choose another seed"
        if nf:
            print(f"{tag}: {nf} near-tie argmax flip")
    p32, p64 = dict(o32.named_parameters()), dict(o64.named_parameters())
    for name, p in ours.named_parameters():
        if not p.requires_grad:
            assert p.grad is None and p64[name].grad is None, name
            continue
        op_check(f"{tag} grad {name}", p.grad, p32[name].grad, p64[name].grad, grad=True)
    if use_bn:
        b32, b64 = dict(o32.named_buffers()), dict(o64.named_buffers())
        for name, b in ours.named_buffers():
            if name.endswith("num_batches_tracked"):
                assert int(b) == int(b64[name]), name
            else:
                op_check(f"{tag} {name}", b, b32[name], b64[name])
    return flips


def _model_args(c):
    return {k: v for k, v in c.items() if k in ("name", "method", "norm", "output_dim")}


def _setup(c, gpu, frozen=(), groups=False, seed=tp.SEED_MODEL):
    cfg = tp._cfg(c["name"])
    ours = tp._ours(**_model_args(c), seed=seed).to(gpu)
    for f in frozen:
        getattr(ours, tf.ATTR[f]).requires_grad_(False)
    if groups:
        opt = tspm_amd.FusedAdam(M.finetune_param_groups(ours, lr=1e-3, weight_decay=1e-3, encoder_lr=1e-4,
                                                         encoder_weight_decay=0.0))
    elif frozen:
        opt = tspm_amd.FusedAdam(M.finetune_param_groups(ours, lr=cfg.lr, weight_decay=cfg.weight_decay, freeze=frozen))
    else:
        opt = tspm_amd.FusedAdam(ours.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
    return cfg, ours, opt


def _oracles(ours, c, frozen=()):
    o32, o64 = pair_from(ours, tp._oracle_builder(**_model_args(c)))
    for o in (o32, o64):
        for f in frozen:
            getattr(o, tf.ATTR[f]).requires_grad_(False)
    return o32, o64


def _three_steps(gpu, key, frozen=(), groups=False, each=None):
    """Three checked steps of a case; ``each(s, ours, opt, st, before)`` runs after every step's checks."""
    c = CASES[key]
    pats = c.get("patterns", PATS)
    cfg, ours, opt = _setup(c, gpu, frozen, groups)
    regress = ("l1", L1_WEIGHT) if c.get("output_dim") == 1 else None
    group = tr.Group(*regress) if regress else None
    use_len = bool(c.get("lengths"))
    st = M.FusedMosiPatternStep(ours, opt, group, B, STEPS, patterns=pats, ragged=use_len, text_lengths=use_len)
    assert st.eng.P == len(pats) and st.eng.enc.B == 2 * B and st.eng.cls.B == len(pats) * B
    assert st.eng.rng_ctr_ptr == opt.flat_groups()[0].hyper.data_ptr() + tspm_amd._lib.HYPER_STEP_OFFSET
    graph = None
    for s in range(3):
        lengths = LENS[s] if use_len else None
        A, V, T, y = tp._batch(c["name"], s, lengths, regression=regress is not None)
        keeps = _our_keeps(cfg, pats, 50 + s)
        o32, o64 = _oracles(ours, c, frozen)
        before = tf._snap(ours, opt, s > 0)
        st.keep_override = {k: v.to(gpu) for k, v in keeps.items()}
        out = st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu), tp._dev(lengths, gpu))
        torch.cuda.synchronize()
        assert tuple(out["logits"].shape)[:2] == (len(pats), B)
        rep = _replicate(A, V, T, y, pats, lengths)
        flips = _check(f"{key} step {s + 1}", ours, _decisions(st.eng, pats), out["logits"], out["loss"], o32, o64, rep,
                       _oracle_keeps(keeps, pats), c.get("method"), regress)
        print(f"[{key} step {s + 1}] flips {flips}")
        if each is not None:
            each(s, ours, opt, st, before)
        if s == 1:
            graph = st.graph
            assert graph is not None  # captured on the second call
    assert st.graph is graph and st.calls == 3  # replayed on the third
    tp._zero_rows(st.eng)  # rows [B, 2B) of the three inputs: still zero after three different batches
    return ours, opt, st


@pytest.mark.parametrize("key", list(CASES))
def test_pattern_train_step_vs_fp64(gpu, key):
    _three_steps(gpu, key)


def test_plain_step_on_the_replicated_batch_meets_the_same_bounds(gpu):
    """The second yardstick (MOSI): ``FusedMosiStep`` at batch P*B on the replicated batch with the mapped masks, each
    step from its own state, under the same bounds against fp64 as the pattern step."""
    c = CASES["mosi"]
    cfg, ours, opt = _setup(c, gpu)
    n = len(PATS) * B
    st = M.FusedMosiStep(ours, opt, None, n, STEPS)
    for s in range(3):
        A, V, T, y = tp._batch("mosi", s)
        okeeps = _oracle_keeps(_our_keeps(cfg, PATS, 50 + s), PATS)
        rep = _replicate(A, V, T, y, PATS, None)
        o32, o64 = _oracles(ours, c)
        st.keep_override = {k: v.to(gpu) for k, v in okeeps.items()}
        out = st.step(rep[0].to(gpu), rep[1].to(gpu), rep[2].to(gpu), rep[3].to(gpu))
        torch.cuda.synchronize()
        _check(f"plain P*B step {s + 1}", ours, tm._decisions(st.eng), out["logits"], out["loss"], o32, o64, rep, okeeps)


def test_two_adam_groups_match_the_per_group_update(gpu):
    """Classifier group at lr 1e-3 / wd 1e-3, encoder group at lr 1e-4 / wd 0: the gradients under the bounds above, and
    every group's update at its own hyper-parameters (test_gpu_mosi_finetune._check_groups_adam: fp64 Adam on our
    gradient x the clip coefficient and our moments)."""
    def each(s, ours, opt, st, before):
        coef = tf._check_total(ours, st)
        tf._check_groups_adam(ours, opt, before, s + 1, coef)
        assert [int(fg.hyper.view(torch.int64)[6]) for fg in opt.flat_groups()] == [s + 1, s + 1]
    _, opt, st = _three_steps(gpu, "mosi", groups=True, each=each)
    assert st.multi and len(opt.flat_groups()) == 2


SENTINEL = 12345.0


def test_a_frozen_textcnn_is_left_alone(gpu):
    """netT frozen: the text columns of ``enc.dfused`` are never written (modalities = 0b011), netT's parameters are
    bitwise unchanged after three steps, have no gradient and no Adam state; the rest meets the bounds."""
    def each(s, ours, opt, st, before):
        col = WIDTHS[0] + WIDTHS[1]
        if s < 2:  # before the next step: a value no gradient takes, in every column
            st.eng.enc.dfused.fill_(SENTINEL)
        else:
            d = st.eng.enc.dfused
            assert bool((d[:, col:] == SENTINEL).all()), "the frozen encoder's columns were written"
            assert not bool((d[:, :col] == SENTINEL).any())
    ours, opt, st = _three_steps(gpu, "mosi", frozen=("text",), each=each)
    assert st.frozen == ("text",) and st.eng.enc.trains == {"a": True, "v": True, "t": False}
    for p, q in zip(ours.netT.parameters(), tp._ours("mosi").netT.parameters()):  # the same seed's initial values
        assert torch.equal(p.cpu(), q) and p.grad is None and p not in opt.state
    assert all(id(p) not in {id(x) for fg in opt.flat_groups() for x in fg.params} for p in ours.netT.parameters())


def test_all_encoders_frozen_never_write_the_embedding_gradients(gpu):
    def each(s, ours, opt, st, before):
        if s < 2:
            st.eng.enc.dfused.fill_(SENTINEL)
            st.eng.cls.dfused.fill_(SENTINEL)
        else:
            assert bool((st.eng.enc.dfused == SENTINEL).all()) and bool((st.eng.cls.dfused == SENTINEL).all())
    ours, opt, st = _three_steps(gpu, "mosei", frozen=("audio", "video", "text"), each=each)
    assert not any(st.eng.enc.trains.values()) and st.eng.enc.wg_ws is None


def test_two_models_of_one_seed_end_bitwise_equal_and_masks_change(gpu):
    """No ``keep_override``: the device draws the masks from (seed, step counter), so two models built from the same seed
    on the same batches end bitwise equal after three steps, and consecutive steps draw different masks."""
    res = []
    for _ in range(2):
        cfg, ours, opt = _setup(CASES["mosei"], gpu)
        st = M.FusedMosiPatternStep(ours, opt, None, B, STEPS)
        masks = []
        for s in range(3):
            A, V, T, y = tp._batch("mosei", s)
            st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
            masks.append((st.eng.enc.keeps[0].clone(), st.eng.cls.keeps[1].clone()))
        torch.cuda.synchronize()
        for s in range(2):
            assert not torch.equal(masks[s][0], masks[s + 1][0]) and not torch.equal(masks[s][1], masks[s + 1][1])
        assert tuple(masks[0][0].shape) == (2 * B, NC) and tuple(masks[0][1].shape) == (7 * B, cfg.cls_layers[0])
        kept = masks[0][0].float().mean().item()
        assert abs(kept - (1 - cfg.text_dropout)) < 0.05  # 3840 draws at keep probability 0.3: sigma 0.0074
        res.append([p.detach().clone() for p in ours.parameters()] + [b.detach().clone() for b in ours.buffers()]
                   + [st.eng.logits.clone(), st.eng.cls.loss.clone()] + [m for pair in masks for m in pair])
    for p, q in zip(*res):
        assert torch.equal(p, q)


def test_all_patterns_loader_runner_and_fit(gpu, tmp_path):
    """20 samples at batch 5: a train epoch on the ``all_patterns`` loader logs one loss per batch and B rows per batch
    in the confusion counts of every selected pattern; ``fit`` with it and a ``fuse_patterns`` valid loader runs two
    epochs and writes the usual metric keys; ``train_step`` takes such a batch and records P*B predictions."""
    N, S = 20, 6
    sel = ["v", "atv", "at"]
    ours = tp._ours("mosi").to(gpu)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=1e-3, weight_decay=1e-3)
    corpus = synthetic_mosi_corpus(N, seed=11, steps=S)
    tr_ds = MOSI(split="train", corpus=corpus, device=gpu, seed=4, selected_patterns=sel)
    va = MOSI(split="valid", corpus=corpus, device=gpu, selected_patterns=sel)
    runner = harness.runner_for(ours, opt, None)
    loader = tr_ds.loader(B, shuffle=True, seed=1, all_patterns=True)
    assert len(loader) == 4
    runner.loader_for(loader, True)
    dense = {m: torch.from_numpy(corpus.data[m]).reshape(N, S, -1) for m in ("audio", "video", "text")}
    seen = []
    for b in loader:  # gathered once, unmasked, into rows [0, B) of the step's inputs
        st = runner.train_pattern_step_for(B, S)
        assert isinstance(st, M.FusedMosiPatternStep) and st.patterns == tuple(sel) and st.log is runner.log
        assert b["all_patterns"] is True and b["patterns"] == sel
        assert "pattern_name" not in b and "fused_patterns" not in b
        assert b["audio"] is st.eng.A and b["label"] is st.eng.labels and b["time_major"] and b["steps"] == S
        lab = b["label"].cpu().numpy()
        rows = [int(np.flatnonzero((dense["audio"] == st.eng.A[:, i].cpu()).flatten(1).all(1))[0]) for i in range(B)]
        assert np.array_equal(lab, corpus.labels[rows]) and not bool(st.eng.A[:, B:].any())
        seen += rows
    assert sorted(seen) == list(range(N)) and seen != list(range(N))  # each sample once, shuffled
    loss, _, metrics, n = runner.train_epoch(loader)
    conf, losses, samples = runner.log.fetch()
    assert n == 4 == len(losses) and np.isfinite(loss) and samples == len(sel) * N  # one loss entry per batch
    per_group = conf.sum(axis=(1, 2)).tolist()
    assert per_group == [N if p in sel else 0 for p in PATTERNS]  # B rows per batch for every selected pattern
    assert ours._fused_step_key(opt, None, B, S, patterns=sel) in ours._steps and len(ours._steps) == 1
    loaders = {"train": loader, "validation": va.loader(B, fuse_patterns=True)}
    hist = harness.fit(ours, opt, None, loaders, epochs=2, early_stopping=False, metrics_path=tmp_path)
    assert len(hist["epoch_metrics"]) == 2
    for block in hist["epoch_metrics"]:
        assert set(block) == {"epoch", "train", "validation"}
        for split in ("train", "validation"):
            assert np.isfinite(block[split]["loss"]) and "timing" in block[split]
            assert any(k.startswith("MSA_") and k.endswith("_ATV") for k in block[split]["metrics"])
    plain = harness.runner_for(ours, opt, None).validate_epoch(va.loader(B))[2]
    assert list(hist["train"][0]) == list(hist["validation"][0]) == list(dict(plain, loss=0.0))
    assert (tmp_path / "epoch_metrics.json").exists()

    class Rec:
        def update_group_all(self, group, **kw):
            self.group, self.kw = group, kw
    rec = Rec()
    batch = {"audio": dense["audio"][:B], "video": dense["video"][:B], "text": dense["text"][:B],
             "label": torch.from_numpy(corpus.labels[:B]), "all_patterns": True, "patterns": sel}
    out = ours.train_step(batch, opt, None, gpu, rec)
    assert np.isfinite(out["loss"]) and rec.group == "classification"
    assert rec.kw["predictions"].shape == (3 * B,) and rec.kw["m_types"].tolist() == [p for p in sel for _ in range(B)]
    assert np.array_equal(rec.kw["targets"], np.tile(corpus.labels[:B], 3))


def test_refusals_name_the_limit(gpu):
    ours = tp._ours("mosi").to(gpu)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=1e-3, weight_decay=1e-3)
    A, V, T, y = tp._batch("mosi", 0)
    batch = {"audio": A, "video": V, "text": T, "label": y, "all_patterns": True, "patterns": list(PATS)}
    with pytest.raises(tspm_amd.TspmError, match="fused step only"):
        ours.train_step(batch, torch.optim.Adam(ours.parameters()), None, gpu, None)
    with pytest.raises(tspm_amd.TspmError, match="allreduce"):
        M.FusedMosiPatternStep(ours, opt, None, B, STEPS, allreduce=lambda: None)
    reg = tp._ours("mosi", output_dim=1).to(gpu)
    ropt = tspm_amd.FusedAdam(reg.parameters(), lr=1e-3, weight_decay=1e-3)
    with pytest.raises(tspm_amd.TspmError, match="at most 1024 rows"):  # 7 x 147 = 1029 rows for the one-launch head
        M.FusedMosiPatternStep(reg, ropt, tr.Group("l1", 1.0), 147, STEPS)
    M.FusedMosiPatternStep(reg, ropt, tr.Group("l1", 1.0), 146, STEPS, patterns=("atv",))  # 146 rows: accepted
    with pytest.raises(ValueError, match="Invalid patterns"):
        M.FusedMosiPatternStep(ours, opt, None, B, STEPS, patterns=["q"])
    with pytest.raises(tspm_amd.TspmError, match="backward=True"):
        ours._pattern_engine(B, STEPS, gpu).forward(tspm_amd._lib.stream_handle(), train=True)
    st = M.FusedMosiPatternStep(ours, opt, None, B, STEPS)
    st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
    ours.netA.requires_grad_(False)
    with pytest.raises(tspm_amd.TspmError, match="requires_grad flags changed"):
        st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
