"""Per-sample text lengths in the UTT-Fusion TextCNN, model level: the ``text_lengths`` mode of MosiEngine / FusedMosiStep /
FusedMosiEvalStep / MonomodalEncoder(TextCNN) and the loader's ``text_lengths``.

The oracle is oracle/mosi_ref.py with its TextCNN forward replaced, here, by the length-aware restatement of
tests/textcnn_len_ref.py (held to the oracle itself, row by row, in test_mosi_text_lengths_cpu.py) beside the LSTM
restatement of test_gpu_mosi_lengths.py (``LenOracle``); the checks, tolerances, forced decisions and dropout-mask
injection are those of test_gpu_mosi.py (``_check_step``).  The seeds of the fused-step test were chosen so
that the fp32 CPU reference's own decisions, forced into the fp64 reference, report no near-tie flip.
"""
import numpy as np
import pytest
import torch

import test_gpu_mosi as tm
import test_gpu_mosi_lengths as tl
import test_gpu_mosi_mono as tmm
import tspm_amd
from oracle import mosi_ref as orc
from parity import Tally, check_adam, check_grad, check_out, pair_from, snapshot
from test_mosi_cpu import _dropin
from textcnn_len_ref import TextLenOracle
from tspm_amd import mosi as M
from tspm_amd.monomodal import FusedMosiMonoEvalStep, FusedMosiMonoStep, fit_monomodal
from tspm_amd.mosi_data import MOSI, synthetic_mosi_corpus

pytestmark = pytest.mark.gpu
B, STEPS = 6, (9, 11, 8)
LENS = [{"audio": [9, 1, 4, 4, 7, 2], "video": [11, 3, 3, 8, 1, 6], "text": [8, 1, 4, 5, 2, 7]},
        {"audio": [2, 9, 5, 1, 8, 8], "video": [4, 10, 1, 11, 2, 7], "text": [3, 8, 6, 1, 8, 4]},
        {"audio": [6, 6, 3, 9, 1, 5], "video": [1, 2, 9, 5, 11, 4], "text": [5, 2, 8, 3, 7, 1]}]
SEEDS = dict(model=3, batch=100, keep=50)


def _patch(monkeypatch, lengths):
    tl._patch(monkeypatch, lengths)  # the LSTM restatement and its flip count
    monkeypatch.setattr(orc, "textcnn_forward", TextLenOracle(lengths["text"]))


def _batch(cfg, lengths, steps=STEPS, seed=77, text_scale=0.3):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(B, steps[0], cfg.audio_dim, generator=g)
    V = 0.5 * torch.randn(B, steps[1], cfg.video_dim, generator=g)
    T = text_scale * torch.randn(B, steps[2], cfg.text_dim, generator=g)
    for i in range(B):  # zero padding past each sample's length, as pad_sequence leaves it
        A[i, lengths["audio"][i]:] = 0
        V[i, lengths["video"][i]:] = 0
        T[i, lengths["text"][i]:] = 0
    return A, V, T, torch.randint(0, 3, (B,), generator=g)


_dev = tl._dev_lengths


# ------------------------------------------------------------------------------------------------
# padding invariance
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["atv", "av"])
def test_logits_do_not_depend_on_the_text_padding(gpu, pattern):
    """Text padded to 8 and to 14 steps: with all three lengths the logits and the three embedding slices are bitwise
    equal; without the ``"text"`` key the text slice and the logits differ.  Under "av" the text is the zeroed tensor
    the dataset delivers: every window is relu(bias), so there the two paddings agree with or without lengths and only
    the equality is asserted."""
    torch.manual_seed(5)
    model = M.build_utt_fusion("mosi", embd_sizes=(8, 12, 8)).to(gpu).eval()
    lengths = LENS[0]
    A, V, T, _ = _batch(orc.MOSI, lengths)
    if pattern == "av":
        T = torch.zeros_like(T)
    T2 = torch.zeros(B, 14, T.shape[2])
    T2[:, :STEPS[2]] = T
    dl = _dev(lengths, gpu)
    no_text = {k: v for k, v in dl.items() if k != "text"}
    out = {}
    for name, t, steps in (("tight", T, STEPS), ("wide", T2, (9, 11, 14))):
        for with_text in (True, False):
            with torch.no_grad():
                logits = model(A.to(gpu), V.to(gpu), t.to(gpu), lengths=dl if with_text else no_text)
            eng = model._engine(B, steps, gpu, True, with_text)
            assert eng.text_lengths == with_text and (eng.text_lens is not None) == with_text
            out[name, with_text] = (eng.fused[:, :8].clone(), eng.fused[:, 8:20].clone(), eng.fused[:, 20:].clone(),
                                    logits.clone())
    for x, y in zip(out["tight", True], out["wide", True]):
        assert torch.equal(x, y)  # bitwise: audio, video and text embeddings, logits
    if pattern == "atv":
        assert not torch.equal(out["tight", False][2], out["wide", False][2])  # the padding competes in the time-max
        assert not torch.equal(out["tight", False][3], out["wide", False][3])
        assert torch.equal(out["tight", False][0], out["tight", True][0])  # the LSTM slices do not see the text lengths
        # text-only lengths: no ragged recurrences, the text slice is the same
        with torch.no_grad():
            model(A.to(gpu), V.to(gpu), T.to(gpu), lengths={"text": dl["text"]})
        eng = model._engine(B, STEPS, gpu, False, True)
        assert eng.lens is None and torch.equal(eng.fused[:, 20:], out["tight", True][2])
        # the standalone encoder takes the same lengths
        assert torch.equal(model.netT(T.to(gpu), dl["text"]), out["tight", True][2])
        assert torch.equal(model.netT(T2.to(gpu), dl["text"]), out["tight", True][2])
        assert not torch.equal(model.netT(T2.to(gpu)), model.netT(T.to(gpu)))


# ------------------------------------------------------------------------------------------------
# fused train steps against fp64, one graph for every length vector
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mosi", "mosei"])
def test_text_length_fused_steps_vs_fp64_with_one_graph(gpu, monkeypatch, name):
    cfg = orc.MOSI if name == "mosi" else orc.MOSEI
    ours = _dropin(SEEDS["model"], cfg=cfg).to(gpu)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
    st = ours.fused_step(opt, None, B, STEPS, ragged=True, text_lengths=True)
    assert st.ragged and st.text_lengths and st.eng.text_lens is not None
    assert st is ours.fused_step(opt, None, B, STEPS, ragged=True, text_lengths=True)
    assert list(ours._steps) == [(id(opt), id(None), B, M.norm_steps(STEPS), "ragged", "text_lengths")]
    tally, graph = Tally(), None
    for s, lengths in enumerate(LENS):
        _patch(monkeypatch, lengths)
        A, V, T, y = _batch(cfg, lengths, seed=SEEDS["batch"] + s)
        keeps = orc.keep_masks(B, SEEDS["keep"] + s, cfg=cfg)
        o32, o64 = pair_from(ours, lambda: orc.build_oracle_utt(SEEDS["model"], cfg=cfg))  # re-anchored to our state
        before = snapshot(ours, opt if s else None)
        st.keep_override = {k: v.to(gpu) for k, v in keeps.items()}
        out = st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu), _dev(lengths, gpu))
        torch.cuda.synchronize()
        C = st.eng.C
        for i, kh in enumerate((3, 4, 5)):  # every stored index inside the row's own windows
            nw = torch.tensor([max(n - kh + 1, 1) for n in lengths["text"]])
            assert bool((st.eng.argmax[:, i * C:(i + 1) * C].long().cpu() < nw[:, None]).all())
        rep = tm._check_step(ours, st, o32, o64, A, V, T, y, keeps, out, tally)
        coef = float(st.eng.clip_coef.item())
        tm._check_adam(ours, opt, before, s + 1, coef, cfg)
        print(f"[{name} text-length step {s + 1}] flips {rep} clip coef {coef:.4f}")
        if s == 1:
            graph = st.graph
            assert graph is not None  # captured on the second call
        if s == 2:
            assert st.graph is graph  # replayed, not recaptured, with new length vectors
    assert len(ours._steps) == 1 and st.calls == 3
    print(tally)


# ------------------------------------------------------------------------------------------------
# text_lengths off: the existing steps, keys and bits; on at full lengths: the same bits through the other kernel
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ragged", [False, True])
def test_the_off_path_keeps_its_keys_and_bits(gpu, ragged):
    cfg, lengths = orc.MOSI, LENS[0]
    A, V, T, y = _batch(cfg, lengths)
    dl = {k: v for k, v in _dev(lengths, gpu).items() if k != "text"} if ragged else None
    tag = ("ragged",) if ragged else ()
    params = []
    for mode in ("off", "direct", "full"):
        m = _dropin(4, cfg=cfg).to(gpu)
        opt = tspm_amd.FusedAdam(m.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
        if mode == "off":  # through the cache with the new keyword at its default / False
            st = m.fused_step(opt, None, B, STEPS, ragged=ragged)
            assert st is m.fused_step(opt, None, B, STEPS, ragged=ragged, text_lengths=False)
            assert list(m._steps) == [(id(opt), id(None), B, M.norm_steps(STEPS)) + tag]  # the key as it always was
            assert not st.text_lengths and st.eng.text_lens is None
            m._engine(B, STEPS, gpu, ragged)
            assert list(m._engines) == [(B, M.norm_steps(STEPS), gpu) + tag]
            with pytest.raises(tspm_amd._lib.TspmError):  # "text" needs a text_lengths step
                st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu), {"text": _dev(lengths, gpu)["text"]})
        elif mode == "direct":  # the step class as callers built it before
            st = M.FusedMosiStep(m, opt, None, B, STEPS, ragged=ragged)
        else:  # text_lengths on, no "text" key: every row at the padded length, through tspm_textcnn_pool_fwd_len
            st = m.fused_step(opt, None, B, STEPS, ragged=ragged, text_lengths=True)
            assert list(m._steps) == [(id(opt), id(None), B, M.norm_steps(STEPS)) + tag + ("text_lengths",)]
        for s in range(3):
            st.keep_override = {k: v.to(gpu) for k, v in orc.keep_masks(B, 60 + s, cfg=cfg).items()}
            if dl is None and mode != "full":
                st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
            else:
                st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu), dl if dl is not None else {})
        torch.cuda.synchronize()
        params.append([p.detach().clone() for p in m.parameters()] + [st.eng.logits.clone(), st.eng.loss.clone()])
    for other in params[1:]:
        for p, q in zip(params[0], other):
            assert torch.equal(p, q)


# ------------------------------------------------------------------------------------------------
# monomodal
# ------------------------------------------------------------------------------------------------
def test_monomodal_textcnn_step_vs_fp64(gpu, monkeypatch):
    feat, T = 768, 8
    lens = LENS[0]["text"]
    monkeypatch.setattr(orc, "textcnn_forward", TextLenOracle(lens))
    ours = tmm._ours("textcnn", feat, gpu, 3)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=tmm.LR, weight_decay=tmm.WD)
    x, y = tmm._batch("textcnn", feat, B, T, 1234)
    for i in range(B):
        x[i, lens[i]:] = 0
    keep = tmm._keep("textcnn", B, 50)
    o32, o64 = pair_from(ours, lambda: tmm.OracleMono(tmm.CASES["textcnn"][1](feat)))
    before = snapshot(ours, None)
    dl = torch.tensor(lens, dtype=torch.int32, device=gpu)
    with pytest.raises(tspm_amd._lib.TspmError):  # a step built without the mode takes no lengths
        FusedMosiMonoStep(ours, opt, None, (B, T, feat)).step(x.to(gpu), y.to(gpu), dl)
    st = FusedMosiMonoStep(ours, opt, None, (B, T, feat), text_lengths=True)
    ours._fused = st
    st.keep_override = {"text": keep.to(gpu)}
    batch = {"text": x.to(gpu), "label": y.to(gpu), "lengths": dl}
    res = ours.train_step(batch, opt, None, gpu, None)  # the public path: batch.get("lengths") -> the text_lengths step
    assert ours._fused is st and st.text_lengths and not st.ragged and st.eng.text_lens is not None
    torch.cuda.synchronize()
    forced = tmm._decisions(st.eng)
    t32, t64 = orc.MosiTrace(forced), orc.MosiTrace(forced)
    r32 = tmm._oracle_step(o32, x, y, keep, t32)
    r64 = tmm._oracle_step(o64, x.double(), y, keep, t64)
    print("flips", tm._flips(t64, forced, {}))
    tally = Tally()
    check_out("logits", st.logits, r32["logits"], r64["logits"], tally)
    check_out("loss", st.loss, r32["loss"].reshape(1), r64["loss"].reshape(1), tally)
    assert abs(res["loss"] - float(r64["loss"])) <= 1e-4 * abs(float(r64["loss"]))
    p32, p64 = dict(o32.named_parameters()), dict(o64.named_parameters())
    for n, p in ours.named_parameters():
        check_grad(f"grad {n}", p.grad, p32[n].grad, p64[n].grad, tally)
    check_adam(ours, opt, *before, 1, lr=tmm.LR, wd=tmm.WD)
    print(tally)


def test_fit_monomodal_reads_the_datasets_text_lengths(gpu, tmp_path):
    ours = tmm._ours("textcnn", 768, gpu, 0)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=tmm.LR, weight_decay=tmm.WD)
    kw = dict(target_modality="text", selected_patterns=["t"], device=gpu, use_lengths=True, text_lengths=True)
    tr_corpus = synthetic_mosi_corpus(24, seed=5, steps=12, min_len=2)
    tr = MOSI(corpus=tr_corpus, split="train", **kw)
    va = MOSI(corpus=synthetic_mosi_corpus(8, seed=6, steps=12, min_len=2), split="valid", **kw)
    b = next(iter(tr.device_loader(8, pad_to=12)))
    assert list(b) == ["text", "label", "pattern_name", "lengths"]
    assert np.array_equal(b["lengths"].cpu().numpy(), tr_corpus.lengths["text"][:8])
    off = MOSI(corpus=tr_corpus, split="train", **{**kw, "text_lengths": False})
    assert "lengths" not in next(iter(off.device_loader(8, pad_to=12)))  # use_lengths alone: as before
    loaders = {"train": tr.loader(8, shuffle=True, seed=0, pad_to=12), "validation": va.loader(8, pad_to=12)}
    h = fit_monomodal(ours, opt, None, loaders, 1, experiment_name="MOSI_Text_Encoder_Pretrain",
                      model_output_path=tmp_path)
    assert np.isfinite(h["metrics_history"]["train"][0]["loss"]) and np.isfinite(h["metrics_history"]["validation"][0]["loss"])
    steps = list(ours._by_buffer.values())
    assert steps and all(st.text_lengths and not st.ragged for st in steps)
    train = [st for st in steps if isinstance(st, FusedMosiMonoStep)]
    assert len(train) == 1 and train[0].graph is not None  # 3 batches of one padded shape: one step, one graph
    # the eval step's embedding is the standalone encoder's with the same lengths
    ours.eval()
    est = [st for st in steps if isinstance(st, FusedMosiMonoEvalStep)][0]
    x = est.X.transpose(0, 1).contiguous()
    assert torch.equal(ours.encoder(x, est.eng.text_lens), est.emb)
    assert not torch.equal(ours.encoder(x), est.emb)


# ------------------------------------------------------------------------------------------------
# the other readers of batch["lengths"]
# ------------------------------------------------------------------------------------------------
def test_autograd_validation_and_embedding_paths_take_the_text_lengths(gpu):
    from parity import rel_l2
    cfg, lengths = orc.MOSI, LENS[1]
    A, V, T, y = _batch(cfg, lengths)
    keeps = {k: v.to(gpu) for k, v in orc.keep_masks(B, 9, cfg=cfg).items()}
    dl = _dev(lengths, gpu)
    fused = _dropin(6, cfg=cfg).to(gpu)
    opt = tspm_amd.FusedAdam(fused.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
    st = fused.fused_step(opt, None, B, STEPS, ragged=True, text_lengths=True)
    st.keep_override = keeps
    st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu), dl)
    auto = _dropin(6, cfg=cfg).to(gpu).train()
    auto._engine(B, STEPS, gpu, True, True).keep_override = keeps
    logits = auto(A.to(gpu), V.to(gpu), T.to(gpu), lengths=dl)  # the autograd node
    torch.nn.functional.cross_entropy(logits, y.to(gpu)).backward()
    torch.cuda.synchronize()
    assert rel_l2(logits, st.eng.logits) <= 1e-6
    for (n, p), (_, q) in zip(auto.named_parameters(), fused.named_parameters()):
        assert rel_l2(p.grad, q.grad) <= 1e-5, n
    # train_step reads batch["lengths"]["text"]: the text_lengths step of the cache
    batch = {"audio": A, "video": V, "text": T, "label": y, "lengths": dl}
    fused.train_step(batch, opt, None, gpu, None)
    assert st.calls == 2 and len(fused._steps) == 1
    # validation_step and get_embeddings
    auto.eval()
    with torch.no_grad():
        ref = auto(A.to(gpu), V.to(gpu), T.to(gpu), lengths=dl).clone()
    emb_ref = auto._engine(B, STEPS, gpu, True, True).fused.clone()
    out = auto.validation_step(batch, None, gpu, None)
    assert torch.equal(auto._engine(B, STEPS, gpu, True, True).logits, ref)
    assert abs(out["loss"] - float(torch.nn.functional.cross_entropy(ref, y.to(gpu)))) <= 1e-5
    emb = auto.get_embeddings([batch], gpu)
    assert np.array_equal(emb["text"][0], emb_ref[:, 128:].cpu().numpy())
    assert np.array_equal(emb["audio"][0], emb_ref[:, :64].cpu().numpy())
    no_text = {**batch, "lengths": {k: v for k, v in dl.items() if k != "text"}}
    other = auto.get_embeddings([no_text], gpu)
    assert not np.array_equal(other["text"][0], emb["text"][0])
    assert np.array_equal(other["audio"][0], emb["audio"][0])
    # the eval step of the harness's kind
    from tspm_amd.metrics import ClassificationLog
    from tspm_amd.mosi_data import PATTERNS
    log = ClassificationLog(gpu, groups=PATTERNS, classes=3)
    ev = M.FusedMosiEvalStep(auto, None, B, STEPS, log, ragged=True, text_lengths=True)
    ev.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu), dl)
    assert ev.eng is auto._engine(B, STEPS, gpu, True, True) and torch.equal(ev.eng.logits, ref)


# ------------------------------------------------------------------------------------------------
# loader and fit
# ------------------------------------------------------------------------------------------------
def test_loader_hands_the_text_lengths_to_the_steps(gpu):
    from tspm_amd import harness
    corpus = synthetic_mosi_corpus(n=24, steps=12, min_len=2)
    ds = MOSI(split="train", corpus=corpus, device=gpu, seed=4, use_lengths=True, text_lengths=True)
    ours = _dropin(8).to(gpu)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=1e-3, weight_decay=1e-3)
    made = []

    def step_for(b, t):
        made.append(ours.fused_step(opt, None, b, t, ragged=True, text_lengths=True))
        return made[-1]
    order = np.arange(24)
    for i, batch in enumerate(ds.device_loader(8, step_for=step_for, pad_to=12)):
        e = made[-1].eng
        idx = order[i * 8:(i + 1) * 8]
        assert batch["lengths"]["text"] is e.text_lens and batch["lengths"]["audio"] is e.lens["a"]
        assert np.array_equal(e.text_lens.cpu().numpy(), corpus.lengths["text"][idx])
        x = e.X.cpu()  # time-major [T, B, F]: zero past each row's length
        for r, n in enumerate(corpus.lengths["text"][idx]):
            assert not bool(x[int(n):, r].any())
    assert len(made) == 3 and all(m is made[0] for m in made)
    other = _dropin(8).to(gpu)  # a step without the text length buffer is refused by the loader
    oopt = tspm_amd.FusedAdam(other.parameters(), lr=1e-3, weight_decay=1e-3)
    with pytest.raises(tspm_amd._lib.TspmError):
        next(iter(ds.device_loader(8, step_for=lambda b, t: other.fused_step(oopt, None, b, t, ragged=True), pad_to=12)))
    # without a step the batch dict carries them
    batch = next(iter(ds.device_loader(8, pad_to=12)))
    assert list(batch["lengths"]) == ["audio", "video", "text"] and batch["lengths"]["text"].dtype == torch.int32
    assert np.array_equal(batch["lengths"]["text"].cpu().numpy(), corpus.lengths["text"][:8])
    # fit: one epoch of 3 batches on the one text_lengths step, finite loss; the runner reads the dataset's flag
    loaders = {"train": ds.loader(8, shuffle=True, seed=1, pad_to=12),
               "validation": MOSI(split="valid", corpus=synthetic_mosi_corpus(n=6, steps=12, min_len=2, seed=2),
                                  device=gpu, use_lengths=True, text_lengths=True).loader(6, pad_to=12)}
    hist = harness.fit(ours, opt, None, loaders, epochs=1, early_stopping=False)
    assert np.isfinite(hist["train"][-1]["loss"]) and np.isfinite(hist["validation"][-1]["loss"])
    assert made[0].calls == 3 and [k[-2:] for k in ours._steps] == [("ragged", "text_lengths")]
    assert any(k[-2:] == ("ragged", "text_lengths") for k in ours._engines)
