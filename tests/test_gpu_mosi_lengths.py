"""Per-sample sequence lengths in the UTT-Fusion LSTM encoders, model level: the ``ragged`` mode of MosiEngine /
FusedMosiStep / MonomodalEncoder and the loader's ``use_lengths``.

The oracle is oracle/mosi_ref.py with its LSTM forward replaced, here, by the length-aware restatement of
test_gpu_lstm_len.py (``len_cell_loop``: row b runs its own L_b steps, checked there against pack_padded_sequence); the
checks, tolerances, forced decisions and dropout-mask injection are those of test_gpu_mosi.py (``_check_step``).  The
"maxpool" index is compared with the restatement's own masked index through near_tie_flips.
"""
import numpy as np
import pytest
import torch

import test_gpu_mosi as tm
import test_gpu_mosi_mono as tmm
import tspm_amd
from oracle import mosi_ref as orc
from parity import Tally, check_adam, check_grad, check_out, near_tie_flips, pair_from, snapshot
from test_gpu_lstm_len import last_of, len_cell_loop, len_embedding, masked_pool
from test_mosi_cpu import _dropin
from tspm_amd import mosi as M
from tspm_amd.monomodal import FusedMosiMonoStep
from tspm_amd.mosi_data import MOSI, MosiCorpus, synthetic_mosi_corpus

pytestmark = pytest.mark.gpu
B, STEPS = 6, (9, 11, 6)
_FLIPS = tm._flips  # the original, before a test patches the module attribute
LENS = [{"audio": [9, 1, 4, 4, 7, 2], "video": [11, 3, 3, 8, 1, 6]},
        {"audio": [2, 9, 5, 1, 8, 8], "video": [4, 10, 1, 11, 2, 7]},
        {"audio": [6, 6, 3, 9, 1, 5], "video": [1, 2, 9, 5, 11, 4]}]


class LenOracle:
    """Replacement of oracle.mosi_ref.lstm_forward: the length-aware restatement, differentiable, with MosiTrace's
    forcing of the "maxpool" index; ``lengths``: {"audio": [...], "video": [...]} (a missing name: full length)."""

    def __init__(self, lengths):
        self.lengths = lengths

    def __call__(self, enc, x, trace=None, site="lstm"):
        Bn, T, _ = x.shape
        lens = self.lengths.get("audio" if ".a." in site else "video") or [T] * Bn
        rnn = enc.rnn
        xg = (x.transpose(0, 1).reshape(T * Bn, -1) @ rnn.weight_ih_l0.T + rnn.bias_ih_l0).reshape(T, Bn, -1)
        _, _, hs, _ = len_cell_loop(xg, rnn.weight_hh_l0, rnn.bias_hh_l0, lens, x.dtype)
        if enc.embd_method == "last":
            return last_of(hs, lens)
        own = masked_pool(hs.detach(), lens)[1]
        idx = own
        if trace is not None:
            trace.pre[site], trace.idx[site] = hs[1:].transpose(0, 1).detach(), own  # [B, T, H], [B, H]
            if trace.force is not None and site in trace.force:
                idx = trace.force[site]
        return len_embedding(hs, lens, idx)


def _flips_len(t64, forced, keeps, use_bn=False):
    """test_gpu_mosi._flips with the LSTM sites compared against the restatement's masked index."""
    rest = {k: v for k, v in forced.items() if not k.startswith("lstm.")}
    rep = _FLIPS(t64, rest, keeps, use_bn)
    for site, f in forced.items():
        if site.startswith("lstm."):
            nf = near_tie_flips(site, f, t64.idx[site], t64.pre[site].double().transpose(1, 2), 2)
            if nf:
                rep[site] = nf
    return rep


def _patch(monkeypatch, lengths):
    monkeypatch.setattr(orc, "lstm_forward", LenOracle(lengths))
    monkeypatch.setattr(tm, "_flips", _flips_len)


def _batch(cfg, lengths, steps=STEPS, seed=77):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(B, steps[0], cfg.audio_dim, generator=g)
    V = 0.5 * torch.randn(B, steps[1], cfg.video_dim, generator=g)
    T = 0.3 * torch.randn(B, steps[2], cfg.text_dim, generator=g)
    for i in range(B):  # zero padding past each sample's length, as pad_sequence leaves it
        A[i, lengths["audio"][i]:] = 0
        V[i, lengths["video"][i]:] = 0
    return A, V, T, torch.randint(0, 3, (B,), generator=g)


def _dev_lengths(lengths, dev):
    return {k: torch.tensor(v, dtype=torch.int32, device=dev) for k, v in lengths.items()}


# ------------------------------------------------------------------------------------------------
# padding invariance
# ------------------------------------------------------------------------------------------------
def test_embeddings_do_not_depend_on_the_padding(gpu):
    torch.manual_seed(5)
    model = M.build_utt_fusion("mosi", embd_sizes=(8, 12, 8)).to(gpu).eval()
    lengths = LENS[0]
    A, V, T, _ = _batch(orc.MOSI, lengths)
    wide = (16, 18, 6)
    A2, V2 = torch.zeros(B, wide[0], A.shape[2]), torch.zeros(B, wide[1], V.shape[2])
    A2[:, :STEPS[0]], V2[:, :STEPS[1]] = A, V
    out = {}
    for name, (a, v), steps in (("tight", (A, V), STEPS), ("wide", (A2, V2), wide)):
        for ragged in (True, False):
            with torch.no_grad():
                logits = model(a.to(gpu), v.to(gpu), T.to(gpu), lengths=_dev_lengths(lengths, gpu) if ragged else None)
            eng = model._engine(B, steps, gpu, ragged)
            out[name, ragged] = (eng.fused[:, :8].clone(), eng.fused[:, 8:20].clone(), logits.clone())
    for x, y in zip(out["tight", True], out["wide", True]):
        assert torch.equal(x, y)  # bitwise: audio embedding, video embedding, logits
    assert not torch.equal(out["tight", False][0], out["wide", False][0])  # without lengths the padding leaks in
    assert not torch.equal(out["tight", False][1], out["wide", False][1])
    assert not torch.equal(out["tight", False][2], out["wide", False][2])
    # a single key: the other encoder runs the full padded length
    with torch.no_grad():
        model(A.to(gpu), V.to(gpu), T.to(gpu), lengths={"audio": _dev_lengths(lengths, gpu)["audio"]})
    eng = model._engine(B, STEPS, gpu, True)
    assert torch.equal(eng.fused[:, :8], out["tight", True][0]) and torch.equal(eng.fused[:, 8:20], out["tight", False][1])
    # the standalone encoder takes the same lengths
    emb = model.netA(A.to(gpu), _dev_lengths(lengths, gpu)["audio"])
    assert torch.equal(emb, out["tight", True][0])


# ------------------------------------------------------------------------------------------------
# fused train steps against fp64, one graph for every length vector
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mosi", "mosei"])
def test_ragged_fused_steps_vs_fp64_with_one_graph(gpu, monkeypatch, name):
    cfg = orc.MOSI if name == "mosi" else orc.MOSEI
    seed = 3
    ours = _dropin(seed, cfg=cfg).to(gpu)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
    st = ours.fused_step(opt, None, B, STEPS, ragged=True)
    assert st.ragged and st.eng.ragged and st is ours.fused_step(opt, None, B, STEPS, ragged=True)
    tally, graph = Tally(), None
    for s, lengths in enumerate(LENS):
        _patch(monkeypatch, lengths)
        A, V, T, y = _batch(cfg, lengths, seed=100 + s)
        keeps = orc.keep_masks(B, 50 + s, cfg=cfg)
        o32, o64 = pair_from(ours, lambda: orc.build_oracle_utt(seed, cfg=cfg))  # re-anchored to our state
        before = snapshot(ours, opt if s else None)
        st.keep_override = {k: v.to(gpu) for k, v in keeps.items()}
        out = st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu), _dev_lengths(lengths, gpu))
        torch.cuda.synchronize()
        rep = tm._check_step(ours, st, o32, o64, A, V, T, y, keeps, out, tally)
        coef = float(st.eng.clip_coef.item())
        tm._check_adam(ours, opt, before, s + 1, coef, cfg)
        print(f"[{name} ragged step {s + 1}] flips {rep} clip coef {coef:.4f}")
        if s == 1:
            graph = st.graph
            assert graph is not None  # captured on the second call
        if s == 2:
            assert st.graph is graph  # replayed, not recaptured, with a new length vector
    assert len(ours._steps) == 1 and st.calls == 3
    print(tally)


# ------------------------------------------------------------------------------------------------
# no lengths given: the existing path, bit for bit
# ------------------------------------------------------------------------------------------------
def test_without_lengths_the_existing_path_and_keys(gpu):
    cfg = orc.MOSI
    A, V, T, y = _batch(cfg, LENS[0])
    models = []
    for via_cache in (True, False):
        m = _dropin(4, cfg=cfg).to(gpu)
        opt = tspm_amd.FusedAdam(m.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
        st = m.fused_step(opt, None, B, STEPS) if via_cache else M.FusedMosiStep(m, opt, None, B, STEPS)
        assert not st.ragged and st.eng.lens is None
        for s in range(3):
            st.keep_override = {k: v.to(gpu) for k, v in orc.keep_masks(B, 60 + s, cfg=cfg).items()}
            if via_cache:
                st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu), lengths=None)
            else:
                st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
        if via_cache:
            assert list(m._steps) == [(id(opt), id(None), B, M.norm_steps(STEPS))]  # the key as it always was
            m._engine(B, STEPS, gpu)
            assert list(m._engines) == [(B, M.norm_steps(STEPS), gpu)]
            m._engine(B, STEPS, gpu, True)
            assert list(m._engines)[1] == (B, M.norm_steps(STEPS), gpu, "ragged")
        models.append(m)
    torch.cuda.synchronize()
    for (n, p), (_, q) in zip(models[0].named_parameters(), models[1].named_parameters()):
        assert torch.equal(p, q), n
    with pytest.raises(tspm_amd._lib.TspmError):  # lengths need a ragged step
        st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu), _dev_lengths(LENS[0], gpu))


# ------------------------------------------------------------------------------------------------
# monomodal
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lstm_last", "lstm_maxpool"])
def test_monomodal_ragged_step_vs_fp64(gpu, monkeypatch, kind):
    feat, T = 5, 9
    lens = LENS[0]["audio"]
    monkeypatch.setattr(orc, "lstm_forward", LenOracle({"audio": lens}))
    ours = tmm._ours(kind, feat, gpu, 3)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=tmm.LR, weight_decay=tmm.WD)
    x, y = tmm._batch(kind, feat, B, T, 1234)
    for i in range(B):
        x[i, lens[i]:] = 0
    o32, o64 = pair_from(ours, lambda: tmm.OracleMono(tmm.CASES[kind][1](feat)))
    before = snapshot(ours, None)
    batch = {"audio": x.to(gpu), "label": y.to(gpu), "lengths": torch.tensor(lens, dtype=torch.int32, device=gpu)}
    res = ours.train_step(batch, opt, None, gpu, None)  # the public path: batch.get("lengths") -> the ragged step
    st = ours._fused
    assert isinstance(st, FusedMosiMonoStep) and st.ragged and st.eng.ragged
    torch.cuda.synchronize()
    forced = tmm._decisions(st.eng)
    t32, t64 = orc.MosiTrace(forced), orc.MosiTrace(forced)
    r32 = tmm._oracle_step(o32, x, y, None, t32)
    r64 = tmm._oracle_step(o64, x.double(), y, None, t64)
    _flips_len(t64, forced, {})
    tally = Tally()
    check_out("logits", st.logits, r32["logits"], r64["logits"], tally)
    check_out("loss", st.loss, r32["loss"].reshape(1), r64["loss"].reshape(1), tally)
    assert abs(res["loss"] - float(r64["loss"])) <= 1e-4 * abs(float(r64["loss"]))
    p32, p64 = dict(o32.named_parameters()), dict(o64.named_parameters())
    for n, p in ours.named_parameters():
        check_grad(f"grad {n}", p.grad, p32[n].grad, p64[n].grad, tally)
    check_adam(ours, opt, *before, 1, lr=tmm.LR, wd=tmm.WD)
    print(tally)


def test_fit_monomodal_reads_the_datasets_lengths(gpu, tmp_path):
    from tspm_amd.monomodal import FusedMosiMonoEvalStep, fit_monomodal
    ours = tmm._ours("lstm_maxpool", 5, gpu, 0)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=tmm.LR, weight_decay=tmm.WD)
    kw = dict(target_modality="audio", selected_patterns=["a"], device=gpu, use_lengths=True)
    tr_corpus = synthetic_mosi_corpus(24, seed=5, steps=12, min_len=3)
    tr = MOSI(corpus=tr_corpus, split="train", **kw)
    va = MOSI(corpus=synthetic_mosi_corpus(8, seed=6, steps=12, min_len=3), split="valid", **kw)
    b = next(iter(tr.device_loader(8, pad_to=12)))
    assert list(b) == ["audio", "label", "pattern_name", "lengths"]
    assert np.array_equal(b["lengths"].cpu().numpy(), tr_corpus.lengths["audio"][:8])
    loaders = {"train": tr.loader(8, shuffle=True, seed=0, pad_to=12), "validation": va.loader(8, pad_to=12)}
    h = fit_monomodal(ours, opt, None, loaders, 1, experiment_name="MOSI_Audio_Encoder_Pretrain",
                      model_output_path=tmp_path)
    assert np.isfinite(h["metrics_history"]["train"][0]["loss"]) and np.isfinite(h["metrics_history"]["validation"][0]["loss"])
    steps = list(ours._by_buffer.values())
    assert steps and all(st.ragged for st in steps)
    train = [st for st in steps if isinstance(st, FusedMosiMonoStep)]
    assert len(train) == 1 and train[0].graph is not None  # 3 batches of one padded shape: one step, one graph
    # the eval step's embedding is the standalone encoder's with the same lengths
    ours.eval()
    est = [st for st in steps if isinstance(st, FusedMosiMonoEvalStep)][0]
    x = est.X.transpose(0, 1).contiguous()
    assert torch.equal(ours.encoder(x, est.eng.lens), est.emb)
    assert not torch.equal(ours.encoder(x), est.emb)


def test_autograd_validation_and_embedding_paths_take_lengths(gpu):
    """The reference's own train_step sequence (autograd node, torch optimizer), validation_step and get_embeddings with
    ``batch["lengths"]``: the gradients are those of the ragged fused step, the embeddings those of forward(lengths=)."""
    from parity import rel_l2
    cfg, lengths = orc.MOSI, LENS[1]
    A, V, T, y = _batch(cfg, lengths)
    keeps = {k: v.to(gpu) for k, v in orc.keep_masks(B, 9, cfg=cfg).items()}
    dl = _dev_lengths(lengths, gpu)
    fused = _dropin(6, cfg=cfg).to(gpu)
    opt = tspm_amd.FusedAdam(fused.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
    st = fused.fused_step(opt, None, B, STEPS, ragged=True)
    st.keep_override = keeps
    st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu), dl)
    auto = _dropin(6, cfg=cfg).to(gpu).train()
    auto._engine(B, STEPS, gpu, True).keep_override = keeps
    logits = auto(A.to(gpu), V.to(gpu), T.to(gpu), lengths=dl)
    torch.nn.functional.cross_entropy(logits, y.to(gpu)).backward()
    torch.cuda.synchronize()
    assert rel_l2(logits, st.eng.logits) <= 1e-6
    for (n, p), (_, q) in zip(auto.named_parameters(), fused.named_parameters()):
        assert rel_l2(p.grad, q.grad) <= 1e-5, n
    # validation_step and get_embeddings read batch["lengths"]
    auto.eval()
    with torch.no_grad():
        ref = auto(A.to(gpu), V.to(gpu), T.to(gpu), lengths=dl).clone()
    emb_ref = auto._engine(B, STEPS, gpu, True).fused.clone()
    batch = {"audio": A, "video": V, "text": T, "label": y, "lengths": dl}
    out = auto.validation_step(batch, None, gpu, None)
    assert torch.equal(auto._engine(B, STEPS, gpu, True).logits, ref)
    assert abs(out["loss"] - float(torch.nn.functional.cross_entropy(ref, y.to(gpu)))) <= 1e-5
    emb = auto.get_embeddings([batch], gpu)
    assert np.array_equal(emb["audio"][0], emb_ref[:, :64].cpu().numpy())
    assert np.array_equal(emb["video"][0], emb_ref[:, 64:128].cpu().numpy())
    nolen = auto.get_embeddings([{k: v for k, v in batch.items() if k != "lengths"}], gpu)
    assert not np.array_equal(nolen["audio"][0], emb["audio"][0])


# ------------------------------------------------------------------------------------------------
# loader
# ------------------------------------------------------------------------------------------------
def test_loader_hands_the_lengths_to_the_ragged_steps(gpu):
    from tspm_amd import harness
    corpus = synthetic_mosi_corpus(n=24, steps=12, min_len=3)
    ds = MOSI(split="train", corpus=corpus, device=gpu, seed=4, use_lengths=True)
    ours = _dropin(8).to(gpu)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=1e-3, weight_decay=1e-3)
    made = []

    def step_for(b, t):
        made.append(ours.fused_step(opt, None, b, t, ragged=True))
        return made[-1]
    order = np.arange(24)
    for i, batch in enumerate(ds.device_loader(8, step_for=step_for, pad_to=12)):
        e = made[-1].eng
        idx = order[i * 8:(i + 1) * 8]
        assert batch["lengths"]["audio"] is e.lens["a"] and batch["lengths"]["video"] is e.lens["v"]
        assert np.array_equal(e.lens["a"].cpu().numpy(), corpus.lengths["audio"][idx])
        assert np.array_equal(e.lens["v"].cpu().numpy(), corpus.lengths["video"][idx])
    assert len(made) == 3 and all(m is made[0] for m in made)
    # without a step the batch dict carries them
    batch = next(iter(ds.device_loader(8, pad_to=12)))
    assert np.array_equal(batch["lengths"]["audio"].cpu().numpy(), corpus.lengths["audio"][:8])
    assert batch["lengths"]["video"].dtype == torch.int32 and "text" not in batch["lengths"]
    # fit: one epoch of 3 batches on one ragged step, finite loss
    loaders = {"train": ds.loader(8, shuffle=True, seed=1, pad_to=12),
               "validation": MOSI(split="valid", corpus=synthetic_mosi_corpus(n=6, steps=12, min_len=3, seed=2),
                                  device=gpu, use_lengths=True).loader(6, pad_to=12)}
    hist = harness.fit(ours, opt, None, loaders, epochs=1, early_stopping=False)
    assert np.isfinite(hist["train"][-1]["loss"]) and np.isfinite(hist["validation"][-1]["loss"])
    assert made[0].calls == 3 and all(k[-1] == "ragged" for k in ours._steps)


def test_split_lengths_trim_the_corpus(gpu, tmp_path):
    """A split with audio_lengths / vision_lengths: use_lengths trims the corpus to them (off: dense, as before)."""
    g = np.random.default_rng(0)
    n, T = 5, 7
    split = {"audio": g.standard_normal((n, T, 5)).astype(np.float32),
             "vision": g.standard_normal((n, T, 20)).astype(np.float32),
             "text": g.standard_normal((n, T, 768)).astype(np.float32),
             "classification_labels": g.integers(0, 3, n).astype(np.int64),
             "audio_lengths": np.array([7, 1, 3, 5, 2]), "vision_lengths": np.array([2, 7, 4, 1, 6])}
    path = tmp_path / "unaligned.npz"
    np.savez(path, **{f"train/{k}": v for k, v in split.items()})
    on = MOSI(path, split="train", device=gpu, use_lengths=True)
    off = MOSI(path, split="train", device=gpu)
    assert np.array_equal(on.corpus.lengths["audio"], split["audio_lengths"])
    assert np.array_equal(on.corpus.lengths["video"], split["vision_lengths"])
    assert np.array_equal(on.corpus.lengths["text"], np.full(n, T))
    assert np.array_equal(off.corpus.lengths["audio"], np.full(n, T)) and hasattr(off.corpus, "true_lengths")
    batch = next(iter(on.device_loader(n)))
    assert tuple(batch["audio"].shape) == (n, 7, 5)
    assert torch.equal(batch["audio"][1, 1:], torch.zeros(6, 5, device=gpu))  # trimmed, then zero-padded
    assert np.array_equal(batch["lengths"]["video"].cpu().numpy(), split["vision_lengths"])
