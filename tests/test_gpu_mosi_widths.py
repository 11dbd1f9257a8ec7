"""UTT-Fusion with LSTM encoders of other widths than 64 — each of netA / netV / netT its own — on the HIP path against
the CPU oracle built from oracle/mosi_ref.py's classes with the same widths in the same seed order.

Criterion as tests/test_gpu_mosi.py (tests/parity.py), its step-level helpers imported: the oracle in fp64 with our
decisions forced into it is the truth; every forced decision that differs from fp64's own must be a near-tie and rare;
logits / loss rel-L2 <= 1e-4, every gradient rel-L2 <= 1e-3 and cosine >= 0.9999 and within 4x the fp32 reference's
error on the same decisions; the clip coefficient against our total norm and Adam exactly; every step from our own
state.  (With seed 3, batch seed 1234 + B and keep seeds 50 + s the fp32 oracle itself flips no decision against fp64
in the three steps of either fusion case, so the flip caps hold for the reference alone.)
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import tspm_amd
from oracle import mosi_ref as orc
from parity import Tally, check_adam, check_grad, check_out, pair_from, rel_l2, snapshot
from test_gpu_mono import _clear
from test_gpu_mosi import _check_adam, _check_step, _flips
from test_gpu_mosi_mono import _decisions as _mono_decisions
from test_gpu_mosi_regress import Group, _scores
from test_gpu_mosi_regress import _check_step as _check_regress_step
from tspm_amd import _lib as L
from tspm_amd import mosi as M
from tspm_amd.monomodal import FusedMosiMonoStep, MonomodalEncoder, fit_monomodal
from tspm_amd.mosi_data import MOSI, synthetic_mosi_corpus

pytestmark = pytest.mark.gpu

# MOSI-style: "last", classifier 208 -> 64/32 -> 3, dropout 0.5, clip 1.0
MOSI_W = (orc.UttConfig(cls_layers=(64, 32)), (32, 128, 48))
# MOSEI-style: 74 / 35-d inputs, "maxpool", use_bn, 96/48, dropouts 0.7 / 0.66, clip 0.5
MOSEI_W = (orc.MOSEI, (100, 36, 64))


def _dropin(seed, cfg, widths, clip=None, output_dim=3):
    ha, hv, ht = widths
    torch.manual_seed(seed)
    a = M.LSTMEncoder(input_size=cfg.audio_dim, hidden_size=ha, embd_method=cfg.embd_method)
    v = M.LSTMEncoder(input_size=cfg.video_dim, hidden_size=hv, embd_method=cfg.embd_method)
    t = M.TextCNN(input_size=768, embd_size=ht, dropout=cfg.text_dropout, in_channels=1, out_channels=128,
                  kernel_heights=[3, 4, 5])
    c = M.FcClassifier(input_dim=ha + hv + ht, layers=list(cfg.cls_layers), output_dim=output_dim,
                       dropout=cfg.cls_dropout, use_bn=cfg.use_bn)
    return M.UttFusionModel(a, v, t, c, clip=cfg.clip if clip is None else clip)


def _oracle(seed, cfg, widths, output_dim=3):
    ha, hv, ht = widths
    torch.manual_seed(seed)
    a = orc.OracleLSTMEncoder(cfg.audio_dim, ha, cfg.embd_method)
    v = orc.OracleLSTMEncoder(cfg.video_dim, hv, cfg.embd_method)
    t = orc.OracleTextCNN(cfg.text_dim, embd_size=ht, dropout=cfg.text_dropout, in_channels=1,
                          out_channels=orc.FILTERS, kernel_heights=list(orc.HEIGHTS))
    c = orc.OracleFcClassifier(ha + hv + ht, list(cfg.cls_layers), output_dim, dropout=cfg.cls_dropout,
                               use_bn=cfg.use_bn)
    return orc.OracleUttFusion(a, v, t, c, clip=cfg.clip)


def test_dropin_and_oracle_share_the_seeded_initialisation():
    for cfg, widths in (MOSI_W, MOSEI_W):
        a, b = _dropin(3, cfg, widths).state_dict(), _oracle(3, cfg, widths).state_dict()
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("case,batch,steps", [(MOSI_W, 5, 9), (MOSEI_W, 6, 12)], ids=["mosi_32_128_48", "mosei_100_36_64"])
def test_fused_step_mixed_widths_vs_oracle(gpu, case, batch, steps):
    """Three steps (eager, captured, replayed): logits, loss, every gradient, the total norm, the clip coefficient,
    Adam and (MOSEI-style) the BatchNorm1d running statistics."""
    cfg, widths = case
    seed = 3
    ours = _dropin(seed, cfg, widths).to(gpu)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
    A, V, T, y = orc.synthetic_batch(batch, steps, seed=1234 + batch, cfg=cfg)
    st = M.FusedMosiStep(ours, opt, None, batch, steps)
    assert st.eng.E == sum(widths) and tuple(st.eng.fused.shape) == (batch, sum(widths))
    tally, coefs = Tally(), []
    for s in range(3):
        keeps = orc.keep_masks(batch, 50 + s, cfg=cfg)
        o32, o64 = pair_from(ours, lambda: _oracle(seed, cfg, widths))
        before = snapshot(ours, opt if s else None)
        st.keep_override = {k: v.to(gpu) for k, v in keeps.items()}
        out = st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        rep = _check_step(ours, st, o32, o64, A, V, T, y, keeps, out, tally)
        coef = float(st.eng.clip_coef.item())
        exp = min(1.0, cfg.clip / (st.eng.total_norm.item() + 1e-6))
        assert abs(coef - exp) <= 1e-6 * exp
        coefs.append(coef)
        _check_adam(ours, opt, before, s + 1, coef, cfg)
        print(f"[widths {widths} B={batch} T={steps} step {s + 1}] flips {rep} norm {st.eng.total_norm.item():.3f} "
              f"clip coef {coef:.4f}")
    assert st.graph is not None
    if cfg.use_bn:
        assert max(coefs) < 1.0, "the clip is active at these gradient norms"
    print(tally)


def test_graph_replay_equals_eager_mixed_widths(gpu):
    cfg, widths = MOSI_W
    res = []
    for use_graph in (False, True):
        ours = _dropin(7, cfg, widths).to(gpu)
        opt = tspm_amd.FusedAdam(ours.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
        st = M.FusedMosiStep(ours, opt, None, 6, 10, use_graph=use_graph)
        A, V, T, y = orc.synthetic_batch(6, 10, seed=5, cfg=cfg)
        for s in range(3):  # eager, capture, replay
            st.keep_override = {k: v.to(gpu) for k, v in orc.keep_masks(6, 90 + s, cfg=cfg).items()}
            st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        assert (st.graph is not None) == use_graph
        res.append(torch.cat([p.detach().reshape(-1) for p in ours.parameters()] + [st.eng.loss.reshape(-1)]).cpu())
    assert torch.equal(res[0], res[1])


def test_lstm_bias_gradients_identical_at_widths_36_100(gpu):
    """b_ih.grad and b_hh.grad are the same column sums of the gate gradients, bitwise, for both encoders at widths
    (36, 100) — with a 36-d audio input, so netA's two weight-gradient products have the same fan-in."""
    cfg = orc.UttConfig(audio_dim=36, cls_layers=(64, 32))  # the audio fan-in EQUALS netA's hidden size
    ours = _dropin(1, cfg, (36, 100, 64)).to(gpu)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
    st = M.FusedMosiStep(ours, opt, None, 32, 20)
    A, V, T, y = orc.synthetic_batch(32, 20, seed=9, cfg=cfg)
    st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
    torch.cuda.synchronize()
    for enc in (ours.netA, ours.netV):
        assert bool(enc.rnn.bias_ih_l0.grad.abs().sum() > 0)
        assert torch.equal(enc.rnn.bias_ih_l0.grad, enc.rnn.bias_hh_l0.grad)


@pytest.mark.parametrize("case", [MOSI_W, MOSEI_W], ids=["mosi_32_128_48", "mosei_100_36_64"])
def test_validation_step_and_embeddings_mixed_widths(gpu, case):
    cfg, widths = case
    ha, hv, ht = widths
    ours = _dropin(6, cfg, widths).to(gpu)
    o = _oracle(6, cfg, widths)
    A, V, T, y = orc.synthetic_batch(7, 9, seed=31, cfg=cfg)
    batch = {"audio": A, "video": V, "text": T, "label": y, "pattern_name": ["atv"] * 7}
    v = ours.validation_step(batch, None, gpu, None)
    r = orc.validation_step(o.double(), A.double(), V.double(), T.double(), y)
    check_out("eval logits", ours._engine(7, 9, gpu).logits, None, r["logits"])
    assert abs(v["loss"] - r["loss"].item()) <= 1e-4 * abs(r["loss"].item())
    emb = ours.get_embeddings([batch], gpu)
    assert emb["audio"][0].shape == (7, ha) and emb["video"][0].shape == (7, hv) and emb["text"][0].shape == (7, ht)
    fused = ours._engine(7, 9, gpu).fused.cpu()
    assert torch.equal(torch.from_numpy(emb["audio"][0]), fused[:, :ha])
    assert torch.equal(torch.from_numpy(emb["video"][0]), fused[:, ha:ha + hv])
    assert torch.equal(torch.from_numpy(emb["text"][0]), fused[:, ha + hv:ha + hv + ht])
    ours.eval()
    with torch.no_grad():  # each slice is the standalone encoder's forward
        assert torch.equal(ours.netA(A.to(gpu)).cpu(), fused[:, :ha])
        assert torch.equal(ours.netV(V.to(gpu)).cpu(), fused[:, ha:ha + hv])
        assert torch.equal(ours.netT(T.to(gpu)).cpu(), fused[:, ha + hv:])
    with torch.no_grad():
        ea = orc.lstm_forward(o.netA.double(), A.double())
        ev = orc.lstm_forward(o.netV.double(), V.double())
    check_out("audio embedding", fused[:, :ha], None, ea)
    check_out("video embedding", fused[:, ha:ha + hv], None, ev)


class OracleMono(nn.Module):
    """train_monomodal.MonomodalEncoder's two attributes around an oracle LSTM encoder of width `hid`."""

    def __init__(self, encoder, hid):
        super().__init__()
        self.encoder = encoder
        self.classifier = nn.Linear(hid, 3)


def _oracle_mono_step(o, x, y, trace):
    o.train()
    for p in o.parameters():
        p.grad = None
    logits = o.classifier(orc.lstm_forward(o.encoder, x, trace, "lstm.a.pool"))
    loss = 0.0 + 1.0 * F.cross_entropy(logits, y)
    loss.backward()
    return {"logits": logits.detach(), "loss": loss.detach(), "preds": logits.detach().argmax(1)}


MONO = [(35, 128, "maxpool", 0.5), (5, 32, "last", 1.0)]


def _mono(feat, hid, mode, dev, seed, fused_head=True):
    torch.manual_seed(seed)
    return MonomodalEncoder(M.LSTMEncoder(feat, hid, mode), hid, 3, fused_head=fused_head).to(dev)


def _mono_batch(feat, scale, seed, b=33, t=12):
    g = torch.Generator().manual_seed(seed)
    return scale * torch.randn(b, t, feat, generator=g), torch.randint(0, 3, (b,), generator=g)


@pytest.mark.parametrize("feat,hid,mode,scale", MONO)
def test_encoder_pretraining_step_vs_oracle(gpu, feat, hid, mode, scale):
    batch, steps = 33, 12
    ours = _mono(feat, hid, mode, gpu, 3)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=1e-3, weight_decay=1e-3)
    x, y = _mono_batch(feat, scale, 1234 + batch)
    st = FusedMosiMonoStep(ours, opt, None, (batch, steps, feat))
    assert st.fused_head
    o32, o64 = pair_from(ours, lambda: OracleMono(orc.OracleLSTMEncoder(feat, hid, mode), hid))
    before = snapshot(ours, None)
    out = st.step(x.to(gpu), y.to(gpu))
    torch.cuda.synchronize()
    forced = _mono_decisions(st.eng)
    t32, t64 = orc.MosiTrace(forced), orc.MosiTrace(forced)
    r32, r64 = _oracle_mono_step(o32, x, y, t32), _oracle_mono_step(o64, x.double(), y, t64)
    rep = _flips(t64, forced, {})
    tally = Tally()
    check_out("logits", out["logits"], r32["logits"], r64["logits"], tally)
    check_out("loss", out["loss"], r32["loss"].reshape(1), r64["loss"].reshape(1), tally)
    p32, p64 = dict(o32.named_parameters()), dict(o64.named_parameters())
    for n, p in ours.named_parameters():
        check_grad(f"grad {n}", p.grad, p32[n].grad, p64[n].grad, tally)
    assert torch.equal(ours.encoder.rnn.bias_ih_l0.grad, ours.encoder.rnn.bias_hh_l0.grad)
    check_adam(ours, opt, *before, 1, lr=1e-3, wd=1e-3)
    clear = _clear(r64["logits"])
    assert torch.equal(out["preds"].cpu()[clear], r64["preds"][clear])
    print(f"[mono {feat}->{hid} {mode}] flips {rep}; {tally}")


@pytest.mark.parametrize("feat,hid,mode,scale", MONO)
def test_encoder_pretraining_fused_head_and_separate_launches_agree(gpu, feat, hid, mode, scale):
    got = {}
    for fh in (True, False):
        ours = _mono(feat, hid, mode, gpu, 11, fh)
        opt = tspm_amd.FusedAdam(ours.parameters(), lr=1e-3, weight_decay=1e-3)
        x, y = _mono_batch(feat, scale, 77)
        st = FusedMosiMonoStep(ours, opt, None, (33, 12, feat))
        assert st.fused_head is fh
        out = st.step(x.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        got[fh] = (out["loss"].item(), torch.cat([p.detach().reshape(-1) for p in ours.parameters()]).cpu(),
                   out["logits"].cpu().clone(), out["preds"].cpu().clone())
    assert abs(got[True][0] - got[False][0]) <= 1e-6 * abs(got[False][0])
    assert rel_l2(got[True][1], got[False][1]) < 1e-4
    clear = _clear(got[False][2].double())
    assert torch.equal(got[True][3][clear], got[False][3][clear])


def test_regression_step_mixed_widths_vs_oracle(gpu):
    """output_dim = 1, widths (32, 128, 48): one L1 step with the one-launch regression head."""
    cfg, widths = MOSI_W
    batch, steps, seed = 5, 9, 3
    ours = _dropin(seed, cfg, widths, output_dim=1).to(gpu)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
    A, V, T, _ = orc.synthetic_batch(batch, steps, seed=1234 + batch, cfg=cfg)
    y = _scores(batch, 77 + batch)
    st = M.FusedMosiStep(ours, opt, Group("l1", 1.0), batch, steps)
    assert st.regress == (L.REGRESS_L1, 1.0)
    keeps = orc.keep_masks(batch, 50, cfg=cfg)
    o32, o64 = pair_from(ours, lambda: _oracle(seed, cfg, widths, output_dim=1))
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
    print(f"[regression widths {widths}] flips {rep}; {tally}")


def test_fit_monomodal_hands_a_128_wide_encoder_to_utt_fusion(gpu, tmp_path):
    ours = _mono(5, 128, "last", gpu, 0)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=1e-3, weight_decay=1e-3)
    tr = MOSI(corpus=synthetic_mosi_corpus(32, seed=5, steps=6), split="train", target_modality="audio",
              selected_patterns=["a"], device=gpu)
    va = MOSI(corpus=synthetic_mosi_corpus(16, seed=6, steps=6), split="valid", target_modality="audio",
              selected_patterns=["a"], device=gpu)
    loaders = {"train": tr.loader(16, shuffle=True, seed=0), "validation": va.loader(16), "test": va.loader(16)}
    h = fit_monomodal(ours, opt, None, loaders, 1, experiment_name="MOSI_Audio_Encoder_Pretrain",
                      model_output_path=tmp_path)
    assert h["encoder_path"] and (tmp_path / "encoder_audio_best.pth").exists()
    enc_sd = torch.load(tmp_path / "encoder_audio_best.pth", weights_only=True)
    assert tuple(enc_sd["rnn.weight_hh_l0"].shape) == (512, 128)
    fusion = M.build_utt_fusion("mosi", embd_sizes=(128, 64, 64))
    fusion.netA.load_state_dict(enc_sd)
    assert list(enc_sd) == list(fusion.netA.state_dict())
    fusion = fusion.to(gpu).eval()
    A, V, T, _ = orc.synthetic_batch(4, 6, seed=9)
    eng = fusion._engine(4, 6, gpu)
    eng.load(A.to(gpu), V.to(gpu), T.to(gpu))
    eng.forward(L.stream_handle(), False)
    torch.cuda.synchronize()
    mono = MonomodalEncoder(M.LSTMEncoder(5, 128), 128, 3)
    mono.encoder.load_state_dict(enc_sd)
    mono = mono.to(gpu).eval()
    with torch.no_grad():
        assert torch.equal(mono.encoder(A.to(gpu)), eng.fused[:, :128])
    with pytest.raises(RuntimeError, match="size mismatch"):
        M.build_utt_fusion("mosi").netA.load_state_dict(enc_sd)


def test_unsupported_width_raises_on_the_first_forward(gpu):
    torch.manual_seed(0)
    m = M.UttFusionModel(M.LSTMEncoder(5, 130), M.LSTMEncoder(20, 64), M.TextCNN(768, 64),
                         M.FcClassifier(130 + 128, [32], 3), clip=1.0).to(gpu).eval()
    A, V, T, _ = orc.synthetic_batch(2, 4, seed=1)
    with pytest.raises(L.TspmError, match="multiple of 4.*128"):
        m(A.to(gpu), V.to(gpu), T.to(gpu))
    with pytest.raises(L.TspmError, match="multiple of 4.*128"):
        M.LSTMEncoder(5, 130).to(gpu)(A.to(gpu))
