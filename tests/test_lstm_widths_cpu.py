"""LSTM encoders of any width up to 128 — the checks that need no GPU: tspm_lstm_fwd_w / tspm_lstm_bwd_w validate every
descriptor before any launch (an accepted call answers TSPM_ERR_LAUNCH = 2 on a machine without a GPU, as in
test_abi.py), ``_lib.lstm_width_supported`` mirrors the kernel limit, and the drop-in constructors take the widths."""
import pytest
import torch
import yaml

import tspm_amd
from tspm_amd import _lib as L
from tspm_amd import mosi as M

INVALID, LAUNCH = 1, 2
P = 4096  # a 16-byte aligned, non-NULL stand-in: never dereferenced, every call returns before or at the launch
BAD_WIDTHS = (0, 2, 6, 130, 132, 256)
GOOD_WIDTHS = (4, 32, 36, 64, 100, 128)


def _fwd(count=1, second=None, **kw):
    f = dict(batch=2, steps=3, hidden=64, ld_out=None, xg=P, w_hh=P, b_hh=P, gates=P, cs=P, hs=P, h_out=P, argmax=None)
    f.update(kw)
    if f["ld_out"] is None:
        f["ld_out"] = f["hidden"]
    g = dict(f)
    g.update(second or {})
    if second and "ld_out" not in second:
        g["ld_out"] = g["hidden"]
    d = (L.LstmFwdDesc * 2)(L.LstmFwdDesc(**f), L.LstmFwdDesc(**g))
    return L.load().tspm_lstm_fwd_w(count, d, None)


def _bwd(count=1, second=None, **kw):
    f = dict(batch=2, steps=3, hidden=64, ld_dh=None, w_hh=P, gates=P, cs=P, dh=P, dgates=P, argmax=None)
    f.update(kw)
    if f["ld_dh"] is None:
        f["ld_dh"] = f["hidden"]
    g = dict(f)
    g.update(second or {})
    if second and "ld_dh" not in second:
        g["ld_dh"] = g["hidden"]
    d = (L.LstmBwdDesc * 2)(L.LstmBwdDesc(**f), L.LstmBwdDesc(**g))
    return L.load().tspm_lstm_bwd_w(count, d, None)


def _no_gpu():
    return not torch.cuda.is_available()


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["fwd", "bwd"])
def test_width_entry_points_refuse_before_launch(call):
    assert call(count=0) == INVALID and call(count=3) == INVALID
    for h in BAD_WIDTHS:
        assert call(hidden=h, **{"ld_out" if call is _fwd else "ld_dh": 256}) == INVALID, h
    assert call(batch=0) == INVALID and call(steps=0) == INVALID
    assert call(steps=257, argmax=P) == INVALID  # uint8 time index
    for h in GOOD_WIDTHS:
        assert call(hidden=h, **{"ld_out" if call is _fwd else "ld_dh": h - 1}) == INVALID, h
    # the second descriptor is validated before the first one launches
    assert call(count=2, hidden=36, second=dict(hidden=130)) == INVALID
    assert call(count=2, hidden=128, second=dict(batch=0)) == INVALID


def test_width_entry_points_refuse_null_buffers():
    for n in ("xg", "w_hh", "gates", "cs", "hs", "h_out"):
        assert _fwd(hidden=36, **{n: None}) == INVALID, n
    for n in ("w_hh", "gates", "cs", "dh", "dgates"):
        assert _bwd(hidden=36, **{n: None}) == INVALID, n
    assert _fwd(hidden=36, w_hh=P + 4) == INVALID  # the float4 loads of W_hh need 16-byte alignment
    lib = L.load()
    assert lib.tspm_lstm_fwd_w(1, None, None) == INVALID and lib.tspm_lstm_bwd_w(1, None, None) == INVALID


@pytest.mark.skipif(not _no_gpu(), reason="an accepted call would launch on the stand-in pointers")
@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["fwd", "bwd"])
def test_width_entry_points_accept_supported_widths(call):
    for h in GOOD_WIDTHS:
        assert call(hidden=h) == LAUNCH, h
        if call is _fwd:
            assert call(hidden=h, b_hh=None) == LAUNCH, h
        assert call(hidden=h, steps=256, argmax=P) == LAUNCH, h
        assert call(hidden=h, steps=300) == LAUNCH, h
    # any mixture of widths, each descriptor with its own batch and steps
    assert call(count=2, hidden=36, second=dict(hidden=128, batch=5, steps=7)) == LAUNCH
    assert call(count=2, hidden=128, second=dict(hidden=4)) == LAUNCH
    assert call(count=2, hidden=64, second=dict(hidden=64)) == LAUNCH


def test_lstm_width_supported_mirrors_the_kernel_limit():
    for h in BAD_WIDTHS + (-4, 1, 3, 5, 127, 129):
        assert not L.lstm_width_supported(h), h
    for h in range(4, 129, 4):
        assert L.lstm_width_supported(h), h
    assert {h for h in range(0, 300) if L.lstm_width_supported(h)} == set(range(4, 129, 4))
    for h in range(0, 140):  # the library agrees at every width (a supported one is only tried where nothing can launch)
        if not L.lstm_width_supported(h):
            assert _fwd(hidden=h, ld_out=256) == INVALID and _bwd(hidden=h, ld_dh=256) == INVALID, h
        elif _no_gpu():
            assert _fwd(hidden=h) == LAUNCH and _bwd(hidden=h) == LAUNCH, h


def test_encoders_construct_at_other_widths():
    enc = M.LSTMEncoder(5, 128)
    assert enc.hidden_size == 128 and tuple(enc.rnn.weight_hh_l0.shape) == (512, 128)
    loader = type("Loader", (yaml.SafeLoader,), {})
    tspm_amd.plugin.register_yaml(loader)
    e = yaml.load("enc: !LSTMEncoder {input_size: 5, hidden_size: 32, embd_method: maxpool}", Loader=loader)["enc"]
    assert isinstance(e, M.LSTMEncoder) and e.hidden_size == 32 and e.embd_method == "maxpool"
    assert tuple(e.rnn.weight_ih_l0.shape) == (128, 5)
    M.LSTMEncoder(5, 130)  # constructs like the reference's; the HIP path refuses it on the first forward


def test_lstm_alloc_names_the_limit():
    for h in (4, 36, 100, 128):
        bufs = M._lstm_alloc(M.LSTMEncoder(5, h, "maxpool"), 3, 2, "cpu")
        assert tuple(bufs["xg"].shape) == (6, 4 * h) and tuple(bufs["hs"].shape) == (9, h)
        assert tuple(bufs["arg"].shape) == (3, h)
    for h in (2, 130, 256):
        with pytest.raises(L.TspmError, match="multiple of 4.*128"):
            M._lstm_alloc(M.LSTMEncoder(5, h), 3, 2, "cpu")


def _manual(name, seed):
    c = M.YAML_CONFIGS[name]
    torch.manual_seed(seed)
    a = M.LSTMEncoder(input_size=c["audio_dim"], hidden_size=64, embd_method=c["embd_method"])
    v = M.LSTMEncoder(input_size=c["video_dim"], hidden_size=64, embd_method=c["embd_method"])
    t = M.TextCNN(input_size=768, embd_size=64, dropout=c["text_dropout"], in_channels=1, out_channels=128,
                  kernel_heights=[3, 4, 5])
    k = M.FcClassifier(input_dim=192, layers=list(c["cls_layers"]), output_dim=3, dropout=c["cls_dropout"],
                       use_bn=c["use_bn"])
    return M.UttFusionModel(a, v, t, k, clip=c["clip"])


@pytest.mark.parametrize("name", ["mosi", "mosei"])
def test_build_utt_fusion_default_is_todays_model(name):
    torch.manual_seed(3)
    sd = M.build_utt_fusion(name).state_dict()
    ref = _manual(name, 3).state_dict()
    assert list(sd) == list(ref) and all(torch.equal(sd[k], ref[k]) for k in sd)
    torch.manual_seed(3)
    sd2 = M.build_utt_fusion(name, embd_sizes=(64, 64, 64)).state_dict()
    assert all(torch.equal(sd[k], sd2[k]) for k in sd)


def test_build_utt_fusion_mixed_widths():
    m = M.build_utt_fusion("mosi", embd_sizes=(32, 128, 48))
    assert (m.netA.hidden_size, m.netV.hidden_size, m.netT.hidden_size) == (32, 128, 48)
    assert m.netC.linears()[0].in_features == 208
    assert tuple(m.netA.rnn.weight_hh_l0.shape) == (128, 32) and tuple(m.netV.rnn.weight_hh_l0.shape) == (512, 128)
    assert m.netT.embd[0].out_features == 48
    r = M.build_utt_fusion("mosei", output_dim=1, embd_sizes=(100, 36, 64))
    assert r.netC.linears()[0].in_features == 200 and r.netC.fc_out.out_features == 1
