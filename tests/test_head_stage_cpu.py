"""The AVMNIST head stage (the fusion head trained on frozen encoders, every pattern in one step), the parts that need no
device: the entry point ``tspm_pattern_head_train_step`` (export, header and ctypes agree; every refusal returns before
any launch, so it runs without a device, and ``_lib.pattern_head_train_supported`` predicts the shape refusals),
``AVMNIST.freeze_encoders`` / ``train()`` pinning and every refusal of ``step.head_stage_frozen``, the loader's
``all_patterns`` mode, the unchanged keys of an unfrozen model, and the fp64 folding identity behind fc0's weight
gradient (tests/head_stage_ref.py, the reference the GPU tests use)."""
import ctypes
import os
import re
import subprocess
import types

import pytest
import torch

import head_stage_ref as R
import tspm_amd
from tspm_amd import _lib as L
from tspm_amd import step as S
from tspm_amd.data import AVMNIST, DeviceLoader, synthetic_corpus

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "tspm.h")
OK, INVALID, WORKSPACE = 0, 1, 3
FAKE = 0x10000  # a 16-byte aligned non-NULL value: a refused call never dereferences (or launches with) it
NAMES = ("tspm_pattern_head_train_step", "tspm_pattern_head_train_workspace")


# ------------------------------------------------------------------------------------------------
# the entry point
# ------------------------------------------------------------------------------------------------
def test_header_export_and_binding_agree():
    src = re.sub(r"\s+", " ", open(HEADER).read())
    assert "int tspm_pattern_head_train_step(const tspm_pattern_head_train_desc* desc, tspm_stream_t stream);" in src
    assert "size_t tspm_pattern_head_train_workspace(int32_t batch, int32_t npat);" in src
    assert "#define TSPM_ABI_VERSION 23 " in src and L.ABI_VERSION == 23 and L.lib().tspm_abi_version() == 23
    so = ctypes.CDLL(L.LIB_PATH)
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert name in L._SIGS and name in L.EXPORTED and hasattr(so, name)
        assert re.search(rf" T {name}$", nm, re.M), name
    assert L._SIGS[NAMES[0]] == (ctypes.c_int32, [ctypes.POINTER(L.PatternHeadTrainDesc), ctypes.c_void_p])
    assert L._SIGS[NAMES[1]] == (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int32])


def test_descriptor_layout_matches_the_header():
    src = re.sub(r"\s+", " ", open(HEADER).read())
    body = re.search(r"typedef struct tspm_pattern_head_train_desc \{(.*?)\} tspm_pattern_head_train_desc;", src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body)
    names, kinds = [], []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        base = decl.split()[0] if not decl.startswith("const") else decl.split()[1]
        for star, n in re.findall(r"(\*?)\s*(\w+)\s*(?:,|$)", decl[decl.index(base) + len(base):]):
            names.append(n)
            kinds.append("ptr" if (star or base.endswith("*")) else base)
    fields = L.PatternHeadTrainDesc._fields_
    assert [n.rstrip("_") for n in names] == [n.rstrip("_") for n, _ in fields]  # (in -> in_ in Python, reserved_)
    size = {"int32_t": 4, "float": 4, "uint64_t": 8, "size_t": 8, "ptr": 8}
    for (n, ct), kind in zip(fields, kinds):
        assert ctypes.sizeof(ct) == size[kind], (n, kind)
        is_ptr = ct is ctypes.c_void_p or hasattr(ct, "contents")
        assert is_ptr == (kind == "ptr"), (n, kind)
    # 10 int32, 3 + 7 pointers, 2 floats, uint64, 13 pointers, size_t: no padding anywhere
    assert ctypes.sizeof(L.PatternHeadTrainDesc) == 10 * 4 + 10 * 8 + 8 + 8 + 13 * 8 + 8
    off = 0
    for n, ct in fields:
        assert getattr(L.PatternHeadTrainDesc, n).offset == off, n
        off += ctypes.sizeof(ct)


def test_workspace_sizes():
    ws = L.lib().tspm_pattern_head_train_workspace
    assert ws(0, 3) == 0 == ws(7, 9) == ws(7, 0) == ws(-1, 3)
    # holds at least the per-row h1 / hh / dlogits / dz3 / row terms of the AVMNIST head and the folds
    B, P, F, H, H2, C = 128, 3, 192, 128, 64, 10
    assert ws(B, P) >= 4 * (P * B * (H + 2 * H2 + C + 2) + 2 * B * (2 * H + F)) and ws(B, P) % 16 == 0
    assert ws(300, 3) > ws(256, 3) > ws(7, 3) > 0


GOOD = dict(batch=7, npat=3, in_=192, w_audio=64, hidden=128, hidden2=64, classes=10, ldx=192, gen_keep=0, x=FAKE,
            x0=FAKE, keep=[1, 0, 1, 1, 0, 1], w0=FAKE, b0=FAKE, w3=FAKE, b3=FAKE, w5=FAKE, b5=FAKE, labels=FAKE, p=0.5,
            loss_weight=1.0, seed=1, counter=FAKE, keep_mask=FAKE, logits=FAKE, gw0=FAKE, gb0=FAKE, gw3=FAKE, gb3=FAKE,
            gw5=FAKE, gb5=FAKE, loss=FAKE, stats=FAKE, adam_step=FAKE, workspace=FAKE, workspace_bytes=1 << 24)


def _call(**kw):
    a = dict(GOOD)
    a.update(kw)
    a["keep"] = None if a["keep"] is None else (ctypes.c_int32 * len(a["keep"]))(*a["keep"])
    return L.lib().tspm_pattern_head_train_step(L.PatternHeadTrainDesc(**a), None)


SHAPE_REFUSALS = [dict(in_=260, ldx=260), dict(hidden=260), dict(hidden2=132), dict(classes=17), dict(in_=190),
                  dict(w_audio=62), dict(hidden=126), dict(hidden2=62), dict(w_audio=0), dict(w_audio=192),
                  dict(npat=0), dict(npat=9, keep=[1] * 18), dict(classes=0), dict(hidden=0),
                  dict(in_=256, ldx=256, hidden=256)]  # 256 x 260 floats of w0 alone: past 160 KiB of LDS
OTHER_REFUSALS = [dict(batch=0), dict(batch=-2), dict(ldx=188), dict(ldx=194), dict(x=FAKE + 4), dict(x0=FAKE + 8),
                  dict(w0=FAKE + 4), dict(w3=FAKE + 4), dict(w5=FAKE + 4), dict(x0=None), dict(p=-0.1), dict(p=1.0),
                  dict(p=1.5), dict(p=float("nan")), dict(keep_mask=None)] + \
                 [{k: None} for k in ("x", "keep", "w0", "b0", "w3", "b3", "w5", "b5", "labels", "logits", "gw0", "gb0",
                                      "gw3", "gb3", "gw5", "gb5", "loss")]
_ids = lambda rs: [",".join(f"{k}={v}" for k, v in r.items())[:40] for r in rs]  # noqa: E731


def test_null_descriptor():
    assert L.lib().tspm_pattern_head_train_step(None, None) == INVALID


@pytest.mark.parametrize("bad", SHAPE_REFUSALS, ids=_ids(SHAPE_REFUSALS))
def test_shape_refusals_and_supported_agree(bad):
    """TSPM_ERR_INVALID with pointers no launch could survive and no device in the process: nothing was launched;
    ``pattern_head_train_supported`` says the same of the shape."""
    a = dict(GOOD)
    a.update(bad)
    assert _call(**bad) == INVALID
    assert not L.pattern_head_train_supported(a["in_"], a["w_audio"], a["hidden"], a["hidden2"], a["classes"], a["npat"])


@pytest.mark.parametrize("bad", OTHER_REFUSALS, ids=_ids(OTHER_REFUSALS))
def test_pointer_and_argument_refusals(bad):
    assert _call(**bad) == INVALID
    assert L.pattern_head_train_supported(192, 64, 128, 64, 10, 3)  # the shape itself is fine


def test_workspace_refusals_and_nullable_arguments():
    need = L.lib().tspm_pattern_head_train_workspace(7, 3)
    assert _call(workspace=None) == WORKSPACE and _call(workspace_bytes=need - 1) == WORKSPACE
    assert _call(workspace=FAKE + 8) == WORKSPACE
    assert _call(workspace=None, hidden=126) == INVALID                       # a bad shape wins over a bad workspace
    # x0 may be NULL only when every pattern keeps both modalities (checked before the workspace)
    assert _call(x0=None, npat=1, keep=[1, 1], workspace=None) == WORKSPACE
    assert _call(x0=None, npat=1, keep=[1, 0], workspace=None) == INVALID
    # stats, adam_step, counter are nullable; without dropout so is keep_mask
    assert _call(stats=None, adam_step=None, counter=None, workspace=None) == WORKSPACE
    assert _call(p=0.0, keep_mask=None, workspace=None) == WORKSPACE


def _lds_floats(F, H, H2, C, P):
    """The launch-1 kernel's LDS in floats: the three weight matrices (rows padded by 4), the sample's row and x0, the
    four half products, P rows of h1 / hh / logits (logits rows padded to a multiple of 4, plus 4), the biases."""
    ldc = ((C + 3) // 4) * 4 + 4
    return H * (F + 4) + H2 * (H + 4) + C * (H2 + 4) + 2 * (F + 4) + 4 * H + P * ((H + 4) + (H2 + 4) + ldc) + H + H2 + C


@pytest.mark.parametrize("shape", [(12, 4, 8, 4, 3, 3), (192, 64, 128, 64, 10, 3), (192, 64, 128, 64, 10, 1),
                                   (192, 64, 128, 64, 10, 8), (256, 128, 64, 32, 16, 8), (64, 32, 256, 64, 16, 8),
                                   (256, 128, 144, 128, 16, 8), (256, 128, 148, 128, 16, 8), (252, 128, 152, 128, 16, 1),
                                   (256, 4, 256, 4, 1, 1)])
def test_supported_follows_the_lds_formula(shape):
    F, wa, H, H2, C, P = shape
    fits = _lds_floats(F, H, H2, C, P) * 4 <= 160 * 1024
    assert L.pattern_head_train_supported(*shape) == fits
    got = _call(in_=F, ldx=F, w_audio=wa, hidden=H, hidden2=H2, classes=C, npat=P, keep=[1, 0] * P, workspace=None)
    assert got == (WORKSPACE if fits else INVALID)  # a supported shape reaches the workspace check


# ------------------------------------------------------------------------------------------------
# freeze_encoders and the refusals
# ------------------------------------------------------------------------------------------------
def _model(dropout=0.5):
    torch.manual_seed(0)
    return tspm_amd.AVMNIST(tspm_amd.ResNet18(1, 64), tspm_amd.ResNet34(1, 128), 128, dropout=dropout)


def _fake_adam(params):
    """A FusedAdam whose flat group holds ``params`` (the real one needs a device; the check reads flat_groups only)."""
    opt = tspm_amd.FusedAdam.__new__(tspm_amd.FusedAdam)
    opt._flat = [types.SimpleNamespace(params=list(params))]
    return opt


def test_freeze_pins_the_encoders_to_eval_whatever_the_mode():
    m = _model()
    assert m.frozen_encoders() == () and S.head_stage_frozen(m) == ()
    assert m.freeze_encoders() is m
    assert m.frozen_encoders() == ("audio_encoder", "image_encoder") == S.head_stage_frozen(m)
    enc = [p for n in m.frozen_encoders() for p in getattr(m, n).parameters()]
    assert enc and all(not p.requires_grad and p.grad is None for p in enc)
    assert all(p.requires_grad for p in m.net.parameters())
    for mode in (True, False, True):
        assert m.train(mode) is m
        assert m.training == mode and m.net.training == mode and m.net[2].training == mode   # the head's dropout follows
        assert not any(mod.training for n in m.frozen_encoders() for mod in getattr(m, n).modules())
    m.eval()
    assert not m.training
    m.train()
    m.unfreeze_encoders()
    assert m.frozen_encoders() == () and all(p.requires_grad for p in m.parameters())
    assert m.audio_encoder.training and m.image_encoder.layer1[0].bn1.training
    m.eval()
    assert not m.audio_encoder.training
    assert S.head_stage_frozen(m) == ()
    # the state_dict keys are what they were
    assert list(_model().state_dict()) == list(m.freeze_encoders().state_dict())


def test_an_unfrozen_model_keeps_its_keys():
    """Nothing frozen: the cache keys are the batch sizes, as before; a frozen model's end in ("frozen", names)."""
    m = _model()
    assert S.train_step_key(m, 128) == 128 and S.train_step_key(m, 1) == 1
    m.freeze_encoders()
    fr = ("frozen", ("audio_encoder", "image_encoder"))
    assert S.train_step_key(m, 128) == (128, fr)
    assert S.train_step_key(m, 4, ("a", "i")) == (("patterns", ("a", "i")), 4, fr)
    m.unfreeze_encoders()
    assert S.train_step_key(m, 128) == 128


def test_refusals_name_the_module_or_parameter():
    fr = lambda m, *a, **k: S.head_stage_frozen(m, *a, **k)  # noqa: E731
    # exactly one encoder frozen
    m = _model().freeze_encoders()
    for p in m.image_encoder.parameters():
        p.requires_grad_(True)
    with pytest.raises(L.TspmError, match=r"exactly one encoder is frozen \(audio_encoder; image_encoder is trainable\)"):
        fr(m)
    m = _model()
    for p in m.image_encoder.parameters():
        p.requires_grad_(False)
    with pytest.raises(L.TspmError, match=r"exactly one encoder is frozen \(image_encoder"):
        fr(m)
    # both frozen by hand, not pinned to eval
    for p in m.audio_encoder.parameters():
        p.requires_grad_(False)
    with pytest.raises(L.TspmError, match="audio_encoder: its parameters have requires_grad=False but the encoder is not "
                                          "pinned to eval"):
        fr(m)
    # frozen properly, then put back in train mode by hand
    m = _model().freeze_encoders()
    m.image_encoder.train()
    with pytest.raises(L.TspmError, match="image_encoder: .*not pinned to eval"):
        fr(m)
    m.train()
    assert fr(m) == m.frozen_encoders()
    # mixed flags inside an encoder
    m = _model()
    m.audio_encoder.layer2[0].conv1.weight.requires_grad_(False)
    with pytest.raises(L.TspmError, match=r"audio_encoder: mixed requires_grad flags.*audio_encoder\.layer2\.0\.conv1\.weight"):
        fr(m)
    # a head parameter that is not trainable (frozen encoders or not)
    for m in (_model(), _model().freeze_encoders()):
        m.net[3].bias.requires_grad_(False)
        with pytest.raises(L.TspmError, match=r"net\.3\.bias: a head parameter that is not trainable"):
            fr(m)
    # allreduce
    m = _model().freeze_encoders()
    with pytest.raises(L.TspmError, match="allreduce: data parallelism for the head stage"):
        fr(m, None, object())
    assert fr(_model(), None, object()) == ()   # an all-trainable model's DP step is not this function's business
    # an all_patterns batch without frozen encoders: the BatchNorm argument
    with pytest.raises(L.TspmError, match="exact only on frozen encoders.*BatchNorm on batch statistics"):
        fr(_model(), all_patterns=True)
    assert fr(_model().freeze_encoders(), all_patterns=True)


def test_optimizer_must_hold_exactly_the_trainable_parameters():
    m = _model()
    before = _fake_adam(m.parameters())            # built before freeze_encoders()
    m.freeze_encoders()
    with pytest.raises(L.TspmError, match=r"audio_encoder\.conv1\.weight is frozen but still in the FusedAdam's flat buffers"
                                          r".*built before freeze_encoders"):
        S.head_stage_frozen(m, before)
    after = _fake_adam(p for p in m.parameters() if p.requires_grad)
    assert S.head_stage_frozen(m, after) == m.frozen_encoders()
    short = _fake_adam(list(m.net.parameters())[1:])
    with pytest.raises(L.TspmError, match=r"net\.0\.weight is trainable but not in the FusedAdam's flat buffers"):
        S.head_stage_frozen(m, short)
    extra = _fake_adam(list(m.net.parameters()) + [torch.nn.Parameter(torch.zeros(4))])
    with pytest.raises(L.TspmError, match="holds parameters that are not the model's"):
        S.head_stage_frozen(m, extra)
    two = _fake_adam(m.net.parameters())
    two._flat = two._flat + [types.SimpleNamespace(params=[])]
    with pytest.raises(L.TspmError, match="one FusedAdam group"):
        S.head_stage_frozen(m, two)
    # an unfrozen model: the optimizer is not looked at
    assert S.head_stage_frozen(_model(), before) == ()


def test_steps_refuse_before_anything_is_built():
    """The step classes call the same check first: no device is touched (this test has none)."""
    m = _model()
    with pytest.raises(L.TspmError, match="exact only on frozen encoders"):
        S.FusedHeadStagePatternStep(m, _fake_adam(m.parameters()), None, 4)
    with pytest.raises(L.TspmError, match="not frozen"):
        S.FusedHeadStageStep(m, _fake_adam(m.parameters()), None, 4)
    m.freeze_encoders()
    with pytest.raises(L.TspmError, match="allreduce"):
        S.FusedHeadStageStep(m, _fake_adam(m.net.parameters()), None, 4, allreduce=object())
    with pytest.raises(L.TspmError, match="frozen but still in"):
        S.FusedHeadStageStep(m, _fake_adam(m.parameters()), None, 4)
    with pytest.raises(L.TspmError, match="frozen encoders .* trains with FusedHeadStageStep"):
        S.FusedTrainStep(m, _fake_adam(m.net.parameters()), None, 4)
    with pytest.raises(ValueError):
        S.FusedHeadStagePatternStep(m, _fake_adam(m.net.parameters()), None, 4, patterns=("a", "x"))
    assert S.DEFAULT_HEAD_STAGE_HEAD in ("kernel", "launches")


# ------------------------------------------------------------------------------------------------
# the loader
# ------------------------------------------------------------------------------------------------
def _ds(split="train", target="multimodal", n=40, **kw):
    return AVMNIST(None, split, target, corpus=synthetic_corpus(n, 6), **kw)


def test_all_pattern_loader_refusals():
    for split in ("valid", "test"):
        with pytest.raises(L.TspmError, match="train split"):
            _ds(split).device_loader(8, all_patterns=True)
    for target in ("audio", "image"):
        with pytest.raises(L.TspmError, match="multimodal"):
            _ds(target=target).device_loader(8, all_patterns=True)
    with pytest.raises(L.TspmError, match="pattern="):
        _ds().device_loader(8, all_patterns=True, pattern="a")
    with pytest.raises(L.TspmError, match="exclude each other"):
        _ds().device_loader(8, all_patterns=True, fuse_patterns=True)
    frac = {"ai": {"audio": 1.0, "image": 1.0}, "a": {"audio": 1.0, "image": 0.3}, "i": {"audio": 0.0, "image": 1.0}}
    with pytest.raises(L.TspmError, match="0 / 1"):
        DeviceLoader(_ds(missing_patterns=frac), 8, all_patterns=True)
    assert len(_ds(missing_patterns=frac, selected_patterns=["ai", "i"]).device_loader(8, all_patterns=True)) == 5
    with pytest.raises(TypeError):
        _ds().device_loader(8, all_paterns=True)


def test_all_pattern_loader_flags_and_order():
    ds = _ds()
    al = ds.device_loader(32, all_patterns=True)
    assert al.all_patterns and not al.fuse_patterns and len(al) == 2 == len(ds.device_loader(32))
    assert len(ds.device_loader(32, all_patterns=True, drop_last=True)) == 1
    assert list(al.items()) == list(range(40))
    # shuffled as before: the same draws from the same generator as the default loader
    g = lambda: torch.Generator().manual_seed(11)  # noqa: E731
    a = ds.device_loader(8, shuffle=True, generator=g(), all_patterns=True).items()
    b = ds.device_loader(8, shuffle=True, generator=g()).items()
    assert list(a) == list(b) and sorted(a) == list(range(40)) and list(a) != list(range(40))
    # the default loaders are what they were
    d = ds.device_loader(32)
    assert not d.all_patterns and not d.fuse_patterns
    assert _ds("valid").device_loader(32, fuse_patterns=True).fuse_patterns


# ------------------------------------------------------------------------------------------------
# the folding identity (fp64): fc0's weight gradient from B + 1 rows per modality equals autograd on the P*B rows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pats", [("a", "ai", "i"), ("a",), ("i", "ai"), ("ai",)], ids="+".join)
@pytest.mark.parametrize("shape", [(5, 12, 4, 8, 4, 3), (7, 192, 64, 128, 64, 10)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_folding_identity_fp64(shape, pats, p):
    B, F, wa, H, H2, C = shape
    x, x0, labels = R.inputs(B, F, C, seed=3)
    W = R.make_head(F, H, H2, C, seed=4)
    keep = R.keep_of(pats)
    mask = (torch.rand(len(pats) * B, H, generator=torch.Generator().manual_seed(5)) >= p).to(torch.uint8) if p else None
    ref = R.chain(x, x0, keep, wa, W, labels, loss_weight=0.7, p=p, mask=mask, dtype=torch.float64)
    gw0, gb0_a, gb0_i = R.folded_fc0_grads(ref["dz0"], x.double(), x0.double(), keep, wa)
    scale = ref["gw0"].abs().max().item()
    assert scale > 0
    assert (gw0 - ref["gw0"]).abs().max().item() <= 1e-13 * max(scale, 1.0)
    assert (gb0_a - ref["gb0"]).abs().max().item() <= 1e-13 and (gb0_i - ref["gb0"]).abs().max().item() <= 1e-13
    # the rows the chain formed are the expand's
    X = ref["X"].view(len(pats), B, F)
    for k, (ka, ki) in enumerate(keep):
        assert torch.equal(X[k, :, :wa], x[:, :wa].double() if ka else x0[:wa].double().expand(B, wa))
        assert torch.equal(X[k, :, wa:], x[:, wa:].double() if ki else x0[wa:].double().expand(B, F - wa))
