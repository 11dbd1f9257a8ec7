"""Every missing-modality pattern of an MMIMDb batch in one eval pass, the parts that need no device: the pattern names,
the two entry points ``tspm_gmu_pattern_fwd`` / ``tspm_bce_logits_patterns`` (export, header and ctypes agree; every
refusal returns before any launch, so it runs without a device, and ``_lib.gmu_pattern_supported`` predicts the shape
refusals), and the algebra the pass rests on, in fp64 on the CPU oracle: choosing, per pattern and modality, the real
row's or the zero-input row's half of the fusion's projection buffer reproduces the eval forward on the masked inputs."""
import ctypes
import os
import re

import pytest
import torch

from oracle import mmimdb_ref as orc
from parity import rel_l2
from tspm_amd import _lib as L
from tspm_amd import mmimdb as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "tspm.h")
OK, INVALID = 0, 1
FAKE = 0x10000  # a non-NULL value: a refused call never dereferences (or launches with) it


def test_pattern_names():
    assert M.norm_mmimdb_patterns() == M.MMIMDB_PATTERNS == ("it", "i", "t") == tuple(M.PATTERNS)
    assert M.norm_mmimdb_patterns(["t", "it"]) == ("t", "it")
    assert M.norm_mmimdb_patterns(("i",)) == ("i",)
    for bad in (["x"], ["it", "ti"], [], ["i", "i"]):
        with pytest.raises(ValueError):
            M.norm_mmimdb_patterns(bad)
    assert M.DEFAULT_PATTERN_FUSION in ("kernel", "launches")


def test_header_export_and_binding_agree():
    src = re.sub(r"\s+", " ", open(HEADER).read())
    assert ("int tspm_gmu_pattern_fwd(int32_t batch, int32_t npat, const int32_t* keep, int32_t d, const float* u, "
            "int32_t ldu, const float* u0, const float* wz, float* h, int32_t ldh, float* gate, float* z, int32_t ldz, "
            "tspm_stream_t stream);") in src
    assert ("int tspm_bce_logits_patterns(int32_t batch, int32_t npat, int32_t classes, const float* logits, "
            "const float* targets, float grad_scale, float threshold, float* loss, float* stats, float* loss_log, "
            "int64_t* counters, int64_t log_capacity, tspm_stream_t stream);") in src
    assert "#define TSPM_ABI_VERSION 23 " in src and L.ABI_VERSION == 23 and L.lib().tspm_abi_version() == 23
    assert f"#define TSPM_GMU_PATTERN_MAX_D {L.GMU_PATTERN_MAX_D} " in src
    assert (4 * L.GMU_PATTERN_MAX_D + 4) * 4 <= 64 * 1024 < (4 * (L.GMU_PATTERN_MAX_D + 1) + 4) * 4  # the LDS carve
    so = ctypes.CDLL(L.LIB_PATH)
    for name in ("tspm_gmu_pattern_fwd", "tspm_bce_logits_patterns"):
        assert name in L.EXPORTED and hasattr(so, name)


# ------------------------------------------------------------------------------------------------
# tspm_gmu_pattern_fwd
# ------------------------------------------------------------------------------------------------
GMU_GOOD = dict(batch=5, npat=3, keep=[1, 1, 1, 0, 0, 1], d=68, u=FAKE, ldu=136, u0=FAKE, wz=FAKE, h=FAKE, ldh=136,
                gate=FAKE, z=FAKE, ldz=68)


def _gmu(**kw):
    a = dict(GMU_GOOD)
    a.update(kw)
    keep = None if a["keep"] is None else (ctypes.c_int32 * len(a["keep"]))(*a["keep"])
    return L.lib().tspm_gmu_pattern_fwd(a["batch"], a["npat"], keep, a["d"], a["u"], a["ldu"], a["u0"], a["wz"], a["h"],
                                        a["ldh"], a["gate"], a["z"], a["ldz"], None)


GMU_SHAPE_REFUSALS = [dict(npat=0), dict(npat=L.MAX_PATTERNS + 1, keep=[1, 1] * (L.MAX_PATTERNS + 1)), dict(d=0),
                      dict(d=-4), dict(d=L.GMU_PATTERN_MAX_D + 1, ldu=2 * L.GMU_PATTERN_MAX_D + 2,
                                       ldh=2 * L.GMU_PATTERN_MAX_D + 2, ldz=L.GMU_PATTERN_MAX_D + 1)]
GMU_OTHER_REFUSALS = [dict(batch=0), dict(batch=-3), dict(keep=[1, 1, 0, 0, 0, 1]), dict(ldu=135), dict(ldh=135),
                      dict(ldz=67), dict(u0=None), dict(u0=None, npat=2, keep=[1, 1, 0, 1])] + \
                     [{k: None} for k in ("keep", "u", "wz", "z")]
_ids = lambda rs: [",".join(f"{k}={v}" for k, v in r.items())[:40] for r in rs]  # noqa: E731


@pytest.mark.parametrize("bad", GMU_SHAPE_REFUSALS, ids=_ids(GMU_SHAPE_REFUSALS))
def test_gmu_pattern_shape_refusals_and_supported_agree(bad):
    """TSPM_ERR_INVALID with pointers no launch could survive and no device in the process: nothing was launched;
    ``gmu_pattern_supported`` says the same of the shape."""
    a = dict(GMU_GOOD)
    a.update(bad)
    assert _gmu(**bad) == INVALID
    assert not L.gmu_pattern_supported(a["d"], a["npat"])


@pytest.mark.parametrize("bad", GMU_OTHER_REFUSALS, ids=_ids(GMU_OTHER_REFUSALS))
def test_gmu_pattern_pointer_and_argument_refusals(bad):
    assert _gmu(**bad) == INVALID
    assert L.gmu_pattern_supported(GMU_GOOD["d"], GMU_GOOD["npat"])  # the shape itself is fine


@pytest.mark.parametrize("d,npat", [(1, 1), (4, 3), (512, 3), (L.GMU_PATTERN_MAX_D, L.MAX_PATTERNS)])
def test_gmu_pattern_supported_shapes(d, npat):
    """A supported shape is refused for its pointers alone: with everything else valid, only the NULL output stops it."""
    assert L.gmu_pattern_supported(d, npat)
    assert _gmu(d=d, npat=npat, keep=[1, 0] * npat, ldu=2 * d, ldh=2 * d, ldz=d, z=None) == INVALID
    assert not L.gmu_pattern_supported(d, 0) and not L.gmu_pattern_supported(0, npat)


# ------------------------------------------------------------------------------------------------
# tspm_bce_logits_patterns
# ------------------------------------------------------------------------------------------------
BCE_GOOD = dict(batch=5, npat=3, classes=23, logits=FAKE, targets=FAKE, grad_scale=1.0, threshold=0.5, loss=FAKE,
                stats=FAKE, loss_log=FAKE, counters=FAKE, log_capacity=16)
BCE_REFUSALS = [dict(batch=0), dict(batch=-1), dict(npat=0), dict(npat=L.MAX_PATTERNS + 1), dict(classes=0),
                dict(logits=None), dict(targets=None), dict(loss=None), dict(counters=None), dict(log_capacity=-1)]


@pytest.mark.parametrize("bad", BCE_REFUSALS, ids=_ids(BCE_REFUSALS))
def test_bce_logits_patterns_refusals(bad):
    a = dict(BCE_GOOD)
    a.update(bad)
    assert L.lib().tspm_bce_logits_patterns(*[a[k] for k in BCE_GOOD], None) == INVALID


# ------------------------------------------------------------------------------------------------
# the algebra, in fp64
# ------------------------------------------------------------------------------------------------
DIMS = dict(image_dim=40, text_dim=12, embed=16, hidden=8, genres=5)


def _oracle64(pooling):
    """A small oracle model in fp64 with non-trivial BatchNorm statistics and affine parameters (a fresh model's zero
    row would be the biases alone)."""
    m = orc.build_oracle_mmimdb(3, pooling=pooling, **DIMS).double()
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                c = mod.num_features
                mod.running_mean.copy_(torch.randn(c, generator=g, dtype=torch.float64) * 0.3)
                mod.running_var.copy_(torch.rand(c, generator=g, dtype=torch.float64) + 0.5)
                mod.weight.copy_(torch.rand(c, generator=g, dtype=torch.float64) + 0.5)
                mod.bias.copy_(torch.randn(c, generator=g, dtype=torch.float64) * 0.2)
    return m.eval()


def _projections(m, I, T):
    f = m.fusion_module
    pa, pb = (f.proj_a, f.proj_b) if m.fusion_type == "pooling" else (f.fc_one, f.fc_two)
    return torch.cat([pa(m.image_model(I)), pb(m.text_model(T))], dim=1)


def _fuse_from_projections(m, U):
    """The fusion after its two projections, restated on U = [proj(image) | proj(text)] (eval mode: no dropout)."""
    f, d = m.fusion_module, U.shape[1] // 2
    a, b = torch.tanh(U[:, :d]), torch.tanh(U[:, d:])
    cat = torch.cat([a, b], dim=1)
    if m.fusion_type != "pooling":
        g = torch.sigmoid(f.hidden_sigmoid(cat))
        return g * a + (1 - g) * b
    if f.pooling_type == "max":
        return torch.max(a, b)
    if f.pooling_type == "attention":
        s = f.attention_layer(cat)
        return s[:, :1] * a + s[:, 1:] * b
    raise AssertionError(f.pooling_type)


@pytest.mark.parametrize("pooling", [None, {"pooling_type": "attention", "hidden_dim": 8, "dropout": 0.1},
                                     {"pooling_type": "max", "dropout": 0.1}], ids=["gmu", "attention", "max"])
def test_selection_at_the_projection_rows_equals_masked_inputs(pooling):
    m = _oracle64(pooling)
    I, T, _ = orc.synthetic_batch(7, seed=5, image_dim=DIMS["image_dim"], text_dim=DIMS["text_dim"],
                                  genres=DIMS["genres"])
    I, T = I.double(), T.double()
    d = DIMS["embed"]
    with torch.no_grad():
        U = _projections(m, I, T)
        u0 = _projections(m, torch.zeros_like(I[:1]), torch.zeros_like(T[:1]))
        assert float(u0.abs().min()) > 0  # the zero row is no zero vector
        for name, (ip, tp) in M.PATTERNS.items():
            sel = torch.cat([U[:, :d] if ip else u0[:, :d].expand(7, d), U[:, d:] if tp else u0[:, d:].expand(7, d)], 1)
            got = m.mm_mlp(_fuse_from_projections(m, sel))
            want = orc.eval_forward(m, I * ip, T * tp)
            e = rel_l2(got, want)
            print(f"{name}: rel-L2 {e:.2e}")
            assert e <= 1e-13, (name, e)
