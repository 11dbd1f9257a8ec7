"""Every missing-modality pattern of an AVMNIST batch in one eval pass, the parts that need no device: the entry point
``tspm_pattern_head_eval`` (export, header and ctypes agree; every refusal returns before any launch, so it runs without
a device, and ``_lib.pattern_head_eval_supported`` predicts the shape refusals), the pattern names, and the loader's
``fuse_patterns`` mode on a synthetic corpus (the refusals and the batch count; the gather itself is device work)."""
import ctypes
import os
import re

import pytest

from tspm_amd import _lib as L
from tspm_amd import step as S
from tspm_amd.data import AVMNIST, DeviceLoader, synthetic_corpus

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "tspm.h")
OK, INVALID, WORKSPACE = 0, 1, 3
FAKE = 0x10000  # a 16-byte aligned non-NULL value: a refused call never dereferences (or launches with) it


def test_header_export_and_binding_agree():
    src = re.sub(r"\s+", " ", open(HEADER).read())
    assert "int tspm_pattern_head_eval(const tspm_pattern_head_eval_desc* desc, tspm_stream_t stream);" in src
    assert "size_t tspm_pattern_head_eval_workspace(int32_t batch, int32_t npat);" in src
    assert "#define TSPM_ABI_VERSION 23 " in src and L.ABI_VERSION == 23 and L.lib().tspm_abi_version() == 23
    assert "#define TSPM_PATTERN_HEAD_MAX_PATTERNS 8 " in src and L.PATTERN_HEAD_MAX_PATTERNS == 8
    so = ctypes.CDLL(L.LIB_PATH)
    for name in ("tspm_pattern_head_eval", "tspm_pattern_head_eval_workspace"):
        assert name in L.EXPORTED and hasattr(so, name)
    # the descriptor's fields, in the header's order, are the binding's (names, and which are pointers)
    body = re.search(r"typedef struct tspm_pattern_head_eval_desc \{(.*?)\} tspm_pattern_head_eval_desc;", src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body)
    names = []
    for decl in body.split(";"):
        names += re.findall(r"(\w+)\s*(?:,|$)", decl.strip())
    assert names == [n.rstrip("_") for n, _ in L.PatternHeadEvalDesc._fields_]
    # 8 int32, 11 pointers, float + int32, 6 pointers, int64, pointer, size_t — no padding anywhere
    assert ctypes.sizeof(L.PatternHeadEvalDesc) == 8 * 4 + 11 * 8 + 8 + 6 * 8 + 8 + 8 + 8
    assert L.lib().tspm_pattern_head_eval_workspace(7, 3) >= 7 * 3 * 4
    assert L.lib().tspm_pattern_head_eval_workspace(0, 3) == 0 == L.lib().tspm_pattern_head_eval_workspace(7, 9)


GOOD = dict(batch=7, npat=3, in_=192, w_audio=64, hidden=128, hidden2=64, classes=10, ldx=192, x=FAKE, x0=FAKE,
            keep=[1, 0, 1, 1, 0, 1], group_id=[0, 1, 2], w0=FAKE, b0=FAKE, w3=FAKE, b3=FAKE, w5=FAKE, b5=FAKE,
            labels=FAKE, loss_weight=1.0, n_groups=3, logits=FAKE, preds=FAKE, loss=FAKE, confusion=FAKE, loss_log=FAKE,
            counters=FAKE, log_capacity=16, workspace=FAKE, workspace_bytes=1 << 20)


def _call(**kw):
    a = dict(GOOD)
    a.update(kw)
    for k in ("keep", "group_id"):
        a[k] = None if a[k] is None else (ctypes.c_int32 * len(a[k]))(*a[k])
    return L.lib().tspm_pattern_head_eval(L.PatternHeadEvalDesc(**a), None)


SHAPE_REFUSALS = [dict(in_=260, ldx=260), dict(hidden=260), dict(hidden2=132), dict(classes=17), dict(in_=190),
                  dict(w_audio=62), dict(hidden=126), dict(hidden2=62), dict(w_audio=0), dict(w_audio=192),
                  dict(npat=0), dict(npat=9, keep=[1] * 18, group_id=[0] * 9), dict(classes=0), dict(hidden=0),
                  dict(in_=256, ldx=256, hidden=256)]  # 256 x 260 floats of w0 alone: past 160 KiB of LDS
OTHER_REFUSALS = [dict(batch=0), dict(batch=-2), dict(ldx=188), dict(ldx=194), dict(x=FAKE + 4), dict(x0=FAKE + 8),
                  dict(w0=FAKE + 4), dict(w3=FAKE + 4), dict(w5=FAKE + 4), dict(x0=None), dict(log_capacity=-1),
                  dict(counters=None), dict(n_groups=0)] + \
                 [{k: None} for k in ("x", "keep", "group_id", "w0", "b0", "w3", "b3", "w5", "b5", "labels", "logits",
                                      "loss")]
_ids = lambda rs: [",".join(f"{k}={v}" for k, v in r.items())[:40] for r in rs]  # noqa: E731


@pytest.mark.parametrize("bad", SHAPE_REFUSALS, ids=_ids(SHAPE_REFUSALS))
def test_shape_refusals_and_supported_agree(bad):
    """TSPM_ERR_INVALID with pointers no launch could survive and no device in the process: nothing was launched;
    ``pattern_head_eval_supported`` says the same of the shape."""
    a = dict(GOOD)
    a.update(bad)
    assert _call(**bad) == INVALID
    assert not L.pattern_head_eval_supported(a["in_"], a["w_audio"], a["hidden"], a["hidden2"], a["classes"], a["npat"])


@pytest.mark.parametrize("bad", OTHER_REFUSALS, ids=_ids(OTHER_REFUSALS))
def test_pointer_and_argument_refusals(bad):
    assert _call(**bad) == INVALID
    assert L.pattern_head_eval_supported(192, 64, 128, 64, 10, 3)  # the shape itself is fine


def test_workspace_refusals_and_nullable_arguments():
    assert _call(workspace=None) == WORKSPACE and _call(workspace_bytes=7 * 3 * 4 - 1) == WORKSPACE
    assert _call(workspace=FAKE + 8) == WORKSPACE
    # a bad shape wins over a bad workspace
    assert _call(workspace=None, hidden=126) == INVALID
    # x0 may be NULL only when every pattern keeps both modalities (checked before the workspace)
    assert _call(x0=None, npat=1, keep=[1, 1], group_id=[1], workspace=None) == WORKSPACE
    assert _call(x0=None, npat=1, keep=[1, 0], group_id=[0], workspace=None) == INVALID
    # the log's pieces are nullable (checked before the workspace): no confusion, no loss log, no counters
    assert _call(confusion=None, n_groups=0, workspace=None) == WORKSPACE
    assert _call(loss_log=None, counters=None, preds=None, workspace=None) == WORKSPACE


@pytest.mark.parametrize("shape", [(12, 4, 8, 4, 3, 3), (192, 64, 128, 64, 10, 3), (192, 64, 128, 64, 10, 1),
                                   (192, 64, 128, 64, 10, 8), (256, 128, 64, 32, 16, 8), (64, 32, 256, 64, 16, 8)])
def test_supported_shapes_reach_the_workspace_check(shape):
    F, wa, H, H2, C, P = shape
    assert L.pattern_head_eval_supported(*shape)
    assert _call(in_=F, ldx=F, w_audio=wa, hidden=H, hidden2=H2, classes=C, npat=P, keep=[1, 0] * P,
                 group_id=list(range(P)), workspace=None) == WORKSPACE


def test_pattern_names():
    assert S.norm_avmnist_patterns() == S.AVMNIST_PATTERNS == tuple(AVMNIST.get_all_possible_patterns()) == ("a", "ai", "i")
    assert S.norm_avmnist_patterns(["i", "ai"]) == ("i", "ai")
    assert S.PATTERN_KEEP == {"a": (1, 0), "ai": (1, 1), "i": (0, 1)}
    for bad in (["x"], ["a", "ia"], [], ["a", "a"]):
        with pytest.raises(ValueError):
            S.norm_avmnist_patterns(bad)
    assert S.DEFAULT_PATTERN_HEAD in ("kernel", "launches")


# ------------------------------------------------------------------------------------------------
# the loader
# ------------------------------------------------------------------------------------------------
def _ds(split="valid", target="multimodal", n=40, **kw):
    return AVMNIST(None, split, target, corpus=synthetic_corpus(n, 6), **kw)


def test_fused_loader_refusals():
    with pytest.raises(L.TspmError, match="valid / test"):
        _ds("train").device_loader(8, fuse_patterns=True)
    for target in ("audio", "image"):
        with pytest.raises(L.TspmError, match="multimodal"):
            _ds(target=target).device_loader(8, fuse_patterns=True)
    with pytest.raises(L.TspmError, match="pattern="):
        _ds().device_loader(8, fuse_patterns=True, pattern="a")
    frac = {"ai": {"audio": 1.0, "image": 1.0}, "a": {"audio": 1.0, "image": 0.3}, "i": {"audio": 0.0, "image": 1.0}}
    with pytest.raises(L.TspmError, match="0 / 1"):
        DeviceLoader(_ds(missing_patterns=frac), 8, fuse_patterns=True)
    # ... unless the fractional pattern is not selected
    assert len(_ds(missing_patterns=frac, selected_patterns=["ai", "i"]).device_loader(8, fuse_patterns=True)) == 5
    with pytest.raises(TypeError):
        _ds().device_loader(8, fuse_paterns=True)


@pytest.mark.parametrize("split", ["valid", "test"])
def test_fused_loader_len_counts_sample_batches(split):
    ds = _ds(split)
    assert len(ds) == 120 and len(ds.device_loader(32)) == 4
    fl = ds.device_loader(32, fuse_patterns=True)
    assert fl.fuse_patterns and len(fl) == 2                       # ceil(40 / 32), not ceil(120 / 32)
    assert len(ds.device_loader(32, fuse_patterns=True, drop_last=True)) == 1
    assert len(ds.device_loader(8, fuse_patterns=True)) == 5
    assert list(fl.items()) == list(range(40))                    # each sample once, in sample order
    # distributed sharding is over the N samples
    shards = [ds.device_loader(8, fuse_patterns=True, rank=r, world_size=2) for r in range(2)]
    assert [len(s) for s in shards] == [3, 3]
    assert sorted(int(i) for s in shards for i in s.items()) == list(range(40))
    # the default loader is what it was
    assert not ds.device_loader(32).fuse_patterns and list(ds.device_loader(32).items()) == list(range(120))
