"""Frozen encoders and per-group Adam, the parts that need no device: the three exports under ABI 23 (header, ctypes and
the library's symbol list agree, struct sizes included), their refusals before any launch, ``finetune_param_groups``, the
refusals of ``check_param_groups`` / ``frozen_encoders`` / ``FusedAdam.launch_multi``, and the cache keys with and without
a frozen set."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tspm_amd import _lib as L
from tspm_amd import mosi as M
from tspm_amd.optim import FusedAdam

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "tspm.h")
NAMES = ("tspm_adam_begin_multi", "tspm_adam_step_multi", "tspm_grad_clip_coef_multi")
INVALID, WORKSPACE = 1, 3
P = 4096  # an aligned non-NULL stand-in, never dereferenced (every call here is refused before a launch)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _params(name):
    return [p.strip() for p in re.search(r"\bint %s\((.*?)\);" % name, _header(), re.S).group(1).split(",")]


def _struct_fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), re.S).group(1)
    return [f.strip() for f in body.split(";") if f.strip()]


# ------------------------------------------------------------------------------------------------
# ABI
# ------------------------------------------------------------------------------------------------
def test_exports_header_and_binding_agree_under_abi_23():
    if not os.path.exists(L.LIB_PATH):
        pytest.fail(f"{L.LIB_PATH} is not built")
    lib = ctypes.CDLL(L.LIB_PATH)
    lib.tspm_abi_version.restype = ctypes.c_int32
    assert lib.tspm_abi_version() == 23 == L.ABI_VERSION
    assert re.search(r"#define TSPM_ABI_VERSION 23\b", open(HEADER).read())
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T tspm_" in ln}
    for name in NAMES:
        assert hasattr(lib, name) and name in exported and name in L.EXPORTED, name
    assert _params(NAMES[0]) == ["int32_t count", "const tspm_adam_seg* segs", "tspm_stream_t stream"]
    assert _params(NAMES[1]) == ["int32_t count", "const tspm_adam_seg* segs", "const float* clip_coef",
                                 "tspm_stream_t stream"]
    # tspm_grad_clip_coef's parameters with (count, grad) replaced by (count, ranges)
    assert _params(NAMES[2]) == ["int32_t count", "const tspm_grad_range* ranges"] + _params("tspm_grad_clip_coef")[2:]
    vp = ctypes.c_void_p
    assert L._SIGS[NAMES[0]] == (ctypes.c_int32, [ctypes.c_int32, ctypes.POINTER(L.AdamSeg), vp])
    assert L._SIGS[NAMES[1]] == (ctypes.c_int32, [ctypes.c_int32, ctypes.POINTER(L.AdamSeg), vp, vp])
    res, args = L._SIGS[NAMES[2]]
    res0, args0 = L._SIGS["tspm_grad_clip_coef"]
    assert res is res0 and list(args) == [ctypes.c_int32, ctypes.POINTER(L.GradRange)] + list(args0[2:])


def test_struct_layouts_match_the_header():
    assert re.search(r"#define TSPM_ADAM_MAX_SEGMENTS 8\b", open(HEADER).read()) and L.ADAM_MAX_SEGMENTS == 8
    seg = _struct_fields("tspm_adam_seg")
    assert seg == ["float* param", "const float* grad", "float* exp_avg", "float* exp_avg_sq", "int64_t count",
                   "tspm_adam_hyper* hyper"]
    assert [n for n, _ in L.AdamSeg._fields_] == [f.split()[-1] for f in seg]
    assert ctypes.sizeof(L.AdamSeg) == 6 * 8 and L.AdamSeg.count.offset == 32 and L.AdamSeg.hyper.offset == 40
    rng = _struct_fields("tspm_grad_range")
    assert rng == ["const float* grad", "int64_t count"]
    assert [n for n, _ in L.GradRange._fields_] == [f.split()[-1] for f in rng]
    assert ctypes.sizeof(L.GradRange) == 16 and L.GradRange.count.offset == 8
    # the C compiler's own sizes, when one is at hand (the header is plain C)
    import shutil
    cc = next((c for c in ("cc", "gcc", "clang") if shutil.which(c)), None)
    if cc is not None:
        src = ('#include "tspm.h"\n_Static_assert(sizeof(tspm_adam_seg) == 48, "seg");\n'
               '_Static_assert(sizeof(tspm_grad_range) == 16, "range");\n'
               '_Static_assert(sizeof(tspm_adam_hyper) == 64, "hyper");\n')
        r = subprocess.run([cc, "-x", "c", "-fsyntax-only", "-I", os.path.dirname(HEADER), "-"], input=src, text=True,
                           capture_output=True)
        assert r.returncode == 0, r.stderr


def _segs(*counts, param=P, hyper=P):
    segs = (L.AdamSeg * max(len(counts), 1))()
    for sg, n in zip(segs, counts):
        sg.param, sg.grad, sg.exp_avg, sg.exp_avg_sq, sg.count, sg.hyper = param, P, P, P, n, hyper
    return segs


def test_refusals_before_any_launch():
    lib = L.load()
    for fn in (lambda n, s: lib.tspm_adam_begin_multi(n, s, None), lambda n, s: lib.tspm_adam_step_multi(n, s, None, None),
               lambda n, s: lib.tspm_adam_step_multi(n, s, P, None)):
        assert fn(0, _segs(4)) == INVALID and fn(9, _segs(*[4] * 9)) == INVALID
        assert fn(1, None) == INVALID
        assert fn(2, _segs(4, -1)) == INVALID
        assert fn(2, _segs(4, 4, param=None)) == INVALID and fn(1, _segs(4, hyper=None)) == INVALID
        assert fn(2, _segs(8, 8, param=P + 4)) == INVALID  # 16-byte alignment, as tspm_adam_step
    # an all-empty list is valid and launches nothing (NULL buffers are fine in an empty segment)
    empty = (L.AdamSeg * 2)()
    assert lib.tspm_adam_step_multi(2, empty, None, None) == 0 and lib.tspm_adam_begin_multi(2, empty, None) == 0

    need = lib.tspm_grad_clip_workspace()

    def clip(n, ranges, max_norm=1.0, coef=P, ws=P, ws_bytes=need):
        arr = (L.GradRange * max(len(ranges), 1))(*[L.GradRange(g, c) for g, c in ranges])
        return lib.tspm_grad_clip_coef_multi(n, arr if ranges else None, 1.0, max_norm, coef, None, ws, ws_bytes, None)

    assert clip(0, [(P, 4)]) == INVALID and clip(9, [(P, 4)] * 9) == INVALID and clip(1, []) == INVALID
    assert clip(2, [(P, 4), (None, 4)]) == INVALID and clip(2, [(P, 4), (P, -1)]) == INVALID
    assert clip(2, [(None, 0), (None, 0)]) == INVALID  # no element at all, as count <= 0 of the single-range call
    assert clip(1, [(P, 4)], coef=None) == INVALID and clip(1, [(P, 4)], max_norm=0.0) == INVALID
    assert clip(2, [(P, 4), (None, 0)], ws=None) == WORKSPACE
    assert clip(2, [(P, 4), (P, 4)], ws_bytes=need - 1) == WORKSPACE
    assert lib.tspm_status_string(WORKSPACE) == b"workspace too small"


# ------------------------------------------------------------------------------------------------
# finetune_param_groups, the frozen set and the refusals
# ------------------------------------------------------------------------------------------------
def _model(name="mosi"):
    torch.manual_seed(0)
    return M.build_utt_fusion(name, embd_sizes=(8, 12, 8))


def _ids(ps):
    return [id(p) for p in ps]


def test_finetune_param_groups():
    m = _model()
    enc = list(m.netA.parameters()) + list(m.netV.parameters()) + list(m.netT.parameters())
    one = M.finetune_param_groups(m, lr=1e-3, weight_decay=1e-3)
    assert len(one) == 1 and _ids(one[0]["params"]) == _ids(m.parameters()) and M.frozen_encoders(m) == ()
    two = M.finetune_param_groups(m, lr=1e-3, weight_decay=1e-3, encoder_lr=1e-4)
    assert [(g["lr"], g["weight_decay"]) for g in two] == [(1e-3, 1e-3), (1e-4, 1e-3)]
    assert _ids(two[0]["params"]) == _ids(m.netC.parameters()) and _ids(two[1]["params"]) == _ids(enc)
    wd = M.finetune_param_groups(m, lr=1e-3, weight_decay=1e-3, encoder_weight_decay=0.0)
    assert [(g["lr"], g["weight_decay"]) for g in wd] == [(1e-3, 1e-3), (1e-3, 0.0)]
    assert all(p.requires_grad for p in m.parameters())
    fr = M.finetune_param_groups(m, lr=1e-3, weight_decay=1e-3, encoder_lr=1e-4, freeze=("text", "audio"))
    assert M.frozen_encoders(m) == ("audio", "text")  # audio, video, text order
    assert _ids(fr[1]["params"]) == _ids(m.netV.parameters()) and _ids(fr[0]["params"]) == _ids(m.netC.parameters())
    assert not any(p.requires_grad for p in list(m.netA.parameters()) + list(m.netT.parameters()))
    assert all(p.requires_grad for p in list(m.netV.parameters()) + list(m.netC.parameters()))
    assert M.check_param_groups(m, fr) == ("audio", "text")
    m2 = _model()
    all3 = M.finetune_param_groups(m2, lr=1e-3, weight_decay=0.0, encoder_lr=1e-4, freeze=("audio", "video", "text"))
    assert len(all3) == 1 and _ids(all3[0]["params"]) == _ids(m2.netC.parameters())
    folded = M.finetune_param_groups(_model(), lr=1e-3, weight_decay=0.0, freeze=("video",))
    assert len(folded) == 1 and len(folded[0]["params"]) == len(list(m.parameters())) - len(list(m.netV.parameters()))
    for bad in (("words",), ("audio", "audio")):
        with pytest.raises(L.TspmError):
            M.finetune_param_groups(_model(), lr=1e-3, weight_decay=0.0, freeze=bad)


def test_refusals_name_the_module_or_parameter():
    m = _model()
    m.netV.rnn.bias_hh_l0.requires_grad_(False)
    with pytest.raises(L.TspmError, match=r"netV.*rnn\.bias_hh_l0"):  # mixed flags
        M.frozen_encoders(m)
    with pytest.raises(L.TspmError, match="netV"):
        M.check_param_groups(m, [dict(params=list(m.parameters()))])
    assert M._frozen_state(m)[0] == ()  # ... which is not a frozen encoder
    m = _model()
    m.netC.fc_out.bias.requires_grad_(False)
    with pytest.raises(L.TspmError, match=r"netC.*fc_out\.bias"):
        M.frozen_encoders(m)
    m = _model()
    ps = list(m.parameters())
    with pytest.raises(L.TspmError, match=r"netA\.rnn\.weight_ih_l0 is in no FusedAdam parameter group"):
        M.check_param_groups(m, [dict(params=ps[1:])])
    with pytest.raises(L.TspmError, match=r"netA\.rnn\.weight_ih_l0 is in parameter groups 0 and 1"):
        M.check_param_groups(m, [dict(params=ps), dict(params=ps[:1])])
    two = M.finetune_param_groups(m, lr=1e-3, weight_decay=0.0, encoder_lr=1e-4)
    assert M.check_param_groups(m, two) == ()
    with pytest.raises(L.TspmError, match="allreduce"):
        M.check_param_groups(m, two, allreduce=lambda: None)
    assert M.check_param_groups(m, [dict(params=ps)], allreduce=lambda: None) == ()  # one group: as before
    nine = [dict(params=[p]) for p in ps[:8]] + [dict(params=ps[8:])]
    with pytest.raises(L.TspmError, match="1..8"):
        M.check_param_groups(m, nine)
    # a frozen parameter may sit in a group (a FusedAdam built after the freeze leaves it out of its flat buffers; the
    # flat-buffer test below is about one built before); an all-frozen group does not count
    M.finetune_param_groups(m, lr=1e-3, weight_decay=0.0, freeze=("audio",))
    assert M.check_param_groups(m, [dict(params=list(m.netC.parameters())), dict(params=list(m.netA.parameters())),
                                    dict(params=list(m.netV.parameters()) + list(m.netT.parameters()))],
                                allreduce=None) == ("audio",)
    with pytest.raises(L.TspmError):  # the step wants FusedAdam before it looks at a device
        M.FusedMosiStep(m, torch.optim.Adam(m.netC.parameters()), None, 6, 9)


class _Flat:
    """A stand-in for FusedAdam's flat group: the parameters its buffers hold (those trainable when it was built)."""

    def __init__(self, params):
        self.params = list(params)


def test_flat_buffers_must_hold_exactly_what_trains_now():
    """FusedAdam fixes its flat buffers when it is built; the flags may change afterwards, in either order."""
    m = _model()
    groups = [dict(params=list(m.parameters()))]
    built_all = [_Flat(m.parameters())]  # the optimizer was built with everything trainable
    assert M.check_param_groups(m, groups, None, built_all) == ()
    m.netA.requires_grad_(False)  # ... and netA frozen afterwards: it would still be updated
    assert M.check_param_groups(m, groups) == ("audio",)  # the groups alone cannot tell
    with pytest.raises(L.TspmError, match=r"netA\.rnn\.weight_ih_l0 is in FusedAdam's flat buffers.*rebuild FusedAdam"):
        M.check_param_groups(m, groups, None, built_all)
    built_frozen = [_Flat(p for p in m.parameters() if p.requires_grad)]  # built with netA frozen
    assert M.check_param_groups(m, groups, None, built_frozen) == ("audio",)
    m.netA.requires_grad_(True)  # ... and unfrozen afterwards: no gradient buffer
    with pytest.raises(L.TspmError, match=r"netA\.rnn\.weight_ih_l0 is not in FusedAdam's flat buffers.*rebuild FusedAdam"):
        M.check_param_groups(m, groups, None, built_frozen)
    # the group count and the allreduce refusal follow the flat groups too
    two = [_Flat(m.netC.parameters()), _Flat(p for n, p in m.named_parameters() if not n.startswith("netC"))]
    with pytest.raises(L.TspmError, match="allreduce"):
        M.check_param_groups(m, groups, lambda: None, two)
    with pytest.raises(L.TspmError, match="not of this model"):  # a stranger's gradient would enter the clip norm
        M.check_param_groups(m, groups, None, built_all + [_Flat([torch.nn.Parameter(torch.zeros(3))])])


def test_flag_state_follows_the_flags_and_the_modules():
    m = _model()
    flags, state = m.flag_state()
    assert all(flags) and len(flags) == len(list(m.parameters())) and state == ((), None)
    assert m.flag_state()[1] is state  # the answer is kept per flag tuple
    m.netV.rnn.bias_hh_l0.requires_grad_(False)
    assert m.flag_state()[1][0] == () and "netV" in m.flag_state()[1][1]  # mixed: an error, no frozen encoder
    m.netV.requires_grad_(False)
    assert m.flag_state()[1] == (("video",), None)
    m.netV.requires_grad_(True)
    assert m.flag_state()[1] is state  # corrected flags: no error lingers
    m.netT = M.TextCNN(input_size=768, embd_size=8).requires_grad_(False)  # a module swapped in
    assert m.flag_state()[1] == (("text",), None) and len(m.flag_state()[0]) == len(list(m.parameters()))


def test_launch_multi_refuses_more_than_eight_groups():
    opt = FusedAdam.__new__(FusedAdam)
    opt.clip_coef = None
    opt.flat_groups = lambda: [object()] * 9
    with pytest.raises(L.TspmError, match="1..8"):
        opt.launch_multi(None)
    opt.flat_groups = lambda: []
    with pytest.raises(L.TspmError):
        opt.launch_multi(None)


def test_cache_keys_with_and_without_a_frozen_set():
    key = (128, 50, "cuda:0")
    assert M._frozen_key(key, ()) is key  # nothing frozen: the key as it always was
    assert M._frozen_key(key, ("audio", "text")) == key + (("frozen", ("audio", "text")),)
    full = M._frozen_key(M._text_lengths_key(M._ragged_key(key, True), True), ("video",))
    assert full == key + ("ragged", "text_lengths", ("frozen", ("video",)))  # after the length modes
    assert M._text_lengths_key(M._ragged_key(key, False), False) is key
    m = _model()
    assert M._frozen_state(m) == ((), None)
    m.netT.requires_grad_(False)
    m.netA.requires_grad_(False)
    assert M._frozen_state(m) == (("audio", "text"), None)
    assert M.ENCODER_MODULES == (("audio", "netA"), ("video", "netV"), ("text", "netT"))
