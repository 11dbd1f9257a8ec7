"""Every missing-modality pattern of a batch from one encoder pass, the parts that need no device: the new entry point
``tspm_pattern_expand`` (export, header, ctypes and a compiled call with the header's prototype agree; every refusal
returns before any launch, so it runs without a device), the loader's ``fuse_patterns`` mode on a synthetic corpus (the
index arithmetic and the refusals; the gather itself is device work), ``norm_patterns`` and the cache keys."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tspm_amd import _lib as L
from tspm_amd import harness
from tspm_amd import mosi as M
from tspm_amd.mosi_data import MOSI, PATTERNS, synthetic_mosi_corpus

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "tspm.h")
INVALID = 1
FAKE = 0x10000  # a 16-byte aligned non-NULL value: a refused call never dereferences (or launches with) it
PROTO = ("int tspm_pattern_expand(int32_t batch, int32_t npat, const int32_t* keep, const int32_t* group_id, "
         "int32_t w_audio, int32_t w_video, int32_t w_text, const float* emb, int64_t ld_emb, float* out, "
         "int64_t ld_out, const void* labels, void* labels_out, int32_t label_bytes, int32_t* groups_out, "
         "tspm_stream_t stream);")


# ------------------------------------------------------------------------------------------------
# the entry point
# ------------------------------------------------------------------------------------------------
def test_header_export_and_binding_agree():
    src = re.sub(r"\s+", " ", open(HEADER).read())
    assert PROTO in src
    assert "#define TSPM_ABI_VERSION 23 " in src and L.ABI_VERSION == 23 and L.lib().tspm_abi_version() == 23
    assert "#define TSPM_MAX_PATTERNS 7 " in src and L.MAX_PATTERNS == 7 == len(PATTERNS)
    assert "tspm_pattern_expand" in L.EXPORTED and hasattr(ctypes.CDLL(L.LIB_PATH), "tspm_pattern_expand")
    res, args = L._SIGS["tspm_pattern_expand"]
    P32, V = ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    assert res is i32 and args == [i32, i32, P32, P32, i32, i32, i32, V, i64, V, i64, V, V, i32, V, V]


_C_OF = {ctypes.c_int32: "int32_t", ctypes.c_int64: "int64_t", ctypes.POINTER(ctypes.c_int32): "pointer",
         ctypes.c_void_p: "pointer"}


def test_compiled_header_prototype_equals_the_binding(tmp_path):
    """PROTO's parameter types are the ctypes binding's, one for one (integer widths and which parameters are
    pointers), and a C file that includes the header and assigns the entry point to a
    function pointer of PROTO's type compiles with -Werror: the compiled header declares exactly that signature."""
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or \
        (rocm_clang if os.path.exists(rocm_clang) else None)
    if cc is None:
        pytest.fail("no C compiler to probe the header")
    res, args = L._SIGS["tspm_pattern_expand"]
    names = re.search(r"tspm_pattern_expand\((.*?)\);", PROTO).group(1).split(", ")
    ctypes_of_header = []
    for decl in names:  # "const int32_t* keep" -> the C type without qualifier and name
        ty = decl.rsplit(" ", 1)[0].replace("const ", "")
        ctypes_of_header.append("pointer" if ty.endswith("*") or ty == "tspm_stream_t" else ty)
    assert ctypes_of_header == [_C_OF[a] for a in args] and _C_OF[res] == "int32_t"
    probe = tmp_path / "probe.c"
    probe.write_text("\n".join([
        '#include "tspm.h"',
        f"typedef {PROTO.replace('tspm_pattern_expand', '(*expand_fn)')[:-1]};",
        "expand_fn fn = tspm_pattern_expand;",
        "typedef char stream_is_a_pointer[sizeof(tspm_stream_t) == sizeof(void*) ? 1 : -1];",
        "typedef char patterns[TSPM_MAX_PATTERNS == 7 ? 1 : -1];"]))
    obj = tmp_path / "probe.o"
    subprocess.run([cc, "-Werror", "-c", "-I", os.path.join(REPO, "include"), str(probe), "-o", str(obj)], check=True)
    bad = tmp_path / "bad.c"  # the probe can fail: one parameter short
    bad.write_text('#include "tspm.h"\nint (*fn)(int32_t, int32_t) = tspm_pattern_expand;\n')
    assert subprocess.run([cc, "-Werror", "-c", "-I", os.path.join(REPO, "include"), str(bad), "-o", str(obj)],
                          capture_output=True).returncode != 0


def _call(**kw):
    a = dict(batch=5, npat=2, keep=[1, 1, 1, 0, 0, 1], group=[0, 6], w=(8, 12, 5), emb=FAKE, ld_emb=32, out=FAKE,
             ld_out=28, labels=FAKE, labels_out=FAKE, label_bytes=8, groups_out=FAKE)
    a.update(kw)
    keep = None if a["keep"] is None else (ctypes.c_int32 * len(a["keep"]))(*a["keep"])
    group = None if a["group"] is None else (ctypes.c_int32 * len(a["group"]))(*a["group"])
    return L.lib().tspm_pattern_expand(a["batch"], a["npat"], keep, group, *a["w"], a["emb"], a["ld_emb"], a["out"],
                                       a["ld_out"], a["labels"], a["labels_out"], a["label_bytes"], a["groups_out"], None)


REFUSALS = [dict(batch=0), dict(batch=-3), dict(npat=0), dict(npat=8, keep=[1] * 24, group=[0] * 8), dict(w=(0, 12, 5)),
            dict(w=(8, -1, 5)), dict(w=(8, 12, 0)), dict(ld_emb=24), dict(ld_out=24), dict(keep=[1, 1, 1, 0, 0, 0]),
            dict(keep=[0, 0, 0, 1, 1, 1]), dict(keep=None), dict(group=None), dict(emb=None), dict(out=None),
            dict(labels=None), dict(labels_out=None), dict(groups_out=None), dict(label_bytes=2), dict(label_bytes=16),
            dict(label_bytes=0)]


@pytest.mark.parametrize("bad", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in r.items())[:40] for r in REFUSALS])
def test_every_refusal_returns_before_any_launch(bad):
    """TSPM_ERR_INVALID with pointers no launch could survive and no device in the process: nothing was launched."""
    assert _call(**bad) == INVALID


# ------------------------------------------------------------------------------------------------
# patterns and keys
# ------------------------------------------------------------------------------------------------
def test_norm_patterns():
    assert M.norm_patterns() == M.ALL_PATTERNS == tuple(PATTERNS) == ("atv", "at", "av", "tv", "a", "t", "v")
    assert M.norm_patterns(["v", "at"]) == ("v", "at")  # a subset, in the given order
    with pytest.raises(ValueError, match="Invalid patterns"):
        M.norm_patterns(["at", "x"])
    with pytest.raises(ValueError):
        M.norm_patterns([])
    with pytest.raises(ValueError):
        M.norm_patterns(["a", "a"])
    torch.manual_seed(0)
    model = M.build_utt_fusion("mosi", embd_sizes=(8, 12, 8))
    x = torch.zeros(2, 6, 5), torch.zeros(2, 6, 20), torch.zeros(2, 6, 768)
    with pytest.raises(ValueError, match="Invalid patterns"):  # as the dataset's constructor, before anything else
        model.forward_patterns(*x, patterns=["atv", "tav"])
    with pytest.raises(L.TspmError, match="no CPU fallback"):
        model.forward_patterns(*x)
    sig = inspect.signature(M.UttFusionModel.forward_patterns).parameters
    assert list(sig) == ["self", "A", "V", "T", "patterns", "lengths"]
    assert sig["patterns"].default is None and sig["lengths"].default is None


def test_existing_keys_are_unchanged_and_the_new_ones_differ():
    key = (128, 50, "cuda:0")
    assert M._frozen_key(M._text_lengths_key(M._ragged_key(key, False), False), ()) is key
    assert M._text_lengths_key(M._ragged_key(key, True), True) == (128, 50, "cuda:0", "ragged", "text_lengths")
    assert list(inspect.signature(M.UttFusionModel._engine).parameters) == ["self", "b", "t", "device", "ragged",
                                                                            "text_lengths"]
    assert list(inspect.signature(M.UttFusionModel.fused_step).parameters) == ["self", "optimizer", "loss_functions",
                                                                               "batch", "steps", "ragged", "text_lengths"]
    assert list(inspect.signature(M.FusedMosiEvalStep.__init__).parameters) == [
        "self", "model", "loss_functions", "batch", "steps", "log", "use_graph", "ragged", "text_lengths"]
    assert list(inspect.signature(M.MosiEngine.__init__).parameters)[:7] == [
        "self", "model", "batch", "steps", "device", "ragged", "text_lengths"]
    pk = M._pattern_key(key, M.ALL_PATTERNS)
    assert pk == (("patterns", M.ALL_PATTERNS),) + key and pk != key
    # every other key of the engine, step and eval_steps caches starts with an int (a batch size or an id)
    assert isinstance(pk[0], tuple) and M._pattern_key(key, ("v", "at")) != pk
    assert list(inspect.signature(M.FusedMosiPatternEvalStep.__init__).parameters) == [
        "self", "model", "loss_functions", "batch", "steps", "log", "patterns", "use_graph", "ragged", "text_lengths"]


def test_runner_keys(monkeypatch):
    """``eval_step_for`` and ``pattern_eval_step_for`` with the step classes replaced by recorders: the per-pattern keys
    are the ones they always were, the fused key has the ("patterns", names) head."""
    made = []

    class Step:
        def __init__(self, model, lf, b, t, log, **kw):
            self.eng, self.kw = ("engine", b, t, tuple(sorted(kw.items()))), kw
            made.append(self)
    monkeypatch.setattr(M, "FusedMosiEvalStep", Step)
    monkeypatch.setattr(M, "FusedMosiPatternEvalStep", Step)
    r = harness.MosiEpochRunner.__new__(harness.MosiEpochRunner)
    r.model = type("Model", (), {"_engine": lambda self, b, t, d, rg, tl: made[-1].eng if made else None,
                                 "_pattern_engine": lambda self, b, t, d, p, rg, tl: made[-1].eng if made else None})()
    r.loss_functions, r.log, r.device = None, None, "cuda:0"
    r.eval_steps, r.ragged, r.text_lengths, r.patterns = {}, False, False, None
    r.eval_step_for(5, (7, 9, 6))
    r.eval_step_for(5, 50, ragged=True, text_lengths=True)
    assert list(r.eval_steps) == [(5, (7, 9, 6)), (5, 50, "ragged", "text_lengths")]
    r.pattern_eval_step_for(5, (7, 9, 6))
    r.patterns = ("v", "at")
    r.pattern_eval_step_for(5, 50, ragged=True)
    assert list(r.eval_steps)[2:] == [(("patterns", M.ALL_PATTERNS), 5, (7, 9, 6)),
                                      (("patterns", ("v", "at")), 5, 50, "ragged")]
    assert made[-1].kw["patterns"] == ("v", "at") and len(set(r.eval_steps)) == 4


# ------------------------------------------------------------------------------------------------
# the loader
# ------------------------------------------------------------------------------------------------
class _Rows:
    """Stands in for the device gather: records the sample rows of every fused batch."""

    def __init__(self, ds, monkeypatch):
        self.rows = []
        monkeypatch.setattr(ds, "_collate_fused", self._collate)
        self.ds = ds

    def _collate(self, rows, step=None, pad_to=0):
        self.rows.append(np.asarray(rows).copy())
        return {"label": rows, "patterns": list(self.ds.selected_patterns), "fused_patterns": True}


def test_fused_loader_refusals_counts_and_order(monkeypatch):
    corpus = synthetic_mosi_corpus(20, seed=3, steps=6)
    dev = torch.device("cpu")  # nothing here touches a device
    with pytest.raises(L.TspmError, match="fuse_patterns"):
        MOSI(split="train", corpus=corpus, device=dev).loader(5, fuse_patterns=True)
    with pytest.raises(L.TspmError, match="fuse_patterns"):
        next(iter(MOSI(split="train", corpus=corpus, device=dev).device_loader(5, fuse_patterns=True)))
    with pytest.raises(L.TspmError, match="fuse_patterns"):
        MOSI(split="valid", corpus=corpus, device=dev, target_modality="audio").loader(5, fuse_patterns=True)
    for split in ("valid", "test"):
        ds = MOSI(split=split, corpus=corpus, device=dev, selected_patterns=["v", "at"])
        assert len(ds) == 40  # the dataset's own length is the per-pattern one, as before
        plain, fused = ds.loader(5), ds.loader(5, fuse_patterns=True)
        assert not plain.fuse_patterns and fused.fuse_patterns
        assert len(plain) == 8 and len(fused) == 4 and len(ds.loader(6, fuse_patterns=True)) == 4
        assert len(ds.loader(6, drop_last=True, fuse_patterns=True)) == 3
        rec = _Rows(ds, monkeypatch)
        batches = list(fused)
        assert len(batches) == 4 and np.array_equal(np.concatenate(rec.rows), np.arange(20))  # once, in sample order
        for b in batches:
            assert b["patterns"] == ["v", "at"] and b["fused_patterns"] is True and "pattern_name" not in b
        rec.rows.clear()
        assert [len(r["label"]) for r in ds.loader(6, fuse_patterns=True)] == [6, 6, 6, 2]
        rec.rows.clear()
        assert [len(r["label"]) for r in ds.loader(6, drop_last=True, fuse_patterns=True)] == [6, 6, 6]
    with pytest.raises(ValueError, match="Invalid patterns"):
        MOSI(split="valid", corpus=corpus, device=dev, selected_patterns=["va"])
    assert inspect.signature(MOSI.loader).parameters["fuse_patterns"].default is False
    assert inspect.signature(MOSI.device_loader).parameters["fuse_patterns"].default is False


def test_runner_points_a_fused_loader_at_the_pattern_step():
    corpus = synthetic_mosi_corpus(10, seed=3, steps=6)
    ds = MOSI(split="valid", corpus=corpus, device=torch.device("cpu"), selected_patterns=["v", "at"])
    r = harness.MosiEpochRunner.__new__(harness.MosiEpochRunner)
    r.patterns = None
    fused, plain = ds.loader(5, fuse_patterns=True), ds.loader(5)
    assert r.loader_for(fused, False).step_for == r.pattern_eval_step_for and r.patterns == ("v", "at")
    assert r.loader_for(plain, False).step_for == r.eval_step_for and r.patterns is None
    assert r.loader_for(plain, True).step_for == r.train_step_for
