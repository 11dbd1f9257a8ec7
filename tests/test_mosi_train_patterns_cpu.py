"""Training every missing-modality pattern of a batch in one step, the parts that need no device: the entry point
``tspm_pattern_expand_bwd`` (export, header, ctypes and a compiled call with the header's prototype agree; every refusal
returns before any launch), the loader's ``all_patterns`` mode on a synthetic corpus (index arithmetic, batch keys and
refusals; the gather itself is device work), the runner's choice of step and the cache keys."""
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
from tspm_amd.mosi_data import MOSI, synthetic_mosi_corpus

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "tspm.h")
INVALID = 1
FAKE = 0x10000  # a 16-byte aligned non-NULL value: a refused call never dereferences (or launches with) it
NAME = "tspm_pattern_expand_bwd"
PROTO = ("int tspm_pattern_expand_bwd(int32_t batch, int32_t npat, const int32_t* keep, int32_t w_audio, "
         "int32_t w_video, int32_t w_text, const float* dout, int64_t ld_dout, float* demb, int64_t ld_demb, "
         "int32_t modalities, tspm_stream_t stream);")


# ------------------------------------------------------------------------------------------------
# the entry point
# ------------------------------------------------------------------------------------------------
def test_header_export_and_binding_agree():
    src = re.sub(r"\s+", " ", open(HEADER).read())
    assert PROTO in src
    assert "#define TSPM_ABI_VERSION 23 " in src and L.ABI_VERSION == 23 and L.lib().tspm_abi_version() == 23
    assert NAME in L.EXPORTED and hasattr(ctypes.CDLL(L.LIB_PATH), NAME)
    res, args = L._SIGS[NAME]
    P32, V = ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    assert res is i32 and args == [i32, i32, P32, i32, i32, i32, V, i64, V, i64, i32, V]


_C_OF = {ctypes.c_int32: "int32_t", ctypes.c_int64: "int64_t", ctypes.POINTER(ctypes.c_int32): "pointer",
         ctypes.c_void_p: "pointer"}


def test_compiled_header_prototype_equals_the_binding(tmp_path):
    """PROTO's parameter types are the ctypes binding's, one for one, and a C file that includes the header and assigns
    the entry point to a function pointer of PROTO's type compiles with -Werror (and one of another type does not)."""
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or \
        (rocm_clang if os.path.exists(rocm_clang) else None)
    if cc is None:
        pytest.fail("no C compiler to probe the header")
    res, args = L._SIGS[NAME]
    names = re.search(NAME + r"\((.*?)\);", PROTO).group(1).split(", ")
    ctypes_of_header = []
    for decl in names:  # "const int32_t* keep" -> the C type without qualifier and name
        ty = decl.rsplit(" ", 1)[0].replace("const ", "")
        ctypes_of_header.append("pointer" if ty.endswith("*") or ty == "tspm_stream_t" else ty)
    assert ctypes_of_header == [_C_OF[a] for a in args] and _C_OF[res] == "int32_t"
    probe = tmp_path / "probe.c"
    probe.write_text("\n".join(['#include "tspm.h"', f"typedef {PROTO.replace(NAME, '(*bwd_fn)')[:-1]};",
                                f"bwd_fn fn = {NAME};"]))
    obj = tmp_path / "probe.o"
    subprocess.run([cc, "-Werror", "-c", "-I", os.path.join(REPO, "include"), str(probe), "-o", str(obj)], check=True)
    bad = tmp_path / "bad.c"  # the probe can fail: the forward's prototype is not the backward's
    bad.write_text(f'#include "tspm.h"\nint (*fn)(int32_t, int32_t, const int32_t*, const int32_t*) = {NAME};\n')
    assert subprocess.run([cc, "-Werror", "-c", "-I", os.path.join(REPO, "include"), str(bad), "-o", str(obj)],
                          capture_output=True).returncode != 0


def _call(**kw):
    a = dict(batch=5, npat=2, keep=[1, 1, 1, 0, 0, 1], w=(8, 12, 5), dout=FAKE, ld_dout=28, demb=FAKE, ld_demb=32,
             modalities=7)
    a.update(kw)
    keep = None if a["keep"] is None else (ctypes.c_int32 * len(a["keep"]))(*a["keep"])
    return L.lib().tspm_pattern_expand_bwd(a["batch"], a["npat"], keep, *a["w"], a["dout"], a["ld_dout"], a["demb"],
                                           a["ld_demb"], a["modalities"], None)


REFUSALS = [dict(batch=0), dict(batch=-3), dict(npat=0), dict(npat=8, keep=[1] * 24), dict(w=(0, 12, 5)),
            dict(w=(8, -1, 5)), dict(w=(8, 12, 0)), dict(ld_dout=24), dict(ld_demb=24), dict(keep=[1, 1, 1, 0, 0, 0]),
            dict(keep=[0, 0, 0, 1, 1, 1]), dict(keep=None), dict(dout=None), dict(demb=None), dict(modalities=0),
            dict(modalities=8), dict(modalities=-1)]


@pytest.mark.parametrize("bad", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in r.items())[:40] for r in REFUSALS])
def test_every_refusal_returns_before_any_launch(bad):
    """TSPM_ERR_INVALID with pointers no launch could survive and no device in the process: nothing was launched."""
    assert _call(**bad) == INVALID


# ------------------------------------------------------------------------------------------------
# keys and signatures
# ------------------------------------------------------------------------------------------------
def test_fused_step_keys_are_unchanged_and_the_pattern_key_differs():
    torch.manual_seed(0)
    model = M.build_utt_fusion("mosi", embd_sizes=(8, 12, 8))
    opt, lf = object(), None
    plain = model._fused_step_key(opt, lf, 5, (7, 9, 6))
    assert plain == (id(opt), id(lf), 5, (7, 9, 6))  # the key fused_step always had
    assert model._fused_step_key(opt, lf, 5, (50, 50, 50), True, True) == (id(opt), id(lf), 5, 50, "ragged",
                                                                           "text_lengths")
    pk = model._fused_step_key(opt, lf, 5, (7, 9, 6), patterns=None)
    assert pk == plain
    pk = model._fused_step_key(opt, lf, 5, (7, 9, 6), patterns=("v", "at"))
    assert pk == (("patterns", ("v", "at")),) + plain and pk != plain
    assert model._fused_step_key(opt, lf, 5, (7, 9, 6), patterns=M.ALL_PATTERNS) != pk
    model.netT.requires_grad_(False)  # the frozen element trails, behind the same head
    assert model._fused_step_key(opt, lf, 5, 50, patterns=("a",)) == (("patterns", ("a",)), id(opt), id(lf), 5, 50,
                                                                      ("frozen", ("text",)))
    assert list(inspect.signature(M.UttFusionModel.fused_step).parameters) == [
        "self", "optimizer", "loss_functions", "batch", "steps", "ragged", "text_lengths"]
    assert list(inspect.signature(M.UttFusionModel.fused_pattern_step).parameters) == [
        "self", "optimizer", "loss_functions", "batch", "steps", "patterns", "ragged", "text_lengths"]
    sig = inspect.signature(M.FusedMosiPatternStep.__init__).parameters
    assert list(sig)[:10] == ["self", "model", "optimizer", "loss_functions", "batch", "steps", "patterns", "use_graph",
                              "ragged", "text_lengths"]
    assert sig["patterns"].default is None and sig["use_graph"].default is True
    assert issubclass(M.FusedMosiPatternStep, M.FusedMosiStep)
    sig = inspect.signature(M.MosiPatternEngine.__init__).parameters
    assert sig["backward"].default is False  # the forward-only engine is the default


def test_train_step_refuses_all_patterns_without_fused_adam():
    torch.manual_seed(0)
    model = M.build_utt_fusion("mosi", embd_sizes=(8, 12, 8))
    batch = {"audio": torch.zeros(2, 6, 5), "video": torch.zeros(2, 6, 20), "text": torch.zeros(2, 6, 768),
             "label": torch.zeros(2, dtype=torch.int64), "all_patterns": True, "patterns": ["atv", "a"]}
    opt = torch.optim.Adam(model.parameters())
    with pytest.raises(L.TspmError, match="fused step only"):
        model.train_step(batch, opt, None, torch.device("cpu"), None)


# ------------------------------------------------------------------------------------------------
# the loader
# ------------------------------------------------------------------------------------------------
class _Rows:
    """Stands in for the device gather: records the sample rows of every all-pattern batch."""

    def __init__(self, ds, monkeypatch):
        self.rows = []
        self.ds = ds
        monkeypatch.setattr(ds, "_collate_unmasked", self._collate)

    def _collate(self, rows, step, pad_to, flag):
        self.rows.append(np.asarray(rows).copy())
        return {"label": rows, "patterns": list(self.ds.selected_patterns), flag: True}


def test_all_patterns_loader_refusals_counts_and_order(monkeypatch):
    corpus = synthetic_mosi_corpus(20, seed=3, steps=6)
    dev = torch.device("cpu")  # nothing here touches a device
    for split in ("valid", "test"):
        with pytest.raises(L.TspmError, match="all_patterns"):
            MOSI(split=split, corpus=corpus, device=dev).loader(5, all_patterns=True)
        with pytest.raises(L.TspmError, match="all_patterns"):
            next(iter(MOSI(split=split, corpus=corpus, device=dev).device_loader(5, all_patterns=True)))
    with pytest.raises(L.TspmError, match="all_patterns"):
        MOSI(split="train", corpus=corpus, device=dev, target_modality="audio").loader(5, all_patterns=True)
    with pytest.raises(L.TspmError, match="all_patterns"):
        MOSI(split="train", corpus=corpus, device=dev).loader(5, fuse_patterns=True, all_patterns=True)
    with pytest.raises(L.TspmError, match="all_patterns"):  # ... on a split fuse_patterns alone would accept, too
        MOSI(split="valid", corpus=corpus, device=dev).loader(5, fuse_patterns=True, all_patterns=True)
    with pytest.raises(L.TspmError, match="fuse_patterns"):  # still refused on train
        MOSI(split="train", corpus=corpus, device=dev).loader(5, fuse_patterns=True)
    ds = MOSI(split="train", corpus=corpus, device=dev, selected_patterns=["v", "at"])
    plain, allp = ds.loader(5), ds.loader(5, all_patterns=True)
    assert not plain.all_patterns and allp.all_patterns and not allp.fuse_patterns
    assert len(allp) == 4 and len(ds.loader(6, all_patterns=True)) == 4
    assert len(ds.loader(6, drop_last=True, all_patterns=True)) == 3
    rec = _Rows(ds, monkeypatch)
    batches = list(allp)
    assert len(batches) == 4 and np.array_equal(np.concatenate(rec.rows), np.arange(20))  # unshuffled: sample order
    for b in batches:
        assert b["patterns"] == ["v", "at"] and b["all_patterns"] is True
        assert "pattern_name" not in b and "fused_patterns" not in b
    rec.rows.clear()
    shuffled = ds.loader(6, shuffle=True, seed=5, all_patterns=True)
    assert [len(b["label"]) for b in shuffled] == [6, 6, 6, 2]
    first = np.concatenate(rec.rows)
    assert sorted(first.tolist()) == list(range(20)) and first.tolist() != list(range(20))  # each sample once, shuffled
    rec.rows.clear()
    assert [len(b["label"]) for b in shuffled] == [6, 6, 6, 2]  # the next epoch: another order, each sample once
    second = np.concatenate(rec.rows)
    assert sorted(second.tolist()) == list(range(20)) and second.tolist() != first.tolist()
    rec.rows.clear()
    assert [len(b["label"]) for b in ds.loader(6, drop_last=True, all_patterns=True)] == [6, 6, 6]
    assert inspect.signature(MOSI.loader).parameters["all_patterns"].default is False
    assert inspect.signature(MOSI.device_loader).parameters["all_patterns"].default is False


def test_runner_points_an_all_patterns_loader_at_the_pattern_train_step():
    corpus = synthetic_mosi_corpus(10, seed=3, steps=6)
    dev = torch.device("cpu")
    tr = MOSI(split="train", corpus=corpus, device=dev, selected_patterns=["v", "at"])
    va = MOSI(split="valid", corpus=corpus, device=dev, selected_patterns=["v", "at"])
    r = harness.MosiEpochRunner.__new__(harness.MosiEpochRunner)
    r.patterns = None
    allp, plain, fused = tr.loader(5, all_patterns=True), tr.loader(5), va.loader(5, fuse_patterns=True)
    assert r.loader_for(allp, True).step_for == r.train_pattern_step_for and r.patterns == ("v", "at")
    assert r.loader_for(plain, True).step_for == r.train_step_for and r.patterns is None
    assert r.loader_for(fused, False).step_for == r.pattern_eval_step_for and r.patterns == ("v", "at")
    assert r.loader_for(va.loader(5), False).step_for == r.eval_step_for and r.patterns is None


def test_runner_builds_the_pattern_step_through_the_models_cache():
    """``train_pattern_step_for`` with the model replaced by a recorder: the patterns are the argument's, else the
    current loader's, else all seven; the runner's log is attached and a captured graph dropped."""
    calls = []

    class Step:
        log, graph = None, "captured"

    class Model:
        def fused_pattern_step(self, opt, lf, b, t, patterns, ragged=False, text_lengths=False):
            calls.append((b, t, patterns, ragged, text_lengths))
            return Step()
    r = harness.MosiEpochRunner.__new__(harness.MosiEpochRunner)
    r.model, r.optimizer, r.loss_functions, r.log = Model(), None, None, object()
    r.ragged, r.text_lengths, r.patterns = False, True, None
    st = r.train_pattern_step_for(5, (7, 9, 6))
    assert st.log is r.log and st.graph is None
    r.patterns = ("v", "at")
    r.train_pattern_step_for(5, 50, ragged=True)
    r.train_pattern_step_for(5, 50, patterns=["a"], text_lengths=False)
    assert calls == [(5, (7, 9, 6), M.ALL_PATTERNS, False, True), (5, 50, ("v", "at"), True, True),
                     (5, 50, ("a",), False, False)]
