"""Per-sample sequence lengths, the parts that need no device: the two exports and their descriptors (header, ctypes
and a compiled sizeof / offsetof probe agree), the ABI version, the cache keys without lengths, the loader's trimming,
and the CPU checks of the length-aware restatement (test_gpu_lstm_len.py holds them; they run here with the non-GPU
suite because they carry no ``gpu`` mark)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tspm_amd import _lib as L
from tspm_amd import mosi as M
from tspm_amd import mosi_data as D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "tspm.h")
FWD_FIELDS = ["batch", "steps", "hidden", "ld_out", "xg", "w_hh", "b_hh", "gates", "cs", "hs", "h_out", "argmax",
              "lengths", "index_bits", "reserved_"]
BWD_FIELDS = ["batch", "steps", "hidden", "ld_dh", "w_hh", "gates", "cs", "dh", "dgates", "argmax", "lengths",
              "index_bits", "reserved_"]


def _header_fields(name):
    src = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            out += [first.split()[-1].lstrip("*")] + [r.strip().lstrip("*") for r in rest]
    return out


def test_library_exports_both_entry_points_under_abi_23():
    if not os.path.exists(L.LIB_PATH):
        pytest.fail(f"{L.LIB_PATH} is not built")
    lib = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(lib, "tspm_lstm_fwd_len") and hasattr(lib, "tspm_lstm_bwd_len")
    lib.tspm_abi_version.restype = ctypes.c_int32
    assert lib.tspm_abi_version() == 23 == L.ABI_VERSION
    assert "tspm_lstm_fwd_len" in L.EXPORTED and "tspm_lstm_bwd_len" in L.EXPORTED
    assert re.search(r"#define TSPM_ABI_VERSION 23\b", open(HEADER).read())


def test_header_declares_the_descriptors_in_the_bound_order():
    assert _header_fields("tspm_lstm_fwd_len_desc") == FWD_FIELDS == [f[0] for f in L.LstmFwdLenDesc._fields_]
    assert _header_fields("tspm_lstm_bwd_len_desc") == BWD_FIELDS == [f[0] for f in L.LstmBwdLenDesc._fields_]
    # the existing descriptors are a prefix, untouched
    assert [f[0] for f in L.LstmFwdDesc._fields_] == FWD_FIELDS[:12] == _header_fields("tspm_lstm_fwd_desc")
    assert [f[0] for f in L.LstmBwdDesc._fields_] == BWD_FIELDS[:10] == _header_fields("tspm_lstm_bwd_desc")
    src = open(HEADER).read()
    for fn, d in (("fwd", "tspm_lstm_fwd_len_desc"), ("bwd", "tspm_lstm_bwd_len_desc")):
        assert re.search(r"int tspm_lstm_%s_len\(int32_t count, const %s\* descs, tspm_stream_t stream\);" % (fn, d), src)


def test_ctypes_layout_equals_the_compiled_header(tmp_path):
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")  # what builds the library
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or \
        (rocm_clang if os.path.exists(rocm_clang) else None)
    if cc is None:
        pytest.fail("no C compiler to probe the header's layout")
    probe = tmp_path / "probe.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "tspm.h"', "int main(void) {"]
    for name, fields in (("tspm_lstm_fwd_len_desc", FWD_FIELDS), ("tspm_lstm_bwd_len_desc", BWD_FIELDS)):
        lines.append(f'  printf("%zu", sizeof({name}));')
        lines += [f'  printf(" %zu", offsetof({name}, {f}));' for f in fields]
        lines.append('  printf("\\n");')
    probe.write_text("\n".join(lines + ["  return 0;", "}"]))
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), str(probe), "-o", str(exe)], check=True)
    rows = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    for row, st in zip(rows, (L.LstmFwdLenDesc, L.LstmBwdLenDesc)):
        got = [int(v) for v in row.split()]
        assert got[0] == ctypes.sizeof(st)
        assert got[1:] == [getattr(st, f[0]).offset for f in st._fields_]


def test_keys_without_lengths_are_the_existing_keys():
    assert M.norm_steps(50) == 50 == M.norm_steps((50, 50, 50)) and M.norm_steps((375, 500, 50)) == (375, 500, 50)
    key = (128, 50, "cuda:0")
    assert M._ragged_key(key, False) is key
    assert M._ragged_key(key, True) == key + ("ragged",)
    assert M.RAGGED_MODALITIES == D.LENGTH_MODALITIES == ("audio", "video")
    import inspect
    for fn, arg in ((M.UttFusionModel.fused_step, "ragged"), (M.UttFusionModel._engine, "ragged"),
                    (M.FusedMosiStep.__init__, "ragged"), (M.FusedMosiEvalStep.__init__, "ragged"),
                    (M.MosiEngine.__init__, "ragged"), (M.MosiEncoderEngine.__init__, "ragged"),
                    (D.MOSI.__init__, "use_lengths")):
        assert inspect.signature(fn).parameters[arg].default is False, fn
    for fn in (M.LSTMEncoder.forward, M.UttFusionModel.forward, M.FusedMosiStep.step, D.DeviceMosiCorpus.gather):
        name = "lengths_out" if fn is D.DeviceMosiCorpus.gather else "lengths"
        assert inspect.signature(fn).parameters[name].default is None, fn


def test_use_lengths_trims_the_split(tmp_path):
    g = np.random.default_rng(0)
    n, T = 5, 7
    split = {"audio": g.standard_normal((n, T, 5)).astype(np.float32),
             "vision": g.standard_normal((n, T, 20)).astype(np.float32),
             "text": g.standard_normal((n, T, 768)).astype(np.float32),
             "classification_labels": g.integers(0, 3, n).astype(np.int64),
             "audio_lengths": np.array([7, 1, 3, 5, 2]), "vision_lengths": np.array([2, 7, 4, 1, 6])}
    path = tmp_path / "unaligned.npz"
    np.savez(path, **{f"train/{k}": v for k, v in split.items()})
    on = D.MOSI(path, split="train", device="cpu", use_lengths=True).corpus
    off = D.MOSI(path, split="train", device="cpu").corpus
    assert np.array_equal(on.lengths["audio"], split["audio_lengths"])
    assert np.array_equal(on.lengths["video"], split["vision_lengths"])
    assert np.array_equal(on.lengths["text"], np.full(n, T))
    assert np.array_equal(on.data["audio"][:7], split["audio"][0]) and np.array_equal(on.data["audio"][7], split["audio"][1, 0])
    assert on.data["audio"].shape[0] == split["audio_lengths"].sum()
    assert np.array_equal(off.lengths["audio"], np.full(n, T))  # the default keeps the dense arrays, as before
    assert np.array_equal(off.true_lengths["video"], split["vision_lengths"])
    assert np.array_equal(on.true_lengths["audio"], split["audio_lengths"])


def test_the_restatement_checks_run_with_the_cpu_suite():
    """The CPU checks of the length-aware restatement live beside it in test_gpu_lstm_len.py without a ``gpu`` mark."""
    import test_gpu_lstm_len as t
    for fn in (t.test_restatement_is_pack_padded_sequence, t.test_fp32_restatement_stays_within_the_flip_cap):
        marks = [m.name for m in getattr(fn, "pytestmark", [])]
        assert "gpu" not in marks
    assert "gpu" in [m.name for m in t.test_lstm_len_vs_fp64.pytestmark]
    t.test_restatement_is_pack_padded_sequence()
