"""Per-sample text lengths in the TextCNN, the parts that need no device: the export under ABI 23 (header, ctypes and the
library's symbol list agree), the refusals of tspm_textcnn_pool_fwd_len before any launch, the cache keys with and without
``text_lengths``, the ``"text"`` key of ``lengths``, the loader's ``"lengths"`` dict, and the float64 restatement
(tests/textcnn_len_ref.py) held to oracle.mosi_ref.textcnn_forward run on each row alone."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import mosi_ref as orc
from textcnn_len_ref import TextLenOracle, clamp_len, n_windows, own_row, pooled_len, textcnn_forward_len
from tspm_amd import _lib as L
from tspm_amd import monomodal as MM
from tspm_amd import mosi as M
from tspm_amd import mosi_data as D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "tspm.h")
NAME = "tspm_textcnn_pool_fwd_len"


# ------------------------------------------------------------------------------------------------
# ABI
# ------------------------------------------------------------------------------------------------
def _params(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return [p.strip() for p in re.search(r"\bint %s\((.*?)\);" % name, src, re.S).group(1).split(",")]


def test_export_header_and_binding_agree_under_abi_23():
    if not os.path.exists(L.LIB_PATH):
        pytest.fail(f"{L.LIB_PATH} is not built")
    lib = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(lib, NAME)
    lib.tspm_abi_version.restype = ctypes.c_int32
    assert lib.tspm_abi_version() == 23 == L.ABI_VERSION
    assert re.search(r"#define TSPM_ABI_VERSION 23\b", open(HEADER).read())
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    assert NAME in {ln.split()[-1] for ln in out.splitlines() if " T tspm_" in ln}
    # the parameters of tspm_textcnn_pool_fwd in their order, plus lengths before the stream
    old, new = _params("tspm_textcnn_pool_fwd"), _params(NAME)
    assert new == old[:-1] + ["const int32_t* lengths", old[-1]]
    res, args = L._SIGS[NAME]
    res0, args0 = L._SIGS["tspm_textcnn_pool_fwd"]
    assert res is res0 and list(args) == list(args0[:-1]) + [ctypes.c_void_p, args0[-1]] and len(args) == len(new)
    assert NAME in L.EXPORTED


def test_refusals_before_any_launch():
    """Every call here is refused (TSPM_ERR_INVALID = 1) before a launch: the pointers are stand-ins."""
    lib = L.load()
    INVALID, P = 1, 4096  # P: an aligned non-NULL stand-in, never dereferenced

    def pool(batch=2, steps=9, nconv=2, heights=(2, 5), channels=4, ld_out=None, conv=P, lengths=P):
        hs = (ctypes.c_int32 * len(heights))(*heights)
        ptrs = (ctypes.c_void_p * 5)(*([conv] * 5))
        return lib.tspm_textcnn_pool_fwd_len(batch, steps, nconv, hs, channels, ptrs, None, None, 1.0, P, P, P,
                                             nconv * channels if ld_out is None else ld_out, lengths, None)

    assert pool(lengths=None) == INVALID  # required
    assert pool(steps=257) == INVALID
    assert pool(heights=(2, 10)) == INVALID  # taller than the sequence
    assert pool(nconv=0) == INVALID and pool(nconv=5, heights=(1, 2, 3, 4, 5)) == INVALID
    assert pool(ld_out=7) == INVALID
    assert pool(conv=None) == INVALID and pool(batch=0) == INVALID


# ------------------------------------------------------------------------------------------------
# keys, keywords, the "text" key
# ------------------------------------------------------------------------------------------------
def test_cache_keys_and_keyword_defaults():
    key = (128, 50, "cuda:0")
    assert M._text_lengths_key(key, False) is key
    assert M._text_lengths_key(M._ragged_key(key, True), True) == key + ("ragged", "text_lengths")
    assert M._text_lengths_key(M._ragged_key(key, False), True) == key + ("text_lengths",)
    assert MM._len_tag(False, False) == () and MM._len_tag(True, False) == ("ragged",)
    assert MM._len_tag(False, True) == ("text_lengths",)
    assert M.RAGGED_MODALITIES == D.LENGTH_MODALITIES == ("audio", "video")
    for fn in (M.UttFusionModel.fused_step, M.UttFusionModel._engine, M.FusedMosiStep.__init__,
               M.FusedMosiEvalStep.__init__, M.MosiEngine.__init__, M.MosiEncoderEngine.__init__, D.MOSI.__init__,
               MM.FusedMosiMonoStep.__init__, MM.FusedMosiMonoEvalStep.__init__, MM.MonomodalEncoder.eval_step_for):
        assert inspect.signature(fn).parameters["text_lengths"].default is False, fn
    assert inspect.signature(M.TextCNN.forward).parameters["lengths"].default is None
    # what a lengths argument asks for: (ragged, text_lengths)
    assert M._split_lengths(None) == (False, False)
    assert M._split_lengths({}) == (True, False) == M._split_lengths({"audio": 0})
    assert M._split_lengths({"text": 0}) == (False, True)
    assert M._split_lengths({"text": 0, "video": 0}) == (True, True)


def test_text_key_is_refused_without_text_lengths():
    M._check_lengths_arg({"audio": 0, "video": 0})  # as before
    M._check_lengths_arg({"audio": 0, "text": 0}, True, True)
    M._check_lengths_arg({"text": 0}, False, True)
    with pytest.raises(L.TspmError):
        M._check_lengths_arg({"text": 0})  # a ragged engine without text_lengths
    with pytest.raises(L.TspmError):
        M._check_lengths_arg({"audio": 0}, False, True)  # a text-only engine has no LSTM length buffers
    with pytest.raises(L.TspmError):
        M._check_lengths_arg({"words": 0}, True, True)


def test_loader_keyword():
    corpus = D.synthetic_mosi_corpus(n=6, steps=9, min_len=2)
    with pytest.raises(L.TspmError):
        D.MOSI(split="train", corpus=corpus, device="cpu", text_lengths=True)  # goes with use_lengths
    off = D.MOSI(split="train", corpus=corpus, device="cpu", use_lengths=True)
    on = D.MOSI(split="train", corpus=corpus, device="cpu", use_lengths=True, text_lengths=True)
    assert tuple(off._length_modalities()) == ("audio", "video") and not off.text_lengths
    assert tuple(on._length_modalities()) == ("audio", "video", "text") and on.text_lengths
    assert tuple(D.MOSI(split="train", corpus=corpus, device="cpu")._length_modalities()) == ()


# ------------------------------------------------------------------------------------------------
# the restatement against the oracle
# ------------------------------------------------------------------------------------------------
STEPS, FEAT, C = 9, 6, 4
LENGTHS = [9, 1, 4, 5, 7, 2, 3, 6]


def _net(seed=0, dropout=0.5):
    torch.manual_seed(seed)
    return orc.OracleTextCNN(FEAT, embd_size=5, out_channels=C, kernel_heights=[3, 4, 5], dropout=dropout).double()


def _x(seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(len(LENGTHS), STEPS, FEAT, generator=g, dtype=torch.float64)
    for b, n in enumerate(LENGTHS):
        x[b, n:] = 0  # the loaders' zero padding
    return x


def test_window_count_and_clamp():
    assert [clamp_len(v, 9) for v in (0, -3, 1000, 4)] == [1, 1, 9, 4]
    assert [n_windows(v, 4, 9) for v in (9, 1, 4, 5, 7, 0, 1000)] == [6, 1, 1, 2, 4, 1, 6]
    row = own_row(torch.ones(9, 2), 2, 5)
    assert row.shape == (5, 2) and row[:2].eq(1).all() and row[2:].eq(0).all()


def test_restatement_is_the_oracle_on_each_row_alone():
    """Rows with L_b >= 5 (every conv has a window inside the row): the oracle on x[b, :L_b] alone, eval and training
    with a keep mask, to 1e-12 in float64."""
    net, x = _net(), _x()
    keep = (torch.rand(len(LENGTHS), 3 * C, generator=torch.Generator().manual_seed(2)) > 0.5).to(torch.uint8)
    for training in (False, True):
        got = textcnn_forward_len(net, x, training, keep, None, LENGTHS)
        for b, n in enumerate(LENGTHS):
            if n < 5:
                continue
            want = orc.textcnn_forward(net, x[b:b + 1, :n], training, keep[b:b + 1])
            assert (got[b] - want[0]).abs().max().item() <= 1e-12, (b, n, training)
    # every length at the padded length: the oracle on the batch
    full = textcnn_forward_len(net, x, False, None, None, None)
    assert (full - orc.textcnn_forward(net, x, False, None)).abs().max().item() <= 1e-12
    # the callable that tests monkeypatch in
    assert torch.equal(TextLenOracle(LENGTHS)(net, x, False, None), textcnn_forward_len(net, x, False, None, None, LENGTHS))


def test_short_rows_are_the_oracle_on_the_zero_padded_row():
    """Rows shorter than a kernel height: conv i's pooled features are the oracle's on the row explicitly zero-padded to
    max(L_b, kh_i) — read from the oracle through a net whose three convs are all conv i (so it accepts that length)."""
    net, x = _net(3), _x(4)
    got = pooled_len(net, x, LENGTHS)
    for i, conv in enumerate((net.conv1, net.conv2, net.conv3)):
        kh = conv.weight.shape[2]
        same = orc.OracleTextCNN(FEAT, embd_size=5, out_channels=C, kernel_heights=[kh] * 3).double()
        for c in (same.conv1, same.conv2, same.conv3):
            c.load_state_dict(conv.state_dict())
        for b, n in enumerate(LENGTHS):
            row = torch.zeros(1, max(n, kh), FEAT, dtype=torch.float64)
            row[0, :n] = x[b, :n]
            tr = orc.MosiTrace()
            orc.textcnn_forward(same, row, False, None, tr)
            pre, idx = tr.pre["text.pool0"], tr.idx["text.pool0"]  # [1, C, n_i(b)], [1, C]
            assert pre.shape[2] == n_windows(n, kh, STEPS)
            want = pre.relu().gather(2, idx.unsqueeze(2))[0, :, 0]
            assert (got[b, i * C:(i + 1) * C] - want).abs().max().item() <= 1e-12, (i, b, n)


def test_trace_records_and_forces_the_time_index():
    net, x = _net(5), _x(6)
    tr = orc.MosiTrace()
    free = textcnn_forward_len(net, x, False, None, tr, LENGTHS)
    assert (free - textcnn_forward_len(net, x, False, None, None, LENGTHS)).abs().max().item() <= 1e-12
    for i, kh in enumerate((3, 4, 5)):
        idx, pre = tr.idx[f"text.pool{i}"], tr.pre[f"text.pool{i}"]
        assert pre.shape == (len(LENGTHS), C, STEPS - kh + 1)
        for b, n in enumerate(LENGTHS):
            nw = n_windows(n, kh, STEPS)
            assert int(idx[b].max()) < nw and torch.isinf(pre[b, :, nw:]).all() and torch.isfinite(pre[b, :, :nw]).all()
    # forcing the recorded decisions reproduces the free forward, and gradients flow
    force = {k: v for k, v in tr.idx.items()}
    force.update({f"text.relu{i}": tr.pre[f"text.pool{i}"].relu().gather(2, tr.idx[f"text.pool{i}"].unsqueeze(2))[:, :, 0] > 0
                  for i in range(3)})
    force["text.embd"] = tr.pre["text.embd"] > 0
    xg = x.clone().requires_grad_(True)
    forced = textcnn_forward_len(net, xg, False, None, orc.MosiTrace(force), LENGTHS)
    assert (forced - free).abs().max().item() <= 1e-12
    forced.sum().backward()
    for b, n in enumerate(LENGTHS):  # no gradient reaches a step that no window of the row covers
        assert not bool(xg.grad[b, max(n, 5):].any())
