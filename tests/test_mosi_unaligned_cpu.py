"""Unaligned MOSI / MOSEI — per-modality sequence lengths and the 16-bit LSTM time index — the checks that need no
GPU: tspm_lstm_fwd_t16 / tspm_lstm_bwd_t16 are declared on both sides of the ABI and validate every descriptor before
any launch (an accepted call answers TSPM_ERR_LAUNCH = 2 on a machine without a GPU, as in test_lstm_widths_cpu.py),
``mosi_data.DeviceMosiCorpus.steps_per_modality`` pads each modality as pad_sequence does, and ``mosi.norm_steps`` is the
one normalisation of ``steps``."""
import os
import re

import numpy as np
import pytest
import torch

import tspm_amd
from tspm_amd import _lib as L
from tspm_amd import mosi as M
from tspm_amd import mosi_data as D

INVALID, LAUNCH = 1, 2
P = 4096  # a 16-byte aligned, non-NULL stand-in: never dereferenced, every call returns before or at the launch
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tspm.h")


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
    return L.load().tspm_lstm_fwd_t16(count, d, None)


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
    return L.load().tspm_lstm_bwd_t16(count, d, None)


def _no_gpu():
    return not torch.cuda.is_available()


def test_both_sides_declare_the_t16_entry_points():
    assert "tspm_lstm_fwd_t16" in L.EXPORTED and "tspm_lstm_bwd_t16" in L.EXPORTED
    lib = L.load()
    assert lib.tspm_lstm_fwd_t16.argtypes[1]._type_ is L.LstmFwdDesc
    assert lib.tspm_lstm_bwd_t16.argtypes[1]._type_ is L.LstmBwdDesc
    assert lib.tspm_abi_version() == 23 == L.ABI_VERSION  # added under ABI 23: the version number stays
    with open(HEADER) as f:
        h = f.read()
    assert re.search(r"int tspm_lstm_fwd_t16\(int32_t count, const tspm_lstm_fwd_desc\* descs, tspm_stream_t stream\);", h)
    assert re.search(r"int tspm_lstm_bwd_t16\(int32_t count, const tspm_lstm_bwd_desc\* descs, tspm_stream_t stream\);", h)
    assert "uint16_t [batch][hidden]" in h  # the cast of the argmax field is documented
    assert "#define TSPM_ABI_VERSION 23" in h


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["fwd", "bwd"])
def test_t16_entry_points_refuse_before_launch(call):
    ld = "ld_out" if call is _fwd else "ld_dh"
    assert call(steps=0, argmax=P) == INVALID and call(steps=65536, argmax=P) == INVALID  # the 16-bit index range
    assert call(steps=0) == INVALID
    for h in (2, 130, 132):
        assert call(hidden=h, **{ld: 256}) == INVALID, h
    assert call(count=0) == INVALID and call(count=3) == INVALID
    assert call(batch=0) == INVALID
    assert call(argmax=P + 1) == INVALID  # a uint16_t buffer is 2-byte aligned
    # the second descriptor is validated when the first is fine, before anything launches
    assert call(count=2, hidden=36, second=dict(hidden=130)) == INVALID
    assert call(count=2, hidden=64, steps=300, argmax=P, second=dict(steps=65536)) == INVALID
    assert call(count=2, hidden=128, second=dict(batch=0)) == INVALID


def test_t16_entry_points_refuse_null_pointers():
    for n in ("xg", "w_hh", "gates", "cs", "hs", "h_out"):
        assert _fwd(hidden=36, **{n: None}) == INVALID, n
    for n in ("w_hh", "gates", "cs", "dh", "dgates"):
        assert _bwd(hidden=36, **{n: None}) == INVALID, n
    lib = L.load()
    assert lib.tspm_lstm_fwd_t16(1, None, None) == INVALID and lib.tspm_lstm_bwd_t16(1, None, None) == INVALID


@pytest.mark.skipif(not _no_gpu(), reason="an accepted call would launch on the stand-in pointers")
@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["fwd", "bwd"])
def test_t16_entry_points_accept_the_range(call):
    for h in (4, 36, 64, 128):
        assert call(hidden=h, steps=1, argmax=P) == LAUNCH, h
        assert call(hidden=h, steps=257, argmax=P) == LAUNCH, h
        assert call(hidden=h, steps=65535, argmax=P) == LAUNCH, h
        assert call(hidden=h, steps=65536) == LAUNCH, h  # without an index the steps are unlimited, as in _w
    assert call(count=2, hidden=36, steps=5, argmax=P, second=dict(hidden=128, batch=5, steps=300)) == LAUNCH
    # the 8-bit entry points keep their limit
    lib = L.load()
    d = (L.LstmFwdDesc * 1)(L.LstmFwdDesc(batch=2, steps=257, hidden=36, ld_out=36, xg=P, w_hh=P, b_hh=P, gates=P, cs=P,
                                          hs=P, h_out=P, argmax=P))
    assert lib.tspm_lstm_fwd_w(1, d, None) == INVALID


def test_lstm_steps_supported_and_the_wide_index_rule():
    assert L.lstm_steps_supported(1, True) and L.lstm_steps_supported(256, True) and L.lstm_steps_supported(65535, True)
    assert not L.lstm_steps_supported(0, True) and not L.lstm_steps_supported(65536, True)
    assert not L.lstm_steps_supported(0, False) and L.lstm_steps_supported(65536, False)
    assert not L.lstm_wide_index((("maxpool", 256), ("maxpool", 5)))
    assert L.lstm_wide_index((("maxpool", 257), ("maxpool", 5))) and L.lstm_wide_index((("last", 5), ("maxpool", 300)))
    assert not L.lstm_wide_index((("last", 500), ("last", 375)))  # no index, no wide index
    # the library agrees with lstm_steps_supported at the edges (a supported count only where nothing can launch)
    for steps in (0, 65536, 70000):
        assert _fwd(steps=steps, argmax=P) == INVALID and _bwd(steps=steps, argmax=P) == INVALID


def test_index_buffers_and_their_host_reads():
    enc = M.LSTMEncoder(5, 36, "maxpool")
    assert M._lstm_alloc(enc, 3, 256, "cpu")["arg"].dtype == torch.uint8
    wide = M._lstm_alloc(enc, 3, 300, "cpu", wide=True)["arg"]
    assert wide.dtype == torch.int16 and tuple(wide.shape) == (3, 36)
    assert M._lstm_alloc(enc, 3, 5, "cpu", wide=True)["arg"].dtype == torch.int16  # the short encoder of a wide launch
    assert M._lstm_alloc(M.LSTMEncoder(5, 36, "last"), 3, 300, "cpu", wide=True)["arg"] is None
    with pytest.raises(L.TspmError, match="16-bit past 256"):
        M._lstm_alloc(enc, 3, 300, "cpu")  # an 8-bit buffer cannot hold the index
    with pytest.raises(L.TspmError, match="65535"):
        M._lstm_alloc(enc, 1, 65536, "cpu", wide=True)
    # the int16 storage holds the unsigned pattern: every host read widens it without sign extension
    raw = torch.tensor([0, 255, 256, 32767, 32768, 65534], dtype=torch.int64)
    stored = torch.from_numpy(raw.numpy().astype(np.uint16).view(np.int16))
    assert stored.dtype == torch.int16 and int(stored[4]) == -32768
    assert torch.equal(L.index_to_int64(stored), raw)
    assert torch.equal(L.index_to_int64(torch.tensor([0, 255], dtype=torch.uint8)), torch.tensor([0, 255]))


def _ragged():
    """The ragged corpus of test_mosi_cpu.py: audio / video 3, 7, 5; text 3, 7, 6."""
    g = np.random.default_rng(0)
    lens = [3, 7, 5]
    seqs = {"audio": [g.standard_normal((l, 5), dtype=np.float32) for l in lens],
            "video": [g.standard_normal((l, 20), dtype=np.float32) for l in lens],
            "text": [g.standard_normal((l, 8), dtype=np.float32) for l in [3, 7, 6]]}
    c = D.MosiCorpus(seqs, np.array([0, 2, 1]))

    class _Dc(D.DeviceMosiCorpus):  # host-side length logic only (no upload)
        def __init__(self, corpus):
            self.host_lengths = corpus.lengths
    return _Dc(c)


def test_steps_per_modality():
    dc = _ragged()
    assert dc.steps_per_modality(np.array([2])) == (5, 5, 6)
    assert dc.steps_per_modality(np.array([0, 1])) == (7, 7, 7)
    assert dc.steps_per_modality(np.array([2]), pad_to=6) == (6, 6, 6)
    assert dc.steps_per_modality(np.array([2]), pad_to={"audio": 9, "text": 2}) == (9, 5, 6)  # per-modality minimum
    assert dc.steps_per_modality(np.array([2]), pad_to=(7, 8, 9)) == (7, 8, 9)
    assert dc.steps_per_modality(np.array([2]), modalities=("text", "audio")) == (6, 5)
    assert dc.steps_per_modality(np.array([], dtype=np.int64), pad_to=(7, 8, 9)) == (7, 8, 9)
    with pytest.raises(tspm_amd._lib.TspmError):
        dc.steps_for(np.array([2]))  # unchanged: the common-length query still refuses the unaligned batch
    assert dc.steps_for(np.array([2]), pad_to=50) == 50 and dc.steps_for(np.array([0, 1])) == 7


def test_batch_steps_keeps_the_common_length_where_steps_for_accepts():
    dc = _ragged()
    assert dc.batch_steps(np.array([0, 1])) == 7 and dc.batch_steps(np.array([0])) == 3
    assert dc.batch_steps(np.array([2]), pad_to=50) == 50  # today's int
    assert dc.batch_steps(np.array([2])) == (5, 5, 6)  # refused today: per modality
    assert dc.batch_steps(np.array([0, 2])) == (5, 5, 6)
    assert dc.batch_steps(np.array([2]), pad_to=(7, 7, 7)) == 7  # a per-modality pad_to whose entries agree
    assert dc.batch_steps(np.array([0, 1, 2]), pad_to=(12, 12, 8)) == (12, 12, 8)
    assert D.pad_of({"audio": 4}, "video") == 0 and D.pad_of((1, 2, 3), "text") == 3 and D.pad_of(5, "text") == 5
    assert D.steps_of((4, 5, 6), "video") == 5 and D.steps_of(9, "video") == 9


def test_norm_steps():
    assert M.norm_steps((50, 50, 50)) == 50 and M.norm_steps([50, 50, 50]) == 50 and M.norm_steps(50) == 50
    assert M.norm_steps((375, 500, 50)) == (375, 500, 50) and M.norm_steps(np.array([7, 9, 6])) == (7, 9, 6)
    assert M.steps_triple(8) == (8, 8, 8) and M.steps_triple((7, 9, 6)) == (7, 9, 6)
    assert isinstance(M.norm_steps(np.int64(8)), int) and all(isinstance(t, int) for t in M.norm_steps(np.array([7, 9, 6])))
    for bad in ((7, 0, 6), (-1, 5, 5), (5, 5, 0), 0):
        with pytest.raises(L.TspmError, match=">= 1"):
            M.norm_steps(bad)
    with pytest.raises(L.TspmError, match="triple"):
        M.norm_steps((7, 9))
    # the TextCNN keeps its 8-bit index: the error names the text length
    with pytest.raises(L.TspmError, match=r"steps <= 255.*text length is 256"):
        M.norm_steps((500, 375, 256))
    with pytest.raises(L.TspmError, match=r"steps <= 255.*text length is 300"):
        M.norm_steps(300)
    assert M.norm_steps((500, 375, 255)) == (500, 375, 255)


def test_step_caches_key_on_the_normalised_steps():
    torch.manual_seed(0)
    m = M.build_utt_fusion("mosi")
    with pytest.raises(L.TspmError, match="MI355X only"):  # the triple form takes the same path: no CPU fallback
        m._engine(2, (8, 8, 8), "cpu")
    with pytest.raises(L.TspmError, match="text length is 256"):
        m._engine(2, (8, 8, 256), "cuda")
    with pytest.raises(L.TspmError, match=">= 1"):
        m.fused_step(None, None, 2, (8, 0, 8))
