"""The attention embedding of the LSTM encoders, the parts that need no device: the constructor (keyword, refusals,
``state_dict`` keys / shapes / order and RNG order against a plain-torch restatement built in the same order), the
reference helper tests/attn_ref.py against an independent composition in float64, the three new descriptors (header,
ctypes and a compiled sizeof / offsetof probe agree), every refusal of the three entry points (they return before any
launch, so they run without a device), and the cache keys of the default models."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch
import torch.nn as nn
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

import attn_ref as R
from test_mosi_lengths_cpu import HEADER, REPO, _header_fields
from tspm_amd import _lib as L
from tspm_amd import mosi as M

INVALID = 1
SEQ_FIELDS = ["batch", "steps", "hidden", "ld_dh", "w_hh", "gates", "cs", "dh", "dgates", "dseq", "wt", "lengths"]
FWD_FIELDS = ["batch", "steps", "hidden", "ld_out", "norm", "reserved_", "r", "p", "u", "alpha", "h_out", "lengths"]
BWD_FIELDS = ["batch", "steps", "hidden", "ld_g", "norm", "reserved_", "g", "alpha", "z", "r", "u", "dp", "du", "dc", "rows",
              "lengths"]
STRUCTS = (("tspm_lstm_bwd_seq_desc", SEQ_FIELDS, L.LstmBwdSeqDesc), ("tspm_attn_pool_fwd_desc", FWD_FIELDS, L.AttnPoolFwdDesc),
           ("tspm_attn_pool_bwd_desc", BWD_FIELDS, L.AttnPoolBwdDesc))


# ------------------------------------------------------------------------------------------------
# the constructor
# ------------------------------------------------------------------------------------------------
def test_attention_needs_an_explicit_norm():
    with pytest.raises(NotImplementedError, match="attention_norm.*'time'.*'unit'"):
        M.LSTMEncoder(5, 64, embd_method="attention")
    for norm in ("time", "unit"):
        enc = M.LSTMEncoder(5, 64, embd_method="attention", attention_norm=norm)
        assert enc.embd_method == "attention" and enc.attention_norm == norm
        assert isinstance(enc.softmax, nn.Softmax) and not list(enc.softmax.parameters())
    with pytest.raises(L.TspmError, match="attention_norm"):
        M.LSTMEncoder(5, 64, embd_method="last", attention_norm="time")
    with pytest.raises(L.TspmError, match="attention_norm"):
        M.LSTMEncoder(5, 64, embd_method="maxpool", attention_norm="unit")
    with pytest.raises(L.TspmError, match="attention_norm"):
        M.LSTMEncoder(5, 64, embd_method="attention", attention_norm="softmax")
    assert M.LSTMEncoder(5, 64).attention_norm is None and M.LSTMEncoder(5, 64, "maxpool").embd_method == "maxpool"


@pytest.mark.parametrize("norm", ["time", "unit"])
def test_state_dict_and_rng_order_are_the_restatements(norm):
    """Keys, shapes and order of the ``state_dict``; same-seed values of ``rnn``, ``attention_layer`` and of a module built
    afterwards; the global RNG state after construction — all equal to the plain-torch restatement built in the same
    order.  The vector comes from a private generator: two builds agree and the global RNG is not touched by it."""
    torch.manual_seed(11)
    ours = M.LSTMEncoder(20, 36, embd_method="attention", attention_norm=norm)
    after_ours = nn.Linear(7, 3)
    state_ours = torch.get_rng_state()
    torch.manual_seed(11)
    ref = R.AttnEncoderRef(20, 36)
    after_ref = nn.Linear(7, 3)
    state_ref = torch.get_rng_state()
    sd, sr = ours.state_dict(), ref.state_dict()
    assert list(sd) == list(sr) and [tuple(v.shape) for v in sd.values()] == [tuple(v.shape) for v in sr.values()]
    assert sorted(sd) == sorted(["attention_vector_weight", "rnn.weight_ih_l0", "rnn.weight_hh_l0", "rnn.bias_ih_l0",
                                 "rnn.bias_hh_l0", "attention_layer.0.weight", "attention_layer.0.bias"])
    assert tuple(sd["attention_vector_weight"].shape) == (36, 1)
    assert [n for n, _ in ours.named_parameters()] == [n for n, _ in ref.named_parameters()]
    for k in sd:
        if k != "attention_vector_weight":
            assert torch.equal(sd[k], sr[k]), k
    assert torch.equal(after_ours.weight, after_ref.weight) and torch.equal(after_ours.bias, after_ref.bias)
    assert torch.equal(state_ours, state_ref)
    v = sd["attention_vector_weight"]
    assert bool((v.abs() <= 1 / 6).all()) and v.std().item() > 0.02  # U(-1/sqrt(36), 1/sqrt(36))
    torch.manual_seed(12)
    again = M.LSTMEncoder(20, 36, embd_method="attention", attention_norm=norm)
    assert torch.equal(again.attention_vector_weight, ours.attention_vector_weight)
    ref.load_state_dict(sd)  # the checkpoint of one loads into the other


def test_build_utt_fusion_keywords():
    import inspect
    sig = inspect.signature(M.build_utt_fusion).parameters
    assert sig["embd_method"].default is None and sig["attention_norm"].default is None
    torch.manual_seed(0)
    default = M.build_utt_fusion("mosi")
    assert default.netA.embd_method == "last" and default.netA.attention_norm is None
    assert "netA.attention_vector_weight" not in default.state_dict()
    torch.manual_seed(0)
    m = M.build_utt_fusion("mosei", embd_method="attention", attention_norm="time")
    assert m.netA.embd_method == m.netV.embd_method == "attention" and m.netV.attention_norm == "time"
    assert M._frozen_state(m) == ((), None)
    m.netA.requires_grad_(False)  # the three attention parameters count as the module's flags
    assert M._frozen_state(m) == (("audio",), None)
    m.netA.attention_vector_weight.requires_grad_(True)
    assert "mixed requires_grad" in M._frozen_state(m)[1]
    with pytest.raises(NotImplementedError):
        M.build_utt_fusion("mosi", embd_method="attention")


def test_keys_of_models_without_attention_are_the_existing_keys():
    key = (128, 50, "cuda:0")
    assert M._frozen_key(M._text_lengths_key(M._ragged_key(key, False), False), ()) is key
    import inspect
    assert list(inspect.signature(M.UttFusionModel._engine).parameters) == ["self", "b", "t", "device", "ragged",
                                                                            "text_lengths"]
    assert list(inspect.signature(M.UttFusionModel.fused_step).parameters) == ["self", "optimizer", "loss_functions",
                                                                               "batch", "steps", "ragged", "text_lengths"]


# ------------------------------------------------------------------------------------------------
# the helper
# ------------------------------------------------------------------------------------------------
def _case(H=12, F=7, B=5, T=9, seed=0):
    torch.manual_seed(seed)
    enc = R.AttnEncoderRef(F, H).double()
    with torch.no_grad():
        enc.attention_vector_weight.uniform_(-1, 1)
    return enc, torch.randn(B, T, F, dtype=torch.float64)


def test_helper_equals_an_independent_composition_in_float64():
    """nn.LSTM over pack_padded_sequence, nn.Linear, tanh, softmax(dim=1) over the valid steps (scores past a length at
    -inf): embedding and every parameter gradient to 1e-12."""
    lens = (9, 1, 4, 4, 7)
    enc, x = _case()
    g = torch.randn(5, 12, dtype=torch.float64)
    (g * R.encode(enc, x, lens, "time")).sum().backward()
    want = {n: p.grad.clone() for n, p in enc.named_parameters()}
    e_helper = R.encode(enc, x, lens, "time").detach()
    enc.zero_grad()
    out, _ = enc.rnn(pack_padded_sequence(x, torch.tensor(lens), batch_first=True, enforce_sorted=False))
    r, _ = pad_packed_sequence(out, batch_first=True, total_length=9)          # [B, T, H]
    s = (enc.attention_layer(r) @ enc.attention_vector_weight).squeeze(2)       # [B, T]
    valid = torch.arange(9).view(1, 9) < torch.tensor(lens).view(5, 1)
    alpha = torch.softmax(s.masked_fill(~valid, float("-inf")), dim=1)
    e = (alpha.unsqueeze(2) * r).sum(1)
    assert (e - e_helper).abs().max().item() <= 1e-12
    (g * e).sum().backward()
    for n, p in enc.named_parameters():
        assert (p.grad - want[n]).abs().max().item() <= 1e-12, n
    # without lengths: the padded length
    assert (R.encode(enc, x, None, "time") - R.encode(enc, x, (9,) * 5, "time")).abs().max().item() == 0


def test_unit_is_the_literal_softmax_over_the_size_1_axis():
    """nn.Softmax(dim=-1) on [B, T, 1] scores: every weight 1, the embedding the plain time-sum, and exact zero
    gradients (not None) for the three attention parameters."""
    enc, x = _case(seed=1)
    r, _ = enc.rnn(x)
    scores = enc.attention_layer(r) @ enc.attention_vector_weight               # [B, T, 1]
    alpha = enc.softmax(scores)
    assert alpha.shape == (5, 9, 1) and bool((alpha == 1).all())
    e = (alpha * r).sum(1)
    assert (e - R.encode(enc, x, None, "unit")).abs().max().item() <= 1e-12
    e.square().sum().backward()
    for p in (enc.attention_vector_weight, enc.attention_layer[0].weight, enc.attention_layer[0].bias):
        assert p.grad is not None and bool((p.grad == 0).all())
    assert enc.rnn.weight_hh_l0.grad.abs().max().item() > 0
    lens = (9, 1, 4, 4, 7)
    want = torch.stack([r[b, :lens[b]].sum(0) for b in range(5)])
    assert (R.encode(enc, x, lens, "unit") - want).abs().max().item() <= 1e-12


def test_pool_alpha_and_z_conventions():
    enc, x = _case(seed=2)
    lens = (9, 1, 4, 4, 7)
    r = R.lstm_outputs(enc.rnn, x, lens).transpose(0, 1)
    lin = enc.attention_layer[0]
    for norm in R.NORMS:
        e, a, z = R.attn_pool(r, lin.weight, lin.bias, enc.attention_vector_weight, lens, norm)
        assert e.shape == (5, 12) and a.shape == (9, 5) and z.shape == (9, 5, 12)
        for b, Lb in enumerate(lens):
            assert bool((a[Lb:, b] == 0).all()) and bool((z[Lb:, b] == 0).all())
            assert abs(a[:Lb, b].sum().item() - (1.0 if norm == "time" else Lb)) <= 1e-12


# ------------------------------------------------------------------------------------------------
# the descriptors and the entry points' refusals
# ------------------------------------------------------------------------------------------------
def test_header_declares_the_descriptors_in_the_bound_order():
    src = open(HEADER).read()
    for name, fields, st in STRUCTS:
        assert _header_fields(name) == fields == [f[0] for f in st._fields_], name
    for fn, d in (("tspm_lstm_bwd_seq", "tspm_lstm_bwd_seq_desc"), ("tspm_attn_pool_fwd", "tspm_attn_pool_fwd_desc"),
                  ("tspm_attn_pool_bwd", "tspm_attn_pool_bwd_desc")):
        assert "int %s(int32_t count, const %s* descs, tspm_stream_t stream);" % (fn, d) in src
        assert fn in L.EXPORTED and hasattr(ctypes.CDLL(L.LIB_PATH), fn)
    assert "#define TSPM_ABI_VERSION 23\n" in src and L.ABI_VERSION == 23
    # the existing length descriptors are untouched
    assert [f[0] for f in L.LstmBwdLenDesc._fields_][:9] == SEQ_FIELDS[:9]


def test_ctypes_layout_equals_the_compiled_header(tmp_path):
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or \
        (rocm_clang if os.path.exists(rocm_clang) else None)
    if cc is None:
        pytest.fail("no C compiler to probe the header's layout")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "tspm.h"', "int main(void) {"]
    for name, fields, _ in STRUCTS:
        lines.append(f'  printf("%zu", sizeof({name}));')
        lines += [f'  printf(" %zu", offsetof({name}, {f}));' for f in fields]
        lines.append('  printf("\\n");')
    probe = tmp_path / "probe.c"
    probe.write_text("\n".join(lines + ["  return 0;", "}"]))
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), str(probe), "-o", str(exe)], check=True)
    rows = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    for row, (_, _, st) in zip(rows, STRUCTS):
        got = [int(v) for v in row.split()]
        assert got[0] == ctypes.sizeof(st)
        assert got[1:] == [getattr(st, f[0]).offset for f in st._fields_]


FAKE = 0x10000  # a 16-byte aligned non-NULL value: a refused call never dereferences (or launches with) it


def _seq_desc(**kw):
    d = L.LstmBwdSeqDesc(batch=2, steps=9, hidden=36, ld_dh=36)
    for n in ("w_hh", "gates", "cs", "dh", "dgates", "dseq", "wt", "lengths"):
        setattr(d, n, FAKE)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _fwd_desc(**kw):
    d = L.AttnPoolFwdDesc(batch=2, steps=9, hidden=36, ld_out=36, norm=0)
    for n in ("r", "p", "u", "alpha", "h_out", "lengths"):
        setattr(d, n, FAKE)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _bwd_desc(**kw):
    d = L.AttnPoolBwdDesc(batch=2, steps=9, hidden=36, ld_g=36, norm=0)
    for n in ("g", "alpha", "z", "r", "u", "dp", "du", "dc", "rows", "lengths"):
        setattr(d, n, FAKE)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


REFUSALS = [
    ("tspm_lstm_bwd_seq", L.LstmBwdSeqDesc, _seq_desc, [dict(lengths=None), dict(hidden=130), dict(hidden=6),
                                                       dict(dh=None, dseq=None), dict(dgates=None), dict(steps=0)]),
    ("tspm_attn_pool_fwd", L.AttnPoolFwdDesc, _fwd_desc, [dict(lengths=None), dict(hidden=130), dict(hidden=6), dict(norm=2),
                                                         dict(norm=-1), dict(p=None), dict(ld_out=35), dict(r=FAKE + 4)]),
    ("tspm_attn_pool_bwd", L.AttnPoolBwdDesc, _bwd_desc, [dict(lengths=None), dict(hidden=130), dict(hidden=6), dict(norm=1),
                                                         dict(norm=2), dict(rows=None), dict(dc=None), dict(ld_g=35)]),
]


@pytest.mark.parametrize("fn,st,make,bad", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_every_refusal_returns_before_any_launch(fn, st, make, bad):
    """TSPM_ERR_INVALID with pointers that no launch could survive and no device in the process: nothing was launched.  A
    bad descriptor is refused alone and after a good one (every descriptor is validated before the first launch)."""
    entry = getattr(L.lib(), fn)
    for kw in bad:
        assert entry(1, (st * 1)(make(**kw)), None) == INVALID, (fn, kw)
        assert entry(2, (st * 2)(make(), make(**kw)), None) == INVALID, (fn, kw, "second")
    for count in (0, 3, -1):
        assert entry(count, (st * 3)(make(), make(), make()), None) == INVALID, (fn, count)
    assert entry(1, None, None) == INVALID
