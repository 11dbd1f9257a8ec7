"""MOSI / MOSEI encoder pre-training, the parts that need no GPU: the tspm_mono_head_step entry point (exported,
bound, refusing bad descriptors before any launch), MonomodalEncoder's state_dict over the MOSI encoders, and the
single-modality MOSI dataset's construction."""
import ctypes

import pytest
import torch

import tspm_amd  # noqa: F401
from tspm_amd import _lib as L
from tspm_amd import monomodal as MM
from tspm_amd import mosi as M
from tspm_amd.mosi_data import MOSI, synthetic_mosi_corpus


def _desc(**kw):
    """A well-formed training descriptor (fake 16-byte-aligned addresses: nothing is launched here)."""
    d = L.MonoHeadDesc(n=128, hid=64, classes=3, ld_emb=64, ld_demb=64, loss_weight=1.0)
    for name in ("emb", "w", "b", "labels", "logits", "loss", "preds", "dw", "db", "demb"):
        setattr(d, name, 16)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_mono_head_step_is_exported_and_bound():
    lib = L.load()
    assert lib.tspm_abi_version() == L.ABI_VERSION == 23
    assert "tspm_mono_head_step" in L._SIGS and hasattr(ctypes.CDLL(L.LIB_PATH), "tspm_mono_head_step")
    # int32 x5, float, 11 pointers
    assert ctypes.sizeof(L.MonoHeadDesc) == 6 * 4 + 11 * 8


@pytest.mark.parametrize("bad", [dict(classes=17), dict(hid=66), dict(n=0), dict(n=1025), dict(emb=None),
                                 dict(demb=None), dict(hid=132, ld_emb=132, ld_demb=132), dict(classes=0),
                                 dict(ld_emb=60), dict(ld_demb=60), dict(emb=20), dict(logits=None), dict(loss=None),
                                 dict(db=None), dict(labels=None)])
def test_mono_head_step_refuses_bad_descriptors_before_launch(bad):
    lib = L.load()
    assert lib.tspm_mono_head_step(ctypes.byref(_desc(**bad)), None) == 1, bad
    assert lib.tspm_mono_head_step(None, None) == 1


def test_monomodal_encoder_state_dict_keys_over_mosi_encoders():
    m = MM.MonomodalEncoder(M.LSTMEncoder(5, 64), 64, 3)
    assert list(m.state_dict()) == ["encoder.rnn.weight_ih_l0", "encoder.rnn.weight_hh_l0", "encoder.rnn.bias_ih_l0",
                                    "encoder.rnn.bias_hh_l0", "classifier.weight", "classifier.bias"]
    assert m.fused_head is MM.FUSED_HEAD_DEFAULT and MM.MonomodalEncoder(M.LSTMEncoder(5, 64), 64, 3,
                                                                         fused_head=False).fused_head is False
    t = MM.MonomodalEncoder(M.TextCNN(768, 64, dropout=0.5), 64, 3)
    enc_keys = [k[len("encoder."):] for k in t.state_dict() if k.startswith("encoder.")]
    assert enc_keys == list(M.build_utt_fusion("mosi").netT.state_dict())
    assert list(m.get_encoder().state_dict()) == list(M.build_utt_fusion("mosi").netA.state_dict())
    assert m._mosi_encoder() and not m._hip_encoder()


def test_mosi_encoders_refuse_the_cpu():
    with pytest.raises(L.TspmError):
        M.TextCNN(768, 64)(torch.zeros(2, 6, 768))
    m = MM.MonomodalEncoder(M.LSTMEncoder(5, 64), 64, 3).train()
    with pytest.raises(L.TspmError):
        m(torch.zeros(2, 6, 5))


def test_mosi_single_modality_dataset_constructs():
    corpus = synthetic_mosi_corpus(12, seed=1, steps=6)
    for m in ("audio", "video", "text"):
        ds = MOSI(corpus=corpus, target_modality=m, device="cpu")
        assert ds.target_modality == m and tuple(ds._want()) == (m,) and len(ds) == 12
    assert tuple(MOSI(corpus=corpus, device="cpu")._want()) == ("audio", "video", "text")
    with pytest.raises(AssertionError, match="Invalid modality provided"):
        MOSI(corpus=corpus, target_modality="image", device="cpu")


def test_loader_bookkeeping_keys_are_reserved():
    batch = {"audio": 0, "label": 1, "pattern_name": 2, "pattern_names": 3, "steps": 4, "time_major": 5}
    assert MM.select_modality_key(batch, "MOSI_Audio_Encoder_Pretrain") == "audio"
