"""MMIMDb encoder pre-training, the parts that need no GPU: the wrapper's state_dict keys, the device-only rule, the
refusal of optimizers and loss groups the fused step cannot take (this encoder has no autograd path), the
tspm_mono_head_bce_desc binding's layout, and the loader's batch keys."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from tspm_amd import _lib as L
from tspm_amd import mmimdb as M
from tspm_amd.monomodal import MonomodalEncoder, bce_head_choice, fit_monomodal, select_modality_key


def _model():
    torch.manual_seed(0)
    return MonomodalEncoder(M.MMIMDbModalityEncoder(8, 4), 4, 3)


def _batch():
    return {"text": torch.zeros(4, 8), "label": torch.zeros(4, 3)}


class _Group(dict):
    pass


def test_state_dict_keys_are_the_reference_wrappers():
    keys = list(_model().state_dict())
    assert keys == ["encoder.net.0.weight", "encoder.net.0.bias", "encoder.net.0.running_mean",
                    "encoder.net.0.running_var", "encoder.net.0.num_batches_tracked", "encoder.net.1.weight",
                    "encoder.net.1.bias", "classifier.weight", "classifier.bias"]
    assert all(k.startswith(("encoder.net.0.", "encoder.net.1.", "classifier.")) for k in keys)
    # the hand-off file's keys are what MMIMDb.get_encoder(...) holds
    fusion_enc = M.MMIMDbModalityEncoder(8, 4)
    assert list(_model().get_encoder().state_dict()) == list(fusion_enc.state_dict())


def test_cpu_tensor_raises_from_the_encoder_and_from_the_wrapper():
    m = _model().eval()
    with pytest.raises(L.TspmError, match="MI355X"):
        m.encoder(torch.zeros(4, 8))
    with pytest.raises(L.TspmError, match="MI355X"):
        m(torch.zeros(4, 8))
    with pytest.raises(L.TspmError, match="MI355X"):
        m.validation_step(_batch(), None, "cpu", None)


def test_other_optimizers_and_loss_groups_are_refused():
    m = _model()
    with pytest.raises(L.TspmError, match="FusedAdam.*no autograd path"):
        m.train_step(_batch(), torch.optim.Adam(m.parameters()), None, "cpu", None)
    ce = _Group(ce=SimpleNamespace(loss_fn=torch.nn.CrossEntropyLoss(), weight=1.0))
    with pytest.raises(L.TspmError, match="loss group.*no autograd path"):
        m.train_step(_batch(), torch.optim.Adam(m.parameters()), ce, "cpu", None)
    with pytest.raises(L.TspmError, match="loss group"):
        m.eval().validation_step(_batch(), ce, "cpu", None)
    with pytest.raises(L.TspmError, match="loss group"):
        m.train_step(_batch(), torch.optim.Adam(m.parameters()), lambda lg, lb: {"total_loss": lg.sum()}, "cpu", None)
    # no parameter received a gradient: nothing was built
    assert all(p.grad is None for p in m.parameters())


def test_non_loss_save_metric_is_refused_before_the_first_epoch():
    with pytest.raises(ValueError, match="save_metric"):
        fit_monomodal(_model(), None, None, {}, 1, experiment_name="MMIMDb_Image_Encoder_Pretrain",
                      save_metric="accuracy")


def test_mono_head_bce_desc_layout():
    """include/tspm.h's tspm_mono_head_bce_desc, written out: five int32 and two floats, four bytes of padding, twelve
    pointers, one size_t."""
    ptr = ctypes.sizeof(ctypes.c_void_p)
    assert ptr == 8
    want, off = {}, 0
    for name in ("n", "hid", "classes", "ld_emb", "ld_demb", "loss_weight", "threshold"):
        want[name], off = off, off + 4
    off = 32  # 28 bytes rounded up to the pointers' alignment
    for name in ("emb", "w", "b", "targets", "logits", "loss", "preds", "dw", "db", "demb", "stats", "workspace",
                 "workspace_bytes"):
        want[name], off = off, off + 8
    got = {name: getattr(L.MonoHeadBceDesc, name).offset for name, _ in L.MonoHeadBceDesc._fields_}
    assert got == want and ctypes.sizeof(L.MonoHeadBceDesc) == off == 136
    assert L.MonoHeadBceDesc.loss_weight.size == 4 and L.MonoHeadBceDesc.workspace_bytes.size == 8


def test_mono_head_bce_entry_points_are_exported_and_refuse_before_launch():
    lib = L.load()
    assert lib.tspm_abi_version() == L.ABI_VERSION  # the entry points are additions: the version number stays
    assert "tspm_mono_head_bce_step" in L._SIGS and hasattr(ctypes.CDLL(L.LIB_PATH), "tspm_mono_head_bce_step")
    assert lib.tspm_mono_head_bce_step(None, None) == 1
    # valid sizes, no pointers: refused (TSPM_ERR_INVALID) without a launch
    d = L.MonoHeadBceDesc(n=128, hid=512, classes=23, ld_emb=512, ld_demb=512, loss_weight=1.0, threshold=0.5)
    assert lib.tspm_mono_head_bce_step(ctypes.byref(d), None) == 1
    for n, hid, classes in ((1025, 512, 23), (128, 516, 23), (128, 30, 23), (128, 512, 33), (0, 512, 23)):
        assert lib.tspm_mono_head_bce_workspace(n, hid, classes) == 0
    # up to 16 workgroups, each with a record of two doubles, db, the counts and dw, behind a 64-byte header
    rec = (4 + 4 * 23 + 23 * 512 + 3) // 4 * 4
    assert lib.tspm_mono_head_bce_workspace(64, 512, 23) == 64 + 8 * rec * 4
    assert lib.tspm_mono_head_bce_workspace(128, 512, 23) == 64 + 16 * rec * 4
    assert lib.tspm_mono_head_bce_workspace(1024, 512, 23) == 64 + 16 * rec * 4
    assert lib.tspm_mono_head_bce_workspace(1, 512, 23) == 64 + rec * 4


def test_head_choice_follows_the_request_the_measured_default_and_the_kernel_limits():
    assert _model().fused_head is None and MonomodalEncoder(M.MMIMDbModalityEncoder(8, 4), 4, 3, fused_head=True).fused_head
    assert bce_head_choice(None, 256, 512, 23) and not bce_head_choice(None, 128, 512, 23)
    assert bce_head_choice(True, 128, 512, 23) and not bce_head_choice(False, 256, 512, 23)
    # outside tspm_mono_head_bce_step's limits the separate launches run, whatever was asked for
    for n, hid, classes in ((1025, 512, 23), (256, 516, 23), (256, 30, 23), (256, 512, 33)):
        assert not bce_head_choice(True, n, hid, classes) and not bce_head_choice(None, n, hid, classes)


def test_mono_loader_batch_keys_select_the_modality():
    class _Corpus:  # MMIMDbCorpus' attributes without a device
        pass
    for modality, name in (("image", "MMIMDb_Image_Encoder_Pretrain"), ("text", "MMIMDb_Text_Encoder_Pretrain")):
        batch = {modality: torch.zeros(2, 8), "label": torch.zeros(2, 3)}
        assert select_modality_key(batch, name) == modality
    c = _Corpus()
    c.n, c.device = 10, "cpu"
    loader = M.MonoLoader(c, "text", 4, False, 0, False)
    assert len(loader) == 3 and len(M.MonoLoader(c, "text", 4, False, 0, True)) == 2
    with pytest.raises(ValueError, match="modality"):
        M.MonoLoader(c, "audio", 4, False, 0, False)
