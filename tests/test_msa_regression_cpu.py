"""Sentiment regression (MOSI / MOSEI ``regression_labels``) checks that need no GPU: the epoch scores computed from
a ``tspm_regress_stats`` record against the direct computation on the raw arrays, the loss-group detection, the float
labels of the corpus, the head kernel's limits and the builder's ``output_dim``."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

from tspm_amd import _lib as L
from tspm_amd import mosi as M
from tspm_amd import msa_metrics as MM

KEYS = ["MAE", "Corr", "Mult_acc_7", "Mult_acc_5", "Mult_acc_3", "Has0_acc_2", "Has0_F1_score", "Non0_acc_2",
        "Non0_F1_score"]
EDGES = np.array([0.0, -0.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 3.0, -3.0, 3.7, -4.2, 1e-7, -1e-7], dtype=np.float32)


def _direct(p, y):
    """The standard CMU-MOSI scores straight from the raw arrays."""
    from sklearn.metrics import accuracy_score, f1_score
    p64, y64 = p.astype(np.float64), y.astype(np.float64)
    out = {"MAE": np.mean(np.abs(p64 - y64)),
           "Corr": np.corrcoef(p64, y64)[0][1] if p64.std() > 0 and y64.std() > 0 else float("nan")}
    for k, name in ((3, "Mult_acc_7"), (2, "Mult_acc_5"), (1, "Mult_acc_3")):
        out[name] = np.mean(np.round(np.clip(p, -k, k)) == np.round(np.clip(y, -k, k)))
    out["Has0_acc_2"] = accuracy_score(y >= 0, p >= 0)
    out["Has0_F1_score"] = f1_score(y >= 0, p >= 0, average="weighted")
    nz = y != 0
    out["Non0_acc_2"] = accuracy_score(y[nz] > 0, p[nz] > 0)
    out["Non0_F1_score"] = f1_score(y[nz] > 0, p[nz] > 0, average="weighted")
    return {k: round(float(v), 4) for k, v in out.items()}


def _groups():
    g = np.random.default_rng(7)
    n = 400
    y = (g.integers(-15, 16, n) / 5.0).astype(np.float32)  # the 0.2 grid of the real labels, zeros included
    p = (y + g.normal(0, 1.2, n)).astype(np.float32)
    yy, pp = np.meshgrid(EDGES, EDGES)
    mixed = (np.concatenate([p, pp.reshape(-1)]), np.concatenate([y, yy.reshape(-1)]))
    positive = (np.abs(p[:60]) + 0.1, np.abs(y[:60]) + 0.2)  # Corr defined, the negative class empty in both tasks
    return {"mixed": mixed, "positive": positive}


@pytest.mark.parametrize("name", ["mixed", "positive"])
def test_msa_regression_equals_the_direct_computation(name):
    p, y = _groups()[name]
    got, want = MM.msa_regression(MM.regression_record(p, y)), _direct(p, y)
    print(name, got)
    assert got == want


def test_msa_regression_keys_order_and_empty_group():
    p, y = _groups()["mixed"]
    assert list(MM.msa_regression(MM.regression_record(p, y))) == KEYS == list(MM.REGRESSION_KEYS)
    empty = MM.msa_regression(MM.regression_record(np.zeros(0), np.zeros(0)))
    assert list(empty) == KEYS and all(np.isnan(v) for v in empty.values())
    flat = MM.msa_regression(MM.regression_record(np.full(5, 1.25), np.linspace(-1, 1, 5)))
    assert np.isnan(flat["Corr"]) and flat["MAE"] == round(float(np.mean(np.abs(1.25 - np.linspace(-1, 1, 5)))), 4)


def test_record_words_round_trip_through_the_device_layout():
    """metrics.regress_records decodes the 66-word device record (tspm_regress_stats) into regression_record's dict."""
    from tspm_amd.metrics import regress_records
    p, y = _groups()["mixed"]
    rec = MM.regression_record(p, y)
    words = np.zeros((2, L.REGRESS_STATS_WORDS), np.int64)
    words[1, 0] = rec["n"]
    words[1, 1:8] = np.array([rec[k] for k in ("sum_abs", "sum_sq", "sum_p", "sum_y", "sum_pp", "sum_yy", "sum_py")]
                             ).view(np.int64)
    words[1, 8:57], words[1, 57:66] = rec["conf7"].reshape(-1), rec["sign3"].reshape(-1)
    dec = regress_records(words)
    assert dec[0]["n"] == 0 and MM.msa_regression(dec[1]) == MM.msa_regression(rec)
    assert np.array_equal(dec[1]["conf7"], rec["conf7"]) and np.array_equal(dec[1]["sign3"], rec["sign3"])


def test_rounding_after_a_narrower_clip_follows_from_conf7():
    """round(clip(x, -k, k)) == clip(round(clip(x, -3, 3)), -k, k): why conf7 carries Acc-5 and Acc-3."""
    g = np.random.default_rng(0)
    x = np.concatenate([g.normal(0, 2.5, 200000).astype(np.float32), np.arange(-9, 10, dtype=np.float32) / 2])
    for k in (1, 2):
        assert np.array_equal(np.round(np.clip(x, -k, k)), np.clip(np.round(np.clip(x, -3, 3)), -k, k))


def _group(fn, weight=1.0, n=1):
    return {f"t{i}": SimpleNamespace(loss_fn=fn, weight=weight) for i in range(n)}


def test_regress_term_detection():
    assert M._regress_term(_group(nn.L1Loss(), 0.5)) == (L.REGRESS_L1, 0.5)
    assert M._regress_term(_group(nn.MSELoss(), 2.0)) == (L.REGRESS_MSE, 2.0)
    assert M._regress_term(_group(nn.L1Loss())) == (0, 1.0)
    assert M._regress_term(_group(nn.L1Loss(), n=2)) is None
    assert M._regress_term(_group(nn.L1Loss(reduction="sum"))) is None
    assert M._regress_term(_group(nn.MSELoss(reduction="none"))) is None
    assert M._regress_term(_group(nn.CrossEntropyLoss())) is None
    assert M._regress_term(None) is None
    # regression mode needs the one-output head as well
    torch.manual_seed(0)
    assert M._regress_mode(M.build_utt_fusion("mosi", output_dim=1), _group(nn.L1Loss())) == (0, 1.0)
    assert M._regress_mode(M.build_utt_fusion("mosi"), _group(nn.L1Loss())) is None


def test_regression_labels_are_float32():
    from tspm_amd import mosi_data as D
    split = {"audio": np.zeros((3, 4, 5)), "vision": np.zeros((3, 4, 20)), "text": np.zeros((3, 4, 8)),
             "classification_labels": np.array([[1], [2], [0]]), "regression_labels": np.array([[0.2], [-1.4], [0.0]])}
    c = D.MosiCorpus.from_split(split, "regression_labels")
    assert c.labels.dtype == np.float32 and c.labels.shape == (3,)
    np.testing.assert_array_equal(c.labels, np.array([0.2, -1.4, 0.0], np.float32))
    s = D.synthetic_mosi_corpus(64, seed=3, steps=4, feats=(5, 20, 8), regression=True)
    assert s.labels.dtype == np.float32 and (s.labels == 0).any() and np.abs(s.labels).max() <= 3
    assert np.allclose(s.labels * 5, np.round(s.labels * 5))
    # the class-label stream of the same seed is what it was
    assert D.synthetic_mosi_corpus(64, seed=3, steps=4, feats=(5, 20, 8)).labels.dtype == np.int64


def test_regress_head_supported_mirrors_the_limits():
    ok = L.regress_head_supported
    assert ok(1, 4) and ok(1024, 128) and ok(128, 32) and ok(256, 48) and ok(128, 64)
    assert not ok(0, 32) and not ok(1025, 32) and not ok(128, 0) and not ok(128, 132) and not ok(128, 30)
    assert L.REGRESS_STATS_WORDS == 66 and L.RegressHeadDesc().n == 0


def test_builder_output_dim_changes_fc_out_only():
    torch.manual_seed(5)
    ref = M.build_utt_fusion("mosi").state_dict()
    torch.manual_seed(5)
    m = M.build_utt_fusion("mosi", output_dim=1)
    sd = m.state_dict()
    assert m.netC.fc_out.out_features == 1 and list(sd) == list(ref)
    same = [k for k in sd if not k.startswith("netC.fc_out.")]
    assert len(same) == 22 and all(torch.equal(sd[k], ref[k]) for k in same)
    assert M.build_utt_fusion("mosei", output_dim=1).netC.fc_out.in_features == 48
