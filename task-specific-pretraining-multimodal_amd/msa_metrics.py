"""The MOSI / MOSEI epoch metric of the UTT-Fusion YAMLs (configs/mosi/centralised/utt_fusion_base_training.yaml
``metrics: MSA: metrics.msa_binary_classification``), restated for the device-count recorder.

Reference: MML_Suite/metrics/msa.py:8-26 (``msa_binarize``) and :44-92 (``msa_binary_classification``).  Classes
are 0 negative / 1 neutral / 2 positive (data/mosi.py classification_labels).  "Has0" scores neutral-vs-rest
over every sample, "Non0" positive-vs-negative over the non-neutral samples.  Reference quirks kept as they are,
because the keys and values must be the reference's: the Recall_* and Precision_* entries are computed with
``f1_score`` (msa.py:54-59,66-71), ``accuracy_score`` takes (preds, truth) — symmetric, so harmless — and every
value is ``round(x, 4)``.

The function is a function of the 3x3 confusion matrix only, so ``metrics.evaluate`` feeds it the expanded
arrays of the device counts (order-independent integer sums: the values are the raw-array call's).
"""
from __future__ import annotations

from typing import Dict

import numpy as np


def msa_binarize(preds: np.ndarray, labels: np.ndarray):
    """msa.py:8-26: (binary_preds, binary_truth, non_zero_indices, non_zero_binary_preds, non_zero_binary_truth)."""
    preds, labels = np.asarray(preds), np.asarray(labels)
    binary_truth = (labels == 1).astype(int)
    binary_preds = (preds == 1).astype(int)
    nz = np.where(labels != 1)[0]
    return binary_preds, binary_truth, nz, (preds[nz] == 2).astype(int), (labels[nz] == 2).astype(int)


def msa_binary_classification(y_true: np.ndarray, y_pred: np.ndarray) -> Dict[str, float]:
    """msa.py:44-92 — the 20 rounded scores, same keys in the same order."""
    from sklearn.metrics import accuracy_score, f1_score

    bp, bt, _, nzp, nzt = msa_binarize(y_pred, y_true)
    out: Dict[str, float] = {}
    for tag, (truth, pred) in (("Non0", (nzt, nzp)), ("Has0", (bt, bp))):
        out[f"{tag}_Accuracy"] = round(accuracy_score(pred, truth), 4)
        for name in ("F1", "Recall", "Precision"):  # all three are f1_score in the reference (msa.py:51-71)
            for avg in ("weighted", "macro", "micro"):
                out[f"{tag}_{name}_{avg}"] = round(f1_score(truth, pred, average=avg), 4)
    return out


# ------------------------------------------------------------------------------------------------
# Sentiment regression (continuous score in [-3, 3]; ``regression_labels``)
# ------------------------------------------------------------------------------------------------
REGRESSION_KEYS = ("MAE", "Corr", "Mult_acc_7", "Mult_acc_5", "Mult_acc_3", "Has0_acc_2", "Has0_F1_score",
                   "Non0_acc_2", "Non0_F1_score")
_SUMS = ("sum_abs", "sum_sq", "sum_p", "sum_y", "sum_pp", "sum_yy", "sum_py")


def regression_record(preds: np.ndarray, labels: np.ndarray) -> Dict[str, object]:
    """The ``tspm_regress_stats`` record (include/tspm.h) of raw predictions / labels, in numpy: ``n``, the seven
    double sums, ``conf7`` [7, 7] and ``sign3`` [3, 3] (rows: label, columns: prediction).  Rows with a NaN label or
    prediction are left out, as the kernel leaves them out."""
    p32, y32 = np.asarray(preds, np.float32).reshape(-1), np.asarray(labels, np.float32).reshape(-1)
    ok = ~(np.isnan(p32) | np.isnan(y32))
    p32, y32 = p32[ok], y32[ok]
    p, y = p32.astype(np.float64), y32.astype(np.float64)
    e = p - y
    rec: Dict[str, object] = {"n": int(p.size), "sum_abs": float(np.abs(e).sum()), "sum_sq": float((e * e).sum()),
                              "sum_p": float(p.sum()), "sum_y": float(y.sum()), "sum_pp": float((p * p).sum()),
                              "sum_yy": float((y * y).sum()), "sum_py": float((p * y).sum())}
    conf7, sign3 = np.zeros((7, 7), np.int64), np.zeros((3, 3), np.int64)
    np.add.at(conf7, (np.round(np.clip(y32, -3, 3)).astype(int) + 3, np.round(np.clip(p32, -3, 3)).astype(int) + 3), 1)
    np.add.at(sign3, (np.sign(y32).astype(int) + 1, np.sign(p32).astype(int) + 1), 1)
    rec["conf7"], rec["sign3"] = conf7, sign3
    return rec


def _weighted_f1(c: np.ndarray) -> float:
    """sklearn's ``f1_score(truth, pred, average="weighted")`` from the confusion matrix c[truth][pred]: per class
    2 TP / (2 TP + FP + FN) (0 when the class occurs in neither), weighted by the class's true count."""
    c = np.asarray(c, np.float64)
    support = c.sum(1)
    if support.sum() == 0:
        return float("nan")
    tp = np.diag(c)
    den = support + c.sum(0)
    f1 = np.divide(2 * tp, den, out=np.zeros_like(tp), where=den > 0)
    return float((f1 * support).sum() / support.sum())


def _acc(c: np.ndarray) -> float:
    c = np.asarray(c, np.float64)
    return float(np.trace(c) / c.sum()) if c.sum() > 0 else float("nan")


def _collapse(conf7: np.ndarray, k: int) -> np.ndarray:
    """conf7 with both indices clipped to [-k, k]: round(clip(x, -k, k)) == clip(round(clip(x, -3, 3)), -k, k)."""
    idx = np.clip(np.arange(-3, 4), -k, k) + k
    out = np.zeros((2 * k + 1, 2 * k + 1), np.int64)
    np.add.at(out, (idx[:, None], idx[None, :]), np.asarray(conf7))
    return out


def msa_regression(record) -> Dict[str, float]:
    """The CMU-MOSI / CMU-MOSEI regression scores of one ``tspm_regress_stats`` record (``regression_record``'s dict):
    MAE, Pearson correlation, 7- / 5- / 3-class accuracy of the rounded clipped score, and the two binary tasks —
    "Has0": y >= 0 against p >= 0 over every row, "Non0": y > 0 against p > 0 over the rows with y != 0 — each as
    accuracy and weighted F1; every value ``round(x, 4)``.  These are the standard definitions of the field, written
    from those definitions: they are not restated from a file of the reference.  Corr is NaN when a variance is 0;
    a score over no rows is NaN."""
    n = int(record["n"])
    s = {k: float(record[k]) for k in _SUMS}
    conf7, sign3 = np.asarray(record["conf7"], np.int64), np.asarray(record["sign3"], np.int64)
    nan = float("nan")
    out: Dict[str, float] = {"MAE": s["sum_abs"] / n if n else nan}
    vp, vy = n * s["sum_pp"] - s["sum_p"] ** 2, n * s["sum_yy"] - s["sum_y"] ** 2
    cov = n * s["sum_py"] - s["sum_p"] * s["sum_y"]
    out["Corr"] = cov / float(np.sqrt(vp * vy)) if n and vp > 0 and vy > 0 else nan
    out["Mult_acc_7"] = _acc(conf7)
    out["Mult_acc_5"] = _acc(_collapse(conf7, 2))
    out["Mult_acc_3"] = _acc(_collapse(conf7, 1))
    has0 = np.array([[sign3[0, 0], sign3[0, 1:].sum()], [sign3[1:, 0].sum(), sign3[1:, 1:].sum()]])
    non0 = np.array([[sign3[0, :2].sum(), sign3[0, 2]], [sign3[2, :2].sum(), sign3[2, 2]]])
    out["Has0_acc_2"], out["Has0_F1_score"] = _acc(has0), _weighted_f1(has0)
    out["Non0_acc_2"], out["Non0_F1_score"] = _acc(non0), _weighted_f1(non0)
    return {k: round(out[k], 4) for k in REGRESSION_KEYS}
