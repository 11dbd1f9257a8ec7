"""Epoch harness: train / validate epochs and the fit loop of MML_Suite/train_multimodal.py on the
fused HIP steps, with the epoch's bookkeeping on the device.

Reference (``MML_Suite/``):
  train_epoch            train_multimodal.py:438-491  per batch model.train_step → loss.item(); mean
  validate_epoch         train_multimodal.py:494-541  per batch model.validation_step → loss.item(); mean
  check_early_stopping   train_multimodal.py:329-377
  _train_loop            train_multimodal.py:554-791  epochs: metrics reset → train → calculate_all_groups
                         → validate → calculate_all_groups → epoch_metrics.json → early stopping →
                         CheckpointManager.save_checkpoint(epoch_{n}.pth, best.pth) → scheduler.step(val loss)
  test                   train_multimodal.py:866-917  load best.pth, validate_epoch on each test split
  CheckpointManager      experiment_utils/checkpoints.py:13-120

What differs is where the per-batch work happens: the reference synchronises on every batch
(``loss.item()`` and the predictions' ``.cpu()``); here each batch is ONE gather launch
(data.DeviceLoader writing into the step's static inputs) plus ONE graph replay that also records
the batch loss and the confusion counts (tspm_classify_update), and the host reads the epoch's
losses and counts once.  Epoch loss = ``np.mean`` of the per-batch fp32 losses as Python floats, as
the reference computes it; metrics via metrics.DeviceMetricRecorder (same keys and values as the
reference's MetricRecorder).
"""
from __future__ import annotations

import json
import time
from pathlib import Path
from typing import Any, Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from .metrics import ClassificationLog, DeviceMetricRecorder, RegressionLog, RegressionMetricRecorder
from .modules import NUM_CLASSES, modality_key
from .step import (FusedCachedEvalStep, FusedCachedHeadStep, FusedEvalStep, FusedHeadStagePatternStep, FusedHeadStageStep,
                   FusedPatternEvalStep, FusedTrainStep, head_stage_frozen, norm_avmnist_patterns, train_step_key)

# the AVMNIST YAML's metric block (configs/avmnist/centralised/train_avmnist_resnet.yaml:105-166)
AVMNIST_METRICS = {
    "metrics": {
        "accuracy": {"function": "sklearn.metrics.accuracy_score", "kwargs": {}},
        "balanced_accuracy": {"function": "sklearn.metrics.balanced_accuracy_score", "kwargs": {}},
        **{f"{m}_{avg}": {"function": f"sklearn.metrics.{fn}", "kwargs": {"average": avg, "zero_division": 0}}
           for m, fn in (("f1", "f1_score"), ("precision", "precision_score"), ("recall", "recall_score"))
           for avg in ("macro", "micro", "weighted")},
        "ConfusionMatrix": {"function": "sklearn.metrics.confusion_matrix", "kwargs": {"labels": list(range(10))}},
    },
    "groups": {"classification": ["accuracy", "balanced_accuracy", "f1_macro", "f1_micro", "f1_weighted",
                                  "precision_macro", "precision_micro", "precision_weighted", "recall_macro",
                                  "recall_micro", "recall_weighted", "ConfusionMatrix"]},
}


# the MOSI / MOSEI UTT-Fusion YAMLs' metric block (configs/mosi/centralised/utt_fusion_base_training.yaml:151-162)
MOSI_METRICS = {
    "metrics": {
        "MSA": {"function": "metrics.msa_binary_classification", "kwargs": {}, "level": "epoch"},
        "ConfusionMatrix": {"function": "sklearn.metrics.confusion_matrix", "kwargs": {"labels": [0, 1, 2]},
                            "level": "epoch"},
    },
    "groups": {"classification": ["MSA", "ConfusionMatrix"]},
}


def check_early_stopping(val_metrics: Dict[str, Any], best_metrics: Optional[Dict[str, Any]], patience: int,
                         min_delta: float, wait: int, mode: str = "minimize",
                         target_metric: str = "loss") -> Tuple[bool, bool, int]:
    """train_multimodal.py:329-377: (is_best, should_continue, wait)."""
    if best_metrics is None:
        return True, True, 0
    value, best = val_metrics.get(target_metric), best_metrics.get(target_metric)
    if value is None or best is None:
        raise ValueError(f"Metric '{target_metric}' not found in val_metrics or best_metrics.")
    if (mode == "minimize" and value < best - min_delta) or (mode == "maximize" and value > best + min_delta):
        return True, True, 0
    wait += 1
    return False, wait < patience, wait


class CheckpointManager:
    """experiment_utils/checkpoints.py:13-120 — same files (``epoch_{n}.pth``, ``best.pth``) and dict
    keys (``model_state_dict``, ``optimizer_state_dict``, ``scheduler_state_dict``); state_dict keys and
    OIHW shapes are the reference's, so checkpoints load on either side."""

    def __init__(self, model_dir, save_metric: str = "loss", mode: str = "minimize", device: str = "cuda"):
        self.model_dir = Path(model_dir)
        self.save_metric, self.mode, self.device = save_metric, mode, device
        self.best_metric = float("inf") if mode == "minimize" else float("-inf")
        self.best_epoch = -1
        self.model_dir.mkdir(parents=True, exist_ok=True)

    def is_better(self, current: float) -> bool:
        return current < self.best_metric if self.mode == "minimize" else current > self.best_metric

    def save_checkpoint(self, model, optimizer, scheduler, epoch: int, metrics: Dict[str, float],
                        is_best: bool = False) -> None:
        state = {"model_state_dict": model.state_dict(), "optimizer_state_dict": optimizer.state_dict()}
        if scheduler is not None:
            state["scheduler_state_dict"] = scheduler.state_dict()
        torch.save(state, self.model_dir / f"epoch_{epoch}.pth")
        if is_best:
            torch.save(state, self.model_dir / "best.pth")
        value = metrics[self.save_metric]
        if self.is_better(value):
            self.best_metric, self.best_epoch = value, epoch

    def load_checkpoint(self, model, optimizer=None, scheduler=None, epoch: Optional[int] = None,
                        load_best: bool = False) -> Dict[str, Any]:
        name = "best.pth" if load_best else (f"epoch_{epoch}.pth" if epoch is not None else "last.pth")
        ck = torch.load(self.model_dir / name, map_location=self.device, weights_only=True)
        model.load_state_dict(ck["model_state_dict"])
        if optimizer is not None and "optimizer_state_dict" in ck:
            optimizer.load_state_dict(ck["optimizer_state_dict"])
        if scheduler is not None and "scheduler_state_dict" in ck:
            scheduler.load_state_dict(ck["scheduler_state_dict"])
        return ck


def cached_epoch_chunks(n_rows: int, batch_size: int, steps_per_call: Optional[int]) -> Tuple[List[int], int]:
    """How an epoch of ``n_rows`` cached rows at ``batch_size`` is cut into host calls → ``(chunks, tail)``: ``chunks``
    are the full batches in order, as calls of that many consecutive batches — ``full // K`` calls of K, then one call
    of the remaining ``full % K`` (5 full batches, K = 4: ``[4, 1]``; K >= full: ``[full]``; K of None or 1: ``[1] *
    full``, the per-batch epoch) — and ``tail`` is the short last batch's row count (0 = none), which always runs on
    the single-batch step.  K is capped at ``_lib.CACHED_HEAD_MAX_STEPS``."""
    if n_rows < 0 or batch_size < 1:
        raise ValueError("cached_epoch_chunks: n_rows >= 0 and batch_size >= 1")
    if steps_per_call is not None and int(steps_per_call) < 1:
        raise ValueError(f"steps_per_call must be >= 1, got {steps_per_call}")
    K = min(int(steps_per_call or 1), L.CACHED_HEAD_MAX_STEPS)
    full, tail = divmod(n_rows, batch_size)
    chunks = [K] * (full // K) + ([full % K] if full % K else [])
    return chunks, tail


class EpochRunner:
    """train_epoch / validate_epoch on the fused steps.  ``loader`` yields collate_fn-style batch dicts
    on the device (data.DeviceLoader / the drop-in DataLoader); batches of the runner's size are fed
    through the static buffers of one captured graph, a smaller last batch through a second one.  A
    ``"fused_patterns"`` batch (the samples once, unmasked) is one ``FusedPatternEvalStep`` replay that writes one loss
    entry per pattern, in pattern order, and every row's count under its pattern.  A model with frozen encoders
    (``AVMNIST.freeze_encoders``) trains on ``FusedHeadStageStep``, and an ``"all_patterns"`` train batch on
    ``FusedHeadStagePatternStep`` (one loss entry per step, every row's count under its pattern); both live in
    ``train_steps`` under ``step.train_step_key``'s keys, which for an all-trainable model are the batch sizes.  A
    ``"cached"`` batch (``data.DeviceLoader(ids_only=True)``: sample indices, no input tensors) runs on the dataset's
    ``embedding_cache(model)`` — ``FusedCachedHeadStep`` (keys with a trailing ``("cached",)``) or
    ``FusedCachedEvalStep`` — with the same loss entries and counts and no encoder launch.  With ``steps_per_call=K``
    an epoch on an ``ids_only`` ``DeviceLoader`` takes the loader's ``epoch_plan()`` and runs K consecutive batches per
    host call (``cached_epoch_chunks``): the same loss entries, order, metrics and batch count as the per-batch epoch."""

    def __init__(self, model, optimizer, loss_functions, metric_config=None, device=None, log_capacity: int = 1 << 16):
        self.model, self.optimizer, self.loss_functions = model, optimizer, loss_functions
        self.device = device or next(model.parameters()).device
        self.log = ClassificationLog(self.device, capacity=log_capacity)
        self.recorder = DeviceMetricRecorder(metric_config or AVMNIST_METRICS, self.log)
        self.train_steps: Dict[int, FusedTrainStep] = {}
        self.eval_steps: Dict[int, FusedEvalStep] = {}
        self.pattern_eval_steps: Dict[Tuple[Tuple[str, ...], int], FusedPatternEvalStep] = {}
        self._epoch_caches: Dict[int, Any] = {}  # dataset id -> its EmbeddingCache, for the running epoch

    def _train_step(self, n: int):
        key = train_step_key(self.model, n)
        st = self.train_steps.get(key)
        if st is None:
            # the flags are read (and every unsupported combination refused) before anything is built
            cls = FusedHeadStageStep if head_stage_frozen(self.model, self.optimizer) else FusedTrainStep
            st = cls(self.model, self.optimizer, self.loss_functions, n)
            self.train_steps[key] = st
        st.log = self.log
        return st

    def train_pattern_step_for(self, n: int, patterns=None) -> FusedHeadStagePatternStep:
        """The cached FusedHeadStagePatternStep for (patterns, batch size) — every pattern of an ``"all_patterns"`` batch
        (``data.AVMNIST.device_loader(all_patterns=True)``) trained in one step on frozen encoders; refused (with the
        BatchNorm argument) for a model whose encoders are not frozen."""
        pats = norm_avmnist_patterns(patterns)
        head_stage_frozen(self.model, self.optimizer, all_patterns=True)
        key = train_step_key(self.model, n, pats)
        st = self.train_steps.get(key)
        if st is None or st.eng_a is not self.model.audio_encoder.engine_for(st.A):  # the model dropped its engines
            st = FusedHeadStagePatternStep(self.model, self.optimizer, self.loss_functions, n, patterns=pats)
            self.train_steps[key] = st
        st.log = self.log
        return st

    def cached_train_step_for(self, n: int, cache, patterns=None, steps: int = 1) -> FusedCachedHeadStep:
        """The FusedCachedHeadStep for (patterns, batch size) on ``cache``: every pattern of the batch when ``patterns``
        is given (an ``"all_patterns"`` batch), else one pattern per sample.  Rebuilt for another cache.  ``steps=K >
        1``: the step that runs K batches of ``n`` per call, under its own key (the single step's plus ``("steps", K)``)."""
        pats = norm_avmnist_patterns(patterns) if patterns is not None else None
        key = train_step_key(self.model, n, pats, cached=True)
        if steps > 1:
            key = key + (("steps", int(steps)),)
        st = self.train_steps.get(key)
        if st is None or st.cache is not cache:
            st = FusedCachedHeadStep(self.model, self.optimizer, self.loss_functions, n, cache, patterns=pats,
                                     per_sample=pats is None, steps=steps)
            self.train_steps[key] = st
        st.log = self.log
        return st

    def cached_eval_step_for(self, n: int, cache, patterns=None, steps: int = 1) -> FusedCachedEvalStep:
        """The FusedCachedEvalStep for (patterns, batch size) on ``cache`` (``patterns``: a ``"fused_patterns"`` batch's;
        None: each row under its own keep flags); kept apart from the other eval steps under a ("cached", ...) key
        (``steps=K > 1``: K batches of ``n`` per call, the key plus ``("steps", K)``)."""
        pats = norm_avmnist_patterns(patterns) if patterns is not None else None
        key = (("cached",), pats, n) + ((("steps", int(steps)),) if steps > 1 else ())
        st = self.pattern_eval_steps.get(key)
        if st is None or st.cache is not cache:
            st = FusedCachedEvalStep(self.model, self.loss_functions, n, cache, self.log, patterns=pats,
                                     per_sample=pats is None, steps=steps)
            self.pattern_eval_steps[key] = st
        st.log = self.log
        return st

    def _multi_step_ok(self, npat: int) -> bool:
        """Whether ``FusedCachedHeadStep(steps > 1)`` takes this model and optimizer (else the epoch runs per batch)."""
        m = self.model
        ea, hd = int(m.embd_size_A), int(m.hidden_dim)
        return (getattr(self.optimizer, "clip_coef", None) is None and
                L.cached_head_train_supported(ea + int(m.embd_size_I), ea, hd, hd // 2, NUM_CLASSES, npat))

    def _cached_epoch(self, loader, steps_per_call: int, train: bool) -> None:
        """A whole ``ids_only`` epoch from the loader's ``epoch_plan()``: ``cached_epoch_chunks``' calls of K batches
        (and of the remaining full batches) on the multi-step steps, the short last batch on the single step."""
        from .data import DeviceLoader
        if not (isinstance(loader, DeviceLoader) and loader.ids_only):
            raise L.TspmError("steps_per_call needs an ids_only data.DeviceLoader (dataset.device_loader(..., "
                              "ids_only=True)): the epoch's sample order must be on the device as one plan")
        plan = loader.epoch_plan()
        if plan["n_batches"] == 0:
            return
        ds, B, ids = plan["dataset"], plan["batch_size"], plan["sample_ids"]
        cache = self._epoch_caches[id(ds)] = ds.embedding_cache(self.model)
        pats = plan.get("patterns")
        npat = len(norm_avmnist_patterns(pats)) if pats is not None else 1
        K = steps_per_call if (not train or self._multi_step_ok(npat)) else 1
        chunks, tail = cached_epoch_chunks(len(ids), B, K)
        step_for = self.cached_train_step_for if train else self.cached_eval_step_for
        at = 0
        for n, k in [(B, c) for c in chunks] + ([(tail, 1)] if tail else []):
            rows = slice(at, at + n * k)
            st = step_for(n, cache, pats, steps=k)
            if pats is not None:
                st.step(ids[rows])
            else:
                st.step(ids[rows], plan["keep"][rows], plan["pattern_ids"][rows])
            at += n * k

    def _cached(self, b, train: bool) -> None:
        """One ``"cached"`` batch on its dataset's embedding cache of this model, looked up once per epoch and dataset.
        A dataset that has no cache of this model yet gets one here — a fill pass over the whole split inside the
        epoch's first batch; ``fit(cache_embeddings=True)`` and ``dataset.embedding_cache(model)`` do it beforehand."""
        ds = b["dataset"]
        cache = self._epoch_caches.get(id(ds))
        if cache is None:
            cache = self._epoch_caches[id(ds)] = ds.embedding_cache(self.model)
        ids = b["sample_ids"]
        pats = b["patterns"] if (b.get("all_patterns") or b.get("fused_patterns")) else None
        st = (self.cached_train_step_for if train else self.cached_eval_step_for)(int(ids.numel()), cache, pats)
        if pats is not None:
            st.step(ids)
        else:
            g = b.get("pattern_ids")
            st.step(ids, b["keep"], g if g is not None else self.log.group_ids(b["pattern_name"]))

    def _eval_step(self, n: int) -> FusedEvalStep:
        st = self.eval_steps.get(n)
        if st is None:
            st = FusedEvalStep(self.model, self.loss_functions, n, self.log)
            self.eval_steps[n] = st
        st.log = self.log
        return st

    def pattern_eval_step_for(self, n: int, patterns=None) -> FusedPatternEvalStep:
        """The cached FusedPatternEvalStep for (patterns, batch size) — every pattern of a ``"fused_patterns"`` batch
        (``data.AVMNIST.device_loader(fuse_patterns=True)``) from one encoder pass; kept apart from ``eval_steps``."""
        key = (norm_avmnist_patterns(patterns), n)
        st = self.pattern_eval_steps.get(key)
        if st is None or st.eng_a is not self.model.audio_encoder.engine_for(st.A):  # the model dropped its engines
            st = FusedPatternEvalStep(self.model, self.loss_functions, n, self.log, patterns=key[0])
            self.pattern_eval_steps[key] = st
        st.log = self.log
        return st

    def _unpack(self, b):
        a, i = b[modality_key(b, "audio")], b[modality_key(b, "image")]
        g = b.get("pattern_ids")
        if g is None:
            g = self.log.group_ids(b["pattern_name"])
        return a, i, b["labels"], g

    def _finish(self, t0: float, loss: Optional[float] = None):
        conf, losses, _ = self.log.fetch()  # the epoch's only host synchronisation
        mean = ClassificationLog.mean_loss(losses)
        metrics = self.recorder.calculate_metrics_for_group("classification", loss=mean, conf=conf)
        return mean, time.time() - t0, metrics, len(losses)

    def train_epoch(self, loader: Iterable[Dict[str, Any]], steps_per_call: Optional[int] = None):
        """→ (mean batch loss, seconds, metrics dict, batches).  ``steps_per_call=K > 1``: ``_cached_epoch``."""
        self.log.reset()
        self._epoch_caches = {}
        t0 = time.time()
        if steps_per_call is not None and int(steps_per_call) > 1:
            self._cached_epoch(loader, int(steps_per_call), True)
            return self._finish(t0)
        fresh_zero = False  # the zero-input embeddings of an all-pattern epoch: refreshed on its first batch only
        for b in loader:
            if b.get("cached"):
                self._cached(b, True)
                continue
            if b.get("all_patterns"):
                a, i = b[modality_key(b, "audio")], b[modality_key(b, "image")]
                st = self.train_pattern_step_for(a.shape[0], b["patterns"])
                st.step(a, i, b["labels"], refresh_zero=not fresh_zero)
                fresh_zero = True
                continue
            a, i, lab, g = self._unpack(b)
            self._train_step(a.shape[0]).step(a, i, lab, g)
        return self._finish(t0)

    @torch.no_grad()
    def validate_epoch(self, loader: Iterable[Dict[str, Any]], steps_per_call: Optional[int] = None):
        self.log.reset()
        self._epoch_caches = {}
        t0 = time.time()
        self.model.eval()
        if steps_per_call is not None and int(steps_per_call) > 1:
            self._cached_epoch(loader, int(steps_per_call), False)
            return self._finish(t0)
        fresh_zero = False  # the zero-input embeddings: refreshed once per epoch (no weight changes inside it)
        for b in loader:
            if b.get("cached"):
                self._cached(b, False)
                continue
            if b.get("fused_patterns"):
                a, i = b[modality_key(b, "audio")], b[modality_key(b, "image")]
                st = self.pattern_eval_step_for(a.shape[0], b["patterns"])
                st.step(a, i, b["labels"], refresh_zero=not fresh_zero)
                fresh_zero = True
                continue
            a, i, lab, g = self._unpack(b)
            self._eval_step(a.shape[0]).step(a, i, lab, g)
        return self._finish(t0)


class MosiEpochRunner:
    """train_epoch / validate_epoch (train_multimodal.py:438-541) for UttFusionModel on the fused steps, over the
    seven missing-modality patterns (data/mosi.py:61-69).  A batch is a collate_fn-style dict — batch-first
    tensors, or the time-major buffers of this runner's own steps when the loader gathered into them
    (``MosiDeviceLoader`` with ``step_for`` pointed here by ``loader_for``) — or, for valid / test, the
    pattern-grouped ``{pattern: sub-batch}`` of data/mosi.py:236-251; each group is one ``validation_step`` (one
    ``FusedMosiEvalStep`` replay: its loss is one entry of the epoch's loss log, its rows go to the confusion
    counts of their pattern).  An ``"ids_only"`` batch (``MOSI.loader(ids_only=True)``: sample indices, no input
    tensors) runs on its dataset's ``embedding_cache(model)`` — ``FusedMosiCachedStep`` / ``FusedMosiCachedEvalStep``,
    the same loss entries and counts with no encoder launch.  A ``"fused_patterns"`` batch (``MOSI.loader(fuse_patterns=True)``: the samples once,
    unmasked) is one ``FusedMosiPatternEvalStep`` replay that writes the same per-pattern entries and counts from one
    encoder pass.  Per-pattern metrics come from ``DeviceMetricRecorder`` with the YAML's MSA and
    confusion-matrix functions (keys ``MSA_Has0_Accuracy_ATV`` ...; metric_recorder.py:147-209)."""

    def __init__(self, model, optimizer, loss_functions, metric_config=None, device=None, log_capacity: int = 1 << 16):
        from .mosi import _regress_mode
        from .mosi_data import PATTERNS
        self.model, self.optimizer, self.loss_functions = model, optimizer, loss_functions
        self.device = device or next(model.parameters()).device
        # regression mode (one-output fc_out, a single mean L1 / MSE term): the regression head's accumulators and
        # the MSA_<key>_<PATTERN> scores of msa_metrics.msa_regression under the group "regression"
        self.regression = _regress_mode(model, loss_functions) is not None
        if self.regression:
            self.log = RegressionLog(self.device, groups=PATTERNS, capacity=log_capacity)
            self.recorder = RegressionMetricRecorder(self.log)
        else:
            self.log = ClassificationLog(self.device, groups=PATTERNS, classes=3, capacity=log_capacity)
            self.recorder = DeviceMetricRecorder(metric_config or MOSI_METRICS, self.log)
        self.eval_steps: Dict[Tuple[int, int], Any] = {}
        self.ragged = False  # the loader's dataset carries per-sample lengths (mosi_data.MOSI(use_lengths=True))
        self.text_lengths = False  # ... and the text lengths too (mosi_data.MOSI(text_lengths=True))
        self.patterns = None  # the selected patterns of a fuse_patterns loader (loader_for)
        self.cached_steps: Dict[Any, Any] = {}  # the steps on a UttEmbeddingCache (ids_only batches)
        self._epoch_caches: Dict[Any, Any] = {}  # (dataset id, steps) -> its cache, for the running epoch

    def train_step_for(self, b: int, t, ragged: Optional[bool] = None, text_lengths: Optional[bool] = None):
        """The model's cached FusedMosiStep for (b, t); ``t`` an ``int`` or a triple (Ta, Tv, Tt) (``mosi.norm_steps``).
        ``ragged`` (default: what the current loader's dataset says): the step that reads per-sample lengths;
        ``text_lengths`` (same default): the step whose TextCNN reads the text lengths."""
        ragged = self.ragged if ragged is None else bool(ragged)
        tl = self.text_lengths if text_lengths is None else bool(text_lengths)
        st = self.model.fused_step(self.optimizer, self.loss_functions, b, t, ragged=ragged, text_lengths=tl)
        if st.log is not self.log:
            st.log, st.graph = self.log, None  # (the step's graph key holds the log: it would re-capture anyway)
        return st

    def eval_step_for(self, b: int, t, ragged: Optional[bool] = None, text_lengths: Optional[bool] = None):
        """The cached FusedMosiEvalStep for (b, t) — rebuilt when the model's engine for that shape is no longer
        the one it captured (``UttFusionModel._apply`` drops the engines on .to() / re-materialisation).  ``t``: an
        ``int`` or a triple (Ta, Tv, Tt), keyed by its normalised value."""
        from .mosi import FusedMosiEvalStep, norm_steps
        t = norm_steps(t)
        ragged = self.ragged if ragged is None else bool(ragged)
        tl = self.text_lengths if text_lengths is None else bool(text_lengths)
        key = ((b, t, "ragged") if ragged else (b, t)) + (("text_lengths",) if tl else ())
        st = self.eval_steps.get(key)
        if st is None or st.eng is not self.model._engine(b, t, self.device, ragged, tl):
            st = FusedMosiEvalStep(self.model, self.loss_functions, b, t, self.log, ragged=ragged, text_lengths=tl)
            self.eval_steps[key] = st
        return st

    def pattern_eval_step_for(self, b: int, t, patterns=None, ragged: Optional[bool] = None,
                              text_lengths: Optional[bool] = None):
        """The cached FusedMosiPatternEvalStep for (patterns, b, t) — every pattern of a batch from one encoder pass
        (``mosi_data.MOSI.loader(fuse_patterns=True)``).  ``patterns`` (default: the current fused loader's
        ``selected_patterns``, else all seven).  Cached in ``eval_steps`` under ``eval_step_for``'s key behind a
        ("patterns", names) head, which no per-pattern key has; rebuilt like those when the model dropped its engines."""
        from .mosi import FusedMosiPatternEvalStep, norm_patterns, norm_steps
        t, pats = norm_steps(t), norm_patterns(self.patterns if patterns is None else patterns)
        ragged = self.ragged if ragged is None else bool(ragged)
        tl = self.text_lengths if text_lengths is None else bool(text_lengths)
        key = (("patterns", pats),) + ((b, t, "ragged") if ragged else (b, t)) + (("text_lengths",) if tl else ())
        st = self.eval_steps.get(key)
        if st is None or st.eng is not self.model._pattern_engine(b, t, self.device, pats, ragged, tl):
            st = FusedMosiPatternEvalStep(self.model, self.loss_functions, b, t, self.log, patterns=pats, ragged=ragged,
                                          text_lengths=tl)
            self.eval_steps[key] = st
        return st

    def train_pattern_step_for(self, b: int, t, patterns=None, ragged: Optional[bool] = None,
                               text_lengths: Optional[bool] = None):
        """The model's cached FusedMosiPatternStep for (patterns, b, t) - every pattern of a batch trained in one step
        (``mosi_data.MOSI.loader(all_patterns=True)``), with this runner's log attached as ``train_step_for`` attaches
        it.  ``patterns`` (default: the current all-pattern loader's ``selected_patterns``, else all seven)."""
        from .mosi import norm_patterns
        ragged = self.ragged if ragged is None else bool(ragged)
        tl = self.text_lengths if text_lengths is None else bool(text_lengths)
        pats = getattr(self, "patterns", None) if patterns is None else patterns
        st = self.model.fused_pattern_step(self.optimizer, self.loss_functions, b, t, norm_patterns(pats), ragged=ragged,
                                           text_lengths=tl)
        if st.log is not self.log:
            st.log, st.graph = self.log, None  # (the step's graph key holds the log: it would re-capture anyway)
        return st

    def loader_for(self, loader, train: bool):
        """Point a ``MosiDeviceLoader`` at this runner's steps (batches gathered straight into their inputs): a
        ``fuse_patterns`` loader at ``pattern_eval_step_for``, a train ``all_patterns`` loader at
        ``train_pattern_step_for``, each with its dataset's selected patterns."""
        self.ragged = bool(getattr(getattr(loader, "ds", None), "use_lengths", False))
        self.text_lengths = bool(getattr(getattr(loader, "ds", None), "text_lengths", False))
        fused = bool(getattr(loader, "fuse_patterns", False)) and not train
        allp = bool(getattr(loader, "all_patterns", False)) and train
        self.patterns = tuple(loader.ds.selected_patterns) if fused or allp else None
        if hasattr(loader, "step_for"):
            loader.step_for = (self.train_pattern_step_for if allp else self.train_step_for if train else
                               self.pattern_eval_step_for if fused else self.eval_step_for)
        return loader

    def cached_train_step_for(self, n: int, cache, patterns=None):
        """The ``FusedMosiCachedStep`` for (patterns, batch size) on ``cache`` (a ``mosi.UttEmbeddingCache``): every
        pattern of the batch when ``patterns`` is given (an ``"all_patterns"`` batch), else one pattern per sample.
        Kept in ``cached_steps``; rebuilt for another cache, optimizer or set of flags."""
        from .mosi import FusedMosiCachedStep, norm_patterns
        pats = norm_patterns(patterns) if patterns is not None else None
        key = ("train", pats, int(n), id(self.optimizer), self.model.flag_state()[0])
        st = self.cached_steps.get(key)
        if st is None or st.cache is not cache:
            st = self.cached_steps[key] = FusedMosiCachedStep(self.model, self.optimizer, self.loss_functions, n, cache,
                                                              patterns=pats, per_sample=pats is None)
        if st.log is not self.log:
            st.log, st.graph = self.log, None
        return st

    def cached_eval_step_for(self, n: int, cache, patterns=None):
        """The ``FusedMosiCachedEvalStep`` for (patterns, batch size) on ``cache`` (``patterns``: a ``"fused_patterns"``
        batch's; None: each row under its own keep flags)."""
        from .mosi import FusedMosiCachedEvalStep, norm_patterns
        pats = norm_patterns(patterns) if patterns is not None else None
        key = ("eval", pats, int(n))
        st = self.cached_steps.get(key)
        if st is None or st.cache is not cache:
            st = self.cached_steps[key] = FusedMosiCachedEvalStep(self.model, self.loss_functions, n, cache, self.log,
                                                                  patterns=pats, per_sample=pats is None)
        st.log = self.log
        return st

    def _cache_of(self, b: Dict[str, Any]):
        """An ``ids_only`` batch's cache: its dataset's ``embedding_cache(model, pad_to)``, looked up once per epoch
        (a dataset without one gets it here, a fill pass inside the epoch's first batch)."""
        ds = b["dataset"]
        key = (id(ds), b["steps"])
        cache = self._epoch_caches.get(key)
        if cache is None:
            cache = self._epoch_caches[key] = ds.embedding_cache(self.model, pad_to=b["pad_to"])
        return cache

    def _cached_step_of(self, b: Dict[str, Any], train: bool):
        pats = b["patterns"] if (b.get("all_patterns") or b.get("fused_patterns")) else None
        step_for = self.cached_train_step_for if train else self.cached_eval_step_for
        return step_for(int(b["rows"].numel()), self._cache_of(b), pats)

    def _train_step_of(self, b: Dict[str, Any]):
        """The train step a batch asks for: the cached step for an ``"ids_only"`` batch, the all-pattern step for an
        ``"all_patterns"`` batch, else the plain one."""
        if b.get("ids_only"):
            return self._cached_step_of(b, True)
        if b.get("all_patterns"):
            return self.train_pattern_step_for(*self._shape(b), patterns=b["patterns"], **self._modes(b))
        return self.train_step_for(*self._shape(b), **self._modes(b))

    def _eval_step_of(self, b: Dict[str, Any]):
        """The eval step a batch asks for: the cached step for an ``"ids_only"`` batch, the fused-pattern step for a
        ``"fused_patterns"`` batch, else the per-pattern one."""
        if b.get("ids_only"):
            return self._cached_step_of(b, False)
        if b.get("fused_patterns"):
            return self.pattern_eval_step_for(*self._shape(b), patterns=b["patterns"], **self._modes(b))
        return self.eval_step_for(*self._shape(b), **self._modes(b))

    def _run(self, st, b: Dict[str, Any]) -> None:
        if b.get("ids_only"):  # sample indices on a UttEmbeddingCache: no inputs, no lengths
            if st.per_sample:
                st.step(b["rows"], b["row_keep"], self.log.group_ids(b["pattern_name"]))
            else:
                st.step(b["rows"])
            return
        if b.get("fused_patterns") or b.get("all_patterns"):  # the step expands labels and group ids on the device
            if b.get("time_major") and b["audio"] is st.eng.A:
                st.run()
            else:
                st.step(b["audio"], b["video"], b["text"], b["label"], b.get("lengths"))
            return
        st.eng.groups.copy_(self.log.group_ids(b.get("pattern_name") or b["pattern_names"]), non_blocking=True)
        if b.get("time_major") and b["audio"] is st.eng.A:
            st.run()  # the gather wrote the inputs (and, for a ragged step, the length buffers) in place
        elif st.ragged or st.text_lengths:
            st.step(b["audio"], b["video"], b["text"], b["label"], b.get("lengths"))
        else:
            st.step(b["audio"], b["video"], b["text"], b["label"])

    @staticmethod
    def _shape(b: Dict[str, Any]) -> Tuple[int, Any]:
        """(rows, steps): the batch's own ``"steps"`` (an ``int``, or the (Ta, Tv, Tt) triple of an unaligned batch) or,
        for a batch-first batch without it, each modality's length read from its own tensor."""
        from .mosi import norm_steps
        steps = b.get("steps") or tuple(int(b[m].shape[1]) for m in ("audio", "video", "text"))
        return int(b["label"].numel()), norm_steps(steps)

    @staticmethod
    def _modes(b: Dict[str, Any]) -> Dict[str, bool]:
        """The step modes a batch asks for: ``ragged`` when it carries lengths, ``text_lengths`` when the text's too."""
        lengths = b.get("lengths")
        return dict(ragged=lengths is not None, text_lengths=isinstance(lengths, dict) and "text" in lengths)

    @staticmethod
    def _groups(b: Dict[str, Any]):
        if "label" in b or b.get("ids_only"):
            return [b]
        return list(b.values())  # {pattern: sub-batch}

    def _finish(self, t0: float):
        conf, losses, _ = self.log.fetch()  # the epoch's only host synchronisation
        mean = ClassificationLog.mean_loss(losses)
        if self.regression:
            metrics = self.recorder.calculate_metrics_for_group("regression", loss=mean, records=conf)
        else:
            metrics = self.recorder.calculate_metrics_for_group("classification", loss=mean, conf=conf)
        return mean, time.time() - t0, metrics, len(losses)

    def train_epoch(self, loader: Iterable[Dict[str, Any]]):
        """→ (mean batch loss, seconds, metrics dict, batches)."""
        self.log.reset()
        self._epoch_caches = {}
        t0 = time.time()
        for b in self.loader_for(loader, True):
            for g in self._groups(b):
                self._run(self._train_step_of(g), g)
        return self._finish(t0)

    @torch.no_grad()
    def validate_epoch(self, loader: Iterable[Dict[str, Any]]):
        self.log.reset()
        self._epoch_caches = {}
        t0 = time.time()
        self.model.eval()
        try:
            for b in self.loader_for(loader, False):
                for g in self._groups(b):
                    self._run(self._eval_step_of(g), g)
        finally:
            self.model.train()
        return self._finish(t0)


def _cached_mosi_loaders(model, loaders: Dict[str, Any]):
    """fit(cache_embeddings=True) on a UTT-Fusion model: the ``ids_only`` twin of every ``MosiDeviceLoader`` (the same
    ``epoch`` counter, hence the same shuffles) and one filled ``UttEmbeddingCache`` per split."""
    from .mosi import ALL_FROZEN, frozen_encoders
    from .mosi_data import MosiDeviceLoader
    if frozen_encoders(model) != ALL_FROZEN:
        raise L.TspmError("cache_embeddings=True needs frozen encoders - all of netA, netV and netT (finetune_param_groups("
                          "..., freeze=('audio', 'video', 'text'))): a trainable encoder's outputs change every step, so "
                          "there is nothing constant to cache")
    out, report = {}, {"fill_seconds": {}, "rows": {}}
    for name, ld in loaders.items():
        if not isinstance(ld, MosiDeviceLoader):
            raise L.TspmError(f"cache_embeddings=True: loaders[{name!r}] must be a mosi_data.MosiDeviceLoader "
                              f"(dataset.loader(...)), got {type(ld).__name__}")
        twin = ld if ld.ids_only else MosiDeviceLoader(ld.ds, ld.batch_size, ld.shuffle, ld.drop_last, ld.seed, None,
                                                      ld.pad_to, ld.group_patterns, ld.fuse_patterns, ld.all_patterns,
                                                      ids_only=True)
        twin.epoch = ld.epoch
        cache = ld.ds.embedding_cache(model, pad_to=ld.pad_to)
        if cache.stale_reason() is not None:
            cache.refresh()
        report["fill_seconds"][name], report["rows"][name] = cache.fill_seconds, cache.n
        out[name] = twin
    print("embedding cache filled: " + ", ".join(f"{k} {report['rows'][k]} rows in {v:.3f} s"
                                                 for k, v in report["fill_seconds"].items()))
    return out, report


def runner_for(model, optimizer, loss_functions, metric_config=None):
    """The epoch runner of the model family: AVMNIST late fusion, or MOSI / MOSEI UTT-Fusion."""
    from .mosi import UttFusionModel
    if isinstance(model, UttFusionModel):
        return MosiEpochRunner(model, optimizer, loss_functions, metric_config)
    return EpochRunner(model, optimizer, loss_functions, metric_config)


def _epoch_block(loss: float, timing: float, n_batches: int, metrics: Dict[str, Any]) -> Dict[str, Any]:
    """One split's entry of epoch_metrics.json (train_multimodal.py:627-718)."""
    out: Dict[str, Any] = {"loss": loss, "timing": {"total_time": timing,
                                                    "avg_batch_time": timing / max(1, n_batches)}}
    for key, value in metrics.items():
        if key == "loss" or not isinstance(value, (int, float)):
            continue
        if key.startswith("f1_") and "_" in key:
            parts = key.split("_")
            name = parts[0] + "_" + parts[1]
            mod = parts[2] if len(parts) >= 3 else "IT"
            out.setdefault(mod, {})[name] = metrics[key]
        else:
            out.setdefault("metrics", {})[key] = value
    return out


def fit(model, optimizer, loss_functions, loaders: Dict[str, Any], epochs: int, *, metric_config=None,
        early_stopping: bool = True, patience: int = 10, min_delta: float = 1e-3, scheduler=None,
        checkpoint_dir=None, metrics_path=None, save_metric: str = "loss", mode: str = "minimize",
        on_epoch=None, fail_on_nonfinite: bool = True, cache_embeddings: bool = False,
        steps_per_call: Optional[int] = None) -> Dict[str, Any]:
    """_train_loop + test (train_multimodal.py:554-917) for the AVMNIST late-fusion model and the MOSI / MOSEI
    UTT-Fusion model (``runner_for``; its loaders: ``mosi_data.MOSI.loader(...)``).  ``loaders``:
    "train", "validation" and optionally "test" → iterables of device batches (a DeviceLoader is
    re-iterated each epoch; call ``set_epoch`` in ``on_epoch`` for DistributedSampler order).
    ``fail_on_nonfinite``: raise FloatingPointError as soon as an epoch's mean training loss is NaN / inf
    (checked at the epoch's one host synchronisation; SURVEY §5 — the reference only turns three numpy
    RuntimeWarnings into errors, train_multimodal.py:46-60, and would keep training on NaN weights).
    ``cache_embeddings`` (AVMNIST on frozen encoders with ``data.DeviceLoader`` loaders, or UTT-Fusion with all three
    encoders frozen and ``mosi_data.MosiDeviceLoader`` loaders - ``steps_per_call`` is not built for it; refused otherwise): before the
    first epoch each split's ``embedding_cache(model)`` is filled once, and every epoch then iterates the ``ids_only``
    twin of its loader — no encoder launch after the fill; metric keys and loss entries per epoch are unchanged.  The
    fill times are reported once under ``history["embedding_cache"]``.  When the best checkpoint is reloaded for the test
    split only the test split's cache is refreshed: the train and validation caches are left stale, and whoever reuses
    those datasets with the model afterwards calls ``refresh()`` on them (``embedding_cache(model, refresh=True)``).
    ``steps_per_call=K`` (with ``cache_embeddings`` only; refused without): every train, validation and test epoch runs
    K consecutive batches per host call (``EpochRunner.train_epoch(loader, steps_per_call=K)``) — the same history."""
    if steps_per_call is not None and not cache_embeddings:
        raise L.TspmError("steps_per_call runs several cached batches per host call: it needs cache_embeddings=True")
    runner = runner_for(model, optimizer, loss_functions, metric_config)
    if steps_per_call is not None and isinstance(runner, MosiEpochRunner):
        raise L.TspmError("steps_per_call is not built for the UTT-Fusion model: its cached head stage runs one step per "
                          "graph replay")
    cache_report = None
    spc = {"steps_per_call": steps_per_call} if steps_per_call is not None else {}
    if cache_embeddings:
        loaders, cache_report = _cached_loaders(model, optimizer, runner, loaders)
    if getattr(runner, "regression", False) and save_metric != "loss":
        raise ValueError(f"save_metric {save_metric!r}: a regression run selects its best epoch by the loss; only "
                         "save_metric='loss' is supported")
    ckpt = CheckpointManager(checkpoint_dir, save_metric, mode) if checkpoint_dir is not None else None
    history: Dict[str, Any] = {"train": [], "validation": [], "epoch_metrics": []}
    best, wait = None, 0
    mfile = Path(metrics_path) / "epoch_metrics.json" if metrics_path is not None else None
    if mfile is not None:
        mfile.parent.mkdir(parents=True, exist_ok=True)
    for epoch in range(1, epochs + 1):
        if on_epoch is not None:
            on_epoch(epoch)
        tr_loss, tr_time, tr_metrics, tr_n = runner.train_epoch(loaders["train"], **spc)
        if fail_on_nonfinite and not np.isfinite(tr_loss):
            raise FloatingPointError(f"non-finite mean training loss {tr_loss} at epoch {epoch}")
        tr_metrics = dict(tr_metrics, loss=tr_loss)
        va_loss, va_time, va_metrics, va_n = runner.validate_epoch(loaders["validation"], **spc)
        va_metrics = dict(va_metrics, loss=va_loss)
        history["train"].append(tr_metrics)
        history["validation"].append(va_metrics)
        history["epoch_metrics"].append({"epoch": epoch, "train": _epoch_block(tr_loss, tr_time, tr_n, tr_metrics),
                                         "validation": _epoch_block(va_loss, va_time, va_n, va_metrics)})
        if mfile is not None:
            with open(mfile, "w") as f:
                json.dump(history["epoch_metrics"], f, indent=4, default=lambda o: np.asarray(o).tolist())
        is_best, cont, wait = check_early_stopping(va_metrics, best, patience, min_delta, wait, mode, save_metric)
        if is_best:
            best = dict(va_metrics)
            if ckpt is not None:
                ckpt.save_checkpoint(model, optimizer, scheduler, epoch, va_metrics, is_best=True)
        if early_stopping and not cont:
            break
        if scheduler is not None:
            if isinstance(scheduler, torch.optim.lr_scheduler.ReduceLROnPlateau):
                scheduler.step(va_metrics["loss"])
            else:
                scheduler.step()
    if "test" in loaders:
        if ckpt is not None and (ckpt.model_dir / "best.pth").exists():
            ckpt.load_checkpoint(model, load_best=True)
            if cache_embeddings:  # load_state_dict made the caches stale (the loaded encoders may differ)
                ld = loaders["test"]
                if isinstance(runner, MosiEpochRunner):  # a UTT-Fusion cache is per (model, steps): the loader's pad_to
                    ld.ds.embedding_cache(model, pad_to=ld.pad_to, refresh=True)
                else:
                    ld.ds.embedding_cache(model, refresh=True)
        te_loss, te_time, te_metrics, _ = runner.validate_epoch(loaders["test"], **spc)
        history["test"] = dict(te_metrics, loss=te_loss)
    history["best"] = best
    if cache_report is not None:
        history["embedding_cache"] = cache_report
    return history


def _cached_loaders(model, optimizer, runner, loaders: Dict[str, Any]):
    """fit(cache_embeddings=True): the ``ids_only`` twin of every loader and one filled cache per split."""
    from .data import DeviceLoader
    if isinstance(runner, MosiEpochRunner):
        return _cached_mosi_loaders(model, loaders)
    if not isinstance(runner, EpochRunner):
        raise L.TspmError("cache_embeddings=True is for the AVMNIST late-fusion model")
    if not head_stage_frozen(model, optimizer):
        raise L.TspmError("cache_embeddings=True needs frozen encoders (AVMNIST.freeze_encoders()): a trainable "
                          "encoder's embeddings change every step, so there is nothing constant to cache")
    out, report = {}, {"fill_seconds": {}, "rows": {}}
    for name, ld in loaders.items():
        if not isinstance(ld, DeviceLoader):
            raise L.TspmError(f"cache_embeddings=True: loaders[{name!r}] must be a data.DeviceLoader "
                              f"(dataset.device_loader(...)), got {type(ld).__name__}")
        twin = ld if ld.ids_only else DeviceLoader(
            ld.ds, ld.batch_size, ld.shuffle, ld.drop_last, ld.generator, rank=ld.rank, world_size=ld.world_size,
            distributed=ld.distributed, seed=ld.seed, pattern=ld.pattern, fuse_patterns=ld.fuse_patterns,
            all_patterns=ld.all_patterns, ids_only=True)
        twin.epoch = ld.epoch
        cache = ld.ds.embedding_cache(model)
        if cache.stale_reason() is not None:
            cache.refresh()
        report["fill_seconds"][name], report["rows"][name] = cache.fill_seconds, cache.n
        out[name] = twin
    print("embedding cache filled: " + ", ".join(f"{k} {report['rows'][k]} rows in {v:.3f} s"
                                                 for k, v in report["fill_seconds"].items()))
    return out, report
