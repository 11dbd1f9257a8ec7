"""Monomodal encoder pre-training on the HIP path (BASELINE.json configs[1]:
ResNet18 audio encoder, batch 256, one MI355X).

Drop-in for ``MonomodalEncoder`` of MML_Suite/train_monomodal.py:64-418 — the wrapper that
train_monomodal.py builds around the YAML's encoder (``!ResNet18`` audio / ``!ResNet34`` image,
configs/avmnist/mono/train_{audio,image}_encoder_resnet.yaml) with ``classifier = nn.Linear(output_dim,
num_classes)``.  The best encoder's ``state_dict`` is saved as ``encoder_{modality}_best.pth``, the file the
pretrained late-fusion config loads (train_monomodal.py:789-802, train_multimodal.py:156-204).

* :class:`MonomodalEncoder` — same constructor, attribute names (``encoder``, ``classifier``),
  ``state_dict`` keys, ``forward`` / ``get_encoder`` / ``train_step`` / ``validation_step`` signatures and
  return dicts (``{"loss", "metrics": {"loss", "accuracy"}}``) as the reference.
* :class:`FusedMonoStep` — ``train_step`` as one HIP graph: encoder forward (libtspm schedule) →
  classifier → cross-entropy → classifier backward → encoder backward → FusedAdam, with the
  ``argmax(logits, 1)`` predictions written on the device (``tspm_classify_update_ex``, logits mode).
* :class:`FusedMonoEvalStep` — ``validation_step`` as one HIP graph (eval-mode BatchNorm).
* :class:`FusedMosiMonoStep` / :class:`FusedMosiMonoEvalStep` — the same two steps around a MOSI / MOSEI
  encoder (``mosi.LSTMEncoder`` "last" / "maxpool", ``mosi.TextCNN``; the reference's ``configs/mosi/mono/``
  pre-training): encoder forward (``mosi.MosiEncoderEngine``) → ``tspm_mono_head_step`` (classifier, CE,
  predictions and the classifier's backward in one launch; ``fused_head=False`` keeps the four separate
  launches) → encoder backward → FusedAdam.  Learning rate, weight decay and batch size are the caller's
  optimizer and loader arguments.  Under a one-output classifier with a single mean L1 / MSE term (float32
  sentiment scores) the head is ``tspm_regress_head_step`` and the epoch log a ``metrics.RegressionLog``.
* :class:`FusedMMIMDbMonoStep` / :class:`FusedMMIMDbMonoEvalStep` — the same two steps around an MMIMDb encoder
  (``mmimdb.MMIMDbModalityEncoder``: BatchNorm1d → Linear) under the multi-label classifier: ``tspm_bn1d_fwd`` →
  ``tspm_linear_fwd`` → the head (``tspm_mono_head_bce_step``, or ``fused_head=False``: ``tspm_linear_fwd``,
  ``tspm_bce_logits``, ``tspm_linear_bwd``) → encoder Linear backward → ``tspm_bn1d_bwd`` → FusedAdam.
* :func:`select_modality_key` — the reference's choice of the batch key (train_monomodal.py:103-128).
* :class:`MonoEpochRunner` / :func:`fit_monomodal` — the epoch loop of ``train_monomodal``
  (train_monomodal.py:536-884) on those steps, one host read per epoch.
"""
from __future__ import annotations

import ctypes
import math
import os
import time
from pathlib import Path
from typing import Any, Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from ._lib import linear_bwd
from .engine import EncoderEngine, prepare_encoder_layout
from .metrics import ClassificationLog, DeviceMetricRecorder, RegressionLog, RegressionMetricRecorder
from .optim import FusedAdam
from .step import _ce_weight, shared_batches_tracked

ARGMAX_LOGITS = 1  # TSPM_ARGMAX_LOGITS (include/tspm.h)
# keys train_monomodal.py:110-112 never treats as a modality (+ this package's device pattern index
# and mosi_data's loader bookkeeping)
_RESERVED = ("labels", "label", "genres", "imdb_ids", "pattern_name", "missing_masks", "sample_idx", "pattern_ids",
             "steps", "time_major", "pattern_names", "lengths")
# MonomodalEncoder(fused_head=...) default for MOSI encoders: tspm_mono_head_step against the four separate launches,
# graph-replayed at B=128, T=50 (scripts/bench_mosi_mono.py, profiles/mosi_mono_head_ab.json)
FUSED_HEAD_DEFAULT = True
# ... and for MMIMDb encoders: tspm_mono_head_bce_step against tspm_linear_fwd + tspm_bce_logits + tspm_linear_bwd,
# graph-replayed at B = 128 / 256, image and text (scripts/bench_mmimdb_mono.py, profiles/mmimdb_mono_head_ab.json;
# DESIGN.md §7): faster beyond the spread at 256 in both cases, not at 128
FUSED_BCE_HEAD_MIN_BATCH = 256  # fused_head=None: the head kernel from this batch size up, the separate launches below
BCE_HEAD_MAX_N, BCE_HEAD_MAX_HID, BCE_HEAD_MAX_CLASSES = 1024, 512, 32  # tspm_mono_head_bce_step's limits


def _exp_name(config) -> str:
    if isinstance(config, str):
        return config
    exp = getattr(config, "experiment", None)
    return str(getattr(exp, "name", "") or "")


def select_modality_key(batch: Dict[Any, Any], experiment_name: str = ""):
    """train_monomodal.py:103-128: skip the bookkeeping keys; with "AVMNIST_Image_Encoder" /
    "AVMNIST_Audio_Encoder" in the experiment name take the first key whose ``str`` names IMAGE /
    AUDIO, otherwise the LAST remaining key.  ``str(Modality.X)`` comes from the un-vendored
    ``modalities`` package (unpinned), so the name test is case-insensitive here."""
    key = None
    for k in batch.keys():
        ks = str(k)
        if ks in _RESERVED or ks.endswith("_missing_index") or ks.endswith("_reverse"):
            continue
        up = ks.upper()
        if "AVMNIST_Image_Encoder" in experiment_name and "IMAGE" in up:
            return k
        if "AVMNIST_Audio_Encoder" in experiment_name and "AUDIO" in up:
            return k
        key = k
    if key is None:
        raise ValueError(f"No modality data found in batch. Available keys: {list(batch.keys())}")
    return key


def _as_tensor(raw) -> torch.Tensor:
    """train_monomodal.py:137-191: a tensor, or a list of tensors / numbers / arrays (stacked).  Lists
    of file paths are not taken: load the corpus with tspm_amd.data.AVMNIST (HBM-resident)."""
    if torch.is_tensor(raw):
        return raw
    if isinstance(raw, list):
        if raw and isinstance(raw[0], str):
            raise L.TspmError("file-path batches: load the corpus with tspm_amd.data.AVMNIST instead")
        items = []
        for it in raw:
            if torch.is_tensor(it):
                items.append(it)
            elif isinstance(it, (int, float)):
                items.append(torch.tensor(it))
            elif isinstance(it, np.ndarray):
                items.append(torch.from_numpy(it))
            else:
                raise TypeError(f"Unsupported data type: {type(it)}")
        return torch.stack(items)
    raise TypeError(f"Unsupported modality data type: {type(raw)}")


def _labels_of(batch: Dict[Any, Any]) -> torch.Tensor:
    """train_monomodal.py:196-219."""
    for k in ("label", "labels", "genres"):
        if k in batch:
            raw = batch[k]
            if isinstance(raw, list):
                if raw and isinstance(raw[0], str):
                    raise TypeError("Cannot convert string labels to tensor without label mapping")
                return torch.tensor(raw)
            return raw
    raise ValueError(f"No labels found in batch. Available keys: {list(batch.keys())}")


def _device_log(metric_recorder) -> Optional[ClassificationLog]:
    return metric_recorder.log if isinstance(metric_recorder, (DeviceMetricRecorder, RegressionMetricRecorder)) else None


def _mono_regress(model, loss_functions):
    """(kind, weight) of the loss group's single mean L1 / MSE term (``mosi._regress_term``) when ``model`` wraps a
    MOSI / MOSEI encoder under a one-output classifier — the sentiment-regression pre-training — else None."""
    if not model._mosi_encoder() or model.classifier.out_features != 1:
        return None
    from .mosi import _regress_term
    return _regress_term(loss_functions)


def _loss_sig(model, loss_functions):
    """What a MOSI monomodal step bakes in from the loss group: (cross-entropy weight, regression term)."""
    return _ce_weight(loss_functions), _mono_regress(model, loss_functions)


class _LinearFn(torch.autograd.Function):
    """``classifier`` (nn.Linear) on libtspm: tspm_linear_fwd / _bwd_weight / _bwd_data."""

    @staticmethod
    def forward(ctx, x, w, b):
        n, fin = x.shape
        fout = w.shape[0]
        y = torch.empty(n, fout, device=x.device, dtype=torch.float32)
        L.check(L.lib().tspm_linear_fwd(n, fin, fout, x.data_ptr(), fin, w.data_ptr(), b.data_ptr(), 0, None, 1.0,
                                        y.data_ptr(), fout, L.stream_handle()), "classifier fwd")
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g = g.contiguous().float()
        n, fin = x.shape
        fout = w.shape[0]
        lib, sh = L.lib(), L.stream_handle()
        gw, gb, gx = torch.empty_like(w), torch.empty(fout, device=g.device), torch.empty_like(x)
        L.check(lib.tspm_linear_bwd_weight(n, fin, fout, x.data_ptr(), fin, g.data_ptr(), fout, gw.data_ptr(),
                                           gb.data_ptr(), sh), "classifier wgrad")
        L.check(lib.tspm_linear_bwd_data(n, fin, fout, g.data_ptr(), fout, w.data_ptr(), gx.data_ptr(), fin, sh),
                "classifier dgrad")
        return gx, gw, gb


class _MonoBuffers(L.GraphRunner):
    """Static device buffers shared by the fused train and eval steps, on the graph runner (key: the log)."""

    def _init_buffers(self, model, x_shape: Tuple[int, ...], log, batch: Optional[int] = None) -> None:
        enc, cls = model.encoder, model.classifier
        self.model, self.log = model, log
        dev = next(model.parameters()).device
        self.device = dev
        self.N = int(x_shape[0] if batch is None else batch)  # batch: the input buffer is time-major [T, B, F]
        self.hid, self.K = cls.in_features, cls.out_features
        hidden = enc.hidden_dim if hasattr(enc, "hidden_dim") else enc.hidden_size
        if self.hid != hidden:
            raise L.TspmError(f"classifier input {self.hid} != encoder hidden_dim {hidden}")
        f32 = dict(device=dev, dtype=torch.float32)
        self.X = torch.zeros(x_shape, **f32)
        self.labels = torch.zeros(self.N, dtype=torch.int64, device=dev)
        self.emb = torch.empty(self.N, self.hid, **f32)
        self.logits = torch.empty(self.N, self.K, **f32)
        self.loss = torch.zeros(1, **f32)
        self.preds = torch.zeros(self.N, dtype=torch.int64, device=dev)

    def _classify(self, lib, sh: int) -> None:
        log = self.log
        L.check(lib.tspm_classify_update_ex(
            self.N, self.K, self.logits.data_ptr(), self.labels.data_ptr(), None, len(log.groups) if log else 1,
            log.conf.data_ptr() if log else None, self.preds.data_ptr(), self.loss.data_ptr(),
            log.loss_log.data_ptr() if log else None, log.counters.data_ptr() if log else None,
            log.capacity if log else 0, ARGMAX_LOGITS, sh), "classify_update")

    def _replay_or_enqueue(self) -> None:
        self.replay_or_enqueue(self._enqueue, (self.log,))  # the metrics log is baked into the captured graph
        self.calls += 1

    def load_batch(self, x: torch.Tensor, labels: torch.Tensor) -> None:
        if x.data_ptr() != self.X.data_ptr():
            self.X.copy_(x.reshape(self.X.shape), non_blocking=True)
        if labels.data_ptr() != self.labels.data_ptr():
            self.labels.copy_(labels.reshape(-1), non_blocking=True)

    def batch_accuracy(self) -> torch.Tensor:
        """mean(pred == label) of the last batch, as a device scalar (no host synchronisation)."""
        return (self.preds == self.labels).float().mean()


class FusedMonoStep(_MonoBuffers):
    """MonomodalEncoder.train_step (train_monomodal.py:97-260) as one HIP graph:

        encoder fwd → classifier → CE → argmax(logits) → classifier bwd → encoder bwd → FusedAdam

    Weight gradients go straight into FusedAdam's flat gradient buffer (overwrite — no zero_grad
    pass).  ``_lib.GraphRunner``'s lifecycle: first call eager, second captures, later calls copy the batch
    into the static buffers (no copy when the caller gathered into them) and replay."""

    def __init__(self, model, optimizer: FusedAdam, loss_functions, x_shape, use_graph: bool = True, log=None):
        self.ce_weight = _ce_weight(loss_functions)
        if self.ce_weight is None:
            raise L.TspmError("FusedMonoStep: the loss group must be a single cross-entropy term")
        if not isinstance(optimizer, FusedAdam):
            raise L.TspmError("FusedMonoStep needs tspm_amd.FusedAdam")
        x_shape = tuple(int(v) for v in x_shape)
        self._init_buffers(model, x_shape, log)
        self.opt = optimizer
        self._init_graph(use_graph, self.device)
        model.train()
        prepare_encoder_layout(model.encoder)
        for p in model.parameters():
            if p.requires_grad and p.grad is None:
                raise L.TspmError("FusedMonoStep: parameter without a FusedAdam gradient view")
        self.eng = EncoderEngine(model.encoder, self.N, x_shape[-2], x_shape[-1], self.device)
        f32 = dict(device=self.device, dtype=torch.float32)
        self.dlogits = torch.empty(self.N, self.K, **f32)
        self.demb = torch.empty(self.N, self.hid, **f32)
        self.stats = torch.zeros(4, **f32)
        self.nbt = shared_batches_tracked(model, self.device)
        self._sig = (id(optimizer), id(loss_functions), x_shape)

    def matches(self, x: torch.Tensor, optimizer, loss_functions) -> bool:
        return self._sig == (id(optimizer), id(loss_functions), tuple(x.shape))

    def _enqueue(self) -> None:
        lib = L.lib()
        sh = torch.cuda.current_stream().cuda_stream
        n, hid, K = self.N, self.hid, self.K
        cls = self.model.classifier
        self.eng.forward(self.X, self.emb, hid, train=True, bump_batches_tracked=False)
        L.check(lib.tspm_linear_fwd(n, hid, K, self.emb.data_ptr(), hid, cls.weight.data_ptr(), cls.bias.data_ptr(), 0,
                                    None, 1.0, self.logits.data_ptr(), K, sh), "classifier fwd")
        L.check(lib.tspm_cross_entropy(n, K, self.logits.data_ptr(), self.labels.data_ptr(), self.loss.data_ptr(),
                                       self.dlogits.data_ptr(), self.ce_weight, self.stats.data_ptr(), sh),
                "cross_entropy")
        self._classify(lib, sh)
        linear_bwd(n, hid, K, self.emb.data_ptr(), hid, self.dlogits.data_ptr(), K, cls.weight.data_ptr(),
                   cls.weight.grad.data_ptr(), cls.bias.grad.data_ptr(), self.demb.data_ptr(), hid, sh)
        self.eng.backward(self.demb, hid)
        L.counters_add(self.nbt)
        self.opt.launch(sh)

    def run(self) -> None:
        """One training step on the batch in the static input buffers."""
        self.model.train()
        self.opt.sync_hyper()
        self._replay_or_enqueue()
        self.opt.note_steps(1)

    def step(self, x: torch.Tensor, labels: torch.Tensor) -> Dict[str, torch.Tensor]:
        self.load_batch(x, labels)
        self.run()
        return {"loss": self.loss, "logits": self.logits, "preds": self.preds}


class FusedMonoEvalStep(_MonoBuffers):
    """MonomodalEncoder.validation_step (train_monomodal.py:262-418) as one HIP graph: eval-mode
    encoder forward (BatchNorm running statistics), classifier, weighted CE, argmax(logits)."""

    def __init__(self, model, loss_functions, x_shape, log=None, use_graph: bool = True):
        self.ce_weight = _ce_weight(loss_functions)
        if self.ce_weight is None:
            raise L.TspmError("FusedMonoEvalStep: the loss group must be a single cross-entropy term")
        x_shape = tuple(int(v) for v in x_shape)
        self._init_buffers(model, x_shape, log)
        self._init_graph(use_graph, self.device)
        self.eng = model.encoder.engine_for(self.X)

    def _enqueue(self) -> None:
        lib = L.lib()
        sh = torch.cuda.current_stream().cuda_stream
        n, hid, K = self.N, self.hid, self.K
        cls = self.model.classifier
        self.eng.forward(self.X, self.emb, hid, train=False)
        L.check(lib.tspm_linear_fwd(n, hid, K, self.emb.data_ptr(), hid, cls.weight.data_ptr(), cls.bias.data_ptr(), 0,
                                    None, 1.0, self.logits.data_ptr(), K, sh), "eval classifier")
        L.check(lib.tspm_cross_entropy(n, K, self.logits.data_ptr(), self.labels.data_ptr(), self.loss.data_ptr(),
                                       None, self.ce_weight, None, sh), "eval cross_entropy")
        self._classify(lib, sh)

    def run(self) -> None:
        self.model.eval()
        self._replay_or_enqueue()

    def step(self, x: torch.Tensor, labels: torch.Tensor) -> Dict[str, torch.Tensor]:
        self.load_batch(x, labels)
        self.run()
        return {"loss": self.loss, "logits": self.logits, "preds": self.preds}


def _len_tag(ragged: bool, text_lengths: bool = False) -> tuple:
    """The trailing cache-key elements of the per-sample-length modes (``ragged``: an LSTMEncoder's, ``text_lengths``: a
    TextCNN's); empty — the key as it always was — with both off."""
    return (("ragged",) if ragged else ()) + (("text_lengths",) if text_lengths else ())


class _MosiMonoBuffers(_MonoBuffers):
    """What the MOSI-encoder train and eval steps share: the single-encoder engine on the step's time-major
    input buffer, and the head — ``tspm_mono_head_step`` or the separate launches."""

    def _init_mosi(self, model, x_shape, log, fused_head: Optional[bool], ragged: bool = False,
                   text_lengths: bool = False) -> None:
        from .mosi import MosiEncoderEngine
        b, t, f = (int(v) for v in x_shape)
        if f != model.encoder.input_size:
            raise L.TspmError(f"input features {f} != encoder input_size {model.encoder.input_size}")
        self._init_buffers(model, (t, b, f), log, batch=b)
        self.T = t
        self.labels_f = torch.zeros(self.N, dtype=torch.float32, device=self.device)  # the regression head's labels
        if self.regress is not None and not L.regress_head_supported(self.N, self.hid):
            raise L.TspmError("the regression head takes at most 1024 rows and an encoder of at most 128 units, a "
                              "multiple of 4")
        self.fused_head = bool(model.fused_head if fused_head is None else fused_head)
        self.ragged = bool(ragged)  # per-sample lengths: the LSTM recurrences read the engine's length buffer
        self.text_lengths = bool(text_lengths)  # ... a TextCNN's pooling reads the engine's text length buffer
        self.eng = MosiEncoderEngine(model.encoder, b, t, self.device, seed=model._rng_seed, x=self.X, emb=self.emb,
                                     ragged=self.ragged, text_lengths=self.text_lengths)
        if self.regress is not None:
            self.preds = self.logits.view(-1)  # the float predictions
        self.demb = self.eng.demb
        model._by_buffer[self.X.data_ptr()] = self

    @property
    def keep_override(self):
        return self.eng.keep_override

    @keep_override.setter
    def keep_override(self, v):
        self.eng.keep_override = v

    def load_batch(self, x: torch.Tensor, labels: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> None:
        """x: a batch-first [B, T, F] batch (one tspm_seq_gather into the time-major buffer), or the step's own
        input buffer (mosi_data.MOSI.device_loader(step_for=...) gathered into it: no copy).  ``lengths`` (a ragged
        or text_lengths step): int [B], copied on the device into the engine's length buffer (or that buffer itself: no
        copy)."""
        if x.data_ptr() != self.X.data_ptr():
            self.eng.load(x)
        self.eng.set_lengths(lengths)
        dst = self.labels_f if self.regress is not None else self.labels  # by the step's mode, cast to its type
        if labels.data_ptr() != dst.data_ptr():
            dst.copy_(labels.reshape(-1), non_blocking=True)

    def _head_regress(self, lib, sh: int, train: bool) -> None:
        """``tspm_regress_head_step``: classifier Linear(hid, 1), the weighted L1 / MSE loss against ``labels_f``, the
        epoch accumulators and loss log of ``log`` (a RegressionLog of one group) and, with ``train``, the
        classifier's backward — the only head of this mode (``fused_head`` is ignored)."""
        cls, log = self.model.classifier, self.log
        if log is not None and not isinstance(log, RegressionLog):
            raise L.TspmError("the regression head records into a metrics.RegressionLog")
        d = L.RegressHeadDesc(n=self.N, hid=self.hid, ld_emb=self.hid, ld_demb=self.hid, kind=self.regress[0],
                              n_groups=1, loss_weight=self.regress[1])
        d.emb, d.w, d.b = self.emb.data_ptr(), cls.weight.data_ptr(), cls.bias.data_ptr()
        d.labels, d.pred, d.loss = self.labels_f.data_ptr(), self.logits.data_ptr(), self.loss.data_ptr()
        if train:
            d.dw, d.db, d.demb = cls.weight.grad.data_ptr(), cls.bias.grad.data_ptr(), self.demb.data_ptr()
        if log is not None:
            d.n_groups, d.stats = len(log.groups), log.records.data_ptr()
            d.loss_log, d.counters, d.log_capacity = log.loss_log.data_ptr(), log.counters.data_ptr(), log.capacity
        L.check(lib.tspm_regress_head_step(ctypes.byref(d), sh), "regress_head_step")

    def _head(self, lib, sh: int, train: bool) -> None:
        n, hid, K = self.N, self.hid, self.K
        cls = self.model.classifier
        if self.regress is not None:
            self._head_regress(lib, sh, train)
            return
        if self.fused_head:
            d = L.MonoHeadDesc()
            d.n, d.hid, d.classes, d.ld_emb, d.ld_demb, d.loss_weight = n, hid, K, hid, hid, self.ce_weight
            d.emb, d.w, d.b = self.emb.data_ptr(), cls.weight.data_ptr(), cls.bias.data_ptr()
            d.labels, d.logits, d.loss = self.labels.data_ptr(), self.logits.data_ptr(), self.loss.data_ptr()
            d.preds = self.preds.data_ptr()
            if train:
                d.dw, d.db, d.demb = cls.weight.grad.data_ptr(), cls.bias.grad.data_ptr(), self.demb.data_ptr()
                d.stats = self.stats.data_ptr()
            L.check(lib.tspm_mono_head_step(ctypes.byref(d), sh), "mono_head_step")
            if self.log is not None:  # the epoch's confusion counts and loss log
                self._classify(lib, sh)
            return
        L.check(lib.tspm_linear_fwd(n, hid, K, self.emb.data_ptr(), hid, cls.weight.data_ptr(), cls.bias.data_ptr(), 0,
                                    None, 1.0, self.logits.data_ptr(), K, sh), "classifier fwd")
        L.check(lib.tspm_cross_entropy(n, K, self.logits.data_ptr(), self.labels.data_ptr(), self.loss.data_ptr(),
                                       self.dlogits.data_ptr() if train else None, self.ce_weight,
                                       self.stats.data_ptr() if train else None, sh), "cross_entropy")
        self._classify(lib, sh)
        if train:
            linear_bwd(n, hid, K, self.emb.data_ptr(), hid, self.dlogits.data_ptr(), K, cls.weight.data_ptr(),
                       cls.weight.grad.data_ptr(), cls.bias.grad.data_ptr(), self.demb.data_ptr(), hid, sh)

    def matches_shape(self, x: torch.Tensor) -> bool:
        return x.data_ptr() == self.X.data_ptr() or tuple(x.shape) == (self.N, self.T, self.X.shape[2])


class FusedMosiMonoStep(_MosiMonoBuffers):
    """MonomodalEncoder.train_step around a MOSI encoder as one HIP graph:

        encoder fwd → tspm_mono_head_step (classifier, CE, argmax, classifier bwd) → encoder bwd → FusedAdam

    ``x_shape`` is the batch-first (B, T, F).  Gradients go straight into FusedAdam's flat views (overwritten);
    no gradient clip (MonomodalEncoder.train_step has none).  The TextCNN's dropout masks are drawn by
    ``tspm_dropout_mask`` on the optimizer's step counter (``keep_override = {"text": mask}`` injects one).  First
    call eager, second captures, later calls replay.

    Regression mode — ``classifier.out_features == 1`` with a single mean L1 / MSE term (float32 sentiment scores):
    the head is ``tspm_regress_head_step`` only.  There is no separate-launch variant to choose from, so
    ``fused_head`` is ignored in this mode; ``preds`` is then the float prediction [B] (a view of ``logits``)."""

    def __init__(self, model, optimizer: FusedAdam, loss_functions, x_shape, use_graph: bool = True, log=None,
                 fused_head: Optional[bool] = None, ragged: bool = False, text_lengths: bool = False):
        self.ce_weight, self.regress = _loss_sig(model, loss_functions)
        if self.ce_weight is None and self.regress is None:
            raise L.TspmError("FusedMosiMonoStep: the loss group must be a single cross-entropy term (or, under a "
                              "one-output classifier, a single mean L1 / MSE term)")
        if not isinstance(optimizer, FusedAdam):
            raise L.TspmError("FusedMosiMonoStep needs tspm_amd.FusedAdam")
        model.train()
        for p in model.parameters():
            if p.requires_grad and p.grad is None:
                raise L.TspmError("FusedMosiMonoStep: parameter without a FusedAdam gradient view")
        self._init_mosi(model, x_shape, log, fused_head, ragged, text_lengths)
        self.opt = optimizer
        self._init_graph(use_graph, self.device)
        self.eng.rng_ctr_ptr = optimizer.flat_groups()[0].hyper.data_ptr() + L.HYPER_STEP_OFFSET
        f32 = dict(device=self.device, dtype=torch.float32)
        self.dlogits = torch.empty(self.N, self.K, **f32)
        self.stats = torch.zeros(4, **f32)
        self._sig = (id(optimizer), id(loss_functions), self.fused_head) + _len_tag(self.ragged, self.text_lengths)

    def matches(self, x: torch.Tensor, optimizer, loss_functions, fused_head: Optional[bool] = None,
                ragged: bool = False, text_lengths: bool = False) -> bool:
        fh = bool(self.model.fused_head if fused_head is None else fused_head)
        sig = (id(optimizer), id(loss_functions), fh) + _len_tag(ragged, text_lengths)
        return self._sig == sig and self.matches_shape(x)

    def _enqueue(self) -> None:
        lib = L.lib()
        sh = torch.cuda.current_stream().cuda_stream
        self.eng.forward(sh, True)
        self._head(lib, sh, True)
        self.eng.backward(sh)
        self.opt.launch(sh)

    def run(self) -> None:
        """One training step on the batch in the static input buffers."""
        self.model.train()
        self.opt.sync_hyper()
        self.eng.apply_keep_override()
        self._replay_or_enqueue()
        self.opt.note_steps(1)

    def step(self, x: torch.Tensor, labels: torch.Tensor,
             lengths: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        self.load_batch(x, labels, lengths)
        self.run()
        return {"loss": self.loss, "logits": self.logits, "preds": self.preds}


class FusedMosiMonoEvalStep(_MosiMonoBuffers):
    """MonomodalEncoder.validation_step around a MOSI encoder as one HIP graph: eval-mode encoder forward (no
    dropout) and the head in forward-only mode (logits, weighted CE, argmax)."""

    def __init__(self, model, loss_functions, x_shape, log=None, use_graph: bool = True,
                 fused_head: Optional[bool] = None, ragged: bool = False, text_lengths: bool = False):
        self.ce_weight, self.regress = _loss_sig(model, loss_functions)
        if self.ce_weight is None and self.regress is None:
            raise L.TspmError("FusedMosiMonoEvalStep: the loss group must be a single cross-entropy term (or, under "
                              "a one-output classifier, a single mean L1 / MSE term)")
        self._init_mosi(model, x_shape, log, fused_head, ragged, text_lengths)
        self._init_graph(use_graph, self.device)

    def _enqueue(self) -> None:
        sh = torch.cuda.current_stream().cuda_stream
        self.eng.forward(sh, False)
        self._head(L.lib(), sh, False)

    def run(self) -> None:
        self.model.eval()
        self._replay_or_enqueue()

    def step(self, x: torch.Tensor, labels: torch.Tensor,
             lengths: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        self.load_batch(x, labels, lengths)
        self.run()
        return {"loss": self.loss, "logits": self.logits, "preds": self.preds}


def _bce_weight_of(loss_functions, who: str) -> float:
    """mmimdb._bce_weight, with anything that is not a loss group refused the same way."""
    from .mmimdb import _bce_weight
    try:
        return _bce_weight(loss_functions)
    except AttributeError:
        raise L.TspmError(f"{who}: the loss group must be a single bce_with_logits term (got "
                          f"{type(loss_functions).__name__})") from None


def bce_head_supported(n: int, hid: int, classes: int) -> bool:
    """tspm_mono_head_bce_step's shape limits (csrc/mmimdb.hip: HB_MAXN / HB_MAXH / HB_MAXC)."""
    return 1 <= n <= BCE_HEAD_MAX_N and 4 <= hid <= BCE_HEAD_MAX_HID and hid % 4 == 0 and \
        1 <= classes <= BCE_HEAD_MAX_CLASSES


def bce_head_choice(requested: Optional[bool], n: int, hid: int, classes: int) -> bool:
    """Whether a step of this shape runs tspm_mono_head_bce_step: ``requested`` (None = the measured default, from
    FUSED_BCE_HEAD_MIN_BATCH rows up), and never outside the kernel's limits (the separate launches take those)."""
    if requested is None:
        requested = n >= FUSED_BCE_HEAD_MIN_BATCH
    return bool(requested) and bce_head_supported(n, hid, classes)


class _MMIMDbMonoBuffers(L.GraphRunner):
    """What the MMIMDb-encoder train and eval steps share: the static buffers for one (batch, in), the graph runner
    (empty key: nothing replaceable is baked in) and the multi-label head — ``tspm_mono_head_bce_step`` or the
    separate launches (``tspm_linear_fwd``, ``tspm_bce_logits``, ``tspm_linear_bwd``)."""

    THRESHOLD = 0.5  # train_monomodal.py: torch.sigmoid(logits) > 0.5

    def _init_mmimdb(self, model, loss_functions, x_shape, fused_head: Optional[bool], who: str) -> None:
        from .mmimdb import MMIMDbModalityEncoder
        enc, cls = model.encoder, model.classifier
        if not isinstance(enc, MMIMDbModalityEncoder):
            raise L.TspmError(f"{who}: the encoder must be an MMIMDbModalityEncoder")
        self.weight = _bce_weight_of(loss_functions, who)
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise L.TspmError(f"{who} runs on the MI355X: move the model to cuda first")
        n, fin = (int(v) for v in x_shape)
        self.bn, self.fc = enc.net[0], enc.net[1]
        if fin != self.bn.num_features:
            raise L.TspmError(f"input features {fin} != encoder input_dim {self.bn.num_features}")
        if cls.in_features != self.fc.out_features:
            raise L.TspmError(f"classifier input {cls.in_features} != encoder output_dim {self.fc.out_features}")
        self.model, self.device, self.N, self.fin = model, dev, n, fin
        self.hid, self.K = cls.in_features, cls.out_features
        self.fused_head = bce_head_choice(model.fused_head if fused_head is None else fused_head, n, self.hid, self.K)
        f32 = dict(device=dev, dtype=torch.float32)
        self.X = torch.zeros(n, fin, **f32)
        self.labels = torch.zeros(n, self.K, **f32)
        self.Xn = torch.empty(n, fin, **f32)
        self.emb = torch.empty(n, self.hid, **f32)
        self.logits = torch.empty(n, self.K, **f32)
        self.loss = torch.zeros(1, **f32)
        self.stats = torch.zeros(3 + 3 * self.K, **f32)  # tspm_bce_logits' accumulators (mmimdb.f1_metrics)
        self._preds = torch.zeros(n, self.K, dtype=torch.uint8, device=dev) if self.fused_head else None
        lib = L.lib()
        if self.fused_head:
            self.head_ws_bytes = int(lib.tspm_mono_head_bce_workspace(n, self.hid, self.K))
            self.head_ws = torch.zeros(self.head_ws_bytes // 4, **f32)  # the arrival counter starts at zero
        # split-K for the long (image) Linear when its output tiles cannot fill the chip, as MMIMDbEngine does
        tiles = -(-n // 32) * -(-self.hid // 32)
        self.splits = 4 if (fin >= 2048 and tiles < 256) else 1
        wsb = lib.tspm_linear_fwd_splitk_workspace(n, fin, self.hid, self.splits) if self.splits > 1 else 0
        self.ws = torch.zeros(max(int(wsb) // 4, 4), **f32)
        self.log = None  # the multi-label counts live in ``stats``; no ClassificationLog on this path

    @property
    def preds(self) -> torch.Tensor:
        """bool [n, classes]: the head kernel's predictions, or (separate launches) sigmoid(logits) > 0.5."""
        if self._preds is not None:
            return self._preds.bool()
        return torch.sigmoid(self.logits) > self.THRESHOLD

    def _encoder_fc(self, lib, sh: int) -> None:
        fc, n = self.fc, self.N
        if self.splits > 1:
            L.check(lib.tspm_linear_fwd_splitk(n, self.fin, self.hid, self.Xn.data_ptr(), self.fin, fc.weight.data_ptr(),
                                               fc.bias.data_ptr(), 0, None, 1.0, self.emb.data_ptr(), self.hid,
                                               self.splits, self.ws.data_ptr(), self.ws.numel() * 4, sh), "encoder fc")
        else:
            L.check(lib.tspm_linear_fwd(n, self.fin, self.hid, self.Xn.data_ptr(), self.fin, fc.weight.data_ptr(),
                                        fc.bias.data_ptr(), 0, None, 1.0, self.emb.data_ptr(), self.hid, sh),
                    "encoder fc")

    def _head(self, lib, sh: int, train: bool) -> None:
        n, hid, K = self.N, self.hid, self.K
        cls = self.model.classifier
        if self.fused_head:
            d = L.MonoHeadBceDesc()
            d.n, d.hid, d.classes, d.ld_emb, d.ld_demb = n, hid, K, hid, hid
            d.loss_weight, d.threshold = self.weight, self.THRESHOLD
            d.emb, d.w, d.b = self.emb.data_ptr(), cls.weight.data_ptr(), cls.bias.data_ptr()
            d.targets, d.logits, d.loss = self.labels.data_ptr(), self.logits.data_ptr(), self.loss.data_ptr()
            d.preds, d.stats = self._preds.data_ptr(), self.stats.data_ptr()
            d.workspace, d.workspace_bytes = self.head_ws.data_ptr(), self.head_ws_bytes
            if train:
                d.dw, d.db, d.demb = cls.weight.grad.data_ptr(), cls.bias.grad.data_ptr(), self.demb.data_ptr()
            L.check(lib.tspm_mono_head_bce_step(ctypes.byref(d), sh), "mono_head_bce_step")
            return
        L.check(lib.tspm_linear_fwd(n, hid, K, self.emb.data_ptr(), hid, cls.weight.data_ptr(), cls.bias.data_ptr(), 0,
                                    None, 1.0, self.logits.data_ptr(), K, sh), "classifier fwd")
        L.check(lib.tspm_bce_logits(n, K, self.logits.data_ptr(), self.labels.data_ptr(), self.loss.data_ptr(),
                                    self.dlogits.data_ptr() if train else None, self.weight, self.THRESHOLD,
                                    self.stats.data_ptr(), sh), "bce_with_logits")
        if train:
            linear_bwd(n, hid, K, self.emb.data_ptr(), hid, self.dlogits.data_ptr(), K, cls.weight.data_ptr(),
                       cls.weight.grad.data_ptr(), cls.bias.grad.data_ptr(), self.demb.data_ptr(), hid, sh)

    def _replay_or_enqueue(self) -> None:
        self.replay_or_enqueue(self._enqueue)
        self.calls += 1

    def load_batch(self, x: torch.Tensor, labels: torch.Tensor) -> None:
        if x.data_ptr() != self.X.data_ptr():
            self.X.copy_(x.reshape(self.X.shape), non_blocking=True)
        if labels.data_ptr() != self.labels.data_ptr():
            self.labels.copy_(labels.reshape(self.labels.shape), non_blocking=True)

    def matches_shape(self, x: torch.Tensor) -> bool:
        return tuple(x.shape) == (self.N, self.fin)

    def step(self, x: torch.Tensor, labels: torch.Tensor) -> Dict[str, torch.Tensor]:
        self.load_batch(x, labels)
        self.run()
        return {"loss": self.loss, "logits": self.logits, "preds": self.preds}


class FusedMMIMDbMonoStep(_MMIMDbMonoBuffers):
    """MonomodalEncoder.train_step around an MMIMDbModalityEncoder (BatchNorm1d(in) → Linear(in, out)) under the
    multi-label classifier as one HIP graph:

        tspm_bn1d_fwd → tspm_linear_fwd → head (tspm_mono_head_bce_step: classifier, BCEWithLogits, predictions,
        F1 counts, classifier backward) → encoder Linear backward → tspm_bn1d_bwd (no dx) → FusedAdam →
        num_batches_tracked

    ``x_shape`` is (batch, in).  ``fused_head=False`` runs the head as ``tspm_linear_fwd``, ``tspm_bce_logits`` and
    ``tspm_linear_bwd`` (also taken for shapes outside the head kernel's limits).  Gradients go straight into
    FusedAdam's flat views (overwritten).  ``_lib.GraphRunner``'s lifecycle: eager, capture, replays."""

    def __init__(self, model, optimizer: FusedAdam, loss_functions, x_shape, use_graph: bool = True, log=None,
                 fused_head: Optional[bool] = None):
        if not isinstance(optimizer, FusedAdam):
            raise L.TspmError("FusedMMIMDbMonoStep needs tspm_amd.FusedAdam (the flat gradient buffer the kernels "
                              "write)")
        self._init_mmimdb(model, loss_functions, x_shape, fused_head, "FusedMMIMDbMonoStep")
        if self.N < 2:
            raise L.TspmError("BatchNorm1d in training mode needs more than one sample per batch")
        model.train()
        for p in model.parameters():
            if p.requires_grad and p.grad is None:
                raise L.TspmError("FusedMMIMDbMonoStep: parameter without a FusedAdam gradient view")
        self.opt = optimizer
        self._init_graph(use_graph, self.device)
        f32 = dict(device=self.device, dtype=torch.float32)
        self.mean, self.inv = torch.zeros(self.fin, **f32), torch.zeros(self.fin, **f32)
        self.demb = torch.empty(self.N, self.hid, **f32)
        self.dXn = torch.empty(self.N, self.fin, **f32)
        self.dlogits = torch.empty(self.N, self.K, **f32)
        self.nbt = shared_batches_tracked(model, self.device, (nn.BatchNorm1d,))
        self._sig = (id(optimizer), id(loss_functions), self.fused_head)

    def matches(self, x: torch.Tensor, optimizer, loss_functions, fused_head: Optional[bool] = None) -> bool:
        fh = bce_head_choice(self.model.fused_head if fused_head is None else fused_head, self.N, self.hid, self.K)
        return self._sig == (id(optimizer), id(loss_functions), fh) and self.matches_shape(x)

    def _enqueue(self) -> None:
        from .mmimdb import _bn
        lib = L.lib()
        sh = torch.cuda.current_stream().cuda_stream
        n, fin, hid = self.N, self.fin, self.hid
        bn, fc = self.bn, self.fc
        g, b, rm, rv, eps, mom = _bn(bn)
        L.check(lib.tspm_bn1d_fwd(n, fin, self.X.data_ptr(), g.data_ptr(), b.data_ptr(), rm.data_ptr(), rv.data_ptr(),
                                  mom, eps, self.mean.data_ptr(), self.inv.data_ptr(), self.Xn.data_ptr(), sh),
                "bn1d_fwd")
        self._encoder_fc(lib, sh)
        self._head(lib, sh, True)
        # encoder Linear: weight and bias gradients, and the data gradient the BatchNorm1d backward needs
        linear_bwd(n, fin, hid, self.Xn.data_ptr(), fin, self.demb.data_ptr(), hid, fc.weight.data_ptr(),
                   fc.weight.grad.data_ptr(), fc.bias.grad.data_ptr(), self.dXn.data_ptr(), fin, sh)
        L.check(lib.tspm_bn1d_bwd(n, fin, self.dXn.data_ptr(), self.X.data_ptr(), self.mean.data_ptr(),
                                  self.inv.data_ptr(), bn.weight.data_ptr(), bn.weight.grad.data_ptr(),
                                  bn.bias.grad.data_ptr(), None, sh), "bn1d_bwd")
        self.opt.launch(sh)
        L.counters_add(self.nbt)

    def run(self) -> None:
        """One training step on the batch in the static input buffers."""
        self.model.train()
        self.opt.sync_hyper()
        self._replay_or_enqueue()
        self.opt.note_steps(1)


class FusedMMIMDbMonoEvalStep(_MMIMDbMonoBuffers):
    """MonomodalEncoder.validation_step around an MMIMDbModalityEncoder as one HIP graph: ``tspm_bn_apply_eval``
    (running statistics), the Linear, and the head in forward-only mode (logits, weighted BCE, predictions, F1
    counts)."""

    def __init__(self, model, loss_functions, x_shape, log=None, use_graph: bool = True,
                 fused_head: Optional[bool] = None):
        self._init_mmimdb(model, loss_functions, x_shape, fused_head, "FusedMMIMDbMonoEvalStep")
        self._init_graph(use_graph, self.device)

    def _enqueue(self) -> None:
        from .mmimdb import _bn
        lib = L.lib()
        sh = torch.cuda.current_stream().cuda_stream
        g, b, rm, rv, eps, _ = _bn(self.bn)
        L.check(lib.tspm_bn_apply_eval(self.N, self.fin, self.X.data_ptr(), rm.data_ptr(), rv.data_ptr(), eps,
                                       g.data_ptr(), b.data_ptr(), 0, None, None, None, None, None, 0,
                                       self.Xn.data_ptr(), sh), "bn_apply_eval")
        self._encoder_fc(lib, sh)
        self._head(lib, sh, False)

    def run(self) -> None:
        self.model.eval()
        self._replay_or_enqueue()


class _MosiMonoFn(torch.autograd.Function):
    """MonomodalEncoder.forward around a MOSI encoder as one autograd node (encoder + classifier on the HIP
    schedule, forward and backward), for the reference's own train_step sequence with a torch optimizer."""

    @staticmethod
    def forward(ctx, x, model: "MonomodalEncoder", lengths, *params):
        eng = model._mosi_engine(x.shape[0], x.shape[1], x.device, **model._len_modes(lengths is not None))
        eng.load(x)
        eng.set_lengths(lengths)
        eng.apply_keep_override()
        sh = L.stream_handle()
        eng.forward(sh, True)
        cls = model.classifier
        n, hid, K = x.shape[0], cls.in_features, cls.out_features
        logits = torch.empty(n, K, device=x.device, dtype=torch.float32)
        L.check(L.lib().tspm_linear_fwd(n, hid, K, eng.emb.data_ptr(), hid, cls.weight.data_ptr(), cls.bias.data_ptr(),
                                        0, None, 1.0, logits.data_ptr(), K, sh), "classifier fwd")
        model._fwd_generation += 1
        ctx.model, ctx.eng, ctx.gen = model, eng, model._fwd_generation
        return logits

    @staticmethod
    def backward(ctx, g):
        model, eng = ctx.model, ctx.eng
        if model._fwd_generation != ctx.gen:
            raise L.TspmError("MonomodalEncoder: another training forward ran before this backward")
        g = g.contiguous().float()
        grads = {id(p): torch.empty_like(p) for p in model.parameters()}
        cls, sh = model.classifier, L.stream_handle()
        n, hid, K = g.shape[0], cls.in_features, cls.out_features
        linear_bwd(n, hid, K, eng.emb.data_ptr(), hid, g.data_ptr(), K, cls.weight.data_ptr(),
                   grads[id(cls.weight)].data_ptr(), grads[id(cls.bias)].data_ptr(), eng.demb.data_ptr(), hid, sh)
        eng.grad_of = lambda p: grads[id(p)]  # noqa: E731
        try:
            eng.backward(sh)
        finally:
            eng.grad_of = lambda p: p.grad  # noqa: E731
        return (None, None, None, *[grads[id(p)] for p in model.parameters()])


class MonomodalEncoder(nn.Module):
    """train_monomodal.py:64-95 drop-in: ``encoder`` + ``classifier``, executed on libtspm."""

    def __init__(self, encoder: nn.Module, output_dim: int, num_classes: int, fused_head: Optional[bool] = None):
        super().__init__()
        self.encoder = encoder
        self.classifier = nn.Linear(output_dim, num_classes)
        self._fused: Optional[FusedMonoStep] = None
        self._eval_steps: Dict[Tuple, FusedMonoEvalStep] = {}
        # MOSI / MOSEI encoders (mosi.LSTMEncoder / mosi.TextCNN): the head in one launch (tspm_mono_head_step)
        # or, fused_head=False, the separate classifier / CE / classify / classifier-backward launches
        # MMIMDb encoders (mmimdb.MMIMDbModalityEncoder): tspm_mono_head_bce_step or, fused_head=False, tspm_linear_fwd /
        # tspm_bce_logits / tspm_linear_bwd.  None = the measured default: FUSED_HEAD_DEFAULT for the MOSI encoders,
        # per batch size for the MMIMDb ones (bce_head_choice)
        if fused_head is None and not self._mmimdb_encoder():
            fused_head = FUSED_HEAD_DEFAULT
        self.fused_head = None if fused_head is None else bool(fused_head)
        self._rng_seed = int(torch.initial_seed()) & ((1 << 63) - 1)  # the TextCNN dropout masks' seed
        self._mosi_engines: Dict[Tuple, Any] = {}
        self._by_buffer: Dict[int, Any] = {}  # input buffer address -> the MOSI step that owns it
        self._fwd_generation = 0

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._mosi_engines = {}
        return out

    def _mosi_engine(self, b: int, t: int, device, ragged: bool = False, text_lengths: bool = False):
        from .mosi import MosiEncoderEngine
        key = (int(b), int(t), device) + _len_tag(ragged, text_lengths)
        eng = self._mosi_engines.get(key)
        if eng is None:
            eng = self._mosi_engines[key] = MosiEncoderEngine(self.encoder, b, t, device, seed=self._rng_seed,
                                                              ragged=ragged, text_lengths=text_lengths)
        return eng

    def _len_modes(self, on: bool) -> Dict[str, bool]:
        """The step / engine keywords of a batch with (``on``) or without per-sample lengths: ``ragged`` around an
        LSTMEncoder, ``text_lengths`` around a TextCNN."""
        from .mosi import TextCNN
        text = isinstance(self.encoder, TextCNN)
        return dict(ragged=bool(on) and not text, text_lengths=bool(on) and text)

    def _lengths_of(self, batch, key) -> Optional[torch.Tensor]:
        """The batch's per-sample lengths for an LSTMEncoder or a TextCNN (``"lengths"``: an int tensor [B], or a dict
        by modality name as the fusion loader delivers — the text modality's only from a ``text_lengths`` dataset);
        None for every other encoder and for a batch without them."""
        lengths = batch.get("lengths") if self._mosi_encoder() else None
        if isinstance(lengths, dict):
            lengths = lengths.get(str(getattr(key, "value", key)).lower().split(".")[-1])
        return lengths

    def forward(self, x, lengths: Optional[torch.Tensor] = None):
        """``lengths`` (an LSTMEncoder or a TextCNN only): int [B], each row's real length (``LSTMEncoder.forward``,
        ``TextCNN.forward``)."""
        if isinstance(x, list):
            x = torch.stack(x)
        if lengths is not None and not self._mosi_encoder():
            raise L.TspmError("MonomodalEncoder: lengths are taken by an LSTMEncoder or a TextCNN only")
        if self._mosi_encoder() and self.training and torch.is_grad_enabled():
            x = x.float()
            if not x.is_cuda:
                raise L.TspmError("MonomodalEncoder (tspm_amd) runs on the MI355X only (there is no CPU fallback)")
            return _MosiMonoFn.apply(x, self, lengths, *self.parameters())
        encoded = self.encoder(x) if lengths is None else self.encoder(x, lengths)
        if encoded.dim() > 2:  # train_monomodal.py:83-86
            encoded = encoded.reshape(encoded.shape[0], -1)
        if not encoded.is_cuda:
            raise L.TspmError("MonomodalEncoder (tspm_amd) runs on the MI355X only (there is no CPU fallback)")
        return _LinearFn.apply(encoded.contiguous().float(), self.classifier.weight, self.classifier.bias)

    def get_encoder(self) -> nn.Module:
        return self.encoder

    # -- steps ------------------------------------------------------------------------------------
    def _inputs(self, batch, config, device):
        key = select_modality_key(batch, _exp_name(config))
        raw = batch[f"{key}_original"] if f"{key}_original" in batch else batch[key]
        x = _as_tensor(raw).to(device, non_blocking=True).float()
        labels = _labels_of(batch).to(device, non_blocking=True)
        return key, x, labels

    def _hip_encoder(self) -> bool:
        from .modules import ResNetEncoder
        return isinstance(self.encoder, ResNetEncoder)

    def _mosi_encoder(self) -> bool:
        from .mosi import LSTMEncoder, TextCNN
        return isinstance(self.encoder, (LSTMEncoder, TextCNN))

    def _mmimdb_encoder(self) -> bool:
        from .mmimdb import MMIMDbModalityEncoder
        return isinstance(self.encoder, MMIMDbModalityEncoder)

    def _check_mmimdb_step(self, x: torch.Tensor, labels: torch.Tensor, optimizer, loss_functions, train: bool) -> None:
        """An MMIMDbModalityEncoder trains and validates on the fused HIP steps only: anything they cannot take is
        refused here (no autograd node is built for this encoder)."""
        who = "MonomodalEncoder around an MMIMDbModalityEncoder"
        try:
            _bce_weight_of(loss_functions, who)
        except L.TspmError as e:
            raise L.TspmError(f"{who}: unsupported loss group ({e}); this encoder has no autograd path") from None
        if train and not isinstance(optimizer, FusedAdam):
            raise L.TspmError(f"{who} trains with tspm_amd.FusedAdam only (got {type(optimizer).__name__}): this "
                              "encoder has no autograd path")
        if not x.is_cuda:
            raise L.TspmError("MonomodalEncoder (tspm_amd) runs on the MI355X only (there is no CPU fallback)")
        if x.dim() != 2 or labels.dim() != 2 or not labels.is_floating_point():
            raise L.TspmError(f"{who}: expected [n, in] features and float multi-hot [n, classes] labels, got "
                              f"{tuple(x.shape)} and {labels.dtype} {tuple(labels.shape)}")

    def train_step_fused(self, x: torch.Tensor, labels: torch.Tensor, optimizer, loss_functions,
                         log: Optional[ClassificationLog] = None,
                         lengths: Optional[torch.Tensor] = None) -> FusedMonoStep:
        """Run one fused step on device tensors and return the step (its loss / logits / preds buffers).  ``lengths``
        (an LSTMEncoder: the ragged step; a TextCNN: the text_lengths step): int [B] — one graph per padded shape whatever
        the lengths."""
        if lengths is not None:
            modes = self._len_modes(True)
            st = self._by_buffer.get(x.data_ptr())
            if not (isinstance(st, FusedMosiMonoStep) and st.matches(x, optimizer, loss_functions, **modes)):
                st = self._fused
            if not (isinstance(st, FusedMosiMonoStep) and st.matches(x, optimizer, loss_functions, **modes)):
                st = FusedMosiMonoStep(self, optimizer, loss_functions, tuple(x.shape), **modes)
            self._fused = st
            st.log = log
            st.step(x, labels, lengths)
            return st
        if self._mmimdb_encoder():
            self._check_mmimdb_step(x, labels, optimizer, loss_functions, True)
            if not isinstance(self._fused, FusedMMIMDbMonoStep) or \
                    not self._fused.matches(x, optimizer, loss_functions):
                self._fused = FusedMMIMDbMonoStep(self, optimizer, loss_functions, tuple(x.shape))
            self._fused.step(x, labels)
            return self._fused
        if self._fused is None or not self._fused.matches(x, optimizer, loss_functions):
            own = self._by_buffer.get(x.data_ptr())
            if self._mosi_encoder():
                self._fused = own if isinstance(own, FusedMosiMonoStep) and own.matches(x, optimizer, loss_functions) \
                    else FusedMosiMonoStep(self, optimizer, loss_functions, tuple(x.shape))
            else:
                self._fused = FusedMonoStep(self, optimizer, loss_functions, tuple(x.shape))
        self._fused.log = log
        self._fused.step(x, labels)
        return self._fused

    def eval_step_for(self, loss_functions, x_shape, log=None, ragged: bool = False,
                      text_lengths: bool = False) -> FusedMonoEvalStep:
        key = tuple(x_shape) + _len_tag(ragged, text_lengths)
        st = self._eval_steps.get(key)
        if self._mmimdb_encoder():
            if st is None or st.weight != _bce_weight_of(loss_functions, "MonomodalEncoder") or \
                    st.fused_head != bce_head_choice(self.fused_head, st.N, st.hid, st.K):
                st = self._eval_steps[key] = FusedMMIMDbMonoEvalStep(self, loss_functions, key)
            return st
        if st is None or (st.ce_weight, getattr(st, "regress", None)) != _loss_sig(self, loss_functions) or \
                getattr(st, "fused_head", self.fused_head) != self.fused_head:
            if ragged or text_lengths:
                st = FusedMosiMonoEvalStep(self, loss_functions, tuple(x_shape), log, ragged=ragged,
                                           text_lengths=text_lengths)
            else:
                cls = FusedMosiMonoEvalStep if self._mosi_encoder() else FusedMonoEvalStep
                st = cls(self, loss_functions, key, log)
            self._eval_steps[key] = st
        st.log = log
        return st

    def _eval_step_of(self, x: torch.Tensor, loss_functions, log=None, ragged: bool = False,
                      text_lengths: bool = False):
        """The eval step for batch x: the step whose input buffer x is (a loader gathered into it), else by shape."""
        own = self._by_buffer.get(x.data_ptr())
        if isinstance(own, FusedMosiMonoEvalStep) and (own.ce_weight, own.regress) == _loss_sig(self, loss_functions) \
                and (own.ragged, own.text_lengths) == (bool(ragged), bool(text_lengths)):
            own.log = log
            return own
        return self.eval_step_for(loss_functions, tuple(x.shape), log, ragged, text_lengths)

    def train_step(self, batch, optimizer, loss_functions, device, metric_recorder, config=None, **kwargs):
        """train_monomodal.py:97-260.  Fused HIP graph with FusedAdam and the single cross-entropy loss
        group; otherwise the reference's autograd sequence on the HIP encoder / classifier."""
        key, x, labels = self._inputs(batch, config, device)
        dlog = _device_log(metric_recorder)
        if self._mmimdb_encoder():
            st = self.train_step_fused(x, labels, optimizer, loss_functions)
            return self._finish(metric_recorder, dlog, key, st.preds, labels, st.loss)
        reg = _mono_regress(self, loss_functions)
        if reg is not None:  # sentiment regression: float32 scores [n]
            labels = labels.float().reshape(-1)
        head_ok = (_ce_weight(loss_functions) is not None if reg is None
                   else L.regress_head_supported(x.shape[0], self.classifier.in_features))
        fused = (not os.environ.get("TSPM_DISABLE_FUSED_STEP") and isinstance(optimizer, FusedAdam)
                 and head_ok and x.is_cuda and labels.dim() == 1
                 and ((self._hip_encoder() and x.dim() in (3, 4)) or (self._mosi_encoder() and x.dim() == 3)))
        lengths = self._lengths_of(batch, key)
        if fused:
            st = self.train_step_fused(x, labels, optimizer, loss_functions, dlog, lengths)
            loss_t, preds = st.loss, st.preds
        else:
            optimizer.zero_grad()
            logits = self.forward(x, lengths) if lengths is not None else self.forward(x)
            if reg is not None:
                logits = logits.reshape(-1)
            loss_t = loss_functions(logits, labels)["total_loss"]
            loss_t.backward()
            optimizer.step()
            with torch.no_grad():
                preds = logits.detach() if reg is not None else \
                    torch.argmax(logits, dim=1) if labels.dim() == 1 else torch.sigmoid(logits) > 0.5
        return self._finish(metric_recorder, dlog, key, preds, labels, loss_t, reg is not None)

    def validation_step(self, batch, loss_functions, device, metric_recorder, config=None, **kwargs):
        """train_monomodal.py:262-418 (the caller puts the model in eval mode, as train_monomodal does)."""
        with torch.no_grad():
            key, x, labels = self._inputs(batch, config, device)
            dlog = _device_log(metric_recorder)
            if self._mmimdb_encoder():
                self._check_mmimdb_step(x, labels, None, loss_functions, False)
                st = self.eval_step_for(loss_functions, tuple(x.shape))
                st.step(x, labels)
                return self._finish(metric_recorder, dlog, key, st.preds, labels, st.loss)
            reg = _mono_regress(self, loss_functions)
            if reg is not None:
                labels = labels.float().reshape(-1)
            head_ok = (_ce_weight(loss_functions) is not None if reg is None
                       else L.regress_head_supported(x.shape[0], self.classifier.in_features))
            if (not self.training and head_ok and x.is_cuda and labels.dim() == 1
                    and ((self._hip_encoder() and x.dim() in (3, 4)) or (self._mosi_encoder() and x.dim() == 3))):
                lengths = self._lengths_of(batch, key)
                st = self._eval_step_of(x, loss_functions, dlog, **self._len_modes(lengths is not None))
                st.step(x, labels, lengths) if lengths is not None else st.step(x, labels)
                loss_t, preds = st.loss, st.preds
            else:
                lengths = self._lengths_of(batch, key)
                logits = self.forward(x, lengths) if lengths is not None else self.forward(x)
                if reg is not None:
                    logits = logits.reshape(-1)
                loss_t = loss_functions(logits, labels)["total_loss"]
                preds = logits if reg is not None else \
                    torch.argmax(logits, dim=1) if labels.dim() == 1 else torch.sigmoid(logits) > 0.5
            return self._finish(metric_recorder, dlog, key, preds, labels, loss_t, reg is not None)

    @staticmethod
    def _finish(metric_recorder, dlog, key, preds, labels, loss_t, regression: bool = False):
        with torch.no_grad():
            if metric_recorder is not None and dlog is None:
                for group_name in metric_recorder.config.groups:
                    metric_recorder.update_group(group_name=group_name, predictions=preds, targets=labels,
                                                 modality=str(key))
            loss = float(loss_t.item() if torch.is_tensor(loss_t) else loss_t)
            metrics = {"loss": loss}
            if labels.dim() == 1 and not regression:
                metrics["accuracy"] = (preds == labels).float().mean().item()
        return {"loss": loss, "metrics": metrics}


# ------------------------------------------------------------------------------------------------
# Epoch harness (train_monomodal.py:536-884)
# ------------------------------------------------------------------------------------------------
def modality_of_experiment(name: str) -> str:
    """train_monomodal.py:793-798: the first of image/text/audio/video among the name's '_' parts."""
    for part in name.lower().split("_"):
        if part in ("image", "text", "audio", "video"):
            return part
    return "unknown"


class MonoEpochRunner:
    """Train / validation epochs of train_monomodal (train_monomodal.py:658-753) on the fused steps.
    Per batch: the batch (device tensors, e.g. a data.DeviceLoader's gather) + one graph replay; the
    per-batch losses and confusion counts stay on the device (``tspm_classify_update_ex``) and per-batch
    accuracies are device scalars, all read once per epoch.  Epoch dict = the reference's
    ``avg_*_metrics``: ``loss`` / ``accuracy`` = np.mean over the batches, updated with the flattened
    metric-recorder results (keys ``f"{metric}_{MODALITY}"``)."""

    def __init__(self, model: MonomodalEncoder, optimizer, loss_functions, experiment_name: str,
                 metric_config=None, device=None, log_capacity: int = 1 << 16):
        from .harness import AVMNIST_METRICS
        self.model, self.optimizer, self.loss_functions = model, optimizer, loss_functions
        self.experiment_name = experiment_name
        self.device = device or next(model.parameters()).device
        self.metric_config = metric_config or AVMNIST_METRICS
        self.log_capacity = log_capacity
        self.log: Optional[ClassificationLog] = None
        self.recorder: Optional[DeviceMetricRecorder] = None
        self.train_steps: Dict[Tuple, FusedMonoStep] = {}
        self._mosi = model._mosi_encoder()
        self._mmimdb = model._mmimdb_encoder()
        self.ragged = False
        self.text_lengths = False
        # sentiment regression (one-output classifier, a single mean L1 / MSE term): the regression head's
        # accumulators, MSA_<key>_<MODALITY> scores under the group "regression", no accuracy
        self.regression = _mono_regress(model, loss_functions) is not None

    # MOSI encoders: ``mosi_data.MOSI.loader(...)``'s ``step_for`` hooks — the loader gathers each batch time-major
    # straight into the step's input buffer (set on every loader that has the attribute, as harness.MosiHarness does)
    def train_step_for(self, b: int, t: int, ragged: Optional[bool] = None, text_lengths: Optional[bool] = None):
        shape = (int(b), int(t), int(self.model.encoder.input_size))
        ragged = self.ragged if ragged is None else bool(ragged)
        tl = self.text_lengths if text_lengths is None else bool(text_lengths)
        key = shape + _len_tag(ragged, tl)
        st = self.train_steps.get(key)
        if st is None or (self._mosi and st.fused_head != self.model.fused_head):
            if ragged or tl:
                st = FusedMosiMonoStep(self.model, self.optimizer, self.loss_functions, shape, ragged=ragged,
                                       text_lengths=tl)
            else:
                cls = FusedMosiMonoStep if self._mosi else FusedMonoStep
                st = cls(self.model, self.optimizer, self.loss_functions, shape)
            self.train_steps[key] = st
        return st

    def eval_step_for(self, b: int, t: int, ragged: Optional[bool] = None, text_lengths: Optional[bool] = None):
        ragged = self.ragged if ragged is None else bool(ragged)
        tl = self.text_lengths if text_lengths is None else bool(text_lengths)
        return self.model.eval_step_for(self.loss_functions, (int(b), int(t), int(self.model.encoder.input_size)),
                                        self.log, ragged, tl)

    def _hook(self, loader, train: bool) -> None:
        from .mosi import LSTMEncoder, TextCNN
        # the loader's dataset carries per-sample lengths (mosi_data.MOSI(use_lengths=True)): the ragged steps; the
        # text lengths too (text_lengths=True): a TextCNN's text_lengths steps
        self.ragged = bool(getattr(getattr(loader, "ds", None), "use_lengths", False)) and \
            isinstance(self.model.encoder, LSTMEncoder)
        self.text_lengths = bool(getattr(getattr(loader, "ds", None), "text_lengths", False)) and \
            isinstance(self.model.encoder, TextCNN)
        if self._mosi and hasattr(loader, "step_for"):
            loader.step_for = self.train_step_for if train else self.eval_step_for

    def _ensure_log(self, key) -> None:
        if self.log is None and self.regression:
            self.log = RegressionLog(self.device, groups=(str(key),), capacity=self.log_capacity)
            self.recorder = RegressionMetricRecorder(self.log)
        elif self.log is None:
            self.log = ClassificationLog(self.device, groups=(str(key),), capacity=self.log_capacity)
            self.recorder = DeviceMetricRecorder(self.metric_config, self.log)

    def _finish(self, t0: float, accs: List[torch.Tensor]) -> Tuple[Dict[str, Any], float]:
        conf, losses, _ = self.log.fetch()  # the epoch's host synchronisation
        acc = torch.stack(accs).cpu().tolist() if accs else []
        mean = ClassificationLog.mean_loss(losses)
        out: Dict[str, Any] = {"loss": mean}
        if acc:
            out["accuracy"] = float(np.mean(acc))
        for g in self.recorder.groups:
            out.update(self.recorder.calculate_metrics_for_group(g, loss=mean, records=conf) if self.regression
                       else self.recorder.calculate_metrics_for_group(g, loss=mean, conf=conf))
        return out, time.time() - t0

    def _batches(self, loader):
        started = False
        for b in loader:
            key, x, lab = self.model._inputs(b, self.experiment_name, self.device)
            self._ensure_log(key)
            if not started:
                self.log.reset()
                started = True
            yield x, lab, self.model._lengths_of(b, key)
        if not started:
            raise ValueError("empty loader")

    def _multilabel_epoch(self, loader, train: bool) -> Tuple[Dict[str, Any], float]:
        """An epoch around an MMIMDbModalityEncoder: per batch one graph replay; the head's F1 accumulators and the
        per-batch losses stay on the device and are read once.  Epoch dict = ``loss`` (np.mean over the batches, as
        the reference) + mmimdb.f1_metrics of the epoch's counts, keys ``f"{metric}_{MODALITY}"``.  A one-row
        training batch is skipped (BatchNorm1d in training mode rejects it, in the reference too)."""
        from .mmimdb import f1_metrics
        t0 = time.time()
        self.model.train(train)
        used: List[Any] = []
        losses: List[torch.Tensor] = []
        key = None
        for b in loader:
            key, x, lab = self.model._inputs(b, self.experiment_name, self.device)
            if not used:
                self.model._check_mmimdb_step(x, lab, self.optimizer, self.loss_functions, train)
            shape = tuple(x.shape)
            if train:
                if shape[0] < 2:
                    continue
                st = self.train_steps.get(shape)
                if st is None or not st.matches(x, self.optimizer, self.loss_functions):
                    st = self.train_steps[shape] = FusedMMIMDbMonoStep(self.model, self.optimizer,
                                                                       self.loss_functions, shape)
            else:
                st = self.model.eval_step_for(self.loss_functions, shape)
            if not any(st is u for u in used):
                st.stats.zero_()
                used.append(st)
            st.load_batch(x, lab)
            st.run()
            losses.append(st.loss.clone())
        if not used:
            raise ValueError("empty loader")
        classes = self.model.classifier.out_features
        host = torch.cat([torch.stack([u.stats for u in used]).sum(0), torch.cat(losses)]).cpu()  # the epoch's one read
        stats, per_batch = host[:3 + 3 * classes], host[3 + 3 * classes:]
        out: Dict[str, Any] = {"loss": float(np.mean(per_batch.numpy()))}
        tag = str(key).replace("z", "").upper()
        for name, v in f1_metrics(stats, classes).items():
            if name != "loss":
                out[f"{name}_{tag}"] = v
        return out, time.time() - t0

    def train_epoch(self, loader: Iterable[Dict[str, Any]]):
        """→ (epoch metrics dict, seconds)."""
        if self._mmimdb:
            return self._multilabel_epoch(loader, True)
        t0 = time.time()
        accs: List[torch.Tensor] = []
        self.model.train()
        self._hook(loader, True)
        for x, lab, lens in self._batches(loader):
            st = self.model._by_buffer.get(x.data_ptr()) if self._mosi else None
            modes = self.model._len_modes(lens is not None)
            if not isinstance(st, FusedMosiMonoStep) or (st.ragged, st.text_lengths) != tuple(modes.values()):
                shape = tuple(x.shape)
                st = (self.train_step_for(*shape[:2], **modes) if self._mosi
                      else self.train_steps.get(shape))
                if st is None:
                    st = FusedMonoStep(self.model, self.optimizer, self.loss_functions, shape)
                    self.train_steps[shape] = st
            st.log = self.log
            st.step(x, lab, lens) if lens is not None else st.step(x, lab)
            if not self.regression:
                accs.append(st.batch_accuracy())
        return self._finish(t0, accs)

    @torch.no_grad()
    def validate_epoch(self, loader: Iterable[Dict[str, Any]]):
        if self._mmimdb:
            return self._multilabel_epoch(loader, False)
        t0 = time.time()
        accs: List[torch.Tensor] = []
        self.model.eval()
        self._hook(loader, False)
        for x, lab, lens in self._batches(loader):
            st = self.model._eval_step_of(x, self.loss_functions, self.log, **self.model._len_modes(lens is not None))
            st.step(x, lab, lens) if lens is not None else st.step(x, lab)
            if not self.regression:
                accs.append(st.batch_accuracy())
        return self._finish(t0, accs)


def fit_monomodal(model: MonomodalEncoder, optimizer, loss_functions, loaders: Dict[str, Any], epochs: int, *,
                  experiment_name: str, model_output_path=None, save_metric: str = "loss",
                  early_stopping: bool = True, patience: int = 10, scheduler_factory=None,
                  metric_config=None) -> Dict[str, Any]:
    """``train_monomodal`` (train_monomodal.py:536-884) on the HIP steps: per epoch train → validate →
    best by ``save_metric`` (strictly lower loss / higher accuracy, no min_delta) → on improvement
    ``epoch_{n}.pth`` + ``best.pth`` (model + optimizer state) and ``encoder_{modality}_best.pth``
    (the encoder's state_dict, the pretrained late-fusion hand-off) → early stopping after
    ``patience`` epochs without improvement → ``scheduler_factory(optimizer)`` built afresh and stepped
    every epoch (the reference re-creates its scheduler each epoch, train_monomodal.py:810-815, so a
    ReduceLROnPlateau never accumulates patience — reproduced, not fixed) → test on the best model."""
    from .harness import CheckpointManager
    if model._mmimdb_encoder() and save_metric != "loss":
        raise ValueError(f"save_metric {save_metric!r}: a multi-label (MMIMDb) pre-training run has no accuracy; "
                         "only save_metric='loss' is supported")
    if _mono_regress(model, loss_functions) is not None and save_metric != "loss":
        raise ValueError(f"save_metric {save_metric!r}: a regression pre-training run has no accuracy; only "
                         "save_metric='loss' is supported")
    runner = MonoEpochRunner(model, optimizer, loss_functions, experiment_name, metric_config)
    out_dir = Path(model_output_path) if model_output_path is not None else None
    ckpt = CheckpointManager(out_dir, save_metric, "minimize" if save_metric == "loss" else "maximize") \
        if out_dir is not None else None
    history: Dict[str, Any] = {"metrics_history": {"train": [], "validation": [], "test": []},
                               "timing_history": {"train": [], "validation": []}}
    best_loss, best_acc, wait = math.inf, 0.0, 0
    modality = modality_of_experiment(experiment_name)
    encoder_path = None
    for epoch in range(epochs):
        tr, tr_t = runner.train_epoch(loaders["train"])
        va, va_t = runner.validate_epoch(loaders["validation"])
        history["metrics_history"]["train"].append(tr)
        history["metrics_history"]["validation"].append(va)
        history["timing_history"]["train"].append(tr_t)
        history["timing_history"]["validation"].append(va_t)
        cur_loss, cur_acc = va["loss"], va.get("accuracy", 0)
        is_best = False
        if save_metric == "loss" and cur_loss < best_loss:
            best_loss, is_best, wait = cur_loss, True, 0
        elif save_metric != "loss" and cur_acc > best_acc:
            best_acc, is_best, wait = cur_acc, True, 0
        else:
            wait += 1
        if is_best and ckpt is not None:
            ckpt.save_checkpoint(model, optimizer, None, epoch, va, is_best=True)
            encoder_path = out_dir / f"encoder_{modality}_best.pth"
            torch.save(model.get_encoder().state_dict(), encoder_path)
        if early_stopping and wait >= patience:
            break
        if scheduler_factory is not None:
            sched = scheduler_factory(optimizer)
            if isinstance(sched, torch.optim.lr_scheduler.ReduceLROnPlateau):
                sched.step(cur_loss)
            else:
                sched.step()
    if "test" in loaders:
        if ckpt is not None and (ckpt.model_dir / "best.pth").exists():
            ckpt.load_checkpoint(model, load_best=True)
        te, te_t = runner.validate_epoch(loaders["test"])
        history["metrics_history"]["test"] = te
        history["timing_history"]["test"] = [te_t]
    history["best_val_loss"] = best_loss
    history["best_val_accuracy"] = best_acc
    history["encoder_path"] = str(encoder_path) if encoder_path is not None else None
    return history
