"""Drop-in replacements for the reference's encoder and fusion classes.

* ``BasicBlock`` / ``ResNetEncoder`` / ``ResNet18`` / ``ResNet34`` — same constructor signatures,
  submodule names, creation + initialisation order (so ``torch.manual_seed`` gives bit-identical
  weights) and ``state_dict`` keys as MML_Suite/models/msa/networks/resnet.py:8-54,113-239.  The
  submodules are parameter containers only: ``forward`` runs the libtspm HIP schedule
  (``engine.EncoderEngine``) and plugs into autograd as one ``torch.autograd.Function`` per encoder.
* ``AVMNIST`` — MML_Suite/models/avmnist.py:188-410 (late fusion by concat → Linear/ReLU/Dropout/
  Linear/ReLU/Linear), with ``train_step`` running the fused native step (``step.FusedTrainStep``:
  forward, cross-entropy, backward, Adam as one captured HIP graph) when the optimizer is this
  package's ``FusedAdam`` and the loss group is the reference's single cross-entropy term; otherwise
  it follows the reference's own autograd sequence with the HIP encoders/head.

Conv weights are kept OHWI (``channels_last`` view of the OIHW parameter); values, shapes and keys
are unchanged, so ``best.pth`` / ``encoder_{mod}_best.pth`` checkpoints interoperate.
"""
from __future__ import annotations

import weakref
from collections import defaultdict
from functools import partial
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from .engine import EncoderEngine, prepare_encoder_layout

NUM_CLASSES = 10  # MML_Suite/data/avmnist.py:29


# ------------------------------------------------------------------------------------------------
# ResNet encoder (parameter containers in the reference's creation order)
# ------------------------------------------------------------------------------------------------
class BasicBlock(nn.Module):
    """Parameter container of resnet.py:8-54 (conv1, bn1, relu, conv2, bn2, downsample)."""
    expansion: int = 1

    def __init__(self, inplanes: int, planes: int, stride: int = 1, downsample: Optional[nn.Module] = None,
                 norm_layer=None) -> None:
        super().__init__()
        if norm_layer is None:
            norm_layer = nn.BatchNorm2d
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn1 = norm_layer(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn2 = norm_layer(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):  # pragma: no cover - blocks run inside the encoder schedule
        raise RuntimeError("BasicBlock is executed by ResNetEncoder's HIP schedule, not standalone")


class ResNetEncoder(nn.Module):
    """resnet.py:113-219 — ResNet encoder for 1-channel AVMNIST inputs, HIP-executed."""

    def __init__(self, block=BasicBlock, layers: Sequence[int] = (2, 2, 2, 2), in_channels: int = 1,
                 hidden_dim: int = 128, zero_init_residual: bool = False, norm_layer=None) -> None:
        super().__init__()
        if isinstance(block, str):
            if block.lower() not in ("basicblock", "basic"):
                raise NotImplementedError(f"block {block!r}: only BasicBlock (ResNet18/34) is on the HIP path")
            block = BasicBlock
        if getattr(block, "expansion", 1) != 1:
            raise NotImplementedError("Bottleneck (ResNet50) is outside the AVMNIST hot path (SURVEY §8)")
        if norm_layer is None:
            norm_layer = nn.BatchNorm2d
        if norm_layer is not nn.BatchNorm2d:
            raise NotImplementedError("only nn.BatchNorm2d is supported on the HIP path")
        self._norm_layer = norm_layer
        self.hidden_dim = hidden_dim
        self.inplanes = 64
        self.dilation = 1
        self.conv1 = nn.Conv2d(in_channels, self.inplanes, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = norm_layer(self.inplanes)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(BasicBlock, 64, layers[0])
        self.layer2 = self._make_layer(BasicBlock, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(BasicBlock, 256, layers[2], stride=2)
        self.layer4 = self._make_layer(BasicBlock, 512, layers[3], stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512 * BasicBlock.expansion, hidden_dim)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        if zero_init_residual:
            for m in self.modules():
                if isinstance(m, BasicBlock):
                    nn.init.constant_(m.bn2.weight, 0)
        self._engines: Dict[Tuple, EncoderEngine] = {}
        self._fwd_generation = 0
        self._weights_generation = 0  # bumped by load_state_dict and by anything that moves the parameters

    def _make_layer(self, block, planes: int, blocks: int, stride: int = 1) -> nn.Sequential:
        norm_layer = self._norm_layer
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(
                nn.Conv2d(self.inplanes, planes * block.expansion, kernel_size=1, stride=stride, bias=False),
                norm_layer(planes * block.expansion),
            )
        layers = [block(self.inplanes, planes, stride, downsample, norm_layer)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes, norm_layer=norm_layer))
        return nn.Sequential(*layers)

    def get_embedding_size(self) -> int:
        return self.hidden_dim

    # -- HIP execution ---------------------------------------------------------------------------
    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._engines = {}  # parameters moved: drop plans bound to old storage
        self._weights_generation = getattr(self, "_weights_generation", 0) + 1
        return out

    def _load_from_state_dict(self, *args, **kwargs):
        # reached by this encoder's own load_state_dict and by any parent's: what was computed from the old weights
        # (EmbeddingCache) is stale from here on
        self._weights_generation = getattr(self, "_weights_generation", 0) + 1
        return super()._load_from_state_dict(*args, **kwargs)

    def engine_for(self, x: torch.Tensor) -> EncoderEngine:
        if x.dim() == 3:
            n, h, w = x.shape
        else:
            n, _, h, w = x.shape
        key = (n, h, w, x.device)
        eng = self._engines.get(key)
        if eng is None:
            prepare_encoder_layout(self)
            eng = EncoderEngine(self, n, h, w, x.device)
            self._engines[key] = eng
        return eng

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not x.is_cuda:
            raise L.TspmError("ResNetEncoder (tspm_amd) runs on the MI355X only; move the model and inputs to the "
                              "ROCm device (there is no CPU fallback)")
        x = x.float()
        if x.dim() == 4 and not x.is_contiguous():
            x = x.contiguous()
        eng = self.engine_for(x)
        params = [p for p in self.parameters()]
        if self.training and torch.is_grad_enabled():
            return _EncoderFn.apply(x, self, eng, *params)
        emb = torch.empty(eng.N, self.hidden_dim, device=x.device, dtype=torch.float32)
        eng.forward(x, emb, self.hidden_dim, train=self.training)
        if self.training:
            self._fwd_generation += 1
        return emb


class _EncoderFn(torch.autograd.Function):
    """One autograd node for the whole encoder: forward = HIP schedule, backward = HIP schedule."""

    @staticmethod
    def forward(ctx, x, enc: ResNetEncoder, eng: EncoderEngine, *params):
        emb = torch.empty(eng.N, enc.hidden_dim, device=x.device, dtype=torch.float32)
        eng.forward(x, emb, enc.hidden_dim, train=True)
        enc._fwd_generation += 1
        ctx.enc, ctx.eng, ctx.gen = enc, eng, enc._fwd_generation
        ctx.n_params = len(params)
        return emb

    @staticmethod
    def backward(ctx, g):
        enc, eng = ctx.enc, ctx.eng
        if enc._fwd_generation != ctx.gen:
            raise L.TspmError("ResNetEncoder: another training forward ran before this backward; the HIP plan "
                              "keeps one set of saved activations per (batch, H, W)")
        g = g.contiguous().float()
        grads: Dict[int, torch.Tensor] = {}

        def grad_of(p):
            t = grads.get(id(p))
            if t is None:
                t = torch.empty_like(p, memory_format=torch.channels_last if p.dim() == 4 else torch.contiguous_format)
                grads[id(p)] = t
            return t

        eng.grad_of = grad_of
        try:
            eng.backward(g, enc.hidden_dim)
        finally:
            eng.grad_of = _engine_default_grad_of
        out = [grads.get(id(p)) for p in enc.parameters()]
        return (None, None, None, *out)


def _engine_default_grad_of(p):
    from .engine import _default_grad_of
    return _default_grad_of(p)


def ResNet18(in_channels: int = 1, hidden_dim: int = 128) -> ResNetEncoder:
    """resnet.py:222-229."""
    return ResNetEncoder(block=BasicBlock, layers=[2, 2, 2, 2], in_channels=in_channels, hidden_dim=hidden_dim)


def ResNet34(in_channels: int = 1, hidden_dim: int = 128) -> ResNetEncoder:
    """resnet.py:232-239."""
    return ResNetEncoder(block=BasicBlock, layers=[3, 4, 6, 3], in_channels=in_channels, hidden_dim=hidden_dim)


# ------------------------------------------------------------------------------------------------
# Fusion model
# ------------------------------------------------------------------------------------------------
def _ce_weight_of(loss_functions):
    from .step import _ce_weight
    return _ce_weight(loss_functions)


def modality_key(batch: Dict[Any, Any], name: str):
    """Find the batch key for modality ``name`` ('audio' / 'image').  The reference keys batches by
    ``modalities.Modality`` members (un-vendored package); accept those, plain strings, or any enum
    whose name/value is the modality name."""
    for k in batch.keys():
        if isinstance(k, str):
            if k.lower() == name:
                return k
            continue
        for attr in ("value", "name"):
            v = getattr(k, attr, None)
            if isinstance(v, str) and v.lower() == name:
                return k
        if str(k).lower().split(".")[-1] == name:
            return k
    raise KeyError(f"batch has no {name!r} modality key (keys: {list(batch.keys())})")


class _HeadFn(torch.autograd.Function):
    """Fusion head  Linear(192,128) → ReLU → Dropout → Linear(128,64) → ReLU → Linear(64,10)
    (models/avmnist.py:219-230) on libtspm kernels; dropout keep-mask drawn on device."""

    @staticmethod
    def forward(ctx, fused, model: "AVMNIST", w0, b0, w3, b3, w5, b5):
        n = fused.shape[0]
        dev = fused.device
        sh = L.stream_handle()
        lib = L.lib()
        hd, h2 = model.hidden_dim, model.hidden_dim // 2
        fused = fused.contiguous()
        h1 = torch.empty(n, hd, device=dev)
        hh = torch.empty(n, h2, device=dev)
        logits = torch.empty(n, NUM_CLASSES, device=dev)
        keep = None
        scale = 1.0
        if model.training and model.dropout_p > 0:
            keep = model._draw_keep(n * hd, dev).view(n, hd)
            scale = 1.0 / (1.0 - model.dropout_p)
        L.check(lib.tspm_linear_fwd(n, fused.shape[1], hd, fused.data_ptr(), fused.shape[1], w0.data_ptr(), b0.data_ptr(),
                                    1, L.ptr(keep), scale, h1.data_ptr(), hd, sh), "head fc0")
        L.check(lib.tspm_linear_fwd(n, hd, h2, h1.data_ptr(), hd, w3.data_ptr(), b3.data_ptr(), 1, None, 1.0,
                                    hh.data_ptr(), h2, sh), "head fc3")
        L.check(lib.tspm_linear_fwd(n, h2, NUM_CLASSES, hh.data_ptr(), h2, w5.data_ptr(), b5.data_ptr(), 0, None, 1.0,
                                    logits.data_ptr(), NUM_CLASSES, sh), "head fc5")
        ctx.save_for_backward(fused, h1, hh, w0, w3, w5)
        ctx.scale = scale
        return logits

    @staticmethod
    def backward(ctx, g):
        fused, h1, hh, w0, w3, w5 = ctx.saved_tensors
        g = g.contiguous().float()
        n = g.shape[0]
        sh = L.stream_handle()
        lib = L.lib()
        hd, h2 = h1.shape[1], hh.shape[1]
        dev = g.device
        gw5, gb5 = torch.empty_like(w5), torch.empty(w5.shape[0], device=dev)
        gw3, gb3 = torch.empty_like(w3), torch.empty(w3.shape[0], device=dev)
        gw0, gb0 = torch.empty_like(w0), torch.empty(w0.shape[0], device=dev)
        dh = torch.empty(n, h2, device=dev)
        dh1 = torch.empty(n, hd, device=dev)
        need_dx = ctx.needs_input_grad[0]  # False on frozen encoders (the head stage): nobody reads dfused
        dfused = torch.empty_like(fused) if need_dx else None
        L.check(lib.tspm_linear_bwd_weight(n, h2, NUM_CLASSES, hh.data_ptr(), h2, g.data_ptr(), NUM_CLASSES,
                                           gw5.data_ptr(), gb5.data_ptr(), sh), "head fc5 wgrad")
        L.check(lib.tspm_linear_bwd_data(n, h2, NUM_CLASSES, g.data_ptr(), NUM_CLASSES, w5.data_ptr(), dh.data_ptr(), h2,
                                         sh), "head fc5 dgrad")
        L.check(lib.tspm_act_bwd(n, h2, dh.data_ptr(), h2, hh.data_ptr(), h2, 1.0, sh), "head relu")
        L.check(lib.tspm_linear_bwd_weight(n, hd, h2, h1.data_ptr(), hd, dh.data_ptr(), h2, gw3.data_ptr(),
                                           gb3.data_ptr(), sh), "head fc3 wgrad")
        L.check(lib.tspm_linear_bwd_data(n, hd, h2, dh.data_ptr(), h2, w3.data_ptr(), dh1.data_ptr(), hd, sh),
                "head fc3 dgrad")
        L.check(lib.tspm_act_bwd(n, hd, dh1.data_ptr(), hd, h1.data_ptr(), hd, ctx.scale, sh), "head relu+dropout")
        F = fused.shape[1]
        L.check(lib.tspm_linear_bwd_weight(n, F, hd, fused.data_ptr(), F, dh1.data_ptr(), hd, gw0.data_ptr(),
                                           gb0.data_ptr(), sh), "head fc0 wgrad")
        if need_dx:
            L.check(lib.tspm_linear_bwd_data(n, F, hd, dh1.data_ptr(), hd, w0.data_ptr(), dfused.data_ptr(), F, sh),
                    "head fc0 dgrad")
        return dfused, None, gw0, gb0, gw3, gb3, gw5, gb5


class AVMNIST(nn.Module):
    """models/avmnist.py:188-410 drop-in (MultimodalMonitoringMixin hooks are not on the hot path)."""

    def __init__(self, audio_encoder: nn.Module, image_encoder: nn.Module, hidden_dim: int, *, dropout: float = 0.0,
                 fusion_fn: str = "concat") -> None:
        super().__init__()
        self.audio_encoder = audio_encoder
        self.image_encoder = image_encoder
        self.embd_size_A = audio_encoder.get_embedding_size()
        self.embd_size_I = image_encoder.get_embedding_size()
        self.hidden_dim = hidden_dim
        fc_fusion = nn.Linear(self.embd_size_A + self.embd_size_I, hidden_dim)
        fc_intermediate = nn.Linear(hidden_dim, hidden_dim // 2)
        fc_out = nn.Linear(hidden_dim // 2, NUM_CLASSES)
        self.dropout_p = float(dropout)
        self.net = nn.Sequential(fc_fusion, nn.ReLU(), nn.Dropout(dropout) if dropout > 0 else nn.Identity(),
                                 fc_intermediate, nn.ReLU(), fc_out)
        if fusion_fn.lower() != "concat":
            raise ValueError(f"Unknown fusion function: {fusion_fn}")
        self.fusion_fn = partial(torch.cat, dim=1)
        self._fused_step = None
        self._rng_seed = int(torch.initial_seed()) & ((1 << 63) - 1)
        self._rng_ctr = None
        self.keep_override: Optional[torch.Tensor] = None  # parity hook: inject the dropout keep-mask
        self._frozen_encoders: Tuple[str, ...] = ()  # freeze_encoders(): the encoders pinned to eval mode

    # -- the head stage: frozen, pre-trained encoders (this project's opt-in; the reference's pretrained YAML ends up
    #    with one all-trainable group and keeps that path) ------------------------------------------------
    ENCODERS = ("audio_encoder", "image_encoder")

    def freeze_encoders(self) -> "AVMNIST":
        """Freeze BOTH encoders for the second training stage (the fusion head on pre-trained encoders): their
        parameters get ``requires_grad_(False)`` and ``grad = None``, and the encoders are pinned to eval mode — a
        frozen encoder always runs on its running statistics, whatever ``train(mode)`` says, so its parameters,
        ``running_mean``, ``running_var`` and ``num_batches_tracked`` never change.  The head's dropout follows
        ``mode`` as before.  Build the optimizer AFTER this call (FusedAdam's flat buffers hold the trainable
        parameters only); ``train_step`` then runs ``step.FusedHeadStageStep``, and an ``all_patterns`` batch
        ``step.FusedHeadStagePatternStep``."""
        for name in self.ENCODERS:
            enc = getattr(self, name)
            for p in enc.parameters():
                p.requires_grad_(False)
                p.grad = None
            enc.eval()
        self._frozen_encoders = tuple(self.ENCODERS)
        self._freeze_generation = getattr(self, "_freeze_generation", 0) + 1
        self._fused_step = None
        return self

    def unfreeze_encoders(self) -> "AVMNIST":
        """Undo ``freeze_encoders``: every encoder parameter trainable again and the encoders back on the model's
        mode.  An optimizer built while they were frozen does not hold them: build a new one."""
        self._frozen_encoders = ()
        self._freeze_generation = getattr(self, "_freeze_generation", 0) + 1
        for name in self.ENCODERS:
            enc = getattr(self, name)
            for p in enc.parameters():
                p.requires_grad_(True)
            enc.train(self.training)
        self._fused_step = None
        return self

    def frozen_encoders(self) -> Tuple[str, ...]:
        """Names of the encoders ``freeze_encoders`` pinned: ``()`` or ``("audio_encoder", "image_encoder")``."""
        return getattr(self, "_frozen_encoders", ())

    def train(self, mode: bool = True) -> "AVMNIST":
        super().train(mode)
        for name in getattr(self, "_frozen_encoders", ()):  # a frozen encoder stays on its running statistics
            getattr(self, name).eval()
        return self

    # -- dropout mask --------------------------------------------------------------------------------
    def _draw_keep(self, count: int, dev: torch.device) -> torch.Tensor:
        if self.keep_override is not None:
            k = self.keep_override.to(device=dev, dtype=torch.uint8).reshape(-1)
            if k.numel() != count:
                raise L.TspmError("keep_override has the wrong number of elements")
            return k
        if self._rng_ctr is None or self._rng_ctr.device != dev:
            self._rng_ctr = torch.zeros(1, dtype=torch.int64, device=dev)
        keep = torch.empty(count, dtype=torch.uint8, device=dev)
        L.check(L.lib().tspm_dropout_mask(count, self.dropout_p, self._rng_seed, self._rng_ctr.data_ptr(),
                                          keep.data_ptr(), L.stream_handle()), "dropout_mask")
        self._rng_ctr.add_(1)
        return keep

    # -- forward (autograd path) ---------------------------------------------------------------------
    def forward(self, A: Optional[torch.Tensor] = None, I: Optional[torch.Tensor] = None, *, is_embd_A: bool = False,
                is_embd_I: bool = False) -> torch.Tensor:
        assert not all((A is None, I is None)), "At least one of A, I must be provided"
        assert not all([is_embd_A, is_embd_I]), "Cannot have all embeddings as True"
        ref = A if A is not None else I
        A = A if A is not None else torch.zeros(I.size(0), self.embd_size_A, device=ref.device)
        I = I if I is not None else torch.zeros(A.size(0), self.embd_size_I, device=ref.device)
        audio = self.audio_encoder(A) if not is_embd_A else A
        image = self.image_encoder(I) if not is_embd_I else I
        fused = self.fusion_fn((audio, image))
        n0, n3, n5 = self.net[0], self.net[3], self.net[5]
        return _HeadFn.apply(fused, self, n0.weight, n0.bias, n3.weight, n3.bias, n5.weight, n5.bias)

    # -- steps ---------------------------------------------------------------------------------------
    def _unpack(self, batch, device):
        ka, ki = modality_key(batch, "audio"), modality_key(batch, "image")
        A = batch[ka].to(device, non_blocking=True).float()
        I = batch[ki].to(device, non_blocking=True).float()
        labels = batch["labels"].to(device, non_blocking=True)
        return A, I, labels, batch.get("pattern_name")

    @staticmethod
    def _device_log(metric_recorder):
        from .metrics import DeviceMetricRecorder
        return metric_recorder.log if isinstance(metric_recorder, DeviceMetricRecorder) else None

    @staticmethod
    def _group_ids(batch, log, miss_type, device):
        g = batch.get("pattern_ids")
        if g is not None:
            return g.to(device, non_blocking=True)
        return log.group_ids(miss_type) if (log is not None and miss_type is not None) else None

    def train_step(self, batch: Dict[Any, Any], optimizer, loss_functions, device, metric_recorder, **kwargs):
        """models/avmnist.py:269-310.  Fused native step when possible (see module docstring).  With a
        metrics.DeviceMetricRecorder the batch's predictions are recorded on the device inside the step's
        HIP graph; with the reference's MetricRecorder they are copied to the host as the reference does."""
        from .step import FusedTrainStep, fused_step_supported
        if batch.get("cached"):
            return self._train_step_cached(batch, optimizer, loss_functions, device, metric_recorder)
        if batch.get("all_patterns"):
            return self._train_step_all_patterns(batch, optimizer, loss_functions, device, metric_recorder)
        A, I, labels, miss_type = self._unpack(batch, device)
        dlog = self._device_log(metric_recorder)
        if fused_step_supported(self, optimizer, loss_functions, A, I):
            if self._fused_step is None or not self._fused_step.matches(A, I, optimizer, loss_functions):
                from .step import FusedHeadStageStep, head_stage_frozen
                # the flags are read (and every unsupported combination refused) before anything is built
                if head_stage_frozen(self, optimizer):
                    self._fused_step = FusedHeadStageStep(self, optimizer, loss_functions, A.shape[0])
                else:
                    self._fused_step = FusedTrainStep(self, optimizer, loss_functions, A.shape[0])
            self._fused_step.log = dlog
            out = self._fused_step.step(A, I, labels, self._group_ids(batch, dlog, miss_type, device))
            logits = out["logits"]
            loss_t = out["loss"]
            if dlog is not None:
                return {"loss": float(loss_t.item())}
        else:
            self.train()
            optimizer.zero_grad()
            logits = self.forward(A=A, I=I)
            loss_t = loss_functions(logits, labels)["total_loss"]
            loss_t.backward()
            optimizer.step()
        if metric_recorder is not None:
            predictions = torch.softmax(logits.detach(), dim=1).argmax(dim=1).cpu().numpy()
            metric_recorder.update_group_all("classification", predictions=predictions,
                                             targets=labels.detach().cpu().numpy(),
                                             m_types=np.array(miss_type if miss_type is not None else []))
        return {"loss": float(loss_t.item())}

    def _train_step_all_patterns(self, batch, optimizer, loss_functions, device, metric_recorder):
        """An ``"all_patterns"`` batch (data.AVMNIST.device_loader(all_patterns=True): the samples once, unmasked): one
        ``FusedHeadStagePatternStep`` — the head trained under every pattern of the batch, on frozen encoders."""
        from .step import FusedHeadStagePatternStep, fused_step_supported, head_stage_frozen, norm_avmnist_patterns
        A, I, labels, _ = self._unpack(batch, device)
        if not fused_step_supported(self, optimizer, loss_functions, A, I):
            raise L.TspmError("an all_patterns batch runs on the fused head-stage step only: it needs this package's "
                              "FusedAdam, a single cross-entropy loss term, device tensors and a fusion head within "
                              "tspm_head_train_step's limits")
        pats = norm_avmnist_patterns(batch["patterns"])
        st = self.__dict__.get("_fused_pattern_step")
        if st is None or not st.matches(A, I, optimizer, loss_functions, pats):
            if not head_stage_frozen(self, optimizer, all_patterns=True):
                raise AssertionError("unreachable: head_stage_frozen(all_patterns=True) refuses an unfrozen model")
            st = FusedHeadStagePatternStep(self, optimizer, loss_functions, A.shape[0], patterns=pats)
            self.__dict__["_fused_pattern_step"] = st
        st.log = self._device_log(metric_recorder)
        out = st.step(A, I, labels, refresh_zero=True)
        if metric_recorder is not None and st.log is None:
            P = len(pats)
            predictions = torch.softmax(out["logits"].detach().reshape(P * A.shape[0], -1), dim=1).argmax(dim=1)
            metric_recorder.update_group_all("classification", predictions=predictions.cpu().numpy(),
                                             targets=np.tile(labels.detach().cpu().numpy(), P),
                                             m_types=np.repeat(np.array(pats), A.shape[0]))
        return {"loss": float(out["loss"].item())}

    # -- the head stage on cached embeddings (EmbeddingCache below; batches of an ``ids_only`` loader) ----------
    def _cache_of(self, batch) -> "EmbeddingCache":
        """The embedding cache a ``"cached"`` batch reads: its dataset's cache of this model (filled here, over the
        whole split, if no epoch runner or ``fit`` has built it yet)."""
        ds = batch.get("dataset")
        if ds is None or not hasattr(ds, "embedding_cache"):
            raise L.TspmError('a "cached" batch names its dataset under "dataset" (data.DeviceLoader(ids_only=True) does)')
        return ds.embedding_cache(self)

    def _train_step_cached(self, batch, optimizer, loss_functions, device, metric_recorder):
        """A ``"cached"`` train batch (data.AVMNIST.device_loader(ids_only=True)): one ``FusedCachedHeadStep`` on the
        dataset's embedding cache of this model — every pattern of the batch for an ``"all_patterns"`` batch, else one
        pattern per sample from the batch's ``"keep"`` flags."""
        from .step import FusedCachedHeadStep, norm_avmnist_patterns, train_step_key
        cache = self._cache_of(batch)
        ids = batch["sample_ids"]
        pats = norm_avmnist_patterns(batch["patterns"]) if batch.get("all_patterns") else None
        key = train_step_key(self, int(ids.numel()), pats, cached=True) + (id(optimizer), id(loss_functions), id(cache))
        steps = self.__dict__.setdefault("_fused_cached_steps", {})
        st = steps.get(key)
        if st is None:
            st = FusedCachedHeadStep(self, optimizer, loss_functions, int(ids.numel()), cache, patterns=pats,
                                     per_sample=pats is None)
            steps[key] = st
        dlog = self._device_log(metric_recorder)
        if metric_recorder is not None and dlog is None:
            raise L.TspmError("a cached batch records its predictions on the device: train_step needs a "
                              "metrics.DeviceMetricRecorder (or use the default loader)")
        st.log = dlog
        if pats is None:
            out = st.step(ids, batch["keep"], batch.get("pattern_ids"))
        else:
            out = st.step(ids)
        return {"loss": float(out["loss"].item())}

    def _validation_step_cached(self, batch, loss_functions, device, metric_recorder):
        """A ``"cached"`` valid / test batch: one ``FusedCachedEvalStep`` on the dataset's embedding cache."""
        from .step import FusedCachedEvalStep, norm_avmnist_patterns
        dlog = self._device_log(metric_recorder)
        if dlog is None:
            raise L.TspmError("a cached batch records its losses and predictions on the device: validation_step needs "
                              "a metrics.DeviceMetricRecorder (or use the default loader)")
        cache = self._cache_of(batch)
        ids = batch["sample_ids"]
        pats = norm_avmnist_patterns(batch["patterns"]) if batch.get("fused_patterns") else None
        key = (pats, int(ids.numel()), id(cache), _ce_weight_of(loss_functions))
        steps = self.__dict__.setdefault("_fused_cached_eval", {})
        st = steps.get(key)
        if st is None:
            st = FusedCachedEvalStep(self, loss_functions, int(ids.numel()), cache, dlog, patterns=pats,
                                     per_sample=pats is None)
            steps[key] = st
        st.log = dlog
        self.eval()
        with torch.no_grad():
            out = st.step(ids) if pats is not None else st.step(ids, batch["keep"], batch.get("pattern_ids"))
            return {"loss": float(out["loss"].mean().item())}

    def eval_step_for(self, loss_functions, batch: int, log=None):
        """The cached FusedEvalStep for this batch size (one HIP graph per size)."""
        from .step import FusedEvalStep
        cache = self.__dict__.setdefault("_fused_eval", {})
        st = cache.get(batch)
        if st is None or st.ce_weight != _ce_weight_of(loss_functions):
            st = FusedEvalStep(self, loss_functions, batch, log)
            cache[batch] = st
        st.log = log
        return st

    # -- every missing-modality pattern of a batch from one encoder pass --------------------------------
    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        # parameters moved (the encoders drop their engines here too): the zero-input embeddings and the steps
        # whose graphs read them are bound to the old storage
        self.__dict__.pop("_zero_emb", None)
        self.__dict__.pop("_fused_pattern_eval", None)
        self.__dict__.pop("_fused_pattern_step", None)
        self.__dict__.pop("_fused_cached_steps", None)
        self.__dict__.pop("_fused_cached_eval", None)
        return out

    def zero_embeddings(self, refresh: bool = True, audio_hw=(32, 94), image_hw=(28, 28)) -> torch.Tensor:
        """``[embd_size_A + embd_size_I]``: each encoder's eval-mode embedding of an all-zero input (what a pattern
        that drops the modality feeds the head; with BatchNorm on running statistics it is the same row for every
        sample).  One device buffer per model with a stable address (captured graphs read it), dropped with the
        encoders' engines when the parameters move.  ``refresh``: recompute it — each encoder's forward on a one-row
        zero input, the two encoders on two streams; a new buffer is always filled.  FusedAdam writes parameters
        through raw pointers, so nothing here can tell whether the weights changed: callers refresh unless they know
        they did not (inside one evaluation epoch)."""
        dev = next(self.parameters()).device
        key = (tuple(audio_hw), tuple(image_hw))
        z = self.__dict__.get("_zero_emb")
        if z is None or z["key"] != key or z["emb"].device != dev:
            f32 = dict(device=dev, dtype=torch.float32)
            z = {"key": key, "emb": torch.zeros(1, self.embd_size_A + self.embd_size_I, **f32),
                 "A": torch.zeros(1, *audio_hw, **f32), "I": torch.zeros(1, 1, *image_hw, **f32)}
            self._zero_emb = z
            refresh = True
        if refresh:
            F, ea = z["emb"].shape[1], self.embd_size_A  # train=False below: running statistics, whatever the mode flag
            main, side = torch.cuda.current_stream(), L.shared_streams(dev, 1)[0]
            with torch.no_grad():
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    self.image_encoder.engine_for(z["I"]).forward(z["I"], z["emb"][:, ea:], F, train=False)
                self.audio_encoder.engine_for(z["A"]).forward(z["A"], z["emb"], F, train=False)
                main.wait_stream(side)
        return z["emb"][0]

    def pattern_eval_step_for(self, loss_functions, batch: int, log=None, patterns=None, head: Optional[str] = None):
        """The cached FusedPatternEvalStep for (patterns, head, batch size) — kept apart from ``eval_step_for``'s."""
        from .step import DEFAULT_PATTERN_HEAD, FusedPatternEvalStep, norm_avmnist_patterns
        pats = norm_avmnist_patterns(patterns)
        key = (pats, head or DEFAULT_PATTERN_HEAD, batch)
        cache = self.__dict__.setdefault("_fused_pattern_eval", {})
        st = cache.get(key)
        if st is None or st.ce_weight != _ce_weight_of(loss_functions):
            st = FusedPatternEvalStep(self, loss_functions, batch, log, patterns=pats, head=head)
            cache[key] = st
        st.log = log
        return st

    def forward_patterns(self, A: torch.Tensor, I: torch.Tensor, patterns=None) -> torch.Tensor:
        """Eval-mode logits ``[P, B, C]`` of the batch under each of ``patterns`` (default ``("a", "ai", "i")``; a
        subset in any order) from one encoder pass, under ``no_grad``; the zero embeddings are refreshed first."""
        dev = next(self.parameters()).device
        was_training = self.training
        try:
            with torch.no_grad():
                A = A.to(dev, non_blocking=True).float()
                I = I.to(dev, non_blocking=True).float()
                st = self.pattern_eval_step_for(None, A.shape[0], None, patterns)
                labels = torch.zeros(A.shape[0], dtype=torch.int64, device=dev)
                return st.step(A, I, labels, refresh_zero=True)["logits"].clone()
        finally:
            if was_training:
                self.train()

    def _validation_step_patterns(self, batch, loss_functions, device, metric_recorder):
        """A ``"fused_patterns"`` batch (data.AVMNIST.device_loader(fuse_patterns=True): the samples once, unmasked)."""
        dlog = self._device_log(metric_recorder)
        if dlog is None:
            raise L.TspmError("a fused-pattern batch records its per-pattern losses and predictions on the device: "
                              "validation_step needs a metrics.DeviceMetricRecorder (or use the default loader)")
        self.eval()
        with torch.no_grad():
            A, I, labels, _ = self._unpack(batch, device)
            st = self.pattern_eval_step_for(loss_functions, A.shape[0], dlog, batch["patterns"])
            out = st.step(A, I, labels, refresh_zero=True)
            return {"loss": float(out["loss"].mean().item())}

    def validation_step(self, batch, loss_functions, device, metric_recorder, return_test_info: bool = False):
        """models/avmnist.py:312-360 (eval-mode BN running stats, dropout off).  With a single
        cross-entropy loss group the batch runs as one FusedEvalStep graph (predictions recorded on the
        device when metric_recorder is a metrics.DeviceMetricRecorder)."""
        if batch.get("cached"):
            return self._validation_step_cached(batch, loss_functions, device, metric_recorder)
        if batch.get("fused_patterns"):
            return self._validation_step_patterns(batch, loss_functions, device, metric_recorder)
        self.eval()
        with torch.no_grad():
            A, I, labels, miss_type = self._unpack(batch, device)
            dlog = self._device_log(metric_recorder)
            if (_ce_weight_of(loss_functions) is not None and A.is_cuda and I.is_cuda and A.dim() == 3
                    and tuple(A.shape[1:]) == (32, 94) and tuple(I.shape[-2:]) == (28, 28)):
                st = self.eval_step_for(loss_functions, A.shape[0], dlog)
                out = st.step(A, I, labels, self._group_ids(batch, dlog, miss_type, device))
                if dlog is not None and not return_test_info:
                    return {"loss": out["loss"].item()}
                loss = out["loss"]
                predictions = out["preds"].cpu().numpy()
            else:
                logits = self.forward(A=A, I=I)
                loss = loss_functions(logits, labels)["total_loss"]
                predictions = torch.softmax(logits, dim=1).argmax(dim=1).cpu().numpy()
            labels_np = labels.cpu().numpy()
            miss_type = np.array(miss_type if miss_type is not None else [])
            if metric_recorder is not None and dlog is None:
                metric_recorder.update_group_all(group_name="classification", predictions=predictions,
                                                 targets=labels_np, m_types=miss_type)
            if return_test_info:
                return {"loss": loss.item(), "predictions": predictions, "labels": labels_np, "miss_types": miss_type}
        return {"loss": loss.item()}

    def get_embeddings(self, dataloader, device) -> Dict[Any, Any]:
        """models/avmnist.py:362-401."""
        embeddings = defaultdict(list)
        self.to(device)
        self.eval()
        for batch in dataloader:
            with torch.no_grad():
                ka, ki = modality_key(batch, "audio"), modality_key(batch, "image")
                A, I, miss_type = batch[ka], batch[ki], np.array(batch["pattern_name"])
                A = A[miss_type == "ai"].to(device).float()
                I = I[miss_type == "ai"].to(device).float()
                embeddings[ka].append(self.audio_encoder(A).detach().cpu().numpy())
                embeddings[ki].append(self.image_encoder(I).detach().cpu().numpy())
                embeddings["label"] += list(batch["labels"])
        return embeddings

    def get_encoder(self, modality) -> nn.Module:
        name = str(getattr(modality, "value", modality)).lower().split(".")[-1]
        if name == "audio":
            return self.audio_encoder
        if name == "image":
            return self.image_encoder
        raise ValueError(f"Unknown modality: {modality}")


# ------------------------------------------------------------------------------------------------
# The frozen encoders' embeddings of a whole split, computed once (the head stage without the encoders)
# ------------------------------------------------------------------------------------------------
class EmbeddingCache:
    """Both frozen encoders' eval-mode embeddings of every sample of a device corpus: ``emb [num_samples][F]`` fp32
    (``F = embd_size_A + embd_size_I``, audio columns first; 60,000 x 192 x 4 B = 46 MB), ``labels_all [num_samples]``
    int64 (the corpus' own label tensor) and ``x0 [F]``, the model's ``zero_embeddings(refresh=True)`` buffer — what a
    pattern that drops a modality feeds the head.  A frozen encoder runs on its running statistics, so each row is a
    function of that sample and of weights that never move: the cache is a constant of the whole head stage, and
    ``step.FusedCachedHeadStep`` / ``FusedCachedEvalStep`` read it by sample index instead of running the encoders.

    The fill (``refresh()``) runs both encoders' eval forward over the corpus in sample order, unmasked, in chunks of
    ``chunk`` rows plus one shorter last chunk, the image encoder on the side stream as the head-stage steps run it,
    writing straight into ``emb``.  It is refused for a model whose encoders are not frozen.

    The cache remembers the model's frozen encoders, its freeze generation, each encoder's weights generation and the
    identity of the encoders' engine tables.  ``unfreeze_encoders()``, ``load_state_dict`` on the model or on an
    encoder, and anything that drops the engines (``.to()``) make it stale; a stale cache is refused at its next use
    with a ``TspmError`` that says to call ``refresh()``.  Weights written through raw pointers (FusedAdam's flat
    buffers, an in-place ``copy_``) cannot be detected, as ``AVMNIST.zero_embeddings`` says of itself: callers who
    change frozen weights that way call ``refresh()``."""

    def __init__(self, model: "AVMNIST", device_corpus, chunk: int = 256):
        if int(chunk) < 1:
            raise ValueError("chunk must be >= 1")
        # the model is held weakly: the dataset's table of caches is keyed by the model and must not keep it alive
        self._model_ref, self.dc, self.chunk = weakref.ref(model), device_corpus, int(chunk)
        self.n = int(device_corpus.n)
        self.ea = int(model.embd_size_A)
        self.F = self.ea + int(model.embd_size_I)
        self.audio_hw, self.image_hw = tuple(device_corpus.audio_shape), tuple(device_corpus.image_shape)
        self.emb: Optional[torch.Tensor] = None
        self.labels_all = device_corpus.labels
        self.x0: Optional[torch.Tensor] = None
        self.fill_seconds = 0.0
        self.fills = 0
        self._stamp = None
        self.refresh()

    @property
    def model(self) -> "AVMNIST":
        m = self._model_ref()
        if m is None:
            raise L.TspmError("this EmbeddingCache's model no longer exists")
        return m

    def _now(self):
        m = self.model
        return (tuple(m.frozen_encoders()), getattr(m, "_freeze_generation", 0),
                getattr(m.audio_encoder, "_weights_generation", 0), getattr(m.image_encoder, "_weights_generation", 0),
                m.audio_encoder._engines, m.image_encoder._engines)

    def stale_reason(self) -> Optional[str]:
        """None while the cache is current, else what changed since the fill."""
        was, now = self._stamp, self._now()
        if now[0] != was[0] or now[1] != was[1]:
            return "the model's encoders were unfrozen (or frozen again) since the fill"
        if now[2] != was[2] or now[3] != was[3] or now[4] is not was[4] or now[5] is not was[5]:
            return "an encoder's weights were loaded or moved (load_state_dict, .to()) since the fill"
        return None

    def check(self, model=None) -> "EmbeddingCache":
        """Refuse a cache built for another model, and a stale one."""
        if model is not None and model is not self.model:
            raise L.TspmError("this EmbeddingCache was built for another model: its rows are that model's encoders' "
                              "embeddings (dataset.embedding_cache(model) builds this model's)")
        why = self.stale_reason()
        if why is not None:
            raise L.TspmError(f"stale EmbeddingCache: {why}; call refresh() on it (with the encoders frozen) before "
                              "the next use")
        return self

    def refresh(self) -> "EmbeddingCache":
        """(Re)compute every row and the zero-input row; returns self."""
        import time
        from .step import head_stage_frozen
        model, dc = self.model, self.dc
        if not head_stage_frozen(model):
            raise L.TspmError("EmbeddingCache: the model's encoders are not frozen (AVMNIST.freeze_encoders()); a "
                              "trainable encoder's embeddings change every step and its BatchNorm runs on batch "
                              "statistics, so there is nothing constant to cache")
        dev = next(model.parameters()).device
        if dev != dc.device:
            raise L.TspmError(f"EmbeddingCache: the model is on {dev}, the corpus on {dc.device}")
        f32 = dict(device=dev, dtype=torch.float32)
        if self.emb is None or self.emb.device != dev:
            self.emb = torch.empty(self.n, self.F, **f32)
        n, F, ea, ch = self.n, self.F, self.ea, min(self.chunk, max(self.n, 1))
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        main, side = torch.cuda.current_stream(), L.shared_streams(dev, 1)[0]
        order = torch.arange(n, dtype=torch.int64, device=dev)
        bufs = {}
        with torch.no_grad():
            for lo in range(0, n, ch):
                b = min(ch, n - lo)
                if b not in bufs:
                    bufs[b] = (torch.empty(b, *self.audio_hw, **f32), torch.empty(b, 1, *self.image_hw, **f32),
                               torch.empty(b, dtype=torch.int64, device=dev))
                A, I, lab = bufs[b]
                dc.gather(order[lo:lo + b], None, None, out=(A, I, lab))
                rows = self.emb[lo:lo + b]
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    model.image_encoder.engine_for(I).forward(I, rows[:, ea:], F, train=False)
                model.audio_encoder.engine_for(A).forward(A, rows, F, train=False)
                main.wait_stream(side)  # the next chunk's gather overwrites I
        self.x0 = model.zero_embeddings(refresh=True, audio_hw=self.audio_hw, image_hw=self.image_hw)
        torch.cuda.synchronize(dev)
        self.fill_seconds = time.perf_counter() - t0
        self.fills += 1
        self._stamp = self._now()
        return self
