"""MOSI UTT-Fusion on the HIP path (BASELINE.json configs[4]).

Drop-ins for the reference's classes, same constructor arguments, attribute names and ``state_dict``
keys (MML_Suite paths):

* ``LSTMEncoder``     models/msa/networks/lstm.py:8-67   (``rnn`` = nn.LSTM parameter container, "last" /
                      "maxpool" / "attention")
* ``TextCNN``         models/msa/networks/textcnn.py:10-69
* ``FcClassifier``    models/msa/networks/classifier.py:83-117
* ``UttFusionModel``  models/msa/utt_fusion.py:25-294 (forward, train_step with clip_grad_norm_,
                      validation_step, get_embeddings, get_encoder)

configs/mosi/centralised/utt_fusion_base_training.yaml: LSTM 5→64 (audio) and 20→64 (video), TextCNN
over 768-d text (3 x 128 filters of heights 3/4/5, dropout 0.5, Linear 384→64 + ReLU), FcClassifier
192 → 192/64/32 → 3 (ReLU + dropout 0.5 per layer), cross-entropy, clip 1.0, Adam lr 1e-3 / wd 1e-3.
configs/mosei/centralised/utt_fusion_train_mosei.yaml (the same model on CMU-MOSEI): LSTM 74→64 and 35→64
with the "maxpool" embedding, TextCNN dropout 0.7, FcClassifier 192 → 96/48 → 3 with ``use_bn`` (Linear →
ReLU → BatchNorm1d → Dropout 0.66), clip 0.5, Adam lr 2e-4 / wd 1e-5, batch 256.

``MosiEngine`` is the step's kernel schedule for a fixed (batch, steps): inputs time-major on the device
([T][B][F], rows (t, b)); LSTM input projections and weight gradients on the MFMA GEMM
(``tspm_linear_*``), the recurrences in ``tspm_lstm_fwd/bwd`` (both encoders in one launch each; with an LSTM
``hidden_size`` other than 64 — any multiple of 4 up to 128, each encoder its own — ``tspm_lstm_fwd_w/bwd_w``), the
TextCNN convolutions on the LDS-staged implicit-GEMM conv kernel (a (h, 768) kernel over [B,1,T,768]
is a 1-D convolution with 768 input channels; the reference's [C,1,h,768] weight is already its OHWI
layout), pooling + dropout in ``tspm_textcnn_pool_fwd``, the sparse TextCNN weight gradient in
``tspm_textcnn_bwd``, the classifier on the small-GEMM kernel, cross-entropy, the clip coefficient
(``tspm_grad_clip_coef``) and Adam (``tspm_adam_step_clip``).  ``FusedMosiStep`` captures all of it as
one HIP graph.

``steps`` is an ``int`` or a triple ``(Ta, Tv, Tt)`` (``norm_steps``) everywhere: on the unaligned CMU-MOSI / CMU-MOSEI files
audio, video and text keep their own frame rates and the reference's ``pad_sequence`` collate pads each modality to its own
batch maximum, so the engine plans every modality's buffers, gather helpers and weight-gradient split at its own length; a
triple of equal numbers is the ``int`` (same cached engine, step and graph, same launches as before).  A launch with a
"maxpool" encoder of more than 256 steps takes ``tspm_lstm_fwd_t16/bwd_t16`` and 16-bit index buffers
(``_lib.lstm_wide_index``); the text length stays within the TextCNN kernels' 255 steps.

Per-sample sequence lengths (this project's addition; the reference runs the padded length): ``ragged`` engines and steps
(``UttFusionModel.forward(..., lengths=...)``, ``fused_step(..., ragged=True)``, ``LSTMEncoder.forward(x, lengths)``) run
the recurrences through ``tspm_lstm_fwd_len/bwd_len`` on persistent ``int32 [B]`` device length buffers, one per LSTM
encoder: each row's state freezes at its own last step (``pack_padded_sequence`` semantics), the buffers are refreshed
device-to-device before each replay, and one captured graph serves every batch of a padded ``steps``.  ``ragged`` is a
trailing element of every cache key, so the keys without it are unchanged.  The text modality's lengths are a separate
opt-in, ``text_lengths`` (``fused_step(..., text_lengths=True)``, a ``"text"`` key in ``lengths``, ``TextCNN.forward(x,
lengths)``): the pooling runs in ``tspm_textcnn_pool_fwd_len`` over each row's own windows on one more ``int32 [B]`` buffer
— the TextCNN of the row's first ``L_b`` steps, whatever the padding — independent of ``ragged`` and a further trailing
key element.  The loaders' zero padding is a precondition for rows shorter than a kernel height (include/tspm.h).

Frozen encoders and several Adam groups (the second stage on pre-trained encoders): an encoder module (``netA`` /
``netV`` / ``netT``) none of whose parameters has ``requires_grad`` is frozen — PyTorch's semantics: the forward is
unchanged (the training-mode TextCNN dropout of a frozen ``netT`` included), its backward is skipped and its parameters
get no gradient and no update.  ``MosiEngine`` learns the frozen set when it is built (a trailing ``("frozen", names)``
element of the engine and ``fused_step`` keys, only when something is frozen); ``FusedMosiStep`` takes a ``FusedAdam`` of
1..8 param groups (``finetune_param_groups`` builds the usual ones) and keeps the optimizer phase at four launches for
any number of them (``tspm_grad_clip_coef_multi``, ``tspm_adam_begin_multi``, ``tspm_adam_step_multi``).  Mixed flags
inside a module, a ``netC`` that is not fully trainable, a trainable parameter in no group, ``allreduce`` with several
groups, and a ``FusedAdam`` whose flat buffers (fixed when it was built) are not exactly the parameters that train now
are refused (``check_param_groups``): set the flags first, then build the optimizer.

The "attention" embedding of the LSTM encoders (lstm.py:21-44): ``LSTMEncoder(..., embd_method="attention",
attention_norm="time" | "unit")`` pools every LSTM output, e = sum_t alpha_t r_t, in ``tspm_attn_pool_fwd`` after the recurrence
(with "time" the score projection tanh(W r_t + c) . u runs on ``tspm_linear_fwd`` over the T*B rows first); the backward is
``tspm_attn_pool_bwd``, the projection's two gradient GEMMs and ``tspm_lstm_bwd_seq``, the backward through time with a
gradient at every step.  Such an encoder always runs the length-taking entry points (its length buffer stays at the padded
length without ``ragged``); the encoders' methods are fixed at construction, so no cache key changes.

Every missing-modality pattern of a batch from one eval pass (this project's addition, opt-in, eval only):
under any pattern a modality is the real input or the zeroed input, so ``MosiPatternEngine`` runs the encoders once over
2B rows (the batch and zero rows), ``tspm_pattern_expand`` builds the P*B classifier rows, labels and group ids, and the
classifier runs once on them — ``UttFusionModel.forward_patterns``, ``FusedMosiPatternEvalStep`` (the per-pattern loss and
metrics launches on row slices: the same log entries as P replays of ``FusedMosiEvalStep``) and
``mosi_data.MOSI.loader(fuse_patterns=True)``.  Its cache keys start with a ("patterns", names) element; no other changes.

Training every pattern of a batch in one step (this project's addition, opt-in; the reference draws one random
pattern per sample, and that path is unchanged): ``FusedMosiPatternStep`` (``UttFusionModel.fused_pattern_step``, an
``"all_patterns"`` batch in ``train_step``, ``mosi_data.MOSI.loader(all_patterns=True)``) runs ``MosiPatternEngine(backward=
True)`` - the encoders forward and backward over the same 2B rows, the classifier over the P*B expanded rows, and between
them ``tspm_pattern_expand_bwd``, the expansion's adjoint, which folds the [P*B, E] classifier-input gradient onto the
[2B, E] encoder rows (ascending-p fp32 sums, no atomics; a frozen encoder's columns untouched).  The loss is the weighted
mean over all P*B rows - a plain step on the replicated batch cat_p(A*ka_p, V*kv_p, T*kt_p); BatchNorm1d takes its
statistics over the P*B rows and updates its running statistics once per step; the TextCNN dropout mask is drawn per
encoder row (2B; shared by the patterns that read the row), the classifier masks per classifier row (P*B).

Sentiment regression (this project's addition; the reference's YAMLs train the three-class variant only): a
one-output ``netC.fc_out`` (``build_utt_fusion(name, output_dim=1)``) with a single mean ``nn.L1Loss`` / ``nn.MSELoss``
term (``_regress_term``) on the float32 ``regression_labels`` runs the same steps with the head — ``fc_out``, the loss,
the per-pattern epoch accumulators, the loss log and ``fc_out``'s backward — in the one launch of
``MosiEngine.head_regress`` (``tspm_regress_head_step``).
"""
from __future__ import annotations

import ctypes
import os
from collections import defaultdict
from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from ._lib import linear_bwd
from .optim import FusedAdam

NUM_CLASSES = 3  # data/mosi.py:26 (classification_labels)
_CLS_SEED_SALT = 0x6A09E667F3BCC909  # the classifier masks' seed = model seed ^ salt (independent of the text masks)
PATTERNS = {"atv": (1.0, 1.0, 1.0), "at": (1.0, 1.0, 0.0), "av": (1.0, 0.0, 1.0), "tv": (0.0, 1.0, 1.0),
            "a": (1.0, 0.0, 0.0), "t": (0.0, 1.0, 0.0), "v": (0.0, 0.0, 1.0)}  # (audio, text, video) data/mosi.py:60-68


# The model / optimizer blocks of the two UTT-Fusion YAMLs (configs/mosi/centralised/utt_fusion_base_training.yaml,
# configs/mosei/centralised/utt_fusion_train_mosei.yaml): what build_utt_fusion constructs, in YAML order.
YAML_CONFIGS = {
    "mosi": dict(audio_dim=5, video_dim=20, text_dim=768, embd_method="last", text_dropout=0.5, cls_layers=(192, 64, 32),
                 cls_dropout=0.5, use_bn=False, clip=1.0, lr=1e-3, weight_decay=1e-3, batch=128),
    "mosei": dict(audio_dim=74, video_dim=35, text_dim=768, embd_method="maxpool", text_dropout=0.7, cls_layers=(96, 48),
                  cls_dropout=0.66, use_bn=True, clip=0.5, lr=2e-4, weight_decay=1e-5, batch=256),
}


def build_utt_fusion(name: str = "mosi", output_dim: int = 3,
                     embd_sizes: Sequence[int] = (64, 64, 64), embd_method: Optional[str] = None,
                     attention_norm: Optional[str] = None) -> "UttFusionModel":
    """UttFusionModel of the named YAML (netA, netV, netT, netC constructed in the YAML's order, so a
    ``torch.manual_seed`` before the call gives the reference's initial weights).  ``output_dim=1`` builds the
    sentiment-regression model (``regression_labels``: a continuous score in [-3, 3]); only ``netC.fc_out``, the last
    module constructed, differs from the default build of the same seed.  ``embd_sizes`` = the (audio, video, text)
    embedding widths (the YAMLs' ``hidden_size`` / ``embd_size`` fields; the LSTM widths within
    ``L.lstm_width_supported``); the classifier's input is their sum.  ``embd_method`` (default: the YAML's) and
    ``attention_norm`` go to both LSTM encoders (``LSTMEncoder``: "attention" needs ``attention_norm`` "time" or
    "unit")."""
    c = YAML_CONFIGS[name]
    ha, hv, ht = (int(w) for w in embd_sizes)
    method = c["embd_method"] if embd_method is None else embd_method
    kw = {} if attention_norm is None else dict(attention_norm=attention_norm)  # the two-argument call as it was
    netA = LSTMEncoder(input_size=c["audio_dim"], hidden_size=ha, embd_method=method, **kw)
    netV = LSTMEncoder(input_size=c["video_dim"], hidden_size=hv, embd_method=method, **kw)
    netT = TextCNN(input_size=c["text_dim"], embd_size=ht, dropout=c["text_dropout"], in_channels=1, out_channels=128,
                   kernel_heights=[3, 4, 5])
    netC = FcClassifier(input_dim=ha + hv + ht, layers=list(c["cls_layers"]), output_dim=output_dim, dropout=c["cls_dropout"],
                        use_bn=c["use_bn"])
    return UttFusionModel(netA, netV, netT, netC, clip=c["clip"])


# ------------------------------------------------------------------------------------------------
# parameter containers (reference attribute names / state_dict keys / construction order)
# ------------------------------------------------------------------------------------------------
ATTENTION_NORMS = ("time", "unit")
_ATTENTION_VECTOR_SEED = 0x5EED_A77E  # the private generator that fills attention_vector_weight


class LSTMEncoder(nn.Module):
    """lstm.py:8-67: one-directional nn.LSTM(batch_first=True); embd "last" = h_n, "maxpool" = max over
    time of r_out (lstm.py:47-52, F.max_pool1d: first maximum), "attention" = sum_t alpha_t r_t (lstm.py:21-44).

    "attention" (DESIGN §3.16): s_t = tanh(W r_t + c) . u with ``attention_layer`` = Sequential(Linear(H, H), Tanh())
    and ``attention_vector_weight`` [H, 1] (the reference's names, shapes and construction order, so the ``state_dict``
    keys are its own).  The normalisation of the scores must be chosen with ``attention_norm``:

    * ``"time"``  alpha = softmax of s over the row's time steps - the Hierarchical-Attention formula the reference's
      docstring describes;
    * ``"unit"``  alpha_t = 1 on every valid step, the embedding is the plain time-sum - what a softmax over the
      trailing size-1 axis of [B, T, 1] scores computes (the reference's code as recalled; checkpoint interoperability).

    Without ``attention_norm`` the method keeps raising ``NotImplementedError``.  ``attention_layer``'s Linear draws from
    the global RNG in its place; the vector, which the reference leaves uninitialised (``torch.Tensor(H, 1)``), is filled
    U(-1/sqrt(H), 1/sqrt(H)) from a private generator of fixed seed and consumes no global RNG."""

    def __init__(self, input_size: int, hidden_size: int, embd_method: str = "last",
                 attention_norm: Optional[str] = None):
        super().__init__()
        self.input_size = input_size
        self.hidden_size = hidden_size
        self.rnn = nn.LSTM(self.input_size, self.hidden_size, batch_first=True)
        assert embd_method in ["maxpool", "attention", "last"]
        if attention_norm is not None and embd_method != "attention":
            raise L.TspmError(f"LSTMEncoder: attention_norm={attention_norm!r} goes with embd_method='attention', not "
                              f"{embd_method!r}")
        if embd_method == "attention":
            if attention_norm is None:
                raise NotImplementedError(
                    "LSTMEncoder HIP path: embd_method='attention' needs attention_norm - choose 'time' (softmax of the "
                    "scores over the row's time steps, the formula of the reference's docstring) or 'unit' (every weight "
                    "1, the plain time-sum: what the reference's Softmax(dim=-1) over [B, T, 1] scores computes)")
            if attention_norm not in ATTENTION_NORMS:
                raise L.TspmError(f"LSTMEncoder: attention_norm is one of {ATTENTION_NORMS}, got {attention_norm!r}")
            self.attention_vector_weight = nn.Parameter(torch.empty(self.hidden_size, 1))
            self.attention_layer = nn.Sequential(nn.Linear(self.hidden_size, self.hidden_size), nn.Tanh())
            self.softmax = nn.Softmax(dim=-1)
            bound = 1.0 / float(self.hidden_size) ** 0.5
            with torch.no_grad():
                self.attention_vector_weight.uniform_(
                    -bound, bound, generator=torch.Generator().manual_seed(_ATTENTION_VECTOR_SEED))
        self.embd_method = embd_method
        self.attention_norm = attention_norm
        self._weights_generation = 0  # bumped by load_state_dict and by anything that moves the parameters

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._weights_generation = getattr(self, "_weights_generation", 0) + 1
        return out

    def _load_from_state_dict(self, *args, **kwargs):
        # reached by this encoder's own load_state_dict and by any parent's: a UttEmbeddingCache is stale from here on
        self._weights_generation = getattr(self, "_weights_generation", 0) + 1
        return super()._load_from_state_dict(*args, **kwargs)

    def forward(self, x: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Inference embedding h_T of x [B, T, input] (gradients flow through UttFusionModel only).  ``lengths`` (int
        tensor [B], optional): each row's real length — the state freezes at the row's own last step
        (``pack_padded_sequence`` semantics, ``tspm_lstm_fwd_len``); without it every row runs the padded length."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()) and x.requires_grad:
            raise L.TspmError("LSTMEncoder: train it inside UttFusionModel (the fused HIP step / its autograd node)")
        return _encode_lstm(self, x, lengths)


class TextCNN(nn.Module):
    """textcnn.py:10-69: Conv2d(in, C, (h_i, input)) x3 → ReLU → time-max → cat → Dropout → Linear + ReLU."""

    def __init__(self, input_size: int, embd_size: int = 128, in_channels: int = 1, out_channels: int = 128,
                 kernel_heights: Sequence[int] = (3, 4, 5), dropout: float = 0.5) -> None:
        super().__init__()
        if in_channels != 1 or len(kernel_heights) != 3:
            raise NotImplementedError("TextCNN HIP path: in_channels 1 and three kernel heights (textcnn.py:24-44)")
        self.conv1 = nn.Conv2d(in_channels, out_channels, (kernel_heights[0], input_size), stride=1, padding=0)
        self.conv2 = nn.Conv2d(in_channels, out_channels, (kernel_heights[1], input_size), stride=1, padding=0)
        self.conv3 = nn.Conv2d(in_channels, out_channels, (kernel_heights[2], input_size), stride=1, padding=0)
        self.dropout = nn.Dropout(dropout)
        self.embd = nn.Sequential(nn.Linear(len(kernel_heights) * out_channels, embd_size), nn.ReLU(inplace=True))
        self.hidden_size = embd_size
        self.heights = [int(k) for k in kernel_heights]
        self.out_channels = out_channels
        self.input_size = input_size
        self._engines: Dict[Any, "MosiEncoderEngine"] = {}
        self._weights_generation = 0  # as LSTMEncoder's

    def convs(self):
        return [self.conv1, self.conv2, self.conv3]

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._engines = {}
        self._weights_generation = getattr(self, "_weights_generation", 0) + 1
        return out

    def _load_from_state_dict(self, *args, **kwargs):
        self._weights_generation = getattr(self, "_weights_generation", 0) + 1
        return super()._load_from_state_dict(*args, **kwargs)

    def forward(self, x: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Inference embedding of x [B, T, input] (no dropout; gradients flow through UttFusionModel or
        MonomodalEncoder only).  ``lengths`` (int tensor [B], optional): each row's real length — the time-max runs over
        the row's own windows (``tspm_textcnn_pool_fwd_len``; rows past a length must be zero padding); without it every
        row pools over the padded length."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()) and x.requires_grad:
            raise L.TspmError("TextCNN: train it inside UttFusionModel or MonomodalEncoder (the fused HIP step / its "
                              "autograd node)")
        L.require_cuda_f32(x, "TextCNN input")
        tl = lengths is not None
        key = _text_lengths_key((x.shape[0], x.shape[1], x.device), tl)
        eng = self._engines.get(key)
        if eng is None:
            eng = self._engines[key] = MosiEncoderEngine(self, x.shape[0], x.shape[1], x.device, text_lengths=tl)
        eng.load(x)
        if tl:
            eng.set_lengths(lengths.to(x.device))
        eng.forward(L.stream_handle(), False)
        return eng.emb.clone()


class FcClassifier(nn.Module):
    """classifier.py:83-117: per layer Linear → ReLU (→ BatchNorm1d) (→ Dropout); fc_out."""

    def __init__(self, input_dim: int, layers: List[int], output_dim: int, *, dropout: float = 0.3,
                 use_bn: bool = False) -> None:
        super().__init__()
        if len(layers) == 0:
            raise NotImplementedError("FcClassifier HIP path: at least one hidden layer")
        self.all_layers = []
        for i in range(0, len(layers)):
            self.all_layers.append(nn.Linear(input_dim, layers[i]))
            self.all_layers.append(nn.ReLU())
            if use_bn:
                self.all_layers.append(nn.BatchNorm1d(layers[i]))
            if dropout > 0:
                self.all_layers.append(nn.Dropout(dropout))
            input_dim = layers[i]
        self.module = nn.Sequential(*self.all_layers)
        self.fc_out = nn.Linear(layers[-1], output_dim)
        self.widths = [int(w) for w in layers]
        self.use_bn = bool(use_bn)

    @property
    def dropout_p(self) -> float:
        """The rate the kernels use, read from the nn.Dropout modules each time (one rate per classifier,
        classifier.py:104-105; 0 when the classifier was built without dropout)."""
        ps = {float(m.p) for m in self.module if isinstance(m, nn.Dropout)}
        if len(ps) > 1:
            raise L.TspmError(f"FcClassifier HIP path: one dropout rate for every layer (found {sorted(ps)})")
        return ps.pop() if ps else 0.0

    @dropout_p.setter
    def dropout_p(self, p: float) -> None:
        drops = [m for m in self.module if isinstance(m, nn.Dropout)]
        if not drops and p > 0:
            raise L.TspmError("FcClassifier was built without dropout layers")
        for m in drops:
            m.p = float(p)

    def linears(self):
        return [m for m in self.module if isinstance(m, nn.Linear)]

    def bns(self):
        return [m for m in self.module if isinstance(m, nn.BatchNorm1d)]


# ------------------------------------------------------------------------------------------------
# kernel schedule
# ------------------------------------------------------------------------------------------------
def _conv_algo(n: int) -> L.ConvAlgo:
    """TextCNN conv tile: the LDS-staged kernel (64-row x 128-channel tiles) when the batch allows,
    else the register-direct kernel's heuristic."""
    if n % 64 == 0:
        return L.ConvAlgo(1, 2, 2, 1, 1, 1)
    return L.ConvAlgo()


TEXT_MAX_STEPS = 255  # the TextCNN kernels keep an 8-bit time index (tspm_textcnn_pool_fwd / tspm_textcnn_bwd)
_MODALITY_ORDER = ("audio", "video", "text")  # the order of a steps triple (Ta, Tv, Tt)


def _text_steps_error(tt: int) -> "L.TspmError":
    return L.TspmError(f"MOSI HIP path: 1 <= kernel heights <= min(5, steps) and steps <= {TEXT_MAX_STEPS} for the text "
                       f"modality (the TextCNN's 8-bit time index); the text length is {tt}")


def norm_steps(steps):
    """The padded length of a step: an ``int`` (every modality runs that many steps — aligned data) or a triple
    ``(Ta, Tv, Tt)`` of the audio, video and text lengths (unaligned CMU-MOSI / CMU-MOSEI: each modality at its own
    frame rate).  → the ``int`` when the three agree, else the tuple of ints; this value is what every cache is keyed by,
    so ``50`` and ``(50, 50, 50)`` name the same engine, step and graph.  Raises on a non-positive length and on a text
    length past the TextCNN's limit."""
    if isinstance(steps, (tuple, list)) or (isinstance(steps, np.ndarray) and steps.ndim == 1):
        if len(steps) != 3:
            raise L.TspmError(f"steps: an int or a triple (Ta, Tv, Tt), got {tuple(steps)!r}")
        tr = tuple(int(t) for t in steps)
    else:
        tr = (int(steps),) * 3
    if min(tr) < 1:
        raise L.TspmError(f"steps: every length must be >= 1, got {tr} (audio, video, text)")
    if tr[2] > TEXT_MAX_STEPS:
        raise _text_steps_error(tr[2])
    return tr[0] if tr[0] == tr[1] == tr[2] else tr


def steps_triple(steps):
    """(Ta, Tv, Tt) of an ``int`` or triple (normalised first)."""
    n = norm_steps(steps)
    return (n, n, n) if isinstance(n, int) else n


def _lstm_alloc(enc: "LSTMEncoder", B: int, T: int, device, backward: bool = True,
                wide: bool = False) -> Dict[str, Optional[torch.Tensor]]:
    """One LSTM's saved activations for a fixed (batch, steps): xg / gates [T*B, 4H], cs [T*B, H], hs [(T+1)*B, H],
    the gate gradients dg [T*B, 4H] (``backward``) and, for the "maxpool" embedding, the time index of each unit's
    maximum [B][H]: uint8, or with ``wide`` (the launch takes tspm_lstm_fwd_t16 / _bwd_t16, ``L.lstm_wide_index``) 16 bits
    as int16 storage holding the unsigned pattern (``L.index_to_int64`` reads it)."""
    if not L.lstm_width_supported(enc.hidden_size):
        raise L.TspmError(f"MOSI HIP path: LSTM hidden size {enc.hidden_size} — the recurrence kernels take a multiple "
                          f"of 4 with 4 <= hidden_size <= 128 (tspm_lstm_fwd_w)")
    indexed = enc.embd_method == "maxpool"
    if not L.lstm_steps_supported(T, indexed) or (indexed and T > L.LSTM_STEPS_U8 and not wide):
        raise L.TspmError(f"MOSI HIP path: {T} LSTM steps with the {enc.embd_method!r} embedding — the time index covers "
                          f"1..{L.LSTM_STEPS_U16} steps (16-bit past {L.LSTM_STEPS_U8})")
    _check_rows(T, B)
    f, H = dict(device=device, dtype=torch.float32), enc.hidden_size
    bufs = dict(xg=torch.empty(T * B, 4 * H, **f), gates=torch.empty(T * B, 4 * H, **f),
                cs=torch.empty(T * B, H, **f), hs=torch.empty((T + 1) * B, H, **f),
                dg=torch.empty(T * B, 4 * H, **f) if backward else None)
    bufs["arg"] = (torch.zeros(B, H, dtype=torch.int16 if wide else torch.uint8, device=device) if indexed else None)
    if _is_attention(enc):
        # the attention pooling: alpha [T, B], the recurrence's own h_out (a scratch: the embedding is the pooling's),
        # with "time" p / z [T*B, H]; to train it, dp and dseq [T*B, H], the per-row du / dc sums and the split-K workspace
        # of dW = dp^T r (a frozen encoder keeps none of these)
        time = enc.attention_norm == "time"
        bufs["alpha"], bufs["hout"] = torch.empty(T, B, **f), torch.empty(B, H, **f)
        bufs["p"] = torch.empty(T * B, H, **f) if time else None
        if backward and time:
            bufs["dp"], bufs["dseq"] = torch.empty(T * B, H, **f), torch.empty(T * B, H, **f)
            bufs["rows"] = torch.empty(B, 2 * H, **f)
            bufs["attn_split"] = sp = max(1, min(32, (T * B) // 128))  # as _lstm_wgrad_plan
            wsb = int(L.lib().tspm_linear_bwd_weight_splitk_workspace(T * B, H, H, sp))
            bufs["attn_ws"] = torch.empty(max(wsb // 4, 1), **f)
    return bufs


MAX_GEMM_ROWS = (1 << 31) - 1  # the dense kernels take the T*B row count as an int32


def _check_rows(T: int, B: int) -> None:
    """The dense kernels of the LSTM half (tspm_linear_fwd over T*B rows, tspm_linear_bwd_weight_splitk reducing over
    them) and the recurrences form every address in 64 bits and their grids from cdiv(rows, 32) x cdiv(4H, 32) tiles, so
    the one limit on rows is the int32 argument itself (the unaligned shapes reach 500 * 256 = 128000): refuse beyond."""
    if T * B > MAX_GEMM_ROWS:
        raise L.TspmError(f"MOSI HIP path: {T} steps x {B} rows = {T * B} LSTM rows exceed {MAX_GEMM_ROWS}")


def _lstm_fwd_prepare(d, enc: "LSTMEncoder", x: torch.Tensor, bufs, B: int, T: int, h_out: int, ld_out: int,
                      sh: int) -> None:
    """The input projection over all T*B rows (launched) and the recurrence's descriptor `d` (filled)."""
    rnn, fin = enc.rnn, enc.input_size
    L.check(L.lib().tspm_linear_fwd(T * B, fin, 4 * enc.hidden_size, x.data_ptr(), fin, rnn.weight_ih_l0.data_ptr(),
                                    rnn.bias_ih_l0.data_ptr(), 0, None, 1.0, bufs["xg"].data_ptr(),
                                    4 * enc.hidden_size, sh), "lstm input projection")
    d.batch, d.steps, d.hidden, d.ld_out = B, T, enc.hidden_size, ld_out
    d.xg, d.w_hh, d.b_hh = bufs["xg"].data_ptr(), rnn.weight_hh_l0.data_ptr(), rnn.bias_hh_l0.data_ptr()
    d.gates, d.cs, d.hs = bufs["gates"].data_ptr(), bufs["cs"].data_ptr(), bufs["hs"].data_ptr()
    d.h_out = h_out
    d.argmax = L.ptr(bufs["arg"])


def _lstm_bwd_desc(d, enc: "LSTMEncoder", bufs, B: int, T: int, dh: int, ld_dh: int) -> None:
    rnn = enc.rnn
    d.batch, d.steps, d.hidden, d.ld_dh = B, T, enc.hidden_size, ld_dh
    d.w_hh, d.gates, d.cs = rnn.weight_hh_l0.data_ptr(), bufs["gates"].data_ptr(), bufs["cs"].data_ptr()
    d.dh, d.dgates = dh, bufs["dg"].data_ptr()
    d.argmax = L.ptr(bufs["arg"])


RAGGED_MODALITIES = ("audio", "video")  # the LSTM encoders (ragged); the TextCNN's "text" key is text_lengths' own


def _ragged_key(key: tuple, ragged: bool) -> tuple:
    """A cache key with the ragged mode in it: unchanged (the key as it always was) when ``ragged`` is off."""
    return key + ("ragged",) if ragged else key


def _text_lengths_key(key: tuple, text_lengths: bool) -> tuple:
    """A cache key with the text-length mode in it, after the ragged element if any: unchanged when it is off."""
    return key + ("text_lengths",) if text_lengths else key


ENCODER_MODULES = (("audio", "netA"), ("video", "netV"), ("text", "netT"))  # modality -> attribute, in key order


def _frozen_state(model: "UttFusionModel"):
    """(frozen, error): ``frozen`` = the modalities, in audio / video / text order, whose encoder module has no
    parameter with ``requires_grad``; ``error`` = why the model cannot be TRAINED on this path (an encoder with mixed
    flags — freezing inside a module is not built — or a ``netC`` that is not fully trainable), or None.  Forward-only
    users never see the error."""
    frozen, error = [], None
    for name, attr in ENCODER_MODULES:
        flags = [(n, p.requires_grad) for n, p in getattr(model, attr).named_parameters()]
        if not any(f for _, f in flags):
            frozen.append(name)
        elif not all(f for _, f in flags) and error is None:
            off = [n for n, f in flags if not f]
            error = (f"{attr}: mixed requires_grad flags ({attr}.{off[0]} is frozen, others are not) - an encoder is "
                     f"trained or frozen as a whole")
    off = [n for n, p in model.netC.named_parameters() if not p.requires_grad]
    if off and error is None:
        error = f"netC: every classifier parameter must be trainable (netC.{off[0]} is frozen)"
    return tuple(frozen), error


def frozen_encoders(model: "UttFusionModel") -> tuple:
    """The frozen encoders of a model to be trained, as modality names in audio / video / text order (``()``: everything
    trains).  An encoder module (``netA`` / ``netV`` / ``netT``) is frozen when none of its parameters has
    ``requires_grad``.  Raises ``TspmError`` naming the module for an encoder with mixed flags or a ``netC`` that is not
    fully trainable."""
    frozen, error = _frozen_state(model)
    if error is not None:
        raise L.TspmError(f"UttFusionModel HIP path: {error}")
    return frozen


def _frozen_key(key: tuple, frozen: tuple) -> tuple:
    """A cache key with the frozen set in it, after the ragged / text_lengths elements: unchanged when nothing is
    frozen."""
    return key + (("frozen", tuple(frozen)),) if frozen else key


def check_param_groups(model: "UttFusionModel", param_groups, allreduce=None, flat_groups=None) -> tuple:
    """What FusedMosiStep asks of (model, optimizer.param_groups, optimizer.flat_groups()) before it builds anything; →
    the frozen set.  Refused with a ``TspmError`` that names the module or parameter: an encoder with mixed flags, a
    ``netC`` not fully trainable (``frozen_encoders``), a trainable parameter in no group (it would get a gradient and
    never an update), a parameter in two groups, more than ``L.ADAM_MAX_SEGMENTS`` groups with trainable parameters, and
    ``allreduce`` with more than one such group (data parallelism with several groups is not built).  ``flat_groups``
    (``FusedAdam.flat_groups()``; None: the groups' parameters by their current flags) is what the kernels update and
    what the clip norm spans: FusedAdam moved the parameters that were trainable WHEN IT WAS BUILT into its flat buffers,
    so those must be exactly the model's trainable parameters now — a parameter frozen since would still be updated
    (weight decay, stale gradients in the norm), one unfrozen since has no gradient buffer; both are refused."""
    frozen = frozen_encoders(model)
    seen: Dict[int, int] = {}
    names = {id(p): n for n, p in model.named_parameters()}
    if flat_groups is None:
        updated = [[p for p in group["params"] if p.requires_grad] for group in param_groups]
        updated = [ps for ps in updated if ps]
    else:
        updated = [list(fg.params) for fg in flat_groups]
    live = len(updated)
    for gi, group in enumerate(param_groups):
        for p in group["params"]:
            if id(p) in seen:
                raise L.TspmError(f"FusedMosiStep: parameter {names.get(id(p), '?')} is in parameter groups {seen[id(p)]} "
                                  f"and {gi}")
            seen[id(p)] = gi
    for n, p in model.named_parameters():
        if p.requires_grad and id(p) not in seen:
            raise L.TspmError(f"FusedMosiStep: trainable parameter {n} is in no FusedAdam parameter group (freeze its "
                              f"module with requires_grad_(False) or give it to the optimizer)")
    flat = {id(p) for ps in updated for p in ps}
    for ps in updated:
        for p in ps:
            if not p.requires_grad or id(p) not in names:
                raise L.TspmError(f"FusedMosiStep: parameter {names.get(id(p), '(not of this model)')} is in FusedAdam's "
                                  f"flat buffers but is not a trainable parameter of the model - frozen after the "
                                  f"optimizer was built? It would still be updated: rebuild FusedAdam")
    for n, p in model.named_parameters():
        if p.requires_grad and id(p) not in flat:
            raise L.TspmError(f"FusedMosiStep: trainable parameter {n} is not in FusedAdam's flat buffers - unfrozen "
                              f"after the optimizer was built? It has no gradient buffer: rebuild FusedAdam")
    if not 1 <= live <= L.ADAM_MAX_SEGMENTS:
        raise L.TspmError(f"FusedMosiStep: 1..{L.ADAM_MAX_SEGMENTS} FusedAdam parameter groups with trainable parameters "
                          f"(one optimizer phase for all of them), got {live}")
    if allreduce is not None and live > 1:
        raise L.TspmError("FusedMosiStep: allreduce (data parallelism) with more than one parameter group is not built")
    return frozen


def finetune_param_groups(model: "UttFusionModel", *, lr: float, weight_decay: float, encoder_lr: Optional[float] = None,
                          encoder_weight_decay: Optional[float] = None, freeze: Sequence[str] = ()) -> List[Dict[str, Any]]:
    """The second-stage experiments on pre-trained encoders as ``FusedAdam`` param groups.  ``freeze``: a subset of
    ("audio", "video", "text") - those encoders get ``requires_grad_(False)`` (the step then skips their backward and
    they are in no group).  → ``[classifier group]`` with the remaining encoders folded in when ``encoder_lr`` and
    ``encoder_weight_decay`` are both None, else ``[classifier group, encoder group]`` with the encoders at
    ``encoder_lr`` / ``encoder_weight_decay`` (each defaulting to the classifier's value) - the reference's
    ``training.encoder_optimizer`` form.  With every encoder frozen there is no encoder group."""
    mods = dict(ENCODER_MODULES)
    bad = [f for f in freeze if f not in mods]
    if bad or len(set(freeze)) != len(tuple(freeze)):
        raise L.TspmError(f"finetune_param_groups: freeze is a subset of {tuple(mods)}, got {tuple(freeze)!r}")
    enc: List[torch.Tensor] = []
    for name, attr in ENCODER_MODULES:
        if name in freeze:
            getattr(model, attr).requires_grad_(False)
        else:
            enc += list(getattr(model, attr).parameters())
    head = dict(params=list(model.netC.parameters()), lr=float(lr), weight_decay=float(weight_decay))
    if encoder_lr is None and encoder_weight_decay is None:
        head["params"] = enc + head["params"]  # model.parameters() order: encoders, then netC
        return [head]
    if not enc:
        return [head]
    return [head, dict(params=enc, lr=float(lr if encoder_lr is None else encoder_lr),
                       weight_decay=float(weight_decay if encoder_weight_decay is None else encoder_weight_decay))]


def _split_lengths(lengths) -> tuple:
    """(ragged, text_lengths) of a ``lengths`` argument: a ``"text"`` key asks for the TextCNN's length input; anything
    else — an empty dict too, as before — for the ragged LSTM recurrences.  ``{"text": ...}`` alone is text-only."""
    if lengths is None:
        return False, False
    tl = isinstance(lengths, dict) and "text" in lengths
    return (not tl) or len(lengths) > 1, tl


def _length_buffer(B: int, T: int, device) -> torch.Tensor:
    """A persistent int32 [B] length buffer of one encoder, at the padded length until a batch's lengths are copied
    in (the captured graph reads it; the kernels clamp every value to 1..T)."""
    return torch.full((B,), int(T), dtype=torch.int32, device=device)


def _set_lengths(buf: torch.Tensor, lengths: Optional[torch.Tensor], T: int, nm: str) -> None:
    """The batch's lengths into an encoder's length buffer: a device-to-device copy on the current stream, no host
    synchronisation (``None``: the encoder runs at the full padded length)."""
    if lengths is None:
        buf.fill_(int(T))
        return
    if not torch.is_tensor(lengths) or lengths.is_floating_point() or lengths.numel() != buf.numel():
        raise L.TspmError(f"lengths[{nm!r}]: an integer tensor of {buf.numel()} elements (one per batch row)")
    if lengths.data_ptr() == buf.data_ptr():
        return  # gathered straight into the buffer (mosi_data.DeviceMosiCorpus.gather(lengths_out=...))
    buf.copy_(lengths.reshape(-1), non_blocking=True)


def _check_lengths_arg(lengths, ragged: bool = True, text_lengths: bool = False) -> None:
    allowed = (RAGGED_MODALITIES if ragged else ()) + (("text",) if text_lengths else ())
    if not isinstance(lengths, dict) or any(k not in allowed for k in lengths):
        raise L.TspmError(f"lengths: a dict with keys among {allowed} (int tensors [B]) for this engine; \"audio\" / "
                          f"\"video\" need ragged=True, and the text modality has a length input only with "
                          f"text_lengths=True")


def _len_desc(d, lengths: torch.Tensor, wide: bool) -> None:
    """The two extra fields of a tspm_lstm_*_len descriptor."""
    d.lengths, d.index_bits = lengths.data_ptr(), 16 if wide else 8


def _lstm_fwd_launch(probs, B: int, sh: int, wide: bool) -> None:
    """The input projections and ONE forward recurrence call: per LSTM (encoder, input, buffers, T, h_out pointer,
    ld_out, length buffer or None); with length buffers (all or none) tspm_lstm_fwd_len, else ``L.lstm_fwd`` picks."""
    ragged = probs[0][6] is not None
    descs = ((L.LstmFwdLenDesc if ragged else L.LstmFwdDesc) * len(probs))()
    for i, (enc, x, bufs, T, h_out, ld_out, lens) in enumerate(probs):
        _lstm_fwd_prepare(descs[i], enc, x, bufs, B, T, h_out, ld_out, sh)
        if ragged:
            _len_desc(descs[i], lens, wide)
    rc = L.lstm_fwd_len(len(probs), descs, sh) if ragged else L.lstm_fwd(len(probs), descs, sh, wide)
    L.check(rc, "lstm_fwd_len" if ragged else "lstm_fwd")


def _lstm_bwd_launch(probs, B: int, sh: int, wide: bool) -> None:
    """ONE backward-through-time call: per LSTM (encoder, buffers, T, dh pointer, ld_dh, length buffer or None).  With
    lengths, dgates past each row's length are written as zeros: the weight-gradient GEMMs keep all T*B rows."""
    ragged = probs[0][5] is not None
    descs = ((L.LstmBwdLenDesc if ragged else L.LstmBwdDesc) * len(probs))()
    for i, (enc, bufs, T, dh, ld_dh, lens) in enumerate(probs):
        _lstm_bwd_desc(descs[i], enc, bufs, B, T, dh, ld_dh)
        if ragged:
            _len_desc(descs[i], lens, wide)
    rc = L.lstm_bwd_len(len(probs), descs, sh) if ragged else L.lstm_bwd(len(probs), descs, sh, wide)
    L.check(rc, "lstm_bwd_len" if ragged else "lstm_bwd")


def _is_attention(enc) -> bool:
    return getattr(enc, "embd_method", None) == "attention"


def _attn_fwd_launch(probs, B: int, sh: int) -> None:
    """The attention pooling after the recurrences: per "attention" LSTM (encoder, buffers, T, embedding pointer,
    ld_out, length buffer); with "time" the score projection p = r W^T + c over the T*B rows first (tspm_linear_fwd;
    "unit" needs no scores), then ONE tspm_attn_pool_fwd for all of them."""
    if not probs:
        return
    lib = L.lib()
    descs = (L.AttnPoolFwdDesc * len(probs))()
    for i, (enc, bufs, T, out, ld_out, lens) in enumerate(probs):
        d, H = descs[i], enc.hidden_size
        r = bufs["hs"].data_ptr() + B * H * 4  # r_t = hs[t + 1]
        if enc.attention_norm == "time":
            lin = enc.attention_layer[0]
            L.check(lib.tspm_linear_fwd(T * B, H, H, r, H, lin.weight.data_ptr(), lin.bias.data_ptr(), 0, None, 1.0,
                                        bufs["p"].data_ptr(), H, sh), "attention projection")
        d.batch, d.steps, d.hidden, d.ld_out, d.norm = B, T, H, ld_out, L.ATTN_NORMS[enc.attention_norm]
        d.r, d.p, d.u = r, L.ptr(bufs["p"]), enc.attention_vector_weight.data_ptr()
        d.alpha, d.h_out, d.lengths = bufs["alpha"].data_ptr(), out, lens.data_ptr()
    L.check(lib.tspm_attn_pool_fwd(len(probs), descs, sh), "attn_pool_fwd")


def _attn_bwd_launch(probs, B: int, sh: int, g) -> None:
    """The attention pooling's backward, before the recurrences': per trainable "attention" LSTM (encoder, buffers, T,
    gradient pointer, ld_g, length buffer).  "time": ONE tspm_attn_pool_bwd (dp, du, dc), then per
    encoder dW = the split-K weight gradient of dp over the T*B rows and dseq = dp W.  "unit": no gradient reaches
    the scores - nothing is launched here and the three parameters' gradients are written as zeros (they still belong
    to their Adam group; the flat buffers hold the previous step's values)."""
    lib = L.lib()
    timed = [p for p in probs if p[0].attention_norm == "time"]
    if timed:
        descs = (L.AttnPoolBwdDesc * len(timed))()
        for i, (enc, bufs, T, dout, ld_g, lens) in enumerate(timed):
            d, H = descs[i], enc.hidden_size
            d.batch, d.steps, d.hidden, d.ld_g, d.norm = B, T, H, ld_g, 0
            d.g, d.alpha, d.z = dout, bufs["alpha"].data_ptr(), bufs["p"].data_ptr()
            d.r, d.u = bufs["hs"].data_ptr() + B * H * 4, enc.attention_vector_weight.data_ptr()
            d.dp, d.rows = bufs["dp"].data_ptr(), bufs["rows"].data_ptr()
            d.du, d.dc = g(enc.attention_vector_weight).data_ptr(), g(enc.attention_layer[0].bias).data_ptr()
            d.lengths = lens.data_ptr()
        L.check(lib.tspm_attn_pool_bwd(len(timed), descs, sh), "attn_pool_bwd")
        for enc, bufs, T, *_ in timed:
            H, lin = enc.hidden_size, enc.attention_layer[0]
            r, ws = bufs["hs"].data_ptr() + B * H * 4, bufs["attn_ws"]
            L.check(lib.tspm_linear_bwd_weight_splitk(T * B, H, H, r, H, bufs["dp"].data_ptr(), H,
                                                      g(lin.weight).data_ptr(), None,  # dc is the pooling backward's
                                                      bufs["attn_split"], ws.data_ptr(), ws.numel() * 4, sh),
                    "attention dW")
            L.check(lib.tspm_linear_bwd_data(T * B, H, H, bufs["dp"].data_ptr(), H, lin.weight.data_ptr(),
                                             bufs["dseq"].data_ptr(), H, sh), "attention dseq")
    for enc, *_ in probs:
        if enc.attention_norm == "unit":
            for p in (enc.attention_vector_weight, enc.attention_layer[0].weight, enc.attention_layer[0].bias):
                g(p).zero_()  # on the current stream, which is the one `sh` names (captured with the step)


def _lstm_bwd_seq_launch(probs, B: int, sh: int) -> None:
    """ONE tspm_lstm_bwd_seq call for the trainable "attention" LSTMs: per LSTM (encoder, buffers, T, dh pointer, ld_dh,
    length buffer).  Every step takes alpha_t g through ``wt`` = alpha and, with "time", dseq on top."""
    descs = (L.LstmBwdSeqDesc * len(probs))()
    for i, (enc, bufs, T, dh, ld_dh, lens) in enumerate(probs):
        d, rnn = descs[i], enc.rnn
        d.batch, d.steps, d.hidden, d.ld_dh = B, T, enc.hidden_size, ld_dh
        d.w_hh, d.gates, d.cs = rnn.weight_hh_l0.data_ptr(), bufs["gates"].data_ptr(), bufs["cs"].data_ptr()
        d.dh, d.dgates, d.wt = dh, bufs["dg"].data_ptr(), bufs["alpha"].data_ptr()
        d.dseq = L.ptr(bufs.get("dseq"))
        d.lengths = lens.data_ptr()
    L.check(L.lib().tspm_lstm_bwd_seq(len(probs), descs, sh), "lstm_bwd_seq")


def _lstm_backward(encs, B: int, sh: int, wide: bool, g) -> None:
    """The backward of the trainable LSTMs of one launch group: per LSTM (encoder, buffers, T, gradient pointer, ld_g,
    length buffer or None).  "attention" encoders: the pooling's backward, then ONE
    tspm_lstm_bwd_seq; the others ONE tspm_lstm_bwd* call as before."""
    attn = [e for e in encs if _is_attention(e[0])]
    rest = [e for e in encs if not _is_attention(e[0])]
    if attn:
        _attn_bwd_launch(attn, B, sh, g)
        _lstm_bwd_seq_launch(attn, B, sh)
    if rest:
        _lstm_bwd_launch(rest, B, sh, wide)


def _lstm_wgrad(enc: "LSTMEncoder", x: torch.Tensor, bufs, B: int, T: int, split: int,
                wg_ws: torch.Tensor, g, sh: int) -> None:
    """The LSTM weight gradients as GEMMs over the T*B rows of dgates (after tspm_lstm_bwd)."""
    lib, rnn, H, fin = L.lib(), enc.rnn, enc.hidden_size, enc.input_size
    ws, wsb = wg_ws.data_ptr(), wg_ws.numel() * 4
    # dW_hh = dgates^T h_{t-1} (rows (t, b) of hs[0:T]); db_hh = column sums of dgates
    L.check(lib.tspm_linear_bwd_weight_splitk(T * B, H, 4 * H, bufs["hs"].data_ptr(), H, bufs["dg"].data_ptr(),
                                              4 * H, g(rnn.weight_hh_l0).data_ptr(),
                                              g(rnn.bias_hh_l0).data_ptr(), split, ws, wsb, sh),
            "lstm dW_hh")
    # dW_ih = dgates^T x; db_ih = the same column sums (same split and order: bitwise db_hh)
    L.check(lib.tspm_linear_bwd_weight_splitk(T * B, fin, 4 * H, x.data_ptr(), fin, bufs["dg"].data_ptr(),
                                              4 * H, g(rnn.weight_ih_l0).data_ptr(),
                                              g(rnn.bias_ih_l0).data_ptr(), split, ws, wsb, sh),
            "lstm dW_ih")


def _lstm_wgrad_plan(B: int, plans, device):
    """LSTM weight gradients reduce over T*B rows into 4H x {in, H} outputs (a few output tiles): split the
    reduction so the launch fills the chip (tspm_linear_bwd_weight_splitk) — one split for both products of an
    encoder (db_ih and db_hh come from two calls and must stay bitwise equal), chosen from that encoder's own T*B.
    ``plans``: (encoder, steps) pairs.  → (the splits in that order, one workspace that holds the largest product)."""
    lib = L.lib()
    sps = [max(1, min(32, (T * B) // 128)) for _, T in plans]
    wsb = max(int(lib.tspm_linear_bwd_weight_splitk_workspace(T * B, fin, 4 * enc.hidden_size, sp))
              for (enc, T), sp in zip(plans, sps) for fin in (enc.input_size, enc.hidden_size))
    return sps, torch.empty(max(wsb // 4, 1), device=device, dtype=torch.float32)


def _text_alloc(o, t: "TextCNN", B: int, T: int, device) -> None:
    """The TextCNN half's plan for a fixed (batch, steps), set as attributes of its owner `o` (MosiEngine or
    MosiEncoderEngine): conv shapes / tiles / outputs / workspace, pooled values and their argmax, the embedding
    Linear's input and the backward's work buffers.  ``o.text_lens`` (set by the owner before this call): the int32 [B]
    text length buffer of a ``text_lengths`` owner, else None."""
    if T > TEXT_MAX_STEPS or min(t.heights) > T or max(t.heights) > 5:
        raise _text_steps_error(T)
    f = dict(device=device, dtype=torch.float32)
    o.ft, o.Tt = t.input_size, T
    C, nc = t.out_channels, 3 * t.out_channels
    o.C, o.nc = C, nc
    o.conv_shapes = [L.ConvShape(B, T, 1, o.ft, C, k, 1, 1, 0, T - k + 1, 1) for k in t.heights]
    o.conv_algo = _conv_algo(B)
    from .engine import tuned_table
    tab = tuned_table()
    o.conv_algos = []
    for s in o.conv_shapes:
        e = tab.get(("fwd", s.n, s.h, s.w, s.c, s.k, s.r, s.s, s.stride))
        o.conv_algos.append(L.ConvAlgo(*e) if e is not None else o.conv_algo)
    o.conv_out = [torch.empty((T - k + 1) * B, C, **f) for k in t.heights]
    lib = L.lib()
    ws = max(lib.tspm_conv_fwd_workspace(ctypes.byref(s), ctypes.byref(al))
             for s, al in zip(o.conv_shapes, o.conv_algos))
    o.conv_ws = torch.zeros(max(int(ws), 256), dtype=torch.uint8, device=device)
    o.pooled = torch.empty(B, nc, **f)
    o.argmax = torch.empty(B, nc, dtype=torch.uint8, device=device)
    o.fc_in = torch.empty(B, nc, **f)
    o.dfc_in = torch.empty(B, nc, **f)
    o.g_work = torch.empty(B, nc, **f)


def _text_forward(o, t: "TextCNN", sh: int, keep: Optional[int], out: int, ld_out: int) -> None:
    """TextCNN forward on owner `o`'s plan: three convolutions (implicit GEMM), pooling + dropout (keep: the
    uint8 mask's pointer or None; with the owner's ``text_lens`` buffer over each row's own windows), embedding Linear +
    ReLU written to `out` (row stride ld_out)."""
    lib, B, T = L.lib(), o.B, o.Tt
    for conv, s, al, y in zip(t.convs(), o.conv_shapes, o.conv_algos, o.conv_out):
        L.check(lib.tspm_conv_fwd(ctypes.byref(s), ctypes.byref(al), o.X.data_ptr(), None,
                                  conv.weight.data_ptr(), y.data_ptr(), None, o.conv_ws.data_ptr(),
                                  o.conv_ws.numel(), sh), "textcnn conv")
    heights = (ctypes.c_int32 * 3)(*t.heights)
    outs = (ctypes.c_void_p * 3)(*[y.data_ptr() for y in o.conv_out])
    biases = (ctypes.c_void_p * 3)(*[cv.bias.data_ptr() for cv in t.convs()])
    tp = t.dropout.p
    scale = 1.0 / (1.0 - tp) if tp < 1 else 0.0
    if o.text_lens is not None:  # text_lengths: each row pools over its own windows
        L.check(lib.tspm_textcnn_pool_fwd_len(B, T, 3, heights, o.C, outs, biases, keep, scale, o.pooled.data_ptr(),
                                              o.argmax.data_ptr(), o.fc_in.data_ptr(), o.nc, o.text_lens.data_ptr(), sh),
                "textcnn pool (lengths)")
    else:
        L.check(lib.tspm_textcnn_pool_fwd(B, T, 3, heights, o.C, outs, biases, keep, scale, o.pooled.data_ptr(),
                                          o.argmax.data_ptr(), o.fc_in.data_ptr(), o.nc, sh), "textcnn pool")
    _text_embed(o, t, sh, out, ld_out)


def _text_embed(o, t: "TextCNN", sh: int, out: int, ld_out: int) -> None:
    """The TextCNN's tail on owner `o`: the embedding Linear + ReLU over ``o.fc_in`` [B, nc] (the pooled, dropped-out
    features) written to `out` (row stride ld_out).  ``_text_forward`` ends with it; the cached head stage
    (``MosiCachedEngine``) starts with it, on an ``fc_in`` that ``tspm_utt_cache_rows`` wrote."""
    emb = t.embd[0]
    L.check(L.lib().tspm_linear_fwd(o.B, o.nc, emb.out_features, o.fc_in.data_ptr(), o.nc, emb.weight.data_ptr(),
                                    emb.bias.data_ptr(), 1, None, 1.0, out, ld_out, sh),
            "textcnn embd")


def _text_backward(o, t: "TextCNN", sh: int, keep: Optional[int], dout: int, ld_d: int, out: int, ld_out: int,
                   g) -> None:
    """TextCNN backward from `dout` (the embedding's gradient, masked in place through the ReLU of `out`):
    embedding Linear, then pooling / dropout and the sparse conv weight gradients."""
    lib, B, T = L.lib(), o.B, o.Tt
    emb = t.embd[0]
    L.check(lib.tspm_act_bwd(B, emb.out_features, dout, ld_d, out, ld_out, 1.0, sh), "textcnn embd relu")
    linear_bwd(B, o.nc, emb.out_features, o.fc_in.data_ptr(), o.nc, dout, ld_d, emb.weight.data_ptr(),
               g(emb.weight).data_ptr(), g(emb.bias).data_ptr(), o.dfc_in.data_ptr(), o.nc, sh)
    heights = (ctypes.c_int32 * 3)(*t.heights)
    dws = (ctypes.c_void_p * 3)(*[g(cv.weight).data_ptr() for cv in t.convs()])
    dbs = (ctypes.c_void_p * 3)(*[g(cv.bias).data_ptr() for cv in t.convs()])
    tp = t.dropout.p
    L.check(lib.tspm_textcnn_bwd(B, T, o.ft, 3, heights, o.C, o.X.data_ptr(), o.dfc_in.data_ptr(),
                                 o.nc, keep, 1.0 / (1.0 - tp) if 0 < tp < 1 else 1.0, o.pooled.data_ptr(),
                                 o.argmax.data_ptr(), dws, dbs, o.g_work.data_ptr(), sh), "textcnn bwd")


def _seq_load(src: torch.Tensor, dst: torch.Tensor, B: int, T: int, index, offs, lens, nm: str, sh: int) -> None:
    """A batch-first [B, T, F] tensor → the time-major buffer `dst` (one tspm_seq_gather: the dense batch seen
    as B sequences of length T).  `dst` may hold more than B rows per step (``MosiPatternEngine``'s 2B): the batch
    goes to the first B, the others are not written."""
    L.require_cuda_f32(src, nm)
    if tuple(src.shape) != (B, T, dst.shape[2]):
        raise L.TspmError(f"{nm} batch shape {tuple(src.shape)} != planned {(B, T, dst.shape[2])} (batch, {nm} "
                          f"steps, features)")
    src = src.contiguous()
    L.check(L.lib().tspm_seq_gather(B, index.data_ptr(), B, src.data_ptr(), offs.data_ptr(), lens.data_ptr(),
                                    dst.shape[2], T, dst.data_ptr(), dst.shape[1] * dst.shape[2], dst.shape[2], None,
                                    None, None, sh), "seq_gather")


class MosiEngine:
    """Execution plan of UttFusionModel for a fixed (batch, steps): pre-allocated time-major buffers, one
    fixed sequence of libtspm launches on the caller's stream (graph-capturable).  ``steps`` is an ``int`` or a triple
    (Ta, Tv, Tt) (``norm_steps``): each modality's input, saved activations, gather helpers and weight-gradient split
    are planned at its own length (``Ts``); ``T`` is the normalised value (the ``int`` on aligned data)."""

    def __init__(self, model: "UttFusionModel", batch: int, steps, device: torch.device, ragged: bool = False,
                 text_lengths: bool = False, *, encoders: bool = True, classifier: bool = True, backward: bool = True):
        """``encoders`` / ``classifier`` / ``backward`` (all on: the train step's engine, as always): a forward-only
        half — ``classifier=False, backward=False`` plans the three encoders up to ``fused`` and nothing after it,
        ``encoders=False, backward=False`` the classifier from ``fused`` on with no LSTM or TextCNN buffer
        (``MosiPatternEngine`` runs one of each, at different row counts).  A half with ``backward`` plans only its own
        masks and gradient buffers: the encoder half ``dfused``, the TextCNN keep mask, the LSTM ``dg`` buffers and
        weight-gradient plan; the classifier half ``dlogits`` / ``dh`` / ``dr`` / ``dfused``, its layers' keep masks and
        the clip buffers."""
        self.m, self.B, self.T, self.device = model, batch, norm_steps(steps), device
        self.ragged, self.text_lengths = bool(ragged), bool(text_lengths)
        # the frozen encoders (no parameter with requires_grad): their backward is skipped.  What cannot be trained (mixed
        # flags, a frozen netC) is looked up by ``backward``, from the flags of that moment - the forward runs whatever
        # the flags are
        self.frozen = _frozen_state(model)[0]
        self.trains = {k: backward and nm not in self.frozen for k, nm in (("a", "audio"), ("v", "video"), ("t", "text"))}
        a, v, t, c = model.netA, model.netV, model.netT, model.netC
        f = dict(device=device, dtype=torch.float32)
        self.Ts = steps_triple(self.T)
        self.E = a.hidden_size + v.hidden_size + t.hidden_size
        if c.linears()[0].in_features != self.E:
            raise L.TspmError("FcClassifier input_dim must equal the sum of the three embedding sizes")
        self.fused = torch.zeros(batch, self.E, **f)
        self.keep_override: Optional[Dict[str, torch.Tensor]] = None
        self.rng_ctr_ptr: Optional[int] = None
        self._host_ctr: Optional[torch.Tensor] = None
        self.concurrent = os.environ.get("TSPM_MOSI_SERIAL", "0") != "1"
        self.side: Optional[torch.cuda.Stream] = None
        self.grad_of = lambda p: p.grad  # noqa: E731  (FusedAdam's flat gradient views)
        self.has_encoders, self.has_classifier = bool(encoders), bool(classifier)
        if encoders:
            self._plan_encoders()
        if classifier:
            self._plan_classifier(backward)
        if backward:
            self._plan_backward()

    def _plan_encoders(self) -> None:
        """The encoders' half: time-major inputs, the LSTMs' saved activations, the length buffers, the TextCNN plan."""
        m, B, device = self.m, self.B, self.device
        a, v, t = m.netA, m.netV, m.netT
        f = dict(device=device, dtype=torch.float32)
        Ta, Tv, Tt = self.Ts
        self.fa, self.fv, self.ft = a.input_size, v.input_size, t.input_size
        self.A = torch.zeros(Ta, B, self.fa, **f)          # time-major inputs, each at its own length
        self.V = torch.zeros(Tv, B, self.fv, **f)
        self.X = torch.zeros(Tt, B, self.ft, **f)
        # one launch runs both recurrences: 16-bit index buffers for both when either is "maxpool" past 256 steps
        self.wide = L.lstm_wide_index(((a.embd_method, Ta), (v.embd_method, Tv)))
        self.lstm = {name: _lstm_alloc(enc, B, T_m, device, backward=self.trains[name], wide=self.wide)
                     for name, enc, T_m in (("a", a, Ta), ("v", v, Tv))}  # a frozen LSTM keeps no dg buffer
        # ragged mode: one persistent int32 [B] length buffer per LSTM encoder, read by tspm_lstm_fwd_len / _bwd_len
        # an "attention" encoder always runs the length-taking entry points (its pooling reads lengths): such an engine
        # keeps the buffers, at the padded length, without ragged too - and both recurrences go through the one call
        self.attn = {"a": _is_attention(a), "v": _is_attention(v)}
        self.lens = ({"a": _length_buffer(B, Ta, device), "v": _length_buffer(B, Tv, device)}
                     if self.ragged or any(self.attn.values()) else None)
        # text_lengths: the TextCNN's own persistent int32 [B] length buffer, read by tspm_textcnn_pool_fwd_len
        self.text_lens = _length_buffer(B, Tt, device) if self.text_lengths else None
        _text_alloc(self, t, B, Tt, device)
        self._index = torch.arange(B, dtype=torch.int64, device=device)
        # the dense batch seen as B sequences of length T_m: per modality (equal lengths share one pair)
        self._lens, self._offs = {}, {}
        for T_m in dict.fromkeys(self.Ts):
            self._lens[T_m] = torch.full((B,), T_m, dtype=torch.int32, device=device)
            self._offs[T_m] = torch.arange(B, dtype=torch.int64, device=device) * T_m

    def _plan_classifier(self, backward: bool = True) -> None:
        """The classifier's half, from ``fused`` on: labels, groups, the layers' outputs, logits, loss (``backward``: the
        gradient buffers too)."""
        B, device, c = self.B, self.device, self.m.netC
        f = dict(device=device, dtype=torch.float32)
        self.labels = torch.zeros(B, dtype=torch.int64, device=device)
        self.labels_f = torch.zeros(B, **f)               # the regression head's float32 labels
        self.groups = torch.zeros(B, dtype=torch.int32, device=device)
        self.widths = c.widths
        self.h = [torch.empty(B, w, **f) for w in self.widths]
        self.logits = torch.empty(B, c.fc_out.out_features, **f)
        # FcClassifier(use_bn): per layer the ReLU output r (the BatchNorm input), its batch statistics and the
        # gradient of r's Linear (the BN backward writes it with the ReLU mask applied)
        self.use_bn = c.use_bn
        if self.use_bn:
            self.r = [torch.empty(B, w, **f) for w in self.widths]
            self.bn_mean = [torch.empty(w, **f) for w in self.widths]
            self.bn_inv = [torch.empty(w, **f) for w in self.widths]
        self.loss = torch.zeros(1, **f)
        self.stats = torch.zeros(4, **f)
        if backward:
            self.dlogits = torch.empty_like(self.logits)
            self.dh = [torch.empty(B, w, **f) for w in self.widths]
            if self.use_bn:
                self.dr = [torch.empty(B, w, **f) for w in self.widths]
            self.dfused = torch.empty(B, self.E, **f)

    def _plan_backward(self) -> None:
        """What only a training engine keeps: the dropout keep masks, the LSTM weight-gradient plan, the clip buffers —
        of the halves this engine holds (a half alone: ``keeps[0]`` is empty without the encoders, there are no
        ``keeps[1:]`` without the classifier; ``dfused`` is the classifier half's, or the encoder half's own)."""
        m, B, device = self.m, self.B, self.device
        f = dict(device=device, dtype=torch.float32)
        # dropout keep masks: TextCNN (before the embedding Linear) + one per classifier layer
        sizes = [self.nc if self.has_encoders else 0] + (self.widths if self.has_classifier else [])
        self.keep_all = torch.ones(B * sum(sizes), dtype=torch.uint8, device=device)
        self.keeps, off = [], 0
        for w in sizes:
            self.keeps.append(self.keep_all[off:off + B * w].view(B, w))
            off += B * w
        Ta, Tv, _ = self.Ts
        plans = [(name, enc, T_m) for name, enc, T_m in (("a", m.netA, Ta), ("v", m.netV, Tv))
                 if self.trains[name] and self.has_encoders]
        self.wg_splits, self.wg_ws = {}, None  # the weight-gradient GEMMs of the trainable LSTMs
        if plans:
            sps, self.wg_ws = _lstm_wgrad_plan(B, [(enc, T_m) for _, enc, T_m in plans], device)
            self.wg_splits = {name: sp for (name, _, _), sp in zip(plans, sps)}
        if not self.has_classifier:
            self.dfused = torch.empty(B, self.E, **f)  # the encoder half's own: tspm_pattern_expand_bwd writes it
            return
        self.clip_coef = torch.ones(1, **f)
        self.total_norm = torch.zeros(1, **f)
        self.clip_ws = torch.zeros(int(L.lib().tspm_grad_clip_workspace()) // 4 + 1, **f)

    # -- inputs -------------------------------------------------------------------------------------
    def set_lengths(self, lengths: Optional[Dict[str, torch.Tensor]]) -> None:
        """Ragged mode: the batch's ``{"audio": int [B], "video": int [B]}`` into the length buffers (device-to-device,
        outside any captured graph, which reads the buffers); an absent key runs that encoder at the full length.  A
        ``text_lengths`` engine takes ``"text"`` the same way; any other engine refuses that key."""
        if not self.ragged and not self.text_lengths:
            if lengths is not None:
                raise L.TspmError("MosiEngine: lengths given to an engine built without ragged=True")
            return
        lengths = lengths or {}
        _check_lengths_arg(lengths, self.ragged, self.text_lengths)
        if self.ragged:
            for nm, key, T_m in (("audio", "a", self.Ts[0]), ("video", "v", self.Ts[1])):
                _set_lengths(self.lens[key], lengths.get(nm), T_m, nm)
        if self.text_lengths:
            _set_lengths(self.text_lens, lengths.get("text"), self.Ts[2], "text")

    def load(self, A: torch.Tensor, V: torch.Tensor, T: torch.Tensor, labels: Optional[torch.Tensor] = None,
             regress: bool = False) -> None:
        """Batch-first [B, T, F] reference tensors → the time-major buffers (tspm_seq_gather: one launch per
        modality, the dense batch seen as B sequences of length T).  ``labels`` go to the int64 ``labels`` of the
        classification head or, with ``regress`` (the caller's mode, not the tensor's dtype), to the float32
        ``labels_f`` of the regression head, cast to the buffer's type either way."""
        sh = L.stream_handle()
        for src, dst, nm, T_m in zip((A, V, T), (self.A, self.V, self.X), _MODALITY_ORDER, self.Ts):
            _seq_load(src, dst, self.B, T_m, self._index, self._offs[T_m], self._lens[T_m], nm, sh)
        if labels is not None:
            dst = self.labels_f if regress else self.labels
            if labels.data_ptr() != dst.data_ptr():
                dst.copy_(labels.reshape(-1).to(dst.dtype), non_blocking=True)

    # -- forward ------------------------------------------------------------------------------------
    def apply_keep_override(self) -> None:
        """Copy injected dropout masks (parity hook: {"text", "cls0", ...} -> uint8) into the keep buffers;
        called before the step runs, outside any captured graph."""
        if self.keep_override is None:
            return
        names = ["text"] + [f"cls{j}" for j in range(len(self.widths))]
        for k, dst in zip(names, self.keeps):
            dst.copy_(self.keep_override[k].reshape(dst.shape).to(torch.uint8), non_blocking=True)

    def _keep_masks(self, train: bool, sh: int) -> None:
        """Fresh keep masks for one training forward: the TextCNN slice (keeps[0]) at the TextCNN's own rate
        (textcnn.py:45, netT.dropout.p), the classifier slices at the classifier's (classifier.py:104-105);
        two independent draws (the classifier's under a derived seed) on the same step counter."""
        pt, pc = float(self.m.netT.dropout.p), float(self.m.netC.dropout_p)
        if not train or (pt <= 0 and pc <= 0) or self.keep_override is not None:
            return
        if self.rng_ctr_ptr is None:
            self._host_ctr = torch.zeros(1, dtype=torch.int64, device=self.device)
            self.rng_ctr_ptr = self._host_ctr.data_ptr()
        lib, seed = L.lib(), self.m._rng_seed
        nt = self.keeps[0].numel()
        if pt > 0:
            L.check(lib.tspm_dropout_mask(nt, pt, seed, self.rng_ctr_ptr, self.keep_all.data_ptr(), sh),
                    "dropout_mask (text)")
        if pc > 0:
            L.check(lib.tspm_dropout_mask(self.keep_all.numel() - nt, pc, seed ^ _CLS_SEED_SALT, self.rng_ctr_ptr,
                                          self.keep_all.data_ptr() + nt, sh), "dropout_mask (classifier)")
        if self._host_ctr is not None and self.rng_ctr_ptr == self._host_ctr.data_ptr():
            self._host_ctr.add_(1)  # outside FusedMosiStep nothing else advances the counter: fresh masks per step

    def _fork(self):
        """Side stream for the LSTM half of the step (it shares no buffer with the TextCNN half until the
        classifier): returns (side torch stream, its handle) after making it wait for the main stream."""
        if self.side is None:
            self.side = L.shared_streams(self.device, 1)[0]
            self._ev = [torch.cuda.Event() for _ in range(4)]
        main = torch.cuda.current_stream(self.device)
        self._ev[0].record(main)
        self.side.wait_event(self._ev[0])
        return self.side, self.side.cuda_stream

    def _join(self) -> None:
        self._ev[1].record(self.side)
        torch.cuda.current_stream(self.device).wait_event(self._ev[1])

    def forward(self, sh: int, train: bool, head: bool = True) -> None:
        """Dropout masks, then the LSTM half (side stream) concurrently with the TextCNN half (caller's
        stream), joined before the classifier; everything graph-capturable.  ``head=False`` stops before
        ``fc_out`` (``head_regress`` runs it)."""
        self._keep_masks(train, sh)
        self._forward_encoders(sh, train)
        self._forward_classifier(sh, train, head)

    def _forward_encoders(self, sh: int, train: bool) -> None:
        """The three encoders into ``fused``: the LSTM half on the side stream, the TextCNN half on the caller's, joined."""
        if self.concurrent:
            side, sh_side = self._fork()
            with torch.cuda.stream(side):
                self._forward_lstm(sh_side)
            self._forward_text(sh, train)
            self._join()
        else:
            self._forward_lstm(sh)
            self._forward_text(sh, train)

    def _forward_lstm(self, sh: int) -> None:
        lib, m = L.lib(), self.m
        B, (Ta, Tv, _) = self.B, self.Ts
        # LSTM input projections over each encoder's T_m*B rows, then both recurrences in one launch
        # (an "attention" encoder's recurrence writes its h_out to a scratch; the pooling that follows writes the embedding)
        encs = (("a", m.netA, self.A, 0, Ta), ("v", m.netV, self.V, m.netA.hidden_size, Tv))
        _lstm_fwd_launch([(enc, x, self.lstm[name], T_m,
                           *((self.lstm[name]["hout"].data_ptr(), enc.hidden_size) if self.attn[name]
                             else (self.fused.data_ptr() + col * 4, self.E)),
                           self.lens[name] if self.lens is not None else None)
                          for name, enc, x, col, T_m in encs], B, sh, self.wide)
        _attn_fwd_launch([(enc, self.lstm[name], T_m, self.fused.data_ptr() + col * 4, self.E, self.lens[name])
                          for name, enc, _, col, T_m in encs if self.attn[name]], B, sh)

    def _forward_text(self, sh: int, train: bool) -> None:
        m, t = self.m, self.m.netT
        keep_t = self.keeps[0].data_ptr() if (train and t.dropout.p > 0) else None
        col_t = m.netA.hidden_size + m.netV.hidden_size
        _text_forward(self, t, sh, keep_t, self.fused.data_ptr() + col_t * 4, self.E)

    def _forward_classifier(self, sh: int, train: bool, head: bool = True) -> None:
        lib, m, B = L.lib(), self.m, self.B
        # FcClassifier: (Linear, ReLU, [BatchNorm1d,] Dropout) per layer, fc_out
        c = m.netC
        cp = c.dropout_p
        x, fin = self.fused, self.E
        if self.use_bn:
            for j, (lin, bn, hbuf) in enumerate(zip(c.linears(), c.bns(), self.h)):
                w = lin.out_features
                L.check(lib.tspm_linear_fwd(B, fin, w, x.data_ptr(), fin, lin.weight.data_ptr(), lin.bias.data_ptr(),
                                            1, None, 1.0, self.r[j].data_ptr(), w, sh), f"classifier {j}")
                if train:
                    keep = self.keeps[1 + j].data_ptr() if cp > 0 else None
                    L.check(lib.tspm_bn1d_fwd_drop(B, w, self.r[j].data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(),
                                                   bn.running_mean.data_ptr(), bn.running_var.data_ptr(),
                                                   float(bn.momentum), float(bn.eps), self.bn_mean[j].data_ptr(),
                                                   self.bn_inv[j].data_ptr(), keep,
                                                   1.0 / (1.0 - cp) if 0 < cp < 1 else 1.0, hbuf.data_ptr(), sh),
                            f"classifier bn {j}")
                else:
                    L.check(lib.tspm_bn_apply_eval(B, w, self.r[j].data_ptr(), bn.running_mean.data_ptr(),
                                                   bn.running_var.data_ptr(), float(bn.eps), bn.weight.data_ptr(),
                                                   bn.bias.data_ptr(), 0, None, None, None, None, None, 0,
                                                   hbuf.data_ptr(), sh), f"classifier bn {j} (eval)")
                x, fin = hbuf, w
            if train:  # num_batches_tracked += 1 of every classifier BatchNorm1d: one launch
                from .step import shared_batches_tracked
                L.counters_add(shared_batches_tracked(m, self.device, (nn.BatchNorm1d,)), 1, sh)
        else:  # Linear + ReLU + Dropout in one launch per layer
            for j, (lin, hbuf) in enumerate(zip(c.linears(), self.h)):
                keep = self.keeps[1 + j].data_ptr() if (train and cp > 0) else None
                L.check(lib.tspm_linear_fwd(B, fin, lin.out_features, x.data_ptr(), fin, lin.weight.data_ptr(),
                                            lin.bias.data_ptr(), 1, keep, 1.0 / (1.0 - cp) if cp < 1 else 0.0,
                                            hbuf.data_ptr(), lin.out_features, sh), f"classifier {j}")
                x, fin = hbuf, lin.out_features
        if not head:
            return
        fo = c.fc_out
        L.check(lib.tspm_linear_fwd(B, fin, fo.out_features, x.data_ptr(), fin, fo.weight.data_ptr(),
                                    fo.bias.data_ptr(), 0, None, 1.0, self.logits.data_ptr(), fo.out_features, sh),
                "classifier out")

    def loss_fn(self, sh: int, weight: float, with_grad: bool, stats: bool = False, rows=None, loss=None) -> None:
        """``rows`` = (first row, count): the cross-entropy of that row slice alone (forward only), written to ``loss``
        (a one-element tensor; default: the engine's)."""
        r0, n = rows if rows is not None else (0, self.B)
        if with_grad and rows is not None:
            raise L.TspmError("MosiEngine.loss_fn: a row slice has no gradient (the mean is over the slice)")
        C = self.logits.shape[1]
        L.check(L.lib().tspm_cross_entropy(n, C, self.logits.data_ptr() + r0 * C * 4, self.labels.data_ptr() + r0 * 8,
                                           (self.loss if loss is None else loss).data_ptr(),
                                           self.dlogits.data_ptr() if with_grad else None, weight,
                                           self.stats.data_ptr() if stats else None, sh), "cross_entropy")

    def classify_update(self, sh: int, lg, rows=None, loss=None) -> None:
        """``tspm_classify_update`` of the rows (default: all) into the ClassificationLog ``lg``: confusion counts by
        group, the loss appended to the epoch's log."""
        r0, n = rows if rows is not None else (0, self.B)
        C = self.logits.shape[1]
        L.check(L.lib().tspm_classify_update(n, C, self.logits.data_ptr() + r0 * C * 4, self.labels.data_ptr() + r0 * 8,
                                             self.groups.data_ptr() + r0 * 4, len(lg.groups), lg.conf.data_ptr(), None,
                                             (self.loss if loss is None else loss).data_ptr(), lg.loss_log.data_ptr(),
                                             lg.counters.data_ptr(), lg.capacity, sh), "classify_update")

    def head_regress(self, sh: int, train: bool, kind: int, weight: float, log=None, rows=None, loss=None) -> None:
        """The regression head in ONE launch (``tspm_regress_head_step``) in place of ``fc_out``'s tspm_linear_fwd,
        tspm_cross_entropy, tspm_classify_update and ``fc_out``'s tspm_linear_bwd: predictions into ``logits``
        [B, 1], the weighted L1 / MSE loss against ``labels_f`` into ``loss``, with ``train`` the gradients of
        ``fc_out`` and ``dh[-1]`` (``backward(sh, from_head=False)`` continues from it), with ``log`` (a
        metrics.RegressionLog) the epoch's per-pattern accumulators and loss log.  ``rows`` = (first row, count): the
        head of that row slice alone (forward only), its loss written to ``loss`` (default: the engine's)."""
        fo, w = self.m.netC.fc_out, self.widths[-1]
        r0, n = rows if rows is not None else (0, self.B)
        if train and rows is not None:
            raise L.TspmError("MosiEngine.head_regress: a row slice runs forward only")
        if fo.out_features != 1 or not L.regress_head_supported(n, w):
            raise L.TspmError(f"regression head: fc_out must be Linear(hid, 1) with hid <= 128 and a multiple of 4 and "
                              f"at most 1024 rows (got Linear({w}, {fo.out_features}), {n} rows)")
        g = self.grad_of
        d = L.RegressHeadDesc(n=n, hid=w, ld_emb=w, ld_demb=w, kind=int(kind), n_groups=1,
                              loss_weight=float(weight))
        d.emb, d.w, d.b = self.h[-1].data_ptr() + r0 * w * 4, fo.weight.data_ptr(), fo.bias.data_ptr()
        d.labels, d.pred = self.labels_f.data_ptr() + r0 * 4, self.logits.data_ptr() + r0 * 4
        d.loss = (self.loss if loss is None else loss).data_ptr()
        if train:
            d.dw, d.db, d.demb = g(fo.weight).data_ptr(), g(fo.bias).data_ptr(), self.dh[-1].data_ptr()
        if log is not None:
            d.groups, d.n_groups, d.stats = self.groups.data_ptr() + r0 * 4, len(log.groups), log.records.data_ptr()
            d.loss_log, d.counters, d.log_capacity = log.loss_log.data_ptr(), log.counters.data_ptr(), log.capacity
        L.check(L.lib().tspm_regress_head_step(ctypes.byref(d), sh), "regress_head_step")

    # -- backward -----------------------------------------------------------------------------------
    def backward(self, sh: int, from_head: bool = True) -> None:
        """``from_head=False``: ``dh[-1]`` and ``fc_out``'s gradients are already written (``head_regress``).  A frozen
        encoder's backward is skipped: no tspm_lstm_bwd* problem, weight-gradient GEMMs or ``dg`` buffer for a frozen
        LSTM (no launch and no side-stream fork with both frozen), no ``_text_backward`` for a frozen ``netT``, and with
        all three frozen layer 0's ``linear_bwd`` gets no ``dx``: ``dfused`` is never written."""
        self._check_flags()
        self._backward_classifier(sh, from_head)
        self._backward_encoders(sh)

    def _check_flags(self) -> None:
        frozen, error = self.m.flag_state()[1]  # the flags now, not those of the engine's construction
        if error is not None:
            raise L.TspmError(f"UttFusionModel HIP path: {error}")
        if frozen != self.frozen:
            raise L.TspmError(f"MosiEngine: requires_grad flags changed since this engine was planned (frozen then: "
                              f"{self.frozen}, now: {frozen})")

    def _backward_classifier(self, sh: int, from_head: bool = True) -> None:
        """``fc_out`` (``from_head``) and the classifier layers, down to ``dfused`` (not written with every encoder
        frozen)."""
        lib, m, g = L.lib(), self.m, self.grad_of
        B = self.B
        c = m.netC
        cscale = 1.0 / (1.0 - c.dropout_p) if c.dropout_p > 0 else 1.0
        lins = c.linears()
        fo = c.fc_out
        if from_head:
            linear_bwd(B, self.widths[-1], fo.out_features, self.h[-1].data_ptr(), self.widths[-1],
                       self.dlogits.data_ptr(), fo.out_features, fo.weight.data_ptr(), g(fo.weight).data_ptr(),
                       g(fo.bias).data_ptr(), self.dh[-1].data_ptr(), self.widths[-1], sh)
        bns = c.bns()
        for j in range(len(lins) - 1, -1, -1):
            w = self.widths[j]
            if self.use_bn:  # Dropout → BatchNorm1d → ReLU backward in one launch: dy of the Linear in dr[j]
                keep = self.keeps[1 + j].data_ptr() if c.dropout_p > 0 else None
                L.check(lib.tspm_bn1d_bwd_drop_relu(B, w, self.dh[j].data_ptr(), keep, cscale, self.r[j].data_ptr(),
                                                    self.bn_mean[j].data_ptr(), self.bn_inv[j].data_ptr(),
                                                    bns[j].weight.data_ptr(), g(bns[j].weight).data_ptr(),
                                                    g(bns[j].bias).data_ptr(), self.dr[j].data_ptr(), sh),
                        "cls bn bwd")
                dy = self.dr[j]
            else:
                L.check(lib.tspm_act_bwd(B, w, self.dh[j].data_ptr(), w, self.h[j].data_ptr(), w, cscale, sh),
                        "cls relu")
                dy = self.dh[j]
            xin, fin = (self.h[j - 1], self.widths[j - 1]) if j > 0 else (self.fused, self.E)
            dx, lddx = (self.dh[j - 1], self.widths[j - 1]) if j > 0 else (self.dfused, self.E)
            if j == 0 and not any(self.trains.values()):
                dx = None  # every encoder frozen: nothing reads the embeddings' gradient
            linear_bwd(B, fin, w, xin.data_ptr(), fin, dy.data_ptr(), w, lins[j].weight.data_ptr(),
                       g(lins[j].weight).data_ptr(), g(lins[j].bias).data_ptr(), L.ptr(dx), lddx, sh)

    def _backward_encoders(self, sh: int) -> None:
        """The trainable encoders' backward from ``dfused``: the LSTM half on the side stream when both halves train."""
        lstm, text = self.trains["a"] or self.trains["v"], self.trains["t"]
        if not (lstm and text):  # a frozen half: the other one (if any) on the caller's stream, no fork
            if text:
                self._backward_text(sh)
            if lstm:
                self._backward_lstm(sh)
            return
        if self.concurrent:
            side, sh_side = self._fork()
            with torch.cuda.stream(side):
                self._backward_lstm(sh_side)
            self._backward_text(sh)
            self._join()
        else:
            self._backward_text(sh)
            self._backward_lstm(sh)

    def _backward_text(self, sh: int) -> None:
        m, t = self.m, self.m.netT
        col_t = m.netA.hidden_size + m.netV.hidden_size
        keep_t = self.keeps[0].data_ptr() if t.dropout.p > 0 else None
        _text_backward(self, t, sh, keep_t, self.dfused.data_ptr() + col_t * 4, self.E,
                       self.fused.data_ptr() + col_t * 4, self.E, self.grad_of)

    def _backward_lstm(self, sh: int) -> None:
        lib, m, g = L.lib(), self.m, self.grad_of
        B, (Ta, Tv, _) = self.B, self.Ts
        # LSTMs: backward through time (one launch for both), then the weight gradients as GEMMs over T_m*B rows
        encs = [e for e in (("a", m.netA, self.A, 0, Ta), ("v", m.netV, self.V, m.netA.hidden_size, Tv))
                if self.trains[e[0]]]  # a frozen LSTM is no problem of the launch
        _lstm_backward([(enc, self.lstm[name], T_m, self.dfused.data_ptr() + col * 4, self.E,
                         self.lens[name] if self.lens is not None else None)
                        for name, enc, _, col, T_m in encs], B, sh, self.wide, g)
        for name, enc, x, _, T_m in encs:
            _lstm_wgrad(enc, x, self.lstm[name], B, T_m, self.wg_splits[name], self.wg_ws, g, sh)

    def clip(self, sh: int, flat_grad, grad_scale: float) -> None:
        """clip_grad_norm_(model.parameters(), clip) coefficient into ``clip_coef`` (utt_fusion.py:188-189).
        ``flat_grad``: the optimizer's flat gradient buffer, or a list of them (one per FusedAdam group) - with more than
        one the norm spans them all in ``tspm_grad_clip_coef_multi``'s two launches.  A frozen parameter is in no flat
        buffer, as clip_grad_norm_ skips parameters without gradients."""
        if isinstance(flat_grad, (list, tuple)) and len(flat_grad) == 1:
            flat_grad = flat_grad[0]
        if isinstance(flat_grad, (list, tuple)):
            ranges = (L.GradRange * len(flat_grad))(*[L.GradRange(t.data_ptr(), t.numel()) for t in flat_grad])
            L.check(L.lib().tspm_grad_clip_coef_multi(len(flat_grad), ranges, grad_scale, float(self.m.clip),
                                                      self.clip_coef.data_ptr(), self.total_norm.data_ptr(),
                                                      self.clip_ws.data_ptr(), self.clip_ws.numel() * 4, sh),
                    "grad_clip_multi")
            return
        L.check(L.lib().tspm_grad_clip_coef(flat_grad.numel(), flat_grad.data_ptr(), grad_scale, float(self.m.clip),
                                            self.clip_coef.data_ptr(), self.total_norm.data_ptr(),
                                            self.clip_ws.data_ptr(), self.clip_ws.numel() * 4, sh), "grad_clip")


class MosiEncoderEngine:
    """Execution plan of ONE MOSI encoder (LSTMEncoder "last" / "maxpool", or TextCNN) for a fixed (batch,
    steps), forward and backward on the caller's stream (graph-capturable) — the encoder pre-training step of
    monomodal.MonomodalEncoder and TextCNN's standalone forward.  The input is time-major in ``X`` [T, B, F];
    the embedding goes to ``emb`` [B, hidden]; ``backward`` consumes its gradient ``demb`` and writes the
    parameter gradients to ``grad_of(p)``.  Same launches as the encoder's half of MosiEngine (shared code):
    LSTM = input projection + tspm_lstm_fwd(count 1) / tspm_lstm_bwd(count 1) + the two split-K weight
    gradients; TextCNN = three convs + pool/dropout + embedding Linear / act_bwd + linear_bwd + textcnn_bwd."""

    def __init__(self, enc: nn.Module, batch: int, steps: int, device, seed: int = 0,
                 x: Optional[torch.Tensor] = None, emb: Optional[torch.Tensor] = None, ragged: bool = False,
                 text_lengths: bool = False):
        if torch.device(device).type != "cuda":
            raise L.TspmError("MOSI encoders (tspm_amd) run on the MI355X only (no CPU fallback)")
        self.enc, self.B, self.T, self.device = enc, int(batch), int(steps), device
        self.ragged, self.text_lengths = bool(ragged), bool(text_lengths)
        if self.ragged and isinstance(enc, TextCNN):
            raise L.TspmError("MosiEncoderEngine: ragged mode is the LSTM encoders' (the TextCNN's length input is "
                              "text_lengths=True)")
        if self.text_lengths and not isinstance(enc, TextCNN):
            raise L.TspmError("MosiEncoderEngine: text_lengths is the TextCNN's length input (an LSTMEncoder takes "
                              "ragged=True)")
        # (an "attention" LSTMEncoder keeps the buffer, at the padded length, without ragged too: its entry points read it)
        self.lens = _length_buffer(self.B, self.T, device) if self.ragged or _is_attention(enc) else None
        # text_lengths: the TextCNN's persistent int32 [B] length buffer, read by tspm_textcnn_pool_fwd_len
        self.text_lens = _length_buffer(self.B, self.T, device) if self.text_lengths else None
        B, T = self.B, self.T
        f = dict(device=device, dtype=torch.float32)
        self.is_text = isinstance(enc, TextCNN)
        if not self.is_text and not isinstance(enc, LSTMEncoder):
            raise L.TspmError(f"MosiEncoderEngine: LSTMEncoder or TextCNN, not {type(enc).__name__}")
        self.hidden = int(enc.hidden_size)
        shape = (T, B, int(enc.input_size))
        if x is not None and (tuple(x.shape) != shape or not x.is_contiguous()):
            raise L.TspmError(f"input buffer {tuple(x.shape)} != time-major {shape}")
        self.X = x if x is not None else torch.zeros(shape, **f)
        self.emb = emb if emb is not None else torch.zeros(B, self.hidden, **f)
        self.demb = torch.empty(B, self.hidden, **f)
        self.keep_override: Optional[Dict[str, torch.Tensor]] = None
        self.rng_ctr_ptr: Optional[int] = None
        self._host_ctr: Optional[torch.Tensor] = None
        self.seed = int(seed)
        self.wide = False
        if self.is_text:
            _text_alloc(self, enc, B, T, device)
            self.keep = torch.ones(B, self.nc, dtype=torch.uint8, device=device)
        else:
            self.wide = L.lstm_wide_index(((enc.embd_method, T),))  # "maxpool" past 256 steps: the 16-bit index
            self.bufs = _lstm_alloc(enc, B, T, device, wide=self.wide)
            (self.wg_split,), self.wg_ws = _lstm_wgrad_plan(B, ((enc, T),), device)
        self.grad_of = lambda p: p.grad  # noqa: E731  (FusedAdam's flat gradient views)
        self._index = torch.arange(B, dtype=torch.int64, device=device)
        self._lens = torch.full((B,), T, dtype=torch.int32, device=device)
        self._offs = torch.arange(B, dtype=torch.int64, device=device) * T

    def set_lengths(self, lengths: Optional[torch.Tensor]) -> None:
        """Ragged / text_lengths mode: the batch's int lengths [B] into the length buffer (``None``: the full padded
        length)."""
        if not self.ragged and not self.text_lengths:
            if lengths is not None:
                raise L.TspmError("MosiEncoderEngine: lengths given to an engine built without ragged=True (an "
                                  "LSTMEncoder) or text_lengths=True (a TextCNN)")
            return
        _set_lengths(self.lens if self.ragged else self.text_lens, lengths, self.T, "input")

    def load(self, x: torch.Tensor) -> None:
        """A batch-first [B, T, F] tensor → the time-major input buffer."""
        _seq_load(x, self.X, self.B, self.T, self._index, self._offs, self._lens, "input", L.stream_handle())

    def apply_keep_override(self) -> None:
        """Copy the injected TextCNN dropout mask (parity hook: {"text": uint8 [B, 3C]}) into the keep buffer;
        called before the step runs, outside any captured graph."""
        if self.keep_override is not None and self.is_text:
            self.keep.copy_(self.keep_override["text"].reshape(self.keep.shape).to(torch.uint8), non_blocking=True)

    def _keep_mask(self, train: bool, sh: int) -> Optional[int]:
        """The TextCNN keep mask of this forward: None in eval / without dropout, the injected mask, or a fresh
        draw of tspm_dropout_mask on the step counter (the optimizer's, or a host-advanced one)."""
        p = float(self.enc.dropout.p) if self.is_text else 0.0
        if not train or p <= 0:
            return None
        if self.keep_override is None:
            if self.rng_ctr_ptr is None:
                self._host_ctr = torch.zeros(1, dtype=torch.int64, device=self.device)
                self.rng_ctr_ptr = self._host_ctr.data_ptr()
            L.check(L.lib().tspm_dropout_mask(self.keep.numel(), p, self.seed, self.rng_ctr_ptr, self.keep.data_ptr(),
                                              sh), "dropout_mask (text)")
            if self._host_ctr is not None and self.rng_ctr_ptr == self._host_ctr.data_ptr():
                self._host_ctr.add_(1)  # nothing else advances a host-owned counter: fresh masks per forward
        return self.keep.data_ptr()

    def forward(self, sh: int, train: bool) -> None:
        B, T = self.B, self.T
        if self.is_text:
            _text_forward(self, self.enc, sh, self._keep_mask(train, sh), self.emb.data_ptr(), self.hidden)
            return
        if _is_attention(self.enc):  # the recurrence's h_out to a scratch, the embedding from the pooling
            _lstm_fwd_launch([(self.enc, self.X, self.bufs, T, self.bufs["hout"].data_ptr(), self.hidden, self.lens)], B,
                             sh, self.wide)
            _attn_fwd_launch([(self.enc, self.bufs, T, self.emb.data_ptr(), self.hidden, self.lens)], B, sh)
            return
        _lstm_fwd_launch([(self.enc, self.X, self.bufs, T, self.emb.data_ptr(), self.hidden, self.lens)], B, sh,
                         self.wide)

    def backward(self, sh: int) -> None:
        """From ``demb`` (modified in place by the TextCNN's ReLU mask) to every parameter gradient."""
        B, T = self.B, self.T
        if self.is_text:
            keep = self.keep.data_ptr() if self.enc.dropout.p > 0 else None
            _text_backward(self, self.enc, sh, keep, self.demb.data_ptr(), self.hidden, self.emb.data_ptr(),
                           self.hidden, self.grad_of)
            return
        _lstm_backward([(self.enc, self.bufs, T, self.demb.data_ptr(), self.hidden, self.lens)], B, sh, self.wide,
                       self.grad_of)
        _lstm_wgrad(self.enc, self.X, self.bufs, B, T, self.wg_split, self.wg_ws, self.grad_of, sh)


def _ce_weight(loss_functions) -> Optional[float]:
    from .step import _ce_weight as ce
    return ce(loss_functions)


def _regress_term(loss_functions):
    """(kind, weight) of the single L1 / MSE term of a LossFunctionGroup — kind ``L.REGRESS_L1`` for ``nn.L1Loss``,
    ``L.REGRESS_MSE`` for ``nn.MSELoss``, both with ``reduction="mean"`` — or None when the group is anything else
    (no group, several terms, another loss or reduction)."""
    try:
        items = list(loss_functions.items())
    except AttributeError:
        return None
    if len(items) != 1:
        return None
    term = items[0][1]
    fn = getattr(term, "loss_fn", None)
    kind = L.REGRESS_L1 if isinstance(fn, nn.L1Loss) else L.REGRESS_MSE if isinstance(fn, nn.MSELoss) else None
    if kind is None or fn.reduction != "mean":
        return None
    return kind, float(getattr(term, "weight", 1.0))


def _regress_mode(model: "UttFusionModel", loss_functions):
    """``_regress_term`` when the model is the regression model (``netC.fc_out`` has one output), else None."""
    return _regress_term(loss_functions) if model.netC.fc_out.out_features == 1 else None


def _loss_mode(who: str, model: "UttFusionModel", loss_functions, head_rows: int):
    """``(weight, regress)`` of the fused step ``who`` whose head runs over ``head_rows`` rows: the weight of a single
    cross-entropy term (else None) and ``_regress_mode``'s (kind, weight) of the one-launch regression head (else None).
    A loss group that is neither, and a regression head outside ``tspm_regress_head_step``'s limits, are refused."""
    weight, regress = _ce_weight(loss_functions), _regress_mode(model, loss_functions)
    if regress is None and weight is None:
        raise L.TspmError(f"{who}: the loss group must be a single cross-entropy term (or, with a one-output fc_out, "
                          f"a single mean L1 / MSE term)")
    if regress is not None and not L.regress_head_supported(head_rows, model.netC.widths[-1]):
        raise L.TspmError(f"{who}: the regression head takes at most 1024 rows and a last classifier layer of at most "
                          f"128 units, a multiple of 4")
    return weight, regress


def _check_regress_log(log) -> None:
    from .metrics import RegressionLog
    if log is not None and not isinstance(log, RegressionLog):
        raise L.TspmError("the regression head records into a metrics.RegressionLog")


class FusedMosiStep(L.GraphRunner):
    """One UTT-Fusion train step — forward, cross-entropy, backward, gradient clip, Adam — as one HIP
    graph (``_lib.GraphRunner``, key: the log; the backward overwrites every gradient, no zero_grad pass).  With a
    one-output ``netC.fc_out`` and a single mean L1 / MSE term (sentiment regression on float32 labels) the head —
    ``fc_out``, the loss, the per-pattern epoch accumulators, the loss log and ``fc_out``'s backward — is the one
    launch of ``MosiEngine.head_regress``; everything else is the classification step's schedule."""

    def __init__(self, model: "UttFusionModel", optimizer: FusedAdam, loss_functions, batch: int, steps,
                 use_graph: bool = True, allreduce=None, ragged: bool = False, text_lengths: bool = False):
        if not isinstance(optimizer, FusedAdam):
            raise L.TspmError("FusedMosiStep needs FusedAdam (the flat gradient buffer the kernels write)")
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise L.TspmError("FusedMosiStep runs on the MI355X: move the model to cuda first")
        # 1..8 groups (the clip norm spans all of them); frozen encoders; refusals name the module or parameter
        # and what FusedAdam's flat buffers hold (fixed when it was built) is exactly what trains now
        fgs = optimizer.flat_groups()
        self.frozen = check_param_groups(model, optimizer.param_groups, allreduce, fgs)
        self._flags = model.flag_state()[0]
        self.multi = len(fgs) > 1
        self.model, self.opt, self.N, self.T = model, optimizer, batch, norm_steps(steps)
        # regress = (kind, weight): the one-launch regression head
        self.weight, self.regress = _loss_mode("FusedMosiStep", model, loss_functions, self._head_rows(batch))
        self.ragged, self.text_lengths = bool(ragged), bool(text_lengths)
        self.eng = self._build_engine(dev, steps)
        # the dropout counter is group 0's step (all groups advance together)
        self.eng.rng_ctr_ptr = fgs[0].hyper.data_ptr() + L.HYPER_STEP_OFFSET
        if model.clip is not None:
            optimizer.clip_coef = self.eng.clip_coef
        self._init_graph(use_graph, dev)
        self.allreduce = allreduce
        self.log = None  # metrics.ClassificationLog (train predictions on the device); RegressionLog in regression mode

    def _head_rows(self, batch: int) -> int:
        """The rows the head runs over (the regression head's limit applies to them)."""
        return batch

    def _build_engine(self, dev, steps):
        return MosiEngine(self.model, self.N, steps, dev, ragged=self.ragged, text_lengths=self.text_lengths)

    @property
    def keep_override(self):
        return self.eng.keep_override

    @keep_override.setter
    def keep_override(self, v):
        self.eng.keep_override = v

    def _fwd_bwd(self) -> None:
        sh = L.stream_handle()
        e = self.eng
        if self.regress is not None:
            _check_regress_log(self.log)
            e.forward(sh, True, head=False)
            e.head_regress(sh, True, *self.regress, self.log)
            e.backward(sh, from_head=False)
            return
        e.forward(sh, True)
        e.loss_fn(sh, self.weight, True, True)
        if self.log is not None:
            e.classify_update(sh, self.log)
        e.backward(sh)

    def _opt(self) -> None:
        sh = L.stream_handle()
        if self.multi:  # several groups: the same four launches (sum of squares, coefficient, counters, update)
            if self.model.clip is not None:
                self.eng.clip(sh, [fg.grad for fg in self.opt.flat_groups()], self.opt.grad_scale)
            self.opt.launch_multi(sh)
            return
        if self.model.clip is not None:
            fg = self.opt.flat_groups()[0]
            self.eng.clip(sh, fg.grad, self.opt.grad_scale)
        self.opt.launch(sh)

    def _all(self) -> None:
        self._fwd_bwd()
        if self.allreduce is None:
            self._opt()

    def step(self, A, V, T, labels, lengths: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """``lengths`` (a ragged and / or text_lengths step only): ``{"audio": int [B], "video": int [B]}`` and, with
        ``text_lengths``, ``"text"``, copied on the device into the length buffers the captured graph reads — one graph
        serves every batch of this padded ``steps``."""
        self.eng.load(A, V, T, labels, self.regress is not None)
        self.eng.set_lengths(lengths)
        self.run()
        return {"loss": self.eng.loss, "logits": self.eng.logits}

    def _bind_log(self) -> tuple:
        """The graph's key, after anything host-side the current log decides is in place: here the log alone (the
        launches carry raw pointers into it)."""
        return (self.log,)

    def run(self) -> None:
        flags, (frozen, _) = self.model.flag_state()
        if flags != self._flags:
            raise L.TspmError(f"FusedMosiStep: requires_grad flags changed since this step was built (frozen then: "
                              f"{self.frozen}, now: {frozen}).  FusedAdam's flat buffers hold what was trainable when it "
                              f"was built: build a new FusedAdam for the new flags, then take model.fused_step(...) with it")
        self.model.train()
        self.opt.sync_hyper()
        self.eng.apply_keep_override()
        if self.model.clip is not None:
            self.opt.clip_coef = self.eng.clip_coef
        self.replay_or_enqueue(self._all, self._bind_log())
        if self.allreduce is not None:
            self.allreduce()
            self._opt()
        self.opt.note_steps(1)
        self.calls += 1


class FusedMosiPatternStep(FusedMosiStep):
    """``FusedMosiStep`` that trains every batch row under each of ``patterns`` (P of the seven missing-modality
    patterns; default all) in one step (``MosiPatternEngine(backward=True)``): the batch arrives
    unmasked, once; the encoders run forward and backward over 2B rows (the batch and zero rows), the classifier over
    the P*B expanded rows.  ``FusedMosiStep``'s order — ``check_param_groups`` (1..8 groups, frozen encoders), forward,
    the loss with its gradient, ``tspm_classify_update`` over the P*B rows with the expanded group ids when a log is
    attached (ONE loss entry per step, confusion counts per pattern), backward, clip, Adam; the graph runner's
    lifecycle (key: the log and its group order); the dropout counter is group 0's step.  The loss is the weighted
    mean cross-entropy over all P*B rows, i.e. a plain step on the replicated batch cat_p(A*ka_p, V*kv_p, T*kt_p) with
    labels and lengths tiled P times; BatchNorm1d (MOSEI) takes its statistics over the P*B rows and updates its running statistics once;
    the TextCNN dropout mask is per encoder row (2B; shared by the patterns that read the row), the classifier masks
    per classifier row (``keep_override``: ``"text"`` [2B, nc], ``"cls{j}"`` [P*B, w_j]).  Regression mode runs
    ``head_regress`` over the P*B rows, so P*B is within the head's 1024 rows or the step is refused.  ``step`` returns
    ``{"loss", "logits"}`` with ``logits`` [P, B, C]; ``run`` serves inputs gathered in place
    (``mosi_data.MOSI.loader(all_patterns=True)``).  ``allreduce`` is refused: data parallelism is not built for this
    step."""

    def __init__(self, model: "UttFusionModel", optimizer: FusedAdam, loss_functions, batch: int, steps, patterns=None,
                 use_graph: bool = True, ragged: bool = False, text_lengths: bool = False, allreduce=None):
        if allreduce is not None:
            raise L.TspmError("FusedMosiPatternStep: allreduce (data parallelism) is not built for the all-pattern step; "
                              "it runs on one device")
        self.patterns = norm_patterns(patterns)
        super().__init__(model, optimizer, loss_functions, batch, steps, use_graph=use_graph, ragged=ragged,
                         text_lengths=text_lengths)

    def _head_rows(self, batch: int) -> int:
        return len(self.patterns) * batch

    def _build_engine(self, dev, steps):
        return MosiPatternEngine(self.model, self.N, steps, dev, self.patterns, ragged=self.ragged,
                                 text_lengths=self.text_lengths, backward=True)

    def _fwd_bwd(self) -> None:
        sh, e = L.stream_handle(), self.eng
        if self.regress is not None:
            _check_regress_log(self.log)
            e.forward(sh, head=False, regress=True, train=True)
            e.cls.head_regress(sh, True, *self.regress, self.log)
            e.backward(sh, from_head=False)
            return
        e.forward(sh, train=True)
        e.cls.loss_fn(sh, self.weight, True, True)
        if self.log is not None:
            e.cls.classify_update(sh, self.log)
        e.backward(sh)

    def step(self, A, V, T, labels, lengths: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """The unmasked batch ([B, T_m, F] each, B labels); ``lengths`` as in ``FusedMosiStep.step`` (B per modality:
        the zero rows run as long as their real rows).  → ``{"loss": [1], "logits": [P, B, C]}``."""
        self.eng.load(A, V, T, labels, self.regress is not None)
        self.eng.set_lengths(lengths)
        self.run()
        return {"loss": self.eng.cls.loss, "logits": self.eng.logits}

    def _bind_log(self) -> tuple:
        # the log's group order decides the ids the expansion writes (host values of the launch)
        if self.log is not None and self.eng.group_names != tuple(self.log.groups):
            self.eng.set_groups(self.log.groups)
        return (self.log, self.eng.group_names)


class FusedMosiEvalStep(L.GraphRunner):
    """``validation_step``'s device work (utt_fusion.py:202-244) for one (batch, steps) shape as one HIP graph:
    eval-mode forward (no dropout; running statistics in the MOSEI classifier BatchNorm1d), the loss group's
    cross-entropy, and ``tspm_classify_update`` (softmax argmax, per-pattern confusion counts, the batch loss
    appended to the epoch's log) — no host synchronisation.  In regression mode (one-output ``fc_out`` and a single
    mean L1 / MSE term) the head is ``MosiEngine.head_regress`` in forward-only mode and ``log`` a RegressionLog.  Inputs are the engine's time-major buffers
    (``mosi_data.MOSI.device_loader(step_for=...)`` gathers into them) or a batch-first batch via ``step``."""

    def __init__(self, model: "UttFusionModel", loss_functions, batch: int, steps, log, use_graph: bool = True,
                 ragged: bool = False, text_lengths: bool = False):
        dev = next(model.parameters()).device
        self.ragged, self.text_lengths = bool(ragged), bool(text_lengths)
        self.model, self.N, self.T, self.log = model, batch, norm_steps(steps), log
        self.weight, self.regress = _loss_mode(type(self).__name__, model, loss_functions, batch)
        self.eng = self._build_engine(dev, steps)
        self._init_graph(use_graph, dev)

    def _build_engine(self, dev, steps):
        return self.model._engine(self.N, steps, dev, self.ragged, self.text_lengths)

    def _bind_log(self) -> tuple:
        """As ``FusedMosiStep._bind_log``: the graph's key is the log."""
        return (self.log,)

    def _all(self) -> None:
        sh, e, lg = L.stream_handle(), self.eng, self.log
        if self.regress is not None:
            _check_regress_log(lg)
            e.forward(sh, False, head=False)
            e.head_regress(sh, False, *self.regress, lg)
            return
        e.forward(sh, False)
        e.loss_fn(sh, self.weight, False)
        e.classify_update(sh, lg)

    def step(self, A, V, T, labels, lengths: Optional[Dict[str, torch.Tensor]] = None) -> None:
        self.eng.load(A, V, T, labels, self.regress is not None)
        self.eng.set_lengths(lengths)
        self.run()

    def run(self) -> None:
        self.model.eval()
        self.replay_or_enqueue(self._all, self._bind_log())
        self.calls += 1


# ------------------------------------------------------------------------------------------------
# every missing-modality pattern of a batch from one encoder pass
# ------------------------------------------------------------------------------------------------
ALL_PATTERNS = tuple(PATTERNS)  # "atv", "at", "av", "tv", "a", "t", "v": data/mosi.py:61-69 order (mosi_data.PATTERNS)


def norm_patterns(patterns=None) -> tuple:
    """The patterns of a fused-pattern pass as a tuple of names: all seven in ``ALL_PATTERNS`` order by default, or the
    given subset in the given order.  Unknown names raise ``ValueError`` (as the dataset's constructor does); an empty or
    repeating selection too."""
    if patterns is None:
        return ALL_PATTERNS
    pats = tuple(str(p) for p in patterns)
    bad = set(pats) - set(ALL_PATTERNS)
    if bad:
        raise ValueError(f"Invalid patterns: {bad}")
    if not pats or len(set(pats)) != len(pats):
        raise ValueError(f"patterns: 1..{len(ALL_PATTERNS)} distinct names among {ALL_PATTERNS}, got {pats!r}")
    return pats


def _pattern_key(key: tuple, patterns: tuple) -> tuple:
    """The cache key of a fused-pattern engine or step: the plain key behind a ("patterns", names) head.  Every other
    key of these caches starts with an int (a batch size or an ``id``), so the two families cannot collide."""
    return (("patterns", tuple(patterns)),) + key


class MosiPatternEngine:
    """The eval-mode forward of a batch under ``patterns`` (P of the seven missing-modality patterns) from ONE encoder
    pass.  Under any pattern a modality is the real input or the zeroed input, so the encoders run once over 2B rows —
    rows [0, B) of the three time-major inputs hold the batch, rows [B, 2B) are zero (zeroed at allocation, never
    written) — and ``enc.fused`` [2B, E] then holds every embedding the patterns need.  ``tspm_pattern_expand`` builds
    the P*B classifier rows (pattern-major: row p*B + b), their labels and group ids in one launch, and the classifier
    runs once on them (no dropout, running statistics in the BatchNorm1d).  ``enc`` is a forward-only ``MosiEngine``
    without a classifier at 2B rows, ``cls`` one without encoders at P*B rows: no LSTM or TextCNN buffer grows with P.
    With ``ragged`` / ``text_lengths`` the length buffers are 2B long and both halves carry the batch's lengths (a zero
    row runs exactly as long as its real row): callers write the first B (``set_lengths``, or the loader's gather), the
    forward mirrors them.

    ``backward=True`` is the training form (``FusedMosiPatternStep``): both halves plan their backward —
    ``enc`` at 2B rows ``dfused`` [2B, E], the LSTM ``dg`` buffers, the weight-gradient plan and the TextCNN keep mask
    [2B, nc]; ``cls`` at P*B rows ``dlogits``, ``dh``, ``dr``, ``dfused`` [P*B, E], its layers' keep masks [P*B, w] and
    the clip buffers.  ``forward(train=True)`` draws the masks and runs both halves in training mode; ``backward`` runs
    the classifier's backward over the P*B rows, ``tspm_pattern_expand_bwd`` (the expansion's adjoint: ``cls.dfused``
    folded onto the 2B rows of ``enc.dfused``, the trainable encoders' columns only) and the encoders' backward over 2B
    rows.  Defined semantics: the loss is the weighted mean over all P*B rows — a plain step on the replicated batch
    cat_p(A*ka_p, V*kv_p, T*kt_p); the MOSEI classifier's BatchNorm1d takes its batch statistics over the P*B rows and
    updates its running statistics once per step, as on the replicated batch; the TextCNN dropout mask is drawn per
    ENCODER row (2B rows: a row's mask is shared by every pattern that reads the row), the classifier masks per
    classifier row (P*B); ``keep_override`` takes ``"text"`` as [2B, nc] and ``"cls{j}"`` as [P*B, w_j].  Real rows and
    zero rows both contribute to every encoder parameter's gradient (a zero row's embedding depends on the biases and,
    with lengths, on the row's own length)."""

    def __init__(self, model: "UttFusionModel", batch: int, steps, device: torch.device, patterns=None,
                 ragged: bool = False, text_lengths: bool = False, groups: Optional[Sequence[str]] = None,
                 backward: bool = False):
        if torch.device(device).type != "cuda":
            raise L.TspmError("UttFusionModel (tspm_amd) runs on the MI355X only (no CPU fallback)")
        self.m, self.B, self.T, self.device = model, int(batch), norm_steps(steps), device
        self.patterns = norm_patterns(patterns)
        self.P = P = len(self.patterns)
        self.ragged, self.text_lengths = bool(ragged), bool(text_lengths)
        B = self.B
        self.trainable = bool(backward)
        self.enc = self._build_enc(steps)
        self.cls = MosiEngine(model, P * B, steps, device, encoders=False, backward=self.trainable)
        self.keep_override: Optional[Dict[str, torch.Tensor]] = None
        self.rng_ctr_ptr: Optional[int] = None
        self._host_ctr: Optional[torch.Tensor] = None
        if self.trainable:  # the clip buffers live on the classifier half
            self.clip, self.clip_coef, self.total_norm = self.cls.clip, self.cls.clip_coef, self.cls.total_norm
        self.Ts, self.E = self.enc.Ts, self.enc.E
        self.labels = torch.zeros(B, dtype=torch.int64, device=device)
        self.labels_f = torch.zeros(B, dtype=torch.float32, device=device)
        self.logits = self.cls.logits.view(P, B, -1)
        self.losses = torch.zeros(P, dtype=torch.float32, device=device)  # one loss per pattern, in pattern order
        self._keep = (ctypes.c_int32 * (3 * P))(*[int(ch in p) for p in self.patterns for ch in "avt"])
        self.set_groups(groups)
        self._plan_inputs()

    def _build_enc(self, steps):
        """The encoder half at 2B rows (``MosiCachedPatternEngine`` puts its cache reader here)."""
        return MosiEngine(self.m, 2 * self.B, steps, self.device, ragged=self.ragged, text_lengths=self.text_lengths,
                          classifier=False, backward=self.trainable)

    def _plan_inputs(self) -> None:
        """What ``load`` / ``set_lengths`` and the loader's gather write: views of the encoder half's inputs."""
        B, device = self.B, self.device
        self.A, self.V, self.X = self.enc.A, self.enc.V, self.enc.X   # [T_m, 2B, F]: the batch in rows [0, B)
        # the first halves of the 2B-long length buffers: what set_lengths and the loader's gather write
        self._len_bufs = ([(self.enc.lens["a"], "audio", self.Ts[0]), (self.enc.lens["v"], "video", self.Ts[1])]
                          if self.ragged else [])
        if self.text_lengths:
            self._len_bufs.append((self.enc.text_lens, "text", self.Ts[2]))
        self.lens = {"a": self.enc.lens["a"][:B], "v": self.enc.lens["v"][:B]} if self.ragged else None
        self.text_lens = self.enc.text_lens[:B] if self.text_lengths else None
        eng = self.enc
        self._index = torch.arange(B, dtype=torch.int64, device=device)
        self._lens = {T_m: eng._lens[T_m][:B] for T_m in eng._lens}
        self._offs = {T_m: eng._offs[T_m][:B] for T_m in eng._offs}

    def set_groups(self, groups: Optional[Sequence[str]]) -> None:
        """The group id of each pattern = its index in ``groups`` (a log's group names; default: ``ALL_PATTERNS``).  Host
        values copied into the launch: set them before a graph is captured."""
        names = list(ALL_PATTERNS if groups is None else groups)
        try:
            self._group = (ctypes.c_int32 * self.P)(*[names.index(p) for p in self.patterns])
        except ValueError:
            raise L.TspmError(f"patterns {self.patterns} are not all among the log's groups {names}") from None
        self.group_names = tuple(names)

    def set_lengths(self, lengths: Optional[Dict[str, torch.Tensor]]) -> None:
        """The batch's B lengths into the first half of each 2B-long length buffer (``MosiEngine.set_lengths``'s rules);
        the forward copies them to the second half."""
        if not self.ragged and not self.text_lengths:
            if lengths is not None:
                raise L.TspmError("MosiPatternEngine: lengths given to an engine built without ragged=True")
            return
        lengths = lengths or {}
        _check_lengths_arg(lengths, self.ragged, self.text_lengths)
        for buf, nm, T_m in self._len_bufs:
            _set_lengths(buf[:self.B], lengths.get(nm), T_m, nm)

    def load(self, A: torch.Tensor, V: torch.Tensor, T: torch.Tensor, labels: Optional[torch.Tensor] = None,
             regress: bool = False) -> None:
        """Batch-first [B, T_m, F] tensors → rows [0, B) of the time-major buffers (``MosiEngine.load``'s launches at
        the 2B-row time stride); ``labels`` as there."""
        sh = L.stream_handle()
        for src, dst, nm, T_m in zip((A, V, T), (self.A, self.V, self.X), _MODALITY_ORDER, self.Ts):
            _seq_load(src, dst, self.B, T_m, self._index, self._offs[T_m], self._lens[T_m], nm, sh)
        if labels is not None:
            dst = self.labels_f if regress else self.labels
            if labels.data_ptr() != dst.data_ptr():
                dst.copy_(labels.reshape(-1).to(dst.dtype), non_blocking=True)

    def apply_keep_override(self) -> None:
        """Copy injected dropout masks (parity hook) into the keep buffers of the two halves: ``"text"`` [2B, nc] (one
        mask per encoder row), ``"cls{j}"`` [P*B, w_j]; called before the step runs, outside any captured graph."""
        if self.keep_override is None:
            return
        dsts = [("text", self.enc.keeps[0])] + [(f"cls{j}", k) for j, k in enumerate(self.cls.keeps[1:])]
        for k, dst in dsts:
            dst.copy_(self.keep_override[k].reshape(dst.shape).to(torch.uint8), non_blocking=True)

    def _keep_masks(self, sh: int) -> None:
        """Fresh keep masks for one training forward (``MosiEngine._keep_masks``'s seeds, rates and counter): the TextCNN
        mask over the 2B encoder rows, the classifier masks over the P*B classifier rows."""
        pt, pc = float(self.m.netT.dropout.p), float(self.m.netC.dropout_p)
        if (pt <= 0 and pc <= 0) or self.keep_override is not None:
            return
        if self.rng_ctr_ptr is None:
            self._host_ctr = torch.zeros(1, dtype=torch.int64, device=self.device)
            self.rng_ctr_ptr = self._host_ctr.data_ptr()
        lib, seed = L.lib(), self.m._rng_seed
        if pt > 0:
            L.check(lib.tspm_dropout_mask(self.enc.keep_all.numel(), pt, seed, self.rng_ctr_ptr,
                                          self.enc.keep_all.data_ptr(), sh), "dropout_mask (text)")
        if pc > 0:
            L.check(lib.tspm_dropout_mask(self.cls.keep_all.numel(), pc, seed ^ _CLS_SEED_SALT, self.rng_ctr_ptr,
                                          self.cls.keep_all.data_ptr(), sh), "dropout_mask (classifier)")
        if self._host_ctr is not None and self.rng_ctr_ptr == self._host_ctr.data_ptr():
            self._host_ctr.add_(1)  # outside FusedMosiPatternStep nothing else advances the counter

    def forward(self, sh: int, head: bool = True, regress: bool = False, train: bool = False) -> None:
        """Length mirror, the encoders over 2B rows, ``tspm_pattern_expand``, the classifier over P*B rows (``head=False``
        stops before ``fc_out``); everything on the caller's stream (the LSTM half forks as in ``MosiEngine``),
        graph-capturable.  ``regress``: the float32 labels travel instead of the int64 ones.  ``train`` (a
        ``backward=True`` engine): the dropout masks are drawn first and both halves run in training mode."""
        B, e, c = self.B, self.enc, self.cls
        if train and not self.trainable:
            raise L.TspmError("MosiPatternEngine: a training forward needs an engine built with backward=True")
        for buf, _, _ in self._len_bufs:
            buf[B:].copy_(buf[:B])  # on the current stream, which is the one `sh` names
        if train:
            self._keep_masks(sh)
        e._forward_encoders(sh, train)
        a, v, t = self.m.netA, self.m.netV, self.m.netT
        src, dst = (self.labels_f, c.labels_f) if regress else (self.labels, c.labels)
        L.check(L.lib().tspm_pattern_expand(B, self.P, self._keep, self._group, a.hidden_size, v.hidden_size,
                                            t.hidden_size, e.fused.data_ptr(), self.E, c.fused.data_ptr(), self.E,
                                            src.data_ptr(), dst.data_ptr(), src.element_size(), c.groups.data_ptr(), sh),
                "pattern_expand")
        c._forward_classifier(sh, train, head)

    def backward(self, sh: int, from_head: bool = True) -> None:
        """The classifier's backward over the P*B rows into ``cls.dfused``, ``tspm_pattern_expand_bwd`` into
        ``enc.dfused`` (``modalities`` = the trainable encoders), the encoders' backward over the 2B rows
        (``MosiEngine``'s, side-stream fork included).  ``from_head=False``: ``cls.head_regress`` wrote ``dh[-1]`` and
        ``fc_out``'s gradients.  With every encoder frozen layer 0's ``linear_bwd`` gets no ``dx`` and neither the
        adjoint nor any encoder backward is launched; ``MosiEngine.backward``'s flag checks."""
        e, c = self.enc, self.cls
        c._check_flags()
        c._backward_classifier(sh, from_head)
        mods = sum(1 << i for i, k in enumerate("avt") if e.trains[k])
        if not mods:
            return
        a, v, t = self.m.netA, self.m.netV, self.m.netT
        L.check(L.lib().tspm_pattern_expand_bwd(self.B, self.P, self._keep, a.hidden_size, v.hidden_size, t.hidden_size,
                                                c.dfused.data_ptr(), self.E, e.dfused.data_ptr(), self.E, mods, sh),
                "pattern_expand_bwd")
        e._backward_encoders(sh)


class FusedMosiPatternEvalStep(FusedMosiEvalStep):
    """``FusedMosiEvalStep`` for every pattern of a batch at once (``MosiPatternEngine``): the batch arrives unmasked,
    once; one HIP graph runs the 2B-row encoder pass, the expansion, the classifier on P*B rows and then, for each
    pattern in order, the existing loss and metrics launches on its B rows (``tspm_cross_entropy`` +
    ``tspm_classify_update``, or ``tspm_regress_head_step`` forward-only in regression mode) — so the epoch's log gets
    the same P loss entries, in pattern order, that P replays of the per-pattern step write, and the per-pattern
    accumulators are filled through the expanded group ids.  The graph runner's lifecycle (key: the log and its group
    order); no host synchronisation; the refusals of ``FusedMosiEvalStep``.  ``step`` takes a batch-first batch,
    ``run`` serves inputs gathered in place (``mosi_data.MOSI.loader(fuse_patterns=True)``)."""

    def __init__(self, model: "UttFusionModel", loss_functions, batch: int, steps, log, patterns=None,
                 use_graph: bool = True, ragged: bool = False, text_lengths: bool = False):
        self.patterns = norm_patterns(patterns)
        super().__init__(model, loss_functions, int(batch), steps, log, use_graph=use_graph, ragged=ragged,
                         text_lengths=text_lengths)

    def _build_engine(self, dev, steps):
        return self.model._pattern_engine(self.N, steps, dev, self.patterns, self.ragged, self.text_lengths)

    def _bind_log(self) -> tuple:
        if self.eng.group_names != tuple(self.log.groups):  # the log's group order decides the ids the launch carries
            self.eng.set_groups(self.log.groups)
        return (self.log, self.eng.group_names)

    def _all(self) -> None:
        sh, e, lg, B = L.stream_handle(), self.eng, self.log, self.N
        if self.regress is not None:
            _check_regress_log(lg)
            e.forward(sh, head=False, regress=True)
            for p in range(e.P):
                e.cls.head_regress(sh, False, *self.regress, lg, rows=(p * B, B), loss=e.losses[p:p + 1])
            return
        e.forward(sh)
        for p in range(e.P):
            e.cls.loss_fn(sh, self.weight, False, rows=(p * B, B), loss=e.losses[p:p + 1])
            e.cls.classify_update(sh, lg, rows=(p * B, B), loss=e.losses[p:p + 1])


# ------------------------------------------------------------------------------------------------
# the head stage on cached encoder features
# ------------------------------------------------------------------------------------------------
ALL_FROZEN = tuple(nm for nm, _ in ENCODER_MODULES)


class UttEmbeddingCache:
    """What the three FROZEN encoders of a ``UttFusionModel`` compute for every sample of one ``mosi_data.MOSI`` split,
    computed once: ``emb [n][W]`` fp32 with row i = ``[ eA(i) | eV(i) | pooled(i) ]``, ``W = ha + hv + nc`` — the two
    LSTM embeddings (any ``embd_method``) and the TextCNN's time-max output (``nc = 3 * out_channels``) BEFORE its
    dropout — ``zero [n_zero][W]``, the same for the zeroed inputs a dropped modality feeds its encoder (one row for the
    split; with ``use_lengths`` one per sample, as a zero row's embedding depends on its own lengths), and
    ``labels_all``, the device corpus's own label tensor (int64, or float32 scores).  A frozen ``netT`` in a train-mode
    model still applies its dropout, so the dropout, the embedding ``Linear nc -> ht`` + ReLU and everything from
    ``fused`` on stay in the step (``FusedMosiCachedStep`` / ``FusedMosiCachedEvalStep``, which read the cache by sample
    index through ``tspm_utt_cache_rows``).  16k rows x 512 columns x 4 B = 33 MB at MOSEI's default widths, twice that
    with per-sample zero rows.

    Without lengths an embedding depends on the padded length (the LSTM runs through the padding), so the cache is
    built for ONE ``steps`` value, the split's corpus-wide padded lengths under the caller's ``pad_to``
    (``DeviceMosiCorpus.batch_steps(arange(n), pad_to)``), and remembers it: its semantics are those of the uncached
    loader with a ``pad_to`` that covers the corpus (one step shape for the epoch), or of the ragged path under any
    padding.

    The fill (``refresh()``) runs forward-only encoder halves ``MosiEngine(model, 2c, steps, classifier=False,
    backward=False)`` exactly as ``MosiPatternEngine.forward`` runs its own: the chunk gathered into rows [0, c), rows
    [c, 2c) left zero, lengths mirrored, ``_forward_encoders(sh, train=False)`` — in sample order, in chunks of
    ``chunk`` rows plus one engine for the short last chunk; no new launch.  It is refused unless all three encoders are
    frozen.  The cache remembers the model's ``flag_state()``, each encoder's weights generation and the generation of
    the model's engine table: a changed flag, ``load_state_dict`` on the model or an encoder (``load_pretrained()``) and
    anything that drops the engines (``.to()``) make it stale, and a stale cache, or another model's, is refused with a
    ``TspmError`` that says to call ``refresh()``.  Weights written through raw pointers (an in-place ``copy_``) cannot
    be detected: whoever changes frozen weights that way calls ``refresh()``."""

    def __init__(self, model: "UttFusionModel", dataset, steps, chunk: int = 128):
        import weakref
        if int(chunk) < 1:
            raise ValueError("chunk must be >= 1")
        # the model is held weakly: the dataset's table of caches is keyed by the model and must not keep it alive
        self._model_ref, self.ds, self.chunk = weakref.ref(model), dataset, int(chunk)
        self.dc = dataset.device_corpus
        self.n, self.steps = int(self.dc.n), norm_steps(steps)
        self.ha, self.hv, self.nc = model.netA.hidden_size, model.netV.hidden_size, 3 * model.netT.out_channels
        self.W = self.ha + self.hv + self.nc
        self.per_sample_zero = bool(dataset.use_lengths)
        self.n_zero = self.n if self.per_sample_zero else 1
        self.emb: Optional[torch.Tensor] = None
        self.zero: Optional[torch.Tensor] = None
        self.labels_all = self.dc.labels
        self.fill_seconds, self.fills, self._stamp = 0.0, 0, None
        self.refresh()

    @property
    def model(self) -> "UttFusionModel":
        m = self._model_ref()
        if m is None:
            raise L.TspmError("this UttEmbeddingCache's model no longer exists")
        return m

    def _now(self):
        m = self.model
        return (m.flag_state()[0], tuple(getattr(getattr(m, attr), "_weights_generation", 0)
                                         for _, attr in ENCODER_MODULES), m._engines_generation)

    def stale_reason(self) -> Optional[str]:
        """None while the cache is current, else what changed since the fill."""
        was, now = self._stamp, self._now()
        if now[0] != was[0]:
            return "the model's requires_grad flags (its frozen encoders) changed since the fill"
        if now[1] != was[1] or now[2] != was[2]:
            return "an encoder's weights were loaded or moved (load_state_dict, load_pretrained, .to()) since the fill"
        return None

    def check(self, model=None) -> "UttEmbeddingCache":
        """Refuse a cache built for another model, and a stale one."""
        if model is not None and model is not self.model:
            raise L.TspmError("this UttEmbeddingCache was built for another model: its rows are that model's encoders' "
                              "outputs (dataset.embedding_cache(model) builds this model's)")
        why = self.stale_reason()
        if why is not None:
            raise L.TspmError(f"stale UttEmbeddingCache: {why}; call refresh() on it (with all three encoders frozen) "
                              "before the next use")
        return self

    def refresh(self) -> "UttEmbeddingCache":
        """(Re)compute every row and the zero rows, into the same storage; returns self."""
        import time
        model, dc, ds = self.model, self.dc, self.ds
        if frozen_encoders(model) != ALL_FROZEN:
            raise L.TspmError("UttEmbeddingCache needs frozen encoders - all of netA, netV and netT (finetune_param_groups("
                              "..., freeze=('audio', 'video', 'text'))): a trainable encoder's outputs change every "
                              "step, so there is nothing constant to cache")
        dev = next(model.parameters()).device
        if dev.type != "cuda" or dev != dc.device:
            raise L.TspmError(f"UttEmbeddingCache: the model is on {dev}, the corpus on {dc.device} (both on the ROCm "
                              f"device)")
        if self.nc % 4 or (self.ha + self.hv) % 4:
            raise L.TspmError("UttEmbeddingCache: the cache rows are moved 16 bytes at a time - TextCNN out_channels and "
                              "the LSTM widths must be multiples of 4")
        f32 = dict(device=dev, dtype=torch.float32)
        if self.emb is None or self.emb.device != dev:
            self.emb = torch.empty(self.n, self.W, **f32)
            self.zero = torch.empty(self.n_zero, self.W, **f32)
        n, hav, ch = self.n, self.ha + self.hv, min(self.chunk, max(self.n, 1))
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        sh = L.stream_handle()
        order = torch.arange(n, dtype=torch.int64, device=dev)
        engines: Dict[int, MosiEngine] = {}
        with torch.no_grad():
            for lo in range(0, n, ch):
                c = min(ch, n - lo)
                eng = engines.get(c)
                if eng is None:
                    eng = engines[c] = MosiEngine(model, 2 * c, self.steps, dev, ragged=ds.use_lengths,
                                                  text_lengths=ds.text_lengths, classifier=False, backward=False)
                    eng.lab = torch.empty(c, dtype=dc.label_dtype, device=dev)
                bufs = ([("audio", eng.lens["a"]), ("video", eng.lens["v"])] if ds.use_lengths else []) + \
                       ([("text", eng.text_lens)] if ds.text_lengths else [])
                dc.gather(order[lo:lo + c], self.steps, {"audio": eng.A, "video": eng.V, "text": eng.X}, True, None,
                          eng.lab, {m: buf[:c] for m, buf in bufs} or None, rows=2 * c)
                for _, buf in bufs:
                    buf[c:].copy_(buf[:c])  # a zero row runs exactly as long as its real row
                eng._forward_encoders(sh, False)
                self.emb[lo:lo + c, :hav].copy_(eng.fused[:c, :hav])
                self.emb[lo:lo + c, hav:].copy_(eng.pooled[:c])
                if self.per_sample_zero:
                    self.zero[lo:lo + c, :hav].copy_(eng.fused[c:, :hav])
                    self.zero[lo:lo + c, hav:].copy_(eng.pooled[c:])
                elif lo == 0:
                    self.zero[0, :hav].copy_(eng.fused[c, :hav])
                    self.zero[0, hav:].copy_(eng.pooled[c])
        torch.cuda.synchronize(dev)
        self.fill_seconds = time.perf_counter() - t0
        self.fills += 1
        self._stamp = self._now()
        return self


class MosiCachedEngine(MosiEngine):
    """``MosiEngine`` whose encoder half is a stand-in that reads a ``UttEmbeddingCache``: it owns ``fused``, ``fc_in``
    and (a training engine) ``keeps[0]`` — no ``A`` / ``V`` / ``X``, ``lstm`` or ``conv_out`` buffer — and its
    ``_forward_encoders`` is ONE ``tspm_utt_cache_rows`` launch (the cached LSTM embeddings into ``fused``, the cached
    pooled features through the TextCNN's dropout into ``fc_in``, the labels) followed by the TextCNN's embedding Linear
    (``_text_embed``).  Everything else — masks, classifier, loss, log, backward, clip — is ``MosiEngine``'s own code.
    ``halves=1`` (``batch`` sample rows, with a classifier half): row b takes each modality from the cache or from the
    zero rows by ``row_keep[b]`` (uint8 [batch][3], written before each run).  ``halves=2`` (``batch`` = 2B rows, no
    classifier): the all-pattern layout ``MosiPatternEngine`` expands, the batch in rows [0, B), its zero rows in
    [B, 2B).  ``rows`` (int64 [B]) are the batch's sample indices.  Refused unless all three encoders are frozen."""

    def __init__(self, model: "UttFusionModel", batch: int, cache: UttEmbeddingCache, device, halves: int = 1, *,
                 classifier: bool = True, backward: bool = True):
        if _frozen_state(model)[0] != ALL_FROZEN:
            raise L.TspmError("the cached UTT-Fusion steps need frozen encoders - all of netA, netV and netT: a trainable "
                              "encoder's outputs change every step, so the cache cannot stand in for it")
        if model.netT.hidden_size % 4:
            raise L.TspmError("the cached UTT-Fusion steps move rows 16 bytes at a time: the TextCNN embd_size must be a "
                              "multiple of 4")
        self.cache, self.halves = cache, int(halves)
        self.rows = torch.zeros(int(batch) // self.halves, dtype=torch.int64, device=device)
        self.row_keep = (torch.ones(int(batch), 3, dtype=torch.uint8, device=device) if self.halves == 1 else None)
        self.label_dst: Optional[torch.Tensor] = None  # halves == 2: the pattern engine's label buffer
        super().__init__(model, batch, cache.steps, device, encoders=True, classifier=classifier, backward=backward)

    def _plan_encoders(self) -> None:
        """The stand-in's plan: the embedding Linear's input, nothing else."""
        t = self.m.netT
        self.C, self.nc = t.out_channels, 3 * t.out_channels
        self.fc_in = torch.empty(self.B, self.nc, device=self.device, dtype=torch.float32)
        self.lens = self.text_lens = None

    def _plan_backward(self) -> None:
        super()._plan_backward()
        if not self.has_classifier:
            del self.dfused  # nothing is trainable below the expansion: no adjoint is ever launched

    def set_lengths(self, lengths) -> None:
        if lengths is not None:
            raise L.TspmError("MosiCachedEngine: the cache holds the lengths' effect already; no lengths are taken")

    def _forward_encoders(self, sh: int, train: bool) -> None:
        m, t, cache = self.m, self.m.netT, self.cache
        tp = float(t.dropout.p)
        use_keep = train and tp > 0
        float_labels = cache.labels_all.dtype == torch.float32
        dst = self.label_dst if self.halves == 2 else (self.labels_f if float_labels else self.labels)
        d = L.UttCacheRowsDesc(batch=self.B // self.halves, halves=self.halves, w_audio=cache.ha, w_video=cache.hv,
                               w_pool=cache.nc, ld_cache=cache.W, ld_av=self.E, ld_pool=self.nc, n_rows=cache.n,
                               n_zero=cache.n_zero, label_bytes=4 if float_labels else 8,
                               scale=(1.0 / (1.0 - tp) if tp < 1 else 0.0) if use_keep else 1.0)
        d.emb, d.zero, d.rows = cache.emb.data_ptr(), cache.zero.data_ptr(), self.rows.data_ptr()
        d.row_keep = L.ptr(self.row_keep)
        if dst is not None:
            d.labels_all, d.labels_out = cache.labels_all.data_ptr(), dst.data_ptr()
        d.keep = self.keeps[0].data_ptr() if use_keep else None
        d.av_out, d.pool_out = self.fused.data_ptr(), self.fc_in.data_ptr()
        L.check(L.lib().tspm_utt_cache_rows(ctypes.byref(d), sh), "utt_cache_rows")
        _text_embed(self, t, sh, self.fused.data_ptr() + (cache.ha + cache.hv) * 4, self.E)


class MosiCachedPatternEngine(MosiPatternEngine):
    """``MosiPatternEngine`` on a ``UttEmbeddingCache``: ``enc`` is a ``MosiCachedEngine(halves=2)`` at 2B rows in
    place of the encoder half, ``cls`` the same classifier half at P*B rows; ``forward`` / ``backward`` /
    ``_keep_masks`` / ``apply_keep_override`` are the parent's, so the mask layout is its own (``"text"`` [2B, nc],
    ``"cls{j}"`` [P*B, w_j]).  The batch is ``rows`` (int64 [B] sample indices); there are no inputs and no lengths."""

    def __init__(self, model: "UttFusionModel", batch: int, cache: UttEmbeddingCache, device, patterns=None,
                 groups: Optional[Sequence[str]] = None, backward: bool = False):
        self.cache = cache
        super().__init__(model, batch, cache.steps, device, patterns, groups=groups, backward=backward)

    def _build_enc(self, steps):
        return MosiCachedEngine(self.m, 2 * self.B, self.cache, self.device, halves=2, classifier=False,
                                backward=self.trainable)

    def _plan_inputs(self) -> None:
        """No inputs and no lengths: the batch is ``rows``, and the cache reader writes this engine's labels."""
        self.rows = self.enc.rows
        self.enc.label_dst = self.labels_f if self.cache.labels_all.dtype == torch.float32 else self.labels
        self._len_bufs, self.lens, self.text_lens = [], None, None


def _cache_for_step(who: str, model: "UttFusionModel", cache, regress) -> UttEmbeddingCache:
    if not isinstance(cache, UttEmbeddingCache):
        raise L.TspmError(f"{who}: cache is a UttEmbeddingCache (mosi_data.MOSI.embedding_cache(model))")
    cache.check(model)
    if (regress is not None) != (cache.labels_all.dtype == torch.float32):
        raise L.TspmError(f"{who}: the regression head goes with float32 labels (regression_labels), cross-entropy with "
                          f"int64 class labels; the cache's corpus carries {cache.labels_all.dtype}")
    return cache


def _load_cached_batch(st, rows: torch.Tensor, row_keep, groups) -> None:
    """A cached step's batch into its engine's index buffers (device-to-device, outside any captured graph)."""
    e = st.eng
    if not torch.is_tensor(rows) or rows.dtype != torch.int64 or rows.numel() != st.N:
        raise L.TspmError(f"{type(st).__name__}: rows is an int64 tensor of {st.N} sample indices")
    e.rows.copy_(rows.reshape(-1), non_blocking=True)
    if st.per_sample:
        if row_keep is None or groups is None:
            raise L.TspmError(f"{type(st).__name__}(per_sample=True): step(rows, row_keep, groups) - uint8 [B][3] keep "
                              f"flags (audio, video, text) and int32 [B] group ids")
        e.row_keep.copy_(row_keep.reshape(st.N, 3).to(torch.uint8), non_blocking=True)
        e.groups.copy_(groups.reshape(-1).to(torch.int32), non_blocking=True)
    elif row_keep is not None or groups is not None:
        raise L.TspmError(f"{type(st).__name__}: row_keep / groups go with per_sample=True (this step runs every pattern)")


class FusedMosiCachedStep(FusedMosiPatternStep):
    """The UTT-Fusion train step of the head stage on a ``UttEmbeddingCache`` (all three encoders frozen): the batch is
    ``rows``, int64 [B] sample indices, and no encoder runs.  EVERY PATTERN (default; ``patterns``: a subset) is
    ``FusedMosiPatternStep``'s schedule with its ``_forward_encoders`` replaced — the two mask draws,
    ``tspm_utt_cache_rows`` (``halves = 2``), the embedding Linear over 2B rows, ``tspm_pattern_expand``, the
    classifier, the loss, ``tspm_classify_update`` or ``head_regress``, the classifier's backward with no ``dx`` at
    layer 0, clip and Adam — with its mask layout (``keep_override``: ``"text"`` [2B, nc], ``"cls{j}"`` [P*B, w_j]).
    ``per_sample=True`` is ``FusedMosiStep``'s schedule and mask layout at B rows: ``tspm_utt_cache_rows`` (``halves =
    1``) writes each row under its own ``row_keep`` flags straight into the classifier half's ``fused``;
    ``step(rows, row_keep, groups)`` takes uint8 [B][3] flags (audio, video, text) and int32 [B] group ids.  With the
    same mask bytes either form is bitwise the uncached step whose encoder leg returns the cache's rows.  Refused, with
    the reason: a trainable encoder, more than one ``FusedAdam`` group, ``allreduce``, a non-``FusedAdam`` optimizer, a
    cache that is stale, another model's or (a regression model on int64 labels, or the reverse) of the wrong labels.
    ``step`` returns ``{"loss", "logits"}``, logits [P, B, C] or [B, C]."""

    def __init__(self, model: "UttFusionModel", optimizer: FusedAdam, loss_functions, batch: int, cache, patterns=None,
                 per_sample: bool = False, use_graph: bool = True, allreduce=None):
        if allreduce is not None:
            raise L.TspmError("FusedMosiCachedStep: allreduce (data parallelism) is not built for the cached head stage")
        if not isinstance(optimizer, FusedAdam):
            raise L.TspmError("FusedMosiCachedStep needs FusedAdam (the flat gradient buffer the kernels write)")
        if frozen_encoders(model) != ALL_FROZEN:
            raise L.TspmError("FusedMosiCachedStep needs frozen encoders - all of netA, netV and netT; with a trainable "
                              "encoder take FusedMosiStep / FusedMosiPatternStep")
        if len(optimizer.flat_groups()) > 1:
            raise L.TspmError("FusedMosiCachedStep: one FusedAdam parameter group (only the classifier trains)")
        self.per_sample = bool(per_sample)
        if self.per_sample and patterns is not None:
            raise L.TspmError("FusedMosiCachedStep: patterns go with the every-pattern form, not per_sample=True")
        self.patterns = None if self.per_sample else norm_patterns(patterns)
        self.cache = _cache_for_step("FusedMosiCachedStep", model, cache, _regress_mode(model, loss_functions))
        FusedMosiStep.__init__(self, model, optimizer, loss_functions, int(batch), cache.steps, use_graph=use_graph)

    def _head_rows(self, batch: int) -> int:
        return batch if self.per_sample else len(self.patterns) * batch

    def _build_engine(self, dev, steps):
        if self.per_sample:
            return MosiCachedEngine(self.model, self.N, self.cache, dev, halves=1)
        return MosiCachedPatternEngine(self.model, self.N, self.cache, dev, self.patterns, backward=True)

    def _fwd_bwd(self) -> None:
        (FusedMosiStep if self.per_sample else FusedMosiPatternStep)._fwd_bwd(self)

    def _bind_log(self) -> tuple:
        key = (FusedMosiStep if self.per_sample else FusedMosiPatternStep)._bind_log(self)
        return key + (self.cache.emb.data_ptr(), self.cache.zero.data_ptr())

    def step(self, rows: torch.Tensor, row_keep: Optional[torch.Tensor] = None,
             groups: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        _load_cached_batch(self, rows, row_keep, groups)
        self.run()
        e = self.eng
        return {"loss": e.loss if self.per_sample else e.cls.loss, "logits": e.logits}

    def run(self) -> None:
        self.cache.check(self.model)
        super().run()


class FusedMosiCachedEvalStep(FusedMosiPatternEvalStep):
    """``FusedMosiPatternEvalStep`` (default; ``patterns``: a subset) or, with ``per_sample=True``,
    ``FusedMosiEvalStep`` on a ``UttEmbeddingCache``: the same loss and log launches, hence the same loss entries in the
    same order and the same counts, behind ``tspm_utt_cache_rows`` and the embedding Linear in place of the encoders; no
    dropout.  ``step(rows[, row_keep, groups])`` as ``FusedMosiCachedStep.step``; the loss returned is the per-pattern
    ``losses`` [P], or the batch's [1]."""

    def __init__(self, model: "UttFusionModel", loss_functions, batch: int, cache, log, patterns=None,
                 per_sample: bool = False, use_graph: bool = True):
        self.per_sample = bool(per_sample)
        if self.per_sample and patterns is not None:
            raise L.TspmError("FusedMosiCachedEvalStep: patterns go with the every-pattern form, not per_sample=True")
        self.patterns = None if self.per_sample else norm_patterns(patterns)
        self.cache = _cache_for_step("FusedMosiCachedEvalStep", model, cache, _regress_mode(model, loss_functions))
        FusedMosiEvalStep.__init__(self, model, loss_functions, int(batch), cache.steps, log, use_graph=use_graph)

    def _build_engine(self, dev, steps):
        if self.per_sample:
            return MosiCachedEngine(self.model, self.N, self.cache, dev, halves=1, backward=False)
        return MosiCachedPatternEngine(self.model, self.N, self.cache, dev, self.patterns)

    def _bind_log(self) -> tuple:
        key = (FusedMosiEvalStep if self.per_sample else FusedMosiPatternEvalStep)._bind_log(self)
        return key + (self.cache.emb.data_ptr(), self.cache.zero.data_ptr())

    def _all(self) -> None:
        (FusedMosiEvalStep if self.per_sample else FusedMosiPatternEvalStep)._all(self)

    def step(self, rows: torch.Tensor, row_keep: Optional[torch.Tensor] = None,
             groups: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        _load_cached_batch(self, rows, row_keep, groups)
        self.run()
        e = self.eng
        return {"loss": e.loss if self.per_sample else e.losses, "logits": e.logits}

    def run(self) -> None:
        self.cache.check(self.model)
        super().run()


# ------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------
def _modality(batch: Dict[Any, Any], name: str):
    for k, v in batch.items():
        kk = str(getattr(k, "value", k)).lower().split(".")[-1]
        if kk == name:
            return v
    raise KeyError(f"batch has no {name!r} modality key (keys: {list(batch.keys())})")


def _batch_steps(A: torch.Tensor, V: torch.Tensor, T: torch.Tensor):
    """(Ta, Tv, Tt) of three batch-first [B, T_m, F] tensors, each modality's length read from its own tensor."""
    for nm, x in zip(_MODALITY_ORDER, (A, V, T)):
        if x.dim() != 3:
            raise L.TspmError(f"{nm}: a batch-first [B, T, F] tensor, got shape {tuple(x.shape)}")
    return (int(A.shape[1]), int(V.shape[1]), int(T.shape[1]))


class _UttFn(torch.autograd.Function):
    """The whole UTT-Fusion forward as one autograd node (HIP schedule forward and backward), for the
    reference's own train_step sequence with a non-fused optimizer."""

    @staticmethod
    def forward(ctx, A, V, T, model: "UttFusionModel", lengths, *params):
        eng = model._engine(A.shape[0], _batch_steps(A, V, T), A.device, *_split_lengths(lengths))
        eng.load(A, V, T)
        eng.set_lengths(lengths)
        eng.apply_keep_override()
        eng.forward(L.stream_handle(), True)
        model._fwd_generation += 1
        ctx.model, ctx.eng, ctx.gen = model, eng, model._fwd_generation
        return eng.logits.clone()

    @staticmethod
    def backward(ctx, g):
        model, eng = ctx.model, ctx.eng
        if model._fwd_generation != ctx.gen:
            raise L.TspmError("UttFusionModel: another training forward ran before this backward")
        eng.dlogits.copy_(g.reshape(eng.dlogits.shape))
        grads: Dict[int, torch.Tensor] = {}

        def grad_of(p):
            t = grads.get(id(p))
            if t is None:
                t = torch.empty_like(p)
                grads[id(p)] = t
            return t
        for p in model.parameters():  # allocate on this stream before the backward forks its side stream
            if p.requires_grad:  # a frozen encoder's backward is skipped: no gradient, None returned
                grad_of(p)
        eng.grad_of = grad_of
        try:
            eng.backward(L.stream_handle())
        finally:
            eng.grad_of = lambda p: p.grad  # noqa: E731
        return (None, None, None, None, None, *[grads.get(id(p)) for p in model.parameters()])


class UttFusionModel(nn.Module):
    """models/msa/utt_fusion.py:25-294 drop-in (MultimodalMonitoringMixin hooks are not on the hot path)."""

    def __init__(self, netA: LSTMEncoder, netV: LSTMEncoder, netT: TextCNN, netC: FcClassifier, *,
                 clip: Optional[float] = None, pretrained_path: Optional[str] = None) -> None:
        super().__init__()
        self.netA = netA
        self.netV = netV
        self.netT = netT
        self.netC = netC
        self.clip = clip
        self.pretrained_path = pretrained_path
        self._rng_seed = int(torch.initial_seed()) & ((1 << 63) - 1)
        self._engines: Dict[Any, MosiEngine] = {}
        self._steps: Dict[Any, FusedMosiStep] = {}
        self._fwd_generation = 0
        self._flag_cache = None
        self._engines_generation = 0  # bumped whenever the engines are dropped (a UttEmbeddingCache's stamp reads it)

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._engines, self._steps, self._flag_cache = {}, {}, None
        self._engines_generation = getattr(self, "_engines_generation", 0) + 1
        return out

    def flag_state(self):
        """(flags, (frozen, error)): the ``requires_grad`` flags of the encoders' and the classifier's parameters as one
        tuple, and ``_frozen_state`` of them.  Asked for on every batch (the cache keys, ``FusedMosiStep.run``), so the
        parameter list is kept per set of modules and the answer per flag tuple: one attribute read per parameter."""
        md = self._modules
        mods = (md["netA"], md["netV"], md["netT"], md["netC"])
        c = self._flag_cache
        if c is None or c[0] != mods:  # a module swapped in (modules compare by identity)
            c = self._flag_cache = (mods, [p for m in mods for p in m.parameters()], {})
        flags = tuple([p.requires_grad for p in c[1]])
        state = c[2].get(flags)
        if state is None:
            state = c[2][flags] = _frozen_state(self)
        return flags, state

    def _engine(self, b: int, t, device, ragged: bool = False, text_lengths: bool = False) -> MosiEngine:
        """The cached MosiEngine for (batch, steps): ``t`` an ``int`` or a triple (Ta, Tv, Tt), keyed by ``norm_steps``;
        a ``ragged`` engine (per-sample lengths) and a ``text_lengths`` engine (the TextCNN's lengths) are separate
        entries, the key without them is unchanged."""
        if torch.device(device).type != "cuda":
            raise L.TspmError("UttFusionModel (tspm_amd) runs on the MI355X only (no CPU fallback)")
        t = norm_steps(t)
        key = _frozen_key(_text_lengths_key(_ragged_key((b, t, device), ragged), text_lengths), self.flag_state()[1][0])
        eng = self._engines.get(key)
        if eng is None:
            eng = MosiEngine(self, b, t, device, ragged=ragged, text_lengths=text_lengths)
            self._engines[key] = eng
        return eng

    def _pattern_engine(self, b: int, t, device, patterns=None, ragged: bool = False,
                        text_lengths: bool = False) -> "MosiPatternEngine":
        """The cached MosiPatternEngine for (patterns, batch, steps): ``_engine``'s key behind a ("patterns", names)
        head (``_pattern_key``), in the same cache — dropped with the others on ``.to()``."""
        if torch.device(device).type != "cuda":
            raise L.TspmError("UttFusionModel (tspm_amd) runs on the MI355X only (no CPU fallback)")
        t, pats = norm_steps(t), norm_patterns(patterns)
        key = _pattern_key(_text_lengths_key(_ragged_key((b, t, device), ragged), text_lengths), pats)
        eng = self._engines.get(key)
        if eng is None:
            eng = self._engines[key] = MosiPatternEngine(self, b, t, device, pats, ragged=ragged,
                                                         text_lengths=text_lengths)
        return eng

    @torch.no_grad()
    def forward_patterns(self, A: torch.Tensor, V: torch.Tensor, T: torch.Tensor, patterns=None,
                         lengths: Optional[Dict[str, torch.Tensor]] = None) -> torch.Tensor:
        """The eval-mode logits of the batch under every missing-modality pattern, [P, B, C], from one encoder pass
        (``MosiPatternEngine``): ``out[p]`` is what ``model.eval()(A * ka, V * kv, T * kt)`` gives for the keep factors
        of ``patterns[p]`` — a missing modality is the zeroed tensor through its encoder — up to summation order (the
        dense kernels' paths depend on the row count).  ``patterns``: all seven in ``ALL_PATTERNS`` order by default, or
        a subset in any order (unknown names: ``ValueError``).  ``A``, ``V``, ``T`` are the unmasked [B, T_m, F]
        sequences; ``lengths`` as in ``forward``.  The module's training flag is not changed."""
        pats = norm_patterns(patterns)
        A, V, T = A.float(), V.float(), T.float()
        if not (A.is_cuda and V.is_cuda and T.is_cuda):
            raise L.TspmError("UttFusionModel (tspm_amd) runs on the MI355X only; move the model and inputs to the "
                              "ROCm device (there is no CPU fallback)")
        eng = self._pattern_engine(A.shape[0], _batch_steps(A, V, T), A.device, pats, *_split_lengths(lengths))
        eng.load(A, V, T)
        eng.set_lengths(lengths)
        eng.forward(L.stream_handle())
        return eng.logits.clone()

    def fused_step(self, optimizer: FusedAdam, loss_functions, batch: int, steps,
                   ragged: bool = False, text_lengths: bool = False) -> FusedMosiStep:
        """The cached FusedMosiStep for (optimizer, loss group, batch, padded steps) — one captured graph per
        padded length (mosi_data.MOSI.device_loader(step_for=...) gathers straight into its inputs).  ``steps``: an
        ``int`` or a triple (Ta, Tv, Tt); the key is ``norm_steps(steps)``, so ``50`` and ``(50, 50, 50)`` give the
        same object.  ``ragged``: the step whose recurrences read per-sample lengths (``step(..., lengths=...)``) — one
        captured graph for every batch of this padded length, whatever its real lengths; a separate cache entry.
        ``text_lengths`` (independent of ``ragged``): the step whose TextCNN pooling reads ``lengths["text"]``; one more
        trailing key element."""
        key = self._fused_step_key(optimizer, loss_functions, batch, steps, ragged, text_lengths)
        st = self._steps.get(key)
        if st is None:
            st = FusedMosiStep(self, optimizer, loss_functions, int(batch), norm_steps(steps), ragged=ragged,
                               text_lengths=text_lengths)
            self._steps[key] = st
        return st

    def _fused_step_key(self, optimizer, loss_functions, batch: int, steps, ragged: bool = False,
                        text_lengths: bool = False, patterns=None) -> tuple:
        """``fused_step``'s cache key; with ``patterns`` the same key behind ``_pattern_key``'s ("patterns", names)
        head (``fused_pattern_step``)."""
        key = _frozen_key(_text_lengths_key(_ragged_key((id(optimizer), id(loss_functions), int(batch),
                                                         norm_steps(steps)), ragged), text_lengths),
                          self.flag_state()[1][0])
        return key if patterns is None else _pattern_key(key, norm_patterns(patterns))

    def fused_pattern_step(self, optimizer: FusedAdam, loss_functions, batch: int, steps, patterns=None,
                           ragged: bool = False, text_lengths: bool = False) -> "FusedMosiPatternStep":
        """The cached ``FusedMosiPatternStep`` for (patterns, optimizer, loss group, batch, padded steps): every row of
        a batch trained under each of ``patterns`` (names among ``ALL_PATTERNS``, default all seven) in one step.  Its
        key is ``fused_step``'s behind a ("patterns", names) head, in the same cache; ``fused_step``'s own keys and
        objects are unchanged."""
        pats = norm_patterns(patterns)
        key = self._fused_step_key(optimizer, loss_functions, batch, steps, ragged, text_lengths, pats)
        st = self._steps.get(key)
        if st is None:
            st = self._steps[key] = FusedMosiPatternStep(self, optimizer, loss_functions, int(batch), norm_steps(steps),
                                                         pats, ragged=ragged, text_lengths=text_lengths)
        return st

    def load_pretrained(self) -> None:
        """utt_fusion.py:63-78 (weights-only checkpoint load)."""
        if self.pretrained_path is None:
            raise ValueError("No pretrained weights loaded.")
        sd = torch.load(self.pretrained_path, map_location="cpu", weights_only=True)
        self.load_state_dict(sd["model_state_dict"])

    def get_encoder(self, modality):
        name = str(getattr(modality, "value", modality)).lower().split(".")[-1]
        enc = {"audio": self.netA, "video": self.netV, "text": self.netT}.get(name)
        if enc is None:
            raise ValueError(f"Unknown modality: {modality}")
        return enc

    def flatten_parameters(self) -> None:
        """utt_fusion.py:142-147 (cuDNN RNN weight flattening; nothing to do on this path)."""

    def forward(self, A: Optional[torch.Tensor] = None, V: Optional[torch.Tensor] = None,
                T: Optional[torch.Tensor] = None, *, is_embd_A: bool = False, is_embd_V: bool = False,
                is_embd_T: bool = False, lengths: Optional[Dict[str, torch.Tensor]] = None) -> torch.Tensor:
        """utt_fusion.py:105-140 with all three modalities given as [B, T, F] sequences (a missing modality
        is the zeroed tensor the dataset delivers, data/base_dataset.py:61-74).  ``lengths`` (this project's addition):
        ``{"audio": int tensor [B], "video": int tensor [B]}``, either key optional — the LSTM encoders then freeze each
        row's state at its own last step (``pack_padded_sequence`` semantics), so the embedding no longer depends on the
        padding.  A ``"text"`` key (optional, alone or with the others) gives the TextCNN each row's length: the time-max
        runs over the row's own windows, so the text embedding no longer depends on the (zero) padding either."""
        assert not all((A is None, V is None, T is None)), "At least one of A, V, T must be provided"
        assert not all([is_embd_A, is_embd_V, is_embd_T]), "Cannot have all embeddings as True"
        if A is None or V is None or T is None or is_embd_A or is_embd_V or is_embd_T:
            raise NotImplementedError("UttFusionModel HIP path: A, V and T sequences (no pre-embedded inputs)")
        A, V, T = A.float(), V.float(), T.float()
        if not (A.is_cuda and V.is_cuda and T.is_cuda):
            raise L.TspmError("UttFusionModel (tspm_amd) runs on the MI355X only; move the model and inputs to the "
                              "ROCm device (there is no CPU fallback)")
        if self.training and torch.is_grad_enabled():
            params = list(self.parameters())
            return _UttFn.apply(A, V, T, self, lengths, *params)
        eng = self._engine(A.shape[0], _batch_steps(A, V, T), A.device, *_split_lengths(lengths))
        eng.load(A, V, T)
        eng.set_lengths(lengths)
        eng.forward(L.stream_handle(), self.training)
        return eng.logits.clone()

    def train_step(self, batch: Dict[str, Any], optimizer, loss_functions, device, metric_recorder,
                   **kwargs: Any) -> Dict[str, Any]:
        """utt_fusion.py:151-200.  With FusedAdam and the single cross-entropy loss group: one FusedMosiStep
        graph (forward, loss, backward, clip_grad_norm_, Adam); otherwise the reference's own sequence
        on the HIP forward/backward (one autograd node).  Regression mode — a one-output ``netC.fc_out`` with a
        single mean L1 / MSE term: float32 labels, the fused step with the one-launch regression head (the autograd
        sequence when the head is outside the kernel's limits), and the float predictions recorded under the
        ``"regression"`` group (this package's name for it).  A batch carrying ``"all_patterns": True`` and
        ``"patterns"`` (``mosi_data.MOSI.loader(all_patterns=True)``: the samples once, unmasked) trains every row under
        every one of those patterns in one ``FusedMosiPatternStep`` and records the P*B predictions against the tiled
        targets with ``m_types`` = the expanded pattern names; that runs on the fused step only (``FusedAdam``) - no
        autograd node is built for it."""
        A = _modality(batch, "audio").to(device).float()
        V = _modality(batch, "video").to(device).float()
        T = _modality(batch, "text").to(device).float()
        labels = batch["label"].to(device)
        miss = batch.get("pattern_name")
        reg = _regress_mode(self, loss_functions)
        if reg is not None:
            labels = labels.float()
        if batch.get("all_patterns"):
            if not isinstance(optimizer, FusedAdam) or not A.is_cuda:
                raise L.TspmError("UttFusionModel.train_step: all-pattern training (an \"all_patterns\" batch) runs on "
                                  "the fused step only - FusedAdam on the ROCm device; there is no autograd node for it")
            pats = norm_patterns(batch["patterns"])
            lengths = batch.get("lengths")
            ragged, tl = _split_lengths(lengths)
            out = self.fused_pattern_step(optimizer, loss_functions, A.shape[0], _batch_steps(A, V, T), pats,
                                          ragged=ragged, text_lengths=tl).step(A, V, T, labels, lengths)
            if metric_recorder is not None:
                names = np.array([p for p in pats for _ in range(A.shape[0])])
                targets = labels.reshape(-1).detach().cpu().numpy()
                if reg is not None:
                    preds = out["logits"].detach().reshape(-1).cpu().numpy()
                else:
                    preds = torch.softmax(out["logits"].detach(), dim=-1).argmax(dim=-1).reshape(-1).cpu().numpy()
                metric_recorder.update_group_all("regression" if reg is not None else "classification",
                                                 predictions=preds, targets=np.tile(targets, len(pats)), m_types=names)
            return {"loss": float(out["loss"].item())}
        head_ok = (_ce_weight(loss_functions) is not None if reg is None
                   else L.regress_head_supported(A.shape[0], self.netC.widths[-1]))
        lengths = batch.get("lengths")  # per-sample lengths (mosi_data.MOSI(use_lengths=True)): the ragged step
        if isinstance(optimizer, FusedAdam) and head_ok and A.is_cuda:
            ragged, tl = _split_lengths(lengths)
            out = self.fused_step(optimizer, loss_functions, A.shape[0], _batch_steps(A, V, T), ragged=ragged,
                                  text_lengths=tl).step(A, V, T, labels, lengths)
            logits, loss = out["logits"], out["loss"]
        else:
            self.train()
            logits = self.forward(A, V, T, lengths=lengths)
            optimizer.zero_grad()
            loss = loss_functions(logits.squeeze(), labels.squeeze())["total_loss"]
            loss.backward()
            if self.clip is not None:
                torch.nn.utils.clip_grad_norm_(self.parameters(), self.clip)
            optimizer.step()
        if metric_recorder is not None and reg is not None:  # the float predictions under the "regression" group
            metric_recorder.update_group_all("regression", predictions=logits.detach().reshape(-1).cpu().numpy(),
                                             targets=labels.reshape(-1).detach().cpu().numpy(),
                                             m_types=np.array(miss if miss is not None else []))
        elif metric_recorder is not None:
            preds = torch.softmax(logits.detach(), dim=-1).argmax(dim=-1).squeeze()
            metric_recorder.update_group_all("classification", predictions=preds.cpu().numpy(),
                                             targets=labels.squeeze().detach().cpu().numpy(),
                                             m_types=np.array(miss if miss is not None else []))
        return {"loss": float(loss.item())}

    @torch.no_grad()
    def validation_step(self, batch: Dict[str, Any], loss_functions, device, metric_recorder,
                        return_test_info: bool = False, **kwargs: Any) -> Dict[str, Any]:
        """utt_fusion.py:202-256: eval-mode forward (no dropout) + the loss group on the HIP kernels."""
        self.eval()
        A = _modality(batch, "audio").to(device).float()
        V = _modality(batch, "video").to(device).float()
        T = _modality(batch, "text").to(device).float()
        labels = batch["label"].to(device)
        miss = np.array(batch.get("pattern_name", []))
        lengths = batch.get("lengths")
        eng = self._engine(A.shape[0], _batch_steps(A, V, T), A.device, *_split_lengths(lengths))
        reg = _regress_mode(self, loss_functions)
        if reg is not None:
            labels = labels.float()
        eng.load(A, V, T, labels, reg is not None)
        eng.set_lengths(lengths)
        sh = L.stream_handle()
        if reg is not None:
            if L.regress_head_supported(eng.B, eng.widths[-1]):
                eng.forward(sh, False, head=False)
                eng.head_regress(sh, False, *reg)
                loss = eng.loss.clone()
            else:
                eng.forward(sh, False)
                loss = loss_functions(eng.logits.squeeze(), labels.squeeze())["total_loss"]
            preds = eng.logits.reshape(-1).clone()
            if metric_recorder is not None:
                metric_recorder.update_group_all("regression", predictions=preds.cpu().numpy(),
                                                 targets=labels.reshape(-1).cpu().numpy(), m_types=miss)
            self.train()
            if return_test_info:
                return {"loss": loss.item(), "predictions": [preds.cpu().numpy()], "labels": [labels.cpu().numpy()],
                        "miss_types": [list(miss)]}
            return {"loss": loss.item()}
        eng.forward(sh, False)
        w = _ce_weight(loss_functions)
        if w is not None:
            eng.loss_fn(sh, w, False)
            loss = eng.loss.clone()
        else:
            loss = loss_functions(eng.logits.squeeze(), labels)["total_loss"]
        preds = torch.softmax(eng.logits, dim=-1).argmax(dim=-1).squeeze()
        if metric_recorder is not None:
            metric_recorder.update_group_all("classification", predictions=preds.cpu().numpy(),
                                             targets=labels.squeeze().cpu().numpy(), m_types=miss)
        self.train()
        if return_test_info:
            return {"loss": loss.item(), "predictions": [preds.cpu().numpy()], "labels": [labels.cpu().numpy()],
                    "miss_types": [list(miss)]}
        return {"loss": loss.item()}

    @torch.no_grad()
    def get_embeddings(self, dataloader, device) -> Dict[Any, List[np.ndarray]]:
        """utt_fusion.py:258-294."""
        self.eval()
        emb: Dict[Any, List[np.ndarray]] = defaultdict(list)
        for batch in dataloader:
            A = _modality(batch, "audio").to(device).float()
            V = _modality(batch, "video").to(device).float()
            T = _modality(batch, "text").to(device).float()
            lengths = batch.get("lengths")
            eng = self._engine(A.shape[0], _batch_steps(A, V, T), A.device, *_split_lengths(lengths))
            eng.load(A, V, T)
            eng.set_lengths(lengths)
            eng.forward(L.stream_handle(), False)
            ha, hv = self.netA.hidden_size, self.netV.hidden_size
            keys = [k for k in batch.keys() if str(getattr(k, "value", k)).lower().split(".")[-1] in
                    ("audio", "video", "text")]
            cols = {"audio": slice(0, ha), "video": slice(ha, ha + hv), "text": slice(ha + hv, eng.E)}
            for k in keys:
                name = str(getattr(k, "value", k)).lower().split(".")[-1]
                emb[k].append(eng.fused[:, cols[name]].cpu().numpy())
            emb["label"] += list(batch["label"])
        return emb


def _encode_lstm(enc: LSTMEncoder, x: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Standalone LSTMEncoder embedding (inference): projection GEMM + one-problem tspm_lstm_fwd (with ``lengths``,
    tspm_lstm_fwd_len)."""
    L.require_cuda_f32(x, "LSTMEncoder input")
    B, T, F = x.shape
    xt = x.transpose(0, 1).contiguous() if T > 1 else x.reshape(1, B, F).contiguous()
    out = torch.empty(B, enc.hidden_size, device=x.device, dtype=torch.float32)
    sh = L.stream_handle()
    wide = L.lstm_wide_index(((enc.embd_method, T),))
    attn = _is_attention(enc)  # always the length-taking entry points (at the padded length without ``lengths``)
    lens = None if lengths is None and not attn else _length_buffer(B, T, x.device)
    if lengths is not None:
        _set_lengths(lens, lengths.to(x.device), T, "input")
    bufs = _lstm_alloc(enc, B, T, x.device, backward=False, wide=wide)
    h_out = bufs["hout"] if attn else out
    _lstm_fwd_launch([(enc, xt, bufs, T, h_out.data_ptr(), enc.hidden_size, lens)], B, sh, wide)
    if attn:
        _attn_fwd_launch([(enc, bufs, T, out.data_ptr(), enc.hidden_size, lens)], B, sh)
    return out
