"""Input stage of the MOSI UTT-Fusion step: the corpus resident in HBM, padded batches assembled on device.

Replaces the reference's host data path for BASELINE.json configs[4]:

    DataLoader(MOSI(...), batch_size, shuffle, collate_fn=dataset.collate_fn)       config/data_config.py:270-290
      → MultimodalSentimentDataset.__getitem__: pattern (random.choice for train,
        pattern-major for valid/test), modality × missing mask                        data/mosi.py:159-196,
                                                                                       data/base_dataset.py:61-74,91-99
      → _collate_train_batch: torch.stack(labels), pad_sequence(batch_first, 0.0)
        per modality; eval batches grouped by pattern                                  data/mosi.py:198-247

Here every modality is packed once into HBM as ragged rows (``data`` [sum(len), F] f32 + per-sample
offsets and lengths), and a batch is one ``tspm_seq_gather`` launch per modality: index gather, zero
padding to the batch's longest sequence (pad_sequence), the pattern's modality mask and the labels —
written either batch-first (the reference's collate layout, for ``collate_fn``) or time-major straight
into a ``FusedMosiStep``'s input buffers (``device_loader(..., step=...)``: no copy at all).

The reference's own MOSI pickles (aligned_50.pkl) hold DENSE arrays — every sample of a split has the
same length per modality — so its pad_sequence is the identity there; ragged corpora (``lengths``) are
padded exactly as pad_sequence pads them.  Known reference defect, not reproduced: _collate_train_batch
reads ``b[""]`` (data/mosi.py:216), a key no sample has, so the reference's own collate raises KeyError;
this collate returns the batch the rest of that function builds.

Pattern semantics follow the MOSI configs (configs/mosi/centralised/utt_fusion_base_training.yaml:72-139:
every modality named in the pattern has missing_rate 0.0, the others are absent), i.e. modality m is
kept iff its letter is in the pattern.  Training patterns are drawn per sample from a seeded torch
generator (the reference uses Python's ``random.choice`` per ``__getitem__``: same distribution, a
different stream).
"""
from __future__ import annotations

import os
import pickle
from typing import Any, Dict, Iterator, List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L

MODALITIES = ("audio", "video", "text")
_PICKLE_KEYS = {"audio": "audio", "video": "vision", "text": "text"}  # data/mosi.py:135-138
PATTERNS = ["atv", "at", "av", "tv", "a", "t", "v"]  # data/mosi.py:61-69 order
LENGTH_MODALITIES = ("audio", "video")  # what use_lengths covers (the LSTM encoders); "text" joins with text_lengths


def pad_of(pad_to, modality: str) -> int:
    """The minimum padded length of one modality: ``pad_to`` is an ``int`` (every modality), a dict by modality name
    (a missing name: no minimum) or a triple in ``MODALITIES`` order (audio, video, text)."""
    if isinstance(pad_to, dict):
        return int(pad_to.get(modality, 0))
    if isinstance(pad_to, (tuple, list)):
        if len(pad_to) != len(MODALITIES):
            raise L.TspmError(f"pad_to: an int, a dict by modality or a triple (audio, video, text), got {pad_to!r}")
        return int(pad_to[MODALITIES.index(modality)])
    return int(pad_to)


def steps_of(steps, modality: str) -> int:
    """One modality's length of a batch's ``steps``: the ``int`` common length or the (audio, video, text) triple."""
    return int(steps) if not isinstance(steps, (tuple, list)) else int(steps[MODALITIES.index(modality)])


def pattern_keep(pattern: str) -> Dict[str, float]:
    """1.0 for every modality whose first letter is in ``pattern`` (configs/mosi/*: missing_rate 0.0)."""
    return {m: 1.0 if m[0] in pattern else 0.0 for m in MODALITIES}


class MosiCorpus:
    """One split: per modality ragged rows packed as [sum(lengths), F] float32 + offsets + lengths; labels."""

    def __init__(self, seqs: Dict[str, Sequence[np.ndarray]], labels: np.ndarray):
        self.labels = np.ascontiguousarray(np.asarray(labels))
        n = self.labels.shape[0]
        self.data, self.offsets, self.lengths, self.feat = {}, {}, {}, {}
        for m in MODALITIES:
            rows = seqs[m]
            if len(rows) != n:
                raise ValueError(f"{m}: {len(rows)} sequences for {n} labels")
            lens = np.array([np.asarray(r).shape[0] for r in rows], dtype=np.int32)
            feat = int(np.asarray(rows[0]).shape[-1])
            self.data[m] = np.ascontiguousarray(np.concatenate([np.asarray(r, np.float32).reshape(-1, feat)
                                                                for r in rows]) if n else np.zeros((0, feat), np.float32))
            self.offsets[m] = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if n else np.zeros(0, np.int64)
            self.lengths[m] = lens
            self.feat[m] = feat

    def __len__(self) -> int:
        return int(self.labels.shape[0])

    @classmethod
    def from_split(cls, split_data: Dict[str, Any], labels_key: str = "classification_labels",
                   lengths: Optional[Dict[str, np.ndarray]] = None) -> "MosiCorpus":
        """The reference pickle's split dict (``audio``/``vision``/``text`` dense [N, T, F] arrays and the
        labels; data/mosi.py:134-152).  ``lengths`` optionally trims each sample to its true length."""
        seqs = {}
        for m in MODALITIES:
            arr = np.asarray(split_data[_PICKLE_KEYS[m]], dtype=np.float32)
            if lengths is not None and m in lengths:
                seqs[m] = [arr[i, :int(lengths[m][i])] for i in range(arr.shape[0])]
            else:
                seqs[m] = list(arr)
        lab = np.asarray(split_data[labels_key])
        lab = lab.astype(np.float32 if "regression" in labels_key else np.int64).reshape(lab.shape[0], -1)
        return cls(seqs, lab[:, 0] if lab.shape[1] == 1 else lab)


def synthetic_mosi_corpus(n: int, seed: int = 1234, steps: int = 50, min_len: Optional[int] = None,
                          feats=(5, 20, 768), regression: bool = False) -> MosiCorpus:
    """MOSI-shaped synthetic split: audio 5-d, video 20-d, text 768-d, 3 classes.  ``min_len``: ragged
    lengths uniform in [min_len, steps] (shared by the three modalities, as in the aligned data); None:
    dense ``steps``-long sequences (aligned_50).  ``regression``: float32 sentiment scores on the 0.2 grid of
    [-3, 3] (zeros included) in place of the class labels."""
    g = np.random.default_rng(seed)
    lens = np.full(n, steps, np.int32) if min_len is None else g.integers(min_len, steps + 1, n).astype(np.int32)
    seqs = {m: [g.standard_normal((int(l), f), dtype=np.float32) for l in lens] for m, f in zip(MODALITIES, feats)}
    if regression:
        return MosiCorpus(seqs, (g.integers(-15, 16, n) / 5.0).astype(np.float32))
    return MosiCorpus(seqs, g.integers(0, 3, n).astype(np.int64))


class DeviceMosiCorpus:
    """The packed corpus in HBM; ``gather`` = one tspm_seq_gather per modality."""

    def __init__(self, corpus: MosiCorpus, device: torch.device):
        self.n = len(corpus)
        self.device = device
        self.feat = dict(corpus.feat)
        self.host_lengths = {m: corpus.lengths[m] for m in MODALITIES}
        self.data = {m: torch.from_numpy(corpus.data[m]).to(device) for m in MODALITIES}
        self.offsets = {m: torch.from_numpy(corpus.offsets[m]).to(device) for m in MODALITIES}
        self.lengths = {m: torch.from_numpy(corpus.lengths[m]).to(device) for m in MODALITIES}
        lab = np.ascontiguousarray(corpus.labels)
        # float32 [n] / [n, 1]: the continuous sentiment score (regression_labels), gathered one float per row
        self.float_labels = lab.dtype == np.float32 and (lab.ndim == 1 or (lab.ndim == 2 and lab.shape[1] == 1))
        if self.float_labels:
            lab = lab.reshape(-1, 1)
        elif lab.dtype != np.int64:
            raise L.TspmError("device gather carries int64 class labels (classification_labels) or float32 scores "
                              "[n] / [n, 1] (regression_labels)")
        self.labels = torch.from_numpy(lab).to(device)
        self.label_dtype = torch.float32 if self.float_labels else torch.int64

    def steps_for(self, index_host: np.ndarray, pad_to: int = 0, modalities: Sequence[str] = MODALITIES) -> int:
        """pad_sequence's padded length, the longest sequence of the batch — per modality in the reference
        (data/mosi.py:225-230); the HIP step runs the three modalities over one common length, so the
        per-modality maxima must agree (aligned data) or all be covered by ``pad_to``."""
        if not len(index_host):
            return pad_to
        mx = [int(self.host_lengths[m][index_host].max()) for m in modalities]
        if max(mx) > pad_to and len(set(mx)) > 1:
            raise L.TspmError(f"unaligned batch: per-modality longest sequences {dict(zip(modalities, mx))} differ "
                              "(pad_sequence pads each to its own length); pass pad_to >= all of them")
        return max(max(mx), pad_to)

    def steps_per_modality(self, index_host: np.ndarray, pad_to=0, modalities: Sequence[str] = MODALITIES):
        """pad_sequence's padded length of each modality on its own (data/mosi.py:225-230): the batch's longest
        sequence of that modality, at least that modality's ``pad_to`` (``pad_of``: an int, a dict or a triple) — a
        tuple in the order of ``modalities``, (Ta, Tv, Tt) by default, the per-modality ``steps`` of the HIP step."""
        if not len(index_host):
            return tuple(pad_of(pad_to, m) for m in modalities)
        return tuple(max(int(self.host_lengths[m][index_host].max()), pad_of(pad_to, m)) for m in modalities)

    def batch_steps(self, index_host: np.ndarray, pad_to=0, modalities: Sequence[str] = MODALITIES):
        """The ``steps`` of a batch: the common length (an ``int``) whenever ``steps_for`` accepts the batch — aligned
        data, or an ``int`` ``pad_to`` that covers every modality — else the per-modality tuple of
        ``steps_per_modality`` (an unaligned batch; an ``int`` again if its entries agree)."""
        if isinstance(pad_to, (int, np.integer)):
            mx = [int(self.host_lengths[m][index_host].max()) for m in modalities] if len(index_host) else [0]
            if not (max(mx) > pad_to and len(set(mx)) > 1):
                return self.steps_for(index_host, int(pad_to), modalities)
        per = self.steps_per_modality(index_host, pad_to, modalities)
        return per[0] if len(set(per)) == 1 else per

    def gather(self, index: torch.Tensor, steps_pad, out: Dict[str, torch.Tensor], time_major: bool,
               masks: Optional[Dict[str, torch.Tensor]] = None, labels_out: Optional[torch.Tensor] = None,
               lengths_out: Optional[Dict[str, torch.Tensor]] = None, rows: Optional[int] = None) -> None:
        """Write the batch ``index`` (device int64) into ``out[m]``: [T, B, F] (time_major) or [B, T, F], for
        the modalities ``out`` names (all three for the fusion step, one for encoder pre-training); int64 labels
        ride on the first launch, float32 labels (``labels_out`` float32 [B]) take one ``tspm_avmnist_gather``
        launch of one float per row (an out-of-range index gives a NaN label).  ``steps_pad``: the common padded
        length, or the (audio, video, text) triple of an unaligned batch — each modality's launch pads to its own.
        ``lengths_out``: ``{modality: int32 [B]}`` device buffers filled with the batch's true lengths
        (``self.lengths[m][index]``, on the device, no host sync) — a ragged step's length buffers, or a batch's
        ``"lengths"``.  ``rows`` (time-major only): ``out[m]`` holds that many rows per step, at least the batch's; the
        batch goes to the first ``len(index)`` of them and the others are not written (a fused-pattern step's 2B-row
        inputs)."""
        lib, sh = L.lib(), L.stream_handle()
        b = int(index.numel())
        nrows = b if rows is None else int(rows)
        if nrows < b or (rows is not None and not time_major):
            raise L.TspmError(f"rows={rows}: a time-major output of at least {b} rows per step")
        for m, buf in (lengths_out or {}).items():
            if buf.dtype != torch.int32 or tuple(buf.shape) != (b,):
                raise L.TspmError(f"lengths_out[{m!r}]: an int32 [{b}] device buffer")
            torch.index_select(self.lengths[m], 0, index, out=buf)
        if labels_out is not None and labels_out.dtype != self.label_dtype:
            raise L.TspmError(f"labels_out is {labels_out.dtype}, the corpus carries {self.label_dtype} labels")
        if self.float_labels and labels_out is not None:
            L.check(lib.tspm_avmnist_gather(b, index.data_ptr(), self.n, self.labels.data_ptr(), 1, None, 0, None, None,
                                            None, None, labels_out.data_ptr(), None, None, sh), "label gather")
            labels_out = None
        for j, m in enumerate([m for m in MODALITIES if m in out]):
            f, dst, tp = self.feat[m], out[m], steps_of(steps_pad, m)
            shape = (tp, nrows, f) if time_major else (b, tp, f)
            if tuple(dst.shape) != shape or not dst.is_contiguous() or dst.dtype != torch.float32:
                raise L.TspmError(f"{m}: output {tuple(dst.shape)} != {shape} (contiguous f32)")
            st_t, st_b = (nrows * f, f) if time_major else (f, tp * f)
            mk = masks.get(m) if masks else None
            L.check(lib.tspm_seq_gather(b, index.data_ptr(), self.n, self.data[m].data_ptr(), self.offsets[m].data_ptr(),
                                        self.lengths[m].data_ptr(), f, tp, dst.data_ptr(), st_t, st_b,
                                        None if mk is None else mk.data_ptr(),
                                        self.labels.data_ptr() if (j == 0 and not self.float_labels) else None,
                                        labels_out.data_ptr() if (j == 0 and labels_out is not None) else None, sh),
                    "seq_gather")


class MOSI(torch.utils.data.Dataset):
    """data/mosi.py:17-301 (MultimodalSentimentDataset / MOSI) drop-in over a device-resident corpus."""

    VALID_SPLITS = ["train", "valid", "test"]
    NUM_CLASSES = 3
    AVAILABLE_MODALITIES = {m: m for m in MODALITIES}

    def __init__(self, data_fp=None, split: str = "train", target_modality: Any = "multimodal", *,
                 missing_patterns=None, selected_patterns: Optional[List[str]] = None,
                 labels_key: str = "classification_labels", aligned: bool = False, length: Optional[int] = None,
                 num_classes: Optional[int] = None, batch_size: int = 1, corpus: Optional[MosiCorpus] = None,
                 device=None, seed: int = 0, allow_pickle: bool = False, use_lengths: bool = False,
                 text_lengths: bool = False) -> None:
        split = split.lower()
        if split not in self.VALID_SPLITS:
            raise AssertionError(f"Invalid split provided, must be one of {self.VALID_SPLITS}")
        self.split, self.labels_key, self.aligned = split, labels_key, aligned
        self.length = length if aligned else None
        if num_classes is not None:
            self.NUM_CLASSES = num_classes
        tm = str(getattr(target_modality, "value", target_modality)).lower().split(".")[-1]
        if tm not in MODALITIES + ("multimodal",):
            raise AssertionError(f"Invalid modality provided, must be one of {list(MODALITIES) + ['multimodal']}")
        # "audio" / "video" / "text": encoder pre-training (train_monomodal) — only that modality is gathered and
        # present in the batch, and batches are flat (the monomodal loop has no per-pattern sub-batches)
        self.target_modality = tm
        self.selected_patterns = list(selected_patterns) if selected_patterns is not None else list(PATTERNS)
        bad = set(self.selected_patterns) - set(PATTERNS)
        if bad:
            raise ValueError(f"Invalid patterns: {bad}")
        self.missing_patterns = missing_patterns
        self._batch_size = batch_size
        self.allow_pickle = allow_pickle
        # use_lengths: batches carry each sample's true audio / video length (``"lengths"``, or written into a ragged
        # step's length buffers) and an unaligned file is trimmed to its audio_lengths / vision_lengths; the LSTM
        # encoders then stop at each sample's own last frame.  text_lengths (with use_lengths): the batches carry the
        # text lengths too (``"lengths"["text"]``, or written into a text_lengths step's buffer) and the TextCNN pools
        # over each sample's own windows; padding rows are zero either way.
        self.use_lengths = bool(use_lengths)
        self.text_lengths = bool(text_lengths)
        if self.text_lengths and not self.use_lengths:
            raise L.TspmError("MOSI: text_lengths=True goes with use_lengths=True")
        if corpus is None:
            corpus = self._load(data_fp)
        self.corpus = corpus
        self.num_samples = len(corpus)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._dev: Optional[DeviceMosiCorpus] = None
        self._gen = torch.Generator().manual_seed(seed)
        self._keep = torch.tensor([[pattern_keep(p)[m] for m in MODALITIES] for p in PATTERNS], dtype=torch.float32)

    def _load(self, data_fp) -> MosiCorpus:
        """An .npz of the reference's split keys (``<split>/audio``, ``<split>/vision``, ...; read with
        allow_pickle=False), or — only with ``allow_pickle=True``, for a data file the user trusts — the
        reference's own split pickle (data/mosi.py:122-152: {"train"/"valid"/"test": {...}}), which
        executes code when loaded."""
        if data_fp is None:
            raise ValueError("MOSI: data_fp or corpus is required")
        path = os.fspath(data_fp)
        if not os.path.exists(path):
            raise FileNotFoundError(f"Data file not found: {path}")
        if path.endswith(".npz"):
            with np.load(path, allow_pickle=False) as z:
                split = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(self.split + "/")}
        else:
            if not self.allow_pickle:
                raise ValueError(f"{path}: pickled dataset files run code when loaded; convert it to .npz or pass "
                                 "allow_pickle=True for a file you trust")
            with open(path, "rb") as f:
                raw = pickle.load(f)  # noqa: S301 (explicit opt-in; data/mosi.py:125-126)
            if self.split not in raw:
                raise KeyError(f"Split '{self.split}' not found in data")
            split = raw[self.split]
        if self.labels_key not in split:
            raise KeyError(f"Labels key '{self.labels_key}' not found in data")
        # The reference keeps the dense [N, T, F] arrays even for unaligned files and never trims them to
        # audio_lengths / vision_lengths (data/mosi.py:134-152: lengths are metadata only); so here.
        # With ``use_lengths`` the corpus is trimmed to them instead (this project's addition).
        true_lengths = None
        if not self.aligned and "audio_lengths" in split:
            true_lengths = {"audio": np.asarray(split["audio_lengths"]).astype(np.int64),
                            "video": np.asarray(split["vision_lengths"]).astype(np.int64)}
        corpus = MosiCorpus.from_split(split, self.labels_key, true_lengths if self.use_lengths else None)
        if true_lengths is not None:
            corpus.true_lengths = true_lengths
        return corpus

    # -- reference Dataset API ----------------------------------------------------------------------
    def __len__(self) -> int:
        return self.num_samples if self.split == "train" else self.num_samples * len(self.selected_patterns)

    @property
    def device_corpus(self) -> DeviceMosiCorpus:
        if self._dev is None:
            self._dev = DeviceMosiCorpus(self.corpus, self.device)
        return self._dev

    def _resolve(self, items: Sequence[int]):
        items = np.asarray(items, dtype=np.int64)
        if self.split == "train":
            pid = torch.randint(len(self.selected_patterns), (len(items),), generator=self._gen).numpy()
            return items, pid
        return items % self.num_samples, items // self.num_samples

    def __getitems__(self, items: Sequence[int]):
        return [("__tspm_batch__", np.asarray(items, dtype=np.int64))]

    def __getitem__(self, idx: int):
        return ("__tspm_batch__", np.asarray([idx], dtype=np.int64))

    def collate_fn(self, batch) -> Dict[str, Any]:
        """data/mosi.py:198-247 on the device: padded batch-first tensors [B, T_max, F] per modality (one
        tspm_seq_gather each), labels, pattern names; valid/test batches grouped by pattern."""
        items = np.concatenate([b[1] for b in batch])
        rows, pid = self._resolve(items)
        if self.split == "train" or self.target_modality != "multimodal":
            return self._collate(rows, pid)
        out = {}
        for p in dict.fromkeys(pid.tolist()):
            sel = pid == p
            out[self.selected_patterns[p]] = self._collate(rows[sel], pid[sel])
        return out

    def _masks(self, pid: np.ndarray) -> Dict[str, torch.Tensor]:
        """Per-row keep factors of the modalities some row of the batch drops (None = all kept)."""
        k = self._keep[[PATTERNS.index(self.selected_patterns[p]) for p in pid]]
        return {m: k[:, j].contiguous().to(self.device, non_blocking=True)
                for j, m in enumerate(MODALITIES) if not bool((k[:, j] == 1.0).all())}

    def _length_modalities(self) -> Sequence[str]:
        """The modalities whose lengths a batch carries: none, the LSTM encoders', or with ``text_lengths`` all three."""
        if not self.use_lengths:
            return ()
        return LENGTH_MODALITIES + (("text",) if self.text_lengths else ())

    def _want(self) -> Sequence[str]:
        """The modalities a batch carries (data.AVMNIST._want's rule)."""
        return MODALITIES if self.target_modality == "multimodal" else (self.target_modality,)

    def _collate_mono(self, rows: np.ndarray, pid: np.ndarray, step=None, pad_to: int = 0) -> Dict[str, Any]:
        """A pre-training batch: the target modality's key, ``label`` and ``pattern_name`` only (the last
        non-bookkeeping key is the modality, monomodal.select_modality_key).  With ``step`` (a monomodal
        FusedMosiMonoStep / FusedMosiMonoEvalStep) the gather writes time-major straight into its input buffer."""
        dc, m = self.device_corpus, self.target_modality
        b, tpad = len(rows), dc.steps_for(rows, pad_of(pad_to, m), (m,))
        index = torch.from_numpy(rows).to(self.device, non_blocking=True)
        masks = {k: v for k, v in self._masks(pid).items() if k == m}
        names = [self.selected_patterns[p] for p in pid]
        ragged = m in self._length_modalities()
        if step is not None:
            if (step.N, step.T) != (b, tpad):
                raise L.TspmError(f"step planned for (B={step.N}, T={step.T}), batch is (B={b}, T={tpad})")
            lab = step.labels_f if dc.float_labels else step.labels
            lens = None
            if ragged:
                lens = getattr(step.eng, "text_lens" if m == "text" else "lens", None)
                if lens is None:
                    raise L.TspmError("use_lengths: the step was built without ragged=True (text: text_lengths=True) "
                                      "(no length buffer)")
            dc.gather(index, tpad, {m: step.X}, True, masks, lab, {m: lens} if ragged else None)
            return {m: step.X, "label": lab, "pattern_name": names, **({"lengths": lens} if ragged else {})}
        out = torch.empty(b, tpad, dc.feat[m], device=self.device)
        lab = torch.empty(b, dtype=dc.label_dtype, device=self.device)
        lens = torch.empty(b, dtype=torch.int32, device=self.device) if ragged else None
        dc.gather(index, tpad, {m: out}, False, masks, lab, {m: lens} if ragged else None)
        return {m: out, "label": lab, "pattern_name": names, **({"lengths": lens} if ragged else {})}

    def _length_buffers_of(self, e) -> Optional[Dict[str, torch.Tensor]]:
        """The length buffers of a step's engine that this dataset's batches fill (None without ``use_lengths``)."""
        if not self.use_lengths:
            return None
        if getattr(e, "lens", None) is None:
            raise L.TspmError("use_lengths: the step was built without ragged=True (no length buffers)")
        lens = {"audio": e.lens["a"], "video": e.lens["v"]}
        if self.text_lengths:
            if getattr(e, "text_lens", None) is None:
                raise L.TspmError("text_lengths: the step was built without text_lengths=True (no text length buffer)")
            lens["text"] = e.text_lens
        return lens

    def _collate(self, rows: np.ndarray, pid: np.ndarray, step=None, pad_to: int = 0) -> Dict[str, Any]:
        if self.target_modality != "multimodal":
            return self._collate_mono(rows, pid, step, pad_to)
        dc = self.device_corpus
        b, tpad = len(rows), dc.batch_steps(rows, pad_to)  # an int, or (Ta, Tv, Tt) for an unaligned batch
        index = torch.from_numpy(rows).to(self.device, non_blocking=True)
        masks = self._masks(pid)
        names = [self.selected_patterns[p] for p in pid]
        if step is not None:
            e = step.eng
            if (e.B, e.T) != (b, tpad):
                raise L.TspmError(f"step planned for (B={e.B}, T={e.T}), batch is (B={b}, T={tpad})")
            lab = e.labels_f if dc.float_labels else e.labels
            lens = self._length_buffers_of(e)
            dc.gather(index, tpad, {"audio": e.A, "video": e.V, "text": e.X}, True, masks, lab, lens)
            return {"audio": e.A, "video": e.V, "text": e.X, "label": lab, "pattern_name": names,
                    "steps": tpad, "time_major": True, **({"lengths": lens} if lens is not None else {})}
        out = {m: torch.empty(b, steps_of(tpad, m), dc.feat[m], device=self.device) for m in MODALITIES}
        lab = torch.empty(b, dtype=dc.label_dtype, device=self.device)
        lens = ({m: torch.empty(b, dtype=torch.int32, device=self.device) for m in self._length_modalities()}
                if self.use_lengths else None)
        dc.gather(index, tpad, out, False, masks, lab, lens)
        return {"audio": out["audio"], "video": out["video"], "text": out["text"], "label": lab,
                "pattern_name": names, "pattern_names": names, "steps": tpad,
                **({"lengths": lens} if lens is not None else {})}

    def _check_fuse_patterns(self) -> None:
        if self.split == "train" or self.target_modality != "multimodal":
            raise L.TspmError(f"fuse_patterns=True is for the multimodal valid / test splits (every sample under every "
                              f"selected pattern); this dataset is split {self.split!r}, target_modality "
                              f"{self.target_modality!r}")

    def _check_all_patterns(self, fuse_patterns: bool = False) -> None:
        if self.split != "train" or self.target_modality != "multimodal" or fuse_patterns:
            raise L.TspmError(f"all_patterns=True is for the multimodal train split (every sample trained under every "
                              f"selected pattern in one step) and excludes fuse_patterns, the valid / test form; this "
                              f"dataset is split {self.split!r}, target_modality {self.target_modality!r}, "
                              f"fuse_patterns={bool(fuse_patterns)}")

    def _collate_fused(self, rows: np.ndarray, step=None, pad_to: int = 0) -> Dict[str, Any]:
        """A fused-pattern batch: the samples once, unmasked, with ``"patterns"`` (the selected patterns, which the step
        expands on the device) and ``"fused_patterns": True`` in place of ``pattern_name``.  With ``step`` (a
        ``FusedMosiPatternEvalStep``) the gather writes rows [0, B) of its 2B-row time-major inputs, its label buffer
        and the first halves of its length buffers."""
        return self._collate_unmasked(rows, step, pad_to, "fused_patterns")

    def _collate_all(self, rows: np.ndarray, step=None, pad_to: int = 0) -> Dict[str, Any]:
        """A train ``all_patterns`` batch: ``_collate_fused``'s batch with ``"all_patterns": True`` in place of
        ``"fused_patterns"``; ``step`` is a ``FusedMosiPatternStep`` (the same 2B-row inputs and buffers)."""
        return self._collate_unmasked(rows, step, pad_to, "all_patterns")

    def _collate_unmasked(self, rows: np.ndarray, step, pad_to, flag: str) -> Dict[str, Any]:
        dc = self.device_corpus
        b, tpad = len(rows), dc.batch_steps(rows, pad_to)
        index = torch.from_numpy(rows).to(self.device, non_blocking=True)
        extra = {"patterns": list(self.selected_patterns), flag: True, "steps": tpad}
        if step is not None:
            e = step.eng
            if (e.B, e.T) != (b, tpad) or list(e.patterns) != list(self.selected_patterns):
                raise L.TspmError(f"step planned for (B={e.B}, T={e.T}, patterns={list(e.patterns)}), batch is (B={b}, "
                                  f"T={tpad}, patterns={self.selected_patterns})")
            lab = e.labels_f if dc.float_labels else e.labels
            lens = self._length_buffers_of(e)
            dc.gather(index, tpad, {"audio": e.A, "video": e.V, "text": e.X}, True, None, lab, lens, rows=2 * b)
            return {"audio": e.A, "video": e.V, "text": e.X, "label": lab, "time_major": True, **extra,
                    **({"lengths": lens} if lens is not None else {})}
        out = {m: torch.empty(b, steps_of(tpad, m), dc.feat[m], device=self.device) for m in MODALITIES}
        lab = torch.empty(b, dtype=dc.label_dtype, device=self.device)
        lens = ({m: torch.empty(b, dtype=torch.int32, device=self.device) for m in self._length_modalities()}
                if self.use_lengths else None)
        dc.gather(index, tpad, out, False, None, lab, lens)
        return {"audio": out["audio"], "video": out["video"], "text": out["text"], "label": lab, **extra,
                **({"lengths": lens} if lens is not None else {})}

    def device_loader(self, batch_size: int, shuffle: bool = False, drop_last: bool = False,
                      generator: Optional[torch.Generator] = None, step_for=None,
                      pad_to: int = 0, group_patterns: Optional[bool] = None,
                      fuse_patterns: bool = False, all_patterns: bool = False,
                      ids_only: bool = False) -> Iterator[Dict[str, Any]]:
        """One epoch of batches gathered on device.  ``step_for(B, T) -> FusedMosiStep`` (or
        ``FusedMosiEvalStep``): gather each batch time-major straight into that step's input buffers.
        ``pad_to``: pad every batch to at least this many steps (the aligned length, e.g. 50 for aligned_50:
        one captured step shape for the whole epoch; pad_sequence pads to the batch maximum, which equals it
        on the reference's dense data) — an ``int``, or per modality a dict / (audio, video, text) triple.  A batch
        whose modalities differ in length (unaligned data) is padded per modality as pad_sequence pads it:
        ``step_for`` then receives the triple (Ta, Tv, Tt), the batch's ``"steps"`` is that triple, and a per-modality
        ``pad_to`` that covers the corpus gives one step shape, hence one graph, for the epoch.
        ``group_patterns`` (default: valid / test splits, as collate_fn):
        each batch is ``{pattern: sub-batch}`` in first-seen order (data/mosi.py:236-251); with a single target
        modality the default is flat batches (``step_for`` then returns the monomodal train / eval step).
        ``fuse_patterns`` (multimodal valid / test splits only): each sample is yielded ONCE, unmasked, in sample order,
        in batches that carry ``"patterns": list(selected_patterns)`` and ``"fused_patterns": True`` and no
        ``pattern_name`` — ``step_for(B, T)`` then returns a ``FusedMosiPatternEvalStep``, which evaluates every
        pattern of the batch from one encoder pass.
        ``all_patterns`` (the multimodal train split only; not with ``fuse_patterns``): the train form of the same — each
        sample ONCE per epoch, unmasked, in the loader's usual (shuffled) order, in batches that carry ``"patterns"`` and
        ``"all_patterns": True`` and neither ``pattern_name`` nor ``fused_patterns``; ``step_for(B, T)`` then returns a
        ``FusedMosiPatternStep``, which trains every pattern of the batch in one step.
        ``ids_only`` (the multimodal target only; for the steps that read an :meth:`embedding_cache`): the same order,
        the same RNG draws and the same number of batches, but no input tensor is gathered and ``step_for`` is not used
        — every batch carries ``"ids_only": True``, ``"rows"`` (int64 [b] sample indices on the device), ``"steps"``
        (the split's corpus-wide padded lengths under ``pad_to``: the cache's), ``"dataset"`` and ``"pad_to"``; an
        ``all_patterns`` / ``fuse_patterns`` batch adds ``"patterns"`` and its flag as above, a plain train batch
        ``"row_keep"`` (uint8 [b][3] on the device: each row's (audio, video, text) keep flags) and ``"pattern_name"``,
        and a grouped valid / test batch is ``{pattern: such a sub-batch}``."""
        if ids_only:
            self._check_ids_only()
        if all_patterns:
            self._check_all_patterns(fuse_patterns)
        if fuse_patterns or all_patterns:
            if fuse_patterns:
                self._check_fuse_patterns()
            ns = self.num_samples
            order = torch.randperm(ns, generator=generator).numpy() if shuffle else np.arange(ns)
            for s in range(0, ns, batch_size):
                rows = order[s:s + batch_size].astype(np.int64)
                if drop_last and len(rows) < batch_size:
                    break
                if ids_only:
                    yield {**self._collate_ids(rows, None, pad_to), "patterns": list(self.selected_patterns),
                           ("all_patterns" if all_patterns else "fused_patterns"): True}
                    continue
                step = step_for(len(rows), self.device_corpus.batch_steps(rows, pad_to)) if step_for is not None else None
                yield (self._collate_all if all_patterns else self._collate_fused)(rows, step, pad_to)
            return
        n = len(self)
        grouped = ((self.split != "train" and self.target_modality == "multimodal") if group_patterns is None
                   else bool(group_patterns))
        order = torch.randperm(n, generator=generator).numpy() if shuffle else np.arange(n)
        for s in range(0, n, batch_size):
            items = order[s:s + batch_size]
            if drop_last and len(items) < batch_size:
                break
            rows, pid = self._resolve(items)
            parts = ([(self.selected_patterns[p], pid == p) for p in dict.fromkeys(pid.tolist())] if grouped
                     else [(None, slice(None))])
            out = {}
            for name, sel in parts:
                r, q = rows[sel], pid[sel]
                if ids_only:
                    out[name] = self._collate_ids(r, q, pad_to)
                elif step_for is not None:
                    want = self._want()
                    t = (self.device_corpus.batch_steps(r, pad_to) if len(want) > 1
                         else self.device_corpus.steps_for(r, pad_of(pad_to, want[0]), want))
                    out[name] = self._collate(r, q, step_for(len(r), t), pad_to)
                    if grouped:
                        yield {name: out[name]}  # the step's buffers are reused: hand each group over at once
                        out = {}
                else:
                    out[name] = self._collate(r, q, None, pad_to)
            if out:
                yield out if grouped else out[None]

    def loader(self, batch_size: int, shuffle: bool = False, drop_last: bool = False, seed: Optional[int] = None,
               step_for=None, pad_to: int = 0, group_patterns: Optional[bool] = None,
               fuse_patterns: bool = False, all_patterns: bool = False, ids_only: bool = False) -> "MosiDeviceLoader":
        """A re-iterable epoch loader (one ``device_loader`` pass per ``iter``), as a DataLoader is.  ``fuse_patterns`` /
        ``all_patterns`` / ``ids_only``: see ``device_loader`` (refused here already for a dataset they are not for)."""
        if ids_only:
            self._check_ids_only()
        if all_patterns:
            self._check_all_patterns(fuse_patterns)
        if fuse_patterns:
            self._check_fuse_patterns()
        return MosiDeviceLoader(self, batch_size, shuffle, drop_last, seed, step_for, pad_to, group_patterns,
                                fuse_patterns, all_patterns, ids_only)

    # -- the frozen encoders' outputs of this split, computed once ---------------------------------------
    def _check_ids_only(self, what: str = "ids_only=True") -> None:
        if self.target_modality != "multimodal":
            raise L.TspmError(f"{what} is for the multimodal target (the cache holds all three encoders' outputs); this "
                              f"dataset's target_modality is {self.target_modality!r}")

    def corpus_steps(self, pad_to=0):
        """The split's corpus-wide padded lengths under ``pad_to`` — ``batch_steps`` of every sample at once: the
        ``steps`` an :meth:`embedding_cache` is built for and an ``ids_only`` batch carries.  A constant of (corpus,
        ``pad_to``), computed once per ``pad_to``: every ``ids_only`` batch asks for it."""
        from .mosi import norm_steps
        memo = self.__dict__.setdefault("_corpus_steps", {})
        key = repr(pad_to)
        if key not in memo:
            memo[key] = norm_steps(self.device_corpus.batch_steps(np.arange(self.num_samples), pad_to))
        return memo[key]

    def _collate_ids(self, rows: np.ndarray, pid: Optional[np.ndarray], pad_to) -> Dict[str, Any]:
        """An ``ids_only`` batch: the sample indices on the device and, with ``pid`` (one pattern per row), the rows'
        keep flags and pattern names.  Nothing is gathered."""
        out = {"ids_only": True, "rows": torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(self.device),
               "steps": self.corpus_steps(pad_to), "dataset": self, "pad_to": pad_to}
        if pid is not None:
            k = self._keep[[PATTERNS.index(self.selected_patterns[p]) for p in pid]]
            out["row_keep"] = (k != 0).to(torch.uint8).contiguous().to(self.device)
            out["pattern_name"] = [self.selected_patterns[p] for p in pid]
        return out

    def embedding_cache(self, model, pad_to=0, chunk: Optional[int] = None, refresh: bool = False):
        """This split's ``mosi.UttEmbeddingCache`` for ``model`` — one per (model, steps), built on first call: the
        three FROZEN encoders' outputs of every sample (the LSTM embeddings and the TextCNN's pooled features before its
        dropout) and of the zeroed inputs, for ``steps`` = :meth:`corpus_steps` of ``pad_to`` (without ``use_lengths``
        an embedding depends on the padded length, so the cache is that of the uncached loader under a ``pad_to`` that
        covers the corpus).  The fill runs the encoders once over the device corpus in sample order, in chunks of
        ``chunk`` rows (128 for a new cache; an existing cache keeps its own unless one is given); ``refresh=True``
        fills an existing cache again.  Refused unless all three encoders are frozen, and for a single-modality
        target.  A cache made stale (a ``requires_grad`` flag, ``load_state_dict``, ``.to()``) is returned as it is and
        refused by the step that reads it until ``refresh()``; weights written through raw pointers cannot be detected,
        so whoever changes frozen weights that way refreshes."""
        import weakref
        from .mosi import UttEmbeddingCache
        self._check_ids_only("embedding_cache")
        steps = self.corpus_steps(pad_to)
        caches = self.__dict__.setdefault("_emb_caches", weakref.WeakKeyDictionary())  # gone with their models
        table = caches.setdefault(model, {})
        c = table.get(steps)
        if c is None:
            c = table[steps] = UttEmbeddingCache(model, self, steps, 128 if chunk is None else chunk)
        else:
            if chunk is not None:
                c.chunk = int(chunk)
            if refresh:
                c.refresh()
        return c

    def get_split(self) -> str:
        return self.split

    def get_selected_patterns(self) -> List[str]:
        return self.selected_patterns

    def get_missing_patterns(self):
        return self.missing_patterns

    @staticmethod
    def get_num_classes(is_classification: bool = True) -> int:
        return 3 if is_classification else 1


class MOSEI(MOSI):
    """data/mosi.py:270-283 (CMU-MOSEI: the same MultimodalSentimentDataset, 3 classes) — the dataset of
    configs/mosei/centralised/utt_fusion_train_mosei.yaml (74-d audio, 35-d video, 768-d text)."""


class MosiDeviceLoader:
    """Re-iterable wrapper of ``MOSI.device_loader`` (a DataLoader is iterated once per epoch): epoch e draws
    its shuffle from ``torch.Generator().manual_seed(seed + e)``; ``step_for`` may be replaced before an epoch
    (the harness points it at its own train / eval steps)."""

    def __init__(self, ds: MOSI, batch_size: int, shuffle: bool, drop_last: bool, seed: Optional[int], step_for,
                 pad_to: int, group_patterns: Optional[bool], fuse_patterns: bool = False, all_patterns: bool = False,
                 ids_only: bool = False):
        self.ds, self.batch_size, self.shuffle, self.drop_last = ds, batch_size, shuffle, drop_last
        self.seed, self.step_for, self.pad_to, self.group_patterns = seed, step_for, pad_to, group_patterns
        self.fuse_patterns = bool(fuse_patterns)
        self.all_patterns = bool(all_patterns)
        self.ids_only = bool(ids_only)
        self.epoch = 0

    def __len__(self) -> int:
        n = self.ds.num_samples if self.fuse_patterns else len(self.ds)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self):
        gen = None
        if self.shuffle:
            gen = torch.Generator()
            gen.manual_seed((self.seed if self.seed is not None else 0) + self.epoch)
        self.epoch += 1
        return self.ds.device_loader(self.batch_size, self.shuffle, self.drop_last, gen, self.step_for, self.pad_to,
                                     self.group_patterns, self.fuse_patterns, self.all_patterns, self.ids_only)
