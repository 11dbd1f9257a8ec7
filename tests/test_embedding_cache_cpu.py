"""The cached head stage without a device: ``ids_only`` loaders against the same loader without the flag (ids, keep
flags, pattern ids, order, ``len``, RNG draws), the ``"cached"`` key of ``step.train_step_key``, the refusals that need
no GPU, and the ctypes descriptors of the new entry points against include/tspm.h."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

from tspm_amd import _lib as L
from tspm_amd.data import AVMNIST, DeviceLoader, synthetic_corpus

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
N = 37


def _ds(split="train", **kw):
    return AVMNIST(None, split, "multimodal", corpus=synthetic_corpus(N, 5), device=CPU, **kw)


def _epoch(ds, rng_seed, **kw):
    """(batches of the ids_only loader, what the same loader without the flag resolves, both generators' end states)."""
    g1, g2 = torch.Generator().manual_seed(rng_seed), torch.Generator().manual_seed(rng_seed)
    cached = DeviceLoader(ds, 8, generator=g1, ids_only=True, **kw)
    plain = DeviceLoader(ds, 8, generator=g2, **kw)
    random.seed(rng_seed)
    batches = list(cached)
    random.seed(rng_seed)
    order = plain.items()
    nb = len(plain)
    order = order[:nb * 8] if plain.drop_last else order
    assert len(cached) == nb == len(batches)
    assert torch.equal(g1.get_state(), g2.get_state())      # the same draws from the loader's generator
    return batches, order, plain


@pytest.mark.parametrize("kw", [dict(), dict(shuffle=True), dict(shuffle=True, drop_last=True),
                                dict(shuffle=True, world_size=2, rank=1, seed=4), dict(world_size=3, rank=0, drop_last=True)],
                         ids=["sequential", "shuffle", "drop_last", "sharded", "sharded_drop_last"])
@pytest.mark.parametrize("split", ["train", "valid"])
def test_ids_only_batches_are_the_plain_loaders_items(split, kw):
    ds = _ds(split)
    batches, order, plain = _epoch(ds, 11, **kw)
    random.seed(11)
    samples, names, am, im = ds._resolve(order)
    state = random.getstate()
    random.seed(11)
    list(DeviceLoader(ds, 8, generator=torch.Generator().manual_seed(11), ids_only=True, **kw))
    assert random.getstate() == state                        # ... and from Python's RNG (the train split's pattern draw)
    ids = torch.cat([b["sample_ids"] for b in batches])
    assert ids.dtype == torch.int64 and np.array_equal(ids.numpy(), samples)
    keep = torch.cat([b["keep"] for b in batches])
    assert keep.dtype == torch.uint8 and keep.shape == (len(samples), 2)
    assert np.array_equal(keep.numpy(), np.stack([am != 0, im != 0], 1).astype(np.uint8))
    assert np.array_equal(torch.cat([b["pattern_ids"] for b in batches]).numpy(), ds.pattern_ids(names))
    assert [n for b in batches for n in b["pattern_name"]] == list(names)
    assert np.array_equal(torch.cat([b["labels"] for b in batches]).numpy(), ds.corpus.labels[samples])
    for b in batches:
        assert b["cached"] is True and b["dataset"] is ds and "audio" not in b and "image" not in b
        assert len(b["sample_ids"]) == len(b["labels"]) == len(b["pattern_name"]) <= 8
    if not kw.get("drop_last") and kw.get("world_size", 1) == 1:
        assert len(ids) == len(ds) and len(batches[-1]["sample_ids"]) == len(ds) % 8


@pytest.mark.parametrize("kw", [dict(), dict(shuffle=True, drop_last=True), dict(shuffle=True, world_size=2, rank=0)],
                         ids=["sequential", "drop_last", "sharded"])
@pytest.mark.parametrize("split,flag", [("train", "all_patterns"), ("valid", "fuse_patterns")])
def test_ids_only_composes_with_the_pattern_loaders(split, flag, kw):
    ds = _ds(split, selected_patterns=["i", "ai"])
    batches, order, plain = _epoch(ds, 7, **{flag: True}, **kw)
    ids = torch.cat([b["sample_ids"] for b in batches])
    assert np.array_equal(ids.numpy(), order) and ids.max().item() < N
    key = "all_patterns" if flag == "all_patterns" else "fused_patterns"
    for b in batches:
        assert b["cached"] is True and b[key] is True and b["patterns"] == ["i", "ai"]
        assert "keep" not in b and "pattern_ids" not in b and "pattern_name" not in b
        assert np.array_equal(b["labels"].numpy(), ds.corpus.labels[b["sample_ids"].numpy()])


class _HostCorpus:
    """Stands in for ``data.DeviceCorpus`` where there is no device: the plain loader's own ``__iter__`` runs against
    it, and ``gather`` hands back what it was asked for (index, masks) next to the labels."""

    def __init__(self, ds):
        self.device, self.labels, self.asked = CPU, torch.from_numpy(ds.corpus.labels), []

    def gather(self, index, audio_mask=None, image_mask=None, want_audio=True, want_image=True, out=None, stream=None):
        self.asked.append((index.clone(), None if audio_mask is None else audio_mask.clone(),
                           None if image_mask is None else image_mask.clone()))
        return None, None, self.labels[index]


@pytest.mark.parametrize("kw", [dict(shuffle=True), dict(shuffle=True, drop_last=True, world_size=2, rank=1, seed=4),
                                dict(shuffle=True, all_patterns=True), dict(fuse_patterns=True)],
                         ids=["shuffle", "sharded_drop_last", "all_patterns", "fuse_patterns"])
def test_ids_only_batches_against_the_plain_loader_iterated(monkeypatch, kw):
    """The plain loader itself, iterated (its gather answered on the host): batch for batch the ``ids_only`` loader
    yields the indices, masks, labels, pattern names and ids that the plain loader hands to its gather and packs."""
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)   # no device here: nothing to pin for
    ds = _ds("valid" if kw.get("fuse_patterns") else "train")
    ds._dev = host = _HostCorpus(ds)
    random.seed(3)
    plain = list(DeviceLoader(ds, 8, generator=torch.Generator().manual_seed(3), **kw))
    state = random.getstate()
    random.seed(3)
    cached = list(DeviceLoader(ds, 8, generator=torch.Generator().manual_seed(3), ids_only=True, **kw))
    assert random.getstate() == state and len(plain) == len(cached) == len(host.asked) > 0
    for pb, cb, (index, am, im) in zip(plain, cached, host.asked):
        assert torch.equal(cb["sample_ids"], index) and torch.equal(cb["labels"], pb["labels"])
        assert cb.get("pattern_name") == pb.get("pattern_name") and cb.get("patterns") == pb.get("patterns")
        assert bool(cb.get("all_patterns")) == bool(pb.get("all_patterns"))
        assert bool(cb.get("fused_patterns")) == bool(pb.get("fused_patterns"))
        if am is None:
            assert "keep" not in cb and "pattern_ids" not in pb
        else:
            assert torch.equal(cb["keep"], torch.stack([am != 0, im != 0], 1).to(torch.uint8))
            assert torch.equal(cb["pattern_ids"], pb["pattern_ids"])


def test_loader_refusals():
    ds = _ds()
    with pytest.raises(L.TspmError, match="excludes out="):
        DeviceLoader(ds, 8, ids_only=True, out=(None, None, None))
    with pytest.raises(L.TspmError, match="excludes out="):
        ds.device_loader(8, ids_only=True, out=(None, None, None))
    frac = AVMNIST(None, "train", "multimodal", corpus=ds.corpus, device=CPU, missing_patterns={
        "ai": {"audio": 1.0, "image": 1.0}, "a": {"audio": 1.0, "image": 0.5}, "i": {"audio": 0.0, "image": 1.0}})
    with pytest.raises(L.TspmError, match="0 / 1 presence probabilities"):
        frac.device_loader(8, ids_only=True)
    mono = AVMNIST(None, "train", "image", corpus=ds.corpus, device=CPU)
    with pytest.raises(L.TspmError, match="multimodal target"):
        mono.device_loader(8, ids_only=True)
    with pytest.raises(L.TspmError, match="multimodal target"):
        mono.embedding_cache(object())
    with pytest.raises(L.TspmError, match="exclude each other"):
        ds.device_loader(8, ids_only=True, all_patterns=True, fuse_patterns=True)
    with pytest.raises(L.TspmError, match="all_patterns=True is for the multimodal train split"):
        _ds("valid").device_loader(8, ids_only=True, all_patterns=True)


def test_cached_train_step_key_and_routing():
    import tspm_amd
    from tspm_amd.step import train_step_key
    model = tspm_amd.AVMNIST(tspm_amd.ResNet18(1, 64), tspm_amd.ResNet34(1, 128), 128)
    assert train_step_key(model, 16) == 16 and train_step_key(model, 16, cached=False) == 16
    model.freeze_encoders()
    fr = ("frozen", ("audio_encoder", "image_encoder"))
    assert train_step_key(model, 16) == (16, fr)
    assert train_step_key(model, 16, ("a", "ai")) == (("patterns", ("a", "ai")), 16, fr)
    assert train_step_key(model, 16, cached=True) == (16, fr, ("cached",))
    assert train_step_key(model, 16, ("a", "ai"), cached=True) == (("patterns", ("a", "ai")), 16, fr, ("cached",))
    # a "cached" batch goes to the cached steps, which ask its dataset for the cache: refused here, without a device,
    # by name
    b = {"cached": True, "sample_ids": torch.arange(4), "labels": torch.zeros(4, dtype=torch.int64)}
    with pytest.raises(L.TspmError, match='names its dataset under "dataset"'):
        model.train_step(b, None, None, CPU, None)
    with pytest.raises(L.TspmError, match="DeviceMetricRecorder"):
        model.validation_step(b, None, CPU, None)
    # the weights generations the cache compares
    ga, gf = model.audio_encoder._weights_generation, model._freeze_generation
    model.load_state_dict(model.state_dict())
    assert model.audio_encoder._weights_generation == ga + 1
    model.image_encoder.load_state_dict(model.image_encoder.state_dict())
    model.audio_encoder.float()
    assert model.audio_encoder._weights_generation == ga + 2
    model.unfreeze_encoders()
    assert model._freeze_generation == gf + 1


def test_supported_mirror():
    assert L.cached_head_train_supported(192, 64, 128, 64, 10, 3) and L.cached_head_train_supported(12, 4, 8, 4, 3, 1)
    for bad in ((192, 64, 128, 64, 10, 9), (192, 0, 128, 64, 10, 1), (192, 62, 128, 64, 10, 1), (260, 64, 128, 64, 10, 1),
                (192, 64, 130, 64, 10, 1), (192, 64, 128, 64, 17, 1)):
        assert not L.cached_head_train_supported(*bad), bad


def _header_struct(name):
    src = open(os.path.join(REPO, "include", "tspm.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype = re.match(r"(const\s+)?\w+", decl).group(0)
        for part in decl[len(ctype):].split(","):
            fields.append((part.strip().lstrip("*").strip(), "*" in part or "*" in ctype, ctype.replace("const ", "")))
    return fields


def test_descriptors_match_the_header():
    """Field for field: the ctypes descriptor's names, order and widths are tspm.h's (``in`` is ``in_`` in Python)."""
    lib = L.load()
    fields = _header_struct("tspm_cached_head_train_desc")
    width = {"int32_t": 4, "int64_t": 8, "uint64_t": 8, "float": 4, "size_t": ctypes.sizeof(ctypes.c_size_t)}
    got = L.CachedHeadTrainDesc._fields_
    assert [n for n, _ in got] == [("in_" if n == "in" else n) for n, _, _ in fields]
    for (n, ct), (_, is_ptr, ctype) in zip(got, fields):
        assert ctypes.sizeof(ct) == (ctypes.sizeof(ctypes.c_void_p) if is_ptr else width[ctype]), n
    assert ctypes.sizeof(L.CachedHeadTrainDesc) == 320
    assert L.CachedHeadTrainDesc.n_rows.offset == 40 and L.CachedHeadTrainDesc.emb.offset == 48
    assert L.CachedHeadTrainDesc.workspace_bytes.offset == 312
    # the workspace is tspm_pattern_head_train_step's; refusals return before any launch (no GPU here)
    for b, p in ((128, 3), (1, 1), (259, 8)):
        assert lib.tspm_cached_head_train_workspace(b, p) == lib.tspm_pattern_head_train_workspace(b, p) > 0
    assert lib.tspm_cached_head_train_workspace(0, 1) == 0 and lib.tspm_cached_head_train_workspace(8, 9) == 0
    assert lib.tspm_cached_head_train_step(None, None) == 1
    assert lib.tspm_cached_head_train_step(ctypes.byref(L.CachedHeadTrainDesc(batch=8, npat=1, in_=192)), None) == 1
    P = 4096
    assert lib.tspm_embed_gather(0, 192, P, 300, 192, P, P, None, 0, None, P, 192, P, None) == 1
    assert lib.tspm_embed_gather(8, 190, P, 300, 192, P, P, None, 0, None, P, 192, P, None) == 1
    assert lib.tspm_embed_gather(8, 192, P, 300, 192, P, P, P, 64, None, P, 192, P, None) == 1   # row_keep without x0
    assert lib.tspm_embed_gather(8, 192, P, 300, 192, P, None, None, 0, None, P, 192, P, None) == 1
    assert len(L._SIGS["tspm_embed_gather"][1]) == 14
