"""The UTT-Fusion embedding cache's pieces that need no GPU: tspm_utt_cache_rows on both sides of the ABI and its
refusals (every one returns before any launch), the ``ids_only`` loader against the tensor loader (order, pattern
draws, ``len``, batch keys - the tensor loader's gather replaced by a recorder of the indices it was handed), and the
Python-side refusals that touch no device."""
import ctypes
import os
import re

import pytest
import torch

import tspm_amd
from tspm_amd import _lib as L
from tspm_amd import harness
from tspm_amd import mosi as M
from tspm_amd import mosi_data as D

INVALID = 1
P = 4096  # a 16-byte aligned, non-NULL stand-in: never dereferenced, every call here returns before a launch
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tspm.h")
N, B, STEPS = 13, 5, (7, 9, 6)


def _desc(**kw):
    f = dict(batch=4, halves=1, w_audio=4, w_video=8, w_pool=12, ld_cache=24, ld_av=12, ld_pool=12, n_rows=6, n_zero=1,
             emb=P, zero=P, rows=P, row_keep=None, labels_all=P, labels_out=P, label_bytes=8, scale=2.0, keep=P,
             av_out=P, pool_out=P)
    f.update(kw)
    return L.UttCacheRowsDesc(**f)


def _call(**kw):
    return L.load().tspm_utt_cache_rows(ctypes.byref(_desc(**kw)), None)


def test_both_sides_declare_the_entry_point():
    assert "tspm_utt_cache_rows" in L.EXPORTED
    lib = L.load()
    assert lib.tspm_utt_cache_rows.argtypes[0]._type_ is L.UttCacheRowsDesc
    assert lib.tspm_abi_version() == 23 == L.ABI_VERSION  # an addition under ABI 23: the version number stays
    with open(HEADER) as f:
        h = f.read()
    assert re.search(r"int tspm_utt_cache_rows\(const tspm_utt_cache_rows_desc\* desc, tspm_stream_t stream\);", h)
    assert "#define TSPM_ABI_VERSION 23" in h
    body = h[h.index("typedef struct tspm_utt_cache_rows_desc {"):h.index("} tspm_utt_cache_rows_desc;")]
    for field, _ in L.UttCacheRowsDesc._fields_:  # the same fields in the same order on both sides
        assert re.search(rf"\b{field}\b", body), field
    order = [body.index(f) for f in ("batch, halves", "n_rows, n_zero", "* emb;", "* zero;", "* rows;", "* row_keep;",
                                     "* labels_all;", "* labels_out;", "label_bytes;", "scale;", "* keep;", "* av_out;",
                                     "* pool_out;")]
    assert order == sorted(order)


def test_every_refusal_returns_before_a_launch():
    for name in ("emb", "zero", "rows", "av_out", "pool_out"):
        assert _call(**{name: None}) == INVALID, name
    for name in ("w_audio", "w_video", "w_pool", "ld_cache", "ld_av", "ld_pool"):
        for bad in (0, -4, _desc().__getattribute__(name) + 2):
            assert _call(**{name: bad}) == INVALID, (name, bad)
    assert _call(ld_cache=20) == INVALID and _call(ld_av=8) == INVALID and _call(ld_pool=8) == INVALID
    for name in ("emb", "zero", "av_out", "pool_out", "keep"):
        assert _call(**{name: P + 4}) == INVALID, name
    for h in (0, 3, -1):
        assert _call(halves=h) == INVALID
    assert _call(halves=2, row_keep=P) == INVALID
    assert _call(n_zero=2) == INVALID and _call(n_zero=0) == INVALID
    assert _call(label_bytes=2) == INVALID and _call(labels_all=None) == INVALID and _call(labels_out=None) == INVALID
    assert _call(batch=0) == INVALID and _call(n_rows=0) == INVALID
    assert L.load().tspm_utt_cache_rows(None, None) == INVALID


# ------------------------------------------------------------------------------------------------
# the ids_only loader on the CPU
# ------------------------------------------------------------------------------------------------
def _ds(corpus, split, **kw):
    return D.MOSI(split=split, corpus=corpus, device="cpu", seed=4, **kw)


@pytest.mark.parametrize("split,kw", [("train", dict(shuffle=True, seed=7)),
                                      ("train", dict(shuffle=True, seed=7, all_patterns=True)),
                                      ("valid", dict()), ("valid", dict(fuse_patterns=True))],
                         ids=["train", "train-all", "valid", "valid-fused"])
def test_ids_only_loader_matches_the_tensor_loader(monkeypatch, split, kw):
    corpus = D.synthetic_mosi_corpus(N, seed=21, steps=6)
    seen = []

    def gather(self, index, steps_pad, out, time_major, masks=None, labels_out=None, lengths_out=None, rows=None):
        seen.append(index.tolist())  # the tensor loader's order, from the indices its gather is handed
    monkeypatch.setattr(D.DeviceMosiCorpus, "gather", gather)
    full, ids = _ds(corpus, split), _ds(corpus, split)
    lf, li = full.loader(B, pad_to=STEPS, **kw), ids.loader(B, pad_to=STEPS, ids_only=True, **kw)
    assert len(lf) == len(li) and li.ids_only and not lf.ids_only
    fused = kw.get("all_patterns") or kw.get("fuse_patterns")
    for epoch in range(2):
        del seen[:]
        bf = list(lf)
        want, n_gathers = list(seen), len(seen)
        bi = list(li)
        assert len(seen) == n_gathers, "the ids_only loader gathered something"
        assert len(bf) == len(bi) == len(lf) == (3 if split == "train" or fused else -(-7 * N // B))
        got = []
        for x, y in zip(bf, bi):
            grouped = "ids_only" not in y
            assert grouped == ("label" not in x) and (not grouped or list(x) == list(y))
            for gx, gy in ([(x[p], y[p]) for p in x] if grouped else [(x, y)]):
                assert gy["ids_only"] is True and gy["steps"] == STEPS == gx["steps"] and gy["dataset"] is ids
                assert gy["rows"].dtype == torch.int64 and gy["pad_to"] == STEPS
                assert not any(k in gy for k in ("audio", "video", "text", "label"))
                got.append(gy["rows"].tolist())
                if fused:
                    flag = "all_patterns" if kw.get("all_patterns") else "fused_patterns"
                    assert gy[flag] is True and gx[flag] is True and gy["patterns"] == gx["patterns"]
                    assert "row_keep" not in gy and "pattern_name" not in gy
                    assert set(gy) == {"ids_only", "rows", "steps", "dataset", "pad_to", "patterns", flag}
                else:
                    assert gy["pattern_name"] == gx["pattern_name"]  # the same pattern draws
                    assert gy["row_keep"].dtype == torch.uint8
                    assert gy["row_keep"].tolist() == [[int(ch in q) for ch in "avt"] for q in gy["pattern_name"]]
                    assert set(gy) == {"ids_only", "rows", "steps", "dataset", "pad_to", "row_keep", "pattern_name"}
        assert got == want  # the same order, batch by batch (and group by group)
        if kw.get("shuffle"):
            assert sorted(sum(got, [])) == list(range(N)) and sum(got, []) != list(range(N))
    assert li.epoch == lf.epoch == 2


def test_python_side_refusals():
    corpus = D.synthetic_mosi_corpus(N, seed=21, steps=6)
    mono = D.MOSI(split="train", corpus=corpus, device="cpu", target_modality="audio")
    with pytest.raises(tspm_amd.TspmError, match="multimodal target"):
        mono.loader(B, ids_only=True)
    with pytest.raises(tspm_amd.TspmError, match="multimodal target"):
        next(iter(mono.device_loader(B, ids_only=True)))
    with pytest.raises(tspm_amd.TspmError, match="multimodal target"):
        mono.embedding_cache(None)
    ds = _ds(corpus, "train")
    assert ds.corpus_steps(STEPS) == STEPS and ds.corpus_steps(0) == 6 and ds.corpus_steps(8) == 8
    with pytest.raises(tspm_amd.TspmError, match="all_patterns=True is for the multimodal train split"):
        _ds(corpus, "valid").loader(B, ids_only=True, all_patterns=True)
    torch.manual_seed(0)
    model = M.build_utt_fusion("mosi", embd_sizes=(8, 12, 8))
    opt = torch.optim.Adam(model.parameters())
    with pytest.raises(tspm_amd.TspmError, match="frozen encoders"):  # a trainable encoder: refused before any device use
        ds.embedding_cache(model, pad_to=STEPS)
    with pytest.raises(tspm_amd.TspmError, match="frozen encoders"):  # (fit's own refusals need a runner: GPU tests)
        harness._cached_mosi_loaders(model, {"train": ds.loader(B)})
    with pytest.raises(tspm_amd.TspmError, match="frozen encoders"):
        M.FusedMosiCachedStep(model, tspm_amd.FusedAdam.__new__(tspm_amd.FusedAdam), None, B, None)
    with pytest.raises(tspm_amd.TspmError, match="FusedAdam"):
        M.FusedMosiCachedStep(model, opt, None, B, None)
    M.finetune_param_groups(model, lr=1e-3, weight_decay=0.0, freeze=("audio", "video", "text"))
    with pytest.raises(tspm_amd.TspmError, match="ROCm"):  # frozen now, but nothing is on the device
        ds.embedding_cache(model, pad_to=STEPS)
    # the weights-generation counters a cache's staleness check reads
    gens = [getattr(model, a)._weights_generation for a in ("netA", "netV", "netT")]
    model.netV.load_state_dict(model.netV.state_dict())
    assert [getattr(model, a)._weights_generation for a in ("netA", "netV", "netT")] == [gens[0], gens[1] + 1, gens[2]]
    engines = model._engines
    model.load_state_dict(model.state_dict())
    model.float()
    assert all(getattr(model, a)._weights_generation >= g + 2 for a, g in zip(("netA", "netV", "netT"), gens))
    assert model._engines is not engines
