"""Several cached head steps per host call, without a device: the C entry point (exported, header against ctypes, every
refusal — they all precede the first launch), ``DeviceLoader.epoch_plan()`` against the same loader iterated, and the
partition of an epoch into host calls."""
import ctypes
import os
import random
import re

import pytest
import torch

from tspm_amd import _lib as L
from tspm_amd.data import AVMNIST, DeviceLoader, synthetic_corpus
from tspm_amd.harness import cached_epoch_chunks

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
N = 43
INVALID, WORKSPACE = 1, 3


# ------------------------------------------------------------------------------------------------
# the ABI
# ------------------------------------------------------------------------------------------------
def test_entry_point_header_and_signature_agree():
    src = open(os.path.join(REPO, "include", "tspm.h")).read()
    m = re.search(r"typedef struct tspm_head_adam_desc \{(.*?)\} tspm_head_adam_desc;", src, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [d.split()[-1].lstrip("*") for d in body.split(";") if d.strip()]
    assert fields == [n for n, _ in L.HeadAdamDesc._fields_] == ["param", "grad", "exp_avg", "exp_avg_sq", "count",
                                                                 "hyper"]
    assert ctypes.sizeof(L.HeadAdamDesc) == 48 and L.HeadAdamDesc.count.offset == 32
    assert int(re.search(r"#define TSPM_CACHED_HEAD_MAX_STEPS (\d+)", src).group(1)) == L.CACHED_HEAD_MAX_STEPS == 64
    decl = re.search(r"int tspm_cached_head_train_steps\((.*?)\);", src, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ["desc", "adam", "steps", "stream"]
    res, args = L._SIGS["tspm_cached_head_train_steps"]
    assert res is ctypes.c_int32 and len(args) == 4 and args[2] is ctypes.c_int32
    assert args[0]._type_ is L.CachedHeadTrainDesc and args[1]._type_ is L.HeadAdamDesc
    assert re.search(r"#define TSPM_ABI_VERSION (\d+)", src).group(1) == "23"
    lib = L.load()
    assert lib.tspm_abi_version() == 23 and hasattr(lib, "tspm_cached_head_train_steps")
    assert ctypes.sizeof(L.AdamHyper) == 64 and L.AdamHyper.step.offset == L.HYPER_STEP_OFFSET


class _Valid:
    """A descriptor pair no check refuses, over addresses nothing here dereferences (the device pointers are plain
    numbers; ``keep`` / ``group_id`` are real host arrays, the only pointers the checks read through).  Each refusal
    below changes ONE thing of it, so the call returns before any launch; the pair itself is never submitted."""
    B, F, WA, H, H2, C, P = 8, 192, 64, 128, 64, 10, 3
    BASE = 1 << 20

    def __init__(self):
        self.keep = (ctypes.c_int32 * 6)(1, 0, 1, 1, 0, 1)
        self.gid = (ctypes.c_int32 * 3)(0, 1, 2)
        sizes = [("w0", self.H * self.F), ("b0", self.H), ("w3", self.H2 * self.H), ("b3", self.H2),
                 ("w5", self.C * self.H2), ("b5", self.C)]
        self.off, at = {}, 0
        for n, c in sizes:
            self.off[n] = at
            at += (c + 3) // 4 * 4
        self.count = at
        self.param, self.grad, self.m, self.v = (self.BASE * i for i in (1, 2, 3, 4))
        self.hyper = self.BASE * 5

    def desc(self, **over):
        p = self.BASE * 6
        f = dict(batch=self.B, npat=self.P, in_=self.F, w_audio=self.WA, hidden=self.H, hidden2=self.H2, classes=self.C,
                 ld_emb=self.F, gen_keep=1, n_groups=3, n_rows=300, emb=p, x0=p + 4096, rows=p + 8192,
                 labels_all=p + 12288, keep=self.keep, group_id=self.gid, row_keep=None, row_group=None,
                 **{n: self.param + 4 * o for n, o in self.off.items()}, p=0.5, loss_weight=1.0, seed=1,
                 counter=self.hyper + L.HYPER_STEP_OFFSET, keep_mask=p + 16384, logits=p + 20480,
                 **{"g" + n: self.grad + 4 * o for n, o in self.off.items()}, loss=p + 24576, stats=None,
                 adam_step=self.hyper + L.HYPER_STEP_OFFSET, confusion=None, loss_log=None, counters=None,
                 log_capacity=0, workspace=self.BASE * 7,
                 workspace_bytes=int(L.lib().tspm_cached_head_train_workspace(self.B, self.P)))
        f.update(over)
        return L.CachedHeadTrainDesc(**f)

    def adam(self, **over):
        f = dict(param=self.param, grad=self.grad, exp_avg=self.m, exp_avg_sq=self.v, count=self.count, hyper=self.hyper)
        f.update(over)
        return L.HeadAdamDesc(**f)


def test_every_refusal_precedes_the_first_launch():
    lib, v = L.load(), _Valid()
    call = lambda d, a, steps=4: lib.tspm_cached_head_train_steps(d, a, steps, None)  # noqa: E731
    assert call(None, None) == INVALID and call(None, v.adam()) == INVALID and call(v.desc(), None) == INVALID
    for steps in (0, -3, L.CACHED_HEAD_MAX_STEPS + 1, 1 << 20):
        assert call(v.desc(), v.adam(), steps) == INVALID, steps
    # what tspm_cached_head_train_step refuses
    for over in (dict(batch=0), dict(npat=0), dict(npat=9), dict(in_=260), dict(hidden=130), dict(classes=17),
                 dict(w_audio=0), dict(w_audio=192), dict(n_rows=0), dict(ld_emb=188), dict(emb=None), dict(rows=None),
                 dict(labels_all=None), dict(keep=None), dict(w0=None), dict(gb5=None), dict(logits=None),
                 dict(loss=None), dict(p=1.0), dict(keep_mask=None), dict(log_capacity=-1), dict(x0=None),
                 dict(emb=v.BASE * 6 + 4), dict(row_keep=4096)):
        assert call(v.desc(**over), v.adam()) == INVALID, over
        assert lib.tspm_cached_head_train_step(v.desc(**over), None) == INVALID, over   # the shared checks
    for over in (dict(workspace=None), dict(workspace_bytes=16), dict(workspace=v.BASE * 7 + 8)):
        assert call(v.desc(**over), v.adam()) == WORKSPACE, over
    # the Adam bases: null, unaligned, count
    for over in (dict(param=None), dict(grad=None), dict(exp_avg=None), dict(exp_avg_sq=None), dict(hyper=None),
                 dict(exp_avg=v.m + 4), dict(exp_avg_sq=v.v + 8), dict(count=0), dict(count=-4)):
        assert call(v.desc(), v.adam(**over)) == INVALID, over
    for base in ("param", "grad"):   # moved as a whole by 4 bytes: unaligned (the tensors move with them)
        moved = {("g" if base == "grad" else "") + n: getattr(v, base) + 4 + 4 * o for n, o in v.off.items()}
        assert call(v.desc(**moved), v.adam(**{base: getattr(v, base) + 4})) == INVALID, base
    # the pointer-range rule: every gradient inside [grad, grad + count), its weight at the same offset of param
    assert call(v.desc(gw3=v.grad - 4 * v.H2 * v.H), v.adam()) == INVALID          # before the range
    assert call(v.desc(gw3=v.grad + 4 * v.count), v.adam()) == INVALID             # behind it
    assert call(v.desc(), v.adam(count=v.count - 8)) == INVALID                    # b5 runs past a shorter range
    assert call(v.desc(gb0=v.BASE * 8), v.adam()) == INVALID                       # elsewhere altogether
    for n in v.off:
        assert call(v.desc(**{n: v.param + 4 * v.off[n] + 16}), v.adam()) == INVALID, n
    assert call(v.desc(w3=v.grad + 4 * v.off["w3"]), v.adam()) == INVALID          # the gradient's own address
    # the step counter is the Adam group's own
    for step in (None, v.hyper, v.hyper + L.HYPER_STEP_OFFSET + 8, v.BASE * 9):
        assert call(v.desc(adam_step=step), v.adam()) == INVALID, step


# ------------------------------------------------------------------------------------------------
# the loader's epoch as one object
# ------------------------------------------------------------------------------------------------
def _ds(split="train", **kw):
    return AVMNIST(None, split, "multimodal", corpus=synthetic_corpus(N, 5), device=CPU, **kw)


CASES = [("train", dict(shuffle=True)), ("train", dict(shuffle=True, all_patterns=True)),
         ("valid", dict(fuse_patterns=True)), ("valid", dict())]


@pytest.mark.parametrize("drop_last", [False, True], ids=["keep_last", "drop_last"])
@pytest.mark.parametrize("split,kw", CASES, ids=["train", "train_all_patterns", "valid_fused", "valid_per_pattern"])
def test_plan_is_the_iteration_concatenated(split, kw, drop_last):
    ds_a, ds_b = _ds(split), _ds(split)
    ga, gb = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    random.seed(9)
    batches = list(DeviceLoader(ds_a, 8, generator=ga, ids_only=True, drop_last=drop_last, **kw))
    state = random.getstate()
    random.seed(9)
    loader = DeviceLoader(ds_b, 8, generator=gb, ids_only=True, drop_last=drop_last, **kw)
    plan = loader.epoch_plan()
    assert random.getstate() == state and torch.equal(ga.get_state(), gb.get_state())
    assert plan["batch_size"] == 8 and plan["n_batches"] == len(loader) == len(batches) > 0
    assert plan["dataset"] is ds_b
    assert getattr(ds_a, "current_pattern", None) == getattr(ds_b, "current_pattern", None)
    for key in ("sample_ids", "labels"):
        want = torch.cat([b[key] for b in batches])
        assert plan[key].dtype == want.dtype and torch.equal(plan[key], want), key
    assert plan["sample_ids"].dtype == torch.int64
    n = len(plan["sample_ids"])
    assert n == (len(batches) * 8 if drop_last else loader._n_items())
    assert [len(b["sample_ids"]) for b in batches] == [min(n, (i + 1) * 8) - i * 8 for i in range(len(batches))]
    fused = "all_patterns" if kw.get("all_patterns") else "fused_patterns" if kw.get("fuse_patterns") else None
    if fused:
        assert plan[fused] is True and plan["patterns"] == batches[0]["patterns"] == list(ds_b.selected_patterns)
        assert "keep" not in plan and "pattern_ids" not in plan and "pattern_names" not in plan
    else:
        assert "patterns" not in plan and "all_patterns" not in plan and "fused_patterns" not in plan
        keep = torch.cat([b["keep"] for b in batches])
        assert plan["keep"].dtype == torch.uint8 and plan["keep"].shape == (n, 2) and torch.equal(plan["keep"], keep)
        assert torch.equal(plan["pattern_ids"], torch.cat([b["pattern_ids"] for b in batches]))
        assert plan["pattern_names"] == [nm for b in batches for nm in b["pattern_name"]]


def test_plan_refusal_and_reuse():
    ds = _ds()
    with pytest.raises(L.TspmError, match="ids_only"):
        DeviceLoader(ds, 8).epoch_plan()
    # a second plan is a second epoch: it draws again
    g = torch.Generator().manual_seed(1)
    ld = DeviceLoader(ds, 8, shuffle=True, generator=g, ids_only=True)
    a, b = ld.epoch_plan(), ld.epoch_plan()
    assert not torch.equal(a["sample_ids"], b["sample_ids"])
    assert sorted(a["sample_ids"].tolist()) == sorted(b["sample_ids"].tolist())


# ------------------------------------------------------------------------------------------------
# the partition of an epoch into host calls
# ------------------------------------------------------------------------------------------------
def test_chunk_partition():
    assert cached_epoch_chunks(43, 8, 4) == ([4, 1], 3)            # 5 full batches, K = 4, a tail of 3
    assert cached_epoch_chunks(43, 8, 5) == ([5], 3) and cached_epoch_chunks(43, 8, 64) == ([5], 3)   # K >= full
    assert cached_epoch_chunks(40, 8, 4) == ([4, 1], 0) and cached_epoch_chunks(48, 8, 3) == ([3, 3], 0)
    assert cached_epoch_chunks(43, 8, 1) == cached_epoch_chunks(43, 8, None) == ([1] * 5, 3)          # per batch
    assert cached_epoch_chunks(3, 8, 4) == ([], 3) and cached_epoch_chunks(0, 8, 4) == ([], 0)
    assert cached_epoch_chunks(60000, 128, 16) == ([16] * 29 + [4], 96)
    big = cached_epoch_chunks(128 * 200, 128, 1000)[0]                                                # capped
    assert big == [L.CACHED_HEAD_MAX_STEPS] * 3 + [8]
    for n, b, k in ((43, 8, 4), (1000, 7, 5), (64, 8, 8)):
        chunks, tail = cached_epoch_chunks(n, b, k)
        assert sum(chunks) * b + tail == n and tail < b and all(1 <= c <= k for c in chunks)
    with pytest.raises(ValueError):
        cached_epoch_chunks(43, 8, 0)


def test_fit_refuses_steps_per_call_without_the_cache():
    from tspm_amd.harness import fit
    with pytest.raises(L.TspmError, match="cache_embeddings=True"):
        fit(None, None, None, {}, 1, steps_per_call=4)
