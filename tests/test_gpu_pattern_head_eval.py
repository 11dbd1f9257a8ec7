"""tspm_pattern_head_eval alone: the fusion head, the weighted cross-entropy and the classification log for every
missing-modality pattern of a batch in one call, against the plain-torch chain in fp64 (the fp32 run of the same chain
on the CPU is the yardstick, parity.op_check).  Shapes: a tiny head with odd sizes, the AVMNIST head at one row and at
seven; patterns: all three, one, and a subset in another order (group ids that are not 0..P-1)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import avmnist_eval_ref as eref
import parity
from tspm_amd import _lib as L

pytestmark = pytest.mark.gpu

SHAPES = [(5, 12, 4, 8, 4, 3), (1, 192, 64, 128, 64, 10), (7, 192, 64, 128, 64, 10)]  # B, F, w_audio, H, H2, C
PATSETS = [("a", "ai", "i"), ("a",), ("i", "ai")]
KEEP = {"a": (1, 0), "ai": (1, 1), "i": (0, 1)}
GID = {"a": 0, "ai": 1, "i": 2}
LOSS_WEIGHT = 0.7
_ids = lambda vals: ["x".join(str(v) for v in s) if isinstance(s[0], int) else "+".join(s) for s in vals]  # noqa: E731


def make_inputs(shape, seed=0):
    B, Fi, wa, H, H2, C = shape
    g = torch.Generator().manual_seed(1000 + seed + B * 7 + Fi)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    t = {"x": r(B, Fi), "x0": r(Fi), "w0": r(H, Fi) / Fi ** 0.5, "b0": r(H) * 0.1, "w3": r(H2, H) / H ** 0.5,
         "b3": r(H2) * 0.1, "w5": r(C, H2) / H2 ** 0.5 * 3, "b5": r(C) * 0.1}
    return t, torch.randint(0, C, (B,), generator=g)


def chain(t, labels, shape, pats, dtype):
    """[P*B, C] logits and [P] losses of the plain chain in ``dtype`` on the CPU."""
    B, Fi, wa, H, H2, C = shape
    c = {k: v.to(dtype) for k, v in t.items()}
    rows = []
    for p in pats:
        ka, ki = KEEP[p]
        rows.append(torch.cat([c["x"][:, :wa] if ka else c["x0"][:wa].expand(B, wa),
                               c["x"][:, wa:] if ki else c["x0"][wa:].expand(B, Fi - wa)], 1))
    h = torch.relu(torch.cat(rows) @ c["w0"].T + c["b0"])
    h = torch.relu(h @ c["w3"].T + c["b3"])
    logits = h @ c["w5"].T + c["b5"]
    loss = torch.stack([LOSS_WEIGHT * F.cross_entropy(logits[i * B:(i + 1) * B], labels) for i in range(len(pats))])
    return logits, loss


def run(dev, shape, pats, t, labels, counters0=(0, 0), capacity=16, ldx=None):
    """One call with every output in a parity.Guarded buffer; returns the outputs on the CPU (and asserts the guards)."""
    B, Fi, wa, H, H2, C = shape
    P = len(pats)
    ldx = ldx or Fi
    d = {k: v.to(dev).contiguous() for k, v in t.items()}
    xg = torch.zeros(B, ldx, device=dev)
    xg[:, :Fi] = d["x"]
    lab = labels.to(dev)
    logits, preds = parity.Guarded(dev, P * B, C), parity.Guarded(dev, P * B, 1, dtype=torch.int64)
    loss, llog = parity.Guarded(dev, P, 1), parity.Guarded(dev, capacity, 1)
    conf = torch.zeros(3, C, C, dtype=torch.int64, device=dev)
    counters = torch.tensor(list(counters0), dtype=torch.int64, device=dev)
    need = int(L.lib().tspm_pattern_head_eval_workspace(B, P))
    assert need >= P * B * 4
    ws = parity.Guarded(dev, need, 1, dtype=torch.uint8)
    keep = (ctypes.c_int32 * (2 * P))(*[k for p in pats for k in KEEP[p]])
    gid = (ctypes.c_int32 * P)(*[GID[p] for p in pats])
    desc = L.PatternHeadEvalDesc(
        batch=B, npat=P, in_=Fi, w_audio=wa, hidden=H, hidden2=H2, classes=C, ldx=ldx, x=xg.data_ptr(),
        x0=d["x0"].data_ptr(), keep=keep, group_id=gid, w0=d["w0"].data_ptr(), b0=d["b0"].data_ptr(),
        w3=d["w3"].data_ptr(), b3=d["b3"].data_ptr(), w5=d["w5"].data_ptr(), b5=d["b5"].data_ptr(),
        labels=lab.data_ptr(), loss_weight=LOSS_WEIGHT, n_groups=3, logits=logits.ptr(), preds=preds.ptr(),
        loss=loss.ptr(), confusion=conf.data_ptr(), loss_log=llog.ptr(), counters=counters.data_ptr(),
        log_capacity=capacity, workspace=ws.ptr(), workspace_bytes=need)
    L.check(L.lib().tspm_pattern_head_eval(desc, L.stream_handle()), "pattern_head_eval")
    torch.cuda.synchronize()
    for name, gd in (("logits", logits), ("preds", preds), ("loss", loss), ("loss_log", llog), ("workspace", ws)):
        gd.intact(name)
    return {"logits": logits.cpu(), "preds": preds.cpu().reshape(-1), "loss": loss.cpu().reshape(-1),
            "loss_log": llog.flat[:capacity].cpu(), "conf": conf.cpu().numpy(), "counters": counters.cpu().tolist()}


def own_confusion(out, labels, shape, pats):
    B, C = shape[0], shape[-1]
    groups = np.repeat([GID[p] for p in pats], B)
    return eref.confusion(np.tile(labels.numpy(), len(pats)), out["preds"].numpy(), groups, 3, C)


@pytest.mark.parametrize("pats", PATSETS, ids=_ids(PATSETS))
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_against_the_fp64_chain(gpu, shape, pats):
    B, C, P = shape[0], shape[-1], len(pats)
    t, labels = make_inputs(shape)
    out = run(gpu, shape, pats, t, labels, counters0=(2, 100))
    l64, s64 = chain(t, labels, shape, pats, torch.float64)
    l32, s32 = chain(t, labels, shape, pats, torch.float32)
    ratios = parity.Ratios()
    parity.op_check(f"logits[{shape},{pats}]", out["logits"], l32, l64, ratios=ratios)
    parity.op_check(f"loss[{shape},{pats}]", out["loss"], s32, s64, ratios=ratios)
    print("worst ratios:", ratios)
    flips = parity.near_tie_flips("preds", out["preds"], eref.predictions(l64), l64, 1)
    print(f"preds: {flips} near-tie flips of {P * B}")
    # the counts are those of the kernel's own predictions, each row under its pattern's group
    assert np.array_equal(out["conf"], own_confusion(out, labels, shape, pats)) and out["conf"].sum() == P * B
    # the predictions are tspm_classify_update's (first maximum of the softmax values) of the kernel's own logits
    assert torch.equal(out["preds"], eref.predictions(out["logits"]))
    # P log entries in pattern order behind the two already there, bitwise loss[p]; both counters advanced
    assert out["loss_log"][2:2 + P].view(torch.int32).tolist() == out["loss"].view(torch.int32).tolist()
    assert out["counters"] == [2 + P, 100 + P * B]
    # a second call on the same inputs is bitwise equal
    again = run(gpu, shape, pats, t, labels, counters0=(2, 100))
    for k in ("logits", "loss", "preds"):
        assert torch.equal(out[k].view(torch.int32) if out[k].dtype == torch.float32 else out[k],
                           again[k].view(torch.int32) if again[k].dtype == torch.float32 else again[k]), k


def test_padded_input_rows(gpu):
    """ldx > in: the padding columns of x are never read into the result."""
    shape, pats = SHAPES[0], PATSETS[0]
    t, labels = make_inputs(shape)
    a, b = run(gpu, shape, pats, t, labels), run(gpu, shape, pats, t, labels, ldx=shape[1] + 8)
    assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["loss"], b["loss"])


def test_exact_tie_gives_the_first_index(gpu):
    shape, pats = SHAPES[2], PATSETS[0]
    t, labels = make_inputs(shape)
    t["w5"][7] = t["w5"][3]           # classes 3 and 7 get the same logit on every row, above every other
    t["b5"][3] = t["b5"][7] = 50.0
    out = run(gpu, shape, pats, t, labels)
    assert torch.equal(out["logits"][:, 3], out["logits"][:, 7])
    assert out["preds"].tolist() == [3] * (3 * shape[0])
    assert np.array_equal(out["conf"], own_confusion(out, labels, shape, pats))


def test_log_capacity_smaller_than_the_pattern_count(gpu):
    shape, pats = SHAPES[0], PATSETS[0]
    t, labels = make_inputs(shape)
    out = run(gpu, shape, pats, t, labels, counters0=(1, 9), capacity=2)  # room for one of the three entries
    assert out["loss_log"][1].item() == out["loss"][0].item()
    assert out["loss_log"][:1].view(torch.int32).item() == 0x7FA5A5A5   # the earlier entry was not touched
    assert out["counters"] == [4, 9 + 3 * shape[0]]                        # the counters advance all the same
    full = run(gpu, shape, pats, t, labels, counters0=(5, 0), capacity=2)   # no room at all
    assert full["counters"] == [8, 3 * shape[0]] and torch.equal(full["loss"], out["loss"])


@pytest.mark.parametrize("bad_label", [10, -1, 1 << 40])
def test_out_of_range_label(gpu, bad_label):
    shape, pats = SHAPES[2], PATSETS[0]
    B, P = shape[0], len(pats)
    t, labels = make_inputs(shape)
    good = run(gpu, shape, pats, t, labels)
    bad_labels = labels.clone()
    bad_labels[4] = bad_label
    out = run(gpu, shape, pats, t, bad_labels)
    assert torch.isnan(out["loss"]).all() and torch.isnan(out["loss_log"][:P]).all()
    assert torch.equal(out["logits"], good["logits"]) and torch.equal(out["preds"], good["preds"])
    keep_rows = np.tile(np.arange(B) != 4, P)
    want = eref.confusion(np.tile(labels.numpy(), P)[keep_rows], out["preds"].numpy()[keep_rows],
                          np.repeat([GID[p] for p in pats], B)[keep_rows], 3, shape[-1])
    assert np.array_equal(out["conf"], want) and out["conf"].sum() == P * (B - 1)
    assert out["counters"] == [P, P * B]


def test_rows_do_not_depend_on_the_batch_or_the_patterns(gpu):
    shape, pats = SHAPES[2], PATSETS[0]
    B, C = shape[0], shape[-1]
    t, labels = make_inputs(shape)
    full = run(gpu, shape, pats, t, labels)["logits"].view(3, B, C)
    # rows 0..2 of the batch of seven, as a batch of three
    t3 = dict(t, x=t["x"][:3].clone())
    sub = run(gpu, (3,) + shape[1:], pats, t3, labels[:3])["logits"].view(3, 3, C)
    assert torch.equal(full[:, :3], sub)
    # a permuted batch gives permuted logits
    perm = torch.tensor([3, 0, 6, 2, 5, 1, 4])
    tp = dict(t, x=t["x"][perm].clone())
    assert torch.equal(run(gpu, shape, pats, tp, labels[perm])["logits"].view(3, B, C), full[:, perm])
    # a pattern's rows are the same whatever other patterns ride along, in whatever order
    two = run(gpu, shape, ("i", "ai"), t, labels)["logits"].view(2, B, C)
    assert torch.equal(two[0], full[2]) and torch.equal(two[1], full[1])
    one = run(gpu, shape, ("a",), t, labels)["logits"].view(1, B, C)
    assert torch.equal(one[0], full[0])


def test_more_samples_than_workgroups(gpu):
    """300 samples on the kernel's 256 workgroups: the second sample of a workgroup equals the same row alone."""
    shape, pats = (300,) + SHAPES[0][1:], PATSETS[0]
    B, C = 300, shape[-1]
    g = torch.Generator().manual_seed(5)
    t, _ = make_inputs(SHAPES[0])
    t["x"] = torch.randn(B, shape[1], generator=g)
    labels = torch.randint(0, C, (B,), generator=g)
    out = run(gpu, shape, pats, t, labels)
    l64, s64 = chain(t, labels, shape, pats, torch.float64)
    l32, s32 = chain(t, labels, shape, pats, torch.float32)
    parity.op_check("logits[300 rows]", out["logits"], l32, l64)
    parity.op_check("loss[300 rows]", out["loss"], s32, s64)
    tail = dict(t, x=t["x"][256:].clone())
    sub = run(gpu, (44,) + shape[1:], pats, tail, labels[256:])["logits"].view(3, 44, C)
    assert torch.equal(out["logits"].view(3, B, C)[:, 256:], sub)
    assert np.array_equal(out["conf"], own_confusion(out, labels, shape, pats))
