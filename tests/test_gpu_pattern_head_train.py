"""tspm_pattern_head_train_step alone: the fusion head's forward, dropout, weighted cross-entropy and weight backward over
every missing-modality pattern of a batch on frozen encoders, in one call, against the plain-torch chain on the
REPLICATED rows in fp64 (tests/head_stage_ref.py; the fp32 CPU run of the same chain is the yardstick, parity.op_check,
gradients with grad=True).  Shapes: a tiny head with odd sizes, the AVMNIST head at one row and at seven, and more
samples than the kernel has workgroups; patterns: all three, one, and a subset in another order; without dropout and
with p = 0.5 on a supplied mask."""
import ctypes

import pytest
import torch

import head_stage_ref as R
import parity
from tspm_amd import _lib as L

pytestmark = pytest.mark.gpu

SHAPES = [(5, 12, 4, 8, 4, 3), (1, 192, 64, 128, 64, 10), (7, 192, 64, 128, 64, 10), (259, 12, 4, 8, 4, 3)]
PATSETS = [("a", "ai", "i"), ("a",), ("i", "ai")]
LOSS_WEIGHT = 0.7
GRADS = ("gw0", "gb0", "gw3", "gb3", "gw5", "gb5")
_ids = lambda vals: ["x".join(str(v) for v in s) if isinstance(s[0], int) else "+".join(s) for s in vals]  # noqa: E731
_CACHE = {}


def case(shape, seed=0):
    """x, x0, labels and the head's weights for a shape (fp32, CPU), built once per shape and never modified."""
    key = (shape, seed)
    if key not in _CACHE:
        B, F, wa, H, H2, C = shape
        x, x0, labels = R.inputs(B, F, C, seed=100 + seed + B)
        _CACHE[key] = (x, x0, labels, R.make_head(F, H, H2, C, seed=7 + seed))
    return _CACHE[key]


def mask_for(shape, P, p=0.5, seed=9):
    B, H = shape[0], shape[3]
    return (torch.rand(P * B, H, generator=torch.Generator().manual_seed(seed)) >= p).to(torch.uint8)


def run(dev, shape, pats, x, x0, labels, W, p=0.0, mask=None, gen_keep=0, seed=0, counter=None, adam_step=None,
        stats0=(0.0, 0.0, 0.0), ldx=None):
    """One call with every output in a parity.Guarded buffer; returns the outputs on the CPU (and asserts the guards)."""
    B, F, wa, H, H2, C = shape
    P = len(pats)
    n = P * B
    ldx = ldx or F
    d = {k: v.to(dev).contiguous() for k, v in W.items()}
    xg = torch.zeros(B, ldx, device=dev)
    xg[:, :F] = x.to(dev)
    x0d, lab = x0.to(dev).contiguous(), labels.to(dev)
    out = {"logits": parity.Guarded(dev, n, C), "loss": parity.Guarded(dev, 1, 1), "gw0": parity.Guarded(dev, H, F),
           "gb0": parity.Guarded(dev, 1, H), "gw3": parity.Guarded(dev, H2, H), "gb3": parity.Guarded(dev, 1, H2),
           "gw5": parity.Guarded(dev, C, H2), "gb5": parity.Guarded(dev, 1, C),
           "mask": parity.Guarded(dev, n, H, dtype=torch.uint8)}
    if mask is not None:
        out["mask"].t.copy_(mask.to(dev))
    stats = torch.tensor(list(stats0) + [0.0], device=dev)
    need = int(L.lib().tspm_pattern_head_train_workspace(B, P))
    ws = parity.Guarded(dev, need, 1, dtype=torch.uint8)
    keep = (ctypes.c_int32 * (2 * P))(*[k for pt in pats for k in R.KEEP[pt]])
    desc = L.PatternHeadTrainDesc(
        batch=B, npat=P, in_=F, w_audio=wa, hidden=H, hidden2=H2, classes=C, ldx=ldx, gen_keep=gen_keep, x=xg.data_ptr(),
        x0=x0d.data_ptr(), keep=keep, w0=d["w0"].data_ptr(), b0=d["b0"].data_ptr(), w3=d["w3"].data_ptr(),
        b3=d["b3"].data_ptr(), w5=d["w5"].data_ptr(), b5=d["b5"].data_ptr(), labels=lab.data_ptr(), p=p,
        loss_weight=LOSS_WEIGHT, seed=seed, counter=None if counter is None else counter.data_ptr(),
        keep_mask=out["mask"].ptr() if p > 0 else None, logits=out["logits"].ptr(),
        **{g: out[g].ptr() for g in GRADS}, loss=out["loss"].ptr(), stats=stats.data_ptr(),
        adam_step=None if adam_step is None else adam_step.data_ptr(), workspace=ws.ptr(), workspace_bytes=need)
    L.check(L.lib().tspm_pattern_head_train_step(desc, L.stream_handle()), "pattern_head_train_step")
    torch.cuda.synchronize()
    for name, gd in out.items():
        if name == "mask" and p == 0:
            assert bool((gd.flat == 0xA5).all()), "keep_mask touched without dropout"
            continue
        gd.intact(name)
    ws.intact("workspace")
    res = {k: v.cpu() for k, v in out.items()}
    for g in ("gb0", "gb3", "gb5", "loss"):
        res[g] = res[g].reshape(-1)
    res["stats"] = stats.cpu()
    return res


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("p", [0.0, 0.5], ids=["p0", "p0.5"])
@pytest.mark.parametrize("pats", PATSETS, ids=_ids(PATSETS))
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_against_the_fp64_chain(gpu, shape, pats, p):
    B, F, wa, H, H2, C = shape
    P = len(pats)
    x, x0, labels, W = case(shape)
    mask = mask_for(shape, P) if p else None
    out = run(gpu, shape, pats, x, x0, labels, W, p=p, mask=mask, stats0=(1.5, 2.0, 3.0))
    keep = R.keep_of(pats)
    r64 = R.chain(x, x0, keep, wa, W, labels, LOSS_WEIGHT, p, mask, torch.float64)
    r32 = R.chain(x, x0, keep, wa, W, labels, LOSS_WEIGHT, p, mask, torch.float32)
    ratios = parity.Ratios()
    tag = f"[{shape},{pats},p={p}]"
    parity.op_check("logits" + tag, out["logits"], r32["logits"], r64["logits"], ratios=ratios)
    parity.op_check("loss" + tag, out["loss"], r32["loss"], r64["loss"], ratios=ratios)
    for g in GRADS:
        parity.op_check(g + tag, out[g], r32["g" + g[1:]], r64["g" + g[1:]], grad=True, ratios=ratios)
    print("worst ratios:", ratios)
    flips = parity.near_tie_flips("preds", out["logits"].argmax(1), r64["logits"].argmax(1), r64["logits"], 1)
    print(f"preds: {flips} near-tie flips of {P * B}")
    # stats: += sum CE, += #(argmax == label) of the kernel's own logits (first maximum), += P*B
    own_correct = int((out["logits"].argmax(1) == labels.repeat(P)).sum())
    assert out["stats"][1].item() == 2.0 + own_correct and out["stats"][2].item() == 3.0 + P * B
    assert abs(out["stats"][0].item() - 1.5 - r64["ce_sum"].item()) <= 1e-5 * (1.5 + r64["ce_sum"].item())
    # the supplied mask is read, not written
    if p:
        assert torch.equal(out["mask"], mask)
    # a second call on the same inputs is bitwise equal
    again = run(gpu, shape, pats, x, x0, labels, W, p=p, mask=mask, stats0=(1.5, 2.0, 3.0))
    for k in ("logits", "loss", "stats") + GRADS:
        assert torch.equal(bits(out[k]), bits(again[k])), k


def test_padded_input_rows(gpu):
    """ldx > in: the padding columns of x are never read into the result."""
    shape, pats = SHAPES[0], PATSETS[0]
    x, x0, labels, W = case(shape)
    a = run(gpu, shape, pats, x, x0, labels, W)
    b = run(gpu, shape, pats, x, x0, labels, W, ldx=shape[1] + 8)
    for k in ("logits", "loss") + GRADS:
        assert torch.equal(bits(a[k]), bits(b[k])), k


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3]], ids=_ids([SHAPES[2], SHAPES[3]]))
def test_generated_mask_is_tspm_dropout_mask_and_adam_step_is_bumped_once(gpu, shape):
    pats = PATSETS[0]
    B, H, P = shape[0], shape[3], len(PATSETS[0])
    x, x0, labels, W = case(shape)
    seed, p = 0x1234_5678_9ABC, 0.5
    ctr = torch.tensor([41], dtype=torch.int64, device=gpu)  # the dropout counter IS Adam's step counter, as in the step
    out = run(gpu, shape, pats, x, x0, labels, W, p=p, gen_keep=1, seed=seed, counter=ctr, adam_step=ctr)
    assert ctr.item() == 42                                   # bumped once, by launch 2
    want = torch.empty(P * B * H, dtype=torch.uint8, device=gpu)
    c41 = torch.tensor([41], dtype=torch.int64, device=gpu)   # ... after launch 1 drew the mask from 41
    L.check(L.lib().tspm_dropout_mask(P * B * H, p, seed, c41.data_ptr(), want.data_ptr(), L.stream_handle()), "mask")
    torch.cuda.synchronize()
    assert torch.equal(out["mask"].reshape(-1), want.cpu())
    assert 0.4 < out["mask"].float().mean().item() < 0.6
    # the same step on the supplied copy of that mask: bitwise the same results
    fed = run(gpu, shape, pats, x, x0, labels, W, p=p, mask=out["mask"], gen_keep=0)
    for k in ("logits", "loss") + GRADS:
        assert torch.equal(bits(out[k]), bits(fed[k])), k
    # without adam_step nothing is bumped
    run(gpu, shape, pats, x, x0, labels, W, p=p, gen_keep=1, seed=seed, counter=ctr)
    assert ctr.item() == 42


def test_rows_do_not_depend_on_the_batch_or_the_patterns(gpu):
    shape, pats = SHAPES[2], PATSETS[0]
    B, F, wa, H, H2, C = shape
    x, x0, labels, W = case(shape)
    mask = mask_for(shape, 3).view(3, B, H)
    full = run(gpu, shape, pats, x, x0, labels, W, p=0.5, mask=mask.reshape(3 * B, H))["logits"].view(3, B, C)
    # rows 0..2 of the batch of seven, as a batch of three
    sub = run(gpu, (3,) + shape[1:], pats, x[:3].clone(), x0, labels[:3], W, p=0.5,
              mask=mask[:, :3].reshape(9, H))["logits"].view(3, 3, C)
    assert torch.equal(full[:, :3], sub)
    # a permuted batch gives permuted logits
    perm = torch.tensor([3, 0, 6, 2, 5, 1, 4])
    got = run(gpu, shape, pats, x[perm].clone(), x0, labels[perm], W, p=0.5,
              mask=mask[:, perm].reshape(3 * B, H))["logits"].view(3, B, C)
    assert torch.equal(got, full[:, perm])
    # a pattern's rows are the same whatever other patterns ride along, in whatever order
    two = run(gpu, shape, ("i", "ai"), x, x0, labels, W, p=0.5,
              mask=mask[[2, 1]].reshape(2 * B, H))["logits"].view(2, B, C)
    assert torch.equal(two[0], full[2]) and torch.equal(two[1], full[1])
    one = run(gpu, shape, ("a",), x, x0, labels, W, p=0.5, mask=mask[0].reshape(B, H))["logits"].view(1, B, C)
    assert torch.equal(one[0], full[0])
    # ... and the labels (a sample's logits know nothing of them)
    other = run(gpu, shape, pats, x, x0, (labels + 1) % C, W, p=0.5, mask=mask.reshape(3 * B, H))["logits"].view(3, B, C)
    assert torch.equal(other, full)


def test_second_sample_of_a_workgroup_equals_the_same_row_alone(gpu):
    """259 samples on the kernel's 256 workgroups: workgroups 0..2 walk two samples each."""
    shape, pats = SHAPES[3], PATSETS[0]
    B, C = shape[0], shape[-1]
    x, x0, labels, W = case(shape)
    out = run(gpu, shape, pats, x, x0, labels, W)["logits"].view(3, B, C)
    tail = run(gpu, (3,) + shape[1:], pats, x[256:].clone(), x0, labels[256:], W)["logits"].view(3, 3, C)
    assert torch.equal(out[:, 256:], tail)


@pytest.mark.parametrize("bad_label", [10, -1, 1 << 40])
def test_out_of_range_label(gpu, bad_label):
    shape, pats = SHAPES[2], PATSETS[0]
    B, P = shape[0], len(pats)
    x, x0, labels, W = case(shape)
    good = run(gpu, shape, pats, x, x0, labels, W)
    bad_labels = labels.clone()
    bad_labels[4] = bad_label
    out = run(gpu, shape, pats, x, x0, bad_labels, W)   # (the guards: nothing written out of bounds either)
    assert torch.isnan(out["loss"]).all() and torch.isnan(out["stats"][0])
    assert torch.equal(out["logits"], good["logits"])
    # every gradient that the bad rows reach is NaN: fc5's wholly (dlogits is NaN on those rows), the others on every
    # unit whose ReLU is open on a bad row.  A unit closed on all of them gets an exact 0 from those rows (the ReLU
    # backward selects, it does not multiply) in both runs, and the other rows' terms are the good run's: bitwise equal
    assert torch.isnan(out["gw5"]).all() and torch.isnan(out["gb5"]).all()
    for g in ("gw3", "gb3", "gw0", "gb0"):
        assert torch.isnan(out[g]).any(), g
        fin = ~torch.isnan(out[g])
        assert torch.equal(out[g][fin], good[g][fin]), g
    # an out-of-range label never counts as correct
    keep_rows = (torch.arange(B) != 4).repeat(P)
    want = int((out["logits"].argmax(1) == labels.repeat(P))[keep_rows].sum())
    assert out["stats"][1].item() == want and out["stats"][2].item() == P * B
