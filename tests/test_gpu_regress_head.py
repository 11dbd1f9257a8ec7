"""tspm_regress_head_step (Linear(hid, 1), weighted L1 / MSE against float32 labels, the Linear's whole backward, the
per-group epoch accumulators and the loss log in one launch) alone against torch: the truth is fp64 autograd, the
yardstick the fp32 run of the same restatement, held to tests/parity.py's op_check bounds (err_ours <= 4 x err_ref32
+ floor; gradients also cosine >= 0.9999).

L1's gradient is a decision (sign(e)): the fp64 reference takes it from the kernel's own fp32 residual (the project's
forced-decision rule), and every case first asserts that no row of the fp64 reference has |e| < 1e-4, so no decision
is close.  Labels are drawn on the 0.2 grid of the real data; the seeds below were checked for that on the CPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

from parity import Guarded, Ratios, op_check
from tspm_amd import _lib as L
from tspm_amd import msa_metrics as MM
from tspm_amd.metrics import regress_records

pytestmark = pytest.mark.gpu
CHUNK = 64  # the kernel's row chunk
HIDS = [4, 32, 48, 64, 128]
SIZES = [1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 128, 257, 1024]
KINDS = {"l1": L.REGRESS_L1, "mse": L.REGRESS_MSE}
MIN_RESIDUAL = 1e-4
SEED_BUMP = {}  # (n, hid) -> extra seed offset where the first draw has a residual within MIN_RESIDUAL of zero
RATIOS = Ratios()


def _inputs(n, hid):
    """Drawn in this order from one seeded generator, in double, and rounded to fp32 once: those fp32 values are the
    inputs of the kernel and of both references."""
    g = torch.Generator().manual_seed(1000 + 131 * n + hid + SEED_BUMP.get((n, hid), 0))
    f64 = dict(generator=g, dtype=torch.float64)
    emb = torch.randn(n, hid, **f64).float()
    w = ((torch.rand(1, hid, **f64) * 2 - 1) * 2 / math.sqrt(hid)).float()
    b = ((torch.rand(1, **f64) * 2 - 1) / math.sqrt(hid)).float()
    labels = (torch.randint(-15, 16, (n,), generator=g).double() / 5).float()
    return emb, w, b, labels


def _reference(emb, w, b, labels, kind, lw, dtype, sign=None):
    """loss = lw * mean l(e) by autograd; L1 with the decision forced: |e| = sign * e where sign is given."""
    emb, w, b = (t.to(dtype).clone().requires_grad_(True) for t in (emb, w, b))
    pred = torch.nn.functional.linear(emb, w, b).reshape(-1)
    e = pred - labels.to(dtype)
    if kind == L.REGRESS_L1:
        s = torch.sign(e.detach()) if sign is None else sign.to(dtype)
        loss = lw * (s * e).mean()
    else:
        loss = lw * (e * e).mean()
    loss.backward()
    return {"pred": pred.detach(), "loss": loss.detach().reshape(1), "dw": w.grad, "db": b.grad, "demb": emb.grad,
            "e": e.detach()}


def _run(dev, emb, w, b, labels, kind, lw=1.0, train=True, ld_emb=None, ld_demb=None, groups=None, stats=None,
         log=None):
    """One launch with every output in a Guarded allocation; returns the outputs on the host."""
    n, hid = emb.shape
    ld_emb, ld_demb = ld_emb or hid, ld_demb or hid
    emb_d = torch.full((n, ld_emb), float("nan"), device=dev)
    emb_d[:, :hid] = emb.to(dev)
    w_d, b_d, lab_d = w.to(dev).contiguous(), b.to(dev).contiguous(), labels.to(dev).contiguous()
    out = dict(pred=Guarded(dev, n, 1), loss=Guarded(dev, 1, 1), dw=Guarded(dev, 1, hid), db=Guarded(dev, 1, 1),
               demb=Guarded(dev, n, hid, ld_demb))
    d = L.RegressHeadDesc(n=n, hid=hid, ld_emb=ld_emb, ld_demb=ld_demb, kind=kind, n_groups=1, loss_weight=lw)
    d.emb, d.w, d.b, d.labels = emb_d.data_ptr(), w_d.data_ptr(), b_d.data_ptr(), lab_d.data_ptr()
    d.pred, d.loss = out["pred"].ptr(), out["loss"].ptr()
    if train:
        d.dw, d.db, d.demb = out["dw"].ptr(), out["db"].ptr(), out["demb"].ptr()
    if stats is not None:
        d.stats, d.n_groups = stats.ptr(), stats.rows
        if groups is not None:
            g_d = groups.to(dev)
            d.groups = g_d.data_ptr()
    if log is not None:
        d.loss_log, d.counters, d.log_capacity = log["loss_log"].ptr(), log["counters"].ptr(), log["loss_log"].width
    L.check(L.lib().tspm_regress_head_step(ctypes.byref(d), L.stream_handle()), "regress_head_step")
    torch.cuda.synchronize()
    for k, gd in out.items():
        gd.intact(k)
    res = {k: gd.cpu() for k, gd in out.items()}
    res["pred"], res["loss"], res["db"] = res["pred"].reshape(-1), res["loss"].reshape(-1), res["db"].reshape(-1)
    res["written"] = {k: not bool(torch.isnan(v).all()) for k, v in res.items()}
    assert torch.equal(emb_d[:, :hid].cpu(), emb) and bool(torch.isnan(emb_d[:, hid:]).all())  # the input untouched
    return res


def _check(o, emb, w, b, labels, kind, lw, tag):
    r64 = _reference(emb, w, b, labels, kind, lw, torch.float64)
    if kind == L.REGRESS_L1:  # no close decision, then the kernel's own signs forced into both references
        assert float(r64["e"].abs().min()) >= MIN_RESIDUAL, f"{tag}: a residual within {MIN_RESIDUAL} of zero"
        sign = torch.sign(o["pred"] - labels)
        assert torch.equal(sign.double(), torch.sign(r64["e"]))
        r64 = _reference(emb, w, b, labels, kind, lw, torch.float64, sign)
        r32 = _reference(emb, w, b, labels, kind, lw, torch.float32, sign)
    else:
        r32 = _reference(emb, w, b, labels, kind, lw, torch.float32)
    for k in ("pred", "loss"):
        op_check(f"{k}[{tag}]", o[k], r32[k], r64[k], ratios=RATIOS)
    for k in ("dw", "db", "demb"):
        op_check(f"{k}[{tag}]", o[k].reshape(r64[k].shape), r32[k], r64[k], grad=True, ratios=RATIOS)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("hid", HIDS)
def test_regress_head_vs_fp64(gpu, hid, n, kind):
    emb, w, b, labels = _inputs(n, hid)
    o = _run(gpu, emb, w, b, labels, KINDS[kind])
    _check(o, emb, w, b, labels, KINDS[kind], 1.0, f"{kind} n={n} hid={hid}")
    print(RATIOS)


@pytest.mark.parametrize("kind", list(KINDS))
def test_regress_head_strided_rows_leave_the_padding_untouched(gpu, kind):
    n, hid = 257, 48
    emb, w, b, labels = _inputs(n, hid)
    o = _run(gpu, emb, w, b, labels, KINDS[kind], ld_emb=hid + 8, ld_demb=hid + 4)  # _run: guards and NaN padding
    _check(o, emb, w, b, labels, KINDS[kind], 1.0, f"{kind} strided")
    dense = _run(gpu, emb, w, b, labels, KINDS[kind])
    for k in ("pred", "loss", "dw", "db", "demb"):
        assert torch.equal(o[k], dense[k]), k


@pytest.mark.parametrize("kind", list(KINDS))
def test_regress_head_loss_weight(gpu, kind):
    emb, w, b, labels = _inputs(128, 32)
    _check(_run(gpu, emb, w, b, labels, KINDS[kind], lw=0.5), emb, w, b, labels, KINDS[kind], 0.5, f"{kind} lw=0.5")


@pytest.mark.parametrize("kind,hid,n", [("l1", 32, CHUNK - 1), ("mse", 128, 257)])
def test_regress_head_forward_only_is_bitwise_the_training_forward(gpu, kind, hid, n):
    emb, w, b, labels = _inputs(n, hid)
    tr, fw = _run(gpu, emb, w, b, labels, KINDS[kind]), _run(gpu, emb, w, b, labels, KINDS[kind], train=False)
    for k in ("pred", "loss"):
        assert torch.equal(tr[k], fw[k]), k
    assert not fw["written"]["dw"] and not fw["written"]["db"] and not fw["written"]["demb"]


@pytest.mark.parametrize("kind,hid,n", [("l1", 64, 128), ("mse", 48, 1024)])
def test_regress_head_is_deterministic(gpu, kind, hid, n):
    emb, w, b, labels = _inputs(n, hid)
    a, c = _run(gpu, emb, w, b, labels, KINDS[kind]), _run(gpu, emb, w, b, labels, KINDS[kind])
    for k in ("pred", "loss", "dw", "db", "demb"):
        assert torch.equal(a[k], c[k]), k


def test_l1_sign_of_zero_is_zero(gpu):
    """A row whose prediction equals its label exactly: gradient 0 from that row, as torch's sign(0)."""
    emb = torch.eye(4)
    w, b = torch.tensor([[0.0, 0.5, -2.5, 3.5]]), torch.zeros(1)
    labels = torch.tensor([0.0, 0.5, 1.0, -1.0])  # rows 0, 1: e == 0; row 2: e < 0; row 3: e > 0
    o = _run(gpu, emb, w, b, labels, L.REGRESS_L1)
    assert torch.equal(o["pred"], w.reshape(-1))
    assert torch.equal(o["dw"].reshape(-1), torch.tensor([0.0, 0.0, -0.25, 0.25])) and o["db"].item() == 0.0
    assert o["loss"].item() == (3.5 + 4.5) / 4


def _stats(dev, groups):
    st = Guarded(dev, groups, L.REGRESS_STATS_WORDS, dtype=torch.int64)
    st.t.zero_()
    return st


def _expected_records(calls, groups):
    """numpy on the kernel's own fp32 predictions: one record per group over every call's rows."""
    recs = []
    for g in range(groups):
        p = np.concatenate([o["pred"].numpy()[gr.numpy() == g] for o, _, gr in calls])
        y = np.concatenate([lab.numpy()[gr.numpy() == g] for _, lab, gr in calls])
        recs.append(MM.regression_record(p, y))
    return recs


def _assert_records(got, want):
    for g, (a, e) in enumerate(zip(got, want)):
        assert a["n"] == e["n"], g
        assert np.array_equal(a["conf7"], e["conf7"]) and np.array_equal(a["sign3"], e["sign3"]), g
        for k in ("sum_abs", "sum_sq", "sum_p", "sum_y", "sum_pp", "sum_yy", "sum_py"):
            print(f"  group {g} {k}: {a[k]!r} vs {e[k]!r}")
            assert abs(a[k] - e[k]) <= 1e-8 * abs(e[k]), (g, k, a[k], e[k])


def test_accumulators_over_three_calls_and_four_groups(gpu):
    """Three calls add into one [4] record buffer: crafted rows with exact predictions 0, 0.5, -2.5, 3.5 (the
    half-to-even cells, both signs of zero, the clip), then two random batches with groups 0..3 and rows whose group
    is out of range.  The int64 fields equal numpy on the kernel's own fp32 predictions exactly; the double sums
    agree to 1e-8 relative (at most 3 * 1024 terms at 2^-53 each; inputs of mean ~0 and spread ~1 cost Pearson's
    cancellation under a factor 10).  The loss log and counters behave as tspm_classify_update's."""
    G = 4
    st = _stats(gpu, G)
    log = {"loss_log": Guarded(gpu, 1, 2), "counters": Guarded(gpu, 1, 2, dtype=torch.int64)}
    log["counters"].t.zero_()
    calls, losses = [], []
    # crafted: hid 4, one-hot embeddings, zero bias
    idx = torch.tensor([0, 1, 2, 3, 0, 1, 2, 3, 1, 2])
    emb, w, b = torch.eye(4)[idx], torch.tensor([[0.0, 0.5, -2.5, 3.5]]), torch.zeros(1)
    labels = torch.tensor([0.0, 0.5, -2.5, 3.5, -0.0, 1.5, -1.5, -3.2, -0.5, 2.5])
    groups = torch.tensor([0, 1, 2, 3, 3, 2, 1, 0, 0, 1], dtype=torch.int32)
    o = _run(gpu, emb, w, b, labels, L.REGRESS_L1, groups=groups, stats=st, log=log)
    assert torch.equal(o["pred"], w.reshape(-1)[idx])
    calls.append((o, labels, groups))
    losses.append(o["loss"].item())
    for n, hid, kind in ((257, 32, L.REGRESS_MSE), (1024, 48, L.REGRESS_L1)):
        emb, w, b, labels = _inputs(n, hid)
        groups = torch.randint(0, G, (n,), generator=torch.Generator().manual_seed(n), dtype=torch.int32)
        groups[5], groups[n - 2] = G, -1  # out of range: left out of every accumulator
        o = _run(gpu, emb, w, b, labels, kind, groups=groups, stats=st, log=log)
        calls.append((o, labels, groups))
        losses.append(o["loss"].item())
    st.intact("stats")
    got = regress_records(st.cpu().numpy())
    want = _expected_records(calls, G)
    assert sum(r["n"] for r in got) == 10 + 257 + 1024 - 4
    _assert_records(got, want)
    # conf7 really saw the half-to-even cells: p = 0.5 -> 0, -2.5 -> -2, 3.5 -> 3 (clipped), y = 1.5 -> 2, -0.5 -> -0
    crafted = MM.regression_record(calls[0][0]["pred"].numpy(), calls[0][1].numpy())
    assert crafted["conf7"][3, 3] == 4 and crafted["conf7"][5, 3] == 1 and crafted["conf7"][1, 1] == 2
    assert crafted["sign3"][1, 1] == 2  # y = +0 and -0 against p = 0
    # loss log: capacity 2 keeps the first two losses, the counters still count every call
    log["loss_log"].intact("loss_log")
    log["counters"].intact("counters")
    assert log["loss_log"].cpu().reshape(-1).tolist() == losses[:2]
    assert log["counters"].cpu().reshape(-1).tolist() == [3, 10 + 257 + 1024]
    # the same three calls into a fresh buffer add the same bits
    st2 = _stats(gpu, G)
    for (o, labels, groups), (n, hid, kind) in zip(calls, ((10, 4, L.REGRESS_L1), (257, 32, L.REGRESS_MSE),
                                                           (1024, 48, L.REGRESS_L1))):
        if hid == 4:
            e2, w2, b2 = torch.eye(4)[idx], torch.tensor([[0.0, 0.5, -2.5, 3.5]]), torch.zeros(1)
        else:
            e2, w2, b2, _ = _inputs(n, hid)
        _run(gpu, e2, w2, b2, labels, kind, groups=groups, stats=st2)
    assert torch.equal(st.cpu(), st2.cpu())


def test_groups_default_to_zero_and_stats_are_optional(gpu):
    emb, w, b, labels = _inputs(128, 64)
    st = _stats(gpu, 1)
    o = _run(gpu, emb, w, b, labels, L.REGRESS_L1, stats=st, train=False)
    _assert_records(regress_records(st.cpu().numpy()), [MM.regression_record(o["pred"].numpy(), labels.numpy())])
    plain = _run(gpu, emb, w, b, labels, L.REGRESS_L1, train=False)
    assert torch.equal(plain["pred"], o["pred"]) and torch.equal(plain["loss"], o["loss"])


@pytest.mark.parametrize("kind", list(KINDS))
def test_nan_label_gives_nan_loss_and_is_left_out_of_the_accumulators(gpu, kind):
    n, hid = CHUNK + 1, 32
    emb, w, b, labels = _inputs(n, hid)
    labels = labels.clone()
    labels[17] = float("nan")
    st = _stats(gpu, 1)
    o = _run(gpu, emb, w, b, labels, KINDS[kind], stats=st)
    assert torch.isnan(o["loss"]).all() and torch.isnan(o["dw"]).all() and torch.isnan(o["db"]).all()
    assert torch.isnan(o["demb"][17]).all() and not torch.isnan(o["pred"]).any()
    keep = torch.arange(n) != 17
    assert not torch.isnan(o["demb"][keep]).any()
    got = regress_records(st.cpu().numpy())
    assert got[0]["n"] == n - 1
    _assert_records(got, [MM.regression_record(o["pred"][keep].numpy(), labels[keep].numpy())])
