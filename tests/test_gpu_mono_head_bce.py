"""tspm_mono_head_bce_step (classifier Linear forward, weighted BCEWithLogits, sigmoid(x) > threshold predictions, the
F1 accumulators and the Linear's whole backward in one launch) alone against torch: the truth is fp64, the comparison
reference fp32 torch on the same fp32-rounded inputs, held to tests/parity.py's bounds (logits / loss rel-L2 <= 1e-4,
gradients rel-L2 <= 1e-3 and cosine >= 0.9999, and within 4x the fp32 reference's own error).  This path has no ReLU,
max or dropout, so no decision is forced; a prediction is compared only where the fp64 logit is further than 1e-3
from the threshold.  Every output lives in a parity.Guarded allocation: a write past an extent fails the test."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from parity import GUARD, Guarded, check_grad, check_out
from tspm_amd import _lib as L

pytestmark = pytest.mark.gpu
CONFIGS = [(512, 23), (64, 5), (36, 1)]
SIZES = [1, 2, 63, 128, 257, 1024]
# elements the fp64 reference leaves out of the prediction check (|logit64| <= 1e-3), for exactly these seeds
# (computed on the CPU); 0 where not listed
NEAR_ZERO = {(512, 23): {63: 3, 128: 2, 257: 8, 1024: 19}, (64, 5): {63: 1, 257: 3, 1024: 11},
             (36, 1): {257: 1, 1024: 3}}
OUTS = ("logits", "loss", "preds", "dw", "db", "demb")


def _inputs(n, hid, classes):
    """Drawn in this order from one seeded generator, in double, and rounded to fp32 once: those fp32 values are
    the inputs of the kernel and of both references."""
    g = torch.Generator().manual_seed(200 + n)
    f64 = dict(generator=g, dtype=torch.float64)
    emb = torch.randn(n, hid, **f64).float()
    w = ((torch.rand(classes, hid, **f64) * 2 - 1) / math.sqrt(hid)).float()
    b = ((torch.rand(classes, **f64) * 2 - 1) / math.sqrt(hid)).float()
    targets = (torch.rand(n, classes, **f64) < 0.15).float()
    return emb, w, b, targets


def _reference(emb, w, b, targets, lw, dtype):
    emb, w, b = (t.to(dtype).clone().requires_grad_(True) for t in (emb, w, b))
    logits = F.linear(emb, w, b)
    loss = lw * F.binary_cross_entropy_with_logits(logits, targets.to(dtype))
    loss.backward()
    return {"logits": logits.detach(), "loss": loss.detach().reshape(1), "dw": w.grad, "db": b.grad, "demb": emb.grad}


_REFS = {}


def _refs(n, hid, classes, lw=1.0):
    key = (n, hid, classes, lw)
    if key not in _REFS:
        inp = _inputs(n, hid, classes)
        _REFS[key] = (inp, _reference(*inp, lw, torch.float32), _reference(*inp, lw, torch.float64))
    return _REFS[key]


class _Call:
    """The device buffers of one descriptor: inputs (emb rows padded with NaN to ld_emb), Guarded outputs, the
    zeroed workspace followed by a guard, and the stats accumulators (zero, then accumulated into)."""

    def __init__(self, dev, emb, w, b, targets, lw=1.0, thr=0.5, train=True, ld_emb=None, ld_demb=None, dims=None,
                 only=None, ws=None):
        n, hid = emb.shape
        classes = w.shape[0]
        self.n, self.hid, self.classes = n, hid, classes
        ld_emb, ld_demb = ld_emb or hid, ld_demb or hid
        self.emb_d = torch.full((n, ld_emb), float("nan"), device=dev)
        self.emb_d[:, :hid] = emb.to(dev)
        self.ins = [w.to(dev).contiguous(), b.to(dev).contiguous(), targets.to(dev).contiguous()]
        self.out = dict(logits=Guarded(dev, n, classes), loss=Guarded(dev, 1, 1),
                        preds=Guarded(dev, n, classes, dtype=torch.uint8), dw=Guarded(dev, classes, hid),
                        db=Guarded(dev, 1, classes), demb=Guarded(dev, n, hid, ld_demb),
                        stats=Guarded(dev, 1, 3 + 3 * classes))
        self.out["stats"].t.zero_()
        d = L.MonoHeadBceDesc(n=n, hid=hid, classes=classes, ld_emb=ld_emb, ld_demb=ld_demb, loss_weight=lw,
                              threshold=thr)
        for k, v in (dims or {}).items():  # the descriptor's claim, for the refusal tests (the buffers stay as built)
            setattr(d, k, v)
        wsb = int(L.lib().tspm_mono_head_bce_workspace(n, hid, classes))
        if ws is None:
            ws = torch.zeros(wsb // 4 + GUARD, device=dev)
            ws[wsb // 4:] = float("inf")
        self.ws = ws
        self.ws_floats = wsb // 4
        d.emb, d.w, d.b, d.targets = self.emb_d.data_ptr(), *(t.data_ptr() for t in self.ins)
        d.logits, d.loss, d.preds = (self.out[k].ptr() for k in ("logits", "loss", "preds"))
        d.stats, d.workspace, d.workspace_bytes = self.out["stats"].ptr(), self.ws.data_ptr(), wsb
        for k in (("dw", "db", "demb") if train else ()) if only is None else only:
            setattr(d, k, self.out[k].ptr())
        self.d = d

    def launch(self) -> int:
        status = L.lib().tspm_mono_head_bce_step(ctypes.byref(self.d), L.stream_handle())
        torch.cuda.synchronize()
        return status

    def result(self, written=OUTS + ("stats",)):
        for k in written:
            self.out[k].intact(k)
        assert bool(torch.isinf(self.ws[self.ws_floats:]).all()), "wrote past the workspace"
        res = {k: self.out[k].cpu() for k in written}
        for k in ("loss", "db", "stats"):
            if k in res:
                res[k] = res[k].reshape(-1)
        res["emb_buf"] = self.emb_d.cpu()
        return res

    def untouched(self, k) -> bool:
        g = self.out[k]
        bits = g.flat.cpu().view(torch.int32 if g.flat.dtype == torch.float32 else torch.uint8)
        return bool((bits == (0x7FA5A5A5 if g.flat.dtype == torch.float32 else 0xA5)).all())


def _run(dev, emb, w, b, targets, **kw):
    c = _Call(dev, emb, w, b, targets, **kw)
    L.check(c.launch(), "mono_head_bce_step")
    train = kw.get("train", True)
    res = c.result(OUTS + ("stats",) if train else ("logits", "loss", "preds", "stats"))
    res["call"] = c
    return res


def _counts_from_preds(preds, targets):
    """oracle.mmimdb_ref.f1_counts restated on the kernel's own predictions: (sum of per-sample F1, [tp, fp, fn] x c)."""
    p, y = preds.bool(), targets > 0.5
    tp, fp, fn = (p & y).sum(1), (p & ~y).sum(1), (~p & y).sum(1)
    den = 2 * tp + fp + fn
    f1 = torch.where(den > 0, 2 * tp.double() / den.clamp(min=1), torch.zeros_like(den, dtype=torch.double))
    per_class = torch.stack([(p & y).sum(0), (p & ~y).sum(0), (~p & y).sum(0)], 1).reshape(-1).float()
    return float(f1.sum()), per_class


def _check_values(o, r32, r64, targets, n, hid, classes, thr=0.5, lw=1.0, pinned=True, launches=1):
    for k in ("logits", "loss"):
        e = check_out(k, o[k], r32[k], r64[k])
        print(f"  {k}: rel-L2 {e:.2e}")
    for k in ("dw", "db", "demb"):
        e = check_grad(k, o[k], r32[k], r64[k])
        print(f"  {k}: rel-L2 {e:.2e}")
    cut = math.log(thr / (1 - thr))  # sigmoid(x) > thr  <=>  x > logit(thr)
    clear = (r64["logits"] - cut).abs() > 1e-3
    excluded = int((~clear).sum())
    print(f"  preds: {excluded} of {n * classes} elements excluded as within 1e-3 of the threshold")
    assert excluded <= (0 if n * classes < 100 else n * classes // 100)
    if pinned:
        assert excluded == NEAR_ZERO.get((hid, classes), {}).get(n, 0)
    assert torch.equal(o["preds"].bool()[clear], (r64["logits"] > cut)[clear])
    assert bool((o["preds"] <= 1).all())
    # stats: tspm_bce_logits' layout, from the kernel's own predictions
    f1, per_class = _counts_from_preds(o["preds"], targets)
    st = o["stats"].double()
    assert torch.equal(o["stats"][3:], per_class * launches) and st[1].item() == float(n * launches)
    want_loss = r64["loss"].item() * n * launches
    assert abs(st[0].item() - want_loss) <= 1e-4 * abs(want_loss)
    assert abs(st[2].item() - f1 * launches) <= 1e-5 * abs(f1 * launches)
    print(f"  stats: loss sum {st[0].item():.6f} (fp64 {want_loss:.6f}), F1 sum {st[2].item():.6f} ({f1:.6f})")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("hid,classes", CONFIGS)
def test_mono_head_bce_vs_fp64(gpu, hid, classes, n):
    (emb, w, b, t), r32, r64 = _refs(n, hid, classes)
    if n >= 128:
        assert bool((t.sum(1) == 0).any()), "these inputs include all-zero target rows (zero_division = 0)"
    _check_values(_run(gpu, emb, w, b, t), r32, r64, t, n, hid, classes)


def test_mono_head_bce_strided_rows_leave_the_padding_untouched(gpu):
    n, hid, classes = 257, 512, 23
    (emb, w, b, t), r32, r64 = _refs(n, hid, classes)
    o = _run(gpu, emb, w, b, t, ld_emb=hid + 8, ld_demb=hid + 4)  # Guarded checks demb's padding columns
    _check_values(o, r32, r64, t, n, hid, classes)
    assert torch.isnan(o["emb_buf"][:, hid:]).all() and torch.equal(o["emb_buf"][:, :hid], emb)
    dense = _run(gpu, emb, w, b, t)
    for k in OUTS + ("stats",):
        assert torch.equal(o[k], dense[k]), k


def test_mono_head_bce_loss_weight_and_threshold(gpu):
    n, hid, classes = 128, 512, 23
    (emb, w, b, t), r32, r64 = _refs(n, hid, classes, 0.5)
    _check_values(_run(gpu, emb, w, b, t, lw=0.5, thr=0.3), r32, r64, t, n, hid, classes, thr=0.3, lw=0.5,
                  pinned=False)


@pytest.mark.parametrize("hid,classes,n", [(64, 5, 63), (512, 23, 257)])
def test_mono_head_bce_forward_only_is_bitwise_the_training_forward(gpu, hid, classes, n):
    emb, w, b, t = _inputs(n, hid, classes)
    tr, fw = _run(gpu, emb, w, b, t), _run(gpu, emb, w, b, t, train=False)
    for k in ("logits", "loss", "preds", "stats"):
        assert torch.equal(tr[k], fw[k]), k
    assert all(fw["call"].untouched(k) for k in ("dw", "db", "demb"))


@pytest.mark.parametrize("hid,classes,n", [(512, 23, 1024), (64, 5, 128)])
def test_mono_head_bce_is_deterministic(gpu, hid, classes, n):
    emb, w, b, t = _inputs(n, hid, classes)
    a, c = _run(gpu, emb, w, b, t), _run(gpu, emb, w, b, t)
    for k in OUTS + ("stats",):
        assert torch.equal(a[k], c[k]), k
    # a second launch on the same workspace (the re-armed arrival counter) gives the same outputs again
    L.check(a["call"].launch(), "second launch")
    again = a["call"].result()
    for k in OUTS:
        assert torch.equal(again[k], a[k]), k


def test_mono_head_bce_workspace_reused_with_other_data(gpu):
    """The partial sums a launch leaves in the workspace never reach the next launch's outputs (the last arriver
    reads what THIS launch's workgroups published, also when its caches hold the previous launch's records)."""
    n, hid, classes = 257, 512, 23
    emb, w, b, t = _inputs(n, hid, classes)
    first = _run(gpu, emb, w, b, t)
    emb2, t2 = (0.5 * emb.flip(0)).contiguous(), t.flip(0).contiguous()
    c = _Call(gpu, emb2, w, b, t2, ws=first["call"].ws)
    L.check(c.launch(), "second launch, other data")
    again, fresh = c.result(), _run(gpu, emb2, w, b, t2)
    for k in OUTS + ("stats",):
        assert torch.equal(again[k], fresh[k]), k
    assert not torch.equal(again["dw"], first["dw"])


def test_mono_head_bce_stats_accumulate_over_launches(gpu):
    n, hid, classes = 63, 64, 5
    (emb, w, b, t), r32, r64 = _refs(n, hid, classes)
    c = _Call(gpu, emb, w, b, t)
    L.check(c.launch(), "first launch")
    L.check(c.launch(), "second launch")
    _check_values(c.result(), r32, r64, t, n, hid, classes, launches=2)


@pytest.mark.parametrize("bad", [dict(dims=dict(hid=516, ld_emb=516, ld_demb=516)), dict(dims=dict(hid=30)),
                                 dict(dims=dict(classes=33)), dict(dims=dict(n=1025)), dict(only=("dw",)),
                                 dict(only=("db",)), dict(only=("demb",))])
def test_mono_head_bce_refuses_bad_descriptors_with_nothing_written(gpu, bad):
    emb, w, b, t = _inputs(16, 64, 5)
    c = _Call(gpu, emb, w, b, t, **bad)
    assert c.launch() == 1, bad  # TSPM_ERR_INVALID
    assert all(c.untouched(k) for k in OUTS)
    assert not c.out["stats"].t.any() and not c.ws[:c.ws_floats].any()
