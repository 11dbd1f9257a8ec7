"""tspm_mono_head_step (classifier Linear forward, weighted cross-entropy, argmax(logits) and the Linear's whole
backward in one launch) alone against torch: the truth is fp64, the comparison reference fp32 torch, held to
tests/parity.py's §8(c) bounds (logits / loss rel-L2 <= 1e-4, gradients rel-L2 <= 1e-3 and cosine >= 0.9999, and
within 4x the fp32 reference's own error)."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from parity import check_grad, check_out
from tspm_amd import _lib as L

pytestmark = pytest.mark.gpu
CONFIGS = [(64, 3), (128, 10)]
SIZES = [1, 2, 63, 128, 257, 1024]


# rows the fp64 reference leaves out of the prediction check as near-ties, for exactly these seeds (computed on the CPU)
NEAR_TIES = {(64, 3): {257: 1, 1024: 2}, (128, 10): {1024: 4}}


def _inputs(n, hid, classes):
    """Drawn in this order from one seeded generator, in double, and rounded to fp32 once: those fp32 values are
    the inputs of the kernel and of both references."""
    g = torch.Generator().manual_seed(100 + n)
    f64 = dict(generator=g, dtype=torch.float64)
    emb = torch.randn(n, hid, **f64).float()
    w = ((torch.rand(classes, hid, **f64) * 2 - 1) / math.sqrt(hid)).float()
    b = ((torch.rand(classes, **f64) * 2 - 1) / math.sqrt(hid)).float()
    labels = torch.randint(0, classes, (n,), generator=g)
    return emb, w, b, labels


def _reference(emb, w, b, labels, lw, dtype):
    emb, w, b = (t.to(dtype).clone().requires_grad_(True) for t in (emb, w, b))
    logits = F.linear(emb, w, b)
    loss = lw * F.cross_entropy(logits, labels)
    loss.backward()
    return {"logits": logits.detach(), "loss": loss.detach().reshape(1), "dw": w.grad, "db": b.grad, "demb": emb.grad}


def _clear(logits64):
    """test_gpu_mono.py's rule: rows whose fp64 top-2 gap exceeds 1e-3 * max(|top|, 1)."""
    if logits64.shape[1] < 2:
        return torch.ones(logits64.shape[0], dtype=torch.bool)
    top2 = logits64.topk(2, dim=1).values
    return (top2[:, 0] - top2[:, 1]) > 1e-3 * top2[:, 0].abs().clamp_min(1)


def _run(dev, emb, w, b, labels, lw=1.0, train=True, ld_emb=None, ld_demb=None, stats=False):
    """One launch; returns the outputs on the host (+ the padded emb / demb buffers for the strided case)."""
    n, hid = emb.shape
    classes = w.shape[0]
    ld_emb, ld_demb = ld_emb or hid, ld_demb or hid
    nan = float("nan")
    emb_d = torch.full((n, ld_emb), nan, device=dev)
    emb_d[:, :hid] = emb.to(dev)
    demb_d = torch.full((n, ld_demb), nan, device=dev)
    w_d, b_d, lab_d = w.to(dev).contiguous(), b.to(dev).contiguous(), labels.to(dev)
    out = dict(logits=torch.full((n, classes), nan, device=dev), loss=torch.full((1,), nan, device=dev),
               preds=torch.full((n,), -7, dtype=torch.int64, device=dev),
               dw=torch.full((classes, hid), nan, device=dev), db=torch.full((classes,), nan, device=dev))
    st = torch.zeros(4, device=dev)
    d = L.MonoHeadDesc(n=n, hid=hid, classes=classes, ld_emb=ld_emb, ld_demb=ld_demb, loss_weight=lw)
    d.emb, d.w, d.b, d.labels = emb_d.data_ptr(), w_d.data_ptr(), b_d.data_ptr(), lab_d.data_ptr()
    d.logits, d.loss, d.preds = out["logits"].data_ptr(), out["loss"].data_ptr(), out["preds"].data_ptr()
    if train:
        d.dw, d.db, d.demb = out["dw"].data_ptr(), out["db"].data_ptr(), demb_d.data_ptr()
    if stats:
        d.stats = st.data_ptr()
    L.check(L.lib().tspm_mono_head_step(ctypes.byref(d), L.stream_handle()), "mono_head_step")
    torch.cuda.synchronize()
    res = {k: v.cpu() for k, v in out.items()}
    res.update(demb=demb_d[:, :hid].cpu(), emb_buf=emb_d.cpu(), demb_buf=demb_d.cpu(), stats=st.cpu())
    return res


_REFS = {}


def _refs(n, hid, classes, lw=1.0):
    key = (n, hid, classes, lw)
    if key not in _REFS:
        inp = _inputs(n, hid, classes)
        _REFS[key] = (inp, _reference(*inp, lw, torch.float32), _reference(*inp, lw, torch.float64))
    return _REFS[key]


def _check_values(o, r32, r64, n):
    for k in ("logits", "loss"):
        e = check_out(k, o[k], r32[k], r64[k])
        print(f"  {k}: rel-L2 {e:.2e}")
    for k in ("dw", "db", "demb"):
        e = check_grad(k, o[k], r32[k], r64[k])
        print(f"  {k}: rel-L2 {e:.2e}")
    clear = _clear(r64["logits"])
    excluded = int((~clear).sum())
    print(f"  preds: {excluded} of {n} rows excluded as near-ties")
    assert excluded <= (0 if n < 100 else n // 100)
    assert excluded == NEAR_TIES.get(tuple(r64["dw"].shape[::-1]), {}).get(n, 0)
    assert torch.equal(o["preds"][clear], r64["logits"].argmax(1)[clear])
    assert ((o["preds"] >= 0) & (o["preds"] < r64["logits"].shape[1])).all()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("hid,classes", CONFIGS)
def test_mono_head_vs_fp64(gpu, hid, classes, n):
    (emb, w, b, labels), r32, r64 = _refs(n, hid, classes)
    o = _run(gpu, emb, w, b, labels, stats=True)
    _check_values(o, r32, r64, n)
    # the three accumulators of tspm_cross_entropy: sum CE, #(argmax == label), n
    assert abs(o["stats"][0].item() - r64["loss"].item() * n) <= 1e-4 * abs(r64["loss"].item() * n) + 1e-6
    assert o["stats"][1].item() == float((o["preds"] == labels).sum()) and o["stats"][2].item() == float(n)


def test_mono_head_strided_rows_leave_the_padding_untouched(gpu):
    n, hid, classes = 257, 64, 3
    (emb, w, b, labels), r32, r64 = _refs(n, hid, classes)
    o = _run(gpu, emb, w, b, labels, ld_emb=hid + 8, ld_demb=hid + 4)
    _check_values(o, r32, r64, n)
    assert torch.isnan(o["emb_buf"][:, hid:]).all() and torch.equal(o["emb_buf"][:, :hid], emb)
    assert torch.isnan(o["demb_buf"][:, hid:]).all() and not torch.isnan(o["demb_buf"][:, :hid]).any()
    dense = _run(gpu, emb, w, b, labels)
    for k in ("logits", "loss", "preds", "dw", "db", "demb"):
        assert torch.equal(o[k], dense[k]), k


def test_mono_head_loss_weight(gpu):
    n, hid, classes = 128, 128, 10
    (emb, w, b, labels), r32, r64 = _refs(n, hid, classes, 0.5)
    _check_values(_run(gpu, emb, w, b, labels, lw=0.5), r32, r64, n)


@pytest.mark.parametrize("hid,classes,n", [(64, 3, 63), (128, 10, 257)])
def test_mono_head_forward_only_is_bitwise_the_training_forward(gpu, hid, classes, n):
    emb, w, b, labels = _inputs(n, hid, classes)
    tr, fw = _run(gpu, emb, w, b, labels), _run(gpu, emb, w, b, labels, train=False)
    for k in ("logits", "loss", "preds"):
        assert torch.equal(tr[k], fw[k]), k
    assert torch.isnan(fw["dw"]).all() and torch.isnan(fw["db"]).all() and torch.isnan(fw["demb_buf"]).all()


@pytest.mark.parametrize("hid,classes,n", [(64, 3, 128), (128, 10, 1024)])
def test_mono_head_is_deterministic(gpu, hid, classes, n):
    emb, w, b, labels = _inputs(n, hid, classes)
    a, c = _run(gpu, emb, w, b, labels), _run(gpu, emb, w, b, labels)
    for k in ("logits", "loss", "preds", "dw", "db", "demb"):
        assert torch.equal(a[k], c[k]), k


def test_mono_head_out_of_range_label_gives_nan(gpu):
    emb, w, b, labels = _inputs(63, 64, 3)
    labels = labels.clone()
    labels[17] = 3  # == classes
    labels[40] = -1
    emb = emb.clone()
    emb[17] = emb[40] = 50 * w[0]  # both rows predict class 0, the class the bounds-safe read falls back to
    o = _run(gpu, emb, w, b, labels, stats=True)
    assert torch.isnan(o["loss"]).all()
    assert torch.isnan(o["dw"]).any() and torch.isnan(o["db"]).any() and torch.isnan(o["demb"][17]).all()
    assert torch.isnan(o["demb"][40]).all()
    assert not torch.isnan(o["logits"]).any()
    # stats[1] = #(argmax == label): a row whose label is out of range never counts, whatever its argmax
    assert o["preds"][17].item() == 0 and o["preds"][40].item() == 0
    assert o["stats"][1].item() == float((o["preds"] == labels).sum()) and o["stats"][2].item() == 63.0
