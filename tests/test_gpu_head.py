"""tspm_head_train_step (ABI 16): the AVMNIST fusion head's forward, weighted cross-entropy and backward in
two launches, against a torch fp64 autograd reference of the same head (MML_Suite/models/avmnist.py:219-230,267;
experiment_utils/loss.py:98-148) fed the kernel's own dropout keep mask.

Bounds (fp32 kernel vs fp64 reference): per element |y - y64| <= 64 * 2^-23 * sum |w||x| style bounds are
awkward through the CE, so the head is held to rel-L2 <= 1e-5 on every output / gradient (the products have
K <= 192; ReLU decisions are forced by feeding the reference the kernel's own h1 > 0 / hh > 0 masks), the
loss to 1e-6 relative, and the keep mask bitwise to tspm_dropout_mask's bits for the same seed / counter."""
import ctypes

import pytest
import torch

import tspm_amd
from tspm_amd import _lib as L

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / max(b.norm().item(), 1e-30)).item()


def _buffers(n, F, H, H2, C, dev, seed):
    g = torch.Generator().manual_seed(seed)
    f = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dev)  # noqa: E731
    ws = dict(x=f(n, F), w0=f(H, F, scale=F ** -0.5), b0=f(H, scale=0.1), w3=f(H2, H, scale=H ** -0.5),
              b3=f(H2, scale=0.1), w5=f(C, H2, scale=H2 ** -0.5), b5=f(C, scale=0.1))
    ws["labels"] = torch.randint(0, C, (n,), generator=g).to(dev)
    z = lambda *s: torch.full(s, float("nan"), device=dev)  # noqa: E731  (every output must be written)
    out = dict(h1=z(n, H), hh=z(n, H2), logits=z(n, C), dlogits=z(n, C), dz3=z(n, H2), dz0=z(n, H), dx=z(n, F),
               row_ws=z(2 * n), gw0=z(H, F), gb0=z(H), gw3=z(H2, H), gb3=z(H2), gw5=z(C, H2), gb5=z(C),
               loss=z(1), stats=torch.zeros(4, device=dev))
    return ws, out


def _run(ws, out, p, weight, keep, gen_keep, seed=1234, counter=None):
    n, F = ws["x"].shape
    H, H2, C = ws["w0"].shape[0], ws["w3"].shape[0], ws["w5"].shape[0]
    d = L.HeadDesc(n=n, in_=F, hidden=H, hidden2=H2, classes=C, ldx=F, lddx=F, gen_keep=gen_keep,
                   p=p, loss_weight=weight, seed=seed, counter=None if counter is None else counter.data_ptr(),
                   keep=keep.data_ptr(), labels=ws["labels"].data_ptr(),
                   **{k: ws[k].data_ptr() for k in ("x", "w0", "b0", "w3", "b3", "w5", "b5")},
                   **{k: v.data_ptr() for k, v in out.items()})
    L.check(L.lib().tspm_head_train_step(ctypes.byref(d), torch.cuda.current_stream().cuda_stream), "head")
    torch.cuda.synchronize()


def _reference(ws, out, keep, p, weight):
    """fp64 autograd through the head with the kernel's ReLU decisions and keep mask."""
    d = {k: v.double().cpu().requires_grad_(k != "labels") for k, v in ws.items() if k != "labels"}
    scale = 1.0 / (1.0 - p) if p > 0 else 1.0
    m1 = (out["h1"].cpu() > 0).double()  # post-dropout > 0  <=>  pre-act > 0 and kept
    m2 = (out["hh"].cpu() > 0).double()
    z0 = d["x"] @ d["w0"].T + d["b0"]
    h1 = z0 * m1 * scale
    z3 = h1 @ d["w3"].T + d["b3"]
    hh = z3 * m2
    logits = hh @ d["w5"].T + d["b5"]
    loss = weight * torch.nn.functional.cross_entropy(logits, ws["labels"].cpu())
    loss.backward()
    return {"h1": h1, "hh": hh, "logits": logits, "loss": loss.reshape(1), "dx": d["x"].grad,
            "gw0": d["w0"].grad, "gb0": d["b0"].grad, "gw3": d["w3"].grad, "gb3": d["b3"].grad,
            "gw5": d["w5"].grad, "gb5": d["b5"].grad}


@pytest.mark.parametrize("n", [4, 13, 32, 128, 1024])
@pytest.mark.parametrize("p,gen", [(0.5, 1), (0.5, 0), (0.0, 0)])
def test_head_train_step_vs_fp64(gpu, n, p, gen):
    F, H, H2, C = 192, 128, 64, 10
    ws, out = _buffers(n, F, H, H2, C, gpu, seed=n)
    keep = (torch.rand(n, H, generator=torch.Generator().manual_seed(7)) > 0.5).to(torch.uint8).to(gpu)
    ctr = torch.tensor([37], dtype=torch.int64, device=gpu)
    _run(ws, out, p, 1.0, keep, gen, counter=ctr)
    if p > 0 and gen:
        ref_keep = torch.empty_like(keep)
        L.check(L.lib().tspm_dropout_mask(n * H, p, 1234, ctr.data_ptr(), ref_keep.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream), "mask")
        torch.cuda.synchronize()
        assert torch.equal(keep, ref_keep)
    r = _reference(ws, out, keep.cpu().double() if p > 0 else torch.ones(n, H, dtype=torch.float64), p, 1.0)
    if p > 0:  # dropped units are exactly 0
        assert bool(((keep == 0) <= (out["h1"] == 0)).all())
    for k in ("h1", "hh", "logits", "dx", "gw0", "gb0", "gw3", "gb3", "gw5", "gb5"):
        assert _rel(out[k], r[k]) < 1e-5, (k, _rel(out[k], r[k]))
    assert abs(out["loss"].item() - r["loss"].item()) <= 1e-6 * abs(r["loss"].item())
    st = out["stats"].cpu()
    assert st[2].item() == n
    correct = (out["logits"].argmax(1) == ws["labels"]).sum().item()
    assert st[1].item() == correct
    assert abs(st[0].item() - r["loss"].item() * n) <= 1e-5 * abs(r["loss"].item() * n)


def test_head_loss_weight_and_bad_label(gpu):
    F, H, H2, C, n = 192, 128, 64, 10, 32
    ws, out = _buffers(n, F, H, H2, C, gpu, seed=3)
    keep = torch.ones(n, H, dtype=torch.uint8, device=gpu)
    _run(ws, out, 0.0, 0.25, keep, 0)
    r = _reference(ws, out, None, 0.0, 0.25)
    assert abs(out["loss"].item() - r["loss"].item()) <= 1e-6 * abs(r["loss"].item())
    assert _rel(out["gw0"], r["gw0"]) < 1e-5
    ws["labels"][5] = 11  # out of range: NaN loss and gradients, no out-of-bounds read
    ws["labels"][6] = -1
    ws["b5"][0] = 100.0   # every row predicts class 0, the class the bounds-safe read falls back to
    _, out2 = _buffers(n, F, H, H2, C, gpu, seed=3)
    _run(ws, out2, 0.0, 1.0, keep, 0)
    assert torch.isnan(out2["loss"]).all() and torch.isnan(out2["dlogits"][5]).all()
    assert torch.isnan(out2["dlogits"][6]).all() and not torch.isnan(out2["dlogits"][7]).any()
    # stats[1] = #(argmax == label): a row whose label is out of range never counts, whatever its argmax
    assert bool((out2["logits"].argmax(1) == 0).all())
    st = out2["stats"].cpu()
    assert st[1].item() == float((ws["labels"] == 0).sum()) and st[2].item() == n


def test_head_invalid_shapes_refused(gpu):
    ws, out = _buffers(8, 190, 128, 64, 10, gpu, seed=1)  # in % 4 != 0
    keep = torch.ones(8, 128, dtype=torch.uint8, device=gpu)
    with pytest.raises(tspm_amd.TspmError):
        _run(ws, out, 0.0, 1.0, keep, 0)
