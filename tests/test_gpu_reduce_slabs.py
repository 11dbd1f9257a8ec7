"""tspm_reduce_slabs called directly (csrc/conv.hip: k_reduce_slabs and k_reduce_slabs_wide, the sums behind the
split weight gradients) against an fp32 CPU emulation of the documented order, bit for bit, and the argmax
conventions of tspm_classify_update_ex (csrc/metrics.hip) on rows built to tell them apart."""
import pytest
import torch

import op_refs as R
from parity import Guarded
from tspm_amd import _lib as L

pytestmark = pytest.mark.gpu
OK, INVALID = 0, 1
ARGMAX_SOFTMAX, ARGMAX_LOGITS = 0, 1  # TSPM_ARGMAX_*


def _sync():
    torch.cuda.synchronize()


def _slabs(count, nslab, stride, seed):
    """[nslab, count] fp32 and the same values laid out `stride` apart in a buffer whose other elements are 1e30.
    The slabs of one element share a magnitude (it varies from element to element): every add then rounds, so another
    order of the adds shows in the low bits (exchanging two neighbouring partial sums changes 5-30 % of the
    elements, the narrow order against the wide one 75 %); slabs of mixed magnitudes hid an exchange of two small
    ones."""
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(nslab, count, generator=g) * 10.0 ** torch.randint(-2, 3, (1, count), generator=g).float()
    return s, R.padded(s, stride)


@pytest.mark.parametrize("count,nslab,stride", [
    (7, 3, 8),          # narrow: one float4 + a 3-element scalar tail
    (1203, 5, 1204),    # narrow: 4*300 + 3, more than one workgroup's worth of float4s
    (1203, 5, 1216),    # ... with slab_stride > count + 3
    (3136, 64, 3136),   # wide: the 7x7 stem weight gradient (64 x 49 floats over 64 slabs)
    (50, 15, 52),       # narrow: one slab short of the wide kernel
    (50, 16, 52),       # wide: every group exactly two slabs, the 4-slab loop never runs
    (50, 17, 64),       # wide: group 0 has a third slab
    (50, 37, 52),       # wide: groups 0-4 run the 4-slab loop once + one more, groups 5-7 the single loop 4 times
    (1, 1, 1),          # narrow: one element, one slab, stride 1 (allowed: nslab = 1)
    (3, 16, 4),         # wide: fewer elements than one workgroup's 32
])
def test_reduce_slabs_bitwise_order(gpu, count, nslab, stride):
    slabs, flat = _slabs(count, nslab, stride, 1000 * nslab + count)
    wide = R.reduce_slabs_is_wide(count, nslab)
    want = R.reduce_slabs_emul(slabs, wide)
    sd = flat.to(gpu)
    out = Guarded(gpu, 1, count)
    L.check(L.lib().tspm_reduce_slabs(count, nslab, stride, sd.data_ptr(), out.ptr(), L.stream_handle()), "reduce_slabs")
    _sync()
    out.intact("reduce_slabs out")
    got = out.cpu().view(-1)
    R.check(f"reduce_slabs.fp64[{count}x{nslab}]", got, slabs.double().sum(0), R.reduce_slabs_tol(slabs))
    bad = got.view(torch.int32) != want.view(torch.int32)
    assert not bool(bad.any()), f"{int(bad.sum())} of {count} elements differ from the documented {'wide' if wide else 'narrow'} " \
                                f"order; first at {int(bad.nonzero()[0])}"


def test_reduce_slabs_refusals(gpu):
    buf = torch.zeros(4 * 64 + 8, device=gpu)
    out = Guarded(gpu, 1, 64)
    lib, sh = L.lib(), L.stream_handle()
    assert lib.tspm_reduce_slabs(16, 4, 64, buf.data_ptr() + 4, out.ptr(), sh) == INVALID   # slabs not 16-byte aligned
    assert lib.tspm_reduce_slabs(16, 4, 64, buf.data_ptr(), out.ptr() + 8, sh) == INVALID   # out not 16-byte aligned
    assert lib.tspm_reduce_slabs(16, 4, 62, buf.data_ptr(), out.ptr(), sh) == INVALID       # stride % 4 with nslab > 1
    assert lib.tspm_reduce_slabs(16, 0, 64, buf.data_ptr(), out.ptr(), sh) == INVALID       # nslab = 0
    assert lib.tspm_reduce_slabs(-1, 4, 64, buf.data_ptr(), out.ptr(), sh) == INVALID
    assert lib.tspm_reduce_slabs(16, 4, 64, None, out.ptr(), sh) == INVALID
    assert lib.tspm_reduce_slabs(0, 4, 64, buf.data_ptr(), out.ptr(), sh) == OK             # nothing to do
    _sync()
    out.intact("refused reduce_slabs")
    assert bool(out.cpu().isnan().all())


# ------------------------------------------------------------------------------------------------
# tspm_classify_update_ex
# ------------------------------------------------------------------------------------------------
def _classify(gpu, logits, labels, groups, n_groups, argmax_of, conf=None):
    n, k = logits.shape
    zd, ld = logits.to(gpu), labels.to(gpu)
    gd = groups.to(gpu) if groups is not None else None
    if conf is None:
        conf = Guarded(gpu, 1, n_groups * k * k, dtype=torch.int64)
        conf.t.zero_()
    pred = Guarded(gpu, 1, n, dtype=torch.int64)
    L.check(L.lib().tspm_classify_update_ex(n, k, zd.data_ptr(), ld.data_ptr(), L.ptr(gd), n_groups, conf.ptr(), pred.ptr(),
                                            None, None, None, 0, argmax_of, L.stream_handle()), "classify_update_ex")
    _sync()
    conf.intact("confusion"); pred.intact("pred_out")
    return pred.cpu().view(-1), conf


def _count(pred, labels, groups, n_groups, k):
    conf = torch.zeros(n_groups, k, k, dtype=torch.int64)
    for r in range(pred.numel()):
        g = int(groups[r]) if groups is not None else 0
        if 0 <= int(labels[r]) < k and 0 <= g < n_groups:
            conf[g, int(labels[r]), int(pred[r])] += 1
    return conf


def test_classify_update_ex_softmax_ties(gpu):
    """Two logits 1 ulp apart with the same fp32 probability: the softmax convention picks the first of them, the
    logits convention the larger."""
    z, first, larger = R.softmax_tie_rows()
    labels = torch.tensor([1, 4, 1, 0])
    for mode, want in ((ARGMAX_SOFTMAX, first), (ARGMAX_LOGITS, larger)):
        pred, conf = _classify(gpu, z, labels, None, 1, mode)
        assert torch.equal(pred, want), f"argmax_of {mode}: {pred.tolist()} != {want.tolist()}"
        assert torch.equal(conf.cpu().view(1, 5, 5), _count(want, labels, None, 1, 5))
    assert not torch.equal(first, larger)


@pytest.mark.parametrize("n,k", [(1, 2), (300, 10), (257, 3)])
def test_classify_update_ex_ordinary_rows(gpu, n, k):
    """On ordinary rows both conventions are torch.argmax; the confusion matrix (with groups, an out-of-range label
    and an out-of-range group left out) and pred_out match a CPU count, and a second call accumulates."""
    gen = torch.Generator().manual_seed(n + k)
    z = torch.randn(n, k, generator=gen) * 3
    z[n // 2, :] = 0.5  # an all-equal row: the first class
    labels = torch.randint(0, k, (n,), generator=gen)
    groups = torch.randint(0, 2, (n,), generator=gen).to(torch.int32)
    if n > 2:
        labels[1], groups[2] = k, 2   # not counted
    want = z.argmax(1)
    assert int(want[n // 2]) == 0
    ref = _count(want, labels, groups, 2, k)
    for mode in (ARGMAX_SOFTMAX, ARGMAX_LOGITS):
        pred, conf = _classify(gpu, z, labels, groups, 2, mode)
        assert torch.equal(pred, want)
        assert torch.equal(conf.cpu().view(2, k, k), ref)
        pred, conf = _classify(gpu, z, labels, groups, 2, mode, conf)
        assert torch.equal(conf.cpu().view(2, k, k), 2 * ref)
    assert L.lib().tspm_classify_update_ex(n, k, None, None, None, 1, None, None, None, None, None, 0, 2,
                                           L.stream_handle()) == INVALID
