"""tspm_textcnn_pool_fwd_len through the C ABI: the TextCNN pooling over each row's own windows.

Row b of conv i (height kh_i) has n_i(b) = max(L_b - kh_i + 1, 1) windows, L_b = lengths[b] clamped to 1..steps.  Every
operation of the kernel is exact in float32 (one add, compares, a select, the mask scale), so the pooled values are held
bitwise to a float32 host restatement and the indices exactly.  Lengths [9, 1, 4, 5, 7] at steps 9 and heights (3, 4, 5):
full, shorter than every height, between two heights, equal to the tallest, general.  The conv outputs are multiples of
1/8 drawn without repetition (and the biases multiples of 1/8), so every window value of a channel is distinct but for
the planted cases and the ReLU's zeros, which the first-maximum rule settles; no case is excluded.  Outputs sit in
sentinel-guarded buffers.  The backward (tspm_textcnn_bwd, unchanged) is fed the masked indices and held to fp64
autograd of tests/textcnn_len_ref.py within the bound test_gpu_seq_ops.py uses for that entry point.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from oracle import mosi_ref as orc
from parity import Guarded, Ratios, op_check
from test_gpu_seq_ops import _pool_fwd, _same
from textcnn_len_ref import n_windows, pooled_len
from tspm_amd import _lib as L

pytestmark = pytest.mark.gpu
B, STEPS, HEIGHTS, C = 5, 9, (3, 4, 5), 4
NC = len(HEIGHTS) * C
LENGTHS = [9, 1, 4, 5, 7]
RATIOS = Ratios()


def _pool_len(gpu, convs, biases, keep, scale, ld, lengths, B=B, steps=STEPS, heights=HEIGHTS):
    n, nc = len(heights), len(heights) * C
    cd = [c.contiguous().to(gpu) for c in convs]
    bd = [b.to(gpu) for b in biases]
    kd = None if keep is None else keep.to(gpu)
    ln = torch.tensor(lengths, dtype=torch.int32, device=gpu)
    pooled, arg, out = Guarded(gpu, B, nc), Guarded(gpu, B, nc, dtype=torch.uint8), Guarded(gpu, B, nc, ld)
    L.check(L.lib().tspm_textcnn_pool_fwd_len(B, steps, n, (ctypes.c_int32 * n)(*heights), C,
                                              (ctypes.c_void_p * n)(*[c.data_ptr() for c in cd]),
                                              (ctypes.c_void_p * n)(*[b.data_ptr() for b in bd]), L.ptr(kd), scale,
                                              pooled.ptr(), arg.ptr(), out.ptr(), ld, ln.data_ptr(), L.stream_handle()),
            "textcnn_pool_fwd_len")
    torch.cuda.synchronize()
    for nme, gd in (("pooled", pooled), ("argmax", arg), ("out", out)):
        gd.intact("textcnn_pool_fwd_len " + nme)
    return pooled.cpu(), arg.cpu(), out.cpu()


def _restate(convs, biases, keep, scale, lengths):
    """float32 on the host: per (row, conv) the first maximum of relu(fl32(y + bias)) over the row's own windows (a NaN
    wins); out = pooled * (keep ? scale : 0)."""
    pooled, arg = torch.zeros(B, NC), torch.zeros(B, NC, dtype=torch.int64)
    for i, kh in enumerate(HEIGHTS):
        for b in range(B):
            n = n_windows(lengths[b], kh, STEPS)
            w = (convs[i][:n, b, :] + biases[i][None, :])  # [n, C], one float32 add
            w = torch.where(w > 0, w, torch.where(w.isnan(), w, torch.zeros(())))
            t = torch.arange(n)[:, None].expand(n, C)
            for c in range(C):
                col = w[:, c]
                if col.isnan().any():
                    pooled[b, i * C + c], arg[b, i * C + c] = float("nan"), int(t[:, c][col.isnan()].max())
                else:
                    pooled[b, i * C + c] = col.max()
                    arg[b, i * C + c] = int(t[:, c][col == col.max()].min())  # the first maximum
    out = pooled if keep is None else pooled * torch.where(keep.bool(), torch.tensor(scale), torch.tensor(0.0))
    return pooled, arg, out


def _case(seed=0, plant=True):
    g = torch.Generator().manual_seed(seed)
    sizes = [(STEPS - kh + 1) * B * C for kh in HEIGHTS]
    perm = torch.randperm(sum(sizes), generator=g).float()
    vals = (perm - sum(sizes) // 3) / 8.0  # distinct multiples of 1/8, about a third of them negative
    convs, off = [], 0
    for kh, sz in zip(HEIGHTS, sizes):
        convs.append(vals[off:off + sz].view(STEPS - kh + 1, B, C).clone())
        off += sz
    biases = [torch.randint(-8, 9, (C,), generator=g).float() / 8.0 for _ in HEIGHTS]
    keep = (torch.rand(B, NC, generator=g) > 0.5).to(torch.uint8)
    planted = {}
    if plant:
        # a strictly larger value just past a row's last window: it must lose (row 4: 5 windows of conv 0; row 1: one
        # window of every conv)
        convs[0][5, 4, 0] = 1000.0
        for i in range(3):
            convs[i][1, 1, :] = 1000.0
        # an exact tie inside the row (row 0, conv 1, 6 windows): the first wins
        convs[1][1, 0, 2] = convs[1][4, 0, 2] = 500.0
        planted[(0, C + 2)] = 1
        # a NaN past the boundary (row 3 of length 5 has 3 windows of conv 0) must not appear; one inside (row 4 has 3
        # windows of conv 2) wins
        convs[0][3, 3, 1] = float("nan")
        convs[2][1, 4, 3] = float("nan")
        planted[(4, 2 * C + 3)] = 1
    return convs, biases, keep, planted


def test_pool_len_is_the_float32_restatement(gpu):
    convs, biases, keep, planted = _case()
    for kp in (keep, None):
        for ld in (NC, NC + 4):
            got = _pool_len(gpu, convs, biases, kp, 2.0, ld, LENGTHS)
            again = _pool_len(gpu, convs, biases, kp, 2.0, ld, LENGTHS)
            ref = _restate(convs, biases, kp, 2.0, LENGTHS)
            assert _same(got[0], ref[0]), "pooled"
            assert torch.equal(got[1].long(), ref[1]), "argmax"
            assert _same(got[2], ref[2]), "out"
            assert all(_same(a, b) for a, b in zip(got, again)), "not deterministic"
    pooled, arg, _ = got
    for i, kh in enumerate(HEIGHTS):  # every index inside the row's own windows
        for b in range(B):
            assert int(arg[b, i * C:(i + 1) * C].max()) < n_windows(LENGTHS[b], kh, STEPS)
    assert float(pooled[4, 0]) < 1000.0 and bool((pooled[1] < 1000.0).all())  # the larger value past the boundary lost
    assert int(arg[0, C + 2]) == 1 and float(pooled[0, C + 2]) == 500.0 + float(biases[1][2])  # the first of the tie
    assert not bool(pooled[3].isnan().any())  # the NaN past row 3's boundary
    assert bool(pooled[4, 2 * C + 3].isnan()) and int(arg[4, 2 * C + 3]) == 1  # the NaN inside row 4
    assert int(pooled.isnan().sum()) == 1
    for (b, c), t in planted.items():
        assert int(arg[b, c]) == t


def test_full_lengths_are_the_unmasked_entry_point_bitwise(gpu):
    convs, biases, keep, _ = _case(1)
    for kp in (keep, None):
        got = _pool_len(gpu, convs, biases, kp, 2.0, NC + 4, [STEPS] * B)
        ref = _pool_fwd(gpu, B, STEPS, HEIGHTS, C, convs, biases, kp, 2.0, NC + 4)
        for a, b, nme in zip(got, ref, ("pooled", "argmax", "out")):
            assert _same(a, b), nme


def test_each_row_is_the_unmasked_entry_point_on_that_row_alone(gpu):
    """Row b, conv i: tspm_textcnn_pool_fwd with nconv = 1 on the row's own windows, steps = max(L_b, kh_i)."""
    convs, biases, keep, _ = _case(2)
    got = _pool_len(gpu, convs, biases, keep, 2.0, NC, LENGTHS)
    for i, kh in enumerate(HEIGHTS):
        for b in range(B):
            n = n_windows(LENGTHS[b], kh, STEPS)
            steps = max(LENGTHS[b], kh)
            assert steps - kh + 1 == n
            alone = _pool_fwd(gpu, 1, steps, (kh,), C, [convs[i][:n, b:b + 1, :].contiguous()], [biases[i]],
                              keep[b:b + 1, i * C:(i + 1) * C].contiguous(), 2.0, C)
            for a, r, nme in zip(got, alone, ("pooled", "argmax", "out")):
                assert _same(a[b:b + 1, i * C:(i + 1) * C], r), (nme, i, b)


def test_lengths_are_clamped_in_the_kernel(gpu):
    convs, biases, keep, _ = _case(3)
    got = _pool_len(gpu, convs, biases, keep, 2.0, NC, [0, -3, 1000, 4, 2 ** 31 - 1])
    ref = _pool_len(gpu, convs, biases, keep, 2.0, NC, [1, 1, STEPS, 4, STEPS])
    host = _restate(convs, biases, keep, 2.0, [1, 1, STEPS, 4, STEPS])
    for a, b, nme in zip(got, ref, ("pooled", "argmax", "out")):
        assert _same(a, b), nme
    assert _same(got[0], host[0]) and torch.equal(got[1].long(), host[1])


def test_bwd_takes_the_masked_indices_vs_fp64_autograd(gpu):
    """x [B, steps, Fe] zero-padded past each length; conv outputs computed on the host in float32, pooled on the device
    with lengths, then tspm_textcnn_bwd on those indices.  Reference: autograd through the restatement in float64 (and
    float32) with the device's indices and ReLU decisions forced."""
    Fe = 33
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, STEPS, Fe, generator=g)
    for b, n in enumerate(LENGTHS):
        x[b, n:] = 0
    torch.manual_seed(11)
    net = orc.OracleTextCNN(Fe, embd_size=4, out_channels=C, kernel_heights=list(HEIGHTS), dropout=0.5)
    cs = (net.conv1, net.conv2, net.conv3)
    with torch.no_grad():  # conv outputs without bias, time-major [Tout][B][C]
        convs = [F.conv2d(x.view(B, 1, STEPS, Fe), cv.weight)[:, :, :, 0].permute(2, 0, 1).contiguous() for cv in cs]
    biases = [cv.bias.detach().clone() for cv in cs]
    keep = (torch.rand(B, NC, generator=g) > 0.3).to(torch.uint8)
    dout = torch.randn(B, NC + 3, generator=g)
    dout[:, NC:] = 1e30  # the padding columns of ld_dout are not gradients
    pooled, arg, _ = _pool_len(gpu, convs, biases, keep, 2.0, NC, LENGTHS)
    force = {}
    for i in range(3):
        force[f"text.pool{i}"] = arg[:, i * C:(i + 1) * C].long()
        force[f"text.relu{i}"] = pooled[:, i * C:(i + 1) * C] > 0
    refs = {}
    for dtype in (torch.float64, torch.float32):
        m = orc.OracleTextCNN(Fe, embd_size=4, out_channels=C, kernel_heights=list(HEIGHTS), dropout=0.5).to(dtype)
        m.load_state_dict(net.state_dict())
        tr = orc.MosiTrace(force)
        h = pooled_len(m, x.to(dtype), LENGTHS, tr)
        (h * keep.to(dtype) * 2.0 * dout[:, :NC].to(dtype)).sum().backward()
        refs[dtype] = ([cv.weight.grad[:, 0] for cv in (m.conv1, m.conv2, m.conv3)],
                       [cv.bias.grad for cv in (m.conv1, m.conv2, m.conv3)])
        if dtype == torch.float64:  # the device's decisions against fp64's own: no flip but a near-tie
            from parity import near_tie_flips
            for i in range(3):
                site = f"text.pool{i}"
                near_tie_flips(site, force[site], tr.idx[site], tr.pre[site].double().relu(), 2)
    xd = x.transpose(0, 1).contiguous().to(gpu)  # time-major [steps][B][Fe]
    n = len(HEIGHTS)
    dws = [Guarded(gpu, C * h, Fe) for h in HEIGHTS]
    dbs = [Guarded(gpu, 1, C) for _ in HEIGHTS]
    work = Guarded(gpu, B, NC)
    dd, kd, pd, ad = dout.to(gpu), keep.to(gpu), pooled.to(gpu), arg.to(gpu)
    L.check(L.lib().tspm_textcnn_bwd(B, STEPS, Fe, n, (ctypes.c_int32 * n)(*HEIGHTS), C, xd.data_ptr(), dd.data_ptr(),
                                     NC + 3, kd.data_ptr(), 2.0, pd.data_ptr(), ad.data_ptr(),
                                     (ctypes.c_void_p * n)(*[d.ptr() for d in dws]),
                                     (ctypes.c_void_p * n)(*[d.ptr() for d in dbs]), work.ptr(), L.stream_handle()),
            "textcnn_bwd")
    torch.cuda.synchronize()
    for d in dws + dbs + [work]:
        d.intact("textcnn_bwd")
    for i, h in enumerate(HEIGHTS):
        op_check(f"textcnn_bwd.dw[len conv{i}]", dws[i].cpu().view(C, h, Fe), refs[torch.float32][0][i],
                 refs[torch.float64][0][i], grad=True, ratios=RATIOS)
        op_check(f"textcnn_bwd.db[len conv{i}]", dbs[i].cpu().view(C), refs[torch.float32][1][i],
                 refs[torch.float64][1][i], grad=True, ratios=RATIOS)
    print("worst ratios:", RATIOS)
