"""The fp32 MFMA small GEMM behind every nn.Linear (csrc/misc.hip: gemm_body under k_gemm_small / k_gemm_pair /
k_gemm_multi, k_splitk_reduce) through each entry point, at the smallest shapes that reach each loop and each
host-side decision of gemm_small / gemm_wk.

Wave count: 1 for K < 64, 2 for 64 <= K < 128, 4 for K >= 128.  The vector loop (32 k per round, 16-byte loads)
needs K >= 128 and every K-contiguous operand 16-byte aligned with ld % 4 == 0; the waves' K chunks are then
multiples of 32, else of 8.  After it come the 32-step unrolled loop and the masked 8-step tail.

Every case runs in regime E (integer data: the result must EQUAL the int64 reference, see op_refs.py) and, where
K >= 128, in regime R (randn data against fp64 within 64 * 2^-23 * sum|a||b|).  Outputs are sentinel-filled
(parity.Guarded): padding columns and the tail must be bit-identical afterwards; input padding is 1e30, so a read
of it cannot go unnoticed.
"""
import ctypes

import pytest
import torch

import op_refs as R
from parity import Guarded
from tspm_amd import _lib as L

pytestmark = pytest.mark.gpu
OK, INVALID, WORKSPACE = 0, 1, 3


def _regimes(k):
    return ("E", "R") if k >= 128 else ("E",)


def _sync():
    torch.cuda.synchronize()


class Prob:
    """One Linear's operands on the device: x [n, fin] (rows ldx apart, starting xlead floats into its buffer),
    w [fout, fin], b [fout], dy [n, fout] (rows lddy apart), keep [n, fout]."""

    def __init__(self, gpu, regime, n, fin, fout, seed=0, ldx=None, xlead=0, lddy=None):
        gen = torch.Generator().manual_seed(1000 * seed + 7 * n + 3 * fin + fout)
        self.gpu, self.regime, self.n, self.fin, self.fout = gpu, regime, n, fin, fout
        self.x, self.w, self.b, self.dy, self.keep = R.gemm_inputs(gen, regime, n, fin, fout)
        self.ldx, self.lddy = ldx or fin, lddy or fout
        self._xd = R.padded(self.x, self.ldx, xlead).to(gpu)
        self._dyd = R.padded(self.dy, self.lddy).to(gpu)
        self.xp, self.dyp = self._xd.data_ptr() + 4 * xlead, self._dyd.data_ptr()
        self.wd, self.bd, self.kd = self.w.to(gpu), self.b.to(gpu), self.keep.to(gpu)

    def tag(self):
        return f"{self.regime} n{self.n} in{self.fin} out{self.fout} ldx{self.ldx} lddy{self.lddy}"


def _fwd(p, bias, relu, keep, ldy=None):
    y = Guarded(p.gpu, p.n, p.fout, ldy)
    L.check(L.lib().tspm_linear_fwd(p.n, p.fin, p.fout, p.xp, p.ldx, p.wd.data_ptr(), p.bd.data_ptr() if bias else None,
                                    int(relu), p.kd.data_ptr() if keep else None, R.KEEP_SCALE, y.ptr(), y.ld,
                                    L.stream_handle()), "linear_fwd")
    _sync()
    y.intact("linear_fwd y")
    return y.cpu()


def _check_fwd(name, p, y, bias, relu, keep):
    ref, tol = R.linear_fwd_ref(p.regime, p.x, p.w, p.b if bias else None, relu, p.keep if keep else None)
    R.check(f"{name}.y[{p.tag()} b{int(bias)} r{int(relu)} k{int(keep)}]", y, ref, tol)


def _bwd_data(p, lddx=None):
    dx = Guarded(p.gpu, p.n, p.fin, lddx)
    L.check(L.lib().tspm_linear_bwd_data(p.n, p.fin, p.fout, p.dyp, p.lddy, p.wd.data_ptr(), dx.ptr(), dx.ld,
                                         L.stream_handle()), "linear_bwd_data")
    _sync()
    dx.intact("linear_bwd_data dx")
    return dx.cpu()


def _bwd_weight(p, with_db=True):
    dw, db = Guarded(p.gpu, p.fout, p.fin), Guarded(p.gpu, 1, p.fout)
    L.check(L.lib().tspm_linear_bwd_weight(p.n, p.fin, p.fout, p.xp, p.ldx, p.dyp, p.lddy, dw.ptr(),
                                           db.ptr() if with_db else None, L.stream_handle()), "linear_bwd_weight")
    _sync()
    dw.intact("linear_bwd_weight dw"); db.intact("linear_bwd_weight db")
    return dw.cpu(), db


def _untouched(g: Guarded) -> bool:
    return bool(g.cpu().isnan().all())  # the sentinel is a NaN pattern; intact() covers the rest


def _check_bwd(name, p, dw=None, db=None, dx=None):
    rdw, rdb, tdw, tdb = R.linear_bwd_weight_ref(p.regime, p.x, p.dy)
    if dw is not None:
        R.check(f"{name}.dw[{p.tag()}]", dw, rdw, tdw)
    if db is not None:
        R.check(f"{name}.db[{p.tag()}]", db, rdb, tdb)
    if dx is not None:
        rdx, tdx = R.linear_bwd_data_ref(p.regime, p.dy, p.w)
        R.check(f"{name}.dx[{p.tag()}]", dx, rdx, tdx)


# ------------------------------------------------------------------------------------------------
# tspm_linear_fwd: K = in
# ------------------------------------------------------------------------------------------------
FWD_CASES = [
    # n, in, out, ldx, xlead: the path the case is meant to hit
    (1, 1, 1, 1, 0),        # one wave, a single masked tail step (k = 0 only); one row, one column
    (31, 7, 31, 7, 0),      # one wave, one masked 8-step tail round
    (33, 63, 33, 63, 0),    # one wave: one unrolled 32-step round, then tail rounds ending in a masked one; 2x2 tiles
    (1, 64, 65, 64, 0),     # two waves of exactly one unrolled round each; three column tiles
    (31, 100, 1, 100, 0),   # two waves with chunks of 56 and 44: unrolled round + unmasked and masked tail rounds
    (33, 127, 31, 127, 0),  # two waves, the second one step short of its chunk
    (31, 128, 33, 128, 0),  # four waves, vector loop: exactly one 32-k vector round each, no tail
    (33, 132, 65, 132, 0),  # vector loop, chunks of 64: wave 2 has only a 4-step masked tail, wave 3 is empty
    (1, 160, 31, 160, 0),   # vector loop: wave 2 one round, wave 3 empty
    (33, 260, 33, 260, 0),  # vector loop, chunks of 96: wave 2 runs two vector rounds AND the masked tail
    (31, 300, 65, 300, 0),  # vector loop, chunks of 96: wave 3 has a 12-step tail (one full, one masked round)
    (33, 130, 33, 130, 0),  # K >= 128 but w's row stride 130 % 4 != 0: fallback, chunks of 40, 40, 40, 10
    (31, 132, 31, 133, 0),  # K >= 128 but ldx = 133: fallback from the vector loop
    (33, 132, 65, 136, 1),  # K >= 128, ldx % 4 == 0 but x starts one float into its buffer: fallback
]


@pytest.mark.parametrize("idx", range(len(FWD_CASES)), ids=[f"n{c[0]}-in{c[1]}-out{c[2]}-ldx{c[3]}-lead{c[4]}"
                                                            for c in FWD_CASES])
def test_linear_fwd_paths(gpu, idx):
    n, fin, fout, ldx, lead = FWD_CASES[idx]
    bias, relu, keep = bool(idx & 1), bool(idx & 2), bool(idx & 4)  # every case with another epilogue
    for regime in _regimes(fin):
        p = Prob(gpu, regime, n, fin, fout, seed=idx, ldx=ldx, xlead=lead)
        for ldy in (fout, fout + 3):
            y = _fwd(p, bias, relu, keep, ldy)
            _check_fwd("linear_fwd", p, y, bias, relu, keep)
        # the plain product too, so that every path is seen without an epilogue that could mask an element
        _check_fwd("linear_fwd", p, _fwd(p, False, False, False), False, False, False)


@pytest.mark.parametrize("bias", [0, 1])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("keep", [0, 1])
def test_linear_fwd_epilogue(gpu, bias, relu, keep):
    """bias NULL / given x ReLU x keep mask NULL / given, written with ldy > out (vector path with a tail)."""
    for regime in ("E", "R"):
        p = Prob(gpu, regime, 33, 132, 33, seed=50)
        _check_fwd("linear_fwd", p, _fwd(p, bias, relu, keep, ldy=40), bias, relu, keep)


# ------------------------------------------------------------------------------------------------
# tspm_linear_bwd_data: K = out; A = dy is K-contiguous (vector loads), B = w is strided
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,fin,fout,lddy", [
    (33, 33, 10, 10),     # one wave, unmasked + masked tail round
    (7, 65, 70, 70),      # two waves (chunks of 40 and 30)
    (31, 31, 128, 128),   # four waves, vector loop on A only: one round each
    (33, 40, 132, 132),   # vector loop on A: wave 2 a 4-step tail, wave 3 empty
    (9, 33, 300, 300),    # vector loop on A: three rounds per wave, 12-step tail in wave 3
    (33, 40, 132, 133),   # lddy % 4 != 0: fallback from the vector loop
])
def test_linear_bwd_data_paths(gpu, n, fin, fout, lddy):
    for regime in _regimes(fout):
        p = Prob(gpu, regime, n, fin, fout, seed=60, lddy=lddy)
        for lddx in (fin, fin + 5):
            _check_bwd("linear_bwd_data", p, dx=_bwd_data(p, lddx))


# ------------------------------------------------------------------------------------------------
# tspm_linear_bwd_weight: K = n, no operand K-contiguous (never the vector loop); db = row sums of the A operand,
# written by the tiles with col0 == 0 only (in > 32 gives tiles with col0 != 0, out > 32 more than one row tile)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,fin,fout", [
    (1, 40, 40),     # one wave, one masked step
    (7, 33, 65),     # one wave, one masked tail round; three row tiles
    (70, 40, 33),    # two waves (40 + 30)
    (130, 65, 40),   # four waves with chunks of 40, 40, 40, 10
    (257, 33, 34),   # four waves with chunks of 72: two unrolled rounds + tail, the last wave 41
])
@pytest.mark.parametrize("with_db", [True, False])
def test_linear_bwd_weight_paths(gpu, n, fin, fout, with_db):
    for regime in _regimes(n):
        p = Prob(gpu, regime, n, fin, fout, seed=70, ldx=fin + (3 if with_db else 0), lddy=fout + (0 if with_db else 5))
        dw, db = _bwd_weight(p, with_db)
        _check_bwd("linear_bwd_weight", p, dw=dw, db=db.cpu().view(fout) if with_db else None)
        if not with_db:
            assert _untouched(db)


# ------------------------------------------------------------------------------------------------
# split-K forward: k_gemm_small over K slices + k_splitk_reduce with the epilogue
# ------------------------------------------------------------------------------------------------
def _fwd_splitk(p, bias, relu, keep, splits, ldy=None, ws_bytes=None, null_ws=False):
    lib = L.lib()
    need = lib.tspm_linear_fwd_splitk_workspace(p.n, p.fin, p.fout, splits)
    y = Guarded(p.gpu, p.n, p.fout, ldy)
    ws = Guarded(p.gpu, 1, max(need, 4), dtype=torch.uint8)
    st = lib.tspm_linear_fwd_splitk(p.n, p.fin, p.fout, p.xp, p.ldx, p.wd.data_ptr(), p.bd.data_ptr() if bias else None,
                                    int(relu), p.kd.data_ptr() if keep else None, R.KEEP_SCALE, y.ptr(), y.ld, splits,
                                    None if null_ws else ws.ptr(), need if ws_bytes is None else ws_bytes,
                                    L.stream_handle())
    _sync()
    y.intact("linear_fwd_splitk y"); ws.intact("linear_fwd_splitk workspace")
    return st, y, need


def test_linear_fwd_splitk_full_epilogue(gpu):
    """(5, 300, 33) in 2 slices of 160 and 140 with bias, ReLU, keep mask and ldy > out, and each of them alone."""
    for regime in ("E", "R"):
        p = Prob(gpu, regime, 5, 300, 33, seed=80)
        for bias, relu, keep, ldy in ((1, 1, 1, 37), (1, 0, 0, 33), (0, 1, 0, 37), (0, 0, 1, 34), (0, 0, 0, 33)):
            st, y, need = _fwd_splitk(p, bias, relu, keep, 2, ldy)
            assert st == OK and need == 2 * 5 * 33 * 4
            _check_fwd("linear_fwd_splitk", p, y.cpu(), bias, relu, keep)


def test_linear_fwd_splitk_collapse_and_single(gpu):
    """(3, 64, 40) asked for 4 slices: slices are multiples of 32, so 2 remain (and the workspace query says so);
    splits = 1 needs no workspace and takes a NULL one."""
    p = Prob(gpu, "E", 3, 64, 40, seed=81)
    st, y, need = _fwd_splitk(p, 1, 1, 1, 4, 43)
    assert st == OK and need == 2 * 3 * 40 * 4
    _check_fwd("linear_fwd_splitk", p, y.cpu(), True, True, True)
    for regime in ("E", "R"):
        p = Prob(gpu, regime, 5, 300, 33, seed=82)
        st, y, need = _fwd_splitk(p, 1, 1, 1, 1, 37, null_ws=True)
        assert st == OK and need == 0
        _check_fwd("linear_fwd_splitk", p, y.cpu(), True, True, True)
        assert torch.equal(y.cpu(), _fwd(p, True, True, True, 37))  # one slice is the plain launch


def test_linear_fwd_splitk_short_workspace(gpu):
    p = Prob(gpu, "E", 5, 300, 33, seed=83)
    need = L.lib().tspm_linear_fwd_splitk_workspace(5, 300, 33, 2)
    for kw in (dict(ws_bytes=need - 4), dict(null_ws=True)):
        st, y, _ = _fwd_splitk(p, 1, 1, 1, 2, 37, **kw)
        assert st == WORKSPACE and _untouched(y)


# ------------------------------------------------------------------------------------------------
# split-K weight gradient (the LSTM weight gradients): the shapes of test_gpu_seq_ops.py in regime E
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,fin,fout,splits", [(33, 64, 256, 2), (80, 20, 256, 3), (736, 5, 256, 8), (100, 70, 30, 1)])
def test_linear_bwd_weight_splitk_exact(gpu, n, fin, fout, splits):
    lib = L.lib()
    need = lib.tspm_linear_bwd_weight_splitk_workspace(n, fin, fout, splits)
    assert (need > 0) == (splits > 1)
    for regime in _regimes(n):
        for ldx, lddy in ((fin, fout), (fin + 5, fout + 3)):
            p = Prob(gpu, regime, n, fin, fout, seed=90, ldx=ldx, lddy=lddy)

            def run():
                dw, db = Guarded(gpu, fout, fin), Guarded(gpu, 1, fout)
                ws = Guarded(gpu, 1, max(need, 4), dtype=torch.uint8)
                L.check(lib.tspm_linear_bwd_weight_splitk(n, fin, fout, p.xp, ldx, p.dyp, lddy, dw.ptr(), db.ptr(), splits,
                                                          ws.ptr(), need, L.stream_handle()), "bwd_weight_splitk")
                _sync()
                dw.intact("splitk dw"); db.intact("splitk db"); ws.intact("splitk workspace")
                return dw.cpu(), db.cpu().view(fout)
            dw, db = run()
            dw2, db2 = run()
            # the b_ih / b_hh property: the same dy gives the same db bits, call after call
            assert torch.equal(dw.view(torch.int32), dw2.view(torch.int32))
            assert torch.equal(db.view(torch.int32), db2.view(torch.int32))
            _check_bwd("linear_bwd_weight_splitk", p, dw=dw, db=db)


# ------------------------------------------------------------------------------------------------
# tspm_linear_bwd: weight-grad (K = n) and data-grad (K = out) in one k_gemm_pair launch; the product with fewer
# waves of its own (wkeff) leaves the launch's extra waves idle
# ------------------------------------------------------------------------------------------------
def _bwd_pair(p, with_db=True, with_dx=True, lddx=None):
    dw, db, dx = Guarded(p.gpu, p.fout, p.fin), Guarded(p.gpu, 1, p.fout), Guarded(p.gpu, p.n, p.fin, lddx)
    L.check(L.lib().tspm_linear_bwd(p.n, p.fin, p.fout, p.xp, p.ldx, p.dyp, p.lddy, p.wd.data_ptr(), dw.ptr(),
                                    db.ptr() if with_db else None, dx.ptr() if with_dx else None, dx.ld,
                                    L.stream_handle()), "linear_bwd")
    _sync()
    for g, nm in ((dw, "dw"), (db, "db"), (dx, "dx")):
        g.intact("linear_bwd " + nm)
    return dw, db, dx


def _bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("n", [7, 70, 130])      # the weight-grad's own wave count: 1, 2, 4
@pytest.mark.parametrize("fout", [10, 70, 132])  # the data-grad's own wave count: 1, 2, 4 (132: vector loop + tail)
def test_linear_bwd_pair_wave_combinations(gpu, n, fout):
    fin = 33
    for regime in _regimes(max(n, fout)):
        p = Prob(gpu, regime, n, fin, fout, seed=100)
        sdw, sdb = _bwd_weight(p, True)
        sdx = _bwd_data(p, fin + 2)
        for with_db, with_dx in ((True, True), (False, True), (True, False)):
            dw, db, dx = _bwd_pair(p, with_db, with_dx, fin + 2)
            assert _bits_equal(dw.cpu(), sdw), "pair dw differs from tspm_linear_bwd_weight"
            _check_bwd("linear_bwd", p, dw=dw.cpu())
            if with_db:
                assert _bits_equal(db.cpu(), sdb.cpu()), "pair db differs from tspm_linear_bwd_weight"
                _check_bwd("linear_bwd", p, db=db.cpu().view(fout))
            else:
                assert _untouched(db)
            if with_dx:
                assert _bits_equal(dx.cpu(), sdx), "pair dx differs from tspm_linear_bwd_data"
                _check_bwd("linear_bwd", p, dx=dx.cpu())
            else:
                assert _untouched(dx)


# ------------------------------------------------------------------------------------------------
# tspm_linear_fwd_pair: two forwards of one shape in one launch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,fin,fout,ldx0,ldx1,lead1", [
    (33, 132, 40, 132, 136, 1),  # problem 0 on the vector loop, problem 1 (x1 one float into its buffer) not
    (31, 64, 33, 64, 70, 0),     # two waves each, ldx0 != ldx1
    (5, 300, 65, 304, 300, 0),   # both on the vector loop
])
def test_linear_fwd_pair(gpu, n, fin, fout, ldx0, ldx1, lead1):
    for regime in _regimes(fin):
        p0 = Prob(gpu, regime, n, fin, fout, seed=110, ldx=ldx0)
        p1 = Prob(gpu, regime, n, fin, fout, seed=111, ldx=ldx1, xlead=lead1)
        y0, y1 = Guarded(gpu, n, fout, fout + 3), Guarded(gpu, n, fout, fout)
        L.check(L.lib().tspm_linear_fwd_pair(n, fin, fout, p0.xp, ldx0, p0.wd.data_ptr(), y0.ptr(), y0.ld, p1.xp, ldx1,
                                             p1.wd.data_ptr(), y1.ptr(), y1.ld, L.stream_handle()), "linear_fwd_pair")
        _sync()
        y0.intact("fwd_pair y0"); y1.intact("fwd_pair y1")
        for p, y in ((p0, y0), (p1, y1)):
            assert _bits_equal(y.cpu(), _fwd(p, False, False, False, y.ld)), "pair output differs from tspm_linear_fwd"
            _check_fwd("linear_fwd_pair", p, y.cpu(), False, False, False)


# ------------------------------------------------------------------------------------------------
# tspm_linear_bwd_multi: up to two Linears' backwards (2-4 products) in one k_gemm_multi launch
# ------------------------------------------------------------------------------------------------
MULTI_SHAPES = [(9, 130, 40), (70, 33, 132)]  # (n, in, out): weight-grads of 1 and 2 waves, data-grads of 1 and 4


def _multi(gpu, probs, dx_given, lddx_off=2, count=None, null_descs=False, lddx_short=False):
    outs, descs = [], (L.LinearBwdDesc * max(len(probs), 1))()
    for i, (p, has_dx) in enumerate(zip(probs, dx_given)):
        dw, db = Guarded(gpu, p.fout, p.fin), Guarded(gpu, 1, p.fout)
        dx = Guarded(gpu, p.n, p.fin, p.fin + lddx_off)
        outs.append((dw, db, dx))
        descs[i] = L.LinearBwdDesc(p.n, p.fin, p.fout, p.ldx, p.lddy, p.fin - 1 if lddx_short else dx.ld, p.xp, p.dyp,
                                   p.wd.data_ptr(), dw.ptr(), db.ptr(), dx.ptr() if has_dx else None)
    st = L.lib().tspm_linear_bwd_multi(len(probs) if count is None else count, None if null_descs else descs,
                                       L.stream_handle())
    _sync()
    for trio in outs:
        for g in trio:
            g.intact("linear_bwd_multi output")
    return st, outs


@pytest.mark.parametrize("which,dx_given", [
    ((0,), (True,)), ((1,), (True,)), ((1,), (False,)),                      # count 1: two products, or one
    ((0, 1), (True, True)), ((0, 1), (False, True)), ((0, 1), (True, False)), ((0, 1), (False, False)),
])
def test_linear_bwd_multi(gpu, which, dx_given):
    """2, 3 and 4 products: every start[] boundary lies between tiles of different problems.  Each descriptor's
    results are bitwise its own tspm_linear_bwd, and exact in regime E."""
    for regime in ("E", "R"):
        probs = [Prob(gpu, regime, *MULTI_SHAPES[i], seed=120 + i, ldx=MULTI_SHAPES[i][1] + i, lddy=MULTI_SHAPES[i][2] + 1)
                 for i in which]
        st, outs = _multi(gpu, probs, dx_given)
        assert st == OK
        for p, has_dx, (dw, db, dx) in zip(probs, dx_given, outs):
            sdw, sdb, sdx = _bwd_pair(p, True, has_dx, dx.ld)
            assert _bits_equal(dw.cpu(), sdw.cpu()) and _bits_equal(db.cpu(), sdb.cpu())
            _check_bwd("linear_bwd_multi", p, dw=dw.cpu(), db=db.cpu().view(p.fout))
            if has_dx:
                assert _bits_equal(dx.cpu(), sdx.cpu())
                _check_bwd("linear_bwd_multi", p, dx=dx.cpu())
            else:
                assert _untouched(dx)


def test_linear_bwd_multi_refusals(gpu):
    probs = [Prob(gpu, "E", *MULTI_SHAPES[i], seed=130 + i) for i in (0, 1)]
    for kw in (dict(count=0), dict(count=3), dict(null_descs=True), dict(lddx_short=True)):
        st, outs = _multi(gpu, probs, (True, True), **kw)
        assert st == INVALID, kw
        assert all(_untouched(g) for trio in outs for g in trio), kw


# ------------------------------------------------------------------------------------------------
# tspm_act_bwd: g = y > 0 ? g * scale : 0, in place, strided
# ------------------------------------------------------------------------------------------------
def test_act_bwd_strided_special_values(gpu):
    n, cols, ldg, ldy = 37, 33, 35, 40
    gen = torch.Generator().manual_seed(140)
    y = torch.randn(n, cols, generator=gen)
    special = torch.tensor([0.0, -0.0, float("nan"), float("inf"), -float("inf"), 3.0, -3.0])
    y.view(-1)[torch.randperm(n * cols, generator=gen)[:7 * 20]] = special.repeat(20)
    g = torch.randn(n, cols, generator=gen)
    scale = 2.0
    gd = Guarded(gpu, n, cols, ldg)
    gd.t.copy_(g)
    yd = R.padded(y, ldy).to(gpu)
    L.check(L.lib().tspm_act_bwd(n, cols, gd.ptr(), ldg, yd.data_ptr(), ldy, scale, L.stream_handle()), "act_bwd")
    _sync()
    gd.intact("act_bwd g")
    want = torch.where(y > 0, g * scale, torch.zeros_like(g))
    assert _bits_equal(gd.cpu(), want)
    assert L.lib().tspm_act_bwd(n, cols, gd.ptr(), cols - 1, yd.data_ptr(), ldy, scale, L.stream_handle()) == INVALID
