"""tspm_cached_head_train_steps alone: K consecutive cached head steps per call, Adam applied in each step's second
launch.  Held BITWISE to K x (tspm_cached_head_train_step on the step's slice of the index vector, then tspm_adam_step on
each of the six tensors) from the same start: parameters, both moments, the last step's gradients, logits and mask, the
loss, stats, the K log entries, counters, confusion counts and the step counter.  The cache, shapes and pattern sets are
test_gpu_cached_head_ops' / test_gpu_pattern_head_train's.

The four flat Adam buffers are laid out as FusedAdam lays a group out — every tensor at an offset rounded up to 4 floats
— between 8 sentinel floats at either end, inside guarded buffers: every sentinel, the padding between the tensors
included, must survive the call.

The reference's tspm_adam_step covers each tensor's slot, i.e. its element count rounded up to 4 floats, which is what
FusedAdam's one launch over the padded group does for it.  A count that is no multiple of 4 would send the last
count % 4 elements through k_adam's scalar tail, which compiles exp_avg_sq to a rounded product plus a rounded product
where the float4 body has one fused multiply-add: the tail is not bitwise the body, no FusedAdam group reaches it, and
the fused launch follows the body (the padding of the REFERENCE's buffers is updated too; it is not compared)."""
import ctypes

import pytest
import torch

import head_stage_ref as R
import parity
import test_gpu_cached_head_ops as CO
import test_gpu_pattern_head_train as T
from tspm_amd import _lib as L

pytestmark = pytest.mark.gpu

SHAPES, PATSETS, GRADS, LOSS_WEIGHT, bits = T.SHAPES, T.PATSETS, T.GRADS, T.LOSS_WEIGHT, T.bits
N_ROWS, INVALID = CO.N_ROWS, CO.INVALID
NAMES = ("w0", "b0", "w3", "b3", "w5", "b5")
EDGE, STEP0, SEED, CAP, N_GROUPS = 8, 41, 0x1234_5678_9ABC, 6, 3
HYPER = (1e-2, 0.9, 0.999, 1e-8, 1e-3, 1.0)  # lr, betas, eps, weight decay, grad_scale
F32_SENTINEL = parity._SENTINEL[torch.float32]


def layout(shape):
    """name -> (offset, rows, cols) in the flat buffers, and their length."""
    B, F, wa, H, H2, C = shape
    dims = {"w0": (H, F), "b0": (1, H), "w3": (H2, H), "b3": (1, H2), "w5": (C, H2), "b5": (1, C)}
    at, off = EDGE, {}
    for n in NAMES:
        at = (at + 3) // 4 * 4
        off[n] = (at,) + dims[n]
        at += dims[n][0] * dims[n][1]
    return off, at + EDGE


def step_rows(shape, K):
    """[K*B] indices: every step its own, each with row 299, row 0 and (B > 3) a repeat."""
    B = shape[0]
    idx = CO.cache_case(shape)[2]
    rows = []
    for k in range(K):
        r = (idx + 37 * k) % N_ROWS
        r[0] = N_ROWS - 1
        if B > 1:
            r[-1] = 0
        if B > 3:
            r[2] = r[1]
        rows.append(r)
    return torch.cat(rows)


class State:
    """Everything one call (or its reference) reads and writes, on the device, with `reset()` to the common start."""

    def __init__(self, dev, shape, pats, K, rk=None, rg=None):
        B, F, wa, H, H2, C = shape
        self.dev, self.shape, self.pats, self.K = dev, shape, pats, K
        self.P = P = 1 if pats is None else len(pats)
        n = P * B
        emb, labels_all, _, x0, W = CO.cache_case(shape)
        self.emb, self.labels_all, self.x0 = emb.to(dev).contiguous(), labels_all.to(dev), x0.to(dev).contiguous()
        self.rows = step_rows(shape, K).to(dev)
        self.rk = None if rk is None else rk.to(dev).to(torch.uint8).contiguous()
        self.rg = None if rg is None else rg.to(dev).to(torch.int32).contiguous()
        self.off, self.total = layout(shape)
        g = torch.Generator().manual_seed(900 + B + F)
        self.init = {"param": torch.zeros(self.total), "exp_avg": torch.zeros(self.total),
                     "exp_avg_sq": torch.zeros(self.total)}
        self.inside = torch.zeros(self.total, dtype=torch.bool)
        for nm in NAMES:
            o, r, c = self.off[nm]
            self.init["param"][o:o + r * c] = W[nm].reshape(-1)
            self.init["exp_avg"][o:o + r * c] = 0.1 * torch.randn(r * c, generator=g)
            self.init["exp_avg_sq"][o:o + r * c] = 0.01 * torch.rand(r * c, generator=g)
            self.inside[o:o + r * c] = True
        self.flat = {k: parity.Guarded(dev, 1, self.total) for k in ("param", "grad", "exp_avg", "exp_avg_sq")}
        self.out = {"logits": parity.Guarded(dev, n, C), "loss": parity.Guarded(dev, 1, 1),
                    "mask": parity.Guarded(dev, n, H, dtype=torch.uint8)}
        need = int(L.lib().tspm_cached_head_train_workspace(B, P))
        self.ws = parity.Guarded(dev, need, 1, dtype=torch.uint8)
        self.hyper = torch.zeros(8, dtype=torch.float64, device=dev)
        self.stats = torch.zeros(4, device=dev)
        self.conf = torch.zeros(N_GROUPS, C, C, dtype=torch.int64, device=dev)
        self.loss_log = torch.zeros(CAP + 2, device=dev)
        self.counters = torch.zeros(2, dtype=torch.int64, device=dev)
        self.keep = self.gid = None
        if pats is not None:
            self.keep = (ctypes.c_int32 * (2 * P))(*[k for pt in pats for k in R.KEEP[pt]])
            self.gid = (ctypes.c_int32 * P)(*[(2, 0, 1)[i % 3] for i in range(P)])
        self.reset()

    def reset(self):
        for k, gd in self.flat.items():
            gd.flat.view(torch.int32).fill_(F32_SENTINEL)
            if k != "grad":
                gd.flat[:self.total][self.inside.to(self.dev)] = self.init[k][self.inside].to(self.dev)
        for gd in self.out.values():
            gd.flat.view(parity._BITS[gd.flat.dtype]).fill_(parity._SENTINEL[gd.flat.dtype])
        self.ws.flat.fill_(parity._SENTINEL[torch.uint8])
        self.hyper.copy_(torch.tensor(HYPER + (0.0, 0.0), dtype=torch.float64))
        self.hyper.view(torch.int64)[6] = STEP0
        self.stats.copy_(torch.tensor([1.5, 2.0, 3.0, 0.0]))
        self.conf.zero_()
        self.loss_log.fill_(-1.0)
        self.counters.copy_(torch.tensor([2, 1000]))
        torch.cuda.synchronize()

    def ptr(self, buf, name):
        return self.flat[buf].ptr() + 4 * self.off[name][0]

    def desc(self, k=0, **over):
        B, F, wa, H, H2, C = self.shape
        step = self.hyper.data_ptr() + L.HYPER_STEP_OFFSET
        f = dict(batch=B, npat=self.P, in_=F, w_audio=wa, hidden=H, hidden2=H2, classes=C, ld_emb=F, gen_keep=1,
                 n_groups=N_GROUPS, n_rows=N_ROWS, emb=self.emb.data_ptr(), x0=self.x0.data_ptr(),
                 rows=self.rows[k * B:].data_ptr(), labels_all=self.labels_all.data_ptr(), keep=self.keep,
                 group_id=self.gid, row_keep=None if self.rk is None else self.rk[k * B:].data_ptr(),
                 row_group=None if self.rg is None else self.rg[k * B:].data_ptr(),
                 **{nm: self.ptr("param", nm) for nm in NAMES}, p=0.5, loss_weight=LOSS_WEIGHT, seed=SEED, counter=step,
                 keep_mask=self.out["mask"].ptr(), logits=self.out["logits"].ptr(),
                 **{"g" + nm: self.ptr("grad", nm) for nm in NAMES}, loss=self.out["loss"].ptr(),
                 stats=self.stats.data_ptr(), adam_step=step, confusion=self.conf.data_ptr(),
                 loss_log=self.loss_log.data_ptr(), counters=self.counters.data_ptr(), log_capacity=CAP,
                 workspace=self.ws.ptr(), workspace_bytes=self.ws.rows)
        f.update(over)
        return L.CachedHeadTrainDesc(**f)

    def adam(self, **over):
        f = dict(param=self.flat["param"].ptr(), grad=self.flat["grad"].ptr(), exp_avg=self.flat["exp_avg"].ptr(),
                 exp_avg_sq=self.flat["exp_avg_sq"].ptr(), count=self.total, hyper=self.hyper.data_ptr())
        f.update(over)
        return L.HeadAdamDesc(**f)

    def call(self, steps=None, dover=None, aover=None):
        return L.lib().tspm_cached_head_train_steps(self.desc(**(dover or {})), self.adam(**(aover or {})),
                                                    self.K if steps is None else steps, L.stream_handle())

    def reference(self):
        """K x (the single step on slice k, then tspm_adam_step on each tensor's slot)."""
        lib, sh = L.lib(), L.stream_handle()
        for k in range(self.K):
            L.check(lib.tspm_cached_head_train_step(self.desc(k), sh), "cached_head_train_step")
            for nm in NAMES:
                o, r, c = self.off[nm]
                L.check(lib.tspm_adam_step((r * c + 3) // 4 * 4, self.ptr("param", nm), self.ptr("grad", nm),
                                           self.ptr("exp_avg", nm), self.ptr("exp_avg_sq", nm), self.hyper.data_ptr(),
                                           sh), "adam_step")
        torch.cuda.synchronize()

    def result(self):
        torch.cuda.synchronize()
        res = {}
        for k, gd in self.flat.items():
            flat = gd.flat.cpu()
            for nm in NAMES:
                o, r, c = self.off[nm]
                res[f"{k}.{nm}"] = flat[o:o + r * c].clone()
            res[f"{k}.outside"] = flat.view(torch.int32)[:self.total][~self.inside].clone()
            res[f"{k}.guard"] = flat.view(torch.int32)[self.total:].clone()
        for k, gd in self.out.items():
            res[k] = gd.cpu()
        res.update(stats=self.stats.cpu(), conf=self.conf.cpu(), loss_log=self.loss_log.cpu(),
                   counters=self.counters.cpu(), step=int(self.hyper.view(torch.int64)[6].item()),
                   hyper=self.hyper[:6].cpu())
        return res

    def intact(self):
        """Every sentinel of the call's own buffers: the ends, the padding between the tensors, the guards."""
        for k, gd in self.flat.items():
            gd.intact(k)
            outside = gd.flat.cpu().view(torch.int32)[:self.total][~self.inside]
            assert bool((outside == F32_SENTINEL).all()), f"{k}: an element outside the six tensors was written"
        for k, gd in self.out.items():
            gd.intact(k)
        self.ws.intact("workspace")


def same(got, ref):
    for k, v in ref.items():
        if k.endswith(".outside") or k.endswith(".guard"):
            continue  # the reference's tspm_adam_step covers each tensor's padded slot
        if isinstance(v, int):
            assert got[k] == v, (k, got[k], v)
        elif v.dtype.is_floating_point:
            assert torch.equal(bits(got[k]), bits(v)), k
        else:
            assert torch.equal(got[k], v), k


def check_against_reference(dev, shape, pats, K, rk=None, rg=None):
    ref = State(dev, shape, pats, K, rk, rg)
    ref.reference()
    want = ref.result()
    st = State(dev, shape, pats, K, rk, rg)
    L.check(st.call(), "cached_head_train_steps")
    got = st.result()
    st.intact()
    same(got, want)
    assert got["step"] == STEP0 + K
    assert got["counters"].tolist() == [2 + K, 1000 + K * st.P * shape[0]]
    assert got["loss_log"][2 + K - 1].item() == got["loss"].item()      # the last step's loss, logged last
    assert len({got["loss_log"][2 + k].item() for k in range(K)}) == K or K == 1  # a different batch and mask per step
    return st, got


@pytest.mark.parametrize("pats", PATSETS, ids=T._ids(PATSETS))
@pytest.mark.parametrize("shape", SHAPES, ids=T._ids(SHAPES))
def test_three_steps_every_pattern_mode(gpu, shape, pats):
    check_against_reference(gpu, shape, pats, 3)


@pytest.mark.parametrize("shape", SHAPES, ids=T._ids(SHAPES))
def test_one_step_is_the_single_step_plus_adam(gpu, shape):
    check_against_reference(gpu, shape, PATSETS[0], 1)


@pytest.mark.parametrize("shape", SHAPES, ids=T._ids(SHAPES))
def test_two_steps_per_sample_mode_mixed_flags(gpu, shape):
    B = shape[0]
    rk = CO.mixed_flags(2 * B, "mixed")
    rg = torch.tensor([2, 0, 1, 1, 0, 2, 0], dtype=torch.int32)[torch.arange(2 * B) % 7]
    check_against_reference(gpu, shape, None, 2, rk, rg)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=T._ids([SHAPES[0], SHAPES[2]]))
def test_captured_and_replayed_calls_are_bitwise_the_eager_call(gpu, shape):
    st, eager = check_against_reference(gpu, shape, PATSETS[0], 3)
    st.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        L.check(st.call(), "cached_head_train_steps (capture)")
    for _ in range(2):
        st.reset()
        graph.replay()
        got = st.result()
        st.intact()
        same(got, eager)
        for k in eager:
            if k.endswith(".outside") or k.endswith(".guard"):
                assert torch.equal(got[k], eager[k]), k


def test_refusals_launch_nothing(gpu):
    shape = SHAPES[0]
    st = State(gpu, shape, PATSETS[0], 3)
    before = st.result()
    elsewhere = torch.zeros(4096, device=gpu)
    other_step = torch.zeros(1, dtype=torch.int64, device=gpu)
    cases = [dict(steps=0), dict(steps=L.CACHED_HEAD_MAX_STEPS + 1), dict(steps=-1),
             dict(dover=dict(gw3=elsewhere.data_ptr())),                        # a gradient outside the Adam range
             dict(dover=dict(gb5=st.flat["grad"].ptr() + 4 * (st.total - 1))),  # ... or running past its end
             dict(dover=dict(w3=st.ptr("param", "w3") + 16)),                   # a weight at another offset
             dict(dover=dict(adam_step=other_step.data_ptr())), dict(dover=dict(adam_step=None)),
             dict(aover=dict(param=None)), dict(aover=dict(grad=None)), dict(aover=dict(exp_avg=None)),
             dict(aover=dict(exp_avg_sq=None)), dict(aover=dict(hyper=None)), dict(aover=dict(count=0)),
             dict(aover=dict(exp_avg=st.flat["exp_avg"].ptr() + 4)),            # 16-byte alignment
             dict(dover=dict(batch=0)), dict(dover=dict(rows=None)), dict(dover=dict(hidden=shape[3] + 2))]
    for kw in cases:
        assert st.call(**kw) == INVALID, kw
    assert L.lib().tspm_cached_head_train_steps(None, st.adam(), 1, L.stream_handle()) == INVALID
    assert L.lib().tspm_cached_head_train_steps(st.desc(), None, 1, L.stream_handle()) == INVALID
    assert st.call(dover=dict(workspace_bytes=15)) == CO.WORKSPACE
    after = st.result()
    st.intact()
    for k, v in before.items():
        assert (after[k] == v) if isinstance(v, int) else torch.equal(
            after[k].view(torch.uint8) if v.dtype.is_floating_point else after[k],
            v.view(torch.uint8) if v.dtype.is_floating_point else v), k
    assert other_step.item() == 0 and not elsewhere.any()
