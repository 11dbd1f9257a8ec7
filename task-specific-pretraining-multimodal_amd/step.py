"""FusedTrainStep — the whole AVMNIST late-fusion train step as one HIP-graph replay.

Replaces the per-batch body of MML_Suite/models/avmnist.py:269-310 (zero_grad → forward →
LossFunctionGroup(CE) → backward → Adam.step) and the backward/optimizer loop of
train_multimodal.py:469-488:

    s0: audio ResNet18 fwd ─┐            ┌─ audio ResNet18 bwd ─┐
    s1: image ResNet34 fwd ─┴─ head fwd ─ CE ─ head bwd ─┴─ image ResNet34 bwd ─┴─ [RCCL] ─ Adam

The two encoders are independent until the fusion concat, so they run as parallel graph branches
on two HIP streams.  Every buffer is allocated once; the first call runs eagerly, the second call
captures the graph, later calls only copy the batch into the static input buffers and replay.
Weight gradients are written straight into FusedAdam's flat gradient buffer (overwrite — no
zero_grad pass); with world_size > 1 the flat buffer is all-reduced between backward and Adam
(``ddp.GradAllReduce``) and 1/world is folded into Adam's gradient scale.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import time
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib as L
from .engine import EncoderEngine, prepare_encoder_layout
from .ddp import PhasedGradAllReduce
from .optim import FusedAdam

NUM_CLASSES = 10


def _ce_weight(loss_functions) -> Optional[float]:
    """Weight of the single cross-entropy term of a LossFunctionGroup (experiment_utils/loss.py:83-148),
    or None when the group is anything else (then the step follows the generic autograd path)."""
    if loss_functions is None:
        return 1.0
    try:
        items = list(loss_functions.items())
    except AttributeError:
        return None
    if len(items) != 1:
        return None
    term = items[0][1]
    fn = getattr(term, "loss_fn", None)
    w = getattr(term, "weight", 1.0)
    if not isinstance(fn, torch.nn.CrossEntropyLoss):
        return None
    if fn.weight is not None or fn.reduction != "mean" or fn.label_smoothing != 0.0:
        return None
    return float(w)


def shared_batches_tracked(model: torch.nn.Module, dev: torch.device,
                           types=(torch.nn.BatchNorm2d,)) -> torch.Tensor:
    """The ``num_batches_tracked`` counters of every BatchNorm2d of ``model`` re-pointed as views of ONE
    int64 device buffer (one add per step instead of one per BN), shared by every fused step of the
    model (e.g. a second one for a partial last batch)."""
    bns = [m for m in model.modules() if isinstance(m, types) and m.num_batches_tracked is not None]
    nbt = getattr(model, "_tspm_nbt", None)
    if not (nbt is not None and nbt.numel() == len(bns) and nbt.device == dev and all(
            m.num_batches_tracked.data_ptr() == nbt[i].data_ptr() for i, m in enumerate(bns))):
        nbt = torch.zeros(len(bns), dtype=torch.int64, device=dev)
        for i, m in enumerate(bns):
            nbt[i] = m.num_batches_tracked.to(dev)
            m.num_batches_tracked = nbt[i]
        model._tspm_nbt = nbt
    return nbt


# tspm_head_train_step's shape limits (csrc/misc.hip: HEAD_MAXIN / HEAD_MAXH / HEAD_MAXH2 / HEAD_MAXC, sizes % 4,
# weights + the 4-row block in at most 160 KiB of LDS — head_lds_floats)
HEAD_MAX_IN, HEAD_MAX_HIDDEN, HEAD_MAX_HIDDEN2, HEAD_MAX_CLASSES = 256, 256, 128, 16


def head_supported(model) -> bool:
    """Python mirror of tspm_head_train_step's argument checks for this model's fusion head: a
    head the kernel would refuse routes AVMNIST.train_step to the autograd path (linear kernels + CE) instead
    of raising on the first fused step."""
    try:
        F = int(model.embd_size_A) + int(model.embd_size_I)
        H = int(model.hidden_dim)
        H2 = H // 2
    except (AttributeError, TypeError):
        return False
    C = NUM_CLASSES
    if not (0 < F <= HEAD_MAX_IN and 0 < H <= HEAD_MAX_HIDDEN and 0 < H2 <= HEAD_MAX_HIDDEN2 and 0 < C <= HEAD_MAX_CLASSES):
        return False
    if F % 4 or H % 4 or H2 % 4:
        return False
    rb = 4  # the larger of the kernel's row blocks (tspm_head_desc.rows_per_block = 4; the default is 1 up to 256 rows)
    ldc = ((C + 3) & ~3) + 4
    floats = H * (F + 4) + H2 * (H + 4) + C * (H2 + 4) + rb * ((F + 4) + (H + 4) + (H2 + 4) + ldc) + (H + H2 + C + rb)
    return floats * 4 <= 160 * 1024


def fused_step_supported(model, optimizer, loss_functions, A: torch.Tensor, I: torch.Tensor) -> bool:
    if os.environ.get("TSPM_DISABLE_FUSED_STEP"):
        return False
    if not isinstance(optimizer, FusedAdam):
        return False
    if _ce_weight(loss_functions) is None:
        return False
    if not (A.is_cuda and I.is_cuda):
        return False
    if not head_supported(model):
        return False
    return A.shape[0] == I.shape[0]


class AdamCarry:
    """Adam updates carried by an encoder's later backward launches (tspm_conv_bwd_adam, ABI 20).

    The backward visits the blocks from the last to the first.  When a block is done its parameters (and, first,
    the fc's) are final and no later launch reads them (``ready``); the next fused dgrad + wgrad launches then carry
    their Adam update as extra workgroups of the same grid (``take``: conv2's launch half of what is pending,
    conv1's the rest), overlapping the latency-bound GEMM tiles instead of following the backward.  Parameters
    are visited in descending flat-buffer order, so what is pending is one contiguous element range of the
    (single) flat group; ``carried`` lists the issued ranges — the caller updates the rest with launch_ranges.
    Bitwise the one-launch update (Adam is element-wise; the carried loop is tspm_adam_step's)."""

    def __init__(self, opt, max_blocks: int = 512, elems_per_block: int = 8192):
        fgs = opt.flat_groups()
        self.fg = fgs[0] if len(fgs) == 1 else None
        self.where = {}
        if self.fg is not None:
            from .optim import _ALIGN
            for p, o in zip(self.fg.params, self.fg.offsets):
                self.where[id(p)] = (o, o + (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN)
        self.lo = self.hi = None  # pending [lo, hi)
        self.carried: List[Tuple[int, int]] = []
        self.max_blocks = max_blocks
        self.elems_per_block = elems_per_block

    def ready(self, params) -> None:
        spans = [self.where.get(id(p)) for p in params]
        if not spans or any(sp is None for sp in spans):
            return
        # the block's spans must tile [a, b) exactly: with a parameter order that interleaves another block's (or
        # the other encoder's) parameters into this range, [min, max) would cover elements whose gradients may
        # still be in flight — such a block stays with the optimizer's own launches
        spans = sorted(spans)
        if any(spans[i][1] != spans[i + 1][0] for i in range(len(spans) - 1)):
            return
        a, b = spans[0][0], spans[-1][1]
        if self.lo is None:
            self.lo, self.hi = a, b
        elif b == self.lo:
            self.lo = a
        # anything else (not adjacent) stays with the caller's own launches

    def take(self, share: float):
        if self.lo is None or share <= 0:
            return None
        n = self.hi - self.lo
        k = n if share >= 1 else min(n, (int(n * share) + 3) // 4 * 4)
        if k <= 0:
            return None
        a, b = self.hi - k, self.hi
        self.hi = a
        if self.hi <= self.lo:
            self.lo = self.hi = None
        self.carried.append((a, b))
        fg = self.fg
        blocks = max(1, min(self.max_blocks, -(-k // self.elems_per_block)))
        return L.AdamJob(fg.param[a:].data_ptr(), fg.grad[a:].data_ptr(), fg.exp_avg[a:].data_ptr(),
                         fg.exp_avg_sq[a:].data_ptr(), k, fg.hyper.data_ptr(), blocks, 0)

    def rest_of(self, ranges):
        """``ranges`` (per group, list of [a, b)) minus the carried ranges."""
        if self.fg is None or not self.carried:
            return ranges
        out = []
        cut = sorted(self.carried)
        for a, b in ranges[0]:
            cur = a
            for c, d in cut:
                if d <= cur or c >= b:
                    continue
                if c > cur:
                    out.append((cur, c))
                cur = max(cur, d)
            if cur < b:
                out.append((cur, b))
        return [out] + list(ranges[1:])


class FusedTrainStep(L.GraphRunner):
    def __init__(self, model, optimizer: FusedAdam, loss_functions, batch: int, audio_hw=(32, 94), image_hw=(28, 28),
                 use_graph: bool = True, allreduce=None, adam_split=True):
        self.model = model
        self.opt = optimizer
        self.loss_functions = loss_functions
        self.ce_weight = _ce_weight(loss_functions)
        if not head_supported(model):
            raise L.TspmError("FusedTrainStep: the fusion head's shape is outside tspm_head_train_step's limits "
                              "(use AVMNIST.train_step, which routes such heads to the autograd path)")
        if head_stage_frozen(model):  # (refuses the unsupported flag combinations itself, naming the parameter)
            raise L.TspmError("FusedTrainStep trains every parameter; a model with frozen encoders "
                              f"{head_stage_frozen(model)} trains with FusedHeadStageStep (AVMNIST.train_step routes it)")
        self.N = batch
        self.allreduce = allreduce
        p0 = next(model.parameters())
        dev = p0.device
        self._init_graph(use_graph, dev)  # graph: forward + backward (+ Adam on one GPU); key (log, keep-mask mode)
        model.train()
        prepare_encoder_layout(model.audio_encoder)
        prepare_encoder_layout(model.image_encoder)
        # flat grads must exist for every parameter (FusedAdam set them as views)
        for p in model.parameters():
            if p.requires_grad and p.grad is None:
                raise L.TspmError("FusedTrainStep: parameter without a FusedAdam gradient view")
        self.eng_a = EncoderEngine(model.audio_encoder, batch, audio_hw[0], audio_hw[1], dev)
        self.eng_i = EncoderEngine(model.image_encoder, batch, image_hw[0], image_hw[1], dev)
        f32 = dict(device=dev, dtype=torch.float32)
        ea, ei = model.embd_size_A, model.embd_size_I
        self.F = ea + ei
        hd = model.hidden_dim
        self.hd, self.h2 = hd, hd // 2
        self.A = torch.empty(batch, audio_hw[0], audio_hw[1], **f32)
        self.I = torch.empty(batch, 1, image_hw[0], image_hw[1], **f32)
        self.labels = torch.zeros(batch, dtype=torch.int64, device=dev)
        self.groups = torch.zeros(batch, dtype=torch.int32, device=dev)  # pattern id per row (metrics)
        # metrics.ClassificationLog: when set, the step also records predictions / confusion counts /
        # the batch loss on the device (train metrics of the epoch, train_multimodal.py:478-491,607-612)
        self.log = None
        self.fused = torch.empty(batch, self.F, **f32)
        self.h1 = torch.empty(batch, hd, **f32)
        self.hh = torch.empty(batch, self.h2, **f32)
        self.logits = torch.empty(batch, NUM_CLASSES, **f32)
        self.dlogits = torch.empty(batch, NUM_CLASSES, **f32)
        self.dh = torch.empty(batch, self.h2, **f32)     # fc3 pre-activation gradient
        self.dh1 = torch.empty(batch, hd, **f32)         # fc0 pre-activation gradient
        self.dfused = torch.empty(batch, self.F, **f32)
        self.row_ws = torch.empty(2 * batch, **f32)       # per-row CE / correct flags (tspm_head_train_step)
        self.keep = torch.ones(batch, hd, dtype=torch.uint8, device=dev)
        self.loss = torch.zeros(1, **f32)
        self.stats = torch.zeros(4, **f32)  # loss*n, correct, n (accumulated on device)
        self.keep_override: Optional[torch.Tensor] = None
        self.nbt = shared_batches_tracked(model, dev)
        # the image encoder's branch runs on a side stream; the DP exchange on a third (one set per process,
        # shared by every step build: L.shared_streams)
        self.side, self.comm = L.shared_streams(dev, 2)
        self.serial = os.environ.get("TSPM_SERIAL", "0") == "1"  # True: one stream (per-kernel timing)
        # the audio encoder's LDS-staged convs with an 82,000-byte LDS floor: one workgroup per CU, leaving room
        # for the image chain, the replayed step's critical path (scripts/overlap_probe.py --dump: image forward +
        # head + image backward + image Adam).  A/B, alternating processes: 2.5907 vs 2.6280 ms (56,000 bytes:
        # 2.613 vs 2.630), profiles/r5/r5i_floor*.json.  TSPM_SLACK_LDS_FLOOR=0 restores the unconstrained launches
        # At batch 1024 the floor costs 1.05 ms per step (10.84 vs 9.79 ms, profiles/r5/r5t_floor_b1024.json: the
        # audio chain's large convs need their occupancy there) and at batch 32 it is neutral (2.6497 vs 2.6459 ms,
        # r5u_floor_b32.json), so the default applies at batches 64-128 only
        self.slack_lds_floor = int(os.environ.get("TSPM_SLACK_LDS_FLOOR", "82000" if 64 <= batch <= 128 else "0"))
        self.slack_parts = os.environ.get("TSPM_SLACK_PARTS", "fb")  # the audio forward (f) and / or backward (b)
        # Adam updates of finished blocks carried by the later backward launches of "image" / "audio" / "both"
        # encoders (AdamCarry; single-GPU split schedule only); "none" = the optimizer's own launches.  A/B,
        # alternating processes (profiles/r5/r5n-r5p): both 2.5526 vs 2.5931 ms with 512 carrying workgroups of
        # 8,192 elements (256 x 16,384: 2.5571 vs 2.5933; image only: 2.5692 vs 2.5965); batch 1024: 9.807 vs
        # 9.866 ms (r5u_carry_b1024.json)
        self.adam_carry = os.environ.get("TSPM_ADAM_CARRY", "both")
        # the head's samples per workgroup (tspm_head_desc.rows_per_block, ABI 21): 0 = the library's default (1 up
        # to 256 rows, else 4); TSPM_HEAD_RB=1 / 4 forces one for A/B (read here, not inside the library)
        self.head_rows_per_block = int(os.environ.get("TSPM_HEAD_RB", "0"))
        self.graph_opt: Optional[torch.cuda.CUDAGraph] = None  # plain DP step: Adam, replayed behind the all-reduce
        # single-GPU step (adam_split): each encoder's parameters updated by Adam on that encoder's stream right
        # after its own backward (the image encoder's beside the audio chain's tail), the head's with the audio
        # encoder's; bitwise the one-launch update (Adam is element-wise).  A cross-stream edge in the middle of
        # the two chains (e.g. the audio layer3/4 update moved to the image stream) serialised the replayed
        # graph: 3.55 ms vs 2.64 (profiles/r4/r4f_ab_adam_schedules.json)
        self.adam_split = adam_split
        # bench.py's exchange block: when a list, the phased DP step appends per step the host's waits for
        # the two step flags and a pair of events (graph end, step end) bracketing the exposed exchange tail
        self.exchange_probe: Optional[list] = None
        self._split_ranges = None
        self._head_bumps_step = False
        self._sig = (id(optimizer), id(loss_functions), batch)
        # dropout RNG counter = FusedAdam's device step counter (distinct per step, graph-safe)
        fgs = optimizer.flat_groups()
        self._rng_ctr_ptr = fgs[0].hyper.data_ptr() + L.HYPER_STEP_OFFSET if fgs else None

    def matches(self, A, I, optimizer, loss_functions) -> bool:
        return self._sig == (id(optimizer), id(loss_functions), A.shape[0]) and tuple(A.shape[1:]) in (
            tuple(self.A.shape[1:]),) and tuple(I.shape[-2:]) == tuple(self.I.shape[-2:])

    # ------------------------------------------------------------------------------------------
    def _head(self, sh: int) -> None:
        """The fusion head's forward, the loss group's cross-entropy and the head's backward in two launches
        (tspm_head_train_step, ABI 16; MML_Suite/models/avmnist.py:219-230,267, experiment_utils/loss.py:98-148):
        h1 / hh / logits / loss, the dropout keep mask (drawn on the device from the step counter unless
        keep_override was copied in), the net.{0,3,5} weight and bias gradients into FusedAdam's flat
        buffer, and dfused = the gradient into both encoders' embeddings."""
        net = self.model.net
        p = float(self.model.dropout_p)
        g = lambda t: t.data_ptr()  # noqa: E731
        d = L.HeadDesc(n=self.N, in_=self.F, hidden=self.hd, hidden2=self.h2, classes=NUM_CLASSES, ldx=self.F,
                       lddx=self.F, gen_keep=1 if (p > 0 and self.keep_override is None) else 0,
                       x=g(self.fused), w0=g(net[0].weight), b0=g(net[0].bias), w3=g(net[3].weight), b3=g(net[3].bias),
                       w5=g(net[5].weight), b5=g(net[5].bias), p=p, loss_weight=self.ce_weight,
                       seed=int(self.model._rng_seed) if p > 0 else 0, counter=self._rng_ctr_ptr if p > 0 else None,
                       keep=g(self.keep), labels=g(self.labels), h1=g(self.h1), hh=g(self.hh), logits=g(self.logits),
                       dlogits=g(self.dlogits), dz3=g(self.dh), dz0=g(self.dh1), dx=g(self.dfused), row_ws=g(self.row_ws),
                       gw0=g(net[0].weight.grad), gb0=g(net[0].bias.grad), gw3=g(net[3].weight.grad),
                       gb3=g(net[3].bias.grad), gw5=g(net[5].weight.grad), gb5=g(net[5].bias.grad),
                       loss=g(self.loss), stats=g(self.stats),
                       adam_step=self._rng_ctr_ptr if self._head_bumps_step else None,
                       rows_per_block=self.head_rows_per_block)
        L.check(L.lib().tspm_head_train_step(d, sh), "head_train_step")

    def _fwd_bwd(self, marks=None) -> None:
        """Enqueue forward + loss + backward on the current stream (+ the side stream for the image encoder).
        ``marks``: two ``_lib.DeviceFlag``s bumped after the audio / image encoder's backward phase 1 (fc,
        layer4, layer3: the same launches, split at the phase boundary), which the DP exchange waits on outside
        the graph (_run_phased)."""
        main = torch.cuda.current_stream()
        ea = self.model.embd_size_A
        side = main if self.serial else self.side
        side.wait_stream(main)
        with torch.cuda.stream(side):
            self.eng_i.forward(self.I, self.fused[:, ea:], self.F, train=True, bump_batches_tracked=False)
        with self._slack_floor("f"):
            self.eng_a.forward(self.A, self.fused, self.F, train=True, bump_batches_tracked=False)
        main.wait_stream(side)
        sh = main.cuda_stream
        # the single-GPU split schedule with one flat group: the head's second launch advances the Adam step
        # counter (tspm_head_desc.adam_step) instead of a tspm_adam_begin launch before the fork
        self._head_bumps_step = (marks is None and self._split_opt() and len(self.opt.flat_groups()) == 1
                                 and os.environ.get("TSPM_HEAD_BUMPS_STEP", "1") != "0")
        # (the head's weight-gradient launch on the image stream, beside the audio backward, was measured slower:
        # 2.604 vs 2.589 ms, profiles/r4/r4m2_ab_head.json)
        self._head(sh)
        self._classify(sh)
        side.wait_stream(main)
        if marks is not None:
            mark_a, mark_i = marks
            with self._slack_floor():
                self.eng_a.backward(self.dfused, self.F, phase=1)
            mark_a.bump(main)
            with torch.cuda.stream(side):
                self.eng_i.backward(self.dfused[:, ea:], self.F, phase=1)
                mark_i.bump(side)
            with self._slack_floor():
                self.eng_a.backward(None, self.F, phase=2)
            with torch.cuda.stream(side):
                self.eng_i.backward(None, self.F, phase=2)
        elif self._split_opt():
            img, rest = self._adam_ranges()
            if not self._head_bumps_step:
                self.opt.launch_begin(main.cuda_stream)  # one step-count increment, before every range
            side.wait_stream(main)
            # each encoder's parameters on its own stream at its chain's end, the head's with the audio encoder's
            # (the increment on the image stream and main joining it before the audio + head ranges, with
            # num_batches_tracked moved to the image stream's start: 2.614 vs 2.595 ms, profiles/r4/r4q_ab_lean.json)
            kw = dict(max_blocks=int(os.environ.get("TSPM_ADAM_CARRY_BLOCKS", "512")),
                      elems_per_block=int(os.environ.get("TSPM_ADAM_CARRY_ELEMS", "8192")))
            ci = AdamCarry(self.opt, **kw) if self.adam_carry in ("image", "both") else None
            ca = AdamCarry(self.opt, **kw) if self.adam_carry in ("audio", "both") else None
            with torch.cuda.stream(side):
                self.eng_i.adam_carry = ci
                try:
                    self.eng_i.backward(self.dfused[:, ea:], self.F)
                finally:
                    self.eng_i.adam_carry = None
                self.opt.launch_ranges(side.cuda_stream, ci.rest_of(img) if ci else img)
            with self._slack_floor():
                self.eng_a.adam_carry = ca
                try:
                    self.eng_a.backward(self.dfused, self.F)
                finally:
                    self.eng_a.adam_carry = None
            self.opt.launch_ranges(main.cuda_stream, ca.rest_of(rest) if ca else rest)
        else:
            with torch.cuda.stream(side):
                self.eng_i.backward(self.dfused[:, ea:], self.F)
            with self._slack_floor():
                self.eng_a.backward(self.dfused, self.F)
        main.wait_stream(side)
        L.counters_add(self.nbt)

    @contextlib.contextmanager
    def _slack_floor(self, part: str = "b"):
        """The audio encoder's LDS-staged conv launches with a minimum LDS allocation (TSPM_SLACK_LDS_FLOOR bytes,
        passed per launch as tspm_conv_algo.lds_floor — ABI 21, no library state), so fewer of its workgroups share
        a CU with the image chain (the replayed step's critical path, scripts/overlap_probe.py --dump).  The floor
        lives on this step's own audio engine and only while its launches are enqueued."""
        floor = self.slack_lds_floor if part in self.slack_parts else 0
        if floor and not self.serial:
            self.eng_a.lds_floor = floor
        try:
            yield
        finally:
            self.eng_a.lds_floor = 0

    def _split_opt(self) -> bool:
        """Adam launched per encoder inside the fwd/bwd enqueue (single GPU, no gradient clipping: the
        range launches have no clip-coefficient form)."""
        return bool(self.adam_split) and self.allreduce is None and getattr(self.opt, "clip_coef", None) is None

    def _adam_ranges(self):
        """FusedAdam flat-buffer ranges per group of (image encoder, audio encoder + head)."""
        if self._split_ranges is None:
            from .ddp import flat_ranges
            img = {id(p) for p in self.model.image_encoder.parameters()}
            out = ([], [])
            for fg in self.opt.flat_groups():
                numels = [p.numel() for p in fg.params]
                sel = [id(p) in img for p in fg.params]
                out[0].append(flat_ranges(fg.offsets, numels, fg.numel, sel))
                out[1].append(flat_ranges(fg.offsets, numels, fg.numel, [not x for x in sel]))
            self._split_ranges = out
        return self._split_ranges

    def phased_allreduce(self, force: bool = False, bucket_mb: float = 64.0, group=None):
        """The overlapped DP exchange for this step: gradient ranges of FusedAdam's flat buffers in
        three phases — (0) head + audio fc/layer4/layer3, (1) image fc/layer4/layer3, (2) both
        encoders' layer2/layer1/stem — each launched as soon as the backward part that writes it
        has run (see _run_phased)."""
        from .ddp import PhasedGradAllReduce, flat_ranges
        sets = [{id(p) for p in self.eng_a.phase_params(1)} | {id(p) for p in self.model.net.parameters()},
                {id(p) for p in self.eng_i.phase_params(1)},
                {id(p) for p in self.eng_a.phase_params(2) + self.eng_i.phase_params(2)}]
        views = [[], [], []]
        ranges = ([], [], [])  # per phase, per flat group: the element ranges (Adam after that phase's exchange)
        for fg in self.opt.flat_groups():
            for p in fg.params:
                if sum(id(p) in st for st in sets) != 1:
                    raise L.TspmError("phased all-reduce: parameter not owned by exactly one backward phase")
            numels = [p.numel() for p in fg.params]
            for k, st in enumerate(sets):
                rk = flat_ranges(fg.offsets, numels, fg.numel, [id(p) in st for p in fg.params])
                ranges[k].append(rk)
                views[k] += [fg.grad[a:b] for a, b in rk]
        self._phase_ranges = ranges
        return PhasedGradAllReduce(views, bucket_mb=bucket_mb, group=group, force=force)

    def _run_phased(self) -> None:
        """DP step with the RCCL exchange overlapped with backward, the whole forward + backward as ONE
        HIP graph (the plain step's two-stream schedule), and each phase's Adam update right behind that
        phase's exchange:
             main (graph): [fwd both + head + audio bwd late ─●─ audio bwd early] ─ RCCL(both early) ─ Adam(early)
             side (graph):                   [image bwd late ─●─ image bwd early] ─┘
             comm:          RCCL(head+audio late) ─ Adam(head+audio late) · RCCL(image late) ─ Adam(image late)
        ● = a step flag (``_lib.DeviceFlag``: a one-thread kernel in the graph publishes a per-step count to
        pinned host memory; the host waits for it before launching the collective — ROCm 7 refuses
        graph-external event records); the collectives run on RCCL's stream, each after the flag of the
        backward part that writes its gradients, and the comm / main streams wait for them before the Adam
        ranges of the same parameters (phase 2's backward reads none of the phase-0/1 parameters).  Adam is
        element-wise, so the per-phase ranges give bitwise the one-launch update."""
        ar = self.allreduce
        if getattr(self.opt, "clip_coef", None) is not None:
            # the per-phase Adam ranges have no clip-coefficient form: refuse instead of ignoring it
            raise L.TspmError("phased DP step: FusedAdam.clip_coef is set, but the per-phase Adam ranges cannot "
                              "apply a clip coefficient; use the plain DP step (allreduce=GradAllReduce)")
        if getattr(self, "_marks", None) is None:
            self._marks = (L.DeviceFlag(), L.DeviceFlag())
        if getattr(self, "_phase_ranges", None) is None:
            raise L.TspmError("phased step: build the exchange with FusedTrainStep.phased_allreduce()")
        self._replay_step(lambda: self._fwd_bwd(marks=self._marks), opt_graph=False)
        # each flag is bumped once per step, after (in graph order) everything main ran before this step
        # (batch upload, the previous step's Adam reading the gradients): once the host has seen it, the
        # gradients it covers are complete, so the exchange launched then needs no device-side wait
        for f in self._marks:
            f.count += 1
        main, comm, r = torch.cuda.current_stream(), self.comm, self._phase_ranges
        probe = self.exchange_probe
        if probe is not None:  # the graph's end on main (the side stream joined it inside the graph)
            ev_graph = torch.cuda.Event(enable_timing=True)
            ev_graph.record(main)
            t0 = time.perf_counter()
        self._marks[0].host_wait(self._marks[0].count)
        if probe is not None:
            t1 = time.perf_counter()
        with torch.cuda.stream(comm):
            ar.wait(ar.launch(0))
            self.opt.launch_begin(comm.cuda_stream)  # one step-count increment, before every range
            self.opt.launch_ranges(comm.cuda_stream, r[0])
        if probe is not None:
            t2 = time.perf_counter()
        self._marks[1].host_wait(self._marks[1].count)
        if probe is not None:
            t3 = time.perf_counter()
        with torch.cuda.stream(comm):
            ar.wait(ar.launch(1))
            self.opt.launch_ranges(comm.cuda_stream, r[1])
        ar.wait(ar.launch(2))  # on main, behind the graph: no stream hop before the last exchange
        main.wait_stream(comm)  # the step-count increment and the phase-0/1 updates before the step ends
        self.opt.launch_ranges(main.cuda_stream, r[2])
        if probe is not None:
            ev_end = torch.cuda.Event(enable_timing=True)
            ev_end.record(main)
            # the window each late phase's exchange has to hide in: from the host seeing that phase's flag to the
            # end of the fwd+bwd graph (the rest of the backward), host clock, the graph's end polled (probe only)
            while not ev_graph.query():
                pass
            t4 = time.perf_counter()
            probe.append({"host_wait_ms": ((t1 - t0) * 1e3, (t3 - t2) * 1e3), "events": (ev_graph, ev_end),
                          "window_ms": ((t4 - t1) * 1e3, (t4 - t3) * 1e3)})

    def close(self) -> None:
        """Release the step's device-side resources in a safe order, before the process group goes away
        (bench.py, the DP tests): wait for every stream (the graph's two, the exchange stream, RCCL's via the
        device), drop the captured graphs (they bump the step flags), then free the flags.  Idempotent; the
        step is unusable afterwards."""
        if getattr(self, "_closed", False):
            return
        self._closed = True
        torch.cuda.synchronize(self.device)
        self.graph, self.graph_opt = None, None
        marks, self._marks = getattr(self, "_marks", None), None
        if marks is not None:
            for f in marks:
                f.close()
        self.allreduce = None
        self.exchange_probe = None

    def _classify(self, sh: int) -> None:
        log = self.log
        if log is None:
            return
        L.check(L.lib().tspm_classify_update(
            self.N, NUM_CLASSES, self.logits.data_ptr(), self.labels.data_ptr(), self.groups.data_ptr(),
            len(log.groups), log.conf.data_ptr(), None, self.loss.data_ptr(), log.loss_log.data_ptr(),
            log.counters.data_ptr(), log.capacity, sh), "classify_update")

    def _opt(self) -> None:
        self.opt.launch(torch.cuda.current_stream().cuda_stream)

    def _enqueue_all(self) -> None:
        self._fwd_bwd()
        if self.allreduce is None and not self._split_opt():
            self._opt()

    # ------------------------------------------------------------------------------------------
    def load_batch(self, A: torch.Tensor, I: torch.Tensor, labels: torch.Tensor,
                   groups: Optional[torch.Tensor] = None) -> None:
        if groups is not None and groups.data_ptr() != self.groups.data_ptr():
            self.groups.copy_(groups.reshape(-1).to(torch.int32), non_blocking=True)
        if A.data_ptr() != self.A.data_ptr():
            self.A.copy_(A.reshape(self.A.shape), non_blocking=True)
        if I.data_ptr() != self.I.data_ptr():
            self.I.copy_(I.reshape(self.I.shape), non_blocking=True)
        if labels.data_ptr() != self.labels.data_ptr():
            self.labels.copy_(labels, non_blocking=True)

    def step(self, A: torch.Tensor, I: torch.Tensor, labels: torch.Tensor,
             groups: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        self.load_batch(A, I, labels, groups)
        self.run()
        return {"loss": self.loss, "logits": self.logits}

    def run(self) -> None:
        """One training step on the batch currently in the static input buffers."""
        if getattr(self, "_closed", False):
            raise L.TspmError("FusedTrainStep.run after close()")
        self.model.train()
        self.opt.sync_hyper()
        if self.keep_override is not None:
            self.keep.copy_(self.keep_override.reshape(self.keep.shape).to(torch.uint8), non_blocking=True)
        if isinstance(self.allreduce, PhasedGradAllReduce):
            self._run_phased()
            self.opt.note_steps(1)
            self.calls += 1
            return
        self._replay_step(self._enqueue_all, opt_graph=self.allreduce is not None)
        if self.allreduce is not None:
            self.allreduce()
            if self.use_graph and self.graph_opt is not None:
                self.graph_opt.replay()
            else:
                self._opt()
        self.opt.note_steps(1)
        self.calls += 1

    def _replay_step(self, enqueue, opt_graph: bool) -> None:
        """``enqueue`` through the runner.  The graph bakes in the metrics log and whether the head draws its keep mask
        or reads the copied-in one.  ``graph_opt`` (``opt_graph``: Adam alone, for the plain DP step) lives and dies
        with ``graph``: dropped when that is found None, captured again right after it."""
        if self.graph is None:
            self.graph_opt = None
        if self.replay_or_enqueue(enqueue, (self.log, self.keep_override is None)):
            self.graph_opt = self.capture_graph(self._opt) if opt_graph else None


class FusedEvalStep(L.GraphRunner):
    """AVMNIST.validation_step (MML_Suite/models/avmnist.py:312-360) as one HIP graph: both encoders in
    eval mode (BatchNorm running statistics) on two streams, the fusion head without dropout, the loss
    (LossFunctionGroup total = weight × CE) and ``tspm_classify_update`` — predictions, per-pattern
    confusion counts and the per-batch loss go to a :class:`metrics.ClassificationLog` on the device,
    so an evaluation epoch has no host round trip per batch.  Shares the encoders' cached HIP plans
    (``ResNetEncoder.engine_for``) with the module forward."""

    def __init__(self, model, loss_functions, batch: int, log=None, audio_hw=(32, 94), image_hw=(28, 28),
                 use_graph: bool = True):
        self.model, self.N, self.log = model, batch, log
        self.ce_weight = _ce_weight(loss_functions)
        if self.ce_weight is None:
            raise L.TspmError("FusedEvalStep: the loss group must be a single cross-entropy term")
        dev = next(model.parameters()).device
        self._init_graph(use_graph, dev)  # key: (log,)
        f32 = dict(device=dev, dtype=torch.float32)
        self.A = torch.zeros(batch, audio_hw[0], audio_hw[1], **f32)
        self.I = torch.zeros(batch, 1, image_hw[0], image_hw[1], **f32)
        self.labels = torch.zeros(batch, dtype=torch.int64, device=dev)
        self.groups = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.eng_a = model.audio_encoder.engine_for(self.A)
        self.eng_i = model.image_encoder.engine_for(self.I)
        ea, ei = model.embd_size_A, model.embd_size_I
        self.F, self.hd = ea + ei, model.hidden_dim
        self.fused = torch.empty(batch, self.F, **f32)
        self.h1 = torch.empty(batch, self.hd, **f32)
        self.hh = torch.empty(batch, self.hd // 2, **f32)
        self.logits = torch.empty(batch, NUM_CLASSES, **f32)
        self.loss = torch.zeros(1, **f32)
        self.preds = torch.zeros(batch, dtype=torch.int64, device=dev)
        self.side = L.shared_streams(dev, 1)[0]

    def load_batch(self, A: torch.Tensor, I: torch.Tensor, labels: torch.Tensor,
                   groups: Optional[torch.Tensor] = None) -> None:
        for dst, src in ((self.A, A), (self.I, I), (self.labels, labels)):
            if src.data_ptr() != dst.data_ptr():
                dst.copy_(src.reshape(dst.shape), non_blocking=True)
        if groups is not None and groups.data_ptr() != self.groups.data_ptr():
            self.groups.copy_(groups.reshape(-1).to(torch.int32), non_blocking=True)

    def _enqueue(self) -> None:
        lib = L.lib()
        main = torch.cuda.current_stream()
        ea = self.model.embd_size_A
        self.side.wait_stream(main)
        with torch.cuda.stream(self.side):
            self.eng_i.forward(self.I, self.fused[:, ea:], self.F, train=False)
        self.eng_a.forward(self.A, self.fused, self.F, train=False)
        main.wait_stream(self.side)
        sh = main.cuda_stream
        n, F, hd, h2 = self.N, self.F, self.hd, self.hd // 2
        net = self.model.net
        L.check(lib.tspm_linear_fwd(n, F, hd, self.fused.data_ptr(), F, net[0].weight.data_ptr(),
                                    net[0].bias.data_ptr(), 1, None, 1.0, self.h1.data_ptr(), hd, sh), "eval fc0")
        L.check(lib.tspm_linear_fwd(n, hd, h2, self.h1.data_ptr(), hd, net[3].weight.data_ptr(),
                                    net[3].bias.data_ptr(), 1, None, 1.0, self.hh.data_ptr(), h2, sh), "eval fc3")
        L.check(lib.tspm_linear_fwd(n, h2, NUM_CLASSES, self.hh.data_ptr(), h2, net[5].weight.data_ptr(),
                                    net[5].bias.data_ptr(), 0, None, 1.0, self.logits.data_ptr(), NUM_CLASSES, sh),
                "eval fc5")
        L.check(lib.tspm_cross_entropy(n, NUM_CLASSES, self.logits.data_ptr(), self.labels.data_ptr(),
                                       self.loss.data_ptr(), None, self.ce_weight, None, sh), "eval cross_entropy")
        log = self.log
        L.check(lib.tspm_classify_update(
            n, NUM_CLASSES, self.logits.data_ptr(), self.labels.data_ptr(), self.groups.data_ptr(),
            len(log.groups) if log is not None else 1, log.conf.data_ptr() if log is not None else None,
            self.preds.data_ptr(), self.loss.data_ptr(), log.loss_log.data_ptr() if log is not None else None,
            log.counters.data_ptr() if log is not None else None, log.capacity if log is not None else 0, sh),
            "eval classify_update")

    def run(self) -> None:
        """Evaluate the batch in the static input buffers (logits, loss, preds; log updated)."""
        self.model.eval()
        self.replay_or_enqueue(self._enqueue, (self.log,))
        self.calls += 1

    def step(self, A, I, labels, groups=None) -> Dict[str, torch.Tensor]:
        self.load_batch(A, I, labels, groups)
        self.run()
        return {"loss": self.loss, "logits": self.logits, "preds": self.preds}


# the AVMNIST missing-modality patterns in ``data.AVMNIST.get_all_possible_patterns()`` order (the classification log's
# group order) and the (audio, image) inputs each keeps
AVMNIST_PATTERNS = ("a", "ai", "i")
PATTERN_KEEP = {"a": (1, 0), "ai": (1, 1), "i": (0, 1)}


def norm_avmnist_patterns(patterns=None) -> Tuple[str, ...]:
    """The patterns of a fused-pattern pass as a tuple of names: all three in ``AVMNIST_PATTERNS`` order by default, or
    the given subset in the given order.  Unknown names raise ``ValueError``; an empty or repeating selection too."""
    if patterns is None:
        return AVMNIST_PATTERNS
    pats = tuple(str(p) for p in patterns)
    bad = set(pats) - set(AVMNIST_PATTERNS)
    if bad:
        raise ValueError(f"Invalid patterns: {bad}\nValid patterns are: {list(AVMNIST_PATTERNS)}")
    if not pats or len(set(pats)) != len(pats):
        raise ValueError(f"patterns: 1..{len(AVMNIST_PATTERNS)} distinct names among {AVMNIST_PATTERNS}, got {pats!r}")
    return pats


# the head of a FusedPatternEvalStep built without head=: "kernel" (tspm_pattern_head_eval) or "launches" (the same
# result from tspm_pattern_expand + tspm_linear_fwd + tspm_cross_entropy + tspm_classify_update); the leg
# that measured faster at batch 128 (profiles/avmnist_patterns.json)
DEFAULT_PATTERN_HEAD = "kernel"


class FusedPatternEvalStep(L.GraphRunner):
    """AVMNIST.validation_step for EVERY missing-modality pattern of a batch from one encoder pass, as one HIP graph.
    In eval mode an encoder's output row depends on that row's input and the weights only, so the embedding of a zeroed
    spectrogram / image is one constant row per encoder (``AVMNIST.zero_embeddings``): the graph holds both encoders
    over the B real rows (two streams) into ``fused [B, F]``, then the head over the P·B (pattern, sample) rows —
    ``head="kernel"``: one ``tspm_pattern_head_eval`` call; ``head="launches"``: a copy-expand to ``[P·B, F]``, three
    ``tspm_linear_fwd`` and per pattern ``tspm_cross_entropy`` + ``tspm_classify_update`` on the row slice (the A/B leg,
    and the fallback for a head outside the kernel's limits).  Either way the log receives P loss entries per batch in
    pattern order and every row's confusion count under its pattern's group.

    ``step(A, I, labels, refresh_zero=True)`` → ``{"loss": [P], "logits": [P, B, C], "preds": [P, B]}`` (views of the
    static outputs).  The zero embeddings are refreshed before each step unless ``refresh_zero=False`` (an evaluation
    epoch refreshes once: weights do not change inside it)."""

    def __init__(self, model, loss_functions, batch: int, log=None, patterns=None, head: Optional[str] = None,
                 audio_hw=(32, 94), image_hw=(28, 28), use_graph: bool = True):
        self.model, self.N, self.log = model, batch, log
        self.ce_weight = _ce_weight(loss_functions)
        if self.ce_weight is None:
            raise L.TspmError("FusedPatternEvalStep: the loss group must be a single cross-entropy term")
        self.patterns = norm_avmnist_patterns(patterns)
        self.P = P = len(self.patterns)
        ea, ei = int(model.embd_size_A), int(model.embd_size_I)
        self.ea, self.F, self.hd, self.h2 = ea, ea + ei, int(model.hidden_dim), int(model.hidden_dim) // 2
        head = DEFAULT_PATTERN_HEAD if head is None else head
        if head not in ("kernel", "launches"):
            raise ValueError(f"head: 'kernel' or 'launches', got {head!r}")
        if head == "kernel" and not L.pattern_head_eval_supported(self.F, ea, self.hd, self.h2, NUM_CLASSES, P):
            head = "launches"
        self.head = head
        dev = next(model.parameters()).device
        self._init_graph(use_graph, dev)  # key: (log, the zero-row buffer's address)
        self.audio_hw, self.image_hw = tuple(audio_hw), tuple(image_hw)
        f32 = dict(device=dev, dtype=torch.float32)
        self.A = torch.zeros(batch, audio_hw[0], audio_hw[1], **f32)
        self.I = torch.zeros(batch, 1, image_hw[0], image_hw[1], **f32)
        self.labels = torch.zeros(batch, dtype=torch.int64, device=dev)
        self.eng_a = model.audio_encoder.engine_for(self.A)
        self.eng_i = model.image_encoder.engine_for(self.I)
        self.x0 = model.zero_embeddings(refresh=False, audio_hw=self.audio_hw, image_hw=self.image_hw)
        self._alloc_head(dev, batch, head)
        self.side = L.shared_streams(dev, 1)[0]

    def _alloc_head(self, dev, batch: int, head: str) -> None:
        """The outputs, the host arrays of the launch arguments and the buffers of the head leg ``head`` — everything
        ``_head_kernel`` / ``_head_launches`` touch besides ``labels`` and ``x0`` (``FusedCachedEvalStep`` shares it)."""
        P, ea, ei = self.P, self.ea, self.F - self.ea
        f32 = dict(device=dev, dtype=torch.float32)
        self.logits = torch.empty(P * batch, NUM_CLASSES, **f32)
        self.loss = torch.zeros(P, **f32)
        self.preds = torch.zeros(P * batch, dtype=torch.int64, device=dev)
        # host arrays of the launch arguments (read at enqueue time only)
        self._keep = (ctypes.c_int32 * (2 * P))(*[k for p in self.patterns for k in PATTERN_KEEP[p]])
        self._gid = (ctypes.c_int32 * P)()
        if head == "kernel":
            self.fused = torch.empty(batch, self.F, **f32)
            need = int(L.lib().tspm_pattern_head_eval_workspace(batch, P))
            self.ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        else:
            # tspm_pattern_expand's layout: rows [0, B) the real embeddings (the encoders write them), rows [B, 2B)
            # the zero-input embeddings of the same rows — here one constant row, broadcast.  The entry point takes
            # three modality widths: the image embedding's columns go in as two halves under the same keep flag
            self.emb2 = torch.empty(2 * batch, self.F, **f32)
            self.fused = self.emb2[:batch]
            self._widths = (ea, ei // 2, ei - ei // 2)
            self._keep3 = (ctypes.c_int32 * (3 * P))(*[k for p in self.patterns
                                                        for k in (PATTERN_KEEP[p][0],) + (PATTERN_KEEP[p][1],) * 2])
            self.x = torch.empty(P * batch, self.F, **f32)
            self.h1 = torch.empty(P * batch, self.hd, **f32)
            self.hh = torch.empty(P * batch, self.h2, **f32)
            self.labels_x = torch.zeros(P * batch, dtype=torch.int64, device=dev)
            self.groups = torch.zeros(P * batch, dtype=torch.int32, device=dev)

    def _group_ids(self) -> List[int]:
        """Each pattern's group in the log (its position among the log's groups; without a log, among all patterns)."""
        gid = self.log.gid if self.log is not None else {p: i for i, p in enumerate(AVMNIST_PATTERNS)}
        try:
            return [int(gid[p]) for p in self.patterns]
        except KeyError as e:
            raise L.TspmError(f"pattern {e} is not one of this log's groups {self.log.groups}") from None

    def load_batch(self, A: torch.Tensor, I: torch.Tensor, labels: torch.Tensor) -> None:
        for dst, src in ((self.A, A), (self.I, I), (self.labels, labels)):
            if src.data_ptr() != dst.data_ptr():
                dst.copy_(src.reshape(dst.shape), non_blocking=True)

    def _head_kernel(self, sh: int) -> None:
        net, log, g = self.model.net, self.log, (lambda t: t.data_ptr())
        d = L.PatternHeadEvalDesc(
            batch=self.N, npat=self.P, in_=self.F, w_audio=self.ea, hidden=self.hd, hidden2=self.h2, classes=NUM_CLASSES,
            ldx=self.F, x=g(self.fused), x0=g(self.x0), keep=self._keep, group_id=self._gid,
            w0=g(net[0].weight), b0=g(net[0].bias), w3=g(net[3].weight), b3=g(net[3].bias), w5=g(net[5].weight),
            b5=g(net[5].bias), labels=g(self.labels), loss_weight=self.ce_weight,
            n_groups=len(log.groups) if log is not None else 1, logits=g(self.logits), preds=g(self.preds),
            loss=g(self.loss), confusion=g(log.conf) if log is not None else None,
            loss_log=g(log.loss_log) if log is not None else None, counters=g(log.counters) if log is not None else None,
            log_capacity=log.capacity if log is not None else 0, workspace=g(self.ws), workspace_bytes=self.ws.numel())
        L.check(L.lib().tspm_pattern_head_eval(d, sh), "pattern_head_eval")

    def _head_launches(self, sh: int) -> None:
        lib, net, log = L.lib(), self.model.net, self.log
        n, F, hd, h2, B = self.P * self.N, self.F, self.hd, self.h2, self.N
        self.emb2[B:].copy_(self.x0.expand(B, F))
        wa, wv, wt = self._widths
        L.check(lib.tspm_pattern_expand(B, self.P, self._keep3, self._gid, wa, wv, wt, self.emb2.data_ptr(), F,
                                        self.x.data_ptr(), F, self.labels.data_ptr(), self.labels_x.data_ptr(), 8,
                                        self.groups.data_ptr(), sh), "pattern eval expand")
        L.check(lib.tspm_linear_fwd(n, F, hd, self.x.data_ptr(), F, net[0].weight.data_ptr(), net[0].bias.data_ptr(), 1,
                                    None, 1.0, self.h1.data_ptr(), hd, sh), "pattern eval fc0")
        L.check(lib.tspm_linear_fwd(n, hd, h2, self.h1.data_ptr(), hd, net[3].weight.data_ptr(), net[3].bias.data_ptr(),
                                    1, None, 1.0, self.hh.data_ptr(), h2, sh), "pattern eval fc3")
        L.check(lib.tspm_linear_fwd(n, h2, NUM_CLASSES, self.hh.data_ptr(), h2, net[5].weight.data_ptr(),
                                    net[5].bias.data_ptr(), 0, None, 1.0, self.logits.data_ptr(), NUM_CLASSES, sh),
                "pattern eval fc5")
        for p in range(self.P):
            lg, ls = self.logits[p * B:(p + 1) * B], self.loss[p:p + 1]
            L.check(lib.tspm_cross_entropy(B, NUM_CLASSES, lg.data_ptr(), self.labels.data_ptr(), ls.data_ptr(), None,
                                           self.ce_weight, None, sh), "pattern eval cross_entropy")
            L.check(lib.tspm_classify_update(
                B, NUM_CLASSES, lg.data_ptr(), self.labels.data_ptr(), self.groups[p * B:(p + 1) * B].data_ptr(),
                len(log.groups) if log is not None else 1, log.conf.data_ptr() if log is not None else None,
                self.preds[p * B:(p + 1) * B].data_ptr(), ls.data_ptr(),
                log.loss_log.data_ptr() if log is not None else None,
                log.counters.data_ptr() if log is not None else None, log.capacity if log is not None else 0, sh),
                "pattern eval classify_update")

    def _enqueue(self) -> None:
        self._bind_log()
        main = torch.cuda.current_stream()
        self.side.wait_stream(main)
        with torch.cuda.stream(self.side):
            self.eng_i.forward(self.I, self.fused[:, self.ea:], self.F, train=False)
        self.eng_a.forward(self.A, self.fused, self.F, train=False)
        main.wait_stream(self.side)
        if self.head == "kernel":
            self._head_kernel(main.cuda_stream)
        else:
            self._head_launches(main.cuda_stream)

    def _bind_log(self) -> None:
        """Group ids of the patterns in the current log, into the launch arguments (host values only), at the top of
        the enqueue that bakes them into the graph."""
        for p, g in enumerate(self._group_ids()):
            self._gid[p] = g

    def run(self, refresh_zero: bool = True) -> None:
        """Evaluate the batch in the static input buffers under every pattern (logits, loss, preds; log updated)."""
        self.model.eval()
        # the graph reads the zero-row buffer by address: a model that dropped its buffer (moved) hands out another
        self.x0 = self.model.zero_embeddings(refresh=refresh_zero, audio_hw=self.audio_hw, image_hw=self.image_hw)
        self.replay_or_enqueue(self._enqueue, (self.log, self.x0.data_ptr()))
        self.calls += 1

    def step(self, A, I, labels, refresh_zero: bool = True) -> Dict[str, torch.Tensor]:
        self.load_batch(A, I, labels)
        self.run(refresh_zero)
        return {"loss": self.loss, "logits": self.logits.view(self.P, self.N, NUM_CLASSES),
                "preds": self.preds.view(self.P, self.N)}


# ------------------------------------------------------------------------------------------------------
# The head stage: the fusion head trained on frozen, pre-trained encoders (AVMNIST.freeze_encoders)
# ------------------------------------------------------------------------------------------------------
ENCODER_NAMES = ("audio_encoder", "image_encoder")


def head_stage_frozen(model, optimizer=None, allreduce=None, all_patterns: bool = False) -> Tuple[str, ...]:
    """The model's frozen encoders as the fused steps may use them: ``()`` for an all-trainable model (the
    ``FusedTrainStep`` path, untouched) or both encoder names for the head stage.  Everything else is refused here,
    before anything is built, with a ``TspmError`` that names the module or parameter: mixed ``requires_grad`` flags
    inside an encoder; exactly one encoder frozen; encoders frozen by hand (``requires_grad_(False)`` without
    ``AVMNIST.freeze_encoders()``, which also pins them to eval mode — train-mode statistics of a frozen encoder are
    out of scope); a head parameter that is not trainable; and, for a frozen model, ``allreduce`` and a ``FusedAdam``
    whose flat buffers are not exactly the model's trainable parameters now.  ``all_patterns``: an all-pattern batch
    needs the frozen encoders and is refused without them."""
    frozen = {}
    for name in ENCODER_NAMES:
        enc = getattr(model, name)
        flags = [(n, p.requires_grad) for n, p in enc.named_parameters()]
        if flags and any(f != flags[0][1] for _, f in flags):
            odd = next(n for n, f in flags if f != flags[0][1])
            raise L.TspmError(f"{name}: mixed requires_grad flags inside an encoder ({name}.{flags[0][0]} is "
                              f"{flags[0][1]}, {name}.{odd} is {not flags[0][1]}); an encoder is frozen as a whole "
                              "(AVMNIST.freeze_encoders()) or not at all")
        frozen[name] = bool(flags) and not flags[0][1]
    pinned = tuple(getattr(model, "frozen_encoders", lambda: ())())
    if sum(frozen.values()) == 1:
        one = next(n for n in ENCODER_NAMES if frozen[n])
        other = next(n for n in ENCODER_NAMES if not frozen[n])
        raise L.TspmError(f"exactly one encoder is frozen ({one}; {other} is trainable): the head stage freezes both "
                          "encoders (AVMNIST.freeze_encoders()); one frozen and one trainable encoder is not supported")
    for name in ENCODER_NAMES:
        enc = getattr(model, name)
        if frozen[name] and (name not in pinned or enc.training):
            raise L.TspmError(f"{name}: its parameters have requires_grad=False but the encoder is not pinned to eval "
                              "mode; a frozen encoder on train-mode BatchNorm statistics is not supported - freeze with "
                              "AVMNIST.freeze_encoders(), which pins it to its running statistics")
        if name in pinned and not frozen[name]:
            raise L.TspmError(f"{name}: pinned by AVMNIST.freeze_encoders() but its parameters are trainable again; "
                              "call AVMNIST.unfreeze_encoders() to train it")
    for n, p in model.net.named_parameters():
        if not p.requires_grad:
            raise L.TspmError(f"net.{n}: a head parameter that is not trainable; the fused steps train the whole head")
    names = tuple(n for n in ENCODER_NAMES if frozen[n])
    if not names:
        if all_patterns:
            raise L.TspmError(
                "an all_patterns batch trains every missing-modality pattern of the batch in one step, which is exact "
                "only on frozen encoders (AVMNIST.freeze_encoders()): a trainable encoder runs BatchNorm on batch "
                "statistics, and the statistics of the B real rows are not those of the P*B replicated, masked rows "
                "(DESIGN 3.19), so one encoder pass cannot stand for the replicated batch")
        return ()
    if allreduce is not None:
        raise L.TspmError("allreduce: data parallelism for the head stage (frozen encoders) is not supported")
    if isinstance(optimizer, FusedAdam):
        fgs = optimizer.flat_groups()
        if len(fgs) != 1:
            raise L.TspmError(f"the head stage updates one FusedAdam group; the optimizer has {len(fgs)} non-empty groups")
        have = {id(p): p for p in fgs[0].params}
        for n, p in model.named_parameters():
            if p.requires_grad != (id(p) in have):
                what = "is trainable but not in" if p.requires_grad else "is frozen but still in"
                raise L.TspmError(f"{n} {what} the FusedAdam's flat buffers: they must hold exactly the model's "
                                  "trainable parameters (optimizer built before freeze_encoders(), or the flags changed "
                                  "since) - build a new FusedAdam(model.parameters())")
        if len(have) != sum(1 for p in model.parameters() if p.requires_grad):
            raise L.TspmError("the FusedAdam holds parameters that are not the model's: build it from "
                              "model.parameters() after freeze_encoders()")
    return names


def train_step_key(model, n: int, patterns=None, cached: bool = False):
    """The cache key of a model's fused train step for batch size ``n``: ``n`` itself for an all-trainable model (every
    existing key unchanged); with frozen encoders a tuple that ends in ``("frozen", names)``; an all-pattern step's
    starts with ``("patterns", names)``.  ``cached``: the step of a ``"cached"`` batch (``FusedCachedHeadStep``) — the
    same tuple with a trailing ``("cached",)`` element, which no other key has."""
    names = tuple(getattr(model, "frozen_encoders", lambda: ())())
    if not names and patterns is None and not cached:
        return n
    key = ((("patterns", tuple(patterns)),) if patterns is not None else ()) + (n,)
    return key + ((("frozen", names),) if names else ()) + ((("cached",),) if cached else ())


class _HeadStageBase(L.GraphRunner):
    """What the two head-stage steps share: the checks, the static inputs, both encoders' eval-mode forward on two
    streams (``FusedEvalStep``'s), the head's flat gradient views, ``tspm_classify_update`` and Adam over the head's
    one flat group (the head launch advances the step counter, so the update is one more launch)."""

    def _setup(self, model, optimizer, loss_functions, batch: int, audio_hw, image_hw, use_graph: bool, what: str):
        self._setup_head(model, optimizer, loss_functions, batch, audio_hw, image_hw, use_graph, what)
        dev, B = self.device, self.N
        f32 = dict(device=dev, dtype=torch.float32)
        self.A = torch.zeros(B, audio_hw[0], audio_hw[1], **f32)
        self.I = torch.zeros(B, 1, image_hw[0], image_hw[1], **f32)
        self.eng_a = model.audio_encoder.engine_for(self.A)
        self.eng_i = model.image_encoder.engine_for(self.I)

    def _setup_head(self, model, optimizer, loss_functions, batch: int, audio_hw, image_hw, use_graph: bool, what: str):
        """Everything of ``_setup`` but the encoders' inputs and engines (``FusedCachedHeadStep`` has neither)."""
        self.model, self.opt, self.loss_functions, self.N = model, optimizer, loss_functions, int(batch)
        self.ce_weight = _ce_weight(loss_functions)
        if self.ce_weight is None:
            raise L.TspmError(f"{what}: the loss group must be a single cross-entropy term")
        if not isinstance(optimizer, FusedAdam):
            raise L.TspmError(f"{what}: the optimizer must be this package's FusedAdam")
        if self.N < 1:
            raise L.TspmError(f"{what}: batch must be >= 1")
        self.frozen = head_stage_frozen(model, optimizer)
        if not self.frozen:
            raise L.TspmError(f"{what}: the model's encoders are not frozen (AVMNIST.freeze_encoders()); an all-trainable "
                              "model trains with FusedTrainStep")
        if not head_supported(model):
            raise L.TspmError(f"{what}: the fusion head's shape is outside tspm_head_train_step's limits")
        dev = next(model.parameters()).device
        self._init_graph(use_graph, dev)
        self.audio_hw, self.image_hw = tuple(audio_hw), tuple(image_hw)
        f32 = dict(device=dev, dtype=torch.float32)
        B = self.N
        self.ea = int(model.embd_size_A)
        self.F = self.ea + int(model.embd_size_I)
        self.hd, self.h2 = int(model.hidden_dim), int(model.hidden_dim) // 2
        self.labels = torch.zeros(B, dtype=torch.int64, device=dev)
        self.loss = torch.zeros(1, **f32)
        self.stats = torch.zeros(4, **f32)  # loss*n, correct, n (accumulated on device)
        self.log = None
        self.keep_override: Optional[torch.Tensor] = None
        self.side = L.shared_streams(dev, 1)[0]
        fg = optimizer.flat_groups()[0]
        self.fg = fg
        # the head's gradients go straight into FusedAdam's flat gradient buffer (its own views, whatever p.grad holds)
        gv = {id(p): g for p, g in zip(fg.params, fg.grad_views)}
        net = model.net
        self.gptr = [gv[id(p)].data_ptr() for p in (net[0].weight, net[0].bias, net[3].weight, net[3].bias,
                                                    net[5].weight, net[5].bias)]
        # dropout RNG counter = FusedAdam's device step counter (group 0's hyper.step)
        self._rng_ctr_ptr = fg.hyper.data_ptr() + L.HYPER_STEP_OFFSET
        self._sig = (id(optimizer), id(loss_functions), self.N, ("frozen", self.frozen))

    def _encoders(self, fused: torch.Tensor) -> int:
        """Both encoders' eval-mode forward into ``fused [B, F]``; returns the main stream's handle."""
        main = torch.cuda.current_stream()
        self.side.wait_stream(main)
        with torch.cuda.stream(self.side):
            self.eng_i.forward(self.I, fused[:, self.ea:], self.F, train=False)
        self.eng_a.forward(self.A, fused, self.F, train=False)
        main.wait_stream(self.side)
        return main.cuda_stream

    def _head_bumps(self) -> bool:
        """The head's second launch advances Adam's step counter (no clip coefficient: the range update has none)."""
        return getattr(self.opt, "clip_coef", None) is None

    def _adam(self, sh: int) -> None:
        if self._head_bumps():
            self.opt.launch_ranges(sh, [[(0, self.fg.numel)]])
        else:
            self.opt.launch(sh)

    def _classify_rows(self, sh: int, n: int, logits, labels, groups) -> None:
        log = self.log
        if log is None:
            return
        L.check(L.lib().tspm_classify_update(
            n, NUM_CLASSES, logits.data_ptr(), labels.data_ptr(), groups.data_ptr(), len(log.groups),
            log.conf.data_ptr(), None, self.loss.data_ptr(), log.loss_log.data_ptr(), log.counters.data_ptr(),
            log.capacity, sh), "classify_update")

    def _load(self, A, I, labels) -> None:
        for dst, src in ((self.A, A), (self.I, I), (self.labels, labels)):
            if src.data_ptr() != dst.data_ptr():
                dst.copy_(src.reshape(dst.shape), non_blocking=True)

    def _still_frozen(self) -> None:
        if tuple(self.model.frozen_encoders()) != self.frozen:
            raise L.TspmError("the model's frozen encoders changed since this step was built: build a new step (and a new "
                              "FusedAdam)")


class FusedHeadStageStep(_HeadStageBase):
    """AVMNIST.train_step on FROZEN encoders as one HIP graph: both encoders' eval-mode forward (running statistics,
    two streams), ``tspm_head_train_step`` over the B rows (its dx goes to a scratch buffer nobody reads),
    ``tspm_classify_update`` when a log is set, Adam over the head's one flat group.  The batch is what the train
    loader yields: one random pattern per sample, masks applied to the inputs.  No encoder backward, no BatchNorm
    statistics update: every encoder parameter and buffer is bitwise unchanged by any number of steps.  Any B >= 1."""

    def __init__(self, model, optimizer: FusedAdam, loss_functions, batch: int, audio_hw=(32, 94), image_hw=(28, 28),
                 use_graph: bool = True, allreduce=None):
        if allreduce is not None:
            head_stage_frozen(model, optimizer, allreduce)  # refuses it for a frozen model, naming why
        self._setup(model, optimizer, loss_functions, batch, audio_hw, image_hw, use_graph, "FusedHeadStageStep")
        dev, B = self.device, self.N
        f32 = dict(device=dev, dtype=torch.float32)
        self.groups = torch.zeros(B, dtype=torch.int32, device=dev)
        self.fused = torch.empty(B, self.F, **f32)
        self.h1 = torch.empty(B, self.hd, **f32)
        self.hh = torch.empty(B, self.h2, **f32)
        self.logits = torch.empty(B, NUM_CLASSES, **f32)
        self.dlogits = torch.empty(B, NUM_CLASSES, **f32)
        self.dh = torch.empty(B, self.h2, **f32)
        self.dh1 = torch.empty(B, self.hd, **f32)
        self.dscratch = torch.empty(B, self.F, **f32)  # the head's dx: written, never read
        self.row_ws = torch.empty(2 * B, **f32)
        self.keep = torch.ones(B, self.hd, dtype=torch.uint8, device=dev)
        self.head_rows_per_block = int(os.environ.get("TSPM_HEAD_RB", "0"))

    def matches(self, A, I, optimizer, loss_functions) -> bool:
        return (self._sig == (id(optimizer), id(loss_functions), A.shape[0], ("frozen", tuple(self.model.frozen_encoders())))
                and tuple(A.shape[1:]) == tuple(self.A.shape[1:]) and tuple(I.shape[-2:]) == tuple(self.I.shape[-2:]))

    def _enqueue(self) -> None:
        sh = self._encoders(self.fused)
        net, g = self.model.net, (lambda t: t.data_ptr())
        p = float(self.model.dropout_p)
        gp = self.gptr
        d = L.HeadDesc(n=self.N, in_=self.F, hidden=self.hd, hidden2=self.h2, classes=NUM_CLASSES, ldx=self.F,
                       lddx=self.F, gen_keep=1 if (p > 0 and self.keep_override is None) else 0,
                       x=g(self.fused), w0=g(net[0].weight), b0=g(net[0].bias), w3=g(net[3].weight), b3=g(net[3].bias),
                       w5=g(net[5].weight), b5=g(net[5].bias), p=p, loss_weight=self.ce_weight,
                       seed=int(self.model._rng_seed) if p > 0 else 0, counter=self._rng_ctr_ptr if p > 0 else None,
                       keep=g(self.keep), labels=g(self.labels), h1=g(self.h1), hh=g(self.hh), logits=g(self.logits),
                       dlogits=g(self.dlogits), dz3=g(self.dh), dz0=g(self.dh1), dx=g(self.dscratch),
                       row_ws=g(self.row_ws), gw0=gp[0], gb0=gp[1], gw3=gp[2], gb3=gp[3], gw5=gp[4], gb5=gp[5],
                       loss=g(self.loss), stats=g(self.stats),
                       adam_step=self._rng_ctr_ptr if self._head_bumps() else None,
                       rows_per_block=self.head_rows_per_block)
        L.check(L.lib().tspm_head_train_step(d, sh), "head_train_step")
        self._classify_rows(sh, self.N, self.logits, self.labels, self.groups)
        self._adam(sh)

    def load_batch(self, A, I, labels, groups=None) -> None:
        if groups is not None and groups.data_ptr() != self.groups.data_ptr():
            self.groups.copy_(groups.reshape(-1).to(torch.int32), non_blocking=True)
        self._load(A, I, labels)

    def run(self) -> None:
        """One head-stage step on the batch in the static input buffers."""
        self._still_frozen()
        self.model.train()  # the head's dropout on; the frozen encoders stay pinned to eval
        self.opt.sync_hyper()
        if self.keep_override is not None:
            self.keep.copy_(self.keep_override.reshape(self.keep.shape).to(torch.uint8), non_blocking=True)
        self.replay_or_enqueue(self._enqueue, (self.log, self.keep_override is None, self._head_bumps()))
        self.opt.note_steps(1)
        self.calls += 1

    def step(self, A, I, labels, groups=None) -> Dict[str, torch.Tensor]:
        self.load_batch(A, I, labels, groups)
        self.run()
        return {"loss": self.loss, "logits": self.logits}


# the head of a FusedHeadStagePatternStep built without head=: "kernel" (tspm_pattern_head_train_step) or "launches"
# (tspm_pattern_expand + tspm_head_train_step over the P*B rows); the leg whose median measured lower at batch 128
# (profiles/avmnist_head_stage.json)
DEFAULT_HEAD_STAGE_HEAD = "kernel"


class FusedHeadStagePatternStep(_HeadStageBase):
    """The head stage on EVERY missing-modality pattern of a batch in one step, as one HIP graph.  A frozen encoder on
    its running statistics is a per-row function and its weights do not move, so the embedding of a zeroed modality is
    one constant row (``AVMNIST.zero_embeddings``) for the whole training: the graph holds both encoders' eval forward
    over the B real, unmasked rows, then the head's forward, cross-entropy, backward over the P*B (pattern, sample)
    rows — ``head="kernel"``: one ``tspm_pattern_head_train_step`` call (fc0 as two half products per sample, its
    weight gradient over B + workgroups rows); ``head="launches"``: ``tspm_pattern_expand`` to ``[P*B, F]`` and
    ``tspm_head_train_step`` with ``n = P*B`` (the A/B leg, and the fallback for a head outside the kernel's limits) —
    then ``tspm_classify_update`` with every row under its pattern's group (ONE loss-log entry per step: the P*B-row
    mean) and Adam.  ``loss`` is ``weight * mean CE`` over all P*B rows.

    ``step(A, I, labels, refresh_zero=False)`` → ``{"loss": [1], "logits": [P, B, C]}``.  The zero embeddings are
    computed when the step is built and again on ``refresh_zero=True`` (``EpochRunner.train_epoch`` asks once per
    epoch; the weights that produce them are frozen)."""

    def __init__(self, model, optimizer: FusedAdam, loss_functions, batch: int, patterns=None, head: Optional[str] = None,
                 log=None, audio_hw=(32, 94), image_hw=(28, 28), use_graph: bool = True):
        self.patterns = norm_avmnist_patterns(patterns)
        self.P = P = len(self.patterns)
        head_stage_frozen(model, optimizer, all_patterns=True)  # an unfrozen model: refused with the BatchNorm argument
        self._setup(model, optimizer, loss_functions, batch, audio_hw, image_hw, use_graph, "FusedHeadStagePatternStep")
        self.log = log
        head = DEFAULT_HEAD_STAGE_HEAD if head is None else head
        if head not in ("kernel", "launches"):
            raise ValueError(f"head: 'kernel' or 'launches', got {head!r}")
        if head == "kernel" and not L.pattern_head_train_supported(self.F, self.ea, self.hd, self.h2, NUM_CLASSES, P):
            head = "launches"
        dev, B = self.device, self.N
        n = P * B
        self.head = head
        f32 = dict(device=dev, dtype=torch.float32)
        self.x0 = model.zero_embeddings(refresh=True, audio_hw=self.audio_hw, image_hw=self.image_hw)
        self.logits = torch.empty(n, NUM_CLASSES, **f32)
        self.keep = torch.ones(n, self.hd, dtype=torch.uint8, device=dev)
        self.labels_x = torch.zeros(n, dtype=torch.int64, device=dev)
        self.groups = torch.zeros(n, dtype=torch.int32, device=dev)
        self._keep2 = (ctypes.c_int32 * (2 * P))(*[k for p in self.patterns for k in PATTERN_KEEP[p]])
        self._gid = (ctypes.c_int32 * P)()
        if head == "kernel":
            self.fused = torch.empty(B, self.F, **f32)
            need = int(L.lib().tspm_pattern_head_train_workspace(B, P))
            self.ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        else:
            # tspm_pattern_expand's layout (FusedPatternEvalStep's launches leg): rows [0, B) the real embeddings,
            # rows [B, 2B) the zero-input row broadcast; the image columns go in as two halves under one keep flag
            ei = self.F - self.ea
            self.emb2 = torch.empty(2 * B, self.F, **f32)
            self.fused = self.emb2[:B]
            self._widths = (self.ea, ei // 2, ei - ei // 2)
            self.x = torch.empty(n, self.F, **f32)
            self.h1 = torch.empty(n, self.hd, **f32)
            self.hh = torch.empty(n, self.h2, **f32)
            self.dlogits = torch.empty(n, NUM_CLASSES, **f32)
            self.dh = torch.empty(n, self.h2, **f32)
            self.dh1 = torch.empty(n, self.hd, **f32)
            self.dscratch = torch.empty(n, self.F, **f32)
            self.row_ws = torch.empty(2 * n, **f32)
            self._keep3 = (ctypes.c_int32 * (3 * P))(*[k for p in self.patterns
                                                        for k in (PATTERN_KEEP[p][0],) + (PATTERN_KEEP[p][1],) * 2])
        self._bound_groups = None  # the group ids last written to ``groups`` (kernel leg)
        self._sig = self._sig + (self.patterns,)

    def matches(self, A, I, optimizer, loss_functions, patterns) -> bool:
        return (self._sig == (id(optimizer), id(loss_functions), A.shape[0],
                              ("frozen", tuple(self.model.frozen_encoders())), tuple(patterns))
                and tuple(A.shape[1:]) == tuple(self.A.shape[1:]) and tuple(I.shape[-2:]) == tuple(self.I.shape[-2:]))

    def _group_ids(self) -> List[int]:
        gid = self.log.gid if self.log is not None else {p: i for i, p in enumerate(AVMNIST_PATTERNS)}
        try:
            return [int(gid[p]) for p in self.patterns]
        except KeyError as e:
            raise L.TspmError(f"pattern {e} is not one of this log's groups {self.log.groups}") from None

    def _enqueue(self) -> None:
        for p, g in enumerate(self._group_ids()):
            self._gid[p] = g
        sh = self._encoders(self.fused)
        self._head(sh)
        self._classify_rows(sh, self.P * self.N, self.logits, self.labels_x, self.groups)
        self._adam(sh)

    def _head(self, sh: int, head: Optional[str] = None) -> None:
        """The head leg alone (forward, loss, weight backward over the P*B rows) from ``fused`` and ``x0``, either way
        (``head``: the leg, by default this step's own)."""
        head = self.head if head is None else head
        net, g = self.model.net, (lambda t: t.data_ptr())
        p = float(self.model.dropout_p)
        gp = self.gptr
        gen_keep = 1 if (p > 0 and self.keep_override is None) else 0
        seed = int(self.model._rng_seed) if p > 0 else 0
        ctr = self._rng_ctr_ptr if p > 0 else None
        bump = self._rng_ctr_ptr if self._head_bumps() else None
        n, B, F = self.P * self.N, self.N, self.F
        if head == "kernel":
            d = L.PatternHeadTrainDesc(
                batch=B, npat=self.P, in_=F, w_audio=self.ea, hidden=self.hd, hidden2=self.h2, classes=NUM_CLASSES,
                ldx=F, gen_keep=gen_keep, x=g(self.fused), x0=g(self.x0), keep=self._keep2, w0=g(net[0].weight),
                b0=g(net[0].bias), w3=g(net[3].weight), b3=g(net[3].bias), w5=g(net[5].weight), b5=g(net[5].bias),
                labels=g(self.labels), p=p, loss_weight=self.ce_weight, seed=seed, counter=ctr, keep_mask=g(self.keep),
                logits=g(self.logits), gw0=gp[0], gb0=gp[1], gw3=gp[2], gb3=gp[3], gw5=gp[4], gb5=gp[5],
                loss=g(self.loss), stats=g(self.stats), adam_step=bump, workspace=g(self.ws),
                workspace_bytes=self.ws.numel())
            L.check(L.lib().tspm_pattern_head_train_step(d, sh), "pattern_head_train_step")
        else:
            # the P*B rows, their labels and their group ids in one launch
            self.emb2[B:].copy_(self.x0.expand(B, F))
            wa, wv, wt = self._widths
            L.check(L.lib().tspm_pattern_expand(B, self.P, self._keep3, self._gid, wa, wv, wt, self.emb2.data_ptr(), F,
                                                self.x.data_ptr(), F, self.labels.data_ptr(), self.labels_x.data_ptr(),
                                                8, self.groups.data_ptr(), sh), "head stage pattern expand")
            d = L.HeadDesc(n=n, in_=F, hidden=self.hd, hidden2=self.h2, classes=NUM_CLASSES, ldx=F, lddx=F,
                           gen_keep=gen_keep, x=g(self.x), w0=g(net[0].weight), b0=g(net[0].bias), w3=g(net[3].weight),
                           b3=g(net[3].bias), w5=g(net[5].weight), b5=g(net[5].bias), p=p, loss_weight=self.ce_weight,
                           seed=seed, counter=ctr, keep=g(self.keep), labels=g(self.labels_x), h1=g(self.h1),
                           hh=g(self.hh), logits=g(self.logits), dlogits=g(self.dlogits), dz3=g(self.dh),
                           dz0=g(self.dh1), dx=g(self.dscratch), row_ws=g(self.row_ws), gw0=gp[0], gb0=gp[1],
                           gw3=gp[2], gb3=gp[3], gw5=gp[4], gb5=gp[5], loss=g(self.loss), stats=g(self.stats),
                           adam_step=bump, rows_per_block=0)
            L.check(L.lib().tspm_head_train_step(d, sh), "head_train_step (P*B rows)")

    def load_batch(self, A, I, labels) -> None:
        """The batch into the static inputs.  The kernel leg never forms the P*B rows, so the per-row labels that
        ``tspm_classify_update`` reads are laid out here, with the other input copies, outside the graph (the launches
        leg's expand writes them)."""
        self._load(A, I, labels)
        if self.head == "kernel" and self.log is not None:
            self.labels_x.view(self.P, self.N).copy_(self.labels.unsqueeze(0).expand(self.P, self.N), non_blocking=True)

    def _bind_groups(self) -> None:
        """Kernel leg: every row's group id for the current log (constant while the log is), written outside the graph."""
        if self.head != "kernel" or self.log is None:
            return
        gids = tuple(self._group_ids())
        if self._bound_groups != gids:
            self.groups.copy_(torch.tensor(gids, dtype=torch.int32).repeat_interleave(self.N), non_blocking=False)
            self._bound_groups = gids

    def run(self, refresh_zero: bool = False) -> None:
        """One head-stage step on the batch in the static input buffers, under every pattern."""
        self._still_frozen()
        self.model.train()
        self.opt.sync_hyper()
        if self.keep_override is not None:
            self.keep.copy_(self.keep_override.reshape(self.keep.shape).to(torch.uint8), non_blocking=True)
        # the graph reads the zero-row buffer by address: a model that dropped its buffer (moved) hands out another
        self.x0 = self.model.zero_embeddings(refresh=refresh_zero, audio_hw=self.audio_hw, image_hw=self.image_hw)
        self._bind_groups()
        self.replay_or_enqueue(self._enqueue, (self.log, self.keep_override is None, self._head_bumps(),
                                               self.x0.data_ptr()))
        self.opt.note_steps(1)
        self.calls += 1

    def step(self, A, I, labels, refresh_zero: bool = False) -> Dict[str, torch.Tensor]:
        self.load_batch(A, I, labels)
        self.run(refresh_zero)
        return {"loss": self.loss, "logits": self.logits.view(self.P, self.N, NUM_CLASSES)}


# ------------------------------------------------------------------------------------------------------
# The head stage on cached embeddings (modules.EmbeddingCache): no encoder launch in a step
# ------------------------------------------------------------------------------------------------------
# the head of a FusedCachedHeadStep built without head=: "kernel" (one tspm_cached_head_train_step call, the log folded
# in) or "launches" (tspm_embed_gather + the uncached head launch + tspm_classify_update); the leg whose median
# measured lower at batch 128, for every pattern (39.4 against 43.8 us) and per sample (37.6 against 39.2 us):
# profiles/avmnist_embedding_cache.json, DESIGN §3.23
DEFAULT_CACHED_HEAD = "kernel"


class FusedCachedHeadStep(_HeadStageBase):
    """The head stage on an ``EmbeddingCache``: the head's forward, cross-entropy, weight backward and Adam over the
    cache rows a batch names by sample index, as one HIP graph without an encoder launch.  Two modes.  Every pattern of
    the batch (``patterns``: names, default all three; ``FusedHeadStagePatternStep``'s semantics, ``logits [P, B, C]``)
    or one pattern per sample (``per_sample=True``: what the default train loader draws — ``FusedHeadStageStep``'s
    semantics with the sample's dropped modality taken from ``cache.x0``, ``logits [B, C]``).

    ``head="kernel"``: one ``tspm_cached_head_train_step`` call, which reads the rows and labels from the cache and
    writes the classification log itself.  ``head="launches"``: ``tspm_embed_gather`` into the static ``fused``, then
    the uncached launch — ``FusedHeadStagePatternStep._head`` (every pattern) or ``tspm_head_train_step`` (per sample)
    — then ``tspm_classify_update``: the A/B leg, bitwise those steps fed ``cache.emb[ids]``, and the fallback for a
    head outside the fused kernel's limits.  Then Adam over the head's one group (the head launch advances the step
    counter).  The dropout seed and counter are the existing steps'.

    ``step(sample_ids, keep=None, groups=None)`` → ``{"loss": [1], "logits"}``: ``sample_ids [B]`` int64, and per
    sample ``keep [B, 2]`` (audio, image; non-zero = the real input) and ``groups [B]`` (the rows' groups in the log).
    Refused: what ``_HeadStageBase`` refuses, a stale cache and a cache built for another model.

    ``steps=K > 1`` (at most ``_lib.CACHED_HEAD_MAX_STEPS``): one call runs K consecutive steps on K batches — the
    static inputs are ``rows [K*B]``, ``row_keep [K*B, 2]`` and ``groups [K*B]``, ``step`` takes ``sample_ids [K*B]``
    (batch k is rows ``[k*B, (k+1)*B)``), and the graph is one ``tspm_cached_head_train_steps`` call: two launches per
    step, Adam applied in the second, no separate Adam launch.  Parameters, moments, log and step counter are bitwise
    those of K ``steps=1`` steps; ``loss`` and ``logits`` are the last step's.  Refused with ``steps > 1``, by name:
    ``head="launches"``, a head outside ``cached_head_train_supported``, a ``keep_override`` and an optimizer with a
    clip coefficient (the fused update has none).  ``steps=1`` is the step described above, launch for launch."""

    def __init__(self, model, optimizer: FusedAdam, loss_functions, batch: int, cache, patterns=None,
                 per_sample: bool = False, head: Optional[str] = None, log=None, use_graph: bool = True,
                 allreduce=None, steps: int = 1):
        self.steps = K = int(steps)
        if not 1 <= K <= L.CACHED_HEAD_MAX_STEPS:
            raise L.TspmError(f"FusedCachedHeadStep: steps must be 1 .. {L.CACHED_HEAD_MAX_STEPS}, got {steps}")
        if allreduce is not None:
            head_stage_frozen(model, optimizer, allreduce)  # refuses it for a frozen model, naming why
        self.per_sample = bool(per_sample)
        if self.per_sample and patterns is not None:
            raise ValueError("per_sample=True draws one pattern per sample from the keep flags; it excludes patterns=")
        self.patterns = () if self.per_sample else norm_avmnist_patterns(patterns)
        self.P = P = 1 if self.per_sample else len(self.patterns)
        cache.check(model)
        self.cache = cache
        self._setup_head(model, optimizer, loss_functions, batch, cache.audio_hw, cache.image_hw, use_graph,
                         "FusedCachedHeadStep")
        self.log = log
        head = DEFAULT_CACHED_HEAD if head is None else head
        if head not in ("kernel", "launches"):
            raise ValueError(f"head: 'kernel' or 'launches', got {head!r}")
        fits = L.cached_head_train_supported(self.F, self.ea, self.hd, self.h2, NUM_CLASSES, P)
        if K > 1:
            if head == "launches":
                raise L.TspmError('FusedCachedHeadStep: steps > 1 runs tspm_cached_head_train_steps; head="launches" '
                                  "has no multi-step form")
            if not fits:
                raise L.TspmError("FusedCachedHeadStep: steps > 1 needs a fusion head inside "
                                  "cached_head_train_supported's limits; this head runs one step per call")
            self._refuse_clip()
        if head == "kernel" and not fits:
            head = "launches"
        self.head = head
        dev, B = self.device, self.N
        n = P * B
        f32 = dict(device=dev, dtype=torch.float32)
        self.x0 = cache.x0
        self.rows = torch.zeros(K * B, dtype=torch.int64, device=dev)
        self.row_keep = torch.ones(K * B, 2, dtype=torch.uint8, device=dev)
        self.groups = torch.zeros(K * B, dtype=torch.int32, device=dev)
        self.logits = torch.empty(n, NUM_CLASSES, **f32)
        self.keep = torch.ones(n, self.hd, dtype=torch.uint8, device=dev)
        self._keep2 = (ctypes.c_int32 * (2 * max(P, 1)))(*[k for p in self.patterns for k in PATTERN_KEEP[p]])
        self._gid = (ctypes.c_int32 * max(P, 1))()
        if head == "kernel":
            need = int(L.lib().tspm_cached_head_train_workspace(B, P))
            self.ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        elif self.per_sample:
            # FusedHeadStageStep's buffers
            self.fused = torch.empty(B, self.F, **f32)
            self.h1 = torch.empty(B, self.hd, **f32)
            self.hh = torch.empty(B, self.h2, **f32)
            self.dlogits = torch.empty(B, NUM_CLASSES, **f32)
            self.dh = torch.empty(B, self.h2, **f32)
            self.dh1 = torch.empty(B, self.hd, **f32)
            self.dscratch = torch.empty(B, self.F, **f32)
            self.row_ws = torch.empty(2 * B, **f32)
        else:
            # FusedHeadStagePatternStep's buffers, for the leg of its _head that fits this head
            self._inner = "kernel" if L.pattern_head_train_supported(self.F, self.ea, self.hd, self.h2, NUM_CLASSES,
                                                                     P) else "launches"
            self.labels_x = torch.zeros(n, dtype=torch.int64, device=dev)
            self.groups_x = torch.zeros(n, dtype=torch.int32, device=dev)
            if self._inner == "kernel":
                self.fused = torch.empty(B, self.F, **f32)
                need = int(L.lib().tspm_pattern_head_train_workspace(B, P))
                self.ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            else:
                ei = self.F - self.ea
                self.emb2 = torch.empty(2 * B, self.F, **f32)
                self.fused = self.emb2[:B]
                self._widths = (self.ea, ei // 2, ei - ei // 2)
                self.x = torch.empty(n, self.F, **f32)
                self.h1 = torch.empty(n, self.hd, **f32)
                self.hh = torch.empty(n, self.h2, **f32)
                self.dlogits = torch.empty(n, NUM_CLASSES, **f32)
                self.dh = torch.empty(n, self.h2, **f32)
                self.dh1 = torch.empty(n, self.hd, **f32)
                self.dscratch = torch.empty(n, self.F, **f32)
                self.row_ws = torch.empty(2 * n, **f32)
                self._keep3 = (ctypes.c_int32 * (3 * P))(*[k for p in self.patterns
                                                            for k in (PATTERN_KEEP[p][0],) + (PATTERN_KEEP[p][1],) * 2])
        self._bound_groups = None
        self._sig = self._sig + (self.patterns, self.per_sample, id(cache)) + ((("steps", K),) if K > 1 else ())

    def _refuse_clip(self) -> None:
        if not self._head_bumps():
            raise L.TspmError("FusedCachedHeadStep: steps > 1 applies Adam inside the weight-gradient launch, which has "
                              "no clip coefficient; this optimizer has one set (clip_coef)")

    def _group_ids(self) -> List[int]:
        gid = self.log.gid if self.log is not None else {p: i for i, p in enumerate(AVMNIST_PATTERNS)}
        try:
            return [int(gid[p]) for p in self.patterns]
        except KeyError as e:
            raise L.TspmError(f"pattern {e} is not one of this log's groups {self.log.groups}") from None

    def _dropout(self):
        p = float(self.model.dropout_p)
        return (p, 1 if (p > 0 and self.keep_override is None) else 0, int(self.model._rng_seed) if p > 0 else 0,
                self._rng_ctr_ptr if p > 0 else None, self._rng_ctr_ptr if self._head_bumps() else None)

    def _gather(self, sh: int, flags: bool) -> None:
        c = self.cache
        L.check(L.lib().tspm_embed_gather(
            self.N, self.F, c.emb.data_ptr(), c.n, self.F, self.rows.data_ptr(), c.labels_all.data_ptr(),
            self.row_keep.data_ptr() if flags else None, self.ea, self.x0.data_ptr() if flags else None,
            self.fused.data_ptr(), self.F, self.labels.data_ptr(), sh), "embed_gather")

    def _enqueue(self) -> None:
        for i, gv in enumerate(self._group_ids()):
            self._gid[i] = gv
        sh = torch.cuda.current_stream().cuda_stream
        net, g, c, log = self.model.net, (lambda t: t.data_ptr()), self.cache, self.log
        p, gen_keep, seed, ctr, bump = self._dropout()
        gp = self.gptr
        if self.head == "kernel":
            d = L.CachedHeadTrainDesc(
                batch=self.N, npat=self.P, in_=self.F, w_audio=self.ea, hidden=self.hd, hidden2=self.h2,
                classes=NUM_CLASSES, ld_emb=self.F, gen_keep=gen_keep, n_groups=len(log.groups) if log is not None else 1,
                n_rows=c.n, emb=g(c.emb), x0=g(self.x0), rows=g(self.rows), labels_all=g(c.labels_all),
                keep=None if self.per_sample else self._keep2, group_id=None if self.per_sample else self._gid,
                row_keep=g(self.row_keep) if self.per_sample else None,
                row_group=g(self.groups) if self.per_sample else None,
                w0=g(net[0].weight), b0=g(net[0].bias), w3=g(net[3].weight), b3=g(net[3].bias), w5=g(net[5].weight),
                b5=g(net[5].bias), p=p, loss_weight=self.ce_weight, seed=seed, counter=ctr, keep_mask=g(self.keep),
                logits=g(self.logits), gw0=gp[0], gb0=gp[1], gw3=gp[2], gb3=gp[3], gw5=gp[4], gb5=gp[5],
                loss=g(self.loss), stats=g(self.stats), adam_step=bump,
                confusion=g(log.conf) if log is not None else None, loss_log=g(log.loss_log) if log is not None else None,
                counters=g(log.counters) if log is not None else None, log_capacity=log.capacity if log is not None else 0,
                workspace=g(self.ws), workspace_bytes=self.ws.numel())
            if self.steps > 1:
                fg = self.fg
                ad = L.HeadAdamDesc(param=g(fg.param), grad=g(fg.grad), exp_avg=g(fg.exp_avg),
                                    exp_avg_sq=g(fg.exp_avg_sq), count=fg.numel, hyper=g(fg.hyper))
                L.check(L.lib().tspm_cached_head_train_steps(d, ad, self.steps, sh), "cached_head_train_steps")
                return  # Adam ran in every step's second launch
            L.check(L.lib().tspm_cached_head_train_step(d, sh), "cached_head_train_step")
        elif self.per_sample:
            self._gather(sh, True)
            d = L.HeadDesc(n=self.N, in_=self.F, hidden=self.hd, hidden2=self.h2, classes=NUM_CLASSES, ldx=self.F,
                           lddx=self.F, gen_keep=gen_keep, x=g(self.fused), w0=g(net[0].weight), b0=g(net[0].bias),
                           w3=g(net[3].weight), b3=g(net[3].bias), w5=g(net[5].weight), b5=g(net[5].bias), p=p,
                           loss_weight=self.ce_weight, seed=seed, counter=ctr, keep=g(self.keep), labels=g(self.labels),
                           h1=g(self.h1), hh=g(self.hh), logits=g(self.logits), dlogits=g(self.dlogits), dz3=g(self.dh),
                           dz0=g(self.dh1), dx=g(self.dscratch), row_ws=g(self.row_ws), gw0=gp[0], gb0=gp[1], gw3=gp[2],
                           gb3=gp[3], gw5=gp[4], gb5=gp[5], loss=g(self.loss), stats=g(self.stats), adam_step=bump,
                           rows_per_block=0)
            L.check(L.lib().tspm_head_train_step(d, sh), "head_train_step")
            self._classify_rows(sh, self.N, self.logits, self.labels, self.groups)
        else:
            self._gather(sh, False)
            grp, self.groups = self.groups, self.groups_x  # _head's expand writes the P*B group ids (launches leg)
            try:
                FusedHeadStagePatternStep._head(self, sh, self._inner)
            finally:
                self.groups = grp
            if log is not None:
                if self._inner == "kernel":  # the rows' labels for tspm_classify_update (the expand writes them otherwise)
                    self.labels_x.view(self.P, self.N).copy_(self.labels.unsqueeze(0).expand(self.P, self.N))
                self._classify_rows(sh, self.P * self.N, self.logits, self.labels_x, self.groups_x)
        self._adam(sh)

    def load_batch(self, sample_ids: torch.Tensor, keep: Optional[torch.Tensor] = None,
                   groups: Optional[torch.Tensor] = None) -> None:
        if sample_ids.numel() != self.steps * self.N:
            raise L.TspmError(f"FusedCachedHeadStep: built for {self.steps * self.N} samples, got {sample_ids.numel()} "
                              "ids")
        if not self.per_sample and (keep is not None or groups is not None):
            raise L.TspmError("FusedCachedHeadStep: keep / groups are per-sample inputs; this step trains every pattern "
                              "of the batch")
        if sample_ids.data_ptr() != self.rows.data_ptr():
            self.rows.copy_(sample_ids.reshape(-1), non_blocking=True)
        if keep is not None and keep.data_ptr() != self.row_keep.data_ptr():
            self.row_keep.copy_(keep.reshape(self.steps * self.N, 2).to(torch.uint8), non_blocking=True)
        if groups is not None and groups.data_ptr() != self.groups.data_ptr():
            self.groups.copy_(groups.reshape(-1).to(torch.int32), non_blocking=True)

    def _bind_groups(self) -> None:
        """Every-pattern launches leg on the fused inner kernel: the P*B rows' group ids, written outside the graph."""
        if self.per_sample or self.head == "kernel" or self._inner != "kernel" or self.log is None:
            return
        gids = tuple(self._group_ids())
        if self._bound_groups != gids:
            self.groups_x.copy_(torch.tensor(gids, dtype=torch.int32).repeat_interleave(self.N), non_blocking=False)
            self._bound_groups = gids

    def run(self) -> None:
        """``steps`` head-stage steps on the cache rows named in the static ``rows`` (and ``row_keep`` / ``groups``)."""
        self._still_frozen()
        self.cache.check(self.model)
        self.model.train()
        if self.steps > 1:
            if self.keep_override is not None:
                raise L.TspmError("FusedCachedHeadStep: steps > 1 draws every step's dropout mask on the device; a "
                                  "keep_override holds one step's mask")
            self._refuse_clip()
        self.opt.sync_hyper()
        if self.keep_override is not None:
            self.keep.copy_(self.keep_override.reshape(self.keep.shape).to(torch.uint8), non_blocking=True)
        self.x0 = self.cache.x0
        self._bind_groups()
        self.replay_or_enqueue(self._enqueue, (self.log, self.keep_override is None, self._head_bumps(),
                                               self.x0.data_ptr(), self.cache.emb.data_ptr(),
                                               tuple(self._group_ids())) + ((("steps", self.steps),)
                                                                             if self.steps > 1 else ()))
        self.opt.note_steps(self.steps)
        self.calls += 1

    def step(self, sample_ids, keep=None, groups=None) -> Dict[str, torch.Tensor]:
        self.load_batch(sample_ids, keep, groups)
        self.run()
        return {"loss": self.loss, "logits": self.logits if self.per_sample else
                self.logits.view(self.P, self.N, NUM_CLASSES)}


class FusedCachedEvalStep(FusedPatternEvalStep):
    """AVMNIST.validation_step on an ``EmbeddingCache``: ``tspm_embed_gather`` into the static ``fused``, then the
    existing eval head, as one HIP graph without an encoder launch.  A fused-pattern batch (``patterns``: names, default
    all three) runs ``FusedPatternEvalStep``'s head (``tspm_pattern_head_eval``, or its launches for a head outside the
    kernel's limits): P loss entries per batch in pattern order and every row's count under its pattern, as that step
    writes them.  A per-pattern batch (``per_sample=True``: each row under its own ``keep`` flags, the dropped modality
    from ``cache.x0``) runs ``FusedEvalStep``'s head launches: one loss entry per batch, the rows under ``groups``.

    ``step(sample_ids, keep=None, groups=None)`` → ``{"loss", "logits", "preds"}``.

    ``steps=K > 1``: one call evaluates K consecutive batches — static ``rows [K*B]``, ``row_keep [K*B, 2]`` and
    ``groups [K*B]``, and the graph holds the launches above K times, the k-th gather reading ``rows[k*B:(k+1)*B]``:
    the log takes the same entries, in batch order, as K single steps; ``loss``, ``logits`` and ``preds`` are the last
    batch's."""

    def __init__(self, model, loss_functions, batch: int, cache, log=None, patterns=None, per_sample: bool = False,
                 head: Optional[str] = None, use_graph: bool = True, steps: int = 1):
        self.steps = K = int(steps)
        if not 1 <= K <= L.CACHED_HEAD_MAX_STEPS:
            raise L.TspmError(f"FusedCachedEvalStep: steps must be 1 .. {L.CACHED_HEAD_MAX_STEPS}, got {steps}")
        self.model, self.N, self.log = model, int(batch), log
        self.ce_weight = _ce_weight(loss_functions)
        if self.ce_weight is None:
            raise L.TspmError("FusedCachedEvalStep: the loss group must be a single cross-entropy term")
        self.per_sample = bool(per_sample)
        if self.per_sample and patterns is not None:
            raise ValueError("per_sample=True evaluates each row under its own keep flags; it excludes patterns=")
        self.patterns = () if self.per_sample else norm_avmnist_patterns(patterns)
        self.P = P = 1 if self.per_sample else len(self.patterns)
        cache.check(model)
        self.cache = cache
        ea, ei = int(model.embd_size_A), int(model.embd_size_I)
        self.ea, self.F, self.hd, self.h2 = ea, ea + ei, int(model.hidden_dim), int(model.hidden_dim) // 2
        head = DEFAULT_PATTERN_HEAD if head is None else head
        if head not in ("kernel", "launches"):
            raise ValueError(f"head: 'kernel' or 'launches', got {head!r}")
        if self.per_sample or not L.pattern_head_eval_supported(self.F, ea, self.hd, self.h2, NUM_CLASSES, P):
            head = "launches"
        self.head = head
        dev = next(model.parameters()).device
        self._init_graph(use_graph, dev)
        self.audio_hw, self.image_hw = cache.audio_hw, cache.image_hw
        f32 = dict(device=dev, dtype=torch.float32)
        B = self.N
        self.rows = torch.zeros(K * B, dtype=torch.int64, device=dev)
        self.row_keep = torch.ones(K * B, 2, dtype=torch.uint8, device=dev)
        self.labels = torch.zeros(B, dtype=torch.int64, device=dev)
        self.x0 = cache.x0
        if self.per_sample:  # FusedEvalStep's head buffers: one row per sample, the rows' groups
            self.logits = torch.empty(B, NUM_CLASSES, **f32)
            self.loss = torch.zeros(1, **f32)
            self.preds = torch.zeros(B, dtype=torch.int64, device=dev)
            self.groups = torch.zeros(K * B, dtype=torch.int32, device=dev)
            self.fused = torch.empty(B, self.F, **f32)
            self.h1 = torch.empty(B, self.hd, **f32)
            self.hh = torch.empty(B, self.h2, **f32)
        else:
            self._alloc_head(dev, B, head)

    def load_batch(self, sample_ids: torch.Tensor, keep: Optional[torch.Tensor] = None,
                   groups: Optional[torch.Tensor] = None) -> None:
        if sample_ids.numel() != self.steps * self.N:
            raise L.TspmError(f"FusedCachedEvalStep: built for {self.steps * self.N} samples, got {sample_ids.numel()} "
                              "ids")
        if not self.per_sample and (keep is not None or groups is not None):
            raise L.TspmError("FusedCachedEvalStep: keep / groups are per-sample inputs; this step evaluates every "
                              "pattern of the batch")
        if sample_ids.data_ptr() != self.rows.data_ptr():
            self.rows.copy_(sample_ids.reshape(-1), non_blocking=True)
        if keep is not None and keep.data_ptr() != self.row_keep.data_ptr():
            self.row_keep.copy_(keep.reshape(self.steps * self.N, 2).to(torch.uint8), non_blocking=True)
        if groups is not None and groups.data_ptr() != self.groups.data_ptr():
            self.groups.copy_(groups.reshape(-1).to(torch.int32), non_blocking=True)

    def _enqueue(self) -> None:
        for k in range(self.steps):
            self._enqueue_batch(k)

    def _enqueue_batch(self, k: int) -> None:
        """The step's launches on batch k of the static inputs (rows, flags and groups ``[k*B, (k+1)*B)``)."""
        lib, c, log = L.lib(), self.cache, self.log
        sh = torch.cuda.current_stream().cuda_stream
        flags = self.per_sample
        at = k * self.N
        L.check(lib.tspm_embed_gather(
            self.N, self.F, c.emb.data_ptr(), c.n, self.F, self.rows[at:].data_ptr(), c.labels_all.data_ptr(),
            self.row_keep[at:].data_ptr() if flags else None, self.ea, self.x0.data_ptr() if flags else None,
            self.fused.data_ptr(), self.F, self.labels.data_ptr(), sh), "embed_gather")
        if not self.per_sample:
            self._bind_log()
            if self.head == "kernel":
                self._head_kernel(sh)
            else:
                self._head_launches(sh)
            return
        # FusedEvalStep's head launches
        n, F, hd, h2, net = self.N, self.F, self.hd, self.h2, self.model.net
        L.check(lib.tspm_linear_fwd(n, F, hd, self.fused.data_ptr(), F, net[0].weight.data_ptr(),
                                    net[0].bias.data_ptr(), 1, None, 1.0, self.h1.data_ptr(), hd, sh), "eval fc0")
        L.check(lib.tspm_linear_fwd(n, hd, h2, self.h1.data_ptr(), hd, net[3].weight.data_ptr(),
                                    net[3].bias.data_ptr(), 1, None, 1.0, self.hh.data_ptr(), h2, sh), "eval fc3")
        L.check(lib.tspm_linear_fwd(n, h2, NUM_CLASSES, self.hh.data_ptr(), h2, net[5].weight.data_ptr(),
                                    net[5].bias.data_ptr(), 0, None, 1.0, self.logits.data_ptr(), NUM_CLASSES, sh),
                "eval fc5")
        L.check(lib.tspm_cross_entropy(n, NUM_CLASSES, self.logits.data_ptr(), self.labels.data_ptr(),
                                       self.loss.data_ptr(), None, self.ce_weight, None, sh), "eval cross_entropy")
        L.check(lib.tspm_classify_update(
            n, NUM_CLASSES, self.logits.data_ptr(), self.labels.data_ptr(), self.groups[at:].data_ptr(),
            len(log.groups) if log is not None else 1, log.conf.data_ptr() if log is not None else None,
            self.preds.data_ptr(), self.loss.data_ptr(), log.loss_log.data_ptr() if log is not None else None,
            log.counters.data_ptr() if log is not None else None, log.capacity if log is not None else 0, sh),
            "eval classify_update")

    def run(self) -> None:
        self.cache.check(self.model)
        self.model.eval()
        self.x0 = self.cache.x0
        self.replay_or_enqueue(self._enqueue, (self.log, self.x0.data_ptr(), self.cache.emb.data_ptr()) +
                               ((("steps", self.steps),) if self.steps > 1 else ()))
        self.calls += 1

    def step(self, sample_ids, keep=None, groups=None) -> Dict[str, torch.Tensor]:
        self.load_batch(sample_ids, keep, groups)
        self.run()
        if self.per_sample:
            return {"loss": self.loss, "logits": self.logits, "preds": self.preds}
        return {"loss": self.loss, "logits": self.logits.view(self.P, self.N, NUM_CLASSES),
                "preds": self.preds.view(self.P, self.N)}
