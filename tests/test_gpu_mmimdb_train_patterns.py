"""Training every missing-modality pattern of an MMIMDb batch in one step: ``FusedMMIMDbPatternStep`` (both fusion legs,
GMU and the five pooling kinds), ``MMIMDb.pattern_step_for``, an ``"all_patterns"`` batch in ``train_step`` and
``fit_mmimdb(all_patterns=True)``.

The criterion is tests/test_gpu_mmimdb.py's (tests/parity.py): the CPU oracle's ``train_step`` on the EXPLICITLY replicated
and masked P·B-row batch, in fp64 with our MaxOut unit choices forced into it, is the truth; the same in fp32 is the
yardstick wherever P·B >= 32 (that file's row threshold); logits / loss rel-L2 <= 1e-4, every gradient rel-L2 <= 1e-3 and
cosine >= 0.9999, running statistics <= 1e-3; Adam exact; every step checked from our own state (eager, capture, replay)."""
import copy

import pytest
import torch

import tspm_amd
from oracle import mmimdb_ref as orc
from parity import GRAD_REL, MAX_FLIP_FRAC, NEAR, Tally, check_adam, check_grad, check_out, op_check, snapshot
from test_gpu_mmimdb import LR, WD, _flips, _sync_oracle
from test_mmimdb_cpu import POOL_KINDS, dropin, pool_cfg
from tspm_amd import _lib as L
from tspm_amd import mmimdb as M

pytestmark = pytest.mark.gpu

ALL = ("it", "i", "t")
H = 512


def _keep(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(2, n, H, generator=g) >= 0.5).to(torch.uint8)


def _replicate(I, T, y, pats):
    """The P·B-row batch the step stands for: row p·B + b is sample b with the modality pattern p drops zeroed."""
    return (torch.cat([I * M.PATTERNS[p][0] for p in pats]), torch.cat([T * M.PATTERNS[p][1] for p in pats]),
            y.repeat(len(pats), 1))


def _decisions(st):
    """Our MaxOut unit choices (0 / 1 / 2 = tie) from the classifier engine's saved unit outputs A1, A2 [P·B, 2h]."""
    out = {}
    for site, A in (("mo1", st.clf.A1), ("mo2", st.clf.A2)):
        a = A.detach().cpu()
        a0, a1 = a[:, :H], a[:, H:]
        out[site] = torch.where(a1 > a0, 1, torch.where(a1 == a0, 2, 0)).to(torch.int8)
    return out


def _check(name, ours, st, o32, o64, I, T, y, keep, out, tally, vs32, kpool=None):
    """test_gpu_mmimdb.py::_check with the oracle on the replicated masked batch."""
    Ir, Tr, yr = _replicate(I, T, y, st.patterns)
    forced = _decisions(st)
    if kpool is not None and st.model.fusion_module.pooling_type == "max":
        ab = st.clf.H.detach().cpu()
        a, b = ab[:, :H], ab[:, H:]
        forced["pool"] = torch.where(b > a, 1, torch.where(b == a, 2, 0)).to(torch.int8)
    t32, t64 = orc.MaxOutTrace(forced), orc.MaxOutTrace(forced)
    r32 = orc.train_step(o32, None, Ir, Tr, yr, keep[0], keep[1], t32, keep_pool=kpool)
    r64 = orc.train_step(o64, None, Ir.double(), Tr.double(), yr.double(), keep[0], keep[1], t64, keep_pool=kpool)
    rep = _flips(t64, forced, keep)
    if "pool" in forced:
        a0, a1 = t64.units["pool"]
        flip = forced["pool"] != (a1 > a0).to(torch.int8)
        flip &= ~((a0 == 0) & (a1 == 0))  # both dropped: exact tie either way
        rms = torch.cat([a0, a1]).pow(2).mean().sqrt().item()
        worst = ((a1 - a0).abs()[flip].max().item() / rms) if flip.any() else 0.0
        assert worst <= NEAR and int(flip.sum()) <= max(1, MAX_FLIP_FRAC * flip.numel()), (int(flip.sum()), worst)
    logits = out["logits"].reshape(-1, out["logits"].shape[-1])
    check_out(f"logits {name}", logits, r32["logits"] if vs32 else None, r64["logits"], tally)
    check_out(f"loss {name}", out["loss"], r32["loss"] if vs32 else None, r64["loss"], tally)
    p32, p64 = dict(o32.named_parameters()), dict(o64.named_parameters())
    for pname, p in ours.named_parameters():
        check_grad(f"{pname} {name}", p.grad, p32[pname].grad if vs32 else None, p64[pname].grad, tally)
    s32, s64 = o32.state_dict(), o64.state_dict()
    for k, v in ours.state_dict().items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            check_out(f"{k} {name}", v, s32[k] if vs32 else None, s64[k], tally, bound=GRAD_REL)
    return rep


def _setup(gpu, B, pats, fusion, seed=0, pooling=None, graph=True):
    ours = dropin(seed, pooling).to(gpu)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=LR, weight_decay=WD)
    st = M.FusedMMIMDbPatternStep(ours, opt, None, B, patterns=pats, fusion=fusion, use_graph=graph)
    o32 = orc.build_oracle_mmimdb(seed, pooling=pooling)
    return ours, opt, st, o32, copy.deepcopy(o32).double()


@pytest.mark.parametrize("fusion", ["kernel", "launches"])
@pytest.mark.parametrize("pats", [ALL, ("t", "it")], ids=["all", "t+it"])
@pytest.mark.parametrize("B", [2, 11, 64])
def test_pattern_step_vs_oracle(gpu, B, pats, fusion):
    ours, opt, st, o32, o64 = _setup(gpu, B, pats, fusion)
    assert st.fusion == fusion and st.patterns == tuple(pats) and st.P == len(pats)
    N = st.P * B
    I, T, y = orc.synthetic_batch(B, seed=77 + B)
    tally = Tally()
    for s in range(3):  # eager, capture, replay
        keep = _keep(N, 10 + s)
        if s > 0:
            _sync_oracle(ours, opt, o32)
            _sync_oracle(ours, opt, o64)
        before = snapshot(ours, opt if s else None)
        st.keep_override = keep.to(gpu)
        out = st.step(I.to(gpu), T.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        assert out["logits"].shape == (st.P, B, 23) and out["loss"].shape == (1,)
        rep = _check(f"s{s}", ours, st, o32, o64, I, T, y, keep, out, tally, vs32=N >= 32)
        check_adam(ours, opt, *before, s + 1, lr=LR, wd=WD)
        print(f"[B={B} {'+'.join(pats)} {fusion} step {s + 1}] maxout flips {rep}")
    assert st.graph is not None and st.calls == 3
    for k, v in ours.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 3, k
    print(tally)


def test_legs_agree_and_replays_repeat(gpu):
    """The two fusion legs on one GMU model, one step from the same state: every gradient of the kernel leg within
    op_check's bound of the launches leg against the fp64 oracle.  Then the same step replayed from a restored state:
    the same bits."""
    B, pats = 11, ALL
    N = len(pats) * B
    I, T, y = orc.synthetic_batch(B, seed=5)
    keep = _keep(N, 3)
    runs = {}
    for fusion in ("kernel", "launches"):
        ours, opt, st, o32, o64 = _setup(gpu, B, pats, fusion)
        st.keep_override = keep.to(gpu)
        out = st.step(I.to(gpu), T.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        runs[fusion] = (ours, st, {k: v.detach().cpu().clone() for k, v in out.items()},
                        {n: p.grad.detach().cpu().clone() for n, p in ours.named_parameters()})
        if fusion == "kernel":
            forced = _decisions(st)
            Ir, Tr, yr = _replicate(I, T, y, pats)
            orc.train_step(o64, None, Ir.double(), Tr.double(), yr.double(), keep[0], keep[1], orc.MaxOutTrace(forced))
            truth = {n: p.grad.detach().clone() for n, p in o64.named_parameters()}
    (_, _, out_k, g_k), (_, _, out_l, g_l) = runs["kernel"], runs["launches"]
    assert torch.equal(out_k["logits"], out_l["logits"])  # the forward legs are bitwise equal (tspm_gmu_pattern_fwd)
    for n in g_k:
        op_check(f"legs.{n}", g_k[n], g_l[n], truth[n], grad=True)
    # replays: restore the parameters the step started from (in place: the graph holds their addresses), replay,
    # compare logits, loss and every gradient bit for bit (the masks are given; Adam runs after the gradients)
    ours, st = runs["kernel"][:2]
    st.step(I.to(gpu), T.to(gpu), y.to(gpu))  # capture
    torch.cuda.synchronize()
    saved = copy.deepcopy(ours.state_dict())
    first = None
    for _ in range(2):
        ours.load_state_dict(saved)
        out = st.step(I.to(gpu), T.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        got = [out["logits"].clone(), out["loss"].clone()] + [p.grad.clone() for p in ours.parameters()]
        if first is None:
            first = got
        else:
            assert all(torch.equal(a, b) for a, b in zip(first, got))


@pytest.mark.parametrize("kind", POOL_KINDS)
def test_pooling_takes_the_launches_leg(gpu, kind):
    B, pats = 5, ALL
    N = len(pats) * B
    cfg = pool_cfg(kind)
    ours, opt, st, o32, o64 = _setup(gpu, B, pats, None, pooling=cfg)
    assert st.fusion == "launches"  # the default leg falls back: no pattern kernel for the pooling
    I, T, y = orc.synthetic_batch(B, seed=88)
    tally = Tally()
    for s in range(2):
        keep = _keep(N, 20 + s)
        kp = (torch.rand(N, 2 * H, generator=torch.Generator().manual_seed(40 + s)) >= 0.1).to(torch.uint8)
        if s > 0:
            _sync_oracle(ours, opt, o32)
            _sync_oracle(ours, opt, o64)
        before = snapshot(ours, opt if s else None)
        st.keep_override = keep.to(gpu)
        st.clf.pool_keep_override = kp.to(gpu)
        out = st.step(I.to(gpu), T.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        _check(f"{kind} s{s}", ours, st, o32, o64, I, T, y, keep, out, tally, vs32=N >= 32,
               kpool=(kp[:, :H], kp[:, H:]))
        check_adam(ours, opt, *before, s + 1, lr=LR, wd=WD)
    print(f"[{kind}] {tally}")


def test_default_dropout_is_the_plain_steps_at_pb_rows(gpu):
    """Without keep_override the masks are those a FusedMMIMDbStep at n = P·B draws with the same seed and counter."""
    B, pats = 8, ALL
    N = len(pats) * B
    I, T, y = orc.synthetic_batch(B, seed=9)
    ours, opt, st, _, _ = _setup(gpu, B, pats, "kernel")
    plain_m = dropin(0).to(gpu)
    plain_m._rng_seed = ours._rng_seed
    plain = M.FusedMMIMDbStep(plain_m, tspm_amd.FusedAdam(plain_m.parameters(), lr=LR, weight_decay=WD), None, N)
    Ir, Tr, yr = (t.to(gpu) for t in _replicate(I, T, y, pats))
    masks = []
    for _ in range(3):  # eager, capture, replay: the counter advances with the optimizer's step
        st.step(I.to(gpu), T.to(gpu), y.to(gpu))
        plain.step(Ir, Tr, yr)
        torch.cuda.synchronize()
        assert st.keep.shape == (2, N, H) and torch.equal(st.keep, plain.eng.keep)
        masks.append(st.keep.clone())
    assert not torch.equal(masks[0], masks[1]) and not torch.equal(masks[1], masks[2])
    assert 0.47 < torch.stack(masks).float().mean().item() < 0.53


def test_it_alone_is_the_plain_step(gpu):
    """patterns=("it",): the replicated batch is the batch; the gradients are the plain step's within check_grad."""
    B = 8
    I, T, y = orc.synthetic_batch(B, seed=13)
    keep = _keep(B, 7)
    ours, opt, st, o32, o64 = _setup(gpu, B, ("it",), None)
    st.keep_override = keep.to(gpu)
    out = st.step(I.to(gpu), T.to(gpu), y.to(gpu))
    plain_m = dropin(0).to(gpu)
    plain = M.FusedMMIMDbStep(plain_m, tspm_amd.FusedAdam(plain_m.parameters(), lr=LR, weight_decay=WD), None, B)
    plain.keep_override = keep.to(gpu)
    ref = plain.step(I.to(gpu), T.to(gpu), y.to(gpu))
    torch.cuda.synchronize()
    r64 = orc.train_step(o64, None, I.double(), T.double(), y.double(), keep[0], keep[1],
                         orc.MaxOutTrace(_decisions(st)))
    tally = Tally()
    check_out("logits", out["logits"][0], ref["logits"], r64["logits"], tally)
    check_out("loss", out["loss"], ref["loss"], r64["loss"], tally)
    p64 = dict(o64.named_parameters())
    for (n, p), q in zip(ours.named_parameters(), plain_m.parameters()):
        check_grad(n, p.grad, q.grad, p64[n].grad, tally)
    print(tally)


def test_train_step_with_an_all_patterns_batch(gpu):
    B = 6
    ours = dropin(0).to(gpu)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=LR, weight_decay=WD)
    I, T, y = orc.synthetic_batch(B, seed=21)

    class Rec:
        def update_group_all(self, group, predictions, targets, m_types):
            self.got = (group, predictions.shape, targets.shape, list(m_types))
    rec = Rec()
    batch = {"image": I, "text": T, "label": y, "all_patterns": True, "patterns": ("t", "it")}
    r = ours.train_step(batch, opt, None, gpu, rec)
    assert torch.isfinite(torch.tensor(r["loss"]))
    assert rec.got == ("classification", (2 * B, 23), (2 * B, 23), ["t"] * B + ["it"] * B)
    st = ours.pattern_step_for(opt, None, B, ("t", "it"))
    assert st.calls == 1 and ours.pattern_step_for(opt, None, B, ["t", "it"]) is st
    ours.train_step({"image": I, "text": T, "label": y, "all_patterns": True}, opt, None, gpu)
    assert ours.pattern_step_for(opt, None, B).patterns == ALL and ours.pattern_step_for(opt, None, B) is not st
    with pytest.raises(ValueError):
        ours.train_step(dict(batch, patterns=("it", "x")), opt, None, gpu)
    ours.to(gpu)  # _apply drops the cached steps: their graphs are bound to the old storage
    assert "_pattern_steps" not in ours.__dict__


def test_fit_mmimdb_all_patterns(gpu):
    """Two epochs on 40 synthetic samples at batch 16 (a last partial batch of 8, through a second step): the plain
    loop's history keys, finite losses, and the train counts over all P·B rows of every batch."""
    I, T, y = orc.synthetic_batch(40, seed=41)
    Iv, Tv, yv = orc.synthetic_batch(20, seed=42)
    hists = {}
    for all_patterns in (False, True):
        ours = dropin(2).to(gpu)
        opt = tspm_amd.FusedAdam(ours.parameters(), lr=1e-4, weight_decay=1e-3)
        hists[all_patterns] = M.fit_mmimdb(ours, opt, M.MMIMDbCorpus(I, T, y, gpu), M.MMIMDbCorpus(Iv, Tv, yv, gpu), 16,
                                           epochs=2, all_patterns=all_patterns)
    plain, fused = hists[False], hists[True]
    assert len(fused) == 2
    for a, b in zip(plain, fused):
        assert set(a) == set(b) and set(a["train"]) == set(b["train"])
        assert all(set(a[k]) == set(b[k]) for k in a if k.startswith("val_") and k != "val_loss")
        vals = [b["train"]["loss"], b["val_loss"]] + [b[f"val_{p}"]["loss"] for p in ALL]
        assert all(torch.isfinite(torch.tensor(v)) for v in vals)
    # last epoch's optimizer steps: 3 per epoch either way (16 + 16 + 8)
    assert int(ours.mm_mlp.net[0].num_batches_tracked) == 6
