"""Frozen encoders and per-group Adam in the UTT-Fusion fused step, model level: ``FusedMosiStep`` with 1..8 ``FusedAdam``
groups (``tspm_grad_clip_coef_multi`` / ``tspm_adam_begin_multi`` / ``tspm_adam_step_multi``), encoders with
``requires_grad_(False)`` (their backward skipped), ``mosi.finetune_param_groups`` and the other readers of such a model.

The oracle is oracle/mosi_ref.py with the same ``requires_grad`` flags; the checks, tolerances, forced decisions and
dropout-mask injection are those of test_gpu_mosi.py (``_check_step``) on the shapes of
test_gpu_mosi_text_lengths.py (B = 6, steps (9, 11, 8)).  The optimizer is held, per group at the group's own
hyper-parameters, to parity.adam_fp64 within parity.adam_tolerance and to an fp64 ``torch.optim.Adam`` of the same groups
stepped from our state on our gradients; the clip total to the float32 neighbours of the fp64 norm of our gradients.
"""
import copy

import numpy as np
import pytest
import torch

import test_gpu_mosi as tm
import test_gpu_mosi_lengths as tl
import test_gpu_mosi_regress as tr
import test_gpu_mosi_text_lengths as tx
import tspm_amd
from oracle import mosi_ref as orc
from parity import Tally, adam_fp64, adam_tolerance, check_grad, check_out, pair_from
from test_gpu_seq_ops import _neighbours
from test_mosi_cpu import _dropin
from tspm_amd import _lib as L
from tspm_amd import mosi as M
from tspm_amd.mosi_data import MOSI, synthetic_mosi_corpus

pytestmark = pytest.mark.gpu
B, STEPS = tx.B, tx.STEPS
FULL = {"audio": [STEPS[0]] * B, "video": [STEPS[1]] * B, "text": [STEPS[2]] * B}
SEEDS = dict(model=3, batch=100, keep=50)
ATTR = dict(M.ENCODER_MODULES)
FROZEN_SETS = [("audio", "video"), ("text",), ("audio",), ("audio", "video", "text")]
OLD_OPT = ["tspm_grad_clip_coef", "tspm_adam_begin", "tspm_adam_step_clip"]
NEW_OPT = ["tspm_grad_clip_coef_multi", "tspm_adam_begin_multi", "tspm_adam_step_multi"]


def _cfg(name):
    return orc.MOSI if name == "mosi" else orc.MOSEI


class _Recorder:
    """``L.lib()`` with every tspm_* call noted by name (the step's launch record, taken on an eager step)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("tspm_"):
            return fn

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call


def _record(monkeypatch):
    rec = _Recorder(L.lib())
    monkeypatch.setattr(L, "lib", lambda: rec)
    return rec


def _opt_calls(calls):
    """The optimizer phase of a launch record (the workspace query at construction is no launch)."""
    return [c for c in calls if "adam" in c or "clip_coef" in c]


def _freeze(model, frozen):
    for name in frozen:
        getattr(model, ATTR[name]).requires_grad_(False)
    return model


def _snap(model, opt, with_state):
    p = {n: q.detach().cpu().double().clone() for n, q in model.named_parameters()}
    if not with_state:
        return p, None, None
    live = [(n, q) for n, q in model.named_parameters() if q.requires_grad]
    return (p, {n: opt.state[q]["exp_avg"].detach().cpu().double().clone() for n, q in live},
            {n: opt.state[q]["exp_avg_sq"].detach().cpu().double().clone() for n, q in live})


def _check_groups_adam(ours, opt, before, step, coef):
    """Every group's update at the group's own hyper-parameters: fp64 Adam (parity.adam_fp64) on OUR gradient x the clip
    coefficient and OUR moments, within parity.adam_tolerance; and an fp64 torch.optim.Adam of the same groups, given our
    state, gradients and step count, lands within the same tolerance."""
    names = {id(p): n for n, p in ours.named_parameters()}
    pb, mb, vb = before
    groups, clones = [], {}
    for g in opt.param_groups:
        lr, wd, (b1, b2), eps = g["lr"], g["weight_decay"], g["betas"], g["eps"]
        qs = []
        for p in g["params"]:
            if not p.requires_grad:
                continue
            n = names[id(p)]
            grad = p.grad.detach().cpu().double() * coef
            exp, _, v = adam_fp64(pb[n], grad, step, lr=lr, wd=wd, b1=b1, b2=b2, eps=eps,
                                  m=None if mb is None else mb[n], v=None if vb is None else vb[n])
            tol = 1e-6 * exp.abs() + adam_tolerance(pb[n], grad, step, v, lr, wd, b1=b1, b2=b2, eps=eps)
            got = p.detach().cpu().double()
            bad = (got - exp).abs() > tol
            assert not bad.any(), (n, step, lr, int(bad.sum()), ((got - exp).abs() / tol).max().item())
            q = pb[n].clone().contiguous().requires_grad_(True)
            q.grad = grad.clone().contiguous()
            clones[n] = (q, got, tol)
            qs.append(q)
        if qs:
            groups.append(dict(params=qs, lr=lr, weight_decay=wd, betas=(b1, b2), eps=eps))
    ref = torch.optim.Adam(groups, foreach=False)
    if mb is not None:
        for n, (q, _, _) in clones.items():
            ref.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": mb[n].clone().contiguous(),
                            "exp_avg_sq": vb[n].clone().contiguous()}
    ref.step()
    for n, (q, got, tol) in clones.items():
        assert bool(((got - q.detach()).abs() <= tol).all()), ("torch.optim.Adam", n, step)


def _norm_of_our_gradients(ours):
    return np.float32(np.sqrt(sum((p.grad.double() ** 2).sum().item() for p in ours.parameters() if p.grad is not None)))


def _check(ours, st, o32, o64, A, V, T, y, keeps, out, tally, regress=None):
    """test_gpu_mosi._check_step (test_gpu_mosi_regress._check_step with ``regress`` = (kind, weight)) for a model with
    frozen encoders: the oracle carries the same flags; a frozen parameter has no gradient on either side, every other
    gradient, the logits, the loss, the total norm and the BatchNorm buffers meet that function's bounds."""
    eng = st.eng
    forced = tm._decisions(eng)
    t32, t64 = orc.MosiTrace(forced), orc.MosiTrace(forced)
    if regress is not None:
        r32 = tr._oracle_step(o32, A, V, T, y, keeps, t32, *regress)
        r64 = tr._oracle_step(o64, A.double(), V.double(), T.double(), y, keeps, t64, *regress)
    else:
        o32.clip = o64.clip = None  # raw gradients; the clip is checked through the total norm
        r32 = orc.train_step(o32, None, A, V, T, y, keeps, t32)
        r64 = orc.train_step(o64, None, A.double(), V.double(), T.double(), y, keeps, t64)
    rep = tm._flips(t64, forced, keeps, eng.use_bn)
    check_out("logits", out["logits"], r32["logits"], r64["logits"], tally)
    check_out("loss", out["loss"], r32["loss"].reshape(1), r64["loss"].reshape(1), tally)
    p32, p64 = dict(o32.named_parameters()), dict(o64.named_parameters())
    for n, p in ours.named_parameters():
        if not p.requires_grad:
            assert p.grad is None and p64[n].grad is None, n
            continue
        check_grad(f"grad {n}", p.grad, p32[n].grad, p64[n].grad, tally)
    norm64 = torch.sqrt(sum((q.grad.double() ** 2).sum() for q in o64.parameters() if q.grad is not None))
    norm32 = torch.sqrt(sum((q.grad.double() ** 2).sum() for q in o32.parameters() if q.grad is not None))
    check_out("total grad norm", eng.total_norm, norm32.reshape(1), norm64.reshape(1), tally)
    if eng.use_bn:
        b32, b64 = dict(o32.named_buffers()), dict(o64.named_buffers())
        for n, b in ours.named_buffers():
            if n.endswith("num_batches_tracked"):
                assert int(b) == int(b64[n]), n
            else:
                check_out(n, b, b32[n], b64[n], tally)
    return rep


def _oracles(ours, frozen, build):
    o32, o64 = pair_from(ours, build)  # re-anchored to our state
    for o in (o32, o64):
        _freeze(o, frozen)
    return o32, o64


def _check_total(ours, st):
    total = st.eng.total_norm.item()
    want = _norm_of_our_gradients(ours)
    print(f"total norm {total:.9e}, fp64 norm of our gradients {float(want):.9e}")
    assert total in _neighbours(want), (total, float(want))
    coef = float(st.eng.clip_coef.item())
    exp = min(1.0, ours.clip / (total + 1e-6))
    assert abs(coef - exp) <= 1e-6 * exp
    return coef


# ------------------------------------------------------------------------------------------------
# two groups against fp64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mosi", "mosei"])
def test_two_group_fused_steps_vs_fp64_on_one_graph(gpu, monkeypatch, name):
    """Classifier group at lr 1e-3 / wd 1e-3, encoder group at lr 1e-4 / wd 0, the clip active (MOSEI's YAML value 0.5 is
    below its gradient norms; MOSI's 1.0 is not at this batch, so 0.05 as in test_gpu_mosi's clipped case): three fused
    steps (eager, captured, replayed) under test_gpu_mosi._check_step."""
    cfg = _cfg(name)
    ours = _dropin(SEEDS["model"], clip=0.05 if name == "mosi" else None, cfg=cfg).to(gpu)
    groups = M.finetune_param_groups(ours, lr=1e-3, weight_decay=1e-3, encoder_lr=1e-4, encoder_weight_decay=0.0)
    assert [(g["lr"], g["weight_decay"]) for g in groups] == [(1e-3, 1e-3), (1e-4, 0.0)]
    opt = tspm_amd.FusedAdam(groups)
    rec = _record(monkeypatch)
    st = ours.fused_step(opt, None, B, STEPS)
    assert st.multi and st.frozen == () and list(ours._steps) == [(id(opt), id(None), B, M.norm_steps(STEPS))]
    assert st.eng.rng_ctr_ptr == opt.flat_groups()[0].hyper.data_ptr() + L.HYPER_STEP_OFFSET
    tally, graph = Tally(), None
    for s in range(3):
        A, V, T, y = tx._batch(cfg, FULL, seed=SEEDS["batch"] + s)
        keeps = orc.keep_masks(B, SEEDS["keep"] + s, cfg=cfg)
        o32, o64 = _oracles(ours, (), lambda: orc.build_oracle_utt(SEEDS["model"], cfg=cfg))
        before = _snap(ours, opt, s > 0)
        st.keep_override = {k: v.to(gpu) for k, v in keeps.items()}
        out = st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        if s == 0:  # the optimizer phase of the eager step: the four launches of one group (two per clip call)
            assert _opt_calls(rec.calls) == NEW_OPT
        rep = tm._check_step(ours, st, o32, o64, A, V, T, y, keeps, out, tally)
        coef = _check_total(ours, st)
        assert coef < 1.0  # the clip acts
        _check_groups_adam(ours, opt, before, s + 1, coef)
        steps = [int(fg.hyper.view(torch.int64)[6]) for fg in opt.flat_groups()]
        assert steps == [s + 1, s + 1]  # all groups advance together
        print(f"[{name} two groups step {s + 1}] flips {rep} clip coef {coef:.4f}")
        if s == 1:
            graph = st.graph
            assert graph is not None
    assert st.graph is graph and st.calls == 3
    print(tally)


def test_two_groups_of_equal_hypers_are_the_one_group_step_bitwise(gpu):
    """clip=None, injected masks: parameters, loss and logits after three steps are bitwise the one-group step's (Adam
    is element-wise).  With the clip active this is not required and not asserted: the sum of squares is partitioned
    over two buffers instead of one, so its double partials are added in another order."""
    cfg = orc.MOSI
    res = []
    for two in (False, True):
        m = _dropin(4, cfg=cfg).to(gpu)
        m.clip = None
        if two:
            opt = tspm_amd.FusedAdam(M.finetune_param_groups(m, lr=cfg.lr, weight_decay=cfg.weight_decay,
                                                             encoder_lr=cfg.lr))
            assert len(opt.flat_groups()) == 2
        else:
            opt = tspm_amd.FusedAdam(m.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
        st = m.fused_step(opt, None, B, STEPS)
        assert st.multi == two
        for s in range(3):
            A, V, T, y = tx._batch(cfg, FULL, seed=20 + s)
            st.keep_override = {k: v.to(gpu) for k, v in orc.keep_masks(B, 60 + s, cfg=cfg).items()}
            st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        res.append([p.detach().clone() for p in m.parameters()] + [st.eng.logits.clone(), st.eng.loss.clone()])
    for p, q in zip(*res):
        assert torch.equal(p, q)


# ------------------------------------------------------------------------------------------------
# frozen sets
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mosi", "mosei"])
@pytest.mark.parametrize("frozen", FROZEN_SETS, ids=["+".join(f) for f in FROZEN_SETS])
def test_frozen_encoders_vs_fp64_and_graph_equals_eager(gpu, monkeypatch, name, frozen):
    cfg = _cfg(name)
    rec = _record(monkeypatch)
    res = []
    for use_graph in (False, True):
        ours = _dropin(SEEDS["model"], cfg=cfg).to(gpu)
        groups = M.finetune_param_groups(ours, lr=1e-3, weight_decay=1e-3, encoder_lr=1e-4, encoder_weight_decay=0.0,
                                         freeze=frozen)
        assert len(groups) == (1 if len(frozen) == 3 else 2) and M.frozen_encoders(ours) == frozen
        opt = tspm_amd.FusedAdam(groups)
        frozen_before = {n: p.detach().clone() for n, p in ours.named_parameters() if not p.requires_grad}
        assert bool(frozen_before) and all(p.grad is None for p in ours.parameters() if not p.requires_grad)
        st = M.FusedMosiStep(ours, opt, None, B, STEPS, use_graph=use_graph)
        assert st.frozen == frozen == st.eng.frozen
        for k, nm in (("a", "audio"), ("v", "video")):
            assert (st.eng.lstm[k]["dg"] is None) == (nm in frozen)
        tally = Tally()
        for s in range(3):
            A, V, T, y = tx._batch(cfg, FULL, seed=SEEDS["batch"] + s)
            keeps = orc.keep_masks(B, SEEDS["keep"] + s, cfg=cfg)
            st.keep_override = {k: v.to(gpu) for k, v in keeps.items()}
            if use_graph:
                st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
                continue
            o32, o64 = _oracles(ours, frozen, lambda: orc.build_oracle_utt(SEEDS["model"], cfg=cfg))
            before = _snap(ours, opt, s > 0)
            del rec.calls[:]
            out = st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
            torch.cuda.synchronize()
            calls = list(rec.calls)
            rep = _check(ours, st, o32, o64, A, V, T, y, keeps, out, tally)
            coef = _check_total(ours, st)
            _check_groups_adam(ours, opt, before, s + 1, coef)
            print(f"[{name} frozen {frozen} step {s + 1}] flips {rep} clip coef {coef:.4f}")
            # the launch record: what a frozen encoder no longer costs
            bwd = [c for c in calls if c.startswith("tspm_lstm_bwd")]
            assert len(bwd) == (0 if {"audio", "video"} <= set(frozen) else 1)
            assert calls.count("tspm_linear_bwd_weight_splitk") == 2 * (2 - len({"audio", "video"} & set(frozen)))
            assert ("tspm_textcnn_bwd" in calls) == ("text" not in frozen)
            assert _opt_calls(calls) == (OLD_OPT if len(groups) == 1 else NEW_OPT)
        torch.cuda.synchronize()
        if use_graph:
            assert st.graph is not None
        else:
            print(tally)
        for n, p in ours.named_parameters():
            if not p.requires_grad:
                assert p.grad is None and torch.equal(p.detach(), frozen_before[n]), n  # bitwise unchanged
        res.append(torch.cat([t.detach().reshape(-1).double() for t in ours.state_dict().values()]
                             + [st.eng.logits.reshape(-1).double(), st.eng.loss.double()]).cpu())
    assert torch.equal(res[0], res[1])  # graph replay = eager, bitwise


def test_changed_flags_are_refused_by_the_built_step(gpu):
    ours = _dropin(1).to(gpu)
    opt = tspm_amd.FusedAdam(M.finetune_param_groups(ours, lr=1e-3, weight_decay=1e-3, freeze=("video",)))
    st = ours.fused_step(opt, None, B, STEPS)
    A, V, T, y = tx._batch(orc.MOSI, FULL)
    st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
    assert [k[-1] for k in ours._steps] == [("frozen", ("video",))]
    ours.netA.requires_grad_(False)
    with pytest.raises(L.TspmError, match="requires_grad flags changed"):
        st.run()
    ours.netA.requires_grad_(True)
    st.run()
    # what the step refuses at construction (the CPU file holds check_param_groups to the same cases)
    with pytest.raises(L.TspmError, match="allreduce"):
        two = _dropin(1).to(gpu)
        M.FusedMosiStep(two, tspm_amd.FusedAdam(M.finetune_param_groups(two, lr=1e-3, weight_decay=0.0, encoder_lr=1e-4)),
                        None, B, STEPS, allreduce=lambda: None)
    with pytest.raises(L.TspmError, match="netT.embd.0.bias"):
        part = _dropin(1).to(gpu)
        M.FusedMosiStep(part, tspm_amd.FusedAdam([p for n, p in part.named_parameters() if n != "netT.embd.0.bias"],
                                                 lr=1e-3), None, B, STEPS)


def test_flags_changed_after_the_optimizer_was_built_are_refused(gpu):
    """FusedAdam's flat buffers hold what was trainable when it was built.  Frozen afterwards, an encoder would still be
    updated (weight decay, stale gradients in the clip norm); unfrozen afterwards, it has no gradient buffer.  Both orders
    are refused by a new step; with a new optimizer the frozen encoder stays bitwise where it was."""
    A, V, T, y = tx._batch(orc.MOSI, FULL)
    ours = _dropin(2).to(gpu)
    opt = tspm_amd.FusedAdam(ours.parameters(), lr=1e-3, weight_decay=1e-3)
    ours.fused_step(opt, None, B, STEPS).step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
    ours.netA.requires_grad_(False)  # after the optimizer was built
    with pytest.raises(L.TspmError, match=r"netA\.rnn\.weight_ih_l0 is in FusedAdam's flat buffers.*rebuild FusedAdam"):
        ours.fused_step(opt, None, B, STEPS)
    before = {n: p.detach().clone() for n, p in ours.netA.named_parameters()}
    opt2 = tspm_amd.FusedAdam(ours.parameters(), lr=1e-3, weight_decay=1e-3)  # rebuilt: netA is in no flat buffer
    st = ours.fused_step(opt2, None, B, STEPS)
    assert st.frozen == ("audio",)
    for _ in range(2):
        st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
    torch.cuda.synchronize()
    for n, p in ours.netA.named_parameters():
        assert torch.equal(p.detach(), before[n]), n
    ours.netA.requires_grad_(True)  # the reverse order: unfrozen after opt2 was built
    with pytest.raises(L.TspmError, match=r"netA\.rnn\.weight_ih_l0 is not in FusedAdam's flat buffers.*rebuild FusedAdam"):
        ours.fused_step(opt2, None, B, STEPS)
    with pytest.raises(L.TspmError, match="build a new FusedAdam"):
        st.run()


def test_the_autograd_node_reads_the_flags_at_backward_time(gpu):
    """Mixed flags are refused in the backward while they are mixed, and no longer once corrected (the engine of the
    all-trainable key is the same object throughout)."""
    A, V, T, y = tx._batch(orc.MOSI, FULL)
    m = _dropin(2).to(gpu).train()

    def loss():
        return torch.nn.functional.cross_entropy(m(A.to(gpu), V.to(gpu), T.to(gpu)), y.to(gpu))
    loss().backward()  # the engine is built with clean flags
    eng = m._engine(B, STEPS, gpu)
    m.netV.rnn.bias_hh_l0.requires_grad_(False)
    with pytest.raises(L.TspmError, match="netV.*mixed requires_grad"):
        loss().backward()
    m.netV.rnn.bias_hh_l0.requires_grad_(True)
    loss().backward()
    assert m._engine(B, STEPS, gpu) is eng and len(m._engines) == 1


# ------------------------------------------------------------------------------------------------
# the other paths
# ------------------------------------------------------------------------------------------------
def test_autograd_node_skips_the_frozen_encoders(gpu, monkeypatch):
    """The reference's own sequence with torch.optim.Adam: frozen parameters get None, the others the fused step's
    gradients bitwise (same kernels, same buffers' contents)."""
    cfg, frozen = orc.MOSI, ("audio", "text")
    A, V, T, y = tx._batch(cfg, FULL)
    keeps = {k: v.to(gpu) for k, v in orc.keep_masks(B, 9, cfg=cfg).items()}
    fused = _freeze(_dropin(6, cfg=cfg).to(gpu), frozen)
    fused.clip = None
    opt = tspm_amd.FusedAdam(fused.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
    st = fused.fused_step(opt, None, B, STEPS)
    st.keep_override = keeps
    st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
    auto = _freeze(_dropin(6, cfg=cfg).to(gpu), frozen).train()
    auto.clip = None
    topt = torch.optim.Adam([p for p in auto.parameters() if p.requires_grad], lr=cfg.lr, weight_decay=cfg.weight_decay)
    eng = auto._engine(B, STEPS, gpu)
    assert eng.frozen == frozen and list(auto._engines) == [(B, M.norm_steps(STEPS), gpu, ("frozen", frozen))]
    eng.keep_override = keeps
    rec = _record(monkeypatch)
    logits = auto(A.to(gpu), V.to(gpu), T.to(gpu))  # the autograd node
    # the node's backward from the fused step's own dlogits (tspm_cross_entropy's; torch's cross-entropy backward rounds
    # them differently, which is the loss's business, not the node's): the same kernels on the same inputs
    logits.backward(st.eng.dlogits.clone())
    torch.cuda.synchronize()
    assert "tspm_textcnn_bwd" not in rec.calls and rec.calls.count("tspm_linear_bwd_weight_splitk") == 2
    assert torch.equal(logits, st.eng.logits)
    for (n, p), (_, q) in zip(auto.named_parameters(), fused.named_parameters()):
        if p.requires_grad:
            assert torch.equal(p.grad, q.grad), n
        else:
            assert p.grad is None and q.grad is None, n
    before = {n: p.detach().clone() for n, p in auto.named_parameters()}
    topt.step()
    for n, p in auto.named_parameters():
        assert torch.equal(p.detach(), before[n]) == (not p.requires_grad), n
    # train_step's non-fused branch, validation_step and get_embeddings on the same model
    batch = {"audio": A, "video": V, "text": T, "label": y}
    assert np.isfinite(auto.train_step(batch, topt, lambda lg, lb: {"total_loss": torch.nn.functional.cross_entropy(lg, lb)},
                                       gpu, None)["loss"])
    assert np.isfinite(auto.validation_step(batch, None, gpu, None)["loss"])
    emb = auto.get_embeddings([batch], gpu)
    assert emb["audio"][0].shape == (B, 64) and np.isfinite(emb["text"][0]).all()
    assert np.isfinite(fused.train_step(batch, opt, None, gpu, None)["loss"]) and st.calls == 2


def test_frozen_lstms_with_ragged_and_text_lengths_vs_fp64(gpu, monkeypatch):
    cfg, frozen, lengths = orc.MOSEI, ("audio", "video"), tx.LENS[0]
    tx._patch(monkeypatch, lengths)
    ours = _dropin(SEEDS["model"], cfg=cfg).to(gpu)
    opt = tspm_amd.FusedAdam(M.finetune_param_groups(ours, lr=1e-3, weight_decay=1e-3, encoder_lr=1e-4,
                                                     encoder_weight_decay=0.0, freeze=frozen))
    st = ours.fused_step(opt, None, B, STEPS, ragged=True, text_lengths=True)
    assert list(ours._steps) == [(id(opt), id(None), B, M.norm_steps(STEPS), "ragged", "text_lengths", ("frozen", frozen))]
    A, V, T, y = tx._batch(cfg, lengths, seed=SEEDS["batch"])
    keeps = orc.keep_masks(B, SEEDS["keep"], cfg=cfg)
    o32, o64 = _oracles(ours, frozen, lambda: orc.build_oracle_utt(SEEDS["model"], cfg=cfg))
    before = _snap(ours, opt, False)
    st.keep_override = {k: v.to(gpu) for k, v in keeps.items()}
    out = st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu), tl._dev_lengths(lengths, gpu))
    torch.cuda.synchronize()
    tally = Tally()
    rep = _check(ours, st, o32, o64, A, V, T, y, keeps, out, tally)
    _check_groups_adam(ours, opt, before, 1, _check_total(ours, st))
    print(f"[ragged + text_lengths, frozen {frozen}] flips {rep}\n{tally}")


def test_regression_with_a_frozen_textcnn_vs_fp64(gpu):
    cfg, frozen = orc.MOSI, ("text",)
    ours = _freeze(tr._dropin(SEEDS["model"], cfg).to(gpu), frozen)
    opt = tspm_amd.FusedAdam(M.finetune_param_groups(ours, lr=1e-3, weight_decay=1e-3, encoder_lr=1e-4))
    group = tr.Group("l1", 1.0)
    st = ours.fused_step(opt, group, B, STEPS)
    assert st.regress is not None and st.frozen == frozen and st.multi
    A, V, T, _ = tx._batch(cfg, FULL, seed=SEEDS["batch"])
    y = tr._scores(B, 77)
    keeps = orc.keep_masks(B, SEEDS["keep"], cfg=cfg)
    o32, o64 = _oracles(ours, frozen, lambda: tr._oracle(SEEDS["model"], cfg))
    before = _snap(ours, opt, False)
    st.keep_override = {k: v.to(gpu) for k, v in keeps.items()}
    out = st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
    torch.cuda.synchronize()
    tally = Tally()
    rep = _check(ours, st, o32, o64, A, V, T, y, keeps, out, tally, regress=("l1", 1.0))
    _check_groups_adam(ours, opt, before, 1, _check_total(ours, st))
    print(f"[regression, frozen {frozen}] flips {rep}\n{tally}")


def test_fit_one_epoch_with_finetune_param_groups(gpu, tmp_path):
    from tspm_amd import harness
    ours = _dropin(8).to(gpu)
    opt = tspm_amd.FusedAdam(M.finetune_param_groups(ours, lr=1e-3, weight_decay=1e-3, encoder_lr=1e-4, freeze=("audio",)))
    frozen_before = {n: p.detach().clone() for n, p in ours.netA.named_parameters()}
    tr_ds = MOSI(split="train", corpus=synthetic_mosi_corpus(n=24, steps=12, min_len=2), device=gpu, seed=4)
    va_ds = MOSI(split="valid", corpus=synthetic_mosi_corpus(n=6, steps=12, min_len=2, seed=2), device=gpu)
    loaders = {"train": tr_ds.loader(8, shuffle=True, seed=1, pad_to=12), "validation": va_ds.loader(6, pad_to=12)}
    hist = harness.fit(ours, opt, None, loaders, epochs=1, early_stopping=False, checkpoint_dir=tmp_path)
    assert np.isfinite(hist["train"][-1]["loss"]) and np.isfinite(hist["validation"][-1]["loss"])
    assert [k[-1] for k in ours._steps] == [("frozen", ("audio",))]
    st = next(iter(ours._steps.values()))
    assert st.calls == 3 and st.multi and st.graph is not None
    for n, p in ours.netA.named_parameters():
        assert torch.equal(p.detach(), frozen_before[n]) and p.grad is None
    best = list(tmp_path.rglob("best.pth"))
    assert len(best) == 1
    sd = torch.load(best[0], map_location="cpu", weights_only=False)
    again = _dropin(9).to(gpu)
    again.load_state_dict(sd["model_state_dict"])
    for (n, p), (_, q) in zip(again.named_parameters(), ours.named_parameters()):
        assert torch.equal(p.detach().cpu(), q.detach().cpu()), n
    opt2 = tspm_amd.FusedAdam(M.finetune_param_groups(again, lr=1e-3, weight_decay=1e-3, encoder_lr=1e-4,
                                                      freeze=("audio",)))
    opt2.load_state_dict(copy.deepcopy(sd["optimizer_state_dict"]))
    assert [fg.step for fg in opt2.flat_groups()] == [3, 3]


def test_the_off_path_keeps_its_keys_and_entry_points(gpu, monkeypatch):
    """One group, nothing frozen: the engine and step keys as they always were, and the optimizer phase on the old entry
    points only (its bits against a build of the parent commit are the A/B of profiles/mosi_finetune.json)."""
    cfg = orc.MOSI
    m = _dropin(4, cfg=cfg).to(gpu)
    opt = tspm_amd.FusedAdam(m.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
    rec = _record(monkeypatch)
    st = m.fused_step(opt, None, B, STEPS)
    assert list(m._steps) == [(id(opt), id(None), B, M.norm_steps(STEPS))] and not st.multi and st.frozen == ()
    m._engine(B, STEPS, gpu)
    assert list(m._engines) == [(B, M.norm_steps(STEPS), gpu)]
    A, V, T, y = tx._batch(cfg, FULL)
    st.step(A.to(gpu), V.to(gpu), T.to(gpu), y.to(gpu))
    torch.cuda.synchronize()
    assert _opt_calls(rec.calls) == OLD_OPT
    assert not [c for c in rec.calls if c.endswith("_multi") and c != "tspm_linear_bwd_multi"]
    assert sum(c.startswith("tspm_lstm_bwd") for c in rec.calls) == 1 and "tspm_textcnn_bwd" in rec.calls
    assert rec.calls.count("tspm_linear_bwd_weight_splitk") == 4
