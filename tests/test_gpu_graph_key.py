"""What a captured step graph bakes in is its key (``_lib.GraphRunner``): a log assigned to a replaying step forces a
re-capture, so nothing is recorded into the log the old graph points into.  UTT-Fusion ("mosi" YAML model) at B = 4,
6 steps; every log stays referenced for the whole test.  And ``FusedMMIMDbStep`` honours ``TSPM_NO_GRAPH``."""
import pytest
import torch

import tspm_amd
from oracle import mmimdb_ref as mm_orc
from oracle import mosi_ref as orc
from test_mmimdb_cpu import dropin
from tspm_amd import mmimdb as MM
from tspm_amd import mosi as M
from tspm_amd.metrics import ClassificationLog
from tspm_amd.mosi_data import PATTERNS

pytestmark = pytest.mark.gpu
B, STEPS = 4, 6


def _model_and_batch(gpu):
    torch.manual_seed(11)
    model = M.build_utt_fusion("mosi").to(gpu)
    g = torch.Generator().manual_seed(12)
    cfg = orc.MOSI
    batch = (torch.randn(B, STEPS, cfg.audio_dim, generator=g), 0.5 * torch.randn(B, STEPS, cfg.video_dim, generator=g),
             0.3 * torch.randn(B, STEPS, cfg.text_dim, generator=g), torch.randint(0, 3, (B,), generator=g))
    return model, [t.to(gpu) for t in batch]


def _log(gpu, groups=PATTERNS):
    return ClassificationLog(gpu, groups=groups, classes=3, capacity=16)


def _state(log):
    torch.cuda.synchronize()
    return [t.clone() for t in (log.conf, log.loss_log, log.counters)]


def _replace_log_on_a_replaying_step(st, batch, log1, log2, entries=1):
    """Three steps into ``log1`` (eager, capture, replay), then ``log2`` assigned without touching ``st.graph`` and one
    more step: ``log1`` must stay bit-for-bit as it was, and the graph must be a new object."""
    assert st.log is log1
    for _ in range(3):
        st.step(*batch)
    graph, before = st.graph, _state(log1)
    assert graph is not None and before[2].tolist()[0] == 3 * entries
    st.log = log2
    st.step(*batch)
    for was, now in zip(before, _state(log1)):
        assert torch.equal(was, now)
    assert st.graph is not None and st.graph is not graph and st.calls == 4
    return graph  # kept alive by the caller: its address is not reused for the new graph


@pytest.mark.parametrize("patterns", [None, ("atv", "a")], ids=["FusedMosiEvalStep", "FusedMosiPatternEvalStep"])
def test_eval_step_records_into_the_log_assigned_after_capture(gpu, patterns):
    model, batch = _model_and_batch(gpu)
    P = 1 if patterns is None else len(patterns)
    order2 = PATTERNS if patterns is None else tuple(reversed(PATTERNS))  # pattern step: the group order changes too
    log1, log2, log3 = _log(gpu), _log(gpu, order2), _log(gpu, order2)

    def build(log):
        if patterns is None:
            return M.FusedMosiEvalStep(model, None, B, STEPS, log)
        return M.FusedMosiPatternEvalStep(model, None, B, STEPS, log, patterns=patterns)
    st = build(log1)
    old = _replace_log_on_a_replaying_step(st, batch, log1, log2, P)
    assert log2.counters.tolist() == [P, P * B]  # exactly one recorded batch (P loss entries, P*B samples)
    # eval mode: the same launches on the same inputs, no float atomics -> a fresh step writes the same bits
    build(log3).step(*batch)
    torch.cuda.synchronize()
    assert log3.counters.tolist() == [P, P * B]
    assert torch.equal(log2.conf, log3.conf) and int(log2.conf.sum()) == P * B
    assert torch.equal(log2.loss_log[:P], log3.loss_log[:P])
    if patterns is not None:
        assert st.eng.group_names == order2 and log2.conf.sum(dim=(1, 2)).nonzero().flatten().tolist() == [2, 6]
    del old


def test_train_step_records_into_the_log_assigned_after_capture(gpu):
    model, batch = _model_and_batch(gpu)
    opt = tspm_amd.FusedAdam(model.parameters(), lr=1e-3, weight_decay=1e-3)
    st = M.FusedMosiStep(model, opt, None, B, STEPS)
    log1, log2 = _log(gpu), _log(gpu)
    st.log = log1  # before the first call
    old = _replace_log_on_a_replaying_step(st, batch, log1, log2)
    assert log2.counters.tolist() == [1, B]
    assert torch.equal(log2.loss_log[:1], st.eng.loss.reshape(1))
    del old


def test_mmimdb_step_honours_no_graph_switch(gpu, monkeypatch):
    n = 4
    I, T, y = (t.to(gpu) for t in mm_orc.synthetic_batch(n, seed=8))
    keep = (torch.rand(2, n, 512, generator=torch.Generator().manual_seed(40)) >= 0.5).to(torch.uint8).to(gpu)

    def run(use_graph):
        model = dropin(0).to(gpu)
        opt = tspm_amd.FusedAdam(model.parameters(), lr=1e-5, weight_decay=1e-3)
        st = MM.FusedMMIMDbStep(model, opt, None, n, use_graph=use_graph)
        st.keep_override = keep
        for _ in range(3):
            out = st.step(I, T, y)
        torch.cuda.synchronize()
        return st, out["loss"].clone(), [v.clone() for v in model.state_dict().values()]
    monkeypatch.setenv("TSPM_NO_GRAPH", "1")
    st, loss, params = run(True)
    assert st.graph is None and st.use_graph is False and st.calls == 3
    monkeypatch.delenv("TSPM_NO_GRAPH")
    ref_st, ref_loss, ref_params = run(False)
    assert ref_st.graph is None and torch.equal(loss, ref_loss)
    assert len(params) == len(ref_params) and all(torch.equal(a, b) for a, b in zip(params, ref_params))
