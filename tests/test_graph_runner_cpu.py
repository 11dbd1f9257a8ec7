"""The capture-and-replay state machine every fused step runs on (``_lib.GraphRunner``), without a GPU: torch's graph
object, the device synchronize and ``_lib.graph_capture`` are replaced by recording fakes, and a minimal step built on
the runner is driven with a counting enqueue callable.  Also the structure the runner exists for: one place in the
package that constructs a graph, one that reads ``TSPM_NO_GRAPH``."""
import contextlib
import glob
import os

import pytest
import torch

import tspm_amd
from tspm_amd import _lib as L


class _FakeGraph:
    made = []

    def __init__(self):
        self.replays = 0
        _FakeGraph.made.append(self)

    def replay(self):
        self.replays += 1


@pytest.fixture
def fakes(monkeypatch):
    """→ the record: graphs made, devices synchronized, graphs captured into (in order)."""
    rec = {"graphs": [], "syncs": [], "captures": []}
    _FakeGraph.made = rec["graphs"]

    @contextlib.contextmanager
    def capture(g):
        rec["captures"].append(g)
        yield

    monkeypatch.delenv("TSPM_NO_GRAPH", raising=False)
    monkeypatch.setattr(torch.cuda, "CUDAGraph", _FakeGraph)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda device=None: rec["syncs"].append(device))
    monkeypatch.setattr(L, "graph_capture", capture)
    return rec


class _Log:
    """Stands for a metrics log: every two compare equal, so only identity can tell them apart."""

    def __eq__(self, other):
        return isinstance(other, _Log)

    def __hash__(self):
        return 0


class _Step(L.GraphRunner):
    def __init__(self, use_graph=True):
        self._init_graph(use_graph, "dev0")
        self.log, self.mode, self.enqueued, self.fail = _Log(), ("a", "b"), 0, False

    def _enqueue(self):
        if self.fail:
            raise RuntimeError("enqueue failed")
        self.enqueued += 1

    def run(self):
        self.replay_or_enqueue(self._enqueue, (self.log, self.mode))
        self.calls += 1


def test_eager_then_capture_then_replay(fakes):
    st = _Step()
    assert st.use_graph is True
    st.run()  # 1: eager, no graph
    assert (st.enqueued, st.calls, st.graph) == (1, 1, None) and not fakes["graphs"] and not fakes["syncs"]
    st.run()  # 2: one capture (the step's device synchronized first, the enqueue inside the capture), one replay
    g = st.graph
    assert fakes["graphs"] == [g] and fakes["captures"] == [g] and fakes["syncs"] == ["dev0"]
    assert (st.enqueued, st.calls, g.replays) == (2, 2, 1)
    st.run()  # 3: the same graph replayed, nothing enqueued
    assert st.graph is g and fakes["graphs"] == [g] and (st.enqueued, st.calls, g.replays) == (2, 3, 2)


def test_key_changes_recapture(fakes):
    st = _Step()
    for _ in range(3):
        st.run()
    g1, log1 = st.graph, st.log
    st.log = _Log()  # another object that compares == equal: identity is what counts
    assert st.log == log1 and st.log is not log1
    st.run()
    g2 = st.graph
    assert g2 is not g1 and fakes["captures"] == [g1, g2] and st.enqueued == 3 and (g1.replays, g2.replays) == (2, 1)
    assert st._captured_key[0] is st.log  # held by reference: its id cannot be reused under the graph
    st.run()
    assert st.graph is g2 and st.enqueued == 3
    st.mode = ("b", "a")  # a changed plain value
    st.run()
    g3 = st.graph
    assert g3 is not g2 and st.enqueued == 4 and g3.replays == 1
    st.mode = tuple(["b", "a"])  # an equal plain value in another object: no re-capture
    st.run()
    assert st.graph is g3 and st.enqueued == 4 and st.calls == 7


def test_graph_none_recaptures(fakes):
    st = _Step()
    for _ in range(3):
        st.run()
    g1 = st.graph
    st.graph = None
    st.run()
    assert st.graph is not None and st.graph is not g1 and len(fakes["graphs"]) == 2 and st.enqueued == 3
    assert st.capture_graph(st._enqueue) is fakes["graphs"][-1] and st.enqueued == 4  # the primitive alone


@pytest.mark.parametrize("off", ["argument", "environment"])
def test_graphs_off_never_creates_a_graph(fakes, monkeypatch, off):
    if off == "environment":
        monkeypatch.setenv("TSPM_NO_GRAPH", "1")
    st = _Step(use_graph=off != "argument")
    assert st.use_graph is False
    for _ in range(4):
        st.run()
    assert (st.enqueued, st.calls, st.graph) == (4, 4, None) and not fakes["graphs"] and not fakes["captures"]


def test_failing_enqueue_leaves_calls_and_graph(fakes):
    st = _Step()
    st.fail = True
    with pytest.raises(RuntimeError):
        st.run()  # eager
    assert (st.calls, st.graph) == (0, None)
    st.fail = False
    for _ in range(3):
        st.run()
    g, key = st.graph, st._captured_key
    st.fail, st.log = True, _Log()  # a re-capture is due, and its enqueue raises
    with pytest.raises(RuntimeError):
        st.run()
    assert st.calls == 3 and st.graph is g and st._captured_key is key and g.replays == 2
    st.fail = False
    st.run()  # the key still differs: captured now
    assert st.calls == 4 and st.graph is not g and st._captured_key[0] is st.log


def test_one_graph_constructor_and_one_switch_in_the_package():
    src = ""
    for path in glob.glob(os.path.join(os.path.dirname(tspm_amd._lib.__file__), "*.py")):
        with open(path) as f:
            src += f.read()
    assert src.count("torch.cuda.CUDAGraph(") == 1
    assert src.count('"TSPM_NO_GRAPH"') == 1  # the one read; docstrings name the switch without the quotes
    assert "_graph_log" not in src and "_graph_gen_keep" not in src
