"""CPU: the timing protocol of the tools (tools/ab_timing.py), checked on fakes — the exact sequence of warm-up calls, resets, synchronises and timed
windows that alternate() issues, for the call counts the tools use; its medians and the spread helper; select_build(); and that every tool that
imports the module compiles.  No GPU: the calls, the reset, the timer, the clock and torch.cuda.synchronize are substituted."""
import importlib.util
import os
import py_compile
import statistics
import sys
import types

import pytest

from conftest import ROOT

spec = importlib.util.spec_from_file_location("ab_timing", os.path.join(ROOT, "tools", "ab_timing.py"))
ab = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ab)

FULLY_CONVERTED = ("time_block_solve_f64", "time_clocks", "time_gravity", "time_integrator", "time_kkt_f64", "time_limits", "time_merit", "time_merit_f32",
                   "time_simulate", "time_simulate_f64", "time_xuref", "time_producers", "time_sqp_iteration")
BUILD_SELECTION_ONLY = ("kkt_time", "lpkc_quick", "time_schur", "default_bits")


class Fakes:
    """n calls that log their name, a timer that logs ("timed", name, reps) without running the call and returns script[window][call], and
    torch.cuda.synchronize logging "sync" — all into one list."""

    def __init__(self, monkeypatch, n, windows):
        self.log = []
        self.names = [f"call{i}" for i in range(n)]
        self.calls = [lambda name=name: self.log.append(name) for name in self.names]
        self.script = [[float((w * 7 + i * 3) * 37 % 101) + 0.25 * i for i in range(n)] for w in range(windows)]       # (columns in no order)
        self.timed = 0
        monkeypatch.setattr(ab, "torch", types.SimpleNamespace(cuda=types.SimpleNamespace(synchronize=lambda: self.log.append("sync"))))

    def timer(self, call, reps):
        i = self.calls.index(call)
        self.log.append(("timed", self.names[i], reps))
        self.timed += 1
        return self.script[(self.timed - 1) // len(self.calls)][i]

    def reset(self, tag="reset"):
        return lambda: self.log.append(tag)

    def expected(self, warmup_rounds, windows, reps, resets):
        """resets: per call, the tag its reset logs, or None."""
        front = [[] if r is None else [r, "sync"] for r in resets]
        warm = sum((front[i] + [name] for i, name in enumerate(self.names)), []) + ["sync"]
        window = sum((front[i] + [("timed", name, reps)] for i, name in enumerate(self.names)), [])
        return warm * warmup_rounds + window * windows


@pytest.mark.parametrize("windows", [7, 4])
@pytest.mark.parametrize("n", [2, 3, 5])
def test_sequence_and_medians_with_a_round_count_warmup(monkeypatch, n, windows):
    f = Fakes(monkeypatch, n, windows)
    kw = {} if windows == 7 else {"windows": windows}                    # (7 is the default)
    med, rounds = ab.alternate(f.calls, 20, reset=f.reset(), warmup_rounds=3, timer=f.timer, **kw)
    assert f.log == f.expected(3, windows, 20, ["reset"] * n)
    assert rounds == f.script
    assert med == [statistics.median(w[i] for w in f.script) for i in range(n)]
    for i in range(n):
        assert ab.min_max(rounds, i) == (min(w[i] for w in f.script), max(w[i] for w in f.script))
    assert ab.windows_of(rounds) == [[round(v, 2) for v in w] for w in f.script]


@pytest.mark.parametrize("n", [2, 3, 5])
def test_sequence_with_a_seconds_warmup(monkeypatch, n):
    f = Fakes(monkeypatch, n, 7)
    ticks = iter(0.02 * k for k in range(100))                           # the start, then one look per round: 0.02, 0.04 < 0.05 <= 0.06
    monkeypatch.setattr(ab, "time", types.SimpleNamespace(perf_counter=lambda: next(ticks)))
    med, rounds = ab.alternate(f.calls, 200, reset=f.reset(), timer=f.timer)
    assert f.log == f.expected(2, 7, 200, ["reset"] * n)
    assert med == [statistics.median(w[i] for w in f.script) for i in range(n)]


def test_sequence_without_a_reset(monkeypatch):
    f = Fakes(monkeypatch, 3, 7)
    ab.alternate(f.calls, 20, warmup_rounds=2, timer=f.timer)
    assert f.log == f.expected(2, 7, 20, [None] * 3)
    assert "sync" not in f.log[-7 * 3:]                                  # nothing between two timed windows


def test_sequence_with_one_reset_per_call(monkeypatch):
    f = Fakes(monkeypatch, 2, 7)
    ab.alternate(f.calls, 1, reset=[f.reset("restore0"), f.reset("restore1")], warmup_rounds=1, timer=f.timer)
    assert f.log == f.expected(1, 7, 1, ["restore0", "restore1"])


def test_no_call_is_timed_during_warmup(monkeypatch):
    f = Fakes(monkeypatch, 2, 7)
    ab.alternate(f.calls, 20, reset=f.reset(), warmup_rounds=5, timer=f.timer)
    first = next(k for k, e in enumerate(f.log) if isinstance(e, tuple))
    assert not any(isinstance(e, str) and e.startswith("call") for e in f.log[first:])      # the timer alone runs a call from here on
    assert sum(e == "call0" for e in f.log[:first]) == 5 and f.timed == 14


def test_select_build(monkeypatch, tmp_path):
    from mpcgpu_amd import _lib
    own = _lib.LIB_PATH
    monkeypatch.setattr(_lib, "LIB_PATH", own)                           # (put back afterwards)
    monkeypatch.setattr(sys, "path", list(sys.path))
    monkeypatch.delenv("AB_LIB", raising=False)

    other = tmp_path / "other_checkout"
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(sys, "argv", ["x.py", "--root", "other_checkout", "30"])
    got = ab.select_build()                                              # (a relative DIR comes back absolute)
    assert os.path.isabs(got) and os.path.realpath(got) == os.path.realpath(other)
    assert sys.argv == ["x.py", "30"] and sys.path[0] == got and _lib.LIB_PATH == own

    monkeypatch.setattr(sys, "path", sys.path[1:])
    monkeypatch.setattr(sys, "argv", ["x.py", "30"])
    assert ab.select_build() == ROOT
    assert sys.argv == ["x.py", "30"] and sys.path[0] == ROOT and _lib.LIB_PATH == own

    monkeypatch.setenv("AB_LIB", "/somewhere/libmpcg_hip.so")
    assert ab.select_build() == ROOT
    assert sys.argv == ["x.py", "30"] and _lib.LIB_PATH == "/somewhere/libmpcg_hip.so"


@pytest.mark.parametrize("tool", ("ab_timing",) + FULLY_CONVERTED + BUILD_SELECTION_ONLY)
def test_tool_compiles(tool, tmp_path):
    py_compile.compile(os.path.join(ROOT, "tools", tool + ".py"), cfile=str(tmp_path / "out.pyc"), doraise=True)
