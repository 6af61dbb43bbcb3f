"""The timing protocol of the tools/time_*.py scripts, once (tools/README.md).

    timed(fn, reps)         device events around `reps` back-to-back calls of fn -> microseconds per call
    alternate(calls, reps)  warm-up rounds of all calls, then `windows` (7) windows, each timing every call once in list order
                            -> (median per call, the raw windows)
    windows_of, min_max     the tail of a record: the windows rounded, the spread of one call's windows
    select_build()          which build is timed: `--root DIR` (another checkout) or AB_LIB=<another libmpcg_hip.so>

Nothing of mpcgpu_amd is imported here before select_build() has chosen it, and nothing touches the GPU before timed() runs."""
import os
import statistics
import sys
import time

import torch


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # microseconds per call


def alternate(calls, reps, windows=7, reset=None, warmup_s=0.05, warmup_rounds=None, timer=timed):
    """Medians of `windows` windows per call and the raw windows (one row per window, one column per call); the windows alternate between the calls.
    reset: a callable, or a list of them parallel to `calls` (None: nothing), run in front of every window and of every warm-up call, outside the timed
    region, with a synchronise behind it.  The warm-up is `warmup_rounds` rounds of every call in turn if given, `warmup_s` seconds of them otherwise,
    a synchronise behind each round; no call is timed in it."""
    resets = list(reset) if isinstance(reset, (list, tuple)) else [reset] * len(calls)

    def prepare(r):
        if r is not None:
            r()
            torch.cuda.synchronize()

    t0, done = time.perf_counter(), 0
    while (done < warmup_rounds) if warmup_rounds is not None else (time.perf_counter() - t0 < warmup_s):
        for r, call in zip(resets, calls):
            prepare(r)
            call()
        torch.cuda.synchronize()
        done += 1
    rounds = []
    for _ in range(windows):
        row = []
        for r, call in zip(resets, calls):
            prepare(r)
            row.append(timer(call, reps))
        rounds.append(row)
    return [statistics.median(w[i] for w in rounds) for i in range(len(calls))], rounds


def windows_of(rounds):
    return [[round(v, 2) for v in w] for w in rounds]


def min_max(rounds, col):
    """The spread of call `col` over its windows: what a comparison between two builds has as its margin."""
    return min(w[col] for w in rounds), max(w[col] for w in rounds)


def select_build():
    """Call before anything of mpcgpu_amd is imported.  Takes `--root DIR` out of sys.argv and puts DIR (default: this checkout) in front of sys.path,
    so that DIR/mpcgpu_amd and its library are the ones timed; with AB_LIB=<.so> in the environment that package loads this library instead of its
    own.  Returns the root."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if "--root" in sys.argv:
        i = sys.argv.index("--root")
        root = os.path.abspath(sys.argv[i + 1])
        del sys.argv[i:i + 2]
    sys.path.insert(0, root)
    if os.environ.get("AB_LIB"):
        from mpcgpu_amd import _lib
        _lib.LIB_PATH = os.environ["AB_LIB"]
    return root
