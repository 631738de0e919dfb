"""The native-call sequence of Richardson-Lucy runs, route by route and mode by mode: every ``_lib.call`` with its entry
name, its sizes and scalars as they are, and every pointer as ``p<allocation>+<byte offset>`` -- the allocation numbered
by its first appearance in the run, so that buffer roles and rotation order are pinned and addresses are not.

    python -m oracle.record_rl_launch_sequences [--device cuda:0]      # rewrites tests/golden/rl_launch_sequences.json

``tests/test_rl_launch_sequence.py`` replays the same runs (``device_runs`` / ``host_runs`` below) on the code under test
and compares; the fixture is recorded on the commit whose launch sequence is to be kept.  Without ``--device`` only the
host part is rewritten.

An integer argument is a pointer when it falls inside an allocation the run can touch: the tensors and numpy arrays that
are reachable -- through lists, tuples, dicts and this package's own objects -- from the local variables of the frames
between the recorded call and the run's caller (the plan and its scratch, the run's own scalars and side volumes, ``y``,
``x0`` and ``out``).  Every allocation seen is kept alive until the run ends, so no address names two of them.  Any other
integer is a size; one beyond 2^31 would be a pointer that was missed and fails the recording.
"""

from __future__ import annotations

import argparse
import ctypes
import json
import sys

from pathlib import Path

import numpy as np
import torch

from shrimpy_amd import _lib

FIXTURE = Path(__file__).resolve().parent.parent / "tests" / "golden" / "rl_launch_sequences.json"
SHAPE = (12, 35, 133)
ITERATIONS = 4
MODES = {"plain": {}, "stats": dict(stats=True), "tol": dict(tol=0.0), "tv": dict(tv_lambda=0.01),
         "tv tol": dict(tv_lambda=0.01, tol=0.0), "accel": dict(acceleration="biggs-andrews"),
         "accel tol": dict(acceleration="biggs-andrews", tol=0.0)}


class Recorder:
    """Stands in for ``_lib.call`` during one run."""

    def __init__(self, real, stop_at):
        self.real, self.stop_at = real, stop_at
        self.calls, self.spans, self.order = [], {}, []     # spans: base address -> (bytes, the object, kept alive)

    def _see(self, obj, seen):
        if id(obj) in seen:
            return
        seen.add(id(obj))
        if isinstance(obj, torch.Tensor):
            store = obj.untyped_storage()
            if store.nbytes():
                self.spans.setdefault(store.data_ptr(), (store.nbytes(), obj))
        elif isinstance(obj, np.ndarray):
            while isinstance(obj.base, np.ndarray):
                obj = obj.base
            if obj.nbytes:
                self.spans.setdefault(obj.ctypes.data, (obj.nbytes, obj))
        elif isinstance(obj, (list, tuple)):
            for v in obj:
                self._see(v, seen)
        elif isinstance(obj, dict):
            for v in obj.values():
                self._see(v, seen)
        elif type(obj).__module__.startswith("shrimpy_amd") and hasattr(obj, "__dict__"):
            self._see(vars(obj), seen)

    def _arg(self, v):
        if v is None:
            return "-"
        if isinstance(v, ctypes.c_float):
            return f"f{v.value!r}"
        if isinstance(v, ctypes.Array):
            return f"array{len(v)}"
        v = int(v)
        for base, (nbytes, _) in self.spans.items():
            if base <= v < base + nbytes:
                if base not in self.order:
                    self.order.append(base)
                return f"p{self.order.index(base)}+{v - base}"
        assert abs(v) < 1 << 31, f"an argument of {v:#x} lies in no allocation the run is known to touch"
        return v

    def __call__(self, name, *args):
        frame, seen = sys._getframe(1), set()
        while frame is not None and frame.f_code is not self.stop_at:
            self._see(frame.f_locals, seen)
            frame = frame.f_back
        if name != "lsr_set_host_threads":      # (its argument is the machine's thread count)
            self.calls.append(" ".join([name] + [str(self._arg(a)) for a in args]))
        return self.real(name, *args)


def record(run) -> list:
    """The calls of ``run()``, one string each: the entry name and its arguments (``-`` for a null pointer)."""
    real = _lib.call
    rec = Recorder(real, record.__code__)
    _lib.call = rec
    try:
        run()
    finally:
        _lib.call = real
    return rec.calls


def device_runs(device):
    """``(name, run)`` for the eight plan kinds of ``tests/test_rl_tv_gpu.py``, every mode and every start."""
    from tests import test_rl_tv_gpu as tvg

    y, x0 = tvg._volumes(SHAPE, device)
    for kind in tvg.KINDS:
        plan = tvg.make_kind(kind, SHAPE, device)
        starts = {"y": lambda: dict(y=y), "x0": lambda: dict(y=y, x0=x0)}
        if getattr(plan, "padded_input", False):
            y_pad = plan.new_padded_input()
            y_pad.view.copy_(y)
            starts["padded y"] = lambda y_pad=y_pad: dict(y=y_pad)
        starts["x0 is out"] = lambda: dict(y=y, x0=(buf := x0.clone()), out=buf)
        for mode, kw in MODES.items():
            for start, args in starts.items():
                def run(plan=plan, kw=kw, args=args):
                    plan(iterations=ITERATIONS, **args(), **kw)
                run()       # (scratch that is allocated on first use is allocated here, not in the recorded run)
                yield f"{kind} | {mode} | {start}", run
        torch.cuda.synchronize(device)


def host_runs():
    """``(name, run)`` for ``host.richardson_lucy`` with a separable and a dense PSF, every mode, from y and from x0."""
    from shrimpy_amd import host
    from tests import rl_fp64_cases as c
    from tests import test_rl_tv_gpu as tvg

    y, x0 = tvg._volumes(SHAPE, "cpu")
    psfs = {"host separable": dict(psf_factors=tvg._sep((5, 3, 5), 1)),
            "host dense": dict(psf=c.taps_nd((3, 5, 3), np.random.default_rng(4)), separable="never")}
    for route, psf in psfs.items():
        for mode, kw in MODES.items():
            kw = {("return_stats" if k == "stats" else k): v for k, v in kw.items()}
            for start, first in (("y", None), ("x0", x0)):
                def run(psf=psf, kw=kw, first=first):
                    host.richardson_lucy(y, iterations=ITERATIONS, x0=first, **psf, **kw)
                yield f"{route} | {mode} | {start}", run


def load(path=FIXTURE) -> dict:
    """``{run name: [call, ...]}`` of a fixture file, which holds every distinct call once (``calls``) and every run as
    indices into that list (``runs``)."""
    doc = json.loads(Path(path).read_text())
    return {name: [doc["calls"][i] for i in run] for name, run in doc["runs"].items()}


def dump(runs: dict, path) -> None:
    calls = sorted({c for run in runs.values() for c in run})
    at = {c: i for i, c in enumerate(calls)}
    rows = [json.dumps(c) for c in calls]
    names = [f"{json.dumps(k)}: {json.dumps([at[c] for c in v], separators=(',', ':'))}" for k, v in sorted(runs.items())]
    lines = ['{"calls": [', ",\n".join(", ".join(rows[i:i + 4]) for i in range(0, len(rows), 4)), '], "runs": {',
             ",\n".join(", ".join(names[i:i + 4]) for i in range(0, len(names), 4)), "}}"]
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    Path(path).write_text("\n".join(lines) + "\n")


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--device", default=None, help="also record the device runs, on this HIP device")
    ap.add_argument("--out", default=str(FIXTURE))
    args = ap.parse_args()
    runs = load() if FIXTURE.exists() else {}
    runs.update({name: record(run) for name, run in host_runs()})
    if args.device is not None:
        runs.update({name: record(run) for name, run in device_runs(torch.device(args.device))})
    dump(runs, args.out)
    print(f"{len(runs)} runs, {Path(args.out).stat().st_size} bytes -> {args.out}")


if __name__ == "__main__":
    main()
