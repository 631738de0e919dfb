"""The Richardson-Lucy iteration loop, once, for every route: the stencil plan's paths, the Fourier plan and the host twins.

A route hands :func:`run` a *stepper* -- ``run(it0, n, x_out, rows, ab=None)`` issues iterations ``it0 .. it0 + n - 1``
(the last one into the dense ``x_out`` when that is not ``None``; ``rows``: the (iterations, 3) scalars or ``None``) --
and a *backend* that issues the launches behind an iteration and reads scalars: :class:`DeviceBackend` (the HIP entry
points, a stream, pinned rows and events) or :class:`HostBackend` (their ``_cpu`` twins, numpy rows read directly).

Two buffer disciplines.  A stepper that ``rotates`` reads one volume and writes another (``ab = (read, written)``;
``volumes()`` names the first two, ``third()`` the one an accelerated run adds): what the launches behind the iteration
need -- x_k for the total-variation launch, p_k and x_k for the extrapolation -- is at hand without a copy.  Every other
stepper updates its working volume ``cur`` in place and copies aside: ``keep()`` returns a copy of ``cur``, ``held`` is
the volume that holds x_k and receives p_{k+1}, ``turn()`` makes ``cur`` hold p_{k+1} and ``held`` x_{k+1} and returns
the volume that holds p_{k+1} besides ``cur`` (:class:`InPlace` for dense device volumes).  ``dense_out``: whether the
stepper can write the last iterate into a dense volume that is not its working volume.

A volume is a dense (Z, Y, X) tensor or a zero-haloed ``PaddedVolume``; :func:`tri` and :func:`view` name either one.
"""

from __future__ import annotations

import ctypes

from dataclasses import dataclass

import numpy as np

from . import _lib

@dataclass
class Request:
    """The checked arguments of one run.  ``tv``: ``(tv_lambda, tv_eps)`` or ``None``; ``init``: x_0."""

    iterations: int
    eps: float
    tol: float | None
    stats: bool             # the caller gets the scalars (``tol`` sums them either way)
    tv: tuple | None
    accelerate: bool
    init: object
    out: object


def check_run(y, iterations, eps, x0, out, stats, tol, tv_lambda, tv_eps, acceleration, require) -> Request:
    """The argument checks every route shares.  ``y``: the (Z, Y, X) volume as a tensor; ``require(t, name)`` validates
    a tensor of the route (device or host, float32, contiguous); ``out``: ``None``, or the tensor to write."""
    from .deconvolve import check_acceleration, check_tv

    tv_lambda, tv_eps = check_tv(tv_lambda, tv_eps)
    accelerate = check_acceleration(acceleration, tv_lambda)
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError("iterations must be >= 0")
    if not eps > 0:
        raise ValueError("eps must be > 0")
    if tol is not None and not (tol >= 0 and np.isfinite(tol)):
        raise ValueError("tol must be a finite number >= 0")
    init = y if x0 is None else require(x0, "x0")
    if tuple(init.shape) != tuple(y.shape):
        raise ValueError(f"x0 must be {tuple(y.shape)}, got {tuple(init.shape)}")
    if out is not None:
        out = require(out, "out")
        if tuple(out.shape) != tuple(y.shape) or out.device != y.device or out.data_ptr() == y.data_ptr():
            raise ValueError(f"out must be a {tuple(y.shape)} tensor on {y.device} and must not alias y (every iteration "
                             "reads y)")
    return Request(iterations, float(eps), None if tol is None else float(tol), bool(stats),
                   (tv_lambda, tv_eps) if tv_lambda > 0 else None, accelerate, init, out)


def tri(v):
    """(pointer, row pitch, plane stride) of a volume's logical window, in elements."""
    if hasattr(v, "logical_ptr"):
        return v.logical_ptr(), v.pitch, v.plane
    return v.data_ptr(), int(v.shape[2]), int(v.shape[1]) * int(v.shape[2])


def view(v):
    """The volume's logical window as a tensor."""
    return v.view if hasattr(v, "logical_ptr") else v


def row_ptr(rows, it: int):
    """Address of row ``it`` of a backend's scalars (a float64 device tensor or numpy array), or ``None``."""
    if rows is None:
        return None
    if hasattr(rows, "data_ptr"):
        return rows.data_ptr() + 8 * rows.stride(0) * it
    return rows.ctypes.data + rows.strides[0] * it


class DeviceBackend:
    """The launches behind an iteration on a HIP device, and its scalars: float64 device rows, copied ``non_blocking``
    to pinned memory behind the iteration that sums them, one event each."""

    suffix = ""

    def __init__(self, shape, device):
        self.shape, self.device = tuple(int(v) for v in shape), device
        self.tail = (_lib.stream_ptr(device),)      # what the device entry points take after the twins' arguments

    def rows(self, n: int, cols: int):
        import torch

        return torch.zeros((n, cols), dtype=torch.float64, device=self.device)

    def workspace(self):
        import torch

        return torch.empty(_lib.call_value("lsr_rl_accel_workspace_bytes", *self.shape) // 8, dtype=torch.float64,
                           device=self.device)

    def watch(self, rows) -> None:
        import torch

        self._src = rows
        self._pinned = torch.empty(tuple(rows.shape), dtype=torch.float64).pin_memory()
        self._arrived = [torch.cuda.Event() for _ in range(len(rows))]

    def post(self, it: int) -> None:
        self._pinned[it].copy_(self._src[it], non_blocking=True)
        self._arrived[it].record()

    def read(self, i: int):
        self._arrived[i].synchronize()
        return self._pinned[i]

    def merged(self, rows, tv_rows):
        import torch

        return torch.cat((rows[:, :1], tv_rows), dim=1)

    def numpy(self, rows) -> np.ndarray:
        return rows.cpu().numpy()


class HostBackend:
    """The ``_cpu`` twins: no stream, no workspace, numpy rows that are read as they are."""

    suffix = "_cpu"

    def __init__(self, shape):
        self.shape, self.tail = tuple(int(v) for v in shape), ()

    def rows(self, n: int, cols: int):
        return np.zeros((n, cols), dtype=np.float64)

    def workspace(self):
        return None

    def watch(self, rows) -> None:
        self._src = rows

    def post(self, it: int) -> None:
        pass

    def read(self, i: int):
        return self._src[i]

    def merged(self, rows, tv_rows):
        return np.concatenate((rows[:, :1], tv_rows), axis=1)

    def numpy(self, rows) -> np.ndarray:
        return rows


class AccelState:
    """What one accelerated run keeps beside its volumes: the inner products of every iteration
    (``dots[k] = <g_k, g_{k-1}>, <g_k, g_k>``), the step lengths ``alphas[k] = a_{k+1}`` and the workspace of the dots
    launch; ``step`` issues the two launches that follow ``x_{k+1} = RL(p_k)``.  ``g`` is the caller's dense volume."""

    def __init__(self, backend, iterations: int, g):
        self.be, self.g = backend, g
        n = max(int(iterations) - 1, 1)
        self.dots, self.alphas = backend.rows(n, 2), backend.rows(n, 1)
        self.work = backend.workspace()

    def step(self, k: int, x1, p, x0) -> None:
        """``x1``, ``p``, ``x0``: the volumes of x_{k+1}, p_k and x_k; p_{k+1} is written over x_k (which is not read
        when ``k == 0``: a_1 = 0)."""
        be = self.be
        _lib.call("lsr_rl_accel_dots_f32" + be.suffix, *tri(x1), *tri(p), self.g.data_ptr(), *be.shape, int(k == 0),
                  row_ptr(self.dots, k), None if self.work is None else self.work.data_ptr(), *be.tail)
        _lib.call("lsr_rl_accel_predict_f32" + be.suffix, *tri(x1), *tri(x0), *be.shape,
                  None if k == 0 else row_ptr(self.dots, k), None if k == 0 else row_ptr(self.dots, k - 1) + 8,
                  row_ptr(self.alphas, k), *be.tail)

    def used(self, done: int) -> np.ndarray:
        """a_1 .. a_{done-1}: the step lengths the ``done`` iterations that ran started from."""
        return self.be.numpy(self.alphas[:max(int(done) - 1, 0), 0]).copy()


class InPlace:
    """The in-place discipline on a device: dense side volumes, allocated on first use and kept between calls until
    ``drop_sides()``.  The stepper sets ``cur``; ``restart()`` precedes every run."""

    rotates = False

    def __init__(self, shape, device):
        self.shape, self.device = tuple(int(v) for v in shape), device
        self._sides = {}
        self.restart()

    def side(self, key):
        import torch

        if key not in self._sides:
            self._sides[key] = torch.empty(self.shape, dtype=torch.float32, device=self.device)
        return self._sides[key]

    def drop_sides(self) -> None:
        self._sides = {}

    def restart(self) -> None:
        self._p, self._h = 0, 1

    def keep(self):
        return self.side(self._p).copy_(view(self.cur))

    @property
    def held(self):
        return self.side(self._h)

    def turn(self):
        """``b`` is free and ``c`` holds p_{k+1}: x_{k+1} is saved from ``cur`` into ``b``, p_{k+1} copied into ``cur``,
        and the two trade places."""
        b, c = self.side(self._p), self.side(self._h)
        b.copy_(view(self.cur))
        view(self.cur).copy_(c)
        self._p, self._h = self._h, self._p
        return c


@dataclass
class Outcome:
    x: object                      # the tensor that holds the estimate: ``out`` where one was given
    done: int                      # iterations that ran
    stopped: bool
    rows: object = None            # the (iterations, 3) scalars as the backend holds them
    stats: object = None           # ``deconvolve.RLStats``, when the scalars were asked for
    alphas: np.ndarray | None = None


def run(req: Request, begin, events=None) -> Outcome:
    """Run ``req``.  ``begin()`` -- not called for zero iterations -- loads x_0 into the route's working volume and
    returns ``(stepper, backend, u0, g)``: ``u0`` is x_0 where the caller left it (y, dense or padded, or an ``x0``
    that the run does not write), or ``None`` when the launches behind iteration 0 must take it from the working
    volume; ``g()`` is the dense volume an accelerated run keeps g_k in.  ``events``: ``(start, end)`` recorded right
    around the launches.

    Plain run without ``tol``: one ``stepper.run`` for all iterations.  Otherwise one iteration per call: RL-TV follows
    each with the total-variation launch (``u`` = the estimate the iteration read, ``v`` = the one it wrote, in place --
    the last one into ``out`` where the stepper can, without ``tol``), an accelerated run each but the last with the two
    launches of ``csrc/rl_accel.hip``.  ``tol``: iteration i's scalars (the TV launch's with RL-TV) are looked at after
    iteration i + 1 has been queued, so nothing waits for the host, and once more after the loop: the estimate returned
    is the one iteration past the first that met ``tol``."""
    from .deconvolve import RLStats

    n, tol, out = req.iterations, req.tol, req.out
    want = req.stats or tol is not None
    if n == 0:
        return Outcome(req.init.clone() if out is None else out.copy_(req.init), 0, False,
                       stats=RLStats.from_array(np.zeros((0, 3)), 0) if want else None,
                       alphas=np.zeros(0) if req.accelerate else None)
    step, be, u0, g = begin()
    rows = be.rows(n, 3) if want else None
    tv_rows = be.rows(n, 2) if want and req.tv else None
    if events:
        events[0].record()
    done, stopped, acc = n, False, None
    if tol is None and not req.tv and not req.accelerate:
        step.run(0, n, out if step.dense_out else None, rows)
        x = out if step.dense_out else view(step.volumes()[n & 1] if step.rotates else step.cur)
    else:
        if tol is not None:
            tested, col = (tv_rows, 0) if req.tv else (rows, 1)
            be.watch(tested)

        def met(i):
            change, total = (float(v) for v in be.read(i)[col:col + 2])
            return total > 0 and change <= tol * total or total == 0

        if req.accelerate:
            acc = AccelState(be, n, g())
        if step.rotates:
            rd, wr = step.volumes()
            hold = step.third() if req.accelerate else None
        for it in range(n):
            last = it + 1 == n
            to_out = out if (last and tol is None and step.dense_out) else None
            if it == 0 and u0 is not None:
                before = u0
            elif step.rotates:
                before = rd
            elif req.tv or req.accelerate:
                before = step.turn() if (req.accelerate and it > 0) else step.keep()
            step.run(it, 1, None if req.tv else to_out, rows, ab=(rd, wr) if step.rotates else None)
            new = wr if step.rotates else step.cur
            target = new if to_out is None else to_out
            x = view(target)
            if req.tv:
                _lib.call("lsr_rl_tv_scale_f32" + be.suffix, *tri(before), *tri(new), *tri(target), *be.shape,
                          ctypes.c_float(req.tv[0]), ctypes.c_float(req.tv[1]), row_ptr(tv_rows, it), *be.tail)
            if req.accelerate and not last:
                acc.step(it, new, before, hold if step.rotates else step.held)
                if step.rotates:
                    rd, wr, hold = hold, rd, wr
            elif step.rotates:
                rd, wr = wr, rd
            done = it + 1
            if tol is not None:
                be.post(it)
                if it >= 1 and met(it - 1):
                    stopped = True
                    break
        if tol is not None and not stopped:
            stopped = bool(met(done - 1))
    if out is not None and x is not out:
        x = out.copy_(x)
    if events:
        events[1].record()
    if tv_rows is not None:      # flux from the RL launch, change and total from the TV launch
        rows = be.merged(rows, tv_rows)
    return Outcome(x, done, stopped, rows, RLStats.from_array(be.numpy(rows), done, stopped) if want else None,
                   acc.used(done) if acc else None)
