"""``deskew`` / ``register`` / ``deconvolve`` / ``reconstruct`` command line (click), YAML-configured.

The north-star keeps "the existing deskew/register/deconvolve CLI + YAML-config surface" of the
CPU path (biahub's; the reference's own CLI has only ``acquire`` and ``gui``,
``shrimpy/cli/main.py:31-33``).  Idiom follows the reference: a click group with ``-h/--help``
(``shrimpy/cli/main.py:21-33``), strictly validated YAML settings (``shrimpy/config.py:82-162``).

    python -m shrimpy_amd.cli deskew      -i raw.zarr -c deskew.yml      -o deskewed.zarr
    python -m shrimpy_amd.cli register    -i in.zarr  -c register.yml    -o registered.zarr
    python -m shrimpy_amd.cli deconvolve  -i in.zarr  -c deconvolve.yml  -o deconvolved.zarr
    python -m shrimpy_amd.cli reconstruct -i raw.zarr -c recon.yml       -o recon.zarr
    python -m shrimpy_amd.cli estimate-registration -s moving.zarr -t target.zarr -o register.yml
    python -m shrimpy_amd.cli characterize-psf -i beads.zarr -c psf.yml -o psf.zarr
    python -m shrimpy_amd.cli phase       -i deskewed.zarr -c phase.yml  -o phase.zarr
    python -m shrimpy_amd.cli estimate-stabilization -i series.zarr -c estimate.yml -o stabilization/
    python -m shrimpy_amd.cli stabilize   -i series.zarr -c stabilization/ -o stabilized.zarr
    python -m shrimpy_amd.cli pyramid     -i store.zarr --levels 4        (adds levels to the store in place)
    python -m shrimpy_amd.cli estimate-stitch -i tiles.zarr -c estimate.yml -o stitch.yml
    python -m shrimpy_amd.cli stitch      -i tiles.zarr -c stitch.yml    -o stitched.zarr
    python -m shrimpy_amd.cli subtract-background -i store.zarr -c background.yml -o flat.zarr
    python -m shrimpy_amd.cli despeckle   -i store.zarr -c despeckle.yml -o clean.zarr
    python -m shrimpy_amd.cli enhance     -i store.zarr -c enhance.yml   -o tubes.zarr
    python -m shrimpy_amd.cli segment     -i store.zarr -c segment.yml   -o labels.zarr
    python -m shrimpy_amd.cli track       -i labels.zarr -c track.yml    -o tracks.zarr
    python -m shrimpy_amd.cli measure     -l tracks.zarr -i store.zarr -c measure.yml -o measurements/
    python -m shrimpy_amd.cli colocalize  -i store.zarr [-l labels.zarr] -c colocalize.yml -o colocalization/

``measure`` reads two stores and writes tables only: per position ``measurements.csv``, one row per timepoint and label (or
track id) with its volume and, per channel of the intensity store, the sum, mean, standard deviation, extremes and weighted
centroid -- on request beside the mean of a ring of local background around each object.  ``colocalize`` relates pairs of
channels: per position ``colocalization_summary.csv`` (Pearson, Manders, overlap coefficients of the whole volume, with fixed or
Costes' automatic thresholds) and, with a label store, ``colocalization.csv`` with the same per object.

Every (position, timepoint, channel) volume is an independent unit.  Launched under
``python -m torch.distributed.run --nproc-per-node N`` each rank takes the units
``rank, rank + N, ...`` on GPU ``LOCAL_RANK`` and writes its own chunks: no data-path collective.
"""

from __future__ import annotations

import contextlib
import functools
import logging
import os
import time

from dataclasses import dataclass
from pathlib import Path
from typing import Callable

import click
import numpy as np

from .settings import (
    BackgroundSettings,
    DeconvolveSettings,
    DeskewSettings,
    DespeckleSettings,
    EnhanceSettings,
    ReconstructSettings,
    RegisterSettings,
)

logger = logging.getLogger("shrimpy_amd")
# RCCL between the ranks of a node needs dmabuf IPC on hosts whose driver supports nothing else (otherwise
# hipIpcGetMemHandle: invalid argument).  The HSA runtime reads this when the first HIP call initialises it, i.e. before
# anything below can run -- so it is set when the CLI module is imported, and only if the caller has not decided.
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
CONTEXT = {"help_option_names": ["-h", "--help"]}


class _EatAllCommand(click.Command):
    """A command whose ``eat_all`` options take every following argument up to the next option -- what biahub's ``-i``
    does ([RECALLED] ``OptionEatAll``), so that a shell glob works: ``-i plate.zarr/*/*/*`` expands to one path per
    position directory.  Done with click's public surface only (the earlier version patched the parser's
    private tables): ``parse_args`` rewrites ``-i a b c`` into ``-i a -i b -i c`` before click sees it, and the options
    are ordinary ``multiple=True`` ones.  An argument that starts with ``-`` ends the list (a directory named ``-x`` has
    to be written ``./-x``)."""

    eat_all: tuple = ()

    def parse_args(self, ctx, args):
        out, i = [], 0
        args = list(args)
        while i < len(args):
            a = args[i]
            out.append(a)
            i += 1
            if a == "--":                       # everything behind it is positional
                out.extend(args[i:])
                break
            if a in self.eat_all:
                first = True
                while i < len(args) and not (args[i].startswith("-") and len(args[i]) > 1):
                    if not first:
                        out.append(a)
                    out.append(args[i])
                    first = False
                    i += 1
        return super().parse_args(ctx, out)


def _eat_all_command(*names):
    """``cls=`` for ``@cli.command``: an :class:`_EatAllCommand` whose options ``names`` eat every following argument."""
    return type("_EatAllCommand_" + "_".join(n.strip("-").replace("-", "_") for n in names), (_EatAllCommand,), {"eat_all": tuple(names)})


def resolve_inputs(paths) -> tuple[Path, tuple[str, ...]]:
    """``(store root, position keys)`` of what ``-i`` was given: ONE store (an HCS plate or a single FOV: every
    position, keys ``()``) or N position directories ``<plate>/<row>/<col>/<fov>`` of one plate (the expansion of
    ``plate.zarr/*/*/*``), grouped by their common plate root."""
    from .io.omezarr import _detect

    paths = [Path(p) for p in ((paths,) if isinstance(paths, (str, os.PathLike)) else paths)]
    if not paths:
        raise click.ClickException("-i needs at least one path")
    for p in paths:
        if not p.exists():
            raise click.ClickException(f"-i: {p} does not exist")
    if len(paths) == 1:
        p = paths[0]
        try:
            _, layout = _detect(p)
        except (FileNotFoundError, ValueError) as exc:
            raise click.ClickException(f"-i: {exc}") from exc
        if layout == "fov" and len(p.resolve().parents) >= 3:
            try:   # a position directory of a plate: process that position of the plate (its key is the plate's)
                root = p.resolve().parents[2]
                if _detect(root)[1] == "hcs":
                    return root, ("/".join(p.resolve().parts[-3:]),)
            except (FileNotFoundError, ValueError):
                pass
        return p, ()
    roots, keys = set(), []
    for p in paths:
        r = p.resolve()
        if len(r.parents) < 3:
            raise click.ClickException(f"-i: {p} is not a <plate>/<row>/<col>/<fov> position directory")
        roots.add(r.parents[2])
        keys.append("/".join(r.parts[-3:]))
    if len(roots) != 1:
        raise click.ClickException(f"-i: the position directories belong to {len(roots)} different plates "
                                   f"({sorted(str(r) for r in roots)}); run them one plate at a time")
    root = roots.pop()
    try:
        if _detect(root)[1] != "hcs":
            raise ValueError(f"{root} is not an HCS plate")
    except (FileNotFoundError, ValueError) as exc:
        raise click.ClickException(f"-i: several paths must be position directories of one plate: {exc}") from exc
    if len(set(keys)) != len(keys):
        raise click.ClickException("-i: a position directory is listed twice")
    return root, tuple(keys)


def _common(fn, input_required: bool = True, config_directory: bool = False):
    fn = click.option("-i", "--input-position-dirpaths", "input_path", required=input_required, multiple=True,
                      type=click.UNPROCESSED,
                      help="Input OME-Zarr store (HCS plate or single FOV), or the position directories of one plate "
                           "(a glob such as plate.zarr/*/*/*).")(fn)
    fn = click.option("-c", "--config-filepath", "config", required=True,
                      type=click.Path(exists=True, dir_okay=config_directory, path_type=Path),
                      help="YAML settings file.")(fn)
    fn = click.option("-o", "--output-dirpath", "output_path", required=True,
                      type=click.Path(path_type=Path),
                      help="Output OME-Zarr store (must not exist, unless --resume).")(fn)
    fn = click.option("-p", "--position", "positions", multiple=True,
                      help='Restrict to these position keys ("row/col/fov"); repeatable.')(fn)
    fn = click.option("--zarr-version", type=click.Choice(["0.4", "0.5"]), default="0.5", show_default=True,
                      help="NGFF version of the output store (0.5 = Zarr v3, what the reference writes: "
                           "shrimpy/dynatrack/tracking.py:1337-1343).")(fn)
    fn = click.option("--resume", is_flag=True,
                      help="Continue an interrupted run: units already completed in the output store "
                           "(same input and settings) are skipped, unfinished ones are rewritten.")(fn)
    fn = click.option("--io", "io_backend", type=click.Choice(["auto", "native", "iohub"]), default="auto",
                      show_default=True,
                      help="Store access: this package's reader/writer, iohub, or native with iohub as the "
                           "fallback for codecs it does not implement.")(fn)
    fn = click.option("--compression", type=click.Choice(["none", "gzip", "zstd", "blosc-zstd"]),
                      default="blosc-zstd", show_default=True,
                      help="Chunk compression of the output (native writer); blosc-zstd is what the acquisition engine "
                           "writes (shrimpy/mantis/mantis_engine.py:474-481), none is the fastest.")(fn)
    fn = click.option("--on-error", "on_error", type=click.Choice(["raise", "skip"]), default="raise", show_default=True,
                      help="skip: a unit whose chunks do not read, whose kernels fail or whose result cannot be written is "
                           "left out and recorded under <output>/.lsr_failed/ (every other unit is written; the command "
                           "exits with status 3 and --resume retries only the failed units) -- the reference likewise "
                           "turns a failed stack into an error record and carries on (shrimpy/dynatrack/worker.py:262-271).")(fn)
    fn = click.option("--levels", type=click.IntRange(1, 8), default=1, show_default=True,
                      help="Multiscale levels per position: arrays \"0\" .. \"N-1\", each the 2x mean of the one above it, "
                           "computed on the device beside the result (1: level \"0\" only).")(fn)
    fn = click.option("--level-factor-z", "level_factor_z", type=click.Choice(["1", "2"]), default="2", show_default=True,
                      help="z factor between pyramid levels (y and x are always 2); 1 for stacks already coarse in z.")(fn)
    return fn


def _pyramid_options(levels, level_factor_z) -> dict:
    """``--levels`` / ``--level-factor-z`` as ``run_store`` keywords; nothing at all for the default of one level (the z
    factor has no meaning then), so that such a run is the call it always was."""
    return {} if int(levels) == 1 else {"levels": int(levels), "level_factor_z": int(level_factor_z)}


def _finish(result: dict) -> None:
    """Print a command's result; exit with status 3 when units were skipped (``--on-error skip``)."""
    click.echo(result)
    failed = result.get("failed") or []
    if failed:
        for f in failed:
            click.echo(f"FAILED {f['position']} t={f['t']} c={f['c']} [{f['stage']}]: {f['error']}", err=True)
        raise SystemExit(3)


def _inputs(input_path, positions):
    """The store and position selection of a command: ``-i`` (one store or N position directories) and ``-p``."""
    root, keys = resolve_inputs(input_path)
    if keys and positions:
        missing = [p for p in positions if p not in keys]
        if missing:
            raise click.ClickException(f"-p {missing}: not among the position directories given to -i")
        keys = tuple(k for k in keys if k in positions)
    return root, tuple(keys) or tuple(positions)


def _distributed():
    """(rank, world, device, created): ranks from the torchrun environment; the process group is
    initialised here for N > 1 (``created`` tells the caller to destroy it again)."""
    import torch

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        # the reference's own rule (shrimpy/preprocessing.py:78-82): no GPU visible -> cpu.  The volumes then
        # run the native host twins (shrimpy_amd/host.py); ranks, if any, meet over gloo.
        created = False
        if world > 1:
            import torch.distributed as dist

            if not dist.is_initialized():
                dist.init_process_group(os.environ.get("LSR_DIST_BACKEND") or "gloo")
                created = True
        return rank, world, torch.device("cpu"), created
    n_dev = torch.cuda.device_count()
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    torch.cuda.set_device(local % n_dev)
    device = torch.device("cuda", local % n_dev)
    created = False
    if world > 1:
        import torch.distributed as dist

        if not dist.is_initialized():
            # one rank per GPU: RCCL.  More ranks than GPUs on the node (ranks share a card, e.g. a
            # rehearsal on a one-GPU box): RCCL refuses duplicate devices, gloo carries the barrier
            # and the timing reduction instead -- the data path has no collective either way.
            backend = os.environ.get("LSR_DIST_BACKEND") or ("nccl" if local_world <= n_dev else "gloo")
            if backend == "nccl":
                dist.init_process_group("nccl", device_id=device)
            else:
                dist.init_process_group(backend)
            created = True
    return rank, world, device, created


def _agree(error: str | None) -> None:
    """Every rank learns whether rank 0's set-up step failed, and all of them stop together --
    a bare barrier would leave the others waiting for the collective timeout."""
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        box = [error]
        dist.broadcast_object_list(box, src=0)
        error = box[0]
    if error:
        raise click.ClickException(error)


def _open_source(path: Path, io_backend: str):
    """``(store, {key: position})`` of the input, through the native reader or iohub.

    ``auto`` = native first (it reads chunks straight into pinned staging slots); when an array uses
    a codec it does not implement and iohub is importable, the whole store is reopened with iohub."""
    from .io.omezarr import UnsupportedCodec, open_ome_zarr

    def positions_of(store):
        return dict(store.positions()) if hasattr(store, "positions") else {"0/0/0": store}

    if io_backend in ("auto", "native"):
        store = open_ome_zarr(path, layout="auto", mode="r", prefer_iohub=False)
        pos = positions_of(store)
        try:
            for p in pos.values():
                p["0"]          # parses the array metadata: raises on an unknown codec
            return store, pos
        except UnsupportedCodec as exc:
            if io_backend == "native":
                raise click.ClickException(str(exc)) from exc
            try:
                import iohub  # noqa: F401
            except ImportError:
                raise click.ClickException(f"{exc} (iohub is not installed either)") from exc
    try:
        from iohub import open_ome_zarr as iohub_open
    except ImportError as exc:
        raise click.ClickException("--io iohub: iohub is not installed") from exc
    store = iohub_open(str(path), layout="auto", mode="r")
    return store, positions_of(store)


@contextlib.contextmanager
def _closing(store):
    """``with _closing(store):`` closes the store on the way out, if it is of a kind that has a ``close``."""
    try:
        yield store
    finally:
        close = getattr(store, "close", None)
        if close:
            close()


def _selected_keys(src_positions, positions) -> list[str]:
    """The position keys of the store that ``-p`` selects (none given: all of them), in the store's order."""
    missing = [p for p in positions if p not in src_positions]
    if missing:
        raise click.ClickException(f"positions {missing} not found; available: {list(src_positions)}")
    keys = [k for k in src_positions if not positions or k in positions]
    if not keys:
        raise click.ClickException("no positions to process")
    return keys


def _channel_plan(settings: ReconstructSettings, names: list[str], nc: int) -> list[bool]:
    """Per channel: does the registration step apply?  ``source_channel_names`` empty = every channel
    (the single-modality case); otherwise only the named ones are warped and every other channel --
    the target included -- goes through the remaining steps unwarped."""
    reg = settings.registration
    if reg is None:
        return [False] * nc
    if not reg.source_channel_names:
        if reg.target_channel_name is not None and nc > 1:
            raise click.ClickException(
                "registration names a target channel but no source_channel_names: list the channels to warp")
        return [True] * nc
    known = list(names) or [str(i) for i in range(nc)]
    wanted = list(reg.source_channel_names) + ([reg.target_channel_name] if reg.target_channel_name else [])
    missing = [n for n in wanted if n not in known]
    if missing:
        raise click.ClickException(f"channels {missing} not in the store (it has {known})")
    if reg.target_channel_name in reg.source_channel_names:
        raise click.ClickException(f"target channel {reg.target_channel_name!r} is also listed as a source")
    return [known[c] in reg.source_channel_names for c in range(nc)]


def _fingerprint(input_path: Path, settings: ReconstructSettings, shape, dtype, keys, extra=None) -> str:
    import hashlib
    import json

    doc = {"input": str(Path(input_path).resolve()), "settings": settings.model_dump(mode="json"),
           "shape": list(shape), "dtype": str(dtype), "positions": list(keys)}
    if extra is not None:     # settings of a step that is not part of ReconstructSettings (the phase command)
        doc["extra"] = extra
    return hashlib.sha256(json.dumps(doc, sort_keys=True).encode()).hexdigest()


class _DoneLedger:
    """Per-unit completion records of an output store: one small file per (position, t, c) under
    ``<store>/.lsr_done/``, written only after the unit's chunks are.

    The reference never overwrites an acquisition and appends its CSV row by row
    (``shrimpy/mantis/mantis_engine.py:458, 480``, ``shrimpy/dynatrack/tracking.py:887-914``); the
    unit of resumption here is likewise the per-(p, t, c) volume.  A record carries
    the fingerprint of (input, settings, geometry): a store written with other settings is never
    silently continued."""

    def __init__(self, store_path: Path, fingerprint: str):
        self.dir = Path(store_path) / ".lsr_done"
        self.fingerprint = fingerprint

    def _file(self, u) -> Path:
        return self.dir / u.position.replace("/", "__") / f"t{u.t}_c{u.c}"

    def check(self) -> None:
        """Refuse a store that records another run's fingerprint (writes nothing)."""
        tag = self.dir / "fingerprint"
        if tag.exists() and tag.read_text().strip() != self.fingerprint:
            raise click.ClickException(
                f"{self.dir.parent} was written from a different input or with different settings; "
                "--resume only continues the same run")

    def begin(self) -> None:
        self.dir.mkdir(parents=True, exist_ok=True)
        self.check()
        tag = self.dir / "fingerprint"
        if not tag.exists():
            tag.write_text(self.fingerprint + "\n")

    def is_done(self, u) -> bool:
        f = self._file(u)
        try:
            return f.read_text().strip() == self.fingerprint
        except FileNotFoundError:
            return False

    def mark(self, u) -> None:
        f = self._file(u)
        f.parent.mkdir(parents=True, exist_ok=True)
        tmp = f.with_name(f.name + ".tmp")
        tmp.write_text(self.fingerprint + "\n")
        os.replace(tmp, f)


class _FailLedger:
    """Units given up under ``--on-error skip``: one JSON file per (position, t, c) under ``<store>/.lsr_failed/`` with
    the stage and the message; removed again when the unit is written by a later (``--resume``) run."""

    def __init__(self, store_path: Path):
        self.dir = Path(store_path) / ".lsr_failed"

    def _file(self, u) -> Path:
        return self.dir / u.position.replace("/", "__") / f"t{u.t}_c{u.c}.json"

    def mark(self, u, stage: str, error: str) -> None:
        import json

        f = self._file(u)
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(json.dumps({"position": u.position, "t": u.t, "c": u.c, "stage": stage, "error": error}) + "\n")

    def clear(self, u) -> None:
        try:
            self._file(u).unlink()
        except FileNotFoundError:
            pass

    def listed(self) -> list[dict]:
        import json

        return [json.loads(f.read_text()) for f in sorted(self.dir.glob("*/*.json"))] if self.dir.exists() else []


def run_store(input_path: Path, output_path: Path, settings: ReconstructSettings, positions=(),
              zarr_version: str = "0.4", reconstructor_factory=None, stage_through_pinned: bool = True,
              resume: bool = False, io_backend: str = "auto", compression: str | None = None,
              device_codec: bool | None = None, on_error: str = "raise", output_channel_names=None,
              fingerprint_extra=None, levels: int = 1, level_factor_z: int = 2) -> dict:
    """Apply ``settings`` to every (position, t, c) volume of ``input_path`` -> ``output_path``.

    ``output_channel_names(names) -> names``: the output store's channel names from the input's (default: the same);
    ``fingerprint_extra``: JSON-able settings of a ``reconstructor_factory`` step, part of the ``--resume`` fingerprint.

    ``device_codec`` (default: on, ``LSR_DEVICE_CODEC=0`` turns it off): with a blosc-zstd output on a GPU the chunk
    frames are written by the device (``io/device_codec.py``) and the host stores them as they are; an input stored as
    blosc-zstd frames crosses PCIe compressed and is decoded by the device.  The decoder gives every blosc block to one
    lane, so a volume takes ~6 ms whatever its size: left to itself (``None``) the run decodes on the device only volumes of
    at least ``LSR_DEVICE_DECODE_MIN_BLOCKS`` blocks (default 8192 = 256 MB of the acquisition's 32 KB blocks; below that
    sixteen host threads are faster); ``True`` decodes on the device whatever the size.
    ``on_error="skip"``: see ``pipeline.run_sharded``; skipped units are listed in the result's ``failed`` (all ranks')
    and recorded under ``<output>/.lsr_failed/``.

    On a GPU the volumes pass through pinned staging slots and copy streams
    (``staging.VolumeStager``) so that reading, upload, kernels, download and writing overlap.

    ``reconstructor_factory(raw_shape, settings, device)`` defaults to
    :class:`shrimpy_amd.pipeline.VolumeReconstructor` (tests inject a stand-in).
    ``resume``: the output may exist; units recorded as complete (``_DoneLedger``) are skipped.

    ``levels`` > 1: every position gets the multiscale arrays ``"0" .. str(levels - 1)`` (``io.omezarr.create_pyramid``).
    The lower levels of a unit are computed from its result while that is on the device (``pyramid.build_levels``, factors
    ``(level_factor_z, 2, 2)``, on the stream of the kernels), copied to the host and encoded there, and written with the
    unit: it counts as complete only when every level is stored.  Level 0 keeps its route, device-written frames included.
    """
    from .pyramid import MAX_LEVELS

    if not 1 <= int(levels) <= MAX_LEVELS or level_factor_z not in (1, 2):
        raise click.ClickException(f"levels must be in 1 .. {MAX_LEVELS} and level_factor_z 1 or 2")
    if int(levels) > 1 and io_backend == "iohub":
        raise click.ClickException("--levels > 1 needs this package's own writer: it cannot be combined with --io iohub")
    rank, world, device, created = _distributed()
    try:
        min_blocks = 0
        if device_codec is None:
            device_codec = os.environ.get("LSR_DEVICE_CODEC", "1") != "0"
            min_blocks = int(os.environ.get("LSR_DEVICE_DECODE_MIN_BLOCKS", "8192") or 0)
        return _run_store(input_path, output_path, settings, positions, zarr_version, reconstructor_factory,
                          stage_through_pinned, resume, io_backend, compression, rank, world, device, device_codec,
                          on_error, min_blocks, output_channel_names, fingerprint_extra, int(levels), int(level_factor_z))
    finally:
        if created:
            import torch.distributed as dist

            dist.destroy_process_group()


def _run_store(input_path, output_path, settings, positions, zarr_version, reconstructor_factory,
               stage_through_pinned, resume, io_backend, compression, rank, world, device, device_codec=True,
               on_error="raise", min_decode_blocks=0, output_channel_names=None, fingerprint_extra=None, levels=1,
               level_factor_z=2) -> dict:
    import torch

    from .io.omezarr import as_volume_array, create_pyramid, open_ome_zarr, position_scale
    from .pipeline import Unit, VolumeReconstructor, enumerate_units, run_sharded

    factory = reconstructor_factory or VolumeReconstructor
    src, src_positions = _open_source(input_path, io_backend)
    use_iohub_out = io_backend == "iohub"
    keys = [k for k in src_positions if not positions or k in positions]
    missing = [p for p in positions if p not in src_positions]
    if missing:
        raise click.ClickException(f"positions {missing} not found; available: {list(src_positions)}")
    if not keys:
        raise click.ClickException("no positions to process")

    # every selected position must have the first one's geometry: checked before anything is written
    arrays = {k: as_volume_array(src_positions[k]["0"]) for k in keys}
    first = src_positions[keys[0]]
    shape5, raw_dtype = tuple(arrays[keys[0]].shape), np.dtype(arrays[keys[0]].dtype)
    if len(shape5) != 5:
        raise click.ClickException(f"position {keys[0]}: expected 5-D TCZYX data, got shape {shape5}")
    odd = {k: (tuple(a.shape), str(a.dtype)) for k, a in arrays.items()
           if tuple(a.shape) != shape5 or np.dtype(a.dtype) != raw_dtype}
    if odd:
        raise click.ClickException(f"positions differ from {keys[0]} {shape5} {raw_dtype}: {odd}; "
                                   "run them separately (-p)")
    nt, nc, nz, ny, nx = shape5
    channel_names = list(first.channel_names)
    warp = _channel_plan(settings, channel_names, nc)

    rec = factory((nz, ny, nx), settings, device)
    rec_unwarped = rec
    if settings.registration is not None and not all(warp):
        rec_unwarped = factory((nz, ny, nx), settings.model_copy(update={"registration": None}), device)
        if tuple(rec_unwarped.output_shape) != tuple(rec.output_shape):
            hint = ("keep_overhang grows the registered channels to the union box, which an unwarped channel cannot share: "
                    "warp every channel (leave source_channel_names empty) or set keep_overhang: false"
                    if settings.registration.keep_overhang else "drop output_shape_zyx or warp every channel")
            raise click.ClickException(
                f"registered channels come out as {tuple(rec.output_shape)} but the unwarped ones as "
                f"{tuple(rec_unwarped.output_shape)}: {hint}")
    oz, oy, ox = rec.output_shape
    out_scale = list(position_scale(first))
    if settings.deskew is not None:
        from .geometry import deskew_geometry, orient_voxel

        d = settings.deskew
        voxel = deskew_geometry((nz, ny, nx), d.ls_angle_deg, d.px_to_scan_ratio, d.keep_overhang,
                                d.average_n_slices, d.pixel_size_um).voxel_size
        # scale metadata as scripts/measure_psf.py:273-276
        out_scale[2:] = [float(v) for v in orient_voxel(voxel, d.orientation)]

    # where output index 0 sits in the target's physical frame: non-zero only when keep_overhang grew the grid below zero
    origin = tuple(getattr(rec, "register_origin", (0, 0, 0)))
    out_translation = [0.0, 0.0] + [float(o) * float(sc) for o, sc in zip(origin, out_scale[2:])] if any(origin) else None
    if levels > 1:     # (a run without a pyramid keeps the fingerprint it always had)
        fingerprint_extra = {"step": fingerprint_extra, "pyramid": {"levels": levels, "fz": level_factor_z}}
    ledger = _DoneLedger(output_path, _fingerprint(input_path, settings, shape5, raw_dtype, keys, fingerprint_extra))
    if output_channel_names is not None:
        channel_names = list(output_channel_names(channel_names or [str(c) for c in range(nc)]))
    fail_ledger = _FailLedger(output_path)
    out_shape5 = (nt, nc, oz, oy, ox)
    from .pyramid import build_levels, level_shapes

    level_shapes5 = [(nt, nc) + tuple(s) for s in level_shapes((oz, oy, ox), levels, level_factor_z)[0]]

    def open_output(mode):
        if use_iohub_out:
            from iohub import open_ome_zarr as iohub_open

            kw = dict(layout="hcs", mode=mode)
            if mode == "w":
                kw.update(channel_names=channel_names, version=zarr_version)
            return iohub_open(str(output_path), **kw)
        return open_ome_zarr(output_path, layout="hcs", mode=mode, channel_names=channel_names,
                             version=zarr_version, prefer_iohub=False)

    # rank 0 creates (or, resuming, checks and completes) the output store; positions are separate
    # arrays on disk, so afterwards every rank writes its own units with no coordination
    error = None
    if rank == 0:
        try:
            exists = Path(output_path).exists() and any(Path(output_path).iterdir())
            if exists and not resume:
                raise FileExistsError(f"{output_path} exists (never overwritten, like the reference); "
                                      "use --resume to continue an interrupted run")
            if exists:
                ledger.check()       # another run's store (other settings, other --levels) is refused as that, first
            dst = open_output("a" if exists else "w")
            have = dict(dst.positions()) if exists else {}
            for key in keys:
                if key in have:
                    for k, want in enumerate(level_shapes5):
                        try:
                            got = tuple(as_volume_array(have[key][str(k)]).shape)
                        except (FileNotFoundError, KeyError) as exc:
                            raise ValueError(f"{output_path}: position {key} has no level {k}") from exc
                        if got != want:
                            raise ValueError(f"{output_path}: position {key} level {k} has shape {got}, this run writes {want}")
                    continue
                row, col, fov = key.split("/")
                pos = dst.create_position(row, col, fov)
                extra = {} if use_iohub_out or compression in (None, "none") else {"compress": compression}
                create_pyramid(pos, out_shape5, "float32", out_scale, levels, level_factor_z, translation=out_translation,
                               **extra)
            dst.close()
            ledger.begin()
        except click.ClickException as exc:
            error = exc.message
        except Exception as exc:  # noqa: BLE001 -- reported on every rank, see _agree
            error = f"{type(exc).__name__}: {exc}"
    _agree(error)
    dst = open_output("a")
    dst_positions = {k: p for k, p in dict(dst.positions()).items() if k in keys}
    dst_arrays = {k: as_volume_array(p["0"]) for k, p in dst_positions.items()}
    # the lower pyramid levels: arrays per position, and per unit in flight what `process` handed over for `store`
    lower_arrays = {k: [as_volume_array(p[str(lv)]) for lv in range(1, levels)] for k, p in dst_positions.items()}
    lower_pending: dict = {}

    units = enumerate_units(keys, nt, range(nc))
    todo = [u for u in units if not (resume and ledger.is_done(u))]
    skipped = len(units) - len(todo)
    if skipped:
        logger.info("resume: %d of %d units already complete", skipped, len(units))

    frames_in = [False]      # set below: the stager decodes the store's chunk frames on the device

    def load(u: Unit, out=None):
        if frames_in[0] and out is not None:
            return arrays[u.position].read_volume_frames(u.t, u.c, out=out)   # file reads only
        return arrays[u.position].read_volume(u.t, u.c, out=out)

    def store(u: Unit, vol):
        from .staging import EncodedVolume

        if isinstance(vol, EncodedVolume):      # chunk frames written on the device: stored as they are
            dst_arrays[u.position].write_encoded_volume(u.t, u.c, vol.frames)
        else:
            host = vol if isinstance(vol, np.ndarray) else vol.cpu().numpy()
            dst_arrays[u.position].write_volume(u.t, u.c, host)
        if levels > 1:
            hosts, ready = lower_pending.pop(u)
            if ready is not None:
                ready.synchronize()           # the copies of this unit's lower levels have landed
            for arr, lv in zip(lower_arrays[u.position], hosts):
                arr.write_volume(u.t, u.c, lv.numpy())
        ledger.mark(u)
        fail_ledger.clear(u)

    def process(data, unit: Unit):
        step = rec if warp[unit.c] else rec_unwarped
        # a step that works differently from unit to unit (stabilize: one matrix per timepoint) hands out its callable
        for_unit = getattr(step, "for_unit", None)
        result = (step if for_unit is None else for_unit(unit))(data)
        if levels > 1:
            lower_pending[unit] = lower_levels(result)
        return result

    def lower_levels(result):
        """Levels 1 .. of a unit's result, on their way to the host: (host tensors, the event behind their copies or None).
        Computed where the result lives, on the current stream -- behind the kernels that wrote it."""
        vol = torch.as_tensor(result)
        if vol.dtype != torch.float32 or not vol.is_contiguous():
            vol = vol.to(torch.float32).contiguous()
        lower = build_levels(vol, levels, level_factor_z)
        if vol.device.type != "cuda":
            return lower, None
        hosts = [torch.empty(lv.shape, dtype=lv.dtype, pin_memory=True).copy_(lv, non_blocking=True) for lv in lower]
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(vol.device))
        return hosts, ready

    stager = None
    if (stage_through_pinned and torch.device(device).type == "cuda"
            and raw_dtype in (np.dtype("uint16"), np.dtype("float32")) and len(todo) > world):
        from .staging import VolumeStager

        # a blosc-zstd output whose chunks are whole planes: the device writes the frames (None: host encoding)
        frame_bytes = None
        if device_codec and not use_iohub_out:
            sizes = {getattr(a, "encoded_frame_bytes", lambda: None)() for a in dst_arrays.values()}
            frame_bytes = sizes.pop() if len(sizes) == 1 else None
        # ... and an input stored as blosc-zstd chunk frames of whole planes is decoded on the device
        layout = None
        if device_codec and todo:
            layout = getattr(arrays[todo[0].position], "compressed_layout", lambda *a: None)(todo[0].t, todo[0].c)
            if layout is not None:
                blocks = layout["n_frames"] * -(-layout["nbytes"] // layout["blocksize"])
                if blocks < min_decode_blocks:
                    logger.info("input chunks decoded on the host: %d blosc blocks per volume, the device decoder pays from %d",
                                blocks, min_decode_blocks)
                    layout = None
        from ._lib import LsrUnsupported

        attempts = [(frame_bytes, layout)] + ([(None, layout)] if frame_bytes and layout else []) \
            + ([(frame_bytes, None)] if frame_bytes and layout else []) + ([(None, None)] if frame_bytes or layout else [])
        # slots each way: with the chunks decoded on the device a unit passes through read -> upload -> decode before the
        # kernels can start, and three slots let the reader work two units ahead of them (LSR_STAGE_DEPTH overrides)
        depth = int(os.environ.get("LSR_STAGE_DEPTH", "0") or 0)
        for fb, lay in attempts:
            try:
                stager = VolumeStager((nz, ny, nx), raw_dtype, (oz, oy, ox), device, encode_frame_bytes=fb, decode_layout=lay,
                                      depth=depth if depth >= 2 else (3 if lay is not None else 2))
                frames_in[0] = lay is not None
                break
            except LsrUnsupported as exc:                # a chunk / block size outside the device codecs' range
                logger.info("device codec not used for %s (%s)", "the output" if fb else "the input", exc)
            except (RuntimeError, MemoryError) as exc:   # not enough pinnable host memory for the slots
                logger.warning("staging slots unavailable (%s): volumes are handed over synchronously", exc)
                stager = None
                break
    try:
        on_gpu = torch.device(device).type == "cuda"
        report = run_sharded(todo, load, process, store, synchronize=torch.cuda.synchronize if on_gpu else None,
                             stager=stager, process_takes_unit=True, on_error=on_error)
    finally:
        if stager is not None:
            try:                               # (LSR_STAGE_EVENTS=1 only; never in the way of the run's own error)
                times = stager.gpu_times() if hasattr(stager, "gpu_times") else None
                if times:
                    logger.warning("GPU time per unit by HIP events: %s", times)
            except Exception as exc:  # noqa: BLE001
                logger.debug("no GPU clocks: %s", exc)
            stager.close()
        for s in (src, dst):
            close = getattr(s, "close", None)
            if close:
                close()
    failed = [{"position": u.position, "t": u.t, "c": u.c, "stage": stage, "error": msg} for u, stage, msg in report.failures]
    for u, stage, msg in report.failures:
        fail_ledger.mark(u, stage, msg)
    if world > 1:                       # every rank returns the whole job's list
        import torch.distributed as dist

        box: list = [None] * world
        dist.all_gather_object(box, failed)
        failed = [f for part in box for f in part]
    nvox = (len(report.units) - len(report.failures)) * nz * ny * nx
    logger.info("rank %d: %d units, %.3g input voxels/s (job %.2fs)", rank, len(report.units),
                nvox / max(report.seconds, 1e-9), report.max_seconds)
    return {"rank": rank, "world_size": world, "units": len(report.units), "units_total": len(units),
            "units_skipped": skipped, "failed": failed, "seconds": report.seconds, "job_seconds": report.max_seconds,
            "stage_seconds": {k: round(v, 4) for k, v in report.stage_seconds.items()},
            # median interval between consecutive units on this rank once the pipeline is full (None: fewer than 4 units)
            "steady_s_per_unit": (round(float(np.median(report.unit_intervals[1:])), 4)
                                  if len(report.unit_intervals) >= 3 else None),
            "device_codec": {"encode": bool(stager is not None and getattr(stager, "encode_frame_bytes", None)),
                             "decode": bool(frames_in[0])},
            "output_shape": (oz, oy, ox)}


@click.group(context_settings=CONTEXT)
@click.option("-v", "--verbose", is_flag=True, help="DEBUG logging.")
def cli(verbose: bool):
    """MI355X light-sheet reconstruction: deskew, affine registration, Richardson-Lucy."""
    logging.basicConfig(level=logging.DEBUG if verbose else logging.INFO,
                        format="%(asctime)s %(levelname)s %(name)s: %(message)s")


def _store_command(name: str, help: str, config_directory: bool = False):
    """Decorator of a ``run_<command>(input_path, config, output_path, positions, zarr_version, resume, io_backend,
    compression, on_error, levels=, level_factor_z=)``: registers the command ``name`` with the shared options (``_common``;
    ``config_directory``: ``-c`` may be a directory) and ``help`` as its ``-h`` text, and leaves the function as it is."""

    def register(run):
        @cli.command(name, cls=_eat_all_command("-i", "--input-position-dirpaths"), help=help)
        @functools.partial(_common, config_directory=config_directory)
        def command(input_path, config, output_path, positions, zarr_version, resume, io_backend, compression, on_error, levels,
                    level_factor_z):
            input_path, positions = _inputs(input_path, positions)
            _finish(run(input_path, config, output_path, positions, zarr_version, resume, io_backend, compression, on_error,
                        **_pyramid_options(levels, level_factor_z)))

        return run

    return register


@cli.command(cls=_eat_all_command("-i", "--input-position-dirpaths"))
@_common
def deskew(input_path, config, output_path, positions, zarr_version, resume, io_backend, compression, on_error, levels,
           level_factor_z):
    """Deskew oblique-plane stacks (config: DeskewSettings YAML)."""
    input_path, positions = _inputs(input_path, positions)
    s = ReconstructSettings(deskew=DeskewSettings.from_yaml(config))
    _finish(run_store(input_path, output_path, s, positions, zarr_version, resume=resume,
                      io_backend=io_backend, compression=compression, on_error=on_error,
                      **_pyramid_options(levels, level_factor_z)))


def _target_shape_zyx(target_path) -> tuple[int, int, int]:
    """(Z, Y, X) of the first position of the store (or position directories) ``-t`` names."""
    from .io.omezarr import as_volume_array

    root, keys = resolve_inputs(target_path)
    store, positions_of = _open_source(root, "auto")
    with _closing(store):
        for key, pos in positions_of.items():
            if not keys or key in keys:
                return tuple(int(v) for v in as_volume_array(pos["0"]).shape[-3:])
    raise click.ClickException(f"-t: no position found in {root}")


@cli.command(cls=_eat_all_command("-i", "--input-position-dirpaths", "-s", "--source-position-dirpaths", "-t", "--target-position-dirpaths"))
@click.option("-s", "--source-position-dirpaths", "source_path", multiple=True, type=click.UNPROCESSED,
              help="The MOVING store / position directories ([RECALLED] biahub's spelling; the same as -i).")
@click.option("-t", "--target-position-dirpaths", "target_path", multiple=True, type=click.UNPROCESSED,
              help="The TARGET store / position directories: its (Z, Y, X) is the output shape when the config gives "
                   "no output_shape_zyx.")
@functools.partial(_common, input_required=False)
def register(input_path, source_path, target_path, config, output_path, positions, zarr_version, resume, io_backend,
             compression, on_error, levels, level_factor_z):
    """Apply an affine registration (config: RegisterSettings YAML with affine_transform_zyx)."""
    input_path, source_path, target_path = (input_path or None), (source_path or None), (target_path or None)
    if (input_path is None) == (source_path is None):
        raise click.ClickException("name the moving store once: -i or -s")
    input_path, positions = _inputs(input_path if input_path is not None else source_path, positions)
    reg = RegisterSettings.from_yaml(config)
    if target_path is not None and reg.output_shape_zyx is None:
        reg = reg.model_copy(update={"output_shape_zyx": _target_shape_zyx(target_path)})
    s = ReconstructSettings(registration=reg)
    _finish(run_store(input_path, output_path, s, positions, zarr_version, resume=resume,
                      io_backend=io_backend, compression=compression, on_error=on_error,
                      **_pyramid_options(levels, level_factor_z)))


@cli.command(cls=_eat_all_command("-i", "--input-position-dirpaths"))
@click.option("--psf-dirpath", "psf_dirpath", default=None, type=click.Path(exists=True, path_type=Path),
              help="A measured PSF: an OME-Zarr bead volume (as scripts/measure_psf.py:273-287 writes them) or a .npy "
                   "ZYX array; overrides psf_path of the config ([RECALLED] biahub's -p, which is the position filter here).")
@_common
def deconvolve(input_path, psf_dirpath, config, output_path, positions, zarr_version, resume, io_backend, compression,
               on_error, levels, level_factor_z):
    """Richardson-Lucy deconvolution (config: DeconvolveSettings YAML)."""
    input_path, positions = _inputs(input_path, positions)
    dec = DeconvolveSettings.from_yaml(config)
    if psf_dirpath is not None:
        dec = dec.model_copy(update={"psf_path": str(psf_dirpath)})
    s = ReconstructSettings(deconvolution=dec)
    _finish(run_store(input_path, output_path, s, positions, zarr_version, resume=resume,
                      io_backend=io_backend, compression=compression, on_error=on_error,
                      **_pyramid_options(levels, level_factor_z)))


@cli.command(cls=_eat_all_command("-i", "--input-position-dirpaths"))
@_common
def reconstruct(input_path, config, output_path, positions, zarr_version, resume, io_backend, compression, on_error, levels,
                level_factor_z):
    """deskew -> register -> deconvolve in one pass (config: ReconstructSettings YAML)."""
    input_path, positions = _inputs(input_path, positions)
    s = ReconstructSettings.from_yaml(config)
    if s.deskew is None and s.registration is None and s.deconvolution is None:
        raise click.ClickException("the config enables no step")
    _finish(run_store(input_path, output_path, s, positions, zarr_version, resume=resume,
                      io_backend=io_backend, compression=compression, on_error=on_error,
                      **_pyramid_options(levels, level_factor_z)))


class _PhaseReconstructor:
    """``run_store``'s per-volume step of the ``phase`` command: one :class:`shrimpy_amd.phase.PhasePlan` for the store's
    volume shape; the volume keeps its shape."""

    def __init__(self, phase_settings, raw_shape, _settings, device):
        from .phase import PhasePlan

        self.device = device
        self.output_shape = tuple(int(n) for n in raw_shape)
        self._plan = PhasePlan(self.output_shape, phase_settings, device)
        logger.info("phase: filter for %s on grid %s ready in %.1f s", self.output_shape, self._plan.grid, self._plan.seconds)

    def __call__(self, raw):
        import torch

        return self._plan(torch.as_tensor(raw, device=self.device).to(torch.float32).contiguous())


@cli.command(cls=_eat_all_command("-i", "--input-position-dirpaths"))
@_common
def phase(input_path, config, output_path, positions, zarr_version, resume, io_backend, compression, on_error, levels,
          level_factor_z):
    """Label-free 3-D phase reconstruction of (deskewed) bright-field volumes (config: PhaseSettings YAML)."""
    from .settings import PhaseSettings

    input_path, positions = _inputs(input_path, positions)
    s = PhaseSettings.from_yaml(config)
    _finish(run_store(input_path, output_path, ReconstructSettings(), positions, zarr_version,
                      reconstructor_factory=functools.partial(_PhaseReconstructor, s), resume=resume, io_backend=io_backend,
                      compression=compression, on_error=on_error,
                      output_channel_names=lambda names: ["Phase3D"] if len(names) == 1 else [f"Phase3D_{n}" for n in names],
                      fingerprint_extra={"phase": s.model_dump(mode="json")}, **_pyramid_options(levels, level_factor_z)))


@cli.command("estimate-registration")
@click.option("-s", "--source-position-dirpaths", "source_path", required=True,
              type=click.Path(exists=True, path_type=Path), help="Store holding the MOVING volume.")
@click.option("-t", "--target-position-dirpaths", "target_path", required=True,
              type=click.Path(exists=True, path_type=Path), help="Store holding the TARGET (fixed) volume.")
@click.option("-o", "--output-filepath", "output_path", required=True, type=click.Path(dir_okay=False, path_type=Path),
              help="RegisterSettings YAML to write (affine_transform_zyx, source_channel_names).")
@click.option("--source-channel", default=None, help="Channel name in the source store (default: the first).")
@click.option("--target-channel", default=None, help="Channel name in the target store (default: the first).")
@click.option("-p", "--position", default=None, help='Position key ("row/col/fov") in both stores (default: the first).')
@click.option("--timepoint", type=int, default=0, show_default=True)
@click.option("--model", type=click.Choice(["affine", "translation"]), default="affine", show_default=True)
@click.option("--no-intensity", is_flag=True, help="Do not fit the gain / offset between the two volumes.")
@click.option("--metric", type=click.Choice(["ssd", "mi"]), default="ssd", show_default=True,
              help="ssd: squared differences under a linear intensity map; mi: mutual information, for two channels "
                   "with different contrast (phase against fluorescence).")
@click.option("--bins", type=click.IntRange(4, 64), default=32, show_default=True,
              help="Histogram bins per axis of --metric mi.")
@click.option("--io", "io_backend", type=click.Choice(["auto", "native", "iohub"]), default="auto", show_default=True)
def estimate_registration(source_path, target_path, output_path, source_channel, target_channel, position, timepoint,
                          model, no_intensity, metric, bins, io_backend):
    """Estimate the affine that maps TARGET indices to SOURCE coordinates (what `register` applies)."""
    click.echo(run_estimate(source_path, target_path, output_path, source_channel, target_channel, position, timepoint,
                            model, not no_intensity, io_backend, metric=metric, bins=bins))


def run_estimate(source_path, target_path, output_path, source_channel=None, target_channel=None, position=None,
                 timepoint: int = 0, model: str = "affine", intensity: bool = True, io_backend: str = "auto",
                 estimator=None, metric: str = "ssd", bins: int = 32) -> dict:
    """Read one volume from each store, estimate, write the ``RegisterSettings`` YAML.
    ``estimator(moving, target, model=, intensity=)`` defaults to :func:`estimate.estimate_affine_zyx`; ``metric=`` and
    ``bins=`` are handed to it only where they differ from its defaults (``"ssd"``, 32)."""
    import torch
    import yaml

    from .io.omezarr import as_volume_array

    _, _, device, created = _distributed()
    try:
        def read(path, channel):
            _, positions = _open_source(path, io_backend)
            key = position or next(iter(positions))
            if key not in positions:
                raise click.ClickException(f"position {key!r} not in {path} (it has {list(positions)})")
            pos = positions[key]
            names = list(pos.channel_names)
            if channel is None:
                c = 0
            elif channel in names:
                c = names.index(channel)
            else:
                raise click.ClickException(f"channel {channel!r} not in {path} (it has {names})")
            arr = as_volume_array(pos["0"])
            if not 0 <= timepoint < arr.shape[0]:
                raise click.ClickException(f"timepoint {timepoint} out of range for {path} (T = {arr.shape[0]})")
            vol = arr.read_volume(timepoint, c)
            return torch.as_tensor(np.ascontiguousarray(vol, dtype=np.float32), device=device), (names[c] if names else str(c))

        moving, src_name = read(source_path, source_channel)
        target, tgt_name = read(target_path, target_channel)
        if estimator is None:
            from .estimate import estimate_affine_zyx as estimator
        if metric not in ("ssd", "mi"):
            raise click.ClickException(f"metric must be ssd or mi, got {metric!r}")
        extra = {}
        if metric != "ssd":
            extra["metric"] = metric
        if int(bins) != 32:
            extra["bins"] = int(bins)
        est = estimator(moving, target, model=model, intensity=intensity, **extra)
        doc = est.to_settings_dict(source_channel_names=[src_name], output_shape_zyx=[int(n) for n in target.shape])
        if Path(source_path).resolve() == Path(target_path).resolve() and tgt_name != src_name:
            doc["target_channel_name"] = tgt_name
        RegisterSettings(**doc)   # what we write must load
        Path(output_path).parent.mkdir(parents=True, exist_ok=True)
        with open(output_path, "w") as f:
            yaml.safe_dump(doc, f, sort_keys=False)
        result = {"output": str(output_path), "metric": metric, "rms": est.rms, "gain": est.gain, "offset": est.offset,
                  "iterations": est.iterations, "converged": est.converged,
                  "affine_transform_zyx": doc["affine_transform_zyx"]}
        if metric == "mi":
            result["mi"] = getattr(est, "mi", float("nan"))
        return result
    finally:
        if created:
            import torch.distributed as dist

            dist.destroy_process_group()


@cli.command("characterize-psf")
@click.option("-i", "--input-position-dirpaths", "input_path", required=True, type=click.Path(exists=True, path_type=Path),
              help="Store holding the bead volume (deskewed, for a PSF that `deconvolve` applies to deskewed data).")
@click.option("-c", "--config-filepath", "config", required=True, type=click.Path(exists=True, dir_okay=False, path_type=Path),
              help="CharacterizeSettings YAML (the keys of scripts/measure_psf.py:20-50, plus axis_labels and patch_size).")
@click.option("-o", "--output-dirpath", "output_path", required=True, type=click.Path(path_type=Path),
              help="OME-Zarr store to write the averaged PSF to (what `deconvolve --psf-dirpath` reads); peaks.csv and "
                   "report.json are written inside it.")
@click.option("-p", "--position", default=None, help='Position key ("row/col/fov") (default: the first).')
@click.option("--timepoint", type=int, default=0, show_default=True)
@click.option("--channel", default=None, help="Channel name (default: the first).")
@click.option("--io", "io_backend", type=click.Choice(["auto", "native", "iohub"]), default="auto", show_default=True)
@click.option("--gaussian-fit/--no-gaussian-fit", "gaussian_fit", default=None,
              help="Fit a 3-D Gaussian to every isolated bead and to the average (overrides the YAML's gaussian_fit).")
@click.option("--alignment", type=click.Choice(["voxel", "subvoxel"]), default=None,
              help="Centre the patches on the peak voxel, or on the fitted sub-voxel centre (Fourier shift; implies the fit). "
                   "Overrides the YAML's alignment.")
def characterize_psf(input_path, config, output_path, position, timepoint, channel, io_backend, gaussian_fit, alignment):
    """Detect the beads of a volume and average them into a PSF (PARITY UNPINNED: the rule is this package's own)."""
    click.echo(run_characterize(input_path, config, output_path, position, timepoint, channel, io_backend,
                                gaussian_fit=gaussian_fit, alignment=alignment))


def run_characterize(input_path, config, output_path, position=None, timepoint: int = 0, channel=None,
                     io_backend: str = "auto", gaussian_fit=None, alignment=None) -> dict:
    """Read one bead volume, characterise it (:func:`psf.characterize_psf`), write the PSF store -- HCS, position
    ``0/0/0``, array ``"0"``, T = C = 1, the input's scale: the layout ``DeconvolveSettings.load_psf`` reads -- with
    ``peaks.csv`` (z, y, x, value, isolated, fwhm_z, fwhm_y, fwhm_x; widths in voxels) and ``report.json`` inside it.
    ``gaussian_fit`` / ``alignment`` (not None) override the YAML; when the fit ran, ``peaks.csv`` gains fit_status, mu_z,
    mu_y, mu_x, fit_fwhm_z, fit_fwhm_y, fit_fwhm_x (along the axes) and fit_fwhm_p0, fit_fwhm_p1, fit_fwhm_p2 (principal,
    widest first), and the report the fit's entries and the ``unfit`` indices."""
    import csv
    import json

    import torch

    from .io.omezarr import as_volume_array, open_ome_zarr, position_scale
    from .psf import characterize_psf as characterize
    from .settings import CharacterizeSettings

    settings = CharacterizeSettings.from_yaml(config)
    override = {k: v for k, v in (("gaussian_fit", gaussian_fit), ("alignment", alignment)) if v is not None}
    if override:
        settings = CharacterizeSettings(**dict(settings.model_dump(), **override))
    output_path = Path(output_path)
    if output_path.exists() and any(output_path.iterdir()):
        raise click.ClickException(f"-o: {output_path} exists and is not empty")
    _, _, device, created = _distributed()
    try:
        _, positions = _open_source(Path(input_path), io_backend)
        key = position or next(iter(positions))
        if key not in positions:
            raise click.ClickException(f"position {key!r} not in {input_path} (it has {list(positions)})")
        pos = positions[key]
        names = list(pos.channel_names)
        if channel is None:
            c = 0
        elif channel in names:
            c = names.index(channel)
        else:
            raise click.ClickException(f"channel {channel!r} not in {input_path} (it has {names})")
        arr = as_volume_array(pos["0"])
        if not 0 <= timepoint < arr.shape[0]:
            raise click.ClickException(f"timepoint {timepoint} out of range for {input_path} (T = {arr.shape[0]})")
        scale = tuple(float(v) for v in position_scale(pos)[-3:])
        volume = torch.as_tensor(np.ascontiguousarray(arr.read_volume(timepoint, c), dtype=np.float32), device=device)
        try:
            res = characterize(volume, settings, scale)
        except ValueError as exc:
            raise click.ClickException(str(exc)) from exc
        psf = res.psf.cpu().numpy()
        with open_ome_zarr(output_path, layout="hcs", mode="w", channel_names=[names[c] if names else "PSF"],
                           version="0.5", prefer_iohub=False) as store:
            out = store.create_position("0", "0", "0").create_zeros("0", shape=(1, 1) + psf.shape, dtype="float32",
                                                                      scale=(1.0, 1.0) + scale)
            out.write_volume(0, 0, psf)
        with open(output_path / "peaks.csv", "w", newline="") as f:
            w = csv.writer(f)
            fit = res.fit
            w.writerow(["z", "y", "x", "value", "isolated", "fwhm_z", "fwhm_y", "fwhm_x"] +
                       ([] if fit is None else ["fit_status", "mu_z", "mu_y", "mu_x", "fit_fwhm_z", "fit_fwhm_y", "fit_fwhm_x",
                                                "fit_fwhm_p0", "fit_fwhm_p1", "fit_fwhm_p2"]))
            for i, ((z, y, x), v, iso, fw) in enumerate(zip(res.peaks, res.values, res.isolated, res.fwhm_vox_zyx)):
                row = [int(z), int(y), int(x), repr(float(v)), int(iso)] + [repr(float(q)) for q in fw]
                if fit is not None:
                    row += [int(fit.status[i])] + [repr(float(q)) for q in (*fit.offset_zyx[i], *fit.fwhm_axis_zyx[i],
                                                                            *fit.fwhm_principal[i])]
                w.writerow(row)
        report = dict(res.report(), input=str(input_path), position=key, timepoint=int(timepoint),
                      channel=names[c] if names else str(c), volume_shape_zyx=[int(n) for n in volume.shape],
                      skipped=[int(i) for i in res.skipped], settings=settings.model_dump(mode="json"),
                      parity="UNPINNED: the detection rule is shrimpy_amd's own (biahub's _characterize_psf is not vendored)")
        if res.unfit is not None:
            report["unfit"] = [int(i) for i in res.unfit]
        with open(output_path / "report.json", "w") as f:
            json.dump(report, f, indent=1)
        return {"output": str(output_path), "n_peaks": report["n_peaks"], "n_isolated": report["n_isolated"],
                "n_averaged": report["n_averaged"], "patch_shape_zyx": report["patch_shape_zyx"],
                "psf_fwhm_vox_zyx": report["psf_fwhm_vox_zyx"], "psf_fwhm_zyx": report["psf_fwhm_zyx"]}
    finally:
        if created:
            import torch.distributed as dist

            dist.destroy_process_group()


def _position_file(key: str) -> str:
    return key.replace("/", "_") + ".yml"


@cli.command("estimate-stabilization", cls=_eat_all_command("-i", "--input-position-dirpaths"))
@click.option("-i", "--input-position-dirpaths", "input_path", required=True, multiple=True, type=click.UNPROCESSED,
              help="Time-lapse store (HCS plate or single FOV), or position directories of one plate.")
@click.option("-c", "--config-filepath", "config", required=True, type=click.Path(exists=True, dir_okay=False, path_type=Path),
              help="EstimateStabilizationSettings YAML.")
@click.option("-o", "--output-dirpath", "output_path", required=True, type=click.Path(file_okay=False, path_type=Path),
              help="Directory for one StabilizationSettings YAML per position, <row>_<col>_<fov>.yml.")
@click.option("-p", "--position", "positions", multiple=True, help='Restrict to these position keys ("row/col/fov").')
@click.option("--io", "io_backend", type=click.Choice(["auto", "native", "iohub"]), default="auto", show_default=True)
def estimate_stabilization_cmd(input_path, config, output_path, positions, io_backend):
    """Estimate the per-timepoint drift of every position (config: EstimateStabilizationSettings YAML)."""
    input_path, positions = _inputs(input_path, positions)
    click.echo(run_estimate_stabilization(input_path, config, output_path, positions, io_backend))


def run_estimate_stabilization(input_path, config, output_path, positions=(), io_backend: str = "auto") -> dict:
    """One ``StabilizationSettings`` YAML per position under ``output_path``; rank ``r`` of ``W`` takes the positions
    ``r, r + W, ...`` (``pipeline.shard_units``).  The pixel size is the store's x scale."""
    import torch

    from .io.omezarr import as_volume_array, position_scale
    from .pipeline import shard_units
    from .settings import EstimateStabilizationSettings, StabilizationSettings
    from .stabilize import estimate_stabilization

    settings = EstimateStabilizationSettings.from_yaml(config)
    rank, world, device, created = _distributed()
    try:
        src, src_positions = _open_source(Path(input_path), io_backend)
        with _closing(src):
            keys = _selected_keys(src_positions, positions)
            output_path = Path(output_path)
            output_path.mkdir(parents=True, exist_ok=True)
            written = []
            for key in shard_units(keys, rank, world):
                pos = src_positions[key]
                names = list(pos.channel_names)
                wanted = [settings.stabilization_estimation_channel] + list(settings.stabilization_channels)
                unknown = [n for n in wanted if n not in names]
                if unknown:
                    raise click.ClickException(f"position {key}: channels {unknown} not in the store (it has {names})")
                c = names.index(settings.stabilization_estimation_channel)
                arr = as_volume_array(pos["0"])
                if len(arr.shape) != 5:
                    raise click.ClickException(f"position {key}: expected 5-D TCZYX data, got shape {tuple(arr.shape)}")
                pixel_size = float(position_scale(pos)[-1])

                def series(arr=arr, c=c):
                    for t in range(int(arr.shape[0])):
                        yield torch.as_tensor(np.ascontiguousarray(arr.read_volume(t, c), dtype=np.float32), device=device)

                try:
                    matrices = estimate_stabilization(series(), settings, pixel_size)
                except ValueError as exc:
                    raise click.ClickException(f"position {key}: {exc}") from exc
                doc = StabilizationSettings(stabilization_estimation_channel=settings.stabilization_estimation_channel,
                                            stabilization_type=settings.stabilization_type,
                                            stabilization_channels=list(settings.stabilization_channels),
                                            affine_transform_zyx_list=[m.tolist() for m in matrices])
                doc.to_yaml(output_path / _position_file(key))
                written.append(_position_file(key))
                logger.info("position %s: drift of %d timepoints estimated (last shift %s)", key, len(matrices),
                            matrices[-1][:3, 3].tolist())
        return {"rank": rank, "world_size": world, "output": str(output_path), "written": written}
    finally:
        if created:
            import torch.distributed as dist

            dist.destroy_process_group()


class _NamedChannelStep:
    """``run_store``'s step of the commands that filter the channels they name and copy the others: ``for_unit`` hands out
    ``apply(volume, param_of(unit))`` (``named`` channels) or a plain copy (every other channel); the volume becomes float32
    and keeps its shape."""

    def __init__(self, param_of, apply, named: bool, raw_shape, device):
        self.device = device
        self.output_shape = tuple(int(n) for n in raw_shape)
        self._param_of, self._apply, self._named = param_of, apply, named

    def for_unit(self, unit):
        import torch

        param = self._param_of(unit) if self._named else None

        def step(raw):
            vol = torch.as_tensor(raw, device=self.device).to(torch.float32).contiguous()
            return self._apply(vol, param) if self._named else vol

        return step


def _run_named_channels(input_path, output_path, channels, keys, positions, zarr_version, param_of, apply, fingerprint_extra,
                        **store_options) -> dict:
    """``run_store`` with ``apply(volume, param_of(unit))`` on every volume of the ``channels`` and a copy of the others.

    ``run_store`` has one way to treat some channels differently from the rest, its channel plan for a registration: the
    channels in ``source_channel_names`` take the step the factory builds from the settings, every other channel the step it
    builds from the same settings with ``registration=None``.  So the plan handed over is an identity registration of
    ``channels`` -- nothing is ever warped by it --, and ``registration is not None`` tells the factory that it is building
    the step of the named channels."""
    plan = ReconstructSettings(registration=RegisterSettings(source_channel_names=channels,
                                                             affine_transform_zyx=np.eye(4).tolist()))

    def factory(raw_shape, plan_settings, device):
        return _NamedChannelStep(param_of, apply, plan_settings.registration is not None, raw_shape, device)

    return run_store(input_path, output_path, plan, tuple(keys) if positions else (), zarr_version,
                     reconstructor_factory=factory, fingerprint_extra=fingerprint_extra, **store_options)


@_store_command("stabilize", "Apply per-timepoint translations (config: a StabilizationSettings YAML, or the directory "
                             "estimate-stabilization wrote).", config_directory=True)
def run_stabilize(input_path, config, output_path, positions=(), zarr_version: str = "0.5", resume: bool = False,
                  io_backend: str = "auto", compression=None, on_error: str = "raise", levels: int = 1,
                  level_factor_z: int = 2) -> dict:
    """``stabilize``: every ``(position, t, c)`` volume of a stabilized channel is moved by its timepoint's matrix, the other
    channels are copied.  ``config``: one ``StabilizationSettings`` file for every position, or a directory that holds
    ``<row>_<col>_<fov>.yml`` per position.  Everything is checked before the output store is created."""
    from .io.omezarr import as_volume_array
    from .settings import StabilizationSettings
    from .stabilize import apply_stabilization

    config = Path(config)
    src, src_positions = _open_source(Path(input_path), io_backend)
    with _closing(src):
        keys = _selected_keys(src_positions, positions)
        per_position = {}
        for key in keys:
            path = config / _position_file(key) if config.is_dir() else config
            if not path.exists():
                raise click.ClickException(f"-c: {config} holds no {_position_file(key)} for position {key}")
            try:
                per_position[key] = StabilizationSettings.from_yaml(path)
            except (ValueError, TypeError) as exc:
                raise click.ClickException(f"{path}: {exc}") from exc
            n_t = int(as_volume_array(src_positions[key]["0"]).shape[0])
            n = len(per_position[key].affine_transform_zyx_list)
            if n != n_t:
                raise click.ClickException(f"{path}: {n} matrices for position {key}, whose store has T = {n_t}")
        first = per_position[keys[0]]
        channels = list(first.stabilization_channels)
        if not channels:
            raise click.ClickException("stabilization_channels is empty: nothing to stabilize")
        odd = [k for k, s in per_position.items() if list(s.stabilization_channels) != channels]
        if odd:
            raise click.ClickException(f"positions {odd} name other stabilization_channels than {keys[0]} ({channels})")
        names = list(src_positions[keys[0]].channel_names)
        unknown = [n for n in channels if n not in names]
        if unknown:
            raise click.ClickException(f"stabilization_channels {unknown} not in the store (it has {names})")
    matrices = {k: [np.asarray(m, dtype=np.float64) for m in s.affine_transform_zyx_list] for k, s in per_position.items()}
    return _run_named_channels(input_path, output_path, channels, keys, positions, zarr_version,
                               lambda unit: matrices[unit.position][unit.t], apply_stabilization,
                               {"stabilize": {k: s.model_dump(mode="json") for k, s in per_position.items()}},
                               resume=resume, io_backend=io_backend, compression=compression, on_error=on_error,
                               levels=levels, level_factor_z=level_factor_z)


@dataclass(frozen=True)
class _ChannelFilter:
    """A command that filters the channels its settings name, as ``_run_channel_filter`` runs it."""

    settings: type              # the settings model the YAML is loaded into
    channels: str               # its field that lists the channels to filter, under the name the messages use
    prepare: Callable           # (settings, scale_zyx) -> the filter's parameter for one position; ValueError: the run is refused
    apply: Callable             # (float32 volume, settings, that parameter) -> the filtered volume
    extra: Callable             # (settings, {position key: parameter}) -> the command's ``fingerprint_extra``


def _run_channel_filter(command: _ChannelFilter, input_path, config, output_path, positions, zarr_version, io_backend,
                        **store_options) -> dict:
    """Load and check the settings, find the parameter of every selected position at its scale -- all of it before the output
    store is created --, then ``_run_named_channels``."""
    from .io.omezarr import position_scale

    try:
        settings = command.settings.from_yaml(config)
    except (ValueError, TypeError) as exc:
        raise click.ClickException(f"{config}: {exc}") from exc
    channels = list(getattr(settings, command.channels))
    if not channels:          # (EnhanceSettings allows it, for segment; the other models have refused it already)
        raise click.ClickException(f"{config}: {command.channels} is empty: nothing to filter")
    src, src_positions = _open_source(Path(input_path), io_backend)
    with _closing(src):
        keys = _selected_keys(src_positions, positions)
        names = list(src_positions[keys[0]].channel_names)
        unknown = [n for n in channels if n not in names]
        if unknown:
            raise click.ClickException(f"{command.channels} {unknown} not in the store (it has {names})")
        parameters = {}
        for key in keys:
            scale = tuple(float(v) for v in position_scale(src_positions[key])[-3:])
            try:
                parameters[key] = command.prepare(settings, scale)
            except ValueError as exc:
                raise click.ClickException(f"position {key}: {exc}") from exc
    return _run_named_channels(input_path, output_path, channels, keys, positions, zarr_version,
                               lambda unit: parameters[unit.position], lambda vol, p: command.apply(vol, settings, p),
                               command.extra(settings, parameters), io_backend=io_backend, **store_options)


def _half_widths_extra(name: str):
    """``_ChannelFilter.extra`` of a command whose parameter is a position's half-widths: the document under ``name``."""
    return lambda settings, half_widths: {name: {"settings": settings.model_dump(mode="json"),
                                                 "half_widths": {k: list(v) for k, v in half_widths.items()}}}


def _background_half_widths(settings, scale):
    from .morphology import half_widths_of

    return half_widths_of(settings.radius, scale)


def _background_apply(vol, settings, half_widths):
    from . import morphology

    return getattr(morphology, settings.op)(vol, half_widths)


_BACKGROUND = _ChannelFilter(BackgroundSettings, "channel_names", _background_half_widths, _background_apply,
                             _half_widths_extra("subtract_background"))


@_store_command("subtract-background", """Subtract a slowly varying background: the top-hat of whole channels (config: a
    BackgroundSettings YAML).

    Every volume of the channels channel_names is replaced by its white top-hat (v - opening(v); op: black_tophat gives
    closing(v) - v) under a box of `radius` micrometres (a number or [z, y, x]; 0 on an axis: no window there) at the
    position's scale; the other channels are copied.  The window has to be wider than the objects that are to stay.""")
def run_subtract_background(input_path, config, output_path, positions=(), zarr_version: str = "0.5", resume: bool = False,
                            io_backend: str = "auto", compression=None, on_error: str = "raise", levels: int = 1,
                            level_factor_z: int = 2) -> dict:
    """``subtract-background``: every ``(position, t, c)`` volume of a named channel is replaced by its top-hat
    (``shrimpy_amd/morphology.py``) at the half-widths ``radius`` comes to at the position's ``(z, y, x)`` scale, the other
    channels are copied.  Everything is checked before the output store is created: the settings, the channels, and the
    half-widths of every position against the kernels' cap."""
    return _run_channel_filter(_BACKGROUND, input_path, config, output_path, positions, zarr_version, io_backend, resume=resume,
                               compression=compression, on_error=on_error, levels=levels, level_factor_z=level_factor_z)


def _despeckle_half_widths(settings, scale):
    from . import rank

    if settings.half_widths is not None:
        half_widths = rank._half_widths(settings.half_widths)
    else:
        half_widths = rank.half_widths_of(settings.radius, scale)
    if settings.percentile is not None:
        rank.rank_of_percentile(settings.percentile, rank.window_size(half_widths))
    return half_widths


def _despeckle_apply(vol, s, half_widths):
    from . import rank

    if s.percentile is not None:
        return rank.percentile_filter(vol, s.percentile, half_widths)
    if s.op == "median":
        return rank.median_filter(vol, half_widths)
    return rank.remove_outliers(vol, half_widths, s.threshold, s.op[len("remove_"):])


_DESPECKLE = _ChannelFilter(DespeckleSettings, "channel_names", _despeckle_half_widths, _despeckle_apply,
                            _half_widths_extra("despeckle"))


@_store_command("despeckle", """Remove hot pixels and speckle: a median / outlier-removal filter of whole channels (config: a
    DespeckleSettings YAML).

    Every volume of the channels channel_names is filtered under a box of `radius` micrometres (a number or [z, y, x]) at the
    position's scale, or of `half_widths` voxels ([z, y, x]; hot pixels of a raw stack: [0, 1, 1]); at most 3 voxels to each
    side.  op: median replaces every voxel by the median of its box (or, with `percentile`, by that percentile);
    remove_bright (the default), remove_dark and remove_both replace only the voxels that differ from the median by more than
    `threshold` and leave the others as they are.  The other channels are copied.""")
def run_despeckle(input_path, config, output_path, positions=(), zarr_version: str = "0.5", resume: bool = False,
                  io_backend: str = "auto", compression=None, on_error: str = "raise", levels: int = 1,
                  level_factor_z: int = 2) -> dict:
    """``despeckle``: every ``(position, t, c)`` volume of a named channel goes through the rank filter
    (``shrimpy_amd/rank.py``) at ``half_widths``, or at the half-widths ``radius`` comes to at the position's ``(z, y, x)``
    scale; the other channels are copied.  Everything is checked before the output store is created: the settings, the
    channels, and the half-widths of every position against the kernel's cap."""
    return _run_channel_filter(_DESPECKLE, input_path, config, output_path, positions, zarr_version, io_backend, resume=resume,
                               compression=compression, on_error=on_error, levels=levels, level_factor_z=level_factor_z)


def _enhance_scales(settings, scale):
    from . import hessian

    sigmas, sampling = settings.scales(scale)
    for sigma in sigmas:
        hessian.blur_radii(sigma, sampling)
    return sigmas, sampling


def _enhance_apply(vol, s, scales):
    from . import hessian

    return hessian.enhance(vol, s.measure, scales[0], scales[1], s.dark)


_ENHANCE = _ChannelFilter(EnhanceSettings, "channels", _enhance_scales, _enhance_apply, lambda settings, scales: {
    "enhance": {"settings": settings.model_dump(mode="json"), "scales": {k: [list(v[0]), list(v[1])] for k, v in scales.items()}}})


@_store_command("enhance", """Enhance tubes, sheets or blobs: a filter on the eigenvalues of the smoothed Hessian (config: an
    EnhanceSettings YAML).

    Every volume of the channels `channels` is replaced by its `measure` -- ridge, tube (Sato's tubeness), sheet, blob, log
    (the scale-normalised Laplacian) or an eigenvalue e1 <= e2 <= e3 --, the maximum over the scales `sigmas_um`
    (micrometres, at the position's scale) or `sigmas` (voxels); dark: true looks for dark structures.  The other channels
    are copied.""")
def run_enhance(input_path, config, output_path, positions=(), zarr_version: str = "0.5", resume: bool = False,
                io_backend: str = "auto", compression=None, on_error: str = "raise", levels: int = 1,
                level_factor_z: int = 2) -> dict:
    """``enhance``: every ``(position, t, c)`` volume of a named channel goes through ``hessian.enhance`` at the settings'
    scales -- ``sigmas_um`` at the position's ``(z, y, x)`` scale, ``sigmas`` on the voxel grid --; the other channels are
    copied.  Everything is checked before the output store is created: the settings, the channels, and the blur radius of
    every scale of every position against the blur's cap."""
    return _run_channel_filter(_ENHANCE, input_path, config, output_path, positions, zarr_version, io_backend, resume=resume,
                               compression=compression, on_error=on_error, levels=levels, level_factor_z=level_factor_z)


def _position_translation(position) -> tuple[float, ...]:
    """(T, C, Z, Y, X) NGFF ``translation`` of a position's level 0 (zeros when absent)."""
    ms = position.zattrs.get("multiscales", [{}])
    ds = ms[0].get("datasets", [{}]) if ms else [{}]
    for t in ds[0].get("coordinateTransformations", []):
        if t.get("type") == "translation":
            return tuple(float(v) for v in t["translation"])
    return (0.0,) * 5


def _wells(keys) -> dict:
    """``{"row/col": [position keys in sorted order]}``."""
    wells: dict = {}
    for k in sorted(keys):
        wells.setdefault(k.rsplit("/", 1)[0], []).append(k)
    return wells


@cli.command("estimate-stitch", cls=_eat_all_command("-i", "--input-position-dirpaths"))
@click.option("-i", "--input-position-dirpaths", "input_path", required=True, multiple=True, type=click.UNPROCESSED,
              help="Tiled store (HCS plate: the fields of view of a well are its tiles), or position directories of one plate.")
@click.option("-c", "--config-filepath", "config", required=True, type=click.Path(exists=True, dir_okay=False, path_type=Path),
              help="EstimateStitchSettings YAML.")
@click.option("-o", "--output-filepath", "output_path", required=True, type=click.Path(dir_okay=False, path_type=Path),
              help="The StitchSettings YAML to write (what `stitch -c` takes).")
@click.option("-p", "--position", "positions", multiple=True, help='Restrict to these position keys ("row/col/fov").')
@click.option("--io", "io_backend", type=click.Choice(["auto", "native", "iohub"]), default="auto", show_default=True)
def estimate_stitch_cmd(input_path, config, output_path, positions, io_backend):
    """Estimate where every field of view of a well sits on the well's canvas (config: EstimateStitchSettings YAML)."""
    input_path, positions = _inputs(input_path, positions)
    click.echo(run_estimate_stitch(input_path, config, output_path, positions, io_backend))


def run_estimate_stitch(input_path, config, output_path, positions=(), io_backend: str = "auto") -> dict:
    """``estimate-stitch``: one ``StitchSettings`` YAML for the whole store, ``total_translation`` keyed by position.  Per well
    the positions in sorted name order are the tiles; timepoint 0 of the estimation channel is correlated.  The store reader
    moves whole volumes: a tile's volume is read once, when its overlap crops are cut (``estimate_translations`` asks for all
    crops of a tile in a row), and only the crops are kept and moved to the device -- one volume is on the host at a time."""
    import torch

    from .io.omezarr import as_volume_array, position_scale
    from .settings import EstimateStitchSettings, StitchSettings
    from .stitch import estimate_translations, grid_placement

    try:
        settings = EstimateStitchSettings.from_yaml(config)
    except (ValueError, TypeError) as exc:
        raise click.ClickException(f"{config}: {exc}") from exc
    rank, world, device, created = _distributed()
    try:
        src, src_positions = _open_source(Path(input_path), io_backend)
        with _closing(src):
            keys = _selected_keys(src_positions, positions)
            total: dict = {}
            for well, names in _wells(keys).items():
                arrays = {k: as_volume_array(src_positions[k]["0"]) for k in names}
                for k, a in arrays.items():
                    if len(a.shape) != 5:
                        raise click.ClickException(f"position {k}: expected 5-D TCZYX data, got shape {tuple(a.shape)}")
                channel_names = list(src_positions[names[0]].channel_names)
                if settings.channel not in channel_names:
                    raise click.ClickException(f"well {well}: channel {settings.channel!r} not in the store "
                                               f"(it has {channel_names})")
                c = channel_names.index(settings.channel)
                shapes = {k: tuple(int(n) for n in a.shape[2:]) for k, a in arrays.items()}
                if settings.initial_placement == "grid":
                    initial = dict(zip(names, grid_placement([shapes[k] for k in names], settings.grid_columns,
                                                             settings.percent_overlap)))
                else:
                    initial = {k: tuple(t / sc for t, sc in zip(_position_translation(src_positions[k])[2:],
                                                                position_scale(src_positions[k])[2:])) for k in names}

                @functools.lru_cache(maxsize=1)
                def volume(k, arrays=arrays, c=c):
                    return arrays[k].read_volume(0, c)

                def crop(k, sl):
                    return torch.as_tensor(np.ascontiguousarray(volume(k)[sl], dtype=np.float32), device=device)

                placed = estimate_translations(crop, shapes, initial, settings)
                total.update({k: [float(v) for v in t] for k, t in placed.items()})
                logger.info("well %s: %d tiles placed", well, len(names))
        if rank == 0:
            Path(output_path).parent.mkdir(parents=True, exist_ok=True)
            StitchSettings(total_translation=total).to_yaml(output_path)
        return {"rank": rank, "world_size": world, "output": str(output_path), "positions": len(total)}
    finally:
        if created:
            import torch.distributed as dist

            dist.destroy_process_group()


# share of the free device memory that the tiles of a unit plus its canvas may take before the canvas is composed in bands
STITCH_RESIDENT_SHARE = 0.8


@_store_command("stitch", "Compose the fields of view of every well into one position per well (config: the StitchSettings YAML "
                          "of estimate-stitch).")
def run_stitch(input_path, config, output_path, positions=(), zarr_version: str = "0.5", resume: bool = False,
               io_backend: str = "auto", compression=None, on_error: str = "raise", levels: int = 1,
               level_factor_z: int = 2) -> dict:
    """``stitch``: per well, timepoint and channel the tiles named in ``total_translation`` are composed
    (``stitch.stitch_tiles``; ``stitch.stitch_banded`` when the tiles plus the canvas exceed ``STITCH_RESIDENT_SHARE`` of the
    free device memory, or ``LSR_STITCH_MAX_RESIDENT_BYTES``) into the output position ``row/col/0``: float32 (uint16 tiles
    are converted on load, exactly), the inputs' ``scale``, ``translation = origin * scale``.  The input is read through
    ``io_backend``; the output is written by this package's own writer.  A unit is one (well, t, c) canvas."""
    import torch

    from .io.omezarr import as_volume_array, create_pyramid, open_ome_zarr, position_scale
    from .pipeline import Unit, enumerate_units, run_sharded
    from .pyramid import MAX_LEVELS, build_levels
    from .settings import StitchSettings
    from .stitch import canvas_geometry, stitch_banded, stitch_tiles

    if not 1 <= int(levels) <= MAX_LEVELS or level_factor_z not in (1, 2):
        raise click.ClickException(f"levels must be in 1 .. {MAX_LEVELS} and level_factor_z 1 or 2")
    try:
        settings = StitchSettings.from_yaml(config)
    except (ValueError, TypeError) as exc:
        raise click.ClickException(f"{config}: {exc}") from exc
    rank, world, device, created = _distributed()
    try:
        src, src_positions = _open_source(Path(input_path), io_backend)
        keys = [k for k in src_positions if (not positions or k in positions) and k in settings.total_translation]
        unknown = [k for k in settings.total_translation if k not in src_positions]
        if unknown:
            raise click.ClickException(f"total_translation names positions {unknown} that the store does not have")
        unplaced = [k for k in src_positions if (not positions or k in positions) and k not in settings.total_translation]
        if unplaced:
            raise click.ClickException(f"positions {unplaced} have no total_translation: restrict the run with -p or estimate them")
        if not keys:
            raise click.ClickException("no positions to process")
        wells = _wells(keys)
        arrays = {k: as_volume_array(src_positions[k]["0"]) for k in keys}
        first = src_positions[keys[0]]
        nt, nc = (int(n) for n in arrays[keys[0]].shape[:2])
        channel_names = list(first.channel_names) or [str(i) for i in range(nc)]
        scale = list(position_scale(first))
        for k, a in arrays.items():
            if len(a.shape) != 5 or tuple(int(n) for n in a.shape[:2]) != (nt, nc):
                raise click.ClickException(f"position {k}: shape {tuple(a.shape)}; expected TCZYX with T = {nt}, C = {nc}")
            if np.dtype(a.dtype) not in (np.dtype("uint16"), np.dtype("float32")):
                raise click.ClickException(f"position {k}: data type {a.dtype}; tiles are uint16 or float32")
            if list(position_scale(src_positions[k])) != scale:
                raise click.ClickException(f"position {k}: scale {position_scale(src_positions[k])} differs from {keys[0]}'s")
        wanted = list(settings.channels) if settings.channels else channel_names
        absent = [n for n in wanted if n not in channel_names]
        if absent:
            raise click.ClickException(f"channels {absent} not in the store (it has {channel_names})")
        source_channel = [channel_names.index(n) for n in wanted]
        translations = {w: np.asarray([settings.total_translation[k] for k in ks], dtype=np.float64) for w, ks in wells.items()}
        shapes = {w: [tuple(int(n) for n in arrays[k].shape[2:]) for k in ks] for w, ks in wells.items()}
        geometry = {w: canvas_geometry(shapes[w], translations[w]) for w in wells}
        out_keys = {w: w + "/0" for w in wells}
        fingerprint = _fingerprint(Path(input_path), settings, (nt, len(wanted)), "float32", keys,
                                   {"stitch": {w: list(g[0]) for w, g in geometry.items()}, "levels": int(levels),
                                    "fz": int(level_factor_z)})
        ledger, fail_ledger = _DoneLedger(output_path, fingerprint), _FailLedger(output_path)

        def open_output(mode):
            return open_ome_zarr(output_path, layout="hcs", mode=mode, channel_names=wanted, version=zarr_version,
                                 prefer_iohub=False)

        error = None
        if rank == 0:
            try:
                exists = Path(output_path).exists() and any(Path(output_path).iterdir())
                if exists and not resume:
                    raise FileExistsError(f"{output_path} exists (never overwritten); use --resume to continue an interrupted run")
                if exists:
                    ledger.check()
                dst = open_output("a" if exists else "w")
                have = dict(dst.positions()) if exists else {}
                for w in wells:
                    if out_keys[w] in have:
                        continue
                    shape, origin = geometry[w]
                    row, col = w.split("/")
                    extra = {} if compression in (None, "none") else {"compress": compression}
                    tr = [0.0, 0.0] + [float(o) * float(sc) for o, sc in zip(origin, scale[2:])]
                    create_pyramid(dst.create_position(row, col, "0"), (nt, len(wanted)) + shape, "float32", scale, int(levels),
                                   int(level_factor_z), translation=tr if any(origin) else None, **extra)
                dst.close()
                ledger.begin()
            except click.ClickException as exc:
                error = exc.message
            except Exception as exc:  # noqa: BLE001 -- reported on every rank, see _agree
                error = f"{type(exc).__name__}: {exc}"
        _agree(error)
        dst = open_output("a")
        dst_positions = dict(dst.positions())
        level_arrays = {w: [as_volume_array(dst_positions[out_keys[w]][str(lv)]) for lv in range(int(levels))] for w in wells}
        well_of = {v: k for k, v in out_keys.items()}
        units = enumerate_units(list(out_keys.values()), nt, range(len(wanted)))
        todo = [u for u in units if not (resume and ledger.is_done(u))]
        on_gpu = torch.device(device).type == "cuda"

        def load(u: Unit):
            c = source_channel[u.c]
            return [np.ascontiguousarray(arrays[k].read_volume(u.t, c), dtype=np.float32) for k in wells[well_of[u.position]]]

        def process(data, u: Unit):
            w = well_of[u.position]
            need = 4 * (sum(int(v.size) for v in data) + int(np.prod(geometry[w][0])))
            budget = os.environ.get("LSR_STITCH_MAX_RESIDENT_BYTES")
            if budget is None and on_gpu:
                budget = STITCH_RESIDENT_SHARE * torch.cuda.mem_get_info(device)[0]
            if budget is not None and need > float(budget):
                canvas = stitch_banded(lambda k: torch.as_tensor(data[k], device=device), shapes[w], translations[w],
                                       settings.blending_exponent, settings.cval, max_resident_bytes=int(float(budget)))
            else:
                canvas = stitch_tiles([torch.as_tensor(v, device=device) for v in data], translations[w],
                                      settings.blending_exponent, settings.cval)
            return [lv.cpu().numpy() for lv in [canvas] + build_levels(canvas, int(levels), int(level_factor_z))]

        def store(u: Unit, hosts):
            for arr, lv in zip(level_arrays[well_of[u.position]], hosts):
                arr.write_volume(u.t, u.c, lv)
            ledger.mark(u)
            fail_ledger.clear(u)

        try:
            report = run_sharded(todo, load, process, store, synchronize=torch.cuda.synchronize if on_gpu else None,
                                 process_takes_unit=True, on_error=on_error)
        finally:
            for s_ in (src, dst):
                close = getattr(s_, "close", None)
                if close:
                    close()
        failed = [{"position": u.position, "t": u.t, "c": u.c, "stage": stage, "error": msg} for u, stage, msg in report.failures]
        for u, stage, msg in report.failures:
            fail_ledger.mark(u, stage, msg)
        if world > 1:
            import torch.distributed as dist

            box: list = [None] * world
            dist.all_gather_object(box, failed)
            failed = [f for part in box for f in part]
        return {"rank": rank, "world_size": world, "units": len(report.units), "units_total": len(units),
                "units_skipped": len(units) - len(todo), "failed": failed, "seconds": report.seconds,
                "job_seconds": report.max_seconds, "wells": {out_keys[w]: list(geometry[w][0]) for w in wells}}
    finally:
        if created:
            import torch.distributed as dist

            dist.destroy_process_group()


def _run_object_store(input_path, output_path, positions, zarr_version, io_backend, compression, channel_name: str, suffix: str,
                      result_key: str, process, check_array=None, check_geometry=None) -> dict:
    """What ``run_segment`` and ``run_track`` share: one channel of every selected position goes in, one int32 array per
    position comes out.  Everything is checked before the output store is created (``check_array(key, array)`` and
    ``check_geometry(key, (scale, translation))`` add a command's own refusals); rank 0 creates the store (channel ``<channel_name><suffix>``, the input's ``scale`` and
    ``translation`` copied); the positions are dealt out by rank, and ``process(key, array, channel, out, geometry, device,
    directory)`` fills ``out`` from channel ``channel`` of ``array`` (``geometry``: the 5-D ``(scale, translation)``,
    ``directory``: the position's, for its tables) and returns the position's entry of ``result[result_key]``."""
    from .io.omezarr import as_volume_array, open_ome_zarr, position_scale

    rank, world, device, created = _distributed()
    try:
        src, src_positions = _open_source(Path(input_path), io_backend)
        with _closing(src):
            keys = _selected_keys(src_positions, positions)
            arrays, channel, geometry = {}, {}, {}
            for k in keys:
                pos = src_positions[k]
                names = list(pos.channel_names)
                if channel_name not in names:
                    raise click.ClickException(f"channel_name {channel_name!r} not in position {k} (it has {names})")
                a = as_volume_array(pos["0"])
                if len(a.shape) != 5:
                    raise click.ClickException(f"position {k}: expected 5-D TCZYX data, got shape {tuple(a.shape)}")
                if check_array is not None:
                    check_array(k, a)
                if int(np.prod(a.shape[2:], dtype=np.int64)) > 2 ** 31 - 1:
                    raise click.ClickException(f"position {k}: a volume of {tuple(a.shape[2:])} has more than 2^31 - 1 voxels")
                arrays[k], channel[k] = a, names.index(channel_name)
                geometry[k] = (list(position_scale(pos)), list(_position_translation(pos)))
                if check_geometry is not None:
                    check_geometry(k, geometry[k])
            out_channel = f"{channel_name}{suffix}"
            error = None
            if rank == 0:
                try:
                    if Path(output_path).exists() and any(Path(output_path).iterdir()):
                        raise FileExistsError(f"{output_path} exists (never overwritten)")
                    dst = open_ome_zarr(output_path, layout="hcs", mode="w", channel_names=[out_channel], version=zarr_version,
                                        prefer_iohub=False)
                    extra = {} if compression in (None, "none") else {"compress": compression}
                    for k in keys:
                        scale, translation = geometry[k]
                        shape = (int(arrays[k].shape[0]), 1) + tuple(int(n) for n in arrays[k].shape[2:])
                        dst.create_position(*k.split("/")).create_zeros("0", shape=shape, dtype="int32", scale=scale,
                                                                        translation=translation if any(translation) else None,
                                                                        **extra)
                    dst.close()
                except Exception as exc:  # noqa: BLE001 -- reported on every rank, see _agree
                    error = f"{type(exc).__name__}: {exc}"
            _agree(error)
            dst = open_ome_zarr(output_path, layout="hcs", mode="a", channel_names=[out_channel], version=zarr_version,
                                prefer_iohub=False)
            dst_positions = dict(dst.positions())
            entries = {}
            t0 = time.perf_counter()
            with _closing(dst):
                for k in keys[rank::world]:
                    out = as_volume_array(dst_positions[k]["0"])
                    entries[k] = process(k, arrays[k], channel[k], out, geometry[k], device, Path(output_path) / k)
            return {"rank": rank, "world_size": world, "positions": len(keys[rank::world]), result_key: entries,
                    "seconds": time.perf_counter() - t0, "failed": []}
    finally:
        if created:
            import torch.distributed as dist

            dist.destroy_process_group()


OBJECT_COLUMNS = ("t", "label", "volume_voxels", "volume_um3", "bbox_z0", "bbox_y0", "bbox_x0", "bbox_z1", "bbox_y1", "bbox_x1",
                  "centroid_z", "centroid_y", "centroid_x", "centroid_z_um", "centroid_y_um", "centroid_x_um",
                  "intensity_sum", "intensity_mean", "intensity_min", "intensity_max",
                  "weighted_centroid_z", "weighted_centroid_y", "weighted_centroid_x")


def object_rows(t: int, table: dict, scale_zyx, translation_zyx) -> list[list]:
    """The ``objects.csv`` rows of one timepoint's table (``segment.region_table`` with intensities), in
    ``OBJECT_COLUMNS`` order.  Physical centroids are ``translation + centroid * scale`` of the position's level 0.  A table
    with an ``inscribed_radius`` column (``SegmentSettings.inscribed_radius``) gets it appended behind them, a table with the
    shape columns (``SegmentSettings.shape``) the values of ``SHAPE_OBJECT_COLUMNS`` behind that."""
    sz, sy, sx = (float(v) for v in scale_zyx)
    rows = []
    for k in range(len(table["label"])):
        c = table["centroid"][k]
        um = [float(o) + float(v) * sc for o, v, sc in zip(translation_zyx, c, (sz, sy, sx))]
        rows.append([int(t), int(table["label"][k]), int(table["volume"][k]), float(table["volume"][k]) * sz * sy * sx,
                     *(int(v) for v in table["bbox"][k]), *(float(v) for v in c), *um,
                     float(table["intensity_sum"][k]), float(table["intensity_mean"][k]), float(table["intensity_min"][k]),
                     float(table["intensity_max"][k]), *(float(v) for v in table["weighted_centroid"][k])])
        if "inscribed_radius" in table:
            rows[-1].append(float(table["inscribed_radius"][k]))
        if "axis_lengths" in table:
            rows[-1] += [*(float(v) for v in table["axis_lengths"][k]), *(float(v) for v in table["major_axis"][k]),
                         float(table["surface_area"][k]), float(table["contact_area"][k]), int(table["n_neighbours"][k]),
                         int(table["touches_border"][k])]
    return rows


# what `shape: true` appends to objects.csv, behind every other column
SHAPE_OBJECT_COLUMNS = ("axis_length_major_um", "axis_length_mid_um", "axis_length_minor_um", "major_axis_z", "major_axis_y",
                        "major_axis_x", "surface_area_um2", "contact_area_um2", "n_neighbours", "touches_border")
CONTACT_COLUMNS = ("t", "label_a", "label_b", "faces_z", "faces_y", "faces_x", "area_um2")


@cli.command(cls=_eat_all_command("-i", "--input-position-dirpaths"))
@click.option("-i", "--input-position-dirpaths", "input_path", required=True, multiple=True, type=click.UNPROCESSED,
              help="Input OME-Zarr store (HCS plate or single FOV), or the position directories of one plate.")
@click.option("-c", "--config-filepath", "config", required=True, type=click.Path(exists=True, dir_okay=False, path_type=Path),
              help="SegmentSettings YAML.")
@click.option("-o", "--output-dirpath", "output_path", required=True, type=click.Path(path_type=Path),
              help="Output OME-Zarr store of int32 labels (must not exist); objects.csv is written beside each position's array.")
@click.option("-p", "--position", "positions", multiple=True, help='Restrict to these position keys ("row/col/fov"); repeatable.')
@click.option("--zarr-version", type=click.Choice(["0.4", "0.5"]), default="0.5", show_default=True,
              help="NGFF version of the output store.")
@click.option("--io", "io_backend", type=click.Choice(["auto", "native", "iohub"]), default="auto", show_default=True,
              help="Store access for the input: this package's reader, iohub, or native with iohub as the fallback.")
@click.option("--compression", type=click.Choice(["none", "gzip", "zstd", "blosc-zstd"]), default="blosc-zstd", show_default=True,
              help="Chunk compression of the output.")
def segment(input_path, config, output_path, positions, zarr_version, io_backend, compression):
    """Label the connected components of one thresholded channel and measure them (config: a SegmentSettings YAML).

    Writes an int32 array "0" with the channel <channel_name>_labels per position, and objects.csv.  There is no --levels:
    a mean pyramid of labels is meaningless (the mean of labels 2 and 4 is not label 3).

    expand_distance (micrometres, the position's scale) grows the filtered labels without overlap; inscribed_radius adds
    the column inscribed_radius_um to objects.csv.  split: true splits touching objects before the size filter: a watershed
    of each object's depth map blurred by split_sigma voxels, basins shallower than split_min_depth (micrometres) merged.

    background_radius (micrometres, a number or [z, y, x]; 0 on an axis: no window there) thresholds the white top-hat of the
    volume under a box of that radius instead of the volume: a slowly varying background goes, objects narrower than the
    window stay.  fill_holes: true fills the holes of the thresholded mask before it is labelled.  median_radius
    (micrometres, a number or [z, y, x]; at most 3 voxels to each side) takes the median of the volume under a box of that
    radius before anything else: speckle goes, edges stay.  enhance ({measure: ridge | tube | sheet | blob | log, sigmas_um:
    [...] or sigmas: [...] in voxels, dark: false}) thresholds a ridge, sheet or blob response of the smoothed Hessian's
    eigenvalues, the maximum over the sigmas, instead of the intensity: tubes, membranes and puncta on an uneven background.

    shape: true measures the final labels and appends to objects.csv the three axis lengths of the ellipsoid with each
    object's second moments and its major axis, the surface area (the staircase area of the voxel faces, about 1.5 times a
    smooth sphere's), the contact area with other labels, the number of neighbours and touches_border.  contacts: true
    writes contacts.csv beside objects.csv: one row per timepoint and pair of labels that share a face, with the shared
    faces per axis and their area.  Plain labels under connectivity 6 never share a face; split and grown labels do."""
    input_path, positions = _inputs(input_path, positions)
    _finish(run_segment(input_path, config, output_path, positions, zarr_version, io_backend, compression))


def run_segment(input_path, config, output_path, positions=(), zarr_version: str = "0.5", io_backend: str = "auto",
                compression=None) -> dict:
    """``segment``: every (position, t) volume of ``channel_name`` goes through ``segment.segment_zyx``; the labels are written
    as ``int32`` (the input's ``scale`` and ``translation`` copied), the object tables of a position's timepoints as
    ``<output>/<position>/objects.csv`` (``OBJECT_COLUMNS``, and ``inscribed_radius_um`` behind them where the setting is on;
    the position's ``(z, y, x)`` scale is the sampling of ``expand_distance`` and of the radius).  With ``shape: true``
    ``SHAPE_OBJECT_COLUMNS`` follow behind every other column; with ``contacts: true`` the touching pairs of every timepoint go
    to ``<output>/<position>/contacts.csv`` (``CONTACT_COLUMNS``; the header alone where nothing touches).  Everything is
    checked before the output store is created; with several ranks the positions are dealt out in turn.  The output is
    written by this package's own writer."""
    import csv

    import torch

    from .segment import contact_table, segment_zyx
    from .settings import SegmentSettings

    try:
        settings = SegmentSettings.from_yaml(config)
    except (ValueError, TypeError) as exc:
        raise click.ClickException(f"{config}: {exc}") from exc

    def position(key, array, channel, out, geometry, device, directory):
        scale, translation = geometry
        rows, counts, touching = [], [], []
        for t in range(int(array.shape[0])):
            vol = np.ascontiguousarray(array.read_volume(t, channel), dtype=np.float32)
            labels, table, n = segment_zyx(torch.as_tensor(vol, device=device), settings, sampling=scale[2:])
            out.write_volume(t, 0, labels.cpu().numpy())
            rows += object_rows(t, table, scale[2:], translation[2:])
            counts.append(int(n))
            if settings.contacts:
                c = contact_table(labels, scale[2:])
                touching += [[int(t), int(a), int(b), *(int(v) for v in f), float(area)]
                             for a, b, f, area in zip(c["a"], c["b"], c["faces_zyx"], c["area"])]

        def write(name, header, lines):
            with open(directory / name, "w", newline="") as fh:
                w = csv.writer(fh)
                w.writerow(header)
                w.writerows([[repr(v) if isinstance(v, float) else v for v in row] for row in lines])

        write("objects.csv", OBJECT_COLUMNS + (("inscribed_radius_um",) if settings.inscribed_radius else ())
              + (SHAPE_OBJECT_COLUMNS if settings.shape else ()), rows)
        if settings.contacts:
            write("contacts.csv", CONTACT_COLUMNS, touching)
        return counts

    def check_radius(key, geometry):
        """``background_radius`` and ``median_radius`` at the position's scale stay within their kernels' caps."""
        from . import rank
        from .morphology import half_widths_of

        try:
            half_widths_of(settings.background_radius, geometry[0][2:])
        except ValueError as exc:
            raise click.ClickException(f"position {key}: background_radius: {exc}") from exc
        try:
            rank.half_widths_of(settings.median_radius, geometry[0][2:])
        except ValueError as exc:
            raise click.ClickException(f"position {key}: median_radius: {exc}") from exc
        if settings.enhance is not None:
            from . import hessian

            sigmas, grid = settings.enhance.scales(geometry[0][2:])
            try:
                for sigma in sigmas:
                    hessian.blur_radii(sigma, grid)
            except ValueError as exc:
                raise click.ClickException(f"position {key}: enhance: {exc}") from exc

    return _run_object_store(input_path, output_path, positions, zarr_version, io_backend, compression, settings.channel_name,
                             "_labels", "objects", position, check_geometry=check_radius)


TRACK_COLUMNS = ("track_id", "t_begin", "t_end", "parent_track_id")
TRACK_OBJECT_COLUMNS = ("t", "label", "track_id", "parent_label", "overlap_voxels", "iou")


@cli.command(cls=_eat_all_command("-i", "--input-position-dirpaths"))
@click.option("-i", "--input-position-dirpaths", "input_path", required=True, multiple=True, type=click.UNPROCESSED,
              help="Input OME-Zarr store of integer labels (HCS plate or single FOV), or the position directories of one plate.")
@click.option("-c", "--config-filepath", "config", required=True, type=click.Path(exists=True, dir_okay=False, path_type=Path),
              help="TrackSettings YAML.")
@click.option("-o", "--output-dirpath", "output_path", required=True, type=click.Path(path_type=Path),
              help="Output OME-Zarr store of int32 track ids (must not exist); tracks.csv and track_objects.csv are written "
                   "beside each position's array.")
@click.option("-p", "--position", "positions", multiple=True, help='Restrict to these position keys ("row/col/fov"); repeatable.')
@click.option("--zarr-version", type=click.Choice(["0.4", "0.5"]), default="0.5", show_default=True,
              help="NGFF version of the output store.")
@click.option("--io", "io_backend", type=click.Choice(["auto", "native", "iohub"]), default="auto", show_default=True,
              help="Store access for the input: this package's reader, iohub, or native with iohub as the fallback.")
@click.option("--compression", type=click.Choice(["none", "gzip", "zstd", "blosc-zstd"]), default="blosc-zstd", show_default=True,
              help="Chunk compression of the output.")
def track(input_path, config, output_path, positions, zarr_version, io_backend, compression):
    """Link the labelled objects of consecutive timepoints by their voxel overlap (config: a TrackSettings YAML).

    Writes an int32 array "0" with the channel <channel_name>_tracks per position (every voxel's track id), tracks.csv
    (track_id, t_begin, t_end, parent_track_id: tracks are contiguous in time, so this is the whole lineage) and
    track_objects.csv (one row per object: its track, the label it was linked to, the shared voxels and their IoU).
    Gap closing is not built: an object that is missing from one frame starts a new track when it comes back."""
    input_path, positions = _inputs(input_path, positions)
    _finish(run_track(input_path, config, output_path, positions, zarr_version, io_backend, compression))


def run_track(input_path, config, output_path, positions=(), zarr_version: str = "0.5", io_backend: str = "auto",
              compression=None) -> dict:
    """``track``: the label volumes of ``channel_name`` of every position go through ``track.Tracker`` in order of ``t`` (each
    is uploaded once; the overlap table of two consecutive frames is ``csrc/overlap.hip``'s, or its host twin's on a CPU-only
    machine); the track ids are written as ``int32`` (the input's ``scale`` and ``translation`` copied), the track table as
    ``<output>/<position>/tracks.csv`` (``TRACK_COLUMNS``) and the per-object links as ``track_objects.csv``
    (``TRACK_OBJECT_COLUMNS``).  Everything is checked before the output store is created; with several ranks the positions are
    dealt out in turn.  The output is written by this package's own writer."""
    import csv

    import torch

    from .settings import TrackSettings
    from .track import Tracker, relabel_by_track

    try:
        settings = TrackSettings.from_yaml(config)
    except (ValueError, TypeError) as exc:
        raise click.ClickException(f"{config}: {exc}") from exc

    def integer_data(key, array):
        if np.dtype(array.dtype).kind not in "iu":
            raise click.ClickException(f"position {key}: data type {array.dtype}; labels are integer data (int32 from segment)")

    def position(key, array, channel, out, geometry, device, directory):
        tracker = Tracker(settings)
        for t in range(int(array.shape[0])):
            vol = np.asarray(array.read_volume(t, channel))
            if vol.size and (int(vol.max()) > 2 ** 31 - 1 or int(vol.min()) < -2 ** 31):
                raise click.ClickException(f"position {key}, t = {t}: a label does not fit int32")
            labels = torch.as_tensor(np.ascontiguousarray(vol, dtype=np.int32), device=device)
            out.write_volume(t, 0, relabel_by_track(labels, tracker.step(labels)).cpu().numpy())
        tracks = tracker.tracks()
        with open(directory / "tracks.csv", "w", newline="") as fh:
            w = csv.writer(fh)
            w.writerow(TRACK_COLUMNS)
            w.writerows(zip(*(tracks[c].tolist() for c in TRACK_COLUMNS)))
        with open(directory / "track_objects.csv", "w", newline="") as fh:
            w = csv.writer(fh)
            w.writerow(TRACK_OBJECT_COLUMNS)
            rows = zip(*(tracks["objects"][c].tolist() for c in TRACK_OBJECT_COLUMNS))
            w.writerows([[repr(v) if isinstance(v, float) else v for v in row] for row in rows])
        return len(tracks["track_id"])

    return _run_object_store(input_path, output_path, positions, zarr_version, io_backend, compression, settings.channel_name,
                             "_tracks", "tracks", position, check_array=integer_data)


MEASURE_COLUMNS = ("t", "label", "volume_voxels", "volume_um3")
# per measured channel `c`: c_sum, c_mean, ...; with a background distance also c_background_voxels, ...
MEASURE_CHANNEL_COLUMNS = ("sum", "mean", "std", "min", "max", "weighted_centroid_z_um", "weighted_centroid_y_um",
                           "weighted_centroid_x_um")
MEASURE_BACKGROUND_COLUMNS = ("background_voxels", "background_mean", "mean_minus_background")


@cli.command(cls=_eat_all_command("-i", "--input-position-dirpaths"))
@click.option("-l", "--labels-dirpath", "labels_path", required=True, type=click.Path(exists=True, file_okay=False, path_type=Path),
              help="OME-Zarr store of integer labels: the output of segment or track, or anything else that wrote integer data.")
@click.option("-i", "--input-position-dirpaths", "input_path", required=True, multiple=True, type=click.UNPROCESSED,
              help="The OME-Zarr store whose channels are measured (HCS plate or single FOV), or the position directories of one plate.")
@click.option("-c", "--config-filepath", "config", required=True, type=click.Path(exists=True, dir_okay=False, path_type=Path),
              help="MeasureSettings YAML.")
@click.option("-o", "--output-dirpath", "output_path", required=True, type=click.Path(path_type=Path),
              help="Output directory (must not exist); measurements.csv is written into <output>/<position>/.")
@click.option("-p", "--position", "positions", multiple=True, help='Restrict to these position keys ("row/col/fov"); repeatable.')
@click.option("--io", "io_backend", type=click.Choice(["auto", "native", "iohub"]), default="auto", show_default=True,
              help="Store access for the inputs: this package's reader, iohub, or native with iohub as the fallback.")
def measure(labels_path, input_path, config, output_path, positions, io_backend):
    """Measure the objects of a label store in the channels of another store (config: a MeasureSettings YAML).

    Writes <output>/<position>/measurements.csv: one row per timepoint and label that has voxels, with the volume and, per
    measured channel c, c_sum, c_mean, c_std, c_min, c_max and the intensity-weighted centroid in micrometres.  uint16 and
    float32 channels are measured as they are stored.  Measuring the output of track gives one row per track id and
    timepoint: the intensity curve of every lineage.

    background_distance (micrometres) adds, per channel, the voxels and the mean of a ring of local background around every
    object -- farther than background_gap from it, within background_gap + background_distance, nearer to it than to any
    other object -- and c_mean_minus_background."""
    input_path, positions = _inputs(input_path, positions)
    _finish(run_measure(labels_path, input_path, config, output_path, positions, io_backend))


def run_measure(labels_path, input_path, config, output_path, positions=(), io_backend: str = "auto") -> dict:
    """``measure``: per (position, t) the label volume of ``label_channel_name`` is uploaded once, ``n`` is its greatest label,
    and every measured channel is uploaded once and goes through ``segment.intensity_table`` (``csrc/intensity.hip``, or its
    host twin on a CPU-only machine) -- uint16 data through the uint16 entry, float32 data through the float32 entry, nothing
    converted; with ``background_distance > 0`` the ring volume (``segment.shell_labels``) is built once per (position, t) and
    every channel takes a second launch on it.  The rows go to ``<output>/<position>/measurements.csv``: ``MEASURE_COLUMNS``,
    then per channel ``c`` the columns ``c_<name>`` of ``MEASURE_CHANNEL_COLUMNS`` (and of ``MEASURE_BACKGROUND_COLUMNS``),
    one row per ``(t, label)`` with voxels, in order of ``t``, then ``label``; physical coordinates are ``translation + index *
    scale`` of the label store's position.  Everything is checked before the output directory is created: the positions exist
    in both stores, the channels exist, the label data is integer and fits int32, ``(T, Z, Y, X)`` and the ``(z, y, x)`` scale
    of the two stores agree per position, the intensity data is uint16 or float32.  With several ranks the positions are dealt
    out in turn."""
    import csv

    import torch

    from .io.omezarr import as_volume_array, position_scale
    from .segment import intensity_table, shell_labels
    from .settings import MeasureSettings

    try:
        settings = MeasureSettings.from_yaml(config)
    except (ValueError, TypeError) as exc:
        raise click.ClickException(f"{config}: {exc}") from exc
    ring = float(settings.background_distance) > 0

    rank, world, device, created = _distributed()
    try:
        label_store, label_positions = _open_source(Path(labels_path), io_backend)
        with _closing(label_store):
            src, src_positions = _open_source(Path(input_path), io_backend)
            with _closing(src):
                missing = [p for p in positions if p not in src_positions]
                if missing:
                    raise click.ClickException(f"positions {missing} not found in {input_path}; available: {list(src_positions)}")
                keys = [k for k in src_positions if not positions or k in positions]
                if not keys:
                    raise click.ClickException("no positions to process")
                plan = {}
                for k in keys:
                    if k not in label_positions:
                        raise click.ClickException(f"position {k} not found in {labels_path}; available: {list(label_positions)}")
                    lpos, pos = label_positions[k], src_positions[k]
                    label_names, names = list(lpos.channel_names), list(pos.channel_names)
                    if settings.label_channel_name not in label_names:
                        raise click.ClickException(f"label_channel_name {settings.label_channel_name!r} not in position {k} of "
                                                   f"{labels_path} (it has {label_names})")
                    measured = list(names) if settings.channels is None else list(settings.channels)
                    absent = [c for c in measured if c not in names]
                    if absent:
                        raise click.ClickException(f"channels {absent} not in position {k} of {input_path} (it has {names})")
                    la, a = as_volume_array(lpos["0"]), as_volume_array(pos["0"])
                    if len(la.shape) != 5 or len(a.shape) != 5:
                        raise click.ClickException(f"position {k}: expected 5-D TCZYX data, got shapes {tuple(la.shape)} and "
                                                   f"{tuple(a.shape)}")
                    if np.dtype(la.dtype).kind not in "iu":
                        raise click.ClickException(f"position {k}: label data type {la.dtype}; labels are integer data")
                    if np.dtype(a.dtype) not in (np.dtype(np.uint16), np.dtype(np.float32)):
                        raise click.ClickException(f"position {k}: intensity data type {a.dtype}; uint16 or float32 is measured")
                    shape, other = (int(la.shape[0]),) + tuple(int(v) for v in la.shape[2:]), (int(a.shape[0]),) + tuple(
                        int(v) for v in a.shape[2:])
                    if shape != other:
                        raise click.ClickException(f"position {k}: the labels are (T, Z, Y, X) = {shape}, the intensities {other}")
                    if int(np.prod(shape[1:], dtype=np.int64)) > 2 ** 31 - 1:
                        raise click.ClickException(f"position {k}: a volume of {shape[1:]} has more than 2^31 - 1 voxels")
                    scale, translation = list(position_scale(lpos)), list(_position_translation(lpos))
                    if not np.allclose(scale[2:], list(position_scale(pos))[2:], rtol=1e-9, atol=0.0):
                        raise click.ClickException(f"position {k}: the labels' (z, y, x) scale is {scale[2:]}, the intensities' "
                                                   f"{list(position_scale(pos))[2:]}")
                    lc = label_names.index(settings.label_channel_name)
                    info = np.iinfo(la.dtype)
                    if info.max > 2 ** 31 - 1:             # (a wider type: its values decide)
                        for t in range(shape[0]):
                            vol = np.asarray(la.read_volume(t, lc))
                            if vol.size and (int(vol.max()) > 2 ** 31 - 1 or int(vol.min()) < -2 ** 31):
                                raise click.ClickException(f"position {k}, t = {t}: a label does not fit int32")
                    plan[k] = (la, lc, a, [(c, names.index(c)) for c in measured], scale, translation)
                error = None
                if rank == 0:
                    try:
                        if Path(output_path).exists():
                            raise FileExistsError(f"{output_path} exists (never overwritten)")
                        Path(output_path).mkdir(parents=True)
                    except Exception as exc:  # noqa: BLE001 -- reported on every rank, see _agree
                        error = f"{type(exc).__name__}: {exc}"
                _agree(error)

                def columns(table, background, scale_zyx, translation_zyx):
                    """The values of one channel behind ``MEASURE_COLUMNS``, row by row for the labels with voxels."""
                    integer = table["sum"].dtype.kind == "u"
                    number = int if integer else float
                    out = []
                    for i in np.flatnonzero(table["count"] > 0):
                        um = [float(o) + float(v) * float(sc)
                              for o, v, sc in zip(translation_zyx, table["weighted_centroid"][i], scale_zyx)]
                        row = [number(table["sum"][i]), float(table["mean"][i]), float(table["std"][i]), number(table["min"][i]),
                               number(table["max"][i]), *um]
                        if background is not None:
                            row += [int(background["count"][i]), float(background["mean"][i]),
                                    float(table["mean"][i]) - float(background["mean"][i])]
                        out.append(row)
                    return out

                entries = {}
                t0 = time.perf_counter()
                for k in keys[rank::world]:
                    la, lc, a, channels, scale, translation = plan[k]
                    sz, sy, sx = (float(v) for v in scale[2:])
                    rows = []
                    for t in range(int(la.shape[0])):
                        labels = torch.as_tensor(np.ascontiguousarray(la.read_volume(t, lc), dtype=np.int32), device=device)
                        n = max(int(labels.max().item()), 0)
                        shell = shell_labels(labels, float(settings.background_distance), float(settings.background_gap),
                                             scale[2:]) if ring and n > 0 else None
                        block = None
                        for _, c in channels:
                            values = torch.as_tensor(np.ascontiguousarray(a.read_volume(t, c)), device=device)
                            table = intensity_table(labels, n, values)
                            background = intensity_table(shell, n, values) if shell is not None else None
                            if block is None:
                                live = np.flatnonzero(table["count"] > 0)
                                block = [[int(t), int(table["label"][i]), int(table["count"][i]), float(table["count"][i]) * sz * sy * sx]
                                         for i in live]
                            for row, more in zip(block, columns(table, background, scale[2:], translation[2:])):
                                row += more
                        rows += block or []
                    header = list(MEASURE_COLUMNS)
                    for name, _ in channels:
                        header += [f"{name}_{c}" for c in MEASURE_CHANNEL_COLUMNS + (MEASURE_BACKGROUND_COLUMNS if ring else ())]
                    directory = Path(output_path) / k
                    directory.mkdir(parents=True, exist_ok=True)
                    with open(directory / "measurements.csv", "w", newline="") as fh:
                        w = csv.writer(fh)
                        w.writerow(header)
                        w.writerows([[repr(v) if isinstance(v, float) else v for v in row] for row in rows])
                    entries[k] = len(rows)
                return {"rank": rank, "world_size": world, "positions": len(keys[rank::world]), "rows": entries,
                        "seconds": time.perf_counter() - t0, "failed": []}
    finally:
        if created:
            import torch.distributed as dist

            dist.destroy_process_group()


# colocalization.csv: COLOCALIZE_COLUMNS, then per pair `A__B_<column>` for COLOCALIZE_PAIR_COLUMNS
COLOCALIZE_COLUMNS = ("t", "label", "volume_voxels")
COLOCALIZE_COUNT_COLUMNS = ("count_both", "count_A", "count_B")
COLOCALIZE_PAIR_COLUMNS = ("pearson", "pearson_above", "manders_m1", "manders_m2", "overlap", "k1", "k2", "fraction_both", "a_in_b",
                           "b_in_a") + COLOCALIZE_COUNT_COLUMNS
# the columns that mean nothing without thresholds (Costes' search found the channels uncorrelated): NaN, counts 0
COLOCALIZE_THRESHOLD_COLUMNS = ("pearson_above", "manders_m1", "manders_m2", "fraction_both", "a_in_b", "b_in_a")
COLOCALIZE_SUMMARY_COLUMNS = ("t", "channel_a", "channel_b", "region", "voxels", "threshold_a", "threshold_b",
                              "thresholds_from") + COLOCALIZE_PAIR_COLUMNS


@cli.command(cls=_eat_all_command("-i", "--input-position-dirpaths"))
@click.option("-i", "--input-position-dirpaths", "input_path", required=True, multiple=True, type=click.UNPROCESSED,
              help="The OME-Zarr store whose channels are related (HCS plate or single FOV), or the position directories of one plate.")
@click.option("-l", "--labels-dirpath", "labels_path", default=None, type=click.Path(exists=True, file_okay=False, path_type=Path),
              help="Optional OME-Zarr store of integer labels (the output of segment or track): adds the per-object table.")
@click.option("-c", "--config-filepath", "config", required=True, type=click.Path(exists=True, dir_okay=False, path_type=Path),
              help="ColocalizeSettings YAML.")
@click.option("-o", "--output-dirpath", "output_path", required=True, type=click.Path(path_type=Path),
              help="Output directory (must not exist); the tables are written into <output>/<position>/.")
@click.option("-p", "--position", "positions", multiple=True, help='Restrict to these position keys ("row/col/fov"); repeatable.')
@click.option("--io", "io_backend", type=click.Choice(["auto", "native", "iohub"]), default="auto", show_default=True,
              help="Store access for the inputs: this package's reader, iohub, or native with iohub as the fallback.")
def colocalize(input_path, labels_path, config, output_path, positions, io_backend):
    """Colocalization of pairs of channels, per volume and per labelled object (config: a ColocalizeSettings YAML).

    Writes <output>/<position>/colocalization_summary.csv: per timepoint and pair of channels Pearson's r (over all voxels and
    over the voxels above both thresholds), Manders' M1 and M2, the overlap coefficient with k1 and k2 and the fractions of
    voxels above the thresholds, for the whole volume and -- with -l -- for the labelled voxels, with the thresholds used.
    With -l it also writes <output>/<position>/colocalization.csv: the same per label that has voxels.

    thresholds: [ta, tb] counts a voxel as signal where it is strictly above; thresholds: costes searches Costes' automatic
    thresholds per timepoint and pair over costes_region (volume, or labelled).  uint16 and float32 channels are taken as they
    are stored; the two channels of a pair must have one type."""
    input_path, positions = _inputs(input_path, positions)
    _finish(run_colocalize(input_path, labels_path, config, output_path, positions, io_backend))


def run_colocalize(input_path, labels_path, config, output_path, positions=(), io_backend: str = "auto") -> dict:
    """``colocalize``: per (position, t) the label volume (with ``labels_path``) and every channel that a pair names are uploaded
    once; per pair the thresholds are the settings' or come from ``colocalize.costes_thresholds``, then one launch of
    ``colocalize.pair_table`` (``csrc/coloc.hip``, or its host twin on a CPU-only machine) without labels gives the whole
    volume's record and, with labels, one more gives the records per object, whose sum over the objects is the labelled
    region's.  ``colocalize.coefficients`` turns the records into the columns.  ``<output>/<position>/colocalization.csv``
    (only with labels): ``COLOCALIZE_COLUMNS``, then per pair ``A__B_<column>`` of ``COLOCALIZE_PAIR_COLUMNS``, one row per
    ``(t, label)`` with voxels.  ``<output>/<position>/colocalization_summary.csv``: ``COLOCALIZE_SUMMARY_COLUMNS``, one row per
    ``t``, pair and region (``volume``, and with labels ``labelled``); ``thresholds_from`` is ``settings``, ``costes`` or
    ``costes:uncorrelated`` -- then the thresholds are NaN and so are the columns that need them.  Everything is checked before
    the output directory is created: the positions exist in both stores, the channels exist, a pair's channels have one type,
    uint16 or float32, the label data is integer and fits int32, ``(T, Z, Y, X)`` and the ``(z, y, x)`` scale of the two stores
    agree per position.  With several ranks the positions are dealt out in turn."""
    import csv

    import torch

    from . import colocalize as K
    from .io.omezarr import as_volume_array, position_scale
    from .settings import ColocalizeSettings

    try:
        settings = ColocalizeSettings.from_yaml(config)
    except (ValueError, TypeError) as exc:
        raise click.ClickException(f"{config}: {exc}") from exc
    with_labels = labels_path is not None
    costes = settings.thresholds == "costes"
    if with_labels and settings.label_channel_name is None:
        raise click.ClickException(f"{config}: label_channel_name is needed with a label store (-l)")
    if not with_labels and costes and settings.costes_region == "labelled":
        raise click.ClickException(f"{config}: costes_region 'labelled' needs a label store (-l)")
    pairs = [tuple(pair) for pair in settings.pairs]
    used = list(dict.fromkeys(name for pair in pairs for name in pair))

    rank, world, device, created = _distributed()
    try:
        with contextlib.ExitStack() as stack:
            label_positions = {}
            if with_labels:
                label_store, label_positions = _open_source(Path(labels_path), io_backend)
                stack.enter_context(_closing(label_store))
            src, src_positions = _open_source(Path(input_path), io_backend)
            stack.enter_context(_closing(src))
            missing = [p for p in positions if p not in src_positions]
            if missing:
                raise click.ClickException(f"positions {missing} not found in {input_path}; available: {list(src_positions)}")
            keys = [k for k in src_positions if not positions or k in positions]
            if not keys:
                raise click.ClickException("no positions to process")
            plan = {}
            for k in keys:
                pos = src_positions[k]
                names = list(pos.channel_names)
                absent = [c for c in used if c not in names]
                if absent:
                    raise click.ClickException(f"channels {absent} not in position {k} of {input_path} (it has {names})")
                a = as_volume_array(pos["0"])
                if len(a.shape) != 5:
                    raise click.ClickException(f"position {k}: expected 5-D TCZYX data, got shape {tuple(a.shape)}")
                if np.dtype(a.dtype) not in (np.dtype(np.uint16), np.dtype(np.float32)):
                    raise click.ClickException(f"position {k}: data type {a.dtype}; uint16 or float32 channels are related")
                shape = (int(a.shape[0]),) + tuple(int(v) for v in a.shape[2:])
                if int(np.prod(shape[1:], dtype=np.int64)) > 2 ** 31 - 1:
                    raise click.ClickException(f"position {k}: a volume of {shape[1:]} has more than 2^31 - 1 voxels")
                la = lc = None
                if with_labels:
                    if k not in label_positions:
                        raise click.ClickException(f"position {k} not found in {labels_path}; available: {list(label_positions)}")
                    lpos = label_positions[k]
                    label_names = list(lpos.channel_names)
                    if settings.label_channel_name not in label_names:
                        raise click.ClickException(f"label_channel_name {settings.label_channel_name!r} not in position {k} of "
                                                   f"{labels_path} (it has {label_names})")
                    la = as_volume_array(lpos["0"])
                    if len(la.shape) != 5:
                        raise click.ClickException(f"position {k}: expected 5-D TCZYX labels, got shape {tuple(la.shape)}")
                    if np.dtype(la.dtype).kind not in "iu":
                        raise click.ClickException(f"position {k}: label data type {la.dtype}; labels are integer data")
                    other = (int(la.shape[0]),) + tuple(int(v) for v in la.shape[2:])
                    if shape != other:
                        raise click.ClickException(f"position {k}: the labels are (T, Z, Y, X) = {other}, the channels {shape}")
                    scale = list(position_scale(lpos))
                    if not np.allclose(scale[2:], list(position_scale(pos))[2:], rtol=1e-9, atol=0.0):
                        raise click.ClickException(f"position {k}: the labels' (z, y, x) scale is {scale[2:]}, the channels' "
                                                   f"{list(position_scale(pos))[2:]}")
                    lc = label_names.index(settings.label_channel_name)
                    if np.iinfo(la.dtype).max > 2 ** 31 - 1:             # (a wider type: its values decide)
                        for t in range(shape[0]):
                            vol = np.asarray(la.read_volume(t, lc))
                            if vol.size and (int(vol.max()) > 2 ** 31 - 1 or int(vol.min()) < -2 ** 31):
                                raise click.ClickException(f"position {k}, t = {t}: a label does not fit int32")
                plan[k] = (a, {c: names.index(c) for c in used}, la, lc)
            error = None
            if rank == 0:
                try:
                    if Path(output_path).exists():
                        raise FileExistsError(f"{output_path} exists (never overwritten)")
                    Path(output_path).mkdir(parents=True)
                except Exception as exc:  # noqa: BLE001 -- reported on every rank, see _agree
                    error = f"{type(exc).__name__}: {exc}"
            _agree(error)

            def values_of(table, known: bool):
                """Per record the values behind ``COLOCALIZE_PAIR_COLUMNS``."""
                columns = K.coefficients(table)
                out = []
                for i in range(len(table)):
                    row = [float(columns[c][i]) if known or c not in COLOCALIZE_THRESHOLD_COLUMNS else float("nan")
                           for c in K.COEFFICIENTS]
                    out.append(row + [int(table[c][i]) if known else 0 for c in COLOCALIZE_COUNT_COLUMNS])
                return out

            def total_of(table):
                """One record: the sum of the records of ``table``."""
                one = np.zeros((1,), dtype=table.dtype)
                for f, v in K._totals(table).items():
                    one[f] = v
                return one

            def write(path, header, rows):
                with open(path, "w", newline="") as fh:
                    w = csv.writer(fh)
                    w.writerow(header)
                    w.writerows([[repr(v) if isinstance(v, float) else v for v in row] for row in rows])

            entries = {}
            t0 = time.perf_counter()
            for k in keys[rank::world]:
                a, index, la, lc = plan[k]
                rows, summary = [], []
                for t in range(int(a.shape[0])):
                    labels, n = None, 1
                    if with_labels:
                        labels = torch.as_tensor(np.ascontiguousarray(la.read_volume(t, lc), dtype=np.int32), device=device)
                        n = max(int(labels.max().item()), 0)
                    volumes = {c: torch.as_tensor(np.ascontiguousarray(a.read_volume(t, index[c])), device=device) for c in used}
                    block = None
                    for ca, cb in pairs:
                        va, vb = volumes[ca], volumes[cb]
                        source, known = "settings", True
                        if costes:
                            found = K.costes_thresholds(labels, n, va, vb, region=settings.costes_region)
                            known = found["status"] == "ok"
                            source = "costes" if known else f"costes:{found['status']}"
                            thresholds = (found["ta"], found["tb"])
                        else:
                            thresholds = tuple(float(np.float32(v)) for v in settings.thresholds)
                        launch = thresholds if known else (float("inf"), float("inf"))
                        regions = [("volume", K.pair_table(None, 1, va, vb, launch))]
                        if with_labels:
                            table = K.pair_table(labels, n, va, vb, launch)
                            regions.append(("labelled", total_of(table)))
                            live = np.flatnonzero(table["count"] > 0)
                            if block is None:
                                block = [[int(t), int(i) + 1, int(table["count"][i])] for i in live]
                            for row, more in zip(block, values_of(table[live], known)):
                                row += more
                        for region, record in regions:
                            summary.append([int(t), ca, cb, region, int(record["count"][0]), float(thresholds[0]),
                                            float(thresholds[1]), source] + values_of(record, known)[0])
                    rows += block or []
                directory = Path(output_path) / k
                directory.mkdir(parents=True, exist_ok=True)
                write(directory / "colocalization_summary.csv", list(COLOCALIZE_SUMMARY_COLUMNS), summary)
                if with_labels:
                    header = list(COLOCALIZE_COLUMNS)
                    for ca, cb in pairs:
                        header += [f"{ca}__{cb}_{c}" for c in COLOCALIZE_PAIR_COLUMNS]
                    write(directory / "colocalization.csv", header, rows)
                entries[k] = {"objects": len(rows), "summary": len(summary)}
            return {"rank": rank, "world_size": world, "positions": len(keys[rank::world]), "rows": entries,
                    "seconds": time.perf_counter() - t0, "failed": []}
    finally:
        if created:
            import torch.distributed as dist

            dist.destroy_process_group()


@cli.command("pyramid", cls=_eat_all_command("-i", "--input-position-dirpaths"))
@click.option("-i", "--input-position-dirpaths", "input_path", required=True, multiple=True, type=click.UNPROCESSED,
              help="The store to add levels to, IN PLACE (HCS plate or single FOV), or position directories of one plate.")
@click.option("-p", "--position", "positions", multiple=True, help='Restrict to these position keys ("row/col/fov").')
@click.option("--levels", type=click.IntRange(2, 8), required=True,
              help="Levels the positions have afterwards: arrays \"1\" .. \"N-1\" are added beside \"0\".")
@click.option("--level-factor-z", "level_factor_z", type=click.Choice(["1", "2"]), default="2", show_default=True,
              help="z factor between levels (y and x are always 2).")
def pyramid_cmd(input_path, positions, levels, level_factor_z):
    """Add multiscale levels to an existing store: each the 2x mean of the one above it (uint16 or float32 data)."""
    input_path, positions = _inputs(input_path, positions)
    _finish(run_pyramid(input_path, positions, levels, int(level_factor_z)))


def run_pyramid(store_path, positions=(), levels: int = 2, level_factor_z: int = 2) -> dict:
    """``pyramid``: levels ``1 .. levels - 1`` of every selected position of ``store_path``, written into it.  One
    (position, t, c) volume at a time (``pipeline.run_sharded``): level 0 is read, the levels are computed where the run's
    device is (``pyramid.build_levels``) and stored.  Level 0's files are not touched; only new arrays and the positions'
    group metadata are written (``io.omezarr.add_pyramid_levels``).  Refused: a position that has a level ``"1"``, data
    that is neither uint16 nor float32, an array this package's reader cannot decode."""
    import torch

    from .io.omezarr import Position, UnsupportedCodec, open_ome_zarr
    from .pipeline import Unit, enumerate_units, run_sharded
    from .pyramid import MAX_LEVELS, build_levels

    if not 2 <= int(levels) <= MAX_LEVELS or level_factor_z not in (1, 2):
        raise click.ClickException(f"levels must be in 2 .. {MAX_LEVELS} and level_factor_z 1 or 2")
    rank, world, device, created = _distributed()
    try:
        store = open_ome_zarr(store_path, layout="auto", mode="a", prefer_iohub=False)
        available = dict(store.positions()) if hasattr(store, "positions") else {"0/0/0": store}
        keys = [k for k in available if not positions or k in positions]
        missing = [p for p in positions if p not in available]
        if missing:
            raise click.ClickException(f"positions {missing} not found; available: {list(available)}")
        if not keys:
            raise click.ClickException("no positions to process")
        # everything is checked on every rank before rank 0 writes anything
        try:
            level0 = {k: available[k]["0"] for k in keys}
        except UnsupportedCodec as exc:
            raise click.ClickException(str(exc)) from exc
        shape5, dtype = tuple(level0[keys[0]].shape), np.dtype(level0[keys[0]].dtype)
        for k, a in level0.items():
            if len(a.shape) != 5:
                raise click.ClickException(f"position {k}: expected 5-D TCZYX data, got shape {tuple(a.shape)}")
            if np.dtype(a.dtype) not in (np.dtype("uint16"), np.dtype("float32")):
                raise click.ClickException(f"position {k}: data type {a.dtype}; pyramid levels are computed for uint16 and float32")
            if tuple(a.shape) != shape5 or np.dtype(a.dtype) != dtype:
                raise click.ClickException(f"position {k} {tuple(a.shape)} {a.dtype} differs from {keys[0]} {shape5} {dtype}; "
                                           "run them separately (-p)")
            if not isinstance(available[k], Position) or (available[k].path / "1").exists() or len(available[k].levels) > 1:
                raise click.ClickException(f"position {k} already has a level '1': this command only adds levels")
        _agree(None)           # (every rank has looked at the store as it was)
        error = None
        if rank == 0:
            try:
                for k in keys:
                    from .io.omezarr import add_pyramid_levels

                    add_pyramid_levels(available[k], levels, level_factor_z)
            except Exception as exc:  # noqa: BLE001 -- reported on every rank, see _agree
                error = f"{type(exc).__name__}: {exc}"
        _agree(error)
        lower = {k: [available[k][str(lv)] for lv in range(1, levels)] for k in keys}
        units = enumerate_units(keys, shape5[0], range(shape5[1]))

        def load(u: Unit):
            return level0[u.position].read_volume(u.t, u.c)

        def process(vol):
            return [lv.cpu() for lv in build_levels(torch.as_tensor(np.ascontiguousarray(vol), device=device), levels,
                                                    level_factor_z)]

        def store_levels(u: Unit, hosts):
            for arr, lv in zip(lower[u.position], hosts):
                arr.write_volume(u.t, u.c, lv.numpy())

        on_gpu = torch.device(device).type == "cuda"
        report = run_sharded(units, load, process, store_levels, synchronize=torch.cuda.synchronize if on_gpu else None)
        return {"rank": rank, "world_size": world, "units": len(report.units), "units_total": len(units),
                "levels": int(levels), "level_factor_z": int(level_factor_z), "seconds": report.seconds,
                "job_seconds": report.max_seconds, "failed": []}
    finally:
        if created:
            import torch.distributed as dist

            dist.destroy_process_group()


STATISTICS_COLUMNS = ("count", "nan_count", "min", "max", "mean", "std")


def _quantile_name(q: float) -> str:
    return f"q_{q!r}"


def _statistics_document(summary: dict) -> dict:
    """One ``stats.summary`` as ``statistics.json`` holds it: the moments, ``quantiles`` under ``q_<q>``, ``median``, ``iqr``."""
    out = {k: summary[k] for k in STATISTICS_COLUMNS}
    out["quantiles"] = {_quantile_name(q): v for q, v in summary["quantiles"].items()}
    out["median"], out["iqr"] = summary["median"], summary["iqr"]
    return out


class _StoreVolumes:
    """The volumes of one channel over a list of ``(array, t, c)`` as a re-iterable of device tensors: every walk reads the
    store again and holds one volume at a time (what ``stats`` pools over)."""

    def __init__(self, sources, device):
        self._sources, self._device = list(sources), device

    def __iter__(self):
        import torch

        for array, t, c in self._sources:
            yield torch.as_tensor(np.ascontiguousarray(array.read_volume(t, c)), device=self._device)


@cli.command(cls=_eat_all_command("-i", "--input-position-dirpaths"))
@click.option("-i", "--input-position-dirpaths", "input_path", required=True, multiple=True, type=click.UNPROCESSED,
              help="The OME-Zarr store whose channels are measured (HCS plate or single FOV), or the position directories of one plate.")
@click.option("-c", "--config-filepath", "config", default=None, type=click.Path(exists=True, dir_okay=False, path_type=Path),
              help="StatisticsSettings YAML (default: every channel, the default quantiles, level volume).")
@click.option("-o", "--output-dirpath", "output_path", required=True, type=click.Path(path_type=Path),
              help="Output directory (must not exist): statistics.json, and <position>/statistics.csv for the volume level.")
@click.option("-p", "--position", "positions", multiple=True, help='Restrict to these position keys ("row/col/fov"); repeatable.')
@click.option("--io", "io_backend", type=click.Choice(["auto", "native", "iohub"]), default="auto", show_default=True,
              help="Store access for the input: this package's reader, iohub, or native with iohub as the fallback.")
@click.option("--write-metadata", "write_metadata", is_flag=True,
              help="Also patch the INPUT store's position groups: `normalization` (per channel fov_statistics and "
                   "dataset_statistics: mean, std, median, iqr) and omero.channels[i].window (min, max, start = q_0.001, "
                   "end = q_0.999).  Needs the levels position and dataset and the quantiles 0.001 and 0.999.")
def statistics(input_path, config, output_path, positions, io_backend, write_metadata):
    """Exact whole-volume statistics of every channel: count, NaN count, min, max, mean, std, quantiles, median and IQR.

    uint16 and float32 data are measured as stored.  Level `volume` uploads each (position, t, channel) volume once and runs
    every pass on the resident volume; levels `position` (pooled over t) and `dataset` (pooled over every selected position)
    each cost one more read of the store per pass of the select (4 for float32, 2 for uint16, times the groups of 8 ranks)."""
    input_path, positions = _inputs(input_path, positions)
    _finish(run_statistics(input_path, config, output_path, positions, io_backend, write_metadata))


def run_statistics(input_path, config, output_path, positions=(), io_backend: str = "auto", write_metadata: bool = False) -> dict:
    """``statistics``: ``stats.summary`` of every selected channel per (position, t) volume, per position and over the dataset,
    as the settings' ``levels`` ask.  ``<output>/<position>/statistics.csv`` (level ``volume``): ``t, channel``,
    ``STATISTICS_COLUMNS``, ``q_<q>`` per quantile, ``median, iqr``.  ``<output>/statistics.json``: ``settings``, ``quantiles``,
    ``positions: {key: {channel: {...}}}`` and ``dataset: {channel: {...}}`` for the levels asked.  Everything is checked before
    the output directory is created: the positions and channels exist, the data is uint16 or float32, one type per channel
    across the positions when the dataset is pooled.  Runs on a CPU-only machine (the host twins).

    ``write_metadata`` patches, through ``Position._patch_zattrs`` and touching nothing else, the INPUT store's position groups
    with ``normalization: {channel: {fov_statistics: {mean, std, median, iqr}, dataset_statistics: {...}}}`` and
    ``omero.channels[i].window = {min, max, start: q_0.001, end: q_0.999}`` (the position's figures).  The ``normalization``
    layout is recalled from VisCy's preprocessing, not checked against it: PARITY UNPINNED."""
    import csv
    import json

    import torch

    from . import stats
    from .io.omezarr import as_volume_array, open_ome_zarr
    from .settings import StatisticsSettings

    try:
        settings = StatisticsSettings.from_yaml(config) if config is not None else StatisticsSettings()
    except (ValueError, TypeError) as exc:
        raise click.ClickException(f"{config}: {exc}") from exc
    levels, qs = set(settings.levels), settings.all_quantiles()
    if write_metadata:
        if not {"position", "dataset"} <= levels:
            raise click.ClickException("--write-metadata needs the levels position and dataset")
        if not {0.001, 0.999} <= set(qs):
            raise click.ClickException("--write-metadata needs the quantiles 0.001 and 0.999 (the contrast window)")
    rank, world, device, created = _distributed()
    try:
        if world > 1 and levels != {"volume"}:
            raise click.ClickException("the levels position and dataset pool on one device: run them with one rank")
        src, src_positions = _open_source(Path(input_path), io_backend)
        with _closing(src):
            keys = _selected_keys(src_positions, positions)
            plan, dtypes = {}, {}
            for k in keys:
                pos = src_positions[k]
                names = list(pos.channel_names)
                measured = list(settings.channel_names) or names
                absent = [c for c in measured if c not in names]
                if absent:
                    raise click.ClickException(f"channel_names {absent} not in position {k} of {input_path} (it has {names})")
                a = as_volume_array(pos["0"])
                if len(a.shape) != 5:
                    raise click.ClickException(f"position {k}: expected 5-D TCZYX data, got shape {tuple(a.shape)}")
                if np.dtype(a.dtype) not in (np.dtype(np.uint16), np.dtype(np.float32)):
                    raise click.ClickException(f"position {k}: data type {a.dtype}; uint16 or float32 is measured")
                for c in measured:
                    if "dataset" in levels and dtypes.setdefault(c, np.dtype(a.dtype)) != np.dtype(a.dtype):
                        raise click.ClickException(f"channel {c}: {dtypes[c]} and {a.dtype} cannot be pooled into one dataset")
                plan[k] = (a, [(c, names.index(c)) for c in measured])
            writable = None
            if write_metadata:
                try:
                    writable = open_ome_zarr(Path(input_path), layout="auto", mode="a", prefer_iohub=False)
                except Exception as exc:  # noqa: BLE001
                    raise click.ClickException(f"--write-metadata: {input_path} cannot be opened for writing: {exc}") from exc
            error = None
            if rank == 0:
                try:
                    if Path(output_path).exists():
                        raise FileExistsError(f"{output_path} exists (never overwritten)")
                    Path(output_path).mkdir(parents=True)
                except Exception as exc:  # noqa: BLE001 -- reported on every rank, see _agree
                    error = f"{type(exc).__name__}: {exc}"
            _agree(error)
            t0 = time.perf_counter()
            document = {"settings": settings.model_dump(mode="json"), "quantiles": qs}
            rows_written = {}
            if "volume" in levels:
                for k in keys[rank::world]:
                    a, channels = plan[k]
                    rows = []
                    for t in range(int(a.shape[0])):
                        for name, c in channels:
                            vol = torch.as_tensor(np.ascontiguousarray(a.read_volume(t, c)), device=device)
                            s = stats.summary(vol, qs)
                            rows.append([t, name] + [s[f] for f in STATISTICS_COLUMNS] + [s["quantiles"][q] for q in qs]
                                        + [s["median"], s["iqr"]])
                    directory = Path(output_path) / k
                    directory.mkdir(parents=True, exist_ok=True)
                    with open(directory / "statistics.csv", "w", newline="") as fh:
                        w = csv.writer(fh)
                        w.writerow(["t", "channel", *STATISTICS_COLUMNS, *[_quantile_name(q) for q in qs], "median", "iqr"])
                        w.writerows([[repr(v) if isinstance(v, float) else v for v in row] for row in rows])
                    rows_written[k] = len(rows)
            if "position" in levels:
                document["positions"] = {
                    k: {name: _statistics_document(stats.summary(
                        _StoreVolumes([(plan[k][0], t, c) for t in range(int(plan[k][0].shape[0]))], device), qs))
                        for name, c in plan[k][1]} for k in keys}
            if "dataset" in levels:
                document["dataset"] = {
                    name: _statistics_document(stats.summary(
                        _StoreVolumes([(plan[k][0], t, dict(plan[k][1])[name]) for k in keys for t in range(int(plan[k][0].shape[0]))],
                                      device), qs))
                    for name in [c for c, _ in plan[keys[0]][1]]}
            if rank == 0:
                with open(Path(output_path) / "statistics.json", "w") as fh:
                    json.dump(document, fh, indent=1)
            if writable is not None:
                available = dict(writable.positions()) if hasattr(writable, "positions") else {keys[0]: writable}
                for k in keys:
                    per_channel = document["positions"][k]

                    def mutate(attrs, per_channel=per_channel, names=list(src_positions[k].channel_names)):
                        four = ("mean", "std", "median", "iqr")
                        attrs["normalization"] = {
                            name: {"fov_statistics": {f: figures[f] for f in four},
                                   "dataset_statistics": {f: document["dataset"][name][f] for f in four}}
                            for name, figures in per_channel.items()}
                        channels = attrs.setdefault("omero", {}).setdefault("channels", [{"label": n} for n in names])
                        for name, figures in per_channel.items():
                            channels[names.index(name)]["window"] = {
                                "min": figures["min"], "max": figures["max"],
                                "start": figures["quantiles"][_quantile_name(0.001)], "end": figures["quantiles"][_quantile_name(0.999)]}

                    available[k]._patch_zattrs(mutate)
            return {"rank": rank, "world_size": world, "positions": len(keys), "rows": rows_written, "levels": sorted(levels),
                    "metadata_written": bool(write_metadata), "seconds": time.perf_counter() - t0, "failed": []}
    finally:
        if created:
            import torch.distributed as dist

            dist.destroy_process_group()


def _statistics_figures(document: dict, where: str, settings) -> tuple[float, float]:
    """``(sub, div)`` of a method from one channel's entry of ``statistics.json``; ``KeyError``: a figure it needs is absent."""
    if settings.method == "zscore":
        return float(document["mean"]), float(document["std"])
    if settings.method == "robust":
        return float(document["median"]), float(document["iqr"])
    found = []
    for p in (settings.lower_percentile, settings.upper_percentile):
        near = [v for name, v in document["quantiles"].items() if abs(float(name[2:]) - p / 100.0) <= 1e-9]
        if not near:
            raise KeyError(f"{where}: no quantile {p / 100.0!r} (percentile {p})")
        found.append(float(near[0]))
    return found[0], found[1] - found[0]


@_store_command("normalize", """Normalize the intensities of whole channels (config: a NormalizeSettings YAML).

    Every volume of the channels channel_names becomes (v - sub) / div in float32; the other channels are copied.  method:
    percentile (sub = the lower_percentile-th percentile, div = the upper_percentile-th minus it; clip: true clamps to
    [0, 1]), zscore (mean and standard deviation) or robust (median and interquartile range).  level: volume computes each
    volume's own statistics in the step -- per timepoint this is the bleach correction --; position and dataset read
    statistics.json from statistics_dirpath (the output of the statistics command at those levels).  A divisor that is 0 or
    not finite becomes 1 and the unit is listed under `degenerate` in the result.""")
def run_normalize(input_path, config, output_path, positions=(), zarr_version: str = "0.5", resume: bool = False,
                  io_backend: str = "auto", compression=None, on_error: str = "raise", levels: int = 1,
                  level_factor_z: int = 2) -> dict:
    """``normalize``: ``stats.rescale`` of every ``(position, t, c)`` volume of a named channel by the figures of its level, the
    other channels copied (``_run_named_channels``).  Everything is checked before the output store is created: the settings,
    the channels, and -- for the levels ``position`` and ``dataset`` -- that ``statistics.json`` holds the position, the channel
    and the figures the method needs.  The result's ``degenerate`` lists the units whose divisor was replaced by 1."""
    import json
    import math

    from . import stats
    from .settings import NormalizeSettings

    try:
        settings = NormalizeSettings.from_yaml(config)
    except (ValueError, TypeError) as exc:
        raise click.ClickException(f"{config}: {exc}") from exc
    channels = list(settings.channel_names)
    src, src_positions = _open_source(Path(input_path), io_backend)
    with _closing(src):
        keys = _selected_keys(src_positions, positions)
        names = list(src_positions[keys[0]].channel_names)
        unknown = [n for n in channels if n not in names]
        if unknown:
            raise click.ClickException(f"channel_names {unknown} not in the store (it has {names})")
    figures = {}
    if settings.level != "volume":
        path = Path(settings.statistics_dirpath) / "statistics.json"
        try:
            document = json.loads(path.read_text())
        except (OSError, ValueError) as exc:
            raise click.ClickException(f"{path}: {exc}") from exc
        for key in keys:
            for name in channels:
                where = f"{path}: " + ("dataset" if settings.level == "dataset" else f"position {key}") + f", channel {name}"
                try:
                    entry = document["dataset"][name] if settings.level == "dataset" else document["positions"][key][name]
                    figures[(key, names.index(name))] = _statistics_figures(entry, where, settings)
                except KeyError as exc:
                    raise click.ClickException(f"{where}: statistics.json lacks {exc.args[0]!r}; run `statistics` with the level "
                                               f"{settings.level} and the quantiles the method needs") from exc
    degenerate = []
    clip = (0.0, 1.0) if settings.clip else None

    def safe(unit, sub, div):
        bad = not (math.isfinite(div) and div != 0.0 and math.isfinite(sub))
        if bad:
            degenerate.append({"position": unit.position, "t": int(unit.t), "c": int(unit.c)})
        return (sub if math.isfinite(sub) else 0.0), (div if math.isfinite(div) and div != 0.0 else 1.0)

    def apply(vol, unit):
        if settings.level == "volume":
            sub, div, bad = stats.normalization(vol, settings.method, settings.lower_percentile, settings.upper_percentile)
            if bad:
                degenerate.append({"position": unit.position, "t": int(unit.t), "c": int(unit.c)})
        else:
            sub, div = safe(unit, *figures[(unit.position, int(unit.c))])
        return stats.rescale(vol, sub, div, clip)

    result = _run_named_channels(input_path, output_path, channels, keys, positions, zarr_version, lambda unit: unit, apply,
                                 {"normalize": {"settings": settings.model_dump(mode="json"),
                                                "figures": {f"{k}:{c}": list(v) for (k, c), v in sorted(figures.items())}}},
                                 resume=resume, io_backend=io_backend, compression=compression, on_error=on_error,
                                 levels=levels, level_factor_z=level_factor_z)
    result["degenerate"] = degenerate
    return result


def main():
    cli()


if __name__ == "__main__":
    main()
