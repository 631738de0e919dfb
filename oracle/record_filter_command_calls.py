"""What the whole-channel filter commands -- ``stabilize``, ``subtract-background``, ``despeckle``, ``enhance`` -- hand to
``run_store``, and their ``-h`` texts: the documents the ``--resume`` fingerprint is hashed from (the plan's
``model_dump(mode="json")`` and ``fingerprint_extra``), the position selection and the keywords the command line sets.

    python -m oracle.record_filter_command_calls      # rewrites tests/golden/filter_command_calls.json

``tests/test_filter_commands_host.py`` replays the same invocations (``invocations`` below) on the code under test and
compares for equality; the fixture is recorded on the commit whose calls are to be kept.  ``cli.run_store`` is replaced by
a function that captures and returns ``{}``, so no output store is written and the documents hold no path and no timing.

The input is the two-position store of the label tests (``tests.test_label_host.make_store``: T = 2, channels BF and GFP,
(12, 40, 48) at scale (0.5, 0.25, 0.25)).  Every command runs once on the whole store with the defaults and once on one
position (``-p``) with every shared option set; ``despeckle`` with ``half_widths`` and with ``radius`` and ``percentile``,
``enhance`` with ``sigmas_um``, ``stabilize`` from a directory of per-position files.
"""

from __future__ import annotations

import json
import tempfile

from pathlib import Path

import yaml

FIXTURE = Path(__file__).resolve().parent.parent / "tests" / "golden" / "filter_command_calls.json"
COMMANDS = ("stabilize", "subtract-background", "despeckle", "enhance")
POSITION = "B/2/1"
OPTIONS = ("-p", POSITION, "--levels", "2", "--level-factor-z", "1", "--resume", "--io", "native", "--compression", "zstd",
           "--on-error", "skip", "--zarr-version", "0.4")
KEYWORDS = ("levels", "level_factor_z", "resume", "io_backend", "compression", "on_error")
SETTINGS = {
    "subtract-background": ("subtract-background", dict(channel_names=["GFP"], radius=[0.0, 0.5, 0.75])),
    "despeckle half_widths": ("despeckle", dict(channel_names=["GFP"], half_widths=[0, 1, 1], threshold=50.0)),
    "despeckle percentile": ("despeckle", dict(channel_names=["GFP"], radius=0.5, op="median", percentile=25.0)),
    "enhance": ("enhance", dict(channels=["GFP"], measure="blob", sigmas_um=[0.5, 0.75])),
}
SHIFTS = {"A/1/0": [(0.0, 0.0, 0.0), (1.0, -2.0, 3.5)], "B/2/1": [(0.0, 0.0, 0.0), (-0.5, 1.25, -4.0)]}     # per timepoint, zyx


def invocations(tmp_path):
    """``(name, argv)`` of every recorded run; writes the store and the configs under ``tmp_path``."""
    from tests import test_label_host as LH

    LH.make_store(tmp_path / "in.zarr")
    directory = tmp_path / "stabilization"
    directory.mkdir()
    for key, shifts in SHIFTS.items():
        matrices = [[[1.0, 0.0, 0.0, z], [0.0, 1.0, 0.0, y], [0.0, 0.0, 1.0, x], [0.0, 0.0, 0.0, 1.0]] for z, y, x in shifts]
        doc = dict(stabilization_estimation_channel="BF", stabilization_type="xyz", stabilization_channels=["GFP"],
                   affine_transform_zyx_list=matrices)
        (directory / (key.replace("/", "_") + ".yml")).write_text(yaml.safe_dump(doc))
    configs = {"stabilize": ("stabilize", directory)}
    for name, (command, settings) in SETTINGS.items():
        configs[name] = (command, tmp_path / (name.replace(" ", "_") + ".yml"))
        configs[name][1].write_text(yaml.safe_dump(settings))
    for name, (command, config) in configs.items():
        argv = [command, "-i", str(tmp_path / "in.zarr"), "-c", str(config), "-o", str(tmp_path / "out.zarr")]
        yield name, argv
        yield f"{name} -p", argv + list(OPTIONS)


def record(cli, tmp_path):
    """``(document, handed)``: the document the fixture holds, and per run the ``(reconstructor_factory, plan)`` handed over."""
    from click.testing import CliRunner

    calls, handed = {}, {}

    def capture(input_path, output_path, settings, positions=(), zarr_version="0.4", reconstructor_factory=None, **kw):
        others = sorted(k for k in kw if k not in KEYWORDS + ("fingerprint_extra",))
        assert not others and name not in calls, f"{name}: a second call of run_store, or one that is given {others} too"
        handed[name] = (reconstructor_factory, settings)
        doc = {"settings": settings.model_dump(mode="json"), "fingerprint_extra": kw.get("fingerprint_extra"),
               "positions": list(positions), "zarr_version": zarr_version, **{k: kw.get(k) for k in KEYWORDS}}
        calls[name] = json.loads(json.dumps(doc))      # (tuples become the lists that json makes of them)
        return {}

    real = cli.run_store
    cli.run_store = capture
    try:
        for name, argv in invocations(Path(tmp_path)):
            r = CliRunner().invoke(cli.cli, argv)
            assert r.exit_code == 0 and name in calls, (name, r.output, r.exception)
    finally:
        cli.run_store = real
    helps = {}
    for command in COMMANDS:
        r = CliRunner().invoke(cli.cli, [command, "-h"], terminal_width=80)
        assert r.exit_code == 0, r.output
        helps[command] = r.output
    return {"calls": calls, "help": helps}, handed


def main() -> None:
    import shrimpy_amd.cli as cli

    with tempfile.TemporaryDirectory() as tmp:
        doc, _ = record(cli, tmp)
    FIXTURE.parent.mkdir(parents=True, exist_ok=True)
    FIXTURE.write_text(json.dumps(doc, indent=1, sort_keys=True) + "\n")
    print(f"{len(doc['calls'])} calls, {len(doc['help'])} help texts, {FIXTURE.stat().st_size} bytes -> {FIXTURE}")


if __name__ == "__main__":
    main()
