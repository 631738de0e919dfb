"""Capture, as data, what the reference's own DynaTrack and preprocessing test files ask of the code this package
stands in for, so that ``tests/test_reference_suites_dropin.py`` checks the drop-in claim without the reference.

    python oracle/capture_dropin.py <reference checkout>

``dynatrack``: the reference's ``shrimpy/tests/test_dynatrack.py`` runs unmodified against the reference's own
estimators (``shrimpy.dynatrack.tracking``), each of the fourteen wrapped by a recorder: every call the suite makes --
the arguments and the reference's result -- goes to ``tests/golden/ref_dropin_dynatrack.npz``.

``preprocessing``: ``shrimpy/tests/test_preprocessing.py`` runs with ``biahub`` (absent upstream) bound to recording
proxies of this package's modules: every name the reference fetches from ``biahub.*`` and every call it makes into it
(the arguments; the results would be this package's own) go to ``tests/golden/ref_dropin_preprocessing.npz``, with what
the reference compares a call against where it does (flat-field: its own ``_flat_field_BF`` on the same volume).

Only arrays, numbers and names are stored.  Calls an estimator makes to another (nested calls) keep their numbers, not
their arrays.  An array the suite drew from a seeded ``np.random.default_rng`` -- scaled, cast, rolled, with a few
elements overwritten -- is stored as that recipe plus the overwritten elements and the SHA-1 of its bytes
(``Store.compact``; ``tests/test_reference_suites_dropin.py::_Arrays`` rebuilds and checks it).  Test infrastructure
only, like the rest of ``oracle/``.
"""

from __future__ import annotations

import hashlib
import json
import re
import sys
import types

from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"

ESTIMATORS = ["_gaussian_blur_3d", "_multiotsu_threshold", "_binary_mask", "_center_of_mass", "_percentile",
              "_intensity_center_of_mass", "_intensity_center_of_mass_to_roi_center", "_multiotsu_center_of_mass",
              "_next_fast_len", "_match_shape", "_phase_cross_corr", "_centered_gaussian_blob", "_roi_center_pcc",
              "_multiotsu_pcc"]
# biahub's modules and the modules of this package bound in their place
BIAHUB = {"biahub.deskew": "shrimpy_amd.deskew", "biahub.settings": "shrimpy_amd.settings",
          "biahub.flat_field_correction": "shrimpy_amd.flatfield"}


class Store:
    """Values -> JSON-able descriptions; arrays (deduplicated) are kept aside for the ``.npz``."""

    def __init__(self):
        self.arrays: dict[str, np.ndarray] = {}
        self._keys: dict[str, str] = {}

    def _put(self, a: np.ndarray) -> str:
        a = np.ascontiguousarray(a)
        h = hashlib.sha1(a.dtype.str.encode() + repr(a.shape).encode() + a.tobytes()).hexdigest()
        if h not in self._keys:
            self._keys[h] = f"a{len(self._keys)}"
            self.arrays[self._keys[h]] = a
        return self._keys[h]

    def enc(self, v):
        import torch

        if isinstance(v, torch.Tensor):
            return {"tensor": self._put(v.detach().cpu().numpy()), "dtype": str(v.dtype).removeprefix("torch.")}
        if isinstance(v, np.ndarray):
            return {"ndarray": self._put(v)}
        if isinstance(v, torch.device):
            return {"device": v.type}
        if isinstance(v, np.generic):
            return {"py": v.item(), "np": v.dtype.name}
        if v is None or isinstance(v, (bool, int, float, str)):
            return {"py": v}
        if isinstance(v, (tuple, list)):
            return {type(v).__name__: [self.enc(x) for x in v]}
        if isinstance(v, dict):
            return {"dict": {str(k): self.enc(x) for k, x in v.items()}}
        raise TypeError(f"cannot record a {type(v).__name__}")

    def save(self, path: Path, manifest: dict) -> None:
        np.savez_compressed(path, manifest=np.array(json.dumps(manifest)), **self.arrays)

    def omit(self, v):
        """The description ``v`` with every array replaced by its shape and type (``{"omitted": shape}``)."""
        if isinstance(v, dict):
            for kind in ("tensor", "ndarray"):
                if kind in v:
                    a = self.arrays[v[kind]]
                    return {"omitted": list(a.shape), "dtype": v.get("dtype", a.dtype.name)}
            return {k: self.omit(x) for k, x in v.items()}
        if isinstance(v, list):
            return [self.omit(x) for x in v]
        return v

    def compact(self, used: set, seeds) -> dict:
        """Keep the arrays in ``used`` only; store each that a seeded ``default_rng(seed).random`` stream reproduces
        (``skip`` values in, times ``scale``, cast, optionally rolled, a few elements overwritten) as that recipe.
        Returns the recipes; ``self.arrays`` then holds the arrays stored as such and the overwritten elements."""
        recipes, kept = {}, {}
        for key in sorted(used, key=lambda k: int(k[1:])):
            a = self.arrays[key]
            r = _recipe(a, seeds)
            if r is None:
                kept[key] = a
                continue
            mask = r.pop("fix", None)
            if mask is not None:
                kept[key + "_mask"], kept[key + "_values"] = np.packbits(mask.ravel()), a[mask]
            r.update(shape=list(a.shape), dtype=a.dtype.name, sha1=hashlib.sha1(a.tobytes()).hexdigest())
            assert np.array_equal(rebuild(r, kept.get(key + "_mask"), kept.get(key + "_values")), a)
            recipes[key] = r
        self.arrays = kept
        return recipes


def _stream(seed: int, n: int) -> np.ndarray:
    return np.random.default_rng(seed).random(n)


def rebuild(r: dict, mask=None, values=None) -> np.ndarray:
    """The array a recipe describes (the inverse of ``_recipe``)."""
    n = int(np.prod(r["shape"]))
    a = (_stream(r["seed"], r["skip"] + n)[r["skip"]:] * r["scale"]).astype(r["dtype"]).reshape(r["shape"])
    if r.get("roll"):
        a = np.roll(a, r["roll"], axis=tuple(range(a.ndim)))
    if mask is not None:
        m = np.unpackbits(mask, count=n).astype(bool).reshape(r["shape"])
        a[m] = values
    return a


def _recipe(a: np.ndarray, seeds, scales=(1.0, 0.1, 0.2, 0.3), volumes=8):
    """A seeded stream that reproduces ``a`` (at most a quarter of its elements overwritten), or None."""
    if a.dtype.kind != "f" or a.size < 64:
        return None
    n = a.size
    for seed in seeds:
        stream = _stream(seed, volumes * n)
        for scale in scales:
            s = (stream * scale).astype(a.dtype)
            # (i) a window of the stream, some elements overwritten: locate it by a few of a's elements
            for k in (0, n // 3, n // 2, n - 1):
                for j in np.flatnonzero(s == a.flat[k])[:4]:
                    skip = int(j) - k
                    if 0 <= skip <= s.size - n:
                        fix = s[skip:skip + n].reshape(a.shape) != a
                        if fix.mean() <= 0.25:
                            return {"seed": seed, "skip": skip, "scale": scale, "fix": fix if fix.any() else None}
            # (ii) the stream's first window, rolled
            head = s[:n].reshape(a.shape)
            for p in np.argwhere(a == head.flat[0])[:4]:
                roll = [int(x) for x in p]
                if np.array_equal(np.roll(head, roll, axis=tuple(range(a.ndim))), a):
                    return {"seed": seed, "skip": 0, "scale": scale, "roll": roll}
    return None


class Outcomes:
    """pytest plugin: how many of the reference's tests passed, failed, were skipped."""

    def __init__(self):
        self.counts = {"passed": 0, "failed": 0, "skipped": 0}

    def pytest_runtest_logreport(self, report):
        if report.when == "call" or report.outcome != "passed":
            self.counts[report.outcome] = self.counts.get(report.outcome, 0) + 1


def _run(target: Path) -> dict:
    import pytest

    out = Outcomes()
    rc = pytest.main([str(target), "--noconftest", "-p", "no:cacheprovider", "-c", "/dev/null",
                      "--rootdir", str(target.parent), "-q"], plugins=[out])
    if rc != 0:
        raise SystemExit(f"the reference's {target.name} did not pass ({rc}): nothing captured")
    return out.counts


def capture_dynatrack(reference: Path) -> None:
    import shrimpy.dynatrack.tracking as tracking

    store, calls, depth = Store(), [], [0]

    def recorder(name, fn):
        def call(*args, **kwargs):
            rec = {"fn": name, "depth": depth[0], "args": store.enc(list(args)), "kwargs": store.enc(kwargs)}
            depth[0] += 1
            try:
                res = fn(*args, **kwargs)
            finally:
                depth[0] -= 1
            rec["result"] = store.enc(res)
            calls.append(rec)
            return res
        return call

    for name in ESTIMATORS:
        setattr(tracking, name, recorder(name, getattr(tracking, name)))
    target = reference / "shrimpy" / "tests" / "test_dynatrack.py"
    counts = _run(target)
    used = set()
    for c in calls:
        if c["depth"]:
            c["args"], c["kwargs"], c["result"] = store.omit(c["args"]), store.omit(c["kwargs"]), store.omit(c["result"])
        else:
            used.update(re.findall(r'"(?:tensor|ndarray)": "(a\d+)"', json.dumps(c)))
    # the seeds the suite's generators are started with (numbers read off the test file)
    seeds = sorted({int(x) for x in re.findall(r"default_rng\((\d+)\)", target.read_text())})
    recipes = store.compact(used, seeds)
    store.save(GOLD / "ref_dropin_dynatrack.npz", {"suite": "shrimpy/tests/test_dynatrack.py", "outcomes": counts,
                                                   "calls": calls, "recipes": recipes})
    print(f"dynatrack: {counts}, {len(calls)} estimator calls, {len(used)} arrays ({len(recipes)} as seeded recipes)")


def _bind_biahub(store, calls: list, fetched: set, twins=None) -> None:
    """Bind ``biahub`` and its modules to recording proxies of this package's modules: every name fetched goes to
    ``fetched``, every call of a function or class to ``calls`` (its arguments; with ``twins[name](...)``, what the
    reference computes for it, as ``reference_result``).  The wrappers keep the wrapped signature, which the
    reference reads to filter settings fields."""
    import functools
    import importlib

    twins = twins or {}

    class Proxy(types.ModuleType):
        def __init__(self, name, target):
            super().__init__(name)
            self._target = target

        def __getattr__(self, attr):
            value = getattr(self._target, attr)
            fetched.add((self.__name__, attr))
            if not isinstance(value, (types.FunctionType, type)):
                return value
            qual = f"{self.__name__}.{attr}"

            @functools.wraps(value)
            def call(*args, **kwargs):
                rec = {"fn": qual, "args": store.enc(list(args)), "kwargs": store.enc(kwargs)}
                if qual in twins:
                    rec["reference_result"] = store.enc(twins[qual](*args, **kwargs))
                calls.append(rec)
                res = value(*args, **kwargs)
                rec["_result"] = res          # for the caller's bookkeeping; not stored
                return res
            return call

    biahub = types.ModuleType("biahub")
    biahub.__path__ = []
    sys.modules["biahub"] = biahub
    for name, ours in BIAHUB.items():
        proxy = Proxy(name, importlib.import_module(ours))
        sys.modules[name] = proxy
        setattr(biahub, name.split(".")[1], proxy)


def capture_preprocessing(reference: Path) -> None:
    import importlib

    import torch

    store, calls, fetched = Store(), [], set()

    def reference_flat_field(vol, axis=0):
        from shrimpy.preprocessing import _LabelfreePreprocessor

        pre = _LabelfreePreprocessor(zyx_shape=np.shape(vol), deskew_settings=None, phase_settings=None, vs_config=None,
                                     output_channel="BF", apply_flatfield=True)
        assert axis == 0
        return pre._flat_field_BF(torch.as_tensor(np.asarray(vol), dtype=torch.float32)).numpy()

    # what the reference itself computes for a call into biahub, where its tests compare the two
    twins = {"biahub.flat_field_correction.flat_field_correction": reference_flat_field}

    _bind_biahub(store, calls, fetched, twins)
    counts = _run(reference / "shrimpy" / "tests" / "test_preprocessing.py")
    for c in calls:
        c.pop("_result")
    store.save(GOLD / "ref_dropin_preprocessing.npz",
               {"suite": "shrimpy/tests/test_preprocessing.py", "outcomes": counts, "modules": BIAHUB,
                "fetched": sorted(map(list, fetched)), "calls": calls})
    print(f"preprocessing: {counts}, names fetched {sorted(fetched)}, {len(calls)} calls")


# the preprocessor runs of tests/test_preprocessing_mirror.py::test_dropin_through_the_reference_preprocessor
PREPROCESSOR_RAW = dict(seed=0, low=80, high=600, shape=(48, 12, 20))
PREPROCESSOR_DESKEW = dict(ls_angle_deg=30.0, pixel_size_um=0.1133, scan_step_um=0.15, keep_overhang=False,
                           average_n_slices=3)
PREPROCESSOR_RUNS = [  # (deskew settings, call keywords)
    (PREPROCESSOR_DESKEW, dict(label="A/1/0", return_intermediates=True)),
    (dict(PREPROCESSOR_DESKEW, orientation="flip_z+rot90", border="grid-constant"), {}),
]


def capture_preprocessor() -> None:
    """The reference's ``build_preprocessor(shape, ["deskew"], ...)`` and one call of the preprocessor it builds, with
    ``biahub`` bound to this package: every name and call it takes from ``biahub`` (settings, the warm-up shape call,
    the deskew call), and what the reference did with the answers -- the shape it kept, the keys it returned, which
    call's result it returned as "BF".  The results themselves are this package's and are not stored."""
    from shrimpy.preprocessing import build_preprocessor

    r = PREPROCESSOR_RAW
    raw = np.random.default_rng(r["seed"]).integers(r["low"], r["high"], r["shape"]).astype(np.uint16)
    store, fetched, runs = Store(), set(), []
    for deskew, call_kw in PREPROCESSOR_RUNS:
        calls = []
        _bind_biahub(store, calls, fetched)
        pre = build_preprocessor(raw.shape, ["deskew"], deskew=dict(deskew), output_channel="BF")
        out = pre(raw, **call_kw)
        results = [c.pop("_result") for c in calls]
        zyx = [i for i, res in enumerate(results) if isinstance(res, tuple) and tuple(res[0]) == tuple(pre._zyx_shape)]
        bf = [i for i, res in enumerate(results) if res is out["BF"]]
        assert len(zyx) == 1 and len(bf) == 1, (zyx, bf)
        runs.append({"deskew": deskew, "call": call_kw, "calls": calls, "zyx_shape": list(pre._zyx_shape),
                     "zyx_from_call": zyx[0], "out_keys": sorted(out), "bf_from_call": bf[0]})
    store.save(GOLD / "ref_dropin_preprocessor.npz", {"raw": r, "modules": BIAHUB, "fetched": sorted(map(list, fetched)),
                                                      "runs": runs})
    print(f"preprocessor: names fetched {sorted(fetched)}, calls {[[c['fn'] for c in x['calls']] for x in runs]}")


def main():
    if len(sys.argv) != 2:
        raise SystemExit("usage: python oracle/capture_dropin.py <reference checkout>")
    reference = Path(sys.argv[1]).resolve()
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(ROOT))
    sys.path.insert(1, str(reference))
    capture_dynatrack(reference)
    capture_preprocessing(reference)
    capture_preprocessor()


if __name__ == "__main__":
    main()
