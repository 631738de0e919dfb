"""The reference's OWN test files, replayed from data with this package standing in for what they exercise.

``oracle/capture_dropin.py`` ran the reference's ``shrimpy/tests/test_dynatrack.py`` (72 tests of its estimators,
trackers and updater) against the reference's own estimators and recorded every call the suite made into them, with
the reference's result; and its ``shrimpy/tests/test_preprocessing.py`` with the absent ``biahub`` bound to this
package, recording every name and call the suite took from ``biahub`` -- including the test that compares the
reference's flat-field with biahub's (skipped upstream: no biahub).  Here each recorded call is made again on this
package's function of the same name (product code on CPU tensors: the native host twins) and must give the
reference's answer, so the reference's suites pass with this package swapped in.  Fixtures:
``tests/golden/ref_dropin_*.npz`` (arrays, numbers and names only; arrays the suite drew from a seeded generator are
stored as that recipe and rebuilt here, checked against the SHA-1 of the recorded bytes).  Calls an estimator made to
another were not part of the suite's own calls (swapped in, the estimators call this package's functions); they keep
their numbers only, and only those that take and return no array are replayed -- 64 of the 156 in the fixture, the
other 92 are not.  The suite's own 49 calls are all replayed in full.

One of them differs: ``_binary_mask(..., otsu_component=1)`` on the reference's otsu-component test gives a mask
3 voxels apart from the reference's, because the 3-class Otsu search inside it lands on a different split that ties
with the reference's to float32 rounding.  That mask is accepted only as such a tie, checked in float64 (see the test).
"""

import hashlib
import importlib
import json
import math

import numpy as np
import torch

ESTIMATORS = ["_gaussian_blur_3d", "_multiotsu_threshold", "_binary_mask", "_center_of_mass", "_percentile",
              "_intensity_center_of_mass", "_intensity_center_of_mass_to_roi_center", "_multiotsu_center_of_mass",
              "_next_fast_len", "_match_shape", "_phase_cross_corr", "_centered_gaussian_blob", "_roi_center_pcc",
              "_multiotsu_pcc"]
# float results: |ours - reference| <= ATOL + RTOL * |reference|
RTOL, ATOL = 1e-5, 1e-5


class _Arrays:
    """The fixture's arrays by key: stored ones as they are, the others rebuilt from their recipe."""

    def __init__(self, z, recipes):
        self._z, self._recipes, self._built = z, recipes, {}

    def __getitem__(self, key):
        from oracle.capture_dropin import rebuild

        if key in self._z.files:
            return self._z[key]
        if key not in self._built:
            r, part = self._recipes[key], (lambda k: self._z[k] if k in self._z.files else None)
            a = rebuild(r, part(key + "_mask"), part(key + "_values"))
            assert hashlib.sha1(a.tobytes()).hexdigest() == r["sha1"], f"{key} does not rebuild to the recorded bytes"
            self._built[key] = a
        return self._built[key]


def _load(golden_dir, name):
    z = np.load(golden_dir / name)
    m = json.loads(str(z["manifest"]))
    return m, _Arrays(z, m.get("recipes", {}))


def _dec(v, z):
    """The recorded value, tensors on the CPU."""
    (kind, x), = ((k, x) for k, x in v.items() if k in ("tensor", "ndarray", "device", "py", "tuple", "list", "dict"))
    if kind == "tensor":
        return torch.as_tensor(z[x].copy()).to(getattr(torch, v["dtype"]))
    if kind == "ndarray":
        return z[x].copy()
    if kind == "device":
        return torch.device("cpu")
    if kind == "py":
        return getattr(np, v["np"])(x) if "np" in v else x
    if kind == "dict":
        return {k: _dec(e, z) for k, e in x.items()}
    return (tuple if kind == "tuple" else list)(_dec(e, z) for e in x)


def _same(ours, want, where):
    if isinstance(want, torch.Tensor):
        assert isinstance(ours, torch.Tensor), f"{where}: {type(ours).__name__} instead of a tensor"
        assert ours.dtype == want.dtype and tuple(ours.shape) == tuple(want.shape), \
            f"{where}: {ours.dtype} {tuple(ours.shape)} instead of {want.dtype} {tuple(want.shape)}"
        o, w = ours.cpu().numpy(), want.numpy()
        if o.dtype.kind in "biu":
            assert np.array_equal(o, w), f"{where}: {int((o != w).sum())} elements differ"
        else:
            assert np.allclose(o, w, rtol=RTOL, atol=ATOL, equal_nan=True), \
                f"{where}: max |difference| {np.nanmax(np.abs(o.astype(np.float64) - w))}"
    elif isinstance(want, (tuple, list)):
        assert isinstance(ours, (tuple, list)) and len(ours) == len(want), f"{where}: {ours!r} instead of {want!r}"
        for i, (a, b) in enumerate(zip(ours, want)):
            _same(a, b, f"{where}[{i}]")
    elif isinstance(want, (bool, np.bool_)) or isinstance(want, (int, np.integer)):
        assert not isinstance(ours, float) and ours == want, f"{where}: {ours!r} instead of {want!r}"
    elif isinstance(want, (float, np.floating)):
        assert math.isclose(float(ours), float(want), rel_tol=RTOL, abs_tol=ATOL), f"{where}: {ours!r} instead of {want!r}"
    else:
        assert ours == want, f"{where}: {ours!r} instead of {want!r}"


def _best_split_with(img, t, component, nbins=256):
    """The largest between-class variance (float64) of a 3-class split of ``img``'s histogram that has ``t`` as its
    threshold ``component`` -- the objective of ``_multiotsu_threshold``, evaluated without float32 rounding."""
    vmin, vmax = float(img.min()), float(img.max())
    hist = torch.histc(img.float(), bins=nbins, min=vmin, max=vmax).double()
    hist /= hist.sum()
    centers = torch.linspace(vmin, vmax, nbins)
    c = centers.double()
    cw, cwm = hist.cumsum(0), (hist * c).cumsum(0)
    mean, eps = cwm[-1], 1e-10
    w0, w1, w2 = cw[:, None], cw[None, :] - cw[:, None], 1.0 - cw[None, :]
    var = (w0 * (cwm[:, None] / w0.clamp_min(eps) - mean) ** 2
           + w1 * ((cwm[None, :] - cwm[:, None]) / w1.clamp_min(eps) - mean) ** 2
           + w2 * ((mean - cwm[None, :]) / w2.clamp_min(eps) - mean) ** 2)
    b = torch.arange(nbins)
    var = var.masked_fill(~((b[None, :] > b[:, None]) & (b[None, :] <= nbins - 2) & (w0 > eps) & (w1 > eps) & (w2 > eps)), -1.0)
    k = int(torch.argmin((centers - t).abs())) - 1      # thresholds are the centres one past the split bins
    return float((var[k, :] if component == 0 else var[:, k]).max())


def test_the_references_dynatrack_tests_pass_with_this_packages_estimators(golden_dir):
    from shrimpy_amd import dynatrack as ours

    m, z = _load(golden_dir, "ref_dropin_dynatrack.npz")
    # the fixture's own record: the reference's suite passed against the reference's estimators when it was captured
    # (this says nothing about this package; the replay below does)
    assert m["outcomes"]["passed"] >= 72 and m["outcomes"]["skipped"] == 0 and m["outcomes"]["failed"] == 0
    assert {c["fn"] for c in m["calls"]} == set(ESTIMATORS)      # the suite reaches every estimator
    assert sum(c["depth"] == 0 for c in m["calls"]) >= 49      # the suite's own calls
    replayed, nested = 0, []
    for i, c in enumerate(m["calls"]):
        if c["depth"]:
            nested.append(c)                      # recorded before the call that made it
            if '"omitted"' in json.dumps(c):
                continue
        ours.invalidate_reference()
        args, kwargs = _dec(c["args"], z), _dec(c["kwargs"], z)
        got, want = getattr(ours, c["fn"])(*args, **kwargs), _dec(c["result"], z)
        replayed += 1
        inner, nested = (nested, []) if not c["depth"] else ([], nested)
        if c["fn"] == "_binary_mask" and not torch.equal(got, want):
            # The 3-class search takes the argmax of a float32 objective, and two splits can tie to its rounding
            # (torch's and numpy's cumulative sums round differently).  The reference's threshold is the one its
            # nested _multiotsu_threshold returned; both must be equally good splits of this package's blurred volume
            # (the same between-class variance to 1e-6 in float64), and the masks may differ only where that volume
            # lies between the two thresholds.
            t_ref = [_dec(n["result"], z) for n in inner if n["fn"] == "_multiotsu_threshold"]
            assert len(t_ref) == 1, f"call {i} _binary_mask: {int((got != want).sum())} elements differ"
            comp = args[2] if len(args) > 2 else kwargs.get("otsu_component", 0)
            blurred, t_ours = ours._blurred_and_threshold(ours._volume(args[0]), args[1] if len(args) > 1 else
                                                         kwargs.get("sigma", 5.0), comp)
            assert torch.equal(got, blurred > t_ours)
            a, b = _best_split_with(blurred, t_ours, comp), _best_split_with(blurred, t_ref[0], comp)
            assert abs(a - b) <= 1e-6 * max(a, b), f"call {i} _binary_mask: threshold {t_ours} (split {a}) against {t_ref[0]} ({b})"
            lo, hi = sorted((t_ours, t_ref[0]))
            between = blurred[got != want]
            assert bool(((between >= lo - ATOL) & (between <= hi + ATOL)).all()), f"call {i} _binary_mask"
            continue
        _same(got, want, f"call {i} {c['fn']}")
    assert replayed >= 100


def test_the_references_preprocessing_tests_pass_with_this_package_bound_as_biahub(golden_dir):
    m, z = _load(golden_dir, "ref_dropin_preprocessing.npz")
    # the fixture's own record of the capture run (not a check of this package; the replay below is)
    assert m["outcomes"]["passed"] >= 12 and m["outcomes"]["skipped"] == 0 and m["outcomes"]["failed"] == 0
    for module, name in m["fetched"]:             # every name the reference takes from biahub is here
        assert hasattr(importlib.import_module(m["modules"][module]), name), f"{module}.{name}"
    assert m["calls"], "the suite makes no call into biahub"
    for c in m["calls"]:
        module, name = c["fn"].rsplit(".", 1)
        got = getattr(importlib.import_module(m["modules"][module]), name)(*_dec(c["args"], z), **_dec(c["kwargs"], z))
        if "reference_result" in c:
            # the reference's own assertion on this pair (shrimpy/tests/test_preprocessing.py: np.allclose, atol=1e-2)
            assert np.allclose(np.asarray(got), _dec(c["reference_result"], z), atol=1e-2), c["fn"]
