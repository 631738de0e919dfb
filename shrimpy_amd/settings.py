"""Settings models of the reconstruction path (pydantic, ``extra="forbid"``, YAML-loadable).

``DeskewSettings`` mirrors ``biahub.settings.DeskewSettings`` as the reference uses it:
constructed from a plain dict (``shrimpy/preprocessing.py:137-140``), dumped with
``.model_dump()`` and filtered to the callee's signature (``:44-56``), attributes
``px_to_scan_ratio`` / ``pixel_size_um`` / ``scan_step_um`` read by ``getattr`` (``:240-242``).
Field names are evidenced at ``shrimpy/dynatrack/tracking.py:200-204``,
``shrimpy/dynatrack/manager.py:297-299`` (scale injection) and
``config/mda/mantis/dynatrack_demo.yaml:161-164``; the ratio rounding rule at
``scripts/measure_psf.py:225``.  The strict-validation idiom is the reference's own
(``shrimpy/config.py:82-127``).

``CharacterizeSettings`` takes the keyword arguments of the reference's PSF script (``scripts/measure_psf.py:20-50``).

``RegisterSettings`` and ``DeconvolveSettings`` have no reference counterpart (registration and
deconvolution are "being developed", ``docs/data_structure.md:58-62``); they follow the same idiom.
"""

from __future__ import annotations

from pathlib import Path
from typing import Union, Literal, Optional

import numpy as np
import yaml

from pydantic import (
    BaseModel,
    ConfigDict,
    NonNegativeFloat,
    NonNegativeInt,
    PositiveFloat,
    PositiveInt,
    field_validator,
    model_validator,
)


class _StrictModel(BaseModel):
    model_config = ConfigDict(extra="forbid")

    @classmethod
    def from_yaml(cls, path: str | Path):
        """Load and validate a YAML settings file."""
        with open(path) as f:
            raw = yaml.safe_load(f)
        if not isinstance(raw, dict):
            raise ValueError(f"{path}: expected a mapping at the top level")
        return cls(**raw)

    def to_yaml(self, path: str | Path) -> None:
        with open(path, "w") as f:
            yaml.safe_dump(self.model_dump(mode="json"), f, sort_keys=False)


class DeskewSettings(_StrictModel):
    """Oblique light-sheet deskew parameters.

    Either ``px_to_scan_ratio`` or ``scan_step_um`` must be given; the ratio is derived as
    ``round(pixel_size_um / scan_step_um, 3)`` when absent.
    """

    pixel_size_um: PositiveFloat
    ls_angle_deg: PositiveFloat
    px_to_scan_ratio: Optional[PositiveFloat] = None
    scan_step_um: Optional[PositiveFloat] = None
    keep_overhang: bool = False
    average_n_slices: PositiveInt = 3
    # Switches over the two conventions SURVEY.md section 8 marks [RECALLED]; the defaults are the
    # canonical output.  They reach ``fast_deskew_zyx`` / ``get_deskewed_data_shape`` through the
    # reference's signature filter like every other field.
    orientation: str = "identity"
    border: Literal["constant", "grid-constant"] = "constant"
    # the value outside the stack (scipy's cval): a number, or "min" = the stack's minimum ([RECALLED] what biahub's
    # deskew_data fills with when its cval is None, so None is taken as "min" too)
    cval: Union[float, Literal["min"], None] = 0.0

    @field_validator("orientation")
    @classmethod
    def _check_orientation(cls, v: str) -> str:
        from .geometry import parse_orientation

        parse_orientation(v)
        return v

    @field_validator("ls_angle_deg")
    @classmethod
    def _angle_range(cls, v: float) -> float:
        if v > 45:
            raise ValueError("light-sheet angle must be in (0, 45] degrees")
        return round(float(v), 2)

    @field_validator("px_to_scan_ratio")
    @classmethod
    def _round_ratio(cls, v):
        return None if v is None else round(float(v), 3)

    @model_validator(mode="after")
    def _derive_ratio(self):
        if self.px_to_scan_ratio is None:
            if self.scan_step_um is None:
                raise ValueError(
                    "if px_to_scan_ratio is not provided, both pixel_size_um and scan_step_um "
                    "must be provided"
                )
            ratio = round(self.pixel_size_um / self.scan_step_um, 3)
            if not ratio > 0:
                raise ValueError("derived px_to_scan_ratio rounds to zero")
            object.__setattr__(self, "px_to_scan_ratio", ratio)
        return self


class RegisterSettings(_StrictModel):
    """Affine registration apply (label-free <-> fluorescence).

    ``affine_transform_zyx`` is a homogeneous 4x4 in ZYX voxel units mapping TARGET (output)
    coordinates to SOURCE (moving) coordinates -- the ``scipy.ndimage.affine_transform`` convention.

    ``source_channel_names``: the channels the transform is applied to (empty = every channel);
    any other channel -- ``target_channel_name`` among them -- passes through unwarped
    (``cli._channel_plan``).

    ``keep_overhang`` ([RECALLED] biahub ``register``): ``False`` crops the result to the target grid
    (``output_shape_zyx``, default the moving volume's own shape); ``True`` grows the output to the UNION of the target
    grid and the moving volume's footprint in target coordinates, so nothing of either is lost: the box's lower corner
    is folded into the matrix (``resolved``), the output shape is the box's.
    """

    source_channel_names: list[str] = []
    target_channel_name: Optional[str] = None
    affine_transform_zyx: list[list[float]]
    output_shape_zyx: Optional[tuple[PositiveInt, PositiveInt, PositiveInt]] = None
    mode: Literal["constant", "grid-constant"] = "constant"
    cval: float = 0.0
    keep_overhang: bool = False

    def resolved(self, source_shape_zyx):
        """``(matrix_4x4, output_shape_zyx, origin_zyx)`` this settings object applies to a moving volume of
        ``source_shape_zyx``: the matrix maps OUTPUT indices to source coordinates, ``origin_zyx`` is where output
        index 0 sits in target coordinates (all zero unless ``keep_overhang``)."""
        m = np.asarray(self.affine_transform_zyx, dtype=np.float64)
        src = tuple(int(v) for v in source_shape_zyx)
        tgt = tuple(int(v) for v in (self.output_shape_zyx or src))
        if not self.keep_overhang:
            return m, tgt, (0, 0, 0)
        a, t = m[:3, :3], m[:3, 3]
        if abs(np.linalg.det(a)) < 1e-12:
            raise ValueError("keep_overhang needs an invertible affine_transform_zyx")
        # the moving volume's voxel centres span [0, n - 1] per axis: its corners in target coordinates
        corners = np.array([[z, y, x] for z in (0, src[0] - 1) for y in (0, src[1] - 1) for x in (0, src[2] - 1)], dtype=np.float64)
        in_target = (np.linalg.inv(a) @ (corners - t).T).T
        lo = np.minimum(0.0, np.floor(in_target.min(axis=0) + 1e-9)).astype(np.int64)
        hi = np.maximum(np.asarray(tgt) - 1.0, np.ceil(in_target.max(axis=0) - 1e-9)).astype(np.int64)
        shape = tuple(int(v) for v in (hi - lo + 1))
        if max(shape) >= 1 << 30:
            raise ValueError(f"keep_overhang: the union box {shape} is absurd (a near-singular transform?)")
        grown = m.copy()
        grown[:3, 3] = a @ lo.astype(np.float64) + t        # output index i is target coordinate i + lo
        return grown, shape, tuple(int(v) for v in lo)

    @field_validator("affine_transform_zyx")
    @classmethod
    def _check_affine(cls, v):
        m = np.asarray(v, dtype=np.float64)
        if m.shape != (4, 4):
            raise ValueError(f"affine_transform_zyx must be 4x4, got {m.shape}")
        if not np.all(np.isfinite(m)):
            raise ValueError("affine_transform_zyx contains non-finite entries")
        if not np.allclose(m[3], [0, 0, 0, 1]):
            raise ValueError("last row of affine_transform_zyx must be [0, 0, 0, 1]")
        return m.tolist()


class DeconvolveSettings(_StrictModel):
    """Richardson-Lucy deconvolution.

    The PSF comes from ``psf_path`` -- a ``.npy`` ZYX array, or an OME-Zarr store (an averaged bead
    volume as the PSF-characterisation tools around the reference write them with iohub,
    ``scripts/measure_psf.py:273-287``: HCS layout, first position, array ``"0"``, T = C = 0) -- or, when
    absent, is the separable anisotropic Gaussian ``gaussian_sigma_zyx`` truncated to
    ``gaussian_shape_zyx``.  ``psf_shape_zyx`` (odd) cuts a measured PSF around its brightest voxel and renormalises
    it to sum 1 (``load_psf``).  PSFs of up to 15 taps per axis run through the stencil kernels; larger dense ones -- the
    15 x 18 x 18 ... 30 x 36 x 18 bead patches of ``scripts/measure_psf.py:187-190`` -- run the iteration in the
    Fourier domain (``method``, ``shrimpy_amd/deconvolve_fft.py``), at a cost that does not depend on their size.

    ``separable="auto"`` picks the cheapest exact form of the PSF: three 1-D kernels (one fused launch
    per iteration), else ``ky (x) kzx`` -- a y kernel times a dense (z, x) stencil, the shape of a
    tilted light-sheet PSF -- else the dense stencil.  A factorisation is accepted when it reproduces
    the PSF to ``separable_rtol`` of its peak: the default only admits PSFs that factor exactly; a
    measured PSF can be run in a factored form by raising it (the PSF used is then the factored
    one).  ``"force"`` insists on three 1-D kernels, ``"never"`` on the dense stencil.

    ``tv_lambda`` in ``[0, 1/6)`` turns on total-variation regularisation (RL-TV, Dey et al. 2006: every iteration's
    result divided by ``1 - tv_lambda * div(grad x / |grad x|)``, the gradient norm floored by ``tv_eps``); typical
    values are 0.001 .. 0.05, ``0`` (the default) is plain Richardson-Lucy.

    ``acceleration="biggs-andrews"`` starts every iteration from a point extrapolated along the last change (Biggs &
    Andrews 1997; no tuning parameter): about 10 iterations then reach the likelihood of 20 plain ones, so lower
    ``iterations`` with it.  Not together with ``tv_lambda > 0``.  ``"none"`` (the default) is plain Richardson-Lucy.
    """

    iterations: NonNegativeInt = 20
    eps: PositiveFloat = 1e-6
    tv_lambda: NonNegativeFloat = 0.0
    tv_eps: PositiveFloat = 1e-6
    acceleration: Literal["none", "biggs-andrews"] = "none"
    psf_path: Optional[str] = None
    psf_shape_zyx: Optional[tuple[PositiveInt, PositiveInt, PositiveInt]] = None
    gaussian_sigma_zyx: tuple[PositiveFloat, PositiveFloat, PositiveFloat] = (2.0, 1.2, 1.2)
    gaussian_shape_zyx: tuple[PositiveInt, PositiveInt, PositiveInt] = (9, 7, 7)
    separable: Literal["auto", "force", "never"] = "auto"
    separable_rtol: PositiveFloat = 1e-6
    # "auto": stencil kernels where a tuned one takes the PSF, the Fourier-domain iteration for dense PSFs beyond
    # them (deconvolve.make_plan); "direct" / "fft" insist on one
    method: Literal["auto", "direct", "fft"] = "auto"

    @field_validator("tv_lambda")
    @classmethod
    def _tv_lambda_below_a_sixth(cls, v):
        from .deconvolve import check_tv

        return check_tv(v, 1.0)[0]

    @model_validator(mode="after")
    def _acceleration_without_tv(self):
        from .deconvolve import check_acceleration

        check_acceleration(self.acceleration, self.tv_lambda)
        return self

    @field_validator("gaussian_shape_zyx")
    @classmethod
    def _odd_taps(cls, v):
        if v is not None and (any(n % 2 == 0 for n in v) or v[0] > 31 or max(v[1:]) > 15):
            raise ValueError("the Gaussian's extents must be odd, <= 15 in plane and <= 31 along z")
        return v

    @field_validator("psf_shape_zyx")
    @classmethod
    def _odd_cut(cls, v):
        if v is not None and (any(n % 2 == 0 for n in v) or max(v) > 129):
            raise ValueError("psf_shape_zyx must be odd and <= 129 per axis (beyond 15 taps per axis -- 31 along z for a "
                             "PSF that factors -- the iteration runs in the Fourier domain)")
        return v

    def load_psf(self):
        """The PSF array this block names (``None`` for the Gaussian): float32 ZYX, cut to ``psf_shape_zyx``
        around its peak when that is given (then non-negative and summing to 1)."""
        import numpy as np

        if not self.psf_path:
            return None
        path = str(self.psf_path)
        if path.endswith(".npy"):
            psf = np.load(path)
        else:
            from pathlib import Path

            from .io.omezarr import as_volume_array, open_ome_zarr

            if not Path(path).is_dir():
                raise FileNotFoundError(f"psf_path {path}: neither a .npy file nor an OME-Zarr store")
            with open_ome_zarr(path, prefer_iohub=False) as store:
                _, pos = next(iter(store.positions()))
                psf = as_volume_array(pos["0"]).read_volume(0, 0)
        psf = np.asarray(psf, dtype=np.float32)
        while psf.ndim > 3 and psf.shape[0] == 1:
            psf = psf[0]
        if psf.ndim != 3:
            raise ValueError(f"psf_path {path}: expected a (Z, Y, X) volume, got shape {psf.shape}")
        if self.psf_shape_zyx is not None:
            want = tuple(int(n) for n in self.psf_shape_zyx)
            peak = np.unravel_index(int(np.argmax(psf)), psf.shape)
            lo = [c - n // 2 for c, n in zip(peak, want)]
            if any(a < 0 or a + n > s for a, n, s in zip(lo, want, psf.shape)):
                raise ValueError(f"psf_path {path}: a {want} window around the peak at {tuple(int(c) for c in peak)} "
                                 f"does not fit the {psf.shape} volume")
            psf = np.clip(psf[tuple(slice(a, a + n) for a, n in zip(lo, want))], 0.0, None)
            total = float(psf.sum(dtype=np.float64))
            if not total > 0:
                raise ValueError(f"psf_path {path}: the cut PSF is empty")
            psf = (psf / total).astype(np.float32)
        elif max(psf.shape) > 129 or (self.method == "direct" and max(psf.shape) > 15):
            raise ValueError(f"psf_path {path}: shape {psf.shape} exceeds "
                             + ("the stencil kernels' 15 taps per axis (method='direct')" if max(psf.shape) <= 129
                                else "129 taps per axis")
                             + "; give psf_shape_zyx (odd) to cut it around its peak")
        return np.ascontiguousarray(psf, dtype=np.float32)


class CharacterizeSettings(_StrictModel):
    """Bead detection and PSF characterisation (``shrimpy_amd/psf.py``, the ``characterize-psf`` command).

    The field names are those of the reference's call sites (``scripts/measure_psf.py:20-50, 194-203, 253-263``:
    ``CharacterizeSettings(**bead_detection_settings, axis_labels=..., patch_size=...)``); the arithmetic behind them is
    biahub's and not vendored -- PARITY UNPINNED, the detection rule is this package's own (an exact sliding-window
    maximum, see ``shrimpy_amd/psf.py``).

    ``blur_kernel_size`` (odd): equal-tap box smoothing before detection; ``min_distance``: the window half-widths in
    voxels (one integer or ``(z, y, x)``, each <= 64); ``threshold_abs``: the least smoothed value of a peak;
    ``exclude_border``: peaks closer than this many voxels to a face are dropped; ``max_num_peaks``: keep the N brightest;
    ``patch_size``: the PSF patch ``(z, y, x)`` in the store's physical units, converted with the store's scale and
    rounded up to odd voxel counts (default: 15 x 18 x 18 voxels, ``scripts/measure_psf.py:187``, i.e. 15 x 19 x 19).
    ``block_size``, ``nms_distance`` and ``device`` are accepted for call-site compatibility and **unused**: they
    parametrise biahub's block-pooling detector, detection here is an exact sliding window and runs where the volume is.
    ``axis_labels`` is recorded in the report only.

    ``gaussian_fit``: also fit a 3-D Gaussian to every isolated bead and to the average (``psf.fit_beads``: centres,
    widths along the axes and along the principal axes); ``alignment``: ``"voxel"`` centres the patches on the peak
    voxel, ``"subvoxel"`` moves each onto its fitted centre with a Fourier shift before averaging (and implies the
    fit); ``fit_max_iter``: the fit's iteration limit.  These three are this package's own, not the reference's.
    """

    block_size: tuple[PositiveInt, PositiveInt, PositiveInt] = (8, 8, 8)
    blur_kernel_size: PositiveInt = 3
    nms_distance: Optional[NonNegativeInt] = None
    min_distance: Union[NonNegativeInt, tuple[NonNegativeInt, NonNegativeInt, NonNegativeInt]] = 20
    threshold_abs: float = 200.0
    max_num_peaks: Optional[PositiveInt] = 500
    exclude_border: tuple[NonNegativeInt, NonNegativeInt, NonNegativeInt] = (5, 5, 5)
    device: str = "cuda"
    axis_labels: tuple[str, str, str] = ("Z", "Y", "X")
    patch_size: Optional[tuple[PositiveFloat, PositiveFloat, PositiveFloat]] = None
    gaussian_fit: bool = False
    alignment: Literal["voxel", "subvoxel"] = "voxel"
    fit_max_iter: PositiveInt = 100

    @field_validator("blur_kernel_size")
    @classmethod
    def _odd_blur(cls, v):
        if v % 2 == 0 or v > 129:
            raise ValueError("blur_kernel_size must be odd (and <= 129)")
        return v

    @field_validator("min_distance")
    @classmethod
    def _window_limit(cls, v):
        if max((v,) if isinstance(v, int) else v) > 64:
            raise ValueError("min_distance: the window half-widths are limited to 64 voxels per axis")
        return v

    @field_validator("threshold_abs")
    @classmethod
    def _finite_threshold(cls, v):
        if not np.isfinite(v):
            raise ValueError("threshold_abs must be finite")
        return v

    def patch_shape_zyx(self, zyx_scale=(1.0, 1.0, 1.0)) -> tuple[int, int, int]:
        """``patch_size`` in voxels of a store with ``zyx_scale``: ``ceil(size / scale)`` rounded up to odd."""
        scale = tuple(float(s) for s in zyx_scale)
        if len(scale) != 3 or not all(s > 0 and np.isfinite(s) for s in scale):
            raise ValueError(f"zyx_scale must be three positive numbers, got {zyx_scale!r}")
        size = self.patch_size if self.patch_size is not None else (15 * scale[0], 18 * scale[1], 18 * scale[2])
        out = []
        for length, s in zip(size, scale):
            n = max(1, int(np.ceil(length / s - 1e-6)))       # (15 * s / s may come out as 15.000000000000002)
            out.append(n if n % 2 else n + 1)
        return tuple(out)


class PhaseTransferFunctionSettings(_StrictModel):
    """Optics of the 3-D phase transfer function; lengths in micrometres.  Field names as the reference's ``phase:`` block
    (``config/mda/mantis/dynatrack_demo.yaml:171-178``; ``yx_pixel_size`` / ``z_pixel_size`` are injected by its caller)."""

    wavelength_illumination: PositiveFloat
    yx_pixel_size: PositiveFloat
    z_pixel_size: PositiveFloat
    z_padding: NonNegativeInt = 0
    index_of_refraction_media: PositiveFloat
    numerical_aperture_detection: PositiveFloat
    numerical_aperture_illumination: PositiveFloat
    invert_phase_contrast: bool = False

    @model_validator(mode="after")
    def _check_optics(self):
        na_ill, na_det, n = (self.numerical_aperture_illumination, self.numerical_aperture_detection,
                             self.index_of_refraction_media)
        if not na_ill <= na_det < n:
            raise ValueError(f"need numerical_aperture_illumination <= numerical_aperture_detection < "
                             f"index_of_refraction_media, got {na_ill}, {na_det}, {n}")
        if (na_ill + na_det) / self.wavelength_illumination > 1.0 / (2.0 * self.yx_pixel_size):
            raise ValueError(f"the transfer function's support (NA_ill + NA_det) / wavelength = "
                             f"{(na_ill + na_det) / self.wavelength_illumination:.4g} / um aliases at yx_pixel_size "
                             f"{self.yx_pixel_size} um (Nyquist {1.0 / (2.0 * self.yx_pixel_size):.4g} / um)")
        return self


class PhaseInverseSettings(_StrictModel):
    """``apply_inverse`` of the reference's ``phase:`` block (``dynatrack_demo.yaml:179-181``)."""

    reconstruction_algorithm: Literal["Tikhonov"] = "Tikhonov"
    regularization_strength: PositiveFloat = 1e-3

    @field_validator("reconstruction_algorithm", mode="before")
    @classmethod
    def _tv_is_not_built(cls, v):
        if v == "TV":
            raise ValueError("reconstruction_algorithm 'TV' (total-variation regularised phase) is not built: use 'Tikhonov'")
        return v


class PhaseSettings(_StrictModel):
    """Label-free 3-D phase reconstruction (``shrimpy_amd/phase.py``, the ``phase`` command): the reference's ``phase:`` block."""

    transfer_function: PhaseTransferFunctionSettings
    apply_inverse: PhaseInverseSettings = PhaseInverseSettings()


def _check_matrix_4x4(v, name="affine_transform_zyx"):
    m = np.asarray(v, dtype=np.float64)
    if m.shape != (4, 4):
        raise ValueError(f"{name} must be 4x4, got {m.shape}")
    if not np.all(np.isfinite(m)):
        raise ValueError(f"{name} contains non-finite entries")
    if not np.allclose(m[3], [0, 0, 0, 1]):
        raise ValueError(f"last row of {name} must be [0, 0, 0, 1]")
    return m.tolist()


class FocusFindingSettings(_StrictModel):
    """``focus_finding_settings`` of :class:`EstimateStabilizationSettings` (``shrimpy_amd/focus.py``); lengths in the
    store's units (micrometres)."""

    center_crop_xy: tuple[PositiveInt, PositiveInt] = (800, 800)
    NA_det: PositiveFloat = 1.35
    lambda_ill: PositiveFloat = 0.5
    midband_fractions: tuple[NonNegativeFloat, PositiveFloat] = (0.125, 0.25)
    threshold_FWHM: NonNegativeFloat = 0.0

    @field_validator("midband_fractions")
    @classmethod
    def _ordered(cls, v):
        if not v[0] < v[1]:
            raise ValueError("midband_fractions must be increasing")
        return v


class PhaseCrossCorrSettings(_StrictModel):
    """``phase_cross_corr_settings`` of :class:`EstimateStabilizationSettings` (``dynatrack._phase_cross_corr``)."""

    t_reference: Literal["first", "previous"] = "first"
    center_crop_xy: tuple[PositiveInt, PositiveInt] = (800, 800)
    maximum_shift: PositiveFloat = 1.0


class EstimateStabilizationSettings(_StrictModel):
    """Drift estimation of a time-lapse (``shrimpy_amd/stabilize.py``, the ``estimate-stabilization`` command).  Field
    names are biahub's [RECALLED]; bead-based estimation, averaging across wells and sub-pixel shifts are not built.

    ``stabilization_method`` ``"focus-finding"`` estimates z from the mid-band spectral power of every plane and takes
    ``stabilization_type`` ``"z"`` or ``"xyz"`` (y and x then come from the phase cross-correlation);
    ``"phase-cross-corr"`` takes ``"xy"`` or ``"xyz"``."""

    stabilization_estimation_channel: str
    stabilization_channels: list[str]
    stabilization_type: Literal["z", "xy", "xyz"]
    stabilization_method: Literal["focus-finding", "phase-cross-corr"] = "focus-finding"
    focus_finding_settings: FocusFindingSettings = FocusFindingSettings()
    phase_cross_corr_settings: PhaseCrossCorrSettings = PhaseCrossCorrSettings()

    @model_validator(mode="after")
    def _check_pair(self):
        allowed = {"focus-finding": ("z", "xyz"), "phase-cross-corr": ("xy", "xyz")}[self.stabilization_method]
        if self.stabilization_type not in allowed:
            raise ValueError(f"stabilization_method {self.stabilization_method!r} estimates stabilization_type "
                             f"{' or '.join(repr(a) for a in allowed)}, not {self.stabilization_type!r}")
        return self


class StabilizationSettings(_StrictModel):
    """What ``estimate-stabilization`` writes and ``stabilize`` applies: one 4x4 matrix per timepoint, ZYX voxel units,
    output index -> input coordinate (the ``scipy.ndimage.affine_transform`` convention, as :class:`RegisterSettings`)."""

    stabilization_estimation_channel: str
    stabilization_type: Literal["z", "xy", "xyz"]
    stabilization_channels: list[str]
    affine_transform_zyx_list: list[list[list[float]]]
    time_indices: Literal["all"] = "all"

    @field_validator("affine_transform_zyx_list")
    @classmethod
    def _check_list(cls, v):
        if not v:
            raise ValueError("affine_transform_zyx_list is empty")
        return [_check_matrix_4x4(m, f"affine_transform_zyx_list[{i}]") for i, m in enumerate(v)]


class EstimateStitchSettings(_StrictModel):
    """Placement estimation of a well's tiles (``shrimpy_amd/stitch.py``, the ``estimate-stitch`` command).  biahub's field
    names where recalled [RECALLED] (``percent_overlap``); PARITY UNPINNED.

    ``initial_placement`` ``"metadata"``: each position's level-0 NGFF ``translation`` divided by its ``scale``;
    ``"grid"``: ``grid_columns`` columns at ``percent_overlap``, the positions of a well in sorted name order, row-major.
    ``maximum_shift`` is the padding factor of ``dynatrack._phase_cross_corr``; a pair whose shift reaches
    ``maximum_shift_voxels`` on an axis is dropped, as is one whose least-squares residual exceeds
    ``outlier_threshold_voxels``."""

    channel: str
    initial_placement: Literal["metadata", "grid"] = "metadata"
    grid_columns: Optional[PositiveInt] = None
    percent_overlap: Optional[NonNegativeFloat] = None
    maximum_shift: PositiveFloat = 1.0
    maximum_shift_voxels: PositiveInt = 32
    min_overlap_voxels: PositiveInt = 8
    outlier_threshold_voxels: PositiveFloat = 2.0
    round_to_integer: bool = True

    @model_validator(mode="after")
    def _check_grid(self):
        if self.initial_placement == "grid":
            if self.grid_columns is None or self.percent_overlap is None:
                raise ValueError('initial_placement "grid" needs grid_columns and percent_overlap')
            if not self.percent_overlap < 100.0:
                raise ValueError("percent_overlap must be below 100")
        return self


class StitchSettings(_StrictModel):
    """What ``estimate-stitch`` writes and ``stitch`` applies: ``total_translation[position] = [z, y, x]`` in voxels of the
    well's canvas (tile voxel ``i`` sits at ``i + t``), the blend (``csrc/stitch.hpp``: weight ``(dy dx)^blending_exponent``)
    and the fill value.  ``channels``: the channels to stitch (default: all)."""

    total_translation: dict[str, list[float]]
    blending_exponent: int = 1
    cval: float = 0.0
    channels: Optional[list[str]] = None

    @field_validator("total_translation")
    @classmethod
    def _check_translations(cls, v):
        if not v:
            raise ValueError("total_translation is empty")
        for key, t in v.items():
            if len(t) != 3 or not all(np.isfinite(float(x)) for x in t):
                raise ValueError(f"total_translation[{key!r}] must be three finite numbers (z, y, x), got {t}")
        return {k: [float(x) for x in t] for k, t in v.items()}

    @field_validator("blending_exponent")
    @classmethod
    def _check_exponent(cls, v):
        if not 0 <= v <= 4:
            raise ValueError("blending_exponent must be in 0 .. 4")
        return v


class EnhanceSettings(_StrictModel):
    """Ridge, sheet and blob filters on the eigenvalues of the Gaussian-smoothed Hessian (``shrimpy_amd/hessian.py``; the
    ``enhance`` command and ``SegmentSettings.enhance``).

    ``measure``: ``ridge`` (the strongest negative curvature: sheets, tubes and blobs), ``tube`` (Sato's tubeness), ``sheet``
    (a bright plate), ``blob`` (negative curvature in every direction), ``log`` (the scale-normalised Laplacian, bright
    positive), or an eigenvalue itself, ``e1 <= e2 <= e3``.  The response is the maximum over the scales given by exactly one
    of ``sigmas_um`` -- in the units of the position's scale (micrometres), blurred and differentiated at that scale -- and
    ``sigmas`` -- in voxels, on the voxel grid.  ``dark: true`` looks for dark structures on a bright background.  ``channels``
    names the channels the ``enhance`` command filters (the others are copied); ``segment`` ignores it."""

    channels: list[str] = []
    measure: Literal["e1", "e2", "e3", "ridge", "tube", "sheet", "blob", "log"]
    sigmas_um: Optional[list[PositiveFloat]] = None
    sigmas: Optional[list[PositiveFloat]] = None
    dark: bool = False

    @model_validator(mode="after")
    def _check_sigmas(self):
        if (self.sigmas_um is None) == (self.sigmas is None):
            raise ValueError("exactly one of sigmas_um and sigmas must be given")
        values = self.sigmas if self.sigmas_um is None else self.sigmas_um
        if not values:
            raise ValueError("sigmas is empty: no scale to filter at")
        if not all(np.isfinite(v) for v in values):
            raise ValueError("sigmas must be finite")
        return self

    def scales(self, sampling) -> tuple[list[float], tuple[float, float, float]]:
        """``(sigmas, sampling)`` for ``hessian.enhance``: ``sigmas_um`` at ``sampling``, ``sigmas`` on the voxel grid."""
        if self.sigmas_um is not None:
            return [float(v) for v in self.sigmas_um], tuple(float(s) for s in sampling)
        return [float(v) for v in self.sigmas], (1.0, 1.0, 1.0)


class PercentileThreshold(_StrictModel):
    """``threshold: {percentile: p}`` of :class:`SegmentSettings`: the ``p``-th percentile (numpy's ``linear`` rule, exact order
    statistics: ``shrimpy_amd/stats.py``) of what is thresholded, taken where ``otsu`` is taken.  ``99.5`` keeps the brightest
    0.5 %."""

    percentile: float

    @field_validator("percentile")
    @classmethod
    def _check_percentile(cls, v):
        if not 0.0 <= v <= 100.0:
            raise ValueError("percentile must lie in [0, 100]")
        return v


class SegmentSettings(_StrictModel):
    """Connected-component segmentation of one channel (``shrimpy_amd/segment.py``, the ``segment`` command).

    ``threshold``: a number, or ``"otsu"`` for the multi-Otsu threshold of the (blurred) volume -- ``sigma`` and
    ``otsu_component`` are those of ``dynatrack._gaussian_blur_3d`` and ``dynatrack._multiotsu_threshold``; with
    ``sigma > 0`` the blurred volume is what is thresholded, the table's intensities are always the input's.
    ``connectivity`` is 6, 18 or 26 (faces; faces and edges; faces, edges and corners).  The default, 6, is
    ``scipy.ndimage.label``'s default structure -- NOT skimage's: ``skimage.measure.label`` defaults to full
    connectivity, 26 in 3-D.  Objects of fewer than ``min_volume`` voxels are dropped and the rest renumbered
    ``1 .. M`` in their old order; ``keep_largest`` keeps the one object of greatest volume (ties: the lowest label).

    ``expand_distance`` (in the units of the position's scale: micrometres from the ``segment`` command) grows the labels
    that survive the filter into the background by at most that distance, without overlap (``skimage``'s ``expand_labels``
    rule on the exact Euclidean distance transform, ``shrimpy_amd/distance.py``); the table is then that of the grown labels.
    ``inscribed_radius`` adds a column of that name: per object the greatest distance from one of its voxels to the nearest
    background voxel, of the final labels (``inscribed_radius_um`` in ``objects.csv``).

    ``split`` splits touching objects after the labelling and before the size filter (``shrimpy_amd/watershed.py``): a
    watershed by steepest ascent of each object's depth map -- the exact Euclidean distance to the background, blurred by a
    Gaussian of ``split_sigma`` voxels -- whose basins are merged where the depth of the pass between them is at most
    ``split_min_depth`` (in the units of ``expand_distance``: micrometres from the ``segment`` command).  The merge depth, not
    the blur, is the knob that makes the result stable; no upstream is pinned for this step (its rule is the specification).
    ``min_volume`` and ``keep_largest`` then act on the split objects.

    ``background_radius`` (a number or ``[z, y, x]``, in the units of ``expand_distance``: micrometres from the ``segment``
    command) takes a slowly varying background away before anything else: the volume is replaced by its white top-hat under a
    box of that radius (``shrimpy_amd/morphology.py``; per axis ``floor(radius / scale + 0.5)`` voxels to each side), then
    blurred and thresholded -- a number, or the multi-Otsu value of what is thresholded.  The window has to be wider than
    the objects.  A component 0 means no window on that axis (``[0, r, r]`` works plane by plane); 0, the default, leaves the
    volume alone.  ``fill_holes`` fills the holes of the thresholded mask before it is labelled
    (``scipy.ndimage.binary_fill_holes``: background that no path of face neighbours joins to the border of the volume), for
    every ``connectivity``.  The table's intensities stay the input's.

    ``median_radius`` (a number or ``[z, y, x]``, the same units) replaces the volume by its median under a box of that radius
    (``shrimpy_amd/rank.py``; at most 3 voxels to each side) before all of the above: speckle and hot pixels go, edges and the
    contacts between objects stay where a Gaussian ``sigma`` would round them off.  0, the default, leaves the volume
    alone.

    ``enhance`` (an :class:`EnhanceSettings` without ``channels``) replaces what is thresholded by a ridge, sheet or blob
    response of the Hessian's eigenvalues (``shrimpy_amd/hessian.py``), after ``median_radius`` and ``background_radius`` and
    before ``sigma`` and the threshold: tubes, membranes and puncta that no threshold of the intensity separates from an
    uneven background.  ``threshold`` -- a number or ``otsu`` -- then applies to the response.  Unset, the default, nothing
    changes.

    ``shape`` measures the final labels' second moments, faces and contacts (``segment.shape_table``) and adds the axis
    lengths, the major axis, the staircase surface area, the contact area, the number of neighbours and ``touches_border`` to
    the table and to ``objects.csv``.  ``contacts`` makes the ``segment`` command write ``contacts.csv``: one row per pair of
    labels that share a face, with the shared faces per axis and their area.  Under connectivity 6 plain labels never share a
    face; split (``split``) and grown (``expand_distance``) labels do."""

    channel_name: str
    threshold: Union[float, Literal["otsu"], PercentileThreshold]
    median_radius: Union[NonNegativeFloat, tuple[NonNegativeFloat, NonNegativeFloat, NonNegativeFloat]] = 0.0
    background_radius: Union[NonNegativeFloat, tuple[NonNegativeFloat, NonNegativeFloat, NonNegativeFloat]] = 0.0
    enhance: Optional[EnhanceSettings] = None
    fill_holes: bool = False
    sigma: NonNegativeFloat = 0.0
    otsu_component: NonNegativeInt = 0
    connectivity: Literal[6, 18, 26] = 6
    min_volume: NonNegativeInt = 0
    keep_largest: bool = False
    inscribed_radius: bool = False
    expand_distance: NonNegativeFloat = 0.0
    split: bool = False
    split_sigma: NonNegativeFloat = 1.0
    split_min_depth: NonNegativeFloat = 0.0
    shape: bool = False
    contacts: bool = False

    @field_validator("threshold")
    @classmethod
    def _check_threshold(cls, v):
        if not isinstance(v, (str, PercentileThreshold)) and not np.isfinite(float(v)):
            raise ValueError("threshold must be a finite number, \"otsu\" or {percentile: p}")
        return v

    @field_validator("background_radius")
    @classmethod
    def _check_background_radius(cls, v):
        if not all(np.isfinite(float(r)) for r in (v if isinstance(v, tuple) else (v,))):
            raise ValueError("background_radius must be finite")
        return v

    @field_validator("median_radius")
    @classmethod
    def _check_median_radius(cls, v):
        if not all(np.isfinite(float(r)) for r in (v if isinstance(v, tuple) else (v,))):
            raise ValueError("median_radius must be finite")
        return v


class BackgroundSettings(_StrictModel):
    """Top-hat background subtraction of whole channels (``shrimpy_amd/morphology.py``, the ``subtract-background`` command).

    Every volume of the channels ``channel_names`` is replaced by its top-hat under a box of ``radius`` -- a number or
    ``[z, y, x]`` in the units of the position's scale (micrometres), per axis ``floor(radius / scale + 0.5)`` voxels to each
    side, a component 0 meaning no window on that axis.  ``op`` ``"white_tophat"`` (``v - opening(v)``) keeps bright
    structures narrower than the window, ``"black_tophat"`` (``closing(v) - v``) dark ones.  The other channels are copied."""

    channel_names: list[str]
    radius: Union[NonNegativeFloat, tuple[NonNegativeFloat, NonNegativeFloat, NonNegativeFloat]]
    op: Literal["white_tophat", "black_tophat"] = "white_tophat"

    @field_validator("channel_names")
    @classmethod
    def _check_channels(cls, v):
        if not v:
            raise ValueError("channel_names is empty: nothing to subtract a background from")
        return v

    @field_validator("radius")
    @classmethod
    def _check_radius(cls, v):
        values = v if isinstance(v, tuple) else (v,)
        if not all(np.isfinite(float(r)) for r in values) or not any(float(r) > 0 for r in values):
            raise ValueError("radius must be finite and positive on at least one axis")
        return v


class DespeckleSettings(_StrictModel):
    """Median, percentile and outlier-removal filtering of whole channels (``shrimpy_amd/rank.py``, the ``despeckle`` command).

    Every volume of the channels ``channel_names`` is filtered under a box given by exactly one of ``radius`` -- a number or
    ``[z, y, x]`` in the units of the position's scale (micrometres), per axis ``floor(radius / scale + 0.5)`` voxels to each
    side -- and ``half_widths`` -- ``[z, y, x]`` in voxels (hot pixels of a raw stack: ``[0, 1, 1]``); a component 0 means no
    window on that axis, and a half-width is at most 3.  ``op``: ``"median"`` replaces every voxel by the median of its box;
    ``"remove_bright"`` (the default), ``"remove_dark"`` and ``"remove_both"`` replace only the voxels that stand out from that
    median by more than ``threshold`` (``v - m > threshold``, ``m - v > threshold``, either) and leave every other voxel as it
    is -- ImageJ's "Remove Outliers"; ``threshold`` is required for them.  With ``percentile`` set (``op`` must be ``"median"``)
    the filter is that percentile of the box instead (``scipy.ndimage.percentile_filter``'s convention).  The other channels
    are copied."""

    channel_names: list[str]
    radius: Optional[Union[NonNegativeFloat, tuple[NonNegativeFloat, NonNegativeFloat, NonNegativeFloat]]] = None
    half_widths: Optional[tuple[NonNegativeInt, NonNegativeInt, NonNegativeInt]] = None
    op: Literal["median", "remove_bright", "remove_dark", "remove_both"] = "remove_bright"
    threshold: Optional[NonNegativeFloat] = None
    percentile: Optional[float] = None

    @field_validator("channel_names")
    @classmethod
    def _check_channels(cls, v):
        if not v:
            raise ValueError("channel_names is empty: nothing to filter")
        return v

    @model_validator(mode="after")
    def _check_consistency(self):
        if (self.radius is None) == (self.half_widths is None):
            raise ValueError("exactly one of radius and half_widths must be given")
        values = self.half_widths if self.radius is None else (self.radius if isinstance(self.radius, tuple) else (self.radius,))
        if not all(np.isfinite(float(r)) for r in values) or not any(float(r) > 0 for r in values):
            raise ValueError("radius / half_widths must be finite and positive on at least one axis")
        if self.op == "median":
            if self.threshold is not None:
                raise ValueError("threshold has no meaning for op: median")
        elif self.threshold is None or not np.isfinite(self.threshold):
            raise ValueError(f"op: {self.op} needs a finite threshold >= 0")
        if self.percentile is not None:
            if self.op != "median":
                raise ValueError("percentile is set: op must be median")
            if not -100.0 <= self.percentile <= 100.0:           # (a NaN too)
                raise ValueError("percentile must be in -100 .. 100")
        return self


class TrackSettings(_StrictModel):
    """Tracking the objects of a label channel over time (``shrimpy_amd/track.py``, the ``track`` command).

    ``channel_name`` is the label channel (``<name>_labels`` from the ``segment`` command).  An object of frame ``t + 1`` is
    linked to the object of frame ``t`` it shares the most voxels with, among those that share at least ``min_overlap_voxels``
    and whose intersection over union is at least ``min_iou``.  With ``divisions`` an object with two or more successors ends
    and each successor starts a track that names it as its parent (the convention of the Cell Tracking Challenge); without,
    the successor with the greatest overlap continues the track and the others start unrelated ones.  No upstream is pinned
    for the linking rule (biahub's ``track`` runs ultrack); gap closing is not built."""

    channel_name: str
    min_overlap_voxels: PositiveInt = 1
    min_iou: float = 0.0
    divisions: bool = True

    @field_validator("min_iou")
    @classmethod
    def _check_min_iou(cls, v):
        if not 0.0 <= v <= 1.0:
            raise ValueError("min_iou must be in 0 .. 1")
        return v


class MeasureSettings(_StrictModel):
    """Measuring the objects of a label store in the channels of another store (``segment.intensity_table``, the ``measure``
    command).

    ``label_channel_name`` is the channel of the label store (``<name>_labels`` from ``segment``, ``<name>_tracks`` from
    ``track``, or any integer channel).  ``channels`` names the channels of the intensity store that are measured, in the order
    of the columns; ``None`` takes every channel in store order.  With ``background_distance > 0`` (micrometres, the position's
    scale) every object is also measured in a ring of local background: the voxels farther than ``background_gap`` from the
    object and within ``background_gap + background_distance`` of it, nearer to it than to any other object
    (``segment.shell_labels``)."""

    label_channel_name: str
    channels: Optional[list[str]] = None
    background_distance: NonNegativeFloat = 0.0
    background_gap: NonNegativeFloat = 0.0

    @field_validator("channels")
    @classmethod
    def _check_channels(cls, v):
        if v is not None and (len(v) == 0 or len(set(v)) != len(v)):
            raise ValueError("channels must name at least one channel, each once (or be null: every channel)")
        return v

    @field_validator("background_distance", "background_gap")
    @classmethod
    def _check_finite(cls, v):
        if not np.isfinite(v):
            raise ValueError("must be finite")
        return v


class ColocalizeSettings(_StrictModel):
    """Colocalization of pairs of channels, per labelled object and per volume (``colocalize.pair_table``, the ``colocalize``
    command).

    ``pairs`` names the pairs ``[a, b]`` of channels of the intensity store, in the order of the columns: at least one, the two
    names of a pair differ, each pair once.  ``label_channel_name`` is the channel of the label store (needed when the command
    is given one).  ``thresholds`` is ``[ta, tb]`` -- a voxel counts as signal in a channel where it is strictly above -- or
    ``"costes"``: Costes' automatic thresholds (``colocalize.costes_thresholds``) per (position, t, pair), over
    ``costes_region``: the whole ``volume`` or the ``labelled`` voxels."""

    pairs: list[list[str]]
    label_channel_name: Optional[str] = None
    thresholds: Union[list[float], Literal["costes"]] = [0.0, 0.0]
    costes_region: Literal["volume", "labelled"] = "volume"

    @field_validator("pairs")
    @classmethod
    def _check_pairs(cls, v):
        if len(v) == 0:
            raise ValueError("pairs must name at least one pair of channels")
        for pair in v:
            if len(pair) != 2 or pair[0] == pair[1]:
                raise ValueError(f"a pair is two different channel names, got {pair!r}")
        if len({tuple(pair) for pair in v}) != len(v):
            raise ValueError("each pair must be named once")
        return v

    @field_validator("thresholds")
    @classmethod
    def _check_thresholds(cls, v):
        if v != "costes" and (len(v) != 2 or any(np.isnan(t) for t in v)):
            raise ValueError("thresholds must be [ta, tb] (two numbers, not NaN) or \"costes\"")
        return v


class StatisticsSettings(_StrictModel):
    """Whole-volume statistics of a store (``shrimpy_amd/stats.py``, the ``statistics`` command).

    ``channel_names``: the channels measured, empty for all.  ``quantiles``: in [0, 1]; 0.25, 0.5 and 0.75 are always added
    (``median`` and ``iqr`` need them).  ``levels``: ``volume`` (one row per (t, channel) in ``statistics.csv``), ``position``
    (pooled over t) and ``dataset`` (pooled over every selected position and t); the last two read the store once more per
    pass."""

    channel_names: list[str] = []
    quantiles: list[float] = [0.001, 0.01, 0.25, 0.5, 0.75, 0.99, 0.999]
    levels: list[Literal["volume", "position", "dataset"]] = ["volume"]

    @field_validator("quantiles")
    @classmethod
    def _check_quantiles(cls, v):
        if any(not 0.0 <= q <= 1.0 for q in v):
            raise ValueError("quantiles must lie in [0, 1]")
        return v

    @field_validator("levels")
    @classmethod
    def _check_levels(cls, v):
        if not v or len(set(v)) != len(v):
            raise ValueError("levels must name at least one of volume, position, dataset, each once")
        return v

    def all_quantiles(self) -> list[float]:
        return sorted({float(q) for q in self.quantiles} | {0.25, 0.5, 0.75})


class NormalizeSettings(_StrictModel):
    """Intensity normalization of whole channels (``shrimpy_amd/stats.py``, the ``normalize`` command): every volume of the
    channels ``channel_names`` becomes ``(v - sub) / div`` in float32, the other channels are copied.

    ``method``: ``percentile`` (``sub`` = the ``lower_percentile``-th percentile, ``div`` = the ``upper_percentile``-th minus
    it; with ``clip`` the result is clamped to [0, 1]), ``zscore`` (mean and standard deviation) or ``robust`` (median and
    interquartile range).  ``level``: ``volume`` takes each volume's own statistics -- per timepoint this is the bleach
    correction --; ``position`` and ``dataset`` read them from the ``statistics.json`` the ``statistics`` command wrote into
    ``statistics_dirpath``.  A divisor that is 0 or not finite becomes 1 and the unit is reported as degenerate."""

    channel_names: list[str]
    method: Literal["percentile", "zscore", "robust"] = "percentile"
    lower_percentile: float = 1.0
    upper_percentile: float = 99.9
    clip: bool = False
    level: Literal["volume", "position", "dataset"] = "volume"
    statistics_dirpath: Optional[str] = None

    @field_validator("channel_names")
    @classmethod
    def _check_channels(cls, v):
        if not v or len(set(v)) != len(v):
            raise ValueError("channel_names must name at least one channel, each once")
        return v

    @model_validator(mode="after")
    def _check(self):
        if not 0.0 <= self.lower_percentile < self.upper_percentile <= 100.0:
            raise ValueError("0 <= lower_percentile < upper_percentile <= 100")
        if self.clip and self.method != "percentile":
            raise ValueError("clip goes with method: percentile (it clamps to [0, 1])")
        if self.level != "volume" and not self.statistics_dirpath:
            raise ValueError(f"level: {self.level} reads statistics.json: statistics_dirpath is required")
        return self


class ReconstructSettings(_StrictModel):
    """Whole per-volume pipeline: (flat-field) -> deskew -> (register) -> (deconvolve)."""

    flatfield: bool = False  # bright-field only: divide out the per-pixel median over Z (reference
    #                          ``RECON_STEPS[0]``, ``shrimpy/preprocessing.py:320-327``)
    deskew: Optional[DeskewSettings] = None
    registration: Optional[RegisterSettings] = None
    deconvolution: Optional[DeconvolveSettings] = None
