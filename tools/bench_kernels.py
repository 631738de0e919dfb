"""Per-kernel timings that bench.py does not cover: affine apply (BASELINE config 3), the dense-PSF
RL launch, and the deskew kernel alone.  Prints one JSON object per kernel.

    python tools/bench_kernels.py [--reps 5]
"""

from __future__ import annotations

import argparse
import ctypes
import json
import sys

from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def timed(fn, reps):
    import torch

    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-dense", action="store_true")
    ap.add_argument("--only-rl", action="store_true", help="skip the affine and deskew sections")
    ap.add_argument("--only-affine", action="store_true", help="only the affine apply section")
    ap.add_argument("--rl-grid", default="171,2048,2270", help="Z,Y,X of the RL launch section")
    ap.add_argument("--psf-sweep", action="store_true", help="only: ms per RL iteration over separable PSF sizes")
    ap.add_argument("--rl-fft", action="store_true", help="only: ms per RL iteration in the Fourier domain (dense PSFs "
                    "beyond the stencil kernels) next to the generic / dense stencils where they exist")
    ap.add_argument("--rl-tv", action="store_true", help="only: ms per total-variation launch and per RL-TV iteration (fused "
                    "separable 9x7x7) beside the plain fused iteration, on --rl-grid")
    ap.add_argument("--rl-accel", action="store_true", help="only: ms per launch of the Biggs-Andrews extrapolation, per "
                    "accelerated iteration and the wall time of 9 / 10 / 15 accelerated beside 20 plain iterations on the "
                    "fused separable, ky (x) kzx and Fourier routes, on --rl-grid")
    ap.add_argument("--peaks", action="store_true", help="only: ms of the bead-detection launches (csrc/peaks.hip) at "
                    "min_distance 5, 10, 25 and 50 and of the box smoothing in front of them, on --rl-grid")
    ap.add_argument("--peaks-host", action="store_true", help="with --peaks: also time scipy.ndimage.maximum_filter for "
                    "the same windows on this box's host cores")
    ap.add_argument("--phase", action="store_true", help="only: one application of the phase reconstruction (yaml optics) on "
                    "--rl-grid, per launch and in total, the warm-up (host transfer function) time, and one Fourier-domain RL "
                    "convolution on the same volume as the yardstick; appended to profiles/phase_config2.jsonl")
    ap.add_argument("--pyramid", action="store_true", help="only: ms of lsr_downsample2_f32 for pyramid levels 1-3 of "
                    "--rl-grid (fz = 2) beside torch's avg_pool3d on the same tensor and a device-to-device copy in the same "
                    "run (median of --reps launches between HIP events, after a warm-up); appended to "
                    "profiles/pyramid_config2.jsonl")
    ap.add_argument("--stitch", action="store_true", help="only: ms of lsr_stitch_f32 for a 2 x 2 grid of --rl-grid tiles at "
                    "10 % overlap (p = 1; integer placement, then a placement fractional on x) beside the torch scatter "
                    "formulation and a device-to-device copy in the same run (median of 5 launches between HIP events after "
                    "2 warm-ups); appended to profiles/stitch_config2.jsonl")
    ap.add_argument("--label", action="store_true", help="only: ms per launch of the labelling (csrc/label.hip: local, merge, "
                    "flatten, count, scan, rank, final; HIP events between the launches, median of --reps calls after a warm-up), "
                    "of the object table and of the relabelling on --rl-grid, for bench.synthetic_raw at its multi-Otsu "
                    "threshold, Bernoulli noise at p = 0.3 (connectivity 6) and an all-foreground volume, beside a device copy "
                    "and scipy.ndimage.label on this box's host at --label-host-grid; appended to profiles/label_config2.jsonl")
    ap.add_argument("--label-host-grid", default="43,512,568", help="Z,Y,X of the scipy.ndimage.label timing of --label")
    ap.add_argument("--watershed", action="store_true", help="only: ms per launch of the watershed (csrc/watershed.hip: local, merge, "
                    "flatten, count, scan, rank, final; HIP events between the launches, median of 3 calls after a warm-up) and of "
                    "the saddle pass on --rl-grid, for the three scenes of --label -- the objects are the labelling's, the surface "
                    "their depth map blurred with sigma 1 -- beside the labelling's seven launches on the same scene and a device "
                    "copy in the same run; appended to profiles/watershed_config2.jsonl")
    ap.add_argument("--overlap", action="store_true", help="only: ms of the label-overlap kernel (csrc/overlap.hip) on --rl-grid for "
                    "the three scenes of --label, each taken as two frames (the second the first rolled by 2 voxels in x), over a "
                    "sweep of the grid cap (HIP events, median of 3 calls after a warm-up), beside a device copy of one int32 "
                    "volume and torch.unique of the packed pairs in the same run, with the global atomics per scene estimated "
                    "from a sample of the workgroups' spans; appended to profiles/overlap_config2.jsonl")
    ap.add_argument("--moments", action="store_true", help="only: ms of the label-moment kernel (csrc/moments.hip) on --rl-grid for "
                    "the three scenes of --label: as shipped, over a sweep of LDS slots and grid caps, and in the plain form without "
                    "an LDS table, beside a device copy, lsr_label_regions_f32 without intensities and the three overlap launches of "
                    "segment.contact_table in the same run; appended to profiles/moments_config2.jsonl")
    ap.add_argument("--intensity", action="store_true", help="only: ms of the label-intensity kernel (csrc/intensity.hip) on --rl-grid "
                    "for the three scenes of --label with the scene as the values: as shipped for float32 and uint16 values, over a "
                    "sweep of LDS slots, grid caps and probe bounds, and in the plain form without an LDS table, beside a device "
                    "copy of one int32 and one float32 volume and lsr_label_regions_f32 with the intensities in the same run; "
                    "appended to profiles/intensity_config2.jsonl")
    ap.add_argument("--coloc", action="store_true", help="only: ms of the colocalization kernel (csrc/coloc.hip) on --rl-grid for the "
                    "three scenes of --label, float32 and uint16 channels, with and without labels; the sweep of LDS slots, grid "
                    "caps and probe bounds and the plain form; beside a device copy of the three volumes and two launches of the "
                    "label-intensity kernel; lines appended to profiles/coloc_config2.jsonl")
    ap.add_argument("--stats", action="store_true", help="only: ms of one digit pass of the whole-volume select (csrc/stats.hip) on "
                    "--rl-grid in both forms (runs reduced inside the wave, one LDS add per voxel), passes 0 and 1, over a sweep of "
                    "the grid cap, float32 and uint16, and of stats.summary end to end, on the bench's bead scene, Bernoulli noise, "
                    "an all-zero volume and the bead scene with its outer quarter set to 0 (HIP events, median of 3 calls after a "
                    "warm-up), beside a device copy of the volume, the rescale kernel, and what torch.quantile and torch.sort do "
                    "on the full volume and on the largest crop they accept; appended to profiles/stats_config2.jsonl")
    ap.add_argument("--coloc-crop", default="1,1024,1024", help="Z,Y,X of the small crop --coloc also times the kernel on")
    ap.add_argument("--edt", action="store_true", help="only: ms per launch of the distance transform (csrc/edt.hip: x, y, z; HIP "
                    "events between the launches, median of 5 calls after a warm-up) on --rl-grid, for bench.synthetic_raw at its "
                    "multi-Otsu threshold, Bernoulli noise at p = 0.3 and an all-foreground volume with one background voxel, "
                    "beside a device copy of an int32 volume in the same run; appended to profiles/edt_config2.jsonl")
    ap.add_argument("--morphology", action="store_true", help="only: ms of the grey-morphology kernels (csrc/morphology.hip: erosion, "
                    "opening, white top-hat) on --rl-grid for the bench's bead scene at half-widths 5, 25, 50 and 128 (HIP events, "
                    "median of 3 calls after a warm-up), beside a device copy of one volume and the three launches of "
                    "lsr_local_max_candidates_f32 at the same half-width (up to 64) in the same run; appended to "
                    "profiles/morphology_config2.jsonl")
    ap.add_argument("--rank", action="store_true", help="only: ms of the rank-filter kernel (csrc/rank.hip) on --rl-grid for the "
                    "bench's bead scene: the median at half-widths (0, 1, 1), (1, 1, 1), (2, 2, 2) and (3, 3, 3), the first two "
                    "again on the generic path (variant = 1), and remove_bright at (0, 1, 1) (HIP events, median of 3 calls after a "
                    "warm-up), beside a device copy of one volume and grey_erosion at the same half-widths in the same run; "
                    "appended to profiles/rank_config2.jsonl")
    ap.add_argument("--hessian", action="store_true", help="only: ms of the Hessian-eigenvalue kernel (csrc/hessian.hip) on --rl-grid "
                    "for the bench's bead scene blurred at sigma 1.5: e1, tube and log with and without accumulate, the three blur "
                    "launches of one scale, enhance at three sigmas end to end (HIP events, median of 3 calls after a warm-up), "
                    "beside a device copy of one volume, the torch fallback (torch.gradient + torch.linalg.eigvalsh) on a shape it "
                    "fits in memory, and the worst eigenvalue error against numpy on a crop; appended to "
                    "profiles/hessian_config2.jsonl")
    ap.add_argument("--flatfield", action="store_true", help="only: ms of the flat-field median (csrc/flatfield.hip, + mean) on the "
                    "config-2 raw shape for its three variants -- integer counts as float32, float values, uint16 counts --, each "
                    "timed --flatfield-repeats times (a repetition: the mean of --reps calls between HIP events after a warm-up), "
                    "so that the spread between repetitions stands beside a before/after difference; appended with --tag to "
                    "profiles/flatfield_pin.jsonl")
    ap.add_argument("--flatfield-repeats", type=int, default=5)
    ap.add_argument("--tag", default="", help="with --flatfield: what the lines are tagged with (the commit measured)")
    ap.add_argument("--mi", action="store_true", help="only: ms per launch of the mutual-information kernels (csrc/estimate_mi.hip: "
                    "joint histogram, gradient) on --mi-grid at strides 1 and 4, 32 and 64 bins, on bench.synthetic_raw "
                    "(background-dominated) and on uniform noise (spread over all cells), beside a torch formulation "
                    "(grid_sample + bincount) and a device copy of the two volumes in the same run (median of 5 launches "
                    "between HIP events after 2 warm-ups); appended to profiles/mi_config3.jsonl")
    ap.add_argument("--mi-grid", default="256,2048,2048", help="Z,Y,X of the --mi section (BASELINE config 3)")
    ap.add_argument("--psf-fit", action="store_true", help="only: ms of lsr_bead_fit_f32 and of lsr_psf_accumulate_shifted_f32 for "
                    "500 and 2000 beads at patches 15x19x19 and 31x37x19 (median of --reps launches between HIP events after a "
                    "warm-up), and the wall time of their host twins on --host-threads threads; appended to "
                    "profiles/psf_fit.jsonl")
    ap.add_argument("--host-threads", type=int, default=16, help="threads of the host twins in the --psf-fit section")
    ap.add_argument("--psf-sweep-wide", action="store_true", help="with --psf-sweep: every pz for in-plane extents 9-15")
    args = ap.parse_args()

    import torch

    import bench
    from shrimpy_amd.deconvolve import RichardsonLucyPlan
    from shrimpy_amd.deskew import deskew_with_matrix
    from shrimpy_amd.geometry import deskew_geometry
    from shrimpy_amd.register import apply_affine_transform_zyx

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(3)

    if args.psf_fit:
        _psf_fit(args, torch, dev)
        return
    if args.flatfield:
        _flatfield(args, torch, dev, g, bench)
        return
    if args.mi:
        _mi(args, torch, dev, g, bench, tuple(int(v) for v in args.mi_grid.split(",")))
        return
    if args.overlap:
        _overlap(args, torch, dev, g, bench, tuple(int(v) for v in args.rl_grid.split(",")))
        return
    if args.moments:
        _moments(args, torch, dev, g, bench, tuple(int(v) for v in args.rl_grid.split(",")))
        return
    if args.intensity:
        _intensity(args, torch, dev, g, bench, tuple(int(v) for v in args.rl_grid.split(",")))
        return
    if args.stats:
        _stats(args, torch, dev, g, bench, tuple(int(v) for v in args.rl_grid.split(",")))
        return
    if args.coloc:
        _coloc(args, torch, dev, g, bench, tuple(int(v) for v in args.rl_grid.split(",")))
        return
    if args.watershed:
        _watershed(args, torch, dev, g, bench, tuple(int(v) for v in args.rl_grid.split(",")))
        return
    if args.edt:
        _edt(args, torch, dev, g, bench, tuple(int(v) for v in args.rl_grid.split(",")))
        return
    if args.hessian:
        _hessian(args, torch, dev, g, bench, tuple(int(v) for v in args.rl_grid.split(",")))
        return
    if args.rank:
        _rank(args, torch, dev, g, bench, tuple(int(v) for v in args.rl_grid.split(",")))
        return
    if args.morphology:
        _morphology(args, torch, dev, g, bench, tuple(int(v) for v in args.rl_grid.split(",")))
        return
    if args.label:
        _label(args, torch, dev, g, bench, tuple(int(v) for v in args.rl_grid.split(",")))
        return
    if args.stitch:
        _stitch(args, torch, dev, g, tuple(int(v) for v in args.rl_grid.split(",")))
        return
    if args.pyramid:
        _pyramid(args, torch, dev, g, tuple(int(v) for v in args.rl_grid.split(",")))
        return
    if args.phase:
        _phase(args, torch, dev, g, tuple(int(v) for v in args.rl_grid.split(",")))
        return
    if args.peaks:
        _peaks(args, torch, dev, g, tuple(int(v) for v in args.rl_grid.split(",")))
        return
    if args.rl_fft:
        _rl_fft(args, torch, dev, g, tuple(int(v) for v in args.rl_grid.split(",")))
        return
    if args.rl_tv:
        _rl_tv(args, torch, dev, g, bench, RichardsonLucyPlan, tuple(int(v) for v in args.rl_grid.split(",")))
        return
    if args.rl_accel:
        _rl_accel(args, torch, dev, g, tuple(int(v) for v in args.rl_grid.split(",")))
        return
    if args.psf_sweep:
        _psf_sweep(args, torch, dev, g, RichardsonLucyPlan, tuple(int(v) for v in args.rl_grid.split(",")))
        return
    if not args.only_rl:
        _affine_and_deskew(args, torch, dev, g, bench, deskew_with_matrix, deskew_geometry, apply_affine_transform_zyx)

    if args.only_affine:
        return
    # ---- RL launches on the config-2 grid: separable (tuned) and dense
    oshape = tuple(int(v) for v in args.rl_grid.split(","))
    if not args.only_rl:
        _estimators(args, torch, dev, g, oshape)
    _rl(args, torch, dev, g, bench, RichardsonLucyPlan, oshape)


def _affine_and_deskew(args, torch, dev, g, bench, deskew_with_matrix, deskew_geometry, apply_affine_transform_zyx):
    # ---- affine apply, config 3: 2048 x 2048 x 256 volume, rotation 2 deg o scale o translation
    shape = (256, 2048, 2048)
    vol = torch.rand(shape, device=dev, generator=g) * 1000
    out = torch.empty_like(vol)
    th = np.deg2rad(2.0)
    rot = np.array([[1, 0, 0], [0, np.cos(th), -np.sin(th)], [0, np.sin(th), np.cos(th)]])
    m = np.eye(4)
    m[:3, :3] = rot @ np.diag([1.0, 0.98, 1.02])
    m[:3, 3] = [3.5, -12.25, 20.75]
    for mode, exact in (("constant", True), ("grid-constant", True), ("constant", False)):
        ms = timed(lambda: apply_affine_transform_zyx(vol, m, mode=mode, out=out, exact=exact), args.reps)
        nbytes = 8.0 * vol.numel()
        print(json.dumps({"kernel": f"affine_kernel ({mode}, {'exact fp64' if exact else 'f32 interp'})", "shape": shape, "ms": ms,
                          "algorithmic_GBps": nbytes / ms / 1e6, "frac_of_8TBps": nbytes / ms / 1e6 / 8000,
                          "voxels_per_s": vol.numel() / (ms * 1e-3)}))
    # maps that couple z with the plane: (a) tilt 1.5 deg about y; (b) the config-3 registration with
    # a 3 deg tilt about y on top (the oblique light-sheet <-> label-free case) -- affine_box.hip;
    # the same maps in grid-constant mode take the general gather kernel (the old path)
    from shrimpy_amd import _lib
    from shrimpy_amd.geometry import as_matrix_3x4

    tilt = np.eye(4)
    c, sn = np.cos(np.deg2rad(1.5)), np.sin(np.deg2rad(1.5))
    tilt[0, 0], tilt[0, 2], tilt[2, 0], tilt[2, 2] = c, -sn, sn, c
    tilt[:3, 3] = [2.0, 0.5, -3.25]
    c3, s3 = np.cos(np.deg2rad(3.0)), np.sin(np.deg2rad(3.0))
    ry = np.array([[c3, 0, -s3], [0, 1, 0], [s3, 0, c3]])
    both = m.copy()
    both[:3, :3] = ry @ m[:3, :3]
    for name, mat in (("tilt 1.5deg about y", tilt), ("config3 o tilt 3deg about y", both)):
        for mode, exact in (("constant", True), ("constant", False), ("grid-constant", True)):
            path = _lib.call_value("lsr_affine_path", shape[0], shape[1], shape[2],
                                   _lib.matrix12(as_matrix_3x4(mat)), _lib.MODE_CONSTANT if mode == "constant" else _lib.MODE_GRID_CONSTANT)
            ms = timed(lambda: apply_affine_transform_zyx(vol, mat, mode=mode, out=out, exact=exact), args.reps)
            nbytes = 8.0 * vol.numel()
            print(json.dumps({"kernel": f"affine ({name}, {mode}, {'exact fp64' if exact else 'f32 interp'})",
                              "path": {0: "gather", 1: "planar", 2: "box"}[path],
                              "shape": shape, "ms": ms, "algorithmic_GBps": nbytes / ms / 1e6,
                              "frac_of_8TBps": nbytes / ms / 1e6 / 8000}))
    del vol, out
    if args.only_affine:
        return

    # ---- flat-field (median over Z + apply / fused deskew), config 2 raw stack of camera counts
    from shrimpy_amd.flatfield import flat_field_pattern

    raw_shape = bench.WORKLOADS["config2"][1]
    raw = torch.randint(80, 600, raw_shape, device=dev, generator=g).to(torch.float32)
    ms = timed(lambda: flat_field_pattern(raw), args.reps)             # camera counts: 2 passes
    print(json.dumps({"kernel": "flat_median_kernel (+ mean), integer counts", "raw": raw_shape, "ms": ms,
                      "passes_GBps": 2 * 4.0 * raw.numel() / ms / 1e6,
                      "frac_of_8TBps_at_2_passes": 2 * 4.0 * raw.numel() / ms / 1e6 / 8000}))
    raw += torch.rand(raw_shape, device=dev, generator=g)              # continuous values: 4 passes
    ms = timed(lambda: flat_field_pattern(raw), args.reps)
    print(json.dumps({"kernel": "flat_median_kernel (+ mean), float values", "raw": raw_shape, "ms": ms,
                      "passes_GBps": 4 * 4.0 * raw.numel() / ms / 1e6,
                      "frac_of_8TBps_at_4_passes": 4 * 4.0 * raw.numel() / ms / 1e6 / 8000}))
    ff = flat_field_pattern(raw)
    dst = torch.empty_like(raw)
    ms = timed(lambda: ff.apply(raw, out=dst), args.reps)
    print(json.dumps({"kernel": "flat_apply_kernel", "raw": raw_shape, "ms": ms,
                      "algorithmic_GBps": 8.0 * raw.numel() / ms / 1e6,
                      "frac_of_8TBps": 8.0 * raw.numel() / ms / 1e6 / 8000}))
    del dst
    geo = deskew_geometry(raw_shape, **bench.DESKEW)
    dsk = torch.empty(geo.output_shape, device=dev)
    for name, kw in (("deskew_kernel<false>, dense output rows", {}), ("deskew_kernel<true> (flat-field fused), dense output rows", {"flat_field": ff})):
        ms = timed(lambda: deskew_with_matrix(raw, geo.matrix_3x4, geo.pre_average_shape, 3, out=dsk, **kw), args.reps)
        print(json.dumps({"kernel": name, "raw": raw_shape, "ms": ms}))
    raw16 = raw.to(torch.uint16)
    ms = timed(lambda: deskew_with_matrix(raw16, geo.matrix_3x4, geo.pre_average_shape, 3, out=dsk), args.reps)
    print(json.dumps({"kernel": "deskew_kernel<false, U16> (uint16 camera counts in)", "raw": raw_shape, "ms": ms,
                      "algorithmic_GBps": (2.0 * raw16.numel() + 4.0 * dsk.numel()) / ms / 1e6}))
    ms = timed(lambda: flat_field_pattern(raw16), args.reps)
    print(json.dumps({"kernel": "flat_median_kernel<U16> (+ mean)", "raw": raw_shape, "ms": ms,
                      "passes_GBps": 2 * 2.0 * raw16.numel() / ms / 1e6}))
    ff16 = flat_field_pattern(raw16)
    ms = timed(lambda: deskew_with_matrix(raw16, geo.matrix_3x4, geo.pre_average_shape, 3, out=dsk, flat_field=ff16),
               args.reps)
    print(json.dumps({"kernel": "deskew_kernel<true, U16> (flat-field fused, uint16 in)", "raw": raw_shape, "ms": ms}))
    del raw, raw16, dsk, ff, ff16

    # ---- deskew alone, config 2 and config 4 mappings
    for name in ("config2", "config4"):
        raw_shape = bench.WORKLOADS[name][1]
        raw = torch.rand(raw_shape, device=dev, generator=g)
        geo = deskew_geometry(raw_shape, **bench.DESKEW)
        dst = torch.empty(geo.output_shape, device=dev)
        nbytes = 4.0 * raw.numel() + 4.0 * dst.numel()
        for border in ("constant", "grid-constant"):
            ms = timed(lambda: deskew_with_matrix(raw, geo.matrix_3x4, geo.pre_average_shape, 3, out=dst, border=border),
                       args.reps)
            # (dense output: rows of Xo floats, 2270 at config 2 -- not a multiple of four, so the stores of a tile row
            # straddle 16-byte boundaries; bench.py's step writes the RL plan's padded, line-aligned volume: 2.3 ms)
            print(json.dumps({"kernel": "deskew_kernel, dense output rows" + ("" if border == "constant" else " (border grid-constant)"),
                              "workload": name, "raw": raw_shape,
                              "out": geo.output_shape, "ms": ms, "algorithmic_GBps": nbytes / ms / 1e6,
                              "frac_of_8TBps": nbytes / ms / 1e6 / 8000}))
        del raw, dst


def _estimators(args, torch, dev, g, oshape):
    """DynaTrack estimators on a deskewed-size volume."""
    from shrimpy_amd import dynatrack as d

    vol = torch.rand(oshape, device=dev, generator=g) * 900 + 100
    n = vol.numel()
    for name, fn, passes in (
        ("_percentile (minmax + histogram)", lambda: d._percentile(vol, 90.0), 2),
        ("_intensity_center_of_mass", lambda: d._intensity_center_of_mass(vol, 150.0), 1),
        ("_gaussian_blur_3d sigma=2 (3 passes, 17 taps)", lambda: d._gaussian_blur_3d(vol, 2.0), 6),
        ("_gaussian_blur_3d sigma=5 (3 passes, 41 taps)", lambda: d._gaussian_blur_3d(vol, 5.0), 6),
        ("_multiotsu_center_of_mass sigma=2 (two volumes)", lambda: d._multiotsu_center_of_mass(vol, vol, 2.0), 20),
    ):
        ms = timed(fn, max(1, args.reps // 2))
        print(json.dumps({"kernel": name, "grid": oshape, "ms": ms, "volume_traversals": passes,
                          "traversal_GBps": passes * 4.0 * n / ms / 1e6}))
    # the reference's default tracker (dynatrack_demo.yaml:107): phase cross-correlation
    mov = torch.roll(vol, shifts=(2, -5, 7), dims=(0, 1, 2))
    shift = d._phase_cross_corr(vol, mov)
    assert shift in ((2, -5, 7), (-2, 5, -7)), shift
    from shrimpy_amd import fft3

    for route, ok in (("x and z legs in this package's kernels, rocFFT along y (fft3.correlation_peak)", True),
                      ("torch.fft.rfftn / irfftn", False)):
        if ok and not fft3.available():
            continue
        d._axis_fft_ok[0] = ok
        d.set_spectrum_cache_bytes(0)
        assert d._phase_cross_corr(vol, mov) == shift
        ms = timed(lambda: d._phase_cross_corr(vol, mov), max(1, args.reps // 2))
        print(json.dumps({"kernel": f"_phase_cross_corr (2 forward + 1 inverse 3-D FFT; {route})", "grid": oshape, "ms": ms,
                          "rolled_by": [2, -5, 7], "found": list(shift)}))
        d.set_spectrum_cache_bytes(8 << 30)
        ms = timed(lambda: d._phase_cross_corr(vol, mov), max(1, args.reps // 2))
        print(json.dumps({"kernel": f"_phase_cross_corr, reference spectrum cached (1 forward + 1 inverse; {route})",
                          "grid": oshape, "ms": ms}))
    d._axis_fft_ok[0] = True
    d.set_spectrum_cache_bytes(0)
    ms = timed(lambda: torch.fft.rfftn(vol), max(1, args.reps // 2))
    print(json.dumps({"kernel": "torch.fft.rfftn alone (rocFFT)", "grid": oshape, "ms": ms}))
    if fft3.available():
        ms = timed(lambda: fft3.rfft3(vol), max(1, args.reps // 2))
        print(json.dumps({"kernel": "fft3.rfft3 alone (at the volume's own shape)", "grid": oshape, "ms": ms}))


def _rl(args, torch, dev, g, bench, RichardsonLucyPlan, oshape):
    y = torch.poisson(torch.full(oshape, 100.0, device=dev), generator=g)
    plans = [("separable 9x7x7, one launch per iteration", RichardsonLucyPlan(oshape, None, dev, psf_factors=bench.gaussian_factors()), 4),
             ("separable 9x7x7, ratio / update launches",
              RichardsonLucyPlan(oshape, None, dev, psf_factors=bench.gaussian_factors(), fused="never"), 4),
             ("rotated 9x7x7 as ky (x) kzx, one launch per iteration (the default)", RichardsonLucyPlan(oshape, bench.rotated_psf(), dev), 4),
             ("rotated 9x7x7 as ky (x) kzx, ratio / update launches",
              RichardsonLucyPlan(oshape, bench.rotated_psf(), dev, fused="never"), 4)]
    if not args.skip_dense:
        plans.append(("dense 9x7x7 (rotated)", RichardsonLucyPlan(oshape, bench.rotated_psf(), dev, separable="never"), 1))
    for name, plan, iters in plans:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        plan(y, iterations=1)
        torch.cuda.synchronize()
        plan(y, iterations=iters, events=ev)
        torch.cuda.synchronize()
        launches = {"fused": 1, "y-separable (fused)": 1, "y-separable (4 launches)": 4}.get(plan.path, 2) * iters
        ms = ev[0].elapsed_time(ev[1]) / launches
        nbytes = 12.0 * y.numel()
        taps = {"fused": 46, "separable": 23, "y-separable": 70, "y-separable (fused)": 140}.get(plan.path, 441)
        plan.release()
        print(json.dumps({"kernel": f"RL launch, {name}", "path": plan.path, "grid": oshape, "ms_per_launch": ms,
                          "algorithmic_GBps": nbytes / ms / 1e6, "frac_of_8TBps": nbytes / ms / 1e6 / 8000,
                          "fma_TFLOPs": 2.0 * taps * y.numel() / ms / 1e9}))


def _psf_sweep(args, torch, dev, g, RichardsonLucyPlan, oshape):
    """ms per RL iteration over separable Gaussian PSFs from 3x3x3 to 15x15x15: which path each takes and where
    the rate leaves the 9x7x7 headline's (12 algorithmic bytes per voxel and iteration in every case)."""
    y = torch.poisson(torch.full(oshape, 100.0, device=dev), generator=g)
    sizes = [(3, 3, 3), (5, 5, 5), (7, 7, 7), (9, 7, 7), (9, 9, 9), (11, 9, 9), (13, 11, 11), (15, 9, 9), (15, 11, 11),
             (15, 15, 15), (5, 15, 15), (15, 3, 3)]
    if args.psf_sweep_wide:     # the in-plane extents where the fused tile shrinks: which form wins per (pz, pyx)
        sizes = [(pz, pyx, pyx) for pyx in (9, 11, 13, 15) for pz in (3, 5, 7, 9, 11, 13, 15)]
    for size in sizes:
        factors = []
        for n in size:
            x = np.arange(n) - n // 2
            k = np.exp(-0.5 * (x / (n / 4.5)) ** 2)
            factors.append((k / k.sum()).astype(np.float32))
        for fused in ("auto", "never"):
            plan = RichardsonLucyPlan(oshape, None, dev, psf_factors=tuple(factors), fused=fused)
            if fused == "never" and plan.path == "fused":
                plan.release()
                continue
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            plan(y, iterations=1)
            torch.cuda.synchronize()
            plan(y, iterations=4, events=ev)
            torch.cuda.synchronize()
            ms = ev[0].elapsed_time(ev[1]) / 4
            path = plan.path
            plan.release()
            print(json.dumps({"kernel": "RL iteration, separable PSF", "psf": list(size), "requested": fused, "path": path,
                              "grid": oshape, "ms_per_iteration": ms, "algorithmic_GBps": 12.0 * y.numel() / ms / 1e6,
                              "frac_of_8TBps": 12.0 * y.numel() / ms / 1e6 / 8000}), flush=True)
            if fused == "auto" and path != "fused":
                break      # (the two-launch form was what ran)


def _rl_tv(args, torch, dev, g, bench, RichardsonLucyPlan, oshape):
    """The total-variation launch of RL-TV (csrc/rl_tv.hip) alone -- between the plan's padded working volumes, in place,
    as an iteration runs it -- and an RL-TV iteration beside the plain fused one, all in this run (12 algorithmic bytes per
    voxel for the TV launch and for the fused RL launch alike)."""
    import ctypes

    from shrimpy_amd import _lib
    from shrimpy_amd.pipeline import gaussian_psf_factors

    y = torch.poisson(torch.full(oshape, 100.0, device=dev), generator=g)
    plan = RichardsonLucyPlan(oshape, None, dev, psf_factors=gaussian_psf_factors((9, 7, 7), (2.0, 1.2, 1.2)))
    out = torch.empty_like(y)
    plan(y, iterations=2, out=out)                                   # fills both working volumes
    a, b = plan._scratch()
    z, yy, xx = oshape
    n = y.numel()
    for label, stats in (("TV launch", None), ("TV launch with the reduction scalars", torch.zeros(2, dtype=torch.float64, device=dev))):
        def launch():
            _lib.call("lsr_rl_tv_scale_f32", a.logical_ptr(), a.pitch, a.plane, b.logical_ptr(), b.pitch, b.plane,
                      b.logical_ptr(), b.pitch, b.plane, z, yy, xx, ctypes.c_float(0.01), ctypes.c_float(1e-6),
                      None if stats is None else stats.data_ptr(), _lib.stream_ptr(dev))
        ms = timed(launch, args.reps)
        print(json.dumps({"kernel": label, "path": plan.path, "grid": oshape, "ms": ms,
                          "algorithmic_GBps": 12.0 * n / ms / 1e6, "frac_of_8TBps": 12.0 * n / ms / 1e6 / 8000}), flush=True)
    for label, kw in (("RL iteration, fused separable 9x7x7", {}), ("RL-TV iteration, fused separable 9x7x7", dict(tv_lambda=0.01)),
                      ("RL iteration, fused separable 9x7x7 (again)", {})):
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        plan(y, iterations=1, out=out, **kw)
        torch.cuda.synchronize()
        iters = max(4, args.reps)
        plan(y, iterations=iters, out=out, events=ev, **kw)
        torch.cuda.synchronize()
        print(json.dumps({"kernel": label, "path": plan.path, "grid": oshape, "iterations": iters,
                          "ms_per_iteration": ev[0].elapsed_time(ev[1]) / iters}), flush=True)
    plan.release()


def _median_ms(fn, reps, torch):
    """Median over `reps` launches, each between its own pair of HIP events, after one warm-up."""
    fn()
    torch.cuda.synchronize()
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in events:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return float(np.median([e0.elapsed_time(e1) for e0, e1 in events]))


def _pyramid(args, torch, dev, g, oshape):
    """Pyramid levels (csrc/pyramid.hip): lsr_downsample2_f32 level by level at fz = 2, 4.5 algorithmic bytes per input
    voxel (4 read, 0.5 written), against the copy rate of this card in this run (2 x 4 bytes per voxel, the figure
    tools/bw_probe.py reports) and against torch.nn.functional.avg_pool3d with the same partial-window rule."""
    from shrimpy_amd import _lib, pyramid

    reps = max(args.reps, 5)
    vol = torch.empty(oshape, dtype=torch.float32, device=dev).normal_(generator=g)
    other = torch.empty_like(vol)
    copy_ms = _median_ms(lambda: other.copy_(vol), reps, torch)
    copy_gbps = 8.0 * vol.numel() / copy_ms / 1e6
    del other
    records = [{"kernel": "device copy (torch copy_)", "grid": list(oshape), "ms": copy_ms, "GBps": copy_gbps}]
    cur = vol
    for level in (1, 2, 3):
        z, y, x = (int(n) for n in cur.shape)
        out = pyramid.downsample2(cur, 2)

        def launch(cur=cur, out=out, z=z, y=y, x=x):
            _lib.call("lsr_downsample2_f32", cur.data_ptr(), z, y, x, out.data_ptr(), 2, _lib.stream_ptr(dev))

        ms = _median_ms(launch, reps, torch)
        nbytes = 4.0 * cur.numel() + 4.0 * out.numel()
        pool = lambda cur=cur: torch.nn.functional.avg_pool3d(cur[None, None], 2, ceil_mode=True, count_include_pad=False)  # noqa: E731
        pool_ms = _median_ms(pool, reps, torch)
        same = bool(torch.allclose(pool()[0, 0], out, rtol=0.0, atol=4 * 2.0 ** -24 * float(cur.abs().max())))
        records.append({"kernel": "lsr_downsample2_f32", "level": level, "fz": 2, "in": [z, y, x], "out": list(out.shape),
                        "ms": ms, "algorithmic_GBps": nbytes / ms / 1e6, "frac_of_copy_rate": nbytes / ms / 1e6 / copy_gbps,
                        "avg_pool3d_ms": pool_ms, "speedup_over_avg_pool3d": pool_ms / ms, "agrees_with_avg_pool3d": same})
        cur = out
    records.append({"kernel": "lsr_downsample2_f32, levels 1-3", "grid": list(oshape),
                    "ms": sum(r["ms"] for r in records[1:]), "avg_pool3d_ms": sum(r["avg_pool3d_ms"] for r in records[1:])})
    stamp = {"sources": _lib.kernel_source_sha16(), "device": torch.cuda.get_device_name(dev), "reps": reps}
    path = ROOT / "profiles" / "pyramid_config2.jsonl"
    with open(path, "a") as f:
        for r in records:
            line = json.dumps({**r, **stamp})
            print(line, flush=True)
            f.write(line + "\n")


def _psf_fit(args, torch, dev):
    """Gaussian fits and the shifted average (csrc/psf_fit.hip): one bead per patch-sized cell of a synthetic volume -- a
    tilted Gaussian (principal sigmas 1.8, 1.0, 0.9 voxels) at a random sub-voxel offset, amplitude 1000-3000 on a background
    of 100 with noise of sigma 10 -- fitted from the cell's centre voxel, then averaged with the fitted offsets."""
    import time

    from shrimpy_amd import _lib, psf

    reps = max(args.reps, 5)
    records = []
    for patch in ((15, 19, 19), (31, 37, 19)):
        for n in (500, 2000):
            cells = (5, 10, n // 50)
            gen = torch.Generator(device=dev).manual_seed(11)
            mu = torch.rand((n, 3), generator=gen, device=dev, dtype=torch.float64) - 0.5
            amp = 1000.0 + 2000.0 * torch.rand(n, generator=gen, device=dev, dtype=torch.float64)
            a = np.deg2rad(20.0)
            axes = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
            w = torch.from_numpy((axes.T / np.array([1.8, 1.0, 0.9]) ** 2) @ axes).to(dev)
            grid = torch.stack(torch.meshgrid(*[torch.arange(m, device=dev, dtype=torch.float64) - m // 2 for m in patch],
                                              indexing="ij"), dim=-1)
            d = grid[None] - mu[:, None, None, None, :]
            beads = 100.0 + amp[:, None, None, None] * torch.exp(-0.5 * torch.einsum("...i,ij,...j->...", d, w, d))
            beads = beads + 10.0 * torch.randn(beads.shape, generator=gen, device=dev, dtype=torch.float64)
            vol = beads.reshape(*cells, *patch).permute(0, 3, 1, 4, 2, 5).reshape(cells[0] * patch[0], cells[1] * patch[1],
                                                                                  cells[2] * patch[2]).float().contiguous()
            del beads, d
            idx = np.stack(np.meshgrid(*[np.arange(c) for c in cells], indexing="ij"), axis=-1).reshape(-1, 3)
            peaks = idx * np.array(patch) + np.array(patch) // 2
            fits = psf.fit_beads(vol, peaks, patch)
            shape = tuple(int(v) for v in vol.shape)
            centres = torch.from_numpy(psf._centres(peaks, shape)).to(dev)
            fit = torch.empty((n, 12), dtype=torch.float64, device=dev)
            status = torch.empty(n, dtype=torch.int32, device=dev)

            def launch_fit():
                _lib.call("lsr_bead_fit_f32", vol.data_ptr(), *shape, centres.data_ptr(), n, *patch, 100, fit.data_ptr(),
                          status.data_ptr(), _lib.stream_ptr(dev))

            fit_ms = _median_ms(launch_fit, reps, torch)
            weights = torch.from_numpy(np.ascontiguousarray(np.concatenate(
                [psf.shift_weights(np.nan_to_num(fits.offset_zyx[:, k]), m) for k, m in enumerate(patch)], axis=1))).to(dev)
            nbytes = ctypes.c_int64(0)
            _lib.call("lsr_psf_shift_scratch_bytes", n, *patch, ctypes.byref(nbytes))
            scratch = torch.empty(nbytes.value // 8, dtype=torch.float64, device=dev)
            stats = torch.empty((n, 2), dtype=torch.float64, device=dev)
            out = torch.empty(patch, dtype=torch.float32, device=dev)

            def launch_shift():
                _lib.call("lsr_psf_accumulate_shifted_f32", vol.data_ptr(), *shape, centres.data_ptr(), n, *patch, stats.data_ptr(),
                          weights.data_ptr(), scratch.data_ptr(), out.data_ptr(), _lib.stream_ptr(dev))

            def launch_plain():
                _lib.call("lsr_psf_accumulate_f32", vol.data_ptr(), *shape, centres.data_ptr(), n, *patch, stats.data_ptr(),
                          out.data_ptr(), _lib.stream_ptr(dev))

            shift_ms, plain_ms = _median_ms(launch_shift, reps, torch), _median_ms(launch_plain, reps, torch)
            _lib.call("lsr_set_host_threads", int(args.host_threads))
            host = vol.cpu()
            t0 = time.perf_counter()
            twin = psf.fit_beads(host, peaks, patch)
            t1 = time.perf_counter()
            psf._average_shifted(host, peaks, np.nan_to_num(twin.offset_zyx), patch)
            t2 = time.perf_counter()
            err = np.abs(fits.offset_zyx - mu.cpu().numpy())[fits.status == 0]
            records.append({"kernel": "lsr_bead_fit_f32 / lsr_psf_accumulate_shifted_f32", "beads": n, "patch": list(patch),
                            "volume": list(shape), "fit_ms": fit_ms, "shifted_average_ms": shift_ms, "plain_average_ms": plain_ms,
                            "twin_fit_ms": 1e3 * (t1 - t0), "twin_shifted_average_ms": 1e3 * (t2 - t1),
                            "host_threads": int(args.host_threads), "converged": int((fits.status == 0).sum()),
                            "statuses_equal_the_twins": bool(np.array_equal(fits.status, twin.status)),
                            "median_centre_error_vox": float(np.median(err)) if len(err) else None,
                            "scratch_MB": nbytes.value / 1e6})
            del vol, scratch
    stamp = {"sources": _lib.kernel_source_sha16(), "device": torch.cuda.get_device_name(dev), "reps": reps}
    path = ROOT / "profiles" / "psf_fit.jsonl"
    with open(path, "a") as f:
        for r in records:
            line = json.dumps({**r, **stamp})
            print(line, flush=True)
            f.write(line + "\n")


def _stitch(args, torch, dev, g, tshape):
    """Stitching (csrc/stitch.hip): one launch for the canvas of a 2 x 2 grid of tiles at 10 % overlap, p = 1.  Algorithmic
    bytes: 4 * (tile voxels touched + canvas voxels) -- every tile voxel is read once, every canvas voxel written once --
    against the copy rate of this card in this run and against the torch scatter formulation (per tile
    acc[box] += w * v; wsum[box] += w, then acc / wsum)."""
    from shrimpy_amd import _lib, stitch

    reps = 5
    z, y, x = tshape
    sy, sx = int(round(0.9 * y)), int(round(0.9 * x))
    tiles = [torch.empty(tshape, dtype=torch.float32, device=dev).normal_(generator=g) for _ in range(4)]
    other = torch.empty_like(tiles[0])
    other.copy_(tiles[0])
    copy_ms = _median_ms(lambda: other.copy_(tiles[0]), reps, torch)
    copy_gbps = 8.0 * other.numel() / copy_ms / 1e6
    del other
    records = [{"kernel": "device copy (torch copy_)", "grid": list(tshape), "ms": copy_ms, "GBps": copy_gbps}]
    for label, fx in (("integer placement", 0.0), ("fractional on x", 0.5)):
        tr = [(0.0, 0.0, 0.0), (0.0, 0.0, sx + fx), (0.0, float(sy), 0.0), (0.0, float(sy), sx + fx)]
        shape, origin = stitch.canvas_geometry([tshape] * 4, tr)
        out = torch.empty(shape, dtype=torch.float32, device=dev)
        table = torch.from_numpy(stitch._host_table(tiles, tr)).to(dev)
        o3, s3 = (ctypes.c_int64 * 3)(*origin), (ctypes.c_int64 * 3)(*shape)

        def launch():
            _lib.call("lsr_stitch_f32", table.data_ptr(), 4, out.data_ptr(), o3, s3, 1, 0.0, _lib.stream_ptr(dev))

        launch()
        ms = _median_ms(launch, reps, torch)
        touched = 4 * z * y * x
        nbytes = 4.0 * (touched + out.numel())
        rec = {"kernel": "lsr_stitch_f32", "placement": label, "tiles": [list(tshape)] * 4, "translations": [list(t) for t in tr],
               "canvas": list(shape), "p": 1, "ms": ms, "algorithmic_GBps": nbytes / ms / 1e6,
               "frac_of_copy_rate": nbytes / ms / 1e6 / copy_gbps}
        if fx == 0.0:
            yy = torch.arange(y, device=dev, dtype=torch.float32)
            xx = torch.arange(x, device=dev, dtype=torch.float32)
            w = (torch.minimum(yy + 1, y - yy)[:, None] * torch.minimum(xx + 1, x - xx)[None, :])[None]
            acc, wsum = torch.empty_like(out), torch.empty_like(out)

            def scatter():
                acc.zero_()
                wsum.zero_()
                for tile, t in zip(tiles, tr):
                    oy, ox = int(t[1]) - origin[1], int(t[2]) - origin[2]
                    acc[:, oy:oy + y, ox:ox + x] += w * tile
                    wsum[:, oy:oy + y, ox:ox + x] += w
                return acc / wsum

            scatter()
            scatter_ms = _median_ms(scatter, reps, torch)
            ref = scatter()
            launch()
            worst = float((ref - out).abs().max())
            rec.update({"torch_scatter_ms": scatter_ms, "speedup_over_torch_scatter": scatter_ms / ms,
                        "max_abs_difference_from_torch_scatter": worst})
            del acc, wsum, ref, w
        records.append(rec)
        del out
    stamp = {"sources": _lib.kernel_source_sha16(), "device": torch.cuda.get_device_name(dev), "reps": reps, "warmups": 2}
    path = ROOT / "profiles" / "stitch_config2.jsonl"
    with open(path, "a") as f:
        for r in records:
            line = json.dumps({**r, **stamp})
            print(line, flush=True)
            f.write(line + "\n")


LABEL_LAUNCHES = ("local", "merge", "flatten", "count", "scan", "rank", "final")
# algorithmic bytes per voxel of each launch (csrc/label.hip): what it must read and write once, chains and gathers aside
LABEL_BYTES_PER_VOXEL = {"local": 8.0, "merge": 4.0, "flatten": 8.0, "count": 4.0, "scan": 0.0, "rank": 4.0, "final": 8.0,
                         "regions": 8.0, "remap": 8.0}


def _label(args, torch, dev, g, bench, oshape):
    """Labelling (csrc/label.hip) at the config-2 deskewed shape: every launch of lsr_label_f32 on its own (HIP events between
    them: lsr_label_profile_f32), lsr_label_regions_f32 with intensities and lsr_label_remap_i32, for three inputs -- the
    bench's bead scene at its multi-Otsu threshold, Bernoulli noise at p = 0.3 (many winding components) and an all-foreground
    volume (one component: the most contended case) -- under connectivity 6.  Beside them the bytes per voxel each launch
    moves, a device copy in the same run, and scipy.ndimage.label on the host at a reduced shape."""
    import time

    from shrimpy_amd import _lib, dynatrack, segment

    reps = max(args.reps, 5)
    z, y, x = oshape
    n = z * y * x
    labels = torch.empty(oshape, dtype=torch.int32, device=dev)
    other = torch.empty_like(labels)
    copy_ms = _median_ms(lambda: other.copy_(labels), reps, torch)
    del other
    records = [{"kernel": "device copy (torch copy_)", "grid": list(oshape), "ms": copy_ms, "GBps": 8.0 * n / copy_ms / 1e6}]
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch = torch.empty(_lib.call_value("lsr_label_scratch_bytes", z, y, x), dtype=torch.uint8, device=dev)
    ms7 = (ctypes.c_float * 7)()

    def scenes():
        vol = bench.synthetic_raw(oshape, 1000, dev)
        yield "bead scene (bench.synthetic_raw) at its multi-Otsu threshold", vol, float(dynatrack._multiotsu_threshold(vol, 0))
        del vol
        yield "Bernoulli noise, p = 0.3", torch.rand(oshape, device=dev, generator=g), 0.7
        yield "all foreground", torch.ones(oshape, dtype=torch.float32, device=dev), 0.5

    for name, vol, threshold in scenes():
        times = []
        for _ in range(reps + 1):
            _lib.call("lsr_label_profile_f32", vol.data_ptr(), z, y, x, ctypes.c_float(threshold), 6, labels.data_ptr(),
                      count.data_ptr(), scratch.data_ptr(), ms7, _lib.stream_ptr(dev))
            times.append(list(ms7))
        med = np.median(np.asarray(times[1:]), axis=0)
        n_objects = int(count.item())
        base = {"input": name, "grid": list(oshape), "connectivity": 6, "threshold": threshold, "objects": n_objects,
                "foreground_fraction": float((labels != 0).sum().item()) / n}
        for launch, ms in zip(LABEL_LAUNCHES, med):
            bpv = LABEL_BYTES_PER_VOXEL[launch]
            records.append({**base, "kernel": f"lsr_label_f32: {launch}", "ms": float(ms), "bytes_per_voxel": bpv,
                            "algorithmic_GBps": bpv * n / float(ms) / 1e6})
        records.append({**base, "kernel": "lsr_label_f32: all seven launches", "ms": float(med.sum()), "Mvox_per_s": n / float(med.sum()) / 1e3})
        if 0 < n_objects <= 200_000_000:
            table = torch.zeros(n_objects * segment.REGION_DTYPE.itemsize, dtype=torch.uint8, device=dev)

            def regions():
                table.zero_()
                _lib.call("lsr_label_regions_f32", labels.data_ptr(), vol.data_ptr(), z, y, x, n_objects, table.data_ptr(),
                          _lib.stream_ptr(dev))

            ms = _median_ms(regions, reps, torch)
            records.append({**base, "kernel": "lsr_label_regions_f32 (with intensities; the table's memset included)", "ms": ms,
                            "bytes_per_voxel": LABEL_BYTES_PER_VOXEL["regions"], "algorithmic_GBps": 8.0 * n / ms / 1e6})
            del table
        lut = torch.arange(n_objects + 1, dtype=torch.int32, device=dev)           # (the identity: labels stay what they are)
        ms = _median_ms(lambda: _lib.call("lsr_label_remap_i32", labels.data_ptr(), n, lut.data_ptr(), n_objects + 1,
                                          _lib.stream_ptr(dev)), reps, torch)
        records.append({**base, "kernel": "lsr_label_remap_i32", "ms": ms, "bytes_per_voxel": LABEL_BYTES_PER_VOXEL["remap"],
                        "algorithmic_GBps": 8.0 * n / ms / 1e6})
        del vol, lut
    # the step a user without these kernels would run: scipy on the host, at a shape it finishes in seconds
    from scipy import ndimage

    hshape = tuple(int(v) for v in args.label_host_grid.split(","))
    mask = np.random.default_rng(3).random(hshape, dtype=np.float32) > 0.7
    t0 = time.perf_counter()
    _, n_host = ndimage.label(mask)
    host_s = time.perf_counter() - t0
    records.append({"kernel": "scipy.ndimage.label on the host (one thread)", "input": "Bernoulli noise, p = 0.3", "grid": list(hshape),
                    "connectivity": 6, "objects": int(n_host), "ms": 1e3 * host_s, "Mvox_per_s": mask.size / host_s / 1e6})
    stamp = {"sources": _lib.kernel_source_sha16(), "device": torch.cuda.get_device_name(dev), "reps": reps, "warmups": 1}
    path = ROOT / "profiles" / "label_config2.jsonl"
    with open(path, "a") as f:
        for r in records:
            line = json.dumps({**r, **stamp})
            print(line, flush=True)
            f.write(line + "\n")


# algorithmic bytes per voxel of each launch of the watershed (csrc/watershed.hip): local reads objects and surface and writes a
# parent word and a direction byte (the halo's re-reads aside), merge reads the direction bytes; the rest is the labelling's
WATERSHED_BYTES_PER_VOXEL = {**LABEL_BYTES_PER_VOXEL, "local": 13.0, "merge": 1.0, "saddles": 12.0}


def _watershed(args, torch, dev, g, bench, oshape):
    """The watershed (csrc/watershed.hip) at the config-2 deskewed shape on the three scenes of --label: the objects are the
    labelling's (connectivity 6), the surface is their depth map (distance.distance_transform_labels, invert) blurred with sigma
    1 -- what SegmentSettings.split runs.  Every launch of lsr_watershed_f32 on its own (HIP events between them:
    lsr_watershed_profile_f32), the labelling's seven launches on the same scene in the same run, and the saddle pass (the
    table's memset included; no wave pre-reduction is built).  All foreground has no background voxel: its depth is +inf
    everywhere, one plateau that the index rule alone orders -- the longest chains this rule can make."""
    from shrimpy_amd import _lib, distance, dynatrack, watershed

    reps = 3
    z, y, x = oshape
    n = z * y * x
    labels = torch.empty(oshape, dtype=torch.int32, device=dev)
    basins = torch.empty_like(labels)
    copy_ms = _median_ms(lambda: basins.copy_(labels), reps, torch)
    records = [{"kernel": "device copy (torch copy_)", "grid": list(oshape), "ms": copy_ms, "GBps": 8.0 * n / copy_ms / 1e6}]
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch = torch.empty(_lib.call_value("lsr_watershed_scratch_bytes", z, y, x), dtype=torch.uint8, device=dev)
    ms7 = (ctypes.c_float * 7)()

    def scenes():
        vol = bench.synthetic_raw(oshape, 1000, dev)
        yield "bead scene (bench.synthetic_raw) at its multi-Otsu threshold", vol, float(dynatrack._multiotsu_threshold(vol, 0))
        del vol
        yield "Bernoulli noise, p = 0.3", torch.rand(oshape, device=dev, generator=g), 0.7
        yield "all foreground", torch.ones(oshape, dtype=torch.float32, device=dev), 0.5

    for name, vol, threshold in scenes():
        times = []
        for _ in range(reps + 1):
            _lib.call("lsr_label_profile_f32", vol.data_ptr(), z, y, x, ctypes.c_float(threshold), 6, labels.data_ptr(),
                      count.data_ptr(), scratch.data_ptr(), ms7, _lib.stream_ptr(dev))
            times.append(list(ms7))
        label_med = np.median(np.asarray(times[1:]), axis=0)
        n_objects = int(count.item())
        del vol
        print(f"# {name}: {n_objects} objects, labelled in {float(label_med.sum()):.2f} ms", flush=True)
        surface = dynatrack._gaussian_blur_3d(distance.distance_transform_labels(labels, (1, 1, 1), invert=True), 1.0)
        torch.cuda.empty_cache()
        times = []
        for _ in range(reps + 1):
            _lib.call("lsr_watershed_profile_f32", labels.data_ptr(), surface.data_ptr(), z, y, x, 6, basins.data_ptr(),
                      count.data_ptr(), scratch.data_ptr(), ms7, _lib.stream_ptr(dev))
            times.append(list(ms7))
        med = np.median(np.asarray(times[1:]), axis=0)
        n_basins = int(count.item())
        print(f"# {name}: {n_basins} basins in {float(med.sum()):.2f} ms", flush=True)
        base = {"input": name, "grid": list(oshape), "connectivity": 6, "objects": n_objects, "basins": n_basins,
                "surface": "depth map (exact EDT), Gaussian sigma 1", "foreground_fraction": float((labels != 0).sum().item()) / n}
        for launch, ms, lms in zip(LABEL_LAUNCHES, med, label_med):
            bpv = WATERSHED_BYTES_PER_VOXEL[launch]
            records.append({**base, "kernel": f"lsr_watershed_f32: {launch}", "ms": float(ms), "bytes_per_voxel": bpv,
                            "algorithmic_GBps": bpv * n / float(ms) / 1e6, "lsr_label_f32_same_launch_ms": float(lms)})
        records.append({**base, "kernel": "lsr_watershed_f32: all seven launches", "ms": float(med.sum()),
                        "Mvox_per_s": n / float(med.sum()) / 1e3, "lsr_label_f32_all_seven_launches_ms": float(label_med.sum())})
        if n_basins >= 2:
            capacity = min(1 << int(4 * n_basins + 1024 - 1).bit_length(), 1 << 30)    # (watershed.basin_saddles' first capacity)
            counts = torch.zeros(2, dtype=torch.int32, device=dev)
            while True:
                table = torch.zeros(capacity * watershed.SADDLE_DTYPE.itemsize, dtype=torch.uint8, device=dev)

                def saddles():
                    table.zero_()
                    _lib.call("lsr_watershed_saddles_f32", labels.data_ptr(), basins.data_ptr(), surface.data_ptr(), z, y, x, 6,
                              capacity, table.data_ptr(), counts.data_ptr(), _lib.stream_ptr(dev))

                ms = _median_ms(saddles, reps, torch)
                claimed, lost = (int(v) for v in counts.cpu().tolist())
                records.append({**base, "kernel": "lsr_watershed_saddles_f32 (the table's memset included; no wave pre-reduction)",
                                "ms": ms, "capacity": capacity, "saddles": claimed, "pairs_without_a_slot": lost,
                                "bytes_per_voxel": WATERSHED_BYTES_PER_VOXEL["saddles"], "algorithmic_GBps": 12.0 * n / ms / 1e6})
                del table
                if lost == 0 or capacity >= 1 << 30:
                    break
                capacity *= 2
        del surface
        torch.cuda.empty_cache()
    stamp = {"sources": _lib.kernel_source_sha16(), "device": torch.cuda.get_device_name(dev), "reps": reps, "warmups": 1}
    path = ROOT / "profiles" / "watershed_config2.jsonl"
    with open(path, "a") as f:
        for r in records:
            line = json.dumps({**r, **stamp})
            print(line, flush=True)
            f.write(line + "\n")


EDT_LAUNCHES = ("x", "y", "z")
# algorithmic bytes per voxel of each launch (csrc/edt.hip) with both outputs asked for: what it must read and write once --
# the x pass's second sweep over its own words and the envelope stacks of y and z aside
EDT_BYTES_PER_VOXEL = {"x": 8.0, "y": 8.0, "z": 12.0}


OVERLAP_STEP = 1024          # voxels one workgroup takes per stride of its span (csrc/overlap.hpp kStep)
OVERLAP_CAPS = (256, 1024, 2048, 4096, 16384, 65536, 262144, 1048576)


def _overlap(args, torch, dev, g, bench, oshape):
    """The label-overlap kernel (csrc/overlap.hip) at the config-2 deskewed shape on the three scenes of --label, labelled under
    connectivity 6; frame t + 1 is frame t rolled by 2 voxels in x.  Per scene: the kernel at every grid cap of OVERLAP_CAPS
    (the table zeroed outside the timed region; 0 = the default is among them), torch.unique of the packed pairs (what a user
    without the kernel would write), and the global atomics: each workgroup flushes one compare-and-swap + add per distinct
    pair of its span, counted here by torch.unique on a sample of 16 spans and scaled to the grid.  The floor is two volume
    reads, 8 bytes per voxel: the device copy of one int32 volume in the same run moves as much."""
    from shrimpy_amd import _lib, dynatrack, segment, track

    reps = 3
    z, y, x = oshape
    n = z * y * x
    lds_slots, default_cap = track.overlap_geometry()
    a = torch.empty(oshape, dtype=torch.int32, device=dev)
    b = torch.empty_like(a)
    copy_ms = _median_ms(lambda: b.copy_(a), reps, torch)
    records = [{"kernel": "device copy of one int32 volume (torch copy_)", "grid": list(oshape), "ms": copy_ms,
                "GBps": 8.0 * n / copy_ms / 1e6}]
    del a, b
    zero3 = (ctypes.c_int32 * 3)(0, 0, 0)

    def scenes():
        vol = bench.synthetic_raw(oshape, 1000, dev)
        yield "bead scene (bench.synthetic_raw) at its multi-Otsu threshold", vol, float(dynatrack._multiotsu_threshold(vol, 0))
        del vol
        yield "Bernoulli noise, p = 0.3", torch.rand(oshape, device=dev, generator=g), 0.7
        yield "all foreground", torch.ones(oshape, dtype=torch.float32, device=dev), 0.5

    def geometry(cap):
        steps = -(-n // OVERLAP_STEP)
        span = -(-steps // min(steps, cap)) * OVERLAP_STEP
        return span, -(-n // span)

    for name, vol, threshold in scenes():
        a, n_objects = segment.label_volume(vol, threshold, 6)
        del vol
        b = torch.roll(a, 2, dims=2).contiguous()
        capacity = 1 << int(4 * min(2 * n_objects, n) + 1024 - 1).bit_length()
        table = torch.zeros(capacity * track.OVERLAP_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        counts = torch.zeros(2, dtype=torch.int32, device=dev)
        base = {"input": name, "grid": list(oshape), "objects": n_objects, "capacity": capacity, "lds_slots": lds_slots,
                "foreground_fraction": float((a != 0).sum().item()) / n}
        pairs = None
        for cap in OVERLAP_CAPS:
            times = []
            for _ in range(reps + 1):
                table.zero_()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _lib.call("lsr_label_overlap_i32", a.data_ptr(), b.data_ptr(), z, y, x, zero3, capacity, table.data_ptr(),
                          counts.data_ptr(), cap, _lib.stream_ptr(dev))
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
            ms = float(np.median(times[1:]))
            claimed, lost = (int(v) for v in counts.cpu().tolist())
            pairs = claimed
            span, blocks = geometry(cap)
            # distinct pairs per span on a sample of the spans: what each of those workgroups flushes
            sample = sorted({int(k) for k in np.linspace(0, blocks - 1, 16)})
            distinct = []
            for k in sample:
                sa, sb = a.view(-1)[k * span:(k + 1) * span], b.view(-1)[k * span:(k + 1) * span]
                fg = (sa > 0) & (sb > 0)
                distinct.append(int(torch.unique((sa[fg].long() << 32) | sb[fg].long()).numel()))
            records.append({**base, "kernel": "lsr_label_overlap_i32", "max_blocks": cap, "default": cap == default_cap,
                            "workgroups": blocks, "span_voxels": span, "ms": ms, "bytes_per_voxel": 8.0,
                            "algorithmic_GBps": 8.0 * n / ms / 1e6, "times_the_copy": ms / copy_ms, "pairs": claimed, "lost": lost,
                            "sampled_spans": len(sample), "distinct_pairs_per_span_mean": float(np.mean(distinct)),
                            "distinct_pairs_per_span_max": int(max(distinct)),
                            "spans_over_the_lds_table": int(sum(d > lds_slots for d in distinct)),
                            "global_atomic_pairs_estimate": float(np.mean(distinct)) * blocks,
                            "global_atomic_pairs_floor": claimed})
        del table

        def unique():
            fg = (a > 0) & (b > 0)
            return torch.unique((a.long() << 32 | b)[fg], return_counts=True)

        keys, _ = unique()
        assert int(keys.numel()) == pairs, "torch.unique and the kernel disagree on the number of pairs"
        del keys
        ms = _median_ms(unique, reps, torch)
        records.append({**base, "kernel": "torch.unique((a.long() << 32 | b)[fg], return_counts=True)", "ms": ms, "pairs": pairs,
                        "times_the_copy": ms / copy_ms})
        del a, b
        torch.cuda.empty_cache()
    stamp = {"sources": _lib.kernel_source_sha16(), "device": torch.cuda.get_device_name(dev), "reps": reps, "warmups": 1,
             "lds_probes": 16, "alternatives": "the grid cap is swept here; the LDS slot count (2048) and the LDS probe bound (16) "
                                               "are compile-time constants of csrc/overlap.hpp and were not varied"}
    path = ROOT / "profiles" / "overlap_config2.jsonl"
    with open(path, "a") as f:
        for r in records:
            line = json.dumps({**r, **stamp})
            print(line, flush=True)
            f.write(line + "\n")


def _label_scenes(torch, dev, g, bench, oshape):
    """``(name, float32 volume, threshold)`` of the three scenes the label tables are measured on."""
    from shrimpy_amd import dynatrack

    vol = bench.synthetic_raw(oshape, 1000, dev)
    yield "bead scene (bench.synthetic_raw) at its multi-Otsu threshold", vol, float(dynatrack._multiotsu_threshold(vol, 0))
    del vol
    yield "Bernoulli noise, p = 0.3", torch.rand(oshape, device=dev, generator=g), 0.7
    yield "all foreground", torch.ones(oshape, dtype=torch.float32, device=dev), 0.5


def _timed_cleared(torch, launch, clear, reps):
    """ms of ``launch`` between HIP events: the median of ``reps`` calls after a warm-up, ``clear()`` outside the timed region."""
    times = []
    for _ in range(reps + 1):
        clear()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times[1:]))


MOMENTS_STEP = 1024          # voxels one workgroup takes per stride of its span (csrc/moments.hpp kStep)
MOMENTS_SLOTS = (64, 128, 256, 512)
MOMENTS_CAPS = (1024, 4096, 8192, 16384, 65536, 262144)
MOMENTS_PROBES = 8           # the LDS probe bound (csrc/moments.hpp kLdsProbes)
MOMENTS_PROBE_SWEEP = (1, 2, 4, 16, 32)


def _moments(args, torch, dev, g, bench, oshape):
    """The label-moment kernel (csrc/moments.hip) at the config-2 deskewed shape on the three scenes of --label, labelled under
    connectivity 6.  Per scene, each the median of 3 calls after a warm-up between HIP events (the tables zeroed outside the timed
    region): the kernel as shipped; the sweep of LDS slots and grid caps through the measurement entry, and once the plain form
    without an LDS table (every run head straight to global atomics); lsr_label_regions_f32 without intensities in the same run;
    the three overlap launches of segment.contact_table.  The floor is one volume read, 4 bytes per voxel: the device copy of one
    int32 volume moves twice as much."""
    from shrimpy_amd import _lib, segment, track

    reps = 3
    z, y, x = oshape
    n = z * y * x
    lds_slots, default_cap = segment.moments_geometry()
    a = torch.empty(oshape, dtype=torch.int32, device=dev)
    b = torch.empty_like(a)
    copy_ms = _median_ms(lambda: b.copy_(a), reps, torch)
    records = [{"kernel": "device copy of one int32 volume (torch copy_)", "grid": list(oshape), "ms": copy_ms,
                "GBps": 8.0 * n / copy_ms / 1e6}]
    del a, b
    stream = _lib.stream_ptr(dev)

    def scenes():
        return _label_scenes(torch, dev, g, bench, oshape)

    def timed(launch, clear):
        return _timed_cleared(torch, launch, clear, reps)

    def geometry(cap):
        steps = -(-n // MOMENTS_STEP)
        span = -(-steps // min(steps, cap)) * MOMENTS_STEP
        return span, -(-n // span)

    for name, vol, threshold in scenes():
        labels, n_objects = segment.label_volume(vol, threshold, 6)
        del vol
        torch.cuda.empty_cache()
        base = {"input": name, "grid": list(oshape), "objects": n_objects, "foreground_fraction": float((labels != 0).sum().item()) / n}
        print(f"# {name}: {n_objects} objects", flush=True)
        table = torch.zeros(max(n_objects, 1) * segment.MOMENTS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        ms = timed(lambda: _lib.call("lsr_label_moments_i32", labels.data_ptr(), z, y, x, n_objects, table.data_ptr(), 0, stream),
                   table.zero_)
        want = table.clone()
        span, blocks = geometry(default_cap)
        records.append({**base, "kernel": "lsr_label_moments_i32", "lds_slots": lds_slots, "lds_probes": MOMENTS_PROBES,
                        "max_blocks": default_cap, "default": True,
                        "workgroups": blocks, "span_voxels": span, "ms": ms, "bytes_per_voxel": 4.0,
                        "algorithmic_GBps": 4.0 * n / ms / 1e6, "times_the_copy": ms / copy_ms})
        forms = [(0, default_cap, 1)] + [(slots, cap, MOMENTS_PROBES) for slots in MOMENTS_SLOTS for cap in MOMENTS_CAPS]
        forms += [(lds_slots, default_cap, probes) for probes in MOMENTS_PROBE_SWEEP]
        for slots, cap, probes in forms:
            ms = timed(lambda: _lib.call("lsr_label_moments_variant_i32", labels.data_ptr(), z, y, x, n_objects, table.data_ptr(),
                                         cap, slots, probes, stream), table.zero_)
            assert torch.equal(table, want), "a form of the kernel disagrees with the shipped one"
            span, blocks = geometry(cap)
            records.append({**base, "kernel": "lsr_label_moments_variant_i32" + (" (plain form: no LDS table)" if slots == 0 else ""),
                            "lds_slots": slots, "lds_probes": probes if slots else 0, "max_blocks": cap,
                            "default": (slots, cap, probes) == (lds_slots, default_cap, MOMENTS_PROBES),
                            "workgroups": blocks, "span_voxels": span, "ms": ms, "times_the_copy": ms / copy_ms})
        del table, want
        regions = torch.zeros(max(n_objects, 1) * segment.REGION_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        ms = timed(lambda: _lib.call("lsr_label_regions_f32", labels.data_ptr(), None, z, y, x, n_objects, regions.data_ptr(), stream),
                   regions.zero_)
        records.append({**base, "kernel": "lsr_label_regions_f32 (intensity = NULL)", "ms": ms, "times_the_copy": ms / copy_ms})
        del regions
        capacity = 1 << int(4 * min(2 * n_objects, n) + 1024 - 1).bit_length()
        pairs = torch.zeros(capacity * track.OVERLAP_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        counts = torch.zeros(2, dtype=torch.int32, device=dev)
        shifts = [(ctypes.c_int32 * 3)(*s) for s in ((1, 0, 0), (0, 1, 0), (0, 0, 1))]

        def contacts():
            for s in shifts:
                _lib.call("lsr_label_overlap_i32", labels.data_ptr(), labels.data_ptr(), z, y, x, s, capacity, pairs.data_ptr(),
                          counts.data_ptr(), 0, stream)

        ms = timed(contacts, pairs.zero_)
        records.append({**base, "kernel": "the three lsr_label_overlap_i32 launches of segment.contact_table (one table)",
                        "capacity": capacity, "lost": int(counts.cpu()[1]), "ms": ms, "times_the_copy": ms / copy_ms})
        del pairs, labels
        torch.cuda.empty_cache()
    stamp = {"sources": _lib.kernel_source_sha16(), "device": torch.cuda.get_device_name(dev), "reps": reps, "warmups": 1}
    path = ROOT / "profiles" / "moments_config2.jsonl"
    with open(path, "a") as f:
        for r in records:
            line = json.dumps({**r, **stamp})
            print(line, flush=True)
            f.write(line + "\n")


INTENSITY_SLOTS = (64, 128, 256, 512)
INTENSITY_CAPS = (1024, 4096, 16384, 65536, 262144)
INTENSITY_PROBES = 8         # the LDS probe bound (csrc/intensity.hpp kLdsProbes)
INTENSITY_PROBE_SWEEP = (1, 2, 4, 16, 32)


def _intensity(args, torch, dev, g, bench, oshape):
    """The label-intensity kernel (csrc/intensity.hip) at the config-2 deskewed shape on the three scenes of --label, labelled
    under connectivity 6, the scene's own float32 volume as the values (and a uint16 image of it).  Per scene, each the median of
    3 calls after a warm-up between HIP events (the tables zeroed outside the timed region): the kernel as shipped for float32
    and for uint16 values; the sweep of LDS slots, grid caps and probe bounds through the measurement entry (float32), and once
    the plain form without an LDS table; lsr_label_regions_f32 WITH the intensities in the same run.  The floor is one read of
    both volumes, 8 bytes per voxel: the device copy of one int32 volume plus one float32 volume moves twice as much.  Every
    form's counts and extremes must equal the shipped form's; the greatest relative difference of a float64 sum is recorded."""
    from shrimpy_amd import _lib, segment

    reps = 3
    z, y, x = oshape
    n = z * y * x
    lds_slots, default_cap = segment.intensity_geometry()
    a, fa = torch.empty(oshape, dtype=torch.int32, device=dev), torch.empty(oshape, dtype=torch.float32, device=dev)
    b, fb = torch.empty_like(a), torch.empty_like(fa)

    def copies():
        b.copy_(a)
        fb.copy_(fa)

    copy_ms = _median_ms(copies, reps, torch)
    records = [{"kernel": "device copy of one int32 volume and one float32 volume (torch copy_)", "grid": list(oshape), "ms": copy_ms,
                "GBps": 16.0 * n / copy_ms / 1e6}]
    del a, b, fa, fb
    stream = _lib.stream_ptr(dev)
    record = segment.INTENSITY_DTYPE_F32.itemsize

    def geometry(cap):
        steps = -(-n // MOMENTS_STEP)
        span = -(-steps // min(steps, cap)) * MOMENTS_STEP
        return span, -(-n // span)

    def split(table):
        """(the integer words of every record: count, extremes and pad; the five float64 sums)"""
        words = table.view(torch.int64).view(-1, record // 8)
        return torch.cat([words[:, :1], words[:, 6:]], dim=1), words[:, 1:6].contiguous().view(torch.float64)

    for name, vol, threshold in _label_scenes(torch, dev, g, bench, oshape):
        labels, n_objects = segment.label_volume(vol, threshold, 6)
        # a uint16 image of the values: scaled into 0 .. 65535, cut to 16 bits through int16 (same bits)
        scale = 65535.0 / max(float(vol.max().item()), 1e-30)
        u16 = (vol.clamp(min=0.0) * scale).to(torch.int32).to(torch.int16).view(torch.uint16)
        torch.cuda.empty_cache()
        base = {"input": name, "grid": list(oshape), "objects": n_objects, "foreground_fraction": float((labels != 0).sum().item()) / n}
        print(f"# {name}: {n_objects} objects", flush=True)
        table = torch.zeros(max(n_objects, 1) * record, dtype=torch.uint8, device=dev)
        span, blocks = geometry(default_cap)
        shipped = {"lds_slots": lds_slots, "lds_probes": INTENSITY_PROBES, "max_blocks": default_cap, "default": True,
                   "workgroups": blocks, "span_voxels": span}
        ms = _timed_cleared(torch, lambda: _lib.call("lsr_label_intensity_u16", labels.data_ptr(), u16.data_ptr(), z, y, x, n_objects,
                                                     table.data_ptr(), 0, stream), table.zero_, reps)
        records.append({**base, "kernel": "lsr_label_intensity_u16", **shipped, "ms": ms, "bytes_per_voxel": 6.0,
                        "algorithmic_GBps": 6.0 * n / ms / 1e6, "times_the_copy": ms / copy_ms})
        del u16
        ms_f32 = _timed_cleared(torch, lambda: _lib.call("lsr_label_intensity_f32", labels.data_ptr(), vol.data_ptr(), z, y, x,
                                                         n_objects, table.data_ptr(), 0, stream), table.zero_, reps)
        want_words, want_sums = (t.clone() for t in split(table))
        forms = [(0, default_cap, 1)] + [(slots, cap, INTENSITY_PROBES) for slots in INTENSITY_SLOTS for cap in INTENSITY_CAPS]
        forms += [(lds_slots, default_cap, probes) for probes in INTENSITY_PROBE_SWEEP]
        swept = []
        for slots, cap, probes in forms:
            ms = _timed_cleared(torch, lambda: _lib.call("lsr_label_intensity_variant", labels.data_ptr(), vol.data_ptr(), 0, z, y, x,
                                                         n_objects, table.data_ptr(), cap, slots, probes, stream), table.zero_, reps)
            words, sums = split(table)
            assert torch.equal(words, want_words), "a form of the kernel disagrees with the shipped one in a count or an extreme"
            difference = float(((sums - want_sums).abs() / want_sums.abs().clamp(min=1e-300)).max().item()) if n_objects else 0.0
            span, blocks = geometry(cap)
            swept.append({**base, "kernel": "lsr_label_intensity_variant (f32)" + (" (plain form: no LDS table)" if slots == 0 else ""),
                          "lds_slots": slots, "lds_probes": probes if slots else 0, "max_blocks": cap,
                          "default": (slots, cap, probes) == (lds_slots, default_cap, INTENSITY_PROBES), "workgroups": blocks,
                          "span_voxels": span, "ms": ms, "times_the_copy": ms / copy_ms,
                          "greatest_relative_difference_of_a_sum": difference})
        del table, want_words, want_sums
        regions = torch.zeros(max(n_objects, 1) * segment.REGION_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        ms_regions = _timed_cleared(torch, lambda: _lib.call("lsr_label_regions_f32", labels.data_ptr(), vol.data_ptr(), z, y, x,
                                                             n_objects, regions.data_ptr(), stream), regions.zero_, reps)
        records.append({**base, "kernel": "lsr_label_intensity_f32", **shipped, "ms": ms_f32, "bytes_per_voxel": 8.0,
                        "algorithmic_GBps": 8.0 * n / ms_f32 / 1e6, "times_the_copy": ms_f32 / copy_ms,
                        "times_faster_than_lsr_label_regions_f32": ms_regions / ms_f32})
        records += swept
        records.append({**base, "kernel": "lsr_label_regions_f32 (with the intensities)", "ms": ms_regions,
                        "times_the_copy": ms_regions / copy_ms})
        del regions, labels, vol
        torch.cuda.empty_cache()
    stamp = {"sources": _lib.kernel_source_sha16(), "device": torch.cuda.get_device_name(dev), "reps": reps, "warmups": 1}
    path = ROOT / "profiles" / "intensity_config2.jsonl"
    with open(path, "a") as f:
        for r in records:
            line = json.dumps({**r, **stamp})
            print(line, flush=True)
            f.write(line + "\n")
    speedup = [r["times_faster_than_lsr_label_regions_f32"] for r in records
               if r.get("input") == "all foreground" and "times_faster_than_lsr_label_regions_f32" in r][0]
    print(f"# all foreground: lsr_label_intensity_f32 is {speedup:.1f} times faster than lsr_label_regions_f32 "
          f"({'meets' if speedup >= 10.0 else 'MISSES'} the condition of 10)", flush=True)


COLOC_SLOTS = (64, 128, 256)
COLOC_CAPS = (4096, 16384, 65536, 262144)
COLOC_PROBES = 8             # the LDS probe bound (csrc/coloc.hpp kLdsProbes)
COLOC_PROBE_SWEEP = (1, 32)


def _coloc(args, torch, dev, g, bench, oshape):
    """The colocalization kernel (csrc/coloc.hip) at the config-2 deskewed shape on the three scenes of --label, labelled under
    connectivity 6: channel a is the scene's own float32 volume, channel b = 0.5 a + uniform noise, the thresholds their means
    (and uint16 images of both).  Per scene, each the median of 3 calls after a warm-up between HIP events (the tables zeroed
    outside the timed region): the kernel as shipped for float32 and uint16 channels, with the labels and without; the sweep of
    LDS slots, grid caps and probe bounds through the measurement entry (float32) and the plain form without an LDS table; two
    launches of lsr_label_intensity_f32 on the same labels (the nearest existing kernel: 16 bytes per voxel where this one reads
    12); and the kernel on the crop --coloc-crop.  torch's own formulation (index_add_ of the fifteen float64 terms) is NOT timed
    here: on the bead scene it did not finish within 7 minutes, neither on 8 planes nor on a (1, 1024, 1024) crop, where the
    kernel takes a fraction of a millisecond -- index_add_ sends every background voxel to one and the same float64 word.  The floor is a device copy of one int32 and two float32 volumes, which moves twice the bytes.
    Every form's counts must equal the shipped form's; the greatest relative difference of a float64 sum is recorded."""
    from shrimpy_amd import _lib, colocalize, segment

    reps = 3
    z, y, x = oshape
    n = z * y * x
    lds_slots, default_cap = colocalize.coloc_geometry()
    a, fa = torch.empty(oshape, dtype=torch.int32, device=dev), torch.empty(oshape, dtype=torch.float32, device=dev)
    b, fb, fc, fd = torch.empty_like(a), torch.empty_like(fa), torch.empty_like(fa), torch.empty_like(fa)

    def copies():
        b.copy_(a)
        fb.copy_(fa)
        fd.copy_(fc)

    class Records(list):
        """Every record is printed when it is made: a long run is never silent, and a stall shows where it is."""

        def append(self, r):
            print(json.dumps(r), flush=True)
            super().append(r)

    copy_ms = _median_ms(copies, reps, torch)
    records = Records()
    records.append({"kernel": "device copy of one int32 volume and two float32 volumes (torch copy_)", "grid": list(oshape), "ms": copy_ms,
                    "GBps": 24.0 * n / copy_ms / 1e6})
    del a, b, fa, fb, fc, fd
    torch.cuda.empty_cache()
    stream = _lib.stream_ptr(dev)
    record = colocalize.COLOC_DTYPE_F32.itemsize
    counts = [colocalize.COLOC_FIELDS.index(f) for f in colocalize.COLOC_COUNTS]
    sums = [i for i in range(16) if i not in counts]

    def geometry(cap, voxels=n):
        steps = -(-voxels // MOMENTS_STEP)
        span = -(-steps // min(steps, cap)) * MOMENTS_STEP
        return span, -(-voxels // span)

    def split(table):
        """(the four counts of every record, its twelve float64 sums)"""
        words = table.view(torch.int64).view(-1, record // 8)
        return words[:, counts].contiguous(), words[:, sums].contiguous().view(torch.float64)

    def timed(launch, table):
        return _timed_cleared(torch, launch, table.zero_, reps)

    def u16_of(vol):
        # scaled into 0 .. 65535, cut to 16 bits through int16 (same bits)
        scale = 65535.0 / max(float(vol.max().item()), 1e-30)
        return (vol.clamp(min=0.0) * scale).to(torch.int32).to(torch.int16).view(torch.uint16)

    for name, vol, threshold in _label_scenes(torch, dev, g, bench, oshape):
        labels, n_objects = segment.label_volume(vol, threshold, 6)
        vb = 0.5 * vol + torch.rand(oshape, device=dev, generator=g) * float(vol.mean().item())
        ta, tb = float(vol.mean().item()), float(vb.mean().item())
        ua, ub = u16_of(vol), u16_of(vb)
        uta, utb = float(ua.to(torch.float32).mean().item()), float(ub.to(torch.float32).mean().item())
        torch.cuda.empty_cache()
        base = {"input": name, "grid": list(oshape), "objects": n_objects, "foreground_fraction": float((labels != 0).sum().item()) / n,
                "thresholds": [ta, tb]}
        print(f"# {name}: {n_objects} objects", flush=True)
        table = torch.zeros(max(n_objects, 1) * record, dtype=torch.uint8, device=dev)
        span, blocks = geometry(default_cap)
        shipped = {"lds_slots": lds_slots, "lds_probes": COLOC_PROBES, "max_blocks": default_cap, "default": True,
                   "workgroups": blocks, "span_voxels": span}
        ms = timed(lambda: _lib.call("lsr_label_coloc_u16", labels.data_ptr(), ua.data_ptr(), ub.data_ptr(), z, y, x, n_objects, uta, utb,
                                     table.data_ptr(), 0, stream), table)
        records.append({**base, "kernel": "lsr_label_coloc_u16", **shipped, "thresholds": [uta, utb], "ms": ms, "bytes_per_voxel": 8.0,
                        "algorithmic_GBps": 8.0 * n / ms / 1e6, "times_the_copy": ms / copy_ms})
        ms_f32 = timed(lambda: _lib.call("lsr_label_coloc_f32", labels.data_ptr(), vol.data_ptr(), vb.data_ptr(), z, y, x, n_objects, ta,
                                         tb, table.data_ptr(), 0, stream), table)
        want_counts, want_sums = (t.clone() for t in split(table))
        records.append({**base, "kernel": "lsr_label_coloc_f32", **shipped, "ms": ms_f32, "bytes_per_voxel": 12.0,
                        "algorithmic_GBps": 12.0 * n / ms_f32 / 1e6, "times_the_copy": ms_f32 / copy_ms})
        forms = [(0, default_cap, 1)] + [(slots, cap, COLOC_PROBES) for slots in COLOC_SLOTS for cap in COLOC_CAPS]
        forms += [(lds_slots, default_cap, probes) for probes in COLOC_PROBE_SWEEP]
        for slots, cap, probes in forms:
            ms = timed(lambda: _lib.call("lsr_label_coloc_variant", labels.data_ptr(), vol.data_ptr(), vb.data_ptr(), 0, z, y, x,
                                         n_objects, ta, tb, table.data_ptr(), cap, slots, probes, stream), table)
            got_counts, got_sums = split(table)
            assert torch.equal(got_counts, want_counts), "a form of the kernel disagrees with the shipped one in a count"
            difference = float(((got_sums - want_sums).abs() / want_sums.abs().clamp(min=1e-300)).max().item()) if n_objects else 0.0
            span, blocks = geometry(cap)
            records.append({**base, "kernel": "lsr_label_coloc_variant (f32)" + (" (plain form: no LDS table)" if slots == 0 else ""),
                            "lds_slots": slots, "lds_probes": probes if slots else 0, "max_blocks": cap,
                            "default": (slots, cap, probes) == (lds_slots, default_cap, COLOC_PROBES), "workgroups": blocks,
                            "span_voxels": span, "ms": ms, "times_the_copy": ms / copy_ms,
                            "greatest_relative_difference_of_a_sum": difference})
        del want_counts, want_sums
        # without labels: the whole volume is one object
        one = torch.zeros(record, dtype=torch.uint8, device=dev)
        for cap in (0,) + COLOC_CAPS:
            span, blocks = geometry(cap or default_cap)
            ms = timed(lambda: _lib.call("lsr_label_coloc_f32", None, vol.data_ptr(), vb.data_ptr(), z, y, x, 1, ta, tb, one.data_ptr(),
                                         cap, stream), one)
            records.append({**base, "kernel": "lsr_label_coloc_f32 (labels = NULL)", "max_blocks": cap or default_cap, "default": cap == 0,
                            "workgroups": blocks, "span_voxels": span, "ms": ms, "bytes_per_voxel": 8.0,
                            "algorithmic_GBps": 8.0 * n / ms / 1e6, "times_the_copy": ms / copy_ms})
        ms = timed(lambda: _lib.call("lsr_label_coloc_u16", None, ua.data_ptr(), ub.data_ptr(), z, y, x, 1, uta, utb, one.data_ptr(), 0,
                                     stream), one)
        records.append({**base, "kernel": "lsr_label_coloc_u16 (labels = NULL)", "max_blocks": default_cap, "default": True, "ms": ms,
                        "bytes_per_voxel": 4.0, "algorithmic_GBps": 4.0 * n / ms / 1e6, "times_the_copy": ms / copy_ms})
        del ua, ub, one
        # the nearest existing kernel: one launch per channel
        tables = torch.zeros(2 * max(n_objects, 1) * segment.INTENSITY_DTYPE_F32.itemsize, dtype=torch.uint8, device=dev)
        half = tables.numel() // 2

        def two_launches():
            _lib.call("lsr_label_intensity_f32", labels.data_ptr(), vol.data_ptr(), z, y, x, n_objects, tables.data_ptr(), 0, stream)
            _lib.call("lsr_label_intensity_f32", labels.data_ptr(), vb.data_ptr(), z, y, x, n_objects, tables[half:].data_ptr(), 0, stream)

        ms = timed(two_launches, tables)
        records.append({**base, "kernel": "two launches of lsr_label_intensity_f32 (one per channel)", "ms": ms, "bytes_per_voxel": 16.0,
                        "times_the_copy": ms / copy_ms, "times_lsr_label_coloc_f32": ms / ms_f32})
        del tables
        # a crop: the size on which a formulation in torch's own operators would be tried
        cz, cy, cx = (min(int(v), full) for v, full in zip(args.coloc_crop.split(","), oshape))
        c_labels, c_a, c_b = (t[z // 2:z // 2 + cz, :cy, :cx].contiguous() for t in (labels, vol, vb))
        ms_crop = timed(lambda: _lib.call("lsr_label_coloc_f32", c_labels.data_ptr(), c_a.data_ptr(), c_b.data_ptr(), cz, cy, cx,
                                          n_objects, ta, tb, table.data_ptr(), 0, stream), table)
        records.append({**base, "grid": [cz, cy, cx], "kernel": "lsr_label_coloc_f32 on the crop", "ms": ms_crop})
        del c_labels, c_a, c_b, table, labels, vol, vb
        torch.cuda.empty_cache()
    stamp = {"sources": _lib.kernel_source_sha16(), "device": torch.cuda.get_device_name(dev), "reps": reps, "warmups": 1}
    path = ROOT / "profiles" / "coloc_config2.jsonl"
    with open(path, "a") as f:
        for r in records:
            f.write(json.dumps({**r, **stamp}) + "\n")


STATS_CAPS = (2048, 8192, 32768, 131072)
STATS_QUANTILES = (0.001, 0.01, 0.25, 0.5, 0.75, 0.99, 0.999)


def _stats(args, torch, dev, g, bench, oshape):
    """One digit pass of the whole-volume select (csrc/stats.hip) at the config-2 deskewed shape, float32 and uint16, on four
    scenes: the bench's bead scene, Bernoulli noise (p = 0.3, values 0 and 1), an all-zero volume and the bead scene with its
    outer quarter (an eighth of x on either side) set to exact 0.  Per scene and type, each the median of 3 calls after a warm-up
    between HIP events: pass 0 with the moment record and pass 1 with the prefixes the seven default quantiles reach, in both
    forms, the kept form over a sweep of the grid cap; stats.summary end to end (wall clock, its synchronisations included) and
    the rescale.  The floor is a device copy of the volume, which moves twice the bytes a pass reads.  Every form and cap must
    give the tables of the first.  Then what torch.quantile and torch.sort do on the full float32 volume and on a 16e6-voxel
    crop."""
    import time

    from shrimpy_amd import _lib
    from shrimpy_amd import stats as ST

    reps = 3
    n = oshape[0] * oshape[1] * oshape[2]
    geo = ST.geometry()

    class Records(list):
        def append(self, r):
            print(json.dumps(r), flush=True)
            super().append(r)

    records = Records()
    src = torch.empty(oshape, dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    copy_ms = {4: _median_ms(lambda: dst.copy_(src), reps, torch)}
    hsrc = torch.zeros(oshape, dtype=torch.int16, device=dev)
    hdst = torch.empty_like(hsrc)
    copy_ms[2] = _median_ms(lambda: hdst.copy_(hsrc), reps, torch)
    for size, ms in copy_ms.items():
        records.append({"kernel": f"device copy of one volume of {size}-byte voxels (torch copy_)", "grid": list(oshape), "ms": ms,
                        "GBps": 2.0 * size * n / ms / 1e6})
    del src, dst, hdst, hsrc
    torch.cuda.empty_cache()

    def scenes():
        vol = bench.synthetic_raw(oshape, 1000, dev)
        yield "bead scene (bench.synthetic_raw)", vol
        eighth = oshape[2] // 8
        vol[:, :, :eighth] = 0.0
        vol[:, :, oshape[2] - eighth:] = 0.0
        yield "bead scene, outer quarter exact 0", vol
        del vol
        yield "Bernoulli noise, p = 0.3", (torch.rand(oshape, device=dev, generator=g) < 0.3).to(torch.float32)
        yield "all zero", torch.zeros(oshape, dtype=torch.float32, device=dev)

    def u16_of(vol):
        scale = 65535.0 / max(float(vol.max().item()), 1e-30)
        return (vol.clamp(min=0.0) * scale).to(torch.int32).to(torch.int16).view(torch.uint16)

    for name, vol in scenes():
        for flat in (vol.reshape(-1), u16_of(vol).reshape(-1)):
            size = flat.element_size()
            kind = "f32" if size == 4 else "u16"
            base = {"input": name, "grid": list(oshape), "dtype": kind}
            table0, _ = ST._pass0(ST._Pool(flat))
            total = int(table0.astype(object).sum())
            state = sorted({ST._walk(table0, r)[0] for q in STATS_QUANTILES for r in ST._bracket(q, total)[:2]})[:geo["K"]]
            plans = {0: ([0], [0]), 1: (state, list(range(len(state))))}
            record = torch.zeros(ST.RECORD_WORDS, dtype=torch.int64, device=dev)
            first = {}
            for p, (prefixes, table_of) in plans.items():
                tables = torch.zeros(len(prefixes) * geo["bins"], dtype=torch.int64, device=dev)
                for form, form_name in ((ST.FORM_RUNS, "runs"), (ST.FORM_PLAIN, "plain")):
                    for cap in (0,) + (STATS_CAPS if form == ST.FORM_RUNS and kind == "f32" else ()):
                        def launch():
                            ST.digit_histogram(flat, p, prefixes, table_of, tables, record if p == 0 else None, cap, form)

                        def clear():
                            tables.zero_()
                            record.zero_()

                        ms = _timed_cleared(torch, launch, clear, reps)
                        got = tables.cpu().numpy().copy()
                        same = bool(np.array_equal(got, first.setdefault(p, got)))
                        records.append({**base, "kernel": f"lsr_digit_histogram_{kind}", "pass": p, "tables": len(prefixes), "form": form_name,
                                        "grid_cap": cap or geo["default_grid_cap"], "default": cap == 0, "ms": ms,
                                        "algorithmic_GBps": size * n / ms / 1e6, "times_the_copy": ms / copy_ms[size],
                                        "tables_equal_the_first": same})
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s = ST.summary(flat, STATS_QUANTILES)
            torch.cuda.synchronize()
            records.append({**base, "kernel": "stats.summary (7 quantiles + quartiles, moments), wall clock", "ms": (time.perf_counter() - t0) * 1e3,
                            "median": s["median"], "iqr": s["iqr"], "count": s["count"], "zero_fraction": float(((flat if size == 4 else flat.view(torch.int16)) == 0).sum().item()) / n})
            out = torch.empty(flat.shape, dtype=torch.float32, device=dev)
            ms = _median_ms(lambda: ST.rescale(flat, 1.0, 3.0, (0.0, 1.0), out), reps, torch)
            records.append({**base, "kernel": f"lsr_rescale_{kind}", "ms": ms, "algorithmic_GBps": (size + 4.0) * n / ms / 1e6})
            del out, tables, record
            torch.cuda.empty_cache()
        del flat
    # torch's own operators on the last scene's shape (values do not matter for what they accept)
    vol = torch.rand(oshape, device=dev, generator=g).reshape(-1)
    for what, count in (("the full volume", n), ("a crop of 16 000 000 voxels", 16_000_000)):
        part = vol[:count]
        for op_name, op in (("torch.quantile(v, 0.5)", lambda: torch.quantile(part, 0.5)), ("torch.sort(v)", lambda: torch.sort(part))):
            try:
                ms = _median_ms(op, reps, torch)
                records.append({"kernel": f"{op_name} on {what}", "voxels": count, "ms": ms})
            except Exception as e:       # (recorded: what torch does is the finding)
                records.append({"kernel": f"{op_name} on {what}", "voxels": count, "error": f"{type(e).__name__}: {str(e)[:300]}"})
            torch.cuda.empty_cache()
    stamp = {"sources": _lib.kernel_source_sha16(), "device": torch.cuda.get_device_name(dev), "reps": reps, "warmups": 1,
             "digit_bits": geo["digit_bits"], "K": geo["K"]}
    with open(ROOT / "profiles" / "stats_config2.jsonl", "a") as f:
        for r in records:
            f.write(json.dumps({**r, **stamp}) + "\n")


def _edt(args, torch, dev, g, bench, oshape):
    """Distance transform (csrc/edt.hip) at the config-2 deskewed shape: every launch of lsr_edt_f32 on its own (HIP events
    between them: lsr_edt_profile_f32), both outputs asked for, unit sampling, for three inputs -- the bench's bead scene at its
    multi-Otsu threshold (sparse foreground: short envelopes), Bernoulli foreground at p = 0.3 and an all-foreground volume with
    one background voxel (one site: every line's envelope is one parabola, the longest distances).  Beside them the bytes per
    voxel each launch must move and a device copy of an int32 volume of the same size in the same run."""
    from shrimpy_amd import _lib, dynatrack

    reps = 5
    z, y, x = oshape
    n = z * y * x
    nearest = torch.empty(oshape, dtype=torch.int32, device=dev)
    other = torch.empty_like(nearest)
    copy_ms = _median_ms(lambda: other.copy_(nearest), reps, torch)
    del other
    records = [{"kernel": "device copy of an int32 volume (torch copy_)", "grid": list(oshape), "ms": copy_ms,
                "GBps": 8.0 * n / copy_ms / 1e6}]
    dist = torch.empty(oshape, dtype=torch.float32, device=dev)
    scratch_bytes = _lib.call_value("lsr_edt_scratch_bytes", z, y, x)
    scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
    sampling = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
    ms3 = (ctypes.c_float * 3)()

    def scenes():
        vol = bench.synthetic_raw(oshape, 1000, dev)
        yield "bead scene (bench.synthetic_raw) at its multi-Otsu threshold", vol, float(dynatrack._multiotsu_threshold(vol, 0))
        del vol
        yield "Bernoulli foreground, p = 0.3", torch.rand(oshape, device=dev, generator=g), 0.7
        one = torch.ones(oshape, dtype=torch.float32, device=dev)
        one[z // 2, y // 2, x // 2] = 0.0
        yield "all foreground but one voxel", one, 0.5

    for name, vol, threshold in scenes():
        times = []
        for _ in range(reps + 1):
            _lib.call("lsr_edt_profile_f32", vol.data_ptr(), z, y, x, ctypes.c_float(threshold), 0, sampling, dist.data_ptr(),
                      nearest.data_ptr(), scratch.data_ptr(), ms3, _lib.stream_ptr(dev))
            times.append(list(ms3))
        med = np.median(np.asarray(times[1:]), axis=0)
        base = {"input": name, "grid": list(oshape), "threshold": threshold, "sampling": [1.0, 1.0, 1.0],
                "site_fraction": float((dist == 0).sum().item()) / n, "max_distance": float(dist.max().item()),
                "scratch_bytes": scratch_bytes}
        for launch, ms in zip(EDT_LAUNCHES, med):
            bpv = EDT_BYTES_PER_VOXEL[launch]
            records.append({**base, "kernel": f"lsr_edt_f32: {launch}", "ms": float(ms), "bytes_per_voxel": bpv,
                            "algorithmic_GBps": bpv * n / float(ms) / 1e6, "copy_time_ratio": float(ms) / (copy_ms * bpv / 8.0)})
        records.append({**base, "kernel": "lsr_edt_f32: all three launches", "ms": float(med.sum()),
                        "Mvox_per_s": n / float(med.sum()) / 1e3})
        del vol
    stamp = {"sources": _lib.kernel_source_sha16(), "device": torch.cuda.get_device_name(dev), "reps": reps, "warmups": 1}
    path = ROOT / "profiles" / "edt_config2.jsonl"
    with open(path, "a") as f:
        for r in records:
            line = json.dumps({**r, **stamp})
            print(line, flush=True)
            f.write(line + "\n")


def _morphology(args, torch, dev, g, bench, oshape):
    """Grey morphology (csrc/morphology.hip) at the config-2 deskewed shape on the bench's bead scene: erosion (3 launches),
    opening (6) and white top-hat (6, the subtraction fused into the last) at cubic half-widths 5, 25, 50 and, if the cap allows,
    128, and the erosion along z, y and x alone (one launch each); a launch moves 8 algorithmic bytes per voxel (one read, one
    write; the top-hat's last one 12).  Beside them, in the same
    run, the floor -- a device copy of one volume, the same 8 bytes per voxel -- and, where the half-width is at most 64, the
    three launches of lsr_local_max_candidates_f32 at the same half-width: the same x and y passes (two volumes written) and
    the z walk with the peak test as its sink."""
    from shrimpy_amd import _lib, morphology

    reps = 3
    z, y, x = oshape
    n = z * y * x
    vol = bench.synthetic_raw(oshape, 1000, dev)
    out = torch.empty_like(vol)
    copy_ms = _median_ms(lambda: out.copy_(vol), reps, torch)
    records = [{"kernel": "device copy of a float32 volume (torch copy_)", "grid": list(oshape), "ms": copy_ms,
                "GBps": 8.0 * n / copy_ms / 1e6}]
    cap = morphology.max_half_width()
    scratch = torch.empty(_lib.call_value("lsr_grey_morph_scratch_bytes", z, y, x), dtype=torch.uint8, device=dev)
    nbytes = ctypes.c_int64(0)
    _lib.call("lsr_local_max_scratch_bytes", z, y, x, ctypes.byref(nbytes))
    assert nbytes.value <= scratch.numel()                  # (two float volumes as well: the same buffer serves)
    capacity = 1 << 20
    index = torch.empty(capacity, dtype=torch.int64, device=dev)
    value = torch.empty(capacity, dtype=torch.float32, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    for r in (5, 25, 50, 128):
        if r > cap:
            continue
        base = {"input": "bead scene (bench.synthetic_raw)", "grid": list(oshape), "half_widths": [r, r, r]}
        for name, launches in (("grey_erosion", 3), ("grey_opening", 6), ("white_tophat", 6)):
            def launch(op=morphology.OPS[name]):
                _lib.call("lsr_grey_morph_f32", vol.data_ptr(), out.data_ptr(), z, y, x, r, r, r, op, scratch.data_ptr(),
                          _lib.stream_ptr(dev))
            ms = _median_ms(launch, reps, torch)
            bpv = 8.0 * launches + (4.0 if name == "white_tophat" else 0.0)
            records.append({**base, "kernel": f"lsr_grey_morph_f32: {name} ({launches} launches)", "ms": ms,
                            "ms_per_launch": ms / launches, "bytes_per_voxel": bpv, "algorithmic_GBps": bpv * n / ms / 1e6,
                            "copy_time_ratio_per_launch": ms / launches / copy_ms})
        for axis, name in enumerate("zyx"):                 # one launch each: the window on one axis only
            rr = [r if a == axis else 0 for a in range(3)]

            def one(rr=rr):
                _lib.call("lsr_grey_morph_f32", vol.data_ptr(), out.data_ptr(), z, y, x, *rr, 0, scratch.data_ptr(),
                          _lib.stream_ptr(dev))
            ms = _median_ms(one, reps, torch)
            records.append({**base, "half_widths": rr, "kernel": f"lsr_grey_morph_f32: grey_erosion along {name} (1 launch)",
                            "ms": ms, "bytes_per_voxel": 8.0, "algorithmic_GBps": 8.0 * n / ms / 1e6,
                            "copy_time_ratio_per_launch": ms / copy_ms})
        if r <= 64:
            def detect():
                _lib.call("lsr_local_max_candidates_f32", vol.data_ptr(), z, y, x, r, r, r, ctypes.c_float(3.0e38), index.data_ptr(),
                          value.data_ptr(), capacity, count.data_ptr(), scratch.data_ptr(), _lib.stream_ptr(dev))
            ms = _median_ms(detect, reps, torch)
            records.append({**base, "kernel": "lsr_local_max_candidates_f32 (3 launches, 2 volumes written)", "ms": ms,
                            "ms_per_launch": ms / 3, "ms_per_volume_written": ms / 2,
                            "copy_time_ratio_per_launch": ms / 3 / copy_ms})
    stamp = {"sources": _lib.kernel_source_sha16(), "device": torch.cuda.get_device_name(dev), "reps": reps, "warmups": 1}
    path = ROOT / "profiles" / "morphology_config2.jsonl"
    with open(path, "a") as f:
        for rec in records:
            line = json.dumps({**rec, **stamp})
            print(line, flush=True)
            f.write(line + "\n")


def _flatfield(args, torch, dev, g, bench):
    """The three median variants of the affine-and-deskew section (same stacks, same generator), each repeated."""
    from shrimpy_amd import _lib
    from shrimpy_amd.flatfield import flat_field_pattern

    raw_shape = bench.WORKLOADS["config2"][1]
    counts = torch.randint(80, 600, raw_shape, device=dev, generator=g).to(torch.float32)
    records = []
    stamp = {"label": args.tag, "sources": _lib.kernel_source_sha16(), "device": torch.cuda.get_device_name(dev),
             "reps": args.reps, "warmups": 1}

    def measure(name, stack, passes, itemsize):
        for rep in range(args.flatfield_repeats):
            ms = timed(lambda: flat_field_pattern(stack), args.reps)
            records.append({"kernel": name, "raw": list(raw_shape), "repetition": rep, "ms": ms,
                            "passes_GBps": passes * itemsize * stack.numel() / ms / 1e6, **stamp})
            print(json.dumps(records[-1]), flush=True)

    measure("flat_median_kernel (+ mean), integer counts", counts, 2, 4.0)
    raw16 = counts.to(torch.uint16)
    counts += torch.rand(raw_shape, device=dev, generator=g)              # continuous values: 4 passes
    measure("flat_median_kernel (+ mean), float values", counts, 4, 4.0)
    del counts
    measure("flat_median_kernel<U16> (+ mean)", raw16, 2, 2.0)
    with open(ROOT / "profiles" / "flatfield_pin.jsonl", "a") as f:
        for rec in records:
            f.write(json.dumps(rec) + "\n")


def _rank(args, torch, dev, g, bench, oshape):
    """Rank filters (csrc/rank.hip) at the config-2 deskewed shape on the bench's bead scene: one launch that moves 8 algorithmic
    bytes per voxel (one read, one write; remove_bright 12).  The median at half-widths (0, 1, 1) and (1, 1, 1) -- kernels that
    sort the window in registers -- and at (2, 2, 2) and (3, 3, 3) -- the generic kernel, which reads the window from LDS on
    each of the 32 sweeps of its bisection --, the first two again with variant = 1 (the generic kernel), and remove_bright at (0, 1, 1).  Beside
    them, in the same run, the floor -- a device copy of one volume, the same 8 bytes per voxel -- and grey_erosion at the same
    half-widths: rank 0 is the same function away from the borders, which is asserted on the interior before anything is timed."""
    from shrimpy_amd import _lib

    reps = 3
    z, y, x = oshape
    n = z * y * x
    vol = bench.synthetic_raw(oshape, 1000, dev)
    out = torch.empty_like(vol)
    copy_ms = _median_ms(lambda: out.copy_(vol), reps, torch)
    records = [{"kernel": "device copy of a float32 volume (torch copy_)", "grid": list(oshape), "ms": copy_ms,
                "GBps": 8.0 * n / copy_ms / 1e6}]
    scratch = torch.empty(_lib.call_value("lsr_grey_morph_scratch_bytes", z, y, x), dtype=torch.uint8, device=dev)
    eroded = torch.empty_like(vol)

    def rank_call(r, rank, op, threshold, variant):
        _lib.call("lsr_rank_filter_f32", vol.data_ptr(), out.data_ptr(), z, y, x, *r, rank, op, ctypes.c_float(threshold), variant,
                  _lib.stream_ptr(dev))

    def erode(r):
        _lib.call("lsr_grey_morph_f32", vol.data_ptr(), eroded.data_ptr(), z, y, x, *r, 0, scratch.data_ptr(), _lib.stream_ptr(dev))

    for r in ((0, 1, 1), (1, 1, 1), (2, 2, 2), (3, 3, 3)):
        window = (2 * r[0] + 1) * (2 * r[1] + 1) * (2 * r[2] + 1)
        base = {"input": "bead scene (bench.synthetic_raw)", "grid": list(oshape), "half_widths": list(r), "window": window}
        rank_call(r, 0, 0, 0.0, 0)
        erode(r)
        inner = tuple(slice(k, -k) if k else slice(None) for k in r)
        assert torch.equal(out[inner], eroded[inner]), f"rank 0 and grey_erosion differ in the interior at {r}"
        variants = (0, 1) if max(r) <= 1 else (0,)
        for variant in variants:
            ms = _median_ms(lambda: rank_call(r, window // 2, 0, 0.0, variant), reps, torch)
            path = "registers" if variant == 0 and max(r) <= 1 else "generic"
            records.append({**base, "kernel": f"lsr_rank_filter_f32: median ({path} path, variant = {variant})", "variant": variant,
                            "path": path, "ms": ms, "bytes_per_voxel": 8.0, "algorithmic_GBps": 8.0 * n / ms / 1e6,
                            "copy_time_ratio": ms / copy_ms})
        if r == (0, 1, 1):
            ms = _median_ms(lambda: rank_call(r, window // 2, 1, 200.0, 0), reps, torch)
            records.append({**base, "kernel": "lsr_rank_filter_f32: remove_bright, threshold 200 (registers path, variant = 0)",
                            "variant": 0, "path": "registers", "ms": ms, "bytes_per_voxel": 12.0,
                            "algorithmic_GBps": 12.0 * n / ms / 1e6, "copy_time_ratio": ms / copy_ms})
        launches = sum(1 for k in r if k)
        ms = _median_ms(lambda: erode(r), reps, torch)
        records.append({**base, "kernel": f"lsr_grey_morph_f32: grey_erosion ({launches} launches)", "ms": ms,
                        "bytes_per_voxel": 8.0 * launches, "copy_time_ratio": ms / copy_ms})
    stamp = {"sources": _lib.kernel_source_sha16(), "device": torch.cuda.get_device_name(dev), "reps": reps, "warmups": 1}
    path = ROOT / "profiles" / "rank_config2.jsonl"
    with open(path, "a") as f:
        for rec in records:
            line = json.dumps({**rec, **stamp})
            print(line, flush=True)
            f.write(line + "\n")


def _hessian(args, torch, dev, g, bench, oshape):
    """Hessian-eigenvalue responses (csrc/hessian.hip) at the config-2 deskewed shape on the bench's bead scene blurred at sigma
    1.5: one launch that moves 8 algorithmic bytes per voxel (one read, one write; 12 with accumulate) and does its arithmetic in
    float64.  Beside it, in the same run, the floor -- a device copy of one volume --, the three blur launches of one scale,
    enhance at three sigmas end to end (three blurs and three launches, two blur buffers and the output allocated inside), the
    torch fallback (torch.gradient nine times, torch.linalg.eigvalsh on float64 matrices) on a shape it fits in memory, and the
    worst eigenvalue error of the device against np.gradient / np.linalg.eigvalsh in float64 on a crop of the scene, in units
    of the bound 2^-23 scale ||H||_F."""
    from shrimpy_amd import _lib, hessian

    reps = 3
    z, y, x = oshape
    n = z * y * x
    vol = bench.synthetic_raw(oshape, 1000, dev)
    out = torch.empty_like(vol)
    copy_ms = _median_ms(lambda: out.copy_(vol), reps, torch)
    records = [{"kernel": "device copy of a float32 volume (torch copy_)", "grid": list(oshape), "ms": copy_ms,
                "GBps": 8.0 * n / copy_ms / 1e6}]
    sigma, sampling = 1.5, (1.0, 1.0, 1.0)
    buffers = hessian._buffers(vol)
    blur_ms = _median_ms(lambda: hessian._blur(vol, sigma, sampling, buffers), reps, torch)
    records.append({"kernel": "lsr_blur_reflect_f32: the three launches of one scale (taps made inside)", "grid": list(oshape),
                    "sigma": sigma, "radii": list(hessian.blur_radii(sigma, sampling)), "ms": blur_ms, "bytes_per_voxel": 24.0,
                    "copy_time_ratio": blur_ms / copy_ms})
    blurred = hessian._blur(vol, sigma, sampling, buffers)

    def respond(measure, accumulate):
        _lib.call("lsr_hessian_response_f32", blurred.data_ptr(), out.data_ptr(), z, y, x, *(ctypes.c_double(s) for s in sampling),
                  ctypes.c_double(sigma * sigma), hessian.MEASURES[measure], 0, accumulate, _lib.stream_ptr(dev))

    base = {"input": "bead scene (bench.synthetic_raw) blurred at sigma 1.5", "grid": list(oshape)}
    for measure in ("e1", "tube", "log"):
        for accumulate in (0, 1):
            out.zero_()
            ms = _median_ms(lambda: respond(measure, accumulate), reps, torch)
            bytes_per_voxel = 12.0 if accumulate else 8.0
            records.append({**base, "kernel": f"lsr_hessian_response_f32: {measure}, accumulate = {accumulate}", "measure": measure,
                            "accumulate": accumulate, "ms": ms, "bytes_per_voxel": bytes_per_voxel,
                            "algorithmic_GBps": bytes_per_voxel * n / ms / 1e6, "copy_time_ratio": ms / copy_ms})
    sigmas = (1.0, 1.5, 2.0)
    ms = _median_ms(lambda: hessian.enhance(vol, "tube", sigmas, sampling), reps, torch)
    records.append({"kernel": "hessian.enhance: tube at three sigmas end to end (9 blur launches, 3 kernel launches)",
                    "input": "bead scene (bench.synthetic_raw)", "grid": list(oshape), "sigmas": list(sigmas), "ms": ms,
                    "copy_time_ratio": ms / copy_ms})
    # the torch fallback, on a crop it fits in memory (the (Z, Y, X, 3, 3) float64 matrices of the whole volume are 57 GB)
    small = (64, 256, 256)
    crop = blurred[:small[0], :small[1], :small[2]].contiguous()

    def fallback():
        g64 = crop.double()
        first = torch.gradient(g64)
        H = torch.empty(small + (3, 3), dtype=torch.float64, device=dev)
        for a in range(3):
            for b in range(a, 3):
                H[..., a, b] = H[..., b, a] = torch.gradient(first[a], dim=b)[0]
        return (sigma * sigma * torch.linalg.eigvalsh(H)).float()

    small_out = torch.empty_like(crop)

    def small_kernel():
        _lib.call("lsr_hessian_response_f32", crop.data_ptr(), small_out.data_ptr(), *small, *(ctypes.c_double(s) for s in sampling),
                  ctypes.c_double(sigma * sigma), 0, 0, 0, _lib.stream_ptr(dev))

    records.append({"kernel": "torch fallback: torch.gradient x 9 + torch.linalg.eigvalsh (float64), all three eigenvalues",
                    "grid": list(small), "ms": _median_ms(fallback, reps, torch)})
    records.append({"kernel": "lsr_hessian_response_f32: e1, accumulate = 0 (one of the three launches the fallback stands for)",
                    "grid": list(small), "ms": _median_ms(small_kernel, reps, torch)})
    # the worst eigenvalue error against numpy in float64, in units of 2^-23 scale ||H||_F, on a crop
    tiny = (40, 48, 56)
    g = blurred[:tiny[0], :tiny[1], :tiny[2]].contiguous()
    g64 = g.cpu().numpy().astype(np.float64)
    first = np.gradient(g64)
    H = np.empty(tiny + (3, 3))
    for a in range(3):
        for b in range(a, 3):
            H[..., a, b] = H[..., b, a] = np.gradient(first[a], axis=b)
    want, norm = sigma * sigma * np.linalg.eigvalsh(H), sigma * sigma * np.sqrt((H * H).sum(axis=(-1, -2)))
    worst = 0.0
    tiny_out = torch.empty_like(g)
    for k in range(3):
        _lib.call("lsr_hessian_response_f32", g.data_ptr(), tiny_out.data_ptr(), *tiny, *(ctypes.c_double(s) for s in sampling),
                  ctypes.c_double(sigma * sigma), k, 0, 0, _lib.stream_ptr(dev))
        err = np.abs(tiny_out.cpu().numpy().astype(np.float64) - want[..., k])
        keep = norm > 0
        worst = max(worst, float(np.max(err[keep] / (2.0 ** -23 * norm[keep]))))
        assert np.all(err <= 2.0 ** -23 * norm), "the eigenvalue bound"
    records.append({"kernel": "lsr_hessian_response_f32: worst eigenvalue error against np.gradient / np.linalg.eigvalsh (float64)",
                    "grid": list(tiny), "worst_error_over_bound": worst, "bound": "2^-23 scale ||H||_F"})
    stamp = {"sources": _lib.kernel_source_sha16(), "device": torch.cuda.get_device_name(dev), "reps": reps, "warmups": 1}
    path = ROOT / "profiles" / "hessian_config2.jsonl"
    with open(path, "a") as f:
        for rec in records:
            line = json.dumps({**rec, **stamp})
            print(line, flush=True)
            f.write(line + "\n")


def _mi(args, torch, dev, g, bench, shape):
    """Mutual-information metric (csrc/estimate_mi.hip): one joint-histogram launch (the entry's two memsets included) and
    one gradient launch under the config-3 registration matrix.  Algorithmic bytes: 4 per sampled target voxel plus the
    moving voxels the samples touch (at most the whole volume) -- reported against the copy rate of this card in this run.
    Torch formulation of the histogram: grid_sample (trilinear, float32 coordinates) slab by slab, the bin rule in tensor
    ops, two weighted bincounts per slab."""
    from shrimpy_amd import _lib, estimate

    reps = 5
    m = bench.registration_matrix()
    m12 = _lib.matrix12(m[:3])
    z, y, x = shape
    centre = np.array([(n - 1) / 2 for n in shape])
    c3, scale = centre.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), max(shape) / 2
    d = ctypes.c_double
    rows, width = _lib.call_value("lsr_affine_mi_gradient_blocks"), _lib.call_value("lsr_affine_mi_gradient_size")
    partial = torch.empty((rows, width), dtype=torch.float64, device=dev)
    records = []

    def torch_histogram(mov, tgt, stride, bins, t_lo, t_hi, m_lo, m_hi, slab=16):
        mt = torch.as_tensor(m[:3], dtype=torch.float32, device=dev)
        ys = torch.arange(0, y, stride, device=dev, dtype=torch.float32)
        xs = torch.arange(0, x, stride, device=dev, dtype=torch.float32)
        size = torch.tensor([x - 1, y - 1, z - 1], dtype=torch.float32, device=dev)
        hist = torch.zeros(bins * bins + 1, dtype=torch.float64, device=dev)
        for z0 in range(0, z, slab * stride):
            zs = torch.arange(z0, min(z, z0 + slab * stride), stride, device=dev, dtype=torch.float32)
            zz, yy, xx = torch.meshgrid(zs, ys, xs, indexing="ij")
            coords = [mt[r, 0] * zz + mt[r, 1] * yy + mt[r, 2] * xx + mt[r, 3] for r in range(3)]
            ok = ((coords[0] >= 0) & (coords[0] < z - 1) & (coords[1] >= 0) & (coords[1] < y - 1) & (coords[2] >= 0)
                  & (coords[2] < x - 1))
            grid = torch.stack([coords[2], coords[1], coords[0]], dim=-1) / size * 2 - 1
            mval = torch.nn.functional.grid_sample(mov[None, None], grid[None], mode="bilinear", align_corners=True)[0, 0][ok]
            tv = tgt[z0:min(z, z0 + slab * stride):stride, ::stride, ::stride][ok]
            a = torch.clamp(torch.floor((tv - t_lo) * bins / (t_hi - t_lo)), 0, bins - 1).long()
            u = torch.clamp((mval - m_lo) * (bins - 1) / (m_hi - m_lo), 0, bins - 1)
            b0 = torch.clamp(torch.floor(u), max=bins - 2)
            f = (u - b0).double()
            cell = a * bins + b0.long()
            hist += torch.bincount(cell, weights=1 - f, minlength=bins * bins + 1)
            hist += torch.bincount(cell + 1, weights=f, minlength=bins * bins + 1)
        return hist[:-1].reshape(bins, bins)

    for label in ("bench.synthetic_raw (background-dominated)", "uniform noise (all cells)"):
        if label.startswith("bench"):
            mov = bench.synthetic_raw(shape, 3000, dev)
            tgt = bench.synthetic_raw(shape, 3001, dev)
        else:
            mov = torch.empty(shape, dtype=torch.float32, device=dev).uniform_(0.0, 1000.0, generator=g)
            tgt = torch.empty(shape, dtype=torch.float32, device=dev).uniform_(0.0, 1000.0, generator=g)
        t_lo, t_hi, m_lo, m_hi = float(tgt.min()), float(tgt.max()), float(mov.min()), float(mov.max())
        other = torch.empty_like(mov)

        def copy_both():
            other.copy_(mov)
            other.copy_(tgt)

        copy_both()
        copy_ms = _median_ms(copy_both, reps, torch)
        copy_gbps = 16.0 * mov.numel() / copy_ms / 1e6
        del other
        records.append({"kernel": "device copy of the two volumes (torch copy_)", "input": label, "grid": list(shape),
                        "ms": copy_ms, "GBps": copy_gbps})
        for stride in (1, 4):
            st = (ctypes.c_int * 3)(stride, stride, stride)
            for bins in (32, 64):
                out = torch.zeros((bins * bins + 1,), dtype=torch.int64, device=dev)
                head = (mov.data_ptr(), z, y, x, tgt.data_ptr(), z, y, x, m12, st)
                tail = (bins, d(t_lo), d(t_hi), d(m_lo), d(m_hi))

                def histogram():
                    _lib.call("lsr_affine_joint_histogram_f32", *head, *tail, out.data_ptr(), out.data_ptr() + 8 * bins * bins,
                              _lib.stream_ptr(dev))

                histogram()
                hist_ms = _median_ms(histogram, reps, torch)
                host = out.cpu().numpy()
                n = int(host[-1])
                hist = host[:-1].reshape(bins, bins).astype(np.float64)
                dl = torch.as_tensor(estimate._mi_dl(hist)).to(dev)

                def gradient():
                    _lib.call("lsr_affine_mi_gradient_f32", *head, c3, d(scale), *tail, dl.data_ptr(), partial.data_ptr(),
                              _lib.stream_ptr(dev))

                gradient()
                grad_ms = _median_ms(gradient, reps, torch)
                samples = -(-z // stride) * -(-y // stride) * -(-x // stride)
                nbytes = 4.0 * samples + 4.0 * min(mov.numel(), 8 * samples)
                rec = {"kernel": "lsr_affine_joint_histogram_f32 / lsr_affine_mi_gradient_f32", "input": label, "grid": list(shape),
                       "stride": stride, "bins": bins, "samples": samples, "counted": n,
                       "largest_cell_share": float(hist.max() / max(hist.sum(), 1.0)), "nonzero_cells": int((hist > 0).sum()),
                       "histogram_ms": hist_ms, "gradient_ms": grad_ms, "histogram_Gsamples_per_s": samples / hist_ms / 1e6,
                       "gradient_Gsamples_per_s": samples / grad_ms / 1e6,
                       "histogram_frac_of_copy_rate": nbytes / hist_ms / 1e6 / copy_gbps,
                       "mutual_information": estimate.mutual_information(hist)}
                if bins == 32:
                    fn = lambda: torch_histogram(mov, tgt, stride, bins, t_lo, t_hi, m_lo, m_hi)  # noqa: E731
                    ref = fn()
                    torch_ms = _median_ms(fn, reps, torch)
                    rec.update({"torch_grid_sample_bincount_ms": torch_ms, "speedup_over_torch": torch_ms / hist_ms,
                                "torch_total_over_kernel_total": float(ref.sum().item() * 65536.0 / max(hist.sum(), 1.0)),
                                "max_cell_difference_from_torch_in_samples": float(np.abs(ref.cpu().numpy() - hist / 65536.0).max())})
                    del ref
                records.append(rec)
                print(json.dumps(rec), flush=True)
        del mov, tgt
        torch.cuda.empty_cache()
    stamp = {"sources": _lib.kernel_source_sha16(), "device": torch.cuda.get_device_name(dev), "reps": reps, "warmups": 2,
             "library": str(_lib.LIB_PATH.name)}
    path = ROOT / "profiles" / "mi_config3.jsonl"
    with open(path, "a") as f:
        for r in records:
            f.write(json.dumps({**r, **stamp}) + "\n")


def _peaks(args, torch, dev, g, oshape):
    """Bead detection (csrc/peaks.hip): the three launches of lsr_local_max_candidates_f32 -- the grey morphology's x and y
    dilation passes and its z walk with the peak test as the sink -- on a smoothed Poisson volume with a few hundred beads,
    per min_distance; 24 algorithmic bytes per voxel (x reads s and writes A, y reads A and writes B, z reads B and s: every
    pass reads its source once, as one stream).  --peaks-host: scipy's maximum_filter over the same window on the host, the step a user
    without this kernel would run."""
    import ctypes
    import time

    from shrimpy_amd import _lib, psf

    z, y, x = oshape
    vol = torch.poisson(torch.full(oshape, 100.0, device=dev), generator=g)
    n = vol.numel()
    beads = torch.randint(0, n, (400,), device=dev, generator=g)
    vol.view(-1)[beads] += 30000.0
    ms = timed(lambda: psf.smooth(vol, 3), args.reps)
    print(json.dumps({"kernel": "lsr_box_smooth_f32, 3 taps per axis (3 launches, float64 between them)", "grid": oshape, "ms": ms,
                      "algorithmic_GBps": 40.0 * n / ms / 1e6}), flush=True)
    s = psf.smooth(vol, 3)
    del vol
    nbytes = ctypes.c_int64(0)
    _lib.call("lsr_local_max_scratch_bytes", z, y, x, ctypes.byref(nbytes))
    scratch = torch.empty(nbytes.value // 4, dtype=torch.float32, device=dev)
    capacity = 1 << 20
    index = torch.empty(capacity, dtype=torch.int64, device=dev)
    value = torch.empty(capacity, dtype=torch.float32, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    for r in (5, 10, 25, 50):
        def launch():
            _lib.call("lsr_local_max_candidates_f32", s.data_ptr(), z, y, x, r, r, r, ctypes.c_float(200.0), index.data_ptr(),
                      value.data_ptr(), capacity, count.data_ptr(), scratch.data_ptr(), _lib.stream_ptr(dev))
        ms = timed(launch, args.reps)
        print(json.dumps({"kernel": "lsr_local_max_candidates_f32 (3 launches)", "grid": oshape, "min_distance": r,
                          "threshold_abs": 200.0, "peaks": int(count.item()), "ms": ms, "Mvox_per_s": n / ms / 1e3,
                          "algorithmic_GBps": 24.0 * n / ms / 1e6, "frac_of_8TBps": 24.0 * n / ms / 1e6 / 8000}), flush=True)
    if args.peaks_host:
        from scipy import ndimage

        host = s.cpu().numpy()
        del s, scratch
        for r in (10, 50):
            t0 = time.perf_counter()
            m = ndimage.maximum_filter(host, size=2 * r + 1, mode="constant", cval=-np.inf)
            found = int(np.count_nonzero((host == m) & (host >= 200.0)))
            sec = time.perf_counter() - t0
            print(json.dumps({"kernel": "scipy.ndimage.maximum_filter + compare (host)", "grid": oshape, "min_distance": r,
                              "maxima": found, "ms": sec * 1e3, "Mvox_per_s": n / sec / 1e6}), flush=True)


def _rl_accel(args, torch, dev, g, oshape):
    """Accelerated RL (csrc/rl_accel.hip): the two launches alone, between the fused plan's padded working volumes as an
    iteration runs them (16 and 12 algorithmic bytes per voxel), then per route -- fused separable 9x7x7, ky (x) kzx
    9x7x7 (a Gaussian turned 30 degrees in (z, x)), Fourier 15x19x19 -- the wall time of 20 plain iterations and of 9, 10
    and 15 accelerated ones, all in this run."""
    from shrimpy_amd import _lib
    from shrimpy_amd.deconvolve import PaddedVolume, make_plan
    from shrimpy_amd.rl_loop import AccelState, DeviceBackend
    from shrimpy_amd.pipeline import gaussian_psf_factors

    y = torch.poisson(torch.full(oshape, 100.0, device=dev), generator=g)
    ks = gaussian_psf_factors((9, 7, 7), (2.0, 1.2, 1.2))
    n = y.numel()
    out = torch.empty_like(y)

    def grid_psf(size, tilt):
        zz, yy, xx = np.meshgrid(*[np.arange(m) - m // 2 for m in size], indexing="ij")
        c, s = np.cos(np.deg2rad(tilt)), np.sin(np.deg2rad(tilt))
        zr, xr = c * zz + s * xx, -s * zz + c * xx
        w = np.exp(-0.5 * ((zr / (size[0] / 4.5)) ** 2 + (yy / (size[1] / 5.8)) ** 2 + (xr / (size[2] / 5.8)) ** 2))
        return (w / w.sum()).astype(np.float32)

    routes = (("fused separable 9x7x7", dict(psf=None, psf_factors=ks)),
              ("ky (x) kzx 9x7x7", dict(psf=grid_psf((9, 7, 7), 30.0))),
              ("Fourier 15x19x19", dict(psf=grid_psf((15, 19, 19), 30.0), method="fft")))
    for route, kw in routes:
        plan = make_plan(oshape, kw.pop("psf"), dev, **kw)
        if route.startswith("fused"):
            plan(y, iterations=2, out=out)                               # fills both working volumes
            a, b = plan._scratch()
            third = PaddedVolume(oshape, plan._path.pad_psf_shape, dev)
            acc = AccelState(DeviceBackend(oshape, dev), 3, torch.zeros_like(y))
            tri = lambda v: (v.logical_ptr(), v.pitch, v.plane)         # noqa: E731
            z, yy, xx = oshape
            d = acc.dots.data_ptr()
            launches = (
                ("accel dots launch", 16.0, lambda: _lib.call(
                    "lsr_rl_accel_dots_f32", *tri(b), *tri(a), acc.g.data_ptr(), z, yy, xx, 0, d + 16, acc.work.data_ptr(),
                    _lib.stream_ptr(dev))),
                ("accel dots launch (first: g not read)", 12.0, lambda: _lib.call(
                    "lsr_rl_accel_dots_f32", *tri(b), *tri(a), acc.g.data_ptr(), z, yy, xx, 1, d, acc.work.data_ptr(),
                    _lib.stream_ptr(dev))),
                ("accel predict launch", 12.0, lambda: _lib.call(
                    "lsr_rl_accel_predict_f32", *tri(b), *tri(third), z, yy, xx, d + 16, d + 8, None, _lib.stream_ptr(dev))))
            for label, nbytes, launch in launches:
                ms = timed(launch, args.reps)
                print(json.dumps({"kernel": label, "grid": oshape, "ms": ms, "bytes_per_voxel": nbytes,
                                  "ns_per_GB": ms * 1e6 / (nbytes * n / 1e9), "algorithmic_GBps": nbytes * n / ms / 1e6,
                                  "frac_of_8TBps": nbytes * n / ms / 1e6 / 8000}), flush=True)
            del third, acc
        walls = {}
        for label, iters, kw2 in (("plain", 20, {}), ("accelerated", 9, dict(acceleration="biggs-andrews")),
                                  ("accelerated", 10, dict(acceleration="biggs-andrews")),
                                  ("accelerated", 15, dict(acceleration="biggs-andrews")), ("plain", 20, {})):
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            plan(y, iterations=2, out=out, **kw2)                        # allocations and first-use costs
            torch.cuda.synchronize()
            plan(y, iterations=iters, out=out, events=ev, **kw2)
            torch.cuda.synchronize()
            ms = ev[0].elapsed_time(ev[1])
            walls.setdefault((label, iters), []).append(ms)
            print(json.dumps({"kernel": f"{iters} {label} RL iterations, {route}", "path": plan.path, "grid": oshape,
                              "iterations": iters, "ms": ms, "ms_per_iteration": ms / iters}), flush=True)
        plain = min(walls[("plain", 20)])
        print(json.dumps({"kernel": f"accelerated against 20 plain iterations, {route}", "path": plan.path, "grid": oshape,
                          "ms_20_plain": plain,
                          **{f"ratio_{k}_accelerated": walls[("accelerated", k)][0] / plain for k in (9, 10, 15)}}), flush=True)
        plan.release()
        del plan
        torch.cuda.empty_cache()


def _rl_fft(args, torch, dev, g, oshape):
    """ms per RL iteration with both convolutions in the Fourier domain (shrimpy_amd/deconvolve_fft.py), over dense PSF
    extents from the stencil kernels' range to a measured bead patch; the stencil route beside it where one exists."""
    from shrimpy_amd.deconvolve import make_plan

    y = torch.poisson(torch.full(oshape, 100.0, device=dev), generator=g)
    rng = np.random.default_rng(4)
    for size in [(9, 7, 7), (11, 9, 9), (13, 13, 13), (15, 15, 15), (15, 19, 19), (21, 15, 15), (31, 37, 19)]:
        zz, yy, xx = np.meshgrid(*[np.arange(n) - n // 2 for n in size], indexing="ij")
        zr, xr = 0.9 * zz + 0.43 * xx, -0.43 * zz + 0.9 * xx
        w = np.exp(-0.5 * ((zr / (size[0] / 5)) ** 2 + (yy / (size[1] / 5)) ** 2 + (xr / (size[2] / 5)) ** 2))
        w = (w * (1 + 0.02 * rng.standard_normal(size))).clip(0).astype(np.float32)
        w /= w.sum()
        for method in ("fft", "direct"):
            if method == "direct" and (max(size) > 15 or size[0] * size[1] * size[2] > 2200):
                continue      # (refused by the stencil plan / minutes per iteration through the generic stencil)
            plan = make_plan(oshape, w, dev, separable="never", method=method)
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            plan(y, iterations=1)
            torch.cuda.synchronize()
            iters = 3 if plan.path != "generic" else 1
            plan(y, iterations=iters, events=ev)
            torch.cuda.synchronize()
            ms = ev[0].elapsed_time(ev[1]) / iters
            row = {"kernel": "RL iteration, dense PSF", "psf": list(size), "method": method, "path": plan.path, "grid": oshape,
                   "ms_per_iteration": ms}
            if plan.path == "fft":
                row["fft_grid"] = list(plan.grid)
            plan.release()
            del plan
            torch.cuda.empty_cache()
            print(json.dumps(row), flush=True)


def _phase(args, torch, dev, g, oshape):
    """One application of the phase reconstruction (shrimpy_amd/phase.py) on a deskewed volume of ``oshape`` with the optics
    of the reference's dynatrack_demo.yaml: ms per launch and in total (HIP events), the warm-up seconds; beside it one
    convolution of the Fourier-domain Richardson-Lucy (forward rows, y, z leg, y back, ratio epilogue) on the same volume
    with a measured-PSF-sized kernel -- the yardstick: the same legs on a grid without the mirror padding."""
    import logging

    from shrimpy_amd import _lib, fft3
    from shrimpy_amd.deconvolve_fft import FftRichardsonLucyPlan
    from shrimpy_amd.phase import PhasePlan

    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(message)s")
    settings = dict(transfer_function=dict(wavelength_illumination=0.450, z_padding=5, index_of_refraction_media=1.4,
                                           numerical_aperture_detection=1.35, numerical_aperture_illumination=0.52,
                                           invert_phase_contrast=False, yx_pixel_size=0.1133, z_pixel_size=0.17),
                    apply_inverse=dict(reconstruction_algorithm="Tikhonov", regularization_strength=0.01))
    y = torch.poisson(torch.full(oshape, 300.0, device=dev), generator=g)
    out = torch.empty_like(y)

    # the yardstick first (its scratch is released before the phase plan's is made)
    psf = np.random.default_rng(4).random((15, 19, 19)).astype(np.float32)
    rl = FftRichardsonLucyPlan(oshape, psf / psf.sum(), dev)
    rl._scratch()

    def rl_convolution():
        rl._forward(y)
        rl._middle(0)
        rl._epilogue("lsr_irfft_rows_rl_f32", _lib.EPI_RATIO, y, out, 1e-6, None)

    rl_ms = timed(rl_convolution, args.reps)
    rl_grid = list(rl.grid)
    rl.release()
    del rl
    torch.cuda.empty_cache()

    plan = PhasePlan(oshape, settings, dev)
    plan(y, out=out)
    gz, gy, gx = plan.grid
    z, yy, x = oshape
    xc, stream = plan._xc, _lib.stream_ptr(dev)
    b = plan._b
    launches = {
        "rows forward": lambda: _lib.call("lsr_phase_rows_forward_c64", y.data_ptr(), z, yy, x, b.data_ptr(), gz, gy, gx,
                                          plan._half.data_ptr(), plan._full.data_ptr(), plan._partial.data_ptr(),
                                          plan._mean.data_ptr(), stream),
        "y forward (hipFFT)": lambda: fft3._exec(dev, fft3._HIPFFT_C2C, gy, gz * xc, b.data_ptr(), b.data_ptr(), fft3._FORWARD),
        "z leg x filter": lambda: _lib.call("lsr_spectrum_multiply_z_c64", plan._filter.data_ptr(), b.data_ptr(),
                                            plan._tw_z.data_ptr(), gz, gy, xc, 0, gz, z, stream),
        "y back (hipFFT)": lambda: fft3._exec(dev, fft3._HIPFFT_C2C, gy, z * xc, b.data_ptr(), b.data_ptr(), fft3._BACKWARD),
        "rows inverse": lambda: _lib.call("lsr_phase_rows_inverse_f32", b.data_ptr(), gz, gy, gx, plan._half.data_ptr(),
                                          plan._full.data_ptr(), plan._mean.data_ptr(), out.data_ptr(), z, yy, x, stream),
    }
    # (each launch alone, on whatever the spectrum buffer holds: the kernels' time does not depend on the values)
    per_launch = {name: timed(fn, args.reps) for name, fn in launches.items()}
    total = timed(lambda: plan(y, out=out), args.reps)       # the whole call, its one wait for the mean included
    row = {"kernel": "phase reconstruction, one application", "shape": list(oshape), "grid": list(plan.grid),
           "ms_per_launch": per_launch, "ms_launches_sum": sum(per_launch.values()), "ms_total": total,
           "warm_up_seconds": plan.seconds, "rl_fft_convolution_ms": rl_ms, "rl_fft_grid": rl_grid,
           "ratio_to_rl_convolution": total / rl_ms, "device": torch.cuda.get_device_name(dev),
           "kernel_sources": _lib.kernel_source_sha16()}
    print(json.dumps(row), flush=True)
    if list(oshape) == [171, 2048, 2270]:
        with open(ROOT / "profiles" / "phase_config2.jsonl", "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
