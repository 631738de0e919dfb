"""The restatement of the tracking rules (``shrimpy_amd/track.py`` states them): the overlap table by ``np.unique`` of the
packed key over the shifted, masked volumes, the linking and the track rules in plain Python loops.  Written independently of
the product; the product's tests compare against this, exactly."""

import numpy as np


def overlap_table(a, b, shift=(0, 0, 0)) -> set:
    """``{(a, b, count)}``: the voxels ``v`` with ``a[v] > 0`` whose partner ``v + shift`` lies in the volume with ``b > 0``."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.ndim == 3
    sel_a, sel_b = [], []
    for n, s in zip(a.shape, shift):
        s = int(s)
        if abs(s) >= n:
            return set()
        sel_a.append(slice(max(0, -s), min(n, n - s)))
        sel_b.append(slice(max(0, s), min(n, n + s)))
    va, vb = a[tuple(sel_a)].astype(np.int64).ravel(), b[tuple(sel_b)].astype(np.int64).ravel()
    fg = (va > 0) & (vb > 0)
    keys, counts = np.unique((va[fg].astype(np.uint64) << np.uint64(32)) | vb[fg].astype(np.uint64), return_counts=True)
    return {(int(k >> np.uint64(32)), int(k & np.uint64(0xFFFFFFFF)), int(c)) for k, c in zip(keys, counts)}


def volumes(labels) -> dict:
    """``{label: voxels}`` of the positive labels."""
    values, counts = np.unique(np.asarray(labels), return_counts=True)
    return {int(v): int(c) for v, c in zip(values, counts) if v > 0}


def link(table: set, va: dict, vb: dict, min_overlap_voxels=1, min_iou=0.0) -> dict:
    """``{b: (parent, overlap, iou)}`` for every object of the later frame."""
    out = {}
    for b in sorted(vb):
        best = None
        for a_, b_, c in sorted(table):                 # ascending a: of equal counts the smaller a stays
            if b_ != b or c < min_overlap_voxels:
                continue
            if float(c) < float(min_iou) * float(va[a_] + vb[b] - c):
                continue
            if best is None or c > best[1]:
                best = (a_, c)
        out[b] = (best[0], best[1], float(best[1]) / float(va[best[0]] + vb[b] - best[1])) if best else (0, 0, 0.0)
    return out


def tracks(frames, min_overlap_voxels=1, min_iou=0.0, divisions=True, shifts=None):
    """``(track_of, tracks, objects)``: per frame ``{label: track}``; ``[(track_id, t_begin, t_end, parent_track_id)]``;
    ``[(t, label, track_id, parent_label, overlap_voxels, iou)]``."""
    track_of, begin, end, parent_track, objects = [], {}, {}, {}, []
    prev, prev_vol = None, None
    for t, frame in enumerate(frames):
        vol = volumes(frame)
        if prev is None:
            links = {b: (0, 0, 0.0) for b in vol}
        else:
            shift = (0, 0, 0) if shifts is None else shifts[t - 1]
            links = link(overlap_table(prev, frame, shift), prev_vol, vol, min_overlap_voxels, min_iou)
        kids = {}
        for b in sorted(links):
            if links[b][0]:
                kids.setdefault(links[b][0], []).append(b)
        now = {}
        for b in sorted(vol):
            a, c, iou = links[b]
            carries = False
            if a:
                if divisions:
                    carries = len(kids[a]) == 1
                else:
                    carries = sorted(kids[a], key=lambda k: (-links[k][1], k))[0] == b
            if carries:
                k = track_of[-1][a]
                end[k] = t
            else:
                k = len(begin) + 1
                begin[k] = end[k] = t
                parent_track[k] = track_of[-1][a] if (a and divisions) else 0
            now[b] = k
            objects.append((t, b, k, a, c, iou))
        track_of.append(now)
        prev, prev_vol = frame, vol
    return track_of, [(k, begin[k], end[k], parent_track[k]) for k in sorted(begin)], objects


def track_volume(labels, track_of: dict):
    """Every voxel's track id."""
    labels = np.asarray(labels)
    out = np.zeros(labels.shape, dtype=np.int32)
    for label, k in track_of.items():
        out[labels == label] = k
    return out
