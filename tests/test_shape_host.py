"""Object shape and contacts on CPU tensors (``segment.shape_table``, ``segment.contact_table``, ``SegmentSettings.shape`` and
``contacts``): eigenvalues against the float64 restatement from raw coordinates, faces and contacts against the brute force
(``tests/moments_ref.py``), and figures worked out for boxes, digitised ellipsoids and two touching balls.  PARITY UNPINNED."""

import numpy as np
import torch

from shrimpy_amd import segment as S
from shrimpy_amd.settings import SegmentSettings
from tests import moments_cases as C
from tests import moments_ref as R
from tests import track_cases as TC

RANDOM_SHAPES = [(1, 1, 1), (1, 1, 2), (4, 5, 6), (5, 9, 130)]
SPLIT_SETTINGS = dict(channel_name="GFP", threshold=0.5, split=True, split_min_depth=1.0)


def tensor(a, device="cpu"):
    return torch.from_numpy(np.array(a, dtype=np.int32, order="C")).to(device)


def random_labels(shape):
    return np.random.default_rng(int(np.prod(shape))).integers(0, 6, shape).astype(np.int32)


def is_axis(got, want) -> bool:
    return bool(np.all(np.abs(got - np.asarray(want, dtype=np.float64)) <= 1e-12))


def contacts_as_dict(table) -> dict:
    assert table["a"].dtype == table["b"].dtype == table["faces_zyx"].dtype == np.int64 and table["area"].dtype == np.float64
    assert np.all(table["a"] < table["b"])
    order = np.lexsort((table["b"], table["a"]))
    assert np.array_equal(order, np.arange(len(order))), "sorted by (a, b)"
    return {(int(a), int(b)): [int(v) for v in f] for a, b, f in zip(table["a"], table["b"], table["faces_zyx"])}


def check_faces_and_contacts(labels, n, device="cpu", sampling=(1, 1, 1)):
    """``shape_table`` and ``contact_table`` against the brute force; returns the shape table."""
    faces, contacts = R.faces_and_contacts(labels, n)
    table = S.shape_table(tensor(labels, device), n, sampling)
    assert table["faces_zyx"].dtype == np.int64 and np.array_equal(table["faces_zyx"], faces)
    got = S.contact_table(tensor(labels, device), sampling)
    assert contacts_as_dict(got) == contacts
    per_label = np.zeros((n, 3), dtype=np.int64)
    neighbours = np.zeros((n,), dtype=np.int64)
    for (a, b), f in contacts.items():
        per_label[a - 1] += f
        per_label[b - 1] += f
        neighbours[a - 1] += 1
        neighbours[b - 1] += 1
    assert np.array_equal(table["contact_faces_zyx"], per_label) and np.array_equal(table["n_neighbours"], neighbours)
    sz, sy, sx = sampling
    areas = np.asarray([sy * sx, sz * sx, sz * sy], dtype=np.float64)
    assert np.array_equal(table["surface_area"], faces.astype(np.float64) @ areas)
    assert np.array_equal(table["contact_area"], per_label.astype(np.float64) @ areas)
    assert np.array_equal(got["area"], got["faces_zyx"].astype(np.float64) @ areas)
    return table


def test_eigenvalues_equal_the_float64_restatement():
    """Within ``1e-12 * l0``: eigh's backward error is a few tens of ``2^-53 |C|``."""
    for shape, sampling in [((4, 5, 6), (1, 1, 1)), ((5, 9, 130), (2.0, 0.5, 0.25))]:
        labels = random_labels(shape)
        table = S.shape_table(tensor(labels), 5, sampling)
        for k in range(1, 6):
            want = R.eigenvalues(labels, k, sampling)
            assert np.all(np.abs(table["eigenvalues"][k - 1] - want) <= 1e-12 * want[0]), (shape, k)
            assert np.array_equal(table["axis_lengths"][k - 1], 2.0 * np.sqrt(5.0 * table["eigenvalues"][k - 1]))
        assert np.allclose(np.linalg.norm(table["major_axis"], axis=1), 1.0, atol=1e-12)


def test_faces_and_contacts_equal_the_brute_force():
    for shape in RANDOM_SHAPES:
        table = check_faces_and_contacts(random_labels(shape), 5, sampling=(2.0, 1.0, 0.5))
        assert table["touches_border"].dtype == np.bool_


def test_a_solid_box():
    labels = TC.boxes((7, 9, 11), (1, 2, 5, 2, 7, 2, 9))          # 3 x 5 x 7, off every border
    table = check_faces_and_contacts(labels, 1)
    assert np.allclose(table["axis_lengths"][0], np.asarray([7.0, 5.0, 3.0]) * np.sqrt(5.0 / 3.0), rtol=1e-12, atol=0)
    assert table["faces_zyx"][0].tolist() == [70, 42, 30] and table["surface_area"][0] == 142.0
    assert is_axis(table["major_axis"][0], (0, 0, 1))
    assert table["n_neighbours"][0] == 0 and table["contact_area"][0] == 0.0 and not table["touches_border"][0]
    assert S.shape_table(tensor(TC.boxes((7, 9, 11), (1, 0, 3, 2, 7, 2, 9))), 1)["touches_border"][0]
    assert S.shape_table(tensor(TC.boxes((7, 9, 11), (1, 2, 5, 2, 7, 4, 11))), 1)["touches_border"][0]


def test_a_single_voxel_is_not_degenerate_and_an_absent_label_is_nan():
    labels = np.zeros((3, 3, 3), dtype=np.int32)
    labels[1, 1, 1] = 1
    table = S.shape_table(tensor(labels), 2, (2.0, 1.0, 1.0))
    assert np.allclose(table["axis_lengths"][0], 2.0 * np.sqrt(5.0 / 12.0) * np.asarray([2.0, 1.0, 1.0]), rtol=1e-12)
    assert table["faces_zyx"][0].tolist() == [2, 2, 2] and is_axis(table["major_axis"][0], (1, 0, 0))
    assert table["volume"][1] == 0 and np.isnan(table["axis_lengths"][1]).all() and not table["touches_border"][1]
    assert table["faces_zyx"][1].tolist() == [0, 0, 0]


def test_digitised_ellipsoids():
    table = S.shape_table(tensor(C.ellipsoid((15, 21, 31), (5, 8, 13))), 1)
    assert np.all(np.abs(table["axis_lengths"][0] / np.asarray([26.0, 16.0, 10.0]) - 1.0) <= 0.005)     # 25.948, 16.058, 9.959
    assert is_axis(table["major_axis"][0], (0, 0, 1))
    turned = S.shape_table(tensor(C.ellipsoid((13, 41, 41), (4, 7, 13), 45.0)), 1)
    assert np.all(np.abs(turned["axis_lengths"][0] / np.asarray([26.0, 14.0, 8.0]) - 1.0) <= 0.02)       # 26.14, 14.14, 7.85
    assert np.all(np.abs(turned["major_axis"][0] - np.asarray([0.0, np.sqrt(0.5), np.sqrt(0.5)])) <= 1e-6)


def test_a_ball_under_anisotropic_sampling():
    ball = C.ellipsoid((9, 15, 15), (3, 6, 6))                    # radius 6 under sampling (2, 1, 1)
    lengths = S.shape_table(tensor(ball), 1, (2.0, 1.0, 1.0))["axis_lengths"][0]                       # 12.28, 12.28, 11.93
    assert lengths.max() / lengths.min() - 1.0 <= 0.03 and abs(lengths.mean() / 12.0 - 1.0) <= 0.03


def test_two_boxes_that_share_a_face():
    labels = TC.boxes((6, 8, 12), (1, 1, 4, 1, 6, 1, 5), (2, 2, 5, 2, 7, 5, 9))      # they meet across x = 4 | 5
    got = S.contact_table(tensor(labels), (2.0, 1.0, 0.5))
    shared = 2 * 4                                                # z 2..3, y 2..5
    assert contacts_as_dict(got) == {(1, 2): [0, 0, shared]} and got["area"].tolist() == [shared * 2.0 * 1.0]
    table = check_faces_and_contacts(labels, 2, sampling=(2.0, 1.0, 0.5))
    assert table["n_neighbours"].tolist() == [1, 1] and table["contact_faces_zyx"].tolist() == [[0, 0, shared]] * 2


def check_two_balls(device="cpu"):
    """Shared with tests/test_shape_gpu.py: returns ``(labels, table, contact_table)``."""
    vol = torch.from_numpy(C.two_balls()).to(device)
    labels, table, n = S.segment_zyx(vol, SegmentSettings(**SPLIT_SETTINGS, shape=True, contacts=True))
    assert n == 2
    host = labels.cpu().numpy()
    faces, contacts = R.faces_and_contacts(host, 2)
    got = S.contact_table(labels)
    assert list(contacts) == [(1, 2)] and contacts_as_dict(got) == contacts
    assert np.array_equal(table["faces_zyx"], faces) and table["n_neighbours"].tolist() == [1, 1]
    assert np.array_equal(table["contact_faces_zyx"], np.asarray([contacts[1, 2]] * 2))
    assert np.array_equal(table["volume"], np.bincount(host.ravel(), minlength=3)[1:])
    _, unsplit, n1 = S.segment_zyx(vol, SegmentSettings(channel_name="GFP", threshold=0.5, shape=True))
    assert n1 == 1 and unsplit["n_neighbours"].tolist() == [0] and is_axis(unsplit["major_axis"][0], (0, 0, 1))
    return labels, table, got


def test_two_balls_split_shape_and_contacts():
    check_two_balls()


def test_the_settings_default_to_off_and_the_table_keeps_its_keys():
    s = SegmentSettings(channel_name="GFP", threshold=0.5)
    assert s.shape is False and s.contacts is False
    assert "contacts.csv" in SegmentSettings.__doc__
    vol = torch.from_numpy(C.two_balls())
    today = ["label", "volume", "bbox", "sum_zyx", "centroid", "intensity_sum", "intensity_mean", "intensity_min", "intensity_max",
             "intensity_sum_zyx", "weighted_centroid"]
    _, table, _ = S.segment_zyx(vol, s)
    assert list(table) == today
    _, table, _ = S.segment_zyx(vol, SegmentSettings(channel_name="GFP", threshold=0.5, contacts=True))
    assert list(table) == today, "contacts is the command's: the table does not change"
    _, table, _ = S.segment_zyx(vol, SegmentSettings(channel_name="GFP", threshold=0.5, shape=True, inscribed_radius=True))
    assert list(table) == today + ["inscribed_radius"] + list(S.SHAPE_COLUMNS)
