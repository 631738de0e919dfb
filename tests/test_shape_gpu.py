"""``shape_table`` and ``contact_table`` on the device: every integer equals the CPU's exactly, on the two-ball scene (split,
measured through ``segment_zyx``) and on (5, 9, 130) random labels; the float columns derive from those integers on the host."""

import numpy as np
import pytest

from shrimpy_amd import segment as S
from tests import test_shape_host as H

pytestmark = pytest.mark.gpu

INTEGERS = S.MOMENT_FIELDS + ("faces_zyx", "contact_faces_zyx", "n_neighbours", "touches_border")


def same_integers(on_device, on_host):
    for k in INTEGERS:
        assert on_device[k].dtype == on_host[k].dtype and np.array_equal(on_device[k], on_host[k]), k


def same_contacts(on_device, on_host):
    assert H.contacts_as_dict(on_device) == H.contacts_as_dict(on_host)
    assert np.array_equal(on_device["area"], on_host["area"])


def test_two_balls_on_the_device(device):
    labels, table, contacts = H.check_two_balls(device)
    host_labels, host_table, host_contacts = H.check_two_balls("cpu")
    assert labels.device.type == "cuda" and np.array_equal(labels.cpu().numpy(), host_labels.numpy())
    same_integers(table, host_table)
    same_contacts(contacts, host_contacts)
    assert np.array_equal(table["axis_lengths"], host_table["axis_lengths"])      # (host code on equal integers)


def test_random_labels_on_the_device(device):
    labels = H.random_labels((5, 9, 130))
    table = H.check_faces_and_contacts(labels, 5, device, sampling=(2.0, 1.0, 0.5))
    same_integers(table, S.shape_table(H.tensor(labels), 5, (2.0, 1.0, 0.5)))
    same_contacts(S.contact_table(H.tensor(labels, device), (2.0, 1.0, 0.5)), S.contact_table(H.tensor(labels), (2.0, 1.0, 0.5)))
