"""CPU-side checks of rows.pack_host, the one packer of host results into the slot layout that match_batch, track.update_batch,
gallery.update_batch and draw_batch upload: the two images byte for byte against arrays written out by hand, at offsets in a larger
buffer, with every image empty, and the four refusals."""
import numpy as np
import pytest
import torch

from densebox_amd import rows as R

ROW13 = [[1, 2, 3, 4, 0.5, 10, 11, 12, 13, 14, 15, 16, 17], [5, 6, 7, 8, 0.25, 20, 21, 22, 23, 24, 25, 26, 27],
         [9, 10, 11, 12, 0.125, 30, 31, 32, 33, 34, 35, 36, 37]]
KEEPS = [[1], [], [0, 0]]                                   # image 2's list is longer than its rows: slots = 2
WANT_KEEP = np.array([[1, 1, 0], [0, 0, 0], [2, 0, 0]], np.int32)


def _inputs(dc):
    r = np.array(ROW13, np.float64)[:, :dc]
    return [r[:2], np.zeros((0, dc)), r[2:]]


def _want_dets(dc):
    z = [0.0] * 13
    return np.array([[ROW13[0], ROW13[1]], [z, z], [ROW13[2], z]], np.float64)[:, :, :dc].copy()


@pytest.mark.parametrize('dc', [5, 13])
def test_images_byte_for_byte(dc):
    p = R.pack_host('f', _inputs(dc), KEEPS)
    assert (p.dc, p.B, p.slots, p.nd, p.nk) == (dc, 3, 2, 3 * 2 * dc * 8, 3 * 3 * 4)
    assert [k.tolist() for k in p.lists] == KEEPS and all(k.dtype == np.int64 for k in p.lists)
    host = np.full(p.nd + p.nk, 0xAA, np.uint8)            # write() defines every byte of its two regions
    p.write(host, 0, p.nd)
    assert host[:p.nd].tobytes() == _want_dets(dc).tobytes()
    assert host[p.nd:].tobytes() == WANT_KEEP.tobytes()


def test_write_at_offsets_leaves_the_rest_untouched():
    p = R.pack_host('f', _inputs(5), KEEPS)
    o_dets, o_keep = 16, 16 + p.nd + 8 + 4
    host = np.full(o_keep + p.nk + 12, 0xAA, np.uint8)
    p.write(host, o_dets, o_keep)
    want = np.full(host.size, 0xAA, np.uint8)
    want[o_dets:o_dets + p.nd] = np.frombuffer(_want_dets(5).tobytes(), np.uint8)
    want[o_keep:o_keep + p.nk] = np.frombuffer(WANT_KEEP.tobytes(), np.uint8)
    assert host.tobytes() == want.tobytes()


def test_every_image_empty_gives_one_slot():
    p = R.pack_host('f', [np.zeros((0, 5)), torch.zeros(0, 5)], [[], torch.zeros(0, dtype=torch.int64)])
    assert (p.dc, p.B, p.slots) == (5, 2, 1)               # the smallest slots the entry points accept
    host = np.full(p.nd + p.nk, 0xAA, np.uint8)
    p.write(host, 0, p.nd)
    assert host.tobytes() == np.zeros((2, 1, 5), np.float64).tobytes() + np.zeros((2, 2), np.int32).tobytes()


def test_tensor_rows_and_lists_pack_as_arrays_do():
    d = _inputs(13)
    a = R.pack_host('f', d, KEEPS)
    b = R.pack_host('f', tuple(torch.from_numpy(x.copy()) for x in d), [torch.tensor(k, dtype=torch.int32) for k in KEEPS], n=3)
    ha, hb = (np.zeros(p.nd + p.nk, np.uint8) for p in (a, b))
    a.write(ha, 0, a.nd)
    b.write(hb, 0, b.nd)
    assert b[2:] == a[2:] and ha.tobytes() == hb.tobytes()


def test_refusals():
    d5, d13 = np.zeros((2, 5)), np.zeros((2, 13))
    for dets, keeps in (([d5], [[0], [1]]), ([], []), (d5, [[0]]), ([d5], None)):
        with pytest.raises(RuntimeError, match='^who: dets and keeps must be non-empty lists with one entry per image$'):
            R.pack_host('who', dets, keeps)
    for dets, keeps in (([d5], [[0], [1]]), ([d5], [[0]])):
        with pytest.raises(RuntimeError, match=r'^who: dets and keeps must be lists with one entry per image \(2 images\)$'):
            R.pack_host('who', dets, keeps, n=2)
    for dets in ([d5, d13], [np.zeros((2, 6))], [np.zeros(5)]):
        with pytest.raises(RuntimeError, match=r'^who: every dets entry must be \[n, 5\] or \[n, 13\], all alike; got \[\['):
            R.pack_host('who', dets, [[0]] * len(dets))
    with pytest.raises(RuntimeError, match=r'^who: every dets entry must be \[n, 13\] \(rows with landmarks\); got \[\[2, 5\]\]$'):
        R.pack_host('who', [d5], [[0]], cols=(13,))
    for bad in ([2], [-1], [0, 5]):
        with pytest.raises(RuntimeError, match=r'^who: keeps\[1\] names a row outside 0\.\.1$'):
            R.pack_host('who', [d5, d5], [[0], bad])
    with pytest.raises(RuntimeError, match='^who: 9 rows in one image exceed 8$'):
        R.pack_host('who', [np.zeros((9, 5))], [[0]], max_slots=8)
    with pytest.raises(RuntimeError, match='^who: 9 rows in one image exceed 8$'):                  # a list longer than the rows counts too
        R.pack_host('who', [d5], [[0] * 9], max_slots=8)
    assert R.pack_host('who', [np.zeros((8, 5))], [[0]], max_slots=8).slots == 8
