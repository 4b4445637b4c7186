"""CPU-side check of the packed layout of dbx_detect_thresh_batch as the Python tail reads it: decode._thresh_fetch_bytes,
decode._unpack_thresh and the threshold branch of track._unpack on hand-made counts and arenas (tests/test_pyramid_thresh_abi.py does the
same for the merge's counts)."""
import numpy as np
import pytest
import torch

from densebox_amd import decode as DC, track as TR


def _counts_words(pairs):
    """int32 [3 B + 1]: the (n_b, pixels above the threshold) pairs, then the [B + 1] prefix of the n_b"""
    n = [p[0] for p in pairs]
    return np.concatenate([np.asarray(pairs, np.int64).reshape(-1), [0], np.cumsum(n)]).astype(np.int32)


@pytest.mark.parametrize('dc', [5, 13])
@pytest.mark.parametrize('pairs', [[(3, 9), (0, 0), (2, 5000)],          # an empty image between two others, the last one cut by the cap
                                   [(0, 0), (0, 0), (0, 0)],             # a call without a row
                                   [(4, 4), (1, 70000), (6, 7)]])
def test_fetch_bytes_and_unpack_on_hand_made_counts(dc, pairs):
    B = len(pairs)
    c = _counts_words(pairs)
    assert c.shape[0] == 3 * B + 1
    n = [p[0] for p in pairs]
    total = sum(n)
    nbytes = DC._thresh_fetch_bytes(c, dc)
    assert nbytes == total * dc * 8 + (total + B) * 4
    # an arena as the kernel packs it: row r of the call holds r in every column; the list of image b keeps its last and its first row
    rows = np.repeat(np.arange(total, dtype=np.float64)[:, None], dc, axis=1)
    lists, want, at = np.zeros(total + B, np.int32), [], 0
    for nb in n:
        keep = [nb - 1, 0][:min(nb, 2)]
        lists[at], lists[at + 1:at + 1 + len(keep)] = len(keep), keep
        want.append(keep)
        at += nb + 1
    arena = np.concatenate([rows.view(np.uint8).reshape(-1), lists.view(np.uint8)])
    assert arena.shape[0] == nbytes
    got = DC._unpack_thresh(c, arena, dc, True)
    assert len(got) == B
    first = 0
    for (d, keep, pixels), (nb, px), w in zip(got, pairs, want):
        assert d.shape == (nb, dc) and d.dtype == np.float64 and d.flags['OWNDATA']
        assert (d == np.arange(first, first + nb, dtype=np.float64)[:, None]).all()
        assert keep == w and all(type(v) is int for v in keep)
        assert pixels == px and type(pixels) is int
        first += nb
    plain = DC._unpack_thresh(c, arena, dc, False)
    assert all(len(r) == 2 for r in plain)
    for (d, keep), (d2, keep2, _) in zip(plain, got):
        assert d.tobytes() == d2.tobytes() and d.shape == d2.shape and keep == keep2
    # the tracker's chunks carry the same rows and lists in tensors of their own, of the capacity of the call
    cap = max(n) + 3
    dets = torch.full((B * cap, dc), -1.0, dtype=torch.float64)
    dets[:total] = torch.from_numpy(rows)
    keep_t = torch.full((B * (cap + 1),), -7, dtype=torch.int32)
    keep_t[:total + B] = torch.from_numpy(lists)
    ids = torch.arange(2 * B * cap, dtype=torch.int32).reshape(2, B, cap)
    tracked = TR._unpack('thresh', (dets, keep_t, torch.from_numpy(c), ids), dc)
    assert len(tracked) == B
    for b, ((d, keep, tid, hits), (d2, keep2)) in enumerate(zip(tracked, plain)):
        assert d.tobytes() == d2.tobytes() and d.shape == d2.shape and d.dtype == np.float64 and keep == keep2
        assert tid.tolist() == ids[0, b, :len(keep)].tolist() and hits.tolist() == ids[1, b, :len(keep)].tolist()
