"""The copy the painters share (csrc/frame_tile.hpp, tile_copy) on each of its word sizes, through both entry points.  Every arena of
viz.draw_batch / redact.redact_batch is 64-aligned, so src and dst there always allow the same 16-byte words; here dst sits at byte
offsets 0, 4 and 1 from src's alignment, which selects the 16-byte, the dword and the byte path.  One frame of 3 x 150 pixels with 3
channels and an empty keep list: every tile takes the copy-through, rows of 450 bytes give ragged heads and tails, and 150 columns
give two overlay tiles and three redaction tiles, the last of each partial."""
import ctypes as C

import numpy as np
import pytest
import torch

from densebox_amd import _lib, redact, viz
from densebox_amd._lib import check, ptr, stream_ptr

pytestmark = pytest.mark.gpu

GUARD = 64                     # sentinel bytes in front of and behind dst
FILL_B = 0xEE
H, W, CH = 3, 150, 3


def _overlay(table, dets, keep):
    rec = viz.Style().record()
    check(_lib.lib().dbx_draw_overlay_batch(ptr(table), 1, CH, H, W, ptr(dets), 5, 1, ptr(keep), None, 1, None, None, None, 0, 0,
                                            C.byref(rec), stream_ptr()))


def _redact(table, dets, keep):
    rec = redact.Redaction().record(5, 0)
    check(_lib.lib().dbx_redact_batch(ptr(table), 1, CH, H, W, ptr(dets), 5, 1, ptr(keep), None, 1, None, 0, 0, 0, C.byref(rec), stream_ptr()))


@pytest.mark.parametrize('off', [0, 4, 1], ids=['words16', 'dwords', 'bytes'])
@pytest.mark.parametrize('launch', [_overlay, _redact], ids=['overlay', 'redact'])
def test_copy_through_on_every_word_size(launch, off):
    img = np.random.default_rng(7).integers(0, 256, (H, W, CH), dtype=np.uint8)
    n = img.size
    src = torch.from_numpy(img.reshape(-1)).cuda()
    whole = torch.full((GUARD + off + n + GUARD,), FILL_B, dtype=torch.uint8, device='cuda')
    assert src.data_ptr() % 64 == 0 and whole.data_ptr() % 64 == 0
    rec = (_lib.OverlayFrame * 1)()
    rec[0].src, rec[0].dst, rec[0].h, rec[0].w = src.data_ptr(), whole.data_ptr() + GUARD + off, H, W
    table = torch.frombuffer(rec, dtype=torch.uint8).cuda()
    dets = torch.zeros((1, 5), dtype=torch.float64, device='cuda')
    keep = torch.zeros((1, 2), dtype=torch.int32, device='cuda')          # the count 0: nothing is painted
    launch(table, dets, keep)
    torch.cuda.synchronize()
    got = whole.cpu().numpy()
    assert (got[:GUARD + off] == FILL_B).all() and (got[GUARD + off + n:] == FILL_B).all(), 'bytes outside dst were written'
    assert np.array_equal(got[GUARD + off:GUARD + off + n], img.reshape(-1))
    assert np.array_equal(src.cpu().numpy(), img.reshape(-1))             # the source is read only
