"""Guarded framed buffers for the whole-buffer kernel tests (tests/test_hip_head2_paths.py, tests/test_hip_aux_paths.py): a framed NHWC
map between two guard bands, its expected content kept on the host, and the comparison of EVERY element of the device copy with it."""
import ctypes as C

import numpy as np
import torch

from densebox_amd._lib import View


class Buf:
    """A framed NHWC buffer (or, with h = w = 1 and pad 0, a plain array of n rows) between two guard bands: `exp` is what it must hold,
    `dev` the device copy, made by upload().  `fill` is the value of the halo and of the guard bands; `interior` [n][h][w][ld] (or
    anything that broadcasts to it) the value of the pixels."""

    def __init__(self, name, n, h, w, pad, ld, tdt, fill, interior=None):
        self.name, self.shape, self.pad, self.ld, self.tdt = name, (n, h, w), pad, ld, tdt
        hp, wp = h + 2 * pad, w + 2 * pad
        self.guard = -(-max(2 * wp * ld, 64) // 64) * 64
        a = np.full(2 * self.guard + n * hp * wp * ld, fill, dtype=np.float64)
        self.body = a[self.guard:self.guard + n * hp * wp * ld].reshape(n, hp, wp, ld)
        if interior is not None:
            self.body[:, pad:pad + h, pad:pad + w] = interior
        self.np = a
        self.dev = None

    def tensor(self, a=None):
        return torch.from_numpy(self.np if a is None else a).to(self.tdt)           # (every value is representable: the cast is exact)

    def host_with_interior(self, interior, c_off=0):
        """The expected content as float64 with channels [c_off, c_off + interior.shape[-1]) of the pixels replaced."""
        n, h, w = self.shape
        a = self.np.copy()
        body = a[self.guard:self.guard + self.body.size].reshape(self.body.shape)
        body[:, self.pad:self.pad + h, self.pad:self.pad + w, c_off:c_off + np.shape(interior)[-1]] = interior
        return a

    def with_interior(self, interior, c_off=0):
        return self.tensor(self.host_with_interior(interior, c_off))

    def upload(self):
        self.dev = self.tensor().cuda()
        return self

    def ptr(self):
        return self.dev.data_ptr() + self.guard * self.dev.element_size()

    def view(self, c=None, null=False, c_off=0):
        n, h, w = self.shape
        return View(None if null else C.c_void_p(self.ptr()), n, h, w, self.pad, self.ld, c_off, c or self.ld)

    def where(self, i):
        """Flat index -> a readable place."""
        if i < self.guard or i >= self.guard + self.body.size:
            return 'guard band (flat index %d, body at [%d, %d))' % (i, self.guard, self.guard + self.body.size)
        n, hp, wp, ld = self.body.shape
        j = i - self.guard
        img, y, x, c = j // (hp * wp * ld), j // (wp * ld) % hp - self.pad, j // ld % wp - self.pad, j % ld
        halo = not (0 <= y < self.shape[1] and 0 <= x < self.shape[2])
        return '%simage %d row %d column %d channel %d (head %d, channel %d)' % ('HALO ' if halo else '', img, y, x, c, c // 512, c % 512)


def assert_holds(buf, want=None, lo=None, hi=None, what=''):
    """The device buffer equals `want` (default: what it was created with) everywhere, or lies in [lo, hi] everywhere (float64 bounds
    are compared in float64: a bound need not be a value of the buffer's type)."""
    got = buf.dev.cpu()
    if lo is None:
        want = buf.tensor() if want is None else want
        bad = got != want
    else:
        if lo.dtype == torch.float64:
            got = got.double()
        bad = ~((got >= lo) & (got <= hi))
        want = lo
    if bool(bad.any()):
        idx = torch.nonzero(bad.flatten())[:, 0]
        i = int(idx[0])
        raise AssertionError('%s %s: %d of %d elements differ, the first at %s: got %r, want %r%s' % (
            what, buf.name, idx.numel(), got.numel(), buf.where(i), float(got.flatten()[i]), float(want.flatten()[i]),
            '' if hi is None else ' .. %r' % float(hi.flatten()[i])))
