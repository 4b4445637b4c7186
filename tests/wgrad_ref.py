"""Float64 CPU reference of the convolution weight gradient and the exact-integer operands of tests/test_hip_wgrad_paths.py
(a helper, not a test file; tests/test_wgrad_ref.py pins it against a plain Python loop).

    dw[o][i][ky][kx] = sum_{n,y,x} dz[n][o][y][x] * x[n][i][y + ky - pad][x + kx - pad]      (x zero outside its extent)
    db[o]            = sum_{n,y,x} dz[n][o][y][x]

Why integers: with x and dz integers in [-3, 3] every product is an integer of magnitude <= 9, and every partial sum of products of
one dw element -- in ANY order and grouping, split-K slabs and their reduction included -- is an integer whose magnitude is at most
A = the same weight gradient of |x| and |dz|.  While A.max() < 2**24 all of these are exactly representable in fp32 (f16 and bf16
hold the integers up to 3 exactly too), so fp32 accumulation commits no rounding anywhere and a correct kernel equals the float64
reference BIT FOR BIT.  The tolerance of the exact cases is therefore zero by derivation, not by measurement; check_exact_premise
asserts the premise from the reference alone."""
import torch
import torch.nn.functional as F

EXACT_LIMIT = 2 ** 24        # integers of magnitude <= 2**24 are exact in fp32; the premise keeps every partial sum strictly below


def _dw64(x, dz, k, pad):
    n, ci, h, w = x.shape
    co, ho, wo = dz.shape[1], dz.shape[2], dz.shape[3]
    assert dz.shape[0] == n and ho == h + 2 * pad - k + 1 and wo == w + 2 * pad - k + 1, 'dz is not the conv output shape'
    xp = F.pad(x, (pad, pad, pad, pad))
    zf = dz.permute(1, 0, 2, 3).reshape(co, -1)
    dw = torch.empty(co, ci, k, k, dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            win = xp[:, :, ky:ky + ho, kx:kx + wo].permute(1, 0, 2, 3).reshape(ci, -1)
            dw[:, :, ky, kx] = zf @ win.t()
    return dw


def wgrad_ref64(x, dz, k, pad):
    """(dw, db, A) in float64 on the CPU for NCHW x [n][ci][h][w] and dz [n][co][ho][wo]: the weight gradient, the bias gradient and
    A = the weight gradient of (|x|, |dz|), i.e. per dw element the sum of the absolute products."""
    x = x.detach().to('cpu', torch.float64)
    dz = dz.detach().to('cpu', torch.float64)
    return _dw64(x, dz, k, pad), dz.sum((0, 2, 3)), _dw64(x.abs(), dz.abs(), k, pad)


def check_exact_premise(A, dz, times=1):
    """The premise of bitwise equality, from the reference alone: `times` accumulated copies of every sum of absolute products, and of
    every bias sum of absolute values, stay below 2**24."""
    amax = float(A.max()) * times
    bmax = float(dz.detach().to('cpu', torch.float64).abs().sum((0, 2, 3)).max()) * times
    assert amax < EXACT_LIMIT, 'exact-integer premise broken: %d x max sum|x dz| = %.0f >= 2**24' % (times, amax)
    assert bmax < EXACT_LIMIT, 'exact-integer premise broken: %d x max sum|dz| = %.0f >= 2**24' % (times, bmax)


def int_operands(seed, n, civ, ci, cov, co, h, w, ho, wo):
    """Seeded integer operands in [-3, 3] as fp32 NCHW: x [n][civ][h][w] with the channels >= ci zero (view padding), dz
    [n][cov][ho][wo] with the channels >= co zero."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    x = torch.zeros(n, civ, h, w)
    x[:, :ci] = torch.randint(-3, 4, (n, ci, h, w), generator=g).float()
    dz = torch.zeros(n, cov, ho, wo)
    dz[:, :co] = torch.randint(-3, 4, (n, co, ho, wo), generator=g).float()
    return x, dz


def impulse_expected(co, ci, k, pad, xpos, zpos):
    """x = one 1 at xpos = (n, channel, y, x), dz = one 1 at zpos: the float64 (dw, db).  dw has at most one nonzero element: tap
    (ky, kx) = (y_x - y_z + pad, x_x - x_z + pad) of [c_z][c_x] when both impulses sit in the same image and the tap exists."""
    dw = torch.zeros(co, ci, k, k, dtype=torch.float64)
    db = torch.zeros(co, dtype=torch.float64)
    db[zpos[1]] = 1.0
    ky, kx = xpos[2] - zpos[2] + pad, xpos[3] - zpos[3] + pad
    if xpos[0] == zpos[0] and 0 <= ky < k and 0 <= kx < k:
        dw[zpos[1], xpos[1], ky, kx] = 1.0
    return dw, db
