"""NumPy restatement of the reference's tone mapping (raw2rgb.py:153-170): three exposures of the image, fused by
OpenCV 4.x MergeMertens with createMergeMertens() defaults (contrast weight 1, saturation weight 1, exposure weight 0),
then the smoothstep curve.  Test infrastructure: the yardstick of tests/test_tonemap*.py.

OpenCV and skimage are not available to this project, so this file restates the algorithm operation by operation, the
way oracle.post.unsharp_mask restates skimage.  It has never been compared with a real cv2 run (PARITY.md says so).

Every pyramid function works on the last two axes of an array [..., H, W] and keeps the array's dtype, so the same code
gives the float32 result (what OpenCV computes) and a float64 one (what the float32 rounding is measured against).
"""
import numpy as np

F32 = np.float32
TIMES = (1.0, 0.5, 2.0)  # raw2rgb.py:161


def exposures(image, times=TIMES):
    """Step 1: uint8 [n][H][W][3], img_as_ubyte(clip(image t, 0, 1)) = rint(. 255), half to even, in the image's own
    precision (float32, or float64 after devignetting).  The image is NOT clipped before it is scaled."""
    image = np.asarray(image)
    assert image.dtype in (np.float32, np.float64)
    ty = image.dtype.type
    return np.stack([np.rint(np.clip(image * ty(t), 0, 1) * ty(255)).astype(np.uint8) for t in times])


def to_float(e):
    """Step 2: float32(e) * float32(1 / 255)."""
    return np.asarray(e).astype(F32) * F32(1.0 / 255.0)


def reflect101(i, n):
    """Border index (d c b | a b c d | c b a), applied until the index is in range; 0 when the axis has length 1."""
    i = np.array(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    while ((i < 0) | (i >= n)).any():
        i = np.where(i < 0, -i, i)
        i = np.where(i >= n, 2 * (n - 1) - i, i)
    return i


def weight_maps(I, mean="mul"):
    """Step 3 up to w: I float32 [n][H][W][3] -> w float32 [n][H][W], in exactly the association of the contract.
    mean="div" computes the channel mean as sum / 3 instead of sum * (1 / 3): the sensitivity experiment."""
    I = np.asarray(I)
    assert I.dtype == F32 and I.ndim == 4 and I.shape[-1] == 3
    H, W = I.shape[1:3]
    I0, I1, I2 = I[..., 0], I[..., 1], I[..., 2]
    g = (I0 * F32(0.299) + I1 * F32(0.587)) + I2 * F32(0.114)
    ym, yp = reflect101(np.arange(H) - 1, H), reflect101(np.arange(H) + 1, H)
    xm, xp = reflect101(np.arange(W) - 1, W), reflect101(np.arange(W) + 1, W)
    contrast = np.abs((((g[:, ym, :] + g[:, :, xm]) + g * F32(-4)) + g[:, :, xp]) + g[:, yp, :])
    s = (I0 + I1) + I2
    m = s * F32(1.0 / 3.0) if mean == "mul" else s / F32(3)
    d0, d1, d2 = I0 - m, I1 - m, I2 - m
    saturation = np.sqrt((d0 * d0 + d1 * d1) + d2 * d2)
    w = contrast * saturation + F32(1e-12)
    assert w.dtype == F32
    return w


def normalise(w):
    """wn_i = w_i / ((w_0 + w_1) + w_2 ...)."""
    ws = w[0]
    for i in range(1, len(w)):
        ws = ws + w[i]
    return w / ws


def levels(H, W):
    """Step 4: L = k for 2^k <= min(H, W) < 2^(k + 1).  OpenCV writes int(logf(float(min)) / logf(2.f)); in float32
    that quotient lands within one rounding of an integer at powers of two, so its value there belongs to the platform's
    logf (levels_float32).  The contract is the table, which is what NumPy's float32 log gives for every min <= 8192."""
    return min(H, W).bit_length() - 1


def levels_float32(m):
    """OpenCV's expression evaluated with NumPy's float32 log."""
    return int(np.log(F32(m)) / np.log(F32(2)))


def _down_axis(a, axis):
    n = a.shape[axis]
    c = 2 * np.arange((n + 1) // 2)

    def t(k):
        return np.take(a, reflect101(c + k, n), axis=axis)

    return ((t(0) * 6 + (t(-1) + t(1)) * 4) + t(-2)) + t(2)


def pyr_down(a):
    """Step 5: [1 4 6 4 1] along x, then along y, then 1/256; samples at 2i, size (n + 1) // 2."""
    return _down_axis(_down_axis(a, -1), -2) * a.dtype.type(1.0 / 256.0)


def _up_axis(s, d, axis):
    n = s.shape[axis]
    assert d in (2 * n, 2 * n - 1)
    i = np.arange(n)
    sm = np.take(s, np.where(i == 0, 1 if n > 1 else 0, i - 1), axis=axis)
    sp = np.take(s, np.minimum(i + 1, n - 1), axis=axis)
    shape = list(s.shape)
    shape[axis] = 2 * n
    out = np.empty(shape, s.dtype)
    ev, od = [slice(None)] * s.ndim, [slice(None)] * s.ndim
    ev[axis], od[axis] = slice(0, None, 2), slice(1, None, 2)
    out[tuple(ev)] = (sm + s * 6) + sp
    out[tuple(od)] = (s + sp) * 4
    return np.take(out, np.arange(d), axis=axis)


def pyr_up(s, shape):
    """Step 6: to (shape[0], shape[1]), each 2n or 2n - 1."""
    return _up_axis(_up_axis(s, shape[1], -1), shape[0], -2) * s.dtype.type(1.0 / 64.0)


def blend(I, wn, dtype=F32):
    """Step 7: I float32 [n][H][W][3], wn float32 [n][H][W] -> R_0 [H][W][3] of `dtype` (every pyramid in `dtype`)."""
    n, H, W, _ = I.shape
    L = levels(H, W)
    G = [np.moveaxis(np.asarray(I), -1, 1).astype(dtype)]  # [n][3][H][W]
    Wp = [np.asarray(wn).astype(dtype)[:, None]]           # [n][1][H][W]
    for _ in range(L):
        G.append(pyr_down(G[-1]))
        Wp.append(pyr_down(Wp[-1]))
    R = []
    for lv in range(L + 1):
        lap = G[lv] - pyr_up(G[lv + 1], G[lv].shape[-2:]) if lv < L else G[lv]
        t = lap * Wp[lv]
        r = t[0]
        for i in range(1, n):
            r = r + t[i]
        R.append(r)
    for lv in range(L, 0, -1):
        R[lv - 1] = R[lv - 1] + pyr_up(R[lv], R[lv - 1].shape[-2:])
    assert R[0].dtype == dtype
    return np.moveaxis(R[0], 0, -1)


def smoothstep(r):
    """Step 8: 3 r^2 - 2 r^3 in r's dtype."""
    return 3 * r ** 2 - 2 * r ** 3


def mertens(exp_u8, smooth=True, dtype=F32, mean="mul"):
    """Steps 2-8 on uint8 exposures [n][H][W][3]: (fused image of `dtype`, normalised float32 weights)."""
    I = to_float(exp_u8)
    wn = normalise(weight_maps(I, mean))
    r = blend(I, wn, dtype)
    return (smoothstep(r) if smooth else r), wn


def tonemap(image, smooth=True, dtype=F32):
    """apply_smoothstep (raw2rgb.py:153-170) of a float32 / float64 image [H][W][3]."""
    return mertens(exposures(image), smooth, dtype)[0]
