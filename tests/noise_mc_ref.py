"""NumPy statement of the Monte-Carlo noise-curve stream of include/hhsr.h ("noise curves of the robustness noise model"),
written from the header: Philox4x32-10 words -> Box-Muller normals -> clipped 3 x 3 patch pairs -> float64 means.

`dtype` switches the arithmetic between float32 (what the kernel computes, up to the last bits of its logf / sincosf)
and float64 (the same stream without float32 rounding: the reference of tests/test_noise_curves.py)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """The four output words of one call; counters are arrays (uint64 holding 32-bit values), the key two ints."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in (c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c0  # < 2^64: both factors are below 2^32
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def normals(level, n_patches, seed, dtype=np.float64):
    """[n_patches, 20] standard normals of brightness index `level`: call k fills columns 4k .. 4k + 3."""
    T = np.dtype(dtype).type
    p = np.arange(n_patches, dtype=np.uint64)
    z = np.empty((n_patches, 20), dtype)
    for k in range(5):
        x = philox4x32_10(p, np.full_like(p, level), np.full_like(p, k), np.zeros_like(p), seed & 0xFFFFFFFF, seed >> 32)
        u = [((w >> np.uint64(8)).astype(dtype) + T(0.5)) * T(2.0 ** -24) for w in x]
        for j in range(2):
            r = np.sqrt(T(-2) * np.log(u[2 * j]))
            th = T(2 * np.pi) * u[2 * j + 1]
            z[:, 4 * k + 2 * j] = r * np.cos(th)
            z[:, 4 * k + 2 * j + 1] = r * np.sin(th)
    return z


def pair_values(level, alpha, beta, n_patches, seed, dtype=np.float64):
    """(0.5 (sd1 + sd2), |m1 - m2|) per patch pair, float64 arrays [n_patches]."""
    T = np.dtype(dtype).type
    z = normals(level, n_patches, seed, dtype)
    b = T(np.float32(level / 1000))  # the torch estimator holds the brightness and the profile in float32
    s = np.sqrt(b * T(np.float32(alpha)) + T(np.float32(beta)))

    def stats(zz):
        p = np.clip(b + s * zz, T(0), T(1))
        tot = p[:, 0].copy()
        for j in range(1, 9):  # left to right
            tot = tot + p[:, j]
        m = tot / T(9)
        d = p - m[:, None]
        ss = d[:, 0] * d[:, 0]
        for j in range(1, 9):
            ss = ss + d[:, j] * d[:, j]
        return m, np.sqrt(ss / T(9))

    m1, sd1 = stats(z[:, 0:9])
    m2, sd2 = stats(z[:, 9:18])
    return (T(0.5) * (sd1 + sd2)).astype(np.float64), np.abs(m1 - m2).astype(np.float64)


def noise_mc(levels, alpha, beta, n_patches, seed, dtype=np.float64):
    """Per level of `levels`: (sigma, diff, se_sigma, se_diff), float64 arrays; SE = std(per-pair value) / sqrt(n)."""
    out = np.empty((4, len(levels)))
    for k, lv in enumerate(levels):
        sv, dv = pair_values(int(lv), alpha, beta, n_patches, seed, dtype)
        out[:, k] = sv.sum() / n_patches, dv.sum() / n_patches, sv.std() / np.sqrt(n_patches), dv.std() / np.sqrt(n_patches)
    return tuple(out)
