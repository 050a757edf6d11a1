"""Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11) restated in numpy, and on
top of it the noise of pck_ensemble_noise as include/pycatkin_amd.h states it:
the yardstick of tests/test_gpu_uncertainty.py, itself checked against the
published known answers in tests/test_uncertainty.py."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (uint32 values, broadcast together) -> [..., 4] uint32."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = (np.asarray(key)[..., i].astype(np.uint64) for i in range(2))
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> S32) ^ c[1] ^ k0, p1 & MASK, (p0 >> S32) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def bits53(w0, w1):
    return ((w0.astype(np.uint64) << S32) | w1.astype(np.uint64)) >> np.uint64(11)


def block(seed, runs, j):
    """Philox block j of every run: [len(runs), 4] uint32."""
    runs = np.asarray(runs, np.uint64)
    ctr = np.stack([runs & MASK, runs >> S32, np.full_like(runs, j), np.zeros_like(runs)], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64)
    return philox4x32_10(ctr, key)


def normal(seed, runs):
    """z of every run (Box-Muller on block 0)."""
    g = block(seed, runs, 0)
    u1 = (bits53(g[:, 0], g[:, 1]) + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    u2 = bits53(g[:, 2], g[:, 3]).astype(np.float64) * 2.0 ** -53
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def uniforms(seed, runs, n_ts):
    """u [n_ts, len(runs)] of the transition states."""
    out = np.empty((n_ts, len(runs)))
    for j in range(1, 1 + (n_ts + 1) // 2):
        t = block(seed, runs, j)
        out[2 * (j - 1)] = bits53(t[:, 0], t[:, 1]).astype(np.float64) * 2.0 ** -53
        if 2 * (j - 1) + 1 < n_ts:
            out[2 * (j - 1) + 1] = bits53(t[:, 2], t[:, 3]).astype(np.float64) * 2.0 ** -53
    return out
