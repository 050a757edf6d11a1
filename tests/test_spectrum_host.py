"""The serial core of k_eig_lane on the CPU (no GPU needed): tests/eig_host_check.hip,
a stand-alone host program over the __host__ __device__ text of csrc/mk_eig.h
(eig_serial: balancing, Hessenberg reduction, double-shift QR), compiled here
with the build's flags and run once in a child process; nothing in it calls
the device.

Every fixture matrix of ns <= 8 must come within 10 x scale (Hausdorff) of its
exact spectrum, with scale = ns eps ||B||_F as the fixture has it; a matrix
with a NaN or an Inf entry is PCK_ST_NONFINITE, one that is given a single
sweep where it needs more is PCK_ST_EIG_NOCONV, and an all-NaN matrix ends."""
import os
import struct
import subprocess

import numpy as np
import pytest

import __graft_entry__ as G
from pycatkin_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
FX = np.load(os.path.join(HERE, 'golden', 'spectrum_fixture.npz'))
NAMES = [str(x) for x in FX['names']]
SMALL = [i for i in range(len(NAMES)) if FX['m%d_A' % i].shape[0] <= _lib.MAX_DYN_LANE]


def hausdorff(a, b):
    d = np.abs(np.asarray(a)[:, None] - np.asarray(b)[None, :])
    return float(max(d.min(axis=0).max(), d.min(axis=1).max()))


def special():
    """(label, matrix, budget, expected status)"""
    hard = FX['m%d_A' % NAMES.index('rand8_0')]
    nan1, inf1 = hard.copy(), hard.copy()
    nan1[3, 5] = np.nan
    inf1[7, 0] = -np.inf
    return [('one NaN', nan1, 0, _lib.ST_NONFINITE), ('one Inf', inf1, 0, _lib.ST_NONFINITE),
            ('all NaN', np.full((8, 8), np.nan), 0, _lib.ST_NONFINITE),
            ('one sweep', hard, 1, _lib.ST_EIG_NOCONV), ('the kernel budget', hard, 300, _lib.ST_OK)]


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    """[(status, scale, w)] of the fixture matrices of ns <= 8, then of special()"""
    d = tmp_path_factory.mktemp('eig_host')
    exe, fin, fout = str(d / 'eig_host_check'), str(d / 'in.bin'), str(d / 'out.bin')
    p = subprocess.run([G.HIPCC] + G.HIPFLAGS + ['-I' + os.path.join(G.ROOT, 'include'), '-o', exe,
                                                 os.path.join(HERE, 'eig_host_check.hip')],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    mats = [(FX['m%d_A' % i], 0) for i in SMALL] + [(A, b) for _, A, b, _ in special()]
    with open(fin, 'wb') as fh:
        fh.write(struct.pack('i', len(mats)))
        for A, budget in mats:
            fh.write(struct.pack('ii', A.shape[0], budget))
            fh.write(np.ascontiguousarray(A, float).tobytes())
    p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    raw, pos, out = np.fromfile(fout), 0, []
    for A, _ in mats:
        ns = A.shape[0]
        out.append((int(raw[pos]), raw[pos + 1], raw[pos + 2:pos + 2 + ns] + 1j * raw[pos + 2 + ns:pos + 2 + 2 * ns]))
        pos += 2 + 2 * ns
    assert pos == raw.size
    return out


def test_fixture_matrices_within_the_bound(host):
    worst = {}
    for (st, sc, w), i in zip(host, SMALL):
        ref, scale, ns = FX['m%d_w' % i], float(FX['m%d_scale' % i]), FX['m%d_A' % i].shape[0]
        assert st == _lib.ST_OK, NAMES[i]
        assert abs(sc - scale) <= 1e-12 * scale, (NAMES[i], sc, scale)
        h = hausdorff(w, ref)
        worst[ns] = max(worst.get(ns, 0.0), h / scale if scale > 0 else h)
        assert h <= 10.0 * scale, (NAMES[i], h, scale)
        # conjugate pairs adjacent, positive imaginary part first
        k = 0
        while k < ns:
            if w[k].imag != 0.0:
                assert w[k].imag > 0.0 and w[k + 1] == np.conj(w[k]), (NAMES[i], w)
                k += 2
            else:
                k += 1
    print('worst Hausdorff distance / scale per size:', {k: '%.3g' % v for k, v in sorted(worst.items())})


def test_statuses(host):
    for (st, sc, w), (label, A, budget, want) in zip(host[len(SMALL):], special()):
        assert st == want, (label, st)
        if want != _lib.ST_OK:
            assert np.isnan(w.real).all() and np.isnan(w.imag).all(), label
        else:
            i = NAMES.index('rand8_0')
            assert hausdorff(w, FX['m%d_w' % i]) <= 10.0 * float(FX['m%d_scale' % i])
