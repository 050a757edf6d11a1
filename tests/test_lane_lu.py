"""The lane LU on the device, swap path included (tests/lane_lu_check.hip, a
stand-alone program compiled here with the build's flags and run once in a
child process): for NS = 2, 4, 5, 8 it factors and solves 256 systems, one
lane each in four wavefronts, with lu() + lu_solve() (the branch on the
wave-uniform `swaps` taken per solve) and with lu() + lu_solve_impl<NS, SWAPS>
chosen once from `swaps`, as the lane integrator's stage sequence does
(mk_solver.h: rodas_stages).  The optimistic no-pivot factorisation this test
was first written against is not in the tree (DESIGN.md "Lane step chain":
it slowed the CSTR sweep), so the second path is the shipped one.

    wavefront 0  diagonally dominant matrices: no lane votes
    wavefront 1  the matrices of wavefront 0, lane 17 needing a swap at column 0
    wavefront 2  every lane swaps, at a column and a row that vary over the
                 lanes (the last column that can swap included); where the
                 column is 0 every third lane's diagonal entry is exactly 0
    wavefront 3  general matrices (singular values in [1, 100]); lane 40 singular
                 (a column of zeros)

The two paths must agree bitwise (factors, solutions, ok) and report a swap
in wavefronts 1 to 3 only; the lanes of
wavefront 1 that do not swap must equal wavefront 0 bitwise; only the singular
lane reports !ok.  Accuracy: the pivoting path against numpy.linalg.solve on
all the non-singular systems (condition number <= 1e3, asserted), relative
error max|x - x_ref| / max|x_ref|, with the tolerance ten times the worst
relative error of a numpy restatement of the same threshold-pivot LU (tau
0.1, true divisions) on the same systems, per NS.  Measured with this seed
(condition numbers at most 36 / 96 / 63 / 87): the restatement's worst
relative error is 2.83e-15 (NS 2), 2.92e-15 (NS 4), 5.21e-15 (NS 5) and
3.13e-14 (NS 8), so the bounds are 2.8e-14, 2.9e-14, 5.2e-14 and 3.1e-13.
The device's worst on an MI355X: 4.7e-15, 2.5e-15, 3.6e-15 and 1.6e-14.
"""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as G

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (2, 4, 5, 8)
NSYS = 256
NPATH = 2          # lu + lu_solve; lu + lu_solve_impl chosen once
SWAP_LANE = 17       # wavefront 1
SINGULAR = 3 * 64 + 40
TAU = 0.1


def _dominant(rng, n, NS):
    """Row- and column-dominant by a factor > 10: elimination keeps the
    dominance, so the threshold rule never swaps."""
    A = rng.uniform(-1.0, 1.0, (n, NS, NS))
    d = (10.0 * NS + 2.0 + rng.uniform(0.0, 1.0, (n, NS))) * rng.choice([-1.0, 1.0], (n, NS))
    A[:, np.arange(NS), np.arange(NS)] = d
    return A


def systems(NS, seed=20240607):
    rng = np.random.default_rng(seed + NS)
    A = np.empty((NSYS, NS, NS))
    A[0:64] = _dominant(rng, 64, NS)
    A[64:128] = A[0:64]
    A[64 + SWAP_LANE, [0, 1]] = A[64 + SWAP_LANE, [1, 0]]      # rows 0 and 1 exchanged
    D = _dominant(rng, 64, NS)
    for lane in range(64):
        k = lane % (NS - 1)
        r = k + 1 + (lane // (NS - 1)) % (NS - 1 - k)
        if lane % 3 == 0:
            D[lane, r, k] = 0.0                  # the diagonal entry after the row exchange
        D[lane, [k, r]] = D[lane, [r, k]]
    A[128:192] = D
    q1 = np.linalg.qr(rng.standard_normal((64, NS, NS)))[0]
    q2 = np.linalg.qr(rng.standard_normal((64, NS, NS)))[0]
    s = 10.0 ** rng.uniform(0.0, 2.0, (64, NS))
    A[192:256] = np.einsum('nij,nj,nkj->nik', q1, s, q2)
    A[SINGULAR, :, min(1, NS - 1)] = 0.0
    b = rng.uniform(-1.0, 1.0, (NSYS, NS))
    b[64:128] = b[0:64]
    return A, b


def threshold_lu_solve(A, b, tau=TAU):
    """numpy restatement of lu() + lu_solve() (mk_device.h) over a batch: the
    threshold rule, the row exchange of the trailing columns, the forward
    sweep and the back substitution from the last column inward, with true
    divisions.  Returns the solutions and the per-column swap flags."""
    A, x = A.copy(), b.copy()
    n, NS, _ = A.shape
    idx = np.arange(n)
    swapped = np.zeros((n, NS), dtype=bool)
    for k in range(NS):
        cand = np.abs(A[:, k:, k])
        cand[:, 0] /= tau
        p = k + np.argmax(cand, axis=1)          # the first largest: the diagonal keeps a tie
        swapped[:, k] = p != k
        rk, rp = A[idx, k, k:].copy(), A[idx, p, k:].copy()
        A[idx, k, k:], A[idx, p, k:] = rp, rk
        xk, xp = x[idx, k].copy(), x[idx, p].copy()
        x[idx, k], x[idx, p] = xp, xk
        for r in range(k + 1, NS):
            m = A[:, r, k] / A[:, k, k]
            A[:, r, k] = m
            A[:, r, k + 1:] -= m[:, None] * A[:, k, k + 1:]
            x[:, r] -= m * x[:, k]
    for k in range(NS - 1, -1, -1):
        v = x[:, k].copy()
        for q in range(NS - 1, k, -1):
            v -= A[:, k, q] * x[:, q]
        x[:, k] = v / A[:, k, k]
    return x, swapped


def rel_err(x, ref):
    return np.abs(x - ref).max(axis=1) / np.abs(ref).max(axis=1)


@pytest.fixture(scope='module')
def device(tmp_path_factory):
    """{NS: (A, b, out)} with out[path][system] = dict(lu, x, ok, fb = the wavefront swapped); one
    compile and one run for the whole module."""
    d = tmp_path_factory.mktemp('lane_lu')
    exe, fin, fout = str(d / 'lane_lu_check'), str(d / 'in.bin'), str(d / 'out.bin')
    p = subprocess.run([G.HIPCC] + G.HIPFLAGS + ['-I' + os.path.join(G.ROOT, 'include'), '-o', exe,
                                                 os.path.join(HERE, 'lane_lu_check.hip')],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    data = {NS: systems(NS) for NS in SIZES}
    with open(fin, 'wb') as fh:
        for NS in SIZES:
            fh.write(np.ascontiguousarray(data[NS][0]).tobytes())
            fh.write(np.ascontiguousarray(data[NS][1]).tobytes())
    p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    raw = np.fromfile(fout, dtype=np.float64)
    res, pos = {}, 0
    for NS in SIZES:
        rec = NS * NS + NS + 2
        o = raw[pos:pos + NPATH * NSYS * rec].reshape(NPATH, NSYS, rec)
        pos += NPATH * NSYS * rec
        res[NS] = (data[NS][0], data[NS][1],
                   dict(lu=o[:, :, :NS * NS], x=o[:, :, NS * NS:NS * NS + NS], ok=o[:, :, NS * NS + NS],
                        fb=o[:, :, NS * NS + NS + 1]))
    assert pos == raw.size
    return res


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize('NS', SIZES)
def test_one_branch_path_equals_per_solve_branch_path_bitwise(device, NS):
    o = device[NS][2]
    # the cases are what they claim to be: no lane of wavefront 0 swaps, some
    # lane of each of the other three does
    for path in range(NPATH):
        assert np.all(o['fb'][path, 0:64] == 0.0)
        assert np.all(o['fb'][path, 64:256] == 1.0)
    for path in (1,):
        for key in ('lu', 'x', 'ok'):
            differ = np.nonzero(bits(o[key][0]).reshape(NSYS, -1) != bits(o[key][path]).reshape(NSYS, -1))[0]
            assert differ.size == 0, (path, key, np.unique(differ)[:10])


@pytest.mark.parametrize('NS', SIZES)
def test_non_swapping_lanes_of_a_voting_wave_are_unchanged(device, NS):
    o = device[NS][2]
    keep = np.arange(64) != SWAP_LANE
    for path in range(NPATH):
        for key in ('lu', 'x', 'ok'):
            assert np.array_equal(bits(o[key][path, 0:64][keep]), bits(o[key][path, 64:128][keep])), (path, key)
    # and the swapping lane did change
    assert not np.array_equal(bits(o['x'][1, SWAP_LANE]), bits(o['x'][1, 64 + SWAP_LANE]))


@pytest.mark.parametrize('NS', SIZES)
def test_only_the_singular_lane_reports_not_ok(device, NS):
    o = device[NS][2]
    for path in range(NPATH):
        bad = np.nonzero(o['ok'][path] != 1.0)[0]
        assert bad.tolist() == [SINGULAR], (path, bad)


@pytest.mark.parametrize('NS', SIZES)
def test_pivoting_path_agrees_with_numpy(device, NS):
    A, b, o = device[NS]
    good = np.arange(NSYS) != SINGULAR
    A, b = A[good], b[good]
    cond = np.linalg.cond(A)
    assert cond.max() <= 1e3, cond.max()
    ref = np.linalg.solve(A, b[:, :, None])[:, :, 0]
    xr, swapped = threshold_lu_solve(A, b)
    # the restatement sees the cases as built: no swap in wavefront 0, one in
    # every lane of wavefront 2 (the last column that can swap among them)
    assert not swapped[0:64].any()
    assert swapped[64 + SWAP_LANE, 0]
    assert swapped[128:192].any(axis=1).all() and swapped[128:192, NS - 2].any()
    tol = 10.0 * rel_err(xr, ref).max()
    err = rel_err(o['x'][0][good], ref)
    print('NS %d: cond max %.3g, numpy restatement worst rel err %.3g, tolerance %.3g, device worst %.3g'
          % (NS, cond.max(), tol / 10.0, tol, err.max()))
    assert err.max() <= tol, (err.max(), tol, int(np.argmax(err)))
