"""Fixture of the device eigenvalue kernels (csrc/mk_eig.h; pck_eigvals,
pck_stability_at): real matrices with their exact spectra.  CPU only; imports
the oracle only.  The tests read the .npz alone.

The yardstick is mpmath.eig at 400 bits on the float matrix, rounded to
complex128.  Per matrix `m<i>_...` (name in `names[i]`):
  A          the matrix [ns, ns]
  w          its exact spectrum (complex128)
  scale      ns * eps * ||B||_F, B = scipy.linalg.matrix_balance(A, permute=False)
             (the backward error of Hessenberg QR on the balanced matrix)
  np_ratio   what numpy reaches: the worst of eigvals(A), eigvals(A.T) and
             eigvals(A[::-1, ::-1]), Hausdorff distance to w over scale
             (asserted <= 10 here: the condition under which a bound of 10 x
             scale on the device tests something)

(a) random row-graded matrices, randn * exp(U(-10, 10)) per row, at ns = 1, 2,
    3, 4, 8, 9, 16, 17, 32, 33 (three each) and 64 (two);
(b) structured: zero, diagonal, upper triangular, a 2 x 2 rotation-scaling
    block embedded at size 3 and 9, companion matrices of well-separated real
    and complex roots (no defective matrices: numpy does not stay inside the
    bound on them);
(c) oracle Jacobians at oracle steady states, full (`..._full`) and reduced on
    the conservation laws (`..._red`): the six volcano points, DMTM at 450 and
    650 K (p = 1e4 Pa), and the CH4 patched _jac_ss at the 8 temperatures of
    ch4_fixture.npz (full only: the reference's test).  The reduced matrix is
    formed in mpmath from the float Jacobian, the laws C in reduced row-echelon
    form and their pivots p_l,
        Jr[i][q] = J[i][q] - sum_l J[i][p_l] C[l][q] / C[l][p_l]   (i, q not pivots),
    and rounded once.  These cases also hold what the device needs to rebuild
    the Jacobian: T, p, desc_names / desc, dyn (the species of the rows), y,
    rnames, kf, kr; the reduced ones `keep` (the non-pivot species, in order)
    and `stable` (exact re_max < -10 * scale: the verdict is decidable).

    OMP_NUM_THREADS=1 python tests/golden/make_spectrum_fixture.py

writes tests/golden/spectrum_fixture.npz (numpy arrays only).
"""
import multiprocessing as mp
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
INPUTS = os.path.join(HERE, 'inputs')
OUT = os.path.join(HERE, 'spectrum_fixture.npz')
sys.path.insert(0, ROOT)

BITS = 400
SEED = 20261021
SIZES = ((1, 3), (2, 3), (3, 3), (4, 3), (8, 3), (9, 3), (16, 3), (17, 3), (32, 3), (33, 3), (64, 2))
VOLCANO = [(-1.0, -1.0), (-2.5, -2.5), (0.5, 0.5), (-2.5, 0.5), (0.5, -2.5), (-1.3, -0.4)]
DMTM = [(450.0, 1e4), (650.0, 1e4)]
NP_RATIO_MAX = 10.0
EPS = float(np.finfo(float).eps)


def hausdorff(a, b):
    d = np.abs(np.asarray(a)[:, None] - np.asarray(b)[None, :])
    return float(max(d.min(axis=0).max(), d.min(axis=1).max()))


def scale_of(A):
    from scipy.linalg import matrix_balance
    B = matrix_balance(np.asarray(A, float), permute=False)[0]
    return A.shape[0] * EPS * float(np.linalg.norm(B))


def exact_spectrum(A):
    import mpmath
    with mpmath.workprec(BITS):
        E = mpmath.eig(mpmath.matrix(A.tolist()), left=False, right=False)
        E = E[0] if isinstance(E, tuple) else E
        return np.array([complex(e) for e in E])


def reduced_mp(J, C, piv):
    """the reduced Jacobian formed in mpmath, rounded once; and the kept species"""
    import mpmath
    n = J.shape[0]
    keep = [i for i in range(n) if i not in piv]
    with mpmath.workprec(BITS):
        Jr = np.zeros((len(keep), len(keep)))
        for a, i in enumerate(keep):
            for b, q in enumerate(keep):
                v = mpmath.mpf(float(J[i, q]))
                for l, p in enumerate(piv):
                    v -= mpmath.mpf(float(J[i, p])) * mpmath.mpf(float(C[l, q])) / mpmath.mpf(float(C[l, p]))
                Jr[a, b] = float(v)
    return Jr, keep


def companion(roots):
    c = np.poly(roots).real
    n = len(roots)
    A = np.zeros((n, n))
    A[0, :] = -c[1:]
    A[np.arange(1, n), np.arange(n - 1)] = 1.0
    return A


def plain_cases():
    rng = np.random.default_rng(SEED)
    for ns, count in SIZES:
        for k in range(count):
            yield 'rand%d_%d' % (ns, k), rng.standard_normal((ns, ns)) * np.exp(rng.uniform(-10.0, 10.0, (ns, 1)))
    yield 'zero4', np.zeros((4, 4))
    yield 'diag5', np.diag([1.0, -2.0, 3.0e3, 1.0e-5, -7.0e-2])
    yield 'triu6', np.triu(rng.standard_normal((6, 6)))
    for n in (3, 9):
        A = np.diag(-1.0 - np.arange(n, dtype=float))
        A[:2, :2] = [[1.0, -2.0], [2.0, 1.0]]
        yield 'rot%d' % n, A
    yield 'comp_real', companion([1.0, 2.0, 3.0, 4.5, -6.0])
    yield 'comp_cplx', companion([1 + 2j, 1 - 2j, -3.0, 0.5 + 0.1j, 0.5 - 0.1j, -4 + 1j, -4 - 1j])


def oracle_cases():
    """name, matrix, extra entries"""
    from oracle import mk_oracle as O

    def classic(name, m, y, desc):
        dyn = list(m.dyn)
        J = m.jac(y)[np.ix_(dyn, dyn)]
        base = dict(T=np.array(float(m.T)), p=np.array(float(m.p)), desc_names=np.array(sorted(desc)),
                    desc=np.array([desc[k] for k in sorted(desc)], float),
                    dyn=np.array([m.snames[q] for q in dyn]), rnames=np.array(m.rnames), y=np.array(y)[dyn],
                    kf=m.kf.copy(), kr=m.kr.copy())
        yield name + '_full', J, base
        C, piv = O._rref(m.conservation())
        Jr, keep = reduced_mp(J, C, piv)
        yield name + '_red', Jr, dict(base, keep=np.array(keep), cons_C=C, cons_piv=np.array(piv))

    spec = O.load_spec(os.path.join(INPUTS, 'COOxVolcano', 'input.json'))
    for eco, eo in VOLCANO:
        r = O.volcano_steady(spec, eco, eo)
        assert r is not None, (eco, eo)
        yield from classic('volcano_%g_%g' % (eco, eo), r['model'], r['y'], dict(ECO=eco, EO=eo))
    spec = O.load_spec(os.path.join(INPUTS, 'DMTM', 'input.json'))
    for T, p in DMTM:
        m = O.ClassicModel(spec, T=T, p=p)
        y, _ = m.solve_odes(rtol=1e-6, atol=1e-12)
        y = m.find_steady(y)
        yield from classic('dmtm_%g_%g' % (T, p), m, y, {})
    cfx = np.load(os.path.join(HERE, 'ch4_fixture.npz'))
    spec = O.ch4_setup(O.load_spec(os.path.join(INPUTS, 'CH4', 'input.json')), 1.0, 1.0)
    for k, T in enumerate(cfx['T']):
        m = O.PatchedModel(spec, T=float(T))
        names = sorted(m.index, key=m.index.get)[m.ngas:]
        assert names == [str(x) for x in cfx['names']]
        yield 'ch4_%d_full' % k, m.jac_ss(cfx['y'][k]), dict(T=np.array(float(T)), y=cfx['y'][k].copy(),
                                                              dyn=np.array(names))


def _one(job):
    name, A, extra = job
    t0 = time.time()
    w = exact_spectrum(A)
    sc = scale_of(A)
    worst = 0.0
    for M in (A, A.T, A[::-1, ::-1]):
        h = hausdorff(np.linalg.eigvals(M), w)
        worst = max(worst, h / sc if sc > 0.0 else h)
    o = dict(A=A, w=w, scale=np.array(sc), np_ratio=np.array(worst))
    o.update(extra)
    if name.endswith('_red'):
        o['stable'] = np.array(bool(w.real.max() < -10.0 * sc))
    return name, o, time.time() - t0


def main():
    t0 = time.time()
    jobs = [(n, A, {}) for n, A in plain_cases()] + list(oracle_cases())
    order = {j[0]: k for k, j in enumerate(jobs)}
    jobs.sort(key=lambda j: -j[1].shape[0])          # the 64 x 64 matrices first
    with mp.get_context('fork').Pool(8) as pool:
        res = pool.map(_one, jobs, chunksize=1)
    res.sort(key=lambda r: order[r[0]])
    out, names = {}, []
    for i, (name, o, dt) in enumerate(res):
        names.append(name)
        for k, v in o.items():
            out['m%d_%s' % (i, k)] = v
        print('%-24s ns %2d  scale %.3e  re_max %+.6e  numpy ratio %.3g%s  (%.0f s)'
              % (name, o['A'].shape[0], float(o['scale']), o['w'].real.max(), float(o['np_ratio']),
                 '  stable %d' % bool(o['stable']) if 'stable' in o else '', dt), flush=True)
        assert float(o['np_ratio']) <= NP_RATIO_MAX, name
    out['names'] = np.array(names)
    np.savez_compressed(OUT, **out)
    print('wrote %s (%d matrices, %d bytes, worst numpy ratio %.3g, %.0f s)'
          % (OUT, len(names), os.path.getsize(OUT), max(float(r[1]['np_ratio']) for r in res), time.time() - t0))


if __name__ == '__main__':
    main()
