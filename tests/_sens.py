"""The analytic degree of rate control (csrc/mk_sens.h: k_drc_adjoint) restated
on the oracle's model in arbitrary precision -- the yardstick of
tests/test_gpu_drc_adjoint.py.  Imports the oracle only, never the product.

At a steady state y of F(y, k) = 0 -- F the oracle's rhs with the
conservation laws in their pivot rows and unit rows on the unreachable
species (ClassicModel.find_steady / _polish) --

    A = dF/dy,  b_j = dF/d ln k_j at fixed K_j (= rowscale_i W_ij net_j on rhs
    rows, 0 on replaced rows),  g = d TOF / dy,
    A^T lambda = g,   xi_j = ([j in tof] net_j - lambda . b_j) / TOF

(old_system.py:490-515 in the limit eps -> 0).  The float inputs -- y, kf, kr,
W, the row scales, the rounded concentration of a fixed species -- are taken
as exact numbers; every operation after them is carried out in `num`:
fractions.Fraction (exact) or mpmath.mpf at the working precision set by the
caller.  Derivatives leave one factor out of a product, never divide by a
concentration."""
from fractions import Fraction

import numpy as np

from oracle import mk_oracle as O


def _solve(A, b, num):
    """Gaussian elimination with partial pivoting on lists of `num`."""
    n = len(b)
    A = [row[:] for row in A]
    b = b[:]
    for k in range(n):
        p = max(range(k, n), key=lambda r: abs(A[r][k]))
        if A[p][k] == 0:
            raise ZeroDivisionError('singular steady Jacobian at column %d' % k)
        A[k], A[p] = A[p], A[k]
        b[k], b[p] = b[p], b[k]
        for r in range(k + 1, n):
            if A[r][k] != 0:
                l = A[r][k] / A[k][k]
                for q in range(k, n):
                    A[r][q] -= l * A[k][q]
                b[r] -= l * b[k]
    x = [num(0)] * n
    for k in range(n - 1, -1, -1):
        s = b[k]
        for q in range(k + 1, n):
            s -= A[k][q] * x[q]
        x[k] = s / A[k][k]
    return x


def adjoint_drc(m, y_full, tof_terms, num=Fraction, kf=None, kr=None):
    """(xi over m.rnames, tof0), both in `num`, at the full state y_full of the
    oracle model m (a ClassicModel)."""
    y = np.asarray(y_full, float)
    kf = m.kf if kf is None else np.asarray(kf, float)
    kr = m.kr if kr is None else np.asarray(kr, float)
    dyn = list(m.dyn)
    nd, R = len(dyn), len(m.rnames)
    pos = {i: a for a, i in enumerate(dyn)}
    cols = [int(i) for i in m.jcols]
    # concentrations: cf * y exact for a dynamic species, the rounded float
    # product (what the device is handed) for a fixed one
    conc = {i: (num(float(y[i])) * num(float(m.cfac[i])) if i in pos else num(float(y[i] * m.cfac[i]))) for i in cols}

    def side(k, E, leave=None):
        v = num(float(k))
        for i in cols:
            e = int(E[i])
            if i == leave:
                if e == 0:
                    return num(0)
                v = v * e * num(float(m.cfac[i])) * conc[i] ** (e - 1)
            elif e:
                v = v * conc[i] ** e
        return v

    net = [side(kf[j], m.Ef[j]) - side(kr[j], m.Er[j]) for j in range(R)]
    dnet = [{a: side(kf[j], m.Ef[j], i) - side(kr[j], m.Er[j], i)
             for i, a in pos.items() if m.Ef[j, i] or m.Er[j, i]} for j in range(R)]
    rs = m.rowscale()
    cstr = m.reactor['kind'] == 'CSTR'
    A = [[num(0)] * nd for _ in range(nd)]
    w = [[num(float(rs[i])) * num(float(m.W[i, j])) if m.W[i, j] != 0.0 else None for j in range(R)] for i in dyn]
    for a, i in enumerate(dyn):
        for j in range(R):
            if w[a][j] is not None:
                for q, d in dnet[j].items():
                    A[a][q] += w[a][j] * d
        if cstr and m.is_gas[i] > 0:
            A[a][a] -= num(float(1.0 / m.reactor['residence_time']))
    replaced = [False] * nd
    C, piv = O._rref(m.conservation())
    for l, p in enumerate(piv):
        A[p] = [num(float(v)) for v in C[l]]
        replaced[p] = True
    for a in np.nonzero(m.unreach[dyn])[0]:
        A[a] = [num(1 if q == a else 0) for q in range(nd)]
        replaced[a] = True
    tof_idx = [j for j, rn in enumerate(m.rnames) if rn in tof_terms]
    g = [num(0)] * nd
    for t in tof_idx:
        for q, d in dnet[t].items():
            g[q] += d
    At = [[A[q][a] for q in range(nd)] for a in range(nd)]
    lam = _solve(At, g, num)
    tof0 = sum((net[t] for t in tof_idx), num(0))
    xi = []
    for j in range(R):
        s = num(1 if j in tof_idx else 0)
        for a in range(nd):
            if w[a][j] is not None and not replaced[a]:
                s -= lam[a] * w[a][j]
        xi.append(net[j] * s / tof0)
    return xi, tof0


def adjoint_drc_mp(m, y_full, tof_terms, bits, kf=None, kr=None):
    """adjoint_drc in mpmath at `bits` of working precision -> (float array, float)"""
    import mpmath
    with mpmath.workprec(bits):
        xi, tof0 = adjoint_drc(m, y_full, tof_terms, mpmath.mpf, kf, kr)
        return [mpmath.mpf(x) for x in xi], mpmath.mpf(tof0)
