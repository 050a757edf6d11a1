"""The multi-objective analytic degree of rate control (csrc/mk_sens_multi.h:
k_multi_adjoint) restated on the oracle's model in arbitrary precision -- the
yardstick of tests/test_gpu_drc_multi.py.  Imports the oracle and
_sens._solve only, never the product.

tests/_sens.py with a general objective.  At a steady state y of F(y, k) = 0
(F, A = dF/dy and b_j = dF/d ln k_j as _sens.py poses them) an objective is a
pair (wr over m.rnames, wy over m.dyn):

    J = sum_j wr_j net_j + sum_a wy_a y_a        (y_a the state variable itself,
                                                 not its concentration cf_a y_a)
    g = dJ/dy,   A^T lambda = g,
    xi_j = net_j (wr_j - sum_a lambda_a w_a W_aj) / J

One elimination per objective (the device factors once and replays; on the CPU
the plain way is the independent one).  The float inputs are taken as exact
numbers; every operation after them is carried out in `num`:
fractions.Fraction or mpmath.mpf at the caller's working precision."""
from fractions import Fraction

import numpy as np

from oracle import mk_oracle as O
from _sens import _solve


def multi_drc(m, y_full, objectives, num=Fraction, kf=None, kr=None):
    """([xi over m.rnames per objective], [J per objective]) in `num` at the
    full state y_full of the oracle model m; objectives: a list of (wr, wy),
    wr over m.rnames and wy over m.dyn (floats, taken as exact)."""
    y = np.asarray(y_full, float)
    kf = m.kf if kf is None else np.asarray(kf, float)
    kr = m.kr if kr is None else np.asarray(kr, float)
    dyn = list(m.dyn)
    nd, R = len(dyn), len(m.rnames)
    pos = {i: a for a, i in enumerate(dyn)}
    cols = [int(i) for i in m.jcols]
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
    At = [[A[q][a] for q in range(nd)] for a in range(nd)]
    xis, vals = [], []
    for wr, wy in objectives:
        wr = [num(float(v)) for v in wr]
        wy = [num(float(v)) for v in wy]
        assert len(wr) == R and len(wy) == nd
        g = list(wy)
        J = num(0)
        for j in range(R):
            if wr[j] != 0:
                J += wr[j] * net[j]
                for q, d in dnet[j].items():
                    g[q] += wr[j] * d
        for a, i in enumerate(dyn):
            if wy[a] != 0:
                J += wy[a] * num(float(y[i]))
        lam = _solve(At, g, num)
        xi = []
        for j in range(R):
            s = wr[j]
            for a in range(nd):
                if w[a][j] is not None and not replaced[a]:
                    s -= lam[a] * w[a][j]
            xi.append(net[j] * s / J)
        xis.append(xi)
        vals.append(J)
    return xis, vals


def multi_drc_mp(m, y_full, objectives, bits, kf=None, kr=None):
    """multi_drc in mpmath at `bits` of working precision -> (mpf lists, mpf list)"""
    import mpmath
    with mpmath.workprec(bits):
        xis, vals = multi_drc(m, y_full, objectives, mpmath.mpf, kf, kr)
        return [[mpmath.mpf(x) for x in xi] for xi in xis], [mpmath.mpf(v) for v in vals]
