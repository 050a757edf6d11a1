"""The bed DRC (csrc/mk_cascade_adjoint.h) restated on the oracle's model in
arbitrary precision -- the yardstick of tests/test_gpu_cascade_drc.py.  Imports
the oracle and _sens._solve only, never the product.

A bed is a list of oracle models, one per cell (make_cascade_fixture.py:
cell_spec; cell c's inflow_state is the gas of cell c-1), and their full
states.  tests/_sens_multi.py with a cell loop: per cell F, A_c = dF/dy and the
replaced rows as there; an objective is a pair (wr over m.rnames, wy over
m.dyn) read for the bed as

    J = (1/N) sum_c sum_j wr_j net_j(y_c) + sum_a wy_a y_{N-1,a}
    g_c = (1/N) sum_j wr_j dnet_j/dy (y_c) + [c = N-1] wy
    A_c^T mu_c = g_c - phi_{c+1} (.) mu_{c+1}        (mu_N = 0),  c = N-1 ... 0
    xi_j = sum_c net_j(y_c) (wr_j / N - sum_a mu_{c,a} w_{c,a} W_aj) / J
    order_in_a = -mu_{0,a} phi_{0,a} u_{0,a} / J

phi_{c,a} = 1 / residence_time on a gas row of a CSTR cell that was not
replaced, else 0; w_{c,a} the row scale, 0 on a replaced row; u_0 the inflow of
cell 0.  The float inputs are taken as exact numbers; every operation after
them is carried out in `num`: fractions.Fraction or mpmath.mpf at the caller's
working precision."""
from fractions import Fraction

import numpy as np

from oracle import mk_oracle as O
from _sens import _solve


def cell_system(m, y_full, num, kf=None, kr=None):
    """One cell at the full state y_full of its oracle model m: dict(net [R],
    dnet [R] of {a: d net_j / d y_a}, A [nd][nd], w [nd][R] (None where W_aj = 0),
    replaced [nd], phi [nd])."""
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
    phi = [num(0)] * nd
    for a, i in enumerate(dyn):
        for j in range(R):
            if w[a][j] is not None:
                for q, d in dnet[j].items():
                    A[a][q] += w[a][j] * d
        if cstr and m.is_gas[i] > 0:
            phi[a] = num(float(1.0 / m.reactor['residence_time']))
            A[a][a] -= phi[a]
    replaced = [False] * nd
    C, piv = O._rref(m.conservation())
    for l, p in enumerate(piv):
        A[p] = [num(float(v)) for v in C[l]]
        replaced[p] = True
    for a in np.nonzero(m.unreach[dyn])[0]:
        A[a] = [num(1 if q == a else 0) for q in range(nd)]
        replaced[a] = True
    phi = [num(0) if replaced[a] else phi[a] for a in range(nd)]
    return dict(net=net, dnet=dnet, A=A, w=w, replaced=replaced, phi=phi)


def cascade_drc(models, ys_full, objectives, num=Fraction, kf=None, kr=None):
    """([xi over rnames per objective], [J per objective], [order_in over dyn
    per objective]) in `num` for the bed of the cell models `models` at their
    full states ys_full; objectives: a list of (wr, wy), wr over m.rnames and wy
    over m.dyn (floats, taken as exact)."""
    N = len(models)
    assert N >= 1 and len(ys_full) == N
    m0 = models[0]
    dyn = list(m0.dyn)
    nd, R = len(dyn), len(m0.rnames)
    cs = [cell_system(m, y, num, kf, kr) for m, y in zip(models, ys_full)]
    u0 = [num(float(m0.yin[i])) for i in dyn]
    yout = np.asarray(ys_full[-1], float)
    xis, vals, orders = [], [], []
    for wr, wy in objectives:
        wr = [num(float(v)) for v in wr]
        wy = [num(float(v)) for v in wy]
        assert len(wr) == R and len(wy) == nd
        J = num(0)
        for c in cs:
            for j in range(R):
                if wr[j] != 0:
                    J += wr[j] * c['net'][j]
        J = J / N
        for a, i in enumerate(dyn):
            if wy[a] != 0:
                J += wy[a] * num(float(yout[i]))
        acc = [num(0)] * R
        mu_dn, phi_dn = [num(0)] * nd, [num(0)] * nd
        for ci in range(N - 1, -1, -1):
            c = cs[ci]
            g = list(wy) if ci == N - 1 else [num(0)] * nd
            for j in range(R):
                if wr[j] != 0:
                    for q, d in c['dnet'][j].items():
                        g[q] += wr[j] * d / N
            for a in range(nd):
                g[a] -= phi_dn[a] * mu_dn[a]
            At = [[c['A'][q][a] for q in range(nd)] for a in range(nd)]
            mu = _solve(At, g, num)
            for j in range(R):
                s = wr[j] / N
                for a in range(nd):
                    if c['w'][a][j] is not None and not c['replaced'][a]:
                        s -= mu[a] * c['w'][a][j]
                acc[j] += c['net'][j] * s
            mu_dn, phi_dn = mu, c['phi']
        xis.append([x / J for x in acc])
        vals.append(J)
        orders.append([-mu_dn[a] * phi_dn[a] * u0[a] / J for a in range(nd)])
    return xis, vals, orders


def cascade_drc_mp(models, ys_full, objectives, bits, kf=None, kr=None):
    """cascade_drc in mpmath at `bits` of working precision -> mpf lists"""
    import mpmath
    with mpmath.workprec(bits):
        xis, vals, orders = cascade_drc(models, ys_full, objectives, mpmath.mpf, kf, kr)
        return ([[mpmath.mpf(x) for x in xi] for xi in xis], [mpmath.mpf(v) for v in vals],
                [[mpmath.mpf(x) for x in o] for o in orders])
