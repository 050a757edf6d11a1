"""The adjoint sensitivities (csrc/mk_sens.h: k_sens_adjoint) restated on the
oracle's model in arbitrary precision -- the yardstick of
tests/test_gpu_sensitivities.py.  Imports the oracle only, never the product.

At a steady state y of F(y, theta) = 0 -- F as tests/_sens.py poses it: the
oracle's rhs with the CSTR flow term, the conservation laws in their pivot
rows and unit rows on the unreachable species (m.unreach) --

    A = dF/dy,  g = d TOF / dy,  A^T lambda = g,
    d TOF / d theta = dTOF/dtheta|_y - lambda . dF/dtheta|_y

for any parameter theta.  With rf_j / rr_j the forward / reverse rate of
reaction j, w_ij = rowscale_i W_ij on rhs rows (0 on replaced rows) and the
bracket s_j = [j in tof] - sum_i lambda_i w_ij:

    xi_j     = (rf_j - rr_j) s_j / TOF          d ln TOF / d ln k_j at fixed K_j
    sf_j     = rf_j s_j / TOF                   d ln TOF / d ln kf_j
    sr_j     = -rr_j s_j / TOF                  d ln TOF / d ln kr_j
    order_q  = sum_j s_j (Ef_jq rf_j - Er_jq rr_j) / TOF    fixed species q
    order_in_i = -lambda_i in_i / (tau TOF)     the CSTR's inflow of gas species i
    dir      = sum_j s_j (rf_j a_j - rr_j c_j) / TOF        a direction (d ln kf, d ln kr)

The float inputs are taken as exact numbers and every operation after them is
carried out in `num` (fractions.Fraction or mpmath.mpf at the caller's working
precision), as in tests/_sens.py."""
from fractions import Fraction

import numpy as np

from oracle import mk_oracle as O

from _sens import _solve

ERR_UNIT_LOG2 = -98          # the guard's constant: err = 2^-98 max rate / |TOF| (mk_sens.h: PCK_SENS_ERR_UNIT)


def adjoint_sens(m, y_full, tof_terms, num=Fraction, kf=None, kr=None, directions=()):
    """dict(xi, sf, sr [R], order {fixed species name: .}, order_in {dynamic
    species with a flow term: .}, dir [len(directions)], tof0, ratio = max rate /
    |TOF|), all in `num`, at the full state y_full of the oracle model m (a
    ClassicModel).  directions: (a, c) pairs of float vectors over m.rnames."""
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

    rf = [side(kf[j], m.Ef[j]) for j in range(R)]
    rr = [side(kr[j], m.Er[j]) for j in range(R)]
    dnet = [{a: side(kf[j], m.Ef[j], i) - side(kr[j], m.Er[j], i)
             for i, a in pos.items() if m.Ef[j, i] or m.Er[j, i]} for j in range(R)]
    rs = m.rowscale()
    cstr = m.reactor['kind'] == 'CSTR'
    A = [[num(0)] * nd for _ in range(nd)]
    w = [[num(float(rs[i])) * num(float(m.W[i, j])) if m.W[i, j] != 0.0 else None for j in range(R)] for i in dyn]
    flow = [num(0)] * nd
    for a, i in enumerate(dyn):
        for j in range(R):
            if w[a][j] is not None:
                for q, d in dnet[j].items():
                    A[a][q] += w[a][j] * d
        if cstr and m.is_gas[i] > 0:
            flow[a] = num(float(1.0 / m.reactor['residence_time']))
            A[a][a] -= flow[a]
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
    tof0 = sum((rf[t] - rr[t] for t in tof_idx), num(0))
    s = []
    for j in range(R):
        v = num(1 if j in tof_idx else 0)
        for a in range(nd):
            if w[a][j] is not None and not replaced[a]:
                v -= lam[a] * w[a][j]
        s.append(v)
    out = dict(tof0=tof0, xi=[(rf[j] - rr[j]) * s[j] / tof0 for j in range(R)],
               sf=[rf[j] * s[j] / tof0 for j in range(R)], sr=[-(rr[j] * s[j]) / tof0 for j in range(R)])
    out['order'] = {m.snames[q]: sum((s[j] * (int(m.Ef[j, q]) * rf[j] - int(m.Er[j, q]) * rr[j]) for j in range(R)),
                                     num(0)) / tof0
                    for q in cols if q not in pos}
    out['order_in'] = {m.snames[i]: (num(0) if replaced[a] else -(lam[a] * flow[a] * num(float(m.yin[i]))) / tof0)
                       for a, i in enumerate(dyn) if flow[a] != 0}
    out['dir'] = [sum((s[j] * (rf[j] * num(float(a[j])) - rr[j] * num(float(c[j]))) for j in range(R)), num(0)) / tof0
                  for a, c in directions]
    big = max(max(abs(v) for v in rf), max(abs(v) for v in rr))
    out['ratio'] = big / abs(tof0)
    return out


def adjoint_sens_mp(m, y_full, tof_terms, bits, kf=None, kr=None, directions=()):
    """adjoint_sens in mpmath at `bits` of working precision (mpf values)"""
    import mpmath
    with mpmath.workprec(bits):
        return adjoint_sens(m, y_full, tof_terms, mpmath.mpf, kf, kr, directions)


def flat(out):
    """The outputs of adjoint_sens as float arrays: sf, sr, order (sorted by
    name), order_in (sorted by name), dir, xi, and the names"""
    f = lambda xs: np.array([float(x) for x in xs], float)
    on, oin = sorted(out['order']), sorted(out['order_in'])
    return dict(sf=f(out['sf']), sr=f(out['sr']), xi=f(out['xi']), order=f([out['order'][k] for k in on]),
                order_names=np.array(on, dtype=str), order_in=f([out['order_in'][k] for k in oin]),
                order_in_names=np.array(oin, dtype=str), dir=f(out['dir']), tof=float(out['tof0']),
                err=float(out['ratio']) * 2.0 ** ERR_UNIT_LOG2)


def stencil_dlnk(k_at, T, h_rel=1.0e-3):
    """(d ln kf / dT, d ln kr / dT) by the 5-point central stencil of k_at(T') ->
    (kf, kr) at h = h_rel T; 0 where a rate constant is 0"""
    h = h_rel * T
    acc = [0.0, 0.0]
    live = [None, None]
    for mlt, wgt in ((-2.0, 1.0), (-1.0, -8.0), (1.0, 8.0), (2.0, -1.0)):
        k = k_at(T + mlt * h)
        for q in (0, 1):
            kq = np.asarray(k[q], float)
            live[q] = kq > 0.0
            acc[q] = acc[q] + wgt * np.log(np.where(live[q], kq, 1.0))
    return tuple(np.where(live[q], acc[q] / (12.0 * h), 0.0) for q in (0, 1))
