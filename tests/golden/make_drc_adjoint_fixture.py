"""Fixture of the analytic degree of rate control (pck_drc_at /
pck_drc_adjoint, csrc/mk_sens.h): steady states of the oracle's models and the
adjoint formula of tests/_sens.py evaluated at them in mpmath.  CPU only; the
GPU tests read the .npz alone.

Per case `c<i>_...` (name in `names[i]`):
  T, p, desc_names / desc     the condition
  tof_terms, dyn, rnames      TOF terms, dynamic species and reactions by name
                              (the oracle's order: every vector below is in it)
  regular                     the oracle's steady rule reports a reached root
  y, y_full                   that root over `dyn` / over every species (the
                              transient end where not regular)
  unreach, dead               dynamic species no reaction can produce
                              (ClassicModel.unreach); reactions whose forward
                              and reverse rates are both exactly 0 at y
  kf, kr                      the oracle's rate constants
  xi_ref, tof_ref             _sens.adjoint_drc at 400 bits (asserted here to
                              agree with an 800-bit run to 1e-60), rounded
  xi_104                      the same algorithm at 104 bits
  xi_pert                     xi_ref recomputed at y (1 +- 1e-6) (a fixed random
                              sign per species): the change the solve's own
                              parity bound on the states allows
  xi_fd                       ClassicModel.drc(eps=1e-3, steady=True) where it
                              finishes in reasonable time, else NaN
NaN where a case is not regular.

    OMP_NUM_THREADS=1 python tests/golden/make_drc_adjoint_fixture.py

writes tests/golden/drc_adjoint_fixture.npz (numpy arrays only).
"""
import copy
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
INPUTS = os.path.join(HERE, 'inputs')
OUT = os.path.join(HERE, 'drc_adjoint_fixture.npz')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, HERE)

BITS, BITS_CHECK = 400, 800
PERT = 1.0e-6               # the parity bound the steady solve is held to (relative, on every state)
EPS_FD = 1.0e-3

DMTM = [(400.0, 1e4), (450.0, 1e4), (600.0, 1e5), (800.0, 1e6)]
CSTR_T = [473.0, 523.0, 573.0]
VOLCANO = [(-1.0, -1.0), (-1.3, -1.1), (0.5, 0.5), (-2.5, 0.5), (-2.5, -2.5), (0.5, -2.5)]
VOLCANO_T = 600.0
SYN_KEYS = ('syn12', 'syn24', 'syn40')
BUTADIENE_CASE = 'with_jonas_byproducts'


def _root(m, method='BDF'):
    """ClassicModel.drc's own steady state"""
    y, _ = m.solve_odes(rtol=1e-6, atol=1e-12, method=method)
    y = m.find_steady(y)
    return y, bool(m.regular)


def cases():
    """name, model, full state, regular, tof terms, T, p, descriptors, finite differences wanted"""
    from oracle import mk_oracle as O
    from _synth import spec_of
    spec = O.load_spec(os.path.join(INPUTS, 'DMTM', 'input.json'))
    for T, p in DMTM:
        m = O.ClassicModel(spec, T=T, p=p)
        y, reg = _root(m)
        yield 'dmtm_%g_%g' % (T, p), m, y, reg, ['r5', 'r9'], T, p, {}, True
    spec = O.load_spec(os.path.join(INPUTS, 'COOxReactor', 'input_Pd111.json'))
    for T in CSTR_T:
        m = O.ClassicModel(spec, T=T)
        y, reg = _root(m, 'LSODA')
        yield 'cstr_%g' % T, m, y, reg, ['CO_ox'], T, m.p, {}, False      # (its FD takes minutes)
    spec = O.load_spec(os.path.join(INPUTS, 'COOxVolcano', 'input.json'))
    for eco, eo in VOLCANO:
        r = O.volcano_steady(spec, eco, eo, T=VOLCANO_T)
        m = r['model']
        yield 'volcano_%g_%g' % (eco, eo), m, r['y'], bool(r['regular']), ['CO_ox'], VOLCANO_T, m.p, \
            dict(ECO=eco, EO=eo), bool(r['regular'])
    from make_synthetic_sizes_fixture import NETS, SEED_NET, T as T_SYN
    from pycatkin_amd.functions.synthetic import synthetic_network
    sfx = dict(np.load(os.path.join(HERE, 'synthetic_sizes_fixture.npz')))
    for key in SYN_KEYS:
        ns, nr = NETS[key]
        net = synthetic_network(n_species=ns, n_reactions=nr, seed=SEED_NET)
        rows = [k for k in range(sfx['desc'].shape[0]) if sfx[key + '_ok'][k] and sfx[key + '_regular'][k]][:2]
        for k in rows:
            m = O.ClassicModel(spec_of(net, sfx['desc'][k], float(T_SYN)), T=float(T_SYN))
            assert [m.snames[i] for i in m.dyn] == [str(x) for x in sfx[key + '_dyn']]
            y = m.y0.copy()
            y[m.dyn] = sfx[key + '_y'][k]
            yield '%s_%d' % (key, k), m, y, True, ['R0'], float(T_SYN), m.p, \
                {'D%d' % q: float(sfx['desc'][k, q]) for q in range(4)}, False
    from make_edge_sizes_fixture import T as T_EDGE, TOF_TERM, edge_net
    efx = dict(np.load(os.path.join(HERE, 'edge_sizes_fixture.npz')))
    k = int(np.nonzero(efx['e64_regular'])[0][0])
    m = O.ClassicModel(spec_of(edge_net('e64'), efx['desc'][k], T_EDGE), T=T_EDGE)
    assert [m.snames[i] for i in m.dyn] == [str(x) for x in efx['e64_dyn']]
    y = m.y0.copy()
    y[m.dyn] = efx['e64_y'][k]
    yield 'e64_%d' % k, m, y, True, [TOF_TERM['e64']], T_EDGE, m.p, \
        {'D%d' % q: float(efx['desc'][k, q]) for q in range(4)}, False
    from make_butadiene_fixture import BD_TERMS, CASES, TEMPS, kept_reactions
    bfx = dict(np.load(os.path.join(HERE, 'butadiene_fixture.npz')))
    base = O.load_spec(os.path.join(INPUTS, 'Butadiene', 'input.json'))
    mkm = O.load_spec(os.path.join(INPUTS, 'Butadiene', 'input_mkm.json'), base_spec=base)
    sp = copy.copy(mkm)
    sp['reactions'] = {r: mkm['reactions'][r]
                       for r in kept_reactions(list(mkm['reactions']), BUTADIENE_CASE, dict(CASES)[BUTADIENE_CASE])}
    ti = int(np.nonzero(bfx['regular_' + BUTADIENE_CASE] & bfx['ok_' + BUTADIENE_CASE])[0][0])
    m = O.ClassicModel(sp, T=float(TEMPS[ti]))
    assert [m.snames[i] for i in m.dyn] == [str(x) for x in bfx['dyn_' + BUTADIENE_CASE]]
    y = m.y0.copy()
    y[m.dyn] = bfx['y_rule_' + BUTADIENE_CASE][ti]
    assert m.unreach[m.dyn].any()           # the case is here for its pinned species
    yield 'butadiene_%s_%g' % (BUTADIENE_CASE, TEMPS[ti]), m, y, True, list(BD_TERMS), float(TEMPS[ti]), m.p, {}, False


def main():
    import mpmath
    import _sens as S
    out, names = {}, []
    rng = np.random.default_rng(20261019)
    t0 = time.time()
    for i, (name, m, y, reg, tof_terms, T, p, desc, fd) in enumerate(cases()):
        pre = 'c%d_' % i
        names.append(name)
        R, dyn = len(m.rnames), list(m.dyn)
        nan = np.full(R, np.nan)
        o = dict(T=np.array(float(T)), p=np.array(float(p)), desc_names=np.array(sorted(desc)),
                 desc=np.array([desc[k] for k in sorted(desc)], float), tof_terms=np.array(tof_terms),
                 dyn=np.array([m.snames[q] for q in dyn]), rnames=np.array(m.rnames), regular=np.array(bool(reg)),
                 y=np.array(y)[dyn], y_full=np.array(y), kf=m.kf.copy(), kr=m.kr.copy(),
                 unreach=np.array(m.unreach[dyn], bool), dead=np.all(m.rates(y) == 0.0, axis=1),
                 xi_ref=nan, xi_104=nan, xi_pert=nan, xi_fd=nan, tof_ref=np.array(m.tof(y, tof_terms)))
        if reg:
            xi4, tof4 = S.adjoint_drc_mp(m, y, tof_terms, BITS)
            xi8, _ = S.adjoint_drc_mp(m, y, tof_terms, BITS_CHECK)
            with mpmath.workprec(BITS_CHECK):
                big = max(abs(x) for x in xi8)
                assert all(abs(a - b) <= mpmath.mpf(10) ** -60 * (abs(b) + mpmath.mpf(10) ** -60 * big)
                           for a, b in zip(xi4, xi8)), name
            o['xi_ref'] = np.array([float(x) for x in xi4])
            o['tof_ref'] = np.array(float(tof4))
            o['xi_104'] = np.array([float(x) for x in S.adjoint_drc_mp(m, y, tof_terms, 104)[0]])
            yp = np.array(y)
            yp[dyn] = yp[dyn] * (1.0 + PERT * rng.choice([-1.0, 1.0], len(dyn)))
            o['xi_pert'] = np.array([float(x) for x in S.adjoint_drc_mp(m, yp, tof_terms, BITS)[0]])
            if fd:
                xf = m.drc(tof_terms, eps=EPS_FD, steady=True)
                o['xi_fd'] = np.array([xf[rn] for rn in m.rnames])
        for k, v in o.items():
            out[pre + k] = v
        print('%-44s regular %d  sum xi %.12f  |104 - ref| %.1e  |pert - ref| %.1e  |fd - ref| %.1e  (%.0f s)'
              % (name, reg, np.nansum(o['xi_ref']), np.nanmax(np.abs(o['xi_104'] - o['xi_ref'])) if reg else 0,
                 np.nanmax(np.abs(o['xi_pert'] - o['xi_ref'])) if reg else 0,
                 np.nanmax(np.abs(o['xi_fd'] - o['xi_ref'])) if (reg and fd) else 0, time.time() - t0), flush=True)
    out['names'] = np.array(names)
    np.savez_compressed(OUT, **out)
    print('wrote %s (%d cases, %.0f s)' % (OUT, len(names), time.time() - t0))


if __name__ == '__main__':
    main()
