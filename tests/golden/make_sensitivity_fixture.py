"""Fixture of the adjoint sensitivities (pck_sens_at / pck_sens_adjoint,
csrc/mk_sens.h: k_sens_adjoint): the formulas of tests/_sens_ext.py in mpmath at
the steady states and rate constants of drc_adjoint_fixture.npz.  CPU only; the
GPU tests read the .npz alone.

For every `regular` case of drc_adjoint_fixture.npz, `c<i>_...` with the same
index i and name (`names[i]`; the models are built as make_drc_adjoint_fixture.py
builds them, without its solves):
  rnames                       reactions (the order of every per-reaction vector)
  sf_ref, sr_ref, xi_ref       _sens_ext.adjoint_sens at 400 bits (asserted equal
                               to an 800-bit run to 1e-60), rounded
  order_ref, order_names       reaction orders in the fixed species
  order_in_ref, order_in_names ... in the inflow of the CSTR's gas species
  dir_a, dir_c, dir_ref        one fixed random direction (d ln kf, d ln kr) and
                               its sensitivity
  tof_ref, err                 the TOF and the guard's bound 2^-98 max rate / |TOF|
  *_104                        the same outputs at 104 bits (double-double)
  *_pert                       ... at 400 bits at y (1 +- 1e-6), a fixed random sign
                               per species: what the solve's parity bound allows
and, for the DMTM and the regular volcano cases with |TOF| > 1e-20:
  a, c                         d ln kf / dT, d ln kr / dT: the 5-point stencil of
                               the oracle's rate constants at h = 1e-3 T
  eapp_ref                     R T^2 x their direction's sensitivity (J/mol)
  eapp_2h, eapp_pert           with the stencil step doubled; at the moved root
  eapp_fd                      R T^2 x the central difference of ln TOF of the
                               oracle's own steady solves at T +- 0.5 K
The guard's constant is asserted here: |out_104 - out_ref| <= err + 2^-52 |out_ref|
for every output of every case, both sides in mpmath before rounding.  The
second term is one ulp of the double the kernel returns: without it four
of the synthetic cases miss (syn12_0, syn12_2, syn24_0, syn24_1; the worst
syn24_1 with 4.5e-20 against err 6.7e-23), by the conditioning of the linear
solve at 104 bits, four orders and more below the rounding of the result; an
exponent raised to cover them (2^-88) would flag volcano_0.5_0.5 at the
default err_max of 1e-9.

    OMP_NUM_THREADS=1 python tests/golden/make_sensitivity_fixture.py

writes tests/golden/sensitivity_fixture.npz (numpy arrays only).
"""
import copy
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
INPUTS = os.path.join(HERE, 'inputs')
SRC = os.path.join(HERE, 'drc_adjoint_fixture.npz')
OUT = os.path.join(HERE, 'sensitivity_fixture.npz')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, HERE)

BITS, BITS_CHECK = 400, 800
PERT = 1.0e-6
SEED = 20261020
DT_FD = 0.5
TOF_MIN_EAPP = 1.0e-20
RGAS = 8.31446262           # J/(K mol), the product's constant
ULP = 2.0 ** -52
KEYS = ('sf', 'sr', 'xi', 'order', 'order_in', 'dir')


def model(name, c):
    """(oracle model, k_at(T) -> (kf, kr) or None, steady_tof(T) or None) of a case of drc_adjoint_fixture.npz"""
    from oracle import mk_oracle as O
    from _synth import spec_of
    key = name.split('_')[0]
    T, p = float(c['T']), float(c['p'])
    if key == 'dmtm':
        spec = O.load_spec(os.path.join(INPUTS, 'DMTM', 'input.json'))

        def k_at(t):
            k = O.rate_constants(spec, t, p)
            return [k[r][0] for r in spec['reactions']], [k[r][1] for r in spec['reactions']]

        def steady_tof(t):
            m = O.ClassicModel(spec, T=t, p=p)
            y, _ = m.solve_odes(rtol=1e-6, atol=1e-12, method='BDF')
            y = m.find_steady(y)          # (at 400 K its rule may report the transient end: root noise)
            return m.tof(y, [str(x) for x in c['tof_terms']])
        return O.ClassicModel(spec, T=T, p=p), k_at, steady_tof
    if key == 'cstr':
        spec = O.load_spec(os.path.join(INPUTS, 'COOxReactor', 'input_Pd111.json'))
        return O.ClassicModel(spec, T=T), None, None
    if key == 'volcano':
        base = O.load_spec(os.path.join(INPUTS, 'COOxVolcano', 'input.json'))
        eco, eo = (float(c['desc'][list(c['desc_names']).index(k)]) for k in ('ECO', 'EO'))

        def at(t):
            spec = copy.deepcopy(base)
            O.set_volcano_point(spec, eco, eo, t)
            return spec

        def k_at(t):
            spec = at(t)
            k = O.rate_constants(spec, t, spec['system']['p'])
            return [k[r][0] for r in spec['reactions']], [k[r][1] for r in spec['reactions']]

        def steady_tof(t):
            r = O.volcano_steady(base, eco, eo, T=t)
            assert r['regular']
            return r['tof']
        return O.ClassicModel(at(T), T=T), k_at, steady_tof
    desc = np.array([float(c['desc'][list(c['desc_names']).index('D%d' % q)]) for q in range(4)]) \
        if len(c['desc_names']) else None
    if key in ('syn12', 'syn24', 'syn40'):
        from make_synthetic_sizes_fixture import NETS, SEED_NET
        from pycatkin_amd.functions.synthetic import synthetic_network
        ns, nr = NETS[key]
        net = synthetic_network(n_species=ns, n_reactions=nr, seed=SEED_NET)
        return O.ClassicModel(spec_of(net, desc, T), T=T), None, None
    if key == 'e64':
        from make_edge_sizes_fixture import edge_net
        return O.ClassicModel(spec_of(edge_net('e64'), desc, T), T=T), None, None
    if key == 'butadiene':
        from make_butadiene_fixture import CASES, kept_reactions
        case = name[len('butadiene_'):name.rindex('_')]
        base = O.load_spec(os.path.join(INPUTS, 'Butadiene', 'input.json'))
        mkm = O.load_spec(os.path.join(INPUTS, 'Butadiene', 'input_mkm.json'), base_spec=base)
        sp = copy.copy(mkm)
        sp['reactions'] = {r: mkm['reactions'][r] for r in kept_reactions(list(mkm['reactions']), case, dict(CASES)[case])}
        return O.ClassicModel(sp, T=T), None, None
    raise KeyError(name)


def main():
    import mpmath
    import _sens_ext as S
    fx = dict(np.load(SRC))
    names = [str(x) for x in fx['names']]
    rng = np.random.default_rng(SEED)
    out, t0 = {'names': np.array(names)}, time.time()
    regular, worst = [], 0.0
    for i, name in enumerate(names):
        pre = 'c%d_' % i
        c = {k[len(pre):]: v for k, v in fx.items() if k.startswith(pre)}
        if not bool(c['regular']):
            continue
        regular.append(i)
        m, k_at, steady_tof = model(name, c)
        assert list(m.rnames) == [str(x) for x in c['rnames']] and [m.snames[q] for q in m.dyn] == [str(x) for x in c['dyn']]
        assert np.array_equal(m.kf, c['kf']) and np.array_equal(m.kr, c['kr']), name
        assert np.array_equal(np.array(m.unreach[list(m.dyn)], bool), c['unreach']), name
        y, tof_terms = c['y_full'], [str(x) for x in c['tof_terms']]
        T, R = float(c['T']), len(m.rnames)
        dirs = [(rng.uniform(-1.0, 1.0, R), rng.uniform(-1.0, 1.0, R))]
        sign = rng.choice([-1.0, 1.0], len(m.dyn))
        eapp = k_at is not None and abs(float(c['tof_ref'])) > TOF_MIN_EAPP
        if eapp:
            dirs.append(S.stencil_dlnk(k_at, T))
            assert np.array_equal(np.asarray(k_at(T)[0]), m.kf) and np.array_equal(np.asarray(k_at(T)[1]), m.kr), name
            dirs.append(S.stencil_dlnk(k_at, T, 2.0e-3))
        r4 = S.adjoint_sens_mp(m, y, tof_terms, BITS, directions=dirs)
        r8 = S.adjoint_sens_mp(m, y, tof_terms, BITS_CHECK, directions=dirs)
        with mpmath.workprec(BITS_CHECK):
            tiny = mpmath.mpf(10) ** -60
            for key in KEYS:
                a4 = list(r4[key].values()) if isinstance(r4[key], dict) else r4[key]
                a8 = list(r8[key].values()) if isinstance(r8[key], dict) else r8[key]
                big = max([abs(x) for x in a8] + [mpmath.mpf(1)])
                assert all(abs(a - b) <= tiny * (abs(b) + big) for a, b in zip(a4, a8)), (name, key)
        ref = S.flat(r4)
        r1 = S.adjoint_sens_mp(m, y, tof_terms, 104, directions=dirs)
        lo = S.flat(r1)
        yp = np.array(y)
        yp[list(m.dyn)] = yp[list(m.dyn)] * (1.0 + PERT * sign)
        pt = S.flat(S.adjoint_sens_mp(m, yp, tof_terms, BITS, directions=dirs))
        o = dict(rnames=np.array(m.rnames), order_names=ref['order_names'], order_in_names=ref['order_in_names'],
                 tof_ref=np.array(ref['tof']), err=np.array(ref['err']), dir_a=dirs[0][0], dir_c=dirs[0][1])
        d104 = over = 0.0
        for key in KEYS:
            o[key + '_ref'], o[key + '_104'], o[key + '_pert'] = ref[key], lo[key], pt[key]
            if key == 'dir':
                o['dir_ref'], o['dir_104'], o['dir_pert'] = ref[key][:1], lo[key][:1], pt[key][:1]
            with mpmath.workprec(BITS):           # before either is rounded to a float
                a1 = list(r1[key].values()) if isinstance(r1[key], dict) else r1[key]
                a4 = list(r4[key].values()) if isinstance(r4[key], dict) else r4[key]
                d104 = max([d104] + [float(abs(a - b)) for a, b in zip(a1, a4)])
                over = max([over] + [float(abs(a - b) - ULP * abs(b)) for a, b in zip(a1, a4)])
        # the guard's constant: the 104-bit run is within err of the answer, every case,
        # beyond one ulp of the double an output is returned in (see the docstring)
        assert over <= ref['err'], (name, d104, over, ref['err'])
        worst = max(worst, d104 / ref['err'])
        if eapp:
            f = RGAS * T * T
            o.update(a=dirs[1][0], c=dirs[1][1], eapp_ref=np.array(f * ref['dir'][1]), eapp_104=np.array(f * lo['dir'][1]),
                     eapp_2h=np.array(f * ref['dir'][2]), eapp_pert=np.array(f * pt['dir'][1]))
            o['eapp_fd'] = np.array(f * (np.log(steady_tof(T + DT_FD)) - np.log(steady_tof(T - DT_FD))) / (2.0 * DT_FD))
        for k, v in o.items():
            out[pre + k] = v
        print('%-40s err %.1e  |104 - ref| %.2e  orders %s%s  (%.0f s)'
              % (name, ref['err'], d104, ' '.join('%s %.6f' % (a, b) for a, b in zip(ref['order_names'], ref['order'])),
                 ('  Eapp %.6f kJ/mol (2h %.1e, pert %.1e, fd %.1e rel)'
                  % (o['eapp_ref'] / 1e3, abs(o['eapp_2h'] / o['eapp_ref'] - 1), abs(o['eapp_pert'] / o['eapp_ref'] - 1),
                     abs(o['eapp_fd'] / o['eapp_ref'] - 1))) if eapp else '', time.time() - t0), flush=True)
    out['regular'] = np.array(regular)
    np.savez_compressed(OUT, **out)
    print('wrote %s (%d cases, worst |104 - ref| / err %.2e, %.0f s)' % (OUT, len(regular), worst, time.time() - t0))


if __name__ == '__main__':
    main()
