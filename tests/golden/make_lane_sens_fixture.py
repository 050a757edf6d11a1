"""Fixture of the one-lane adjoint kernels (csrc/mk_sens_lane.h) and of the
descriptor sensitivities (System.descriptor_sensitivity_at / _batch): the
formulas of tests/_sens_ext.py in mpmath, as make_sensitivity_fixture.py runs
them.  CPU only; the GPU tests read the .npz alone.

The volcano (NS 4) and CSTR (NS 6) cases of drc_adjoint_fixture.npz /
sensitivity_fixture.npz are the one-lane kernels' references as they stand.
This fixture adds

(a) `n<k>_...`, names[k] = l3_0, l3_1, l7_0, l7_1, l8_0, l8_1: the networks
    tests/_synth.edge_network of NETS below at NS = 3, 7 and 8 (8 is the
    kernels' limit; l8 is e8a of make_edge_sizes_fixture.py, its roots read from
    edge_sizes_fixture.npz), two conditions each at the oracle's roots
    (mk_oracle.steady_rule as make_edge_sizes_fixture.py calls it).  Every
    species row of these networks has several CSR entries (3 species in 8
    reactions, 7 in 21, 8 in 28).  The TOF term of l3 / l7 is the reaction with
    the largest net rate among those whose net rate is at least 0.1 (|rf| +
    |rr|) at both roots.
(b) `n<k>_...`, names[k] = pin_0: one hand-made state of the chain-only edge
    network PIN (5 species, 5 reactions: no random step, so the last adsorbate
    of a chain is a leaf with one reaction).  The leaf and its chain parent
    are set to exactly 0: the leaf has y = 0 and an exactly zero rate, which is
    the kernels' pinned row (a unit row); the reference gets it through
    `unreach`, set by hand here.  The formulas are linear algebra at the given
    state: it need not be steady, and it is not.
    Fields of (a) and (b): those of a case of drc_adjoint_fixture.npz (T, p,
    desc_names, desc, tof_terms, dyn, rnames, y, y_full, kf, kr, unreach) and
    of sensitivity_fixture.npz (sf / sr / xi / order / order_in / dir _ref,
    _104 and _pert, order_names, order_in_names, dir_a, dir_c, tof_ref, err),
    plus `net`, the key of NETS.
(c) `d<k>_...`, dnames[k]: three regular volcano nodes -- volcano_-1_-1 and
    volcano_-1.3_-1.1 of sensitivity_fixture.npz (its regular Eapp cases; the
    third, volcano_0.5_0.5, is replaced by the node VOLCANO_NODE below, see
    there) -- with the fields of a case of drc_adjoint_fixture.npz and:
      ddesc_names            ECO, EO
      ddesc_a, ddesc_c       [2, R] d ln kf / d desc, d ln kr / d desc: 5-point
                             stencils of the oracle's rate constants at h =
                             1e-3 eV
      ddesc_ref, _104, _pert [2] d ln TOF / d desc (1/eV): their directions'
                             sensitivities at 400 bits, at 104 bits, and at 400
                             bits at y (1 +- 1e-6)
      ddesc_2h               with the stencil step doubled
      ddesc_fd               the central difference of ln TOF of the oracle's
                             own steady solves at desc +- 1e-3 eV
    Asserted: |ddesc_2h - ddesc_ref| <= 1e-9 |ddesc_ref| for every stored case,
    so none straddles an energy clamp (max(dGa, 0)).

Every 400-bit run is asserted equal to an 800-bit run to 1e-60, and the guard's
constant holds as in make_sensitivity_fixture.py.

    OMP_NUM_THREADS=1 python tests/golden/make_lane_sens_fixture.py

writes tests/golden/lane_sens_fixture.npz (numpy arrays only).
"""
import copy
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
INPUTS = os.path.join(HERE, 'inputs')
OUT = os.path.join(HERE, 'lane_sens_fixture.npz')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, HERE)

BITS, BITS_CHECK = 400, 800
PERT = 1.0e-6
SEED = 20261021
ULP = 2.0 ** -52
KEYS = ('sf', 'sr', 'xi', 'order', 'order_in', 'dir')
H_DESC = 1.0e-3             # eV, System.dlnk_ddesc_batch's default step
DESC = ('ECO', 'EO')
CLAMP_TOL = 1.0e-9

# key: (species, reactions, seed of edge_network); l8 is make_edge_sizes_fixture's e8a
NETS = {'l3': (3, 8, 3), 'l7': (7, 21, 5), 'l8': (8, 28, 1), 'pin': (5, 5, 2)}
T = 500.0
T_END = 1.0e8
N_TRY = 8                   # descriptor vectors tried for two regular roots
MIN_TOF_RATIO = 0.1


def lane_net(key):
    """The plain-data network of a key of NETS."""
    from _synth import edge_network
    ns, nr, seed = NETS[key]
    return edge_network(ns, nr, seed)


def pinned_pair(net):
    """(leaf, parent): the last adsorbate of PIN whose only reaction is its
    chain step parent <-> leaf."""
    ads = net['adsorbates']
    for leaf in reversed(ads):
        its = [(kind, reac, prod) for kind, reac, prod in net['reactions'] if leaf in reac or leaf in prod]
        if len(its) == 1 and its[0][0] == 'surf' and len(its[0][1]) == 1 and its[0][2] == [leaf]:
            return leaf, its[0][1][0]
    raise AssertionError('no leaf adsorbate')


def _descriptors():
    return np.random.default_rng(SEED).uniform(-0.5, 0.5, (N_TRY, 4))


def _roots(key):
    """Two (descriptor vector, model, full state) at the oracle's roots, and the TOF term."""
    from _synth import spec_of
    from oracle import mk_oracle as O
    from make_edge_sizes_fixture import ROOT_DIST, STEADY_ATOL
    net = lane_net(key)
    if key == 'l8':
        from make_edge_sizes_fixture import NETS as ENETS, TOF_TERM
        assert ENETS['e8a'] == NETS['l8']
        efx = dict(np.load(os.path.join(HERE, 'edge_sizes_fixture.npz')))
        assert float(efx['T']) == T
        out = []
        for k in np.nonzero(efx['e8a_regular'])[0][:2]:
            m = O.ClassicModel(spec_of(net, efx['desc'][k], T), T=T)
            assert [m.snames[i] for i in m.dyn] == [str(x) for x in efx['e8a_dyn']]
            y = m.y0.copy()
            y[m.dyn] = efx['e8a_y'][k]
            out.append((efx['desc'][k], m, y))
        return out, TOF_TERM['e8a']
    out = []
    for d in _descriptors():
        m = O.ClassicModel(spec_of(net, d, T), T=T)
        m._set_reach(m.y0)
        r = O.steady_rule(m, dist=ROOT_DIST, dist_atol=STEADY_ATOL, budget=400000, t_end=T_END)
        if r is not None and r['regular']:
            out.append((d, m, r['y']))
        if len(out) == 2:
            break
    assert len(out) == 2, key
    best, term = 0.0, None
    for j, rn in enumerate(out[0][1].rnames):
        rates = [m.rates(y)[j] for _, m, y in out]
        if all(abs(r[0] - r[1]) >= MIN_TOF_RATIO * (abs(r[0]) + abs(r[1])) for r in rates):
            v = min(abs(r[0] - r[1]) for r in rates)
            if v > best:
                best, term = v, rn
    assert term is not None, key
    return out, term


def _pinned():
    """The hand-made state of PIN: coverages 0.3 / 0.2 / ... on the other
    species, the leaf and its parent exactly 0."""
    from _synth import spec_of
    from oracle import mk_oracle as O
    net = lane_net('pin')
    leaf, parent = pinned_pair(net)
    d = _descriptors()[0]
    m = O.ClassicModel(spec_of(net, d, T), T=T)
    y = m.y0.copy()
    vals = iter((0.3, 0.2, 0.15, 0.1, 0.05, 0.04, 0.03))
    for i in m.dyn:
        y[i] = 0.0 if m.snames[i] in (leaf, parent) else next(vals)
    unreach = np.zeros(len(m.snames), bool)
    unreach[m.snames.index(leaf)] = True
    m.unreach = unreach                   # by hand: the kernels find the row by y = 0 and a zero rate
    j = [q for q, rn in enumerate(m.rnames) if m.W[m.snames.index(leaf), q] != 0.0]
    assert len(j) == 1 and np.all(m.rates(y)[j[0]] == 0.0)
    assert m.rhs(y)[m.snames.index(parent)] != 0.0           # the parent is at 0 but not pinned
    return [(d, m, y)], 'R0'


def _check_800(name, r4, r8):
    import mpmath
    with mpmath.workprec(BITS_CHECK):
        tiny = mpmath.mpf(10) ** -60
        for key in KEYS:
            a4 = list(r4[key].values()) if isinstance(r4[key], dict) else r4[key]
            a8 = list(r8[key].values()) if isinstance(r8[key], dict) else r8[key]
            big = max([abs(x) for x in a8] + [mpmath.mpf(1)])
            assert all(abs(a - b) <= tiny * (abs(b) + big) for a, b in zip(a4, a8)), (name, key)


def _runs(name, m, y, tof_terms, dirs, sign):
    """(ref, 104-bit, perturbed) flat outputs of _sens_ext.adjoint_sens; the
    800-bit check and the guard's constant asserted."""
    import mpmath
    import _sens_ext as S
    r4 = S.adjoint_sens_mp(m, y, tof_terms, BITS, directions=dirs)
    _check_800(name, r4, S.adjoint_sens_mp(m, y, tof_terms, BITS_CHECK, directions=dirs))
    r1 = S.adjoint_sens_mp(m, y, tof_terms, 104, directions=dirs)
    ref, lo = S.flat(r4), S.flat(r1)
    yp = np.array(y)
    yp[list(m.dyn)] = yp[list(m.dyn)] * (1.0 + PERT * sign)
    pt = S.flat(S.adjoint_sens_mp(m, yp, tof_terms, BITS, directions=dirs))
    d104 = over = 0.0
    for key in KEYS:
        with mpmath.workprec(BITS):
            a1 = list(r1[key].values()) if isinstance(r1[key], dict) else r1[key]
            a4 = list(r4[key].values()) if isinstance(r4[key], dict) else r4[key]
            d104 = max([d104] + [float(abs(a - b)) for a, b in zip(a1, a4)])
            over = max([over] + [float(abs(a - b) - ULP * abs(b)) for a, b in zip(a1, a4)])
    assert over <= ref['err'], (name, d104, over, ref['err'])
    return ref, lo, pt, d104


def stencil_desc(k_at, x, h):
    """(d ln kf / dx, d ln kr / dx) by the 5-point central stencil of k_at(x') ->
    (kf, kr) at the absolute step h; 0 where a rate constant is 0
    (_sens_ext.stencil_dlnk with an absolute step)."""
    acc = [0.0, 0.0]
    live = [None, None]
    for mlt, wgt in ((-2.0, 1.0), (-1.0, -8.0), (1.0, 8.0), (2.0, -1.0)):
        k = k_at(x + mlt * h)
        for q in (0, 1):
            kq = np.asarray(k[q], float)
            live[q] = kq > 0.0
            acc[q] = acc[q] + wgt * np.log(np.where(live[q], kq, 1.0))
    return tuple(np.where(live[q], acc[q] / (12.0 * h), 0.0) for q in (0, 1))


def new_cases(out, rng, t0):
    names = []
    for key in ('l3', 'l7', 'l8', 'pin'):
        rows, term = _pinned() if key == 'pin' else _roots(key)
        for q, (d, m, y) in enumerate(rows):
            name, pre = '%s_%d' % (key, q), 'n%d_' % len(names)
            names.append(name)
            dyn, R = list(m.dyn), len(m.rnames)
            dirs = [(rng.uniform(-1.0, 1.0, R), rng.uniform(-1.0, 1.0, R))]
            sign = rng.choice([-1.0, 1.0], len(dyn))
            ref, lo, pt, d104 = _runs(name, m, y, [term], dirs, sign)
            desc = {'D%d' % k: float(d[k]) for k in range(4)}
            o = dict(net=np.array(key), T=np.array(T), p=np.array(float(m.p)), desc_names=np.array(sorted(desc)),
                     desc=np.array([desc[k] for k in sorted(desc)], float), tof_terms=np.array([term]),
                     dyn=np.array([m.snames[i] for i in dyn]), rnames=np.array(m.rnames), y=np.array(y)[dyn],
                     y_full=np.array(y), kf=m.kf.copy(), kr=m.kr.copy(), unreach=np.array(m.unreach[dyn], bool),
                     order_names=ref['order_names'], order_in_names=ref['order_in_names'], tof_ref=np.array(ref['tof']),
                     err=np.array(ref['err']), dir_a=dirs[0][0], dir_c=dirs[0][1])
            for k2 in KEYS:
                o[k2 + '_ref'], o[k2 + '_104'], o[k2 + '_pert'] = ref[k2], lo[k2], pt[k2]
            for k2, v in o.items():
                out[pre + k2] = v
            print('%-10s NS %d R %d  TOF %s %.3e  err %.1e  |104 - ref| %.2e  pinned %d  (%.0f s)'
                  % (name, len(dyn), R, term, ref['tof'], ref['err'], d104, int(o['unreach'].sum()), time.time() - t0),
                  flush=True)
    out['names'] = np.array(names)


# volcano_0.5_0.5, the third regular Eapp case of sensitivity_fixture.npz, is not
# stored: there d ln TOF / d E_CO is 7.7e-9 / eV next to d ln TOF / d E_O = -26.9,
# a cancellation to 1e-10 of its terms, and the two stencil steps differ by 2.4e-6
# of it -- above the 1e-9 the generator holds every stored case to (no clamp
# switches there; the number is too small for a relative bound).  The node below
# takes its place, on the same ridge as the other two.
VOLCANO_SKIPPED = 'volcano_0.5_0.5'
VOLCANO_NODE = (-0.7, -0.9)


def volcano_cases(out, rng, t0):
    """`d<k>_...`, dnames[k]: the condition, state and rate constants (the
    fields of a case of drc_adjoint_fixture.npz) and the ddesc_* references."""
    from oracle import mk_oracle as O
    sx = dict(np.load(os.path.join(HERE, 'sensitivity_fixture.npz')))
    fx = dict(np.load(os.path.join(HERE, 'drc_adjoint_fixture.npz')))
    names = [str(x) for x in fx['names']]
    base = O.load_spec(os.path.join(INPUTS, 'COOxVolcano', 'input.json'))
    ids = [i for i in sx['regular'] if names[i].startswith('volcano_') and 'c%d_eapp_ref' % i in sx]
    assert len(ids) == 3 and VOLCANO_SKIPPED in [names[i] for i in ids]
    todo = []
    for i in ids:
        if names[i] == VOLCANO_SKIPPED:
            continue
        pre = 'c%d_' % i
        c = {k[len(pre):]: v for k, v in fx.items() if k.startswith(pre)}
        todo.append((names[i], float(c['T']), {k: float(c['desc'][list(c['desc_names']).index(k)]) for k in DESC},
                     c['y_full'], c))
    Tn = todo[0][1]
    r = O.volcano_steady(base, VOLCANO_NODE[0], VOLCANO_NODE[1], T=Tn)
    assert r['regular']
    todo.append(('volcano_%g_%g' % VOLCANO_NODE, Tn, dict(ECO=VOLCANO_NODE[0], EO=VOLCANO_NODE[1]), r['y'], None))
    dnames = []
    for name, Tv, x0, y_full, c in todo:
        pre = 'd%d_' % len(dnames)
        dnames.append(name)

        def at(x):
            spec = copy.deepcopy(base)
            O.set_volcano_point(spec, x['ECO'], x['EO'], Tv)
            return spec

        def k_of(key):
            def k_at(v):
                spec = at(dict(x0, **{key: v}))
                k = O.rate_constants(spec, Tv, spec['system']['p'])
                return [k[r][0] for r in spec['reactions']], [k[r][1] for r in spec['reactions']]
            return k_at
        m = O.ClassicModel(at(x0), T=Tv)
        if c is not None:
            assert list(m.rnames) == [str(x) for x in c['rnames']]
            assert np.array_equal(m.kf, c['kf']) and np.array_equal(m.kr, c['kr']), name
        tof_terms = ['CO_ox']
        dirs = [stencil_desc(k_of(k), x0[k], H_DESC) for k in DESC] + \
               [stencil_desc(k_of(k), x0[k], 2.0 * H_DESC) for k in DESC]
        sign = rng.choice([-1.0, 1.0], len(m.dyn))
        ref, lo, pt, _ = _runs(name, m, y_full, tof_terms, dirs, sign)
        fd = []
        for k in DESC:
            tof = []
            for sgn in (1.0, -1.0):
                x = dict(x0, **{k: x0[k] + sgn * H_DESC})
                r = O.volcano_steady(base, x['ECO'], x['EO'], T=Tv)
                assert r['regular'], (name, k)
                tof.append(r['tof'])
            fd.append((np.log(tof[0]) - np.log(tof[1])) / (2.0 * H_DESC))
        dyn = list(m.dyn)
        o = dict(T=np.array(Tv), p=np.array(float(m.p)), desc_names=np.array(sorted(x0)),
                 desc=np.array([x0[k] for k in sorted(x0)], float), tof_terms=np.array(tof_terms),
                 dyn=np.array([m.snames[q] for q in dyn]), rnames=np.array(m.rnames), y=np.array(y_full)[dyn],
                 y_full=np.array(y_full), kf=m.kf.copy(), kr=m.kr.copy(), tof_ref=np.array(ref['tof']),
                 err=np.array(ref['err']), xi_ref=ref['xi'],
                 ddesc_names=np.array(DESC), ddesc_a=np.array([dirs[q][0] for q in (0, 1)]),
                 ddesc_c=np.array([dirs[q][1] for q in (0, 1)]), ddesc_ref=ref['dir'][:2], ddesc_104=lo['dir'][:2],
                 ddesc_pert=pt['dir'][:2], ddesc_2h=ref['dir'][2:4], ddesc_fd=np.array(fd))
        # no stored case straddles an energy clamp: the doubled step gives the same derivative
        assert np.all(np.abs(o['ddesc_2h'] - o['ddesc_ref']) <= CLAMP_TOL * np.abs(o['ddesc_ref'])), \
            (name, o['ddesc_2h'], o['ddesc_ref'])
        for k2, v in o.items():
            out[pre + k2] = v
        rel = lambda a: np.max(np.abs(a / o['ddesc_ref'] - 1.0))
        print('%-20s d ln TOF / d ECO %.9f  / d EO %.9f 1/eV (2h %.1e, pert %.1e, fd %.1e rel)  (%.0f s)'
              % (name, o['ddesc_ref'][0], o['ddesc_ref'][1], rel(o['ddesc_2h']), rel(o['ddesc_pert']),
                 rel(o['ddesc_fd']), time.time() - t0), flush=True)
    out['dnames'] = np.array(dnames)


def main():
    out, t0 = {}, time.time()
    rng = np.random.default_rng(SEED)
    new_cases(out, rng, t0)
    volcano_cases(out, rng, t0)
    np.savez_compressed(OUT, **out)
    print('wrote %s (%d new cases, %d volcano cases, %.0f s)' % (OUT, len(out['names']), len(out['dnames']),
                                                                  time.time() - t0))


if __name__ == '__main__':
    main()
