"""Oracle fixture of the networks at the size and packing limits of the
lane-group kernels (tests/test_gpu_edge_sizes.py; tests/_synth.py:
edge_network), one per kernel switch or packed-field limit:

  e8a    8 /  28   last network on the one-lane path
  e8b    8 /  29   the same size, sent to the group path by the LDS rule
  e9     9 /  27   first size past PCK_MAX_DYN_LANE
  e16   16 / 256   quad kernel at exactly 64 KiB of LDS; reaction index 255
  e17   17 /  51   first row of the 32-lane kernel
  e32   32 /  96   full 32-lane group
  e33   33 /  99   first row of the 64-lane kernel
  e64   64 / 256   PCK_MAX_DYN with PCK_MAX_RXN: species 63, reaction 255
  x3    12 /  30   3 A2 <-> A3 + 2 s: exponent 3, forward and reverse
  x31   12 /  30   31 A2 <-> A3 + 30 s: PCK_GRP_MAX_EXP
  p6    64 / 120   one reaction with six distinct dynamic participants, the
                   species at plan index 0 and 63 among them (rates only: not
                   in the fixture)

N = 8 conditions each, random descriptors (np.random.default_rng(11), uniform
in [-0.5, 0.5]^4), T = 500 K.  Per network the oracle stores

  * the transient from the start state at 9 times (0 and 8 log-spaced times
    1e-5 .. 1e2 s): mk_oracle.ClassicModel rhs / jac, scipy LSODA at rtol
    1e-12 / atol 1e-20 with t_eval;
  * the steady-state rule to t_end = 1e8 s (mk_oracle.steady_rule as in
    make_synthetic_sizes_fixture.py): y, `regular`, `crit`, and the TOF of
    the network's TOF_TERM with `tofabs` = |rf| + |rr| of that reaction at y.
    The adsorption R0 is no use as a TOF here: these cycles turn over slowly
    next to the adsorption equilibrium, so its net rate cancels to 1e-3 ..
    1e-11 of its terms and a relative bound on it tests nothing.  TOF_TERM
    is, per network, the reaction with the largest net rate among those
    whose net rate is at least 0.1 (|rf| + |rr|) at all 8 steady states
    (the generator asserts that ratio).

The generator asserts that the oracle answers every condition of every
network and finds at least 6 of the 8 regular (the seeds below were chosen
for that).

    OMP_NUM_THREADS=1 python tests/golden/make_edge_sizes_fixture.py [--workers 8]

writes tests/golden/edge_sizes_fixture.npz (numpy arrays only).
"""
import argparse
import multiprocessing as mp
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'edge_sizes_fixture.npz')
# key: (species, reactions, seed of edge_network)
NETS = {'e8a': (8, 28, 1), 'e8b': (8, 29, 1), 'e9': (9, 27, 2), 'e16': (16, 256, 1), 'e17': (17, 51, 1),
        'e32': (32, 96, 1), 'e33': (33, 99, 1), 'e64': (64, 256, 2), 'x3': (12, 30, 2), 'x31': (12, 30, 2),
        'p6': (64, 120, 1)}
TOF_TERM = {'e8a': 'R10', 'e8b': 'R26', 'e9': 'R26', 'e16': 'R3', 'e17': 'R6', 'e32': 'R12', 'e33': 'R97',
            'e64': 'R191', 'x3': 'R19', 'x31': 'R1'}
MIN_TOF_RATIO = 0.1         # |rf - rr| / (|rf| + |rr|) of the TOF term at every steady state
FIXTURE_KEYS = ('e8a', 'e8b', 'e9', 'e16', 'e17', 'e32', 'e33', 'e64', 'x3', 'x31')
# the reaction with the large exponent: `e` A2 <-> A3 + (e - 1) s, inserted
# after the chain, i.e. at index 2 + (12 - 2) = 12
X_EXP = {'x3': 3, 'x31': 31}
X_INDEX = 12
N = 8
T = 500.0
T_END = 1.0e8
T_OUT = np.concatenate([[0.0], np.logspace(-5.0, 2.0, 8)])
ROOT_DIST = 1.0e-6          # pycatkin_amd/classes/system.py ROOT_DIST
STEADY_ATOL = 1.0e-22       # STEADY_TRANSIENT[1]
MIN_REGULAR = 6


def descriptors():
    return np.random.default_rng(11).uniform(-0.5, 0.5, (N, 4))


def power_reaction(e):
    """`e` A2 <-> A3 + (e - 1) s"""
    return (['A2'] * e, ['A3'] + ['s'] * (e - 1))


def tune_power_reaction(net, e, j=X_INDEX):
    """Energies at which both directions of `e` A2 <-> A3 + (e - 1) s count at
    every descriptor vector: A2 independent of the descriptors with e E(A2)
    = -0.62 eV next to E(A3) = -0.6 +- 0.5 eV (at the generator's E0 ~ -0.5
    eV, e E(A2) = -15 eV at e = 31 and one direction's barrier is 15 eV),
    and a low intrinsic barrier, so that k c^e stands above 1e-6 of the
    adsorption rates at c in [0.5, 1] (test_gpu_edge_sizes asserts it)."""
    net['E0'][2] = -0.62 / e
    net['Ed'][2] = 0.0
    net['E0'][3] = -0.6
    net['Ed'][3] = [0.5, 0.0, 0.0, 0.0]
    net['beta'][j] = 0.1
    return net


def tune_wide_reaction(net, names, j):
    """Energies at which both directions of p6's six-participant step
    q0 + q1 + q2 <-> q3 + q4 + s, and its derivative by the sixth participant
    (kr c3 c4), stand far above the floors of the rate comparisons: the five
    adsorbates independent of the descriptors, both sides at -0.6 eV, a low
    intrinsic barrier (test_gpu_edge_sizes asserts the magnitudes)."""
    for nm, e in zip(names[:5], (-0.2, -0.2, -0.2, -0.3, -0.3)):
        a = net['adsorbates'].index(nm)
        net['E0'][a] = e
        net['Ed'][a] = 0.0
    net['beta'][j] = 0.1
    return net


P6_INDEX = 2 + 62           # the wide reaction follows the chain of 63 adsorbates


def p6_names(dyn):
    """The six participants of p6's wide reaction from the plan's species
    order: index 0, index 63 and four in between."""
    return [dyn[i] for i in (0, 13, 27, 41, 55, 63)]


def edge_net(key):
    """The plain-data network of a key of NETS."""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    sys.path.insert(0, ROOT)
    from _synth import edge_network
    ns, nr, seed = NETS[key]
    if key in X_EXP:
        return tune_power_reaction(edge_network(ns, nr, seed, extra=(power_reaction(X_EXP[key]),)), X_EXP[key])
    if key == 'p6':
        from pycatkin_amd.functions.synthetic import synthetic_system
        dyn = synthetic_system(edge_network(ns, nr, seed))[0].plan().dyn      # the order does not depend on reactions
        q = p6_names(dyn)
        return tune_wide_reaction(edge_network(ns, nr, seed, extra=((q[:3], q[3:]),)), q, P6_INDEX)
    return edge_network(ns, nr, seed)


def _cond(arg):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from scipy.integrate import solve_ivp
    from _synth import spec_of
    from oracle import mk_oracle as O
    key, k, d = arg
    m = O.ClassicModel(spec_of(edge_net(key), np.asarray(d), T), T=T)
    dyn = m.dyn
    names = [m.snames[i] for i in dyn]
    m._set_reach(m.y0)
    sol = solve_ivp(lambda t, y: m.rhs(y), (0.0, T_OUT[-1]), m.y0, method='LSODA', jac=lambda t, y: m.jac(y),
                    rtol=1e-12, atol=1e-20, t_eval=T_OUT)
    traj = sol.y[dyn].T if sol.status == 0 else np.full((T_OUT.size, len(dyn)), np.nan)     # [n_out, NS]
    r = O.steady_rule(m, dist=ROOT_DIST, dist_atol=STEADY_ATOL, budget=400000, t_end=T_END)
    if r is None or sol.status != 0:
        nan = np.full(len(dyn), np.nan)
        return key, k, dict(ok=False, regular=False, crit=np.inf, y=nan, tof=np.nan, tofabs=np.nan, traj=traj), names
    # |rf| + |rr| of the TOF term at the answer: the scale its net rate must not cancel against
    tofabs = float(np.abs(m.rates(r['y'])[m.rnames.index(TOF_TERM[key])]).sum())
    return key, k, dict(ok=True, regular=r['regular'], crit=r['crit'], y=r['y'][dyn], tof=m.tof(r['y'], [TOF_TERM[key]]),
                        tofabs=tofabs, traj=traj), names


def generate(keys, workers):
    D = descriptors()
    jobs = [(key, k, D[k]) for key in sorted(keys, key=lambda q: -NETS[q][0] * NETS[q][1]) for k in range(N)]
    res, names = {}, {}
    with mp.get_context('spawn').Pool(workers) as pool:
        for key, k, o, nm in pool.imap_unordered(_cond, jobs):
            res[(key, k)], names[key] = o, nm
    out = dict(desc=D, T=np.array(T), t_end=np.array(T_END), t_out=T_OUT)
    for key in keys:
        rows = [res[(key, k)] for k in range(N)]
        out[key + '_dyn'] = np.array(names[key])
        for f in ('ok', 'regular'):
            out[key + '_' + f] = np.array([r[f] for r in rows], bool)
        for f in ('crit', 'tof', 'tofabs', 'y', 'traj'):
            out[key + '_' + f] = np.array([r[f] for r in rows], float)
        print('%s: %d / %d answered, %d steady state reached' % (key, out[key + '_ok'].sum(), N,
                                                                  out[key + '_regular'].sum()), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workers', type=int, default=8)
    ap.add_argument('--keys', default=','.join(FIXTURE_KEYS), help='probe a subset (nothing is written)')
    args = ap.parse_args()
    keys = tuple(args.keys.split(','))
    t = time.time()
    out = generate(keys, args.workers)
    for key in keys:
        assert out[key + '_ok'].all(), (key, out[key + '_ok'])
        assert out[key + '_regular'].sum() >= MIN_REGULAR, (key, out[key + '_regular'])
        assert np.all(np.abs(out[key + '_tof']) >= MIN_TOF_RATIO * out[key + '_tofabs']), (key, out[key + '_tof'])
    if keys == FIXTURE_KEYS:
        np.savez_compressed(OUT, **out)
        print('wrote %s (%.0f s)' % (OUT, time.time() - t))


if __name__ == '__main__':
    main()
