"""Uncertainty-ensemble goldens (pycatkin/classes/uncertainty.py).

(1) draw_*   the REFERENCE's own Uncertainty class, imported unmodified, run
             over the reference's Reaction / ReactionDerivedReaction objects
             on duck-typed states (make_golden.DuckState; the reference's
             state.py needs `ase`, absent here): after np.random.seed(SEED),
             mu = 0, sigma = 0.05, the key order and values of 8 consecutive
             get_correlated_state_noises() dicts, for DMTM and for the
             Butadiene MKM set p123_p124_p156.
(2) dmtm_*   DMTM, 3 temperatures (450, 600, 750 K at the input's pressure)
             x (1 unperturbed + 32 runs): the draws of (1) continued to 32
             runs, the same for every temperature, set as add_to_energy in
             the oracle spec and solved with the oracle's steady rule
             (oracle.mk_oracle.steady_rule: the device's rule restated):
             y, tof (r5 + r9), regular, crit.
(3) bd_*     Butadiene p123_p124_p156 (19 dynamic species), 2 temperatures
             (623, 823 K) x (1 + 8 runs), the draws of (1) on the BASE spec's
             states (the derived reactions take their energies there), the
             same rule: y, tof (BD_TERMS), regular, crit.

Every classification must be unambiguous: the rule's criterion `crit`
(max_i (|root_i - y_i| - 1e-22) / |root_i|, threshold 1e-6) at least 10x away
from the threshold on either side, asserted here, so the device test compares
every run and drops none.

Output: tests/golden/uncertainty_fixture.npz.
    OMP_NUM_THREADS=1 python tests/golden/make_uncertainty_fixture.py [--workers 8]
"""
import argparse
import copy
import multiprocessing as mp
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

SEED = 20261019
MU, SIGMA = 0.0, 0.05
DMTM_T = [450.0, 600.0, 750.0]
DMTM_RUNS = 32
DMTM_TERMS = ['r5', 'r9']
BD_T = [623.0, 823.0]
BD_RUNS = 8
BD_CASE = 'p123_p124_p156'
DIST = 1.0e-6
OUT = os.path.join(HERE, 'uncertainty_fixture.npz')
DMTM_INPUT = os.path.join(HERE, 'inputs', 'DMTM', 'input.json')


def reference_draws(ref_sys, nruns):
    """nruns consecutive get_correlated_state_noises() dicts of the reference's
    class after np.random.seed(SEED): (keys, values [nruns, n_keys])."""
    from pycatkin.classes.uncertainty import Uncertainty
    unc = Uncertainty(sys=ref_sys, mu=MU, sigma=SIGMA, nruns=nruns)
    np.random.seed(SEED)
    draws = [unc.get_correlated_state_noises() for _ in range(nruns)]
    keys = list(draws[0])
    assert all(list(d) == keys for d in draws)
    return keys, np.array([[d[k] for k in keys] for d in draws], float)


_specs = {}


def _init():
    import make_butadiene_fixture as MB
    from oracle import mk_oracle as O
    MB._init()
    _specs['dmtm'] = O.load_spec(DMTM_INPUT)
    _specs['bd'] = MB.case_spec(BD_CASE, dict(MB.CASES)[BD_CASE])
    _specs['bd_base'] = MB._base


def _job(arg):
    """One oracle solve: the steady rule on a spec with the noises as add_to_energy."""
    import make_butadiene_fixture as MB
    from oracle import mk_oracle as O
    kind, T, keys, vals = arg
    spec = _specs[kind]
    target = _specs['bd_base'] if kind == 'bd' else spec          # (3): the base spec's states
    saved = {k: target['states'][k]['add_to_energy'] for k in keys}
    try:
        for k, v in zip(keys, vals):
            target['states'][k]['add_to_energy'] = float(v)
        m = O.ClassicModel(spec, T=T)
        out = O.steady_rule(m, budget=400000)
        assert out is not None, (kind, T)
        terms = DMTM_TERMS if kind == 'dmtm' else MB.BD_TERMS
        return dict(y=out['y'][m.dyn], tof=m.tof(out['y'], terms), regular=out['regular'], crit=out['crit'],
                    dyn=[m.snames[i] for i in m.dyn])
    finally:
        for k, v in saved.items():
            target['states'][k]['add_to_energy'] = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workers', type=int, default=8)
    args = ap.parse_args()
    import make_butadiene_fixture as MB
    import make_golden as MG
    from oracle import mk_oracle as O
    store = dict(seed=SEED, mu=MU, sigma=SIGMA)

    # (1) the reference's draws
    dmtm_spec = O.load_spec(DMTM_INPUT)
    dk, dv = reference_draws(MG.build_reference_system(dmtm_spec, 'classic'), DMTM_RUNS)
    MB._init()
    bd_spec = MB.case_spec(BD_CASE, dict(MB.CASES)[BD_CASE])
    bk, bv = reference_draws(MB.reference_system(bd_spec, MB._base), BD_RUNS)
    store.update(draw_dmtm_keys=np.array(dk), draw_dmtm_vals=dv[:8], draw_bd_keys=np.array(bk), draw_bd_vals=bv[:8])
    # the perturbed butadiene states live in the base system
    assert all(k in MB._base['states'] for k in bk)

    # (2), (3): run 0 is the unperturbed member
    dnoise = np.vstack([np.zeros((1, len(dk))), dv])              # [1 + 32, keys]
    bnoise = np.vstack([np.zeros((1, len(bk))), bv])              # [1 + 8, keys]
    jobs = [('dmtm', T, dk, dnoise[r]) for T in DMTM_T for r in range(1 + DMTM_RUNS)]
    jobs += [('bd', T, bk, bnoise[r]) for T in BD_T for r in range(1 + BD_RUNS)]
    with mp.get_context('fork').Pool(args.workers, initializer=_init) as pool:
        res = pool.map(_job, jobs, chunksize=1)
    for tag, Ts, B, noise, keys in (('dmtm', DMTM_T, 1 + DMTM_RUNS, dnoise, dk), ('bd', BD_T, 1 + BD_RUNS, bnoise, bk)):
        rs = [r for j, r in zip(jobs, res) if j[0] == tag]
        crit = np.array([r['crit'] for r in rs]).reshape(len(Ts), B)
        regular = np.array([bool(r['regular']) for r in rs]).reshape(len(Ts), B)
        # unambiguous: a reached root at least 10x inside the threshold, a
        # transient end at least 10x outside (inf: Newton found no root)
        sure = np.where(regular, crit <= DIST / 10.0, crit >= DIST * 10.0)
        assert sure.all(), (tag, crit[~sure], np.argwhere(~sure))
        store[tag + '_T'] = np.array(Ts)
        store[tag + '_dyn'] = np.array(rs[0]['dyn'])
        store[tag + '_noise_keys'] = np.array(keys)
        store[tag + '_noise'] = noise[1:].T                         # [keys, runs]
        store[tag + '_y'] = np.array([r['y'] for r in rs]).reshape(len(Ts), B, -1).transpose(2, 0, 1)   # [NS, n_rep, B]
        store[tag + '_tof'] = np.array([r['tof'] for r in rs]).reshape(len(Ts), B)
        store[tag + '_regular'] = regular
        store[tag + '_crit'] = crit
        print('%s: %d conditions, regular %d, crit of roots <= %.2e, of transient ends >= %.2e' % (
            tag, regular.size, regular.sum(), crit[regular].max() if regular.any() else 0.0,
            crit[~regular].min() if (~regular).any() else np.inf))
    np.savez_compressed(OUT, **store)
    print('wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
