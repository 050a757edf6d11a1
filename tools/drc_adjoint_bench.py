"""Time the analytic degree of rate control (pck_drc_adjoint, csrc/mk_sens.h;
its steps in csrc/mk_adjoint.h) against the finite-difference one (pck_drc) and against its own pieces.

  dmtm      the bench's 64 x 64 grid of T 400-800 K x p 1e4-1e6 Pa, TOF = r5 + r9,
            steady solves (System.drc_batch(steady=True)'s settings)
  volcano   the 1024 x 1024 COOx volcano grid at 600 K, TOF = CO_ox
  syn24     the 64 conditions of tests/golden/synthetic_sizes_fixture.npz tiled
            to 4 096, TOF = R0 (24 species, 72 reactions: the FD is 145 solves)

Per workload, each one launch sequence on the current stream:
  fd        pck_drc, eps 5e-2 (2R+1 steady solves per condition; only for the
            workloads named by --fd)
  adjoint   pck_drc_adjoint (one steady solve + k_drc_adjoint)
  solve     pck_solve alone, the same parameters
  at        pck_drc_at alone at the solve's states (k_drc_adjoint + nothing else)

HIP events around `reps` back-to-back calls, the median of `--rounds` rounds
with the spread.  Prints one JSON line per workload.  Needs the GPU.

    python tools/drc_adjoint_bench.py [--workloads dmtm,volcano,syn24] [--rounds 5] [--fd dmtm,syn24]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INPUTS = os.path.join(ROOT, 'tests', 'golden', 'inputs')


def dmtm(P, grid):
    sim = P.read_from_input_file(os.path.join(INPUTS, 'DMTM', 'input.json'))
    TT, pp = np.meshgrid(np.linspace(400.0, 800.0, grid), np.logspace(4.0, 6.0, grid), indexing='ij')
    return sim, ('r5', 'r9'), dict(T=TT.ravel(), p=pp.ravel()), TT.size


def volcano(P, grid):
    from pycatkin_amd.functions.volcano import set_volcano_energies
    sim = P.read_from_input_file(os.path.join(INPUTS, 'COOxVolcano', 'input.json'))
    set_volcano_energies(sim)
    be = np.linspace(-2.5, 0.5, grid)
    E1, E2 = np.meshgrid(be, be, indexing='ij')
    return sim, ('CO_ox',), dict(T=np.full(E1.size, 600.0), desc={'ECO': E1.ravel(), 'EO': E2.ravel()}), E1.size


def syn24(P, n):
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    from make_synthetic_sizes_fixture import NETS, SEED_NET, T, T_END
    from pycatkin_amd.functions.synthetic import synthetic_network, synthetic_system
    ns, nr = NETS['syn24']
    sim = synthetic_system(synthetic_network(n_species=ns, n_reactions=nr, seed=SEED_NET), t_end=T_END)[0]
    D = dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'synthetic_sizes_fixture.npz')))['desc']
    D = np.tile(D, ((n + D.shape[0] - 1) // D.shape[0], 1))[:n]
    return sim, ('R0',), dict(T=np.full(n, float(T)), desc={'D%d' % k: D[:, k].copy() for k in range(4)}), n


def run(name, sim, terms, kw, n, a, torch):
    from pycatkin_amd.classes.system import (ROOT_DIST, SCREEN_MARGIN, SCREEN_MAX_LANE_SPECIES, SCREEN_RTOL,
                                             STEADY_TRANSIENT)
    plan, net = sim.plan(terms), sim.device(terms)
    T, p, d, fx, y0, inflow = sim._inputs(net, plan, n, kw['T'], kw.get('p'), kw.get('desc'), None, None, None)
    times = sim.params['times'] or [0.0, 1.0e4]
    screen = (SCREEN_RTOL, SCREEN_MARGIN) if net.NDYN <= SCREEN_MAX_LANE_SPECIES else None
    prm = dict(t0=times[0], t_end=times[-1], rtol=STEADY_TRANSIENT[0], atol=STEADY_TRANSIENT[1], max_steps=200000,
               newton=True, root_dist=ROOT_DIST, screen=screen)
    dev = lambda x: None if x is None else torch.as_tensor(np.asarray(x, float), dtype=torch.float64, device='cuda')
    T, p, d, fx, y0, inflow = (dev(x) for x in (T, p, d, fx, y0, inflow))
    kf, kr = net.rate_constants(n, T, p, d)
    kf, kr = kf.contiguous(), kr.contiguous()
    state = {}

    def solve():
        state['s'] = net.solve(n, T, p, y0, d, fx, inflow, out=state.get('s'), **prm)

    def adjoint():
        state['a'] = net.drc_adjoint(n, T, p, y0, d, fx, inflow, **prm)

    def fd():
        state['f'] = net.drc(n, T, p, y0, d, fx, inflow, drc_eps=5.0e-2, **prm)

    def at():
        state['t'] = net.drc_at(n, T, p, state['s']['y'], kf, kr, d, fx, inflow, state['s']['status'])

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps          # ms per call

    todo = [('solve', solve, a.reps), ('at', at, a.reps), ('adjoint', adjoint, a.reps)]
    if name in a.fd.split(','):
        todo.append(('fd', fd, 1))
    for _, fn, _ in todo:                          # warm-up (hipRTC compiles, the memory pool)
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k, _, _ in todo}
    for _ in range(a.rounds):
        for k, fn, reps in todo:
            ms[k].append(timed(fn, reps))
    res = dict(workload=name, conditions=n, species=net.NDYN, reactions=net.NRXN, group_lanes=net.group_lanes())
    for k, v in ms.items():
        res[k + '_ms'] = round(float(np.median(v)), 4)
        res[k + '_ms_min_max'] = [round(float(min(v)), 4), round(float(max(v)), 4)]
    if 'fd' in ms:
        res['fd_over_adjoint'] = round(res['fd_ms'] / res['adjoint_ms'], 2)
        res['fd_over_solve'] = round(res['fd_ms'] / res['solve_ms'], 2)
    res['adjoint_over_solve'] = round(res['adjoint_ms'] / res['solve_ms'], 3)
    st = state['a']['status'].cpu().numpy()
    res['adjoint_status_counts'] = {int(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))}
    ok = st == 0
    xa = state['a']['xi'].cpu().numpy()[:, ok]
    res['adjoint_sum_rule_worst'] = float(np.max(np.abs(xa.sum(axis=0) - 1.0))) if ok.any() else None
    if 'f' in state:
        both = ok & (state['f']['status'].cpu().numpy() == 0)
        res['fd_eps5e-2_minus_adjoint_worst'] = float(np.max(np.abs(
            state['f']['xi'].cpu().numpy()[:, both] - state['a']['xi'].cpu().numpy()[:, both]))) if both.any() else None
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workloads', default='dmtm,volcano,syn24')
    ap.add_argument('--dmtm-grid', type=int, default=64)
    ap.add_argument('--volcano-grid', type=int, default=1024)
    ap.add_argument('--syn24-n', type=int, default=4096)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--fd', default='dmtm,syn24', help='workloads that also time the finite-difference pck_drc')
    a = ap.parse_args()
    import torch
    import pycatkin_amd as P
    size = dict(dmtm=a.dmtm_grid, volcano=a.volcano_grid, syn24=a.syn24_n)
    for name in a.workloads.split(','):
        sim, terms, kw, n = dict(dmtm=dmtm, volcano=volcano, syn24=syn24)[name](P, size[name])
        run(name, sim, terms, kw, n, a, torch)


if __name__ == '__main__':
    main()
