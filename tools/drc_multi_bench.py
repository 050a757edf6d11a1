"""Time the multi-objective analytic degree of rate control (pck_drc_multi_at,
csrc/mk_sens_multi.h: k_multi_adjoint; the steps both group kernels share are in
csrc/mk_adjoint.h) against the single-objective kernel of
the same tree (pck_drc_at, csrc/mk_sens.h: k_drc_adjoint), interleaved in one
process.

  dmtm      the bench's 64 x 64 grid of T 400-800 K x p 1e4-1e6 Pa
  syn24     the 64 conditions of tests/golden/synthetic_sizes_fixture.npz tiled
            to 4 096 (24 species, 72 reactions)
  volcano   the 1024 x 1024 COOx volcano grid at 600 K
  cstr      the Pd111 CSTR at 10 000 temperatures 423-623 K

Per workload one steady solve gives the states; then, each a kernel alone at
those states on the current stream:
  drc_at    pck_drc_at, the workload's TOF terms compiled into the plan
  K1        pck_drc_multi_at, the same TOF terms as the one objective
  K2        ... and a second rate objective (the first TOF term alone)
  KNS       every dynamic species as a coverage objective (K = NS)
On a network of at most 8 dynamic species (volcano, cstr) K1 / K2 / KNS are
also timed on the one-lane kernel (csrc/mk_sens_multi_lane.h:
k_lane_multi_adjoint, pck_network_set_multi_lanes) as lane_K1 / lane_K2 /
lane_KNS, beside the group kernel in the same rounds.

HIP events around `reps` back-to-back calls, the median of `--rounds` rounds
with the spread; the rounds interleave all of them.  Prints one JSON line per
workload with the K = 1 time over drc_at's, the increment per objective,
(KNS - K1) / (NS - 1), and for the one-lane kernel group over lane per K and
the worst |xi_lane - xi_group| over the answered conditions.  Needs the GPU.

    python tools/drc_multi_bench.py [--workloads dmtm,syn24,volcano,cstr] [--rounds 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def run(name, sim, terms, kw, n, a, torch):
    from pycatkin_amd.classes.system import (ROOT_DIST, SCREEN_MARGIN, SCREEN_MAX_LANE_SPECIES, SCREEN_RTOL,
                                             STEADY_TRANSIENT)
    plan, net = sim.plan(terms), sim.device(terms)
    plan0, net0 = sim.plan(()), sim.device(())
    assert plan0.reactions == plan.reactions and plan0.dyn == plan.dyn
    T, p, d, fx, y0, inflow = sim._inputs(net, plan, n, kw['T'], kw.get('p'), kw.get('desc'), None, None, None)
    times = sim.params['times'] or [0.0, 1.0e4]
    screen = (SCREEN_RTOL, SCREEN_MARGIN) if net.NDYN <= SCREEN_MAX_LANE_SPECIES else None
    prm = dict(t0=times[0], t_end=times[-1], rtol=STEADY_TRANSIENT[0], atol=STEADY_TRANSIENT[1], max_steps=200000,
               newton=True, root_dist=ROOT_DIST, screen=screen)
    dev = lambda x: None if x is None else torch.as_tensor(np.asarray(x, float), dtype=torch.float64, device='cuda')
    T, p, d, fx, y0, inflow = (dev(x) for x in (T, p, d, fx, y0, inflow))
    kf, kr = net.rate_constants(n, T, p, d)
    kf, kr = kf.contiguous(), kr.contiguous()
    s = net.solve(n, T, p, y0, d, fx, inflow, **prm)
    y, st = s['y'], s['status']
    NS, R = net.NDYN, net.NRXN
    _, wr1, _ = sim._objectives(plan0, [tuple(terms)])
    _, wr2, _ = sim._objectives(plan0, [tuple(terms), (terms[0],)])
    wr1, wr2, wyn = dev(wr1), dev(wr2), dev(np.eye(NS))
    state = {}

    def drc_at():
        state['at'] = net.drc_at(n, T, p, y, kf, kr, d, fx, inflow, st)

    def multi(key, wr, wy, mode=0):
        def fn():
            net0.set_multi_lanes(mode)
            state[key] = net0.drc_multi_at(n, T, p, y, kf, kr, wr, wy, d, fx, inflow, st)
            state[key + '_lanes'] = net0.sens_lanes()
        return fn

    todo = [('drc_at', drc_at), ('K1', multi('K1', wr1, None)), ('K2', multi('K2', wr2, None)),
            ('KNS', multi('KNS', None, wyn))]
    one_lane = NS <= 8
    if one_lane:
        todo += [('lane_K1', multi('lane_K1', wr1, None, 1)), ('lane_K2', multi('lane_K2', wr2, None, 1)),
                 ('lane_KNS', multi('lane_KNS', None, wyn, 1))]

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps          # ms per call

    for _, fn in todo:                             # warm-up (the memory pool)
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k, _ in todo}
    for _ in range(a.rounds):
        for k, fn in todo:
            ms[k].append(timed(fn, a.reps))
    net0.set_multi_lanes(0)
    res = dict(workload=name, conditions=n, species=NS, reactions=R, lanes=state['K1_lanes'])
    for k, v in ms.items():
        res[k + '_ms'] = round(float(np.median(v)), 4)
        res[k + '_ms_min_max'] = [round(float(min(v)), 4), round(float(max(v)), 4)]
    res['K1_over_drc_at'] = round(res['K1_ms'] / res['drc_at_ms'], 3)
    res['ms_per_objective'] = round((res['KNS_ms'] - res['K1_ms']) / max(NS - 1, 1), 4)
    res['second_objective_ms'] = round(res['K2_ms'] - res['K1_ms'], 4)
    ok = (state['K1']['status'] == 0)
    xa, xm = state['at']['xi'][:, ok], state['K1']['xi'][0][:, ok]
    res['status_counts'] = {int(k): int(v) for k, v in zip(*np.unique(state['K1']['status'].cpu().numpy(),
                                                                      return_counts=True))}
    res['K1_minus_drc_at_worst'] = float((xa - xm).abs().max()) if bool(ok.any()) else None
    if one_lane:
        assert state['lane_K1_lanes'] == 1 and state['K1_lanes'] > 1
        for k in ('K1', 'K2', 'KNS'):
            res['group_over_lane_' + k] = round(res[k + '_ms'] / res['lane_' + k + '_ms'], 3)
            g, l = state[k], state['lane_' + k]
            assert bool((g['status'] == l['status']).all()) and bool((g['ostatus'] == l['ostatus']).all())
            both = (g['ostatus'] == 0).unsqueeze(1).expand_as(g['xi'])
            dx = (g['xi'] - l['xi'])[both]
            res['lane_minus_group_worst_' + k] = float(dx.abs().max()) if dx.numel() else None
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workloads', default='dmtm,syn24,volcano')
    ap.add_argument('--dmtm-grid', type=int, default=64)
    ap.add_argument('--volcano-grid', type=int, default=1024)
    ap.add_argument('--syn24-n', type=int, default=4096)
    ap.add_argument('--cstr-n', type=int, default=10000)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    import torch
    import pycatkin_amd as P
    from drc_adjoint_bench import dmtm, syn24, volcano
    from sens_adjoint_bench import cstr
    size = dict(dmtm=a.dmtm_grid, volcano=a.volcano_grid, syn24=a.syn24_n, cstr=a.cstr_n)
    for name in a.workloads.split(','):
        sim, terms, kw, n = dict(dmtm=dmtm, volcano=volcano, syn24=syn24, cstr=cstr)[name](P, size[name])
        run(name, sim, terms, kw, n, a, torch)


if __name__ == '__main__':
    main()
