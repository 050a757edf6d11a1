"""Time the device eigenvalue path (pck_stability_at: pck_jacobian, the
restriction to the conservation class, csrc/mk_eig.h: k_eig_lane / k_eig_grp<G>)
against today's host path on the same Jacobians (pck_jacobian, the copy to the
host, np.linalg.eigvals).

  volcano   the 1024 x 1024 COOx volcano grid at 600 K, at its solved states,
            reduce = 1 (3 x 3 matrices; both schedules)
  ch4       the patched CH4 system at 16 384 temperatures 473-573 K, at the ends
            of its transients to 1e4 s, reduce = 0 (16 x 16: the reference's test)
  syn24     the 64 conditions of tests/golden/synthetic_sizes_fixture.npz tiled
            to 4 096, at their solved states, reduce = 1

Device: inputs resident, HIP events around `reps` back-to-back calls, the
median of `--rounds` rounds with the spread, after a warm-up call; the rounds
interleave the schedules.  Host: wall clock of jacobian + copy + eigvals on the
first `--host-sample` conditions, scaled by conditions / sample (LAPACK's cost
per matrix does not depend on the batch; the scaling is stated in the output as
host_scaled_from).  Prints one JSON line per workload.  Needs the GPU.

    python tools/spectrum_bench.py [--workloads volcano,ch4,syn24] [--rounds 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
INPUTS = os.path.join(ROOT, 'tests', 'golden', 'inputs')


def ch4(P, n):
    s = P.read_from_input_file(os.path.join(INPUTS, 'CH4', 'input.json'), formulation='patched')
    for r, st in (('C_ads', 'sC'), ('O_ads', 'sO')):
        s.reactions[r].dErxn_user = 1.0
        s.states[st].Gelec = 1.0
    s.build()
    return s, (), dict(T=np.linspace(473.0, 573.0, n)), n


def states(name, sim, net, plan, n, T, p, d, fx, y0, inflow):
    """(y, status) the workload's stability is asked at"""
    from pycatkin_amd.classes.system import (ROOT_DIST, SCREEN_MARGIN, SCREEN_MAX_LANE_SPECIES, SCREEN_RTOL,
                                             STEADY_TRANSIENT)
    if name == 'ch4':                              # SteadyStateSolver.solve_ode_batch's transient
        y0 = sim._to_plan(plan, sim.initial_system[len(sim.gas_indices):][:, None])[:, 0]
        s = net.solve(n, T, p, np.repeat(y0[:, None], n, axis=1), d, fx, inflow, t0=0.0, t_end=1.0e4, rtol=1e-10,
                      atol=1e-12, max_steps=200000)
    else:
        times = sim.params['times'] or [0.0, 1.0e4]
        screen = (SCREEN_RTOL, SCREEN_MARGIN) if net.NDYN <= SCREEN_MAX_LANE_SPECIES else None
        s = net.solve(n, T, p, y0, d, fx, inflow, t0=times[0], t_end=times[-1], rtol=STEADY_TRANSIENT[0],
                      atol=STEADY_TRANSIENT[1], max_steps=200000, newton=True, root_dist=ROOT_DIST, screen=screen)
    return s['y'], s['status']


def run(name, sim, kw, n, reduce, a, torch):
    from pycatkin_amd import _lib as L
    plan, net = sim.plan(()), sim.device(())
    T, p, d, fx, y0, inflow = sim._inputs(net, plan, n, kw['T'], kw.get('p'), kw.get('desc'), None, None, None)
    dev = lambda x: None if x is None else torch.as_tensor(np.array(x, float), dtype=torch.float64, device='cuda')
    T, p = dev(np.broadcast_to(np.asarray(T, float), (n,))), dev(np.broadcast_to(np.asarray(p, float), (n,)))
    d, fx, inflow = dev(d), dev(fx), dev(inflow)
    kf, kr = net.rate_constants(n, T, p, d)
    kf, kr = kf.contiguous(), kr.contiguous()
    y, st = states(name, sim, net, plan, n, T, p, d, fx, y0, inflow)
    st = torch.zeros_like(st)                      # every condition is computed, whatever the solve said
    ns_eff = net.NDYN - (net.NCONS if reduce else 0)
    modes = [('group', L.SENS_LANES_GROUP)] + ([('lane', L.SENS_LANES_ONE)] if ns_eff <= L.MAX_DYN_LANE else [])
    state = {}

    def call(key, mode):
        def fn():
            state[key] = net.stability_at(n, T, p, y, kf, kr, d, fx, inflow, st, reduce=reduce, lanes=mode,
                                          want=('re_max', 'scale', 'status'))
        return fn

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps          # ms per call

    todo = [(k, call(k, m)) for k, m in modes]
    for _, fn in todo:                             # warm-up (the memory pool)
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k, _ in todo}
    for _ in range(a.rounds):
        for k, fn in todo:
            ms[k].append(timed(fn, a.reps))
    # today's host path on a subsample, full Jacobian (what test_convergence_batch does)
    m = min(n, a.host_sample)
    sub = lambda x: None if x is None else (x[..., :m].contiguous() if x.shape[-1] == n else x)
    host = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        J = net.jacobian(m, sub(T), sub(p), sub(y), sub(kf), sub(kr), sub(d), sub(fx), sub(inflow)).cpu().numpy()
        w = np.linalg.eigvals(np.moveaxis(J, 2, 0))
        host.append((time.perf_counter() - t0) * 1e3 * n / m)
    res = dict(workload=name, conditions=n, species=net.NDYN, ns_eff=ns_eff, reduce=int(reduce),
               host_ms=round(float(np.median(host)), 2), host_scaled_from=m)
    for k, v in ms.items():
        res[k + '_ms'] = round(float(np.median(v)), 4)
        res[k + '_ms_min_max'] = [round(float(min(v)), 4), round(float(max(v)), 4)]
        res[k + '_lanes'] = state[k]['lanes']
        res['host_over_' + k] = round(res['host_ms'] / res[k + '_ms'], 1)
        s = state[k]['status'].cpu().numpy()
        res[k + '_status_counts'] = {int(q): int(c) for q, c in zip(*np.unique(s, return_counts=True))}
    ok = (state['group']['status'] == 0)
    rm, sc = state['group']['re_max'][ok], state['group']['scale'][ok]
    res['verdicts'] = dict(stable=int((rm < -sc).sum()), unstable=int((rm > sc).sum()),
                           marginal=int(((rm >= -sc) & (rm <= sc)).sum()))
    if not reduce:                                 # the host's full-matrix re_max on the subsample, for the record
        d_ = np.abs(w.real.max(axis=1) - state['group']['re_max'][:m].cpu().numpy())
        res['re_max_minus_host_over_scale_worst'] = float(np.nanmax(d_ / state['group']['scale'][:m].cpu().numpy()))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workloads', default='volcano,ch4,syn24')
    ap.add_argument('--volcano-grid', type=int, default=1024)
    ap.add_argument('--ch4-n', type=int, default=16384)
    ap.add_argument('--syn24-n', type=int, default=4096)
    ap.add_argument('--host-sample', type=int, default=4096)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    import torch
    import pycatkin_amd as P
    from drc_adjoint_bench import syn24, volcano
    for name in a.workloads.split(','):
        if name == 'volcano':
            sim, _, kw, n = volcano(P, a.volcano_grid)
        elif name == 'syn24':
            sim, _, kw, n = syn24(P, a.syn24_n)
        elif name == 'ch4':
            sim, _, kw, n = ch4(P, a.ch4_n)
        else:
            raise SystemExit('unknown workload %r' % name)
        run(name, sim, kw, n, name != 'ch4', a, torch)


if __name__ == '__main__':
    main()
