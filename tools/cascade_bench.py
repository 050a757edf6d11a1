"""Time the fused reactor cascade (System.solve_cascade_batch(method='fused'):
pck_solve_cascade, csrc/mk_cascade.h) against the march a user writes with the
single-tank API: a loop of System.solve_batch(to_numpy=False, inflow=previous
outlet) over the cells of a CSTReactor carrying one cell's numbers.

  Pd111 (examples/COOxReactor), temperatures 423-623 K, `cells` in --cells,
  n in --sizes (the loop runs with wave_order='off' from 131 072 conditions,
  where solve_batch's 'auto' would add the cost-order preview)

One GPU, HIP events around `reps` back-to-back calls, fused and loop
alternated in the same process, the median of `--rounds` rounds with the
spread, after a warm-up of every shape.  Also recorded: the integrator steps of
both (start='system'; they should agree) and of the fused march with
start='upstream'.  Status counts: the bed summary for the fused march, the last
cell's status for the loop.  Prints one JSON line per (n, cells).  Needs the GPU.

    python tools/cascade_bench.py [--sizes 10000,262144] [--cells 8,32] [--rounds 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INPUTS = os.path.join(ROOT, 'tests', 'golden', 'inputs')
BED = dict(residence_time=4.5, volume=1.8e-7, catalyst_area=3.82e-9)
TOF = ('CO_ox',)


def pd111(P, reactor):
    s = P.read_from_input_file(os.path.join(INPUTS, 'COOxReactor', 'input_Pd111.json'))
    s.add_reactor(reactor)
    s._plans.clear()
    return s


def run(P, torch, n, cells, a):
    from pycatkin_amd import _lib as L
    T = np.linspace(423.0, 623.0, n)
    bed = pd111(P, P.PFReactor(cells=cells, **BED))
    cell = pd111(P, P.CSTReactor(**{k: v / cells for k, v in BED.items()}))
    plan = cell.plan(TOF)
    off = int(plan.ip[L.I_HDR + L.D_DYN])
    flow = torch.as_tensor(np.asarray(plan.dp[off: off + 4 * len(plan.dyn)]).reshape(-1, 4)[:, 3] != 0.0,
                           device='cuda')[:, None]
    inflow0 = torch.as_tensor(np.tile(plan.inflow_default[:, None], (1, n)), dtype=torch.float64, device='cuda')
    order = 'off' if n >= 131072 else 'auto'
    state = {}

    def fused(start):
        def fn():
            state['fused_' + start] = bed.solve_cascade_batch(T=T, tof_terms=TOF, start=start, method='fused',
                                                              profile=False, to_numpy=False)
        return fn

    def loop():
        cur, steps = inflow0, 0
        for _ in range(cells):
            r = cell.solve_batch(T=T, inflow=cur, tof_terms=TOF, steady=True, to_numpy=False, wave_order=order)
            cur = torch.where(flow, r['y'], cur)
            steps = steps + r['nsteps'].sum(dtype=torch.int64)
        state['loop'] = dict(y=r['y'], status=r['status'], steps=steps)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.reps            # ms per call

    todo = [('fused', fused('system')), ('loop', loop), ('fused_upstream', fused('upstream'))]
    for _, fn in todo:                                 # warm-up: hipRTC, the memory pool
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k, _ in todo}
    for _ in range(a.rounds):
        for k, fn in todo:
            ms[k].append(timed(fn))
    res = dict(workload='pd111_cascade', conditions=n, cells=cells, loop_wave_order=order)
    for k, v in ms.items():
        res[k + '_ms'] = round(float(np.median(v)), 4)
        res[k + '_ms_min_max'] = [round(float(min(v)), 4), round(float(max(v)), 4)]
    res['loop_over_fused'] = round(res['loop_ms'] / res['fused_ms'], 3)
    f, u, lp = state['fused_system'], state['fused_upstream'], state['loop']
    res['fused_steps'] = int(f['nsteps'].sum(dtype=torch.int64))
    res['loop_steps'] = int(lp['steps'])
    res['fused_upstream_steps'] = int(u['nsteps'].sum(dtype=torch.int64))
    res['upstream_steps_saved'] = round(1.0 - res['fused_upstream_steps'] / res['fused_steps'], 4)
    for k, r in (('fused', f), ('fused_upstream', u), ('loop', lp)):
        s = r['status'].cpu().numpy()
        res[k + '_status_counts'] = {int(q): int(c) for q, c in zip(*np.unique(s, return_counts=True))}
    ok = ((f['status'] == 0) & (lp['status'] == 0)).cpu().numpy()
    ya, yb = f['y'].cpu().numpy()[:, ok], lp['y'].cpu().numpy()[:, ok]
    res['outlet_fused_vs_loop_worst'] = float(np.max(np.abs(ya - yb) / (1e-7 * np.abs(yb) + 1e-14)))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='10000,262144')
    ap.add_argument('--cells', default='8,32')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    import torch
    import pycatkin_amd as P
    for n in (int(x) for x in a.sizes.split(',')):
        for cells in (int(x) for x in a.cells.split(',')):
            run(P, torch, n, cells, a)


if __name__ == '__main__':
    main()
