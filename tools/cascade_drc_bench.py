"""Time the bed DRC (pck_cascade_drc_at / pck_cascade_drc,
csrc/mk_cascade_adjoint.h) against the bed solve it follows.

  Pd111 (examples/COOxReactor), temperatures 423-623 K, `cells` in --cells,
  n in --sizes, K = 1 (the bed-mean TOF) and K = 3 (TOF, outlet CO, outlet CO2)

Three things per (n, cells, K), inputs resident on the device:
  adjoint   DeviceNetwork.cascade_drc_at at the cell states of a solve (the
            kernel k_bed_adjoint, its workspace allocation and its outputs)
  drc       DeviceNetwork.cascade_drc (pck_cascade_drc: solve, then adjoint)
  solve     DeviceNetwork.solve_cascade(profile=False) with the same parameters
and one line with cells = 1 at --sizes' first size against the one-lane
multi-objective kernel (drc_multi_at, set_multi_lanes(ONE)): the cost of the
cell loop's bookkeeping.

One GPU, HIP events around `reps` back-to-back calls, the three alternated in
the same process, the median of `--rounds` rounds with the spread, after a
warm-up of every shape.  Prints one JSON line per row.  Needs the GPU.

    python tools/cascade_drc_bench.py [--sizes 10000,262144] [--cells 8,32] [--rounds 5]
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


def pd111(P, reactor):
    s = P.read_from_input_file(os.path.join(INPUTS, 'COOxReactor', 'input_Pd111.json'))
    s.add_reactor(reactor)
    s._plans.clear()
    return s


def objectives(plan, K):
    wr, wy = np.zeros((K, len(plan.reactions))), np.zeros((K, len(plan.dyn)))
    wr[0, plan.reactions.index('CO_ox')] = 1.0
    for m, name in enumerate(('CO', 'CO2')[:K - 1]):
        wy[m + 1, plan.dyn.index(name)] = 1.0
    return wr, wy


def timed(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps            # ms per call


def measure(torch, todo, a):
    for _, fn in todo:                             # warm-up: hipRTC, the memory pool
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k, _ in todo}
    for _ in range(a.rounds):
        for k, fn in todo:
            ms[k].append(timed(torch, fn, a.reps))
    res = {}
    for k, v in ms.items():
        res[k + '_ms'] = round(float(np.median(v)), 4)
        res[k + '_ms_min_max'] = [round(float(min(v)), 4), round(float(max(v)), 4)]
    return res


def setup(P, torch, n, cells):
    from pycatkin_amd.classes.system import ROOT_DIST, SCREEN_MARGIN, SCREEN_RTOL, STEADY_TRANSIENT
    s = pd111(P, P.PFReactor(cells=cells, **BED) if cells > 1 else P.CSTReactor(**BED))
    plan, net = s.plan(()), s.device(())
    f64 = dict(dtype=torch.float64, device='cuda')
    T = torch.linspace(423.0, 623.0, n, **f64)
    _, p, d, fx, y0, inflow = s._inputs(net, plan, n, None, None, None, None, None, None)
    y0, inflow = torch.as_tensor(y0, **f64), torch.as_tensor(inflow, **f64)
    times = s.params['times'] or [0.0, 1.0e4]
    kw = dict(t0=times[0], t_end=times[-1], rtol=STEADY_TRANSIENT[0], atol=STEADY_TRANSIENT[1], max_steps=200000,
              newton=True, root_dist=ROOT_DIST, screen=(SCREEN_RTOL, SCREEN_MARGIN), wave_order=-1)
    return s, plan, net, (T, p, d, fx, y0, inflow), kw


def run(P, torch, n, cells, K, a):
    s, plan, net, (T, p, d, fx, y0, inflow), kw = setup(P, torch, n, cells)
    wr, wy = objectives(plan, K)
    wr, wy = torch.as_tensor(wr, dtype=torch.float64, device='cuda'), torch.as_tensor(wy, dtype=torch.float64, device='cuda')
    base = net.solve_cascade(n, T, p, y0, cells, d, fx, inflow, profile=True, want_k=True, **kw)
    state = {}

    def adjoint():
        state['adjoint'] = net.cascade_drc_at(n, T, p, base['y_cells'], base['kf'], base['kr'], wr, wy, d, fx, inflow,
                                              base['status_cells'])

    def drc():
        state['drc'] = net.cascade_drc(n, T, p, y0, cells, wr, wy, d, fx, inflow, **kw)

    def solve():
        state['solve'] = net.solve_cascade(n, T, p, y0, cells, d, fx, inflow, profile=False, **kw)

    res = dict(workload='pd111_cascade_drc', conditions=n, cells=cells, K=K)
    res.update(measure(torch, [('adjoint', adjoint), ('drc', drc), ('solve', solve)], a))
    res['adjoint_over_solve'] = round(res['adjoint_ms'] / res['solve_ms'], 4)
    st = state['drc']['status'].cpu().numpy()
    res['drc_status_counts'] = {int(q): int(c) for q, c in zip(*np.unique(st, return_counts=True))}
    ok = st == 0
    xa, xb = state['adjoint']['xi'].cpu().numpy()[..., ok], state['drc']['xi'].cpu().numpy()[..., ok]
    res['xi_at_vs_drc_max_abs'] = float(np.max(np.abs(xa - xb))) if ok.any() else None
    print(json.dumps(res), flush=True)


def run_one_cell(P, torch, n, K, a):
    from pycatkin_amd import _lib as L
    s, plan, net, (T, p, d, fx, y0, inflow), kw = setup(P, torch, n, 1)
    wr, wy = objectives(plan, K)
    base = net.solve_cascade(n, T, p, y0, 1, d, fx, inflow, profile=True, want_k=True, **kw)
    net.set_multi_lanes(L.SENS_LANES_ONE)
    y = base['y_cells'][0].contiguous()
    st = base['status_cells'][0].contiguous()

    def bed():
        net.cascade_drc_at(n, T, p, base['y_cells'], base['kf'], base['kr'], wr, wy, d, fx, inflow, base['status_cells'],
                           want_order_in=False)

    def tank():
        net.drc_multi_at(n, T, p, y, base['kf'], base['kr'], wr, wy, d, fx, inflow, st)

    res = dict(workload='pd111_cascade_drc_one_cell', conditions=n, cells=1, K=K)
    res.update(measure(torch, [('bed_adjoint', bed), ('lane_multi_adjoint', tank)], a))
    res['bed_over_tank'] = round(res['bed_adjoint_ms'] / res['lane_multi_adjoint_ms'], 4)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='10000,262144')
    ap.add_argument('--cells', default='8,32')
    ap.add_argument('--objectives', default='1,3')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    import torch
    import pycatkin_amd as P
    sizes = [int(x) for x in a.sizes.split(',')]
    for K in (int(x) for x in a.objectives.split(',')):
        run_one_cell(P, torch, sizes[0], K, a)
    for n in sizes:
        for cells in (int(x) for x in a.cells.split(',')):
            for K in (int(x) for x in a.objectives.split(',')):
                run(P, torch, n, cells, K, a)


if __name__ == '__main__':
    main()
