"""Time the adjoint sensitivities (pck_sens_at / pck_sens_adjoint, csrc/mk_sens.h:
k_sens_adjoint) against the analytic degree of rate control they extend
(pck_drc_at: k_drc_adjoint) on the same inputs, and the whole
sensitivity_batch(eapp=True) path against the steady solve it starts with.

Workloads as tools/drc_adjoint_bench.py: dmtm (64 x 64 grid), syn24 (4 096
conditions), volcano (1024 x 1024 grid); cstr (the Pd111 CSTR, a sweep of 10 000
temperatures 423 .. 623 K; its Eapp is refused -- the row scale depends on T -- so
its direction is the fixed a = c = 1).  --adjoint-kernel group | lane picks the
adjoint kernels (csrc/mk_sens.h over csrc/mk_adjoint.h / csrc/mk_sens_lane.h; lane: networks of at
most 8 dynamic species).  Per workload, on the current stream:
  solve       pck_solve alone (System.sensitivity_batch's settings)
  drc_at      pck_drc_at at the solve's states: k_drc_adjoint alone
  sens_at     pck_sens_at at the same states, every output, one direction
              (d ln k / dT): k_sens_adjoint alone
  sens_xi     pck_sens_at asked for what pck_drc_at gives only (no sf / sr /
              order / dir / err outputs): the price of the shared body
  dlnk        the four pck_rate_constants launches and the logarithms of the stencil
  eapp_batch  dlnk + pck_sens_adjoint (solve + k_sens_adjoint): sensitivity_batch(eapp=True)

HIP events around `reps` back-to-back calls, the median of `--rounds` rounds
with the spread.  Prints one JSON line per workload.  Needs the GPU.

    python tools/sens_adjoint_bench.py [--workloads dmtm,syn24,volcano,cstr] [--rounds 5]
                                       [--adjoint-kernel group|lane]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def run(name, sim, terms, kw, n, a, torch):
    from pycatkin_amd import _lib as L
    from pycatkin_amd.engine import _ptr, _stream
    from pycatkin_amd.classes.system import (ROOT_DIST, SCREEN_MARGIN, SCREEN_MAX_LANE_SPECIES, SCREEN_RTOL,
                                             STEADY_TRANSIENT)
    plan, net = sim.plan(terms), sim.device(terms)
    net.set_sens_lanes(L.SENS_LANES_MODES[a.adjoint_kernel])
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

    def drc_at():
        state['t'] = net.drc_at(n, T, p, state['s']['y'], kf, kr, d, fx, inflow, state['s']['status'])

    def dlnk():
        if name == 'cstr':
            state['k'] = (torch.ones_like(kf), torch.ones_like(kr))
        else:
            state['k'] = sim._dlnk_dT(net, n, T, p, d)

    def sens_at():
        state['e'] = net.sens_at(n, T, p, state['s']['y'], kf, kr, d, fx, inflow, state['s']['status'],
                                 directions=state['k'])

    xi = torch.zeros((net.NRXN, n), dtype=torch.float64, device='cuda')
    tof0 = torch.empty(n, dtype=torch.float64, device='cuda')
    st = torch.empty(n, dtype=torch.int32, device='cuda')

    def sens_xi():
        c, keep = net.conditions(n, T, p, d, fx, None, inflow)
        o = L.SensOut()
        o.xi, o.ld_xi, o.tof0, o.status = _ptr(xi), n, _ptr(tof0), _ptr(st)
        L.check(net.lib.pck_sens_at(net.h, C.byref(c), _ptr(kf), _ptr(kr), n, _ptr(state['s']['y']), n,
                                    _ptr(state['s']['status']), None, 0.0, C.byref(o), _stream(torch)))

    def eapp_batch():
        dlnk()
        state['b'] = net.sens_adjoint(n, T, p, y0, d, fx, inflow, directions=state['k'], **prm)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps          # ms per call

    todo = [('solve', solve), ('drc_at', drc_at), ('dlnk', dlnk), ('sens_at', sens_at), ('sens_xi', sens_xi),
            ('eapp_batch', eapp_batch)]
    for _, fn in todo:                             # warm-up (hipRTC compiles, the memory pool)
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k, _ in todo}
    for _ in range(a.rounds):
        for k, fn in todo:
            ms[k].append(timed(fn, a.reps))
    res = dict(workload=name, adjoint_kernel=a.adjoint_kernel, lanes_per_condition=net.sens_lanes(), conditions=n, species=net.NDYN, reactions=net.NRXN, fixed=net.NFIX)
    for k, v in ms.items():
        res[k + '_ms'] = round(float(np.median(v)), 4)
        res[k + '_ms_min_max'] = [round(float(min(v)), 4), round(float(max(v)), 4)]
    res['sens_at_over_drc_at'] = round(res['sens_at_ms'] / res['drc_at_ms'], 3)
    res['sens_xi_over_drc_at'] = round(res['sens_xi_ms'] / res['drc_at_ms'], 3)
    res['eapp_batch_over_solve'] = round(res['eapp_batch_ms'] / res['solve_ms'], 3)
    sb = state['b']['status'].cpu().numpy()
    res['eapp_batch_status_counts'] = {int(k): int(v) for k, v in zip(*np.unique(sb, return_counts=True))}
    same = torch.equal(torch.nan_to_num(state['e']['xi']), torch.nan_to_num(state['t']['xi'])) and \
        torch.equal(torch.nan_to_num(xi), torch.nan_to_num(state['t']['xi']))
    res['xi_bitwise_equal_to_drc_at'] = bool(same)
    print(json.dumps(res), flush=True)


def cstr(P, n):
    sim = P.read_from_input_file(os.path.join(ROOT, 'tests', 'golden', 'inputs', 'COOxReactor', 'input_Pd111.json'))
    return sim, ('CO_ox',), dict(T=np.linspace(423.0, 623.0, n)), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workloads', default='dmtm,syn24,volcano')
    ap.add_argument('--dmtm-grid', type=int, default=64)
    ap.add_argument('--volcano-grid', type=int, default=1024)
    ap.add_argument('--syn24-n', type=int, default=4096)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--cstr-n', type=int, default=10000)
    ap.add_argument('--adjoint-kernel', choices=('group', 'lane'), default='group')
    a = ap.parse_args()
    import torch
    import pycatkin_amd as P
    import drc_adjoint_bench as B
    size = dict(dmtm=a.dmtm_grid, volcano=a.volcano_grid, syn24=a.syn24_n, cstr=a.cstr_n)
    for name in a.workloads.split(','):
        sim, terms, kw, n = dict(dmtm=B.dmtm, volcano=B.volcano, syn24=B.syn24, cstr=cstr)[name](P, size[name])
        run(name, sim, terms, kw, n, a, torch)


if __name__ == '__main__':
    main()
