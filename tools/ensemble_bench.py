"""Time the pieces of an uncertainty ensemble (pycatkin_amd/classes/uncertainty.py).

Workload: DMTM, 64 temperatures (400..800 K) x 4096 runs = 262 144 conditions,
sigma 0.05 eV, steady solve, TOF = r5 + r9.

  noise     one pck_ensemble_noise launch writing the [1 + n_ts, n] descriptor
            matrix, against a hipMemsetAsync of the same bytes (its floor: the
            kernel is store-bound)
  solve     one pck_solve launch over the ensemble (the matrix stays on the device)
  stats     pck_ensemble_stats of the TOF and of every dynamic species (2 launches)
  host_*    the same ensemble fed the host way: scalar np.random draws in the
            reference's order (uncertainty.py:35-65) for the 4096 runs, the
            matrix tiled and uploaded, and np.mean / np.std per temperature on
            the downloaded TOF / coverages -- wall clock, device idle before
            and after

Device pieces: HIP events around `reps` back-to-back launches, the median of
`--rounds` rounds with the spread.  Prints one JSON line.  Needs the GPU.

    python tools/ensemble_bench.py [--temps 64] [--runs 4096] [--rounds 5]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--temps', type=int, default=64)
    ap.add_argument('--runs', type=int, default=4096)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--solve-reps', type=int, default=2)
    a = ap.parse_args()

    import torch
    import pycatkin_amd as P
    from pycatkin_amd.classes.system import ROOT_DIST, STEADY_TRANSIENT
    from pycatkin_amd.engine import _stream, ensemble_noise, ensemble_stats
    sim = P.read_from_input_file(os.path.join(ROOT, 'tests', 'golden', 'inputs', 'DMTM', 'input.json'))
    unc = P.Uncertainty(sys=sim, mu=0.0, sigma=0.05, nruns=a.runs)
    terms = ('r5', 'r9')
    ens = unc._ensemble()
    plan, net = ens.plan(terms), ens.device(terms)
    n_rep, B = a.temps, a.runs
    n = n_rep * B
    D = len(plan.descriptors)
    Th = np.repeat(np.linspace(400.0, 800.0, n_rep), B)
    T = torch.as_tensor(Th, device='cuda')
    desc = torch.empty((D, n), dtype=torch.float64, device='cuda')
    _, p, _, fxc, y0, inflow = ens._inputs(net, plan, n, Th, None, desc, None, None, None)
    times = ens.params['times'] or [0.0, 1.0e4]
    out = dict(y=torch.empty((net.NDYN, n), dtype=torch.float64, device='cuda'),
               tof=torch.empty(n, dtype=torch.float64, device='cuda'),
               status=torch.empty(n, dtype=torch.int32, device='cuda'),
               nsteps=torch.empty(n, dtype=torch.int32, device='cuda'))
    hip = C.CDLL('libamdhip64.so.7')            # the runtime torch has loaded (pycatkin_amd/_lib.py: load)
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    stream = _stream(torch)

    def noise():
        ensemble_noise(7, B, n_rep, D - 1, False, unc.mu, unc.sigma, 0, out=desc)

    def memset():
        assert hip.hipMemsetAsync(desc.data_ptr(), 0, desc.numel() * 8, stream) == 0

    def solve():
        net.solve(n, T, p, y0, desc, fxc, inflow, out=out, t0=times[0], t_end=times[-1], rtol=STEADY_TRANSIENT[0],
                  atol=STEADY_TRANSIENT[1], max_steps=200000, newton=True, newton_iters=60, root_dist=ROOT_DIST)

    def stats():
        return (ensemble_stats(out['tof'], out['status'], (0, 4), B, 0),
                ensemble_stats(out['y'], out['status'], (0, 4), B, 0))

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps          # ms per call

    memset()
    noise()
    solve()
    stats()
    torch.cuda.synchronize()
    ms = dict(noise=[], memset=[], solve=[], stats=[])
    for _ in range(a.rounds):
        ms['memset'].append(timed(memset, a.reps))
        ms['noise'].append(timed(noise, a.reps))
        ms['solve'].append(timed(solve, a.solve_reps))
        ms['stats'].append(timed(stats, a.reps))
    s_tof, s_y = stats()
    torch.cuda.synchronize()

    # the host way, once per round: draws, upload, download + numpy statistics
    host = dict(draw=[], upload=[], stats=[])
    names = unc.descriptor_names()
    for _ in range(a.rounds):
        np.random.seed(7)
        t0 = time.perf_counter()
        d = unc._desc_of(unc.sample_noises(B, rng='numpy'), B)
        t1 = time.perf_counter()
        up = torch.as_tensor(np.tile(np.stack([d[k] for k in names]), (1, n_rep)), device='cuda')
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        tof, y, st = out['tof'].cpu().numpy(), out['y'].cpu().numpy(), out['status'].cpu().numpy()
        okc = np.isin(st, (0, 4)).reshape(n_rep, B)
        h_mean = np.array([tof.reshape(n_rep, B)[c][okc[c]].mean() for c in range(n_rep)])
        h_std = np.array([tof.reshape(n_rep, B)[c][okc[c]].std() for c in range(n_rep)])
        for q in range(y.shape[0]):
            for c in range(n_rep):
                v = y[q].reshape(n_rep, B)[c][okc[c]]
                v.mean(), v.std()
        t3 = time.perf_counter()
        host['draw'].append((t1 - t0) * 1e3)
        host['upload'].append((t2 - t1) * 1e3)
        host['stats'].append((t3 - t2) * 1e3)
        assert up.shape == desc.shape
    st = out['status'].cpu().numpy()
    med = lambda v: round(float(np.median(v)), 4)
    span = lambda v: [round(float(min(v)), 4), round(float(max(v)), 4)]
    res = dict(workload='DMTM uncertainty ensemble', temperatures=n_rep, runs=B, conditions=n, descriptors=D,
               desc_bytes=int(desc.numel() * 8))
    for k, v in ms.items():
        res[k + '_ms'], res[k + '_ms_min_max'] = med(v), span(v)
    for k, v in host.items():
        res['host_' + k + '_ms'], res['host_' + k + '_ms_min_max'] = med(v), span(v)
    res['noise_over_memset'] = round(res['noise_ms'] / res['memset_ms'], 3)
    res['noise_GBps'] = round(desc.numel() * 8 / (res['noise_ms'] * 1e-3) / 1e9, 1)
    res['solve_conditions_per_s'] = round(n / (res['solve_ms'] * 1e-3), 1)
    res['status_counts'] = {int(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))}
    res['stats_match_numpy'] = bool(np.allclose(s_tof['mean'].cpu().numpy(), h_mean, rtol=1e-12)
                                    and np.allclose(s_tof['std'].cpu().numpy(), h_std, rtol=1e-10))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
