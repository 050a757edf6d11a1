"""Time pck_energy_span against its floor, pck_energies on the same plan.

Workload: the DMTM 'full_pes' landscape (20 entries, 7 TS) on a T x p grid
(default 1024 x 1024 = 1 048 576 conditions, T 400..800 K, p 1e4..1e6 Pa).

  span      one pck_energy_span launch writing tof, espan, i_tdts, i_tdi
  energies  one pck_energies launch on the same network: the same thermo
            features and energy program, every register written, no span

Each is warmed up, then timed with device events around `--reps` back-to-back
launches, alternating the two, `--rounds` times; the median round is reported
with the spread.  Prints one JSON line.  Needs the GPU: there is no fallback.

    python tools/espan_bench.py [--grid 1024] [--reps 20] [--rounds 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grid', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()

    import torch
    import pycatkin_amd as P
    from pycatkin_amd import _lib as L
    from pycatkin_amd.engine import _ptr, _stream
    sim = P.read_from_input_file(os.path.join(ROOT, 'tests', 'golden', 'inputs', 'DMTM', 'input.json'))
    pes = sim.energy_landscapes['full_pes']
    net, regs, dnames = pes._device()
    assert not dnames
    g = a.grid
    n = g * g
    T = torch.linspace(400.0, 800.0, g, dtype=torch.float64, device='cuda').repeat_interleave(g).contiguous()
    p = torch.logspace(4.0, 6.0, g, dtype=torch.float64, device='cuda').repeat(g).contiguous()
    cond, keep = net.conditions(n, T, p)
    ls = L.Landscape()
    ls.n_pts = len(regs['free'])
    for k, (r, t) in enumerate(zip(regs['free'], pes.is_ts())):
        ls.reg[k] = r
        ls.ts_mask |= int(t) << k
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device='cuda')
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device='cuda')
    outs = dict(tof=f64(n), espan=f64(n), i_tdts=i32(n), i_tdi=i32(n))
    o = L.SpanOutputs()
    for k, t in outs.items():
        setattr(o, k, _ptr(t))
    o.ld_x = o.ld_e = n
    ereg = f64(net.NREG, n)
    stream = _stream(torch)

    def span():
        L.check(net.lib.pck_energy_span(net.h, C.byref(cond), C.byref(ls), C.byref(o), stream))

    def energies():
        L.check(net.lib.pck_energies(net.h, C.byref(cond), _ptr(ereg), n, stream))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.reps          # ms per launch

    for _ in range(a.warmup):
        span()
        energies()
    torch.cuda.synchronize()
    ts, te = [], []
    for _ in range(a.rounds):
        ts.append(timed(span))
        te.append(timed(energies))
    # the two launches agree on what they share: the landscape's last energy is dgrxn's register
    chk = net.energy_span(4096, T[:4096], p[:4096], (regs['free'], pes.is_ts()), want=('tof', 'energy'))
    ref = net.energies(4096, T[:4096], p[:4096])
    same = bool(torch.equal(chk['energy'][-1], ref[regs['free'][-1]] - ref[regs['free'][0]]))
    ms_s, ms_e = float(np.median(ts)), float(np.median(te))
    print(json.dumps(dict(workload='DMTM full_pes', conditions=n, nfeat=net.nfeat, nreg=net.NREG,
                          span_ms=round(ms_s, 4), span_ms_min_max=[round(min(ts), 4), round(max(ts), 4)],
                          energies_ms=round(ms_e, 4), energies_ms_min_max=[round(min(te), 4), round(max(te), 4)],
                          span_conditions_per_s=round(n / (ms_s * 1e-3), 1),
                          energies_conditions_per_s=round(n / (ms_e * 1e-3), 1),
                          span_over_energies=round(ms_s / ms_e, 3), energies_agree=same,
                          tof_finite=bool(torch.isfinite(outs['tof']).all()))))


if __name__ == '__main__':
    main()
