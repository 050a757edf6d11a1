"""Fixture of the one-lane multi-objective analytic degree of rate control
(csrc/mk_sens_multi_lane.h: k_lane_multi_adjoint): the formula of
tests/_sens_multi.py in mpmath at the stored states and rate constants of
lane_sens_fixture.npz.  CPU only; the GPU tests read the two .npz alone.

The volcano (NS 4) and CSTR (NS 6) cases of drc_multi_fixture.npz are the
kernel's references as they stand.  This fixture adds the cases l3_0/1, l7_0/1,
l8_0/1 (NS 3, 7 and 8 -- the kernel's limit --, two roots each) and pin_0 (a
pinned species) of lane_sens_fixture.npz.  The models are rebuilt from
make_lane_sens_fixture.lane_net and the stored descriptors; their kf / kr are
asserted equal to the stored ones.

Per case `m<i>_...` (name in `names[i]`), the layout of drc_multi_fixture.npz:
  src                  index of the case in lane_sens_fixture.npz (`n<src>_`: T,
                       p, desc, dyn, rnames, y, y_full, kf, kr, unreach are read
                       from there)
  labels               one per objective
  wr [K, R], wy [K, NS]   the objectives over the source's rnames / dyn
  val_ref, xi_ref      _sens_multi.multi_drc at 400 bits, rounded
  xi_104               the same at 104 bits
  dropped              labels of the objectives turned down (below)

Objectives of a case, by the rules of make_drc_multi_fixture.py: its own TOF
terms; 2.5 x the net rate of the best-conditioned reaction outside the TOF
terms (the smallest max(rf, rr) / |net|); a two-term weighted mix (the TOF terms
+ 0.5 x that reaction); every non-zero dynamic species as a coverage objective.
On l8 that is K = 11 > 8.

An objective is turned down, and recorded in `dropped`, where its 400- and
800-bit runs disagree (make_drc_multi_fixture.py's bound), where a rate
objective's net rate has no digits (below 1e-6 of the largest net rate: the
root's residual, objectives_all there), or where the 104-bit run misses
TOL_104 (1 + |xi_ref|): such an objective is conditioned beyond what any
double-double evaluation can be held to at 1e-11.  Asserted here and in
tests/test_multi_lane.py: in every l* case at most one coverage objective of a
non-zero species is missing and the TOF objective is present.

    OMP_NUM_THREADS=1 python tests/golden/make_drc_multi_lane_fixture.py

writes tests/golden/drc_multi_lane_fixture.npz (numpy arrays only).
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SRC = os.path.join(HERE, 'lane_sens_fixture.npz')
OUT = os.path.join(HERE, 'drc_multi_lane_fixture.npz')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, HERE)

from make_lane_sens_fixture import BITS, BITS_CHECK, lane_net  # noqa: E402

CASES = ('l3_0', 'l3_1', 'l7_0', 'l7_1', 'l8_0', 'l8_1', 'pin_0')
TOL_104 = 1.0e-11
NO_DIGITS = 1.0e-6
MAX_COVERAGES_MISSING = 1


def model(c):
    """The oracle model of a case of lane_sens_fixture.npz (c: its entries)."""
    from _synth import spec_of
    from oracle import mk_oracle as O
    names = [str(k) for k in c['desc_names']]
    d = np.array([float(c['desc'][names.index('D%d' % k)]) for k in range(4)])
    T = float(c['T'])
    m = O.ClassicModel(spec_of(lane_net(str(c['net'])), d, T), T=T)
    unreach = np.zeros(len(m.snames), bool)
    unreach[list(m.dyn)] = np.asarray(c['unreach'], bool)
    m.unreach = unreach
    return m


def objectives(m, c):
    """labels, wr [K, R], wy [K, NS], and the rate objectives without digits"""
    rn, dyn = list(m.rnames), [m.snames[q] for q in m.dyn]
    R, NS = len(rn), len(dyn)
    y = np.asarray(c['y'], float)
    rr = m.rates(np.asarray(c['y_full'], float))
    net = rr[:, 0] - rr[:, 1]
    labels, wr, wy = [], [], []

    def add(label, r=None, s=None):
        a, b = np.zeros(R), np.zeros(NS)
        for k, w in (r or {}).items():
            a[rn.index(k)] += w
        for k, w in (s or {}).items():
            b[dyn.index(k)] += w
        labels.append(label), wr.append(a), wy.append(b)

    tof = [str(t) for t in c['tof_terms']]
    add('tof', r={t: 1.0 for t in tof})
    others = [j for j in range(R) if rn[j] not in tof and net[j] != 0.0]
    j = min(others, key=lambda q: rr[q].max() / abs(net[q]))
    add('2.5 ' + rn[j], r={rn[j]: 2.5})
    mix = {t: 1.0 for t in tof}
    mix[rn[j]] = mix.get(rn[j], 0.0) + 0.5
    add('mix', r=mix)
    for a in range(NS):
        if y[a] != 0.0:
            add('[%s]' % dyn[a], s={dyn[a]: 1.0})
    wr, wy = np.array(wr), np.array(wy)
    vals = wr @ net
    nodigits = [labels[q] for q in range(len(labels)) if wr[q].any() and abs(vals[q]) < NO_DIGITS * np.abs(net).max()]
    return labels, wr, wy, nodigits


def main():
    import mpmath
    import _sens_multi as SM
    src = dict(np.load(SRC))
    snames = [str(x) for x in src['names']]
    out, names = {}, []
    t0 = time.time()
    for i, name in enumerate(CASES):
        si = snames.index(name)
        pre = 'n%d_' % si
        c = {k[len(pre):]: v for k, v in src.items() if k.startswith(pre)}
        m = model(c)
        assert np.array_equal(m.kf, c['kf']) and np.array_equal(m.kr, c['kr']), name
        assert list(m.rnames) == [str(x) for x in c['rnames']]
        assert [m.snames[q] for q in m.dyn] == [str(x) for x in c['dyn']]
        y = np.asarray(c['y_full'], float)
        labels, wr, wy, nodigits = objectives(m, c)
        obj = list(zip(wr, wy))
        xi4, v4 = SM.multi_drc_mp(m, y, obj, BITS)
        xi8, _ = SM.multi_drc_mp(m, y, obj, BITS_CHECK)
        f = lambda rows: np.array([[float(x) for x in r] for r in rows])
        ref, lo = f(xi4), f(SM.multi_drc_mp(m, y, obj, 104)[0])
        keep, dropped = [], []
        for q, label in enumerate(labels):
            with mpmath.workprec(BITS_CHECK):
                # make_drc_multi_fixture.py's bound of the 400- against the 800-bit run
                big = max(abs(x) for x in xi8[q])
                agree = all(abs(a - b) <= mpmath.mpf(10) ** -60 * (abs(b) + mpmath.mpf(10) ** -40 * big)
                            for a, b in zip(xi4[q], xi8[q]))
            d104 = np.max(np.abs(lo[q] - ref[q]) / (1.0 + np.abs(ref[q])))
            why = ('400 and 800 bits disagree' if not agree else 'net rate without digits' if label in nodigits
                   else '104 bits off by %.1e' % d104 if not d104 <= TOL_104 else None)
            if why:
                dropped.append(label)
                print('  %s: %s turned down (%s)' % (name, label, why), flush=True)
            else:
                keep.append(q)
        if name.startswith('l'):
            cov = [lb for lb in dropped if lb.startswith('[')]
            assert len(cov) <= MAX_COVERAGES_MISSING and 'tof' not in dropped, (name, dropped)
        o = dict(src=np.array(si), labels=np.array([labels[q] for q in keep]), wr=wr[keep], wy=wy[keep],
                 val_ref=np.array([float(v4[q]) for q in keep]), xi_ref=ref[keep], xi_104=lo[keep],
                 dropped=np.array(dropped, dtype=str))
        for k, v in o.items():
            out['m%d_%s' % (i, k)] = v
        names.append(name)
        d = np.abs(o['xi_104'] - o['xi_ref']) / (1.0 + np.abs(o['xi_ref']))
        print('%-6s NS %d R %d  K %2d (%d turned down)  |104 - ref| / (1 + |ref|) %.1e  sums %s  (%.0f s)'
              % (name, len(m.dyn), len(m.rnames), len(keep), len(dropped), d.max(),
                 ' '.join('%.3g' % s for s in o['xi_ref'].sum(axis=1)), time.time() - t0), flush=True)
    out['names'] = np.array(names)
    np.savez_compressed(OUT, **out)
    print('wrote %s (%d cases, %d bytes, %.0f s)' % (OUT, len(names), os.path.getsize(OUT), time.time() - t0))


if __name__ == '__main__':
    main()
