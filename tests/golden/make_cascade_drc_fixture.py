"""Fixture of the bed DRC (csrc/mk_cascade_adjoint.h: pck_cascade_drc_at): the
backward adjoint sweep of tests/_sens_cascade.py in mpmath at the stored cell
states of cascade_fixture.npz, and a check of that formula against central
differences of the oracle's own march.  CPU only; the tests read the .npz alone.

Cases: the COOxReactor Pd111 bed (NS 6; the site balance sits in an adsorbate
row, a row without flow, so the replaced-row path of phi and w is exercised) as
1, 2 and 8 cells (make_cascade_fixture.py: cell_spec), start 'system', at
  548.0 K   both the 2- and the 8-cell bed ignited
  498.0 K   the poisoned side
  448.0 K, 598.0 K
Every cell of every case is `regular` and `ref_ok` in cascade_fixture.npz
(asserted), and no temperature lies within one grid step (12.5 K) of the
ignition jump at 535.5 K, where the derivative is not defined across the fold
(asserted; the finite-difference check below would fail there as well).

Objectives per case: the bed-mean TOF (CO_ox); the outlet concentration of
every gas species; one weighted mix (TOF + 2 x outlet CO2 + 0.5 x outlet CO; no
quasi-equilibrated step in it: the net rate of CO_ads at a float root carries
the rounding of forward and reverse rates 1e9 times larger, which the
finite-difference check would measure instead of the formula).  An objective
is turned down, and recorded in `dropped`, by the rules of
make_drc_multi_lane_fixture.py: its 400- and 800-bit runs disagree, a rate
objective's value has no digits (below 1e-6 of the largest net rate), or the
104-bit run misses TOL_104 (1 + |xi_ref|).  Asserted: the TOF objective and at
least one outlet objective survive in every case.

Not in the fixture: an NS = 8 case (tests/_synth.py's networks have no product
gas, so a steady bed of them converts nothing and its TOF is zero: there is no
derivative for the finite-difference check; the kernel's NS = 8 path is checked
at generic states in tests/test_gpu_cascade_drc.py) and a case with a pinned
species or a conservation law pivoting in a flow row (DESIGN.md "Bed DRC").

Per case `c<i>_...` (name in `names[i]`):
  T, cells, y_cells [cells, NS] (dyn order), y_full [cells, n_species], kf, kr,
  inflow [NS], labels, wr [K, R], wy [K, NS], dropped
  val_ref [K], xi_ref [K, R], order_in_ref [K, NS]   400 bits, equal to an 800-bit run
  xi_104, order_in_104                               the same at 104 bits
  fd_ratio     worst |xi_fd(eps) - xi_ref| / (10 |xi_fd(eps) - xi_fd(2 eps)| + 1e-9 (1 + |xi_ref|))
and `dyn`, `rnames`, `species`, `fd_eps`, `fd_ratio` (the worst over the cases).

The formula itself is asserted.  For every case and every surviving objective
each (kf_j, kr_j) is scaled by 1 +- eps at fixed K_j, every cell is solved again
with the oracle's Newton from the stored root with the perturbed upstream
cell's gas as its inflow, and the central difference of ln J is compared with
xi_ref; the same for the CO feed against order_in_ref.  The difference's own
error is judged from two steps: |xi_fd(eps) - xi_ref| <= 10 |xi_fd(eps) -
xi_fd(2 eps)| + 1e-9 (1 + |xi_ref|).  Every single-cell bed is asserted equal to
_sens_multi.multi_drc_mp at 400 bits to 1e-60.

    OMP_NUM_THREADS=1 python tests/golden/make_cascade_drc_fixture.py

writes tests/golden/cascade_drc_fixture.npz (numpy arrays only).
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SRC = os.path.join(HERE, 'cascade_fixture.npz')
OUT = os.path.join(HERE, 'cascade_drc_fixture.npz')
INPUT = os.path.join(HERE, 'inputs', 'COOxReactor', 'input_Pd111.json')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, HERE)

from make_cascade_fixture import cell_spec  # noqa: E402

BITS, BITS_CHECK = 400, 800
TEMPS = (548.0, 498.0, 448.0, 598.0)
CELLS = (1, 2, 8)
JUMP, GRID_STEP = 535.5, 12.5
TOF = ('CO_ox',)
TOL_104 = 1.0e-11
NO_DIGITS = 1.0e-6
FD_EPS = 1.0e-3
FEED = 'CO'


def bed_models(spec, T, y_full):
    """The cell models of a bed at the stored full states y_full [cells, n_species]."""
    from oracle import mk_oracle as O
    cells = len(y_full)
    cs = cell_spec(spec, cells)
    ms, inflow = [], None
    for c in range(cells):
        m = O.ClassicModel(cs, T=float(T), inflow_state=inflow)
        ms.append(m)
        inflow = {m.snames[i]: float(y_full[c][i]) for i in m.gas_idx}
    return ms


def objectives(m, ms, y_full, tof, mix):
    rn, dyn = list(m.rnames), [m.snames[q] for q in m.dyn]
    R, NS = len(rn), len(dyn)
    labels, wr, wy = [], [], []

    def add(label, r=None, s=None):
        a, b = np.zeros(R), np.zeros(NS)
        for k, w in (r or {}).items():
            a[rn.index(k)] += w
        for k, w in (s or {}).items():
            b[dyn.index(k)] += w
        labels.append(label), wr.append(a), wy.append(b)

    add('tof', r={t: 1.0 for t in tof})
    gases = [m.snames[i] for i in m.gas_idx]
    for g in gases:
        add('outlet[%s]' % g, s={g: 1.0})
    add('mix', r={tof[0]: 1.0}, s=mix)
    wr, wy = np.array(wr), np.array(wy)
    nets = np.array([(lambda rr: rr[:, 0] - rr[:, 1])(mc.rates(np.asarray(y, float))) for mc, y in zip(ms, y_full)])
    vals = (wr @ nets.T).mean(axis=1)
    nodigits = [labels[q] for q in range(len(labels))
                if wr[q].any() and not wy[q].any() and abs(vals[q]) < NO_DIGITS * np.abs(nets).max()]
    return labels, wr, wy, nodigits


def march(spec, T, y_full, wr, wy, scale=None, feed=None):
    """The objectives' values (float) of the oracle's own march from the stored
    roots: scale = (j, f) multiplies kf_j and kr_j by f, feed = (species, f) the
    inflow of cell 0."""
    from oracle import mk_oracle as O
    cells = len(y_full)
    cs = cell_spec(spec, cells)
    inflow, nets, y = None, [], None
    for c in range(cells):
        m = O.ClassicModel(cs, T=float(T), inflow_state=inflow)
        if c == 0 and feed is not None:
            m.yin[m.idx[feed[0]]] *= feed[1]
        if scale is not None:
            m.kf[scale[0]] *= scale[1]
            m.kr[scale[0]] *= scale[1]
        y = m.find_steady(np.array(y_full[c], float))
        assert m.regular, (T, cells, c, scale, feed)
        rr = m.rates(y)
        nets.append(rr[:, 0] - rr[:, 1])
        inflow = {m.snames[i]: float(y[i]) for i in m.gas_idx}
    return wr @ np.mean(nets, axis=0) + wy @ y[list(m.dyn)]


def fd(spec, T, y_full, wr, wy, eps, **which):
    k, v = next(iter(which.items()))
    a = march(spec, T, y_full, wr, wy, **{k: (v, 1.0 + eps)})
    b = march(spec, T, y_full, wr, wy, **{k: (v, 1.0 - eps)})
    return (a - b) / (2.0 * eps * march(spec, T, y_full, wr, wy))


def do_case(name, spec, T, y_full, tof, mix, feed, t0):
    """One case: references, the turned-down objectives, the checks -> its entries."""
    import mpmath
    import _sens_cascade as SC
    import _sens_multi as SM
    cells = len(y_full)
    ms = bed_models(spec, T, y_full)
    m = ms[0]
    labels, wr, wy, nodigits = objectives(m, ms, y_full, tof, mix)
    obj = list(zip(wr, wy))
    xi4, v4, o4 = SC.cascade_drc_mp(ms, y_full, obj, BITS)
    xi8, v8, o8 = SC.cascade_drc_mp(ms, y_full, obj, BITS_CHECK)
    xl, _, ol = SC.cascade_drc_mp(ms, y_full, obj, 104)
    f = lambda rows: np.array([[float(x) for x in r] for r in rows])
    ref, oref, lo, olo = f(xi4), f(o4), f(xl), f(ol)
    if cells == 1:
        xm, vm = SM.multi_drc_mp(m, y_full[0], obj, BITS)
        with mpmath.workprec(BITS_CHECK):
            big = max(abs(x) for r in xm for x in r)
            assert all(abs(a - b) <= mpmath.mpf(10) ** -60 * (abs(b) + big)
                       for ra, rb in zip(xi4, xm) for a, b in zip(ra, rb)), name
            assert all(abs(a - b) <= mpmath.mpf(10) ** -60 * abs(b) for a, b in zip(v4, vm)), name
    keep, dropped = [], []
    for q, label in enumerate(labels):
        with mpmath.workprec(BITS_CHECK):
            big = max(abs(x) for x in xi8[q])
            agree = all(abs(a - b) <= mpmath.mpf(10) ** -60 * (abs(b) + mpmath.mpf(10) ** -40 * big)
                        for a, b in zip(list(xi4[q]) + list(o4[q]), list(xi8[q]) + list(o8[q])))
        d104 = max(np.max(np.abs(lo[q] - ref[q]) / (1.0 + np.abs(ref[q]))),
                   np.max(np.abs(olo[q] - oref[q]) / (1.0 + np.abs(oref[q]))))
        why = ('400 and 800 bits disagree' if not agree else 'net rate without digits' if label in nodigits
               else '104 bits off by %.1e' % d104 if not d104 <= TOL_104 else None)
        if why:
            dropped.append(label)
            print('  %s: %s turned down (%s)' % (name, label, why), flush=True)
        else:
            keep.append(q)
    kept = [labels[q] for q in keep]
    assert 'tof' in kept and any(lb.startswith('outlet[') for lb in kept), (name, dropped)
    # the formula against central differences of the oracle's own march
    wk, yk = wr[keep], wy[keep]
    R = len(m.rnames)
    fd1 = np.stack([fd(spec, T, y_full, wk, yk, FD_EPS, scale=j) for j in range(R)], axis=1)
    fd2 = np.stack([fd(spec, T, y_full, wk, yk, 2.0 * FD_EPS, scale=j) for j in range(R)], axis=1)
    bound = 10.0 * np.abs(fd1 - fd2) + 1.0e-9 * (1.0 + np.abs(ref[keep]))
    ratio = float(np.max(np.abs(fd1 - ref[keep]) / bound))
    assert ratio <= 1.0, (name, ratio, fd1, ref[keep])
    a = [m.snames[q] for q in m.dyn].index(feed)
    g1 = fd(spec, T, y_full, wk, yk, FD_EPS, feed=feed)
    g2 = fd(spec, T, y_full, wk, yk, 2.0 * FD_EPS, feed=feed)
    gb = 10.0 * np.abs(g1 - g2) + 1.0e-9 * (1.0 + np.abs(oref[keep][:, a]))
    ratio = max(ratio, float(np.max(np.abs(g1 - oref[keep][:, a]) / gb)))
    assert ratio <= 1.0, (name, ratio, g1, oref[keep][:, a])
    o = dict(T=np.array(T), cells=np.array(cells), y_cells=y_full[:, list(m.dyn)], y_full=y_full, kf=m.kf, kr=m.kr,
             inflow=m.yin[list(m.dyn)], labels=np.array(kept), wr=wk, wy=yk,
             val_ref=np.array([float(v4[q]) for q in keep]), xi_ref=ref[keep], order_in_ref=oref[keep],
             xi_104=lo[keep], order_in_104=olo[keep], dropped=np.array(dropped, dtype=str),
             fd_ratio=np.array(ratio), dyn=np.array([m.snames[q] for q in m.dyn]), rnames=np.array(list(m.rnames)),
             species=np.array(m.snames))
    d = np.abs(o['xi_104'] - o['xi_ref']) / (1.0 + np.abs(o['xi_ref']))
    print('%-16s K %d (%d turned down)  |104 - ref| / (1 + |ref|) %.1e  fd ratio %.2e  sums %s  (%.0f s)'
          % (name, len(keep), len(dropped), d.max(), ratio,
             ' '.join('%.3g' % s for s in o['xi_ref'].sum(axis=1)), time.time() - t0), flush=True)
    return o


def main():
    from oracle import mk_oracle as O
    src = np.load(SRC)
    spec = O.load_spec(INPUT)
    grid = list(src['T'])
    out, names = {}, []
    t0 = time.time()

    def store(name, o):
        for k, v in o.items():
            out['c%d_%s' % (len(names), k)] = v
        names.append(name)

    for T in TEMPS:
        assert abs(T - JUMP) >= GRID_STEP, T
        ti = grid.index(T)
        for cells in CELLS:
            tag = 'c%d_system' % cells
            assert src['ref_ok_' + tag][ti] and src['regular_' + tag][ti].all(), (T, cells)
            y_full = np.array(src['y_' + tag][ti], float)
            store('pd111_T%g_c%d' % (T, cells),
                  do_case('pd111_T%g_c%d' % (T, cells), spec, T, y_full, TOF, {'CO2': 2.0, 'CO': 0.5}, FEED, t0))
    nolet = [n for i, n in enumerate(names) if any(str(x).startswith('outlet[') for x in out['c%d_dropped' % i])]
    print('cases that lost an outlet objective:', nolet)
    assert len(nolet) <= 1
    worst_fd = max(float(out['c%d_fd_ratio' % i]) for i in range(len(names)))
    out['names'] = np.array(names)
    out['dyn'] = out['c0_dyn']
    out['rnames'] = out['c0_rnames']
    out['species'] = out['c0_species']
    out['fd_eps'] = np.array(FD_EPS)
    out['fd_ratio'] = np.array(worst_fd)
    np.savez_compressed(OUT, **out)
    print('wrote %s (%d cases, %d bytes, worst fd ratio %.2e, %.0f s)'
          % (OUT, len(names), os.path.getsize(OUT), worst_fd, time.time() - t0))


if __name__ == '__main__':
    main()
