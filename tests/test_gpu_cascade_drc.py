"""Bed DRC on the device (pck_cascade_drc_at / pck_cascade_drc,
System.cascade_drc_at / cascade_drc_batch; csrc/mk_cascade_adjoint.h) against
the arbitrary-precision fixture tests/golden/cascade_drc_fixture.npz
(make_cascade_drc_fixture.py, whose formula is checked against finite
differences of the oracle's march), against the one-lane multi-objective kernel
for a bed of one cell, end to end behind the fused cascade solve, and its gate,
batch independence and refusals.

Bounds.  At the fixture's states: 1e-12 + 1e-12 |ref| + 10 |xi_104 - ref|, the
shape of tests/test_gpu_multi_lane.py (double-double carries ~104 bits).  End to
end: 2 |xi_pert - xi_ref| + 1e-10 |ref|, xi_pert the restatement at the device's
own cell states at 104 bits, which prices the root error in, as
tests/test_gpu_drc_adjoint.py does.  Worst ratios seen: DESIGN.md "Bed DRC"."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')
sys.path.insert(0, HERE)
sys.path.insert(0, GOLD)

BED = dict(residence_time=4.5, volume=1.8e-7, catalyst_area=3.82e-9)   # COOxReactor/input_Pd111.json
TOF = ('CO_ox',)
ST_NEWTON, ST_SENS_SINGULAR = 4, 7


@pytest.fixture(scope='module')
def P():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    import pycatkin_amd
    return pycatkin_amd


@pytest.fixture(scope='module')
def fx():
    return np.load(os.path.join(GOLD, 'cascade_drc_fixture.npz'))


def cases(fx, cells):
    out = []
    for i in range(len(fx['names'])):
        pre = 'c%d_' % i
        c = {k[len(pre):]: fx[k] for k in fx.files if k.startswith(pre)}
        if int(c['cells']) == cells:
            out.append(c)
    return out


def pd111(P, inputs, reactor):
    s = P.read_from_input_file(os.path.join(inputs, 'COOxReactor', 'input_Pd111.json'))
    s.add_reactor(reactor)
    s._plans.clear()
    return s


def bed(P, inputs, cells):
    return pd111(P, inputs, P.PFReactor(cells=cells, **BED))


def tiled(fx, s, cs, n):
    """Keyword arguments of System.cascade_drc_at for n conditions, condition i
    the case cs[i % len(cs)], in the plan's species and reaction order."""
    plan = s.plan(())
    dyn, rn = [str(x) for x in fx['dyn']], [str(x) for x in fx['rnames']]
    sp, rx = [dyn.index(a) for a in plan.dyn], [rn.index(a) for a in plan.reactions]
    pick = [cs[i % len(cs)] for i in range(n)]
    return dict(Y_cells=np.stack([c['y_cells'][:, sp] for c in pick], axis=2),
                T=np.array([float(c['T']) for c in pick]),
                inflow=np.stack([c['inflow'][sp] for c in pick], axis=1),
                k=(np.stack([c['kf'][rx] for c in pick], axis=1), np.stack([c['kr'][rx] for c in pick], axis=1)),
                wr=cs[0]['wr'][:, rx], wy=cs[0]['wy'][:, sp]), sp, rx


def bound(ref, lo):
    return 1e-12 + 1e-12 * np.abs(ref) + 10.0 * np.abs(lo - ref)


# ------------------------------------------------------------------ 1. the fixture's states
@pytest.mark.parametrize('cells', [1, 2, 8])
def test_fixture_states(P, inputs, fx, cells):
    """xi, order_in and val at the stored cell states within the bound, in
    batches of 1, 63, 64 and 65 (tiled cases); a case's result is bitwise the
    same alone and inside each batch."""
    s = bed(P, inputs, cells)
    cs = cases(fx, cells)
    assert len(cs) == 4 and all(np.array_equal(c['wr'], cs[0]['wr']) and np.array_equal(c['wy'], cs[0]['wy']) for c in cs)
    alone = []
    for c in cs:
        kw, sp, rx = tiled(fx, s, [c], 1)
        alone.append(s.cascade_drc_at(**kw))
    worst = 0.0
    for q, (c, r) in enumerate(zip(cs, alone)):
        assert r['status'][0] == 0 and np.all(r['ostatus'] == 0)
        xi, oi = r['xi'][:, :, 0], r['order_in'][:, :, 0]
        xr, orf = c['xi_ref'][:, rx], c['order_in_ref'][:, sp]
        rx_ratio = np.abs(xi - xr) / bound(xr, c['xi_104'][:, rx])
        oi_ratio = np.abs(oi - orf) / bound(orf, c['order_in_104'][:, sp])
        worst = max(worst, float(rx_ratio.max()), float(oi_ratio.max()))
        print('cells %d T %g: worst xi ratio %.3g, order_in ratio %.3g' % (cells, float(c['T']), rx_ratio.max(), oi_ratio.max()))
        np.testing.assert_allclose(r['val'][:, 0], c['val_ref'], rtol=1e-14)
    assert worst <= 1.0, worst
    for n in (63, 64, 65):
        kw, _, _ = tiled(fx, s, cs, n)
        r = s.cascade_drc_at(**kw)
        assert np.all(r['status'] == 0) and np.all(r['ostatus'] == 0)
        for i in range(n):
            a = alone[i % 4]
            for key in ('xi', 'order_in', 'val'):
                assert np.array_equal(r[key][..., i], a[key][..., 0]), (n, i, key)


# ------------------------------------------------------------------ 2. one cell is the tank
def test_one_cell_against_the_one_lane_multi_kernel(P, inputs, fx):
    """cells = 1 against drc_multi_at on the one-lane kernel at the same
    states: val bitwise; xi bitwise as well (N = 1 runs the same operations in
    the same order; the issue's fallback bound is 1e-13 (1 + |xi|))."""
    from pycatkin_amd import _lib as L
    s = pd111(P, inputs, P.CSTReactor(**BED))
    cs = cases(fx, 1)
    n = 65
    kw, sp, rx = tiled(fx, s, cs, n)
    plan, net = s.plan(()), s.device(())
    T, p, d, fxc, _, inflow = s._inputs(net, plan, n, kw['T'], None, None, None, None, kw['inflow'])
    kf, kr = kw['k']
    a = net.cascade_drc_at(n, T, p, kw['Y_cells'], kf, kr, kw['wr'], kw['wy'], d, fxc, inflow)
    net.set_multi_lanes(L.SENS_LANES_ONE)
    b = net.drc_multi_at(n, T, p, kw['Y_cells'][0], kf, kr, kw['wr'], kw['wy'], d, fxc, inflow)
    assert net.sens_lanes() == 1
    g = lambda t: t.cpu().numpy()
    assert np.array_equal(g(a['status']), g(b['status'])) and np.array_equal(g(a['ostatus']), g(b['ostatus']))
    assert np.array_equal(g(a['val']), g(b['val']))
    xa, xb = g(a['xi']), g(b['xi'])
    print('cells = 1 vs k_lane_multi_adjoint: max |dxi| / (1 + |xi|) = %.3g' % np.max(np.abs(xa - xb) / (1 + np.abs(xb))))
    assert np.array_equal(xa, xb)


# ------------------------------------------------------------------ 3. end to end
@pytest.mark.parametrize('cells', [2, 8])
def test_cascade_drc_batch_end_to_end(P, inputs, fx, cells):
    """cascade_drc_batch on the Pd111 PFReactor at the fixture's temperatures,
    start 'system': every bed status 0, xi within 2 |xi_pert - xi_ref| + 1e-10
    |ref| of xi_ref."""
    import _sens_cascade as SC
    from make_cascade_drc_fixture import INPUT, bed_models
    from oracle import mk_oracle as O
    s = bed(P, inputs, cells)
    cs = cases(fx, cells)
    gases = ['CO', 'O2', 'CO2']
    r = s.cascade_drc_batch(tof_terms=TOF, outlet=gases, T=np.array([float(c['T']) for c in cs]), start='system')
    assert r['labels'] == ['tof'] + ['outlet[%s]' % g for g in gases]
    assert np.all(r['status'] == 0) and np.all(r['ostatus'] == 0) and np.all(r['status_cells'] == 0)
    plan = s.plan(())
    species, dyn = [str(x) for x in fx['species']], [str(x) for x in fx['dyn']]
    rn = [str(x) for x in fx['rnames']]
    spec = O.load_spec(INPUT)
    worst = 0.0
    for i, c in enumerate(cs):
        labels = [str(x) for x in c['labels']]
        rows = [labels.index(lb) for lb in r['labels']]
        y_full = np.array(c['y_full'], float)
        for a, name in enumerate(plan.dyn):
            y_full[:, species.index(name)] = r['y_cells'][:, a, i]
        ms = bed_models(spec, float(c['T']), y_full)
        xp, _, _ = SC.cascade_drc_mp(ms, y_full, list(zip(c['wr'][rows], c['wy'][rows])), 104)
        xp = np.array([[float(x) for x in row] for row in xp])
        ref = c['xi_ref'][rows]
        xi = r['xi'][:, [r['reactions'].index(nm) for nm in rn], i]
        tol = 2.0 * np.abs(xp - ref) + 1e-10 * np.abs(ref)
        ok = np.abs(xi - ref) <= tol
        ratio = float(np.max(np.abs(xi - ref) / np.maximum(tol, 1e-300)))
        worst = max(worst, ratio)
        print('cells %d T %g: worst |xi - ref| / bound %.3g' % (cells, float(c['T']), ratio))
        assert ok.all(), (float(c['T']), xi, ref, xp)
        np.testing.assert_allclose(r['val'][:, i], c['val_ref'][rows], rtol=1e-6)


# ------------------------------------------------------------------ 4. the gate
def test_gate_and_neighbours(P, inputs, fx):
    """n = 65 beds of 8 cells: a bed with a status-4 cell keeps 4, a bed with a
    NaN state and a singular bed (every rate constant zero: the adsorbate rows
    vanish) report PCK_ST_SENS_SINGULAR; each gets NaN xi and order_in, and
    every other bed's result is bitwise what it is without them."""
    s = bed(P, inputs, 8)
    n = 65
    kw, _, _ = tiled(fx, s, cases(fx, 8), n)
    clean = s.cascade_drc_at(**kw)
    assert np.all(clean['status'] == 0)
    st = np.zeros((8, n), np.int32)
    st[3, 5] = ST_NEWTON
    Y = kw['Y_cells'].copy()
    Y[2, 1, 17] = np.nan
    kf, kr = kw['k'][0].copy(), kw['k'][1].copy()
    kf[:, 64] = 0.0
    kr[:, 64] = 0.0
    r = s.cascade_drc_at(**dict(kw, Y_cells=Y, k=(kf, kr), status_cells=st))
    bad = {5: ST_NEWTON, 17: ST_SENS_SINGULAR, 64: ST_SENS_SINGULAR}
    for i, code in bad.items():
        assert r['status'][i] == code and np.all(r['ostatus'][:, i] == code), (i, r['status'][i], r['ostatus'][:, i])
        assert np.isnan(r['xi'][:, [r['reactions'].index(nm) for nm in s.plan(()).reactions], i]).all()
        assert np.isnan(r['order_in'][:, :, i]).all()
    assert np.array_equal(r['val'][:, 5], clean['val'][:, 5])       # finite states: val is written
    assert np.isnan(r['val'][:, 17]).all()                         # a NaN state: no val
    rest = [i for i in range(n) if i not in bad]
    for key in ('xi', 'order_in', 'val', 'status', 'ostatus'):
        assert np.array_equal(r[key][..., rest], clean[key][..., rest]), key


# ------------------------------------------------------------------ 5. refusals
def test_refusals(P, inputs, fx):
    from make_edge_sizes_fixture import T as T_EDGE, T_END, edge_net
    from pycatkin_amd import _lib as L
    from pycatkin_amd.functions.synthetic import synthetic_system
    # nine dynamic species: PCK_E_SIZE
    s9 = synthetic_system(edge_net('e9'), t_end=T_END)[0]
    plan9, net9 = s9.plan(()), s9.device(())
    assert net9.NDYN == 9
    T, p, d, fxc, _, inflow = s9._inputs(net9, plan9, 1, [float(T_EDGE)], None, {'D%d' % q: [0.0] for q in range(4)},
                                         None, None, None)
    kf, kr = net9.rate_constants(1, T, p, d)
    wy = np.eye(9)[:1]
    with pytest.raises(RuntimeError, match=r'error -3: bed DRC: the one-lane kernel only \(at most 8 dynamic species\)'):
        net9.cascade_drc_at(1, T, p, np.full((2, 9, 1), 0.1), kf, kr, None, wy, d, fxc, inflow)
    with pytest.raises(ValueError, match='at most 8 dynamic species'):
        s9.add_reactor(P.CSTReactor(**BED))
        s9._plans.clear()
        s9.cascade_drc_batch(cells=2, outlet=[plan9.dyn[0]], T=[float(T_EDGE)], desc={'D%d' % q: [0.0] for q in range(4)})
    # cells out of range, a network without a flow row: PCK_E_ARG
    s = pd111(P, inputs, P.CSTReactor(**BED))
    kw, _, _ = tiled(fx, s, cases(fx, 2), 1)
    plan, net = s.plan(()), s.device(())
    T, p, d, fxc, _, inflow = s._inputs(net, plan, 1, kw['T'], None, None, None, None, kw['inflow'])
    for cells in (0, L.MAX_CELLS + 1):
        with pytest.raises(RuntimeError, match=r'error -1: bed DRC: cells must be in 1\.\.4096'):
            net.cascade_drc_at(1, T, p, kw['Y_cells'], kw['k'][0], kw['k'][1], kw['wr'], kw['wy'], d, fxc, inflow,
                               cells=cells)
    sid = pd111(P, inputs, P.InfiniteDilutionReactor())
    pid, nid = sid.plan(()), sid.device(())
    T, p, d, fxc, _, inflow = sid._inputs(nid, pid, 1, [500.0], None, None, None, None, None)
    kf, kr = nid.rate_constants(1, T, p, d)
    with pytest.raises(RuntimeError, match=r'error -1: bed DRC: the network has no flow row'):
        nid.cascade_drc_at(1, T, p, np.full((2, nid.NDYN, 1), 0.25), kf, kr, None, np.eye(nid.NDYN)[:1], d, fxc, inflow)
    # the single-tank analyses name the bed's own call
    with pytest.raises(ValueError, match='cascade_drc_batch'):
        bed(P, inputs, 2).drc_batch(TOF, T=[548.0], steady=True, method='analytic')


# ------------------------------------------------------------------ 6. the size limit, NS = 8
SYNTH_SEED, SYNTH_T, SYNTH_CELLS = 3, 500.0, 3


def synth8(P, cells):
    """tests/_synth.py's edge_network(6, 9, SYNTH_SEED) -- s, five adsorbates and
    two gases: eight dynamic species in a CSTR -- as a bed of `cells` cells with
    the Pd111 bed's reactor numbers: (device System carrying one cell's numbers,
    the bed's oracle spec).  The network has no product gas, so a steady bed
    converts nothing and its TOF is zero; the formula is algebraic in the states,
    so it is checked here at generic (not steady) states instead."""
    from _synth import edge_network, spec_of
    from pycatkin_amd.functions.synthetic import synthetic_system
    net = edge_network(6, 9, SYNTH_SEED)
    s = synthetic_system(net, T=SYNTH_T)[0]
    s.add_reactor(P.CSTReactor(**{k: v / cells for k, v in BED.items()}))
    s._plans.clear()
    spec = spec_of(net, np.zeros(4), SYNTH_T)
    spec['reactor'] = dict(kind='CSTR', **BED)
    spec['system']['inflow_state'] = {g[0]: g[4] for g in net['gases']}
    return s, spec


def synth_states(m, cells, variant):
    """Generic positive cell states [cells, n_species] on the site balance."""
    rng = np.random.default_rng(100 + variant)
    y = np.zeros((cells, len(m.snames)))
    for c in range(cells):
        cov = rng.uniform(0.05, 1.0, len(m.ads_idx))
        y[c, m.ads_idx] = cov / cov.sum()
        y[c, m.gas_idx] = m.yin[m.gas_idx] * rng.uniform(0.5, 1.0, len(m.gas_idx))
    return y


def synth_objectives(m):
    rn, dyn = list(m.rnames), [m.snames[q] for q in m.dyn]
    wr, wy = np.zeros((5, len(rn))), np.zeros((5, len(dyn)))
    wr[0, rn.index('R0')] = 2.5
    wy[1, dyn.index(m.snames[m.gas_idx[0]])] = 1.0
    wy[2, dyn.index(m.snames[m.gas_idx[1]])] = 1.0
    wr[3, rn.index('R1')], wy[3, dyn.index(m.snames[m.gas_idx[0]])] = 1.0, 0.5
    wy[4, dyn.index('A0')] = 1.0
    return wr, wy


@pytest.mark.parametrize('cells', [1, SYNTH_CELLS])
def test_eight_species_limit(P, inputs, cells):
    """NS = 8, the kernel's limit: 80 KiB of dynamic LDS (the raised limit of the
    launch) and all eight fields of the pivot bookkeeping.  n = 65 conditions of
    two kinds; xi, order_in and val against tests/_sens_cascade.py at 200 bits
    within 1e-12 + 1e-12 |ref| + 10 |xi_104 - ref|; and for cells = 1 bitwise
    equal to k_lane_multi_adjoint."""
    import _sens_cascade as SC
    from make_cascade_drc_fixture import bed_models
    from make_cascade_fixture import cell_spec
    from oracle import mk_oracle as O
    from pycatkin_amd import _lib as L
    s, spec = synth8(P, cells)
    plan, net = s.plan(()), s.device(())
    assert net.NDYN == 8
    n = 65
    refs, ys = [], []
    for v in range(2):
        m = O.ClassicModel(cell_spec(spec, cells), T=SYNTH_T)
        y_full = synth_states(m, cells, v)
        ms = bed_models(spec, SYNTH_T, y_full)
        wr, wy = synth_objectives(m)
        obj = list(zip(wr, wy))
        hi = SC.cascade_drc_mp(ms, y_full, obj, 200)
        lo = SC.cascade_drc_mp(ms, y_full, obj, 104)
        f = lambda rows: np.array([[float(x) for x in r] for r in rows])
        refs.append(dict(xi=f(hi[0]), val=np.array([float(x) for x in hi[1]]), oi=f(hi[2]), xi_lo=f(lo[0]), oi_lo=f(lo[2])))
        ys.append(y_full)
    dyn, rn = [m.snames[q] for q in m.dyn], list(m.rnames)
    assert list(plan.dyn) == dyn and list(plan.reactions) == rn
    Y = np.stack([ys[i % 2][:, list(m.dyn)] for i in range(n)], axis=2)
    kf, kr = np.tile(m.kf[:, None], (1, n)), np.tile(m.kr[:, None], (1, n))
    desc = {'D%d' % q: np.zeros(n) for q in range(4)}
    inflow = np.tile(m.yin[list(m.dyn)][:, None], (1, n))
    r = s.cascade_drc_at(Y, wr=wr, wy=wy, T=np.full(n, SYNTH_T), desc=desc, inflow=inflow, k=(kf, kr))
    assert np.all(r['status'] == 0) and np.all(r['ostatus'] == 0)
    worst = 0.0
    for i in range(n):
        ref = refs[i % 2]
        xi = r['xi'][:, [r['reactions'].index(nm) for nm in rn], i]
        worst = max(worst, float(np.max(np.abs(xi - ref['xi']) / bound(ref['xi'], ref['xi_lo']))),
                    float(np.max(np.abs(r['order_in'][:, :, i] - ref['oi']) / bound(ref['oi'], ref['oi_lo']))))
        np.testing.assert_allclose(r['val'][:, i], ref['val'], rtol=1e-14)
    print('NS 8, cells %d: worst ratio to the bound %.3g' % (cells, worst))
    assert worst <= 1.0, worst
    for i in range(2, n):
        for key in ('xi', 'order_in', 'val'):
            assert np.array_equal(r[key][..., i], r[key][..., i % 2]), (i, key)
    if cells == 1:
        T, p, d, fxc, _, tin = s._inputs(net, plan, n, np.full(n, SYNTH_T), None, desc, None, None, inflow)
        a = net.cascade_drc_at(n, T, p, Y, kf, kr, wr, wy, d, fxc, tin)
        net.set_multi_lanes(L.SENS_LANES_ONE)
        b = net.drc_multi_at(n, T, p, Y[0], kf, kr, wr, wy, d, fxc, tin)
        assert net.sens_lanes() == 1
        for key in ('status', 'ostatus', 'val', 'xi'):
            assert np.array_equal(a[key].cpu().numpy(), b[key].cpu().numpy()), key


# ------------------------------------------------------------------ 7. pck_cascade_drc's own buffers
def test_padded_ld_c_without_status_cells(P, inputs, fx):
    """pck_cascade_drc with tof_cells on a padded leading dimension (ld_c = n + 3)
    and no status_cells or y_cells of the caller's: the entry point's own status
    buffer shares ld_c and is sized by it.  The result is bitwise that of the
    ordinary call, and the pad columns of tof_cells are not written."""
    import ctypes as C
    from pycatkin_amd import _lib as L
    from pycatkin_amd.classes.system import ROOT_DIST, SCREEN_MARGIN, SCREEN_RTOL, STEADY_TRANSIENT
    from pycatkin_amd.engine import _ptr, _stream
    cells, n, ld = 8, 5, 8
    s = bed(P, inputs, cells)
    plan, net = s.plan(TOF), s.device(TOF)             # with the TOF terms: tof_cells is the objective per cell
    torch = net.torch
    T = np.linspace(440.0, 600.0, n)
    T, p, d, fxc, y0, inflow = s._inputs(net, plan, n, T, None, None, None, None, None)
    wr = np.zeros((1, len(plan.reactions)))
    wr[0, plan.reactions.index('CO_ox')] = 1.0
    kw = dict(t0=0.0, t_end=(s.params['times'] or [0.0, 1.0e4])[-1], rtol=STEADY_TRANSIENT[0], atol=STEADY_TRANSIENT[1],
              max_steps=200000, newton=True, root_dist=ROOT_DIST, screen=(SCREEN_RTOL, SCREEN_MARGIN), wave_order=-1)
    ref = net.cascade_drc(n, T, p, y0, cells, wr, None, d, fxc, inflow, **kw)
    ob, o, out, keep2 = net._multi_io(n, wr, None)
    c, keep = net.conditions(n, T, p, d, fxc, y0, inflow)
    prm = net.params(**kw)
    tof_cells = torch.full((cells, ld), -7.0, dtype=torch.float64, device='cuda')
    nsteps = torch.empty(n, dtype=torch.int32, device='cuda')
    cas = L.Cascade()
    cas.cells, cas.start = cells, L.CASCADE_START_Y0
    cas.tof_cells, cas.ld_c = _ptr(tof_cells), ld
    L.check(net.lib.pck_cascade_drc(net.h, C.byref(c), C.byref(prm), C.byref(cas), C.byref(ob), C.byref(o), None, n,
                                    _ptr(nsteps), _stream(torch)))
    torch.cuda.synchronize()
    for key in ('val', 'xi', 'status', 'ostatus'):
        assert np.array_equal(out[key].cpu().numpy(), ref[key].cpu().numpy()), key
    assert np.all(ref['status'].cpu().numpy() == 0)
    tc = tof_cells.cpu().numpy()
    assert np.all(tc[:, n:] == -7.0) and np.all(np.isfinite(tc[:, :n])) and np.all(tc[:, :n] != -7.0)
    np.testing.assert_allclose(tc[:, :n].mean(axis=0), out['val'].cpu().numpy()[0], rtol=1e-9)
