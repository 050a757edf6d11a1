"""Reactor cascade on the device (pck_solve_cascade, System.solve_cascade_batch)
against the oracle fixture (tests/golden/cascade_fixture.npz), against the
march written out with System.solve_batch(inflow=...) on a CSTReactor carrying
one cell's numbers, and its march rules, batch independence and refusals.

Bounds: the oracle bound of tests/test_gpu_parity.py (close_cov: 1e-6
relative, floor 1e-15) for states against the oracle; between two compilations
of one solve (fused k_cascade against k_solve) the bound of
test_compiled_cstr_plan_matches_runtime_plan, 1e-7 relative, floor 1e-14."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
BED = dict(residence_time=4.5, volume=1.8e-7, catalyst_area=3.82e-9)   # COOxReactor/input_Pd111.json
TOF = ('CO_ox',)


@pytest.fixture(scope='module')
def P():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    import pycatkin_amd
    return pycatkin_amd


@pytest.fixture(scope='module')
def fixture():
    return np.load(os.path.join(GOLD, 'cascade_fixture.npz'))


def close_cov(a, b, rtol, floor):
    a, b = np.asarray(a), np.asarray(b)
    return np.all(np.abs(a - b) <= rtol * np.abs(b) + floor)


def worst_ratio(a, b, rtol, floor):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / (rtol * np.abs(b) + floor))) if a.size else 0.0


def pd111(P, inputs, reactor):
    s = P.read_from_input_file(os.path.join(inputs, 'COOxReactor', 'input_Pd111.json'))
    s.add_reactor(reactor)
    s._plans.clear()
    return s


def bed(P, inputs, cells):
    return pd111(P, inputs, P.PFReactor(cells=cells, **BED))


def cell(P, inputs, cells):
    """A CSTReactor carrying one cell's numbers."""
    return pd111(P, inputs, P.CSTReactor(**{k: v / cells for k, v in BED.items()}))


def flow_rows(plan):
    from pycatkin_amd import _lib as L
    off = int(plan.ip[L.I_HDR + L.D_DYN])
    return np.asarray(plan.dp[off: off + 4 * len(plan.dyn)]).reshape(len(plan.dyn), 4)[:, 3] != 0.0


def written_loop(s, cells, start, n, y0=None, **kw):
    """The parent's own march: `cells` calls of solve_batch(inflow=previous
    outlet) on the cell system s, the rules of pck_solve_cascade on the host."""
    plan = s.plan(TOF)
    fl = flow_rows(plan)
    ns = len(plan.dyn)
    inflow = np.tile(plan.inflow_default[:, None], (1, n))
    y0 = np.tile(plan.y0_default[:, None], (1, n)) if y0 is None else np.array(y0)
    out = dict(y_cells=np.full((cells, ns, n), np.nan), tof_cells=np.full((cells, n), np.nan),
               status_cells=np.zeros((cells, n), np.int32), nsteps_cells=np.zeros((cells, n), np.int32),
               cell_fail=np.full(n, -1, np.int32), y=np.full((ns, n), np.nan))
    fail = np.zeros(n, np.int32)
    for c in range(cells):
        r = s.solve_batch(y0=y0, inflow=inflow, tof_terms=TOF, steady=True, **kw)
        live = fail == 0
        out['y_cells'][c][:, live] = r['y'][:, live]
        out['tof_cells'][c, live] = r['tof'][live]
        out['status_cells'][c] = np.where(live, r['status'], fail)
        out['nsteps_cells'][c, live] = r['nsteps'][live]
        out['y'][:, live] = r['y'][:, live]
        bad = live & (r['status'] >= 1) & (r['status'] <= 3)
        out['cell_fail'][bad] = c
        fail = np.where(bad, r['status'], fail)
        go = fail == 0
        inflow = np.where(go[None, :] & fl[:, None], r['y'], inflow)
        if start == 'upstream':
            y0 = np.where(go[None, :], r['y'], y0)
    out['status'] = np.where(fail != 0, fail, 4 * np.any(out['status_cells'] == 4, axis=0)).astype(np.int32)
    out['nsteps'] = out['nsteps_cells'].sum(0).astype(np.int32)
    out['tof'] = np.where(fail != 0, np.nan, out['tof_cells'].sum(0) / cells)
    return out


def same_march(a, b, rtol=1e-7, floor=1e-14):
    """Statuses, failing cells and NaN pattern equal; status-0 cells' states
    and TOFs within the two-compilation bound."""
    assert np.array_equal(a['status_cells'], b['status_cells'])
    assert np.array_equal(a['status'], b['status'])
    assert np.array_equal(a['cell_fail'], b['cell_fail'])
    assert np.array_equal(np.isnan(a['y_cells']), np.isnan(b['y_cells']))
    assert np.array_equal(np.isnan(a['tof_cells']), np.isnan(b['tof_cells']))
    ok = a['status_cells'] == 0
    ya, yb = np.moveaxis(a['y_cells'], 1, 0)[:, ok], np.moveaxis(b['y_cells'], 1, 0)[:, ok]
    assert close_cov(ya, yb, rtol, floor), worst_ratio(ya, yb, rtol, floor)
    np.testing.assert_allclose(a['tof_cells'][ok], b['tof_cells'][ok], rtol=rtol)
    allok = a['status'] == 0
    assert close_cov(a['y'][:, allok], b['y'][:, allok], rtol, floor)
    np.testing.assert_allclose(a['tof'][allok], b['tof'][allok], rtol=rtol)


@pytest.fixture(scope='module')
def march65(P, inputs):
    """n = 65 temperatures (one full wavefront and one lane), 8 cells: the
    fused march and the written-out loop in both start modes, computed once."""
    T = np.linspace(423.0, 623.0, 65)
    out = {}
    for start in ('system', 'upstream'):
        out['fused', start] = bed(P, inputs, 8).solve_cascade_batch(T=T, tof_terms=TOF, start=start, method='fused')
        out['written', start] = written_loop(cell(P, inputs, 8), 8, start, 65, T=T)
    return T, out


@pytest.mark.parametrize('start', ['system', 'upstream'])
@pytest.mark.parametrize('cells', [1, 2, 8])
def test_oracle_parity(P, inputs, fixture, cells, start):
    """Every cell with an oracle answer: status 0 and its state within the
    oracle bound (1e-6 relative, floor 1e-15), cell c at most (c+1) times it.
    Worst ratio to the unscaled bound seen per cell: DESIGN.md "Reactor cascade"."""
    tag = 'c%d_%s' % (cells, start)
    ref, ok = fixture['y_' + tag], fixture['ref_ok_' + tag]
    assert ok.sum() >= (17 if cells == 1 else 16)
    assert fixture['regular_' + tag][ok].all()
    s = bed(P, inputs, cells)
    r = s.solve_cascade_batch(T=fixture['T'], tof_terms=TOF, start=start)
    plan = s.plan(TOF)
    pos = [list(fixture['species']).index(x) for x in plan.dyn]
    have = ~np.isnan(ref[:, :, 0])                      # [17, cells]: cells the oracle solved
    worst = []
    for c in range(cells):
        m = have[:, c]
        got, want = r['y_cells'][c][:, m], ref[m, c][:, pos].T
        worst.append(worst_ratio(got, want, 1e-6, 1e-15))
        print('cells %d start %s cell %d: worst ratio to the bound %.3g' % (cells, start, c, worst[-1]))
    for c in range(cells):
        m = have[:, c]
        assert np.all(r['status_cells'][c][m] == 0), (c, r['status_cells'][c])
        assert worst[c] <= c + 1, (c, worst)
    assert np.all(r['cell_fail'] == -1)
    co = plan.dyn.index('CO')
    np.testing.assert_array_equal(r['conversion']['CO'], 1.0 - r['y'][co] / 0.02)


@pytest.mark.parametrize('start', ['system', 'upstream'])
def test_fused_matches_written_loop(march65, start):
    T, m = march65
    a, b = m['fused', start], m['written', start]
    assert np.all(a['status'] == 0), a['status']
    same_march(a, b)


@pytest.mark.parametrize('start', ['system', 'upstream'])
def test_loop_method_matches_fused(P, inputs, march65, start):
    T, m = march65
    b = bed(P, inputs, 8).solve_cascade_batch(T=T, tof_terms=TOF, start=start, method='loop')
    same_march(m['fused', start], b)
    assert np.array_equal(m['fused', start]['nsteps_cells'].shape, b['nsteps_cells'].shape)


def test_upstream_start_saves_steps(march65):
    T, m = march65
    assert m['fused', 'upstream']['nsteps'].sum() < m['fused', 'system']['nsteps'].sum()


def test_one_cell_is_solve_batch(P, inputs):
    T = np.linspace(423.0, 623.0, 65)
    a = bed(P, inputs, 1).solve_cascade_batch(T=T, tof_terms=TOF)
    b = cell(P, inputs, 1).solve_batch(T=T, tof_terms=TOF, steady=True)
    assert np.array_equal(a['status'], b['status']) and np.all(a['status'] == 0)
    assert np.all(a['cell_fail'] == -1)
    assert close_cov(a['y'], b['y'], 1e-7, 1e-14), worst_ratio(a['y'], b['y'], 1e-7, 1e-14)
    np.testing.assert_allclose(a['tof'], b['tof'], rtol=1e-7)
    np.testing.assert_array_equal(a['y'], a['y_cells'][0])
    # a plain CSTReactor with cells=1 is the same bed
    c = cell(P, inputs, 1).solve_cascade_batch(cells=1, T=T, tof_terms=TOF)
    np.testing.assert_array_equal(a['y'], c['y'])


def volcano_bed(P, inputs, reactor):
    from pycatkin_amd.functions.volcano import set_volcano_energies
    s = P.read_from_input_file(os.path.join(inputs, 'COOxVolcano', 'input.json'))
    s.add_reactor(reactor)
    set_volcano_energies(s)
    s.params['inflow_state'] = {'CO': 0.02, 'O2': 0.08}
    s._plans.clear()
    return s


def _volcano_written(s, cells, n, kw):
    """written_loop for the volcano network (descriptors, explicit tolerances)."""
    plan = s.plan(TOF)
    fl = flow_rows(plan)
    inflow = np.tile(plan.inflow_default[:, None], (1, n))
    ys, tofs, sts = [], [], []
    for c in range(cells):
        r = s.solve_batch(inflow=inflow, **kw)
        ys.append(r['y']); tofs.append(r['tof']); sts.append(r['status'])
        assert not np.any((r['status'] >= 1) & (r['status'] <= 3))
        inflow = np.where(fl[:, None], r['y'], inflow)
    return np.stack(ys), np.stack(tofs), np.stack(sts)


def _volcano_case(P, inputs, want_plan):
    cells, n = 4, 64
    rng = np.random.default_rng(11)
    kw = dict(T=np.full(n, 600.0), desc={'ECO': rng.uniform(-2.0, 0.0, n), 'EO': rng.uniform(-2.0, 0.0, n)},
              tof_terms=TOF, steady=True, t_end=3600.0, rtol=1e-9, atol=1e-13)
    s = volcano_bed(P, inputs, P.PFReactor(cells=cells, **BED))
    net = s.device(TOF)
    assert net.compiled_plan == 0
    a = s.solve_cascade_batch(method='fused', **{k: v for k, v in kw.items() if k != 'steady'})
    assert net.plan_id() == want_plan
    w = volcano_bed(P, inputs, P.CSTReactor(**{k: v / cells for k, v in BED.items()}))
    yb, tb, sb = _volcano_written(w, cells, n, kw)
    # the bounds of test_jit_plan_matches_runtime_plan, over whole beds
    both = np.all(a['status_cells'] == 0, axis=0) & np.all(sb == 0, axis=0)
    assert np.mean(both) > 0.9, (np.unique(a['status_cells'], return_counts=True), np.unique(sb, return_counts=True))
    assert np.mean(np.any(a['status_cells'] != sb, axis=0)) < 0.05
    ya, yb = a['y_cells'][:, :, both], yb[:, :, both]
    assert close_cov(ya, yb, 1e-7, 1e-14), worst_ratio(ya, yb, 1e-7, 1e-14)
    tof = np.max(np.abs(a['tof_cells'][:, both] - tb[:, both]) / np.abs(tb[:, both]))
    assert tof <= 1e-6, tof


def test_jit_plan_cascade(P, inputs):
    """The volcano network in a PFReactor has no compiled-in plan: the cascade
    runs k_cascade over the plan hipRTC specialises for it."""
    _volcano_case(P, inputs, 100)


def test_runtime_plan_cascade(P, inputs, monkeypatch):
    """PCK_JIT=0: the same bed on k_cascade<PlanRT<NS>>."""
    monkeypatch.setenv('PCK_JIT', '0')
    _volcano_case(P, inputs, 0)


def test_march_stops_at_step_budget(P, inputs):
    """Every cell starts from the condition's own first-cell steady state
    (start='system' with that y0): the first cell then takes a few steps and
    the cells behind it, whose inflow differs, more.  max_steps is chosen
    between the step counts of that unrestricted march (no screening trip, so
    a cell's nsteps is its one solve's; an integrator budget, not a device
    fault): conditions whose later cells need more report PCK_ST_MAXSTEPS
    there, with cell_fail, the NaN tail and the failing status as the
    written-out loop; conditions that never fail are bitwise the unrestricted
    answers."""
    T = np.linspace(423.0, 623.0, 65)
    s = bed(P, inputs, 8)
    y0 = s.solve_cascade_batch(T=T, tof_terms=TOF)['y_cells'][0]
    free = s.solve_cascade_batch(T=T, y0=y0, tof_terms=TOF, screen=None)
    assert np.all(free['status'] == 0)
    ns = free['nsteps_cells']
    print('steps per cell (rows) and condition:\n', ns)
    first, later, most = ns[0], ns[1:].max(0), ns.max(0)
    budget, gap = None, 1                              # no cell's own count at the budget or next to it
    for m in range(int(most.max()) - gap - 1, gap, -1):
        if np.any((first < m - gap) & (later > m + gap)) and np.any(most < m - gap) \
                and not np.any(np.abs(ns - m) <= gap):
            budget = m
            break
    assert budget is not None, ns
    a = s.solve_cascade_batch(T=T, y0=y0, tof_terms=TOF, screen=None, max_steps=budget)
    b = written_loop(cell(P, inputs, 8), 8, 'system', 65, y0=y0, T=T, screen=None, max_steps=budget)
    failed = a['cell_fail'] >= 0
    assert np.any(a['cell_fail'] >= 1) and np.any(~failed)
    assert np.all(a['status'][failed] == 1) and np.all(a['status'][~failed] == 0)
    same_march(a, b)
    for j in np.nonzero(failed)[0]:
        c = a['cell_fail'][j]
        assert np.all(a['status_cells'][c:, j] == 1) and np.all(a['status_cells'][:c, j] == 0)
        assert np.all(np.isnan(a['y_cells'][c + 1:, :, j])) and np.all(np.isnan(a['tof_cells'][c + 1:, j]))
        assert np.all(np.isfinite(a['y_cells'][:c + 1, :, j])) and np.isnan(a['tof'][j])
        assert np.all(a['nsteps_cells'][c + 1:, j] == 0)
        np.testing.assert_array_equal(a['y'][:, j], a['y_cells'][c, :, j])
    for k in ('y', 'tof', 'nsteps', 'y_cells', 'tof_cells', 'status_cells', 'nsteps_cells'):
        np.testing.assert_array_equal(a[k][..., ~failed], free[k][..., ~failed], err_msg=k)


def test_batch_independence(P, inputs):
    T = np.linspace(423.0, 623.0, 65)
    s = bed(P, inputs, 8)
    runs = [s.solve_cascade_batch(T=T[:n], tof_terms=TOF, start='upstream') for n in (1, 63, 64, 65)]
    for r in runs[1:]:
        for k in ('y', 'tof', 'status', 'nsteps', 'cell_fail', 'y_cells', 'tof_cells', 'status_cells',
                  'nsteps_cells'):
            np.testing.assert_array_equal(r[k][..., 0], runs[0][k][..., 0], err_msg=k)
        np.testing.assert_array_equal(r['conversion']['CO'][0], runs[0]['conversion']['CO'][0])


def test_refusals(P, inputs):
    from pycatkin_amd import _lib as L
    s = bed(P, inputs, 2)
    plan, net = s.plan(TOF), s.device(TOF)
    n = 3
    args = (n, np.linspace(450.0, 550.0, n), 1.0e5, plan.y0_default)
    kw = dict(inflow=plan.inflow_default, t_end=3600.0, rtol=1e-6, atol=1e-22, newton=True, root_dist=1e-6)

    def refused(code, cells=2, net=net, args=args, **over):
        with pytest.raises(RuntimeError, match=r'C-ABI error %d:' % code):
            net.solve_cascade(*args, cells, **{**kw, **over})

    assert np.all(net.solve_cascade(*args, 2, **kw)['status'].cpu().numpy() == 0)
    refused(L.E_ARG, cells=0)
    refused(L.E_ARG, cells=L.MAX_CELLS + 1)
    refused(L.E_ARG, start=2)
    refused(L.E_ARG, t_out=[0.0, 1.0])
    refused(L.E_ARG, retry=(1e-9, 1e-24))
    refused(L.E_ARG, activity=True)
    # a network without a flow row
    v = P.read_from_input_file(os.path.join(inputs, 'COOxVolcano', 'input.json'))
    from pycatkin_amd.functions.volcano import set_volcano_energies
    set_volcano_energies(v)
    vp, vn = v.plan(TOF), v.device(TOF)
    with pytest.raises(RuntimeError, match=r'C-ABI error %d:.*flow' % L.E_ARG):
        vn.solve_cascade(1, 600.0, 1.0e5, vp.y0_default, 2, desc=np.array([[-1.0], [-1.0]]),
                         fixc=vp.fix_default * vp.fix_conc_factor, **{k: x for k, x in kw.items() if k != 'inflow'})
    # beyond the one-lane limits, or forced onto the group solver: PCK_E_SIZE, checked first
    net.set_plan_mode(L.PLAN_GROUP)
    refused(L.E_SIZE)
    refused(L.E_SIZE, cells=0)
    net.set_plan_mode(L.PLAN_AUTO)
    with pytest.raises(ValueError, match='start'):
        net.solve_cascade(*args, 2, start='downstream', **kw)
    with pytest.raises(ValueError, match='method'):
        net.solve_cascade(*args, 2, method='auto', **kw)


def test_large_network_takes_the_loop(P, inputs):
    """DMTM in a CSTR has more than 8 dynamic species: 'fused' raises with the
    one-lane limit, 'auto' marches with the loop on the lane-group kernels."""
    from pycatkin_amd import _lib as L
    s = P.read_from_input_file(os.path.join(inputs, 'DMTM', 'input.json'))
    s.add_reactor(P.CSTReactor(residence_time=4.5, volume=1.8e-7, catalyst_area=3.82e-9))
    s.names_to_indices()
    s._plans.clear()
    plan = s.plan(())
    assert len(plan.dyn) > L.MAX_DYN_LANE
    gas = [x for i, x in enumerate(plan.dyn) if flow_rows(plan)[i]]
    inflow = np.zeros(len(plan.dyn))
    for x in gas:
        inflow[plan.dyn.index(x)] = 0.1
    kw = dict(cells=2, T=np.array([400.0, 450.0]), inflow=inflow, t_end=10.0)
    with pytest.raises(ValueError, match='8 dynamic species'):
        s.solve_cascade_batch(method='fused', **kw)
    with pytest.raises(RuntimeError, match=r'C-ABI error %d:' % L.E_SIZE):
        s.device(()).solve_cascade(2, kw['T'], 1.0e5, plan.y0_default, 2, inflow=inflow, t_end=10.0, newton=True)
    a = s.solve_cascade_batch(method='auto', **kw)
    b = s.solve_cascade_batch(method='loop', **kw)
    assert a['status_cells'].shape == (2, 2) and set(np.unique(a['status'])) <= {0, 4}
    for k in ('y', 'y_cells', 'status_cells', 'nsteps_cells'):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
