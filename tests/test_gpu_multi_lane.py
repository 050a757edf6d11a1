"""The one-lane multi-objective DRC kernel on the device
(csrc/mk_sens_multi_lane.h: k_lane_multi_adjoint; pck_network_set_multi_lanes;
adjoint_kernel='lane' of System.drc_objectives_at / _batch,
selectivity_control_batch, coverage_control_batch) against the NS <= 8 cases of
drc_multi_fixture.npz (the volcano, NS 4; the CSTR, NS 6) and every case of
drc_multi_lane_fixture.npz (NS 3, 7, 8 and a pinned species).

The kernel's bounds are those of the group kernels (test_gpu_drc_multi.py):
|xi - ref| <= 1e-12 (1 + |ref|) + 10 |xi_104 - ref|, val within 1e-12 relative.
The two kernels compute the same formulas in double-double and differ only in
the order of their sums."""
import os

import numpy as np
import pytest

import test_gpu_drc_adjoint as D
import test_gpu_drc_multi as DM
import test_gpu_lane_sens as GL
import test_multi_lane as ML

pytestmark = pytest.mark.gpu

P = D.P
OLD = [nm for nm in DM.NAMES if nm.startswith(('volcano_', 'cstr_'))]
CASES = OLD + ML.NAMES
ST_NONFINITE, ST_NEWTON, ST_SENS_SINGULAR = 3, 4, 7


def mcase(name):
    """A case of either fixture, its source case (condition, state, rate
    constants, the single-objective xi_ref) under 'c'."""
    if name in OLD:
        return DM.mcase(name)
    m = ML.mcase(ML.NAMES.index(name))
    m['c'] = dict(m['s'], name=name)
    GL.lane_system(str(m['c']['net']))
    return m


def at_state(P, inputs, m, n=1, objectives=None, status_in=None, kernel='lane'):
    """System.drc_objectives_at at the fixture's state -> the result with xi
    [K, R, n] over the fixture's reactions, and the lanes of the launch"""
    c = m['c']
    s, kw = DM.state(P, inputs, c, n)
    out = s.drc_objectives_at(DM.objectives_of(m) if objectives is None else objectives, kw.pop('Y'),
                              status_in=status_in, adjoint_kernel=kernel, **kw)
    out['xi'] = out['xi'][:, [out['reactions'].index(str(r)) for r in c['rnames']]]
    out['lanes'] = s.device(()).sens_lanes()
    return out


_AT = {}


def at1(P, inputs, name):
    if name not in _AT:
        _AT[name] = at_state(P, inputs, mcase(name))
    return _AT[name]


# ------------------------------------------------------------------ 1. the kernel
def test_cases_cover_the_lane_networks():
    assert len([nm for nm in OLD if nm.startswith('volcano_')]) >= 2
    assert len([nm for nm in OLD if nm.startswith('cstr_')]) == 2
    assert any('[CO2]' in [str(x) for x in DM.mcase(nm)['labels']] for nm in OLD)      # a gas objective


@pytest.mark.parametrize('name', CASES)
def test_lane_kernel_at_fixture_states(P, inputs, name):
    """adjoint_kernel='lane' at the fixtures' states and rate constants: every
    xi within 1e-12 (1 + |ref|) + 10 |xi_104 - ref|, every value within 1e-12
    relative, the TOF objective's xi within 1e-12 + 1e-12 |ref| of the
    single-objective fixture's xi_ref, every status 0, one lane per condition.
    NS 3 .. 8 (l8: 80 KiB of dynamic LDS, above the default limit), the CSTR's
    flow rows, T-dependent row scale and gas objective, the pinned row."""
    m = mcase(name)
    out = at1(P, inputs, name)
    assert out['lanes'] == 1
    err = np.abs(out['xi'][:, :, 0] - m['xi_ref'])
    verr = np.abs(out['val'][:, 0] - m['val_ref']) / np.abs(m['val_ref'])
    print('%s: worst |xi - xi_ref| %.3e (over its bound: %.3e), val rel %.3e'
          % (name, err.max(), (err / DM.allowed(m)).max(), verr.max()))
    assert out['status'][0] == 0 and np.all(out['ostatus'] == 0)
    assert np.all(err <= DM.allowed(m)), (name, err.max(), np.unravel_index(np.argmax(err / DM.allowed(m)), err.shape))
    assert np.all(verr <= 1e-12), (name, verr)
    labels = [str(x) for x in m['labels']]
    assert 'tof' in labels
    old = m['c']['xi_ref']
    d = np.abs(out['xi'][labels.index('tof'), :, 0] - old)
    print('%s: TOF objective against the single-objective fixture %.3e' % (name, d.max()))
    assert np.all(d <= 1e-12 + 1e-12 * np.abs(old)), (name, d.max())
    if name.startswith('l8'):
        assert len(m['c']['dyn']) == 8


# ------------------------------------------------------------------ 2. divergence inside a wavefront
def kinds_of(P, inputs, roots, keep, equal=None):
    """The four kinds of condition of one network -- its two roots, the first
    root made singular (every rate constant but `keep`'s zeroed, and with equal
    = (a, b) the state of species a set to that of b), the second root gated by
    status_in = 4 -- as columns (Y, kf, kr, T, p, desc, status_in) in plan order."""
    c0 = roots[0]['c']
    s = D.system(P, inputs, c0['name'])
    plan = s.plan(())
    dyn, rn = [str(x) for x in c0['dyn']], [str(x) for x in c0['rnames']]
    rows = [rn.index(r) for r in plan.reactions]
    cols = []
    for which, sing, gate in ((0, False, 0), (1, False, 0), (0, True, 0), (1, False, ST_NEWTON)):
        c = roots[which]['c']
        assert [str(x) for x in c['rnames']] == rn and [str(x) for x in c['dyn']] == dyn
        y = c['y'][[dyn.index(nm) for nm in plan.dyn]].copy()
        kf, kr = c['kf'][rows].copy(), c['kr'][rows].copy()
        if sing:
            z = np.array([r != keep for r in plan.reactions])
            kf[z] = 0.0
            kr[z] = 0.0
            if equal:
                y[plan.dyn.index(equal[0])] = y[plan.dyn.index(equal[1])]
        cols.append(dict(y=y, kf=kf, kr=kr, T=float(c['T']), p=float(c['p']), si=gate,
                         desc={str(k): float(v) for k, v in zip(c['desc_names'], c['desc'])}))
    return s, cols


def run_cols(s, cols, objectives, kernel='lane'):
    n = len(cols)
    out = s.drc_objectives_at(objectives, np.stack([c['y'] for c in cols], axis=1),
                              k=(np.stack([c['kf'] for c in cols], axis=1), np.stack([c['kr'] for c in cols], axis=1)),
                              T=np.array([c['T'] for c in cols]), p=np.array([c['p'] for c in cols]),
                              desc={k: np.array([c['desc'][k] for c in cols]) for k in cols[0]['desc']},
                              status_in=np.array([c['si'] for c in cols], np.int32), adjoint_kernel=kernel)
    assert s.device(()).sens_lanes() == (1 if kernel == 'lane' else 16) and out['xi'].shape[2] == n
    return out


NETWORKS = {'l8': (('l8_0', 'l8_1'), None, None), 'volcano': (('volcano_-1_-1', 'volcano_-2.5_0.5'), 'CO_ox', ('sO', 'sCO'))}
_KINDS = {}


def singles(P, inputs, key, kernel='lane'):
    """(System, the four kinds, the objectives, each kind's n = 1 answer by the named kernel)"""
    if (key, kernel) not in _KINDS:
        names, keep, equal = NETWORKS[key]
        roots = [mcase(nm) for nm in names]
        keep = str(roots[0]['c']['tof_terms'][0]) if keep is None else keep
        s, cols = kinds_of(P, inputs, roots, keep, equal)
        objs = DM.objectives_of(roots[0])
        _KINDS[key, kernel] = s, cols, objs, [run_cols(s, [c], objs, kernel) for c in cols]
    return _KINDS[key, kernel]


@pytest.mark.parametrize('key', ['l8', 'volcano'])
def test_the_four_kinds_alone(P, inputs, key):
    """At n = 1: the roots answer (status 0), the singular condition has status
    7 and the gated one its 4, in `status` and in every `ostatus`, with NaN xi
    and their values written."""
    s, cols, objs, one = singles(P, inputs, key)
    K = len(objs)
    assert key != 'l8' or K > 8
    for q, st in enumerate((0, 0, ST_SENS_SINGULAR, ST_NEWTON)):
        assert one[q]['status'][0] == st, (q, one[q]['status'])
        assert np.all(one[q]['ostatus'] == st), (q, one[q]['ostatus'])
        assert np.all(np.isfinite(one[q]['val'])), q
        active = [j for j, r in enumerate(one[q]['reactions']) if r in s.plan(()).reactions]
        assert np.all(np.isnan(one[q]['xi'][:, active])) if st else np.all(np.isfinite(one[q]['xi']))
    # the tof objective of the singular condition is the kept reaction's net rate: finite and not 0
    assert one[2]['val'][0, 0] != 0.0
    np.testing.assert_array_equal(one[3]['val'], one[1]['val'])


def check_conditions_diverge(P, inputs, key, n, kernel):
    s, cols, objs, one = singles(P, inputs, key, kernel)
    r = run_cols(s, [cols[q % 4] for q in range(n)], objs, kernel)
    for q in range(n):
        ref = one[q % 4]
        assert r['status'][q] == ref['status'][0], q
        for k2 in ('val', 'xi', 'ostatus'):
            np.testing.assert_array_equal(r[k2][..., q], ref[k2][..., 0], err_msg='%s condition %d' % (k2, q))
    if n >= 4:
        assert np.count_nonzero(r['status'] == ST_SENS_SINGULAR) == len([q for q in range(n) if q % 4 == 2])
        assert np.count_nonzero(r['status'] == ST_NEWTON) == len([q for q in range(n) if q % 4 == 3])


@pytest.mark.parametrize('n', [1, 63, 64, 65, 130])
@pytest.mark.parametrize('key', ['l8', 'volcano'])
def test_lanes_of_a_wavefront_diverge(P, inputs, key, n):
    """The four kinds interleaved in one call (different pivot orders, a lane
    that leaves at the factorisation, a gated one): every condition's val, xi,
    status and ostatus are bitwise its own n = 1 answer."""
    check_conditions_diverge(P, inputs, key, n, 'lane')


@pytest.mark.parametrize('n', [3, 4, 5, 9])
@pytest.mark.parametrize('key', ['l8', 'volcano'])
def test_groups_of_a_wavefront_diverge(P, inputs, key, n):
    """The same by the group kernel (csrc/mk_sens_multi.h: k_multi_adjoint<16>, 16
    lanes per condition as run_cols asserts, four conditions to a wavefront and
    a block): a partly filled block, a full one, the first condition of the
    second and third blocks.  The singular condition's group goes through the
    objective loop with status 7 beside groups that solve; every condition is
    bitwise its own n = 1 group-kernel answer."""
    check_conditions_diverge(P, inputs, key, n, 'group')


# ------------------------------------------------------------------ 3. objectives are independent
def test_each_objective_alone_is_its_row(P, inputs):
    """l8_0, K > 8: objective m computed alone (K = 1) is bitwise its row in the
    full call."""
    m = mcase('l8_0')
    ref = at1(P, inputs, 'l8_0')
    K = ref['xi'].shape[0]
    assert K > 8
    for k in range(K):
        out = at_state(P, inputs, m, objectives=DM.objectives_of(m, [k]))
        assert out['xi'].shape[0] == 1 and out['lanes'] == 1 and out['ostatus'][0, 0] == 0
        np.testing.assert_array_equal(out['xi'][0], ref['xi'][k])
        np.testing.assert_array_equal(out['val'][0], ref['val'][k])


def test_objective_on_the_pinned_species(P, inputs):
    """pin_0: the coverage of the pinned species (y = 0 exactly) as one more
    objective has the value 0, NaN xi and ostatus 3 for it alone; the
    condition's status stays 0 and the other rows are bitwise unchanged."""
    m = mcase('pin_0')
    c = m['c']
    ref = at1(P, inputs, 'pin_0')
    dyn = [str(x) for x in c['dyn']]
    pinned = [dyn[a] for a in np.nonzero(c['unreach'])[0]]
    assert len(pinned) == 1 and c['y'][dyn.index(pinned[0])] == 0.0
    objs = DM.objectives_of(m)
    out = at_state(P, inputs, m, objectives=objs[:2] + [pinned[0]] + objs[2:])
    assert out['lanes'] == 1 and out['status'][0] == 0
    assert out['ostatus'][:, 0].tolist() == [0, 0, ST_NONFINITE] + [0] * (len(objs) - 2)
    assert out['val'][2, 0] == 0.0 and np.all(np.isnan(out['xi'][2]))
    keep = [0, 1] + list(range(3, len(objs) + 1))
    np.testing.assert_array_equal(out['xi'][keep], ref['xi'])
    np.testing.assert_array_equal(out['val'][keep], ref['val'])


# ------------------------------------------------------------------ 4. the modes
def test_nine_species_refuse_lane_and_auto_takes_the_group_kernel(P, inputs):
    from make_edge_sizes_fixture import T as T_EDGE, T_END, edge_net
    from pycatkin_amd.functions.synthetic import synthetic_system
    efx = dict(np.load(os.path.join(ML.HERE, 'golden', 'edge_sizes_fixture.npz')))
    s = synthetic_system(edge_net('e9'), t_end=T_END)[0]
    plan = s.plan(())
    k = int(np.nonzero(efx['e9_regular'])[0][0])
    dyn = [str(x) for x in efx['e9_dyn']]
    Y = efx['e9_y'][k][[dyn.index(nm) for nm in plan.dyn]][:, None]
    kw = dict(T=[float(T_EDGE)], desc={'D%d' % q: [float(efx['desc'][k, q])] for q in range(4)})
    net = s.device(())
    assert net.NDYN == 9
    objs = [nm for a, nm in enumerate(plan.dyn) if Y[a, 0] != 0.0][:3]
    with pytest.raises(RuntimeError, match=r'error -3: one-lane multi-objective DRC: at most 8 dynamic species'):
        net.set_multi_lanes(1)
    with pytest.raises(RuntimeError, match=r'error -3'):
        s.drc_objectives_at(objs, Y, adjoint_kernel='lane', **kw)
    with pytest.raises(RuntimeError, match=r'error -1'):
        net.set_multi_lanes(3)
    out = s.drc_objectives_at(objs, Y, adjoint_kernel='auto', **kw)
    assert net.sens_lanes() == 16 and out['status'][0] == 0 and np.all(out['ostatus'] == 0)
    ref = s.drc_objectives_at(objs, Y, adjoint_kernel='group', **kw)
    assert net.sens_lanes() == 16
    np.testing.assert_array_equal(out['xi'], ref['xi'])


def test_the_two_modes_are_independent(P, inputs):
    """set_multi_lanes does not move drc_at, set_sens_lanes does not move
    drc_objectives_at; 'auto' takes one lane on four species."""
    m = mcase('volcano_-1_-1')
    c = m['c']
    s, kw = DM.state(P, inputs, c, 1)
    Y = kw.pop('Y')
    tt = ('CO_ox',)
    net_t, net_0 = s.device(tt), s.device(())
    try:
        net_t.set_multi_lanes(1)
        s.drc_at(tt, Y, adjoint_kernel='group', **kw)
        assert net_t.sens_lanes() == 16
        net_0.set_sens_lanes(1)
        out = s.drc_objectives_at(DM.objectives_of(m), Y, **kw)
        assert net_0.sens_lanes() == 16
        lane = s.drc_objectives_at(DM.objectives_of(m), Y, adjoint_kernel='lane', **kw)
        assert net_0.sens_lanes() == 1
        auto = s.drc_objectives_at(DM.objectives_of(m), Y, adjoint_kernel='auto', **kw)
        assert net_0.sens_lanes() == 1
        np.testing.assert_array_equal(auto['xi'], lane['xi'])
        again = s.drc_objectives_at(DM.objectives_of(m), Y, **kw)
        assert net_0.sens_lanes() == 16
        np.testing.assert_array_equal(again['xi'], out['xi'])
    finally:
        net_t.set_multi_lanes(0)
        net_0.set_sens_lanes(0)
        net_0.set_multi_lanes(0)


# ------------------------------------------------------------------ 5. the full path
@pytest.mark.parametrize('name', OLD)
def test_objectives_batch_from_the_start_state(P, inputs, name):
    """drc_objectives_batch(adjoint_kernel='lane'): the solve and the K adjoint
    solves together from the default start state: status 0 and every xi within
    2 max_j |xi_pert - xi_ref| plus the bound of test 1; nsteps is returned."""
    m = mcase(name)
    c = m['c']
    s = D.system(P, inputs, c['name'])
    out = s.drc_objectives_batch(DM.objectives_of(m), adjoint_kernel='lane', **D.cond(c, 1))
    assert s.device(()).sens_lanes() == 1
    assert out['status'][0] == 0 and np.all(out['ostatus'] == 0), (out['status'], out['ostatus'])
    assert out['nsteps'].shape == (1,) and out['nsteps'][0] > 0
    xi = out['xi'][:, [out['reactions'].index(str(r)) for r in c['rnames']], 0]
    allow = 2.0 * np.abs(m['xi_pert'] - m['xi_ref']).max(axis=1)[:, None] + DM.allowed(m)
    err = np.abs(xi - m['xi_ref'])
    print('%s: worst |xi - xi_ref| %.3e, worst over its bound %.3e, nsteps %d'
          % (name, err.max(), (err / allow).max(), out['nsteps'][0]))
    assert np.all(err <= allow), (name, err.max(), np.unravel_index(np.argmax(err / allow), err.shape))


# ------------------------------------------------------------------ 6. a small grid
def test_coverage_control_on_a_small_volcano_grid(P, inputs):
    """Volcano 32 x 32 at 600 K: one solve_batch, then coverage_control_batch at
    its states with 'lane' and with 'group': identical status, ostatus and NaN
    pattern, `coverage` bitwise equal (it is y_i itself).  The worst
    |dcc_lane - dcc_group| is printed, not asserted: the two kernels sum in
    different orders and no bound for ill-conditioned corner nodes can be
    derived in advance."""
    c = DM.mcase('volcano_-1_-1')['c']
    s = D.system(P, inputs, c['name'])
    g = np.linspace(-2.5, 0.5, 32)
    eco, eo = (a.ravel() for a in np.meshgrid(g, g, indexing='ij'))
    n = eco.size
    kw = dict(T=np.full(n, 600.0), p=np.full(n, float(c['p'])), desc={'ECO': eco, 'EO': eo})
    r = s.solve_batch(tof_terms=(), steady=True, **kw)
    assert r['y'].shape == (4, n)
    out = {}
    for kernel, lanes in (('lane', 1), ('group', 16)):
        out[kernel] = s.coverage_control_batch(None, Y=r['y'], status_in=r['status'], adjoint_kernel=kernel, **kw)
        assert s.device(()).sens_lanes() == lanes
    a, b = out['lane'], out['group']
    assert a['species'] == b['species'] == list(s.plan(()).dyn)
    np.testing.assert_array_equal(a['status'], b['status'])
    np.testing.assert_array_equal(a['ostatus'], b['ostatus'])
    np.testing.assert_array_equal(np.isnan(a['dcc']), np.isnan(b['dcc']))
    np.testing.assert_array_equal(a['coverage'], b['coverage'])
    np.testing.assert_array_equal(a['coverage'], r['y'])
    ok = a['status'] == 0
    assert ok.sum() >= n // 2, np.unique(a['status'], return_counts=True)
    d = np.where(np.isnan(a['dcc']), 0.0, np.abs(a['dcc'] - b['dcc']))
    i, j, q = np.unravel_index(np.argmax(d), d.shape)
    print('volcano 32 x 32: %d of %d conditions answered (statuses %s); %d of %d finite entries differ'
          % (ok.sum(), n, dict(zip(*(x.tolist() for x in np.unique(a['status'], return_counts=True)))),
             np.count_nonzero(d), np.count_nonzero(~np.isnan(a['dcc']))))
    if d[i, j, q] > 0.0:
        print('volcano 32 x 32: worst |dcc_lane - dcc_group| %.3e (dcc %.6e) for [%s], reaction %s at ECO %.4f EO %.4f'
              % (d[i, j, q], b['dcc'][i, j, q], a['species'][i], a['reactions'][j], eco[q], eo[q]))
    rel = d / (1.0 + np.abs(np.where(np.isnan(b['dcc']), 0.0, b['dcc'])))
    print('volcano 32 x 32: worst |dcc_lane - dcc_group| / (1 + |dcc_group|) %.3e; median over conditions of the '
          'per-condition worst %.3e' % (rel.max(), np.median(rel.max(axis=(0, 1))[ok])))
