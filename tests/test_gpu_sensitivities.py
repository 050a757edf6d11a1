"""The adjoint sensitivities on the device (csrc/mk_sens.h: k_sens_adjoint, its
steps and output tail in csrc/mk_adjoint.h;
pck_sens_at, pck_sens_adjoint; System.sensitivity_at / sensitivity_batch)
against tests/golden/sensitivity_fixture.npz (make_sensitivity_fixture.py: the
formulas of tests/_sens_ext.py at 400 bits, at the states and rate constants of
drc_adjoint_fixture.npz).

The kernel's bound (test 1), for every output:
    |out - ref| <= 1e-12 (1 + |ref|) + 10 |out_104 - ref|
with out_104 the fixture's own 104-bit run: where double-double itself is the
limit (DMTM at 400 K, 1.9e-14) the kernel is held to ten times that."""
import os

import numpy as np
import pytest

import test_gpu_drc_adjoint as D

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SX = dict(np.load(os.path.join(HERE, 'golden', 'sensitivity_fixture.npz')))
NAMES = D.NAMES
assert [str(x) for x in SX['names']] == NAMES
REGULAR = [int(i) for i in SX['regular']]
GUARDED = [i for i in REGULAR if float(SX['c%d_err' % i]) <= 1e-9]
FLAGGED = [i for i in REGULAR if i not in GUARDED]
EAPP = [i for i in REGULAR if 'c%d_eapp_ref' % i in SX]
ST_SENS_PRECISION = 8
P = D.P                                        # the module fixture: the package, or skip without a device


def scase(i):
    """The case of both fixtures: states, rate constants and xi_ref from
    drc_adjoint_fixture.npz, the new references from sensitivity_fixture.npz."""
    c = D.case(i)
    pre = 'c%d_' % i
    c.update({k[len(pre):]: v for k, v in SX.items() if k.startswith(pre) and k[len(pre):] not in ('rnames', 'xi_ref')})
    assert [str(x) for x in SX[pre + 'rnames']] == [str(x) for x in c['rnames']]
    return c


def sens_at(P, inputs, c, n=1, directions='fixture', status_in=None, **kw):
    """System.sensitivity_at at the fixture's state and rate constants, tiled
    to n conditions; per-reaction outputs over the fixture's reactions,
    orders over the fixture's names.  directions: 'fixture' (its random one),
    None, or a list of (a, c) over the fixture's reactions."""
    s = D.system(P, inputs, c['name'])
    tof_terms = tuple(str(t) for t in c['tof_terms'])
    plan = s.plan(tof_terms)
    dyn, rn = [str(x) for x in c['dyn']], [str(x) for x in c['rnames']]
    assert sorted(plan.dyn) == sorted(dyn)
    Y = np.repeat(c['y'][[dyn.index(nm) for nm in plan.dyn]][:, None], n, axis=1)
    rows = [rn.index(r) for r in plan.reactions]
    k = (np.repeat(c['kf'][rows][:, None], n, axis=1), np.repeat(c['kr'][rows][:, None], n, axis=1))
    if isinstance(directions, str):
        directions = [(c['dir_a'], c['dir_c'])]
    dirs = None
    if directions:
        dirs = tuple(np.stack([np.repeat(np.asarray(d[q], float)[rows][:, None], n, axis=1) for d in directions])
                     for q in (0, 1))
    out = s.sensitivity_at(tof_terms, Y, k=k, status_in=status_in, directions=dirs, **D.cond(c, n), **kw)
    r = {key: np.array([out[key][x] for x in rn]) for key in ('xi', 'sf', 'sr')}
    assert set(str(x) for x in c['order_names']) <= set(out['order']) == set(plan.fix)
    # a fixed species no rate depends on is not among the fixture's names: its order is exactly 0
    for name in set(plan.fix) - set(str(x) for x in c['order_names']):
        assert np.all(out['order'][name] == 0.0) or np.all(np.isnan(out['order'][name]))
    r['order'] = np.array([out['order'][str(x)] for x in c['order_names']]).reshape(len(c['order_names']), n)
    assert sorted(out['order_inflow']) == sorted(str(x) for x in c['order_in_names'])
    r['order_in'] = np.array([out['order_inflow'][str(x)] for x in c['order_in_names']]).reshape(len(c['order_in_names']), n)
    for key in ('dir', 'tof0', 'status', 'err'):
        r[key] = out[key]
    r['active'] = np.array([x in plan.reactions for x in rn])      # a ghost reaction's entries are 0 by convention
    return r


_AT = {}


def at1(P, inputs, i, **kw):
    key = (i,) + tuple(sorted(kw.items()))
    if key not in _AT:
        _AT[key] = sens_at(P, inputs, scase(i), **kw)
    return _AT[key]


def bound(c, key):
    ref = c[key + '_ref']
    return 1e-12 * (1.0 + np.abs(ref)) + 10.0 * np.abs(c[key + '_104'] - ref)


OUTPUTS = ('sf', 'sr', 'order', 'order_in', 'dir')


# ------------------------------------------------------------------ 1. the kernel
def test_eighteen_cases_pass_the_default_guard():
    assert len(GUARDED) == 18 and [NAMES[i] for i in FLAGGED] == ['volcano_-2.5_0.5']


@pytest.mark.parametrize('i', GUARDED, ids=[NAMES[i] for i in GUARDED])
def test_sensitivity_at_fixture_states(P, inputs, i):
    """pck_sens_at at the fixture's states and rate constants: sf, sr, the
    orders, the inflow orders (the CSTR) and the fixture's direction within the
    kernel's bound; status 0; err is the fixture's.  Covers G = 16, 32 and 64
    (syn40, e64) and the pinned rows (Butadiene)."""
    c = scase(i)
    r = at1(P, inputs, i)
    assert r['status'][0] == 0
    for key in OUTPUTS:
        got, ref = r[key][:, 0], c[key + '_ref']
        assert got.shape == ref.shape, key
        if ref.size:
            err = np.abs(got - ref)
            print('%s %s: worst |out - ref| %.3e (bound there %.3e)' % (c['name'], key, err.max(),
                                                                       bound(c, key)[int(np.argmax(err))]))
            assert np.all(err <= bound(c, key)), (c['name'], key, err.max())
    assert np.all(D.within(r['xi'][:, 0], c['xi_ref']))
    assert abs(r['err'][0] - c['err']) <= 1e-12 * c['err']
    assert all(np.all(np.isfinite(r[key])) for key in OUTPUTS)


def test_cstr_has_inflow_orders_and_syn_has_orders(P, inputs):
    """The cases are not vacuous: the CSTR's orders are all inflow orders, the
    synthetic and Butadiene networks have O(1) orders in their fixed species."""
    c = scase(D.idx('cstr_')[0])
    assert len(c['order_in_names']) >= 2 and np.max(np.abs(c['order_in_ref'])) > 1e-3
    assert np.max(np.abs(scase(D.idx('syn12_')[0])['order_ref'])) > 1.0
    assert np.max(np.abs(scase(D.idx('butadiene_')[0])['order_ref'])) > 0.5


# ------------------------------------------------------------------ 2. the guard
def test_precision_guard_flags_the_tiny_tof(P, inputs):
    """volcano_-2.5_0.5 (TOF 1.8e-43, max rate / |TOF| 7e34): status 8, NaN sf /
    sr / order / dir, xi within the analytic DRC's bound; with err_max = 0 the
    same call answers with finite numbers and status 0."""
    i = FLAGGED[0]
    c = scase(i)
    r = at1(P, inputs, i)
    assert r['status'][0] == ST_SENS_PRECISION and r['err'][0] > 1.0
    for key in ('sf', 'sr', 'order', 'dir'):
        v = r[key][r['active']] if key in ('sf', 'sr') else r[key]
        assert v.size and np.all(np.isnan(v)), key
    assert np.all(D.within(r['xi'][:, 0], c['xi_ref'])) and np.isfinite(r['tof0'][0])
    r0 = at1(P, inputs, i, err_max=0.0)
    assert r0['status'][0] == 0
    for key in ('sf', 'sr', 'order', 'dir', 'xi'):
        assert np.all(np.isfinite(r0[key])), key
    np.testing.assert_array_equal(r0['xi'], r['xi'])


# ------------------------------------------------------------------ 3. directions
DIRS = [D.idx('dmtm_')[1], D.idx('syn24_')[0], D.idx('volcano_')[0]]


@pytest.mark.parametrize('i', DIRS, ids=[NAMES[i] for i in DIRS])
def test_directions(P, inputs, i):
    """a = c = 1 is sum_j xi_j; a_j = ef_jq, c_j = er_jq is order[q]; two
    directions in one call equal the two single calls bitwise.  (The fixture's
    random direction is held to the kernel's bound in test 1.)"""
    c = scase(i)
    s = D.system(P, inputs, c['name'])
    net = s.device(tuple(str(t) for t in c['tof_terms']))
    plan = s.plan(tuple(str(t) for t in c['tof_terms']))
    rn = [str(x) for x in c['rnames']]
    R = len(rn)
    base = at1(P, inputs, i)
    ones = (np.ones(R), np.ones(R))
    r1 = sens_at(P, inputs, c, directions=[ones])
    assert abs(r1['dir'][0, 0] - base['xi'][:, 0].sum()) <= 1e-12
    # the fixed-species exponents of the compiled network (PCK_I_OFF_FOLDF / _FOLDR)
    from pycatkin_amd import _lib as L
    F = net.NFIX
    ef = np.asarray(plan.ip[plan.ip[L.I_OFF_FOLDF]: plan.ip[L.I_OFF_FOLDF] + net.NRXN * F]).reshape(net.NRXN, F)
    er = np.asarray(plan.ip[plan.ip[L.I_OFF_FOLDR]: plan.ip[L.I_OFF_FOLDR] + net.NRXN * F]).reshape(net.NRXN, F)
    q = int(np.argmax(np.abs(ef).sum(0) + np.abs(er).sum(0)))
    expo = tuple(np.array([float(e[plan.reactions.index(x), q]) if x in plan.reactions else 0.0 for x in rn])
                 for e in (ef, er))               # (a ghost reaction is not in the compiled network)
    assert np.any(expo[0] + expo[1] > 0)
    r2 = sens_at(P, inputs, c, directions=[expo])
    order_q = base['order'][[str(x) for x in c['order_names']].index(plan.fix[q]), 0]
    assert abs(r2['dir'][0, 0] - order_q) <= 1e-12 * (1.0 + abs(order_q))
    both = sens_at(P, inputs, c, directions=[ones, expo])
    assert both['dir'].shape == (2, 1)
    assert both['dir'][0, 0] == r1['dir'][0, 0] and both['dir'][1, 0] == r2['dir'][0, 0]


# ------------------------------------------------------------------ 4. the full path
def _full(P, inputs, key):
    ids = [i for i in EAPP if NAMES[i].startswith(key)]
    s, kw, tof_terms, _ = D.full_path(P, inputs, ids)
    return ids, s.sensitivity_batch(tof_terms, eapp=True, **kw)


@pytest.mark.parametrize('key,count', [('dmtm_', 4), ('volcano_', 3)])
def test_sensitivity_batch_orders_and_eapp(P, inputs, key, count):
    """The solve, the adjoint and the stencil together, from the default start
    state: orders within 2 |order_pert - order_ref| + the kernel's bound
    (order_pert: the reference at the root moved by 1e-6 per species, the
    solve's parity bound); Eapp within 2 |eapp_pert - eapp_ref| + 2 |eapp_2h -
    eapp_ref| + 1e-10 |eapp_ref| (the last: the device's rate constants against
    the oracle's through the stencil), and within 10 |eapp_fd - eapp_ref| of the
    oracle's own finite difference at 450 K and above."""
    ids, out = _full(P, inputs, key)
    assert len(ids) == count
    assert np.all(out['status'] == 0), out['status']
    worst = 0.0
    for k, i in enumerate(ids):
        c = scase(i)
        got = np.array([out['order'][str(x)][k] for x in c['order_names']])
        allow = 2.0 * np.abs(c['order_pert'] - c['order_ref']) + bound(c, 'order')
        err = np.abs(got - c['order_ref'])
        print('%s: orders %s, worst error %.3e (allowed %.3e)' % (c['name'], got, err.max(), allow[int(np.argmax(err))]))
        assert np.all(err <= allow), (c['name'], got, c['order_ref'])
        ref = float(c['eapp_ref'])
        e = abs(out['eapp'][k] - ref)
        tol_root = 2.0 * abs(float(c['eapp_pert']) - ref) + 2.0 * abs(float(c['eapp_2h']) - ref)
        worst = max(worst, e / abs(ref))
        print('%s: Eapp %.6f kJ/mol, |Eapp - ref| / |ref| %.3e (root + stencil terms %.3e, rate-constant term 1e-10)'
              % (c['name'], out['eapp'][k] / 1e3, e / abs(ref), tol_root / abs(ref)))
        assert e <= tol_root + 1e-10 * abs(ref), (c['name'], out['eapp'][k], ref)
        if float(c['T']) >= 450.0:
            assert abs(out['eapp'][k] - float(c['eapp_fd'])) <= 10.0 * abs(float(c['eapp_fd']) - ref), c['name']
        assert abs(out['tof0'][k] - float(c['tof_ref'])) <= 1e-6 * abs(float(c['tof_ref']))
    print('worst |Eapp - ref| / |ref| %.3e' % worst)


# ------------------------------------------------------------------ 5. orders vs the device's own finite differences
@pytest.mark.parametrize('key,pos,species,tol', [('volcano_', 0, 'CO', 1e-5), ('dmtm_', 2, 'CH4', 1e-6)])
def test_order_vs_device_finite_difference(P, inputs, key, pos, species, tol):
    """order[species] against the central difference of ln TOF of two steady
    solves with that species' pressure scaled by 1 +- 1e-3: the quotient's
    O(delta^2) term and the solve's 1e-6 parity leave this margin."""
    i = D.idx(key)[pos]
    s, kw, tof_terms, cs = D.full_path(P, inputs, [i])
    plan = s.plan(tof_terms)
    out = s.sensitivity_batch(tof_terms, **kw)
    assert out['status'][0] == 0
    delta = 1e-3
    fix = np.repeat(np.asarray(plan.fix_default, float)[:, None], 2, axis=1)
    fix[plan.fix.index(species)] *= [1.0 + delta, 1.0 - delta]
    kw2 = {k: (np.repeat(v, 2) if k in ('T', 'p') else {a: np.repeat(b, 2) for a, b in v.items()} if k == 'desc' else v)
           for k, v in kw.items()}
    r = s.solve_batch(tof_terms=tof_terms, steady=True, fix=fix, **kw2)
    assert np.all(r['status'] == 0), r['status']
    fd = (np.log(r['tof'][0]) - np.log(r['tof'][1])) / (np.log1p(delta) - np.log1p(-delta))
    print('%s: order[%s] %.9f, finite difference %.9f' % (NAMES[i], species, out['order'][species][0], fd))
    assert abs(out['order'][species][0] - fd) <= tol


# ------------------------------------------------------------------ 6. packing
ALL_KEYS = ('xi', 'sf', 'sr', 'order', 'order_in', 'dir', 'tof0', 'err')


@pytest.mark.parametrize('key,n', [('dmtm_', 3), ('dmtm_', 5), ('dmtm_', 63), ('dmtm_', 65), ('syn24_', 3),
                                   ('syn24_', 65)])
def test_tiled_conditions_are_bitwise_equal(P, inputs, key, n):
    """n copies of one condition (ragged last wavefronts) equal the n = 1
    answer bitwise in every output."""
    i = D.idx(key)[0]
    ref = at1(P, inputs, i)
    r = sens_at(P, inputs, scase(i), n=n)
    assert np.all(r['status'] == 0)
    for k in ALL_KEYS:
        np.testing.assert_array_equal(r[k], np.repeat(ref[k], n, axis=-1), err_msg=k)


def test_status_in_gates_conditions(P, inputs):
    """status_in = [0, 4, 0, 4, 0]: the 0 columns are the n = 1 answer bitwise,
    the others keep 4 and get NaN everywhere but a finite tof0."""
    i = D.idx('dmtm_')[1]
    ref = at1(P, inputs, i)
    si = np.array([0, 4, 0, 4, 0], np.int32)
    r = sens_at(P, inputs, scase(i), n=5, status_in=si)
    assert r['status'].tolist() == si.tolist()
    assert np.all(np.isfinite(r['tof0']))
    for k in ('xi', 'sf', 'sr', 'order', 'dir', 'err'):
        v = r[k][r['active']] if k in ('xi', 'sf', 'sr') else r[k]
        assert np.all(np.isnan(v[..., si != 0])), k
        for q in np.nonzero(si == 0)[0]:
            np.testing.assert_array_equal(r[k][..., q], ref[k][..., 0], err_msg=k)


# ------------------------------------------------------------------ 7. the analytic DRC is unchanged
@pytest.mark.parametrize('i', [D.idx('dmtm_')[1], D.idx('syn24_')[0], D.idx('e64_')[0]],
                         ids=['dmtm_450', 'syn24_0', 'e64'])
def test_xi_is_drc_at_bitwise(P, inputs, i):
    xi, tof0, st = D.at1(P, inputs, i)
    r = at1(P, inputs, i)
    assert st[0] == 0 and r['status'][0] == 0
    np.testing.assert_array_equal(r['xi'], xi)
    np.testing.assert_array_equal(r['tof0'], tof0)


# ------------------------------------------------------------------ 8. refusals
def test_eapp_refusals(P, inputs):
    s = D.system(P, inputs, 'cstr_473')
    with pytest.raises(ValueError, match='row scale'):
        s.sensitivity_batch(('CO_ox',), T=[523.0], eapp=True)
    from pycatkin_amd.functions.volcano import set_volcano_energies
    v = P.read_from_input_file(os.path.join(inputs, 'COOxVolcano', 'input.json'))
    set_volcano_energies(v)
    v.reactions['CO_ox'].dEa_fwd_user = {600.0: 0.8, 650.0: 0.9}
    v._plans.clear()
    with pytest.raises(ValueError, match='temperature-keyed'):
        v.sensitivity_batch(('CO_ox',), T=[600.0], desc={'ECO': -1.0, 'EO': -1.0}, eapp=True)
    with pytest.raises(ValueError, match='steady'):
        D.system(P, inputs, 'dmtm_400_10000').sensitivity_batch(('r5', 'r9'), T=[500.0], steady=False)


def test_one_condition_conveniences(P, inputs):
    """System.reaction_orders / apparent_activation_energy at the volcano's
    (-1, -1): the fixture's numbers; a flagged condition raises with its status."""
    i = D.idx('volcano_')[0]
    c = scase(i)
    from pycatkin_amd.functions.volcano import set_volcano_energies
    s = P.read_from_input_file(os.path.join(inputs, 'COOxVolcano', 'input.json'))
    set_volcano_energies(s)
    s.desc_defaults = {str(k): float(v) for k, v in zip(c['desc_names'], c['desc'])}
    s.params['temperature'], s.params['pressure'] = float(c['T']), float(c['p'])
    tof_terms = [str(t) for t in c['tof_terms']]
    orders = s.reaction_orders(tof_terms)
    ea = s.apparent_activation_energy(tof_terms)
    for x, ref, pert in zip(c['order_names'], c['order_ref'], c['order_pert']):
        assert abs(orders[str(x)] - ref) <= 2.0 * abs(pert - ref) + 1e-12 * (1.0 + abs(ref))
    assert abs(ea - float(c['eapp_ref'])) <= 1e-5 * abs(float(c['eapp_ref']))
    with pytest.raises(RuntimeError, match='status 8'):
        s._check(ST_SENS_PRECISION, 'reaction_orders')
