"""The multi-objective analytic degree of rate control on the device
(csrc/mk_sens_multi.h: k_multi_adjoint; pck_drc_multi_at,
pck_drc_multi_adjoint; System.drc_objectives_at / _batch,
selectivity_control_batch, coverage_control_batch) against tests/golden/
drc_multi_fixture.npz (make_drc_multi_fixture.py: the formula of
tests/_sens_multi.py at 400 bits, at the states and rate constants of
drc_adjoint_fixture.npz).

The kernel's bound is the project's own for the adjoint outputs
(test_gpu_sensitivities.py): |out - ref| <= 1e-12 (1 + |ref|) + 10 |xi_104 - ref|,
xi_104 the fixture's run of the same algorithm at 104 bits."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
sys.path.insert(0, HERE)
from test_gpu_drc_adjoint import case as src_case, cond, system  # noqa: E402  (the Systems of the fixture cases)

MX = dict(np.load(os.path.join(HERE, 'golden', 'drc_multi_fixture.npz')))
NAMES = [str(x) for x in MX['names']]
ST_NONFINITE = 3


@pytest.fixture(scope='module')
def P():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    import pycatkin_amd
    return pycatkin_amd


def mcase(name):
    """A case of the multi fixture with its source case (the condition, the
    state, the rate constants) under 'c'."""
    i = NAMES.index(name)
    pre = 'm%d_' % i
    m = {k[len(pre):]: v for k, v in MX.items() if k.startswith(pre)}
    m['name'] = name
    m['c'] = src_case(int(m['src']))
    return m


def objectives_of(m, rows=None):
    """The fixture's weights as the dicts System.drc_objectives_at takes"""
    rn, dyn = [str(x) for x in m['c']['rnames']], [str(x) for x in m['c']['dyn']]
    out = []
    for k in (range(len(m['wr'])) if rows is None else rows):
        out.append({'rates': {rn[j]: float(w) for j, w in enumerate(m['wr'][k]) if w != 0.0},
                    'species': {dyn[a]: float(w) for a, w in enumerate(m['wy'][k]) if w != 0.0}})
    return out


def state(P, inputs, c, n):
    """(System, kwargs of drc_objectives_at) at the source case's state and
    rate constants, tiled to n conditions"""
    s = system(P, inputs, c['name'])
    plan = s.plan(())
    dyn, rn = [str(x) for x in c['dyn']], [str(x) for x in c['rnames']]
    assert sorted(plan.dyn) == sorted(dyn)
    Y = np.repeat(c['y'][[dyn.index(nm) for nm in plan.dyn]][:, None], n, axis=1)
    rows = [rn.index(r) for r in plan.reactions]
    k = (np.repeat(c['kf'][rows][:, None], n, axis=1), np.repeat(c['kr'][rows][:, None], n, axis=1))
    return s, dict(Y=Y, k=k, **cond(c, n))


def at_state(P, inputs, m, n=1, objectives=None, status_in=None):
    """System.drc_objectives_at at the fixture's state -> the result with xi
    [K, R, n] over the fixture's reactions"""
    c = m['c']
    s, kw = state(P, inputs, c, n)
    out = s.drc_objectives_at(objectives_of(m) if objectives is None else objectives, kw.pop('Y'),
                              status_in=status_in, **kw)
    order = [out['reactions'].index(str(r)) for r in c['rnames']]
    out['xi'] = out['xi'][:, order]
    return out


_AT = {}


def at1(P, inputs, name):
    if name not in _AT:
        _AT[name] = at_state(P, inputs, mcase(name))
    return _AT[name]


def allowed(m):
    return 1e-12 * (1.0 + np.abs(m['xi_ref'])) + 10.0 * np.abs(m['xi_104'] - m['xi_ref'])


# ------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize('name', NAMES)
def test_objectives_at_fixture_states(P, inputs, name):
    """pck_drc_multi_at at the fixture's states and rate constants: every xi
    within 1e-12 (1 + |ref|) + 10 |xi_104 - ref|, every value within 1e-12
    relative (the bound test_drc_at_fixture_states puts on tof0), and the xi of
    the TOF objective within 1e-12 + 1e-12 |xi_ref| of drc_adjoint_fixture's
    xi_ref.  G = 16 (DMTM -- K = 22 > G for dmtm_450_all --, the CSTR with a gas
    objective, the volcano, syn12), 32 (syn24), 64 (syn40, e64: above 64 KiB of
    LDS) and pinned rows (Butadiene)."""
    m = mcase(name)
    out = at1(P, inputs, name)
    err = np.abs(out['xi'][:, :, 0] - m['xi_ref'])
    verr = np.abs(out['val'][:, 0] - m['val_ref']) / np.abs(m['val_ref'])
    print('%s: worst |xi - xi_ref| %.3e (over its bound: %.3e), val rel %.3e'
          % (name, err.max(), (err / allowed(m)).max(), verr.max()))
    assert out['status'][0] == 0 and np.all(out['ostatus'] == 0)
    assert np.all(err <= allowed(m)), (name, err.max(), np.unravel_index(np.argmax(err / allowed(m)), err.shape))
    assert np.all(verr <= 1e-12), (name, verr)
    if str(m['labels'][0]) == 'tof':
        old = m['c']['xi_ref']
        d = np.abs(out['xi'][0, :, 0] - old)
        print('%s: TOF objective against the single-objective fixture %.3e' % (name, d.max()))
        assert np.all(d <= 1e-12 + 1e-12 * np.abs(old)), (name, d.max())


# ------------------------------------------------------------------ 2. identities, no fixture
# Each identity is held to 1e-12 of its largest term, the largest over the
# reactions: the kernel's own bound on an xi is absolute in the objective's
# largest xi (the 1 of 1e-12 (1 + |ref|): xi of O(1) exist in every objective
# here), not relative to each entry -- an xi_j of 1e-25 next to one of 0.9 has
# no relative digits to offer, in the fixture's 104-bit run either.
MIXED = [n for n in NAMES if n != 'dmtm_450_all']


@pytest.mark.parametrize('name', MIXED)
def test_linearity(P, inputs, name):
    """J_mix xi_mix = J_a xi_a + J_b xi_b for the objective whose weights are
    the sum of two others (TOF terms + largest coverage)."""
    m = mcase(name)
    out = at1(P, inputs, name)
    k, a, b = (int(v) for v in m['mix'])
    J, xi = out['val'][:, 0], out['xi'][:, :, 0]
    terms = np.array([J[k] * xi[k], J[a] * xi[a], J[b] * xi[b]])
    res = np.abs(terms[0] - terms[1] - terms[2])
    print('%s: linearity residual %.3e of %.3e' % (name, res.max(), np.abs(terms).max()))
    assert J[k] == J[a] + J[b] or abs(J[k] - J[a] - J[b]) <= 1e-15 * np.abs(J[[k, a, b]]).max()
    assert res.max() <= 1e-12 * np.abs(terms).max()


def test_site_conservation(P, inputs):
    """sum_i C_li y_i xi_(i),j = 0 for each conservation law l and reaction j:
    the laws hold at every k, so their derivative vanishes -- the 11 coverage
    objectives of the K = 22 case, DMTM at 450 K."""
    m = mcase('dmtm_450_all')
    out = at1(P, inputs, 'dmtm_450_all')
    s = system(P, inputs, m['c']['name'])
    plan = s.plan(())
    dyn = [str(x) for x in m['c']['dyn']]
    assert [str(x) for x in m['labels'][:len(dyn)]] == ['[%s]' % d for d in dyn]
    C = np.asarray(plan.conservation)[:, [plan.dyn.index(d) for d in dyn]]
    assert C.shape[0] >= 1
    terms = C[:, :, None] * (out['val'][:len(dyn), 0][:, None] * out['xi'][:len(dyn), :, 0])[None]     # [l, i, j]
    res = np.abs(terms.sum(axis=1))
    print('site conservation: residual %.3e of %.3e' % (res.max(), np.abs(terms).max()))
    for l in range(C.shape[0]):
        assert res[l].max() <= 1e-12 * np.abs(terms[l]).max(), (l, res[l].max())


@pytest.mark.parametrize('name', NAMES)
def test_sum_over_reactions_is_the_fixtures(P, inputs, name):
    """sum_j xi_mj against the fixture's own sum, not against 0 or 1: for a
    coverage in an infinite-dilution reactor the rule sum = 0 holds only to the
    stored root's residual (-3.9e-8 at dmtm_400 in exact arithmetic)."""
    m = mcase(name)
    out = at1(P, inputs, name)
    got, ref = out['xi'][:, :, 0].sum(axis=1), m['xi_ref'].sum(axis=1)
    big = np.abs(m['xi_ref']).max(axis=1)
    print('%s: worst |sum - sum_ref| / largest term %.3e' % (name, (np.abs(got - ref) / big).max()))
    assert np.all(np.abs(got - ref) <= 1e-12 * big), (name, got - ref)


# ------------------------------------------------------------------ 3. the conveniences
DMTM = ['dmtm_400_10000', 'dmtm_450_10000', 'dmtm_600_100000']


def _reorder(r, key, c):
    order = [r['reactions'].index(str(x)) for x in c['rnames']]
    return r[key][..., order, :]


@pytest.mark.parametrize('name', DMTM)
def test_selectivity_control_is_the_difference_bitwise(P, inputs, name):
    """selectivity_control_batch(r5 / (r5 + r9)) at the fixture's state: the
    K = 2 launch gives the difference of test 1's two rows bitwise (an
    objective's answer does not depend on its neighbours) and the ratio of
    their values."""
    m = mcase(name)
    ref = at1(P, inputs, name)
    assert [str(x) for x in m['labels'][:2]] == ['tof', 'r5']
    s, kw = state(P, inputs, m['c'], 1)
    r = s.selectivity_control_batch(('r5',), ('r5', 'r9'), **kw)
    assert r['status'][0] == 0
    np.testing.assert_array_equal(_reorder(r, 'dsc', m['c'])[:, 0], ref['xi'][1, :, 0] - ref['xi'][0, :, 0])
    assert r['selectivity'][0] == ref['val'][1, 0] / ref['val'][0, 0]


@pytest.mark.parametrize('name', ['dmtm_450_10000', 'cstr_573', 'syn24_0'])
def test_coverage_control_is_the_rows_bitwise(P, inputs, name):
    """coverage_control_batch of the fixture's coverage objectives at its
    state: the rows of test 1, bitwise; species=None is every dynamic species."""
    m = mcase(name)
    ref = at1(P, inputs, name)
    rows = [k for k in range(len(m['wr'])) if not m['wr'][k].any() and m['wy'][k].sum() == 1.0
            and np.count_nonzero(m['wy'][k]) == 1]
    dyn = [str(x) for x in m['c']['dyn']]
    species = [dyn[int(np.argmax(m['wy'][k]))] for k in rows]
    assert len(species) >= 3
    s, kw = state(P, inputs, m['c'], 1)
    r = s.coverage_control_batch(species, **kw)
    np.testing.assert_array_equal(_reorder(r, 'dcc', m['c']), ref['xi'][rows])
    np.testing.assert_array_equal(r['coverage'], ref['val'][rows])
    every = s.coverage_control_batch(None, **kw)
    assert every['species'] == list(s.plan(()).dyn) and every['dcc'].shape[0] == len(dyn)
    for sp, k in zip(species, rows):
        np.testing.assert_array_equal(_reorder(every, 'dcc', m['c'])[every['species'].index(sp)], ref['xi'][k])


def test_conveniences_against_the_oracles_finite_difference(P, inputs):
    """DMTM at 600 K / 1e5 Pa: the selectivity control and the coverage
    controls within 10 x the distance of the oracle's central difference
    (eps = 1e-3, find_steady on each side) from the exact limit."""
    m = mcase('dmtm_600_100000')
    c = m['c']
    s, kw = state(P, inputs, c, 1)
    r = s.selectivity_control_batch(('r5',), ('r5', 'r9'), **kw)
    fd, ref = m['xi_fd'][1] - m['xi_fd'][0], m['xi_ref'][1] - m['xi_ref'][0]
    bound = 10.0 * np.abs(fd - ref).max()
    d = np.abs(_reorder(r, 'dsc', c)[:, 0] - fd)
    print('selectivity: |dsc - fd| %.3e (bound %.3e)' % (d.max(), bound))
    assert d.max() <= bound
    dyn = [str(x) for x in c['dyn']]
    for k in range(len(m['wr'])):
        if m['wr'][k].any() or np.count_nonzero(m['wy'][k]) != 1:
            continue
        sp = dyn[int(np.argmax(m['wy'][k]))]
        cc = s.coverage_control_batch([sp], **kw)
        bound = 10.0 * np.abs(m['xi_fd'][k] - m['xi_ref'][k]).max()
        d = np.abs(_reorder(cc, 'dcc', c)[0, :, 0] - m['xi_fd'][k])
        print('coverage %s: |dcc - fd| %.3e (bound %.3e)' % (sp, d.max(), bound))
        assert d.max() <= bound, sp


# ------------------------------------------------------------------ 4. the full path
@pytest.mark.parametrize('name', ['dmtm_450_10000', 'dmtm_600_100000', 'volcano_-1_-1'])
def test_objectives_batch_from_the_start_state(P, inputs, name):
    """The solve and the K adjoint solves together, from the default start
    state: status 0 and every xi within 2 max_j |xi_pert - xi_ref| (xi_ref
    recomputed at the root moved by 1e-6 relative in every species, the parity
    bound the steady solve is held to) plus the bound of test 1."""
    m = mcase(name)
    c = m['c']
    s = system(P, inputs, c['name'])
    kw = cond(c, 1)
    if name.startswith('dmtm'):
        kw.update(t_end=1e14)          # as test_gpu_drc_adjoint.full_path: the transient is on its root by then
    out = s.drc_objectives_batch(objectives_of(m), **kw)
    assert out['status'][0] == 0 and np.all(out['ostatus'] == 0), (out['status'], out['ostatus'])
    xi = out['xi'][:, [out['reactions'].index(str(r)) for r in c['rnames']], 0]
    allow = 2.0 * np.abs(m['xi_pert'] - m['xi_ref']).max(axis=1)[:, None] + allowed(m)
    err = np.abs(xi - m['xi_ref'])
    print('%s: worst |xi - xi_ref| %.3e, worst over its bound %.3e, nsteps %d'
          % (name, err.max(), (err / allow).max(), out['nsteps'][0]))
    assert np.all(err <= allow), (name, err.max(), np.unravel_index(np.argmax(err / allow), err.shape))


# ------------------------------------------------------------------ 5. shapes
@pytest.mark.parametrize('name,n', [('dmtm_450_10000', 1), ('dmtm_450_10000', 3), ('dmtm_450_10000', 5),
                                    ('dmtm_450_10000', 63), ('dmtm_450_10000', 65), ('syn24_0', 3), ('syn24_0', 65)])
def test_tiled_conditions_are_bitwise_equal(P, inputs, name, n):
    """G = 16 packs 4 conditions into a wavefront, G = 32 two: n copies of one
    condition (ragged last wavefronts) all equal the n = 1 answer bitwise."""
    ref = at1(P, inputs, name)
    out = at_state(P, inputs, mcase(name), n=n)
    assert np.all(out['status'] == 0) and np.all(out['ostatus'] == 0)
    np.testing.assert_array_equal(out['xi'], np.repeat(ref['xi'], n, axis=2))
    np.testing.assert_array_equal(out['val'], np.repeat(ref['val'], n, axis=1))


def test_one_objective_alone_equals_itself_among_22(P, inputs):
    """K = 1 against the same objective inside the K = 22 launch, bitwise, for a
    coverage (row 6) and a rate (row 16)."""
    m = mcase('dmtm_450_all')
    ref = at1(P, inputs, 'dmtm_450_all')
    assert ref['xi'].shape[0] == 22
    for k in (6, 16):
        out = at_state(P, inputs, m, objectives=objectives_of(m, [k]))
        assert out['xi'].shape[0] == 1
        np.testing.assert_array_equal(out['xi'][0], ref['xi'][k])
        np.testing.assert_array_equal(out['val'][0], ref['val'][k])


def test_status_in_gates_conditions(P, inputs):
    """status_in = [0, 4, 0, 4, 0]: the 0 rows are the n = 1 answer bitwise;
    the others keep 4 (status and every ostatus), get NaN xi and their values."""
    name = 'dmtm_450_10000'
    ref = at1(P, inputs, name)
    si = np.array([0, 4, 0, 4, 0], np.int32)
    out = at_state(P, inputs, mcase(name), n=5, status_in=si)
    assert out['status'].tolist() == si.tolist()
    assert np.all(out['ostatus'] == si[None, :])
    assert np.all(np.isnan(out['xi'][:, :, si != 0]))
    np.testing.assert_array_equal(out['val'], np.repeat(ref['val'], 5, axis=1))
    for k in np.nonzero(si == 0)[0]:
        np.testing.assert_array_equal(out['xi'][:, :, k], ref['xi'][:, :, 0])


def test_objective_on_a_pinned_species(P, inputs):
    """Butadiene: an objective on a species no reaction can produce (y = 0
    exactly) has the value 0: NaN xi and ostatus 3 for that objective alone;
    the condition's status stays 0 and the other objectives are bitwise what
    they are without it."""
    name = 'butadiene_with_jonas_byproducts_798'
    m = mcase(name)
    c = m['c']
    ref = at1(P, inputs, name)
    dyn = [str(x) for x in c['dyn']]
    pinned = [dyn[a] for a in np.nonzero(c['unreach'])[0] if c['y'][a] == 0.0]
    assert pinned
    objs = objectives_of(m)
    out = at_state(P, inputs, m, objectives=objs[:2] + [pinned[0]] + objs[2:])
    assert out['status'][0] == 0
    assert out['ostatus'][:, 0].tolist() == [0, 0, ST_NONFINITE] + [0] * (len(objs) - 2)
    assert out['val'][2, 0] == 0.0 and np.all(np.isnan(out['xi'][2]))
    keep = [0, 1] + list(range(3, len(objs) + 1))
    np.testing.assert_array_equal(out['xi'][keep], ref['xi'])
    np.testing.assert_array_equal(out['val'][keep], ref['val'])


def test_a_network_without_tof_terms_is_accepted(P, inputs):
    """The objectives are data of the call: the plan has no TOF terms (pck_drc_at
    refuses such a network), one network serves every set of objectives, and the
    group kernel answers whatever the network's adjoint mode says."""
    m = mcase('volcano_-1_-1')
    s = system(P, inputs, m['c']['name'])
    net = s.device(())
    assert net.NTOF == 0 and list(s.plan(()).tof_terms) == []
    net.set_sens_lanes(1)                       # one lane per condition for drc_at / sens_at
    try:
        out = at_state(P, inputs, m)
        assert net.sens_lanes() == 16
    finally:
        net.set_sens_lanes(0)
    np.testing.assert_array_equal(out['xi'], at1(P, inputs, 'volcano_-1_-1')['xi'])
    assert s.device(()) is net
    _, kw = state(P, inputs, m['c'], 1)
    with pytest.raises(RuntimeError, match='no TOF terms'):
        s.drc_at((), kw.pop('Y'), **kw)
