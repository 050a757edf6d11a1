"""The one-lane adjoint kernels on the device (csrc/mk_sens_lane.h:
k_lane_drc_adjoint, k_lane_sens_adjoint; adjoint_kernel='lane') and the
descriptor sensitivities (System.descriptor_sensitivity_at / _batch) against
drc_adjoint_fixture.npz, sensitivity_fixture.npz and lane_sens_fixture.npz.

The kernel's bounds are those of the group kernels (test_gpu_drc_adjoint.within
for xi, test_gpu_sensitivities.bound for every other output): the two kernels
compute the same formulas in double-double and differ only in the order of
their sums."""
import os

import numpy as np
import pytest

import test_gpu_drc_adjoint as D
import test_gpu_sensitivities as SG
import test_lane_sens as LS

pytestmark = pytest.mark.gpu

P = D.P
NAMES = D.NAMES
LANE_OLD = [i for i in SG.GUARDED if NAMES[i].startswith(('volcano_', 'cstr_'))]
VOLCANO_ALL = D.idx('volcano_')
OUTPUTS = SG.OUTPUTS
ST_SENS_SINGULAR, ST_SENS_PRECISION = 7, 8
H = 1.0e-3


def lane_system(key):
    """The product's System of a network of make_lane_sens_fixture.NETS, registered
    where test_gpu_drc_adjoint.system looks its cases up (by the name's prefix)."""
    if key not in D._SYS:
        from make_lane_sens_fixture import T_END, lane_net
        from pycatkin_amd.functions.synthetic import synthetic_system
        D._SYS[key] = synthetic_system(lane_net(key), t_end=T_END)[0]
    return D._SYS[key]


def any_case(tag):
    """('c', i): a case of the two older fixtures; ('n', k): a new one."""
    kind, k = tag
    if kind == 'c':
        return SG.scase(k)
    c = LS.ncase(k)
    lane_system(str(c['net']))
    return c


TAGS = [('c', i) for i in LANE_OLD] + [('n', k) for k in range(len(LS.NAMES))]
TAG_IDS = [NAMES[i] for i in LANE_OLD] + LS.NAMES
_AT = {}


def at1(P, inputs, tag, kernel='lane', **kw):
    key = (tag, kernel) + tuple(sorted(kw.items()))
    if key not in _AT:
        _AT[key] = SG.sens_at(P, inputs, any_case(tag), adjoint_kernel=kernel, **kw)
    return _AT[key]


def net_of(P, inputs, c):
    s = D.system(P, inputs, c['name'])
    return s.device(tuple(str(t) for t in c['tof_terms']))


# ------------------------------------------------------------------ 1. the kernel
def test_cases_cover_the_lane_networks():
    assert len([i for i in LANE_OLD if NAMES[i].startswith('volcano_')]) == 3
    assert len([i for i in LANE_OLD if NAMES[i].startswith('cstr_')]) == 3


@pytest.mark.parametrize('tag', TAGS, ids=TAG_IDS)
def test_lane_kernel_at_fixture_states(P, inputs, tag):
    """adjoint_kernel='lane' at the fixture's states and rate constants: xi
    within 1e-12 + 1e-12 |ref|, every other output within 1e-12 (1 + |ref|) +
    10 |out_104 - ref|, err to 1e-12 relative, status 0, one lane per
    condition; the same call with 'group' reports 16.  NS 3 .. 8, the CSTR's
    flow rows and T-dependent row scale, the pinned row."""
    c = any_case(tag)
    r = at1(P, inputs, tag)
    net = net_of(P, inputs, c)
    assert net.sens_lanes() == 1
    assert r['status'][0] == 0
    for key in OUTPUTS:
        got, ref = r[key][:, 0], c[key + '_ref']
        assert got.shape == ref.shape, key
        if ref.size:
            err = np.abs(got - ref)
            print('%s %s: worst |out - ref| %.3e (bound there %.3e)' % (c['name'], key, err.max(),
                                                                       SG.bound(c, key)[int(np.argmax(err))]))
            assert np.all(err <= SG.bound(c, key)), (c['name'], key, err.max())
    exi = np.abs(r['xi'][:, 0] - c['xi_ref'])
    print('%s xi: worst |xi - ref| %.3e' % (c['name'], exi.max()))
    assert np.all(D.within(r['xi'][:, 0], c['xi_ref'])), (c['name'], exi.max())
    assert abs(r['err'][0] - c['err']) <= 1e-12 * c['err']
    assert abs(r['tof0'][0] - c['tof_ref']) <= 1e-12 * abs(c['tof_ref'])
    g = at1(P, inputs, tag, kernel='group')
    assert net.sens_lanes() == 16 and g['status'][0] == 0
    if c['name'].startswith('pin'):
        assert c['unreach'].sum() == 1


# ------------------------------------------------------------------ 2. the guard
def test_lane_precision_guard(P, inputs):
    """volcano_-2.5_0.5: status 8 and NaN in everything but xi / tof0 / err; with
    err_max = 0 finite outputs and status 0."""
    tag = ('c', SG.FLAGGED[0])
    c = any_case(tag)
    r = at1(P, inputs, tag)
    assert net_of(P, inputs, c).sens_lanes() == 1
    assert r['status'][0] == ST_SENS_PRECISION and r['err'][0] > 1.0
    for key in ('sf', 'sr', 'order', 'dir'):
        v = r[key][r['active']] if key in ('sf', 'sr') else r[key]
        assert v.size and np.all(np.isnan(v)), key
    assert np.all(D.within(r['xi'][:, 0], c['xi_ref'])) and np.isfinite(r['tof0'][0])
    r0 = at1(P, inputs, tag, err_max=0.0)
    assert r0['status'][0] == 0
    for key in ('sf', 'sr', 'order', 'dir', 'xi'):
        assert np.all(np.isfinite(r0[key])), key
    np.testing.assert_array_equal(r0['xi'], r['xi'])


# ------------------------------------------------------------------ 3. the DRC kernel
def drc_at_lane(P, inputs, c, kernel='lane'):
    s = D.system(P, inputs, c['name'])
    tof_terms = tuple(str(t) for t in c['tof_terms'])
    plan = s.plan(tof_terms)
    dyn, rn = [str(x) for x in c['dyn']], [str(x) for x in c['rnames']]
    Y = c['y'][[dyn.index(nm) for nm in plan.dyn]][:, None]
    rows = [rn.index(r) for r in plan.reactions]
    out = s.drc_at(tof_terms, Y, k=(c['kf'][rows][:, None], c['kr'][rows][:, None]), adjoint_kernel=kernel, **D.cond(c))
    return np.array([out[r] for r in rn]), out['tof0'], out['status']


@pytest.mark.parametrize('tag', [TAGS[0], TAGS[3], ('n', 2), ('n', 5), ('n', 6)],
                         ids=[TAG_IDS[0], TAG_IDS[3], 'l7_0', 'l8_1', 'pin_0'])
def test_drc_at_lane_is_sensitivity_at_lane_bitwise(P, inputs, tag):
    c = any_case(tag)
    xi, tof0, st = drc_at_lane(P, inputs, c)
    assert net_of(P, inputs, c).sens_lanes() == 1
    r = at1(P, inputs, tag)
    assert st[0] == 0
    np.testing.assert_array_equal(xi, r['xi'])
    np.testing.assert_array_equal(tof0, r['tof0'])


# ------------------------------------------------------------------ 4. divergence inside a wavefront
def interleaved(P, inputs, cases, n, status_in=None, k_zero_but=None, kernel='lane'):
    """sensitivity_at(adjoint_kernel=kernel) of n conditions, condition q the
    case cases[q % len(cases)]: its own state, rate constants and descriptors.
    k_zero_but = {position in `cases`: reaction}: that case's rate constants
    all 0 but the named reaction's, and its O* coverage set to its CO* one."""
    c0 = cases[0]
    s = D.system(P, inputs, c0['name'])
    tof_terms = tuple(str(t) for t in c0['tof_terms'])
    plan = s.plan(tof_terms)
    dyn, rn = [str(x) for x in c0['dyn']], [str(x) for x in c0['rnames']]
    rows = [rn.index(r) for r in plan.reactions]
    pick = [q % len(cases) for q in range(n)]
    Y = np.stack([cases[q]['y'][[dyn.index(nm) for nm in plan.dyn]] for q in pick], axis=1)
    kf = np.stack([cases[q]['kf'][rows] for q in pick], axis=1)
    kr = np.stack([cases[q]['kr'][rows] for q in pick], axis=1)
    for pos, keep in (k_zero_but or {}).items():
        m = np.array([r != keep for r in plan.reactions])
        for col in [q for q in range(n) if pick[q] == pos]:
            kf[m, col] = 0.0
            kr[m, col] = 0.0
            Y[plan.dyn.index('sO'), col] = Y[plan.dyn.index('sCO'), col]      # d net / d CO* = d net / d O*
    desc = {str(k): np.array([float(cases[q]['desc'][j]) for q in pick]) for j, k in enumerate(c0['desc_names'])}
    a = np.repeat(SG.scase(VOLCANO_ALL[0])['dir_a'][rows][None, :, None], n, axis=2)
    cc = np.repeat(SG.scase(VOLCANO_ALL[0])['dir_c'][rows][None, :, None], n, axis=2)
    out = s.sensitivity_at(tof_terms, Y, k=(kf, kr), T=np.full(n, float(c0['T'])), p=np.full(n, float(c0['p'])),
                           desc=desc, status_in=status_in, directions=(a, cc), adjoint_kernel=kernel)
    assert s.device(tof_terms).sens_lanes() == (1 if kernel == 'lane' else 16)
    flat = {key: np.array([out[key][x] for x in plan.reactions]) for key in ('xi', 'sf', 'sr')}
    flat['order'] = np.array([out['order'][x] for x in plan.fix]).reshape(len(plan.fix), n)
    for key in ('dir', 'tof0', 'status', 'err'):
        flat[key] = out[key]
    return flat


_ONE = {}


def volcano_singles(P, inputs, k_zero_but=None, kernel='lane'):
    """The n = 1 answer of each of the six volcano cases, by the named kernel."""
    key = (kernel,) + tuple(sorted((k_zero_but or {}).items()))
    if key not in _ONE:
        cases = [D.case(i) for i in VOLCANO_ALL]
        _ONE[key] = cases, [interleaved(P, inputs, [c], 1, k_zero_but={0: k_zero_but[pos]} if pos in (k_zero_but or {})
                                        else None, kernel=kernel) for pos, c in enumerate(cases)]
    return _ONE[key]


FLAT_KEYS = ('xi', 'sf', 'sr', 'order', 'dir', 'tof0', 'err')


def check_conditions_diverge(P, inputs, n, kernel):
    cases, one = volcano_singles(P, inputs, kernel=kernel)
    assert len(cases) == 6 and SG.FLAGGED[0] in VOLCANO_ALL
    sts = [int(o['status'][0]) for o in one]
    assert ST_SENS_PRECISION in sts and 0 in sts
    si = np.array([4 if q % 5 == 2 else 0 for q in range(n)], np.int32)
    r = interleaved(P, inputs, cases, n, status_in=si, kernel=kernel)
    for q in range(n):
        ref = one[q % 6]
        if si[q]:
            assert r['status'][q] == 4 and r['tof0'][q] == ref['tof0'][0]
            for key in ('xi', 'sf', 'sr', 'order', 'dir', 'err'):
                assert np.all(np.isnan(r[key][..., q])), (key, q)
        else:
            assert r['status'][q] == ref['status'][0], q
            for key in FLAT_KEYS:
                np.testing.assert_array_equal(r[key][..., q], ref[key][..., 0], err_msg='%s lane %d' % (key, q))


def check_singular_beside_regular(P, inputs, n, kernel):
    zero = {1: 'CO_ox'}
    cases, one = volcano_singles(P, inputs, zero, kernel=kernel)
    assert one[1]['status'][0] == ST_SENS_SINGULAR and np.isfinite(one[1]['tof0'][0]) and one[1]['tof0'][0] != 0.0
    assert np.all(np.isnan(one[1]['xi'])) and np.all(np.isnan(one[1]['dir']))
    r = interleaved(P, inputs, cases, n, k_zero_but=zero, kernel=kernel)
    for q in range(n):
        ref = one[q % 6]
        assert r['status'][q] == ref['status'][0], q
        for key in FLAT_KEYS:
            np.testing.assert_array_equal(r[key][..., q], ref[key][..., 0], err_msg='%s lane %d' % (key, q))
    assert np.count_nonzero(r['status'] == ST_SENS_SINGULAR) == len([q for q in range(n) if q % 6 == 1])


@pytest.mark.parametrize('n', [3, 63, 64, 65, 129])
def test_lanes_of_a_wavefront_diverge(P, inputs, n):
    """All six volcano cases interleaved in one call (different pivot orders,
    the flagged case among them), status_in 4 on every fifth lane: every lane
    is bitwise its own n = 1 answer; a gated lane has NaN outputs, a tof0 and
    keeps its 4."""
    check_conditions_diverge(P, inputs, n, 'lane')


@pytest.mark.parametrize('n', [3, 65])
def test_singular_lane_beside_regular_ones(P, inputs, n):
    """One case with every rate constant but CO_ox's zeroed and equal CO* and O*
    coverages: the rows of M for CO* and O* are identical (and the O2* row of
    the Jacobian is zero), neither a conservation row, so the elimination
    meets an exactly zero pivot -> status 7 (PCK_ST_SENS_SINGULAR, a handled
    status) and NaN on that lane alone; its neighbours are bitwise their n = 1
    answers."""
    check_singular_beside_regular(P, inputs, n, 'lane')


# The same two with adjoint_kernel='group' (csrc/mk_sens.h: k_sens_adjoint<16>;
# sens_lanes() == 16 is asserted in interleaved): the volcano has 4 species, so
# four conditions share one wavefront and one block.  n = 3, 4, 5, 9: a partly
# filled block, a full one, the first condition of the second and third blocks.
GROUP_N = [3, 4, 5, 9]


@pytest.mark.parametrize('n', GROUP_N)
def test_groups_of_a_wavefront_diverge(P, inputs, n):
    """As test_lanes_of_a_wavefront_diverge by the group kernel: the groups of a
    wavefront pivot differently and leave at different exits; every condition
    is bitwise its own n = 1 group-kernel answer, a gated one has NaN outputs,
    a tof0 and keeps its 4."""
    check_conditions_diverge(P, inputs, n, 'group')


@pytest.mark.parametrize('n', GROUP_N)
def test_singular_group_beside_regular_ones(P, inputs, n):
    """As test_singular_lane_beside_regular_ones by the group kernel: status 7
    and NaN on the singular condition alone, whose group leaves at the
    factorisation while the other groups of its wavefront go on."""
    check_singular_beside_regular(P, inputs, n, 'group')


# ------------------------------------------------------------------ 5. beyond the one-lane limit
def test_nine_species_refuse_lane_and_auto_takes_the_group_kernel(P, inputs):
    from make_edge_sizes_fixture import T as T_EDGE, T_END, TOF_TERM, edge_net
    from pycatkin_amd.functions.synthetic import synthetic_system
    efx = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'edge_sizes_fixture.npz')))
    s = synthetic_system(edge_net('e9'), t_end=T_END)[0]
    tof_terms = (TOF_TERM['e9'],)
    plan = s.plan(tof_terms)
    k = int(np.nonzero(efx['e9_regular'])[0][0])
    dyn = [str(x) for x in efx['e9_dyn']]
    Y = efx['e9_y'][k][[dyn.index(nm) for nm in plan.dyn]][:, None]
    kw = dict(T=[float(T_EDGE)], desc={'D%d' % q: [float(efx['desc'][k, q])] for q in range(4)})
    net = s.device(tof_terms)
    assert net.NDYN == 9
    with pytest.raises(RuntimeError, match=r'error -3: one-lane adjoint: at most 8 dynamic species'):
        s.drc_at(tof_terms, Y, adjoint_kernel='lane', **kw)
    with pytest.raises(RuntimeError, match=r'error -3'):
        s.sensitivity_at(tof_terms, Y, adjoint_kernel='lane', **kw)
    out = s.drc_at(tof_terms, Y, adjoint_kernel='auto', **kw)
    assert net.sens_lanes() == 16 and out['status'][0] == 0
    ref = s.drc_at(tof_terms, Y, adjoint_kernel='group', **kw)
    for r in plan.reactions:
        assert out[r][0] == ref[r][0]
    with pytest.raises(RuntimeError, match=r'error -1'):
        net.set_sens_lanes(3)


# ------------------------------------------------------------------ 6. descriptor sensitivities
DCASES = [LS.dcase(k) for k in range(len(LS.DNAMES))]
SIGMA = {'ECO': 0.1, 'EO': 0.2}
_DB = {}


def desc_batch(P, inputs):
    if 'r' not in _DB:
        s = D.system(P, inputs, 'volcano_')
        kw = dict(T=np.array([float(c['T']) for c in DCASES]), p=np.array([float(c['p']) for c in DCASES]),
                  desc={str(k): np.array([float(c['desc'][q]) for c in DCASES])
                        for q, k in enumerate(DCASES[0]['desc_names'])})
        _DB['r'] = s.descriptor_sensitivity_batch(('CO_ox',), desc_sigma=SIGMA, **kw)
        _DB['lanes'] = s.device(('CO_ox',)).sens_lanes()
    return _DB['r']


def test_descriptor_sensitivity_batch_vs_fixture(P, inputs):
    """The solve, the stencils and the adjoint together from the default start
    state: d ln TOF / d desc within 2 |ddesc_pert - ref| + 2 |ddesc_2h - ref| +
    1e-10 |ref| (the root, the stencil, the device's rate constants against the
    oracle's), and within 10 |ddesc_fd - ref| of the oracle's own finite
    difference; one lane per condition by default."""
    out = desc_batch(P, inputs)
    assert _DB['lanes'] == 1
    assert np.all(out['status'] == 0), out['status']
    assert sorted(out['dlntof_ddesc']) == ['ECO', 'EO'] and out['nsteps'].shape == (3,)
    miss = []
    for k, c in enumerate(DCASES):
        for q, name in enumerate(c['ddesc_names']):
            got, ref = out['dlntof_ddesc'][str(name)][k], c['ddesc_ref'][q]
            allow = 2.0 * abs(c['ddesc_pert'][q] - ref) + 2.0 * abs(c['ddesc_2h'][q] - ref) + 1e-10 * abs(ref)
            allow_fd = 10.0 * abs(c['ddesc_fd'][q] - ref)
            print('%s d ln TOF / d %s: %.9f, |out - ref| %.3e (allowed %.3e), |out - fd| %.3e (allowed %.3e)'
                  % (c['name'], name, got, abs(got - ref), allow, abs(got - c['ddesc_fd'][q]), allow_fd))
            if not (abs(got - ref) <= allow and abs(got - c['ddesc_fd'][q]) <= allow_fd):
                miss.append((c['name'], str(name)))
        assert abs(out['tof0'][k] - float(c['tof_ref'])) <= 1e-6 * abs(float(c['tof_ref']))
    assert not miss, miss


def test_std_lntof_is_the_formula_on_the_returned_gradients(P, inputs):
    out = desc_batch(P, inputs)
    g = out['dlntof_ddesc']
    np.testing.assert_array_equal(out['std_lntof'], np.sqrt((g['ECO'] * SIGMA['ECO']) ** 2 + (g['EO'] * SIGMA['EO']) ** 2))
    assert np.all(out['std_lntof'] > 0.0)


@pytest.mark.parametrize('k', range(len(DCASES)), ids=LS.DNAMES)
def test_descriptor_sensitivity_at_fixture_states(P, inputs, k):
    """At the fixture's state and rate constants the root term is gone: the
    kernel's own bound, 1e-12 (1 + |ref|) + 10 |ddesc_104 - ref|."""
    c = DCASES[k]
    s = D.system(P, inputs, c['name'])
    plan = s.plan(('CO_ox',))
    dyn, rn = [str(x) for x in c['dyn']], [str(x) for x in c['rnames']]
    Y = c['y'][[dyn.index(nm) for nm in plan.dyn]][:, None]
    rows = [rn.index(r) for r in plan.reactions]
    out = s.descriptor_sensitivity_at(('CO_ox',), Y, k=(c['kf'][rows][:, None], c['kr'][rows][:, None]), **D.cond(c))
    assert s.device(('CO_ox',)).sens_lanes() == 1 and out['status'][0] == 0
    got = np.array([out['dlntof_ddesc'][str(x)][0] for x in c['ddesc_names']])
    allow = 1e-12 * (1.0 + np.abs(c['ddesc_ref'])) + 10.0 * np.abs(c['ddesc_104'] - c['ddesc_ref'])
    err = np.abs(got - c['ddesc_ref'])
    print('%s: |out - ref| %s (allowed %s)' % (c['name'], err, allow))
    assert np.all(err <= allow), (c['name'], err, allow)
    xi = np.array([out['xi'][x][0] for x in rn])
    assert np.all(D.within(xi, c['xi_ref']))


# ------------------------------------------------------------------ 7. against the device's own finite difference
def test_eco_gradient_vs_device_finite_difference(P, inputs):
    """dlntof_ddesc['ECO'] at (-1, -1) against the central difference of ln tof of
    a 2-condition solve_batch at ECO +- 1e-3 eV.  Allowed: 10 |ddesc_fd - ref| of
    the fixture (what the oracle's own difference quotient misses the limit by:
    the O(h^2) term and its solves) plus the solve's 1e-6 parity on each of the
    two TOFs over 2 h."""
    c = DCASES[0]
    assert c['name'] == 'volcano_-1_-1'
    out = desc_batch(P, inputs)
    s = D.system(P, inputs, c['name'])
    eco, eo = (float(c['desc'][list(c['desc_names']).index(k)]) for k in ('ECO', 'EO'))
    r = s.solve_batch(tof_terms=('CO_ox',), steady=True, T=np.full(2, float(c['T'])), p=np.full(2, float(c['p'])),
                      desc={'ECO': np.array([eco + H, eco - H]), 'EO': np.full(2, eo)})
    assert np.all(r['status'] == 0), r['status']
    fd = (np.log(r['tof'][0]) - np.log(r['tof'][1])) / (2.0 * H)
    got = out['dlntof_ddesc']['ECO'][0]
    tol = 10.0 * abs(c['ddesc_fd'][0] - c['ddesc_ref'][0]) + 2.0e-6 / (2.0 * H)
    print('d ln TOF / d ECO %.9f, device finite difference %.9f, |difference| %.3e, tolerance %.3e'
          % (got, fd, abs(got - fd), tol))
    assert abs(got - fd) <= tol
