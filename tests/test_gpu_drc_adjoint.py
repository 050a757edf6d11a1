"""The analytic degree of rate control on the device (csrc/mk_sens.h over
csrc/mk_adjoint.h:
k_drc_adjoint; pck_drc_at, pck_drc_adjoint; System.drc_at,
System.drc_batch(method='analytic')) against tests/golden/
drc_adjoint_fixture.npz (make_drc_adjoint_fixture.py: the adjoint formula of
tests/_sens.py at 400 bits, at the oracle's steady states).

The bound of the kernel itself, |xi - xi_ref| <= 1e-12 + 1e-12 |xi_ref|, is a
sandwich: the same algorithm at 104 bits (the fixture's xi_104, asserted here
within 1e-14 of xi_ref) passes it by four orders, at 80 bits it misses by
4.7e-10 and in fp64 by 5e-2 (DMTM, 400 K; DESIGN.md "Analytic DRC")."""
import copy
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
FIXTURE = os.path.join(HERE, 'golden', 'drc_adjoint_fixture.npz')
FX = dict(np.load(FIXTURE))
NAMES = [str(x) for x in FX['names']]
REGULAR = [i for i in range(len(NAMES)) if bool(FX['c%d_regular' % i])]
ABS, REL = 1e-12, 1e-12                      # the kernel's bound (test 1)
ST_NONFINITE, ST_NEWTON = 3, 4


def case(i):
    pre = 'c%d_' % i
    c = {k[len(pre):]: v for k, v in FX.items() if k.startswith(pre)}
    c['name'] = NAMES[i]
    return c


def idx(prefix):
    return [i for i, nm in enumerate(NAMES) if nm.startswith(prefix)]


@pytest.fixture(scope='module')
def P():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    import pycatkin_amd
    return pycatkin_amd


_SYS = {}


def system(P, inputs, name):
    """The product's System of a fixture case (one per network and process)."""
    key = name.split('_')[0]
    if key in _SYS:
        return _SYS[key]
    if key == 'dmtm':
        s = P.read_from_input_file(os.path.join(inputs, 'DMTM', 'input.json'))
    elif key == 'cstr':
        s = P.read_from_input_file(os.path.join(inputs, 'COOxReactor', 'input_Pd111.json'))
    elif key == 'volcano':
        from pycatkin_amd.functions.volcano import set_volcano_energies
        s = P.read_from_input_file(os.path.join(inputs, 'COOxVolcano', 'input.json'))
        set_volcano_energies(s)
    elif key in ('syn12', 'syn24', 'syn40'):
        from make_synthetic_sizes_fixture import NETS, SEED_NET, T_END
        from pycatkin_amd.functions.synthetic import synthetic_network, synthetic_system
        ns, nr = NETS[key]
        s = synthetic_system(synthetic_network(n_species=ns, n_reactions=nr, seed=SEED_NET), t_end=T_END)[0]
    elif key == 'e64':
        from make_edge_sizes_fixture import T_END, edge_net
        from pycatkin_amd.functions.synthetic import synthetic_system
        s = synthetic_system(edge_net('e64'), t_end=T_END)[0]
    elif key == 'butadiene':
        from make_butadiene_fixture import CASES, kept_reactions
        from pycatkin_amd.functions.load_input import read_from_input_file
        d = os.path.join(inputs, 'Butadiene')
        dft = read_from_input_file(os.path.join(d, 'input.json'))
        s = copy.deepcopy(read_from_input_file(os.path.join(d, 'input_mkm.json'), base_system=dft))
        cname = name[len('butadiene_'):name.rindex('_')]
        keep = kept_reactions(list(s.reactions), cname, dict(CASES)[cname])
        for r in list(s.reactions):
            if r not in keep:
                del s.reactions[r]
        s.names_to_indices()
    else:
        raise KeyError(name)
    _SYS[key] = s
    return s


def cond(c, n=1):
    return dict(T=np.full(n, float(c['T'])), p=np.full(n, float(c['p'])),
                desc={str(k): np.full(n, float(v)) for k, v in zip(c['desc_names'], c['desc'])} or None)


def at_fixture_state(P, inputs, c, n=1, tof_terms=None, k_scale=None, status_in=None):
    """System.drc_at at the fixture's state and rate constants, tiled to n
    conditions -> (xi [R, n] over the fixture's reactions, tof0, status)."""
    s = system(P, inputs, c['name'])
    tof_terms = tuple(str(t) for t in c['tof_terms']) if tof_terms is None else tof_terms
    plan = s.plan(tof_terms)
    dyn, rn = [str(x) for x in c['dyn']], [str(x) for x in c['rnames']]
    assert sorted(plan.dyn) == sorted(dyn)
    Y = np.repeat(c['y'][[dyn.index(nm) for nm in plan.dyn]][:, None], n, axis=1)
    rows = [rn.index(r) for r in plan.reactions]
    kf, kr = c['kf'][rows].copy(), c['kr'][rows].copy()
    if k_scale is not None:
        for name, f in k_scale.items():
            kf[plan.reactions.index(name)] *= f
            kr[plan.reactions.index(name)] *= f
    k = (np.repeat(kf[:, None], n, axis=1), np.repeat(kr[:, None], n, axis=1))
    out = s.drc_at(tof_terms, Y, k=k, status_in=status_in, **cond(c, n))
    return np.array([out[r] for r in rn]), out['tof0'], out['status']


_AT = {}


def at1(P, inputs, i):
    if i not in _AT:
        _AT[i] = at_fixture_state(P, inputs, case(i))
    return _AT[i]


def within(xi, ref):
    return np.abs(xi - ref) <= ABS + REL * np.abs(ref)


# ------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize('i', REGULAR, ids=[NAMES[i] for i in REGULAR])
def test_drc_at_fixture_states(P, inputs, i):
    """pck_drc_at at the fixture's states and rate constants vs xi_ref:
    |xi - xi_ref| <= 1e-12 + 1e-12 |xi_ref|, tof0 to 1e-12 relative; the
    fixture's own 104-bit run within 1e-14.  Covers G = 16 (DMTM, the CSTR,
    the volcano, syn12), 32 (syn24) and 64 (syn40, e64) and the pinned rows
    (Butadiene)."""
    c = case(i)
    assert np.all(np.abs(c['xi_104'] - c['xi_ref']) <= 1e-14 + 1e-14 * np.abs(c['xi_ref']))
    xi, tof0, st = at1(P, inputs, i)
    err = np.abs(xi[:, 0] - c['xi_ref'])
    print('%s: worst |xi - xi_ref| %.3e, tof0 rel %.3e' % (c['name'], err.max(),
                                                           abs(tof0[0] - c['tof_ref']) / abs(c['tof_ref'])))
    assert st[0] == 0
    assert np.all(within(xi[:, 0], c['xi_ref'])), (c['name'], err.max(), int(np.argmax(err)))
    assert abs(tof0[0] - c['tof_ref']) <= 1e-12 * abs(c['tof_ref'])


# ------------------------------------------------------------------ 2. the full path
FULL = idx('dmtm_') + idx('syn24_') + [i for i in idx('volcano_') if i in REGULAR]


def full_path(P, inputs, ids):
    """drc_batch(method='analytic') from the default start state, the cases
    `ids` (one network) in one launch -> (dict, plan reactions)"""
    cs = [case(i) for i in ids]
    s = system(P, inputs, cs[0]['name'])
    tof_terms = tuple(str(t) for t in cs[0]['tof_terms'])
    kw = dict(T=np.array([float(c['T']) for c in cs]), p=np.array([float(c['p']) for c in cs]))
    if len(cs[0]['desc_names']):
        kw['desc'] = {str(k): np.array([float(c['desc'][q]) for c in cs]) for q, k in enumerate(cs[0]['desc_names'])}
    if cs[0]['name'].startswith('dmtm'):
        # the default steady tolerances, to t_end = 1e14 s: at 400 K / 1e4 Pa (TOF
        # 7e-14 / s) the transient is still 2e-5 from its root at the input's
        # 1e12 s (mk_oracle.steady_rule: crit 2.0e-5, status 4) and on it at
        # 1e14 s (crit 1.7e-11)
        kw.update(t_end=1e14)
    return s, kw, tof_terms, cs


@pytest.mark.parametrize('key', ['dmtm_', 'syn24_', 'volcano_'])
def test_drc_batch_analytic_vs_fixture(P, inputs, key):
    """The solve and the adjoint together: every status 0, xi within
    2 max_j |xi_pert - xi_ref| + the kernel's bound of xi_ref, where xi_pert is
    xi_ref recomputed at the root moved by 1e-6 relative in every species (the
    parity bound the steady solve is held to, test_gpu_group.py)."""
    ids = [i for i in FULL if NAMES[i].startswith(key)]
    s, kw, tof_terms, cs = full_path(P, inputs, ids)
    out = s.drc_batch(tof_terms, steady=True, method='analytic', **kw)
    assert np.all(out['status'] == 0), out['status']
    for k, c in enumerate(cs):
        xi = np.array([out[str(r)][k] for r in c['rnames']])
        allow = 2.0 * np.max(np.abs(c['xi_pert'] - c['xi_ref'])) + ABS + REL * np.abs(c['xi_ref'])
        err = np.abs(xi - c['xi_ref'])
        print('%s: worst |xi - xi_ref| %.3e (allowed %.3e), nsteps %d' % (c['name'], err.max(), allow.min(),
                                                                         out['nsteps'][k]))
        assert np.all(err <= allow), (c['name'], err.max(), allow.min())
        assert abs(out['tof0'][k] - c['tof_ref']) <= 1e-6 * abs(c['tof_ref'])


# ------------------------------------------------------------------ 3. analytic vs finite differences
def test_analytic_vs_device_fd_dmtm(P, inputs):
    """method='analytic' against the device's own method='fd' at eps 1e-3 on
    the four DMTM conditions: within 10 x the oracle FD's distance from the
    exact limit, max |xi_fd - xi_ref| over the fixture's DMTM conditions at
    450 K and above (3.2e-6, at 450 K; at 400 K, TOF 7e-14 / s, the oracle's
    own difference quotient is 1.1e-3 away and sets no yardstick)."""
    ids = idx('dmtm_')
    s, kw, tof_terms, cs = full_path(P, inputs, ids)
    bound = 10.0 * max(np.max(np.abs(c['xi_fd'] - c['xi_ref'])) for c in cs if float(c['T']) >= 450.0)
    assert bound <= 10.0 * 3.3e-6
    a = s.drc_batch(tof_terms, steady=True, method='analytic', **kw)
    f = s.drc_batch(tof_terms, steady=True, method='fd', eps=1e-3, **kw)
    assert np.all(a['status'] == 0) and np.all(f['status'] == 0), (a['status'], f['status'])
    for k, c in enumerate(cs):
        d = np.array([abs(a[str(r)][k] - f[str(r)][k]) for r in c['rnames']])
        print('%s: worst |analytic - fd| %.3e (bound %.3e)' % (c['name'], d.max(), bound))
    for k, c in enumerate(cs):
        d = np.array([abs(a[str(r)][k] - f[str(r)][k]) for r in c['rnames']])
        assert d.max() <= bound, (c['name'], d.max(), bound)


# ------------------------------------------------------------------ 4. sum rule
@pytest.mark.parametrize('i', [i for i in REGULAR if not NAMES[i].startswith('cstr')],
                         ids=[NAMES[i] for i in REGULAR if not NAMES[i].startswith('cstr')])
def test_sum_rule(P, inputs, i):
    """sum_j xi_j = 1 within 1e-6 (the bound of the FD tests) on every
    infinite-dilution case; the CSTR's flow rate is not scaled with the k's."""
    xi, _, _ = at1(P, inputs, i)
    assert abs(xi[:, 0].sum() - 1.0) <= 1e-6, xi[:, 0].sum()


# ------------------------------------------------------------------ 5. statuses
def test_not_reached_conditions_pass_their_status_through(P, inputs):
    """The two volcano corners the steady rule does not accept keep status 4
    through drc_batch(method='analytic'): NaN xi, a finite tof0; the regular
    points of the same launch answer as alone."""
    ids = idx('volcano_')
    corners = [k for k, i in enumerate(ids) if i not in REGULAR]
    assert len(corners) == 2
    s, kw, tof_terms, cs = full_path(P, inputs, ids)
    out = s.drc_batch(tof_terms, steady=True, method='analytic', **kw)
    for k, c in enumerate(cs):
        xi = np.array([out[str(r)][k] for r in s.plan(tof_terms).reactions])
        if k in corners:
            assert out['status'][k] == ST_NEWTON, (c['name'], out['status'])
            assert np.all(np.isnan(xi)) and np.isfinite(out['tof0'][k])
        else:
            assert out['status'][k] == 0
            ref = np.array([c['xi_ref'][[str(x) for x in c['rnames']].index(r)] for r in s.plan(tof_terms).reactions])
            allow = 2.0 * np.max(np.abs(c['xi_pert'] - c['xi_ref'])) + ABS + REL * np.abs(ref)
            assert np.all(np.abs(xi - ref) <= allow), (c['name'], xi, ref)


def test_status_in_gates_conditions(P, inputs):
    """pck_drc_at with status_in = [0, 4, 0, 4, 0]: the 0 rows are the n = 1
    answer bitwise, the others keep 4 and get NaN xi and a tof0."""
    i = idx('dmtm_')[1]
    ref, tref, _ = at1(P, inputs, i)
    si = np.array([0, 4, 0, 4, 0], np.int32)
    xi, tof0, st = at_fixture_state(P, inputs, case(i), n=5, status_in=si)
    assert st.tolist() == si.tolist()
    assert np.all(np.isnan(xi[:, si != 0])) and np.all(np.isfinite(tof0))
    for k in np.nonzero(si == 0)[0]:
        np.testing.assert_array_equal(xi[:, k], ref[:, 0])
        assert tof0[k] == tref[0]


def test_zero_tof_is_nonfinite(P, inputs):
    """A TOF term whose kf = kr = 0 (DMTM, tof_terms = r9 alone with both rate
    constants zeroed): TOF0 = 0 -> PCK_ST_NONFINITE and NaN xi."""
    c = case(idx('dmtm_')[2])
    xi, tof0, st = at_fixture_state(P, inputs, c, tof_terms=('r9',), k_scale={'r9': 0.0})
    assert st[0] == ST_NONFINITE and tof0[0] == 0.0
    assert np.all(np.isnan(xi))


# ------------------------------------------------------------------ 6. geometry
@pytest.mark.parametrize('key,n', [('dmtm_', 3), ('dmtm_', 5), ('dmtm_', 63), ('dmtm_', 65), ('syn24_', 3),
                                   ('syn24_', 65)])
def test_tiled_conditions_are_bitwise_equal(P, inputs, key, n):
    """G = 16 packs 4 conditions into a wavefront, G = 32 two: n copies of
    one condition (ragged last wavefronts at 3, 5, 63, 65) all equal the n = 1
    answer bitwise -- no leak between the conditions of a wavefront."""
    i = idx(key)[0]
    ref, tref, _ = at1(P, inputs, i)
    xi, tof0, st = at_fixture_state(P, inputs, case(i), n=n)
    assert np.all(st == 0)
    np.testing.assert_array_equal(xi, np.repeat(ref, n, axis=1))
    np.testing.assert_array_equal(tof0, np.repeat(tref, n))


# ------------------------------------------------------------------ 7. the largest network
def test_e64_full_group(P, inputs):
    """64 species, reaction index 255: G = 64, the 64 x 64 double-double
    matrix is the launch's whole LDS block, 64 KiB for the one condition of a
    wavefront.  Finite and within the kernel's bound."""
    i = idx('e64_')[0]
    c = case(i)
    s = system(P, inputs, c['name'])
    net = s.device(tuple(str(t) for t in c['tof_terms']))
    assert net.NDYN == 64 and net.NRXN == 256
    xi, tof0, st = at1(P, inputs, i)
    assert st[0] == 0 and np.all(np.isfinite(xi))
    assert np.all(within(xi[:, 0], c['xi_ref']))


# ------------------------------------------------------------------ 8. pinned species
def test_pinned_species_butadiene(P, inputs):
    """Butadiene with_jonas_byproducts: the species no reaction can produce sit
    at exactly 0 with an exactly zero rate and get unit rows (newton_pinned;
    the reference has them on the oracle's `unreach`).  Finite, within the
    kernel's bound, and exactly 0 for every reaction that runs in neither
    direction (the fixture's `dead`: both rates exactly 0 -- the reactions
    among unreachable species)."""
    i = idx('butadiene_')[0]
    c = case(i)
    assert c['unreach'].any() and c['dead'].any()
    xi, tof0, st = at1(P, inputs, i)
    assert st[0] == 0 and np.all(np.isfinite(xi))
    assert np.all(within(xi[:, 0], c['xi_ref']))
    assert np.all(xi[c['dead'], 0] == 0.0)
