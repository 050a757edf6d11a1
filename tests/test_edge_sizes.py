"""Host side of the size and packing limits (no device): the edge_network
helper (tests/_synth.py), the oracle fixture of tests/golden/
make_edge_sizes_fixture.py, and the plan layer's refusals (network.py:
compile_system) at 65 species, 257 reactions and 17 TOF terms.  The device
side is tests/test_gpu_edge_sizes.py."""
import os
import sys

import numpy as np
import pytest

from oracle import mk_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
from make_edge_sizes_fixture import (FIXTURE_KEYS, MIN_REGULAR, MIN_TOF_RATIO, N, NETS, P6_INDEX,  # noqa: E402
                                     ROOT_DIST, STEADY_ATOL, T, T_END, T_OUT, TOF_TERM, X_EXP, X_INDEX, edge_net)

FIXTURE = os.path.join(HERE, 'golden', 'edge_sizes_fixture.npz')


@pytest.fixture(scope='module')
def fx():
    return dict(np.load(FIXTURE))


def _plan(net, tof_terms=()):
    from pycatkin_amd.functions.synthetic import synthetic_system
    return synthetic_system(net)[0].plan(tuple(tof_terms))


def test_edge_network_is_deterministic_and_connected():
    """edge_network: the same dict for the same seed, another for another;
    the first two reactions are the adsorptions, the chain reaches every
    adsorbate, `extra` follows the chain, every step conserves sites; 3 to 64
    species; synthetic_network's stream is untouched (its own generator)."""
    from _synth import edge_network
    from pycatkin_amd.functions.synthetic import synthetic_network
    before = synthetic_network(n_species=12, n_reactions=36, seed=1)
    extra = ((['A2'] * 3, ['A3', 's', 's']),)
    a, b = edge_network(12, 30, 4, extra=extra), edge_network(12, 30, 4, extra=extra)
    after = synthetic_network(n_species=12, n_reactions=36, seed=1)
    assert before['reactions'] == after['reactions'] and before['E0'].tolist() == after['E0'].tolist()
    assert a['reactions'] == b['reactions'] and a['adsorbates'] == b['adsorbates']
    for f in ('E0', 'Ed', 'beta'):
        assert a[f].tolist() == b[f].tolist()
    assert edge_network(12, 30, 5, extra=extra)['E0'].tolist() != a['E0'].tolist()
    assert set(a) == set(before)
    assert a['reactions'][12] == ('surf',) + extra[0]
    for ns, nr in ((3, 3), (3, 7), (4, 9), (8, 28), (64, 256)):
        net = edge_network(ns, nr, 0)
        rx = net['reactions']
        assert len(net['adsorbates']) == ns - 1 and len(rx) == nr and len(net['beta']) == nr
        assert rx[0] == ('ads', ['G0', 's'], ['A0']) and rx[1][0] == 'ads' and rx[1][1] == ['G1', 's', 's']
        made = {'A0'}
        for k in range(1, ns - 1):                                 # the chain: A_i -> A_k from an earlier A_i
            kind, reac, prod = rx[1 + k]
            assert kind == 'surf' and prod == ['A%d' % k] and len(reac) == 1 and reac[0] in made
            made.add(prod[0])
        assert made == set(net['adsorbates'])
        for kind, reac, prod in rx:
            sites = lambda side: sum(1 for s in side if not s.startswith('G'))  # noqa: E731
            assert sites(reac) == sites(prod)
        plan = _plan(net)
        assert len(plan.dyn) == ns and len(plan.reactions) == nr
    for bad in (2, 65):
        with pytest.raises(ValueError):
            edge_network(bad, 80, 0)
    # further gases adsorb molecularly after the chain and `extra`; the first two keep their reactions
    g4 = edge_network(12, 30, 4, n_gases=4, extra=extra)
    assert g4['reactions'][:13] == a['reactions'][:13] and len(g4['gases']) == 4
    assert g4['reactions'][13:15] == [('ads', ['G2', 's'], ['A1']), ('ads', ['G3', 's'], ['A2'])]
    plan = _plan(g4)
    assert len(plan.fix) == 4 and len(plan.reactions) == 30


@pytest.mark.parametrize('key', sorted(NETS))
def test_edge_plans_have_the_sizes_of_the_table(key):
    """Every network under test builds a plan with its species and reaction
    counts, one site balance over all species; e8a / e8b sit on the two
    sides of the one-lane path's LDS rule (mk_solver.h lds_bytes(R, 8, 128)
    <= 64 KiB up to R = 28); p6's wide reaction holds plan index 0 and 63."""
    net = edge_net(key)
    plan = _plan(net, ('R0',))
    ns, nr, _ = NETS[key]
    assert len(plan.dyn) == ns and len(plan.reactions) == nr and plan.conservation.shape == (1, ns)
    assert plan.reactions == ['R%d' % j for j in range(nr)]
    if key in X_EXP:
        kind, reac, prod = net['reactions'][X_INDEX]
        assert reac == ['A2'] * X_EXP[key] and prod == ['A3'] + ['s'] * (X_EXP[key] - 1)
    if key == 'p6':
        _, reac, prod = net['reactions'][2 + 62]
        q = sorted(plan.dyn.index(nm) for nm in reac + prod)
        assert len(set(q)) == 6 and q[0] == 0 and q[5] == 63, q


@pytest.mark.parametrize('key', ['x3', 'x31', 'limit8'])
def test_edge_power_step_counts_in_the_rates(key):
    """At the conditions of the device test (test_gpu_edge_sizes.
    rate_inputs) the net rate of the `e` A2 <-> A3 + (e - 1) s step stands
    above 1e-6 of the largest |f| at every condition, and each direction
    alone at one condition at least: the step cannot hide under the 1e-12
    floor of the comparison."""
    from _synth import spec_of
    from test_gpu_edge_sizes import limit_net, rate_inputs
    net, j, e = (limit_net(8, 28, 'both'), 8, 32) if key == 'limit8' else (edge_net(key), X_INDEX, X_EXP[key])
    dyn = list(_plan(net).dyn)
    n, D, Tn, y = rate_inputs(dyn, raised=('A2', 's'))
    fwd, rev = [], []
    for c in range(n):
        m = O.ClassicModel(spec_of(net, D[c], Tn[c]), T=Tn[c])
        full = m.y0.copy()
        pos = [m.idx[nm] for nm in dyn]
        full[pos] = y[:, c]
        big = np.abs(m.rhs(full)[pos]).max()
        rf, rr = m.rates(full)[m.rnames.index('R%d' % j)]
        assert np.isfinite(m.jac(full)).all()
        assert abs(rf - rr) > 1e-6 * big, (c, rf, rr, big)
        fwd.append(rf > 1e-6 * big)
        rev.append(rr > 1e-6 * big)
    assert any(fwd) and any(rev), (fwd, rev)


def test_edge_wide_step_counts_in_the_rates():
    """p6's six-participant step at the conditions of the device test: both
    directions stand above 1e-6 of the largest rate and of the largest |f|,
    and its derivative by the sixth participant (the site s, plan index 63:
    kr c3 c4, the only use of bits 26..31 of the CSR entry) above 1e-6 of the
    largest Jacobian entry -- six orders above the comparison's floors."""
    from _synth import spec_of
    from test_gpu_edge_sizes import rate_inputs
    net = edge_net('p6')
    dyn = list(_plan(net).dyn)
    _, reac, prod = net['reactions'][P6_INDEX]
    assert dyn.index(prod[2]) == 63 and dyn.index(reac[0]) == 0
    n, D, Tn, y = rate_inputs(dyn)
    for c in range(n):
        m = O.ClassicModel(spec_of(net, D[c], Tn[c]), T=Tn[c])
        full = m.y0.copy()
        pos = [m.idx[nm] for nm in dyn]
        full[pos] = y[:, c]
        rates, J = m.rates(full), m.jac(full)[np.ix_(pos, pos)]
        j = m.rnames.index('R%d' % P6_INDEX)
        dcol = m.kr[j] * y[dyn.index(prod[0]), c] * y[dyn.index(prod[1]), c]
        assert rates[j].min() > 1e-6 * np.abs(rates).max(), (c, rates[j], np.abs(rates).max())
        assert rates[j].min() > 1e-6 * np.abs(m.rhs(full)[pos]).max()
        assert dcol > 1e-6 * np.abs(J).max(), (c, dcol, np.abs(J).max())
        # and the column of s holds that term on the rows of the five adsorbates
        rows = [dyn.index(nm) for nm in reac + prod[:2]]
        assert np.all(np.abs(J[rows, 63]) > 1e-6 * np.abs(J).max()), (c, J[rows, 63])


@pytest.mark.parametrize('key', FIXTURE_KEYS)
def test_edge_sizes_fixture_reproduces(fx, key):
    """The oracle answered all 8 conditions of every network and found at
    least 6 regular; re-run here at two conditions (the LSODA transient at
    1e-12 / 1e-20 and the steady rule) it gives the fixture's rows at rtol
    1e-9, over the species of the product's plan."""
    from scipy.integrate import solve_ivp
    from _synth import spec_of
    net = edge_net(key)
    plan = _plan(net, ('R0',))
    assert list(plan.dyn) == [str(x) for x in fx[key + '_dyn']]
    assert fx[key + '_ok'].shape == (N,) and fx[key + '_ok'].all()
    assert fx[key + '_regular'].sum() >= MIN_REGULAR
    # the TOF term's net rate does not cancel: a relative bound on it means something
    assert np.all(np.abs(fx[key + '_tof']) >= MIN_TOF_RATIO * fx[key + '_tofabs']), fx[key + '_tof'] / fx[key + '_tofabs']
    np.testing.assert_array_equal(fx['t_out'], T_OUT)
    for k in (0, N - 1):
        m = O.ClassicModel(spec_of(net, fx['desc'][k], float(T)), T=float(T))
        m._set_reach(m.y0)
        sol = solve_ivp(lambda t, y: m.rhs(y), (0.0, T_OUT[-1]), m.y0, method='LSODA', jac=lambda t, y: m.jac(y),
                        rtol=1e-12, atol=1e-20, t_eval=T_OUT)
        assert sol.status == 0
        np.testing.assert_allclose(sol.y[m.dyn].T, fx[key + '_traj'][k], rtol=1e-9, atol=1e-20)
        r = O.steady_rule(m, dist=ROOT_DIST, dist_atol=STEADY_ATOL, budget=400000, t_end=T_END)
        assert bool(r['regular']) == bool(fx[key + '_regular'][k])
        np.testing.assert_allclose(r['y'][m.dyn], fx[key + '_y'][k], rtol=1e-9, atol=1e-25)
        tofabs = np.abs(m.rates(r['y'])[m.rnames.index(TOF_TERM[key])]).sum()
        np.testing.assert_allclose(tofabs, fx[key + '_tofabs'][k], rtol=1e-9)
        np.testing.assert_allclose(m.tof(r['y'], [TOF_TERM[key]]), fx[key + '_tof'][k], rtol=1e-9)


def _grown(net):
    """`net` plus one adsorbate, made from A0 by one more chain step"""
    ads = net['adsorbates'] + ['A%d' % len(net['adsorbates'])]
    return dict(net, adsorbates=ads, reactions=net['reactions'] + [('surf', ['A0'], [ads[-1]])],
                E0=np.append(net['E0'], -0.5), Ed=np.vstack([net['Ed'], [0.5, 0.0, 0.0, 0.0]]),
                beta=np.append(net['beta'], 0.7))


def test_plan_layer_refuses_oversize_networks():
    """System.plan (network.py: compile_system) raises ValueError for 65
    dynamic species, 257 reactions and 17 TOF terms (MAX_DYN, MAX_RXN,
    MAX_TOF of _lib.py = PCK_MAX_DYN / _RXN / _TOF) and accepts 64, 256 and
    16."""
    from _synth import edge_network
    from pycatkin_amd import _lib as L
    assert (L.MAX_DYN, L.MAX_RXN, L.MAX_TOF) == (64, 256, 16)
    plan = _plan(edge_network(64, 255, 0))
    assert len(plan.dyn) == 64 and len(plan.reactions) == 255
    with pytest.raises(ValueError, match='65 dynamic species'):
        _plan(_grown(edge_network(64, 255, 0)))
    plan = _plan(edge_network(16, 256, 0))
    assert len(plan.reactions) == 256
    with pytest.raises(ValueError, match='257 active reactions'):
        _plan(edge_network(16, 257, 0))
    net = edge_net('e17')
    plan = _plan(net, ['R%d' % j for j in range(16)])
    assert len(plan.ip) > 0
    with pytest.raises(ValueError, match='too many TOF terms'):
        _plan(net, ['R%d' % j for j in range(17)])
