"""The lane-group kernels (csrc/mk_group.h, csrc/mk_quad.h, dispatch in
csrc/mk_kernels.hip) at the sizes where they switch and the values where
their packed records run out: tests/golden/make_edge_sizes_fixture.py lists
the networks (tests/_synth.py: edge_network) and what each pins.

  a. rates, Jacobian, rate constants and reaction rates of every network
     against the oracle's model at 5 conditions (a ragged last wavefront at
     4, 2 and 1 groups per wavefront): rtol 1e-10, floor 1e-12 x the largest
     entry (the bound of test_synthetic_rates_jacobian_vs_oracle);
  b. trajectories and steady solves against tests/golden/
     edge_sizes_fixture.npz: 1e-6 relative with a 1e-12 floor on the dense
     output (test_synthetic_trajectory_on_32_lane_groups), the bounds and the
     flip rule of test_synthetic_sizes_steady_vs_oracle on the steady rule;
  c. the kernel variants of one size against each other;
  d. the limits: 16 TOF terms, exponent 32 and seven participants refused
     on the group path and served on the one-lane path.

Every network is built once per process (module cache) and every kernel
variant compiled once (the library caches hipRTC kernels by the network's
digest), so a later case of the same network pays no second compile."""
import os
import sys
import time

import numpy as np
import pytest

from oracle import mk_oracle as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
from make_edge_sizes_fixture import (FIXTURE_KEYS, MIN_REGULAR, NETS, P6_INDEX, ROOT_DIST, T, T_END,  # noqa: E402
                                     TOF_TERM, X_EXP, X_INDEX, edge_net, power_reaction, tune_power_reaction)

FIXTURE = os.path.join(HERE, 'golden', 'edge_sizes_fixture.npz')
ALL_KEYS = FIXTURE_KEYS + ('p6',)
# lanes per condition of the solver kernel the size selects (0: one-lane path)
LANES = {'e8a': 0, 'e8b': 4, 'e9': 4, 'e16': 4, 'e17': 32, 'e32': 32, 'e33': 64, 'e64': 64, 'x3': 4, 'x31': 4}
JIT_PLAN = 100              # DeviceNetwork.plan_id(): the hipRTC-specialised one-lane plan


@pytest.fixture(scope='module')
def P():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    import pycatkin_amd
    return pycatkin_amd


@pytest.fixture(scope='module')
def fx():
    return dict(np.load(FIXTURE))


_NETS = {}


def _net(key):
    if key not in _NETS:
        _NETS[key] = edge_net(key)
    return _NETS[key]


def _system(net, **kw):
    from pycatkin_amd.functions.synthetic import synthetic_system
    return synthetic_system(net, **kw)[0]


def _desc(D):
    """descriptor dict of a [n, 4] array"""
    return {'D%d' % k: np.ascontiguousarray(D[:, k]) for k in range(4)}


def close(a, b, rtol, floor):
    a, b = np.asarray(a), np.asarray(b)
    return np.all(np.abs(a - b) <= rtol * np.abs(b) + floor)


def _timed(label, t0):
    """wall time of a network's first solve (its hipRTC compiles included)"""
    print('%s: %.1f s' % (label, time.time() - t0))


# ------------------------------------------------------------------ a. rates
def rate_inputs(dyn, raised=()):
    """5 conditions: descriptors in +-0.5, T over 450..650 K, random states
    (the species in `raised` from [0.5, 1], so that a 31st power of them
    stays a normal number and above the floor of the comparison)."""
    rng = np.random.default_rng(31)
    n, NS = 5, len(dyn)
    D = rng.uniform(-0.5, 0.5, (n, 4))
    Tn = np.linspace(450.0, 650.0, n)
    y = rng.uniform(0.0, 2.0 / NS, (NS, n))
    for nm in raised:
        y[dyn.index(nm)] = rng.uniform(0.5, 1.0, n)
    return n, D, Tn, y


def rates_vs_oracle(net, raised=(), power=None, wide=None):
    """rate_constants, species_rates, jacobian and reaction_rates of `net`
    against the oracle's model; power = (reaction index, exponent) of an
    `e` A2 <-> A3 + (e - 1) s step whose net rate must stand above 1e-6 of
    the largest |f| at every condition, each direction alone at one at
    least; wide = index of p6's q0 + q1 + q2 <-> q3 + q4 + s step, whose two
    directions and whose derivative by the sixth participant (column s) must
    stand above 1e-6 of the largest rate / Jacobian entry at every
    condition, six orders above the floors.  Returns (System, DeviceNetwork)."""
    from _synth import spec_of
    sim = _system(net)
    plan = sim.plan()
    dnet = sim.device()
    dyn = list(plan.dyn)
    NS, R = len(dyn), len(plan.reactions)
    assert dnet.NDYN == NS and dnet.NRXN == R
    n, D, Tn, y = rate_inputs(dyn, raised)
    Tt, p, d, fxc, y0, inflow = sim._inputs(dnet, plan, n, Tn, None, _desc(D), None, None, None)
    kf, kr = dnet.rate_constants(n, Tt, p, d)
    f = dnet.species_rates(n, Tt, p, y, kf, kr, d, fxc, inflow).cpu().numpy()
    J = dnet.jacobian(n, Tt, p, y, kf, kr, d, fxc, inflow).cpu().numpy()
    rf, rr = (x.cpu().numpy() for x in dnet.reaction_rates(n, Tt, p, y, kf, kr, d, fxc))
    kf, kr = kf.cpu().numpy(), kr.cpu().numpy()
    fwd = rev = False
    for c in range(n):
        m = O.ClassicModel(spec_of(net, D[c], Tn[c]), T=Tn[c])
        full = m.y0.copy()
        pos = [m.idx[nm] for nm in dyn]
        full[pos] = y[:, c]
        rx = [m.rnames.index(r) for r in plan.reactions]
        fr, Jr = m.rhs(full)[pos], m.jac(full)[np.ix_(pos, pos)]
        rates = m.rates(full)[rx]
        if power is not None:
            # the power step from the oracle's own k and the mass-action
            # products: both directions count in f at every condition
            j, e = power
            a2, a3, s = (y[dyn.index(nm), c] for nm in ('A2', 'A3', 's'))
            pf, pr = m.kf[rx[j]] * a2 ** e, m.kr[rx[j]] * a3 * s ** (e - 1)
            np.testing.assert_allclose(rates[j], [pf, pr], rtol=1e-12)
            big = np.abs(fr).max()
            print('c %d: power step rf %.3g rr %.3g, max |f| %.3g' % (c, pf, pr, big))
            assert abs(pf - pr) > 1e-6 * big, (c, pf, pr, big)
            fwd, rev = fwd or pf > 1e-6 * big, rev or pr > 1e-6 * big
        if wide is not None:
            # the sixth participant's concentration enters the reverse rate
            # only, and the column it selects in the CSR entry (bits 26..31)
            # carries only kr c3 c4: both must count in what is compared
            _, reac, prod = net['reactions'][wide]
            c3, c4 = (y[dyn.index(nm), c] for nm in prod[:2])
            dcol = m.kr[rx[wide]] * c3 * c4
            col = dyn.index(prod[2])
            print('c %d: wide step rf %.3g rr %.3g of max %.3g, d/dc_63 %.3g of max |J| %.3g, max |J[:, 63]| %.3g' % (
                c, rates[wide, 0], rates[wide, 1], np.abs(rates).max(), dcol, np.abs(Jr).max(), np.abs(Jr[:, col]).max()))
            assert rates[wide].min() > 1e-6 * np.abs(rates).max(), (c, rates[wide], np.abs(rates).max())
            assert rates[wide].min() > 1e-6 * np.abs(fr).max(), (c, rates[wide], np.abs(fr).max())
            assert dcol > 1e-6 * np.abs(Jr).max(), (c, dcol, np.abs(Jr).max())
        np.testing.assert_allclose(kf[:, c], m.kf[rx], rtol=1e-10, atol=1e-12 * m.kf.max())
        np.testing.assert_allclose(kr[:, c], m.kr[rx], rtol=1e-10, atol=1e-12 * m.kr.max())
        np.testing.assert_allclose(f[:, c], fr, rtol=1e-10, atol=1e-12 * np.abs(fr).max())
        np.testing.assert_allclose(J[:, :, c], Jr, rtol=1e-10, atol=1e-12 * np.abs(Jr).max())
        np.testing.assert_allclose(rf[:, c], rates[:, 0], rtol=1e-10, atol=1e-12 * np.abs(rates).max())
        np.testing.assert_allclose(rr[:, c], rates[:, 1], rtol=1e-10, atol=1e-12 * np.abs(rates).max())
    assert power is None or (fwd and rev)
    return sim, dnet


@pytest.mark.parametrize('key', ALL_KEYS)
def test_edge_rates_jacobian_vs_oracle(P, key):
    """Rate constants, species rates, Jacobian and reaction rates at 5
    conditions against the oracle: the 16- / 32- / 64-lane rate kernels at
    their first and last row, species index 63, reaction index 255, the
    exponent-3 and exponent-31 steps (the ipow branch of spow), the sixth
    participant at plan index 63, and the one-lane kernels on e8a."""
    net = _net(key)
    ns, nr, _ = NETS[key]
    assert len(net['adsorbates']) + 1 == ns and len(net['reactions']) == nr
    if key in X_EXP:
        e = X_EXP[key]
        assert net['reactions'][X_INDEX] == ('surf',) + tuple(power_reaction(e))
        sim, dnet = rates_vs_oracle(net, raised=('A2', 's'), power=(X_INDEX, e))
    else:
        sim, dnet = rates_vs_oracle(net, wide=P6_INDEX if key == 'p6' else None)
    plan = sim.plan()
    if key == 'p6':
        # the wide reaction follows the chain (index 64): six distinct
        # participants, plan index 0 and 63 among them, 63 (the site s, the
        # last product) the sixth in the ascending species order of the
        # packed record
        _, reac, prod = net['reactions'][P6_INDEX]
        q = sorted(plan.dyn.index(nm) for nm in reac + prod)
        assert len(set(q)) == 6 and q[0] == 0 and q[5] == 63 and plan.dyn.index(prod[2]) == 63, q
    if key == 'e8a':
        # Nothing reports which rate kernel answered (the group diagnostics
        # are written by solves only).  What is pinned: a solve of this
        # network runs a one-lane plan and leaves group_lanes() at 0, and the
        # one-lane rate kernels are the only ones that take an exponent of 32
        # or seven participants (test_edge_one_lane_path_serves_wide_records,
        # against test_edge_group_path_refuses_wide_records on 12 species).
        r = sim.solve_batch(T=np.full(2, T), desc=_desc(np.zeros((2, 4))), t_end=1.0)
        assert np.all(r['status'] == 0)
        assert dnet.group_lanes() == 0 and dnet.plan_id() in (0, JIT_PLAN)


# ------------------------------------------------- b. solves vs the fixture
@pytest.mark.parametrize('key', FIXTURE_KEYS)
def test_edge_trajectory_vs_oracle(P, fx, key):
    """Dense output (solve_batch(t_out=...)) of the 8 conditions at rtol
    1e-10 / atol 1e-14, 9 samples 0 .. 1e2 s, against the oracle's LSODA at
    1e-12 / 1e-20: 1e-6 relative with a 1e-12 floor, on the kernel the size
    selects (e16: the quad kernel's launch with exactly 64 KiB of LDS)."""
    sim = _system(_net(key))
    plan = sim.plan()
    D, t_out = fx['desc'], fx['t_out']
    n = D.shape[0]
    t0 = time.time()
    r = sim.solve_batch(T=np.full(n, float(T)), desc=_desc(D), t0=0.0, t_end=float(t_out[-1]), rtol=1e-10,
                        atol=1e-14, t_out=t_out)
    _timed('%s trajectory solve' % key, t0)
    dnet = sim.device()
    assert dnet.group_lanes() == LANES[key]
    if key == 'e8a':
        assert dnet.plan_id() in (0, JIT_PLAN)
    assert np.all(r['status'] == 0), r['status']
    pos = [plan.dyn.index(str(nm)) for nm in fx[key + '_dyn']]
    traj = r['traj'][:, pos, :]                                  # [n_out, NS, n]
    ref = np.transpose(fx[key + '_traj'], (1, 2, 0))             # [n_out, NS, n]
    err = np.abs(traj - ref)
    print('%s: max |traj - ref| / (1e-6 |ref| + 1e-12) = %.3g' % (key, (err / (1e-6 * np.abs(ref) + 1e-12)).max()))
    bad = ~(err <= 1e-6 * np.abs(ref) + 1e-12)
    assert not bad.any(), (np.argwhere(bad)[:6].tolist(), err.max())
    np.testing.assert_array_equal(r['y'][pos], traj[-1])        # the last sample is the end state
    C = plan.conservation
    np.testing.assert_allclose(C @ r['y'], np.repeat((C @ plan.y0_default)[:, None], n, axis=1), rtol=0, atol=1e-10)


@pytest.mark.parametrize('key', FIXTURE_KEYS)
def test_edge_steady_vs_oracle(P, fx, key):
    """One steady solve of the 8 conditions (solve_batch(steady=True) to
    t_end = 1e8 s, the default STEADY_TRANSIENT tolerances) against the
    oracle's rule, with the bounds of test_synthetic_sizes_steady_vs_oracle:
    1e-6 on coverages (floor 1e-20) and the TOF where both sides report the
    root (the TOF term is the network's TOF_TERM, a step whose net rate does
    not cancel; make_edge_sizes_fixture.py), 1e-5 where neither does, the classification differing
    only where the oracle's criterion lies within a factor 2 of ROOT_DIST --
    at most 1 such flip, at least 6 of 8 roots on both sides.  (e8b: the
    'auto' screening pass of networks of <= 8 species would move the solve
    to the 16-lane kernel; it is off here, so the quad kernel answers.)"""
    sim = _system(_net(key), t_end=T_END)
    terms = (TOF_TERM[key],)
    plan = sim.plan(terms)
    D = fx['desc']
    n = D.shape[0]
    kw = dict(screen=None) if key == 'e8b' else {}
    t0 = time.time()
    r = sim.solve_batch(T=np.full(n, float(T)), desc=_desc(D), tof_terms=terms, steady=True, **kw)
    _timed('%s steady solve' % key, t0)
    dnet = sim.device(terms)
    assert dnet.group_lanes() == LANES[key]
    if key == 'e8a':
        assert dnet.plan_id() in (0, JIT_PLAN)
    st = r['status']
    assert set(np.unique(st).tolist()) <= {0, 4}, np.unique(st, return_counts=True)
    names = [str(x) for x in fx[key + '_dyn']]
    y = r['y'][[plan.dyn.index(nm) for nm in names]].T
    ok = fx[key + '_ok']
    assert ok.all()
    reg, dev = fx[key + '_regular'], st == 0
    flips = np.nonzero(dev != reg)[0]
    for f in flips:
        assert 0.5 * ROOT_DIST <= fx[key + '_crit'][f] <= 2.0 * ROOT_DIST, (key, int(f), st[f], fx[key + '_crit'][f])
    assert len(flips) <= 1, flips
    ref = fx[key + '_y']
    both = dev & reg
    neither = ~dev & ~reg
    assert both.sum() >= MIN_REGULAR, both.sum()
    err = np.abs(y - ref) / (np.abs(ref) + 1e-300)
    print('%s: statuses %s, max rel err at roots %.3g' % (key, st.tolist(), err[both].max()))
    ok_root = np.abs(y - ref) <= 1e-6 * np.abs(ref) + 1e-20
    assert np.all(ok_root[both]), (key, np.nonzero(both & ~np.all(ok_root, axis=1))[0][:5], err[both].max())
    ok_tr = np.abs(y - ref) <= 1e-5 * np.abs(ref) + 1e-20
    assert np.all(ok_tr[neither]), (key, np.nonzero(neither & ~np.all(ok_tr, axis=1))[0][:5])
    tof, tref = r['tof'], fx[key + '_tof']
    print('%s: TOF %s, |tof - ref| / |ref| = %s' % (key, np.array2string(tref, precision=2),
                                                   np.array2string(np.abs(tof - tref) / np.abs(tref), precision=2)))
    assert np.all(np.abs(tof[both] - tref[both]) <= 1e-6 * np.abs(tref[both])), \
        (key, np.max(np.abs(tof[both] - tref[both]) / np.abs(tref[both])))
    C = plan.conservation
    np.testing.assert_allclose(C @ r['y'], np.repeat((C @ plan.y0_default)[:, None], n, axis=1), rtol=0, atol=1e-10)


# ------------------------------------------------------- c. kernel variants
def _steady(key, fx):
    """a fresh System of the network and its steady solve of the 8 conditions"""
    sim = _system(_net(key), t_end=T_END)
    D = fx['desc']
    r = sim.solve_batch(T=np.full(D.shape[0], float(T)), desc=_desc(D), tof_terms=(TOF_TERM[key],), steady=True)
    return r, sim.device((TOF_TERM[key],))


@pytest.mark.parametrize('key', ['e17', 'e32', 'e33', 'e64'])
def test_edge_exact_size_kernel_matches_padded(P, fx, monkeypatch, key):
    """The exact-size hipRTC table kernel (PCK_GRP_CT=0: k_solve_grp<17, 32, 1>
    ...) and the padded compiled-in one (PCK_JIT=0: k_solve_grp<32, 32, 1> /
    <64, 64, 1>) at the first and the last row of the 32- and 64-lane
    groups: bitwise-equal states, TOFs, statuses and step counts, as
    test_group_exact_size_kernel_matches_compiled has it on DMTM and the
    comment in rec_rate claims for every build.

    At 33 and 64 species this failed while the padded 64-lane kernel kept a
    partial-pivoting LU next to the hipRTC kernels' threshold-pivoted
    grp_lu64 (mk_group.h: grp_lu): step counts 1017 against 1018 (e33) and
    1239 / 1170 against 1238 / 1167 (e64), states off by up to 7e-11.  Both
    builds now factorise with grp_lu64."""
    monkeypatch.setenv('PCK_GRP_CT', '0')
    a, da = _steady(key, fx)
    assert da.group_kernel() == 1 and da.group_lanes() == LANES[key]
    monkeypatch.setenv('PCK_JIT', '0')
    b, db = _steady(key, fx)
    assert db.group_kernel() == 0 and db.group_lanes() == LANES[key]
    monkeypatch.delenv('PCK_JIT')
    monkeypatch.delenv('PCK_GRP_CT')
    assert set(np.unique(a['status']).tolist()) <= {0, 4}
    print('%s: statuses %s / %s, steps %s / %s, max |dy| per condition %s, |dtof| %s' % (
        key, a['status'].tolist(), b['status'].tolist(), a['nsteps'].tolist(), b['nsteps'].tolist(),
        np.array2string(np.abs(a['y'] - b['y']).max(axis=0), precision=2),
        np.array2string(np.abs(a['tof'] - b['tof']), precision=2)))
    for k in ('status', 'nsteps', 'y', 'tof'):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.parametrize('key', ['e17', 'e32'])
def test_edge_compile_time_network_matches_tables(P, fx, monkeypatch, key):
    """The 32-lane kernel with the network compiled in (the default,
    group_kernel() == 2) against the record-table kernel (PCK_GRP_CT=0) at
    17 and 32 species: the same statuses, states and TOFs at 1e-9 with a
    1e-14 floor (the DMTM bound of
    test_group_compile_time_network_matches_tables)."""
    a, da = _steady(key, fx)
    assert da.group_kernel() == 2
    monkeypatch.setenv('PCK_GRP_CT', '0')
    b, db = _steady(key, fx)
    assert db.group_kernel() == 1
    monkeypatch.delenv('PCK_GRP_CT')
    print('%s: statuses %s / %s, max |dy| %.3g' % (key, a['status'].tolist(), b['status'].tolist(),
                                                  np.abs(a['y'] - b['y']).max()))
    np.testing.assert_array_equal(a['status'], b['status'])
    assert close(a['y'], b['y'], rtol=1e-9, floor=1e-14), np.abs(a['y'] - b['y']).max()
    assert close(a['tof'], b['tof'], rtol=1e-9, floor=1e-14), (a['tof'], b['tof'])


@pytest.mark.parametrize('key', ['e33', 'e64'])
def test_edge_balanced_walk_matches_row_loops(P, monkeypatch, key):
    """Rates and Jacobian of the 64-lane kernel with the balanced walk of the
    species CSR forced (PCK_GRP_BALANCE=2: walk slots with entry indices up
    to 14 bits, piece slots past species 63) against the per-row loops (=0):
    rtol 1e-12, floor 1e-14 x max, as test_balanced_walk_matches_row_loops."""
    def evaluate():
        sim = _system(_net(key))
        plan, dnet = sim.plan(), sim.device()
        n, D, Tn, y = rate_inputs(list(plan.dyn))
        Tt, p, d, fxc, y0, inflow = sim._inputs(dnet, plan, n, Tn, None, _desc(D), None, None, None)
        kf, kr = dnet.rate_constants(n, Tt, p, d)
        return (dnet.species_rates(n, Tt, p, y, kf, kr, d, fxc, inflow).cpu().numpy(),
                dnet.jacobian(n, Tt, p, y, kf, kr, d, fxc, inflow).cpu().numpy())

    monkeypatch.setenv('PCK_GRP_BALANCE', '2')
    fb, Jb = evaluate()
    monkeypatch.setenv('PCK_GRP_BALANCE', '0')
    fr, Jr = evaluate()
    monkeypatch.delenv('PCK_GRP_BALANCE')
    np.testing.assert_allclose(fb, fr, rtol=1e-12, atol=1e-14 * np.abs(fr).max())
    np.testing.assert_allclose(Jb, Jr, rtol=1e-12, atol=1e-14 * np.abs(Jr).max())


@pytest.mark.parametrize('key', ['x31', 'e16'])
def test_edge_quad_kernel_matches_16_lane_kernel(P, fx, monkeypatch, key):
    """The quad kernel (the default at <= 16 species) against the 16-lane
    kernel (PCK_GRP_QUAD=0) on the exponent-31 network and on 16 species /
    256 reactions: the same statuses, states and TOFs at 1e-9 with a 1e-14
    floor (the bound of test_quad_group_kernel_matches_lane_group).  The
    steady quad kernels are the ones test_edge_steady_vs_oracle compiled
    earlier in the process; the 16-lane kernel with the network compiled in
    is compiled here, which on e16 takes minutes (DESIGN.md "Size and
    packing limits")."""
    t0 = time.time()
    a, da = _steady(key, fx)
    assert da.group_kernel() == 3 and da.group_lanes() == 4
    monkeypatch.setenv('PCK_GRP_QUAD', '0')
    b, db = _steady(key, fx)
    assert db.group_kernel() == 2 and db.group_lanes() == 16
    monkeypatch.delenv('PCK_GRP_QUAD')
    _timed('%s quad and 16-lane steady solves' % key, t0)
    print('%s: statuses %s / %s, max |dy| %.3g' % (key, a['status'].tolist(), b['status'].tolist(),
                                                  np.abs(a['y'] - b['y']).max()))
    np.testing.assert_array_equal(a['status'], b['status'])
    assert close(a['y'], b['y'], rtol=1e-9, floor=1e-14), np.abs(a['y'] - b['y']).max()
    assert close(a['tof'], b['tof'], rtol=1e-9, floor=1e-14), (a['tof'], b['tof'])


# ------------------------------------------------------------------ d. limits
def test_edge_sixteen_tof_terms(P, fx):
    """PCK_MAX_TOF = 16 terms on the 17-species network, a transient to 1e2
    s: the device's TOF is the sum of the oracle's net rates of those 16
    reactions at the device's own end state (rtol 1e-10, floor 1e-12 x
    sum(|rf| + |rr|))."""
    from _synth import spec_of
    net = _net('e17')
    terms = tuple('R%d' % j for j in list(range(15)) + [50])
    assert len(terms) == 16
    sim = _system(net)
    plan = sim.plan(terms)
    D = fx['desc']
    n = D.shape[0]
    r = sim.solve_batch(T=np.full(n, float(T)), desc=_desc(D), tof_terms=terms, t0=0.0, t_end=1.0e2)
    assert sim.device(terms).NTOF == 16
    assert np.all(r['status'] == 0), r['status']
    for c in range(n):
        m = O.ClassicModel(spec_of(net, D[c], float(T)), T=float(T))
        full = m.y0.copy()
        full[[m.idx[nm] for nm in plan.dyn]] = r['y'][:, c]
        rates = m.rates(full)[[m.rnames.index(t) for t in terms]]
        ref = float(np.sum(rates[:, 0] - rates[:, 1]))
        assert abs(r['tof'][c] - ref) <= 1e-10 * abs(ref) + 1e-12 * np.abs(rates).sum(), (c, r['tof'][c], ref)


SEVEN = (['A0', 'A1', 'A2', 'A3'], ['A4', 'A5', 's', 's'])      # A0..A5 and s: seven dynamic participants


def limit_net(n_species, n_reactions, which):
    """edge_network plus 32 A2 <-> A3 + 31 s ('exp'), the seven-participant
    step ('part') or both; the extras follow the chain (index n_species)."""
    from _synth import edge_network
    extra = {'exp': (power_reaction(32),), 'part': (SEVEN,), 'both': (power_reaction(32), SEVEN)}[which]
    net = edge_network(n_species, n_reactions, 5, extra=extra)
    if which != 'part':
        tune_power_reaction(net, 32, n_species)
    return net


@pytest.mark.parametrize('which,cause', [('exp', 'exponent above 31'), ('part', 'more than 6 dynamic participants')])
def test_edge_group_path_refuses_wide_records(P, which, cause):
    """A 12-species network (group path) with an exponent of 32, or with
    seven dynamic participants in one reaction, does not fit the packed
    records (PCK_GRP_MAX_EXP, PCK_GRP_MAX_PART): species_rates, jacobian and
    solve_batch raise the C-ABI's PCK_E_SIZE naming that cause, and a normal
    solve in the same process still works afterwards."""
    sim = _system(limit_net(12, 30, which))
    plan, dnet = sim.plan(), sim.device()
    n, D, Tn, y = rate_inputs(list(plan.dyn), raised=('A2', 's'))
    Tt, p, d, fxc, y0, inflow = sim._inputs(dnet, plan, n, Tn, None, _desc(D), None, None, None)
    kf, kr = dnet.rate_constants(n, Tt, p, d)
    good = _system(_net('x3'))

    def works():
        r = good.solve_batch(T=np.full(n, float(T)), desc=_desc(D), t_end=1.0)
        assert np.all(r['status'] == 0), r['status']

    with pytest.raises(RuntimeError, match=cause):
        dnet.species_rates(n, Tt, p, y, kf, kr, d, fxc, inflow)
    works()
    with pytest.raises(RuntimeError, match=cause):
        dnet.jacobian(n, Tt, p, y, kf, kr, d, fxc, inflow)
    works()
    with pytest.raises(RuntimeError, match=cause):
        sim.solve_batch(T=Tn, desc=_desc(D), t_end=1.0)
    works()


def test_edge_one_lane_path_serves_wide_records(P):
    """The same two reactions in an 8-species / 28-reaction network run on
    the one-lane kernels (exponents to PCK_MAX_EXP, any number of
    participants): rates and Jacobian match the oracle at the bound of (a),
    and a solve reports a one-lane plan."""
    net = limit_net(8, 28, 'both')
    assert net['reactions'][8] == ('surf',) + tuple(power_reaction(32)) and net['reactions'][9][1:] == tuple(SEVEN)
    sim, dnet = rates_vs_oracle(net, raised=('A2', 's'), power=(8, 32))
    r = sim.solve_batch(T=np.full(2, float(T)), desc=_desc(np.zeros((2, 4))), t_end=1.0)
    assert np.all(r['status'] == 0), r['status']
    assert dnet.group_lanes() == 0 and dnet.plan_id() in (0, JIT_PLAN)
