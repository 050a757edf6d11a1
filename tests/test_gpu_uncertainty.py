"""The uncertainty ensemble on the device (pycatkin_amd/classes/uncertainty.py,
csrc/tu_ensemble.hip): pck_ensemble_noise against the numpy restatement of
Philox4x32-10 (tests/_philox.py), pck_ensemble_stats against exact rational
arithmetic on the same doubles, and Uncertainty's ensemble / drop-in methods
against tests/golden/uncertainty_fixture.npz (make_uncertainty_fixture.py).

Bounds.
  noise row 0: 1e-13 * sigma absolute -- log, sqrt and cos are each within
    about 2 ulp on both sides and |z| < 9 (ulp(8) = 1.8e-15); measured worst
    1.11e-15 * sigma.  Rows 1+k: bitwise the device's row 0 times the restated u.
  statistics: count, min, max exact; mean and std within
    max(8 x the error of np.mean / np.std on the same values, 32 ulp of the
    exact result) -- Chan merges cost O(log2 n) roundings; measured worst
    std 1.73 ulp, mean 75.9 ulp (numpy's own worst at that size: 31.1 ulp; the
    mixed-sign data, whose mean is small against its values).
  ensembles: the bounds of test_dmtm_pressure_sweep_vs_oracle (1e-6 relative,
    1e-15 floor on coverages) and test_butadiene_steady_sweep_vs_oracle."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _philox  # noqa: E402
from test_uncertainty import butadiene_system, dmtm_system  # noqa: E402

FIXTURE = os.path.join(HERE, 'golden', 'uncertainty_fixture.npz')
MU, SIGMA, SEED = 0.3, 0.05, 0x9E3779B97F4A7C15


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


# -- pck_ensemble_noise ------------------------------------------------------------
_restated = {}


def restated(n_runs, n_ts, run_first):
    """(z [n_runs], u [n_ts, n_runs]) of runs run_first .. from tests/_philox.py."""
    key = (n_runs, n_ts, run_first)
    if key not in _restated:
        runs = np.arange(n_runs, dtype=np.uint64) + np.uint64(run_first)
        _restated[key] = (_philox.normal(SEED, runs), _philox.uniforms(SEED, runs, n_ts))
    return _restated[key]


@pytest.mark.parametrize('run_first', [0, 2 ** 32 - 3])
@pytest.mark.parametrize('n_runs', [1, 63, 64, 65, 1000])
def test_noise_kernel_vs_restatement(P, n_runs, run_first):
    import torch
    from pycatkin_amd.engine import ensemble_noise
    worst = 0.0
    for n_rep in (1, 3):
        for n_ts in (0, 1, 2, 7):
            for lead in (0, 1):
                B = n_runs + lead
                pad = 5
                out = torch.full((1 + n_ts + 1, n_rep * B + pad), -7.0, dtype=torch.float64, device='cuda')
                ensemble_noise(SEED, n_runs, n_rep, n_ts, lead, MU, SIGMA, run_first, out=out)
                m = out.cpu().numpy()
                assert np.all(m[:, n_rep * B:] == -7.0) and np.all(m[1 + n_ts:] == -7.0)      # padding untouched
                blocks = m[:1 + n_ts, :n_rep * B].reshape(1 + n_ts, n_rep, B)
                for c in range(1, n_rep):
                    assert np.array_equal(blocks[:, c], blocks[:, 0])                          # replicas
                if lead:
                    assert np.all(blocks[:, :, 0] == 0.0) and not np.any(np.signbit(blocks[:, :, 0]))
                got = blocks[:, 0, lead:]
                z, u = restated(n_runs, n_ts, run_first)
                err = np.abs(got[0] - (MU + SIGMA * z)).max()
                worst = max(worst, err)
                assert err <= 1e-13 * SIGMA, (n_runs, n_rep, n_ts, lead, err)
                assert np.array_equal(got[1:], got[0][None, :] * u)                            # bitwise
    print('noise row 0: worst |device - restated| = %.3g * sigma' % (worst / SIGMA))


def test_noise_of_a_run_depends_on_seed_and_run_alone(P):
    from pycatkin_amd.engine import ensemble_noise
    full = ensemble_noise(SEED, 1000, 1, 7, False, MU, SIGMA, 0).cpu().numpy()
    part = ensemble_noise(SEED, 100, 3, 7, True, MU, SIGMA, 500).cpu().numpy()
    assert np.array_equal(part[:, 1:101], full[:, 500:600])
    assert np.array_equal(part[:, 203:303], full[:, 500:600])
    other = ensemble_noise(SEED + 1, 100, 1, 7, False, MU, SIGMA, 500).cpu().numpy()
    assert not np.any(other == full[:, 500:600])


def test_noise_moments(P):
    from pycatkin_amd.engine import ensemble_noise
    N = 2 ** 20
    m = ensemble_noise(12345, N, 1, 1, False, MU, SIGMA, 0).cpu().numpy()
    z = (m[0] - MU) / SIGMA
    u = m[1] / m[0]
    assert abs(z.mean()) <= 5.0 / math.sqrt(N), z.mean()
    assert abs(z.var() - 1.0) <= 5.0 * math.sqrt(2.0 / N), z.var()
    assert abs(u.mean() - 0.5) <= 5.0 * math.sqrt(1.0 / 12.0 / N), u.mean()
    assert u.min() >= 0.0 and u.max() < 1.0 + 1e-15


def test_noise_arguments(P):
    import torch
    from pycatkin_amd import _lib as L
    lib = L.load()
    buf = torch.zeros((3, 10), dtype=torch.float64, device='cuda')
    call = lambda *a: lib.pck_ensemble_noise(*a)
    assert call(1, 0, 4, 2, 2, 1, 0.0, 1.0, buf.data_ptr(), 10, None) == 0
    assert call(1, 0, 4, 2, 2, 1, 0.0, 1.0, None, 10, None) == L.E_ARG
    assert call(1, 0, -1, 2, 2, 1, 0.0, 1.0, buf.data_ptr(), 10, None) == L.E_ARG
    assert call(1, 0, 4, 2, -2, 1, 0.0, 1.0, buf.data_ptr(), 10, None) == L.E_ARG
    assert call(1, 0, 4, 2, 2, 1, 0.0, 1.0, buf.data_ptr(), 9, None) == L.E_ARG
    assert b'ld_desc' in lib.pck_last_error()
    o = L.EnsStats()
    assert lib.pck_ensemble_stats(None, 10, 1, None, 1, 1, 10, 0, o, None) == L.E_ARG
    assert lib.pck_ensemble_stats(buf.data_ptr(), 9, 1, None, 1, 1, 10, 0, o, None) == L.E_ARG
    assert lib.pck_ensemble_stats(buf.data_ptr(), 10, 1, None, 1, 1, 10, -1, o, None) == L.E_ARG


# -- pck_ensemble_stats ------------------------------------------------------------
def exact_stats(xs):
    """(mean, std) of the doubles xs as Fractions: sums of integers scaled by a
    power of two; the square root to 2^-300 of the result."""
    n = len(xs)
    parts = [math.frexp(x) for x in xs]
    emin = min(e for _, e in parts) - 53
    ints = [int(m * 2.0 ** 53) << (e - 53 - emin) for m, e in parts]
    s1, s2 = sum(ints), sum(i * i for i in ints)
    scale = Fraction(2) ** emin
    var_num = n * s2 - s1 * s1
    k = 300 + max(0, -var_num.bit_length() // 2)
    return Fraction(s1, n) * scale, Fraction(math.isqrt(var_num << (2 * k)), n << k) * scale


def ulps(err, exact):
    return float(err / Fraction(math.ulp(float(exact)))) if exact != 0 else (0.0 if err == 0 else math.inf)


def stats_data(kind, rows, n_rep, block, rng):
    """values [rows, n_rep * block], status [n_rep * block] or None."""
    n = n_rep * block
    status = None
    if kind == 'offset':                       # (i)
        v = 1.0e8 + rng.standard_normal((rows, n))
    elif kind == 'loguniform':                 # (ii)
        v = 10.0 ** rng.uniform(-30.0, 0.0, (rows, n))
    elif kind == 'equal':                      # (iii)
        v = np.repeat(rng.uniform(-3.0, 3.0, (rows, 1)) * 1.0e5, n, axis=1)
    else:                                      # (iv) non-finite entries and refused statuses, (v) an empty block
        v = rng.standard_normal((rows, n)) * 10.0 ** rng.uniform(-3.0, 3.0, (rows, n))
        bad = rng.uniform(size=(rows, n)) < 0.15
        v[bad] = rng.choice([np.nan, np.inf, -np.inf], size=int(bad.sum()))
        status = rng.choice([0, 4, 1, 2, 3, 5, 40, -1], size=n, p=[0.5, 0.2, 0.05, 0.05, 0.05, 0.05, 0.05, 0.05])
        if kind == 'empty':
            status[:block] = 3                                     # nothing accepted by status
            if n_rep > 1:
                v[:, block:2 * block] = np.nan                     # nothing finite
        status = status.astype(np.int32)
    return v, status


@pytest.mark.parametrize('block', [1, 2, 63, 64, 65, 257, 4096])
def test_stats_kernel_vs_exact_arithmetic(P, block):
    import torch
    from pycatkin_amd.engine import ensemble_stats
    rng = np.random.default_rng(block)
    worst = dict(mean=0.0, std=0.0, np_mean=0.0, np_std=0.0)
    for kind in ('offset', 'loguniform', 'equal', 'refused', 'empty'):
        V, S = stats_data(kind, 5, 3, block, rng)
        dV = torch.as_tensor(V, device='cuda')
        dS = None if S is None else torch.as_tensor(S, device='cuda')
        exact = {}
        for skip in (0, 1):
            for n_rep in (1, 3):
                for n_rows in (1, 5):
                    n = n_rep * block
                    view, st = dV[:n_rows, :n], (None if dS is None else dS[:n])
                    r = {k: t.cpu().numpy() for k, t in ensemble_stats(view, st, (0, 4), block, skip).items()}
                    again = {k: t.cpu().numpy() for k, t in ensemble_stats(view, st, (0, 4), block, skip).items()}
                    for k in r:
                        assert r[k].shape == (n_rows, n_rep)
                        assert np.array_equal(r[k], again[k], equal_nan=True), k          # launch to launch
                    for q in range(n_rows):
                        for c in range(n_rep):
                            x = V[q, c * block + skip:(c + 1) * block]
                            keep = np.isfinite(x)
                            if S is not None:
                                keep &= np.isin(S[c * block + skip:(c + 1) * block], (0, 4))
                            x = x[keep]
                            where = (kind, block, skip, n_rep, n_rows, q, c)
                            assert r['count'][q, c] == x.size, where
                            if x.size == 0:
                                assert np.isnan(r['mean'][q, c]) and np.isnan(r['std'][q, c]), where
                                assert r['min'][q, c] == np.inf and r['max'][q, c] == -np.inf, where
                                continue
                            assert r['min'][q, c] == x.min() and r['max'][q, c] == x.max(), where
                            if (q, c, skip) not in exact:
                                exact[(q, c, skip)] = exact_stats([float(t) for t in x])
                            for name, ex, ref in (('mean', exact[(q, c, skip)][0], np.mean(x)),
                                                  ('std', exact[(q, c, skip)][1], np.std(x))):
                                err = abs(Fraction(float(r[name][q, c])) - ex)
                                np_err = abs(Fraction(float(ref)) - ex)
                                assert err <= max(8 * np_err, 32 * Fraction(math.ulp(float(ex)))), \
                                    (where, name, float(r[name][q, c]), float(ex), float(err), float(np_err))
                                worst[name] = max(worst[name], ulps(err, ex))
                                worst['np_' + name] = max(worst['np_' + name], ulps(np_err, ex))
                            if kind == 'equal':
                                assert r['std'][q, c] == 0.0 and r['mean'][q, c] == x[0], where
        if kind == 'empty':
            assert np.all(r['count'][:, 0] == 0)
    print('stats block %d: worst error in ulp of the exact result: mean %.2f (numpy %.2f), std %.2f (numpy %.2f)'
          % (block, worst['mean'], worst['np_mean'], worst['std'], worst['np_std']))


def test_statistics_wrapper_host_and_device(P):
    import torch
    rng = np.random.default_rng(0)
    v = rng.standard_normal((2, 12))
    st = np.array([0, 4, 1, 0] * 3, np.int32)
    r = P.Uncertainty.statistics(v, st, block=4, skip=1)
    assert isinstance(r['mean'], np.ndarray) and r['mean'].shape == (2, 3) and np.all(r['count'] == 2)
    np.testing.assert_allclose(r['mean'], v.reshape(2, 3, 4)[:, :, [1, 3]].mean(axis=2), rtol=1e-14)
    d = P.Uncertainty.statistics(torch.as_tensor(v[0], device='cuda'))
    assert d['std'].is_cuda and d['std'].shape == (1,)
    np.testing.assert_allclose(d['std'].cpu().numpy(), [v[0].std()], rtol=1e-14)
    with pytest.raises(ValueError):
        P.Uncertainty.statistics(v, block=5)


def check_stats(stats, per_run, status, skip, where):
    """stats (solve_ensemble's) against the exact statistics of the per-run
    arrays it was reduced from, within the stats kernel's bound."""
    arrays = [('tof', per_run['tof'][None], {k: np.asarray(v)[None] for k, v in stats['tof'].items()}),
              ('y', per_run['y'], stats['y'])]
    n_rep = status.shape[0]
    for tag, v, s in arrays:
        for q in range(v.shape[0]):
            for c in range(n_rep):
                x = v[q, c, skip:]
                x = x[np.isfinite(x) & np.isin(status[c, skip:], (0, 4))]
                assert s['count'][q, c] == x.size and x.size > 0, (where, tag, q, c)
                assert s['min'][q, c] == x.min() and s['max'][q, c] == x.max()
                ex = exact_stats([float(t) for t in x])
                for name, e, ref in (('mean', ex[0], np.mean(x)), ('std', ex[1], np.std(x))):
                    err, np_err = abs(Fraction(float(s[name][q, c])) - e), abs(Fraction(float(ref)) - e)
                    assert err <= max(8 * np_err, 32 * Fraction(math.ulp(float(e)))), (where, tag, name, q, c)
    bad = (~np.isin(status[:, skip:], (0, 4))).sum(axis=1)
    assert np.array_equal(stats['n_failed'], bad), (where, stats['n_failed'], bad)


# -- ensembles against the oracle ------------------------------------------------------
def test_dmtm_ensemble_vs_oracle(P, inputs, fx):
    """Fixture (2): 3 temperatures x (1 + 32) members in one launch of 99 conditions."""
    unc = P.Uncertainty(sys=dmtm_system(inputs), mu=0.0, sigma=0.05, nruns=32)
    noises = {str(k): fx['dmtm_noise'][j] for j, k in enumerate(fx['dmtm_noise_keys'])}
    r = unc.solve_ensemble(T=fx['dmtm_T'], noises=noises, tof_terms=('r5', 'r9'), steady=True)
    assert r['y'].shape[1:] == (3, 33) and r['tof'].shape == (3, 33) and r['status'].shape == (3, 33)
    assert np.array_equal(r['status'] == 0, fx['dmtm_regular']), (r['status'], fx['dmtm_crit'])
    assert np.all(np.isin(r['status'], (0, 4)))
    plan = unc._ensemble().plan(('r5', 'r9'))
    order = [list(fx['dmtm_dyn']).index(s) for s in plan.dyn]
    ref = fx['dmtm_y'][order]
    ey = np.abs(r['y'] - ref) / (np.abs(ref) + 1e-300)
    et = np.abs(r['tof'] - fx['dmtm_tof']) / np.abs(fx['dmtm_tof'])
    print('DMTM ensemble: worst relative error y %.3g (above the floor), tof %.3g'
          % (ey[np.abs(ref) > 1e-9].max(), et.max()))
    assert np.all(np.abs(r['y'] - ref) <= 1e-6 * np.abs(ref) + 1e-15), ey.max()
    assert np.all(np.abs(r['tof'] - fx['dmtm_tof']) <= 1e-6 * np.abs(fx['dmtm_tof'])), et.max()
    # the members differ, the base member is the unperturbed one, the noises are the ones given
    assert np.ptp(r['tof'], axis=1).min() > 0.0
    for k, v in noises.items():
        assert np.array_equal(r['noises'][k], v)
    assert r['stats']['species'] == list(plan.dyn)
    check_stats(r['stats'], r, r['status'], 1, 'dmtm')


def test_butadiene_ensemble_vs_oracle(P, inputs, fx, monkeypatch):
    """Fixture (3): p123_p124_p156 (19 species, the 32-lane group kernel), 2
    temperatures x (1 + 8) members, the noise on the base system's states;
    one device network serves the ensemble."""
    from make_butadiene_fixture import BD_TERMS
    from pycatkin_amd.engine import DeviceNetwork
    made = []
    orig = DeviceNetwork.__init__

    def counting(self, *a, **kw):
        made.append(1)
        return orig(self, *a, **kw)
    monkeypatch.setattr(DeviceNetwork, '__init__', counting)
    sim, _ = butadiene_system(inputs)
    unc = P.Uncertainty(sys=sim, mu=0.0, sigma=0.05, nruns=8)
    terms = tuple(t for t in BD_TERMS if t in sim.reactions)
    noises = {str(k): fx['bd_noise'][j] for j, k in enumerate(fx['bd_noise_keys'])}
    r = unc.solve_ensemble(T=fx['bd_T'], noises=noises, tof_terms=terms, steady=True)
    ens = unc._ensemble()
    assert ens.device(terms).group_lanes() == 32
    assert len(made) == 1
    st = r['status']
    assert np.all(np.isin(st, (0, 4))), st
    assert np.array_equal(st == 0, fx['bd_regular']), (st, fx['bd_crit'])
    plan = ens.plan(terms)
    order = [list(fx['bd_dyn']).index(s) for s in plan.dyn]
    ref = fx['bd_y'][order]
    bad = ~(np.abs(r['y'] - ref) <= 1e-6 * np.abs(ref) + 1e-15)
    assert not bad.any(), (np.argwhere(bad)[:8].tolist(), (np.abs(r['y'] - ref) / (np.abs(ref) + 1e-9)).max())
    assert np.all(np.abs(r['tof'] - fx['bd_tof']) <= 1e-6 * np.abs(fx['bd_tof']) + 1e-300), (r['tof'], fx['bd_tof'])
    check_stats(r['stats'], r, st, 1, 'butadiene')


# -- drop-in --------------------------------------------------------------------------
def test_dropin_get_mean_property_value(P, inputs):
    """uncertainty.py:98-125 on a one-lane network (COOxReactor Pd111, nruns = 4):
    run 0 is the plain system's solve_odes, runs 1.. the reference-style loop
    (set_correlated_state_noises -> a float-modified copy -> solve_odes), the
    mean and std numpy's over runs 1...  1e-9: the ensemble network adds a
    descriptor (0 for run 0) to each perturbed energy where the loop's copies
    add a float, so the energies agree to rounding (1e-16 of ~1e2 eV, / kT:
    ~1e-12 relative in a rate constant)."""
    sim = P.read_from_input_file(os.path.join(inputs, 'COOxReactor', 'input_Pd111.json'))
    plain = P.read_from_input_file(os.path.join(inputs, 'COOxReactor', 'input_Pd111.json'))
    plain.solve_odes()
    assert plain.device().NDYN <= 8
    # the property: the largest coverage below 1 % (the noise moves it; the gas rows barely change)
    i = int(np.argmax(np.where(plain.solution[-1] < 1.0e-2, plain.solution[-1], 0.0)))
    handle = lambda s: s.solution[-1][i]
    unc = P.Uncertainty(sys=sim, mu=0.0, sigma=0.05, nruns=4)
    np.random.seed(11)
    values, mean, std = unc.get_mean_property_value(handle)
    assert values.shape == (5,) and sorted(unc.noisy_sys) == [0, 1, 2, 3, 4]
    assert values[0] == pytest.approx(handle(plain), rel=1e-9)
    assert set(unc.state_noises[0].values()) == {0.0} and list(unc.state_noises[0]) == list(unc.state_noises[1])
    np.random.seed(11)
    again = [unc.get_correlated_state_noises() for _ in range(4)]
    assert [unc.state_noises[k] for k in range(1, 5)] == again
    loop = []
    for run in range(1, 5):
        s = unc.set_correlated_state_noises(unc.state_noises[run])
        s.solve_odes()
        loop.append(handle(s))
        assert np.array_equal(unc.noisy_sys[run].times, s.times)
        # species far below the transient's atol are resolved against it, not relatively
        np.testing.assert_allclose(unc.noisy_sys[run].solution[-1], s.solution[-1], rtol=1e-9,
                                   atol=1e-9 * sim.params['atol'])
    print('drop-in: values', values, 'loop', loop)
    np.testing.assert_allclose(values[1:], loop, rtol=1e-9)
    assert len(set(values)) == 5
    assert mean == np.mean(values[1:]) and std == np.std(values[1:])
    # a member answers single-condition calls from the shared ensemble network
    m = unc.noisy_sys[2]
    assert m._plans is unc.noisy_sys[0]._plans
    ref = unc.set_correlated_state_noises(unc.state_noises[2])
    np.testing.assert_allclose(m.reaction_terms(m.solution[-1]), ref.reaction_terms(m.solution[-1]), rtol=1e-9)


# -- device rng, end to end ---------------------------------------------------------------
def test_device_rng_end_to_end(P, inputs):
    unc = P.Uncertainty(sys=dmtm_system(inputs), mu=0.0, sigma=0.05, nruns=256)
    T = [450.0, 600.0, 750.0]
    kw = dict(T=T, nruns=256, rng='device', seed=7, tof_terms=('r5', 'r9'), steady=True)
    a = unc.solve_ensemble(**kw)
    b = unc.solve_ensemble(**kw)
    assert a['y'].shape[1:] == (3, 257)
    for k in ('y', 'tof', 'status', 'nsteps'):
        assert np.array_equal(a[k], b[k]), k
    for k in ('mean', 'std', 'count', 'min', 'max'):
        assert np.array_equal(a['stats']['tof'][k], b['stats']['tof'][k]), k
        assert np.array_equal(a['stats']['y'][k], b['stats']['y'][k]), k
    noises = unc.sample_noises(256, rng='device', seed=7)
    assert list(a['noises']) == list(noises)
    for k, v in noises.items():
        assert v.shape == (256,) and np.array_equal(a['noises'][k], v), k
    ads, tss = unc.noise_states()
    assert abs(noises[ads[0]].std() - 0.05) < 0.05 * 5.0 / math.sqrt(2 * 256)
    # the base column is the unperturbed system
    base = unc.sys.solve_batch(T=T, tof_terms=('r5', 'r9'), steady=True)
    assert np.array_equal(a['status'][:, 0], base['status'])
    np.testing.assert_allclose(a['y'][:, :, 0], base['y'], rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(a['tof'][:, 0], base['tof'], rtol=1e-9)
    assert np.all(np.isin(a['status'], (0, 4))) and np.all(a['stats']['n_failed'] == 0)
    check_stats(a['stats'], a, a['status'], 1, 'device rng')
    # on the device from end to end
    d = unc.solve_ensemble(to_numpy=False, **kw)
    assert d['tof'].is_cuda and d['stats']['y']['mean'].is_cuda and d['noises'][ads[0]].is_cuda
    assert np.array_equal(d['stats']['tof']['mean'].cpu().numpy(), a['stats']['tof']['mean'])


# -- energy span -------------------------------------------------------------------------
def test_energy_span_ensemble(P, inputs):
    """energy_span_fixture.npz part (c): 70 members of a correlated ensemble on
    the DMTM landscape at 600 K, at the bounds of test_gpu_energy_span.py."""
    from test_gpu_energy_span import check
    fx = dict(np.load(os.path.join(HERE, 'golden', 'energy_span_fixture.npz')))
    sim = dmtm_system(inputs)
    unc = P.Uncertainty(sys=sim, mu=0.0, sigma=0.1, nruns=70)
    noises = {str(s): fx['ens_noise'] for s in fx['ens_ads']}
    noises.update({str(s): fx['ens_ts_noise'][k] for k, s in enumerate(fx['ens_ts'])})
    r = unc.energy_span_ensemble('full_pes', T=600.0, p=sim.params['pressure'], noises=noises)
    assert r['tof'].shape == (70,)
    check(r, fx, 'ens')
    assert np.ptp(r['tof']) > 0.0
    # the caller's landscape is untouched
    assert sim.energy_landscapes['full_pes'].evaluate_batch(T=600.0, p=sim.params['pressure'])['tof'].shape == (1,)
