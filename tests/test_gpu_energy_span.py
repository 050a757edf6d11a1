"""pck_energy_span on the device against the reference's own Energy class
(tests/golden/energy_span_fixture.npz, written by make_energy_span_fixture.py).

Bounds.  Between three summation orders of the same float64 state energies
the reference's TOF moves by 3.3e-12 relative at 400 K (1.3e-13 at 800 K;
fixture 'spread_tof'): the absolute energies reach 722 eV and their differences
are divided by kT.  tof is held to 1e-10 relative (30x that spread); Espan,
Eapp and the energies to 1e-10 relative + 1e-12 absolute; the contributions to
1e-10 absolute.  The TOF-determining indices must be equal wherever the
reference's two largest contributions lie at least 1e-6 apart, which must
leave out at most 2 % of the conditions."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'energy_span_fixture.npz')
R, EV2JMOL, KB, H = 8.31446262, 96.485 * 1.0e3, 1.380662e-23, 6.626176e-34


@pytest.fixture(scope='module')
def fx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return dict(np.load(FIXTURE))


@pytest.fixture(scope='module')
def dmtm(inputs, fx):
    import pycatkin_amd as P
    return P.read_from_input_file(os.path.join(inputs, 'DMTM', 'input.json'))


def close(a, b, rtol, atol=0.0):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = np.abs(a - b) - (rtol * np.abs(b) + atol)
    assert np.all(err <= 0.0), (float(np.max(np.abs(a - b))), float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))))


def check(r, fx, prefix, cols=slice(None), max_skipped=0.02):
    """The bounds of the module docstring on an evaluate_batch result against fixture block `prefix`."""
    g = lambda k: fx['%s_%s' % (prefix, k)][..., cols]
    close(r['tof'], g('tof'), 1e-10)
    for k in ('Espan', 'Eapp', 'dGrxn', 'energies'):
        close(r[k], g(k), 1e-10, 1e-12)
    close(r['xTDTS'], g('xTDTS'), 0.0, 1e-10)
    close(r['xTDI'], g('xTDI'), 0.0, 1e-10)
    sure = (g('gap_ts') >= 1e-6) & (g('gap_int') >= 1e-6)
    assert np.mean(~sure) <= max_skipped
    assert np.array_equal(r['iTDTS'][sure], g('iTDTS')[sure])
    assert np.array_equal(r['iTDI'][sure], g('iTDI')[sure])
    assert list(r['lTi']) == list(fx[prefix + '_lTi']) and list(r['lIj']) == list(fx[prefix + '_lIj'])
    return sure


# -- (a) DMTM full_pes ---------------------------------------------------------
@pytest.mark.parametrize('etype', ['free', 'electronic'])
def test_dmtm_landscape_51_conditions(dmtm, fx, etype):
    pes = dmtm.energy_landscapes['full_pes']
    r = pes.evaluate_batch(T=fx['dmtm_T'], p=fx['dmtm_p'], etype=etype)
    assert r['tof'].shape == (51,) and r['xTDTS'].shape == (7, 51) and r['xTDI'].shape == (11, 51)
    check(r, fx, 'dmtm_' + etype)


# -- (b) random landscapes -----------------------------------------------------
def stub_landscape(is_ts, energies=None, tag='rnd'):
    """A landscape of one-state entries whose free energies are per-condition
    descriptors e00, e01, ... (or the given constants)."""
    import pycatkin_amd as P
    states = [P.State(state_type='TS' if t else 'adsorbate', name='%s%d' % ('T' if t else 'I', k), Gelec=0.0,
                      Gfree=P.Descriptor('e%02d' % k) if energies is None else float(energies[k]))
              for k, t in enumerate(is_ts)]
    return P.Energy(name=tag, minima=[[s] for s in states])


def desc_of(E, cols=slice(None)):
    return {'e%02d' % k: E[k, cols] for k in range(E.shape[0])}


@pytest.fixture(scope='module')
def rnd(fx):
    out = {}
    for tag in ('rnd4', 'rnd5', 'rnd9', 'rnd20', 'rnd64', 'tie9'):
        pes = stub_landscape(list(fx[tag + '_isTS']), tag=tag)
        out[tag] = (pes, pes.evaluate_batch(T=fx[tag + '_T'], p=1.0e5, desc=desc_of(fx[tag + '_E'])))
    return out


@pytest.mark.parametrize('tag', ['rnd4', 'rnd5', 'rnd9', 'rnd20', 'rnd64'])
def test_random_landscapes_70_conditions(rnd, fx, tag):
    """One launch of 70 conditions (a full wavefront and a ragged 6); rnd64's
    columns exceed the LDS budget and run from the HBM scratch."""
    pes, r = rnd[tag]
    assert r['tof'].shape == (70,) and r['energies'].shape == (len(pes.minima), 70)
    check(r, fx, tag)


def test_tied_contributions_give_the_first_index(rnd, fx):
    """Two equal adjacent TS (3, 4) and two equal adjacent intermediates (1, 2):
    the reference reports the first of each pair (energy.py:282-287)."""
    pes, r = rnd['tie9']
    check(r, fx, 'tie9', max_skipped=1.0)
    assert np.array_equal(r['xTDTS'][0], r['xTDTS'][1]) and np.array_equal(r['xTDI'][0], r['xTDI'][1])
    ts, it = fx['tie9_tied_ts'], fx['tie9_tied_int']
    assert ts.sum() >= 10 and it.sum() >= 10
    assert np.all(r['iTDTS'][ts] == 3) and np.all(r['iTDI'][it] == 1)
    assert not np.any(r['iTDTS'] == 4) and not np.any(r['iTDI'] == 2)


@pytest.mark.parametrize('tag', ['rnd4', 'rnd5', 'rnd9', 'rnd20', 'rnd64'])
def test_single_condition_and_broadcast_temperature(rnd, fx, tag):
    pes, full = rnd[tag]
    E, T = fx[tag + '_E'], fx[tag + '_T']
    c = 37
    one = pes.evaluate_batch(T=T[c:c + 1], p=1.0e5, desc=desc_of(E, slice(c, c + 1)))          # n = 1
    assert one['tof'].shape == (1,)
    check(one, fx, tag, slice(c, c + 1), max_skipped=1.0)
    # every condition at T[c]: a scalar (stride 0) and a full column (stride 1) agree bit for bit
    s0 = pes.evaluate_batch(T=float(T[c]), p=1.0e5, desc=desc_of(E))
    s1 = pes.evaluate_batch(T=np.full(70, T[c]), p=np.full(70, 1.0e5), desc=desc_of(E))
    for k in ('tof', 'Espan', 'Eapp', 'dGrxn', 'iTDTS', 'iTDI', 'xTDTS', 'xTDI', 'energies'):
        assert np.array_equal(s0[k], s1[k]), k
        assert np.array_equal(s0[k][..., c], full[k][..., c]), k


def test_nan_descriptor_is_confined_to_its_column(rnd, fx):
    pes, full = rnd['rnd9']
    E = fx['rnd9_E'].copy()
    E[3, 5] = np.nan
    r = pes.evaluate_batch(T=fx['rnd9_T'], p=1.0e5, desc=desc_of(E))
    for k in ('tof', 'Espan', 'Eapp', 'dGrxn'):
        assert np.isnan(r[k][5]), k
    assert np.all(np.isnan(r['xTDTS'][:, 5])) and np.all(np.isnan(r['xTDI'][:, 5]))
    assert r['iTDTS'][5] == -1 and r['iTDI'][5] == -1
    rest = np.arange(70) != 5
    for k in ('tof', 'Espan', 'Eapp', 'dGrxn', 'iTDTS', 'iTDI', 'xTDTS', 'xTDI'):
        assert np.array_equal(r[k][..., rest], full[k][..., rest]), k


# -- (c) modifier ensemble ---------------------------------------------------------
def test_modifier_ensemble_70_members(inputs, fx):
    import pycatkin_amd as P
    sim = P.read_from_input_file(os.path.join(inputs, 'DMTM', 'input.json'))
    pes = sim.energy_landscapes['full_pes']
    before = pes.evaluate_batch(T=600.0, p=sim.params['pressure'])
    desc = {'ads': fx['ens_noise']}
    for s in fx['ens_ads']:
        sim.states[str(s)].set_energy_modifier(P.Descriptor('ads'))
    for k, s in enumerate(fx['ens_ts']):
        sim.states[str(s)].set_energy_modifier(P.Descriptor('ts_' + str(s)))
        desc['ts_' + str(s)] = fx['ens_ts_noise'][k]
    r = pes.evaluate_batch(T=600.0, p=sim.params['pressure'], desc=desc)      # not the stale plan
    assert r['tof'].shape == (70,) and before['tof'].shape == (1,)
    check(r, fx, 'ens')
    assert np.ptp(r['tof']) > 0.0
    # the electronic landscape does not see the modifiers
    e = pes.evaluate_batch(T=600.0, p=sim.params['pressure'], desc=desc, etype='electronic')
    close(e['energies'][:, 0], fx['dmtm_electronic_energies'][:, 0], 1e-10, 1e-12)
    assert np.ptp(e['energies'], axis=1).max() == 0.0


# -- drop-in path -------------------------------------------------------------------
def at(fx, T, p=1.0e5):
    return int(np.nonzero((fx['dmtm_T'] == T) & (fx['dmtm_p'] == p))[0][0])


@pytest.mark.parametrize('T, tdts, tdi', [(400.0, 'TS6', 'sCH3OH'), (800.0, 'TS3', 's2OCH4')])
def test_evaluate_energy_span_model(dmtm, fx, capsys, T, tdts, tdi):
    pes = dmtm.energy_landscapes['full_pes']
    c = at(fx, T)
    capsys.readouterr()
    tof, Espan, TDTS, TDI, num_i, num_j, lTi, lIj = pes.evaluate_energy_span_model(T=T, p=dmtm.params['pressure'])
    assert capsys.readouterr().out == str(fx['dmtm_free_stdout'][c])
    assert (TDTS, TDI) == (tdts, tdi) == (str(fx['dmtm_free_TDTS'][c]), str(fx['dmtm_free_TDI'][c]))
    close(tof, fx['dmtm_free_tof'][c], 1e-10)
    close(Espan, fx['dmtm_free_Espan'][c], 1e-10, 1e-12)
    close(num_i, fx['dmtm_free_xTDTS'][:, c], 0.0, 1e-10)
    close(num_j, fx['dmtm_free_xTDI'][:, c], 0.0, 1e-10)
    assert isinstance(num_i, list) and lTi == list(fx['dmtm_free_lTi']) and lIj == list(fx['dmtm_free_lIj'])
    land = pes.energy_landscape
    assert (land['T'], land['p']) == (T, dmtm.params['pressure'])
    for etype in ('free', 'electronic'):
        close([land[etype][k] for k in range(20)], fx['dmtm_%s_energies' % etype][:, c], 1e-10, 1e-12)
    assert [land['isTS'][k] for k in range(20)] == list(fx['dmtm_free_isTS'])


def test_run_energy_span_temperatures_and_save_pes_energies(inputs, fx, tmp_path, capsys):
    """test/test_1.py step 6: the four goldens read back from the summary CSV."""
    import pandas as pd
    import pycatkin_amd as P
    from pycatkin_amd.functions import presets
    sim = P.read_from_input_file(os.path.join(inputs, 'DMTM', 'input.json'))
    temps = [float(T) for T in np.linspace(400.0, 800.0, 17)]
    out = str(tmp_path) + os.sep
    capsys.readouterr()
    presets.run_energy_span_temperatures(sim, temps, save_results=True, csv_path=out)
    text = capsys.readouterr().out
    cols = [at(fx, T) for T in temps]
    assert text == 'Landscape full_pes:\n-----------------\n' + ''.join(str(fx['dmtm_free_stdout'][c]) for c in cols)
    assert sim.params['temperature'] == 800.0
    df = pd.read_csv(out + 'energy_span_summary_full_pes.csv')
    assert list(df.columns) == ['Temperature (K)', 'TOF (1/s)', 'Espan (eV)', 'TDTS', 'TDI']
    assert list(df['Temperature (K)']) == temps
    assert (df['TDTS'][0], df['TDI'][0]) == ('TS6', 'sCH3OH')
    assert (df['TDTS'][len(temps) - 1], df['TDI'][len(temps) - 1]) == ('TS3', 's2OCH4')
    close(df['TOF (1/s)'].values, fx['dmtm_free_tof'][cols], 1e-10)
    close(df['Espan (eV)'].values, fx['dmtm_free_Espan'][cols], 1e-10, 1e-12)
    xi = pd.read_csv(out + 'energy_span_xTDTS_full_pes.csv', header=None, skiprows=1).values
    xj = pd.read_csv(out + 'energy_span_xTDI_full_pes.csv', header=None, skiprows=1).values
    close(xi[:, 1:].T, fx['dmtm_free_xTDTS'][:, cols], 0.0, 1e-10)
    close(xj[:, 1:].T, fx['dmtm_free_xTDI'][:, cols], 0.0, 1e-10)
    head = open(out + 'energy_span_xTDTS_full_pes.csv').readline().strip().split(',')
    assert head == ['Temperature (K)'] + list(fx['dmtm_free_lTi'])
    # save_pes_energies at the params the sweep left (800 K, 1 bar)
    presets.save_pes_energies(sim, csv_path=out)
    df = pd.read_csv(out + 'full_pes_energy_landscape_800.0K_1.0bar.csv')
    assert list(df.columns) == ['State', 'Free (eV)', 'Electronic (eV)']
    assert list(df['State']) == sim.energy_landscapes['full_pes'].labels
    c = at(fx, 800.0)
    close(df['Free (eV)'].values, fx['dmtm_free_energies'][:, c], 1e-10, 1e-12)
    close(df['Electronic (eV)'].values, fx['dmtm_electronic_energies'][:, c], 1e-10, 1e-12)


# -- overflow ------------------------------------------------------------------------
def logspace_span(E, is_ts, T):
    """The reference's formulas (energy.py:250-300) restated in logs."""
    x = np.asarray(E, float) * EV2JMOL / (R * T)
    N = len(x)
    ts = [i for i in range(N - 1) if is_ts[i]]
    im = [j for j in range(1, N - 1) if not is_ts[j]]
    X = np.array([[x[i] - x[j] - (x[N - 1] if i >= j else 0.0) for j in im] for i in ts])
    m = X.max()
    S = np.exp(X - m)
    lnden = m + np.log(S.sum())
    lt = -x[N - 1] - 1.0 - lnden
    return dict(Eapp=lt * (-R * T) * 1.0e-3, lntof=np.log(KB * T / H) + lt, xTDTS=S.sum(axis=1) / S.sum(),
                xTDI=S.sum(axis=0) / S.sum(), iTDTS=ts[int(np.argmax(S.sum(axis=1)))],
                iTDI=im[int(np.argmax(S.sum(axis=0)))])


def test_no_overflow_where_the_reference_overflows(fx):
    """[0, 12, -12, -1] eV at 150 K: X/RT = 1857, the reference returns inf / NaN."""
    E, is_ts, T = [0.0, 12.0, -12.0, -1.0], [0, 1, 0, 0], 150.0
    r = stub_landscape(is_ts, E, 'steep').evaluate_batch(T=T, p=1.0e5)
    for k in ('tof', 'Espan', 'Eapp', 'dGrxn', 'xTDTS', 'xTDI', 'energies'):
        assert not np.any(np.isnan(r[k])), k
    assert r['iTDTS'][0] == 1 and r['iTDI'][0] == 2
    assert np.array_equal(r['xTDTS'][:, 0], [1.0]) and np.array_equal(r['xTDI'][:, 0], [1.0])
    ref = logspace_span(E, is_ts, T)
    close(r['Eapp'][0], ref['Eapp'], 1e-12)
    assert r['tof'][0] == 0.0 or np.isfinite(r['tof'][0])
    close(r['Espan'][0], 24.0, 1e-12)


def test_pair_by_pair_sum_where_the_maxima_do_not_meet(fx):
    """The highest TS, the lowest intermediate and exp(-drxn/RT) do not share a
    pair and lie > 1e300 apart: the shifted separable sum underflows and the
    lane sums the pairs one by one."""
    E, is_ts, T = [0.0, 12.0, 12.0, -12.0, -12.0, -11.7], [0, 0, 1, 0, 1, 0], 150.0
    r = stub_landscape(is_ts, E, 'apart').evaluate_batch(T=T, p=1.0e5)
    ref = logspace_span(E, is_ts, T)
    close(r['Eapp'][0], ref['Eapp'], 1e-12)
    close(r['xTDTS'][:, 0], ref['xTDTS'], 0.0, 1e-12)
    close(r['xTDI'][:, 0], ref['xTDI'], 0.0, 1e-12)
    assert (r['iTDTS'][0], r['iTDI'][0]) == (ref['iTDTS'], ref['iTDI']) == (2, 3)
    assert r['tof'][0] == 0.0 and ref['lntof'] < -745.0


# -- refusals ------------------------------------------------------------------------
@pytest.mark.parametrize('is_ts, message', [
    ([0, 1, 0], 'entries'),
    ([1, 0, 1, 0, 0], 'first landscape entry is a transition state'),
    ([0, 0, 1, 0, 1], 'last landscape entry is a transition state'),
    ([0, 0, 0, 0, 0], 'no transition state'),
    ([0, 1, 1, 1, 0], 'no intermediate'),
    ([0, 1] + [0] * 63, 'entries'),
])
def test_refused_landscapes(rnd, is_ts, message):
    pes, _ = rnd['rnd64']
    net, regs, _ = pes._device()
    regs = (regs['free'] + regs['free'])[:len(is_ts)]
    with pytest.raises(RuntimeError, match=message):
        net.energy_span(1, 500.0, 1.0e5, (regs, is_ts), desc=np.zeros(64))
