"""Energy-span goldens from the REFERENCE's own Energy class
(pycatkin/classes/energy.py, importable where the reference tree is present;
not on the GPU box).

What runs from the reference, unmodified: Energy.construct_energy_landscape
and Energy.evaluate_energy_span_model.  What is supplied here: the states --
make_golden.DuckState (free energies from oracle.mk_oracle.Thermo) for the
DMTM landscape, and stub states that return a given number for the random
landscapes.

  (a) dmtm_*   DMTM 'full_pes', 17 temperatures 400..800 K x p in {1e4, 1e5, 1e6} Pa,
               both etypes: the eight return values, the landscape dicts, stdout
  (b) rnd<N>_* random landscapes, N in {4, 5, 9, 20, 64}, 70 conditions each, and
               tie9_*: N = 9 with two equal adjacent TS and two equal adjacent
               intermediates (the first-maximum rule)
  (c) ens_*    DMTM at 600 K, 70 members of a correlated energy-noise ensemble
               (the structure of pycatkin/classes/uncertainty.py:35-65)
  spread_*     per DMTM temperature, the relative spread of the float64 TOF
               between three summation orders of the same state energies

Output: tests/golden/energy_span_fixture.npz.
Run:    python tests/golden/make_energy_span_fixture.py
"""
import contextlib
import io
import math
import os
import sys

import numpy as np

os.environ.setdefault('MPLBACKEND', 'Agg')
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import make_golden as MG  # noqa: E402  (puts the reference tree on sys.path)
from oracle import mk_oracle as O  # noqa: E402
from pycatkin.classes.energy import Energy  # noqa: E402
from pycatkin.constants.physical_constants import R, eVtokJ, h, kB  # noqa: E402

INPUT = os.path.join(HERE, 'inputs', 'DMTM', 'input.json')
TEMPS = np.linspace(400.0, 800.0, 17)          # examples/DMTM/dmtm.py
PRESSURES = [1.0e4, 1.0e5, 1.0e6]
NCOND = 70                                     # one full wavefront and a ragged 6


def evaluate(pes, T, p, etype):
    """One reference evaluation: (return tuple, stdout, landscape dict)."""
    pes.energy_landscape = None
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = pes.evaluate_energy_span_model(T=T, p=p, etype=etype)
    return res, buf.getvalue(), pes.energy_landscape


def indices(is_ts, num_i, num_j):
    """energy.py:282-287: landscape indices of the first maxima."""
    ts = [k for k in range(len(is_ts)) if is_ts[k] == 1]
    it = [k for k in range(len(is_ts))][1:]
    it = [k for k in it if is_ts[k] == 0]
    return ts[[i for i in range(len(num_i)) if num_i[i] == max(num_i)][0]], \
        it[[j for j in range(len(num_j)) if num_j[j] == max(num_j)][0]]


def top_gap(v):
    s = np.sort(np.asarray(v, float))
    return s[-1] - s[-2] if s.size > 1 else 1.0


def collect(pes, conds, etype, setup=None):
    """Evaluate `pes` at every (T, p) of conds; setup(c) prepares condition c."""
    out = dict(tof=[], Espan=[], Eapp=[], dGrxn=[], iTDTS=[], iTDI=[], xTDTS=[], xTDI=[], energies=[], gap_ts=[],
               gap_int=[], stdout=[], TDTS=[], TDI=[])
    for c, (T, p) in enumerate(conds):
        if setup is not None:
            setup(c)
        (tof, Espan, TDTS, TDI, num_i, num_j, lTi, lIj), text, land = evaluate(pes, T, p, etype)
        N = len(land['isTS'])
        is_ts = [land['isTS'][k] for k in range(N)]
        it, ii = indices(is_ts, num_i, num_j)
        assert pes.labels[it] == TDTS and pes.labels[ii] == TDI
        out['tof'].append(tof)
        out['Espan'].append(Espan)
        out['Eapp'].append(np.log((h * tof) / (kB * T)) * (-R * T) * 1.0e-3)        # energy.py:300
        out['dGrxn'].append(land[etype][N - 1])
        out['iTDTS'].append(it)
        out['iTDI'].append(ii)
        out['xTDTS'].append(num_i)
        out['xTDI'].append(num_j)
        out['energies'].append([land[etype][k] for k in range(N)])
        out['gap_ts'].append(top_gap(num_i))
        out['gap_int'].append(top_gap(num_j))
        out['stdout'].append(text)
        out['TDTS'].append(TDTS)
        out['TDI'].append(TDI)
    out['lTi'], out['lIj'], out['isTS'] = lTi, lIj, is_ts
    return out


def pack(store, prefix, r, keep_stdout=False):
    for k in ('tof', 'Espan', 'Eapp', 'dGrxn', 'gap_ts', 'gap_int'):
        store['%s_%s' % (prefix, k)] = np.array(r[k], float)
    for k in ('iTDTS', 'iTDI', 'isTS'):
        store['%s_%s' % (prefix, k)] = np.array(r[k], np.int32)
    store['%s_xTDTS' % prefix] = np.array(r['xTDTS'], float).T          # [nTi, n]
    store['%s_xTDI' % prefix] = np.array(r['xTDI'], float).T            # [nIj-1, n]
    store['%s_energies' % prefix] = np.array(r['energies'], float).T    # [N, n]
    for k in ('lTi', 'lIj', 'TDTS', 'TDI'):
        store['%s_%s' % (prefix, k)] = np.array(r[k])
    if keep_stdout:
        store['%s_stdout' % prefix] = np.array(r['stdout'])
    for k in ('tof', 'Espan', 'Eapp', 'dGrxn', 'xTDTS', 'xTDI', 'energies'):
        assert np.all(np.isfinite(np.array(r[k], float))), (prefix, k)     # no reference output is non-finite


# ----------------------------------------------------------------------------
# (a) + (c): the DMTM landscape over DuckStates
# ----------------------------------------------------------------------------
def dmtm_landscape(spec):
    import json
    pes = json.load(open(INPUT))['energy landscapes']['full_pes']
    states = {n: MG.DuckState(spec, n) for n in spec['states']}
    return Energy(name='full_pes', minima=[[states[s] for s in entry] for entry in pes['minima']], labels=None)


def span_logspace(E, is_ts, T):
    """TOF of landscape energies E (eV, relative to E[0]) -- the reference's
    formula with the pair sum shifted by its maximum."""
    x = np.asarray(E, float) * eVtokJ * 1.0e3 / (R * T)
    N = len(x)
    X = [x[i] - x[j] - (x[N - 1] if i >= j else 0.0) for i in range(N - 1) if is_ts[i]
         for j in range(1, N - 1) if not is_ts[j]]
    m = max(X)
    return (kB * T / h) * math.exp(-x[N - 1] - 1.0 - m - math.log(math.fsum(math.exp(v - m) for v in X)))


def summation_spread(spec, minima, is_ts, T, p):
    th = O.Thermo(spec, T, p)
    G = {s: th.free(s) for entry in minima for s in entry}
    fwd = [sum(G[s] for s in entry) for entry in minima]
    rev = [sum(G[s] for s in reversed(entry)) for entry in minima]
    sym = []
    for entry in minima:                     # states shared with entry 0 cancel before any number is added
        a, b = list(entry), list(minima[0])
        for s in list(a):
            if s in b:
                a.remove(s)
                b.remove(s)
        sym.append(math.fsum([G[s] for s in a] + [-G[s] for s in b]))
    tofs = [span_logspace([e - E[0] for e in E], is_ts, T) for E in (fwd, rev)] + [span_logspace(sym, is_ts, T)]
    return (max(tofs) - min(tofs)) / np.mean(tofs)


def main():
    import json
    store = {}
    spec = O.load_spec(INPUT)
    p0 = spec['system']['p']
    conds = [(float(T), p) for p in PRESSURES for T in TEMPS]
    store['dmtm_T'] = np.array([c[0] for c in conds])
    store['dmtm_p'] = np.array([c[1] for c in conds])
    res = {}
    for etype in ('free', 'electronic'):
        res[etype] = collect(dmtm_landscape(spec), conds, etype)
        pack(store, 'dmtm_' + etype, res[etype], keep_stdout=True)
    # test/test_1.py step 6 at the input's pressure
    at = {(T, p): c for c, (T, p) in enumerate(conds)}
    f = res['free']
    assert (f['TDTS'][at[(400.0, p0)]], f['TDI'][at[(400.0, p0)]]) == ('TS6', 'sCH3OH')
    assert (f['TDTS'][at[(800.0, p0)]], f['TDI'][at[(800.0, p0)]]) == ('TS3', 's2OCH4')
    minima = json.load(open(INPUT))['energy landscapes']['full_pes']['minima']
    store['spread_T'] = TEMPS
    store['spread_tof'] = np.array([summation_spread(spec, minima, f['isTS'], float(T), p0) for T in TEMPS])

    # (b) random landscapes over stub states
    class Stub:
        def __init__(self, name, state_type):
            self.name, self.state_type, self.G, self.Gelec = name, state_type, 0.0, 0.0

        def get_free_energy(self, T, p, verbose=False):
            return self.G

    rng = np.random.default_rng(20240607)
    gaps = [np.minimum(r['gap_ts'], r['gap_int']) for r in res.values()]
    for tag, N in (('rnd4', 4), ('rnd5', 5), ('rnd9', 9), ('rnd20', 20), ('rnd64', 64), ('tie9', 9)):
        if N == 4:
            is_ts = [0, 1, 0, 0]
        elif tag == 'tie9':
            is_ts = [0, 0, 0, 1, 1, 0, 1, 1, 0]
        else:
            is_ts = [0] + [int(v) for v in rng.integers(0, 2, N - 2)] + [0]
            is_ts[1], is_ts[N - 3], is_ts[N - 2] = 0, 1, 1         # intermediate at 1, adjacent TS, TS at N-2
        stubs = [Stub('%s%d' % ('T' if is_ts[k] else 'I', k), 'TS' if is_ts[k] else 'adsorbate') for k in range(N)]
        pes = Energy(name=tag, minima=[[s] for s in stubs], labels=None)
        E = rng.uniform(-1.5, 1.5, (N, NCOND))
        T = rng.uniform(300.0, 900.0, NCOND)
        if tag == 'tie9':
            # the two adjacent TS (3, 4) share the highest TS energy and the two
            # adjacent intermediates (1, 2) the lowest intermediate energy
            E[3] = E[4] = np.max(E[[3, 4, 6, 7]], axis=0)
            E[1] = E[2] = np.min(E[[1, 2, 5]], axis=0)

        def setup(c, stubs=stubs, E=E):
            for k, s in enumerate(stubs):
                s.G = float(E[k, c])
        r = collect(pes, [(float(t), 1.0e5) for t in T], 'free', setup)
        pack(store, tag, r)
        store[tag + '_E'], store[tag + '_T'] = E, T
        if tag == 'tie9':
            r_i, r_j = np.array(r['iTDTS']), np.array(r['iTDI'])
            assert np.sum(r_i == 3) >= 10 and np.sum(r_j == 1) >= 10, (r_i, r_j)   # the first of each tied pair
            assert not np.any(r_i == 4) and not np.any(r_j == 2)
            store['tie9_tied_ts'] = (r_i == 3)
            store['tie9_tied_int'] = (r_j == 1)
        else:
            gaps.append(np.minimum(r['gap_ts'], r['gap_int']))
        # |Ti - Ij - dGij| <= 6 max|E| relative to entry 0: the reference cannot overflow
        assert float(6.0 * np.max(np.abs(E)) * eVtokJ * 1.0e3 / (R * 300.0)) < 709.0

    # (c) correlated energy-noise ensemble on the DMTM landscape (uncertainty.py:35-65)
    rng = np.random.default_rng(0)
    pes = dmtm_landscape(spec)
    seen = []
    for entry in pes.minima:
        for s in entry:
            if s.name not in seen:
                seen.append(s.name)
    ads = [s for s in seen if spec['states'][s]['type'] == 'adsorbate']
    tss = [s for s in seen if spec['states'][s]['type'] == 'TS']
    noise = np.zeros(NCOND)
    ts_noise = np.zeros((len(tss), NCOND))
    for c in range(NCOND):
        noise[c] = rng.normal(0.0, 0.1)
        ts_noise[:, c] = noise[c] * rng.uniform(0.0, 1.0, len(tss))

    def setup(c):
        for s in ads:
            spec['states'][s]['add_to_energy'] = float(noise[c])
        for k, s in enumerate(tss):
            spec['states'][s]['add_to_energy'] = float(ts_noise[k, c])
    r = collect(pes, [(600.0, p0)] * NCOND, 'free', setup)
    pack(store, 'ens', r)
    # the electronic energies do not see the modifiers
    e = collect(pes, [(600.0, p0)] * 2, 'electronic', setup)
    assert np.array_equal(np.array(e['energies'][0]), np.array(res['electronic']['energies'][0]))
    store['ens_noise'], store['ens_ts_noise'] = noise, ts_noise
    store['ens_ads'], store['ens_ts'] = np.array(ads), np.array(tss)
    gaps.append(np.minimum(r['gap_ts'], r['gap_int']))

    # near ties of the reference's own top two contributions (deliberate ties aside)
    allg = np.concatenate(gaps)
    share = float(np.mean(allg < 1.0e-6))
    assert share <= 0.02, share
    print('near-tie share %.4f over %d conditions; TOF spread %.2e (400 K) %.2e (800 K)'
          % (share, allg.size, store['spread_tof'][0], store['spread_tof'][-1]))
    out = os.path.join(HERE, 'energy_span_fixture.npz')
    np.savez_compressed(out, **store)
    print('wrote %s (%d bytes)' % (out, os.path.getsize(out)))


if __name__ == '__main__':
    main()
