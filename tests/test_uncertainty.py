"""Uncertainty (pycatkin_amd/classes/uncertainty.py), the parts that need no
GPU: the reference's draw order (tests/golden/uncertainty_fixture.npz part
(1), written from the reference's own class), the partition of the states,
the single ensemble plan, and the Philox4x32-10 restatement the GPU test
measures the noise kernel with."""
import copy
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'golden'))
import _philox  # noqa: E402
from make_butadiene_fixture import CASES, kept_reactions  # noqa: E402

FIXTURE = os.path.join(HERE, 'golden', 'uncertainty_fixture.npz')


@pytest.fixture(scope='module')
def fx():
    return dict(np.load(FIXTURE))


def dmtm_system(inputs):
    import pycatkin_amd as P
    return P.read_from_input_file(os.path.join(inputs, 'DMTM', 'input.json'))


def butadiene_system(inputs, case='p123_p124_p156'):
    """butadiene_mkm.py:47-61: the MKM on its DFT base system, the set's reactions only."""
    from pycatkin_amd.functions.load_input import read_from_input_file
    d = os.path.join(inputs, 'Butadiene')
    dft = read_from_input_file(os.path.join(d, 'input.json'))
    s = copy.deepcopy(read_from_input_file(os.path.join(d, 'input_mkm.json'), base_system=dft))
    keep = kept_reactions(list(s.reactions), case, dict(CASES)[case])
    for r in list(s.reactions):
        if r not in keep:
            del s.reactions[r]
    s.names_to_indices()
    return s, dft


@pytest.mark.parametrize('which', ['dmtm', 'bd'])
def test_reference_draw_order(inputs, fx, which):
    """After the same np.random.seed, 8 consecutive get_correlated_state_noises()
    dicts are the reference's: the same keys in the same order, the same bits."""
    import pycatkin_amd as P
    sim = dmtm_system(inputs) if which == 'dmtm' else butadiene_system(inputs)[0]
    unc = P.Uncertainty(sys=sim, mu=float(fx['mu']), sigma=float(fx['sigma']), nruns=8)
    keys, vals = [str(k) for k in fx['draw_%s_keys' % which]], fx['draw_%s_vals' % which]
    np.random.seed(int(fx['seed']))
    for run in range(8):
        d = unc.get_correlated_state_noises()
        assert list(d) == keys
        assert [d[k] for k in keys] == list(vals[run])
    # sample_noises(rng='numpy') is the same stream, run by run
    s = unc.sample_noises(8, rng='numpy', seed=int(fx['seed']))
    ads, tss = unc.noise_states()
    assert list(s) == ads + tss
    for j, k in enumerate(keys):
        assert np.array_equal(s[k], vals[:, j])


def test_noise_states_partition_dmtm(inputs):
    import pycatkin_amd as P
    sim = dmtm_system(inputs)
    unc = P.Uncertainty(sys=sim, mu=0.0, sigma=0.05)
    ads, tss = unc.noise_states()
    assert ads and tss and not set(ads) & set(tss)
    assert all(unc.sys.states[a].state_type == 'adsorbate' for a in ads)
    assert all(unc.sys.states[t].state_type == 'TS' for t in tss)
    # every adsorbate / TS of a reaction, nothing else
    want_ads = {s.name for r in unc.sys.reactions.values() for s in r.reactants + r.products if s.state_type == 'adsorbate'}
    want_ts = {s.name for r in unc.sys.reactions.values() for s in (r.TS or [])}
    assert set(ads) == want_ads and set(tss) == want_ts
    np.random.seed(3)
    d = unc.get_correlated_state_noises()
    assert len({d[a] for a in ads}) == 1                     # one shared value
    assert len({d[t] for t in tss}) == len(tss)              # one value each
    noisy = unc.set_correlated_state_noises(d)
    for name, st in noisy.states.items():
        if name in d:
            assert st.add_to_energy == d[name]
        else:                                                # gas, surface: untouched
            assert st.state_type in ('gas', 'surface') or name not in want_ads | want_ts
            assert st.add_to_energy == sim.states[name].add_to_energy
    assert all(sim.states[n].add_to_energy is None for n in d)


def test_state_of_a_deleted_reaction_is_untouched(inputs):
    import pycatkin_amd as P
    sim = dmtm_system(inputs)
    full_ads, full_ts = P.Uncertainty(sys=sim).noise_states()
    victim = [r for r in sim.reactions.values() if r.TS][-1]
    gone_ts = victim.TS[0].name
    del sim.reactions[victim.name]
    unc = P.Uncertainty(sys=sim, sigma=0.05)
    ads, tss = unc.noise_states()
    assert gone_ts in full_ts and gone_ts not in tss and len(tss) == len(full_ts) - 1
    ens = unc.ensemble_system()
    assert ens.states[gone_ts].add_to_energy is None
    assert len(ens.plan().descriptors) == 1 + len(tss)


def test_butadiene_names_come_from_the_base_system(inputs, fx):
    import pycatkin_amd as P
    sim, dft = butadiene_system(inputs)
    unc = P.Uncertainty(sys=sim, sigma=0.05)
    ads, tss = unc.noise_states()
    assert ads + tss and sorted(ads + tss) == sorted(str(k) for k in fx['draw_bd_keys'])
    assert all(n in dft.states for n in ads + tss)
    assert not any(n in sim.states and sim.states[n].state_type == 'adsorbate' for n in tss)
    ens = unc.ensemble_system()
    # the MKM's own adsorbates (the dynamic species) carry no modifier: the
    # derived reactions take their energies from the base reactions' states
    from pycatkin_amd.energy import LinearForm
    carried = [s for r in ens.reactions.values() for s in
               r.base_reaction.reactants + r.base_reaction.products + (r.base_reaction.TS or [])
               if isinstance(s.add_to_energy, LinearForm)]
    assert {s.name for s in carried} == set(ads + tss)


@pytest.mark.parametrize('which', ['dmtm', 'bd'])
def test_one_plan_for_every_noise_draw(inputs, which):
    import pycatkin_amd as P
    sim = dmtm_system(inputs) if which == 'dmtm' else butadiene_system(inputs)[0]
    before = {n: copy.deepcopy(s.add_to_energy) for n, s in sim.states.items()}
    unc = P.Uncertainty(sys=sim, mu=0.0, sigma=0.05, nruns=4)
    ads, tss = unc.noise_states()
    ens = unc._ensemble()
    plan = ens.plan()
    assert list(plan.descriptors) == ['@unc:ads'] + ['@unc:ts:' + t for t in tss]
    assert len(plan.descriptors) == 1 + len(tss)
    ip, dp = plan.ip.copy(), plan.dp.copy()
    np.random.seed(1)
    a = unc.sample_noises(4, rng='numpy')
    np.random.seed(2)
    b = unc.sample_noises(4, rng='numpy')
    assert not np.array_equal(a[ads[0]], b[ads[0]])
    assert unc._ensemble() is ens and ens.plan() is plan
    assert np.array_equal(plan.ip, ip) and np.array_equal(plan.dp, dp, equal_nan=True)
    # a second ensemble system of the same sys compiles to the same blobs
    other = unc.ensemble_system().plan()
    assert np.array_equal(other.ip, ip) and np.array_equal(other.dp, dp, equal_nan=True)
    # neither the caller's system nor the class's copy is modified
    for s in (sim, unc.sys):
        assert {n: st.add_to_energy for n, st in s.states.items()} == before
        assert getattr(s, 'descriptor_order', None) is None and getattr(s, 'desc_defaults', None) is None
    assert len(sim.plan().descriptors) == 0


def test_member_systems_share_the_ensemble_plan(inputs):
    import pycatkin_amd as P
    unc = P.Uncertainty(sys=dmtm_system(inputs), sigma=0.05)
    ens = unc._ensemble()
    m = unc._member(ens, {k: 0.01 for k in ens.descriptor_order})
    assert m.plan() is ens.plan() and m._plans is ens._plans
    assert m.desc_defaults != ens.desc_defaults and m.params is not ens.params


KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_restatement_known_answers():
    """The published Philox4x32-10 known-answer vectors (Random123 kat_vectors)."""
    for ctr, key, out in KAT:
        got = _philox.philox4x32_10(np.array(ctr, np.uint64), np.array(key, np.uint64))
        assert tuple(int(x) for x in got) == out
    # vectorised over counters, and the block() counter layout (lo, hi, j, 0)
    ctr = np.array([k[0] for k in KAT[:1]] * 3, np.uint64)
    assert np.array_equal(_philox.philox4x32_10(ctr, np.zeros(2, np.uint64)), np.array([KAT[0][2]] * 3, np.uint32))
    run = (0x85a308d3 << 32) | 0x243f6a88
    seed = (0x299f31d0 << 32) | 0xa4093822
    got = _philox.philox4x32_10(np.array([[run & 0xffffffff, run >> 32, 0x13198a2e, 0]], np.uint64),
                                np.array([seed & 0xffffffff, seed >> 32], np.uint64))
    assert np.array_equal(_philox.block(seed, [run], 0x13198a2e), got)
    u = _philox.uniforms(7, np.arange(100, dtype=np.uint64), 3)
    z = _philox.normal(7, np.arange(100, dtype=np.uint64))
    assert u.shape == (3, 100) and np.all((u >= 0.0) & (u < 1.0)) and np.all(np.isfinite(z))
