"""The bed DRC on the CPU: the restatement tests/_sens_cascade.py against its
fixture (tests/golden/cascade_drc_fixture.npz, make_cascade_drc_fixture.py),
against tests/_sens_multi.py for a bed of one cell, and against the closed form
of a linear two-cell bed; the Python surface that needs no device.  The kernel
itself is checked in tests/test_gpu_cascade_drc.py."""
import ctypes
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')
sys.path.insert(0, HERE)
sys.path.insert(0, GOLD)

import _sens_cascade as SC  # noqa: E402
import _sens_multi as SM  # noqa: E402


@pytest.fixture(scope='module')
def fx():
    return np.load(os.path.join(GOLD, 'cascade_drc_fixture.npz'))


@pytest.fixture(scope='module')
def spec():
    from oracle import mk_oracle as O
    return O.load_spec(os.path.join(GOLD, 'inputs', 'COOxReactor', 'input_Pd111.json'))


def case(fx, i):
    pre = 'c%d_' % i
    return {k[len(pre):]: fx[k] for k in fx.files if k.startswith(pre)}


def test_fixture_contents(fx):
    """What the generator promises: 12 Pd111 cases (4 temperatures x 1, 2, 8
    cells), the TOF and an outlet objective in each, at most one case without
    its outlet objectives, the finite-difference check of the formula passed."""
    names = [str(n) for n in fx['names']]
    assert len(names) == 12
    assert sorted({int(case(fx, i)['cells']) for i in range(12)}) == [1, 2, 8]
    lost = 0
    for i in range(12):
        c = case(fx, i)
        labels = [str(x) for x in c['labels']]
        assert 'tof' in labels and any(lb.startswith('outlet[') for lb in labels), names[i]
        lost += any(str(x).startswith('outlet[') for x in c['dropped'])
        assert float(c['fd_ratio']) <= 1.0
        K, R, NS = len(labels), len(fx['rnames']), len(fx['dyn'])
        assert c['xi_ref'].shape == (K, R) and c['order_in_ref'].shape == (K, NS)
        assert c['y_cells'].shape == (int(c['cells']), NS)
    assert lost <= 1
    assert float(fx['fd_ratio']) <= 1.0


@pytest.mark.parametrize('i', range(12))
def test_restatement_at_104_bits(fx, spec, i):
    """_sens_cascade at 104 bits at the stored states: the stored xi_104 /
    order_in_104 again (the same arithmetic: 1e-15), hence xi_ref within the
    GPU test's bound."""
    from make_cascade_drc_fixture import bed_models
    c = case(fx, i)
    ms = bed_models(spec, float(c['T']), c['y_full'])
    assert np.array_equal(ms[0].kf, c['kf']) and np.array_equal(ms[0].kr, c['kr'])
    xi, val, oi = SC.cascade_drc_mp(ms, c['y_full'], list(zip(c['wr'], c['wy'])), 104)
    xi = np.array([[float(x) for x in r] for r in xi])
    oi = np.array([[float(x) for x in r] for r in oi])
    np.testing.assert_allclose(xi, c['xi_104'], rtol=1e-15, atol=1e-300)
    np.testing.assert_allclose(oi, c['order_in_104'], rtol=1e-15, atol=1e-300)
    assert np.all(np.abs(xi - c['xi_ref']) <= 1e-12 + 1e-12 * np.abs(c['xi_ref']) + 10 * np.abs(c['xi_104'] - c['xi_ref']))
    np.testing.assert_allclose([float(v) for v in val], c['val_ref'], rtol=1e-15)


@pytest.mark.parametrize('i', [0, 3, 6, 9])
def test_one_cell_is_the_tank(fx, spec, i):
    """A bed of one cell is _sens_multi's single tank, exactly (rationals)."""
    from make_cascade_drc_fixture import bed_models
    c = case(fx, i)
    assert int(c['cells']) == 1
    ms = bed_models(spec, float(c['T']), c['y_full'])
    obj = list(zip(c['wr'], c['wy']))
    xi, val, _ = SC.cascade_drc(ms, c['y_full'], obj, Fraction)
    xm, vm = SM.multi_drc(ms[0], c['y_full'][0], obj, Fraction)
    assert xi == xm and val == vm


class _LinearCell:
    """One species A fed at u, consumed by A -> (nothing tracked) at k a: the
    attributes of the oracle model that _sens_cascade reads."""
    snames = ['A']
    rnames = ['R0']
    dyn = [0]
    jcols = np.array([0])
    cfac = np.array([1.0])
    Ef = np.array([[1.0]])
    Er = np.array([[0.0]])
    W = np.array([[-1.0]])
    is_gas = np.array([1.0])
    unreach = np.array([False])

    def __init__(self, k, tau, u):
        self.kf, self.kr = np.array([k]), np.array([0.0])
        self.reactor = dict(kind='CSTR', residence_time=tau)
        self.yin = np.array([u])

    def rowscale(self):
        return np.array([1.0])

    def conservation(self):
        return np.zeros((0, 1))


def test_linear_two_cell_bed_closed_form():
    """a_c = u_c phi / (phi + k): outlet a_1 = u r^2 with r = phi / (phi + k), so
    d ln a_1 / d ln k = -2 k / (phi + k); the bed-mean rate k u r (1 + r) / 2 has
    d ln J / d ln k = 1 - (k / (phi + k)) (1 + r / (1 + r)); both are linear in
    the feed: order_in = 1."""
    k, tau, u = Fraction(6), Fraction(1, 2), Fraction(5, 4)     # r = 1/4: every state exact in binary
    phi = 1 / tau
    r = phi / (phi + k)
    a0, a1 = u * r, u * r * r
    ms = [_LinearCell(float(k), float(tau), float(u)), _LinearCell(float(k), float(tau), float(a0))]
    ys = [np.array([float(a0)]), np.array([float(a1)])]
    assert Fraction(float(a0)) == a0 and Fraction(float(a1)) == a1
    xi, val, oi = SC.cascade_drc(ms, ys, [([0.0], [1.0]), ([1.0], [0.0])], Fraction)
    s = k / (phi + k)
    assert val == [a1, k * u * r * (1 + r) / 2]
    assert xi[0] == [-2 * s]
    assert xi[1] == [1 - s * (1 + r / (1 + r))]
    assert oi == [[Fraction(1)], [Fraction(1)]]


def test_pfr_system_refuses_single_tank_drc():
    """drc_batch, drc_at and the multi-objective forms on a PFReactor system
    raise and name cascade_drc_batch (no device is touched before the check)."""
    import pycatkin_amd as P
    s = P.read_from_input_file(os.path.join(GOLD, 'inputs', 'COOxReactor', 'input_Pd111.json'))
    s.add_reactor(P.PFReactor(cells=2, residence_time=4.5, volume=1.8e-7, catalyst_area=3.82e-9))
    y = np.zeros((6, 1))
    for call in (lambda: s.drc_batch(('CO_ox',), T=500.0, steady=True, method='analytic'),
                 lambda: s.drc_at(('CO_ox',), y, T=500.0),
                 lambda: s.drc_objectives_at([('CO_ox',)], y, T=500.0),
                 lambda: s.drc_objectives_batch([('CO_ox',)], T=500.0)):
        with pytest.raises(ValueError, match='cascade_drc_batch'):
            call()


def test_binding_lists_the_entry_points():
    from pycatkin_amd import _lib
    for name in ('pck_cascade_drc_at', 'pck_cascade_drc'):
        assert name in _lib.EXPORTED and name in _lib.OPTIONAL
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'pycatkin_amd.h')).read()
    assert '#define PCK_ABI_VERSION %d' % _lib.ABI_VERSION in hdr


def test_null_arguments_are_refused_without_a_device():
    """check_cond runs before anything touches the device."""
    from pycatkin_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        pytest.skip('library not built (run __graft_entry__.build())')
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('pck_cascade_drc_at', 'pck_cascade_drc'):
        fn = getattr(lib, name)
        fn.restype = ctypes.c_int
        args = [None] * (15 if name == 'pck_cascade_drc_at' else 10)
        if name == 'pck_cascade_drc_at':
            args[4], args[6], args[7], args[9], args[13] = (ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int32(1),
                                                            ctypes.c_int64(0), ctypes.c_int64(0))
        else:
            args[7] = ctypes.c_int64(0)
        assert fn(*args) == _lib.E_ARG
