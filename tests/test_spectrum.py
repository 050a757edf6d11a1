"""Linear stability, the parts that need no GPU (DESIGN.md "Linear stability"):
the C-ABI declarations of pck_eigvals / pck_stability_at / pck_stability, the
Python argument checks of System.stability_at / stability_batch and of the
opt-in eig='device' path of the convergence check, and the consistency of
tests/golden/spectrum_fixture.npz."""
import inspect
import os
import re

import numpy as np
import pytest

import test_capi as CAPI
from pycatkin_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
FX = np.load(os.path.join(HERE, 'golden', 'spectrum_fixture.npz'))
NAMES = [str(x) for x in FX['names']]
VOLCANO = [(-1.0, -1.0), (-2.5, -2.5), (0.5, 0.5), (-2.5, 0.5), (0.5, -2.5), (-1.3, -0.4)]


def case(name):
    pre = 'm%d_' % NAMES.index(name)
    return {k[len(pre):]: FX[k] for k in FX.files if k.startswith(pre)}


# ------------------------------------------------------------------ the C-ABI
def test_new_symbols_are_declared_and_bound():
    for sym in ('pck_eigvals', 'pck_stability_at', 'pck_stability'):
        assert sym in CAPI.declared_symbols(), sym
        assert sym in _lib.EXPORTED, sym
    txt = open(CAPI.HDR).read()
    assert re.search(r'#define PCK_ST_EIG_NOCONV 9\b', txt) and _lib.ST_EIG_NOCONV == 9
    assert re.search(r'#define PCK_ABI_VERSION 10\b', txt) and _lib.ABI_VERSION == 10
    assert re.search(r'int pck_eigvals\(const double\* a, int ns, int64_t n, int64_t ld, const int32_t\* status_in, '
                     r'double re_tol,\s+int lanes, const pck_eig_out\* out, int32_t\* lanes_used, void\* stream\);', txt)
    assert _lib.EIG_LANES_MODES == {'group': _lib.SENS_LANES_GROUP, 'lane': _lib.SENS_LANES_ONE,
                                    'auto': _lib.SENS_LANES_AUTO}
    # pck_eig_out and its binding name the same members in the same order
    body = re.search(r'typedef struct \{([^}]*)\} pck_eig_out;', re.sub(r'/\*.*?\*/', '', txt, flags=re.S)).group(1)
    members = re.findall(r'\b(\w+)\s*;', body)
    assert members == [f[0] for f in _lib.EigOut._fields_]


# ------------------------------------------------------------------ the Python argument checks
@pytest.fixture(scope='module')
def volcano(inputs):
    import pycatkin_amd as P
    from pycatkin_amd.functions.volcano import set_volcano_energies
    s = P.read_from_input_file(os.path.join(inputs, 'COOxVolcano', 'input.json'))
    set_volcano_energies(s)
    return s


DESC0 = {'ECO': -1.0, 'EO': -1.0}


@pytest.mark.parametrize('bad', ['lanes', 'Lane', '', None, 1])
def test_eig_kernel_value_error(volcano, bad):
    """Raised before anything touches a device."""
    with pytest.raises(ValueError, match='eig_kernel'):
        volcano.stability_at(np.full((4, 1), 0.25), T=[600.0], desc=DESC0, eig_kernel=bad)
    with pytest.raises(ValueError, match='eig_kernel'):
        volcano.stability_batch(T=[600.0], desc=DESC0, eig_kernel=bad)


def test_stability_shape_mismatches(volcano):
    with pytest.raises(ValueError, match='dynamic species'):
        volcano.stability_at(np.full((3, 2), 0.25), T=[600.0, 600.0], desc=DESC0)
    with pytest.raises(ValueError, match='status_in'):
        volcano.stability_at(np.full((4, 2), 0.25), T=[600.0, 600.0], desc=DESC0, status_in=[0, 0, 0])
    R = len(volcano.plan().reactions)
    with pytest.raises(ValueError, match='kf, kr'):
        volcano.stability_at(np.full((4, 2), 0.25), T=[600.0, 600.0], desc=DESC0, k=(np.ones((R, 1)), np.ones((R, 2))))
    with pytest.raises(ValueError, match='steady'):
        volcano.stability_batch(T=[600.0], desc=DESC0, steady=False)


@pytest.mark.parametrize('bad', ['gpu', 'Host', '', None, 0])
def test_eig_value_error(bad):
    """An unknown eig is refused first: no solver, system or device is looked at."""
    from pycatkin_amd.classes.solver import SteadyStateSolver
    from pycatkin_amd.functions.analysis import solve_descriptor_grid
    with pytest.raises(ValueError, match='eig must be'):
        SteadyStateSolver.test_convergence_batch(None, np.zeros((2, 1)), eig=bad)
    with pytest.raises(ValueError, match='eig must be'):
        SteadyStateSolver.solve_ode_batch(None, T=[500.0], eig=bad)
    with pytest.raises(ValueError, match='eig must be'):
        solve_descriptor_grid(None, [0.0], [0.0], eig=bad)


def test_host_is_the_default():
    from pycatkin_amd.classes.solver import SteadyStateSolver
    from pycatkin_amd.functions.analysis import solve_descriptor_grid
    for f in (SteadyStateSolver.test_convergence_batch, SteadyStateSolver.solve_ode_batch, solve_descriptor_grid):
        assert inspect.signature(f).parameters['eig'].default == 'host', f
    from pycatkin_amd.classes.system import System
    p = inspect.signature(System.stability_at).parameters
    assert p['reduce'].default is True and p['eig_kernel'].default == 'auto' and p['spectrum'].default is False


# ------------------------------------------------------------------ the fixture
def test_fixture_cases():
    for ns in (1, 2, 3, 4, 8, 9, 16, 17, 32, 33, 64):
        assert sum(n.startswith('rand%d_' % ns) for n in NAMES) >= 2, ns
    for n in ('zero4', 'diag5', 'triu6', 'rot3', 'rot9', 'comp_real', 'comp_cplx'):
        assert n in NAMES
    for eco, eo in VOLCANO:
        assert 'volcano_%g_%g_full' % (eco, eo) in NAMES and 'volcano_%g_%g_red' % (eco, eo) in NAMES
    for T in (450, 650):
        assert 'dmtm_%d_10000_full' % T in NAMES and 'dmtm_%d_10000_red' % T in NAMES
    assert sum(n.startswith('ch4_') for n in NAMES) == 8
    assert np.array_equal([float(case('ch4_%d_full' % k)['T']) for k in range(8)],
                          np.load(os.path.join(HERE, 'golden', 'ch4_fixture.npz'))['T'])


@pytest.mark.parametrize('name', NAMES)
def test_fixture_matrix_is_consistent(name):
    """The spectrum is that of the matrix (trace and count), the scale is
    ns eps ||B||_F of scipy's balanced matrix, and numpy stays within 10 x
    scale of the exact spectrum: a bound of 10 x scale tests something."""
    from scipy.linalg import matrix_balance
    c = case(name)
    A, w = c['A'], c['w']
    ns = A.shape[0]
    assert A.shape == (ns, ns) and w.shape == (ns,)
    B = matrix_balance(A, permute=False)[0]
    sc = ns * np.finfo(float).eps * np.linalg.norm(B)
    assert abs(sc - float(c['scale'])) <= 1e-14 * sc
    assert float(c['np_ratio']) <= 10.0
    assert abs(w.sum().real - np.trace(A)) <= 4 * ns * np.finfo(float).eps * max(np.abs(np.diag(A)).sum(), np.abs(w).sum())
    # conjugate pairs (a real eigenvalue keeps the 400-bit run's imaginary dust, ~1e-120)
    assert abs(w.imag.sum()) <= 1e-15 * np.abs(w).sum()
    d = np.abs(np.linalg.eigvals(A)[:, None] - w[None, :])
    assert max(d.min(axis=0).max(), d.min(axis=1).max()) <= 10.0 * sc


@pytest.mark.parametrize('eco,eo', VOLCANO)
def test_reduced_volcano_spectrum_has_no_structural_zero(eco, eo):
    """The full Jacobian has an eigenvalue within scale of 0 at every point: the
    site-conservation law's structural zero (|w| <= 4e-9 against a scale of up
    to 4e3).  The reduced spectrum has exactly one eigenvalue fewer within
    scale of 0, and none at all at the four points the generator marks
    `stable`.  At (0.5, 0.5) and (0.5, -2.5) a genuine eigenvalue (-2.5e3 and
    -2.1e-4) is itself smaller than scale (3.0e3 and 1.4e2) in the full and in
    the reduced matrix: those two points are not decidable in fp64."""
    full, red = case('volcano_%g_%g_full' % (eco, eo)), case('volcano_%g_%g_red' % (eco, eo))
    nf = int((np.abs(full['w']) <= float(full['scale'])).sum())
    nr = int((np.abs(red['w']) <= float(red['scale'])).sum())
    assert nf >= 1 and np.abs(full['w']).min() <= 4e-9
    assert nr == nf - 1
    assert red['A'].shape == (3, 3) and len(red['cons_piv']) == 1
    if bool(red['stable']):
        assert nr == 0 and red['w'].real.max() < -10.0 * float(red['scale'])
    assert bool(red['stable']) == ((eco, eo) not in ((0.5, 0.5), (0.5, -2.5)))


def test_ch4_thresholds_are_decidable():
    """+1e2 and -1e2 are farther than 10 x scale (at most 5.6) from every exact
    re_max (~1e-8) of the CH4 Jacobians; the reference's 1e-2 is inside scale."""
    for k in range(8):
        c = case('ch4_%d_full' % k)
        sc, rm = float(c['scale']), c['w'].real.max()
        assert 0.04 <= sc <= 0.6 and abs(rm) <= 1e-6
        assert abs(rm - 1e2) > 10 * sc and abs(rm + 1e2) > 10 * sc and 1e-2 < sc
