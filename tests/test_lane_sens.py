"""The one-lane adjoint kernels (csrc/mk_sens_lane.h) and the descriptor
sensitivities, the part that needs no device: the fixture
tests/golden/lane_sens_fixture.npz (make_lane_sens_fixture.py), the two new
C-ABI symbols, the argument checks of the new Python calls, and the kernels'
metadata in the built library."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from pycatkin_amd import _lib

import test_capi as CAPI

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, 'golden'))
LX = dict(np.load(os.path.join(HERE, 'golden', 'lane_sens_fixture.npz')))
NAMES = [str(x) for x in LX['names']]
DNAMES = [str(x) for x in LX['dnames']]
KEYS = ('sf', 'sr', 'xi', 'order', 'order_in', 'dir')


def ncase(k):
    pre = 'n%d_' % k
    c = {key[len(pre):]: v for key, v in LX.items() if key.startswith(pre)}
    c['name'] = NAMES[k]
    return c


def dcase(k):
    pre = 'd%d_' % k
    c = {key[len(pre):]: v for key, v in LX.items() if key.startswith(pre)}
    c['name'] = DNAMES[k]
    return c


# ------------------------------------------------------------------ the fixture
def test_fixture_cases():
    """NS = 3, 7 and 8 (the kernels' limit), two roots each, and the pinned state."""
    assert NAMES == ['l3_0', 'l3_1', 'l7_0', 'l7_1', 'l8_0', 'l8_1', 'pin_0']
    assert [len(ncase(k)['dyn']) for k in range(7)] == [3, 3, 7, 7, 8, 8, 5]
    assert _lib.MAX_DYN_LANE == 8
    assert len(DNAMES) == 3 and all(nm.startswith('volcano_') for nm in DNAMES)


@pytest.mark.parametrize('k', range(len(NAMES)), ids=NAMES)
def test_fixture_new_cases_are_consistent(k):
    """Shapes; sf + sr = xi; the 104-bit run within the guard's err of the
    reference (beyond an ulp of the result); the perturbed run finite; every
    species row of the network has several CSR entries."""
    c = ncase(k)
    R, NS = len(c['rnames']), len(c['dyn'])
    assert c['kf'].shape == c['kr'].shape == (R,) and c['y'].shape == (NS,) and c['unreach'].shape == (NS,)
    assert c['dir_a'].shape == c['dir_c'].shape == (R,) and c['dir_ref'].shape == (1,)
    for key in KEYS:
        ref, lo, pt = c[key + '_ref'], c[key + '_104'], c[key + '_pert']
        assert ref.shape == lo.shape == pt.shape and np.all(np.isfinite(ref)) and np.all(np.isfinite(pt)), key
        assert np.all(np.abs(lo - ref) <= float(c['err']) + 2.0 ** -51 * np.abs(ref)), key
    assert np.all(np.abs(c['sf_ref'] + c['sr_ref'] - c['xi_ref']) <= 1e-15 * (np.abs(c['sf_ref']) + np.abs(c['sr_ref'])))
    assert np.isfinite(c['tof_ref']) and float(c['tof_ref']) != 0.0 and float(c['err']) <= 1e-9
    from make_lane_sens_fixture import NETS, lane_net
    net = lane_net(str(c['net']))
    assert NETS[str(c['net'])][0] == NS and len(net['reactions']) == R
    if not c['name'].startswith('pin'):
        assert not c['unreach'].any()
        for sp in net['adsorbates'] + ['s']:
            assert sum(1 for _, a, b in net['reactions'] if sp in a or sp in b) >= 2, sp


def test_fixture_pinned_state():
    """The leaf and its chain parent are exactly 0, the leaf alone is pinned."""
    from make_lane_sens_fixture import lane_net, pinned_pair
    c = ncase(NAMES.index('pin_0'))
    leaf, parent = pinned_pair(lane_net('pin'))
    dyn = [str(x) for x in c['dyn']]
    assert c['y'][dyn.index(leaf)] == 0.0 and c['y'][dyn.index(parent)] == 0.0
    assert c['unreach'].tolist() == [nm == leaf for nm in dyn]
    assert np.count_nonzero(c['y']) == len(dyn) - 2


@pytest.mark.parametrize('k', range(len(DNAMES)), ids=DNAMES)
def test_fixture_descriptor_cases_are_consistent(k):
    """No stored case straddles an energy clamp (the doubled step gives the same
    derivative to 1e-9); the 104-bit run and the oracle's own finite difference
    are near the reference."""
    c = dcase(k)
    R = len(c['rnames'])
    assert [str(x) for x in c['ddesc_names']] == ['ECO', 'EO']
    assert c['ddesc_a'].shape == c['ddesc_c'].shape == (2, R)
    ref = c['ddesc_ref']
    assert ref.shape == (2,) and np.all(np.isfinite(ref)) and np.all(np.abs(ref) > 1.0)
    assert np.all(np.abs(c['ddesc_2h'] - ref) <= 1e-9 * np.abs(ref))
    assert np.all(np.abs(c['ddesc_104'] - ref) <= 1e-12 * np.abs(ref))
    assert np.all(np.abs(c['ddesc_pert'] - ref) <= 1e-4 * np.abs(ref))
    assert np.all(np.abs(c['ddesc_fd'] - ref) <= 1e-4 * np.abs(ref))
    # E_CO enters CO adsorption, E_O oxygen adsorption: each direction moves some rate constant
    assert np.any(c['ddesc_a'][0] != 0.0) or np.any(c['ddesc_c'][0] != 0.0)
    assert np.any(c['ddesc_a'][1] != 0.0) or np.any(c['ddesc_c'][1] != 0.0)


def test_two_volcano_cases_are_the_sensitivity_fixtures():
    """Their states and rate constants are those of drc_adjoint_fixture.npz."""
    fx = dict(np.load(os.path.join(HERE, 'golden', 'drc_adjoint_fixture.npz')))
    names = [str(x) for x in fx['names']]
    shared = [nm for nm in DNAMES if nm in names]
    assert shared == ['volcano_-1_-1', 'volcano_-1.3_-1.1']
    for nm in shared:
        c, pre = dcase(DNAMES.index(nm)), 'c%d_' % names.index(nm)
        for key in ('y', 'kf', 'kr', 'T', 'p', 'desc'):
            np.testing.assert_array_equal(c[key], fx[pre + key], err_msg=key)


# ------------------------------------------------------------------ the C-ABI
def test_new_symbols_are_declared_and_bound():
    assert 'pck_network_set_sens_lanes' in CAPI.declared_symbols() and 'pck_network_sens_lanes' in CAPI.declared_symbols()
    assert 'pck_network_set_sens_lanes' in _lib.EXPORTED and 'pck_network_sens_lanes' in _lib.EXPORTED
    txt = open(CAPI.HDR).read()
    assert re.search(r'int pck_network_set_sens_lanes\(pck_network\* net, int mode\);', txt)
    assert re.search(r'int pck_network_sens_lanes\(const pck_network\* net, int32_t\* lanes\);', txt)
    for name, val in (('GROUP', 0), ('ONE', 1), ('AUTO', 2)):
        assert re.search(r'#define PCK_SENS_LANES_%s %d\b' % (name, val), txt)
        assert getattr(_lib, 'SENS_LANES_' + name) == val
    assert _lib.SENS_LANES_MODES == {'group': 0, 'lane': 1, 'auto': 2}
    assert re.search(r'#define PCK_ABI_VERSION 10\b', txt) and _lib.ABI_VERSION == 10


@pytest.mark.skipif(not os.path.isfile(_lib.LIB_PATH), reason='library not built (run __graft_entry__.build())')
def test_new_symbols_ctypes_signatures():
    lib = _lib.load()
    assert lib.pck_network_set_sens_lanes.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert lib.pck_network_sens_lanes.argtypes == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)]
    assert lib.pck_network_set_sens_lanes.restype is ctypes.c_int and lib.pck_network_sens_lanes.restype is ctypes.c_int
    # the argument checks that need no network
    assert lib.pck_network_set_sens_lanes(None, 0) == _lib.E_ARG
    g = ctypes.c_int32(-1)
    assert lib.pck_network_sens_lanes(None, ctypes.byref(g)) == _lib.E_ARG


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
def test_adjoint_kernel_value_error(volcano, bad):
    """Raised before anything touches a device."""
    s, tt, Y = volcano, ('CO_ox',), np.full((4, 1), 0.25)
    with pytest.raises(ValueError, match='adjoint_kernel'):
        s.drc_at(tt, Y, T=[600.0], desc=DESC0, adjoint_kernel=bad)
    with pytest.raises(ValueError, match='adjoint_kernel'):
        s.drc_batch(tt, T=[600.0], desc=DESC0, steady=True, method='analytic', adjoint_kernel=bad)
    with pytest.raises(ValueError, match='adjoint_kernel'):
        s.sensitivity_at(tt, Y, T=[600.0], desc=DESC0, adjoint_kernel=bad)
    with pytest.raises(ValueError, match='adjoint_kernel'):
        s.sensitivity_batch(tt, T=[600.0], desc=DESC0, adjoint_kernel=bad)
    with pytest.raises(ValueError, match='adjoint_kernel'):
        s.descriptor_sensitivity_at(tt, Y, T=[600.0], desc=DESC0, adjoint_kernel=bad)
    with pytest.raises(ValueError, match='adjoint_kernel'):
        s.descriptor_sensitivity_batch(tt, T=[600.0], desc=DESC0, adjoint_kernel=bad)


def test_unknown_descriptor_value_error(volcano):
    s, tt = volcano, ('CO_ox',)
    assert sorted(k for k in s.plan(tt).descriptors if not k.startswith('@T:')) == ['ECO', 'EO']
    with pytest.raises(ValueError, match="unknown descriptor 'EH'"):
        s.descriptor_sensitivity_batch(tt, T=[600.0], desc=DESC0, names=['ECO', 'EH'])
    with pytest.raises(ValueError, match="unknown descriptor 'EH'"):
        s.descriptor_sensitivity_at(tt, np.full((4, 1), 0.25), T=[600.0], desc=DESC0, names=['EH'])
    with pytest.raises(ValueError, match="unknown descriptor 'EH'"):
        s.dlnk_ddesc_batch(names=['EH'], T=[600.0], desc=DESC0)


def test_temperature_keyed_descriptor_value_error(volcano):
    s, tt = volcano, ('CO_ox',)
    with pytest.raises(ValueError, match='temperature-keyed'):
        s.descriptor_sensitivity_batch(tt, T=[600.0], desc=DESC0, names=['@T:CO_ox.dEa_fwd_user'])
    with pytest.raises(ValueError, match='temperature-keyed'):
        s.dlnk_ddesc_batch(names=['@T:x'], T=[600.0], desc=DESC0)


def test_desc_sigma_key_not_requested_value_error(volcano):
    s, tt = volcano, ('CO_ox',)
    with pytest.raises(ValueError, match='desc_sigma'):
        s.descriptor_sensitivity_batch(tt, T=[600.0], desc=DESC0, names=['ECO'], desc_sigma={'ECO': 0.1, 'EO': 0.1})
    with pytest.raises(ValueError, match='desc_sigma'):
        s.descriptor_sensitivity_at(tt, np.full((4, 1), 0.25), T=[600.0], desc=DESC0, desc_sigma={'EH': 0.1})
    with pytest.raises(ValueError, match='steady'):
        s.descriptor_sensitivity_batch(tt, T=[600.0], desc=DESC0, steady=False)


# ------------------------------------------------------------------ the kernels in the built library
@pytest.mark.skipif(not (os.path.isfile(_lib.LIB_PATH) and os.path.isfile(CAPI.LLVM + '/llvm-readelf')),
                    reason='library or ROCm LLVM tools absent')
def test_lane_kernels_exist_and_use_no_scratch(tmp_path):
    """k_lane_drc_adjoint and k_lane_sens_adjoint are in the library's gfx950
    code object with private_segment_fixed_size == 0: their run-time indexed
    arrays are in LDS, none went to scratch."""
    meta = CAPI._kernel_metadata(_lib.LIB_PATH, tmp_path)
    for stem in ('k_lane_drc_adjoint', 'k_lane_sens_adjoint'):
        hits = {k: v for k, v in meta.items() if stem in k}
        assert len(hits) == 1, (stem, sorted(hits))
        (name, (vgpr, agpr, scratch)), = hits.items()
        print('%s: %d VGPRs, %d AGPRs, scratch %d' % (name, vgpr, agpr, scratch))
        assert scratch == 0, name
        assert vgpr + agpr <= 168, name            # 3 waves per SIMD; LDS, not registers, sets the occupancy
