"""The one-lane multi-objective DRC kernel (csrc/mk_sens_multi_lane.h), the
part that needs no device: the fixture tests/golden/drc_multi_lane_fixture.npz
(make_drc_multi_lane_fixture.py), the new C-ABI symbol, the argument check of
the Python calls, and the kernel's metadata in the built library."""
import ctypes
import os
import re

import numpy as np
import pytest

from pycatkin_amd import _lib

import test_capi as CAPI

HERE = os.path.dirname(os.path.abspath(__file__))
LX = dict(np.load(os.path.join(HERE, 'golden', 'lane_sens_fixture.npz')))
MX = dict(np.load(os.path.join(HERE, 'golden', 'drc_multi_lane_fixture.npz')))
NAMES = [str(x) for x in MX['names']]
TOL_104 = 1.0e-11


def mcase(i):
    pre = 'm%d_' % i
    c = {k[len(pre):]: v for k, v in MX.items() if k.startswith(pre)}
    c['name'] = NAMES[i]
    pre = 'n%d_' % int(c['src'])
    c['s'] = {k[len(pre):]: v for k, v in LX.items() if k.startswith(pre)}
    return c


# ------------------------------------------------------------------ the fixture
def test_fixture_cases():
    """The cases of lane_sens_fixture.npz, by name and index; K > 8 on l8_0."""
    assert NAMES == ['l3_0', 'l3_1', 'l7_0', 'l7_1', 'l8_0', 'l8_1', 'pin_0']
    lnames = [str(x) for x in LX['names']]
    assert [lnames[int(mcase(i)['src'])] for i in range(len(NAMES))] == NAMES
    assert [len(mcase(i)['s']['dyn']) for i in range(len(NAMES))] == [3, 3, 7, 7, 8, 8, 5]
    assert len(mcase(NAMES.index('l8_0'))['labels']) > 8


@pytest.mark.parametrize('i', range(len(NAMES)), ids=NAMES)
def test_fixture_case_is_consistent(i):
    """Shapes; no empty objective; the 104-bit run within 1e-11 (1 + |ref|) of
    the reference for every stored objective; at most one coverage objective
    of a non-zero species missing and the TOF objective present (l* cases);
    what was turned down is recorded by label."""
    c = mcase(i)
    s = c['s']
    R, NS, K = len(s['rnames']), len(s['dyn']), len(c['labels'])
    labels, dropped = [str(x) for x in c['labels']], [str(x) for x in c['dropped']]
    assert c['wr'].shape == (K, R) and c['wy'].shape == (K, NS)
    assert c['val_ref'].shape == (K,) and c['xi_ref'].shape == c['xi_104'].shape == (K, R)
    assert np.all(np.isfinite(c['xi_ref'])) and np.all(np.isfinite(c['val_ref'])) and np.all(c['val_ref'] != 0.0)
    assert all(c['wr'][m].any() or c['wy'][m].any() for m in range(K))
    assert len(set(labels)) == K and not set(labels) & set(dropped)
    d = np.abs(c['xi_104'] - c['xi_ref']) / (1.0 + np.abs(c['xi_ref']))
    print('%s: K %d, |xi_104 - xi_ref| / (1 + |xi_ref|) <= %.1e, turned down %s' % (c['name'], K, d.max(), dropped))
    assert np.all(d <= TOL_104)
    # the objectives: the TOF terms, the rate mix, the coverages of the non-zero species
    dyn = [str(x) for x in s['dyn']]
    nonzero = ['[%s]' % dyn[a] for a in range(NS) if s['y'][a] != 0.0]
    assert set(labels) | set(dropped) >= set(nonzero) | {'tof', 'mix'}
    for lb in nonzero:
        if lb in labels:
            m = labels.index(lb)
            assert not c['wr'][m].any() and np.count_nonzero(c['wy'][m]) == 1 and c['wy'][m][dyn.index(lb[1:-1])] == 1.0
            assert c['val_ref'][m] == s['y'][dyn.index(lb[1:-1])]
    if c['name'].startswith('l'):
        assert 'tof' in labels
        assert sum(1 for lb in nonzero if lb not in labels) <= 1
    if 'tof' in labels:
        m = labels.index('tof')
        rn = [str(x) for x in s['rnames']]
        want = np.zeros(R)
        for t in s['tof_terms']:
            want[rn.index(str(t))] += 1.0
        np.testing.assert_array_equal(c['wr'][m], want)
        assert not c['wy'][m].any()
        # the single-objective fixture's reference is the same number
        assert np.all(np.abs(c['xi_ref'][m] - s['xi_ref']) <= 1e-14 * (1.0 + np.abs(s['xi_ref'])))


# ------------------------------------------------------------------ the C-ABI
def test_new_symbol_is_declared_and_bound():
    assert 'pck_network_set_multi_lanes' in CAPI.declared_symbols()
    assert 'pck_network_set_multi_lanes' in _lib.EXPORTED
    txt = open(CAPI.HDR).read()
    assert re.search(r'int pck_network_set_multi_lanes\(pck_network\* net, int mode\);', txt)
    assert re.search(r'#define PCK_ABI_VERSION 10\b', txt) and _lib.ABI_VERSION == 10


@pytest.mark.skipif(not os.path.isfile(_lib.LIB_PATH), reason='library not built (run __graft_entry__.build())')
def test_new_symbol_ctypes_signature():
    lib = _lib.load()
    assert lib.pck_network_set_multi_lanes.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert lib.pck_network_set_multi_lanes.restype is ctypes.c_int
    # the argument check that needs no network
    assert lib.pck_network_set_multi_lanes(None, 0) == _lib.E_ARG
    assert lib.pck_network_set_multi_lanes(None, 1) == _lib.E_ARG


# ------------------------------------------------------------------ the Python argument check
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
    s, Y = volcano, np.full((4, 1), 0.25)
    with pytest.raises(ValueError, match='adjoint_kernel'):
        s.drc_objectives_at([('CO_ox',)], Y, T=[600.0], desc=DESC0, adjoint_kernel=bad)
    with pytest.raises(ValueError, match='adjoint_kernel'):
        s.drc_objectives_batch([('CO_ox',)], T=[600.0], desc=DESC0, adjoint_kernel=bad)
    for kw in (dict(Y=Y), dict()):
        with pytest.raises(ValueError, match='adjoint_kernel'):
            s.selectivity_control_batch(('CO_ox',), ('CO_ads',), T=[600.0], desc=DESC0, adjoint_kernel=bad, **kw)
        with pytest.raises(ValueError, match='adjoint_kernel'):
            s.coverage_control_batch(T=[600.0], desc=DESC0, adjoint_kernel=bad, **kw)


# ------------------------------------------------------------------ the kernel in the built library
@pytest.mark.skipif(not (os.path.isfile(_lib.LIB_PATH) and os.path.isfile(CAPI.LLVM + '/llvm-readelf')),
                    reason='library or ROCm LLVM tools absent')
def test_lane_multi_kernel_exists_and_uses_no_scratch(tmp_path):
    """Exactly one k_lane_multi_adjoint in the library's gfx950 code object,
    with private_segment_fixed_size == 0: its run-time indexed arrays are in
    LDS, none went to scratch.  Its name hides from the counts of the other
    adjoint families."""
    meta = CAPI._kernel_metadata(_lib.LIB_PATH, tmp_path)
    hits = {k: v for k, v in meta.items() if 'k_lane_multi_adjoint' in k}
    assert len(hits) == 1, sorted(hits)
    (name, (vgpr, agpr, scratch)), = hits.items()
    print('%s: %d VGPRs, %d AGPRs, scratch %d' % (name, vgpr, agpr, scratch))
    assert scratch == 0, name
    assert vgpr + agpr <= 168, name                # 3 waves per SIMD at the least; LDS sets the occupancy
    for stem in ('k_multi_adjoint', 'k_drc_adjoint', 'k_sens_adjoint', 'k_lane_drc_adjoint', 'k_lane_sens_adjoint'):
        assert stem not in name
