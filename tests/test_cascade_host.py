"""Reactor cascade, host side (no GPU): the PFReactor class, the loader key,
argument validation of System.solve_cascade_batch, the PFReactor guard of the
single-tank calls, and the committed fixture against its script."""
import importlib.util
import json
import os

import numpy as np
import pytest

import pycatkin_amd as P
from pycatkin_amd.constants.physical_constants import bartoPa, kB

HERE = os.path.dirname(os.path.abspath(__file__))
BED = dict(residence_time=4.5, volume=1.8e-7, catalyst_area=3.82e-9)


def pd111(inputs, reactor=None):
    s = P.read_from_input_file(os.path.join(inputs, 'COOxReactor', 'input_Pd111.json'))
    if reactor is not None:
        s.add_reactor(reactor)
        s._plans.clear()
    return s


@pytest.mark.parametrize('cells', [1, 3, 8])
def test_row_coefficients(cells):
    r = P.PFReactor(cells=cells, **BED)
    assert isinstance(r, P.CSTReactor) and r.cells == cells
    assert r.row_coefficients(True) == (1.0, 0.0, 0.0)
    rs0, rsT, fl = r.row_coefficients(False)
    assert rs0 == 0.0
    assert rsT == kB * BED['catalyst_area'] / BED['volume'] / bartoPa      # A/V of a cell is the bed's
    assert fl == cells / BED['residence_time']
    # one cell is the CSTR
    assert P.PFReactor(cells=1, **BED).row_coefficients(False) == P.CSTReactor(**BED).row_coefficients(False)
    # the bed from a flow rate
    assert P.PFReactor(cells=cells, volume=2.0, catalyst_area=1.0, flow_rate=4.0).row_coefficients(False)[2] == cells / 0.5


@pytest.mark.parametrize('cells', [0, -1, 2.5])
def test_cells_must_be_a_positive_integer(cells):
    with pytest.raises(ValueError, match='cells'):
        P.PFReactor(cells=cells, **BED)


def test_plan_carries_the_cell_coefficients(inputs):
    """The compiled plan of a PFReactor system: gas rows dynamic, the flow
    column cells / residence_time."""
    from pycatkin_amd import _lib as L
    a = pd111(inputs, P.PFReactor(cells=8, **BED)).plan(('CO_ox',))
    b = pd111(inputs).plan(('CO_ox',))
    assert a.dyn == b.dyn and a.fix == b.fix == []
    off = int(a.ip[L.I_HDR + L.D_DYN])
    da = np.asarray(a.dp[off: off + 4 * len(a.dyn)]).reshape(-1, 4)
    db = np.asarray(b.dp[off: off + 4 * len(b.dyn)]).reshape(-1, 4)
    np.testing.assert_array_equal(da[:, :3], db[:, :3])
    np.testing.assert_array_equal(da[:, 3], np.where(db[:, 3] != 0.0, 8 / 4.5, 0.0))


def test_loader_parses_pfreactor(inputs, tmp_path):
    src = os.path.join(inputs, 'COOxReactor', 'input_Pd111.json')
    d = json.load(open(src))
    d['reactor'] = {'PFReactor': dict(d['reactor']['CSTReactor'], cells=5)}
    for st in d['states'].values():                  # data paths are relative to the input file
        if 'path' in st:
            st['path'] = os.path.join(os.path.dirname(src), st['path'])
    path = tmp_path / 'input_pfr.json'
    path.write_text(json.dumps(d))
    s = P.read_from_input_file(str(path))
    assert isinstance(s.reactor, P.PFReactor) and s.reactor.cells == 5
    assert s.reactor.residence_time == 4.5
    d['reactor'] = {'TubeReactor': {}}
    path.write_text(json.dumps(d))
    with pytest.raises(TypeError, match='PFReactor'):
        P.read_from_input_file(str(path))


def test_single_tank_calls_refuse_a_pfreactor(inputs):
    s = pd111(inputs, P.PFReactor(cells=4, **BED))
    for call in (lambda: s.solve_batch(T=[500.0]), s.solve_odes, s.find_steady):
        with pytest.raises(ValueError, match='solve_cascade_batch'):
            call()


def test_argument_validation(inputs):
    """Raised before any device work."""
    s = pd111(inputs, P.PFReactor(cells=4, **BED))
    with pytest.raises(ValueError, match='start'):
        s.solve_cascade_batch(T=[500.0], start='downstream')
    with pytest.raises(ValueError, match='method'):
        s.solve_cascade_batch(T=[500.0], method='fast')
    for cells in (0, -3, 2.5, 4097, True):
        with pytest.raises(ValueError, match='cells'):
            s.solve_cascade_batch(cells=cells, T=[500.0])
    with pytest.raises(ValueError, match='cells'):       # the flow rate is one of 4 cells
        s.solve_cascade_batch(cells=8, T=[500.0])
    c = pd111(inputs)
    with pytest.raises(ValueError, match='cells'):       # a CSTReactor has no count of its own
        c.solve_cascade_batch(T=[500.0])
    from pycatkin_amd.functions.volcano import set_volcano_energies
    v = P.read_from_input_file(os.path.join(inputs, 'COOxVolcano', 'input.json'))
    set_volcano_energies(v)
    with pytest.raises(ValueError, match='flow'):                 # gas held fixed: identical cells
        v.solve_cascade_batch(cells=2, T=[500.0])


def test_committed_fixture_is_the_scripts():
    """One case regenerated (2 cells, 'upstream', 423 K) and compared."""
    spec = importlib.util.spec_from_file_location('make_cascade_fixture',
                                                  os.path.join(HERE, 'golden', 'make_cascade_fixture.py'))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    f = np.load(os.path.join(HERE, 'golden', 'cascade_fixture.npz'))
    np.testing.assert_array_equal(f['T'], M.TEMPS)
    assert tuple(f['cells']) == M.CELLS
    for cells in M.CELLS:
        for start in M.STARTS:
            assert f['y_c%d_%s' % (cells, start)].shape == (17, cells, len(f['species']))
            # the issue's count: an oracle answer on at least 33 of the 34 (T, cells in (2, 8)) cases
            assert f['ref_ok_c%d_%s' % (cells, start)].sum() >= (17 if cells != 2 else 16)
    from oracle import mk_oracle as O
    y, regular, ok = M.case(O.load_spec(M.INPUT), M.TEMPS[0], 2, 'upstream')
    assert ok and f['ref_ok_c2_upstream'][0]
    np.testing.assert_allclose(y, f['y_c2_upstream'][0], rtol=1e-12, atol=1e-300)
    np.testing.assert_array_equal(regular, f['regular_c2_upstream'][0])
    # not a vacuous fixture: at 535.5 K the 2-cell bed is ignited, the 8-cell bed CO-poisoned
    co = list(f['species']).index('CO')
    assert 1.0 - f['y_c2_system'][9, -1, co] / 0.02 > 0.5
    assert 1.0 - f['y_c8_system'][9, -1, co] / 0.02 < 1e-6
