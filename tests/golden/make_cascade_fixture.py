"""Reactor-cascade goldens from the oracle alone (oracle/mk_oracle.py; the
reference tree is not needed): the COOxReactor Pd111 bed as `cells` CSTR cells
in series, the tanks-in-series model of System.solve_cascade_batch.

Grid: T = linspace(423, 623, 17) K, cells in (1, 2, 8), both start modes.
Each cell is a ClassicModel on a copy of the spec whose residence_time, volume
and catalyst_area are the bed's divided by `cells`, with inflow_state set to
the previous cell's gas (cell 0: the input file's), solved by
oracle.steady_rule at its defaults.  start 'system': every cell's transient
starts from the input file's start state; 'upstream': from the final state of
the cell before it.

Stored per (cells, start): y_c<cells>_<start> [17, cells, n_species] (every
cell's full state, species in `species` order; NaN from the first cell without
an oracle answer on), regular_c<cells>_<start> [17, cells] (the cell's answer
is a reached root), ref_ok_c<cells>_<start> [17] (False where steady_rule
returned None for a cell: both scipy integrators exceeded the rule's budget).

Output: tests/golden/cascade_fixture.npz.
Run:    python tests/golden/make_cascade_fixture.py   (about a minute on 8 cores)
"""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import mk_oracle as O  # noqa: E402

INPUT = os.path.join(HERE, 'inputs', 'COOxReactor', 'input_Pd111.json')
TEMPS = np.linspace(423.0, 623.0, 17)
CELLS = (1, 2, 8)
STARTS = ('system', 'upstream')


def cell_spec(spec, cells):
    """The spec of one cell: 1/cells of the bed's residence time, volume and area."""
    s = copy.deepcopy(spec)
    for k in ('residence_time', 'volume', 'catalyst_area'):
        s['reactor'][k] = spec['reactor'][k] / cells
    return s


def case(spec, T, cells, start):
    """(y [cells, n_species], regular [cells], ref_ok) of one bed."""
    cs = cell_spec(spec, cells)
    inflow, prev = None, None
    y, regular, ok = None, np.zeros(cells, bool), True
    for c in range(cells):
        m = O.ClassicModel(cs, T=float(T), inflow_state=inflow)
        if y is None:
            y = np.full((cells, len(m.snames)), np.nan)
        if start == 'upstream' and prev is not None:
            m.y0 = prev.copy()
        r = O.steady_rule(m)
        if r is None:
            ok = False
            break
        y[c], regular[c] = r['y'], r['regular']
        prev = np.asarray(r['y'], float)
        inflow = {m.snames[i]: float(prev[i]) for i in m.gas_idx}
    return y, regular, ok


def _job(args):
    T, cells, start = args
    return case(O.load_spec(INPUT), T, cells, start)


def main():
    from multiprocessing import Pool
    spec = O.load_spec(INPUT)
    jobs = [(T, cells, start) for cells in CELLS for start in STARTS for T in TEMPS]
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        res = pool.map(_job, jobs, chunksize=1)
    out = dict(T=TEMPS, cells=np.array(CELLS), species=np.array(O.ClassicModel(spec, T=TEMPS[0]).snames))
    it = iter(res)
    for cells in CELLS:
        for start in STARTS:
            rows = [next(it) for _ in TEMPS]
            tag = 'c%d_%s' % (cells, start)
            out['y_' + tag] = np.stack([r[0] for r in rows])
            out['regular_' + tag] = np.stack([r[1] for r in rows])
            out['ref_ok_' + tag] = np.array([r[2] for r in rows])
            print(tag, 'ref_ok %d / %d' % (out['ref_ok_' + tag].sum(), len(TEMPS)),
                  'regular cells %d / %d' % (out['regular_' + tag].sum(), out['regular_' + tag].size))
    np.savez_compressed(os.path.join(HERE, 'cascade_fixture.npz'), **out)


if __name__ == '__main__':
    main()
