"""Energy: the energy landscape of a reaction path and its energy-span model,
with the reference's constructor and methods (pycatkin/classes/energy.py).

The reference evaluates one (T, p) at a time in Python: every state's free
energy, then a TS x intermediate matrix of exponentials.  Here the entries'
energies are LinearForms (pycatkin_amd/energy.py), compiled once into an
energy-only device plan, and pck_energy_span runs the landscape and the span
model for a whole batch of conditions in one launch (evaluate_batch).
"""
from __future__ import annotations

import warnings

import numpy as np

from ..constants.physical_constants import eVtokcal, eVtokJ, kcaltoJ
from ..energy import as_form


def _form_key(f):
    """The content of a LinearForm: what a compiled plan depends on."""
    return (tuple(sorted((k, v) for k, v in f.terms.items() if v != 0.0)),
            tuple(sorted((cid, _form_key(inner)) for cid, inner in f.clamps.items())))


class Energy:
    """Mirror of pycatkin.classes.energy.Energy (energy.py:10-326)."""

    def __init__(self, name='landscape', minima=None, labels=None, path_to_pickle=None):
        if path_to_pickle:
            raise NotImplementedError('pickled energy landscapes are not loaded (no unpickling of external files)')
        self.name = name
        self.minima = minima
        if labels is not None:
            self.labels = labels
        else:
            self.labels = [i[0].name for i in minima]
        self.energy_landscape = None
        if self.minima is None:
            print('No states loaded.')
        if self.labels is not None:
            assert (len(self.labels) == len(self.minima))
        self._plan = None

    # -- symbolic landscape -----------------------------------------------------
    def is_ts(self):
        """energy.py:59: an entry is a TS when any of its states is."""
        return [1 if True in [s.state_type == 'TS' for s in entry] else 0 for entry in self.minima]

    def landscape_forms(self):
        """{'free': [...], 'electronic': [...]}: every entry's energy relative to
        entry 0 as a LinearForm (energy.py:52-58).  A state present in both
        entries cancels here, symbolically, so its energy never enters the
        difference.  'electronic' sums Gelec alone: an energy modifier
        (add_to_energy) acts on the free energies only, as in the reference."""
        out = {}
        for etype, get in (('free', lambda s: s.free_form()), ('electronic', lambda s: s.elec_form())):
            sums = [sum((get(s) for s in entry), as_form(0.0)) for entry in self.minima]
            out[etype] = [f - sums[0] for f in sums]
        return out

    def _device(self):
        """(network, {etype: registers}, descriptor names) of the current forms:
        one plan holds both etypes (2N registers) and is rebuilt whenever a form
        changes (a new energy modifier, a mutated user energy)."""
        from ..engine import DeviceNetwork
        from ..network import compile_forms
        forms = self.landscape_forms()
        flat = forms['free'] + forms['electronic']
        key = tuple(_form_key(f) for f in flat)
        if self._plan is None or self._plan[0] != key:
            states = {s.name: s for entry in self.minima for s in entry}
            ip, dp, regs, dnames = compile_forms(flat, states)
            n = len(self.minima)
            self._plan = (key, DeviceNetwork(ip, dp), {'free': regs[:n], 'electronic': regs[n:]}, list(dnames))
        return self._plan[1:]

    @staticmethod
    def _descriptors(dnames, desc, n, T):
        if not dnames:
            return None
        from ..energy import TKEYED
        given = [k for k in dnames if not k.startswith('@T:')]
        if given and (desc is None or any(k not in desc for k in given)):
            raise ValueError('landscape energies depend on descriptors %s; pass desc=' % given)
        Tn = np.broadcast_to(np.asarray(T, float).ravel(), (n,))
        return np.stack([np.array([TKEYED[k][float(t)] for t in Tn]) if k.startswith('@T:')
                         else np.broadcast_to(np.asarray(desc[k], float).ravel(), (n,)) for k in dnames])

    # -- batched entry ------------------------------------------------------------
    def evaluate_batch(self, T=None, p=None, desc=None, etype='free', to_numpy=True):
        """The energy-span model for a batch of conditions in one launch.
        T, p: scalars or arrays of one length n (scalars broadcast); None takes
        the (T, p) of the stored landscape.  desc: {name: scalar or array} for
        forms that depend on Descriptors.  Returns a dict: tof (1/s), Espan
        (eV), Eapp (kJ/mol), dGrxn (eV), iTDTS, iTDI (landscape indices; -1
        where an energy is not finite) [n]; xTDTS [nTi, n], xTDI [nIj-1, n];
        lTi, lIj (their labels); energies [N, n] (eV, relative to entry 0)."""
        if etype not in ('free', 'electronic'):
            raise KeyError(etype)
        if (T is None or p is None) and self.energy_landscape is None:
            raise ValueError('evaluate_batch needs T and p (no landscape has been constructed yet)')
        T = self.energy_landscape['T'] if T is None else T
        p = self.energy_landscape['p'] if p is None else p
        net, regs, dnames = self._device()
        sizes = [int(np.size(x)) for x in [T, p] + list((desc or {}).values()) if np.ndim(x) > 0]
        n = max(sizes) if sizes else 1
        d = self._descriptors(dnames, desc, n, T)
        ts = self.is_ts()
        r = net.energy_span(n, T, p, (regs[etype], ts), d)
        out = dict(tof=r['tof'], Espan=r['espan'], Eapp=r['eapp'], dGrxn=r['dgrxn'], iTDTS=r['i_tdts'],
                   iTDI=r['i_tdi'], xTDTS=r['x_ts'], xTDI=r['x_int'], energies=r['energy'])
        if to_numpy:
            out = {k: v.cpu().numpy() for k, v in out.items()}
        N = len(ts)
        out['lTi'] = [self.labels[k] for k in range(N) if ts[k] == 1]
        out['lIj'] = [self.labels[k] for k in range(N) if ts[k] == 0][1:-1]
        return out

    # -- the reference's methods ----------------------------------------------------
    def construct_energy_landscape(self, T, p, verbose=False):
        """energy.py:39-60: free and electronic energies of every entry relative
        to the first, from one device call."""
        net, regs, dnames = self._device()
        d = self._descriptors(dnames, None, 1, T)
        vals = net.energies(1, float(T), float(p), None if d is None else d[:, 0]).cpu().numpy()[:, 0]
        ts = self.is_ts()
        self.energy_landscape = dict({'free': {}, 'electronic': {}, 'isTS': {}, 'T': T, 'p': p})
        for sind in range(len(self.minima)):
            for etype in ('free', 'electronic'):
                self.energy_landscape[etype][sind] = float(vals[regs[etype][sind]] - vals[regs[etype][0]])
            self.energy_landscape['isTS'][sind] = ts[sind]

    def draw_energy_landscape(self, T, p, etype='free', eunits='eV', legend_location='upper right',
                              verbose=False, path=None, show_labels=False, figtitle=None):
        """energy.py:62-156.  Plotting is out of scope: warns and skips."""
        warnings.warn('Energy.draw_energy_landscape: plotting is not part of pycatkin_amd; the figure is skipped '
                      '(presets.save_pes_energies writes the energies)', stacklevel=2)

    def draw_energy_landscape_simple(self, T, p, fig, ax, linecolor='k', etype='free', eunits='eV',
                                     verbose=False, show_labels=False):
        """energy.py:158-236.  Plotting is out of scope: warns and returns the axes untouched."""
        warnings.warn('Energy.draw_energy_landscape_simple: plotting is not part of pycatkin_amd; '
                      'the figure is skipped', stacklevel=2)
        return fig, ax

    def evaluate_energy_span_model(self, T, p, etype='free', verbose=False, opath=None):
        """energy.py:238-318 for one condition.  Returns
        (tof, Espan, TDTS, TDI, num_i, num_j, lTi, lIj) and prints the reference's lines."""
        if self.energy_landscape is None:
            self.construct_energy_landscape(T=T, p=p, verbose=verbose)
        elif self.energy_landscape['T'] != T or self.energy_landscape['p'] != p:
            self.construct_energy_landscape(T=T, p=p, verbose=verbose)
        r = self.evaluate_batch(T=float(T), p=float(p), etype=etype)
        return self._report(r, 0, T, opath)

    def _report(self, r, c, T, opath=None):
        """The reference's return tuple, printed block (energy.py:301-310) and
        opath file (:312-316) for condition c of an evaluate_batch result."""
        if r['iTDTS'][c] < 0:
            raise ValueError('energy landscape %s has a non-finite energy at T = %s' % (self.name, T))
        tof, Espan, Eapp = r['tof'][c], float(r['Espan'][c]), r['Eapp'][c]
        drxn = float(r['dGrxn'][c]) * eVtokJ * 1.0e3
        TDTS, TDI = self.labels[int(r['iTDTS'][c])], self.labels[int(r['iTDI'][c])]
        num_i = [v for v in r['xTDTS'][:, c]]
        num_j = [v for v in r['xTDI'][:, c]]
        print('Energy span model results (%1.0f K): ' % T)
        print('* TOF = % .3g 1/s' % tof)
        print('* Espan = %.3g eV = %.3g kcal/mol = %.3g kJ/mol' % (Espan, Espan * eVtokcal, Espan * eVtokJ))
        print('* TDTS is %s.' % TDTS)
        print('* TDI is %s.' % TDI)
        print('* dGrxn = %.3g eV = %.3g kcal/mol = %.3g kJ/mol' % (drxn * 1.0e-3 / eVtokJ, drxn / kcaltoJ, drxn * 1.0e-3))
        print('* Eapp = %.3g eV = %.3g kcal/mol = %.3g kJ/mol' % (Eapp / eVtokJ, Eapp * 1.0e3 / kcaltoJ, Eapp))
        if opath is not None:
            with open(opath, 'w') as tfile:
                tfile.write(str(tof) + '\n')
                tfile.write(', '.join([str(i) for i in num_i] + ['\n']))
                tfile.write(', '.join([str(j) for j in num_j] + ['\n']))
        return tof, Espan, TDTS, TDI, num_i, num_j, list(r['lTi']), list(r['lIj'])

    def save_pickle(self, path=None):
        """energy.py:320-326.  Pickling is out of scope."""
        raise NotImplementedError('energy landscapes are not pickled; presets.save_pes_energies writes the energies')
