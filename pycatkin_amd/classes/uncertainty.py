"""Uncertainty: the reference's energy-noise ensemble (pycatkin/classes/uncertainty.py)
as one batched device solve.

The reference deep-copies the system `nruns` times, adds a correlated random
modifier to every adsorbate and transition-state energy of each copy, runs
solve_odes on each and reduces a property over the runs.  Here the modifiers
are per-condition descriptors of ONE network ('@unc:ads' for the adsorbates'
shared value, '@unc:ts:<name>' per transition state): the whole ensemble --
every base condition times every run -- is one solve_batch launch,
pck_ensemble_noise draws the noise on the device and pck_ensemble_stats
reduces over the runs there (DESIGN.md "Uncertainty ensemble").
"""
from __future__ import annotations

import copy

import numpy as np

from ..energy import Descriptor
from .reaction import ReactionDerivedReaction

ADS = '@unc:ads'
TS = '@unc:ts:'
EXTRA = '@unc:state:'


class Uncertainty:
    """Mirror of pycatkin.classes.uncertainty.Uncertainty (uncertainty.py:6-125)."""

    def __init__(self, sys=None, mu=0.0, sigma=0.01, nruns=1):
        self.sys = copy.deepcopy(sys)
        self.mu = mu
        self.sigma = sigma
        self.nruns = nruns
        self.noisy_sys = None
        self.state_noises = None
        self._ens = None

    # -- the reference's draws (global np.random, uncertainty.py:23-65) ----------
    def get_noise(self, noise_type='white'):
        """uncertainty.py:23-33"""
        if noise_type == 'white':
            return np.random.normal(loc=self.mu, scale=self.sigma, size=None)
        elif noise_type == 'uniform':
            return np.random.uniform()
        return 0.0

    @staticmethod
    def _walk(system):
        """(intermediates, transition states) of every reaction in order; a
        ReactionDerivedReaction contributes its base reaction's states."""
        for rx in system.reactions.values():
            src = rx.base_reaction if isinstance(rx, ReactionDerivedReaction) else rx
            yield list(src.reactants) + list(src.products), list(src.TS) if src.TS else []

    def get_correlated_state_noises(self):
        """uncertainty.py:35-65: one white-noise value shared by the adsorbates,
        times a uniform variate per transition state, in first-seen order."""
        noise = self.get_noise(noise_type='white')
        state_noises = dict()
        for intermediates, transition_states in self._walk(self.sys):
            for reac in intermediates:
                if reac.state_type == 'adsorbate':
                    if reac.name not in state_noises.keys():
                        state_noises[reac.name] = noise
            for reac in transition_states:
                if reac.name not in state_noises.keys():
                    frac = self.get_noise(noise_type='uniform')
                    state_noises[reac.name] = (noise * frac)
        return state_noises

    def set_correlated_state_noises(self, state_noises):
        """uncertainty.py:67-96: a deep copy of the system with the noises as the
        states' (float) energy modifiers.  The copy compiles a network of its
        own; the ensemble methods below do not use it."""
        noisy_sys = copy.deepcopy(self.sys)
        for intermediates, transition_states in self._walk(noisy_sys):
            for reac in intermediates:
                if reac.state_type == 'adsorbate':
                    reac.set_energy_modifier(state_noises[reac.name])
            for reac in transition_states:
                reac.set_energy_modifier(state_noises[reac.name])
        return noisy_sys

    # -- the ensemble as one network ----------------------------------------------
    def noise_states(self):
        """(adsorbates, transition_states): the perturbed states' names in
        first-seen order over sys.reactions."""
        ads, tss = [], []
        for intermediates, transition_states in self._walk(self.sys):
            for s in intermediates:
                if s.state_type == 'adsorbate' and s.name not in ads and s.name not in tss:
                    ads.append(s.name)
            for s in transition_states:
                if s.name not in tss and s.name not in ads:
                    tss.append(s.name)
        return ads, tss

    def descriptor_names(self):
        """The ensemble network's descriptors in device order: row k of the
        noise matrix (pck_ensemble_noise) is descriptor k."""
        return [ADS] + [TS + t for t in self.noise_states()[1]]

    def ensemble_system(self):
        """A deep copy of sys whose perturbed states carry descriptors as energy
        modifiers: Descriptor('@unc:ads') on every adsorbate, '@unc:ts:<name>'
        on transition state <name>.  One plan of 1 + n_ts descriptors and one
        device network serve every member of any ensemble.  Those are the
        plan's only descriptors: a system whose energies already depend on
        descriptors of its own (or on temperature-keyed user energies) is
        refused when the plan is compiled (KeyError)."""
        ens = copy.deepcopy(self.sys)
        ads, tss = self.noise_states()
        for intermediates, transition_states in self._walk(ens):
            for s in intermediates:
                if s.state_type == 'adsorbate' and s.name in ads:
                    s.set_energy_modifier(Descriptor(ADS))
            for s in transition_states:
                if s.name in tss:
                    s.set_energy_modifier(Descriptor(TS + s.name))
        ens.descriptor_order = self.descriptor_names()
        ens.desc_defaults = {k: 0.0 for k in ens.descriptor_order}
        return ens

    def _ensemble(self):
        if self._ens is None:
            self._ens = self.ensemble_system()
        return self._ens

    def _desc_of(self, noises, n):
        """{state: values} -> {descriptor: array [n]}; states not named get 0.
        The adsorbates share one descriptor, so their values must agree."""
        ads, tss = self.noise_states()
        unknown = [k for k in noises if k not in ads and k not in tss]
        if unknown:
            raise KeyError('noises name states the ensemble does not perturb: %s' % unknown)
        d = {k: np.zeros(n) for k in self.descriptor_names()}
        shared = [np.broadcast_to(np.asarray(noises[a], float), (n,)) for a in ads if a in noises]
        if shared:
            if any(not np.array_equal(shared[0], x) for x in shared[1:]):
                raise ValueError('the adsorbates of an ensemble share one noise value per run')
            d[ADS] = np.array(shared[0])
        for t in tss:
            if t in noises:
                d[TS + t] = np.array(np.broadcast_to(np.asarray(noises[t], float), (n,)))
        return d

    def _named(self, matrix, B, lead):
        """Rows of a noise matrix (first block, runs only) as {state name: values}."""
        ads, tss = self.noise_states()
        out = {a: matrix[0, lead:B] for a in ads}
        out.update({t: matrix[1 + k, lead:B] for k, t in enumerate(tss)})
        return out

    def sample_noises(self, nruns=None, rng='numpy', seed=None, run_first=0):
        """{state name: array [nruns]} of one ensemble's noise.
        rng='numpy': the reference's draws from the global np.random, run by
        run in its order (seeded here only if `seed` is given).
        rng='device': pck_ensemble_noise, Philox4x32-10 keyed by `seed`
        (None: 0), runs run_first .. run_first + nruns - 1."""
        nruns = self.nruns if nruns is None else int(nruns)
        if rng == 'numpy':
            if seed is not None:
                np.random.seed(seed)
            draws = [self.get_correlated_state_noises() for _ in range(nruns)]
            ads, tss = self.noise_states()
            return {k: np.array([d[k] for d in draws], float) for k in ads + tss}
        if rng != 'device':
            raise ValueError("rng must be 'numpy' or 'device', not %r" % (rng,))
        from ..engine import ensemble_noise
        m = ensemble_noise(seed or 0, nruns, 1, len(self.noise_states()[1]), False, self.mu, self.sigma, run_first)
        return self._named(m.cpu().numpy(), nruns, 0)

    def solve_ensemble(self, T=None, p=None, nruns=None, noises=None, rng='device', seed=0, tof_terms=(),
                       include_base=True, run_first=0, **solve_batch_kw):
        """The whole ensemble in one solve_batch launch: n_rep base conditions
        (T, p: scalars or arrays of one length; None: the system's) times
        B = nruns + include_base members, the runs of a base condition
        contiguous and its unperturbed member first (the block layout of
        include/pycatkin_amd.h).

        noises: {state name: array [nruns]} to use for every base condition;
        else they are drawn, rng='device' by pck_ensemble_noise under `seed`
        (the descriptor matrix never leaves the device) or rng='numpy' in the
        reference's order from the global np.random (seeded only by a non-zero
        `seed`).  Other keywords go to solve_batch (steady=True, t_end=, ...).

        Returns solve_batch's arrays reshaped to [..., n_rep, B], plus
        'noises' {state name: [nruns]} and 'stats': pck_ensemble_stats over
        the runs (the base member skipped) of the TOF ('tof') and of every
        dynamic species ('y', rows in 'species' order), each a dict of count,
        mean, std, min, max per base condition; runs of status 0 and 4 count,
        1, 2 and 3 do not and are reported as 'n_failed'.  to_numpy=False
        keeps every array on the device."""
        from ..engine import _torch, ensemble_noise, ensemble_stats
        torch = _torch()
        to_numpy = solve_batch_kw.pop('to_numpy', True)
        ens = self._ensemble()
        nruns = self.nruns if nruns is None else int(nruns)
        lead = int(bool(include_base))
        B = nruns + lead
        Tb = np.atleast_1d(np.asarray(ens.params['temperature'] if T is None else T, float)).ravel()
        pb = np.atleast_1d(np.asarray(ens.params['pressure'] if p is None else p, float)).ravel()
        n_rep = max(Tb.size, pb.size)
        Tb, pb = np.broadcast_to(Tb, (n_rep,)), np.broadcast_to(pb, (n_rep,))
        n = n_rep * B
        names = self.descriptor_names()
        if noises is None and rng == 'numpy':
            noises = self.sample_noises(nruns, 'numpy', seed or None)
        if noises is not None:
            d = self._desc_of(noises, nruns)
            block = np.zeros((len(names), B))
            block[:, lead:] = np.stack([d[k] for k in names])
            desc = torch.as_tensor(np.tile(block, (1, n_rep)), dtype=torch.float64, device='cuda')
        elif rng == 'device':
            desc = ensemble_noise(seed, nruns, n_rep, len(names) - 1, lead, self.mu, self.sigma, run_first)
        else:
            raise ValueError("rng must be 'numpy' or 'device', not %r" % (rng,))
        r = ens.solve_batch(T=np.repeat(Tb, B), p=np.repeat(pb, B), desc=desc, tof_terms=tuple(tof_terms),
                            to_numpy=False, **solve_batch_kw)
        # status: which runs count (tof's own count also leaves out a non-finite TOF)
        ok = (0, 4)
        stats = dict(tof=ensemble_stats(r['tof'], r['status'], ok, B, lead),
                     y=ensemble_stats(r['y'], r['status'], ok, B, lead),
                     species=list(ens.plan(tuple(tof_terms)).dyn))
        counted = ensemble_stats(torch.ones(n, dtype=torch.float64, device='cuda'), r['status'], ok, B, lead,
                                 want=('count',))['count']
        stats['n_failed'] = nruns - counted
        out = {k: v.reshape(tuple(v.shape[:-1]) + (n_rep, B)) for k, v in r.items()}
        out['noises'] = self._named(desc, B, lead)
        out['stats'] = stats
        if to_numpy:
            host = lambda x: x.cpu().numpy() if hasattr(x, 'cpu') else x
            out = {k: ({a: ({b: host(w) for b, w in v.items()} if isinstance(v, dict) else host(v))
                        for a, v in x.items()} if isinstance(x, dict) else host(x)) for k, x in out.items()}
        return out

    @staticmethod
    def statistics(values, status=None, ok=(0, 4), block=None, skip=0):
        """pck_ensemble_stats: count, mean, population std, min and max of
        `values` [n_rows, n] (or [n]) over the columns skip .. block-1 of every
        block of `block` columns (None: all n), counting the finite values
        whose `status` [n] (optional) is one of `ok`.  Host arrays in, host
        arrays out; device tensors stay on the device."""
        from ..engine import ensemble_stats
        on_device = hasattr(values, 'is_cuda')
        r = ensemble_stats(values, status, ok, block, skip)
        return r if on_device else {k: v.cpu().numpy() for k, v in r.items()}

    # -- the reference's drop-in methods (uncertainty.py:98-125) --------------------
    def _member(self, ens, values):
        """A member system: the ensemble system's states, reactions and plan
        cache (shared: no network is compiled or uploaded for it) with its
        own descriptor values, parameters and results."""
        s = copy.copy(ens)
        s.params = copy.deepcopy(ens.params)
        s.desc_defaults = dict(values)
        s.solution = s.times = s.full_steady = s.rates = None
        return s

    def get_noisy_sys_samples(self):
        """uncertainty.py:98-113: noisy_sys[0] the unperturbed system,
        noisy_sys[1..nruns] with the reference's draws, every one with .times
        and .solution as solve_odes fills them -- from one batched launch over
        the nruns + 1 members."""
        ens = self._ensemble()
        nruns = int(self.nruns)
        self.state_noises = dict()
        for run in range(1, nruns + 1):
            self.state_noises[run] = copy.deepcopy(self.get_correlated_state_noises())
        keys = list(self.state_noises[1].keys()) if nruns else []
        self.state_noises[0] = dict(zip(keys, np.zeros(len(keys))))
        n = nruns + 1
        cols = self._desc_of({k: np.array([self.state_noises[run][k] for run in range(n)]) for k in keys}, n)
        plan = ens.plan()
        times = ens.output_times()
        inside = times[times >= float(ens.params['times'][0])]
        r = ens.solve_batch(T=np.full(n, float(ens.params['temperature'])), desc=cols, t_out=inside)
        self.noisy_sys = dict()
        for run in range(n):
            ens._check(r['status'][run], 'get_noisy_sys_samples (run %d)' % run)
            s = self._member(ens, {k: float(v[run]) for k, v in cols.items()})
            sol = np.empty((times.size, len(plan.species)))
            sol[:times.size - inside.size] = s._full(plan, plan.y0_default)
            for k in range(inside.size):
                sol[times.size - inside.size + k] = s._full(plan, r['traj'][k, :, run])
            s.times, s.solution = times, sol
            self.noisy_sys[run] = s
        self.sys.times, self.sys.solution = times, self.noisy_sys[0].solution.copy()

    def get_mean_property_value(self, property_handle):
        """uncertainty.py:115-125: (values of runs 0..nruns, mean, std over runs 1..)."""
        self.get_noisy_sys_samples()
        property_values = np.array([property_handle(self.noisy_sys[i]) for i in self.noisy_sys.keys()])
        mean_property_value = np.mean(property_values[1::])
        std_property_value = np.std(property_values[1::])
        return property_values, mean_property_value, std_property_value

    # -- energy-span model of the ensemble --------------------------------------------
    def energy_span_ensemble(self, landscape, T=None, p=None, noises=None, nruns=None, rng='device', seed=0,
                             etype='free', to_numpy=True):
        """The energy-span model (Energy.evaluate_batch, pck_energy_span) of
        every member: `landscape` names one of sys.energy_landscapes, T and p
        are scalars, `noises` {state name: array [nruns]} may name any state
        of the system (a state outside the reaction walk gets a descriptor of
        its own); without it they are drawn as in solve_ensemble."""
        ens = copy.deepcopy(self._ensemble())
        pes = ens.energy_landscapes[landscape] if isinstance(landscape, str) else landscape
        nruns = self.nruns if nruns is None else int(nruns)
        ads, tss = self.noise_states()
        if noises is None:
            noises = self.sample_noises(nruns, rng, seed if rng == 'device' else (seed or None))
        else:
            nruns = max(int(np.size(v)) for v in noises.values())
        walk = {k: v for k, v in noises.items() if k in ads or k in tss}
        desc = self._desc_of(walk, nruns)
        # a state outside the reaction walk (an adsorbate only the landscape holds)
        extra = [k for k in noises if k not in walk]
        found = set()
        for s in list(ens.states.values()) + [s for entry in pes.minima for s in entry]:
            if s.name in extra:
                s.set_energy_modifier(Descriptor(EXTRA + s.name))
                found.add(s.name)
        if found != set(extra):
            raise KeyError('noises name unknown states %s' % sorted(set(extra) - found))
        for k in extra:
            desc[EXTRA + k] = np.array(np.broadcast_to(np.asarray(noises[k], float), (nruns,)))
        T = ens.params['temperature'] if T is None else T
        p = ens.params['pressure'] if p is None else p
        r = pes.evaluate_batch(T=T, p=p, desc=desc, etype=etype, to_numpy=to_numpy)
        r['noises'] = dict(noises)
        return r
