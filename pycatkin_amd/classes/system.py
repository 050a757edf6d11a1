"""System: the reference's System API on top of the batched device solver.

Reference-API methods (pycatkin/classes/old_system.py -- the API every example
driver uses -- and the steady-state helpers of the patched
pycatkin/classes/system.py) are kept with their names and argument meaning.
Each of them is a batch of one through the same C-ABI the batched methods
(`*_batch`) use; there is no CPU compute path.
"""
from __future__ import annotations

import copy
from typing import NamedTuple

import numpy as np

from ..constants.physical_constants import R, bartoPa, eVtokJ, h, kB
from .. import _lib as _L
from ..energy import TKEYED, LinearForm
from .reaction import Reaction
from .reactor import InfiniteDilutionReactor, PFReactor, Reactor
from .state import State


# Steady-state solves (steady=True; DESIGN.md "Steady state").  The transient
# to t_end is integrated at STEADY_TRANSIENT = (rtol, atol), Newton polishes
# its end state, and the root is the answer only if the transient has reached
# it: every dynamic species within ROOT_DIST * |root| + atol of it
# (pck_solve_params.root_dist).  Otherwise (status 4) the answer is the
# transient end at t_end -- the reference's System.activity semantics
# (old_system.py:517-529, what examples/COOxVolcano/cooxvolcano.py:47 reports).
# The tiny atol makes the error control relative on every coverage, down to
# the 1e-16 free sites of an O-poisoned surface whose product the TOF is, so
# that the distance test compares two well-resolved states; the rtol is what
# the 1e-6 bound on log10(TOF) needs with margin: measured on the 89 043
# degenerate points of the 1024 x 1024 volcano grid against a 1e-12 / 1e-24
# run (tools/retry_probe.py, profiles/r3/retry_probe.json), 1e-6 / 1e-22 is
# within 2.7e-8 relative.  On that grid one transient at these tolerances
# costs less than round 3's input-tolerance pass plus a tight retry of the
# degenerate points (6.1 ms against 7.5 ms per step, profiles/r4/tolerance_ab).
STEADY_TRANSIENT = (1.0e-6, 1.0e-22)
ROOT_DIST = 1.0e-6
# round-3 name of the tight tolerances (the retry pass, now optional)
DEGENERATE_RETRY = STEADY_TRANSIENT
# Screening pass of steady solves (round 5, pck_solve_params.screen_rtol;
# DESIGN.md "Screening pass"): the rule first at rtol SCREEN_RTOL (atol scaled
# alike), a root accepted there only within SCREEN_MARGIN * ROOT_DIST * |root|
# + atol (the caller's, round 6) of the screening transient's end.  With that
# absolute term a margin of 0.1 sent ~15 % of the CSTR sweep's trips to a full
# solve (2.8 vs 1.4 ms); 0.5 accepts all of them and 2 % more of the volcano
# grid (2.32 vs 2.37 ms), with 0 status changes on both against the single
# pass (profiles/r6/ab_screen_acceptance, screen_check_*_m0.5.json); every other condition is solved again at
# STEADY_TRANSIENT exactly as without screening.  A transient that has settled
# on its root ends on it at any tolerance, so the accepted conditions report
# the same root.
SCREEN_RTOL = 3.0e-2
SCREEN_MARGIN = 0.5
# 'auto' screens the one-lane networks (<= 8 dynamic species: the volcano and
# CSTR configs); the lane-group kernels screen too when asked (screen=rtol),
# but a network that rarely reaches its root by t_end (the synthetic one
# never does) would then solve most conditions twice
SCREEN_MAX_LANE_SPECIES = 8


def _retry_tolerances(retry):
    """solve_batch's `retry`: None -> no second pass, 'auto' -> STEADY_TRANSIENT,
    else a positive (rtol, atol) pair (any sequence or array of two)."""
    if isinstance(retry, str):
        if retry != 'auto':
            raise ValueError("retry must be 'auto', None or an (rtol, atol) pair, not %r" % retry)
        return DEGENERATE_RETRY
    if retry is None:
        return None
    r = np.asarray(retry, float).ravel()
    if r.size != 2 or not np.all(r > 0.0):
        raise ValueError('retry must be a positive (rtol, atol) pair, not %r' % (retry,))
    return float(r[0]), float(r[1])


class SteadyStateResults(NamedTuple):
    """system.py:20-30"""
    x: np.ndarray
    success: bool


class System:
    """Holds states, reactions and a reactor; solves batches of MK models.

    formulation: 'classic' (old_system.py, default) or 'patched' (system.py).
    rate_model:  'classic' (thermodynamic reverse rate for non-activated
                 adsorption/desorption -- what the reference's goldens pin) or
                 'patched' (kads/kdes, reaction.py:135-162)."""

    def __init__(self, times=None, start_state=None, inflow_state=None, T=293.15, p=101325.0,
                 use_jacobian=True, ode_solver='solve_ivp', nsteps=1e4, rtol=1e-8, atol=1e-10,
                 xtol=1e-8, ftol=1e-8, verbose=False, y0=None, min_tol=1e-32,
                 formulation='classic', rate_model='classic', path_to_pickle=None):
        if path_to_pickle:
            raise NotImplementedError('pickled systems are not loaded (no unpickling of external files)')
        self.states = dict()
        self.unique_states = set()
        self.reactions = dict()
        self.reactor = None
        self.energy_landscapes = None
        self.formulation = formulation
        self.rate_model = rate_model
        self.min_tol = min_tol
        self.snames = None
        self.solution = None
        self.times = None
        self.full_steady = None
        self.rates = None
        self.rate_constants = None
        self._plans = {}
        # Optional (both None: nothing changes).  descriptor_order: the
        # descriptor names of every plan of this system, in device order (names
        # no energy uses included); desc_defaults: {descriptor: value} used
        # where a call passes no `desc`.  An uncertainty ensemble sets both
        # (classes/uncertainty.py): its members share one plan and answer
        # single-condition calls with their own noise values.
        self.descriptor_order = None
        self.desc_defaults = None
        self.set_parameters(times=times, start_state=start_state, inflow_state=inflow_state, T=T, p=p,
                            use_jacobian=use_jacobian, ode_solver=ode_solver, nsteps=nsteps, rtol=rtol, atol=atol,
                            xtol=xtol, ftol=ftol, verbose=verbose)

    # -- setup (old_system.py:49-175, system.py:90-187) ------------------------
    def set_parameters(self, times=None, start_state=None, inflow_state=None, T=293.15, p=101325.0,
                       use_jacobian=True, ode_solver='solve_ivp', nsteps=1e4, rtol=1e-8, atol=1e-10,
                       xtol=1e-8, ftol=1e-8, verbose=False):
        self.params = dict(times=copy.deepcopy(times), start_state=copy.deepcopy(start_state),
                           inflow_state=copy.deepcopy(inflow_state), temperature=T, pressure=p, rtol=rtol,
                           atol=atol, xtol=xtol, ftol=ftol, jacobian=use_jacobian, nsteps=int(nsteps),
                           ode_solver=ode_solver, verbose=verbose)

    def __deepcopy__(self, memo):
        """A deep copy (butadiene_mkm.py:47, analysis.py:40) starts with an
        empty plan cache: device networks are not copied."""
        out = self.__class__.__new__(self.__class__)
        memo[id(self)] = out
        for k, v in self.__dict__.items():
            setattr(out, k, {} if k == '_plans' else copy.deepcopy(v, memo))
        return out

    # patched-API attribute names
    @property
    def T(self):
        return self.params['temperature']

    @T.setter
    def T(self, v):
        self.params['temperature'] = v

    @property
    def p(self):
        return self.params['pressure']

    @p.setter
    def p(self, v):
        self.params['pressure'] = v

    @property
    def start_state(self):
        return self.params['start_state'] or {}

    @property
    def inflow_state(self):
        return self.params['inflow_state'] or {}

    def add_state(self, state):
        assert isinstance(state, State), 'state %s MUST be an instance of State' % state
        if state.name in self.unique_states:
            raise ValueError('Found two copies of state %s. State names must be unique!' % state.name)
        self.unique_states.add(state.name)
        self.states[state.name] = state
        self.snames = sorted(self.states)
        self._plans.clear()

    def add_reaction(self, reaction):
        assert isinstance(reaction, Reaction), 'reaction %s MUST be an instance of Reaction' % reaction
        self.reactions[reaction.name] = reaction
        self._plans.clear()

    def add_reactor(self, reactor):
        assert isinstance(reactor, Reactor)
        self.reactor = reactor
        self._plans.clear()

    def add_energy_landscape(self, energy_landscape):
        if self.energy_landscapes is None:
            self.energy_landscapes = dict()
        self.energy_landscapes[energy_landscape.name] = energy_landscape

    def names_to_indices(self):
        """old_system.py:99-152 index bookkeeping (kept for API compatibility)."""
        self.snames = sorted(self.states)
        ads, gas = set(), set()
        for r in self.reactions.values():
            for s in r.reactants + r.products:
                if s.state_type in ('adsorbate', 'surface'):
                    ads.add(self.snames.index(s.name))
                elif s.state_type == 'gas':
                    gas.add(self.snames.index(s.name))
        self.adsorbate_indices = sorted(ads)
        self.gas_indices = sorted(gas)
        n = len(self.snames)
        if self.reactor is not None:
            self.reactor.set_indices([1 if i in ads else 0 for i in range(n)], [1 if i in gas else 0 for i in range(n)])
            self.dynamic_indices = self.reactor.get_dynamic_indices(self.adsorbate_indices, self.gas_indices)

    def build(self):
        """Index bookkeeping: old_system.py:99-152 (classic) or system.py:167-187
        (patched: coverage_map, gas_indices, index_map, rate_map,
        initial_system, reaction_matrix)."""
        if self.formulation == 'patched':
            return self._build_patched()
        return self.names_to_indices()

    # -- patched-formulation API (pycatkin/classes/system.py) --------------------
    def _build_patched(self):
        """system.py:191-394: index_map (gas first, then each surface followed by
        its adsorbates), coverage_map {surface: set of indices}, gas_indices,
        rate_map, initial_system (normalised, capped at min_tol) and the +-1
        reaction_matrix (species x non-ghost reactions, products win)."""
        order = self.index_map_ordered()
        self.index_map = {s: i for i, s in enumerate(order)}
        self.gas_indices = {i for i, s in enumerate(order) if self.states[s].state_type == 'gas'}
        self.coverage_map = {sf: {self.index_map[x] for x in grp} for sf, grp in self._coverage_names.items()}
        self.rate_map = {}
        for name, rx in self.reactions.items():
            if str(rx.reac_type).upper() == 'GHOST':
                continue
            self.rate_map[name] = {'reac': [self.index_map[x.name] for x in rx.reactants],
                                   'prod': [self.index_map[x.name] for x in rx.products],
                                   'site_density': 1.0 / rx.area if rx.area else 0.0, 'scaling': rx.scaling}
        self.initial_system = self.initial_vector()
        M = np.zeros((len(order), len(self.rate_map)))
        for j, rm in enumerate(self.rate_map.values()):
            M[rm['reac'], j] = -1.0
            M[rm['prod'], j] = 1.0
        self.reaction_matrix = M
        return self

    def _patched_eval(self):
        if self.formulation != 'patched':
            raise RuntimeError('the System._fun_ss / get_dydt family belongs to the patched formulation '
                               '(System(formulation="patched"), pycatkin/classes/system.py)')
        if getattr(self, 'initial_system', None) is None:
            self._build_patched()
        plan = self.plan()
        net = self.device()
        ngas = len(self.gas_indices)
        return plan, net, ngas

    def _device_state(self, plan, y_full):
        """(surface part in plan.dyn order, gas concentrations x p in plan.fix order)."""
        y_full = np.asarray(y_full, float).ravel()
        idx = self.index_map
        yd = np.array([y_full[idx[s]] for s in plan.dyn])
        fx = np.array([y_full[idx[s]] for s in plan.fix]) * float(self.p)
        return yd, fx

    def _rates_batch(self, Y, desc=None):
        """forward / backward rates [n_reactions, m] (rate_map order) at full
        compositions Y [n_species, m] (gas fractions x p), one device launch;
        `desc` {name: [m]} for a network with descriptor energies."""
        plan, net, ngas = self._patched_eval()
        Y = np.asarray(Y, float)
        m = Y.shape[1]
        idx = self.index_map
        yd = Y[[idx[s] for s in plan.dyn]]
        fx = Y[[idx[s] for s in plan.fix]] * float(self.p)
        T, p, d, _, _, _ = self._inputs(net, plan, m, np.full(m, float(self.T)), float(self.p), desc,
                                        None, None, None)
        kf, kr = net.rate_constants(m, T, p, d)
        rf, rr = net.reaction_rates(m, T, p, yd, kf, kr, d, fx)
        rf, rr = rf.cpu().numpy(), rr.cpu().numpy()
        names = list(self.rate_map)
        order = [plan.reactions.index(name) for name in names]
        return rf[order], rr[order]

    def _calc_rates(self, y):
        """system.py:345-376: (n_reactions, 2) forward / backward rates at the
        full composition y (gas fractions x p), on the device."""
        rf, rr = self._rates_batch(np.asarray(y, float).reshape(-1, 1))
        return np.stack([rf[:, 0], rr[:, 0]], axis=1)

    def get_dydt(self, y):
        """system.py:396-416: reaction_matrix @ (r_fwd - r_rev) for every tracked species."""
        rates = self._calc_rates(y)
        return self.reaction_matrix @ (rates[:, 0] - rates[:, 1])

    def get_dydt_batch(self, Y, desc=None):
        """get_dydt for compositions Y [n_species, m] in one launch."""
        rf, rr = self._rates_batch(Y, desc)
        return self.reaction_matrix @ (rf - rr)

    def get_forward_only(self, y):
        """system.py:418-433 (the reference multiplies by the backward column)."""
        return self.reaction_matrix @ self._calc_rates(y)[:, 1]

    def _jac(self, y):
        """system.py:437-491: d r_j / d y_k (n_reactions x n_species).  Every
        species enters a side of a reaction with exponent 1 (a repeated species
        with its count), so d(k prod c)/d y_k = k prod(others) (x p for a gas):
        the rate of that side with y_k set to 1 -- one device launch evaluates
        the rates at all n_species such compositions.  The reference's P_term
        (system.py:478-484) multiplies by p only when ANOTHER species of the
        side is a gas, so the column of a gas species itself carries no p:
        that column is divided by p here to return the reference's matrix
        (the device integrators use the exact derivative)."""
        self._patched_eval()
        y = np.asarray(y, float).ravel()
        n = len(y)
        Y = np.repeat(y[:, None], n, axis=1)
        Y[np.arange(n), np.arange(n)] = 1.0
        rf, rr = self._rates_batch(Y)
        out = np.zeros((len(self.rate_map), n))
        for j, (name, rm) in enumerate(self.rate_map.items()):
            for lst, other, sgn, r in ((rm['reac'], rm['prod'], 1.0, rf), (rm['prod'], rm['reac'], -1.0, rr)):
                for i in set(lst):
                    if i in other:
                        raise RuntimeError('Species %d appreas on both sides of reaction %s' % (i, name))
                    cnt = lst.count(i)
                    # side rate at y_i = 1 is k prod(others) y_i^0 -> times cnt y_i^(cnt-1)
                    out[j, i] = sgn * r[j, i] * (cnt * y[i] ** (cnt - 1) if cnt > 1 else 1.0)
                    if i in self.gas_indices:
                        out[j, i] /= float(self.p)
        return out

    def get_jacobian(self, y):
        """system.py:493-508: reaction_matrix @ _jac(y)."""
        return self.reaction_matrix @ self._jac(y)

    def _ss_pre(self, y_surf):
        """system.py:512-526"""
        self._patched_eval()
        y_gas = self.initial_system[sorted(self.gas_indices)]
        return np.concatenate([y_gas, np.asarray(y_surf, float)])

    def _fun_ss(self, y_surf):
        """system.py:528-545: surface rates at the invariant gas composition (device pck_species_rates)."""
        return self._fun_ss_batch(np.asarray(y_surf, float)[:, None])[:, 0]

    def _jac_ss(self, y_surf):
        """system.py:547-564: surface block of the Jacobian (device pck_jacobian)."""
        return self._jac_ss_batch(np.asarray(y_surf, float)[:, None])[:, :, 0]

    def _fun_ss_batch(self, Y, desc=None, T=None):
        """_fun_ss for a batch of surface states Y [n_surface, n] in one launch
        (`desc` / `T`: per-condition descriptor energies / temperatures)."""
        plan, net, ngas = self._patched_eval()
        n = Y.shape[1]
        T = float(self.T) if T is None else T
        T, p, d, fx, y0, inflow = self._inputs(net, plan, n, T, None, desc, None, None, None)
        kf, kr = net.rate_constants(n, T, p, d)
        return net.species_rates(n, T, p, self._to_plan(plan, Y), kf, kr, d, fx, inflow).cpu().numpy()[self._from_plan(plan)]

    def _jac_ss_batch(self, Y, desc=None, T=None):
        plan, net, ngas = self._patched_eval()
        n = Y.shape[1]
        T = float(self.T) if T is None else T
        T, p, d, fx, y0, inflow = self._inputs(net, plan, n, T, None, desc, None, None, None)
        kf, kr = net.rate_constants(n, T, p, d)
        J = net.jacobian(n, T, p, self._to_plan(plan, Y), kf, kr, d, fx, inflow).cpu().numpy()
        inv = self._from_plan(plan)
        return J[np.ix_(inv, inv)]

    def _jac_ss_re_max_batch(self, Y, desc=None, T=None):
        """(largest real part of the eigenvalues of _jac_ss, status) [n] of the
        surface states Y [n_surface, n], Jacobian and eigenvalues on the
        device (pck_stability_at, the full matrix: solver.py:102-106)"""
        plan, net, ngas = self._patched_eval()
        n = Y.shape[1]
        T = float(self.T) if T is None else T
        T, p, d, fx, y0, inflow = self._inputs(net, plan, n, T, None, desc, None, None, None)
        kf, kr = net.rate_constants(n, T, p, d)
        r = net.stability_at(n, T, p, self._to_plan(plan, Y), kf, kr, d, fx, inflow, None, reduce=False,
                             lanes=_L.SENS_LANES_AUTO, want=('re_max', 'status'))
        return r['re_max'].cpu().numpy(), r['status'].cpu().numpy()

    def _surface_order(self):
        return [s for s in sorted(self.index_map, key=self.index_map.get) if self.index_map[s] not in self.gas_indices]

    def _to_plan(self, plan, Y):
        """surface states in index_map order -> plan.dyn order"""
        order = self._surface_order()
        return np.asarray(Y, float)[[order.index(s) for s in plan.dyn]]

    def _from_plan(self, plan):
        """permutation taking plan.dyn order back to index_map order"""
        return [plan.dyn.index(s) for s in self._surface_order()]

    # -- patched-formulation bookkeeping (system.py:191-328) -------------------
    def index_map_ordered(self):
        ads = [n for n, s in self.states.items() if s.state_type == 'adsorbate']
        gas = sorted(n for n, s in self.states.items() if s.state_type == 'gas')
        surf = sorted(n for n, s in self.states.items() if s.state_type == 'surface')
        order = list(gas)
        self._coverage_names = {}
        for sf in surf:
            grp = [sf] + [a for a in ads if a[0] == sf]
            self._coverage_names[sf] = grp
            order += grp
        return order

    def initial_vector(self):
        """system.py:282-328: normalised gas fractions and site coverages, capped at min_tol."""
        order = self.index_map_ordered()
        pos = {s: i for i, s in enumerate(order)}
        y = np.zeros(len(order))
        for d in (self.start_state, self.inflow_state):
            for k, v in d.items():
                y[pos[k]] = v
        gi = [pos[s] for s in order if self.states[s].state_type == 'gas']
        if gi:
            y[gi] /= np.sum(y[gi])
        for grp in self._coverage_names.values():
            ii = [pos[s] for s in grp]
            y[ii] /= np.sum(y[ii])
        return np.where(y < self.min_tol, self.min_tol, y)

    def start_state_values(self):
        return dict(self.start_state)

    def inflow_state_values(self):
        return dict(self.inflow_state)

    # -- compilation -------------------------------------------------------------
    def plan(self, tof_terms=(), descriptors=None):
        from ..network import compile_system
        if descriptors is None:
            descriptors = getattr(self, 'descriptor_order', None)
        key = (tuple(tof_terms), tuple(descriptors) if descriptors else None, self.formulation, self.rate_model,
               self._energy_key())
        if key not in self._plans:
            if self.snames is None:
                self.snames = sorted(self.states)
            plan = compile_system(self, tof_terms=tof_terms, descriptors=descriptors, rate_model=self.rate_model)
            self._plans[key] = [plan, None]
        return self._plans[key][0]

    def device(self, tof_terms=(), descriptors=None):
        from ..engine import DeviceNetwork
        plan = self.plan(tof_terms, descriptors)
        key = [k for k, v in self._plans.items() if v[0] is plan][0]
        if self._plans[key][1] is None:
            self._plans[key][1] = DeviceNetwork.from_plan(plan)
        return self._plans[key][1]

    def _energy_key(self):
        """User energies may be mutated between calls (volcano drivers): key the cache on them."""
        out = []
        for r in self.reactions.values():
            for a in ('dErxn_user', 'dEa_fwd_user', 'dEa_rev_user', 'dGrxn_user', 'dGa_fwd_user', 'dGa_rev_user'):
                v = getattr(r, a, None)
                if isinstance(v, dict):             # temperature-keyed (energy.tkeyed)
                    v = tuple(sorted((float(k), float(x)) for k, x in v.items()))
                out.append(repr(v) if isinstance(v, LinearForm) else v)
        return tuple(out)

    # -- batch inputs --------------------------------------------------------------
    def _inputs(self, net, plan, n, T, p, desc, y0, fix, inflow):
        T = self.params['temperature'] if T is None else T
        p = self.params['pressure'] if p is None else p
        d = None
        if desc is None:
            desc = getattr(self, 'desc_defaults', None)
        if plan.descriptors and desc is not None and not isinstance(desc, dict):
            # a [D, n] matrix in plan.descriptors order, host or device (an
            # ensemble's noise matrix never leaves the device)
            if any(k.startswith('@T:') for k in plan.descriptors):
                raise ValueError('a descriptor matrix cannot fill temperature-keyed user energies; pass a dict')
            if tuple(desc.shape) != (len(plan.descriptors), n):
                raise ValueError('descriptor matrix has shape %s, expected (%d, %d)'
                                 % (tuple(desc.shape), len(plan.descriptors), n))
            d = desc
        elif plan.descriptors:
            given = [k for k in plan.descriptors if not k.startswith('@T:')]
            if given and desc is None:
                raise ValueError('network depends on descriptors %s' % given)
            Tn = np.broadcast_to(np.asarray(T, float), (n,))
            cols = []
            for k in plan.descriptors:
                if k.startswith('@T:'):             # temperature-keyed user energy (energy.tkeyed)
                    table = TKEYED[k]
                    cols.append(np.array([table[float(t)] for t in Tn]))
                else:
                    cols.append(np.broadcast_to(np.asarray(desc[k], float), (n,)))
            d = np.stack(cols)
        if fix is None:
            if plan.formulation == 'patched':
                pp = np.broadcast_to(np.asarray(p, float), (n,))
                fix = plan.fix_default[:, None] * pp[None, :] if len(plan.fix) else None
            else:
                fix = plan.fix_default * plan.fix_conc_factor
        else:
            fix = np.asarray(fix, float) * (plan.fix_conc_factor[:, None] if np.ndim(fix) == 2 else plan.fix_conc_factor)
        y0 = plan.y0_default if y0 is None else y0
        inflow = plan.inflow_default if inflow is None else inflow
        return T, p, d, fix, y0, inflow

    @staticmethod
    def _n(*xs):
        sizes = [int(np.size(x)) for x in xs if x is not None and np.ndim(x) > 0]
        return max(sizes) if sizes else 1

    # -- batched entry points ------------------------------------------------------
    def rate_constants_batch(self, T=None, p=None, desc=None):
        """kf, kr [active reactions, n] (reaction.py:94 for every condition)."""
        plan = self.plan((), None)
        net = self.device((), None)
        n = self._n(T, p, *(desc or {}).values()) if desc else self._n(T, p)
        T, p, d, _, _, _ = self._inputs(net, plan, n, T, p, desc, None, None, None)
        kf, kr = net.rate_constants(n, T, p, d)
        return kf.cpu().numpy(), kr.cpu().numpy()

    def solve_batch(self, T=None, p=None, desc=None, y0=None, fix=None, inflow=None, tof_terms=(),
                    steady=False, activity=False, t_end=None, t0=None, rtol=None, atol=None, max_steps=200000,
                    newton_iters=60, to_numpy=True, t_out=None, retry=None, root_dist='auto', screen='auto',
                    wave_order='auto'):
        """Transient solve to t_end (solve_odes), optionally polished to the
        steady state (find_steady), with TOF or activity per condition; with
        t_out, also the dynamic state at those times ('traj' [n_out, NS, n],
        RODAS4P dense output).

        steady=True: the transient runs at STEADY_TRANSIENT (1e-6 / 1e-22)
        unless rtol / atol are given here -- the System's params['rtol'] /
        ['atol'] (the input file's) are NOT used for steady solves, since the
        rule's distance test needs relative error control on every coverage
         -- and the Newton root of its end state is reported (status
        0) where the transient has reached it to `root_dist` ('auto':
        ROOT_DIST when t_end > t0, else 0 -- a polish of the given state, as
        find_steady); elsewhere the transient end (status 4).  `retry` =
        (rtol, atol) integrates the status-4 conditions again at those
        tolerances in a second launch (None: no second pass).  `screen`
        ('auto': SCREEN_RTOL for steady solves with root_dist > 0, no retry
        and no t_out; None: off; a number: the screening rtol) runs the rule
        at that loose tolerance first and solves only the conditions it does
        not accept at the transient tolerances ('auto' on one-lane networks
        only; a number screens the 16- / 32-lane group networks too, a network
        of at most 16 species then running on the 16-lane kernel instead of
        the quad one; networks of more than 32 species refuse it).
        `wave_order` ('auto', 'on', 'off'; pck_solve_params.wave_order): the
        one-lane solver's cost-ordered dispatch, a preview of 4 samples per
        wavefront that puts the costliest wavefronts first ('auto': from
        131 072 conditions).  It pays where costs vary a lot across the batch
        (the volcano grid) and is overhead where they do not: a 262 144-
        temperature CSTR sweep takes 1.71 ms with it off against 2.36 ms
        (DESIGN.md "Round 6")."""
        if wave_order not in ('auto', 'on', 'off'):
            raise ValueError("wave_order must be 'auto', 'on' or 'off', not %r" % (wave_order,))
        self._refuse_pfr('solve_batch')
        plan = self.plan(tuple(tof_terms), None)
        net = self.device(tuple(tof_terms), None)
        if desc is not None and not isinstance(desc, dict):
            n = max(self._n(T, p), int(desc.shape[1]))
        else:
            n = self._n(*([T, p] + (list(desc.values()) if desc else [])))
        if y0 is not None and np.ndim(y0) == 2:
            n = max(n, np.shape(y0)[1])
        T, p, d, fx, y0, inflow = self._inputs(net, plan, n, T, p, desc, y0, fix, inflow)
        times = self.params['times'] or [0.0, 1.0e4]
        t0 = times[0] if t0 is None else t0
        t_end = times[-1] if t_end is None else t_end
        if steady:
            rtol = STEADY_TRANSIENT[0] if rtol is None else rtol
            atol = STEADY_TRANSIENT[1] if atol is None else atol
        if isinstance(root_dist, str):
            if root_dist != 'auto':
                raise ValueError("root_dist must be 'auto' or a number in [0, 1)")
            root_dist = ROOT_DIST if (steady and t_end > t0) else 0.0
        if isinstance(screen, str):
            if screen != 'auto':
                raise ValueError("screen must be 'auto', None or an rtol")
            screen = SCREEN_RTOL if (steady and root_dist > 0.0 and retry is None and t_out is None
                                     and net.NDYN <= SCREEN_MAX_LANE_SPECIES) else None
        out = net.solve(n, T, p, y0, d, fx, inflow, t0=t0, t_end=t_end,
                        rtol=self.params['rtol'] if rtol is None else rtol,
                        atol=self.params['atol'] if atol is None else atol,
                        max_steps=max_steps, newton=steady, newton_iters=newton_iters, activity=activity,
                        t_out=t_out, retry=_retry_tolerances(retry) if steady else None,
                        root_dist=float(root_dist) if steady else 0.0,
                        screen=(float(screen), SCREEN_MARGIN) if (steady and screen) else None,
                        wave_order={'auto': 0, 'on': 1, 'off': -1}[wave_order])
        if to_numpy:
            return {k: v.cpu().numpy() for k, v in out.items()}
        return out

    def _refuse_pfr(self, what, instead='solve_cascade_batch', verb='solves'):
        """A PFReactor's coefficients are one cell's: the single-reactor calls
        would silently answer for one cell of the bed."""
        if isinstance(self.reactor, PFReactor):
            raise ValueError('%s %s a single stirred tank; a PFReactor (%d cells) is %s by '
                             '%s' % (what, verb, self.reactor.cells, 'solved' if verb == 'solves' else 'analysed',
                                     instead))

    def _cascade_cells(self, cells):
        """The cell count of a bed call: the PFReactor's, or the caller's."""
        if cells is None:
            if not isinstance(self.reactor, PFReactor):
                raise ValueError('cells is required unless the reactor is a PFReactor')
            cells = self.reactor.cells
        if isinstance(cells, bool) or int(cells) != cells or not 1 <= int(cells) <= _L.MAX_CELLS:
            raise ValueError('cells must be an integer in 1..%d, not %r' % (_L.MAX_CELLS, cells))
        cells = int(cells)
        if isinstance(self.reactor, PFReactor) and cells != self.reactor.cells:
            raise ValueError('cells=%d differs from the PFReactor\'s %d (its flow rate is one cell\'s)'
                             % (cells, self.reactor.cells))
        return cells

    def _bed_objectives(self, plan, tof_terms, outlet, wr, wy):
        """(labels, wr [K, active reactions], wy [K, dynamic species]) of a bed
        DRC call: the bed-mean TOF of tof_terms, one outlet concentration per
        name in `outlet`, then the rows of wr / wy as given."""
        obs = []
        if tof_terms:
            obs.append({'rates': {}, 'label': 'tof'})
            for name in tof_terms:
                obs[0]['rates'][name] = obs[0]['rates'].get(name, 0.0) + 1.0
        for name in ([outlet] if isinstance(outlet, str) else list(outlet or ())):
            obs.append({'species': {name: 1.0}, 'label': 'outlet[%s]' % name})
        labels, a, b = self._objectives(plan, obs) if obs else ([], np.zeros((0, len(plan.reactions))),
                                                                np.zeros((0, len(plan.dyn))))
        if wr is not None or wy is not None:
            xr = None if wr is None else np.atleast_2d(np.asarray(wr, float))
            xy = None if wy is None else np.atleast_2d(np.asarray(wy, float))
            K = (xr if xr is not None else xy).shape[0]
            xr = np.zeros((K, len(plan.reactions))) if xr is None else xr
            xy = np.zeros((K, len(plan.dyn))) if xy is None else xy
            if xr.shape != (K, len(plan.reactions)) or xy.shape != (K, len(plan.dyn)):
                raise ValueError('wr / wy must be [K, %d] / [K, %d] (plan.reactions / plan.dyn order)'
                                 % (len(plan.reactions), len(plan.dyn)))
            labels = labels + ['w%d' % m for m in range(K)]
            a, b = np.vstack([a, xr]), np.vstack([b, xy])
        if not labels:
            raise ValueError('no objectives: give tof_terms, outlet, wr or wy')
        return labels, a, b

    def _bed_net(self, what):
        """(plan, device network) of a bed DRC call: a reactor with flow and at
        most MAX_DYN_LANE dynamic species."""
        plan = self.plan((), None)
        off = int(plan.ip[_L.I_HDR + _L.D_DYN])
        flow = np.asarray(plan.dp[off: off + 4 * len(plan.dyn)]).reshape(len(plan.dyn), 4)[:, 3]
        if not np.any(flow != 0.0):
            raise ValueError('%s needs a reactor with flow (CSTReactor or PFReactor)' % what)
        if len(plan.dyn) > _L.MAX_DYN_LANE:
            raise ValueError('%s runs on the one-lane adjoint kernel: at most %d dynamic species (this network '
                             'has %d)' % (what, _L.MAX_DYN_LANE, len(plan.dyn)))
        return plan, self.device((), None)

    def _bed_dict(self, plan, labels, r, n):
        out = self._multi_dict(plan, labels, r, n)
        if 'order_in' in r:
            out['order_in'] = r['order_in'].cpu().numpy()
        for key in ('cell_fail', 'y_cells', 'status_cells'):
            if key in r:
                out[key] = r[key].cpu().numpy()
        return out

    def cascade_drc_at(self, Y_cells, tof_terms=(), outlet=None, wr=None, wy=None, T=None, p=None, desc=None,
                       fix=None, inflow=None, status_cells=None, k=None):
        """The degree of rate control of a catalyst bed at given cell states
        Y_cells [cells, n_dynamic, n] (plan.dyn order; solve_cascade_batch's
        'y_cells'), without a solve: one backward adjoint sweep through the
        cells per condition, in one launch (pck_cascade_drc_at; DESIGN.md "Bed
        DRC").  Objectives as in cascade_drc_batch.  status_cells [cells, n]
        (optional): a bed is computed only if every cell's status is 0, else it
        keeps its bed status (the first failing cell's, else 4) and gets NaN.  k = (kf, kr) as in drc_at.
        Returns dict(labels, reactions, val [K, n], xi [K, R, n], order_in
        [K, NS, n], status [n], ostatus [K, n])."""
        plan, net = self._bed_net('cascade_drc_at')
        labels, a, b = self._bed_objectives(plan, tuple(tof_terms), outlet, wr, wy)
        Y = np.asarray(Y_cells, float)
        if Y.ndim == 2:
            Y = Y[:, :, None]
        if Y.ndim != 3 or Y.shape[1] != net.NDYN:
            raise ValueError('Y_cells must be [cells, %d, n]' % net.NDYN)
        self._cascade_cells(Y.shape[0])
        n = Y.shape[2]
        T, p, d, fx, _, inflow = self._inputs(net, plan, n, T, p, desc, None, fix, inflow)
        kf, kr = net.rate_constants(n, T, p, d) if k is None else k
        r = net.cascade_drc_at(n, T, p, Y, kf, kr, a, b, d, fx, inflow, status_cells)
        return self._bed_dict(plan, labels, r, n)

    def cascade_drc_batch(self, cells=None, tof_terms=(), outlet=None, wr=None, wy=None, T=None, p=None, desc=None,
                          y0=None, fix=None, inflow=None, t_end=None, rtol=None, atol=None, max_steps=200000,
                          newton_iters=60, screen='auto', start='system'):
        """Which rate constants control a catalyst bed: solve_cascade_batch
        (steady, method='fused') and then the adjoint sweep of cascade_drc_at at
        its cell states, with the solve's own rate constants (pck_cascade_drc;
        DESIGN.md "Bed DRC").  Objectives, in this order: tof_terms gives the
        bed-mean TOF (solve_cascade_batch's 'tof'); outlet=['CO', ...] one
        outlet-concentration objective per species; wr [K, active reactions] /
        wy [K, dynamic species] further weighted objectives (bed mean of the net
        rates / outlet state).  xi[m, j] = d ln J_m / d ln k_j at fixed K_j;
        order_in[m, i] = d ln J_m / d ln inflow_i.  For a fed species with inflow
        y_in and outlet y_out the conversion X = 1 - y_out / y_in has
        d ln X / d ln k_j = -xi . y_out / (y_in - y_out), xi the outlet
        objective's.  A bed with a cell that did not report a reached root
        (status 4) or that failed keeps that status and gets NaN.  Networks of
        at most 8 dynamic species; a larger one raises.  The remaining arguments
        are solve_cascade_batch's.  Returns dict(labels, reactions, val [K, n],
        xi [K, R, n], order_in [K, NS, n], status [n], ostatus [K, n], nsteps
        [n], cell_fail [n], y_cells [cells, NS, n], status_cells [cells, n])."""
        if start not in _L.CASCADE_START_MODES:
            raise ValueError("start must be 'system' or 'upstream', not %r" % (start,))
        cells = self._cascade_cells(cells)
        plan, net = self._bed_net('cascade_drc_batch')
        labels, a, b = self._bed_objectives(plan, tuple(tof_terms), outlet, wr, wy)
        if desc is not None and not isinstance(desc, dict):
            n = max(self._n(T, p), int(desc.shape[1]))
        else:
            n = self._n(*([T, p] + (list(desc.values()) if desc else [])))
        for x in (y0, inflow):
            if x is not None and np.ndim(x) == 2:
                n = max(n, np.shape(x)[1])
        T, p, d, fx, y0, inflow = self._inputs(net, plan, n, T, p, desc, y0, fix, inflow)
        times = self.params['times'] or [0.0, 1.0e4]
        t0 = times[0]
        t_end = times[-1] if t_end is None else t_end
        rtol = STEADY_TRANSIENT[0] if rtol is None else rtol
        atol = STEADY_TRANSIENT[1] if atol is None else atol
        root_dist = ROOT_DIST if t_end > t0 else 0.0
        if isinstance(screen, str):
            if screen != 'auto':
                raise ValueError("screen must be 'auto', None or an rtol")
            screen = SCREEN_RTOL if (root_dist > 0.0 and net.NDYN <= SCREEN_MAX_LANE_SPECIES) else None
        r = net.cascade_drc(n, T, p, y0, cells, a, b, d, fx, inflow, start=start, t0=t0, t_end=t_end, rtol=rtol,
                            atol=atol, max_steps=max_steps, newton=True, newton_iters=newton_iters,
                            root_dist=float(root_dist), screen=(float(screen), SCREEN_MARGIN) if screen else None,
                            wave_order=-1)
        return self._bed_dict(plan, labels, r, n)

    def solve_cascade_batch(self, cells=None, T=None, p=None, desc=None, y0=None, fix=None, inflow=None,
                            tof_terms=(), steady=True, t_end=None, rtol=None, atol=None, max_steps=200000,
                            newton_iters=60, root_dist='auto', screen='auto', start='system', method='auto',
                            profile=True, to_numpy=True):
        """A catalyst bed as `cells` CSTR cells in series at each condition
        (tanks in series, DESIGN.md "Reactor cascade"): cell c is solved as
        solve_batch(steady=...) solves a CSTR, with the gas of cell c-1 as its
        inflow (cell 0: `inflow`).  cells=None takes the PFReactor's count;
        with a plain CSTReactor, cells=N is N copies of the reactor as
        configured.  Tolerances and the screen / root_dist defaults are
        solve_batch's.  start: 'system' (every cell's transient starts from
        y0 -- what a loop of solve_batch(inflow=previous outlet) computes) or
        'upstream' (from the final state of the cell before).  method:
        'fused' (pck_solve_cascade, one launch; networks of at most 8 dynamic
        species), 'loop' (`cells` solves with device tensors, any network),
        'auto' (fused where available).
        A cell that reports status 4 passes its transient end on; an
        integrator failure (1-3) stops that condition's march: cell_fail holds
        the cell, later cells are NaN with that status.  Returns y [NS, n]
        (the outlet), tof [n] (mean of the cell TOFs; NaN where the march
        stopped), status [n] (the failing status, else 4 if any cell reported
        4, else 0), nsteps [n] (sum), cell_fail [n] (-1: none), conversion
        {gas: 1 - y_out / inflow} for the flow species with positive inflow
        and, with profile, y_cells [cells, NS, n], tof_cells, status_cells,
        nsteps_cells [cells, n]."""
        if start not in _L.CASCADE_START_MODES:
            raise ValueError("start must be 'system' or 'upstream', not %r" % (start,))
        if method not in ('auto', 'fused', 'loop'):
            raise ValueError("method must be 'auto', 'fused' or 'loop', not %r" % (method,))
        if cells is None:
            if not isinstance(self.reactor, PFReactor):
                raise ValueError('cells is required unless the reactor is a PFReactor')
            cells = self.reactor.cells
        if isinstance(cells, bool) or int(cells) != cells or not 1 <= int(cells) <= _L.MAX_CELLS:
            raise ValueError('cells must be an integer in 1..%d, not %r' % (_L.MAX_CELLS, cells))
        cells = int(cells)
        if isinstance(self.reactor, PFReactor) and cells != self.reactor.cells:
            raise ValueError('cells=%d differs from the PFReactor\'s %d (its flow rate is one cell\'s)'
                             % (cells, self.reactor.cells))
        plan = self.plan(tuple(tof_terms), None)
        off = int(plan.ip[_L.I_HDR + _L.D_DYN])
        flow = np.asarray(plan.dp[off: off + 4 * len(plan.dyn)]).reshape(len(plan.dyn), 4)[:, 3]
        if not np.any(flow != 0.0):
            raise ValueError('solve_cascade_batch needs a reactor with flow (CSTReactor or PFReactor)')
        one_lane = len(plan.dyn) <= _L.MAX_DYN_LANE
        if method == 'fused' and not one_lane:
            raise ValueError("method='fused' runs on the one-lane solver: at most %d dynamic species (this network "
                             "has %d); use method='loop'" % (_L.MAX_DYN_LANE, len(plan.dyn)))
        if method == 'auto':
            method = 'fused' if one_lane else 'loop'
        net = self.device(tuple(tof_terms), None)
        if desc is not None and not isinstance(desc, dict):
            n = max(self._n(T, p), int(desc.shape[1]))
        else:
            n = self._n(*([T, p] + (list(desc.values()) if desc else [])))
        for x in (y0, inflow):
            if x is not None and np.ndim(x) == 2:
                n = max(n, np.shape(x)[1])
        T, p, d, fx, y0, inflow = self._inputs(net, plan, n, T, p, desc, y0, fix, inflow)
        times = self.params['times'] or [0.0, 1.0e4]
        t0 = times[0]
        t_end = times[-1] if t_end is None else t_end
        if steady:
            rtol = STEADY_TRANSIENT[0] if rtol is None else rtol
            atol = STEADY_TRANSIENT[1] if atol is None else atol
        if isinstance(root_dist, str):
            if root_dist != 'auto':
                raise ValueError("root_dist must be 'auto' or a number in [0, 1)")
            root_dist = ROOT_DIST if (steady and t_end > t0) else 0.0
        if isinstance(screen, str):
            if screen != 'auto':
                raise ValueError("screen must be 'auto', None or an rtol")
            screen = SCREEN_RTOL if (steady and root_dist > 0.0 and net.NDYN <= SCREEN_MAX_LANE_SPECIES) else None
        out = net.solve_cascade(n, T, p, y0, cells, d, fx, inflow, start=start, method=method, profile=profile,
                                t0=t0, t_end=t_end,
                                rtol=self.params['rtol'] if rtol is None else rtol,
                                atol=self.params['atol'] if atol is None else atol,
                                max_steps=max_steps, newton=steady, newton_iters=newton_iters,
                                root_dist=float(root_dist) if steady else 0.0,
                                screen=(float(screen), SCREEN_MARGIN) if (steady and screen) else None,
                                wave_order=-1)
        torch = net.torch
        tin = torch.as_tensor(np.asarray(inflow, float), dtype=torch.float64, device='cuda') \
            if not torch.is_tensor(inflow) else inflow.to(dtype=torch.float64, device='cuda')
        if tin.dim() == 1:
            tin = tin[:, None].expand(len(plan.dyn), n)
        out['conversion'] = {}
        for i, name in enumerate(plan.dyn):
            if flow[i] != 0.0 and bool((tin[i] > 0.0).all()):
                out['conversion'][name] = 1.0 - out['y'][i] / tin[i]
        if to_numpy:
            return {k: ({s: v.cpu().numpy() for s, v in x.items()} if isinstance(x, dict) else x.cpu().numpy())
                    for k, x in out.items()}
        return out

    def drc_batch(self, tof_terms, T=None, p=None, desc=None, eps=1.0e-3, steady=False, t_end=None, rtol=None,
                  atol=None, max_steps=200000, y0=None, fix=None, inflow=None, screen='auto', method='fd', adjoint_kernel='group'):
        """Degree of rate control of every reaction (old_system.py:490-515) for a batch.
        steady=True: each of the 2R+1 solves is a steady-state solve with
        solve_batch's rule (STEADY_TRANSIENT unless rtol / atol are given;
        the root where the transient has reached it to ROOT_DIST, else the
        transient end: the condition's status is then 4).  `screen`: as in
        solve_batch (each of the 2R+1 solves screened on its own).

        method='fd' (the default) is the reference's central difference over
        k_j (1 +- eps).  method='analytic' (steady=True only) takes one steady
        solve and one adjoint solve of the steady Jacobian per condition
        instead of 2R+1 solves (pck_drc_adjoint; DESIGN.md "Analytic DRC"):
        xi_j = d ln TOF / d ln k_j at fixed K_j, the eps -> 0 limit of the
        reference's definition, so it differs from an eps = 5e-2 run by
        O(eps^2).  `eps` is ignored for 'analytic'.  A condition whose solve
        did not report a reached root keeps that status (4, ...) and gets NaN
        xi: a transient end has no implicit-function sensitivity; status 7: a
        singular steady Jacobian.  `screen` then applies to the one solve.
        `adjoint_kernel` ('analytic' only): as in drc_at.

        Returns {reaction name: xi [n]} (ghost reactions: 0) plus 'tof0', 'status'
        and 'nsteps'."""
        self._refuse_pfr('drc_batch', 'cascade_drc_batch', 'analyses')
        if method not in ('fd', 'analytic'):
            raise ValueError("method must be 'fd' or 'analytic', not %r" % (method,))
        if method == 'analytic' and not steady:
            raise ValueError("method='analytic' needs steady=True: the analytic degree of rate control is "
                             "the sensitivity of a steady state")
        mode = self._adjoint_mode(adjoint_kernel)
        plan = self.plan(tuple(tof_terms), None)
        net = self.device(tuple(tof_terms), None)
        if method == 'analytic':
            net.set_sens_lanes(mode)
        n = self._n(T, p, *(desc.values() if desc else []))
        for a in (y0, fix, inflow):
            if a is not None and np.ndim(a) == 2:
                n = max(n, np.shape(a)[1])
        T, p, d, fx, y0, inflow = self._inputs(net, plan, n, T, p, desc, y0, fix, inflow)
        times = self.params['times'] or [0.0, 1.0e4]
        if steady:
            rtol = STEADY_TRANSIENT[0] if rtol is None else rtol
            atol = STEADY_TRANSIENT[1] if atol is None else atol
        if isinstance(screen, str):
            if screen != 'auto':
                raise ValueError("screen must be 'auto', None or an rtol")
            screen = SCREEN_RTOL if (steady and net.NDYN <= SCREEN_MAX_LANE_SPECIES) else None
        run = net.drc_adjoint if method == 'analytic' else net.drc
        r = run(n, T, p, y0, d, fx, inflow, t0=times[0], t_end=times[-1] if t_end is None else t_end,
                rtol=self.params['rtol'] if rtol is None else rtol,
                atol=self.params['atol'] if atol is None else atol, max_steps=max_steps, newton=steady,
                drc_eps=eps, root_dist=ROOT_DIST if steady else 0.0,
                screen=(float(screen), SCREEN_MARGIN) if (steady and screen) else None)
        return self._drc_dict(plan, r, n)

    def _drc_dict(self, plan, r, n):
        xi = r['xi'].cpu().numpy()
        out = {name: (xi[plan.reactions.index(name)] if name in plan.reactions else np.zeros(n))
               for name in plan.all_reactions}
        out['tof0'] = r['tof0'].cpu().numpy()
        out['status'] = r['status'].cpu().numpy()
        if 'nsteps' in r:
            out['nsteps'] = r['nsteps'].cpu().numpy()
        return out

    @staticmethod
    def _adjoint_mode(adjoint_kernel):
        """pck_network_set_sens_lanes' / pck_network_set_multi_lanes' mode of
        adjoint_kernel = 'group' | 'lane' | 'auto'."""
        if not isinstance(adjoint_kernel, str) or adjoint_kernel not in _L.SENS_LANES_MODES:
            raise ValueError("adjoint_kernel must be 'group', 'lane' or 'auto', not %r" % (adjoint_kernel,))
        return _L.SENS_LANES_MODES[adjoint_kernel]

    def drc_at(self, tof_terms, Y, T=None, p=None, desc=None, fix=None, inflow=None, status_in=None, k=None,
               adjoint_kernel='group'):
        """Analytic degree of rate control (drc_batch's method='analytic') at
        given steady states Y [n_dynamic, n] in plan.dyn order -- solve_batch's
        'y' -- without a solve (pck_drc_at).  The states are taken as steady.
        status_in ([n], optional): only its 0 rows are computed, the others
        keep their status and get NaN xi.  k = (kf, kr) [active reactions, n]:
        rate constants to use instead of the network's own at (T, p, desc).
        adjoint_kernel: 'group' (16, 32 or 64 lanes per condition, the
        default), 'lane' (one lane per condition: networks of at most 8 dynamic
        species, a larger one raises) or 'auto' ('lane' where the network
        allows it); the two kernels agree to rounding (DESIGN.md "One-lane
        adjoint").
        Returns {reaction name: xi [n]} (ghost reactions: 0) plus 'tof0' and 'status'."""
        self._refuse_pfr('drc_at', 'cascade_drc_batch', 'analyses')
        mode = self._adjoint_mode(adjoint_kernel)
        plan = self.plan(tuple(tof_terms), None)
        net = self.device(tuple(tof_terms), None)
        net.set_sens_lanes(mode)
        Y = np.asarray(Y, float)
        if Y.ndim == 1:
            Y = Y[:, None]
        if Y.shape[0] != net.NDYN:
            raise ValueError('Y has %d rows for %d dynamic species' % (Y.shape[0], net.NDYN))
        n = Y.shape[1]
        T, p, d, fx, _, inflow = self._inputs(net, plan, n, T, p, desc, None, fix, inflow)
        kf, kr = net.rate_constants(n, T, p, d) if k is None else k
        return self._drc_dict(plan, net.drc_at(n, T, p, Y, kf, kr, d, fx, inflow, status_in), n)

    # -- multi-objective DRC (DESIGN.md "Multi-objective DRC") ----------------------------
    @staticmethod
    def _objectives(plan, objectives):
        """(labels, wr [K, active reactions], wy [K, dynamic species]) of a list
        of objectives: a str names a dynamic species (its coverage / state
        variable), a tuple or list of reaction names is the sum of their net
        rates (a name given twice counts twice, as in tof_terms), a dict
        {'rates': {name: w}, 'species': {name: w}} any weighted mix.  Host work
        only; ValueError names the offender."""
        if isinstance(objectives, (str, dict)):
            objectives = [objectives]
        objectives = list(objectives)
        if not objectives:
            raise ValueError('no objectives')
        K = len(objectives)
        wr, wy, labels = np.zeros((K, len(plan.reactions))), np.zeros((K, len(plan.dyn))), []

        def rate(m, name, w):
            if name not in plan.reactions:
                what = 'not an active reaction' if name in plan.all_reactions else 'an unknown reaction'
                raise ValueError('objective %d: %r is %s' % (m, name, what))
            wr[m, plan.reactions.index(name)] += float(w)

        def species(m, name, w):
            if name in plan.fix:
                raise ValueError('objective %d: %r is a fixed species; only a dynamic species has a sensitivity' % (m, name))
            if name not in plan.dyn:
                raise ValueError('objective %d: %r is an unknown species' % (m, name))
            wy[m, plan.dyn.index(name)] += float(w)

        for m, ob in enumerate(objectives):
            if isinstance(ob, str):
                species(m, ob, 1.0)
                labels.append(ob)
            elif isinstance(ob, (tuple, list)):
                for name in ob:
                    if not isinstance(name, str):
                        raise ValueError('objective %d: %r is not a reaction name' % (m, name))
                    rate(m, name, 1.0)
                labels.append('+'.join(ob))
            elif isinstance(ob, dict):
                extra = set(ob) - {'rates', 'species', 'label'}
                if extra:
                    raise ValueError("objective %d: unknown keys %s (expected 'rates', 'species', 'label')"
                                     % (m, sorted(extra)))
                for name, w in (ob.get('rates') or {}).items():
                    rate(m, name, w)
                for name, w in (ob.get('species') or {}).items():
                    species(m, name, w)
                labels.append(str(ob['label']) if 'label' in ob else ' + '.join(
                    ['%g %s' % (w, nm) for nm, w in (ob.get('rates') or {}).items()] +
                    ['%g [%s]' % (w, nm) for nm, w in (ob.get('species') or {}).items()]))
            else:
                raise ValueError('objective %d: %r is neither a species name, a list of reaction names nor a dict'
                                 % (m, ob))
            if not (wr[m].any() or wy[m].any()):
                raise ValueError('objective %d (%r) is empty: every weight is zero' % (m, ob))
        return labels, wr, wy

    def _multi_dict(self, plan, labels, r, n):
        xi = r['xi'].cpu().numpy()
        K = xi.shape[0]
        full = np.zeros((K, len(plan.all_reactions), n))
        for j, name in enumerate(plan.all_reactions):
            if name in plan.reactions:
                full[:, j] = xi[:, plan.reactions.index(name)]
        out = dict(labels=list(labels), reactions=list(plan.all_reactions), val=r['val'].cpu().numpy(), xi=full,
                   status=r['status'].cpu().numpy(), ostatus=r['ostatus'].cpu().numpy())
        if 'nsteps' in r:
            out['nsteps'] = r['nsteps'].cpu().numpy()
        return out

    def drc_objectives_at(self, objectives, Y, T=None, p=None, desc=None, fix=None, inflow=None, status_in=None,
                          k=None, adjoint_kernel='group'):
        """The analytic degree of rate control of several objectives at given
        steady states Y [n_dynamic, n] (plan.dyn order), from one factorisation
        of the steady Jacobian and one adjoint solve per objective
        (pck_drc_multi_at; DESIGN.md "Multi-objective DRC").  An objective is a
        str (a dynamic species: its coverage, or a CSTR's outlet concentration),
        a tuple / list of reaction names (the sum of their net rates, as
        tof_terms) or a dict {'rates': {name: w}, 'species': {name: w}}; an
        unknown name, a fixed species or an empty objective raises ValueError.
        The objectives are data of the call: the plan without TOF terms serves
        all of them, and changing them never rebuilds a network.  T, p, desc,
        fix, inflow, status_in and k as in drc_at.  adjoint_kernel: 'group' (16,
        32 or 64 lanes per condition, the default), 'lane' (one lane per
        condition: networks of at most 8 dynamic species, a larger one raises)
        or 'auto' ('lane' where the network allows it); a choice of its own,
        independent of drc_at's; the two kernels agree to rounding (DESIGN.md
        "Multi-objective DRC, one lane").
        Returns dict(labels [K], reactions [R] (every reaction; ghost reactions
        get 0), val [K, n] (the objectives' values), xi [K, R, n]
        (d ln J_m / d ln k_j at fixed K_j), status [n], ostatus [K, n] (3: a
        zero or non-finite objective, NaN xi for it alone))."""
        self._refuse_pfr('drc_objectives_at', 'cascade_drc_batch', 'analyses')
        mode = self._adjoint_mode(adjoint_kernel)
        plan = self.plan((), None)
        labels, wr, wy = self._objectives(plan, objectives)
        net = self.device((), None)
        net.set_multi_lanes(mode)
        Y = np.asarray(Y, float)
        if Y.ndim == 1:
            Y = Y[:, None]
        if Y.shape[0] != net.NDYN:
            raise ValueError('Y has %d rows for %d dynamic species' % (Y.shape[0], net.NDYN))
        n = Y.shape[1]
        T, p, d, fx, _, inflow = self._inputs(net, plan, n, T, p, desc, None, fix, inflow)
        kf, kr = net.rate_constants(n, T, p, d) if k is None else k
        r = net.drc_multi_at(n, T, p, Y, kf, kr, wr, wy, d, fx, inflow, status_in)
        return self._multi_dict(plan, labels, r, n)

    def drc_objectives_batch(self, objectives, T=None, p=None, desc=None, t_end=None, rtol=None, atol=None,
                             max_steps=200000, y0=None, fix=None, inflow=None, screen='auto',
                             adjoint_kernel='group'):
        """drc_objectives_at at the steady states of one steady solve per
        condition (pck_drc_multi_adjoint): the arguments of
        drc_batch(steady=True, method='analytic').  A condition whose solve did
        not report a reached root keeps that status and gets NaN xi.
        adjoint_kernel: as in drc_objectives_at.  Returns what
        drc_objectives_at returns plus 'nsteps'."""
        self._refuse_pfr('drc_objectives_batch', 'cascade_drc_batch', 'analyses')
        mode = self._adjoint_mode(adjoint_kernel)
        plan = self.plan((), None)
        labels, wr, wy = self._objectives(plan, objectives)
        net = self.device((), None)
        net.set_multi_lanes(mode)
        n = self._n(T, p, *(desc.values() if desc else []))
        for a in (y0, fix, inflow):
            if a is not None and np.ndim(a) == 2:
                n = max(n, np.shape(a)[1])
        T, p, d, fx, y0, inflow = self._inputs(net, plan, n, T, p, desc, y0, fix, inflow)
        times = self.params['times'] or [0.0, 1.0e4]
        rtol = STEADY_TRANSIENT[0] if rtol is None else rtol
        atol = STEADY_TRANSIENT[1] if atol is None else atol
        if isinstance(screen, str):
            if screen != 'auto':
                raise ValueError("screen must be 'auto', None or an rtol")
            screen = SCREEN_RTOL if net.NDYN <= SCREEN_MAX_LANE_SPECIES else None
        r = net.drc_multi_adjoint(n, T, p, y0, wr, wy, d, fx, inflow, t0=times[0],
                                  t_end=times[-1] if t_end is None else t_end, rtol=rtol, atol=atol,
                                  max_steps=max_steps, newton=True, root_dist=ROOT_DIST,
                                  screen=(float(screen), SCREEN_MARGIN) if screen else None)
        return self._multi_dict(plan, labels, r, n)

    def _objectives_run(self, objectives, Y, k, status_in, kw):
        if Y is not None:
            return self.drc_objectives_at(objectives, Y, k=k, status_in=status_in, **kw)
        if k is not None or status_in is not None:
            raise ValueError('k and status_in go with given states Y')
        return self.drc_objectives_batch(objectives, **kw)

    def selectivity_control_batch(self, num_terms, den_terms, Y=None, k=None, status_in=None, **kw):
        """Degree of selectivity control d ln (r_num / r_den) / d ln k_j =
        xi_num - xi_den, with r_num and r_den sums of net rates (reaction names
        as tof_terms): the two objectives of one launch, so one factorisation.
        kw as for drc_objectives_batch; with Y (and optionally k, status_in),
        at those states as drc_objectives_at.  adjoint_kernel = 'group' |
        'lane' | 'auto' (in kw) chooses the kernel as in drc_objectives_at.
        Returns dict(reactions [R], dsc [R, n], selectivity [n], status [n] (the
        condition's, or 3 where either rate is zero or not finite), xi_num,
        xi_den [R, n], val_num, val_den [n])."""
        r = self._objectives_run([tuple(num_terms), tuple(den_terms)], Y, k, status_in, kw)
        st = np.where(r['status'] != 0, r['status'], r['ostatus'].max(axis=0))
        out = dict(reactions=r['reactions'], dsc=r['xi'][0] - r['xi'][1], selectivity=r['val'][0] / r['val'][1],
                   status=st, xi_num=r['xi'][0], xi_den=r['xi'][1], val_num=r['val'][0], val_den=r['val'][1])
        if 'nsteps' in r:
            out['nsteps'] = r['nsteps']
        return out

    def coverage_control_batch(self, species=None, Y=None, k=None, status_in=None, **kw):
        """Degree of coverage control d ln y_i / d ln k_j of the dynamic species
        `species` (None: every dynamic species, plan.dyn order) -- for a CSTR's
        gas species the control of its outlet concentration: len(species)
        objectives of one launch.  kw (adjoint_kernel = 'group' | 'lane' |
        'auto' among them), Y, k, status_in as in selectivity_control_batch.
        Returns dict(species, reactions [R], dcc [len(species), R, n], coverage
        [len(species), n], status [n], ostatus [len(species), n] (3: a species
        at exactly 0, NaN dcc for it alone))."""
        if species is None:
            species = list(self.plan((), None).dyn)
        elif isinstance(species, str):
            species = [species]
        for s in species:
            if not isinstance(s, str):
                raise ValueError('%r is not a species name' % (s,))
        r = self._objectives_run(list(species), Y, k, status_in, kw)
        out = dict(species=list(species), reactions=r['reactions'], dcc=r['xi'], coverage=r['val'],
                   status=r['status'], ostatus=r['ostatus'])
        if 'nsteps' in r:
            out['nsteps'] = r['nsteps']
        return out

    # -- adjoint sensitivities (DESIGN.md "Adjoint sensitivities") ------------------------
    def _dlnk_dT(self, net, n, T, p, d):
        """(d ln kf / dT, d ln kr / dT) [NRXN, n] on the device: the 5-point
        central stencil of the network's rate constants at h = 1e-3 T (four
        launches), 0 where a rate constant is 0."""
        torch = net.torch
        if torch.is_tensor(T):
            Tn = T.to(dtype=torch.float64, device='cuda').reshape(-1).expand(n)
        else:
            Tn = torch.as_tensor(np.broadcast_to(np.asarray(T, float), (n,)).copy(), dtype=torch.float64, device='cuda')
        hh = 1.0e-3 * Tn
        acc = [0.0, 0.0]
        live = [None, None]
        for m, w in ((-2.0, 1.0), (-1.0, -8.0), (1.0, 8.0), (2.0, -1.0)):
            k = net.rate_constants(n, Tn + m * hh, p, d)
            for q in (0, 1):
                acc[q] = acc[q] + w * torch.log(k[q])
                live[q] = k[q] > 0.0
        zero = torch.zeros((), dtype=torch.float64, device='cuda')
        return tuple(torch.where(live[q], acc[q] / (12.0 * hh), zero) for q in (0, 1))

    def _eapp_check(self, plan):
        if any(k.startswith('@T:') for k in plan.descriptors):
            raise ValueError('apparent activation energy: the plan has temperature-keyed user energies (%s); a '
                             'tabulated energy has no temperature derivative'
                             % ', '.join(k for k in plan.descriptors if k.startswith('@T:')))
        ns = len(plan.dyn)
        off = int(plan.ip[_L.I_HDR + _L.D_DYN])
        dyn = np.asarray(plan.dp[off: off + 4 * ns]).reshape(ns, 4)
        if np.any(dyn[:, 2] != 0.0):
            raise ValueError('apparent activation energy: the row scale of this reactor depends on T (the CSTR\'s '
                             'gas rows); its term is not implemented')

    def dlnk_dT_batch(self, T=None, p=None, desc=None):
        """(a, c) = (d ln kf / dT, d ln kr / dT), [active reactions, n] device
        tensors, at fixed p and descriptors: the direction whose sensitivity
        is d ln TOF / dT (sensitivity_batch's eapp).  5-point central stencil
        of the rate constants at h = 1e-3 T; 0 where a rate constant is 0
        (irreversible steps).  Refuses temperature-keyed ('@T:') plans."""
        plan = self.plan((), None)
        net = self.device((), None)
        if any(k.startswith('@T:') for k in plan.descriptors):
            raise ValueError('dlnk_dT_batch: a temperature-keyed user energy has no temperature derivative')
        n = self._n(T, p, *(desc or {}).values()) if desc else self._n(T, p)
        T, p, d, _, _, _ = self._inputs(net, plan, n, T, p, desc, None, None, None)
        return self._dlnk_dT(net, n, T, p, d)

    def _sens_dict(self, plan, r, n, T, eapp):
        """The device dict of sens_at / sens_adjoint by name, on the host."""
        h = {k: v.cpu().numpy() for k, v in r.items()}
        out = {}
        for key in ('xi', 'sf', 'sr'):
            out[key] = {name: (h[key][plan.reactions.index(name)] if name in plan.reactions else np.zeros(n))
                        for name in plan.all_reactions}
        out['order'] = {name: h['order'][q] for q, name in enumerate(plan.fix)}
        off = int(plan.ip[_L.I_HDR + _L.D_DYN])
        flow = np.asarray(plan.dp[off: off + 4 * len(plan.dyn)]).reshape(len(plan.dyn), 4)[:, 3]
        out['order_inflow'] = {name: h['order_in'][i] for i, name in enumerate(plan.dyn) if flow[i] != 0.0}
        nd = h['dir'].shape[0] - (1 if eapp else 0)
        out['dir'] = h['dir'][:nd]
        if eapp:
            Tn = np.broadcast_to(np.asarray(T, float), (n,))
            out['eapp'] = R * Tn * Tn * h['dir'][nd]
        for key in ('tof0', 'status', 'err', 'nsteps'):
            if key in h:
                out[key] = h[key]
        return out

    def _sens_directions(self, net, plan, n, T, p, d, directions, eapp):
        """User directions [ND, R, n] (or None) plus, last, d ln k / dT for eapp."""
        torch = net.torch
        a = c = None
        if directions is not None:
            a, c = (torch.as_tensor(x, dtype=torch.float64, device='cuda') for x in directions)
            if a.dim() == 2:
                a, c = a[None], c[None]
            if tuple(a.shape) != (a.shape[0], net.NRXN, n) or tuple(c.shape) != tuple(a.shape):
                raise ValueError('directions: expected two [ND, %d, %d] arrays in plan.reactions order, got %s and %s'
                                 % (net.NRXN, n, tuple(a.shape), tuple(c.shape)))
        if eapp:
            ta, tc = self._dlnk_dT(net, n, T, p, d)
            a = ta[None] if a is None else torch.cat([a, ta[None]])
            c = tc[None] if c is None else torch.cat([c, tc[None]])
        return None if a is None else (a, c)

    def sensitivity_at(self, tof_terms, Y, T=None, p=None, desc=None, fix=None, inflow=None, status_in=None, k=None,
                       directions=None, err_max=1.0e-9, eapp=False, adjoint_kernel='group'):
        """First-order sensitivities of the TOF at given steady states Y
        [n_dynamic, n] (plan.dyn order), from the adjoint solve of the analytic
        degree of rate control (pck_sens_at) -- arguments as drc_at.  Returns
        a dict:
          'xi', 'sf', 'sr'  {reaction: [n]}: d ln TOF / d ln k_j at fixed K_j, and
                            d ln TOF / d ln kf_j, d ln TOF / d ln kr_j separately
                            (sf + sr = xi; ghost reactions 0)
          'order'           {fixed species: [n]}: d ln TOF / d ln (its concentration)
          'order_inflow'    {dynamic species with a flow term: [n]}: the order in
                            its inflow concentration (the CSTR)
          'dir'             [ND, n]: sum_j (a_mj sf_j + c_mj sr_j) for directions =
                            (a, c), [ND, active reactions, n] each in
                            plan.reactions order (d ln kf, d ln kr)
          'eapp'            [n] J/mol with eapp=True: R T^2 d ln TOF / dT at fixed
                            p, gas composition and descriptors (dlnk_dT_batch)
          'tof0', 'status', 'err' [n].
        A condition whose err = 2^-98 max rate / |TOF| exceeds err_max has
        status 8 and NaN everywhere but 'xi', 'tof0', 'err': double-double no
        longer resolves the per-direction numbers there (err_max <= 0: no
        guard).  adjoint_kernel: as in drc_at."""
        mode = self._adjoint_mode(adjoint_kernel)
        plan = self.plan(tuple(tof_terms), None)
        if eapp:
            self._eapp_check(plan)
        net = self.device(tuple(tof_terms), None)
        net.set_sens_lanes(mode)
        Y = np.asarray(Y, float)
        if Y.ndim == 1:
            Y = Y[:, None]
        if Y.shape[0] != net.NDYN:
            raise ValueError('Y has %d rows for %d dynamic species' % (Y.shape[0], net.NDYN))
        n = Y.shape[1]
        T, p, d, fx, _, inflow = self._inputs(net, plan, n, T, p, desc, None, fix, inflow)
        dirs = self._sens_directions(net, plan, n, T, p, d, directions, eapp)
        kf, kr = net.rate_constants(n, T, p, d) if k is None else k
        r = net.sens_at(n, T, p, Y, kf, kr, d, fx, inflow, status_in, directions=dirs, err_max=err_max)
        return self._sens_dict(plan, r, n, T, eapp)

    def sensitivity_batch(self, tof_terms, T=None, p=None, desc=None, steady=True, t_end=None, rtol=None, atol=None,
                          max_steps=200000, y0=None, fix=None, inflow=None, screen='auto', directions=None,
                          eapp=False, err_max=1.0e-9, adjoint_kernel='group'):
        """One steady solve per condition (drc_batch's rule and options) and
        sensitivity_at at its states, in two launches (pck_sens_adjoint).
        Returns sensitivity_at's dict plus 'nsteps'.  A condition whose solve
        did not report a reached root keeps that status (4, ...) and gets NaN.
        adjoint_kernel: as in drc_at."""
        if not steady:
            raise ValueError('sensitivity_batch needs steady=True: the adjoint sensitivities are those of a '
                             'steady state')
        mode = self._adjoint_mode(adjoint_kernel)
        plan = self.plan(tuple(tof_terms), None)
        if eapp:
            self._eapp_check(plan)
        net = self.device(tuple(tof_terms), None)
        net.set_sens_lanes(mode)
        n = self._n(T, p, *(desc.values() if desc else []))
        for a in (y0, fix, inflow):
            if a is not None and np.ndim(a) == 2:
                n = max(n, np.shape(a)[1])
        T, p, d, fx, y0, inflow = self._inputs(net, plan, n, T, p, desc, y0, fix, inflow)
        dirs = self._sens_directions(net, plan, n, T, p, d, directions, eapp)
        times = self.params['times'] or [0.0, 1.0e4]
        rtol = STEADY_TRANSIENT[0] if rtol is None else rtol
        atol = STEADY_TRANSIENT[1] if atol is None else atol
        if isinstance(screen, str):
            if screen != 'auto':
                raise ValueError("screen must be 'auto', None or an rtol")
            screen = SCREEN_RTOL if net.NDYN <= SCREEN_MAX_LANE_SPECIES else None
        r = net.sens_adjoint(n, T, p, y0, d, fx, inflow, directions=dirs, err_max=err_max, t0=times[0],
                             t_end=times[-1] if t_end is None else t_end, rtol=rtol, atol=atol, max_steps=max_steps,
                             newton=True, root_dist=ROOT_DIST,
                             screen=(float(screen), SCREEN_MARGIN) if screen else None)
        return self._sens_dict(plan, r, n, T, eapp)

    # -- linear stability (DESIGN.md "Linear stability") --------------------------------------
    @staticmethod
    def _eig_mode(eig_kernel):
        """the `lanes` argument of pck_stability_at / pck_stability of
        eig_kernel = 'group' | 'lane' | 'auto'."""
        if not isinstance(eig_kernel, str) or eig_kernel not in _L.EIG_LANES_MODES:
            raise ValueError("eig_kernel must be 'group', 'lane' or 'auto', not %r" % (eig_kernel,))
        return _L.EIG_LANES_MODES[eig_kernel]

    @staticmethod
    def _stability_dict(r, spectrum):
        out = {k: r[k].cpu().numpy() for k in _L.EIG_OUTPUTS}
        if spectrum:
            out['wr'], out['wi'] = r['wr'].cpu().numpy(), r['wi'].cpu().numpy()
        if 'nsteps' in r:
            out['nsteps'] = r['nsteps'].cpu().numpy()
        out['lanes'] = r['lanes']
        verdict = np.full(out['re_max'].shape, 'marginal', dtype='<U8')
        verdict[out['re_max'] < -out['scale']] = 'stable'
        verdict[out['re_max'] > out['scale']] = 'unstable'
        verdict[out['status'] != 0] = ''
        out['verdict'] = verdict
        return out

    def stability_at(self, Y, T=None, p=None, desc=None, fix=None, inflow=None, status_in=None, k=None, reduce=True,
                     eig_kernel='auto', spectrum=False, re_tol=0.0):
        """Linear stability of the states Y [n_dynamic, n] in plan.dyn order --
        solve_batch's 'y' -- without a solve (pck_stability_at): the
        eigenvalues of the Jacobian of every condition, on the device.
        reduce: the Jacobian restricted to the conservation class (n_dynamic -
        n_laws eigenvalues, no structural zero) instead of the full one (the
        reference's test, solver.py:102-106).  status_in, k as in drc_at.
        eig_kernel: 'lane' (one lane per condition, at most 8 eigenvalues),
        'group' (16, 32 or 64 lanes) or 'auto'.
        Returns dict(re_max, im_max, re_min, scale, n_pos (real part > re_tol),
        status, verdict, lanes) and, with spectrum, wr / wi [ns_eff, n].
        scale = ns_eff * eps * ||B||_F is the size of fp64 rounding in the
        eigenvalues: verdict is 'stable' where re_max < -scale, 'unstable'
        where re_max > scale, else 'marginal' (not resolved in fp64); '' for a
        condition whose status is not 0 (its numbers are NaN)."""
        mode = self._eig_mode(eig_kernel)
        plan = self.plan((), None)
        Y = np.asarray(Y, float)
        if Y.ndim == 1:
            Y = Y[:, None]
        if Y.ndim != 2 or Y.shape[0] != len(plan.dyn):
            raise ValueError('Y has shape %s for %d dynamic species' % (Y.shape, len(plan.dyn)))
        n = Y.shape[1]
        if status_in is not None and np.size(status_in) != n:
            raise ValueError('status_in has %d entries for %d conditions' % (np.size(status_in), n))
        if k is not None and any(tuple(np.shape(a)) != (len(plan.reactions), n) for a in k):
            raise ValueError('k = (kf, kr) must each have shape (%d, %d)' % (len(plan.reactions), n))
        net = self.device((), None)
        T, p, d, fx, _, inflow = self._inputs(net, plan, n, T, p, desc, None, fix, inflow)
        kf, kr = net.rate_constants(n, T, p, d) if k is None else k
        want = _L.EIG_OUTPUTS + (('wr', 'wi') if spectrum else ())
        r = net.stability_at(n, T, p, Y, kf, kr, d, fx, inflow, status_in, reduce=reduce, re_tol=re_tol, lanes=mode,
                             want=want)
        return self._stability_dict(r, spectrum)

    def stability_batch(self, T=None, p=None, desc=None, steady=True, t_end=None, rtol=None, atol=None,
                        max_steps=200000, y0=None, fix=None, inflow=None, screen='auto', reduce=True,
                        eig_kernel='auto', spectrum=False, re_tol=0.0):
        """One steady solve per condition (sensitivity_batch's rule and
        options) and stability_at at its states (pck_stability).  Returns
        stability_at's dict plus 'nsteps'.  A condition whose solve did not
        report a reached root keeps that status and gets NaN."""
        if not steady:
            raise ValueError('stability_batch needs steady=True: linear stability is that of a steady state')
        mode = self._eig_mode(eig_kernel)
        plan = self.plan((), None)
        net = self.device((), None)
        n = self._n(T, p, *(desc.values() if desc else []))
        for a in (y0, fix, inflow):
            if a is not None and np.ndim(a) == 2:
                n = max(n, np.shape(a)[1])
        T, p, d, fx, y0, inflow = self._inputs(net, plan, n, T, p, desc, y0, fix, inflow)
        times = self.params['times'] or [0.0, 1.0e4]
        rtol = STEADY_TRANSIENT[0] if rtol is None else rtol
        atol = STEADY_TRANSIENT[1] if atol is None else atol
        if isinstance(screen, str):
            if screen != 'auto':
                raise ValueError("screen must be 'auto', None or an rtol")
            screen = SCREEN_RTOL if net.NDYN <= SCREEN_MAX_LANE_SPECIES else None
        want = _L.EIG_OUTPUTS + (('wr', 'wi') if spectrum else ())
        r = net.stability(n, T, p, y0, d, fx, inflow, reduce=reduce, re_tol=re_tol, lanes=mode, want=want,
                          t0=times[0], t_end=times[-1] if t_end is None else t_end, rtol=rtol, atol=atol,
                          max_steps=max_steps, newton=True, root_dist=ROOT_DIST,
                          screen=(float(screen), SCREEN_MARGIN) if screen else None)
        return self._stability_dict(r, spectrum)

    # -- descriptor sensitivities (DESIGN.md "One-lane adjoint") ----------------------------
    @staticmethod
    def _desc_names(plan, names):
        """The descriptors to differentiate in: `names`, or every descriptor of
        the plan that is not temperature-keyed."""
        if names is None:
            return [k for k in plan.descriptors if not k.startswith('@T:')]
        names = [names] if isinstance(names, str) else [str(k) for k in names]
        for k in names:
            if k.startswith('@T:'):
                raise ValueError('descriptor %r is a temperature-keyed user energy: a tabulated energy is no '
                                 'descriptor to differentiate in' % (k,))
            if k not in plan.descriptors:
                raise ValueError('unknown descriptor %r (the plan has %s)'
                                 % (k, ', '.join(x for x in plan.descriptors if not x.startswith('@T:')) or 'none'))
        return names

    def _dlnk_ddesc(self, net, plan, n, T, p, d, names, h):
        """{name: (d ln kf / d desc, d ln kr / d desc)} [NRXN, n] on the device:
        the 5-point central stencil of the network's rate constants in that
        descriptor at the absolute step h (four launches per descriptor), 0
        where a rate constant is 0.  The twin of _dlnk_dT."""
        torch = net.torch
        dt = torch.as_tensor(d, dtype=torch.float64, device='cuda')
        zero = torch.zeros((), dtype=torch.float64, device='cuda')
        out = {}
        for name in names:
            q = list(plan.descriptors).index(name)
            acc = [0.0, 0.0]
            live = [None, None]
            for m, w in ((-2.0, 1.0), (-1.0, -8.0), (1.0, 8.0), (2.0, -1.0)):
                dm = dt.clone()
                dm[q] += m * h
                k = net.rate_constants(n, T, p, dm)
                for s in (0, 1):
                    acc[s] = acc[s] + w * torch.log(k[s])
                    live[s] = k[s] > 0.0
            out[name] = tuple(torch.where(live[s], acc[s] / (12.0 * h), zero) for s in (0, 1))
        return out

    def dlnk_ddesc_batch(self, names=None, T=None, p=None, desc=None, h=1.0e-3):
        """{descriptor: (a, c)} with (a, c) = (d ln kf / d desc, d ln kr / d desc),
        [active reactions, n] device tensors in 1/eV, at fixed T, p and the
        other descriptors: the directions whose sensitivity is d ln TOF / d
        desc (descriptor_sensitivity_batch).  5-point central stencil of the
        rate constants at the absolute step h (eV); 0 where a rate constant is
        0 (irreversible steps).  names=None: every descriptor of the plan that
        is not temperature-keyed; an '@T:' key or an unknown name raises
        ValueError.  The derivative is undefined where an energy clamp of the
        energy program (max(dGa, 0), the register clamps) switches within 2 h
        of the point: the stencil then straddles the kink."""
        plan = self.plan((), None)
        names = self._desc_names(plan, names)
        net = self.device((), None)
        n = self._n(T, p, *(desc or {}).values()) if isinstance(desc, dict) else \
            (max(self._n(T, p), int(desc.shape[1])) if desc is not None else self._n(T, p))
        T, p, d, _, _, _ = self._inputs(net, plan, n, T, p, desc, None, None, None)
        return self._dlnk_ddesc(net, plan, n, T, p, d, names, float(h))

    @staticmethod
    def _desc_sigma(names, desc_sigma):
        if desc_sigma is None:
            return None
        extra = [k for k in desc_sigma if k not in names]
        if extra:
            raise ValueError('desc_sigma has %s, not among the requested descriptors %s' % (extra, names))
        return {k: float(desc_sigma[k]) for k in names if k in desc_sigma}

    def _desc_sens_dict(self, plan, r, n, names, sigma):
        h = {k: v.cpu().numpy() for k, v in r.items()}
        out = {'dlntof_ddesc': {name: h['dir'][m] for m, name in enumerate(names)},
               'xi': {name: (h['xi'][plan.reactions.index(name)] if name in plan.reactions else np.zeros(n))
                      for name in plan.all_reactions}}
        for key in ('tof0', 'status', 'err', 'nsteps'):
            if key in h:
                out[key] = h[key]
        if sigma is not None:
            # first-order propagation of independent descriptor errors
            out['std_lntof'] = np.sqrt(sum((out['dlntof_ddesc'][k] * s) ** 2 for k, s in sigma.items()))
        return out

    def _desc_directions(self, net, plan, n, T, p, d, names, h):
        torch = net.torch
        ac = self._dlnk_ddesc(net, plan, n, T, p, d, names, h)
        return torch.stack([ac[k][0] for k in names]), torch.stack([ac[k][1] for k in names])

    def descriptor_sensitivity_at(self, tof_terms, Y, T=None, p=None, desc=None, fix=None, inflow=None,
                                  status_in=None, k=None, names=None, desc_sigma=None, err_max=1.0e-9,
                                  adjoint_kernel='auto', h=1.0e-3):
        """d ln TOF / d descriptor at given steady states Y [n_dynamic, n]
        (arguments as sensitivity_at): the (a, c) of dlnk_ddesc_batch stacked as
        directions of one adjoint solve (pck_sens_at).  Returns
          'dlntof_ddesc'   {descriptor: [n]} in 1/eV, for `names` (None: every
                           descriptor that is not temperature-keyed)
          'xi'             {reaction: [n]}
          'tof0', 'status', 'err' [n]
          'std_lntof'      [n] with desc_sigma = {descriptor: sigma in eV}:
                           sqrt(sum_d (dlntof_ddesc_d sigma_d)^2), the first-order
                           error bar of ln TOF for independent descriptor errors
        Guard and statuses as sensitivity_at: NaN gradients where the status
        is not 0.  The gradients inherit dlnk_ddesc_batch's caveat at energy
        clamps.  adjoint_kernel: as in drc_at ('auto': one lane per condition
        where the network allows it)."""
        mode = self._adjoint_mode(adjoint_kernel)
        plan = self.plan(tuple(tof_terms), None)
        names = self._desc_names(plan, names)
        sigma = self._desc_sigma(names, desc_sigma)
        if not names:
            raise ValueError('descriptor sensitivities: the network has no descriptor')
        net = self.device(tuple(tof_terms), None)
        net.set_sens_lanes(mode)
        Y = np.asarray(Y, float)
        if Y.ndim == 1:
            Y = Y[:, None]
        if Y.shape[0] != net.NDYN:
            raise ValueError('Y has %d rows for %d dynamic species' % (Y.shape[0], net.NDYN))
        n = Y.shape[1]
        T, p, d, fx, _, inflow = self._inputs(net, plan, n, T, p, desc, None, fix, inflow)
        dirs = self._desc_directions(net, plan, n, T, p, d, names, float(h))
        kf, kr = net.rate_constants(n, T, p, d) if k is None else k
        r = net.sens_at(n, T, p, Y, kf, kr, d, fx, inflow, status_in, directions=dirs, err_max=err_max)
        return self._desc_sens_dict(plan, r, n, names, sigma)

    def descriptor_sensitivity_batch(self, tof_terms, T=None, p=None, desc=None, names=None, desc_sigma=None,
                                     adjoint_kernel='auto', steady=True, t_end=None, rtol=None, atol=None,
                                     max_steps=200000, y0=None, fix=None, inflow=None, screen='auto',
                                     err_max=1.0e-9, h=1.0e-3):
        """One steady solve per condition (sensitivity_batch's rule and options)
        and descriptor_sensitivity_at at its states (pck_sens_adjoint): d ln TOF
        / d E_CO and d ln TOF / d E_O at every node of a volcano grid, and with
        desc_sigma the error bar they imply.  Returns
        descriptor_sensitivity_at's dict plus 'nsteps'."""
        if not steady:
            raise ValueError('descriptor_sensitivity_batch needs steady=True: the adjoint sensitivities are those '
                             'of a steady state')
        mode = self._adjoint_mode(adjoint_kernel)
        plan = self.plan(tuple(tof_terms), None)
        names = self._desc_names(plan, names)
        sigma = self._desc_sigma(names, desc_sigma)
        if not names:
            raise ValueError('descriptor sensitivities: the network has no descriptor')
        net = self.device(tuple(tof_terms), None)
        net.set_sens_lanes(mode)
        if desc is not None and not isinstance(desc, dict):
            n = max(self._n(T, p), int(desc.shape[1]))
        else:
            n = self._n(T, p, *(desc.values() if desc else []))
        for a in (y0, fix, inflow):
            if a is not None and np.ndim(a) == 2:
                n = max(n, np.shape(a)[1])
        T, p, d, fx, y0, inflow = self._inputs(net, plan, n, T, p, desc, y0, fix, inflow)
        dirs = self._desc_directions(net, plan, n, T, p, d, names, float(h))
        times = self.params['times'] or [0.0, 1.0e4]
        rtol = STEADY_TRANSIENT[0] if rtol is None else rtol
        atol = STEADY_TRANSIENT[1] if atol is None else atol
        if isinstance(screen, str):
            if screen != 'auto':
                raise ValueError("screen must be 'auto', None or an rtol")
            screen = SCREEN_RTOL if net.NDYN <= SCREEN_MAX_LANE_SPECIES else None
        r = net.sens_adjoint(n, T, p, y0, d, fx, inflow, directions=dirs, err_max=err_max, t0=times[0],
                             t_end=times[-1] if t_end is None else t_end, rtol=rtol, atol=atol, max_steps=max_steps,
                             newton=True, root_dist=ROOT_DIST,
                             screen=(float(screen), SCREEN_MARGIN) if screen else None)
        return self._desc_sens_dict(plan, r, n, names, sigma)

    # -- reference API (one condition) -------------------------------------------------
    def _full(self, plan, ydyn):
        """Dynamic state -> vector over all states in reference order."""
        order = plan.species
        y = np.zeros(len(order))
        pos = {s: i for i, s in enumerate(order)}
        if plan.formulation == 'patched':
            y[:] = self.initial_vector()
        else:
            for s, v in (self.start_state or {}).items():
                y[pos[s]] = v
        for i, s in enumerate(plan.dyn):
            y[pos[s]] = ydyn[i]
        return y

    def output_times(self):
        """old_system.py:363-368: [0] + nsteps log-spaced times from times[0]
        (1e-8 if 0) to times[-1] -- the reference's `ode` path output grid.
        The `solve_ivp` path stores every BDF step instead (old_system.py:350-358),
        which no other integrator reproduces; it gets the same grid here."""
        t0, t1 = float(self.params['times'][0]), float(self.params['times'][-1])
        n = int(self.params['nsteps'])
        out = np.concatenate((np.zeros(1), np.logspace(np.log10(t0 if t0 else 1.0e-8), np.log10(t1), num=n,
                                                        endpoint=True)))
        # 10**log10(t1) can land one ulp above t1 (7200 -> 7200.000000000001):
        # the last sample is the end of the integration, exactly
        out[-1] = t1
        return out

    def solve_odes(self):
        """old_system.py:315-383: integrate params['times'][0] -> [-1]; self.times /
        self.solution hold the state at output_times() (device dense output)."""
        self._refuse_pfr('solve_odes')
        plan = self.plan()
        times = self.output_times()
        inside = times[times >= float(self.params['times'][0])]
        r = self.solve_batch(T=[self.params['temperature']], t_out=inside)
        self._check(r['status'][0], 'solve_odes')
        traj = r['traj'][:, :, 0]
        sol = np.empty((times.size, len(plan.species)))
        sol[:times.size - inside.size] = self._full(plan, plan.y0_default)
        for k in range(inside.size):
            sol[times.size - inside.size + k] = self._full(plan, traj[k])
        self.times = times
        self.solution = sol
        return self.solution

    def write_results(self, path=''):
        """old_system.py:531-568: rates_/coverages_/pressures_<T>K_<p>bar.csv over
        self.times (forward and reverse rate of every reaction at each sample
        from one device launch of pck_reaction_rates)."""
        import os
        import pandas as pd
        if path != '' and not os.path.isdir(path):
            os.makedirs(path, exist_ok=True)
        plan = self.plan()
        T = self.params['temperature']
        p = self.params['pressure']
        tag = ('%1.1f' % T) + 'K_' + ('%1.1f' % (p / bartoPa)) + 'bar.csv'
        names = list(plan.species)
        st = self.states
        ads = [i for i, s in enumerate(names) if st[s].state_type in ('adsorbate', 'surface') and s in plan.dyn + plan.fix]
        gas = [i for i, s in enumerate(names) if st[s].state_type == 'gas' and s in plan.dyn + plan.fix]
        rates = self._rates_at(plan, self.solution)
        rheader = ['Time (s)'] + [x for r in self.reactions.values() for x in (r.name + '_fwd', r.name + '_rev')]
        times = self.times.reshape(-1, 1)
        pd.DataFrame(np.concatenate((times, rates), axis=1), columns=rheader).to_csv(path + 'rates_' + tag,
                                                                                     index=False)
        pd.DataFrame(np.concatenate((times, self.solution[:, ads]), axis=1),
                     columns=['Time (s)'] + [names[i] for i in ads]).to_csv(path + 'coverages_' + tag, index=False)
        pd.DataFrame(np.concatenate((times, self.solution[:, gas]), axis=1),
                     columns=['Time (s)'] + [names[i] for i in gas]).to_csv(path + 'pressures_' + tag, index=False)

    def _rates_at(self, plan, full_states):
        """[n_samples, 2 * n_reactions] (fwd, rev interleaved, reference order) at
        full state vectors (classic units), one pck_reaction_rates launch."""
        net = self.device()
        m = full_states.shape[0]
        pos = {s: i for i, s in enumerate(plan.species)}
        yd = np.stack([full_states[:, pos[s]] for s in plan.dyn]) if plan.dyn else np.zeros((0, m))
        fx = (np.stack([full_states[:, pos[s]] for s in plan.fix]) * plan.fix_conc_factor[:, None]
              if plan.fix else None)
        T = np.full(m, float(self.params['temperature']))
        Tt, p, d, _, _, _ = self._inputs(net, plan, m, T, None, None, None, None, None)
        kf, kr = net.rate_constants(m, Tt, p, d)
        rf, rr = net.reaction_rates(m, Tt, p, yd, kf, kr, d, fx)
        rf, rr = rf.cpu().numpy(), rr.cpu().numpy()
        out = np.zeros((m, 2 * len(plan.all_reactions)))
        for j, name in enumerate(plan.all_reactions):
            if name in plan.reactions:
                a = plan.reactions.index(name)
                out[:, 2 * j], out[:, 2 * j + 1] = rf[a], rr[a]
        return out

    def find_steady(self, *args, **kw):
        """old_system.py:385-468 find_steady(store_steady, plot_comparison, path) for
        formulation 'classic'; system.py:566-639 find_steady(max_iters, y0, method)
        -> SteadyStateResults for formulation 'patched'."""
        self._refuse_pfr('find_steady')
        if self.formulation == 'patched':
            return self.find_steady_state(*args, **kw)
        return self._find_steady_classic(*args, **kw)

    def _find_steady_classic(self, store_steady=False, plot_comparison=False, path=None):
        plan = self.plan()
        if self.solution is not None:
            pos = {s: i for i, s in enumerate(plan.species)}
            y0 = np.array([self.solution[-1][pos[s]] for s in plan.dyn])
        else:
            y0 = plan.y0_default
        r = self.solve_batch(T=[self.params['temperature']], y0=y0[:, None], t_end=self.params['times'][0],
                             t0=self.params['times'][0], steady=True)
        # status 4: a degenerate root; the reference's least_squares returns
        # wherever xtol stops it (old_system.py:426-433), the device returns
        # the transient end it started from -- never an error
        self._check(r['status'][0], 'find_steady', degenerate_ok=True)
        full = self._full(plan, r['y'][:, 0])
        if store_steady:
            self.full_steady = full
        return full

    @staticmethod
    def _check(st, what, degenerate_ok=False):
        """Raise on a failed solve (1 max steps, 2 step failure, 3 non-finite);
        status 4 (no steady state reached by t_end: the transient end is
        reported) and 5 (the same after a failed `retry` pass: the first
        pass's transient) are results where the reference's steady-state path
        would return one."""
        if st != 0 and not (degenerate_ok and st in (4, 5, 6)):
            raise RuntimeError('%s: device solver status %d (1 max steps, 2 step failure, 3 non-finite, '
                               '4 no steady state reached: transient end, 5 the same with the first-pass '
                               'transient, 6 a DRC mixing reached roots and transient ends, 7 a singular steady '
                               'Jacobian in the analytic DRC, 8 rates too large against the TOF for the '
                               'double-double adjoint sensitivities)' % (what, st))

    def reaction_terms(self, y):
        """old_system.py:202-225: rates (n_reactions, 2) at the full state y."""
        plan = self.plan()
        kf, kr = self.rate_constants_batch(T=[self.params['temperature']])
        pos = {s: i for i, s in enumerate(plan.species)}
        y = np.asarray(y, float).ravel()
        self.rates = np.zeros((len(plan.all_reactions), 2))
        for j, name in enumerate(plan.all_reactions):
            if name not in plan.reactions:
                continue
            a = plan.reactions.index(name)
            rx = self.reactions[name]
            rf, rr = kf[a, 0], kr[a, 0]
            for side, acc in ((rx.reactants, 0), (rx.products, 1)):
                v = rf if acc == 0 else rr
                for s in side:
                    if s.name in pos:
                        c = y[pos[s.name]]
                        if s.state_type == 'gas':
                            c = c * (bartoPa if plan.formulation == 'classic' else self.params['pressure'])
                        v *= c
                if acc == 0:
                    rf = v
                else:
                    rr = v
            self.rates[j] = (rf, rr)
        return self.rates

    def run_and_return_tof(self, tof_terms, ss_solve=False):
        """old_system.py:470-488"""
        r = self.solve_batch(T=[self.params['temperature']], tof_terms=tuple(tof_terms), steady=ss_solve)
        self._check(r['status'][0], 'run_and_return_tof', degenerate_ok=True)
        return float(r['tof'][0])

    def activity(self, tof_terms, ss_solve=False):
        """old_system.py:517-529 (eV)"""
        r = self.solve_batch(T=[self.params['temperature']], tof_terms=tuple(tof_terms), steady=ss_solve,
                             activity=True)
        self._check(r['status'][0], 'activity', degenerate_ok=True)
        return float(r['tof'][0])

    def degree_of_rate_control(self, tof_terms, ss_solve=False, eps=1.0e-3, method='fd'):
        """old_system.py:490-515.  method='analytic' (with ss_solve): drc_batch's
        analytic route, eps ignored; a condition that has not reached a
        steady state then has NaN xi.  As the reference's (whose ss_solve path
        returns wherever least_squares stops), a condition whose transient has
        not reached a steady state (status 4) still returns its xi: every TOF
        of the central difference is then that solve's answer by
        solve_batch's rule (a root reached, or the transient end at t_end)."""
        r = self.drc_batch(tof_terms, T=[self.params['temperature']], eps=eps, steady=ss_solve, method=method)
        self._check(r['status'][0], 'degree_of_rate_control', degenerate_ok=True)
        if r['status'][0] == 6:
            import warnings
            warnings.warn('degree_of_rate_control: the perturbed solves fall on both sides of the steady rule '
                          '(some reached a root, some report the transient end at t_end): the central '
                          'differences mix the two and xi measures the rule switching (status 6)')
        return {k: float(r[k][0]) for k in self.reactions}

    def reaction_orders(self, tof_terms, ss_solve=True):
        """{fixed species: d ln TOF / d ln (its pressure)} plus the inflow orders of
        a CSTR's gas species, at the System's temperature and pressure
        (sensitivity_batch; modelled on degree_of_rate_control(method='analytic')).
        Raises where the condition is flagged (no steady state reached, a
        singular Jacobian, status 8: not resolvable in double-double)."""
        if not ss_solve:
            raise ValueError('reaction_orders needs ss_solve=True: the orders are those of a steady state')
        r = self.sensitivity_batch(tof_terms, T=[self.params['temperature']])
        self._check(r['status'][0], 'reaction_orders')
        out = {k: float(v[0]) for k, v in r['order'].items()}
        out.update({k: float(v[0]) for k, v in r['order_inflow'].items()})
        return out

    def apparent_activation_energy(self, tof_terms):
        """R T^2 d ln TOF / dT (J/mol) of the steady state at the System's
        temperature and pressure, at fixed gas composition
        (sensitivity_batch(eapp=True)).  Raises where the condition is flagged."""
        r = self.sensitivity_batch(tof_terms, T=[self.params['temperature']], eapp=True)
        self._check(r['status'][0], 'apparent_activation_energy')
        return float(r['eapp'][0])

    # patched-API steady state (system.py:566-639)
    def find_steady_state(self, max_iters=30, y0=None, method=None):
        """system.py:566-639.  The reference restarts scipy `root` from a random
        guess until the surface rates vanish and the sites sum to one; here the
        guess (y0, or the start state: deterministic) is first integrated to
        params['times'][-1] (1e6 s when no times are set) so that Newton
        starts in the basin of the stable root, then polished."""
        plan = self.plan()
        yd = plan.y0_default if y0 is None else np.asarray(y0, float)[len(plan.fix):]
        times = self.params.get('times')
        t_end = float(times[-1]) if times is not None and len(times) else 1.0e6
        r = self.solve_batch(T=[self.params['temperature']], y0=np.asarray(yd)[:, None],
                             t0=0.0, t_end=t_end, steady=True, newton_iters=max(int(max_iters), 60))
        x = np.concatenate([plan.fix_default, r['y'][:, 0]])
        return SteadyStateResults(x, bool(r['status'][0] == 0))
