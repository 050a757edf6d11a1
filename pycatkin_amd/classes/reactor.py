"""Reactor classes with the reference's constructors (pycatkin/classes/reactor.py).

On the device a reactor is three per-species coefficients of the dynamic
rows: rowscale = rs0 + rs_T*T, a flow rate and a concentration factor
(pycatkin_amd/network.py builds them).  These classes only carry the inputs.
"""
from ..constants.physical_constants import bartoPa, kB


class Reactor:
    """reactor.py:8-86"""

    def __init__(self, name='reactor', volume=None, catalyst_area=None, residence_time=None, flow_rate=None,
                 path_to_pickle=None):
        if path_to_pickle:
            raise NotImplementedError('pickled reactors are not loaded (no unpickling of external files)')
        self.name = name
        self.volume = volume
        self.catalyst_area = catalyst_area
        self.residence_time = residence_time
        self.flow_rate = flow_rate
        self.scaling = None
        self.is_adsorbate = None
        self.is_gas = None
        self.dynamic_indices = None

    def set_scaling(self, T):
        """reactor.py:34-41"""
        self.scaling = kB * T * self.catalyst_area / self.volume

    def set_indices(self, is_adsorbate, is_gas):
        self.is_adsorbate = list(is_adsorbate)
        self.is_gas = list(is_gas)

    def get_dynamic_indices(self, adsorbate_indices, gas_indices):
        self.dynamic_indices = list(adsorbate_indices)
        return self.dynamic_indices

    # device coefficients for a dynamic species: (rowscale0, rowscale_T, flow_rate)
    def row_coefficients(self, is_adsorbate):
        return (1.0, 0.0, 0.0) if is_adsorbate else (0.0, 0.0, 0.0)


class InfiniteDilutionReactor(Reactor):
    """reactor.py:89-122: gas pressures are boundary conditions."""


class CSTReactor(Reactor):
    """reactor.py:125-189: gas rows scaled by kB*T*A/V/bartoPa plus flow."""

    def __init__(self, name='reactor', volume=None, catalyst_area=None, residence_time=None, flow_rate=None):
        super().__init__(residence_time=residence_time, flow_rate=flow_rate, volume=volume,
                         catalyst_area=catalyst_area, name=name)
        if self.residence_time is None:
            assert self.flow_rate is not None and self.volume is not None
            self.residence_time = self.volume / self.flow_rate

    def get_dynamic_indices(self, adsorbate_indices, gas_indices):
        self.dynamic_indices = list(adsorbate_indices) + list(gas_indices)
        return self.dynamic_indices

    def row_coefficients(self, is_adsorbate):
        if is_adsorbate:
            return (1.0, 0.0, 0.0)
        return (0.0, kB * self.catalyst_area / self.volume / bartoPa, 1.0 / self.residence_time)


class PFReactor(CSTReactor):
    """A catalyst bed as `cells` equal CSTR cells in series (tanks in series):
    the outlet gas of cell k is the inflow of cell k+1.  volume, catalyst_area
    and residence_time (or flow_rate) describe the whole bed; the device
    coefficients are one cell's.  Solved by System.solve_cascade_batch."""

    def __init__(self, name='reactor', volume=None, catalyst_area=None, residence_time=None, flow_rate=None, cells=1):
        super().__init__(name=name, volume=volume, catalyst_area=catalyst_area, residence_time=residence_time,
                         flow_rate=flow_rate)
        if int(cells) != cells or int(cells) < 1:
            raise ValueError('PFReactor: cells must be an integer >= 1, not %r' % (cells,))
        self.cells = int(cells)

    def row_coefficients(self, is_adsorbate):
        if is_adsorbate:
            return (1.0, 0.0, 0.0)
        # a cell has 1/cells of the bed's volume, area and residence time:
        # A/V is the bed's, the flow rate is cells / residence_time
        return (0.0, kB * self.catalyst_area / self.volume / bartoPa, self.cells / self.residence_time)
