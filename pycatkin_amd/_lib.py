"""ctypes binding of the C-ABI in include/pycatkin_amd.h (libpycatkin_amd.so).

This is the ONLY compute path of the package: there is no CPU fallback.  If
the shared library is missing or the process has no HIP device the calls
raise instead of silently computing something else.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# PCK_LIB selects an alternative in-tree build (A/B experiments of tools/ab_variants.sh)
LIB_PATH = os.environ.get('PCK_LIB') or os.path.join(_HERE, 'libpycatkin_amd.so')

# symbols declared in include/pycatkin_amd.h (checked by tests/test_capi.py)
EXPORTED = ('pck_abi_version', 'pck_last_error', 'pck_network_create', 'pck_network_destroy',
            'pck_network_dims', 'pck_network_group_lanes', 'pck_network_set_plan_mode', 'pck_energies', 'pck_rate_constants', 'pck_species_rates',
            'pck_reaction_rates', 'pck_jacobian', 'pck_solve', 'pck_solve_cascade', 'pck_drc', 'pck_energy_span', 'pck_ensemble_noise',
            'pck_ensemble_stats', 'pck_drc_at', 'pck_drc_adjoint', 'pck_sens_at', 'pck_sens_adjoint',
            'pck_network_set_sens_lanes', 'pck_network_sens_lanes', 'pck_drc_multi_at', 'pck_drc_multi_adjoint',
            'pck_network_set_multi_lanes', 'pck_eigvals', 'pck_stability_at', 'pck_stability', 'pck_cascade_drc_at',
            'pck_cascade_drc')
# entry points added without a new ABI version: a library built before them still loads, and the call that
# needs one says so (engine.py)
OPTIONAL = ('pck_cascade_drc_at', 'pck_cascade_drc')

ABI_VERSION = 10

# header slot indices (must match the enums of include/pycatkin_amd.h)
I_VERSION, I_NDESC, I_NTH, I_NREG, I_NRXN, I_NDYN, I_NFIX, I_NCONS, I_NTOF = range(9)
I_OFF_TH, I_OFF_REG, I_OFF_RX, I_OFF_EXPF, I_OFF_EXPR, I_OFF_FOLDF, I_OFF_FOLDR, I_OFF_CPIV, I_OFF_TOF = range(9, 18)
I_HDR = 18
D_TH, D_FREQ, D_REGCOEF, D_RX, D_STOICH, D_DYN, D_CONS = range(7)
D_NBLK = 7
IP_MIN = I_HDR + D_NBLK

RX_ARRHENIUS, RX_ADS_KEQ, RX_DES_KEQ, RX_ADS_KDES, RX_DES_KDES = range(5)
TH_VIB, TH_GAS = 1, 2
MAX_DYN, MAX_DYN_LANE, MAX_RXN, MAX_CONS, MAX_TOF = 64, 8, 256, 4, 16
MAX_PES = 64
PLAN_AUTO, PLAN_RUNTIME, PLAN_GROUP = 0, 1, 2
SENS_LANES_GROUP, SENS_LANES_ONE, SENS_LANES_AUTO = 0, 1, 2
# adjoint_kernel= of the System calls -> pck_network_set_sens_lanes / pck_network_set_multi_lanes mode
SENS_LANES_MODES = {'group': SENS_LANES_GROUP, 'lane': SENS_LANES_ONE, 'auto': SENS_LANES_AUTO}
ST_OK, ST_MAXSTEPS, ST_STEPFAIL, ST_NONFINITE, ST_NEWTON, ST_NEWTON_LOOSE, ST_DRC_MIXED = range(7)
ST_SENS_SINGULAR = 7
ST_SENS_PRECISION = 8
ST_EIG_NOCONV = 9
# eig_kernel= of the stability calls -> the `lanes` argument of pck_eigvals / pck_stability_at / pck_stability
# the per-condition outputs of pck_eig_out beside the spectrum wr / wi
EIG_OUTPUTS = ('re_max', 'im_max', 're_min', 'scale', 'n_pos', 'status')
EIG_LANES_MODES = {'group': SENS_LANES_GROUP, 'lane': SENS_LANES_ONE, 'auto': SENS_LANES_AUTO}
E_ARG, E_HIP, E_SIZE = -1, -2, -3
MAX_CELLS = 4096
CASCADE_START_Y0, CASCADE_START_UPSTREAM = 0, 1
# start= of the cascade calls -> pck_cascade.start
CASCADE_START_MODES = {'system': CASCADE_START_Y0, 'upstream': CASCADE_START_UPSTREAM}


class Conditions(C.Structure):
    _fields_ = [('n', C.c_int64),
                ('T', C.c_void_p), ('sT', C.c_int64),
                ('p', C.c_void_p), ('sp', C.c_int64),
                ('desc', C.c_void_p), ('ld_desc', C.c_int64), ('s_desc', C.c_int64),
                ('fixc', C.c_void_p), ('ld_fix', C.c_int64), ('s_fix', C.c_int64),
                ('y0', C.c_void_p), ('ld_y0', C.c_int64), ('s_y0', C.c_int64),
                ('inflow', C.c_void_p), ('ld_in', C.c_int64), ('s_in', C.c_int64)]


class SolveParams(C.Structure):
    _fields_ = [('t0', C.c_double), ('t_end', C.c_double), ('rtol', C.c_double), ('atol', C.c_double),
                ('max_steps', C.c_int32), ('newton', C.c_int32), ('newton_iters', C.c_int32),
                ('want_activity', C.c_int32), ('drc_eps', C.c_double), ('t_out', C.c_void_p), ('n_out', C.c_int64),
                ('retry_rtol', C.c_double), ('retry_atol', C.c_double), ('wave_order', C.c_int32),
                ('root_dist', C.c_double), ('screen_rtol', C.c_double), ('screen_margin', C.c_double)]


class Outputs(C.Structure):
    _fields_ = [('y', C.c_void_p), ('ld_y', C.c_int64), ('tof', C.c_void_p), ('status', C.c_void_p),
                ('nsteps', C.c_void_p), ('kf', C.c_void_p), ('kr', C.c_void_p), ('ld_k', C.c_int64),
                ('traj', C.c_void_p), ('ld_traj', C.c_int64)]


class Cascade(C.Structure):
    _fields_ = [('cells', C.c_int32), ('start', C.c_int32), ('y_cells', C.c_void_p), ('ld_yc', C.c_int64),
                ('tof_cells', C.c_void_p), ('status_cells', C.c_void_p), ('nsteps_cells', C.c_void_p),
                ('ld_c', C.c_int64), ('cell_fail', C.c_void_p)]


class Landscape(C.Structure):
    _fields_ = [('n_pts', C.c_int32), ('reg', C.c_int32 * MAX_PES), ('ts_mask', C.c_uint64)]


class SpanOutputs(C.Structure):
    _fields_ = [('tof', C.c_void_p), ('espan', C.c_void_p), ('eapp', C.c_void_p), ('dgrxn', C.c_void_p),
                ('i_tdts', C.c_void_p), ('i_tdi', C.c_void_p), ('x_ts', C.c_void_p), ('x_int', C.c_void_p),
                ('ld_x', C.c_int64), ('energy', C.c_void_p), ('ld_e', C.c_int64)]


class EnsStats(C.Structure):
    _fields_ = [('count', C.c_void_p), ('mean', C.c_void_p), ('std', C.c_void_p), ('min', C.c_void_p),
                ('max', C.c_void_p), ('ld_out', C.c_int64)]


class SensOut(C.Structure):
    _fields_ = [('xi', C.c_void_p), ('ld_xi', C.c_int64), ('sf', C.c_void_p), ('sr', C.c_void_p), ('ld_s', C.c_int64),
                ('order', C.c_void_p), ('ld_order', C.c_int64), ('order_in', C.c_void_p), ('ld_in', C.c_int64),
                ('dir', C.c_void_p), ('ld_dir', C.c_int64), ('err', C.c_void_p), ('tof0', C.c_void_p),
                ('status', C.c_void_p)]


class SensDirs(C.Structure):
    _fields_ = [('nd', C.c_int64), ('a', C.c_void_p), ('c', C.c_void_p), ('ld', C.c_int64), ('stride', C.c_int64)]


class MultiObj(C.Structure):
    _fields_ = [('K', C.c_int), ('wr', C.c_void_p), ('wy', C.c_void_p)]


class MultiOut(C.Structure):
    _fields_ = [('val', C.c_void_p), ('ld_val', C.c_int64), ('xi', C.c_void_p), ('ld_xi', C.c_int64),
                ('status', C.c_void_p), ('ostatus', C.c_void_p), ('ld_os', C.c_int64)]


class EigOut(C.Structure):
    _fields_ = [('wr', C.c_void_p), ('wi', C.c_void_p), ('ld_w', C.c_int64), ('re_max', C.c_void_p),
                ('im_max', C.c_void_p), ('re_min', C.c_void_p), ('scale', C.c_void_p), ('n_pos', C.c_void_p),
                ('status', C.c_void_p)]


_lib = None


def load():
    """Load libpycatkin_amd.so (built by __graft_entry__.build()); raise if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise RuntimeError('pycatkin_amd: %s not found -- run `python -c "import __graft_entry__ as g; g.build()"` '
                           '(hipcc --offload-arch=gfx950); there is no CPU fallback' % LIB_PATH)
    # torch first: its HIP runtime (libamdhip64.so.7, bundled with the wheel) is
    # then the one our library's libamdhip64.so.7 dependency binds to, so the
    # process has a single HIP/HSA runtime and device buffers are shared.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    vp, i64, i32p = C.c_void_p, C.c_int64, C.POINTER(C.c_int32)
    lib.pck_abi_version.restype = C.c_int
    lib.pck_last_error.restype = C.c_char_p
    # before any symbol is bound: an older library lacks the newer ones
    if lib.pck_abi_version() != ABI_VERSION:
        raise RuntimeError('pycatkin_amd: ABI mismatch (library %d, python %d)' % (lib.pck_abi_version(), ABI_VERSION))
    lib.pck_network_create.argtypes = [vp, i64, vp, i64, C.POINTER(vp)]
    lib.pck_network_destroy.argtypes = [vp]
    lib.pck_network_dims.argtypes = [vp, i32p]
    lib.pck_network_group_lanes.argtypes = [vp, i32p]
    lib.pck_network_set_plan_mode.argtypes = [vp, C.c_int]
    lib.pck_network_set_sens_lanes.argtypes = [vp, C.c_int]
    lib.pck_network_sens_lanes.argtypes = [vp, i32p]
    lib.pck_network_set_multi_lanes.argtypes = [vp, C.c_int]
    lib.pck_energies.argtypes = [vp, C.POINTER(Conditions), vp, i64, vp]
    lib.pck_rate_constants.argtypes = [vp, C.POINTER(Conditions), vp, vp, i64, vp]
    lib.pck_species_rates.argtypes = [vp, C.POINTER(Conditions), vp, vp, i64, vp, i64, vp, vp]
    lib.pck_jacobian.argtypes = [vp, C.POINTER(Conditions), vp, vp, i64, vp, i64, vp, vp]
    lib.pck_reaction_rates.argtypes = [vp, C.POINTER(Conditions), vp, vp, i64, vp, i64, vp, vp, i64, vp]
    lib.pck_solve.argtypes = [vp, C.POINTER(Conditions), C.POINTER(SolveParams), C.POINTER(Outputs), vp]
    lib.pck_solve_cascade.argtypes = [vp, C.POINTER(Conditions), C.POINTER(SolveParams), C.POINTER(Cascade),
                                      C.POINTER(Outputs), vp]
    lib.pck_drc.argtypes = [vp, C.POINTER(Conditions), C.POINTER(SolveParams), vp, i64, vp, vp, vp, vp]
    lib.pck_drc_at.argtypes = [vp, C.POINTER(Conditions), vp, vp, i64, vp, i64, vp, vp, i64, vp, vp, vp]
    lib.pck_drc_adjoint.argtypes = [vp, C.POINTER(Conditions), C.POINTER(SolveParams), vp, i64, vp, vp, vp, vp]
    lib.pck_sens_at.argtypes = [vp, C.POINTER(Conditions), vp, vp, i64, vp, i64, vp, C.POINTER(SensDirs), C.c_double,
                                C.POINTER(SensOut), vp]
    lib.pck_sens_adjoint.argtypes = [vp, C.POINTER(Conditions), C.POINTER(SolveParams), C.POINTER(SensDirs), C.c_double,
                                     C.POINTER(SensOut), vp, vp]
    lib.pck_drc_multi_at.argtypes = [vp, C.POINTER(Conditions), vp, vp, i64, vp, i64, vp, C.POINTER(MultiObj),
                                     C.POINTER(MultiOut), vp]
    lib.pck_drc_multi_adjoint.argtypes = [vp, C.POINTER(Conditions), C.POINTER(SolveParams), C.POINTER(MultiObj),
                                          C.POINTER(MultiOut), vp, vp]
    lib.pck_eigvals.argtypes = [vp, C.c_int, i64, i64, vp, C.c_double, C.c_int, C.POINTER(EigOut), i32p, vp]
    lib.pck_stability_at.argtypes = [vp, C.POINTER(Conditions), vp, vp, i64, vp, i64, vp, C.c_int, C.c_double, C.c_int,
                                     C.POINTER(EigOut), i32p, vp]
    lib.pck_stability.argtypes = [vp, C.POINTER(Conditions), C.POINTER(SolveParams), C.c_int, C.c_double, C.c_int,
                                  C.POINTER(EigOut), i32p, vp, vp]
    lib.pck_energy_span.argtypes = [vp, C.POINTER(Conditions), C.POINTER(Landscape), C.POINTER(SpanOutputs), vp]
    lib.pck_ensemble_noise.argtypes = [C.c_uint64, C.c_uint64, i64, i64, i64, C.c_int, C.c_double, C.c_double, vp, i64, vp]
    lib.pck_ensemble_stats.argtypes = [vp, i64, i64, vp, C.c_uint32, i64, i64, i64, C.POINTER(EnsStats), vp]
    if hasattr(lib, 'pck_cascade_drc_at'):
        lib.pck_cascade_drc_at.argtypes = [vp, C.POINTER(Conditions), vp, vp, i64, vp, i64, C.c_int32, vp, i64,
                                           C.POINTER(MultiObj), C.POINTER(MultiOut), vp, i64, vp]
    if hasattr(lib, 'pck_cascade_drc'):
        lib.pck_cascade_drc.argtypes = [vp, C.POINTER(Conditions), C.POINTER(SolveParams), C.POINTER(Cascade),
                                        C.POINTER(MultiObj), C.POINTER(MultiOut), vp, i64, vp, vp]
    for name in EXPORTED:
        if name in OPTIONAL and not hasattr(lib, name):
            continue
        if name not in ('pck_last_error',):
            getattr(lib, name).restype = C.c_int
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        msg = load().pck_last_error().decode(errors='replace')
        raise RuntimeError('pycatkin_amd C-ABI error %d: %s' % (rc, msg))
