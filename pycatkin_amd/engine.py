"""Device execution of a compiled network through the C-ABI.

PyTorch-ROCm is used for device buffers and the current HIP stream only;
every number is computed by the HIP kernels of libpycatkin_amd.so.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib as L
from .constants.physical_constants import bartoPa


_POISON = os.environ.get('PCK_DEBUG_POISON') == '1'
EIG_OUTPUTS = L.EIG_OUTPUTS


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError('pycatkin_amd needs a HIP device (MI355X); torch.cuda.is_available() is False '
                           'and there is no CPU fallback')
    return torch


def _stream(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class DeviceNetwork:
    """A NetworkPlan uploaded to the current device (pck_network_create)."""

    def __init__(self, ip, dp, plan=None):
        self.lib = L.load()
        self.torch = _torch()
        self.plan = plan
        self._ip = np.ascontiguousarray(ip, np.int32)
        self._dp = np.ascontiguousarray(dp, np.float64)
        h = C.c_void_p()
        L.check(self.lib.pck_network_create(self._ip.ctypes.data_as(C.c_void_p), self._ip.size,
                                            self._dp.ctypes.data_as(C.c_void_p), self._dp.size, C.byref(h)))
        self.h = h
        dims = (C.c_int32 * 11)()
        L.check(self.lib.pck_network_dims(self.h, dims))
        (self.D, self.NTH, self.NREG, self.NRXN, self.NDYN, self.NFIX, self.NCONS, self.NTOF,
         self.nfeat, self.compiled_plan) = list(dims)[:10]

    def plan_id(self):
        """Solver plan of the last lane solve: a compiled-in id (csrc/networks.h),
        100 = hipRTC-specialised at run time (csrc/mk_jit.h), 0 = runtime plan."""
        dims = (C.c_int32 * 11)()
        L.check(self.lib.pck_network_dims(self.h, dims))
        return int(dims[9])

    def group_kernel(self):
        """Kernel of the last lane-group solve: 0 compiled-in record tables,
        1 hipRTC exact-size record tables, 2 hipRTC with the network compiled
        in (mk_group.h: ct_rhs / ct_jac)."""
        dims = (C.c_int32 * 11)()
        L.check(self.lib.pck_network_dims(self.h, dims))
        return int(dims[10])

    def group_lanes(self):
        """Lanes per condition of the last lane-group solve: 4 (quad-group
        kernel), 16, 32 or 64 (group width G); 0 before any group solve."""
        g = C.c_int32(0)
        L.check(self.lib.pck_network_group_lanes(self.h, C.byref(g)))
        return int(g.value)

    def set_sens_lanes(self, mode):
        """Lanes per condition of the adjoint kernels (drc_at, drc_adjoint,
        sens_at, sens_adjoint): 0 = the 16- / 32- / 64-lane group kernels (the
        default), 1 = one lane per condition (networks of up to 8 dynamic
        species; a larger one raises), 2 = one lane where the network allows
        it, else the group kernels (pck_network_set_sens_lanes)."""
        L.check(self.lib.pck_network_set_sens_lanes(self.h, int(mode)))

    def set_multi_lanes(self, mode):
        """Lanes per condition of the multi-objective kernels (drc_multi_at,
        drc_multi_adjoint), modes as set_sens_lanes and independent of it: 0 =
        the group kernels (the default), 1 = one lane per condition (up to 8
        dynamic species; a larger network raises), 2 = one lane where the
        network allows it (pck_network_set_multi_lanes)."""
        L.check(self.lib.pck_network_set_multi_lanes(self.h, int(mode)))

    def sens_lanes(self):
        """Lanes per condition of the last adjoint launch: 1, 16, 32 or 64; 0
        before any."""
        g = C.c_int32(0)
        L.check(self.lib.pck_network_sens_lanes(self.h, C.byref(g)))
        return int(g.value)

    def set_plan_mode(self, mode):
        """A/B switch: 0 / False = auto, 1 / True = runtime plan (never the
        compiled-in one), 2 = lane-group solver."""
        L.check(self.lib.pck_network_set_plan_mode(self.h, int(mode)))

    @classmethod
    def from_plan(cls, plan):
        return cls(plan.ip, plan.dp, plan)

    def __del__(self):
        try:
            if getattr(self, 'h', None) is not None and self.h.value:
                self.lib.pck_network_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # -- inputs -----------------------------------------------------------------
    def _col(self, x, n, name):
        """(tensor, stride): a scalar broadcasts with stride 0."""
        torch = self.torch
        t = torch.as_tensor(x, dtype=torch.float64, device='cuda')
        if t.dim() == 0 or t.numel() == 1:
            return t.reshape(1).contiguous(), 0
        t = t.reshape(-1).contiguous()
        if t.numel() != n:
            raise ValueError('%s has %d entries for %d conditions' % (name, t.numel(), n))
        return t, 1

    def _mat(self, x, rows, n, name):
        """[rows, n] matrix or a [rows] column broadcast to every condition."""
        torch = self.torch
        if rows == 0 or x is None:
            return torch.zeros(1, dtype=torch.float64, device='cuda'), 0, 0
        t = torch.as_tensor(x, dtype=torch.float64, device='cuda')
        if t.dim() == 1:
            if t.numel() != rows:
                raise ValueError('%s: expected %d rows' % (name, rows))
            return t.contiguous(), 1, 0
        if tuple(t.shape) != (rows, n):
            raise ValueError('%s: expected shape (%d, %d), got %s' % (name, rows, n, tuple(t.shape)))
        t = t.contiguous()
        return t, n, 1

    def conditions(self, n, T, p, desc=None, fixc=None, y0=None, inflow=None):
        keep = []
        c = L.Conditions()
        c.n = int(n)
        tT, c.sT = self._col(T, n, 'T')
        tp, c.sp = self._col(p, n, 'p')
        keep += [tT, tp]
        c.T, c.p = _ptr(tT), _ptr(tp)
        td, c.ld_desc, c.s_desc = self._mat(desc, self.D, n, 'descriptors')
        tf, c.ld_fix, c.s_fix = self._mat(fixc, self.NFIX, n, 'fixed species')
        keep += [td, tf]
        c.desc, c.fixc = _ptr(td), _ptr(tf)
        if y0 is not None:
            ty, c.ld_y0, c.s_y0 = self._mat(y0, self.NDYN, n, 'y0')
            keep.append(ty)
            c.y0 = _ptr(ty)
        if inflow is not None:
            ti, c.ld_in, c.s_in = self._mat(inflow, self.NDYN, n, 'inflow')
            keep.append(ti)
            c.inflow = _ptr(ti)
        return c, keep

    # -- kernels ------------------------------------------------------------------
    def energies(self, n, T, p, desc=None):
        torch = self.torch
        c, keep = self.conditions(n, T, p, desc)
        out = torch.empty((max(self.NREG, 1), max(n, 1)), dtype=torch.float64, device='cuda')
        L.check(self.lib.pck_energies(self.h, C.byref(c), _ptr(out), out.shape[1], _stream(torch)))
        return out[:self.NREG, :n]

    SPAN_OUTPUTS = ('tof', 'espan', 'eapp', 'dgrxn', 'i_tdts', 'i_tdi', 'x_ts', 'x_int', 'energy')

    def energy_span(self, n, T, p, landscape, desc=None, want=SPAN_OUTPUTS):
        """pck_energy_span: the energy-span model of `landscape` = (registers of
        the N entries, isTS flags) for n conditions in one launch.  Returns a
        dict of the outputs named in `want` (pck_span_outputs' members):
        tof, espan, eapp, dgrxn [n]; i_tdts, i_tdi [n] int32 landscape
        indices; x_ts [nTi, n], x_int [nIj-1, n]; energy [N, n]."""
        torch = self.torch
        regs, is_ts = landscape
        regs = [int(r) for r in regs]
        N = len(regs)
        if len(is_ts) != N:
            raise ValueError('landscape has %d registers and %d isTS flags' % (N, len(is_ts)))
        ls = L.Landscape()
        ls.n_pts = N
        for k in range(min(N, L.MAX_PES)):
            ls.reg[k] = regs[k]
            if is_ts[k]:
                ls.ts_mask |= 1 << k
        unknown = set(want) - set(self.SPAN_OUTPUTS)
        if unknown:
            raise ValueError('unknown energy-span outputs %s' % sorted(unknown))
        c, keep = self.conditions(n, T, p, desc)
        n_ts = sum(1 for k in range(1, N - 1) if is_ts[k])
        rows = dict(x_ts=n_ts, x_int=N - 2 - n_ts, energy=N)
        out = {}
        for k in self.SPAN_OUTPUTS:
            if k not in want:
                continue
            if k in rows:
                out[k] = torch.empty((max(rows[k], 1), max(n, 1)), dtype=torch.float64, device='cuda')
            else:
                out[k] = torch.empty(max(n, 1), dtype=torch.int32 if k.startswith('i_') else torch.float64,
                                     device='cuda')
        o = L.SpanOutputs()
        for k, t in out.items():
            setattr(o, k, _ptr(t))
        o.ld_x = o.ld_e = max(n, 1)
        L.check(self.lib.pck_energy_span(self.h, C.byref(c), C.byref(ls), C.byref(o), _stream(torch)))
        return {k: (t[:max(rows[k], 0), :n] if k in rows else t[:n]) for k, t in out.items()}

    def rate_constants(self, n, T, p, desc=None):
        torch = self.torch
        c, keep = self.conditions(n, T, p, desc)
        kf = torch.empty((max(self.NRXN, 1), max(n, 1)), dtype=torch.float64, device='cuda')
        kr = torch.empty_like(kf)
        L.check(self.lib.pck_rate_constants(self.h, C.byref(c), _ptr(kf), _ptr(kr), kf.shape[1], _stream(torch)))
        return kf[:self.NRXN, :n], kr[:self.NRXN, :n]

    def species_rates(self, n, T, p, y, kf, kr, desc=None, fixc=None, inflow=None):
        torch = self.torch
        c, keep = self.conditions(n, T, p, desc, fixc, None, inflow)
        y = torch.as_tensor(y, dtype=torch.float64, device='cuda').reshape(self.NDYN, n).contiguous()
        kf, kr = kf.contiguous(), kr.contiguous()
        out = torch.empty_like(y)
        L.check(self.lib.pck_species_rates(self.h, C.byref(c), _ptr(kf), _ptr(kr), kf.shape[1], _ptr(y), n,
                                           _ptr(out), _stream(torch)))
        return out

    def reaction_rates(self, n, T, p, y, kf, kr, desc=None, fixc=None):
        """pck_reaction_rates: (rf, rr) [NRXN, n] at states y [NDYN, n]."""
        torch = self.torch
        c, keep = self.conditions(n, T, p, desc, fixc, None, None)
        y = torch.as_tensor(y, dtype=torch.float64, device='cuda').reshape(self.NDYN, n).contiguous()
        kf, kr = kf.contiguous(), kr.contiguous()
        rf = torch.empty((max(self.NRXN, 1), n), dtype=torch.float64, device='cuda')
        rr = torch.empty_like(rf)
        L.check(self.lib.pck_reaction_rates(self.h, C.byref(c), _ptr(kf), _ptr(kr), kf.shape[1], _ptr(y), n, _ptr(rf),
                                            _ptr(rr), n, _stream(torch)))
        return rf[:self.NRXN], rr[:self.NRXN]

    def jacobian(self, n, T, p, y, kf, kr, desc=None, fixc=None, inflow=None):
        torch = self.torch
        c, keep = self.conditions(n, T, p, desc, fixc, None, inflow)
        y = torch.as_tensor(y, dtype=torch.float64, device='cuda').reshape(self.NDYN, n).contiguous()
        kf, kr = kf.contiguous(), kr.contiguous()
        out = torch.empty((self.NDYN * self.NDYN, n), dtype=torch.float64, device='cuda')
        L.check(self.lib.pck_jacobian(self.h, C.byref(c), _ptr(kf), _ptr(kr), kf.shape[1], _ptr(y), n,
                                      _ptr(out), _stream(torch)))
        return out.reshape(self.NDYN, self.NDYN, n)

    @staticmethod
    def params(t_end, t0=0.0, rtol=1e-8, atol=1e-10, max_steps=100000, newton=False, newton_iters=60,
               activity=False, drc_eps=1e-3, retry=None, wave_order=0, root_dist=0.0, screen=None):
        """retry = (rtol, atol): with newton, the conditions whose polish meets a
        degenerate root (status 4) are integrated again at these tolerances
        and report that transient end (pck_solve_params.retry_rtol).
        screen = (rtol, margin): the screening pass of steady solves
        (pck_solve_params.screen_rtol / screen_margin)."""
        p = L.SolveParams()
        p.t0, p.t_end, p.rtol, p.atol = float(t0), float(t_end), float(rtol), float(atol)
        p.max_steps, p.newton, p.newton_iters = int(max_steps), int(bool(newton)), int(newton_iters)
        p.want_activity, p.drc_eps = int(bool(activity)), float(drc_eps)
        if retry is not None:
            p.retry_rtol, p.retry_atol = float(retry[0]), float(retry[1])
        p.wave_order = int(wave_order)     # 0 auto, 1 on, -1 off (pck_solve_params.wave_order)
        p.root_dist = float(root_dist)     # newton: the root only if the transient reached it
        if screen is not None:
            p.screen_rtol, p.screen_margin = float(screen[0]), float(screen[1])
        return p

    def solve(self, n, T, p, y0, desc=None, fixc=None, inflow=None, want_k=False, out=None, t_out=None, **kw):
        """pck_solve: returns dict(y [NS,n], tof [n] (or activity), status, nsteps)
        and, with t_out (ascending sample times), traj [n_out, NS, n]."""
        torch = self.torch
        c, keep = self.conditions(n, T, p, desc, fixc, y0, inflow)
        prm = self.params(**kw)
        tt = None
        if t_out is not None:
            tt = torch.as_tensor(np.asarray(t_out, float).ravel(), dtype=torch.float64, device='cuda').contiguous()
            if tt.numel() and bool((tt[1:] < tt[:-1]).any()):
                raise ValueError('t_out must be ascending')
            prm.t_out, prm.n_out = _ptr(tt).value, int(tt.numel())
        if out is None:
            out = dict(y=torch.empty((self.NDYN, n), dtype=torch.float64, device='cuda'),
                       tof=torch.empty(n, dtype=torch.float64, device='cuda'),
                       status=torch.empty(n, dtype=torch.int32, device='cuda'),
                       nsteps=torch.empty(n, dtype=torch.int32, device='cuda'))
            if want_k:
                out['kf'] = torch.empty((self.NRXN, n), dtype=torch.float64, device='cuda')
                out['kr'] = torch.empty_like(out['kf'])
        if _POISON:
            # diagnostics (PCK_DEBUG_POISON=1): every output starts as NaN / -7,
            # so an element the kernels never write shows in the result
            for k, v in out.items():
                v.fill_(float('nan') if v.is_floating_point() else -7)
        o = L.Outputs()
        o.y, o.ld_y = _ptr(out['y']), n
        o.tof, o.status, o.nsteps = _ptr(out['tof']), _ptr(out['status']), _ptr(out['nsteps'])
        if 'kf' in out:
            o.kf, o.kr, o.ld_k = _ptr(out['kf']), _ptr(out['kr']), n
        if tt is not None and tt.numel():
            # samples a failed solve never reaches stay NaN
            out['traj'] = torch.full((tt.numel(), self.NDYN, n), float('nan'), dtype=torch.float64, device='cuda')
            o.traj, o.ld_traj = _ptr(out['traj']), n
        L.check(self.lib.pck_solve(self.h, C.byref(c), C.byref(prm), C.byref(o), _stream(torch)))
        return out

    def _cascade_out(self, n, cells, profile, want_k):
        torch = self.torch
        out = dict(y=torch.empty((self.NDYN, n), dtype=torch.float64, device='cuda'),
                   tof=torch.empty(n, dtype=torch.float64, device='cuda'),
                   status=torch.empty(n, dtype=torch.int32, device='cuda'),
                   nsteps=torch.empty(n, dtype=torch.int32, device='cuda'),
                   cell_fail=torch.empty(n, dtype=torch.int32, device='cuda'))
        if profile:
            out['y_cells'] = torch.empty((cells, self.NDYN, n), dtype=torch.float64, device='cuda')
            out['tof_cells'] = torch.empty((cells, n), dtype=torch.float64, device='cuda')
            out['status_cells'] = torch.empty((cells, n), dtype=torch.int32, device='cuda')
            out['nsteps_cells'] = torch.empty((cells, n), dtype=torch.int32, device='cuda')
        if want_k:
            out['kf'] = torch.empty((self.NRXN, n), dtype=torch.float64, device='cuda')
            out['kr'] = torch.empty_like(out['kf'])
        return out

    def solve_cascade(self, n, T, p, y0, cells, desc=None, fixc=None, inflow=None, start='system', method='fused',
                      profile=True, want_k=False, t_out=None, **kw):
        """pck_solve_cascade: `cells` CSTR cells in series per condition, cell c
        fed by cell c-1 (cell 0 by `inflow`), each solved by the rule of solve
        with the parameters **kw (params); the network's coefficients are one
        cell's.  start: 'system' (every cell's transient from y0) or
        'upstream' (from the cell before).  method: 'fused' (one launch, the
        one-lane solver only) or 'loop' (`cells` calls of solve with device
        tensors, any kernel family).  Returns dict(y [NS,n] the outlet, tof
        [n] the mean cell TOF, status, nsteps [n], cell_fail [n], -1 where no
        cell failed) and, with profile, y_cells [cells,NS,n], tof_cells,
        status_cells, nsteps_cells [cells,n].  (start may also be the integer
        of pck_cascade.start; t_out is passed on for the library to refuse.)"""
        torch = self.torch
        if isinstance(start, str) and start not in L.CASCADE_START_MODES:
            raise ValueError("start must be 'system' or 'upstream', not %r" % (start,))
        start = L.CASCADE_START_MODES[start] if isinstance(start, str) else int(start)
        if method not in ('fused', 'loop'):
            raise ValueError("method must be 'fused' or 'loop', not %r" % (method,))
        cells = int(cells)
        if method == 'loop':
            return self._cascade_loop(n, T, p, y0, cells, desc, fixc, inflow, start, profile, want_k, kw)
        c, keep = self.conditions(n, T, p, desc, fixc, y0, inflow)
        prm = self.params(**kw)
        if t_out is not None:
            tt = torch.as_tensor(np.asarray(t_out, float).ravel(), dtype=torch.float64, device='cuda').contiguous()
            keep.append(tt)
            prm.t_out, prm.n_out = _ptr(tt).value, int(tt.numel())
        # sized for the refusals too (cells out of range is the library's to refuse)
        out = self._cascade_out(n, min(max(cells, 1), L.MAX_CELLS), profile, want_k)
        if _POISON:
            for v in out.values():
                v.fill_(float('nan') if v.is_floating_point() else -7)
        o = L.Outputs()
        o.y, o.ld_y = _ptr(out['y']), n
        o.tof, o.status, o.nsteps = _ptr(out['tof']), _ptr(out['status']), _ptr(out['nsteps'])
        if want_k:
            o.kf, o.kr, o.ld_k = _ptr(out['kf']), _ptr(out['kr']), n
        cas = L.Cascade()
        cas.cells, cas.start = cells, start
        cas.cell_fail = _ptr(out['cell_fail'])
        if profile:
            cas.y_cells, cas.ld_yc = _ptr(out['y_cells']), n
            cas.tof_cells, cas.status_cells = _ptr(out['tof_cells']), _ptr(out['status_cells'])
            cas.nsteps_cells, cas.ld_c = _ptr(out['nsteps_cells']), n
        L.check(self.lib.pck_solve_cascade(self.h, C.byref(c), C.byref(prm), C.byref(cas), C.byref(o), _stream(torch)))
        return out

    def _cascade_loop(self, n, T, p, y0, cells, desc, fixc, inflow, start, profile, want_k, kw):
        """The march of solve_cascade as `cells` calls of solve, everything on
        the device: the same rules (pck_solve_cascade), on any kernel family."""
        torch = self.torch
        if not 1 <= cells <= L.MAX_CELLS:
            raise ValueError('cells must be in 1..%d, not %d' % (L.MAX_CELLS, cells))
        if start not in (L.CASCADE_START_Y0, L.CASCADE_START_UPSTREAM):
            raise ValueError('unknown cascade start mode %r' % (start,))
        off = self._dp_off(L.D_DYN)
        flow = torch.as_tensor(self._dp[off: off + 4 * self.NDYN].reshape(self.NDYN, 4)[:, 3] != 0.0, device='cuda')
        if not bool(flow.any()):
            raise ValueError('reactor cascade: the network has no flow row (every cell would be the same)')
        if inflow is None:
            raise ValueError('reactor cascade: inflow required')
        out = self._cascade_out(n, cells, True, want_k)
        ti, _, _ = self._mat(inflow, self.NDYN, n, 'inflow')
        ty, _, _ = self._mat(y0, self.NDYN, n, 'y0')
        cur_in = (ti[:, None].expand(self.NDYN, n) if ti.dim() == 1 else ti).clone()
        cur_y0 = (ty[:, None].expand(self.NDYN, n) if ty.dim() == 1 else ty).clone()
        nan = float('nan')
        fail = torch.zeros(n, dtype=torch.int32, device='cuda')
        out['cell_fail'].fill_(-1)
        for cell in range(cells):
            r = self.solve(n, T, p, cur_y0, desc, fixc, cur_in, want_k=want_k and cell == 0, **kw)
            if want_k and cell == 0:
                out['kf'], out['kr'] = r['kf'], r['kr']
            dead = fail != 0
            st = torch.where(dead, fail, r['status'])
            newfail = (~dead) & (st >= L.ST_MAXSTEPS) & (st <= L.ST_NONFINITE)
            out['y_cells'][cell] = torch.where(dead[None, :], torch.full_like(r['y'], nan), r['y'])
            out['tof_cells'][cell] = torch.where(dead, torch.full_like(r['tof'], nan), r['tof'])
            out['status_cells'][cell] = st
            out['nsteps_cells'][cell] = torch.where(dead, torch.zeros_like(r['nsteps']), r['nsteps'])
            out['cell_fail'][newfail] = cell
            fail = torch.where(newfail, st, fail)
            go = (fail == 0)
            out['y'][:, ~dead] = r['y'][:, ~dead]
            upd = go[None, :] & flow[:, None]
            cur_in = torch.where(upd, r['y'], cur_in)
            if start == L.CASCADE_START_UPSTREAM:
                cur_y0 = torch.where(go[None, :], r['y'], cur_y0)
        stc = out['status_cells']
        out['status'] = torch.where(fail != 0, fail, (stc == L.ST_NEWTON).any(0).to(torch.int32) * L.ST_NEWTON)
        out['nsteps'] = out['nsteps_cells'].sum(0, dtype=torch.int32)
        out['tof'] = out['tof_cells'].sum(0) / cells           # NaN where the march stopped
        out['tof'] = torch.where(fail != 0, torch.full_like(out['tof'], nan), out['tof'])
        if not profile:
            for k in ('y_cells', 'tof_cells', 'status_cells', 'nsteps_cells'):
                del out[k]
        return out

    def _dp_off(self, blk):
        """Offset of block `blk` (L.D_*) in the plan's double blob."""
        return int(self._ip[L.I_HDR + blk])

    def drc(self, n, T, p, y0, desc=None, fixc=None, inflow=None, **kw):
        torch = self.torch
        c, keep = self.conditions(n, T, p, desc, fixc, y0, inflow)
        prm = self.params(**kw)
        xi = torch.zeros((max(self.NRXN, 1), n), dtype=torch.float64, device='cuda')
        tof0 = torch.empty(n, dtype=torch.float64, device='cuda')
        st = torch.empty(n, dtype=torch.int32, device='cuda')
        ns = torch.empty(n, dtype=torch.int32, device='cuda')
        L.check(self.lib.pck_drc(self.h, C.byref(c), C.byref(prm), _ptr(xi), n, _ptr(tof0), _ptr(st), _ptr(ns),
                                 _stream(torch)))
        return dict(xi=xi[:self.NRXN], tof0=tof0, status=st, nsteps=ns)

    def drc_at(self, n, T, p, y, kf, kr, desc=None, fixc=None, inflow=None, status_in=None):
        """pck_drc_at: the analytic degree of rate control at the steady states
        y [NDYN, n] (kf, kr [NRXN, n] as rate_constants gives them); status_in
        ([n] int32, optional): only its 0 rows are computed.  Returns
        dict(xi [NRXN, n], tof0 [n], status [n])."""
        torch = self.torch
        c, keep = self.conditions(n, T, p, desc, fixc, None, inflow)
        y = torch.as_tensor(y, dtype=torch.float64, device='cuda').reshape(self.NDYN, n).contiguous()
        kf = torch.as_tensor(kf, dtype=torch.float64, device='cuda').reshape(self.NRXN, n).contiguous()
        kr = torch.as_tensor(kr, dtype=torch.float64, device='cuda').reshape(self.NRXN, n).contiguous()
        si = None
        if status_in is not None:
            si = torch.as_tensor(status_in, dtype=torch.int32, device='cuda').reshape(-1).contiguous()
            if si.numel() != n:
                raise ValueError('status_in has %d entries for %d conditions' % (si.numel(), n))
        xi = torch.zeros((max(self.NRXN, 1), n), dtype=torch.float64, device='cuda')
        tof0 = torch.empty(n, dtype=torch.float64, device='cuda')
        st = torch.empty(n, dtype=torch.int32, device='cuda')
        L.check(self.lib.pck_drc_at(self.h, C.byref(c), _ptr(kf), _ptr(kr), n, _ptr(y), n, _ptr(si), _ptr(xi), n,
                                    _ptr(tof0), _ptr(st), _stream(torch)))
        return dict(xi=xi[:self.NRXN], tof0=tof0, status=st)

    def drc_adjoint(self, n, T, p, y0, desc=None, fixc=None, inflow=None, **kw):
        """pck_drc_adjoint: one steady solve (kw as for solve; newton=True is
        required) and the analytic degree of rate control at its states.
        Returns what drc returns."""
        torch = self.torch
        c, keep = self.conditions(n, T, p, desc, fixc, y0, inflow)
        prm = self.params(**kw)
        xi = torch.zeros((max(self.NRXN, 1), n), dtype=torch.float64, device='cuda')
        tof0 = torch.empty(n, dtype=torch.float64, device='cuda')
        st = torch.empty(n, dtype=torch.int32, device='cuda')
        ns = torch.empty(n, dtype=torch.int32, device='cuda')
        L.check(self.lib.pck_drc_adjoint(self.h, C.byref(c), C.byref(prm), _ptr(xi), n, _ptr(tof0), _ptr(st),
                                         _ptr(ns), _stream(torch)))
        return dict(xi=xi[:self.NRXN], tof0=tof0, status=st, nsteps=ns)

    def _sens_io(self, n, directions):
        """(pck_sens_out, pck_sens_dirs or None, output tensors, tensors to keep
        alive) of sens_at / sens_adjoint."""
        torch = self.torch
        f64 = dict(dtype=torch.float64, device='cuda')
        keep, dirs, nd = [], None, 0
        if directions is not None:
            a, c = (torch.as_tensor(x, **f64) for x in directions)
            if a.dim() == 2:
                a, c = a[None], c[None]
            nd = int(a.shape[0])
            if tuple(a.shape) != (nd, self.NRXN, n) or tuple(c.shape) != tuple(a.shape):
                raise ValueError('directions: expected two [ND, %d, %d] arrays, got %s and %s'
                                 % (self.NRXN, n, tuple(a.shape), tuple(c.shape)))
            a, c = a.contiguous(), c.contiguous()
            keep += [a, c]
            dirs = L.SensDirs()
            dirs.nd, dirs.a, dirs.c, dirs.ld, dirs.stride = nd, _ptr(a), _ptr(c), n, self.NRXN * n
        t = dict(xi=torch.zeros((max(self.NRXN, 1), n), **f64), sf=torch.zeros((max(self.NRXN, 1), n), **f64),
                 sr=torch.zeros((max(self.NRXN, 1), n), **f64), order=torch.zeros((max(self.NFIX, 1), n), **f64),
                 order_in=torch.zeros((max(self.NDYN, 1), n), **f64), dir=torch.zeros((max(nd, 1), n), **f64),
                 err=torch.empty(n, **f64), tof0=torch.empty(n, **f64),
                 status=torch.empty(n, dtype=torch.int32, device='cuda'))
        o = L.SensOut()
        o.xi, o.ld_xi, o.sf, o.sr, o.ld_s = _ptr(t['xi']), n, _ptr(t['sf']), _ptr(t['sr']), n
        o.order, o.ld_order, o.order_in, o.ld_in = _ptr(t['order']), n, _ptr(t['order_in']), n
        o.dir, o.ld_dir = _ptr(t['dir']), n
        o.err, o.tof0, o.status = _ptr(t['err']), _ptr(t['tof0']), _ptr(t['status'])
        for k, rows in (('xi', self.NRXN), ('sf', self.NRXN), ('sr', self.NRXN), ('order', self.NFIX),
                        ('order_in', self.NDYN), ('dir', nd)):
            t[k] = t[k][:rows]
        return o, dirs, t, keep

    def sens_at(self, n, T, p, y, kf, kr, desc=None, fixc=None, inflow=None, status_in=None, directions=None,
                err_max=1e-9):
        """pck_sens_at: the adjoint sensitivities at the steady states y
        [NDYN, n] (kf, kr [NRXN, n]).  directions = (a, c), [ND, NRXN, n] each
        (or [NRXN, n] for one): d ln kf, d ln kr.  Returns dict(xi, sf, sr
        [NRXN, n], order [NFIX, n], order_in [NDYN, n], dir [ND, n], err, tof0,
        status [n]); a condition with err > err_max has status 8 and NaN in
        everything but xi, tof0, err (err_max <= 0: no guard)."""
        torch = self.torch
        c, keep = self.conditions(n, T, p, desc, fixc, None, inflow)
        y = torch.as_tensor(y, dtype=torch.float64, device='cuda').reshape(self.NDYN, n).contiguous()
        kf = torch.as_tensor(kf, dtype=torch.float64, device='cuda').reshape(self.NRXN, n).contiguous()
        kr = torch.as_tensor(kr, dtype=torch.float64, device='cuda').reshape(self.NRXN, n).contiguous()
        si = None
        if status_in is not None:
            si = torch.as_tensor(status_in, dtype=torch.int32, device='cuda').reshape(-1).contiguous()
            if si.numel() != n:
                raise ValueError('status_in has %d entries for %d conditions' % (si.numel(), n))
        o, dirs, out, keep2 = self._sens_io(n, directions)
        L.check(self.lib.pck_sens_at(self.h, C.byref(c), _ptr(kf), _ptr(kr), n, _ptr(y), n, _ptr(si),
                                     C.byref(dirs) if dirs is not None else None, float(err_max), C.byref(o),
                                     _stream(torch)))
        return out

    def sens_adjoint(self, n, T, p, y0, desc=None, fixc=None, inflow=None, directions=None, err_max=1e-9, **kw):
        """pck_sens_adjoint: one steady solve (kw as for solve; newton=True is
        required) and sens_at at its states.  Returns what sens_at returns
        plus nsteps."""
        torch = self.torch
        c, keep = self.conditions(n, T, p, desc, fixc, y0, inflow)
        prm = self.params(**kw)
        o, dirs, out, keep2 = self._sens_io(n, directions)
        out['nsteps'] = torch.empty(n, dtype=torch.int32, device='cuda')
        L.check(self.lib.pck_sens_adjoint(self.h, C.byref(c), C.byref(prm), C.byref(dirs) if dirs is not None else None,
                                          float(err_max), C.byref(o), _ptr(out['nsteps']), _stream(torch)))
        return out

    def _multi_io(self, n, wr, wy):
        """(pck_multi_obj, pck_multi_out, output tensors, tensors to keep alive)
        of drc_multi_at / drc_multi_adjoint: wr [K, NRXN] and / or wy [K, NDYN]."""
        torch = self.torch
        f64 = dict(dtype=torch.float64, device='cuda')
        if wr is None and wy is None:
            raise ValueError('objectives: wr and wy are both None')
        keep = []
        K = None
        for w, cols, name in ((wr, self.NRXN, 'wr'), (wy, self.NDYN, 'wy')):
            if w is None:
                keep.append(None)
                continue
            w = torch.as_tensor(w, **f64)
            if w.dim() == 1:
                w = w[None]
            if w.dim() != 2 or w.shape[1] != cols or w.shape[0] < 1 or (K is not None and w.shape[0] != K):
                raise ValueError('objectives: %s has shape %s, expected (K, %d)' % (name, tuple(w.shape), cols))
            K = int(w.shape[0])
            keep.append(w.contiguous())
        ob = L.MultiObj()
        ob.K, ob.wr, ob.wy = K, _ptr(keep[0]), _ptr(keep[1])
        R = self.NRXN
        t = dict(val=torch.empty((K, n), **f64), xi=torch.zeros((K * max(R, 1), n), **f64),
                 status=torch.empty(n, dtype=torch.int32, device='cuda'),
                 ostatus=torch.empty((K, n), dtype=torch.int32, device='cuda'))
        o = L.MultiOut()
        o.val, o.ld_val, o.xi, o.ld_xi = _ptr(t['val']), n, _ptr(t['xi']), n
        o.status, o.ostatus, o.ld_os = _ptr(t['status']), _ptr(t['ostatus']), n
        t['xi'] = t['xi'][:K * R].reshape(K, R, n)
        return ob, o, t, keep

    def drc_multi_at(self, n, T, p, y, kf, kr, wr=None, wy=None, desc=None, fixc=None, inflow=None, status_in=None):
        """pck_drc_multi_at: the degree of rate control of K objectives
        J_m = wr[m] . net + wy[m] . y (wr [K, NRXN], wy [K, NDYN]; either may be
        None) at the steady states y [NDYN, n], from one factorisation and K
        adjoint solves; the kernel by set_multi_lanes.  Returns dict(val [K, n],
        xi [K, NRXN, n], status [n], ostatus [K, n])."""
        torch = self.torch
        ob, o, out, keep2 = self._multi_io(n, wr, wy)
        c, keep = self.conditions(n, T, p, desc, fixc, None, inflow)
        y = torch.as_tensor(y, dtype=torch.float64, device='cuda').reshape(self.NDYN, n).contiguous()
        kf = torch.as_tensor(kf, dtype=torch.float64, device='cuda').reshape(self.NRXN, n).contiguous()
        kr = torch.as_tensor(kr, dtype=torch.float64, device='cuda').reshape(self.NRXN, n).contiguous()
        si = None
        if status_in is not None:
            si = torch.as_tensor(status_in, dtype=torch.int32, device='cuda').reshape(-1).contiguous()
            if si.numel() != n:
                raise ValueError('status_in has %d entries for %d conditions' % (si.numel(), n))
        L.check(self.lib.pck_drc_multi_at(self.h, C.byref(c), _ptr(kf), _ptr(kr), n, _ptr(y), n, _ptr(si),
                                          C.byref(ob), C.byref(o), _stream(torch)))
        return out

    def drc_multi_adjoint(self, n, T, p, y0, wr=None, wy=None, desc=None, fixc=None, inflow=None, **kw):
        """pck_drc_multi_adjoint: one steady solve (kw as for solve; newton=True
        is required) and drc_multi_at at its states.  Returns what drc_multi_at
        returns plus nsteps."""
        torch = self.torch
        ob, o, out, keep2 = self._multi_io(n, wr, wy)
        c, keep = self.conditions(n, T, p, desc, fixc, y0, inflow)
        prm = self.params(**kw)
        out['nsteps'] = torch.empty(n, dtype=torch.int32, device='cuda')
        L.check(self.lib.pck_drc_multi_adjoint(self.h, C.byref(c), C.byref(prm), C.byref(ob), C.byref(o),
                                               _ptr(out['nsteps']), _stream(torch)))
        return out

    def _cascade_drc_fn(self, name):
        fn = getattr(self.lib, name, None)
        if fn is None:
            raise RuntimeError('pycatkin_amd: %s lacks %s (the bed DRC) -- rebuild the library '
                               '(__graft_entry__.build())' % (L.LIB_PATH, name))
        return fn

    def cascade_drc_at(self, n, T, p, y_cells, kf, kr, wr=None, wy=None, desc=None, fixc=None, inflow=None,
                       status_cells=None, cells=None, want_order_in=True):
        """pck_cascade_drc_at: the degree of rate control of K bed objectives
        J_m = mean over the cells of wr[m] . net + wy[m] . y_outlet at the cell
        states y_cells [cells, NDYN, n] of a reactor cascade (solve_cascade's
        profile), kf / kr [NRXN, n]: one backward adjoint sweep through the
        cells in one launch.  status_cells [cells, n] (optional) gates a bed
        whose cells are not all status 0.  Returns dict(val [K, n], xi
        [K, NRXN, n], status [n], ostatus [K, n]) and, with want_order_in,
        order_in [K, NDYN, n] = d ln J_m / d ln inflow_i.  (cells defaults to
        y_cells' first dimension; the library refuses a count out of range.)"""
        torch = self.torch
        fn = self._cascade_drc_fn('pck_cascade_drc_at')
        ob, o, out, keep2 = self._multi_io(n, wr, wy)
        c, keep = self.conditions(n, T, p, desc, fixc, None, inflow)
        y = torch.as_tensor(y_cells, dtype=torch.float64, device='cuda')
        if y.dim() != 3 or y.shape[1] != self.NDYN or y.shape[2] != n:
            raise ValueError('y_cells has shape %s, expected (cells, %d, %d)' % (tuple(y.shape), self.NDYN, n))
        y = y.contiguous()
        cells = int(y.shape[0]) if cells is None else int(cells)
        if 1 <= cells <= L.MAX_CELLS and cells > y.shape[0]:
            raise ValueError('cells = %d, but y_cells holds %d cells' % (cells, y.shape[0]))
        kf = torch.as_tensor(kf, dtype=torch.float64, device='cuda').reshape(self.NRXN, n).contiguous()
        kr = torch.as_tensor(kr, dtype=torch.float64, device='cuda').reshape(self.NRXN, n).contiguous()
        sc = None
        if status_cells is not None:
            sc = torch.as_tensor(status_cells, dtype=torch.int32, device='cuda').contiguous()
            if sc.dim() != 2 or sc.shape[0] != y.shape[0] or sc.shape[1] != n:
                raise ValueError('status_cells has shape %s, expected (%d, %d)' % (tuple(sc.shape), y.shape[0], n))
        oi = None
        if want_order_in:
            oi = torch.empty((ob.K * self.NDYN, n), dtype=torch.float64, device='cuda')
            out['order_in'] = oi.reshape(ob.K, self.NDYN, n)
        L.check(fn(self.h, C.byref(c), _ptr(kf), _ptr(kr), n, _ptr(y), n, cells, _ptr(sc), n, C.byref(ob), C.byref(o),
                   _ptr(oi), n, _stream(torch)))
        return out

    def cascade_drc(self, n, T, p, y0, cells, wr=None, wy=None, desc=None, fixc=None, inflow=None, start='system',
                    want_order_in=True, **kw):
        """pck_cascade_drc: solve_cascade (fused; kw as for solve, newton=True
        is required) and cascade_drc_at at its cell states, with the solve's
        own rate constants.  Returns what cascade_drc_at returns plus nsteps
        [n], cell_fail [n], y_cells [cells, NDYN, n] and status_cells
        [cells, n]."""
        torch = self.torch
        fn = self._cascade_drc_fn('pck_cascade_drc')
        if isinstance(start, str) and start not in L.CASCADE_START_MODES:
            raise ValueError("start must be 'system' or 'upstream', not %r" % (start,))
        start = L.CASCADE_START_MODES[start] if isinstance(start, str) else int(start)
        cells = int(cells)
        ob, o, out, keep2 = self._multi_io(n, wr, wy)
        c, keep = self.conditions(n, T, p, desc, fixc, y0, inflow)
        prm = self.params(**kw)
        nc = min(max(cells, 1), L.MAX_CELLS)       # sized for the refusals too
        out['nsteps'] = torch.empty(n, dtype=torch.int32, device='cuda')
        out['cell_fail'] = torch.empty(n, dtype=torch.int32, device='cuda')
        out['y_cells'] = torch.empty((nc, self.NDYN, n), dtype=torch.float64, device='cuda')
        out['status_cells'] = torch.empty((nc, n), dtype=torch.int32, device='cuda')
        cas = L.Cascade()
        cas.cells, cas.start = cells, start
        cas.cell_fail = _ptr(out['cell_fail'])
        cas.y_cells, cas.ld_yc = _ptr(out['y_cells']), n
        cas.status_cells, cas.ld_c = _ptr(out['status_cells']), n
        oi = None
        if want_order_in:
            oi = torch.empty((ob.K * self.NDYN, n), dtype=torch.float64, device='cuda')
            out['order_in'] = oi.reshape(ob.K, self.NDYN, n)
        L.check(fn(self.h, C.byref(c), C.byref(prm), C.byref(cas), C.byref(ob), C.byref(o), _ptr(oi), n,
                   _ptr(out['nsteps']), _stream(torch)))
        return out

    def stability_at(self, n, T, p, y, kf, kr, desc=None, fixc=None, inflow=None, status_in=None, reduce=True,
                     re_tol=0.0, lanes=L.SENS_LANES_AUTO, want=EIG_OUTPUTS):
        """pck_stability_at: the eigenvalues of the Jacobian at the states y
        [NDYN, n] (kf, kr [NRXN, n] as rate_constants gives them), full or
        reduced on the conservation laws; status_in as in drc_at.  Returns the
        outputs of `want` (device tensors) plus 'lanes'."""
        torch = self.torch
        c, keep = self.conditions(n, T, p, desc, fixc, None, inflow)
        y = torch.as_tensor(y, dtype=torch.float64, device='cuda').reshape(self.NDYN, n).contiguous()
        kf = torch.as_tensor(kf, dtype=torch.float64, device='cuda').reshape(self.NRXN, n).contiguous()
        kr = torch.as_tensor(kr, dtype=torch.float64, device='cuda').reshape(self.NRXN, n).contiguous()
        si = _status_in(torch, status_in, n)
        ns_eff = self.NDYN - (self.NCONS if reduce else 0)
        o, out = _eig_io(torch, ns_eff, n, want)
        used = C.c_int32(0)
        L.check(self.lib.pck_stability_at(self.h, C.byref(c), _ptr(kf), _ptr(kr), n, _ptr(y), n, _ptr(si),
                                          int(bool(reduce)), float(re_tol), int(lanes), C.byref(o), C.byref(used),
                                          _stream(torch)))
        out['lanes'] = int(used.value)
        return out

    def stability(self, n, T, p, y0, desc=None, fixc=None, inflow=None, reduce=True, re_tol=0.0,
                  lanes=L.SENS_LANES_AUTO, want=EIG_OUTPUTS, **kw):
        """pck_stability: one steady solve (kw as for solve; newton=True is
        required) and stability_at at its states.  Returns what stability_at
        returns plus nsteps."""
        torch = self.torch
        c, keep = self.conditions(n, T, p, desc, fixc, y0, inflow)
        prm = self.params(**kw)
        ns_eff = self.NDYN - (self.NCONS if reduce else 0)
        o, out = _eig_io(torch, ns_eff, n, want)
        out['nsteps'] = torch.empty(n, dtype=torch.int32, device='cuda')
        used = C.c_int32(0)
        L.check(self.lib.pck_stability(self.h, C.byref(c), C.byref(prm), int(bool(reduce)), float(re_tol), int(lanes),
                                       C.byref(o), C.byref(used), _ptr(out['nsteps']), _stream(torch)))
        out['lanes'] = int(used.value)
        return out


def _status_in(torch, status_in, n):
    if status_in is None:
        return None
    si = torch.as_tensor(status_in, dtype=torch.int32, device='cuda').reshape(-1).contiguous()
    if si.numel() != n:
        raise ValueError('status_in has %d entries for %d conditions' % (si.numel(), n))
    return si


def _eig_io(torch, ns, n, want, ld=None):
    """(pck_eig_out, output tensors) of the eigenvalue calls; `want` names the
    outputs ('wr' / 'wi' come together as the spectrum [ns, ld])."""
    bad = [k for k in want if k not in EIG_OUTPUTS + ('wr', 'wi')]
    if bad:
        raise ValueError('unknown eigenvalue outputs %r' % (bad,))
    ld = n if ld is None else ld
    o, out = L.EigOut(), {}
    for k in want:
        if k in ('wr', 'wi'):
            out[k] = torch.empty((ns, ld), dtype=torch.float64, device='cuda')
            o.ld_w = ld
        else:
            out[k] = torch.empty(n, dtype=torch.int32 if k in ('n_pos', 'status') else torch.float64, device='cuda')
        setattr(o, k, _ptr(out[k]).value)
    return o, out


def eigvals(a, n=None, status_in=None, re_tol=0.0, lanes=L.SENS_LANES_AUTO, want=EIG_OUTPUTS + ('wr', 'wi'),
            out=None):
    """pck_eigvals: the eigenvalues of n real ns x ns matrices a [ns, ns, ld]
    (the layout of DeviceNetwork.jacobian; a device tensor, or anything
    torch.as_tensor takes), the first n <= ld of them (default: all).  `out`:
    tensors to write into instead of fresh ones (spectrum rows [ns, ld]).
    Returns the outputs of `want` (device tensors) plus 'lanes' (1, 16, 32 or
    64 lanes per matrix)."""
    lib, torch = L.load(), _torch()
    a = torch.as_tensor(a, dtype=torch.float64, device='cuda')
    if a.dim() != 3 or a.shape[0] != a.shape[1]:
        raise ValueError('a must be [ns, ns, n], got %s' % (tuple(a.shape),))
    a = a.contiguous()
    ns, ld = int(a.shape[0]), int(a.shape[2])
    n = ld if n is None else int(n)
    si = _status_in(torch, status_in, n)
    if out is None:
        o, out = _eig_io(torch, ns, n, want, ld)
    else:
        o, out = L.EigOut(), dict(out)
        for k, v in out.items():
            setattr(o, k, _ptr(v).value)
        o.ld_w = ld
    used = C.c_int32(0)
    L.check(lib.pck_eigvals(_ptr(a), ns, n, ld, _ptr(si), float(re_tol), int(lanes), C.byref(o), C.byref(used),
                            _stream(torch)))
    out['lanes'] = int(used.value)
    return out


_form_cache = {}


def descriptor_values(dnames, T, desc=None):
    """The descriptor column of one condition at temperature T: a
    temperature-keyed user energy ('@T:' descriptor, energy.tkeyed) is looked
    up in its table at T (KeyError on a missing T, like the reference's
    dErxn_user[T], reaction.py:228-262); any other descriptor comes from
    `desc` (ValueError if it is not given)."""
    from .energy import TKEYED
    given = [k for k in dnames if not k.startswith('@T:')]
    if given and desc is None:
        raise ValueError('forms depend on descriptors %s; pass desc=' % given)
    return np.array([TKEYED[k][float(T)] if k.startswith('@T:') else desc[k] for k in dnames], float)


def evaluate_forms(forms, T, p, states=None, desc=None):
    """Evaluate LinearForms (eV) for one condition on the device (kernel 1)."""
    from .network import compile_forms
    states_map = {s.name: s for s in (states or [])}
    ip, dp, regs, dnames = compile_forms(forms, states_map)
    d = None if not dnames else descriptor_values(dnames, T, desc)
    net = DeviceNetwork(ip, dp)
    vals = net.energies(1, float(T), float(p), d).cpu().numpy()[:, 0]
    return [float(vals[r]) for r in regs]


def single_reaction_rate_constants(rxn, T, p):
    """Reaction.calc_rate_constants for one condition through kernel (1)."""
    from .network import NetworkPlan  # noqa: F401
    from .classes.system import System
    from .classes.reactor import InfiniteDilutionReactor
    s = System()
    seen = {}
    for st in list(rxn.reactants) + list(rxn.products) + list(rxn.TS or []):
        seen[st.name] = st
    for st in seen.values():
        s.add_state(st)
    s.add_reaction(rxn)
    s.add_reactor(InfiniteDilutionReactor())
    kf, kr = s.rate_constants_batch(T=[float(T)], p=float(p))
    return float(kf[0, 0]), float(kr[0, 0])


# -- uncertainty ensemble (csrc/tu_ensemble.hip) ---------------------------------
def ensemble_noise(seed, n_runs, n_rep=1, n_ts=0, lead_zero=False, mu=0.0, sigma=0.01, run_first=0, out=None):
    """pck_ensemble_noise: the [1 + n_ts, n_rep * (n_runs + lead_zero)] device
    matrix of an ensemble's correlated energy noise (row 0 the adsorbates'
    shared value, row 1+k transition state k's), in the block layout of
    include/pycatkin_amd.h.  `out`: a contiguous float64 device matrix of at
    least that many columns to write into (its other columns stay untouched)."""
    torch = _torch()
    lib = L.load()
    B = int(n_runs) + int(bool(lead_zero))
    if out is None:
        out = torch.empty((1 + int(n_ts), max(int(n_rep) * B, 0)), dtype=torch.float64, device='cuda')
    elif (out.dtype != torch.float64 or not out.is_cuda or out.dim() != 2 or not out.is_contiguous()
          or out.shape[0] < 1 + int(n_ts)):
        raise ValueError('out must be a contiguous float64 device matrix of at least %d rows' % (1 + int(n_ts)))
    L.check(lib.pck_ensemble_noise(int(seed) & (2 ** 64 - 1), int(run_first) & (2 ** 64 - 1), int(n_runs), int(n_rep),
                                   int(n_ts), int(bool(lead_zero)), float(mu), float(sigma), _ptr(out),
                                   int(out.shape[1]), _stream(torch)))
    return out


STAT_OUTPUTS = ('count', 'mean', 'std', 'min', 'max')


def ensemble_stats(values, status=None, ok=(0, 4), block=None, skip=0, want=STAT_OUTPUTS):
    """pck_ensemble_stats on a device matrix `values` [n_rows, n] (or [n]):
    count / mean / population std / min / max over the columns
    c*block + skip .. c*block + block - 1 of each of the n // block blocks
    (block None: one block of n), counting the finite values whose `status`
    ([n] int32 device tensor, optional) is one of `ok`.  Returns a dict of
    device tensors [n_rows, n_rep] ([n_rep] for a 1-D input)."""
    torch = _torch()
    lib = L.load()
    v = torch.as_tensor(values, dtype=torch.float64, device='cuda')
    one_d = v.dim() == 1
    if one_d:
        v = v.reshape(1, -1)
    if v.dim() != 2:
        raise ValueError('values must be [n_rows, n] or [n]')
    if v.stride(1) != 1 and v.shape[1] > 1 or (v.shape[0] > 1 and v.stride(0) < v.shape[1]):
        v = v.contiguous()
    n_rows, n = int(v.shape[0]), int(v.shape[1])
    ld_v = int(v.stride(0)) if n_rows > 1 else max(n, 1)
    block = n if block is None else int(block)
    if block < 0 or skip < 0 or (block == 0 and n) or (block and n % block):
        raise ValueError('%d columns are not whole blocks of %d' % (n, block))
    n_rep = n // block if block else 0
    st = None
    if status is not None:
        st = torch.as_tensor(status, dtype=torch.int32, device='cuda').reshape(-1).contiguous()
        if st.numel() != n:
            raise ValueError('status has %d entries for %d columns' % (st.numel(), n))
    mask = 0
    for s in ok:
        if not 0 <= int(s) < 32:
            raise ValueError('status codes to accept must lie in 0..31')
        mask |= 1 << int(s)
    unknown = set(want) - set(STAT_OUTPUTS)
    if unknown:
        raise ValueError('unknown statistics %s' % sorted(unknown))
    out = {k: torch.empty((n_rows, max(n_rep, 1)), dtype=torch.int32 if k == 'count' else torch.float64,
                          device='cuda') for k in STAT_OUTPUTS if k in want}
    o = L.EnsStats()
    for k, t in out.items():
        setattr(o, k, _ptr(t))
    o.ld_out = max(n_rep, 1)
    L.check(lib.pck_ensemble_stats(_ptr(v), ld_v, n_rows, _ptr(st), mask, n_rep, block, int(skip), C.byref(o),
                                   _stream(torch)))
    return {k: (t[0, :n_rep] if one_d else t[:, :n_rep]) for k, t in out.items()}
