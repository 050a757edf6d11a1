// Analytic degree of rate control at given steady states (old_system.py:490
// System.degree_of_rate_control in the limit eps -> 0): one adjoint solve per
// condition instead of 2R+1 steady solves.
//
// With F(y, k) = 0 the steady equations as mk_solver.h: newton poses them
// (rhs rows; conservation law l in row cpiv(l); a unit row for a pinned
// species), A = dF/dy, b_j = dF/d ln k_j at fixed K_j (= rowscale_i S_ij net_j
// on rhs rows, 0 on replaced rows) and g = d TOF / dy:
//
//     A^T lambda = g,     xi_j = ([j in tof] net_j - lambda . b_j) / TOF
//
// Everything is double-double (mk_device.h: dd): at a steady state the
// Jacobian entries are sums of +-1e9 terms of quasi-equilibrated steps next to
// O(1e-7) turnover terms, the matrix has condition ~1e16 after equilibration,
// and fp64 assembly alone loses every digit of xi (DESIGN.md "Analytic DRC").
//
// Layout: the group schedule of mk_adjoint.h, whose steps (assemble,
// equilibrate, factor, solve) and outputs (sens_gate, sens_tail) these kernels
// string together: G = 16 / 32 / 64 lanes per condition (mk_kernels.hip:
// grp_g), lane i owns species i.  The G x G double-double matrix M = A^T of a
// group lives in LDS (16 G^2 bytes; nothing else does): lane i assembles row i
// of A from its row of the species CSR (GrpView), i.e. column i of M -- one
// writer per entry, plain stores, no atomics -- and then factors and
// substitutes row i of M.  Once the matrix is dead, lambda_i w_i is parked in
// M[0..G).  Rate constants, fixed-species concentrations and the state are read
// from HBM where they are used (they stay in L1 / L2).
#pragma once
#include "mk_adjoint.h"

namespace pck {

// LDS bytes of a 64-thread block: 64 / G matrices of G x G double-doubles
__host__ __device__ constexpr size_t sens_lds_bytes(int G) { return (size_t)(64 / G) * G * G * sizeof(dd); }

// The body of k_drc_adjoint (EXT = false: xi[j][ld_xi] for every active
// reaction, tof0 and status per condition) and of k_sens_adjoint (EXT = true:
// the outputs of SensExt as well, xi optional).  A zero or non-finite TOF or a
// gated status_in ends a condition before LDS is touched (sens_gate); a zero
// pivot or a non-finite lambda is PCK_ST_SENS_SINGULAR for the condition.
template <int G, bool EXT>
__device__ __forceinline__ void sens_body(const NetView& nv, const GrpView& gv, const CondView& cv, const double* kf,
                                          const double* kr, int64_t ld_k, const double* yin, int64_t ld_y,
                                          const int32_t* status_in, double* xi, int64_t ld_xi, double* tof0,
                                          int32_t* status, const SensExt& ex) {
    extern __shared__ double lds[];
    const int grp = threadIdx.x / G, gl = threadIdx.x % G;
    const int64_t c = (int64_t)blockIdx.x * (64 / G) + grp;
    if (c >= cv.n) return;                         // group-uniform exit, as every exit below; no block barriers
    const int NS = nv.NDYN;
    const bool row = gl < NS;
    dd* M = (dd*)lds + (size_t)grp * G * G;        // M[q * G + i] = A[i][q]
    const SensIn in{kf, kr, ld_k, yin, ld_y, cv.fixc, cv.ld_fix, cv.s_fix, c};

    dd tof;
    if (!sens_gate<G, EXT>(nv, gv, in, ex, status_in, gl, xi, ld_xi, tof0, status, tof)) return;

    double rs;
    const bool repl = grp_assemble<G>(nv, gv, cv, in, M, gl, row, rs);
    // g = d TOF / dy, lane q its own component
    dd g = dd_of(0.0);
    if (row)
        for (int t = 0; t < nv.NTOF; ++t) grp_g_add<false>(nv, gv, in, nv.tof[t], 1.0, gl, g);
    double dc, sr;
    grp_equilibrate<G>(M, NS, gl, row, dc, sr);
    g = dd_scale(g, sr);

    int step;
    dd lam = dd_of(0.0);
    bool ok = grp_factor<G, true>(M, NS, gl, row, step, g);      // the one g eliminated along
    if (ok) {
        lam = grp_solve<G, true>(M, NS, gl, row, step, g);
        ok = grp_finite<G>(lam, row);
    }
    if (!ok) {
        sens_fail<G, EXT>(nv, ex, c, gl, xi, ld_xi, status, PCK_ST_SENS_SINGULAR);
        return;
    }
    lam = dd_scale(lam, dc);
    // lambda_i x (b_j's row weight) where every lane can read it: the matrix is done
    wsync();
    if (row) M[gl] = dd_mul(lam, repl ? 0.0 : rs);
    wsync();
    sens_tail<G, EXT>(nv, gv, cv, in, ex, gl, tof, xi, ld_xi, status, M, lam, repl);
}

// xi[j][ld_xi] for every active reaction, tof0 and status per condition.
template <int G>
__global__ void __launch_bounds__(64) k_drc_adjoint(NetView nv, GrpView gv, CondView cv, const double* kf,
                                                    const double* kr, int64_t ld_k, const double* yin, int64_t ld_y,
                                                    const int32_t* status_in, double* xi, int64_t ld_xi,
                                                    double* tof0, int32_t* status) {
    sens_body<G, false>(nv, gv, cv, kf, kr, ld_k, yin, ld_y, status_in, xi, ld_xi, tof0, status, SensExt{});
}

// The same adjoint solve spent on every first-order sensitivity of the TOF
// (SensExt): per-direction sensitivities, reaction orders, user directions.
template <int G>
__global__ void __launch_bounds__(64) k_sens_adjoint(NetView nv, GrpView gv, CondView cv, const double* kf,
                                                     const double* kr, int64_t ld_k, const double* yin, int64_t ld_y,
                                                     const int32_t* status_in, double* xi, int64_t ld_xi,
                                                     double* tof0, int32_t* status, SensExt ex) {
    sens_body<G, true>(nv, gv, cv, kf, kr, ld_k, yin, ld_y, status_in, xi, ld_xi, tof0, status, ex);
}

#define PCK_SIG_SENS                                                                                          \
    NetView, GrpView, CondView, const double*, const double*, int64_t, const double*, int64_t, const int32_t*, \
        double*, int64_t, double*, int32_t*
#define PCK_INST_SENS(X) X(16) X(32) X(64)
#define PCK_DO_SENS(EXT, GG)                                         \
    EXT template __global__ void k_drc_adjoint<GG>(PCK_SIG_SENS); \
    EXT template __global__ void k_sens_adjoint<GG>(PCK_SIG_SENS, SensExt);

}  // namespace pck
