// Multi-objective analytic degree of rate control: one assembly and one
// factorisation of the steady Jacobian per condition, then K adjoint solves.
//
// The objectives are data of the call, not of the plan: objective m is
//
//     J_m = sum_j wr[m][j] net_j + sum_i wy[m][i] y_i
//
// (a sum of net rates -- a TOF, one side of a selectivity -- and / or of state
// variables -- a coverage, an outlet concentration of a CSTR), and with F, A
// and b_j as csrc/mk_sens.h poses them and g_m = dJ_m / dy
//
//     A^T lambda_m = g_m,   s_mj = wr[m][j] - sum_i lambda_mi w_i S_ij,
//     xi[m][j] = d ln J_m / d ln k_j at fixed K_j = net_j s_mj / J_m.
//
// Assembly, replaced rows, equilibration, the LU and the solve are the group
// schedule of mk_adjoint.h, as sens_body (mk_sens.h) uses them: the LU carries
// no right-hand side and keeps the multiplier l of a row at step k in the entry
// it annihilates, so that every objective replays the forward elimination on
// its own g_m (G multiply-subtracts per step for the group, against G^2 / 2 of
// the factorisation) and then back-substitutes.  What differs from sens_body:
// the matrix is factored before any objective is judged (val is written for
// every condition), a non-finite entry of L or U is PCK_ST_SENS_SINGULAR, and a
// non-finite lambda_m is PCK_ST_NONFINITE for that objective alone.
//
// Layout: as sens_body, G = 16 / 32 / 64 lanes per condition, lane i owns
// species i and row i of M = A^T in LDS.  The matrix has to survive the K
// solves, so lambda_mi w_i is parked in G double-doubles of its own behind the
// matrix: 16 (G^2 + G) bytes per group, 66 560 bytes at G = 64 -- above the
// 64 KiB a kernel may ask for by default (the launch raises the limit).
// Nothing is sized by K: the objectives are a run-time loop.
//
// Only val and xi: the per-direction split rf_j s_mj / J_m of a coverage
// objective is not safe in double-double and no guard for it is known
// (DESIGN.md "Multi-objective DRC").
#pragma once
#include "mk_sens.h"

namespace pck {

// the objectives (pck_multi_obj) and the outputs (pck_multi_out) of the C-ABI
struct MultiObj {
    int K;
    const double* wr;                    // [K][NRXN] or null (all zero)
    const double* wy;                    // [K][NDYN] or null (all zero)
};
struct MultiOut {
    double* val; int64_t ld_val;         // [K][ld_val]
    double* xi; int64_t ld_xi;           // [K * NRXN][ld_xi], row m * NRXN + j
    int32_t* status;                     // [n], optional
    int32_t* ostatus; int64_t ld_os;     // [K][ld_os], optional
};

// LDS bytes of a 64-thread block: per group the matrix and G parked values
__host__ __device__ constexpr size_t multi_lds_bytes(int G) { return (size_t)(64 / G) * (G * G + G) * sizeof(dd); }

template <int G>
__device__ __forceinline__ void multi_body(const NetView& nv, const GrpView& gv, const CondView& cv, const double* kf,
                                           const double* kr, int64_t ld_k, const double* yin, int64_t ld_y,
                                           const int32_t* status_in, const MultiObj& ob, const MultiOut& out) {
    extern __shared__ double lds[];
    const int grp = threadIdx.x / G, gl = threadIdx.x % G;
    const int64_t c = (int64_t)blockIdx.x * (64 / G) + grp;
    if (c >= cv.n) return;                         // group-uniform exit; no block barriers below
    const int NS = nv.NDYN, R = nv.NRXN;
    const bool row = gl < NS;
    dd* M = (dd*)lds + (size_t)grp * (G * G + G);  // M[q * G + i] = A[i][q]
    dd* Lw = M + G * G;                            // lambda_mi w_i of the objective at hand
    const SensIn in{kf, kr, ld_k, yin, ld_y, cv.fixc, cv.ld_fix, cv.s_fix, c};
    const double NaN = __builtin_nan("");

    int st = status_in ? status_in[c] : PCK_ST_OK;
    double sr = 1.0, dc = 1.0, wi = 0.0;
    int step = -1;
    if (st == PCK_ST_OK) {                         // group-uniform
        double rs;
        const bool repl = grp_assemble<G>(nv, gv, cv, in, M, gl, row, rs);
        wi = repl ? 0.0 : rs;                      // b_j's weight on this row
        grp_equilibrate<G>(M, NS, gl, row, dc, sr);
        dd none = dd_of(0.0);                      // no right-hand side is carried
        if (!(grp_factor<G, false>(M, NS, gl, row, step, none) && grp_factor_finite<G>(M, NS, gl, row)))
            st = PCK_ST_SENS_SINGULAR;
    }
    if (gl == 0 && out.status) out.status[c] = st;

    for (int m = 0; m < ob.K; ++m) {
        const double* wr = ob.wr ? ob.wr + (int64_t)m * R : nullptr;
        const double* wy = ob.wy ? ob.wy + (int64_t)m * NS : nullptr;
        double* xi = out.xi + (int64_t)m * R * out.ld_xi + c;
        // J_m in double-double, the same bits on every lane
        dd jp = dd_of(0.0);
        if (wr)
            for (int j = gl; j < R; j += G) {
                const double w = wr[j];
                if (w == 0.0) continue;
                dd rf, rr;
                sens_fr(nv, gv, in, j, rf, rr);
                jp = dd_add(jp, dd_mul(dd_sub(rf, rr), w));
            }
        if (wy && row) jp = dd_add(jp, two_prod(wy[gl], yin[gl * ld_y + c]));
        const dd J = gsum_dd<G>(jp);
        const double Jd = J.hi + J.lo;
        if (gl == 0) out.val[m * out.ld_val + c] = Jd;
        int so = st;
        if (so == PCK_ST_OK && !(isfinite(Jd) && Jd != 0.0)) so = PCK_ST_NONFINITE;
        if (so != PCK_ST_OK) {                     // group-uniform
            for (int j = gl; j < R; j += G) xi[j * out.ld_xi] = NaN;
            if (gl == 0 && out.ostatus) out.ostatus[m * out.ld_os + c] = so;
            continue;
        }

        // g_m = dJ_m / dy, lane q its own component, in the row scale of M
        dd g = dd_of(0.0);
        if (row) {
            if (wr)
                for (int j = 0; j < R; ++j)
                    if (wr[j] != 0.0) grp_g_add<true>(nv, gv, in, j, wr[j], gl, g);
            if (wy) g = dd_add(g, dd_of(wy[gl]));
            g = dd_scale(g, sr);
        }
        const dd lam = grp_solve<G, false>(M, NS, gl, row, step, g);
        if (!grp_finite<G>(lam, row)) {            // group-uniform: an overflow of this objective alone
            for (int j = gl; j < R; j += G) xi[j * out.ld_xi] = NaN;
            if (gl == 0 && out.ostatus) out.ostatus[m * out.ld_os + c] = PCK_ST_NONFINITE;
            continue;
        }
        // lambda_mi x (b_j's row weight) where every lane can read it
        wsync();                                   // the readers of the previous objective are done
        if (row) Lw[gl] = dd_mul(dd_scale(lam, dc), wi);
        wsync();
        // xi[m][j] = net_j s_mj / J_m, lane per reaction
        for (int j = gl; j < R; j += G) {
            dd rf, rr;
            sens_fr(nv, gv, in, j, rf, rr);
            const dd s = adj_bracket(nv, j, wr ? wr[j] : 0.0, [&](int i) { return Lw[i]; });
            const dd x = dd_div(dd_mul(dd_sub(rf, rr), s), J);
            xi[j * out.ld_xi] = x.hi + x.lo;
        }
        if (gl == 0 && out.ostatus) out.ostatus[m * out.ld_os + c] = PCK_ST_OK;
    }
}

// val[m], xi[m][j] and the statuses of K objectives per condition.
template <int G>
__global__ void __launch_bounds__(64) k_multi_adjoint(NetView nv, GrpView gv, CondView cv, const double* kf,
                                                      const double* kr, int64_t ld_k, const double* yin, int64_t ld_y,
                                                      const int32_t* status_in, MultiObj ob, MultiOut out) {
    multi_body<G>(nv, gv, cv, kf, kr, ld_k, yin, ld_y, status_in, ob, out);
}

#define PCK_SIG_MULTI                                                                                          \
    NetView, GrpView, CondView, const double*, const double*, int64_t, const double*, int64_t, const int32_t*, \
        MultiObj, MultiOut
#define PCK_INST_MULTI(X) X(16) X(32) X(64)
#define PCK_DO_MULTI(EXT, GG) EXT template __global__ void k_multi_adjoint<GG>(PCK_SIG_MULTI);

}  // namespace pck
