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
// Assembly, replaced rows and equilibration are sens_body's, statement for
// statement.  The LU differs in two points: no right-hand side is eliminated
// along, and the multiplier l of a row at step k is kept in the entry it
// annihilates (M[gl * G + k], dead in sens_body), so that every objective
// replays the forward elimination on its own g_m (G multiply-subtracts per
// step for the group, against G^2 / 2 of the factorisation) and then
// back-substitutes as sens_body does.
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
    double yi = 0.0, sr = 1.0, dc = 1.0, wi = 0.0;
    int step = -1;
    if (st == PCK_ST_OK) {                         // group-uniform
        for (int q = 0; q < G; ++q) M[q * G + gl] = dd_of(0.0);
        // row gl of A into column gl of M, and the row's rate f
        double rs = 0.0;
        bool pv = false;
        int law = -1;
        dd f = dd_of(0.0);
        if (row) {
            const double* d = nv.dyn + 4 * gl;
            const double T = cv.T[c * cv.sT];
            rs = (d[2] != 0.0) ? d[1] + d[2] * T : d[1];   // reactor.py:34-41, as mk_group.h: grp_setup
            const double fl = d[3];
            yi = yin[gl * ld_y + c];
            for (int e = gv.row[gl]; e < gv.row[gl + 1]; ++e) {
                const uint4 q4 = gv.ent[e];
                const int r = ent_r(q4), np = ent_np(q4);
                const dd w = two_prod(rs, ent_s(q4));
                const uint4 rec = gv.rx[r];
                dd a, b;
                sens_keff(nv, in, r, a, b);
                f = dd_add(f, dd_mul(w, sens_rate(nv, in, rec, a, b, -1)));
                for (int k = 0; k < np; ++k) {
                    dd* m = M + ent_species(q4, k) * G + gl;
                    *m = dd_add(*m, dd_mul(w, sens_rate(nv, in, rec, a, b, k)));
                }
            }
            if (fl != 0.0) {                        // the CSTR flow term fl (in - y)
                const double yin_i = cv.inflow ? cv.inflow[gl * cv.ld_in + c * cv.s_in] : 0.0;
                f = dd_add(f, dd_mul(two_sum(yin_i, -yi), fl));
                M[gl * G + gl] = dd_add(M[gl * G + gl], dd_of(-fl));
            }
            for (int l = 0; l < nv.NCONS; ++l)
                if (nv.cpiv[l] == gl) { pv = true; law = l; }
        }
        // rows replaced as in mk_solver.h: newton -- the conservation laws in
        // their pivot rows, a unit row for a pinned species (newton_pinned)
        const bool pin = row && !pv && yi == 0.0 && f.hi == 0.0 && f.lo == 0.0;
        if (pv)
            for (int q = 0; q < NS; ++q) M[q * G + gl] = dd_of(nv.C[law * NS + q]);
        if (pin)
            for (int q = 0; q < NS; ++q) M[q * G + gl] = dd_of(q == gl ? 1.0 : 0.0);
        wi = (pv || pin) ? 0.0 : rs;               // b_j's weight on this row
        wsync();

        // equilibration by powers of two (exact): the columns of M (the rows of
        // A), then its rows; both scales are kept for the objectives
        for (int q = 0; q < NS; ++q) {
            const double s = inv_pow2(gmax<G>(row ? fabs(M[gl * G + q].hi) : 0.0));
            if (row) M[gl * G + q] = dd_scale(M[gl * G + q], s);
            if (q == gl) dc = s;
        }
        if (row) {
            double m = 0.0;
            for (int q = 0; q < NS; ++q) m = fmax(m, fabs(M[gl * G + q].hi));
            sr = inv_pow2(m);
            for (int q = 0; q < NS; ++q) M[gl * G + q] = dd_scale(M[gl * G + q], sr);
        }

        // LU with partial pivoting, row per lane.  Rows are not moved: `step`
        // is the column a row was the pivot of.  The multiplier of a row stays
        // in the entry it annihilates.
        bool ok = true;
        for (int k = 0; k < NS; ++k) {
            const bool fr = row && step < 0;
            double a = fr ? fabs(M[gl * G + k].hi) : -1.0;
            if (a != a) a = INFINITY;              // a NaN must not hide behind fmax
            const double m = gmax<G>(a);
            if (!(m > 0.0) || !isfinite(m)) { ok = false; break; }    // group-uniform
            const int p = (G - 1) - gmaxi<G>((fr && a == m) ? (G - 1) - gl : -1);     // the lowest such lane
            if (gl == p) step = k;
            const dd piv = M[p * G + k];
            if (fr && gl != p) {
                const dd l = dd_div(M[gl * G + k], piv);
                for (int q = k + 1; q < NS; ++q) M[gl * G + q] = dd_sub(M[gl * G + q], dd_mul(l, M[p * G + q]));
                M[gl * G + k] = l;
            }
            wsync();                               // the next pivot row is complete before it is read
        }
        // a non-finite factor anywhere in L or U
        if (ok) {
            double fin = 1.0;
            if (row)
                for (int q = 0; q < NS; ++q) fin = isfinite(M[gl * G + q].hi + M[gl * G + q].lo) ? fin : 0.0;
            ok = gmin<G>(fin) > 0.0;
        }
        if (!ok) st = PCK_ST_SENS_SINGULAR;
    }
    if (gl == 0 && out.status) out.status[c] = st;

    // forward / reverse side of reaction j
    auto sides = [&](int j, dd& rf, dd& rr) {
        sens_keff(nv, in, j, rf, rr);
        sens_sides(nv, in, gv.rx[j], rf, rr, -1);
    };
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
                sides(j, rf, rr);
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
                for (int j = 0; j < R; ++j) {
                    const double w = wr[j];
                    if (w == 0.0) continue;
                    const uint4 rec = gv.rx[j];
                    const int np = rx_np(rec);
                    for (int k = 0; k < np; ++k) {
                        if ((rx_field(rec, k) & 63) != gl) continue;
                        dd a, b;
                        sens_keff(nv, in, j, a, b);
                        g = dd_add(g, dd_mul(sens_rate(nv, in, rec, a, b, k), w));
                    }
                }
            if (wy) g = dd_add(g, dd_of(wy[gl]));
            g = dd_scale(g, sr);
        }
        // the forward elimination replayed from the stored multipliers: at step
        // k every row still free then, the pivot apart, subtracts l g_pivot
        for (int k = 0; k < NS; ++k) {
            const int p = gmaxi<G>((row && step == k) ? gl : -1);
            const dd gp = gbcast_dd<G>(g, p);
            if (row && step > k) g = dd_sub(g, dd_mul(M[gl * G + k], gp));
        }
        // back substitution: lane k keeps lambda_k
        dd lam = dd_of(0.0);
        for (int k = NS - 1; k >= 0; --k) {
            const int p = gmaxi<G>((row && step == k) ? gl : -1);
            const dd x = dd_div(gbcast_dd<G>(g, p), M[p * G + k]);
            if (gl == k) lam = x;
            if (row && step < k) g = dd_sub(g, dd_mul(M[gl * G + k], x));
        }
        const double lsum = lam.hi + lam.lo;
        if (!(gmin<G>((!row || isfinite(lsum)) ? 1.0 : 0.0) > 0.0)) {     // group-uniform: an overflow of this objective alone
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
            sides(j, rf, rr);
            dd s = dd_of(wr ? wr[j] : 0.0);
            for (int i = 0; i < NS; ++i) {
                const double sv = nv.S[i * R + j];
                if (sv != 0.0) s = dd_sub(s, dd_mul(Lw[i], sv));
            }
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
