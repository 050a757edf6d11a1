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
// Layout: G = 16 / 32 / 64 lanes per condition (mk_kernels.hip: grp_g), lane i
// owns species i.  The G x G double-double matrix M = A^T of a group lives in
// LDS (16 G^2 bytes; nothing else does): lane i assembles row i of A from its
// row of the species CSR (GrpView), i.e. column i of M -- one writer per
// entry, plain stores, no atomics -- and then factors and substitutes row i
// of M.  Rate constants, fixed-species concentrations and the state are read
// from HBM where they are used (they stay in L1 / L2).
#pragma once
#include "mk_group.h"

namespace pck {

#pragma clang fp contract(off)
__device__ __forceinline__ dd dd_sub(dd a, dd b) { return dd_add(a, dd_neg(b)); }
// a / b: three quotient digits, each from an exact remainder (the long
// division of Hida, Li, Bailey: "Library for double-double and quad-double
// arithmetic", 2007), ~2^-104 relative
__device__ __forceinline__ dd dd_div(dd a, dd b) {
    const double q1 = a.hi / b.hi;
    dd r = dd_sub(a, dd_mul(b, q1));
    const double q2 = r.hi / b.hi;
    r = dd_sub(r, dd_mul(b, q2));
    const double q3 = r.hi / b.hi;
    const dd q = quick_two_sum(q1, q2);
    return dd_add(q, dd_of(q3));
}
#pragma clang fp contract(fast)

__device__ __forceinline__ dd dd_scale(dd a, double p2) { return {a.hi * p2, a.lo * p2}; }   // p2 a power of two: exact
// 2^-e with |v| in [2^(e-1), 2^e); 1 for v = 0
__device__ __forceinline__ double inv_pow2(double v) {
    if (!(v > 0.0) || !isfinite(v)) return 1.0;
    int e;
    (void)frexp(v, &e);
    return ldexp(1.0, -e);
}

// Inputs of one condition, read where they are used.
struct SensIn {
    const double* kf; const double* kr; int64_t ld_k;   // [R][ld_k], as pck_rate_constants gives them
    const double* y; int64_t ld_y;                      // [NS][ld_y]
    const double* fixc; int64_t ld_fix, s_fix;          // [NFIX][..]
    int64_t c;
};

// effective rate constants of reaction j: the fixed species folded in
// (mk_group.h: grp_setup), every product exact
__device__ __forceinline__ void sens_keff(const NetView& nv, const SensIn& in, int j, dd& a, dd& b) {
    a = dd_of(in.kf[j * in.ld_k + in.c]);
    b = dd_of(in.kr[j * in.ld_k + in.c]);
    for (int q = 0; q < nv.NFIX; ++q) {
        const int ea = nv.foldf[j * nv.NFIX + q], eb = nv.foldr[j * nv.NFIX + q];
        if (ea | eb) {
            const dd v = dd_of(in.fixc[q * in.ld_fix + in.c * in.s_fix]);
            if (ea) a = dd_mul(a, dd_pow(v, ea));
            if (eb) b = dd_mul(b, dd_pow(v, eb));
        }
    }
}

// net rate of the record's reaction (k0 < 0, as mk_group.h: tab_rhs_dd forms
// it), or its derivative in the state of participant k0: that factor's power
// is lowered by one and multiplied by exponent and concentration factor --
// never a division by a concentration, so y_q = 0 is an ordinary case
//
// sens_sides leaves the forward side in a and the reverse side in b;
// sens_rate is their difference
__device__ __forceinline__ void sens_sides(const NetView& nv, const SensIn& in, const uint4& rec, dd& a, dd& b, int k0) {
#pragma unroll
    for (int k = 0; k < PCK_GRP_MAX_PART; ++k) {
        const int f = rx_field(rec, k);
        const int q = f & 63, ef = (f >> 6) & 31, er = f >> 11;
        if (ef | er) {
            const double cf = nv.dyn[4 * q];
            const dd cq = two_prod(cf, in.y[q * in.ld_y + in.c]);
            if (k == k0) {
                a = ef ? dd_mul(dd_mul(dd_mul(a, dd_pow(cq, ef - 1)), cf), (double)ef) : dd_of(0.0);
                b = er ? dd_mul(dd_mul(dd_mul(b, dd_pow(cq, er - 1)), cf), (double)er) : dd_of(0.0);
            } else {
                if (ef) a = dd_mul(a, dd_pow(cq, ef));
                if (er) b = dd_mul(b, dd_pow(cq, er));
            }
        } else if (k == k0) {
            a = b = dd_of(0.0);
        }
    }
}
__device__ __forceinline__ dd sens_rate(const NetView& nv, const SensIn& in, const uint4& rec, dd a, dd b, int k0) {
    sens_sides(nv, in, rec, a, b, k0);
    return dd_sub(a, b);
}

template <int G>
__device__ __forceinline__ dd gbcast_dd(dd v, int src) { return {gbcast<G>(v.hi, src), gbcast<G>(v.lo, src)}; }

// LDS bytes of a 64-thread block: 64 / G matrices of G x G double-doubles
__host__ __device__ constexpr size_t sens_lds_bytes(int G) { return (size_t)(64 / G) * G * G * sizeof(dd); }

// What k_sens_adjoint writes beyond xi (pck_sens_out / pck_sens_dirs of the
// C-ABI): every pointer optional.  With s_j = cnt_j - sum_i lambda_i w_i S_ij
// the bracket of xi_j, rf_j / rr_j the forward / reverse rate of reaction j:
//   sf[j], sr[j]     rf_j s_j / TOF, -rr_j s_j / TOF                  [R][ld_s]
//   order[q]         sum_j s_j (ef_jq rf_j - er_jq rr_j) / TOF        [NFIX][ld_o]
//   order_in[i]      -lambda_i fl_i in_i / TOF (0 without a flow term) [NDYN][ld_oi]
//   dir[m]           sum_j s_j (rf_j a_mj - rr_j c_mj) / TOF          [nd][ld_dir]
//   err              2^-98 max_j max(rf_j, rr_j) / |TOF|              [n]
struct SensExt {
    double* sf; double* sr; int64_t ld_s;
    double* order; int64_t ld_o;
    double* order_in; int64_t ld_oi;
    const double* a; const double* c; int64_t ld_ac, s_ac;   // [nd][R][ld_ac], direction m at m * s_ac
    int nd;
    double* dir; int64_t ld_dir;
    double* err;
    double err_max;                                          // <= 0: no guard
};
#define PCK_SENS_ERR_UNIT 0x1p-98

// NaN into every output of SensExt of condition c, one lane per entry
template <int G>
__device__ __forceinline__ void sens_ext_nan(const NetView& nv, const SensExt& ex, int64_t c, int gl, bool with_err) {
    const double NaN = __builtin_nan("");
    for (int j = gl; j < nv.NRXN; j += G) {
        if (ex.sf) ex.sf[j * ex.ld_s + c] = NaN;
        if (ex.sr) ex.sr[j * ex.ld_s + c] = NaN;
    }
    if (ex.order)
        for (int q = gl; q < nv.NFIX; q += G) ex.order[q * ex.ld_o + c] = NaN;
    if (ex.order_in && gl < nv.NDYN) ex.order_in[gl * ex.ld_oi + c] = NaN;
    if (ex.dir)
        for (int m = gl; m < ex.nd; m += G) ex.dir[m * ex.ld_dir + c] = NaN;
    if (with_err && ex.err && gl == 0) ex.err[c] = NaN;
}

// The body of k_drc_adjoint (EXT = false: xi[j][ld_xi] for every active
// reaction, tof0 and status per condition) and of k_sens_adjoint (EXT = true:
// the outputs of SensExt as well, xi optional).  status_in (optional): only
// PCK_ST_OK conditions are computed, the others keep their status and get NaN
// outputs; tof0 is written for every condition.
template <int G, bool EXT>
__device__ __forceinline__ void sens_body(const NetView& nv, const GrpView& gv, const CondView& cv, const double* kf,
                                          const double* kr, int64_t ld_k, const double* yin, int64_t ld_y,
                                          const int32_t* status_in, double* xi, int64_t ld_xi, double* tof0,
                                          int32_t* status, const SensExt& ex) {
    extern __shared__ double lds[];
    const int grp = threadIdx.x / G, gl = threadIdx.x % G;
    const int64_t c = (int64_t)blockIdx.x * (64 / G) + grp;
    if (c >= cv.n) return;                         // group-uniform exit; no block barriers below
    const int NS = nv.NDYN, R = nv.NRXN;
    const bool row = gl < NS;
    dd* M = (dd*)lds + (size_t)grp * G * G;        // M[q * G + i] = A[i][q]
    const SensIn in{kf, kr, ld_k, yin, ld_y, cv.fixc, cv.ld_fix, cv.s_fix, c};
    const double NaN = __builtin_nan("");

    // TOF in double-double (old_system.py:482-488), the same bits on every lane
    dd tofp = dd_of(0.0);
    for (int t = gl; t < nv.NTOF; t += G) {
        const int r = nv.tof[t];
        dd a, b;
        sens_keff(nv, in, r, a, b);
        tofp = dd_add(tofp, sens_rate(nv, in, gv.rx[r], a, b, -1));
    }
    const dd tof = gsum_dd<G>(tofp);
    const double tofd = tof.hi + tof.lo;
    if (gl == 0 && tof0) tof0[c] = tofd;
    int st = status_in ? status_in[c] : PCK_ST_OK;
    if (st == PCK_ST_OK && !(isfinite(tofd) && tofd != 0.0)) st = PCK_ST_NONFINITE;
    if (st != PCK_ST_OK) {                         // group-uniform
        if (!EXT || xi)
            for (int j = gl; j < R; j += G) xi[j * ld_xi + c] = NaN;
        if constexpr (EXT) sens_ext_nan<G>(nv, ex, c, gl, true);
        if (gl == 0 && status) status[c] = st;
        return;
    }

    for (int q = 0; q < G; ++q) M[q * G + gl] = dd_of(0.0);
    // row gl of A into column gl of M, and the row's rate f
    double yi = 0.0, rs = 0.0;
    double flin = 0.0;                             // EXT: the inflow in_i of a row with a flow term
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
        if (fl != 0.0) {                            // the CSTR flow term fl (in - y)
            const double yin_i = cv.inflow ? cv.inflow[gl * cv.ld_in + c * cv.s_in] : 0.0;
            f = dd_add(f, dd_mul(two_sum(yin_i, -yi), fl));
            if constexpr (EXT) flin = yin_i;
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
    const double wi = (pv || pin) ? 0.0 : rs;      // b_j's weight on this row
    wsync();

    // g = d TOF / dy, lane q its own component
    dd g = dd_of(0.0);
    if (row) {
        for (int t = 0; t < nv.NTOF; ++t) {
            const int r = nv.tof[t];
            const uint4 rec = gv.rx[r];
            const int np = rx_np(rec);
            for (int k = 0; k < np; ++k) {
                if ((rx_field(rec, k) & 63) != gl) continue;
                dd a, b;
                sens_keff(nv, in, r, a, b);
                g = dd_add(g, sens_rate(nv, in, rec, a, b, k));
            }
        }
    }

    // equilibration by powers of two (exact): the columns of M (the rows of
    // A: rate rows up to 1e9, conservation rows O(1)), then its rows
    double dc = 1.0;
    for (int q = 0; q < NS; ++q) {
        const double s = inv_pow2(gmax<G>(row ? fabs(M[gl * G + q].hi) : 0.0));
        if (row) M[gl * G + q] = dd_scale(M[gl * G + q], s);
        if (q == gl) dc = s;
    }
    if (row) {
        double m = 0.0;
        for (int q = 0; q < NS; ++q) m = fmax(m, fabs(M[gl * G + q].hi));
        const double s = inv_pow2(m);
        for (int q = 0; q < NS; ++q) M[gl * G + q] = dd_scale(M[gl * G + q], s);
        g = dd_scale(g, s);
    }

    // LU with partial pivoting, row per lane, the right-hand side eliminated
    // along.  Rows are not moved: `step` is the column a row was the pivot of.
    int step = -1;
    bool ok = true;
    for (int k = 0; k < NS; ++k) {
        const bool fr = row && step < 0;
        double a = fr ? fabs(M[gl * G + k].hi) : -1.0;
        if (a != a) a = INFINITY;                  // a NaN must not hide behind fmax
        const double m = gmax<G>(a);
        if (!(m > 0.0) || !isfinite(m)) { ok = false; break; }    // group-uniform
        const int p = (G - 1) - gmaxi<G>((fr && a == m) ? (G - 1) - gl : -1);     // the lowest such lane
        if (gl == p) step = k;
        const dd piv = M[p * G + k];
        const dd gp = gbcast_dd<G>(g, p);
        if (fr && gl != p) {
            const dd l = dd_div(M[gl * G + k], piv);
            for (int q = k + 1; q < NS; ++q) M[gl * G + q] = dd_sub(M[gl * G + q], dd_mul(l, M[p * G + q]));
            g = dd_sub(g, dd_mul(l, gp));
        }
        wsync();                                   // the next pivot row is complete before it is read
    }
    // back substitution: lane k keeps lambda_k
    dd lam = dd_of(0.0);
    if (ok) {
        for (int k = NS - 1; k >= 0; --k) {
            const int p = gmaxi<G>((row && step == k) ? gl : -1);
            const dd x = dd_div(gbcast_dd<G>(g, p), M[p * G + k]);
            if (gl == k) lam = x;
            if (row && step < k) g = dd_sub(g, dd_mul(M[gl * G + k], x));
        }
    }
    const double lsum = lam.hi + lam.lo;
    ok = ok && gmin<G>((!row || isfinite(lsum)) ? 1.0 : 0.0) > 0.0;
    if (!ok) {
        if (!EXT || xi)
            for (int j = gl; j < R; j += G) xi[j * ld_xi + c] = NaN;
        if constexpr (EXT) sens_ext_nan<G>(nv, ex, c, gl, true);
        if (gl == 0 && status) status[c] = PCK_ST_SENS_SINGULAR;
        return;
    }
    // lambda_i x (b_j's row weight) where every lane can read it: the matrix is done
    wsync();
    if (row) M[gl] = dd_mul(dd_scale(lam, dc), wi);
    wsync();
    // the bracket s_j = [j in tof] - sum_i lambda_i w_i S_ij and the two sides of reaction j
    auto terms = [&](int j, dd& rf, dd& rr) -> dd {
        sens_keff(nv, in, j, rf, rr);
        sens_sides(nv, in, gv.rx[j], rf, rr, -1);
        int cnt = 0;
        for (int t = 0; t < nv.NTOF; ++t) cnt += (nv.tof[t] == j);
        dd s = dd_of((double)cnt);
        for (int i = 0; i < NS; ++i) {
            const double sv = nv.S[i * R + j];
            if (sv != 0.0) s = dd_sub(s, dd_mul(M[i], sv));
        }
        return s;
    };
    // xi_j = net_j s_j / TOF, lane per reaction
    double rmax = 0.0;
    for (int j = gl; j < R; j += G) {
        dd rf, rr;
        const dd s = terms(j, rf, rr);
        if (!EXT || xi) {
            const dd x = dd_div(dd_mul(dd_sub(rf, rr), s), tof);
            xi[j * ld_xi + c] = x.hi + x.lo;
        }
        if constexpr (EXT) {
            const double m = fmax(fabs(rf.hi), fabs(rr.hi));
            rmax = (m != m) ? INFINITY : fmax(rmax, m);
        }
    }
    if constexpr (EXT) {
        // the guard: sf_j needs s_j to TOF / rf_j absolute, and the double-double
        // lambda gives it to ~2^-98 (DESIGN.md "Adjoint sensitivities")
        const double err = PCK_SENS_ERR_UNIT * gmax<G>(rmax) / fabs(tofd);
        if (gl == 0 && ex.err) ex.err[c] = err;
        if (ex.err_max > 0.0 && !(err <= ex.err_max)) {          // group-uniform
            sens_ext_nan<G>(nv, ex, c, gl, false);
            if (gl == 0 && status) status[c] = PCK_ST_SENS_PRECISION;
            return;
        }
        if (ex.sf || ex.sr) {
            for (int j = gl; j < R; j += G) {
                dd rf, rr;
                const dd s = terms(j, rf, rr);
                const dd xf = dd_div(dd_mul(rf, s), tof), xr = dd_div(dd_mul(rr, s), tof);
                if (ex.sf) ex.sf[j * ex.ld_s + c] = xf.hi + xf.lo;
                if (ex.sr) ex.sr[j * ex.ld_s + c] = -(xr.hi + xr.lo);
            }
        }
        // reaction orders in the fixed species: the group's lanes share the sum over j
        if (ex.order) {
            for (int q = 0; q < nv.NFIX; ++q) {
                dd acc = dd_of(0.0);
                for (int j = gl; j < R; j += G) {
                    const int ea = nv.foldf[j * nv.NFIX + q], eb = nv.foldr[j * nv.NFIX + q];
                    if (!(ea | eb)) continue;
                    dd rf, rr;
                    const dd s = terms(j, rf, rr);
                    acc = dd_add(acc, dd_mul(s, dd_sub(dd_mul(rf, (double)ea), dd_mul(rr, (double)eb))));
                }
                const dd x = dd_div(gsum_dd<G>(acc), tof);
                if (gl == 0) ex.order[q * ex.ld_o + c] = x.hi + x.lo;
            }
        }
        // ... and in the inflow of a species with a flow term (not scaled by the row scale)
        if (ex.order_in && row) {
            const double fl = nv.dyn[4 * gl + 3];
            dd x = dd_of(0.0);
            if (fl != 0.0 && !(pv || pin)) x = dd_div(dd_mul(dd_mul(dd_scale(lam, dc), -fl), flin), tof);
            ex.order_in[gl * ex.ld_oi + c] = x.hi + x.lo;
        }
        // user directions (d ln kf, d ln kr)
        if (ex.dir) {
            for (int m = 0; m < ex.nd; ++m) {
                const double* am = ex.a + m * ex.s_ac;
                const double* cm = ex.c + m * ex.s_ac;
                dd acc = dd_of(0.0);
                for (int j = gl; j < R; j += G) {
                    dd rf, rr;
                    const dd s = terms(j, rf, rr);
                    acc = dd_add(acc, dd_mul(s, dd_sub(dd_mul(rf, am[j * ex.ld_ac + c]), dd_mul(rr, cm[j * ex.ld_ac + c]))));
                }
                const dd x = dd_div(gsum_dd<G>(acc), tof);
                if (gl == 0) ex.dir[m * ex.ld_dir + c] = x.hi + x.lo;
            }
        }
    }
    if (gl == 0 && status) status[c] = PCK_ST_OK;
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
