// The adjoint core of the sensitivity kernels: A^T lambda = g at a steady
// state in double-double (mk_device.h: dd), and the outputs that follow lambda.
// A, b_j and the replaced rows are posed in mk_sens.h.
//
// For every kernel (group and one-lane): the double-double helpers, SensIn,
// sens_keff / sens_sides / sens_rate, SensExt.  For the group kernels of
// mk_sens.h and mk_sens_multi.h (G = 16 / 32 / 64 lanes per condition, lane i
// owns species i and row i of M = A^T, M[q * G + i] = A[i][q] in LDS, every exit
// group-uniform) the four steps, once:
//   grp_assemble     row i of A into column i of M, rows replaced
//   grp_equilibrate  columns, then rows, by powers of two (exact)
//   grp_factor       LU with partial pivoting, rows not moved; CARRY: the one g
//                    of a single-objective kernel is eliminated along, else the
//                    multipliers are stored for grp_solve's replay
//   grp_solve        (replay of the elimination on g, then) back substitution
// and the single-objective kernels' gate and outputs (sens_gate, sens_tail,
// sens_ext_nan).  The one-lane kernels (mk_sens_lane.h, mk_sens_multi_lane.h)
// keep their own serial text of the steps (DESIGN.md "Adjoint core").
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
// forward / reverse rate of reaction j
__device__ __forceinline__ void sens_fr(const NetView& nv, const GrpView& gv, const SensIn& in, int j, dd& rf, dd& rr) {
    sens_keff(nv, in, j, rf, rr);
    sens_sides(nv, in, gv.rx[j], rf, rr, -1);
}

// the row scale of species i at temperature T (reactor.py:34-41, as mk_group.h: grp_setup)
__device__ __forceinline__ double adj_rs(const NetView& nv, int i, double T) {
    const double* d = nv.dyn + 4 * i;
    return (d[2] != 0.0) ? d[1] + d[2] * T : d[1];
}
// the conservation law whose pivot row is row i, or -1
__device__ __forceinline__ int adj_law(const NetView& nv, int i) {
    int law = -1;
    for (int l = 0; l < nv.NCONS; ++l)
        if (nv.cpiv[l] == i) law = l;
    return law;
}
__device__ __forceinline__ double adj_inflow(const CondView& cv, int i, int64_t c) {
    return cv.inflow ? cv.inflow[i * cv.ld_in + c * cv.s_in] : 0.0;
}

// the bracket s_j = s0 - sum_i lambda_i w_i S_ij of xi_j; lw(i) = lambda_i w_i
template <class LW>
__device__ __forceinline__ dd adj_bracket(const NetView& nv, int j, double s0, LW lw) {
    dd s = dd_of(s0);
    for (int i = 0; i < nv.NDYN; ++i) {
        const double sv = nv.S[i * nv.NRXN + j];
        if (sv != 0.0) s = dd_sub(s, dd_mul(lw(i), sv));
    }
    return s;
}

// ----------------------------------------------------------------------------
// the group schedule
// ----------------------------------------------------------------------------
template <int G>
__device__ __forceinline__ dd gbcast_dd(dd v, int src) { return {gbcast<G>(v.hi, src), gbcast<G>(v.lo, src)}; }

// Zero M, then row gl of A into column gl of M and the row's rate f.  Rows
// are replaced as in mk_solver.h: newton -- the conservation laws in their
// pivot rows, a unit row for a pinned species (newton_pinned).  True if the
// lane's row was replaced; rs: its row scale (0 on a lane without a row; b_j's
// weight w_i on the row is rs, or 0 if replaced).
template <int G>
__device__ __forceinline__ bool grp_assemble(const NetView& nv, const GrpView& gv, const CondView& cv, const SensIn& in,
                                             dd* M, int gl, bool row, double& rs) {
    const int NS = nv.NDYN;
    for (int q = 0; q < G; ++q) M[q * G + gl] = dd_of(0.0);
    double yi = 0.0;
    rs = 0.0;
    int law = -1;
    dd f = dd_of(0.0);
    if (row) {
        rs = adj_rs(nv, gl, cv.T[in.c * cv.sT]);
        const double fl = nv.dyn[4 * gl + 3];
        yi = in.y[gl * in.ld_y + in.c];
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
            f = dd_add(f, dd_mul(two_sum(adj_inflow(cv, gl, in.c), -yi), fl));
            M[gl * G + gl] = dd_add(M[gl * G + gl], dd_of(-fl));
        }
        law = adj_law(nv, gl);
    }
    const bool pv = law >= 0;
    const bool pin = row && !pv && yi == 0.0 && f.hi == 0.0 && f.lo == 0.0;
    if (pv)
        for (int q = 0; q < NS; ++q) M[q * G + gl] = dd_of(nv.C[law * NS + q]);
    if (pin)
        for (int q = 0; q < NS; ++q) M[q * G + gl] = dd_of(q == gl ? 1.0 : 0.0);
    wsync();
    return pv || pin;
}

// dJ/dy of reaction r's net rate (times w if W) added to g, lane q its own component
template <bool W>
__device__ __forceinline__ void grp_g_add(const NetView& nv, const GrpView& gv, const SensIn& in, int r, double w, int gl,
                                          dd& g) {
    const uint4 rec = gv.rx[r];
    const int np = rx_np(rec);
    for (int k = 0; k < np; ++k) {
        if ((rx_field(rec, k) & 63) != gl) continue;
        dd a, b;
        sens_keff(nv, in, r, a, b);
        const dd v = sens_rate(nv, in, rec, a, b, k);
        g = dd_add(g, W ? dd_mul(v, w) : v);
    }
}

// Equilibration by powers of two (exact): the columns of M (the rows of A:
// rate rows up to 1e9, conservation rows O(1)), then its rows.  dc: the scale
// of column gl; sr: the scale of row gl, which the caller applies to g.
template <int G>
__device__ __forceinline__ void grp_equilibrate(dd* M, int NS, int gl, bool row, double& dc, double& sr) {
    dc = sr = 1.0;
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
}

// LU with partial pivoting, row per lane.  Rows are not moved: `step` is the
// column a row was the pivot of.  The multiplier of a row stays in the entry
// it annihilates.  False (group-uniform) on a zero or non-finite pivot.
// CARRY: the right-hand side g (lane q its own component) is eliminated along
// and no multiplier is kept -- the single-objective kernels' one solve without
// the replay of grp_solve, which costs them a second pass of NS dependent
// steps (DESIGN.md "Adjoint core").
template <int G, bool CARRY>
__device__ __forceinline__ bool grp_factor(dd* M, int NS, int gl, bool row, int& step, dd& g) {
    step = -1;
    for (int k = 0; k < NS; ++k) {
        const bool fr = row && step < 0;
        double a = fr ? fabs(M[gl * G + k].hi) : -1.0;
        if (a != a) a = INFINITY;                  // a NaN must not hide behind fmax
        const double m = gmax<G>(a);
        if (!(m > 0.0) || !isfinite(m)) return false;
        const int p = (G - 1) - gmaxi<G>((fr && a == m) ? (G - 1) - gl : -1);     // the lowest such lane
        if (gl == p) step = k;
        const dd piv = M[p * G + k];
        dd gp;
        if constexpr (CARRY) gp = gbcast_dd<G>(g, p);
        if (fr && gl != p) {
            const dd l = dd_div(M[gl * G + k], piv);
            for (int q = k + 1; q < NS; ++q) M[gl * G + q] = dd_sub(M[gl * G + q], dd_mul(l, M[p * G + q]));
            if constexpr (CARRY) g = dd_sub(g, dd_mul(l, gp));
            else M[gl * G + k] = l;
        }
        wsync();                                   // the next pivot row is complete before it is read
    }
    return true;
}
// no non-finite factor anywhere in L or U (group-uniform)
template <int G>
__device__ __forceinline__ bool grp_factor_finite(const dd* M, int NS, int gl, bool row) {
    double fin = 1.0;
    if (row)
        for (int q = 0; q < NS; ++q) fin = isfinite(M[gl * G + q].hi + M[gl * G + q].lo) ? fin : 0.0;
    return gmin<G>(fin) > 0.0;
}

// lambda of A^T lambda = g (g: lane q its own component, in the row scale of
// M; CARRIED: already eliminated by grp_factor<G, true>), lane k its lambda_k in
// the column scale of M.
template <int G, bool CARRIED>
__device__ __forceinline__ dd grp_solve(const dd* M, int NS, int gl, bool row, int step, dd g) {
    // the forward elimination replayed from the stored multipliers: at step
    // k every row still free then, the pivot apart, subtracts l g_pivot
    if constexpr (!CARRIED)
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
    return lam;
}
// every lambda_k finite (group-uniform)
template <int G>
__device__ __forceinline__ bool grp_finite(dd lam, bool row) {
    const double lsum = lam.hi + lam.lo;
    return gmin<G>((!row || isfinite(lsum)) ? 1.0 : 0.0) > 0.0;
}

// ----------------------------------------------------------------------------
// the single-objective group kernels (mk_sens.h): gate and outputs, G lanes
// per condition, lane gl of them
// ----------------------------------------------------------------------------
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
// a condition without sensitivities: NaN into xi and (EXT) every output of SensExt, its status st
template <int G, bool EXT>
__device__ __forceinline__ void sens_fail(const NetView& nv, const SensExt& ex, int64_t c, int gl, double* xi,
                                          int64_t ld_xi, int32_t* status, int st) {
    if (!EXT || xi)
        for (int j = gl; j < nv.NRXN; j += G) xi[j * ld_xi + c] = __builtin_nan("");
    if constexpr (EXT) sens_ext_nan<G>(nv, ex, c, gl, true);
    if (gl == 0 && status) status[c] = st;
}

// The TOF in double-double (old_system.py:482-488), the same bits on every
// lane, into tof and tof0 (written for every condition).  status_in
// (optional): only PCK_ST_OK conditions are computed, the others keep their
// status and get NaN outputs, as a condition with a zero or non-finite TOF
// (PCK_ST_NONFINITE) does.  False (uniform over the G lanes) for those.
template <int G, bool EXT>
__device__ __forceinline__ bool sens_gate(const NetView& nv, const GrpView& gv, const SensIn& in, const SensExt& ex,
                                          const int32_t* status_in, int gl, double* xi, int64_t ld_xi, double* tof0,
                                          int32_t* status, dd& tof) {
    dd tofp = dd_of(0.0);
    for (int t = gl; t < nv.NTOF; t += G) {
        const int r = nv.tof[t];
        dd a, b;
        sens_keff(nv, in, r, a, b);
        tofp = dd_add(tofp, sens_rate(nv, in, gv.rx[r], a, b, -1));
    }
    tof = gsum_dd<G>(tofp);
    const double tofd = tof.hi + tof.lo;
    if (gl == 0 && tof0) tof0[in.c] = tofd;
    int st = status_in ? status_in[in.c] : PCK_ST_OK;
    if (st == PCK_ST_OK && !(isfinite(tofd) && tofd != 0.0)) st = PCK_ST_NONFINITE;
    if (st == PCK_ST_OK) return true;
    sens_fail<G, EXT>(nv, ex, in.c, gl, xi, ld_xi, status, st);
    return false;
}

// Everything after lambda: xi_j = net_j s_j / TOF and (EXT) the guard and the
// outputs of SensExt, then the status.  LW[i] = lambda_i w_i, readable by every
// lane (LDS); lam = lambda_gl and repl = row gl was replaced, the lane's own.
// Sums over j: strided partials, then gsum_dd.
template <int G, bool EXT>
__device__ __forceinline__ void sens_tail(const NetView& nv, const GrpView& gv, const CondView& cv, const SensIn& in,
                                          const SensExt& ex, int gl, dd tof, double* xi, int64_t ld_xi,
                                          int32_t* status, const dd* LW, dd lam, bool repl) {
    const int R = nv.NRXN;
    const int64_t c = in.c;
    // the bracket s_j = [j in tof] - sum_i lambda_i w_i S_ij and the two sides of reaction j
    auto terms = [&](int j, dd& rf, dd& rr) -> dd {
        sens_fr(nv, gv, in, j, rf, rr);
        int cnt = 0;
        for (int t = 0; t < nv.NTOF; ++t) cnt += (nv.tof[t] == j);
        return adj_bracket(nv, j, (double)cnt, [&](int i) { return LW[i]; });
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
        const double err = PCK_SENS_ERR_UNIT * gmax<G>(rmax) / fabs(tof.hi + tof.lo);
        if (gl == 0 && ex.err) ex.err[c] = err;
        if (ex.err_max > 0.0 && !(err <= ex.err_max)) {          // uniform over the G lanes
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
        // reaction orders in the fixed species: the lanes share the sum over j
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
        if (ex.order_in && gl < nv.NDYN) {
            const double fl = nv.dyn[4 * gl + 3];
            dd x = dd_of(0.0);
            if (fl != 0.0 && !repl) x = dd_div(dd_mul(dd_mul(lam, -fl), adj_inflow(cv, gl, c)), tof);
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

}  // namespace pck
