// Bed DRC: the multi-objective adjoint of mk_sens_multi_lane.h swept backward
// through the cells of a reactor cascade (mk_cascade.h), one lane per
// condition, one launch (pck_cascade_drc_at; DESIGN.md "Bed DRC").
//
// A bed of N cells at one condition: y_c the state of cell c, u_c its inflow on
// the flow rows (cond->inflow for c = 0, y_{c-1} else), F(y_c, u_c, k) = 0 the
// steady equations of one cell as mk_sens_multi_lane.h poses them, A_c = dF/dy.
//   J_m = (1/N) sum_c sum_j wr[m][j] net_j(y_c) + sum_i wy[m][i] y_{N-1,i}
// The kernel carries nu = N mu, so that nothing is divided before the end:
//   A_c^T nu_{m,c} = sum_j wr[m][j] dnet_j/dy (y_c) + [c = N-1] N wy[m]
//                    - phi_{c+1} (.) nu_{m,c+1}                 c = N-1 ... 0
//   acc[m][j] = sum_c net_j(y_c) (wr[m][j] - sum_i nu_{m,c,i} w_{c,i} S_ij)
//   D_m = sum_c sum_j wr[m][j] net_j(y_c) + N sum_i wy[m][i] y_{N-1,i}   (= N J_m)
//   xi[m][j] = acc[m][j] / D_m,   order_in[m][i] = -nu_{m,0,i} phi_{0,i} u_{0,i} / D_m
// w_{c,i} the row scale, phi_{c,i} the flow rate fl_i, each 0 where row i of cell
// c was replaced.  For N = 1 this is k_lane_multi_adjoint statement for
// statement.  All double-double, the sums over the cells included.
//
// Per cell: assembly, row replacement, equilibration and the LU with its
// multipliers kept are k_lane_multi_adjoint's text (DESIGN.md "Adjoint core":
// why the one-lane kernels keep their own); then per objective the right-hand
// side, the replayed elimination, the back substitution and the cell's terms.
// LDS as there: entry e of lane l at double-double index e * 64 + l, (NS^2 +
// 2 NS) entries, sized by NS alone.  What a lane carries from cell to cell and
// cannot keep in registers (K is a run-time count) lives in a device workspace
// of double-doubles laid out [row][ld_ws], a wavefront's access contiguous:
//   rows [0, K NS)                 nu_{m,c+1}, row m NS + i
//   rows [K NS, K NS + K R)        acc[m][j]
//   rows [.., + K)                 sum_c sum_j wr[m][j] net_j(y_c)
//   rows [.., + K)                 hi != 0: an adjoint solve of objective m overflowed
// The cell loop's trip count is the launch's; a gated or failed lane skips the
// work of its trips by predication.  No barrier, no atomics, no cross-lane
// operation: a condition's result does not depend on its lane, its block or
// the size of the batch.
//
// The kernel is k_bed_adjoint, not k_cascade_*: tests/test_cascade_kernel_budget.py
// counts the code object's kernels whose name contains "k_cascade" as the
// instances of the solve kernel.
#pragma once
#include "mk_sens_multi.h"

namespace pck {

// the budget of mk_sens_multi_lane.h: 16 (NS^2 + 2 NS) 64 bytes per block
__host__ __device__ constexpr size_t cascade_adjoint_lds_bytes(int NS) {
    return (size_t)(NS * NS + 2 * NS) * 64 * sizeof(dd);
}
typedef double cadj_v2d __attribute__((ext_vector_type(2)));    // one 16-byte access per double-double
// rows of the workspace, each ld_ws double-doubles
__host__ __device__ constexpr int64_t cascade_adjoint_ws_rows(int K, int NS, int R) {
    return (int64_t)K * (NS + R + 2);
}

struct CascadeAdj {
    const double* y_cells; int64_t ld_yc;     // [cells][NS][ld_yc]
    const int32_t* status_cells; int64_t ld_c;   // [cells][ld_c] or null
    int cells;
    double* order_in; int64_t ld_oi;          // [K * NS][ld_oi] or null
    cadj_v2d* ws; int64_t ld_ws;             // cascade_adjoint_ws_rows(K, NS, R) rows
};

#define PCK_SIG_CASCADE_ADJOINT \
    NetView nv, GrpView gv, CondView cv, const double *kf, const double *kr, int64_t ld_k, CascadeAdj ca, MultiObj ob, MultiOut out

// (the split build, csrc/mk_inst.h: defined in tu_cascade_adjoint.hip, declared where it is launched)
#if defined(PCK_SPLIT_TU) && PCK_SPLIT_TU && !defined(PCK_KERNEL_TU)
__global__ void k_bed_adjoint(PCK_SIG_CASCADE_ADJOINT);
#else

__global__ void __launch_bounds__(64) k_bed_adjoint(PCK_SIG_CASCADE_ADJOINT) {
    extern __shared__ __attribute__((aligned(16))) cadj_v2d lds_cadj[];
    const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (c >= cv.n) return;                         // per lane, as every exit below: no barrier anywhere
    const int NS = nv.NDYN, R = nv.NRXN, K = ob.K, N = ca.cells;
    cadj_v2d* const L = lds_cadj + threadIdx.x;
    auto ld = [&](int e) -> dd { const cadj_v2d v = L[e * 64]; return dd{v.x, v.y}; };
    auto put = [&](int e, dd v) { L[e * 64] = cadj_v2d{v.hi, v.lo}; };
    cadj_v2d* const W = ca.ws + c;
    auto wld = [&](int64_t row) -> dd { const cadj_v2d v = W[row * ca.ld_ws]; return dd{v.x, v.y}; };
    auto wput = [&](int64_t row, dd v) { W[row * ca.ld_ws] = cadj_v2d{v.hi, v.lo}; };
    const int eG = NS * NS, eW = NS * NS + NS;
    const int64_t wXI = (int64_t)K * NS, wJ = wXI + (int64_t)K * R, wF = wJ + K;
    const double NaN = __builtin_nan("");
    const double T = cv.T[c * cv.sT];

    // the gate, pck_solve_cascade's summary: the first failing status (1..3) in cell order, else the largest
    // other status that is not PCK_ST_OK (PCK_ST_NEWTON)
    int st = PCK_ST_OK;
    if (ca.status_cells) {
        int bad = 0, other = 0;
        for (int cell = 0; cell < N; ++cell) {
            const int s = ca.status_cells[(int64_t)cell * ca.ld_c + c];
            if (s >= PCK_ST_MAXSTEPS && s <= PCK_ST_NONFINITE) bad = bad ? bad : s;
            else if (s != PCK_ST_OK) other = s > other ? s : other;
        }
        st = bad ? bad : other;
    }
    bool fin_y = true;                             // every cell state finite: val is defined
    unsigned repl_dn = 0;                          // the replaced rows of cell + 1 (phi_{c+1})

    for (int cell = N - 1; cell >= 0; --cell) {
        const double* ycell = ca.y_cells + (int64_t)cell * NS * ca.ld_yc;
        const double* yup = cell > 0 ? ycell - (int64_t)NS * ca.ld_yc : nullptr;
        const SensIn in{kf, kr, ld_k, ycell, ca.ld_yc, cv.fixc, cv.ld_fix, cv.s_fix, c};
        const bool last = cell == N - 1;
        for (int i = 0; i < NS; ++i) fin_y = fin_y && isfinite(ycell[i * ca.ld_yc + c]);

        unsigned repl = 0;                         // bit i: row i is replaced
        unsigned stp = 0xffffffffu, rof = 0u;      // the pivot bookkeeping (below)
        if (st == PCK_ST_OK) {
            for (int e = 0; e < eG; ++e) put(e, dd_of(0.0));
            // row i of A into column i of M; rows replaced as in mk_solver.h: newton --
            // the conservation laws in their pivot rows, a unit row for a pinned species
            for (int i = 0; i < NS; ++i) {
                const double rs = adj_rs(nv, i, T);
                const double fl = nv.dyn[4 * i + 3];
                const double yi = ycell[i * ca.ld_yc + c];
                dd f = dd_of(0.0);
                for (int e = gv.row[i]; e < gv.row[i + 1]; ++e) {
                    const uint4 q4 = gv.ent[e];
                    const int r = ent_r(q4), np = ent_np(q4);
                    const dd w = two_prod(rs, ent_s(q4));
                    const uint4 rec = gv.rx[r];
                    dd a, b;
                    sens_keff(nv, in, r, a, b);
                    f = dd_add(f, dd_mul(w, sens_rate(nv, in, rec, a, b, -1)));
                    for (int k = 0; k < np; ++k) {
                        const int m = ent_species(q4, k) * NS + i;
                        put(m, dd_add(ld(m), dd_mul(w, sens_rate(nv, in, rec, a, b, k))));
                    }
                }
                if (fl != 0.0) {                    // the flow term fl (u - y), u the upstream cell's state
                    const double ui = yup ? yup[i * ca.ld_yc + c] : adj_inflow(cv, i, c);
                    f = dd_add(f, dd_mul(two_sum(ui, -yi), fl));
                    put(i * NS + i, dd_add(ld(i * NS + i), dd_of(-fl)));
                }
                const int law = adj_law(nv, i);
                const bool pv = law >= 0;
                const bool pin = !pv && yi == 0.0 && f.hi == 0.0 && f.lo == 0.0;
                if (pv)
                    for (int q = 0; q < NS; ++q) put(q * NS + i, dd_of(nv.C[law * NS + q]));
                if (pin)
                    for (int q = 0; q < NS; ++q) put(q * NS + i, dd_of(q == i ? 1.0 : 0.0));
                if (pv || pin) repl |= 1u << i;
            }

            // equilibration by powers of two (exact): the columns of M, then its rows
            for (int q = 0; q < NS; ++q) {
                double m = 0.0;
                for (int r = 0; r < NS; ++r) m = fmax(m, fabs(ld(r * NS + q).hi));
                const double s = inv_pow2(m);
                for (int r = 0; r < NS; ++r) put(r * NS + q, dd_scale(ld(r * NS + q), s));
                put(eW + q, dd{s, 1.0});
            }
            for (int r = 0; r < NS; ++r) {
                double m = 0.0;
                for (int q = 0; q < NS; ++q) m = fmax(m, fabs(ld(r * NS + q).hi));
                const double s = inv_pow2(m);
                for (int q = 0; q < NS; ++q) put(r * NS + q, dd_scale(ld(r * NS + q), s));
                put(eW + r, dd{ld(eW + r).hi, s});
            }

            // LU with partial pivoting, rows not moved, the multipliers kept
            // (mk_sens_multi_lane.h: stp, rof)
            bool ok = true;
            for (int k = 0; k < NS; ++k) {
                double m = -1.0;
                int p = 0;
                for (int r = 0; r < NS; ++r) {
                    if (((stp >> (4 * r)) & 15u) != 15u) continue;
                    double a = fabs(ld(r * NS + k).hi);
                    if (a != a) a = INFINITY;          // a NaN must not hide behind the maximum
                    if (a > m) { m = a; p = r; }       // the lowest such row
                }
                if (!(m > 0.0) || !isfinite(m)) { ok = false; break; }
                stp = (stp & ~(15u << (4 * p))) | ((unsigned)k << (4 * p));
                rof |= (unsigned)p << (4 * k);
                const dd piv = ld(p * NS + k);
                for (int r = 0; r < NS; ++r) {
                    if (((stp >> (4 * r)) & 15u) != 15u) continue;
                    const dd l = dd_div(ld(r * NS + k), piv);
                    for (int q = k + 1; q < NS; ++q) put(r * NS + q, dd_sub(ld(r * NS + q), dd_mul(l, ld(p * NS + q))));
                    put(r * NS + k, l);
                }
            }
            if (ok)
                for (int e = 0; e < eG; ++e) {
                    const dd v = ld(e);
                    ok = ok && isfinite(v.hi + v.lo);
                }
            if (!ok) st = PCK_ST_SENS_SINGULAR;
        }

        // forward / reverse side of reaction j in this cell
        auto sides = [&](int j, dd& rf, dd& rr) {
            sens_keff(nv, in, j, rf, rr);
            sens_sides(nv, in, gv.rx[j], rf, rr, -1);
        };
        for (int m = 0; m < K; ++m) {
            const double* wr = ob.wr ? ob.wr + (int64_t)m * R : nullptr;
            const double* wy = ob.wy ? ob.wy + (int64_t)m * NS : nullptr;
            // the rate part of J_m, summed over the cells (every lane: val is written for a gated bed too)
            {
                dd J = last ? dd_of(0.0) : wld(wJ + m);
                if (wr)
                    for (int j = 0; j < R; ++j) {
                        const double w = wr[j];
                        if (w == 0.0) continue;
                        dd rf, rr;
                        sides(j, rf, rr);
                        J = dd_add(J, dd_mul(dd_sub(rf, rr), w));
                    }
                wput(wJ + m, J);
            }
            if (st != PCK_ST_OK) continue;

            // the right-hand side in the row scale of M
            for (int q = 0; q < NS; ++q) put(eG + q, (wy && last) ? two_prod(wy[q], (double)N) : dd_of(0.0));
            if (wr)
                for (int j = 0; j < R; ++j) {
                    const double w = wr[j];
                    if (w == 0.0) continue;
                    const uint4 rec = gv.rx[j];
                    const int np = rx_np(rec);
                    dd a, b;
                    sens_keff(nv, in, j, a, b);
                    for (int k = 0; k < np; ++k) {
                        const int q = rx_field(rec, k) & 63;
                        if (q >= NS) continue;
                        put(eG + q, dd_add(ld(eG + q), dd_mul(sens_rate(nv, in, rec, a, b, k), w)));
                    }
                }
            if (!last)                             // - phi_{c+1} (.) nu_{m,c+1}
                for (int q = 0; q < NS; ++q) {
                    const double fl = nv.dyn[4 * q + 3];
                    if (fl != 0.0 && !((repl_dn >> q) & 1u))
                        put(eG + q, dd_sub(ld(eG + q), dd_mul(wld((int64_t)m * NS + q), fl)));
                }
            for (int q = 0; q < NS; ++q) put(eG + q, dd_scale(ld(eG + q), ld(eW + q).lo));
            // the forward elimination replayed from the stored multipliers
            for (int k = 0; k < NS; ++k) {
                const dd gp = ld(eG + (int)((rof >> (4 * k)) & 15u));
                for (int r = 0; r < NS; ++r)
                    if ((int)((stp >> (4 * r)) & 15u) > k) put(eG + r, dd_sub(ld(eG + r), dd_mul(ld(r * NS + k), gp)));
            }
            // back substitution: nu_k into the g slot of its pivot row
            bool fin = true;
            for (int k = NS - 1; k >= 0; --k) {
                const int p = (int)((rof >> (4 * k)) & 15u);
                const dd x = dd_div(ld(eG + p), ld(p * NS + k));
                for (int r = 0; r < NS; ++r)
                    if ((int)((stp >> (4 * r)) & 15u) < k) put(eG + r, dd_sub(ld(eG + r), dd_mul(ld(r * NS + k), x)));
                put(eG + p, x);
                const double lsum = x.hi + x.lo;
                fin = fin && isfinite(lsum);
            }
            // an overflow fails this objective alone, here and in every cell upstream
            {
                const double f0 = last ? 0.0 : wld(wF + m).hi;
                wput(wF + m, dd_of((f0 != 0.0 || !fin) ? 1.0 : 0.0));
            }
            // nu_mi scaled back and stored for the next trip; times the row weight, parked over nu_mi
            for (int i = 0; i < NS; ++i) {
                const int p = (int)((rof >> (4 * i)) & 15u);
                const dd nu = dd_scale(ld(eG + p), ld(eW + i).hi);
                wput((int64_t)m * NS + i, nu);
                put(eG + p, dd_mul(nu, ((repl >> i) & 1u) ? 0.0 : adj_rs(nv, i, T)));
            }
            // the cell's term of acc[m][j]
            for (int j = 0; j < R; ++j) {
                dd rf, rr;
                sides(j, rf, rr);
                const dd s = adj_bracket(nv, j, wr ? wr[j] : 0.0,
                                         [&](int i) { return ld(eG + (int)((rof >> (4 * i)) & 15u)); });
                const dd x = dd_mul(dd_sub(rf, rr), s);
                wput(wXI + (int64_t)m * R + j, last ? x : dd_add(wld(wXI + (int64_t)m * R + j), x));
            }
        }
        repl_dn = repl;
    }
    if (out.status) out.status[c] = st;

    // the outputs: repl_dn is cell 0's mask now, the nu rows hold nu_{m,0}
    const double* yout = ca.y_cells + (int64_t)(N - 1) * NS * ca.ld_yc;
    for (int m = 0; m < K; ++m) {
        const double* wy = ob.wy ? ob.wy + (int64_t)m * NS : nullptr;
        double* xi = out.xi + (int64_t)m * R * out.ld_xi + c;
        double* oi = ca.order_in ? ca.order_in + (int64_t)m * NS * ca.ld_oi + c : nullptr;
        // D_m = N J_m: the rate sum over the cells, then the outlet terms in index order
        const dd Jr = wld(wJ + m);
        dd D = Jr, J = dd_div(Jr, dd_of((double)N));
        if (wy)
            for (int i = 0; i < NS; ++i) {
                const dd t = two_prod(wy[i], yout[i * ca.ld_yc + c]);
                J = dd_add(J, t);
                D = dd_add(D, dd_mul(t, (double)N));
            }
        const double Jd = J.hi + J.lo;
        out.val[m * out.ld_val + c] = fin_y ? Jd : NaN;
        int so = st;
        if (so == PCK_ST_OK && !(isfinite(Jd) && Jd != 0.0)) so = PCK_ST_NONFINITE;
        if (so == PCK_ST_OK && wld(wF + m).hi != 0.0) so = PCK_ST_NONFINITE;
        if (out.ostatus) out.ostatus[m * out.ld_os + c] = so;
        if (so != PCK_ST_OK) {
            for (int j = 0; j < R; ++j) xi[j * out.ld_xi] = NaN;
            if (oi)
                for (int i = 0; i < NS; ++i) oi[i * ca.ld_oi] = NaN;
            continue;
        }
        for (int j = 0; j < R; ++j) {
            const dd x = dd_div(wld(wXI + (int64_t)m * R + j), D);
            xi[j * out.ld_xi] = x.hi + x.lo;
        }
        if (oi)
            for (int i = 0; i < NS; ++i) {
                const double fl = nv.dyn[4 * i + 3];
                dd x = dd_of(0.0);
                if (fl != 0.0 && !((repl_dn >> i) & 1u))
                    x = dd_div(dd_mul(dd_mul(wld((int64_t)m * NS + i), -fl), adj_inflow(cv, i, c)), D);
                oi[i * ca.ld_oi] = x.hi + x.lo;
            }
    }
}
#endif

}  // namespace pck
