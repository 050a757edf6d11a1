// The multi-objective adjoint of mk_sens_multi.h with one lane per condition,
// for the networks of the one-lane solve path (1 <= NS <= PCK_MAX_DYN_LANE
// dynamic species): the schedule of mk_sens_lane.h applied to the algorithm of
// multi_body.
//
// Formulas, statuses and outputs are multi_body's, all double-double; assembly,
// row replacement and equilibration are sens_lane_body's, statement for
// statement.  Lane l of block b is condition 64 b + l and does everything for
// it serially: no cross-lane operation, no barrier, every exit and every
// `continue` of the objective loop per lane, and the lanes of a wavefront may
// pivot differently.  Sums that the group kernels reduce over lanes run in
// index order here, so the two agree to rounding, not bitwise; a condition's
// result does not depend on its lane, its block or the size of the batch.
//
// The LU keeps no right-hand side: the multiplier of row r at step k stays in
// the entry it annihilates, and every objective replays the forward
// elimination on its own g_m before it back-substitutes.
//
// LDS as mk_sens_lane.h: entry e of lane l at double-double index e * 64 + l,
// every wavefront access 64 contiguous 16-byte slots.  Entries of one lane:
//   [0, NS^2)             M = A^T, then its L and U; M[r][q] at r NS + q
//   [NS^2, NS^2 + NS)     g_m; then lambda_m (row p holds the unknown it was
//                         the pivot of); then lambda_mi w_i, parked in place
//   [NS^2 + NS, + 2 NS)   {column scale of column i, row scale of row i}
// The matrix has to survive the K solves, and still this is the budget of the
// single-objective one-lane kernels, 16 (NS^2 + 2 NS) 64 bytes per block (24 /
// 48 / 80 KiB at NS 4 / 6 / 8): the row weight w_i is not stored -- it is the
// row scale `rs` of nv.dyn at T, or 0 where the `repl` bit says the row was
// replaced -- so its half-slot beside the column scale holds the row scale of
// M that every g_m needs.  Nothing is sized by K: the objectives are a run-time
// loop.  The pivot bookkeeping is two registers of 4-bit fields (NS <= 8).
#pragma once
#include "mk_sens_multi.h"

namespace pck {

__host__ __device__ constexpr int multi_lane_entries(int NS) { return NS * NS + 2 * NS; }
__host__ __device__ constexpr size_t multi_lane_lds_bytes(int NS) {
    return (size_t)multi_lane_entries(NS) * 64 * sizeof(dd);
}

typedef double multi_v2d __attribute__((ext_vector_type(2)));   // one 16-byte LDS access per double-double

#define PCK_SIG_MULTI_LANE                                                                                    \
    NetView nv, GrpView gv, CondView cv, const double *kf, const double *kr, int64_t ld_k, const double *yin, \
        int64_t ld_y, const int32_t *status_in, MultiObj ob, MultiOut out

// (the split build, csrc/mk_inst.h: defined in tu_sens_multi_lane.hip, declared where it is launched)
#if defined(PCK_SPLIT_TU) && PCK_SPLIT_TU && !defined(PCK_KERNEL_TU)
__global__ void k_lane_multi_adjoint(PCK_SIG_MULTI_LANE);
#else

// val[m], xi[m][j] and the statuses of K objectives per condition: arguments
// and outputs as k_multi_adjoint.
__global__ void __launch_bounds__(64) k_lane_multi_adjoint(PCK_SIG_MULTI_LANE) {
    extern __shared__ __attribute__((aligned(16))) multi_v2d lds_mlane[];
    const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (c >= cv.n) return;                         // per lane, as every exit below: no barrier anywhere
    const int NS = nv.NDYN, R = nv.NRXN;
    multi_v2d* const L = lds_mlane + threadIdx.x;
    auto ld = [&](int e) -> dd { const multi_v2d v = L[e * 64]; return dd{v.x, v.y}; };
    auto put = [&](int e, dd v) { L[e * 64] = multi_v2d{v.hi, v.lo}; };
    const int eG = NS * NS, eW = NS * NS + NS;
    const SensIn in{kf, kr, ld_k, yin, ld_y, cv.fixc, cv.ld_fix, cv.s_fix, c};
    const double NaN = __builtin_nan("");

    int st = status_in ? status_in[c] : PCK_ST_OK;
    const double T = cv.T[c * cv.sT];
    unsigned repl = 0;                             // bit i: row i is replaced
    unsigned stp = 0xffffffffu, rof = 0u;          // the pivot bookkeeping (below)
    if (st == PCK_ST_OK) {
        for (int e = 0; e < eG; ++e) put(e, dd_of(0.0));
        // row i of A into column i of M; rows replaced as in mk_solver.h: newton --
        // the conservation laws in their pivot rows, a unit row for a pinned species
        for (int i = 0; i < NS; ++i) {
            const double* d = nv.dyn + 4 * i;
            const double rs = (d[2] != 0.0) ? d[1] + d[2] * T : d[1];   // reactor.py:34-41, as mk_group.h: grp_setup
            const double fl = d[3];
            const double yi = yin[i * ld_y + c];
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
            if (fl != 0.0) {                        // the CSTR flow term fl (in - y)
                const double yin_i = cv.inflow ? cv.inflow[i * cv.ld_in + c * cv.s_in] : 0.0;
                f = dd_add(f, dd_mul(two_sum(yin_i, -yi), fl));
                put(i * NS + i, dd_add(ld(i * NS + i), dd_of(-fl)));
            }
            int law = -1;
            for (int l = 0; l < nv.NCONS; ++l)
                if (nv.cpiv[l] == i) law = l;
            const bool pv = law >= 0;
            const bool pin = !pv && yi == 0.0 && f.hi == 0.0 && f.lo == 0.0;
            if (pv)
                for (int q = 0; q < NS; ++q) put(q * NS + i, dd_of(nv.C[law * NS + q]));
            if (pin)
                for (int q = 0; q < NS; ++q) put(q * NS + i, dd_of(q == i ? 1.0 : 0.0));
            if (pv || pin) repl |= 1u << i;        // b_j's weight on this row: 0 if replaced, else rs
        }

        // equilibration by powers of two (exact): the columns of M (the rows of
        // A: rate rows up to 1e9, conservation rows O(1)), then its rows; both
        // scales are kept for the objectives
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

        // LU with partial pivoting.  Rows are not moved: field r of `stp` is the
        // column row r was the pivot of (15: none yet), field k of `rof` the
        // pivot row of column k.  The multiplier of a row stays in the entry it
        // annihilates.
        bool ok = true;
        for (int k = 0; k < NS; ++k) {
            double m = -1.0;
            int p = 0;
            for (int r = 0; r < NS; ++r) {
                if (((stp >> (4 * r)) & 15u) != 15u) continue;
                double a = fabs(ld(r * NS + k).hi);
                if (a != a) a = INFINITY;              // a NaN must not hide behind the maximum
                if (a > m) { m = a; p = r; }           // the lowest such row
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
        // a non-finite factor anywhere in L or U
        if (ok)
            for (int e = 0; e < eG; ++e) {
                const dd v = ld(e);
                ok = ok && isfinite(v.hi + v.lo);
            }
        if (!ok) st = PCK_ST_SENS_SINGULAR;
    }
    if (out.status) out.status[c] = st;

    // forward / reverse side of reaction j
    auto sides = [&](int j, dd& rf, dd& rr) {
        sens_keff(nv, in, j, rf, rr);
        sens_sides(nv, in, gv.rx[j], rf, rr, -1);
    };
    for (int m = 0; m < ob.K; ++m) {
        const double* wr = ob.wr ? ob.wr + (int64_t)m * R : nullptr;
        const double* wy = ob.wy ? ob.wy + (int64_t)m * NS : nullptr;
        double* xi = out.xi + (int64_t)m * R * out.ld_xi + c;
        // J_m in double-double, summed in index order
        dd J = dd_of(0.0);
        if (wr)
            for (int j = 0; j < R; ++j) {
                const double w = wr[j];
                if (w == 0.0) continue;
                dd rf, rr;
                sides(j, rf, rr);
                J = dd_add(J, dd_mul(dd_sub(rf, rr), w));
            }
        if (wy)
            for (int i = 0; i < NS; ++i) J = dd_add(J, two_prod(wy[i], yin[i * ld_y + c]));
        const double Jd = J.hi + J.lo;
        out.val[m * out.ld_val + c] = Jd;
        int so = st;
        if (so == PCK_ST_OK && !(isfinite(Jd) && Jd != 0.0)) so = PCK_ST_NONFINITE;
        if (so != PCK_ST_OK) {
            for (int j = 0; j < R; ++j) xi[j * out.ld_xi] = NaN;
            if (out.ostatus) out.ostatus[m * out.ld_os + c] = so;
            continue;
        }

        // g_m = dJ_m / dy in the row scale of M
        for (int q = 0; q < NS; ++q) put(eG + q, dd_of(wy ? wy[q] : 0.0));
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
        for (int q = 0; q < NS; ++q) put(eG + q, dd_scale(ld(eG + q), ld(eW + q).lo));
        // the forward elimination replayed from the stored multipliers: at step
        // k every row whose pivot step is later than k subtracts l g_pivot
        for (int k = 0; k < NS; ++k) {
            const dd gp = ld(eG + (int)((rof >> (4 * k)) & 15u));
            for (int r = 0; r < NS; ++r)
                if ((int)((stp >> (4 * r)) & 15u) > k) put(eG + r, dd_sub(ld(eG + r), dd_mul(ld(r * NS + k), gp)));
        }
        // back substitution: lambda_k into the g slot of its pivot row
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
        if (!fin) {                                // an overflow of this objective alone
            for (int j = 0; j < R; ++j) xi[j * out.ld_xi] = NaN;
            if (out.ostatus) out.ostatus[m * out.ld_os + c] = PCK_ST_NONFINITE;
            continue;
        }
        // lambda_mi scaled back, times b_j's row weight, parked over lambda_mi
        for (int i = 0; i < NS; ++i) {
            const int p = (int)((rof >> (4 * i)) & 15u);
            const double* d = nv.dyn + 4 * i;
            const double rs = (d[2] != 0.0) ? d[1] + d[2] * T : d[1];
            const double wi = ((repl >> i) & 1u) ? 0.0 : rs;
            put(eG + p, dd_mul(dd_scale(ld(eG + p), ld(eW + i).hi), wi));
        }
        // xi[m][j] = net_j s_mj / J_m
        for (int j = 0; j < R; ++j) {
            dd rf, rr;
            sides(j, rf, rr);
            dd s = dd_of(wr ? wr[j] : 0.0);
            for (int i = 0; i < NS; ++i) {
                const double sv = nv.S[i * R + j];
                if (sv != 0.0) s = dd_sub(s, dd_mul(ld(eG + (int)((rof >> (4 * i)) & 15u)), sv));
            }
            const dd x = dd_div(dd_mul(dd_sub(rf, rr), s), J);
            xi[j * out.ld_xi] = x.hi + x.lo;
        }
        if (out.ostatus) out.ostatus[m * out.ld_os + c] = PCK_ST_OK;
    }
}
#endif

}  // namespace pck
