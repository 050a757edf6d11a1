// The adjoint solve of mk_sens.h with one lane per condition, for the networks
// of the one-lane solve path (1 <= NS <= PCK_MAX_DYN_LANE dynamic species: the
// volcano, NS 4; the Pd111 CSTR, NS 6).  On those the group kernels leave most
// of their 16 lanes idle through the factorisation (12 of 16 on the volcano).
//
// Formulas, row replacement, statuses and outputs are those of sens_body
// (mk_sens.h), all double-double; what differs is the schedule.  Lane l of
// block b is condition 64 b + l and does everything for it serially: no
// cross-lane operation, no barrier, every early exit (status_in, zero TOF,
// singular matrix, the guard) per lane, and the lanes of a wavefront may pivot
// differently.  Sums that the group kernels reduce over lanes run in index
// order here, so the two agree to rounding, not bitwise.
//
// The per-condition arrays are indexed at run time (pivoting), so they live in
// LDS, not in registers: entry e of lane l at double-double index e * 64 + l,
// which makes every wavefront access 64 contiguous 16-byte slots (one
// ds_read_b128 / ds_write_b128 per entry, conflict-free in each of its lane
// groups).  Entries of one lane:
//   [0, NS^2)             M = A^T, M[r][q] at r NS + q
//   [NS^2, NS^2 + NS)     g, eliminated along; then lambda (row p holds the
//                         unknown it was the pivot of), scaled back at the end
//   [NS^2 + NS, + 2 NS)   {column scale, row weight w_i}; then lambda_i w_i
// 16 (NS^2 + 2 NS) 64 bytes per block: 24 KiB at NS 4, 48 KiB at 6, 80 KiB at 8
// (above the 64 KiB default: the launch raises the kernel's dynamic-LDS limit).
// The pivot bookkeeping is two registers of 4-bit fields (NS <= 8).
#pragma once
#include "mk_sens.h"

namespace pck {

__host__ __device__ constexpr int sens_lane_entries(int NS) { return NS * NS + 2 * NS; }
__host__ __device__ constexpr size_t sens_lane_lds_bytes(int NS) {
    return (size_t)sens_lane_entries(NS) * 64 * sizeof(dd);
}

typedef double sens_v2d __attribute__((ext_vector_type(2)));   // one 16-byte LDS access per double-double

#define PCK_SIG_SENS_LANE                                                                                     \
    NetView nv, GrpView gv, CondView cv, const double *kf, const double *kr, int64_t ld_k, const double *yin, \
        int64_t ld_y, const int32_t *status_in, double *xi, int64_t ld_xi, double *tof0, int32_t *status

// (the split build, csrc/mk_inst.h: defined in tu_sens_lane.hip, declared where they are launched)
#if defined(PCK_SPLIT_TU) && PCK_SPLIT_TU && !defined(PCK_KERNEL_TU)
__global__ void k_lane_drc_adjoint(PCK_SIG_SENS_LANE);
__global__ void k_lane_sens_adjoint(PCK_SIG_SENS_LANE, SensExt ex);
#else

// NaN into every output of SensExt of condition c (sens_ext_nan, one lane)
__device__ __forceinline__ void sens_lane_nan(const NetView& nv, const SensExt& ex, int64_t c, bool with_err) {
    const double NaN = __builtin_nan("");
    for (int j = 0; j < nv.NRXN; ++j) {
        if (ex.sf) ex.sf[j * ex.ld_s + c] = NaN;
        if (ex.sr) ex.sr[j * ex.ld_s + c] = NaN;
    }
    if (ex.order)
        for (int q = 0; q < nv.NFIX; ++q) ex.order[q * ex.ld_o + c] = NaN;
    if (ex.order_in)
        for (int i = 0; i < nv.NDYN; ++i) ex.order_in[i * ex.ld_oi + c] = NaN;
    if (ex.dir)
        for (int m = 0; m < ex.nd; ++m) ex.dir[m * ex.ld_dir + c] = NaN;
    if (with_err && ex.err) ex.err[c] = NaN;
}

// The body of k_lane_drc_adjoint (EXT = false) and k_lane_sens_adjoint (EXT =
// true): arguments and outputs as sens_body.
template <bool EXT>
__device__ __forceinline__ void sens_lane_body(const NetView& nv, const GrpView& gv, const CondView& cv,
                                               const double* kf, const double* kr, int64_t ld_k, const double* yin,
                                               int64_t ld_y, const int32_t* status_in, double* xi, int64_t ld_xi,
                                               double* tof0, int32_t* status, const SensExt& ex) {
    extern __shared__ __attribute__((aligned(16))) sens_v2d lds_lane[];
    const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (c >= cv.n) return;                         // per lane, as every exit below: no barrier anywhere
    const int NS = nv.NDYN, R = nv.NRXN;
    sens_v2d* const L = lds_lane + threadIdx.x;
    auto ld = [&](int e) -> dd { const sens_v2d v = L[e * 64]; return dd{v.x, v.y}; };
    auto put = [&](int e, dd v) { L[e * 64] = sens_v2d{v.hi, v.lo}; };
    const int eG = NS * NS, eW = NS * NS + NS;
    const SensIn in{kf, kr, ld_k, yin, ld_y, cv.fixc, cv.ld_fix, cv.s_fix, c};
    const double NaN = __builtin_nan("");

    // TOF in double-double (old_system.py:482-488)
    dd tof = dd_of(0.0);
    for (int t = 0; t < nv.NTOF; ++t) {
        const int r = nv.tof[t];
        dd a, b;
        sens_keff(nv, in, r, a, b);
        tof = dd_add(tof, sens_rate(nv, in, gv.rx[r], a, b, -1));
    }
    const double tofd = tof.hi + tof.lo;
    if (tof0) tof0[c] = tofd;
    int st = status_in ? status_in[c] : PCK_ST_OK;
    if (st == PCK_ST_OK && !(isfinite(tofd) && tofd != 0.0)) st = PCK_ST_NONFINITE;
    if (st != PCK_ST_OK) {
        if (!EXT || xi)
            for (int j = 0; j < R; ++j) xi[j * ld_xi + c] = NaN;
        if constexpr (EXT) sens_lane_nan(nv, ex, c, true);
        if (status) status[c] = st;
        return;
    }

    for (int e = 0; e < eW; ++e) put(e, dd_of(0.0));
    // row i of A into column i of M; rows replaced as in mk_solver.h: newton --
    // the conservation laws in their pivot rows, a unit row for a pinned species
    const double T = cv.T[c * cv.sT];
    unsigned repl = 0;                             // bit i: row i is replaced
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
        if (fl != 0.0) {                            // the CSTR flow term fl (in - y)
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
        if (pv || pin) repl |= 1u << i;
        put(eW + i, dd{1.0, (pv || pin) ? 0.0 : rs});   // {column scale (below), b_j's weight on this row}
    }

    // g = d TOF / dy
    for (int t = 0; t < nv.NTOF; ++t) {
        const int r = nv.tof[t];
        const uint4 rec = gv.rx[r];
        const int np = rx_np(rec);
        dd a, b;
        sens_keff(nv, in, r, a, b);
        for (int k = 0; k < np; ++k) {
            const int q = rx_field(rec, k) & 63;
            put(eG + q, dd_add(ld(eG + q), sens_rate(nv, in, rec, a, b, k)));
        }
    }

    // equilibration by powers of two (exact): the columns of M (the rows of
    // A: rate rows up to 1e9, conservation rows O(1)), then its rows
    for (int q = 0; q < NS; ++q) {
        double m = 0.0;
        for (int r = 0; r < NS; ++r) m = fmax(m, fabs(ld(r * NS + q).hi));
        const double s = inv_pow2(m);
        for (int r = 0; r < NS; ++r) put(r * NS + q, dd_scale(ld(r * NS + q), s));
        put(eW + q, dd{s, ld(eW + q).lo});
    }
    for (int r = 0; r < NS; ++r) {
        double m = 0.0;
        for (int q = 0; q < NS; ++q) m = fmax(m, fabs(ld(r * NS + q).hi));
        const double s = inv_pow2(m);
        for (int q = 0; q < NS; ++q) put(r * NS + q, dd_scale(ld(r * NS + q), s));
        put(eG + r, dd_scale(ld(eG + r), s));
    }

    // LU with partial pivoting, the right-hand side eliminated along.  Rows are
    // not moved: field r of `stp` is the column row r was the pivot of (15:
    // none yet), field k of `rof` the pivot row of column k.
    unsigned stp = 0xffffffffu, rof = 0u;
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
        const dd piv = ld(p * NS + k), gp = ld(eG + p);
        for (int r = 0; r < NS; ++r) {
            if (((stp >> (4 * r)) & 15u) != 15u) continue;
            const dd l = dd_div(ld(r * NS + k), piv);
            for (int q = k + 1; q < NS; ++q) put(r * NS + q, dd_sub(ld(r * NS + q), dd_mul(l, ld(p * NS + q))));
            put(eG + r, dd_sub(ld(eG + r), dd_mul(l, gp)));
        }
    }
    // back substitution: lambda_k into the g slot of its pivot row
    if (ok) {
        for (int k = NS - 1; k >= 0; --k) {
            const int p = (int)((rof >> (4 * k)) & 15u);
            const dd x = dd_div(ld(eG + p), ld(p * NS + k));
            for (int r = 0; r < NS; ++r)
                if ((int)((stp >> (4 * r)) & 15u) < k) put(eG + r, dd_sub(ld(eG + r), dd_mul(ld(r * NS + k), x)));
            put(eG + p, x);
            const double lsum = x.hi + x.lo;
            ok = ok && isfinite(lsum);
        }
    }
    if (!ok) {
        if (!EXT || xi)
            for (int j = 0; j < R; ++j) xi[j * ld_xi + c] = NaN;
        if constexpr (EXT) sens_lane_nan(nv, ex, c, true);
        if (status) status[c] = PCK_ST_SENS_SINGULAR;
        return;
    }
    // lambda_i scaled back (kept for the inflow orders), and lambda_i x (b_j's row weight)
    for (int i = 0; i < NS; ++i) {
        const int p = (int)((rof >> (4 * i)) & 15u);
        const dd sw = ld(eW + i);
        const dd lam = dd_scale(ld(eG + p), sw.hi);
        put(eG + p, lam);
        put(eW + i, dd_mul(lam, sw.lo));
    }
    // the bracket s_j = [j in tof] - sum_i lambda_i w_i S_ij and the two sides of reaction j
    auto terms = [&](int j, dd& rf, dd& rr) -> dd {
        sens_keff(nv, in, j, rf, rr);
        sens_sides(nv, in, gv.rx[j], rf, rr, -1);
        int cnt = 0;
        for (int t = 0; t < nv.NTOF; ++t) cnt += (nv.tof[t] == j);
        dd s = dd_of((double)cnt);
        for (int i = 0; i < NS; ++i) {
            const double sv = nv.S[i * R + j];
            if (sv != 0.0) s = dd_sub(s, dd_mul(ld(eW + i), sv));
        }
        return s;
    };
    // xi_j = net_j s_j / TOF
    double rmax = 0.0;
    for (int j = 0; j < R; ++j) {
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
        // the guard (mk_sens.h; DESIGN.md "Adjoint sensitivities")
        const double err = PCK_SENS_ERR_UNIT * rmax / fabs(tofd);
        if (ex.err) ex.err[c] = err;
        if (ex.err_max > 0.0 && !(err <= ex.err_max)) {
            sens_lane_nan(nv, ex, c, false);
            if (status) status[c] = PCK_ST_SENS_PRECISION;
            return;
        }
        if (ex.sf || ex.sr) {
            for (int j = 0; j < R; ++j) {
                dd rf, rr;
                const dd s = terms(j, rf, rr);
                const dd xf = dd_div(dd_mul(rf, s), tof), xr = dd_div(dd_mul(rr, s), tof);
                if (ex.sf) ex.sf[j * ex.ld_s + c] = xf.hi + xf.lo;
                if (ex.sr) ex.sr[j * ex.ld_s + c] = -(xr.hi + xr.lo);
            }
        }
        // reaction orders in the fixed species
        if (ex.order) {
            for (int q = 0; q < nv.NFIX; ++q) {
                dd acc = dd_of(0.0);
                for (int j = 0; j < R; ++j) {
                    const int ea = nv.foldf[j * nv.NFIX + q], eb = nv.foldr[j * nv.NFIX + q];
                    if (!(ea | eb)) continue;
                    dd rf, rr;
                    const dd s = terms(j, rf, rr);
                    acc = dd_add(acc, dd_mul(s, dd_sub(dd_mul(rf, (double)ea), dd_mul(rr, (double)eb))));
                }
                const dd x = dd_div(acc, tof);
                ex.order[q * ex.ld_o + c] = x.hi + x.lo;
            }
        }
        // ... and in the inflow of a species with a flow term (not scaled by the row scale)
        if (ex.order_in) {
            for (int i = 0; i < NS; ++i) {
                const double fl = nv.dyn[4 * i + 3];
                dd x = dd_of(0.0);
                if (fl != 0.0 && !((repl >> i) & 1u)) {
                    const double flin = cv.inflow ? cv.inflow[i * cv.ld_in + c * cv.s_in] : 0.0;
                    const dd lam = ld(eG + (int)((rof >> (4 * i)) & 15u));
                    x = dd_div(dd_mul(dd_mul(lam, -fl), flin), tof);
                }
                ex.order_in[i * ex.ld_oi + c] = x.hi + x.lo;
            }
        }
        // user directions (d ln kf, d ln kr)
        if (ex.dir) {
            for (int m = 0; m < ex.nd; ++m) {
                const double* am = ex.a + m * ex.s_ac;
                const double* cm = ex.c + m * ex.s_ac;
                dd acc = dd_of(0.0);
                for (int j = 0; j < R; ++j) {
                    dd rf, rr;
                    const dd s = terms(j, rf, rr);
                    acc = dd_add(acc, dd_mul(s, dd_sub(dd_mul(rf, am[j * ex.ld_ac + c]), dd_mul(rr, cm[j * ex.ld_ac + c]))));
                }
                const dd x = dd_div(acc, tof);
                ex.dir[m * ex.ld_dir + c] = x.hi + x.lo;
            }
        }
    }
    if (status) status[c] = PCK_ST_OK;
}

// xi[j][ld_xi] for every active reaction, tof0 and status per condition.
__global__ void __launch_bounds__(64) k_lane_drc_adjoint(PCK_SIG_SENS_LANE) {
    sens_lane_body<false>(nv, gv, cv, kf, kr, ld_k, yin, ld_y, status_in, xi, ld_xi, tof0, status, SensExt{});
}

// ... and the outputs of SensExt.
__global__ void __launch_bounds__(64) k_lane_sens_adjoint(PCK_SIG_SENS_LANE, SensExt ex) {
    sens_lane_body<true>(nv, gv, cv, kf, kr, ld_k, yin, ld_y, status_in, xi, ld_xi, tof0, status, ex);
}
#endif

}  // namespace pck
