// Batched eigenvalues of small real matrices (the steady Jacobians of a batch
// of conditions), fp64: balancing by powers of two (scaling only), Householder
// reduction to upper Hessenberg form, Francis double-shift QR on the active
// window, eigenvalues only (EISPACK balanc / orthes / hqr; the balancing takes
// LAPACK dgebal's norms and guards, so the balanced matrix B is the one
// scipy.linalg.matrix_balance(J, permute=False) returns).
//
// Two schedules over the same formulas:
//   k_eig_lane     one lane per condition (ns <= PCK_MAX_DYN_LANE): the serial
//                  core below over an accessor, element e of lane l at
//                  M[e * 64 + l] in LDS (all dynamic indexing goes through LDS,
//                  no private arrays).  The core is __host__ __device__: a
//                  stand-alone host program runs the same text on the CPU
//                  (tests/eig_host_check.hip).
//   k_eig_grp<G>   G = 16 / 32 / 64 lanes per condition (ns <= G), the matrix
//                  G x G in LDS as the adjoint kernels lay out theirs
//                  (A[i][q] at M[q * G + i]).  Reflectors are applied from the
//                  left with one lane per column and from the right with one
//                  lane per row; the small shared quantities (norms, shifts,
//                  the 3-element bulge reflectors, the deflation scan) are
//                  computed by every lane of the group from broadcast LDS
//                  reads, so every lane of a group holds the same bits and
//                  no value crosses lanes but through LDS.
//
// Every loop has a static bound: the balancing sweeps and their shift loops,
// the reduction, and the QR sweeps (30 * max(10, ns) in all; a matrix that
// exhausts them gets PCK_ST_EIG_NOCONV).  A matrix with a non-finite entry
// never enters them (PCK_ST_NONFINITE).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "pycatkin_amd.h"

namespace pck {

#define PCK_EIG_BAL_SWEEPS 32     /* balancing sweeps over the matrix at most */
#define PCK_EIG_BAL_SHIFTS 1100   /* doublings of one scale factor at most (the exponent range of fp64 is 2098) */
#define PCK_EIG_EPS 2.220446049250313e-16
// dgebal's guards: sfmin1 = dlamch('S') / dlamch('P'), sfmin2 = 2 sfmin1
#define PCK_EIG_SFMIN2 (2.0 * (2.2250738585072014e-308 / 2.220446049250313e-16))
#define PCK_EIG_SFMAX2 (1.0 / PCK_EIG_SFMIN2)

__host__ __device__ inline int eig_budget(int ns) { return 30 * (ns > 10 ? ns : 10); }

// re_max / im_max / re_min / n_pos of the eigenvalues found so far
struct EigStats {
    double re_max, im_max, re_min;
    int n_pos;
    bool bad;                     // a non-finite eigenvalue
};
__host__ __device__ inline void eig_stats_init(EigStats& s) {
    s.re_max = -INFINITY; s.im_max = 0.0; s.re_min = INFINITY; s.n_pos = 0; s.bad = false;
}
__host__ __device__ inline void eig_stats_add(EigStats& s, double re, double im, double re_tol) {
    im = fabs(im);
    if (!isfinite(re) || !isfinite(im)) s.bad = true;
    if (re > s.re_max) { s.re_max = re; s.im_max = im; }
    else if (re == s.re_max && im > s.im_max) s.im_max = im;
    if (re < s.re_min) s.re_min = re;
    if (re > re_tol) ++s.n_pos;
}

// dgebal's scale factor of one index from the 2-norms c (column) and r (row)
// and the largest entries ca / ra: true if row and column are to be scaled
// (row by 1 / f, column by f)
__host__ __device__ inline bool eig_bal_factor(double c, double r, double ca, double ra, double& f) {
    f = 1.0;
    if (c == 0.0 || r == 0.0) return false;
    double g = r / 2.0;
    const double s = c + r;
    for (int it = 0; it < PCK_EIG_BAL_SHIFTS; ++it) {
        if (!(c < g && fmax(f, fmax(c, ca)) < PCK_EIG_SFMAX2 && fmin(r, fmin(g, ra)) > PCK_EIG_SFMIN2)) break;
        f *= 2.0; c *= 2.0; ca *= 2.0; r /= 2.0; g /= 2.0; ra /= 2.0;
    }
    g = c / 2.0;
    for (int it = 0; it < PCK_EIG_BAL_SHIFTS; ++it) {
        if (!(g >= r && fmax(r, ra) < PCK_EIG_SFMAX2 && fmin(fmin(f, c), fmin(g, ca)) > PCK_EIG_SFMIN2)) break;
        f /= 2.0; c /= 2.0; g /= 2.0; ca /= 2.0; r *= 2.0; ra *= 2.0;
    }
    if (!((c + r) < 0.95 * s)) return false;
    return f != 1.0;
}

// the closing 2 x 2 block [[y, .], [., x]] with w the product of its off-diagonal
// entries and t the accumulated shift: a real pair or a conjugate pair
// (re0, im0) the eigenvalue of the upper index, positive imaginary part first
__host__ __device__ inline void eig_close2(double x, double y, double w, double t, double& re0, double& im0,
                                           double& re1, double& im1) {
    const double p = 0.5 * (y - x), q = p * p + w;
    double z = sqrt(fabs(q));
    x += t;
    if (q >= 0.0) {
        z = p + copysign(z, p);
        re0 = re1 = x + z;
        if (z != 0.0) re1 = x - w / z;
        im0 = im1 = 0.0;
    } else {
        re0 = re1 = x + p;
        im0 = z; im1 = -z;
    }
}

// ----------------------------------------------------------------------------
// the serial core: A has get(i, j) / set(i, j, v); E has put(index, re, im)
// ----------------------------------------------------------------------------
template <class A>
__host__ __device__ inline bool eig_all_finite(A& a, int n) {
    bool ok = true;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) ok = ok && isfinite(a.get(i, j));
    return ok;
}

// balancing; returns the Frobenius norm of the balanced matrix
template <class A>
__host__ __device__ inline double eig_balance(A& a, int n) {
    for (int sw = 0; sw < PCK_EIG_BAL_SWEEPS; ++sw) {
        bool noconv = false;
        for (int i = 0; i < n; ++i) {
            double c = 0.0, r = 0.0, ca = 0.0, ra = 0.0;
            for (int j = 0; j < n; ++j) {
                const double v = a.get(j, i), u = a.get(i, j);
                c += v * v; ca = fmax(ca, fabs(v));
                r += u * u; ra = fmax(ra, fabs(u));
            }
            double f;
            if (!eig_bal_factor(sqrt(c), sqrt(r), ca, ra, f)) continue;
            noconv = true;
            const double g = 1.0 / f;
            for (int j = 0; j < n; ++j) a.set(i, j, a.get(i, j) * g);
            for (int j = 0; j < n; ++j) a.set(j, i, a.get(j, i) * f);
        }
        if (!noconv) break;
    }
    double fro = 0.0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) { const double v = a.get(i, j); fro += v * v; }
    return sqrt(fro);
}

// Householder reduction to upper Hessenberg form; the vector of step m is
// parked in column m - 1 below the subdiagonal, which the step annihilates
template <class A>
__host__ __device__ inline void eig_hessenberg(A& a, int n) {
    for (int m = 1; m < n - 1; ++m) {
        double scale = 0.0;
        for (int i = m; i < n; ++i) scale += fabs(a.get(i, m - 1));
        if (scale == 0.0) continue;
        double h = 0.0;
        for (int i = n - 1; i >= m; --i) {
            const double v = a.get(i, m - 1) / scale;
            a.set(i, m - 1, v);
            h += v * v;
        }
        const double vm = a.get(m, m - 1);
        const double g = -copysign(sqrt(h), vm);
        h -= vm * g;
        a.set(m, m - 1, vm - g);
        for (int j = m; j < n; ++j) {
            double f = 0.0;
            for (int i = n - 1; i >= m; --i) f += a.get(i, m - 1) * a.get(i, j);
            f /= h;
            for (int i = m; i < n; ++i) a.set(i, j, a.get(i, j) - f * a.get(i, m - 1));
        }
        for (int i = 0; i < n; ++i) {
            double f = 0.0;
            for (int j = n - 1; j >= m; --j) f += a.get(j, m - 1) * a.get(i, j);
            f /= h;
            for (int j = m; j < n; ++j) a.set(i, j, a.get(i, j) - f * a.get(j, m - 1));
        }
        a.set(m, m - 1, scale * g);
        for (int i = m + 1; i < n; ++i) a.set(i, m - 1, 0.0);
    }
}

// Francis double-shift QR on the Hessenberg matrix; PCK_ST_OK or PCK_ST_EIG_NOCONV
template <class A, class E>
__host__ __device__ inline int eig_hqr(A& a, int n, E& out, int budget) {
    double anorm = 0.0;
    for (int i = 0; i < n; ++i)
        for (int j = (i > 0 ? i - 1 : 0); j < n; ++j) anorm += fabs(a.get(i, j));
    int nn = n - 1, its = 0, tot = 0;
    double t = 0.0;
    // every trip either deflates (at most n of them) or spends one sweep of the budget
    for (int trip = 0; trip < budget + n + 1 && nn >= 0; ++trip) {
        int l = nn;
        for (; l >= 1; --l) {
            double s = fabs(a.get(l - 1, l - 1)) + fabs(a.get(l, l));
            if (s == 0.0) s = anorm;
            if (fabs(a.get(l, l - 1)) + s == s) {
                a.set(l, l - 1, 0.0);
                break;
            }
        }
        double x = a.get(nn, nn);
        if (l == nn) {
            out.put(nn, x + t, 0.0);
            nn -= 1; its = 0;
            continue;
        }
        double y = a.get(nn - 1, nn - 1), w = a.get(nn, nn - 1) * a.get(nn - 1, nn);
        if (l == nn - 1) {
            double r0, i0, r1, i1;
            eig_close2(x, y, w, t, r0, i0, r1, i1);
            out.put(nn - 1, r0, i0);
            out.put(nn, r1, i1);
            nn -= 2; its = 0;
            continue;
        }
        if (tot >= budget) return PCK_ST_EIG_NOCONV;
        if (its == 10 || its == 20) {             // exceptional shift
            t += x;
            for (int i = 0; i <= nn; ++i) a.set(i, i, a.get(i, i) - x);
            const double s = fabs(a.get(nn, nn - 1)) + fabs(a.get(nn - 1, nn - 2));
            y = x = 0.75 * s;
            w = -0.4375 * s * s;
        }
        ++its; ++tot;
        double p = 0.0, q = 0.0, r = 0.0, z;
        int m = nn - 2;
        for (; m >= l; --m) {
            z = a.get(m, m);
            r = x - z;
            double s = y - z;
            p = (r * s - w) / a.get(m + 1, m) + a.get(m, m + 1);
            q = a.get(m + 1, m + 1) - z - r - s;
            r = a.get(m + 2, m + 1);
            s = fabs(p) + fabs(q) + fabs(r);
            p /= s; q /= s; r /= s;
            if (m == l) break;
            const double u = fabs(a.get(m, m - 1)) * (fabs(q) + fabs(r));
            const double v = fabs(p) * (fabs(a.get(m - 1, m - 1)) + fabs(z) + fabs(a.get(m + 1, m + 1)));
            if (u + v == v) break;
        }
        for (int i = m + 2; i <= nn; ++i) {
            a.set(i, i - 2, 0.0);
            if (i != m + 2) a.set(i, i - 3, 0.0);
        }
        for (int k = m; k <= nn - 1; ++k) {
            if (k != m) {
                p = a.get(k, k - 1);
                q = a.get(k + 1, k - 1);
                r = (k != nn - 1) ? a.get(k + 2, k - 1) : 0.0;
                x = fabs(p) + fabs(q) + fabs(r);
                if (x != 0.0) { p /= x; q /= x; r /= x; }
            }
            const double s = copysign(sqrt(p * p + q * q + r * r), p);
            if (s == 0.0 || s != s) continue;
            if (k == m) {
                if (l != m) a.set(k, k - 1, -a.get(k, k - 1));
            } else {
                a.set(k, k - 1, -s * x);
            }
            p += s;
            const double hx = p / s, hy = q / s, hz = r / s;
            q /= p; r /= p;
            const bool three = k != nn - 1;
            for (int j = k; j <= nn; ++j) {
                double pp = a.get(k, j) + q * a.get(k + 1, j);
                if (three) {
                    pp += r * a.get(k + 2, j);
                    a.set(k + 2, j, a.get(k + 2, j) - pp * hz);
                }
                a.set(k + 1, j, a.get(k + 1, j) - pp * hy);
                a.set(k, j, a.get(k, j) - pp * hx);
            }
            const int mmin = nn < k + 3 ? nn : k + 3;
            for (int i = l; i <= mmin; ++i) {
                double pp = hx * a.get(i, k) + hy * a.get(i, k + 1);
                if (three) {
                    pp += hz * a.get(i, k + 2);
                    a.set(i, k + 2, a.get(i, k + 2) - pp * r);
                }
                a.set(i, k + 1, a.get(i, k + 1) - pp * q);
                a.set(i, k, a.get(i, k) - pp);
            }
        }
    }
    return nn < 0 ? PCK_ST_OK : PCK_ST_EIG_NOCONV;
}

// the eigenvalues of the n x n matrix behind `a` (overwritten): PCK_ST_OK,
// PCK_ST_NONFINITE or PCK_ST_EIG_NOCONV; scale = n eps ||B||_F; budget: QR sweeps
// in all (eig_budget(n); the host check also runs a budget of 1)
template <class A, class E>
__host__ __device__ inline int eig_serial(A& a, int n, E& out, double& scale, int budget) {
    scale = NAN;
    if (!eig_all_finite(a, n)) return PCK_ST_NONFINITE;
    scale = (double)n * PCK_EIG_EPS * eig_balance(a, n);
    eig_hessenberg(a, n);
    return eig_hqr(a, n, out, budget);
}

#if defined(__HIPCC__)
// ----------------------------------------------------------------------------
// outputs (pck_eig_out by value) of one condition, written by one lane
// ----------------------------------------------------------------------------
struct EigEmit {
    pck_eig_out o;
    int64_t c;
    double re_tol;
    EigStats st;
    __device__ __forceinline__ void put(int k, double re, double im) {
        eig_stats_add(st, re, im, re_tol);
        if (o.wr) o.wr[(int64_t)k * o.ld_w + c] = re;
        if (o.wi) o.wi[(int64_t)k * o.ld_w + c] = im;
    }
};

__device__ __forceinline__ void eig_write_summary(const pck_eig_out& o, int64_t c, int ns, int status, const EigStats& st,
                                                   double scale) {
    const bool ok = status == PCK_ST_OK;
    if (!ok) {
        for (int k = 0; k < ns; ++k) {
            if (o.wr) o.wr[(int64_t)k * o.ld_w + c] = NAN;
            if (o.wi) o.wi[(int64_t)k * o.ld_w + c] = NAN;
        }
    }
    if (o.re_max) o.re_max[c] = ok ? st.re_max : NAN;
    if (o.im_max) o.im_max[c] = ok ? st.im_max : NAN;
    if (o.re_min) o.re_min[c] = ok ? st.re_min : NAN;
    if (o.scale) o.scale[c] = ok ? scale : NAN;
    if (o.n_pos) o.n_pos[c] = ok ? st.n_pos : -1;
    if (o.status) o.status[c] = status;
}

// ----------------------------------------------------------------------------
// one lane per condition
// ----------------------------------------------------------------------------
struct EigLaneMat {
    double* m;                    // this lane's element 0
    int n;
    __device__ __forceinline__ double get(int i, int j) const { return m[(i * n + j) * 64]; }
    __device__ __forceinline__ void set(int i, int j, double v) { m[(i * n + j) * 64] = v; }
};

inline size_t eig_lane_lds_bytes(int ns) { return (size_t)ns * ns * 64 * sizeof(double); }

__global__ void __launch_bounds__(64) k_eig_lane(const double* __restrict__ a, int ns, int64_t n, int64_t ld,
                                                 const int32_t* __restrict__ status_in, double re_tol, pck_eig_out o) {
    extern __shared__ double eig_lds[];
    const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (c >= n) return;
    EigEmit em;
    em.o = o; em.c = c; em.re_tol = re_tol;
    eig_stats_init(em.st);
    int status = status_in ? status_in[c] : PCK_ST_OK;
    double scale = NAN;
    if (status == PCK_ST_OK) {
        EigLaneMat A{eig_lds + threadIdx.x, ns};
        for (int e = 0; e < ns * ns; ++e) A.m[e * 64] = a[(int64_t)e * ld + c];
        status = eig_serial(A, ns, em, scale, eig_budget(ns));
        if (status == PCK_ST_OK && em.st.bad) status = PCK_ST_NONFINITE;
    }
    eig_write_summary(o, c, ns, status, em.st, scale);
}

// ----------------------------------------------------------------------------
// G lanes per condition
// ----------------------------------------------------------------------------
// LDS traffic of one step is complete before the next step reads it (the order
// the adjoint kernels keep between their steps, mk_group.h: wsync)
__device__ __forceinline__ void eig_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

template <int G>
inline size_t eig_grp_lds_bytes() { return (size_t)64 * G * sizeof(double); }

#define EA(i, q) M[(q) * G + (i)]

// Balancing, index after index as the serial core (a scaled row changes the
// norms of the columns after it): every lane forms the two norms of index i,
// lane j scales entries (i, j) and (j, i).  Returns ||B||_F.
template <int G>
__device__ __forceinline__ double eig_grp_balance(double* M, int n, int gl, bool on) {
    bool bal = on;
    for (int sw = 0; sw < PCK_EIG_BAL_SWEEPS; ++sw) {
        if (!__any(bal)) break;                    // wave-uniform
        bool noconv = false;
        for (int i = 0; i < n; ++i) {
            double f = 1.0;
            bool doit = false;
            if (bal) {
                double c = 0.0, r = 0.0, ca = 0.0, ra = 0.0;
                for (int j = 0; j < n; ++j) {
                    const double v = EA(j, i), u = EA(i, j);
                    c += v * v; ca = fmax(ca, fabs(v));
                    r += u * u; ra = fmax(ra, fabs(u));
                }
                doit = eig_bal_factor(sqrt(c), sqrt(r), ca, ra, f);
            }
            eig_sync();
            if (doit) {
                noconv = true;
                const double g = 1.0 / f;
                if (gl < n) {
                    if (gl == i) {
                        EA(i, i) = (EA(i, i) * g) * f;
                    } else {
                        EA(i, gl) = EA(i, gl) * g;
                        EA(gl, i) = EA(gl, i) * f;
                    }
                }
            }
            eig_sync();
        }
        bal = bal && noconv;
    }
    double fro = 0.0;
    if (on)
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) { const double v = EA(i, j); fro += v * v; }
    return sqrt(fro);
}

template <int G>
__device__ __forceinline__ void eig_grp_hessenberg(double* M, int n, int gl, bool on) {
    for (int m = 1; m < n - 1; ++m) {
        double scale = 0.0, h = 0.0, g = 0.0, vown = 0.0;
        if (on) {
            for (int i = m; i < n; ++i) scale += fabs(EA(i, m - 1));
            if (scale != 0.0) {
                double vm = 0.0;
                for (int i = n - 1; i >= m; --i) {
                    const double v = EA(i, m - 1) / scale;
                    h += v * v;
                    if (i == gl) vown = v;
                    if (i == m) vm = v;
                }
                g = -copysign(sqrt(h), vm);
                h -= vm * g;
                if (gl == m) vown = vm - g;
            }
        }
        const bool doit = on && scale != 0.0;
        eig_sync();
        if (doit && gl >= m && gl < n) EA(gl, m - 1) = vown;           // the vector, parked
        eig_sync();
        if (doit && gl >= m && gl < n) {                               // from the left: lane gl owns column gl
            double f = 0.0;
            for (int i = n - 1; i >= m; --i) f += EA(i, m - 1) * EA(i, gl);
            f /= h;
            for (int i = m; i < n; ++i) EA(i, gl) = EA(i, gl) - f * EA(i, m - 1);
        }
        eig_sync();
        if (doit && gl < n) {                                          // from the right: lane gl owns row gl
            double f = 0.0;
            for (int j = n - 1; j >= m; --j) f += EA(j, m - 1) * EA(gl, j);
            f /= h;
            for (int j = m; j < n; ++j) EA(gl, j) = EA(gl, j) - f * EA(j, m - 1);
        }
        eig_sync();
        if (doit && gl >= m && gl < n) EA(gl, m - 1) = (gl == m) ? scale * g : 0.0;
        eig_sync();
    }
}

// The QR sweeps.  The trip loop runs in wave-uniform control flow until every
// group of the wavefront is done; a finished group is predicated off.  Lane 0
// of a group writes its eigenvalues.
template <int G>
__device__ __forceinline__ int eig_grp_hqr(double* M, int n, int gl, bool on, EigEmit& em) {
    double anorm = 0.0;
    if (on)
        for (int i = 0; i < n; ++i)
            for (int j = (i > 0 ? i - 1 : 0); j < n; ++j) anorm += fabs(EA(i, j));
    const int budget = eig_budget(n);
    int nn = n - 1, its = 0, tot = 0, status = PCK_ST_OK;
    double t = 0.0;
    bool act = on;
    for (int trip = 0; trip < budget + n + 1; ++trip) {
        if (!__any(act)) break;                    // wave-uniform
        // ---- the deflation scan and the closing blocks (reads only)
        int l = 0, m = 0;
        bool sweep = false, exc = false, zero_sub = false;
        double x = 0.0, y = 0.0, w = 0.0, p = 0.0, q = 0.0, r = 0.0;
        if (act) {
            for (l = nn; l >= 1; --l) {
                double s = fabs(EA(l - 1, l - 1)) + fabs(EA(l, l));
                if (s == 0.0) s = anorm;
                if (fabs(EA(l, l - 1)) + s == s) { zero_sub = true; break; }
            }
            x = EA(nn, nn);
            if (l == nn) {
                if (gl == 0) em.put(nn, x + t, 0.0);
                else eig_stats_add(em.st, x + t, 0.0, em.re_tol);
                nn -= 1; its = 0;
            } else {
                y = EA(nn - 1, nn - 1);
                w = EA(nn, nn - 1) * EA(nn - 1, nn);
                if (l == nn - 1) {
                    double r0, i0, r1, i1;
                    eig_close2(x, y, w, t, r0, i0, r1, i1);
                    if (gl == 0) {
                        em.put(nn - 1, r0, i0);
                        em.put(nn, r1, i1);
                    } else {
                        eig_stats_add(em.st, r0, i0, em.re_tol);
                        eig_stats_add(em.st, r1, i1, em.re_tol);
                    }
                    nn -= 2; its = 0;
                } else if (tot >= budget) {
                    status = PCK_ST_EIG_NOCONV;
                    act = false;
                } else {
                    sweep = true;
                    exc = its == 10 || its == 20;
                    ++its; ++tot;
                }
            }
            if (nn < 0) act = false;
        }
        eig_sync();
        if (zero_sub && gl == 0) EA(l, l - 1) = 0.0;
        if (exc) {                                 // exceptional shift: lane i its diagonal entry
            t += x;
            if (gl <= nn) EA(gl, gl) = EA(gl, gl) - x;
            const double s = fabs(EA(nn, nn - 1)) + fabs(EA(nn - 1, nn - 2));
            y = x = 0.75 * s;
            w = -0.4375 * s * s;
        }
        eig_sync();
        // ---- the start of the bulge: two consecutive small subdiagonal entries
        if (sweep) {
            for (m = nn - 2; m >= l; --m) {
                const double z = EA(m, m);
                r = x - z;
                double s = y - z;
                p = (r * s - w) / EA(m + 1, m) + EA(m, m + 1);
                q = EA(m + 1, m + 1) - z - r - s;
                r = EA(m + 2, m + 1);
                s = fabs(p) + fabs(q) + fabs(r);
                p /= s; q /= s; r /= s;
                if (m == l) break;
                const double u = fabs(EA(m, m - 1)) * (fabs(q) + fabs(r));
                const double v = fabs(p) * (fabs(EA(m - 1, m - 1)) + fabs(z) + fabs(EA(m + 1, m + 1)));
                if (u + v == v) break;
            }
        }
        eig_sync();
        if (sweep && gl >= m + 2 && gl <= nn) {
            EA(gl, gl - 2) = 0.0;
            if (gl != m + 2) EA(gl, gl - 3) = 0.0;
        }
        eig_sync();
        // ---- the sweep: step k of every sweeping group at once
        for (int k = 0; k < n - 1; ++k) {
            const bool stepk = sweep && k >= m && k <= nn - 1;
            bool doit = false;
            double hx = 0.0, hy = 0.0, hz = 0.0, sub = 0.0;
            const bool three = k != nn - 1;
            if (stepk) {
                if (k != m) {
                    p = EA(k, k - 1);
                    q = EA(k + 1, k - 1);
                    r = three ? EA(k + 2, k - 1) : 0.0;
                    x = fabs(p) + fabs(q) + fabs(r);
                    if (x != 0.0) { p /= x; q /= x; r /= x; }
                }
                const double s = copysign(sqrt(p * p + q * q + r * r), p);
                if (!(s == 0.0 || s != s)) {
                    doit = true;
                    sub = (k == m) ? ((l != m) ? -EA(k, k - 1) : 0.0) : -s * x;
                    p += s;
                    hx = p / s; hy = q / s; hz = r / s;
                    q /= p; r /= p;
                }
            }
            eig_sync();
            if (doit) {
                if (gl == 0 && !(k == m && l == m)) EA(k, k - 1) = sub;
                if (gl >= k && gl <= nn) {         // from the left: lane gl owns column gl
                    double pp = EA(k, gl) + q * EA(k + 1, gl);
                    if (three) {
                        pp += r * EA(k + 2, gl);
                        EA(k + 2, gl) = EA(k + 2, gl) - pp * hz;
                    }
                    EA(k + 1, gl) = EA(k + 1, gl) - pp * hy;
                    EA(k, gl) = EA(k, gl) - pp * hx;
                }
            }
            eig_sync();
            if (doit) {
                const int mmin = nn < k + 3 ? nn : k + 3;
                if (gl >= l && gl <= mmin) {       // from the right: lane gl owns row gl
                    double pp = hx * EA(gl, k) + hy * EA(gl, k + 1);
                    if (three) {
                        pp += hz * EA(gl, k + 2);
                        EA(gl, k + 2) = EA(gl, k + 2) - pp * r;
                    }
                    EA(gl, k + 1) = EA(gl, k + 1) - pp * q;
                    EA(gl, k) = EA(gl, k) - pp;
                }
            }
            eig_sync();
        }
    }
    if (act) status = PCK_ST_EIG_NOCONV;
    return status;
}

template <int G>
__global__ void __launch_bounds__(64) k_eig_grp(const double* __restrict__ a, int ns, int64_t n, int64_t ld,
                                                const int32_t* __restrict__ status_in, double re_tol, pck_eig_out o) {
    extern __shared__ double eig_lds[];
    constexpr int PER = 64 / G;
    const int grp = threadIdx.x / G, gl = threadIdx.x % G;
    const int64_t c = (int64_t)blockIdx.x * PER + grp;
    double* M = eig_lds + grp * G * G;
    const bool have = c < n;
    int status = have ? (status_in ? status_in[c] : PCK_ST_OK) : PCK_ST_NONFINITE;
    bool on = have && status == PCK_ST_OK;
    // row gl of the matrix; a non-finite entry anywhere in the group's matrix
    bool bad = false;
    if (on && gl < ns)
        for (int q = 0; q < ns; ++q) {
            const double v = a[((int64_t)gl * ns + q) * ld + c];
            EA(gl, q) = v;
            bad = bad || !isfinite(v);
        }
    const unsigned long long votes = __ballot(bad);
    const unsigned long long mine = (G == 64) ? ~0ull : (((1ull << (G & 63)) - 1ull) << (grp * G));
    if (on && (votes & mine)) {
        status = PCK_ST_NONFINITE;
        on = false;
    }
    eig_sync();
    EigEmit em;
    em.o = o; em.c = c; em.re_tol = re_tol;
    eig_stats_init(em.st);
    const double fro = eig_grp_balance<G>(M, ns, gl, on);
    const double scale = (double)ns * PCK_EIG_EPS * fro;
    eig_grp_hessenberg<G>(M, ns, gl, on);
    const int st = eig_grp_hqr<G>(M, ns, gl, on, em);
    if (on) {
        status = st;
        if (status == PCK_ST_OK && em.st.bad) status = PCK_ST_NONFINITE;
    }
    if (have && gl == 0) eig_write_summary(o, c, ns, status, em.st, scale);
}
#undef EA
#endif  // __HIPCC__

}  // namespace pck
