// Eigenvalue kernels (csrc/mk_eig.h) + pck_eigvals (gfx950 / MI355X), and what
// pck_stability_at (mk_kernels.hip) launches through pck::launch_eig /
// pck::launch_eig_reduce.
//
//   k_eig_lane     one lane per condition, ns <= PCK_MAX_DYN_LANE
//   k_eig_grp<G>   G = 16 / 32 / 64 lanes per condition
//   k_eig_reduce   the Jacobian restricted to the conservation class
//
// Plain HIP C++: vector loads and stores only, no atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "mk_eig.h"

namespace pck {
// the calling thread's error message lives in mk_kernels.hip (pck_last_error)
int set_error(int code, const char* msg);
int launch_eig(const double* a, int ns, int64_t n, int64_t ld, const int32_t* status_in, double re_tol, int lanes,
               const pck_eig_out* out, int32_t* lanes_used, hipStream_t s);
int launch_eig_reduce(const double* C, const int32_t* cpiv, int NS, int NCONS, const double* jac, int64_t ld,
                      int64_t n, double* jr, hipStream_t s);
}  // namespace pck

namespace {

#define EIG_HIPCHK(x)                                                                 \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) {                                                       \
            char m_[256];                                                             \
            snprintf(m_, sizeof(m_), "HIP error: %s (%d)", hipGetErrorString(e_), (int)e_); \
            return pck::set_error(PCK_E_HIP, m_);                                     \
        }                                                                             \
    } while (0)

// One thread per condition: Jr[i][q] = J[i][q] - sum_l J[i][p_l] C[l][q] / C[l][p_l]
// over the non-pivot species i, q in their order (C in reduced row-echelon form,
// p_l its pivots): d/dy_q of row i with the pivot species eliminated by the laws.
__global__ void __launch_bounds__(256) k_eig_reduce(const double* __restrict__ C, const int32_t* __restrict__ cpiv,
                                                    int NS, int NCONS, const double* __restrict__ jac, int64_t ld,
                                                    int64_t n, double* __restrict__ jr) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    uint64_t piv = 0;                               // NS <= 64
    for (int l = 0; l < NCONS; ++l) piv |= 1ull << cpiv[l];
    const int nr = NS - NCONS;
    int ri = 0;
    for (int i = 0; i < NS; ++i) {
        if ((piv >> i) & 1ull) continue;
        int rq = 0;
        for (int q = 0; q < NS; ++q) {
            if ((piv >> q) & 1ull) continue;
            double v = jac[((int64_t)i * NS + q) * ld + c];
            for (int l = 0; l < NCONS; ++l) {
                const int p = cpiv[l];
                v -= jac[((int64_t)i * NS + p) * ld + c] * C[l * NS + q] / C[l * NS + p];
            }
            jr[((int64_t)ri * nr + rq) * ld + c] = v;
            ++rq;
        }
        ++ri;
    }
}

template <int G>
int launch_grp(const double* a, int ns, int64_t n, int64_t ld, const int32_t* status_in, double re_tol,
               const pck_eig_out& o, hipStream_t s) {
    const int64_t nb = (n + (64 / G) - 1) / (64 / G);
    if (nb > 0x7fffffffLL) return pck::set_error(PCK_E_SIZE, "eigenvalues: more than 2^31 - 1 workgroups");
    hipLaunchKernelGGL(pck::k_eig_grp<G>, dim3((unsigned)nb), dim3(64), pck::eig_grp_lds_bytes<G>(), s, a, ns, n, ld,
                       status_in, re_tol, o);
    EIG_HIPCHK(hipGetLastError());
    return PCK_OK;
}

}  // namespace

int pck::launch_eig(const double* a, int ns, int64_t n, int64_t ld, const int32_t* status_in, double re_tol,
                    int lanes, const pck_eig_out* out, int32_t* lanes_used, hipStream_t s) {
    if (!a || !out) return pck::set_error(PCK_E_ARG, "eigenvalues: a or out is NULL");
    if (ns < 1) return pck::set_error(PCK_E_ARG, "eigenvalues: ns < 1");
    if (n < 0) return pck::set_error(PCK_E_ARG, "eigenvalues: negative batch size");
    if (lanes != PCK_SENS_LANES_GROUP && lanes != PCK_SENS_LANES_ONE && lanes != PCK_SENS_LANES_AUTO)
        return pck::set_error(PCK_E_ARG, "eigenvalues: unknown lanes mode");
    if (ns > PCK_MAX_DYN) return pck::set_error(PCK_E_SIZE, "eigenvalues: ns > PCK_MAX_DYN");
    if (lanes == PCK_SENS_LANES_ONE && ns > PCK_MAX_DYN_LANE)
        return pck::set_error(PCK_E_SIZE, "eigenvalues: one lane per condition takes ns <= PCK_MAX_DYN_LANE");
    if (ld < n || ((out->wr || out->wi) && out->ld_w < n))
        return pck::set_error(PCK_E_ARG, "eigenvalues: a leading dimension is below n");
    const bool one = lanes != PCK_SENS_LANES_GROUP && ns <= PCK_MAX_DYN_LANE;
    const int G = ns <= 16 ? 16 : ns <= 32 ? 32 : 64;
    if (lanes_used) *lanes_used = one ? 1 : G;
    if (n == 0) return PCK_OK;
    if (one) {
        const int64_t nb = (n + 63) / 64;
        if (nb > 0x7fffffffLL) return pck::set_error(PCK_E_SIZE, "eigenvalues: more than 2^31 - 1 workgroups");
        hipLaunchKernelGGL(pck::k_eig_lane, dim3((unsigned)nb), dim3(64), pck::eig_lane_lds_bytes(ns), s, a, ns, n, ld,
                           status_in, re_tol, *out);
        EIG_HIPCHK(hipGetLastError());
        return PCK_OK;
    }
    if (G == 16) return launch_grp<16>(a, ns, n, ld, status_in, re_tol, *out, s);
    if (G == 32) return launch_grp<32>(a, ns, n, ld, status_in, re_tol, *out, s);
    return launch_grp<64>(a, ns, n, ld, status_in, re_tol, *out, s);
}

int pck::launch_eig_reduce(const double* C, const int32_t* cpiv, int NS, int NCONS, const double* jac, int64_t ld,
                           int64_t n, double* jr, hipStream_t s) {
    if (n == 0) return PCK_OK;
    const int64_t nb = (n + 255) / 256;
    if (nb > 0x7fffffffLL) return pck::set_error(PCK_E_SIZE, "eigenvalues: more than 2^31 - 1 workgroups");
    hipLaunchKernelGGL(k_eig_reduce, dim3((unsigned)nb), dim3(256), 0, s, C, cpiv, NS, NCONS, jac, ld, n, jr);
    EIG_HIPCHK(hipGetLastError());
    return PCK_OK;
}

// np.linalg.eigvals of a batch (solver.py:102-106, :156-158), on the device.
extern "C" int pck_eigvals(const double* a, int ns, int64_t n, int64_t ld, const int32_t* status_in, double re_tol,
                           int lanes, const pck_eig_out* out, int32_t* lanes_used, void* stream) {
    return pck::launch_eig(a, ns, n, ld, status_in, re_tol, lanes, out, lanes_used, (hipStream_t)stream);
}
