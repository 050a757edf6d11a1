// Uncertainty-ensemble kernels + their C-ABI entry points (gfx950 / MI355X).
//
//   k_ens_noise   the correlated energy noise of a whole ensemble, written as
//                 the descriptor matrix pck_conditions.desc reads
//                 (Uncertainty.get_correlated_state_noises, uncertainty.py:35-65):
//                 counter-based Philox4x32-10, one thread per (run, Philox block)
//   k_ens_stats   count / mean / population std / min / max over the runs of
//                 each base condition (get_mean_property_value,
//                 uncertainty.py:115-125): per-thread Welford, Chan merges across
//                 the wavefront (__shfl_xor) and across wavefronts (LDS), in a
//                 fixed order: bitwise the same from launch to launch
//
// Both are plain HIP C++: vector loads and stores only, no atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "pycatkin_amd.h"

namespace pck {
// the calling thread's error message lives in mk_kernels.hip (pck_last_error)
int set_error(int code, const char* msg);
}  // namespace pck

namespace {

#define ENS_HIPCHK(x)                                                                 \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) {                                                       \
            char m_[256];                                                             \
            snprintf(m_, sizeof(m_), "HIP error: %s (%d)", hipGetErrorString(e_), (int)e_); \
            return pck::set_error(PCK_E_HIP, m_);                                     \
        }                                                                             \
    } while (0)

// ----------------------------------------------------------------------------
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy
// as 1, 2, 3", SC'11).  The high halves of the two 32 x 32 products come from
// __umulhi, the low halves from the wrapping 32-bit multiply.
// ----------------------------------------------------------------------------
struct U4 { uint32_t x, y, z, w; };

__device__ __forceinline__ U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(M0, c.x), lo0 = M0 * c.x;
        const uint32_t hi1 = __umulhi(M1, c.z), lo1 = M1 * c.z;
        c = U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
        k0 += W0;
        k1 += W1;
    }
    return c;
}

// 53 bits of (w0, w1): ((w0 * 2^32 + w1) >> 11)
__device__ __forceinline__ uint64_t bits53(uint32_t w0, uint32_t w1) {
    return (((uint64_t)w0 << 32) | (uint64_t)w1) >> 11;
}

#define ENS_TWO_M53 1.1102230246251565e-16 /* 2^-53 */
#define ENS_TWO_PI 6.283185307179586

// Thread (i, jy, z): column i of a block of B = n_runs + lead_zero columns,
// Philox block jy (0: row 0, the shared white noise; jy >= 1: the rows of
// transition states 2(jy-1) and 2(jy-1)+1), replicas c = z, z + gridDim.z, ...
// Every thread draws block 0 (row 0 is a factor of every other row) through
// the same instructions, so a row 1+k is bitwise the stored row 0 times u.
__global__ void __launch_bounds__(256) k_ens_noise(uint32_t k0, uint32_t k1, uint64_t run_first, int64_t n_runs,
                                                   int64_t n_rep, int n_ts, int lead_zero, double mu, double sigma,
                                                   double* __restrict__ desc, int64_t ld_desc) {
    const int64_t B = n_runs + lead_zero;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const int jy = (int)blockIdx.y;
    const bool zero = lead_zero && i == 0;
    const uint64_t run = run_first + (uint64_t)(i - lead_zero);
    const uint32_t r_lo = (uint32_t)run, r_hi = (uint32_t)(run >> 32);
    double v0 = 0.0, v1 = 0.0;
    if (!zero) {
        const U4 g = philox4x32_10(U4{r_lo, r_hi, 0u, 0u}, k0, k1);
        const double u1 = (double)(bits53(g.x, g.y) + 1ull) * ENS_TWO_M53;   // (0, 1]
        const double u2 = (double)bits53(g.z, g.w) * ENS_TWO_M53;            // [0, 1)
        const double zn = sqrt(-2.0 * log(u1)) * cos(ENS_TWO_PI * u2);
        const double row0 = mu + sigma * zn;
        if (jy == 0) {
            v0 = row0;
        } else {
            const U4 t = philox4x32_10(U4{r_lo, r_hi, (uint32_t)jy, 0u}, k0, k1);
            v0 = row0 * ((double)bits53(t.x, t.y) * ENS_TWO_M53);
            v1 = row0 * ((double)bits53(t.z, t.w) * ENS_TWO_M53);
        }
    }
    const int row_a = jy == 0 ? 0 : 1 + 2 * (jy - 1);
    const bool two = jy > 0 && 2 * (jy - 1) + 1 < n_ts;
    for (int64_t c = blockIdx.z; c < n_rep; c += gridDim.z) {
        double* col = desc + c * B + i;
        col[(int64_t)row_a * ld_desc] = v0;
        if (two) col[(int64_t)(row_a + 1) * ld_desc] = v1;
    }
}

// ----------------------------------------------------------------------------
// statistics over runs
// ----------------------------------------------------------------------------
// (n, mean, M2, min, max) of a set of values.  The mean is carried as an
// unevaluated sum hi + lo of two doubles: the deviation d = x - mean then
// keeps its full relative accuracy when the values lie close together far
// from 0 (a mean of 1e8 with unit spread), where a one-double Welford mean
// loses cond * eps in M2.
struct Acc {
    int n;
    double hi, lo, m2, mn, mx;
};

// (no fused multiply-adds here: the error term of a two-sum needs the rounded sum)
__device__ __forceinline__ void mean_add(Acc& a, double q) {
#pragma clang fp contract(off)
    const double s = a.hi + q;
    const double bb = s - a.hi;
    const double e = ((a.hi - (s - bb)) + (q - bb)) + a.lo;
    a.hi = s + e;
    a.lo = e - (a.hi - s);
}

// Welford: one value
__device__ __forceinline__ void acc_push(Acc& a, double x) {
#pragma clang fp contract(off)
    a.n += 1;
    const double d = (x - a.hi) - a.lo;
    const double q = d / (double)a.n;
    mean_add(a, q);
    a.m2 += d * (d - q);
    a.mn = fmin(a.mn, x);
    a.mx = fmax(a.mx, x);
}

// Chan, Golub, LeVeque: a <- a U b
__device__ __forceinline__ void acc_merge(Acc& a, const Acc& b) {
#pragma clang fp contract(off)
    if (b.n == 0) return;
    if (a.n == 0) {
        a = b;
        return;
    }
    const double na = (double)a.n, nb = (double)b.n, n = na + nb;
    const double d = (b.hi - a.hi) + (b.lo - a.lo);
    mean_add(a, d * (nb / n));
    a.m2 = (a.m2 + b.m2) + d * d * (na * (nb / n));
    a.n += b.n;
    a.mn = fmin(a.mn, b.mn);
    a.mx = fmax(a.mx, b.mx);
}

__device__ __forceinline__ Acc acc_shfl_xor(const Acc& a, int mask) {
    Acc b;
    b.n = __shfl_xor(a.n, mask, 64);
    b.hi = __shfl_xor(a.hi, mask, 64);
    b.lo = __shfl_xor(a.lo, mask, 64);
    b.m2 = __shfl_xor(a.m2, mask, 64);
    b.mn = __shfl_xor(a.mn, mask, 64);
    b.mx = __shfl_xor(a.mx, mask, 64);
    return b;
}

// butterfly over the 64 lanes; the lower lane of each pair is the left operand,
// so both lanes of a pair hold the same bits and the order is fixed
__device__ __forceinline__ void acc_wave_reduce(Acc& a, int lane) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        Acc b = acc_shfl_xor(a, m);
        if (lane & m) {
            acc_merge(b, a);
            a = b;
        } else {
            acc_merge(a, b);
        }
    }
}

#define ENS_MAX_WAVES 16

// One workgroup per (row q, block c): blockIdx.x = q * n_rep + c.
__global__ void __launch_bounds__(1024) k_ens_stats(const double* __restrict__ v, int64_t ld_v,
                                                    const int32_t* __restrict__ status, uint32_t ok_mask,
                                                    int64_t n_rep, int64_t block, int64_t skip, pck_ens_stats out) {
    __shared__ Acc part[ENS_MAX_WAVES];
    const int64_t q = (int64_t)blockIdx.x / n_rep, c = (int64_t)blockIdx.x % n_rep;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const double* row = v + q * ld_v + c * block;
    const int32_t* st = status ? status + c * block : nullptr;
    Acc a{0, 0.0, 0.0, 0.0, INFINITY, -INFINITY};
    for (int64_t i = skip + threadIdx.x; i < block; i += blockDim.x) {
        const double x = row[i];
        bool ok = isfinite(x);
        if (st) {
            const int32_t s = st[i];
            ok = ok && s >= 0 && s < 32 && ((ok_mask >> s) & 1u);
        }
        if (ok) acc_push(a, x);
    }
    acc_wave_reduce(a, lane);
    if (nw > 1) {
        if (lane == 0) part[wave] = a;
        __syncthreads();
        if (wave != 0) return;
        a = lane < nw ? part[lane] : Acc{0, 0.0, 0.0, 0.0, INFINITY, -INFINITY};
        acc_wave_reduce(a, lane);
    }
    if (threadIdx.x == 0) {
        const int64_t o = q * out.ld_out + c;
        const double n = (double)a.n;
        if (out.count) out.count[o] = a.n;
        if (out.mean) out.mean[o] = a.n ? a.hi + a.lo : NAN;
        if (out.std) out.std[o] = a.n ? sqrt(a.m2 / n) : NAN;
        if (out.min) out.min[o] = a.mn;
        if (out.max) out.max[o] = a.mx;
    }
}

}  // namespace

// Uncertainty.get_correlated_state_noises (uncertainty.py:35-65) for every run
// of an ensemble.
extern "C" int pck_ensemble_noise(uint64_t seed, uint64_t run_first, int64_t n_runs, int64_t n_rep, int64_t n_ts,
                                  int lead_zero, double mu, double sigma, double* desc, int64_t ld_desc,
                                  void* stream) {
    if (!desc) return pck::set_error(PCK_E_ARG, "pck_ensemble_noise: desc is NULL");
    if (n_runs < 0 || n_rep < 0 || n_ts < 0) return pck::set_error(PCK_E_ARG, "pck_ensemble_noise: negative size");
    if (lead_zero != 0 && lead_zero != 1) return pck::set_error(PCK_E_ARG, "pck_ensemble_noise: lead_zero must be 0 or 1");
    const int64_t B = n_runs + lead_zero;
    if (n_rep > 0 && B > INT64_MAX / n_rep) return pck::set_error(PCK_E_ARG, "pck_ensemble_noise: n_rep * B overflows");
    if (ld_desc < n_rep * B) return pck::set_error(PCK_E_ARG, "pck_ensemble_noise: ld_desc < n_rep * (n_runs + lead_zero)");
    const int64_t ny = 1 + (n_ts + 1) / 2;
    if (ny > 65535) return pck::set_error(PCK_E_SIZE, "pck_ensemble_noise: more than 131068 transition states");
    if (B == 0 || n_rep == 0) return PCK_OK;
    const int64_t nx = (B + 255) / 256;
    if (nx > 0x7fffffffLL) return pck::set_error(PCK_E_SIZE, "pck_ensemble_noise: more than 2^39 runs in one call");
    // replicas are split over gridDim.z only until the grid holds ~1024
    // workgroups (4 per CU): a thread writes n_rep / nz columns per row of the
    // values it computed once
    int64_t nz = 1024 / (nx * ny);
    nz = nz < 1 ? 1 : (nz > n_rep ? n_rep : nz);
    if (nz > 65535) nz = 65535;
    hipLaunchKernelGGL(k_ens_noise, dim3((unsigned)nx, (unsigned)ny, (unsigned)nz), dim3(256), 0, (hipStream_t)stream,
                       (uint32_t)seed, (uint32_t)(seed >> 32), run_first, n_runs, n_rep, (int)n_ts, lead_zero, mu,
                       sigma, desc, ld_desc);
    ENS_HIPCHK(hipGetLastError());
    return PCK_OK;
}

// The workgroup of one (row, block): one wavefront up to 256 values a block,
// 4 wavefronts up to 16384, 16 beyond (a lane reads at most 4 / 64 / many
// values).  The geometry depends on `block` alone, so does the merge order.
static int ens_stats_threads(int64_t block) { return block <= 256 ? 64 : (block <= 16384 ? 256 : 1024); }

// np.mean / np.std over runs (uncertainty.py:115-125) for every property row
// and base condition.
extern "C" int pck_ensemble_stats(const double* v, int64_t ld_v, int64_t n_rows, const int32_t* status,
                                  uint32_t ok_mask, int64_t n_rep, int64_t block, int64_t skip,
                                  const pck_ens_stats* out, void* stream) {
    if (!v || !out) return pck::set_error(PCK_E_ARG, "pck_ensemble_stats: v or out is NULL");
    if (n_rows < 0 || n_rep < 0 || block < 0 || skip < 0) return pck::set_error(PCK_E_ARG, "pck_ensemble_stats: negative size");
    if (n_rep > 0 && block > INT64_MAX / n_rep) return pck::set_error(PCK_E_ARG, "pck_ensemble_stats: n_rep * block overflows");
    if (ld_v < n_rep * block) return pck::set_error(PCK_E_ARG, "pck_ensemble_stats: ld_v < n_rep * block");
    const bool any = out->count || out->mean || out->std || out->min || out->max;
    if (any && out->ld_out < n_rep) return pck::set_error(PCK_E_ARG, "pck_ensemble_stats: ld_out < n_rep");
    if (!any || n_rows == 0 || n_rep == 0) return PCK_OK;
    if (n_rows > 0x7fffffffLL / n_rep) return pck::set_error(PCK_E_SIZE, "pck_ensemble_stats: n_rows * n_rep exceeds 2^31 - 1");
    hipLaunchKernelGGL(k_ens_stats, dim3((unsigned)(n_rows * n_rep)), dim3(ens_stats_threads(block)), 0,
                       (hipStream_t)stream, v, ld_v, status, ok_mask, n_rep, block, skip, *out);
    ENS_HIPCHK(hipGetLastError());
    return PCK_OK;
}
