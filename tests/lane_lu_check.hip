// Stand-alone check of the lane LU (tests/test_lane_lu.py compiles and runs it):
//   lane_lu_check IN OUT
// IN holds, for NS = 2, 4, 5, 8 in turn, 256 matrices [256][NS][NS] and 256
// right-hand sides [256][NS] (fp64, row-major).  Every system is factored and
// solved twice on the device, one lane per system, four wavefronts of 64:
//   path 0  lu() + lu_solve(): the branch on the wave-uniform `swaps` taken
//           per solve
//   path 1  lu() + lu_solve_impl<NS, SWAPS>, SWAPS chosen once from `swaps`:
//           what the lane integrator's stage sequence runs (mk_solver.h:
//           rodas_stages)
// OUT gets, per NS and per path, [256] records of NS*NS factors, NS solution
// entries, ok (0 / 1) and whether the wavefront swapped a row (swaps != 0).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../pycatkin_amd/csrc/mk_device.h"

#define CHECK(x)                                                                       \
    do {                                                                               \
        hipError_t e_ = (x);                                                           \
        if (e_ != hipSuccess) {                                                        \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                    \
            return 2;                                                                  \
        }                                                                              \
    } while (0)

constexpr int NSYS = 256;
constexpr int NPATH = 2;

template <int NS>
__global__ void __launch_bounds__(64) k_check(const double* A0, const double* b0, double* out) {
    constexpr int REC = NS * NS + NS + 2;
    const int c = blockIdx.x * 64 + threadIdx.x;   // grid = NSYS / 64 blocks of 64: c < NSYS
    const double* Ac = A0 + (size_t)c * NS * NS;
    auto load = [&](double (&M)[NS][NS]) {
#pragma unroll
        for (int i = 0; i < NS; ++i)
#pragma unroll
            for (int q = 0; q < NS; ++q) M[i][q] = Ac[i * NS + q];
    };
    auto store = [&](int path, const double (&M)[NS][NS], const double (&x)[NS], bool ok, bool fb) {
        double* o = out + ((size_t)path * NSYS + c) * REC;
#pragma unroll
        for (int i = 0; i < NS; ++i)
#pragma unroll
            for (int q = 0; q < NS; ++q) o[i * NS + q] = M[i][q];
#pragma unroll
        for (int i = 0; i < NS; ++i) o[NS * NS + i] = x[i];
        o[NS * NS + NS] = ok ? 1.0 : 0.0;
        o[NS * NS + NS + 1] = fb ? 1.0 : 0.0;
    };
    double A[NS][NS], x[NS];
    int piv[NS];
    unsigned sw;
    {
        load(A);
#pragma unroll
        for (int i = 0; i < NS; ++i) x[i] = b0[c * NS + i];
        const bool ok = pck::lu<NS>(A, piv, sw);
        pck::lu_solve<NS>(A, piv, sw, x);
        store(0, A, x, ok, sw != 0u);
    }
    {
        load(A);
#pragma unroll
        for (int i = 0; i < NS; ++i) x[i] = b0[c * NS + i];
        const bool ok = pck::lu<NS>(A, piv, sw);
        const unsigned swu = (unsigned)__builtin_amdgcn_readfirstlane((int)sw);
        if (swu == 0u)
            pck::lu_solve_impl<NS, false>(A, piv, 0u, x);
        else
            pck::lu_solve_impl<NS, true>(A, piv, swu, x);
        store(1, A, x, ok, swu != 0u);
    }
}

template <int NS>
int run(FILE* in, FILE* outf) {
    constexpr int REC = NS * NS + NS + 2;
    std::vector<double> A((size_t)NSYS * NS * NS), b((size_t)NSYS * NS), out((size_t)NPATH * NSYS * REC);
    if (fread(A.data(), sizeof(double), A.size(), in) != A.size()) return 3;
    if (fread(b.data(), sizeof(double), b.size(), in) != b.size()) return 3;
    double *dA, *db, *dout;
    CHECK(hipMalloc(&dA, A.size() * sizeof(double)));
    CHECK(hipMalloc(&db, b.size() * sizeof(double)));
    CHECK(hipMalloc(&dout, out.size() * sizeof(double)));
    CHECK(hipMemcpy(dA, A.data(), A.size() * sizeof(double), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(db, b.data(), b.size() * sizeof(double), hipMemcpyHostToDevice));
    k_check<NS><<<NSYS / 64, 64>>>(dA, db, dout);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out.data(), dout, out.size() * sizeof(double), hipMemcpyDeviceToHost));
    CHECK(hipFree(dA));
    CHECK(hipFree(db));
    CHECK(hipFree(dout));
    if (fwrite(out.data(), sizeof(double), out.size(), outf) != out.size()) return 4;
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 1;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* outf = fopen(argv[2], "wb");
    if (!in || !outf) {
        fprintf(stderr, "cannot open %s / %s\n", argv[1], argv[2]);
        return 1;
    }
    int rc = run<2>(in, outf);
    if (!rc) rc = run<4>(in, outf);
    if (!rc) rc = run<5>(in, outf);
    if (!rc) rc = run<8>(in, outf);
    fclose(in);
    if (fclose(outf) != 0 && !rc) rc = 4;
    return rc;
}
