// The serial eigenvalue core of k_eig_lane (csrc/mk_eig.h: eig_serial) on the
// CPU: a stand-alone host program over the very text the kernel runs, no device
// call at run time (tests/test_spectrum_host.py).
//
//   eig_host_check in.bin out.bin
//
// in.bin:  int32 count, then per matrix: int32 ns, int32 budget (0: the
//          kernel's eig_budget(ns)), ns * ns doubles (row-major)
// out.bin: per matrix: status, scale, wr[ns], wi[ns] as doubles
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../pycatkin_amd/csrc/mk_eig.h"

struct HostMat {
    double* m;
    int n;
    double get(int i, int j) const { return m[i * n + j]; }
    void set(int i, int j, double v) { m[i * n + j] = v; }
};
struct HostOut {
    double* wr;
    double* wi;
    void put(int k, double re, double im) { wr[k] = re; wi[k] = im; }
};

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 3;
    int32_t count = 0;
    if (fread(&count, sizeof(count), 1, fi) != 1) return 4;
    for (int32_t k = 0; k < count; ++k) {
        int32_t hdr[2];
        if (fread(hdr, sizeof(int32_t), 2, fi) != 2) return 4;
        const int ns = hdr[0];
        if (ns < 1 || ns > PCK_MAX_DYN) return 5;
        std::vector<double> a((size_t)ns * ns), rec(2 + 2 * (size_t)ns, NAN);
        if (fread(a.data(), sizeof(double), a.size(), fi) != a.size()) return 4;
        HostMat A{a.data(), ns};
        HostOut E{rec.data() + 2, rec.data() + 2 + ns};
        double scale;
        const int st = pck::eig_serial(A, ns, E, scale, hdr[1] > 0 ? hdr[1] : pck::eig_budget(ns));
        rec[0] = (double)st;
        rec[1] = scale;
        if (st != PCK_ST_OK)
            for (int i = 0; i < 2 * ns; ++i) rec[2 + i] = NAN;
        if (fwrite(rec.data(), sizeof(double), rec.size(), fo) != rec.size()) return 6;
    }
    fclose(fi);
    if (fclose(fo) != 0) return 6;
    return 0;
}
