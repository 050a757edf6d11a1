// Reactor cascade (tanks in series): `cells` CSTR cells at one temperature,
// marched by one lane per condition in one launch (pck_solve_cascade).
//
// Cell c is solved by the rule of a pck_solve steady solve (solve_lane of
// mk_solver.h: screening trip, full solve where the trip is not accepted,
// Newton polish with the distance test); its inflow on the flow rows
// (fl != 0) is the state of cell c-1 on those rows, cell 0 takes the
// condition's inflow.  Rate constants and fixed species are the condition's:
// lane_setup and load_keff run once per lane.
//
// Per-lane LDS (stride = blockDim), after the [kf R][kr R][inflow NS] block of
// lane_setup: [start NS][sums 3].  `start` is the state a cell's transient
// begins from (y0, or with PCK_CASCADE_START_UPSTREAM the previous cell's
// final state); solve_cell reads it from there as solve_lane reads cv.y0, so
// that it is not held in registers across the screening trip.  The running
// sums (TOF; steps and the any-cell-reported-4 flag; failing status and cell)
// live in the three `sums` slots: the compiled-plan CSTR solvers sit at the
// register limit, and the sums would add to the live set of the integrator.
// No lane reads another lane's column, so no barrier is needed.
#pragma once
#include "mk_solver.h"

namespace pck {

struct CascadeArgs {
    int cells, start;
    double* y_cells; int64_t ld_yc;      // [cells][NS][ld_yc] or nullptr
    double* tof_cells; int32_t* status_cells; int32_t* nsteps_cells; int64_t ld_c;   // [cells][ld_c], each or nullptr
    int32_t* cell_fail;                  // [n] or nullptr
};

#define PCK_CASCADE_SUMS 3

// X(id, type): the compiled-in plans (networks.h) that have a flow row, the
// CSTR networks -- a cascade of cells without flow is refused
#define PCK_INST_CASCADE_CT(X) X(2, nets::CstrPd111) X(3, nets::CstrAuPd)

__host__ __device__ inline size_t cascade_lds_bytes(int R, int NS, int B) {
    return lds_bytes(R, NS, B) + sizeof(double) * (size_t)(NS + PCK_CASCADE_SUMS) * B;
}

// One cell's solve: solve_lane's sequence from the start state in the lane's
// LDS column ys (stride ks).  Returns the status; ns = integrator steps.
template <class P, class K>
__device__ __forceinline__ int solve_cell(const P& p, const Lane<P::NS>& L, const K& k, const SolveArgs& a,
                                          const double* ys, int ks, double (&y)[P::NS], int& ns, const TrajOut& to) {
    constexpr int NS = P::NS;
    int st, total = 0, nsp = 0;
    if (a.screen_rtol > 0.0) {
#pragma unroll
        for (int i = 0; i < NS; ++i) y[i] = ys[i * ks];
        st = integrate<false>(p, L, k, y, a.t0, a.t_end, a.screen_rtol, a.screen_atol, a.screen_max_steps, nsp,
                              a.cons_rows != 0, to);
        if (st == PCK_ST_OK && a.newton) st = newton(p, L, k, y, a.newton_iters, a.screen_dist, a.atol);
        total = nsp;
        if (st == PCK_ST_OK) {
            ns = total;
            return st;
        }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) y[i] = ys[i * ks];
    st = integrate<false>(p, L, k, y, a.t0, a.t_end, a.rtol, a.atol, a.max_steps, nsp, a.cons_rows != 0, to);
    if (st == PCK_ST_OK && a.newton) st = newton(p, L, k, y, a.newton_iters, a.root_dist, a.atol);
    total += nsp;
    ns = total;
    return st;
}

// SolveArgs: y / tof / status / nsteps are the summaries (outlet state, mean
// cell TOF, summary status, summed steps); G, idx, worder, t_out are not used.
template <class P>
__global__ void __launch_bounds__(PCK_SOLVE_BLOCK) __attribute__((amdgpu_waves_per_eu(PCK_SOLVE_WAVES)))
k_cascade(NetView nv, CondView cv, const double* kf, const double* kr, int64_t ld_k, SolveArgs a, CascadeArgs ca) {
    constexpr int NS = P::NS;
    extern __shared__ double lds[];
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int R = nv.NRXN;
    const int ks = blockDim.x;
    P p(nv);
    typename KFor<P>::type k;
    if constexpr (!P::CT) {
        k.kf = lds + threadIdx.x;
        k.kr = lds + (size_t)R * ks + threadIdx.x;
        k.ks = ks;
    }
    if (c >= cv.n) return;              // (no barrier below: a lane owns its LDS column)
    Lane<NS> L;
    lane_setup(p, nv, cv, c, L, lds + threadIdx.x, ks);
    load_keff(p, nv, cv, c, kf, kr, ld_k, k, -1, 1.0);
    double* ins = lds + threadIdx.x + (size_t)2 * R * ks;      // lane_setup's inflow block
    double* ys = ins + (size_t)NS * ks;
    double* sums = ys + (size_t)NS * ks;
    int* isum = (int*)(sums + ks);                             // [0] steps, [1] a cell reported PCK_ST_NEWTON
    int* ifail = (int*)(sums + 2 * ks);                        // [0] failing status (0: none), [1] its cell
#pragma unroll
    for (int i = 0; i < NS; ++i) ys[i * ks] = cv.y0[i * cv.ld_y0 + c * cv.s_y0];
    sums[0] = 0.0;
    isum[0] = 0; isum[1] = 0;
    ifail[0] = 0; ifail[1] = -1;
    const TrajOut to{nullptr, 0, nullptr, 0, c};
    const double nan = __builtin_nan("");
    for (int cell = 0; cell < ca.cells; ++cell) {
        const int64_t oc = (int64_t)cell * ca.ld_c + c;
        const int failed = ifail[0];
        if (failed) {
            // the march stopped upstream: NaN states and TOFs, the failing status
            if (ca.y_cells) {
#pragma unroll
                for (int i = 0; i < NS; ++i) ca.y_cells[((int64_t)cell * NS + i) * ca.ld_yc + c] = nan;
            }
            if (ca.tof_cells) ca.tof_cells[oc] = nan;
            if (ca.status_cells) ca.status_cells[oc] = failed;
            if (ca.nsteps_cells) ca.nsteps_cells[oc] = 0;
            continue;
        }
        double y[NS];
        int ns = 0;
        int st = solve_cell(p, L, k, a, ys, ks, y, ns, to);
        const double tof = lane_tof(p, nv, k, y);
        bool fin = isfinite(tof);
#pragma unroll
        for (int i = 0; i < NS; ++i) fin = fin && isfinite(y[i]);
        if (!fin && st == PCK_ST_OK) st = PCK_ST_NONFINITE;
        if (ca.y_cells) {
#pragma unroll
            for (int i = 0; i < NS; ++i) ca.y_cells[((int64_t)cell * NS + i) * ca.ld_yc + c] = y[i];
        }
        if (ca.tof_cells) ca.tof_cells[oc] = tof;
        if (ca.status_cells) ca.status_cells[oc] = st;
        if (ca.nsteps_cells) ca.nsteps_cells[oc] = ns;
        // the outlet is the last solved cell (a failing cell's state included)
        if (a.y) {
#pragma unroll
            for (int i = 0; i < NS; ++i) a.y[i * a.ld_y + c] = y[i];
        }
        sums[0] += tof;
        isum[0] += ns;
        if (st == PCK_ST_NEWTON) isum[1] = 1;
        if (st >= PCK_ST_MAXSTEPS && st <= PCK_ST_NONFINITE) {
            ifail[0] = st;
            ifail[1] = cell;
        } else {
            // this cell's gas is the next cell's inflow
#pragma unroll
            for (int i = 0; i < NS; ++i)
                if (p.fl(i) != 0.0) ins[i * ks] = y[i];
            if (ca.start == PCK_CASCADE_START_UPSTREAM) {
#pragma unroll
                for (int i = 0; i < NS; ++i) ys[i * ks] = y[i];
            }
        }
    }
    const int failed = ifail[0];
    if (a.tof) a.tof[c] = failed ? nan : sums[0] / (double)ca.cells;
    if (a.status) a.status[c] = failed ? failed : (isum[1] ? PCK_ST_NEWTON : PCK_ST_OK);
    if (a.nsteps) a.nsteps[c] = isum[0];
    if (ca.cell_fail) ca.cell_fail[c] = ifail[1];
}

}  // namespace pck
