/* pycatkin_amd C-ABI: batched mean-field microkinetic (MK) solves on MI355X.
 *
 * One "condition" = one independent MK model instance (a temperature /
 * pressure / descriptor-grid point).  Every per-condition array is
 * structure-of-arrays, device-resident, fp64: element (k, c) of an array with
 * leading dimension ld and condition stride s lives at ptr[k*ld + c*s]; a
 * stride of 0 broadcasts one column to every condition.
 *
 * The network is compiled host-side (pycatkin_amd/network.py) into two flat
 * blobs -- int32 `ip` and float64 `dp` -- whose layout is given by the
 * PCK_I_* / PCK_D_* header slots below, and uploaded once with
 * pck_network_create().
 *
 * Each entry point replaces one reference (PyCatKin) Python routine that a
 * ctypes / FFI binding would call for the whole batch:
 *
 *   pck_rate_constants  <- Reaction.calc_rate_constants      pycatkin/classes/reaction.py:94
 *                          (+ State.calc_free_energy          pycatkin/classes/state.py:367,
 *                             ScalingState.calc_free_energy   state.py:519,
 *                             UserDefinedReaction.calc_reaction_energy reaction.py:222)
 *   pck_species_rates   <- System.species_odes + Reactor.rhs  pycatkin/classes/old_system.py:227,
 *                                                             pycatkin/classes/reactor.py:91,141
 *                          System.get_dydt / _fun_ss          pycatkin/classes/system.py:396,528
 *   pck_jacobian        <- System.species_jacobian + Reactor.jacobian old_system.py:293, reactor.py:103,161
 *                          System.get_jacobian / _jac_ss      system.py:493,547
 *   pck_reaction_rates  <- System._calc_rates                 system.py:345
 *                          System.reaction_terms              old_system.py:202
 *   pck_solve           <- System.solve_odes (+ find_steady)  old_system.py:315 (385)
 *                          SteadyStateSolver.solve_ode        pycatkin/classes/solver.py:374
 *                          System.run_and_return_tof / activity old_system.py:470,517
 *   pck_drc             <- System.degree_of_rate_control      old_system.py:490
 *   pck_drc_at          <- System.degree_of_rate_control      old_system.py:490 (its eps -> 0 limit,
 *   pck_drc_adjoint        analytic: one steady solve + one adjoint solve instead of 2R+1 solves)
 *   pck_sens_at         <- (none: the reference has no reaction orders, apparent activation
 *   pck_sens_adjoint       energy or per-direction sensitivities; the same adjoint solve gives them)
 *   pck_drc_multi_at    <- (none: selectivity and coverage control, the rate-control matrix:
 *   pck_drc_multi_adjoint  K objectives passed per call, one factorisation, K adjoint solves)
 *   pck_energy_span     <- Energy.construct_energy_landscape  pycatkin/classes/energy.py:39
 *                          Energy.evaluate_energy_span_model  energy.py:238
 *   pck_ensemble_noise  <- Uncertainty.get_correlated_state_noises pycatkin/classes/uncertainty.py:35
 *   pck_ensemble_stats  <- Uncertainty.get_mean_property_value uncertainty.py:115 (np.mean / np.std over runs)
 *   pck_eigvals         <- the np.linalg.eigvals of SteadyStateSolver.test_convergence
 *   pck_stability_at       pycatkin/classes/solver.py:102-106 and of solve_ode solver.py:156-158
 *   pck_stability          (Jacobian and eigenvalues on the device; + the reduced Jacobian)
 *
 * All functions return 0 on success and a negative PCK_E_* code on failure;
 * pck_last_error() returns a message for the calling thread.  Device pointers
 * only; `stream` is a hipStream_t (NULL = default stream).  Launches are
 * asynchronous on `stream` unless noted.  A network handle is read-only after
 * pck_network_create: every call allocates its own scratch in stream order
 * on `stream` (hipMallocAsync / hipFreeAsync), so calls on different streams
 * may share one network.
 */
#ifndef PYCATKIN_AMD_H
#define PYCATKIN_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCK_ABI_VERSION 10

/* error codes */
#define PCK_OK 0
#define PCK_E_ARG (-1)      /* bad argument / blob layout */
#define PCK_E_HIP (-2)      /* HIP runtime error */
#define PCK_E_SIZE (-3)     /* network exceeds the compiled kernel limits */

/* kernel limits.  Networks with up to PCK_MAX_DYN_LANE dynamic species run
 * one condition per lane (state, Jacobian and LU in VGPRs); larger ones (up to
 * PCK_MAX_DYN) run one condition per lane group of 16/32/64 lanes, one
 * species row per lane (csrc/mk_group.h). */
#define PCK_MAX_DYN 64      /* dynamic species per condition (solver kernels) */
#define PCK_MAX_DYN_LANE 8  /* ... on the one-lane-per-condition path */
#define PCK_MAX_DYN_PLAN 64 /* dynamic species a plan may hold (rate constants / energies) */
#define PCK_MAX_RXN 256     /* active reactions */
#define PCK_MAX_EXP 255     /* stoichiometric exponent */
#define PCK_MAX_CONS 4      /* conservation laws */
#define PCK_MAX_TOF 16      /* TOF terms */
#define PCK_MAX_PES 64      /* entries of an energy landscape (pck_energy_span) */

/* int32 blob header slots (ip[0..PCK_I_HDR)) */
enum {
    PCK_I_VERSION = 0, /* == PCK_ABI_VERSION */
    PCK_I_NDESC,       /* D: descriptors per condition */
    PCK_I_NTH,         /* thermo states (vib/tran/rot features) */
    PCK_I_NREG,        /* energy-program registers */
    PCK_I_NRXN,        /* active reactions R */
    PCK_I_NDYN,        /* dynamic species NS */
    PCK_I_NFIX,        /* fixed (non-dynamic) species F */
    PCK_I_NCONS,       /* conservation laws m */
    PCK_I_NTOF,        /* TOF terms */
    PCK_I_OFF_TH,      /* -> th: NTH x {kind, freq_off, freq_cnt, rot_shape} */
    PCK_I_OFF_REG,     /* -> reg_ptr[NREG+1], reg_clamp[NREG], reg_feat[nnz] */
    PCK_I_OFF_RX,      /* -> rx: NRXN x {type, reversible, reg_ga, reg_grxn, reg_erxn, arr_if_barrier} */
    PCK_I_OFF_EXPF,    /* -> forward exponents  [NRXN][NDYN] */
    PCK_I_OFF_EXPR,    /* -> reverse exponents  [NRXN][NDYN] */
    PCK_I_OFF_FOLDF,   /* -> forward fixed-species exponents [NRXN][NFIX] */
    PCK_I_OFF_FOLDR,   /* -> reverse fixed-species exponents [NRXN][NFIX] */
    PCK_I_OFF_CPIV,    /* -> pivot row of each conservation law [NCONS] */
    PCK_I_OFF_TOF,     /* -> active-reaction index of each TOF term [NTOF] */
    PCK_I_HDR
};

/* float64 blob header-less layout: offsets are stored in the int blob */
enum {
    PCK_D_OFF_SLOT0 = PCK_I_HDR, /* ip[PCK_D_OFF_SLOT0 + k] = dp offset of block k: */
    PCK_D_TH = 0,    /* th: NTH x {zpe [eV], mass [amu], sigma, rotI = sqrt(prod nonzero I) [kg m^2], Gvibr given (NaN = compute)} */
    PCK_D_FREQ,      /* frequency table (Hz) */
    PCK_D_REGCOEF,   /* reg_coef[nnz] */
    PCK_D_RX,        /* rx: NRXN x {kads_c, kdes_c, kdes_texp} */
    PCK_D_STOICH,    /* S[NDYN][NRXN] (weights incl. scaling / site density) */
    PCK_D_DYN,       /* dyn: NDYN x {conc_factor, rowscale0, rowscale_T, flow_rate} */
    PCK_D_CONS,      /* C[NCONS][NDYN] */
    PCK_D_NBLK
};
#define PCK_IP_MIN (PCK_I_HDR + PCK_D_NBLK)

/* register feature index space: 0 = constant 1, 1 = T, 2 .. 2+D-1 = descriptors,
 * then 3 per thermo state (vib, tran, rot), then earlier registers. */

/* reaction rate-constant types (reaction.py:94-168) */
enum {
    PCK_RX_ARRHENIUS = 0,  /* kf = kBT/h exp(-max(dGa,0)/RT); kr = kf/exp(-dGrxn/RT) */
    PCK_RX_ADS_KEQ = 1,    /* kf = kads;  kr = kads/exp(-dGrxn/RT) (classic) */
    PCK_RX_DES_KEQ = 2,    /* kr = kads;  kf = kads*exp(-dGrxn/RT) (classic) */
    PCK_RX_ADS_KDES = 3,   /* kf = kads;  kr = kdes(-dErxn) (reaction.py:135-147) */
    PCK_RX_DES_KDES = 4    /* kf = kdes(dErxn); kr = kads (reaction.py:150-162) */
};

/* thermo state kinds (bit flags) */
#define PCK_TH_VIB 1
#define PCK_TH_GAS 2

typedef struct pck_network pck_network;

/* Per-condition inputs (device pointers; see stride rule above). */
typedef struct {
    int64_t n;                       /* number of conditions */
    const double* T;  int64_t sT;    /* temperature [K] */
    const double* p;  int64_t sp;    /* pressure [Pa] (free energies only) */
    const double* desc; int64_t ld_desc, s_desc;   /* [D][..] descriptor values (eV) */
    const double* fixc; int64_t ld_fix, s_fix;     /* [F][..] fixed-species concentrations */
    const double* y0; int64_t ld_y0, s_y0;         /* [NS][..] initial dynamic state */
    const double* inflow; int64_t ld_in, s_in;     /* [NS][..] inflow (CSTR gas rows) */
} pck_conditions;

typedef struct {
    double t0, t_end;      /* integrate from t0 to t_end */
    double rtol, atol;     /* local error control (RMS norm) */
    int32_t max_steps;     /* per condition */
    int32_t newton;        /* 1: polish to f(y)=0 after the transient (find_steady) */
    int32_t newton_iters;  /* max Newton iterations */
    int32_t want_activity; /* 1: write activity (eV) instead of TOF into tof_out */
    double drc_eps;        /* pck_drc only: relative k perturbation */
    const double* t_out;   /* pck_solve: n_out ascending sample times in [t0, t_end] (device), or NULL */
    int64_t n_out;         /*   the state at each is written to pck_outputs.traj (dense output) */
    double retry_rtol;     /* with newton: a condition whose polish meets a degenerate root */
    double retry_atol;     /*   (PCK_ST_NEWTON) is integrated again, t0..t_end, at these tolerances,
                            *   by a second launch over the compacted list of such conditions on
                            *   the same stream (pck_solve only; 0: off); its y / tof become that
                            *   transient end,
                            *   the reference's System.activity semantics (old_system.py:517-529),
                            *   status stays PCK_ST_NEWTON and nsteps adds the retry's steps; a
                            *   retry that fails keeps the first pass's y / tof (PCK_ST_NEWTON_LOOSE) */
    int32_t wave_order;    /* pck_solve on the lane solver: dispatch the 64-condition wavefronts in
                            *   descending cost, predicted by a preview of 4 lanes of each (a loose
                            *   transient, or the screening trip at rtol 0.2 when the solve screens:
                            *   a wavefront with a sample it does not accept skips its trip);
                            *   1 on, -1 off, 0 auto (on for n >= 131072).  It pays where costs vary
                            *   across the batch and is overhead on a uniform-cost sweep.  Results
                            *   do not depend on it beyond rounding: the same 64 conditions share a
                            *   wavefront either way, and a skipped trip's lanes answer from the
                            *   full solve (the same root to ~1e-13). */
    double root_dist;      /* with newton (> 0): the Newton root is reported (PCK_ST_OK) only if the
                            *   transient end it started from lies within root_dist * |root_i| + atol
                            *   of it in every dynamic species -- the transient has reached that steady
                            *   state by t_end; otherwise the transient end is reported with
                            *   PCK_ST_NEWTON (old_system.py:517-529 System.activity semantics).
                            *   0: any converged, balanced, non-negative root is reported
                            *   (old_system.py:385-468 find_steady from a given state). */
    double screen_rtol;    /* with newton and root_dist > 0 (no trajectory): a screening pass at
                            *   rtol = screen_rtol (atol scaled alike) whose Newton root is accepted
                            *   (PCK_ST_OK) only if the screening transient's end lies within
                            *   screen_margin * root_dist * |root_i| + atol (the caller's atol) of
                            *   it; every other condition solves again from y0 at rtol / atol in the
                            *   same launch, exactly as without screening (y, tof, status of that
                            *   solve; nsteps adds the two trips).  A transient that has settled on
                            *   a root ends on it at any tolerance, so the accepted conditions report
                            *   the root the single pass would (DESIGN.md "Screening pass").  Runs on
                            *   the one-lane solver and the 16- and 32-lane group kernels, pck_solve
                            *   and pck_drc; a network of <= 16 species then leaves the quad-group
                            *   kernel for the 16-lane one; networks of > 32 species (64-lane
                            *   groups) refuse it with PCK_E_ARG.  0: off. */
    double screen_margin;  /*   fraction of root_dist for the screening pass's acceptance (0: 0.1) */
} pck_solve_params;

/* Outputs of pck_solve (device pointers; any may be NULL). */
typedef struct {
    double* y; int64_t ld_y;   /* [NS][ld_y] final dynamic state */
    double* tof;               /* [n] TOF (1/s) or activity (eV) */
    int32_t* status;           /* [n] PCK_ST_* */
    int32_t* nsteps;           /* [n] accepted + rejected steps */
    double* kf; double* kr;    /* [NRXN][ld_k] optional rate-constant dump */
    int64_t ld_k;
    double* traj; int64_t ld_traj;   /* [n_out][NS][ld_traj] states at pck_solve_params.t_out
                                      * (System.solve_odes' solution, old_system.py:350-376);
                                      * needs the hipRTC-specialised kernels (PCK_JIT != 0) */
} pck_outputs;

/* per-condition status codes */
#define PCK_ST_OK 0
#define PCK_ST_MAXSTEPS 1
#define PCK_ST_STEPFAIL 2
#define PCK_ST_NONFINITE 3
/* no steady state reached by t_end (with root_dist: the transient has not
 * reached a root; without: Newton met a degenerate root): y / tof are the
 * transient end at t_end */
#define PCK_ST_NEWTON 4
/* a degenerate root whose tight retry transient failed (step budget / step
 * size): y and tof are the first pass's transient end at the caller's
 * tolerances -- what the reference's own lsoda path reports */
#define PCK_ST_NEWTON_LOOSE 5
/* pck_drc with newton: the 2R+1 solves of a condition fall on both sides of
 * the steady rule (some report a reached root, PCK_ST_OK, others the
 * transient end, PCK_ST_NEWTON / _LOOSE): the central differences then mix
 * two definitions of the answer and xi measures the rule switching, not rate
 * control.  xi / tof0 are still written. */
#define PCK_ST_DRC_MIXED 6
/* pck_drc_at / pck_drc_adjoint: the steady Jacobian (conservation rows in
 * place) has a zero pivot or a non-finite factor; xi are NaN */
#define PCK_ST_SENS_SINGULAR 7
/* pck_sens_at / pck_sens_adjoint: max_j max(rf_j, rr_j) / |TOF| is so large that
 * double-double no longer resolves the per-direction sensitivities (err > err_max):
 * sf, sr, order, order_in and dir are NaN; xi and tof0 are written and reliable */
#define PCK_ST_SENS_PRECISION 8
/* pck_eigvals / pck_stability_at / pck_stability: the QR iteration spent its
 * 30 * max(10, ns) sweeps without isolating every eigenvalue; outputs are NaN */
#define PCK_ST_EIG_NOCONV 9

int pck_abi_version(void);
const char* pck_last_error(void);

/* Upload a compiled network (host blobs) to the current device. */
int pck_network_create(const int32_t* ip, int64_t n_ip, const double* dp, int64_t n_dp,
                       pck_network** out);
int pck_network_destroy(pck_network* net);
/* Sizes of a created network: dims[0..10] = D, NTH, NREG, NRXN, NDYN, NFIX, NCONS, NTOF,
 * n_features, plan id: a compiled-in plan (csrc/networks.h), PCK_PLAN_ID_JIT once a
 * lane solve ran the plan hipRTC specialised for this network (csrc/mk_jit.h;
 * PCK_JIT=0 in the environment disables it), 0 = runtime plan; and the kernel of the
 * last lane-group solve: 0 compiled-in record tables, 1 hipRTC exact-size record
 * tables, 2 hipRTC with the network compiled in (PCK_GRP_CT=0 disables it). */
#define PCK_PLAN_ID_JIT 100
int pck_network_dims(const pck_network* net, int32_t* dims);
/* Lanes per condition of the last lane-group solve (networks beyond the
 * one-lane limits): 4 for the quad-group kernel (csrc/mk_quad.h, <= 16
 * species), else the group width G = 16, 32 or 64 (csrc/mk_group.h: grp_g);
 * 0 before any group solve.  Diagnostic: which kernel answered. */
int pck_network_group_lanes(const pck_network* net, int32_t* lanes);
/* Solver selection (A/B checks): PCK_PLAN_AUTO (default: compiled-in plan when
 * the structural digest matches, else the runtime plan, lane-group solver
 * beyond the one-lane limits), PCK_PLAN_RUNTIME (never the compiled-in plan),
 * PCK_PLAN_GROUP (always the lane-group solver). */
#define PCK_PLAN_AUTO 0
#define PCK_PLAN_RUNTIME 1
#define PCK_PLAN_GROUP 2
int pck_network_set_plan_mode(pck_network* net, int mode);

/* Energy-program registers (eV) per condition: out[r][ld_out], r < NREG.
 * Replaces State.get_free_energy (state.py:388) / Reaction.get_reaction_energy
 * (reaction.py:171) / get_reaction_barriers (reaction.py:182) for a batch.
 * Networks with NDYN == 0 are accepted for this call and pck_rate_constants. */
int pck_energies(const pck_network* net, const pck_conditions* cond, double* out, int64_t ld_out,
                 void* stream);

/* kf, kr: [NRXN][ld_k] outputs (1/s or 1/(s Pa^n) as the reference's). */
int pck_rate_constants(const pck_network* net, const pck_conditions* cond,
                       double* kf, double* kr, int64_t ld_k, void* stream);

/* Effective rates of the dynamic species at states y ([NS][ld_y]):
 * dydt[NS][ld_y] = rowscale * (S . net_rates) + flow.  kf/kr as produced by
 * pck_rate_constants (fixed species are folded in here). */
int pck_species_rates(const pck_network* net, const pck_conditions* cond,
                      const double* kf, const double* kr, int64_t ld_k,
                      const double* y, int64_t ld_y, double* dydt, void* stream);

/* Forward and reverse rate of every active reaction at states y ([NS][ld_y]),
 * fixed-species concentrations folded in: rf, rr [NRXN][ld_r].
 * Replaces System._calc_rates (pycatkin/classes/system.py:345) and
 * System.reaction_terms (pycatkin/classes/old_system.py:202). */
int pck_reaction_rates(const pck_network* net, const pck_conditions* cond,
                       const double* kf, const double* kr, int64_t ld_k,
                       const double* y, int64_t ld_y, double* rf, double* rr, int64_t ld_r,
                       void* stream);

/* Jacobian d(dydt)/dy: jac[(i*NS + k)][ld_y] (row-major per condition). */
int pck_jacobian(const pck_network* net, const pck_conditions* cond,
                 const double* kf, const double* kr, int64_t ld_k,
                 const double* y, int64_t ld_y, double* jac, void* stream);

/* Fused: rate constants -> stiff integration t0..t_end (L-stable Rosenbrock
 * W-method) -> optional Newton steady-state polish -> TOF / activity. */
int pck_solve(const pck_network* net, const pck_conditions* cond,
              const pck_solve_params* prm, const pck_outputs* out, void* stream);

/* Reactor cascade (tanks in series; csrc/mk_cascade.h): `cells` equal CSTR cells at
 * the condition's temperature, marched by one lane per condition in one launch.  Cell
 * c is solved by the rule of pck_solve with these params (prm->newton, root_dist and
 * screen_rtol as there); its inflow on the flow rows (species with a flow rate) is the
 * dynamic state of cell c-1 on those rows, cell 0 takes cond->inflow.  The network's
 * flow rate and row scale are one cell's (classes/reactor.py: PFReactor).  Rate
 * constants and fixed-species concentrations are the condition's, computed once.
 * start: PCK_CASCADE_START_Y0, every cell's transient starts from cond->y0 (what a
 * loop of pck_solve calls computes); PCK_CASCADE_START_UPSTREAM, from the final state
 * of the cell before it (cell 0 from y0).
 * A cell that ends with PCK_ST_NEWTON passes its transient end downstream.  A cell
 * that ends with an integrator failure (PCK_ST_MAXSTEPS / _STEPFAIL / _NONFINITE)
 * stops the condition's march: its index goes to cell_fail and every later cell of
 * the condition gets NaN states and TOFs, that status and 0 steps.
 * Per-cell outputs (optional, device pointers): */
#define PCK_MAX_CELLS 4096
#define PCK_CASCADE_START_Y0 0
#define PCK_CASCADE_START_UPSTREAM 1
typedef struct {
    int32_t cells, start;
    double* y_cells; int64_t ld_yc;          /* [cells][NS][ld_yc] or NULL */
    double* tof_cells; int32_t* status_cells; int32_t* nsteps_cells; int64_t ld_c;  /* [cells][ld_c], each may be NULL */
    int32_t* cell_fail;                      /* [n], -1 where no cell failed; may be NULL */
} pck_cascade;
/* pck_outputs: y the outlet (the state of the last solved cell, the failing one where
 * the march stopped); tof the mean of the cell TOFs (equal catalyst area per cell; NaN
 * where the march stopped); status the failing status if there is one, else
 * PCK_ST_NEWTON if any cell reported it, else PCK_ST_OK; nsteps the sum over the cells;
 * kf / kr dumped as by pck_solve.
 * PCK_E_SIZE (checked first): a network beyond the one-lane limits (PCK_MAX_DYN_LANE
 * species, the k_eff block in LDS) or one set to PCK_PLAN_GROUP.  PCK_E_ARG: cells
 * outside 1..PCK_MAX_CELLS, an unknown start, t_out / traj, retry_rtol != 0,
 * want_activity, or a network without a flow row (identical cells).  wave_order is
 * ignored (no preview).  Plans as pck_solve: compiled-in, hipRTC (PCK_JIT=0 disables
 * it), runtime. */
int pck_solve_cascade(const pck_network* net, const pck_conditions* cond, const pck_solve_params* prm,
                      const pck_cascade* cas, const pck_outputs* out, void* stream);

/* Degree of rate control for every active reaction (old_system.py:490):
 * xi[j][ld_xi] = (TOF(k_j*(1+eps)) - TOF(k_j*(1-eps))) / (2 eps TOF0).
 * tof0 (optional) receives the unperturbed TOF; status (optional) the worst
 * status of the 2R+1 solves (PCK_ST_NONFINITE also for a zero / non-finite
 * TOF0; PCK_ST_DRC_MIXED where they mix reached roots and transient ends);
 * nsteps (optional) the sum of their integrator steps. */
int pck_drc(const pck_network* net, const pck_conditions* cond,
            const pck_solve_params* prm, double* xi, int64_t ld_xi,
            double* tof0, int32_t* status, int32_t* nsteps, void* stream);

/* Analytic degree of rate control (old_system.py:490 System.degree_of_rate_control
 * in the limit eps -> 0) at given steady states y ([NS][ld_y]), kf / kr as
 * pck_rate_constants gives them: xi[j][ld_xi] = d ln TOF / d ln k_j at fixed K_j for
 * every active reaction, from one adjoint solve per condition,
 *   A^T lambda = dTOF/dy,   xi_j = ([j in tof] net_j - lambda . dF/dln k_j) / TOF0,
 * with F the steady equations as pck_solve's Newton polish poses them (the
 * conservation laws in their pivot rows, a unit row for a species that is exactly 0
 * with an exactly zero rate) and A = dF/dy.  Rates, Jacobian, factorisation and
 * substitution are double-double: the matrix has condition ~1e16 at a steady state
 * and fp64 leaves no digit of xi (DESIGN.md "Analytic DRC").  The states are taken
 * as steady; nothing checks that they are.
 * status_in (optional) gates the conditions: only PCK_ST_OK rows are computed, any
 * other keeps its status and gets NaN xi.  tof0 (optional) is written for every
 * condition.  status (optional): PCK_ST_NONFINITE for a zero or non-finite TOF0,
 * PCK_ST_SENS_SINGULAR for a zero pivot or a non-finite factor (NaN xi both).
 * Networks of up to PCK_MAX_DYN species and PCK_MAX_RXN reactions whose reactions
 * fit the lane-group records (<= 6 dynamic participants, exponents <= 31), else
 * PCK_E_SIZE; a network without TOF terms is PCK_E_ARG. */
int pck_drc_at(const pck_network* net, const pck_conditions* cond, const double* kf, const double* kr,
               int64_t ld_k, const double* y, int64_t ld_y, const int32_t* status_in,
               double* xi, int64_t ld_xi, double* tof0, int32_t* status, void* stream);

/* System.degree_of_rate_control(ss_solve=True) (old_system.py:490) in the limit
 * eps -> 0: one steady solve (pck_solve with prm->newton = 1: rule, root_dist,
 * screening, retry and wave order as given) and then pck_drc_at at its states.  Same
 * outputs as pck_drc; prm->drc_eps and prm->want_activity are ignored.  A condition
 * whose solve did not report a reached root (status != PCK_ST_OK) keeps that status:
 * its xi are NaN, its tof0 the TOF of the state the solve reports.  nsteps
 * (optional): the solve's steps.  PCK_E_ARG: prm->newton == 0 (a transient end has
 * no implicit-function sensitivity), a trajectory request (t_out / n_out). */
int pck_drc_adjoint(const pck_network* net, const pck_conditions* cond, const pck_solve_params* prm,
                    double* xi, int64_t ld_xi, double* tof0, int32_t* status, int32_t* nsteps, void* stream);

/* Adjoint sensitivities of the TOF at steady states: what pck_drc_at's adjoint
 * vector lambda gives beyond xi.  For any parameter theta of the steady equations
 *   d TOF / d theta = dTOF/dtheta|_y - lambda . dF/dtheta|_y,
 * and with s_j = [j in tof] - sum_i lambda_i w_i S_ij (the bracket of xi_j; w_i the row
 * scale, 0 on a replaced row) and rf_j / rr_j the forward / reverse rate of reaction j
 * every output below is a sum of s_j rf_j and s_j rr_j.  Device pointers, each
 * optional (NULL: not wanted); [rows][ld] with ld >= n. */
typedef struct {
    double* xi; int64_t ld_xi;        /* [NRXN][ld_xi]  d ln TOF / d ln k_j at fixed K_j = (rf_j - rr_j) s_j / TOF,
                                       *   bitwise what pck_drc_at writes */
    double* sf; double* sr;           /* [NRXN][ld_s]   d ln TOF / d ln kf_j = rf_j s_j / TOF and
                                       *   d ln TOF / d ln kr_j = -rr_j s_j / TOF, each at the other fixed
                                       *   (sf + sr = xi) */
    int64_t ld_s;
    double* order; int64_t ld_order;  /* [NFIX][ld_order]  reaction order d ln TOF / d ln c_q in the
                                       *   concentration of every fixed species q:
                                       *   sum_j s_j (ef_jq rf_j - er_jq rr_j) / TOF, ef / er its exponents */
    double* order_in; int64_t ld_in;  /* [NDYN][ld_in]  d ln TOF / d ln in_i in the inflow of a dynamic
                                       *   species with a flow term fl (in - y) (the CSTR's gas rows):
                                       *   -lambda_i fl_i in_i / TOF; 0 for a row without a flow term or a
                                       *   replaced row */
    double* dir; int64_t ld_dir;      /* [nd][ld_dir]  the directions of pck_sens_dirs */
    double* err;                      /* [n]  the guard's bound, 2^-98 max_j max(rf_j, rr_j) / |TOF| */
    double* tof0;                     /* [n]  the TOF at the given states (every condition) */
    int32_t* status;                  /* [n]  PCK_ST_* */
} pck_sens_out;

/* User directions: dir[m] = sum_j (a_mj sf_j + c_mj sr_j), the derivative of ln TOF
 * along d ln kf_j = a_mj, d ln kr_j = c_mj, summed in double-double and rounded once.
 * a = c = 1 gives sum_j xi_j; a_j = d ln kf_j / dT, c_j = d ln kr_j / dT gives
 * d ln TOF / dT at fixed gas composition (the apparent activation energy over R T^2);
 * a state-energy or thermodynamic-DRC direction is one row.  Device pointers. */
typedef struct {
    int64_t nd;                       /* number of directions (0: none) */
    const double* a; const double* c; /* [nd][NRXN][ld]: entry (m, j) of condition i at m * stride + j * ld + i */
    int64_t ld, stride;               /* ld >= n; stride >= NRXN * ld */
} pck_sens_dirs;

/* The adjoint sensitivities at given steady states y ([NS][ld_y]), kf / kr as
 * pck_rate_constants gives them: pck_drc_at's assembly, factorisation and adjoint solve
 * (double-double throughout), then the outputs of pck_sens_out.  dirs may be NULL.
 * The guard: sf_j = rf_j s_j / TOF needs s_j to an absolute accuracy of TOF / rf_j,
 * which xi_j = (rf_j - rr_j) s_j / TOF does not, and double-double carries s_j to about
 * 2^-98.  err = 2^-98 max_j max(rf_j, rr_j) / |TOF| bounds the error of every output
 * but xi; with err_max > 0, a condition with err > err_max gets NaN sf, sr, order,
 * order_in and dir and PCK_ST_SENS_PRECISION, its xi, tof0 and err as always
 * (err_max <= 0: no guard; 1e-9 keeps every regular steady state of the test networks
 * with |TOF| > 1e-40).  The bound is safe, not tight.
 * status_in, PCK_ST_NONFINITE and PCK_ST_SENS_SINGULAR as pck_drc_at: NaN in every
 * output but tof0.  Sizes and refusals as pck_drc_at; PCK_E_ARG also for a leading
 * dimension below n or directions without a / c / dir. */
int pck_sens_at(const pck_network* net, const pck_conditions* cond, const double* kf, const double* kr,
                int64_t ld_k, const double* y, int64_t ld_y, const int32_t* status_in,
                const pck_sens_dirs* dirs, double err_max, const pck_sens_out* out, void* stream);

/* One steady solve (pck_solve with prm->newton = 1, as pck_drc_adjoint) and then
 * pck_sens_at at its states, with the solve's own rate constants.  dirs are per
 * condition of `cond`.  nsteps (optional): the solve's steps.  A condition whose solve
 * did not report a reached root keeps that status and gets NaN outputs (tof0: the TOF
 * of the state the solve reports).  PCK_E_ARG: prm->newton == 0, a trajectory request. */
int pck_sens_adjoint(const pck_network* net, const pck_conditions* cond, const pck_solve_params* prm,
                     const pck_sens_dirs* dirs, double err_max, const pck_sens_out* out, int32_t* nsteps,
                     void* stream);

/* Lanes per condition of the adjoint kernels behind pck_drc_at, pck_drc_adjoint,
 * pck_sens_at and pck_sens_adjoint: PCK_SENS_LANES_GROUP (default: G = 16, 32 or 64
 * lanes own one condition, csrc/mk_sens.h over the steps of csrc/mk_adjoint.h),
 * PCK_SENS_LANES_ONE (one lane per condition, csrc/mk_sens_lane.h: the same formulas, statuses and outputs, every
 * step serial in its lane; networks of up to PCK_MAX_DYN_LANE dynamic species, else
 * PCK_E_SIZE from this call), PCK_SENS_LANES_AUTO (one lane up to PCK_MAX_DYN_LANE
 * species, else the group kernels).  Any other mode is PCK_E_ARG.  The two kinds
 * agree to rounding, not bitwise (sums over reactions run in another order); the
 * argument checks of the four entry points are the same in every mode. */
#define PCK_SENS_LANES_GROUP 0
#define PCK_SENS_LANES_ONE 1
#define PCK_SENS_LANES_AUTO 2
int pck_network_set_sens_lanes(pck_network* net, int mode);
/* Lanes per condition of the last adjoint launch: 1, 16, 32 or 64; 0 before any.
 * Diagnostic, as pck_network_group_lanes: which kernel answered. */
int pck_network_sens_lanes(const pck_network* net, int32_t* lanes);

/* Multi-objective analytic degree of rate control: K objectives that are data of the
 * call, not of the plan (a network without TOF terms is accepted),
 *   J_m = sum_j wr[m][j] net_j + sum_i wy[m][i] y_i,
 * net_j the net rate of active reaction j (plan order), y_i the state variable of
 * dynamic species i as given (not its concentration cf_i y_i): a sum of net rates
 * (a TOF; num and den of a selectivity), a coverage or a CSTR's outlet concentration
 * (one entry of wy), or any mix.  Device pointers, per network, not per condition;
 * either may be NULL (all zero), not both. */
typedef struct {
    int K;                            /* number of objectives, >= 1 */
    const double* wr;                 /* [K][NRXN] */
    const double* wy;                 /* [K][NDYN] */
} pck_multi_obj;

/* Device pointers; [rows][ld] with ld >= n.  val and xi are required. */
typedef struct {
    double* val; int64_t ld_val;      /* [K][ld_val]  J_m at the given states (every condition) */
    double* xi; int64_t ld_xi;        /* [K * NRXN][ld_xi]  row m * NRXN + j: d ln J_m / d ln k_j at fixed K_j */
    int32_t* status;                  /* [n]  PCK_ST_* of the condition (optional) */
    int32_t* ostatus; int64_t ld_os;  /* [K][ld_os]  PCK_ST_* of each objective (optional) */
} pck_multi_out;

/* The degree of rate control of K objectives at given steady states y ([NS][ld_y]),
 * kf / kr as pck_rate_constants gives them (the reference has none of this: its
 * degree_of_rate_control knows one TOF; replaces nothing in the reference).
 * pck_drc_at's assembly and equilibration, one LU factorisation whose multipliers are
 * kept, and per objective one adjoint solve on the stored factors,
 *   A^T lambda_m = dJ_m/dy,   xi[m][j] = net_j (wr[m][j] - sum_i lambda_mi w_i S_ij) / J_m
 * (w_i the row scale, 0 on a replaced row), double-double throughout (csrc/mk_sens_multi.h;
 * assembly, LU and solve in csrc/mk_adjoint.h).
 * xi_num - xi_den is the control of the selectivity J_num / J_den; a coverage
 * objective gives d ln theta_i / d ln k_j.  Only val and xi: the per-direction
 * split, reaction orders and user directions of pck_sens_at are not offered per
 * objective, since rf_j s_mj / J_m of a coverage objective is not safe in
 * double-double and no guard is known (DESIGN.md "Multi-objective DRC").
 * status_in (optional) gates the conditions as in pck_drc_at.  status:
 * PCK_ST_SENS_SINGULAR for a zero pivot or a non-finite factor; such a condition and a
 * gated one get NaN in every xi, and that status in every ostatus.  ostatus[m]:
 * PCK_ST_NONFINITE for a zero or non-finite J_m (or an adjoint solve that overflows):
 * NaN xi[m][:] for that objective alone.  val is written for every condition.
 * The kernel is chosen by pck_network_set_multi_lanes (below), whatever
 * pck_network_set_sens_lanes says: by default the 16- / 32- / 64-lane group kernels;
 * pck_network_sens_lanes reports G afterwards, or 1 after a one-lane launch.  Sizes as
 * pck_drc_at (PCK_E_SIZE); PCK_E_ARG: K < 1, NULL obj / out / val / xi, wr and wy both
 * NULL, a leading dimension below n. */
int pck_drc_multi_at(const pck_network* net, const pck_conditions* cond, const double* kf, const double* kr,
                     int64_t ld_k, const double* y, int64_t ld_y, const int32_t* status_in,
                     const pck_multi_obj* obj, const pck_multi_out* out, void* stream);

/* One steady solve (pck_solve with prm->newton = 1, as pck_drc_adjoint) and then
 * pck_drc_multi_at at its states, with the solve's own rate constants (replaces
 * nothing in the reference).  nsteps (optional): the solve's steps.  A condition
 * whose solve did not report a reached root keeps that status and gets NaN xi (val:
 * the objectives at the state the solve reports).  PCK_E_ARG: prm->newton == 0, a
 * trajectory request, and what pck_drc_multi_at refuses. */
int pck_drc_multi_adjoint(const pck_network* net, const pck_conditions* cond, const pck_solve_params* prm,
                          const pck_multi_obj* obj, const pck_multi_out* out, int32_t* nsteps, void* stream);

/* Lanes per condition of the kernel behind pck_drc_multi_at and pck_drc_multi_adjoint,
 * a mode of its own beside pck_network_set_sens_lanes (neither changes what the other's
 * entry points run): PCK_SENS_LANES_GROUP (default: k_multi_adjoint<G>,
 * csrc/mk_sens_multi.h), PCK_SENS_LANES_ONE (one lane per condition,
 * csrc/mk_sens_multi_lane.h: the same formulas, statuses and outputs, every step serial
 * in its lane; networks of up to PCK_MAX_DYN_LANE dynamic species, else PCK_E_SIZE from
 * this call), PCK_SENS_LANES_AUTO (one lane up to PCK_MAX_DYN_LANE species, else the
 * group kernels).  Any other mode is PCK_E_ARG.  The two kinds agree to rounding, not
 * bitwise (sums over reactions and species run in another order); the argument checks
 * of the two entry points are the same in every mode. */
int pck_network_set_multi_lanes(pck_network* net, int mode);

/* Bed DRC (csrc/mk_cascade_adjoint.h): the degree of rate control of K objectives of a
 * reactor cascade of `cells` cells (pck_solve_cascade) at given cell states, by one
 * backward adjoint sweep through the cells in one launch, one lane per condition
 * (networks of up to PCK_MAX_DYN_LANE dynamic species).  pck_multi_obj is read for a bed as
 *   J_m = (1/cells) sum_c sum_j wr[m][j] net_j(y_c) + sum_i wy[m][i] y_{cells-1,i}:
 * wr weights the bed mean of the net rates (with the TOF terms: the tof of
 * pck_solve_cascade), wy the outlet state.  With F(y_c, u_c, k) = 0 the steady equations
 * of cell c as pck_drc_multi_at poses them (u_c its inflow: cond->inflow for c = 0, the
 * state of cell c-1 on the flow rows else), A_c = dF/dy, w_{c,i} the row scale and
 * phi_{c,i} the flow rate of row i, each 0 where row i of cell c was replaced,
 *   A_c^T mu_{m,c} = dJ_m/dy_c - phi_{c+1} (.) mu_{m,c+1}      c = cells-1 ... 0,  mu_{m,cells} = 0
 *   xi[m][j] = sum_c net_j(y_c) (wr[m][j] / cells - sum_i mu_{m,c,i} w_{c,i} S_ij) / J_m
 *   order_in[m][i] = -mu_{m,0,i} phi_{0,i} inflow_i / J_m      (d ln J_m / d ln inflow_i)
 * double-double throughout; for cells = 1 this is pck_drc_multi_at (one-lane kernel) term
 * for term.  y_cells [cells][NDYN][ld_yc] as pck_solve_cascade writes it; status_cells
 * [cells][ld_c] (optional): a condition is computed only if every cell is PCK_ST_OK, else
 * it keeps its bed status as pck_solve_cascade reports it (the first failing status in cell order,
 * else PCK_ST_NEWTON) and gets NaN in every xi and order_in and that status in every ostatus.  order_in [K * NDYN][ld_oi]
 * (optional), row m * NDYN + i.  pck_multi_out as for pck_drc_multi_at: val[m] = J_m for
 * every condition whose cell states are all finite, NaN otherwise; status
 * PCK_ST_SENS_SINGULAR for a zero pivot or a non-finite factor in any cell; ostatus[m]
 * PCK_ST_NONFINITE for a zero or non-finite J_m or an adjoint solve that overflows, which
 * fails that objective alone.  A condition's result does not depend on the batch.
 * PCK_E_SIZE: more than PCK_MAX_DYN_LANE dynamic species, or a network beyond the
 * lane-group records (as pck_drc_at).  PCK_E_ARG: cells outside 1..PCK_MAX_CELLS, a network
 * without a flow row, K < 1, NULL obj / out / val / xi, wr and wy both NULL, a leading
 * dimension below n.  n == 0 returns PCK_OK.
 * Device memory: the call allocates, on the stream and for its own length, a workspace of
 * 16 K (NDYN + NRXN + 2) n bytes (what a lane carries from cell to cell), whatever `cells`
 * is; PCK_E_HIP if that does not fit.  Results do not depend on the batch, so a large
 * batch may be split into calls. */
int pck_cascade_drc_at(const pck_network* net, const pck_conditions* cond, const double* kf, const double* kr,
                       int64_t ld_k, const double* y_cells, int64_t ld_yc, int32_t cells,
                       const int32_t* status_cells, int64_t ld_c, const pck_multi_obj* obj,
                       const pck_multi_out* out, double* order_in, int64_t ld_oi, void* stream);

/* pck_solve_cascade (prm->newton = 1 required; cas->start as given) and then
 * pck_cascade_drc_at at its cell states, with the solve's own rate constants.  cas: the
 * per-cell outputs are written as by pck_solve_cascade; y_cells and status_cells are
 * allocated per call where they are NULL.  nsteps (optional): the steps summed over the
 * cells.  A bed with a cell that did not report a reached root keeps that status and gets
 * NaN xi.  PCK_E_ARG: prm->newton == 0, and what pck_solve_cascade and pck_cascade_drc_at
 * refuse. */
int pck_cascade_drc(const pck_network* net, const pck_conditions* cond, const pck_solve_params* prm,
                    const pck_cascade* cas, const pck_multi_obj* obj, const pck_multi_out* out,
                    double* order_in, int64_t ld_oi, int32_t* nsteps, void* stream);

/* An energy landscape (energy.py:12 Energy.minima): n_pts entries along the
 * reaction coordinate, 4 <= n_pts <= PCK_MAX_PES, each the energy-program
 * register that holds its energy (eV).  Entry 0 is the reference every energy
 * is taken relative to, and entry n_pts-1 the end of the cycle (its energy is
 * the reaction energy); neither may be a transition state.  Passed from host
 * memory. */
typedef struct {
    int32_t n_pts;               /* N */
    int32_t reg[PCK_MAX_PES];    /* register (< NREG) of entry k */
    uint64_t ts_mask;            /* bit k set: entry k is a transition state */
} pck_landscape;

/* Outputs of pck_energy_span (device pointers; any may be NULL).  nTi = TS
 * entries, nIj-1 = intermediates among entries 1..N-2 (energy.py:250-255). */
typedef struct {
    double* tof;                 /* [n] turnover frequency (1/s); may underflow to 0 */
    double* espan;               /* [n] E(TDTS) - E(TDI) (eV) */
    double* eapp;                /* [n] apparent activation energy (kJ/mol, energy.py:300), from ln tof */
    double* dgrxn;               /* [n] energy of the last entry (eV) */
    int32_t* i_tdts;             /* [n] landscape index of the TOF-determining TS (-1: non-finite energy) */
    int32_t* i_tdi;              /* [n] ... of the TOF-determining intermediate */
    double* x_ts;                /* [nTi][ld_x] TS contributions (num_i), TS entries in landscape order */
    double* x_int;               /* [nIj-1][ld_x] intermediate contributions (num_j), likewise */
    int64_t ld_x;
    double* energy; int64_t ld_e;   /* [N][ld_e] landscape energies (eV) relative to entry 0 */
} pck_span_outputs;

/* Energy-span model of a landscape for every condition, one launch:
 * the energy program -> the N landscape energies -> TOF, energy span, the
 * TOF-determining states and every state's contribution
 * (Energy.construct_energy_landscape energy.py:39 +
 *  Energy.evaluate_energy_span_model energy.py:238).  The sums of exponentials
 * are carried as a shift plus a sum and the TOF in logs, so no energy makes
 * an output overflow; a condition with a non-finite energy gets NaN outputs
 * and indices -1.  Takes an energy-only network (NDYN = NRXN = 0) or any other.
 * PCK_E_ARG: N outside 4..PCK_MAX_PES, a register out of range, entry 0 or
 * N-1 a TS, no TS or no intermediate among entries 1..N-2. */
int pck_energy_span(const pck_network* net, const pck_conditions* cond, const pck_landscape* pes,
                    const pck_span_outputs* out, void* stream);

/* ---- uncertainty ensemble (pycatkin/classes/uncertainty.py) -------------------
 * An ensemble is n_rep blocks of B = n_runs + lead_zero consecutive conditions,
 * one block per base condition (a temperature, say): run r of block c is
 * condition c*B + lead_zero + r, so the runs of one base condition are
 * contiguous (the 64 lanes of a wavefront share a temperature).  With
 * lead_zero the first condition of each block is the unperturbed system (the
 * reference's noisy_sys[0]).
 *
 * pck_ensemble_noise writes the [1 + n_ts][ld_desc] descriptor matrix that
 * pck_conditions.desc reads (s_desc = 1) for the whole ensemble -- what
 * Uncertainty.get_correlated_state_noises (uncertainty.py:35-65) draws per run
 * with one np.random.normal and one np.random.uniform per transition state:
 *   row 0     mu + sigma * z_r     the white noise every adsorbate of run r shares
 *   row 1+k   row0 * u_{r,k}       transition state k < n_ts; u uniform in [0, 1),
 *                                  independent of mu and sigma (the reference's
 *                                  quirk, kept)
 * and exactly 0 in every row of a block's lead column.  Columns beyond
 * n_rep*B are not touched.  Every value is computed once per thread and
 * written to each replica c.
 *
 * Generator: Philox4x32-10 (Salmon et al., SC'11), counter-based.  Key =
 * (lo32(seed), hi32(seed)); counter = (lo32(run), hi32(run), j, 0) with
 * run = run_first + r.  A 53-bit uniform from output words (w0, w1) is
 * ((w0 * 2^32 + w1) >> 11) * 2^-53.  Block j = 0: (w0, w1) -> u1 taken as
 * (k + 1) * 2^-53 (never 0), (w2, w3) -> u2, and the Box-Muller normal
 * z = sqrt(-2 ln u1) * cos(2 pi u2) with 2 pi = 6.283185307179586.  Block
 * j >= 1: (w0, w1) -> u of transition state 2(j-1), (w2, w3) -> u of
 * 2(j-1)+1.  The noise of a run depends on (seed, run) alone -- not on n_runs,
 * n_rep or the launch geometry -- so an ensemble is reproducible and a shard
 * that starts at run_first draws the numbers the whole ensemble would.
 *
 * PCK_E_ARG: desc NULL, a negative size, lead_zero not 0 / 1,
 * ld_desc < n_rep * B. */
int pck_ensemble_noise(uint64_t seed, uint64_t run_first, int64_t n_runs, int64_t n_rep, int64_t n_ts,
                       int lead_zero, double mu, double sigma, double* desc, int64_t ld_desc, void* stream);

/* Outputs of pck_ensemble_stats (device pointers; any may be NULL), each
 * [n_rows][ld_out] with ld_out >= n_rep. */
typedef struct {
    int32_t* count;              /* accepted columns */
    double* mean;                /* NaN when count is 0 */
    double* std;                 /* population standard deviation (np.std, ddof 0); NaN when count is 0 */
    double* min;                 /* +inf when count is 0 */
    double* max;                 /* -inf when count is 0 */
    int64_t ld_out;
} pck_ens_stats;

/* Statistics over the runs of every base condition, for n_rows properties at
 * once -- the np.mean / np.std of Uncertainty.get_mean_property_value
 * (uncertainty.py:115-125).  For row q of v ([n_rows][ld_v]) and block c < n_rep
 * the columns c*block + skip .. c*block + block - 1 are reduced (skip = 1 leaves
 * out an ensemble's unperturbed lead column).  A column counts when its value
 * is finite and, with status ([n_rep*block] PCK_ST_* codes, may be NULL), bit
 * status[col] of ok_mask is set (a status outside 0..31 never counts).
 * Per-thread Welford updates, then Chan's pairwise merge of (n, mean, M2)
 * across the wavefront and across wavefronts, in an order fixed by `block`
 * alone: no atomics, no sum of squares, bitwise the same from launch to launch.
 * One workgroup per (row, block): 64 threads up to block = 256, 256 up to
 * 16384, 1024 beyond.  PCK_E_ARG: v or out NULL, a negative size,
 * ld_v < n_rep*block, ld_out < n_rep. */
int pck_ensemble_stats(const double* v, int64_t ld_v, int64_t n_rows, const int32_t* status, uint32_t ok_mask,
                       int64_t n_rep, int64_t block, int64_t skip, const pck_ens_stats* out, void* stream);

/* ---- linear stability: eigenvalues of steady Jacobians --------------------------
 * Outputs of pck_eigvals / pck_stability_at / pck_stability (device pointers, each
 * optional), per condition.  A condition whose status is not PCK_ST_OK gets NaN in
 * every double and -1 in n_pos. */
typedef struct {
    double* wr; double* wi; int64_t ld_w;   /* [ns_eff][ld_w] real / imaginary parts; a conjugate pair is
                                             *   adjacent, positive imaginary part first; the order is
                                             *   otherwise unspecified */
    double* re_max;              /* [n] spectral abscissa: the largest real part */
    double* im_max;              /* [n] |Im| of that eigenvalue (the largest among equal real parts) */
    double* re_min;              /* [n] the most negative real part */
    double* scale;               /* [n] ns_eff * eps * ||B||_F, B the scale-balanced matrix: the size of
                                  *   fp64 rounding in the eigenvalues (the backward error of Hessenberg QR
                                  *   on B), not a bound for ill-conditioned ones.  An eigenvalue smaller
                                  *   than scale is not resolved: its sign means nothing */
    int32_t* n_pos;              /* [n] eigenvalues with real part > re_tol */
    int32_t* status;             /* [n] PCK_ST_* */
} pck_eig_out;

/* Eigenvalues of n real ns x ns matrices in the layout pck_jacobian writes (entry
 * (i, k) of condition c at a[(i*ns + k)*ld + c]; never modified), fp64: balancing by
 * powers of two (scaling only), Householder reduction to Hessenberg form, Francis
 * double-shift QR (csrc/mk_eig.h).  Network-free.  Replaces the np.linalg.eigvals of
 * SteadyStateSolver.test_convergence (pycatkin/classes/solver.py:102-106) and of
 * solve_ode (solver.py:156-158) for a batch.
 * lanes: PCK_SENS_LANES_ONE (one lane per condition, ns <= PCK_MAX_DYN_LANE, else
 * PCK_E_SIZE), PCK_SENS_LANES_GROUP (16 / 32 / 64 lanes per condition),
 * PCK_SENS_LANES_AUTO (one lane up to PCK_MAX_DYN_LANE, else groups).  lanes_used
 * (optional, host): 1, 16, 32 or 64.  The result for a matrix does not depend on the
 * rest of the batch, bit for bit.
 * status_in (optional) gates the conditions as in pck_drc_at: a row that is not
 * PCK_ST_OK keeps its status.  PCK_ST_NONFINITE: a non-finite entry (or eigenvalue);
 * PCK_ST_EIG_NOCONV: the sweep budget is spent.
 * PCK_E_ARG: ns < 1, ld (or ld_w with wr / wi) below n, NULL a / out, an unknown
 * mode; PCK_E_SIZE: ns > PCK_MAX_DYN.  n = 0 is a no-op. */
int pck_eigvals(const double* a, int ns, int64_t n, int64_t ld, const int32_t* status_in, double re_tol,
                int lanes, const pck_eig_out* out, int32_t* lanes_used, void* stream);

/* Linear stability at given states y ([NS][ld_y]), kf / kr as pck_rate_constants
 * gives them: pck_jacobian into stream-ordered scratch, then the kernel of
 * pck_eigvals -- the Jacobian never leaves the device (solver.py:102-106, :156-158
 * copy it to the host for np.linalg.eigvals).
 * reduce = 0: the full Jacobian, ns_eff = NS (the reference's test; with a
 * conservation law it has a structurally zero eigenvalue that fp64 returns as
 * +- scale).  reduce = 1: the Jacobian restricted to the conservation class,
 * ns_eff = NS - NCONS: with the laws C in reduced row-echelon form and pivots p_l,
 *   Jr[i][q] = J[i][q] - sum_l J[i][p_l] C[l][q] / C[l][p_l]   (i, q not pivots),
 * whose spectrum has no structural zero (NCONS = 0: the same matrix).
 * PCK_E_ARG also for reduce outside 0 / 1, NS - NCONS < 1, bad kf / kr / y. */
int pck_stability_at(const pck_network* net, const pck_conditions* cond, const double* kf, const double* kr,
                     int64_t ld_k, const double* y, int64_t ld_y, const int32_t* status_in, int reduce,
                     double re_tol, int lanes, const pck_eig_out* out, int32_t* lanes_used, void* stream);

/* One steady solve (pck_solve with prm->newton = 1, as pck_drc_adjoint) and then
 * pck_stability_at at its states, with the solve's own rate constants.  nsteps
 * (optional): the solve's steps.  A condition without a reached root keeps that
 * status and gets NaN outputs.  PCK_E_ARG: prm->newton == 0, a trajectory request. */
int pck_stability(const pck_network* net, const pck_conditions* cond, const pck_solve_params* prm, int reduce,
                  double re_tol, int lanes, const pck_eig_out* out, int32_t* lanes_used, int32_t* nsteps,
                  void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PYCATKIN_AMD_H */
