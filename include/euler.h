/*
 * euler.h — C ABI of libeuler_hip.so: the MI355X-native replacement for the simulation path of
 * cgmb/euler (reference main.c: sim_init :209, sim_step :843, draw :953 and the file-scope
 * arrays g_u/g_v/g_marker_count/... :64-100 they communicate through).
 *
 * Plain C, plain pointers and sizes; no HIP or torch types.  Host code (the `euler` CLI, the
 * reference's own main loop, bench.py, pytest via ctypes) sees only this file.
 *
 * Every function returns EULER_OK (0) or a negative EULER_E* code and never calls exit()
 * (reference behaviour replaced: main.c:212-215 fprintf+exit(1)).  euler_last_error() returns
 * a thread-local human-readable message for the last failure.
 *
 * A handle is single-caller (not re-entrant), like the reference's globals.
 */
#ifndef EULER_H
#define EULER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EULER_ABI_VERSION 2   /* 2: euler_comm_ops.exchange, row-slab snapshots */

enum {
  EULER_OK = 0,
  EULER_EINVAL = -1,     /* bad argument */
  EULER_ENOMEM = -2,     /* host or device allocation failed */
  EULER_EIO = -3,        /* scenario file unreadable (reference: "Could not load %s!", main.c:213) */
  EULER_EHIP = -4,       /* a HIP runtime call failed / no gfx950 device */
  EULER_ESTATE = -5,     /* call order violated (e.g. step before a scenario is loaded) */
  EULER_ETIMEOUT = -6,   /* an in-kernel bounded wait expired (band pipeline) */
  EULER_ECOMM = -7       /* multi-GPU communicator failure */
};

/* How dot(a,b) (reference main.c:629-639, a sequential row-major double sum) is evaluated. */
enum {
  EULER_DOT_AUTO = 0,        /* SEQUENTIAL when X*Y <= 65536, else TREE */
  EULER_DOT_SEQUENTIAL = 1,  /* one thread adds in the reference's order: bit-identical results */
  EULER_DOT_TREE = 2         /* fixed-shape parallel reduction: deterministic, differs in the last ulps */
};

/* Preconditioner of the pressure solve. */
enum {
  EULER_PRECOND_IC0 = 0,     /* the reference's incomplete Cholesky (main.c:580-627), evaluated as a
                                dependency-ordered wavefront: bit-identical to the sequential sweep */
  EULER_PRECOND_JACOBI = 1,  /* z = r/diag: NOT the reference's iterates; for roofline comparison only */
  EULER_PRECOND_IC0_TILE = 2, /* tile-local IC(0) (SURVEY 7 hard part 1(b): "tile-local IC(0) = block-Jacobi-IC"): the reference's
                                three recurrences (main.c:586-626) restricted to blocks - a block = the cells of one 64-row band
                                whose skew records t = x + y % 64 fall into one tile of euler_config.precond_tile_records records
                                (a parallelogram of 64 rows x W columns); couplings between blocks are dropped from the factor and
                                from both triangular solves.  A block lives in the registers of one wave, so r -= alpha A s,
                                max |r|, both solves and dot(z,r) are ONE pass over memory (k_precond_tile), bandwidth-bound
                                instead of latency-bound, and nothing couples row slabs.  NOT the reference's iterates: the same
                                solution where PCG converges (tolerance parity), ~25-35 % more iterations (tools/precond_study.py).
                                Restated in the oracle (eo_sim.tile_records): GPU = oracle bit for bit in EULER_DOT_SEQUENTIAL. */
  EULER_PRECOND_IC0_TILE2 = 3,/* TWO-LEVEL (round 3): the tile-local IC(0) above (64 x 16 blocks) plus a coarse correction,
                                    z = M_tile^-1 r + P (P^T A P)^-1 P^T r,
                                P = piecewise constants over coarse cells of (64 m)^2 grid cells restricted to the fluid, m the smallest
                                power of two that leaves at most 256 coarse cells (16 x 16 of them on a square grid).  The block-local
                                factor has no coupling beyond a block; the coarse space restores the long-range part of the inverse, which is
                                what the first hundred iterations of a large solve live on: 2-4x fewer iterations than the REFERENCE's IC(0)
                                to the reference's tolerance (2048^2 tank: 402 vs 1726), the reference's residual-after-100 in ~44 iterations
                                on the saturated 8192^2 tank (docs/solver_two_level.md).  Same traffic
                                per iteration as the tile-local mode (the coarse part is 3 doubles per tile out, one double per coarse cell
                                in) + one small launch.  NOT the reference's iterates; symmetric positive definite, so PCG converges to the same
                                solution.  Restated in the oracle (eo_sim.coarse_m): GPU = oracle to rounding (tolerance, not bits: the
                                coarse sums are formed in another order).  One GPU only; EULER_DOT_TREE. */
  EULER_PRECOND_IC0_TILE_MG = 4 /* MULTILEVEL (round 3; round 5: bilinear node grids): the same, with the coarse correction taken from a hierarchy instead of one level,
                                    z = M_tile^-1 r + P_0 V(P_0^T r),
                                level 0 = a grid of nodes 8 cells apart (node (I, J) at the centre of cell (8 J + 4, 8 I + 4)), P_0 = bilinear interpolation from the four nodes
                                around a cell, restricted to the fluid; every further level = every other node of the one below, bilinear again (full weighting); Galerkin
                                operators (exact nine-point stencils), one symmetric V-cycle (damped Jacobi before and after: 0.8, per node less where a Gershgorin bound of 1.6
                                demands it - spray drops), the top level (<= 64 nodes) solved
                                with the dense pseudo-inverse of the two-level mode.  The number of iterations to the reference's tolerance does not grow with the grid:
                                ~30 on a tank at rest at any size, 40-50 on moving water, where the reference's IC(0) needs 231 (256^2), 880 (1024^2), thousands (8192^2)
                                and rounds 3-4's piecewise-constant aggregates of 16 cells needed 105-150.  Cost per iteration: the tile-local mode's two passes (+ 72
                                doubles of partial sums per 1024-cell tile) + five launches over node grids 1/64 the size of the grid and less.  Restated in the oracle
                                (eo_sim.coarse_mg): GPU = oracle to rounding.  EULER_DOT_TREE.  One GPU, or row slabs without mailboxes (euler_config.slab_*).  On slabs the cycle is SPLIT BY ROWS
                                wherever a level of <= 16384 nodes lies above level 0 and the slabs are a few bands thick (docs/solver_multilevel.md; EULER_OPT_MG_SPLIT_LEVEL): a rank takes
                                its own tiles' share down to that level, windows of it are all-gathered inside the G1 exchange (0.16 MB per iteration at 16384^2 on 8 ranks), the
                                neighbours' shares on a rank's halo rows travel with the edge rows of z, the coarse levels run replicated, the fine levels on the own node rows, and
                                one more 40-byte exchange sums the correction's share of dot(z, r); per solve the operators are formed by their owners.  Otherwise (small grids,
                                thin slabs, EULER_OPT_MG_SPLIT_LEVEL = -1) the cycle runs replicated: one all-reduce per solve makes the level-0 operator whole, every rank
                                contributes its node rows to the G1 all-gather (cells / 64 doubles over all ranks: 32 MB at 16384^2).  Either way every rank computes the same bits.  Water cut off from the air (a singular
                                system): the right-hand side is made compatible with the region's indicator, and the correction is kept mean-free over the region so that
                                the pressure's constant - which the reference's clamp p >= 0 makes observable - is the tile-local factor's, i.e. very nearly the reference's. */
};

/* IC(0) sweep implementation (same arithmetic, different schedule). */
enum {
  EULER_SWEEP_AUTO = 0,
  EULER_SWEEP_BAND = 1,      /* one wave per 64-row band streaming band-skewed records, bands pipelined
                                through tagged granules (DESIGN.md "IC(0) sweeps") */
  EULER_SWEEP_SIMPLE = 2     /* one workgroup, one barrier per anti-diagonal (debug / cross-check) */
};

typedef struct euler_config {
  int32_t abi_version;     /* EULER_ABI_VERSION */
  int32_t X, Y;            /* grid size; reference: compile-time enum X=100, Y=40 (main.c:22-25) */
  int32_t device;          /* HIP device ordinal */
  int32_t max_iterations;  /* PCG cap, reference 100 (main.c:735) */
  double  tol;             /* inf-norm tolerance, reference (double)1e-6f (main.c:736) */
  int32_t dot_mode;        /* EULER_DOT_* */
  int32_t precond;         /* EULER_PRECOND_* */
  int32_t sweep_mode;      /* EULER_SWEEP_* */
  int32_t max_substeps;    /* reference 8 (main.c:851) */
  float   frame_time;      /* reference 0.1f (main.c:849) */
  float   viscosity;       /* 0 = inviscid like the reference (no diffusion stage exists there) */
  int32_t pcg_poll_interval; /* PCG iterations launched between convergence polls (default 8) */
  int32_t rainbow;         /* args_t.rainbow / g_rainbow_enabled (main.c:54,75,1020): carry the dye fields */
  int32_t precond_tile_records; /* EULER_PRECOND_IC0_TILE: records per tile, 8, 16 or 32 (0 = default 16); tile k of a band =
                                   records [k * W, (k + 1) * W) */
  int32_t slab_rank, slab_nranks; /* slab_nranks >= 1 (0 = off): ROW SLABS FOR EVERY STAGE.  This handle is rank slab_rank of a job of
                                   slab_nranks processes, one per GPU; it owns the rows of its 64-row bands (euler_slab_info) and
                                   allocates ONLY those rows (+ 1 ghost row below, 2 above) of every grid and only the markers inside
                                   them - per-rank memory ~ 1/slab_nranks.  Install a communicator of the same rank / size
                                   (euler_set_comm / euler_set_comm_rccl) BEFORE loading a scenario.  Fields are then exchanged as the
                                   owned rows (euler_get_field), markers as the local ones with their global array index
                                   (EULER_F_MARKER_KEYS); euler_set_field(U / V) takes the own rows and is COLLECTIVE (it refreshes the
                                   neighbours' ghost rows).  Needs EULER_PRECOND_IC0_TILE or slab-local IC(0) coupling. */
  int32_t slab_band_lo, slab_band_hi; /* row slabs: this rank's 64-row bands [lo, hi) given explicitly (hi > lo) instead of the even split
                                   nbands * rank / nranks - for partitions that balance the FLUID (a dam break settles into the
                                   lowest third of the tank: even row slabs leave most ranks with air).  The ranks' ranges must tile
                                   [0, nbands) in rank order; euler_set_comm* checks it against the neighbours.  0, 0 = even split. */
  int32_t pcg_precision;   /* EULER_PCG_F64 (0, default: the reference's double vectors, main.c:577-578,716) or EULER_PCG_F32: every solver vector in float, sums and
                              scalars in double - BASELINE configs[1]'s "fp32".  NOT the reference's iterates (tolerance parity only, restated in the oracle:
                              eo_sim.pcg_f32); runs in the resident solver, so it needs what that needs (below) and euler_create refuses it otherwise. */
  int32_t resident;        /* EULER_RESIDENT_AUTO (0): a solve whose ACTIVE 16-record chunks (those holding fluid) all find a wave on the chip at once - at most
                              4 x (resident workgroups): 2048 chunks = 2 M cells of water in double, 3072 in float on an MI355X; BASELINE configs[1] (1024^2 dam break)
                              always, configs[4] (4096^2 waterfall) while its water is below that - runs the tile-local PCG (EULER_PRECOND_IC0_TILE, one GPU, EULER_DOT_TREE,
                              tiles of 16 records) as ONE persistent launch whose vectors stay in registers (csrc/k_resident.hip): same arithmetic, sums folded per
                              workgroup, so the iterates agree with the multi-kernel form to rounding; decided per solve.  EULER_RESIDENT_OFF (1): always the
                              multi-kernel form. */
} euler_config;

enum { EULER_PCG_F64 = 0, EULER_PCG_F32 = 1 };
enum { EULER_RESIDENT_AUTO = 0, EULER_RESIDENT_OFF = 1 };

typedef struct euler_sim euler_sim; /* opaque */

/* Arrays readable/writable through euler_get_field/euler_set_field.  All grids are row-major
 * [Y][X], full size even for the staggered U/V samples (main.c:62-67). */
enum {
  EULER_F_U = 0,          /* float  g_u     main.c:64 */
  EULER_F_V,              /* float  g_v     main.c:65 */
  EULER_F_UTMP,           /* float  g_utmp  main.c:66 */
  EULER_F_VTMP,           /* float  g_vtmp  main.c:67 */
  EULER_F_SOLID,          /* uint8  g_solid main.c:71 */
  EULER_F_SOURCE,         /* uint8  g_source main.c:72 */
  EULER_F_SINK,           /* uint8  g_sink  main.c:73 */
  EULER_F_COUNT,          /* uint8  g_marker_count main.c:96 */
  EULER_F_PREV_COUNT,     /* uint8  g_prev_marker_count main.c:97 */
  EULER_F_MARKERS,        /* float2[n_markers] g_markers main.c:95, in the reference's array order */
  EULER_F_PRECON,         /* double g_precon main.c:577 (persistent state) */
  EULER_F_PRESSURE,       /* double p — a stack local of project(), main.c:739; exposed here.  Whole-grid handles form the finished, clamped pressure in device memory only when
                             it is asked for (the velocity update keeps it in LDS): the call costs one pass over the solver arrays the first time after a substep */
  EULER_F_PCG_B, EULER_F_PCG_R, EULER_F_PCG_Z, EULER_F_PCG_S, EULER_F_PCG_Q, /* double, main.c:716-745,578.  Test surface: after a solve S is the search
                                                              direction of the last iteration that ran (+0 off the fluid and when the right-hand side was
                                                              all zero); Q holds A s only where a solve stores it (docs/solver_tile_local.md: most do not any more).
                                                              After a solve that ran in the resident kernel (euler_resident_info) Z, S and Q do not exist in
                                                              memory: euler_get_field returns EULER_ESTATE for them until a multi-kernel solve has run */
  EULER_F_CELLMASK,       /* uint8: bit0 fluid, bit1..4 fluid at x+1,y+1,x-1,y-1, bits5-7 a_diag (g_a, main.c:552) */
  EULER_F_DYE_R, EULER_F_DYE_G, EULER_F_DYE_B,             /* float g_r, g_g, g_b (main.c:76-78); euler_config.rainbow only */
  EULER_F_DYE_RTMP, EULER_F_DYE_GTMP, EULER_F_DYE_BTMP,    /* float g_rtmp, g_gtmp, g_btmp (main.c:79-81): state, because the
                                                              reference copies them back whole (main.c:875-881) */
  EULER_F_MARKER_KEYS,    /* uint32[n local markers]: row-slab handles only - the position of each local marker in the reference's
                             g_markers array (EULER_F_MARKERS of all ranks, ordered by key, IS that array) */
  EULER_F__COUNT
};

/* Stages of one substep, in the reference's order (main.c:855-893).  Fused stages are listed
 * as the reference stages they cover; the arrays they leave behind equal the reference's after
 * the LAST covered stage. */
enum {
  EULER_STAGE_ADVECT_MARKERS = 0,   /* advect_markers            main.c:464-537 */
  EULER_STAGE_REFRESH_COUNTS,       /* refresh_marker_counts     main.c:102-117 */
  EULER_STAGE_SOURCES,              /* update_fluid_sources      main.c:276-298 */
  EULER_STAGE_EXTRAPOLATE,          /* extrapolate(U), extrapolate(V), zero_bounds(U), zero_bounds(V)  main.c:865-868 */
  EULER_STAGE_ADVECT_VELOCITY,      /* advect_u, advect_v, apply_body_forces, zero_bounds x2          main.c:871-889 */
  EULER_STAGE_PROJECT,              /* project                   main.c:709-806 */
  EULER_STAGE__COUNT
};

/* Single PCG building blocks on the handle's device vectors (kernel-level parity tests and
 * micro-benchmarks).  Operands are the EULER_F_PCG_* arrays. */
enum {
  EULER_OP_BUILD_SYSTEM = 0, /* b, r=b, p=0, cell mask from UTMP/VTMP and dt      main.c:713-741 */
  EULER_OP_PRECON_FACTOR,    /* E^-1 into PRECON                                  main.c:586-600 */
  EULER_OP_FORWARD_SOLVE,    /* Q = L^-1 R                                        main.c:602-613 */
  EULER_OP_BACKWARD_SOLVE,   /* Z = L^-T Q                                        main.c:615-626 */
  EULER_OP_APPLY_A,          /* Z = A S                                           main.c:679-691 */
  EULER_OP_DOT_ZR,           /* scalar <- dot(Z,R)                                main.c:629-639 */
  EULER_OP_DOT_ZS,           /* scalar <- dot(Z,S) */
  EULER_OP_INF_NORM_R,       /* scalar <- max |R|                                 main.c:654-667 */
  EULER_OP_UPDATE_PR,        /* P += a S; R -= a Z (a = scalar argument)          main.c:753-754 */
  EULER_OP_UPDATE_SEARCH,    /* S = Z + a S                                       main.c:669-677 */
  EULER_OP__COUNT
};

typedef struct euler_stats {
  uint64_t frames;              /* euler_step calls completed */
  uint64_t total_substeps;
  uint64_t total_pcg_iterations;
  int32_t  last_substeps;       /* substeps of the last frame (1..8) */
  int32_t  last_pcg_iterations; /* PCG iterations summed over the last frame */
  double   last_residual;       /* inf-norm of r when the last solve stopped */
  float    last_dt;             /* dt of the last substep */
  uint64_t n_markers;
  int32_t  source_exhausted;    /* g_source_exhausted, main.c:94 */
  uint64_t rng_state;           /* xorshift64* state (function-static in the reference, main.c:204) */
  uint64_t marker_dt_events;    /* collisions that shortened dt for later markers (main.c:501,518) */
  uint64_t marker_multi_events; /* markers with more than one such collision (expected 0 under the CFL bound) */
  uint64_t fluid_cells;
} euler_stats;

/* ---- life cycle ------------------------------------------------------------------------- */
int  euler_config_default(euler_config* cfg);              /* reference constants, X=100, Y=40 */
int  euler_create(const euler_config* cfg, euler_sim** out);   /* allocates HBM; needs a gfx950 GPU */
void euler_destroy(euler_sim* sim);
const char* euler_last_error(void);
int  euler_abi_version(void);
int  euler_resident_info(euler_sim* sim, uint64_t out[3]); /* {this handle's solves may use the resident solver (euler_config.resident), solves it ran, solves that fell back to the multi-kernel path} */

/* ---- scenario = sim_init (main.c:209-274) ----------------------------------------------- */
/* upscale = 0: the reference's streaming parser at native resolution.
 * upscale = 1: nearest-neighbour resample of the text onto the interior (this build's extension;
 *              DESIGN.md "Scenario upscaling"). */
int euler_load_scenario_mem(euler_sim* sim, const char* text, int32_t len, int32_t upscale);
int euler_load_scenario_file(euler_sim* sim, const char* path, int32_t upscale);
int euler_load_half_tank(euler_sim* sim);   /* synthetic config 3: solid ring, fluid in y < Y/2, at rest */
/* `tanks` such tanks on top of each other, each closed (solid where two meet): tank k is the single tank of an X x (Y / tanks) grid
 * in rows [k Y / tanks, (k+1) Y / tanks).  The weak-scaling workload: one tank per row slab.  tanks = 1 is euler_load_half_tank. */
int euler_load_half_tanks(euler_sim* sim, int32_t tanks);

/* Host-only pieces of sim_init, usable without a GPU (parser / marker seeding parity tests).
 * Outputs are caller-owned; solid/source/sink/fluid are [Y][X] uint8, markers float2[4*X*Y]. */
int euler_parse_scenario(const char* text, int32_t len, int32_t X, int32_t Y, int32_t upscale,
                         uint8_t* solid, uint8_t* source, uint8_t* sink, uint8_t* fluid);
int euler_seed_markers(const uint8_t* fluid, int32_t X, int32_t Y, uint64_t* rng_state,
                       float* markers_xy, uint64_t* n_markers);

/* ---- stepping = sim_step (main.c:843-900) ------------------------------------------------ */
int euler_step(euler_sim* sim);                    /* one frame: <= max_substeps CFL substeps */
int euler_timestep(euler_sim* sim, float frame_time_left, float* dt);   /* calculate_timestep, main.c:834-841 */
int euler_substep(euler_sim* sim, float dt);       /* stages 2..11 of sim_step with a given dt */
int euler_stage(euler_sim* sim, int32_t stage, float dt);   /* one EULER_STAGE_* (teacher-forced tests).  Row-slab handles: COLLECTIVE - the stage over the own rows with the
                                                                exchanges that belong to it (stages 0 .. 5 with one dt are a substep); not with euler_config.rainbow */
int euler_pcg_op(euler_sim* sim, int32_t op, float dt, double scalar_in, double* scalar_out);   /* one EULER_OP_* (kernel-level parity tests);
 * EULER_EINVAL for the preconditioner operations of a handle in EULER_PRECOND_IC0_TILE2 (its coarse level exists inside a solve only) */
/* Switch the preconditioner of the following solves (EULER_PRECOND_*; tile_records as euler_config.precond_tile_records,
 * 0 = default).  The solver's arrays do not depend on it; g_precon keeps whatever the last factorisation left. */
int euler_set_precond(euler_sim* sim, int32_t precond, int32_t tile_records);
/* The iteration budget and tolerance of the following solves (euler_config.max_iterations / tol; reference: 100 and 1e-6f,
 * main.c:735-736).  max_iterations <= 0 or tol < 0 leave the respective value as it is. */
int euler_set_solver(euler_sim* sim, int32_t max_iterations, double tol);

/* ---- state access ------------------------------------------------------------------------ */
int euler_get_field(euler_sim* sim, int32_t field, void* dst, size_t dst_bytes);
int euler_set_field(euler_sim* sim, int32_t field, const void* src, size_t src_bytes);
int euler_set_markers(euler_sim* sim, const float* xy, uint64_t n);
int euler_set_rng(euler_sim* sim, uint64_t rng_state, int32_t source_exhausted);
int euler_get_stats(euler_sim* sim, euler_stats* out);

/* ---- state snapshots: checkpoint / resume --------------------------------
 * Everything the reference keeps in file-scope variables (main.c:64-100, 204, 577), so that a resumed
 * run continues bit for bit.  File layout, little-endian:
 *   char[8] "EULERSNP"; u32 version = 1; i32 X, Y; u32 0; u64 n_markers; u64 rng_state;
 *   i32 source_exhausted; i32 0; u64 frames, total_substeps, total_pcg_iterations;          (72 bytes)
 *   f32[Y][X] u, v, utmp, vtmp;  u8[Y][X] solid, source, sink, count, prev_count;  f64[Y][X] precon;
 *   [version = 2, handles created with euler_config.rainbow: f32[Y][X] g_r, g_g, g_b, g_rtmp, g_gtmp, g_btmp;]
 *   f32[n_markers][2] markers in array order;  u64 FNV-1a-64 of all preceding bytes.
 * euler_load_state needs a handle of the same X, Y.  (euler_amd.read_snapshot / write_snapshot mirror
 * the format in numpy.)
 * ROW SLABS (version 3): every rank of a job calls euler_save_state with the SAME path and writes its own part file
 * "<path>.<rank>of<nranks>": the 72-byte header above with version = 3, then i32 nranks, rank, band_lo, band_hi, row_lo, row_hi,
 * u64 n_local_markers; the arrays above restricted to the rank's OWN rows [row_lo, row_hi); f32[n_local][2] markers,
 * u32[n_local] their keys (positions in the reference's g_markers); FNV-1a-64.  (Handles created with euler_config.rainbow: the
 * header's reserved word is 1 and the six dye arrays follow precon, as in version 2.)  Rank 0 also writes the manifest at <path>:
 * char[8] "EULERMAN"; u32 3; i32 X, Y, nranks; nranks x {i32 band_lo, band_hi}.
 * euler_load_state is independent of how a state was written: a whole-grid handle or a slab of ANY partition loads from a single
 * file or from a manifest, taking its rows (ghost rows included) and the markers inside its rows from the parts that hold them.
 * Resuming a 3-rank job on 2 ranks, on one GPU, or on a re-balanced partition is save + load.  On a row-slab handle the call is
 * collective (communicator installed first, like euler_load_scenario_*). */
int euler_save_state(euler_sim* sim, const char* path);
int euler_load_state(euler_sim* sim, const char* path);
/* ---- session files: checkpoints that carry the clock, the forcing, heat, tracers, bodies and the density control (docs/session.md) ----
 * A snapshot above is the reference's state.  A SESSION is everything a whole-grid handle holds that the next substep depends on: loading one puts the handle into
 * the saving handle's state, whatever it held before, and the continued run equals the uninterrupted one bit for bit - fields, markers in order, RNG, clock,
 * temperature, tracer records, body origins, reseed totals, frame counters.  File layout, little-endian: the 72-byte header above with version = 4, bit 0 of the
 * word behind Y set where the six dye arrays are present; the arrays of version 1 (with the bit: of version 2) in their order; the markers; then CHUNKS, each
 *   char tag[4]; u32 chunk_version = 1; u64 payload_bytes; the payload, padded with zeros to a multiple of 8 bytes
 * - all of them, always, in this order, with an "off" record where a feature is off:
 *   "TIME"  f64 the clock (euler_get_time)
 *   "FORC"  euler_forcing; nboxes x euler_force_box.  A handle that never called euler_set_forcing holds the default record (euler_forcing_default): what a substep
 *           launches is a function of the record's VALUES alone (the forced kernels run iff the uniform part differs from (0, -10) or shakes, the box pass iff
 *           nboxes > 0), so "never set" and "set to the default" are one state and a restored handle launches what the saver launched
 *   "HEAT"  i32 on, i32 0; euler_heat; nboxes x euler_heat_box; with on: f32[Y][X] the field as euler_heat_get_field returns it (off: the default record, no boxes)
 *   "TRAC"  u64 n; n x euler_tracer, verbatim, retired ones included
 *   "BODY"  i32 n, i32 0; n x euler_body; n x {i32 ox, oy}, the remembered origins
 *   "RSED"  euler_reseed; euler_reseed_stats
 *   "SETT"  the settings that can change a bit of the run (the table in docs/session.md; 320 bytes)
 *   "STAT"  i32 last_substeps, last_pcg_iterations; f64 last_residual; f32 last_dt; u32 0; u64 marker_dt_events, marker_multi_events: what euler_get_stats reports
 *           beside the header's counters and the marker state, so that the first line a resumed run logs is the one the saving run logged
 *   "END\0" empty
 * and the u64 FNV-1a-64 of all preceding bytes.  Written under "<path>.tmp" and renamed, like the other files.
 * euler_load_session reads and checks the WHOLE file before the handle changes - the checksum, X, Y, the dye bit, the marker capacity, the chunks' order and their
 * sizes against the counts inside them (an unknown tag or chunk version is named), every record through the check of its euler_set_* call, the heat field's values,
 * the tracers (a finite position, or flagged LOST; reserved 0), every cell of every body's rectangle at its remembered origin solid in the file's own solid grid,
 * and SETT against the handle's own settings: the settings are CHECKED, not applied.  A refused load leaves the handle exactly as it was.  Then the core is restored
 * as euler_load_state restores it, and the rest without the side effects of switching it on: no SOLID edit and no marker is deleted for a body, the reseed totals
 * are the file's, the file's ambient replaces the handle's, cells without markers hold it (as behind euler_heat_set_field), and a feature that is off in the file is
 * off afterwards.  Not carried: the pressure (each solve starts from 0; no snapshot ever held it).
 * Refusals: a null sim or path, a flag bit other than EULER_SESSION_IGNORE_SETTINGS (EULER_EINVAL); a row-slab handle (EULER_ESTATE, "slab"); euler_save_session
 * with nothing loaded (EULER_ESTATE); a file that cannot be opened, is truncated or fails its checksum (EULER_EIO); a settings mismatch (EULER_ESTATE, naming the first
 * field that differs with both values; EULER_SESSION_IGNORE_SETTINGS skips this comparison and nothing else); everything else about the file EULER_EINVAL.
 * euler_load_state accepts a version-4 file too: it verifies the checksum, takes the core and ignores the chunks - on a row-slab handle of any partition as well. */
enum { EULER_SESSION_IGNORE_SETTINGS = 1 };
int euler_save_session(euler_sim* sim, const char* path);
int euler_load_session(euler_sim* sim, const char* path, uint32_t flags);
size_t euler_field_bytes(const euler_sim* sim, int32_t field);   /* current size in bytes */

/* ---- render = draw_rows (main.c:914-951) ------------------------------------------------- */
/* Fetches only the visible window of the count grid from HBM.  Writes at most cap bytes into out
 * and stores the full length in *len (call with cap=0 to size the buffer).  On a row-slab handle the call is COLLECTIVE: the
 * visible rows are gathered from the ranks that own them and every rank returns the same frame. */
int euler_render(euler_sim* sim, int32_t wx, int32_t wy, char* out, int32_t cap, int32_t* len);
/* The same formatter over caller-supplied host grids (no GPU needed). */
int euler_render_grids(const uint8_t* solid, const uint8_t* sink, const uint8_t* count,
                       int32_t X, int32_t Y, int32_t wx, int32_t wy, char* out, int32_t cap, int32_t* len);
/* --rainbow: every water glyph carries a 24-bit colour escape built from the dye (main.c:902-912, 936-937;
 * misc/color.h:6-14).  euler_render uses it when the handle was created with euler_config.rainbow. */
int euler_render_grids_rgb(const uint8_t* solid, const uint8_t* sink, const uint8_t* count,
                           const float* r, const float* g, const float* b,
                           int32_t X, int32_t Y, int32_t wx, int32_t wy, char* out, int32_t cap, int32_t* len);
/* colorize() (main.c:187-201), the reference's 'r' key (main.c:970-973): recolour the current fluid. */
int euler_colorize(euler_sim* sim);

/* ---- whole-domain overview (docs/overview.md) ---------------------------------------------- */
/* euler_render shows one glyph per CELL: at 4096^2 a 98 x 38 corner under the ceiling.  The overview reduces the whole interior
 * ON THE DEVICE to a W x H raster of boxes of cells; only the W * H records cross to the host.  Everything in a record is an
 * integer sum or a maximum of non-negative floats, so the result does not depend on the order of the reduction (tests compare bits). */
typedef struct euler_overview_px {   /* one output pixel = one box of interior cells; 48 bytes */
  uint32_t cells;       /* cells in the box */
  uint32_t solid;       /* cells with solid != 0 */
  uint32_t sink;        /* cells with solid == 0 && sink != 0 */
  uint32_t water;       /* cells with solid == 0 && sink == 0 && count > 0 */
  uint32_t marks;       /* sum over the water cells of min(count, 3): the reference's glyph index (draw_rows) */
  float    max_speed2;  /* max over the water cells of dx*dx + dy*dy, dx = (u[i] + u[i-1]) / 2, dy = (v[i] + v[i-X]) / 2
                           (the cell-centre velocity k_advect_dye starts from); 0 without water; a NaN term is skipped */
  uint64_t dye[3];      /* sum over the water cells of q(r), q(g), q(b), q(x) = (uint32_t)(clamp(x, 0, 1) * 16777216.f) and q(NaN) = 0;
                           0 on handles without euler_config.rainbow */
} euler_overview_px;
/* The boxes: only the interior is shown, Xi = X - 2 columns and Yi = Y - 2 rows; 1 <= W <= Xi and 1 <= H <= Yi (else EULER_EINVAL), so no box
 * is empty.  Pixel column px covers the cells x = 1 + floor(px * Xi / W) ... floor((px + 1) * Xi / W); pixel row py = 0 is the TOP of the
 * picture: row py covers y = Y - 2 - floor(py * Yi / H) down to y = Y - 1 - floor((py + 1) * Yi / H).  out holds W * H records, row py at
 * out + py * W; out_bytes must be exactly W * H * sizeof(euler_overview_px).  One launch on the handle's stream that only READS the state
 * (the arrays euler_get_field returns for U, V, COUNT, SOLID, SINK, DYE_*): stepping afterwards gives the bits of a run that never called it.
 * The device buffer of the records comes with the first call and grows with W * H (EULER_ENOMEM: the handle unchanged).  A handle
 * without a loaded state: EULER_ESTATE.  On a row-slab handle the call is COLLECTIVE, as euler_render is: it needs the communicator (else EULER_ESTATE), every rank
 * calls with the same arguments and every rank gets the same bytes - those of a whole-grid handle holding the same state (each rank reduces its own rows, the
 * integer records are gathered and folded on the device: docs/observer_passes.md "On row slabs").  So are euler_render_fit and euler_overview_box. */
int euler_overview(euler_sim* sim, int32_t W, int32_t H, euler_overview_px* out, size_t out_bytes);
/* Host formatters over such records (no GPU needed).  The class of a pixel, in this order: 2 * solid >= cells: solid ('X'); else, with
 * open = cells - solid - sink: sink > 0 && sink >= open: sink ('='); else k = min(3, (marks + open - 1) / open) is the glyph index of
 * draw_rows (rounded up: a thin sheet still shows as 'o'; 0 is air).
 * euler_overview_text: those classes through the frame formatter of euler_render (its colour runs, escapes and line ends), W x H glyphs; rainbow != 0:
 * every water glyph carries the colour of the box's mean dye, dye[c] / (water * 2^24).  With one cell per pixel (W = X - 2, H = Y - 2) the
 * text is euler_render(sim, X - 2, Y - 2) byte for byte; with the dye each colour byte is within 1 of it (q truncates to 24 bits).
 * Same sizing protocol as euler_render. */
int euler_overview_text(const euler_overview_px* px, int32_t W, int32_t H, int32_t rainbow,
                        char* out, int32_t cap, int32_t* len);
enum {
  EULER_IMAGE_COVERAGE = 0,   /* water = (64, 128, 255) */
  EULER_IMAGE_DYE = 1,        /* water = the sRGB bytes of the box's mean dye (the formula of the coloured frame); records without dye: black water */
  EULER_IMAGE_SPEED = 2       /* water = ((int)(255 t + 0.5), 128, (int)(255 (1 - t) + 0.5)), t = min(1, sqrtf(max_speed2) / speed_scale) */
};
/* W * H * 3 bytes, row 0 = top.  Per channel (solid * S + sink * K + water * Wc + cells / 2) / cells in integers, air = 0, S = 128, K = 64,
 * Wc by mode (above).  EULER_IMAGE_SPEED needs speed_scale > 0; another mode, rgb_bytes != W * H * 3: EULER_EINVAL. */
int euler_overview_rgb(const euler_overview_px* px, int32_t W, int32_t H, int32_t mode, float speed_scale,
                       uint8_t* rgb, size_t rgb_bytes);
/* The fit-to-window frame: euler_overview with W = min(wx, X - 2), H = min(wy, Y - 2), then euler_overview_text (coloured on a handle created
 * with euler_config.rainbow).  Sizing protocol of euler_render; wx < 1 or wy < 1: EULER_EINVAL. */
int euler_render_fit(euler_sim* sim, int32_t wx, int32_t wy, char* out, int32_t cap, int32_t* len);

/* ---- pan-and-zoom viewport (docs/viewport.md) ------------------------------------------------ */
/* The overview of a BOX of interior cells [x0, x1] x [y0, y1] (inclusive, as for euler_diagnostics below): 1 <= x0 <= x1 <= X - 2 and
 * 1 <= y0 <= y1 <= Y - 2, Bw = x1 - x0 + 1, Bh = y1 - y0 + 1, 1 <= W <= Bw, 1 <= H <= Bh, out_bytes exactly W * H * sizeof(euler_overview_px): else
 * EULER_EINVAL.  Pixel column px covers x = x0 + floor(px * Bw / W) ... x0 + floor((px + 1) * Bw / W) - 1; pixel row py = 0 is the top and covers
 * y = y1 - floor(py * Bh / H) down to y1 + 1 - floor((py + 1) * Bh / H).  The records are euler_overview_px as above; with the whole interior as the
 * box they are euler_overview's, which is this call on (1, 1, X - 2, Y - 2): the same launch, the same device buffer and its growth (EULER_ENOMEM: the
 * handle unchanged), the same EULER_ESTATE refusals.  Reads the state only. */
int euler_overview_box(euler_sim* sim, int32_t x0, int32_t y0, int32_t x1, int32_t y1,
                       int32_t W, int32_t H, euler_overview_px* out, size_t out_bytes);
/* Above one cell per pixel: the MARKERS of the box (EULER_F_MARKERS, sub-cell positions) counted on the device into a raster of scale x scale
 * sub-pixels per cell.  scale is 1, 2, 4, 8 or 16; W = Bw * scale, H = Bh * scale, W * H <= 2^24 and out_bytes == W * H * 4: else EULER_EINVAL.
 * out[r * W + c] is the number of markers m with c = floor((m.x - x0) * scale) and r = H - 1 - floor((m.y - y0) * scale), counted only where
 * 0 <= c < W and 0 <= H - 1 - r < H (cell x is [x, x + 1), row 0 = top); a marker with a non-finite coordinate counts nowhere.  Positions are
 * below 2^24 and x0 is an integer no larger than an in-box m.x: the float subtraction is exact, the multiplication by a power of two is exact,
 * and the counts are integers that do not depend on the launch geometry (tests compare them exactly).  One pass over the marker array behind a
 * clear of the raster, on the handle's stream; it only READS the markers: stepping afterwards gives the bits of a run that never called it.
 * The raster's device buffer comes with the first call, grows on demand (EULER_ENOMEM: the handle unchanged) and goes with euler_destroy.
 * EULER_ESTATE without a loaded state.  On a row-slab handle the call is COLLECTIVE: it needs the communicator (else EULER_ESTATE), every rank calls with the same
 * arguments, counts its own markers into the raster rows of its own cell rows, and every rank gets the same bytes - the whole-grid handle's. */
int euler_marker_raster(euler_sim* sim, int32_t x0, int32_t y0, int32_t x1, int32_t y1,
                        int32_t scale, uint32_t* out, size_t out_bytes);
/* Host formatter of a magnified view (no GPU needed).  cells: the box at ONE cell per record (Bw x Bh records, row 0 = top); raster: the
 * (Bh * scale) x (Bw * scale) counts of euler_marker_raster over the same box.  Every cell becomes scale x scale glyphs through the frame formatter
 * of euler_render: a solid cell (the class of euler_overview_text) 'X', a sink cell '=', else the glyph index min(3, count of the sub-pixel), 0 = air;
 * rainbow != 0: a water glyph carries its cell's mean-dye colour.  Bw, Bh < 1, a scale other than 1, 2, 4, 8, 16 or more than 2^24 glyphs:
 * EULER_EINVAL.  Same sizing protocol as euler_render. */
int euler_view_text(const euler_overview_px* cells, const uint32_t* raster, int32_t Bw, int32_t Bh,
                    int32_t scale, int32_t rainbow, char* out, int32_t cap, int32_t* len);
/* The frame of a box in a window of wx x wy glyphs (wx < 1 or wy < 1: EULER_EINVAL).  Where the window holds the box at least twice in both
 * directions (Bw * 2 <= wx and Bh * 2 <= wy): the largest scale <= 16 with Bw * scale <= wx and Bh * scale <= wy, euler_overview_box at one cell per
 * pixel, euler_marker_raster, euler_view_text.  Otherwise euler_overview_box with W = min(wx, Bw), H = min(wy, Bh), then euler_overview_text.  Coloured
 * on a handle created with euler_config.rainbow.  Sizing protocol of euler_render.  On a row-slab handle the call is COLLECTIVE like the calls it is made of: it
 * needs the communicator (else EULER_ESTATE) and returns the same bytes on every rank, the whole-grid handle's. */
int euler_render_view(euler_sim* sim, int32_t x0, int32_t y0, int32_t x1, int32_t y1,
                      int32_t wx, int32_t wy, char* out, int32_t cap, int32_t* len);

/* ---- flow diagnostics (docs/diagnostics.md) ------------------------------------------------------ */
/* How good is a frame?  One pass ON THE DEVICE over a box of interior cells [x0, x1] x [y0, y1] (inclusive) reduces u, v, count and solid to the
 * record below; only its 88 bytes cross to the host.  A FLUID cell is the reference's is_fluid on a non-solid cell: count > 0 && !solid.  Per fluid
 * cell i = y * X + x, in float32 without contraction:
 *   d  = ((u[i] - u[i-1]) + v[i]) - v[i-X]            the divergence the velocity update left behind (main.c:720 in its order, h = 1)
 *   s2 = dx*dx + dy*dy, dx = (u[i] + u[i-1]) / 2, dy = (v[i] + v[i-X]) / 2      the cell-centre speed squared (euler_overview_px.max_speed2)
 *   qd(a) = (uint64_t)((a < 256 ? a : 256) * 16777216.f)              2^-24 units, saturating at 256
 *   qk(s) = (uint64_t)((s < 16777216.f ? s : 16777216.f) * 4294967296.f)    2^-32 units, saturating at 2^24
 * Both scales are powers of two: the multiply is exact, the conversion truncates - the same on host and device.  d and s2 are judged separately:
 * a NaN d adds nothing to div_l1 / max_div, a NaN s2 nothing to ke_* / max_speed2, and a cell with either counts ONCE in nonfinite; an infinity
 * saturates its sum and shows in its maximum.  The maxima are taken on the unsigned bit patterns of the non-negative floats.  Every field is an
 * integer sum or such a maximum, so the record does not depend on the launch geometry (tests compare bits).  No sum can wrap: a whole-grid handle
 * has at most 2^28 cells, a term is at most 2^32 (qd, the low half of qk), 2^24 (the high half) or 255 * 2^25 (count * x): every sum stays below 2^61. */
enum { EULER_DIAG_CROWDED = 8 };   /* a cell counts as crowded from this many markers on: twice the seeding density of 4 (main.c:255-266); the uint8 count wraps at 256 */
typedef struct euler_diag {      /* 88 bytes, no padding */
  uint64_t cells;      /* cells of the box */
  uint64_t fluid;      /* cells with count > 0 && !solid */
  uint64_t markers;    /* sum of count over the fluid cells */
  uint64_t crowded;    /* fluid cells with count >= EULER_DIAG_CROWDED */
  uint64_t mass_x;     /* sum of count * x over the fluid cells */
  uint64_t mass_y;     /* sum of count * y */
  uint64_t div_l1;     /* sum of qd(|d|) */
  uint64_t ke_hi, ke_lo; /* sums of qk(s2) >> 32 and qk(s2) & 0xffffffff */
  uint32_t count_max;  /* max count over the fluid cells */
  uint32_t nonfinite;  /* fluid cells whose d or s2 is a NaN (counted once) */
  float    max_div;    /* max |d| */
  float    max_speed2; /* max s2 */
} euler_diag;
typedef struct euler_diag_values {   /* what a user reads off a record; all 0 when fluid == 0 */
  double mean_abs_div;      /* div_l1 / 2^24 / fluid */
  double kinetic_energy;    /* 0.5 * (ke_hi + ke_lo / 2^32): density 1, cell volume 1 */
  double com_x, com_y;      /* mass_x / markers, mass_y / markers: the markers' centre of mass in cell indices */
  double markers_per_cell;  /* markers / fluid */
  double crowded_fraction;  /* crowded / fluid */
} euler_diag_values;
/* The box must lie in the interior, 1 <= x0 <= x1 <= X - 2 and 1 <= y0 <= y1 <= Y - 2, and out_bytes must be sizeof(euler_diag): else EULER_EINVAL.
 * EULER_ESTATE without a loaded state.  On a row-slab handle the call is COLLECTIVE: it needs the communicator (else EULER_ESTATE), every rank calls with the same
 * arguments and gets the same record, the whole-grid handle's - the ranks' records of their own rows, gathered and summed on the device.  One launch on the handle's stream
 * that only READS u, v, count, solid and the tile map: stepping afterwards gives the bits of a run that never called it.  The 88-byte device record
 * comes with the first call (EULER_ENOMEM: the handle unchanged) and goes with euler_destroy. */
int euler_diagnostics(euler_sim* sim, int32_t x0, int32_t y0, int32_t x1, int32_t y1, euler_diag* out, size_t out_bytes);
int euler_diag_derive(const euler_diag* rec, euler_diag_values* out);   /* host only, no GPU */

/* ---- flow raster (docs/flow_raster.md) ------------------------------------------------------------ */
/* Where does the water turn, which way does it move, how is the pressure spread?  The box, the raster and the pixel geometry of euler_overview_box
 * (a flow pixel covers the cells of the overview pixel at the same index), reduced on the device to the record below.  Per cell i = y * X + x, in
 * float32 without contraction; WATER is the overview's: !solid && !sink && count > 0.
 *   dx = (u[i] + u[i-1]) / 2, dy = (v[i] + v[i-X]) / 2        the cell-centre velocity of a water cell (euler_overview_px.max_speed2)
 *   w  = (v[i+1] - v[i]) - (u[i+X] - u[i])                    the vorticity (h = 1) at the NODE of cell (x, y), its top-right corner; the node is WET when
 *                                                             the cells i, i+1, i+X, i+X+1 are all water, and belongs to the pixel of cell (x, y) (for a cell in
 *                                                             the box's last column or top row the neighbours lie outside the box, inside the grid)
 *   pf = (float)p                                             p: the double euler_get_field(EULER_F_PRESSURE) returns for a water cell
 *   qv(a) = (uint64_t)((a < 4096.f ? a : 4096.f) * 1048576.f), a >= 0                               2^-20 units, saturating at 2^12
 *   qp(a) = (uint64_t)((a > 0.f ? (a < 16777216.f ? a : 16777216.f) : 0.f) * 256.f)                 2^-8 units, saturating at 2^24
 * Both scales are powers of two: the multiply is exact, the conversion truncates - the same on host and device.  A NaN term adds nothing to its sums
 * and maxima; an infinity saturates its sum and shows in its maximum; -0.f counts on the positive side with 0.  No sum can wrap (a term is at most 2^32,
 * a grid has at most 2^28 cells).  Every field is an integer sum or a maximum of non-negative floats taken on their bit patterns: the record does not
 * depend on the launch geometry, the atomics or the tile map (tests compare bits). */
enum { EULER_FLOW_PRESSURE = 1 };   /* flags: also reduce the pressure (p_sum, max_p) */
typedef struct euler_flow_px {   /* 88 bytes, no padding */
  uint32_t cells;       /* cells of the pixel */
  uint32_t water;       /* water cells */
  uint32_t nodes;       /* wet nodes whose vorticity is not a NaN */
  uint32_t nonfinite;   /* water cells with a NaN in any term they contribute (dx, dy, the w of their wet node, pf with the flag); once per cell */
  uint64_t u_pos, u_neg;   /* sums of qv(dx) over the water cells with dx >= 0, of qv(-dx) over those with dx < 0 */
  uint64_t v_pos, v_neg;   /* the same for dy */
  uint64_t w_pos, w_neg;   /* the same for w over the wet nodes */
  uint64_t p_sum;       /* sum of qp(pf) over the water cells; 0 without EULER_FLOW_PRESSURE */
  float    max_speed2;  /* max dx*dx + dy*dy over the water cells */
  float    max_abs_w;   /* max fabsf(w) over the wet nodes */
  float    max_p;       /* max of pf > 0 ? pf : 0; 0 without the flag */
  uint32_t reserved;    /* 0 */
} euler_flow_px;
/* The box, W and H as for euler_overview_box; out_bytes exactly W * H * sizeof(euler_flow_px) and no flag bit but EULER_FLOW_PRESSURE: else EULER_EINVAL.
 * EULER_ESTATE without a loaded state.  On a row-slab handle the call is COLLECTIVE: it needs the communicator (else EULER_ESTATE), every rank calls with the same
 * arguments and gets the same bytes, the whole-grid handle's.  Reads the state only: stepping afterwards gives the bits of a run that never
 * called it (with the flag the pending pressure is first finished in memory, as euler_get_field(EULER_F_PRESSURE) does).  The records' device buffer
 * comes with the first call, grows with W * H (EULER_ENOMEM: the handle unchanged) and goes with euler_destroy; no whole-grid staging copy is made. */
int euler_flow_raster(euler_sim* sim, int32_t x0, int32_t y0, int32_t x1, int32_t y1,
                      int32_t W, int32_t H, int32_t flags, euler_flow_px* out, size_t out_bytes);
/* Host only, no GPU: paints a field of the flow records into the dye sums of overview records of the same box, raster and state, so that every
 * formatter that shows the dye shows the field: euler_overview_text / euler_view_text with rainbow = 1, euler_overview_rgb(EULER_IMAGE_DYE).
 * Per pixel, in double: m_w = (w_pos - w_neg) / 2^20 / nodes (0 without nodes); m_p = p_sum / 256 / water; m_u = (u_pos - u_neg) / 2^20 / water, m_v
 * alike, m_s = sqrt(m_u^2 + m_v^2).  VORTICITY: t = clamp(m_w / scale, -1, 1), linear colour (1, 1-t, 1-t) for t >= 0, (1+t, 1+t, 1) for t < 0 (white in
 * the middle, red one way, blue the other).  PRESSURE, SPEED: t = clamp(m / scale, 0, 1), colour (t, 0.5, 1-t).  dye[c] = water * q((float)L_c) with the
 * q of euler_overview_px: the formatters' mean dye is exactly q(L_c) / 2^24.  Only px[k].dye is written.  EULER_EINVAL with px unchanged: a null
 * pointer, W < 1, H < 1, an unknown field, a scale that is not a finite positive number, a pixel whose cells or water differ between the rasters. */
enum { EULER_PAINT_VORTICITY = 0, EULER_PAINT_PRESSURE = 1, EULER_PAINT_SPEED = 2 };
int euler_flow_paint(const euler_flow_px* flow, euler_overview_px* px, int32_t W, int32_t H, int32_t field, double scale);

/* ---- batched gauges (docs/gauges.md) -------------------------------------------------------------- */
/* How high does the water stand at a column, where is the front, what load does a gate carry, how much passes under it, what does a pressure sensor
 * read?  A LIST of small instruments - each a kind and an inclusive box of interior cells - evaluated on the device in one launch and one read-back.
 * Per cell i = y * X + x, float32 without contraction; a FLUID cell is the diagnostics': count > 0 && !solid.  pf = (float)p, p the double
 * euler_get_field(EULER_F_PRESSURE) returns for the cell; qp, qv are euler_flow_px's.  A signed term a adds qv(a) to the _pos sum when a >= 0 (-0.f too)
 * and qv(-a) to the _neg sum otherwise.  A NaN term adds nothing to its sums and maxima and counts its cell once in nonfinite; an infinity saturates its
 * sum and shows in its maximum.  Every kind fills cells, fluid and the extent; beyond that
 *   LEVEL     nothing: hi_y over a strip of columns is a wave gauge, hi_x / lo_x a front tracker
 *   PRESSURE  over the fluid cells: a_pos = sum qp(pf), max_a = max(pf > 0 ? pf : 0), terms = fluid; a one-cell box is a pressure sensor
 *   FORCE     what the fluid cells of the box put on the solid cells they touch (h = 1, density 1: a wetted face carries pf): solid at x+1: qp(pf) into
 *             a_pos, at x-1: a_neg, at y+1: b_pos, at y-1: b_neg; terms counts wetted faces; max_a, max_b the largest face pressure in x and in y.  The
 *             solid neighbour may lie outside the box and on the border ring: the load on a gate is the box of the gate grown by one cell
 *   FLUX      per cell of the box its right face u[i] and its top face v[i], where the face is live as the velocity advection tests it:
 *             (count[i] || count[i+1]) && !(solid[i] || solid[i+1]) for u, with i+X for v; u into a_pos / a_neg, v into b_pos / b_neg; terms counts live
 *             faces of both kinds; max_a = max |u|, max_b = max |v|.  A box one column wide gives the discharge through x + 1/2
 * No sum can wrap: a term is at most 2^32 and a box has at most 2^28 cells.  Every field is an integer sum, an integer extreme or a maximum of
 * non-negative floats taken on their bit patterns: a record does not depend on launch geometry, atomics or the tile map (tests compare bits). */
typedef struct euler_gauge {      /* 24 bytes */
  int32_t kind;                   /* EULER_GAUGE_* */
  int32_t x0, y0, x1, y1;         /* inclusive, inside [1, X-2] x [1, Y-2] */
  int32_t reserved;               /* must be 0 */
} euler_gauge;
enum { EULER_GAUGE_LEVEL = 0, EULER_GAUGE_PRESSURE = 1, EULER_GAUGE_FORCE = 2, EULER_GAUGE_FLUX = 3 };
#define EULER_GAUGES_MAX 1024
typedef struct euler_gauge_rec {  /* 72 bytes, no padding */
  uint32_t cells, fluid;                /* cells of the box; fluid cells */
  uint32_t lo_x, hi_x, lo_y, hi_y;      /* extent of the fluid cells of the box; lo = 0xffffffff, hi = 0 when fluid == 0 */
  uint32_t terms, nonfinite;            /* terms summed (per kind, above); cells with a NaN term */
  uint64_t a_pos, a_neg, b_pos, b_neg;
  float    max_a, max_b;
} euler_gauge_rec;
typedef struct euler_gauge_values {   /* what a user reads off a record; all 0 when fluid == 0 */
  double a, b;        /* (a_pos - a_neg) / scale, (b_pos - b_neg) / scale; scale 2^8 for PRESSURE and FORCE, 2^20 for FLUX */
  double mean_a;      /* a / terms (0 without terms): the mean pressure of a PRESSURE gauge */
  double depth;       /* hi_y - lo_y + 1 */
} euler_gauge_values;
/* n gauges, 1 <= n <= EULER_GAUGES_MAX, into n records; gauges may overlap and repeat.  Refusals in this order: a null pointer (EULER_EINVAL), a row-slab
 * handle without a communicator, nothing loaded (EULER_ESTATE); n out of range or out_bytes != n * sizeof(euler_gauge_rec) (EULER_EINVAL); then per gauge, naming its index: an
 * unknown kind, reserved != 0, a box outside the interior or with x0 > x1 or y0 > y1 (EULER_EINVAL).  A refused call allocates nothing and leaves out
 * untouched.  Reads the state only: stepping afterwards gives the bits of a run that never called it (with a PRESSURE or FORCE gauge in the list the
 * pending pressure is first finished in memory, as euler_get_field(EULER_F_PRESSURE) does).  The device buffer of the pass comes with the first call, grows
 * with the list (EULER_ENOMEM: the handle unchanged) and goes with euler_destroy.  On a row-slab handle the call is COLLECTIVE: every rank calls with the same list
 * and gets the same records, the whole-grid handle's - each rank evaluates the tiles of the boxes in its own bands, the records are gathered and folded (sums added, extents and
 * maxima by min / max) on the device. */
int euler_gauges(euler_sim* sim, const euler_gauge* g, int32_t n, euler_gauge_rec* out, size_t out_bytes);
int euler_gauge_derive(const euler_gauge_rec* rec, int32_t kind, euler_gauge_values* out);   /* host only, no GPU; EULER_EINVAL: a null pointer, an unknown kind */

/* ---- device-side scene editing (docs/editing.md) -------------------------------------------------- */
/* Open a gate, drop a block of water, raise a wall, drain a pool while the run goes on: a box of interior cells [x0, x1] x [y0, y1] (inclusive, as for
 * euler_diagnostics) and the markers in it are edited ON THE DEVICE; nothing but a few counters crosses to the host.  A marker is "in the box" when
 * (floorf(m.x), floorf(m.y)) is a cell of the box.
 *   op       masks of the box's cells                 markers                       count of the box's cells
 *   SOLID    solid = 1, source = sink = 0             those in the box deleted      0
 *   SINK     sink = 1, solid = source = 0             those in the box deleted      0
 *   DRAIN    unchanged                                those in the box deleted      0
 *   CLEAR    solid = source = sink = 0                unchanged                     unchanged
 *   SOURCE   source = 1, solid = sink = 0, then seeded as by FILL (the parser's '?', main.c:230-232)
 *   FILL     unchanged                                appended                      4 where seeded
 * DELETING is refresh_marker_counts' removal (main.c:105-116) with "in the box" as its condition: the array is walked in order, a deleted marker is
 * replaced by the current last one, which is examined next.  SEEDING is sim_init's (main.c:255-266): the eligible cells - those of the box with
 * !solid && !sink && count == 0 after the op's mask change - are taken x outer, y inner; each appends four markers at the end of the array, marker k at
 * x = i + (k < 2 ? 0 : 0.5f) + randf() / 2, y = j + (k % 2 ? 0 : 0.5f) + randf() / 2, the x draw first, off the handle's one xorshift stream (the
 * sources' stream: euler_set_rng / euler_stats.rng_state), 8 draws per cell: euler_seed_markers over the eligible mask from the current state.  A draw
 * of exactly 1.0 puts a marker on its cell's far edge; the next refresh counts it where it lies.
 * With E eligible cells and n markers, n + 4 E > 4 X Y - 1: EULER_EINVAL, the state unchanged.  Not touched: u, v, utmp, vtmp, prev_count, precon, the
 * dye (euler_colorize recolours), the frame and solver counters, the exhausted latch; the next substep's stages meet the new masks as the reference's
 * would.  A continuation is therefore the reference's from the edited state, bit for bit, and equals loading the host-edited snapshot.
 * Refusals, in this order: a null handle EULER_EINVAL; a row-slab handle EULER_ESTATE (solid and source cells are facts a slab only gets from a load);
 * nothing loaded EULER_ESTATE; a box outside the interior (1 <= x0 <= x1 <= X - 2, 1 <= y0 <= y1 <= Y - 2) or an unknown op EULER_EINVAL.  A refused
 * call changes and allocates nothing.  The call works in the marker stage's scratch: no new device buffer (the source stage's draw buffer follows the number of source cells,
 * as after euler_set_field(EULER_F_SOURCE)); it waits for the device twice. */
enum { EULER_EDIT_SOLID = 0, EULER_EDIT_CLEAR = 1, EULER_EDIT_SINK = 2, EULER_EDIT_SOURCE = 3, EULER_EDIT_FILL = 4, EULER_EDIT_DRAIN = 5 };
int euler_edit_box(euler_sim* sim, int32_t op, int32_t x0, int32_t y0, int32_t x1, int32_t y1);

/* ---- forcing: gravity vector, shaken tank, force boxes (docs/forcing.md) --------------------------- */
/* Tilt or shake the tank, drive a current with a pump, run in reduced or zero gravity.  The handle keeps a double clock `time` (0 after a load, advanced
 * by time += (double)dt behind every substep of euler_step / euler_substep, in substep order; euler_stage does not advance it; it is not part of a
 * snapshot: euler_load_state leaves it at 0 and the forcing as set, the caller restores both; a session file, euler_save_session, carries both).  The uniform acceleration of a substep is
 * euler_forcing_at(f, time at the start of that substep): in double, a[0] = (float)(gx + shake_x sin(2 pi shake_hz t + shake_phase)), a[1] likewise from
 * gy, shake_y.  Per live face (live as for the FLUX gauge above), float32 without contraction, last in the velocity advection (with MacCormack: behind the
 * clamp): a live v face gets out += a[1] * dt, always; a live u face gets out += a[0] * dt ONLY when a[0] != 0.f (x + 0.f is not x for x = -0.f).  Then,
 * in front of the diffusion extension, the boxes: for k = 0 .. nboxes - 1 in list order, for every cell i of box k, utmp[i] += fx_k * dt where the cell's
 * right face is live and vtmp[i] += fy_k * dt where its top face is live (the product rounded, then the add).  Boxes may overlap and repeat: the adds on a
 * face come in list order.  A face that is not live stays 0.  The default record (0, -10, no shake, no boxes) is the reference's k_gravity: a handle that
 * holds it runs the kernels and produces the bits of one that never called euler_set_forcing. */
#define EULER_FORCE_BOXES_MAX 64
typedef struct euler_force_box { int32_t x0, y0, x1, y1; float fx, fy; } euler_force_box;   /* 24 bytes; inclusive, inside [1, X-2] x [1, Y-2] */
typedef struct euler_forcing {     /* 48 bytes, no padding */
  float   gx, gy;                  /* uniform acceleration; default 0, -10 */
  float   shake_x, shake_y;        /* amplitudes of a harmonic acceleration of the tank frame; default 0 */
  double  shake_hz, shake_phase;   /* frequency in 1 / s of simulated time, phase in radians */
  int32_t nboxes, reserved;        /* reserved must be 0 */
  double  reserved2;               /* must be 0 */
} euler_forcing;
int euler_forcing_default(euler_forcing* f);
/* Refusals, in this order: a null sim or f (EULER_EINVAL); a row-slab handle without a communicator (EULER_ESTATE, "slab" in the text); nothing loaded
 * (EULER_ESTATE); reserved or reserved2 not 0; a non-finite value or |gx|, |gy|, |shake_x|, |shake_y| > 1e4; shake_hz < 0 or non-finite, a non-finite
 * phase; nboxes outside [0, EULER_FORCE_BOXES_MAX] or boxes == NULL with nboxes > 0; a box's fx or fy non-finite or beyond 1e4 in size (a value comes in
 * front of any box's place); a box outside the interior or with x0 > x1 / y0 > y1, naming the index of the first such box (all EULER_EINVAL).  A refused call changes and allocates nothing.  May be called between any two calls - frames,
 * substeps, stages; touches no grid.  The boxes and their tile table go to a device buffer of the handle once per call (grown on demand, counted in
 * euler_hbm_bytes, released by euler_destroy).  On a row-slab handle with a communicator the call is COLLECTIVE (docs/forcing.md "On row slabs"): behind its own
 * checks every rank compares a digest of the record and the list with the others; if any rank refused its own or the digests differ, every rank returns an error
 * and nothing has changed.  The codes are NOT the same on every rank: the rank whose own record was refused returns its EULER_EINVAL with its reason, every other rank
 * EULER_ESTATE with "differs between ranks" in the text - a job tests for != EULER_OK.  Last refusal there, behind the agreement: a buffer that one rank could not
 * reserve is EULER_ENOMEM on every rank, and every rank is left without boxes.  A rank keeps the table entries of its own bands.  The
 * uniform part is formed from the rank's own clock: euler_set_time is local, the caller keeps the ranks' clocks equal. */
int euler_set_forcing(euler_sim* sim, const euler_forcing* f, const euler_force_box* boxes);   /* boxes may be NULL when nboxes == 0 */
int euler_get_forcing(euler_sim* sim, euler_forcing* f, euler_force_box* boxes, int32_t cap);  /* boxes may be NULL (the record alone); else cap >= nboxes */
int euler_forcing_at(const euler_forcing* f, double t, float a[2]);   /* host only, no GPU */
int euler_get_time(euler_sim* sim, double* t);
int euler_set_time(euler_sim* sim, double t);   /* EULER_EINVAL: a non-finite t */

/* ---- temperature: an advected scalar with buoyancy, heaters and diffusion (docs/heat.md) ----------- */
/* An ACTIVE scalar T, one float per cell, cell-centred like the dye: the flow carries it, boxes heat or cool it, it diffuses, and (Boussinesq) it makes water
 * lighter or heavier.  A cell is fluid when its marker count is not 0.  INVARIANT: behind euler_set_heat, euler_heat_set_field, euler_heat_fill and every
 * completed substep every cell without markers holds exactly `ambient`, in memory and in what euler_heat_get_field returns - so the field does not depend on
 * launch geometry or the tile map, and water that euler_edit_box(FILL) adds starts at `ambient`.  Whole-grid handles only.  Per substep, float32 without
 * contraction (docs/heat.md has every operation):
 *   EULER_STAGE_SOURCES, behind the dye's work: a cell with prev_count == 0 && count != 0 takes the mean of its 3 x 3 neighbours with prev_count != 0, summed
 *     y-major then x and divided by their number n; n == 0: `ambient`.  Then every cell with source != 0 takes source_t, whatever its count.
 *   EULER_STAGE_ADVECT_VELOCITY, behind the velocity advection, its uniform forcing and the force boxes, in front of the viscosity extension:
 *     a. T moves as one dye channel under the handle's transport options (reading the stage's input u, v); only fluid cells take the result.
 *     b. for k = 0 .. nboxes - 1 in list order, every fluid cell of box k: FIX: T = value; RATE: T = fl(T + fl(value dt)).
 *     c. kappa > 0: Jacobi from b's values, c = fl(kappa dt), T' = fl(T + fl(c acc)), acc = 0 then acc = fl(acc + fl(T_n - T)) for the left, right, lower and
 *        upper neighbour in that order where that neighbour is fluid (solids and air are insulated).
 *     d. cells without markers take `ambient`.
 *     e. beta != 0, (ax, ay) the substep's uniform acceleration ((0, -10) or euler_forcing_at at the handle's clock): a live v face i (live as for the force
 *        boxes) has Tf = fl(fl(T[i] + T[i+X]) / 2) when both cells are fluid, else the fluid cell's T; d = fl(Tf - ambient); d == 0: the face is not touched;
 *        else vtmp[i] = fl(vtmp[i] - fl(fl(beta d) fl(ay dt))).  A live u face likewise with i + 1, ax and utmp, and only when ax != 0.  Faces that are not
 *        live are neither read nor written.
 * With beta == 0 the heat changes no bit of u, v, markers, counts, RNG or dye.  With any beta a field that is `ambient` everywhere changes none of them
 * either WHERE THE TRANSPORT REPRODUCES THE CONSTANT: fl(fl(fl(1 - f) a) + fl(f a)) is a again for a = 0 and for a power of two, not for every float - with
 * ambient = 20, say, a transported cell can come out one ulp off and the buoyancy acts on that ulp (docs/heat.md).  Choose such an ambient where this matters.  A handle that never calls
 * euler_set_heat launches what it always launched.  Heat is no part of a snapshot: a scenario load and euler_load_state keep the record and reset the field
 * to `ambient`.  A session file (euler_save_session) carries the record, the boxes and the field. */
#define EULER_HEAT_BOXES_MAX 64
enum { EULER_HEAT_FIX = 0, EULER_HEAT_RATE = 1 };
typedef struct euler_heat_box { int32_t x0, y0, x1, y1; float value; int32_t kind; } euler_heat_box;   /* 24 bytes; inclusive, inside [1, X-2] x [1, Y-2] */
typedef struct euler_heat {        /* 32 bytes, no padding */
  float   ambient;                 /* T0: the temperature of water nobody heated, and of every cell without markers; default 0 */
  float   beta;                    /* expansion coefficient; 0 = a passive scalar; default 0 */
  float   kappa;                   /* diffusivity, 0 <= kappa <= 2.5 (kappa dt / h^2 <= 0.25 for every dt <= the 0.1 s frame, h = 1); default 0 */
  float   source_t;                /* what the scenario's source cells hold; default 0 */
  int32_t nboxes, reserved;        /* reserved must be 0 */
  double  reserved2;               /* must be 0 */
} euler_heat;
int euler_heat_default(euler_heat* h);
/* h == NULL switches heat off: the handle launches what it launched before and keeps its buffers; the next switching-on starts from `ambient` everywhere.
 * The first call with a record reserves the arrays (device buffers of the handle, counted in euler_hbm_bytes, grow-only, released by euler_destroy) and sets
 * every cell to `ambient`; a later one replaces beta, kappa, source_t and the boxes and keeps the field.  Refusals, in this order: a null sim
 * (EULER_EINVAL); a row-slab handle without a communicator (EULER_ESTATE, "slab"); nothing loaded (EULER_ESTATE); then EULER_EINVAL for: reserved or reserved2 not 0; a non-finite value or
 * |ambient|, |beta|, |source_t| > 1e4; kappa outside [0, 2.5]; another ambient than the live one (the dry cells hold it); nboxes outside
 * [0, EULER_HEAT_BOXES_MAX] or boxes == NULL with nboxes > 0; a box with an unknown kind, a non-finite value or |value| > 1e4, outside the interior or
 * inverted, naming the first such box.  A refused call changes and allocates nothing.  On a row-slab handle with a communicator the call is COLLECTIVE, h == NULL
 * included, with the agreement of euler_set_forcing behind its own checks and its codes - the refusing rank its own EULER_EINVAL, the others EULER_ESTATE; a failed
 * reservation on one rank EULER_ENOMEM on all, heat on or off as it was and without boxes (docs/heat.md "On row slabs"); the field is the rank's window, two halves of it. */
int euler_set_heat(euler_sim* sim, const euler_heat* h, const euler_heat_box* boxes);
int euler_get_heat(euler_sim* sim, euler_heat* h, euler_heat_box* boxes, int32_t cap);   /* EULER_ESTATE while heat is off; boxes may be NULL, else cap >= nboxes */
/* The field, X * Y floats, row-major; on a row-slab handle the rank's own rows, (row_hi - row_lo) * X floats, and euler_heat_set_field / euler_heat_fill are COLLECTIVE
 * there (they end with the exchange of T's ghost rows).  Refused: a null argument (EULER_EINVAL), a row-slab handle without a communicator, nothing loaded or heat off (EULER_ESTATE), another byte
 * count, a box outside the interior or inverted, a value that is not finite or beyond 1e4 in size (EULER_EINVAL).  euler_heat_set_field writes `ambient`
 * over what the caller gave for cells without markers; euler_heat_fill sets T = value in the cells of the box that hold markers, now. */
int euler_heat_get_field(euler_sim* sim, float* dst, size_t bytes);
int euler_heat_set_field(euler_sim* sim, const float* src, size_t bytes);
int euler_heat_fill(euler_sim* sim, int32_t x0, int32_t y0, int32_t x1, int32_t y1, float value);
/* The temperature per pixel: the box, the raster, the pixel edges and the definition of water (solid == 0 && sink == 0 && count != 0) are
 * euler_overview_box's.  d = T - ambient of a water cell goes to the sum of its sign - t_pos += qv(d) for d >= 0 (-0.f too), t_neg += qv(-d) for d < 0,
 * qv the flow raster's: min(a, 4096) * 2^20, truncated - and to the maximum of its side, taken on bit patterns; a NaN goes to neither (the cell still counts
 * as water), an infinity is the clamp's 4096 in the sums and itself in the maxima.  Integer sums and bit-pattern maxima: the record does not depend on the
 * launch geometry.  On a row-slab handle COLLECTIVE like euler_overview_box: every rank reads the whole-grid bytes.  Refusals: a null argument (EULER_EINVAL), a row-slab
 * handle without a communicator, nothing loaded or heat off (EULER_ESTATE), a box outside the interior, W or
 * H < 1 or above the box's extent, another byte count than W * H records (EULER_EINVAL).  Reads the state only. */
typedef struct euler_heat_px {       /* 32 bytes */
  uint32_t cells;                    /* cells of the pixel */
  uint32_t water;                    /* water cells of the pixel */
  uint64_t t_pos, t_neg;             /* the sums of qv(d) over water cells with d >= 0, and of qv(-d) over those with d < 0 */
  float    max_above, max_below;     /* the maxima of d and of -d where positive; 0 where there is none */
} euler_heat_px;
int euler_heat_raster(euler_sim* sim, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t W, int32_t H, euler_heat_px* out, size_t out_bytes);
/* Host only, no GPU: paints heat records into the dye sums of overview records of the same box, raster and state, as euler_flow_paint paints the
 * vorticity: m = (t_pos - t_neg) / 2^20 / water (0 without water), t = clamp(m / scale, -1, 1); t >= 0: (1, 1 - t, 1 - t), white to red; t < 0:
 * (1 + t, 1 + t, 1), white to blue; dye[c] = water * q(colour[c]).  Only px[k].dye is written.  EULER_EINVAL with px unchanged: a null heat or px, W or
 * H < 1, a scale that is not finite and positive, records whose cells or water differ from px's.  (`ambient` is the raster's own: the records hold
 * differences; the argument is kept for callers that label a legend and must be finite.) */
int euler_heat_paint(const euler_heat_px* heat, euler_overview_px* px, int32_t W, int32_t H, float ambient, double scale);

/* ---- passive tracers: device-side pathlines, streaklines and a raster (docs/tracers.md) ------------ */
/* Where does this water go, how long does it stay, does it ever reach that corner?  A set of TRACERS lives on the device and moves with the flow by the
 * marker's own rule; the fluid's markers cannot answer (their array order changes with every deletion, their dt is shortened by earlier markers'
 * collisions: they are state, not instruments).  Whenever EULER_STAGE_ADVECT_MARKERS runs on a whole-grid handle with tracers - euler_step, euler_substep,
 * euler_stage - ONE extra launch (profile class marker_advect), issued on the handle's stream BEFORE the marker launches of that stage, advects all of them.
 * It reads the row-major u, v, count, solid and sink as they stand at that moment and the stage's dt, follows EULER_OPT_ADVECT_RK2 as the markers do, and
 * touches no other state: a handle with tracers produces the fields, markers and RNG state of one without, and a handle that never adds one launches
 * exactly what it launched before.  One tracer, one substep, float32 without contraction:
 *   1. RETIRED set: nothing changes.
 *   2. cx = (int)floorf(x), cy = (int)floorf(y); x or y not finite, cx outside [0, X-1] or cy outside [0, Y-1]: flags |= RETIRED | LOST, stop (before any grid read).
 *   3. solid[cy*X+cx]: flags |= RETIRED | IN_SOLID, stop; else sink[..]: flags |= RETIRED | IN_SINK, stop.  The position stays.
 *   4. wet = count[..] != 0; (x', y') = the walk of ONE marker through the substep (main.c:464-537 for an array of one marker) with the stage's full dt:
 *      a tracer never sees the dt an earlier marker's collision shortened and never shortens anyone's.
 *   5. path += sqrtf(dx*dx + dy*dy), dx = x' - x, dy = y' - y (sqrtf correctly rounded); age += dt; wet_time += dt only if wet; ++substeps.
 *   6. WET becomes wet; WAS_DRY is set for good if !wet; x, y = x', y'.
 * A tracer in air does not move (the masked velocity there is 0).  Scenario loads, the half-tank loaders and euler_load_state clear the tracers;
 * euler_set_field, euler_set_markers, euler_edit_box, euler_set_forcing and euler_set_time leave them alone (a wall raised over a tracer retires it on
 * its next substep).  Tracers are not part of a snapshot; a session file (euler_save_session) carries their records.  Whole-grid handles only. */
#define EULER_TRACERS_MAX (1u << 22)
enum { EULER_TRACER_WET = 1, EULER_TRACER_RETIRED = 2, EULER_TRACER_IN_SOLID = 4, EULER_TRACER_IN_SINK = 8,
       EULER_TRACER_LOST = 16, EULER_TRACER_WAS_DRY = 32 };
typedef struct euler_tracer {   /* 32 bytes, no padding */
  float    x, y;        /* position in the markers' units (k_side_length = 1: cell (floorf(x), floorf(y))) */
  float    path;        /* sum over its substeps of sqrtf(dx*dx + dy*dy), dx = x' - x, dy = y' - y */
  float    age;         /* sum of the dt of its substeps */
  float    wet_time;    /* sum of the dt of the substeps it began in a cell with count > 0 */
  uint32_t substeps;    /* substeps it was advected in */
  uint32_t flags;       /* EULER_TRACER_* */
  uint32_t reserved;    /* 0 */
} euler_tracer;
/* Appends n tracers at (xy[2k], xy[2k+1]), all other words 0: one host-to-device copy.  Refusals, in this order: a null handle (EULER_EINVAL); a row-slab
 * handle (EULER_ESTATE); nothing loaded (EULER_ESTATE); n > 0 with a null xy; count + n > EULER_TRACERS_MAX; a position that is not finite or outside
 * 1 <= x < X - 1, 1 <= y < Y - 1, naming the first such index (all EULER_EINVAL).  A refused call changes and allocates nothing; n == 0 is a no-op.  A
 * position inside a solid or sink cell is accepted and retires on its first substep.  The store is one device buffer of the handle, counted in
 * euler_hbm_bytes, doubled on demand (the records keep their bits; EULER_ENOMEM: the handle unchanged) and released by euler_destroy. */
int euler_tracers_add(euler_sim* sim, const float* xy, size_t n);
int euler_tracers_count(euler_sim* sim, size_t* n);
/* Records [first, first + n) in the order they were added: one copy and one wait.  EULER_EINVAL: first + n > count, out_bytes != n * 32; n == 0 succeeds. */
int euler_tracers_get(euler_sim* sim, size_t first, size_t n, euler_tracer* out, size_t out_bytes);
int euler_tracers_clear(euler_sim* sim);   /* count = 0; the buffer stays */
/* The tracers per pixel: the box, W, H and the pixel geometry of euler_overview_box; out_bytes exactly W * H * 4 and no flag bit but
 * EULER_TRACER_RASTER_ALL: else EULER_EINVAL.  out[py * W + px] is the number of tracers whose cell (floorf(x), floorf(y)) lies in the box and is covered
 * by pixel (px, py); retired tracers count only with EULER_TRACER_RASTER_ALL; a tracer with a non-finite coordinate counts nowhere.  The pixel of a cell is
 * formed in integers (column c = cx - x0 of the box: px = ((c + 1) * W - 1) / Bw; row r = y1 - cy from the top: py = ((r + 1) * H - 1) / Bh) and the
 * counts are integer adds: they do not depend on the launch geometry (tests compare them exactly).  One pass over the records behind a clear of the
 * raster; it reads only.  Without tracers: a raster of zeros.  EULER_ESTATE without a loaded state and on a row-slab handle. */
enum { EULER_TRACER_RASTER_ALL = 1 };   /* also count retired tracers */
int euler_tracer_raster(euler_sim* sim, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t W, int32_t H,
                        int32_t flags, uint32_t* out, size_t out_bytes);
/* Host only, no GPU: paints a tracer raster into the dye sums of overview records of the same box and raster, as euler_flow_paint does.  Where
 * counts[k] > 0 && px[k].water > 0: dye[c] = water * q(fg[c]) with the q of euler_overview_px; where bg is not NULL, counts[k] == 0 and water > 0:
 * dye[c] = water * q(bg[c]); everything else stays (a tracer shows only on water pixels).  Only px[k].dye is written.  EULER_EINVAL with px unchanged:
 * a null counts, px or fg, W < 1 or H < 1. */
int euler_tracer_paint(const uint32_t* counts, euler_overview_px* px, int32_t W, int32_t H,
                       const float fg[3], const float* bg /* 3 floats or NULL */);

/* ---- moving bodies: solid boxes that push water at a prescribed velocity (docs/bodies.md) ---------- */
/* A piston, a paddle, a plunger, a sliding sluice: up to EULER_BODIES_MAX solid rectangles of whole cells that follow a prescribed path through the water.
 * THE LAW OF MOTION is a stateless function of the handle's clock (euler_get_time), computed on the host in double: p(t) = x + vx t + amp_x sin(2 pi hz t + phase),
 * px = clamp(p(t), 2, X - 2 - w), ox = (int)floor(px + 0.5); the same in y with h and Y.  The clamp keeps the rectangle [ox, ox + w - 1] x [oy, oy + h - 1] inside
 * [2, X - 3] x [2, Y - 3] for all time: a body that reaches the edge stops there.  euler_body_at is that function; no sin runs on the device.
 * PER SUBSTEP of euler_step / euler_substep with step dt at clock t, in front of the tracers' and the markers' advection (euler_stage: in
 * EULER_STAGE_ADVECT_MARKERS; the clock does not advance there, so a repeated stage call shifts nothing twice):
 *   1. for each body in list order the target (tx, ty) is the origin of euler_body_at(t + dt);
 *   2. the body moves from its remembered origin (ox, oy) to the target one cell at a time, all x shifts first, then y.  A shift by +1 in x: every marker with
 *      floorf(m.x) == ox + w and oy <= floorf(m.y) <= oy + h - 1 takes m.x = fl(m.x + 1.f) (the water is pushed ahead of the face and keeps its place in the
 *      array); the cells of column ox + w get the masks and the count of EULER_EDIT_SOLID (solid = 1, source = sink = 0, count = 0); column ox gets
 *      EULER_EDIT_CLEAR (a body carves what it passes through); ox += 1.  Mirrored for -1 (the markers of column ox - 1 take fl(m.x - 1.f)) and for y.  The counts of
 *      the cells the markers land in are not updated: the refresh that follows counts them where they lie (a marker that lands in a wall is deleted there);
 *   3. when any body shifted, every body's rectangle gets the SOLID masks and the zero counts again in list order (one body's CLEAR cannot open another).
 * A substep in which no body shifts launches nothing here.
 * THE WALL VELOCITY of the substep is the mean velocity over it, wx = (float)((px(t + dt) - px(t)) / (double)dt) and wy likewise (0 while the body is clamped).  At the
 * start of EULER_STAGE_PROJECT, for the bodies in list order, a u face on the left or right edge of a body's rectangle takes utmp = wx when its outside cell has
 * count != 0 && !solid and wx != 0.f; the v faces of the lower and upper edge take vtmp = wy likewise.  The same faces are set back to 0.f behind the stage.  The
 * right-hand side picks the velocity up (every fluid cell reads its four faces, solid ones too); the velocity update leaves u = v = 0 on the body's faces.  A body
 * with wx == wy == 0 is bit for bit a wall made by euler_edit_box.
 * Bodies are not part of a snapshot: a scenario load and euler_load_state drop them (n = 0; their cells are whatever the loaded masks say); a session file (euler_save_session) carries the list and the
 * remembered origins.  Whole-grid handles only. */
#define EULER_BODIES_MAX 16
typedef struct euler_body {          /* 64 bytes, no padding */
  double  x, y;                      /* lower-left corner at t = 0, in cells, continuous */
  double  hz, phase;                 /* of the harmonic part; 1/s of simulated time, radians */
  float   vx, vy;                    /* constant velocity, cells per second */
  float   amp_x, amp_y;              /* amplitude of the harmonic part, cells */
  int32_t w, h;                      /* size in cells, >= 1 */
  int32_t reserved[2];               /* 0 */
} euler_body;
typedef struct euler_body_state { double px, py; int32_t ox, oy; } euler_body_state;   /* 24 bytes */
/* host only, no GPU.  EULER_EINVAL: a null pointer, w or h < 1, w > X - 4 or h > Y - 4 (no place inside the clamp range) */
int euler_body_at(const euler_body* b, double t, int32_t X, int32_t Y, euler_body_state* out);
/* Replaces the handle's list at its present clock: the rectangles of the old list are cleared (the mask change of EULER_EDIT_CLEAR), each new body's rectangle is made
 * solid exactly as EULER_EDIT_SOLID does (markers inside deleted), and the origin of each body is remembered.  n == 0 (bodies may be NULL) removes them.
 * Refusals, in this order: a null sim (EULER_EINVAL); a row-slab handle (EULER_ESTATE); nothing loaded (EULER_ESTATE); then EULER_EINVAL for n outside
 * [0, EULER_BODIES_MAX] or a null list with n > 0; per body, naming the first bad one: reserved not 0; a non-finite value; w, h < 1, w > X - 4 or h > Y - 4; hz < 0;
 * a speed bound |vx| + 2 pi hz |amp_x| > 10 (or the same in y) cells per second - one cell per 0.1 s frame.  A refused call changes and allocates nothing.
 * While bodies are set, euler_edit_box refuses (EULER_ESTATE) a box that intersects a body's current rectangle. */
int euler_set_bodies(euler_sim* sim, const euler_body* bodies, int32_t n);
/* The list as set (bodies may be NULL, else cap >= *n on return: EULER_EINVAL otherwise) and, where now is not NULL, per body the position at the handle's clock with
 * the REMEMBERED origin in ox, oy (the cells that are solid now); *n the number of bodies. */
int euler_get_bodies(euler_sim* sim, euler_body* bodies, int32_t cap, euler_body_state* now, int32_t* n);

/* ---- marker density control: thin crowded cells, refill torn holes (docs/reseed.md) ---------- */
/* Opt-in, whole-grid handles only; the reference has nothing like it, and a handle that never switches it on launches what it launched and gives the same bits.
 * While it is on, one PASS runs as the tail of every EULER_STAGE_REFRESH_COUNTS - in a substep and in euler_stage, not in the refresh a load runs - on the marker
 * array and the count grid the refresh has just left (h = 1):
 *   thinning (thin_above != 0)
 *     1. the crowded cells are those whose count BYTE exceeds thin_above; the first max_cells of them in row-major order are LISTED, the others add to `deferred`;
 *     2. marker i lies in cell (cx, cy) = (floorf(x), floorf(y)) and there in sub-cell sx = min((int)floorf((x - (float)cx) * 4.f), 3), sy alike (both operations
 *        are exact);
 *     3. in each of the 16 sub-cells of a listed cell the marker with the lowest array index survives, every other marker of a listed cell is deleted;
 *     4. the deletion is the reference's loop m[i--] = m[--n] (main.c:105-116) over delete flags computed before it begins, each travelling with its marker;
 *     5. count of a listed cell becomes the number of its occupied sub-cells (>= 1); prev_count and every other grid stay.
 *   filling (fill_holes), behind the thinning
 *     1. a hole is an interior cell with count == 0 && prev_count != 0, neither solid nor sink nor source, whose eight neighbours all have count != 0 || solid;
 *     2. the first max_fill holes in row-major order are listed, the others add to `deferred`;
 *     3. listed hole k appends one marker at (x + rx, y + ry), ry = draw 2 k and rx = draw 2 k + 1 of the handle's one stream from where it stands (the order of
 *        update_fluid_sources, main.c:288), and its count becomes 1; appending stops when the array holds max_markers - 1 markers (the holes left over add to
 *        `deferred`; the source stage's latch is not written);
 *     4. u, v, the dye and the temperature are untouched: the cell was water one refresh ago, its samples stand, and no extrapolation fires (prev_count != 0).
 * Tracers and dye are not pushed.  The settings survive a scenario load and euler_load_state like the options; they are not part of a snapshot.
 * A session file (euler_save_session) carries the record and the totals. */
typedef struct euler_reseed {      /* 32 bytes, no padding */
  int32_t thin_above;   /* 0: no thinning; else 4 ... 254: a cell whose count byte exceeds it is thinned */
  int32_t fill_holes;   /* 0 / 1 */
  int32_t max_cells;    /* crowded cells thinned per pass; 0 = 65536; at most 1 << 20 */
  int32_t max_fill;     /* holes filled per pass;           0 = 65536; at most 1 << 20 */
  int32_t reserved[4];  /* 0 */
} euler_reseed;
typedef struct euler_reseed_stats { uint64_t removed, added, cells_thinned, deferred; } euler_reseed_stats;   /* totals since the last euler_set_reseed */
/* NULL or an all-zero record switches the pass off.  Refusals, in this order: a null sim (EULER_EINVAL); a row-slab handle (EULER_ESTATE); nothing loaded
 * (EULER_ESTATE); then EULER_EINVAL with the field named: reserved not 0; thin_above not 0 and outside [4, 254]; fill_holes outside {0, 1}; max_cells or max_fill
 * negative or above 1 << 20.  A refused call changes and allocates nothing.  An accepted one zeroes the totals. */
int euler_set_reseed(euler_sim* sim, const euler_reseed* r);
/* The record as set (all zero: off; the limits as given, 0 where the default stands) and the totals; either pointer may be NULL. */
int euler_get_reseed(euler_sim* sim, euler_reseed* r, euler_reseed_stats* stats);

/* ---- run-long envelopes: arrival time, wet time, peak speed and peak pressure per cell (docs/envelope.md) ---- */
/* Opt-in, whole-grid handles only; a handle that never switches it on launches what it launched.  While channels are on, the handle holds one plane per channel of
 * one 32-bit word per cell of the X x Y grid, and every EULER_STAGE_PROJECT ends - behind the bodies' face withdrawal, in a substep and in euler_stage - with one
 * update of the interior cells that are FLUID at that moment (count != 0 && !solid, as the gauges define it), in float32 without contraction:
 *   channel               initial word            update
 *   EULER_ENV_ARRIVAL     0xffffffff ("never")    a word that is still 0xffffffff becomes the bits of t_end = (float)(euler_get_time() + (double)dt), the clock taken
 *                                                 before the substep
 *   EULER_ENV_WET         +0.f                    w = w + dt
 *   EULER_ENV_SPEED       +0.f                    the maximum, as bit patterns, of the word and s2 = dx*dx + dy*dy, dx = (u[i] + u[i-1]) / 2, dy = (v[i] + v[i-X]) / 2
 *   EULER_ENV_PRESSURE    +0.f                    the maximum of the word and pf > 0.f ? pf : 0.f, pf = (float) of the double euler_get_field(EULER_F_PRESSURE) shows
 * A NaN in s2 or pf is skipped.  A cell that is not fluid is not touched in any channel: a cell that is solid now keeps what it gathered while it was wet.  The clock
 * does not advance inside euler_stage, so a repeated euler_stage(EULER_STAGE_PROJECT) accumulates again with the same t_end.  With the pressure channel on the pending
 * pressure is finished first (as euler_get_field does); nothing else of the state is touched: fields, markers, generator and counters are those of a handle without it.
 * The planes are not part of a snapshot or of a session file: a scenario load, euler_load_state and euler_load_session switch the envelope off. */
enum { EULER_ENV_ARRIVAL = 1, EULER_ENV_WET = 2, EULER_ENV_SPEED = 4, EULER_ENV_PRESSURE = 8, EULER_ENV_ALL = 15 };
/* Refusals of the calls below, in this order, changing and allocating nothing: a null handle or pointer (EULER_EINVAL); a row-slab handle (EULER_ESTATE, "slab" in
 * the text); nothing loaded (EULER_ESTATE); then EULER_EINVAL for the call's own arguments.
 * euler_set_envelope: channels is a set of EULER_ENV_* bits (a bit outside EULER_ENV_ALL: refused).  A newly enabled channel's plane is allocated (EULER_ENOMEM: the
 * handle as it was) and takes its initial words, a disabled one is freed, one that stays enabled keeps its words; 0 switches the feature off.  The substep count
 * starts from 0 whenever the envelope goes from off to on.  The planes are counted in euler_hbm_bytes: 4 X Y bytes each, the pressure's - kept in the solver's
 * band-skewed order - 4 S bytes for the S elements of a skewed array. */
int euler_set_envelope(euler_sim* sim, uint32_t channels);
/* the channels that are on and the substeps accumulated since the envelope was switched on or last reset; either pointer may be NULL */
int euler_get_envelope(euler_sim* sim, uint32_t* channels, uint64_t* substeps);
/* the enabled planes back to their initial words, the substep count to 0 */
int euler_envelope_reset(euler_sim* sim);
/* One plane, row-major, X * Y words (row 0 first); channel is exactly one enabled bit and bytes == 4 * X * Y: else EULER_EINVAL.  euler_envelope_set_field restores
 * a plane the caller kept: an arrival word must be 0xffffffff or a finite float >= 0, any other channel's word a finite float >= +0 (no NaN, no -0.f); otherwise
 * EULER_EINVAL with the first bad index named and the plane unchanged. */
int euler_envelope_get_field(euler_sim* sim, int32_t channel, float* dst, size_t bytes);
int euler_envelope_set_field(euler_sim* sim, int32_t channel, const float* src, size_t bytes);
typedef struct euler_envelope_px {   /* one pixel = one box of interior cells; 32 bytes.  Integer sums and extremes of bit patterns: exact in any order */
  uint32_t cells;        /* cells of the box */
  uint32_t touched;      /* ... whose arrival word is set (0 with that channel off) */
  uint32_t arrival_min;  /* the unsigned minimum of the arrival words (bits of a float; 0xffffffff: no cell was reached, or the channel is off) */
  uint32_t arrival_max;  /* the maximum over the words that are set; 0: none */
  uint32_t wet_max;      /* maxima of the words as bit patterns; 0 with the channel off */
  uint32_t speed2_max;
  uint32_t p_max;
  uint32_t reserved;     /* 0 */
} euler_envelope_px;
/* The planes per pixel: the box, W, H, the pixel geometry and the row order of euler_overview_box; out_bytes exactly W * H * sizeof(euler_envelope_px).  Reads the
 * planes only (they are a history: the tile map of the present state does not apply). */
int euler_envelope_raster(euler_sim* sim, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t W, int32_t H, euler_envelope_px* out, size_t out_bytes);
/* host only, no GPU: W * H * 3 bytes, row 0 = top.  A pixel with touched == 0 is (0, 0, 0) - for a channel other than the arrival, only if that
 * channel's extreme is 0 as well: with the arrival channel off nothing counts as touched, and the extreme alone says whether water was there.  Otherwise t = clamp(value / scale, 0, 1) in double, value = arrival_min, wet_max,
 * sqrt(speed2_max) or p_max read as floats, and the colour is (255, 255 (1 - t), 255 (1 - t)), truncated.  EULER_EINVAL with rgb untouched: a null pointer, W or H < 1,
 * a channel that is not one EULER_ENV_* bit, a scale that is not finite and positive, rgb_bytes != W * H * 3. */
int euler_envelope_rgb(const euler_envelope_px* px, int32_t W, int32_t H, int32_t channel, double scale, uint8_t* rgb, size_t rgb_bytes);

/* ---- multi-GPU: 1-D row slabs (DESIGN.md "Multi-GPU") ------------------------------ */
/* One process per GPU.  Two layouts share the communicator interface below:
 *   row slabs for EVERY stage (euler_config.slab_nranks >= 1; the default of bench.py --gpus N): a handle holds only the rows of
 *     its 64-row bands (+ ghost rows) of every field and the markers inside them; ghost rows of u / v / counts, marker migration,
 *     the dt all-reduce and the distributed PCG all go through these operations;
 *   round 1's layout (euler_set_comm on a full-size handle): only the pressure solve - project(), main.c:709-806 - is partitioned
 *     into slabs of bands, the cheap stages run replicated on the whole grid.  Kept because its exact IC(0) coupling
 *     (EULER_SLAB_EXACT) is the one multi-rank mode that reproduces the single-GPU ITERATES.
 * The library drives the substep and calls these operations at its exchange points; the host program implements them
 * (euler_amd/slab.py: torch.distributed) or installs the library's own RCCL communicator (euler_set_comm_rccl).
 * All pointers are DEVICE pointers into the handle's buffers; operations must be ordered on the
 * stream given to euler_set_stream.  Each returns 0 on success. */
typedef struct euler_comm_ops {
  void*   ctx;
  int32_t rank, nranks;
  /* in-place all-reduce of `count` doubles: sum (is_max = 0) or max (is_max = 1) */
  int (*allreduce)(void* ctx, void* dev_f64, int32_t count, int32_t is_max);
  /* ghost rows of the search vector: send_lo/recv_lo <-> rank-1, send_hi/recv_hi <-> rank+1
   * (`count` doubles each; the ends of the chain skip the missing side) */
  int (*halo)(void* ctx, void* send_lo, void* send_hi, void* recv_lo, void* recv_hi, int32_t count);
  /* point-to-point: rank `src` sends nbytes at dev_ptr, rank `dst` receives into its own dev_ptr */
  int (*chain)(void* ctx, void* dev_ptr, int64_t nbytes, int32_t src, int32_t dst);
  /* all-gather: rank r contributes bytes [off[r], off[r]+cnt[r]) of the array at dev_base */
  int (*allgather)(void* ctx, void* dev_base, const int64_t* off, const int64_t* cnt);
  /* ONE exchange for a PCG iteration's latency-bound traffic (SURVEY 8e "fuse ... into one message pair"; optional - null: the
   * library issues halo + allgather instead): `count` doubles to / from each neighbour exactly like halo (count = 0: none), AND
   * an all-gather of `nsmall` doubles per rank: rank r's contribution sits at small[r * nsmall] (in place), every rank ends up
   * with all of them, which it folds in rank order - the same bits everywhere.  The built-in RCCL communicator issues all of it
   * as one group of sends and receives. */
  int (*exchange)(void* ctx, void* send_lo, void* send_hi, void* recv_lo, void* recv_hi, int32_t count, void* small, int32_t nsmall);
} euler_comm_ops;

enum {
  EULER_SLAB_EXACT = 1,   /* band hand-off rows forwarded rank to rank: the reference's IC(0), the
                             1-GPU iterates; the triangular sweeps then run one slab after another */
  EULER_SLAB_LOCAL = 0    /* IC(0) restricted to each slab (block-Jacobi across slabs): slabs sweep
                             concurrently; NOT the reference's iterates (tolerance only) */
};
int euler_set_comm(euler_sim* sim, const euler_comm_ops* ops, int32_t coupling);

/* The library's own communicator: the four operations above issued straight to RCCL (xGMI on an
 * MI355X node) on the handle's stream - no host code between two kernels of a PCG iteration.
 * Rank 0 creates an id (EULER_RCCL_ID_BYTES bytes = ncclUniqueId) and the launcher hands the same
 * bytes to every rank over whatever host channel it has (torchrun's store, MPI, a file); then every
 * rank calls euler_set_comm_rccl collectively, after hipSetDevice-equivalent euler_create on its own
 * GPU.  RCCL is bound at run time (dlopen of librccl.so.1; a copy already in the process is reused);
 * EULER_ECOMM if it is absent.  nranks = 1 is accepted and keeps the communicator code path (self-test). */
#define EULER_RCCL_ID_BYTES 128
int euler_rccl_unique_id(void* id_out, int32_t cap);
int euler_rccl_version(void);                                  /* NCCL-style version code, -1 if unavailable */
int euler_set_comm_rccl(euler_sim* sim, const void* unique_id, int32_t id_bytes, int32_t rank, int32_t nranks,
                        int32_t coupling);
/* Per-handle options (round 5): the forms and test hooks that used to be EULER_* environment variables read once per process.  Two handles of one process may
 * differ.  euler_set_option validates the value and the moment (a key that shapes allocations or a communicator must be set before what it shapes exists) and leaves
 * the handle untouched when it refuses; none of the keys changes a result's bits unless its line says so. */
enum {
  EULER_OPT_P_STEPS = 1,            /* 2, 4 or 8 (default): p += alpha s is applied N iterations at a time out of a ring of N search arrays (the fmadds of main.c:753 in their order: the same bits) */
  EULER_OPT_TILE_STORE_AS = 2,      /* 1: k_search_apply stores A s' and the r update reads it back (round 3's form; the same bits); 0 (default): formed twice */
  EULER_OPT_TILE_REVERSE = 3,       /* 0: k_precond_tile walks the chunk list upwards; 1 (default): downwards */
  EULER_OPT_RESIDENT_CAP = 4,       /* > 0: the resident solver's capacity in workgroups, at most the device's own (tests: a scene that outgrows the chip); 0: the device's */
  EULER_OPT_GRID4_MIN_CELLS = 5,    /* grids of at least this many cells run extrapolate / zero_bounds four cells per thread (default 2^22; the same bits) */
  EULER_OPT_SLAB_FUSION = 6,        /* 1: with the mailboxes connected, read the neighbouring slabs' edge rows where they live (set on every rank, before euler_p2p_connect) */
  EULER_OPT_RCCL_SMALL = 7,         /* the small all-gather inside the RCCL exchange: 0 by size (default), 1 always ncclAllGather, 2 always sends / receives (before euler_set_comm_rccl) */
  EULER_OPT_RCCL_NO_EXCHANGE = 8,   /* 1: the built-in communicator without the fused exchange (halo + allgather instead: the same traffic; before euler_set_comm_rccl) */
  EULER_OPT_MARKERS_ROWMAJOR = 9,   /* 1: the marker stages read the row-major grids (A-B timing; the same bits) */
  EULER_OPT_SA_RUN = 10,            /* 8 (default), 16, 32: pair-records per wave of k_search_apply (experiments).  16 / 32: the parity and the plain tile-local mode on one GPU only - refused (EULER_ESTATE) while a communicator or a coarse-correction mode is installed, and a handle that gets one later runs runs of 8 whatever the value */
  EULER_OPT_NO_INTERIOR = 11,       /* 1: no constant-mask instantiation for interior chunks (experiments; the same bits) */
  EULER_OPT_BUILD_GATHER = 12,      /* 1: the assembly as one diagonal gather (rounds 1-2; the same bits) */
  EULER_OPT_RESIDENT_FORCE_TIMEOUT = 13, /* test hook: the next n resident launches give up at once as if a wait had run out (error word 1): the time-out path */
  EULER_OPT_MG_SPLIT_LEVEL = 14,    /* multilevel mode on row slabs: the level whose right-hand side the ranks all-gather (below it every rank works on its own rows, docs/solver_multilevel.md): 0 (default) by size,
                                       n > 0 that level (tests: the split on small grids), -1 never (the cycle replicated from level 0 on).  The same value on every rank */
  EULER_OPT_MG_SPLIT_ACTIVE = 15,   /* read only: the gather level the last multilevel solve on row slabs ran with, 0 while the cycle runs replicated */
  EULER_OPT_MARKERS_TWO_PASS = 16,  /* 1: advect_markers and refresh_marker_counts as separate passes over the marker array (rounds 1-5; A-B timing; the same bits); 0 (default): the advection pass bins what it writes */
  EULER_OPT_BUILD_TWO_PASS = 17,    /* 1: the assembly as a row-major pass + a skewed gather (rounds 3-5; A-B timing; the same bits); 0 (default): one pass over parallelograms of the band-skewed layout */
  EULER_OPT_VELOCITY_TWO_PASS = 18, /* 1: k_finish_p + k_velocity_update as in rounds 1-5 (A-B timing; the same bits); 0 (default): one pass */
  EULER_OPT_NO_TILE_MAP = 19,       /* 1: the grid passes visit every cell as in rounds 1-5 (A-B timing; the same bits); 0 (default): tiles of 64 x 64 cells with no water in or next to them in
                                       the count grid and the previous one are left alone by advect_u / advect_v, zero_bounds, extrapolate and the marker stage's copies (their output there is the zeros already in place) */
  EULER_OPT_PROFILE_STRIDE = 20,    /* n >= 1 (default 1): euler_profile_enable brackets every n-th launch of an enabled kernel class with its event pair (a pair costs the stream
                                       a few microseconds of serialisation: all ~230 launches of an 8192^2 substep bracketed cost bench.py's headline 3.9 %); the class's time and
                                       launch count are those of the bracketed launches */
  EULER_OPT_TILE_STORE_Z = 21,      /* 1: k_precond_tile stores z and k_search_apply reads it (rounds 2-6; the same bits); 0 (default): the tile-local mode on one GPU stores only z's halo
                                       and k_search_apply forms z again from r; every solve still ends with z stored whole */
  EULER_OPT_ADVECT_RK2 = 22,        /* CHANGES THE BITS.  0 (default): the reference's forward-Euler transport; 1: the midpoint rule (RK2) for the back-traces of u, v and the dye and for
                                       the marker move (docs/advection_rk2.md).  May change between any two calls; a row-slab handle refuses 1 (EULER_ESTATE: the midpoint
                                       samples reach one row beyond the slab's ghost rows) */
  EULER_OPT_ADVECT_MACCORMACK = 23, /* CHANGES THE BITS.  0 (default): the reference's semi-Lagrangian transport; 1: MacCormack with the Selle et al. clamp for u, v and the dye
                                       (docs/advection_maccormack.md), with either trace of EULER_OPT_ADVECT_RK2.  May change between any two calls; the first switch to 1
                                       allocates two grids of scratch (EULER_ENOMEM: nothing changed); a row-slab handle refuses 1 (EULER_ESTATE: the correction reads the
                                       forward result one row beyond the own rows) */
  EULER_OPT__COUNT
};
int euler_set_option(euler_sim* sim, int32_t key, int64_t value);
int euler_get_option(euler_sim* sim, int32_t key, int64_t* value);

int euler_comm_calls(euler_sim* sim, uint64_t out[5]);         /* built-in communicator: allreduce, halo, chain, allgather, exchange calls so far */

/* Peer-to-peer mailboxes for the latency-bound exchanges (csrc/comm_p2p.hip): the three 8-byte all-reduces
 * and the ghost-row exchange of every PCG iteration become direct writes into the peers' mailboxes (HIP IPC
 * mappings of fine-grained device memory; xGMI between the GPUs of a node) - one small kernel each, no
 * collective library in the loop, sums formed in rank order (bit-identical on every rank).  The bulk
 * transfers (band hand-off rows, all-gather of p) stay on the communicator installed before.
 *   1. every rank:  euler_p2p_export(sim, handle)          -> EULER_P2P_HANDLE_BYTES bytes (IPC handles)
 *   2. the launcher gathers the handles of all ranks, in rank order, on every rank (any host channel)
 *   3. every rank:  euler_p2p_connect(sim, handles, nranks) after euler_set_comm[_rccl]; maps the mailboxes and
 *      proves the path with an all-reduce of known values.  On failure the installed communicator stays as it is. */
#define EULER_P2P_HANDLE_BYTES 256   /* four hipIpcMemHandle_t: the mailbox and the z / s / s2 arrays (read across slab boundaries) */
int euler_p2p_export(euler_sim* sim, void* handle_out, int32_t cap);
int euler_p2p_connect(euler_sim* sim, const void* handles, int32_t nranks);
int euler_p2p_disconnect(euler_sim* sim);                      /* back to the installed communicator; frees the mailbox */
int euler_p2p_calls(euler_sim* sim, uint64_t out[2]);          /* all-reduces, ghost-row exchanges over the mailboxes so far */
int euler_set_stream(euler_sim* sim, void* hip_stream);   /* run on the caller's HIP stream (e.g. torch's) */
int euler_slab_info(euler_sim* sim, int32_t* band_lo, int32_t* band_hi, int32_t* nbands);

/* ---- measurement ------------------------------------------------------------------------- */
/* Per-kernel-class timing with HIP events on the library's own stream.  class_mask bit i
 * enables class i (see euler_profile_class_name); 0 disables. */
int euler_profile_enable(euler_sim* sim, uint64_t class_mask);
int euler_profile_class_count(void);
const char* euler_profile_class_name(int32_t cls);
int euler_profile_get(euler_sim* sim, int32_t cls, double* total_ms, uint64_t* launches);
int euler_profile_reset(euler_sim* sim);
/* Device-to-device copy bandwidth probe (float4 copy kernel), GB/s read+write. */
int euler_measure_copy_bandwidth(euler_sim* sim, size_t bytes, int32_t reps, double* gbps);
int euler_measure_exchange(euler_sim* sim, int32_t reps, int32_t row_doubles, int32_t nsmall, double* us_per_exchange);   /* collective: one exchange point of a distributed PCG iteration over the installed communicator, HIP-event time per call */
int euler_device_name(euler_sim* sim, char* out, int32_t cap);
/* Device memory the handle holds NOW (a row-slab handle: its slab only): the counted bytes of the handle's memory ledger (docs/handle_memory.md) - everything it
 * allocated at creation and since (the solver's ring and halo buffers with the first solve that needs them, a coarse mode's arrays when it is selected, every
 * feature's buffers), except the source cells' draws and the transfer scratch of euler_get_field / euler_set_field. */
uint64_t euler_hbm_bytes(const euler_sim* sim);
/* Diagnostics: the band pipeline of the most recent IC(0) sweep launch.  For each of this rank's bands in
 * sweep order, 8 words: wave entry, first block's boundary ready, wave exit (100 MHz constant clock
 * ticks), (blocks run << 32 | blocks that had to wait for the previous band), and four hand-off time
 * stamps that only a development build fills (k_sweep.hip SW_TRACE_HANDOFF; else 0).  `out` holds
 * 8 * cap_bands words.  Returns the number of bands written (<= cap_bands) or a negative error. */
int euler_sweep_timeline(euler_sim* sim, uint64_t* out, int32_t cap_bands);

#ifdef __cplusplus
}
#endif
#endif /* EULER_H */
