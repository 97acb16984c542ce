// k_pcg.h — internal: what the files of the pressure solve share (k_pcg.hip, k_sweep.hip, k_tile.hip, k_search.hip; k_coarse.hip, k_mg.hip, k_mg_cycle.hip, k_mg_split.hip, k_resident.hip, k_slab.hip, k_grid.hip).
//
// HBM layout.  Every solver array (b, p, r, z, s, q, precon, cell mask) is private to the solver,
// so it is stored BAND-SKEWED rather than row-major (struct SkewGeom, euler_dev.h):
//     element (row y, column x)  ->  band b = y / 64, lane l = y % 64, record t = x + l
//                                    index  = (b * TS + (t & ~1)) * 64 + 2 * l + (t & 1)
// (T = X + 63 rounded up to even records per band, band stride TS = roundup32(T) + 64 records).
// A record (the 64 elements of one t) is exactly what one wave touches in one step of the IC(0)
// wavefront sweeps (lane l at column t - l).  Records are stored in PAIRS: a lane's elements of
// records 2P and 2P+1 are adjacent, so one 16-byte access per lane serves two steps of a sweep
// (1 KB per wave, perfectly coalesced, no LDS transposition; a lone wave pays per memory
// instruction, not per byte).  The backward sweep walks the same pairs downwards.  The 5-point
// neighbours are the pair partner / the facing element of the adjacent pair (left, right) and the
// same of the neighbouring lane (down, up): still coalesced; band-crossing neighbours of lane 0 /
// lane 63 go through the index function.  Padding entries (t - l outside [0,X), rows >= Y) carry
// mask 0 for ever: every kernel treats them as non-fluid cells, which removes all edge predicates.
//
// Device-resident control: alpha, beta, sigma, the residual norm, the iteration count and the
// `done` flag live in PcgScalars in HBM; every kernel reads them first and returns at once after
// convergence, so the host enqueues iterations without a round trip and polls `done` every few
// iterations.
//
// Bit-exactness: every element-wise kernel evaluates the reference's expression in the
// reference's association order (-ffp-contract=off); the IC(0) sweeps have no reduction, so any
// dependency-respecting schedule gives the sequential sweep's bits; dot() is either replayed in
// the reference's row-major order (EULER_DOT_SEQUENTIAL) or reduced in a fixed tree.
#pragma once

#include "euler_dev.h"
#include "k_mg.h"

#define COMM_CALL(expr) do { if ((expr) != 0) { eu_set_error("communicator callback failed: %s", #expr); return EULER_ECOMM; } } while (0)
// element range of this rank (the whole array without a communicator)
#define LOC(ptr) ((ptr) + S->e_lo)
enum { SW_FACTOR = 0, SW_FORWARD = 1, SW_BACKWARD = 2 };      // the sweeps of eu_launch_sweep

// ---- launchers that cross the solver's files
int eu_launch_build_system(euler_sim* S, float dt);                      // k_grid.hip
int eu_launch_velocity_update(euler_sim* S, float dt, int finish);
int eu_launch_band_ranges(euler_sim* S);                                 // k_sweep.hip
int eu_launch_sweep(euler_sim* S, int op, int cls, int force, int fin_qq = -1);
int eu_launch_factor_tile(euler_sim* S, int force);                      // k_tile.hip
int eu_launch_precond_tile(euler_sim* S, int rupd, int sweeps, int fin_dot, int force, double alpha, bool r_only = false, int zform = -1);
int eu_launch_search_apply(euler_sim* S, int it);                        // k_search.hip
int eu_launch_finish_p(euler_sim* S);                                    // k_pcg.hip: the p += alpha s still due, in memory
int eu_launch_dot(euler_sim* S, const double* a, const double* b, int fin_op, int force);
int eu_comm_exchange(euler_sim* S, double* send_lo, double* send_hi, double* recv_lo, double* recv_hi, int count, double* small, int nsmall);
int eu_comm_finish(euler_sim* S, int fin_op, int is_max, int force);
int eu_comm_halo_two(euler_sim* S, double* a, double* b);
bool tile_recompute(const euler_sim* S);
int p_steps(const euler_sim* S);

// scalar epilogues of the reductions (pcg_scalar_step)
enum { FIN_SIGMA_INIT = 0, FIN_ALPHA, FIN_RNORM, FIN_BETA, FIN_STORE_ONLY, FIN_TO_COMM };
#define FIN_VIA_P2P 0x100   // multi-rank with mailboxes: the last block all-reduces its total peer to peer, then applies the epilogue

// ---- what a handle's configuration selects
// tile-local IC(0) in its production form: everything between two apply_a passes in one kernel (k_precond_tile)
static inline bool tile_fused(const euler_sim* S) { return eu_is_tile(S) && S->cfg.sweep_mode != EULER_SWEEP_SIMPLE; }
// several ranks in tile-local mode without mailboxes: the neighbouring slabs' edge rows travel as compact rows (k_pcg.hip "ghost rows")
static inline bool ghost_mode(const euler_sim* S) { return S->has_comm && !S->p2p_on && tile_fused(S); }
enum { XR_ZSEND_LO = 0, XR_ZSEND_HI, XR_ZRECV_LO, XR_ZRECV_HI, XR_GS_LO0, XR_GS_LO1, XR_GS_HI0, XR_GS_HI1 };
static inline double* xrow(const euler_sim* S, int k) { return S->xrows + (size_t)k * S->xrow_len; }
static inline int sa_run(const euler_sim* S) {   // short runs while long ones would leave CUs without a wave
  if (S->opt[EULER_OPT_SA_RUN] != 8 && !S->has_comm && !eu_is_two_level(S)) return (int)S->opt[EULER_OPT_SA_RUN];      // (experiments: 16, 32)
  // measured (same box, tile-local mode): 8192^2 - 8: 346 us, 16: 358, 32: 376 (113 / 134 / 185 VGPRs: occupancy beats the window's
  // two extra pair loads per run, which hit L2); 16384^2, scanning every run's masks - 8: 1412 us, 32: 1389; with the list of active
  // chunks (runs of 8 only) - 8: 1177 us, 32: 1401
  return 8;
}
// z is not stored either (round 7): the r update's k_precond_tile leaves only z's halo (TileArgs::zform 1) and the next k_search_apply<.., ZR> forms z again from r
// with the same tile solve.  8 bytes per fluid cell and iteration less: 8192^2 (docs/solver_tile_local.md).  One GPU, the plain tile-local mode, tree dots, runs of one tile;
// EULER_OPT_TILE_STORE_Z restores the stored form.  z stays observable: every solve ends with z stored whole (tile_z_begin / eu_launch_project)
static inline bool tile_z_recompute(const euler_sim* S) {
  return tile_recompute(S) && tile_fused(S) && !eu_is_two_level(S) && S->tile_w == 16 && !S->has_comm && !S->slab_on && S->band_lo == 0 &&
         S->opt[EULER_OPT_TILE_STORE_Z] == 0 && S->chunk_list && S->tile_table;
}
static inline int fin_or_comm(const euler_sim* S, int fin_op) {
  return S->has_comm ? (S->p2p_on ? (fin_op | FIN_VIA_P2P) : (int)FIN_TO_COMM) : fin_op;
}

#ifdef __HIPCC__
#define RED_THREADS 1024
typedef double sw_d2 __attribute__((ext_vector_type(2)));   // a lane's pair of records (16-byte accesses)

__device__ __forceinline__ bool pcg_idle(const PcgScalars* sc) { return sc->done || !sc->nonzero; }

#define DPP_WAVE_SHL1 0x130
#define DPP_WAVE_SHR1 0x138

// lane l <- neighbouring lane's v; the lane without a source (0 for shr, 63 for shl) receives `edge`
template <int CTRL>
__device__ __forceinline__ double wave_shift_inject(double v, double edge) {
  const int lo = __builtin_amdgcn_update_dpp(__double2loint(edge), __double2loint(v), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(__double2hiint(edge), __double2hiint(v), CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}


__device__ __forceinline__ void pcg_scalar_step(PcgScalars* sc, int op, double v) {
  switch (op) {
    case FIN_SIGMA_INIT: sc->sigma = v; break;                                        // main.c:748
    case FIN_ALPHA: sc->zs = v; sc->alpha_prev = sc->alpha; sc->alpha = sc->sigma / v; sc->alpha_hist[sc->iters & 7] = sc->alpha; sc->iters += 1; break;     // main.c:750-752
    case FIN_RNORM: sc->rnorm = v; if (v <= sc->tol) sc->done = 1; break;             // main.c:756
    case FIN_BETA: sc->sigma_new = v; sc->beta = v / sc->sigma; sc->sigma = v; break; // main.c:762-765
    case FIN_TO_COMM: sc->comm_val = v; if (sc->comm_slot) *sc->comm_slot = v; break;   // multi-rank: the epilogue runs after the exchange
    default: sc->sigma_new = v; break;
  }
}

// fixed-shape block reductions of an NT-thread block; result valid in thread 0
template <int NT = RED_THREADS>
__device__ __forceinline__ double block_sum(double v) {
  __shared__ double sw[NT / 64];
  v = eu_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) for (int k = 0; k < NT / 64; ++k) t += sw[k];
  return t;
}
template <int NT = RED_THREADS>
__device__ __forceinline__ double block_max(double v) {
  __shared__ double sm[NT / 64];
  v = eu_wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) for (int k = 0; k < NT / 64; ++k) t = sm[k] > t ? sm[k] : t;
  return t;
}

// "Last block reduces": each block publishes its partial (8-byte agent-scope atomic store =
// write-through), drains, takes a ticket; the block that draws the last ticket folds ALL partials
// in index order (so the result does not depend on arrival order: deterministic) and applies the
// scalar epilogue.  Saves one launch + one kernel boundary per reduction (3 per PCG iteration).
// Hand-off form: 8-byte agent atomics on both sides (MI355X_MICROARCH "valid forms").
template <bool IS_MAX, int NT = RED_THREADS>
__device__ __forceinline__ void block_finish(double v_block, double* partial, unsigned int* counter, PcgScalars* sc, int op) {
  __shared__ int am_last;
  if (threadIdx.x == 0) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(&partial[blockIdx.x]),
                       (unsigned long long)__double_as_longlong(v_block), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned int t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    am_last = t == gridDim.x - 1;
  }
  __syncthreads();
  if (!am_last) return;
  double v = 0.0;
  for (unsigned int i = threadIdx.x; i < gridDim.x; i += NT) {
    const double w = __longlong_as_double((long long)__hip_atomic_load(
        reinterpret_cast<unsigned long long*>(&partial[i]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    if (IS_MAX) v = w > v ? w : v; else v += w;
  }
  v = IS_MAX ? block_max<NT>(v) : block_sum<NT>(v);
  if (op & FIN_VIA_P2P) { v = p2p_allreduce_block<IS_MAX>(sc, v); op &= 0xff; }   // op is uniform: every thread of this block is here
  if (threadIdx.x == 0) {
    pcg_scalar_step(sc, op, v);
    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next reduction
  }
}

// What a neighbouring RANK reads across a slab boundary (k_search_apply<true>: the edge rows of z and of the search
// direction) is stored once more WRITE-THROUGH at system scope by the kernel that has it in registers anyway, and every
// thread drains its stores before the block joins the reduction whose all-reduce releases the readers: the remote loads
// then do not depend on what a kernel boundary flushes.  `edges` bit 0 / 1: this slab has a neighbour below / above.
__device__ __forceinline__ void st_system(const double* p, double v) {
  asm volatile("global_store_dwordx2 %0, %1, off sc0 sc1" :: "v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ bool slab_edge_row(size_t e, int l, int TS, int nb_local, int edges) {
  if (l != 0 && l != 63) return false;
  const int band = (int)(e / ((size_t)TS * 64));
  return l == 0 ? ((edges & 1) && band == 0) : ((edges & 2) && band == nb_local - 1);
}
__device__ __forceinline__ double ld_system(const double* p) {
  double v;
  asm volatile("global_load_dwordx2 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
  return v;
}

struct SlabNeighbours {
  const double *z_dn, *s_dn, *z_up, *s_up;   // SLAB 1: the arrays of rank-1 / rank+1, offset like the local ones; null = no such rank
  int nb_local;                              // bands of this slab
  // SLAB 2 (the default with several ranks in tile-local mode): the neighbouring slabs' edge rows as COMPACT rows of X doubles
  // indexed by the column - z as it arrived with the iteration's one exchange, s as this rank keeps it up to date ITSELF: the
  // ghost cell's s' = z + beta s is formed here with the owner's expression (identical bits) and stored for the next iteration,
  // so only z ever travels.  null = no such rank.
  const double *zrow_dn, *srow_dn, *zrow_up, *srow_up;
  double *snew_dn, *snew_up;
};

// z = M^-1 r of ONE tile of W records (tile-local IC(0), main.c:602-626 restricted to the tile): L q = r, then L^T z = q from the tile's last
// record down.  mm: the cells' masks by pair-record, rr: r, pp: E^-1, zz: q on the way, z at the end.  k_precond_tile (DOT: dot(z, r) over the
// fluid cells, accumulated into dsum in the order of the backward recurrence) and k_search_apply<.., ZR> (forming z again from r) share it:
// the same expressions under -ffp-contract=off, so both get the same bits.  Every lane of the wave takes part (DPP shifts).
template <int W, bool DOT>
__device__ __forceinline__ void tile_solve(const unsigned int* mm, const sw_d2* rr, const sw_d2* pp, sw_d2* zz, double& dsum) {
  // L q = r (main.c:602-613).  What travels from cell to cell is m = (-1 * precon) * q, the term both consumers subtract.
  double own = -0.0, out = -0.0;
#pragma unroll
  for (int j = 0; j < W; ++j) {
    const int cm = (int)((mm[j >> 1] >> ((j & 1) * 8)) & 0xff);
    const double cin = (j & 1) ? rr[j >> 1].y : rr[j >> 1].x, cpre = (j & 1) ? pp[j >> 1].y : pp[j >> 1].x;
    const double nbv = wave_shift_inject<DPP_WAVE_SHR1>(out, -0.0);
    const double t = cin - own - nbv;
    const double qv = t * cpre;
    const double res = (cm & CM_FLUID) ? qv : 0.0;
    const double carry = -1.0 * cpre * res;
    own = carry; out = carry;
    if (j & 1) zz[j >> 1].y = res; else zz[j >> 1].x = res;
  }
  // L^T z = q (main.c:615-626), from the tile's last record down
  own = 0.0; out = 0.0;
#pragma unroll
  for (int j = W - 1; j >= 0; --j) {
    const int cm = (int)((mm[j >> 1] >> ((j & 1) * 8)) & 0xff);
    const double cin = (j & 1) ? zz[j >> 1].y : zz[j >> 1].x, cpre = (j & 1) ? pp[j >> 1].y : pp[j >> 1].x;
    const double nbv = wave_shift_inject<DPP_WAVE_SHL1>(out, 0.0);
    const double kr = ((cm & CM_RIGHT) ? -1.0 : 0.0) * cpre, ku = ((cm & CM_UP) ? -1.0 : 0.0) * cpre;
    const double t = cin - kr * own - ku * nbv;
    const double zv = t * cpre;
    const double res = (cm & CM_FLUID) ? zv : 0.0;
    own = res; out = res;
    if (DOT && (cm & CM_FLUID)) dsum += res * ((j & 1) ? rr[j >> 1].y : rr[j >> 1].x);
    if (j & 1) zz[j >> 1].y = res; else zz[j >> 1].x = res;
  }
}
// ZR (k_search_apply<.., ZR>, tile_z_recompute): z is not read from memory but formed again from r; what the run's window and its edge lanes
// need of the NEIGHBOURING tiles' z, k_precond_tile left behind in its "z halo only" form (TileArgs::zform 1):
//   halo  [band][tile][2][64]: record 0 / record 15 of every tile, all lanes (the records next to the neighbouring tiles)
//   rows  [band][2][X]: lane 0's / lane 63's z by column (what the bands below / above read across the band boundary)
struct ZrArgs { const double* r; const double* pre; const double* table; const double* halo; const double* rows; int X; };
struct CoarseRef { const double* y; int shift, nx, ny, band0; };   // y[ny][nx] over coarse cells of (1 << shift)^2 grid cells (COARSE 1) / over the multilevel mode's level-0 nodes (COARSE 2); band0: the global index of the arrays' band 0
struct SaHist { const double* s[6]; };   // PMODE N: the arrays of s_(k-N+1) .. s_(k-2) (N - 2 of them), offset like s_old

struct SweepArgs {
  SkewGeom g;
  const uint8_t* mask;
  const unsigned int* fbits_fwd;   // [nbands][fb_stride][64]: bit j of word (band, g, lane) = fluid flag of the lane's cell in
  const unsigned int* fbits_bwd;   // step 8g+j of the forward / backward sweep (k_pack_fbits); one dword load per block
  int fb_stride;
  double* pre;            // precon: in/out for SW_FACTOR, in otherwise
  const double* in;       // r (forward) / q (backward); unused for factor
  double* out;            // q (forward) / z (backward); unused for factor
  unsigned long long* granules;   // [nbands][gran_stride][2] tagged hand-off of a band's edge row
  int gran_stride;
  // k_sweep_skew<OP, true> (exact coupling over the peer-to-peer mailboxes, comm_p2p.hip): the slab's first band takes
  // its boundary row from the own mailbox (written by the previous slab's last band on ANOTHER GPU while both kernels
  // run), the slab's last band announces into the next slab's mailbox; one row of gran_stride granule pairs each
  const unsigned long long* xg_in;
  unsigned long long* xg_out;
  const int4* ranges;     // per band: active block ranges {fwd B0, fwd B1, bwd B0, bwd B1} (k_band_ranges)
  int band_lo, nb_local;  // this rank's bands [band_lo, band_lo + nb_local)
  int couple;             // 1: the first/last local band is coupled to the neighbouring rank's band
  unsigned int* ticket;
  unsigned int ticket_base;
  unsigned int epoch;
  const PcgScalars* sc;
  int force;
  int* error;
  unsigned long long* timeline;   // [nbands][8] {entry, first block ready, exit, blocks << 32 | stalled blocks, 4 development words} (euler_sweep_timeline)
  int tile_w;                     // k_sweep_simple only: > 0 = tile-local IC(0) with tiles of tile_w records (the cross-check of k_precond_tile)
  // forward sweep, tree-dot mode, one rank: dot(z, r) of the preconditioner application this sweep starts, formed HERE as
  // dot(q, q) - z = L^-T q and q = L^-1 r, so z.r = (L^-T q).(L q) = q.q exactly in real arithmetic (the backward solve applies
  // the transpose of the forward solve's L: same precon, symmetric couplings), a sum of squares with no cancellation.  It
  // replaces a launch that re-read z and r (17 B per cell); EULER_DOT_SEQUENTIAL keeps the reference's own dot(z, r).
  int fin_qq;                     // scalar epilogue (FIN_SIGMA_INIT / FIN_BETA) or -1
  double* qq_partial;             // [bands of the launch]
  unsigned int* qq_counter;
  PcgScalars* sc_w;
};

struct TileArgs {
  SkewGeom g;
  const uint8_t* mask;
  double* pre;            // factor: in/out; solve: in
  double* r;              // solve: r (updated in place when rupd)
  const double* as;       // A s of this iteration (rupd only)
  double* z;
  int band_lo, nb_local;
  int rupd;               // 1: r -= alpha A s first and report max |r| (a PCG iteration); 0: z = M^-1 r only (start of a solve)
  int sweeps;             // 0: the last iteration of the budget - only r and its norm are needed
  int fin_dot;            // scalar epilogue of dot(z, r): FIN_SIGMA_INIT / FIN_BETA / FIN_STORE_ONLY, -1 = none (replayed sequentially)
  int via;                // 0 single rank, FIN_VIA_P2P, or FIN_TO_COMM (multi-rank: how the two results reach the other ranks)
  double* part_max; double* part_dot;
  unsigned int* counter;
  const unsigned int* list;   // W == 16 inside a solve: the ascending list of active tiles (euler_dev.h "Active chunks"), else null
  const double* table;        // W == 16: E^-1 of an interior tile (k_tile_table); with it, listed interior tiles skip masks and precon
  PcgScalars* sc;
  int force;
  double alpha_arg;       // force: alpha of the r update (single building block, tests)
  double* pair_slot;      // FIN_TO_COMM: where this rank's {max |r|, dot(z,r)} go (its slot of the all-gather buffer)
  // several ranks, compact ghost rows (k_search_apply SLAB 2): the slab's lowest / highest row of z goes out as a row of X doubles,
  // written by the lanes that hold it (lane 0 of band edge_lo, lane 63 of band edge_hi); null / -1 = no neighbour on that side
  double *zsend_lo, *zsend_hi;
  int edge_lo, edge_hi;
  int reverse;            // walk the tiles in descending order
  double* cpart;          // two-level mode (k_coarse.hip): per tile, the sums of the (updated) r over its fluid cells by coarse column: [tile][3]; multilevel mode (k_mg_cycle.hip): [tile][MG_PART = 72] = [group][row slot][column slot] (k_mg.h)
  int cshift;             // two-level mode: log2 of the coarse cell width in grid cells (the multilevel mode's node spacing is the constant MG_G0: nothing reads this there)
  int cmode, cnx, cny;    // cmode 2: the multilevel mode's bilinear restriction onto cnx x cny nodes of level 0
  // RECOMP (k_precond_tile<16, true>): `as` is the search direction s' itself and the pass forms A s' from it.  On row slabs the rows across
  // the slab boundary are the compact ghost rows of s' that k_search_apply SLAB 2 keeps (indexed by the column); null = no neighbouring slab
  const double *gs_lo, *gs_hi;
  // W == 16, one GPU (tile_z_recompute): how z leaves the pass and what it tells the solve's flag PcgScalars::zfix.  -1: stored whole, the flag is left alone;
  // 0: stored whole, flag cleared; 1: "z halo only" - only what the next k_search_apply<.., ZR> cannot form itself goes to zhalo / zrows (ZrArgs), flag set;
  // 2: the end of a solve: runs only where the flag is set (z is then M^-1 of the r in memory: nothing has touched r since) and stores z whole, flag cleared
  int zform;
  double *zhalo, *zrows;
};

// one cell of the E^-1 recurrence (main.c:586-600): own / nbv = precon of the left / lower neighbour
__device__ __forceinline__ double factor_step(double aa, double own, double nbv) {
  const double cl = -1.0 * own, cb = -1.0 * nbv;
  double e = aa - cl * cl - cb * cb;
  if (e < 0.25 * aa) e = (aa != 0.0) ? aa : 1.0;
  return 1.0 / sqrt(e);
}

// sums over aligned groups of lanes: two quad permutes (and the mirror of the half row), fixed order
template <int CTRL>
__device__ __forceinline__ double dpp_move(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double group_sum(double v) {      // over an aligned group of MG_LG lanes (k_mg.h), in every lane of it
  v = v + dpp_move<0xB1>(v);       // quad_perm [1, 0, 3, 2]
  v = v + dpp_move<0x4E>(v);       // quad_perm [2, 3, 0, 1]
  if (MG_LG == 8) v = v + dpp_move<0x141>(v);      // row_half_mirror
  return v;
}
#endif  // __HIPCC__
