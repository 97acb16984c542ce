// k_mg_split.hip — row slabs: the multilevel preconditioner's cycle split by rows (round 5).
// Replicated, the cycle costs every rank the whole of it and an all-gather of level 0's right-hand side (cells / 64 doubles: 32 MB at 16384^2) per iteration.  Split:
//   * the way DOWN is linear, so a rank takes what ITS tiles contribute (zero elsewhere) down to the gather level Lg (the first of <= MG_GATHER_MAX nodes) on the rows that
//     share can reach, and the ranks all-gather WINDOWS of that level (own rows + a few): k_mg_split_unpack adds them up in rank order - the same bits everywhere;
//   * from Lg to the dense level and back to Lg everything runs replicated as before (small);
//   * the way back UP below Lg needs the TRUE right-hand sides on a rank's rows and their halo: the neighbours' shares on those rows (ZONES) travel with the edge rows of z
//     in the same neighbour exchange, and every rank computes levels Lg - 1 .. 0 for its own rows (+ 1) only;
//   * the correction's share of dot(z, r), x_0 . rhs_0, then lives on the ranks' own rows: ONE more 5-double all-gather behind the cycle (beta cannot wait for the next
//     exchange point) - three exchange points per iteration instead of two, for a level 0 of 1 / ranks the work and an all-gather of kilobytes.
// Needs every zone to reach into the NEXT rank only (slabs of a few bands); else - and on small grids, where level 0 is the gather level - the replicated form runs.
// Which rows of which level a rank packs, sends, receives, overwrites and sums is plain C, eu_mg_split_plan_fill (euler_host.c; tests/test_mg_split_host.py); the kernels
// here run through the cycle's own launchers (k_mg.h, k_mg_cycle.hip) and the setup's (k_mg.hip).
#include "k_pcg.h"

struct MgSplitSeg { int level, row0, row1, off; };      // behind the exchange: rows of a level's right-hand side that change (a neighbour's share arrives, or leftovers must go)
struct MgSplitDst {
  int nseg, total, X;
  MgSplitSeg seg[4 * MG_MAXLEV];
  int own[MG_MAXLEV][2], zr[2][MG_MAXLEV][2], zoff[2][MG_MAXLEV];
};
struct MgSplitMsg { int rows[2][MG_MAXLEV][2], off[2][MG_MAXLEV]; int Lg, X, zone; };
struct MgSplitWin { int n; int lo[64], hi[64]; };
static_assert(MG_SPLIT_MAXR == 64 && sizeof(MgSplitSeg) == sizeof(eu_mg_seg), "the kernels' records are filled from the plan");
struct MgSplitState {
  int valid;                // 1: every rank runs the split cycle
  eu_mg_split_plan P;
  int zone_doubles;         // the (uniform) length of a zone message: the most over the ranks
  MgSplitDst D;
  MgSplitMsg M;
  MgSplitWin W;
  double* msg;      // [4][X + zone]: send lo / hi, receive lo / hi
  double* gc;       // [ranks][1 + MG_NULL_MAX]: {x_0 . rhs_0 over the own rows, gauge sums}
  // the operators, per solve (eu_mg_setup): every level below the gather level is formed where it is OWNED (P.O) and MG_SETUP_HALO rows travel to either neighbour, level by
  // level; the gather level's owned rows are all-gathered
  int setup_ok;
  double* sbuf;     // [4][9 (MG_SETUP_HALO + 1) nx_0]
  double* abuf;     // [ranks][aslot]
};
static inline MgSplitState* mg_split_state(const euler_sim* S) { return static_cast<MgSplitState*>(S->mg_split); }

static void mg_split_free(euler_sim* S, MgSplitState* st) {
  eu_dev_free_group(S, EU_MEM_SPLIT);
  st->msg = st->gc = st->sbuf = st->abuf = nullptr;
}
// the sum over the ranks of n doubles, through the scratch of the cycle's partials (rewritten by the next cycle)
static bool mg_split_agree(euler_sim* S, double* v, int n) {
  double* dv = S->mg_dot;
  return hipMemcpyAsync(dv, v, n * sizeof(double), hipMemcpyHostToDevice, S->stream) == hipSuccess && S->bulk.allreduce(S->bulk.ctx, dv, n, 1) == 0 &&
         hipMemcpyAsync(v, dv, n * sizeof(double), hipMemcpyDeviceToHost, S->stream) == hipSuccess && hipStreamSynchronize(S->stream) == hipSuccess;
}
static const eu_mg_split_plan* mg_split_plan(euler_sim* S) {
  if (S->mg_split) return mg_split_state(S)->valid ? &mg_split_state(S)->P : nullptr;
  MgSplitState* st = new (std::nothrow) MgSplitState();
  if (!st) return nullptr;
  S->mg_split = st;
  eu_mg_split_plan& P = st->P;
  const int R = S->bulk.nranks, me = S->bulk.rank, Lg = eu_mg_gather_level(S->mg_levels, S->mg_nx, S->mg_ny, S->opt[EULER_OPT_MG_SPLIT_LEVEL]);
  if (!S->has_comm || !S->slab_on || S->p2p_on || R > MG_SPLIT_MAXR || R < 2 || Lg < 1 || !S->mg_a) return nullptr;
  const bool planned = eu_mg_split_plan_fill(&P, S->mg_levels, S->mg_nx, S->mg_ny, Lg, R, me, S->part_lo, S->part_hi, 4 * MG_MAXLEV) == EULER_OK;
  // every rank must come to the same verdict and the same message length: the plan's inputs are the partition (the same everywhere), so one all-reduce of {failed, zone} settles both
  double v[3] = {!planned || P.beyond ? 1.0 : 0.0, (double)P.zone, (double)P.setup_bad};
  if (!mg_split_agree(S, v, 3) || v[0] != 0.0) return nullptr;
  st->zone_doubles = (int)v[1];
  st->setup_ok = v[2] == 0.0;
  // what the kernels either side of the exchange need of the plan
  const int X = S->X;
  MgSplitMsg& M = st->M;
  M.Lg = Lg; M.X = X; M.zone = st->zone_doubles;
  MgSplitDst& D = st->D;
  D.nseg = P.nseg; D.total = P.total; D.X = X;
  for (int k = 0; k < P.nseg; ++k) D.seg[k] = MgSplitSeg{P.seg[k].level, P.seg[k].row0, P.seg[k].row1, P.seg[k].off};
  for (int side = 0; side < 2; ++side)
    for (int l = 0; l < MG_MAXLEV; ++l) {
      M.rows[side][l][0] = P.zs[side][l][0]; M.rows[side][l][1] = P.zs[side][l][1]; M.off[side][l] = P.zoff_s[side][l];
      if (l >= Lg) continue;
      D.own[l][0] = P.I[l][me][0]; D.own[l][1] = P.I[l][me][1];
      D.zr[side][l][0] = P.zr[side][l][0]; D.zr[side][l][1] = P.zr[side][l][1]; D.zoff[side][l] = P.zoff_r[side][l];
    }
  MgSplitWin& W = st->W;
  W.n = R;
  for (int r = 0; r < R; ++r) { W.lo[r] = P.I[Lg][r][0]; W.hi[r] = P.I[Lg][r][1]; }
  int local_fail = P.overflow;      // what can fail on ONE rank (the segment table, the allocations): settled by a second all-reduce, so that every rank runs the same cycle
  const size_t mlen = (size_t)X + st->zone_doubles;
  if (eu_dalloc(S, &st->msg, 4 * mlen, EU_MEM_SPLIT, EU_DEV_QUIET) || eu_dalloc(S, &st->gc, (size_t)R * (1 + MG_NULL_MAX), EU_MEM_SPLIT, EU_DEV_QUIET) ||
      hipMemsetAsync(st->msg, 0, 4 * mlen * sizeof(double), S->stream) != hipSuccess || hipMemsetAsync(st->gc, 0, (size_t)R * (1 + MG_NULL_MAX) * sizeof(double), S->stream) != hipSuccess ||
      (st->setup_ok && (eu_dalloc(S, &st->sbuf, 4 * (size_t)9 * (MG_SETUP_HALO + 1) * S->mg_nx[0], EU_MEM_SPLIT, EU_DEV_QUIET) ||
                        eu_dalloc(S, &st->abuf, (size_t)R * P.aslot, EU_MEM_SPLIT, EU_DEV_QUIET) ||
                        hipMemsetAsync(st->sbuf, 0, 4 * (size_t)9 * (MG_SETUP_HALO + 1) * S->mg_nx[0] * sizeof(double), S->stream) != hipSuccess ||
                        hipMemsetAsync(st->abuf, 0, (size_t)R * P.aslot * sizeof(double), S->stream) != hipSuccess))) {
    local_fail = 1;
  }
  // A rank that failed here alone would run the replicated cycle (two exchange points, an all-reduce of A_0) against the others' split cycle (three, halo + all-gather):
  // mismatched collectives, a hang.  One more all-reduce (once per plan): every rank takes the split cycle or none does.
  double lf = (double)local_fail;
  if (!mg_split_agree(S, &lf, 1)) lf = 1.0;
  if (lf != 0.0) {
    if (local_fail) eu_set_error("the split cycle's segment table or message buffers could not be set up on this rank; every rank falls back to the replicated cycle");
    mg_split_free(S, st);
    return nullptr;
  }
  st->valid = 1;
  S->opt[EULER_OPT_MG_SPLIT_ACTIVE] = Lg;
  return &P;
}
bool eu_mg_split(euler_sim* S) { return eu_is_mg(S) && mg_split_plan(S) != nullptr; }
bool eu_mg_split_setup(euler_sim* S) { return mg_split_plan(S) != nullptr && mg_split_state(S)->setup_ok; }
int eu_mg_split_nsmall(euler_sim* S) { return mg_split_state(S)->P.nsmall; }
int eu_mg_split_count(euler_sim* S) { return S->X + mg_split_state(S)->zone_doubles; }
double* eu_mg_split_msg(euler_sim* S, int k) { return mg_split_state(S)->msg + (size_t)k * ((size_t)S->X + mg_split_state(S)->zone_doubles); }
double* eu_mg_split_gc(euler_sim* S) { return mg_split_state(S)->gc; }
void eu_mg_split_release(euler_sim* S) {
  MgSplitState* st = mg_split_state(S);
  if (!st) return;
  mg_split_free(S, st);
  delete st;
  S->mg_split = nullptr;
  S->opt[EULER_OPT_MG_SPLIT_ACTIVE] = 0;
}

// pack: this rank's share on the rows a neighbour needs (ZONES) behind the edge row of z that k_precond_tile wrote into the message; its window of the gather level into
// its slot of the all-gather
__global__ __launch_bounds__(256) void k_mg_split_pack(MgHier H, MgSplitMsg M, double* __restrict__ msg_lo, double* __restrict__ msg_hi, double* __restrict__ slot, int w0, int w1, int win_rows) {
  const int side = blockIdx.y;      // 0 / 1: the messages; 2: the window
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (side == 2) {
    const int nx = H.nx[M.Lg];
    if (i >= (size_t)win_rows * nx) return;
    const int row = w0 + (int)(i / nx);
    slot[2 + i] = row < w1 ? H.rhs[H.off[M.Lg] + (size_t)row * nx + i % nx] : 0.0;
    return;
  }
  double* msg = side == 0 ? msg_lo : msg_hi;
  const size_t e = i;
  if (e >= (size_t)M.zone) return;
  double v = 0.0;
  for (int l = 0; l < M.Lg; ++l) {
    const size_t n = (size_t)(M.rows[side][l][1] - M.rows[side][l][0]) * H.nx[l];
    if (e >= (size_t)M.off[side][l] && e < (size_t)M.off[side][l] + n) { v = H.rhs[H.off[l] + (size_t)M.rows[side][l][0] * H.nx[l] + (e - M.off[side][l])]; break; }
  }
  msg[M.X + e] = v;
}
// unpack: (y = 0) the rows of D's segments become TRUE right-hand sides: this rank's share where its tiles reach (elsewhere the memory holds leftovers), + the lower neighbour's,
// + the upper one's - in that order; (y = 1, 2) the neighbours' edge rows of z into the compact rows k_search_apply reads; (y = 3) the gather level, whole, from the ranks'
// windows in rank order
__global__ __launch_bounds__(256) void k_mg_split_unpack(MgHier H, MgSplitDst D, int Lg, const double* __restrict__ msg_lo, const double* __restrict__ msg_hi, double* __restrict__ zlo,
                                                         double* __restrict__ zhi, const double* __restrict__ xbuf, int slotlen, MgSplitWin W) {
  const int what = blockIdx.y;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (what == 3) {
    const int nx = H.nx[Lg];
    if (i >= (size_t)nx * H.ny[Lg]) return;
    const int row = (int)(i / nx);
    double t = 0.0;
    for (int r = 0; r < W.n; ++r)
      if (row >= W.lo[r] && row < W.hi[r]) t = t + xbuf[(size_t)r * slotlen + 2 + (size_t)(row - W.lo[r]) * nx + i % nx];
    H.rhs[H.off[Lg] + i] = t;
    return;
  }
  if (what == 1) { if (zlo && i < (size_t)D.X) zlo[i] = msg_lo[i]; return; }
  if (what == 2) { if (zhi && i < (size_t)D.X) zhi[i] = msg_hi[i]; return; }
  if (i >= (size_t)D.total) return;
  for (int k = 0; k < D.nseg; ++k) {
    const MgSplitSeg& s = D.seg[k];
    const int l = s.level, nx = H.nx[l];
    const size_t n = (size_t)(s.row1 - s.row0) * nx;
    if (i < (size_t)s.off || i >= (size_t)s.off + n) continue;
    const size_t e = i - s.off;
    const int row = s.row0 + (int)(e / nx), col = (int)(e % nx);
    double* dst = H.rhs + H.off[l] + (size_t)row * nx + col;
    double v = (row >= D.own[l][0] && row < D.own[l][1]) ? *dst : 0.0;
    if (row >= D.zr[0][l][0] && row < D.zr[0][l][1]) v = v + msg_lo[D.X + D.zoff[0][l] + (size_t)(row - D.zr[0][l][0]) * nx + col];
    if (row >= D.zr[1][l][0] && row < D.zr[1][l][1]) v = v + msg_hi[D.X + D.zoff[1][l] + (size_t)(row - D.zr[1][l][0]) * nx + col];
    *dst = v;
    return;
  }
}
// behind the cycle: the ranks' {x_0 . rhs_0 over their own rows, gauge sums} -> dot(z, r) with its epilogue; the gauge of cut-off regions on this rank's rows
__global__ __launch_bounds__(256) void k_mg_split_fold(PcgScalars* sc, const double* __restrict__ vals, int R, int fin_op, int force, MgHier H, const double* __restrict__ nullv, const double* __restrict__ n0,
                                                       size_t nstride, const double* __restrict__ m0, int row0, int row1) {
  const bool idle = !force && pcg_idle(sc);
  if (idle) return;
  const int n_null = (int)nullv[MG_NULL_MAX * 256];
  const size_t n0n = (size_t)H.nx[0] * H.ny[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double v = 0.0;
    for (int r = 0; r < R; ++r) v += vals[(size_t)r * (1 + MG_NULL_MAX)];
    v = sc->sigma_new + v;
    if (fin_op == FIN_SIGMA_INIT) sc->sigma = v;
    else if (fin_op == FIN_BETA) { sc->sigma_new = v; sc->beta = v / sc->sigma; sc->sigma = v; }
    else sc->sigma_new = v;
  }
  for (int q = 0; q < n_null && q < MG_NULL_MAX; ++q) {
    double tot = 0.0;
    for (int r = 0; r < R; ++r) tot += vals[(size_t)r * (1 + MG_NULL_MAX) + 1 + q];
    const double mn = m0[(size_t)MG_NULL_MAX * n0n + q];
    if (!(mn > 0.0)) continue;
    const double cq = tot / mn;
    const size_t lo = (size_t)row0 * H.nx[0], hi = (size_t)row1 * H.nx[0];
    for (size_t c = lo + (size_t)blockIdx.x * 256 + threadIdx.x; c < hi; c += (size_t)gridDim.x * 256) {
      const double nv = n0[(size_t)q * nstride + c];
      if (nv != 0.0) H.x[c] = H.x[c] - nv * cq;
    }
  }
}

// the split cycle's launches.  pre: before the G1 exchange (k_precond_tile has left the tiles' partial sums and, in the messages, the edge rows of z)
int eu_mg_split_pre(euler_sim* S) {
  MgSplitState* st = mg_split_state(S);
  const eu_mg_split_plan& P = st->P;
  const MgHier H = mg_hier(S);
  const int me = P.rank, Lg = P.Lg;
  eu_prof_begin(S, KC_COARSE_CYCLE);
  int rc = eu_mg_launch_down1(S, eu_mg_down_args(S, H, 0, 1, -1), true, P.I[1][me][0], P.I[1][me][1]);      // level 0 -> 1 from this rank's tiles
  if (rc) return rc;
  for (int lA = 1; lA < Lg;) {
    const int lB = lA + 3 < Lg ? lA + 3 : Lg;
    MgDownArgs A = eu_mg_down_args(S, H, lA, lB, -1);
    A.clip_lo = P.I[lA][me][0]; A.clip_hi = P.I[lA][me][1];
    rc = eu_mg_launch_down(S, A, false, P.I[lB][me][0], P.I[lB][me][1]);
    if (rc) return rc;
    lA = lB;
  }
  const size_t win = (size_t)P.win_rows * S->mg_nx[Lg], most = win > (size_t)st->zone_doubles ? win : (size_t)st->zone_doubles;
  const size_t mlen = (size_t)S->X + st->zone_doubles;
  hipLaunchKernelGGL(k_mg_split_pack, dim3((unsigned)((most + 255) / 256), 3), dim3(256), 0, S->stream, H, st->M, st->msg, st->msg + mlen, S->mg_xbuf + (size_t)me * P.nsmall,
                     P.I[Lg][me][0], P.I[Lg][me][1], P.win_rows);
  eu_prof_end(S, KC_COARSE_CYCLE);
  return EULER_OK;
}
// mid: behind the exchange - the true right-hand sides, the replicated middle, the way up on the own rows; leaves {x_0 . rhs_0, gauge sums} of the own rows in this rank's slot of gc
int eu_mg_split_mid(euler_sim* S, int fin_op, int force, double* zrecv_lo, double* zrecv_hi) {
  MgSplitState* st = mg_split_state(S);
  const eu_mg_split_plan& P = st->P;
  const MgHier H = mg_hier(S);
  const int me = P.rank, Lg = P.Lg, lC = eu_mg_entry_level(S->mg_levels, S->mg_nx, S->mg_ny);
  if (eu_mg_check_tail(S, "")) return EULER_EINVAL;
  eu_prof_begin(S, KC_COARSE_CYCLE);
  const size_t mlen = (size_t)S->X + st->zone_doubles, ng = (size_t)S->mg_nx[Lg] * S->mg_ny[Lg];
  size_t most = ng > (size_t)st->D.total ? ng : (size_t)st->D.total;
  if ((size_t)S->X > most) most = S->X;
  hipLaunchKernelGGL(k_mg_split_unpack, dim3((unsigned)((most + 255) / 256), 4), dim3(256), 0, S->stream, H, st->D, Lg, st->msg + 2 * mlen, st->msg + 3 * mlen, S->band_lo > 0 ? zrecv_lo : nullptr,
                     S->band_hi < S->geom.nbands ? zrecv_hi : nullptr, S->mg_xbuf, P.nsmall, st->W);
  int lA = Lg;
  do {      // replicated: the gather level down to the entry level, the tail, back up to the entry level
    const int lB = lA + 3 < lC ? lA + 3 : lC;
    MgDownArgs A = eu_mg_down_args(S, H, lA, lB, lC);
    A.force = force;
    int rc = eu_mg_launch_down(S, A, false);
    if (rc) return rc;
    lA = lB;
  } while (lA < lC);
  MgUpArgs U = eu_mg_up_args(S, H, lC, fin_op, force);
  if (lC > Lg) { MgUpArgs V = U; V.l0 = Lg; eu_mg_launch_up(S, V); }                                       // ... and to the gather level
  if (Lg > 1) { MgUpArgs V = U; V.l0 = 1; V.lC = Lg; eu_mg_launch_up(S, V, P.NX[1][0], P.NX[1][1]); }      // the own rows: levels Lg - 1 .. 1
  U.row_lo = MG_RPB * S->part_lo[me]; U.row_hi = MG_RPB * S->part_hi[me];
  U.slot = st->gc + (size_t)me * (1 + MG_NULL_MAX);
  eu_mg_launch_up0(S, U, P.NX[0][0], P.NX[0][1]);
  eu_prof_end(S, KC_COARSE_CYCLE);
  return EULER_OK;
}
// fold: behind the all-gather of gc
int eu_mg_split_fold(euler_sim* S, int fin_op, int force) {
  MgSplitState* st = mg_split_state(S);
  const eu_mg_split_plan& P = st->P;
  hipLaunchKernelGGL(k_mg_split_fold, dim3(64), dim3(256), 0, S->stream, S->sc, st->gc, P.ranks, fin_op, force, mg_hier(S), S->cc_null, S->mg_null0, (size_t)S->mg_cells, S->mg_m0, P.NX[0][0], P.NX[0][1]);
  return EULER_OK;
}

// row slabs: from this rank's tiles, the node rows [RPB band_lo - 1, RPB band_hi + 1) of level 0's right-hand side (clipped to the grid) into `dst`
__global__ __launch_bounds__(256) void k_mg_gather_rows(const double* __restrict__ part, double* __restrict__ dst, int nx0, int row0, int row1, int ntb, int band_lo, int band_hi) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= nx0 * (row1 - row0)) return;
  dst[k] = mg_gather0(part, row0 + k / nx0, k % nx0, ntb, band_lo, band_hi);
}
int eu_mg_slab_rows(euler_sim* S) {
  const int ny0 = S->mg_ny[0];
  const int row0 = MG_RPB * S->band_lo - 1 < 0 ? 0 : MG_RPB * S->band_lo - 1, row1 = MG_RPB * S->band_hi + 1 > ny0 ? ny0 : MG_RPB * S->band_hi + 1;
  const int cells = (row1 - row0) * S->mg_nx[0];
  if (cells > 0)
    LAUNCH(S, KC_COARSE_CYCLE, k_mg_gather_rows, dim3((cells + 255) / 256), dim3(256), S->mg_part, S->mg_xbuf + (size_t)S->bulk.rank * S->mg_xslot + 2, S->mg_nx[0], row0, row1, S->geom.T / 16,
           S->band_lo, S->band_hi);
  return EULER_OK;
}

// rows of a level's nine planes <-> a message (plane-major there too); mode 0: pack, 1: unpack (replace), 2: unpack, adding on the rows [add0, add1) (level 0: both ranks'
// cells reach the node rows at a slab boundary; the entries are small multiples of 2^-12, their sums exact)
__global__ __launch_bounds__(256) void k_mg_sten_rows(double* __restrict__ a, size_t n, int nx, int row0, int rows, double* __restrict__ msg, int mode, int add0, int add1) {
  const size_t per = (size_t)rows * nx, i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= 9 * per) return;
  const size_t k = i / per, e = i % per;
  double* cell = a + k * n + (size_t)row0 * nx + e;
  if (mode == 0) msg[i] = *cell;
  else {
    const int row = row0 + (int)(e / nx);
    *cell = (mode == 2 && row >= add0 && row < add1) ? *cell + msg[i] : msg[i];
  }
}
// the gather level's operator, whole, from the owners' rows
struct MgOwners { int n; int lo[64], hi[64]; };
__global__ __launch_bounds__(256) void k_mg_sten_gathered(double* __restrict__ a, size_t n, int nx, const double* __restrict__ abuf, int aslot, MgOwners W) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= 9 * n) return;
  const size_t k = i / n, c = i % n;
  const int row = (int)(c / nx);
  for (int r = 0; r < W.n; ++r)
    if (row >= W.lo[r] && row < W.hi[r]) { a[i] = abuf[(size_t)r * aslot + k * (size_t)(W.hi[r] - W.lo[r]) * nx + (size_t)(row - W.lo[r]) * nx + c % nx]; return; }
}
int eu_mg_setup_split(euler_sim* S) {
  MgSplitState* st = mg_split_state(S);
  const eu_mg_split_plan& P = st->P;
  const int me = P.rank, R = P.ranks, Lg = P.Lg, nx0 = S->mg_nx[0];
  const size_t n0 = (size_t)nx0 * S->mg_ny[0];
  const int s0 = P.I[0][me][0], s1 = P.I[0][me][1];      // the rows this rank's tiles reach
  HIPCHK(hipMemset2DAsync(S->mg_a0i + (size_t)s0 * nx0, n0 * sizeof(unsigned long long), 0, (size_t)(s1 - s0) * nx0 * sizeof(unsigned long long), 9, S->stream));
  int rc = eu_mg_assemble0(S, (size_t)s0 * nx0, (size_t)(s1 - s0) * nx0);
  if (rc) return rc;
  const size_t blen = (size_t)9 * (MG_SETUP_HALO + 1) * nx0;
  double *send_lo = st->sbuf, *send_hi = st->sbuf + blen, *recv_lo = st->sbuf + 2 * blen, *recv_hi = st->sbuf + 3 * blen;
  const bool has_lo = me > 0, has_hi = me + 1 < R;
  for (int l = 0; l <= Lg; ++l) {
    const int nx = S->mg_nx[l], ny = S->mg_ny[l], o0 = P.O[l][me][0], o1 = P.O[l][me][1];
    double* a = S->mg_a + 9 * S->mg_off[l];
    const size_t n = (size_t)nx * ny;
    if (l > 0 && o1 > o0) eu_mg_coarsen(S, l, o0, o1);
    if (l == Lg) break;
    // the rows either neighbour needs of this rank / this rank of them: MG_SETUP_HALO owned rows; level 0 one more - the shared row across the boundary, as a share
    const int extra = l == 0 ? 1 : 0, rows = MG_SETUP_HALO + extra;
    const unsigned nb = (unsigned)(((size_t)9 * rows * nx + 255) / 256);
    if (has_lo) hipLaunchKernelGGL(k_mg_sten_rows, dim3(nb), dim3(256), 0, S->stream, a, n, nx, o0 - extra, rows, send_lo, 0, 0, 0);
    if (has_hi) hipLaunchKernelGGL(k_mg_sten_rows, dim3(nb), dim3(256), 0, S->stream, a, n, nx, o1 - MG_SETUP_HALO, rows, send_hi, 0, 0, 0);
    COMM_CALL(S->bulk.halo(S->bulk.ctx, send_lo, send_hi, recv_lo, recv_hi, 9 * rows * nx));
    if (has_lo) hipLaunchKernelGGL(k_mg_sten_rows, dim3(nb), dim3(256), 0, S->stream, a, n, nx, o0 - MG_SETUP_HALO, rows, recv_lo, l == 0 ? 2 : 1, s0, s1);
    if (has_hi) hipLaunchKernelGGL(k_mg_sten_rows, dim3(nb), dim3(256), 0, S->stream, a, n, nx, o1 - extra, rows, recv_hi, l == 0 ? 2 : 1, s0, s1);
  }
  {      // the gather level: the owners' rows to everybody
    const int nx = S->mg_nx[Lg], o0 = P.O[Lg][me][0], o1 = P.O[Lg][me][1];
    const size_t n = (size_t)nx * S->mg_ny[Lg];
    double* a = S->mg_a + 9 * S->mg_off[Lg];
    if (o1 > o0) hipLaunchKernelGGL(k_mg_sten_rows, dim3((unsigned)(((size_t)9 * (o1 - o0) * nx + 255) / 256)), dim3(256), 0, S->stream, a, n, nx, o0, o1 - o0, st->abuf + (size_t)me * P.aslot, 0, 0, 0);
    int64_t off[64], cnt[64];
    for (int r = 0; r < R; ++r) { off[r] = (int64_t)8 * P.aslot * r; cnt[r] = (int64_t)8 * P.aslot; }
    COMM_CALL(S->bulk.allgather(S->bulk.ctx, st->abuf, off, cnt));
    MgOwners W;
    W.n = R;
    for (int r = 0; r < R; ++r) { W.lo[r] = P.O[Lg][r][0]; W.hi[r] = P.O[Lg][r][1]; }
    hipLaunchKernelGGL(k_mg_sten_gathered, dim3((unsigned)((9 * n + 255) / 256)), dim3(256), 0, S->stream, a, n, nx, st->abuf, P.aslot, W);
  }
  int i0 = P.O[0][me][0] - MG_SETUP_HALO, i1 = P.O[0][me][1] + MG_SETUP_HALO;
  if (i0 < 0) i0 = 0;
  if (i1 > S->mg_ny[0]) i1 = S->mg_ny[0];
  eu_mg_setup_tail(S, Lg + 1, i0, i1);
  return EULER_OK;
}
