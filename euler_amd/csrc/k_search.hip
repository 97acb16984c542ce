// k_search.hip — the apply_a pass of a tile-local PCG iteration: s' = z + beta s, A s' and dot(s', A s') in one launch (k_search_apply), with p += alpha s riding along.
#include "k_pcg.h"

#include <type_traits>

// update_search (main.c:669-677) of one iteration fused into apply_a (main.c:679-691) of the next:
//     s' = z + beta s   and   out = A s'   in one pass, out going to a scratch array (the forward solve's q, dead here).
// A cell needs s' of its four neighbours, which it recomputes from z and the old s (the same expression its owner
// evaluates: identical bits) - hence s' goes to a SECOND array, or a neighbour could read a half-updated s.
// Saves a launch and 9 bytes per cell and iteration.  Same pair-per-thread structure as k_apply_a.
// Several ranks (row slabs): the cells across a slab boundary belong to the neighbouring rank, and so do their z and s.
// With the neighbours' arrays mapped (comm_p2p.hip) the kernel reads those two values where they live - a handful of
// system-scope loads over xGMI for the lanes on the slab's edge rows - and forms the neighbour's s' with the owner's
// expression.  No ghost-row exchange, no extra launch: every rank's z is final before anyone gets here (the all-reduce
// behind dot(z,r) separates the backward sweeps from this kernel) and nobody overwrites z or the old s before the
// all-reduce at the end of this kernel.
// PMODE (tile-local mode, where no other kernel of the iteration touches p - k_precond_tile does the rest of main.c:753-765):
//   1  tile-local mode, an odd iteration: p is left alone
//   N = 2, 4, 8  an iteration k >= N, k a multiple of N: p = (..(p + alpha_(k-N) s_(k-N)) + ..) + alpha_(k-1) s_(k-1) - the N fmadds of
//      main.c:753 that are due, in their order, hence the reference's bits.  s_(k-1) is this pass's s_old; s_(k-N) sits in the array the
//      pass is about to overwrite with s_k (the search directions turn through a ring of N arrays), read by the thread that overwrites
//      it; the N - 2 in between come from `hist`.  p is read and written every N-th iteration: (2 w + (N - 1) w) / N bytes per cell and
//      iteration - 12 (N = 2, rounds 3-4), 10 (N = 4), 9 (N = 8) instead of 16.
//
// Schedule.  A wave walks a run of SA_RUN consecutive pair-records of one band (lane = row) with a three-deep window of s'
// in registers - the pair before, the pair itself, the pair after - so every element of z and s is loaded ONCE, by one
// 16-byte access per lane, and the four neighbours of a cell come out of the window: left / right are the lane's own
// registers, down / up the neighbouring lane's by a DPP wave shift (the band-skewed layout puts the lower / upper row's
// value of the same column one record earlier / later in the neighbouring lane).  Only lane 0 / lane 63 look outside
// their band (two lanes of one 8-byte load each per element).  Against one thread per pair gathering six neighbours with
// twelve strided 8-byte loads (round 1) that is 11 instead of 19 memory instructions per pair, and the HBM traffic drops
// from 1.28x to the algorithmic bytes.
//
// INTERIOR chunks (EU_CHUNK_INTERIOR in the list entry: every cell fluid, four fluid neighbours, a_diag 4 - most of a deep tank)
// take a second instantiation of the run body with the masks as compile-time constants: no mask loads, no selects.
#define SA_THREADS 256
struct SaPair { sw_d2 z, so; double ez0, es0, ez1, es1; };   // one pair-record of a lane + the out-of-band vertical neighbours of its two elements

// SA_RUN pair-records per wave: 8 (more waves in flight - at 1024^2 runs of 32 would leave 300 waves for 256 CUs - and the granularity
// of the active-chunk list); 16 / 32 remain for experiments (sa_run)
// COARSE (two-level preconditioner, k_coarse.hip): z stands for z + P y wherever s' = z + beta s is formed - y of the cell's coarse
// cell is looked up (a lane's columns of one run cross at most one coarse column boundary) and added first, like the oracle's z += P y.
__device__ __forceinline__ double pick3(int t, int tb1, int tb2, double v0, double v1, double v2) {
  double v = v0;
  v = t >= tb1 ? v1 : v;
  v = t >= tb2 ? v2 : v;
  return v;
}
// STORE false: A s' is not stored (`out` is ignored) - k_precond_tile<16, true> forms it again from s' instead of reading it back
// COARSE 2 (multilevel preconditioner, k_mg.hip; x_0 is the result of the cycle, k_mg_cycle.hip): z + P_0 x_0 with P_0 bilinear from the level-0 nodes - the lane combines its two node rows once per run (four node columns
// cover the run and its window), every cell then interpolates along its row; the expression is mg_interp0's, so a cell gets the same bits whoever forms its s'.
// ZR (SLAB 0, SA_RUN 8, the list of active chunks; k_pcg.h tile_z_recompute): z is formed again from r by the run's own tile solve (tile_solve, E^-1 from the
// LDS table for interior chunks as in k_precond_tile) - the previous k_precond_tile stored only what the neighbouring tiles' z contributes (ZrArgs)
template <int SLAB, int PMODE, int SA_RUN, int COARSE = 0, bool STORE = true, bool ZR = false>   // SLAB 1: several ranks, the neighbouring slabs' arrays are mapped; 2: their edge rows as compact rows (nbr); 0: nbr is ignored
// (multilevel mode, one GPU, seven of eight passes: four waves per SIMD - 128 registers, one of them spilled - since the lanes' level-0 node values live in LDS: 212 -> 197 us at 8192^2;
// forced onto the 150 registers of the select-chain form the same bound cost 100 bytes of scratch and 288 us)
// (the tile-local mode's pass has 98 registers, four waves; squeezed to 96 for five - 12 bytes of scratch - it takes 180 us instead of 169)
__global__ __launch_bounds__(SA_THREADS, (COARSE == 2 && PMODE == 1 && SLAB == 0) ? 4 : 1) void k_search_apply(const double* __restrict__ s_old, const double* __restrict__ z,
                                                             double* __restrict__ s_new, double* __restrict__ out,
                                                             const uint8_t* __restrict__ mask, SkewGeom g,
                                                             double* __restrict__ partial, PcgScalars* sc, int force,
                                                             unsigned int* counter, int fin_op, SlabNeighbours nbr,
                                                             double* __restrict__ p, double* s_new_base, double* s_old_base,
                                                             const unsigned int* __restrict__ chunk_list,      // SA_RUN == 8 only: the solve's active runs
                                                             CoarseRef cref, SaHist hist, ZrArgs zr) {
  static_assert(PMODE == 1 || PMODE == 2 || PMODE == 4 || PMODE == 8, "PMODE: p is left alone (1) or takes the N fmadds that are due (the ring's length)");
  static_assert(!ZR || (SLAB == 0 && SA_RUN == 8 && COARSE == 0), "ZR: one GPU, runs of one tile, no coarse part");
  __shared__ double s_cy[COARSE == 2 ? SA_THREADS / 64 : 1][COARSE == 2 ? MG_NI + 1 : 1][64];      // multilevel mode: a lane's node values of the run (own row / the row across the band boundary)
  __shared__ double s_ce[COARSE == 2 ? SA_THREADS / 64 : 1][COARSE == 2 ? MG_NI + 1 : 1][64];
  if (!force && pcg_idle(sc)) return;
  __shared__ sw_d2 s_ztab[ZR ? 8 : 1][64];      // ZR: E^-1 of an interior tile (k_tile_table), as k_precond_tile keeps it
  if (ZR) {
    for (int k = threadIdx.x; k < 8 * 64; k += SA_THREADS) (&s_ztab[0][0])[k] = reinterpret_cast<const sw_d2*>(zr.table)[k];
    __syncthreads();
  }
  const double beta = sc->beta;
  (void)s_new_base; (void)s_old_base;
  // PMODE N: alpha of the iterations k - N .. k - 1 (k = the iterations counted so far: this launch's own alpha is written by its LAST block)
  constexpr int NPA = PMODE >= 2 ? PMODE : 2;
  double al[NPA] = {};
  if (PMODE >= 2) {
    const int k = sc->iters;
#pragma unroll
    for (int j = 0; j < NPA; ++j) al[j] = sc->alpha_hist[(k - NPA + j) & 7];
  }
  const int lane = threadIdx.x & 63;
  const int TS = g.TS, npairs = TS / 2;
  const int nb_local = (int)(g.S / ((size_t)TS * 64));
  const int cpb = (npairs + SA_RUN - 1) / SA_RUN, total = nb_local * cpb;
  const int n_waves = gridDim.x * (SA_THREADS / 64);
  const bool edge_lane = lane == 0 || lane == 63;
  double t = 0.0;
  // with the list of active chunks (euler_dev.h) a wave never visits an empty run, and a run's masks are loaded with its data
  const bool listed = chunk_list != nullptr;
  const int ntb16 = g.T / 16;
  const int todo = listed ? (int)sc->n_chunks : total;
  typedef std::integral_constant<bool, true> yes_t;
  typedef std::integral_constant<bool, false> no_t;
  for (int i = blockIdx.x * (SA_THREADS / 64) + (threadIdx.x >> 6); i < todo; i += n_waves) {
    int c = i, per = cpb;
    bool interior = false;
    if (listed) { const unsigned int ent = chunk_list[i]; interior = (ent & EU_CHUNK_INTERIOR) != 0; c = (int)(ent & ~EU_CHUNK_INTERIOR); per = ntb16; }
    const int lb = c / per, P0 = (c % per) * SA_RUN, P1 = ZR ? P0 + SA_RUN : (P0 + SA_RUN < npairs ? P0 + SA_RUN : npairs);      // (ZR: a listed tile ends below T < TS)
    const size_t bbase = (size_t)lb * TS * 64 + 2 * lane;     // element (band, record 0, lane)
    auto run = [&](auto full_tag) {
      constexpr bool FULL = decltype(full_tag)::value;
      // the cell masks of the run; a run without fluid is skipped whole
      unsigned int mm[SA_RUN];
      unsigned int any = 0;
#pragma unroll
      for (int j = 0; j < SA_RUN; ++j) {
        if (FULL) mm[j] = CM_INTERIOR | (CM_INTERIOR << 8);
        else mm[j] = P0 + j < P1 ? (unsigned int)*reinterpret_cast<const unsigned short*>(mask + bbase + (size_t)(P0 + j) * 128) : 0u;
        any |= mm[j];
      }
      if (!FULL && !listed && !__ballot(((any | (any >> 8)) & CM_FLUID) != 0)) return;
      // ZR: z of the run's tile from r, the same bits as the k_precond_tile that updated r
      sw_d2 zz[ZR ? SA_RUN : 1];
      if (ZR) {
        sw_d2 rr[SA_RUN], pp[SA_RUN];
#pragma unroll
        for (int j = 0; j < SA_RUN; ++j) {
          rr[j] = *reinterpret_cast<const sw_d2*>(zr.r + bbase + (size_t)(P0 + j) * 128);
          pp[j] = FULL ? s_ztab[j][lane] : *reinterpret_cast<const sw_d2*>(zr.pre + bbase + (size_t)(P0 + j) * 128);
        }
        double none = 0.0;
        tile_solve<2 * SA_RUN, false>(mm, rr, pp, zz, none);
      }
      const int ztile = P0 / SA_RUN;      // ZR: the run's tile within its band
      // where lane 0 / lane 63 find the row below / above their band (the adjacent band's lane 63 / lane 0), relative to pair 0:
      // even element (record 2P):  below = record 2P + 63 of band - 1, above = record 2P - 63 of band + 1; odd element: + 1
      const bool up_remote = SLAB == 1 && nbr.z_up && lb + 1 == nb_local, dn_remote = SLAB == 1 && nbr.z_dn && lb == 0;
      const double* ez = lane == 0 ? (dn_remote ? nbr.z_dn : z) : (up_remote ? nbr.z_up : z);
      const double* es = lane == 0 ? (dn_remote ? nbr.s_dn : s_old) : (up_remote ? nbr.s_up : s_old);
      const bool remote = lane == 0 ? dn_remote : up_remote;
      const long long e0_base = lane == 0 ? ((long long)(lb - 1) * TS + 62) * 64 + 127 : ((long long)(lb + 1) * TS - 64) * 64 + 1;
      const long long e1_base = lane == 0 ? ((long long)(lb - 1) * TS + 64) * 64 + 126 : ((long long)(lb + 1) * TS - 62) * 64;
      const unsigned int vbit = lane == 0 ? CM_DOWN : CM_UP;
      // SLAB 2: lane 0 of the slab's first band / lane 63 of its last one find the row across the slab boundary in the compact
      // rows, at the cell's column: even element (record 2P) of lane 0 sits in column 2P, of lane 63 in column 2P - 63
      const bool ghost = SLAB == 2 && (lane == 0 ? (nbr.zrow_dn != nullptr && lb == 0) : (nbr.zrow_up != nullptr && lb + 1 == nb_local));
      const double* gz = lane == 0 ? nbr.zrow_dn : nbr.zrow_up;
      const double* gs = lane == 0 ? nbr.srow_dn : nbr.srow_up;
      double* gsn = lane == 0 ? nbr.snew_dn : nbr.snew_up;
      const int gcol = lane == 0 ? 0 : -63;
      // ZR: the rows across the band boundary are lane 63's of the band below / lane 0's of the band above, by column (ZrArgs::rows)
      const double* zrow = ZR ? zr.rows + (long long)(lane == 0 ? 2 * lb - 1 : 2 * lb + 2) * zr.X : nullptr;
      // COARSE: this lane's columns in the run (pairs P0 - 1 .. P1: 20 records at most) start in aggregate column Ja, reach Ja + 1 at record
      // tb1 and Ja + 2 at record tb2 (aggregates of 16: three columns; of 64 and more: two); the lane's row decides the aggregate row
      double cy0 = 0.0, cy1 = 0.0, cy2 = 0.0, ce0 = 0.0, ce1 = 0.0, ce2 = 0.0;
      double (*cyv)[64] = s_cy[COARSE == 2 ? threadIdx.x >> 6 : 0];
      double (*cev)[64] = s_ce[COARSE == 2 ? threadIdx.x >> 6 : 0];
      int ctb1 = 0x7fffffff, ctb2 = 0x7fffffff, cJb = 0;
      (void)cJb;
      if (COARSE == 2) {
        // the lane's columns in the run and its window (records 2 (P0 - 1) .. 2 P1 + 1: 20 at most) lie between the node columns Jb .. Jb + MG_NI (spacing MG_G0); the column of
        // record t lies between Jb + m and Jb + m + 1 from record ctb[m] on.  Nodes beyond the grid repeat the outermost one (constant there)
        cJb = (2 * (P0 - 1) - lane - MG_G0 / 2) >> MG_LOG;
        ctb1 = MG_G0 * (cJb + 1) + lane + MG_G0 / 2;
        const int row = (cref.band0 + lb) * 64 + lane;
        const int hi_ = cref.nx - 1;
        int i0, i1;
        double fy;
        mg_cell_w(row, cref.ny, i0, i1, fy);
        const double* y0 = cref.y + (size_t)i0 * cref.nx;
        const double* y1 = cref.y + (size_t)i1 * cref.nx;
#pragma unroll
        for (int q = 0; q <= MG_NI; ++q) { const int c = cJb + q < 0 ? 0 : (cJb + q < hi_ ? cJb + q : hi_); cyv[q][lane] = mg_rows(y0[c], y1[c], fy); }
#pragma unroll
        for (int q = 0; q <= MG_NI; ++q) cev[q][lane] = 0.0;
        if (edge_lane) {      // the row across the band boundary
          const int re = row + (lane == 0 ? -1 : 1);
          if (re >= 0 && re < MG_G0 * cref.ny) {
            mg_cell_w(re, cref.ny, i0, i1, fy);
            y0 = cref.y + (size_t)i0 * cref.nx; y1 = cref.y + (size_t)i1 * cref.nx;
#pragma unroll
            for (int q = 0; q <= MG_NI; ++q) { const int c = cJb + q < 0 ? 0 : (cJb + q < hi_ ? cJb + q : hi_); cev[q][lane] = mg_rows(y0[c], y1[c], fy); }
          }
        }
      }
      // (the node values sit in LDS, [node column][lane]: a record picks its interval by arithmetic and reads two of them - conflict-free, and twenty registers fewer than arrays
      // with a chain of selects per record)
      auto p0y = [&](int t, double (*av)[64]) __attribute__((always_inline)) {      // (P_0 x_0) at the lane's column of record t, from a row's node values
        const double f = (double)((t - lane - MG_G0 / 2) & (MG_G0 - 1)) * (1.0 / MG_G0);
        int m = t >= ctb1 ? ((t - ctb1) >> MG_LOG) + 1 : 0;
        m = m < MG_NI - 1 ? m : MG_NI - 1;
        return mg_lerp_x(av[m][lane], av[m + 1][lane], f);
      };
      if (COARSE == 1) {
        const int xa = 2 * (P0 - 1) - lane, Ja = (xa > 0 ? xa : 0) >> cref.shift;
        const int row = (cref.band0 + lb) * 64 + lane;
        const size_t I = (size_t)(row >> cref.shift) * cref.nx;
        ctb1 = ((Ja + 1) << cref.shift) + lane;
        ctb2 = ((Ja + 2) << cref.shift) + lane;
        cy0 = Ja < cref.nx ? cref.y[I + Ja] : 0.0;
        cy1 = Ja + 1 < cref.nx ? cref.y[I + Ja + 1] : 0.0;
        cy2 = Ja + 2 < cref.nx ? cref.y[I + Ja + 2] : 0.0;
        if (edge_lane) {      // the row across the band boundary may belong to the neighbouring aggregate row (same columns)
          const int re = row + (lane == 0 ? -1 : 1);
          const bool inside = re >= 0 && (re >> cref.shift) < cref.ny;
          const size_t Ie = (size_t)((inside ? re : row) >> cref.shift) * cref.nx;
          ce0 = (inside && Ja < cref.nx) ? cref.y[Ie + Ja] : 0.0;
          ce1 = (inside && Ja + 1 < cref.nx) ? cref.y[Ie + Ja + 1] : 0.0;
          ce2 = (inside && Ja + 2 < cref.nx) ? cref.y[Ie + Ja + 2] : 0.0;
        }
      }
      auto load_pair = [&](int P, SaPair& d, unsigned int m) __attribute__((always_inline)) {
        d.ez0 = d.es0 = d.ez1 = d.es1 = 0.0;
        if (P < 0 || P >= npairs) { d.z = sw_d2{0.0, 0.0}; d.so = sw_d2{0.0, 0.0}; return; }   // outside the band: never a fluid cell's neighbour
        if (ZR) {      // (P - P0 is a constant once the run's loop is unrolled) the window's pairs of the neighbouring tiles: record 15 of the one before, record 0 of the one after
          const int j = P - P0;
          if (j >= 0 && j < SA_RUN) d.z = zz[j >= 0 && j < SA_RUN ? j : 0];
          else if (j < 0) d.z = sw_d2{0.0, zr.halo[((size_t)lb * ntb16 + ztile - 1) * 128 + 64 + lane]};
          else d.z = sw_d2{ztile + 1 < ntb16 ? zr.halo[((size_t)lb * ntb16 + ztile + 1) * 128 + lane] : 0.0, 0.0};
        } else {
          d.z = *reinterpret_cast<const sw_d2*>(z + bbase + (size_t)P * 128);
        }
        d.so = *reinterpret_cast<const sw_d2*>(s_old + bbase + (size_t)P * 128);
        if (edge_lane) {
          if ((m & CM_FLUID) && (m & vbit)) {
            const long long k = e0_base + (long long)P * 128;
            if (ZR) { d.ez0 = zrow[2 * P + gcol]; d.es0 = s_old[k]; }
            else if (SLAB == 2 && ghost) { d.ez0 = gz[2 * P + gcol]; d.es0 = gs[2 * P + gcol]; }
            else if (SLAB == 1 && remote) { d.ez0 = ld_system(ez + k); d.es0 = ld_system(es + k); } else { d.ez0 = ez[k]; d.es0 = es[k]; }
          }
          if (((m >> 8) & CM_FLUID) && ((m >> 8) & vbit)) {
            const long long k = e1_base + (long long)P * 128;
            if (ZR) { d.ez1 = zrow[2 * P + 1 + gcol]; d.es1 = s_old[k]; }
            else if (SLAB == 2 && ghost) { d.ez1 = gz[2 * P + 1 + gcol]; d.es1 = gs[2 * P + 1 + gcol]; }
            else if (SLAB == 1 && remote) { d.ez1 = ld_system(ez + k); d.es1 = ld_system(es + k); } else { d.ez1 = ez[k]; d.es1 = es[k]; }
          }
          if (COARSE == 1) {      // (harmless where nothing was loaded: the value is then never selected)
            d.ez0 = d.ez0 + pick3(2 * P, ctb1, ctb2, ce0, ce1, ce2);
            d.ez1 = d.ez1 + pick3(2 * P + 1, ctb1, ctb2, ce0, ce1, ce2);
          }
          if (COARSE == 2) {
            d.ez0 = d.ez0 + p0y(2 * P, cev);
            d.ez1 = d.ez1 + p0y(2 * P + 1, cev);
          }
        }
        if (COARSE == 1) {        // z + P y of the lane's own two cells (records 2P, 2P + 1)
          d.z.x = d.z.x + pick3(2 * P, ctb1, ctb2, cy0, cy1, cy2);
          d.z.y = d.z.y + pick3(2 * P + 1, ctb1, ctb2, cy0, cy1, cy2);
        }
        if (COARSE == 2) {
          d.z.x = d.z.x + p0y(2 * P, cyv);
          d.z.y = d.z.y + p0y(2 * P + 1, cyv);
        }
      };
      auto sprime = [&](const SaPair& d) __attribute__((always_inline)) { return sw_d2{d.z.x + beta * d.so.x, d.z.y + beta * d.so.y}; };   // s' = z + beta s (main.c:674)
      SaPair A, B, Cn;
      load_pair(P0 - 1, A, 0u);
      load_pair(P0, B, mm[0]);
      load_pair(P0 + 1, Cn, SA_RUN > 1 ? mm[1] : 0u);
      double prev_y = sprime(A).y;
      sw_d2 cur = sprime(B);
#pragma unroll
      for (int j = 0; j < SA_RUN; ++j) {
        const int P = P0 + j;
        if (P < P1) {                                       // (wave-uniform)
          SaPair D;
          load_pair(P + 2 <= P1 ? P + 2 : -1, D, j + 2 < SA_RUN ? mm[j + 2] : 0u);      // the pair after the next, in flight while this one computes
          const unsigned int m0 = mm[j] & 0xff, m1 = mm[j] >> 8;
          const sw_d2 nxt = sprime(Cn);
          // the rows below / above: the neighbouring lane's registers (every lane takes part: a lane whose own pair holds no
          // fluid still serves its neighbours); lane 0 / 63 inject what they fetched from the adjacent band
          const double e0 = B.ez0 + beta * B.es0, e1 = B.ez1 + beta * B.es1;
          if (SLAB == 2 && ghost && edge_lane) {            // the ghost cells' s' for the next iteration (the owner forms the same bits)
            if ((mm[j] & CM_FLUID) && (mm[j] & vbit)) gsn[2 * P + gcol] = e0;
            if (((mm[j] >> 8) & CM_FLUID) && ((mm[j] >> 8) & vbit)) gsn[2 * P + 1 + gcol] = e1;
          }
          const double dn0 = wave_shift_inject<DPP_WAVE_SHR1>(prev_y, e0), up0 = wave_shift_inject<DPP_WAVE_SHL1>(cur.y, e0);
          const double dn1 = wave_shift_inject<DPP_WAVE_SHR1>(cur.x, e1), up1 = wave_shift_inject<DPP_WAVE_SHL1>(nxt.x, e1);
          if ((m0 | m1) & CM_FLUID) {
            const size_t i = bbase + (size_t)P * 128;
            sw_d2 cc = B.so, o = {0.0, 0.0};                // cc: the pair's s' (a non-fluid element keeps its old value, +0)
            if (PMODE >= 2) {
              sw_d2 pv = *reinterpret_cast<const sw_d2*>(p + i);
              constexpr int NP = PMODE >= 2 ? PMODE : 2;
              sw_d2 sv[NP];
              sv[0] = *reinterpret_cast<const sw_d2*>(s_new + i);      // s of N iterations ago, about to be overwritten
#pragma unroll
              for (int j = 1; j < NP - 1; ++j) sv[j] = *reinterpret_cast<const sw_d2*>(hist.s[j - 1] + i);
              sv[NP - 1] = B.so;
#pragma unroll
              for (int j = 0; j < NP; ++j) {
                if (m0 & CM_FLUID) pv.x = pv.x + sv[j].x * al[j];
                if (m1 & CM_FLUID) pv.y = pv.y + sv[j].y * al[j];
              }
              *reinterpret_cast<sw_d2*>(p + i) = pv;        // a non-fluid partner is written back unchanged
            }
            if (m0 & CM_FLUID) cc.x = cur.x;
            if (m1 & CM_FLUID) cc.y = cur.y;
            if (m0 & CM_FLUID) {                            // apply_a (main.c:679-691): diag, right, up, left, down
              double v = (double)(int)(m0 >> CM_DIAG_SHIFT) * cc.x;
              v = v - ((m0 & CM_RIGHT) ? cc.y : 0.0);
              v = v - ((m0 & CM_UP) ? up0 : 0.0);
              v = v - ((m0 & CM_LEFT) ? prev_y : 0.0);
              v = v - ((m0 & CM_DOWN) ? dn0 : 0.0);
              o.x = v;
              t += v * cc.x;
            }
            if (m1 & CM_FLUID) {
              double v = (double)(int)(m1 >> CM_DIAG_SHIFT) * cc.y;
              v = v - ((m1 & CM_RIGHT) ? nxt.x : 0.0);
              v = v - ((m1 & CM_UP) ? up1 : 0.0);
              v = v - ((m1 & CM_LEFT) ? cc.x : 0.0);
              v = v - ((m1 & CM_DOWN) ? dn1 : 0.0);
              o.y = v;
              t += v * cc.y;
            }
            if ((m0 & m1) & CM_FLUID) *reinterpret_cast<sw_d2*>(s_new + i) = cc;
            else if (m0 & CM_FLUID) s_new[i] = cc.x;
            else s_new[i + 1] = cc.y;
            if (STORE) {
              if ((m0 & m1) & CM_FLUID) *reinterpret_cast<sw_d2*>(out + i) = o;
              else if (m0 & CM_FLUID) out[i] = o.x;
              else out[i + 1] = o.y;
            }
            if (SLAB == 1 && slab_edge_row(i, lane, TS, nb_local, (nbr.z_dn ? 1 : 0) | (nbr.z_up ? 2 : 0))) {   // the rows the neighbours will read
              if (m0 & CM_FLUID) st_system(s_new + i, cc.x);
              if (m1 & CM_FLUID) st_system(s_new + i + 1, cc.y);
            }
          }
          prev_y = cur.y; cur = nxt;
          B = Cn; Cn = D;
        }
      }
    };
    if (SA_RUN == 8 && interior) run(yes_t()); else run(no_t());
  }
  if (SLAB == 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // landed before this block joins the all-reduce (block_sum syncs)
  t = block_sum<SA_THREADS>(t);
  if (fin_op >= 0) block_finish<false, SA_THREADS>(t, partial, counter, sc, fin_op);   // fin_op < 0: dot(out, s') is replayed sequentially
}

static inline unsigned sa_blocks(const euler_sim* S, int run) {   // one wave per run of pair-records, at most 2048 blocks (the partials)
  return eu_blocks((size_t)(S->band_hi - S->band_lo) * ((S->geom.TS / 2 + run - 1) / run), SA_THREADS / 64, 2048);
}
// one launch of k_search_apply: what its instantiations have in common
struct SaCall { SkewGeom gl; int fin; SlabNeighbours nbr; CoarseRef cref; SaHist hist; ZrArgs zr; };
template <int SLAB, int PMODE, int RUN, int COARSE, bool STORE, bool ZR = false>
static void sa_launch(euler_sim* S, const SaCall& c) {
  LAUNCH(S, KC_APPLY_A, (k_search_apply<SLAB, PMODE, RUN, COARSE, STORE, ZR>), dim3(sa_blocks(S, RUN)), dim3(SA_THREADS), LOC(S->s), LOC(S->z), LOC(S->s2),
         LOC(S->q), LOC(S->cellmask), c.gl, S->partial, S->sc, 0, S->red_counter, c.fin, c.nbr, LOC(S->p), S->s2, S->s, RUN == 8 ? S->chunk_list : (const unsigned int*)nullptr, c.cref, c.hist, c.zr);
}
// The instantiations that exist.  Runs of 16 / 32 (experiments, sa_run): the plain configurations with the ring of two only, 16 on one GPU only; everything else runs of 8,
// and only those may leave A s' out (STORE false, tile_recompute).  Rings of 4 / 8 (p_steps): never with the mailboxes (SLAB 1)
template <int SLAB, int COARSE, int PMODE>
static void sa_pick_run(euler_sim* S, const SaCall& c, int run, bool store) {
  if constexpr (COARSE == 0 && SLAB != 2 && PMODE <= 2) {
    if constexpr (SLAB == 0) { if (run == 16) return sa_launch<SLAB, PMODE, 16, COARSE, true>(S, c); }
    if (run != 8) return sa_launch<SLAB, PMODE, 32, COARSE, true>(S, c);
  }
  if (store) sa_launch<SLAB, PMODE, 8, COARSE, true>(S, c); else sa_launch<SLAB, PMODE, 8, COARSE, false>(S, c);
}
template <int SLAB, int COARSE>
static void sa_pick(euler_sim* S, const SaCall& c, int pmode, int run, bool store) {      // pmode: 1 or the ring's length (2, 4, 8)
  if constexpr (SLAB != 1) {
    if (pmode == 8) return sa_pick_run<SLAB, COARSE, 8>(S, c, run, store);
    if (pmode == 4) return sa_pick_run<SLAB, COARSE, 4>(S, c, run, store);
  }
  if (pmode == 2) sa_pick_run<SLAB, COARSE, 2>(S, c, run, store); else sa_pick_run<SLAB, COARSE, 1>(S, c, run, store);
}
// iterations >= 1 of a single-GPU solve: s' = z + beta s and A s' in one launch; returns with S->s = s' and A s' in S->q
int eu_launch_search_apply(euler_sim* S, int it) {
  const bool seq = S->cfg.dot_mode == EULER_DOT_SEQUENTIAL && !S->has_comm;
  SlabNeighbours nbr = {nullptr, nullptr, nullptr, nullptr, S->band_hi - S->band_lo, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  const bool direct = S->has_comm && eu_p2p_has_neighbour_arrays(S);   // (opt-in) read the neighbouring slabs' z and s where they live
  const bool ghost = ghost_mode(S);
  if (ghost) {      // the neighbours' z rows came with G1; the ghost rows of s are kept here (two generations, like s / s2)
    const int c = S->gs_cur;
    if (S->band_lo > 0) { nbr.zrow_dn = xrow(S, XR_ZRECV_LO); nbr.srow_dn = xrow(S, XR_GS_LO0 + c); nbr.snew_dn = xrow(S, XR_GS_LO0 + (c ^ 1)); }
    if (S->band_hi < S->geom.nbands) { nbr.zrow_up = xrow(S, XR_ZRECV_HI); nbr.srow_up = xrow(S, XR_GS_HI0 + c); nbr.snew_up = xrow(S, XR_GS_HI0 + (c ^ 1)); }
    S->gs_cur = c ^ 1;
  } else if (direct) {   // addressed with this rank's offsets (the arrays are full-size everywhere)
    eu_p2p_neighbour_arrays(S, &nbr.z_dn, &nbr.s_dn, &nbr.z_up, &nbr.s_up);
    if (nbr.z_dn) { nbr.z_dn += S->e_lo; nbr.s_dn += S->e_lo; }
    if (nbr.z_up) { nbr.z_up += S->e_lo; nbr.s_up += S->e_lo; }
  } else if (S->has_comm) {   // the default: one exchange brings the neighbours' edge rows of z and s into the adjacent bands' storage
    if (int rc = eu_comm_halo_two(S, S->z, S->s)) return rc;
  }
  // p += alpha s rides along, two iterations' worth on every even iteration (k_search_apply PMODE) - in every configuration since
  // round 3: the parity mode's k_update_pr read and wrote p on every iteration for nothing but this
  const int steps = S->s_ring_n;
  const int pmode = (it >= steps && it % steps == 0) ? steps : 1;
  const bool mg = eu_is_mg(S);
  SaCall c = {S->geom, S->has_comm ? fin_or_comm(S, FIN_ALPHA) : (seq ? -1 : (int)FIN_ALPHA), nbr,
              {mg ? S->mg_x : S->cc_y, mg ? 0 : S->coarse_shift, mg ? S->mg_nx[0] : S->coarse_nx, mg ? S->mg_ny[0] : S->coarse_ny, S->band_lo},
              {{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}}, {S->r, S->precon, S->tile_table, S->zhalo, S->zrows, S->X}};
  c.gl.S = S->e_cnt;
  for (int j = 1; j + 1 < steps; ++j) c.hist.s[j - 1] = LOC(S->s_ring[j]);      // PMODE N (it a multiple of N): s_(it-N+j) sits in ring[j]
  const int run = sa_run(S);
  const bool store = !tile_recompute(S);      // false: A s' is not stored (k_precond_tile<16, true> forms it again)
  const bool coarse = eu_is_two_level(S) && tile_fused(S);      // z + P y: runs of 8 (the list)
  if (S->z_halo_last) sa_launch<0, 1, 8, 0, false, true>(S, c);      // z formed again from r (tile_z_recompute): the previous k_precond_tile left its halo only - odd passes only (PMODE 1)
  else if (coarse && ghost) sa_pick<2, 2>(S, c, pmode, run, store);      // coarse correction on row slabs (multilevel mode): the ghost rows of z get their P y here as well
  else if (coarse && mg) sa_pick<0, 2>(S, c, pmode, run, store);
  else if (coarse) sa_pick<0, 1>(S, c, pmode, run, store);
  else if (ghost) sa_pick<2, 0>(S, c, pmode, run, store);      // (tile-local mode; several ranks: runs of 8)
  else if (direct) sa_pick<1, 0>(S, c, pmode, run, store);
  else sa_pick<0, 0>(S, c, pmode, run, store);
  S->s = S->s_ring[it % steps]; S->s2 = S->s_ring[(it + 1) % steps];      // (two arrays: the swap of rounds 1-4)
  S->s_launched = it + 1;
  if (seq) eu_launch_dot(S, S->q, S->s, FIN_ALPHA, 0);      // (`seq` is exactly eu_launch_dot's condition for the sequential replay, k_dot_sequential of k_pcg.hip: change the two together)
  return S->has_comm ? eu_comm_finish(S, FIN_ALPHA, 0, 0) : EULER_OK;
}
