// k_mg.hip — the coarse part of the MULTILEVEL preconditioner (EULER_PRECOND_IC0_TILE_MG, include/euler.h; round 5):
//
//     z = M_tile^-1 r + P_0 V(P_0^T r)
//
// M_tile = the tile-local IC(0) of k_tile.hip.  Level 0 = a grid of NODES, node (I, J) at the centre of grid cell (8 J + 4, 8 I + 4) (MG_G0 = 8, k_mg.h: two node columns per
// tile width, eight node rows per band); P_0 = bilinear interpolation from the four nodes around a cell (weights in eighths), restricted to the fluid, constant beyond the
// outermost nodes.  Level l + 1 = every other node of level l in both directions (its node J sits ON node 2 J), bilinear again: weights 1, 1/2 - full weighting.  Because nodes
// sit AT cell centres / on finer nodes, a hat is 0 at the neighbouring nodes and the Galerkin operators A_0 = P_0^T A P_0, A_(l+1) = P^T A_l P are exact NINE-POINT
// stencils (a[k][c]: the entry that couples node c = (I, J) to node (I + k / 3 - 1, J + k % 3 - 1); A_0's entries are multiples of 2^-12: integer sums, exact in any order).
// V = one symmetric V-cycle: damped Jacobi (per-node omega, k_mg.h) from a zero guess, restricted residual, recursion, correction, Jacobi again; the top level (<= 64 nodes) is
// the dense pseudo-inverse of k_coarse.hip (factor, inverse, null-space fix for water cut off from the air).
//
// History: rounds 3-4 used piecewise constants over 16 x 16 blocks (aggregation: 5-point stencils with integer entries, the correction scaled by 1.7) and ONE launch per
// level and direction (12 launches, 63 us per iteration at 8192^2).  Bilinear spaces on nodes 16 cells apart halved the iteration count, nodes 8 cells apart nearly halved it
// again (tank at rest to 1e-6: 104 -> 52 -> 30; tools/r05/mg_proto.py) for a level 0 of four times the nodes.  The cycle runs in FOUR to SIX launches whatever the depth:
//
//   k_mg_down1<true>  (level 0 of more than MG_SMALL_LEVEL0 nodes) gathers the level-0 right-hand side from the tiles' partial sums (k_precond_tile leaves MG_PART = 72
//                     doubles per tile: [group of 8 lanes][row slot][column slot], k_mg.h) and takes it down ONE level on workgroups of 256 threads
//   k_mg_down<..>     the next (up to three) level transitions per launch; every workgroup owns a tile of the OUTPUT level and recomputes the halo it needs of the levels
//                     below in LDS (Jacobi step, residual, restriction: a level transition is three LDS phases, no launch); the workgroup that draws the last ticket of the
//                     launch that reaches the entry level then runs every level of <= 1024 nodes - down, the dense top, up again - alone, out of LDS and registers
//   k_mg_up           from that level's result back to level 1 (level 0 on small grids): every workgroup owns a 32 x 32 tile and recomputes the halos of the coarser levels
//   k_mg_up0          level 1 -> level 0 on small workgroups; its last workgroup folds x_0 . rhs_0 into dot(z, r) and applies the scalar epilogue
// Every one of them leaves at once behind convergence (sc->done; round 6).
//
// Three files behind k_mg.h: this one holds the hierarchy (eu_mg_alloc; the levels' dimensions are plain C, eu_mg_levels in euler_host.c), the per-solve operators
// (eu_mg_setup), P_0 at single cells and the null-space kernels; k_mg_cycle.hip the four kernels above, their launchers and the cycle (eu_mg_solve); k_mg_split.hip the
// cycle split by rows on row slabs.  Each kernel is compiled in one of them only.
//
// The CPU restatement the tests check all of this against: the test oracle's mg_build / mg_vcycle (same formulas; sums in another order: agreement to rounding).
// No reference counterpart (the reference has ONE preconditioner, main.c:580-627).
#include "k_pcg.h"

// (a failed allocation gives back what the attempt already holds: the next attempt starts from nothing - ADVICE r5)
#define MGALLOC(p, n, flags) do { int _rc = eu_dalloc(S, &(p), (n), EU_MEM_MG, (flags)); if (_rc) { eu_mg_release(S); return _rc; } } while (0)
int eu_mg_check_tail(const euler_sim* S, const char* why) {
  const int behind = S->mg_levels - 1 - eu_mg_entry_level(S->mg_levels, S->mg_nx, S->mg_ny);
  if (behind <= MG_TAIL_LEVELS) return EULER_OK;
  eu_set_error("multilevel preconditioner: %d levels behind the entry level (at most %d)%s", behind, MG_TAIL_LEVELS, why);
  return EULER_EINVAL;
}
int eu_mg_check_tiles0(const euler_sim* S, const char* why) {
  const size_t tiles0 = (size_t)((S->mg_nx[0] + 31) / 32) * ((S->mg_ny[0] + 31) / 32);
  if (tiles0 <= MG_DOT_BLOCKS) return EULER_OK;
  eu_set_error("multilevel preconditioner: %zu tiles of level 0 (at most %d)%s", tiles0, MG_DOT_BLOCKS, why);
  return EULER_EINVAL;
}
int eu_mg_alloc(euler_sim* S) {
  if (S->mg_dot) return EULER_OK;
  const int levels = eu_mg_levels(S->X, S->geom.nbands, S->mg_nx, S->mg_ny, S->mg_off);
  if (levels < 0) { eu_set_error("multilevel preconditioner: more than %d levels", MG_MAXLEV); return EULER_EINVAL; }
  S->mg_levels = levels;
  S->mg_cells = S->mg_off[levels - 1] + (size_t)S->mg_nx[levels - 1] * S->mg_ny[levels - 1];
  const size_t n0 = (size_t)S->mg_nx[0] * S->mg_ny[0];
  // the limits of the cycle's launches, checked where the mode is SELECTED (euler_create, euler_set_precond) - not inside a solve, behind the substep's marker stages
  if (eu_mg_check_tail(S, ": the grid is too large for this mode") || eu_mg_check_tiles0(S, ": the grid is too large for this mode")) { S->mg_levels = 0; return EULER_EINVAL; }
  MGALLOC(S->mg_a, 9 * S->mg_cells, EU_MEM_ZERO);
  MGALLOC(S->mg_a0i, 9 * n0, 0);
  MGALLOC(S->mg_rhs, 3 * S->mg_cells, EU_MEM_ZERO);
  S->mg_x = S->mg_rhs + S->mg_cells; S->mg_wd = S->mg_rhs + 2 * S->mg_cells;
  MGALLOC(S->mg_part, (S->chunk_cap + 64) * MG_PART, EU_MEM_ZERO);
  MGALLOC(S->mg_null0, (size_t)MG_NULL_MAX * S->mg_cells, EU_MEM_ZERO);      // the indicators of cut-off regions on every level (k_mg_null_prolong)
  MGALLOC(S->mg_inner0, n0, EU_MEM_ZERO);
  {      // level 0's stencil under deep water: A_0 = K (x) M + M (x) K with the 1-D mass and stiffness sums of the hats (multiples of 1 / G0^2: exact)
    double M[3] = {0, 0, 0}, K[3] = {-1.0 / MG_G0, 2.0 / MG_G0, -1.0 / MG_G0};
    for (int k = -(MG_G0 - 1); k <= MG_G0 - 1; ++k) { const double w = 1.0 - (k < 0 ? -k : k) / (double)MG_G0; M[1] += w * w; }
    for (int k = 0; k < MG_G0; ++k) M[0] += (1.0 - k / (double)MG_G0) * (k / (double)MG_G0);
    M[2] = M[0];
    for (int q = 0; q < 9; ++q) S->mg_ic[q] = K[q % 3] * M[q / 3] + M[q % 3] * K[q / 3];
  }
  MGALLOC(S->mg_m0, MG_NULL_MAX * n0 + MG_NULL_MAX, EU_MEM_ZERO);
  MGALLOC(S->mg_dot, (1 + MG_NULL_MAX) * MG_DOT_BLOCKS + 2, EU_MEM_ZERO);      // per-workgroup partials of x_0 . rhs_0 and of the gauge sums, then the tickets of k_mg_up and k_mg_down
  return EULER_OK;
}
#undef MGALLOC
void eu_mg_release(euler_sim* S) {
  eu_mg_split_release(S);
  eu_dev_free_group(S, EU_MEM_MG);
  S->mg_inner0 = nullptr;
  S->mg_wd = nullptr;
  S->mg_a = S->mg_rhs = S->mg_x = S->mg_part = S->mg_dot = S->mg_xbuf = S->mg_null0 = S->mg_m0 = nullptr;
  S->mg_a0i = nullptr; S->mg_xslot = 0;
}

// ------------------------------------------------------------------------------------------ per solve: the operators
// A_0 = P_0^T A P_0 from the tiles' masks.  With c' = a_diag - (fluid neighbours) (the air neighbours of a cell) and p_i = P_0^T e_i (a cell's four weights),
//     A = sum_i c'_i e_i e_i^T + sum_edges (e_i - e_j)(e_i - e_j)^T      =>      A_0 = sum_i c'_i p_i p_i^T + sum_edges (p_i - p_j)(p_i - p_j)^T
// and since the weights are linear between two nodes, p_i - p_j of a horizontal edge is (1 / MG_G0)(e_J - e_(J+1)) in x times the row weights wy - the same for every
// edge of that row between the nodes J and J + 1 (0 beyond the outermost nodes) - and likewise for vertical edges.  So a lane (one row, 16 consecutive columns: at
// most MG_NSEG = three node intervals) only counts: per interval, its horizontal edges H, sum c' wx wx^T and sum over its vertical edges of wx wx^T (three integers each, in
// 1 / MG_G0^2), and adds row weights x those to the stencil entries - 64 integer adds per lane into a window in LDS, flushed by 64-bit atomics (units of 1 / MG_G0^4 = 2^-12: exact).
#define MG_WIN_R (MG_RPB + 2)                 // node rows a band's 64 rows touch
#define MG_WIN_C (80 / MG_G0 + 2)             // node columns a tile's 79 columns touch (8: 12, 16: 7)
#define MG_WIN (MG_WIN_R * MG_WIN_C * 9)
// one tile's sums into the wave's window.  SYNTH: every cell deep inside the water (CM_INTERIOR) - no mask is read
template <bool SYNTH>
__device__ __forceinline__ void mg_tile_window(int* win, const uint8_t* __restrict__ mask, const SkewGeom& g, int lane, int band, int k, int nx0, int ny0) {
  const size_t base = ((size_t)band * g.TS + (size_t)k * 16) * 64 + 2 * lane;
  // the lane's row against the node rows (weights in 1 / G0)
  const int uy = 64 * band + lane - MG_G0 / 2, I0 = uy >> MG_LOG;
  int wy0 = MG_G0 - (uy & (MG_G0 - 1)), wy1 = uy & (MG_G0 - 1);
  if (I0 < 0) { wy0 = 0; wy1 = MG_G0; }
  if (I0 >= ny0 - 1) { wy0 = MG_G0; wy1 = 0; }
  const bool vert_ok = I0 >= 0 && I0 <= ny0 - 2;
  const int Jb = (16 * k - lane - MG_G0 / 2) >> MG_LOG;      // node interval of the lane's first column
  int H[MG_NSEG], C[MG_NSEG][3], V[MG_NSEG][3];
#pragma unroll
  for (int m = 0; m < MG_NSEG; ++m) { H[m] = 0; C[m][0] = C[m][1] = C[m][2] = 0; V[m][0] = V[m][1] = V[m][2] = 0; }
#pragma unroll
  for (int P = 0; P < 8; ++P) {
    const unsigned int mm = SYNTH ? (unsigned int)(CM_INTERIOR | (CM_INTERIOR << 8)) : (unsigned int)*reinterpret_cast<const unsigned short*>(mask + base + P * 128);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const unsigned int cm = (mm >> (8 * h)) & 0xff;
      if (!(cm & CM_FLUID)) continue;
      const int ux = 16 * k + 2 * P + h - lane - MG_G0 / 2, J0 = ux >> MG_LOG;
      int w0 = MG_G0 - (ux & (MG_G0 - 1)), w1 = ux & (MG_G0 - 1);
      if (J0 < 0) { w0 = 0; w1 = MG_G0; }
      if (J0 >= nx0 - 1) { w0 = MG_G0; w1 = 0; }
      const int cp = (int)(cm >> CM_DIAG_SHIFT) - __popc(cm & (CM_RIGHT | CM_UP | CM_LEFT | CM_DOWN));
      const int hh = ((cm & CM_RIGHT) && J0 >= 0 && J0 <= nx0 - 2) ? 1 : 0;
      const int vv = (cm & CM_UP) ? 1 : 0;
      const int q00 = w0 * w0, q01 = w0 * w1, q11 = w1 * w1;
#pragma unroll
      for (int m = 0; m < MG_NSEG; ++m)
        if (J0 - Jb == m) { H[m] += hh; C[m][0] += cp * q00; C[m][1] += cp * q01; C[m][2] += cp * q11; V[m][0] += vv * q00; V[m][1] += vv * q01; V[m][2] += vv * q11; }
    }
  }
  const int rI0 = I0 - (MG_RPB * band - 1);
  const int cbase = (16 * k - 63 - MG_G0 / 2) >> MG_LOG;      // the window's first node column
#pragma unroll
  for (int sg = 0; sg < MG_NSEG; ++sg) {
    const int cJ0 = Jb + sg - cbase;
    const int Mx[2][2] = {{C[sg][0] + H[sg], C[sg][1] - H[sg]}, {C[sg][1] - H[sg], C[sg][2] + H[sg]}};
    const int Vx[2][2] = {{V[sg][0], V[sg][1]}, {V[sg][1], V[sg][2]}};
    const int wy[2] = {wy0, wy1};
#pragma unroll
    for (int ra = 0; ra < 2; ++ra)
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int ca = 0; ca < 2; ++ca)
#pragma unroll
          for (int cb = 0; cb < 2; ++cb) {
            int val = wy[ra] * wy[rb] * Mx[ca][cb];
            if (vert_ok) val += (ra == rb ? 1 : -1) * Vx[ca][cb];
            if (val != 0) atomicAdd(&win[((rI0 + ra) * MG_WIN_C + cJ0 + ca) * 9 + (rb - ra + 1) * 3 + (cb - ca + 1)], val);
          }
  }
}
__global__ __launch_bounds__(256) void k_mg_assemble0(const uint8_t* __restrict__ mask, SkewGeom g, const unsigned int* __restrict__ list, const PcgScalars* sc,
                                                      int band_lo, int nx0, int ny0, unsigned long long* __restrict__ a0i) {
  __shared__ int s_win[4][MG_WIN];
  __shared__ int s_deep[MG_WIN];      // the window of a tile deep inside the water, away from the outermost nodes: the same integers whatever the tile (round 6)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int* win = s_win[wv];
  for (int e = lane; e < MG_WIN; e += 64) win[e] = 0;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const int ntb = g.T / 16, todo = (int)sc->n_chunks;
  const int n_waves = gridDim.x * 4;
  const size_t n0 = (size_t)nx0 * ny0;
  // A tile's rows sit at 64 band + lane, its columns at 16 k + ... - lane: against nodes 8 cells apart every tile meets them at the same offsets, so an INTERIOR tile (the
  // chunk list's top bit: every cell CM_INTERIOR) whose cells lie between the outermost nodes adds the same 1080 integers as any other - formed ONCE per workgroup here, by
  // the very code below on a mask of CM_INTERIOR (band 2, tile 8 of a level that is wide enough for them), and flushed without reading a mask or touching the window
  // (most of a tank: 16384^2 dam break 563 -> 475 us per solve - what is left are the ~700 memory-side adds of a tile's window).
  if (wv == 0) {
    mg_tile_window<true>(win, mask, g, lane, 2, 8, 1 << 20, 1 << 20);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int e = lane; e < MG_WIN; e += 64) { s_deep[e] = win[e]; win[e] = 0; }
  }
  __syncthreads();
  for (int w = blockIdx.x * 4 + wv; w < todo; w += n_waves) {
    const unsigned int entry = list[w];
    const int tile = (int)(entry & ~EU_CHUNK_INTERIOR);
    const int band = band_lo + tile / ntb, k = tile % ntb;
    // no row of the tile below node row 0 or above the last but one, no column left of node column 0 or right of the last but one (the clamps of mg_tile_window never act)
    const bool deep = (entry & EU_CHUNK_INTERIOR) != 0 && band >= 1 && MG_RPB * band + MG_RPB - 1 <= ny0 - 2 && 16 * k - 63 - MG_G0 / 2 >= 0 && ((16 * k + 15 - MG_G0 / 2) >> MG_LOG) <= nx0 - 2;
    if (!deep) {
      mg_tile_window<false>(win, mask, g, lane, band, k, nx0, ny0);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    const int cbase = (16 * k - 63 - MG_G0 / 2) >> MG_LOG;      // the window's first node column
    for (int e = lane; e < MG_WIN; e += 64) {
      const int v = deep ? s_deep[e] : win[e];
      if (v == 0) continue;
      if (!deep) win[e] = 0;
      const int kk = e % 9, cJ = (e / 9) % MG_WIN_C, rI = e / (9 * MG_WIN_C);
      const int I = MG_RPB * band - 1 + rI, J = cbase + cJ;
      if (I >= 0 && I < ny0 && J >= 0 && J < nx0) atomicAdd(&a0i[(size_t)kk * n0 + (size_t)I * nx0 + J], (unsigned long long)(long long)v);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}
// (the nine planes' entries [first, first + count) each: a rank of a split cycle converts the rows its tiles reach)
__global__ __launch_bounds__(256) void k_mg_convert0(const unsigned long long* __restrict__ a0i, double* __restrict__ a, size_t n0, size_t first, size_t count) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= 9 * count) return;
  const size_t e = (i / count) * n0 + first + i % count;
  a[e] = (double)(long long)a0i[e] * (1.0 / ((double)MG_G0 * MG_G0 * MG_G0 * MG_G0));
}

// A_(l+1) = P^T A_l P, per node of level l + 1 and stencil entry: entry q of node (I, J) = sum over the fine nodes m under (I, J) and the fine nodes n under the
// coarse neighbour (I, J) + q of w(m) A_l[m, n] w(n) - at most 3 x 3 x 3 x 3 terms, walked in a fixed order (rows [r0, r1) of the coarse level).
// A workgroup takes MGC_TI x MGC_TJ coarse nodes: the nine entries of the (2 TI + 1) x (2 TJ + 1) fine nodes under them come into LDS row by row (coalesced; the one-thread-per-
// entry form of rounds 4-5 read every fine entry up to nine times at a stride of two nodes: 654 us per solve at 16384^2, six times its bytes' worth), the sums are formed
// from there - the same terms in the same order, a thread per (node, entry) - and leave through LDS as rows of one entry.
#define MGC_TI 8
#define MGC_TJ 16
#define MGC_PH (2 * MGC_TI + 1)
#define MGC_PW (2 * MGC_TJ + 1)
__global__ __launch_bounds__(256) void k_mg_coarsen(const double* __restrict__ af, int fnx, int fny, double* __restrict__ ac, int cnx, int cny, const PcgScalars* sc, int r0, int r1) {
  if (!sc->nonzero) return;
  __shared__ double sa[9][MGC_PH * MGC_PW];      // 40 KB
  __shared__ double so[9][MGC_TI * MGC_TJ];      // 9 KB: [entry][node of the tile]
  const int tilesx = (cnx + MGC_TJ - 1) / MGC_TJ;
  const int I0 = r0 + (int)(blockIdx.x / tilesx) * MGC_TI, J0 = (int)(blockIdx.x % tilesx) * MGC_TJ;
  const int fi0 = 2 * I0 - 1, fj0 = 2 * J0 - 1;
  const size_t fn = (size_t)fnx * fny, cn = (size_t)cnx * cny;
  for (int k = threadIdx.x; k < 9 * MGC_PH * MGC_PW; k += 256) {
    const int e = k / (MGC_PH * MGC_PW), c = k % (MGC_PH * MGC_PW), mi = fi0 + c / MGC_PW, mj = fj0 + c % MGC_PW;
    sa[e][c] = (mi >= 0 && mi < fny && mj >= 0 && mj < fnx) ? af[(size_t)e * fn + (size_t)mi * fnx + mj] : 0.0;      // (beyond the level: +0, and its weight is 0)
  }
  __syncthreads();
#pragma unroll 1
  for (int k = threadIdx.x; k < 9 * MGC_TI * MGC_TJ; k += 256) {
    const int node = k / 9, q = k % 9;
    const int I = I0 + node / MGC_TJ, J = J0 + node % MGC_TJ, I2 = I + q / 3 - 1, J2 = J + q % 3 - 1;
    double acc = 0.0;
    if (I < r1 && J < cnx && I2 >= 0 && I2 < cny && J2 >= 0 && J2 < cnx) {
      // The weights once per thread - of the fine rows 2 I + dy on node I (wmy) and, for dy + ey = -2 .. 2, on the neighbour I2 (wny); the same along x; wn = wny wnx - instead
      // of one mg_w1 per term, and EVERY term added: the oracle's mg_build skips the terms whose weight is 0, which are +-0 here (the entries are finite) and leave a sum that
      // started from +0 as it is - the same bits without 81 branches around 81 LDS reads (the pass was bound by exactly that: 654 -> 290 us per solve at 16384^2).
      double wmy[3], wmx[3], wny[5], wnx[5];
#pragma unroll
      for (int d = 0; d < 3; ++d) { wmy[d] = mg_w1(I, 2 * I + d - 1, fny, cny); wmx[d] = mg_w1(J, 2 * J + d - 1, fnx, cnx); }
#pragma unroll
      for (int d = 0; d < 5; ++d) { wny[d] = mg_w1(I2, 2 * I + d - 2, fny, cny); wnx[d] = mg_w1(J2, 2 * J + d - 2, fnx, cnx); }
      const int m0 = (2 * I - fi0) * MGC_PW + (2 * J - fj0);
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const double wM = wmy[dy + 1] * wmx[dx + 1];
          const int m = m0 + dy * MGC_PW + dx;
          double a[9];
#pragma unroll
          for (int e = 0; e < 9; ++e) a[e] = sa[e][m];
#pragma unroll
          for (int ey = -1; ey <= 1; ++ey)
#pragma unroll
            for (int ex = -1; ex <= 1; ++ex) {
              const double wN = wny[dy + ey + 2] * wnx[dx + ex + 2];
              acc += wM * a[(ey + 1) * 3 + ex + 1] * wN;
            }
        }
    }
    so[q][node] = acc;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < 9 * MGC_TI * MGC_TJ; k += 256) {      // rows of MGC_TJ consecutive nodes of one entry
    const int q = k / (MGC_TI * MGC_TJ), node = k % (MGC_TI * MGC_TJ), I = I0 + node / MGC_TJ, J = J0 + node % MGC_TJ;
    if (I < r1 && J < cnx) ac[(size_t)q * cn + (size_t)I * cnx + J] = so[q][node];
  }
}
// (launch: one workgroup per tile of the coarse rows [r0, r1))
static inline unsigned mg_coarsen_blocks(int cnx, int r0, int r1) { return (unsigned)(((cnx + MGC_TJ - 1) / MGC_TJ) * ((r1 - r0 + MGC_TI - 1) / MGC_TI)); }

// per solve: A_0 from the tiles, the coarser operators, the dense top level's stencil as five arrays for k_coarse_factor
__global__ __launch_bounds__(256) void k_mg_top_stencil(const double* __restrict__ at, int n, double* __restrict__ out) {      // out: [9][n] -> the factor kernel reads d, e, n, ne, nw = entries 4, 5, 7, 8, 6
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < 9 * n) out[i] = at[i];
}
__global__ __launch_bounds__(256) void k_mg_inner0(MgHier H, uint8_t* __restrict__ inner, size_t first, size_t count) {      // a node whose nine entries are deep water's (bit for bit: both sides are exact)
  const size_t n = (size_t)H.nx[0] * H.ny[0], c = first + (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= first + count) return;
  bool same = true, none = true;
#pragma unroll
  for (int k = 0; k < 9; ++k) { const double v = H.a[(size_t)k * n + c]; same = same && v == H.ic[k]; none = none && v == 0.0; }
  inner[c] = same ? 1 : none ? 2 : 0;      // 2 (round 6): no fluid under the node's hat - the level-0 kernels load neither its entries nor omega / d nor its right-hand side
}
__global__ __launch_bounds__(256) void k_mg_wd(const double* __restrict__ a, const unsigned int* offs, int nl, MgHier H, double* __restrict__ wd) {
  (void)a; (void)offs; (void)nl;
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int l = blockIdx.y;
  const size_t n = (size_t)H.nx[l] * H.ny[l];
  if (c >= n) return;
  const double* st = mg_sten(H, l);
  const double d = st[4 * n + c];
  double off = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) if (k != 4) off = off + fabs(st[(size_t)k * n + c]);
  double om = d != 0.0 ? MG_THETA / (1.0 + off / d) : 0.0;      // (k_mg.h MG_THETA; oracle: mg_damping - the same expressions)
  if (om > MG_OMEGA) om = MG_OMEGA;
  wd[H.off[l] + c] = d != 0.0 ? om / d : 0.0;
}
// the launches eu_mg_setup shares with the setup by owners (k_mg_split.hip: eu_mg_setup_split; both zero the rows of mg_a0i they assemble first).  A_0's integer sums from
// this rank's tiles, then the nine planes' entries [first, first + count) as doubles
int eu_mg_assemble0(euler_sim* S, size_t first, size_t count) {
  const size_t n0 = (size_t)S->mg_nx[0] * S->mg_ny[0];
  HIPCHK(hipMemsetAsync(S->mg_part, 0, (S->chunk_cap + 64) * MG_PART * sizeof(double), S->stream));      // (tiles outside this solve's list contribute nothing)
  LAUNCH(S, KC_PRECON_FACTOR, k_mg_assemble0, dim3(eu_blocks(S->chunk_cap, 4, 2048)), dim3(256), S->cellmask, S->geom, S->chunk_list, S->sc, S->band_lo, S->mg_nx[0], S->mg_ny[0], S->mg_a0i);
  LAUNCH(S, KC_PRECON_FACTOR, k_mg_convert0, dim3((unsigned)((9 * count + 255) / 256)), dim3(256), S->mg_a0i, S->mg_a, n0, first, count);
  return EULER_OK;
}
// the rows [r0, r1) of level l's operator from level l - 1's
void eu_mg_coarsen(euler_sim* S, int l, int r0, int r1) {
  LAUNCH(S, KC_PRECON_FACTOR, k_mg_coarsen, dim3(mg_coarsen_blocks(S->mg_nx[l], r0, r1)), dim3(256), S->mg_a + 9 * S->mg_off[l - 1], S->mg_nx[l - 1], S->mg_ny[l - 1],
         S->mg_a + 9 * S->mg_off[l], S->mg_nx[l], S->mg_ny[l], S->sc, r0, r1);
}
// the levels l0 .. top, whole, each from the one below; level 0's flags on its rows [i0, i1); omega / diagonal per node of every level below the dense one (the cycle's Jacobi
// steps multiply)
void eu_mg_setup_tail(euler_sim* S, int l0, int i0, int i1) {
  const size_t n0 = (size_t)S->mg_nx[0] * S->mg_ny[0], first = (size_t)i0 * S->mg_nx[0], count = (size_t)(i1 - i0) * S->mg_nx[0];
  for (int l = l0; l < S->mg_levels; ++l) eu_mg_coarsen(S, l, 0, S->mg_ny[l]);
  hipLaunchKernelGGL(k_mg_inner0, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, S->stream, mg_hier(S), S->mg_inner0, first, count);
  hipLaunchKernelGGL(k_mg_wd, dim3((unsigned)((n0 + 255) / 256), (unsigned)S->mg_levels), dim3(256), 0, S->stream, (const double*)nullptr, (const unsigned int*)nullptr, 0, mg_hier(S), S->mg_wd);
}
int eu_mg_setup(euler_sim* S) {
  const size_t n0 = (size_t)S->mg_nx[0] * S->mg_ny[0];
  if (S->has_comm && eu_mg_split_setup(S)) return eu_mg_setup_split(S);
  HIPCHK(hipMemsetAsync(S->mg_a0i, 0, 9 * n0 * sizeof(unsigned long long), S->stream));
  int rc = eu_mg_assemble0(S, 0, n0);
  if (rc) return rc;
  // row slabs, the cycle replicated: a node row collects cells of the ranks either side of a slab boundary.  The entries are multiples of 2^-12 far below 2^37: their sums are
  // exact in any order, so ONE all-reduce makes A_0 whole and bit-identical everywhere (the split cycle exchanges rows with the neighbours instead)
  if (S->has_comm) COMM_CALL(S->bulk.allreduce(S->bulk.ctx, S->mg_a, (int32_t)(9 * n0), 0));
  eu_mg_setup_tail(S, 1, 0, S->mg_ny[0]);
  return EULER_OK;
}

// ------------------------------------------------------------------------------------------ P_0 at single cells (the first search direction, ghost rows, the null-space fix)
__global__ __launch_bounds__(256) void k_mg_search_init(double* __restrict__ s, const double* __restrict__ z, const uint8_t* __restrict__ mask, const double* __restrict__ y,
                                                        SkewGeom g, int nx0, int ny0, size_t e_lo, size_t e_cnt, const PcgScalars* sc) {
  if (pcg_idle(sc)) return;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < e_cnt; k += (size_t)gridDim.x * blockDim.x) {
    const size_t e = e_lo + k;
    double v = z[e];
    if (mask[e] & CM_FLUID) {
      int band, t, l;
      skew_decode(g, e, band, t, l);
      v = v + mg_interp0(y, nx0, ny0, t - l, band * 64 + l);
    }
    s[e] = v;
  }
}
int eu_mg_search_init(euler_sim* S) {
  LAUNCH(S, KC_UPDATE_SEARCH, k_mg_search_init, dim3(eu_blocks(S->e_cnt, 256 * 4, 4096)), dim3(256), S->s, S->z, S->cellmask, S->mg_x, S->geom, S->mg_nx[0], S->mg_ny[0], S->e_lo, S->e_cnt, S->sc);
  return EULER_OK;
}
__global__ __launch_bounds__(256) void k_mg_add_row(double* __restrict__ row, const double* __restrict__ y, int X, int yrow, int nx0, int ny0, const PcgScalars* sc) {
  if (pcg_idle(sc)) return;
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x < X) row[x] = row[x] + mg_interp0(y, nx0, ny0, x, yrow);
}
int eu_mg_add_row(euler_sim* S, double* row, int yrow) {
  LAUNCH(S, KC_UPDATE_SEARCH, k_mg_add_row, dim3((S->X + 255) / 256), dim3(256), row, S->mg_x, S->X, yrow, S->mg_nx[0], S->mg_ny[0], S->sc);
  return EULER_OK;
}

// ------------------------------------------------------------------------------------------ water cut off from the air: what the gauge of k_mg_up needs, per solve
// m_0[q] = P_0^T (the indicator of region q on the cells): a cell's four weights (multiples of 1 / 256: integer atomics, exact) where the level-0 indicator, sampled
// through P_0, says "inside"; then m_0 . n_0.  Both kernels return at once when no region is cut off (the usual case).
__global__ __launch_bounds__(256) void k_mg_null_mass(const uint8_t* __restrict__ mask, SkewGeom g, size_t e_lo, size_t e_cnt, const double* __restrict__ nullv, const double* __restrict__ n0,
                                                      size_t nstride, int nx0, int ny0, unsigned long long* __restrict__ acc, const PcgScalars* sc) {
  const int count = (int)nullv[MG_NULL_MAX * 256];
  if (!sc->nonzero || count <= 0) return;
  const size_t n0n = (size_t)nx0 * ny0;
  for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < e_cnt; k += (size_t)gridDim.x * 256) {
    const size_t e = e_lo + k;
    if (!(mask[e] & CM_FLUID)) continue;
    int band, t, l;
    skew_decode(g, e, band, t, l);
    const int x = t - l, y = band * 64 + l;
    int jx0, jx1, jy0, jy1;
    double fx, fy;
    mg_cell_w(x, nx0, jx0, jx1, fx);
    mg_cell_w(y, ny0, jy0, jy1, fy);
    const int wx1 = (int)(fx * MG_G0), wx0 = MG_G0 - wx1, wy1 = (int)(fy * MG_G0), wy0 = MG_G0 - wy1;
    for (int q = 0; q < MG_NULL_MAX && q < count; ++q) {
      if (!(mg_interp0(n0 + (size_t)q * nstride, nx0, ny0, x, y) > 0.5)) continue;
      unsigned long long* a = acc + (size_t)q * n0n;
      if (wy0 * wx0) atomicAdd(&a[(size_t)jy0 * nx0 + jx0], (unsigned long long)(wy0 * wx0));
      if (wy0 * wx1) atomicAdd(&a[(size_t)jy0 * nx0 + jx1], (unsigned long long)(wy0 * wx1));
      if (wy1 * wx0) atomicAdd(&a[(size_t)jy1 * nx0 + jx0], (unsigned long long)(wy1 * wx0));
      if (wy1 * wx1) atomicAdd(&a[(size_t)jy1 * nx0 + jx1], (unsigned long long)(wy1 * wx1));
    }
  }
}
__global__ __launch_bounds__(256) void k_mg_null_convert(const unsigned long long* __restrict__ acc, const double* __restrict__ nullv, size_t n, double* __restrict__ m0, const PcgScalars* sc) {
  const int count = (int)nullv[MG_NULL_MAX * 256];
  if (!sc->nonzero || count <= 0) return;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) m0[i] = (double)acc[i] * (1.0 / ((double)MG_G0 * MG_G0));
}
__global__ __launch_bounds__(1024) void k_mg_null_finish(const double* __restrict__ nullv, const double* __restrict__ n0, size_t nstride, size_t n0n, double* __restrict__ m0, const PcgScalars* sc) {
  const int count = (int)nullv[MG_NULL_MAX * 256];
  if (!sc->nonzero || count <= 0) return;
  __shared__ double s_red[16];
  const int q = blockIdx.x;
  if (q >= count) { if (threadIdx.x == 0) m0[(size_t)MG_NULL_MAX * n0n + q] = 0.0; return; }
  double t = 0.0;
  for (size_t c = threadIdx.x; c < n0n; c += 1024) t += m0[(size_t)q * n0n + c] * n0[(size_t)q * nstride + c];
  t = eu_wave_sum(t);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) { double v = 0.0; for (int k = 0; k < 16; ++k) v += s_red[k]; m0[(size_t)MG_NULL_MAX * n0n + q] = v; }
}
int eu_mg_null_setup(euler_sim* S) {      // behind k_mg_null_prolong (k_coarse.hip: eu_launch_coarse_consistent)
  const size_t n0n = (size_t)S->mg_nx[0] * S->mg_ny[0];
  if (S->has_comm) {
    // row slabs: a region's cells lie on several ranks, so m_0 is a sum over the ranks - an all-reduce of 4 n_0 doubles that only a job with a cut-off region needs.  Whether
    // there is one is the same on every rank (the dense level is replicated): one host round trip per solve decides (row-slab handles only)
    double cnt = 0.0;
    HIPCHK(hipMemcpyAsync(&cnt, S->cc_null + MG_NULL_MAX * 256, sizeof(double), hipMemcpyDeviceToHost, S->stream));
    HIPCHK(hipStreamSynchronize(S->stream));
    if (!(cnt > 0.0)) return EULER_OK;
  }
  HIPCHK(hipMemsetAsync(S->mg_a0i, 0, MG_NULL_MAX * n0n * sizeof(unsigned long long), S->stream));      // (A_0's integer sums are converted by now: the array is scratch)
  LAUNCH(S, KC_PRECON_FACTOR, k_mg_null_mass, dim3(eu_blocks(S->e_cnt, 256 * 8, 512)), dim3(256), S->cellmask, S->geom, S->e_lo, S->e_cnt, S->cc_null, S->mg_null0, S->mg_cells,
         S->mg_nx[0], S->mg_ny[0], S->mg_a0i, S->sc);
  LAUNCH(S, KC_PRECON_FACTOR, k_mg_null_convert, dim3((unsigned)((MG_NULL_MAX * n0n + 255) / 256)), dim3(256), S->mg_a0i, S->cc_null, MG_NULL_MAX * n0n, S->mg_m0, S->sc);
  // m_0 . n_0 from this rank's share of m_0 - it lies on the rows its cells reach, where the rank holds the indicator whatever the cycle's form (a split cycle prolongs it on
  // the own rows only) - then shares and scalars are summed over the ranks together (the shares: multiples of 1 / 64, exact in any order)
  LAUNCH(S, KC_PRECON_FACTOR, k_mg_null_finish, dim3(MG_NULL_MAX), dim3(1024), S->cc_null, S->mg_null0, S->mg_cells, n0n, S->mg_m0, S->sc);
  if (S->has_comm) COMM_CALL(S->bulk.allreduce(S->bulk.ctx, S->mg_m0, (int32_t)(MG_NULL_MAX * n0n + MG_NULL_MAX), 0));
  return EULER_OK;
}
