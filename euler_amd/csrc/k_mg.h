// k_mg.h — internal: what the multilevel preconditioner's coarse part (k_mg.hip: the hierarchy and the per-solve operators; k_mg_cycle.hip: the V-cycle; k_mg_split.hip: the cycle
// split by rows) shares among its files and with the fine-grid passes (k_tile.hip, k_search.hip) and k_coarse.hip.  The limits and the planning in plain C: euler_host.h.
#pragma once

#include "euler_dev.h"

#define MG_OMEGA 0.8         // damped Jacobi on every level below the dense one (tools/r05/mg_proto.py: 0.7 - 1.0 are within two iterations of each other, 1.1 costs 40 %)
// The Jacobi steps damp per node, omega_i = min(MG_OMEGA, MG_THETA / (1 + sum |off-diagonals| / d)): Gershgorin then keeps D~^-1 A below MG_THETA < 2 everywhere.  A regular node's
// off-diagonals add up to its diagonal (0.8 either way); a drop of spray - one fluid cell between four nodes - is a rank-one block of eigenvalue 4 d that plain omega = 0.8 multiplies
// by 1 - 3.2 per step: as the waterfall filled with spray the cycle stopped approximating the coarse solve and PCG fell back to the tile-local mode's iteration counts (oracle: mg_damping)
#define MG_THETA 1.6
// Level 0's node spacing in grid cells: node (I, J) sits AT the centre of cell (G0 J + G0 / 2, G0 I + G0 / 2).  8 (round 5): a tank at rest needs 30 PCG iterations to 1e-6 where
// 16 - the tile width - needs 52 and round 4's aggregates of 16 needed 104 (tools/r05/mg_proto.py; dam break at impact 39 / 65 / 109, waterfall 37 / 63 / 124), for a level 0 of
// four times the nodes.  Everything below follows from it: a band of 64 rows holds MG_RPB node rows; the lanes 8 G - 4 .. 8 G + 3 of a tile (GROUP G = (lane + 4) >> 3: 0 .. 8,
// the first and the last half groups) lie between the same two node rows I0 = 8 band + G - 1 and I0 + 1, and their 16 + 7 columns between the four node columns
// Jq .. Jq + 3, Jq = 2 k - G - 1 (k: the tile's index in its band): a tile leaves 9 groups x 2 node rows x 4 node columns = 72 sums (160 per tile with groups of four lanes,
// until the two quads between the same node rows were merged: mg_gather0, below, then takes 4 loads per node instead of 16).  MG_G0 and MG_RPB themselves: euler_host.h.
#define MG_LOG 3
#define MG_LG 4                                // the quad: what a DPP butterfly adds in registers; the two quads of a group meet in LDS
#define MG_NGRP 9
#define MG_NSEG (16 / MG_G0 + 1)               // node intervals a lane's 16 columns can touch
#define MG_NSLOT 4
#define MG_PART (MG_NGRP * 2 * MG_NSLOT)       // doubles k_precond_tile leaves per tile: group x row slot x column slot, stored [band][group][tile][row slot][column slot] (mg_gather0)
#define MG_NI ((19 + MG_G0 - 1) / MG_G0 + 1)  // node intervals the 20 records of a k_search_apply run and its window can touch
static_assert(MG_G0 == 8, "MG_G0: the tiles' partial sums (k_precond_tile, mg_gather0) are laid out for nodes 8 cells apart");
#define MG_NULL_MAX 4        // indicators of fluid regions cut off from the air that are kept (k_coarse.hip CC_NULL_MAX)
#define MG_DOT_BLOCKS 4096   // workgroups of k_mg_up at most (tiles of 32 x 32 nodes of level 0: 16384^2 has 4096 with G0 = 8)
#define MG_FIN_SLOT 7        // k_mg_up's epilogue on row slabs with a split cycle: x_0 . rhs_0 of the own rows is ADDED to the rank's slot instead of applied

int  eu_mg_alloc(euler_sim* S);
void eu_mg_release(euler_sim* S);
int  eu_mg_setup(euler_sim* S);                                   // per solve: the operators of every level (the dense top level's stencil is S->mg_a + 9 * S->mg_off[top])
int  eu_mg_solve(euler_sim* S, int fin_op, int force);            // per iteration: the V-cycle, x_0 . rhs_0 into dot(z, r), the scalar epilogue
int  eu_mg_search_init(euler_sim* S);                             // s = z + P_0 x_0
int  eu_mg_add_row(euler_sim* S, double* row, int yrow);          // + P_0 x_0 on a compact row of cells
int  eu_mg_null_setup(euler_sim* S);                              // per solve, behind the indicators' way down the levels: what the gauge of a cut-off region needs
int  eu_mg_slab_rows(euler_sim* S);                              // row slabs: this rank's share of level 0's right-hand side into its slot of the exchange buffer
// row slabs, the cycle split by rows (k_mg_split.hip "row slabs: the cycle split by rows"): whether this handle runs it, the all-gather's doubles per rank, the neighbour messages
// (k = 0, 1 send to the rank below / above, 2, 3 what arrived from them; doubles each: eu_mg_split_count), the ranks' {x_0 . rhs_0, gauge sums}
bool eu_mg_split(euler_sim* S);
int  eu_mg_split_nsmall(euler_sim* S);
int  eu_mg_split_count(euler_sim* S);
double* eu_mg_split_msg(euler_sim* S, int k);
double* eu_mg_split_gc(euler_sim* S);
int  eu_mg_split_pre(euler_sim* S);
int  eu_mg_split_mid(euler_sim* S, int fin_op, int force, double* zrecv_lo, double* zrecv_hi);
int  eu_mg_split_fold(euler_sim* S, int fin_op, int force);
void eu_mg_split_release(euler_sim* S);
bool eu_mg_split_setup(euler_sim* S);                             // ... and whether it forms the operators by owners as well (k_mg_split.hip: eu_mg_setup_split)
int  eu_mg_setup_split(euler_sim* S);
// the limits of the cycle's launches, checked where the mode is selected and again by every cycle; `why` ends the message
int  eu_mg_check_tail(const euler_sim* S, const char* why);      // at most MG_TAIL_LEVELS levels behind the entry level
int  eu_mg_check_tiles0(const euler_sim* S, const char* why);    // at most MG_DOT_BLOCKS tiles of 32 x 32 nodes of level 0

#ifdef __HIPCC__
// A cell's column c (or row) against n nodes, node j AT the centre of cell G0 j + G0 / 2: the node left of / at the cell and the weight f (a multiple of 1 / G0) of the next one;
// beyond the outermost nodes the interpolant is constant (weight clamps, oracle: mg_w0)
__device__ __forceinline__ void mg_cell_w(int c, int n, int& j0, int& j1, double& f) {
  const int u = c - MG_G0 / 2;
  int j = u >> MG_LOG;
  double w = (double)(u & (MG_G0 - 1)) * (1.0 / MG_G0);
  if (j < 0) { j = 0; w = 0.0; }
  int k = j + 1;
  if (k > n - 1) { k = n - 1; w = 0.0; }
  j0 = j; j1 = k; f = w;
}
// the two values a row of cells sees at a node column: rows combined first (oracle mg_interp0: lo / hi), then mg_lerp_x along the row
__device__ __forceinline__ double mg_rows(double v0, double v1, double fy) { return (1.0 - fy) * v0 + fy * v1; }
__device__ __forceinline__ double mg_lerp_x(double lo, double hi, double fx) { return (1.0 - fx) * lo + fx * hi; }
// (P_0 y) at cell (x, yrow)
__device__ __forceinline__ double mg_interp0(const double* __restrict__ y, int nx0, int ny0, int x, int yrow) {
  int jx0, jx1, jy0, jy1;
  double fx, fy;
  mg_cell_w(x, nx0, jx0, jx1, fx);
  mg_cell_w(yrow, ny0, jy0, jy1, fy);
  const double lo = mg_rows(y[(size_t)jy0 * nx0 + jx0], y[(size_t)jy1 * nx0 + jx0], fy);
  const double hi = mg_rows(y[(size_t)jy0 * nx0 + jx1], y[(size_t)jy1 * nx0 + jx1], fy);
  return mg_lerp_x(lo, hi, fx);
}

// ------------------------------------------------------------------------------------------ hierarchy
struct MgHier {
  int nl;                          // levels, the dense top included
  int nx[MG_MAXLEV], ny[MG_MAXLEV];
  unsigned int off[MG_MAXLEV];     // first node of level l in the pooled arrays
  const double* a;                 // stencils: level l at a + 9 * off[l], entry k of node c at [k * n_l + c]
  double* rhs;
  double* x;
  const double* wd;                // omega / diagonal per node (0 where the node carries no fluid): the Jacobi steps multiply
  const uint8_t* inner0;           // level 0: 1 where a node's stencil is the one of deep water (`ic`), 2 where it is all zeros (no fluid under the node): the two level-0 kernels then load a byte instead of nine doubles
  double ic[9], icwd;
};
static inline MgHier mg_hier(const euler_sim* S) {
  MgHier H;
  H.nl = S->mg_levels;
  for (int l = 0; l < MG_MAXLEV; ++l) { H.nx[l] = l < H.nl ? S->mg_nx[l] : 0; H.ny[l] = l < H.nl ? S->mg_ny[l] : 0; H.off[l] = l < H.nl ? (unsigned int)S->mg_off[l] : 0u; }
  H.a = S->mg_a; H.rhs = S->mg_rhs; H.x = S->mg_x; H.wd = S->mg_wd;
  H.inner0 = S->mg_inner0;
  for (int k = 0; k < 9; ++k) H.ic[k] = S->mg_ic[k];
  {      // deep water's omega_i / d (k_mg_wd's expressions: a node flagged "inner" must get the bits its own entries would give)
    const double d = S->mg_ic[4];
    double off = 0.0;
    for (int k = 0; k < 9; ++k) if (k != 4) off = off + fabs(S->mg_ic[k]);
    double om = d != 0.0 ? MG_THETA / (1.0 + off / d) : 0.0;
    if (om > MG_OMEGA) om = MG_OMEGA;
    H.icwd = d != 0.0 ? om / d : 0.0;
  }
  return H;
}
__device__ __forceinline__ const double* mg_sten(const MgHier& H, int l) { return H.a + 9 * (size_t)H.off[l]; }

// weight of node j of a finer level (fn nodes) on node Jc of the next one (cn nodes), whose node Jc sits on the finer level's node 2 Jc
__device__ __forceinline__ double mg_w1(int Jc, int j, int fn, int cn) {
  if (j < 0 || j >= fn || Jc < 0 || Jc >= cn) return 0.0;
  if (j == 2 * Jc) return 1.0;
  if (j == 2 * Jc - 1) return 0.5;
  if (j == 2 * Jc + 1) return Jc + 1 <= cn - 1 ? 0.5 : 1.0;      // (the last fine node, odd, without a node to its right: constant)
  return 0.0;
}

// Level 0's right-hand side from the tiles' sums (k_precond_tile: [band][group][tile][row slot][column slot], k_mg.h).  Node row I collects row slot 0 of the groups with
// I0 = I and row slot 1 of those with I0 = I - 1; I0 = 8 b + G - 1, so one group per node row - two HALF groups (G = 8 of band b - 1, G = 0 of band b) where the row lies
// across a band boundary; node column J lies in the slots of exactly two tiles of a group, k = (J + G - 1) >> 1 (slot 2 or 3) and k + 1 (slot 0 or 1).  Four loads per node
// (eight across a band boundary), every one issued before the first add; a fixed order.
__device__ __forceinline__ double mg_gather0(const double* __restrict__ part, int I, int J, int ntb, int band_lo, int band_hi) {
  double v[8];
#pragma unroll
  for (int rs = 0; rs < 2; ++rs) {
    const int I0 = I - rs;
    const int b1 = (I0 + 1) >> MG_LOG, G1 = I0 + 1 - MG_RPB * b1;      // (I0 >= -1)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int b = h == 0 ? b1 : b1 - 1, G = h == 0 ? G1 : 8;
      const bool grp = (h == 0 || G1 == 0) && b >= band_lo && b < band_hi;
      const int ka = (J + G - 1) >> 1;
      const double* row = part + (((size_t)(grp ? b - band_lo : 0) * MG_NGRP + (size_t)G) * ntb) * (2 * MG_NSLOT) + rs * MG_NSLOT;      // [band][group][tile][row slot][column slot]
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int k = ka + u, q = J - (2 * k - G - 1);      // u = 0: slot 2 or 3; u = 1: slot 0 or 1
        const bool ok = grp && k >= 0 && k < ntb;
        v[rs * 4 + h * 2 + u] = ok ? row[(size_t)k * (2 * MG_NSLOT) + q] : 0.0;
      }
    }
  }
  double t = 0.0;
#pragma unroll
  for (int u = 0; u < 8; ++u) t = t + v[u];
  return t;
}

struct MgDownArgs {
  MgHier H;
  int lA, lB;                 // from the right-hand side of level lA to that of level lB (lA <= lB)
  int tile;                   // edge of a workgroup's tile of level lB
  int cap0, cap1;             // doubles per LDS patch of the levels lA, lA + 2 / lA + 1, lA + 3
  int tail;                   // the workgroup that draws the last ticket goes on with the levels >= lB (all of <= 1024 nodes), the dense top and the way back up to lB
  const double* part;         // GATHER: the tiles' partial sums
  int ntb, band_lo, band_hi;
  const double* inv;          // the dense top level's inverse [n_top][n_top]
  unsigned int* ticket;
  const PcgScalars* sc;
  // row slabs, split cycle (eu_mg_split_*): the launch covers the tile rows [tile_row0, tile_row0 + gridDim.x / tiles_x) of the output level only, and the entry level's
  // right-hand side counts as 0 outside the rows [clip_lo, clip_hi) - this rank's share lives there, the memory beyond holds other iterations' leftovers
  int tile_row0, clip_lo, clip_hi;
  int force;                  // 0: a launch behind convergence (sc->done) or of a solve that never started (!sc->nonzero) returns at once - every workgroup alike, no ticket is drawn
};

// up: x_l = x2 + omega (rhs - A x2) / d with x2 = the Jacobi step + P x_(l+1), for the levels below the tail's entry level down to 0.  A workgroup owns a tile of
// level 0 and recomputes what it needs of the coarser levels: x_l on `X_l`, x2 on X_l grown by one, x_(l+1) on the nodes around that.
struct MgUpArgs {
  MgHier H;
  int lC;                     // the level whose result is in H.x already (the tail's entry level; 0: nothing to do but the dot product)
  int l0;                     // the finest level this launch computes (k_mg_up: > 0 when level 0 is left to k_mg_up0; then no dot product, no epilogue)
  int tile, cap;              // edge of a workgroup's tile of level l0; doubles per LDS patch
  int row_lo, row_hi;         // node rows of level 0 whose x . rhs this rank adds to dot(z, r) (row slabs: the own rows)
  PcgScalars* sc;
  int fin_op, force;
  double* dot_part;           // [MG_DOT_BLOCKS] partials of x_0 . rhs_0, then [MG_NULL_MAX][MG_DOT_BLOCKS] partials of m_0 . x_0 (the gauge, below)
  unsigned int* ticket;
  const double* nullv;        // k_coarse.hip's cc_null: [.. + MG_NULL_MAX * 256] = the number of fluid regions cut off from the air
  const double* n0;           // [MG_NULL_MAX][nstride]: their indicators on the levels (level 0 first)
  const double* m0;           // [MG_NULL_MAX][n_0]: P_0^T of their indicators on the cells; [MG_NULL_MAX * n_0 + q] = m_0 . n_0
  size_t nstride;
  int tile_row0;              // row slabs, split cycle: the launch covers the tile rows from here on (of level l0)
  double* slot;               // ... and k_mg_up0 leaves {x_0 . rhs_0 over the own rows, the gauge sums} HERE instead of applying them: they are summed over the ranks first (k_mg_split_fold)
};

// k_mg_cycle.hip: the cycle's argument records and launchers.  Each launch covers the rows [r0, r1) of its output level (lB, level 1, l0, level 0) by the tile rows
// that hold them - the split cycle's launches; r1 < 0: the whole level.  Every kernel is compiled there alone
MgDownArgs eu_mg_down_args(const euler_sim* S, const MgHier& H, int lA, int lB, int lC);
MgUpArgs   eu_mg_up_args(const euler_sim* S, const MgHier& H, int lC, int fin_op, int force);
int  eu_mg_launch_down(euler_sim* S, MgDownArgs A, bool gather, int r0 = 0, int r1 = -1);      // k_mg_down<gather>
int  eu_mg_launch_down1(euler_sim* S, MgDownArgs A, bool gather, int r0 = 0, int r1 = -1);     // k_mg_down1<gather>
int  eu_mg_launch_up(euler_sim* S, MgUpArgs V, int r0 = 0, int r1 = -1);                       // k_mg_up
int  eu_mg_launch_up0(euler_sim* S, MgUpArgs U, int r0 = 0, int r1 = -1);                      // k_mg_up0
// k_mg.hip: the launches eu_mg_setup shares with the setup by owners
int  eu_mg_assemble0(euler_sim* S, size_t first, size_t count);
void eu_mg_coarsen(euler_sim* S, int l, int r0, int r1);
void eu_mg_setup_tail(euler_sim* S, int l0, int i0, int i1);
#endif
