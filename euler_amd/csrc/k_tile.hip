// k_tile.hip — the tile-local preconditioner: everything between two apply_a passes of a PCG iteration in one launch (k_precond_tile), its factor (k_factor_tile) and the interior tiles' table.
#include "k_pcg.h"

#include <type_traits>

// Tile-local IC(0) (EULER_PRECOND_IC0_TILE): the three recurrences of k_sweep.hip restricted to blocks - a block = the cells of one
// band whose records fall into one tile [k W, (k+1) W), a parallelogram of 64 rows x W columns.  In the band-skewed layout
// a tile is W consecutive records = one contiguous piece of every solver array, and it is small enough to live in the
// REGISTERS of one wave (W = 16: 16 doubles per lane and vector).  So one wave loads a tile's r, A s and precon once, and
// does everything the PCG iteration needs between two apply_a passes without another trip to memory:
//     r -= alpha A s (fmadd, main.c:754) ; max |r| (inf_norm, main.c:756) ; q = L^-1 r ; z = L^-T q (main.c:602-626) ; dot(z, r)
// = kernels K2, K3, K4 and dot() of SURVEY 8d in ONE pass: 5 w + 1 = 41 bytes per cell instead of 6w+1 + 3w+1 + 4w+1 + ... .
// (p += alpha s rides along with the next apply_a pass, which reads s anyway: k_search_apply<.., true>.)
// The wavefront inside the tile is the one of k_sweep_skew (lane l at record t, lower / upper row by DPP wave shifts), fully
// unrolled with static register indices; tiles are independent, so thousands of waves stream at once and the kernel is
// bound by HBM bandwidth, not by a dependency chain.  The compiler schedules it (nothing to hand-issue: occupancy hides
// the latency).  Each wave walks tiles wave_id, wave_id + n_waves, ...; per-lane sums are folded in that fixed order,
// then per wave, per block, and by the last block over all blocks in index order: deterministic.
#define PT_THREADS 256
// fixed-shape reductions of a PT_THREADS block; result valid in thread 0
__device__ __forceinline__ void tile_block_reduce(double& mx, double& sm) {
  __shared__ double s_mx[PT_THREADS / 64], s_sm[PT_THREADS / 64];
  mx = eu_wave_max(mx);
  sm = eu_wave_sum(sm);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { s_mx[threadIdx.x >> 6] = mx; s_sm[threadIdx.x >> 6] = sm; }
  __syncthreads();
  if (threadIdx.x == 0) {
    mx = s_mx[0]; sm = s_sm[0];
    for (int k = 1; k < PT_THREADS / 64; ++k) { mx = s_mx[k] > mx ? s_mx[k] : mx; sm += s_sm[k]; }
  }
}

// E^-1 of an INTERIOR tile of 16 records (every cell fluid with a_diag 4): the recurrence starts from precon 0 on the tile's left
// edge and below lane 0 and sees the same coefficients everywhere, so its 16 x 64 values are the same for every interior tile of
// every solve.  Computed once per handle by the arithmetic of k_factor_tile (same bits); k_precond_tile keeps it in LDS instead of
// streaming 8 bytes per cell of precon from HBM.  One wave.  tab[P][lane] = {record 2P, record 2P + 1}.
__global__ __launch_bounds__(64) void k_tile_table(double* __restrict__ tab) {
  const int lane = threadIdx.x & 63;
  double own = 0.0, out = 0.0;
  sw_d2 pp[8];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const double nbv = wave_shift_inject<DPP_WAVE_SHR1>(out, 0.0);
    const double res = factor_step(4.0, own, nbv);
    own = res; out = res;
    if (j & 1) pp[j >> 1].y = res; else pp[j >> 1].x = res;
  }
#pragma unroll
  for (int P = 0; P < 8; ++P) reinterpret_cast<sw_d2*>(tab)[P * 64 + lane] = pp[P];
}
int eu_launch_tile_table(euler_sim* S) {
  hipLaunchKernelGGL(k_tile_table, dim3(1), dim3(64), 0, S->stream, S->tile_table);
  return EULER_OK;
}

template <int W>
__global__ __launch_bounds__(PT_THREADS) void k_factor_tile(TileArgs a) {
  if (!a.force && pcg_idle(a.sc)) return;
  const int lane = threadIdx.x & 63;
  const int ntb = a.g.T / W, total = a.nb_local * ntb;
  const int n_waves = gridDim.x * (PT_THREADS / 64);
  for (int tile = blockIdx.x * (PT_THREADS / 64) + (threadIdx.x >> 6); tile < total; tile += n_waves) {
    const int band = a.band_lo + tile / ntb, k = tile % ntb;
    const size_t base = ((size_t)band * a.g.TS + (size_t)k * W) * 64 + 2 * lane;
    unsigned int mm[W / 2];
    unsigned int any = 0;
#pragma unroll
    for (int P = 0; P < W / 2; ++P) { mm[P] = *reinterpret_cast<const unsigned short*>(a.mask + base + P * 128); any |= mm[P]; }
    if (!__ballot(((any | (any >> 8)) & CM_FLUID) != 0)) continue;     // no fluid in this tile: precon stays what it is
    sw_d2 pp[W / 2];
#pragma unroll
    for (int P = 0; P < W / 2; ++P) pp[P] = *reinterpret_cast<const sw_d2*>(a.pre + base + P * 128);
    double own = 0.0, out = 0.0;      // a tile starts where a band starts: precon 0 to the left and below
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const int cm = (int)((mm[j >> 1] >> ((j & 1) * 8)) & 0xff);
      const double cpre = (j & 1) ? pp[j >> 1].y : pp[j >> 1].x;
      const double nbv = wave_shift_inject<DPP_WAVE_SHR1>(out, 0.0);
      const double aa = (double)(cm >> CM_DIAG_SHIFT);               // main.c:586-600
      const double res = (cm & CM_FLUID) ? factor_step(aa, own, nbv) : cpre;     // non-fluid: the stale entry stays (and is what the neighbours read)
      own = res; out = res;
      if (j & 1) pp[j >> 1].y = res; else pp[j >> 1].x = res;
    }
#pragma unroll
    for (int P = 0; P < W / 2; ++P) *reinterpret_cast<sw_d2*>(a.pre + base + P * 128) = pp[P];
  }
}

// RECOMP (W == 16, inside a solve): the r update's A s' is not read back from memory - k_search_apply did not store it - but formed
// again from s' with the expression of k_search_apply / k_apply_a (main.c:679-691: diag, right, up, left, down; identical bits): the
// tile's 16 records of s' plus the pair-record before and after it, the rows below lane 0 / above lane 63 by ONE load (lanes 0-15 fetch
// the 16 values below, lanes 48-63 the 16 above; v_readlane hands them to the DPP shifts).  8 bytes per cell and iteration that are
// neither written nor read: 8192^2, k_search_apply 296-314 -> 232-239 us, this kernel 210-214 -> 209-223 us.
#ifndef PT_RECOMP_BLOCKS
#define PT_RECOMP_BLOCKS 1
#endif
// CMODE: 0 no coarse part, 1 two-level mode (three sums per tile), 2 multilevel mode (the bilinear restriction: 48 sums per tile) - a template parameter so that the
// tile-local mode's own instantiation keeps its registers (151: three waves per SIMD)
template <int W, bool RECOMP = false, int CMODE = 0>
__global__ __launch_bounds__(PT_THREADS, RECOMP ? PT_RECOMP_BLOCKS : 1) void k_precond_tile(TileArgs a) {
  if (!a.force && (a.zform == 2 ? a.sc->zfix == 0 : pcg_idle(a.sc))) return;
  const int lane = threadIdx.x & 63;
  const int ntb = a.g.T / W, total = a.nb_local * ntb;
  const int n_waves = gridDim.x * (PT_THREADS / 64);
  const double nalpha = -(a.force ? a.alpha_arg : a.sc->alpha);
  double mx = 0.0, dsum = 0.0;
  const bool listed = W == 16 && a.list != nullptr;
  const int todo = listed ? (int)a.sc->n_chunks : total;
  // E^-1 of an interior tile, the same for all of them (k_tile_table): in LDS for the whole launch
  constexpr int TABP = W == 16 ? 8 : 1;
  __shared__ sw_d2 s_tab[TABP][64];
  __shared__ double s_cpart[CMODE == 2 ? PT_THREADS / 64 : 1][CMODE == 2 ? 16 * 2 * MG_NSLOT : 1];      // multilevel mode: a wave's partial sums on their way out
  (void)s_cpart;
  const bool have_tab = W == 16 && listed && a.table != nullptr;
  if (have_tab) {
    for (int k = threadIdx.x; k < TABP * 64; k += PT_THREADS) (&s_tab[0][0])[k] = reinterpret_cast<const sw_d2*>(a.table)[k];
    __syncthreads();
  }
  typedef std::integral_constant<bool, true> yes_t;
  typedef std::integral_constant<bool, false> no_t;
  for (int i = blockIdx.x * (PT_THREADS / 64) + (threadIdx.x >> 6); i < todo; i += n_waves) {
    // (reverse: start where the previous pass - k_search_apply, ascending - ended, i.e. on what the Infinity Cache still holds)
    const int ii = a.reverse ? todo - 1 - i : i;
    const unsigned int ent = listed ? a.list[ii] : (unsigned int)ii;
    const bool interior = have_tab && (ent & EU_CHUNK_INTERIOR) != 0;
    const int tile = (int)(listed ? ent & ~EU_CHUNK_INTERIOR : ent);
    const int band = a.band_lo + tile / ntb, k = tile % ntb;
    const size_t base = ((size_t)band * a.g.TS + (size_t)k * W) * 64 + 2 * lane;
    auto run = [&](auto full_tag) {
      constexpr bool FULL = decltype(full_tag)::value;      // interior tile: masks are constants, precon comes from the table
      unsigned int mm[W / 2];
      unsigned int any = 0;
#pragma unroll
      for (int P = 0; P < W / 2; ++P) {
        mm[P] = FULL ? (unsigned int)(CM_INTERIOR | (CM_INTERIOR << 8)) : (unsigned int)*reinterpret_cast<const unsigned short*>(a.mask + base + P * 128);
        any |= mm[P];
      }
      if (!FULL && !listed && !__ballot(((any | (any >> 8)) & CM_FLUID) != 0)) return;     // no fluid in this tile: r, z stay +0 there
      sw_d2 rr[W / 2], qq[W / 2], pp[W / 2];
#pragma unroll
      for (int P = 0; P < W / 2; ++P) {
        rr[P] = *reinterpret_cast<const sw_d2*>(a.r + base + P * 128);
        if (RECOMP && a.rupd) continue;              // (E^-1 is fetched behind the r update: PT_RECOMP_LATE)
        if (!a.sweeps) pp[P] = sw_d2{0.0, 0.0};      // (the r update alone - the parity mode's use of this kernel - needs no E^-1)
        else if (FULL) pp[P] = s_tab[P < TABP ? P : 0][lane];
        else pp[P] = *reinterpret_cast<const sw_d2*>(a.pre + base + P * 128);
        if (!RECOMP && a.rupd) qq[P] = *reinterpret_cast<const sw_d2*>(a.as + base + P * 128);
      }
      if (RECOMP && a.rupd) {
        const int npairs = a.g.TS / 2, P0 = k * (W / 2);
        sw_d2 ss[W / 2 + 2];
#pragma unroll
        for (int P = -1; P <= W / 2; ++P)
          ss[P + 1] = (P0 + P >= 0 && P0 + P < npairs) ? *reinterpret_cast<const sw_d2*>(a.as + base + (long long)P * 128) : sw_d2{0.0, 0.0};
        // lane L < 16: s' of the cell below lane 0's cell of record k W + L (column k W + L, row 64 band - 1);
        // lane L >= 48: of the cell above lane 63's cell of record k W + L - 48 (column k W + L - 48 - 63, row 64 (band + 1))
        double ev = 0.0;
        if (lane < 16) {
          const int x = k * W + lane;
          if (x < a.g.X) {
            if (a.gs_lo && band == a.band_lo) ev = a.gs_lo[x];
            else if (band > 0) ev = a.as[skew_index(a.g, x, 64 * band - 1)];
          }
        } else if (lane >= 48) {
          const int x = k * W + lane - 48 - 63;
          if (x >= 0 && x < a.g.X) {
            if (a.gs_hi && band == a.band_lo + a.nb_local - 1) ev = a.gs_hi[x];
            else if (band + 1 < a.g.nbands) ev = a.as[skew_index(a.g, x, 64 * (band + 1))];
          }
        }
        const int ev_lo = __double2loint(ev), ev_hi = __double2hiint(ev);
#pragma unroll
        for (int P = 0; P < W / 2; ++P) {
          const unsigned int m0 = mm[P] & 0xff, m1 = mm[P] >> 8;
          const sw_d2 cc = ss[P + 1];
          const double prev_y = ss[P].y, nxt_x = ss[P + 2].x;
          const double d0 = __hiloint2double(__builtin_amdgcn_readlane(ev_hi, 2 * P), __builtin_amdgcn_readlane(ev_lo, 2 * P));
          const double d1 = __hiloint2double(__builtin_amdgcn_readlane(ev_hi, 2 * P + 1), __builtin_amdgcn_readlane(ev_lo, 2 * P + 1));
          const double u0 = __hiloint2double(__builtin_amdgcn_readlane(ev_hi, 48 + 2 * P), __builtin_amdgcn_readlane(ev_lo, 48 + 2 * P));
          const double u1 = __hiloint2double(__builtin_amdgcn_readlane(ev_hi, 49 + 2 * P), __builtin_amdgcn_readlane(ev_lo, 49 + 2 * P));
          const double dn0 = wave_shift_inject<DPP_WAVE_SHR1>(prev_y, d0), up0 = wave_shift_inject<DPP_WAVE_SHL1>(cc.y, u0);
          const double dn1 = wave_shift_inject<DPP_WAVE_SHR1>(cc.x, d1), up1 = wave_shift_inject<DPP_WAVE_SHL1>(nxt_x, u1);
          double v = (double)(int)(m0 >> CM_DIAG_SHIFT) * cc.x;      // apply_a (main.c:679-691): diag, right, up, left, down
          v = v - ((m0 & CM_RIGHT) ? cc.y : 0.0);
          v = v - ((m0 & CM_UP) ? up0 : 0.0);
          v = v - ((m0 & CM_LEFT) ? prev_y : 0.0);
          v = v - ((m0 & CM_DOWN) ? dn0 : 0.0);
          // r -= alpha A s' (fmadd, main.c:754) and max |r| over fluid cells, as below
          if (m0 & CM_FLUID) { rr[P].x = rr[P].x + v * nalpha; const double w = fabs(rr[P].x); if (w > mx) mx = w; }
          v = (double)(int)(m1 >> CM_DIAG_SHIFT) * cc.y;
          v = v - ((m1 & CM_RIGHT) ? nxt_x : 0.0);
          v = v - ((m1 & CM_UP) ? up1 : 0.0);
          v = v - ((m1 & CM_LEFT) ? cc.x : 0.0);
          v = v - ((m1 & CM_DOWN) ? dn1 : 0.0);
          if (m1 & CM_FLUID) { rr[P].y = rr[P].y + v * nalpha; const double w = fabs(rr[P].y); if (w > mx) mx = w; }
          *reinterpret_cast<sw_d2*>(a.r + base + P * 128) = rr[P];
        }
      }
      if (!RECOMP && a.rupd) {      // r -= alpha z (fmadd, main.c:754, evaluated as r + z * (-alpha) like k_update_pr) and max |r| over fluid cells
#pragma unroll
        for (int P = 0; P < W / 2; ++P) {
          if (mm[P] & CM_FLUID) { rr[P].x = rr[P].x + qq[P].x * nalpha; const double v = fabs(rr[P].x); if (v > mx) mx = v; }
          if ((mm[P] >> 8) & CM_FLUID) { rr[P].y = rr[P].y + qq[P].y * nalpha; const double v = fabs(rr[P].y); if (v > mx) mx = v; }
          *reinterpret_cast<sw_d2*>(a.r + base + P * 128) = rr[P];
        }
      }
      if (!a.sweeps) return;
      if (W == 16 && CMODE == 2) {
        // multilevel mode (k_mg.hip; the sums are gathered by mg_gather0, k_mg.h): P_0^T r of this tile, P_0 bilinear from the nodes at the cells (G0 J + G0 / 2, G0 I + G0 / 2), G0 = MG_G0 = 8.  The eight lanes of a GROUP
        // (k_mg.h) lie between the same two node rows I0, I0 + 1; a lane's 16 columns between at most MG_NSEG + 1 node columns starting at Jb (its own), the group's between
        // MG_NSLOT = 4 starting at Jq.  A record's weight of the right-hand node is rec + b with b constant over a segment, so a lane accumulates sum rv and sum rec rv per
        // segment, turns them into its node-column sums, shifts them to the group's slots and multiplies by its two row weights (weights in 1 / G0)
        const int quad = lane >> 2, G = (lane + 4) >> 3;      // the group: lanes 8 G - 4 .. 8 G + 3 (k_mg.h)
        const int uy = 64 * band + lane - MG_G0 / 2, I0 = uy >> MG_LOG;
        double wy1 = (double)(uy & (MG_G0 - 1)), wy0 = (double)MG_G0 - wy1;
        if (I0 < 0) { wy0 = 0.0; wy1 = (double)MG_G0; }
        if (I0 >= a.cny - 1) { wy0 = (double)MG_G0; wy1 = 0.0; }
        const int x0 = 16 * k - lane - MG_G0 / 2, Jb = x0 >> MG_LOG, tbase = MG_G0 * Jb - x0;      // tbase in (-G0, 0]: records >= tbase + G0 m lie in segment m
        const int Jq = 2 * k - G - 1;      // the group's first node column: Jb - Jq is 1 for the group's first lane (whose third segment is empty), 0 for the others
        double sg_s[MG_NSEG], sg_t[MG_NSEG];
#pragma unroll
        for (int m = 0; m < MG_NSEG; ++m) { sg_s[m] = 0.0; sg_t[m] = 0.0; }
#pragma unroll
        for (int j = 0; j < W; ++j) {
          const int cm = (int)((mm[j >> 1] >> ((j & 1) * 8)) & 0xff);
          const double rv = (cm & CM_FLUID) ? ((j & 1) ? rr[j >> 1].y : rr[j >> 1].x) : 0.0;
          const double jv = rv * (double)j;
#pragma unroll
          for (int m = 0; m < MG_NSEG; ++m) {
            const bool in = (m == 0 || j >= tbase + MG_G0 * m) && (m == MG_NSEG - 1 || j < tbase + MG_G0 * (m + 1));
            sg_s[m] += in ? rv : 0.0; sg_t[m] += in ? jv : 0.0;
          }
        }
        double cn[MG_NSEG + 1];
#pragma unroll
        for (int m = 0; m <= MG_NSEG; ++m) cn[m] = 0.0;
#pragma unroll
        for (int m = 0; m < MG_NSEG; ++m) {
          double u1 = sg_t[m] + (double)(-tbase - MG_G0 * m) * sg_s[m], u0 = (double)MG_G0 * sg_s[m] - u1;      // weights of the nodes Jb + m + 1 / Jb + m
          if (Jb + m < 0) { u0 = 0.0; u1 = (double)MG_G0 * sg_s[m]; }                                             // beyond the outermost nodes: constant
          if (Jb + m >= a.cnx - 1) { u0 = (double)MG_G0 * sg_s[m]; u1 = 0.0; }
          cn[m] += u0; cn[m + 1] += u1;
        }
        const bool shifted = Jb != Jq;
        wy0 *= 1.0 / (MG_G0 * MG_G0); wy1 *= 1.0 / (MG_G0 * MG_G0);
        // Two DPP steps add the products over a quad; the two quads of a group meet in a row of LDS on the way out, and the tile's MG_PART sums leave as ONE contiguous
        // piece of LDS; they leave as nine pieces of eight doubles (below; single scattered doubles cost 44 us per pass at 8192^2, rounds 3-5 wrote one piece of 72 per tile)
        double* sp = s_cpart[threadIdx.x >> 6];
#pragma unroll
        for (int q = 0; q < MG_NSLOT; ++q) {
          const double lo = cn[q], hi = q >= 1 ? cn[q - 1] : 0.0;
          const double cs = shifted ? hi : lo;
          const double p0 = group_sum(wy0 * cs), p1 = group_sum(wy1 * cs);
          if ((lane & 3) == 0) { sp[quad * 2 * MG_NSLOT + q] = p0; sp[quad * 2 * MG_NSLOT + MG_NSLOT + q] = p1; }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        {
          // [band][group][tile][row slot][column slot] (round 6; [band][tile][group][row slot][column slot] before): a tile leaves nine whole 64-byte lines, next to its
          // neighbours' - what a node row of k_mg_down1 gathers (two tiles' slots per node, node after node) is then CONTIGUOUS: the gather fetched 3.5 x the bytes it used
          double* cp = a.cpart + ((size_t)(tile / ntb) * MG_NGRP * ntb + (size_t)k) * (2 * MG_NSLOT);
#pragma unroll
          for (int u = 0; u < (MG_PART + 63) / 64; ++u) {
            const int e = lane + 64 * u;
            if (e < MG_PART) {
              const int g = e / (2 * MG_NSLOT), w = e % (2 * MG_NSLOT);      // group g = quads 2 g - 1 and 2 g (the half groups: quad 0 / quad 15 alone)
              const double va = g > 0 ? sp[(2 * g - 1) * 2 * MG_NSLOT + w] : 0.0, vb = g < 8 ? sp[(2 * g) * 2 * MG_NSLOT + w] : 0.0;
              cp[((size_t)g * ntb) * (2 * MG_NSLOT) + w] = va + vb;
            }
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        __builtin_amdgcn_wave_barrier();
      } else if (W == 16 && CMODE == 1) {      // P^T r of this tile: cell (lane, record k W + j) sits in column k W + j - lane; at most three coarse columns per tile
        const int xl = k * W - 63, J0 = (xl > 0 ? xl : 0) >> a.cshift;
        double c0 = 0.0, c1 = 0.0, c2 = 0.0;
#pragma unroll
        for (int j = 0; j < W; ++j) {
          const int cm = (int)((mm[j >> 1] >> ((j & 1) * 8)) & 0xff);
          const double rv = (cm & CM_FLUID) ? ((j & 1) ? rr[j >> 1].y : rr[j >> 1].x) : 0.0;
          const int x = k * W + j - lane;
          const int b = ((x > 0 ? x : 0) >> a.cshift) - J0;
          c0 += b == 0 ? rv : 0.0; c1 += b == 1 ? rv : 0.0; c2 += b == 2 ? rv : 0.0;
        }
        c0 = eu_wave_sum(c0); c1 = eu_wave_sum(c1); c2 = eu_wave_sum(c2);
        if (lane == 0) { double* cp = a.cpart + (size_t)tile * 3; cp[0] = c0; cp[1] = c1; cp[2] = c2; }
      }
      if (RECOMP && a.rupd) {      // the window of s' is dead: E^-1 takes its registers (the barrier keeps the compiler from hoisting these loads above the r update)
        asm volatile("" ::: "memory");
#pragma unroll
        for (int P = 0; P < W / 2; ++P) pp[P] = FULL ? s_tab[P < TABP ? P : 0][lane] : *reinterpret_cast<const sw_d2*>(a.pre + base + P * 128);
      }
      // z = M_tile^-1 r (L q = r, L^T z = q: main.c:602-626) with dot(z, r) on the fly
      tile_solve<W, true>(mm, rr, pp, qq, dsum);
      if (W == 16 && a.zform == 1) {      // (wave-uniform) "z halo only": what the next k_search_apply<.., ZR> cannot form itself (ZrArgs)
        double* h = a.zhalo + ((size_t)band * ntb + k) * 128;
        h[lane] = qq[0].x;
        h[64 + lane] = qq[W / 2 - 1].y;
        if (lane == 0 || lane == 63) {
          double* row = a.zrows + ((size_t)band * 2 + (lane == 63 ? 1 : 0)) * a.g.X;
#pragma unroll
          for (int j = 0; j < W; ++j) {
            const int x = k * W + j - lane;      // the lane's column in record k W + j
            if (x >= 0 && x < a.g.X) row[x] = (j & 1) ? qq[j >> 1].y : qq[j >> 1].x;
          }
        }
      } else {
#pragma unroll
        for (int P = 0; P < W / 2; ++P) *reinterpret_cast<sw_d2*>(a.z + base + P * 128) = qq[P];
      }
      if (band == a.edge_lo || band == a.edge_hi) {      // (wave-uniform) the rows the neighbouring slabs need, as compact rows
        const bool lo = band == a.edge_lo && lane == 0, hi = band == a.edge_hi && lane == 63;
#pragma unroll
        for (int j = 0; j < W; ++j) {
          const double zv = (j & 1) ? qq[j >> 1].y : qq[j >> 1].x;
          const int x_lo = k * W + j, x_hi = k * W + j - 63;      // the column of lane 0 / lane 63 in record k W + j
          if (lo && x_lo < a.g.X) a.zsend_lo[x_lo] = zv;
          if (hi && x_hi >= 0 && x_hi < a.g.X) a.zsend_hi[x_hi] = zv;
        }
      }
    };
    if (W == 16 && interior) run(yes_t()); else run(no_t());
  }
  // ---- the two reductions: block -> partials -> the last block folds them in index order and applies the scalar epilogues
  tile_block_reduce(mx, dsum);
  __shared__ int am_last;
  if (threadIdx.x == 0) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(&a.part_max[blockIdx.x]), (unsigned long long)__double_as_longlong(mx), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(&a.part_dot[blockIdx.x]), (unsigned long long)__double_as_longlong(dsum), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned int t = __hip_atomic_fetch_add(a.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    am_last = t == gridDim.x - 1;
  }
  __syncthreads();
  if (!am_last) return;
  double vmax = 0.0, vsum = 0.0;
  for (unsigned int i = threadIdx.x; i < gridDim.x; i += PT_THREADS) {
    const double m = __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<unsigned long long*>(&a.part_max[i]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    const double d = __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<unsigned long long*>(&a.part_dot[i]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    vmax = m > vmax ? m : vmax; vsum += d;
  }
  tile_block_reduce(vmax, vsum);
  if (a.via == FIN_VIA_P2P) {      // uniform: every thread of this block is here
    if (a.rupd) vmax = p2p_allreduce_block<true>(a.sc, vmax);
    if (a.fin_dot >= 0) vsum = p2p_allreduce_block<false>(a.sc, vsum);
  }
  if (threadIdx.x == 0) {
    if (a.via == FIN_TO_COMM) { a.pair_slot[0] = vmax; a.pair_slot[1] = vsum; }   // the epilogues run after the all-gather (k_pair_fold)
    else {
      if (a.rupd) pcg_scalar_step(a.sc, FIN_RNORM, vmax);
      if (a.fin_dot >= 0 && !(a.rupd && a.sc->done)) pcg_scalar_step(a.sc, a.fin_dot, vsum);
    }
    if (a.zform >= 0) a.sc->zfix = a.zform == 1 ? 1u : 0u;
    __hip_atomic_store(a.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// max |r| and dot(z,r) of all ranks after ONE exchange ("fuse the latter two into one ... message pair"): every rank
// folds the gathered pairs in rank order - identical bits everywhere - and applies the two scalar epilogues
__global__ void k_pair_fold(PcgScalars* sc, const double* __restrict__ pairs, int stride, int R, int rupd, int fin_dot, int force) {
  if (!force && pcg_idle(sc)) return;
  double vmax = 0.0, vsum = 0.0;
  for (int r = 0; r < R; ++r) { vmax = pairs[(size_t)stride * r] > vmax ? pairs[(size_t)stride * r] : vmax; vsum += pairs[(size_t)stride * r + 1]; }
  if (rupd) pcg_scalar_step(sc, FIN_RNORM, vmax);
  if (fin_dot >= 0 && !(rupd && sc->done)) pcg_scalar_step(sc, fin_dot, vsum);
}
static TileArgs make_tile_args(euler_sim* S, int force) {
  TileArgs a;
  a.g = S->geom; a.mask = S->cellmask; a.pre = S->precon; a.r = S->r; a.as = S->tile_as_override ? S->tile_as_override : S->q; a.z = S->z;
  a.band_lo = S->band_lo; a.nb_local = S->band_hi - S->band_lo;
  a.rupd = 0; a.sweeps = 1; a.fin_dot = -1;
  a.via = S->has_comm ? (S->p2p_on ? (int)FIN_VIA_P2P : (int)FIN_TO_COMM) : 0;
  a.part_max = S->partial; a.part_dot = S->partial2; a.counter = S->red_counter; a.sc = S->sc; a.force = force; a.alpha_arg = 0.0;
  a.pair_slot = S->pair_buf + 2 * (S->has_comm ? S->comm.rank : 0);
  a.list = !force ? S->chunk_list : nullptr;      // (tiles of 16 records only; forced single operations may run on masks no solve has listed)
  a.table = S->tile_table;
  a.zsend_lo = a.zsend_hi = nullptr; a.edge_lo = a.edge_hi = -1;
  // descending: k_search_apply walks the chunks upwards, so this pass starts on what the Infinity Cache still holds of it - and ends
  // where the next k_search_apply starts.  8192^2: 548 -> 536 us per iteration (EULER_OPT_TILE_REVERSE 0 restores the ascending order)
  a.reverse = S->opt[EULER_OPT_TILE_REVERSE] != 0;
  a.cpart = nullptr; a.cshift = 0; a.cmode = 0; a.cnx = a.cny = 0;
  a.gs_lo = a.gs_hi = nullptr;
  a.zform = -1; a.zhalo = S->zhalo; a.zrows = S->zrows;
  if (ghost_mode(S)) {
    if (S->band_lo > 0) { a.zsend_lo = xrow(S, XR_ZSEND_LO); a.edge_lo = S->band_lo; }
    if (S->band_hi < S->geom.nbands) { a.zsend_hi = xrow(S, XR_ZSEND_HI); a.edge_hi = S->band_hi - 1; }
  }
  return a;
}
static inline unsigned tile_blocks(const euler_sim* S, int w) {      // one wave per tile of w records, at most 2048 blocks (the partials)
  return eu_blocks((size_t)(S->band_hi - S->band_lo) * (S->geom.T / w), PT_THREADS / 64, 2048);
}
typedef void (*TileKernel)(TileArgs);
int eu_launch_factor_tile(euler_sim* S, int force) {
  const TileKernel k = S->tile_w == 8 ? k_factor_tile<8> : S->tile_w == 32 ? k_factor_tile<32> : k_factor_tile<16>;
  LAUNCH(S, KC_PRECON_FACTOR, k, dim3(tile_blocks(S, S->tile_w)), dim3(PT_THREADS), make_tile_args(S, force));
  return EULER_OK;
}
// [r -= alpha A s, max |r|,] z = M^-1 r, dot(z, r) with its scalar epilogue fin_dot (FIN_SIGMA_INIT / FIN_BETA / FIN_STORE_ONLY)
// r_only: the kernel's first half alone - r -= alpha A s and max |r| with its epilogue (`done`) - over 16-record chunks whatever the
// handle's tile width: how EVERY non-tile configuration (the reference's IC(0), Jacobi) updates r since round 3 (p rides in k_search_apply)
int eu_launch_precond_tile(euler_sim* S, int rupd, int sweeps, int fin_dot, int force, double alpha, bool r_only, int zform) {
  const bool seq = S->cfg.dot_mode == EULER_DOT_SEQUENTIAL && !S->has_comm;
  TileArgs a = make_tile_args(S, force);
  a.rupd = rupd; a.sweeps = sweeps; a.fin_dot = (seq || !sweeps) ? -1 : fin_dot; a.alpha_arg = alpha;
  a.zform = zform;
  // two-level mode: the tile pass also leaves P^T r per tile and only STORES its share of dot(z, r); k_coarse_solve adds the coarse
  // share and applies the epilogue
  const bool two_level = eu_is_two_level(S) && sweeps && !r_only && !force && a.list != nullptr;
  const int fin_real = a.fin_dot;
  if (two_level) {
    const bool mg = eu_is_mg(S);
    a.cpart = mg ? S->mg_part : S->cc_part; a.cshift = mg ? 0 : S->coarse_shift;
    a.cmode = mg ? 2 : 1; a.cnx = mg ? S->mg_nx[0] : 0; a.cny = mg ? S->mg_ny[0] : 0;
    if (a.fin_dot >= 0) a.fin_dot = FIN_STORE_ONLY;
  }
  // row slabs + coarse correction: the pair and this rank's rows of the level-0 right-hand side travel in ONE slot of ONE all-gather inside the G1 exchange
  double* xsmall = S->pair_buf;
  int nsmall = 2;
  bool split = false;      // multilevel mode: the cycle split by rows (k_mg_split.hip) - the edge rows of z go straight into its messages
  if (two_level && a.via == FIN_TO_COMM) {
    split = eu_is_mg(S) && ghost_mode(S) && eu_mg_split(S);
    nsmall = eu_coarse_comm_slots(S);
    if (nsmall < 0) return EULER_ENOMEM;
    xsmall = S->mg_xbuf;
    a.pair_slot = xsmall + (size_t)S->comm.rank * nsmall;
    if (split) {
      if (a.zsend_lo) a.zsend_lo = eu_mg_split_msg(S, 0);
      if (a.zsend_hi) a.zsend_hi = eu_mg_split_msg(S, 1);
    }
  }
  const int w = r_only ? 16 : S->tile_w, cls = r_only ? KC_UPDATE_PR : zform == 2 ? KC_MISC : KC_PRECOND_TILE;      // (the pass at the end of a solve is not an iteration's)
  // (r_only: the other modes' r update - A s' would sit in q behind k_search_apply, in z behind the solve's first k_apply_a, which stores it)
  const bool recomp = rupd && !force && tile_recompute(S) && (r_only ? S->tile_as_override == S->q : !S->tile_as_override);
  if (recomp) {      // A s' is formed from the search direction (S->s behind k_search_apply's swap, or s_0 behind k_apply_a) and, on row slabs, the ghost rows of s' of its generation
    a.as = S->s;
    if (ghost_mode(S)) {
      if (S->band_lo > 0) a.gs_lo = xrow(S, XR_GS_LO0 + S->gs_cur);
      if (S->band_hi < S->geom.nbands) a.gs_hi = xrow(S, XR_GS_HI0 + S->gs_cur);
    }
  }
  const TileKernel k = w == 8 ? k_precond_tile<8> : w == 32 ? k_precond_tile<32>
                     : a.cmode == 2 ? (recomp ? k_precond_tile<16, true, 2> : k_precond_tile<16, false, 2>)
                     : a.cmode == 1 ? (recomp ? k_precond_tile<16, true, 1> : k_precond_tile<16, false, 1>)
                     : (recomp ? k_precond_tile<16, true> : k_precond_tile<16>);
  LAUNCH(S, cls, k, dim3(tile_blocks(S, w)), dim3(PT_THREADS), a);
  if (two_level && a.via != FIN_TO_COMM) { int rc = eu_launch_coarse_solve(S, fin_real, force); if (rc) return rc; }
  // the reference's row-major dot(z, r), a no-op once max |r| <= tol.  `seq` is exactly the condition under which eu_launch_dot replays the dot with k_dot_sequential
  // (k_pcg.hip: that kernel lives there); whoever changes one of the two conditions changes the other
  if (seq && sweeps && fin_dot >= 0) eu_launch_dot(S, S->z, S->r, fin_dot, force);
  if (a.via == FIN_TO_COMM) {          // no mailboxes: G1 - both results (and, in the solve, the edge rows of the new z) in ONE exchange, then the epilogues
    const int R = S->comm.nranks;
    const bool rows = ghost_mode(S) && !force;
    int rc = !two_level ? EULER_OK : split ? eu_mg_split_pre(S) : eu_launch_coarse_pre(S, force);
    if (rc) return rc;
    if (split) rc = eu_comm_exchange(S, eu_mg_split_msg(S, 0), eu_mg_split_msg(S, 1), eu_mg_split_msg(S, 2), eu_mg_split_msg(S, 3), eu_mg_split_count(S), xsmall, nsmall);
    else rc = eu_comm_exchange(S, xrow(S, XR_ZSEND_LO), xrow(S, XR_ZSEND_HI), xrow(S, XR_ZRECV_LO), xrow(S, XR_ZRECV_HI), rows ? S->X : 0, xsmall, nsmall);
    if (rc) return rc;
    hipLaunchKernelGGL(k_pair_fold, dim3(1), dim3(1), 0, S->stream, S->sc, xsmall, nsmall, R, rupd, a.fin_dot, force);
    if (split) {      // a third exchange point: the ranks' shares of the correction's dot product (and of the gauge sums) live on their own rows
      if ((rc = eu_mg_split_mid(S, fin_real, force, xrow(S, XR_ZRECV_LO), xrow(S, XR_ZRECV_HI)))) return rc;
      if ((rc = eu_comm_exchange(S, nullptr, nullptr, nullptr, nullptr, 0, eu_mg_split_gc(S), 1 + MG_NULL_MAX))) return rc;
      return eu_mg_split_fold(S, fin_real, force);
    }
    // coarse correction on row slabs: the tiles' shares of dot(z, r) are folded (stored, not applied); the V-cycle - its level-0 right-hand
    // side the sum of the ranks' shares, the rest replicated - adds its share and applies the epilogue, the same bits on every rank
    if (two_level) { rc = eu_launch_coarse_scatter(S); if (rc) return rc; rc = eu_launch_coarse_solve(S, fin_real, force); if (rc) return rc; }
  }
  return EULER_OK;
}
