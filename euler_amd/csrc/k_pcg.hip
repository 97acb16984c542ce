// k_pcg.hip — the pressure solve: preconditioned conjugate gradient on the masked 5-point
// Laplacian (reference project(), main.c:709-767, and its kernels main.c:580-702): the element-wise kernels, the exchanges and the host driver.
// The arrays' layout and what the solver's files share: k_pcg.h; the parity mode's sweeps: k_sweep.hip; the tile-local passes: k_tile.hip (k_precond_tile) and k_search.hip (k_search_apply).
#include "k_pcg.h"

#include <cmath>
#include <vector>

// second stage: one workgroup folds the per-block partials in a fixed order
template <bool IS_MAX>
__global__ __launch_bounds__(RED_THREADS) void k_reduce_final(const double* __restrict__ partial, int n, PcgScalars* sc,
                                                              int op, int force) {
  if (!force && pcg_idle(sc)) return;
  double v = 0.0;
  for (int i = threadIdx.x; i < n; i += RED_THREADS) {
    const double w = partial[i];
    if (IS_MAX) v = w > v ? w : v; else v += w;
  }
  v = IS_MAX ? block_max(v) : block_sum(v);
  if (threadIdx.x == 0) pcg_scalar_step(sc, op, v);
}

// dot(a,b) over fluid cells -> per-block partials (tree mode); layout-agnostic.  EDGES: `a` is z of a slab (see above).
template <bool EDGES>
__global__ __launch_bounds__(RED_THREADS) void k_dot_partial(const double* __restrict__ a, const double* __restrict__ b,
                                                             const uint8_t* __restrict__ mask, size_t S,
                                                             double* __restrict__ partial, PcgScalars* sc, int force,
                                                             unsigned int* counter, int fin_op, int TS, int nb_local, int edges) {
  if (!force && pcg_idle(sc)) return;
  const size_t chunk = (((S + gridDim.x - 1) / gridDim.x) + 1) & ~(size_t)1;   // S is even: whole 16-byte pairs per thread
  const size_t lo = (size_t)blockIdx.x * chunk, hi = lo + chunk < S ? lo + chunk : S;
  double t = 0.0;
  for (size_t i = lo + 2 * (size_t)threadIdx.x; i < hi; i += 2 * RED_THREADS) {
    const unsigned int mm = *reinterpret_cast<const unsigned short*>(mask + i);
    if (!((mm | (mm >> 8)) & CM_FLUID)) continue;
    const sw_d2 av = *reinterpret_cast<const sw_d2*>(a + i), bv = *reinterpret_cast<const sw_d2*>(b + i);
    if (mm & CM_FLUID) t += av.x * bv.x;
    if ((mm >> 8) & CM_FLUID) t += av.y * bv.y;
    if (EDGES && slab_edge_row(i, (int)((i & 127) >> 1), TS, nb_local, edges)) {
      if (mm & CM_FLUID) st_system(a + i, av.x);
      if ((mm >> 8) & CM_FLUID) st_system(a + i + 1, av.y);
    }
  }
  if (EDGES) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every thread's write-through stores have landed (block_sum syncs)
  t = block_sum(t);
  block_finish<false>(t, partial, counter, sc, fin_op);
}

// dot(a,b) replayed in the reference's ROW-MAJOR order (main.c:629-639): bit-identical; for small grids (and every bit-exact test).
// The running sum is ONE dependent chain of additions - nothing can split it - so the kernel is built around keeping that chain fed: wave 0's first lane
// adds while waves 1..3 gather the NEXT tile's products (a[i] b[i] of fluid cells, +0.0 elsewhere) into the other half of a double buffer, one
// barrier per tile.  Two things shorten the chain itself, both exact: a group of 64 consecutive cells without fluid is skipped (its ballot is 0), and inside a
// group every entry is added, fluid or not - x + (+0.0) = x for every x except -0.0, and the sum is never -0.0 (it starts as +0.0, and +0.0 + -0.0 = +0.0) -
// which makes the inner loop branch-free: 64 LDS reads in flight, 64 dependent v_add_f64.  Round 3's form (a branch and an LDS round trip per cell, the
// gather not overlapped) took ~1.5 ms per dot at 384 x 448 and was most of the GPU suite's wall time.
#define SEQ_TILE 4096
__global__ __launch_bounds__(256) void k_dot_sequential(const double* __restrict__ a, const double* __restrict__ b,
                                                        const uint8_t* __restrict__ mask, SkewGeom g, PcgScalars* sc,
                                                        int op, int force) {
  if (!force && pcg_idle(sc)) return;
  __shared__ double prod[2][SEQ_TILE];
  __shared__ unsigned long long any[2][SEQ_TILE / 64];
  const size_t C = (size_t)g.X * g.Y;
  const int ntiles = (int)((C + SEQ_TILE - 1) / SEQ_TILE);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double total = 0.0;   // `double total = 0.f`
  for (int tile = -1; tile < ntiles; ++tile) {
    if (wave > 0 && tile + 1 < ntiles) {            // gather tile + 1
      const int buf = (tile + 1) & 1;
      const size_t base = (size_t)(tile + 1) * SEQ_TILE;
      for (int grp = wave - 1; grp < SEQ_TILE / 64; grp += 3) {
        const size_t c = base + (size_t)grp * 64 + lane;
        bool f = false;
        double pr = 0.0;
        if (c < C) {
          const size_t i = skew_index(g, (int)(c % g.X), (int)(c / g.X));
          f = (mask[i] & CM_FLUID) != 0;
          if (f) pr = a[i] * b[i];
        }
        prod[buf][grp * 64 + lane] = pr;
        const unsigned long long bal = __ballot(f);
        if (lane == 0) any[buf][grp] = bal;
      }
    }
    if (threadIdx.x == 0 && tile >= 0) {            // the chain over tile
      const int buf = tile & 1;
      for (int grp = 0; grp < SEQ_TILE / 64; ++grp) {
        if (any[buf][grp] == 0ull) continue;
        const double* pp = &prod[buf][grp * 64];
        double v[64];
#pragma unroll
        for (int k = 0; k < 64; ++k) v[k] = pp[k];
#pragma unroll
        for (int k = 0; k < 64; ++k) total += v[k];
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) pcg_scalar_step(sc, op, total);
}

// ------------------------------------------------------------------------------------------
// apply_a (main.c:679-691): z = A s on fluid cells (other entries of z stay 0).
// In tree mode the block also leaves its partial of dot(z,s).
__global__ __launch_bounds__(RED_THREADS) void k_apply_a(const double* __restrict__ s, double* __restrict__ z,
                                                         const uint8_t* __restrict__ mask, SkewGeom g,
                                                         double* __restrict__ partial, PcgScalars* sc, int force,
                                                         unsigned int* counter, int fin_op) {
  if (!force && pcg_idle(sc)) return;
  const size_t S = g.S;
  const size_t chunk = (((S + gridDim.x - 1) / gridDim.x) + 127) & ~(size_t)127;   // whole record pairs per block
  const size_t lo = (size_t)blockIdx.x * chunk, hi = lo + chunk < S ? lo + chunk : S;
  double t = 0.0;
  // One thread per PAIR of records of a lane (euler_dev.h): elements i = (t even, l) and i+1 = (t+1, l) come
  // with one 16-byte load and are each other's right / left neighbour.  The others:
  //   even element: left (t-1, l) = i-127, up (t+1, l+1) = i+3, down (t-1, l-1) = i-129
  //   odd element : right (t+2, l) = i+128, up (t+2, l+1) = i+130, down (t, l-1) = i-2
  // (the adjacent band's lane 0 / 63 through the index function when l = 63 / 0).
  for (size_t i = lo + 2 * (size_t)threadIdx.x; i < hi; i += 2 * RED_THREADS) {
    const unsigned int mm = *reinterpret_cast<const unsigned short*>(mask + i);
    const unsigned int m0 = mm & 0xff, m1 = mm >> 8;
    if (!((m0 | m1) & CM_FLUID)) continue;
    const sw_d2 c = *reinterpret_cast<const sw_d2*>(s + i);
    const int l = (int)((i & 127) >> 1);
    sw_d2 o = {0.0, 0.0};
    if (m0 & CM_FLUID) {
      double v = (double)(int)(m0 >> CM_DIAG_SHIFT) * c.x;
      v = v - ((m0 & CM_RIGHT) ? c.y : 0.0);
      if (m0 & CM_UP) {
        size_t up = i + 3;
        if (l == 63) { int band, tt, ll; skew_decode(g, i, band, tt, ll); up = skew_index(g, tt - 63, 64 * (band + 1)); }
        v = v - s[up];
      } else {
        v = v - 0.0;
      }
      v = v - ((m0 & CM_LEFT) ? s[i - 127] : 0.0);
      if (m0 & CM_DOWN) {
        size_t dn = i - 129;
        if (l == 0) { int band, tt, ll; skew_decode(g, i, band, tt, ll); dn = skew_index(g, tt, 64 * band - 1); }
        v = v - s[dn];
      } else {
        v = v - 0.0;
      }
      o.x = v;
      t += v * c.x;
    }
    if (m1 & CM_FLUID) {
      double v = (double)(int)(m1 >> CM_DIAG_SHIFT) * c.y;
      v = v - ((m1 & CM_RIGHT) ? s[i + 128] : 0.0);
      if (m1 & CM_UP) {
        size_t up = i + 130;
        if (l == 63) { int band, tt, ll; skew_decode(g, i + 1, band, tt, ll); up = skew_index(g, tt - 63, 64 * (band + 1)); }
        v = v - s[up];
      } else {
        v = v - 0.0;
      }
      v = v - ((m1 & CM_LEFT) ? c.x : 0.0);
      if (m1 & CM_DOWN) {
        size_t dn = i - 2;
        if (l == 0) { int band, tt, ll; skew_decode(g, i + 1, band, tt, ll); dn = skew_index(g, tt, 64 * band - 1); }
        v = v - s[dn];
      } else {
        v = v - 0.0;
      }
      o.y = v;
      t += v * c.y;
    }
    // z of a non-fluid cell stays what it is (0): write the pair only where both are fluid, else element-wise
    if ((m0 & m1) & CM_FLUID) *reinterpret_cast<sw_d2*>(z + i) = o;
    else if (m0 & CM_FLUID) z[i] = o.x;
    else z[i + 1] = o.y;
  }
  t = block_sum(t);
  if (fin_op >= 0) block_finish<false>(t, partial, counter, sc, fin_op);   // fin_op < 0: dot(z,s) is replayed sequentially
}

// p += alpha s ; r -= alpha z (fmadd x2, main.c:753-754) ; per-block max |r| (inf_norm, main.c:654-667)
__global__ __launch_bounds__(RED_THREADS) void k_update_pr(double* __restrict__ p, double* __restrict__ r,
                                                           const double* __restrict__ s, const double* __restrict__ z,
                                                           const uint8_t* __restrict__ mask, size_t S,
                                                           double* __restrict__ partial, PcgScalars* sc, int force,
                                                           double alpha_arg, unsigned int* counter, int fin_op) {
  if (!force && pcg_idle(sc)) return;
  const double alpha = force ? alpha_arg : sc->alpha;
  const double nalpha = -alpha;
  const size_t chunk = (((S + gridDim.x - 1) / gridDim.x) + 1) & ~(size_t)1;   // whole 16-byte pairs per thread
  const size_t lo = (size_t)blockIdx.x * chunk, hi = lo + chunk < S ? lo + chunk : S;
  double mx = 0.0;
  for (size_t i = lo + 2 * (size_t)threadIdx.x; i < hi; i += 2 * RED_THREADS) {
    const unsigned int mm = *reinterpret_cast<const unsigned short*>(mask + i);
    const bool f0 = (mm & CM_FLUID) != 0, f1 = ((mm >> 8) & CM_FLUID) != 0;
    if (!(f0 | f1)) continue;
    const sw_d2 sv = *reinterpret_cast<const sw_d2*>(s + i), zv = *reinterpret_cast<const sw_d2*>(z + i);
    sw_d2 pv = *reinterpret_cast<const sw_d2*>(p + i), rv = *reinterpret_cast<const sw_d2*>(r + i);
    if (f0) { pv.x = pv.x + sv.x * alpha; rv.x = rv.x + zv.x * nalpha; const double a = fabs(rv.x); if (a > mx) mx = a; }
    if (f1) { pv.y = pv.y + sv.y * alpha; rv.y = rv.y + zv.y * nalpha; const double a = fabs(rv.y); if (a > mx) mx = a; }
    *reinterpret_cast<sw_d2*>(p + i) = pv;      // a non-fluid partner is written back unchanged
    *reinterpret_cast<sw_d2*>(r + i) = rv;
  }
  mx = block_max(mx);
  if (fin_op >= 0) block_finish<true>(mx, partial, counter, sc, fin_op);
}

// max |r| only (EULER_OP_INF_NORM_R)
__global__ __launch_bounds__(RED_THREADS) void k_inf_norm(const double* __restrict__ r, const uint8_t* __restrict__ mask,
                                                          size_t S, double* __restrict__ partial) {
  const size_t chunk = (S + gridDim.x - 1) / gridDim.x;
  const size_t lo = (size_t)blockIdx.x * chunk, hi = lo + chunk < S ? lo + chunk : S;
  double mx = 0.0;
  for (size_t i = lo + threadIdx.x; i < hi; i += RED_THREADS)
    if (mask[i] & CM_FLUID) { const double a = fabs(r[i]); if (a > mx) mx = a; }
  mx = block_max(mx);
  if (threadIdx.x == 0) partial[blockIdx.x] = mx;
}

// s = z + beta s (update_search, main.c:669-677); with COPY: s = z (the memcpy at main.c:746)
template <bool COPY>
__global__ __launch_bounds__(256) void k_update_search(double* __restrict__ s, const double* __restrict__ z,
                                                       const uint8_t* __restrict__ mask, size_t S, const PcgScalars* sc,
                                                       int force, double beta_arg) {
  if (!force && pcg_idle(sc)) return;
  const double beta = force ? beta_arg : sc->beta;
  for (size_t i = 2 * ((size_t)blockIdx.x * blockDim.x + threadIdx.x); i < S; i += 2 * (size_t)gridDim.x * blockDim.x) {
    const sw_d2 zv = *reinterpret_cast<const sw_d2*>(z + i);
    if (COPY) { *reinterpret_cast<sw_d2*>(s + i) = zv; continue; }
    const unsigned int mm = *reinterpret_cast<const unsigned short*>(mask + i);
    const bool f0 = (mm & CM_FLUID) != 0, f1 = ((mm >> 8) & CM_FLUID) != 0;
    if (!(f0 | f1)) continue;
    sw_d2 sv = *reinterpret_cast<const sw_d2*>(s + i);
    if (f0) sv.x = zv.x + beta * sv.x;
    if (f1) sv.y = zv.y + beta * sv.y;
    *reinterpret_cast<sw_d2*>(s + i) = sv;      // a non-fluid partner is written back unchanged
  }
}

// the slab's edge rows of a skewed array once more, write-through at system scope (see st_system): row y0 and / or y1
__global__ __launch_bounds__(256) void k_publish_edge_rows(double* arr, SkewGeom g, int y0, int y1, const PcgScalars* sc) {
  if (pcg_idle(sc)) return;
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= g.X) return;
  const int y = blockIdx.y == 0 ? y0 : y1;
  if (y < 0) return;
  double* p = arr + skew_index(g, x, y);
  st_system(p, *p);
}

// Jacobi stand-in preconditioner (not the reference's iterates; roofline comparison only)
__global__ __launch_bounds__(256) void k_jacobi(const double* __restrict__ r, double* __restrict__ z,
                                                const uint8_t* __restrict__ mask, size_t S, const PcgScalars* sc, int force) {
  if (!force && pcg_idle(sc)) return;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < S; i += (size_t)gridDim.x * blockDim.x) {
    const uint8_t m = mask[i];
    const int d = m >> CM_DIAG_SHIFT;
    z[i] = (m & CM_FLUID) ? r[i] / (double)(d ? d : 1) : 0.0;
  }
}

// the p += alpha s (fmadd, main.c:753) that are still due when a solve ends: with `iters` iterations counted and N at a time applied by the
// k_search_apply pass of every N-th iteration k >= N (the terms below k), those from the last such k (or from 0) to iters - 1, in their order
struct SRing { const double* s[8]; int n, steps; };      // the ring: s_j sits in s[j % n]
__global__ __launch_bounds__(256) void k_finish_p(double* __restrict__ p, const uint8_t* __restrict__ mask, size_t e_lo, size_t S,
                                                  const PcgScalars* sc, SRing ring) {
  if (!sc->nonzero || sc->iters == 0) return;
  const int n_it = sc->iters;
  const int from = n_it - 1 >= ring.steps ? (n_it - 1) / ring.steps * ring.steps : 0;
  const int cnt = n_it - from;      // 1 .. steps
  double al[8];
  const double* sp[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { const int it = from + (j < cnt ? j : 0); al[j] = sc->alpha_hist[it & 7]; sp[j] = ring.s[it % ring.n] + e_lo; }
  for (size_t i = 2 * ((size_t)blockIdx.x * blockDim.x + threadIdx.x); i < S; i += 2 * (size_t)gridDim.x * blockDim.x) {
    const unsigned int mm = *reinterpret_cast<const unsigned short*>(mask + i);
    const bool f0 = (mm & CM_FLUID) != 0, f1 = ((mm >> 8) & CM_FLUID) != 0;
    if (!(f0 | f1)) continue;
    sw_d2 pv = *reinterpret_cast<const sw_d2*>(p + i);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j < cnt) {      // (uniform)
        const sw_d2 sv = *reinterpret_cast<const sw_d2*>(sp[j] + i);
        if (f0) pv.x = pv.x + sv.x * al[j];
        if (f1) pv.y = pv.y + sv.y * al[j];
      }
    }
    *reinterpret_cast<sw_d2*>(p + i) = pv;
  }
}

// (of the last multi-kernel solve: its ring and scalars stand until the next solve starts)
int eu_launch_finish_p(euler_sim* S) {
  if (S->s_ring_n <= 0) return EULER_OK;
  SRing ring;
  for (int k = 0; k < 8; ++k) ring.s[k] = S->s_ring[k < S->s_ring_n ? k : 0];
  ring.n = S->s_ring_n; ring.steps = S->s_ring_n;
  LAUNCH(S, KC_UPDATE_PR, k_finish_p, dim3(eu_blocks(S->e_cnt, 256 * 4, 4096)), dim3(256), S->p + S->e_lo, S->cellmask + S->e_lo, S->e_lo, S->e_cnt, S->sc, ring);
  return EULER_OK;
}

// ---- multi-rank helpers ---------------------------------------------------------------------
__global__ void k_scalar_epilogue(PcgScalars* sc, int op, int force) {   // after the all-reduce of comm_val
  if (!force && pcg_idle(sc)) return;
  pcg_scalar_step(sc, op, sc->comm_val);
}
__global__ void k_nonzero_to_comm(PcgScalars* sc) { sc->comm_val = sc->nonzero ? 1.0 : 0.0; }
__global__ void k_nonzero_from_comm(PcgScalars* sc) { sc->nonzero = sc->comm_val != 0.0; }

// one grid row (band, lane) of a skewed array <-> a contiguous buffer of X doubles
__global__ __launch_bounds__(256) void k_pack_row(const double* __restrict__ skew, double* __restrict__ row, SkewGeom g, int band, int lane) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x < g.X) row[x] = skew[skew_index(g, x, band * 64 + lane)];
}
__global__ __launch_bounds__(256) void k_unpack_row(double* __restrict__ skew, const double* __restrict__ row, SkewGeom g, int band, int lane) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x < g.X) skew[skew_index(g, x, band * 64 + lane)] = row[x];
}

// the edge rows of two skewed vectors <-> the neighbour buffers, one launch: blockIdx.y = 2 * side + vector.
// PACK: lowest own row (band_lo, lane 0) -> lo buffer, highest (band_hi - 1, lane 63) -> hi buffer; else the rows that arrived
// land in the adjacent bands' storage, (band_lo - 1, lane 63) and (band_hi, lane 0).
template <bool PACK>
__global__ __launch_bounds__(256) void k_halo_rows2(double* a, double* b, double* lo, double* hi, SkewGeom g, int band_lo, int band_hi,
                                                    int has_lo, int has_hi) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= g.X) return;
  const int side = blockIdx.y >> 1, vec = blockIdx.y & 1;
  if (side == 0 ? !has_lo : !has_hi) return;
  double* arr = vec ? b : a;
  double* buf = (side ? hi : lo) + (size_t)vec * g.X;
  const int y = PACK ? (side ? 64 * band_hi - 1 : 64 * band_lo) : (side ? 64 * band_hi : 64 * band_lo - 1);
  double* e = arr + skew_index(g, x, y);
  if (PACK) buf[x] = *e; else *e = buf[x];
}

// ---- "ghost rows": the default with several ranks in tile-local mode (no mailboxes) ------------------------------------------
// A PCG iteration has TWO exchange points, each ONE call of euler_comm_ops.exchange (RCCL: one group of sends / receives):
//   G1  behind k_precond_tile:  the slab's edge rows of z to the two neighbours + {max |r|, dot(z,r)} of every rank to every rank
//   G2  behind k_search_apply:  the partial of dot(s, A s) of every rank to every rank
// and every rank folds what arrived in rank order (identical bits everywhere: alpha, beta and `done` stay in step without a
// broadcast).  Against round 2 (halo(z, s) - all-reduce(alpha) - all-gather{max |r|, dot}: three exchanges, two pack / unpack
// launches): the edge rows leave k_precond_tile as compact rows and are read by k_search_apply as compact rows (no pack, no
// unpack), and s does not travel at all - a rank keeps its ghost rows of s current by itself (k_search_apply SLAB 2).
int eu_comm_exchange(euler_sim* S, double* send_lo, double* send_hi, double* recv_lo, double* recv_hi, int count, double* small, int nsmall) {
  if (S->bulk.exchange) {
    COMM_CALL(S->bulk.exchange(S->bulk.ctx, send_lo, send_hi, recv_lo, recv_hi, count, small, nsmall));
    return EULER_OK;
  }
  // a communicator without the fused operation: the same traffic as a neighbour exchange and an all-gather
  if (count > 0) COMM_CALL(S->bulk.halo(S->bulk.ctx, send_lo, send_hi, recv_lo, recv_hi, count));
  if (nsmall > 0) {
    int64_t off[64], cnt[64];
    for (int r = 0; r < S->bulk.nranks && r < 64; ++r) { off[r] = (int64_t)8 * nsmall * r; cnt[r] = (int64_t)8 * nsmall; }
    COMM_CALL(S->bulk.allgather(S->bulk.ctx, small, off, cnt));
  }
  return EULER_OK;
}
__global__ void k_alpha_fold(PcgScalars* sc, const double* __restrict__ vals, int R, int force) {   // G2: dot(s, A s) = sum over ranks, in rank order
  if (!force && pcg_idle(sc)) return;
  double v = 0.0;
  for (int r = 0; r < R; ++r) v += vals[r];
  pcg_scalar_step(sc, FIN_ALPHA, v);
}

// rank-local reduction result (left in comm_val by FIN_TO_COMM) -> all-reduce -> scalar epilogue
int eu_comm_finish(euler_sim* S, int fin_op, int is_max, int force) {
  if (S->p2p_on) return EULER_OK;   // the reduction's last block already exchanged the partials and applied the epilogue
  if (fin_op == FIN_ALPHA && ghost_mode(S)) {      // G2
    if (int rc = eu_comm_exchange(S, nullptr, nullptr, nullptr, nullptr, 0, S->alpha_buf, 1)) return rc;
    hipLaunchKernelGGL(k_alpha_fold, dim3(1), dim3(1), 0, S->stream, S->sc, S->alpha_buf, S->comm.nranks, force);
    return EULER_OK;
  }
  COMM_CALL(S->comm.allreduce(S->comm.ctx, &S->sc->comm_val, 1, is_max));
  hipLaunchKernelGGL(k_scalar_epilogue, dim3(1), dim3(1), 0, S->stream, S->sc, fin_op, force);
  return EULER_OK;
}

// ghost rows of the search vector s for apply_a: my lowest row goes to rank-1, my highest to rank+1
static int comm_halo_s(euler_sim* S) {
  if (S->p2p_on) return eu_p2p_halo_skewed(S, S->s);   // one launch: rows leave from and land in the skewed array
  const int X = S->X, nbk = (X + 255) / 256;
  double *send_lo = S->halo_buf, *send_hi = S->halo_buf + X, *recv_lo = S->halo_buf + 2 * X, *recv_hi = S->halo_buf + 3 * X;
  const bool has_lo = S->band_lo > 0, has_hi = S->band_hi < S->geom.nbands;
  if (has_lo) hipLaunchKernelGGL(k_pack_row, dim3(nbk), dim3(256), 0, S->stream, S->s, send_lo, S->geom, S->band_lo, 0);
  if (has_hi) hipLaunchKernelGGL(k_pack_row, dim3(nbk), dim3(256), 0, S->stream, S->s, send_hi, S->geom, S->band_hi - 1, 63);
  COMM_CALL(S->comm.halo(S->comm.ctx, send_lo, send_hi, recv_lo, recv_hi, X));
  if (has_lo) hipLaunchKernelGGL(k_unpack_row, dim3(nbk), dim3(256), 0, S->stream, S->s, recv_lo, S->geom, S->band_lo - 1, 63);
  if (has_hi) hipLaunchKernelGGL(k_unpack_row, dim3(nbk), dim3(256), 0, S->stream, S->s, recv_hi, S->geom, S->band_hi, 0);
  return EULER_OK;
}

static inline int loc_red_blocks(const euler_sim* S) { return (int)eu_blocks(S->e_cnt, EU_RED_ELEMS, 2048); }

int eu_launch_dot(euler_sim* S, const double* a, const double* b, int fin_op, int force) {
  if (S->cfg.dot_mode == EULER_DOT_SEQUENTIAL && !S->has_comm) {
    LAUNCH(S, KC_DOT, k_dot_sequential, dim3(1), dim3(256), a, b, S->cellmask, S->geom, S->sc, fin_op, force);
    return EULER_OK;
  }
  const int edges = (a == S->z && S->has_comm && eu_p2p_has_neighbour_arrays(S)) ? ((S->band_lo > 0 ? 1 : 0) | (S->band_hi < S->geom.nbands ? 2 : 0)) : 0;
  LAUNCH(S, KC_DOT, edges ? k_dot_partial<true> : k_dot_partial<false>, dim3(loc_red_blocks(S)), dim3(RED_THREADS), LOC(a), LOC(b), LOC(S->cellmask), S->e_cnt,
         S->partial, S->sc, force, S->red_counter, fin_or_comm(S, fin_op), edges ? S->geom.TS : 0, edges ? S->band_hi - S->band_lo : 0, edges);
  return S->has_comm ? eu_comm_finish(S, fin_op, 0, force) : EULER_OK;
}

// A s' never goes to memory: k_search_apply leaves it out and the r update (k_precond_tile<16, true>) forms it again from s' (the same bits).
// Not where somebody else reads the array - the sequential replay of dot(s, A s) - nor where the rows across a slab boundary are not at hand:
// the mailbox configurations (comm_p2p.hip) and the reference's IC(0) on several ranks.  EULER_OPT_TILE_STORE_AS restores the stored form.
bool tile_recompute(const euler_sim* S) {
  if (S->opt[EULER_OPT_TILE_STORE_AS] || sa_run(S) != 8) return false;
  if (!tile_fused(S)) return !S->has_comm && S->cfg.dot_mode != EULER_DOT_SEQUENTIAL;      // (the r update of the other modes is this kernel's first half)
  if (S->tile_w != 16) return false;
  if (S->has_comm) return ghost_mode(S);
  return S->cfg.dot_mode != EULER_DOT_SEQUENTIAL;
}
// the halo buffers (ZrArgs), allocated by the first solve that runs the form; false: no room - the solve keeps the stored form (the same bits)
static bool tile_z_begin(euler_sim* S) {
  S->z_halo_last = 0;
  if (!tile_z_recompute(S)) return false;
  if (!S->zhalo) {
    const size_t nh = (size_t)S->geom.nbands * (S->geom.T / 16) * 128, nr = (size_t)S->geom.nbands * 2 * S->X;
    if (eu_dalloc(S, &S->zhalo, nh, EU_MEM_HANDLE, EU_DEV_QUIET)) return false;
    if (eu_dalloc(S, &S->zrows, nr, EU_MEM_HANDLE, EU_DEV_QUIET)) { (void)eu_dev_free(S, S->zhalo); S->zhalo = nullptr; return false; }
    HIPCHK(hipMemsetAsync(S->zhalo, 0, nh * sizeof(double), S->stream));
    HIPCHK(hipMemsetAsync(S->zrows, 0, nr * sizeof(double), S->stream));
  }
  return true;
}

// ghost rows of TWO skewed vectors in one exchange (z and s before the fused search + apply_a pass: the neighbouring
// slabs' edge rows land in the adjacent bands' storage, where k_search_apply's lanes 0 / 63 look for them)
int eu_comm_halo_two(euler_sim* S, double* a, double* b) {
  if (S->p2p_on) { int rc = eu_p2p_halo_skewed(S, a); return rc ? rc : eu_p2p_halo_skewed(S, b); }
  const int X = S->X, nbk = (X + 255) / 256;
  double *send_lo = S->halo_buf, *send_hi = S->halo_buf + 2 * X, *recv_lo = S->halo_buf + 4 * X, *recv_hi = S->halo_buf + 6 * X;
  const int has_lo = S->band_lo > 0, has_hi = S->band_hi < S->geom.nbands;
  // one launch packs the four rows (2 vectors x lowest / highest own row), one unpacks the four that arrived
  hipLaunchKernelGGL(k_halo_rows2<true>, dim3(nbk, 4), dim3(256), 0, S->stream, a, b, send_lo, send_hi, S->geom, S->band_lo, S->band_hi, has_lo, has_hi);
  COMM_CALL(S->comm.halo(S->comm.ctx, send_lo, send_hi, recv_lo, recv_hi, 2 * X));
  hipLaunchKernelGGL(k_halo_rows2<false>, dim3(nbk, 4), dim3(256), 0, S->stream, a, b, recv_lo, recv_hi, S->geom, S->band_lo, S->band_hi, has_lo, has_hi);
  return EULER_OK;
}

// dot(z, r) rides in the forward sweep as dot(q, q) (SweepArgs::fin_qq): one rank, tree-dot mode, the band schedule
static inline bool dot_rides_in_sweep(const euler_sim* S) { return S->cfg.precond == EULER_PRECOND_IC0 && S->cfg.sweep_mode != EULER_SWEEP_SIMPLE && !S->has_comm && S->cfg.dot_mode != EULER_DOT_SEQUENTIAL; }
static int launch_precondition(euler_sim* S, int force, int fin_dot = -1) {   // z = M^-1 r [and the scalar epilogue of dot(z, r)]
  if (S->cfg.precond == EULER_PRECOND_JACOBI) {
    LAUNCH(S, KC_JACOBI, k_jacobi, dim3(eu_blocks(S->e_cnt, 256 * 4, 4096)), dim3(256), LOC(S->r), LOC(S->z), LOC(S->cellmask),
           S->e_cnt, S->sc, force);
    return fin_dot >= 0 ? eu_launch_dot(S, S->z, S->r, fin_dot, force) : EULER_OK;
  }
  const bool ride = fin_dot >= 0 && dot_rides_in_sweep(S);
  int rc = eu_launch_sweep(S, SW_FORWARD, KC_FORWARD_SOLVE, force, ride ? fin_dot : -1);
  if (rc) return rc;
  if ((rc = eu_launch_sweep(S, SW_BACKWARD, KC_BACKWARD_SOLVE, force))) return rc;
  return fin_dot >= 0 && !ride ? eu_launch_dot(S, S->z, S->r, fin_dot, force) : EULER_OK;
}

static int launch_apply_a_and_alpha(euler_sim* S, int force) {
  const bool seq = S->cfg.dot_mode == EULER_DOT_SEQUENTIAL && !S->has_comm;
  if (S->has_comm && ghost_mode(S) && !force) {
    // the first search direction is z_0, whose edge rows arrived with the exchange behind the solve's first k_precond_tile: they
    // become the ghost rows of s - in the adjacent bands' storage for this one pass (k_apply_a looks there), and generation 0 of
    // the compact rows k_search_apply keeps current from here on
    const int X = S->X, nbk = (X + 255) / 256;
    const bool coarse = eu_is_two_level(S);      // (the first search direction is z_0 + P y then: the ghost rows take the P y of their own cells)
    if (S->band_lo > 0) {
      HIPCHK(hipMemcpyAsync(xrow(S, XR_GS_LO0), xrow(S, XR_ZRECV_LO), (size_t)X * 8, hipMemcpyDeviceToDevice, S->stream));
      if (coarse) { int rc = eu_launch_coarse_add_row(S, xrow(S, XR_GS_LO0), 64 * S->band_lo - 1); if (rc) return rc; }
      hipLaunchKernelGGL(k_unpack_row, dim3(nbk), dim3(256), 0, S->stream, S->s, xrow(S, XR_GS_LO0), S->geom, S->band_lo - 1, 63);
    }
    if (S->band_hi < S->geom.nbands) {
      HIPCHK(hipMemcpyAsync(xrow(S, XR_GS_HI0), xrow(S, XR_ZRECV_HI), (size_t)X * 8, hipMemcpyDeviceToDevice, S->stream));
      if (coarse) { int rc = eu_launch_coarse_add_row(S, xrow(S, XR_GS_HI0), 64 * S->band_hi); if (rc) return rc; }
      hipLaunchKernelGGL(k_unpack_row, dim3(nbk), dim3(256), 0, S->stream, S->s, xrow(S, XR_GS_HI0), S->geom, S->band_hi, 0);
    }
    S->gs_cur = 0;
  } else if (S->has_comm) { int rc = comm_halo_s(S); if (rc) return rc; }
  SkewGeom gl = S->geom;
  gl.S = S->e_cnt;
  double* out = tile_fused(S) ? S->q : S->z;     // tile-local mode: A s always lands in q (k_precond_tile reads it there and writes z)
  LAUNCH(S, KC_APPLY_A, k_apply_a, dim3(loc_red_blocks(S)), dim3(RED_THREADS), LOC(S->s), LOC(out), LOC(S->cellmask), gl,
         S->partial, S->sc, force, S->red_counter, seq ? -1 : fin_or_comm(S, FIN_ALPHA));
  if (seq)
    LAUNCH(S, KC_DOT, k_dot_sequential, dim3(1), dim3(256), out, S->s, S->cellmask, S->geom, S->sc, (int)FIN_ALPHA, force);
  return S->has_comm ? eu_comm_finish(S, FIN_ALPHA, 0, force) : EULER_OK;
}

// p += alpha s, N iterations at a time (k_search_apply PMODE N): 8 - the search directions turn through a ring of eight arrays, six of them allocated when the
// first solve needs them (8192^2: 431 -> 421 us per iteration against 4, 473 -> 450 for 4 against 2); 2 (rounds 3-4: s and s2 alone) with the mailboxes, whose
// peers map exactly those two, and with the experimental run lengths.  EULER_OPT_P_STEPS 2 / 4 select the shorter rings (the same bits: the fmadds of main.c:753
// are applied in their order either way).
int p_steps(const euler_sim* S) {
  if (S->p2p_on || sa_run(S) != 8) return 2;
  return (int)S->opt[EULER_OPT_P_STEPS];
}
// the ring of this solve: [0], [1] = s, s2 as the solve finds them, then the extra arrays (zeroed once; like s and s2 they are only ever written on fluid cells)
static int ring_begin(euler_sim* S) {
  const int n = p_steps(S);
  if (!S->s_base[0]) { S->s_base[0] = S->s; S->s_base[1] = S->s2; }      // the two arrays of the handle (whichever way round the solves so far left them)
  if (n > 2) { S->s = S->s_base[0]; S->s2 = S->s_base[1]; }             // (the last solve may have ended on one of the extra arrays)
  else if (S->s != S->s_base[0] && S->s != S->s_base[1]) { S->s = S->s_base[0]; S->s2 = S->s_base[1]; }
  else if (S->s2 != S->s_base[0] && S->s2 != S->s_base[1]) S->s2 = S->s == S->s_base[0] ? S->s_base[1] : S->s_base[0];
  S->s_ring[0] = S->s; S->s_ring[1] = S->s2;
  for (int k = 2; k < n; ++k) {
    if (!S->s_ring_alloc[k]) {
      const size_t elems = S->Sw + EU_SKEW_SLACK;
      if (eu_dev_alloc(S, &S->s_ring_alloc[k], elems * sizeof(double), EU_MEM_RING, EU_DEV_QUIET)) {
        // no room for the ring (13 GB at 16384^2 on one GPU): the solve goes on with the handle's own two arrays - the same bits (tests/test_gpu_tile_precond.py: the
        // forms test), p is updated every second iteration instead of every eighth - rather than fail a substep whose marker stage has already run
        eu_dev_free_group(S, EU_MEM_RING);
        for (void*& d : S->s_ring_alloc) d = nullptr;
        S->opt[EULER_OPT_P_STEPS] = 2;
        return ring_begin(S);
      }
      HIPCHK(hipMemsetAsync(S->s_ring_alloc[k], 0, elems * sizeof(double), S->stream));
    }
    S->s_ring[k] = static_cast<double*>(S->s_ring_alloc[k]) + EU_SKEW_SLACK - S->skew_off;
  }
  S->s_ring_n = n;
  S->s_launched = 0;
  return EULER_OK;
}
// EULER_F_PCG_S: the search direction of the last iteration that RAN (launches behind convergence return at once but still turn the ring)
double* eu_current_search_direction(euler_sim* S) {
  if (S->s_ring_n < 2 || S->s_launched <= 0) return S->s;
  (void)hipStreamSynchronize(S->stream);      // sc_host: copied at the end of the solve
  const int ran = S->sc_host->nonzero ? S->sc_host->iters : 0;
  if (ran <= 0 || ran > S->s_launched) return S->s;
  return S->s_ring[(ran - 1) % S->s_ring_n];
}

__global__ void k_pcg_reset(PcgScalars* sc, double tol, int max_iters) {
  sc->sigma = sc->zs = sc->sigma_new = sc->alpha = sc->alpha_prev = sc->beta = sc->rnorm = 0.0;
  sc->tol = tol; sc->nonzero = 0; sc->done = 0; sc->iters = 0; sc->max_iters = max_iters; sc->zfix = 0;
}

// multilevel mode on one GPU: the first search direction s = z + P y is formed by the first k_search_apply itself (project_first_direction)
static inline bool first_direction_folded(const euler_sim* S) { return tile_fused(S) && eu_is_mg(S) && !S->has_comm && S->cfg.dot_mode != EULER_DOT_SEQUENTIAL && sa_run(S) == 8; }
// what the phases of one solve hand on (eu_launch_project) and cannot form again from the handle
struct Solve {
  PcgScalars prev;                  // the previous solve's final scalars
  int pred_iters;                   // the iterations this solve is expected to take (0: no prediction)
  bool drain_poll;                  // blocking convergence polls (mailboxes)
  bool zr, zr_ran;                  // z formed twice (tile_z_begin); a pass of this solve left z's halo only
  bool solved;                      // the resident attempt ended the solve
};

// 1. bookkeeping and chunk prediction, then the assembly of this system
static int project_begin(euler_sim* S, float dt, Solve& v) {
  S->s_launched = 0;      // (EULER_F_PCG_S: no multi-kernel iteration of this solve has run yet)
  S->z_halo_last = 0;
  S->pcg_fields_resident = 0;
  v.prev = *S->sc_host;      // (the previous solve's final scalars: a resident launch that has to be redone must not leave its own in their place)
  // the previous solve's final scalars are in sc_host by now (copied at its end, synced since)
  S->solve_iters[S->solve_seq & 255] = S->sc_host->nonzero ? S->sc_host->iters : -1;
  if (S->solve_seq > 0) { S->res_last_chunks = S->sc_host->n_chunks; S->res_have_last = 1; }      // (the resident solver's guess for this solve, below)
  S->solve_seq += 1;
  // Convergence polls never drain the queue (round 6): the host enqueues a chunk of iterations, a 48-byte copy of the scalars and an event, and then waits for the
  // copy behind the PREVIOUS chunk - the GPU always has the next chunk queued behind the one whose outcome the host is waiting for.  What is queued behind
  // convergence returns at once (every per-iteration kernel reads sc->done first), so a late poll costs launches, not work.  The chunk length follows a
  // prediction: a solve that converged in k iterations is followed by one that needs about k (scenes change slowly) - chunks of pcg_poll_interval up to k - 2,
  // chunks of 2 from there on (rounds 1-5: a blocking poll every pcg_poll_interval iterations for converging solves: ~27 us of idle GPU each, and up to
  // pcg_poll_interval - 1 launches behind convergence that, in the multilevel mode's cycle, did their whole work).
  // (several ranks: nonzero / done / iters are the same on every rank, so all ranks cut the same chunks and stop behind the same one)
  v.pred_iters = (S->sc_host->nonzero && S->sc_host->done && S->sc_host->iters < S->cfg.max_iterations) ? S->sc_host->iters : 0;
  // With the peer-to-peer mailboxes a rank's kernels WAIT inside the kernel for their peers' (comm_p2p.hip).  Ranks that share one GPU (the tests) then need the queue to run
  // dry now and then - a process whose kernels spin while the other's are queued behind them makes a 2 s test take 200 - so converging solves keep rounds 1-5's blocking
  // poll there (solves that ran into the cap polled one chunk late before, and still do).
  v.drain_poll = S->p2p_on && !(S->sc_host->nonzero && !S->sc_host->done && S->sc_host->iters >= S->cfg.max_iterations);
  S->prof_iter = -1;
  LAUNCH(S, KC_MISC, k_pcg_reset, dim3(1), dim3(1), S->sc, S->cfg.tol, S->cfg.max_iterations);
  eu_launch_build_system(S, dt);
  if (S->has_comm) {   // all_zero(r) over the whole grid
    hipLaunchKernelGGL(k_nonzero_to_comm, dim3(1), dim3(1), 0, S->stream, S->sc);
    COMM_CALL(S->comm.allreduce(S->comm.ctx, &S->sc->comm_val, 1, 1));
    hipLaunchKernelGGL(k_nonzero_from_comm, dim3(1), dim3(1), 0, S->stream, S->sc);
  }
  return EULER_OK;
}

// 2. the resident attempt and its redo; v.solved: the solve ended here
static int project_resident(euler_sim* S, float dt, Solve& v) {
  // Small grids (every chunk finds a wave on the chip at once): the whole solve as ONE persistent launch (k_resident.hip).  Two host round trips per solve -
  // the number of active chunks before the launch, its error word behind it - instead of one per eight iterations.
  const bool res_skip = S->res_skip_once != 0;
  S->res_skip_once = 0;
  if (!res_skip && eu_resident_eligible(S)) {
    // Whether this solve's active chunks fit is decided from the PREVIOUS solve's count (scenes change slowly; sc_host holds it: copied at the end of every solve) - no host
    // round trip in front of the launch: the kernel is launched over the device's whole capacity, the workgroups beyond (n_chunks + 3) / 4 leave at once, and a solve that
    // does not fit after all says so itself (error word 2) and is redone below.  The first solve of a handle asks the device.
    const unsigned int cap_chunks = 4u * (unsigned int)eu_resident_capacity(S, S->cfg.pcg_precision == EULER_PCG_F32);
    unsigned int guess = S->res_last_chunks;
    if (!S->res_have_last) {
      HIPCHK(hipMemcpyAsync(S->sc_host, S->sc, sizeof(PcgScalars), hipMemcpyDeviceToHost, S->stream));
      HIPCHK(hipStreamSynchronize(S->stream));
      guess = S->sc_host->n_chunks;
    }
    if (guess + guess / 16 + 8 <= cap_chunks || S->cfg.pcg_precision == EULER_PCG_F32) {
      v.solved = true;      // (every way out of this block ends the solve: its result, an error, or the redo's)
      S->prof_iter = -2;
      if (int rc = eu_launch_resident(S, cap_chunks)) return rc;      // (a no-op on the device when the right-hand side is all zero: main.c:742, p = 0 from the assembly)
      HIPCHK(hipMemcpyAsync(S->sc_host, S->sc, sizeof(PcgScalars), hipMemcpyDeviceToHost, S->stream));
      HIPCHK(hipStreamSynchronize(S->stream));
      S->res_last_chunks = S->sc_host->n_chunks; S->res_have_last = 1;
      const int err = *S->res_err;
      if (err == 0) {
        if (S->sc_host->nonzero) { S->res_solves += 1; S->pcg_fields_resident = 1; }      // (z, s, q never left the registers: EULER_F_PCG_Z / _S / _Q have nothing to show)
        return eu_launch_velocity_update(S, dt, 0);      // (the resident kernel wrote the final p; sc_host is current)
      }
      *S->res_err = 0;
      if (S->cfg.pcg_precision == EULER_PCG_F32 && err == 2) { eu_set_error("EULER_PCG_F32: the solve's active chunks do not fit the resident solver"); return EULER_EHIP; }
      // (a time-out on an EULER_PCG_F32 handle: this system and every later one are solved in DOUBLE by the multi-kernel path - the substep's markers have moved already,
      // so failing here would leave the handle between two stages; euler_resident_info reports the fallback)
      if (err != 2) { S->res_fallbacks += 1; S->res_disabled = 1; }      // a wait ran out (the workgroups were not all resident - another process on the device?): the handle keeps to the multi-kernel path from here on
      // (error 2: more active chunks than fit - the scene grew; this system with the multi-kernel path: k_pcg_reset + the assembly again, written whole)
      S->solve_seq -= 1;
      eu_vd_solver_arrays_foreign(&S->vd);
      S->res_skip_once = 1;
      *S->sc_host = v.prev;      // (solve_iters[] and the look-ahead of the redo are the previous SOLVE's, not the aborted launch's)
      return eu_launch_project(S, dt);
    }
    // (too many active chunks last time: the multi-kernel path below; its final copy of the scalars keeps the count current)
  }
  return EULER_OK;
}

// 3. first z and first search direction
static int project_first_direction(euler_sim* S, Solve& v) {
  int rc;
  // if (!all_zero(r)) { ... }: every kernel below is a no-op when sc->nonzero == 0
  const bool tile = tile_fused(S), two_level = tile && eu_is_two_level(S);
  if (two_level && S->has_comm && !(eu_is_mg(S) && ghost_mode(S) && S->slab_on)) {
    eu_set_error("coarse-correction preconditioners with several ranks: EULER_PRECOND_IC0_TILE_MG on row slabs without mailboxes only");
    return EULER_EINVAL;
  }
  if (two_level && (rc = eu_launch_coarse_setup(S))) return rc;   // P^T A P of this system, its factor and inverse (k_coarse.hip)
  if (two_level && (rc = eu_launch_coarse_consistent(S))) return rc;   // (water cut off from the air: r = b made compatible with the singular A)
  v.zr = tile && tile_z_begin(S);      // (the first pass stores z whole: the copy s_0 = z and k_apply_a read it)
  if (tile) {                                                     // E^-1 per tile, then z = M^-1 r and sigma = dot(z, r) in one pass
    if ((rc = eu_launch_factor_tile(S, 0))) return rc;
    if ((rc = eu_launch_precond_tile(S, 0, 1, FIN_SIGMA_INIT, 0, 0.0))) return rc;
  } else {
  if (S->cfg.precond != EULER_PRECOND_JACOBI && (rc = eu_launch_sweep(S, SW_FACTOR, KC_PRECON_FACTOR, 0))) return rc;   // once per solve
  if ((rc = launch_precondition(S, 0, FIN_SIGMA_INIT))) return rc;
  }
  if ((rc = ring_begin(S))) return rc;      // (S->s = ring[0] takes the first search direction)
  // multilevel mode on one GPU: the first search direction s = z + P y is formed by the first k_search_apply itself (beta is 0 behind k_pcg_reset, and 0 times what an earlier
  // solve left in the ring is 0) - a copy pass and a k_apply_a less per solve.  Only there: no recorded digest pins this mode's zeros' signs (z = -0 comes out as +0)
  if (first_direction_folded(S)) {
    // (below) - beta = 0 times what an earlier solve left in ring[n - 1].  That product is only 0 while the array is finite: a solve that broke down (tol = 0 runs where
    // z . s reaches 0: alpha = 0 / 0) leaves Inf / NaN there, and 0 x Inf = NaN would poison every later solve - such a solve's ring is cleared first
    const PcgScalars& ps = v.prev;
    if (ps.nonzero && !(std::isfinite(ps.alpha) && std::isfinite(ps.beta) && std::isfinite(ps.rnorm) && std::isfinite(ps.sigma) && std::isfinite(ps.zs)))
      for (int k = 0; k < S->s_ring_n; ++k) HIPCHK(hipMemsetAsync(S->s_ring[k] + S->skew_off, 0, S->Sw * sizeof(double), S->stream));
  }
  else if (two_level) { if ((rc = eu_launch_coarse_search_init(S))) return rc; }      // s = z + P y
  else
  LAUNCH(S, KC_UPDATE_SEARCH, k_update_search<true>, dim3(eu_blocks(S->e_cnt, 256 * 4, 4096)), dim3(256), LOC(S->s), LOC(S->z),
         LOC(S->cellmask), S->e_cnt, S->sc, 0, 0.0);
  if (S->has_comm && eu_p2p_has_neighbour_arrays(S)) {   // the neighbours read these rows of s in the second iteration's k_search_apply
    const int y0 = S->band_lo > 0 ? 64 * S->band_lo : -1, y1 = S->band_hi < S->geom.nbands ? 64 * S->band_hi - 1 : -1;
    LAUNCH(S, KC_UPDATE_SEARCH, k_publish_edge_rows, dim3((S->X + 255) / 256, 2), dim3(256), S->s, S->geom, y0, y1, S->sc);
  }
  // ranks with their neighbours' z and s mapped run the fused kernel too (it reads across the slab boundary directly)
  // update_search of iteration k rides along with apply_a of iteration k + 1 in every configuration (several ranks: the ghost
  // rows of z and s are exchanged in front of it)
  // s' of non-fluid cells is never written: with two arrays the second one is cleared per solve as ever; a ring of four keeps what earlier solves left
  // off the fluid - nothing reads those elements unmasked, EULER_F_PCG_S shows them as +0 (s_stale) - rather than clear three arrays per solve
  // (s_stale with two arrays as well: the copy s = z above carries what z holds in tiles that are no longer active)
  if (S->s_ring_n == 2) HIPCHK(hipMemsetAsync(LOC(S->s2), 0, S->e_cnt * sizeof(double), S->stream));
  S->s_stale = 1;
  return EULER_OK;
}

// 4. the chunked iteration loop with its two polling schemes
static int project_iterate(euler_sim* S, Solve& v) {
  int rc;
  HIPCHK(hipMemcpyAsync(S->sc_host, S->sc, sizeof(PcgScalars), hipMemcpyDeviceToHost, S->stream));
  HIPCHK(hipStreamSynchronize(S->stream));
  const int poll = S->cfg.pcg_poll_interval > 0 ? S->cfg.pcg_poll_interval : 8;
  const int max_it = S->cfg.max_iterations;
  const bool tile = tile_fused(S), fold0 = first_direction_folded(S);
  int it = 0, chunk = 0;
  bool stop = !S->sc_host->nonzero;   // all_zero(r): main.c:742
  S->s_none = stop ? 1 : 0;           // (no search direction exists: EULER_F_PCG_S reads as +0)
  while (it < max_it && !stop) {
    int chunk_end = it + poll;
    if (!v.drain_poll && v.pred_iters > 0 && it < v.pred_iters + poll && chunk_end > v.pred_iters - 2) {      // around the predicted end: short chunks (the first of them ends at pred - 2)
      const int lo = v.pred_iters - 2 < chunk_end ? v.pred_iters - 2 : chunk_end;
      chunk_end = lo > it + 2 ? lo : it + 2;
    }
    if (chunk_end > max_it) chunk_end = max_it;
    for (; it < chunk_end; ++it) {
      S->prof_iter = it;
      const bool fused = it > 0 || fold0;   // update_search of iteration it-1 rides along with this apply_a (A s' lands in q)
      if (it == 0 && fold0) { S->s = S->s_ring[S->s_ring_n - 1]; S->s2 = S->s_ring[0]; }      // (the pass writes ring[0], the first direction's place; what it reads of s counts 0 times)
      if ((rc = fused ? eu_launch_search_apply(S, it) : launch_apply_a_and_alpha(S, 0))) return rc;
      if (tile) {
        // r -= alpha A s, max |r| (sets `done`), z = M^-1 r, beta = dot(z, r) / sigma: one pass; on the last iteration of the
        // budget only r and its norm (main.c:760-765 would be computed and never consumed)
        S->prof_iter = it;
        // tile_z_recompute: z's halo only where the next k_search_apply forms z again - a PMODE 1 pass (the ring's flush, PMODE N, keeps the stored form: with the
        // tile solve on top of its N - 1 extra streams it would hold 204 registers, two waves per SIMD) that is not the last (iteration max_it - 2 stores z whole)
        const int nx = it + 1, steps = S->s_ring_n;
        const bool next_odd = !(nx >= steps && nx % steps == 0);
        const int zform = v.zr && it + 1 < max_it ? (it + 2 < max_it && next_odd ? 1 : 0) : -1;
        if ((rc = eu_launch_precond_tile(S, 1, it + 1 < max_it, FIN_BETA, 0, 0.0, false, zform))) return rc;
        S->z_halo_last = zform == 1;
        v.zr_ran = v.zr_ran || zform == 1;
        continue;
      }
      // r -= alpha A s, max |r| (sets `done`): the first half of the tile pass, over the solve's active chunks (A s sits in q, or in z
      // behind the first apply_a); p += alpha s rides in k_search_apply / k_finish_p
      S->tile_as_override = fused ? S->q : S->z;
      rc = eu_launch_precond_tile(S, 1, 0, -1, 0, 0.0, true);
      S->tile_as_override = nullptr;
      if (rc) return rc;
      if (it + 1 < max_it) {   // the tail of the last iteration (main.c:760-765) is never consumed
        // these belong to iteration `it` but only run if it did not converge: tag them it+1 so that
        // they count as active only when the device went on to iteration it+1
        S->prof_iter = it + 1;
        if ((rc = launch_precondition(S, 0, FIN_BETA))) return rc;
      }
    }
    if (it < max_it && v.drain_poll) {
      HIPCHK(hipMemcpyAsync(S->sc_host, S->sc, sizeof(PcgScalars), hipMemcpyDeviceToHost, S->stream));
      HIPCHK(hipStreamSynchronize(S->stream));
      stop = S->sc_host->done != 0;
    } else
    if (it < max_it) {   // poll the device-side convergence flag (identical on every rank): one chunk late, see above
      const int slot = chunk & 1;
      if (chunk > 0) {                                      // the poll behind the previous chunk
        HIPCHK(hipEventSynchronize(S->poll_event[slot ^ 1]));
        stop = S->poll_host[slot ^ 1].done != 0;
      }
      HIPCHK(hipMemcpyAsync(&S->poll_host[slot], S->sc, sizeof(PcgScalars), hipMemcpyDeviceToHost, S->stream));
      HIPCHK(hipEventRecord(S->poll_event[slot], S->stream));
      ++chunk;
    }
  }
  return EULER_OK;
}

// 5. the finish: z whole again, the last p += alpha s, the pressure exchange, the velocity update
static int project_finish(euler_sim* S, float dt, const Solve& v) {
  int rc;
  S->prof_iter = -2;
  // z whole again where the solve's last z-forming pass left its halo only (converged before iteration max_it - 2): from r, which nothing has touched since - the same bits
  S->z_halo_last = 0;
  if (v.zr_ran && (rc = eu_launch_precond_tile(S, 0, 1, -1, 0, 0.0, false, 2))) return rc;
  // the last p += alpha s (the others rode along with the apply_a passes): in memory where a communicator needs the finished rows (and in the two-pass form), else inside the
  // velocity update's pass (k_grid.hip k_velocity_update_para)
  const bool finish_in_update = !S->has_comm && !S->slab_on && S->opt[EULER_OPT_VELOCITY_TWO_PASS] == 0;
  if (!finish_in_update) { if ((rc = eu_launch_finish_p(S))) return rc; }
  if (S->s_ring_n > 2) { S->s = S->s_base[0]; S->s2 = S->s_base[1]; }      // between solves S->s / S->s2 are the handle's own two arrays (EULER_F_PCG_S finds the last direction in the ring)
  if (S->has_comm && S->slab_on) {
    // row slabs: the velocity update of the highest own row reads p one row up (main.c:800) - one ghost row from the rank above
    const int X = S->X, nbk = (X + 255) / 256;
    double *send_lo = S->halo_buf, *send_hi = S->halo_buf + X, *recv_lo = S->halo_buf + 2 * X, *recv_hi = S->halo_buf + 3 * X;
    if (S->band_lo > 0) hipLaunchKernelGGL(k_pack_row, dim3(nbk), dim3(256), 0, S->stream, S->p, send_lo, S->geom, S->band_lo, 0);
    COMM_CALL(S->bulk.halo(S->bulk.ctx, send_lo, send_hi, recv_lo, recv_hi, X));
    if (S->band_hi < S->geom.nbands) hipLaunchKernelGGL(k_unpack_row, dim3(nbk), dim3(256), 0, S->stream, S->p, recv_hi, S->geom, S->band_hi, 0);
  } else if (S->has_comm) {   // every rank needs the whole pressure field for the replicated velocity update
    const int n = S->comm.nranks, nb = S->geom.nbands;
    std::vector<int64_t> off(n), cnt(n);
    for (int k = 0; k < n; ++k) {
      const int64_t lo = (int64_t)nb * k / n, hi = (int64_t)nb * (k + 1) / n;
      off[k] = lo * S->geom.TS * 64 * 8;
      cnt[k] = (hi - lo) * S->geom.TS * 64 * 8;
    }
    COMM_CALL(S->comm.allgather(S->comm.ctx, S->p, off.data(), cnt.data()));
  }
  if ((rc = eu_launch_velocity_update(S, dt, finish_in_update ? 1 : 0))) return rc;
  HIPCHK(hipMemcpyAsync(S->sc_host, S->sc, sizeof(PcgScalars), hipMemcpyDeviceToHost, S->stream));
  return EULER_OK;
}

// project() (main.c:709-806).  With a communicator every launch below covers this rank's bands
// only; the exchange points are: OR of all_zero(r), the band hand-off rows around each sweep
// (exact coupling), the ghost rows of s before apply_a, one scalar all-reduce per reduction, and
// the all-gather of p before the (replicated) velocity update.
int eu_launch_project(euler_sim* S, float dt) {
  Solve v = {};
  int rc;
  if ((rc = project_begin(S, dt, v))) return rc;
  if ((rc = project_resident(S, dt, v)) || v.solved) return rc;
  if ((rc = project_first_direction(S, v))) return rc;
  if ((rc = project_iterate(S, v))) return rc;
  return project_finish(S, dt, v);
}

// single building blocks for kernel-level parity tests (euler_pcg_op)
int eu_launch_pcg_op(euler_sim* S, int op, float dt, double a, double* out) {
  S->s_none = 0;
  S->s_launched = 0;      // (a single operation works on S->s as it stands)
  const bool want_scalar = op == EULER_OP_DOT_ZR || op == EULER_OP_DOT_ZS || op == EULER_OP_INF_NORM_R;
  const size_t SS = S->geom.S;
  if (eu_is_two_level(S) && (op == EULER_OP_PRECON_FACTOR || op == EULER_OP_FORWARD_SOLVE || op == EULER_OP_BACKWARD_SOLVE)) {
    // the coarse level is assembled over a solve's chunk list and lives in the solve: a single forced operation would return the tile level alone
    eu_set_error("euler_pcg_op: the preconditioner of EULER_PRECOND_IC0_TILE2 / _MG is not available as a single operation (select EULER_PRECOND_IC0_TILE for its tile level)");
    return EULER_EINVAL;
  }
  switch (op) {
    case EULER_OP_BUILD_SYSTEM:
      LAUNCH(S, KC_MISC, k_pcg_reset, dim3(1), dim3(1), S->sc, S->cfg.tol, S->cfg.max_iterations);
      eu_launch_build_system(S, dt);
      break;
    case EULER_OP_PRECON_FACTOR: if (tile_fused(S)) eu_launch_factor_tile(S, 1); else eu_launch_sweep(S, SW_FACTOR, KC_PRECON_FACTOR, 1); break;
    // tile-local mode has no forward solve of its own (q lives in registers): BACKWARD_SOLVE runs the whole Z = M^-1 R
    case EULER_OP_FORWARD_SOLVE: if (!tile_fused(S)) eu_launch_sweep(S, SW_FORWARD, KC_FORWARD_SOLVE, 1); break;
    case EULER_OP_BACKWARD_SOLVE:
      if (tile_fused(S)) eu_launch_precond_tile(S, 0, 1, FIN_STORE_ONLY, 1, 0.0); else eu_launch_sweep(S, SW_BACKWARD, KC_BACKWARD_SOLVE, 1);
      break;
    case EULER_OP_APPLY_A:
      LAUNCH(S, KC_APPLY_A, k_apply_a, dim3(S->red_blocks), dim3(RED_THREADS), S->s, S->z, S->cellmask, S->geom,
             S->partial, S->sc, 1, S->red_counter, -1);
      break;
    case EULER_OP_DOT_ZR: eu_launch_dot(S, S->z, S->r, FIN_STORE_ONLY, 1); break;
    case EULER_OP_DOT_ZS: eu_launch_dot(S, S->z, S->s, FIN_STORE_ONLY, 1); break;
    case EULER_OP_INF_NORM_R:
      LAUNCH(S, KC_UPDATE_PR, k_inf_norm, dim3(S->red_blocks), dim3(RED_THREADS), S->r, S->cellmask, SS, S->partial);
      LAUNCH(S, KC_REDUCE_FINAL, k_reduce_final<true>, dim3(1), dim3(RED_THREADS), S->partial, S->red_blocks, S->sc,
             (int)FIN_STORE_ONLY, 1);
      break;
    case EULER_OP_UPDATE_PR:
      LAUNCH(S, KC_UPDATE_PR, k_update_pr, dim3(S->red_blocks), dim3(RED_THREADS), S->p, S->r, S->s, S->z, S->cellmask,
             SS, S->partial, S->sc, 1, a, S->red_counter, -1);
      break;
    case EULER_OP_UPDATE_SEARCH:
      LAUNCH(S, KC_UPDATE_SEARCH, k_update_search<false>, dim3(eu_blocks(SS, 256 * 4, 4096)), dim3(256), S->s, S->z,
             S->cellmask, SS, S->sc, 1, a);
      break;
    default: eu_set_error("unknown pcg op %d", op); return EULER_EINVAL;
  }
  HIPCHK(hipMemcpyAsync(S->sc_host, S->sc, sizeof(PcgScalars), hipMemcpyDeviceToHost, S->stream));
  HIPCHK(hipStreamSynchronize(S->stream));
  if (want_scalar && out) *out = S->sc_host->sigma_new;
  return EULER_OK;
}
