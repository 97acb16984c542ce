// k_mg_cycle.hip — the multilevel preconditioner's V-cycle (k_mg.hip's header comment describes it; the hierarchy and the per-solve operators live there): the kernels
// k_mg_down1, k_mg_down, k_mg_up, k_mg_up0, their launchers (k_mg.h: the split cycle of k_mg_split.hip launches the same kernels on row ranges through them) and the
// replicated cycle, eu_mg_solve.
#include "k_pcg.h"

// ------------------------------------------------------------------------------------------ per iteration: the cycle
struct MgRect { int i0, i1, j0, j1; };      // rows [i0, i1) x columns [j0, j1)
__device__ __forceinline__ int mg_rw(const MgRect& r) { return r.j1 - r.j0; }
__device__ __forceinline__ int mg_rn(const MgRect& r) { return (r.i1 - r.i0) * (r.j1 - r.j0); }
__device__ __forceinline__ MgRect mg_grow(const MgRect& r, int ny, int nx) {
  return MgRect{r.i0 > 0 ? r.i0 - 1 : 0, r.i1 < ny ? r.i1 + 1 : ny, r.j0 > 0 ? r.j0 - 1 : 0, r.j1 < nx ? r.j1 + 1 : nx};
}
// the nodes of level l whose residual feeds the nodes `c` of level l + 1
__device__ __forceinline__ MgRect mg_fine_of(const MgRect& c, int ny, int nx) {
  MgRect f = {2 * c.i0 - 1, 2 * c.i1, 2 * c.j0 - 1, 2 * c.j1};
  if (f.i0 < 0) f.i0 = 0;
  if (f.j0 < 0) f.j0 = 0;
  if (f.i1 > ny) f.i1 = ny;
  if (f.j1 > nx) f.j1 = nx;
  return f;
}
// the nodes of level l that the owner of the nodes `c` of level l + 1 writes (a partition of level l)
__device__ __forceinline__ MgRect mg_owned_of(const MgRect& c, int cny, int cnx, int ny, int nx) {
  return MgRect{2 * c.i0, c.i1 == cny ? ny : 2 * c.i1, 2 * c.j0, c.j1 == cnx ? nx : 2 * c.j1};
}
__device__ __forceinline__ bool mg_in(const MgRect& r, int i, int j) { return i >= r.i0 && i < r.i1 && j >= r.j0 && j < r.j1; }

#define MG_DOWN_THREADS 1024
#define MG_SPLIT 704          // threads [0, MG_SPLIT) serve a launch's second level (<= 25 x 25 nodes + a row of slack), the others its third (<= 11 x 11)

__device__ __forceinline__ void mg_st_agent(double* p, double v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double mg_ld_agent(const double* p) {
  return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// (A_l v)[c] over a patch of v in LDS: entries k = 0 .. 8 in this order, neighbours outside the grid skipped
__device__ __forceinline__ double mg_apply_patch(const double* __restrict__ a, size_t n, size_t c, int i, int j, int ny, int nx, const double* v, const MgRect& R) {
  const int w = mg_rw(R);
  double t = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int i2 = i + k / 3 - 1, j2 = j + k % 3 - 1;
    if (i2 < 0 || i2 >= ny || j2 < 0 || j2 >= nx) continue;
    t = t + a[(size_t)k * n + c] * v[(i2 - R.i0) * w + (j2 - R.j0)];
  }
  return t;
}

// the tail: levels lB .. top by ONE workgroup of 1024 threads, a thread per node (tid < n_l); vectors in LDS, stencils in registers
__device__ void mg_tail(const MgDownArgs& A, double* lds) {
  const MgHier& H = A.H;
  const int tid = threadIdx.x, top = H.nl - 1, nt = top - A.lB;      // nt stencil levels, then the dense one
  const int ntop = H.nx[top] * H.ny[top];
  // LDS: per stencil level of the tail two vectors (x1 -> x, t / x2), then the dense level's right-hand side and result, then its inverse
  double* vec[MG_TAIL_LEVELS];
  double* p = lds;
#pragma unroll
  for (int q = 0; q < MG_TAIL_LEVELS; ++q) { vec[q] = p; if (q < nt) p += 2 * (size_t)H.nx[A.lB + q] * H.ny[A.lB + q]; }
  double* top_rhs = p;
  double* top_y = p + ntop;
  double* s_inv = p + 2 * ntop;
  // everything this workgroup needs from memory, in one batch: the entry level's right-hand side (published by all workgroups), the stencils, the inverse
  double rhs[MG_TAIL_LEVELS], a[MG_TAIL_LEVELS][9], wd[MG_TAIL_LEVELS];
#pragma unroll
  for (int q = 0; q < MG_TAIL_LEVELS; ++q) {
    rhs[q] = 0.0; wd[q] = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) a[q][k] = 0.0;
    if (q < nt) {
      const int l = A.lB + q;
      const size_t n = (size_t)H.nx[l] * H.ny[l];
      if ((size_t)tid < n) {
        const double* st = mg_sten(H, l);
#pragma unroll
        for (int k = 0; k < 9; ++k) a[q][k] = st[(size_t)k * n + tid];
        wd[q] = H.wd[H.off[l] + tid];
      }
    }
  }
  {
    const size_t n = (size_t)H.nx[A.lB] * H.ny[A.lB];
    if ((size_t)tid < n) rhs[0] = mg_ld_agent(H.rhs + H.off[A.lB] + tid);
  }
  for (int e = tid; e < ntop * ntop; e += MG_DOWN_THREADS) s_inv[e] = A.inv[e];
  // ---- down
#pragma unroll
  for (int q = 0; q < MG_TAIL_LEVELS; ++q) {
    if (q >= nt) break;
    const int l = A.lB + q, nx = H.nx[l], ny = H.ny[l], n = nx * ny;
    const int cnx = H.nx[l + 1], cny = H.ny[l + 1], cn = cnx * cny;
    double* x1 = vec[q];
    double* tt = vec[q] + n;
    if (tid < n) x1[tid] = wd[q] * rhs[q];
    __syncthreads();
    if (tid < n) {
      const int i = tid / nx, j = tid % nx;
      double t = 0.0;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const int i2 = i + k / 3 - 1, j2 = j + k % 3 - 1;
        if (i2 < 0 || i2 >= ny || j2 < 0 || j2 >= nx) continue;
        t = t + a[q][k] * x1[i2 * nx + j2];
      }
      tt[tid] = wd[q] != 0.0 ? rhs[q] - t : 0.0;
    }
    __syncthreads();
    if (tid < cn) {      // full weighting: rows outer, columns inner
      const int I = tid / cnx, J = tid % cnx;
      double t = 0.0;
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const double w = mg_w1(I, 2 * I + dy, ny, cny) * mg_w1(J, 2 * J + dx, nx, cnx);
          if (w != 0.0) t = t + w * tt[(2 * I + dy) * nx + 2 * J + dx];
        }
      if (q + 1 < MG_TAIL_LEVELS && q + 1 < nt) rhs[q + 1] = t;
      if (q + 1 == nt) top_rhs[tid] = t;      // the dense level's right-hand side
    }
  }
  if (nt == 0 && tid < ntop) top_rhs[tid] = rhs[0];      // (the entry level IS the dense level)
  __syncthreads();
  // ---- the dense level: y = inv rhs, 16 threads per row
  {
    double* rt = top_rhs;
    double* yt = top_y;
    const int row = tid >> 4, part = tid & 15;
    double v = 0.0;
    if (row < ntop) for (int c = part; c < ntop; c += 16) v += s_inv[row * ntop + c] * rt[c];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (row < ntop && part == 0) yt[row] = v;
    __syncthreads();
    if (nt == 0 && tid < ntop) H.x[H.off[top] + tid] = yt[tid];
  }
  // ---- up
#pragma unroll
  for (int q = MG_TAIL_LEVELS - 1; q >= 0; --q) {
    if (q >= nt) continue;
    const int l = A.lB + q, nx = H.nx[l], ny = H.ny[l], n = nx * ny;
    const int cnx = H.nx[l + 1], cny = H.ny[l + 1];
    double* x1 = vec[q];            // becomes x
    double* x2 = vec[q] + n;
    const double* e = q + 1 == nt ? top_y : vec[q + 1 < MG_TAIL_LEVELS ? q + 1 : q];
    if (tid < n) {
      const int i = tid / nx, j = tid % nx;
      const int I = i >> 1, J = j >> 1;
      const int I1 = (i & 1) && I + 1 <= cny - 1 ? I + 1 : I, J1 = (j & 1) && J + 1 <= cnx - 1 ? J + 1 : J;
      const double fy = (i & 1) && I + 1 <= cny - 1 ? 0.5 : 0.0, fx = (j & 1) && J + 1 <= cnx - 1 ? 0.5 : 0.0;
      const double lo = (1.0 - fx) * e[I * cnx + J] + fx * e[I * cnx + J1];
      const double hi = (1.0 - fx) * e[I1 * cnx + J] + fx * e[I1 * cnx + J1];
      x2[tid] = wd[q] != 0.0 ? x1[tid] + ((1.0 - fy) * lo + fy * hi) : 0.0;
    }
    __syncthreads();
    double xv = 0.0;
    if (tid < n) {
      const int i = tid / nx, j = tid % nx;
      double t = 0.0;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const int i2 = i + k / 3 - 1, j2 = j + k % 3 - 1;
        if (i2 < 0 || i2 >= ny || j2 < 0 || j2 >= nx) continue;
        t = t + a[q][k] * x2[i2 * nx + j2];
      }
      xv = wd[q] != 0.0 ? x2[tid] + wd[q] * (rhs[q] - t) : 0.0;
    }
    __syncthreads();
    if (tid < n) { x1[tid] = xv; if (q == 0) H.x[H.off[l] + tid] = xv; }
    __syncthreads();
  }
}

// One level of the way down inside a workgroup: the residual behind the Jacobi step (in place of the right-hand side patch), then full weighting into the next level's
// patch.  The stencils of the NS nodes a thread handles sit in registers (loaded when the kernel starts, together with everything else that does not depend on the
// level above: the phases wait for LDS only); the threads [toff, toff + ...) do the work (the small levels of a launch use disjoint thread ranges, so a thread holds the
// first level's slots and at most one more).
template <int NS>
__device__ __forceinline__ void mg_prefetch_sten(const MgHier& H, int l, const MgRect& T, int toff, double (&a)[NS][9]) {
  const int tid = (int)threadIdx.x - toff, nx = H.nx[l], tw = mg_rw(T), tn = mg_rn(T);
  const size_t n = (size_t)nx * H.ny[l];
  const double* st = mg_sten(H, l);
#pragma unroll
  for (int u = 0; u < NS; ++u) {
    const int e = tid + u * MG_DOWN_THREADS;
    const bool on = tid >= 0 && e < tn;
    const size_t c = on ? (size_t)(T.i0 + e / tw) * nx + T.j0 + e % tw : 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) a[u][k] = on ? st[(size_t)k * n + c] : 0.0;
  }
}
template <int NS>
__device__ __forceinline__ void mg_residual_patch(const MgHier& H, int l, const MgRect& R, const MgRect& T, int toff, const double (&a)[NS][9], double* prhs, const double* px1) {
  const int tid = (int)threadIdx.x - toff, nx = H.nx[l], ny = H.ny[l], w = mg_rw(R), tw = mg_rw(T), tn = mg_rn(T);
#pragma unroll
  for (int u = 0; u < NS; ++u) {
    const int e = tid + u * MG_DOWN_THREADS;
    if (tid < 0 || e >= tn) continue;
    const int i = T.i0 + e / tw, j = T.j0 + e % tw;
    const int pe = (i - R.i0) * w + (j - R.j0);
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int i2 = i + k / 3 - 1, j2 = j + k % 3 - 1;
      if (i2 < 0 || i2 >= ny || j2 < 0 || j2 >= nx) continue;
      t = t + a[u][k] * px1[pe + (k / 3 - 1) * w + (k % 3 - 1)];
    }
    prhs[pe] = a[u][4] != 0.0 ? prhs[pe] - t : 0.0;
  }
}

template <bool GATHER>
__global__ __launch_bounds__(MG_DOWN_THREADS) void k_mg_down(MgDownArgs A) {
  extern __shared__ double lds[];
  __shared__ int s_last;
  if (!A.force && pcg_idle(A.sc)) return;      // (the host polls late: launches queued behind convergence do no work - main.c:757 has left the loop)
  const MgHier& H = A.H;
  const int tid = threadIdx.x;
  const int tiles_x = (H.nx[A.lB] + A.tile - 1) / A.tile;
  const int ti = A.tile_row0 + blockIdx.x / tiles_x, tj = blockIdx.x % tiles_x;
  MgRect own = {ti * A.tile, (ti + 1) * A.tile, tj * A.tile, (tj + 1) * A.tile};
  if (own.i1 > H.ny[A.lB]) own.i1 = H.ny[A.lB];
  if (own.j1 > H.nx[A.lB]) own.j1 = H.nx[A.lB];
  // the rectangles of level l: R = the right-hand side this workgroup needs, T = where it needs the residual, O = what it writes out
  auto rects = [&](int l, MgRect& R, MgRect& T, MgRect& O) {
    MgRect r = own, o = own, t = own;
    for (int k = A.lB - 1; k >= l; --k) {
      o = mg_owned_of(o, H.ny[k + 1], H.nx[k + 1], H.ny[k], H.nx[k]);
      t = mg_fine_of(r, H.ny[k], H.nx[k]);
      r = mg_grow(t, H.ny[k], H.nx[k]);
    }
    R = r; T = t; O = o;
  };
  const int nt = A.lB - A.lA;      // transitions of this launch: 0 .. 3
  double* buf[2] = {lds, lds + 2 * (size_t)A.cap0};
  int cap[2] = {A.cap0, A.cap1};
  // ---- everything that does not depend on another level, in one batch: the stencils of the nodes this thread handles (level lA: up to three per thread; lA + 1 and lA + 2:
  // one, on the threads below / from MG_SPLIT), omega / diagonal of the right-hand-side nodes, the entry level's right-hand side itself
  double a0[3][9], an[1][9], w0[3], wn = 0.0;      // (an: level lA + 1's stencil on the threads below MG_SPLIT, level lA + 2's on the others)
  MgRect R0, T0, O0;
  rects(A.lA, R0, T0, O0);
  if (nt >= 1) mg_prefetch_sten<3>(H, A.lA, T0, 0, a0);
#pragma unroll
  for (int k = 0; k < 9; ++k) an[0][k] = 0.0;
  if (nt >= 2 && tid < MG_SPLIT) { MgRect R, T, O; rects(A.lA + 1, R, T, O); mg_prefetch_sten<1>(H, A.lA + 1, T, 0, an); }
  if (nt >= 3 && tid >= MG_SPLIT) { MgRect R, T, O; rects(A.lA + 2, R, T, O); mg_prefetch_sten<1>(H, A.lA + 2, T, MG_SPLIT, an); }
  {      // omega / diagonal of the level this thread writes a right-hand side of in the restriction phases: lA + 1 on the threads below MG_SPLIT, lA + 2 from there
    if (nt >= 2 && tid < MG_SPLIT) { MgRect R, T, O; rects(A.lA + 1, R, T, O); if (tid < mg_rn(R)) wn = H.wd[H.off[A.lA + 1] + (size_t)(R.i0 + tid / mg_rw(R)) * H.nx[A.lA + 1] + R.j0 + tid % mg_rw(R)]; }
    if (nt >= 3 && tid >= MG_SPLIT) { MgRect R, T, O; rects(A.lA + 2, R, T, O); const int e = tid - MG_SPLIT; if (e < mg_rn(R)) wn = H.wd[H.off[A.lA + 2] + (size_t)(R.i0 + e / mg_rw(R)) * H.nx[A.lA + 2] + R.j0 + e % mg_rw(R)]; }
  }
  {
    const int l = A.lA, nx = H.nx[l], w = mg_rw(R0), rn = mg_rn(R0);
    double v0[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const int e = tid + u * MG_DOWN_THREADS;
      v0[u] = 0.0; w0[u] = 0.0;
      if (e >= rn) continue;
      const int i = R0.i0 + e / w, j = R0.j0 + e % w;
      const size_t c = (size_t)i * nx + j;
      w0[u] = H.wd[H.off[l] + c];
      v0[u] = GATHER ? mg_gather0(A.part, i, j, A.ntb, A.band_lo, A.band_hi) : ((i >= A.clip_lo && i < A.clip_hi) ? H.rhs[H.off[l] + c] : 0.0);
    }
    double* prhs = buf[0];
    double* px1 = buf[0] + cap[0];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const int e = tid + u * MG_DOWN_THREADS;
      if (e >= rn) continue;
      const int i = R0.i0 + e / w, j = R0.j0 + e % w;
      if (GATHER && mg_in(O0, i, j)) {
        const size_t c = (size_t)i * nx + j;
        if (A.tail && nt == 0) mg_st_agent(H.rhs + H.off[l] + c, v0[u]);
        else H.rhs[H.off[l] + c] = v0[u];
      }
      prhs[e] = v0[u];
      px1[e] = w0[u] * v0[u];
    }
  }
  __syncthreads();
  // ---- level transitions lA -> lA + 1 -> ... -> lB
  for (int l = A.lA; l < A.lB; ++l) {
    const int rel = l - A.lA, cur = rel & 1;
    MgRect R, T, O, Rc, Tc, Oc;
    rects(l, R, T, O);
    rects(l + 1, Rc, Tc, Oc);
    const int nx = H.nx[l], ny = H.ny[l];
    const int cnx = H.nx[l + 1], cny = H.ny[l + 1];
    double* prhs = buf[cur];
    double* px1 = buf[cur] + cap[cur];
    double* crhs = buf[cur ^ 1];
    double* cx1 = buf[cur ^ 1] + cap[cur ^ 1];
    const int w = mg_rw(R);
    // residual behind the Jacobi step, in place of the right-hand side
    if (rel == 0) mg_residual_patch<3>(H, l, R, T, 0, a0, prhs, px1);
    else if (rel == 1) mg_residual_patch<1>(H, l, R, T, 0, an, prhs, px1);
    else mg_residual_patch<1>(H, l, R, T, MG_SPLIT, an, prhs, px1);
    __syncthreads();
    // full weighting -> the next level's right-hand side (and its Jacobi step): the threads below MG_SPLIT for lA + 1 (and for a launch's last level), from MG_SPLIT for lA + 2
    const int toff = rel == 1 && l + 1 < A.lB ? MG_SPLIT : 0;
    const int cw = mg_rw(Rc), cn = mg_rn(Rc);
    for (int e = tid - toff; e >= 0 && e < cn; e += MG_DOWN_THREADS) {
      const int I = Rc.i0 + e / cw, J = Rc.j0 + e % cw;
      const size_t c = (size_t)I * cnx + J;
      double t = 0.0;
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const double wgt = mg_w1(I, 2 * I + dy, ny, cny) * mg_w1(J, 2 * J + dx, nx, cnx);
          if (wgt != 0.0) t = t + wgt * prhs[(2 * I + dy - R.i0) * w + (2 * J + dx - R.j0)];
        }
      if (mg_in(Oc, I, J)) {
        if (A.tail && l + 1 == A.lB) mg_st_agent(H.rhs + H.off[l + 1] + c, t);
        else H.rhs[H.off[l + 1] + c] = t;
      }
      if (l + 1 < A.lB) { crhs[e] = t; cx1[e] = wn * t; }      // (one node per thread on these levels: wn is this node's omega / diagonal)
    }
    __syncthreads();
  }
  if (!A.tail) return;
  // ---- the last workgroup to get here takes the small levels
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const unsigned int t = __hip_atomic_fetch_add(A.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = t == gridDim.x - 1;
    if (s_last) __hip_atomic_store(A.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!s_last) return;
  mg_tail(A, lds);
}

#ifndef MG_UP_THREADS
#define MG_UP_THREADS 1024
#endif
__device__ __forceinline__ MgRect mg_coarse_around(const MgRect& f, int cny, int cnx) {
  MgRect c = {f.i0 >> 1, ((f.i1 - 1) >> 1) + 2, f.j0 >> 1, ((f.j1 - 1) >> 1) + 2};
  if (c.i1 > cny) c.i1 = cny;
  if (c.j1 > cnx) c.j1 = cnx;
  return c;
}
__global__ __launch_bounds__(MG_UP_THREADS) void k_mg_up(MgUpArgs A) {
  extern __shared__ double lds[];
  __shared__ double s_red[MG_UP_THREADS / 64];
  __shared__ int s_last;
  const MgHier& H = A.H;
  const int tid = threadIdx.x;
  if (!A.force && pcg_idle(A.sc)) return;      // behind convergence the level arrays are dead and the scalar epilogue must not run: every workgroup leaves at once (round 6; rounds 3-5 did the whole pass and skipped the epilogue)
  // Water cut off from the air (rare): its pressure is determined up to a constant, PCG delivers the one with n . M p = 0 (M the preconditioner, n the region's indicator)
  // and the reference's clamp (main.c:773-779) makes that constant observable.  The tile-local factor alone gives, like the reference's own, very nearly "mean 0 over the
  // region"; the dense level's pseudo-inverse keeps that, the Jacobi steps of the levels in between do not - so the correction is made mean-free over the CELLS of every
  // such region: x_0 -= n_0 (m_0 . x_0) / (m_0 . n_0).  The workgroups leave partials of m_0 . x_0, the last one folds them and corrects x_0 (oracle: mg_gauge).
  const int n_null = (int)A.nullv[MG_NULL_MAX * 256];
  const size_t n0n = (size_t)H.nx[0] * H.ny[0];
  double gv[MG_NULL_MAX] = {0.0, 0.0, 0.0, 0.0};
  const int L0 = A.l0;
  const int tiles_x = (H.nx[L0] + A.tile - 1) / A.tile;
  const int ti = A.tile_row0 + blockIdx.x / tiles_x, tj = blockIdx.x % tiles_x;
  MgRect own = {ti * A.tile, (ti + 1) * A.tile, tj * A.tile, (tj + 1) * A.tile};
  if (own.i1 > H.ny[L0]) own.i1 = H.ny[L0];
  if (own.j1 > H.nx[L0]) own.j1 = H.nx[L0];
  auto rects = [&](int l, MgRect& X, MgRect& X2) {      // X_l: where x_l is needed; X2_l = X_l grown by one
    MgRect x = own, x2 = mg_grow(own, H.ny[L0], H.nx[L0]);
    for (int k = L0 + 1; k <= l; ++k) { x = mg_coarse_around(x2, H.ny[k], H.nx[k]); x2 = mg_grow(x, H.ny[k], H.nx[k]); }
    X = x; X2 = x2;
  };
  double* bx[2] = {lds, lds + A.cap};      // x of the level above / of this level, alternating
  double* b2 = lds + 2 * (size_t)A.cap;    // x2 of this level
  // ---- everything that does not depend on the level above, in one batch.  Level 0: two nodes of X2 and one of X per thread; the coarser levels are small - the thread
  // ranges [off_l, off_l + |X2_l|) are disjoint, so a thread serves level 0 and at most one more (`myl`)
  double w2a[2] = {0.0, 0.0}, r2a[2] = {0.0, 0.0}, a0[9], w0 = 0.0, r0 = 0.0;      // level 0
  double w2m = 0.0, r2m = 0.0, am[9], wm = 0.0, rm = 0.0;                              // level myl
  int myl = -1, mye = 0;
#pragma unroll
  for (int k = 0; k < 9; ++k) { a0[k] = 0.0; am[k] = 0.0; }
  if (A.lC > L0) {
    MgRect X, X2;
    rects(L0, X, X2);
    const int nx = H.nx[L0];
    const size_t n = (size_t)nx * H.ny[L0];
    const int w2 = mg_rw(X2), w = mg_rw(X);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int e = tid + u * MG_UP_THREADS;
      if (e < mg_rn(X2)) { const size_t c = H.off[L0] + (size_t)(X2.i0 + e / w2) * nx + X2.j0 + e % w2; w2a[u] = H.wd[c]; r2a[u] = H.rhs[c]; }
    }
    if (tid < mg_rn(X)) {
      const size_t c = (size_t)(X.i0 + tid / w) * nx + X.j0 + tid % w;
      const double* st = mg_sten(H, L0);
#pragma unroll
      for (int k = 0; k < 9; ++k) a0[k] = st[(size_t)k * n + c];
      w0 = H.wd[H.off[L0] + c]; r0 = H.rhs[H.off[L0] + c];
    }
    int off = 0;
    for (int l = L0 + 1; l < A.lC; ++l) {
      rects(l, X, X2);
      const int e = tid - off, n2 = mg_rn(X2);
      if (e >= 0 && e < n2) {
        myl = l; mye = e;
        const int lnx = H.nx[l];
        const size_t ln = (size_t)lnx * H.ny[l];
        const int lw2 = mg_rw(X2), lw = mg_rw(X);
        const size_t c2 = (size_t)(X2.i0 + e / lw2) * lnx + X2.j0 + e % lw2;
        w2m = H.wd[H.off[l] + c2]; r2m = H.rhs[H.off[l] + c2];
        if (e < mg_rn(X)) {
          const size_t c = (size_t)(X.i0 + e / lw) * lnx + X.j0 + e % lw;
          const double* st = mg_sten(H, l);
#pragma unroll
          for (int k = 0; k < 9; ++k) am[k] = st[(size_t)k * ln + c];
          wm = H.wd[H.off[l] + c]; rm = H.rhs[H.off[l] + c];
        }
      }
      off += n2;
    }
    rects(A.lC, X, X2);
    const int cw = mg_rw(X), cnx = H.nx[A.lC];
    double* dst = bx[A.lC & 1];
    for (int e = tid; e < mg_rn(X); e += MG_UP_THREADS) dst[e] = H.x[H.off[A.lC] + (size_t)(X.i0 + e / cw) * cnx + X.j0 + e % cw];
    __syncthreads();
  }
  double dv = 0.0;
  for (int l = A.lC - 1; l >= L0; --l) {
    MgRect X, X2, Xc, X2c;
    rects(l, X, X2);
    rects(l + 1, Xc, X2c);
    const int nx = H.nx[l], ny = H.ny[l];
    const int cnx = H.nx[l + 1], cny = H.ny[l + 1];
    const double* e_ = bx[(l + 1) & 1];
    double* xo = bx[l & 1];
    const int w2 = mg_rw(X2), cw = mg_rw(Xc), w = mg_rw(X);
    // x2 = the Jacobi step + P x_(l+1) on X2
    auto x2_at = [&](int e, double wdv, double rv) __attribute__((always_inline)) {
      const int i = X2.i0 + e / w2, j = X2.j0 + e % w2;
      const int I = i >> 1, J = j >> 1;
      const bool oy = (i & 1) && I + 1 <= cny - 1, ox = (j & 1) && J + 1 <= cnx - 1;
      const int I1 = oy ? I + 1 : I, J1 = ox ? J + 1 : J;
      const double fy = oy ? 0.5 : 0.0, fx = ox ? 0.5 : 0.0;
      const double lo = (1.0 - fx) * e_[(I - Xc.i0) * cw + (J - Xc.j0)] + fx * e_[(I - Xc.i0) * cw + (J1 - Xc.j0)];
      const double hi = (1.0 - fx) * e_[(I1 - Xc.i0) * cw + (J - Xc.j0)] + fx * e_[(I1 - Xc.i0) * cw + (J1 - Xc.j0)];
      b2[e] = wdv != 0.0 ? wdv * rv + ((1.0 - fy) * lo + fy * hi) : 0.0;
    };
    if (l == L0) {
#pragma unroll
      for (int u = 0; u < 2; ++u) { const int e = tid + u * MG_UP_THREADS; if (e < mg_rn(X2)) x2_at(e, w2a[u], r2a[u]); }
    } else if (l == myl) x2_at(mye, w2m, r2m);
    __syncthreads();
    // x = x2 + (omega / d) (rhs - A x2) on X
    auto x_at = [&](int e, const double (&a)[9], double wdv, double rv) __attribute__((always_inline)) {
      const int i = X.i0 + e / w, j = X.j0 + e % w;
      const int pe = (i - X2.i0) * w2 + (j - X2.j0);
      double t = 0.0;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const int i2 = i + k / 3 - 1, j2 = j + k % 3 - 1;
        if (i2 < 0 || i2 >= ny || j2 < 0 || j2 >= nx) continue;
        t = t + a[k] * b2[pe + (k / 3 - 1) * w2 + (k % 3 - 1)];
      }
      const double xv = wdv != 0.0 ? b2[pe] + wdv * (rv - t) : 0.0;
      xo[e] = xv;
      if (l == L0 && L0 > 0) { if (mg_in(own, i, j)) H.x[H.off[L0] + (size_t)i * nx + j] = xv; }      // (level 0 follows in k_mg_up0)
      if (l == 0) {
        const size_t c = (size_t)i * nx + j;
        if (n_null > 0) {
          mg_st_agent(H.x + c, xv);
#pragma unroll
          for (int q = 0; q < MG_NULL_MAX; ++q) if (q < n_null) gv[q] += A.m0[(size_t)q * n0n + c] * xv;
        } else H.x[c] = xv;
        if (i >= A.row_lo && i < A.row_hi) dv += xv * rv;
      }
    };
    if (l == L0) { if (tid < mg_rn(X)) x_at(tid, a0, w0, r0); }
    else if (l == myl && mye < mg_rn(X)) x_at(mye, am, wm, rm);
    __syncthreads();
  }
  if (A.lC == 0) {      // level 0 is the tail's own level: only the dot product is left
    const int w = mg_rw(own), nx = H.nx[0];
    for (int e = tid; e < mg_rn(own); e += MG_UP_THREADS) {
      const int i = own.i0 + e / w, j = own.j0 + e % w;
      const size_t c = (size_t)i * nx + j;
      const double xv = n_null > 0 ? mg_ld_agent(H.x + c) : H.x[c];      // (written by the tail workgroup of the launch before)
      if (i >= A.row_lo && i < A.row_hi) dv += xv * H.rhs[c];
#pragma unroll
      for (int q = 0; q < MG_NULL_MAX; ++q) if (q < n_null) gv[q] += A.m0[(size_t)q * n0n + c] * xv;
    }
  }
  if (L0 > 0) return;      // (L0 > 0: level 0, the dot product and the epilogue are k_mg_up0's)
  for (int q = 0; q < n_null && q < MG_NULL_MAX; ++q) {
    double g = q == 0 ? gv[0] : q == 1 ? gv[1] : q == 2 ? gv[2] : gv[3];
    g = eu_wave_sum(g);
    __syncthreads();
    if ((tid & 63) == 0) s_red[tid >> 6] = g;
    __syncthreads();
    if (tid == 0) {
      double t = 0.0;
      for (int k = 0; k < MG_UP_THREADS / 64; ++k) t += s_red[k];
      mg_st_agent(A.dot_part + (size_t)(1 + q) * MG_DOT_BLOCKS + blockIdx.x, t);
    }
  }
  dv = eu_wave_sum(dv);
  __syncthreads();
  if ((tid & 63) == 0) s_red[tid >> 6] = dv;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // EVERY thread's x_0 stores have left before the workgroup's ticket is drawn (as in k_mg_down): the gauge pass of the last workgroup reads them
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int k = 0; k < MG_UP_THREADS / 64; ++k) t += s_red[k];
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(&A.dot_part[blockIdx.x]), (unsigned long long)__double_as_longlong(t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    s_last = __hip_atomic_fetch_add(A.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  for (int q = 0; q < n_null && q < MG_NULL_MAX; ++q) {      // the gauge: every workgroup's x_0 is in memory (agent-scope stores, drained before the tickets)
    double g = 0.0;
    for (unsigned int k = tid; k < gridDim.x; k += MG_UP_THREADS) g += mg_ld_agent(A.dot_part + (size_t)(1 + q) * MG_DOT_BLOCKS + k);
    g = eu_wave_sum(g);
    __syncthreads();
    if ((tid & 63) == 0) s_red[tid >> 6] = g;
    __syncthreads();
    double tot = 0.0;
    for (int k = 0; k < MG_UP_THREADS / 64; ++k) tot += s_red[k];
    const double mn = A.m0[(size_t)MG_NULL_MAX * n0n + q];
    if (mn > 0.0) {
      const double cq = tot / mn;
      for (size_t c = tid; c < n0n; c += MG_UP_THREADS) {
        const double nv = A.n0[(size_t)q * A.nstride + c];
        if (nv != 0.0) mg_st_agent(H.x + c, mg_ld_agent(H.x + c) - nv * cq);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  double t = 0.0;
  for (unsigned int k = tid; k < gridDim.x; k += MG_UP_THREADS)
    t += __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<unsigned long long*>(&A.dot_part[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  t = eu_wave_sum(t);
  __syncthreads();
  if ((tid & 63) == 0) s_red[tid >> 6] = t;
  __syncthreads();
  if (tid == 0) {
    double v = 0.0;
    for (int k = 0; k < MG_UP_THREADS / 64; ++k) v += s_red[k];
    if (A.fin_op == MG_FIN_SLOT) { A.sc->comm_val2 = v; if (A.sc->comm_slot) A.sc->comm_slot[1] += v; }      // (row slabs, split cycle: this rank's share travels with the pair)
    else {
      v = A.sc->sigma_new + v;      // k_precond_tile left dot(z_tile, r) there (FIN_STORE_ONLY)
      if (A.fin_op == FIN_SIGMA_INIT) A.sc->sigma = v;                                                       // main.c:748
      else if (A.fin_op == FIN_BETA) { A.sc->sigma_new = v; A.sc->beta = v / A.sc->sigma; A.sc->sigma = v; }   // main.c:762-765
      else A.sc->sigma_new = v;
    }
    __hip_atomic_store(A.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ------------------------------------------------------------------------------------------ the big level: level 0 <-> level 1 on small workgroups
// Level 0 holds most of the hierarchy's nodes (1024^2 of them on an 8192^2 grid).  The kernels above give a workgroup of 1024 threads one tile and hide nothing behind
// anything - right for the small levels, whose cost is the chain of phases.  Level 0 is the opposite case: many tiles, little work in each.  These two kernels take it with
// workgroups of 256 threads, several nodes per thread, loads issued where they are needed: five or six workgroups share a CU and one's phase waits behind another's loads
// (8192^2: 101 + 87 us for the two ends of the cycle as 1024-thread workgroups -> see DESIGN.md).
#ifndef MG_FINE_THREADS
#define MG_FINE_THREADS 256
#endif
// k_mg_down1: level 0's right-hand side from the tiles' partial sums (GATHER) or from H.rhs (row slabs: summed over the ranks before), its residual behind the Jacobi step,
// full weighting -> level 1's right-hand side.  A workgroup owns tile x tile nodes of level 1.
template <bool GATHER>
__global__ __launch_bounds__(MG_FINE_THREADS) void k_mg_down1(MgDownArgs A) {
  extern __shared__ double lds[];
  if (!A.force && pcg_idle(A.sc)) return;      // (as k_mg_down: nothing behind convergence)
  const MgHier& H = A.H;
  const int tid = threadIdx.x;
  const int nx = H.nx[0], ny = H.ny[0], cnx = H.nx[1], cny = H.ny[1];
  const size_t n = (size_t)nx * ny;
  const int tiles_x = (cnx + A.tile - 1) / A.tile;
  const int ti = A.tile_row0 + blockIdx.x / tiles_x, tj = blockIdx.x % tiles_x;
  MgRect own = {ti * A.tile, (ti + 1) * A.tile, tj * A.tile, (tj + 1) * A.tile};
  if (own.i1 > cny) own.i1 = cny;
  if (own.j1 > cnx) own.j1 = cnx;
  const MgRect O = mg_owned_of(own, cny, cnx, ny, nx), T = mg_fine_of(own, ny, nx), R = mg_grow(T, ny, nx);
  double* prhs = lds;
  double* px1 = lds + A.cap0;
  const double* st = mg_sten(H, 0);
  const int w = mg_rw(R), tw = mg_rw(T);
  for (int e = tid; e < mg_rn(R); e += MG_FINE_THREADS) {
    const int i = R.i0 + e / w, j = R.j0 + e % w;
    const size_t c = (size_t)i * nx + j;
    const double v = GATHER ? mg_gather0(A.part, i, j, A.ntb, A.band_lo, A.band_hi) : ((i >= A.clip_lo && i < A.clip_hi) ? H.rhs[c] : 0.0);      // (a staged, band-by-band gather out of LDS was built and measured: 167 us against 90)
    if (GATHER && mg_in(O, i, j)) H.rhs[c] = v;
    prhs[e] = v;
    const uint8_t in0 = H.inner0[c];      // 1: deep water (constants), 2: no fluid under the node (every entry 0, omega / d = 0: nothing else is loaded), 0: its own nine entries
    px1[e] = (in0 == 1 ? H.icwd : in0 == 2 ? 0.0 : H.wd[c]) * v;
  }
  __syncthreads();
  for (int e = tid; e < mg_rn(T); e += MG_FINE_THREADS) {
    const int i = T.i0 + e / tw, j = T.j0 + e % tw;
    const size_t c = (size_t)i * nx + j;
    const int pe = (i - R.i0) * w + (j - R.j0);
    const uint8_t in0 = H.inner0[c];
    if (in0 == 1) {      // deep water: the stencil is a constant (an interior node has all eight neighbours inside the grid)
      double t = 0.0;
#pragma unroll
      for (int k = 0; k < 9; ++k) t = t + H.ic[k] * px1[pe + (k / 3 - 1) * w + (k % 3 - 1)];
      prhs[pe] = prhs[pe] - t;
    } else if (in0 == 2) prhs[pe] = 0.0;      // (d == 0 below, without the loads)
    else {
      const double d = st[(size_t)4 * n + c];
      const double t = mg_apply_patch(st, n, c, i, j, ny, nx, px1, R);
      prhs[pe] = d != 0.0 ? prhs[pe] - t : 0.0;
    }
  }
  __syncthreads();
  const int ow = mg_rw(own);
  for (int e = tid; e < mg_rn(own); e += MG_FINE_THREADS) {
    const int I = own.i0 + e / ow, J = own.j0 + e % ow;
    double t = 0.0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const double wgt = mg_w1(I, 2 * I + dy, ny, cny) * mg_w1(J, 2 * J + dx, nx, cnx);
        if (wgt != 0.0) t = t + wgt * prhs[(2 * I + dy - R.i0) * w + (2 * J + dx - R.j0)];
      }
    H.rhs[H.off[1] + (size_t)I * cnx + J] = t;
  }
}

// k_mg_up0: level 0's result from level 1's (H.x), x_0 . rhs_0 into dot(z, r), the scalar epilogue, the gauge of cut-off regions (k_mg_up's last part, for level 0).
// A workgroup owns tile x tile nodes of level 0.
__global__ __launch_bounds__(MG_FINE_THREADS) void k_mg_up0(MgUpArgs A) {
  extern __shared__ double lds[];
  __shared__ double s_red[MG_FINE_THREADS / 64];
  __shared__ int s_last;
  const MgHier& H = A.H;
  const int tid = threadIdx.x;
  if (!A.force && pcg_idle(A.sc)) return;      // (as k_mg_up)
  const int n_null = (int)A.nullv[MG_NULL_MAX * 256];
  const int nx = H.nx[0], ny = H.ny[0], cnx = H.nx[1], cny = H.ny[1];
  const size_t n0n = (size_t)nx * ny;
  double gv[MG_NULL_MAX] = {0.0, 0.0, 0.0, 0.0};
  const int tiles_x = (nx + A.tile - 1) / A.tile;
  const int ti = A.tile_row0 + blockIdx.x / tiles_x, tj = blockIdx.x % tiles_x;
  MgRect X = {ti * A.tile, (ti + 1) * A.tile, tj * A.tile, (tj + 1) * A.tile};
  if (X.i1 > ny) X.i1 = ny;
  if (X.j1 > nx) X.j1 = nx;
  const MgRect X2 = mg_grow(X, ny, nx), Xc = mg_coarse_around(X2, cny, cnx);
  double* e_ = lds;                  // level 1's result on Xc
  double* b2 = lds + A.cap;          // x2 on X2
  const double* st = mg_sten(H, 0);
  const int w2 = mg_rw(X2), cw = mg_rw(Xc), w = mg_rw(X);
  for (int e = tid; e < mg_rn(Xc); e += MG_FINE_THREADS) e_[e] = H.x[H.off[1] + (size_t)(Xc.i0 + e / cw) * cnx + Xc.j0 + e % cw];
  __syncthreads();
  for (int e = tid; e < mg_rn(X2); e += MG_FINE_THREADS) {
    const int i = X2.i0 + e / w2, j = X2.j0 + e % w2;
    const size_t c = (size_t)i * nx + j;
    const uint8_t in0 = H.inner0[c];
    if (in0 == 2) { b2[e] = 0.0; continue; }      // (omega / d == 0 below, without the loads: the air above a tank, most of a dam break's grid)
    const double wdv = in0 == 1 ? H.icwd : H.wd[c], rv = H.rhs[c];
    const int I = i >> 1, J = j >> 1;
    const bool oy = (i & 1) && I + 1 <= cny - 1, ox = (j & 1) && J + 1 <= cnx - 1;
    const int I1 = oy ? I + 1 : I, J1 = ox ? J + 1 : J;
    const double fy = oy ? 0.5 : 0.0, fx = ox ? 0.5 : 0.0;
    const double lo = (1.0 - fx) * e_[(I - Xc.i0) * cw + (J - Xc.j0)] + fx * e_[(I - Xc.i0) * cw + (J1 - Xc.j0)];
    const double hi = (1.0 - fx) * e_[(I1 - Xc.i0) * cw + (J - Xc.j0)] + fx * e_[(I1 - Xc.i0) * cw + (J1 - Xc.j0)];
    b2[e] = wdv != 0.0 ? wdv * rv + ((1.0 - fy) * lo + fy * hi) : 0.0;
  }
  __syncthreads();
  double dv = 0.0;
  for (int e = tid; e < mg_rn(X); e += MG_FINE_THREADS) {
    const int i = X.i0 + e / w, j = X.j0 + e % w;
    const size_t c = (size_t)i * nx + j;
    const uint8_t in0 = H.inner0[c];
    const bool inner = in0 == 1, empty = in0 == 2;
    const double wdv = inner ? H.icwd : empty ? 0.0 : H.wd[c], rv = empty ? 0.0 : H.rhs[c];      // (an empty node's x_0 is 0 and adds 0 to x_0 . rhs_0)
    const int pe2 = (i - X2.i0) * w2 + (j - X2.j0);
    double t = 0.0;
    if (inner) {
#pragma unroll
      for (int k = 0; k < 9; ++k) t = t + H.ic[k] * b2[pe2 + (k / 3 - 1) * w2 + (k % 3 - 1)];
    } else if (!empty) t = mg_apply_patch(st, n0n, c, i, j, ny, nx, b2, X2);
    const double xv = wdv != 0.0 ? b2[pe2] + wdv * (rv - t) : 0.0;
    if (n_null > 0) {
      mg_st_agent(H.x + c, xv);
#pragma unroll
      for (int q = 0; q < MG_NULL_MAX; ++q) if (q < n_null && i >= A.row_lo && i < A.row_hi) gv[q] += A.m0[(size_t)q * n0n + c] * xv;
    } else H.x[c] = xv;
    if (i >= A.row_lo && i < A.row_hi) dv += xv * rv;
  }
  for (int q = 0; q < n_null && q < MG_NULL_MAX; ++q) {
    double g = q == 0 ? gv[0] : q == 1 ? gv[1] : q == 2 ? gv[2] : gv[3];
    g = eu_wave_sum(g);
    __syncthreads();
    if ((tid & 63) == 0) s_red[tid >> 6] = g;
    __syncthreads();
    if (tid == 0) {
      double t = 0.0;
      for (int k = 0; k < MG_FINE_THREADS / 64; ++k) t += s_red[k];
      mg_st_agent(A.dot_part + (size_t)(1 + q) * MG_DOT_BLOCKS + blockIdx.x, t);
    }
  }
  dv = eu_wave_sum(dv);
  __syncthreads();
  if ((tid & 63) == 0) s_red[tid >> 6] = dv;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every thread's x_0 stores have left before the ticket (see k_mg_up)
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int k = 0; k < MG_FINE_THREADS / 64; ++k) t += s_red[k];
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(&A.dot_part[blockIdx.x]), (unsigned long long)__double_as_longlong(t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    s_last = __hip_atomic_fetch_add(A.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  if (A.slot && tid < MG_NULL_MAX) A.slot[1 + tid] = 0.0;
  __syncthreads();
  for (int q = 0; q < n_null && q < MG_NULL_MAX; ++q) {      // the gauge: every workgroup's x_0 is in memory (agent-scope stores, drained before the tickets)
    double g = 0.0;
    for (unsigned int k = tid; k < gridDim.x; k += MG_FINE_THREADS) g += mg_ld_agent(A.dot_part + (size_t)(1 + q) * MG_DOT_BLOCKS + k);
    g = eu_wave_sum(g);
    __syncthreads();
    if ((tid & 63) == 0) s_red[tid >> 6] = g;
    __syncthreads();
    double tot = 0.0;
    for (int k = 0; k < MG_FINE_THREADS / 64; ++k) tot += s_red[k];
    const double mn = A.m0[(size_t)MG_NULL_MAX * n0n + q];
    if (A.slot) { if (tid == 0) A.slot[1 + q] = tot; }
    else if (mn > 0.0) {
      const double cq = tot / mn;
      for (size_t c = tid; c < n0n; c += MG_FINE_THREADS) {
        const double nv = A.n0[(size_t)q * A.nstride + c];
        if (nv != 0.0) mg_st_agent(H.x + c, mg_ld_agent(H.x + c) - nv * cq);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  double t = 0.0;
  for (unsigned int k = tid; k < gridDim.x; k += MG_FINE_THREADS)
    t += __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<unsigned long long*>(&A.dot_part[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  t = eu_wave_sum(t);
  __syncthreads();
  if ((tid & 63) == 0) s_red[tid >> 6] = t;
  __syncthreads();
  if (tid == 0) {
    double v = 0.0;
    for (int k = 0; k < MG_FINE_THREADS / 64; ++k) v += s_red[k];
    if (A.slot) { A.slot[0] = v; __hip_atomic_store(A.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return; }      // (split cycle: the ranks' shares are summed first)
    v = A.sc->sigma_new + v;      // k_precond_tile left dot(z_tile, r) there (FIN_STORE_ONLY)
    if (A.fin_op == FIN_SIGMA_INIT) A.sc->sigma = v;                                                       // main.c:748
    else if (A.fin_op == FIN_BETA) { A.sc->sigma_new = v; A.sc->beta = v / A.sc->sigma; A.sc->sigma = v; }   // main.c:762-765
    else A.sc->sigma_new = v;
    __hip_atomic_store(A.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ------------------------------------------------------------------------------------------ host side
static size_t mg_tail_lds(const euler_sim* S, int lB) {
  size_t d = 0;
  for (int l = lB; l < S->mg_levels; ++l) d += 2 * (size_t)S->mg_nx[l] * S->mg_ny[l];      // (the dense level: its right-hand side and result)
  const size_t ntop = (size_t)S->mg_nx[S->mg_levels - 1] * S->mg_ny[S->mg_levels - 1];
  return (d + ntop * ntop) * sizeof(double);
}
static int mg_set_lds(const void* fn, size_t bytes) {
  if (bytes > 48 * 1024) HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return EULER_OK;
}

static inline unsigned int* mg_tick_down(const euler_sim* S) { return reinterpret_cast<unsigned int*>(S->mg_dot + (1 + MG_NULL_MAX) * MG_DOT_BLOCKS + 1); }
static inline unsigned int* mg_tick_up(const euler_sim* S) { return reinterpret_cast<unsigned int*>(S->mg_dot + (1 + MG_NULL_MAX) * MG_DOT_BLOCKS); }
#ifndef MG_MIN_BLOCKS
#define MG_MIN_BLOCKS 64
#endif
MgDownArgs eu_mg_down_args(const euler_sim* S, const MgHier& H, int lA, int lB, int lC) {
  MgDownArgs A;
  A.H = H; A.lA = lA; A.lB = lB;
  const int steps = lB - lA;
  A.tile = steps == 3 ? 4 : steps == 2 ? 8 : steps == 1 ? 16 : 32;
  // a small level (grids up to 1024^2): the launch is latency, not work - smaller tiles until MG_MIN_BLOCKS workgroups share it (1024^2: 16 workgroups -> 64)
  while (steps > 0 && A.tile > 4 && (size_t)((S->mg_nx[lB] + A.tile - 1) / A.tile) * ((S->mg_ny[lB] + A.tile - 1) / A.tile) < MG_MIN_BLOCKS) A.tile /= 2;
  int e = A.tile, c[4] = {0, 0, 0, 0};
  c[steps] = e * e;
  for (int k = steps - 1; k >= 0; --k) { e = 2 * e + 3; c[k] = e * e; }
  A.cap0 = c[0] > c[2] ? c[0] : c[2]; A.cap1 = c[1] > c[3] ? c[1] : c[3];
  A.tail = lB == lC;
  A.part = S->mg_part; A.ntb = S->geom.T / 16; A.band_lo = S->band_lo; A.band_hi = S->band_hi;
  A.inv = S->cc_inv; A.ticket = mg_tick_down(S); A.sc = S->sc;
  A.tile_row0 = 0; A.clip_lo = 0; A.clip_hi = 0x7fffffff; A.force = 0;
  return A;
}
MgUpArgs eu_mg_up_args(const euler_sim* S, const MgHier& H, int lC, int fin_op, int force) {
  MgUpArgs U;
  U.H = H; U.lC = lC; U.l0 = 0; U.tile = 32; U.cap = 36 * 36;
  U.row_lo = 0; U.row_hi = S->mg_ny[0];
  U.sc = S->sc; U.fin_op = fin_op; U.force = force; U.dot_part = S->mg_dot; U.ticket = mg_tick_up(S);
  U.nullv = S->cc_null; U.n0 = S->mg_null0; U.m0 = S->mg_m0; U.nstride = S->mg_cells;
  U.tile_row0 = 0; U.slot = nullptr;
  return U;
}
// The launchers.  Each covers the rows [r0, r1) of its OUTPUT level l by the tile rows (edge `tile`) that hold them - the split cycle's launches; r1 < 0: the whole level.
// Returns the number of workgroups (0: nothing to launch), the first tile row in *row0
static unsigned mg_grid(const euler_sim* S, int l, int tile, int r0, int r1, int* row0) {
  *row0 = r1 < 0 ? 0 : r0 / tile;
  const int trows = (r1 < 0 ? (S->mg_ny[l] + tile - 1) / tile : (r1 + tile - 1) / tile) - *row0;
  return trows <= 0 ? 0u : (unsigned)(((S->mg_nx[l] + tile - 1) / tile) * trows);
}
int eu_mg_launch_down(euler_sim* S, MgDownArgs A, bool gather, int r0, int r1) {
  size_t lds = 2 * ((size_t)A.cap0 + A.cap1) * sizeof(double);
  if (A.tail) { const size_t t = mg_tail_lds(S, A.lB); if (t > lds) lds = t; }
  const unsigned nblk = mg_grid(S, A.lB, A.tile, r0, r1, &A.tile_row0);
  if (!nblk) return EULER_OK;
  if (gather) { int rc = mg_set_lds(reinterpret_cast<const void*>(&k_mg_down<true>), lds); if (rc) return rc; hipLaunchKernelGGL(k_mg_down<true>, dim3(nblk), dim3(MG_DOWN_THREADS), lds, S->stream, A); }
  else { int rc = mg_set_lds(reinterpret_cast<const void*>(&k_mg_down<false>), lds); if (rc) return rc; hipLaunchKernelGGL(k_mg_down<false>, dim3(nblk), dim3(MG_DOWN_THREADS), lds, S->stream, A); }
  return EULER_OK;
}
int eu_mg_launch_down1(euler_sim* S, MgDownArgs A, bool gather, int r0, int r1) {      // level 0 -> 1 on small workgroups
  const size_t lds = 2 * (size_t)A.cap0 * sizeof(double);
  const unsigned nblk = mg_grid(S, 1, A.tile, r0, r1, &A.tile_row0);
  if (!nblk) return EULER_OK;
  if (gather) hipLaunchKernelGGL(k_mg_down1<true>, dim3(nblk), dim3(MG_FINE_THREADS), lds, S->stream, A);
  else hipLaunchKernelGGL(k_mg_down1<false>, dim3(nblk), dim3(MG_FINE_THREADS), lds, S->stream, A);
  return EULER_OK;
}
int eu_mg_launch_up(euler_sim* S, MgUpArgs V, int r0, int r1) {
  const unsigned nblk = mg_grid(S, V.l0, V.tile, r0, r1, &V.tile_row0);
  if (nblk) hipLaunchKernelGGL(k_mg_up, dim3(nblk), dim3(MG_UP_THREADS), 3 * (size_t)V.cap * sizeof(double), S->stream, V);
  return EULER_OK;
}
int eu_mg_launch_up0(euler_sim* S, MgUpArgs U, int r0, int r1) {
  const unsigned nblk = mg_grid(S, 0, U.tile, r0, r1, &U.tile_row0);
  if (nblk) hipLaunchKernelGGL(k_mg_up0, dim3(nblk), dim3(MG_FINE_THREADS), 2 * (size_t)U.cap * sizeof(double), S->stream, U);
  return EULER_OK;
}

// the cycle: H.rhs[level 0] -> H.x[level 0]; `gather`: level 0's right-hand side comes from the tiles' partial sums (else it is in H.rhs already).
// Level 0 of more than MG_SMALL_LEVEL0 nodes: k_mg_down1, k_mg_down<false> x 1 .. 2 (the last one with the tail), k_mg_up for the levels between, k_mg_up0.  A small level 0
// (grids up to 1024^2): k_mg_down<gather> with the tail, then k_mg_up for what is left and the dot product.
static int launch_mg_cycle(euler_sim* S, int fin_op, int force, bool gather) {
  eu_prof_begin(S, KC_COARSE_CYCLE);      // ONE event pair around the whole cycle
  const MgHier H = mg_hier(S);
  const int lC = eu_mg_entry_level(S->mg_levels, S->mg_nx, S->mg_ny);
  if (eu_mg_check_tail(S, "")) return EULER_EINVAL;
  auto down_args = [&](int lA, int lB) { MgDownArgs A = eu_mg_down_args(S, H, lA, lB, lC); A.force = force; return A; };
  const MgUpArgs U = eu_mg_up_args(S, H, lC, fin_op, force);
  if (eu_mg_check_tiles0(S, "")) return EULER_EINVAL;
  const bool small = (size_t)S->mg_nx[0] * S->mg_ny[0] <= MG_SMALL_LEVEL0;
  // a small level 0 (grids up to 1024^2): the launches are the cost, not the nodes - ONE launch down (gather, every transition, its last workgroup the small levels), ONE back up
  // with the dot product (1024^2: 6 launches per iteration -> 4).  Else level 0 -> 1 on small workgroups first
  if (!small) { MgDownArgs A = down_args(0, 1); A.tail = 0; int rc = eu_mg_launch_down1(S, A, gather); if (rc) return rc; }
  int lA = small ? 0 : 1;
  do {      // three transitions per launch; the one that reaches lC goes on with the tail (lC == lA: the tail alone)
    const int lB = lA + 3 < lC ? lA + 3 : lC;
    int rc = eu_mg_launch_down(S, down_args(lA, lB), small && lA == 0 && gather);
    if (rc) return rc;
    lA = lB;
  } while (lA < lC);
  if (small) {
    MgUpArgs V = U;
    while (V.tile > 8 && (size_t)((S->mg_nx[0] + V.tile - 1) / V.tile) * ((S->mg_ny[0] + V.tile - 1) / V.tile) < MG_MIN_BLOCKS) V.tile /= 2;
    V.cap = (V.tile + 4) * (V.tile + 4);
    eu_mg_launch_up(S, V);
  } else {
    if (lC > 1) { MgUpArgs V = U; V.l0 = 1; eu_mg_launch_up(S, V); }      // back up to level 1
    eu_mg_launch_up0(S, U);
  }
  eu_prof_end(S, KC_COARSE_CYCLE);
  return EULER_OK;
}

int eu_mg_solve(euler_sim* S, int fin_op, int force) { return launch_mg_cycle(S, fin_op, force, !S->has_comm); }
