// k_gauges.hip — euler_gauges (include/euler.h, docs/gauges.md): a LIST of small instruments - wave gauges, pressure sensors, the load on a wall, the
// discharge through a section - evaluated on the device in one launch and one read-back.  The four older passes reduce one large box; this one reduces up
// to 1024 small, unrelated boxes of four kinds.
//
// The host checks the list and cuts every box along the 64 x 64 tile grid into chunks (eu_gauge_chunks, euler_host.c): a chunk lies in one tile, hence in one
// band of the skewed arrays and under one flag of the tile map.  The initial records (lo_* = 0xffffffff, the rest 0) and the chunk table go up in ONE copy;
// one workgroup takes one chunk, so the kind test is uniform across it.
//   LEVEL, FLUX      lanes lie along a grid row, waves take rows: the masks and the faces u[i], v[i] are read in the grid's order
//   PRESSURE, FORCE  the walk of k_flow_pressure: lane l sits at row 64 band + l and reads contiguous pair-records of the band-skewed pressure over the
//                    chunk's columns, waves take every fourth pair-record; rowmajor_tmp is never touched: a gauge costs the cells of its box, not the grid
// A lane sums in registers, the waves fold by ob_wave, one lane per wave goes to an LDS record, and the workgroup issues ONE set of integer global atomics
// (64-bit add, unsigned add / min / max, no value returned) into the gauge's record.  No float is ever added across lanes and none goes through an atomic:
// every field is an integer sum, an integer extreme or a maximum of bit patterns, so a record is the same whatever the order of chunks, waves and lanes.
// With the tile map a chunk in a dry tile counts its cells and leaves (FLUX: unless the tile right of it or above it is wet - its last column and top row
// hold faces those tiles' water makes live).
//
// The pass only reads the state and touches none of the handle's validity flags (with a PRESSURE or FORCE gauge the pending pressure is finished first, as
// euler_get_field does).
#include "k_observe.h"
#include "euler_host.h"

#include <stdlib.h>
#include <string.h>

int eu_pressure_current(euler_sim* S);      // k_grid.hip

#define GA_T 256          // threads per workgroup: four waves
#define GA_MAX_WG 32768   // workgroups of a launch; beyond, a workgroup takes several chunks in turn

static_assert(sizeof(euler_gauge) == 24 && sizeof(eu_gauge_chunk) == 24, "euler_gauge and a chunk are six 32-bit words");
static_assert(sizeof(euler_gauge_rec) == 72, "euler_gauge_rec is 72 bytes without padding");
static_assert(offsetof(euler_gauge_rec, cells) == 0 && offsetof(euler_gauge_rec, fluid) == 4 && offsetof(euler_gauge_rec, lo_x) == 8 && offsetof(euler_gauge_rec, hi_x) == 12 &&
              offsetof(euler_gauge_rec, lo_y) == 16 && offsetof(euler_gauge_rec, hi_y) == 20 && offsetof(euler_gauge_rec, terms) == 24 && offsetof(euler_gauge_rec, nonfinite) == 28 &&
              offsetof(euler_gauge_rec, a_pos) == 32 && offsetof(euler_gauge_rec, a_neg) == 40 && offsetof(euler_gauge_rec, b_pos) == 48 && offsetof(euler_gauge_rec, b_neg) == 56 &&
              offsetof(euler_gauge_rec, max_a) == 64 && offsetof(euler_gauge_rec, max_b) == 68, "k_gauges addresses a record as 32-bit words and the four sums behind a_pos as one array");

struct GaArgs {
  const uint8_t *solid, *count;
  const float *u, *v;
  const double* p;
  SkewGeom g;
  ObTiles tiles;
  const eu_gauge_chunk* chunks;
  unsigned int nchunks;
  euler_gauge_rec* out;
};

// a lane's share of a chunk.  w[]: fluid, lo_x, hi_x, lo_y, hi_y, terms, nonfinite, max_a bits, max_b bits; s[]: a_pos, a_neg, b_pos, b_neg
#define GA_NW 9
struct GaAcc {
  unsigned int w[GA_NW];
  unsigned long long s[4];
};
enum { GA_FLUID = 0, GA_LOX, GA_HIX, GA_LOY, GA_HIY, GA_TERMS, GA_BAD, GA_MAXA, GA_MAXB };
// how field k folds (0 add, 1 min, 2 max) and the 32-bit word of the record it goes to
__device__ __forceinline__ int ga_op(int k) { return k == GA_LOX || k == GA_LOY ? 1 : (k == GA_FLUID || k == GA_TERMS || k == GA_BAD ? 0 : 2); }
__device__ __forceinline__ int ga_word(int k) { return k < GA_MAXA ? k + 1 : 16 + (k - GA_MAXA); }

__device__ __forceinline__ void ga_clear(GaAcc& a) {
#pragma unroll
  for (int k = 0; k < GA_NW; ++k) a.w[k] = 0u;
  a.w[GA_LOX] = a.w[GA_LOY] = 0xffffffffu;
#pragma unroll
  for (int f = 0; f < 4; ++f) a.s[f] = 0ull;
}
__device__ __forceinline__ void ga_fluid(GaAcc& a, int x, int y) {
  const unsigned int ux = (unsigned int)x, uy = (unsigned int)y;
  a.w[GA_FLUID] += 1u;
  a.w[GA_LOX] = ux < a.w[GA_LOX] ? ux : a.w[GA_LOX]; a.w[GA_HIX] = ux > a.w[GA_HIX] ? ux : a.w[GA_HIX];
  a.w[GA_LOY] = uy < a.w[GA_LOY] ? uy : a.w[GA_LOY]; a.w[GA_HIY] = uy > a.w[GA_HIY] ? uy : a.w[GA_HIY];
}

// qv, qp of include/euler.h (euler_flow_px)
__device__ __forceinline__ unsigned long long ga_qv(float a) { return (unsigned long long)((a < 4096.f ? a : 4096.f) * 1048576.f); }
__device__ __forceinline__ unsigned long long ga_qp(float a) { return (unsigned long long)((a > 0.f ? (a < 16777216.f ? a : 16777216.f) : 0.f) * 256.f); }
// a face velocity that is live: counted, summed on the side of its sign (-0.f: the positive one) and into the maximum of |a|; a NaN only reports itself
__device__ __forceinline__ bool ga_face(GaAcc& acc, int pos, int mx, float a) {
  acc.w[GA_TERMS] += 1u;
  if (a != a) return true;
  if (a >= 0.f) acc.s[pos] += ga_qv(a);
  else acc.s[pos + 1] += ga_qv(-a);
  ob_max_bits(acc.w[mx], fabsf(a));
  return false;
}

// LEVEL, FLUX: lanes along a grid row, waves take rows
__device__ __forceinline__ void ga_walk_rows(const GaArgs& a, const eu_gauge_chunk& c, int wave, int lane, GaAcc& acc) {
  typedef ObRow<1, false, false> Row;
  const size_t X = (size_t)a.g.X;
  const int x = c.x0 + lane;
  if (x > c.x1) return;
  for (int y = c.y0 + wave; y <= c.y1; y += GA_T / 64) {
    const size_t i = (size_t)y * X + (size_t)x;
    const unsigned int so = Row::bytes(a.solid, i), cn = Row::bytes(a.count, i);
    if (cn && !so) ga_fluid(acc, x, y);
    if (c.kind != EULER_GAUGE_FLUX) continue;
    // the faces right of the cell and above it, live as k_advect_velocity tests them (i + 1 <= X - 1 and row y + 1 <= Y - 1 lie inside the grid)
    bool bad = false;
    if ((cn | Row::bytes(a.count, i + 1)) && !(so | Row::bytes(a.solid, i + 1))) {
      float t;
      Row::cells(&t, a.u, i);
      bad |= ga_face(acc, 0, GA_MAXA, t);
    }
    if ((cn | Row::bytes(a.count, i + X)) && !(so | Row::bytes(a.solid, i + X))) {
      float t;
      Row::cells(&t, a.v, i);
      bad |= ga_face(acc, 2, GA_MAXB, t);
    }
    acc.w[GA_BAD] += bad ? 1u : 0u;
  }
}

// PRESSURE, FORCE: the band-skewed array in its own order (euler_dev.h skew_index).  Lane l holds the cells (t - l, 64 band + l), (t + 1 - l, 64 band + l) of
// pair-record t; every cell of the chunk is in exactly one (lane, pair-record)
__device__ __forceinline__ void ga_walk_skewed(const GaArgs& a, const eu_gauge_chunk& c, int wave, int lane, GaAcc& acc) {
  const size_t X = (size_t)a.g.X;
  const int band = c.y0 >> 6, y = band * 64 + lane;
  if (y < c.y0 || y > c.y1) return;
  const int tbase = (c.x0 + (c.y0 & 63)) & ~1, tend = c.x1 + (c.y1 & 63);      // the pair-records that hold a cell of the chunk in SOME lane
  const double* base = a.p + (size_t)band * a.g.TS * 64 + 2 * lane;
  const size_t rowi = (size_t)y * X;
  for (int t = tbase + 2 * wave; t <= tend; t += 2 * (GA_T / 64)) {
    const int xa = t - lane;
    if (xa + 1 < c.x0 || xa > c.x1) continue;      // not in this lane
    const double2 pp = *reinterpret_cast<const double2*>(base + (size_t)t * 64);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int x = xa + e;
      if (x < c.x0 || x > c.x1) continue;
      const size_t i = rowi + (size_t)x;
      if (!a.count[i] || a.solid[i]) continue;
      ga_fluid(acc, x, y);
      const float pf = (float)(e ? pp.y : pp.x);
      if (c.kind == EULER_GAUGE_PRESSURE) {
        acc.w[GA_TERMS] += 1u;
        if (pf == pf) {
          acc.s[0] += ga_qp(pf);
          ob_max_bits(acc.w[GA_MAXA], pf > 0.f ? pf : 0.f);
        } else acc.w[GA_BAD] += 1u;
      } else {      // the solid cells this fluid cell touches (a box lies in the interior: its neighbours lie in the grid)
        const bool fr = a.solid[i + 1] != 0, fl = a.solid[i - 1] != 0, ft = a.solid[i + X] != 0, fb = a.solid[i - X] != 0;
        const unsigned int faces = (unsigned int)fr + (unsigned int)fl + (unsigned int)ft + (unsigned int)fb;
        if (!faces) continue;
        acc.w[GA_TERMS] += faces;
        if (pf != pf) { acc.w[GA_BAD] += 1u; continue; }
        const unsigned long long q = ga_qp(pf);
        const float pm = pf > 0.f ? pf : 0.f;
        if (fr) acc.s[0] += q;
        if (fl) acc.s[1] += q;
        if (ft) acc.s[2] += q;
        if (fb) acc.s[3] += q;
        if (fr || fl) ob_max_bits(acc.w[GA_MAXA], pm);
        if (ft || fb) ob_max_bits(acc.w[GA_MAXB], pm);
      }
    }
  }
}

__global__ __launch_bounds__(GA_T) void k_gauges(const GaArgs a) {
  __shared__ unsigned int lw[GA_T / 64][GA_NW];
  __shared__ unsigned long long ls[GA_T / 64][4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (unsigned int ci = blockIdx.x; ci < a.nchunks; ci += gridDim.x) {      // (the chunk, and every test on it, is uniform across the workgroup)
    const eu_gauge_chunk c = a.chunks[ci];
    unsigned int* ow = reinterpret_cast<unsigned int*>(a.out + c.gauge);
    if (tid == GA_T - 1) atomicAdd(ow, (unsigned int)(c.x1 - c.x0 + 1) * (unsigned int)(c.y1 - c.y0 + 1));      // cells: also of a dry tile
    const int tx = c.x0 >> 6, ty = c.y0 >> 6;
    bool wet = a.tiles.wet(tx, ty);
    if (!wet && c.kind == EULER_GAUGE_FLUX)      // a face in the tile's last column or top row is live by the water of the tile beyond it
      wet = (((c.x1 + 1) >> 6) != tx && a.tiles.wet(tx + 1, ty)) || (((c.y1 + 1) >> 6) != ty && a.tiles.wet(tx, ty + 1));
    if (!wet) continue;      // no marker in the tile: no fluid cell, no term
    GaAcc acc;
    ga_clear(acc);
    if (c.kind == EULER_GAUGE_LEVEL || c.kind == EULER_GAUGE_FLUX) ga_walk_rows(a, c, wave, lane, acc);
    else ga_walk_skewed(a, c, wave, lane, acc);
    // the wave folds; one lane goes to LDS
#pragma unroll
    for (int k = 0; k < GA_NW; ++k) {
      const int op = ga_op(k);
      acc.w[k] = op == 0 ? ob_wave<ObSum>(acc.w[k]) : (op == 1 ? ob_wave<ObMin>(acc.w[k]) : ob_wave<ObMax>(acc.w[k]));
    }
#pragma unroll
    for (int f = 0; f < 4; ++f) acc.s[f] = ob_wave<ObSum>(acc.s[f]);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < GA_NW; ++k) lw[wave][k] = acc.w[k];
#pragma unroll
      for (int f = 0; f < 4; ++f) ls[wave][f] = acc.s[f];
    }
    __syncthreads();
    // one set of atomics per workgroup: thread k takes field k of the four waves
    if (tid < GA_NW) {
      const int op = ga_op(tid);
      unsigned int r = lw[0][tid];
      for (int w = 1; w < GA_T / 64; ++w) {
        const unsigned int t = lw[w][tid];
        r = op == 0 ? r + t : (op == 1 ? (t < r ? t : r) : (t > r ? t : r));
      }
      unsigned int* o = ow + ga_word(tid);
      if (op == 0) { if (r) atomicAdd(o, r); }
      else if (op == 1) { if (r != 0xffffffffu) atomicMin(o, r); }
      else if (r) atomicMax(o, r);
    } else if (tid < GA_NW + 4) {
      const int f = tid - GA_NW;
      unsigned long long r = 0ull;
      for (int w = 0; w < GA_T / 64; ++w) r += ls[w][f];
      if (r) atomicAdd(reinterpret_cast<unsigned long long*>(ow + 8) + f, r);
    }
    __syncthreads();      // (the LDS records are the next chunk's)
  }
}

namespace {
struct GaStage {      // the host's copy of what goes up: freed on every way out, behind the copy that may still read it
  void* p = nullptr;
  hipStream_t busy = nullptr;
  bool in_flight = false;
  ~GaStage() {
    if (in_flight) (void)hipStreamSynchronize(busy);
    free(p);
  }
};
}

extern "C" int euler_gauges(euler_sim* S, const euler_gauge* g, int32_t n, euler_gauge_rec* out, size_t out_bytes) {
  const char* who = "euler_gauges";
  int rc = eu_observe_enter(S, who, nullptr, g ? (const void*)out : nullptr, 1, 1, 1, 1);
  if (rc) return rc;
  if (n < 1 || n > EULER_GAUGES_MAX) { eu_set_error("%s: %d gauges (1 ... %d)", who, n, EULER_GAUGES_MAX); return EULER_EINVAL; }
  const size_t rec_bytes = (size_t)n * sizeof(euler_gauge_rec);
  if (out_bytes != rec_bytes) { eu_set_error("%s: %zu bytes given, %zu expected", who, out_bytes, rec_bytes); return EULER_EINVAL; }
  const char* what = "";
  const int bad = eu_gauge_check(g, n, S->X, S->Y, &what);
  if (bad >= 0) {
    eu_set_error("%s: gauge %d (kind %d, box [%d, %d] x [%d, %d], reserved %d): %s [1, %d] x [1, %d]", who, bad, g[bad].kind, g[bad].x0, g[bad].x1, g[bad].y0, g[bad].y1, g[bad].reserved, what, S->X - 2, S->Y - 2);
    return EULER_EINVAL;
  }
  // (row slabs: chunks are cut along the tile grid and a slab is whole 64-row bands, so every chunk has one owner; this rank's table holds its own only)
  const int band_lo = S->slab_on ? S->band_lo : 0, band_hi = S->slab_on ? S->band_hi : INT32_MAX;
  const size_t nchunks = eu_gauge_chunks_bands(g, n, band_lo, band_hi, nullptr);
  if (nchunks > 0xffffffffull) { eu_set_error("%s: %zu chunks", who, nchunks); return EULER_EINVAL; }
  const size_t bytes = rec_bytes + nchunks * sizeof(eu_gauge_chunk);      // the records first (72 n bytes: the chunk table stays 8-byte aligned)
  GaStage st;
  if (!(st.p = malloc(bytes))) { eu_set_error("%s: %zu bytes of host memory for the chunk table", who, bytes); return EULER_ENOMEM; }
  euler_gauge_rec* init = (euler_gauge_rec*)st.p;
  memset(init, 0, rec_bytes);
  bool pressure = false, faces = false;
  for (int k = 0; k < n; ++k) {
    init[k].lo_x = init[k].lo_y = 0xffffffffu;
    pressure |= g[k].kind == EULER_GAUGE_PRESSURE || g[k].kind == EULER_GAUGE_FORCE;
    faces |= g[k].kind == EULER_GAUGE_FLUX;      // (FORCE looks across a row edge too, at the solid grid: the load's, never stale)
  }
  eu_gauge_chunks_bands(g, n, band_lo, band_hi, (eu_gauge_chunk*)((char*)st.p + rec_bytes));
  rc = eu_devbuf_reserve(S, who, "the records and the chunk table", &S->gauge_buf, bytes);
  if (!rc && pressure) rc = eu_pressure_current(S);      // (k_velocity_update_para leaves the last fmadds and the clamp to whoever looks)
  eu_slab_plan plan;
  if (S->slab_on) {      // collective: every rank's n records of its own chunks (the initial records where it has none), gathered and folded by add / min / max
    if (eu_slab_plan_flat(&plan, S->cfg.slab_nranks, n)) { eu_set_error("%s: %d ranks", who, S->cfg.slab_nranks); return EULER_EINVAL; }
    rc = eu_observe_slab_open(S, who, rc, (size_t)plan.total * sizeof(euler_gauge_rec), faces ? EU_OBS_ROWS_GAUGES : EU_OBS_ROWS_NONE);
  }
  if (rc) return rc;
  st.busy = S->stream; st.in_flight = true;
  HIPCHK(hipMemcpyAsync(S->gauge_buf.p, st.p, bytes, hipMemcpyHostToDevice, S->stream));
  GaArgs a;
  a.solid = S->solid; a.count = S->count; a.u = S->u; a.v = S->v; a.p = S->p; a.g = S->geom;
  a.tiles = eu_observe_tiles(S);
  a.out = (euler_gauge_rec*)S->gauge_buf.p;
  a.chunks = (const eu_gauge_chunk*)((const char*)S->gauge_buf.p + rec_bytes);
  a.nchunks = (unsigned int)nchunks;
  if (nchunks) LAUNCH(S, KC_MISC, k_gauges, dim3((unsigned)(nchunks < GA_MAX_WG ? nchunks : GA_MAX_WG)), dim3(GA_T), a);      // (a slab that owns no chunk launches nothing)
  HIPCHK(hipGetLastError());
  if (S->slab_on) {
    HIPCHK(hipMemcpyAsync(eu_observe_slab_mine(S, &plan, EU_OBS_REC_GAUGE), S->gauge_buf.p, rec_bytes, hipMemcpyDeviceToDevice, S->stream));
    if ((rc = eu_observe_slab_fold(S, &plan, EU_OBS_REC_GAUGE, S->gauge_buf.p))) return rc;
  }
  return eu_observe_readback(S, out, &S->gauge_buf, rec_bytes);      // (waits for the stream: the host's copy is free to go)
}
