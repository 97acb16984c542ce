// k_envelope.hip — the run-long envelopes (include/euler.h, docs/envelope.md): per cell, when the water first arrived, how long the cell stayed wet, and the
// peaks of speed and pressure, gathered on the device at the end of every substep (run_stage, driver.hip: the tail of EULER_STAGE_PROJECT).
//
// A handle with channels on holds one plane of 32-bit words per channel.  Arrival, wet time and speed lie row-major like u and v; the pressure's peak lies in the
// band-skewed order of S->p (euler_dev.h skew_index - a function of the grid's size alone: nothing a caller sets moves an element), so that its update is one
// coalesced read-modify-write beside the read of p.  Only euler_envelope_get_field / _set_field and the raster un-skew it.
//   k_envelope_cells<VEC>   one workgroup per 64 x 64 tile, lanes along a grid row with VEC cells each (k_observe.h: 4 where X % 4 == 0, else 1).  A tile whose
//                           tile-map flag is clear is left at once: no marker, no fluid cell, nothing changes.  A lane none of whose cells is fluid loads no plane
//                           and stores nothing; u and v are loaded only with the speed channel on (the channel set is a kernel argument: uniform branches)
//   k_envelope_pressure     the walk of k_flow_pressure / k_gauges: lane l sits at row 64 band + l and takes pair-records of the skewed array, one 16-byte load of
//                           p and one 8-byte load and store of the plane per lane; a workgroup takes 64 pair-records of a band and leaves at once when the three
//                           tile columns they cross are dry.  Fluid is count != 0 && !solid read from the grids, as in k_gauges - not the solver's mask
//   k_envelope_raster       one workgroup per pixel (and, where a pixel's box is large, per slice of its rows): lanes walk the box, the waves fold by ob_wave,
//                           one lane per wave goes to LDS, and the workgroup issues ONE set of integer global atomics, skipping identities
// Every word is written by exactly one lane per launch and every record field is an integer sum or an extreme of bit patterns: no float is added across lanes, none
// goes through an atomic.  The update touches no validity flag; with the pressure channel on it first finishes the pending pressure (eu_pressure_current).
#include "k_observe.h"
#include "euler_host.h"

#include <stdlib.h>
#include <string.h>

int eu_pressure_current(euler_sim* S);      // k_grid.hip

#define EN_T 256            // threads per workgroup: four waves
#define EN_PAIRS 64         // pair-records of a band per workgroup of k_envelope_pressure
#define EN_WG_CELLS (1 << 15)   // cells a workgroup of the raster should walk before a pixel's rows are split
enum { EN_ARRIVAL = 0, EN_WET, EN_SPEED, EN_PRESSURE, EN_PLANES };
#define EN_NEVER 0xffffffffu

static_assert(sizeof(euler_envelope_px) == 32 && offsetof(euler_envelope_px, cells) == 0 && offsetof(euler_envelope_px, touched) == 4 && offsetof(euler_envelope_px, arrival_min) == 8 &&
              offsetof(euler_envelope_px, arrival_max) == 12 && offsetof(euler_envelope_px, wet_max) == 16 && offsetof(euler_envelope_px, speed2_max) == 20 &&
              offsetof(euler_envelope_px, p_max) == 24 && offsetof(euler_envelope_px, reserved) == 28, "k_envelope_raster addresses a record as eight 32-bit words");

struct EnCellArgs {
  const uint8_t *solid, *count;
  const float *u, *v;
  unsigned int *arrival, *wet, *speed;      // null: the channel is off
  ObTiles tiles;
  int X, Y, ntx;
  unsigned int t_end_bits;
  float dt;
};

template <int VEC>
__device__ __forceinline__ void en_load(unsigned int* d, const unsigned int* g, size_t i) {
  if constexpr (VEC == 4) {
    const uint4 t = *reinterpret_cast<const uint4*>(g + i);
    d[0] = t.x; d[1] = t.y; d[2] = t.z; d[3] = t.w;
  } else d[0] = g[i];
}
template <int VEC>
__device__ __forceinline__ void en_store(unsigned int* g, size_t i, const unsigned int* d) {
  if constexpr (VEC == 4) *reinterpret_cast<uint4*>(g + i) = make_uint4(d[0], d[1], d[2], d[3]);
  else g[i] = d[0];
}

template <int VEC>
__global__ __launch_bounds__(EN_T) void k_envelope_cells(const EnCellArgs a) {
  typedef ObRow<VEC, false, false> Row;
  const int tx = (int)(blockIdx.x % (unsigned int)a.ntx), ty = (int)(blockIdx.x / (unsigned int)a.ntx);
  if (!a.tiles.wet(tx, ty)) return;      // (the whole workgroup: no marker in the tile)
  constexpr int LPR = 64 / VEC, RPW = EN_T / LPR;      // lanes per tile row, rows per pass of the workgroup
  const int tid = threadIdx.x, x0 = tx * 64 + (tid % LPR) * VEC;
  if (x0 >= a.X) return;
  const size_t X = (size_t)a.X;
  for (int r = tid / LPR; r < 64; r += RPW) {
    const int y = ty * 64 + r;
    if (y < 1) continue;
    if (y > a.Y - 2) break;
    const size_t i = (size_t)y * X + (size_t)x0;
    const unsigned int so = Row::bytes(a.solid, i), cn = Row::bytes(a.count, i);
    bool fluid[VEC], any = false;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const int x = x0 + k;
      fluid[k] = x >= 1 && x <= a.X - 2 && ((cn >> (8 * k)) & 0xffu) != 0u && ((so >> (8 * k)) & 0xffu) == 0u;
      any |= fluid[k];
    }
    if (!any) continue;      // nothing of this lane's changes: no plane is loaded, nothing is stored
    unsigned int w[VEC];
    if (a.arrival) {
      en_load<VEC>(w, a.arrival, i);
      bool changed = false;
#pragma unroll
      for (int k = 0; k < VEC; ++k) if (fluid[k] && w[k] == EN_NEVER) { w[k] = a.t_end_bits; changed = true; }
      if (changed) en_store<VEC>(a.arrival, i, w);
    }
    if (a.wet) {
      en_load<VEC>(w, a.wet, i);
#pragma unroll
      for (int k = 0; k < VEC; ++k) if (fluid[k]) w[k] = __float_as_uint(__uint_as_float(w[k]) + a.dt);
      en_store<VEC>(a.wet, i, w);
    }
    if (a.speed) {
      Row row;
      Row::cells(row.vv, a.v, i);
      Row::cells(row.vd, a.v, i - X);
      Row::cells(row.uu + 1, a.u, i);
      row.uu[0] = a.u[i - 1];
      en_load<VEC>(w, a.speed, i);
      bool changed = false;
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        if (!fluid[k]) continue;
        const unsigned int before = w[k];
        ob_max_bits(w[k], row.speed2(k));
        changed |= w[k] != before;
      }
      if (changed) en_store<VEC>(a.speed, i, w);
    }
  }
}

struct EnPressArgs {
  const uint8_t *solid, *count;
  const double* p;
  unsigned int* peak;      // band-skewed like p
  SkewGeom g;
  ObTiles tiles;
  int nchunks;             // workgroups per band
};

__global__ __launch_bounds__(EN_T) void k_envelope_pressure(const EnPressArgs a) {
  const int band = (int)(blockIdx.x / (unsigned int)a.nchunks), t0 = (int)(blockIdx.x % (unsigned int)a.nchunks) * (2 * EN_PAIRS);
  // the cells of records [t0, t0 + 2 EN_PAIRS) lie in columns [t0 - 63, t0 + 2 EN_PAIRS - 1]: the tile columns they cross, clipped to the grid
  {
    const int xa = t0 - 63 > 0 ? t0 - 63 : 0, xb = t0 + 2 * EN_PAIRS - 1 < a.g.X - 1 ? t0 + 2 * EN_PAIRS - 1 : a.g.X - 1;
    bool wet = false;
    for (int tx = xa >> 6; tx <= (xb >> 6); ++tx) wet |= a.tiles.wet(tx, band);
    if (!wet) return;      // (the whole workgroup)
  }
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int y = band * 64 + lane;
  if (y < 1 || y > a.g.Y - 2) return;
  const size_t rowi = (size_t)y * (size_t)a.g.X;
  const size_t base = (size_t)band * a.g.TS * 64 + 2 * (size_t)lane;
  for (int pr = wave; pr < EN_PAIRS; pr += EN_T / 64) {
    const int t = t0 + 2 * pr, xa = t - lane;      // pair-record t holds the cells (xa, y), (xa + 1, y) in this lane
    bool f[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int x = xa + e;
      f[e] = x >= 1 && x <= a.g.X - 2;
      if (f[e]) f[e] = a.count[rowi + (size_t)x] != 0 && a.solid[rowi + (size_t)x] == 0;
    }
    if (!f[0] && !f[1]) continue;
    const size_t el = base + (size_t)t * 64;
    const double2 pp = *reinterpret_cast<const double2*>(a.p + el);
    uint2 w = *reinterpret_cast<const uint2*>(a.peak + el);
    const uint2 before = w;
    if (f[0]) { const float pf = (float)pp.x; ob_max_bits(w.x, pf > 0.f ? pf : 0.f); }
    if (f[1]) { const float pf = (float)pp.y; ob_max_bits(w.y, pf > 0.f ? pf : 0.f); }
    if (w.x != before.x || w.y != before.y) *reinterpret_cast<uint2*>(a.peak + el) = w;
  }
}

// the planes' update at the end of EULER_STAGE_PROJECT (run_stage tests S->env_channels first)
int eu_launch_envelope(euler_sim* S, float dt) {
  const uint32_t ch = S->env_channels;
  if (!ch) return EULER_OK;
  const float t_end = (float)(S->time + (double)dt);
  if (ch & EULER_ENV_PRESSURE) {      // the one thing an observer may do to the state (docs/gauges.md): the pending pressure finished and clamped in memory
    int rc = eu_pressure_current(S);
    if (rc) return rc;
  }
  if (ch & (EULER_ENV_ARRIVAL | EULER_ENV_WET | EULER_ENV_SPEED)) {
    EnCellArgs a;
    a.solid = S->solid; a.count = S->count; a.u = S->u; a.v = S->v;
    a.arrival = S->env_plane[EN_ARRIVAL]; a.wet = S->env_plane[EN_WET]; a.speed = S->env_plane[EN_SPEED];
    a.tiles = eu_observe_tiles(S);
    a.X = S->X; a.Y = S->Y; a.ntx = (S->X + 63) / 64;
    memcpy(&a.t_end_bits, &t_end, sizeof t_end);
    a.dt = dt;
    const dim3 grid((unsigned)a.ntx * (unsigned)((S->Y + 63) / 64));
    if (S->X % 4 == 0) LAUNCH(S, KC_MISC, k_envelope_cells<4>, grid, dim3(EN_T), a);
    else LAUNCH(S, KC_MISC, k_envelope_cells<1>, grid, dim3(EN_T), a);
  }
  if (ch & EULER_ENV_PRESSURE) {
    EnPressArgs a;
    a.solid = S->solid; a.count = S->count; a.p = S->p; a.peak = S->env_plane[EN_PRESSURE]; a.g = S->geom;
    a.tiles = eu_observe_tiles(S);
    a.nchunks = (S->X + 63 + 2 * EN_PAIRS - 1) / (2 * EN_PAIRS);      // a band's X + 63 live records
    LAUNCH(S, KC_MISC, k_envelope_pressure, dim3((unsigned)a.nchunks * (unsigned)S->geom.nbands), dim3(EN_T), a);
  }
  HIPCHK(hipGetLastError());
  S->env_substeps += 1;
  return EULER_OK;
}

// ------------------------------------------------------------------------------------------ the store
static size_t en_plane_words(const euler_sim* S, int k) { return k == EN_PRESSURE ? S->geom.S : S->C; }

static int en_init_plane(euler_sim* S, int k) {
  HIPCHK(hipMemsetAsync(S->env_plane[k], k == EN_ARRIVAL ? 0xff : 0, en_plane_words(S, k) * sizeof(unsigned int), S->stream));
  return EULER_OK;
}

// a null argument, a row-slab handle, nothing loaded: the refusals every call below makes first, in this order
static int en_enter(const euler_sim* S, const char* who, const void* arg) {
  if (!S || !arg) { eu_set_error("%s: null argument", who); return EULER_EINVAL; }
  if (S->slab_on) { eu_set_error("%s: not on a row-slab handle (the planes cover the whole grid)", who); return EULER_ESTATE; }
  if (!S->loaded) { eu_set_error("%s: no scenario loaded", who); return EULER_ESTATE; }
  return EULER_OK;
}

int eu_envelope_off(euler_sim* S) {
  bool any = false;
  for (int k = 0; k < EN_PLANES; ++k) any |= S->env_plane[k] != nullptr;
  if (any) HIPCHK(hipStreamSynchronize(S->stream));      // (a launch may still write them)
  for (int k = 0; k < EN_PLANES; ++k) {
    if (S->env_plane[k]) (void)eu_dev_free(S, S->env_plane[k]);
    S->env_plane[k] = nullptr;
  }
  S->env_channels = 0;
  S->env_substeps = 0;
  return EULER_OK;
}

extern "C" int euler_set_envelope(euler_sim* S, uint32_t channels) {
  const char* who = "euler_set_envelope";
  int rc = en_enter(S, who, S);
  if (rc) return rc;
  if (channels & ~(uint32_t)EULER_ENV_ALL) { eu_set_error("%s: channels 0x%x (bits of EULER_ENV_ALL = 0x%x)", who, channels, EULER_ENV_ALL); return EULER_EINVAL; }
  if (!channels) return eu_envelope_off(S);
  // the new planes first: a failure frees what this call allocated and leaves the handle as it was
  unsigned int* fresh[EN_PLANES] = {nullptr, nullptr, nullptr, nullptr};
  for (int k = 0; k < EN_PLANES; ++k) {
    if (!(channels & (1u << k)) || S->env_plane[k]) continue;
    if (eu_dalloc(S, &fresh[k], en_plane_words(S, k), EU_MEM_HANDLE, EU_DEV_QUIET)) {
      for (int j = 0; j < k; ++j) if (fresh[j]) (void)eu_dev_free(S, fresh[j]);
      eu_set_error("%s: %zu bytes of device memory for a plane", who, en_plane_words(S, k) * sizeof(unsigned int));
      return EULER_ENOMEM;
    }
  }
  HIPCHK(hipStreamSynchronize(S->stream));      // (a launch may still write a plane that goes)
  for (int k = 0; k < EN_PLANES; ++k) {
    if (fresh[k]) {
      S->env_plane[k] = fresh[k];
      if ((rc = en_init_plane(S, k))) return rc;
    } else if (!(channels & (1u << k)) && S->env_plane[k]) {
      (void)eu_dev_free(S, S->env_plane[k]);
      S->env_plane[k] = nullptr;
    }
  }
  if (!S->env_channels) S->env_substeps = 0;
  S->env_channels = channels;
  HIPCHK(hipStreamSynchronize(S->stream));
  return EULER_OK;
}

extern "C" int euler_get_envelope(euler_sim* S, uint32_t* channels, uint64_t* substeps) {
  int rc = en_enter(S, "euler_get_envelope", S);
  if (rc) return rc;
  if (channels) *channels = S->env_channels;
  if (substeps) *substeps = S->env_substeps;
  return EULER_OK;
}

extern "C" int euler_envelope_reset(euler_sim* S) {
  int rc = en_enter(S, "euler_envelope_reset", S);
  if (rc) return rc;
  for (int k = 0; k < EN_PLANES; ++k)
    if (S->env_plane[k] && (rc = en_init_plane(S, k))) return rc;
  S->env_substeps = 0;
  HIPCHK(hipStreamSynchronize(S->stream));
  return EULER_OK;
}

// the pressure's plane between the solver's order and the caller's row-major one
__global__ __launch_bounds__(256) void k_envelope_unskew(const unsigned int* __restrict__ skew, unsigned int* __restrict__ rowmajor, SkewGeom g) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (size_t)g.X * g.Y) rowmajor[i] = skew[skew_index(g, (int)(i % g.X), (int)(i / g.X))];
}
__global__ __launch_bounds__(256) void k_envelope_skew(const unsigned int* __restrict__ rowmajor, unsigned int* __restrict__ skew, SkewGeom g) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (size_t)g.X * g.Y) skew[skew_index(g, (int)(i % g.X), (int)(i / g.X))] = rowmajor[i];
}

// the checks of get_field / set_field behind en_enter: channel is exactly one enabled bit, bytes == 4 X Y
static int en_field_args(const euler_sim* S, const char* who, int32_t channel, size_t bytes) {
  const int k = eu_envelope_index(channel);
  if (k < 0 || !(S->env_channels & (uint32_t)channel)) { eu_set_error("%s: channel %d is not one enabled channel (enabled: 0x%x)", who, channel, S->env_channels); return -1; }
  if (bytes != S->C * sizeof(float)) { eu_set_error("%s: %zu bytes given, %zu expected", who, bytes, S->C * sizeof(float)); return -1; }
  return k;
}

namespace {
struct EnTmp {      // transfer scratch of the pressure plane's conversion: uncounted, freed on every way out
  euler_sim* S;
  unsigned int* p = nullptr;
  explicit EnTmp(euler_sim* s) : S(s) {}
  ~EnTmp() {
    if (!p) return;
    (void)hipStreamSynchronize(S->stream);
    (void)eu_dev_free(S, p);
  }
};
}

extern "C" int euler_envelope_get_field(euler_sim* S, int32_t channel, float* dst, size_t bytes) {
  const char* who = "euler_envelope_get_field";
  int rc = en_enter(S, who, dst);
  if (rc) return rc;
  const int k = en_field_args(S, who, channel, bytes);
  if (k < 0) return EULER_EINVAL;
  const unsigned int* src = S->env_plane[k];
  EnTmp tmp(S);
  if (k == EN_PRESSURE) {
    if ((rc = eu_dalloc(S, &tmp.p, S->C, EU_MEM_HANDLE, EU_MEM_UNCOUNTED))) return rc;
    hipLaunchKernelGGL(k_envelope_unskew, dim3(eu_blocks(S->C, 256)), dim3(256), 0, S->stream, src, tmp.p, S->geom);
    src = tmp.p;
  }
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, S->stream));
  HIPCHK(hipStreamSynchronize(S->stream));
  return EULER_OK;
}

extern "C" int euler_envelope_set_field(euler_sim* S, int32_t channel, const float* src, size_t bytes) {
  const char* who = "euler_envelope_set_field";
  int rc = en_enter(S, who, src);
  if (rc) return rc;
  const int k = en_field_args(S, who, channel, bytes);
  if (k < 0) return EULER_EINVAL;
  const size_t bad = eu_envelope_check_words(channel, (const uint32_t*)src, S->C);
  if (bad != (size_t)-1) {
    uint32_t w;
    memcpy(&w, src + bad, sizeof w);
    eu_set_error("%s: word %zu (0x%08x) of channel %d is not %sa finite float >= +0", who, bad, w, channel, channel == EULER_ENV_ARRIVAL ? "0xffffffff or " : "");
    return EULER_EINVAL;
  }
  EnTmp tmp(S);
  if (k == EN_PRESSURE) {
    if ((rc = eu_dalloc(S, &tmp.p, S->C, EU_MEM_HANDLE, EU_MEM_UNCOUNTED))) return rc;
    HIPCHK(hipMemcpyAsync(tmp.p, src, bytes, hipMemcpyHostToDevice, S->stream));
    hipLaunchKernelGGL(k_envelope_skew, dim3(eu_blocks(S->C, 256)), dim3(256), 0, S->stream, (const unsigned int*)tmp.p, S->env_plane[k], S->geom);
  } else HIPCHK(hipMemcpyAsync(S->env_plane[k], src, bytes, hipMemcpyHostToDevice, S->stream));
  HIPCHK(hipStreamSynchronize(S->stream));
  return EULER_OK;
}

// ------------------------------------------------------------------------------------------ the raster
struct EnRasArgs {
  const unsigned int *arrival, *wet, *speed, *peak;      // null: the channel is off and its fields keep their identities
  SkewGeom g;
  int W, H, nsplit;
  int bx0, by1, Bw, Bh;
  euler_envelope_px* out;
};

__global__ __launch_bounds__(256) void k_envelope_px_init(euler_envelope_px* out, unsigned int n) {
  const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  euler_envelope_px r;
  r.cells = r.touched = r.arrival_max = r.wet_max = r.speed2_max = r.p_max = r.reserved = 0u;
  r.arrival_min = EN_NEVER;
  out[i] = r;
}

// a lane's share: cells, touched (sums); arrival_min (min); arrival_max, wet_max, speed2_max, p_max (max) - the record's first seven words in their order
#define EN_NW 7
__device__ __forceinline__ int en_op(int k) { return k < 2 ? 0 : (k == 2 ? 1 : 2); }

__global__ __launch_bounds__(EN_T) void k_envelope_raster(const EnRasArgs a) {
  __shared__ unsigned int lw[EN_T / 64][EN_NW];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const unsigned int Xi = (unsigned int)a.Bw, Yi = (unsigned int)a.Bh;
  const unsigned int pix = blockIdx.x / (unsigned int)a.nsplit, sp = blockIdx.x % (unsigned int)a.nsplit;
  const int px = (int)(pix % (unsigned int)a.W), py = (int)(pix / (unsigned int)a.W);
  // the pixel's box of cells (the geometry of euler_overview_box) and this workgroup's slice of its rows
  const int xa = a.bx0 + (int)((unsigned long long)px * Xi / (unsigned int)a.W), xb = a.bx0 - 1 + (int)((unsigned long long)(px + 1) * Xi / (unsigned int)a.W);
  const int ytop = a.by1 - (int)((unsigned long long)py * Yi / (unsigned int)a.H), ybot = a.by1 + 1 - (int)((unsigned long long)(py + 1) * Yi / (unsigned int)a.H);
  const int nrows = ytop - ybot + 1;
  const int yhi = ytop - (int)((long long)sp * nrows / a.nsplit), ylo = ytop - (int)((long long)(sp + 1) * nrows / a.nsplit) + 1;
  const unsigned int ncols = (unsigned int)(xb - xa + 1), ncells = ncols * (unsigned int)(yhi - ylo + 1);
  unsigned int acc[EN_NW] = {0u, 0u, EN_NEVER, 0u, 0u, 0u, 0u};
  for (unsigned int c = (unsigned int)tid; c < ncells; c += EN_T) {
    const int x = xa + (int)(c % ncols), y = ylo + (int)(c / ncols);
    const size_t i = (size_t)y * (size_t)a.g.X + (size_t)x;
    acc[0] += 1u;
    if (a.arrival) {
      const unsigned int w = a.arrival[i];
      acc[2] = w < acc[2] ? w : acc[2];      // ("never" is the identity)
      if (w != EN_NEVER) { acc[1] += 1u; acc[3] = w > acc[3] ? w : acc[3]; }
    }
    if (a.wet) { const unsigned int w = a.wet[i]; acc[4] = w > acc[4] ? w : acc[4]; }
    if (a.speed) { const unsigned int w = a.speed[i]; acc[5] = w > acc[5] ? w : acc[5]; }
    if (a.peak) { const unsigned int w = a.peak[skew_index(a.g, x, y)]; acc[6] = w > acc[6] ? w : acc[6]; }
  }
#pragma unroll
  for (int k = 0; k < EN_NW; ++k) {
    const int op = en_op(k);
    acc[k] = op == 0 ? ob_wave<ObSum>(acc[k]) : (op == 1 ? ob_wave<ObMin>(acc[k]) : ob_wave<ObMax>(acc[k]));
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < EN_NW; ++k) lw[wave][k] = acc[k];
  }
  __syncthreads();
  if (tid < EN_NW) {      // one set of atomics per workgroup: thread k takes field k of the four waves
    const int op = en_op(tid);
    unsigned int r = lw[0][tid];
    for (int w = 1; w < EN_T / 64; ++w) {
      const unsigned int t = lw[w][tid];
      r = op == 0 ? r + t : (op == 1 ? (t < r ? t : r) : (t > r ? t : r));
    }
    unsigned int* o = reinterpret_cast<unsigned int*>(a.out + (size_t)py * a.W + px) + tid;
    if (op == 0) { if (r) atomicAdd(o, r); }
    else if (op == 1) { if (r != EN_NEVER) atomicMin(o, r); }
    else if (r) atomicMax(o, r);
  }
}

extern "C" int euler_envelope_raster(euler_sim* S, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t W, int32_t H, euler_envelope_px* out, size_t out_bytes) {
  const char* who = "euler_envelope_raster";
  int rc = eu_observe_enter(S, who, "the planes cover the whole grid", out, x0, y0, x1, y1);
  if (rc) return rc;
  const int Bw = x1 - x0 + 1, Bh = y1 - y0 + 1;
  if (W < 1 || H < 1 || W > Bw || H > Bh) { eu_set_error("%s: a raster of %d x %d for a box of %d x %d cells", who, W, H, Bw, Bh); return EULER_EINVAL; }
  const size_t n = (size_t)W * (size_t)H;
  if (out_bytes != n * sizeof(euler_envelope_px)) { eu_set_error("%s: %zu bytes given, %zu expected", who, out_bytes, n * sizeof(euler_envelope_px)); return EULER_EINVAL; }
  if ((rc = eu_devbuf_reserve(S, who, "the records", &S->env_ras_buf, out_bytes))) return rc;
  EnRasArgs a;
  a.arrival = S->env_plane[EN_ARRIVAL]; a.wet = S->env_plane[EN_WET]; a.speed = S->env_plane[EN_SPEED]; a.peak = S->env_plane[EN_PRESSURE];
  a.g = S->geom; a.W = W; a.H = H; a.bx0 = x0; a.by1 = y1; a.Bw = Bw; a.Bh = Bh;
  a.out = (euler_envelope_px*)S->env_ras_buf.p;
  const long long cols_max = (Bw + W - 1) / W, rows_max = (Bh + H - 1) / H, rows_min = Bh / H;
  long long ns = (cols_max * rows_max + EN_WG_CELLS - 1) / EN_WG_CELLS;      // slices of a pixel's rows
  a.nsplit = (int)(ns < 1 ? 1 : (ns > rows_min ? rows_min : ns));
  LAUNCH(S, KC_MISC, k_envelope_px_init, dim3(eu_blocks(n, 256)), dim3(256), a.out, (unsigned int)n);      // (W H <= the interior's cells < 2^30)
  LAUNCH(S, KC_MISC, k_envelope_raster, dim3((unsigned)(n * (size_t)a.nsplit)), dim3(EN_T), a);
  HIPCHK(hipGetLastError());
  return eu_observe_readback(S, out, &S->env_ras_buf, out_bytes);
}
