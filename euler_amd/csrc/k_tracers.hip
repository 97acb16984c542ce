// k_tracers.hip — passive tracers (include/euler.h, docs/tracers.md): a store of 32-byte records on the device that moves with the flow by the marker's
// own rule, one extra launch in front of the marker launches of EULER_STAGE_ADVECT_MARKERS, and the raster that counts the records per pixel of an
// overview box.
//
// A tracer is an ARRAY OF ONE MARKER: advect_one<false, RK2> (k_advect_one.h) with the stage's full dt for both time arguments.  It never sees the dt the
// chain of the fluid's markers shortened and never shortens anyone's; it reads the row-major u, v, count, solid and sink as they stand in front of the
// marker launches - no column-major copy, no tile map - and touches none of the handle's validity flags.
#include "euler_dev.h"
#include "k_transport.h"
#include "k_advect_one.h"

#include <stdlib.h>
#include <string.h>

#define TR_T 256                 // threads per workgroup, one record per lane
#define TR_MIN_RECORDS 256u      // the store's first allocation; it doubles from there

// a record as its two 16-byte halves: {x, y, path, age} and {wet_time, substeps, flags, reserved}
struct TrLo { float x, y, path, age; };
struct TrHi { float wet_time; uint32_t substeps, flags, reserved; };
static_assert(sizeof(euler_tracer) == 32 && sizeof(TrLo) == 16 && sizeof(TrHi) == 16, "euler_tracer is two 16-byte halves");

// One lane, one record, one chain: position -> cell -> mask bytes -> the walk's gathers -> store.  Lane l of a wave loads bytes [32 l, 32 l + 16) and
// [32 l + 16, 32 l + 32): the two instructions together move the wave's 2 KB whole.  A wave whose records are all retired (or lie behind n) leaves after
// its load; in a live wave only the lanes whose record changed store.
template <bool RK2>
__global__ __launch_bounds__(TR_T) void k_advect_tracers(euler_tracer* __restrict__ rec, unsigned int n, const float* __restrict__ u, const float* __restrict__ v,
                                                         const uint8_t* __restrict__ solid, const uint8_t* __restrict__ sink, GridRef g, float dt) {
  const unsigned int i = blockIdx.x * TR_T + threadIdx.x;
  float4 lo = make_float4(0.f, 0.f, 0.f, 0.f);
  uint4 hi = make_uint4(0u, 0u, EULER_TRACER_RETIRED, 0u);      // (a lane behind n: retired, never stored)
  float4* p = reinterpret_cast<float4*>(rec + i);
  if (i < n) { lo = p[0]; hi = *reinterpret_cast<const uint4*>(p + 1); }
  const bool live = (hi.z & EULER_TRACER_RETIRED) == 0u;
  if (!__any(live)) return;
  if (!live) return;      // (no cross-lane operation below)
  const float x = lo.x, y = lo.y;
  // the cell (floorf(x), floorf(y)) lies in the grid exactly when 0 <= x < X and 0 <= y < Y; a NaN fails, an infinity too: decided before any grid read
  if (!(x >= 0.f && x < (float)g.X && y >= 0.f && y < (float)g.Y)) {
    hi.z |= EULER_TRACER_RETIRED | EULER_TRACER_LOST;
  } else {
    const size_t c = (size_t)(int)floorf(y) * g.X + (size_t)(int)floorf(x);
    const uint8_t so = solid[c], si = sink[c], cn = g.count[c];
    if (so) hi.z |= EULER_TRACER_RETIRED | EULER_TRACER_IN_SOLID;
    else if (si) hi.z |= EULER_TRACER_RETIRED | EULER_TRACER_IN_SINK;
    else {
      const bool wet = cn != 0;
      const AdvectOut o = advect_one<false, RK2>(g, u, v, solid, x, y, dt, dt);
      const float dx = o.px - x, dy = o.py - y;
      lo.z = lo.z + sqrtf(dx * dx + dy * dy);      // (correctly rounded under this build's flags: docs/tracers.md)
      lo.w = lo.w + dt;
      if (wet) hi.x = __float_as_uint(__uint_as_float(hi.x) + dt);
      hi.y += 1u;
      hi.z = wet ? (hi.z | EULER_TRACER_WET) : ((hi.z & ~(uint32_t)EULER_TRACER_WET) | EULER_TRACER_WAS_DRY);
      lo.x = o.px; lo.y = o.py;
      p[0] = lo;
    }
  }
  *reinterpret_cast<uint4*>(p + 1) = hi;
}

int eu_launch_advect_tracers(euler_sim* S, float dt) {
  const unsigned int n = (unsigned int)S->n_tracers;      // (<= EULER_TRACERS_MAX = 2^22)
  if (!n) return EULER_OK;
  const GridRef g = eu_grid_ref(S);
  euler_tracer* rec = (euler_tracer*)S->tracer_buf.p;
  eu_flag(S->opt[EULER_OPT_ADVECT_RK2] != 0, [&](auto R) {
    LAUNCH(S, KC_MARKER_ADVECT, k_advect_tracers<decltype(R)::value>, dim3(eu_blocks(n, TR_T)), dim3(TR_T), rec, n, S->u, S->v, S->solid, S->sink, g, dt);
  });
  return EULER_OK;
}

// ------------------------------------------------------------------------------------------ the store
// room for `need` records: the capacity doubles (from TR_MIN_RECORDS, up to EULER_TRACERS_MAX) and the records move over bit for bit; a failure leaves the handle as it was
static int tr_reserve(euler_sim* S, size_t need) {
  const size_t cap = S->tracer_buf.bytes / sizeof(euler_tracer);
  if (need <= cap) return EULER_OK;
  size_t ncap = cap ? 2 * cap : TR_MIN_RECORDS;
  while (ncap < need) ncap *= 2;
  if (ncap > EULER_TRACERS_MAX) ncap = EULER_TRACERS_MAX;
  return eu_devbuf_reserve(S, "euler_tracers_add", "the tracers", &S->tracer_buf, ncap * sizeof(euler_tracer), S->n_tracers * sizeof(euler_tracer));
}

extern "C" int euler_tracers_add(euler_sim* S, const float* xy, size_t n) {
  const char* who = "euler_tracers_add";
  if (!S) { eu_set_error("%s: null argument", who); return EULER_EINVAL; }
  if (S->slab_on) { eu_set_error("%s: not on a row-slab handle (a slab holds the rows of its own bands only)", who); return EULER_ESTATE; }
  if (!S->loaded) { eu_set_error("%s: no scenario loaded", who); return EULER_ESTATE; }
  char why[160];
  if (eu_tracers_check(xy, n, S->n_tracers, S->X, S->Y, why, sizeof why)) { eu_set_error("%s: %s", who, why); return EULER_EINVAL; }
  if (!n) return EULER_OK;
  euler_tracer* host = (euler_tracer*)calloc(n, sizeof(euler_tracer));      // all other words 0
  if (!host) { eu_set_error("%s: %zu bytes of host memory", who, n * sizeof(euler_tracer)); return EULER_ENOMEM; }
  for (size_t k = 0; k < n; ++k) { host[k].x = xy[2 * k]; host[k].y = xy[2 * k + 1]; }
  int rc = tr_reserve(S, S->n_tracers + n);
  if (!rc) {
    hipError_t e = hipMemcpyAsync((euler_tracer*)S->tracer_buf.p + S->n_tracers, host, n * sizeof(euler_tracer), hipMemcpyHostToDevice, S->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(S->stream);      // (the staging copy is free to go)
    if (e != hipSuccess) rc = eu_hip_fail(e, "euler_tracers_add: upload", __FILE__, __LINE__);
  }
  free(host);
  if (!rc) S->n_tracers += n;
  return rc;
}

extern "C" int euler_tracers_count(euler_sim* S, size_t* n) {
  if (!S || !n) { eu_set_error("euler_tracers_count: null argument"); return EULER_EINVAL; }
  *n = S->n_tracers;
  return EULER_OK;
}

extern "C" int euler_tracers_get(euler_sim* S, size_t first, size_t n, euler_tracer* out, size_t out_bytes) {
  const char* who = "euler_tracers_get";
  if (!S || (n && !out)) { eu_set_error("%s: null argument", who); return EULER_EINVAL; }
  if (first > S->n_tracers || n > S->n_tracers - first) { eu_set_error("%s: records [%zu, %zu + %zu) of %zu", who, first, first, n, S->n_tracers); return EULER_EINVAL; }
  if (out_bytes != n * sizeof(euler_tracer)) { eu_set_error("%s: %zu bytes given, %zu expected", who, out_bytes, n * sizeof(euler_tracer)); return EULER_EINVAL; }
  if (!n) return EULER_OK;
  HIPCHK(hipMemcpyAsync(out, (const euler_tracer*)S->tracer_buf.p + first, out_bytes, hipMemcpyDeviceToHost, S->stream));
  HIPCHK(hipStreamSynchronize(S->stream));
  return EULER_OK;
}

extern "C" int euler_tracers_clear(euler_sim* S) {
  if (!S) { eu_set_error("euler_tracers_clear: null argument"); return EULER_EINVAL; }
  S->n_tracers = 0;      // (the buffer stays)
  return EULER_OK;
}

// ------------------------------------------------------------------------------------------ the raster
// One pass over the records behind a clear of the raster, one record per lane.  A record counts in the pixel that covers its cell (floorf(x), floorf(y)); the
// cell lies in the box exactly when x0 <= x < x1 + 1 and y0 <= y < y1 + 1 (integers below 2^24 as floats: exact; a NaN fails, an infinity the upper bound).
// The pixel of a cell, in integers: column c = cx - x0 of the box lies in the pixel column px with floor(px Bw / W) <= c < floor((px + 1) Bw / W), which is
// px = ((c + 1) W - 1) / Bw; rows alike from the top, r = y1 - cy (euler_host.h eu_tracer_pixel).  Integer adds: the counts do not depend on the launch geometry.
struct TrRasterArgs {
  const euler_tracer* rec;
  unsigned int n;
  float fx0, fy0, fx1, fy1;      // x0, y0, x1 + 1, y1 + 1
  int x0, y1, Bw, Bh, W, H, all;
  unsigned int* out;
};

__global__ __launch_bounds__(TR_T) void k_tracer_raster(const TrRasterArgs a) {
  const unsigned int i = blockIdx.x * TR_T + threadIdx.x;
  bool in = false;
  float x = 0.f, y = 0.f;
  if (i < a.n) {
    const float4 lo = *reinterpret_cast<const float4*>(a.rec + i);
    const uint32_t flags = a.all ? 0u : a.rec[i].flags;
    x = lo.x; y = lo.y;
    in = !(flags & EULER_TRACER_RETIRED) && x >= a.fx0 && x < a.fx1 && y >= a.fy0 && y < a.fy1;
  }
  if (!__any(in)) return;      // nothing of this wave lies in the box: no memory traffic beyond the load
  if (!in) return;
  const int c = (int)x - a.x0, r = a.y1 - (int)y;      // (x, y >= 1: truncation is floor)
  const unsigned int px = (unsigned int)(eu_tracer_pixel(c, a.Bw, a.W)), py = (unsigned int)(eu_tracer_pixel(r, a.Bh, a.H));
  atomicAdd(&a.out[(size_t)py * a.W + px], 1u);
}

extern "C" int euler_tracer_raster(euler_sim* S, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t W, int32_t H, int32_t flags, uint32_t* out, size_t out_bytes) {
  const char* who = "euler_tracer_raster";
  int rc = eu_observe_enter(S, who, "tracers live on whole-grid handles", out, x0, y0, x1, y1);
  if (rc) return rc;
  const int Bw = x1 - x0 + 1, Bh = y1 - y0 + 1;
  if (W < 1 || H < 1 || W > Bw || H > Bh) { eu_set_error("%s: a raster of %d x %d for a box of %d x %d cells", who, W, H, Bw, Bh); return EULER_EINVAL; }
  const size_t bytes = (size_t)W * (size_t)H * sizeof(uint32_t);
  if (out_bytes != bytes) { eu_set_error("%s: %zu bytes given, %zu expected", who, out_bytes, bytes); return EULER_EINVAL; }
  if (flags & ~EULER_TRACER_RASTER_ALL) { eu_set_error("%s: unknown flag bits %d", who, flags & ~EULER_TRACER_RASTER_ALL); return EULER_EINVAL; }
  rc = eu_devbuf_reserve(S, who, "the raster", &S->tracer_ras_buf, bytes);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(S->tracer_ras_buf.p, 0, bytes, S->stream));
  if (S->n_tracers) {
    TrRasterArgs a;
    a.rec = (const euler_tracer*)S->tracer_buf.p; a.n = (unsigned int)S->n_tracers;
    a.fx0 = (float)x0; a.fy0 = (float)y0; a.fx1 = (float)(x1 + 1); a.fy1 = (float)(y1 + 1);
    a.x0 = x0; a.y1 = y1; a.Bw = Bw; a.Bh = Bh; a.W = W; a.H = H; a.all = (flags & EULER_TRACER_RASTER_ALL) != 0;
    a.out = (unsigned int*)S->tracer_ras_buf.p;
    LAUNCH(S, KC_MISC, k_tracer_raster, dim3(eu_blocks(a.n, TR_T)), dim3(TR_T), a);
    HIPCHK(hipGetLastError());
  }
  return eu_observe_readback(S, out, &S->tracer_ras_buf, bytes);
}
