// k_viewport.hip — euler_marker_raster and euler_render_view (include/euler.h, docs/viewport.md): the markers of a box of cells counted on the
// device into a raster of scale x scale sub-pixels per cell, and the frame of a box in a window (below one cell per glyph: the box overview of
// k_overview.hip; above: the raster through euler_view_text).
//
// One pass over the marker array, 8 bytes per marker, two markers (one 16-byte load) per lane.  A marker's sub-pixel is
//   c = floor((m.x - x0) * scale), r = H - 1 - floor((m.y - y0) * scale):
// inside the box the subtraction is exact (positions below 2^24, x0 an integer <= m.x) and so is the multiplication by a power of two; outside
// it the rounded difference lies on the same side of 0 and of Bw as the exact one.  The counts are therefore integers of exact arithmetic,
// whatever the launch geometry.  A wave without a marker in the box leaves after its load; in the others, a lane whose two markers share a
// sub-pixel carries a weight of 2, and a RUN of lanes on one sub-pixel (the array keeps neighbours in space neighbours in memory) folds to its first
// lane, which issues one 32-bit integer add whose result nobody reads.
//
// The pass only reads the marker array and touches none of the handle's validity flags.
#include "euler_dev.h"

#include <stdlib.h>

#define VR_T 256              // threads per workgroup: 512 markers
#define VR_MAX_PIXELS (1 << 24)

struct VrArgs {
  const float4* m2;           // the marker array, two markers per element
  unsigned long long n;       // markers
  float fx0, fy0, fs, fW, fH; // the box origin, the scale and the raster's extent as floats (all exact: integers <= 2^24)
  float fylo, fyhi;           // the sub-pixel rows counted, from the box's bottom: 0 and fH; row slabs: those of the rank's own cell rows (a marker on its way to a neighbour is the neighbour's)
  int W, H;
  unsigned int* out;
};

// the sub-pixel of a position; false: outside the box (a NaN fails every comparison, an infinity the upper ones)
__device__ __forceinline__ bool vr_pixel(const VrArgs& a, float x, float y, unsigned int& pix) {
  const float sx = (x - a.fx0) * a.fs, sy = (y - a.fy0) * a.fs;
  const bool in = sx >= 0.f && sx < a.fW && sy >= a.fylo && sy < a.fyhi;
  pix = in ? (unsigned int)(a.H - 1 - (int)sy) * (unsigned int)a.W + (unsigned int)(int)sx : 0u;      // (W * H <= 2^24: no wrap)
  return in;
}

// bin_aggregated (euler_dev.h) for row-major pixels with a weight of 1 or 2 per lane: the first lane of a run of live lanes on one pixel adds the run's weights
__device__ __forceinline__ void vr_add_runs(unsigned int* out, bool live, unsigned int pix, unsigned int w) {
  const int lane = threadIdx.x & 63;
  const unsigned int ppix = __shfl_up(pix, 1, 64);
  const bool plive = __shfl_up((int)live, 1, 64) != 0;
  const bool head = live && (lane == 0 || !plive || ppix != pix);
  const unsigned long long heads = __ballot(head), lives = __ballot(live), twos = __ballot(live && w == 2u);
  if (!head) return;      // (no cross-lane operation below)
  // the run ends before the next head or the next dead lane
  const unsigned long long above = lane == 63 ? 0ull : ((heads | ~lives) >> (lane + 1));
  const int run = above ? __ffsll((long long)above) : 64 - lane;
  const unsigned long long span = (run == 64 ? ~0ull : ((1ull << run) - 1ull)) << lane;
  atomicAdd(&out[pix], (unsigned int)run + (unsigned int)__popcll(twos & span));
}

__global__ __launch_bounds__(VR_T) void k_marker_raster(const VrArgs a) {
  const unsigned long long j = (unsigned long long)blockIdx.x * VR_T + threadIdx.x, i0 = 2ull * j;      // this lane's markers: i0, i0 + 1
  bool in0 = false, in1 = false;
  unsigned int pix0 = 0u, pix1 = 0u;
  if (i0 + 1ull < a.n) {
    const float4 p = a.m2[j];
    in0 = vr_pixel(a, p.x, p.y, pix0);
    in1 = vr_pixel(a, p.z, p.w, pix1);
  } else if (i0 < a.n) {      // an odd count: the last marker alone
    const float2 p = reinterpret_cast<const float2*>(a.m2)[i0];
    in0 = vr_pixel(a, p.x, p.y, pix0);
  }
  if (!__any(in0 || in1)) return;      // nothing of this wave lies in the box: no memory traffic beyond the load
  const bool same = in0 && in1 && pix0 == pix1, second = in0 && in1 && !same;
  vr_add_runs(a.out, in0 || in1, in0 ? pix0 : pix1, same ? 2u : 1u);
  if (__any(second)) vr_add_runs(a.out, second, pix1, 1u);
}

// the clear and the pass alone, on the handle's stream, into the raster of S->vr_buf (tools/viewport_cost.py times the pass through the KC_MISC class)
// ya, yb: the cell rows counted (the box's; row slabs: the rank's own rows of it, ya > yb: none); n: the markers of the array
static int vr_launch(euler_sim* S, int x0, int y0, int scale, int W, int H, int ya, int yb, unsigned long long n) {
  HIPCHK(hipMemsetAsync(S->vr_buf.p, 0, (size_t)W * H * sizeof(unsigned int), S->stream));
  if (!n || ya > yb) return EULER_OK;
  VrArgs a;
  a.m2 = reinterpret_cast<const float4*>(S->markers[S->cur]); a.n = n;
  a.fx0 = (float)x0; a.fy0 = (float)y0; a.fs = (float)scale; a.fW = (float)W; a.fH = (float)H;
  a.fylo = (float)((ya - y0) * scale); a.fyhi = (float)((yb + 1 - y0) * scale);      // (the box's rows: 0 and fH)
  a.W = W; a.H = H; a.out = (unsigned int*)S->vr_buf.p;
  const unsigned long long nwg = (n + 2ull * VR_T - 1ull) / (2ull * VR_T);      // (at most max_markers / 512: far below 2^31 on any grid euler_create accepts)
  LAUNCH(S, KC_MISC, k_marker_raster, dim3((unsigned)nwg), dim3(VR_T), a);
  HIPCHK(hipGetLastError());
  return EULER_OK;
}

// euler_marker_raster behind the entry checks (euler_render_view enters once for both of its passes)
static int vr_entered(euler_sim* S, int x0, int y0, int x1, int y1, int scale, uint32_t* out, size_t out_bytes) {
  if (scale != 1 && scale != 2 && scale != 4 && scale != 8 && scale != 16) { eu_set_error("euler_marker_raster: scale %d: 1, 2, 4, 8 or 16", scale); return EULER_EINVAL; }
  const long long W = (long long)(x1 - x0 + 1) * scale, H = (long long)(y1 - y0 + 1) * scale;
  if (W * H > VR_MAX_PIXELS) { eu_set_error("euler_marker_raster: a raster of %lld x %lld pixels (at most 2^24)", W, H); return EULER_EINVAL; }
  const size_t n = (size_t)(W * H);
  if (out_bytes != n * sizeof(uint32_t)) { eu_set_error("euler_marker_raster: %zu bytes given, %zu expected", out_bytes, n * sizeof(uint32_t)); return EULER_EINVAL; }
  int rc = eu_devbuf_reserve(S, "euler_marker_raster", "the raster", &S->vr_buf, out_bytes);
  if (S->slab_on) {      // collective: a rank counts its own markers into the raster rows of its own cell rows - disjoint between ranks -, an in-place all-gather makes the raster whole
    int64_t off[EU_SLAB_PLAN_MAXR], cnt[EU_SLAB_PLAN_MAXR];
    const int R = S->cfg.slab_nranks;
    if (R > EU_SLAB_PLAN_MAXR) { eu_set_error("euler_marker_raster: %d ranks", R); return EULER_EINVAL; }
    int ya = 0, yb = -1;
    for (int r = 0; r < R; ++r) {      // raster row H - 1 - k holds sub-row k from the box's bottom: the rows [ya, yb] are the raster rows H - (yb + 1 - y0) scale ... H - 1 - (ya - y0) scale
      int a0, b0;
      const int some = eu_slab_clip_rows(S->part_lo[r], S->part_hi[r], S->Y, y0, y1, &a0, &b0);
      off[r] = some ? (int64_t)(H - (long long)(b0 + 1 - y0) * scale) * W * (int64_t)sizeof(uint32_t) : 0;
      cnt[r] = some ? (int64_t)(b0 - a0 + 1) * scale * W * (int64_t)sizeof(uint32_t) : 0;
      if (r == S->cfg.slab_rank) { ya = a0; yb = b0; }
    }
    rc = eu_observe_slab_open(S, "euler_marker_raster", rc, 0, EU_OBS_ROWS_NONE);
    unsigned long long n_loc = 0;      // (read here, not through eu_sync_marker_state: between two stages the host's count is the substep's, and stays)
    if (!rc) {
      HIPCHK(hipMemcpyAsync(&n_loc, &S->ms->n_loc, sizeof n_loc, hipMemcpyDeviceToHost, S->stream));
      HIPCHK(hipStreamSynchronize(S->stream));
      rc = vr_launch(S, x0, y0, scale, (int)W, (int)H, ya, yb, n_loc);
    }
    if (!rc) rc = eu_observe_slab_gather_in_place(S, S->vr_buf.p, off, cnt);
  } else
  if (!rc) rc = vr_launch(S, x0, y0, scale, (int)W, (int)H, y0, y1, S->n_markers_host);
  return rc ? rc : eu_observe_readback(S, out, &S->vr_buf, out_bytes);
}

extern "C" int euler_marker_raster(euler_sim* S, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t scale, uint32_t* out, size_t out_bytes) {
  const int rc = eu_observe_enter(S, "euler_marker_raster", nullptr, out, x0, y0, x1, y1);
  return rc ? rc : vr_entered(S, x0, y0, x1, y1, scale, out, out_bytes);
}

extern "C" int euler_render_view(euler_sim* S, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t wx, int32_t wy, char* out, int32_t cap, int32_t* len) {
  if (!S || !len || wx < 1 || wy < 1) { eu_set_error("euler_render_view: bad argument"); return EULER_EINVAL; }
  int rc = eu_observe_enter(S, "euler_render_view", nullptr, len, x0, y0, x1, y1);
  if (rc) return rc;
  const int Bw = x1 - x0 + 1, Bh = y1 - y0 + 1;
  int scale = 0;      // 0: at or below one cell per glyph
  if ((long long)Bw * 2 <= wx && (long long)Bh * 2 <= wy)
    for (scale = 16; (long long)Bw * scale > wx || (long long)Bh * scale > wy; scale >>= 1) {}
  const int W = scale ? Bw : (wx < Bw ? wx : Bw), H = scale ? Bh : (wy < Bh ? wy : Bh);
  const size_t bytes = (size_t)W * H * sizeof(euler_overview_px), rbytes = scale ? (size_t)Bw * scale * Bh * scale * sizeof(uint32_t) : 0;
  euler_overview_px* px = (euler_overview_px*)malloc(bytes);
  uint32_t* ras = scale ? (uint32_t*)malloc(rbytes) : nullptr;
  rc = px && (!scale || ras) ? EULER_OK : EULER_ENOMEM;
  if (rc) eu_set_error("euler_render_view: %zu bytes of host memory", bytes + rbytes);
  if (!rc) rc = eu_overview_entered(S, "euler_overview_box", x0, y0, x1, y1, W, H, px, bytes);
  if (!rc && scale) rc = vr_entered(S, x0, y0, x1, y1, scale, ras, rbytes);
  if (!rc) rc = scale ? euler_view_text(px, ras, Bw, Bh, scale, S->cfg.rainbow, out, cap, len) : euler_overview_text(px, W, H, S->cfg.rainbow, out, cap, len);
  free(px); free(ras);
  return rc;
}
