// k_transport.h — the semi-Lagrangian transport that the velocity (k_grid.hip), the dye (k_dye.hip), the temperature (k_heat.hip), the markers (k_markers.hip,
// k_advect_one.h) and the tracers (k_tracers.hip) share (docs/transport.md): the masked bilinear interpolation, the midpoint rule, the back-trace of a grid sample
// and the MacCormack value on the device; on the host the GridRef of a handle and the step from a run-time flag to a template argument.
// Every expression here is pinned bit for bit (tests/*_ref.py, the oracle): the library is built without contraction, and the ORDER of the operations is the reference's.
#pragma once
#include "euler_dev.h"

#include <type_traits>

struct GridRef {
  int X, Y;
  const uint8_t* count;   // g_fluid alias (main.c:99)
  float ux_lim, uy_lim, vx_lim, vy_lim;
};
static inline GridRef eu_grid_ref(const euler_sim* S) { return GridRef{S->X, S->Y, S->count, S->interp_lim[0], S->interp_lim[1], S->interp_lim[2], S->interp_lim[3]}; }

// A run-time flag as a template argument: f(std::true_type{}) or f(std::false_type{}).  A launcher names each kernel template once,
//   eu_flag(S->opt[...] != 0, [&](auto R) { LAUNCH(S, cls, (k<decltype(R)::value>), ...); });
// and nests two of these for two flags.
template <class F>
static inline void eu_flag(bool on, F&& f) {
  if (on) f(std::true_type{});
  else f(std::false_type{});
}

// typed cell property (p_property/u_property/v_property, main.c:119-138)
__device__ __forceinline__ bool eu_prop_p(const uint8_t* g, size_t i) { return g[i] != 0; }
__device__ __forceinline__ bool eu_prop_u(const uint8_t* g, size_t i) { return (g[i] != 0) | (g[i + 1] != 0); }
__device__ __forceinline__ bool eu_prop_v(const uint8_t* g, size_t i, int X) { return (g[i] != 0) | (g[i + X] != 0); }

__device__ __forceinline__ float eu_lerp(float x0, float x1, float f) { return (1.f - f) * x0 + f * x1; }   // main.c:311-313
__device__ __forceinline__ float eu_frac(float f, bool start_ok, bool end_ok) {                            // main.c:301-309
  return !start_ok ? 1.f : (!end_ok ? 0.f : f);
}
__device__ __forceinline__ float eu_clampf(float lo, float x, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

// interpolate(), main.c:337-364, written once.  TYPE 0 = cell centres (P), 1 = U samples, 2 = V samples.
// CONSUMERS of the transposed inputs (TR): uT, vT and countT are left UNWRITTEN over tiles without water (k_transpose_for_markers, lean - eu_valid.h countT_clean), so a
// sample of q is valid only where its bit of the props byte is set; the bytes over an idle tile are the zeros an earlier full pass left, its samples are whatever was there.
// Read a sample without its bit and the lean and the plain form stop giving the same bits.
// TR: q and g.count are stored COLUMN-major, [x][y] (the marker stage's copies: k_markers.hip) - the same values, the strides swapped
// PROPS: g.count does not hold counts but, per cell, the typed fluid properties of the four corners of an interpolation whose BASE cell it is (bits 0-3 U-typed, 4-7 V-typed,
// corner order v00 v01 v10 v11; k_transpose_for_markers): one byte gather instead of six
// MC (EULER_OPT_ADVECT_MACCORMACK, docs/advection_maccormack.md): also report whether any corner is valid and, with LIM, the min (lo) and max (hi) of q over the valid
// corners, folded in the order 00, 01, 10, 11 with strict compares; without MC the three are left alone.
// (One body, not helpers that hand the corner flags on: flags that cross a function boundary change the code of every kernel that interpolates - profiles/transport_refactor.md.)
template <int TYPE, bool TR, bool PROPS, bool MC, bool LIM>
__device__ __forceinline__ float eu_interp_any(const GridRef& g, const float* __restrict__ q, float ix, float iy, bool& any, float& lo, float& hi) {
  ix = eu_clampf(0.f, ix, TYPE == 1 ? g.ux_lim : g.vx_lim);   // P extent = (X, Y): x like V, y like U
  iy = eu_clampf(0.f, iy, TYPE == 2 ? g.vy_lim : g.uy_lim);
  float wx, wy;
  const float fx = modff(ix, &wx), fy = modff(iy, &wy);
  const int bx = (int)wx, by = (int)wy;
  const size_t sx = TR ? (size_t)g.Y : (size_t)1, sy = TR ? (size_t)1 : (size_t)g.X;      // one step in x / in y
  const size_t i00 = (size_t)by * sy + (size_t)bx * sx;
  // the four samples are loaded unconditionally and next to the mask bytes (the clamps keep all of them inside the arrays,
  // ghost rows included): one memory round trip instead of two - the kernels that interpolate are latency-bound
  const float r00 = q[i00], r01 = q[i00 + sx], r10 = q[i00 + sy], r11 = q[i00 + sy + sx];
  bool v00, v01, v10, v11;
  if (PROPS && TYPE != 0) {
    // ONE byte instead of six counts - the passes that interpolate are bound by their gather instructions and the lines each touches
    const unsigned int nb = g.count[i00] >> (TYPE == 1 ? 0 : 4);
    v00 = (nb & 1u) != 0; v01 = (nb & 2u) != 0; v10 = (nb & 4u) != 0; v11 = (nb & 8u) != 0;
  } else
  if (TYPE == 0) {
    v00 = g.count[i00] != 0; v01 = g.count[i00 + sx] != 0;
    v10 = g.count[i00 + sy] != 0; v11 = g.count[i00 + sy + sx] != 0;
  } else if (TYPE == 1) {
    const bool c0 = g.count[i00] != 0, c1 = g.count[i00 + sx] != 0, c2 = g.count[i00 + 2 * sx] != 0;
    const bool d0 = g.count[i00 + sy] != 0, d1 = g.count[i00 + sy + sx] != 0, d2 = g.count[i00 + sy + 2 * sx] != 0;
    v00 = c0 | c1; v01 = c1 | c2; v10 = d0 | d1; v11 = d1 | d2;
  } else {
    const bool c0 = g.count[i00] != 0, c1 = g.count[i00 + sx] != 0;
    const bool d0 = g.count[i00 + sy] != 0, d1 = g.count[i00 + sy + sx] != 0;
    const bool e0 = g.count[i00 + 2 * sy] != 0, e1 = g.count[i00 + 2 * sy + sx] != 0;
    v00 = c0 | d0; v01 = c1 | d1; v10 = d0 | e0; v11 = d1 | e1;
  }
  if (MC) {
    any = v00 | v01 | v10 | v11;
    if (LIM) {
      lo = __builtin_inff(); hi = -__builtin_inff();
      if (v00) { lo = r00 < lo ? r00 : lo; hi = r00 > hi ? r00 : hi; }
      if (v01) { lo = r01 < lo ? r01 : lo; hi = r01 > hi ? r01 : hi; }
      if (v10) { lo = r10 < lo ? r10 : lo; hi = r10 > hi ? r10 : hi; }
      if (v11) { lo = r11 < lo ? r11 : lo; hi = r11 > hi ? r11 : hi; }
    }
  }
  const float q00 = v00 ? r00 : 0.f, q01 = v01 ? r01 : 0.f;
  const float q10 = v10 ? r10 : 0.f, q11 = v11 ? r11 : 0.f;
  const float lf = eu_frac(fy, v00, v10), rf = eu_frac(fy, v01, v11);
  const float lv = eu_lerp(q00, q10, lf), rv = eu_lerp(q01, q11, rf);
  const float hf = eu_frac(fx, v00 | v10, v01 | v11);
  return eu_lerp(lv, rv, hf);
}
template <int TYPE, bool TR = false, bool PROPS = TR>
__device__ __forceinline__ float eu_interp(const GridRef& g, const float* __restrict__ q, float ix, float iy) {
  bool any;
  float lo, hi;
  return eu_interp_any<TYPE, TR, PROPS, false, false>(g, q, ix, iy, any, lo, hi);
}
// ... over row-major q with the count masks, for the MacCormack passes
template <int TYPE, bool LIM>
__device__ __forceinline__ float eu_interp_mc(const GridRef& g, const float* __restrict__ q, float ix, float iy, bool& any, float& lo, float& hi) {
  return eu_interp_any<TYPE, false, false, true, LIM>(g, q, ix, iy, any, lo, hi);
}
// out = f + 0.5 (q0 - b), clamped to [lo, hi]; f alone where the forward or the backward interpolation had no valid corner
__device__ __forceinline__ float eu_mc_correct(float f, float q0, float b, bool a1, bool a2, float lo, float hi) {
  if (!(a1 && a2)) return f;
  const float out = f + 0.5f * (q0 - b);
  return out < lo ? lo : (out > hi ? hi : out);
}

// the index (x, y) carried back along the velocity (dx, dy) for dt (main.c:392-393): the one place where the trace is spelt out
__device__ __forceinline__ float2 eu_back(float x, float y, float dx, float dy, float dt) { return make_float2(x - dx * dt / EU_H, y - dy * dt / EU_H); }

// EULER_OPT_ADVECT_RK2 (docs/advection_rk2.md): the midpoint rule.  The start-point velocity (d0x, d0y) at index (x, y) of the given index space is carried half a step,
// hdt = 0.5f * dt, back; the velocity interpolated there replaces it in the unchanged back-trace.  Index spaces (EU_H = 1): a position maps to u index pos - (1, 0.5),
// v index pos - (0.5, 1), p index pos - (0.5, 0.5).  The two gathers of each helper do not depend on each other: they are issued together.
template <bool TR = false>
__device__ __forceinline__ float2 eu_mid_vel_uidx(const GridRef& g, const float* __restrict__ u, const float* __restrict__ v, float x, float y, float d0x, float d0y, float hdt) {
  const float2 m = eu_back(x, y, d0x, d0y, hdt);
  return make_float2(eu_interp<1, TR>(g, u, m.x, m.y), eu_interp<2, TR>(g, v, m.x + 0.5f, m.y - 0.5f));      // (vidx_from_u)
}
template <bool TR = false>
__device__ __forceinline__ float2 eu_mid_vel_vidx(const GridRef& g, const float* __restrict__ u, const float* __restrict__ v, float x, float y, float d0x, float d0y, float hdt) {
  const float2 m = eu_back(x, y, d0x, d0y, hdt);
  return make_float2(eu_interp<1, TR>(g, u, m.x - 0.5f, m.y + 0.5f), eu_interp<2, TR>(g, v, m.x, m.y));      // (uidx_from_v)
}
template <bool TR = false>
__device__ __forceinline__ float2 eu_mid_vel_pidx(const GridRef& g, const float* __restrict__ u, const float* __restrict__ v, float x, float y, float d0x, float d0y, float hdt) {
  const float2 m = eu_back(x, y, d0x, d0y, hdt);
  return make_float2(eu_interp<1, TR>(g, u, m.x - 0.5f, m.y), eu_interp<2, TR>(g, v, m.x, m.y - 0.5f));
}
// a marker: velocity_at (main.c:440-449) half a step FORWARD from position (px, py)
template <bool TR = false>
__device__ __forceinline__ float2 eu_mid_vel_pos(const GridRef& g, const float* __restrict__ u, const float* __restrict__ v, float px, float py, float v0x, float v0y, float hdt) {
  const float mx = px + hdt * v0x, my = py + hdt * v0y;
  return make_float2(eu_interp<1, TR>(g, u, mx / EU_H - 1.f, my / EU_H - 0.5f), eu_interp<2, TR>(g, v, mx / EU_H - 0.5f, my / EU_H - 1.f));
}

// The back-trace of the grid sample at index (x, y) of an index space - EU_SPACE_P: cell centres, _U / _V: the faces - whose start velocity (d0x, d0y) the caller has
// formed: (px, py) is where the sample comes from (RK2: along the midpoint velocity) and, with BACK, (qx, qy) is the same trace run with -dt - MacCormack's way back
// from the forward result.  Forward before backward, the midpoints before the points: the order the kernels always had.
enum { EU_SPACE_P = 0, EU_SPACE_U = 1, EU_SPACE_V = 2 };
struct EuTrace { float px, py, qx, qy; };
template <int SPACE, bool RK2, bool BACK>
__device__ __forceinline__ EuTrace eu_trace(const GridRef& g, const float* __restrict__ u, const float* __restrict__ v, float x, float y, float d0x, float d0y, float dt) {
  auto mid = [&](float hdt) {
    if (SPACE == EU_SPACE_U) return eu_mid_vel_uidx(g, u, v, x, y, d0x, d0y, hdt);
    if (SPACE == EU_SPACE_V) return eu_mid_vel_vidx(g, u, v, x, y, d0x, d0y, hdt);
    return eu_mid_vel_pidx(g, u, v, x, y, d0x, d0y, hdt);
  };
  const float bdt = -dt;
  float2 fd = make_float2(d0x, d0y), bd = fd;
  if (RK2) {
    fd = mid(0.5f * dt);
    if (BACK) bd = mid(0.5f * bdt);
  }
  const float2 p = eu_back(x, y, fd.x, fd.y, dt);
  EuTrace t = {p.x, p.y, 0.f, 0.f};
  if (BACK) { const float2 q = eu_back(x, y, bd.x, bd.y, bdt); t.qx = q.x; t.qy = q.y; }
  return t;
}

// the MacCormack value of one sample of q (q0: its own value, qf: the forward results): the forward interpolation with the limiter's bounds, the backward one into qf,
// half the round-trip error added and the result clamped
template <int TYPE>
__device__ __forceinline__ float eu_mc_value(const GridRef& g, const float* __restrict__ q, const float* __restrict__ qf, float q0, const EuTrace& t) {
  bool a1, a2;
  float lo, hi;
  const float f = eu_interp_mc<TYPE, true>(g, q, t.px, t.py, a1, lo, hi);
  const float b = eu_interp_mc<TYPE, false>(g, qf, t.qx, t.qy, a2, lo, hi);
  return eu_mc_correct(f, q0, b, a1, a2, lo, hi);
}
