// k_advect_one.h — the walk of ONE marker through one substep (main.c:464-537 for a single marker): what the marker kernels (k_markers.hip) and the
// passive tracers (k_tracers.hip, docs/tracers.md) share.  The chain that couples the markers of an array - `dt -= t_prev` on the function parameter - is
// k_markers.hip's; here a caller gets the marker's new position and the collision it would report (theta, delta, events).
#pragma once
#include "euler_dev.h"
#include "k_transport.h"

#include <float.h>

struct AdvectOut { float px, py, theta, delta; int events; };

__device__ __forceinline__ float time_to(float p0, float p1, float vel) {   // main.c:451-457
  return fabsf(vel) > 0.f ? (p1 - p0) / vel : FLT_MAX;
}

// TR: u, v, g.count and solid are the COLUMN-major copies (k_transpose_for_markers): the marker array walks the grid column by column (main.c:243-266), so a wave's
// 64 markers sit in ~16 cells of one column - 16-17 cache lines per gather in the row-major fields, one or two in the column-major ones.  The same values: the same bits.
// RK2 (EULER_OPT_ADVECT_RK2): the walk runs with the velocity at the midpoint p + (dt_mid / 2) v(p) instead of v(p); nothing else changes.  dt_mid is always the
// SUBSTEP's dt, never the one the chain shortened (dt): theta and delta then do not depend on the chain, and the walk / pass-B replay stays valid as it is.
// The midpoint's components are bounded by the maxima calculate_timestep uses (a masked bilinear interpolation is a convex combination of live samples, or 0), so it lies
// <= 0.375 cells from p and the displacement stays <= 0.75 cells: still at most one boundary per axis.  With TR, uT / vT are not refreshed in tiles the last copy left
// alone (k_transpose_for_markers, lean): such stale samples are never read here either - eu_interp<.., TR> uses a sample only where its corner bit in countT is set, and
// that bit belongs to the sample's cell, not to the query point, so a midpoint lookup sees exactly the live samples a start-point lookup there would.
// (The rule for any new reader of uT / vT / countT: k_transport.h eu_interp, docs/stage_validity.md.)
template <bool TR, bool RK2>
__device__ __forceinline__ AdvectOut advect_one(const GridRef& g, const float* __restrict__ u, const float* __restrict__ v,
                                                const uint8_t* __restrict__ solid, float px, float py, float dt, float dt_mid) {
  AdvectOut o;
  o.events = 0; o.theta = 0.f; o.delta = 0.f;
  // velocity_at (main.c:440-449)
  float vx = eu_interp<1, TR>(g, u, px / EU_H - 1.f, py / EU_H - 0.5f);
  float vy = eu_interp<2, TR>(g, v, px / EU_H - 0.5f, py / EU_H - 1.f);
  if (RK2) { const float2 m = eu_mid_vel_pos<TR>(g, u, v, px, py, vx, vy, 0.5f * dt_mid); vx = m.x; vy = m.y; }
  auto is_solid = [&](int sy_, int sx_) -> bool { return solid[TR ? (size_t)sx_ * g.Y + sy_ : (size_t)sy_ * g.X + sx_] != 0; };
  int xi = (int)floorf(px / EU_H), yi = (int)floorf(py / EU_H);
  const int xdir = vx > 0 ? 1 : -1;
  int nxi = xi + (vx > 0 ? 1 : 0);
  float npx = nxi * EU_H;
  const int ydir = vy > 0 ? 1 : -1;
  int nyi = yi + (vy > 0 ? 1 : 0);
  float npy = nyi * EU_H;
  float tx = time_to(px, npx, vx);
  const int xoff = vx < 0 ? -1 : 0;
  float ty = time_to(py, npy, vy);
  const int yoff = vy < 0 ? -1 : 0;
  float t_prev = 0.f, t_near = fminf(tx, ty);
  int guard = 0;
  while (t_near < dt && guard++ < 64) {
    if (tx < ty) {
      if (is_solid(yi, nxi + xoff)) {
        if (t_prev > 0.f) { if (o.events == 0) { o.theta = t_near; o.delta = t_prev; } o.events++; }
        px = px + t_prev * vx; py = py + t_prev * vy;
        dt -= t_prev; t_near = 0.f; vx = 0.f; tx = FLT_MAX;
        ty = time_to(py, npy, vy);
      } else {
        xi = nxi; nxi = xi + xdir; npx = nxi * EU_H;
        tx = time_to(px, npx, vx);
      }
    } else {
      if (is_solid(nyi + yoff, xi)) {
        if (t_prev > 0.f) { if (o.events == 0) { o.theta = t_near; o.delta = t_prev; } o.events++; }
        px = px + t_prev * vx; py = py + t_prev * vy;
        dt -= t_prev; t_near = 0.f; vy = 0.f; ty = FLT_MAX;
        tx = time_to(px, npx, vx);
      } else {
        yi = nyi; nyi = yi + ydir; npy = nyi * EU_H;
        ty = time_to(py, npy, vy);
      }
    }
    t_prev = t_near;
    t_near = fminf(tx, ty);
  }
  const float t = (t_near < FLT_MAX) ? dt : t_prev;
  o.px = px + t * vx;
  o.py = py + t * vy;
  return o;
}
