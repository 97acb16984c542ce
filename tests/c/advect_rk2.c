/* advect_rk2.c - test-side restatement of the midpoint (RK2) transport of EULER_OPT_ADVECT_RK2
 * (docs/advection_rk2.md), on top of the oracle's exported eo_interpolate and eo_sim arrays.
 *
 * Every function takes `rk2`: 0 bypasses the midpoint, and the function is then the oracle's own
 * forward-Euler stage statement for statement (eo_advect_u / _v / _p / eo_advect_markers), which
 * the host tests check bit for bit before anything relies on the midpoint path.
 *
 * Built at test time: gcc -O2 -ffp-contract=off -shared, linked against liboracle.so. */
#include <float.h>
#include <math.h>
#include <stddef.h>

#include "euler_oracle.h"

#define H_CELL 1.0f
#define AT(s, y, x) ((size_t)(y) * (size_t)(s)->X + (size_t)(x))

static inline int prop(const eo_sim* s, const uint8_t* g, int x, int y, int type) {
  size_t i = AT(s, y, x);
  switch (type) {
    case EO_U: return (g[i] != 0) | (g[i + 1] != 0);
    case EO_V: return (g[i] != 0) | (g[i + (size_t)s->X] != 0);
    default:   return g[i] != 0;
  }
}

void ar_advect_u(const eo_sim* s, const float* u, const float* v, float dt, float* out, int rk2) {
  const float hdt = 0.5f * dt;
  for (int y = 0; y < s->Y; ++y)
    for (int x = 0; x < s->X - 1; ++x) {
      if (!prop(s, s->count, x, y, EO_U)) continue;
      float dx = u[AT(s, y, x)];
      float dy = eo_interpolate(s, v, x + 0.5f, y - 0.5f, EO_V);
      if (rk2) {
        float mx = x - dx * hdt / H_CELL, my = y - dy * hdt / H_CELL;
        dx = eo_interpolate(s, u, mx, my, EO_U);
        dy = eo_interpolate(s, v, mx + 0.5f, my - 0.5f, EO_V);
      }
      float px = x - dx * dt / H_CELL, py = y - dy * dt / H_CELL;
      out[AT(s, y, x)] = eo_interpolate(s, u, px, py, EO_U);
    }
}

void ar_advect_v(const eo_sim* s, const float* u, const float* v, float dt, float* out, int rk2) {
  const float hdt = 0.5f * dt;
  for (int y = 0; y < s->Y - 1; ++y)
    for (int x = 0; x < s->X; ++x) {
      if (!prop(s, s->count, x, y, EO_V)) continue;
      float dy = v[AT(s, y, x)];
      float dx = eo_interpolate(s, u, x - 0.5f, y + 0.5f, EO_U);
      if (rk2) {
        float mx = x - dx * hdt / H_CELL, my = y - dy * hdt / H_CELL;
        dy = eo_interpolate(s, v, mx, my, EO_V);
        dx = eo_interpolate(s, u, mx - 0.5f, my + 0.5f, EO_U);
      }
      float px = x - dx * dt / H_CELL, py = y - dy * dt / H_CELL;
      out[AT(s, y, x)] = eo_interpolate(s, v, px, py, EO_V);
    }
}

void ar_advect_p(const eo_sim* s, const float* q, const float* u, const float* v, float dt, float* out, int rk2) {
  const float hdt = 0.5f * dt;
  for (int y = 0; y < s->Y; ++y)
    for (int x = 0; x < s->X; ++x) {
      if (!s->count[AT(s, y, x)]) continue;
      float dy = (v[AT(s, y, x)] + v[AT(s, y - 1, x)]) / 2;
      float dx = (u[AT(s, y, x)] + u[AT(s, y, x - 1)]) / 2;
      if (rk2) {
        float mx = x - dx * hdt / H_CELL, my = y - dy * hdt / H_CELL;
        dx = eo_interpolate(s, u, mx - 0.5f, my, EO_U);
        dy = eo_interpolate(s, v, mx, my - 0.5f, EO_V);
      }
      float px = x - dx * dt / H_CELL, py = y - dy * dt / H_CELL;
      out[AT(s, y, x)] = eo_interpolate(s, q, px, py, EO_P);
    }
}

static inline float time_to(float p0, float p1, float vel) {
  return fabsf(vel) > 0.f ? (p1 - p0) / vel : FLT_MAX;
}

/* eo_advect_markers statement for statement, the dt chain included (dt -= t_prev on the parameter,
 * main.c:501,518); the midpoint always uses the substep's dt (hdt), never the shortened one.
 * Returns the number of collisions that shortened dt. */
int ar_advect_markers(eo_sim* s, float dt, int rk2) {
  const float hdt = 0.5f * dt;
  int events = 0;
  for (size_t m = 0; m < s->n_markers; ++m) {
    float px = s->markers[m].x, py = s->markers[m].y;
    float vx = eo_interpolate(s, s->u, px / H_CELL - 1.f, py / H_CELL - 0.5f, EO_U);
    float vy = eo_interpolate(s, s->v, px / H_CELL - 0.5f, py / H_CELL - 1.f, EO_V);
    if (rk2) {
      float mx = px + hdt * vx, my = py + hdt * vy;
      vx = eo_interpolate(s, s->u, mx / H_CELL - 1.f, my / H_CELL - 0.5f, EO_U);
      vy = eo_interpolate(s, s->v, mx / H_CELL - 0.5f, my / H_CELL - 1.f, EO_V);
    }
    int xi = (int)floorf(px / H_CELL), yi = (int)floorf(py / H_CELL);

    int xdir = vx > 0 ? 1 : -1, nxi = xi + (vx > 0 ? 1 : 0);
    float npx = nxi * H_CELL;
    float tx = time_to(px, npx, vx);
    int xoff = vx < 0 ? -1 : 0;

    int ydir = vy > 0 ? 1 : -1, nyi = yi + (vy > 0 ? 1 : 0);
    float npy = nyi * H_CELL;
    float ty = time_to(py, npy, vy);
    int yoff = vy < 0 ? -1 : 0;

    float t_prev = 0.f, t_near = fminf(tx, ty);
    while (t_near < dt) {
      if (tx < ty) {
        if (s->solid[AT(s, yi, nxi + xoff)]) {
          if (t_prev > 0.f) events++;
          px = px + t_prev * vx; py = py + t_prev * vy;
          dt -= t_prev; t_near = 0; vx = 0.f; tx = FLT_MAX;
          ty = time_to(py, npy, vy);
        } else {
          xi = nxi; nxi = xi + xdir; npx = nxi * H_CELL;
          tx = time_to(px, npx, vx);
        }
      } else {
        if (s->solid[AT(s, nyi + yoff, xi)]) {
          if (t_prev > 0.f) events++;
          px = px + t_prev * vx; py = py + t_prev * vy;
          dt -= t_prev; t_near = 0; vy = 0.f; ty = FLT_MAX;
          tx = time_to(px, npx, vx);
        } else {
          yi = nyi; nyi = yi + ydir; npy = nyi * H_CELL;
          ty = time_to(py, npy, vy);
        }
      }
      t_prev = t_near;
      t_near = fminf(tx, ty);
    }
    float t = (t_near < FLT_MAX) ? dt : t_prev;
    s->markers[m].x = px + t * vx;
    s->markers[m].y = py + t * vy;
  }
  return events;
}
