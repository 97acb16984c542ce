/* advect_maccormack.c - test-side restatement of the MacCormack transport of EULER_OPT_ADVECT_MACCORMACK
 * (docs/advection_maccormack.md), on top of the oracle's exported eo_interpolate and eo_sim arrays.
 *
 * The traces are advect_rk2.c's (included here, unchanged) with a signed step: trace(+dt) is the product's
 * back-trace, trace(-dt) the same code with -dt.  Every function takes `mc`: 0 bypasses the correction, and
 * the function is then advect_rk2.c's stage statement for statement, which the host tests check bit for bit.
 * The limiter's corners restate eo_interpolate's clamp (nextafterf(extent - 1, 0)), its modff and its masks.
 *
 * Built at test time: gcc -O2 -ffp-contract=off -shared, linked against liboracle.so. */
#include <stdlib.h>
#include <string.h>

#include "advect_rk2.c"

static inline int ext_x(const eo_sim* s, int type) { return type == EO_U ? s->X - 1 : s->X; }
static inline int ext_y(const eo_sim* s, int type) { return type == EO_V ? s->Y - 1 : s->Y; }
static inline float clampf_(float lo, float x, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

/* the corners eo_interpolate(s, q, ix, iy, type) reads and its masks mark valid: their min and max (folded 00, 01, 10, 11 with strict
 * compares) and how many there are */
static int corners(const eo_sim* s, const float* q, float ix, float iy, int type, float* lo, float* hi) {
  ix = clampf_(0, ix, nextafterf((float)(ext_x(s, type) - 1), 0));
  iy = clampf_(0, iy, nextafterf((float)(ext_y(s, type) - 1), 0));
  float wx, wy;
  (void)modff(ix, &wx); (void)modff(iy, &wy);
  const int bx = (int)wx, by = (int)wy;
  const int xs[4] = {bx, bx + 1, bx, bx + 1}, ys[4] = {by, by, by + 1, by + 1};
  int n = 0;
  float l = INFINITY, h = -INFINITY;
  for (int k = 0; k < 4; ++k) {
    if (!prop(s, s->count, xs[k], ys[k], type)) continue;
    const float r = q[AT(s, ys[k], xs[k])];
    l = r < l ? r : l;
    h = r > h ? r : h;
    ++n;
  }
  *lo = l; *hi = h;
  return n;
}

static void trace_u(const eo_sim* s, const float* u, const float* v, int x, int y, float st, int rk2, float* px, float* py) {
  const float hdt = 0.5f * st;
  float dx = u[AT(s, y, x)];
  float dy = eo_interpolate(s, v, x + 0.5f, y - 0.5f, EO_V);
  if (rk2) {
    float mx = x - dx * hdt / H_CELL, my = y - dy * hdt / H_CELL;
    dx = eo_interpolate(s, u, mx, my, EO_U);
    dy = eo_interpolate(s, v, mx + 0.5f, my - 0.5f, EO_V);
  }
  *px = x - dx * st / H_CELL; *py = y - dy * st / H_CELL;
}

static void trace_v(const eo_sim* s, const float* u, const float* v, int x, int y, float st, int rk2, float* px, float* py) {
  const float hdt = 0.5f * st;
  float dy = v[AT(s, y, x)];
  float dx = eo_interpolate(s, u, x - 0.5f, y + 0.5f, EO_U);
  if (rk2) {
    float mx = x - dx * hdt / H_CELL, my = y - dy * hdt / H_CELL;
    dy = eo_interpolate(s, v, mx, my, EO_V);
    dx = eo_interpolate(s, u, mx - 0.5f, my + 0.5f, EO_U);
  }
  *px = x - dx * st / H_CELL; *py = y - dy * st / H_CELL;
}

static void trace_p(const eo_sim* s, const float* u, const float* v, int x, int y, float st, int rk2, float* px, float* py) {
  const float hdt = 0.5f * st;
  float dy = (v[AT(s, y, x)] + v[AT(s, y - 1, x)]) / 2;
  float dx = (u[AT(s, y, x)] + u[AT(s, y, x - 1)]) / 2;
  if (rk2) {
    float mx = x - dx * hdt / H_CELL, my = y - dy * hdt / H_CELL;
    dx = eo_interpolate(s, u, mx - 0.5f, my, EO_U);
    dy = eo_interpolate(s, v, mx, my - 0.5f, EO_V);
  }
  *px = x - dx * st / H_CELL; *py = y - dy * st / H_CELL;
}

/* steps 3 and 4 of the semantics */
static float correct(float f, float q0, float b, int n1, int n2, float lo, float hi) {
  if (!n1 || !n2) return f;
  float out = f + 0.5f * (q0 - b);
  return out < lo ? lo : (out > hi ? hi : out);
}

static int live(const eo_sim* s, int x, int y, int type) { return prop(s, s->count, x, y, type) && !prop(s, s->solid, x, y, type); }

/* advect_u (type EO_U) or advect_v (EO_V) without gravity: out is written where the face has the fluid property, like ar_advect_u / _v
 * (faces with the solid property keep the forward value: zero_bounds clears them).  lo / hi (may be NULL): the limiter's bounds per live face,
 * +inf / -inf where the forward interpolation found no valid corner, NaN on other faces */
static void advect_face(const eo_sim* s, const float* u, const float* v, float dt, float* out, int rk2, int mc, int type, float* lo, float* hi) {
  const int ex = ext_x(s, type), ey = ext_y(s, type);
  const float* q = type == EO_U ? u : v;
  const size_t C = (size_t)s->X * s->Y;
  float* fw = (float*)calloc(C, sizeof(float));      /* the grid of step-1 results: the forward value on live faces, 0 on every other */
  if (lo) for (size_t i = 0; i < C; ++i) { lo[i] = NAN; hi[i] = NAN; }
  for (int y = 0; y < ey; ++y)
    for (int x = 0; x < ex; ++x) {
      if (!prop(s, s->count, x, y, type)) continue;
      float px, py;
      if (type == EO_U) trace_u(s, u, v, x, y, dt, rk2, &px, &py);
      else trace_v(s, u, v, x, y, dt, rk2, &px, &py);
      const float f = eo_interpolate(s, q, px, py, type);
      out[AT(s, y, x)] = f;
      if (live(s, x, y, type)) fw[AT(s, y, x)] = f;
    }
  if (mc)
    for (int y = 0; y < ey; ++y)
      for (int x = 0; x < ex; ++x) {
        if (!live(s, x, y, type)) continue;
        float px, py, qx, qy, l, h, l2, h2;
        if (type == EO_U) { trace_u(s, u, v, x, y, dt, rk2, &px, &py); trace_u(s, u, v, x, y, -dt, rk2, &qx, &qy); }
        else { trace_v(s, u, v, x, y, dt, rk2, &px, &py); trace_v(s, u, v, x, y, -dt, rk2, &qx, &qy); }
        const int n1 = corners(s, q, px, py, type, &l, &h);
        const int n2 = corners(s, fw, qx, qy, type, &l2, &h2);
        const float b = eo_interpolate(s, fw, qx, qy, type);
        out[AT(s, y, x)] = correct(fw[AT(s, y, x)], q[AT(s, y, x)], b, n1, n2, l, h);
        if (lo) { lo[AT(s, y, x)] = l; hi[AT(s, y, x)] = h; }
      }
  free(fw);
}

void am_advect_u(const eo_sim* s, const float* u, const float* v, float dt, float* out, int rk2, int mc, float* lo, float* hi) {
  advect_face(s, u, v, dt, out, rk2, mc, EO_U, lo, hi);
}
void am_advect_v(const eo_sim* s, const float* u, const float* v, float dt, float* out, int rk2, int mc, float* lo, float* hi) {
  advect_face(s, u, v, dt, out, rk2, mc, EO_V, lo, hi);
}

/* advect_p + the whole-array memcpy (main.c:424-438, 875-881) of one channel: tmp takes the forward result on fluid cells (the rest of it keeps
 * its content), q the corrected value on fluid cells and tmp's value on every other.  lo / hi as above, per fluid cell */
void am_advect_p(const eo_sim* s, float* q, const float* u, const float* v, float dt, float* tmp, int rk2, int mc, float* lo, float* hi) {
  const size_t C = (size_t)s->X * s->Y;
  if (lo) for (size_t i = 0; i < C; ++i) { lo[i] = NAN; hi[i] = NAN; }
  for (int y = 0; y < s->Y; ++y)
    for (int x = 0; x < s->X; ++x) {
      if (!s->count[AT(s, y, x)]) continue;
      float px, py;
      trace_p(s, u, v, x, y, dt, rk2, &px, &py);
      tmp[AT(s, y, x)] = eo_interpolate(s, q, px, py, EO_P);
    }
  float* res = (float*)malloc(C * sizeof(float));
  memcpy(res, tmp, C * sizeof(float));
  if (mc)
    for (int y = 0; y < s->Y; ++y)
      for (int x = 0; x < s->X; ++x) {
        if (!s->count[AT(s, y, x)]) continue;
        float px, py, qx, qy, l, h, l2, h2;
        trace_p(s, u, v, x, y, dt, rk2, &px, &py);
        trace_p(s, u, v, x, y, -dt, rk2, &qx, &qy);
        const int n1 = corners(s, q, px, py, EO_P, &l, &h);
        const int n2 = corners(s, tmp, qx, qy, EO_P, &l2, &h2);
        const float b = eo_interpolate(s, tmp, qx, qy, EO_P);
        res[AT(s, y, x)] = correct(tmp[AT(s, y, x)], q[AT(s, y, x)], b, n1, n2, l, h);
        if (lo) { lo[AT(s, y, x)] = l; hi[AT(s, y, x)] = h; }
      }
  memcpy(q, res, C * sizeof(float));
  free(res);
}
