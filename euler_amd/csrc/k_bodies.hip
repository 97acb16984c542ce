// k_bodies.hip — euler_set_bodies (include/euler.h, docs/bodies.md): solid rectangles of whole cells that move through the water on a prescribed path.
//
// Everything about the path is host arithmetic in double (euler_body_at, euler_host.c): the device only ever sees whole-cell origins and two floats of wall
// velocity per body.  Three pieces, all on the handle's stream:
//   push    k_body_push, one launch per unit shift and only in a substep where some body shifts: the one pass over the marker array.  Two markers per lane as one
//           16-byte load (k_edit_markers' layout); a marker in the strip ahead of the moving face takes fl(coordinate +- 1.f) and keeps its place in the array;
//           a lane without such a marker stores nothing, so a wave without one leaves after its load.
//   masks   the strip ahead becomes solid, the strip behind is cleared, and behind the last shift every rectangle is made solid again: the cell pass of
//           euler_edit_box itself (k_edit_cells: a dword per four cells where X % 4 == 0, the bytes an edge cuts left alone), in the marker stage's profile class.
//   faces   k_body_faces, one launch for all bodies in front of eu_launch_project and one behind it: a thread owns one perimeter face of one body and walks ALL
//           bodies in list order, so the value a shared face ends up with is the list order's whatever the geometry; two threads that own the same face (two
//           bodies' perimeters meet there) compute and store the same word.  The ≤ 16 records travel by value in the kernel's arguments.
// No atomics, no inline assembly.  A face is written only where its outside cell has the typed fluid property (count != 0 && !solid) and is set back to zero by the
// second launch: outside EULER_STAGE_PROJECT utmp / vtmp are zero wherever that property does not hold, as utmp_clean promises (docs/stage_validity.md).
#include "euler_dev.h"
#include "euler_host.h"

#include <math.h>
#include <string.h>

#include <vector>

int eu_pressure_current(euler_sim* S);                                        // k_grid.hip
int eu_set_source_count(euler_sim* S, size_t nsrc);                           // driver.hip

static_assert(sizeof(euler_body) == 64 && offsetof(euler_body, x) == 0 && offsetof(euler_body, y) == 8 && offsetof(euler_body, hz) == 16 && offsetof(euler_body, phase) == 24 &&
              offsetof(euler_body, vx) == 32 && offsetof(euler_body, vy) == 36 && offsetof(euler_body, amp_x) == 40 && offsetof(euler_body, amp_y) == 44 &&
              offsetof(euler_body, w) == 48 && offsetof(euler_body, h) == 52 && offsetof(euler_body, reserved) == 56, "euler_body is 64 bytes without padding");
static_assert(sizeof(euler_body_state) == 24 && offsetof(euler_body_state, ox) == 16 && offsetof(euler_body_state, oy) == 20, "euler_body_state is 24 bytes");

// ---- push: the markers of the strip [lo, lo + 1) along `axis`, [c0, c1) across it, move by d = +-1.f along the axis.  floorf(a) == k is k <= a < k + 1 for the
// integers below 2^24 a grid has; a NaN is in no strip.
__device__ __forceinline__ bool bd_hit(float a, float c, float lo, float c0, float c1) { return a >= lo && a < lo + 1.f && c >= c0 && c < c1; }

template <int AXIS>
__global__ __launch_bounds__(256) void k_body_push(float4* __restrict__ m2, unsigned long long n, float lo, float c0, float c1, float d) {
  const unsigned long long j = (unsigned long long)blockIdx.x * 256 + threadIdx.x, i0 = 2ull * j;
  if (i0 + 1ull < n) {
    float4 p = m2[j];
    const bool h0 = AXIS == 0 ? bd_hit(p.x, p.y, lo, c0, c1) : bd_hit(p.y, p.x, lo, c0, c1);
    const bool h1 = AXIS == 0 ? bd_hit(p.z, p.w, lo, c0, c1) : bd_hit(p.w, p.z, lo, c0, c1);
    if (!(h0 | h1)) return;
    if (AXIS == 0) { if (h0) p.x += d; if (h1) p.z += d; }
    else           { if (h0) p.y += d; if (h1) p.w += d; }
    m2[j] = p;      // (both markers are this lane's own: the one that was not hit gets its own bits back)
  } else if (i0 < n) {      // an odd count: the last marker alone
    float2* m = reinterpret_cast<float2*>(m2);
    float2 p = m[i0];
    if (!(AXIS == 0 ? bd_hit(p.x, p.y, lo, c0, c1) : bd_hit(p.y, p.x, lo, c0, c1))) return;
    if (AXIS == 0) p.x += d; else p.y += d;
    m[i0] = p;
  }
}

// ---- faces
struct BdRec { int ox, oy, w, h; float wx, wy; };
struct BdRecs { int n, total; int first[EULER_BODIES_MAX + 1]; BdRec r[EULER_BODIES_MAX]; };      // first[k]: the index of body k's first face among all perimeter faces

__global__ __launch_bounds__(256) void k_body_faces(float* __restrict__ utmp, float* __restrict__ vtmp, const uint8_t* __restrict__ count, const uint8_t* __restrict__ solid,
                                                    int X, BdRecs B, int impose) {
  const int t = (int)(blockIdx.x * 256 + threadIdx.x);
  if (t >= B.total) return;
  int own = 0;
  while (own + 1 < B.n && t >= B.first[own + 1]) ++own;      // (uniform bounds, at most 15 steps)
  const eu_body_face f = eu_body_face_at(B.r[own].ox, B.r[own].oy, B.r[own].w, B.r[own].h, t - B.first[own]);
  // every body that has this face on its perimeter, in list order: the last one whose rule fires decides
  bool fire = false;
  float val = 0.f;
  for (int k = 0; k < B.n; ++k) {
    const BdRec q = B.r[k];
    const float wv = f.axis == 0 ? q.wx : q.wy;
    if (wv == 0.f) continue;
    int cx, cy;      // the cell outside body k across the face, if the face is on k's perimeter
    if (f.axis == 0) {
      if (f.fy < q.oy || f.fy > q.oy + q.h - 1) continue;
      if (f.fx == q.ox - 1) cx = q.ox - 1; else if (f.fx == q.ox + q.w - 1) cx = q.ox + q.w; else continue;
      cy = f.fy;
    } else {
      if (f.fx < q.ox || f.fx > q.ox + q.w - 1) continue;
      if (f.fy == q.oy - 1) cy = q.oy - 1; else if (f.fy == q.oy + q.h - 1) cy = q.oy + q.h; else continue;
      cx = f.fx;
    }
    const size_t c = (size_t)cy * (size_t)X + (size_t)cx;      // (inside [1, X - 2] x [1, Y - 2]: the clamp of euler_body_at)
    if (count[c] != 0 && solid[c] == 0) { fire = true; val = wv; }
  }
  if (!fire) return;
  const size_t i = (size_t)f.fy * (size_t)X + (size_t)f.fx;
  (f.axis == 0 ? utmp : vtmp)[i] = impose ? val : 0.f;
}

// the substep's wall velocity of body k: the mean velocity over [t, t + dt], so that velocity x time is the displacement; 0 while the body is clamped
static void bd_wall_velocity(const euler_sim* S, int k, float dt, float* wx, float* wy) {
  euler_body_state a, b;
  (void)euler_body_at(&S->bodies[k], S->time, S->X, S->Y, &a);
  (void)euler_body_at(&S->bodies[k], S->time + (double)dt, S->X, S->Y, &b);
  *wx = (float)((b.px - a.px) / (double)dt);
  *wy = (float)((b.py - a.py) / (double)dt);
}

int eu_launch_body_faces(euler_sim* S, float dt, int impose) {
  if (S->n_bodies < 1 || !(dt > 0.f)) return EULER_OK;
  BdRecs B;
  memset(&B, 0, sizeof B);
  B.n = S->n_bodies;
  bool any = false;
  for (int k = 0; k < B.n; ++k) {
    B.first[k] = B.total;
    B.r[k] = BdRec{S->body_ox[k], S->body_oy[k], S->bodies[k].w, S->bodies[k].h, 0.f, 0.f};
    bd_wall_velocity(S, k, dt, &B.r[k].wx, &B.r[k].wy);
    if (!isfinite(B.r[k].wx)) B.r[k].wx = 0.f;      // (a dt so small that the quotient overflows: no wall velocity rather than an infinite one)
    if (!isfinite(B.r[k].wy)) B.r[k].wy = 0.f;
    any |= B.r[k].wx != 0.f || B.r[k].wy != 0.f;
    B.total += eu_body_nfaces(B.r[k].w, B.r[k].h);
  }
  B.first[B.n] = B.total;
  if (!any) return EULER_OK;      // every body at rest: walls, nothing to launch
  LAUNCH(S, KC_BUILD_SYSTEM, k_body_faces, dim3(eu_blocks((size_t)B.total, 256)), dim3(256), S->utmp, S->vtmp, S->count, S->solid, S->X, B, impose);
  HIPCHK(hipGetLastError());
  return EULER_OK;
}

// ---- the unit shifts of a substep
static int bd_push(euler_sim* S, const int fill[4], eu_body_shift s) {
  const unsigned long long n = S->n_markers_host;
  if (!n) return EULER_OK;
  float4* m2 = reinterpret_cast<float4*>(S->markers[S->cur]);
  const dim3 grid(eu_blocks((size_t)((n + 1) / 2), 256));
  if (s.axis == 0) LAUNCH(S, KC_MARKER_ADVECT, k_body_push<0>, grid, dim3(256), m2, n, (float)fill[0], (float)fill[1], (float)(fill[3] + 1), (float)s.dir);
  else             LAUNCH(S, KC_MARKER_ADVECT, k_body_push<1>, grid, dim3(256), m2, n, (float)fill[1], (float)fill[0], (float)(fill[2] + 1), (float)s.dir);
  HIPCHK(hipGetLastError());
  return EULER_OK;
}

int eu_launch_bodies_shift(euler_sim* S, float dt) {
  if (S->n_bodies < 1) return EULER_OK;
  int32_t tx[EULER_BODIES_MAX], ty[EULER_BODIES_MAX];
  bool any = false;
  for (int k = 0; k < S->n_bodies; ++k) {
    euler_body_state st;
    (void)euler_body_at(&S->bodies[k], S->time + (double)dt, S->X, S->Y, &st);
    tx[k] = st.ox; ty[k] = st.oy;
    any |= tx[k] != S->body_ox[k] || ty[k] != S->body_oy[k];
  }
  if (!any) return EULER_OK;
  int rc = eu_pressure_current(S);      // an edit's obligations (k_edit.hip): the pending pressure is finished from the solver's arrays as they stand ...
  if (rc) return rc;
  eu_vd_masks_changed(&S->vd);          // ... and nothing one stage prepared for the next describes the masks, the counts or the markers any more
  for (int k = 0; k < S->n_bodies; ++k) {
    const int w = S->bodies[k].w, h = S->bodies[k].h;
    // the unit shifts of this body, x first then y: at most two per axis under the speed bound, as many as it takes behind a caller who moved the clock
    std::vector<eu_body_shift> plan((size_t)eu_body_plan(S->body_ox[k], S->body_oy[k], tx[k], ty[k], nullptr, 0));
    (void)eu_body_plan(S->body_ox[k], S->body_oy[k], tx[k], ty[k], plan.data(), (int64_t)plan.size());
    for (const eu_body_shift s : plan) {
      int fill[4], clear[4];
      eu_body_strips(S->body_ox[k], S->body_oy[k], w, h, s, fill, clear);
      if ((rc = bd_push(S, fill, s))) return rc;
      if (S->n_source_cells) {      // the strip may cover source cells: the source stage's cell count follows (a handle without source cells reads nothing back)
        size_t covered = 0;
        if ((rc = eu_edit_source_census(S, KC_MARKER_ADVECT, fill[0], fill[1], fill[2], fill[3], &covered))) return rc;
        if (covered && (rc = eu_set_source_count(S, S->n_source_cells - covered))) return rc;
      }
      if ((rc = eu_edit_cells_box(S, KC_MARKER_ADVECT, EULER_EDIT_SOLID, fill[0], fill[1], fill[2], fill[3]))) return rc;
      if ((rc = eu_edit_cells_box(S, KC_MARKER_ADVECT, EULER_EDIT_CLEAR, clear[0], clear[1], clear[2], clear[3]))) return rc;
      if (s.axis == 0) S->body_ox[k] += s.dir; else S->body_oy[k] += s.dir;
    }
  }
  for (int k = 0; k < S->n_bodies; ++k)      // one body's CLEAR cannot open another
    if ((rc = eu_edit_cells_box(S, KC_MARKER_ADVECT, EULER_EDIT_SOLID, S->body_ox[k], S->body_oy[k], S->body_ox[k] + S->bodies[k].w - 1, S->body_oy[k] + S->bodies[k].h - 1))) return rc;
  if (S->heat_on && (rc = eu_heat_dry(S))) return rc;      // (the cells the bodies emptied hold ambient, as every cell without markers: docs/heat.md)
  return EULER_OK;
}

// ---- the entry points
extern "C" int euler_set_bodies(euler_sim* S, const euler_body* bodies, int32_t n) {
  const char* who = "euler_set_bodies";
  if (!S) { eu_set_error("%s: null argument", who); return EULER_EINVAL; }
  if (S->slab_on) { eu_set_error("%s: not on a row-slab handle (solid cells are facts a slab only gets from a load)", who); return EULER_ESTATE; }
  if (!S->loaded) { eu_set_error("%s: no scenario loaded", who); return EULER_ESTATE; }
  char why[256];
  if (eu_body_check(bodies, n, S->X, S->Y, why, sizeof why)) { eu_set_error("%s: %s", who, why); return EULER_EINVAL; }
  // the list it replaces: the rectangles are opened (the bodies are gone first, so that euler_edit_box does not refuse their own cells)
  const int n_old = S->n_bodies;
  S->n_bodies = 0;
  int rc = EULER_OK;
  for (int k = 0; k < n_old && !rc; ++k)
    rc = euler_edit_box(S, EULER_EDIT_CLEAR, S->body_ox[k], S->body_oy[k], S->body_ox[k] + S->bodies[k].w - 1, S->body_oy[k] + S->bodies[k].h - 1);
  for (int k = 0; k < n && !rc; ++k) {
    euler_body_state st;
    (void)euler_body_at(&bodies[k], S->time, S->X, S->Y, &st);
    S->body_ox[k] = st.ox; S->body_oy[k] = st.oy;
    rc = euler_edit_box(S, EULER_EDIT_SOLID, st.ox, st.oy, st.ox + bodies[k].w - 1, st.oy + bodies[k].h - 1);
  }
  if (rc) return rc;      // (a device failure: the handle has no bodies)
  if (n > 0) memcpy(S->bodies, bodies, (size_t)n * sizeof(euler_body));
  S->n_bodies = n;
  return EULER_OK;
}

extern "C" int euler_get_bodies(euler_sim* S, euler_body* bodies, int32_t cap, euler_body_state* now, int32_t* n) {
  if (!S || !n) { eu_set_error("euler_get_bodies: null argument"); return EULER_EINVAL; }
  if (bodies && cap < S->n_bodies) { eu_set_error("euler_get_bodies: room for %d bodies, %d set", cap, S->n_bodies); return EULER_EINVAL; }
  if (now && cap < S->n_bodies) { eu_set_error("euler_get_bodies: room for %d states, %d bodies set", cap, S->n_bodies); return EULER_EINVAL; }
  for (int k = 0; k < S->n_bodies; ++k) {
    if (bodies) bodies[k] = S->bodies[k];
    if (now) {
      (void)euler_body_at(&S->bodies[k], S->time, S->X, S->Y, &now[k]);
      now[k].ox = S->body_ox[k]; now[k].oy = S->body_oy[k];
    }
  }
  *n = S->n_bodies;
  return EULER_OK;
}
