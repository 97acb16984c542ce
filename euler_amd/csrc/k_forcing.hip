// k_forcing.hip — euler_set_forcing (include/euler.h, docs/forcing.md): the force boxes ("pumps") of a handle, the entry points of the forcing record and the clock.
//
// The uniform part of the forcing - gravity vector and shake - is an argument of the velocity advection's forced instantiations (k_grid.hip).  The boxes are this
// file: one launch per substep when the handle has boxes, inside eu_launch_advect_velocity, behind the advection and in front of the diffusion extension.
//
// The host checks the list and cuts it along the 64 x 64 tile grid into a tile table (eu_force_tiles, euler_host.c): one entry per tile that any box touches, with
// the boxes that touch it as a bit set.  Boxes and table go up once per euler_set_forcing.  One workgroup takes one tile; a thread owns 16 fixed cells of it (its
// column, every fourth row).  For each of its cells that lies in a box it loads the two faces, walks the tile's boxes from bit 0 up - the LIST order - adding
// fl(fx dt), fl(fy dt) in registers where the cell lies in the box and the face is live, and stores each face once.  No atomics, no two threads on one face:
// overlapping and repeated boxes add in list order whatever the launch geometry.
//
// A face is live as k_advect_velocity tests it, read off the row-major count / solid bytes as the FLUX gauge reads them; a box lies in the interior, so the
// second cells i + 1 and i + X lie in the grid.  Faces that are not live are neither read nor written: utmp / vtmp stay zero outside the typed fluid property, and
// nothing else is written - no validity flag changes (docs/stage_validity.md).  With the tile map a tile leaves at once when it, the tile right of it and the tile
// above it are dry: then no cell of it has a live face.
//
// Row slabs (docs/forcing.md "On row slabs"): a tile lies in one 64-row band, so each rank keeps the table entries of its own bands (eu_box_table_upload) and the
// kernel runs as it stands - global (x, y) through the window-shifted pointers, count[i + X] / solid[i + X] of the top row in the ghost rows, no tile map there.
// euler_set_forcing is collective on a slab handle: the ranks agree on the record and the list before anything changes (eu_slab_agree).
#include "k_observe.h"
#include "k_boxes.h"
#include "euler_host.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#define FO_T 256      // threads per workgroup: four waves, a wave along 64 columns

static_assert(sizeof(euler_force_box) == 24 && offsetof(euler_force_box, x0) == 0 && offsetof(euler_force_box, y0) == 4 && offsetof(euler_force_box, x1) == 8 &&
              offsetof(euler_force_box, y1) == 12 && offsetof(euler_force_box, fx) == 16 && offsetof(euler_force_box, fy) == 20, "euler_force_box is six 32-bit words");
static_assert(sizeof(euler_forcing) == 48 && offsetof(euler_forcing, gx) == 0 && offsetof(euler_forcing, gy) == 4 && offsetof(euler_forcing, shake_x) == 8 &&
              offsetof(euler_forcing, shake_y) == 12 && offsetof(euler_forcing, shake_hz) == 16 && offsetof(euler_forcing, shake_phase) == 24 &&
              offsetof(euler_forcing, nboxes) == 32 && offsetof(euler_forcing, reserved) == 36 && offsetof(euler_forcing, reserved2) == 40, "euler_forcing is 48 bytes without padding");
static_assert(sizeof(eu_force_tile) == 16, "a tile table entry is 16 bytes");
#define FO_BOX_BYTES (EULER_FORCE_BOXES_MAX * sizeof(euler_force_box))      // the boxes stand in front of the table (1536 bytes: the table stays 8-byte aligned)

__global__ __launch_bounds__(FO_T) void k_force_boxes(float* __restrict__ utmp, float* __restrict__ vtmp, const uint8_t* __restrict__ count, const uint8_t* __restrict__ solid,
                                                      int X, ObTiles tiles, const euler_force_box* __restrict__ boxes, const eu_force_tile* __restrict__ table, float dt) {
  const eu_force_tile t = table[blockIdx.x];      // (the tile, its boxes and every test on them are uniform across the workgroup)
  if (tiles.tmap && !tiles.wet(t.tx, t.ty) && !tiles.wet(t.tx + 1, t.ty) && !tiles.wet(t.tx, t.ty + 1)) return;      // (the map carries a ring of zeros right of and above the grid)
  const int x = t.tx * 64 + (int)(threadIdx.x & 63);
  for (int r = 0; r < 64 / (FO_T / 64); ++r) {
    const int y = t.ty * 64 + r * (FO_T / 64) + (int)(threadIdx.x >> 6);
    if (!eu_boxes_hold(boxes, t.boxes, x, y)) continue;
    const size_t i = (size_t)y * (size_t)X + (size_t)x;
    const bool cn = count[i] != 0, so = solid[i] != 0;
    const bool live_u = (cn | (count[i + 1] != 0)) && !(so | (solid[i + 1] != 0));
    const bool live_v = (cn | (count[i + X] != 0)) && !(so | (solid[i + X] != 0));
    if (!live_u && !live_v) continue;
    float fu = live_u ? utmp[i] : 0.f, fv = live_v ? vtmp[i] : 0.f;
    for (unsigned long long m = t.boxes; m; m &= m - 1) {      // bit 0 first: the list order
      const euler_force_box b = boxes[__ffsll((long long)m) - 1];
      if (x < b.x0 || x > b.x1 || y < b.y0 || y > b.y1) continue;
      fu += b.fx * dt;      // (the product rounded, then the add: the library is built without contraction)
      fv += b.fy * dt;
    }
    if (live_u) utmp[i] = fu;
    if (live_v) vtmp[i] = fv;
  }
}

int eu_launch_force_boxes(euler_sim* S, float dt) {
  if (S->forcing.nboxes < 1 || !S->force_ntiles) return EULER_OK;
  const euler_force_box* boxes = (const euler_force_box*)S->force_buf.p;
  const eu_force_tile* table = (const eu_force_tile*)((const char*)S->force_buf.p + FO_BOX_BYTES);
  LAUNCH(S, KC_ADVECT_VELOCITY, k_force_boxes, dim3(S->force_ntiles), dim3(FO_T), S->utmp, S->vtmp, S->count, S->solid, S->X, eu_observe_tiles(S), boxes, table, dt);
  HIPCHK(hipGetLastError());
  return EULER_OK;
}

extern "C" int euler_set_forcing(euler_sim* S, const euler_forcing* f, const euler_force_box* boxes) {
  const char* who = "euler_set_forcing";
  if (!S || !f) { eu_set_error("%s: null argument", who); return EULER_EINVAL; }
  if (S->slab_on && !S->has_comm) { eu_set_error("%s: row-slab handle without a communicator", who); return EULER_ESTATE; }      // (collective there: the ranks agree on the record)
  if (!S->loaded) { eu_set_error("%s: no scenario loaded", who); return EULER_ESTATE; }
  char why[256];
  int rc = EULER_OK;
  if (eu_forcing_check(f, boxes, S->X, S->Y, why, sizeof why)) { eu_set_error("%s: %s", who, why); rc = EULER_EINVAL; }
  // a slab handle: every rank takes part in the comparison, whatever its own check said; nothing has changed yet (docs/forcing.md "On row slabs")
  if (S->slab_on) rc = eu_slab_agree(S, who, rc, rc ? 0ull : eu_forcing_digest(f, boxes));
  if (rc) return rc;
  unsigned int ntiles = 0;      // (a slab handle keeps the table entries of its own bands; force_ntiles == 0: this rank launches nothing)
  if (f->nboxes > 0) rc = eu_box_table_upload(S, who, &S->force_buf, boxes, f->nboxes, sizeof(euler_force_box), EULER_FORCE_BOXES_MAX, &ntiles);
  // a slab handle: a rank that alone could not hold its table must not go on with the old list beside neighbours that took the new one - the failure is every
  // rank's, and every rank is left WITHOUT boxes (the buffers of those that succeeded already hold the new table; the record stays the old one otherwise)
  if (S->slab_on && (rc = eu_slab_all_ok(S, who, rc))) { S->forcing.nboxes = 0; S->force_ntiles = 0; }
  if (rc) return rc;
  S->force_ntiles = ntiles;
  if (f->nboxes > 0) memcpy(S->force_boxes, boxes, (size_t)f->nboxes * sizeof(euler_force_box));
  S->forcing = *f;
  S->force_uniform = !(f->gx == 0.f && f->gy == EU_G && f->shake_x == 0.f && f->shake_y == 0.f);      // the reference's (0, k_gravity): the kernels a handle always ran
  return EULER_OK;
}

extern "C" int euler_get_forcing(euler_sim* S, euler_forcing* f, euler_force_box* boxes, int32_t cap) {
  if (!S || !f) { eu_set_error("euler_get_forcing: null argument"); return EULER_EINVAL; }
  if (boxes && cap < S->forcing.nboxes) { eu_set_error("euler_get_forcing: room for %d boxes, %d set", cap, S->forcing.nboxes); return EULER_EINVAL; }
  *f = S->forcing;
  if (boxes && S->forcing.nboxes > 0) memcpy(boxes, S->force_boxes, (size_t)S->forcing.nboxes * sizeof(euler_force_box));
  return EULER_OK;
}

extern "C" int euler_get_time(euler_sim* S, double* t) {
  if (!S || !t) { eu_set_error("euler_get_time: null argument"); return EULER_EINVAL; }
  *t = S->time;
  return EULER_OK;
}

extern "C" int euler_set_time(euler_sim* S, double t) {
  if (!S) { eu_set_error("euler_set_time: null argument"); return EULER_EINVAL; }
  if (!isfinite(t)) { eu_set_error("euler_set_time: t must be finite"); return EULER_EINVAL; }
  S->time = t;
  return EULER_OK;
}
