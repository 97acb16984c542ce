// k_heat.hip — euler_set_heat (include/euler.h, docs/heat.md): a temperature the flow carries, that boxes heat or cool, that diffuses and that makes water lighter
// or heavier.  The passes of a substep, the entry points of the record and of the field.
//
// T is one float per cell, row-major, cell-centred like the dye; a cell is fluid when its count is not 0.  Behind every completed substep a cell without markers
// holds `ambient`: the passes that write every cell (extension, transport, diffusion) say so for the dry ones, and they go from one half of heat_buf to the other
// - S->heat_cur says which half holds T -, so none of them reads what another thread of the same launch writes:
//   EULER_STAGE_SOURCES          k_heat_extend     the dye's extrapolate(q, P) for one channel with ambient where no neighbour was fluid, then the source cells
//   EULER_STAGE_ADVECT_VELOCITY  k_heat_advect     the dye's advect_p for one channel (RK2: the midpoint trace); dry cells take ambient.  MacCormack: the forward
//                                                  result of the fluid cells into mc_u (free between the velocity's correction and the next substep), then
//                                k_heat_correct    k_mc_correct_dye for one channel; dry cells take ambient
//                                k_heat_boxes      nboxes > 0: FIX and RATE boxes in list order, the force boxes' scheme - one workgroup per 64 x 64 tile that any box
//                                                  touches, the tile's boxes as a bit set walked from bit 0, a thread owns its 16 cells: no atomics, in place
//                                k_heat_diffuse    kappa > 0: k_diffuse_velocity's arithmetic over fluid neighbours; dry cells take ambient
//                                k_heat_buoyancy   beta != 0: live faces of utmp / vtmp only - what the advection leaves for the next pass stands, no validity flag
//                                                  changes (docs/stage_validity.md)
// Boxes and diffusion touch fluid cells and read fluid neighbours only, so the dry cells' ambient may come with the transport.  No pass here consults the tile map:
// EULER_OPT_NO_TILE_MAP cannot change a bit.
#include "k_observe.h"
#include "k_transport.h"
#include "k_boxes.h"
#include "euler_host.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

static_assert(sizeof(euler_heat_box) == 24 && offsetof(euler_heat_box, x0) == 0 && offsetof(euler_heat_box, y0) == 4 && offsetof(euler_heat_box, x1) == 8 &&
              offsetof(euler_heat_box, y1) == 12 && offsetof(euler_heat_box, value) == 16 && offsetof(euler_heat_box, kind) == 20, "euler_heat_box is six 32-bit words");
static_assert(sizeof(euler_heat) == 32 && offsetof(euler_heat, ambient) == 0 && offsetof(euler_heat, beta) == 4 && offsetof(euler_heat, kappa) == 8 &&
              offsetof(euler_heat, source_t) == 12 && offsetof(euler_heat, nboxes) == 16 && offsetof(euler_heat, reserved) == 20 && offsetof(euler_heat, reserved2) == 24,
              "euler_heat is 32 bytes without padding");
#define HE_BOX_BYTES (EULER_HEAT_BOXES_MAX * sizeof(euler_heat_box))      // the boxes stand in front of the table (1536 bytes: the table stays 8-byte aligned)

// every cell takes val (switching on, a load)
__global__ __launch_bounds__(256) void k_heat_set(float* __restrict__ t, size_t n, float val) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) t[i] = val;
}
// euler_heat_set_field: the caller's values where a cell holds markers, ambient elsewhere
__global__ __launch_bounds__(256) void k_heat_mask(const float* __restrict__ src, float* __restrict__ t, const uint8_t* __restrict__ count, size_t n, float ambient) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) t[i] = count[i] ? src[i] : ambient;
}

// extrapolate(q, P) for T (k_extrapolate_dye's sum: y-major then x, divided by the number of terms), ambient where no neighbour was fluid; then the source cells.
// Out of place: a source cell that was fluid is read by its new neighbours with the value it had
__global__ __launch_bounds__(256) void k_heat_extend(const float* __restrict__ tin, float* __restrict__ tout, const uint8_t* __restrict__ prev, const uint8_t* __restrict__ cur,
                                                     const uint8_t* __restrict__ source, int X, int Y, float ambient, float source_t, int ya, int yb) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = ya + blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= X || y >= yb) return;
  const size_t i = (size_t)y * X + x;
  float r;
  if (source[i]) r = source_t;
  else if (prev[i] || !cur[i]) r = tin[i];
  else {
    const int x0 = x > 0 ? x - 1 : 0, x1 = x + 1 < X ? x + 1 : X - 1;
    const int y0 = y > 0 ? y - 1 : 0, y1 = y + 1 < Y ? y + 1 : Y - 1;
    float t = 0.f;
    int n = 0;
    for (int yy = y0; yy <= y1; ++yy)
      for (int xx = x0; xx <= x1; ++xx) {
        const size_t j = (size_t)yy * X + xx;
        if (prev[j]) { t += tin[j]; ++n; }
      }
    r = n ? t / n : ambient;
  }
  tout[i] = r;
}

// advect_p for T (k_advect_dye's trace and interpolation).  FWD: the forward pass of MacCormack - fluid cells only, into the scratch the correction reads under the
// count masks; else every cell is written, the dry ones with ambient
template <bool RK2, bool FWD>
__global__ __launch_bounds__(256) void k_heat_advect(const float* __restrict__ tin, float* __restrict__ tout, const float* __restrict__ u, const float* __restrict__ v,
                                                     GridRef gr, float dt, float ambient, int ya, int yb) {
  const int X = gr.X;
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = ya + blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= X || y >= yb) return;
  const size_t i = (size_t)y * X + x;
  if (!gr.count[i]) {                            // never fluid on the border ring (all sink): i - X, i - 1 exist below
    if (!FWD) tout[i] = ambient;
    return;
  }
  const float dy = (v[i] + v[i - X]) / 2;
  const float dx = (u[i] + u[i - 1]) / 2;
  const EuTrace t = eu_trace<EU_SPACE_P, RK2, false>(gr, u, v, (float)x, (float)y, dx, dy, dt);
  tout[i] = eu_interp<0>(gr, tin, t.px, t.py);
}

// k_mc_correct_dye for T: q the field, qf its forward result; dry cells take ambient
template <bool RK2>
__global__ __launch_bounds__(256) void k_heat_correct(const float* __restrict__ q, const float* __restrict__ qf, float* __restrict__ out, const float* __restrict__ u,
                                                      const float* __restrict__ v, GridRef gr, float dt, float ambient) {
  const int X = gr.X;
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= X || y >= gr.Y) return;
  const size_t i = (size_t)y * X + x;
  if (!gr.count[i]) { out[i] = ambient; return; }
  const float dy = (v[i] + v[i - X]) / 2;
  const float dx = (u[i] + u[i - 1]) / 2;
  const EuTrace t = eu_trace<EU_SPACE_P, RK2, true>(gr, u, v, (float)x, (float)y, dx, dy, dt);
  out[i] = eu_mc_value<0>(gr, q, qf, q[i], t);
}

// the boxes: one workgroup per table entry, a thread owns its column's every fourth row of the tile.  A cell in some box of the tile lies in the interior
__global__ __launch_bounds__(256) void k_heat_boxes(float* __restrict__ t, const uint8_t* __restrict__ count, int X, const euler_heat_box* __restrict__ boxes,
                                                    const eu_force_tile* __restrict__ table, float dt) {
  const eu_force_tile e = table[blockIdx.x];      // (the tile, its boxes and every test on them are uniform across the workgroup)
  const int x = e.tx * 64 + (int)(threadIdx.x & 63);
  for (int r = 0; r < 16; ++r) {
    const int y = e.ty * 64 + r * 4 + (int)(threadIdx.x >> 6);
    if (!eu_boxes_hold(boxes, e.boxes, x, y)) continue;
    const size_t i = (size_t)y * (size_t)X + (size_t)x;
    if (!count[i]) continue;
    float q = t[i];
    for (unsigned long long m = e.boxes; m; m &= m - 1) {      // bit 0 first: the list order
      const euler_heat_box b = boxes[__ffsll((long long)m) - 1];
      if (x < b.x0 || x > b.x1 || y < b.y0 || y > b.y1) continue;
      q = b.kind == EULER_HEAT_FIX ? b.value : q + b.value * dt;      // (the product rounded, then the add: the library is built without contraction)
    }
    t[i] = q;
  }
}

// one explicit diffusion step over the fluid cells, k_diffuse_velocity's arithmetic: Jacobi from tin; solids and air are insulated; dry cells take ambient
__global__ __launch_bounds__(256) void k_heat_diffuse(const float* __restrict__ tin, float* __restrict__ tout, const uint8_t* __restrict__ count, int X, float c,
                                                      float ambient, int ya, int yb) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = ya + blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= X || y >= yb) return;
  const size_t i = (size_t)y * X + x;
  if (!count[i]) { tout[i] = ambient; return; }      // (never fluid on the border ring: the four neighbours exist)
  const float q = tin[i];
  float acc = 0.f;
  if (count[i - 1]) acc += tin[i - 1] - q;
  if (count[i + 1]) acc += tin[i + 1] - q;
  if (count[i - X]) acc += tin[i - X] - q;
  if (count[i + X]) acc += tin[i + X] - q;
  tout[i] = q + c * acc;
}

// Boussinesq: a live face (k_force_boxes' test) whose temperature differs from ambient gets -beta (Tf - ambient) a dt; ax == 0 leaves the u faces alone
__global__ __launch_bounds__(256) void k_heat_buoyancy(const float* __restrict__ t, float* __restrict__ utmp, float* __restrict__ vtmp, const uint8_t* __restrict__ count,
                                                       const uint8_t* __restrict__ solid, int X, int Y, float ambient, float beta, float ax, float ay, float dt, int ya, int yb) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = ya + blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= X || y >= yb) return;
  const size_t i = (size_t)y * X + x;
  const bool cn = count[i] != 0, so = solid[i] != 0;
  if (y < Y - 1) {
    const bool c2 = count[i + X] != 0;
    if ((cn | c2) && !(so | (solid[i + X] != 0))) {
      const float tf = (cn && c2) ? (t[i] + t[i + X]) / 2.f : (cn ? t[i] : t[i + X]);
      const float d = tf - ambient;
      if (d != 0.f) { const float k = beta * d, g = ay * dt; vtmp[i] = vtmp[i] - k * g; }
    }
  }
  if (ax != 0.f && x < X - 1) {
    const bool c2 = count[i + 1] != 0;
    if ((cn | c2) && !(so | (solid[i + 1] != 0))) {
      const float tf = (cn && c2) ? (t[i] + t[i + 1]) / 2.f : (cn ? t[i] : t[i + 1]);
      const float d = tf - ambient;
      if (d != 0.f) { const float k = beta * d, g = ax * dt; utmp[i] = utmp[i] - k * g; }
    }
  }
}

// behind an edit: every cell without markers takes ambient (in place, a cell is its own thread's)
__global__ __launch_bounds__(256) void k_heat_dry(float* __restrict__ t, const uint8_t* __restrict__ count, size_t n, float ambient) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n && !count[i]) t[i] = ambient;
}

// euler_heat_raster, first launch: every record of the W x H raster with its cell count (euler_overview_box's pixel edges) and zeros.  A row slab: the Hl pixel
// rows from py0 on that this rank's rows [cy0, cy1] of the box touch, each with the cells of those rows only - the shares' counts add up to the whole-grid one
__global__ __launch_bounds__(256) void k_heat_ras_init(euler_heat_px* __restrict__ out, int W, int H, int Bw, int Bh, int Hl, int py0, int by1, int cy0, int cy1) {
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= (size_t)W * (size_t)Hl) return;
  const unsigned long long px = k % (unsigned int)W, py = (unsigned long long)py0 + k / (unsigned int)W;
  const unsigned int wpx = (unsigned int)((px + 1) * (unsigned int)Bw / (unsigned int)W) - (unsigned int)(px * (unsigned int)Bw / (unsigned int)W);
  const int ytop = by1 - (int)(py * (unsigned int)Bh / (unsigned int)H), ybot = by1 + 1 - (int)((py + 1) * (unsigned int)Bh / (unsigned int)H);      // the pixel row's cell rows
  const int yhi = ytop < cy1 ? ytop : cy1, ylo = ybot > cy0 ? ybot : cy0;
  const unsigned int hpx = yhi >= ylo ? (unsigned int)(yhi - ylo + 1) : 0u;
  euler_heat_px r;
  r.cells = wpx * hpx; r.water = 0u; r.t_pos = 0ull; r.t_neg = 0ull; r.max_above = 0.f; r.max_below = 0.f;
  out[k] = r;
}
// ... second launch: a thread per cell of the box, a wave along 64 columns; a water cell goes to the record of its pixel with integer adds and bit-pattern maxima
// (exact in any order).  qv is the flow raster's: min(a, 4096) 2^20, truncated; a NaN goes to no sum and no maximum
__global__ __launch_bounds__(256) void k_heat_raster(const float* __restrict__ t, const uint8_t* __restrict__ solid, const uint8_t* __restrict__ sink, const uint8_t* __restrict__ count,
                                                     euler_heat_px* __restrict__ out, int X, int bx0, int ry0, int nrows, int by1, int Bw, int Bh, int W, int H, int py0,
                                                     float ambient) {      // rows ry0 ... ry0 + nrows - 1 of the box (a row slab: the own ones), records from pixel row py0 on
  const int cx = blockIdx.x * 64 + (int)(threadIdx.x & 63), cy = blockIdx.y * 4 + (int)(threadIdx.x >> 6);
  if (cx >= Bw || cy >= nrows) return;
  const int x = bx0 + cx, y = ry0 + cy;
  const size_t i = (size_t)y * (size_t)X + (size_t)x;
  if (solid[i] || sink[i] || !count[i]) return;
  const int px = (int)(((unsigned long long)(cx + 1) * (unsigned int)W - 1ull) / (unsigned int)Bw);      // the pixel column whose range holds x ...
  const int py = (int)(((unsigned long long)(by1 - y + 1) * (unsigned int)H - 1ull) / (unsigned int)Bh);  // ... and the pixel row, counted from the top
  euler_heat_px* o = out + (size_t)(py - py0) * W + px;
  atomicAdd(&o->water, 1u);
  const float d = t[i] - ambient;
  if (d != d) return;
  const float a = d >= 0.f ? d : -d;
  const unsigned long long q = (unsigned long long)((a < 4096.f ? a : 4096.f) * 1048576.f);
  if (q) atomicAdd(reinterpret_cast<unsigned long long*>(d >= 0.f ? &o->t_pos : &o->t_neg), q);
  if (a > 0.f) atomicMax(reinterpret_cast<unsigned int*>(d >= 0.f ? &o->max_above : &o->max_below), __float_as_uint(a));
}
static_assert(sizeof(euler_heat_px) == 32 && offsetof(euler_heat_px, water) == 4 && offsetof(euler_heat_px, t_pos) == 8 && offsetof(euler_heat_px, t_neg) == 16 &&
              offsetof(euler_heat_px, max_above) == 24 && offsetof(euler_heat_px, max_below) == 28, "euler_heat_px is 32 bytes without padding");

// ------------------------------------------------------------------------------------------ the launchers
// The passes run over the handle's own rows [row_lo, row_hi) - the whole grid without slabs.  A half of heat_buf holds the window (own rows + ghost rows, Cw floats;
// the grid without slabs) and is addressed with GLOBAL (x, y) through a base shifted by win_off, like u (euler_dev.h).  On a row slab one ghost row of T below and
// one above the own rows hold the neighbours' current values behind every stage and every call that writes T (docs/heat.md "On row slabs"): eu_slab_exchange_heat
static inline dim3 heat_grid(const euler_sim* S) { return dim3((S->X + 63) / 64, (S->row_hi - S->row_lo + 3) / 4); }
static inline float* heat_half(const euler_sim* S, int k) { return (float*)S->heat_buf.p + (size_t)k * S->Cw - S->win_off; }
static inline float* heat_t(const euler_sim* S) { return heat_half(S, S->heat_cur); }
static inline float* heat_other(const euler_sim* S) { return heat_half(S, S->heat_cur ^ 1); }
static inline size_t heat_own0(const euler_sim* S) { return (size_t)S->row_lo * S->X; }                       // the first own cell ...
static inline size_t heat_own_n(const euler_sim* S) { return (size_t)(S->row_hi - S->row_lo) * S->X; }       // ... and how many there are
float* eu_heat_field(const euler_sim* S) { return heat_t(S); }      // (k_slab.hip: the field whose ghost rows travel)

int eu_heat_reset(euler_sim* S) {      // the whole window: the ghost rows hold ambient as the neighbours' rows do
  if (!S->heat_on) return EULER_OK;
  S->heat_cur = 0;
  S->heat_ghost_stale = 0;
  LAUNCH(S, KC_MISC, k_heat_set, dim3(eu_blocks(S->Cw, 256)), dim3(256), heat_t(S) + S->win_off, S->Cw, S->heat.ambient);
  HIPCHK(hipGetLastError());
  return EULER_OK;
}

int eu_heat_dry(euler_sim* S) {
  LAUNCH(S, KC_MISC, k_heat_dry, dim3(eu_blocks(heat_own_n(S), 256)), dim3(256), heat_t(S) + heat_own0(S), S->count + heat_own0(S), heat_own_n(S), S->heat.ambient);
  HIPCHK(hipGetLastError());
  return EULER_OK;
}

// (on a row slab: behind the exchange of the count grids that follows the sources - the 3 x 3 reads prev_count across the row edges -, and in front of T's)
int eu_launch_heat_sources(euler_sim* S) {
  LAUNCH(S, KC_EXTRAPOLATE, k_heat_extend, heat_grid(S), dim3(256), heat_t(S), heat_other(S), S->prev_count, S->count, S->source, S->X, S->Y, S->heat.ambient, S->heat.source_t,
         S->row_lo, S->row_hi);
  S->heat_cur ^= 1;
  S->heat_ghost_stale = 1;
  return EULER_OK;
}

static int heat_launch_boxes(euler_sim* S, int cls, const eu_devbuf* buf, unsigned int ntiles, float dt) {
  const euler_heat_box* boxes = (const euler_heat_box*)buf->p;
  const eu_force_tile* table = (const eu_force_tile*)((const char*)buf->p + HE_BOX_BYTES);
  LAUNCH(S, cls, k_heat_boxes, dim3(ntiles), dim3(256), heat_t(S), S->count, S->X, boxes, table, dt);
  HIPCHK(hipGetLastError());
  return EULER_OK;
}

int eu_launch_heat_advect(euler_sim* S, float dt, const float acc[2]) {
  const GridRef g = eu_grid_ref(S);
  const float amb = S->heat.ambient;
  // MacCormack: the forward result into mc_u (it came with the option), then the correction; else the one pass into the other half
  eu_flag(S->opt[EULER_OPT_ADVECT_RK2] != 0, [&](auto R) {
    eu_flag(S->opt[EULER_OPT_ADVECT_MACCORMACK] != 0, [&](auto M) {
      constexpr bool RK2 = decltype(R)::value, MC = decltype(M)::value;
      LAUNCH(S, KC_ADVECT_VELOCITY, (k_heat_advect<RK2, MC>), heat_grid(S), dim3(256), heat_t(S), MC ? S->mc_u : heat_other(S), S->u, S->v, g, dt, amb, S->row_lo, S->row_hi);
      if (MC) LAUNCH(S, KC_ADVECT_VELOCITY, k_heat_correct<RK2>, heat_grid(S), dim3(256), heat_t(S), S->mc_u, heat_other(S), S->u, S->v, g, dt, amb);      // (never on a row slab)
    });
  });
  S->heat_cur ^= 1;
  S->heat_ghost_stale = 1;
  // (a row slab: this rank's entries of the table - none when no box touches its bands)
  if (S->heat.nboxes > 0 && S->heat_ntiles) { int rc = heat_launch_boxes(S, KC_ADVECT_VELOCITY, &S->heat_box_buf, S->heat_ntiles, dt); if (rc) return rc; }
  // Row slabs: the diffusion reads T one row below and above the own rows, the buoyancy one row above - each behind an exchange of what the passes before it wrote,
  // and only then: with kappa == 0 and beta == 0 T's ghost rows travel with vtmp's, behind this stage (k_slab.hip)
  if (S->heat.kappa > 0.f) {
    if (S->slab_on) { int rc = eu_slab_exchange_heat(S); if (rc) return rc; }
    const float c = S->heat.kappa * dt;
    LAUNCH(S, KC_ADVECT_VELOCITY, k_heat_diffuse, heat_grid(S), dim3(256), heat_t(S), heat_other(S), S->count, S->X, c, amb, S->row_lo, S->row_hi);
    S->heat_cur ^= 1;
    S->heat_ghost_stale = 1;
  }
  if (S->heat.beta != 0.f) {
    if (S->slab_on) { int rc = eu_slab_exchange_heat(S); if (rc) return rc; }
    LAUNCH(S, KC_ADVECT_VELOCITY, k_heat_buoyancy, heat_grid(S), dim3(256), heat_t(S), S->utmp, S->vtmp, S->count, S->solid, S->X, S->Y, amb, S->heat.beta, acc[0], acc[1], dt,
           S->row_lo, S->row_hi);
  }
  HIPCHK(hipGetLastError());
  return EULER_OK;
}

// ------------------------------------------------------------------------------------------ the entry points
extern "C" int euler_set_heat(euler_sim* S, const euler_heat* h, const euler_heat_box* boxes) {
  const char* who = "euler_set_heat";
  if (!S) { eu_set_error("%s: null argument", who); return EULER_EINVAL; }
  if (S->slab_on && !S->has_comm) { eu_set_error("%s: row-slab handle without a communicator", who); return EULER_ESTATE; }      // (collective there: the ranks agree on the record)
  if (!S->loaded) { eu_set_error("%s: no scenario loaded", who); return EULER_ESTATE; }
  char why[320];
  int rc = EULER_OK;
  if (h && eu_heat_check(h, boxes, S->X, S->Y, S->heat_on ? &S->heat.ambient : nullptr, why, sizeof why)) { eu_set_error("%s: %s", who, why); rc = EULER_EINVAL; }
  // a slab handle: every rank takes part in the comparison, whatever its own check said, switching off included - a rank with heat off would skip an exchange its
  // neighbour waits in; nothing has changed yet (docs/heat.md "On row slabs")
  if (S->slab_on) rc = eu_slab_agree(S, who, rc, rc ? 0ull : eu_heat_digest(h, boxes));
  if (rc) return rc;
  if (!h) { S->heat_on = 0; return EULER_OK; }      // off: the buffers stay, the next switching-on starts from ambient
  rc = eu_devbuf_reserve(S, who, "the temperature and its scratch copy", &S->heat_buf, 2 * S->Cw * sizeof(float));      // (the window: the grid without slabs)
  unsigned int ntiles = 0;
  if (!rc && h->nboxes > 0) rc = eu_box_table_upload(S, who, &S->heat_box_buf, boxes, h->nboxes, sizeof(euler_heat_box), EULER_HEAT_BOXES_MAX, &ntiles);
  // a slab handle: a rank that alone could not reserve its buffers must not stay off beside neighbours that switch on and wait for it in T's exchange - the failure
  // is every rank's.  Heat stays on or off as it was, on every rank WITHOUT boxes (the buffers of the ranks that succeeded already hold the new table)
  if (S->slab_on && (rc = eu_slab_all_ok(S, who, rc))) { S->heat.nboxes = 0; S->heat_ntiles = 0; }
  if (rc) return rc;
  const int was_on = S->heat_on;
  S->heat = *h;
  S->heat_ntiles = ntiles;
  if (h->nboxes > 0) memcpy(S->heat_boxes, boxes, (size_t)h->nboxes * sizeof(euler_heat_box));
  S->heat_on = 1;
  if (!was_on && (rc = eu_heat_reset(S))) { S->heat_on = 0; return rc; }
  return EULER_OK;
}

extern "C" int euler_get_heat(euler_sim* S, euler_heat* h, euler_heat_box* boxes, int32_t cap) {
  if (!S || !h) { eu_set_error("euler_get_heat: null argument"); return EULER_EINVAL; }
  if (!S->heat_on) { eu_set_error("euler_get_heat: heat is off"); return EULER_ESTATE; }
  if (boxes && cap < S->heat.nboxes) { eu_set_error("euler_get_heat: room for %d boxes, %d set", cap, S->heat.nboxes); return EULER_EINVAL; }
  *h = S->heat;
  if (boxes && S->heat.nboxes > 0) memcpy(boxes, S->heat_boxes, (size_t)S->heat.nboxes * sizeof(euler_heat_box));
  return EULER_OK;
}

// the refusals the field calls share: a null argument, a slab handle, nothing loaded, heat off
static int heat_field_enter(euler_sim* S, const void* arg, const char* who) {
  if (!S || !arg) { eu_set_error("%s: null argument", who); return EULER_EINVAL; }
  if (S->slab_on && !S->has_comm) { eu_set_error("%s: row-slab handle without a communicator", who); return EULER_ESTATE; }
  if (!S->loaded) { eu_set_error("%s: no scenario loaded", who); return EULER_ESTATE; }
  if (!S->heat_on) { eu_set_error("%s: heat is off (euler_set_heat)", who); return EULER_ESTATE; }
  return EULER_OK;
}

// (a row-slab handle moves its own rows, (row_hi - row_lo) X floats, as euler_get_field / euler_set_field do there)
extern "C" int euler_heat_get_field(euler_sim* S, float* dst, size_t bytes) {
  const char* who = "euler_heat_get_field";
  int rc = heat_field_enter(S, dst, who);
  if (rc) return rc;
  const size_t n = heat_own_n(S);
  if (bytes != n * sizeof(float)) { eu_set_error("%s: %zu bytes, the field has %zu", who, bytes, n * sizeof(float)); return EULER_EINVAL; }
  HIPCHK(hipMemcpyAsync(dst, heat_t(S) + heat_own0(S), bytes, hipMemcpyDeviceToHost, S->stream));
  HIPCHK(hipStreamSynchronize(S->stream));
  return EULER_OK;
}

// On a row slab COLLECTIVE, as euler_set_field(EULER_F_U) is there: it ends with the exchange of T's ghost rows
extern "C" int euler_heat_set_field(euler_sim* S, const float* src, size_t bytes) {
  const char* who = "euler_heat_set_field";
  int rc = heat_field_enter(S, src, who);
  if (rc) return rc;
  const size_t n = heat_own_n(S);
  if (bytes != n * sizeof(float)) { eu_set_error("%s: %zu bytes, the field has %zu", who, bytes, n * sizeof(float)); rc = EULER_EINVAL; }
  for (size_t i = 0; i < n && !rc; ++i)
    if (!eu_heat_value_ok(src[i])) { eu_set_error("%s: cell %zu holds %g (finite and at most 1e4 in size)", who, i, (double)src[i]); rc = EULER_EINVAL; }
  if (S->slab_on) {      // (one rank's bad value is every rank's refusal: nobody waits in the exchange below for a rank that has left)
    int worst = 0;
    const int rs = eu_slab_status_sync(S, rc, &worst);
    if (rs) return rs;
    if (!rc && worst) { eu_set_error("%s: another rank refused its values", who); rc = EULER_ESTATE; }
  }
  if (rc) return rc;
  // up into the other half, then through the count mask into this one (the copy is waited for: src is the caller's)
  HIPCHK(hipMemcpyAsync(heat_other(S) + heat_own0(S), src, bytes, hipMemcpyHostToDevice, S->stream));
  LAUNCH(S, KC_MISC, k_heat_mask, dim3(eu_blocks(n, 256)), dim3(256), heat_other(S) + heat_own0(S), heat_t(S) + heat_own0(S), S->count + heat_own0(S), n, S->heat.ambient);
  HIPCHK(hipGetLastError());
  if (S->slab_on && (rc = eu_slab_exchange_heat(S))) return rc;
  HIPCHK(hipStreamSynchronize(S->stream));
  return EULER_OK;
}

extern "C" int euler_heat_fill(euler_sim* S, int32_t x0, int32_t y0, int32_t x1, int32_t y1, float value) {
  const char* who = "euler_heat_fill";
  int rc = heat_field_enter(S, S, who);
  if (rc) return rc;
  char why[160];
  if (eu_heat_box_check(x0, y0, x1, y1, S->X, S->Y, why, sizeof why)) { eu_set_error("%s: %s", who, why); return EULER_EINVAL; }
  if (!eu_heat_value_ok(value)) { eu_set_error("%s: value %g must be finite and at most 1e4 in size", who, (double)value); return EULER_EINVAL; }
  const euler_heat_box b = {x0, y0, x1, y1, value, EULER_HEAT_FIX};      // the boxes' kernel on a one-box list
  unsigned int ntiles = 0;
  if ((rc = eu_box_table_upload(S, who, &S->heat_fill_buf, &b, 1, sizeof(euler_heat_box), EULER_HEAT_BOXES_MAX, &ntiles))) return rc;
  // (outside a substep: the class of k_colorize, not one a cost tool sums.  A row slab: the rank's own entries of the one-box table, nothing where the box lies on
  // other ranks; then T's ghost rows - every rank refuses alike above, so the call is collective there)
  if (ntiles && (rc = heat_launch_boxes(S, KC_MISC, &S->heat_fill_buf, ntiles, 0.f))) return rc;
  if (S->slab_on && (rc = eu_slab_exchange_heat(S))) return rc;
  HIPCHK(hipStreamSynchronize(S->stream));
  return EULER_OK;
}

extern "C" int euler_heat_raster(euler_sim* S, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t W, int32_t H, euler_heat_px* out, size_t out_bytes) {
  const char* who = "euler_heat_raster";
  int rc = eu_observe_enter(S, who, nullptr, out, x0, y0, x1, y1);      // (collective on a row-slab handle, like every observer pass there)
  if (rc) return rc;
  if (!S->heat_on) { eu_set_error("%s: heat is off (euler_set_heat)", who); return EULER_ESTATE; }
  const int Bw = x1 - x0 + 1, Bh = y1 - y0 + 1;
  if (W < 1 || H < 1 || W > Bw || H > Bh) { eu_set_error("%s: a raster of %d x %d for a box of %d x %d cells", who, W, H, Bw, Bh); return EULER_EINVAL; }
  const size_t n = (size_t)W * (size_t)H;
  if (out_bytes != n * sizeof(euler_heat_px)) { eu_set_error("%s: %zu bytes given, %zu expected", who, out_bytes, n * sizeof(euler_heat_px)); return EULER_EINVAL; }
  rc = eu_devbuf_reserve(S, who, "the records", &S->heat_ras_buf, out_bytes);
  if (S->slab_on) {      // each rank reduces its own rows of the box into its share of the staging area; the shares fold on the device (k_observe_slab.hip): integer sums and
                         // maxima of bit patterns, so every rank reads the whole-grid bytes.  No row beyond the own ones is read: no exchange
    eu_slab_plan plan;
    const int rp = eu_observe_slab_plan(S, &plan, y0, y1, W, H);      // (the same on every rank)
    if (rp) return rp;
    if ((rc = eu_observe_slab_open(S, who, rc, (size_t)plan.total * sizeof(euler_heat_px), EU_OBS_ROWS_NONE))) return rc;
    const int r = S->cfg.slab_rank;
    if (plan.cnt[r]) {
      euler_heat_px* mine = (euler_heat_px*)eu_observe_slab_mine(S, &plan, EU_OBS_REC_HEAT);
      const int Hl = plan.p_hi[r] - plan.p_lo[r] + 1, ya = plan.ya[r], nrows = plan.yb[r] - plan.ya[r] + 1;
      LAUNCH(S, KC_MISC, k_heat_ras_init, dim3(eu_blocks((size_t)W * Hl, 256)), dim3(256), mine, W, H, Bw, Bh, Hl, plan.p_lo[r], y1, ya, plan.yb[r]);
      LAUNCH(S, KC_MISC, k_heat_raster, dim3((Bw + 63) / 64, (nrows + 3) / 4), dim3(256), heat_t(S), S->solid, S->sink, S->count, mine, S->X, x0, ya, nrows, y1, Bw, Bh, W, H,
             plan.p_lo[r], S->heat.ambient);
      HIPCHK(hipGetLastError());
    }
    if ((rc = eu_observe_slab_fold(S, &plan, EU_OBS_REC_HEAT, S->heat_ras_buf.p))) return rc;
    return eu_observe_readback(S, out, &S->heat_ras_buf, out_bytes);
  }
  if (rc) return rc;
  euler_heat_px* rec = (euler_heat_px*)S->heat_ras_buf.p;
  LAUNCH(S, KC_MISC, k_heat_ras_init, dim3(eu_blocks(n, 256)), dim3(256), rec, W, H, Bw, Bh, H, 0, y1, y0, y1);
  LAUNCH(S, KC_MISC, k_heat_raster, dim3((Bw + 63) / 64, (Bh + 3) / 4), dim3(256), heat_t(S), S->solid, S->sink, S->count, rec, S->X, x0, y0, Bh, y1, Bw, Bh, W, H, 0, S->heat.ambient);
  HIPCHK(hipGetLastError());
  return eu_observe_readback(S, out, &S->heat_ras_buf, out_bytes);
}
