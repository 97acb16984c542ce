// k_diagnostics.hip — euler_diagnostics (include/euler.h, docs/diagnostics.md): a box of interior cells reduced on the device to ONE euler_diag record -
// residual divergence, kinetic energy, mass and centre of mass, marker crowding.  Every field is an integer sum or a maximum of non-negative floats
// (compared as unsigned bit patterns): whatever order the cells arrive in, the record is the same.
//
// One launch.  A workgroup owns DG_T * VEC columns of the box and one segment of at most DG_ROWS rows that lies inside one row of 64 x 64 tiles.  Lanes lie
// along a grid row (four cells each where the rows are 16-byte aligned) and walk DOWN the segment: the row of v below a cell is the next row's own v and is
// kept in registers, so a row costs one load of count, solid, u and v each plus the cell to the left of the lane's first.  A lane sums in registers; a wave
// folds by shuffles and goes to the workgroup's LDS record once; the workgroup goes to the device record once, twelve lanes with one integer atomic each.
// With the tile map a lane whose tile holds no water reads nothing at all.
//
// The pass only reads the state and touches none of the handle's validity flags.
#include "k_observe.h"

#define DG_T 256        // threads per workgroup
#define DG_ROWS 32      // rows a workgroup walks: divides 64, so a segment never crosses a row of 64 x 64 tiles (one tile-map flag per lane and segment);
                        // chosen by measurement, profiles/diagnostics.md
static_assert(64 % DG_ROWS == 0, "a segment must lie inside one row of tiles");

struct DgArgs {
  const uint8_t *solid, *count;
  const float *u, *v;
  ObTiles tiles;
  int X;
  int x0, y0, x1, y1;       // the box, inclusive
  int ncol;                 // workgroups along x
  euler_diag* out;          // zeroed in front of the launch
};

struct DgAcc {
  unsigned long long mass_x, mass_y, div_l1, ke_hi, ke_lo;
  unsigned int fluid, markers, crowded, nonfinite, count_max, div_bits, s2_bits;
};

// the workgroup's record in LDS, in the order of euler_diag's 64-bit fields behind `cells`, then its 32-bit ones
struct DgShared {
  unsigned long long q[8];      // fluid, markers, crowded, mass_x, mass_y, div_l1, ke_hi, ke_lo
  unsigned int w[4];            // count_max, nonfinite, max_div bits, max_speed2 bits
};

// VEC: cells per lane (k_observe.h)
template <int VEC>
__global__ __launch_bounds__(DG_T) void k_diagnostics(const DgArgs a) {
  __shared__ DgShared sh;
  const int tid = threadIdx.x;
  if (tid < 8) sh.q[tid] = 0ull;
  else if (tid < 12) sh.w[tid - 8] = 0u;
  __syncthreads();
  const int cx = (int)(blockIdx.x % (unsigned int)a.ncol), seg = (int)(blockIdx.x / (unsigned int)a.ncol);      // (neighbouring workgroups lie along a row)
  const int r0 = (a.y0 / DG_ROWS + seg) * DG_ROWS;
  const int ylo = r0 > a.y0 ? r0 : a.y0, yhi = r0 + DG_ROWS - 1 < a.y1 ? r0 + DG_ROWS - 1 : a.y1;      // this segment: rows yhi down to ylo
  const int x = ob_xbase(VEC, a.x0) + (cx * DG_T + tid) * VEC;      // the lane's first column
  DgAcc acc;
  acc.mass_x = acc.mass_y = acc.div_l1 = acc.ke_hi = acc.ke_lo = 0ull;
  acc.fluid = acc.markers = acc.crowded = acc.nonfinite = acc.count_max = acc.div_bits = acc.s2_bits = 0u;
  // (four aligned cells share a tile column, the segment's rows a tile row)
  if (x <= a.x1 && a.tiles.wet(x >> 6, ylo >> 6)) {
    const size_t X = (size_t)a.X;
    bool in[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) in[k] = x + k >= a.x0 && x + k <= a.x1;      // box edges that cut the lane's group
    ObRow<VEC, false, false> row;
    row.load_v(a.v, (size_t)yhi * X + (size_t)x);      // v of the row being visited: from here on, the row below of the one before
    for (int y = yhi; y >= ylo; --y) {
      row.template load<false>(a.solid, nullptr, a.count, a.u, a.v, nullptr, X, (size_t)y * X + (size_t)x, true);
      unsigned int row_marks = 0u;
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const unsigned int s = row.solid(k), c = row.count(k);
        if (in[k] && c && !s) {
          acc.fluid += 1u;
          row_marks += c;
          acc.crowded += c >= (unsigned int)EULER_DIAG_CROWDED ? 1u : 0u;
          acc.count_max = c > acc.count_max ? c : acc.count_max;
          acc.mass_x += (unsigned long long)c * (unsigned int)(x + k);
          const float d = row.divergence(k), s2 = row.speed2(k);
          if (d == d) {
            const float ad = fabsf(d);
            ob_max_bits(acc.div_bits, ad);
            acc.div_l1 += (unsigned long long)((ad < 256.f ? ad : 256.f) * 16777216.f);
          }
          if (s2 == s2) {
            ob_max_bits(acc.s2_bits, s2);
            const unsigned long long q = (unsigned long long)((s2 < 16777216.f ? s2 : 16777216.f) * 4294967296.f);
            acc.ke_hi += q >> 32; acc.ke_lo += q & 0xffffffffull;
          }
          acc.nonfinite += (d != d || s2 != s2) ? 1u : 0u;
        }
      }
      acc.markers += row_marks;
      acc.mass_y += (unsigned long long)row_marks * (unsigned int)y;
      row.carry_v();
    }
  }
  // every lane of the workgroup arrives here: fold across the wave, one lane per wave goes to LDS, twelve lanes of the workgroup to the record
  const unsigned int fluid = ob_wave<ObSum>(acc.fluid);
  if (fluid) {      // (wave-uniform)
    const unsigned int markers = ob_wave<ObSum>(acc.markers), crowded = ob_wave<ObSum>(acc.crowded), nonfinite = ob_wave<ObSum>(acc.nonfinite);
    const unsigned int count_max = ob_wave<ObMax>(acc.count_max), div_bits = ob_wave<ObMax>(acc.div_bits), s2_bits = ob_wave<ObMax>(acc.s2_bits);
    const unsigned long long mass_x = ob_wave<ObSum>(acc.mass_x), mass_y = ob_wave<ObSum>(acc.mass_y), div_l1 = ob_wave<ObSum>(acc.div_l1);
    const unsigned long long ke_hi = ob_wave<ObSum>(acc.ke_hi), ke_lo = ob_wave<ObSum>(acc.ke_lo);
    if ((tid & 63) == 0) {
      atomicAdd(&sh.q[0], (unsigned long long)fluid); atomicAdd(&sh.q[1], (unsigned long long)markers); atomicAdd(&sh.q[2], (unsigned long long)crowded);
      atomicAdd(&sh.q[3], mass_x); atomicAdd(&sh.q[4], mass_y); atomicAdd(&sh.q[5], div_l1); atomicAdd(&sh.q[6], ke_hi); atomicAdd(&sh.q[7], ke_lo);
      atomicMax(&sh.w[0], count_max); atomicAdd(&sh.w[1], nonfinite); atomicMax(&sh.w[2], div_bits); atomicMax(&sh.w[3], s2_bits);
    }
  }
  __syncthreads();
  // (euler_diag: cells at 0, the eight sums behind it, then count_max, nonfinite, max_div, max_speed2)
  unsigned long long* oq = reinterpret_cast<unsigned long long*>(a.out);
  unsigned int* ow = reinterpret_cast<unsigned int*>(a.out) + 18;
  if (blockIdx.x == 0 && tid == 12) atomicAdd(oq, (unsigned long long)(a.x1 - a.x0 + 1) * (unsigned long long)(a.y1 - a.y0 + 1));
  if (sh.q[0] == 0ull) return;      // no water under this workgroup: nothing to add
  if (tid < 8) { if (sh.q[tid]) atomicAdd(oq + 1 + tid, sh.q[tid]); }
  else if (tid == 9) { if (sh.w[1]) atomicAdd(ow + 1, sh.w[1]); }
  else if (tid < 12) { const int f = tid - 8; if (sh.w[f]) atomicMax(ow + f, sh.w[f]); }
}

static_assert(sizeof(euler_diag) == 88, "euler_diag is 88 bytes without padding");
static_assert(offsetof(euler_diag, fluid) == 8 && offsetof(euler_diag, ke_lo) == 64 && offsetof(euler_diag, count_max) == 72 && offsetof(euler_diag, max_speed2) == 84,
              "k_diagnostics addresses the record by these offsets");

// the reduction alone, on the handle's stream, into the record of S->diag_buf (tools/diagnostics_cost.py times it through the KC_MISC class)
// (row slabs: the box is the rank's rows of the caller's box and `out` the rank's record in the staging area - the kernel needs no clip of its own: cells, mass_y and
// the segments all follow the box it is given)
static int dg_launch(euler_sim* S, int x0, int y0, int x1, int y1, euler_diag* out) {
  const bool vec = S->X % 4 == 0;
  DgArgs a;
  a.solid = S->solid; a.count = S->count; a.u = S->u; a.v = S->v;
  a.tiles = eu_observe_tiles(S);
  a.X = S->X; a.x0 = x0; a.y0 = y0; a.x1 = x1; a.y1 = y1; a.out = out;
  const int xbase = ob_xbase(vec ? 4 : 1, x0), span = DG_T * (vec ? 4 : 1);
  a.ncol = (x1 - xbase + span) / span;
  const int nseg = y1 / DG_ROWS - y0 / DG_ROWS + 1;
  HIPCHK(hipMemsetAsync(out, 0, sizeof(euler_diag), S->stream));
  const dim3 grid((unsigned)((long long)a.ncol * nseg));      // (a workgroup per 256 x 32 cells at the least: far below 2^31 on any grid euler_create accepts)
  if (vec) LAUNCH(S, KC_MISC, (k_diagnostics<4>), grid, dim3(DG_T), a);
  else LAUNCH(S, KC_MISC, (k_diagnostics<1>), grid, dim3(DG_T), a);
  HIPCHK(hipGetLastError());
  return EULER_OK;
}

extern "C" int euler_diagnostics(euler_sim* S, int32_t x0, int32_t y0, int32_t x1, int32_t y1, euler_diag* out, size_t out_bytes) {
  int rc = eu_observe_enter(S, "euler_diagnostics", nullptr, out, x0, y0, x1, y1);
  if (rc) return rc;
  if (out_bytes != sizeof(euler_diag)) { eu_set_error("euler_diagnostics: %zu bytes given, %zu expected", out_bytes, sizeof(euler_diag)); return EULER_EINVAL; }
  rc = eu_devbuf_reserve(S, "euler_diagnostics", "the record", &S->diag_buf, sizeof(euler_diag));
  if (S->slab_on) {      // collective: every rank's record of its own rows of the box (zeros where it has none), gathered and folded into the record on every rank
    eu_slab_plan plan;
    int ya, yb;
    const int mine = eu_slab_clip_rows(S->band_lo, S->band_hi, S->Y, y0, y1, &ya, &yb);
    if (eu_slab_plan_flat(&plan, S->cfg.slab_nranks, 1)) { eu_set_error("euler_diagnostics: %d ranks", S->cfg.slab_nranks); return EULER_EINVAL; }
    rc = eu_observe_slab_open(S, "euler_diagnostics", rc, (size_t)plan.total * sizeof(euler_diag), EU_OBS_ROWS_CELLS);
    if (!rc) rc = mine ? dg_launch(S, x0, ya, x1, yb, (euler_diag*)eu_observe_slab_mine(S, &plan, EU_OBS_REC_DIAG)) : eu_observe_slab_clear_mine(S, &plan, EU_OBS_REC_DIAG);
    if (!rc) rc = eu_observe_slab_fold(S, &plan, EU_OBS_REC_DIAG, S->diag_buf.p);
  } else
  if (!rc) rc = dg_launch(S, x0, y0, x1, y1, (euler_diag*)S->diag_buf.p);
  return rc ? rc : eu_observe_readback(S, out, &S->diag_buf, sizeof(euler_diag));
}
