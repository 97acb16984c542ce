// k_overview.hip — euler_overview / euler_overview_box (include/euler.h, docs/overview.md, docs/viewport.md): a box of interior cells - the whole
// interior for euler_overview - reduced on the device to a W x H raster of euler_overview_px records, one box of cells per record.  Every field of a record is an integer sum or a maximum of non-negative
// floats (compared as unsigned bit patterns): whatever order the cells arrive in, the record is the same.
//
// One launch.  A workgroup owns a run of WHOLE pixel boxes of one pixel row - npc <= OV_NPC pixel columns, about OV_SPAN cells wide -
// and, where the boxes are tall, one of nsplit slices of their rows.  Lanes lie along a grid row (four cells each where the rows are
// 16-byte aligned) and walk down the rows of the slice: a lane's columns - and with them its pixels - do not change on the way, so a
// lane sums in registers and goes to the LDS table of its workgroup's pixels ONCE per walk; lanes of a wave that all sit in one pixel fold by shuffles
// first.  The table is written out once: with plain stores where the workgroup saw the whole box (nsplit = 1), else with integer
// atomics into records the host zeroed.  With the tile map, a 64 x 64 tile without water is read for its solid / sink bytes only.
//
// The pass only reads the state and touches none of the handle's validity flags.
#include "k_observe.h"

#include <stdlib.h>

#define OV_T 256        // threads per workgroup
#define OV_NPC 256      // pixels in a workgroup's LDS table
#define OV_SPAN 1024    // cells along x a workgroup aims at: OV_T lanes x 4 cells
#define OV_WG_CELLS (1 << 15)   // cells a workgroup should walk before the boxes' rows are split

struct OvArgs {
  const uint8_t *solid, *sink, *count;
  const float *u, *v, *dye[3];
  ObTiles tiles;
  int X, Y, W, H, npc, nsplit;
  int bx0, by1, Bw, Bh;     // the box: its left column, its top row, its extent in cells (the whole interior: 1, Y - 2, X - 2, Y - 2)
  int py0, cy0, cy1, add;   // row slabs (k_observe_slab.hip): the first pixel row launched - out starts there -, the rows of the box this rank owns, and "out is zeroed: add";
                            // a whole-grid handle: 0, the box's rows, nsplit > 1
  euler_overview_px* out;
};

struct OvAcc {
  unsigned int solid, sink, water, marks, max_bits;
  unsigned long long dye[3];
};
__device__ __forceinline__ void ov_clear(OvAcc& a) { a.solid = a.sink = a.water = a.marks = a.max_bits = 0u; a.dye[0] = a.dye[1] = a.dye[2] = 0ull; }
__device__ __forceinline__ void ov_merge(OvAcc& a, const OvAcc& b) {
  a.solid += b.solid; a.sink += b.sink; a.water += b.water; a.marks += b.marks;
  a.max_bits = b.max_bits > a.max_bits ? b.max_bits : a.max_bits;
  a.dye[0] += b.dye[0]; a.dye[1] += b.dye[1]; a.dye[2] += b.dye[2];
}
struct OvTable {
  unsigned int w[5][OV_NPC];          // solid, sink, water, marks, max_speed2 bits
  unsigned long long dye[3][OV_NPC];
};
template <bool DYE>
__device__ __forceinline__ void ov_to_table(OvTable& t, int p, const OvAcc& a) {
  if (a.solid) atomicAdd(&t.w[0][p], a.solid);
  if (a.sink) atomicAdd(&t.w[1][p], a.sink);
  if (a.water) {
    atomicAdd(&t.w[2][p], a.water);
    atomicAdd(&t.w[3][p], a.marks);
    if (a.max_bits) atomicMax(&t.w[4][p], a.max_bits);
    if (DYE) for (int c = 0; c < 3; ++c) if (a.dye[c]) atomicAdd(&t.dye[c][p], a.dye[c]);
  }
}

// VEC: cells per lane (k_observe.h)
template <int VEC, bool DYE>
__global__ __launch_bounds__(OV_T) void k_overview(const OvArgs a) {
  __shared__ OvTable tab;
  const int tid = threadIdx.x;
  const unsigned int Xi = (unsigned int)a.Bw, Yi = (unsigned int)a.Bh;
  const unsigned int groups = (unsigned int)((a.W + a.npc - 1) / a.npc), slice = blockIdx.x / groups;      // (neighbouring workgroups lie along a row)
  const int p0 = (int)(blockIdx.x % groups) * a.npc, p1 = p0 + a.npc < a.W ? p0 + a.npc : a.W;      // this workgroup's pixel columns [p0, p1)
  const int py = a.py0 + (int)(slice / (unsigned int)a.nsplit), sp = (int)(slice % (unsigned int)a.nsplit);
  const int xa = a.bx0 + (int)((unsigned long long)p0 * Xi / (unsigned int)a.W), xb = a.bx0 - 1 + (int)((unsigned long long)p1 * Xi / (unsigned int)a.W);      // its columns [xa, xb]
  const int ytop = a.by1 - (int)((unsigned long long)py * Yi / (unsigned int)a.H), ybot = a.by1 + 1 - (int)((unsigned long long)(py + 1) * Yi / (unsigned int)a.H);
  const int nrows = ytop - ybot + 1;
  const int shi = ytop - (int)((long long)sp * nrows / a.nsplit), slo = ytop - (int)((long long)(sp + 1) * nrows / a.nsplit) + 1;      // this slice: rows shi down to slo ...
  const int yhi = shi < a.cy1 ? shi : a.cy1, ylo = slo > a.cy0 ? slo : a.cy0;      // ... of which this rank owns yhi down to ylo (a whole-grid handle: all)
  if (yhi < ylo) return;      // (the whole workgroup: nothing of the slice is here)
  for (int k = tid; k < OV_NPC; k += OV_T) {
    for (int f = 0; f < 5; ++f) tab.w[f][k] = 0u;
    for (int c = 0; c < 3; ++c) tab.dye[c][k] = 0ull;
  }
  __syncthreads();
  const size_t X = (size_t)a.X;
  const int xbase = ob_xbase(VEC, xa);      // (the cells an edge cuts are masked below)
  // (the trip count is the same for the lanes of a wave up to the last pass: the shuffles below run behind a wave-uniform test)
  for (int xc = xbase; xc <= xb; xc += OV_T * VEC) {
    const int x0 = xc + tid * VEC;
    OvAcc acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) ov_clear(acc[k]);
    if (x0 <= xb) {
      const int tx = x0 >> 6;      // (four aligned cells share a tile column)
      for (int y = yhi; y >= ylo;) {
        const int ty = y >> 6;
        const int yend = (ty << 6) > ylo ? (ty << 6) : ylo;
        const bool wet = a.tiles.wet(tx, ty);
        for (; y >= yend; --y) {
          ObRow<VEC, true, DYE> row;
          row.load(a.solid, a.sink, a.count, a.u, a.v, a.dye, X, (size_t)y * X + (size_t)x0, wet);
#pragma unroll
          for (int k = 0; k < VEC; ++k) {
            const unsigned int s = row.solid(k), n = row.sink(k), c = row.count(k);
            if (s) acc[k].solid += 1u;
            else if (n) acc[k].sink += 1u;
            else if (wet && c) {
              acc[k].water += 1u;
              acc[k].marks += c < 3u ? c : 3u;
              ob_max_bits(acc[k].max_bits, row.speed2(k));
              if (DYE) for (int ch = 0; ch < 3; ++ch) acc[k].dye[ch] += ob_q24(row.dye[ch][k]);
            }
          }
        }
      }
    }
    // the walk is over: each cell column to its pixel of the table
    int pk[VEC], pmin = 0x7fffffff, pmax = -1;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const int x = x0 + k;
      pk[k] = x >= xa && x <= xb ? (int)(((unsigned long long)(x - a.bx0 + 1) * (unsigned int)a.W - 1ull) / Xi) - p0 : -1;      // the column px whose range holds x
      if (pk[k] >= 0) { pmin = pk[k] < pmin ? pk[k] : pmin; pmax = pk[k] > pmax ? pk[k] : pmax; }
    }
    const int wmin = ob_wave<ObMin>(pmin), wmax = ob_wave<ObMax>(pmax);
    if (wmin == wmax) {      // the whole wave sits in one pixel (wide boxes): fold across the lanes, one lane goes to the table
      OvAcc t;
      ov_clear(t);
#pragma unroll
      for (int k = 0; k < VEC; ++k) if (pk[k] >= 0) ov_merge(t, acc[k]);
      t.solid = ob_wave<ObSum>(t.solid); t.sink = ob_wave<ObSum>(t.sink); t.water = ob_wave<ObSum>(t.water); t.marks = ob_wave<ObSum>(t.marks);
      t.max_bits = ob_wave<ObMax>(t.max_bits);
      if (DYE) for (int c = 0; c < 3; ++c) t.dye[c] = ob_wave<ObSum>(t.dye[c]);
      if ((tid & 63) == 0) ov_to_table<DYE>(tab, wmin, t);
    } else {
      OvAcc t;
      int cur = -1;
      ov_clear(t);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        if (pk[k] < 0) continue;
        if (pk[k] != cur) { if (cur >= 0) ov_to_table<DYE>(tab, cur, t); cur = pk[k]; ov_clear(t); }
        ov_merge(t, acc[k]);
      }
      if (cur >= 0) ov_to_table<DYE>(tab, cur, t);
    }
  }
  __syncthreads();
  for (int k = tid; k < p1 - p0; k += OV_T) {
    const int p = p0 + k;
    const unsigned int wpx = (unsigned int)((unsigned long long)(p + 1) * Xi / (unsigned int)a.W) - (unsigned int)((unsigned long long)p * Xi / (unsigned int)a.W);
    const unsigned int cells = wpx * (unsigned int)(yhi - ylo + 1);
    euler_overview_px* o = a.out + (size_t)(py - a.py0) * a.W + p;
    if (!a.add) {
      euler_overview_px r;
      r.cells = cells; r.solid = tab.w[0][k]; r.sink = tab.w[1][k]; r.water = tab.w[2][k]; r.marks = tab.w[3][k];
      r.max_speed2 = __uint_as_float(tab.w[4][k]);
      r.dye[0] = tab.dye[0][k]; r.dye[1] = tab.dye[1][k]; r.dye[2] = tab.dye[2][k];
      *o = r;
    } else {      // a slice of the box's rows, or a rank's share of them: added to the record the host zeroed (integers and a maximum: exact in any order)
      if (cells) atomicAdd(&o->cells, cells);
      if (tab.w[0][k]) atomicAdd(&o->solid, tab.w[0][k]);
      if (tab.w[1][k]) atomicAdd(&o->sink, tab.w[1][k]);
      if (tab.w[2][k]) {
        atomicAdd(&o->water, tab.w[2][k]);
        atomicAdd(&o->marks, tab.w[3][k]);
        if (tab.w[4][k]) atomicMax(reinterpret_cast<unsigned int*>(&o->max_speed2), tab.w[4][k]);
        for (int c = 0; c < 3; ++c) if (tab.dye[c][k]) atomicAdd(reinterpret_cast<unsigned long long*>(&o->dye[c]), tab.dye[c][k]);
      }
    }
  }
}

// the reduction alone, on the handle's stream, into the records of S->ov_buf (tools/overview_cost.py times it through the KC_MISC class)
// plan: row slabs - the records go to this rank's share of the staging area, the pixel rows its rows touch only
static int ov_launch(euler_sim* S, int x0, int y0, int x1, int y1, int W, int H, const eu_slab_plan* plan = nullptr) {
  const int Xi = x1 - x0 + 1, Yi = y1 - y0 + 1;      // (the box's extent: npc and nsplit follow it)
  OvArgs a;
  a.solid = S->solid; a.sink = S->sink; a.count = S->count; a.u = S->u; a.v = S->v;
  for (int c = 0; c < 3; ++c) a.dye[c] = S->dye[c];
  a.tiles = eu_observe_tiles(S);
  a.X = S->X; a.Y = S->Y; a.W = W; a.H = H; a.out = (euler_overview_px*)S->ov_buf.p;
  a.bx0 = x0; a.by1 = y1; a.Bw = Xi; a.Bh = Yi;
  long long npc = (long long)OV_SPAN * W / Xi;      // pixel columns per workgroup: about OV_SPAN cells wide, at least one box, at most the table
  a.npc = (int)(npc < 1 ? 1 : (npc > OV_NPC ? OV_NPC : npc));
  const long long span = ((long long)a.npc * Xi + W - 1) / W, rows_max = (Yi + H - 1) / H, rows_min = Yi / H;
  long long ns = (span * rows_max + OV_WG_CELLS - 1) / OV_WG_CELLS;      // slices of a box's rows
  a.nsplit = (int)(ns < 1 ? 1 : (ns > rows_min ? rows_min : ns));
  a.py0 = 0; a.cy0 = y0; a.cy1 = y1; a.add = a.nsplit > 1;
  int Hl = H;      // pixel rows launched
  if (plan) {
    const int r = S->cfg.slab_rank;
    int rc = eu_observe_slab_clear_mine(S, plan, EU_OBS_REC_OVERVIEW);
    if (rc || plan->cnt[r] == 0) return rc;      // (no row of the box is here: nothing to launch, nothing to contribute)
    a.out = (euler_overview_px*)eu_observe_slab_mine(S, plan, EU_OBS_REC_OVERVIEW);
    a.py0 = plan->p_lo[r]; a.cy0 = plan->ya[r]; a.cy1 = plan->yb[r]; a.add = 1;
    Hl = plan->p_hi[r] - plan->p_lo[r] + 1;
  } else if (a.nsplit > 1) HIPCHK(hipMemsetAsync(S->ov_buf.p, 0, (size_t)W * H * sizeof(euler_overview_px), S->stream));
  const long long nwg = (long long)((W + a.npc - 1) / a.npc) * Hl * a.nsplit;      // (at most a workgroup per 256 cells: far below 2^31 on any grid euler_create accepts)
  const dim3 grid((unsigned)nwg);
  const bool vec = S->X % 4 == 0, dye = S->dye[0] != nullptr;
  if (vec && dye) LAUNCH(S, KC_MISC, (k_overview<4, true>), grid, dim3(OV_T), a);
  else if (vec) LAUNCH(S, KC_MISC, (k_overview<4, false>), grid, dim3(OV_T), a);
  else if (dye) LAUNCH(S, KC_MISC, (k_overview<1, true>), grid, dim3(OV_T), a);
  else LAUNCH(S, KC_MISC, (k_overview<1, false>), grid, dim3(OV_T), a);
  HIPCHK(hipGetLastError());
  return EULER_OK;
}

// euler_overview_box behind the entry checks (euler_render_view enters once for both of its passes)
int eu_overview_entered(euler_sim* S, const char* who, int x0, int y0, int x1, int y1, int W, int H, euler_overview_px* out, size_t out_bytes) {
  if (W < 1 || H < 1 || W > x1 - x0 + 1 || H > y1 - y0 + 1) { eu_set_error("%s: a raster of %d x %d for a box of %d x %d cells", who, W, H, x1 - x0 + 1, y1 - y0 + 1); return EULER_EINVAL; }
  const size_t n = (size_t)W * (size_t)H;
  if (out_bytes != n * sizeof(euler_overview_px)) { eu_set_error("%s: %zu bytes given, %zu expected", who, out_bytes, n * sizeof(euler_overview_px)); return EULER_EINVAL; }
  int rc = eu_devbuf_reserve(S, "euler_overview", "the records", &S->ov_buf, out_bytes);
  if (S->slab_on) {      // collective: the own rows into this rank's share, the shares folded into the records on every rank
    eu_slab_plan plan;
    const int rp = eu_observe_slab_plan(S, &plan, y0, y1, W, H);      // (the same on every rank)
    if (rp) return rp;
    rc = eu_observe_slab_open(S, who, rc, (size_t)plan.total * sizeof(euler_overview_px), EU_OBS_ROWS_CELLS);
    if (!rc) rc = ov_launch(S, x0, y0, x1, y1, W, H, &plan);
    if (!rc) rc = eu_observe_slab_fold(S, &plan, EU_OBS_REC_OVERVIEW, S->ov_buf.p);
  } else if (!rc) rc = ov_launch(S, x0, y0, x1, y1, W, H);
  return rc ? rc : eu_observe_readback(S, out, &S->ov_buf, out_bytes);
}

// the call behind euler_overview (the whole interior) and euler_overview_box
static int ov_call(euler_sim* S, const char* who, int x0, int y0, int x1, int y1, int W, int H, euler_overview_px* out, size_t out_bytes) {
  const int rc = eu_observe_enter(S, who, nullptr, out, x0, y0, x1, y1);
  return rc ? rc : eu_overview_entered(S, who, x0, y0, x1, y1, W, H, out, out_bytes);
}

extern "C" int euler_overview(euler_sim* S, int32_t W, int32_t H, euler_overview_px* out, size_t out_bytes) {
  if (!S) { eu_set_error("euler_overview: null argument"); return EULER_EINVAL; }
  return ov_call(S, "euler_overview", 1, 1, S->X - 2, S->Y - 2, W, H, out, out_bytes);
}

extern "C" int euler_overview_box(euler_sim* S, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t W, int32_t H, euler_overview_px* out, size_t out_bytes) {
  return ov_call(S, "euler_overview_box", x0, y0, x1, y1, W, H, out, out_bytes);
}

extern "C" int euler_render_fit(euler_sim* S, int32_t wx, int32_t wy, char* out, int32_t cap, int32_t* len) {
  if (!S || !len || wx < 1 || wy < 1) { eu_set_error("euler_render_fit: bad argument"); return EULER_EINVAL; }
  const int W = wx < S->X - 2 ? wx : S->X - 2, H = wy < S->Y - 2 ? wy : S->Y - 2;
  const size_t bytes = (size_t)W * H * sizeof(euler_overview_px);
  euler_overview_px* px = (euler_overview_px*)malloc(bytes);
  if (!px) return EULER_ENOMEM;
  int rc = euler_overview(S, W, H, px, bytes);
  if (!rc) rc = euler_overview_text(px, W, H, S->cfg.rainbow, out, cap, len);
  free(px);
  return rc;
}
