// k_flow.hip — euler_flow_raster (include/euler.h, docs/flow_raster.md): a box of interior cells reduced on the device to a W x H raster of euler_flow_px
// records - signed sums of the cell-centre velocity, of the vorticity at the wet nodes and of the pressure, with their maxima.  The box, the raster and the
// pixel edges are euler_overview_box's.  Every field of a record is an integer sum or a maximum of non-negative floats (compared as unsigned bit patterns):
// whatever order the cells arrive in, the record is the same.
//
// The velocity part is k_overview's geometry: a workgroup owns a run of WHOLE pixel boxes of one pixel row (npc <= FL_NPC pixel columns, about FL_SPAN
// cells wide) and, where the boxes are tall, one of nsplit slices of their rows.  Lanes lie along a grid row (four cells each where the rows are 16-byte
// aligned) and walk DOWN the rows: the row above a cell - whose u and whose water bits the vorticity of the cell's node needs - is the row just visited and
// is carried in registers, as is v (the row below is the next row's own).  A row costs the loads of k_overview's row plus the one cell right of the lane's
// group.  A lane sums in registers and goes to the workgroup's LDS table once per walk; the table is written out once: with plain stores where the
// workgroup saw the whole box (nsplit = 1), else with integer atomics into records the host zeroed.  With the tile map a lane skips the rows of a 64 x 64
// tile without water: no cell of it is water, so none of its nodes is wet; the neighbours a wet tile reads in a dry one hold the zeros the map stands for.
//
// The pressure part is a second small kernel in the order of the band-skewed array (euler_dev.h skew_index): a wave reads pair-records - 128 doubles,
// contiguous - lane l holding the two neighbouring cells (t - l, 64 band + l), (t + 1 - l, 64 band + l) of each, and walks FP_RUN of them: its row and with
// it its pixel row stay, its pixel column only grows, so a lane sums in registers while the pixel stays and goes to the record with integer atomics when it
// changes.  No row-major staging copy of the array is made.
//
// The pass only reads the state and touches none of the handle's validity flags (with EULER_FLOW_PRESSURE the pending pressure is finished first, as
// euler_get_field does).
#include "k_observe.h"

int eu_pressure_current(euler_sim* S);      // k_grid.hip

#define FL_T 256        // threads per workgroup
#define FL_NPC 256      // pixels in a workgroup's LDS table
#define FL_SPAN 1024    // cells along x a workgroup aims at: FL_T lanes x 4 cells
#define FL_WG_CELLS (1 << 14)   // cells a workgroup should walk before the boxes' rows are split: half of k_overview's, chosen by measurement (profiles/flow.md)
#define FP_RUN 16       // pair-records a wave of the pressure part walks

struct FlArgs {
  const uint8_t *solid, *sink, *count;
  const float *u, *v;
  ObTiles tiles;
  int X, W, H, npc, nsplit;
  int bx0, by1, Bw, Bh;     // the box: its left column, its top row, its extent in cells
  int py0, cy0, cy1, add;   // row slabs (k_overview.hip OvArgs): the first pixel row launched, the rows of the box this rank owns, "out is zeroed: add"
  euler_flow_px* out;
};

struct FlAcc {
  unsigned int water, nodes, nonfinite, s2_bits, w_bits;
  unsigned long long s[6];      // u_pos, u_neg, v_pos, v_neg, w_pos, w_neg
};
__device__ __forceinline__ void fl_clear(FlAcc& a) {
  a.water = a.nodes = a.nonfinite = a.s2_bits = a.w_bits = 0u;
#pragma unroll
  for (int f = 0; f < 6; ++f) a.s[f] = 0ull;
}
__device__ __forceinline__ void fl_merge(FlAcc& a, const FlAcc& b) {
  a.water += b.water; a.nodes += b.nodes; a.nonfinite += b.nonfinite;
  a.s2_bits = b.s2_bits > a.s2_bits ? b.s2_bits : a.s2_bits;
  a.w_bits = b.w_bits > a.w_bits ? b.w_bits : a.w_bits;
#pragma unroll
  for (int f = 0; f < 6; ++f) a.s[f] += b.s[f];
}
struct FlTable {
  unsigned int w[5][FL_NPC];          // water, nodes, nonfinite, max_speed2 bits, max_abs_w bits
  unsigned long long s[6][FL_NPC];
};
__device__ __forceinline__ void fl_to_table(FlTable& t, int p, const FlAcc& a) {
  if (!a.water) return;      // (no water cell: no node, no term)
  atomicAdd(&t.w[0][p], a.water);
  if (a.nodes) atomicAdd(&t.w[1][p], a.nodes);
  if (a.nonfinite) atomicAdd(&t.w[2][p], a.nonfinite);
  if (a.s2_bits) atomicMax(&t.w[3][p], a.s2_bits);
  if (a.w_bits) atomicMax(&t.w[4][p], a.w_bits);
#pragma unroll
  for (int f = 0; f < 6; ++f) if (a.s[f]) atomicAdd(&t.s[f][p], a.s[f]);
}

// qv, qp of include/euler.h
__device__ __forceinline__ unsigned long long fl_qv(float a) { return (unsigned long long)((a < 4096.f ? a : 4096.f) * 1048576.f); }
__device__ __forceinline__ unsigned long long fl_qp(float a) { return (unsigned long long)((a > 0.f ? (a < 16777216.f ? a : 16777216.f) : 0.f) * 256.f); }
// a term that is not a NaN to the sum of its sign (-0.f: the positive side)
__device__ __forceinline__ void fl_signed(unsigned long long& pos, unsigned long long& neg, float a) {
  if (a >= 0.f) pos += fl_qv(a);
  else neg += fl_qv(-a);
}
__device__ __forceinline__ bool fl_water1(const uint8_t* solid, const uint8_t* sink, const uint8_t* count, size_t i) { return !solid[i] && !sink[i] && count[i]; }
// the water bits of a lane's VEC cells (packed bytes) and of the cell right of them (bit VEC)
template <int VEC>
__device__ __forceinline__ unsigned int fl_water_bits(unsigned int so, unsigned int si, unsigned int cn, bool right) {
  unsigned int m = right ? 1u << VEC : 0u;
#pragma unroll
  for (int k = 0; k < VEC; ++k) if (!((so >> (8 * k)) & 0xffu) && !((si >> (8 * k)) & 0xffu) && ((cn >> (8 * k)) & 0xffu)) m |= 1u << k;
  return m;
}

// VEC: cells per lane (k_observe.h)
template <int VEC>
__global__ __launch_bounds__(FL_T) void k_flow(const FlArgs a) {
  typedef ObRow<VEC, true, false> Row;
  __shared__ FlTable tab;
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
  for (int k = tid; k < FL_NPC; k += FL_T) {
    for (int f = 0; f < 5; ++f) tab.w[f][k] = 0u;
    for (int f = 0; f < 6; ++f) tab.s[f][k] = 0ull;
  }
  __syncthreads();
  const size_t X = (size_t)a.X;
  const int xbase = ob_xbase(VEC, xa);      // (the cells an edge cuts are masked below)
  // (the trip count is the same for the lanes of a wave up to the last pass: the shuffles below run behind a wave-uniform test)
  for (int xc = xbase; xc <= xb; xc += FL_T * VEC) {
    const int x0 = xc + tid * VEC;
    FlAcc acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) fl_clear(acc[k]);
    if (x0 <= xb) {
      const int tx = x0 >> 6;      // (four aligned cells share a tile column)
      const size_t ne = (size_t)(x0 + VEC < a.X ? VEC : a.X - 1 - x0);      // the cell right of the group, kept inside its row (the group's last cell is then outside every box)
      bool in[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) in[k] = x0 + k >= xa && x0 + k <= xb;
      for (int y = yhi; y >= ylo;) {
        const int ty = y >> 6;
        const int yend = (ty << 6) > ylo ? (ty << 6) : ylo;
        if (!a.tiles.wet(tx, ty)) { y = yend - 1; continue; }      // no water in the tile: no water cell, no wet node
        // the first row of a walk: the row above it - its u, its water bits - and its own v; from then on they are carried
        float ua[VEC], vv[VEC];
        unsigned int wa;
        {
          const size_t i = (size_t)(y + 1) * X + (size_t)x0;
          Row::cells(ua, a.u, i);
          wa = fl_water_bits<VEC>(Row::bytes(a.solid, i), Row::bytes(a.sink, i), Row::bytes(a.count, i), fl_water1(a.solid, a.sink, a.count, i + ne));
          Row::cells(vv, a.v, i - X);
        }
        for (; y >= yend; --y) {
          const size_t i = (size_t)y * X + (size_t)x0;
          float uu[VEC + 1], vd[VEC];
          const unsigned int wb = fl_water_bits<VEC>(Row::bytes(a.solid, i), Row::bytes(a.sink, i), Row::bytes(a.count, i), fl_water1(a.solid, a.sink, a.count, i + ne));
          Row::cells(uu + 1, a.u, i);
          uu[0] = a.u[i - 1];
          Row::cells(vd, a.v, i - X);
          const float vx = a.v[i + ne];
          const unsigned int node = wb & (wb >> 1) & wa & (wa >> 1);      // bit k: the node of cell k is wet
#pragma unroll
          for (int k = 0; k < VEC; ++k) {
            if (!in[k] || !((wb >> k) & 1u)) continue;
            const float dx = (uu[k + 1] + uu[k]) / 2.f, dy = (vv[k] + vd[k]) / 2.f;
            acc[k].water += 1u;
            ob_max_bits(acc[k].s2_bits, dx * dx + dy * dy);
            if (dx == dx) fl_signed(acc[k].s[0], acc[k].s[1], dx);
            if (dy == dy) fl_signed(acc[k].s[2], acc[k].s[3], dy);
            bool bad = dx != dx || dy != dy;
            if ((node >> k) & 1u) {
              const float vr = k + 1 < VEC ? vv[k + 1] : vx;
              const float w = (vr - vv[k]) - (ua[k] - uu[k + 1]);
              if (w == w) {
                acc[k].nodes += 1u;
                fl_signed(acc[k].s[4], acc[k].s[5], w);
                ob_max_bits(acc[k].w_bits, fabsf(w));
              } else bad = true;
            }
            acc[k].nonfinite += bad ? 1u : 0u;
          }
          wa = wb;
#pragma unroll
          for (int k = 0; k < VEC; ++k) { ua[k] = uu[k + 1]; vv[k] = vd[k]; }
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
      FlAcc t;
      fl_clear(t);
#pragma unroll
      for (int k = 0; k < VEC; ++k) if (pk[k] >= 0) fl_merge(t, acc[k]);
      t.water = ob_wave<ObSum>(t.water);
      if (t.water) {      // (wave-uniform)
        t.nodes = ob_wave<ObSum>(t.nodes); t.nonfinite = ob_wave<ObSum>(t.nonfinite);
        t.s2_bits = ob_wave<ObMax>(t.s2_bits); t.w_bits = ob_wave<ObMax>(t.w_bits);
#pragma unroll
        for (int f = 0; f < 6; ++f) t.s[f] = ob_wave<ObSum>(t.s[f]);
        if ((tid & 63) == 0) fl_to_table(tab, wmin, t);
      }
    } else {
      FlAcc t;
      int cur = -1;
      fl_clear(t);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        if (pk[k] < 0) continue;
        if (pk[k] != cur) { if (cur >= 0) fl_to_table(tab, cur, t); cur = pk[k]; fl_clear(t); }
        fl_merge(t, acc[k]);
      }
      if (cur >= 0) fl_to_table(tab, cur, t);
    }
  }
  __syncthreads();
  for (int k = tid; k < p1 - p0; k += FL_T) {
    const int p = p0 + k;
    const unsigned int wpx = (unsigned int)((unsigned long long)(p + 1) * Xi / (unsigned int)a.W) - (unsigned int)((unsigned long long)p * Xi / (unsigned int)a.W);
    const unsigned int cells = wpx * (unsigned int)(yhi - ylo + 1);
    euler_flow_px* o = a.out + (size_t)(py - a.py0) * a.W + p;
    if (!a.add) {
      euler_flow_px r;
      r.cells = cells; r.water = tab.w[0][k]; r.nodes = tab.w[1][k]; r.nonfinite = tab.w[2][k];
      r.u_pos = tab.s[0][k]; r.u_neg = tab.s[1][k]; r.v_pos = tab.s[2][k]; r.v_neg = tab.s[3][k]; r.w_pos = tab.s[4][k]; r.w_neg = tab.s[5][k];
      r.p_sum = 0ull;
      r.max_speed2 = __uint_as_float(tab.w[3][k]); r.max_abs_w = __uint_as_float(tab.w[4][k]); r.max_p = 0.f; r.reserved = 0u;
      *o = r;
    } else {      // a slice of the box's rows, or a rank's share of them: added to the record the host zeroed (integers and maxima: exact in any order)
      if (cells) atomicAdd(&o->cells, cells);
      if (tab.w[0][k]) {
        atomicAdd(&o->water, tab.w[0][k]);
        if (tab.w[1][k]) atomicAdd(&o->nodes, tab.w[1][k]);
        if (tab.w[2][k]) atomicAdd(&o->nonfinite, tab.w[2][k]);
        if (tab.w[3][k]) atomicMax(reinterpret_cast<unsigned int*>(&o->max_speed2), tab.w[3][k]);
        if (tab.w[4][k]) atomicMax(reinterpret_cast<unsigned int*>(&o->max_abs_w), tab.w[4][k]);
        unsigned long long* os = reinterpret_cast<unsigned long long*>(&o->u_pos);      // (u_pos ... w_neg lie in the table's order)
        for (int f = 0; f < 6; ++f) if (tab.s[f][k]) atomicAdd(os + f, tab.s[f][k]);
      }
    }
  }
}

static_assert(sizeof(euler_flow_px) == 88, "euler_flow_px is 88 bytes without padding");
static_assert(offsetof(euler_flow_px, water) == 4 && offsetof(euler_flow_px, nodes) == 8 && offsetof(euler_flow_px, nonfinite) == 12 && offsetof(euler_flow_px, u_pos) == 16 &&
              offsetof(euler_flow_px, u_neg) == 24 && offsetof(euler_flow_px, v_pos) == 32 && offsetof(euler_flow_px, v_neg) == 40 && offsetof(euler_flow_px, w_pos) == 48 &&
              offsetof(euler_flow_px, w_neg) == 56 && offsetof(euler_flow_px, p_sum) == 64 && offsetof(euler_flow_px, max_speed2) == 72 && offsetof(euler_flow_px, max_abs_w) == 76 &&
              offsetof(euler_flow_px, max_p) == 80 && offsetof(euler_flow_px, reserved) == 84, "k_flow addresses the six sums behind u_pos as one array");

// ---- the pressure part: S->p in its own, band-skewed order
struct FpArgs {
  const double* p;
  SkewGeom g;
  const uint8_t *solid, *sink, *count;
  const float *u, *v;
  int W, H;
  int bx0, by0, bx1, by1, Bw, Bh;     // the box, inclusive, and its extent
  int band0, nbands, runs, tbase;     // the bands the box crosses (row slabs: of this rank's); runs of FP_RUN pair-records per band, from record tbase (even) on
  int py0;                            // row slabs: the pixel row out starts at (0 on a whole-grid handle)
  euler_flow_px* out;
};

// is one of the velocity terms of water cell (x, y) a NaN?  Then k_flow has counted the cell in nonfinite already (the pressure part asks only where pf is a NaN)
__device__ static bool fp_velocity_nan(const FpArgs& a, int x, int y) {
  const size_t X = (size_t)a.g.X, i = (size_t)y * X + (size_t)x;
  const float dx = (a.u[i] + a.u[i - 1]) / 2.f, dy = (a.v[i] + a.v[i - X]) / 2.f;
  if (dx != dx || dy != dy) return true;
  if (!fl_water1(a.solid, a.sink, a.count, i + 1) || !fl_water1(a.solid, a.sink, a.count, i + X) || !fl_water1(a.solid, a.sink, a.count, i + X + 1)) return false;
  const float w = (a.v[i + 1] - a.v[i]) - (a.u[i + X] - a.u[i]);
  return w != w;
}

struct FpAcc { unsigned long long sum; unsigned int max_bits, nonfinite; };
__device__ __forceinline__ void fp_flush(euler_flow_px* o, FpAcc& c) {
  if (c.sum) atomicAdd(reinterpret_cast<unsigned long long*>(&o->p_sum), c.sum);
  if (c.max_bits) atomicMax(reinterpret_cast<unsigned int*>(&o->max_p), c.max_bits);
  if (c.nonfinite) atomicAdd(&o->nonfinite, c.nonfinite);
  c.sum = 0ull; c.max_bits = 0u; c.nonfinite = 0u;
}

__global__ __launch_bounds__(256) void k_flow_pressure(const FpArgs a) {
  const unsigned int wave = blockIdx.x * 4u + (threadIdx.x >> 6);
  const int l = threadIdx.x & 63;
  if (wave >= (unsigned int)a.nbands * (unsigned int)a.runs) return;      // (a whole wave)
  const int band = a.band0 + (int)(wave / (unsigned int)a.runs), run = (int)(wave % (unsigned int)a.runs);
  const int y = band * 64 + l;
  if (y < a.by0 || y > a.by1) return;
  const int py = (int)(((unsigned long long)(a.by1 - y + 1) * (unsigned int)a.H - 1ull) / (unsigned int)a.Bh);      // the pixel row whose range holds y
  euler_flow_px* orow = a.out + (size_t)(py - a.py0) * a.W;
  const int t0 = a.tbase + run * 2 * FP_RUN;
  const double* base = a.p + ((size_t)band * a.g.TS + (size_t)t0) * 64 + 2 * l;      // (skew_index of record t0, lane l)
  const size_t rowi = (size_t)y * (size_t)a.g.X;
  FpAcc c = {0ull, 0u, 0u};
  int cur = -1;
  for (int r = 0; r < FP_RUN; ++r) {
    const int t = t0 + 2 * r;
    if (t > a.bx1 + 63) break;      // behind the box's last record in every lane
    const double2 pp = *reinterpret_cast<const double2*>(base + (size_t)r * 128);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int x = t + e - l;
      if (x < a.bx0 || x > a.bx1 || !fl_water1(a.solid, a.sink, a.count, rowi + (size_t)x)) continue;
      const int px = (int)(((unsigned long long)(x - a.bx0 + 1) * (unsigned int)a.W - 1ull) / (unsigned int)a.Bw);
      if (px != cur) { if (cur >= 0) fp_flush(orow + cur, c); cur = px; }
      const float pf = (float)(e ? pp.y : pp.x);
      if (pf == pf) {
        c.sum += fl_qp(pf);
        ob_max_bits(c.max_bits, pf > 0.f ? pf : 0.f);
      } else if (!fp_velocity_nan(a, x, y)) c.nonfinite += 1u;
    }
  }
  if (cur >= 0) fp_flush(orow + cur, c);
}

// the velocity part alone, on the handle's stream, into the records of S->flow_buf (tools/flow_cost.py times it through the KC_MISC class)
// plan: row slabs - the records go to this rank's share of the staging area, the pixel rows its rows touch only
static int fl_launch(euler_sim* S, int x0, int y0, int x1, int y1, int W, int H, const eu_slab_plan* plan = nullptr) {
  const int Xi = x1 - x0 + 1, Yi = y1 - y0 + 1;      // (the box's extent: npc and nsplit follow it)
  FlArgs a;
  a.solid = S->solid; a.sink = S->sink; a.count = S->count; a.u = S->u; a.v = S->v;
  a.tiles = eu_observe_tiles(S);
  a.X = S->X; a.W = W; a.H = H; a.out = (euler_flow_px*)S->flow_buf.p;
  a.bx0 = x0; a.by1 = y1; a.Bw = Xi; a.Bh = Yi;
  long long npc = (long long)FL_SPAN * W / Xi;      // pixel columns per workgroup: about FL_SPAN cells wide, at least one box, at most the table
  a.npc = (int)(npc < 1 ? 1 : (npc > FL_NPC ? FL_NPC : npc));
  const long long span = ((long long)a.npc * Xi + W - 1) / W, rows_max = (Yi + H - 1) / H, rows_min = Yi / H;
  long long ns = (span * rows_max + FL_WG_CELLS - 1) / FL_WG_CELLS;      // slices of a box's rows
  a.nsplit = (int)(ns < 1 ? 1 : (ns > rows_min ? rows_min : ns));
  a.py0 = 0; a.cy0 = y0; a.cy1 = y1; a.add = a.nsplit > 1;
  int Hl = H;      // pixel rows launched
  if (plan) {
    const int r = S->cfg.slab_rank;
    int rc = eu_observe_slab_clear_mine(S, plan, EU_OBS_REC_FLOW);
    if (rc || plan->cnt[r] == 0) return rc;      // (no row of the box is here: nothing to launch, nothing to contribute)
    a.out = (euler_flow_px*)eu_observe_slab_mine(S, plan, EU_OBS_REC_FLOW);
    a.py0 = plan->p_lo[r]; a.cy0 = plan->ya[r]; a.cy1 = plan->yb[r]; a.add = 1;
    Hl = plan->p_hi[r] - plan->p_lo[r] + 1;
  } else if (a.nsplit > 1) HIPCHK(hipMemsetAsync(S->flow_buf.p, 0, (size_t)W * H * sizeof(euler_flow_px), S->stream));
  const long long nwg = (long long)((W + a.npc - 1) / a.npc) * Hl * a.nsplit;      // (at most a workgroup per 256 cells: far below 2^31 on any grid euler_create accepts)
  const dim3 grid((unsigned)nwg);
  if (S->X % 4 == 0) LAUNCH(S, KC_MISC, (k_flow<4>), grid, dim3(FL_T), a);
  else LAUNCH(S, KC_MISC, (k_flow<1>), grid, dim3(FL_T), a);
  HIPCHK(hipGetLastError());
  return EULER_OK;
}

// the pressure part, behind the velocity part on the same stream: adds p_sum, max_p and the cells only a NaN pressure makes nonfinite
static int fp_launch(euler_sim* S, int x0, int y0, int x1, int y1, int W, int H, const eu_slab_plan* plan = nullptr) {
  FpArgs a;
  a.p = S->p; a.g = S->geom;
  a.solid = S->solid; a.sink = S->sink; a.count = S->count; a.u = S->u; a.v = S->v;
  a.W = W; a.H = H; a.bx0 = x0; a.by0 = y0; a.bx1 = x1; a.by1 = y1; a.Bw = x1 - x0 + 1; a.Bh = y1 - y0 + 1;
  a.band0 = y0 >> 6; a.nbands = (y1 >> 6) - a.band0 + 1;
  a.py0 = 0;
  a.out = (euler_flow_px*)S->flow_buf.p;
  if (plan) {      // the own bands the box crosses: the skewed p of a slab holds them (shifted by skew_off, and finished in memory)
    const int r = S->cfg.slab_rank;
    if (plan->cnt[r] == 0) return EULER_OK;
    a.band0 = plan->ya[r] >> 6; a.nbands = (plan->yb[r] >> 6) - a.band0 + 1;
    a.py0 = plan->p_lo[r];
    a.out = (euler_flow_px*)eu_observe_slab_mine(S, plan, EU_OBS_REC_FLOW);
  }
  a.tbase = x0 & ~1;      // records x0 ... x1 + 63 of a band hold the box's columns
  a.runs = (x1 + 63 - a.tbase) / (2 * FP_RUN) + 1;
  const long long waves = (long long)a.nbands * a.runs;
  LAUNCH(S, KC_MISC, k_flow_pressure, dim3((unsigned)((waves + 3) / 4)), dim3(256), a);
  HIPCHK(hipGetLastError());
  return EULER_OK;
}

extern "C" int euler_flow_raster(euler_sim* S, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t W, int32_t H, int32_t flags, euler_flow_px* out, size_t out_bytes) {
  const char* who = "euler_flow_raster";
  int rc = eu_observe_enter(S, who, nullptr, out, x0, y0, x1, y1);
  if (rc) return rc;
  if (W < 1 || H < 1 || W > x1 - x0 + 1 || H > y1 - y0 + 1) { eu_set_error("%s: a raster of %d x %d for a box of %d x %d cells", who, W, H, x1 - x0 + 1, y1 - y0 + 1); return EULER_EINVAL; }
  const size_t n = (size_t)W * (size_t)H;
  if (out_bytes != n * sizeof(euler_flow_px)) { eu_set_error("%s: %zu bytes given, %zu expected", who, out_bytes, n * sizeof(euler_flow_px)); return EULER_EINVAL; }
  if (flags & ~EULER_FLOW_PRESSURE) { eu_set_error("%s: unknown flag bits %d", who, flags & ~EULER_FLOW_PRESSURE); return EULER_EINVAL; }
  rc = eu_devbuf_reserve(S, who, "the records", &S->flow_buf, out_bytes);
  if (!rc && (flags & EULER_FLOW_PRESSURE)) rc = eu_pressure_current(S);      // (k_velocity_update_para leaves the last fmadds and the clamp to whoever looks)
  eu_slab_plan plan;
  const eu_slab_plan* pl = S->slab_on ? &plan : nullptr;
  if (pl) {      // collective: the own rows into this rank's share, the shares folded into the records on every rank
    const int rp = eu_observe_slab_plan(S, &plan, y0, y1, W, H);      // (the same on every rank)
    if (rp) return rp;
    rc = eu_observe_slab_open(S, who, rc, (size_t)plan.total * sizeof(euler_flow_px), EU_OBS_ROWS_FLOW);
  }
  if (!rc) rc = fl_launch(S, x0, y0, x1, y1, W, H, pl);
  if (!rc && (flags & EULER_FLOW_PRESSURE)) rc = fp_launch(S, x0, y0, x1, y1, W, H, pl);
  if (!rc && pl) rc = eu_observe_slab_fold(S, pl, EU_OBS_REC_FLOW, S->flow_buf.p);
  return rc ? rc : eu_observe_readback(S, out, &S->flow_buf, out_bytes);
}
