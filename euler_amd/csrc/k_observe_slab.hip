// k_observe_slab.hip — the read-only observer passes on a row-slab handle (docs/observer_passes.md "On row slabs"): what turns the ranks' partial records into the
// whole-grid records on every rank.
//
// A pass's kernels reduce, on each rank, the rows of the box that the rank owns (the row clip of k_overview / k_flow / k_diagnostics, the own chunks of k_gauges)
// into this rank's share of ONE staging area laid out rank after rank (eu_slab_plan, euler_host.c: every rank works the same plan out of the partition).  The shares
// travel by euler_comm_ops.allgather as bytes - the all-reduce carries doubles, and the sums reach 2^61 - and k_observe_fold folds them into the pass's own buffer,
// from which eu_observe_readback returns them.  Every field of a record is an integer sum, an integer extreme or a maximum of bit patterns: the fold of the partial
// records IS the record a whole-grid handle forms, bit for bit, in whatever order.
//
// The fold: one thread owns one output record - lanes along the pixels of a row - and loops over the at most nranks shares that hold its pixel row, a whole record per
// vector load (16 bytes where the record's size keeps it aligned, else 8); it adds, or takes the minimum or maximum of, 32-bit words and adds 64-bit ones as a small per-type table
// says.  No atomics, no order between ranks.
#include "k_pcg.h"

enum { FO_ADD = 0, FO_MAX, FO_MIN, FO_ADD64, FO_HI };      // a 32-bit word: added, max, min (unsigned); the low word of a 64-bit sum; its high word (folded with the low one)
#define FO_MAXW 22
struct FoldOps { unsigned char op[FO_MAXW + 2]; };

#define A FO_ADD
#define X FO_MAX
#define N FO_MIN
#define Q FO_ADD64, FO_HI
static const FoldOps fold_ops[EU_OBS_REC__COUNT] = {
  {{A, A, A, A, A, X, Q, Q, Q}},                                     // euler_overview_px: cells solid sink water marks | max_speed2 | dye[3]
  {{A, A, A, A, Q, Q, Q, Q, Q, Q, Q, X, X, X, A}},                   // euler_flow_px: cells water nodes nonfinite | u_pos ... w_neg p_sum | max_speed2 max_abs_w max_p | reserved
  {{Q, Q, Q, Q, Q, Q, Q, Q, Q, X, A, X, X}},                         // euler_diag: cells ... ke_lo | count_max | nonfinite | max_div max_speed2
  {{A, A, N, X, N, X, A, A, Q, Q, Q, Q, X, X}},                      // euler_gauge_rec: cells fluid | lo_x hi_x lo_y hi_y | terms nonfinite | a_pos ... b_neg | max_a max_b
  {{A, A, Q, Q, X, X}},                                              // euler_heat_px: cells water | t_pos t_neg | max_above max_below
};
#undef A
#undef X
#undef N
#undef Q
static const int fold_words[EU_OBS_REC__COUNT] = {12, 22, 22, 18, 8};
static_assert(sizeof(euler_overview_px) == 48 && sizeof(euler_flow_px) == 88 && sizeof(euler_diag) == 88 && sizeof(euler_gauge_rec) == 72, "the fold tables are written for these records");
static_assert(offsetof(euler_overview_px, max_speed2) == 20 && offsetof(euler_overview_px, dye) == 24, "euler_overview_px: five counts, a maximum, three 64-bit sums");
static_assert(offsetof(euler_flow_px, u_pos) == 16 && offsetof(euler_flow_px, max_speed2) == 72 && offsetof(euler_flow_px, reserved) == 84, "euler_flow_px: four counts, seven 64-bit sums, three maxima");
static_assert(offsetof(euler_diag, count_max) == 72 && offsetof(euler_diag, nonfinite) == 76 && offsetof(euler_diag, max_div) == 80, "euler_diag: nine 64-bit sums, a maximum, a count, two maxima");
static_assert(sizeof(euler_heat_px) == 32 && offsetof(euler_heat_px, t_pos) == 8 && offsetof(euler_heat_px, max_above) == 24, "euler_heat_px: two counts, two 64-bit sums, two maxima");
static_assert(offsetof(euler_gauge_rec, lo_x) == 8 && offsetof(euler_gauge_rec, terms) == 24 && offsetof(euler_gauge_rec, a_pos) == 32 && offsetof(euler_gauge_rec, max_a) == 64, "euler_gauge_rec");

size_t eu_observe_rec_bytes(int type) { return (size_t)fold_words[type] * 4; }

struct FoldArgs {
  const unsigned int* stage;      // the gathered shares: rank r's records from record plan.off[r] on, its pixel rows plan.p_lo[r] ... plan.p_hi[r]
  unsigned int* dst;              // plan.W x plan.H records
  eu_slab_plan plan;
  FoldOps ops;
};

// NW: 32-bit words of a record; VW: words per load (4 where NW * 4 is a multiple of 16, so that every record of a 16-byte aligned area is)
template <int NW, int VW>
__global__ __launch_bounds__(256) void k_observe_fold(const FoldArgs a) {
  typedef unsigned int vec_t __attribute__((ext_vector_type(VW)));
  static_assert(NW % VW == 0 && NW <= FO_MAXW, "whole vectors");
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, W = (size_t)a.plan.W;
  if (idx >= W * (size_t)a.plan.H) return;
  const int py = (int)(idx / W);
  const size_t px = idx % W;
  int first, last;
  eu_slab_row_ranks(&a.plan, py, &first, &last);
  unsigned int acc[NW];
#pragma unroll
  for (int k = 0; k < NW; ++k) acc[k] = a.ops.op[k] == FO_MIN ? 0xffffffffu : 0u;
  for (int r = 0; r < a.plan.nranks; ++r) {      // (r is uniform: the plan is read with scalar loads; at most nranks shares hold a pixel row)
    if (r < first || r > last) continue;
    const vec_t* src = reinterpret_cast<const vec_t*>(a.stage + ((size_t)a.plan.off[r] + (size_t)(py - a.plan.p_lo[r]) * W + px) * NW);
    unsigned int w[NW];
#pragma unroll
    for (int j = 0; j < NW / VW; ++j) {
      const vec_t t = src[j];
#pragma unroll
      for (int e = 0; e < VW; ++e) w[j * VW + e] = t[e];
    }
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      const int op = a.ops.op[k];      // (uniform)
      if (op == FO_ADD) acc[k] += w[k];
      else if (op == FO_MAX) acc[k] = w[k] > acc[k] ? w[k] : acc[k];
      else if (op == FO_MIN) acc[k] = w[k] < acc[k] ? w[k] : acc[k];
      else if (op == FO_ADD64) {
        const unsigned long long s = (((unsigned long long)acc[k + 1] << 32) | acc[k]) + (((unsigned long long)w[k + 1] << 32) | w[k]);
        acc[k] = (unsigned int)s; acc[k + 1] = (unsigned int)(s >> 32);
      }
    }
  }
  vec_t* dst = reinterpret_cast<vec_t*>(a.dst + idx * NW);
#pragma unroll
  for (int j = 0; j < NW / VW; ++j) {
    vec_t t;
#pragma unroll
    for (int e = 0; e < VW; ++e) t[e] = acc[j * VW + e];
    dst[j] = t;
  }
}

int eu_observe_slab_plan(const euler_sim* S, eu_slab_plan* P, int y0, int y1, int W, int H) {
  if (eu_slab_plan_raster(P, S->cfg.slab_nranks, S->part_lo, S->part_hi, S->Y, y0, y1, W, H)) {
    eu_set_error("row slabs: no plan for rows [%d, %d] as %d x %d records over %d ranks", y0, y1, W, H, S->cfg.slab_nranks);
    return EULER_EINVAL;
  }
  return EULER_OK;
}

int eu_observe_slab_open(euler_sim* S, const char* who, int local_rc, size_t stage_bytes, int rows) {
  int rc = local_rc;
  if (!rc && stage_bytes) rc = eu_devbuf_reserve(S, who, "the ranks' partial records", &S->obs_stage_buf, stage_bytes);
  int worst = rc;
  const int rs = eu_slab_status_sync(S, rc, &worst);      // (a rank that could not allocate must not leave the others waiting in the all-gather)
  if (rs) return rs;
  if (worst) {
    if (!rc) eu_set_error("%s: another rank could not reserve its device buffers", who);
    return rc ? rc : EULER_ENOMEM;
  }
  return eu_slab_exchange_observed(S, rows);
}

int eu_observe_slab_clear_mine(euler_sim* S, const eu_slab_plan* P, int type) {
  const size_t bytes = (size_t)P->cnt[S->cfg.slab_rank] * eu_observe_rec_bytes(type);
  if (bytes) HIPCHK(hipMemsetAsync(eu_observe_slab_mine(S, P, type), 0, bytes, S->stream));
  return EULER_OK;
}

int eu_observe_slab_gather_in_place(euler_sim* S, void* base, const int64_t* off, const int64_t* cnt) {
  COMM_CALL(S->bulk.allgather(S->bulk.ctx, base, off, cnt));
  return EULER_OK;
}

int eu_observe_slab_fold(euler_sim* S, const eu_slab_plan* P, int type, void* dst) {
  int64_t off[EU_SLAB_PLAN_MAXR], cnt[EU_SLAB_PLAN_MAXR];
  eu_slab_plan_bytes(P, (int64_t)eu_observe_rec_bytes(type), off, cnt);
  int rc = eu_observe_slab_gather_in_place(S, S->obs_stage_buf.p, off, cnt);
  if (rc) return rc;
  FoldArgs a;
  a.stage = (const unsigned int*)S->obs_stage_buf.p; a.dst = (unsigned int*)dst; a.plan = *P; a.ops = fold_ops[type];
  const dim3 grid(eu_blocks((size_t)P->W * (size_t)P->H, 256));
  if (type == EU_OBS_REC_OVERVIEW) LAUNCH(S, KC_MISC, (k_observe_fold<12, 4>), grid, dim3(256), a);
  else if (type == EU_OBS_REC_GAUGE) LAUNCH(S, KC_MISC, (k_observe_fold<18, 2>), grid, dim3(256), a);
  else if (type == EU_OBS_REC_HEAT) LAUNCH(S, KC_MISC, (k_observe_fold<8, 4>), grid, dim3(256), a);
  else LAUNCH(S, KC_MISC, (k_observe_fold<22, 2>), grid, dim3(256), a);
  HIPCHK(hipGetLastError());
  return EULER_OK;
}
