/* euler_host.h — internal declarations shared by the host C file and the HIP driver. */
#ifndef EULER_HOST_H
#define EULER_HOST_H
#include "euler.h"
#ifdef __cplusplus
extern "C" {
#endif
uint32_t euler_rng_next_u32(uint64_t* state);
float    euler_rng_next_float(uint64_t* state);
int      euler_half_tank_grids(int32_t X, int32_t Y, uint8_t* solid, uint8_t* source, uint8_t* sink, uint8_t* fluid);
int      euler_half_tanks_grids(int32_t X, int32_t Y, int32_t tanks, uint8_t* solid, uint8_t* source, uint8_t* sink, uint8_t* fluid);
uint64_t euler_rng_jump(uint64_t state, uint64_t steps);   /* xorshift64* state after `steps` more steps */
int      euler_seed_markers_rows(const uint8_t* fluid, int32_t X, int32_t Y, int32_t row_lo, int32_t row_hi, uint64_t* rng_state,
                                 float* markers_xy, uint32_t* keys, uint64_t cap, uint64_t* n_total, uint64_t* n_kept);
#define EULER_RNG_SEED 0x9bd185c449534b91ull /* main.c:204 */
/* euler_gauges (k_gauges.hip, docs/gauges.md): the list checked and cut along the 64 x 64 tile grid.  A chunk lies in one tile, hence in one band of the skewed arrays */
typedef struct eu_gauge_chunk { int32_t gauge, kind, x0, y0, x1, y1; } eu_gauge_chunk;
int      eu_gauge_check(const euler_gauge* g, int32_t n, int32_t X, int32_t Y, const char** what);   /* the index of the first gauge refused (what: why), -1: none */
size_t   eu_gauge_chunks(const euler_gauge* g, int32_t n, eu_gauge_chunk* out);   /* out == NULL: the count only; the list must have passed eu_gauge_check */
/* ... and only the chunks of the 64-row bands [band_lo, band_hi), in the order eu_gauge_chunks lists them: a chunk lies in one band, so over the ranks of a
 * row-slab job these tables are a partition of the whole-grid one */
size_t   eu_gauge_chunks_bands(const euler_gauge* g, int32_t n, int32_t band_lo, int32_t band_hi, eu_gauge_chunk* out);
/* The observer passes on row slabs (k_observe_slab.hip, docs/observer_passes.md "On row slabs"): what every rank works out alike about a box of rows
 * [y0, y1] shown as H pixel rows of W records, from the ranks' band ranges alone.  Rank r reduces the box's rows inside its own, [ya[r], yb[r]] (ya > yb: none),
 * into the pixel rows they touch, [p_lo[r], p_hi[r]] (p_lo > p_hi: none) with py(y) = ((y1 - y + 1) H - 1) / (y1 - y0 + 1), the kernels' formula; its partial records
 * sit at record off[r] of the staging area, cnt[r] = (p_hi - p_lo + 1) W of them, rank after rank without gaps: total <= (H + nranks - 1) W. */
#define EU_SLAB_PLAN_MAXR 16
typedef struct eu_slab_plan {
  int32_t nranks, W, H, y0, y1;
  int32_t ya[EU_SLAB_PLAN_MAXR], yb[EU_SLAB_PLAN_MAXR];
  int32_t p_lo[EU_SLAB_PLAN_MAXR], p_hi[EU_SLAB_PLAN_MAXR];
  int64_t off[EU_SLAB_PLAN_MAXR], cnt[EU_SLAB_PLAN_MAXR];
  int64_t total;
} eu_slab_plan;
/* the rows of [y0, y1] inside the bands [band_lo, band_hi) of a grid of Y rows; returns 1 and [*ya, *yb] if there are any, else 0 and *ya > *yb */
int      eu_slab_clip_rows(int32_t band_lo, int32_t band_hi, int32_t Y, int32_t y0, int32_t y1, int32_t* ya, int32_t* yb);
/* the plan of a raster; EULER_EINVAL: nranks outside 1 ... EU_SLAB_PLAN_MAXR, band ranges that are not ascending, an empty box or W, H < 1 or H above the box's rows */
int      eu_slab_plan_raster(eu_slab_plan* P, int32_t nranks, const int32_t* band_lo, const int32_t* band_hi, int32_t Y, int32_t y0, int32_t y1, int32_t W, int32_t H);
/* the plan of n records that EVERY rank contributes whole (euler_diagnostics: n = 1, euler_gauges): one pixel row of n records, rank r's copy at record r n */
int      eu_slab_plan_flat(eu_slab_plan* P, int32_t nranks, int32_t n);
/* the byte offsets and counts of the all-gather (euler_comm_ops.allgather) for records of rec_bytes */
void     eu_slab_plan_bytes(const eu_slab_plan* P, int64_t rec_bytes, int64_t* off, int64_t* cnt);
/* the ranks whose partial records hold pixel row py: [*first, *last] (they are consecutive: rows ascend with the rank, pixel rows descend); the fold kernel's loop */
int      eu_slab_plan_contributors(const eu_slab_plan* P, int32_t py, int32_t* first, int32_t* last);
/* euler_set_forcing (k_forcing.hip, docs/forcing.md): the record and the list checked, and the list cut along the 64 x 64 tile grid into a TILE TABLE: one entry per
 * tile that any box touches, with the boxes that touch it as a bit set - bit k = box k, walked from bit 0 up: the ascending list (at most 64 boxes) */
typedef struct eu_force_tile { int32_t tx, ty; uint64_t boxes; } eu_force_tile;
int      eu_forcing_check(const euler_forcing* f, const euler_force_box* boxes, int32_t X, int32_t Y, char* why, size_t cap);   /* EULER_OK, or EULER_EINVAL with the reason in why */
size_t   eu_force_tiles(const euler_force_box* b, int32_t n, int32_t X, int32_t Y, eu_force_tile* out);   /* out == NULL: the count only; the list must have passed eu_forcing_check; (size_t)-1: no memory */
/* passive tracers (k_tracers.hip, docs/tracers.md): the refusals of euler_tracers_add that need no device, in its order - n > 0 with a null xy, count + n >
 * EULER_TRACERS_MAX, a position that is not finite or outside 1 <= x < X - 1, 1 <= y < Y - 1 (the first such index is named) */
int      eu_tracers_check(const float* xy, size_t n, size_t count, int32_t X, int32_t Y, char* why, size_t cap);   /* EULER_OK, or EULER_EINVAL with the reason in why */
/* the K x K lattice of a box of cells, K in {1, 2, 4}: cell x outer, cell y inner, i outer, j inner, at x + (i + 0.5f) / K, y + (j + 0.5f) / K (every term exact in
 * float32 below 2^21).  Returns the number of points, Bw * Bh * K * K; xy == NULL: the count only; 0: an empty box or another K */
size_t   eu_tracer_lattice(int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t K, float* xy);
#ifdef __cplusplus
}
#endif
/* the pixel of euler_overview_box's geometry that covers column c (0 <= c < B) of a box of B columns shown as W <= B pixels - rows alike, counted from the top:
 * the px with floor(px B / W) <= c < floor((px + 1) B / W).  floor(px B / W) <= c  <=>  px B < (c + 1) W  <=>  px <= ((c + 1) W - 1) / B */
#ifdef __HIPCC__
__host__ __device__
#endif
static inline int32_t eu_tracer_pixel(int32_t c, int32_t B, int32_t W) { return (int32_t)((((int64_t)c + 1) * W - 1) / B); }
/* eu_slab_plan_contributors, shared with the fold kernel: the first and the last rank whose pixel rows hold py (first > last: none) */
#ifdef __HIPCC__
__host__ __device__
#endif
static inline void eu_slab_row_ranks(const eu_slab_plan* P, int32_t py, int32_t* first, int32_t* last) {
  int32_t f = P->nranks, l = -1;
  for (int32_t r = 0; r < P->nranks; ++r)
    if (P->p_lo[r] <= py && py <= P->p_hi[r]) { if (r < f) f = r; l = r; }
  *first = f; *last = l;
}
#endif
