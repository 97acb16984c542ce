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
int      eu_interior_box_ok(int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t X, int32_t Y);   /* 1 <= x0 <= x1 <= X - 2 and 1 <= y0 <= y1 <= Y - 2: the test behind every box a caller hands in */
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
/* boxes: n records `stride` bytes apart that begin with x0, y0, x1, y1 as four int32_t (euler_force_box, euler_heat_box); out == NULL: the count only; the list must
 * have passed its check; (size_t)-1: no memory */
size_t   eu_force_tiles(const void* boxes, size_t stride, int32_t n, int32_t X, int32_t Y, eu_force_tile* out);
/* ... and only the entries of the tile rows [band_lo, band_hi) (clipped to the grid's), in the order eu_force_tiles lists them.  A tile lies in one 64-row band and a
 * row slab is cut at band boundaries, so over the ranks of a row-slab job these tables are a partition of the whole-grid one; a rank no box touches gets 0 entries */
size_t   eu_force_tiles_bands(const void* boxes, size_t stride, int32_t n, int32_t X, int32_t Y, int32_t band_lo, int32_t band_hi, eu_force_tile* out);
/* what the ranks of a row-slab job compare before euler_set_forcing / euler_set_heat change anything: FNV-1a over the record's bytes and the first nboxes boxes'
 * (slots beyond nboxes are not read); h == NULL - switching heat off - has a digest of its own */
uint64_t eu_forcing_digest(const euler_forcing* f, const euler_force_box* boxes);
uint64_t eu_heat_digest(const euler_heat* h, const euler_heat_box* boxes);
/* euler_set_heat (k_heat.hip, docs/heat.md): refusals 4 - 9 of include/euler.h in their order - the ones that need no device; live: the ambient of a handle whose
 * heat is on (NULL: off, any ambient passes).  The tile table of the heat boxes is the force boxes': eu_force_tiles with the stride of euler_heat_box */
int      eu_heat_check(const euler_heat* h, const euler_heat_box* boxes, int32_t X, int32_t Y, const float* live, char* why, size_t cap);   /* EULER_OK, or EULER_EINVAL with the reason in why */
/* the refusals of euler_heat_fill / euler_heat_set_field that need no device: the box, the value */
int      eu_heat_box_check(int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t X, int32_t Y, char* why, size_t cap);
int      eu_heat_value_ok(float x);   /* finite and at most 1e4 in size */
/* passive tracers (k_tracers.hip, docs/tracers.md): the refusals of euler_tracers_add that need no device, in its order - n > 0 with a null xy, count + n >
 * EULER_TRACERS_MAX, a position that is not finite or outside 1 <= x < X - 1, 1 <= y < Y - 1 (the first such index is named) */
int      eu_tracers_check(const float* xy, size_t n, size_t count, int32_t X, int32_t Y, char* why, size_t cap);   /* EULER_OK, or EULER_EINVAL with the reason in why */
/* the K x K lattice of a box of cells, K in {1, 2, 4}: cell x outer, cell y inner, i outer, j inner, at x + (i + 0.5f) / K, y + (j + 0.5f) / K (every term exact in
 * float32 below 2^21).  Returns the number of points, Bw * Bh * K * K; xy == NULL: the count only; 0: an empty box or another K */
size_t   eu_tracer_lattice(int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t K, float* xy);
/* moving bodies (k_bodies.hip, docs/bodies.md): the refusals of euler_set_bodies that need no device, in its order; the unit shifts that take a body from its
 * remembered origin to its target - all x shifts first, then y -; and the faces of a rectangle's perimeter */
int      eu_body_check(const euler_body* b, int32_t n, int32_t X, int32_t Y, char* why, size_t cap);   /* EULER_OK, or EULER_EINVAL with the reason in why */
/* the envelopes (k_envelope.hip, docs/envelope.md): channel is exactly one EULER_ENV_* bit -> its index 0 ... 3, else -1; and the words euler_envelope_set_field
 * accepts for it - arrival: 0xffffffff or a finite float >= 0, the others: a finite float >= +0 (no NaN, no -0.f) -: the index of the first bad word, (size_t)-1: none */
int      eu_envelope_index(int32_t channel);
size_t   eu_envelope_check_words(int32_t channel, const uint32_t* w, size_t n);
typedef struct eu_body_shift { int32_t axis, dir; } eu_body_shift;   /* axis 0: x, 1: y; dir +1 or -1 */
/* the number of unit shifts from (ox, oy) to (tx, ty), |tx - ox| + |ty - oy|; out (may be NULL) takes the first min(count, cap) of them */
int64_t  eu_body_plan(int32_t ox, int32_t oy, int32_t tx, int32_t ty, eu_body_shift* out, int64_t cap);
/* the strip a shift solidifies and the one it clears, inclusive boxes {x0, y0, x1, y1}, for a body of w x h at (ox, oy) BEFORE the shift */
void     eu_body_strips(int32_t ox, int32_t oy, int32_t w, int32_t h, eu_body_shift s, int32_t fill[4], int32_t clear[4]);
/* face k of the 2 h + 2 w perimeter faces of the rectangle at (ox, oy): k in [0, h): the left edge's u faces, bottom up; [h, 2 h): the right edge's;
 * [2 h, 2 h + w): the lower edge's v faces, left to right; then the upper edge's.  (fx, fy) is the cell whose u / v sample the face is, (cx, cy) the cell OUTSIDE the
 * body across the face */
typedef struct eu_body_face { int32_t axis, fx, fy, cx, cy; } eu_body_face;
#ifdef __HIPCC__
__host__ __device__
#endif
static inline int32_t eu_body_nfaces(int32_t w, int32_t h) { return 2 * h + 2 * w; }
#ifdef __HIPCC__
__host__ __device__
#endif
static inline eu_body_face eu_body_face_at(int32_t ox, int32_t oy, int32_t w, int32_t h, int32_t k) {
  eu_body_face f;
  if (k < h)              { f.axis = 0; f.fx = ox - 1;     f.fy = oy + k;           f.cx = ox - 1; f.cy = f.fy; }
  else if (k < 2 * h)     { f.axis = 0; f.fx = ox + w - 1; f.fy = oy + k - h;       f.cx = ox + w; f.cy = f.fy; }
  else if (k < 2 * h + w) { f.axis = 1; f.fx = ox + k - 2 * h;     f.fy = oy - 1;     f.cx = f.fx; f.cy = oy - 1; }
  else                    { f.axis = 1; f.fx = ox + k - 2 * h - w; f.fy = oy + h - 1; f.cx = f.fx; f.cy = oy + h; }
  return f;
}
/* marker density control (k_reseed.hip, docs/reseed.md): the refusals of euler_set_reseed that need no device, in its order; the limits a record stands for; the
 * sub-cell of a coordinate; and ONE pass restated sequentially over host arrays - what the kernels are held to */
#define EU_RESEED_DEFAULT_LIMIT 65536
#define EU_RESEED_MAX_LIMIT (1 << 20)
int      eu_reseed_check(const euler_reseed* r, char* why, size_t cap);   /* EULER_OK, or EULER_EINVAL with the reason in why; r must not be NULL */
#ifdef __HIPCC__
__host__ __device__
#endif
static inline int32_t eu_reseed_limit(int32_t given) { return given ? given : EU_RESEED_DEFAULT_LIMIT; }
/* m: a coordinate, c = floorf(m) as an int.  The subtraction is exact (Sterbenz, or c = 0), the product a power of two */
#ifdef __HIPCC__
__host__ __device__
#endif
static inline int32_t eu_reseed_subcell(float m, int32_t c) {
  const int32_t s = (int32_t)__builtin_floorf((m - (float)c) * 4.f);
  return s < 3 ? s : 3;
}
/* markers_xy holds *n markers and has room for max_markers; the totals are ADDED to stats (may be NULL).  EULER_EINVAL: a null array, a record eu_reseed_check
 * refuses, X or Y < 3; EULER_ENOMEM: no scratch.  Markers must lie inside the grid. */
int      eu_reseed_pass(const euler_reseed* r, int32_t X, int32_t Y, float* markers_xy, uint64_t* n, uint64_t max_markers, uint8_t* count, const uint8_t* prev_count,
                        const uint8_t* solid, const uint8_t* sink, const uint8_t* source, uint64_t* rng_state, euler_reseed_stats* stats);
/* The multilevel preconditioner's node grids and the plan of its cycle split by rows (k_mg.h, k_mg_split.hip, docs/solver_multilevel_row_slabs.md): everything that
 * follows from the grid's size and the ranks' band ranges alone.  Row ranges are half open, [lo, hi); an empty zone is {0, 0}. */
#ifndef MG_G0
#define MG_G0 8              /* level 0's node spacing in grid cells (k_mg.h) */
#endif
#define MG_RPB (64 / MG_G0)  /* node rows of level 0 per band */
#define MG_MAXLEV 12
#define MG_TOP_MAX 64        /* nodes of the dense top level at most (its inverse lives in LDS: 32 KB) */
#define MG_TAIL_MAX 1024     /* nodes of the first level the one-workgroup tail of k_mg_down takes: the ENTRY level */
#define MG_TAIL_LEVELS 4     /* stencil levels of the tail at most (1024 -> 272 -> 72 -> top would be 3) */
#define MG_SMALL_LEVEL0 16384 /* nodes of level 0 up to which the cycle runs as two launches of the general kernels, and is never split */
#define MG_GATHER_MAX 16384  /* the split cycle's GATHER level: the first of at most this many nodes */
#define MG_SETUP_HALO 6      /* rows of a level's operator that travel to either neighbour in the split setup */
#define MG_SPLIT_MAXR 64     /* ranks of a split cycle at most */
/* level l = nx[l] x ny[l] nodes at node off[l] of the pooled arrays (arrays of MG_MAXLEV), halved until at most MG_TOP_MAX are left; returns the number of levels,
 * EULER_EINVAL: more than MG_MAXLEV (or X, nbands < 1) */
int      eu_mg_levels(int32_t X, int32_t nbands, int32_t* nx, int32_t* ny, size_t* off);
int      eu_mg_entry_level(int32_t levels, const int32_t* nx, const int32_t* ny);   /* the first level of <= MG_TAIL_MAX nodes (the top level if none is) */
/* the gather level; 0: the cycle is not split.  forced (EULER_OPT_MG_SPLIT_LEVEL) < 0: never split, > 0: that level, the entry level at most */
int      eu_mg_gather_level(int32_t levels, const int32_t* nx, const int32_t* ny, int64_t forced);
typedef struct eu_mg_seg { int32_t level, row0, row1, off; } eu_mg_seg;
typedef struct eu_mg_split_plan {
  int32_t Lg, ranks, rank;
  int32_t I[MG_MAXLEV][MG_SPLIT_MAXR][2];   /* [level <= Lg][rank]: the node rows a rank's own tiles can contribute to (its share's support) */
  int32_t O[MG_MAXLEV][MG_SPLIT_MAXR][2];   /* [level <= Lg][rank]: the rows it OWNS - level 0: its bands' node rows; a coarser row belongs to the owner of the fine row under it */
  int32_t NR[MG_MAXLEV][2];                 /* [level < Lg] this rank: the node rows whose TRUE right-hand side its way up needs */
  int32_t NX[MG_MAXLEV][2];                 /* ... and the rows of x_l it computes */
  int32_t zs[2][MG_MAXLEV][2];              /* [side 0: the rank below / 1: above][level]: rows of this rank's share the neighbour on that side needs */
  int32_t zr[2][MG_MAXLEV][2];              /* rows of that neighbour's share this rank needs: zs[1] of rank r IS zr[0] of rank r + 1, and the other way round */
  int32_t zoff_s[2][MG_MAXLEV], zoff_r[2][MG_MAXLEV];   /* offsets inside a zone message, in doubles */
  int32_t zone;                             /* doubles of this rank's longest zone message (the job uses the maximum over the ranks) */
  int32_t beyond;                           /* 1: a rank other than the two neighbours contributes to rows this rank needs - the cycle cannot be split */
  int32_t setup_bad;                        /* 1: a rank owns fewer than MG_SETUP_HALO rows of a level below Lg, or this rank reads beyond its owned rows + halo: operators replicated */
  int32_t aslot;                            /* doubles per rank of the gather level's operator all-gather: 9 x the most rows a rank owns x nx[Lg] */
  int32_t win_rows, nsmall;                 /* window rows per rank at level Lg (the most over the ranks); doubles per all-gather slot: 2 + win_rows nx[Lg] */
  /* behind the exchange: the rows of NR whose right-hand side changes - a neighbour's share arrives, or leftovers outside the own support must go - as ascending
   * runs that do not touch, packed at off; overflow: more runs than the table holds (they are dropped, never written past it) */
  int32_t nseg, total, overflow;
  eu_mg_seg seg[4 * MG_MAXLEV];
} eu_mg_split_plan;
/* rank's plan for gather level Lg over the partition part_lo / part_hi (bands of the ny[0] / MG_RPB; ascending, no rank empty).  EULER_EINVAL: a null pointer, Lg outside
 * 1 ... levels - 1, nranks outside 2 ... MG_SPLIT_MAXR, such a partition, or counts beyond int32.  seg_cap: table entries to use (<= 4 MG_MAXLEV, which callers pass) */
int      eu_mg_split_plan_fill(eu_mg_split_plan* P, int32_t levels, const int32_t* nx, const int32_t* ny, int32_t Lg, int32_t nranks, int32_t rank,
                               const int32_t* part_lo, const int32_t* part_hi, int32_t seg_cap);
/* session files (snapshot.hip, include/euler.h "session files", docs/session.md): a version-4 snapshot in memory - composed, and parsed and checked whole, without a
 * device.  The SETT chunk's payload: every setting that can change a bit of a run and that the file does not otherwise fix; opt[k] is the value of EULER_OPT_* key k
 * (opt[0] and the keys beyond nopts - 1 are 0) */
#define EU_SESSION_OPTS 32
typedef struct eu_session_settings {      /* 320 bytes, no padding */
  int32_t  max_iterations, dot_mode, precond, tile_records, sweep_mode, max_substeps, rainbow, pcg_precision, resident, pcg_poll_interval;
  uint32_t viscosity_bits, frame_time_bits;      /* the floats' bit patterns */
  double   tol;
  int32_t  nopts, reserved;                      /* EULER_OPT__COUNT of the writer; 0 */
  int64_t  opt[EU_SESSION_OPTS];
} eu_session_settings;
/* What a session holds beside the arrays of the core.  The byte pointers may be unaligned (a chunk begins wherever the markers end): read them with memcpy.  For the
 * composer they point to the caller's arrays, for the parser into the buffer it was given. */
typedef struct eu_session {
  int32_t  X, Y, dye;                        /* dye: the six dye arrays are present (bit 0 of the header's reserved word) */
  uint64_t n_markers, rng_state;
  int32_t  source_exhausted;
  uint64_t frames, total_substeps, total_pcg_iterations;
  const unsigned char* solid;                /* the file's own solid grid, X * Y bytes (set by the parser; the composer does not read it) */
  double   time;
  euler_forcing forcing;  euler_force_box force_boxes[EULER_FORCE_BOXES_MAX];
  int32_t  heat_on;
  euler_heat heat;        euler_heat_box heat_boxes[EULER_HEAT_BOXES_MAX];
  const unsigned char* heat_field;           /* X * Y floats where heat_on, else NULL */
  uint64_t n_tracers;
  const unsigned char* tracers;              /* n_tracers records of 32 bytes */
  int32_t  n_bodies;
  euler_body bodies[EULER_BODIES_MAX];
  int32_t  body_ox[EULER_BODIES_MAX], body_oy[EULER_BODIES_MAX];
  euler_reseed reseed;
  euler_reseed_stats reseed_stats;
  eu_session_settings settings;
  /* the STAT chunk: what euler_stats reports beside the header's three counters and the marker state */
  int32_t  last_substeps, last_pcg_iterations;
  double   last_residual;
  float    last_dt;
  uint64_t marker_dt_events, marker_multi_events;
} eu_session;
uint64_t eu_fnv1a64(uint64_t h, const void* p, size_t n);   /* h = EU_FNV_BASIS to begin */
#define EU_FNV_BASIS 14695981039346656037ull
size_t   eu_session_core_bytes(int32_t X, int32_t Y, int32_t dye, uint64_t n_markers);   /* header, arrays and markers: where the chunks begin */
size_t   eu_session_chunk_bytes(const eu_session* s);          /* all chunks, END included, without the trailer */
size_t   eu_session_put_chunks(const eu_session* s, unsigned char* out);   /* writes them; returns eu_session_chunk_bytes */
/* The whole file in buf: header, sizes, checksum, every chunk in its order and every record through its host check; reads no byte beyond n, writes only *out and why.
 * X, Y, dye, max_markers: the loading handle's.  EULER_EIO: truncated or the checksum fails; EULER_EINVAL: everything else. */
int      eu_session_parse(const void* buf, size_t n, int32_t X, int32_t Y, int32_t dye, uint64_t max_markers, eu_session* out, char* why, size_t cap);
/* 0: the settings agree; 1: why names the first field that differs, with both values.  Not compared: the options that cannot change a bit of a whole-grid run and
 * are not settings of it (docs/session.md) */
int      eu_session_settings_diff(const eu_session_settings* file, const eu_session_settings* handle, char* why, size_t cap);
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
