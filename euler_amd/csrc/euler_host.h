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
#endif
