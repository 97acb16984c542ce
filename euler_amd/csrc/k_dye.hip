// k_dye.hip — the `--rainbow` dye (reference main.c:75-83): three cell-centred colour fields that are
// coloured at init (colorize, main.c:187-201), extended into new fluid cells (extrapolate(.., P),
// main.c:859-863), refreshed at source cells (main.c:283,292-294) and advected with the flow
// (advect_p + the whole-array memcpy, main.c:424-438, 873-882).  Cosmetic: nothing here feeds back
// into the flow.  Element-wise gathers over row-major arrays, the three channels share one launch.
#include "euler_dev.h"
#include "k_transport.h"

// misc/color.h:16-34: period 6, values in [0, 1]
__device__ __forceinline__ float hsv_basis(float t) {
  t -= 6.f * floorf(1.f / 6 * t);
  if (t < 0.f) t += 6.f;
  if (t < 1.f) return t;
  if (t < 3.f) return 1.f;
  if (t < 4.f) return 4.f - t;
  return 0.f;
}

// colorize (main.c:187-201): fluid cells only; k_initial_color_period = 60 cells (main.c:83)
__global__ __launch_bounds__(256) void k_colorize(float* r, float* g, float* b, const uint8_t* __restrict__ count,
                                                  const uint8_t* __restrict__ source, int X, int y0, int y1) {   // rows [y0, y1) of this rank
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = y0 + blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= X || y >= y1) return;
  const size_t i = (size_t)y * X + x;
  if (!count[i]) return;
  float t = 0.f;
  if (!source[i]) t = (x + y) * 6.f / 60.f;
  r[i] = hsv_basis(t + 2.f);
  g[i] = hsv_basis(t);
  b[i] = hsv_basis(t - 2.f);
}

// extrapolate(q, P) (main.c:158-185) for the three channels: a cell that just became fluid takes the mean
// of its previously-fluid 3x3 neighbours, summed y-major then x.  In place is race-free (writes go to cells
// without the prev-fluid property, reads to cells with it).
__global__ __launch_bounds__(256) void k_extrapolate_dye(float* r, float* g, float* b, const uint8_t* __restrict__ prev,
                                                         const uint8_t* __restrict__ cur, int X, int Y, int ry0, int ry1) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = ry0 + blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= X || y >= ry1) return;
  const size_t i = (size_t)y * X + x;
  if (prev[i] || !cur[i]) return;
  const int x0 = x > 0 ? x - 1 : 0, x1 = x + 1 < X ? x + 1 : X - 1;
  const int y0 = y > 0 ? y - 1 : 0, y1 = y + 1 < Y ? y + 1 : Y - 1;
  float tr = 0.f, tg = 0.f, tb = 0.f;
  int n = 0;
  for (int yy = y0; yy <= y1; ++yy)
    for (int xx = x0; xx <= x1; ++xx) {
      const size_t j = (size_t)yy * X + xx;
      if (prev[j]) { tr += r[j]; tg += g[j]; tb += b[j]; ++n; }
    }
  r[i] = tr / n; g[i] = tg / n; b[i] = tb / n;   // n == 0 -> 0/0 like the Release reference
}

// the source colour (main.c:283,292-294): every source cell, every substep
__global__ __launch_bounds__(256) void k_dye_sources(float* r, float* g, float* b, const uint8_t* __restrict__ source,
                                                     size_t i0, size_t C, float t) {   // cells [i0, i0 + C): this rank's rows
  const size_t i = i0 + (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= i0 + C || !source[i]) return;
  r[i] = hsv_basis(t + 2.f);
  g[i] = hsv_basis(t);
  b[i] = hsv_basis(t - 2.f);
}

// advect_p (main.c:424-438) for the three channels; only fluid cells of the outputs are written.  RK2 (EULER_OPT_ADVECT_RK2): the back-trace starts from the
// velocity at the midpoint of the face average (k_transport.h eu_trace)
template <bool RK2>
__global__ __launch_bounds__(256) void k_advect_dye(const float* __restrict__ r, const float* __restrict__ g,
                                                    const float* __restrict__ b, float* __restrict__ rout,
                                                    float* __restrict__ gout, float* __restrict__ bout,
                                                    const float* __restrict__ u, const float* __restrict__ v, GridRef gr, float dt, int y0, int y1) {
  const int X = gr.X;
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = y0 + blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= X || y >= y1) return;
  const size_t i = (size_t)y * X + x;
  if (!gr.count[i]) return;                     // never fluid on the border ring (all sink): i - X, i - 1 exist
  const float dy = (v[i] + v[i - X]) / 2;
  const float dx = (u[i] + u[i - 1]) / 2;
  const EuTrace t = eu_trace<EU_SPACE_P, RK2, false>(gr, u, v, (float)x, (float)y, dx, dy, dt);
  rout[i] = eu_interp<0>(gr, r, t.px, t.py);
  gout[i] = eu_interp<0>(gr, g, t.px, t.py);
  bout[i] = eu_interp<0>(gr, b, t.px, t.py);
}

// EULER_OPT_ADVECT_MACCORMACK, the correction pass of one or two channels (q1 null: one) behind k_advect_dye<RK2> (docs/advection_maccormack.md): per fluid cell the forward
// trace again (its value and the limiter's lo / hi), the backward trace - the same code with -dt - into the forward result qf, half the round-trip error added, the result
// clamped.  Every other cell takes qf's value: out is what the whole-array copy moves into g_r / g_g / g_b, as main.c:875-881 moves the scratch array
template <bool RK2>
__global__ __launch_bounds__(256) void k_mc_correct_dye(const float* __restrict__ q0, const float* __restrict__ qf0, float* __restrict__ out0,
                                                        const float* __restrict__ q1, const float* __restrict__ qf1, float* __restrict__ out1,
                                                        const float* __restrict__ u, const float* __restrict__ v, GridRef gr, float dt, int y0, int y1) {
  const int X = gr.X;
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = y0 + blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= X || y >= y1) return;
  const size_t i = (size_t)y * X + x;
  if (!gr.count[i]) {
    out0[i] = qf0[i];
    if (q1) out1[i] = qf1[i];
    return;
  }
  const float dy = (v[i] + v[i - X]) / 2;
  const float dx = (u[i] + u[i - 1]) / 2;
  const EuTrace t = eu_trace<EU_SPACE_P, RK2, true>(gr, u, v, (float)x, (float)y, dx, dy, dt);
  out0[i] = eu_mc_value<0>(gr, q0, qf0, q0[i], t);
  if (q1) out1[i] = eu_mc_value<0>(gr, q1, qf1, q1[i], t);
}

static inline dim3 cell_grid(const euler_sim* S) { return dim3((S->X + 63) / 64, (S->row_hi - S->row_lo + 3) / 4); }   // this rank's rows (all of them without slabs)

int eu_launch_colorize(euler_sim* S) {
  if (!S->dye[0]) return EULER_OK;
  LAUNCH(S, KC_MISC, k_colorize, cell_grid(S), dim3(256), S->dye[0], S->dye[1], S->dye[2], S->count, S->source, S->X, S->row_lo, S->row_hi);
  return EULER_OK;
}

int eu_launch_dye_extrapolate(euler_sim* S) {
  if (!S->dye[0]) return EULER_OK;
  LAUNCH(S, KC_EXTRAPOLATE, k_extrapolate_dye, cell_grid(S), dim3(256), S->dye[0], S->dye[1], S->dye[2], S->prev_count, S->count, S->X, S->Y, S->row_lo, S->row_hi);
  return EULER_OK;
}

int eu_launch_dye_sources(euler_sim* S) {
  if (!S->dye[0] || S->n_source_cells == 0) return EULER_OK;
  // k_source_color_period = 10 s (main.c:82); g_frame_count is a uint16_t (main.c:88) = frames completed so far
  const float t = 0.6f / 10.f * (uint16_t)S->stats.frames;
  const size_t i0 = (size_t)S->row_lo * S->X, n = (size_t)(S->row_hi - S->row_lo) * S->X;
  LAUNCH(S, KC_SOURCES, k_dye_sources, dim3(eu_blocks(n, 256)), dim3(256), S->dye[0], S->dye[1], S->dye[2], S->source, i0, n, t);
  return EULER_OK;
}

int eu_launch_dye_advect(euler_sim* S, float dt) {
  if (!S->dye[0]) return EULER_OK;
  const GridRef g = eu_grid_ref(S);
  const bool rk2 = S->opt[EULER_OPT_ADVECT_RK2] != 0;      // (never on a row slab: euler_set_option refuses it there)
  eu_flag(rk2, [&](auto R) {
    LAUNCH(S, KC_ADVECT_VELOCITY, k_advect_dye<decltype(R)::value>, cell_grid(S), dim3(256), S->dye[0], S->dye[1], S->dye[2], S->dye[3], S->dye[4], S->dye[5],
           S->u, S->v, g, dt, S->row_lo, S->row_hi);
  });
  // memcpy(g_r, g_rtmp, sizeof(g_r)) x3 (main.c:875,878,881): the WHOLE scratch array, stale non-fluid entries included (a row slab: its own rows)
  const size_t o = (size_t)S->row_lo * S->X, n = (size_t)(S->row_hi - S->row_lo) * S->X;
  if (S->opt[EULER_OPT_ADVECT_MACCORMACK]) {      // (a whole-grid handle): the corrected r, g into the velocity scratch, copied over the old ones; then b the same way
    float* sc[2] = {S->mc_u, S->mc_v};
    auto correct = [&](const float* q0, const float* qf0, float* out0, const float* q1, const float* qf1, float* out1) {
      eu_flag(rk2, [&](auto R) {
        LAUNCH(S, KC_ADVECT_VELOCITY, k_mc_correct_dye<decltype(R)::value>, cell_grid(S), dim3(256), q0, qf0, out0, q1, qf1, out1, S->u, S->v, g, dt, S->row_lo, S->row_hi);
      });
    };
    correct(S->dye[0], S->dye[3], sc[0], S->dye[1], S->dye[4], sc[1]);
    for (int k = 0; k < 2; ++k) HIPCHK(hipMemcpyAsync(S->dye[k] + o, sc[k] + o, n * sizeof(float), hipMemcpyDeviceToDevice, S->stream));
    correct(S->dye[2], S->dye[5], sc[0], nullptr, nullptr, nullptr);
    HIPCHK(hipMemcpyAsync(S->dye[2] + o, sc[0] + o, n * sizeof(float), hipMemcpyDeviceToDevice, S->stream));
    return EULER_OK;
  }
  for (int k = 0; k < 3; ++k) HIPCHK(hipMemcpyAsync(S->dye[k] + o, S->dye[3 + k] + o, n * sizeof(float), hipMemcpyDeviceToDevice, S->stream));
  return EULER_OK;
}
