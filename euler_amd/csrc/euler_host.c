/*
 * euler_host.c — host-only C parts of libeuler_hip.so: scenario text -> cell grids, the
 * xorshift64* stream, initial marker seeding, the ASCII frame formatter, and the formatters of the
 * whole-domain overview's records (text through the same frame formatter, RGB), the magnified frame of the viewport, the values derived from a diagnostics record,
 * the painter that shows a field of the flow raster through those formatters, the host side of the batched gauges (list check, chunk table, derived values), and the host side of the forcing (defaults, the uniform acceleration at a time, the check of
 * the record and its boxes, the tile table).
 *
 * These are the pieces of the reference's sim_init (main.c:209-274) and draw_rows
 * (main.c:914-951) that never touch the hot path; they run once (init) or over a terminal-sized
 * window (render), so they stay on the host.  Everything here is exported through include/euler.h
 * and usable without a GPU.
 */
#include "euler_host.h"

#include <pthread.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* ---- xorshift64* high half (misc/rng.c:5-20) and randf (main.c:203-207) ------------------- */

uint32_t euler_rng_next_u32(uint64_t* state) {
  uint64_t x = *state;
  x ^= x >> 12;
  x ^= x << 25;
  x ^= x >> 27;
  *state = x;
  return (uint32_t)((x * 0x2545F4914F6CDD1Dull) >> 32);
}

float euler_rng_next_float(uint64_t* state) {
  /* closed [0,1]: divide by UINT32_MAX in double, then narrow (main.c:206) */
  return (float)(euler_rng_next_u32(state) / (double)UINT32_MAX);
}

/* Jump-ahead: the state update is linear over GF(2), so k steps are the 64 x 64 bit matrix M^k; col[i][b] = M^(2^i) e_b.  A row-slab
 * handle uses it to skip the cells of other ranks' rows while it walks the ONE seeding stream (below). */
#define RNG_JUMPS 48
static uint64_t g_jump[RNG_JUMPS][64];
static pthread_once_t g_jump_once = PTHREAD_ONCE_INIT;   /* handles may load scenarios from several threads at once */
static uint64_t jump_apply(const uint64_t* col, uint64_t x) {
  uint64_t y = 0;
  while (x) { y ^= col[__builtin_ctzll(x)]; x &= x - 1; }
  return y;
}
static void jump_fill(void) {
  for (int b = 0; b < 64; ++b) { uint64_t x = 1ull << b; x ^= x >> 12; x ^= x << 25; x ^= x >> 27; g_jump[0][b] = x; }
  for (int i = 1; i < RNG_JUMPS; ++i)
    for (int b = 0; b < 64; ++b) g_jump[i][b] = jump_apply(g_jump[i - 1], g_jump[i - 1][b]);
}
static void jump_init(void) { pthread_once(&g_jump_once, jump_fill); }
uint64_t euler_rng_jump(uint64_t state, uint64_t steps) {
  jump_init();
  for (int i = 0; steps && i < RNG_JUMPS; ++i, steps >>= 1)
    if (steps & 1) state = jump_apply(g_jump[i], state);
  return state;
}

/* ---- scenario text ---------------------------------------------------------------------- */

static void classify(char c, size_t i, uint8_t* solid, uint8_t* source, uint8_t* sink, uint8_t* fluid) {
  switch (c) { /* main.c:226-235; anything else is empty */
    case 'X': solid[i] = 1; break;
    case '0': fluid[i] = 1; break;
    case '?': fluid[i] = 1; source[i] = 1; break;
    case '=': sink[i] = 1; break;
    default: break;
  }
}

int euler_parse_scenario(const char* text, int32_t len, int32_t X, int32_t Y, int32_t upscale,
                         uint8_t* solid, uint8_t* source, uint8_t* sink, uint8_t* fluid) {
  if (!text || len < 0 || X < 4 || Y < 4 || !solid || !source || !sink || !fluid) return EULER_EINVAL;
  const size_t C = (size_t)X * (size_t)Y;
  memset(solid, 0, C); memset(source, 0, C); memset(sink, 0, C); memset(fluid, 0, C);

  if (!upscale) {
    /* The reference consumes the text as a stream (main.c:218-241): the first line fills row
     * Y-2, each line fills x = 1..X-2; a line that reaches the width limit has its remainder
     * (including its newline) discarded. */
    int32_t pos = 0;
    for (int32_t y = Y - 2; y > 0 && pos < len; --y) {
      int32_t x = 1;
      while (x < X - 1 && pos < len) {
        char c = text[pos++];
        if (c == '\n') break;
        classify(c, (size_t)y * X + x, solid, source, sink, fluid);
        ++x;
      }
      if (x == X - 1)
        while (pos < len && text[pos++] != '\n') {}
    }
  } else {
    /* Build extension: nearest-neighbour resample of a Wf x Hf picture onto the interior.
     * ch(x,y) = line[(Y-2-y)*Hf/(Y-2)][(x-1)*Wf/(X-2)], missing characters are blanks. */
    int32_t Hf = 0, Wf = 0;
    for (int32_t i = 0, w = 0; i <= len; ++i) {
      if (i == len || text[i] == '\n') {
        if (i < len || w > 0) { ++Hf; if (w > Wf) Wf = w; }
        w = 0;
      } else ++w;
    }
    if (Hf == 0 || Wf == 0) return EULER_EINVAL;
    int32_t* start = (int32_t*)malloc(sizeof(int32_t) * (size_t)Hf * 2);
    if (!start) return EULER_ENOMEM;
    int32_t* length = start + Hf;
    int32_t k = 0, s0 = 0;
    for (int32_t i = 0; i <= len; ++i)
      if (i == len || text[i] == '\n') {
        if (i < len || i > s0) { start[k] = s0; length[k] = i - s0; ++k; }
        s0 = i + 1;
      }
    for (int32_t y = 1; y <= Y - 2; ++y) {
      int64_t fr = ((int64_t)(Y - 2 - y) * Hf) / (Y - 2);
      for (int32_t x = 1; x <= X - 2; ++x) {
        int64_t fc = ((int64_t)(x - 1) * Wf) / (X - 2);
        char c = fc < length[fr] ? text[start[fr] + fc] : ' ';
        classify(c, (size_t)y * X + x, solid, source, sink, fluid);
      }
    }
    free(start);
  }
  /* sink ring around the domain (main.c:244-252) */
  for (int32_t y = 0; y < Y; ++y) { sink[(size_t)y * X] = 1; sink[(size_t)y * X + X - 1] = 1; }
  for (int32_t x = 0; x < X; ++x) { sink[x] = 1; sink[(size_t)(Y - 1) * X + x] = 1; }
  return EULER_OK;
}

/* `tanks` closed tanks on top of each other (1 = SURVEY 8d config 3): tank k takes the rows [k H, (k+1) H), H = Y / tanks,
 * a solid ring one cell inside its border, fluid in its lower half; the rows where two tanks meet are solid as well, so that
 * every tank is the single tank of an X x H grid (the weak-scaling workload: one tank per row slab). */
int euler_half_tanks_grids(int32_t X, int32_t Y, int32_t tanks, uint8_t* solid, uint8_t* source, uint8_t* sink, uint8_t* fluid) {
  if (tanks < 1 || Y % tanks) return EULER_EINVAL;
  const int32_t H = Y / tanks;
  if (X < 6 || H < 6) return EULER_EINVAL;
  const size_t C = (size_t)X * (size_t)Y;
  memset(solid, 0, C); memset(source, 0, C); memset(sink, 0, C); memset(fluid, 0, C);
  for (int32_t y = 1; y <= Y - 2; ++y) {
    const int32_t ly = y % H;
    for (int32_t x = 1; x <= X - 2; ++x) {
      size_t i = (size_t)y * X + x;
      if (ly == 0 || ly == H - 1 || ly == 1 || ly == H - 2 || x == 1 || x == X - 2) solid[i] = 1;
      else if (ly < H / 2) fluid[i] = 1;
    }
  }
  for (int32_t y = 0; y < Y; ++y) { sink[(size_t)y * X] = 1; sink[(size_t)y * X + X - 1] = 1; }
  for (int32_t x = 0; x < X; ++x) { sink[x] = 1; sink[(size_t)(Y - 1) * X + x] = 1; }
  return EULER_OK;
}
int euler_half_tank_grids(int32_t X, int32_t Y, uint8_t* solid, uint8_t* source, uint8_t* sink, uint8_t* fluid) {
  return euler_half_tanks_grids(X, Y, 1, solid, source, sink, fluid);
}

/* Four jittered markers per fluid cell (main.c:255-266): columns outer, rows inner, quadrant
 * k = 0..3, the x jitter drawn before the y jitter, all arithmetic in float. */
int euler_seed_markers(const uint8_t* fluid, int32_t X, int32_t Y, uint64_t* rng_state,
                       float* markers_xy, uint64_t* n_markers) {
  if (!fluid || !rng_state || !markers_xy || !n_markers) return EULER_EINVAL;
  uint64_t n = 0;
  for (int32_t cx = 0; cx < X; ++cx)
    for (int32_t cy = 0; cy < Y; ++cy) {
      if (!fluid[(size_t)cy * X + cx]) continue;
      for (int k = 0; k < 4; ++k) {
        float jx = euler_rng_next_float(rng_state) / 2;
        float mx = cx + (k < 2 ? 0 : 0.5f) + jx;
        float jy = euler_rng_next_float(rng_state) / 2;
        float my = cy + (k % 2 ? 0 : 0.5f) + jy;
        markers_xy[2 * n] = 1.f * mx;     /* k_side_length = 1 (main.c:58,262) */
        markers_xy[2 * n + 1] = 1.f * my;
        ++n;
      }
    }
  *n_markers = n;
  return EULER_OK;
}

/* The same stream, keeping only the markers whose row floor(y) lies in [row_lo, row_hi) together with their index in the whole
 * array (a row-slab handle: every rank walks the one sequential RNG stream, none stores the whole array).  Two passes by the
 * caller: markers_xy == NULL counts (n_total, n_kept), the second call fills (the RNG state is only advanced by the caller's
 * copy).  cap = room in markers_xy / keys. */
int euler_seed_markers_rows(const uint8_t* fluid, int32_t X, int32_t Y, int32_t row_lo, int32_t row_hi, uint64_t* rng_state,
                            float* markers_xy, uint32_t* keys, uint64_t cap, uint64_t* n_total, uint64_t* n_kept) {
  if (!fluid || !rng_state || !n_total || !n_kept) return EULER_EINVAL;
  /* A cell's markers land in its own row or (a jitter of exactly 0.5) the next one: only the cells of rows [lo2, row_hi) can give
   * this rank a marker.  The cells below and above them in a column are skipped - 4 keys and 8 draws each - with a jump. */
  const int32_t lo2 = row_lo > 0 ? row_lo - 1 : 0, hi2 = row_hi < Y ? row_hi : Y;
  uint32_t* below = (uint32_t*)calloc((size_t)X, sizeof(uint32_t));
  uint32_t* above = (uint32_t*)calloc((size_t)X, sizeof(uint32_t));
  if (!below || !above) { free(below); free(above); return EULER_ENOMEM; }
  for (int32_t cy = 0; cy < lo2; ++cy)
    for (int32_t cx = 0; cx < X; ++cx) below[cx] += fluid[(size_t)cy * X + cx] != 0;
  for (int32_t cy = hi2; cy < Y; ++cy)
    for (int32_t cx = 0; cx < X; ++cx) above[cx] += fluid[(size_t)cy * X + cx] != 0;
  uint64_t n = 0, kept = 0;
  int rc = EULER_OK;
  for (int32_t cx = 0; cx < X && rc == EULER_OK; ++cx) {
    n += 4ull * below[cx];
    *rng_state = euler_rng_jump(*rng_state, 8ull * below[cx]);
    for (int32_t cy = lo2; cy < hi2; ++cy) {
      if (!fluid[(size_t)cy * X + cx]) continue;
      for (int k = 0; k < 4; ++k) {
        float jx = euler_rng_next_float(rng_state) / 2;
        float mx = cx + (k < 2 ? 0 : 0.5f) + jx;
        float jy = euler_rng_next_float(rng_state) / 2;
        float my = cy + (k % 2 ? 0 : 0.5f) + jy;
        const int32_t row = (int32_t)floorf(1.f * my);
        if (row >= row_lo && row < row_hi) {
          if (markers_xy) {
            if (kept >= cap) { rc = EULER_ENOMEM; break; }
            markers_xy[2 * kept] = 1.f * mx; markers_xy[2 * kept + 1] = 1.f * my; keys[kept] = (uint32_t)n;
          }
          ++kept;
        }
        ++n;
      }
      if (rc != EULER_OK) break;
    }
    n += 4ull * above[cx];
    *rng_state = euler_rng_jump(*rng_state, 8ull * above[cx]);
  }
  free(below); free(above);
  if (rc != EULER_OK) return rc;
  *n_total = n; *n_kept = kept;
  return EULER_OK;
}

/* ---- frame formatter (draw_rows, main.c:914-951; escape codes misc/terminal.h:36,53,60) ---- */

static int render_rows(const uint8_t* solid, const uint8_t* sink, const uint8_t* count,
                       const float* cr, const float* cg, const float* cb,
                       int32_t X, int32_t Y, int32_t wx, int32_t wy, char* out, int32_t cap, int32_t* len) {
  if (!solid || !sink || !count || !len) return EULER_EINVAL;
  static const char glyph[4] = {' ', 'o', 'O', '0'};
  static const char blue[] = "\x1B[34m", reset[] = "\x1B[0m", clear_line[] = "\x1b[K", crlf[] = "\r\n";
  const int dye = cr && cg && cb;
  int64_t n = 0;
#define EMIT(s, k) do { for (int _i = 0; _i < (int)(k); ++_i) { if (out && n < cap) out[n] = (s)[_i]; ++n; } } while (0)
  int32_t cutoff = Y - 1 - wy;
  if (cutoff < 1) cutoff = 1;
  /* the reference's `for (y = Y-1; y-- > cutoff;)` visits y = Y-2 ... cutoff inclusive */
  for (int32_t y = Y - 2; y >= cutoff; --y) {
    int water_run = 0;
    for (int32_t x = 1; x < X - 1 && x < wx + 1; ++x) {
      size_t i = (size_t)y * X + x;
      if (solid[i]) {
        if (water_run) EMIT(reset, 4);
        EMIT("X", 1);
        water_run = 0;
      } else if (sink[i]) {
        if (water_run) EMIT(reset, 4);
        EMIT("=", 1);           /* the run flag is deliberately left as is (main.c:927-931) */
      } else {
        int k = count[i] < 3 ? count[i] : 3;
        if (!water_run && k && !dye) EMIT(blue, 5);
        else if (k && dye) {    /* buffer_append_color (main.c:902-912): sRGB ~ x^(1/2.2), byte = (int)clamp(0, end*x, end) */
          char esc[32];
          const float end = nextafterf(256.f, 0.f);
          const float lin[3] = {cr[i], cg[i], cb[i]};
          int byte[3];
          for (int c = 0; c < 3; ++c) {
            float v = end * powf(lin[c], 1 / 2.2f);
            byte[c] = (int)(v < 0.f ? 0.f : (v > end ? end : v));
          }
          int m = snprintf(esc, sizeof esc, "\x1B[38;2;%d;%d;%dm", byte[0], byte[1], byte[2]);
          EMIT(esc, m);
        } else if (water_run && !k) EMIT(reset, 4);
        EMIT(&glyph[k], 1);
        water_run = k != 0;
      }
    }
    EMIT(reset, 4);
    EMIT(clear_line, 3);
    if (y > cutoff) EMIT(crlf, 2);
  }
#undef EMIT
  *len = (int32_t)n;
  return EULER_OK;
}

int euler_render_grids(const uint8_t* solid, const uint8_t* sink, const uint8_t* count,
                       int32_t X, int32_t Y, int32_t wx, int32_t wy, char* out, int32_t cap, int32_t* len) {
  return render_rows(solid, sink, count, NULL, NULL, NULL, X, Y, wx, wy, out, cap, len);
}

int euler_render_grids_rgb(const uint8_t* solid, const uint8_t* sink, const uint8_t* count,
                           const float* r, const float* g, const float* b,
                           int32_t X, int32_t Y, int32_t wx, int32_t wy, char* out, int32_t cap, int32_t* len) {
  if (!r || !g || !b) return EULER_EINVAL;
  return render_rows(solid, sink, count, r, g, b, X, Y, wx, wy, out, cap, len);
}

/* ---- whole-domain overview: host formatters over euler_overview_px records (include/euler.h, docs/overview.md) ---- */

enum { OV_AIR = 0, OV_SOLID = 4, OV_SINK = 5 };   /* 1..3: the glyph index of draw_rows */

static int overview_class(const euler_overview_px* p) {
  if (2ull * p->solid >= p->cells) return OV_SOLID;
  const uint64_t open = (uint64_t)p->cells - p->solid - p->sink;
  if (p->sink > 0 && p->sink >= open) return OV_SINK;
  const uint64_t k = ((uint64_t)p->marks + open - 1) / open;     /* open >= 1 here: solid < cells / 2 and sink < open */
  return k < 3 ? (int)k : 3;
}

/* buffer_append_color's byte (main.c:902-912) as render_rows forms it */
static int overview_srgb_byte(float lin) {
  const float end = nextafterf(256.f, 0.f);
  float v = end * powf(lin, 1 / 2.2f);
  return (int)(v < 0.f ? 0.f : (v > end ? end : v));
}

static float overview_mean_dye(const euler_overview_px* p, int c) {
  return p->water ? (float)((double)p->dye[c] / ((double)p->water * 16777216.0)) : 0.f;
}

int euler_overview_text(const euler_overview_px* px, int32_t W, int32_t H, int32_t rainbow,
                        char* out, int32_t cap, int32_t* len) {
  if (!px || !len || W < 1 || H < 1) return EULER_EINVAL;
  /* a (W + 2) x (H + 2) grid of the classes with a border ring that is never drawn: render_rows does the rest */
  const int32_t X = W + 2, Y = H + 2;
  const size_t C = (size_t)X * (size_t)Y;
  uint8_t* g = (uint8_t*)calloc(3, C);
  float* col = rainbow ? (float*)calloc(3 * C, sizeof(float)) : NULL;
  if (!g || (rainbow && !col)) { free(g); free(col); return EULER_ENOMEM; }
  for (int32_t py = 0; py < H; ++py)
    for (int32_t p = 0; p < W; ++p) {
      const euler_overview_px* r = px + (size_t)py * W + p;
      const size_t i = (size_t)(H - py) * X + (size_t)(p + 1);      /* pixel row 0 is the top: grid row Y - 2 */
      const int k = overview_class(r);
      if (k == OV_SOLID) g[i] = 1;
      else if (k == OV_SINK) g[C + i] = 1;
      else g[2 * C + i] = (uint8_t)k;
      if (col) for (int c = 0; c < 3; ++c) col[c * C + i] = overview_mean_dye(r, c);
    }
  int rc = render_rows(g, g + C, g + 2 * C, col, col ? col + C : NULL, col ? col + 2 * C : NULL, X, Y, W, H, out, cap, len);
  free(g);
  free(col);
  return rc;
}

/* ---- pan-and-zoom viewport: the magnified frame (include/euler.h, docs/viewport.md) ---- */

int euler_view_text(const euler_overview_px* cells, const uint32_t* raster, int32_t Bw, int32_t Bh,
                    int32_t scale, int32_t rainbow, char* out, int32_t cap, int32_t* len) {
  if (!cells || !raster || !len || Bw < 1 || Bh < 1) return EULER_EINVAL;
  if (scale != 1 && scale != 2 && scale != 4 && scale != 8 && scale != 16) return EULER_EINVAL;
  if ((int64_t)Bw * scale * ((int64_t)Bh * scale) > (1 << 24)) return EULER_EINVAL;
  /* as euler_overview_text: a (W + 2) x (H + 2) grid with a border ring that is never drawn, scale x scale sub-pixels per cell */
  const int32_t W = Bw * scale, H = Bh * scale, X = W + 2, Y = H + 2;
  const size_t C = (size_t)X * (size_t)Y;
  uint8_t* g = (uint8_t*)calloc(3, C);
  float* col = rainbow ? (float*)calloc(3 * C, sizeof(float)) : NULL;
  if (!g || (rainbow && !col)) { free(g); free(col); return EULER_ENOMEM; }
  for (int32_t cy = 0; cy < Bh; ++cy)
    for (int32_t cx = 0; cx < Bw; ++cx) {
      const euler_overview_px* r = cells + (size_t)cy * Bw + cx;
      const int k = overview_class(r);
      float dye[3] = {0.f, 0.f, 0.f};
      if (col) for (int c = 0; c < 3; ++c) dye[c] = overview_mean_dye(r, c);
      for (int32_t sy = 0; sy < scale; ++sy)
        for (int32_t sx = 0; sx < scale; ++sx) {
          const int32_t py = cy * scale + sy, p = cx * scale + sx;
          const size_t i = (size_t)(H - py) * X + (size_t)(p + 1);      /* raster row 0 is the top: grid row Y - 2 */
          if (k == OV_SOLID) g[i] = 1;
          else if (k == OV_SINK) g[C + i] = 1;
          else { const uint32_t n = raster[(size_t)py * W + p]; g[2 * C + i] = (uint8_t)(n < 3 ? n : 3); }
          if (col) for (int c = 0; c < 3; ++c) col[c * C + i] = dye[c];
        }
    }
  int rc = render_rows(g, g + C, g + 2 * C, col, col ? col + C : NULL, col ? col + 2 * C : NULL, X, Y, W, H, out, cap, len);
  free(g);
  free(col);
  return rc;
}

int euler_overview_rgb(const euler_overview_px* px, int32_t W, int32_t H, int32_t mode, float speed_scale,
                       uint8_t* rgb, size_t rgb_bytes) {
  if (!px || !rgb || W < 1 || H < 1 || rgb_bytes != (size_t)W * (size_t)H * 3) return EULER_EINVAL;
  if (mode != EULER_IMAGE_COVERAGE && mode != EULER_IMAGE_DYE && mode != EULER_IMAGE_SPEED) return EULER_EINVAL;
  if (mode == EULER_IMAGE_SPEED && !(speed_scale > 0.f)) return EULER_EINVAL;      /* (a NaN fails the comparison too) */
  const size_t n = (size_t)W * (size_t)H;
  for (size_t i = 0; i < n; ++i) {
    const euler_overview_px* r = px + i;
    int wc[3] = {64, 128, 255};
    if (mode == EULER_IMAGE_DYE) {
      for (int c = 0; c < 3; ++c) wc[c] = overview_srgb_byte(overview_mean_dye(r, c));
    } else if (mode == EULER_IMAGE_SPEED) {
      float t = sqrtf(r->max_speed2) / speed_scale;
      if (!(t < 1.f)) t = 1.f;
      wc[0] = (int)(255.f * t + 0.5f); wc[1] = 128; wc[2] = (int)(255.f * (1.f - t) + 0.5f);
    }
    for (int c = 0; c < 3; ++c) {
      const uint64_t cells = r->cells ? r->cells : 1;
      rgb[3 * i + c] = (uint8_t)(((uint64_t)r->solid * 128 + (uint64_t)r->sink * 64 + (uint64_t)r->water * (uint64_t)wc[c] + cells / 2) / cells);
    }
  }
  return EULER_OK;
}

/* ---- the envelopes' host side (include/euler.h, docs/envelope.md): the channel index, the words a restored plane may hold, the image ---- */

int eu_envelope_index(int32_t channel) {
  switch (channel) {
    case EULER_ENV_ARRIVAL: return 0;
    case EULER_ENV_WET: return 1;
    case EULER_ENV_SPEED: return 2;
    case EULER_ENV_PRESSURE: return 3;
    default: return -1;
  }
}

size_t eu_envelope_check_words(int32_t channel, const uint32_t* w, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    if (channel == EULER_ENV_ARRIVAL && w[i] == 0xffffffffu) continue;
    if (w[i] >= 0x7f800000u) return i;      /* an infinity, a NaN or a set sign bit (-0.f too) */
  }
  return (size_t)-1;
}

static float envelope_word(uint32_t w) {
  float f;
  memcpy(&f, &w, sizeof f);
  return f;
}

int euler_envelope_rgb(const euler_envelope_px* px, int32_t W, int32_t H, int32_t channel, double scale, uint8_t* rgb, size_t rgb_bytes) {
  if (!px || !rgb || W < 1 || H < 1 || eu_envelope_index(channel) < 0) return EULER_EINVAL;
  if (!isfinite(scale) || !(scale > 0.0)) return EULER_EINVAL;
  if (rgb_bytes != (size_t)W * (size_t)H * 3) return EULER_EINVAL;
  const size_t n = (size_t)W * (size_t)H;
  for (size_t i = 0; i < n; ++i) {
    const euler_envelope_px* r = px + i;
    const uint32_t word = channel == EULER_ENV_ARRIVAL ? r->arrival_min : (channel == EULER_ENV_WET ? r->wet_max : (channel == EULER_ENV_SPEED ? r->speed2_max : r->p_max));
    const int dark = channel == EULER_ENV_ARRIVAL ? r->touched == 0 : (r->touched == 0 && word == 0);
    if (dark) { rgb[3 * i] = rgb[3 * i + 1] = rgb[3 * i + 2] = 0; continue; }
    double value = (double)envelope_word(word);
    if (channel == EULER_ENV_SPEED) value = sqrt(value);
    double t = value / scale;
    t = t > 0.0 ? (t < 1.0 ? t : 1.0) : 0.0;      /* (a NaN: 0) */
    const uint8_t c = (uint8_t)(255.0 * (1.0 - t));
    rgb[3 * i] = 255; rgb[3 * i + 1] = c; rgb[3 * i + 2] = c;
  }
  return EULER_OK;
}

/* ---- flow diagnostics: what a user reads off an euler_diag record (include/euler.h, docs/diagnostics.md) ---- */

int euler_diag_derive(const euler_diag* rec, euler_diag_values* out) {
  if (!rec || !out) return EULER_EINVAL;
  memset(out, 0, sizeof *out);
  if (!rec->fluid) return EULER_OK;
  const double fluid = (double)rec->fluid, markers = (double)rec->markers;      /* (markers >= fluid > 0) */
  out->mean_abs_div = (double)rec->div_l1 / 16777216.0 / fluid;
  out->kinetic_energy = 0.5 * ((double)rec->ke_hi + (double)rec->ke_lo / 4294967296.0);
  out->com_x = (double)rec->mass_x / markers;
  out->com_y = (double)rec->mass_y / markers;
  out->markers_per_cell = markers / fluid;
  out->crowded_fraction = (double)rec->crowded / fluid;
  return EULER_OK;
}

/* ---- flow raster: a field of euler_flow_px records painted into the dye sums of overview records (include/euler.h, docs/flow_raster.md) ---- */

static uint32_t paint_q24(float x) {      /* q(x) of euler_overview_px */
  const float c = x > 0.f ? (x > 1.f ? 1.f : x) : 0.f;
  return (uint32_t)(c * 16777216.f);
}
static double paint_clamp(double t, double lo) { return t < lo ? lo : (t > 1.0 ? 1.0 : t); }

int euler_flow_paint(const euler_flow_px* flow, euler_overview_px* px, int32_t W, int32_t H, int32_t field, double scale) {
  if (!flow || !px || W < 1 || H < 1) return EULER_EINVAL;
  if (field != EULER_PAINT_VORTICITY && field != EULER_PAINT_PRESSURE && field != EULER_PAINT_SPEED) return EULER_EINVAL;
  if (!(scale > 0.0) || !isfinite(scale)) return EULER_EINVAL;
  const size_t n = (size_t)W * (size_t)H;
  for (size_t k = 0; k < n; ++k)      /* the two rasters are of one box, raster and state */
    if (flow[k].cells != px[k].cells || flow[k].water != px[k].water) return EULER_EINVAL;
  for (size_t k = 0; k < n; ++k) {
    const euler_flow_px* f = flow + k;
    const double water = (double)f->water;
    double lin[3];
    if (field == EULER_PAINT_VORTICITY) {
      const double m = f->nodes ? ((double)f->w_pos - (double)f->w_neg) / 1048576.0 / (double)f->nodes : 0.0;
      const double t = paint_clamp(m / scale, -1.0);
      if (t >= 0.0) { lin[0] = 1.0; lin[1] = 1.0 - t; lin[2] = 1.0 - t; }
      else { lin[0] = 1.0 + t; lin[1] = 1.0 + t; lin[2] = 1.0; }
    } else {
      double m = 0.0;
      if (f->water && field == EULER_PAINT_PRESSURE) m = (double)f->p_sum / 256.0 / water;
      else if (f->water) {
        const double mu = ((double)f->u_pos - (double)f->u_neg) / 1048576.0 / water, mv = ((double)f->v_pos - (double)f->v_neg) / 1048576.0 / water;
        m = sqrt(mu * mu + mv * mv);
      }
      const double t = paint_clamp(m / scale, 0.0);
      lin[0] = t; lin[1] = 0.5; lin[2] = 1.0 - t;
    }
    for (int c = 0; c < 3; ++c) px[k].dye[c] = (uint64_t)f->water * paint_q24((float)lin[c]);
  }
  return EULER_OK;
}

/* the temperature's painter: the vorticity field's white - red - blue mapping over the mean difference from ambient (include/euler.h, docs/heat.md) */
int euler_heat_paint(const euler_heat_px* heat, euler_overview_px* px, int32_t W, int32_t H, float ambient, double scale) {
  if (!heat || !px || W < 1 || H < 1) return EULER_EINVAL;
  if (!(scale > 0.0) || !isfinite(scale) || !isfinite(ambient)) return EULER_EINVAL;
  const size_t n = (size_t)W * (size_t)H;
  for (size_t k = 0; k < n; ++k)      /* the two rasters are of one box, raster and state */
    if (heat[k].cells != px[k].cells || heat[k].water != px[k].water) return EULER_EINVAL;
  for (size_t k = 0; k < n; ++k) {
    const euler_heat_px* f = heat + k;
    const double m = f->water ? ((double)f->t_pos - (double)f->t_neg) / 1048576.0 / (double)f->water : 0.0;
    const double t = paint_clamp(m / scale, -1.0);
    double lin[3];
    if (t >= 0.0) { lin[0] = 1.0; lin[1] = 1.0 - t; lin[2] = 1.0 - t; }
    else { lin[0] = 1.0 + t; lin[1] = 1.0 + t; lin[2] = 1.0; }
    for (int c = 0; c < 3; ++c) px[k].dye[c] = (uint64_t)f->water * paint_q24((float)lin[c]);
  }
  return EULER_OK;
}

/* ---- batched gauges: the list checked, cut into chunks, and the values read off a record (include/euler.h, docs/gauges.md) ---- */

int eu_interior_box_ok(int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t X, int32_t Y) { return !(x0 < 1 || y0 < 1 || x1 > X - 2 || y1 > Y - 2 || x0 > x1 || y0 > y1); }

int eu_gauge_check(const euler_gauge* g, int32_t n, int32_t X, int32_t Y, const char** what) {
  for (int32_t k = 0; k < n; ++k) {
    const char* w = NULL;
    if (g[k].kind < EULER_GAUGE_LEVEL || g[k].kind > EULER_GAUGE_FLUX) w = "an unknown kind";
    else if (g[k].reserved != 0) w = "reserved is not 0";
    else if (!eu_interior_box_ok(g[k].x0, g[k].y0, g[k].x1, g[k].y1, X, Y)) w = "its box is not inside the interior";
    if (w) { if (what) *what = w; return k; }
  }
  return -1;
}

size_t eu_gauge_chunks(const euler_gauge* g, int32_t n, eu_gauge_chunk* out) { return eu_gauge_chunks_bands(g, n, 0, INT32_MAX, out); }

size_t eu_gauge_chunks_bands(const euler_gauge* g, int32_t n, int32_t band_lo, int32_t band_hi, eu_gauge_chunk* out) {
  size_t m = 0;
  for (int32_t k = 0; k < n; ++k) {
    const int32_t tx0 = g[k].x0 >> 6, tx1 = g[k].x1 >> 6, by0 = g[k].y0 >> 6, by1 = g[k].y1 >> 6;
    const int32_t ty0 = by0 > band_lo ? by0 : band_lo, ty1 = by1 < band_hi - 1 ? by1 : band_hi - 1;      /* the tile rows of the box inside the bands */
    if (ty0 > ty1) continue;
    if (!out) { m += (size_t)(tx1 - tx0 + 1) * (size_t)(ty1 - ty0 + 1); continue; }
    for (int32_t ty = ty0; ty <= ty1; ++ty)
      for (int32_t tx = tx0; tx <= tx1; ++tx) {      /* the tile clipped to the box */
        eu_gauge_chunk* c = out + m++;
        c->gauge = k; c->kind = g[k].kind;
        c->x0 = tx == tx0 ? g[k].x0 : tx << 6; c->x1 = tx == tx1 ? g[k].x1 : (tx << 6) + 63;
        c->y0 = ty == by0 ? g[k].y0 : ty << 6; c->y1 = ty == by1 ? g[k].y1 : (ty << 6) + 63;
      }
  }
  return m;
}

/* ---- the observer passes on row slabs: what every rank works out alike from the band ranges (euler_host.h, docs/observer_passes.md "On row slabs") ---- */

int eu_slab_clip_rows(int32_t band_lo, int32_t band_hi, int32_t Y, int32_t y0, int32_t y1, int32_t* ya, int32_t* yb) {
  const int64_t lo = (int64_t)band_lo * 64, hi = (int64_t)band_hi * 64 < Y ? (int64_t)band_hi * 64 : Y;      /* the rank's rows [lo, hi) */
  *ya = (int32_t)(y0 > lo ? y0 : lo);
  *yb = (int32_t)(y1 < hi - 1 ? y1 : hi - 1);
  if (*ya <= *yb) return 1;
  *ya = 0; *yb = -1;
  return 0;
}

static void slab_plan_offsets(eu_slab_plan* P) {
  int64_t at = 0;
  for (int32_t r = 0; r < P->nranks; ++r) {
    P->cnt[r] = P->p_lo[r] <= P->p_hi[r] ? (int64_t)(P->p_hi[r] - P->p_lo[r] + 1) * P->W : 0;
    P->off[r] = at;
    at += P->cnt[r];
  }
  P->total = at;
}

int eu_slab_plan_raster(eu_slab_plan* P, int32_t nranks, const int32_t* band_lo, const int32_t* band_hi, int32_t Y, int32_t y0, int32_t y1, int32_t W, int32_t H) {
  if (!P || !band_lo || !band_hi || nranks < 1 || nranks > EU_SLAB_PLAN_MAXR || Y < 1 || y0 < 0 || y1 >= Y || y0 > y1 || W < 1 || H < 1 || H > y1 - y0 + 1) return EULER_EINVAL;
  for (int32_t r = 0; r < nranks; ++r)
    if (band_lo[r] < 0 || band_hi[r] < band_lo[r] || band_hi[r] > (Y + 63) / 64 || (r > 0 && band_lo[r] < band_hi[r - 1])) return EULER_EINVAL;
  memset(P, 0, sizeof *P);
  P->nranks = nranks; P->W = W; P->H = H; P->y0 = y0; P->y1 = y1;
  const int64_t Bh = (int64_t)y1 - y0 + 1;
  for (int32_t r = 0; r < nranks; ++r) {
    P->p_lo[r] = 0; P->p_hi[r] = -1;
    if (!eu_slab_clip_rows(band_lo[r], band_hi[r], Y, y0, y1, &P->ya[r], &P->yb[r])) continue;
    P->p_lo[r] = (int32_t)((((int64_t)y1 - P->yb[r] + 1) * H - 1) / Bh);      /* the pixel row of the rank's top row ... */
    P->p_hi[r] = (int32_t)((((int64_t)y1 - P->ya[r] + 1) * H - 1) / Bh);      /* ... and of its bottom row */
  }
  slab_plan_offsets(P);
  return EULER_OK;
}

int eu_slab_plan_flat(eu_slab_plan* P, int32_t nranks, int32_t n) {
  if (!P || nranks < 1 || nranks > EU_SLAB_PLAN_MAXR || n < 1) return EULER_EINVAL;
  memset(P, 0, sizeof *P);
  P->nranks = nranks; P->W = n; P->H = 1;
  for (int32_t r = 0; r < nranks; ++r) { P->ya[r] = 0; P->yb[r] = -1; P->p_lo[r] = P->p_hi[r] = 0; }
  slab_plan_offsets(P);
  return EULER_OK;
}

void eu_slab_plan_bytes(const eu_slab_plan* P, int64_t rec_bytes, int64_t* off, int64_t* cnt) {
  for (int32_t r = 0; r < P->nranks; ++r) { off[r] = P->off[r] * rec_bytes; cnt[r] = P->cnt[r] * rec_bytes; }
}

int eu_slab_plan_contributors(const eu_slab_plan* P, int32_t py, int32_t* first, int32_t* last) {
  if (!P || !first || !last || py < 0 || py >= P->H) return EULER_EINVAL;
  eu_slab_row_ranks(P, py, first, last);
  return EULER_OK;
}

/* ---- the multilevel preconditioner: its node grids and the plan of the cycle split by rows (euler_host.h, docs/solver_multilevel_row_slabs.md) ---- */

int eu_mg_levels(int32_t X, int32_t nbands, int32_t* nx, int32_t* ny, size_t* off) {
  if (!nx || !ny || !off || X < 1 || nbands < 1 || nbands > INT32_MAX / MG_RPB) return EULER_EINVAL;
  int32_t w = (X - 1) / MG_G0 + 1, h = MG_RPB * nbands;
  size_t at = 0;
  for (int l = 0; l < MG_MAXLEV; ++l) {
    nx[l] = w; ny[l] = h; off[l] = at; at += (size_t)w * (size_t)h;
    if ((int64_t)w * h <= MG_TOP_MAX) return l + 1;
    w = (w + 1) / 2; h = (h + 1) / 2;
  }
  return EULER_EINVAL;
}

static int64_t mg_nodes(const int32_t* nx, const int32_t* ny, int l) { return (int64_t)nx[l] * ny[l]; }

int eu_mg_entry_level(int32_t levels, const int32_t* nx, const int32_t* ny) {
  int l = 0;
  while (l < levels - 1 && mg_nodes(nx, ny, l) > MG_TAIL_MAX) ++l;
  return l;
}

int eu_mg_gather_level(int32_t levels, const int32_t* nx, const int32_t* ny, int64_t forced) {
  const int lC = eu_mg_entry_level(levels, nx, ny);
  if (forced < 0) return 0;
  if (forced > 0) return (int)(forced < lC ? forced : lC);
  if (mg_nodes(nx, ny, 0) <= MG_SMALL_LEVEL0) return 0;
  int l = 0;
  while (l < lC && mg_nodes(nx, ny, l) > MG_GATHER_MAX) ++l;
  return l;
}

static void mg_clip(int32_t* r, int32_t n) { if (r[0] < 0) r[0] = 0; if (r[1] > n) r[1] = n; if (r[1] < r[0]) r[1] = r[0]; }
/* the rows two ranges share: out = them and their number, or {0, 0} and 0 */
static int32_t mg_meet(const int32_t* a, const int32_t* b, int32_t* out) {
  const int32_t lo = a[0] > b[0] ? a[0] : b[0], hi = a[1] < b[1] ? a[1] : b[1];
  out[0] = hi > lo ? lo : 0; out[1] = hi > lo ? hi : 0;
  return out[1] - out[0];
}
/* what the way up of the rank with the bands [lo, hi) needs on the levels below Lg: x_l on NX, computed from the true right-hand side on NR = NX grown by a row;
 * the next level's NX = the coarse rows around NR (mg_coarse_around, k_mg_cycle.hip) */
static void mg_need(const int32_t* ny, int Lg, int32_t lo, int32_t hi, int32_t (*NX)[2], int32_t (*NR)[2]) {
  int32_t x0 = MG_RPB * lo - 1, x1 = MG_RPB * hi + 1;
  for (int l = 0; l < Lg; ++l) {
    NX[l][0] = x0; NX[l][1] = x1; mg_clip(NX[l], ny[l]);
    NR[l][0] = NX[l][0] - 1; NR[l][1] = NX[l][1] + 1; mg_clip(NR[l], ny[l]);
    x0 = NR[l][0] >> 1; x1 = ((NR[l][1] - 1) >> 1) + 2;
  }
}

int eu_mg_split_plan_fill(eu_mg_split_plan* P, int32_t levels, const int32_t* nx, const int32_t* ny, int32_t Lg, int32_t nranks, int32_t rank,
                          const int32_t* part_lo, const int32_t* part_hi, int32_t seg_cap) {
  if (!P || !nx || !ny || !part_lo || !part_hi || levels < 2 || levels > MG_MAXLEV || Lg < 1 || Lg > levels - 1 || nranks < 2 || nranks > MG_SPLIT_MAXR ||
      rank < 0 || rank >= nranks || seg_cap < 0 || seg_cap > 4 * MG_MAXLEV) return EULER_EINVAL;
  for (int l = 0; l <= Lg; ++l) if (nx[l] < 1 || ny[l] < 1) return EULER_EINVAL;
  if (mg_nodes(nx, ny, 0) > INT32_MAX / 18) return EULER_EINVAL;      /* every count below is at most 18 x level 0's nodes */
  for (int r = 0; r < nranks; ++r)
    if (part_lo[r] < 0 || part_hi[r] <= part_lo[r] || part_hi[r] > ny[0] / MG_RPB || (r > 0 && part_lo[r] < part_hi[r - 1])) return EULER_EINVAL;
  memset(P, 0, sizeof *P);
  const int me = rank, R = nranks;
  P->Lg = Lg; P->ranks = R; P->rank = me;
  for (int r = 0; r < R; ++r) {
    /* supports: a fine row f feeds the coarse rows i with |f - 2 i| <= 1, and the residual reaches one row beyond the support: ceil((a - 2) / 2) ... floor((b + 1) / 2) */
    int32_t a = MG_RPB * part_lo[r] - 1, b = MG_RPB * part_hi[r] + 1;
    for (int l = 0; l <= Lg; ++l) {
      P->I[l][r][0] = a; P->I[l][r][1] = b; mg_clip(P->I[l][r], ny[l]);
      a = P->I[l][r][0] - 2 >= 0 ? (P->I[l][r][0] - 1) / 2 : 0; b = (P->I[l][r][1] + 1) / 2 + 1;
    }
    /* owners */
    a = MG_RPB * part_lo[r]; b = MG_RPB * part_hi[r];
    for (int l = 0; l <= Lg; ++l) {
      P->O[l][r][0] = a; P->O[l][r][1] = b;
      if (l < Lg && b - a < MG_SETUP_HALO) P->setup_bad = 1;
      a = (a + 1) / 2; b = (b + 1) / 2;
    }
    const int32_t own = P->O[Lg][r][1] - P->O[Lg][r][0], win = P->I[Lg][r][1] - P->I[Lg][r][0];
    if (9 * own * nx[Lg] > P->aslot) P->aslot = 9 * own * nx[Lg];
    if (win > P->win_rows) P->win_rows = win;
  }
  P->nsmall = 2 + P->win_rows * nx[Lg];
  mg_need(ny, Lg, part_lo[me], part_hi[me], P->NX, P->NR);
  /* zones: what the neighbour on either side needs of my share, what I need of its share; its need is computed as mine is */
  for (int side = 0; side < 2; ++side) {
    const int nb = side == 0 ? me - 1 : me + 1;
    if (nb < 0 || nb >= R) continue;
    int32_t nbX[MG_MAXLEV][2], nbR[MG_MAXLEV][2], offs = 0, offr = 0;
    mg_need(ny, Lg, part_lo[nb], part_hi[nb], nbX, nbR);
    for (int l = 0; l < Lg; ++l) {
      P->zoff_s[side][l] = offs; P->zoff_r[side][l] = offr;
      offs += mg_meet(P->I[l][me], nbR[l], P->zs[side][l]) * nx[l];
      offr += mg_meet(P->I[l][nb], P->NR[l], P->zr[side][l]) * nx[l];
    }
    if (offs > P->zone) P->zone = offs;
    if (offr > P->zone) P->zone = offr;
  }
  /* a zone may reach into the next rank only: no rank beyond may contribute to what I need (the supports ascend with the rank: the nearest such rank decides) */
  for (int far = me - 2; far <= me + 2; far += 4)
    for (int l = 0; l < Lg && far >= 0 && far < R; ++l) { int32_t t[2]; if (mg_meet(P->I[l][far], P->NR[l], t)) P->beyond = 1; }
  /* the setup by owners: what this rank reads of a level must lie within its owned rows + halo */
  for (int l = 0; l < Lg; ++l) {
    int32_t lo = P->I[l][me][0] - 1, hi = P->I[l][me][1] + 1;                                     /* the way down: the residual one row beyond the share's support */
    lo = P->NR[l][0] < lo ? P->NR[l][0] : lo; hi = P->NR[l][1] > hi ? P->NR[l][1] : hi;           /* the way up */
    const int32_t c0 = 2 * P->O[l + 1][me][0] - 1, c1 = 2 * P->O[l + 1][me][1];                   /* the next level's owned rows are formed from these */
    int32_t rd[2] = {c0 < lo ? c0 : lo, c1 > hi ? c1 : hi};
    if (rd[0] < 0) rd[0] = 0;
    if (rd[1] > ny[l]) rd[1] = ny[l];
    if (rd[0] < P->O[l][me][0] - MG_SETUP_HALO || rd[1] > P->O[l][me][1] + MG_SETUP_HALO) P->setup_bad = 1;
  }
  /* the segment table */
  for (int l = 0; l < Lg; ++l) {
    int32_t run0 = -1;
    for (int32_t row = P->NR[l][0]; row <= P->NR[l][1]; ++row) {
      const int touched = row < P->NR[l][1] && (!(row >= P->I[l][me][0] && row < P->I[l][me][1]) || (row >= P->zr[0][l][0] && row < P->zr[0][l][1]) ||
                                                (row >= P->zr[1][l][0] && row < P->zr[1][l][1]));
      if (touched && run0 < 0) run0 = row;
      if (!touched && run0 >= 0) {
        if (P->nseg >= seg_cap) P->overflow = 1;
        else {
          const eu_mg_seg s = {l, run0, row, P->total};
          P->seg[P->nseg++] = s;
          P->total += (row - run0) * nx[l];
        }
        run0 = -1;
      }
    }
  }
  return EULER_OK;
}

/* ---- forcing: the record's defaults and its uniform part, the list checked and cut into the tile table (include/euler.h, docs/forcing.md) ---- */

int euler_forcing_default(euler_forcing* f) {
  if (!f) return EULER_EINVAL;
  memset(f, 0, sizeof *f);
  f->gy = -10.f;      /* k_gravity (main.c:60) */
  return EULER_OK;
}

int euler_forcing_at(const euler_forcing* f, double t, float a[2]) {
  if (!f || !a) return EULER_EINVAL;
  const double s = sin(2.0 * 3.14159265358979323846 * f->shake_hz * t + f->shake_phase);
  a[0] = (float)((double)f->gx + (double)f->shake_x * s);
  a[1] = (float)((double)f->gy + (double)f->shake_y * s);
  return EULER_OK;
}

static int force_value_ok(float x) { return isfinite(x) && fabsf(x) <= 1e4f; }

int eu_forcing_check(const euler_forcing* f, const euler_force_box* boxes, int32_t X, int32_t Y, char* why, size_t cap) {
#define REFUSE(...) do { if (why && cap) snprintf(why, cap, __VA_ARGS__); return EULER_EINVAL; } while (0)
  if (f->reserved != 0 || f->reserved2 != 0.0) REFUSE("reserved and reserved2 must be 0");
  if (!force_value_ok(f->gx) || !force_value_ok(f->gy) || !force_value_ok(f->shake_x) || !force_value_ok(f->shake_y))
    REFUSE("gravity (%g, %g) and shake (%g, %g) must be finite and at most 1e4 in size", (double)f->gx, (double)f->gy, (double)f->shake_x, (double)f->shake_y);
  if (!isfinite(f->shake_hz) || f->shake_hz < 0.0 || !isfinite(f->shake_phase)) REFUSE("shake_hz %g must be finite and >= 0, shake_phase %g finite", f->shake_hz, f->shake_phase);
  if (f->nboxes < 0 || f->nboxes > EULER_FORCE_BOXES_MAX) REFUSE("%d boxes (0 ... %d)", f->nboxes, EULER_FORCE_BOXES_MAX);
  if (f->nboxes > 0 && !boxes) REFUSE("%d boxes and a null list", f->nboxes);
  for (int32_t k = 0; k < f->nboxes; ++k)
    if (!force_value_ok(boxes[k].fx) || !force_value_ok(boxes[k].fy)) REFUSE("box %d: force (%g, %g) must be finite and at most 1e4 in size", k, (double)boxes[k].fx, (double)boxes[k].fy);
  for (int32_t k = 0; k < f->nboxes; ++k) {
    const euler_force_box* b = boxes + k;
    if (!eu_interior_box_ok(b->x0, b->y0, b->x1, b->y1, X, Y))
      REFUSE("box %d: [%d, %d] x [%d, %d] is not inside the interior [1, %d] x [1, %d]", k, b->x0, b->x1, b->y0, b->y1, X - 2, Y - 2);
  }
#undef REFUSE
  return EULER_OK;
}

/* (eu_gauge_chunks cuts every box for itself, a tile that n boxes touch n times; here a tile comes once and carries its boxes, so the tiles' bit sets are formed
 * over the tile grid and the touched ones listed row by row) */
size_t eu_force_tiles(const void* boxes, size_t stride, int32_t n, int32_t X, int32_t Y, eu_force_tile* out) {
  return eu_force_tiles_bands(boxes, stride, n, X, Y, 0, (Y + 63) >> 6, out);
}

/* (a tile row is a band: the entries with band_lo <= ty < band_hi, in the order the whole table lists them) */
size_t eu_force_tiles_bands(const void* boxes, size_t stride, int32_t n, int32_t X, int32_t Y, int32_t band_lo, int32_t band_hi, eu_force_tile* out) {
  if (n < 1) return 0;
  const int32_t tnx = (X + 63) >> 6, tny = (Y + 63) >> 6;
  if (band_lo < 0) band_lo = 0;
  if (band_hi > tny) band_hi = tny;
  uint64_t* set = (uint64_t*)calloc((size_t)tnx * (size_t)tny, sizeof(uint64_t));
  if (!set) return (size_t)-1;
  for (int32_t k = 0; k < n; ++k) {
    const int32_t* r = (const int32_t*)((const char*)boxes + (size_t)k * stride);      /* x0, y0, x1, y1 */
    for (int32_t ty = r[1] >> 6; ty <= r[3] >> 6; ++ty)
      for (int32_t tx = r[0] >> 6; tx <= r[2] >> 6; ++tx) set[(size_t)ty * tnx + tx] |= 1ull << k;
  }
  size_t m = 0;
  for (int32_t ty = band_lo; ty < band_hi; ++ty)
    for (int32_t tx = 0; tx < tnx; ++tx) {
      const uint64_t s = set[(size_t)ty * tnx + tx];
      if (!s) continue;
      if (out) { out[m].tx = tx; out[m].ty = ty; out[m].boxes = s; }
      ++m;
    }
  free(set);
  return m;
}

/* the record and the first nboxes boxes as bytes (neither struct has padding): what the ranks of a row-slab job compare.  A count outside the list's range - a record
 * its check refuses - is hashed as it stands, without boxes */
static uint64_t record_digest(const void* rec, size_t rec_bytes, const void* boxes, size_t box_bytes, int32_t nboxes, int32_t max_boxes) {
  uint64_t h = eu_fnv1a64(EU_FNV_BASIS, rec, rec_bytes);
  if (boxes && nboxes > 0 && nboxes <= max_boxes) h = eu_fnv1a64(h, boxes, (size_t)nboxes * box_bytes);
  return h;
}

uint64_t eu_forcing_digest(const euler_forcing* f, const euler_force_box* boxes) {
  return record_digest(f, sizeof *f, boxes, sizeof *boxes, f->nboxes, EULER_FORCE_BOXES_MAX);
}

uint64_t eu_heat_digest(const euler_heat* h, const euler_heat_box* boxes) {
  if (!h) return eu_fnv1a64(EU_FNV_BASIS, "off", 3);      /* switching off (euler_set_heat with a null record) against a rank that switches on */
  return record_digest(h, sizeof *h, boxes, sizeof *boxes, h->nboxes, EULER_HEAT_BOXES_MAX);
}

/* ---- moving bodies: the law of motion, the list checked, the unit shifts and their strips (include/euler.h, docs/bodies.md) ---- */

static double body_clamp(double p, double lo, double hi) { return p < lo ? lo : p > hi ? hi : p; }

int euler_body_at(const euler_body* b, double t, int32_t X, int32_t Y, euler_body_state* out) {
  if (!b || !out || b->w < 1 || b->h < 1 || b->w > X - 4 || b->h > Y - 4) return EULER_EINVAL;
  const double s = sin(2.0 * 3.14159265358979323846 * b->hz * t + b->phase);
  const double px = b->x + (double)b->vx * t + (double)b->amp_x * s, py = b->y + (double)b->vy * t + (double)b->amp_y * s;
  /* (a NaN fails both comparisons of the clamp: euler_set_bodies lets none in; here it is held at the lower bound so that the origin is always a cell of the grid) */
  out->px = px == px ? body_clamp(px, 2.0, (double)(X - 2 - b->w)) : 2.0;
  out->py = py == py ? body_clamp(py, 2.0, (double)(Y - 2 - b->h)) : 2.0;
  out->ox = (int32_t)floor(out->px + 0.5);
  out->oy = (int32_t)floor(out->py + 0.5);
  return EULER_OK;
}

int eu_body_check(const euler_body* b, int32_t n, int32_t X, int32_t Y, char* why, size_t cap) {
#define REFUSE(...) do { if (why && cap) snprintf(why, cap, __VA_ARGS__); return EULER_EINVAL; } while (0)
  if (n < 0 || n > EULER_BODIES_MAX) REFUSE("%d bodies (0 ... %d)", n, EULER_BODIES_MAX);
  if (n > 0 && !b) REFUSE("%d bodies and a null list", n);
  const double two_pi = 2.0 * 3.14159265358979323846;
  for (int32_t k = 0; k < n; ++k) {      /* the first body that fails any of its tests */
    const euler_body* q = b + k;
    if (q->reserved[0] != 0 || q->reserved[1] != 0) REFUSE("body %d: reserved must be 0", k);
    if (!isfinite(q->x) || !isfinite(q->y) || !isfinite(q->hz) || !isfinite(q->phase) || !isfinite(q->vx) || !isfinite(q->vy) || !isfinite(q->amp_x) || !isfinite(q->amp_y))
      REFUSE("body %d: a value that is not finite", k);
    if (q->w < 1 || q->h < 1 || q->w > X - 4 || q->h > Y - 4) REFUSE("body %d: %d x %d cells do not fit [2, %d] x [2, %d]", k, q->w, q->h, X - 3, Y - 3);
    if (q->hz < 0.0) REFUSE("body %d: hz %g must be >= 0", k, q->hz);
    const double sx = fabs((double)q->vx) + two_pi * q->hz * fabs((double)q->amp_x), sy = fabs((double)q->vy) + two_pi * q->hz * fabs((double)q->amp_y);
    if (sx > 10.0 || sy > 10.0) REFUSE("body %d: a speed of up to (%g, %g) cells per second, more than 10", k, sx, sy);
  }
#undef REFUSE
  return EULER_OK;
}

int64_t eu_body_plan(int32_t ox, int32_t oy, int32_t tx, int32_t ty, eu_body_shift* out, int64_t cap) {
  const int64_t nx = tx >= ox ? (int64_t)tx - ox : (int64_t)ox - tx, ny = ty >= oy ? (int64_t)ty - oy : (int64_t)oy - ty;
  for (int64_t k = 0; out && k < nx + ny && k < cap; ++k) {
    out[k].axis = k < nx ? 0 : 1;
    out[k].dir = k < nx ? (tx > ox ? 1 : -1) : (ty > oy ? 1 : -1);
  }
  return nx + ny;
}

void eu_body_strips(int32_t ox, int32_t oy, int32_t w, int32_t h, eu_body_shift s, int32_t fill[4], int32_t clear[4]) {
  if (s.axis == 0) {
    const int32_t xf = s.dir > 0 ? ox + w : ox - 1, xc = s.dir > 0 ? ox : ox + w - 1;
    fill[0] = fill[2] = xf; clear[0] = clear[2] = xc;
    fill[1] = clear[1] = oy; fill[3] = clear[3] = oy + h - 1;
  } else {
    const int32_t yf = s.dir > 0 ? oy + h : oy - 1, yc = s.dir > 0 ? oy : oy + h - 1;
    fill[1] = fill[3] = yf; clear[1] = clear[3] = yc;
    fill[0] = clear[0] = ox; fill[2] = clear[2] = ox + w - 1;
  }
}

/* ---- marker density control: the record checked, one pass restated sequentially (include/euler.h, docs/reseed.md) ---- */

int eu_reseed_check(const euler_reseed* r, char* why, size_t cap) {
#define REFUSE(...) do { if (why && cap) snprintf(why, cap, __VA_ARGS__); return EULER_EINVAL; } while (0)
  for (int k = 0; k < 4; ++k)
    if (r->reserved[k] != 0) REFUSE("reserved must be 0");
  if (r->thin_above != 0 && (r->thin_above < 4 || r->thin_above > 254)) REFUSE("thin_above %d is neither 0 nor in [4, 254]", r->thin_above);
  if (r->fill_holes != 0 && r->fill_holes != 1) REFUSE("fill_holes %d is neither 0 nor 1", r->fill_holes);
  if (r->max_cells < 0 || r->max_cells > EU_RESEED_MAX_LIMIT) REFUSE("max_cells %d is outside [0, %d]", r->max_cells, EU_RESEED_MAX_LIMIT);
  if (r->max_fill < 0 || r->max_fill > EU_RESEED_MAX_LIMIT) REFUSE("max_fill %d is outside [0, %d]", r->max_fill, EU_RESEED_MAX_LIMIT);
#undef REFUSE
  return EULER_OK;
}

int eu_reseed_pass(const euler_reseed* r, int32_t X, int32_t Y, float* m, uint64_t* n_io, uint64_t max_markers, uint8_t* count, const uint8_t* prev_count,
                   const uint8_t* solid, const uint8_t* sink, const uint8_t* source, uint64_t* rng_state, euler_reseed_stats* stats) {
  if (!r || !m || !n_io || !count || !prev_count || !solid || !sink || !source || !rng_state || X < 3 || Y < 3 || eu_reseed_check(r, NULL, 0)) return EULER_EINVAL;
  const size_t C = (size_t)X * (size_t)Y;
  uint64_t n = *n_io, removed = 0, added = 0, thinned = 0, deferred = 0;
  if (r->thin_above) {
    /* the list: slot[c] = 1 + the cell's rank in it, 0 for every other cell */
    const uint64_t cap = (uint64_t)eu_reseed_limit(r->max_cells);
    uint32_t* slot = (uint32_t*)calloc(C, sizeof *slot);
    uint8_t* gone = (uint8_t*)calloc(n ? n : 1, 1);
    uint64_t K = 0;
    if (slot && gone)
      for (size_t c = 0; c < C; ++c)
        if (count[c] > r->thin_above) { if (K < cap) slot[c] = (uint32_t)++K; else ++deferred; }
    uint8_t* seen = slot && gone ? (uint8_t*)calloc(K ? 16 * K : 1, 1) : NULL;
    if (!seen) { free(slot); free(gone); return EULER_ENOMEM; }
    /* the flags, before any deletion: ascending i, so the first marker met in a sub-cell is the one with the lowest index */
    for (uint64_t i = 0; i < n; ++i) {
      const int32_t cx = (int32_t)floorf(m[2 * i]), cy = (int32_t)floorf(m[2 * i + 1]);
      const uint32_t k = slot[(size_t)cy * X + cx];
      if (!k) continue;
      uint8_t* s = seen + 16 * (size_t)(k - 1) + 4 * eu_reseed_subcell(m[2 * i + 1], cy) + eu_reseed_subcell(m[2 * i], cx);
      if (*s) gone[i] = 1; else *s = 1;
    }
    /* refresh_marker_counts' loop (main.c:105-116): the last marker takes the place of a deleted one - with its flag - and is examined next */
    for (uint64_t i = 0; i < n;) {
      if (!gone[i]) { ++i; continue; }
      --n; ++removed;
      m[2 * i] = m[2 * n]; m[2 * i + 1] = m[2 * n + 1]; gone[i] = gone[n];
    }
    for (size_t c = 0; c < C; ++c) {
      if (!slot[c]) continue;
      int occ = 0;
      for (int q = 0; q < 16; ++q) occ += seen[16 * (size_t)(slot[c] - 1) + q];
      count[c] = (uint8_t)occ;
    }
    thinned = K;
    free(slot); free(gone); free(seen);
  }
  if (r->fill_holes) {
    const uint64_t cap = (uint64_t)eu_reseed_limit(r->max_fill);
    uint8_t* hole = (uint8_t*)calloc(C, 1);      /* all of them first: a filled hole must not count as a wet neighbour of the next */
    if (!hole) return EULER_ENOMEM;
    for (int32_t y = 1; y < Y - 1; ++y)
      for (int32_t x = 1; x < X - 1; ++x) {
        const size_t c = (size_t)y * X + x;
        if (count[c] != 0 || prev_count[c] == 0 || solid[c] || sink[c] || source[c]) continue;
        int wet = 1;
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx) {
            const size_t q = (size_t)(y + dy) * X + (x + dx);
            if ((dx || dy) && count[q] == 0 && !solid[q]) wet = 0;
          }
        hole[c] = (uint8_t)wet;
      }
    uint64_t listed = 0;
    for (size_t c = 0; c < C; ++c) {
      if (!hole[c]) continue;
      if (listed == cap || n + 1 > max_markers - 1) { ++deferred; continue; }
      ++listed;
      const float ry = euler_rng_next_float(rng_state), rx = euler_rng_next_float(rng_state);
      m[2 * n] = (float)(int32_t)(c % (size_t)X) + rx; m[2 * n + 1] = (float)(int32_t)(c / (size_t)X) + ry;
      ++n; ++added;
      count[c] = 1;
    }
    free(hole);
  }
  *n_io = n;
  if (stats) { stats->removed += removed; stats->added += added; stats->cells_thinned += thinned; stats->deferred += deferred; }
  return EULER_OK;
}

/* ---- temperature: the record's defaults, the record and the list checked, the boxes' tile table is eu_force_tiles' (include/euler.h, docs/heat.md) ---- */

int euler_heat_default(euler_heat* h) {
  if (!h) return EULER_EINVAL;
  memset(h, 0, sizeof *h);
  return EULER_OK;
}

int eu_heat_value_ok(float x) { return force_value_ok(x); }

int eu_heat_box_check(int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t X, int32_t Y, char* why, size_t cap) {
  if (!eu_interior_box_ok(x0, y0, x1, y1, X, Y)) {
    if (why && cap) snprintf(why, cap, "[%d, %d] x [%d, %d] is not inside the interior [1, %d] x [1, %d]", x0, x1, y0, y1, X - 2, Y - 2);
    return EULER_EINVAL;
  }
  return EULER_OK;
}

int eu_heat_check(const euler_heat* h, const euler_heat_box* boxes, int32_t X, int32_t Y, const float* live, char* why, size_t cap) {
#define REFUSE(...) do { if (why && cap) snprintf(why, cap, __VA_ARGS__); return EULER_EINVAL; } while (0)
  if (h->reserved != 0 || h->reserved2 != 0.0) REFUSE("reserved and reserved2 must be 0");
  if (!isfinite(h->kappa) || !force_value_ok(h->ambient) || !force_value_ok(h->beta) || !force_value_ok(h->source_t))
    REFUSE("ambient %g, beta %g and source_t %g must be finite and at most 1e4 in size, kappa %g finite", (double)h->ambient, (double)h->beta, (double)h->source_t, (double)h->kappa);
  if (!(h->kappa >= 0.f && h->kappa <= 2.5f)) REFUSE("kappa %g is outside [0, 2.5]", (double)h->kappa);
  if (live && !(h->ambient == *live)) REFUSE("ambient %g is not the live one, %g (the cells without markers hold it)", (double)h->ambient, (double)*live);
  if (h->nboxes < 0 || h->nboxes > EULER_HEAT_BOXES_MAX) REFUSE("%d boxes (0 ... %d)", h->nboxes, EULER_HEAT_BOXES_MAX);
  if (h->nboxes > 0 && !boxes) REFUSE("%d boxes and a null list", h->nboxes);
  for (int32_t k = 0; k < h->nboxes; ++k) {      /* the first box that fails any of its tests */
    const euler_heat_box* b = boxes + k;
    char place[160];
    if (b->kind != EULER_HEAT_FIX && b->kind != EULER_HEAT_RATE) REFUSE("box %d: kind %d is neither EULER_HEAT_FIX nor EULER_HEAT_RATE", k, b->kind);
    if (!force_value_ok(b->value)) REFUSE("box %d: value %g must be finite and at most 1e4 in size", k, (double)b->value);
    if (eu_heat_box_check(b->x0, b->y0, b->x1, b->y1, X, Y, place, sizeof place)) REFUSE("box %d: %s", k, place);
  }
#undef REFUSE
  return EULER_OK;
}

int euler_gauge_derive(const euler_gauge_rec* rec, int32_t kind, euler_gauge_values* out) {
  if (!rec || !out || kind < EULER_GAUGE_LEVEL || kind > EULER_GAUGE_FLUX) return EULER_EINVAL;
  memset(out, 0, sizeof *out);
  if (!rec->fluid) return EULER_OK;
  const double scale = kind == EULER_GAUGE_FLUX ? 1048576.0 : 256.0;
  out->a = ((double)rec->a_pos - (double)rec->a_neg) / scale;
  out->b = ((double)rec->b_pos - (double)rec->b_neg) / scale;
  out->mean_a = rec->terms ? out->a / (double)rec->terms : 0.0;
  out->depth = (double)rec->hi_y - (double)rec->lo_y + 1.0;
  return EULER_OK;
}

/* ---- passive tracers: the checks of euler_tracers_add that need no device, the lattice of a box, the painter (include/euler.h, docs/tracers.md) ---- */

int eu_tracers_check(const float* xy, size_t n, size_t count, int32_t X, int32_t Y, char* why, size_t cap) {
#define REFUSE(...) do { if (why && cap) snprintf(why, cap, __VA_ARGS__); return EULER_EINVAL; } while (0)
  if (n > 0 && !xy) REFUSE("%zu tracers and a null list", n);
  if (count > EULER_TRACERS_MAX || n > EULER_TRACERS_MAX - count) REFUSE("%zu + %zu tracers (at most %u)", count, n, (unsigned)EULER_TRACERS_MAX);
  const float xl = (float)(X - 1), yl = (float)(Y - 1);
  for (size_t k = 0; k < n; ++k) {
    const float x = xy[2 * k], y = xy[2 * k + 1];
    if (!(x >= 1.f && x < xl && y >= 1.f && y < yl))      /* (a NaN fails every comparison, an infinity one of them) */
      REFUSE("tracer %zu: (%g, %g) is not a finite position inside [1, %d) x [1, %d)", k, (double)x, (double)y, X - 1, Y - 1);
  }
#undef REFUSE
  return EULER_OK;
}

size_t eu_tracer_lattice(int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t K, float* xy) {
  if ((K != 1 && K != 2 && K != 4) || x0 > x1 || y0 > y1) return 0;
  const size_t n = (size_t)(x1 - x0 + 1) * (size_t)(y1 - y0 + 1) * (size_t)(K * K);
  if (!xy) return n;
  size_t m = 0;
  for (int32_t x = x0; x <= x1; ++x)
    for (int32_t y = y0; y <= y1; ++y)
      for (int32_t i = 0; i < K; ++i)
        for (int32_t j = 0; j < K; ++j) {
          xy[2 * m] = (float)x + ((float)i + 0.5f) / (float)K;
          xy[2 * m + 1] = (float)y + ((float)j + 0.5f) / (float)K;
          ++m;
        }
  return n;
}

int euler_tracer_paint(const uint32_t* counts, euler_overview_px* px, int32_t W, int32_t H, const float fg[3], const float* bg) {
  if (!counts || !px || !fg || W < 1 || H < 1) return EULER_EINVAL;
  const size_t n = (size_t)W * (size_t)H;
  for (size_t k = 0; k < n; ++k) {
    if (!px[k].water) continue;      /* a tracer shows only on water pixels */
    const float* col = counts[k] > 0 ? fg : bg;
    if (!col) continue;
    for (int c = 0; c < 3; ++c) px[k].dye[c] = (uint64_t)px[k].water * paint_q24(col[c]);
  }
  return EULER_OK;
}

/* ---- session files: a version-4 snapshot composed, parsed and checked in memory (include/euler.h "session files", docs/session.md) ---- */

uint64_t eu_fnv1a64(uint64_t h, const void* p, size_t n) {
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}

#define SE_HEADER 72u
#define SE_CHUNK_HEADER 16u
#define SE_NCHUNKS 9
static const char SE_TAGS[SE_NCHUNKS][4] = {{'T', 'I', 'M', 'E'}, {'F', 'O', 'R', 'C'}, {'H', 'E', 'A', 'T'}, {'T', 'R', 'A', 'C'},
                                   {'B', 'O', 'D', 'Y'}, {'R', 'S', 'E', 'D'}, {'S', 'E', 'T', 'T'}, {'S', 'T', 'A', 'T'}, {'E', 'N', 'D', 0}};
static size_t se_pad8(size_t n) { return (n + 7u) & ~(size_t)7u; }

size_t eu_session_core_bytes(int32_t X, int32_t Y, int32_t dye, uint64_t n_markers) {
  const size_t C = (size_t)X * (size_t)Y;
  return SE_HEADER + C * 29u + (dye ? C * 24u : 0u) + (size_t)n_markers * 8u;
}

/* the payload sizes of the chunks, in file order */
static void se_payloads(const eu_session* s, size_t out[SE_NCHUNKS]) {
  const size_t C = (size_t)s->X * (size_t)s->Y;
  out[0] = 8;
  out[1] = sizeof(euler_forcing) + (size_t)s->forcing.nboxes * sizeof(euler_force_box);
  out[2] = 8 + sizeof(euler_heat) + (size_t)s->heat.nboxes * sizeof(euler_heat_box) + (s->heat_on ? C * 4u : 0u);
  out[3] = 8 + (size_t)s->n_tracers * sizeof(euler_tracer);
  out[4] = 8 + (size_t)s->n_bodies * (sizeof(euler_body) + 8u);
  out[5] = sizeof(euler_reseed) + sizeof(euler_reseed_stats);
  out[6] = sizeof(eu_session_settings);
  out[7] = 40;
  out[8] = 0;
}

size_t eu_session_chunk_bytes(const eu_session* s) {
  size_t pay[SE_NCHUNKS], n = 0;
  se_payloads(s, pay);
  for (int k = 0; k < SE_NCHUNKS; ++k) n += SE_CHUNK_HEADER + se_pad8(pay[k]);
  return n;
}

size_t eu_session_put_chunks(const eu_session* s, unsigned char* out) {
  size_t pay[SE_NCHUNKS];
  se_payloads(s, pay);
  const size_t C = (size_t)s->X * (size_t)s->Y;
  unsigned char* w = out;
#define PUT(p, n) do { if ((n) > 0) memcpy(w, (p), (n)); w += (n); } while (0)
  for (int k = 0; k < SE_NCHUNKS; ++k) {
    const uint32_t version = 1;
    const uint64_t bytes = (uint64_t)pay[k];
    unsigned char* const start = w + SE_CHUNK_HEADER;
    PUT(SE_TAGS[k], 4); PUT(&version, 4); PUT(&bytes, 8);
    const int32_t zero = 0;
    switch (k) {
      case 0: PUT(&s->time, 8); break;
      case 1: PUT(&s->forcing, sizeof s->forcing); PUT(s->force_boxes, (size_t)s->forcing.nboxes * sizeof(euler_force_box)); break;
      case 2: { const int32_t on = s->heat_on ? 1 : 0;
        PUT(&on, 4); PUT(&zero, 4); PUT(&s->heat, sizeof s->heat); PUT(s->heat_boxes, (size_t)s->heat.nboxes * sizeof(euler_heat_box));
        if (on) PUT(s->heat_field, C * 4u);
        break; }
      case 3: PUT(&s->n_tracers, 8); PUT(s->tracers, (size_t)s->n_tracers * sizeof(euler_tracer)); break;
      case 4: PUT(&s->n_bodies, 4); PUT(&zero, 4); PUT(s->bodies, (size_t)s->n_bodies * sizeof(euler_body));
        for (int32_t b = 0; b < s->n_bodies; ++b) { PUT(&s->body_ox[b], 4); PUT(&s->body_oy[b], 4); }
        break;
      case 5: PUT(&s->reseed, sizeof s->reseed); PUT(&s->reseed_stats, sizeof s->reseed_stats); break;
      case 6: PUT(&s->settings, sizeof s->settings); break;
      case 7: PUT(&s->last_substeps, 4); PUT(&s->last_pcg_iterations, 4); PUT(&s->last_residual, 8); PUT(&s->last_dt, 4); PUT(&zero, 4);
        PUT(&s->marker_dt_events, 8); PUT(&s->marker_multi_events, 8);
        break;
      default: break;
    }
    while ((size_t)(w - start) < se_pad8(pay[k])) *w++ = 0;
  }
#undef PUT
  return (size_t)(w - out);
}

int eu_session_parse(const void* buf, size_t n, int32_t X, int32_t Y, int32_t dye, uint64_t max_markers, eu_session* out, char* why, size_t cap) {
#define REFUSE(code, ...) do { if (why && cap) snprintf(why, cap, __VA_ARGS__); return (code); } while (0)
  if (!buf || !out || X < 3 || Y < 3) REFUSE(EULER_EINVAL, "null argument or a grid below 3 x 3");
  const unsigned char* b = (const unsigned char*)buf;
  eu_session s;
  memset(&s, 0, sizeof s);
  uint32_t version, reserved;
  int32_t reserved2;
  if (n < SE_HEADER + 8u) REFUSE(EULER_EIO, "truncated: %zu bytes are less than a header and a checksum", n);
  if (memcmp(b, "EULERSNP", 8) != 0) REFUSE(EULER_EINVAL, "not an euler state snapshot");
  memcpy(&version, b + 8, 4); memcpy(&s.X, b + 12, 4); memcpy(&s.Y, b + 16, 4); memcpy(&reserved, b + 20, 4);
  memcpy(&s.n_markers, b + 24, 8); memcpy(&s.rng_state, b + 32, 8); memcpy(&s.source_exhausted, b + 40, 4); memcpy(&reserved2, b + 44, 4);
  memcpy(&s.frames, b + 48, 8); memcpy(&s.total_substeps, b + 56, 8); memcpy(&s.total_pcg_iterations, b + 64, 8);
  if (version != 4) REFUSE(EULER_EINVAL, "snapshot version %u is not a session file (version 4)", version);
  if (s.X != X || s.Y != Y) REFUSE(EULER_EINVAL, "session grid %dx%d does not fit this %dx%d handle", s.X, s.Y, X, Y);
  if ((reserved & ~1u) != 0 || reserved2 != 0) REFUSE(EULER_EINVAL, "reserved header words %u, %d", reserved, reserved2);
  s.dye = (int32_t)(reserved & 1u);
  if (s.dye != (dye != 0)) REFUSE(EULER_EINVAL, "the session %s the dye fields but this handle was created %s euler_config.rainbow", s.dye ? "carries" : "lacks", dye ? "with" : "without");
  if (s.n_markers > max_markers) REFUSE(EULER_EINVAL, "the session holds %llu markers, more than this handle's capacity %llu", (unsigned long long)s.n_markers, (unsigned long long)max_markers);
  const size_t C = (size_t)X * (size_t)Y, core = eu_session_core_bytes(X, Y, s.dye, s.n_markers), end = n - 8u;
  if (core > end) REFUSE(EULER_EIO, "truncated: the arrays and markers need %zu bytes, the file has %zu", core + 8u, n);
  uint64_t stored;
  memcpy(&stored, b + end, 8);
  if (stored != eu_fnv1a64(EU_FNV_BASIS, b, end)) REFUSE(EULER_EIO, "truncated or corrupt (checksum)");
  s.solid = b + SE_HEADER + C * 16u;
  /* the chunks: each in its place, its size the one its own counts give */
  size_t at = core;
  for (int k = 0; k < SE_NCHUNKS; ++k) {
    char tag[5] = {0, 0, 0, 0, 0};
    uint32_t cv;
    uint64_t bytes;
    if (end - at < SE_CHUNK_HEADER) REFUSE(EULER_EINVAL, "the chunks end in front of %.4s (every session ends with an END chunk)", SE_TAGS[k]);
    memcpy(tag, b + at, 4); memcpy(&cv, b + at + 4, 4); memcpy(&bytes, b + at + 8, 8);
    for (int c = 0; c < 4; ++c) if (tag[c] != 0 && (tag[c] < 32 || tag[c] > 126)) tag[c] = '?';
    if (memcmp(b + at, SE_TAGS[k], 4) != 0) {
      int known = 0;
      for (int j = 0; j < SE_NCHUNKS; ++j) known |= memcmp(b + at, SE_TAGS[j], 4) == 0;
      if (known) REFUSE(EULER_EINVAL, "chunk %s stands where %.4s belongs (the chunks come once each, in a fixed order)", tag, SE_TAGS[k]);
      REFUSE(EULER_EINVAL, "unknown chunk tag '%s' where %.4s belongs", tag, SE_TAGS[k]);
    }
    if (cv != 1) REFUSE(EULER_EINVAL, "chunk %s: unknown chunk version %u", tag, cv);
    at += SE_CHUNK_HEADER;
    if (bytes > end - at || se_pad8((size_t)bytes) > end - at) REFUSE(EULER_EINVAL, "chunk %s: %llu bytes of payload, %zu left in the file", tag, (unsigned long long)bytes, end - at);
    const unsigned char* p = b + at;
    const size_t len = (size_t)bytes;
    size_t want = 0;
    char rec[320];
#define SIZE_IS(w) do { want = (w); if (len != want) REFUSE(EULER_EINVAL, "chunk %s: %zu bytes of payload, its counts give %zu", tag, len, want); } while (0)
#define AT_LEAST(w) do { if (len < (size_t)(w)) REFUSE(EULER_EINVAL, "chunk %s: %zu bytes of payload are less than its fixed part, %zu", tag, len, (size_t)(w)); } while (0)
    switch (k) {
      case 0:
        SIZE_IS(8);
        memcpy(&s.time, p, 8);
        if (!isfinite(s.time)) REFUSE(EULER_EINVAL, "chunk TIME: the clock is not finite");
        break;
      case 1:
        AT_LEAST(sizeof s.forcing);
        memcpy(&s.forcing, p, sizeof s.forcing);
        if (s.forcing.nboxes < 0 || s.forcing.nboxes > EULER_FORCE_BOXES_MAX) REFUSE(EULER_EINVAL, "chunk FORC: %d boxes (0 ... %d)", s.forcing.nboxes, EULER_FORCE_BOXES_MAX);
        SIZE_IS(sizeof s.forcing + (size_t)s.forcing.nboxes * sizeof(euler_force_box));
        memcpy(s.force_boxes, p + sizeof s.forcing, (size_t)s.forcing.nboxes * sizeof(euler_force_box));
        if (eu_forcing_check(&s.forcing, s.force_boxes, X, Y, rec, sizeof rec)) REFUSE(EULER_EINVAL, "chunk FORC: %s", rec);
        break;
      case 2: {
        int32_t pad;
        AT_LEAST(8 + sizeof s.heat);
        memcpy(&s.heat_on, p, 4); memcpy(&pad, p + 4, 4); memcpy(&s.heat, p + 8, sizeof s.heat);
        if ((s.heat_on != 0 && s.heat_on != 1) || pad != 0) REFUSE(EULER_EINVAL, "chunk HEAT: on = %d, pad = %d", s.heat_on, pad);
        if (s.heat.nboxes < 0 || s.heat.nboxes > EULER_HEAT_BOXES_MAX) REFUSE(EULER_EINVAL, "chunk HEAT: %d boxes (0 ... %d)", s.heat.nboxes, EULER_HEAT_BOXES_MAX);
        const size_t fixed = 8 + sizeof s.heat + (size_t)s.heat.nboxes * sizeof(euler_heat_box);
        SIZE_IS(fixed + (s.heat_on ? C * 4u : 0u));
        memcpy(s.heat_boxes, p + 8 + sizeof s.heat, (size_t)s.heat.nboxes * sizeof(euler_heat_box));
        if (eu_heat_check(&s.heat, s.heat_boxes, X, Y, NULL, rec, sizeof rec)) REFUSE(EULER_EINVAL, "chunk HEAT: %s", rec);
        if (s.heat_on) {
          s.heat_field = p + fixed;
          for (size_t i = 0; i < C; ++i) {
            float t;
            memcpy(&t, s.heat_field + 4u * i, 4);
            if (!eu_heat_value_ok(t)) REFUSE(EULER_EINVAL, "chunk HEAT: cell %zu holds %g (finite and at most 1e4 in size)", i, (double)t);
          }
        }
        break; }
      case 3:
        AT_LEAST(8);
        memcpy(&s.n_tracers, p, 8);
        if (s.n_tracers > EULER_TRACERS_MAX) REFUSE(EULER_EINVAL, "chunk TRAC: %llu tracers (at most %u)", (unsigned long long)s.n_tracers, (unsigned)EULER_TRACERS_MAX);
        SIZE_IS(8 + (size_t)s.n_tracers * sizeof(euler_tracer));
        s.tracers = p + 8;
        for (uint64_t i = 0; i < s.n_tracers; ++i) {
          euler_tracer t;
          memcpy(&t, s.tracers + (size_t)i * sizeof t, sizeof t);
          if (t.reserved != 0) REFUSE(EULER_EINVAL, "chunk TRAC: tracer %llu: reserved must be 0", (unsigned long long)i);
          if (!(isfinite(t.x) && isfinite(t.y)) && (t.flags & (EULER_TRACER_RETIRED | EULER_TRACER_LOST)) != (EULER_TRACER_RETIRED | EULER_TRACER_LOST))
            REFUSE(EULER_EINVAL, "chunk TRAC: tracer %llu: a position that is not finite on a record that is not flagged lost", (unsigned long long)i);
        }
        break;
      case 4: {
        int32_t pad;
        AT_LEAST(8);
        memcpy(&s.n_bodies, p, 4); memcpy(&pad, p + 4, 4);
        if (s.n_bodies < 0 || s.n_bodies > EULER_BODIES_MAX || pad != 0) REFUSE(EULER_EINVAL, "chunk BODY: %d bodies (0 ... %d), pad = %d", s.n_bodies, EULER_BODIES_MAX, pad);
        SIZE_IS(8 + (size_t)s.n_bodies * (sizeof(euler_body) + 8u));
        memcpy(s.bodies, p + 8, (size_t)s.n_bodies * sizeof(euler_body));
        if (eu_body_check(s.bodies, s.n_bodies, X, Y, rec, sizeof rec)) REFUSE(EULER_EINVAL, "chunk BODY: %s", rec);
        for (int32_t q = 0; q < s.n_bodies; ++q) {
          const unsigned char* o = p + 8 + (size_t)s.n_bodies * sizeof(euler_body) + 8u * (size_t)q;
          memcpy(&s.body_ox[q], o, 4); memcpy(&s.body_oy[q], o + 4, 4);
          const int32_t ox = s.body_ox[q], oy = s.body_oy[q], w = s.bodies[q].w, h = s.bodies[q].h;
          if (ox < 2 || oy < 2 || ox > X - 2 - w || oy > Y - 2 - h) REFUSE(EULER_EINVAL, "chunk BODY: body %d: the origin (%d, %d) leaves [2, %d] x [2, %d]", q, ox, oy, X - 2 - w, Y - 2 - h);
          for (int32_t y = oy; y < oy + h; ++y)
            for (int32_t x = ox; x < ox + w; ++x)
              if (!s.solid[(size_t)y * (size_t)X + (size_t)x]) REFUSE(EULER_EINVAL, "chunk BODY: body %d stands at (%d, %d) but cell (%d, %d) of the session's solid grid is open", q, ox, oy, x, y);
        }
        break; }
      case 5:
        SIZE_IS(sizeof s.reseed + sizeof s.reseed_stats);
        memcpy(&s.reseed, p, sizeof s.reseed); memcpy(&s.reseed_stats, p + sizeof s.reseed, sizeof s.reseed_stats);
        if (eu_reseed_check(&s.reseed, rec, sizeof rec)) REFUSE(EULER_EINVAL, "chunk RSED: %s", rec);
        break;
      case 6:
        SIZE_IS(sizeof s.settings);
        memcpy(&s.settings, p, sizeof s.settings);
        if (s.settings.reserved != 0 || s.settings.nopts < 1 || s.settings.nopts > EU_SESSION_OPTS) REFUSE(EULER_EINVAL, "chunk SETT: nopts = %d, reserved = %d", s.settings.nopts, s.settings.reserved);
        break;
      case 7: {
        int32_t pad;
        SIZE_IS(40);
        memcpy(&s.last_substeps, p, 4); memcpy(&s.last_pcg_iterations, p + 4, 4); memcpy(&s.last_residual, p + 8, 8); memcpy(&s.last_dt, p + 16, 4); memcpy(&pad, p + 20, 4);
        memcpy(&s.marker_dt_events, p + 24, 8); memcpy(&s.marker_multi_events, p + 32, 8);
        if (pad != 0) REFUSE(EULER_EINVAL, "chunk STAT: pad = %d", pad);
        break; }
      default:
        SIZE_IS(0);
        break;
    }
#undef SIZE_IS
#undef AT_LEAST
    at += se_pad8(len);
  }
  if (at != end) REFUSE(EULER_EINVAL, "%zu bytes between the END chunk and the checksum", end - at);
#undef REFUSE
  *out = s;
  return EULER_OK;
}

int eu_session_settings_diff(const eu_session_settings* f, const eu_session_settings* h, char* why, size_t cap) {
#define DIFF_I(field) do { if (f->field != h->field) { if (why && cap) snprintf(why, cap, "%s: the session has %lld, the handle %lld", #field, (long long)f->field, (long long)h->field); return 1; } } while (0)
  DIFF_I(max_iterations); DIFF_I(dot_mode); DIFF_I(precond); DIFF_I(tile_records); DIFF_I(sweep_mode); DIFF_I(max_substeps); DIFF_I(rainbow); DIFF_I(pcg_precision);
  DIFF_I(resident); DIFF_I(pcg_poll_interval);
#undef DIFF_I
  float a, b;
  memcpy(&a, &f->viscosity_bits, 4); memcpy(&b, &h->viscosity_bits, 4);
  if (f->viscosity_bits != h->viscosity_bits) { if (why && cap) snprintf(why, cap, "viscosity: the session has %.9g, the handle %.9g", (double)a, (double)b); return 1; }
  memcpy(&a, &f->frame_time_bits, 4); memcpy(&b, &h->frame_time_bits, 4);
  if (f->frame_time_bits != h->frame_time_bits) { if (why && cap) snprintf(why, cap, "frame_time: the session has %.9g, the handle %.9g", (double)a, (double)b); return 1; }
  if (memcmp(&f->tol, &h->tol, 8) != 0) { if (why && cap) snprintf(why, cap, "tol: the session has %.17g, the handle %.17g", f->tol, h->tol); return 1; }
  const int32_t nopts = f->nopts > h->nopts ? f->nopts : h->nopts;
  for (int32_t k = 1; k < nopts && k < EU_SESSION_OPTS; ++k) {
    if (k == EULER_OPT_RESIDENT_FORCE_TIMEOUT || k == EULER_OPT_MG_SPLIT_ACTIVE || k == EULER_OPT_PROFILE_STRIDE) continue;      /* a test hook that counts down, a read-only result, a measurement's stride */
    if (f->opt[k] != h->opt[k]) { if (why && cap) snprintf(why, cap, "option %d: the session has %lld, the handle %lld", k, (long long)f->opt[k], (long long)h->opt[k]); return 1; }
  }
  return 0;
}
