/* sanitize_reseed.c - the host side of the marker density control (docs/reseed.md) under ASan + UBSan, as a stand-alone program: eu_reseed_check's refusals
 * and their order, the sub-cell index on and next to its boundaries, eu_reseed_pass on hand-made states (a thinned cell, a wrapped count byte, the limits,
 * the eight-neighbour rule, the array's capacity) and on random ones against invariants, the --reseed parser and the line of totals.
 * Built and run by tests/test_reseed_host.py; prints "clean" when every check held. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "euler.h"
#include "euler_host.h"
#include "cli_reseed.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static euler_reseed rec(int thin, int fill, int max_cells, int max_fill) {
  euler_reseed r;
  memset(&r, 0, sizeof r);
  r.thin_above = thin; r.fill_holes = fill; r.max_cells = max_cells; r.max_fill = max_fill;
  return r;
}

static int refused(const euler_reseed* r, const char* word) {
  char why[160] = "";
  const int rc = eu_reseed_check(r, why, sizeof why);
  if (rc != EULER_EINVAL || !strstr(why, word)) { fprintf(stderr, "expected a refusal with \"%s\", got %d \"%s\"\n", word, rc, why); return 0; }
  return 1;
}

static void check_refusals(void) {
  euler_reseed r = rec(16, 1, 0, 0);
  CHECK(sizeof(euler_reseed) == 32 && sizeof(euler_reseed_stats) == 32);
  CHECK(eu_reseed_check(&r, NULL, 0) == EULER_OK);
  r = rec(0, 0, 0, 0); CHECK(eu_reseed_check(&r, NULL, 0) == EULER_OK);
  r = rec(4, 0, 1 << 20, 1 << 20); CHECK(eu_reseed_check(&r, NULL, 0) == EULER_OK);
  r = rec(254, 1, 1, 1); CHECK(eu_reseed_check(&r, NULL, 0) == EULER_OK);
  /* in this order: reserved, thin_above, fill_holes, the limits */
  r = rec(3, 2, -1, -1); r.reserved[3] = 1; CHECK(refused(&r, "reserved"));
  r = rec(3, 2, -1, -1); CHECK(refused(&r, "thin_above"));
  r = rec(255, 0, 0, 0); CHECK(refused(&r, "thin_above"));
  r = rec(-16, 0, 0, 0); CHECK(refused(&r, "thin_above"));
  r = rec(1, 0, 0, 0); CHECK(refused(&r, "thin_above"));
  r = rec(16, 2, -1, -1); CHECK(refused(&r, "fill_holes"));
  r = rec(16, -1, 0, 0); CHECK(refused(&r, "fill_holes"));
  r = rec(16, 1, -1, -1); CHECK(refused(&r, "max_cells"));
  r = rec(16, 1, (1 << 20) + 1, 0); CHECK(refused(&r, "max_cells"));
  r = rec(16, 1, 0, -1); CHECK(refused(&r, "max_fill"));
  r = rec(16, 1, 0, (1 << 20) + 1); CHECK(refused(&r, "max_fill"));
  CHECK(eu_reseed_check(&r, NULL, 0) == EULER_EINVAL);      /* no room for the reason: the code alone */
  CHECK(eu_reseed_limit(0) == 65536 && eu_reseed_limit(7) == 7);
}

static void check_subcell(void) {
  CHECK(eu_reseed_subcell(5.f, 5) == 0 && eu_reseed_subcell(5.25f, 5) == 1 && eu_reseed_subcell(5.5f, 5) == 2 && eu_reseed_subcell(5.75f, 5) == 3);
  CHECK(eu_reseed_subcell(nextafterf(5.25f, 0.f), 5) == 0 && eu_reseed_subcell(nextafterf(5.5f, 0.f), 5) == 1 && eu_reseed_subcell(nextafterf(6.f, 0.f), 5) == 3);
  CHECK(eu_reseed_subcell(0.f, 0) == 0 && eu_reseed_subcell(nextafterf(1.f, 0.f), 0) == 3);
  CHECK(eu_reseed_subcell(1000.75f, 1000) == 3 && eu_reseed_subcell(nextafterf(16384.f, 0.f), 16383) == 3);
  CHECK(eu_reseed_subcell(6.f, 5) == 3);      /* the clamp: a coordinate the caller's floor would never pair with this cell */
}

typedef struct scene {
  int X, Y;
  size_t C;
  uint8_t *count, *prev, *solid, *sink, *source;
  float* m;
  uint64_t n, cap, rng;
} scene;

static scene scene_new(int X, int Y) {
  scene s;
  memset(&s, 0, sizeof s);
  s.X = X; s.Y = Y; s.C = (size_t)X * Y; s.cap = 4 * s.C; s.rng = 0x9bd185c449534b91ull;
  s.count = calloc(s.C, 1); s.prev = calloc(s.C, 1); s.solid = calloc(s.C, 1); s.sink = calloc(s.C, 1); s.source = calloc(s.C, 1);
  s.m = calloc(2 * s.cap, sizeof(float));      /* EXACTLY the capacity: a marker written past max_markers - 1 would be caught */
  if (!s.count || !s.prev || !s.solid || !s.sink || !s.source || !s.m) { fprintf(stderr, "out of memory\n"); exit(2); }
  for (int y = 0; y < Y; ++y) { s.sink[(size_t)y * X] = 1; s.sink[(size_t)y * X + X - 1] = 1; }
  for (int x = 0; x < X; ++x) { s.sink[x] = 1; s.sink[(size_t)(Y - 1) * X + x] = 1; }
  return s;
}
static void scene_free(scene* s) { free(s->count); free(s->prev); free(s->solid); free(s->sink); free(s->source); free(s->m); }
static void put(scene* s, float x, float y) { s->m[2 * s->n] = x; s->m[2 * s->n + 1] = y; ++s->n; }
static void rebin(scene* s, int also_prev) {      /* count = the bins, as the refresh leaves them (the byte wraps) */
  uint32_t* c32 = calloc(s->C, sizeof *c32);
  if (!c32) exit(2);
  for (uint64_t i = 0; i < s->n; ++i) ++c32[(size_t)floorf(s->m[2 * i + 1]) * s->X + (size_t)floorf(s->m[2 * i])];
  for (size_t c = 0; c < s->C; ++c) { s->count[c] = (uint8_t)c32[c]; if (also_prev) s->prev[c] = s->count[c]; }
  free(c32);
}
static int run(scene* s, const euler_reseed* r, euler_reseed_stats* st) {
  return eu_reseed_pass(r, s->X, s->Y, s->m, &s->n, s->cap, s->count, s->prev, s->solid, s->sink, s->source, &s->rng, st);
}

static void check_thinning(void) {
  scene s = scene_new(20, 12);
  /* cell (5, 4): 20 markers, five to a sub-cell in four sub-cells, among them duplicates and boundary values; cell (7, 4): 260 (the byte reads 4: left alone);
   * cell (9, 4): 300 (the byte reads 44: thinned); cell (3, 3): 3 markers (left alone) */
  const float fx[4] = {0.f, 0.25f, 0.5f, 0.75f};
  for (int k = 0; k < 20; ++k) put(&s, 5.f + fx[k % 4], 4.f + fx[k % 4]);
  for (int k = 0; k < 260; ++k) put(&s, 7.f + (float)(k % 16) / 16.f, 4.f + (float)(k / 16 % 16) / 16.f);
  for (int k = 0; k < 300; ++k) put(&s, 9.f + (float)(k % 16) / 16.f, 4.f + (float)(k / 16 % 16) / 16.f);
  for (int k = 0; k < 3; ++k) put(&s, 3.5f, 3.5f);
  rebin(&s, 1);
  CHECK(s.count[4 * 20 + 5] == 20 && s.count[4 * 20 + 7] == 4 && s.count[4 * 20 + 9] == 44);
  euler_reseed r = rec(16, 0, 0, 0);
  euler_reseed_stats st;
  memset(&st, 0, sizeof st);
  const uint64_t rng0 = s.rng;
  CHECK(run(&s, &r, &st) == EULER_OK);
  CHECK(s.count[4 * 20 + 5] == 4 && s.count[4 * 20 + 7] == 4 && s.count[4 * 20 + 9] == 16 && s.count[3 * 20 + 3] == 3);
  CHECK(st.cells_thinned == 2 && st.removed == 16 + 284 && st.added == 0 && st.deferred == 0 && s.n == 583 - 300 && s.rng == rng0);
  /* the survivors of cell (5, 4) are its first four markers: still in front, in order (nothing in front of them was deleted) */
  for (int k = 0; k < 4; ++k) CHECK(s.m[2 * k] == 5.f + fx[k] && s.m[2 * k + 1] == 4.f + fx[k]);
  /* max_cells = 1: the first crowded cell in row-major order is thinned, the other deferred; a second pass takes it */
  scene_free(&s);
  s = scene_new(20, 12);
  for (int k = 0; k < 40; ++k) { put(&s, 12.f + (float)(k % 8) / 8.f, 6.f + (float)(k / 8) / 8.f); put(&s, 4.f + (float)(k % 8) / 8.f, 2.f + (float)(k / 8) / 8.f); }
  rebin(&s, 1);
  r = rec(16, 0, 1, 0);
  memset(&st, 0, sizeof st);
  CHECK(run(&s, &r, &st) == EULER_OK);
  CHECK(st.cells_thinned == 1 && st.deferred == 1 && s.count[2 * 20 + 4] == 12 && s.count[6 * 20 + 12] == 40);
  CHECK(run(&s, &r, &st) == EULER_OK);
  CHECK(st.cells_thinned == 2 && st.deferred == 1 && s.count[6 * 20 + 12] == 12 && s.n == 24 && st.removed == 56);
  scene_free(&s);
}

static void check_filling(void) {
  scene s = scene_new(16, 10);
  /* a 7 x 5 block of water, one marker per cell, with holes at (4, 4) - all neighbours wet -, at (7, 4) - its right neighbour (8, 4) solid: a hole -, and an
   * empty cell at the block's edge (2, 3), whose left neighbours are dry: no hole */
  for (int y = 3; y <= 7; ++y)
    for (int x = 2; x <= 8; ++x) s.prev[(size_t)y * 16 + x] = 1;
  s.solid[4 * 16 + 8] = 1;
  for (int y = 3; y <= 7; ++y)
    for (int x = 2; x <= 8; ++x)
      if (!((x == 4 && y == 4) || (x == 7 && y == 4) || (x == 2 && y == 3) || (x == 8 && y == 4))) put(&s, (float)x + 0.5f, (float)y + 0.5f);
  rebin(&s, 0);
  euler_reseed r = rec(0, 1, 0, 1);
  euler_reseed_stats st;
  memset(&st, 0, sizeof st);
  const uint64_t n0 = s.n;
  uint64_t rng = s.rng;
  CHECK(run(&s, &r, &st) == EULER_OK);      /* max_fill = 1: (4, 4) fills, (7, 4) is deferred */
  CHECK(st.added == 1 && st.deferred == 1 && s.n == n0 + 1 && s.count[4 * 16 + 4] == 1 && s.count[4 * 16 + 7] == 0 && s.count[3 * 16 + 2] == 0);
  const float ry = euler_rng_next_float(&rng), rx = euler_rng_next_float(&rng);      /* y first */
  CHECK(s.m[2 * n0] == 4.f + rx && s.m[2 * n0 + 1] == 4.f + ry && s.rng == rng);
  CHECK(run(&s, &r, &st) == EULER_OK);
  CHECK(st.added == 2 && st.deferred == 1 && s.count[4 * 16 + 7] == 1);
  CHECK(run(&s, &r, &st) == EULER_OK);      /* nothing left */
  CHECK(st.added == 2 && st.deferred == 1 && s.n == n0 + 2);
  /* a sink, a source and a solid cell are no holes; nor is a cell whose prev_count is 0 */
  s.count[5 * 16 + 5] = 0; s.sink[5 * 16 + 5] = 1;
  s.count[6 * 16 + 3] = 0; s.source[6 * 16 + 3] = 1;
  s.count[6 * 16 + 6] = 0; s.prev[6 * 16 + 6] = 0;
  CHECK(run(&s, &r, &st) == EULER_OK);
  CHECK(st.added == 2);
  scene_free(&s);
  /* the capacity: n = max_markers - 2 and three holes: one fills */
  s = scene_new(8, 8);
  for (size_t c = 0; c < s.C; ++c) { s.prev[c] = 1; s.count[c] = 1; s.sink[c] = 0; }
  s.count[2 * 8 + 2] = s.count[2 * 8 + 5] = s.count[5 * 8 + 3] = 0;
  s.n = s.cap - 2;
  for (uint64_t i = 0; i < s.n; ++i) { s.m[2 * i] = 1.5f; s.m[2 * i + 1] = 1.5f; }
  r = rec(0, 1, 0, 0);
  memset(&st, 0, sizeof st);
  CHECK(run(&s, &r, &st) == EULER_OK);
  CHECK(st.added == 1 && st.deferred == 2 && s.n == s.cap - 1 && s.count[2 * 8 + 2] == 1 && s.count[2 * 8 + 5] == 0);
  CHECK(run(&s, &r, &st) == EULER_OK);
  CHECK(st.added == 1 && st.deferred == 4 && s.n == s.cap - 1);
  scene_free(&s);
}

static uint32_t lcg(uint32_t* s) { *s = *s * 1664525u + 1013904223u; return *s >> 8; }

static void check_random(void) {
  uint32_t seed = 12345u;
  for (int round = 0; round < 12; ++round) {
    const int X = 9 + (int)(lcg(&seed) % 40u), Y = 7 + (int)(lcg(&seed) % 30u);
    scene s = scene_new(X, Y);
    for (int y = 1; y < Y - 1; ++y)
      for (int x = 1; x < X - 1; ++x) {
        const uint32_t q = lcg(&seed) % 100u;
        const size_t c = (size_t)y * X + x;
        if (q < 12) s.solid[c] = 1; else if (q < 15) s.sink[c] = 1; else if (q < 18) s.source[c] = 1;
        s.prev[c] = lcg(&seed) % 4u != 0;
      }
    const uint64_t n = (uint64_t)(3 * s.C);
    for (uint64_t i = 0; i < n; ++i) {
      int x, y;
      do { x = 1 + (int)(lcg(&seed) % (uint32_t)(X - 2)); y = 1 + (int)(lcg(&seed) % (uint32_t)(Y - 2)); } while (s.solid[(size_t)y * X + x]);
      if (lcg(&seed) % 3u == 0) { x = 1 + (x % 3); y = 1 + (y % 3); if (s.solid[(size_t)y * X + x]) continue; }      /* clumps */
      put(&s, (float)x + (float)(lcg(&seed) % 64u) / 64.f, (float)y + (float)(lcg(&seed) % 64u) / 64.f);
    }
    rebin(&s, 0);
    euler_reseed r = rec(4 + (int)(lcg(&seed) % 20u), (int)(lcg(&seed) % 2u), (int)(lcg(&seed) % 5u), (int)(lcg(&seed) % 5u));
    euler_reseed_stats st;
    memset(&st, 0, sizeof st);
    const uint64_t n0 = s.n;
    CHECK(run(&s, &r, &st) == EULER_OK);
    CHECK(s.n == n0 - st.removed + st.added && s.n <= s.cap - 1);
    for (uint64_t i = 0; i < s.n; ++i) CHECK(s.m[2 * i] >= 1.f && s.m[2 * i] <= (float)(X - 1) && s.m[2 * i + 1] >= 1.f && s.m[2 * i + 1] <= (float)(Y - 1));
    scene_free(&s);
  }
  /* bad arguments */
  scene s = scene_new(8, 8);
  euler_reseed r = rec(16, 1, 0, 0);
  CHECK(eu_reseed_pass(NULL, 8, 8, s.m, &s.n, s.cap, s.count, s.prev, s.solid, s.sink, s.source, &s.rng, NULL) == EULER_EINVAL);
  CHECK(eu_reseed_pass(&r, 8, 8, NULL, &s.n, s.cap, s.count, s.prev, s.solid, s.sink, s.source, &s.rng, NULL) == EULER_EINVAL);
  CHECK(eu_reseed_pass(&r, 2, 8, s.m, &s.n, s.cap, s.count, s.prev, s.solid, s.sink, s.source, &s.rng, NULL) == EULER_EINVAL);
  r.thin_above = 2;
  CHECK(run(&s, &r, NULL) == EULER_EINVAL);
  r = rec(0, 0, 0, 0);
  CHECK(run(&s, &r, NULL) == EULER_OK && s.n == 0);
  scene_free(&s);
}

static void check_parser(void) {
  euler_reseed r;
  CHECK(parse_reseed("16", &r) == 0 && r.thin_above == 16 && r.fill_holes == 0 && r.max_cells == 0 && r.max_fill == 0);
  CHECK(parse_reseed("16:fill", &r) == 0 && r.thin_above == 16 && r.fill_holes == 1);
  CHECK(parse_reseed("0:fill", &r) == 0 && r.thin_above == 0 && r.fill_holes == 1);
  CHECK(parse_reseed("300", &r) == 0 && r.thin_above == 300);      /* the value is euler_set_reseed's to refuse */
  CHECK(parse_reseed("", &r) == -1 && parse_reseed("fill", &r) == -1 && parse_reseed("16:", &r) == -1 && parse_reseed("16:fil", &r) == -1);
  CHECK(parse_reseed("16:fill:", &r) == -1 && parse_reseed("16x", &r) == -1 && parse_reseed(":fill", &r) == -1 && parse_reseed("16 :fill", &r) == -1);
  euler_reseed_stats st = {1, 2, 3, 4};
  char line[160];
  FILE* f = tmpfile();
  if (f) {
    CHECK(print_reseed_totals(f, &st) > 0);
    rewind(f);
    CHECK(fgets(line, sizeof line, f) && !strcmp(line, "reseed removed 1 added 2 cells_thinned 3 deferred 4\n"));
    fclose(f);
  }
}

int main(void) {
  check_refusals();
  check_subcell();
  check_thinning();
  check_filling();
  check_random();
  check_parser();
  if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
  puts("clean");
  return 0;
}
