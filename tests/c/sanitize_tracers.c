/*
 * sanitize_tracers.c — the host code of the passive tracers (docs/tracers.md) under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU, after the
 * pattern of sanitize_forcing.c: the checks of euler_tracers_add that need no device, the lattice of a box, the painter and the pixel of a cell
 * (euler_amd/csrc/euler_host.c, euler_host.h) and the three spec parsers of `euler --tracer / --tracer-box / --emit` with the CSV line
 * (euler_amd/cli/cli_tracers.h).  Built and run by tests/test_tracers_host.py.  Exit code 0 = clean.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "euler_host.h"
#include "cli_tracers.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static int refused(const float* xy, size_t n, size_t count, int X, int Y, const char* word) {
  char why[256] = "";
  if (eu_tracers_check(xy, n, count, X, Y, why, sizeof why) != EULER_EINVAL || !strstr(why, word)) { fprintf(stderr, "expected a refusal with \"%s\", got \"%s\"\n", word, why); return 1; }
  return eu_tracers_check(xy, n, count, X, Y, NULL, 0) != EULER_EINVAL;      /* no room for the reason: the same answer */
}

/* the lattice of a box in a buffer of exactly its size (one point too many is a heap overflow the sanitizer reports) */
static int lattice_case(int x0, int y0, int x1, int y1, int K) {
  const size_t n = eu_tracer_lattice(x0, y0, x1, y1, K, NULL);
  CHECK(n == (size_t)(x1 - x0 + 1) * (size_t)(y1 - y0 + 1) * (size_t)(K * K));
  float* xy = malloc(n * 2 * sizeof *xy);
  CHECK(xy && eu_tracer_lattice(x0, y0, x1, y1, K, xy) == n);
  size_t m = 0;
  for (int x = x0; x <= x1; ++x)
    for (int y = y0; y <= y1; ++y)
      for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j, ++m) {
          CHECK(xy[2 * m] == (float)(x + (i + 0.5) / K) && xy[2 * m + 1] == (float)(y + (j + 0.5) / K));      /* exact in float32: eighths below 2^21 */
          CHECK((int)floorf(xy[2 * m]) == x && (int)floorf(xy[2 * m + 1]) == y);
        }
  CHECK(m == n);
  free(xy);
  return 0;
}

int main(void) {
  const int X = 264, Y = 136;
  /* ---- every refusal of the check, and their order */
  {
    const float ok[] = {1.f, 1.f, 262.99f, 134.99f, 100.5f, 50.25f};
    CHECK(eu_tracers_check(ok, 3, 0, X, Y, NULL, 0) == EULER_OK && eu_tracers_check(NULL, 0, 0, X, Y, NULL, 0) == EULER_OK);
    CHECK(eu_tracers_check(ok, 3, EULER_TRACERS_MAX - 3, X, Y, NULL, 0) == EULER_OK && eu_tracers_check(NULL, 0, EULER_TRACERS_MAX, X, Y, NULL, 0) == EULER_OK);
    char why[64] = "";
    CHECK(eu_tracers_check(ok, 3, 0, X, Y, why, sizeof why) == EULER_OK && why[0] == 0);
    if (refused(NULL, 1, 0, X, Y, "null")) return 1;
    if (refused(ok, 3, EULER_TRACERS_MAX - 2, X, Y, "at most")) return 1;
    if (refused(ok, 1, EULER_TRACERS_MAX, X, Y, "at most")) return 1;
    if (refused(ok, (size_t)-1, 5, X, Y, "at most")) return 1;      /* (no wrap of count + n) */
    const float wrong[][2] = {{NAN, 5.f}, {5.f, NAN}, {INFINITY, 5.f}, {5.f, -INFINITY}, {0.999f, 5.f}, {5.f, 0.5f}, {263.f, 5.f}, {5.f, 135.f}, {-3.f, 5.f}, {3e38f, 5.f}, {0.f, 0.f}};
    for (unsigned w = 0; w < sizeof wrong / sizeof *wrong; ++w)
      for (int at = 0; at < 3; ++at) {
        float bad[6];
        char word[16];
        memcpy(bad, ok, sizeof ok);
        bad[2 * at] = wrong[w][0]; bad[2 * at + 1] = wrong[w][1];
        snprintf(word, sizeof word, "tracer %d:", at);
        if (refused(bad, 3, 0, X, Y, word)) return 1;
      }
    /* the order: the null list before the count, the count before a position; the first bad index is the one named */
    const float bad2[] = {5.f, 5.f, NAN, 5.f, 0.f, 0.f};
    if (refused(NULL, 3, EULER_TRACERS_MAX, X, Y, "null")) return 1;
    if (refused(bad2, 3, EULER_TRACERS_MAX, X, Y, "at most")) return 1;
    if (refused(bad2, 3, 0, X, Y, "tracer 1:")) return 1;
    char tiny[8];      /* a reason longer than its room is cut, not overrun */
    CHECK(eu_tracers_check(bad2, 3, 0, X, Y, tiny, sizeof tiny) == EULER_EINVAL && strlen(tiny) == sizeof tiny - 1);
  }
  /* ---- the lattice: one cell, boxes touching X - 2 / Y - 2, every K */
  {
    const int ks[] = {1, 2, 4};
    for (int q = 0; q < 3; ++q) {
      if (lattice_case(1, 1, 1, 1, ks[q]) || lattice_case(X - 2, Y - 2, X - 2, Y - 2, ks[q]) || lattice_case(X - 5, 3, X - 2, 9, ks[q]) ||
          lattice_case(7, Y - 4, 12, Y - 2, ks[q]) || lattice_case(1, 1, X - 2, Y - 2, ks[q])) return 1;
      /* what the lattice of the last cell gives is what the check takes */
      float xy[32];
      const size_t n = eu_tracer_lattice(X - 2, Y - 2, X - 2, Y - 2, ks[q], xy);
      CHECK(n == (size_t)(ks[q] * ks[q]) && eu_tracers_check(xy, n, 0, X, Y, NULL, 0) == EULER_OK);
    }
    CHECK(eu_tracer_lattice(1, 1, 2, 2, 3, NULL) == 0 && eu_tracer_lattice(1, 1, 2, 2, 0, NULL) == 0 && eu_tracer_lattice(1, 1, 2, 2, 8, NULL) == 0);
    CHECK(eu_tracer_lattice(3, 1, 2, 2, 2, NULL) == 0 && eu_tracer_lattice(1, 3, 2, 2, 2, NULL) == 0);
    CHECK(lattice_case(1048570, 1048570, 1048575, 1048575, 4) == 0);      /* below 2^21: still exact */
  }
  /* ---- the pixel of a cell against the covering definition, every (B, W) with 1 <= W <= B <= 40 */
  for (int B = 1; B <= 40; ++B)
    for (int W = 1; W <= B; ++W)
      for (int c = 0; c < B; ++c) {
        int hit = -1, hits = 0;
        for (int p = 0; p < W; ++p) if ((p * B) / W <= c && c <= ((p + 1) * B) / W - 1) { hit = p; ++hits; }
        CHECK(hits == 1 && eu_tracer_pixel(c, B, W) == hit);
      }
  CHECK(eu_tracer_pixel(2147483645, 2147483646, 2147483646) == 2147483645 && eu_tracer_pixel(2147483645, 2147483646, 1) == 0);      /* (64-bit inside) */
  /* ---- the painter: water == 0, counts == 0, a null bg, the refusals */
  {
    enum { W = 3, H = 2 };
    euler_overview_px px[W * H], was[W * H];
    memset(px, 0, sizeof px);
    for (int k = 0; k < W * H; ++k) { px[k].cells = 9; px[k].water = (uint32_t)(k % 3 == 2 ? 0 : 4 + k); px[k].marks = 77; for (int c = 0; c < 3; ++c) px[k].dye[c] = 1000u + (unsigned)k; }
    memcpy(was, px, sizeof px);
    const uint32_t counts[W * H] = {2, 0, 5, 0, 1, 0};
    const float fg[3] = {1.f, 0.9f, 0.f}, bg[3] = {0.25f, 0.5f, 1.f}, odd[3] = {NAN, -3.f, 7.f};
    CHECK(euler_tracer_paint(NULL, px, W, H, fg, bg) == EULER_EINVAL && euler_tracer_paint(counts, NULL, W, H, fg, bg) == EULER_EINVAL &&
          euler_tracer_paint(counts, px, W, H, NULL, bg) == EULER_EINVAL && euler_tracer_paint(counts, px, 0, H, fg, bg) == EULER_EINVAL &&
          euler_tracer_paint(counts, px, W, 0, fg, bg) == EULER_EINVAL && memcmp(px, was, sizeof px) == 0);
    CHECK(euler_tracer_paint(counts, px, W, H, fg, NULL) == EULER_OK);
    for (int k = 0; k < W * H; ++k) {
      const int on = counts[k] > 0 && was[k].water > 0;
      CHECK(px[k].dye[0] == (on ? (uint64_t)was[k].water * 16777216u : was[k].dye[0]));
      CHECK(px[k].dye[1] == (on ? (uint64_t)was[k].water * (uint32_t)(0.9f * 16777216.f) : was[k].dye[1]));
      CHECK(px[k].dye[2] == (on ? 0u : was[k].dye[2]));
      CHECK(px[k].cells == was[k].cells && px[k].water == was[k].water && px[k].marks == was[k].marks && px[k].solid == 0 && px[k].sink == 0 && px[k].max_speed2 == 0.f);
    }
    memcpy(px, was, sizeof px);
    CHECK(euler_tracer_paint(counts, px, W, H, fg, bg) == EULER_OK);
    for (int k = 0; k < W * H; ++k) {
      if (!was[k].water) { CHECK(memcmp(px + k, was + k, sizeof *px) == 0); continue; }      /* a tracer shows only on water pixels */
      CHECK(px[k].dye[0] == (uint64_t)was[k].water * (counts[k] ? 16777216u : 4194304u) && px[k].dye[2] == (uint64_t)was[k].water * (counts[k] ? 0u : 16777216u));
    }
    CHECK(euler_tracer_paint(counts, px, W, H, odd, odd) == EULER_OK);      /* q clamps: a NaN and a negative give 0, beyond 1 gives 2^24 */
    for (int k = 0; k < W * H; ++k) if (was[k].water) CHECK(px[k].dye[0] == 0 && px[k].dye[1] == 0 && px[k].dye[2] == (uint64_t)was[k].water * 16777216u);
  }
  /* ---- the command's three spec parsers and the CSV line */
  {
    cli_seed s;
    cli_emitter e;
    CHECK(parse_tracer("3.5,7.25", &s) == 0 && s.k == 0 && s.x == 3.5f && s.y == 7.25f);
    CHECK(parse_tracer("-1,1e3", &s) == 0 && s.x == -1.f && s.y == 1000.f);      /* (the position is checked against the grid later) */
    CHECK(parse_tracer_box("10,20,30,40:2", &s) == 0 && s.k == 2 && s.box[0] == 10 && s.box[1] == 20 && s.box[2] == 30 && s.box[3] == 40);
    CHECK(parse_tracer_box("1,1,1,1:1", &s) == 0 && s.k == 1 && parse_tracer_box("-3,5,9,9:4", &s) == 0 && s.k == 4 && s.box[0] == -3);
    CHECK(parse_emit("5,6", &e) == 0 && e.x == 5.f && e.y == 6.f && e.every == 1);
    CHECK(parse_emit("5.5,6.5:3", &e) == 0 && e.x == 5.5f && e.y == 6.5f && e.every == 3 && parse_emit("5,6:1", &e) == 0 && e.every == 1);
    const char* bad_t[] = {"", ",", "1", "1,", "1,2,", "1,2x", "1;2", "a,b", "nan,0", "0,inf", "1,2:3", " ", "1e39,0"};
    const char* bad_b[] = {"", "1,2,3,4", "1,2,3,4:", "1,2,3,4:3", "1,2,3,4:0", "1,2,3,4:8", "1,2,3,4:2x", "1,2,3:2", "1,2,3,4,5:2", "a,b,c,d:2", "1.5,2,3,4:2", "1,2,3,4;2", "1,2,3,4:-1"};
    const char* bad_e[] = {"", "1", "1,", "1,2:", "1,2:0", "1,2:-4", "1,2:x", "1,2:3x", "1,2x", "1,2:3:4", "nan,1", "1,inf:2", "1;2", "1,2,3"};
    for (unsigned k = 0; k < sizeof bad_t / sizeof *bad_t; ++k) if (parse_tracer(bad_t[k], &s) == 0) { fprintf(stderr, "--tracer accepted: \"%s\"\n", bad_t[k]); return 1; }
    for (unsigned k = 0; k < sizeof bad_b / sizeof *bad_b; ++k) if (parse_tracer_box(bad_b[k], &s) == 0) { fprintf(stderr, "--tracer-box accepted: \"%s\"\n", bad_b[k]); return 1; }
    for (unsigned k = 0; k < sizeof bad_e / sizeof *bad_e; ++k) if (parse_emit(bad_e[k], &e) == 0) { fprintf(stderr, "--emit accepted: \"%s\"\n", bad_e[k]); return 1; }
    CHECK(cli_tracer_inside(1.f, 1.f, X, Y) && cli_tracer_inside(262.99f, 134.99f, X, Y) && !cli_tracer_inside(263.f, 5.f, X, Y) && !cli_tracer_inside(5.f, 135.f, X, Y) &&
          !cli_tracer_inside(0.99f, 5.f, X, Y) && !cli_tracer_inside(NAN, 5.f, X, Y));
    const euler_tracer t = {1.5f, 2.25f, 0.125f, 0.5f, 0.25f, 7u, 33u, 0u};
    char line[256], tiny[8];
    const int len = format_tracer_line(line, sizeof line, 3, 0.75, 12, &t);
    CHECK(len > 0 && (size_t)len == strlen(line) && !strcmp(line, "3,0.75,12,1.5,2.25,0.125,0.5,0.25,7,33\n"));
    CHECK(format_tracer_line(tiny, sizeof tiny, 3, 0.75, 12, &t) == len && strlen(tiny) == sizeof tiny - 1);
    CHECK(!strcmp(k_tracers_header, "frame,time,index,x,y,path,age,wet_time,substeps,flags\n"));
  }
  printf("sanitize_tracers: clean\n");
  return 0;
}
