/*
 * sanitize_gauges.c — the host code of the batched gauges (docs/gauges.md) under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU, after the
 * pattern of sanitize_host.c: the list check and the chunk-table builder of euler_gauges (euler_amd/csrc/euler_host.c), euler_gauge_derive, and the spec
 * parser and line formatter of `euler --gauge / --gauges` (euler_amd/cli/cli_gauges.h).  Built and run by tests/test_gauges_host.py.  Exit code 0 = clean.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "euler_host.h"
#include "cli_gauges.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed line %d: %s\n", __LINE__, #c); return 1; } } while (0)

/* the chunks of a list: each inside one 64 x 64 tile and inside its gauge's box, in the gauge's kind, and together every cell of every box exactly once */
static int chunks_case(const euler_gauge* g, int n, int X, int Y) {
  const char* what = NULL;
  CHECK(eu_gauge_check(g, n, X, Y, &what) == -1 && what == NULL);
  const size_t m = eu_gauge_chunks(g, n, NULL);
  eu_gauge_chunk* c = malloc((m ? m : 1) * sizeof *c);      /* exactly the count: one chunk too many is a heap overflow the sanitizer reports */
  CHECK(c && eu_gauge_chunks(g, n, c) == m);
  unsigned char* seen = calloc((size_t)X * Y, 1);
  CHECK(seen);
  size_t at = 0;
  for (int k = 0; k < n; ++k) {
    memset(seen, 0, (size_t)X * Y);
    size_t cells = 0;
    for (; at < m && c[at].gauge == k; ++at) {
      const eu_gauge_chunk* q = c + at;
      CHECK(q->kind == g[k].kind && q->x0 <= q->x1 && q->y0 <= q->y1);
      CHECK(q->x0 >= g[k].x0 && q->x1 <= g[k].x1 && q->y0 >= g[k].y0 && q->y1 <= g[k].y1);
      CHECK((q->x0 >> 6) == (q->x1 >> 6) && (q->y0 >> 6) == (q->y1 >> 6));
      for (int y = q->y0; y <= q->y1; ++y)
        for (int x = q->x0; x <= q->x1; ++x) { CHECK(!seen[(size_t)y * X + x]); seen[(size_t)y * X + x] = 1; ++cells; }
    }
    CHECK(cells == (size_t)(g[k].x1 - g[k].x0 + 1) * (size_t)(g[k].y1 - g[k].y0 + 1));
  }
  CHECK(at == m);
  free(seen); free(c);
  return 0;
}

int main(void) {
  /* ---- the list check: the first gauge refused, and why */
  {
    const int X = 264, Y = 136;
    euler_gauge g[4] = {{EULER_GAUGE_LEVEL, 1, 1, X - 2, Y - 2, 0}, {EULER_GAUGE_FLUX, 63, 63, 64, 128, 0}, {EULER_GAUGE_FORCE, 5, 5, 5, 5, 0}, {EULER_GAUGE_PRESSURE, 64, 64, 127, 127, 0}};
    if (chunks_case(g, 4, X, Y)) return 1;
    CHECK(eu_gauge_chunks(g, 4, NULL) == 5 * 3 + 2 * 3 + 1 + 1);
    const char* what = NULL;
    euler_gauge bad[3];
    const euler_gauge wrong[] = {{4, 1, 1, 2, 2, 0}, {-1, 1, 1, 2, 2, 0}, {0, 1, 1, 2, 2, 7}, {0, 0, 1, 2, 2, 0}, {0, 1, 0, 2, 2, 0}, {0, 1, 1, X - 1, 2, 0}, {0, 1, 1, 2, Y - 1, 0}, {0, 3, 1, 2, 2, 0}, {0, 1, 3, 2, 2, 0}};
    for (unsigned w = 0; w < sizeof wrong / sizeof *wrong; ++w)
      for (int at = 0; at < 3; ++at) {
        for (int k = 0; k < 3; ++k) bad[k] = g[k];
        bad[at] = wrong[w];
        what = NULL;
        CHECK(eu_gauge_check(bad, 3, X, Y, &what) == at && what && strlen(what) > 0);
        CHECK(eu_gauge_check(bad, 3, X, Y, NULL) == at);
      }
    CHECK(eu_gauge_check(g, 0, X, Y, &what) == -1);
  }
  /* ---- the chunk table: random lists on grids whose sides are and are not multiples of the tile */
  {
    const int sizes[][2] = {{8, 8}, {66, 65}, {128, 64}, {129, 193}, {1031, 70}};
    uint64_t rng = EULER_RNG_SEED;
    for (unsigned s = 0; s < sizeof sizes / sizeof *sizes; ++s) {
      const int X = sizes[s][0], Y = sizes[s][1];
      euler_gauge g[40];
      for (int k = 0; k < 40; ++k) {
        const int xa = 1 + (int)(euler_rng_next_u32(&rng) % (uint32_t)(X - 2)), xb = 1 + (int)(euler_rng_next_u32(&rng) % (uint32_t)(X - 2));
        const int ya = 1 + (int)(euler_rng_next_u32(&rng) % (uint32_t)(Y - 2)), yb = 1 + (int)(euler_rng_next_u32(&rng) % (uint32_t)(Y - 2));
        g[k].kind = (int32_t)(euler_rng_next_u32(&rng) % 4u); g[k].reserved = 0;
        g[k].x0 = xa < xb ? xa : xb; g[k].x1 = xa < xb ? xb : xa; g[k].y0 = ya < yb ? ya : yb; g[k].y1 = ya < yb ? yb : ya;
      }
      g[0].x0 = g[0].y0 = 1; g[0].x1 = X - 2; g[0].y1 = Y - 2;      /* the whole interior */
      g[1] = g[0];                                                  /* ... twice */
      g[2].x0 = g[2].x1 = X - 2; g[2].y0 = g[2].y1 = Y - 2;         /* the last cell */
      if (chunks_case(g, 40, X, Y)) { fprintf(stderr, "grid %d x %d\n", X, Y); return 1; }
    }
    /* the most a call takes: 1024 one-cell gauges */
    euler_gauge* many = calloc(EULER_GAUGES_MAX, sizeof *many);
    CHECK(many);
    for (int k = 0; k < EULER_GAUGES_MAX; ++k) { many[k].kind = k % 4; many[k].x0 = many[k].x1 = 1 + k % 100; many[k].y0 = many[k].y1 = 1 + k % 37; }
    if (chunks_case(many, EULER_GAUGES_MAX, 102, 40)) return 1;
    CHECK(eu_gauge_chunks(many, EULER_GAUGES_MAX, NULL) == EULER_GAUGES_MAX);
    free(many);
  }
  /* ---- euler_gauge_derive */
  {
    euler_gauge_rec r;
    euler_gauge_values v;
    memset(&r, 0, sizeof r);
    r.lo_x = r.lo_y = 0xffffffffu;
    memset(&v, 0xff, sizeof v);
    CHECK(euler_gauge_derive(&r, EULER_GAUGE_FORCE, &v) == EULER_OK && v.a == 0.0 && v.b == 0.0 && v.mean_a == 0.0 && v.depth == 0.0);      /* fluid == 0 */
    r.fluid = 3; r.lo_y = 7; r.hi_y = 9; r.lo_x = 2; r.hi_x = 2; r.terms = 4;
    r.a_pos = 1ull << 60; r.a_neg = (1ull << 60) - 512; r.b_neg = 0xffffffffffffffffull; r.b_pos = 1;
    CHECK(euler_gauge_derive(&r, EULER_GAUGE_PRESSURE, &v) == EULER_OK && v.a == 2.0 && v.mean_a == 0.5 && v.depth == 3.0 && v.b < -7.2e16);
    CHECK(euler_gauge_derive(&r, EULER_GAUGE_FLUX, &v) == EULER_OK && v.a == 512.0 / 1048576.0);
    r.terms = 0;
    CHECK(euler_gauge_derive(&r, EULER_GAUGE_LEVEL, &v) == EULER_OK && v.mean_a == 0.0);
    CHECK(euler_gauge_derive(NULL, 0, &v) == EULER_EINVAL && euler_gauge_derive(&r, 0, NULL) == EULER_EINVAL);
    CHECK(euler_gauge_derive(&r, 4, &v) == EULER_EINVAL && euler_gauge_derive(&r, -1, &v) == EULER_EINVAL);
  }
  /* ---- the command's spec parser and line formatter */
  {
    euler_gauge g;
    CHECK(parse_gauge("level:1,2,3,4", &g) == 0 && g.kind == EULER_GAUGE_LEVEL && g.x0 == 1 && g.y0 == 2 && g.x1 == 3 && g.y1 == 4 && g.reserved == 0);
    CHECK(parse_gauge("pressure:10,20,10,20", &g) == 0 && g.kind == EULER_GAUGE_PRESSURE);
    CHECK(parse_gauge("force:5,5,9,9", &g) == 0 && g.kind == EULER_GAUGE_FORCE);
    CHECK(parse_gauge("flux:-3,5,9,9", &g) == 0 && g.kind == EULER_GAUGE_FLUX && g.x0 == -3);      /* (the box is checked against the grid later) */
    const char* bad[] = {"", ":", "level", "level:", "level:1,2,3", "level:1,2,3,4,", "level:1,2,3,4x", "Level:1,2,3,4", "heat:1,2,3,4", "pressures:1,2,3,4",
                         "pressureforce:1,2,3,4", "flux 1,2,3,4", "flux:1;2;3;4", "flux:a,b,c,d", "levelxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxx:1,2,3,4", "3:1,2,3,4"};
    for (unsigned k = 0; k < sizeof bad / sizeof *bad; ++k) if (parse_gauge(bad[k], &g) == 0) { fprintf(stderr, "accepted: \"%s\"\n", bad[k]); return 1; }
    euler_gauge_rec r;
    memset(&r, 0, sizeof r);
    r.cells = 0xffffffffu; r.fluid = 0xffffffffu; r.lo_x = 0; r.hi_x = 0xfffffffeu; r.lo_y = 0; r.hi_y = 0xfffffffeu; r.terms = 0xffffffffu; r.nonfinite = 0xffffffffu;
    r.a_neg = r.b_neg = 0xffffffffffffffffull; r.max_a = 3.4028234e38f; r.max_b = 1.17549435e-38f;
    char line[512], tiny[8];
    const int len = format_gauge_line(line, sizeof line, 2147483647, MAX_GAUGES - 1, EULER_GAUGE_PRESSURE, &r);      /* the longest line there is */
    CHECK(len > 0 && (size_t)len < sizeof line && strlen(line) == (size_t)len && line[len - 1] == '\n');
    CHECK(strncmp(line, "2147483647,63,pressure,4294967295,4294967295,0,4294967294,0,4294967294,4294967295,-7.20575940e+16,-7.20575940e+16,3.40282347e+38,1.17549435e-38,4294967295", 40) == 0);
    CHECK(format_gauge_line(tiny, sizeof tiny, 1, 2, EULER_GAUGE_FLUX, &r) == format_gauge_line(NULL, 0, 1, 2, EULER_GAUGE_FLUX, &r) && strlen(tiny) == sizeof tiny - 1);
    CHECK(format_gauge_line(line, sizeof line, 0, 0, 9, &r) < 0);
    CHECK(strncmp(k_gauges_header, "frame,gauge,kind,", 17) == 0 && k_gauges_header[strlen(k_gauges_header) - 1] == '\n');
  }
  printf("sanitize_gauges: clean\n");
  return 0;
}
