/* sanitize_bodies.c - the host side of the moving bodies (docs/bodies.md) under ASan + UBSan, as a stand-alone program: eu_body_check's refusals and their
 * order, euler_body_at at the clamps and at the ties of floor(px + 0.5), the unit-shift plans and their strips, the perimeter enumeration, the --body parser.
 * Built and run by tests/test_bodies_host.py; prints "clean" when every check held. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "euler.h"
#include "euler_host.h"
#include "cli_bodies.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static euler_body make(int w, int h, double x, double y, float vx, float vy) {
  euler_body b;
  memset(&b, 0, sizeof b);
  b.w = w; b.h = h; b.x = x; b.y = y; b.vx = vx; b.vy = vy;
  return b;
}

static int refused(const euler_body* b, int n, int X, int Y, const char* word) {
  char why[256] = "";
  const int rc = eu_body_check(b, n, X, Y, why, sizeof why);
  if (rc != EULER_EINVAL || !strstr(why, word)) { fprintf(stderr, "expected a refusal with \"%s\", got %d \"%s\"\n", word, rc, why); return 0; }
  return 1;
}

static void check_refusals(void) {
  const int X = 96, Y = 64;
  euler_body good[3] = {make(4, 20, 10, 5, 3.f, 0.f), make(1, 1, 50, 30, 0.f, -2.f), make(12, 3, 30, 40, 0.f, 0.f)};
  good[2].amp_x = 1.5f; good[2].hz = 1.0;      /* 2 pi 1.5 = 9.42 <= 10 */
  char why[64];
  CHECK(eu_body_check(good, 3, X, Y, why, sizeof why) == EULER_OK);
  CHECK(eu_body_check(NULL, 0, X, Y, NULL, 0) == EULER_OK);
  /* 4: n outside [0, 16], a null list */
  CHECK(refused(good, -1, X, Y, "bodies (0"));
  CHECK(refused(good, 17, X, Y, "bodies (0"));
  CHECK(refused(NULL, 2, X, Y, "null list"));
  /* 5, per body and in this order: reserved, non-finite, size, hz < 0, speed */
  euler_body b[3];
#define RESET() memcpy(b, good, sizeof b)
  RESET(); b[1].reserved[1] = 7; b[1].x = NAN; b[1].w = 0; b[1].hz = -1; b[1].vx = 50.f; CHECK(refused(b, 3, X, Y, "body 1: reserved"));
  RESET(); b[0].reserved[0] = -1; CHECK(refused(b, 3, X, Y, "body 0: reserved"));
  RESET(); b[1].x = NAN; b[1].w = 0; b[1].hz = -1; b[1].vx = 50.f; CHECK(refused(b, 3, X, Y, "body 1: a value that is not finite"));
  {
    const double bad_d[3] = {NAN, INFINITY, -INFINITY};
    for (int k = 0; k < 3; ++k) {
      RESET(); b[2].y = bad_d[k]; CHECK(refused(b, 3, X, Y, "body 2: a value"));
      RESET(); b[2].hz = bad_d[k]; CHECK(refused(b, 3, X, Y, "body 2: a value"));
      RESET(); b[2].phase = bad_d[k]; CHECK(refused(b, 3, X, Y, "body 2: a value"));
      RESET(); b[2].vx = (float)bad_d[k]; CHECK(refused(b, 3, X, Y, "body 2: a value"));
      RESET(); b[2].vy = (float)bad_d[k]; CHECK(refused(b, 3, X, Y, "body 2: a value"));
      RESET(); b[2].amp_x = (float)bad_d[k]; CHECK(refused(b, 3, X, Y, "body 2: a value"));
      RESET(); b[2].amp_y = (float)bad_d[k]; CHECK(refused(b, 3, X, Y, "body 2: a value"));
    }
  }
  RESET(); b[1].w = 0; b[1].hz = -1; b[1].vx = 50.f; CHECK(refused(b, 3, X, Y, "body 1: 0 x 1"));
  RESET(); b[0].h = -3; CHECK(refused(b, 3, X, Y, "body 0:"));
  RESET(); b[0].w = X - 3; CHECK(refused(b, 3, X, Y, "body 0:"));
  RESET(); b[0].h = Y - 3; CHECK(refused(b, 3, X, Y, "body 0:"));
  RESET(); b[0].w = X - 4; b[0].h = Y - 4; CHECK(eu_body_check(b, 3, X, Y, why, sizeof why) == EULER_OK);      /* the largest body fits */
  RESET(); b[1].hz = -1e-9; b[1].vx = 50.f; CHECK(refused(b, 3, X, Y, "body 1: hz"));
  RESET(); b[1].vx = 10.5f; CHECK(refused(b, 3, X, Y, "body 1: a speed"));
  RESET(); b[1].vy = -10.5f; CHECK(refused(b, 3, X, Y, "body 1: a speed"));
  RESET(); b[2].amp_x = 1.6f; CHECK(refused(b, 3, X, Y, "body 2: a speed"));      /* 2 pi 1.6 = 10.05 */
  RESET(); b[2].amp_y = -1.6f; CHECK(refused(b, 3, X, Y, "body 2: a speed"));
  RESET(); b[0].vx = 10.f; b[0].vy = -10.f; CHECK(eu_body_check(b, 3, X, Y, why, sizeof why) == EULER_OK);      /* the bound itself passes */
  /* the first bad body is the one named */
  RESET(); b[2].reserved[0] = 1; b[0].vx = 11.f; CHECK(refused(b, 3, X, Y, "body 0: a speed"));
  /* sixteen bodies pass, a short reason buffer is respected */
  euler_body many[EULER_BODIES_MAX];
  for (int k = 0; k < EULER_BODIES_MAX; ++k) many[k] = make(1 + k % 3, 1 + k % 5, 2 + 5 * k, 2 + 3 * k, 0.f, 0.f);
  CHECK(eu_body_check(many, EULER_BODIES_MAX, X, Y, why, sizeof why) == EULER_OK);
  many[15].w = 0;
  char tiny[4];
  CHECK(eu_body_check(many, EULER_BODIES_MAX, X, Y, tiny, sizeof tiny) == EULER_EINVAL && strlen(tiny) == 3);
#undef RESET
}

static void check_body_at(void) {
  const int X = 96, Y = 64;
  euler_body_state s;
  euler_body b = make(4, 20, 10.0, 5.0, 3.f, -1.f);
  CHECK(euler_body_at(NULL, 0, X, Y, &s) == EULER_EINVAL && euler_body_at(&b, 0, X, Y, NULL) == EULER_EINVAL);
  CHECK(euler_body_at(&b, 0.0, X, Y, &s) == EULER_OK && s.px == 10.0 && s.py == 5.0 && s.ox == 10 && s.oy == 5);
  CHECK(euler_body_at(&b, 2.0, X, Y, &s) == EULER_OK && s.px == 16.0 && s.py == 3.0 && s.ox == 16 && s.oy == 3);
  /* the clamps: [2, X - 2 - w] and [2, Y - 2 - h]; the rectangle stays inside [2, X - 3] x [2, Y - 3] */
  CHECK(euler_body_at(&b, 1000.0, X, Y, &s) == EULER_OK && s.px == X - 2 - 4 && s.ox == X - 6 && s.ox + 4 - 1 == X - 3 && s.py == 2.0 && s.oy == 2);
  CHECK(euler_body_at(&b, -1000.0, X, Y, &s) == EULER_OK && s.px == 2.0 && s.ox == 2 && s.py == Y - 2 - 20 && s.oy + 20 - 1 == Y - 3);
  /* ties of floor(px + 0.5): x.5 goes up, below it down; negative directions alike */
  b = make(1, 1, 10.5, 20.5, 0.f, 0.f);
  CHECK(euler_body_at(&b, 0.0, X, Y, &s) == EULER_OK && s.ox == 11 && s.oy == 21);
  b.x = nextafter(10.5, 0.0); b.y = nextafter(20.5, 100.0);
  CHECK(euler_body_at(&b, 0.0, X, Y, &s) == EULER_OK && s.ox == 10 && s.oy == 21);
  b.x = 2.0; b.y = nextafter(2.5, 0.0);
  CHECK(euler_body_at(&b, 0.0, X, Y, &s) == EULER_OK && s.ox == 2 && s.oy == 2);
  /* the largest body has one place */
  b = make(X - 4, Y - 4, 50.0, -7.0, 9.f, 9.f);
  CHECK(euler_body_at(&b, 3.0, X, Y, &s) == EULER_OK && s.ox == 2 && s.oy == 2 && s.px == 2.0 && s.py == 2.0);
  b.w = X - 3;
  CHECK(euler_body_at(&b, 0.0, X, Y, &s) == EULER_EINVAL);
  b.w = 0;
  CHECK(euler_body_at(&b, 0.0, X, Y, &s) == EULER_EINVAL);
  /* the harmonic part: a quarter period puts the body at the amplitude */
  b = make(2, 2, 40.0, 30.0, 0.f, 0.f);
  b.amp_x = 6.f; b.amp_y = -3.f; b.hz = 0.5;
  CHECK(euler_body_at(&b, 0.5, X, Y, &s) == EULER_OK && fabs(s.px - 46.0) < 1e-12 && fabs(s.py - 27.0) < 1e-12 && s.ox == 46 && s.oy == 27);
  b.phase = 3.14159265358979323846 / 2;
  CHECK(euler_body_at(&b, 0.0, X, Y, &s) == EULER_OK && s.ox == 46 && s.oy == 27);
  /* a NaN that got past the check still yields a cell of the grid */
  b.x = NAN;
  CHECK(euler_body_at(&b, 0.0, X, Y, &s) == EULER_OK && s.ox == 2);
}

static void check_plans(void) {
  eu_body_shift s[8];
  CHECK(eu_body_plan(5, 7, 5, 7, s, 8) == 0);
  CHECK(eu_body_plan(5, 7, 5, 7, NULL, 0) == 0);
  const int d[5] = {-2, -1, 0, 1, 2};
  for (int a = 0; a < 5; ++a)
    for (int c = 0; c < 5; ++c) {
      memset(s, 0x7f, sizeof s);
      const int64_t n = eu_body_plan(20, 30, 20 + d[a], 30 + d[c], s, 8);
      CHECK(n == abs(d[a]) + abs(d[c]));
      int x = 20, y = 30, seen_y = 0;
      for (int64_t k = 0; k < n; ++k) {
        CHECK((s[k].axis == 0 || s[k].axis == 1) && (s[k].dir == 1 || s[k].dir == -1));
        if (s[k].axis == 1) seen_y = 1; else CHECK(!seen_y);      /* all x shifts first */
        if (s[k].axis == 0) x += s[k].dir; else y += s[k].dir;
      }
      CHECK(x == 20 + d[a] && y == 30 + d[c]);
      CHECK(eu_body_plan(20, 30, 20 + d[a], 30 + d[c], NULL, 0) == n);      /* the count alone */
      if (n > 1) {      /* a short table is not written past */
        memset(s, 0x7f, sizeof s);
        CHECK(eu_body_plan(20, 30, 20 + d[a], 30 + d[c], s, 1) == n && s[1].axis == 0x7f7f7f7f);
      }
    }
  /* the strips of a 3 x 5 body at (10, 20) */
  int fill[4], clear[4];
  const eu_body_shift px = {0, 1}, mx = {0, -1}, py = {1, 1}, my = {1, -1};
  eu_body_strips(10, 20, 3, 5, px, fill, clear);
  CHECK(fill[0] == 13 && fill[2] == 13 && fill[1] == 20 && fill[3] == 24 && clear[0] == 10 && clear[2] == 10 && clear[1] == 20 && clear[3] == 24);
  eu_body_strips(10, 20, 3, 5, mx, fill, clear);
  CHECK(fill[0] == 9 && fill[2] == 9 && clear[0] == 12 && clear[2] == 12 && fill[1] == 20 && fill[3] == 24);
  eu_body_strips(10, 20, 3, 5, py, fill, clear);
  CHECK(fill[1] == 25 && fill[3] == 25 && fill[0] == 10 && fill[2] == 12 && clear[1] == 20 && clear[3] == 20 && clear[0] == 10 && clear[2] == 12);
  eu_body_strips(10, 20, 3, 5, my, fill, clear);
  CHECK(fill[1] == 19 && fill[3] == 19 && clear[1] == 24 && clear[3] == 24);
  /* a 1 x 1 body: the strip is a cell, the cleared strip the body itself */
  eu_body_strips(7, 8, 1, 1, px, fill, clear);
  CHECK(fill[0] == 8 && fill[1] == 8 && fill[2] == 8 && fill[3] == 8 && clear[0] == 7 && clear[1] == 8 && clear[2] == 7 && clear[3] == 8);
}

/* the faces of a rectangle, against their definition: every u face between a body cell and a cell left or right of the body, every v face likewise, each once */
static void check_perimeter_of(int ox, int oy, int w, int h, int X, int Y) {
  const int n = eu_body_nfaces(w, h);
  CHECK(n == 2 * w + 2 * h);
  unsigned char* seen = (unsigned char*)calloc((size_t)X * Y * 2, 1);
  CHECK(seen != NULL);
  if (!seen) return;
  for (int k = 0; k < n; ++k) {
    const eu_body_face f = eu_body_face_at(ox, oy, w, h, k);
    CHECK(f.axis == 0 || f.axis == 1);
    CHECK(f.fx >= 1 && f.fx <= X - 2 && f.fy >= 1 && f.fy <= Y - 2 && f.cx >= 1 && f.cx <= X - 2 && f.cy >= 1 && f.cy <= Y - 2);
    const int in_c = f.cx >= ox && f.cx < ox + w && f.cy >= oy && f.cy < oy + h;
    CHECK(!in_c);      /* the outside cell is outside */
    /* the face's two cells: (fx, fy) and its right (u) or upper (v) neighbour; one is the outside cell, the other a cell of the body */
    const int ax = f.fx + (f.axis == 0), ay = f.fy + (f.axis == 1);
    const int first_is_out = f.fx == f.cx && f.fy == f.cy, second_is_out = ax == f.cx && ay == f.cy;
    CHECK(first_is_out != second_is_out);
    const int bx = first_is_out ? ax : f.fx, by = first_is_out ? ay : f.fy;
    CHECK(bx >= ox && bx < ox + w && by >= oy && by < oy + h);
    unsigned char* cell = &seen[((size_t)f.fy * X + f.fx) * 2 + f.axis];
    CHECK(*cell == 0);      /* each face once */
    *cell = 1;
  }
  free(seen);
}

static void check_perimeters(void) {
  const int X = 96, Y = 64;
  check_perimeter_of(10, 20, 1, 1, X, Y);
  check_perimeter_of(10, 20, 1, 9, X, Y);
  check_perimeter_of(10, 20, 12, 1, X, Y);
  check_perimeter_of(10, 20, 12, 3, X, Y);
  check_perimeter_of(2, 2, 5, 4, X, Y);                      /* touching the lower clamps */
  check_perimeter_of(X - 2 - 5, Y - 2 - 4, 5, 4, X, Y);      /* ... and the upper ones */
  check_perimeter_of(2, 2, X - 4, Y - 4, X, Y);              /* the largest body */
  const eu_body_face f0 = eu_body_face_at(10, 20, 3, 5, 0), f5 = eu_body_face_at(10, 20, 3, 5, 5), f10 = eu_body_face_at(10, 20, 3, 5, 10), f13 = eu_body_face_at(10, 20, 3, 5, 13);
  CHECK(f0.axis == 0 && f0.fx == 9 && f0.fy == 20 && f0.cx == 9);
  CHECK(f5.axis == 0 && f5.fx == 12 && f5.fy == 20 && f5.cx == 13);
  CHECK(f10.axis == 1 && f10.fx == 10 && f10.fy == 19 && f10.cy == 19);
  CHECK(f13.axis == 1 && f13.fx == 10 && f13.fy == 24 && f13.cy == 25);
}

static void check_parser(void) {
  euler_body b;
  CHECK(parse_body("4,200:20,2:0,0:6,0:0.5", &b) == 0 && b.w == 4 && b.h == 200 && b.x == 20 && b.y == 2 && b.vx == 0 && b.vy == 0 && b.amp_x == 6.f && b.amp_y == 0 &&
        b.hz == 0.5 && b.phase == 0 && b.reserved[0] == 0 && b.reserved[1] == 0);
  CHECK(parse_body("2,6:4.5,3:3.5,-1", &b) == 0 && b.w == 2 && b.h == 6 && b.x == 4.5 && b.y == 3 && b.vx == 3.5f && b.vy == -1.f && b.hz == 0 && b.amp_x == 0);
  CHECK(parse_body("1,1:5,5:0,0:1,2:0.25:90", &b) == 0 && fabs(b.phase - 3.14159265358979323846 / 2) < 1e-15 && b.amp_y == 2.f);
  const char* bad[] = {"", "4", "4,200", "4,200:20", "4,200:20,2", "4,200:20,2:0", "4,200:20,2:0,0x", "4,200:20,2:0,0:", "4,200:20,2:0,0:6", "4,200:20,2:0,0:6,0",
                       "4,200:20,2:0,0:6,0:", "4,200:20,2:0,0:6,0:0.5x", "4,200:20,2:0,0:6,0:0.5:", "4,200:20,2:0,0:6,0:0.5:30x", "4,200:20,2:0,0:6,0:0.5:30:1", "x,1:2,2:0,0",
                       "4;200:20,2:0,0"};
  for (size_t k = 0; k < sizeof bad / sizeof *bad; ++k) {
    if (parse_body(bad[k], &b) != -1) { fprintf(stderr, "parse_body accepted \"%s\"\n", bad[k]); ++failures; }
  }
}

int main(void) {
  check_refusals();
  check_body_at();
  check_plans();
  check_perimeters();
  check_parser();
  if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
  puts("clean");
  return 0;
}
