/*
 * sanitize_forcing.c — the host code of the forcing (docs/forcing.md) under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU, after the pattern of
 * sanitize_gauges.c: the check of the record and the list and the tile-table builder of euler_set_forcing (euler_amd/csrc/euler_host.c), euler_forcing_default /
 * euler_forcing_at, and the three spec parsers of `euler --gravity / --shake / --force` (euler_amd/cli/cli_forcing.h).  Built and run by
 * tests/test_forcing_host.py.  Exit code 0 = clean.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "euler_host.h"
#include "cli_forcing.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed line %d: %s\n", __LINE__, #c); return 1; } } while (0)

/* the table of a list: one entry per tile that a box touches, in row order, each with exactly the boxes that touch it */
static int tiles_case(const euler_force_box* b, int n, int X, int Y) {
  euler_forcing f;
  char why[256] = "";
  CHECK(euler_forcing_default(&f) == EULER_OK);
  f.nboxes = n;
  CHECK(eu_forcing_check(&f, b, X, Y, why, sizeof why) == EULER_OK && why[0] == 0);
  const size_t m = eu_force_tiles(b, sizeof(euler_force_box), n, X, Y, NULL);
  CHECK(m != (size_t)-1 && (n == 0) == (m == 0));
  eu_force_tile* t = malloc((m ? m : 1) * sizeof *t);      /* exactly the count: one entry too many is a heap overflow the sanitizer reports */
  CHECK(t && eu_force_tiles(b, sizeof(euler_force_box), n, X, Y, t) == m);
  const int tnx = (X + 63) / 64, tny = (Y + 63) / 64;
  size_t at = 0;
  for (int ty = 0; ty < tny; ++ty)
    for (int tx = 0; tx < tnx; ++tx) {
      uint64_t want = 0;
      for (int k = 0; k < n; ++k)
        if (b[k].x0 <= tx * 64 + 63 && b[k].x1 >= tx * 64 && b[k].y0 <= ty * 64 + 63 && b[k].y1 >= ty * 64) want |= 1ull << k;
      if (!want) continue;
      CHECK(at < m && t[at].tx == tx && t[at].ty == ty && t[at].boxes == want);
      ++at;
    }
  CHECK(at == m);
  free(t);
  return 0;
}

static int refused(const euler_forcing* f, const euler_force_box* b, int X, int Y, const char* word) {
  char why[256] = "";
  if (eu_forcing_check(f, b, X, Y, why, sizeof why) != EULER_EINVAL || !strstr(why, word)) { fprintf(stderr, "expected a refusal with \"%s\", got \"%s\"\n", word, why); return 1; }
  return eu_forcing_check(f, b, X, Y, NULL, 0) != EULER_EINVAL;      /* no room for the reason: the same answer */
}

int main(void) {
  const int X = 264, Y = 136;
  /* ---- the tile table */
  {
    const euler_force_box b[] = {{60, 60, 70, 70, 1.f, 0.f},        /* across x = 63|64 and y = 63|64: four tiles */
                                 {100, 120, 140, 130, 0.f, 2.f},    /* across x = 127|128 and y = 127|128 */
                                 {63, 5, 64, 5, 1.f, 1.f}, {5, 63, 5, 64, 1.f, 1.f}, {127, 127, 128, 128, -1.f, -1.f},
                                 {X - 2, Y - 2, X - 2, Y - 2, 3.f, 3.f}, {1, 1, X - 2, Y - 2, 0.5f, 0.5f},      /* the last cell; the whole interior */
                                 {200, 1, X - 2, 63, 1.f, 1.f}, {60, 60, 70, 70, 1.f, 0.f}};                    /* touching X - 2; a repeat */
    for (int n = 0; n <= (int)(sizeof b / sizeof *b); ++n) if (tiles_case(b, n, X, Y)) return 1;
    CHECK(eu_force_tiles(b, sizeof(euler_force_box), 1, X, Y, NULL) == 4 && eu_force_tiles(b, sizeof(euler_force_box), 7, X, Y, NULL) == 5 * 3);
    euler_force_box many[EULER_FORCE_BOXES_MAX];      /* 64 boxes on one tile */
    for (int k = 0; k < EULER_FORCE_BOXES_MAX; ++k) { many[k].x0 = 64 + k % 8; many[k].x1 = 64 + k % 8 + k / 8; many[k].y0 = 64 + k / 8; many[k].y1 = 64 + 7; many[k].fx = (float)k; many[k].fy = -1.f; }
    if (tiles_case(many, EULER_FORCE_BOXES_MAX, X, Y)) return 1;
    eu_force_tile one;
    CHECK(eu_force_tiles(many, sizeof(euler_force_box), EULER_FORCE_BOXES_MAX, X, Y, &one) == 1 && one.tx == 1 && one.ty == 1 && one.boxes == 0xffffffffffffffffull);
    /* random lists on grids whose sides are and are not multiples of the tile */
    const int sizes[][2] = {{8, 8}, {66, 65}, {128, 64}, {129, 193}, {1031, 70}};
    uint64_t rng = EULER_RNG_SEED;
    for (unsigned s = 0; s < sizeof sizes / sizeof *sizes; ++s) {
      const int gx = sizes[s][0], gy = sizes[s][1];
      for (int k = 0; k < EULER_FORCE_BOXES_MAX; ++k) {
        const int xa = 1 + (int)(euler_rng_next_u32(&rng) % (uint32_t)(gx - 2)), xb = 1 + (int)(euler_rng_next_u32(&rng) % (uint32_t)(gx - 2));
        const int ya = 1 + (int)(euler_rng_next_u32(&rng) % (uint32_t)(gy - 2)), yb = 1 + (int)(euler_rng_next_u32(&rng) % (uint32_t)(gy - 2));
        many[k].x0 = xa < xb ? xa : xb; many[k].x1 = xa < xb ? xb : xa; many[k].y0 = ya < yb ? ya : yb; many[k].y1 = ya < yb ? yb : ya;
      }
      many[3].x0 = many[3].x1 = gx - 2; many[3].y0 = many[3].y1 = gy - 2;
      if (tiles_case(many, EULER_FORCE_BOXES_MAX, gx, gy) || tiles_case(many, 17, gx, gy)) { fprintf(stderr, "grid %d x %d\n", gx, gy); return 1; }
    }
  }
  /* ---- every refusal of the check, and their order */
  {
    euler_forcing d, f;
    euler_force_box ok[2] = {{1, 1, 2, 2, 1.f, 1.f}, {3, 3, X - 2, Y - 2, -1.f, 0.f}}, bad[2];
    CHECK(euler_forcing_default(&d) == EULER_OK && d.gx == 0.f && d.gy == -10.f && d.shake_x == 0.f && d.shake_y == 0.f && d.shake_hz == 0.0 && d.shake_phase == 0.0 &&
          d.nboxes == 0 && d.reserved == 0 && d.reserved2 == 0.0 && euler_forcing_default(NULL) == EULER_EINVAL);
    CHECK(eu_forcing_check(&d, NULL, X, Y, NULL, 0) == EULER_OK);
    f = d; f.nboxes = 2; CHECK(eu_forcing_check(&f, ok, X, Y, NULL, 0) == EULER_OK);
    f = d; f.reserved = 1; if (refused(&f, NULL, X, Y, "reserved")) return 1;
    f = d; f.reserved2 = 1e-300; if (refused(&f, NULL, X, Y, "reserved")) return 1;
    f = d; f.reserved2 = NAN; if (refused(&f, NULL, X, Y, "reserved")) return 1;
    const float wrong[] = {NAN, INFINITY, -INFINITY, 10000.5f, -1.0001e4f, 3e38f};
    for (unsigned w = 0; w < sizeof wrong / sizeof *wrong; ++w) {
      f = d; f.gx = wrong[w]; if (refused(&f, NULL, X, Y, "gravity")) return 1;
      f = d; f.gy = wrong[w]; if (refused(&f, NULL, X, Y, "gravity")) return 1;
      f = d; f.shake_x = wrong[w]; if (refused(&f, NULL, X, Y, "shake")) return 1;
      f = d; f.shake_y = wrong[w]; if (refused(&f, NULL, X, Y, "shake")) return 1;
      for (int at = 0; at < 2; ++at) {
        char word[16];
        snprintf(word, sizeof word, "box %d: force", at);
        f = d; f.nboxes = 2; memcpy(bad, ok, sizeof ok); bad[at].fx = wrong[w]; if (refused(&f, bad, X, Y, word)) return 1;
        memcpy(bad, ok, sizeof ok); bad[at].fy = wrong[w]; if (refused(&f, bad, X, Y, word)) return 1;
      }
    }
    f = d; f.gx = 1e4f; f.gy = -1e4f; f.shake_x = 1e4f; f.shake_y = -1e4f; CHECK(eu_forcing_check(&f, NULL, X, Y, NULL, 0) == EULER_OK);      /* the bound itself is allowed */
    f = d; f.shake_hz = -1e-9; if (refused(&f, NULL, X, Y, "shake_hz")) return 1;
    f = d; f.shake_hz = INFINITY; if (refused(&f, NULL, X, Y, "shake_hz")) return 1;
    f = d; f.shake_hz = NAN; if (refused(&f, NULL, X, Y, "shake_hz")) return 1;
    f = d; f.shake_phase = NAN; if (refused(&f, NULL, X, Y, "shake_phase")) return 1;
    f = d; f.shake_phase = -INFINITY; if (refused(&f, NULL, X, Y, "shake_phase")) return 1;
    f = d; f.nboxes = -1; if (refused(&f, ok, X, Y, "boxes")) return 1;
    f = d; f.nboxes = EULER_FORCE_BOXES_MAX + 1; if (refused(&f, ok, X, Y, "boxes")) return 1;
    f = d; f.nboxes = 1; if (refused(&f, NULL, X, Y, "null")) return 1;
    const euler_force_box out[] = {{0, 1, 2, 2, 0, 0}, {1, 0, 2, 2, 0, 0}, {1, 1, X - 1, 2, 0, 0}, {1, 1, 2, Y - 1, 0, 0}, {3, 1, 2, 2, 0, 0}, {1, 3, 2, 2, 0, 0}, {-5, -5, -4, -4, 0, 0}};
    for (unsigned w = 0; w < sizeof out / sizeof *out; ++w)
      for (int at = 0; at < 2; ++at) {
        char word[16];
        snprintf(word, sizeof word, "box %d: [", at);
        f = d; f.nboxes = 2; memcpy(bad, ok, sizeof ok); bad[at] = out[w]; if (refused(&f, bad, X, Y, word)) return 1;
      }
    /* the order: reserved before a value, a value before shake_hz, shake_hz before the count, the count before a box's force, every force before any box's place */
    f = d; f.reserved = 1; f.gx = NAN; f.shake_hz = -1; f.nboxes = 99; if (refused(&f, NULL, X, Y, "reserved")) return 1;
    f.reserved = 0; if (refused(&f, NULL, X, Y, "gravity")) return 1;
    f.gx = 0; if (refused(&f, NULL, X, Y, "shake_hz")) return 1;
    f.shake_hz = 0; if (refused(&f, NULL, X, Y, "boxes")) return 1;
    f.nboxes = 2; memcpy(bad, ok, sizeof ok); bad[0] = out[0]; bad[1].fy = NAN; if (refused(&f, bad, X, Y, "box 1: force")) return 1;
    bad[1].fy = 0; if (refused(&f, bad, X, Y, "box 0: [")) return 1;
  }
  /* ---- euler_forcing_at */
  {
    euler_forcing f;
    float a[2] = {7.f, 7.f};
    euler_forcing_default(&f);
    CHECK(euler_forcing_at(&f, 0.0, a) == EULER_OK && a[0] == 0.f && a[1] == -10.f);
    CHECK(euler_forcing_at(&f, 1e300, a) == EULER_OK && a[0] == 0.f && a[1] == -10.f);
    CHECK(euler_forcing_at(NULL, 0.0, a) == EULER_EINVAL && euler_forcing_at(&f, 0.0, NULL) == EULER_EINVAL);
    f.gx = 3.f; f.gy = -8.f; f.shake_x = 2.f; f.shake_y = -1.f; f.shake_hz = 0.25; f.shake_phase = 0.0;
    CHECK(euler_forcing_at(&f, 1.0, a) == EULER_OK && a[0] == 5.f && a[1] == -9.f);      /* sin(pi / 2) = 1 exactly in double */
    CHECK(euler_forcing_at(&f, 0.0, a) == EULER_OK && a[0] == 3.f && a[1] == -8.f);
    f.shake_hz = 1e300; f.shake_phase = -1e300;
    CHECK(euler_forcing_at(&f, 1e300, a) == EULER_OK && a[0] != a[0]);      /* an overflowing argument: NaN out, no trap */
    CHECK(euler_forcing_at(&f, 1.0, a) == EULER_OK && fabsf(a[0] - 3.f) <= 2.f && fabsf(a[1] + 8.f) <= 1.f);
  }
  /* ---- the command's three spec parsers */
  {
    euler_forcing f;
    euler_force_box b;
    euler_forcing_default(&f);
    CHECK(parse_gravity("3,-7.5", &f) == 0 && f.gx == 3.f && f.gy == -7.5f);
    CHECK(parse_gravity("0,0", &f) == 0 && f.gx == 0.f && f.gy == 0.f && parse_gravity("-1e4,1e4", &f) == 0);
    CHECK(parse_shake("1,2:0.5", &f) == 0 && f.shake_x == 1.f && f.shake_y == 2.f && f.shake_hz == 0.5 && f.shake_phase == 0.0);
    CHECK(parse_shake("0.5,0:2:90", &f) == 0 && f.shake_x == 0.5f && f.shake_y == 0.f && f.shake_hz == 2.0 && f.shake_phase == 90.0 * CLI_DEG_TO_RAD);
    CHECK(parse_shake("1,1:0:-720", &f) == 0 && f.shake_hz == 0.0);
    CHECK(parse_force("2.5,-1:10,20,30,40", &b) == 0 && b.fx == 2.5f && b.fy == -1.f && b.x0 == 10 && b.y0 == 20 && b.x1 == 30 && b.y1 == 40);
    CHECK(parse_force("0,0:-3,5,9,9", &b) == 0 && b.x0 == -3);      /* (the box is checked against the grid later) */
    const char* bad_g[] = {"", ",", "1", "1,", "1,2,", "1,2x", "1;2", "a,b", "nan,0", "0,inf", "1e5,0", "0,-10000.5", "1,2:3", " "};
    const char* bad_s[] = {"", "1,2", "1,2:", "1,2:x", "1,2:0.5:", "1,2:0.5:90:", "1,2:0.5:90x", "1,2:0.5x", "1,2:-0.5", "1,2:nan", "1,2:inf", "1,2:1:nan", "1,2:1:inf", "1e5,0:1", "nan,0:1", "1:2:3", "1,2,3:4"};
    const char* bad_f[] = {"", "1,2", "1,2:", "1,2:1,2,3", "1,2:1,2,3,4,", "1,2:1,2,3,4x", "1,2:a,b,c,d", "1:1,2,3,4", "nan,0:1,2,3,4", "0,1e5:1,2,3,4", "1,2;1,2,3,4", "1,2:1;2;3;4", "inf,0:1,1,1,1"};
    for (unsigned k = 0; k < sizeof bad_g / sizeof *bad_g; ++k) if (parse_gravity(bad_g[k], &f) == 0) { fprintf(stderr, "--gravity accepted: \"%s\"\n", bad_g[k]); return 1; }
    for (unsigned k = 0; k < sizeof bad_s / sizeof *bad_s; ++k) if (parse_shake(bad_s[k], &f) == 0) { fprintf(stderr, "--shake accepted: \"%s\"\n", bad_s[k]); return 1; }
    for (unsigned k = 0; k < sizeof bad_f / sizeof *bad_f; ++k) if (parse_force(bad_f[k], &b) == 0) { fprintf(stderr, "--force accepted: \"%s\"\n", bad_f[k]); return 1; }
  }
  printf("sanitize_forcing: clean\n");
  return 0;
}
