/*
 * sanitize_heat.c — the host code of the temperature (docs/heat.md) under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU, after the pattern of
 * sanitize_forcing.c: the check of the record and the list of euler_set_heat with every refusal in its order, the box and value checks of euler_heat_fill /
 * euler_heat_set_field, the tile table of the heat boxes, the painter (euler_amd/csrc/euler_host.c) and the spec parsers of `euler --heat / --heat-source /
 * --heat-box / --heat-init` (euler_amd/cli/cli_heat.h).  Built and run by tests/test_heat_host.py.  Exit code 0 = clean.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "euler_host.h"
#include "cli_heat.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed line %d: %s\n", __LINE__, #c); return 1; } } while (0)

/* the table of a list: one entry per tile that a box touches, in row order, each with exactly the boxes that touch it */
static int tiles_case(const euler_heat_box* b, int n, int X, int Y) {
  euler_heat h;
  char why[320] = "";
  CHECK(euler_heat_default(&h) == EULER_OK);
  h.nboxes = n;
  CHECK(eu_heat_check(&h, b, X, Y, NULL, why, sizeof why) == EULER_OK && why[0] == 0);
  const size_t m = eu_force_tiles(b, sizeof(euler_heat_box), n, X, Y, NULL);
  CHECK(m != (size_t)-1 && (n == 0) == (m == 0));
  eu_force_tile* t = malloc((m ? m : 1) * sizeof *t);      /* exactly the count: one entry too many is a heap overflow the sanitizer reports */
  CHECK(t && eu_force_tiles(b, sizeof(euler_heat_box), n, X, Y, t) == m);
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

static int refused_live(const euler_heat* h, const euler_heat_box* b, int X, int Y, const float* live, const char* word) {
  char why[320] = "";
  if (eu_heat_check(h, b, X, Y, live, why, sizeof why) != EULER_EINVAL || !strstr(why, word)) { fprintf(stderr, "expected a refusal with \"%s\", got \"%s\"\n", word, why); return 1; }
  return eu_heat_check(h, b, X, Y, live, NULL, 0) != EULER_EINVAL;      /* no room for the reason: the same answer */
}
static int refused(const euler_heat* h, const euler_heat_box* b, int X, int Y, const char* word) { return refused_live(h, b, X, Y, NULL, word); }

int main(void) {
  const int X = 264, Y = 136;
  /* ---- the tile table */
  {
    const euler_heat_box b[] = {{60, 60, 70, 70, 1.f, EULER_HEAT_FIX},        /* across x = 63|64 and y = 63|64: four tiles */
                                {100, 120, 140, 130, 2.f, EULER_HEAT_RATE},   /* across x = 127|128 and y = 127|128 */
                                {63, 5, 64, 5, 1.f, EULER_HEAT_RATE}, {5, 63, 5, 64, 1.f, EULER_HEAT_FIX}, {127, 127, 128, 128, -1.f, EULER_HEAT_RATE},
                                {X - 2, Y - 2, X - 2, Y - 2, 3.f, EULER_HEAT_FIX}, {1, 1, X - 2, Y - 2, 0.5f, EULER_HEAT_RATE},      /* the last cell; the whole interior */
                                {200, 1, X - 2, 63, 1.f, EULER_HEAT_FIX}, {60, 60, 70, 70, 1.f, EULER_HEAT_FIX}};                    /* touching X - 2; a repeat */
    for (int n = 0; n <= (int)(sizeof b / sizeof *b); ++n) if (tiles_case(b, n, X, Y)) return 1;
    CHECK(eu_force_tiles(b, sizeof(euler_heat_box), 1, X, Y, NULL) == 4 && eu_force_tiles(b, sizeof(euler_heat_box), 7, X, Y, NULL) == 5 * 3);
    euler_heat_box many[EULER_HEAT_BOXES_MAX];      /* 64 boxes on one tile */
    for (int k = 0; k < EULER_HEAT_BOXES_MAX; ++k) { many[k].x0 = 64 + k % 8; many[k].x1 = 64 + k % 8 + k / 8; many[k].y0 = 64 + k / 8; many[k].y1 = 64 + 7; many[k].value = (float)k; many[k].kind = k & 1; }
    if (tiles_case(many, EULER_HEAT_BOXES_MAX, X, Y)) return 1;
    eu_force_tile one;
    CHECK(eu_force_tiles(many, sizeof(euler_heat_box), EULER_HEAT_BOXES_MAX, X, Y, &one) == 1 && one.tx == 1 && one.ty == 1 && one.boxes == 0xffffffffffffffffull);
    /* random lists on grids whose sides are and are not multiples of the tile */
    const int sizes[][2] = {{8, 8}, {66, 65}, {128, 64}, {129, 193}, {1031, 70}};
    uint64_t rng = EULER_RNG_SEED;
    for (unsigned s = 0; s < sizeof sizes / sizeof *sizes; ++s) {
      const int gx = sizes[s][0], gy = sizes[s][1];
      for (int k = 0; k < EULER_HEAT_BOXES_MAX; ++k) {
        const int xa = 1 + (int)(euler_rng_next_u32(&rng) % (uint32_t)(gx - 2)), xb = 1 + (int)(euler_rng_next_u32(&rng) % (uint32_t)(gx - 2));
        const int ya = 1 + (int)(euler_rng_next_u32(&rng) % (uint32_t)(gy - 2)), yb = 1 + (int)(euler_rng_next_u32(&rng) % (uint32_t)(gy - 2));
        many[k].x0 = xa < xb ? xa : xb; many[k].x1 = xa < xb ? xb : xa; many[k].y0 = ya < yb ? ya : yb; many[k].y1 = ya < yb ? yb : ya;
      }
      many[3].x0 = many[3].x1 = gx - 2; many[3].y0 = many[3].y1 = gy - 2;
      if (tiles_case(many, EULER_HEAT_BOXES_MAX, gx, gy) || tiles_case(many, 17, gx, gy)) { fprintf(stderr, "grid %d x %d\n", gx, gy); return 1; }
    }
  }
  /* ---- every refusal of the check, and their order */
  {
    euler_heat d, h;
    euler_heat_box ok[2] = {{1, 1, 2, 2, 1.f, EULER_HEAT_FIX}, {3, 3, X - 2, Y - 2, -1.f, EULER_HEAT_RATE}}, bad[2];
    CHECK(euler_heat_default(&d) == EULER_OK && d.ambient == 0.f && d.beta == 0.f && d.kappa == 0.f && d.source_t == 0.f && d.nboxes == 0 && d.reserved == 0 &&
          d.reserved2 == 0.0 && euler_heat_default(NULL) == EULER_EINVAL);
    CHECK(eu_heat_check(&d, NULL, X, Y, NULL, NULL, 0) == EULER_OK);
    h = d; h.nboxes = 2; CHECK(eu_heat_check(&h, ok, X, Y, NULL, NULL, 0) == EULER_OK);
    h = d; h.reserved = 1; if (refused(&h, NULL, X, Y, "reserved")) return 1;
    h = d; h.reserved2 = 1e-300; if (refused(&h, NULL, X, Y, "reserved")) return 1;
    h = d; h.reserved2 = NAN; if (refused(&h, NULL, X, Y, "reserved")) return 1;
    const float wrong[] = {NAN, INFINITY, -INFINITY, 10000.5f, -1.0001e4f, 3e38f};
    for (unsigned w = 0; w < sizeof wrong / sizeof *wrong; ++w) {
      h = d; h.ambient = wrong[w]; if (refused(&h, NULL, X, Y, "ambient")) return 1;
      h = d; h.beta = wrong[w]; if (refused(&h, NULL, X, Y, "beta")) return 1;
      h = d; h.source_t = wrong[w]; if (refused(&h, NULL, X, Y, "source_t")) return 1;
      h = d; h.kappa = wrong[w]; if (refused(&h, NULL, X, Y, "kappa")) return 1;
      for (int at = 0; at < 2; ++at) {
        char word[16];
        snprintf(word, sizeof word, "box %d: value", at);
        h = d; h.nboxes = 2; memcpy(bad, ok, sizeof ok); bad[at].value = wrong[w]; if (refused(&h, bad, X, Y, word)) return 1;
      }
    }
    h = d; h.ambient = 1e4f; h.beta = -1e4f; h.source_t = -1e4f; h.kappa = 2.5f; CHECK(eu_heat_check(&h, NULL, X, Y, NULL, NULL, 0) == EULER_OK);      /* the bounds themselves are allowed */
    h = d; h.kappa = -1e-9f; if (refused(&h, NULL, X, Y, "outside")) return 1;
    h = d; h.kappa = 2.5000002f; if (refused(&h, NULL, X, Y, "outside")) return 1;
    h = d; h.kappa = -0.f; CHECK(eu_heat_check(&h, NULL, X, Y, NULL, NULL, 0) == EULER_OK);
    /* the live ambient */
    float live = 20.f;
    h = d; h.ambient = 20.f; CHECK(eu_heat_check(&h, NULL, X, Y, &live, NULL, 0) == EULER_OK);
    h = d; h.ambient = 20.000002f; if (refused_live(&h, NULL, X, Y, &live, "live")) return 1;
    h = d; if (refused_live(&h, NULL, X, Y, &live, "live")) return 1;
    live = 0.f; h = d; h.ambient = -0.f; CHECK(eu_heat_check(&h, NULL, X, Y, &live, NULL, 0) == EULER_OK);      /* (equal as floats) */
    h = d; h.nboxes = -1; if (refused(&h, ok, X, Y, "boxes")) return 1;
    h = d; h.nboxes = EULER_HEAT_BOXES_MAX + 1; if (refused(&h, ok, X, Y, "boxes")) return 1;
    h = d; h.nboxes = 1; if (refused(&h, NULL, X, Y, "null")) return 1;
    const int kinds[] = {-1, 2, 1 << 30};
    for (unsigned w = 0; w < sizeof kinds / sizeof *kinds; ++w)
      for (int at = 0; at < 2; ++at) {
        char word[16];
        snprintf(word, sizeof word, "box %d: kind", at);
        h = d; h.nboxes = 2; memcpy(bad, ok, sizeof ok); bad[at].kind = kinds[w]; if (refused(&h, bad, X, Y, word)) return 1;
      }
    const euler_heat_box out[] = {{0, 1, 2, 2, 0, 0}, {1, 0, 2, 2, 0, 0}, {1, 1, X - 1, 2, 0, 0}, {1, 1, 2, Y - 1, 0, 0}, {3, 1, 2, 2, 0, 0}, {1, 3, 2, 2, 0, 0}, {-5, -5, -4, -4, 0, 0}};
    for (unsigned w = 0; w < sizeof out / sizeof *out; ++w) {
      for (int at = 0; at < 2; ++at) {
        char word[16];
        snprintf(word, sizeof word, "box %d: [", at);
        h = d; h.nboxes = 2; memcpy(bad, ok, sizeof ok); bad[at] = out[w]; if (refused(&h, bad, X, Y, word)) return 1;
      }
      char why[160] = "";
      CHECK(eu_heat_box_check(out[w].x0, out[w].y0, out[w].x1, out[w].y1, X, Y, why, sizeof why) == EULER_EINVAL && strstr(why, "interior"));
      CHECK(eu_heat_box_check(out[w].x0, out[w].y0, out[w].x1, out[w].y1, X, Y, NULL, 0) == EULER_EINVAL);
    }
    CHECK(eu_heat_box_check(1, 1, X - 2, Y - 2, X, Y, NULL, 0) == EULER_OK && eu_heat_box_check(X - 2, Y - 2, X - 2, Y - 2, X, Y, NULL, 0) == EULER_OK);
    CHECK(eu_heat_value_ok(1e4f) && eu_heat_value_ok(-1e4f) && eu_heat_value_ok(-0.f) && !eu_heat_value_ok(NAN) && !eu_heat_value_ok(INFINITY) && !eu_heat_value_ok(10000.5f));
    /* the order: reserved, a value, kappa's range, the live ambient, the count, the null list, then the FIRST box that fails any of its tests */
    live = 5.f;
    h = d; h.reserved = 1; h.beta = NAN; h.kappa = 3.f; h.nboxes = 99; if (refused_live(&h, NULL, X, Y, &live, "reserved")) return 1;
    h.reserved = 0; if (refused_live(&h, NULL, X, Y, &live, "beta")) return 1;
    h.beta = 0; if (refused_live(&h, NULL, X, Y, &live, "outside")) return 1;
    h.kappa = 1.f; if (refused_live(&h, NULL, X, Y, &live, "live")) return 1;
    h.ambient = 5.f; if (refused_live(&h, NULL, X, Y, &live, "boxes")) return 1;
    h.nboxes = 2; if (refused_live(&h, NULL, X, Y, &live, "null")) return 1;
    memcpy(bad, ok, sizeof ok); bad[0] = out[0]; bad[1].value = NAN; if (refused_live(&h, bad, X, Y, &live, "box 0: [")) return 1;
    bad[0] = ok[0]; bad[0].kind = 7; if (refused_live(&h, bad, X, Y, &live, "box 0: kind")) return 1;
    bad[0].kind = 0; if (refused_live(&h, bad, X, Y, &live, "box 1: value")) return 1;
    bad[1].value = 0; CHECK(eu_heat_check(&h, bad, X, Y, &live, NULL, 0) == EULER_OK);
  }
  /* ---- the painter: exactly W * H records read and written */
  {
    enum { PW = 3, PH = 2 };
    euler_heat_px* hp = calloc(PW * PH, sizeof *hp);
    euler_overview_px* px = calloc(PW * PH, sizeof *px);
    CHECK(hp && px);
    for (int k = 0; k < PW * PH; ++k) { hp[k].cells = px[k].cells = 4; hp[k].water = px[k].water = (uint32_t)k % 4; hp[k].t_pos = (uint64_t)k << 21; hp[k].t_neg = (uint64_t)(5 - k) << 20; }
    CHECK(euler_heat_paint(hp, px, PW, PH, 20.f, 1.5) == EULER_OK && px[0].dye[0] == 0 && px[5].dye[0] == (uint64_t)16777216 && px[5].dye[1] < px[5].dye[0]);
    CHECK(euler_heat_paint(NULL, px, PW, PH, 0.f, 1.0) == EULER_EINVAL && euler_heat_paint(hp, NULL, PW, PH, 0.f, 1.0) == EULER_EINVAL && euler_heat_paint(hp, px, 0, PH, 0.f, 1.0) == EULER_EINVAL);
    CHECK(euler_heat_paint(hp, px, PW, PH, 0.f, 0.0) == EULER_EINVAL && euler_heat_paint(hp, px, PW, PH, 0.f, NAN) == EULER_EINVAL && euler_heat_paint(hp, px, PW, PH, NAN, 1.0) == EULER_EINVAL);
    hp[4].water += 1; CHECK(euler_heat_paint(hp, px, PW, PH, 0.f, 1.0) == EULER_EINVAL);
    free(hp); free(px);
  }
  /* ---- the command's spec parsers */
  {
    euler_heat h;
    euler_heat_box b;
    cli_heat_init f;
    float t = 7.f;
    euler_heat_default(&h);
    CHECK(parse_heat("20:0.5", &h) == 0 && h.ambient == 20.f && h.beta == 0.5f && h.kappa == 0.f);
    CHECK(parse_heat("-3.5:-2:2.5", &h) == 0 && h.ambient == -3.5f && h.beta == -2.f && h.kappa == 2.5f && parse_heat("1e4:-1e4:0", &h) == 0);
    CHECK(parse_heat_source("-12.5", &t) == 0 && t == -12.5f && parse_heat_source("1e4", &t) == 0);
    CHECK(parse_heat_box("fix:60:10,20,30,40", &b) == 0 && b.kind == EULER_HEAT_FIX && b.value == 60.f && b.x0 == 10 && b.y0 == 20 && b.x1 == 30 && b.y1 == 40);
    CHECK(parse_heat_box("rate:-2.5:-3,5,9,9", &b) == 0 && b.kind == EULER_HEAT_RATE && b.value == -2.5f && b.x0 == -3);      /* (the box is checked against the grid later) */
    CHECK(parse_heat_init("9:1,2,3,4", &f) == 0 && f.value == 9.f && f.box[0] == 1 && f.box[1] == 2 && f.box[2] == 3 && f.box[3] == 4);
    const char* bad_h[] = {"", ":", "1", "1:", "1:2:", "1:2x", "1;2", "a:b", "nan:0", "0:inf", "1e5:0", "0:-10000.5", "1:2:3:4", "1:2:-0.1", "1:2:2.6", "1:2:nan", " ", "1,2"};
    const char* bad_s[] = {"", "x", "1x", "nan", "inf", "1e5", "-10000.5", "1:2", " "};
    const char* bad_b[] = {"", "fix", "fix:", "fix:1", "fix:1:", "fix:1:1,2,3", "fix:1:1,2,3,4,", "fix:1:1,2,3,4x", "fix:a:1,2,3,4", "hold:1:1,2,3,4", "FIX:1:1,2,3,4", "fix:nan:1,2,3,4", "rate:1e5:1,2,3,4",
                           "rate;1:1,2,3,4", "rate:1:1;2;3;4", "fix:inf:1,1,1,1", "1:1,2,3,4", "rate:1,2,3,4"};
    const char* bad_i[] = {"", "1", "1:", "1:1,2,3", "1:1,2,3,4,", "1:1,2,3,4x", "a:1,2,3,4", "nan:1,2,3,4", "1e5:1,2,3,4", "1;1,2,3,4", "fix:1:1,2,3,4", "inf:1,1,1,1"};
    for (unsigned k = 0; k < sizeof bad_h / sizeof *bad_h; ++k) if (parse_heat(bad_h[k], &h) == 0) { fprintf(stderr, "--heat accepted: \"%s\"\n", bad_h[k]); return 1; }
    for (unsigned k = 0; k < sizeof bad_s / sizeof *bad_s; ++k) if (parse_heat_source(bad_s[k], &t) == 0) { fprintf(stderr, "--heat-source accepted: \"%s\"\n", bad_s[k]); return 1; }
    for (unsigned k = 0; k < sizeof bad_b / sizeof *bad_b; ++k) if (parse_heat_box(bad_b[k], &b) == 0) { fprintf(stderr, "--heat-box accepted: \"%s\"\n", bad_b[k]); return 1; }
    for (unsigned k = 0; k < sizeof bad_i / sizeof *bad_i; ++k) if (parse_heat_init(bad_i[k], &f) == 0) { fprintf(stderr, "--heat-init accepted: \"%s\"\n", bad_i[k]); return 1; }
  }
  printf("sanitize_heat: clean\n");
  return 0;
}
