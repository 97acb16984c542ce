/*
 * sanitize_slab_observers.c — the host planning of the observer passes on row slabs (docs/observer_passes.md "On row slabs") under AddressSanitizer +
 * UndefinedBehaviorSanitizer, on the CPU, after the pattern of sanitize_gauges.c: eu_slab_clip_rows, eu_slab_plan_raster, eu_slab_plan_flat, eu_slab_plan_bytes,
 * eu_slab_plan_contributors and eu_gauge_chunks_bands (euler_amd/csrc/euler_host.c) on random and on degenerate input.  Built and run by
 * tests/test_slab_observers_host.py.  Exit code 0 = clean.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "euler_host.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static int rnd(int lo, int hi) {      /* lo ... hi inclusive */
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return lo + (int)((rng_state * 0x2545F4914F6CDD1Dull >> 33) % (uint64_t)(hi - lo + 1));
}

/* a partition of nb bands over R ranks, every rank at least one band */
static void partition(int nb, int R, int32_t* lo, int32_t* hi) {
  int extra[EU_SLAB_PLAN_MAXR + 1], cuts[EU_SLAB_PLAN_MAXR + 1];
  for (int r = 1; r < R; ++r) extra[r] = rnd(0, nb - R);
  for (int a = 1; a < R; ++a)
    for (int b = a + 1; b < R; ++b)
      if (extra[b] < extra[a]) { const int t = extra[a]; extra[a] = extra[b]; extra[b] = t; }
  cuts[0] = 0; cuts[R] = nb;
  for (int r = 1; r < R; ++r) cuts[r] = r + extra[r];      /* ascending extras + r: strictly ascending cuts inside (0, nb) */
  for (int r = 0; r < R; ++r) { lo[r] = cuts[r]; hi[r] = cuts[r + 1]; }
}

static int raster_case(int Y, int R, const int32_t* lo, const int32_t* hi, int y0, int y1, int W, int H) {
  eu_slab_plan P;
  CHECK(eu_slab_plan_raster(&P, R, lo, hi, Y, y0, y1, W, H) == EULER_OK);
  const int Bh = y1 - y0 + 1;
  /* every row of the box in exactly one rank's clipped range */
  int* owner = malloc((size_t)Bh * sizeof *owner);
  CHECK(owner);
  for (int k = 0; k < Bh; ++k) owner[k] = -1;
  int64_t at = 0;
  for (int r = 0; r < R; ++r) {
    int32_t ya, yb;
    const int some = eu_slab_clip_rows(lo[r], hi[r], Y, y0, y1, &ya, &yb);
    CHECK(ya == P.ya[r] && yb == P.yb[r] && some == (ya <= yb));
    for (int y = ya; y <= yb; ++y) { CHECK(y >= y0 && y <= y1 && owner[y - y0] == -1); owner[y - y0] = r; }
    CHECK(P.off[r] == at && P.cnt[r] == (some ? (int64_t)(P.p_hi[r] - P.p_lo[r] + 1) * W : 0));
    if (some) CHECK(0 <= P.p_lo[r] && P.p_lo[r] <= P.p_hi[r] && P.p_hi[r] < H);
    at += P.cnt[r];
  }
  CHECK(at == P.total && P.total <= (int64_t)(H + R - 1) * W);
  for (int k = 0; k < Bh; ++k) CHECK(owner[k] >= 0);
  /* the contributors of every pixel row: the owners of its rows, consecutive */
  for (int py = 0; py < H; ++py) {
    const int ytop = y1 - (int)((int64_t)py * Bh / H), ybot = y1 + 1 - (int)((int64_t)(py + 1) * Bh / H);
    int32_t first, last;
    CHECK(eu_slab_plan_contributors(&P, py, &first, &last) == EULER_OK);
    CHECK(first == owner[ybot - y0] && last == owner[ytop - y0]);      /* rows ascend with the rank */
    for (int y = ybot; y <= ytop; ++y) CHECK(owner[y - y0] >= first && owner[y - y0] <= last);
    for (int r = first; r <= last; ++r) CHECK(P.p_lo[r] <= py && py <= P.p_hi[r]);
  }
  int32_t f, l;
  CHECK(eu_slab_plan_contributors(&P, -1, &f, &l) == EULER_EINVAL && eu_slab_plan_contributors(&P, H, &f, &l) == EULER_EINVAL);
  int64_t off[EU_SLAB_PLAN_MAXR], cnt[EU_SLAB_PLAN_MAXR];
  eu_slab_plan_bytes(&P, 88, off, cnt);
  for (int r = 0; r < R; ++r) CHECK(off[r] == 88 * P.off[r] && cnt[r] == 88 * P.cnt[r]);
  free(owner);
  return 0;
}

/* the chunk tables of the ranks: in rank order, the whole-grid table */
static int chunks_case(const euler_gauge* g, int n, int R, const int32_t* lo, const int32_t* hi) {
  const size_t m = eu_gauge_chunks(g, n, NULL);
  eu_gauge_chunk* whole = malloc((m ? m : 1) * sizeof *whole);
  CHECK(whole && eu_gauge_chunks(g, n, whole) == m);
  unsigned char* seen = calloc(m ? m : 1, 1);
  CHECK(seen);
  size_t sum = 0;
  for (int r = 0; r < R; ++r) {
    const size_t mr = eu_gauge_chunks_bands(g, n, lo[r], hi[r], NULL);
    eu_gauge_chunk* c = malloc((mr ? mr : 1) * sizeof *c);      /* exactly the count: one chunk too many is a heap overflow the sanitizer reports */
    CHECK(c && eu_gauge_chunks_bands(g, n, lo[r], hi[r], c) == mr);
    size_t w = 0;
    for (size_t k = 0; k < mr; ++k) {
      CHECK((c[k].y0 >> 6) >= lo[r] && (c[k].y1 >> 6) < hi[r]);
      while (w < m && memcmp(whole + w, c + k, sizeof *c) != 0) ++w;      /* in the whole table's order */
      CHECK(w < m && !seen[w]);
      seen[w++] = 1;
    }
    sum += mr;
    free(c);
  }
  CHECK(sum == m);
  free(seen); free(whole);
  return 0;
}

int main(void) {
  int32_t lo[EU_SLAB_PLAN_MAXR + 1], hi[EU_SLAB_PLAN_MAXR + 1];
  eu_slab_plan P;
  /* ---- degenerate input: refused, nothing read or written out of bounds */
  lo[0] = 0; hi[0] = 4;
  CHECK(eu_slab_plan_raster(NULL, 1, lo, hi, 256, 1, 254, 4, 4) == EULER_EINVAL);
  CHECK(eu_slab_plan_raster(&P, 0, lo, hi, 256, 1, 254, 4, 4) == EULER_EINVAL && eu_slab_plan_raster(&P, EU_SLAB_PLAN_MAXR + 1, lo, hi, 256, 1, 254, 4, 4) == EULER_EINVAL);
  CHECK(eu_slab_plan_raster(&P, 1, NULL, hi, 256, 1, 254, 4, 4) == EULER_EINVAL && eu_slab_plan_raster(&P, 1, lo, NULL, 256, 1, 254, 4, 4) == EULER_EINVAL);
  CHECK(eu_slab_plan_raster(&P, 1, lo, hi, 256, 5, 4, 1, 1) == EULER_EINVAL && eu_slab_plan_raster(&P, 1, lo, hi, 256, 1, 256, 1, 1) == EULER_EINVAL);
  CHECK(eu_slab_plan_raster(&P, 1, lo, hi, 256, 1, 10, 0, 1) == EULER_EINVAL && eu_slab_plan_raster(&P, 1, lo, hi, 256, 1, 10, 1, 0) == EULER_EINVAL);
  CHECK(eu_slab_plan_raster(&P, 1, lo, hi, 256, 1, 10, 1, 11) == EULER_EINVAL && eu_slab_plan_raster(&P, 1, lo, hi, 256, -1, 10, 1, 1) == EULER_EINVAL);
  lo[1] = 3; hi[1] = 5;      /* overlapping, and beyond the grid */
  CHECK(eu_slab_plan_raster(&P, 2, lo, hi, 256, 1, 254, 4, 4) == EULER_EINVAL);
  lo[1] = 4; hi[1] = 5;
  CHECK(eu_slab_plan_raster(&P, 2, lo, hi, 256, 1, 254, 4, 4) == EULER_EINVAL);
  CHECK(eu_slab_plan_flat(NULL, 1, 1) == EULER_EINVAL && eu_slab_plan_flat(&P, 0, 1) == EULER_EINVAL && eu_slab_plan_flat(&P, EU_SLAB_PLAN_MAXR + 1, 1) == EULER_EINVAL && eu_slab_plan_flat(&P, 2, 0) == EULER_EINVAL);
  int32_t ya, yb;
  CHECK(eu_slab_clip_rows(0, 1, 200, 64, 70, &ya, &yb) == 0 && ya > yb);
  CHECK(eu_slab_clip_rows(3, 4, 200, 1, 198, &ya, &yb) == 1 && ya == 192 && yb == 198);      /* the last band: 8 rows */
  CHECK(eu_slab_clip_rows(0, 1 << 25, 2147483647, 1, 2147483645, &ya, &yb) == 1 && ya == 1 && yb == 2147483645);      /* no overflow at the largest grid */
  /* ---- the flat plan: every rank a whole copy */
  for (int R = 1; R <= EU_SLAB_PLAN_MAXR; ++R) {
    CHECK(eu_slab_plan_flat(&P, R, 1024) == EULER_OK && P.total == 1024 * (int64_t)R && P.H == 1 && P.W == 1024);
    for (int r = 0; r < R; ++r) CHECK(P.off[r] == 1024 * (int64_t)r && P.cnt[r] == 1024);
    int32_t f, l;
    CHECK(eu_slab_plan_contributors(&P, 0, &f, &l) == EULER_OK && f == 0 && l == R - 1);
  }
  /* ---- the cases of the GPU tests, by hand */
  {
    const int32_t l3[3] = {0, 2, 4}, h3[3] = {2, 4, 6};
    if (raster_case(330, 3, l3, h3, 1, 328, 7, 2)) return 1;       /* H = 2 on 3 ranks */
    if (raster_case(330, 3, l3, h3, 127, 128, 5, 2)) return 1;     /* two rows across a boundary */
    if (raster_case(330, 3, l3, h3, 130, 200, 3, 37)) return 1;    /* inside one rank */
    CHECK(eu_slab_plan_raster(&P, 3, l3, h3, 330, 1, 328, 7, 2) == EULER_OK && P.p_lo[1] == 0 && P.p_hi[1] == 1 && P.total == 4 * 7);      /* the middle rank holds both pixel rows */
    const int32_t lu[3] = {0, 1, 3}, hu[3] = {1, 3, 6};
    if (raster_case(330, 3, lu, hu, 63, 64, 1, 1)) return 1;       /* one pixel, two ranks */
    if (raster_case(330, 3, lu, hu, 1, 328, 1, 328)) return 1;     /* H = Bh */
  }
  /* ---- random partitions, boxes and rasters */
  for (int it = 0; it < 4000; ++it) {
    const int R = rnd(1, EU_SLAB_PLAN_MAXR), nb = rnd(R, R + 20), Y = 64 * (nb - 1) + rnd(1, 64);
    if (Y < 3) continue;
    partition(nb, R, lo, hi);
    int y0 = rnd(1, Y - 2), y1 = rnd(1, Y - 2);
    if (y0 > y1) { const int t = y0; y0 = y1; y1 = t; }
    const int Bh = y1 - y0 + 1, H = it % 3 == 0 ? Bh : rnd(1, Bh), W = rnd(1, 40);
    if (raster_case(Y, R, lo, hi, y0, y1, W, H)) return 1;
    euler_gauge g[6];
    const int X = rnd(3, 300);
    for (int k = 0; k < 6; ++k) {
      int xa = rnd(1, X - 2), xb = rnd(1, X - 2), a = rnd(1, Y - 2), b = rnd(1, Y - 2);
      if (xa > xb) { const int t = xa; xa = xb; xb = t; }
      if (a > b) { const int t = a; a = b; b = t; }
      g[k].kind = rnd(0, 3); g[k].x0 = xa; g[k].x1 = xb; g[k].y0 = a; g[k].y1 = b; g[k].reserved = 0;
    }
    if (it % 8 == 0 && chunks_case(g, 6, R, lo, hi)) return 1;
  }
  printf("clean\n");
  return 0;
}
