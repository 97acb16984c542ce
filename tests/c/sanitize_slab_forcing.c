/*
 * sanitize_slab_forcing.c — the host code that forcing and temperature add for row slabs (docs/forcing.md, docs/heat.md "On row slabs") under AddressSanitizer +
 * UndefinedBehaviorSanitizer, on the CPU, after the pattern of sanitize_forcing.c: the band-filtered tile table (eu_force_tiles_bands) and the digests the ranks
 * compare (eu_forcing_digest, eu_heat_digest; euler_amd/csrc/euler_host.c); and the handle's memory ledger (eu_mem.h) through what euler_set_heat reserves on a slab
 * handle - two halves of the rank's window and the box buffer, grown the way eu_devbuf_reserve grows a buffer - with every allocation failing in turn, up to
 * euler_destroy's eu_mem_free_all: the count reads 0 and every block went back once.  Built and run by tests/test_slab_forcing_host.py.  Exit code 0 = clean.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "euler_host.h"
#include "eu_mem.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed line %d: %s\n", __LINE__, #c); return 1; } } while (0)

/* a host allocator that counts, and fails its fail_at-th allocation (-1: never) */
typedef struct Host { int allocs, frees, fail_at; } Host;
static void* host_alloc(void* ctx, size_t bytes) {
  Host* h = ctx;
  if (h->allocs == h->fail_at) { h->fail_at = -1; return NULL; }      /* (once) */
  ++h->allocs;
  return malloc(bytes);
}
static void host_free(void* ctx, void* p) { ++((Host*)ctx)->frees; free(p); }
static int host_zero(void* ctx, void* p, size_t bytes) { (void)ctx; memset(p, 0, bytes); return 0; }

/* every band range [lo, hi): exactly the whole table's entries with lo <= ty < hi, in its order; the buffers hold exactly the count */
static int bands_case(const euler_force_box* b, int n, int X, int Y) {
  const int tny = (Y + 63) / 64;
  const size_t m = eu_force_tiles(b, sizeof *b, n, X, Y, NULL);
  CHECK(m != (size_t)-1);
  eu_force_tile* all = malloc((m ? m : 1) * sizeof *all);
  CHECK(all && eu_force_tiles(b, sizeof *b, n, X, Y, all) == m);
  for (int lo = 0; lo <= tny; ++lo)
    for (int hi = lo; hi <= tny; ++hi) {
      size_t want = 0;
      for (size_t k = 0; k < m; ++k) want += all[k].ty >= lo && all[k].ty < hi;
      CHECK(eu_force_tiles_bands(b, sizeof *b, n, X, Y, lo, hi, NULL) == want);
      eu_force_tile* t = malloc((want ? want : 1) * sizeof *t);      /* one entry too many is a heap overflow the sanitizer reports */
      CHECK(t && eu_force_tiles_bands(b, sizeof *b, n, X, Y, lo, hi, t) == want);
      size_t at = 0;
      for (size_t k = 0; k < m; ++k)
        if (all[k].ty >= lo && all[k].ty < hi) { CHECK(t[at].tx == all[k].tx && t[at].ty == all[k].ty && t[at].boxes == all[k].boxes); ++at; }
      CHECK(at == want);
      free(t);
    }
  /* a range beyond the grid is clipped, one in front of it too */
  CHECK(eu_force_tiles_bands(b, sizeof *b, n, X, Y, -3, tny + 5, NULL) == m && eu_force_tiles_bands(b, sizeof *b, n, X, Y, tny, tny + 5, NULL) == 0);
  free(all);
  return 0;
}

int main(void) {
  const int sizes[][2] = {{103, 150}, {200, 192}, {264, 136}, {8, 8}, {129, 193}};
  uint64_t rng = EULER_RNG_SEED;
  euler_force_box many[EULER_FORCE_BOXES_MAX];
  for (unsigned s = 0; s < sizeof sizes / sizeof *sizes; ++s) {
    const int X = sizes[s][0], Y = sizes[s][1];
    for (int k = 0; k < EULER_FORCE_BOXES_MAX; ++k) {
      const int xa = 1 + (int)(euler_rng_next_u32(&rng) % (uint32_t)(X - 2)), xb = 1 + (int)(euler_rng_next_u32(&rng) % (uint32_t)(X - 2));
      const int ya = 1 + (int)(euler_rng_next_u32(&rng) % (uint32_t)(Y - 2)), yb = 1 + (int)(euler_rng_next_u32(&rng) % (uint32_t)(Y - 2));
      many[k].x0 = xa < xb ? xa : xb; many[k].x1 = xa < xb ? xb : xa; many[k].y0 = ya < yb ? ya : yb; many[k].y1 = ya < yb ? yb : ya;
      many[k].fx = (float)k; many[k].fy = -1.f;
    }
    many[3].x0 = many[3].x1 = X - 2; many[3].y0 = many[3].y1 = Y - 2;      /* the last cell: the last band, however few rows it has */
    if (Y > 66) { many[5].y0 = 63; many[5].y1 = 64; }                     /* across rows 63|64 */
    if (Y > 130) { many[7].y0 = 127; many[7].y1 = 128; many[7].x0 = many[7].x1 = X - 2; }      /* across rows 127|128, touching X - 2 */
    many[9].x0 = 1; many[9].x1 = X - 2; many[9].y0 = Y - 3; many[9].y1 = Y - 2;               /* reaching Y - 2 inside the last band, however short */
    const int counts[] = {0, 1, 7, 17, EULER_FORCE_BOXES_MAX};
    for (unsigned c = 0; c < sizeof counts / sizeof *counts; ++c)
      if (bands_case(many, counts[c], X, Y)) { fprintf(stderr, "grid %d x %d, %d boxes\n", X, Y, counts[c]); return 1; }
  }
  /* ---- the digests: exactly nboxes boxes are read (the lists below are allocated to that size), a change anywhere changes them */
  {
    euler_forcing f;
    euler_forcing_default(&f);
    CHECK(eu_forcing_digest(&f, NULL) == eu_forcing_digest(&f, many));      /* no boxes: the list is not read */
    for (int n = 1; n <= EULER_FORCE_BOXES_MAX; n += 21) {
      euler_force_box* b = malloc((size_t)n * sizeof *b);
      CHECK(b);
      memcpy(b, many, (size_t)n * sizeof *b);
      f.nboxes = n;
      const uint64_t d = eu_forcing_digest(&f, b);
      CHECK(d == eu_forcing_digest(&f, many));      /* slots beyond nboxes do not count */
      b[n - 1].fy = 2.f;
      CHECK(d != eu_forcing_digest(&f, b));
      free(b);
    }
    f.nboxes = -1; (void)eu_forcing_digest(&f, many);      /* a count its check refuses: no box is read */
    f.nboxes = EULER_FORCE_BOXES_MAX + 1; (void)eu_forcing_digest(&f, many);
    euler_heat h;
    memset(&h, 0, sizeof h);
    euler_heat_box hb[2] = {{1, 1, 5, 5, 2.f, EULER_HEAT_FIX}, {2, 2, 6, 6, -1.f, EULER_HEAT_RATE}};
    h.nboxes = 2;
    const uint64_t d = eu_heat_digest(&h, hb);
    CHECK(d == eu_heat_digest(&h, hb) && d != eu_heat_digest(NULL, NULL) && eu_heat_digest(NULL, hb) == eu_heat_digest(NULL, NULL));
    h.kappa = 0.5f; CHECK(d != eu_heat_digest(&h, hb));
    h.nboxes = EULER_HEAT_BOXES_MAX + 1; (void)eu_heat_digest(&h, hb);
  }
  /* ---- the ledger under a slab handle's heat: per rank the window is the own rows + 1 ghost row below + 2 above, clipped to the grid */
  {
    const int grids[][2] = {{200, 192}, {103, 150}};
    const int parts[][4] = {{0, 1, 2, 3}, {0, 1, 3, 3}};      /* band cuts: three ranks of one band; two ranks, 0-1 and 1-3 */
    for (int g = 0; g < 2; ++g)
      for (int r = 0; r < 3 && parts[g][r] < parts[g][r + 1]; ++r) {
        const int X = grids[g][0], Y = grids[g][1];
        const int row_lo = 64 * parts[g][r], row_hi = 64 * parts[g][r + 1] < Y ? 64 * parts[g][r + 1] : Y;
        const int win_lo = row_lo - 1 > 0 ? row_lo - 1 : 0, win_hi = row_hi + 2 < Y ? row_hi + 2 : Y;
        const size_t heat = 2 * sizeof(float) * (size_t)X * (size_t)(win_hi - win_lo);
        const size_t head = EULER_HEAT_BOXES_MAX * sizeof(euler_heat_box);
        const size_t nt = eu_force_tiles_bands(many, sizeof *many, 17, X, Y, parts[g][r], parts[g][r + 1], NULL);
        for (int fail_at = -1; fail_at < 4; ++fail_at) {      /* -1: nothing fails; else the fail_at-th allocation does */
          Host h = {0, 0, fail_at};
          const eu_mem_ops ops = {host_alloc, host_free, host_zero, &h};
          eu_mem m;
          m.n = 0;
          void *other = NULL, *field = NULL, *box = NULL, *grown = NULL;
          int rc = eu_mem_alloc(&m, &ops, &other, 4096, EU_MEM_SLAB, EU_MEM_ZERO);      /* something the handle held before */
          const size_t before = eu_mem_counted(&m);
          if (!rc) rc = eu_mem_alloc(&m, &ops, &field, heat, EU_MEM_HANDLE, 0);
          if (!rc) CHECK(eu_mem_counted(&m) == before + heat);      /* exactly 2 * 4 * X * (window rows) */
          if (!rc) rc = eu_mem_alloc(&m, &ops, &box, head, EU_MEM_HANDLE, 0);         /* a rank no box touches: the boxes alone */
          if (!rc) {      /* ... then a list that reaches it: the buffer grows - the new block first, the old one goes behind it (eu_devbuf_reserve) */
            const size_t at = eu_mem_counted(&m);
            rc = eu_mem_alloc(&m, &ops, &grown, head + (nt + 1) * sizeof(eu_force_tile), EU_MEM_HANDLE, 0);
            if (!rc) { CHECK(eu_mem_free_one(&m, &ops, box) == EULER_OK); CHECK(eu_mem_counted(&m) == before + heat + head + (nt + 1) * sizeof(eu_force_tile)); }
            else CHECK(eu_mem_counted(&m) == at);      /* a failed growth leaves ledger and buffer as they were */
          }
          CHECK((fail_at >= 0) == (rc != 0));
          eu_mem_free_all(&m, &ops);      /* euler_destroy */
          CHECK(m.n == 0 && eu_mem_counted(&m) == 0 && h.allocs == h.frees);
        }
      }
  }
  printf("sanitize_slab_forcing: clean\n");
  return 0;
}
