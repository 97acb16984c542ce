/*
 * sanitize_mg_split.c — the host planning of the multilevel preconditioner's cycle split by rows (docs/solver_multilevel_row_slabs.md) under AddressSanitizer +
 * UndefinedBehaviorSanitizer, on the CPU, after the pattern of sanitize_slab_observers.c: eu_mg_levels, eu_mg_entry_level, eu_mg_gather_level and
 * eu_mg_split_plan_fill (euler_amd/csrc/euler_host.c) on random partitions up to MG_SPLIT_MAXR ranks, on the largest grids the mode accepts, on MG_MAXLEV levels,
 * with a segment table too short, and on input that is refused.  Built and run by tests/test_mg_split_host.py.  Exit code 0 = clean.
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
  int extra[MG_SPLIT_MAXR + 1], cuts[MG_SPLIT_MAXR + 1];
  for (int r = 1; r < R; ++r) extra[r] = rnd(0, nb - R);
  for (int a = 1; a < R; ++a)
    for (int b = a + 1; b < R; ++b)
      if (extra[b] < extra[a]) { const int t = extra[a]; extra[a] = extra[b]; extra[b] = t; }
  cuts[0] = 0; cuts[R] = nb;
  for (int r = 1; r < R; ++r) cuts[r] = r + extra[r];      /* ascending extras + r: strictly ascending cuts inside (0, nb) */
  for (int r = 0; r < R; ++r) { lo[r] = cuts[r]; hi[r] = cuts[r + 1]; }
}

/* every rank's plan of one partition at one gather level, each into a heap block of exactly the struct's size; the ranges inside the levels, the messages symmetric */
static int plan_case(int levels, const int32_t* nx, const int32_t* ny, int Lg, int R, const int32_t* lo, const int32_t* hi, int seg_cap) {
  eu_mg_split_plan* P = malloc((size_t)R * sizeof *P);
  CHECK(P);
  int32_t zone = 0;
  for (int r = 0; r < R; ++r) {
    eu_mg_split_plan* p = P + r;
    CHECK(eu_mg_split_plan_fill(p, levels, nx, ny, Lg, R, r, lo, hi, seg_cap) == EULER_OK);
    CHECK(p->Lg == Lg && p->ranks == R && p->rank == r && p->nseg >= 0 && p->nseg <= seg_cap && p->total >= 0);
    for (int l = 0; l <= Lg; ++l)
      for (int q = 0; q < R; ++q) CHECK(0 <= p->I[l][q][0] && p->I[l][q][0] < p->I[l][q][1] && p->I[l][q][1] <= ny[l] && 0 <= p->O[l][q][0] && p->O[l][q][0] <= p->O[l][q][1] && p->O[l][q][1] <= ny[l]);
    for (int l = 0; l < Lg; ++l) CHECK(0 <= p->NR[l][0] && p->NR[l][0] <= p->NX[l][0] && p->NX[l][0] < p->NX[l][1] && p->NX[l][1] <= p->NR[l][1] && p->NR[l][1] <= ny[l]);
    int32_t at = 0;
    for (int k = 0; k < p->nseg; ++k) {
      const eu_mg_seg* s = p->seg + k;
      CHECK(s->level >= 0 && s->level < Lg && s->row0 >= p->NR[s->level][0] && s->row0 < s->row1 && s->row1 <= p->NR[s->level][1] && s->off == at);
      at += (s->row1 - s->row0) * nx[s->level];
    }
    CHECK(at == p->total);
    for (int k = p->nseg; k < 4 * MG_MAXLEV; ++k) CHECK(p->seg[k].row1 == 0);      /* nothing behind the table's end */
    CHECK(p->win_rows > 0 && p->nsmall == 2 + p->win_rows * nx[Lg] && p->aslot >= 0 && (p->beyond | 1) == 1 && (p->setup_bad | 1) == 1 && (p->overflow | 1) == 1);
    if (seg_cap == 4 * MG_MAXLEV) CHECK(!p->overflow);
    zone = p->zone > zone ? p->zone : zone;
  }
  for (int r = 0; r + 1 < R; ++r)
    for (int l = 0; l < Lg; ++l) {
      CHECK(memcmp(P[r].zs[1][l], P[r + 1].zr[0][l], sizeof P[r].zs[1][l]) == 0 && P[r].zoff_s[1][l] == P[r + 1].zoff_r[0][l]);
      CHECK(memcmp(P[r + 1].zs[0][l], P[r].zr[1][l], sizeof P[r].zs[1][l]) == 0 && P[r + 1].zoff_s[0][l] == P[r].zoff_r[1][l]);
    }
  for (int r = 0; r < R; ++r) CHECK(P[r].zone >= 0 && P[r].zone <= zone);
  free(P);
  return 0;
}

static int grid_case(int X, int nb, int R, const int32_t* lo, const int32_t* hi) {
  /* arrays of exactly MG_MAXLEV entries on the heap: one level too many is an overflow the sanitizer reports */
  int32_t* nx = malloc(MG_MAXLEV * sizeof *nx);
  int32_t* ny = malloc(MG_MAXLEV * sizeof *ny);
  size_t* off = malloc(MG_MAXLEV * sizeof *off);
  CHECK(nx && ny && off);
  const int levels = eu_mg_levels(X, nb, nx, ny, off);
  CHECK(levels >= 1 && levels <= MG_MAXLEV);
  const int lC = eu_mg_entry_level(levels, nx, ny);
  CHECK(lC >= 0 && lC < levels && eu_mg_gather_level(levels, nx, ny, -1) == 0 && eu_mg_gather_level(levels, nx, ny, 0) <= lC && eu_mg_gather_level(levels, nx, ny, INT64_MAX) == lC);
  for (int Lg = 1; Lg <= lC; ++Lg) {
    if (plan_case(levels, nx, ny, Lg, R, lo, hi, 4 * MG_MAXLEV)) return 1;
    if (plan_case(levels, nx, ny, Lg, R, lo, hi, rnd(0, 3))) return 1;      /* a forced overflow of the segment table */
  }
  free(nx); free(ny); free(off);
  return 0;
}

int main(void) {
  int32_t lo[MG_SPLIT_MAXR + 1], hi[MG_SPLIT_MAXR + 1], nx[MG_MAXLEV], ny[MG_MAXLEV];
  size_t off[MG_MAXLEV];
  eu_mg_split_plan P;
  /* ---- the levels: refusals, MG_MAXLEV levels exactly, one more */
  CHECK(eu_mg_levels(0, 4, nx, ny, off) == EULER_EINVAL && eu_mg_levels(64, 0, nx, ny, off) == EULER_EINVAL && eu_mg_levels(64, 4, NULL, ny, off) == EULER_EINVAL);
  CHECK(eu_mg_levels(64, 4, nx, NULL, off) == EULER_EINVAL && eu_mg_levels(64, 4, nx, ny, NULL) == EULER_EINVAL);
  CHECK(eu_mg_levels(8 * 16384, 16384 / 8, nx, ny, off) == MG_MAXLEV && nx[MG_MAXLEV - 1] * ny[MG_MAXLEV - 1] <= MG_TOP_MAX);      /* 16384 x 16384 nodes ... 8 x 8 */
  CHECK(eu_mg_levels(8 * 32768, 32768 / 8, nx, ny, off) == EULER_EINVAL);
  CHECK(eu_mg_levels(2147483647, 1, nx, ny, off) == EULER_EINVAL && eu_mg_levels(1, 268435455, nx, ny, off) == EULER_EINVAL);      /* no overflow on the way to the refusal */
  CHECK(eu_mg_levels(1, 268435456, nx, ny, off) == EULER_EINVAL);
  /* ---- the plan: refusals, nothing read or written out of bounds */
  const int levels = eu_mg_levels(1024, 32, nx, ny, off);
  lo[0] = 0; hi[0] = 15; lo[1] = 15; hi[1] = 16; lo[2] = 16; hi[2] = 32;
  CHECK(levels == 6 && eu_mg_split_plan_fill(&P, levels, nx, ny, 2, 3, 1, lo, hi, 4 * MG_MAXLEV) == EULER_OK);
  CHECK(eu_mg_split_plan_fill(NULL, levels, nx, ny, 2, 3, 1, lo, hi, 4 * MG_MAXLEV) == EULER_EINVAL && eu_mg_split_plan_fill(&P, levels, NULL, ny, 2, 3, 1, lo, hi, 4 * MG_MAXLEV) == EULER_EINVAL);
  CHECK(eu_mg_split_plan_fill(&P, levels, nx, NULL, 2, 3, 1, lo, hi, 4 * MG_MAXLEV) == EULER_EINVAL && eu_mg_split_plan_fill(&P, levels, nx, ny, 2, 3, 1, NULL, hi, 4 * MG_MAXLEV) == EULER_EINVAL);
  CHECK(eu_mg_split_plan_fill(&P, levels, nx, ny, 2, 3, 1, lo, NULL, 4 * MG_MAXLEV) == EULER_EINVAL);
  CHECK(eu_mg_split_plan_fill(&P, levels, nx, ny, 0, 3, 1, lo, hi, 4 * MG_MAXLEV) == EULER_EINVAL && eu_mg_split_plan_fill(&P, levels, nx, ny, levels, 3, 1, lo, hi, 4 * MG_MAXLEV) == EULER_EINVAL);
  CHECK(eu_mg_split_plan_fill(&P, 1, nx, ny, 1, 3, 1, lo, hi, 4 * MG_MAXLEV) == EULER_EINVAL && eu_mg_split_plan_fill(&P, MG_MAXLEV + 1, nx, ny, 2, 3, 1, lo, hi, 4 * MG_MAXLEV) == EULER_EINVAL);
  CHECK(eu_mg_split_plan_fill(&P, levels, nx, ny, 2, 1, 0, lo, hi, 4 * MG_MAXLEV) == EULER_EINVAL && eu_mg_split_plan_fill(&P, levels, nx, ny, 2, MG_SPLIT_MAXR + 1, 0, lo, hi, 4 * MG_MAXLEV) == EULER_EINVAL);
  CHECK(eu_mg_split_plan_fill(&P, levels, nx, ny, 2, 3, -1, lo, hi, 4 * MG_MAXLEV) == EULER_EINVAL && eu_mg_split_plan_fill(&P, levels, nx, ny, 2, 3, 3, lo, hi, 4 * MG_MAXLEV) == EULER_EINVAL);
  CHECK(eu_mg_split_plan_fill(&P, levels, nx, ny, 2, 3, 1, lo, hi, -1) == EULER_EINVAL && eu_mg_split_plan_fill(&P, levels, nx, ny, 2, 3, 1, lo, hi, 4 * MG_MAXLEV + 1) == EULER_EINVAL);
  hi[2] = 33;      /* beyond the grid */
  CHECK(eu_mg_split_plan_fill(&P, levels, nx, ny, 2, 3, 1, lo, hi, 4 * MG_MAXLEV) == EULER_EINVAL);
  hi[2] = 32; lo[1] = 14;      /* overlapping */
  CHECK(eu_mg_split_plan_fill(&P, levels, nx, ny, 2, 3, 1, lo, hi, 4 * MG_MAXLEV) == EULER_EINVAL);
  lo[1] = 16;      /* an empty rank */
  CHECK(eu_mg_split_plan_fill(&P, levels, nx, ny, 2, 3, 1, lo, hi, 4 * MG_MAXLEV) == EULER_EINVAL);
  /* ---- the partitions of the GPU suite, by hand: valid, valid, refused */
  lo[1] = 15;
  int beyond = 0;      /* 1024 x 2048, 0-15,15-16,16-32 at level 3: the outer ranks reach across the one-band slab */
  for (int r = 0; r < 3; ++r) {
    CHECK(eu_mg_split_plan_fill(&P, levels, nx, ny, 3, 3, r, lo, hi, 4 * MG_MAXLEV) == EULER_OK);
    beyond |= P.beyond;
  }
  CHECK(beyond == 1);
  {
    const int32_t l3[3] = {0, 7, 8}, h3[3] = {7, 8, 16};
    const int lv = eu_mg_levels(512, 16, nx, ny, off);
    for (int Lg = 1; Lg <= 2; ++Lg)
      for (int r = 0; r < 3; ++r) CHECK(eu_mg_split_plan_fill(&P, lv, nx, ny, Lg, 3, r, l3, h3, 4 * MG_MAXLEV) == EULER_OK && !P.beyond);
    if (plan_case(lv, nx, ny, 2, 3, l3, h3, 4 * MG_MAXLEV)) return 1;
  }
  /* ---- the largest grid the mode accepts (16384^2: 4096 tiles of level 0, 4 levels behind the entry level) on 2 ... 64 ranks, slabs of one band among them */
  for (int R = 2; R <= MG_SPLIT_MAXR; R += R < 8 ? 1 : 8) {
    partition(256, R, lo, hi);
    if (grid_case(16384, 256, R, lo, hi)) return 1;
    for (int r = 0; r < R; ++r) { lo[r] = r; hi[r] = r + 1; }      /* one band each but the last */
    hi[R - 1] = 256;
    if (grid_case(16384, 256, R, lo, hi)) return 1;
  }
  /* ---- MG_MAXLEV levels: the planner takes what eu_mg_levels gives, beyond what the cycle's launches accept */
  partition(16384, MG_SPLIT_MAXR, lo, hi);
  CHECK(eu_mg_levels(8, 16384, nx, ny, off) == MG_MAXLEV);      /* one node column, 131072 node rows */
  if (grid_case(8, 16384, MG_SPLIT_MAXR, lo, hi)) return 1;
  /* ---- random grids and partitions */
  for (int it = 0; it < 1500; ++it) {
    const int R = it % 50 == 0 ? MG_SPLIT_MAXR : rnd(2, 16), nb = rnd(R, R + 40), X = rnd(1, 4200);
    partition(nb, R, lo, hi);
    if (grid_case(X, nb, R, lo, hi)) return 1;
  }
  printf("clean\n");
  return 0;
}
