/*
 * sanitize_session.c — the session file's composer, parser and settings comparison (euler_host.c: eu_session_put_chunks, eu_session_parse,
 * eu_session_settings_diff; docs/session.md) under AddressSanitizer and UBSan, without a GPU: a stand-alone program with its own main, run directly.
 * A valid 12 x 9 session is composed in memory; then every truncation of it, single-byte flips of the header, the chunk headers and the counts (with the
 * checksum left stale, and with it made right again), oversized counts, chunks out of order, a duplicate, a missing END, an unknown tag or chunk version,
 * a body over an open cell, a heat value beyond 1e4, an unflagged tracer without a position.  Each is refused with the expected code; every buffer handed in
 * has exactly the bytes of the file (the sanitizer sees a read one byte beyond it) and is compared with a copy afterwards, and a refused call leaves *out alone.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "euler_host.h"

#define GX 12
#define GY 9
#define C (GX * GY)
#define NM 5
#define NCHUNKS 9
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

static size_t g_core;
static size_t g_off[NCHUNKS + 1];      /* where each chunk begins; [NCHUNKS]: where the trailer stands */

static void seal(unsigned char* f, size_t n) {
  const uint64_t sum = eu_fnv1a64(EU_FNV_BASIS, f, n - 8);
  memcpy(f + n - 8, &sum, 8);
}

/* the parser on an exact-size copy; the copy must come back unchanged, and *out too when the call refuses */
static int parse(const unsigned char* f, size_t n, eu_session* out_or_null) {
  unsigned char* copy = (unsigned char*)malloc(n ? n : 1);
  eu_session* s = (eu_session*)malloc(sizeof *s);
  eu_session* pattern = (eu_session*)malloc(sizeof *s);
  char why[400] = "";
  CHECK(copy && s && pattern);
  if (n) memcpy(copy, f, n);
  memset(s, 0xAB, sizeof *s); memset(pattern, 0xAB, sizeof *pattern);
  const int rc = eu_session_parse(copy, n, GX, GY, 0, 4 * C, s, why, sizeof why);
  CHECK(n == 0 || memcmp(copy, f, n) == 0);
  CHECK(rc == EULER_OK || rc == EULER_EINVAL || rc == EULER_EIO);
  if (rc) { CHECK(memcmp(s, pattern, sizeof *s) == 0); CHECK(why[0] != '\0'); }
  else if (out_or_null) {
    *out_or_null = *s;      /* (its byte pointers go with the copy: turned into offsets from the file's start) */
    out_or_null->solid = f + (s->solid - copy);
    out_or_null->heat_field = s->heat_field ? f + (s->heat_field - copy) : NULL;
    out_or_null->tracers = f + (s->tracers - copy);
  }
  free(copy); free(s); free(pattern);
  return rc;
}

/* a file from the core of `f` and the given chunks of it, in the given order */
static unsigned char* reorder(const unsigned char* f, const int* order, int n_order, size_t* n_out) {
  size_t n = g_core + 8;
  for (int k = 0; k < n_order; ++k) n += g_off[order[k] + 1] - g_off[order[k]];
  unsigned char* g = (unsigned char*)malloc(n);
  CHECK(g);
  memcpy(g, f, g_core);
  size_t at = g_core;
  for (int k = 0; k < n_order; ++k) { const size_t len = g_off[order[k] + 1] - g_off[order[k]]; memcpy(g + at, f + g_off[order[k]], len); at += len; }
  seal(g, n);
  *n_out = n;
  return g;
}

int main(void) {
  /* ---- a valid session: a solid ring, a 2 x 2 body at (4, 3), five markers, heat on, three tracers (one lost), two force boxes, reseed on */
  static unsigned char solid[C];
  static float field[C];
  static euler_tracer tracers[3];
  eu_session* s = (eu_session*)calloc(1, sizeof *s);
  CHECK(s);
  for (int y = 0; y < GY; ++y) for (int x = 0; x < GX; ++x) solid[y * GX + x] = x == 0 || y == 0 || x == GX - 1 || y == GY - 1 || (x >= 4 && x <= 5 && y >= 3 && y <= 4);
  s->X = GX; s->Y = GY; s->dye = 0; s->n_markers = NM; s->rng_state = 0x1234567ull; s->frames = 6; s->total_substeps = 31; s->total_pcg_iterations = 977;
  s->time = 0.6000000052154064;
  euler_forcing_default(&s->forcing);
  s->forcing.gx = 1.5f; s->forcing.shake_x = 2.f; s->forcing.shake_hz = 0.5; s->forcing.nboxes = 2;
  s->force_boxes[0] = (euler_force_box){1, 1, 3, 2, 4.f, 0.f}; s->force_boxes[1] = (euler_force_box){7, 2, 10, 7, 0.f, -3.f};
  s->heat_on = 1;
  euler_heat_default(&s->heat);
  s->heat.beta = 0.5f; s->heat.kappa = 0.3f; s->heat.source_t = 8.f; s->heat.nboxes = 1;
  s->heat_boxes[0] = (euler_heat_box){1, 1, 2, 2, 16.f, EULER_HEAT_FIX};
  for (int i = 0; i < C; ++i) field[i] = (float)(i % 7);
  s->heat_field = (const unsigned char*)field;
  tracers[0] = (euler_tracer){2.5f, 2.5f, 1.f, 0.6f, 0.6f, 31u, EULER_TRACER_WET, 0u};
  tracers[1] = (euler_tracer){4.5f, 3.5f, 0.f, 0.f, 0.f, 0u, EULER_TRACER_RETIRED | EULER_TRACER_IN_SOLID, 0u};
  tracers[2] = (euler_tracer){NAN, 1.5f, 0.f, 0.f, 0.f, 0u, EULER_TRACER_RETIRED | EULER_TRACER_LOST, 0u};
  s->n_tracers = 3; s->tracers = (const unsigned char*)tracers;
  s->n_bodies = 1;
  s->bodies[0] = (euler_body){3.0, 3.0, 0.25, 0.0, 1.f, 0.f, 1.f, 0.f, 2, 2, {0, 0}};
  s->body_ox[0] = 4; s->body_oy[0] = 3;
  s->reseed.thin_above = 16; s->reseed.fill_holes = 1;
  s->reseed_stats = (euler_reseed_stats){5, 2, 1, 0};
  s->settings.max_iterations = 100; s->settings.dot_mode = 1; s->settings.max_substeps = 8; s->settings.pcg_poll_interval = 8; s->settings.tol = 1e-6;
  s->settings.nopts = EULER_OPT__COUNT; s->settings.opt[EULER_OPT_P_STEPS] = 8; s->settings.opt[EULER_OPT_ADVECT_RK2] = 1;
  s->last_substeps = 5; s->last_pcg_iterations = 160; s->last_residual = 3e-7; s->last_dt = 0.02f; s->marker_dt_events = 4;

  g_core = eu_session_core_bytes(GX, GY, 0, NM);
  CHECK(g_core == 72 + 29 * C + 8 * NM);
  const size_t chunk_bytes = eu_session_chunk_bytes(s), n = g_core + chunk_bytes + 8;
  unsigned char* f = (unsigned char*)calloc(1, n);
  CHECK(f);
  const uint32_t version = 4;
  const int32_t gx = GX, gy = GY;
  const uint64_t nm = NM;
  memcpy(f, "EULERSNP", 8); memcpy(f + 8, &version, 4); memcpy(f + 12, &gx, 4); memcpy(f + 16, &gy, 4); memcpy(f + 24, &nm, 8); memcpy(f + 32, &s->rng_state, 8);
  memcpy(f + 48, &s->frames, 8); memcpy(f + 56, &s->total_substeps, 8); memcpy(f + 64, &s->total_pcg_iterations, 8);
  memcpy(f + 72 + 16 * C, solid, C);
  for (int k = 0; k < NM; ++k) { const float m[2] = {1.5f + (float)k, 1.25f}; memcpy(f + 72 + 29 * C + 8 * k, m, 8); }
  CHECK(eu_session_put_chunks(s, f + g_core) == chunk_bytes);
  seal(f, n);
  {      /* the chunk table, read off the headers */
    size_t at = g_core;
    for (int k = 0; k < NCHUNKS; ++k) {
      uint64_t bytes;
      g_off[k] = at;
      memcpy(&bytes, f + at + 8, 8);
      at += 16 + (((size_t)bytes + 7) & ~(size_t)7);
    }
    g_off[NCHUNKS] = at;
    CHECK(at == n - 8);
  }

  /* ---- the valid file parses to what went in */
  eu_session* t = (eu_session*)calloc(1, sizeof *t);
  CHECK(t && parse(f, n, t) == EULER_OK);
  CHECK(t->X == GX && t->Y == GY && t->dye == 0 && t->n_markers == NM && t->rng_state == s->rng_state && t->frames == 6 && t->total_substeps == 31 && t->total_pcg_iterations == 977);
  CHECK(memcmp(&t->time, &s->time, 8) == 0 && memcmp(&t->forcing, &s->forcing, sizeof s->forcing) == 0 && memcmp(t->force_boxes, s->force_boxes, 2 * sizeof(euler_force_box)) == 0);
  CHECK(t->heat_on == 1 && memcmp(&t->heat, &s->heat, sizeof s->heat) == 0 && memcmp(t->heat_boxes, s->heat_boxes, sizeof(euler_heat_box)) == 0 && memcmp(t->heat_field, field, sizeof field) == 0);
  CHECK(t->n_tracers == 3 && memcmp(t->tracers, tracers, sizeof tracers) == 0 && memcmp(t->solid, solid, C) == 0);
  CHECK(t->n_bodies == 1 && memcmp(t->bodies, s->bodies, sizeof(euler_body)) == 0 && t->body_ox[0] == 4 && t->body_oy[0] == 3);
  CHECK(memcmp(&t->reseed, &s->reseed, sizeof s->reseed) == 0 && memcmp(&t->reseed_stats, &s->reseed_stats, sizeof s->reseed_stats) == 0);
  CHECK(memcmp(&t->settings, &s->settings, sizeof s->settings) == 0);
  CHECK(t->last_substeps == 5 && t->last_pcg_iterations == 160 && t->last_residual == 3e-7 && t->last_dt == 0.02f && t->marker_dt_events == 4 && t->marker_multi_events == 0);
  /* null arguments, another grid, the dye bit, the marker capacity */
  {
    char why[200];
    eu_session u;
    CHECK(eu_session_parse(NULL, n, GX, GY, 0, 4 * C, &u, why, sizeof why) == EULER_EINVAL && eu_session_parse(f, n, GX, GY, 0, 4 * C, NULL, why, sizeof why) == EULER_EINVAL);
    CHECK(eu_session_parse(f, n, GX + 1, GY, 0, 4 * C, &u, why, sizeof why) == EULER_EINVAL && strstr(why, "12x9"));
    CHECK(eu_session_parse(f, n, GX, GY, 1, 4 * C, &u, why, sizeof why) == EULER_EINVAL && strstr(why, "dye"));
    CHECK(eu_session_parse(f, n, GX, GY, 0, NM - 1, &u, why, sizeof why) == EULER_EINVAL && strstr(why, "capacity"));
    CHECK(eu_session_parse(f, n, GX, GY, 0, NM, &u, NULL, 0) == EULER_OK);
  }

  /* ---- every truncation */
  for (size_t m = 0; m < n; ++m) CHECK(parse(f, m, NULL) != EULER_OK);
  /* ... also with the checksum made right for the shorter file: nothing but the structure refuses it */
  for (size_t m = g_core + 8; m < n; ++m) {
    unsigned char* g = (unsigned char*)malloc(m);
    CHECK(g);
    memcpy(g, f, m);
    seal(g, m);
    CHECK(parse(g, m, NULL) == EULER_EINVAL);
    free(g);
  }

  /* ---- single-byte flips: the header, every chunk header, the counts */
  {
    static const unsigned char masks[3] = {0x01, 0x80, 0xFF};
    size_t at[72 + 16 * NCHUNKS + 64];
    int strict[72 + 16 * NCHUNKS + 64];      /* 1: refused with EULER_EINVAL even behind a right checksum */
    size_t na = 0;
    for (size_t b = 0; b < 72; ++b) { at[na] = b; strict[na++] = b < 24 || (b >= 44 && b < 48); }      /* magic, version, GX, GY, the reserved words; (n_markers: refused one way or the other; the rest is state) */
    for (int k = 0; k < NCHUNKS; ++k) for (size_t b = 0; b < 16; ++b) { at[na] = g_off[k] + b; strict[na++] = 1; }
    for (size_t b = 0; b < 4; ++b) { at[na] = g_off[1] + 16 + 32 + b; strict[na++] = 1; }      /* FORC nboxes */
    for (size_t b = 0; b < 8; ++b) { at[na] = g_off[2] + 16 + b; strict[na++] = 1; }           /* HEAT on, pad */
    for (size_t b = 0; b < 4; ++b) { at[na] = g_off[2] + 16 + 8 + 16 + b; strict[na++] = 1; }  /* HEAT nboxes */
    for (size_t b = 0; b < 8; ++b) { at[na] = g_off[3] + 16 + b; strict[na++] = 1; }           /* TRAC n */
    for (size_t b = 0; b < 8; ++b) { at[na] = g_off[4] + 16 + b; strict[na++] = 1; }           /* BODY n, pad */
    unsigned char* g = (unsigned char*)malloc(n);
    CHECK(g);
    for (size_t k = 0; k < na; ++k)
      for (int m = 0; m < 3; ++m) {
        memcpy(g, f, n);
        g[at[k]] ^= masks[m];
        CHECK(parse(g, n, NULL) != EULER_OK);      /* the stale checksum, or an earlier test */
        seal(g, n);
        const int rc = parse(g, n, NULL);
        if (strict[k]) CHECK(rc == EULER_EINVAL);
        else if (at[k] >= 24 && at[k] < 32) CHECK(rc != EULER_OK);
        else CHECK(rc == EULER_OK);
      }
    /* the trailer itself */
    for (size_t b = n - 8; b < n; ++b) { memcpy(g, f, n); g[b] ^= 0x10; CHECK(parse(g, n, NULL) == EULER_EIO); }
    /* oversized counts behind a right checksum */
    const uint64_t many = 1ull << 40;
    const int32_t boxes65 = 65, bodies17 = 17, minus = -1;
    memcpy(g, f, n); memcpy(g + g_off[3] + 16, &many, 8); seal(g, n); CHECK(parse(g, n, NULL) == EULER_EINVAL);
    memcpy(g, f, n); memcpy(g + g_off[1] + 16 + 32, &boxes65, 4); seal(g, n); CHECK(parse(g, n, NULL) == EULER_EINVAL);
    memcpy(g, f, n); memcpy(g + g_off[1] + 16 + 32, &minus, 4); seal(g, n); CHECK(parse(g, n, NULL) == EULER_EINVAL);
    memcpy(g, f, n); memcpy(g + g_off[2] + 16 + 8 + 16, &boxes65, 4); seal(g, n); CHECK(parse(g, n, NULL) == EULER_EINVAL);
    memcpy(g, f, n); memcpy(g + g_off[4] + 16, &bodies17, 4); seal(g, n); CHECK(parse(g, n, NULL) == EULER_EINVAL);
    memcpy(g, f, n); memcpy(g + g_off[4] + 16, &minus, 4); seal(g, n); CHECK(parse(g, n, NULL) == EULER_EINVAL);
    memcpy(g, f, n); memcpy(g + g_off[0] + 8, &many, 8); seal(g, n); CHECK(parse(g, n, NULL) == EULER_EINVAL);      /* a payload size beyond the file */
    memcpy(g, f, n); memcpy(g + 24, &many, 8); seal(g, n); CHECK(parse(g, n, NULL) == EULER_EINVAL);               /* n_markers beyond the capacity */
    /* records the host checks refuse */
    const float hot = 10001.f, qnan = NAN;
    const uint32_t one = 1;
    memcpy(g, f, n); memcpy(g + g_off[2] + 16 + 8 + 32 + 24 + 4 * 17, &hot, 4); seal(g, n); CHECK(parse(g, n, NULL) == EULER_EINVAL);      /* a cell of the field */
    memcpy(g, f, n); memcpy(g + g_off[2] + 16 + 8 + 12, &hot, 4); seal(g, n); CHECK(parse(g, n, NULL) == EULER_EINVAL);                    /* source_t */
    memcpy(g, f, n); memcpy(g + g_off[3] + 16 + 8, &qnan, 4); seal(g, n); CHECK(parse(g, n, NULL) == EULER_EINVAL);                         /* tracer 0 has no position and no flag */
    memcpy(g, f, n); memcpy(g + g_off[3] + 16 + 8 + 28, &one, 4); seal(g, n); CHECK(parse(g, n, NULL) == EULER_EINVAL);                    /* tracer 0: reserved */
    memcpy(g, f, n); { const double dnan = NAN; memcpy(g + g_off[0] + 16, &dnan, 8); } seal(g, n); CHECK(parse(g, n, NULL) == EULER_EINVAL);   /* the clock */
    memcpy(g, f, n); memcpy(g + g_off[5] + 16, &one, 4); seal(g, n); CHECK(parse(g, n, NULL) == EULER_EINVAL);                             /* thin_above = 1 */
    /* a body over an open cell: the solid grid opened under it, the origin moved, the origin outside the grid */
    memcpy(g, f, n); g[72 + 16 * C + 4 * GX + 5] = 0; seal(g, n); CHECK(parse(g, n, NULL) == EULER_EINVAL);
    const int32_t ox6 = 6, far = 1 << 30;
    memcpy(g, f, n); memcpy(g + g_off[4] + 16 + 8 + 64, &ox6, 4); seal(g, n); CHECK(parse(g, n, NULL) == EULER_EINVAL);
    memcpy(g, f, n); memcpy(g + g_off[4] + 16 + 8 + 64, &far, 4); seal(g, n); CHECK(parse(g, n, NULL) == EULER_EINVAL);
    memcpy(g, f, n); memcpy(g + g_off[4] + 16 + 8 + 64 + 4, &minus, 4); seal(g, n); CHECK(parse(g, n, NULL) == EULER_EINVAL);
    free(g);
  }

  /* ---- the sequence of chunks */
  {
    size_t m;
    unsigned char* g;
    const int same[NCHUNKS] = {0, 1, 2, 3, 4, 5, 6, 7, 8};
    g = reorder(f, same, NCHUNKS, &m); CHECK(m == n && memcmp(g, f, n) == 0 && parse(g, m, NULL) == EULER_OK); free(g);
    const int swapped[NCHUNKS] = {1, 0, 2, 3, 4, 5, 6, 7, 8};
    g = reorder(f, swapped, NCHUNKS, &m); CHECK(parse(g, m, NULL) == EULER_EINVAL); free(g);
    const int twice[NCHUNKS + 1] = {0, 1, 1, 2, 3, 4, 5, 6, 7, 8};
    g = reorder(f, twice, NCHUNKS + 1, &m); CHECK(parse(g, m, NULL) == EULER_EINVAL); free(g);
    g = reorder(f, same, NCHUNKS - 1, &m); CHECK(parse(g, m, NULL) == EULER_EINVAL); free(g);      /* no END */
    const int no_heat[NCHUNKS - 1] = {0, 1, 3, 4, 5, 6, 7, 8};
    g = reorder(f, no_heat, NCHUNKS - 1, &m); CHECK(parse(g, m, NULL) == EULER_EINVAL); free(g);
    const int after_end[NCHUNKS + 1] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 0};
    g = reorder(f, after_end, NCHUNKS + 1, &m); CHECK(parse(g, m, NULL) == EULER_EINVAL); free(g);
    g = reorder(f, same, 0, &m); CHECK(parse(g, m, NULL) == EULER_EINVAL); free(g);                /* a version 4 header over a plain snapshot's bytes */
    g = reorder(f, same, NCHUNKS, &m);
    memcpy(g + g_off[5], "WIND", 4); seal(g, m);
    {
      char why[200];
      eu_session u;
      CHECK(eu_session_parse(g, m, GX, GY, 0, 4 * C, &u, why, sizeof why) == EULER_EINVAL && strstr(why, "WIND"));      /* refused by name */
      const uint32_t v2 = 2;
      memcpy(g + g_off[5], "RSED", 4); memcpy(g + g_off[5] + 4, &v2, 4); seal(g, m);
      CHECK(eu_session_parse(g, m, GX, GY, 0, 4 * C, &u, why, sizeof why) == EULER_EINVAL && strstr(why, "RSED") && strstr(why, "version 2"));
    }
    free(g);
  }

  /* ---- the settings: equal, the first field that differs with both values, the three options that are no settings */
  {
    char why[200] = "";
    eu_session_settings a = s->settings, b = s->settings;
    CHECK(eu_session_settings_diff(&a, &b, why, sizeof why) == 0 && why[0] == '\0');
    b.precond = 2; b.opt[EULER_OPT_ADVECT_RK2] = 0;
    CHECK(eu_session_settings_diff(&a, &b, why, sizeof why) == 1 && strstr(why, "precond") && strstr(why, "has 0") && strstr(why, "handle 2"));
    b = a; b.opt[EULER_OPT_ADVECT_RK2] = 0;
    CHECK(eu_session_settings_diff(&a, &b, why, sizeof why) == 1 && strstr(why, "option 22"));
    b = a; b.viscosity_bits = 0x3dcccccdu;
    CHECK(eu_session_settings_diff(&a, &b, why, sizeof why) == 1 && strstr(why, "viscosity"));
    b = a; b.tol = 1e-7;
    CHECK(eu_session_settings_diff(&a, &b, why, sizeof why) == 1 && strstr(why, "tol"));
    b = a; b.opt[EULER_OPT_PROFILE_STRIDE] = 4; b.opt[EULER_OPT_RESIDENT_FORCE_TIMEOUT] = 1; b.opt[EULER_OPT_MG_SPLIT_ACTIVE] = 1;
    CHECK(eu_session_settings_diff(&a, &b, NULL, 0) == 0);
    b = a; b.max_substeps = 4;
    CHECK(eu_session_settings_diff(&a, &b, NULL, 0) == 1);
  }
  free(t); free(f); free(s);
  printf("clean\n");
  return 0;
}
