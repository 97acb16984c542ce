/* The stage hand-off flags (euler_amd/csrc/eu_valid.h) without a GPU.
 *  (a) the canonical order: three substeps of a whole-grid handle from eu_vd_replaced, with the branches each launcher takes, against a table
 *      written from the launchers' conditions - default options, each A-B option, viscosity on;
 *  (b) soundness: every sequence of up to DEPTH events from eu_vd_replaced; after every prefix each query must equal what a naive second model
 *      says - the promise in eu_valid.h's table, evaluated by scanning the log of events backwards.
 * Prints "stage validity: ok ..." and exits 0, or the offending sequences and exits 1. */
#include <stdio.h>
#include <string.h>

#include "eu_valid.h"
#include "euler.h"

#define DEPTH 5      /* 28 events: 28^5 = 17 M sequences, 18 M prefixes, about 2 s with -O2; depth 6 would be a minute */

/* ------------------------------------------------------------------------------------------------------------------ the event alphabet: every branch variant */
enum {
  E_REPLACED, E_EDITED, E_MASKS, E_FOREIGN,
  E_BEGIN0, E_BEGIN1, E_BEGIN2, E_BEGIN3, E_BEGIN4, E_BEGIN5,      /* eu_vd_stage_begin(EULER_STAGE_*) */
  E_TIMESTEP, E_TRANSPOSED, E_BLOCKED, E_BINNING, E_ADVM_PLAIN, E_ADVM_FUSED, E_REFRESHED, E_SOURCES, E_EXTRAPOLATED,
  E_ADVV, E_ADVV_VISCOUS, E_ASSEMBLED,
  E_VU_TWO_PASS, E_VU_ONE, E_VU_ONE_RING, E_VU_ONE_MAX, E_VU_ONE_RING_MAX,      /* (without MAX: a row slab's one-pass update) */
  E_PRESSURE_CURRENT, E__COUNT
};
static const char* const e_name[E__COUNT] = {
  "replaced", "edited", "masks_changed", "solver_arrays_foreign", "stage_begin(ADVECT_MARKERS)", "stage_begin(REFRESH_COUNTS)", "stage_begin(SOURCES)",
  "stage_begin(EXTRAPOLATE)", "stage_begin(ADVECT_VELOCITY)", "stage_begin(PROJECT)", "timestep_ran", "transposed", "blocked_rebuilt", "binning_began",
  "advected_markers(0)", "advected_markers(1)", "refreshed", "sources_ran", "extrapolated", "advected_velocity(0)", "advected_velocity(viscous)", "assembled",
  "velocity_updated(two pass)", "velocity_updated(1,0,0)", "velocity_updated(1,ring,0)", "velocity_updated(1,0,max)", "velocity_updated(1,ring,max)", "pressure_made_current"};

static void apply(eu_valid* v, int e) {
  switch (e) {
    case E_REPLACED: eu_vd_replaced(v); break;
    case E_EDITED: eu_vd_edited(v); break;
    case E_MASKS: eu_vd_masks_changed(v); break;
    case E_FOREIGN: eu_vd_solver_arrays_foreign(v); break;
    case E_BEGIN0: case E_BEGIN1: case E_BEGIN2: case E_BEGIN3: case E_BEGIN4: case E_BEGIN5: eu_vd_stage_begin(v, EULER_STAGE_ADVECT_MARKERS + (e - E_BEGIN0)); break;
    case E_TIMESTEP: eu_vd_timestep_ran(v); break;
    case E_TRANSPOSED: eu_vd_transposed(v); break;
    case E_BLOCKED: eu_vd_blocked_rebuilt(v); break;
    case E_BINNING: eu_vd_binning_began(v); break;
    case E_ADVM_PLAIN: eu_vd_advected_markers(v, 0); break;
    case E_ADVM_FUSED: eu_vd_advected_markers(v, 1); break;
    case E_REFRESHED: eu_vd_refreshed(v); break;
    case E_SOURCES: eu_vd_sources_ran(v); break;
    case E_EXTRAPOLATED: eu_vd_extrapolated(v); break;
    case E_ADVV: eu_vd_advected_velocity(v, 0); break;
    case E_ADVV_VISCOUS: eu_vd_advected_velocity(v, 1); break;
    case E_ASSEMBLED: eu_vd_assembled(v); break;
    case E_VU_TWO_PASS: eu_vd_velocity_updated(v, 0, 0, 0); break;
    case E_VU_ONE: eu_vd_velocity_updated(v, 1, 0, 0); break;
    case E_VU_ONE_RING: eu_vd_velocity_updated(v, 1, 1, 0); break;
    case E_VU_ONE_MAX: eu_vd_velocity_updated(v, 1, 0, 1); break;
    case E_VU_ONE_RING_MAX: eu_vd_velocity_updated(v, 1, 1, 1); break;
    case E_PRESSURE_CURRENT: eu_vd_pressure_made_current(v); break;
  }
}

/* ------------------------------------------------------------------------------------------------------------------ the naive model: the log, scanned backwards.
 * lg[0] is always the E_REPLACED of a zeroed handle (creation); "the start" below is running off the front of the log. */
static int lg[DEPTH + 64], ln;

static int outside_write(int e) { return e == E_EDITED || e == E_MASKS || e == E_REPLACED; }      /* of u, v, utmp, vtmp, a count grid or the markers */
static int one_pass_update(int e) { return e >= E_VU_ONE && e <= E_VU_ONE_RING_MAX; }
static int forms_maxima(int e) { return e == E_VU_ONE_MAX || e == E_VU_ONE_RING_MAX; }
/* writes u or v without leaving their maxima in ms */
static int writes_uv(int e) { return outside_write(e) || e == E_EXTRAPOLATED || e == E_ADVV_VISCOUS || e == E_VU_TWO_PASS || e == E_VU_ONE || e == E_VU_ONE_RING; }

/* what memory's pressure lacks: the last one-pass update says (ring: 1, else 2) unless the assembly wrote p afresh, somebody finished it or the state was replaced since.
   (A two-pass update leaves the pressure as it found it: finished.) */
static int m_pressure_owes(void) {
  for (int i = ln - 1; i >= 0; --i) {
    if (lg[i] == E_VU_ONE_RING || lg[i] == E_VU_ONE_RING_MAX) return 1;
    if (lg[i] == E_VU_ONE || lg[i] == E_VU_ONE_MAX) return 2;
    if (lg[i] == E_ASSEMBLED || lg[i] == E_PRESSURE_CURRENT || lg[i] == E_REPLACED) return 0;
  }
  return 0;
}
/* ms's maxima: zero after a timestep (and at the start); behind an update that formed them, those of u, v as they stand (2) while nothing else has written u, v since, else stale (1).
   (Conservative by design: an outside write counts as "written" whichever array it went to.) */
static int m_maxima(void) {
  int written = 0;
  for (int i = ln - 1; i >= 0; --i) {
    if (lg[i] == E_TIMESTEP) return 0;
    if (forms_maxima(lg[i])) return written ? 1 : 2;
    if (writes_uv(lg[i])) written = 1;
  }
  return 0;
}
/* something a pass left with respect to the count grid, aged by the refreshes since: 1 - none, 2 - exactly one, 0 - more, an outside write since, or never left */
static int m_aged(int made_a, int made_b, int unmade) {
  int refreshes = 0;
  for (int i = ln - 1; i >= 0; --i) {
    if (outside_write(lg[i]) || lg[i] == unmade) return 0;
    if (lg[i] == E_REFRESHED) ++refreshes;
    if (lg[i] == made_a || lg[i] == made_b) return refreshes == 0 ? 1 : refreshes == 1 ? 2 : 0;
  }
  return 0;
}
static int m_uv_clean(void) {      /* (any one-pass update; a two-pass one leaves the promise as it found it: it zeroes the same samples) */
  int refreshes = 0;
  for (int i = ln - 1; i >= 0; --i) {
    if (outside_write(lg[i])) return 0;
    if (lg[i] == E_REFRESHED) ++refreshes;
    if (one_pass_update(lg[i])) return refreshes == 0 ? 1 : refreshes == 1 ? 2 : 0;
  }
  return 0;
}
static int m_utmp_clean(void) { return m_aged(E_ADVV, E_ADVV, E_ADVV_VISCOUS); }
static int m_countT_clean(void) { return m_aged(E_TRANSPOSED, E_TRANSPOSED, -1); }
/* zero_bounds ran and the count grid has not changed since */
static int m_uv_zb(void) {
  for (int i = ln - 1; i >= 0; --i) {
    if (lg[i] == E_EXTRAPOLATED) return 1;
    if (outside_write(lg[i]) || lg[i] == E_REFRESHED || lg[i] == E_SOURCES) return 0;
  }
  return 0;
}
static int m_count32_dirty(void) {
  for (int i = ln - 1; i >= 1; --i) {
    if (lg[i] == E_BINNING) return 1;
    if (lg[i] == E_REFRESHED) return 0;
  }
  return 0;
}
/* a fused marker advection, and since then no outside write, no refresh, no source stage, no other advection - and (conservative by design) no stage but the refresh begun */
static int m_prebinned(void) {
  for (int i = ln - 1; i >= 0; --i) {
    const int e = lg[i];
    if (e == E_ADVM_FUSED) return 1;
    if (outside_write(e) || e == E_ADVM_PLAIN || e == E_REFRESHED || e == E_SOURCES || (e >= E_BEGIN0 && e <= E_BEGIN5 && e != E_BEGIN1)) return 0;
  }
  return 0;
}
static int m_tile_map(void) {
  for (int i = ln - 1; i >= 0; --i) {
    if (lg[i] == E_REFRESHED) return 1;
    if (outside_write(lg[i])) return 0;
  }
  return 0;
}
static int m_mask_copy_due(int rebuilt) {      /* blockedT / solidT: a mask changed (or everything was replaced) and the copy has not been rebuilt since */
  for (int i = ln - 1; i >= 0; --i) {
    if (lg[i] == rebuilt) return 0;
    if (lg[i] == E_MASKS || lg[i] == E_REPLACED) return 1;
  }
  return 1;
}
static int m_lean_ok(void) {
  for (int i = ln - 1; i >= 1; --i) {
    if (lg[i] == E_ASSEMBLED) return 1;
    if (lg[i] == E_FOREIGN) return 0;
  }
  return 0;
}

static long long n_checked, n_bad;
static void differ(const char* what, int got, int want) {
  if (++n_bad > 12) return;
  printf("  %s = %d, the log says %d after:", what, got, want);
  for (int i = 1; i < ln; ++i) printf(" %s%s", e_name[lg[i]], i + 1 < ln ? "," : "");
  printf("\n");
}
#define SAME(what, got, want) do { const int g_ = (got), w_ = (want); if (g_ != w_) differ(what, g_, w_); } while (0)
static void check(const eu_valid* v) {
  ++n_checked;
  const int maxima = m_maxima(), solidT_due = m_mask_copy_due(E_TRANSPOSED), pre = m_prebinned();
  SAME("pressure_owes", eu_vd_pressure_owes(v), m_pressure_owes());
  SAME("timestep_mode", eu_vd_timestep_mode(v), maxima);
  SAME("update_clears_maxima", eu_vd_update_clears_maxima(v, 1), maxima != 0);
  SAME("lean_zero_bounds", eu_vd_lean_zero_bounds(v, 0, 0), m_uv_clean() == 2);
  SAME("update_skips_zeros", eu_vd_update_skips_zeros(v, 0), m_uv_zb());
  SAME("count32_must_clear", eu_vd_count32_must_clear(v), m_count32_dirty());
  SAME("prebinned", eu_vd_prebinned(v), pre);
  SAME("touch_known", eu_vd_touch_known(v, 0), pre);
  SAME("tile_map", eu_vd_tile_map(v, 0), m_tile_map());
  SAME("lean_advect", eu_vd_lean_advect(v, 1, 0), m_utmp_clean() == 2);
  SAME("lean_transpose", eu_vd_lean_transpose(v, 1), m_countT_clean() == 2 && !solidT_due);
  SAME("solidT_due", eu_vd_solidT_due(v), solidT_due);
  SAME("blocked_due", eu_vd_blocked_due(v), m_mask_copy_due(E_BLOCKED));
  SAME("lean_assembly", eu_vd_lean_assembly(v, 1), m_lean_ok());
}
static void walk(eu_valid v, int depth) {
  check(&v);
  if (depth == 0) return;
  for (int e = 0; e < E__COUNT; ++e) {
    eu_valid w = v;
    apply(&w, e);
    lg[ln++] = e;
    walk(w, depth - 1);
    --ln;
  }
}
static eu_valid fresh(void) {
  eu_valid v;
  memset(&v, 0, sizeof v);
  eu_vd_replaced(&v);
  lg[0] = E_REPLACED; ln = 1;
  return v;
}

/* ------------------------------------------------------------------------------------------------------------------ (a) the canonical order
 * The branches of a whole-grid handle's launchers (tile-mode preconditioner, multi-kernel solve: the ring is in use), as events; what each lean decision saw, per substep. */
struct opts { int markers_two_pass, velocity_two_pass, no_tile_map, rowmajor, viscous; };
enum { P_DT, P_MAP, P_TRANSPOSE, P_PREBIN, P_TOUCH, P_ZB, P_ADVECT, P_ASSEMBLY, P_SKIP0, P_CLEARMAX, P_OWES, P__COUNT };
static const char* const p_name[P__COUNT] = {"timestep_mode", "tile_map (marker stage)", "lean_transpose", "prebinned", "touch_known", "lean_zero_bounds", "lean_advect",
                                             "lean_assembly", "update_skips_zeros", "update_clears_maxima", "pressure_owes (end)"};
static void substep(eu_valid* v, const struct opts* o, int* p) {
  memset(p, 0, P__COUNT * sizeof *p);
  p[P_DT] = eu_vd_timestep_mode(v); eu_vd_timestep_ran(v);
  eu_vd_stage_begin(v, EULER_STAGE_ADVECT_MARKERS);
  p[P_MAP] = eu_vd_tile_map(v, o->no_tile_map);
  if (!o->rowmajor) {
    p[P_TRANSPOSE] = eu_vd_lean_transpose(v, p[P_MAP]);
    eu_vd_transposed(v);
    if (!o->markers_two_pass) { if (eu_vd_blocked_due(v)) eu_vd_blocked_rebuilt(v); eu_vd_binning_began(v); }
    eu_vd_advected_markers(v, !o->markers_two_pass);
  } else eu_vd_advected_markers(v, 0);
  eu_vd_stage_begin(v, EULER_STAGE_REFRESH_COUNTS);
  p[P_PREBIN] = eu_vd_prebinned(v); p[P_TOUCH] = eu_vd_touch_known(v, o->no_tile_map);
  if (!p[P_PREBIN]) { if (eu_vd_blocked_due(v)) eu_vd_blocked_rebuilt(v); eu_vd_binning_began(v); }
  eu_vd_refreshed(v);
  eu_vd_stage_begin(v, EULER_STAGE_SOURCES);
  eu_vd_sources_ran(v);
  eu_vd_stage_begin(v, EULER_STAGE_EXTRAPOLATE);
  p[P_ZB] = eu_vd_lean_zero_bounds(v, 0, o->velocity_two_pass);
  eu_vd_extrapolated(v);
  eu_vd_stage_begin(v, EULER_STAGE_ADVECT_VELOCITY);
  p[P_ADVECT] = eu_vd_lean_advect(v, eu_vd_tile_map(v, o->no_tile_map), o->viscous);
  eu_vd_advected_velocity(v, o->viscous);
  eu_vd_stage_begin(v, EULER_STAGE_PROJECT);
  p[P_ASSEMBLY] = eu_vd_lean_assembly(v, 1);
  eu_vd_assembled(v);
  if (!o->velocity_two_pass) {
    p[P_SKIP0] = eu_vd_update_skips_zeros(v, 0); p[P_CLEARMAX] = eu_vd_update_clears_maxima(v, 1);
    eu_vd_velocity_updated(v, 1, 1, 1);
  } else eu_vd_velocity_updated(v, 0, 0, 0);
  p[P_OWES] = eu_vd_pressure_owes(v);
}
static int canonical(const char* name, struct opts o, const int off[P__COUNT]) {
  /* default options.  Substep 1: only what its own advection binned and its own zero_bounds zeroed is known (no tile map before the first refresh, the solver arrays are
     not yet a solve's).  From substep 2 on every lean form: the k_dt-only timestep, countT / u, v / utmp, vtmp each one refresh old. */
  static const int want1[P__COUNT] = {EU_DT_MAXSQ, 0, 0, 1, 1, 0, 0, 0, 1, 0, 1}, want23[P__COUNT] = {EU_DT_ONLY, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1};
  eu_valid v = fresh();
  int bad = 0, p[P__COUNT];
  for (int s = 1; s <= 3; ++s) {
    substep(&v, &o, p);
    for (int k = 0; k < P__COUNT; ++k) {
      const int want = off[k] ? 0 : (s == 1 ? want1[k] : want23[k]);      /* (every "off" value is 0: EU_DT_MAXSQ, nothing owed, not lean) */
      if (p[k] != want) { printf("  canonical order, %s, substep %d: %s = %d, expected %d\n", name, s, p_name[k], p[k], want); ++bad; }
    }
  }
  return bad;
}

int main(void) {
  int bad = 0;
  /* (a) - exactly the predicates the option's branch feeds turn off */
  static const int none[P__COUNT] = {0};
  static const int markers_two_pass[P__COUNT] = {[P_PREBIN] = 1, [P_TOUCH] = 1};
  static const int velocity_two_pass[P__COUNT] = {[P_DT] = 1, [P_ZB] = 1, [P_SKIP0] = 1, [P_OWES] = 1};      /* (p is finished in memory; no maxima are left; uv_clean is never set) */
  static const int no_tile_map[P__COUNT] = {[P_MAP] = 1, [P_TRANSPOSE] = 1, [P_TOUCH] = 1, [P_ADVECT] = 1};   /* (the lean zero_bounds and the kept counters do not read the map) */
  static const int rowmajor[P__COUNT] = {[P_TRANSPOSE] = 1, [P_PREBIN] = 1, [P_TOUCH] = 1};
  static const int viscous[P__COUNT] = {[P_ADVECT] = 1};
  bad += canonical("default", (struct opts){0, 0, 0, 0, 0}, none);
  bad += canonical("EULER_OPT_MARKERS_TWO_PASS", (struct opts){1, 0, 0, 0, 0}, markers_two_pass);
  bad += canonical("EULER_OPT_VELOCITY_TWO_PASS", (struct opts){0, 1, 0, 0, 0}, velocity_two_pass);
  bad += canonical("EULER_OPT_NO_TILE_MAP", (struct opts){0, 0, 1, 0, 0}, no_tile_map);
  bad += canonical("EULER_OPT_MARKERS_ROWMAJOR", (struct opts){0, 0, 0, 1, 0}, rowmajor);
  bad += canonical("viscosity > 0", (struct opts){0, 0, 0, 0, 1}, viscous);
  /* the handle facts gate the queries: a row slab, the A-B options and viscosity say no whatever the flags say */
  {
    eu_valid v = fresh();
    int p[P__COUNT];
    const struct opts o = {0, 0, 0, 0, 0};
    substep(&v, &o, p); substep(&v, &o, p);
    eu_vd_timestep_ran(&v); eu_vd_stage_begin(&v, EULER_STAGE_ADVECT_MARKERS); eu_vd_transposed(&v); eu_vd_advected_markers(&v, 1); eu_vd_stage_begin(&v, EULER_STAGE_REFRESH_COUNTS);
    if (!eu_vd_touch_known(&v, 0) || eu_vd_touch_known(&v, 1)) { printf("  touch_known ignores EULER_OPT_NO_TILE_MAP\n"); ++bad; }
    eu_vd_refreshed(&v); eu_vd_extrapolated(&v);
    if (!eu_vd_tile_map(&v, 0) || eu_vd_tile_map(&v, 1)) { printf("  tile_map ignores map_off\n"); ++bad; }
    if (!eu_vd_lean_zero_bounds(&v, 0, 0) || eu_vd_lean_zero_bounds(&v, 1, 0) || eu_vd_lean_zero_bounds(&v, 0, 1)) { printf("  lean_zero_bounds ignores a fact\n"); ++bad; }
    if (!eu_vd_lean_advect(&v, 1, 0) || eu_vd_lean_advect(&v, 0, 0) || eu_vd_lean_advect(&v, 1, 1)) { printf("  lean_advect ignores a fact\n"); ++bad; }
    if (!eu_vd_update_skips_zeros(&v, 0) || eu_vd_update_skips_zeros(&v, 1)) { printf("  update_skips_zeros ignores slab_on\n"); ++bad; }
    if (!eu_vd_lean_assembly(&v, 1) || eu_vd_lean_assembly(&v, 0)) { printf("  lean_assembly ignores tile_band\n"); ++bad; }
    eu_vd_velocity_updated(&v, 1, 1, 1);
    if (!eu_vd_update_clears_maxima(&v, 1) || eu_vd_update_clears_maxima(&v, 0)) { printf("  update_clears_maxima ignores do_max\n"); ++bad; }
  }
  /* the two holes this check was written for, by name: a stage that rewrites u, v behind a velocity update must not leave the k_dt-only timestep standing */
  {
    eu_valid v = fresh();
    eu_vd_velocity_updated(&v, 1, 1, 1); eu_vd_stage_begin(&v, EULER_STAGE_ADVECT_VELOCITY); eu_vd_advected_velocity(&v, 1);
    if (eu_vd_timestep_mode(&v) != EU_DT_CLEAR_MAXSQ) { printf("  PROJECT, viscous ADVECT_VELOCITY: timestep_mode = %d\n", eu_vd_timestep_mode(&v)); ++bad; }
    v = fresh();
    eu_vd_velocity_updated(&v, 1, 1, 1); eu_vd_assembled(&v); eu_vd_velocity_updated(&v, 0, 0, 0);
    if (eu_vd_timestep_mode(&v) != EU_DT_CLEAR_MAXSQ) { printf("  PROJECT, PROJECT with EULER_OPT_VELOCITY_TWO_PASS: timestep_mode = %d\n", eu_vd_timestep_mode(&v)); ++bad; }
  }
  /* (b) */
  walk(fresh(), DEPTH);
  if (n_bad) printf("  ... %lld differences in all\n", n_bad);
  if (bad || n_bad) { printf("stage validity: FAILED\n"); return 1; }
  printf("stage validity: ok (%lld prefixes of up to %d events over %d)\n", n_checked, DEPTH, (int)E__COUNT);
  return 0;
}
