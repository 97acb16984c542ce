/* eu_valid.h - what one pass of a handle leaves behind for the next, and whether it still holds.  Plain C (C99 and C++), host only, no HIP:
 * tests/c/stage_validity.c checks every transition below against the definitions in this comment, exhaustively, without a GPU.
 * docs/stage_validity.md is the same page for somebody adding a pass.
 *
 * The stages are lean: each skips work that an earlier pass has made redundant.  A flag of eu_valid PROMISES that the earlier pass's
 * result still stands.  Nothing outside this file reads or writes a flag: a pass that has run reports it with an EVENT, a pass about
 * to choose its form asks a QUERY.  Whoever writes u, v, utmp, vtmp, the count grids, the markers or the masks from outside the
 * substep's own sequence calls eu_vd_edited (masks: eu_vd_masks_changed; everything at once: eu_vd_replaced) BEFORE the first write.
 *
 * flag           promises                                                   established by              aged by a refresh    broken by
 * -------------------------------------------------------------------------------------------------------------------------------------------------
 * p_pending      0: p in memory is finished and clamped; 1: memory lacks    velocity_updated (one       -                    (settled by) assembled,
 *                the last fmadds and the clamp; 2: the clamp only           pass: ring in use 1, else 2)                     pressure_made_current, replaced
 * maxsq_state    ms->max_u2_bits / max_v2_bits: 0 - zero; 2 - the maxima    velocity_updated (one pass  -                    2 -> 1: edited, extrapolated,
 *                of u, v AS THEY STAND; 1 - maxima of an earlier u, v       with do_max): 2;                                 advected_velocity (viscous: u, v are
 *                                                                           timestep_ran: 0                                  its scratch), any other velocity update
 * uv_clean       1: the last one-pass velocity update left every sample     velocity_updated (one pass) 1 -> 2 -> 0          edited
 *                without the fluid property / with the solid property zero
 *                and no refresh has run since; 2: ... and exactly one has
 * uv_zb          zero_bounds has run with the count grid as it stands       extrapolated                -> 0                 edited, sources_ran
 * count32_dirty  the binning counters hold something                        binning_began               -> 0 (cleared)       -
 * prebin_valid   the marker advection DIRECTLY in front binned its own      advected_markers (fused)    -> 0 (consumed)      edited, sources_ran, a marker advection
 *                output: counters and delete ballot stand                                                                    that did not, any stage but the refresh
 * tmap_valid     both tile maps describe count / prev_count                 refreshed                   -                    edited
 * utmp_clean     1: utmp / vtmp are zero wherever the typed fluid property  advected_velocity           1 -> 2 -> 0          edited, advected_velocity (viscous:
 *                of the count grid does not hold; 2: ... of prev_count      (inviscid)                                       the diffusion writes them behind it)
 * countT_clean   the same for countT                                        transposed                  1 -> 2 -> 0          edited
 * blocked_dirty  blockedT (sink | solid, column-major) is out of date       masks_changed               -                    (settled by) blocked_rebuilt
 * solidT_dirty   solidT is out of date                                      masks_changed               -                    (settled by) transposed
 * lean_ok        the solver arrays have only been written by solves since   assembled                   -                    solver_arrays_foreign
 *                chunk_prev was current
 *
 * (edited includes masks_changed and replaced, which call it.)  The 1 -> 2 -> 0 flags serve passes that compare the count grid with the
 * previous one: their readers want exactly 2, "one refresh ago".
 *
 * Deliberately more conservative than the promise needs (the check's model says the same): every stage but the refresh drops prebin_valid,
 * not only those that touch the markers; sources_ran drops uv_zb and prebin_valid in a scene without source cells too; replaced and
 * edited lower maxsq_state to 1 where the maxima are in fact zero again (a load); a two-pass velocity update leaves uv_clean unset although
 * it zeroes the same samples; a viscous advection drops utmp_clean although the diffusion keeps the zeros.
 *
 * Row-slab handles run the shared launchers and so report the same events; every query that matters there takes slab_on and says no. */
#ifndef EU_VALID_H
#define EU_VALID_H

#include "euler.h"

typedef struct eu_valid {
  int p_pending, maxsq_state, uv_clean, uv_zb, count32_dirty, prebin_valid, tmap_valid, utmp_clean, countT_clean, blocked_dirty, solidT_dirty, lean_ok;
} eu_valid;

/* ---- events: outside writers ------------------------------------------------------------------------------------------------------------- */
/* somebody other than the substep's own sequence is about to write u, v, utmp, vtmp, a count grid or the markers */
static inline void eu_vd_edited(eu_valid* v) {
  v->prebin_valid = 0;                               /* (k_advect_bin_a2's counts and delete ballot) */
  if (v->maxsq_state == 2) v->maxsq_state = 1;       /* (k_velocity_update_para's maxima of u, v: stale, cleared before the next accumulation) */
  v->uv_clean = 0; v->uv_zb = 0;                     /* (what the lean zero_bounds / the velocity update's skipped zero stores rely on) */
  v->tmap_valid = 0; v->utmp_clean = 0; v->countT_clean = 0;
}
/* ... the solid or the sink grid: the marker stage's column-major copies follow at their next use */
static inline void eu_vd_masks_changed(eu_valid* v) {
  eu_vd_edited(v);
  v->blocked_dirty = 1; v->solidT_dirty = 1;
}
/* the grids of the handle are (re)written whole - allocation, a scenario load, a snapshot: nothing one stage prepared for the next describes them any more */
static inline void eu_vd_replaced(eu_valid* v) {
  eu_vd_masks_changed(v);
  v->p_pending = 0;
}
/* the solver arrays hold something no solve of this handle wrote (euler_set_precond, euler_set_field on a skewed field, euler_load_state, the resident redo):
   the next assembly writes them whole */
static inline void eu_vd_solver_arrays_foreign(eu_valid* v) { v->lean_ok = 0; }

/* ---- events: the stage sequence, each reported by the launcher that ran ------------------------------------------------------------------------ */
/* euler_stage / a substep is about to run this stage: what k_advect_bin_a2 binned belongs to the refresh that follows it DIRECTLY */
static inline void eu_vd_stage_begin(eu_valid* v, int stage) {
  if (stage != EULER_STAGE_REFRESH_COUNTS) v->prebin_valid = 0;
}
/* k_dt or k_maxsq<true> formed dt: either leaves the maxima zero for the next accumulation */
static inline void eu_vd_timestep_ran(eu_valid* v) { v->maxsq_state = 0; }
/* k_transpose_for_markers wrote uT, vT, countT (and solidT where it was due) */
static inline void eu_vd_transposed(eu_valid* v) { v->solidT_dirty = 0; v->countT_clean = 1; }
static inline void eu_vd_blocked_rebuilt(eu_valid* v) { v->blocked_dirty = 0; }
/* a pass is about to add into count32 (from here until the next k_narrow_counts<true>) */
static inline void eu_vd_binning_began(eu_valid* v) { v->count32_dirty = 1; }
/* fused: the passes binned what they wrote (k_advect_bin_a2, pass B) - consumed by the refresh that follows, dropped by anything else in between */
static inline void eu_vd_advected_markers(eu_valid* v, int fused) { v->prebin_valid = fused ? 1 : 0; }
/* k_narrow_counts<true>: prev <- cur, cur <- the counters, the counters <- 0, both tile maps written.  The grids rotate HERE, so the ageing is here too:
   a scenario load refreshes without a stage around it */
static inline void eu_vd_refreshed(eu_valid* v) {
  v->uv_clean = v->uv_clean == 1 ? 2 : 0;            /* (prev <- cur: once is what k_zero_bounds4<true> expects) */
  v->utmp_clean = v->utmp_clean == 1 ? 2 : 0; v->countT_clean = v->countT_clean == 1 ? 2 : 0;      /* (the same for what the tile map's readers left) */
  v->uv_zb = 0;                                      /* (the count grid changes) */
  v->prebin_valid = 0;
  v->tmap_valid = 1;                                 /* (both maps are what this pass saw; EULER_OPT_NO_TILE_MAP only stops the READERS) */
  v->count32_dirty = 0;
}
/* the source stage ran (k_source_place sets the tile flags of what it fills itself): the count grid changes, markers join */
static inline void eu_vd_sources_ran(eu_valid* v) { v->uv_zb = 0; v->prebin_valid = 0; }
/* the marker density control ran behind the refresh (k_reseed.hip, docs/reseed.md): markers leave and join, a count changes - a thinned cell stays wet, a filled
   hole was water one refresh ago and its tile's flag is set by the pass itself, as k_source_place does.  What the source stage drops, for the same reasons; both
   are down already behind a refresh, so the event changes nothing there: it keeps the promise where somebody calls the pass from elsewhere */
static inline void eu_vd_reseeded(eu_valid* v) { v->uv_zb = 0; v->prebin_valid = 0; }
/* extrapolate + zero_bounds wrote u, v (inside a substep the timestep has consumed the maxima long before) */
static inline void eu_vd_extrapolated(eu_valid* v) {
  if (v->maxsq_state == 2) v->maxsq_state = 1;
  v->uv_zb = 1;
}
/* k_advect_velocity wrote utmp / vtmp; viscous: the diffusion extension behind it rewrites them and uses u, v as its Jacobi scratch */
static inline void eu_vd_advected_velocity(eu_valid* v, int viscous) {
  v->utmp_clean = viscous ? 0 : 1;
  if (viscous && v->maxsq_state == 2) v->maxsq_state = 1;
}
/* the assembly wrote p afresh (whatever the last solve left unfinished in memory is gone with it); its chunk flags describe everything that is non-zero from here on */
static inline void eu_vd_assembled(eu_valid* v) { v->p_pending = 0; v->lean_ok = 1; }
/* one_pass: k_velocity_update_para - finished and clamped the pressure in LDS only (ring_use: memory still lacks the last fmadds too), left the air's and the
   walls' samples zero and, with do_max, the maxima of u, v as they stand in ms.  Otherwise k_finish_p + k_velocity_update: p is finished in memory.
   Every form writes u, v: maxima it did not form itself are stale */
static inline void eu_vd_velocity_updated(eu_valid* v, int one_pass, int ring_use, int do_max) {
  if (one_pass) { v->uv_clean = 1; v->p_pending = ring_use ? 1 : 2; }
  if (one_pass && do_max) v->maxsq_state = 2;
  else if (v->maxsq_state == 2) v->maxsq_state = 1;
}
/* eu_pressure_current formed the finished, clamped pressure in memory */
static inline void eu_vd_pressure_made_current(eu_valid* v) { v->p_pending = 0; }

/* ---- queries: one per lean decision; handle facts (row slabs, options, viscosity) come in as ints --------------------------------------------------- */
/* the tile map describes both count grids and the caller may use it (map_off: no map allocated, a row slab, EULER_OPT_NO_TILE_MAP) */
static inline int eu_vd_tile_map(const eu_valid* v, int map_off) { return v->tmap_valid && !map_off; }
/* k_zero_bounds4<true>: exactly one refresh between the last one-pass velocity update and now, nobody edited the state */
static inline int eu_vd_lean_zero_bounds(const eu_valid* v, int slab_on, int two_pass) { return !slab_on && v->uv_clean == 2 && !two_pass; }
/* k_advect_velocity over the tile map: utmp / vtmp are what this kernel left one refresh ago */
static inline int eu_vd_lean_advect(const eu_valid* v, int map_on, int viscous) { return map_on && v->utmp_clean == 2 && !viscous; }
/* k_transpose_for_markers over the tile map */
static inline int eu_vd_lean_transpose(const eu_valid* v, int map_on) { return map_on && v->countT_clean == 2 && !v->solidT_dirty; }
static inline int eu_vd_solidT_due(const eu_valid* v) { return v->solidT_dirty; }
static inline int eu_vd_blocked_due(const eu_valid* v) { return v->blocked_dirty; }
static inline int eu_vd_count32_must_clear(const eu_valid* v) { return v->count32_dirty; }
/* the refresh keeps the counters and the delete ballot of the advection in front; with the tile map in use that pass also marked every tile a marker entered */
static inline int eu_vd_prebinned(const eu_valid* v) { return v->prebin_valid; }
static inline int eu_vd_touch_known(const eu_valid* v, int no_tile_map) { return v->prebin_valid && !no_tile_map; }
/* eu_launch_timestep on a whole-grid handle */
enum { EU_DT_MAXSQ = 0, EU_DT_CLEAR_MAXSQ = 1, EU_DT_ONLY = 2 };      /* k_maxsq<true>; the same behind a clear of stale maxima; k_dt alone on the maxima as they stand */
static inline int eu_vd_timestep_mode(const eu_valid* v) { return v->maxsq_state; }
/* k_velocity_update_para need not store the zeros of the air and the walls again */
static inline int eu_vd_update_skips_zeros(const eu_valid* v, int slab_on) { return !slab_on && v->uv_zb; }
/* ... and must clear maxima no timestep consumed before it accumulates its own */
static inline int eu_vd_update_clears_maxima(const eu_valid* v, int do_max) { return do_max && v->maxsq_state != 0; }
/* what eu_pressure_current owes: 0 - nothing, 1 - the last fmadds and the clamp, 2 - the clamp */
static inline int eu_vd_pressure_owes(const eu_valid* v) { return v->p_pending; }
/* k_build_system<true>: tile_band - a tile-mode preconditioner with the band schedule */
static inline int eu_vd_lean_assembly(const eu_valid* v, int tile_band) { return tile_band && v->lean_ok; }

#endif
