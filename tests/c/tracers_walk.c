/* tracers_walk.c - the walk of passive tracers (docs/tracers.md) for tests/tracers_ref.py: every tracer is an ARRAY OF ONE MARKER handed to the
 * oracle-side marker walk (ar_advect_markers of advect_rk2.c; rk2 = 0: eo_advect_markers statement for statement), so the dt chain of a marker array
 * never couples two tracers and never reaches the fluid's markers, which are put back as they were.
 *
 * Built at test time: gcc -O2 -ffp-contract=off -shared, linked against liboracle.so. */
#include "advect_rk2.c"

void tr_walk(eo_sim* s, float* xy, size_t n, float dt, int rk2) {
  eo_vec2f* const keep = s->markers;
  const size_t keep_n = s->n_markers;
  for (size_t k = 0; k < n; ++k) {
    eo_vec2f one = {xy[2 * k], xy[2 * k + 1]};
    s->markers = &one; s->n_markers = 1;
    (void)ar_advect_markers(s, dt, rk2);
    xy[2 * k] = one.x; xy[2 * k + 1] = one.y;
  }
  s->markers = keep; s->n_markers = keep_n;
}
