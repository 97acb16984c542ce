/*
 * cli_tracers.h — the host-only parts of `euler --tracer / --tracer-box / --emit / --tracers` (docs/tracers.md): the parsers of the three specs and the
 * formatter of a CSV line.  In a header of their own so that tests/c/sanitize_tracers.c runs them under the sanitizers without the command's main().
 */
#ifndef EULER_CLI_TRACERS_H
#define EULER_CLI_TRACERS_H
#include <stdio.h>
#include <string.h>

#include "euler.h"

#define MAX_CLI_TRACERS 1024
#define MAX_TRACER_BOXES 64
#define MAX_EMITTERS 64

/* what is added once behind the load, in command-line order: a point (k = 0) or the k x k lattice of a box of cells */
typedef struct cli_seed { int k; float x, y; int box[4]; } cli_seed;
typedef struct cli_emitter { float x, y; int every; } cli_emitter;

static int cli_tracer_finite(float v) { return v >= -3.4028234663852886e38f && v <= 3.4028234663852886e38f; }      /* (a NaN fails both comparisons) */

/* X,Y -> a point (checked against the grid later); -1: malformed or not finite */
static int parse_tracer(const char* arg, cli_seed* s) {
  char tail;
  memset(s, 0, sizeof *s);
  if (sscanf(arg, "%f,%f%c", &s->x, &s->y, &tail) != 2) return -1;
  return cli_tracer_finite(s->x) && cli_tracer_finite(s->y) ? 0 : -1;
}

/* X0,Y0,X1,Y1:K -> the lattice of a box (checked against the grid later); -1: malformed or K not 1, 2 or 4 */
static int parse_tracer_box(const char* arg, cli_seed* s) {
  char tail;
  memset(s, 0, sizeof *s);
  if (sscanf(arg, "%d,%d,%d,%d:%d%c", &s->box[0], &s->box[1], &s->box[2], &s->box[3], &s->k, &tail) != 5) return -1;
  return s->k == 1 || s->k == 2 || s->k == 4 ? 0 : -1;
}

/* X,Y[:EVERY] -> an emitter, EVERY >= 1 (default 1); -1: malformed, not finite or EVERY < 1 */
static int parse_emit(const char* arg, cli_emitter* e) {
  char tail;
  e->every = 1;
  const int n = sscanf(arg, "%f,%f:%d%c", &e->x, &e->y, &e->every, &tail);
  if (n == 2) {      /* no EVERY: nothing may follow Y */
    if (sscanf(arg, "%f,%f%c", &e->x, &e->y, &tail) != 2) return -1;
    e->every = 1;
  } else if (n != 3) return -1;
  return cli_tracer_finite(e->x) && cli_tracer_finite(e->y) && e->every >= 1 ? 0 : -1;
}

/* a position euler_tracers_add takes on an X x Y grid */
static int cli_tracer_inside(float x, float y, int X, int Y) { return x >= 1.f && x < (float)(X - 1) && y >= 1.f && y < (float)(Y - 1); }

static const char k_tracers_header[] = "frame,time,index,x,y,path,age,wet_time,substeps,flags\n";
static int format_tracer_line(char* out, size_t cap, int frame, double time, size_t index, const euler_tracer* t) {
  return snprintf(out, cap, "%d,%.9g,%zu,%.9g,%.9g,%.9g,%.9g,%.9g,%u,%u\n", frame, time, index, (double)t->x, (double)t->y, (double)t->path, (double)t->age,
                  (double)t->wet_time, (unsigned)t->substeps, (unsigned)t->flags);
}
#endif
