/*
 * cli_bodies.h — the host-only part of `euler --body` (docs/bodies.md): the parser of the spec.
 * In a header of its own so that tests/c/sanitize_bodies.c runs it under the sanitizers without the command's main().
 */
#ifndef EULER_CLI_BODIES_H
#define EULER_CLI_BODIES_H
#include <stdio.h>
#include <string.h>

#include "euler.h"

#define MAX_BODIES EULER_BODIES_MAX
#define CLI_BODY_DEG_TO_RAD (3.14159265358979323846 / 180.0)

/* W,H:X,Y:VX,VY[:AX,AY:HZ[:DEG]] -> the body, the phase in radians; -1: malformed (a missing or a trailing character).  The values are euler_set_bodies' to refuse. */
static int parse_body(const char* arg, euler_body* b) {
  double deg = 0.0;
  char tail;
  memset(b, 0, sizeof *b);
  int n = sscanf(arg, "%d,%d:%lf,%lf:%f,%f:%f,%f:%lf:%lf%c", &b->w, &b->h, &b->x, &b->y, &b->vx, &b->vy, &b->amp_x, &b->amp_y, &b->hz, &deg, &tail);
  if (n == 6) {      /* no harmonic part: nothing may follow VY */
    if (sscanf(arg, "%d,%d:%lf,%lf:%f,%f%c", &b->w, &b->h, &b->x, &b->y, &b->vx, &b->vy, &tail) != 6) return -1;
  } else if (n == 9) {      /* no phase: nothing may follow HZ */
    if (sscanf(arg, "%d,%d:%lf,%lf:%f,%f:%f,%f:%lf%c", &b->w, &b->h, &b->x, &b->y, &b->vx, &b->vy, &b->amp_x, &b->amp_y, &b->hz, &tail) != 9) return -1;
  } else if (n != 10) return -1;
  b->phase = deg * CLI_BODY_DEG_TO_RAD;
  return 0;
}
#endif
