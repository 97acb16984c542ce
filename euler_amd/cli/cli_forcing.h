/*
 * cli_forcing.h — the host-only parts of `euler --gravity / --shake / --force` (docs/forcing.md): the parsers of the three specs.
 * In a header of their own so that tests/c/sanitize_forcing.c runs them under the sanitizers without the command's main().
 */
#ifndef EULER_CLI_FORCING_H
#define EULER_CLI_FORCING_H
#include <stdio.h>
#include <string.h>

#include "euler.h"

#define MAX_FORCE_BOXES EULER_FORCE_BOXES_MAX
#define CLI_DEG_TO_RAD (3.14159265358979323846 / 180.0)

/* a value euler_set_forcing takes: finite (a NaN fails both comparisons) and at most 1e4 in size */
static int cli_force_value(float v) { return v >= -1e4f && v <= 1e4f; }
static int cli_finite(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }

/* GX,GY -> f->gx, f->gy; -1: malformed (a missing or a trailing character) or out of range */
static int parse_gravity(const char* arg, euler_forcing* f) {
  float gx, gy;
  char tail;
  if (sscanf(arg, "%f,%f%c", &gx, &gy, &tail) != 2 || !cli_force_value(gx) || !cli_force_value(gy)) return -1;
  f->gx = gx; f->gy = gy;
  return 0;
}

/* SX,SY:HZ[:PHASE_DEG] -> the shake of f, the phase in radians; -1: malformed or out of range (HZ < 0 too) */
static int parse_shake(const char* arg, euler_forcing* f) {
  float sx, sy;
  double hz, deg = 0.0;
  char tail;
  const int n = sscanf(arg, "%f,%f:%lf:%lf%c", &sx, &sy, &hz, &deg, &tail);
  if (n == 3) {      /* no phase: nothing may follow HZ */
    if (sscanf(arg, "%f,%f:%lf%c", &sx, &sy, &hz, &tail) != 3) return -1;
  } else if (n != 4) return -1;
  if (!cli_force_value(sx) || !cli_force_value(sy) || !cli_finite(hz) || hz < 0.0 || !cli_finite(deg)) return -1;
  f->shake_x = sx; f->shake_y = sy; f->shake_hz = hz; f->shake_phase = deg * CLI_DEG_TO_RAD;
  return 0;
}

/* FX,FY:X0,Y0,X1,Y1 -> the box (checked against the grid later); -1: malformed or a force out of range */
static int parse_force(const char* arg, euler_force_box* b) {
  char tail;
  memset(b, 0, sizeof *b);
  if (sscanf(arg, "%f,%f:%d,%d,%d,%d%c", &b->fx, &b->fy, &b->x0, &b->y0, &b->x1, &b->y1, &tail) != 6) return -1;
  return cli_force_value(b->fx) && cli_force_value(b->fy) ? 0 : -1;
}
#endif
