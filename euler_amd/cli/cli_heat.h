/*
 * cli_heat.h — the host-only parts of `euler --heat / --heat-source / --heat-box / --heat-init` (docs/heat.md): the parsers of the specs.
 * In a header of their own so that tests/c/sanitize_heat.c runs them under the sanitizers without the command's main().
 */
#ifndef EULER_CLI_HEAT_H
#define EULER_CLI_HEAT_H
#include <stdio.h>
#include <string.h>

#include "euler.h"

#define MAX_HEAT_BOXES EULER_HEAT_BOXES_MAX
#define MAX_HEAT_INITS 64
#define CLI_PAINT_HEAT 3      /* --paint heat:S, behind the three EULER_PAINT_* fields of the flow raster */

typedef struct cli_heat_init { float value; int box[4]; } cli_heat_init;

/* a value euler_set_heat takes: finite (a NaN fails both comparisons) and at most 1e4 in size */
static int cli_heat_value(float v) { return v >= -1e4f && v <= 1e4f; }

/* AMBIENT:BETA[:KAPPA] -> h->ambient, h->beta, h->kappa (0 when left out); -1: malformed (a missing or a trailing character) or out of range */
static int parse_heat(const char* arg, euler_heat* h) {
  float amb, beta, kappa = 0.f;
  char tail;
  const int n = sscanf(arg, "%f:%f:%f%c", &amb, &beta, &kappa, &tail);
  if (n == 2) {      /* no kappa: nothing may follow BETA */
    if (sscanf(arg, "%f:%f%c", &amb, &beta, &tail) != 2) return -1;
  } else if (n != 3) return -1;
  if (!cli_heat_value(amb) || !cli_heat_value(beta) || !(kappa >= 0.f && kappa <= 2.5f)) return -1;
  h->ambient = amb; h->beta = beta; h->kappa = kappa;
  return 0;
}

/* T -> *t; -1: malformed or out of range */
static int parse_heat_source(const char* arg, float* t) {
  float v;
  char tail;
  if (sscanf(arg, "%f%c", &v, &tail) != 1 || !cli_heat_value(v)) return -1;
  *t = v;
  return 0;
}

/* fix|rate:VALUE:X0,Y0,X1,Y1 -> the box (checked against the grid later); -1: malformed, another kind or a value out of range */
static int parse_heat_box(const char* arg, euler_heat_box* b) {
  char tail;
  memset(b, 0, sizeof *b);
  if (!strncmp(arg, "fix:", 4)) { b->kind = EULER_HEAT_FIX; arg += 4; }
  else if (!strncmp(arg, "rate:", 5)) { b->kind = EULER_HEAT_RATE; arg += 5; }
  else return -1;
  if (sscanf(arg, "%f:%d,%d,%d,%d%c", &b->value, &b->x0, &b->y0, &b->x1, &b->y1, &tail) != 5) return -1;
  return cli_heat_value(b->value) ? 0 : -1;
}

/* VALUE:X0,Y0,X1,Y1 -> one euler_heat_fill (the box is checked against the grid later); -1: malformed or a value out of range */
static int parse_heat_init(const char* arg, cli_heat_init* f) {
  char tail;
  memset(f, 0, sizeof *f);
  if (sscanf(arg, "%f:%d,%d,%d,%d%c", &f->value, &f->box[0], &f->box[1], &f->box[2], &f->box[3], &tail) != 5) return -1;
  return cli_heat_value(f->value) ? 0 : -1;
}
#endif
