/*
 * cli_gauges.h — the host-only parts of `euler --gauge / --gauges` (docs/gauges.md): the parser of a gauge spec and the formatter of a CSV line.
 * In a header of their own so that tests/c/sanitize_gauges.c runs them under the sanitizers without the command's main().
 */
#ifndef EULER_CLI_GAUGES_H
#define EULER_CLI_GAUGES_H
#include <stdio.h>
#include <string.h>

#include "euler.h"

#define MAX_GAUGES 64
static const char* const k_gauge_kinds[4] = {"level", "pressure", "force", "flux"};      /* EULER_GAUGE_* in their order */
static const char k_gauges_header[] = "frame,gauge,kind,cells,fluid,lo_x,hi_x,lo_y,hi_y,terms,a,b,max_a,max_b,nonfinite\n";

/* KIND:X0,Y0,X1,Y1 -> the gauge; -1: malformed (an unknown kind, a missing or a trailing character) */
static int parse_gauge(const char* arg, euler_gauge* g) {
  char kind[10], tail;
  memset(g, 0, sizeof *g);
  if (sscanf(arg, "%9[a-z]:%d,%d,%d,%d%c", kind, &g->x0, &g->y0, &g->x1, &g->y1, &tail) != 5) return -1;
  for (g->kind = 0; g->kind < 4; ++g->kind) if (!strcmp(kind, k_gauge_kinds[g->kind])) return 0;
  return -1;
}

/* one line of the file into buf; the length it has (snprintf's: >= cap means cut short), negative on failure */
static int format_gauge_line(char* buf, size_t cap, int frame, int index, int kind, const euler_gauge_rec* r) {
  euler_gauge_values v;
  if (euler_gauge_derive(r, kind, &v) != EULER_OK) return -1;
  return snprintf(buf, cap, "%d,%d,%s,%u,%u,%u,%u,%u,%u,%u,%.9g,%.9g,%.9g,%.9g,%u\n", frame, index, k_gauge_kinds[kind], (unsigned)r->cells, (unsigned)r->fluid, (unsigned)r->lo_x,
                  (unsigned)r->hi_x, (unsigned)r->lo_y, (unsigned)r->hi_y, (unsigned)r->terms, v.a, v.b, (double)r->max_a, (double)r->max_b, (unsigned)r->nonfinite);
}
#endif
