/*
 * cli_reseed.h — the host-only part of `euler --reseed` (docs/reseed.md): the parser of the spec and the line of totals.
 * In a header of its own so that tests/c/sanitize_reseed.c runs it under the sanitizers without the command's main().
 */
#ifndef EULER_CLI_RESEED_H
#define EULER_CLI_RESEED_H
#include <stdio.h>
#include <string.h>

#include "euler.h"

/* THIN[:fill] -> the record, the limits at their defaults; THIN = 0 with :fill is filling only.  -1: malformed (no number, a trailing character, another word than
 * `fill`).  The values are euler_set_reseed's to refuse. */
static int parse_reseed(const char* arg, euler_reseed* r) {
  int thin = 0, used = 0;
  memset(r, 0, sizeof *r);
  if (sscanf(arg, "%d%n", &thin, &used) != 1 || used < 1) return -1;
  if (arg[used] != '\0' && strcmp(arg + used, ":fill") != 0) return -1;
  r->thin_above = thin;
  r->fill_holes = arg[used] != '\0';
  return 0;
}

/* the four totals on one line; returns what fprintf returns */
static int print_reseed_totals(FILE* f, const euler_reseed_stats* s) {
  return fprintf(f, "reseed removed %llu added %llu cells_thinned %llu deferred %llu\n", (unsigned long long)s->removed, (unsigned long long)s->added,
                 (unsigned long long)s->cells_thinned, (unsigned long long)s->deferred);
}
#endif
