/*
 * cli_session.h — `euler --session-out / --session-every / --session-in` (docs/session.md): which flags cannot stand beside --session-in, the frame a resumed run
 * begins with, and the write of a session.  In a header of its own beside the other cli_*.h.
 */
#ifndef EULER_CLI_SESSION_H
#define EULER_CLI_SESSION_H
#include <stdio.h>

#include "euler.h"

/* what the command line said about state that a session file carries; every non-zero word is a usage error beside --session-in */
typedef struct cli_session_clash {
  int scenario, resume, upscale, forcing, heat, bodies, reseed, seeds;
} cli_session_clash;
/* NULL: none; else the flag to name */
static const char* cli_session_conflict(const cli_session_clash* c) {
  if (c->scenario) return "a scenario file";
  if (c->resume) return "--resume";
  if (c->upscale) return "--upscale";
  if (c->forcing) return "--gravity / --shake / --force";
  if (c->heat) return "--heat / --heat-source / --heat-box / --heat-init";
  if (c->bodies) return "--body";
  if (c->reseed) return "--reseed";
  if (c->seeds) return "--tracer / --tracer-box";
  return NULL;
}

/* the frame counter a run from a session begins with: the file's `frames`; -1: the handle refused */
static long long cli_session_first_frame(euler_sim* sim) {
  euler_stats st;
  if (euler_get_stats(sim, &st) != EULER_OK || st.frames > 0x7fffffffull) return -1;
  return (long long)st.frames;
}

/* 0, or -1 with the library's message on stderr (the file appears under its name only when complete: written as FILE.tmp and renamed) */
static int cli_session_save(euler_sim* sim, const char* path) {
  if (euler_save_session(sim, path) == EULER_OK) return 0;
  fprintf(stderr, "%s\n", euler_last_error());
  return -1;
}
#endif
