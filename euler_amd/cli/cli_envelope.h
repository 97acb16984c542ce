/*
 * cli_envelope.h — the host-only part of `euler --envelope / --envelope-out / --envelope-ppm` (docs/envelope.md): the parsers of the specs, the names of the
 * files and the writer that puts a file down under `.tmp` and renames it.  In a header of its own so that tests/c/sanitize_envelope.c runs it under the sanitizers
 * without the command's main().
 */
#ifndef EULER_CLI_ENVELOPE_H
#define EULER_CLI_ENVELOPE_H
#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "euler.h"

#define CLI_ENVELOPE_CHANNELS 4
static const char* const k_cli_envelope_names[CLI_ENVELOPE_CHANNELS] = {"arrival", "wet", "speed", "pressure"};      /* bit k = 1 << k */

/* CH[,CH...], CH one of arrival | wet | speed | pressure | all -> the EULER_ENV_* bits.  -1: malformed (an empty item, another word, nothing at all) */
static int parse_envelope(const char* arg, uint32_t* channels) {
  uint32_t ch = 0;
  const char* p = arg;
  for (;;) {
    const char* e = strchr(p, ',');
    const size_t n = e ? (size_t)(e - p) : strlen(p);
    int k;
    if (n == 3 && !strncmp(p, "all", 3)) ch |= EULER_ENV_ALL;
    else {
      for (k = 0; k < CLI_ENVELOPE_CHANNELS; ++k)
        if (strlen(k_cli_envelope_names[k]) == n && !strncmp(p, k_cli_envelope_names[k], n)) break;
      if (k == CLI_ENVELOPE_CHANNELS) return -1;
      ch |= 1u << k;
    }
    if (!e) break;
    p = e + 1;
  }
  *channels = ch;
  return 0;
}

/* PREFIX:S_ARRIVAL,S_WET,S_SPEED,S_PRESSURE, cut at the LAST colon (a prefix may hold one) -> the prefix (at most cap - 1 characters) and the four scales, each
 * finite and > 0.  -1: malformed (no colon, an empty or over-long prefix, not four numbers, a trailing character, a scale out of range) */
static int parse_envelope_ppm(const char* arg, char* prefix, size_t cap, double scale[CLI_ENVELOPE_CHANNELS]) {
  const char* c = strrchr(arg, ':');
  if (!c || c == arg || (size_t)(c - arg) >= cap) return -1;
  char tail = 0;
  if (sscanf(c + 1, "%lf,%lf,%lf,%lf%c", &scale[0], &scale[1], &scale[2], &scale[3], &tail) != 4) return -1;
  for (int k = 0; k < CLI_ENVELOPE_CHANNELS; ++k) if (!isfinite(scale[k]) || !(scale[k] > 0.0)) return -1;
  memcpy(prefix, arg, (size_t)(c - arg));
  prefix[c - arg] = '\0';
  return 0;
}

/* PREFIX.<channel>.<ext> into out; -1: no room */
static int cli_envelope_path(char* out, size_t cap, const char* prefix, int k, const char* ext) {
  const int n = snprintf(out, cap, "%s.%s.%s", prefix, k_cli_envelope_names[k], ext);
  return n > 0 && (size_t)n < cap ? 0 : -1;
}

/* head (may be NULL) and bytes to path.tmp, then renamed to path: a reader never sees half a file.  -1 with errno set: it could not be written */
static int cli_envelope_write(const char* path, const char* head, const void* data, size_t bytes) {
  const size_t n = strlen(path) + 5;
  char* tmp = (char*)malloc(n);
  if (!tmp) { errno = ENOMEM; return -1; }
  snprintf(tmp, n, "%s.tmp", path);
  FILE* f = fopen(tmp, "wb");
  int ok = f != NULL;
  if (ok && head) ok = fputs(head, f) >= 0;
  if (ok) ok = fwrite(data, 1, bytes, f) == bytes;
  if (f && fclose(f) != 0) ok = 0;
  if (ok) ok = rename(tmp, path) == 0;
  const int e = errno;
  if (!ok && f) (void)remove(tmp);
  free(tmp);
  errno = e;
  return ok ? 0 : -1;
}
#endif
