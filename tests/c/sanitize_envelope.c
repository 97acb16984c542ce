/* sanitize_envelope.c - the host side of the run-long envelopes (docs/envelope.md) under ASan + UBSan, as a stand-alone program: the channel index, the checker of
 * the words euler_envelope_set_field accepts, euler_envelope_rgb's refusals and colours at the edges of its clamp, the --envelope and --envelope-ppm parsers, the file
 * names and the writer that renames.  Built and run by tests/test_envelope_host.py; prints "clean" when every check held. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "euler.h"
#include "euler_host.h"
#include "cli_envelope.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static uint32_t bits(float f) { uint32_t w; memcpy(&w, &f, sizeof w); return w; }

static void check_index_and_words(void) {
  CHECK(eu_envelope_index(EULER_ENV_ARRIVAL) == 0 && eu_envelope_index(EULER_ENV_WET) == 1 && eu_envelope_index(EULER_ENV_SPEED) == 2 && eu_envelope_index(EULER_ENV_PRESSURE) == 3);
  CHECK(eu_envelope_index(0) == -1 && eu_envelope_index(3) == -1 && eu_envelope_index(EULER_ENV_ALL) == -1 && eu_envelope_index(16) == -1 && eu_envelope_index(-1) == -1);
  const size_t none = (size_t)-1;
  /* exact-size heap blocks: a read past the end is the sanitizer's to find */
  const size_t n = 9;
  uint32_t* w = (uint32_t*)malloc(n * sizeof *w);
  if (!w) { ++failures; return; }
  const float good[9] = {0.f, 1.f, 1e-45f, 3.4028235e38f, 0.5f, 12.f, 7.25f, 100.f, 2.f};
  for (size_t k = 0; k < n; ++k) w[k] = bits(good[k]);
  const int chans[4] = {EULER_ENV_ARRIVAL, EULER_ENV_WET, EULER_ENV_SPEED, EULER_ENV_PRESSURE};
  for (int c = 0; c < 4; ++c) CHECK(eu_envelope_check_words(chans[c], w, n) == none);
  CHECK(eu_envelope_check_words(EULER_ENV_WET, w, 0) == none);
  /* "never" passes for the arrival alone */
  w[4] = 0xffffffffu;
  CHECK(eu_envelope_check_words(EULER_ENV_ARRIVAL, w, n) == none);
  for (int c = 1; c < 4; ++c) CHECK(eu_envelope_check_words(chans[c], w, n) == 4);
  /* the first bad index is named: -0.f, a negative, the infinities, NaNs of either sign */
  const uint32_t bad[7] = {0x80000000u, bits(-1.f), bits(INFINITY), bits(-INFINITY), 0x7fc00000u, 0xffc00000u, 0x7f800001u};
  for (int k = 0; k < 7; ++k)
    for (int c = 0; c < 4; ++c) {
      for (size_t j = 0; j < n; ++j) w[j] = bits(good[j]);
      w[8] = bad[k];
      CHECK(eu_envelope_check_words(chans[c], w, n) == 8);
      w[2] = bad[(k + 1) % 7];
      CHECK(eu_envelope_check_words(chans[c], w, n) == 2);
      CHECK(eu_envelope_check_words(chans[c], w, 2) == none);
    }
  free(w);
}

static void check_rgb(void) {
  enum { W = 3, H = 2 };
  euler_envelope_px* px = (euler_envelope_px*)calloc(W * H, sizeof *px);
  uint8_t* rgb = (uint8_t*)malloc(W * H * 3);
  if (!px || !rgb) { ++failures; free(px); free(rgb); return; }
  for (int k = 0; k < W * H; ++k) px[k].arrival_min = 0xffffffffu;
  /* pixel 1: reached at t = 0.5, wet 2 s, speed^2 16, p 50; pixel 2: the arrival channel off, a peak pressure alone; pixel 3: touched, everything 0;
   * pixel 4: beyond every scale; pixel 5: touched with a NaN word */
  px[1].cells = 4; px[1].touched = 2; px[1].arrival_min = bits(0.5f); px[1].arrival_max = bits(0.75f); px[1].wet_max = bits(2.f); px[1].speed2_max = bits(16.f); px[1].p_max = bits(50.f);
  px[2].cells = 4; px[2].p_max = bits(25.f);
  px[3].cells = 1; px[3].touched = 1; px[3].arrival_min = bits(0.f);
  px[4].cells = 1; px[4].touched = 1; px[4].arrival_min = bits(1e30f); px[4].wet_max = bits(INFINITY); px[4].speed2_max = bits(1e30f); px[4].p_max = bits(1e30f);
  px[5].cells = 1; px[5].touched = 1; px[5].arrival_min = 0x7fc00000u; px[5].p_max = 0x7fc00000u;
  memset(rgb, 7, W * H * 3);
  CHECK(euler_envelope_rgb(px, W, H, EULER_ENV_ARRIVAL, 1.0, rgb, W * H * 3) == EULER_OK);
  CHECK(rgb[0] == 0 && rgb[1] == 0 && rgb[2] == 0);                      /* never reached: black */
  CHECK(rgb[3] == 255 && rgb[4] == 127 && rgb[5] == 127);                /* t = 0.5: 255 * 0.5 = 127.5, truncated */
  CHECK(rgb[6] == 0 && rgb[7] == 0 && rgb[8] == 0);                      /* touched == 0 */
  CHECK(rgb[9] == 255 && rgb[10] == 255 && rgb[11] == 255);              /* reached at t = 0: white */
  CHECK(rgb[12] == 255 && rgb[13] == 0 && rgb[14] == 0);                 /* beyond the scale: red */
  CHECK(rgb[15] == 255 && rgb[16] == 255 && rgb[17] == 255);             /* a NaN: t = 0 */
  CHECK(euler_envelope_rgb(px, W, H, EULER_ENV_PRESSURE, 100.0, rgb, W * H * 3) == EULER_OK);
  CHECK(rgb[0] == 0 && rgb[3] == 255 && rgb[4] == 127);                  /* 50 / 100 */
  CHECK(rgb[6] == 255 && rgb[7] == 191 && rgb[8] == 191);                /* the arrival channel off: the extreme alone decides; 255 * 0.75 = 191.25 */
  CHECK(rgb[9] == 255 && rgb[10] == 255);                                /* touched, the extreme 0: white, not black */
  CHECK(rgb[12] == 255 && rgb[13] == 0);
  CHECK(euler_envelope_rgb(px, W, H, EULER_ENV_SPEED, 8.0, rgb, W * H * 3) == EULER_OK);
  CHECK(rgb[3] == 255 && rgb[4] == 127);                                 /* sqrt(16) / 8 */
  CHECK(rgb[6] == 0 && rgb[7] == 0);                                     /* untouched and no peak: black */
  CHECK(euler_envelope_rgb(px, W, H, EULER_ENV_WET, 4.0, rgb, W * H * 3) == EULER_OK);
  CHECK(rgb[3] == 255 && rgb[4] == 127 && rgb[13] == 0);
  /* the refusals leave rgb untouched */
  memset(rgb, 7, W * H * 3);
  CHECK(euler_envelope_rgb(NULL, W, H, EULER_ENV_WET, 1.0, rgb, W * H * 3) == EULER_EINVAL);
  CHECK(euler_envelope_rgb(px, W, H, EULER_ENV_WET, 1.0, NULL, W * H * 3) == EULER_EINVAL);
  CHECK(euler_envelope_rgb(px, 0, H, EULER_ENV_WET, 1.0, rgb, 0) == EULER_EINVAL);
  CHECK(euler_envelope_rgb(px, W, -1, EULER_ENV_WET, 1.0, rgb, W * H * 3) == EULER_EINVAL);
  CHECK(euler_envelope_rgb(px, W, H, 0, 1.0, rgb, W * H * 3) == EULER_EINVAL);
  CHECK(euler_envelope_rgb(px, W, H, 3, 1.0, rgb, W * H * 3) == EULER_EINVAL);
  CHECK(euler_envelope_rgb(px, W, H, EULER_ENV_ALL, 1.0, rgb, W * H * 3) == EULER_EINVAL);
  CHECK(euler_envelope_rgb(px, W, H, EULER_ENV_WET, 0.0, rgb, W * H * 3) == EULER_EINVAL);
  CHECK(euler_envelope_rgb(px, W, H, EULER_ENV_WET, -1.0, rgb, W * H * 3) == EULER_EINVAL);
  CHECK(euler_envelope_rgb(px, W, H, EULER_ENV_WET, NAN, rgb, W * H * 3) == EULER_EINVAL);
  CHECK(euler_envelope_rgb(px, W, H, EULER_ENV_WET, INFINITY, rgb, W * H * 3) == EULER_EINVAL);
  CHECK(euler_envelope_rgb(px, W, H, EULER_ENV_WET, 1.0, rgb, W * H * 3 - 1) == EULER_EINVAL);
  CHECK(euler_envelope_rgb(px, W, H, EULER_ENV_WET, 1.0, rgb, W * H * 3 + 1) == EULER_EINVAL);
  for (int k = 0; k < W * H * 3; ++k) CHECK(rgb[k] == 7);
  free(px); free(rgb);
}

static void check_parsers(void) {
  uint32_t ch = 99;
  CHECK(parse_envelope("all", &ch) == 0 && ch == EULER_ENV_ALL);
  CHECK(parse_envelope("arrival", &ch) == 0 && ch == EULER_ENV_ARRIVAL);
  CHECK(parse_envelope("wet,speed", &ch) == 0 && ch == (EULER_ENV_WET | EULER_ENV_SPEED));
  CHECK(parse_envelope("pressure,arrival,pressure", &ch) == 0 && ch == (EULER_ENV_PRESSURE | EULER_ENV_ARRIVAL));
  CHECK(parse_envelope("speed,all", &ch) == 0 && ch == EULER_ENV_ALL);
  ch = 99;
  const char* bad[] = {"", ",", "wet,", ",wet", "wet,,speed", "Wet", "wets", "we", "al", "alll", "wet speed", "wet;speed", "15", "arrival,pressur"};
  for (size_t k = 0; k < sizeof bad / sizeof *bad; ++k) CHECK(parse_envelope(bad[k], &ch) == -1 && ch == 99);

  char prefix[16];
  double s[CLI_ENVELOPE_CHANNELS];
  CHECK(parse_envelope_ppm("out/run:2,3.5,10,1e3", prefix, sizeof prefix, s) == 0 && !strcmp(prefix, "out/run") && s[0] == 2.0 && s[1] == 3.5 && s[2] == 10.0 && s[3] == 1000.0);
  CHECK(parse_envelope_ppm("a:b:1,1,1,1", prefix, sizeof prefix, s) == 0 && !strcmp(prefix, "a:b"));      /* cut at the LAST colon */
  CHECK(parse_envelope_ppm("123456789012345:1,1,1,1", prefix, sizeof prefix, s) == 0 && strlen(prefix) == 15);      /* the longest prefix that fits */
  const char* badp[] = {"", "p", ":1,1,1,1", "p:", "p:1,1,1", "p:1,1,1,1,1", "p:1,1,1,1x", "p:1,1,1,0", "p:-1,1,1,1", "p:1,nan,1,1", "p:1,1,inf,1", "p:1;1;1;1",
                        "1234567890123456:1,1,1,1", "p:1e999,1,1,1"};
  for (size_t k = 0; k < sizeof badp / sizeof *badp; ++k) CHECK(parse_envelope_ppm(badp[k], prefix, sizeof prefix, s) == -1);

  char path[24];
  CHECK(cli_envelope_path(path, sizeof path, "run", 0, "f32") == 0 && !strcmp(path, "run.arrival.f32"));
  CHECK(cli_envelope_path(path, sizeof path, "run", 3, "ppm") == 0 && !strcmp(path, "run.pressure.ppm"));
  CHECK(cli_envelope_path(path, sizeof path, "a-prefix-too-long", 3, "ppm") == -1);
}

static void check_writer(const char* dir) {
  char path[600], tmp[640];
  snprintf(path, sizeof path, "%s/plane.wet.f32", dir);
  snprintf(tmp, sizeof tmp, "%s.tmp", path);
  const float data[5] = {0.f, 1.5f, 2.f, 0.25f, 7.f};
  CHECK(cli_envelope_write(path, NULL, data, sizeof data) == 0);
  CHECK(access(tmp, F_OK) != 0);      /* renamed: no .tmp is left */
  float back[6];
  FILE* f = fopen(path, "rb");
  CHECK(f && fread(back, 1, sizeof back, f) == sizeof data && !memcmp(back, data, sizeof data));
  if (f) fclose(f);
  CHECK(cli_envelope_write(path, "P6\n1 1\n255\n", "abc", 3) == 0);      /* over an older file, with a head */
  char text[32];
  f = fopen(path, "rb");
  const size_t n = f ? fread(text, 1, sizeof text, f) : 0;
  CHECK(n == 14 && !memcmp(text, "P6\n1 1\n255\nabc", 14));
  if (f) fclose(f);
  remove(path);
  snprintf(path, sizeof path, "%s/no-such-directory/plane.f32", dir);
  CHECK(cli_envelope_write(path, NULL, data, sizeof data) == -1);
}

int main(int argc, char** argv) {
  check_index_and_words();
  check_rgb();
  check_parsers();
  check_writer(argc > 1 ? argv[1] : ".");
  if (failures) { fprintf(stderr, "sanitize_envelope: %d checks failed\n", failures); return 1; }
  printf("sanitize_envelope: clean\n");
  return 0;
}
