/*
 * euler — command-line front end over the C ABI of libeuler_hip.so.
 *
 * Mirrors the reference's program (main.c:961-1042): `euler [--rainbow] <scenario>` loads a scenario
 * text file, then loops  key -> step -> wait -> draw  at 10 frames per second.  On a terminal it behaves
 * like the reference: raw mode (misc/terminal.c:62-83), the window size from TIOCGWINSZ and SIGWINCH
 * (main.c:1004-1014), and the keys  p pause / f advance one frame while paused / r recolour the dye /
 * q quit  (main.c:961-980) with the pause gate of sim_step (main.c:844-846, 896-898).  Without a
 * terminal, or with --dump, it writes the frames as plain bytes (tests); --keys feeds the same key
 * handler one character per frame ('.' = no key) so that the gate is testable without a tty.
 *
 *   euler [--rainbow] [--size XxY] [--upscale] [--frames N] [--window WxH] [--dump] [--no-pace]
 *         [--keys STRING] [--resume FILE] [--checkpoint FILE] [--fit] [--view X0,Y0,X1,Y1] [--edit F:OP:X0,Y0,X1,Y1]...
 *         [--ppm PREFIX [--ppm-size WxH] [--ppm-every N] [--ppm-mode coverage|dye|speed:SCALE]] [--stats FILE [--stats-every N]]
 *         [--paint vorticity:S|pressure:S|speed:S] [--gauge level|pressure|force|flux:X0,Y0,X1,Y1]... [--gauges FILE [--gauges-every N]]
 *         [--gravity GX,GY] [--shake SX,SY:HZ[:PHASE_DEG]] [--force FX,FY:X0,Y0,X1,Y1]... [--body W,H:X,Y:VX,VY[:AX,AY:HZ[:DEG]]]...
 *         [--reseed THIN[:fill]] [--envelope CH[,CH...] [--envelope-out PREFIX] [--envelope-ppm PREFIX:S_ARRIVAL,S_WET,S_SPEED,S_PRESSURE]]
 *         [--tracer X,Y]... [--tracer-box X0,Y0,X1,Y1:K]... [--emit X,Y[:EVERY]]... [--tracers FILE [--tracers-every N]] [--tracers-show]
 *         [--session-out FILE [--session-every N]] [--session-in FILE] <scenario>
 * --resume continues from a state snapshot (include/euler.h) instead of the scenario's initial state
 * (the scenario argument may then be omitted); --checkpoint writes one after the last frame.
 * --fit draws the WHOLE interior fitted into the window (euler_render_fit: boxes of cells reduced on the device, docs/overview.md) instead of
 * one glyph per cell of the window's corner.  --ppm writes PREFIX%06d.ppm (binary P6) of the whole interior after every N-th frame (default 1;
 * frame 0 included), WxH boxes (default: the interior divided by the smallest integer that brings both sides to <= 1024), coloured by
 * coverage, by the dye (the default with --rainbow) or by speed (blue = 0 ... red = SCALE cells per second and above).
 * --view draws the box of interior cells [X0, X1] x [Y0, Y1] fitted into the window (euler_render_view, docs/viewport.md): boxes of cells where the box is
 * larger than the window, the markers' raster at 2 ... 16 glyphs per cell where the window holds it at least twice.  With it, and only with it, the keys
 * h j k l pan left / down / up / right by a quarter of the box (clamped to the interior), + halves the box about its centre (never below 4 x 4 cells),
 * - doubles it (clamped) and 0 shows the whole interior; --ppm then shows the box (--ppm-size clamped to it, the default divisor rule applied to it).
 * --fit --view is a usage error.
 * --edit (up to 64 times) edits the box of interior cells [X0, X1] x [Y0, Y1] and the markers in it on the device (euler_edit_box, docs/editing.md) right
 * before the step that produces frame F, in command-line order (F = 0: before frame 0 is drawn); OP is one of solid clear sink source fill drain.  A
 * malformed edit or a box outside the interior is a usage error.  With --view, and only with it, the keys X (solid) C (clear) S (sink) O (source) W (fill)
 * D (drain) edit the BRUSH: the viewed box shrunk about its centre to a quarter of its sides - with Bw = X1 - X0 + 1: w = max(1, Bw / 4), from
 * X0 + (Bw - w) / 2 on; the same in y.
 * --paint colours the frame of --fit / --view (both of its regimes) and the images of --ppm by a field of the flow raster (euler_flow_raster + euler_flow_paint,
 * docs/flow_raster.md) in place of the dye: the mean vorticity of a pixel from blue (-S) over white to red (+S), its mean pressure or the speed of its mean
 * velocity from blue (0) to red (S and above); the images are then written in the dye mode.  The pressure is reduced only for pressure:.  It needs --fit, --view
 * or --ppm: on its own it is a usage error.  With --view, and only with it, the key v cycles unpainted -> vorticity -> pressure -> speed at the scales given
 * or the defaults 1, 1000 and 10.
 * --heat AMBIENT:BETA[:KAPPA] switches the temperature on (euler_set_heat, docs/heat.md), set once behind the load and the forcing: the water starts at AMBIENT,
 * expands with BETA, diffuses with KAPPA (0 ... 2.5).  --heat-source T is what the scenario's source cells hold; --heat-box fix|rate:VALUE:X0,Y0,X1,Y1 (up to 64
 * times, in command-line order) holds the water of a box at VALUE or changes it at VALUE per second; --heat-init VALUE:X0,Y0,X1,Y1 (repeatable) sets the water of a
 * box to VALUE before frame 0 (euler_heat_fill).  --paint heat:S colours by the mean temperature of a pixel, from blue (AMBIENT - S) over white to red
 * (AMBIENT + S) (euler_heat_raster + euler_heat_paint); the key v does not cycle through it.  A malformed spec, a 65th box, a value out of range, a box
 * outside the interior, and --heat-source, --heat-box, --heat-init or --paint heat: without --heat are usage errors.  Without --heat every byte is as before.
 * --stats writes FILE (created or truncated) as CSV: a header line, then one line after every N-th frame (default 1; frame 0 included) with the frame's
 * solver figures (euler_get_stats) and the flow diagnostics of the whole interior (euler_diagnostics + euler_diag_derive, docs/diagnostics.md).
 * --gauge (up to 64 times) places an instrument on the box of interior cells [X0, X1] x [Y0, Y1]: level (extent of the fluid), pressure, force (on the solid
 * cells the box's fluid touches) or flux (through the right and top faces of its cells); --gauges writes FILE (created or truncated) as CSV: a header line,
 * then one line per gauge after every N-th frame (--gauges-every, default 1; frame 0 included), all gauges of a frame from ONE euler_gauges call
 * (docs/gauges.md).  --gauge without --gauges or the reverse, a malformed spec, a box outside the interior and a 65th gauge are usage errors.
 * --gravity, --shake and --force drive the tank (euler_set_forcing, docs/forcing.md), set once behind the load (also behind --resume: a snapshot records
 * neither the forcing nor the clock): the uniform acceleration (default 0,-10), a harmonic acceleration of the tank frame of amplitude SX,SY at HZ per second
 * of simulated time with the phase in degrees, and (up to 64 times) an acceleration FX,FY on the live faces of the cells of the box [X0, X1] x [Y0, Y1], in
 * command-line order.  A malformed spec, a 65th box, a box outside the interior and a value out of range (beyond 1e4 in size, not finite, HZ < 0) are usage
 * errors.  Without the three the forcing is never touched.
 * --body (up to 16 times, in command-line order) is a solid box of W x H cells with its lower-left corner at X,Y at t = 0 that moves at VX,VY cells per second plus
 * a harmonic part of amplitude AX,AY cells at HZ per second of simulated time with the phase in degrees, and pushes the water (euler_set_bodies, docs/bodies.md);
 * set once behind the load, the forcing and the heat.  A malformed spec, a 17th body and a value euler_set_bodies refuses exit with status 1.  Without it every
 * byte is as before.
 * --reseed THIN[:fill] switches the marker density control on (euler_set_reseed, docs/reseed.md) behind the load and the bodies: a cell whose count exceeds THIN
 * (4 ... 254) is thinned to one marker per quarter-cell square, with :fill a single-cell hole in the water gets a marker back; THIN = 0 with :fill fills only.  The
 * totals - markers removed and added, cells thinned, cells deferred - go on one line to stderr at exit.  A malformed spec is a usage error, a value
 * euler_set_reseed refuses exits with status 1.  Without it every byte is as before.
 * --envelope CH[,CH...] (CH one of arrival wet speed pressure all) switches the run-long envelopes on (euler_set_envelope, docs/envelope.md), set once behind the
 * load and all the other set-up: per cell the time the water first arrived, the time it stayed, the peak speed squared and the peak pressure, gathered at the end of
 * every substep.  --envelope-out PREFIX writes PREFIX.<channel>.f32 at exit, one file per enabled channel: the plane raw, little-endian, row-major, X * Y words;
 * --envelope-ppm PREFIX:S_ARRIVAL,S_WET,S_SPEED,S_PRESSURE writes PREFIX.<channel>.ppm at exit: the whole interior at min(X - 2, 1024) x min(Y - 2, 1024) pixels,
 * white to red over the channel's scale (seconds, seconds, cells per second, pressure), black where the water never was (euler_envelope_raster +
 * euler_envelope_rgb).  Both are written under .tmp and renamed.  A malformed spec and --envelope-out or --envelope-ppm without --envelope are usage errors.
 * Beside --session-in, --envelope is allowed: a session file does not carry the planes, so they start fresh.  Without the three every byte is as before.
 * --tracer (up to 1024 times) and --tracer-box (up to 64 times; the K x K lattice of every cell of the box, K = 1, 2 or 4) place passive tracers
 * (euler_tracers_add, docs/tracers.md), added once behind the load in command-line order.  --emit (up to 64 times) is a point that releases a tracer right before
 * the step that produces frame F whenever F % EVERY == 0 (default 1; F = 0 counts: before frame 0 is drawn) - a streakline; the emitters of a frame go in
 * command-line order in ONE euler_tracers_add and are silently skipped once the store is full.  --tracers writes FILE (created or truncated) as CSV: a header line, then
 * one line per tracer after every N-th frame (--tracers-every, default 1; frame 0 included).  --tracers-show paints the pixels that hold a live tracer yellow in the
 * frame of --fit / --view (both regimes) and the images of --ppm (euler_tracer_raster + euler_tracer_paint, behind any --paint; the other water pixels blue unless
 * --rainbow or --paint colour them; the images are then written in the dye mode); with --view, and only with it, the key t toggles it.  A malformed spec, a 1025th
 * tracer, a 65th box or emitter, a position or box outside the interior and --tracers-show without --fit, --view or --ppm are usage errors.
 * --session-out FILE writes a session file (euler_save_session, docs/session.md: the snapshot plus clock, forcing, heat, tracers, bodies, reseed record and totals)
 * after the last frame; with --session-every N also behind every N-th frame, to the same name (written as FILE.tmp and renamed: a reader never sees half a file).
 * --session-in FILE starts from a session instead of a scenario: the frame counter begins at the file's `frames` F0, so --edit F:..., --emit's schedule, the frame
 * columns of --stats / --gauges / --tracers, the numbers of --ppm and --frames N (absolute) continue, and from `--- frame F0` on the output is the uninterrupted
 * run's.  Frame F0 is drawn and logged as the saving run drew it; the edits and emitters of frames <= F0 are the saving run's and are not applied again.  What the
 * file carries cannot be given again: a scenario, --resume, --upscale, --gravity, --shake, --force, --heat*, --body, --reseed, --tracer and --tracer-box beside
 * --session-in are usage errors.  The settings (--size, --rainbow, --solver, --max-iterations, --advection, --maccormack) are given again and checked against the
 * file: a mismatch exits with status 1 and names the field.  --checkpoint and --resume are unchanged.
 */
#include <errno.h>
#include <signal.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/ioctl.h>
#include <termios.h>
#include <time.h>
#include <unistd.h>

#include "euler.h"
#include "cli_gauges.h"
#include "cli_forcing.h"
#include "cli_bodies.h"
#include "cli_reseed.h"
#include "cli_heat.h"
#include "cli_tracers.h"
#include "cli_session.h"
#include "cli_envelope.h"
#include "euler_host.h"      /* eu_tracer_lattice */

static void usage(const char* argv0) {
  fprintf(stderr, "usage: %s [--rainbow] [--size XxY] [--upscale] [--frames N] [--window WxH] [--dump] [--no-pace] [--keys STRING] "
                  "[--resume FILE] [--checkpoint FILE] [--solver reference|tile|tile-fp32|two-level|multilevel] [--max-iterations N] [--advection rk1|rk2] [--maccormack] "
                  "[--fit] [--view X0,Y0,X1,Y1] [--edit F:solid|clear|sink|source|fill|drain:X0,Y0,X1,Y1]... [--ppm PREFIX [--ppm-size WxH] [--ppm-every N] [--ppm-mode coverage|dye|speed:SCALE]] [--stats FILE [--stats-every N]] [--paint vorticity:S|pressure:S|speed:S|heat:S] [--gauge level|pressure|force|flux:X0,Y0,X1,Y1]... [--gauges FILE [--gauges-every N]] [--gravity GX,GY] [--shake SX,SY:HZ[:PHASE_DEG]] [--force FX,FY:X0,Y0,X1,Y1]... [--body W,H:X,Y:VX,VY[:AX,AY:HZ[:DEG]]]... [--reseed THIN[:fill]] [--envelope arrival|wet|speed|pressure|all[,...] [--envelope-out PREFIX] [--envelope-ppm PREFIX:S_ARRIVAL,S_WET,S_SPEED,S_PRESSURE]] [--heat AMBIENT:BETA[:KAPPA] [--heat-source T] [--heat-box fix|rate:VALUE:X0,Y0,X1,Y1]... [--heat-init VALUE:X0,Y0,X1,Y1]...] [--tracer X,Y]... [--tracer-box X0,Y0,X1,Y1:K]... [--emit X,Y[:EVERY]]... [--tracers FILE [--tracers-every N]] [--tracers-show] [--session-out FILE [--session-every N]] [--session-in FILE] <scenario>\n", argv0);
}

/* ---- terminal (misc/terminal.c) ------------------------------------------------------------ */
static struct termios g_orig_termios;
static int g_raw = 0;
static volatile sig_atomic_t g_resized = 0;

static void write_all(const char* s, size_t n) {
  while (n) {
    ssize_t k = write(STDOUT_FILENO, s, n);
    if (k < 0) { if (errno == EINTR) continue; return; }
    s += k; n -= (size_t)k;
  }
}
static void restore_terminal(void) {
  if (!g_raw) return;
  tcsetattr(STDIN_FILENO, TCSAFLUSH, &g_orig_termios);
  write_all("\x1b[?25h", 6);   /* show cursor */
  g_raw = 0;
}
static int enable_raw_mode(void) {
  if (tcgetattr(STDIN_FILENO, &g_orig_termios) == -1) return -1;
  struct termios raw = g_orig_termios;
  raw.c_iflag &= ~(tcflag_t)(BRKINT | ICRNL | INPCK | ISTRIP | IXON);
  raw.c_oflag &= ~(tcflag_t)(OPOST);
  raw.c_cflag |= (tcflag_t)(CS8);
  raw.c_lflag &= ~(tcflag_t)(ECHO | ICANON | IEXTEN | ISIG);
  raw.c_cc[VMIN] = 0;
  raw.c_cc[VTIME] = 0;
  if (tcsetattr(STDIN_FILENO, TCSAFLUSH, &raw) == -1) return -1;
  g_raw = 1;
  atexit(restore_terminal);
  return 0;
}
static void on_winch(int sig) { (void)sig; g_resized = 1; }
static int window_size(int* wx, int* wy) {
  struct winsize ws;
  if (ioctl(STDOUT_FILENO, TIOCGWINSZ, &ws) == -1 || ws.ws_col == 0) return -1;
  *wx = ws.ws_col; *wy = ws.ws_row;
  return 0;
}

/* ---- --ppm: the whole interior, or the box of --view, as a binary PPM (euler_overview / euler_overview_box + euler_overview_rgb) ---------------- */
/* --paint: the field of the flow raster over the box (NULL: the whole interior of xi x yi cells) and raster of the records px, painted into their dye sums */
static int paint_records(euler_sim* sim, const int* box, int xi, int yi, euler_overview_px* px, int W, int H, int field, double scale) {
  const size_t n = (size_t)W * (size_t)H;
  if (field == CLI_PAINT_HEAT) {      /* the temperature's raster and painter (docs/heat.md) */
    euler_heat h;
    euler_heat_px* hp = (euler_heat_px*)malloc(n * sizeof *hp);
    if (!hp) { fprintf(stderr, "--paint: out of memory\n"); return -1; }
    int rh = euler_get_heat(sim, &h, NULL, 0);
    if (rh == EULER_OK) rh = euler_heat_raster(sim, box ? box[0] : 1, box ? box[1] : 1, box ? box[2] : xi, box ? box[3] : yi, W, H, hp, n * sizeof *hp);
    if (rh != EULER_OK) fprintf(stderr, "%s\n", euler_last_error());
    else if ((rh = euler_heat_paint(hp, px, W, H, h.ambient, scale)) != EULER_OK) fprintf(stderr, "--paint: the heat records do not match the overview's\n");
    free(hp);
    return rh == EULER_OK ? 0 : -1;
  }
  euler_flow_px* fl = (euler_flow_px*)malloc(n * sizeof *fl);
  if (!fl) { fprintf(stderr, "--paint: out of memory\n"); return -1; }
  int rc = euler_flow_raster(sim, box ? box[0] : 1, box ? box[1] : 1, box ? box[2] : xi, box ? box[3] : yi, W, H, field == EULER_PAINT_PRESSURE ? EULER_FLOW_PRESSURE : 0, fl, n * sizeof *fl);
  if (rc != EULER_OK) fprintf(stderr, "%s\n", euler_last_error());
  else if ((rc = euler_flow_paint(fl, px, W, H, field, scale)) != EULER_OK) fprintf(stderr, "--paint: the flow records do not match the overview's\n");
  free(fl);
  return rc == EULER_OK ? 0 : -1;
}

/* --tracers-show: the tracer raster of the box (NULL: the whole interior) at the records' raster, painted into their dye sums; blue_rest: the other water pixels blue */
static int show_tracers(euler_sim* sim, const int* box, int xi, int yi, euler_overview_px* px, int W, int H, int blue_rest) {
  static const float fg[3] = {1.f, 0.9f, 0.f}, bg[3] = {0.25f, 0.5f, 1.f};
  const size_t n = (size_t)W * (size_t)H;
  uint32_t* counts = (uint32_t*)malloc(n * sizeof *counts);
  if (!counts) { fprintf(stderr, "--tracers-show: out of memory\n"); return -1; }
  int rc = euler_tracer_raster(sim, box ? box[0] : 1, box ? box[1] : 1, box ? box[2] : xi, box ? box[3] : yi, W, H, 0, counts, n * sizeof *counts);
  if (rc != EULER_OK) fprintf(stderr, "%s\n", euler_last_error());
  else if ((rc = euler_tracer_paint(counts, px, W, H, fg, blue_rest ? bg : NULL)) != EULER_OK) fprintf(stderr, "--tracers-show: the painter refused\n");
  free(counts);
  return rc == EULER_OK ? 0 : -1;
}

/* paint < 0: unpainted; else the records are painted with that field at pscale and the image is written in the dye mode */
static int write_ppm_frame(euler_sim* sim, const char* prefix, int frame, const int* box, int xi, int yi, int W, int H, int mode, float scale, int paint, double pscale, int show, int rainbow) {
  const size_t n = (size_t)W * (size_t)H;
  euler_overview_px* px = (euler_overview_px*)malloc(n * sizeof *px);
  uint8_t* rgb = (uint8_t*)malloc(n * 3);
  char* path = (char*)malloc(strlen(prefix) + 32);
  int ok = px && rgb && path;
  if (!ok) fprintf(stderr, "--ppm: out of memory\n");
  if (ok && (box ? euler_overview_box(sim, box[0], box[1], box[2], box[3], W, H, px, n * sizeof *px) : euler_overview(sim, W, H, px, n * sizeof *px)) != EULER_OK) {
    fprintf(stderr, "%s\n", euler_last_error());
    ok = 0;
  }
  if (ok && paint >= 0 && paint_records(sim, box, xi, yi, px, W, H, paint, pscale) != 0) ok = 0;
  if (ok && show && show_tracers(sim, box, xi, yi, px, W, H, !rainbow && paint < 0) != 0) ok = 0;
  if (ok && euler_overview_rgb(px, W, H, paint >= 0 || show ? EULER_IMAGE_DYE : mode, scale, rgb, n * 3) != EULER_OK) {
    fprintf(stderr, "%s\n", euler_last_error());
    ok = 0;
  }
  if (ok) {
    sprintf(path, "%s%06d.ppm", prefix, frame);
    FILE* f = fopen(path, "wb");
    ok = f && fprintf(f, "P6\n%d %d\n255\n", W, H) > 0 && fwrite(rgb, 1, n * 3, f) == n * 3;
    if (f && fclose(f) != 0) ok = 0;
    if (!ok) fprintf(stderr, "--ppm: cannot write %s: %s\n", path, strerror(errno));
  }
  free(px); free(rgb); free(path);
  return ok ? 0 : -1;
}

/* ---- --envelope-out, --envelope-ppm: the planes and their images at exit (docs/envelope.md) ---------------- */
static int write_envelopes(euler_sim* sim, uint32_t channels, int X, int Y, const char* out_prefix, const char* ppm_prefix, const double* scale) {
  const int W = X - 2 < 1024 ? X - 2 : 1024, H = Y - 2 < 1024 ? Y - 2 : 1024;
  const size_t cells = (size_t)X * (size_t)Y, n = (size_t)W * (size_t)H, plen = strlen(out_prefix ? out_prefix : "") + strlen(ppm_prefix ? ppm_prefix : "") + 32;
  float* plane = out_prefix ? (float*)malloc(cells * sizeof *plane) : NULL;
  euler_envelope_px* px = ppm_prefix ? (euler_envelope_px*)malloc(n * sizeof *px) : NULL;
  uint8_t* rgb = ppm_prefix ? (uint8_t*)malloc(n * 3) : NULL;
  char* path = (char*)malloc(plen);
  char head[64];
  int ok = path && (!out_prefix || plane) && (!ppm_prefix || (px && rgb));
  if (!ok) fprintf(stderr, "--envelope: out of memory\n");
  if (ok && ppm_prefix && euler_envelope_raster(sim, 1, 1, X - 2, Y - 2, W, H, px, n * sizeof *px) != EULER_OK) { fprintf(stderr, "%s\n", euler_last_error()); ok = 0; }
  for (int k = 0; ok && k < CLI_ENVELOPE_CHANNELS; ++k) {
    if (!(channels & (1u << k))) continue;
    if (out_prefix) {
      if (euler_envelope_get_field(sim, 1 << k, plane, cells * sizeof *plane) != EULER_OK) { fprintf(stderr, "%s\n", euler_last_error()); ok = 0; break; }
      if (cli_envelope_path(path, plen, out_prefix, k, "f32") != 0 || cli_envelope_write(path, NULL, plane, cells * sizeof *plane) != 0) {
        fprintf(stderr, "--envelope-out: cannot write %s: %s\n", path, strerror(errno)); ok = 0; break;
      }
    }
    if (ppm_prefix) {
      if (euler_envelope_rgb(px, W, H, 1 << k, scale[k], rgb, n * 3) != EULER_OK) { fprintf(stderr, "--envelope-ppm: the painter refused\n"); ok = 0; break; }
      snprintf(head, sizeof head, "P6\n%d %d\n255\n", W, H);
      if (cli_envelope_path(path, plen, ppm_prefix, k, "ppm") != 0 || cli_envelope_write(path, head, rgb, n * 3) != 0) {
        fprintf(stderr, "--envelope-ppm: cannot write %s: %s\n", path, strerror(errno)); ok = 0; break;
      }
    }
  }
  free(plane); free(px); free(rgb); free(path);
  return ok ? 0 : -1;
}

/* ---- --stats: one CSV line per frame (euler_get_stats + euler_diagnostics of the whole interior + euler_diag_derive) ---------------- */
static const char k_stats_header[] = "frame,substeps,pcg_iterations,residual,fluid,markers,count_max,crowded,max_div,mean_abs_div,kinetic_energy,com_x,com_y,nonfinite\n";
static int write_stats_line(euler_sim* sim, FILE* out, const char* path, int frame, int X, int Y) {
  euler_stats st;
  euler_diag d;
  euler_diag_values v;
  if (euler_get_stats(sim, &st) != EULER_OK || euler_diagnostics(sim, 1, 1, X - 2, Y - 2, &d, sizeof d) != EULER_OK || euler_diag_derive(&d, &v) != EULER_OK) {
    fprintf(stderr, "%s\n", euler_last_error());
    return -1;
  }
  const int ok = fprintf(out, "%d,%d,%d,%.9g,%llu,%llu,%u,%llu,%.9g,%.9g,%.9g,%.9g,%.9g,%u\n", frame, (int)st.last_substeps, (int)st.last_pcg_iterations, st.last_residual,
                         (unsigned long long)d.fluid, (unsigned long long)d.markers, (unsigned)d.count_max, (unsigned long long)d.crowded, (double)d.max_div, v.mean_abs_div,
                         v.kinetic_energy, v.com_x, v.com_y, (unsigned)d.nonfinite) > 0 && fflush(out) == 0;
  if (!ok) fprintf(stderr, "--stats: cannot write %s: %s\n", path, strerror(errno));
  return ok ? 0 : -1;
}

/* ---- --gauges: one CSV line per gauge and frame, all gauges of a frame from one euler_gauges call (docs/gauges.md) ---------------- */
static int write_gauge_lines(euler_sim* sim, FILE* out, const char* path, int frame, const euler_gauge* g, int n) {
  euler_gauge_rec rec[MAX_GAUGES];
  char line[512];
  if (euler_gauges(sim, g, n, rec, (size_t)n * sizeof *rec) != EULER_OK) { fprintf(stderr, "%s\n", euler_last_error()); return -1; }
  int ok = 1;
  for (int k = 0; ok && k < n; ++k) {
    const int len = format_gauge_line(line, sizeof line, frame, k, g[k].kind, rec + k);
    ok = len > 0 && (size_t)len < sizeof line && fputs(line, out) >= 0;
  }
  ok = ok && fflush(out) == 0;
  if (!ok) fprintf(stderr, "--gauges: cannot write %s: %s\n", path, strerror(errno));
  return ok ? 0 : -1;
}

/* ---- --tracers: one CSV line per tracer and frame (euler_tracers_get, docs/tracers.md) ---------------- */
static int write_tracer_lines(euler_sim* sim, FILE* out, const char* path, int frame) {
  size_t n = 0;
  double t = 0.0;
  char line[256];
  if (euler_tracers_count(sim, &n) != EULER_OK || euler_get_time(sim, &t) != EULER_OK) { fprintf(stderr, "%s\n", euler_last_error()); return -1; }
  euler_tracer* rec = (euler_tracer*)malloc((n ? n : 1) * sizeof *rec);
  if (!rec) { fprintf(stderr, "--tracers: out of memory\n"); return -1; }
  if (euler_tracers_get(sim, 0, n, rec, n * sizeof *rec) != EULER_OK) { fprintf(stderr, "%s\n", euler_last_error()); free(rec); return -1; }
  int ok = 1;
  for (size_t k = 0; ok && k < n; ++k) {
    const int len = format_tracer_line(line, sizeof line, frame, t, k, rec + k);
    ok = len > 0 && (size_t)len < sizeof line && fputs(line, out) >= 0;
  }
  ok = ok && fflush(out) == 0;
  if (!ok) fprintf(stderr, "--tracers: cannot write %s: %s\n", path, strerror(errno));
  free(rec);
  return ok ? 0 : -1;
}
/* --emit: the emitters due at frame f, in command-line order, in one euler_tracers_add; those the store has no room for are skipped */
static int emit_tracers(euler_sim* sim, const cli_emitter* e, int n, int f) {
  float xy[2 * MAX_EMITTERS];
  size_t m = 0, have = 0;
  if (euler_tracers_count(sim, &have) != EULER_OK) { fprintf(stderr, "%s\n", euler_last_error()); return -1; }
  for (int k = 0; k < n; ++k)
    if (f % e[k].every == 0 && have + m < EULER_TRACERS_MAX) { xy[2 * m] = e[k].x; xy[2 * m + 1] = e[k].y; ++m; }
  if (m && euler_tracers_add(sim, xy, m) != EULER_OK) { fprintf(stderr, "%s\n", euler_last_error()); return -1; }
  return 0;
}
/* --tracer / --tracer-box: everything placed on the command line, in its order, in one euler_tracers_add behind the load */
static int add_seeds(euler_sim* sim, const cli_seed* s, int n) {
  size_t total = 0;
  for (int k = 0; k < n; ++k) total += s[k].k ? eu_tracer_lattice(s[k].box[0], s[k].box[1], s[k].box[2], s[k].box[3], s[k].k, NULL) : 1;
  if (!total) return 0;
  if (total > EULER_TRACERS_MAX) { fprintf(stderr, "--tracer-box: %zu tracers (at most %u)\n", total, (unsigned)EULER_TRACERS_MAX); return -1; }
  float* xy = (float*)malloc(total * 2 * sizeof *xy);
  if (!xy) { fprintf(stderr, "--tracer: out of memory\n"); return -1; }
  size_t m = 0;
  for (int k = 0; k < n; ++k) {
    if (s[k].k) m += eu_tracer_lattice(s[k].box[0], s[k].box[1], s[k].box[2], s[k].box[3], s[k].k, xy + 2 * m);
    else { xy[2 * m] = s[k].x; xy[2 * m + 1] = s[k].y; ++m; }
  }
  const int rc = euler_tracers_add(sim, xy, total);
  if (rc != EULER_OK) fprintf(stderr, "%s\n", euler_last_error());
  free(xy);
  return rc == EULER_OK ? 0 : -1;
}

/* ---- the reference's loop state (main.c:85-88) ----------------------------------------------- */
typedef struct app {
  euler_sim* sim;
  int pause;                    /* g_pause */
  unsigned temp_unpause;        /* g_temp_unpause_counter */
  int rainbow;
  int view;                     /* --view: the box below is drawn and the pan / zoom keys act on it */
  int box[4];                   /* x0, y0, x1, y1, inclusive, inside the interior */
  int xi, yi;                   /* the interior: X - 2, Y - 2 */
  int failed;                   /* a brush key's edit was refused */
  int paint;                    /* --paint / the key v: -1 unpainted, else EULER_PAINT_* */
  double paint_scale[4];        /* the scale of each field: the one given, else 1, 1000, 10; [CLI_PAINT_HEAT]: 10 */
  int show;                     /* --tracers-show / the key t: the pixels that hold a live tracer are painted */
} app_t;

/* ---- --paint: the frame of --fit / --view with the flow field in place of the dye (docs/flow_raster.md) ----------------------------------- */
static int parse_paint(const char* arg, int* field, double* scale) {
  static const char* const fmt[4] = {"vorticity:%lf%c", "pressure:%lf%c", "speed:%lf%c", "heat:%lf%c"};      /* EULER_PAINT_* in their order, then CLI_PAINT_HEAT */
  char tail;
  for (*field = 0; *field < 4; ++*field)
    if (sscanf(arg, fmt[*field], scale, &tail) == 1) return *scale > 0.0 && *scale <= 1.7976931348623157e308 ? 0 : -1;
  return -1;
}
/* what euler_render_fit (view = 0: b is the whole interior) and euler_render_view (view = 1) draw, from the same records painted; a malloc'd frame, NULL on failure */
static char* painted_frame(app_t* a, const int* b, int view, int wx, int wy, int32_t* len) {
  if (wx < 1 || wy < 1) { fprintf(stderr, "--paint: a window of %d x %d\n", wx, wy); return NULL; }
  const int bw = b[2] - b[0] + 1, bh = b[3] - b[1] + 1;
  int scale = 0;      /* euler_render_view's rule; 0: at or below one cell per glyph */
  if (view && (long long)bw * 2 <= wx && (long long)bh * 2 <= wy)
    for (scale = 16; (long long)bw * scale > wx || (long long)bh * scale > wy; scale >>= 1) {}
  const int W = scale ? bw : (wx < bw ? wx : bw), H = scale ? bh : (wy < bh ? wy : bh);
  const size_t n = (size_t)W * (size_t)H, rbytes = scale ? (size_t)bw * scale * bh * scale * sizeof(uint32_t) : 0;
  euler_overview_px* px = (euler_overview_px*)malloc(n * sizeof *px);
  uint32_t* ras = scale ? (uint32_t*)malloc(rbytes) : NULL;
  char* out = NULL;
  int ok = px && (!scale || ras);
  if (!ok) fprintf(stderr, "--paint: out of memory\n");
  if (ok && (euler_overview_box(a->sim, b[0], b[1], b[2], b[3], W, H, px, n * sizeof *px) != EULER_OK ||
             (scale && euler_marker_raster(a->sim, b[0], b[1], b[2], b[3], scale, ras, rbytes) != EULER_OK))) { fprintf(stderr, "%s\n", euler_last_error()); ok = 0; }
  if (ok && a->paint >= 0 && paint_records(a->sim, b, a->xi, a->yi, px, W, H, a->paint, a->paint_scale[a->paint]) != 0) ok = 0;
  if (ok && a->show && show_tracers(a->sim, b, a->xi, a->yi, px, W, H, !a->rainbow && a->paint < 0) != 0) ok = 0;
  for (int pass = 0; ok && pass < 2; ++pass) {      /* the sizing protocol: the length, then the bytes */
    const int32_t cap = pass ? *len : 0;
    if (pass && !(out = (char*)malloc((size_t)cap + 1))) { fprintf(stderr, "--paint: out of memory\n"); ok = 0; break; }
    if ((scale ? euler_view_text(px, ras, bw, bh, scale, 1, out, cap, len) : euler_overview_text(px, W, H, 1, out, cap, len)) != EULER_OK) { fprintf(stderr, "--paint: the frame formatter refused\n"); ok = 0; }
  }
  free(px); free(ras);
  if (!ok) { free(out); out = NULL; }
  return out;
}

/* ---- --edit and the brush keys: euler_edit_box (docs/editing.md) ------------------------------------------------------------------------ */
#define MAX_EDITS 64
typedef struct edit { int frame, op, box[4]; } edit_t;
static const char* const k_edit_ops[6] = {"solid", "clear", "sink", "source", "fill", "drain"};      /* EULER_EDIT_* in their order */
static int parse_edit(const char* arg, edit_t* e) {
  char op[8], tail;
  if (sscanf(arg, "%d:%7[a-z]:%d,%d,%d,%d%c", &e->frame, op, &e->box[0], &e->box[1], &e->box[2], &e->box[3], &tail) != 6 || e->frame < 0) return -1;
  for (e->op = 0; e->op < 6; ++e->op) if (!strcmp(op, k_edit_ops[e->op])) return 0;
  return -1;
}
static int apply_edit(euler_sim* sim, int op, const int* b) {
  if (euler_edit_box(sim, op, b[0], b[1], b[2], b[3]) == EULER_OK) return 0;
  fprintf(stderr, "%s\n", euler_last_error());
  return -1;
}

/* --view's keys: pan by a quarter of the box, halve / double it about its centre, all clamped to the interior [1, xi] x [1, yi] */
static void zoom_axis(int* lo, int* hi, int limit, int nw) {
  const int w = *hi - *lo + 1;
  int l = nw < w ? *lo + (w - nw) / 2 : *lo - (nw - w) / 2;
  if (l < 1) l = 1;
  if (l + nw - 1 > limit) l = limit - nw + 1;
  *lo = l; *hi = l + nw - 1;
}
static void view_key(app_t* a, char c) {
  int* b = a->box;
  const int bw = b[2] - b[0] + 1, bh = b[3] - b[1] + 1;
  const int dx = bw / 4 > 1 ? bw / 4 : 1, dy = bh / 4 > 1 ? bh / 4 : 1;
  int s;
  if (c == 'h') { s = dx < b[0] - 1 ? dx : b[0] - 1; b[0] -= s; b[2] -= s; }
  else if (c == 'l') { s = dx < a->xi - b[2] ? dx : a->xi - b[2]; b[0] += s; b[2] += s; }
  else if (c == 'j') { s = dy < b[1] - 1 ? dy : b[1] - 1; b[1] -= s; b[3] -= s; }
  else if (c == 'k') { s = dy < a->yi - b[3] ? dy : a->yi - b[3]; b[1] += s; b[3] += s; }
  else if (c == '+') {
    zoom_axis(&b[0], &b[2], a->xi, bw / 2 >= 4 ? bw / 2 : (bw < 4 ? bw : 4));
    zoom_axis(&b[1], &b[3], a->yi, bh / 2 >= 4 ? bh / 2 : (bh < 4 ? bh : 4));
  } else if (c == '-') {
    zoom_axis(&b[0], &b[2], a->xi, 2 * bw < a->xi ? 2 * bw : a->xi);
    zoom_axis(&b[1], &b[3], a->yi, 2 * bh < a->yi ? 2 * bh : a->yi);
  } else if (c == '0') { b[0] = 1; b[1] = 1; b[2] = a->xi; b[3] = a->yi; }
  else if (c == 'v') a->paint = a->paint >= EULER_PAINT_SPEED ? -1 : a->paint + 1;      /* unpainted -> vorticity -> pressure -> speed -> unpainted */
  else if (c == 't') a->show = !a->show;
  else if (c && strchr("XCSOWD", c)) {      /* the brush: the box shrunk about its centre to a quarter of its sides */
    static const int ops[6] = {EULER_EDIT_SOLID, EULER_EDIT_CLEAR, EULER_EDIT_SINK, EULER_EDIT_SOURCE, EULER_EDIT_FILL, EULER_EDIT_DRAIN};
    const int w = bw / 4 > 1 ? bw / 4 : 1, h = bh / 4 > 1 ? bh / 4 : 1;
    const int brush[4] = {b[0] + (bw - w) / 2, b[1] + (bh - h) / 2, b[0] + (bw - w) / 2 + w - 1, b[1] + (bh - h) / 2 + h - 1};
    if (apply_edit(a->sim, ops[strchr("XCSOWD", c) - "XCSOWD"], brush) != 0) a->failed = 1;
  }
}

/* process_keypress (main.c:961-980); returns 0 on 'q' */
static int handle_key(app_t* a, char c) {
  if (c == 'p') a->pause = !a->pause;
  else if (c == 'f') a->temp_unpause++;
  else if (c == 'r') { if (a->rainbow && euler_colorize(a->sim) != EULER_OK) fprintf(stderr, "%s\n", euler_last_error()); }
  else if (c == 'q') return 0;
  else if (a->view) view_key(a, c);
  return 1;
}

/* sim_step's gate (main.c:844-846, 896-898) around euler_step */
static int gated_step(app_t* a) {
  if (a->pause && a->temp_unpause == 0) return EULER_OK;
  int rc = euler_step(a->sim);
  if (a->temp_unpause) a->temp_unpause--;
  return rc;
}

int main(int argc, char** argv) {
  euler_config cfg;
  euler_config_default(&cfg);
  int upscale = 0, frames = -1, wx = 98, wy = 38, dump = 0, pace = 1, window_given = 0, advect_rk2 = 0, maccormack = 0;
  const char* scenario = NULL;
  const char* resume = NULL;
  const char* checkpoint = NULL;
  const char* keys = NULL;
  int fit = 0, ppm_w = 0, ppm_h = 0, ppm_every = 1, ppm_mode = -1;
  float ppm_scale = 1.f;
  const char* ppm = NULL;
  const char* stats = NULL;
  int stats_every = 1;
  euler_gauge gauge_list[MAX_GAUGES];
  int n_gauges = 0, gauges_every = 1;
  const char* gauges = NULL;
  int view = 0, vbox[4] = {0, 0, 0, 0};
  edit_t edits[MAX_EDITS];
  int n_edits = 0;
  int paint = -1;
  double paint_scale[4] = {1.0, 1000.0, 10.0, 10.0};
  euler_heat heat;
  euler_heat_box heat_boxes[MAX_HEAT_BOXES];
  cli_heat_init heat_inits[MAX_HEAT_INITS];
  int heat_given = 0, heat_extra = 0, n_heat_boxes = 0, n_heat_inits = 0;
  euler_heat_default(&heat);
  euler_forcing forcing;
  euler_force_box force_boxes[MAX_FORCE_BOXES];
  int forcing_given = 0, n_force_boxes = 0;
  euler_forcing_default(&forcing);
  euler_body bodies[MAX_BODIES];
  int n_bodies = 0;
  euler_reseed reseed;
  int reseed_given = 0;
  uint32_t envelope = 0;
  int envelope_given = 0;
  const char* envelope_out = NULL;
  static char envelope_ppm[4096];
  double envelope_scale[CLI_ENVELOPE_CHANNELS];
  int envelope_ppm_given = 0;
  static cli_seed seeds[MAX_CLI_TRACERS + MAX_TRACER_BOXES];
  cli_emitter emitters[MAX_EMITTERS];
  int n_seeds = 0, n_points = 0, n_tboxes = 0, n_emitters = 0, tracers_every = 1, tracers_show = 0;
  const char* tracers = NULL;
  const char* session_out = NULL;
  const char* session_in = NULL;
  int session_every = 0;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--size") && i + 1 < argc) { if (sscanf(argv[++i], "%dx%d", &cfg.X, &cfg.Y) != 2) { usage(argv[0]); return 1; } }
    else if (!strcmp(argv[i], "--window") && i + 1 < argc) { if (sscanf(argv[++i], "%dx%d", &wx, &wy) != 2) { usage(argv[0]); return 1; } window_given = 1; }
    else if (!strcmp(argv[i], "--frames") && i + 1 < argc) frames = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--rainbow")) cfg.rainbow = 1;                                                     /* main.c:992 */
    else if (!strcmp(argv[i], "--upscale")) upscale = 1;
    else if (!strcmp(argv[i], "--dump")) dump = 1;
    else if (!strcmp(argv[i], "--no-pace")) pace = 0;
    else if (!strcmp(argv[i], "--keys") && i + 1 < argc) keys = argv[++i];
    else if (!strcmp(argv[i], "--resume") && i + 1 < argc) resume = argv[++i];
    else if (!strcmp(argv[i], "--checkpoint") && i + 1 < argc) checkpoint = argv[++i];
    /* the pressure solver's preconditioner (include/euler.h EULER_PRECOND_*): `reference` (default) = main.c:577-627, bit-identical iterates;
     * the others reach the same pressure where the solve converges - `multilevel` in 30-60 iterations whatever the grid size, so with
     * --max-iterations lifted above the reference's 100 (main.c:735) a large grid is actually SOLVED each substep */
    else if (!strcmp(argv[i], "--solver") && i + 1 < argc) {
      const char* v = argv[++i];
      if (!strcmp(v, "reference")) cfg.precond = EULER_PRECOND_IC0;
      else if (!strcmp(v, "tile")) cfg.precond = EULER_PRECOND_IC0_TILE;
      else if (!strcmp(v, "tile-fp32")) { cfg.precond = EULER_PRECOND_IC0_TILE; cfg.pcg_precision = EULER_PCG_F32; cfg.dot_mode = EULER_DOT_TREE; }   /* solver vectors in float (resident solver: small grids) */
      else if (!strcmp(v, "two-level")) cfg.precond = EULER_PRECOND_IC0_TILE2;
      else if (!strcmp(v, "multilevel")) cfg.precond = EULER_PRECOND_IC0_TILE_MG;
      else { usage(argv[0]); return 1; }
    }
    /* transport (include/euler.h EULER_OPT_ADVECT_RK2): `rk1` (default) = the reference's forward Euler, `rk2` = the midpoint rule (docs/advection_rk2.md).
     * A snapshot does not record it: a --resume run passes it again */
    else if (!strcmp(argv[i], "--advection") && i + 1 < argc) {
      const char* v = argv[++i];
      if (!strcmp(v, "rk1")) advect_rk2 = 0;
      else if (!strcmp(v, "rk2")) advect_rk2 = 1;
      else { usage(argv[0]); return 1; }
    }
    /* include/euler.h EULER_OPT_ADVECT_MACCORMACK: the MacCormack correction with the clamp on top of either trace (docs/advection_maccormack.md); not recorded in a snapshot */
    else if (!strcmp(argv[i], "--maccormack")) maccormack = 1;
    /* the whole-domain overview (docs/overview.md) */
    else if (!strcmp(argv[i], "--fit")) fit = 1;
    /* the pan-and-zoom viewport (docs/viewport.md) */
    else if (!strcmp(argv[i], "--view") && i + 1 < argc) {
      char tail;
      if (sscanf(argv[++i], "%d,%d,%d,%d%c", &vbox[0], &vbox[1], &vbox[2], &vbox[3], &tail) != 4) { usage(argv[0]); return 1; }
      view = 1;
    }
    /* scripted edits of the running scene (docs/editing.md) */
    else if (!strcmp(argv[i], "--edit") && i + 1 < argc) { if (n_edits == MAX_EDITS || parse_edit(argv[++i], &edits[n_edits++]) != 0) { usage(argv[0]); return 1; } }
    else if (!strcmp(argv[i], "--ppm") && i + 1 < argc) ppm = argv[++i];
    else if (!strcmp(argv[i], "--ppm-size") && i + 1 < argc) { if (sscanf(argv[++i], "%dx%d", &ppm_w, &ppm_h) != 2 || ppm_w < 1 || ppm_h < 1) { usage(argv[0]); return 1; } }
    else if (!strcmp(argv[i], "--ppm-every") && i + 1 < argc) { ppm_every = atoi(argv[++i]); if (ppm_every < 1) { usage(argv[0]); return 1; } }
    else if (!strcmp(argv[i], "--ppm-mode") && i + 1 < argc) {
      const char* v = argv[++i];
      char tail;
      if (!strcmp(v, "coverage")) ppm_mode = EULER_IMAGE_COVERAGE;
      else if (!strcmp(v, "dye")) ppm_mode = EULER_IMAGE_DYE;
      else if (sscanf(v, "speed:%f%c", &ppm_scale, &tail) == 1 && ppm_scale > 0.f) ppm_mode = EULER_IMAGE_SPEED;
      else { usage(argv[0]); return 1; }
    }
    /* a field of the flow raster in place of the dye (docs/flow_raster.md) */
    else if (!strcmp(argv[i], "--paint") && i + 1 < argc) {
      double sc;
      if (parse_paint(argv[++i], &paint, &sc) != 0) { usage(argv[0]); return 1; }
      paint_scale[paint] = sc;
    }
    /* the flow diagnostics as CSV (docs/diagnostics.md) */
    else if (!strcmp(argv[i], "--stats") && i + 1 < argc) stats = argv[++i];
    else if (!strcmp(argv[i], "--stats-every") && i + 1 < argc) { stats_every = atoi(argv[++i]); if (stats_every < 1) { usage(argv[0]); return 1; } }
    /* the batched gauges as CSV (docs/gauges.md) */
    else if (!strcmp(argv[i], "--gauge") && i + 1 < argc) { if (n_gauges == MAX_GAUGES || parse_gauge(argv[++i], &gauge_list[n_gauges++]) != 0) { usage(argv[0]); return 1; } }
    else if (!strcmp(argv[i], "--gauges") && i + 1 < argc) gauges = argv[++i];
    else if (!strcmp(argv[i], "--gauges-every") && i + 1 < argc) { gauges_every = atoi(argv[++i]); if (gauges_every < 1) { usage(argv[0]); return 1; } }
    /* forcing: gravity vector, shaken tank, force boxes (docs/forcing.md) */
    else if (!strcmp(argv[i], "--gravity") && i + 1 < argc) { if (parse_gravity(argv[++i], &forcing) != 0) { usage(argv[0]); return 1; } forcing_given = 1; }
    else if (!strcmp(argv[i], "--shake") && i + 1 < argc) { if (parse_shake(argv[++i], &forcing) != 0) { usage(argv[0]); return 1; } forcing_given = 1; }
    else if (!strcmp(argv[i], "--force") && i + 1 < argc) { if (n_force_boxes == MAX_FORCE_BOXES || parse_force(argv[++i], &force_boxes[n_force_boxes++]) != 0) { usage(argv[0]); return 1; } forcing_given = 1; }
    /* moving bodies (docs/bodies.md) */
    else if (!strcmp(argv[i], "--body") && i + 1 < argc) { if (n_bodies == MAX_BODIES || parse_body(argv[++i], &bodies[n_bodies++]) != 0) { usage(argv[0]); return 1; } }
    /* temperature: the record, the source cells' value, heat boxes in command-line order, fills of the start (docs/heat.md) */
    else if (!strcmp(argv[i], "--heat") && i + 1 < argc) { if (parse_heat(argv[++i], &heat) != 0) { usage(argv[0]); return 1; } heat_given = 1; }
    else if (!strcmp(argv[i], "--heat-source") && i + 1 < argc) { if (parse_heat_source(argv[++i], &heat.source_t) != 0) { usage(argv[0]); return 1; } heat_extra = 1; }
    else if (!strcmp(argv[i], "--heat-box") && i + 1 < argc) { if (n_heat_boxes == MAX_HEAT_BOXES || parse_heat_box(argv[++i], &heat_boxes[n_heat_boxes++]) != 0) { usage(argv[0]); return 1; } heat_extra = 1; }
    else if (!strcmp(argv[i], "--heat-init") && i + 1 < argc) { if (n_heat_inits == MAX_HEAT_INITS || parse_heat_init(argv[++i], &heat_inits[n_heat_inits++]) != 0) { usage(argv[0]); return 1; } heat_extra = 1; }
    /* passive tracers: points, lattices, emitters, the CSV and the painting (docs/tracers.md) */
    else if (!strcmp(argv[i], "--tracer") && i + 1 < argc) { if (n_points++ == MAX_CLI_TRACERS || parse_tracer(argv[++i], &seeds[n_seeds++]) != 0) { usage(argv[0]); return 1; } }
    else if (!strcmp(argv[i], "--tracer-box") && i + 1 < argc) { if (n_tboxes++ == MAX_TRACER_BOXES || parse_tracer_box(argv[++i], &seeds[n_seeds++]) != 0) { usage(argv[0]); return 1; } }
    else if (!strcmp(argv[i], "--emit") && i + 1 < argc) { if (n_emitters == MAX_EMITTERS || parse_emit(argv[++i], &emitters[n_emitters++]) != 0) { usage(argv[0]); return 1; } }
    else if (!strcmp(argv[i], "--tracers") && i + 1 < argc) tracers = argv[++i];
    else if (!strcmp(argv[i], "--tracers-every") && i + 1 < argc) { tracers_every = atoi(argv[++i]); if (tracers_every < 1) { usage(argv[0]); return 1; } }
    else if (!strcmp(argv[i], "--tracers-show")) tracers_show = 1;
    else if (!strcmp(argv[i], "--max-iterations") && i + 1 < argc) { cfg.max_iterations = atoi(argv[++i]); if (cfg.max_iterations < 1) { usage(argv[0]); return 1; } }
    /* marker density control (docs/reseed.md) */
    else if (!strcmp(argv[i], "--reseed") && i + 1 < argc) { if (parse_reseed(argv[++i], &reseed) != 0) { usage(argv[0]); return 1; } reseed_given = 1; }
    /* run-long envelopes (docs/envelope.md) */
    else if (!strcmp(argv[i], "--envelope") && i + 1 < argc) { if (parse_envelope(argv[++i], &envelope) != 0) { usage(argv[0]); return 1; } envelope_given = 1; }
    else if (!strcmp(argv[i], "--envelope-out") && i + 1 < argc) envelope_out = argv[++i];
    else if (!strcmp(argv[i], "--envelope-ppm") && i + 1 < argc) { if (parse_envelope_ppm(argv[++i], envelope_ppm, sizeof envelope_ppm, envelope_scale) != 0) { usage(argv[0]); return 1; } envelope_ppm_given = 1; }
    /* session files (docs/session.md) */
    else if (!strcmp(argv[i], "--session-out") && i + 1 < argc) session_out = argv[++i];
    else if (!strcmp(argv[i], "--session-every") && i + 1 < argc) { session_every = atoi(argv[++i]); if (session_every < 1) { usage(argv[0]); return 1; } }
    else if (!strcmp(argv[i], "--session-in") && i + 1 < argc) session_in = argv[++i];
    else if (argv[i][0] == '-') { fprintf(stderr, "Unrecognized input: %s\n", argv[i]); return 1; }   /* main.c:995 */
    else scenario = argv[i];
  }
  if (!scenario && !resume && !session_in) { usage(argv[0]); return 1; }                                        /* main.c:986-989 */
  if (session_every && !session_out) { usage(argv[0]); return 1; }
  if ((envelope_out || envelope_ppm_given) && !envelope_given) { usage(argv[0]); return 1; }
  if (session_in) {      /* what the file carries cannot be given again */
    const cli_session_clash clash = {scenario != NULL, resume != NULL, upscale, forcing_given, heat_given || heat_extra, n_bodies, reseed_given, n_seeds};
    const char* what = cli_session_conflict(&clash);
    if (what) { fprintf(stderr, "--session-in: %s comes from the session file\n", what); usage(argv[0]); return 1; }
  }

  if (view && (fit || vbox[0] < 1 || vbox[1] < 1 || vbox[2] > cfg.X - 2 || vbox[3] > cfg.Y - 2 || vbox[0] > vbox[2] || vbox[1] > vbox[3])) { usage(argv[0]); return 1; }
  for (int k = 0; k < n_edits; ++k) {
    const int* eb = edits[k].box;
    if (eb[0] < 1 || eb[1] < 1 || eb[2] > cfg.X - 2 || eb[3] > cfg.Y - 2 || eb[0] > eb[2] || eb[1] > eb[3]) { usage(argv[0]); return 1; }
  }
  if (paint >= 0 && !fit && !view && !ppm) { usage(argv[0]); return 1; }
  if ((n_gauges > 0) != (gauges != NULL)) { usage(argv[0]); return 1; }
  for (int k = 0; k < n_gauges; ++k) {
    const euler_gauge* gb = &gauge_list[k];
    if (gb->x0 < 1 || gb->y0 < 1 || gb->x1 > cfg.X - 2 || gb->y1 > cfg.Y - 2 || gb->x0 > gb->x1 || gb->y0 > gb->y1) { usage(argv[0]); return 1; }
  }
  for (int k = 0; k < n_force_boxes; ++k) {
    const euler_force_box* fb = &force_boxes[k];
    if (fb->x0 < 1 || fb->y0 < 1 || fb->x1 > cfg.X - 2 || fb->y1 > cfg.Y - 2 || fb->x0 > fb->x1 || fb->y0 > fb->y1) { usage(argv[0]); return 1; }
  }
  forcing.nboxes = n_force_boxes;
  if (!heat_given && (heat_extra || (paint == CLI_PAINT_HEAT && !session_in))) { usage(argv[0]); return 1; }      /* --heat-source, --heat-box, --heat-init, --paint heat: only with --heat */
  for (int k = 0; k < n_heat_boxes; ++k) {
    const euler_heat_box* hb = &heat_boxes[k];
    if (hb->x0 < 1 || hb->y0 < 1 || hb->x1 > cfg.X - 2 || hb->y1 > cfg.Y - 2 || hb->x0 > hb->x1 || hb->y0 > hb->y1) { usage(argv[0]); return 1; }
  }
  for (int k = 0; k < n_heat_inits; ++k) {
    const int* ib = heat_inits[k].box;
    if (ib[0] < 1 || ib[1] < 1 || ib[2] > cfg.X - 2 || ib[3] > cfg.Y - 2 || ib[0] > ib[2] || ib[1] > ib[3]) { usage(argv[0]); return 1; }
  }
  heat.nboxes = n_heat_boxes;
  for (int k = 0; k < n_seeds; ++k) {
    const int* tb = seeds[k].box;
    if (seeds[k].k ? (tb[0] < 1 || tb[1] < 1 || tb[2] > cfg.X - 2 || tb[3] > cfg.Y - 2 || tb[0] > tb[2] || tb[1] > tb[3]) : !cli_tracer_inside(seeds[k].x, seeds[k].y, cfg.X, cfg.Y)) { usage(argv[0]); return 1; }
  }
  for (int k = 0; k < n_emitters; ++k) if (!cli_tracer_inside(emitters[k].x, emitters[k].y, cfg.X, cfg.Y)) { usage(argv[0]); return 1; }
  if (tracers_show && !fit && !view && !ppm) { usage(argv[0]); return 1; }
  const int ppm_size_given = ppm_w > 0;
  if (ppm && view) {      /* the size follows the box frame by frame (below) */
    if (ppm_mode < 0) ppm_mode = cfg.rainbow ? EULER_IMAGE_DYE : EULER_IMAGE_COVERAGE;
  } else if (ppm) {
    const int xi = cfg.X - 2, yi = cfg.Y - 2;
    if (!ppm_w) {      /* the interior divided by the smallest integer that brings both sides to <= 1024 */
      int d = 1;
      while (xi / d > 1024 || yi / d > 1024) ++d;
      ppm_w = xi / d > 1 ? xi / d : 1; ppm_h = yi / d > 1 ? yi / d : 1;
    }
    if (ppm_w > xi || ppm_h > yi) { usage(argv[0]); return 1; }
    if (ppm_mode < 0) ppm_mode = cfg.rainbow ? EULER_IMAGE_DYE : EULER_IMAGE_COVERAGE;
  }
  int (*render)(euler_sim*, int32_t, int32_t, char*, int32_t, int32_t*) = fit ? euler_render_fit : euler_render;

  const int interactive = !dump && isatty(STDIN_FILENO) && isatty(STDOUT_FILENO);
  if (interactive && !window_given) {
    if (window_size(&wx, &wy) == -1) { perror("get_window_size"); return 1; }                                    /* main.c:1004-1008 */
    struct sigaction sa;
    sigemptyset(&sa.sa_mask);
    sa.sa_flags = 0;
    sa.sa_handler = on_winch;
    sigaction(SIGWINCH, &sa, 0);
  }

  app_t app;
  memset(&app, 0, sizeof app);
  app.rainbow = cfg.rainbow;
  app.view = view; app.xi = cfg.X - 2; app.yi = cfg.Y - 2;
  memcpy(app.box, vbox, sizeof vbox);
  app.paint = paint;
  memcpy(app.paint_scale, paint_scale, sizeof paint_scale);
  app.show = tracers_show;
  if (euler_create(&cfg, &app.sim) != EULER_OK || euler_set_option(app.sim, EULER_OPT_ADVECT_RK2, advect_rk2) != EULER_OK ||
      euler_set_option(app.sim, EULER_OPT_ADVECT_MACCORMACK, maccormack) != EULER_OK ||
      (session_in ? euler_load_session(app.sim, session_in, 0) : resume ? euler_load_state(app.sim, resume) : euler_load_scenario_file(app.sim, scenario, upscale)) != EULER_OK ||
      (forcing_given && euler_set_forcing(app.sim, &forcing, n_force_boxes ? force_boxes : NULL) != EULER_OK) ||
      (heat_given && euler_set_heat(app.sim, &heat, n_heat_boxes ? heat_boxes : NULL) != EULER_OK) ||      /* (behind the load and the forcing) */
      (n_bodies && euler_set_bodies(app.sim, bodies, n_bodies) != EULER_OK) ||
      (reseed_given && euler_set_reseed(app.sim, &reseed) != EULER_OK) ||
      (envelope_given && euler_set_envelope(app.sim, envelope) != EULER_OK)) {      /* (beside --session-in too: the file does not carry the planes, they start fresh) */
    fprintf(stderr, "%s\n", euler_last_error());
    return 1;
  }
  for (int k = 0; k < n_heat_inits; ++k)
    if (euler_heat_fill(app.sim, heat_inits[k].box[0], heat_inits[k].box[1], heat_inits[k].box[2], heat_inits[k].box[3], heat_inits[k].value) != EULER_OK) {
      fprintf(stderr, "%s\n", euler_last_error());
      return 1;
    }
  if (add_seeds(app.sim, seeds, n_seeds) != 0) return 1;
  const long long first = session_in ? cli_session_first_frame(app.sim) : 0;      /* a session continues its frame numbers */
  if (first < 0) { fprintf(stderr, "%s\n", euler_last_error()); return 1; }
  const int f0 = (int)first;
  if (interactive) {
    if (enable_raw_mode() == -1) { perror("failed to enable raw mode"); return 1; }
    write_all("\x1b[2J\x1b[H", 7);      /* clear_screen_now */
  }
  FILE* stats_file = NULL;
  int rc_exit = 0;
  if (stats) {
    stats_file = fopen(stats, "w");
    if (!stats_file || fputs(k_stats_header, stats_file) < 0 || fflush(stats_file) != 0) { fprintf(stderr, "--stats: cannot write %s: %s\n", stats, strerror(errno)); rc_exit = 1; }
  }
  FILE* gauges_file = NULL;
  if (gauges && !rc_exit) {
    gauges_file = fopen(gauges, "w");
    if (!gauges_file || fputs(k_gauges_header, gauges_file) < 0 || fflush(gauges_file) != 0) { fprintf(stderr, "--gauges: cannot write %s: %s\n", gauges, strerror(errno)); rc_exit = 1; }
  }
  FILE* tracers_file = NULL;
  if (tracers && !rc_exit) {
    tracers_file = fopen(tracers, "w");
    if (!tracers_file || fputs(k_tracers_header, tracers_file) < 0 || fflush(tracers_file) != 0) { fprintf(stderr, "--tracers: cannot write %s: %s\n", tracers, strerror(errno)); rc_exit = 1; }
  }
  int32_t cap = 0;
  char* buf = NULL;
  struct timespec next;
  clock_gettime(CLOCK_MONOTONIC, &next);
  size_t key_pos = 0;
  for (int f = f0; !rc_exit && (frames < 0 || f <= frames); ++f) {
    if (f > f0) {
      /* one key per frame: a scripted one (--keys) or whatever the terminal has (non-blocking read) */
      char c = '\0';
      if (keys) { if (keys[key_pos]) c = keys[key_pos++]; }
      else if (interactive) { if (read(STDIN_FILENO, &c, 1) == -1 && errno != EAGAIN && errno != EINTR) { perror("read"); rc_exit = 1; break; } }
      if (!handle_key(&app, c)) break;
      if (app.failed) { rc_exit = 1; break; }
      for (int k = 0; k < n_edits && !rc_exit; ++k) if (edits[k].frame == f && apply_edit(app.sim, edits[k].op, edits[k].box) != 0) rc_exit = 1;
      if (rc_exit) break;
      if (n_emitters && emit_tracers(app.sim, emitters, n_emitters, f) != 0) { rc_exit = 1; break; }
      if (gated_step(&app) != EULER_OK) { fprintf(stderr, "%s\n", euler_last_error()); rc_exit = 1; break; }
      if (pace && !dump) {                  /* 10 frames per second (main.c:1036, misc/time.c:17-32) */
        next.tv_nsec += 100000000L;
        if (next.tv_nsec >= 1000000000L) { next.tv_nsec -= 1000000000L; next.tv_sec += 1; }
        struct timespec now;
        clock_gettime(CLOCK_MONOTONIC, &now);
        if (now.tv_sec > next.tv_sec || (now.tv_sec == next.tv_sec && now.tv_nsec > next.tv_nsec)) next = now;   /* running late: no catch-up burst */
        else clock_nanosleep(CLOCK_MONOTONIC, TIMER_ABSTIME, &next, NULL);
      }
    }
    else if (!session_in) for (int k = 0; k < n_edits && !rc_exit; ++k) if (edits[k].frame == 0 && apply_edit(app.sim, edits[k].op, edits[k].box) != 0) rc_exit = 1;      /* before frame 0 is drawn */
    if (rc_exit) break;
    if (f == 0 && !session_in && n_emitters && emit_tracers(app.sim, emitters, n_emitters, 0) != 0) { rc_exit = 1; break; }
    if (g_resized) {                        /* handle_window_size_changed (main.c:1010-1014) */
      g_resized = 0;
      if (window_size(&wx, &wy) == 0) write_all("\x1b[2J\x1b[H", 7);
    }
    int32_t len = 0;
    const int* b = app.box;
    const int whole[4] = {1, 1, app.xi, app.yi};
    char* painted = NULL;      /* --paint / the key v: the frame of --fit / --view from the painted records */
    if ((app.paint >= 0 || app.show) && (fit || view) && !(painted = painted_frame(&app, view ? b : whole, view, wx, wy, &len))) { rc_exit = 1; break; }
#define RENDER(out, cap) (view ? euler_render_view(app.sim, b[0], b[1], b[2], b[3], wx, wy, (out), (cap), &len) : render(app.sim, wx, wy, (out), (cap), &len))
    if (painted) {}
    else if (RENDER(NULL, 0) != EULER_OK) { fprintf(stderr, "%s\n", euler_last_error()); rc_exit = 1; break; }
    if (!painted && len > cap) {
      cap = len + 4096;
      char* nb = (char*)realloc(buf, (size_t)cap);
      if (!nb) { rc_exit = 1; break; }
      buf = nb;
    }
    if (!painted && (RENDER(buf, cap) != EULER_OK || len > cap)) { fprintf(stderr, "%s\n", euler_last_error()); rc_exit = 1; break; }
    if (dump) {
      printf("--- frame %d (%d bytes)\n", f, (int)len);
      fwrite(painted ? painted : buf, 1, (size_t)len, stdout);
      printf("\n");
    } else {                               /* draw (main.c:953-959) */
      fflush(stdout);
      write_all("\x1b[H", 3);              /* reposition cursor */
      write_all(painted ? painted : buf, (size_t)len);
      write_all("\x1b[?25l", 6);           /* hide cursor */
    }
#undef RENDER
    free(painted);
    const int pf = app.paint;
    const double ps = pf >= 0 ? app.paint_scale[pf] : 0.0;
    if (ppm && view && f % ppm_every == 0) {      /* the box as it stands: --ppm-size clamped to it, else the divisor rule of the whole interior applied to it */
      const int bw = b[2] - b[0] + 1, bh = b[3] - b[1] + 1;
      int w = ppm_w < bw ? ppm_w : bw, h = ppm_h < bh ? ppm_h : bh;
      if (!ppm_size_given) {
        int d = 1;
        while (bw / d > 1024 || bh / d > 1024) ++d;
        w = bw / d > 1 ? bw / d : 1; h = bh / d > 1 ? bh / d : 1;
      }
      if (write_ppm_frame(app.sim, ppm, f, b, app.xi, app.yi, w, h, ppm_mode, ppm_scale, pf, ps, app.show, app.rainbow) != 0) { rc_exit = 1; break; }
    } else if (ppm && f % ppm_every == 0 && write_ppm_frame(app.sim, ppm, f, NULL, app.xi, app.yi, ppm_w, ppm_h, ppm_mode, ppm_scale, pf, ps, app.show, app.rainbow) != 0) { rc_exit = 1; break; }
    if (stats_file && f % stats_every == 0 && write_stats_line(app.sim, stats_file, stats, f, cfg.X, cfg.Y) != 0) { rc_exit = 1; break; }
    if (gauges_file && f % gauges_every == 0 && write_gauge_lines(app.sim, gauges_file, gauges, f, gauge_list, n_gauges) != 0) { rc_exit = 1; break; }
    if (tracers_file && f % tracers_every == 0 && write_tracer_lines(app.sim, tracers_file, tracers, f) != 0) { rc_exit = 1; break; }
    if (session_every && f > f0 && f % session_every == 0 && cli_session_save(app.sim, session_out) != 0) { rc_exit = 1; break; }
  }
  if (interactive) { write_all("\x1b[2J\x1b[H", 7); restore_terminal(); }
  if (stats_file && fclose(stats_file) != 0 && !rc_exit) { fprintf(stderr, "--stats: cannot write %s: %s\n", stats, strerror(errno)); rc_exit = 1; }
  if (tracers_file && fclose(tracers_file) != 0 && !rc_exit) { fprintf(stderr, "--tracers: cannot write %s: %s\n", tracers, strerror(errno)); rc_exit = 1; }
  if (gauges_file && fclose(gauges_file) != 0 && !rc_exit) { fprintf(stderr, "--gauges: cannot write %s: %s\n", gauges, strerror(errno)); rc_exit = 1; }
  if (!rc_exit && checkpoint && euler_save_state(app.sim, checkpoint) != EULER_OK) { fprintf(stderr, "%s\n", euler_last_error()); rc_exit = 1; }
  if (!rc_exit && session_out && cli_session_save(app.sim, session_out) != 0) rc_exit = 1;
  if (!rc_exit && (envelope_out || envelope_ppm_given) && write_envelopes(app.sim, envelope, cfg.X, cfg.Y, envelope_out, envelope_ppm_given ? envelope_ppm : NULL, envelope_scale) != 0) rc_exit = 1;
  euler_stats st;
  if (euler_get_stats(app.sim, &st) == EULER_OK)
    fprintf(stderr, "frames %llu substeps %llu pcg_iterations %llu markers %llu\n", (unsigned long long)st.frames,
            (unsigned long long)st.total_substeps, (unsigned long long)st.total_pcg_iterations, (unsigned long long)st.n_markers);
  euler_reseed_stats rs;
  if (reseed_given && euler_get_reseed(app.sim, NULL, &rs) == EULER_OK) (void)print_reseed_totals(stderr, &rs);
  free(buf);
  euler_destroy(app.sim);
  return rc_exit;
}
