// snapshot.hip — state snapshots (checkpoint / resume) for whole-grid AND row-slab handles, and euler_render on
// a row-slab handle.
//
// A snapshot is everything the reference keeps in file-scope variables (main.c:64-100, 204, 577): the four velocity fields, the
// five cell grids, g_precon, the marker array in order, the RNG state and the source latch - plus this build's frame counters.
// Little-endian; layouts documented in include/euler.h.
//   * a whole-grid handle writes ONE file (version 1, version 2 with the dye);
//   * a job of row slabs writes one PART file per rank (version 3: the rank's own rows, its markers WITH their keys = their
//     positions in the reference's array) and, rank 0, a small manifest under the given name listing the ranks' band ranges;
//   * euler_save_session (at the end of this file) writes version 4: the layout of version 1 / 2 followed by tagged chunks for the state this build added to the
//     reference's.  The loader below takes the core of such a file and passes its chunks through the checksum unread.
// Loading is independent of how the state was written: any handle - whole grid, or a slab of ANY partition - takes its rows
// (ghost rows included: the files of a job hold every row) and the markers inside its rows from whichever files hold them.  So a
// 3-rank job can be resumed on 2 ranks, or on one GPU, or with another (fluid-balanced) partition: the re-partitioning of a run
// whose water has moved is save + load.
#include "euler_dev.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

int eu_set_source_count(euler_sim* S, size_t nsrc);   // driver.hip

static uint64_t snap_fnv(uint64_t h, const void* p, size_t n) {
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}
struct SnapHeader {
  char magic[8]; uint32_t version; int32_t X, Y; uint32_t reserved;
  uint64_t n_markers, rng_state; int32_t source_exhausted; int32_t reserved2;
  uint64_t frames, total_substeps, total_pcg_iterations;
};
struct SlabHeader {      // follows SnapHeader in a version 3 part file
  int32_t nranks, rank, band_lo, band_hi, row_lo, row_hi;
  uint64_t n_loc;
};
struct ManifestHeader { char magic[8]; uint32_t version; int32_t X, Y, nranks; };   // then nranks x {int32 band_lo, band_hi}
static const int SNAP_F32[] = {EULER_F_U, EULER_F_V, EULER_F_UTMP, EULER_F_VTMP};
static const int SNAP_U8[] = {EULER_F_SOLID, EULER_F_SOURCE, EULER_F_SINK, EULER_F_COUNT, EULER_F_PREV_COUNT};
static const int SNAP_DYE[] = {EULER_F_DYE_R, EULER_F_DYE_G, EULER_F_DYE_B, EULER_F_DYE_RTMP, EULER_F_DYE_GTMP, EULER_F_DYE_BTMP};   // version 2 only

static std::string part_name(const char* path, int rank, int nranks) {
  char suffix[64];
  snprintf(suffix, sizeof suffix, ".%dof%d", rank, nranks);
  return std::string(path) + suffix;
}

// ------------------------------------------------------------------------------------------ save
// Files appear under their final names only when complete: every file is written under "<name>.tmp" and renamed.  Row slabs (collective): the ranks
// agree (one all-reduce of the status) that every part file was written and closed before any of them is renamed, and again that every rename
// succeeded before rank 0 puts the manifest in place - a manifest never names a part that is missing or belongs to an older state, and a rank
// that fails makes the call fail on every rank.
// chunks (a session file, version 4: whole-grid handles only): the bytes that follow the markers, under the same checksum
static int write_part_file(euler_sim* S, const euler_stats& st, const std::string& tmp, bool slab, int nranks, int rank, const std::vector<unsigned char>* chunks = nullptr) {
  FILE* f = fopen(tmp.c_str(), "wb");
  if (!f) { eu_set_error("cannot open %s for writing", tmp.c_str()); return EULER_EIO; }
  int rc = EULER_OK;
  SnapHeader h;
  memset(&h, 0, sizeof h);
  memcpy(h.magic, "EULERSNP", 8);
  h.version = slab ? 3 : (S->dye[0] ? 2 : 1); h.reserved = (slab && S->dye[0]) ? 1 : 0;      // (version 3 with the dye: reserved = 1)
  if (chunks) { h.version = 4; h.reserved = S->dye[0] ? 1 : 0; }
  h.X = S->X; h.Y = S->Y; h.n_markers = st.n_markers; h.rng_state = st.rng_state;
  h.source_exhausted = st.source_exhausted; h.frames = st.frames; h.total_substeps = st.total_substeps;
  h.total_pcg_iterations = st.total_pcg_iterations;
  uint64_t sum = snap_fnv(14695981039346656037ull, &h, sizeof h);
  bool ok = fwrite(&h, sizeof h, 1, f) == 1;
  const uint64_t n_loc = S->n_markers_host;      // exact: euler_get_stats synced the marker state
  if (slab) {
    SlabHeader sh;
    memset(&sh, 0, sizeof sh);
    sh.nranks = nranks; sh.rank = rank; sh.band_lo = S->band_lo; sh.band_hi = S->band_hi; sh.row_lo = S->row_lo; sh.row_hi = S->row_hi; sh.n_loc = n_loc;
    sum = snap_fnv(sum, &sh, sizeof sh);
    ok = ok && fwrite(&sh, sizeof sh, 1, f) == 1;
  }
  const size_t Cr = (size_t)(S->row_hi - S->row_lo) * S->X;      // cells of the own rows (the whole grid without slabs)
  std::vector<unsigned char> buf;
  try { buf.resize(Cr * 8 > n_loc * 8 ? Cr * 8 : (size_t)n_loc * 8); } catch (...) { fclose(f); return EULER_ENOMEM; }
  auto put = [&](int field, size_t bytes) {
    if (!ok || !bytes) return;
    rc = euler_get_field(S, field, buf.data(), bytes);
    if (rc) { ok = false; return; }
    sum = snap_fnv(sum, buf.data(), bytes);
    ok = fwrite(buf.data(), 1, bytes, f) == bytes;
  };
  for (int fd : SNAP_F32) put(fd, Cr * 4);
  for (int fd : SNAP_U8) put(fd, Cr);
  put(EULER_F_PRECON, Cr * 8);
  if (S->dye[0]) for (int fd : SNAP_DYE) put(fd, Cr * 4);
  put(EULER_F_MARKERS, (size_t)n_loc * 8);
  if (slab) put(EULER_F_MARKER_KEYS, (size_t)n_loc * 4);
  if (chunks && ok && !chunks->empty()) {
    sum = snap_fnv(sum, chunks->data(), chunks->size());
    ok = fwrite(chunks->data(), 1, chunks->size(), f) == chunks->size();
  }
  ok = ok && fwrite(&sum, 8, 1, f) == 1;
  ok = (fclose(f) == 0) && ok;
  if (rc) return rc;
  if (!ok) { eu_set_error("short write to %s", tmp.c_str()); return EULER_EIO; }
  return EULER_OK;
}

extern "C" int euler_save_state(euler_sim* S, const char* path) {
  if (!S || !path) return EULER_EINVAL;
  euler_stats st;
  int rc = euler_get_stats(S, &st);
  const bool slab = S->slab_on != 0;
  if (rc && !slab) return rc;
  const int nranks = slab ? S->cfg.slab_nranks : 1, rank = slab ? S->cfg.slab_rank : 0;
  const std::string file = slab ? part_name(path, rank, nranks) : std::string(path);
  const std::string tmp = file + ".tmp";
  if (!rc) rc = write_part_file(S, st, tmp, slab, nranks, rank);
  auto agree = [&](int local, const char* what) -> int {      // row slabs: non-zero on every rank if any rank failed
    if (!slab || !S->has_comm) return local;
    int worst = local;
    const int rc2 = eu_slab_status_sync(S, local, &worst);
    if (rc2) return rc2;
    if (worst && !local) eu_set_error("euler_save_state(%s): another rank failed to %s", path, what);
    return worst;
  };
  if ((rc = agree(rc, "write its part file"))) { remove(tmp.c_str()); return rc; }
  if (rename(tmp.c_str(), file.c_str()) != 0) { eu_set_error("cannot rename %s to %s", tmp.c_str(), file.c_str()); rc = EULER_EIO; }
  if ((rc = agree(rc, "put its part file in place"))) return rc;
  if (slab && rank == 0) {      // the manifest: which part holds which bands - last, and complete when it appears
    const std::string mtmp = std::string(path) + ".tmp";
    FILE* m = fopen(mtmp.c_str(), "wb");
    bool mok = m != nullptr;
    if (mok) {
      ManifestHeader mh;
      memset(&mh, 0, sizeof mh);
      memcpy(mh.magic, "EULERMAN", 8);
      mh.version = 3; mh.X = S->X; mh.Y = S->Y; mh.nranks = nranks;
      mok = fwrite(&mh, sizeof mh, 1, m) == 1;
      for (int r = 0; r < nranks && mok; ++r) { const int32_t b[2] = {S->part_lo[r], S->part_hi[r]}; mok = fwrite(b, sizeof b, 1, m) == 1; }
      mok = (fclose(m) == 0) && mok;
      mok = mok && rename(mtmp.c_str(), path) == 0;
    }
    if (!mok) { eu_set_error("cannot write the manifest %s", path); rc = EULER_EIO; }
  }
  return agree(rc, "write the manifest");
}

// ------------------------------------------------------------------------------------------ load
namespace {
struct Part {
  std::string file;
  const void* mem = nullptr;        // a session already in memory (euler_load_session): read from there, not from `file`
  size_t mem_n = 0;
  SnapHeader h;
  int row_lo, row_hi;               // rows the FILE holds
  int keep_lo, keep_hi;             // rows of it kept in memory: those the handle's window needs
  uint64_t n_loc;                   // markers in the file
  bool keyed;                       // version 3: markers carry keys; else a marker's key is its index
  // kept in memory: the rows [keep_lo, keep_hi) of every field section, and the markers whose row lies in [mark_lo, mark_hi) with their keys
  std::vector<unsigned char> sec[16];
  std::vector<float> mk;
  std::vector<unsigned int> keys;
  bool has_dye() const { return h.version == 2 || ((h.version == 3 || h.version == 4) && (h.reserved & 1u) == 1); }
  const unsigned char* rows(int k, int y) const { return sec[k].data() + (size_t)(y - keep_lo) * h.X * elem(k); }      // row y (kept) of section k
  static size_t elem(int k) { return k <= 3 ? 4 : (k <= 8 ? 1 : (k == 9 ? 8 : 4)); }      // 0..3 f32 fields, 4..8 u8 grids, 9 precon, 10..15 dye
};

// One pass over the file in 4 MB pieces: the checksum covers every byte, memory holds only what the handle needs - the rows of its window and the markers
// inside [mark_lo, mark_hi) - so a whole-grid snapshot of 16384^2 (7.8 GB + 2.7 GB of markers) loaded into eight row slabs costs each rank its own eighth,
// not the whole file.
int read_part(Part& p, int need_lo, int need_hi, int mark_lo, int mark_hi) {
  FILE* f = p.mem ? fmemopen(const_cast<void*>(p.mem), p.mem_n, "rb") : fopen(p.file.c_str(), "rb");
  if (!f) { eu_set_error("cannot open %s", p.file.c_str()); return EULER_EIO; }
  struct Closer { FILE* f; ~Closer() { fclose(f); } } closer{f};
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  if (n < (long)(sizeof(SnapHeader) + 8) || fread(&p.h, sizeof p.h, 1, f) != 1 || memcmp(p.h.magic, "EULERSNP", 8) != 0 || p.h.version < 1 || p.h.version > 4) {
    eu_set_error("%s is not an euler state snapshot (version 1, 2, 3 or 4)", p.file.c_str()); return EULER_EINVAL;
  }
  uint64_t sum = snap_fnv(14695981039346656037ull, &p.h, sizeof p.h);
  size_t body = sizeof(SnapHeader);
  p.row_lo = 0; p.row_hi = p.h.Y; p.n_loc = p.h.n_markers; p.keyed = false;
  if (p.h.version == 3) {
    SlabHeader sh;
    if ((size_t)n < sizeof(SnapHeader) + sizeof sh + 8 || fread(&sh, sizeof sh, 1, f) != 1) { eu_set_error("%s is truncated (slab header)", p.file.c_str()); return EULER_EIO; }
    sum = snap_fnv(sum, &sh, sizeof sh);
    body += sizeof sh;
    p.row_lo = sh.row_lo; p.row_hi = sh.row_hi; p.n_loc = sh.n_loc; p.keyed = true;
  }
  if (p.h.X <= 0 || p.row_hi < p.row_lo) { eu_set_error("%s: bad header", p.file.c_str()); return EULER_EINVAL; }
  const size_t X = (size_t)p.h.X, C = (size_t)(p.row_hi - p.row_lo) * X;
  const size_t want = body + C * 29 + (p.has_dye() ? C * 24 : 0) + (size_t)p.n_loc * (p.keyed ? 12 : 8) + 8;
  // (version 4, a session file: the chunks stand between the markers and the checksum; this loader passes them through the checksum and reads none)
  if (p.h.version == 4 ? (size_t)n < want : (size_t)n != want) { eu_set_error("%s is truncated or corrupt (size)", p.file.c_str()); return EULER_EIO; }
  const size_t chunk_bytes = (size_t)n - want;
  p.keep_lo = need_lo > p.row_lo ? need_lo : p.row_lo; p.keep_hi = need_hi < p.row_hi ? need_hi : p.row_hi;
  if (p.keep_hi < p.keep_lo) p.keep_hi = p.keep_lo;
  std::vector<unsigned char> chunk;
  try { chunk.resize((size_t)4 << 20); } catch (...) { return EULER_ENOMEM; }
  // a stretch of `bytes` bytes of the file; `sink(offset in the stretch, data, length)` sees every piece in order
  auto stream = [&](size_t bytes, auto&& sink) -> bool {
    for (size_t done = 0; done < bytes;) {
      const size_t len = bytes - done < chunk.size() ? bytes - done : chunk.size();
      if (fread(chunk.data(), 1, len, f) != len) return false;
      sum = snap_fnv(sum, chunk.data(), len);
      sink(done, chunk.data(), len);
      done += len;
    }
    return true;
  };
  const int nsec = p.has_dye() ? 16 : 10;
  for (int k = 0; k < nsec; ++k) {
    const size_t e = Part::elem(k), lo = (size_t)(p.keep_lo - p.row_lo) * X * e, hi = (size_t)(p.keep_hi - p.row_lo) * X * e;      // kept bytes of the section
    try { p.sec[k].resize(hi - lo); } catch (...) { return EULER_ENOMEM; }
    unsigned char* dst = p.sec[k].data();
    const bool ok = stream(C * e, [&](size_t off, const unsigned char* d, size_t len) {
      const size_t a = off > lo ? off : lo, b2 = off + len < hi ? off + len : hi;
      if (b2 > a) memcpy(dst + (a - lo), d + (a - off), b2 - a);
    });
    if (!ok) { eu_set_error("%s: short read", p.file.c_str()); return EULER_EIO; }
  }
  // markers: those whose row lies in [mark_lo, mark_hi); the indices kept decide which keys are kept from the stretch behind them
  std::vector<uint64_t> kept;
  unsigned char carry[8];
  size_t ncarry = 0;
  uint64_t mi = 0;
  bool oom = false;
  bool ok = stream((size_t)p.n_loc * 8, [&](size_t, const unsigned char* d, size_t len) {
    size_t pos = 0;
    while (pos < len && !oom) {
      float m[2];
      if (ncarry || len - pos < 8) {      // a marker split across two pieces
        const size_t take = 8 - ncarry < len - pos ? 8 - ncarry : len - pos;
        memcpy(carry + ncarry, d + pos, take); ncarry += take; pos += take;
        if (ncarry < 8) break;
        memcpy(m, carry, 8); ncarry = 0;
      } else { memcpy(m, d + pos, 8); pos += 8; }
      const int y = (int)floorf(m[1] / EU_H);
      if (y >= mark_lo && y < mark_hi) {
        try { p.mk.push_back(m[0]); p.mk.push_back(m[1]); kept.push_back(mi); } catch (...) { oom = true; }
      }
      ++mi;
    }
  });
  if (oom) return EULER_ENOMEM;
  if (!ok) { eu_set_error("%s: short read", p.file.c_str()); return EULER_EIO; }
  if (p.keyed) {
    size_t next = 0;
    try { p.keys.resize(kept.size()); } catch (...) { return EULER_ENOMEM; }
    ncarry = 0; mi = 0;
    ok = stream((size_t)p.n_loc * 4, [&](size_t, const unsigned char* d, size_t len) {      // (4 MB pieces are whole multiples of 4 bytes)
      for (size_t pos = 0; pos + 4 <= len; pos += 4, ++mi)
        if (next < kept.size() && kept[next] == mi) { memcpy(&p.keys[next], d + pos, 4); ++next; }
    });
    if (!ok) { eu_set_error("%s: short read", p.file.c_str()); return EULER_EIO; }
  } else {
    try { p.keys.resize(kept.size()); } catch (...) { return EULER_ENOMEM; }
    for (size_t i = 0; i < kept.size(); ++i) p.keys[i] = (unsigned int)kept[i];
  }
  if (chunk_bytes && !stream(chunk_bytes, [](size_t, const unsigned char*, size_t) {})) { eu_set_error("%s: short read", p.file.c_str()); return EULER_EIO; }
  uint64_t stored = 0;
  if (fread(&stored, 8, 1, f) != 1 || stored != sum) { eu_set_error("%s is truncated or corrupt (checksum)", p.file.c_str()); return EULER_EIO; }
  return EULER_OK;
}
}  // namespace

// everything of a load that is this rank's own business (files, host buffers, uploads): NO collective in here, so a failure leaves no other rank waiting
static int load_state_local(euler_sim* S, const char* path, SnapHeader* h_out, const void* mem = nullptr, size_t mem_n = 0) {
  // what is there: one whole-grid file, or a manifest naming the part files of a job
  std::vector<Part> parts;
  if (mem) {
    Part p;
    p.file = path; p.mem = mem; p.mem_n = mem_n; p.row_lo = 0; p.row_hi = S->Y;
    parts.push_back(p);
  } else {
    FILE* f = fopen(path, "rb");
    if (!f) { eu_set_error("cannot open %s", path); return EULER_EIO; }
    char magic[8] = {0};
    const bool got = fread(magic, 8, 1, f) == 1;
    if (got && memcmp(magic, "EULERMAN", 8) == 0) {
      ManifestHeader mh;
      fseek(f, 0, SEEK_SET);
      if (fread(&mh, sizeof mh, 1, f) != 1 || mh.version != 3 || mh.nranks < 1 || mh.nranks > 64) { fclose(f); eu_set_error("%s: bad manifest", path); return EULER_EINVAL; }
      for (int r = 0; r < mh.nranks; ++r) {
        int32_t b[2];
        if (fread(b, sizeof b, 1, f) != 1) { fclose(f); eu_set_error("%s: bad manifest", path); return EULER_EINVAL; }
        Part p;
        p.file = part_name(path, r, mh.nranks);
        p.row_lo = 64 * b[0]; p.row_hi = 64 * b[1] < mh.Y ? 64 * b[1] : mh.Y;      // (confirmed by the part's own header when it is read)
        parts.push_back(p);
      }
    } else {
      Part p;
      p.file = path; p.row_lo = 0; p.row_hi = S->Y;
      parts.push_back(p);
    }
    fclose(f);
  }
  // a handle needs the rows of its window (ghost rows included) and the markers inside its own rows: only the parts that overlap
  const int X = S->X, Y = S->Y;
  const int need_lo = S->slab_on ? S->win_lo : 0, need_hi = S->slab_on ? S->win_hi : Y;
  std::vector<Part*> use;
  for (Part& p : parts) {
    if (p.row_hi <= need_lo || p.row_lo >= need_hi) continue;
    int rc = read_part(p, need_lo, need_hi, S->slab_on ? S->row_lo : 0, S->slab_on ? S->row_hi : Y);
    if (rc) return rc;
    if (p.h.X != X || p.h.Y != Y) { eu_set_error("snapshot grid %dx%d does not fit this %dx%d handle", p.h.X, p.h.Y, X, Y); return EULER_EINVAL; }
    use.push_back(&p);
  }
  if (use.empty()) { eu_set_error("%s holds no rows of this handle", path); return EULER_EINVAL; }
  const SnapHeader& h0 = use[0]->h;
  const bool dye = use[0]->has_dye();
  if (dye != (S->dye[0] != nullptr)) {
    eu_set_error("%s %s the dye fields but this handle was created %s euler_config.rainbow", path, dye ? "carries" : "lacks", S->dye[0] ? "with" : "without");
    return EULER_EINVAL;
  }
  for (Part* p : use)
    if (p->h.n_markers != h0.n_markers || p->h.rng_state != h0.rng_state || p->h.frames != h0.frames) { eu_set_error("%s: the part files belong to different states", path); return EULER_EINVAL; }

  // ---- rows [need_lo, need_hi) of a field section from the parts
  const int rows = need_hi - need_lo;
  std::vector<unsigned char> buf((size_t)rows * X * 8);
  std::vector<char> have((size_t)rows);
  auto gather = [&](int section, int elem, int y0, int y1) -> bool {      // rows [y0, y1) -> buf
    std::fill(have.begin(), have.end(), 0);
    for (Part* p : use) {
      const int a = p->row_lo > y0 ? p->row_lo : y0, b = p->row_hi < y1 ? p->row_hi : y1;
      if (b <= a) continue;
      memcpy(buf.data() + (size_t)(a - y0) * X * elem, p->rows(section, a), (size_t)(b - a) * X * elem);
      for (int y = a; y < b; ++y) have[(size_t)(y - y0)] = 1;
    }
    for (int y = y0; y < y1; ++y) if (!have[(size_t)(y - y0)]) { eu_set_error("%s: row %d is in none of the part files", path, y); return false; }
    return true;
  };
  HIPCHK(hipStreamSynchronize(S->stream));
  float* f32[4] = {S->u, S->v, S->utmp, S->vtmp};
  uint8_t* u8[5] = {S->solid, S->source, S->sink, S->count, S->prev_count};
  for (int k = 0; k < 4; ++k) {
    if (!gather(k, 4, need_lo, need_hi)) return EULER_EINVAL;
    HIPCHK(hipMemcpy(f32[k] + (size_t)need_lo * X, buf.data(), (size_t)rows * X * 4, hipMemcpyHostToDevice));
  }
  size_t nsrc = 0;
  for (int k = 0; k < 5; ++k) {
    if (!gather(4 + k, 1, need_lo, need_hi)) return EULER_EINVAL;
    HIPCHK(hipMemcpy(u8[k] + (size_t)need_lo * X, buf.data(), (size_t)rows * X, hipMemcpyHostToDevice));
    if (k == 1) for (size_t i = (size_t)(S->row_lo - need_lo) * X; i < (size_t)(S->row_hi - need_lo) * X; ++i) nsrc += buf[i] != 0;
  }
  int rc = eu_set_source_count(S, nsrc);
  if (rc) return rc;
  if (!gather(9, 8, S->row_lo, S->row_hi)) return EULER_EINVAL;      // g_precon: the own rows, into the band-skewed array
  if ((rc = euler_set_field(S, EULER_F_PRECON, buf.data(), (size_t)(S->row_hi - S->row_lo) * X * 8))) return rc;
  if (dye)      // the window's rows (ghost rows included), like u and v
    for (int k = 0; k < 6; ++k) {
      if (!gather(10 + k, 4, need_lo, need_hi)) return EULER_EINVAL;
      HIPCHK(hipMemcpy(S->dye[k] + (size_t)need_lo * X, buf.data(), (size_t)rows * X * 4, hipMemcpyHostToDevice));
    }

  // ---- markers: those inside the own rows, with their keys (a whole-grid handle: all of them, ordered by key)
  std::vector<float> mk;
  std::vector<unsigned int> keys;
  uint64_t n_loc = 0;
  if (!S->slab_on) {
    if (h0.n_markers > S->max_markers) { eu_set_error("snapshot holds %llu markers, more than this handle's capacity", (unsigned long long)h0.n_markers); return EULER_EINVAL; }
    try { mk.resize(2 * (size_t)h0.n_markers + 2); } catch (...) { return EULER_ENOMEM; }
    std::vector<char> seen;
    try { seen.assign((size_t)h0.n_markers, 0); } catch (...) { return EULER_ENOMEM; }
    uint64_t placed = 0;
    for (Part* p : use) {
      const float* m = p->mk.data();
      const unsigned int* kk = p->keys.data();
      for (uint64_t i = 0; i < p->keys.size(); ++i) {
        const uint64_t key = kk[i];
        if (key >= h0.n_markers) { eu_set_error("%s: marker key %llu out of range", path, (unsigned long long)key); return EULER_EINVAL; }
        if (seen[(size_t)key]) { eu_set_error("%s: marker key %llu appears twice", path, (unsigned long long)key); return EULER_EINVAL; }
        seen[(size_t)key] = 1;
        mk[2 * key] = m[2 * i]; mk[2 * key + 1] = m[2 * i + 1];
        ++placed;
      }
    }
    if (placed != h0.n_markers) { eu_set_error("%s: the part files hold %llu of %llu markers", path, (unsigned long long)placed, (unsigned long long)h0.n_markers); return EULER_EINVAL; }
    if ((rc = euler_set_markers(S, mk.data(), h0.n_markers))) return rc;
    if ((rc = euler_set_rng(S, h0.rng_state, h0.source_exhausted))) return rc;
  } else {
    for (Part* p : use) {      // (read_part kept exactly the markers inside the own rows)
      mk.insert(mk.end(), p->mk.begin(), p->mk.end());
      keys.insert(keys.end(), p->keys.begin(), p->keys.end());
    }
    n_loc = keys.size();
    if (n_loc > S->max_markers) { eu_set_error("row slab %d: %llu markers in its rows, more than its capacity %zu", S->cfg.slab_rank, (unsigned long long)n_loc, S->max_markers); return EULER_ENOMEM; }
    if (n_loc) {
      HIPCHK(hipMemcpy(S->markers[S->cur], mk.data(), (size_t)n_loc * 8, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(S->keys[S->cur], keys.data(), (size_t)n_loc * 4, hipMemcpyHostToDevice));
    }
    MarkerState m0;
    memset(&m0, 0, sizeof m0);
    m0.n = h0.n_markers; m0.n_loc = n_loc; m0.max_markers = 4 * S->C; m0.rng_state = h0.rng_state; m0.exhausted = h0.source_exhausted;
    HIPCHK(hipMemcpy(S->ms, &m0, sizeof m0, hipMemcpyHostToDevice));
    S->n_markers_host = n_loc;
  }
  *h_out = h0;
  return EULER_OK;
}

static int load_state_finish(euler_sim* S, const SnapHeader& h0);

// Collective on a row-slab handle: every rank loads its rows and markers on its own, then the ranks AGREE on the outcome (one all-reduce of the
// status) before the first collective of the restore - a missing or corrupt part file, a row no file holds, more markers than a slab's capacity or
// an allocation failure on ONE rank fails the call on EVERY rank (the handle is then unloaded everywhere) instead of leaving the others waiting.
extern "C" int euler_load_state(euler_sim* S, const char* path) {
  if (!S || !path) return EULER_EINVAL;
  if (S->slab_on && !S->has_comm) { eu_set_error("row-slab handle: install the communicator before loading a snapshot"); return EULER_ESTATE; }
  SnapHeader h0;
  memset(&h0, 0, sizeof h0);
  int rc = load_state_local(S, path, &h0);
  if (S->slab_on) {
    int worst = rc;
    const int rc2 = eu_slab_status_sync(S, rc, &worst);
    if (rc2) return rc2;
    if (worst) {
      if (!rc) eu_set_error("euler_load_state(%s): another rank could not load its part of the state", path);
      S->loaded = 0;
      return rc ? rc : worst;
    }
    // every rank compared the headers of the part files IT read; ranks whose rows lie in different files must have seen the same state too (an overwrite that died between
    // the renames of the parts leaves old and new files side by side)
    const double id[4] = {(double)h0.frames, (double)(h0.rng_state & 0xffffffffull), (double)(h0.rng_state >> 32), (double)h0.n_markers};
    int same = 1;
    if ((rc = eu_slab_same_everywhere(S, id, 4, &same))) return rc;
    if (!same) { eu_set_error("euler_load_state(%s): the ranks read part files of different states (an interrupted overwrite?)", path); S->loaded = 0; return EULER_EINVAL; }
    if ((rc = eu_slab_after_restore(S))) return rc;      // collective: the source cells of all ranks
    if ((rc = eu_sync_marker_state(S))) return rc;
  } else if (rc) return rc;
  return load_state_finish(S, h0);
}

// behind the arrays and markers of a load: the validity flags, the counters, and the extras by the rules of a snapshot
static int load_state_finish(euler_sim* S, const SnapHeader& h0) {
  int rc;
  eu_vd_solver_arrays_foreign(&S->vd);      // the solver arrays may hold another state's pressure and masks: the next assembly writes them whole
  eu_vd_replaced(&S->vd);      // (the solid / sink grids were replaced)
  memset(&S->stats, 0, sizeof S->stats);
  S->stats.frames = h0.frames; S->stats.total_substeps = h0.total_substeps; S->stats.total_pcg_iterations = h0.total_pcg_iterations;
  S->time = 0.0;      // (the clock is no part of a snapshot and the forcing stays as set: the caller restores both, docs/forcing.md)
  S->n_tracers = 0;   // (tracers are no part of a snapshot either: docs/tracers.md)
  S->n_bodies = 0;    // (nor are the moving bodies: docs/bodies.md)
  if ((rc = eu_envelope_off(S))) return rc;      // (nor are the envelopes' planes, in a snapshot or in a session file: docs/envelope.md)
  if ((rc = eu_heat_reset(S))) return rc;      // (nor is the temperature: the record stays as set, the field starts from ambient, docs/heat.md)
  S->loaded = 1;
  return EULER_OK;
}

// ------------------------------------------------------------------------------------------ session files (version 4; include/euler.h, docs/session.md)
// The core of a snapshot followed by tagged chunks for everything else a whole-grid handle holds.  The chunks are composed, parsed and checked in plain C
// (euler_host.c: eu_session_put_chunks, eu_session_parse); this file gathers the handle's state for the composer and puts a parsed session into the handle.
// No kernel of its own: the core goes through the loader above, the heat field through euler_heat_set_field (its mask pass writes `ambient` over the dry
// cells: k_heat_mask serves where k_heat_dry would), everything else is host state or a plain copy.
static void session_settings(const euler_sim* S, eu_session_settings* t) {
  memset(t, 0, sizeof *t);
  t->max_iterations = S->cfg.max_iterations; t->dot_mode = S->cfg.dot_mode; t->precond = S->cfg.precond; t->tile_records = S->tile_w;
  t->sweep_mode = S->cfg.sweep_mode; t->max_substeps = S->cfg.max_substeps; t->rainbow = S->dye[0] ? 1 : 0; t->pcg_precision = S->cfg.pcg_precision;
  t->resident = S->cfg.resident; t->pcg_poll_interval = S->cfg.pcg_poll_interval;
  memcpy(&t->viscosity_bits, &S->cfg.viscosity, 4); memcpy(&t->frame_time_bits, &S->cfg.frame_time, 4);
  t->tol = S->cfg.tol;
  t->nopts = EULER_OPT__COUNT;
  for (int k = 1; k < EULER_OPT__COUNT; ++k) t->opt[k] = (int64_t)S->opt[k];
}
static_assert(EULER_OPT__COUNT <= EU_SESSION_OPTS, "the SETT chunk has room for every option key");
static_assert(sizeof(eu_session_settings) == 320 && offsetof(eu_session_settings, viscosity_bits) == 40 && offsetof(eu_session_settings, tol) == 48 &&
              offsetof(eu_session_settings, nopts) == 56 && offsetof(eu_session_settings, opt) == 64, "eu_session_settings is 320 bytes without padding");

static int session_enter(euler_sim* S, const char* path, const char* who) {
  if (!S || !path) { eu_set_error("%s: null argument", who); return EULER_EINVAL; }
  if (S->slab_on) { eu_set_error("%s: not on a row-slab handle (a slab holds none of what a session adds to a snapshot; euler_save_state / euler_load_state serve it)", who); return EULER_ESTATE; }
  return EULER_OK;
}

extern "C" int euler_save_session(euler_sim* S, const char* path) {
  const char* who = "euler_save_session";
  int rc = session_enter(S, path, who);
  if (rc) return rc;
  if (!S->loaded) { eu_set_error("%s: no scenario loaded", who); return EULER_ESTATE; }
  euler_stats st;
  if ((rc = euler_get_stats(S, &st))) return rc;      // (syncs the marker state: the reseed totals below are current)
  eu_session* s = (eu_session*)calloc(1, sizeof(eu_session));
  if (!s) return EULER_ENOMEM;
  struct Free { eu_session* s; ~Free() { free(s); } } guard{s};
  s->X = S->X; s->Y = S->Y; s->dye = S->dye[0] ? 1 : 0;
  s->time = S->time;
  s->forcing = S->forcing;
  if (S->forcing.nboxes > 0) memcpy(s->force_boxes, S->force_boxes, (size_t)S->forcing.nboxes * sizeof(euler_force_box));
  std::vector<float> field;
  std::vector<euler_tracer> tracers;
  try { if (S->heat_on) field.resize(S->C); tracers.resize(S->n_tracers); } catch (...) { return EULER_ENOMEM; }
  s->heat_on = S->heat_on ? 1 : 0;
  if (S->heat_on) {
    s->heat = S->heat;
    if (S->heat.nboxes > 0) memcpy(s->heat_boxes, S->heat_boxes, (size_t)S->heat.nboxes * sizeof(euler_heat_box));
    if ((rc = euler_heat_get_field(S, field.data(), S->C * sizeof(float)))) return rc;
    s->heat_field = (const unsigned char*)field.data();
  }
  s->n_tracers = S->n_tracers;
  if (S->n_tracers && (rc = euler_tracers_get(S, 0, S->n_tracers, tracers.data(), S->n_tracers * sizeof(euler_tracer)))) return rc;
  s->tracers = (const unsigned char*)tracers.data();
  s->n_bodies = S->n_bodies;
  for (int k = 0; k < S->n_bodies; ++k) { s->bodies[k] = S->bodies[k]; s->body_ox[k] = S->body_ox[k]; s->body_oy[k] = S->body_oy[k]; }
  if ((rc = euler_get_reseed(S, &s->reseed, &s->reseed_stats))) return rc;
  session_settings(S, &s->settings);
  s->last_substeps = st.last_substeps; s->last_pcg_iterations = st.last_pcg_iterations; s->last_residual = st.last_residual; s->last_dt = st.last_dt;
  s->marker_dt_events = st.marker_dt_events; s->marker_multi_events = st.marker_multi_events;
  std::vector<unsigned char> chunks;
  try { chunks.resize(eu_session_chunk_bytes(s)); } catch (...) { return EULER_ENOMEM; }
  (void)eu_session_put_chunks(s, chunks.data());
  const std::string tmp = std::string(path) + ".tmp";
  if ((rc = write_part_file(S, st, tmp, false, 1, 0, &chunks))) { remove(tmp.c_str()); return rc; }
  if (rename(tmp.c_str(), path) != 0) { eu_set_error("cannot rename %s to %s", tmp.c_str(), path); return EULER_EIO; }
  return EULER_OK;
}

extern "C" int euler_load_session(euler_sim* S, const char* path, uint32_t flags) {
  const char* who = "euler_load_session";
  int rc = session_enter(S, path, who);
  if (rc) return rc;
  if (flags & ~(uint32_t)EULER_SESSION_IGNORE_SETTINGS) { eu_set_error("%s: unknown flag bits %#x", who, flags); return EULER_EINVAL; }
  // ---- the whole file, read and checked before the handle changes
  std::vector<unsigned char> buf;
  {
    FILE* f = fopen(path, "rb");
    if (!f) { eu_set_error("cannot open %s", path); return EULER_EIO; }
    struct Closer { FILE* f; ~Closer() { fclose(f); } } closer{f};
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (n < 0) { eu_set_error("cannot read %s", path); return EULER_EIO; }
    try { buf.resize((size_t)n); } catch (...) { return EULER_ENOMEM; }
    if (n > 0 && fread(buf.data(), 1, (size_t)n, f) != (size_t)n) { eu_set_error("%s: short read", path); return EULER_EIO; }
  }
  eu_session* s = (eu_session*)calloc(1, sizeof(eu_session));
  if (!s) return EULER_ENOMEM;
  struct Free { eu_session* s; ~Free() { free(s); } } guard{s};
  char why[400];
  if ((rc = eu_session_parse(buf.data(), buf.size(), S->X, S->Y, S->dye[0] ? 1 : 0, S->max_markers, s, why, sizeof why))) { eu_set_error("%s(%s): %s", who, path, why); return rc; }
  if (!(flags & EULER_SESSION_IGNORE_SETTINGS)) {
    eu_session_settings mine;
    session_settings(S, &mine);
    if (eu_session_settings_diff(&s->settings, &mine, why, sizeof why)) {
      eu_set_error("%s(%s): the settings differ - %s (create the handle with the session's settings, or pass EULER_SESSION_IGNORE_SETTINGS)", who, path, why);
      return EULER_ESTATE;
    }
  }
  // ---- the device memory the extras need, while a failure still leaves the handle as it was (grow-only buffers: their contents stay)
  const bool reseed_on = s->reseed.thin_above != 0 || s->reseed.fill_holes != 0;
  if (s->heat_on && (rc = eu_devbuf_reserve(S, who, "the temperature and its scratch copy", &S->heat_buf, 2 * S->C * sizeof(float)))) return rc;
  if (s->n_tracers > S->tracer_buf.bytes / sizeof(euler_tracer)) {      // (the store's own policy: doubling from 256 records; nothing of the old records is kept)
    size_t cap = 256;
    while (cap < s->n_tracers) cap *= 2;
    if ((rc = eu_devbuf_reserve(S, who, "the tracers", &S->tracer_buf, cap * sizeof(euler_tracer)))) return rc;
  }
  if (reseed_on) {      // (what euler_set_reseed below would reserve)
    const size_t max_cells = (size_t)eu_reseed_limit(s->reseed.max_cells), max_fill = (size_t)eu_reseed_limit(s->reseed.max_fill);
    if ((rc = eu_devbuf_reserve(S, who, "the hole mask", &S->rs_mask_buf, ((S->C + 63) / 64 + 1) * sizeof(unsigned long long)))) return rc;
    if ((rc = eu_devbuf_reserve(S, who, "the cell list", &S->rs_cell_buf, max_cells * sizeof(unsigned int)))) return rc;
    if ((rc = eu_devbuf_reserve(S, who, "the sub-cell slots", &S->rs_slot_buf, 16 * max_cells * sizeof(unsigned int)))) return rc;
    if ((rc = eu_devbuf_reserve(S, who, "the draws", &S->rs_draw_buf, 2 * max_fill * sizeof(float)))) return rc;
  }
  // ---- the core, as euler_load_state restores it (from the bytes just checked, not from the file again)
  SnapHeader h0;
  memset(&h0, 0, sizeof h0);
  if ((rc = load_state_local(S, path, &h0, buf.data(), buf.size()))) return rc;
  S->heat_on = 0;      // (off unless the session says otherwise; load_state_finish then has no field to reset)
  if ((rc = load_state_finish(S, h0))) return rc;
  // ---- the extras, without the side effects of switching them on
  S->time = s->time;
  if ((rc = euler_set_forcing(S, &s->forcing, s->force_boxes))) return rc;      // (the record, the box table and what follows from the values: no grid is touched)
  if (s->heat_on) {
    // from off: any ambient passes, the arrays are there, the field is set to the session's ambient and then replaced; euler_heat_set_field writes ambient over
    // the cells without markers - for an honest file a no-op by the field's invariant
    if ((rc = euler_set_heat(S, &s->heat, s->heat_boxes))) return rc;
    std::vector<float> field;
    try { field.resize(S->C); } catch (...) { return EULER_ENOMEM; }
    memcpy(field.data(), s->heat_field, S->C * sizeof(float));
    if ((rc = euler_heat_set_field(S, field.data(), S->C * sizeof(float)))) return rc;
  }
  if (s->n_tracers) {      // the records byte for byte
    HIPCHK(hipMemcpyAsync(S->tracer_buf.p, s->tracers, (size_t)s->n_tracers * sizeof(euler_tracer), hipMemcpyHostToDevice, S->stream));
    HIPCHK(hipStreamSynchronize(S->stream));
  }
  S->n_tracers = (size_t)s->n_tracers;
  for (int k = 0; k < s->n_bodies; ++k) { S->bodies[k] = s->bodies[k]; S->body_ox[k] = s->body_ox[k]; S->body_oy[k] = s->body_oy[k]; }
  S->n_bodies = s->n_bodies;      // (the masks already hold the rectangles: no SOLID edit, no marker deleted)
  if ((rc = euler_set_reseed(S, &s->reseed))) return rc;      // (zeroes the totals ...)
  const unsigned long long totals[4] = {s->reseed_stats.removed, s->reseed_stats.added, s->reseed_stats.cells_thinned, s->reseed_stats.deferred};
  HIPCHK(hipMemcpyAsync(&S->ms->rs_removed, totals, sizeof totals, hipMemcpyHostToDevice, S->stream));      // (... which are the session's)
  const unsigned long long events[2] = {s->marker_dt_events, s->marker_multi_events};
  HIPCHK(hipMemcpyAsync(&S->ms->total_dt_events, events, sizeof events, hipMemcpyHostToDevice, S->stream));
  S->stats.last_substeps = s->last_substeps; S->stats.last_pcg_iterations = s->last_pcg_iterations; S->stats.last_residual = s->last_residual; S->stats.last_dt = s->last_dt;
  return eu_sync_marker_state(S);
}

// ------------------------------------------------------------------------------------------ render on a row-slab handle
// draw_rows (main.c:914-951) reads g_solid, g_sink, g_marker_count in the visible rows [max(Y-1-wy, 1), Y-1).  Collective: every
// rank contributes the visible rows it owns (an all-gather per grid, in place in a staging buffer), and every rank formats the same
// frame.  A terminal-sized window is a few dozen rows of the top slab; the call works for any window.
int eu_slab_render(euler_sim* S, int wx, int wy, char* out, int cap, int* len) {
  if (!S->has_comm) { eu_set_error("row-slab handle without a communicator"); return EULER_ESTATE; }
  const int X = S->X, Y = S->Y, R = S->cfg.slab_nranks;
  int cutoff = Y - 1 - wy;
  if (cutoff < 1) cutoff = 1;
  const int vis_lo = cutoff, vis_hi = Y - 1 > cutoff ? Y - 1 : cutoff, vrows = vis_hi - vis_lo;
  const bool dye = S->dye[0] != nullptr;
  // planes: solid, sink, count (bytes) and, with --rainbow, g_r, g_g, g_b (floats)
  const int nplanes = dye ? 6 : 3;
  const void* grids[6] = {S->solid, S->sink, S->count, S->dye[0], S->dye[1], S->dye[2]};
  const size_t elem[6] = {1, 1, 1, 4, 4, 4};
  size_t poff[7] = {0};
  for (int k = 0; k < nplanes; ++k) poff[k + 1] = poff[k] + (size_t)vrows * X * elem[k];
  uint8_t* stage = nullptr;
  HIPCHK(hipMalloc((void**)&stage, poff[nplanes] + 16));
  std::vector<int64_t> off(R), cnt(R);
  int rc = EULER_OK;
  for (int k = 0; k < nplanes && !rc && vrows > 0; ++k) {
    for (int r = 0; r < R; ++r) {
      const int lo = 64 * S->part_lo[r], hi = 64 * S->part_hi[r] < Y ? 64 * S->part_hi[r] : Y;
      const int a = lo > vis_lo ? lo : vis_lo, b = hi < vis_hi ? hi : vis_hi;
      off[r] = (int64_t)poff[k] + (b > a ? (int64_t)(a - vis_lo) * X * (int64_t)elem[k] : 0);
      cnt[r] = b > a ? (int64_t)(b - a) * X * (int64_t)elem[k] : 0;
      if (r == S->cfg.slab_rank && b > a)
        (void)hipMemcpyAsync(stage + off[r], static_cast<const char*>(grids[k]) + (size_t)a * X * elem[k], (size_t)cnt[r], hipMemcpyDeviceToDevice, S->stream);
    }
    if (S->bulk.allgather(S->bulk.ctx, stage, off.data(), cnt.data()) != 0) { eu_set_error("communicator callback failed: render all-gather"); rc = EULER_ECOMM; }
  }
  const size_t C = S->C;
  uint8_t* g = rc ? nullptr : (uint8_t*)calloc(3, C);      // (untouched pages of the full-size planes are never committed)
  float* col = (rc || !dye) ? nullptr : (float*)calloc(3 * C, sizeof(float));
  if (!rc && (!g || (dye && !col))) rc = EULER_ENOMEM;
  if (!rc) {
    for (int k = 0; k < nplanes && vrows > 0; ++k) {
      void* dst = k < 3 ? (void*)(g + (size_t)k * C + (size_t)vis_lo * X) : (void*)(col + (size_t)(k - 3) * C + (size_t)vis_lo * X);
      if (hipMemcpyAsync(dst, stage + poff[k], poff[k + 1] - poff[k], hipMemcpyDeviceToHost, S->stream) != hipSuccess) rc = EULER_EHIP;
    }
    if (hipStreamSynchronize(S->stream) != hipSuccess) rc = EULER_EHIP;
  }
  if (!rc) rc = dye ? euler_render_grids_rgb(g, g + C, g + 2 * C, col, col + C, col + 2 * C, X, Y, wx, wy, out, cap, len)
                    : euler_render_grids(g, g + C, g + 2 * C, X, Y, wx, wy, out, cap, len);
  free(g);
  free(col);
  (void)hipFree(stage);
  return rc;
}
