// k_reseed.hip — marker density control (include/euler.h euler_set_reseed, docs/reseed.md): one pass behind refresh_marker_counts that thins the cells whose count
// byte exceeds a bound down to one marker per quarter-cell square and puts one marker into every single-cell hole that tore open inside the water.
//
// The pass changes the marker array as the reference's own loops would: deleting is refresh_marker_counts' swap-with-last removal (main.c:105-116) over delete flags
// computed beforehand (k_compact_markers, shared with the refresh and the editor), appending is update_fluid_sources' order and draws (main.c:276-298) off the
// handle's one xorshift stream.  All launches are sized by what the host knows already (n_markers_host, the record's limits); what the device finds - K listed
// cells, D deletions, the holes - stays on the device, and every kernel behind such a number leaves at once when it is zero:
//   k_rs_cells    one pass over the cells: "count byte > thin_above" and "hole" balloted into two bit masks, row-major bit order
//   select        the crowded mask -> the ascending cell list (eu_ordered_select)
//   k_rs_plan     the first K = min(found, max_cells) cells into the pass's own list, their 16 K sub-cell slots cleared; the totals
//   k_rs_claim    the markers, two per lane: a marker of a listed cell finds the cell's rank by binary search and claims its sub-cell: atomicMin(slot, index)
//   k_rs_ballot   the markers again: "listed and not the claimant" balloted into the delete mask; then select, k_compact_markers
//   k_rs_counts   a thread per listed cell: count <- occupied slots; n -= D
//   select        the hole mask -> the ascending hole list
//   k_rs_fill_plan / k_rs_draws / k_rs_place   the source stage's three kernels without the latch: how many append, the draws in parallel, the markers
// Plain C++: vector loads and stores, 32-bit integer atomics.
#include "euler_dev.h"

#include <string.h>

#define RS_NONE 0xffffffffu      // an empty sub-cell slot

// ---- bit j of the low 16 -> bit 4 j: the four ballots of a lane's four cells interleave into a mask word
__device__ __forceinline__ unsigned long long rs_spread4(unsigned long long x) {
  x &= 0xffffull;
  x = (x | (x << 24)) & 0x000000ff000000ffull;
  x = (x | (x << 12)) & 0x000f000f000f000full;
  x = (x | (x << 6)) & 0x0303030303030303ull;
  x = (x | (x << 3)) & 0x1111111111111111ull;
  return x;
}
// bit k of the low 32 -> bit 2 k (two markers per lane: k_edit.hip ed_spread)
__device__ __forceinline__ unsigned long long rs_spread2(unsigned long long v) {
  v &= 0xffffffffull;
  v = (v | (v << 16)) & 0x0000ffff0000ffffull;
  v = (v | (v << 8)) & 0x00ff00ff00ff00ffull;
  v = (v | (v << 4)) & 0x0f0f0f0f0f0f0f0full;
  v = (v | (v << 2)) & 0x3333333333333333ull;
  v = (v | (v << 1)) & 0x5555555555555555ull;
  return v;
}

// the hole test of one interior candidate (count == 0 && prev_count != 0 already): no mask of its own, and every one of the eight neighbours wet or solid
__device__ __forceinline__ bool rs_is_hole(const uint8_t* __restrict__ count, const uint8_t* __restrict__ solid, const uint8_t* __restrict__ sink, const uint8_t* __restrict__ source,
                                           int X, int Y, int x, int y) {
  if (x < 1 || y < 1 || x > X - 2 || y > Y - 2) return false;
  const size_t c = (size_t)y * X + x;
  if (solid[c] | sink[c] | source[c]) return false;
  bool wet = true;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      if (dx == 0 && dy == 0) continue;
      const size_t q = (size_t)(y + dy) * X + (x + dx);
      wet = wet && (count[q] != 0 || solid[q] != 0);
    }
  return wet;
}

// ---- cells.  A lane takes VEC consecutive cells of the row-major grids (VEC = 4 where X % 4 == 0: the four bytes are one word of one row), a wave 64 VEC cells =
// VEC whole words of either mask, which it always writes.  tmap (the tile map, where the handle may use it): a wave whose cells lie in tiles with no water in
// the count grid or in the previous one writes zeros and leaves - nothing is crowded there and nothing was water a refresh ago.
template <int VEC>
__global__ __launch_bounds__(256) void k_rs_cells(const uint8_t* __restrict__ count, const uint8_t* __restrict__ prev, const uint8_t* __restrict__ solid,
                                                  const uint8_t* __restrict__ sink, const uint8_t* __restrict__ source, int X, int Y, unsigned int thin, int fill,
                                                  const uint8_t* __restrict__ tmap, int tnx, int tn,
                                                  unsigned long long* __restrict__ crowded_mask, unsigned long long* __restrict__ hole_mask) {
  const size_t C = (size_t)X * Y, nwords = (C + 63) / 64;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, i = t * VEC;
  const int lane = (int)(threadIdx.x & 63);
  const size_t w0 = (t - lane) * VEC, word0 = w0 >> 6;      // the wave's first cell and first mask word
  if (w0 >= C) return;
  bool idle = false;
  if (tmap) {      // (uniform over the wave)
    const size_t last = (w0 + 64 * VEC < C ? w0 + 64 * VEC : C) - 1;
    const int y0 = (int)(w0 / X), y1 = (int)(last / X);
    unsigned int any = 0;
    for (int y = y0; y <= y1; ++y) {
      const int xa = y == y0 ? (int)(w0 % X) : 0, xb = y == y1 ? (int)(last % X) : X - 1;
      for (int tx = xa >> 6; tx <= xb >> 6; ++tx) { const int q = (y >> 6) * tnx + tx; any |= (unsigned int)tmap[q] | tmap[tn + q]; }
    }
    idle = any == 0;
  }
  unsigned int cr = 0, ho = 0;      // bit k: cell i + k
  if (!idle && i < C) {
    unsigned int cn, pv = 0;
    if (VEC == 4) { cn = *reinterpret_cast<const unsigned int*>(count + i); if (fill) pv = *reinterpret_cast<const unsigned int*>(prev + i); }
    else { cn = count[i]; if (fill) pv = prev[i]; }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const unsigned int c = (cn >> (8 * k)) & 0xffu, p = (pv >> (8 * k)) & 0xffu;
      if (thin && c > thin) cr |= 1u << k;
      if (fill && c == 0u && p != 0u && rs_is_hole(count, solid, sink, source, X, Y, (int)((i + k) % X), (int)((i + k) / X))) ho |= 1u << k;
    }
  }
  if (VEC == 1) {
    const unsigned long long bc = __ballot(cr != 0), bh = __ballot(ho != 0);
    if (lane == 0) { if (thin) crowded_mask[word0] = bc; if (fill) hole_mask[word0] = bh; }
  } else {
    unsigned long long bc[4], bh[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { bc[k] = __ballot((cr >> k) & 1u); bh[k] = __ballot((ho >> k) & 1u); }
    if ((lane & 15) == 0) {      // lanes 16 q .. 16 q + 15 are word q: cell 4 (l & 15) + k is bit 4 (l & 15) + k
      const int q = lane >> 4;
      if (word0 + q < nwords) {
        unsigned long long wc = 0, wh = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { wc |= rs_spread4(bc[k] >> (16 * q)) << k; wh |= rs_spread4(bh[k] >> (16 * q)) << k; }
        if (thin) crowded_mask[word0 + q] = wc;
        if (fill) hole_mask[word0 + q] = wh;
      }
    }
  }
}

// ---- the list of this pass: the first K crowded cells, their slots empty; one thread keeps the books
__global__ __launch_bounds__(256) void k_rs_plan(const unsigned int* __restrict__ found, unsigned int* __restrict__ cells, unsigned int* __restrict__ slot,
                                                 MarkerState* ms, unsigned int max_cells) {
  const unsigned int total = ms->rs_crowded, K = total < max_cells ? total : max_cells;
  for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < 16 * (size_t)K; j += (size_t)gridDim.x * blockDim.x) {
    slot[j] = RS_NONE;
    if (j < K) cells[j] = found[j];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ms->rs_k = K;
    ms->rs_thinned += K;
    ms->rs_deferred += total - K;
  }
}

// the rank of cell c in the ascending list, or RS_NONE
__device__ __forceinline__ unsigned int rs_rank(const unsigned int* __restrict__ cells, unsigned int K, unsigned int c) {
  unsigned int lo = 0, hi = K;
  while (lo < hi) { const unsigned int mid = (lo + hi) >> 1; if (cells[mid] < c) lo = mid + 1; else hi = mid; }
  return lo < K && cells[lo] == c ? lo : RS_NONE;
}
// the slot of a marker: 16 k + 4 sy + sx where its cell is listed, else RS_NONE.  The count byte comes first: most markers sit in cells that are not crowded and
// never search (a listed cell is crowded; a crowded cell beyond max_cells is not listed)
__device__ __forceinline__ unsigned int rs_marker_slot(float px, float py, const uint8_t* __restrict__ count, int X, unsigned int thin,
                                                       const unsigned int* __restrict__ cells, unsigned int K) {
  const int cx = (int)floorf(px), cy = (int)floorf(py);
  const unsigned int c = (unsigned int)cy * (unsigned int)X + (unsigned int)cx;
  if ((unsigned int)count[c] <= thin) return RS_NONE;
  const unsigned int k = rs_rank(cells, K, c);
  if (k == RS_NONE) return RS_NONE;
  return 16u * k + 4u * (unsigned int)eu_reseed_subcell(py, cy) + (unsigned int)eu_reseed_subcell(px, cx);
}

// ---- claim: markers 2 t and 2 t + 1 per lane, one 16-byte load (k_edit_markers' layout)
__global__ __launch_bounds__(256) void k_rs_claim(const float4* __restrict__ m2, const uint8_t* __restrict__ count, int X, unsigned int thin,
                                                  const unsigned int* __restrict__ cells, unsigned int* __restrict__ slot, const MarkerState* ms) {
  const unsigned int K = ms->rs_k;
  if (K == 0) return;
  const unsigned long long n = ms->n, j = (unsigned long long)blockIdx.x * 256 + threadIdx.x, i0 = 2ull * j;
  if (i0 + 1ull < n) {
    const float4 p = m2[j];
    const unsigned int s0 = rs_marker_slot(p.x, p.y, count, X, thin, cells, K), s1 = rs_marker_slot(p.z, p.w, count, X, thin, cells, K);
    if (s0 != RS_NONE) atomicMin(&slot[s0], (unsigned int)i0);
    if (s1 != RS_NONE) atomicMin(&slot[s1], (unsigned int)i0 + 1u);
  } else if (i0 < n) {      // an odd count: the last marker alone
    const float2 p = reinterpret_cast<const float2*>(m2)[i0];
    const unsigned int s0 = rs_marker_slot(p.x, p.y, count, X, thin, cells, K);
    if (s0 != RS_NONE) atomicMin(&slot[s0], (unsigned int)i0);
  }
}

// ---- ballot: delete where listed and not the claimant.  The wave's 128 markers are two words of the mask, always written (the select behind reads every word
// of the launch's range); no cell listed: zeros, before any marker is loaded
__global__ __launch_bounds__(256) void k_rs_ballot(const float4* __restrict__ m2, const uint8_t* __restrict__ count, int X, unsigned int thin,
                                                   const unsigned int* __restrict__ cells, const unsigned int* __restrict__ slot, const MarkerState* ms,
                                                   unsigned long long* __restrict__ delmask, unsigned long long nwords) {
  const unsigned int K = ms->rs_k;
  const unsigned long long j = (unsigned long long)blockIdx.x * 256 + threadIdx.x, i0 = 2ull * j;
  const int lane = (int)(threadIdx.x & 63);
  const unsigned long long w = (i0 - 2ull * lane) >> 6;      // the wave's first word
  if (K == 0) {
    if (lane < 2 && w + lane < nwords) delmask[w + lane] = 0ull;
    return;
  }
  const unsigned long long n = ms->n;
  bool d0 = false, d1 = false;
  if (i0 + 1ull < n) {
    const float4 p = m2[j];
    const unsigned int s0 = rs_marker_slot(p.x, p.y, count, X, thin, cells, K), s1 = rs_marker_slot(p.z, p.w, count, X, thin, cells, K);
    d0 = s0 != RS_NONE && slot[s0] != (unsigned int)i0;
    d1 = s1 != RS_NONE && slot[s1] != (unsigned int)i0 + 1u;
  } else if (i0 < n) {
    const float2 p = reinterpret_cast<const float2*>(m2)[i0];
    const unsigned int s0 = rs_marker_slot(p.x, p.y, count, X, thin, cells, K);
    d0 = s0 != RS_NONE && slot[s0] != (unsigned int)i0;
  }
  const unsigned long long b0 = __ballot(d0), b1 = __ballot(d1);
  if (lane == 0 || lane == 32) {      // lanes 0-31 are the first word, lanes 32-63 the second; marker 2 l + t is bit 2 (l & 31) + t
    const unsigned long long h0 = lane ? b0 >> 32 : b0, h1 = lane ? b1 >> 32 : b1, ww = w + (lane ? 1ull : 0ull);
    if (ww < nwords) delmask[ww] = rs_spread2(h0) | (rs_spread2(h1) << 1);
  }
}

// ---- the counts of the listed cells: the occupied slots; the deletions leave the books
__global__ __launch_bounds__(256) void k_rs_counts(uint8_t* __restrict__ count, const unsigned int* __restrict__ cells, const unsigned int* __restrict__ slot, MarkerState* ms) {
  const unsigned int K = ms->rs_k;
  for (unsigned int k = blockIdx.x * blockDim.x + threadIdx.x; k < K; k += gridDim.x * blockDim.x) {
    const uint4* s = reinterpret_cast<const uint4*>(slot + 16u * k);
    unsigned int occ = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) { const uint4 v = s[q]; occ += (v.x != RS_NONE) + (v.y != RS_NONE) + (v.z != RS_NONE) + (v.w != RS_NONE); }
    count[cells[k]] = (uint8_t)occ;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && K) {
    const unsigned int D = ms->n_deleted;
    ms->n -= D;
    ms->rs_removed += D;
  }
}

// ---- filling: k_source_draws without the latch (one thread) ...
__global__ void k_rs_fill_plan(MarkerState* ms, const RngJump* __restrict__ J, unsigned int max_fill) {
  const unsigned long long n = ms->n, cap = ms->max_markers - 1;
  const unsigned int holes = ms->rs_holes;
  unsigned long long n_app = holes < max_fill ? holes : max_fill;
  const unsigned long long room = n < cap ? cap - n : 0ull;
  if (n_app > room) n_app = room;
  ms->rs_rng0 = ms->rng_state;
  ms->rng_state = eu_rng_jump(J, ms->rng_state, 2 * n_app);      // two draws per appended marker
  ms->rs_n0 = n;
  ms->rs_fill = (unsigned int)n_app;
  ms->n = n + n_app;
  ms->rs_added += n_app;
  ms->rs_deferred += holes - n_app;
}
// ... k_source_fill's draws: a thread jumps to its chunk of the one stream
#define RS_CHUNK 32
__global__ __launch_bounds__(256) void k_rs_draws(const MarkerState* ms, const RngJump* __restrict__ J, float* __restrict__ draws) {
  const unsigned long long n_app = ms->rs_fill;
  const unsigned long long c0 = ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) * RS_CHUNK;
  if (c0 >= n_app) return;
  unsigned long long st = eu_rng_jump(J, ms->rs_rng0, 2 * c0);
  const unsigned long long c1 = c0 + RS_CHUNK < n_app ? c0 + RS_CHUNK : n_app;
  for (unsigned long long c = c0; c < c1; ++c) {
    st = eu_rng_step(st); draws[2 * c] = eu_rng_float(st);          // y first (main.c:288)
    st = eu_rng_step(st); draws[2 * c + 1] = eu_rng_float(st);
  }
}
// ... and k_source_place: the hole's count was 0
__global__ __launch_bounds__(256) void k_rs_place(float2* __restrict__ m, uint8_t* __restrict__ count, const unsigned int* __restrict__ holes, const float* __restrict__ draws,
                                                  const MarkerState* ms, int X, uint8_t* __restrict__ tmap, int tnx) {
  const unsigned int n_app = ms->rs_fill;
  const unsigned long long n0 = ms->rs_n0;
  for (unsigned int k = blockIdx.x * blockDim.x + threadIdx.x; k < n_app; k += gridDim.x * blockDim.x) {
    const unsigned int c = holes[k];
    const int x = (int)(c % (unsigned)X), y = (int)(c / (unsigned)X);
    const float ry = draws[2 * k], rx = draws[2 * k + 1];
    m[n0 + k] = make_float2(EU_H * (x + rx), EU_H * (y + ry));
    count[c] = 1;
    if (tmap) tmap[(y >> 6) * tnx + (x >> 6)] = 1;      // the tile map (euler_dev.h): the tile holds water now - the hole may be its only water
  }
}

int eu_launch_reseed(euler_sim* S) {      // (whole-grid handles, behind eu_launch_refresh_counts: count, prev_count and both tile maps are what it left)
  const euler_reseed& r = S->reseed;
  const unsigned int max_cells = (unsigned int)eu_reseed_limit(r.max_cells), max_fill = (unsigned int)eu_reseed_limit(r.max_fill), thin = (unsigned int)r.thin_above;
  const unsigned long long n = S->n_markers_host;      // an upper bound of the device's count behind the refresh; the kernels go by ms->n
  const size_t cwords = (S->C + 63) / 64;
  unsigned long long* hole_mask = (unsigned long long*)S->rs_mask_buf.p;
  unsigned int *cells = (unsigned int*)S->rs_cell_buf.p, *slot = (unsigned int*)S->rs_slot_buf.p;
  const uint8_t* tmap = eu_tile_map_on(S) ? (const uint8_t*)S->tmap : (const uint8_t*)nullptr;
  int rc;
  eu_vd_reseeded(&S->vd);
  if ((S->X & 3) == 0)
    LAUNCH(S, KC_MARKER_BIN, k_rs_cells<4>, dim3(eu_blocks((S->C + 3) / 4, 256)), dim3(256), S->count, S->prev_count, S->solid, S->sink, S->source, S->X, S->Y, thin, r.fill_holes,
           tmap, S->tmap_nx, S->tmap_n, S->cellmask64, hole_mask);
  else
    LAUNCH(S, KC_MARKER_BIN, k_rs_cells<1>, dim3(eu_blocks(S->C, 256)), dim3(256), S->count, S->prev_count, S->solid, S->sink, S->source, S->X, S->Y, thin, r.fill_holes,
           tmap, S->tmap_nx, S->tmap_n, S->cellmask64, hole_mask);
  if (thin) {
    if ((rc = eu_ordered_select(S, S->cellmask64, cwords, S->sel_idx, &S->ms->rs_crowded))) return rc;
    LAUNCH(S, KC_MARKER_BIN, k_rs_plan, dim3(eu_blocks(16 * (size_t)max_cells, 256, 1024)), dim3(256), S->sel_idx, cells, slot, S->ms, max_cells);
    const size_t nwords = (size_t)((n + 63) / 64);
    if (n) {
      const float4* m2 = reinterpret_cast<const float4*>(S->markers[S->cur]);
      const dim3 grid(eu_blocks((size_t)((n + 1) / 2), 256));
      LAUNCH(S, KC_MARKER_BIN, k_rs_claim, grid, dim3(256), m2, S->count, S->X, thin, cells, slot, S->ms);
      LAUNCH(S, KC_MARKER_BIN, k_rs_ballot, grid, dim3(256), m2, S->count, S->X, thin, cells, slot, S->ms, S->evmask, (unsigned long long)nwords);
      if ((rc = eu_ordered_select(S, S->evmask, nwords, S->sel_idx, &S->ms->n_deleted))) return rc;
      if ((rc = eu_marker_compact(S, S->evmask))) return rc;
      LAUNCH(S, KC_MARKER_COMPACT, k_rs_counts, dim3(eu_blocks(max_cells, 256, 256)), dim3(256), S->count, cells, slot, S->ms);
    }
  }
  if (r.fill_holes) {
    if ((rc = eu_ordered_select(S, hole_mask, cwords, S->sel_idx, &S->ms->rs_holes))) return rc;
    LAUNCH(S, KC_SOURCES, k_rs_fill_plan, dim3(1), dim3(1), S->ms, S->rng_jump, max_fill);
    LAUNCH(S, KC_SOURCES, k_rs_draws, dim3(eu_blocks(((size_t)max_fill + RS_CHUNK - 1) / RS_CHUNK, 256)), dim3(256), S->ms, S->rng_jump, (float*)S->rs_draw_buf.p);
    LAUNCH(S, KC_SOURCES, k_rs_place, dim3(eu_blocks(max_fill, 256, 2048)), dim3(256), S->markers[S->cur], S->count, S->sel_idx, (const float*)S->rs_draw_buf.p, S->ms, S->X,
           S->tmap, S->tmap_nx);
  }
  HIPCHK(hipGetLastError());
  return EULER_OK;
}

// ---- the entry points
extern "C" int euler_set_reseed(euler_sim* S, const euler_reseed* r) {
  const char* who = "euler_set_reseed";
  if (!S) { eu_set_error("%s: null argument", who); return EULER_EINVAL; }
  if (S->slab_on) { eu_set_error("%s: not on a row-slab handle (the pass walks the whole marker array and the whole count grid)", who); return EULER_ESTATE; }
  if (!S->loaded) { eu_set_error("%s: no scenario loaded", who); return EULER_ESTATE; }
  euler_reseed rec;
  memset(&rec, 0, sizeof rec);
  if (r) rec = *r;
  char why[160];
  if (eu_reseed_check(&rec, why, sizeof why)) { eu_set_error("%s: %s", who, why); return EULER_EINVAL; }
  const bool on = rec.thin_above != 0 || rec.fill_holes != 0;
  int rc;
  if (on) {      // grow-only: a failure leaves the handle as it was
    const size_t max_cells = (size_t)eu_reseed_limit(rec.max_cells), max_fill = (size_t)eu_reseed_limit(rec.max_fill);
    if ((rc = eu_devbuf_reserve(S, who, "the hole mask", &S->rs_mask_buf, ((S->C + 63) / 64 + 1) * sizeof(unsigned long long)))) return rc;
    if ((rc = eu_devbuf_reserve(S, who, "the cell list", &S->rs_cell_buf, max_cells * sizeof(unsigned int)))) return rc;
    if ((rc = eu_devbuf_reserve(S, who, "the sub-cell slots", &S->rs_slot_buf, 16 * max_cells * sizeof(unsigned int)))) return rc;
    if ((rc = eu_devbuf_reserve(S, who, "the draws", &S->rs_draw_buf, 2 * max_fill * sizeof(float)))) return rc;
  }
  HIPCHK(hipMemsetAsync(&S->ms->rs_removed, 0, 4 * sizeof(unsigned long long), S->stream));      // the totals count from this call
  if ((rc = eu_sync_marker_state(S))) return rc;
  S->reseed = rec;
  S->reseed_on = on ? 1 : 0;
  return EULER_OK;
}

extern "C" int euler_get_reseed(euler_sim* S, euler_reseed* r, euler_reseed_stats* stats) {
  if (!S) { eu_set_error("euler_get_reseed: null argument"); return EULER_EINVAL; }
  if (r) *r = S->reseed;
  if (stats) {      // the mirror every call that runs the device ends with (eu_sync_marker_state)
    stats->removed = S->ms_host->rs_removed; stats->added = S->ms_host->rs_added;
    stats->cells_thinned = S->ms_host->rs_thinned; stats->deferred = S->ms_host->rs_deferred;
  }
  return EULER_OK;
}
