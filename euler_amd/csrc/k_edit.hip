// k_edit.hip — euler_edit_box (include/euler.h, docs/editing.md): a box of interior cells and the markers in it edited where they live.
//
// An edit is what the reference would do to the same state with its own tools: deleting is refresh_marker_counts' swap-with-last removal
// (main.c:105-116) with "the marker lies in the box" as the condition, seeding is sim_init's loop (main.c:255-266) over the eligible cells of the
// box, off the handle's one xorshift stream.  Four passes, all on the handle's stream:
//   census   (read only) the eligible cells E and the source cells of the box: the capacity check and the source bookkeeping, one read-back;
//   markers  SOLID / SINK / DRAIN: "in the box" balloted into a delete mask, eu_ordered_select, k_compact_markers;
//   cells    the masks and the zero counts of the box; SOURCE / FILL: the eligible cells balloted into a bit mask in column-major bit order;
//   seed     SOURCE / FILL: eu_ordered_select over that mask; the thread of rank k jumps the stream to draw 8 k and stores its cell's four markers.
// No new device buffer: the masks and lists are the marker stage's own scratch (evmask, cellmask64, sel_idx), the counts travel in the per-stage words
// of MarkerState, which every substep overwrites before it reads them.
#include "euler_dev.h"
#include "k_observe.h"

int eu_pressure_current(euler_sim* S);                                        // k_grid.hip
int eu_set_source_count(euler_sim* S, size_t nsrc);                           // driver.hip
int eu_marker_compact(euler_sim* S, const unsigned long long* delmask);       // k_markers.hip

struct EdBox { int x0, y0, x1, y1, Bh; };

__device__ __forceinline__ bool ed_eligible(int op, unsigned int so, unsigned int si, unsigned int cn) {      // after the op's mask change: SOURCE clears solid and sink
  return cn == 0u && (op == EULER_EDIT_SOURCE || (so == 0u && si == 0u));
}

// ---- census: E into ms->n_events, the box's source cells into ms->n_actual (both cleared by the host first).  Reads only.
template <int VEC>
__global__ __launch_bounds__(256) void k_edit_census(const uint8_t* __restrict__ solid, const uint8_t* __restrict__ source, const uint8_t* __restrict__ sink,
                                                     const uint8_t* __restrict__ count, int X, EdBox b, int op, MarkerState* ms) {
  const int xb = ob_xbase(VEC, b.x0) + 64 * VEC * (int)blockIdx.x, yb = b.y0 + 4 * (int)blockIdx.y;
  const int x = xb + VEC * (int)(threadIdx.x & 63), y = yb + (int)(threadIdx.x >> 6);
  unsigned int e = 0, s = 0;
  if (y <= b.y1 && x <= b.x1) {
    const size_t i = (size_t)y * X + x;
    const unsigned int so = ObRow<VEC, true, false>::bytes(solid, i), sr = ObRow<VEC, true, false>::bytes(source, i), si = ObRow<VEC, true, false>::bytes(sink, i),
                       cn = ObRow<VEC, true, false>::bytes(count, i);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      if (x + k < b.x0 || x + k > b.x1) continue;
      const unsigned int sh = 8 * k;
      s += ((sr >> sh) & 0xffu) != 0u;
      e += (op == EULER_EDIT_SOURCE || op == EULER_EDIT_FILL) && ed_eligible(op, (so >> sh) & 0xffu, (si >> sh) & 0xffu, (cn >> sh) & 0xffu);
    }
  }
  e = ob_wave<ObSum>(e); s = ob_wave<ObSum>(s);
  if ((threadIdx.x & 63) == 0) {
    if (e) atomicAdd(&ms->n_events, e);
    if (s) atomicAdd(&ms->n_actual, s);
  }
}

// ---- cells: a workgroup takes 64 x 64 cells of the box.  Lanes lie along a row, VEC cells each (k_observe.h: groups aligned to absolute x & ~3, the cells an
// edge cuts keep their bytes); SOURCE / FILL: the tile's eligibility goes through LDS to lanes along a COLUMN, whose ballot is 64 consecutive bits of the mask -
// bit (x - x0) * Bh + (y - y0), the order sim_init seeds in (x outer, y inner).  The mask was cleared by the host; two columns may share a word: atomic or.
template <int VEC>
__global__ __launch_bounds__(256) void k_edit_cells(uint8_t* __restrict__ solid, uint8_t* __restrict__ source, uint8_t* __restrict__ sink, uint8_t* __restrict__ count,
                                                    int X, EdBox b, int op, unsigned long long* __restrict__ mask) {
  __shared__ uint8_t tile[64][65];
  const int xb = ob_xbase(VEC, b.x0) + 64 * (int)blockIdx.x, yb = b.y0 + 64 * (int)blockIdx.y;
  constexpr int LPR = 64 / VEC, RPP = 256 / LPR;      // lanes per row, rows per pass
  const int xq = VEC * (int)(threadIdx.x % LPR), r = (int)(threadIdx.x / LPR);
  const bool seed = op == EULER_EDIT_SOURCE || op == EULER_EDIT_FILL;
  for (int k = r; k < 64; k += RPP) {
    const int x = xb + xq, y = yb + k;
    unsigned int el = 0u;
    if (y <= b.y1 && x <= b.x1) {
      const size_t i = (size_t)y * X + x;
      unsigned int in = 0u;      // 0xff per byte of the group that is a cell of the box
#pragma unroll
      for (int j = 0; j < VEC; ++j) if (x + j >= b.x0 && x + j <= b.x1) in |= 0xffu << (8 * j);
      const unsigned int one = in & 0x01010101u;
      auto put = [&](uint8_t* g, unsigned int old, unsigned int val) {
        const unsigned int w = (old & ~in) | (val & in);
        if constexpr (VEC == 4) *reinterpret_cast<unsigned int*>(g + i) = w; else g[i] = (uint8_t)w;
      };
      using Row = ObRow<VEC, true, false>;
      if (seed) {
        const unsigned int so = Row::bytes(solid, i), si = Row::bytes(sink, i), cn = Row::bytes(count, i);
#pragma unroll
        for (int j = 0; j < VEC; ++j)
          if (((in >> (8 * j)) & 1u) && ed_eligible(op, (so >> (8 * j)) & 0xffu, (si >> (8 * j)) & 0xffu, (cn >> (8 * j)) & 0xffu)) el |= 1u << (8 * j);
        if (op == EULER_EDIT_SOURCE) { put(source, Row::bytes(source, i), one); put(solid, so, 0u); put(sink, si, 0u); }
      } else {
        if (op != EULER_EDIT_DRAIN) {      // SOLID, SINK, CLEAR: the three masks
          put(solid, Row::bytes(solid, i), op == EULER_EDIT_SOLID ? one : 0u);
          put(sink, Row::bytes(sink, i), op == EULER_EDIT_SINK ? one : 0u);
          put(source, Row::bytes(source, i), 0u);
        }
        if (op != EULER_EDIT_CLEAR) put(count, Row::bytes(count, i), 0u);      // SOLID, SINK, DRAIN: the markers of the box are gone
      }
    }
    if (seed) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) tile[k][xq + j] = (uint8_t)((el >> (8 * j)) & 1u);
    }
  }
  if (!seed) return;      // (uniform over the launch)
  __syncthreads();
  const int l = (int)(threadIdx.x & 63), w = (int)(threadIdx.x >> 6);
  for (int c = w; c < 64; c += 4) {      // column xb + c, rows yb + l
    const int x = xb + c;
    if (x < b.x0 || x > b.x1) continue;      // (uniform over the wave)
    const unsigned long long bits = __ballot(tile[l][c] != 0);      // (rows behind y1 and cells outside the box carry 0)
    if (l != 0 || bits == 0ull) continue;
    const unsigned long long bit0 = (unsigned long long)(x - b.x0) * (unsigned long long)b.Bh + (unsigned long long)(yb - b.y0);
    const int sh = (int)(bit0 & 63ull);
    atomicOr(&mask[bit0 >> 6], bits << sh);
    if (sh && (bits >> (64 - sh))) atomicOr(&mask[(bit0 >> 6) + 1], bits >> (64 - sh));
  }
}

// ---- markers: two per lane (one 16-byte load), "in the box" balloted into the delete mask.  floorf(m.x) in [x0, x1] is x0 <= m.x < x1 + 1 (integers below
// 2^24 are exact floats; a NaN is in no box).  The mask was cleared by the host: a wave with no marker in the box leaves after its load (k_viewport.hip).
__device__ __forceinline__ unsigned long long ed_spread(unsigned long long v) {      // bit k of the low 32 -> bit 2 k
  v &= 0xffffffffull;
  v = (v | (v << 16)) & 0x0000ffff0000ffffull;
  v = (v | (v << 8)) & 0x00ff00ff00ff00ffull;
  v = (v | (v << 4)) & 0x0f0f0f0f0f0f0f0full;
  v = (v | (v << 2)) & 0x3333333333333333ull;
  v = (v | (v << 1)) & 0x5555555555555555ull;
  return v;
}
__global__ __launch_bounds__(256) void k_edit_markers(const float4* __restrict__ m2, unsigned long long n, float fx0, float fy0, float fx1, float fy1,
                                                      unsigned long long* __restrict__ delmask) {
  const unsigned long long j = (unsigned long long)blockIdx.x * 256 + threadIdx.x, i0 = 2ull * j;
  bool in0 = false, in1 = false;
  if (i0 + 1ull < n) {
    const float4 p = m2[j];
    in0 = p.x >= fx0 && p.x < fx1 && p.y >= fy0 && p.y < fy1;
    in1 = p.z >= fx0 && p.z < fx1 && p.w >= fy0 && p.w < fy1;
  } else if (i0 < n) {      // an odd count: the last marker alone
    const float2 p = reinterpret_cast<const float2*>(m2)[i0];
    in0 = p.x >= fx0 && p.x < fx1 && p.y >= fy0 && p.y < fy1;
  }
  const unsigned long long b0 = __ballot(in0), b1 = __ballot(in1);
  if ((b0 | b1) == 0ull) return;
  // the wave's 128 markers are two words of the mask: lanes 0-31 the first, lanes 32-63 the second; marker 2 l + t is bit 2 (l & 31) + t
  const int lane = (int)(threadIdx.x & 63);
  if (lane != 0 && lane != 32) return;
  const unsigned long long h0 = lane ? b0 >> 32 : b0, h1 = lane ? b1 >> 32 : b1;
  const unsigned long long word = ed_spread(h0) | (ed_spread(h1) << 1);
  if (word) delmask[(j >> 5)] = word;      // (a set bit is a marker below n: the word lies inside the mask)
}

// ---- seed: the thread of rank k takes the k-th eligible cell in column-major order; draws 8 k .. 8 k + 7 of the stream are its cell's (euler_seed_markers, euler_host.c)
__global__ __launch_bounds__(256) void k_edit_seed(float2* __restrict__ m, uint8_t* __restrict__ count, const unsigned int* __restrict__ elig, const MarkerState* ms,
                                                   const RngJump* __restrict__ J, int X, EdBox b) {
  const unsigned int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= ms->n_events) return;
  const unsigned int c = elig[k];
  const int cx = b.x0 + (int)(c / (unsigned int)b.Bh), cy = b.y0 + (int)(c % (unsigned int)b.Bh);
  unsigned long long st = eu_rng_jump(J, ms->rng_state, 8ull * k);
  float2* out = m + ms->n + 4ull * k;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    st = eu_rng_step(st);
    const float jx = eu_rng_float(st) / 2;
    const float mx = cx + (q < 2 ? 0 : 0.5f) + jx;
    st = eu_rng_step(st);
    const float jy = eu_rng_float(st) / 2;
    const float my = cy + (q % 2 ? 0 : 0.5f) + jy;
    out[q] = make_float2(EU_H * mx, EU_H * my);
  }
  count[(size_t)cy * X + cx] = 4;
}

// ---- the bookkeeping, one thread, behind the passes that read it: the deletions leave, the seeded markers join, the stream moves on by 8 draws per cell
__global__ void k_edit_commit(MarkerState* ms, const RngJump* __restrict__ J, int deleted, int seeded) {
  if (deleted) ms->n -= ms->n_deleted;
  if (seeded) {
    const unsigned long long E = ms->n_events;
    ms->n += 4ull * E;
    ms->rng_state = eu_rng_jump(J, ms->rng_state, 8ull * E);
  }
}

template <int VEC>
static int ed_run(euler_sim* S, int op, const EdBox& b) {
  const int X = S->X, Bw = b.x1 - b.x0 + 1, span = b.x1 - ob_xbase(VEC, b.x0) + 1;
  const bool del = op == EULER_EDIT_SOLID || op == EULER_EDIT_SINK || op == EULER_EDIT_DRAIN, seed = op == EULER_EDIT_SOURCE || op == EULER_EDIT_FILL;
  int rc = eu_pressure_current(S);      // the pending pressure is finished from the solver's arrays as they stand
  if (rc) return rc;
  // census: what the edit would seed, the source cells it covers, and the marker count as the device has it
  HIPCHK(hipMemsetAsync(&S->ms->n_events, 0, 2 * sizeof(unsigned int), S->stream));      // (n_events, n_actual)
  LAUNCH(S, KC_MISC, k_edit_census<VEC>, dim3((unsigned)((span + 64 * VEC - 1) / (64 * VEC)), (unsigned)((b.Bh + 3) / 4)), dim3(256), S->solid, S->source, S->sink, S->count, X, b, op, S->ms);
  if ((rc = eu_sync_marker_state(S))) return rc;
  const unsigned long long n = S->ms_host->n, E = S->ms_host->n_events, src_old = S->ms_host->n_actual;
  if (seed && n + 4ull * E > (unsigned long long)S->max_markers - 1ull) {
    eu_set_error("euler_edit_box: %llu markers and %llu cells to seed: more than the %llu the array holds", n, E, (unsigned long long)S->max_markers - 1ull);
    return EULER_EINVAL;
  }
  eu_vd_edited(&S->vd);
  if (del && n) {
    const size_t nwords = (size_t)((n + 63) / 64);
    HIPCHK(hipMemsetAsync(S->evmask, 0, nwords * sizeof(unsigned long long), S->stream));
    LAUNCH(S, KC_MISC, k_edit_markers, dim3(eu_blocks((size_t)((n + 1) / 2), 256)), dim3(256), reinterpret_cast<const float4*>(S->markers[S->cur]), n, (float)b.x0, (float)b.y0,
           (float)(b.x1 + 1), (float)(b.y1 + 1), S->evmask);
    if ((rc = eu_ordered_select(S, S->evmask, nwords, S->sel_idx, &S->ms->n_deleted))) return rc;
    if ((rc = eu_marker_compact(S, S->evmask))) return rc;
  }
  const size_t ewords = ((size_t)Bw * b.Bh + 63) / 64;
  if (seed) HIPCHK(hipMemsetAsync(S->cellmask64, 0, ewords * sizeof(unsigned long long), S->stream));
  LAUNCH(S, KC_MISC, k_edit_cells<VEC>, dim3((unsigned)((span + 63) / 64), (unsigned)((b.Bh + 63) / 64)), dim3(256), S->solid, S->source, S->sink, S->count, X, b, op, S->cellmask64);
  if (seed && E) {
    if ((rc = eu_ordered_select(S, S->cellmask64, ewords, S->sel_idx, &S->ms->n_events))) return rc;
    LAUNCH(S, KC_MISC, k_edit_seed, dim3(eu_blocks((size_t)E, 256)), dim3(256), S->markers[S->cur], S->count, S->sel_idx, S->ms, S->rng_jump, X, b);
  }
  if ((del && n) || (seed && E)) hipLaunchKernelGGL(k_edit_commit, dim3(1), dim3(1), 0, S->stream, S->ms, S->rng_jump, del && n ? 1 : 0, seed && E ? 1 : 0);
  HIPCHK(hipGetLastError());
  if (op != EULER_EDIT_DRAIN && op != EULER_EDIT_FILL) {      // a mask changed: the marker stage's column-major copies and the source stage's cell count follow
    eu_vd_masks_changed(&S->vd);
    const size_t src_new = S->n_source_cells - (size_t)src_old + (op == EULER_EDIT_SOURCE ? (size_t)Bw * b.Bh : 0);
    if (src_new != S->n_source_cells && (rc = eu_set_source_count(S, src_new))) return rc;
  }
  if (S->heat_on && (rc = eu_heat_dry(S))) return rc;      // (the temperature of the cells the edit emptied: ambient, as in every cell without markers - docs/heat.md)
  return eu_sync_marker_state(S);      // the host's marker count is in step again
}

// ---- the moving bodies' use of the passes above (k_bodies.hip, docs/bodies.md): the cell pass of SOLID or CLEAR over a strip or a rectangle, in the profile class of
// the stage that shifts, and the source cells a strip is about to cover.  The caller has done an edit's bookkeeping (eu_pressure_current, eu_vd_masks_changed).
int eu_edit_cells_box(euler_sim* S, int cls, int op, int x0, int y0, int x1, int y1) {
  const EdBox b{x0, y0, x1, y1, y1 - y0 + 1};
  if ((S->X & 3) == 0) {
    const int span = x1 - ob_xbase(4, x0) + 1;
    LAUNCH(S, cls, k_edit_cells<4>, dim3((unsigned)((span + 63) / 64), (unsigned)((b.Bh + 63) / 64)), dim3(256), S->solid, S->source, S->sink, S->count, S->X, b, op, S->cellmask64);
  } else {
    const int span = x1 - ob_xbase(1, x0) + 1;
    LAUNCH(S, cls, k_edit_cells<1>, dim3((unsigned)((span + 63) / 64), (unsigned)((b.Bh + 63) / 64)), dim3(256), S->solid, S->source, S->sink, S->count, S->X, b, op, S->cellmask64);
  }
  HIPCHK(hipGetLastError());
  return EULER_OK;
}
int eu_edit_source_census(euler_sim* S, int cls, int x0, int y0, int x1, int y1, size_t* nsrc) {      // (one read-back: only handles with source cells come here)
  const EdBox b{x0, y0, x1, y1, y1 - y0 + 1};
  HIPCHK(hipMemsetAsync(&S->ms->n_events, 0, 2 * sizeof(unsigned int), S->stream));      // (n_events, n_actual)
  if ((S->X & 3) == 0) {
    const int span = x1 - ob_xbase(4, x0) + 1;
    LAUNCH(S, cls, k_edit_census<4>, dim3((unsigned)((span + 255) / 256), (unsigned)((b.Bh + 3) / 4)), dim3(256), S->solid, S->source, S->sink, S->count, S->X, b, (int)EULER_EDIT_SOLID, S->ms);
  } else {
    const int span = x1 - ob_xbase(1, x0) + 1;
    LAUNCH(S, cls, k_edit_census<1>, dim3((unsigned)((span + 63) / 64), (unsigned)((b.Bh + 3) / 4)), dim3(256), S->solid, S->source, S->sink, S->count, S->X, b, (int)EULER_EDIT_SOLID, S->ms);
  }
  HIPCHK(hipGetLastError());
  int rc = eu_sync_marker_state(S);
  if (!rc) *nsrc = (size_t)S->ms_host->n_actual;
  return rc;
}

extern "C" int euler_edit_box(euler_sim* S, int32_t op, int32_t x0, int32_t y0, int32_t x1, int32_t y1) {
  int rc = eu_observe_enter(S, "euler_edit_box", "solid and source cells are facts a slab only gets from a load", S, x0, y0, x1, y1);
  if (rc) return rc;
  if (op < EULER_EDIT_SOLID || op > EULER_EDIT_DRAIN) { eu_set_error("euler_edit_box: op %d: one of EULER_EDIT_*", (int)op); return EULER_EINVAL; }
  for (int k = 0; k < S->n_bodies; ++k) {      // a moving body's cells are the body's: its next shift would undo the edit half way (docs/bodies.md)
    const int bx = S->body_ox[k], by = S->body_oy[k];
    if (x0 <= bx + S->bodies[k].w - 1 && x1 >= bx && y0 <= by + S->bodies[k].h - 1 && y1 >= by) {
      eu_set_error("euler_edit_box: the box [%d, %d] x [%d, %d] intersects body %d at [%d, %d] x [%d, %d]", x0, x1, y0, y1, k, bx, bx + S->bodies[k].w - 1, by, by + S->bodies[k].h - 1);
      return EULER_ESTATE;
    }
  }
  const EdBox b{x0, y0, x1, y1, y1 - y0 + 1};
  return (S->X & 3) == 0 ? ed_run<4>(S, op, b) : ed_run<1>(S, op, b);
}
