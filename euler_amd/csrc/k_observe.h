// k_observe.h — what the read-only observer passes share on the device (k_overview.hip, k_diagnostics.hip, k_viewport.hip;
// docs/observer_passes.md): the wave fold, the loader of a lane's cells of one grid row, the per-cell terms and the tile-map arguments.
// The host side of a pass - entry checks, device buffer, copy back - is eu_observe_* / eu_devbuf_* (euler_dev.h, k_observe.hip).
//
// A pass built from these only reads the state.  Its results are integer sums and maxima of bit patterns: exact in whatever order the cells arrive.
#pragma once
#include "euler_dev.h"

// ---- fold over the 64 lanes of a wave: an xor butterfly, EVERY lane gets the result (the passes test it wave-uniformly)
struct ObSum { template <class T> __device__ static T of(T a, T b) { return a + b; } };
struct ObMax { template <class T> __device__ static T of(T a, T b) { return b > a ? b : a; } };
struct ObMin { template <class T> __device__ static T of(T a, T b) { return b < a ? b : a; } };
template <class Op, class T>
__device__ __forceinline__ T ob_wave(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = Op::of(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- the tile map as a kernel argument: null = every 64 x 64 tile is read whole.  The map is a superset: a cleared flag means no cell of the tile holds markers
struct ObTiles {
  const uint8_t* tmap;
  int tnx;
  __device__ __forceinline__ bool wet(int tx, int ty) const { return !tmap || tmap[ty * tnx + tx] != 0; }
};
static inline ObTiles eu_observe_tiles(const euler_sim* S) { return ObTiles{eu_tile_map_on(S) ? S->tmap : nullptr, S->tmap_nx}; }

// ---- lanes lie along a grid row, VEC cells each: 4 where X % 4 == 0 (every row starts 16-byte aligned: one dword of each byte grid, one float4 of
// each field), else 1.  Lane groups stay aligned to ABSOLUTE x & ~3 whatever the box: the cells an edge cuts are masked by the caller
__host__ __device__ static inline int ob_xbase(int vec, int x0) { return vec == 4 ? (x0 & ~3) : x0; }

// a lane's cells of row y from column x0 on (i = y * X + x0): the byte grids packed one cell per byte, u with the face left of the first cell in
// uu[0], v of the row (vv) and of the row below (vd), the dye.  A dry tile (wet = false) is read for its solid / sink bytes only: cn = 0, the rest unset
template <int VEC, bool SINK, bool DYE>
struct ObRow {
  unsigned int so, si, cn;
  float uu[VEC + 1], vv[VEC], vd[VEC], dye[3][VEC];

  static __device__ __forceinline__ void cells(float* d, const float* g, size_t i) {
    if constexpr (VEC == 4) {
      const float4 t = *reinterpret_cast<const float4*>(g + i);
      d[0] = t.x; d[1] = t.y; d[2] = t.z; d[3] = t.w;
    } else d[0] = g[i];
  }
  static __device__ __forceinline__ unsigned int bytes(const uint8_t* g, size_t i) {
    if constexpr (VEC == 4) return *reinterpret_cast<const unsigned int*>(g + i);
    else return g[i];
  }
  __device__ __forceinline__ void load_v(const float* v, size_t i) { cells(vv, v, i); }
  // V = false: the caller carries vv over from the row above (carry_v) and loads the first row's itself
  template <bool V = true>
  __device__ __forceinline__ void load(const uint8_t* solid, const uint8_t* sink, const uint8_t* count, const float* u, const float* v, const float* const* dy, size_t X, size_t i, bool wet) {
    so = bytes(solid, i);
    si = SINK ? bytes(sink, i) : 0u;
    cn = 0u;
    if (!wet) return;
    cn = bytes(count, i);
    if (DYE) for (int c = 0; c < 3; ++c) cells(dye[c], dy[c], i);
    if (V) load_v(v, i);
    cells(vd, v, i - X);
    cells(uu + 1, u, i);
    uu[0] = u[i - 1];
  }
  __device__ __forceinline__ void carry_v() {
#pragma unroll
    for (int k = 0; k < VEC; ++k) vv[k] = vd[k];
  }
  __device__ __forceinline__ unsigned int solid(int k) const { return (so >> (8 * k)) & 0xffu; }
  __device__ __forceinline__ unsigned int sink(int k) const { return (si >> (8 * k)) & 0xffu; }
  __device__ __forceinline__ unsigned int count(int k) const { return (cn >> (8 * k)) & 0xffu; }
  // the face-average speed^2 of cell k, and the divergence of main.c:720 in its association order (h = 1)
  __device__ __forceinline__ float speed2(int k) const {
    const float dx = (uu[k + 1] + uu[k]) / 2.f, dy = (vv[k] + vd[k]) / 2.f;
    return dx * dx + dy * dy;
  }
  __device__ __forceinline__ float divergence(int k) const { return ((uu[k + 1] - uu[k]) + vv[k]) - vd[k]; }
};

// q(x) of include/euler.h: clamp to [0, 1] (a NaN: 0), times 2^24 (exact), truncated
__device__ __forceinline__ unsigned int ob_q24(float x) {
  const float c = x > 0.f ? (x > 1.f ? 1.f : x) : 0.f;
  return (unsigned int)(c * 16777216.f);
}
// a non-negative float into a running maximum kept as its bit pattern (x >= +0: unsigned order = float order); a NaN is skipped
__device__ __forceinline__ void ob_max_bits(unsigned int& m, float x) {
  const unsigned int bits = __float_as_uint(x);
  if (x == x && bits > m) m = bits;
}
