// k_diagnostics.hip — euler_diagnostics (include/euler.h, docs/diagnostics.md): a box of interior cells reduced on the device to ONE euler_diag record -
// residual divergence, kinetic energy, mass and centre of mass, marker crowding.  Every field is an integer sum or a maximum of non-negative floats
// (compared as unsigned bit patterns): whatever order the cells arrive in, the record is the same.
//
// One launch.  A workgroup owns DG_T * VEC columns of the box and one segment of at most DG_ROWS rows that lies inside one row of 64 x 64 tiles.  Lanes lie
// along a grid row (four cells each where the rows are 16-byte aligned) and walk DOWN the segment: the row of v below a cell is the next row's own v and is
// kept in registers, so a row costs one load of count, solid, u and v each plus the cell to the left of the lane's first.  A lane sums in registers; a wave
// folds by shuffles and goes to the workgroup's LDS record once; the workgroup goes to the device record once, twelve lanes with one integer atomic each.
// With the tile map a lane whose tile holds no water reads nothing at all.
//
// The pass only reads the state and touches none of the handle's validity flags.
#include "euler_dev.h"

#define DG_T 256        // threads per workgroup
#define DG_ROWS 32      // rows a workgroup walks: divides 64, so a segment never crosses a row of 64 x 64 tiles (one tile-map flag per lane and segment);
                        // chosen by measurement, profiles/diagnostics.md
static_assert(64 % DG_ROWS == 0, "a segment must lie inside one row of tiles");

struct DgArgs {
  const uint8_t *solid, *count;
  const float *u, *v;
  const uint8_t* tmap;      // null: every tile is read
  int tnx;
  int X;
  int x0, y0, x1, y1;       // the box, inclusive
  int ncol;                 // workgroups along x
  euler_diag* out;          // zeroed in front of the launch
};

struct DgAcc {
  unsigned long long mass_x, mass_y, div_l1, ke_hi, ke_lo;
  unsigned int fluid, markers, crowded, nonfinite, count_max, div_bits, s2_bits;
};

__device__ __forceinline__ unsigned int dg_wave_sum(unsigned int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned long long dg_wave_sum64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned int dg_wave_max(unsigned int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const unsigned int w = __shfl_xor(v, o, 64); v = w > v ? w : v; }
  return v;
}

// the workgroup's record in LDS, in the order of euler_diag's 64-bit fields behind `cells`, then its 32-bit ones
struct DgShared {
  unsigned long long q[8];      // fluid, markers, crowded, mass_x, mass_y, div_l1, ke_hi, ke_lo
  unsigned int w[4];            // count_max, nonfinite, max_div bits, max_speed2 bits
};

// VEC: cells per lane - 4 where X % 4 == 0 (every row starts 16-byte aligned: one dword of each byte grid, one float4 of u and v), else 1
template <int VEC>
__global__ __launch_bounds__(DG_T) void k_diagnostics(const DgArgs a) {
  __shared__ DgShared sh;
  const int tid = threadIdx.x;
  if (tid < 8) sh.q[tid] = 0ull;
  else if (tid < 12) sh.w[tid - 8] = 0u;
  __syncthreads();
  const int cx = (int)(blockIdx.x % (unsigned int)a.ncol), seg = (int)(blockIdx.x / (unsigned int)a.ncol);      // (neighbouring workgroups lie along a row)
  const int r0 = (a.y0 / DG_ROWS + seg) * DG_ROWS;
  const int ylo = r0 > a.y0 ? r0 : a.y0, yhi = r0 + DG_ROWS - 1 < a.y1 ? r0 + DG_ROWS - 1 : a.y1;      // this segment: rows yhi down to ylo
  const int xbase = VEC == 4 ? (a.x0 & ~3) : a.x0;
  const int x = xbase + (cx * DG_T + tid) * VEC;      // the lane's first column
  DgAcc acc;
  acc.mass_x = acc.mass_y = acc.div_l1 = acc.ke_hi = acc.ke_lo = 0ull;
  acc.fluid = acc.markers = acc.crowded = acc.nonfinite = acc.count_max = acc.div_bits = acc.s2_bits = 0u;
  // (four aligned cells share a tile column, the segment's rows a tile row; the tile map is a superset: a cleared flag means no cell of the tile holds markers)
  if (x <= a.x1 && (!a.tmap || a.tmap[(ylo >> 6) * a.tnx + (x >> 6)] != 0)) {
    const size_t X = (size_t)a.X;
    bool in[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) in[k] = x + k >= a.x0 && x + k <= a.x1;      // box edges that cut the lane's group
    float vv[VEC];      // v of the row being visited: loaded as the row below of the one before
    {
      const size_t i = (size_t)yhi * X + (size_t)x;
      if constexpr (VEC == 4) {
        const float4 v4 = *reinterpret_cast<const float4*>(a.v + i);
        vv[0] = v4.x; vv[1] = v4.y; vv[2] = v4.z; vv[3] = v4.w;
      } else vv[0] = a.v[i];
    }
    for (int y = yhi; y >= ylo; --y) {
      const size_t i = (size_t)y * X + (size_t)x;
      unsigned int so, cn;
      float uu[VEC + 1], vd[VEC];
      if constexpr (VEC == 4) {
        so = *reinterpret_cast<const unsigned int*>(a.solid + i);
        cn = *reinterpret_cast<const unsigned int*>(a.count + i);
        const float4 u4 = *reinterpret_cast<const float4*>(a.u + i);
        const float4 w4 = *reinterpret_cast<const float4*>(a.v + i - X);
        uu[0] = a.u[i - 1]; uu[1] = u4.x; uu[2] = u4.y; uu[3] = u4.z; uu[4] = u4.w;
        vd[0] = w4.x; vd[1] = w4.y; vd[2] = w4.z; vd[3] = w4.w;
      } else {
        so = a.solid[i]; cn = a.count[i];
        uu[0] = a.u[i - 1]; uu[1] = a.u[i];
        vd[0] = a.v[i - X];
      }
      unsigned int row_marks = 0u;
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const unsigned int s = (so >> (8 * k)) & 0xffu, c = (cn >> (8 * k)) & 0xffu;
        if (in[k] && c && !s) {
          acc.fluid += 1u;
          row_marks += c;
          acc.crowded += c >= (unsigned int)EULER_DIAG_CROWDED ? 1u : 0u;
          acc.count_max = c > acc.count_max ? c : acc.count_max;
          acc.mass_x += (unsigned long long)c * (unsigned int)(x + k);
          const float d = ((uu[k + 1] - uu[k]) + vv[k]) - vd[k];      // main.c:720 in its order, h = 1
          const float dx = (uu[k + 1] + uu[k]) / 2.f, dy = (vv[k] + vd[k]) / 2.f;
          const float s2 = dx * dx + dy * dy;
          if (d == d) {
            const float ad = fabsf(d);
            const unsigned int bits = __float_as_uint(ad);      // (ad >= +0: unsigned order = float order)
            acc.div_bits = bits > acc.div_bits ? bits : acc.div_bits;
            acc.div_l1 += (unsigned long long)((ad < 256.f ? ad : 256.f) * 16777216.f);
          }
          if (s2 == s2) {
            const unsigned int bits = __float_as_uint(s2);
            acc.s2_bits = bits > acc.s2_bits ? bits : acc.s2_bits;
            const unsigned long long q = (unsigned long long)((s2 < 16777216.f ? s2 : 16777216.f) * 4294967296.f);
            acc.ke_hi += q >> 32; acc.ke_lo += q & 0xffffffffull;
          }
          acc.nonfinite += (d != d || s2 != s2) ? 1u : 0u;
        }
      }
      acc.markers += row_marks;
      acc.mass_y += (unsigned long long)row_marks * (unsigned int)y;
#pragma unroll
      for (int k = 0; k < VEC; ++k) vv[k] = vd[k];
    }
  }
  // every lane of the workgroup arrives here: fold across the wave, one lane per wave goes to LDS, twelve lanes of the workgroup to the record
  const unsigned int fluid = dg_wave_sum(acc.fluid);
  if (fluid) {      // (wave-uniform)
    const unsigned int markers = dg_wave_sum(acc.markers), crowded = dg_wave_sum(acc.crowded), nonfinite = dg_wave_sum(acc.nonfinite);
    const unsigned int count_max = dg_wave_max(acc.count_max), div_bits = dg_wave_max(acc.div_bits), s2_bits = dg_wave_max(acc.s2_bits);
    const unsigned long long mass_x = dg_wave_sum64(acc.mass_x), mass_y = dg_wave_sum64(acc.mass_y), div_l1 = dg_wave_sum64(acc.div_l1);
    const unsigned long long ke_hi = dg_wave_sum64(acc.ke_hi), ke_lo = dg_wave_sum64(acc.ke_lo);
    if ((tid & 63) == 0) {
      atomicAdd(&sh.q[0], (unsigned long long)fluid); atomicAdd(&sh.q[1], (unsigned long long)markers); atomicAdd(&sh.q[2], (unsigned long long)crowded);
      atomicAdd(&sh.q[3], mass_x); atomicAdd(&sh.q[4], mass_y); atomicAdd(&sh.q[5], div_l1); atomicAdd(&sh.q[6], ke_hi); atomicAdd(&sh.q[7], ke_lo);
      atomicMax(&sh.w[0], count_max); atomicAdd(&sh.w[1], nonfinite); atomicMax(&sh.w[2], div_bits); atomicMax(&sh.w[3], s2_bits);
    }
  }
  __syncthreads();
  // (euler_diag: cells at 0, the eight sums behind it, then count_max, nonfinite, max_div, max_speed2)
  unsigned long long* oq = reinterpret_cast<unsigned long long*>(a.out);
  unsigned int* ow = reinterpret_cast<unsigned int*>(a.out) + 18;
  if (blockIdx.x == 0 && tid == 12) atomicAdd(oq, (unsigned long long)(a.x1 - a.x0 + 1) * (unsigned long long)(a.y1 - a.y0 + 1));
  if (sh.q[0] == 0ull) return;      // no water under this workgroup: nothing to add
  if (tid < 8) { if (sh.q[tid]) atomicAdd(oq + 1 + tid, sh.q[tid]); }
  else if (tid == 9) { if (sh.w[1]) atomicAdd(ow + 1, sh.w[1]); }
  else if (tid < 12) { const int f = tid - 8; if (sh.w[f]) atomicMax(ow + f, sh.w[f]); }
}

static_assert(sizeof(euler_diag) == 88, "euler_diag is 88 bytes without padding");
static_assert(offsetof(euler_diag, fluid) == 8 && offsetof(euler_diag, ke_lo) == 64 && offsetof(euler_diag, count_max) == 72 && offsetof(euler_diag, max_speed2) == 84,
              "k_diagnostics addresses the record by these offsets");

// the reduction alone, on the handle's stream, into S->diag_buf (tools/diagnostics_cost.py times it through the KC_MISC class)
static int dg_launch(euler_sim* S, int x0, int y0, int x1, int y1) {
  const bool vec = S->X % 4 == 0;
  DgArgs a;
  a.solid = S->solid; a.count = S->count; a.u = S->u; a.v = S->v;
  a.tmap = eu_tile_map_on(S) ? S->tmap : nullptr; a.tnx = S->tmap_nx;
  a.X = S->X; a.x0 = x0; a.y0 = y0; a.x1 = x1; a.y1 = y1; a.out = S->diag_buf;
  const int xbase = vec ? (x0 & ~3) : x0, span = DG_T * (vec ? 4 : 1);
  a.ncol = (x1 - xbase + span) / span;
  const int nseg = y1 / DG_ROWS - y0 / DG_ROWS + 1;
  HIPCHK(hipMemsetAsync(S->diag_buf, 0, sizeof(euler_diag), S->stream));
  const dim3 grid((unsigned)((long long)a.ncol * nseg));      // (a workgroup per 256 x 32 cells at the least: far below 2^31 on any grid euler_create accepts)
  if (vec) LAUNCH(S, KC_MISC, (k_diagnostics<4>), grid, dim3(DG_T), a);
  else LAUNCH(S, KC_MISC, (k_diagnostics<1>), grid, dim3(DG_T), a);
  HIPCHK(hipGetLastError());
  return EULER_OK;
}

extern "C" int euler_diagnostics(euler_sim* S, int32_t x0, int32_t y0, int32_t x1, int32_t y1, euler_diag* out, size_t out_bytes) {
  if (!S || !out) { eu_set_error("euler_diagnostics: null argument"); return EULER_EINVAL; }
  if (S->slab_on) { eu_set_error("euler_diagnostics: not on a row-slab handle (the record of a box is the sum over the slabs it crosses)"); return EULER_ESTATE; }
  if (!S->loaded) { eu_set_error("euler_diagnostics: no scenario loaded"); return EULER_ESTATE; }
  if (x0 < 1 || y0 < 1 || x1 > S->X - 2 || y1 > S->Y - 2 || x0 > x1 || y0 > y1) {
    eu_set_error("euler_diagnostics: box [%d, %d] x [%d, %d] is not inside the interior [1, %d] x [1, %d]", (int)x0, (int)x1, (int)y0, (int)y1, S->X - 2, S->Y - 2);
    return EULER_EINVAL;
  }
  if (out_bytes != sizeof(euler_diag)) { eu_set_error("euler_diagnostics: %zu bytes given, %zu expected", out_bytes, sizeof(euler_diag)); return EULER_EINVAL; }
  if (!S->diag_buf) {      // the device record: allocated by the first call (a failure leaves the handle as it was)
    euler_diag* nb = nullptr;
    if (hipMalloc((void**)&nb, sizeof(euler_diag)) != hipSuccess) {
      (void)hipGetLastError();
      eu_set_error("euler_diagnostics: %zu bytes of device memory for the record", sizeof(euler_diag));
      return EULER_ENOMEM;
    }
    S->diag_buf = nb;
    S->hbm_bytes += sizeof(euler_diag);
  }
  const int rc = dg_launch(S, x0, y0, x1, y1);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(out, S->diag_buf, sizeof(euler_diag), hipMemcpyDeviceToHost, S->stream));
  HIPCHK(hipStreamSynchronize(S->stream));
  return EULER_OK;
}

void eu_diagnostics_release(euler_sim* S) {
  if (S->diag_buf) (void)hipFree(S->diag_buf);
  S->diag_buf = nullptr;
}
