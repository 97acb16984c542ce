// k_sweep.hip — the parity mode's preconditioner: IC(0) as wavefront sweeps over the band-skewed arrays (k_pcg.h), one workgroup per band.
#include "k_pcg.h"

#include <type_traits>

// ==========================================================================================
// IC(0): E^-1 factor, forward solve, backward solve (apply_preconditioner, main.c:580-627).
//
// Cell (x,y) depends on its left and lower neighbours (forward) or right and upper (backward):
// a 2-D recurrence with no reduction, so every dependency-respecting schedule reproduces the
// sequential sweep bit for bit.
//
// NOTE on the reference's coefficients: get_a_minus_i(y,x) = get_a_plus_i(y,x-1) = is_fluid(y,x)
// ? -1 : 0 (main.c:561-575) is ALWAYS -1 for the fluid cell being visited, whatever its left or
// lower neighbour is.  Hence (a) the E^-1 recurrence reads the STALE precon[] of neighbours that
// are no longer fluid (precon[] persists, main.c:577, and is only written on fluid cells), and
// (b) the forward solve needs no neighbour mask: q is +0 on non-fluid cells.  The backward solve
// uses get_a_plus_i/j(y,x) = is_fluid of the right/upper neighbour.

// one wave per band arrives with its partial; the last one folds all partials in band order (deterministic) and applies the epilogue
__device__ __forceinline__ void sweep_qq_arrive(const SweepArgs& a, int ord, double lane_sum) {
  const int lane = threadIdx.x & 63;
  const double v = eu_wave_sum(lane_sum);
  int last = 0;
  if (lane == 0) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(&a.qq_partial[ord]), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    last = __hip_atomic_fetch_add(a.qq_counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned int)a.nb_local - 1;
  }
  last = __builtin_amdgcn_readfirstlane(last);
  if (!last) return;
  double t = 0.0;
  for (int k = lane; k < a.nb_local; k += 64)
    t += __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<unsigned long long*>(&a.qq_partial[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  t = eu_wave_sum(t);
  if (lane == 0) {
    pcg_scalar_step(a.sc_w, a.fin_qq, t);
    __hip_atomic_store(a.qq_counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <int OP>
__device__ __forceinline__ double sweep_cell(uint8_t m, double in, double pre_here, double own_val, double own_pre,
                                             double nb_val, double nb_pre) {
  // own_* : previous cell of the same row in sweep order (left for forward, right for backward)
  // nb_*  : same column in the previous row in sweep order (below for forward, above for backward)
  if (OP == SW_FACTOR) {
    if (!(m & CM_FLUID)) return pre_here;           // untouched (stale) entry
    const double a = (double)(int)(m >> CM_DIAG_SHIFT);
    const double cl = -1.0 * own_val;               // get_a_minus_i * precon[y][x-1]
    const double cb = -1.0 * nb_val;                // get_a_minus_j * precon[y-1][x]
    double e = a - cl * cl - cb * cb;
    if (e < 0.25 * a) e = (a != 0.0) ? a : 1.0;
    return 1.0 / sqrt(e);
  } else if (OP == SW_FORWARD) {
    if (!(m & CM_FLUID)) return 0.0;
    const double t = in - -1.0 * own_pre * own_val - -1.0 * nb_pre * nb_val;
    return t * pre_here;
  } else {
    if (!(m & CM_FLUID)) return 0.0;
    const double cr = (m & CM_RIGHT) ? -1.0 : 0.0, cu = (m & CM_UP) ? -1.0 : 0.0;
    const double t = in - cr * pre_here * own_val - cu * pre_here * nb_val;
    return t * pre_here;
  }
}

// --- debug / cross-check schedule: one workgroup, one barrier per anti-diagonal ---------------
template <int OP>
__global__ __launch_bounds__(1024) void k_sweep_simple(SweepArgs a) {
  if (!a.force && pcg_idle(a.sc)) return;
  const SkewGeom g = a.g;
  const int X = g.X, Y = g.Y;
  constexpr bool BWD = OP == SW_BACKWARD;
  double* dst = OP == SW_FACTOR ? a.pre : a.out;
  for (int d = 0; d < X + Y - 1; ++d) {
    for (int yl = threadIdx.x; yl < Y; yl += 1024) {
      const int xl = d - yl;
      if (xl < 0 || xl >= X) continue;
      const int x = BWD ? X - 1 - xl : xl, y = BWD ? Y - 1 - yl : yl;
      const size_t i = skew_index(g, x, y);
      const uint8_t m = a.mask[i];
      if (OP == SW_FACTOR && !(m & CM_FLUID)) continue;
      double r = 0.0;
      if (m & CM_FLUID) {   // fluid cells are interior: the neighbours exist
        const size_t io = skew_index(g, BWD ? x + 1 : x - 1, y), in_ = skew_index(g, x, BWD ? y + 1 : y - 1);
        double own_val = OP == SW_FACTOR ? a.pre[io] : dst[io];
        double nb_val = OP == SW_FACTOR ? a.pre[in_] : dst[in_];
        double own_pre = OP == SW_FORWARD ? a.pre[io] : 0.0, nb_pre = OP == SW_FORWARD ? a.pre[in_] : 0.0;
        if (a.tile_w > 0) {   // tile-local IC(0): a cut coupling carries what the wavefront carries into a tile
          const int l = y & 63, t = x + l;
          const bool cut = (BWD ? t + 1 : t) % a.tile_w == 0;
          if (cut) { own_val = 0.0; own_pre = 1.0; }                                   // forward: (-1 * 1) * (+0) = -0.0
          if (cut || l == (BWD ? 63 : 0)) { nb_val = 0.0; nb_pre = 1.0; }
        }
        r = sweep_cell<OP>(m, OP == SW_FACTOR ? 0.0 : a.in[i], a.pre[i], own_val, own_pre, nb_val, nb_pre);
      }
      dst[i] = r;
    }
    __syncthreads();
  }
}

// --- production schedule: one workgroup per 64-row band = a compute wave + two helper waves ---------
// Compute wave.  Lane l owns row 64 b + l.  Forward: records t = 0, 1, ..., lane l is at column t - l,
// the row below arrives from lane l-1 (DPP wave_shr:1), the previous column is the lane's own
// register.  Backward: records T-1, T-2, ..., the row above arrives from lane l+1 (DPP wave_shl:1).
// The unit of work is 8 steps = one hand-off block, fully unrolled; records come in pairs (a lane's elements of
// records 2P, 2P+1 are adjacent), so every stream moves two steps per 16-byte access, and the operands of the
// next two or three blocks are in flight into rotating register sets while a block computes (fluid flags: 8
// steps to a dword).  A lone wave is bound by instruction ISSUE and by the latency of whatever it waits
// for, so the compute wave touches global memory only for its streams and everything about the band
// hand-off lives in the helper waves (own SIMDs, own vmcnt):
//   * the compute wave drops every step's carry row into an LDS ring (two rows per ds_write2st64_b64); the
//     ANNOUNCE wave gathers the edge lane's (63 forward / 0 backward: logical column s-63) values block by
//     block and publishes them to the next band as 16-byte granule pairs {lo, epoch, hi, epoch}
//     (write-through stores), up to 8 groups per store;
//   * the FETCH wave polls the previous band's granules with 4 loads in flight, each covering up to 8 blocks
//     ahead of the compute wave, and parks validated boundary values in a second LDS ring; the compute wave
//     reads a block's 8 values as broadcasts two steps before the previous block ends - they become the `old`
//     operand of the DPP shift, i.e. what the lane without a shift source receives.
// The waves talk through three monotonic LDS counters (blocks computed / boundary blocks deposited /
// groups announced); a wave's LDS operations execute in order, so "data, then counter" needs no fence.
// Bands take their order from a ticket, so a band only ever waits on a band that is already
// running: no residency assumption, no deadlock; every spin is bounded (sticky error -> ETIMEOUT).
// One band per workgroup (= per CU) on purpose: the CU's vector-memory path is shared - a second compute wave
// on the CU costs each +18 % per step, four run 2.2x slower (tools/micro/step_bench2).
// Measured and rejected: staging the compute wave's streams through LDS as well (a load wave feeding an
// operand ring by LDS-DMA, a store wave draining a result ring; the compute wave without any global access).
// A stand-alone model of the step promised 27 ns instead of 40; the real kernel, with its per-block
// bookkeeping and five waves on the CU, ran 40 ns/step for a lone band and 50-55 ns with neighbours, and the
// load wave could not keep the ring full from HBM at 8192^2 (1.6x slower sweeps).  Bit-exact, but not faster.
// Measured and rejected: placing consecutive bands on one XCD (every 8th workgroup) with write-through or
// with plain granule stores - the hand-off lag does not move (4.6-4.8 us per band either way).
// Measured and rejected at 8192^2 (per-step time there is ~1.25x / 1.4x that of an L2-resident grid):
// a fourth wave touching the coming records' cache lines 10 blocks ahead (L2 prefetch: no gain forward,
// 1.2x slower backward - the touches cross the same per-CU memory path), and padding the band stride
// against HBM channel aliasing (no effect).
// Measured and rejected (round 1, last experiment): polling through the SCALAR memory path.  tools/micro/poll_bench: one hop
// costs 480-640 ns with vector sc1 polls (more behind this kernel's deep prefetch queue: ~1.1 us), 450 ns with
// `s_load_dwordx4 glc` polls whatever the CU's vector traffic does, same- or cross-XCD (sc1 stores; sc0 loads and plain
// cross-XCD stores read stale).  But a scalar round trip carries at most ~256 B (64 SGPRs) = the granules of two blocks and
// must be retired whole (out-of-order returns): a single scalar poller delivered a block every ~400 ns, the compute wave
// needs one every 210-300 ns, and the sweeps ran 1.6x slower (72 -> 123 us).  What is left to try: two scalar pollers on
// alternate blocks (a fourth wave), or tag-free compact rows behind a drained progress word.
// Records t >= T of a band and the 32 records in front of each array are dead padding (mask 0):
// the loop runs whole groups of 3 blocks and prefetches unconditionally.
#define SW_BLK 8
#define SW_RING 64            // carry rows kept in LDS (8 blocks)
#define SW_BND_RING 16        // boundary blocks kept in LDS
#define SW_SPIN_LIMIT (1u << 22)
#ifndef SW_TRACE_HANDOFF
#define SW_TRACE_HANDOFF 0   // development build: time stamps of one hand-off (column block 40) in the timeline words 4..7
#endif
#define SW_TRACE_CB 40

struct SweepShared {
  double pub[SW_RING][64];            // carry rows of the last SW_RING steps (ring slot = step & 63)
  double bnd[SW_BND_RING][SW_BLK];    // boundary values, ring slot = (block - B0) & 15
  unsigned int dep_done, pub_done;    // helper -> compute: boundary blocks deposited, groups announced (one 8-byte read)
  unsigned int comp_done;             // compute -> helper: blocks computed
  unsigned int abort;
  int ord;
};
__device__ __forceinline__ unsigned int lds_get(const unsigned int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void lds_put(unsigned int* p, unsigned int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
#define SW_COMPILER_FENCE() asm volatile("" ::: "memory")

template <int OP, bool XG = false>
__global__ __launch_bounds__(192) void k_sweep_skew(SweepArgs a) {
  __shared__ SweepShared sh;
  const int lane = threadIdx.x & 63;
  const int role = threadIdx.x >> 6;                  // 0 compute, 1 announce, 2 fetch boundaries
  if (threadIdx.x == 0) {
    sh.ord = (int)(atomicAdd(a.ticket, 1u) - a.ticket_base);        // position in the band pipeline
    sh.dep_done = 0; sh.pub_done = 0; sh.comp_done = 0; sh.abort = 0;
  }
  __syncthreads();
  const int ord = __builtin_amdgcn_readfirstlane(sh.ord);
  if (!a.force && pcg_idle(a.sc)) return;
  const unsigned long long t_entry = wall_clock64();
  constexpr bool BWD = OP == SW_BACKWARD;
  constexpr int CTRL = BWD ? DPP_WAVE_SHL1 : DPP_WAVE_SHR1;
  constexpr int EDGE = BWD ? 0 : 63;                  // the lane whose results the next band needs
  const SkewGeom g = a.g;
  const int X = g.T - 63, T = g.T, TS = g.TS, nb = g.nbands;   // X: hand-off columns live in step space, [0, T - 63) (T is even: g.X or g.X + 1)
  // `ord` counts this launch's (= this rank's) bands in sweep order; gord is the position in the
  // global band pipeline, which also names the hand-off rows (forwarded rank to rank when coupled)
  const int band = BWD ? a.band_lo + a.nb_local - 1 - ord : a.band_lo + ord;
  const int gord = BWD ? nb - 1 - band : band;
  const bool has_prev = ord > 0 || (a.couple && gord > 0);            // a band before us in sweep order
  const bool publish = ord + 1 < a.nb_local || (a.couple && gord + 1 < nb);
  unsigned long long* gr_out = a.granules + (size_t)gord * a.gran_stride * 2;
  const unsigned long long* gr_in = a.granules + (size_t)(has_prev ? gord - 1 : 0) * a.gran_stride * 2;
  if (XG) {   // the band pipeline continues across GPUs: same granules, same epochs, system-scope accesses (below)
    if (ord + 1 == a.nb_local && gord + 1 < nb) gr_out = a.xg_out;
    if (ord == 0 && gord > 0) gr_in = a.xg_in;
  }

  // Active range (forward / backward solves only).  Outside the 32-step-aligned block range
  // [B0, B1) every cell of the band is non-fluid, so its results are constants that are already in
  // memory (q, z = +0, zeroed per solve) and the values it would hand on are CONST (z: +0; the
  // forward carry m = (-1*precon)*(+0) = -0.0).  The band runs only [B0, B1); an empty band returns at
  // once, and nobody waits for it.  The previous band's range tells which column blocks it
  // announces: [pB0 - 8, pB1 - 8); outside that window the consumer substitutes CONST and does
  // not poll.  The factor sweep always runs the full range (a stale precon is not a constant).
  constexpr bool RANGED = OP != SW_FACTOR;
  constexpr double CONST = OP == SW_FORWARD ? -0.0 : 0.0;
  constexpr int BODY_HALF = 4;                                          // blocks a range is a multiple of: the loop body
  const int full_blocks = BODY_HALF * (((T + SW_BLK - 1) / SW_BLK + BODY_HALF - 1) / BODY_HALF);
  const int ncolblk = (X + SW_BLK - 1) / SW_BLK;
  int B0 = 0, B1 = full_blocks, win_lo = 0, win_hi = ncolblk;
  if (RANGED && a.ranges) {
    const int4 mine = a.ranges[band];
    B0 = BWD ? mine.z : mine.x; B1 = BWD ? mine.w : mine.y;
    if (B0 >= B1) {                                    // no fluid in this band
      if (OP == SW_FORWARD && a.fin_qq >= 0 && role == 0) sweep_qq_arrive(a, ord, 0.0);
      return;
    }
    if (has_prev) {
      const int4 prv = a.ranges[BWD ? band + 1 : band - 1];
      const int pB0 = BWD ? prv.z : prv.x, pB1 = BWD ? prv.w : prv.y;
      win_lo = pB0 - 8 > 0 ? pB0 - 8 : 0;
      win_hi = pB1 - 8 < ncolblk ? pB1 - 8 : ncolblk;   // empty producer: win_hi <= win_lo
    }
  }
  const int NBLK = B1 - B0;
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

  // =========================== helper waves: the band hand-off ===================================
  // wave 1 announces this band's edge values to the next band, wave 2 fetches the previous band's
  if (role == 1) {
    if (!publish) return;
    const int t8 = lane >> 3, k8 = lane & 7;            // this lane serves group (next + t8), column k8 of it
    auto announce = [&](int col, double v, bool on) {
      if (on && col >= 0 && col < X) {
        const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
        const u32x4 gq = {(unsigned int)bits, a.epoch, (unsigned int)(bits >> 32), a.epoch};
        if (XG) asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" :: "v"(&gr_out[(size_t)col * 2]), "v"(gq) : "memory");
        else asm volatile("global_store_dwordx4 %0, %1, off sc1" :: "v"(&gr_out[(size_t)col * 2]), "v"(gq) : "memory");
      }
    };
    int next_pub = 0;                                   // groups announced so far (relative to B0)
    unsigned int spins = 0;
    while (next_pub < NBLK) {
      const int cdone = (int)lds_get(&sh.comp_done);
      SW_COMPILER_FENCE();
      if (next_pub < cdone) {
        // the group of block b = logical columns 8(b-8) .. 8(b-8)+7 of the edge row, produced in steps
        // 8b-1 .. 8b+6, is complete once block b is (up to 8 groups per pass)
        int n = cdone - next_pub; n = n < 8 ? n : 8;
        const int b = B0 + next_pub + t8;
        const double v = sh.pub[(SW_BLK * b - 1 + k8) & (SW_RING - 1)][EDGE];
        announce(SW_BLK * (b - 8) + k8, v, t8 < n);
        if (SW_TRACE_HANDOFF && lane == 0 && SW_TRACE_CB + 8 - B0 >= next_pub && SW_TRACE_CB + 8 - B0 < next_pub + n)
          a.timeline[(size_t)ord * 8 + 5] = wall_clock64();
        next_pub += n;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the ring rows are read: the compute wave may reuse them
        lds_put(&sh.pub_done, (unsigned int)next_pub);
        spins = 0;
        continue;
      }
      if (lds_get(&sh.abort)) return;
      if (++spins > (SW_SPIN_LIMIT << 3)) { if (lane == 0) atomicExch(a.error, 2); lds_put(&sh.abort, 1u); return; }
#ifdef SW_ANNOUNCE_SLEEP       // the announce wave yields while it has nothing to announce (tools/r03: sweep ablations)
      __builtin_amdgcn_s_sleep(SW_ANNOUNCE_SLEEP);
#endif
    }
    // The edge row's column of the very last step (8*B1 - 1) opens the group of a block that never runs.
    // The next band reads it only when X + 63 is a multiple of 16 (factor sweep: full range, full window).
    announce(SW_BLK * (B1 - 8), sh.pub[(SW_BLK * B1 - 1) & (SW_RING - 1)][EDGE], lane == 0);
    return;
  }
  if (role == 2) {
    if (!has_prev) return;
    // Four polls are kept in flight (re-issued as they are retired, so they space themselves a quarter
    // of a round trip apart): a granule is then seen about half a round trip after it lands instead
    // of one and a half.  Each poll covers up to 8 blocks from the deposit front at its issue; every
    // lane always loads (clamped address) so that the in-order vmcnt bookkeeping is exact.
    const int t8 = lane >> 3, k8 = lane & 7;            // this lane serves block (base + t8), column k8 of it
    int next_dep = 0;                                   // boundary blocks deposited so far (relative to B0)
    unsigned int spins = 0;
    struct Poll { u32x4 gv; int base, n; };
    Poll q0, q1, q2, q3;
    auto issue = [&](Poll& q) {
      const int cdone = (int)lds_get(&sh.comp_done);
      SW_COMPILER_FENCE();
      int n = cdone + SW_BND_RING - 2 - next_dep;               // ring slots the compute wave is done with
      n = n < NBLK - next_dep ? n : NBLK - next_dep;
      q.n = n < 8 ? n : 8; q.base = next_dep;
      const int blk = B0 + next_dep + t8, xl = SW_BLK * blk + k8;
      const bool want = t8 < q.n && blk >= win_lo && blk < win_hi && xl < X;
      const unsigned long long* p = &gr_in[want ? (size_t)xl * 2 : 0];
      if (XG) asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1" : "=&v"(q.gv) : "v"(p) : "memory");
      else asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=&v"(q.gv) : "v"(p) : "memory");
    };
    auto retire = [&](Poll& q) {                        // the oldest of the four polls in flight
      asm volatile("s_waitcnt vmcnt(3)" : "+v"(q.gv) :: "memory");
      const int blk = B0 + q.base + t8, xl = SW_BLK * blk + k8;
      const bool mine = t8 < q.n;
      const bool want = mine && blk >= win_lo && blk < win_hi && xl < X;   // else: nothing is announced there, CONST
      const bool ready = mine && (!want || (q.gv[1] == a.epoch && q.gv[3] == a.epoch));
      const unsigned long long notready = ~__ballot(ready);
      const int m = notready ? (__ffsll((long long)notready) - 1) >> 3 : 8;      // leading blocks whose 8 columns are all there
      const int fresh0 = next_dep - q.base;                                        // blocks a younger poll's elder already deposited
      if (m > fresh0) {
        if (t8 >= fresh0 && t8 < m) sh.bnd[(q.base + t8) & (SW_BND_RING - 1)][k8] = want ? __hiloint2double((int)q.gv[2], (int)q.gv[0]) : CONST;
        SW_COMPILER_FENCE();
        if (SW_TRACE_HANDOFF && lane == 0 && SW_TRACE_CB - B0 >= next_dep && SW_TRACE_CB - B0 < q.base + m)
          a.timeline[(size_t)ord * 8 + 6] = wall_clock64();
        next_dep = q.base + m;
        lds_put(&sh.dep_done, (unsigned int)next_dep);
        spins = 0;
      } else {
        ++spins;
      }
    };
    issue(q0); issue(q1); issue(q2); issue(q3);
    while (next_dep < NBLK) {
      retire(q0); issue(q0);
      retire(q1); issue(q1);
      retire(q2); issue(q2);
      retire(q3); issue(q3);
#ifdef SW_FETCH_SLEEP          // fewer polls per microsecond (tools/r03: sweep ablations)
      __builtin_amdgcn_s_sleep(SW_FETCH_SLEEP);
#endif
      if (lds_get(&sh.abort) || spins > SW_SPIN_LIMIT) break;
    }
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(q0.gv), "+v"(q1.gv), "+v"(q2.gv), "+v"(q3.gv) :: "memory");   // before their registers are reused
    if (spins > SW_SPIN_LIMIT) { if (lane == 0) atomicExch(a.error, 2); lds_put(&sh.abort, 1u); }
    return;
  }

  // ====================================== compute wave ========================================
  unsigned int stalls = 0;
  // Per-lane stream pointers at (this band, first record pair of the range, this lane).  Records come in
  // pairs (euler_dev.h): a lane's elements of records 2P and 2P+1 are adjacent, so ONE 16-byte access per
  // stream serves two steps - a lone wave pays per memory instruction (~16 cycles each whatever the width).
  // A block = 8 steps = 4 pairs = 4 KB per 8-byte stream; pair p of the block is addressed with the
  // immediate offset p * PSTEP (backward: descending).  T is even, so the backward sweep starts on the odd
  // record of a pair: step 2p is the pair's odd element (.y), step 2p+1 its even one (.x).
  constexpr int PSTEP = BWD ? -1024 : 1024;           // bytes from pair to pair for an 8-byte stream
  const size_t pair0 = (size_t)band * TS * 64 + (size_t)(BWD ? T - 2 - SW_BLK * B0 : SW_BLK * B0) * 64 + 2 * lane;   // element index
  const char* p_in = reinterpret_cast<const char*>((OP == SW_FACTOR ? a.pre : a.in) + pair0);   // operands of the block being prefetched
  const char* p_pre = reinterpret_cast<const char*>(a.pre + pair0);
  const char* p_msk = reinterpret_cast<const char*>(a.mask + pair0);      // factor: 2 mask bytes per pair
  const unsigned int* p_fb = (BWD ? a.fbits_bwd : a.fbits_fwd) + ((size_t)band * a.fb_stride + B0) * 64 + lane;
  char* p_out = reinterpret_cast<char*>((OP == SW_FACTOR ? a.pre : a.out) + pair0);   // results of the block being computed

  // Operand sets in rotation: while block k computes from one set, the records of the next DIST blocks are in
  // flight into the others (HBM latency under load exceeds one block time).  Forward and backward: four sets, distance 3
  // (round 1's backward sweep streamed its coefficients {a_i precon, a_j precon} as a third and fourth 16-byte load per pair
  // and had registers for three sets only; round 2 rebuilds them from precon and two flag bits: 2 loads per pair like the
  // forward sweep, 16 B per cell less traffic, and room for the fourth set).  Factor: two sets, distance 1 (compiler-managed loads).
  constexpr int DIST = OP == SW_FACTOR ? 1 : 3;
  struct Operands { sw_d2 in[4], pre[4]; int m[4]; unsigned int fb; };    // per pair: .x = even record, .y = odd record
  Operands opA, opB, opC, opD;
  // forward / backward: the record loads are issued BY HAND (inline asm) and retired by counted
  // s_waitcnt in front of each pair of steps.  hipcc's own wait insertion loses track of the issue order at
  // control-flow joins and then waits for every operation older than this block's loads -
  // including the result stores issued a few cycles earlier, i.e. a store round trip per block.
  // Memory operations of a wave retire in issue order, and the order here is fixed by construction:
  //     fetch(k):   fb, then per pair p the LOADS_PER_PAIR loads          (LOADS = 4 * LOADS_PER_PAIR + 1)
  //     compute(k): one 16-byte result store behind each pair of steps
  //   => before pair p of block k everything up to the pair's last load is needed, and behind it were issued
  //      (3 - p) * LOADS_PER_PAIR loads of fetch(k), then per block of prefetch distance [4 older stores and] one
  //      whole fetch, and p stores: vmcnt((3 - p) * LOADS_PER_PAIR + DIST * LOADS + p) is exact for the first
  //      blocks and never waits for a younger fetch.
  // tools/check_sweep_isa.py proves on the generated ISA that no in-flight operand is ever touched.
  constexpr int LOADS_PER_PAIR = 2;
  constexpr int LOADS = 4 * LOADS_PER_PAIR + 1;
  auto fetch_block = [&](Operands& o) {
    if constexpr (OP == SW_FACTOR) {
#pragma unroll
      for (int pp = 0; pp < 4; ++pp) {
        o.in[pp] = sw_d2{0.0, 0.0};
        o.pre[pp] = *reinterpret_cast<const sw_d2*>(p_pre + pp * PSTEP);
        o.m[pp] = (int)*reinterpret_cast<const unsigned short*>(p_msk + pp * (PSTEP / 8));   // the two cell-mask bytes of the pair
      }
      o.fb = 0u;
    } else {
      // only the flags, 8 steps to a dword (bits 0-7 fluid; backward: bits 8-15 fluid to the right, 16-23 fluid above) - a byte
      // load per step costs as much as the rest of the step
      asm volatile("global_load_dword %0, %1, off" : "=&v"(o.fb) : "v"(p_fb) : "memory");
#define SW_LOAD_PAIR(P)                                                                                                     \
      asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=&v"(o.in[P]) : "v"(p_in), "n"((P) * PSTEP));             \
      asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=&v"(o.pre[P]) : "v"(p_pre), "n"((P) * PSTEP));           \
      o.m[P] = 0;
      SW_LOAD_PAIR(0) SW_LOAD_PAIR(1) SW_LOAD_PAIR(2) SW_LOAD_PAIR(3)
#undef SW_LOAD_PAIR
      asm volatile("" ::: "memory");
    }
    p_in += 4 * PSTEP; p_pre += 4 * PSTEP; p_msk += 4 * (PSTEP / 8); p_fb += 64;
  };

  // wait (rarely) until the helper's counter reaches `target`
  auto await = [&](const unsigned int* cnt, int target) {
    ++stalls;
    for (unsigned int spins = 0; (int)lds_get(cnt) < target;) {
      if (lds_get(&sh.abort)) break;
      if (++spins > SW_SPIN_LIMIT) { if (lane == 0) atomicExch(a.error, 2); lds_put(&sh.abort, 1u); break; }
      __builtin_amdgcn_s_sleep(1);
    }
    SW_COMPILER_FENCE();
  };

  // Steady state is straight-line code: a lone wave pays ~30 cycles for every taken branch, so the
  // per-band facts (is there a band before us / after us) select one of four instantiations of the loop.
  unsigned long long t_first = 0;
  double qq = 0.0;           // forward: the lane's share of dot(q, q)
  auto sweep = [&](auto hp_c, auto pb_c) {
    constexpr bool HP = decltype(hp_c)::value;    // a band before us in sweep order: boundary values from the helper
    constexpr bool PB = decltype(pb_c)::value;    // a band after us: carry rows for the helper
    fetch_block(opA);                             // (per instantiation: an in-flight operand must never be copied)
    if (DIST >= 2) fetch_block(opB);
    if (DIST >= 3) fetch_block(opC);
    // Loop-carried state.  What travels between cells is, per operation:
    //   factor   : precon itself (left neighbour = own register, lower neighbour = lane-1)
    //   forward  : m = (-1*precon)*q of a cell - exactly the term its right neighbour (same lane, next
    //              step) AND its upper neighbour (lane+1, next step) subtract (main.c:607-609), so it
    //              is formed once and shifted; the precon of the lower row is never loaded
    //   backward : z (the coefficients belong to the consuming cell, main.c:620-622)
    double own = CONST;      // carried value of the previous column of this row
    qq = 0.0;
    double out = CONST;      // carried value this lane hands to the next lane
    // boundary values of the block about to run / of the one after it (what the lane without a shift source
    // receives); two sets like the operands, so that the next block's are read half a block ahead
    double beA[SW_BLK], beB[SW_BLK];
    auto read_boundary = [&](int rel, double (&be)[SW_BLK]) {
      const double* slot = sh.bnd[rel & (SW_BND_RING - 1)];
#pragma unroll
      for (int j = 0; j < SW_BLK; ++j) be[j] = HP ? slot[j] : CONST;
    };
    if (PB) sh.pub[(SW_BLK * B0 - 1) & (SW_RING - 1)][lane] = CONST;   // "step B0*8 - 1": the band was all non-fluid before its range
    if (HP) await(&sh.dep_done, 1);
    read_boundary(0, beA);
    t_first = wall_clock64();

    // one hand-off block = 8 steps: compute from `cur`, refill `nxt` with the block after the next
    auto run_block = [&](int blk, Operands& cur, Operands& nxt, double (&be)[SW_BLK], double (&be_next)[SW_BLK]) {
      const int rel = blk - B0;
      fetch_block(nxt);
      // the helpers' progress, read well ahead of its use: boundary blocks deposited, groups announced
      unsigned long long prog = 0;
      if (HP || PB) prog = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(&sh.dep_done), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      // Pin the software pipeline: all loads of block blk+1 are issued here, ahead of the compute phase
      // (left alone, hipcc's scheduler sinks them between the steps and waits for them a few
      // instructions later; measured 1.4-2x slower per step).
      __builtin_amdgcn_sched_barrier(0);
      double* ring = &sh.pub[(SW_BLK * blk) & (SW_RING - 1)][lane];
      double prev_carry = CONST, prev_res = 0.0;
      auto step = [&](auto jc) {
        constexpr int j = decltype(jc)::value;
        constexpr int P = j >> 1;                         // the pair of records this step belongs to
        constexpr bool ODD = ((j & 1) != 0) != BWD;       // does the step use the pair's odd record (.y)?
        if constexpr (OP != SW_FACTOR && (j & 1) == 0) {  // retire this pair's records (see fetch_block)
          constexpr int N0 = (3 - P) * LOADS_PER_PAIR + DIST * LOADS + P, N = N0 < 63 ? N0 : 63;
          asm volatile("s_waitcnt vmcnt(%3)" : "+v"(cur.in[P]), "+v"(cur.pre[P]), "+v"(cur.fb) : "n"(N) : "memory");
        }
        // the edge lane consumes logical column s = 8*blk + j of the previous band
        const double nbv = wave_shift_inject<CTRL>(out, be[j]);   // 2 DPP moves
        const double cin = ODD ? cur.in[P].y : cur.in[P].x, cpre = ODD ? cur.pre[P].y : cur.pre[P].x;
        // sign-extended fluid flag (0 / -1): masking is two v_and
        const int cm = OP == SW_FACTOR ? ((cur.m[P] >> (ODD ? 8 : 0)) & 0xff) : ((int)(cur.fb << (31 - j)) >> 31);
        double res, carry;
        if (OP == SW_FACTOR) {               // main.c:586-600; own / nbv are precon of the left / lower cell
          const double aa = (double)(cm >> CM_DIAG_SHIFT);
          const double cl = -1.0 * own, cb = -1.0 * nbv;
          double e = aa - cl * cl - cb * cb;
          if (e < 0.25 * aa) e = (aa != 0.0) ? aa : 1.0;
          res = (cm & CM_FLUID) ? 1.0 / sqrt(e) : cpre;      // non-fluid: the stale entry stays
          carry = res;
        } else if (OP == SW_FORWARD) {       // main.c:602-613: t = r - (-1*pre_l)*q_l - (-1*pre_b)*q_b
          const double t = cin - own - nbv;
          const double qv = t * cpre;
          res = __hiloint2double(__double2hiint(qv) & cm, __double2loint(qv) & cm);   // +0 on non-fluid cells
          carry = -1.0 * cpre * res;         // this cell's term in its right and upper neighbours
          qq = __builtin_fma(res, res, qq);  // dot(q, q) = dot(z, r) (SweepArgs::fin_qq): one instruction, not part of the bit-exact arithmetic
        } else {                             // main.c:615-626: t = q - (a_i*pre)*z_r - (a_j*pre)*z_u
          // the cell's coefficients a_i precon, a_j precon (main.c:621-622), a = -1 / 0 by the fluid flag of the right / upper
          // neighbour: (-1.0 or +0.0) * precon, the reference's product, from two sign-extended flag bits (off the carried chain)
          const int fr = (int)(cur.fb << (23 - j)) >> 31, fu = (int)(cur.fb << (15 - j)) >> 31;
          const double kr = __hiloint2double((int)0xBFF00000 & fr, 0) * cpre, ku = __hiloint2double((int)0xBFF00000 & fu, 0) * cpre;
          const double t = cin - kr * own - ku * nbv;
          const double zv = t * cpre;
          res = __hiloint2double(__double2hiint(zv) & cm, __double2loint(zv) & cm);   // +0 on non-fluid cells
          carry = res;
        }
        // the pair's two results leave with one 16-byte store behind its second step ({even, odd} record order)
        if (j & 1) *reinterpret_cast<sw_d2*>(p_out + P * PSTEP) = BWD ? sw_d2{res, prev_res} : sw_d2{prev_res, res};
        prev_res = res;
        own = carry;
        out = carry;
        // the announce wave gathers the edge lane's entry; two rows per LDS instruction (ds_write2st64_b64)
        if (PB && (j & 1)) { ring[(j - 1) * 64] = prev_carry; ring[j * 64] = carry; }
        prev_carry = carry;
      };
      step(std::integral_constant<int, 0>()); step(std::integral_constant<int, 1>()); step(std::integral_constant<int, 2>());
      step(std::integral_constant<int, 3>());
      step(std::integral_constant<int, 4>()); step(std::integral_constant<int, 5>());
      if (HP) {
        // two steps before the block ends (an LDS round trip): the next block's boundary values (deposited once
        // dep_done > rel+1; past the range: whatever is there).  A starved wave waits here, as late as possible.
        if (__builtin_expect(rel + 1 < NBLK && (int)(unsigned int)prog < rel + 2, 0)) await(&sh.dep_done, rel + 2);
        read_boundary(rel + 1, be_next);
        if (SW_TRACE_HANDOFF && blk + 1 == SW_TRACE_CB && lane == 0) a.timeline[(size_t)ord * 8 + 7] = wall_clock64();
      }
      step(std::integral_constant<int, 6>()); step(std::integral_constant<int, 7>());
      __builtin_amdgcn_sched_barrier(0);
      p_out += 4 * PSTEP;
      if (HP || PB) { SW_COMPILER_FENCE(); lds_put(&sh.comp_done, (unsigned int)(rel + 1)); }
      if (SW_TRACE_HANDOFF && blk == SW_TRACE_CB + 8 && lane == 0) a.timeline[(size_t)ord * 8 + 4] = wall_clock64();
      // block blk+1 overwrites the ring rows of block blk-7, which the groups up to block blk-6 read
      // (announced once pub_done >= rel-5)
      if (PB && __builtin_expect(rel + 1 < NBLK && (int)(unsigned int)(prog >> 32) < rel - 5, 0)) await(&sh.pub_done, rel - 5);
    };

    // At block k the wave computes from set k mod (DIST + 1) and refills the set of block k - 1.  The body is 4 blocks
    // and the ranges are multiples of 4 in every sweep.  (A mid-body exit is correct too, but hipcc then merges the tails of
    // the rare wait paths and tools/check_sweep_isa.py, which follows every branch both ways, can no longer prove it.)
    for (int blk = B0; blk < B1; blk += 4) {
      if (DIST == 3) {          // forward, backward: four sets
        run_block(blk, opA, opD, beA, beB);
        run_block(blk + 1, opB, opA, beB, beA);
        run_block(blk + 2, opC, opB, beA, beB);
        run_block(blk + 3, opD, opC, beB, beA);
      } else {                  // factor: two sets
        run_block(blk, opA, opB, beA, beB);
        run_block(blk + 1, opB, opA, beB, beA);
        run_block(blk + 2, opA, opB, beA, beB);
        run_block(blk + 3, opB, opA, beB, beA);
      }
    }
    // retire the prefetch that ran past the range before anything else reuses its registers (the kernel
    // end would wait for it anyway; it also keeps tools/check_sweep_isa.py's path exploration exact)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  };
  typedef std::integral_constant<bool, true> yes_t;
  typedef std::integral_constant<bool, false> no_t;
  if (has_prev) { if (publish) sweep(yes_t(), yes_t()); else sweep(yes_t(), no_t()); }
  else          { if (publish) sweep(no_t(), yes_t()); else sweep(no_t(), no_t()); }
  if (OP == SW_FORWARD && a.fin_qq >= 0) sweep_qq_arrive(a, ord, qq);
  if (lane == 0) {
    unsigned long long* tl = a.timeline + (size_t)ord * 8;
    tl[0] = t_entry; tl[1] = t_first; tl[2] = wall_clock64(); tl[3] = ((unsigned long long)(B1 - B0) << 32) | stalls;
  }
}

// ==========================================================================================
// host-side launch helpers
static SweepArgs make_sweep_args(euler_sim* S, int op, int force) {
  SweepArgs a;
  a.g = S->geom;
  a.mask = S->cellmask; a.fbits_fwd = S->fbits_fwd; a.fbits_bwd = S->fbits_bwd; a.fb_stride = S->fb_stride; a.pre = S->precon;
  a.in = op == SW_FORWARD ? S->r : S->q;
  a.out = op == SW_FORWARD ? S->q : S->z;
  a.granules = S->granules; a.gran_stride = S->gran_stride; a.ticket = S->ticket;
  a.xg_in = nullptr; a.xg_out = nullptr;
  a.ranges = S->band_ranges;
  a.band_lo = S->band_lo; a.nb_local = S->band_hi - S->band_lo; a.couple = S->has_comm && S->couple;
  a.ticket_base = S->ticket_base; a.epoch = S->epoch;
  a.sc = S->sc; a.force = force; a.error = &S->ms->error;
  a.timeline = S->sweep_timeline;
  a.tile_w = eu_is_tile(S) ? S->tile_w : 0;
  a.fin_qq = -1; a.qq_partial = S->partial; a.qq_counter = S->red_counter; a.sc_w = S->sc;
  return a;
}

// ---- active ranges of the bands (per solve) ---------------------------------------------------
// For each 64-row band: the first / last record t = x + lane that holds a fluid cell, turned into
// 32-step aligned block ranges of the forward (step = t) and backward (step = T-1-t) sweeps; the
// upper end leaves at least one all-non-fluid step inside the range (see k_sweep_skew).  Computed
// from the row-major count grid, which every rank holds in full.
__global__ __launch_bounds__(1024) void k_band_ranges(const uint8_t* __restrict__ count, int X, int Y, int T, int4* __restrict__ ranges, int band0) {
  __shared__ int s_lo, s_hi;
  const int band = band0 + blockIdx.x;
  if (threadIdx.x == 0) { s_lo = 0x7fffffff; s_hi = -1; }
  __syncthreads();
  int lo = 0x7fffffff, hi = -1;
  const int rows = Y - band * 64 < 64 ? Y - band * 64 : 64;
  for (int x = threadIdx.x; x < X; x += 1024) {
    for (int l0 = 0; l0 < rows; l0 += 8) {          // 8 independent loads in flight per thread
      uint8_t c[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) c[k] = l0 + k < rows ? count[(size_t)(band * 64 + l0 + k) * X + x] : (uint8_t)0;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (c[k]) { const int t = x + l0 + k; lo = t < lo ? t : lo; hi = t > hi ? t : hi; }
    }
  }
  if (hi >= 0) { atomicMin(&s_lo, lo); atomicMax(&s_hi, hi); }
  __syncthreads();
  if (threadIdx.x == 0) {
    int4 r = make_int4(0, 0, 0, 0);
    if (s_hi >= 0) {
      const int f0 = s_lo / 32 * 32, f1 = (s_hi + 2 + 31) / 32 * 32;                       // forward steps [f0, f1): whole groups of 4 blocks
      const int b0 = (T - 1 - s_hi) / 32 * 32, b1 = (T - 1 - s_lo + 2 + 31) / 32 * 32;     // backward steps [b0, b1): whole groups of 4 blocks
      r = make_int4(f0 / 8, f1 / 8, b0 / 8, b1 / 8);
    }
    ranges[band] = r;
  }
}
// flags of the sweeps, 8 steps to a dword: word (band, g, lane) bit j = fluid flag of the lane's cell in step 8g + j
// of the forward sweep (record 8g + j) / of the backward sweep (record T-1 - 8g - j); 0 outside [0, T).  The backward word
// also carries the cell's CM_RIGHT (bits 8-15) and CM_UP (bits 16-23) flags
__global__ __launch_bounds__(256) void k_pack_fbits(const uint8_t* __restrict__ cellmask, SkewGeom g, unsigned int* __restrict__ fwd,
                                                    unsigned int* __restrict__ bwd, int fb_stride, int band_lo, int nb_local) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)nb_local * fb_stride * 64) return;
  const int lane = (int)(i & 63);
  const int gi = (int)((i >> 6) % fb_stride), band = band_lo + (int)((i >> 6) / fb_stride);
  const uint8_t* base = cellmask + (size_t)band * g.TS * 64 + 2 * lane;   // paired records: (t & ~1) * 64 + 2 * lane + (t & 1)
  unsigned int wf = 0, wb = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int tf = 8 * gi + j, tb = g.T - 1 - 8 * gi - j;
    if (tf < g.T && (base[(size_t)(tf & ~1) * 64 + (tf & 1)] & CM_FLUID)) wf |= 1u << j;
    if (tb >= 0) {      // backward: the cell's fluid flag and the two neighbour flags its coefficients are built from
      const unsigned int m = base[(size_t)(tb & ~1) * 64 + (tb & 1)];
      if (m & CM_FLUID) wb |= 1u << j;
      if (m & CM_RIGHT) wb |= 1u << (8 + j);
      if (m & CM_UP) wb |= 1u << (16 + j);
    }
  }
  const size_t o = ((size_t)band * fb_stride + gi) * 64 + lane;
  fwd[o] = wf; bwd[o] = wb;
}
int eu_launch_band_ranges(euler_sim* S) {
  if (eu_is_tile(S)) return EULER_OK;   // no band pipeline, no packed flags: k_precond_tile reads the cell mask
  // a rank needs the ranges of its own bands and of the band before / after its slab (the hand-off windows)
  const bool nbrs = S->has_comm && S->couple && !S->slab_on;   // (a row-slab handle does not hold the neighbours' count rows)
  const int b0 = nbrs && S->band_lo > 0 ? S->band_lo - 1 : S->band_lo, b1 = nbrs && S->band_hi < S->geom.nbands ? S->band_hi + 1 : S->band_hi;
  LAUNCH(S, KC_BUILD_SYSTEM, k_band_ranges, dim3(b1 - b0), dim3(1024), S->count, S->X, S->Y, S->geom.T, S->band_ranges, b0);
  const int nbl = S->band_hi - S->band_lo;
  const size_t n = (size_t)nbl * S->fb_stride * 64;
  LAUNCH(S, KC_BUILD_SYSTEM, k_pack_fbits, dim3((unsigned)((n + 255) / 256)), dim3(256), S->cellmask, S->geom, S->fbits_fwd, S->fbits_bwd,
         S->fb_stride, S->band_lo, nbl);
  return EULER_OK;
}

int eu_launch_sweep(euler_sim* S, int op, int cls, int force, int fin_qq) {
  typedef void (*Kernel)(SweepArgs);
  static const Kernel simple[3] = {k_sweep_simple<SW_FACTOR>, k_sweep_simple<SW_FORWARD>, k_sweep_simple<SW_BACKWARD>};
  static const Kernel skew[3] = {k_sweep_skew<SW_FACTOR>, k_sweep_skew<SW_FORWARD>, k_sweep_skew<SW_BACKWARD>};
  static const Kernel skew_xg[3] = {k_sweep_skew<SW_FACTOR, true>, k_sweep_skew<SW_FORWARD, true>, k_sweep_skew<SW_BACKWARD, true>};
  if (S->cfg.sweep_mode == EULER_SWEEP_SIMPLE) {
    LAUNCH(S, cls, simple[op], dim3(1), dim3(1024), make_sweep_args(S, op, force));
    return EULER_OK;
  }
  const bool BWD = op == SW_BACKWARD;
  const int nb = S->geom.nbands, nbl = S->band_hi - S->band_lo;
  const bool chain = S->has_comm && S->couple;
  const int64_t row_bytes = (int64_t)S->gran_stride * 2 * 8;
  // global pipeline positions of my first / last band in sweep order
  const int g_first = BWD ? nb - S->band_hi : S->band_lo, g_last = g_first + nbl - 1;
  const int r = S->comm.rank, prev_rank = BWD ? r + 1 : r - 1, next_rank = BWD ? r - 1 : r + 1;
  S->epoch += 1;
  if (chain && S->p2p_on) {
    // exact coupling over the mailboxes: all slabs launch at once and the band pipeline runs on across the GPUs -
    // the previous slab's last band announces straight into this rank's mailbox while this kernel is running
    SweepArgs a = make_sweep_args(S, op, force);
    eu_p2p_xgran(S, BWD ? 1 : 0, &a.xg_in, &a.xg_out);
    LAUNCH(S, cls, skew_xg[op], dim3(nbl), dim3(192), a);
    S->ticket_base += (unsigned)nbl;
    return EULER_OK;
  }
  if (chain && g_first > 0)   // the edge row of the band before mine arrives from the previous slab
    COMM_CALL(S->comm.chain(S->comm.ctx, S->granules + (size_t)(g_first - 1) * S->gran_stride * 2, row_bytes, prev_rank, r));
  SweepArgs a = make_sweep_args(S, op, force);
  a.fin_qq = fin_qq;
  LAUNCH(S, cls, skew[op], dim3(nbl), dim3(192), a);
  S->ticket_base += (unsigned)nbl;
  if (chain && g_last + 1 < nb)
    COMM_CALL(S->comm.chain(S->comm.ctx, S->granules + (size_t)g_last * S->gran_stride * 2, row_bytes, r, next_rank));
  return EULER_OK;
}
