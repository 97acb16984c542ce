// k_observe.hip — the host side that the read-only observer passes share (k_overview.hip, k_diagnostics.hip, k_viewport.hip;
// docs/observer_passes.md): a pass enters, reserves its device buffer, launches, and reads back.  The device side is k_observe.h; what a row-slab handle adds
// between the launch and the read-back - the all-gather of the ranks' partial records and their fold - is k_observe_slab.hip.
#include "euler_dev.h"

// the checks every pass makes first, in this order; its own (raster, scale, byte count) come behind.  All of them depend on the arguments and on facts every rank
// of a row-slab job shares, so there every rank refuses alike, before any exchange
int eu_observe_enter(const euler_sim* S, const char* who, const char* slab_reason, const void* out, int x0, int y0, int x1, int y1) {
  if (!S || !out) { eu_set_error("%s: null argument", who); return EULER_EINVAL; }
  if (S->slab_on && slab_reason) { eu_set_error("%s: not on a row-slab handle (%s)", who, slab_reason); return EULER_ESTATE; }
  if (S->slab_on && !S->has_comm) { eu_set_error("%s: row-slab handle without a communicator", who); return EULER_ESTATE; }      // (a pass that runs on slabs is collective there)
  if (!S->loaded) { eu_set_error("%s: no scenario loaded", who); return EULER_ESTATE; }
  if (x0 < 1 || y0 < 1 || x1 > S->X - 2 || y1 > S->Y - 2 || x0 > x1 || y0 > y1) {
    eu_set_error("%s: box [%d, %d] x [%d, %d] is not inside the interior [1, %d] x [1, %d]", who, x0, x1, y0, y1, S->X - 2, S->Y - 2);
    return EULER_EINVAL;
  }
  return EULER_OK;
}

// room for `bytes`: allocated by the first call, grown on demand and never shrunk; the old buffer is freed behind whatever of the stream still reads it
int eu_devbuf_reserve(euler_sim* S, const char* who, const char* what, eu_devbuf* b, size_t bytes) {
  if (bytes <= b->bytes) return EULER_OK;
  void* nb = nullptr;
  if (hipMalloc(&nb, bytes) != hipSuccess) {
    (void)hipGetLastError();
    eu_set_error("%s: %zu bytes of device memory for %s", who, bytes, what);
    return EULER_ENOMEM;
  }
  if (b->p) HIPCHK(hipStreamSynchronize(S->stream));
  eu_devbuf_release(S, b);
  b->p = nb; b->bytes = bytes;
  S->hbm_bytes += bytes;
  return EULER_OK;
}

void eu_devbuf_release(euler_sim* S, eu_devbuf* b) {
  if (b->p) (void)hipFree(b->p);
  S->hbm_bytes -= b->bytes;
  b->p = nullptr; b->bytes = 0;
}

int eu_observe_readback(euler_sim* S, void* out, const eu_devbuf* b, size_t bytes) {
  HIPCHK(hipMemcpyAsync(out, b->p, bytes, hipMemcpyDeviceToHost, S->stream));
  HIPCHK(hipStreamSynchronize(S->stream));
  return EULER_OK;
}
