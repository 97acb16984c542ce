// k_observe.hip — the host side that the read-only observer passes share (k_overview.hip, k_diagnostics.hip, k_viewport.hip;
// docs/observer_passes.md): a pass enters, reserves its device buffer, launches, and reads back.  The device side is k_observe.h; what a row-slab handle adds
// between the launch and the read-back - the all-gather of the ranks' partial records and their fold - is k_observe_slab.hip.
#include "euler_dev.h"
#include "k_boxes.h"

#include <stdlib.h>
#include <string.h>

// the checks every pass makes first, in this order; its own (raster, scale, byte count) come behind.  All of them depend on the arguments and on facts every rank
// of a row-slab job shares, so there every rank refuses alike, before any exchange
int eu_observe_enter(const euler_sim* S, const char* who, const char* slab_reason, const void* out, int x0, int y0, int x1, int y1) {
  if (!S || !out) { eu_set_error("%s: null argument", who); return EULER_EINVAL; }
  if (S->slab_on && slab_reason) { eu_set_error("%s: not on a row-slab handle (%s)", who, slab_reason); return EULER_ESTATE; }
  if (S->slab_on && !S->has_comm) { eu_set_error("%s: row-slab handle without a communicator", who); return EULER_ESTATE; }      // (a pass that runs on slabs is collective there)
  if (!S->loaded) { eu_set_error("%s: no scenario loaded", who); return EULER_ESTATE; }
  if (!eu_interior_box_ok(x0, y0, x1, y1, S->X, S->Y)) {
    eu_set_error("%s: box [%d, %d] x [%d, %d] is not inside the interior [1, %d] x [1, %d]", who, x0, x1, y0, y1, S->X - 2, S->Y - 2);
    return EULER_EINVAL;
  }
  return EULER_OK;
}

// room for `bytes`: allocated by the first call, grown on demand and never shrunk; the first `keep` bytes of the old buffer move over bit for bit, and the old buffer
// is freed behind whatever of the stream still reads it.  The new block is recorded before the old one goes: a failure leaves buffer and ledger as they were
int eu_devbuf_reserve(euler_sim* S, const char* who, const char* what, eu_devbuf* b, size_t bytes, size_t keep) {
  if (bytes <= b->bytes) return EULER_OK;
  void* nb = nullptr;
  if (eu_dev_alloc(S, &nb, bytes, EU_MEM_HANDLE, EU_DEV_QUIET)) {
    eu_set_error("%s: %zu bytes of device memory for %s", who, bytes, what);
    return EULER_ENOMEM;
  }
  if (keep && hipMemcpyAsync(nb, b->p, keep, hipMemcpyDeviceToDevice, S->stream) != hipSuccess) {
    (void)hipGetLastError(); (void)eu_dev_free(S, nb);
    eu_set_error("%s: the records could not be moved", who);
    return EULER_EHIP;
  }
  if (b->p) {
    const hipError_t e = hipStreamSynchronize(S->stream);
    if (e != hipSuccess) { (void)eu_dev_free(S, nb); return eu_hip_fail(e, "hipStreamSynchronize", __FILE__, __LINE__); }
  }
  (void)eu_dev_free(S, b->p);
  b->p = nb; b->bytes = bytes;
  return EULER_OK;
}

int eu_observe_readback(euler_sim* S, void* out, const eu_devbuf* b, size_t bytes) {
  HIPCHK(hipMemcpyAsync(out, b->p, bytes, hipMemcpyDeviceToHost, S->stream));
  HIPCHK(hipStreamSynchronize(S->stream));
  return EULER_OK;
}

// a list of boxes with its tile table (k_boxes.h): built on the host, then up in one copy
int eu_box_table_upload(euler_sim* S, const char* who, eu_devbuf* buf, const void* boxes, int32_t n, size_t box_bytes, int32_t max_boxes, unsigned int* ntiles) {
  const size_t head = (size_t)max_boxes * box_bytes;      // (1536 bytes for either list: the table stays 8-byte aligned)
  // (a row-slab handle keeps the entries of its own bands: a tile belongs to one rank.  Its table may be empty - the callers launch nothing then)
  const int b_lo = S->slab_on ? S->band_lo : 0, b_hi = S->slab_on ? S->band_hi : (S->Y + 63) >> 6;
  const size_t nt = eu_force_tiles_bands(boxes, box_bytes, n, S->X, S->Y, b_lo, b_hi, nullptr);
  const size_t bytes = head + (nt == (size_t)-1 ? 0 : nt) * sizeof(eu_force_tile);
  char* st = nt == (size_t)-1 ? nullptr : (char*)calloc(1, bytes);
  if (!st || eu_force_tiles_bands(boxes, box_bytes, n, S->X, S->Y, b_lo, b_hi, (eu_force_tile*)(st + head)) != nt) {
    free(st);
    eu_set_error("%s: host memory for the tile table", who);
    return EULER_ENOMEM;
  }
  memcpy(st, boxes, (size_t)n * box_bytes);
  int rc = eu_devbuf_reserve(S, who, "the boxes and the tile table", buf, bytes);
  if (!rc) {      // (the copy queues behind the substeps that still read the old table; the host's copy is freed once it has gone up)
    const hipError_t e1 = hipMemcpyAsync(buf->p, st, bytes, hipMemcpyHostToDevice, S->stream), e2 = hipStreamSynchronize(S->stream);
    if (e1 != hipSuccess || e2 != hipSuccess) rc = eu_hip_fail(e1 != hipSuccess ? e1 : e2, "the copy of the boxes and the tile table", __FILE__, __LINE__);
  }
  free(st);
  if (!rc) *ntiles = (unsigned int)nt;
  return rc;
}
