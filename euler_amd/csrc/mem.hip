// mem.hip — the device side of a handle's memory ledger (eu_mem.h, docs/handle_memory.md): the ledger's operations over hipMalloc / hipFree / hipMemset.  The only
// place outside the communicators and the function-local scratch of snapshot.hip and the measurement helpers where a handle's device memory is allocated or freed.
#include "euler_dev.h"

// ctx: where the HIP error of a failed call is left for eu_dev_alloc's message
static void* mem_hip_alloc(void* ctx, size_t bytes) {
  void* p = nullptr;
  const hipError_t e = hipMalloc(&p, bytes);
  if (e == hipSuccess) return p;
  *(hipError_t*)ctx = e;
  (void)hipGetLastError();
  return nullptr;
}
static void mem_hip_free(void*, void* p) { (void)hipFree(p); }
static int mem_hip_zero(void* ctx, void* p, size_t bytes) {
  const hipError_t e = hipMemset(p, 0, bytes);
  if (e != hipSuccess) *(hipError_t*)ctx = e;
  return e != hipSuccess;
}
static eu_mem_ops mem_hip_ops(hipError_t* why) { return eu_mem_ops{mem_hip_alloc, mem_hip_free, mem_hip_zero, why}; }

int eu_dev_alloc(euler_sim* S, void** p, size_t bytes, int group, int flags) {
  hipError_t why = hipSuccess;
  const eu_mem_ops ops = mem_hip_ops(&why);
  if (eu_mem_full(&S->mem)) { eu_set_error("the handle's memory ledger is full: %d blocks (eu_mem.h EU_MEM_CAP)", EU_MEM_CAP); return EULER_ENOMEM; }      // (never silent, whoever asks)
  const int rc = eu_mem_alloc(&S->mem, &ops, p, bytes, group, flags & (EU_MEM_ZERO | EU_MEM_UNCOUNTED));
  if (!rc || (flags & EU_DEV_QUIET)) return rc;
  if (why != hipSuccess) return eu_hip_fail(why, rc == EULER_EHIP ? "hipMemset of a new device block" : "hipMalloc", __FILE__, __LINE__);
  eu_set_error("a device block of %zu bytes in group %d was asked for", bytes, group);
  return rc;
}

int eu_dev_free(euler_sim* S, void* raw) {
  if (!raw) return EULER_OK;
  const eu_mem_ops ops = mem_hip_ops(nullptr);
  const int rc = eu_mem_free_one(&S->mem, &ops, raw);
  if (rc) eu_set_error("eu_dev_free: the handle's ledger does not hold this block");
  return rc;
}
void eu_dev_free_group(euler_sim* S, int group) {
  const eu_mem_ops ops = mem_hip_ops(nullptr);
  eu_mem_free_group(&S->mem, &ops, group);
}
void eu_dev_free_all(euler_sim* S) {
  const eu_mem_ops ops = mem_hip_ops(nullptr);
  eu_mem_free_all(&S->mem, &ops);
}
