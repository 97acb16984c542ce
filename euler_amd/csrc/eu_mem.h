/* eu_mem.h - the ledger of a handle's device memory: every persistent block the handle holds is recorded here when it is allocated, freed from here and
 * counted here (euler_hbm_bytes).  Plain C (C99 and C++), host only, no HIP: tests/c/sanitize_mem.c drives every operation below over malloc, with the k-th
 * allocation made to fail, under the address sanitizer and its leak check, without a GPU.  docs/handle_memory.md is the same page for somebody adding a buffer.
 *
 * The ledger is a fixed table inside the handle (euler_sim::mem; all zero = empty, which is what calloc leaves).  An entry holds the RAW pointer the allocator
 * returned, its bytes, its group and whether it counts.  The handle's own fields may hold the same block shifted (the row-major arrays by win_off, the skewed ones
 * by skew_off and their stagger): nobody needs to undo that arithmetic, because nothing but the ledger ever frees.
 *
 * Every operation takes an eu_mem_ops record {alloc, free, zero, ctx}: the device side passes hipMalloc / hipFree / hipMemset (mem.hip), the host test malloc /
 * free / memset.  alloc returns NULL when there is no room; zero returns non-zero when the fill failed.
 *
 * group          lifetime                                                          released by
 * ---------------------------------------------------------------------------------------------------------------------------------------
 * EU_MEM_HANDLE  from the call that needs the block until euler_destroy; single    euler_destroy (grow-only buffers and draws: eu_mem_free_one
 *                blocks may be replaced by a larger one (eu_devbuf_reserve)        of the old block once the new one is recorded)
 * EU_MEM_RING    the search directions' extra arrays (k_pcg.hip ring_begin)        ring_begin when one of them finds no room, euler_destroy
 * EU_MEM_COARSE  the dense coarse level (k_coarse.hip eu_coarse_alloc)             eu_coarse_release
 * EU_MEM_MG      the multilevel arrays and their exchange buffer (k_mg.hip)        eu_mg_release
 * EU_MEM_SPLIT   the split cycle's message buffers (k_mg_split.hip)                eu_mg_split_release, a plan the ranks do not agree on
 * EU_MEM_SLAB    the row slabs' exchange scratch (k_slab.hip)                      eu_slab_release
 *
 * Who may call what.  eu_mem_alloc: whoever gives the handle a block, through the device wrapper (euler_dev.h eu_dalloc) and nowhere else.  eu_mem_free_one: the
 * owner of a single block it replaces or drops, with the raw pointer.  eu_mem_free_group: the release function of that group, which then nulls its own fields.
 * eu_mem_free_all: euler_destroy, for a finished handle and a half-built one alike.  eu_mem_counted: euler_hbm_bytes.  Nobody calls ops->alloc or ops->free on a
 * handle's block directly.
 *
 * What a failed call leaves behind.  eu_mem_alloc that fails - a size of zero (EULER_EINVAL), a full table or no room (EULER_ENOMEM), a fill that failed
 * (EULER_EHIP) - records nothing, leaves nothing allocated and leaves *out as it was; a full table is found BEFORE the allocator is asked.  eu_mem_free_one of a
 * pointer that is not in the table (never recorded, freed already, NULL) returns EULER_EINVAL and does not reach ops->free.  The other operations cannot fail.
 * Growing a buffer is "allocate the new block, then free the old one": when the new block fails, the old one is still recorded and counted.
 *
 * What counts.  eu_mem_counted is the sum of the bytes of the entries without EU_MEM_UNCOUNTED, formed from the table whenever it is asked: there is no second
 * figure to keep in step. */
#ifndef EU_MEM_H
#define EU_MEM_H

#include <stddef.h>

#include "euler.h"

enum { EU_MEM_HANDLE = 0, EU_MEM_RING, EU_MEM_COARSE, EU_MEM_MG, EU_MEM_SPLIT, EU_MEM_SLAB, EU_MEM__GROUPS };
enum { EU_MEM_ZERO = 1, EU_MEM_UNCOUNTED = 2 };      /* eu_mem_alloc's flags */
#define EU_MEM_CAP 256      /* allocation sites of a handle with everything switched on: about 130 (docs/handle_memory.md) */

typedef struct eu_mem_ops {
  void* (*alloc)(void* ctx, size_t bytes);
  void (*free)(void* ctx, void* p);
  int (*zero)(void* ctx, void* p, size_t bytes);
  void* ctx;
} eu_mem_ops;

typedef struct eu_mem_entry { void* p; size_t bytes; unsigned char group, uncounted; } eu_mem_entry;
typedef struct eu_mem { int n; eu_mem_entry e[EU_MEM_CAP]; } eu_mem;      /* e[0 .. n) are live, in no particular order */

static inline int eu_mem_full(const eu_mem* m) { return m->n >= EU_MEM_CAP; }

static inline int eu_mem_alloc(eu_mem* m, const eu_mem_ops* ops, void** out, size_t bytes, int group, int flags) {
  if (!bytes || group < 0 || group >= EU_MEM__GROUPS) return EULER_EINVAL;
  if (eu_mem_full(m)) return EULER_ENOMEM;
  void* p = ops->alloc(ops->ctx, bytes);
  if (!p) return EULER_ENOMEM;
  if ((flags & EU_MEM_ZERO) && ops->zero(ops->ctx, p, bytes)) { ops->free(ops->ctx, p); return EULER_EHIP; }
  eu_mem_entry* e = &m->e[m->n++];
  e->p = p; e->bytes = bytes; e->group = (unsigned char)group; e->uncounted = (flags & EU_MEM_UNCOUNTED) ? 1 : 0;
  *out = p;
  return EULER_OK;
}

static inline int eu_mem_free_one(eu_mem* m, const eu_mem_ops* ops, void* p) {
  if (!p) return EULER_EINVAL;
  for (int k = 0; k < m->n; ++k)
    if (m->e[k].p == p) {
      m->e[k] = m->e[--m->n];      /* (the last entry fills the hole) */
      ops->free(ops->ctx, p);
      return EULER_OK;
    }
  return EULER_EINVAL;
}

static inline void eu_mem_free_group(eu_mem* m, const eu_mem_ops* ops, int group) {
  int kept = 0;
  for (int k = 0; k < m->n; ++k) {
    if (m->e[k].group == group) ops->free(ops->ctx, m->e[k].p);
    else m->e[kept++] = m->e[k];
  }
  m->n = kept;
}

static inline void eu_mem_free_all(eu_mem* m, const eu_mem_ops* ops) {
  for (int k = 0; k < m->n; ++k) ops->free(ops->ctx, m->e[k].p);
  m->n = 0;
}

static inline size_t eu_mem_counted(const eu_mem* m) {
  size_t b = 0;
  for (int k = 0; k < m->n; ++k) if (!m->e[k].uncounted) b += m->e[k].bytes;
  return b;
}

#endif
