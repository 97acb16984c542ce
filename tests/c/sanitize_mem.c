/* sanitize_mem.c - the ledger of a handle's device memory (euler_amd/csrc/eu_mem.h) over malloc-backed ops that fail the k-th allocation on request.  Stand-alone:
 * built with -fsanitize=address,undefined and run with detect_leaks=1 by tests/test_mem_host.py.  The ops count every block they hand out and take back, refuse to
 * free what they did not hand out (or hand out twice), and the leak check sees whatever is left. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "eu_mem.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

/* ---- the allocator under the ledger ---------------------------------------------------------------------------------------------------------- */
#define LIVE_MAX 1024
typedef struct host_ctx {
  int calls, fail_at;      /* allocations asked for so far; the one (0-based) that fails, -1: none */
  int zero_fail;           /* the next fill fails */
  int nlive, bad_free;     /* blocks out; frees of a block that is not out */
  void* live[LIVE_MAX];
} host_ctx;

static void* h_alloc(void* c, size_t bytes) {
  host_ctx* h = (host_ctx*)c;
  if (h->calls++ == h->fail_at) return NULL;
  CHECK(h->nlive < LIVE_MAX);
  unsigned char* p = (unsigned char*)malloc(bytes);
  CHECK(p);
  memset(p, 0xa5, bytes);      /* (a block is NOT zero unless the ledger's caller asked for it) */
  h->live[h->nlive++] = p;
  return p;
}
static void h_free(void* c, void* p) {
  host_ctx* h = (host_ctx*)c;
  for (int k = 0; k < h->nlive; ++k)
    if (h->live[k] == p) { h->live[k] = h->live[--h->nlive]; free(p); return; }
  h->bad_free++;      /* never handed out, or freed already: NOT passed on to free */
}
static int h_zero(void* c, void* p, size_t bytes) {
  host_ctx* h = (host_ctx*)c;
  if (h->zero_fail) { h->zero_fail = 0; return 1; }
  memset(p, 0, bytes);
  return 0;
}
static eu_mem_ops ops_of(host_ctx* h) { eu_mem_ops o = {h_alloc, h_free, h_zero, h}; return o; }
static void ctx_init(host_ctx* h, int fail_at) { memset(h, 0, sizeof *h); h->fail_at = fail_at; }

/* the counted bytes by the definition: the sum over what was recorded, counted and not yet freed */
static size_t counted_by_hand(const eu_mem* m) {
  size_t b = 0;
  for (int k = 0; k < m->n; ++k) if (!m->e[k].uncounted) b += m->e[k].bytes;
  return b;
}
static int group_entries(const eu_mem* m, int g) { int n = 0; for (int k = 0; k < m->n; ++k) n += m->e[k].group == g; return n; }
static int all_zero(const void* p, size_t n) { for (size_t k = 0; k < n; ++k) if (((const unsigned char*)p)[k]) return 0; return 1; }

/* ---- a creation-like sequence: N allocations across all groups, some zeroed, some uncounted -------------------------------------------------- */
#define SEQ_N 40
static size_t seq_bytes(int k) { return (size_t)(1 + (k * 37) % 200) * (k % 5 == 0 ? 64 : 1); }
static int seq_group(int k) { return k % EU_MEM__GROUPS; }
static int seq_flags(int k) { return (k % 3 == 0 ? EU_MEM_ZERO : 0) | (k % 7 == 3 ? EU_MEM_UNCOUNTED : 0); }

static void creation_failing_at(int fail_at) {
  host_ctx h;
  ctx_init(&h, fail_at);
  eu_mem_ops ops = ops_of(&h);
  eu_mem m;
  memset(&m, 0, sizeof m);      /* (what calloc leaves in the handle) */
  void* ptr[SEQ_N];
  size_t want = 0;
  int made = 0;
  for (int k = 0; k < SEQ_N; ++k) {
    void* const canary = (void*)&h;
    ptr[k] = canary;
    const int rc = eu_mem_alloc(&m, &ops, &ptr[k], seq_bytes(k), seq_group(k), seq_flags(k));
    if (k == fail_at) {      /* as euler_create does: the first failure ends the sequence */
      CHECK(rc == EULER_ENOMEM && ptr[k] == canary && m.n == made && h.nlive == made);
      CHECK(eu_mem_counted(&m) == want);
      break;
    }
    CHECK(rc == EULER_OK && ptr[k] != canary && ptr[k] != NULL);
    ++made;
    if (!(seq_flags(k) & EU_MEM_UNCOUNTED)) want += seq_bytes(k);
    if (seq_flags(k) & EU_MEM_ZERO) CHECK(all_zero(ptr[k], seq_bytes(k)));
    else CHECK(*(unsigned char*)ptr[k] == 0xa5);
    CHECK(m.n == made && h.nlive == made);
    CHECK(eu_mem_counted(&m) == want && counted_by_hand(&m) == want);
  }
  CHECK(made == (fail_at < 0 ? SEQ_N : fail_at));
  eu_mem_free_all(&m, &ops);
  CHECK(m.n == 0 && h.nlive == 0 && h.bad_free == 0 && eu_mem_counted(&m) == 0);
  eu_mem_free_all(&m, &ops);      /* (a second euler_destroy-like pass finds nothing) */
  CHECK(h.bad_free == 0);
}

/* ---- free-one -------------------------------------------------------------------------------------------------------------------------------- */
static void free_one(void) {
  host_ctx h;
  ctx_init(&h, -1);
  eu_mem_ops ops = ops_of(&h);
  eu_mem m;
  memset(&m, 0, sizeof m);
  void *a = NULL, *b = NULL, *c = NULL;
  CHECK(!eu_mem_alloc(&m, &ops, &a, 100, EU_MEM_HANDLE, 0) && !eu_mem_alloc(&m, &ops, &b, 200, EU_MEM_MG, EU_MEM_UNCOUNTED) && !eu_mem_alloc(&m, &ops, &c, 300, EU_MEM_HANDLE, 0));
  int stranger;
  CHECK(eu_mem_free_one(&m, &ops, &stranger) == EULER_EINVAL);          /* never recorded */
  CHECK(eu_mem_free_one(&m, &ops, NULL) == EULER_EINVAL);
  CHECK(eu_mem_free_one(&m, &ops, (char*)a + 8) == EULER_EINVAL);       /* a shifted pointer is not the block */
  CHECK(m.n == 3 && h.nlive == 3 && h.bad_free == 0 && eu_mem_counted(&m) == 400);
  CHECK(eu_mem_free_one(&m, &ops, a) == EULER_OK);
  CHECK(m.n == 2 && h.nlive == 2 && eu_mem_counted(&m) == 300);
  CHECK(eu_mem_free_one(&m, &ops, a) == EULER_EINVAL);                  /* freed already: reported, and free never sees it */
  CHECK(m.n == 2 && h.nlive == 2 && h.bad_free == 0);
  CHECK(eu_mem_free_one(&m, &ops, b) == EULER_OK && eu_mem_counted(&m) == 300);      /* (it did not count) */
  CHECK(eu_mem_free_one(&m, &ops, c) == EULER_OK && eu_mem_counted(&m) == 0 && m.n == 0 && h.nlive == 0 && h.bad_free == 0);
  /* refused before the allocator is asked: no bytes, no such group */
  const int calls = h.calls;
  CHECK(eu_mem_alloc(&m, &ops, &a, 0, EU_MEM_HANDLE, 0) == EULER_EINVAL && eu_mem_alloc(&m, &ops, &a, 8, EU_MEM__GROUPS, 0) == EULER_EINVAL && eu_mem_alloc(&m, &ops, &a, 8, -1, 0) == EULER_EINVAL);
  CHECK(h.calls == calls && m.n == 0);
  /* a fill that fails: the block goes back, nothing is recorded */
  h.zero_fail = 1;
  void* z = &stranger;
  CHECK(eu_mem_alloc(&m, &ops, &z, 64, EU_MEM_SLAB, EU_MEM_ZERO) == EULER_EHIP && z == (void*)&stranger && m.n == 0 && h.nlive == 0 && h.bad_free == 0);
}

/* ---- free-a-group ---------------------------------------------------------------------------------------------------------------------------- */
static void free_group(void) {
  host_ctx h;
  ctx_init(&h, -1);
  eu_mem_ops ops = ops_of(&h);
  eu_mem m;
  memset(&m, 0, sizeof m);
  void* ptr[SEQ_N];
  size_t counted[EU_MEM__GROUPS] = {0}, total = 0;
  int entries[EU_MEM__GROUPS] = {0};
  for (int k = 0; k < SEQ_N; ++k) {
    CHECK(!eu_mem_alloc(&m, &ops, &ptr[k], seq_bytes(k), seq_group(k), seq_flags(k)));
    entries[seq_group(k)]++;
    if (!(seq_flags(k) & EU_MEM_UNCOUNTED)) { counted[seq_group(k)] += seq_bytes(k); total += seq_bytes(k); }
  }
  for (int g = EU_MEM__GROUPS - 1; g >= 1; --g) {      /* every group but the handle's, one after the other */
    const int before = m.n;
    eu_mem_free_group(&m, &ops, g);
    total -= counted[g];
    CHECK(m.n == before - entries[g] && h.nlive == m.n && group_entries(&m, g) == 0 && h.bad_free == 0);
    CHECK(eu_mem_counted(&m) == total);
    for (int o = 0; o < g; ++o) CHECK(group_entries(&m, o) == entries[o]);
    for (int k = 0; k < SEQ_N; ++k)      /* the others' blocks are still theirs to write */
      if (seq_group(k) < g) memset(ptr[k], 0x11, seq_bytes(k));
    eu_mem_free_group(&m, &ops, g);      /* released already: nothing to do */
    CHECK(m.n == before - entries[g] && h.bad_free == 0);
  }
  /* a released group takes blocks again, and one of the kept entries can still be freed alone */
  void *again = NULL, *again2 = NULL;
  CHECK(!eu_mem_alloc(&m, &ops, &again, 4096, EU_MEM_MG, EU_MEM_ZERO) && !eu_mem_alloc(&m, &ops, &again2, 100, EU_MEM_MG, EU_MEM_UNCOUNTED));
  CHECK(all_zero(again, 4096) && group_entries(&m, EU_MEM_MG) == 2 && eu_mem_counted(&m) == total + 4096);
  CHECK(eu_mem_free_one(&m, &ops, ptr[0]) == EULER_OK);      /* (k = 0: the handle's group, counted) */
  CHECK(eu_mem_counted(&m) == total + 4096 - seq_bytes(0));
  eu_mem_free_group(&m, &ops, EU_MEM_MG);
  CHECK(eu_mem_counted(&m) == total - seq_bytes(0) && group_entries(&m, EU_MEM_HANDLE) == entries[EU_MEM_HANDLE] - 1);
  eu_mem_free_all(&m, &ops);
  CHECK(m.n == 0 && h.nlive == 0 && h.bad_free == 0);
}

/* ---- grow-and-replace, as eu_devbuf_reserve does: the new block first, the old one behind it ----------------------------------------------------- */
typedef struct buf { void* p; size_t bytes; } buf;
static int reserve(eu_mem* m, const eu_mem_ops* ops, buf* b, size_t bytes, size_t keep) {
  if (bytes <= b->bytes) return EULER_OK;
  void* nb = NULL;
  if (eu_mem_alloc(m, ops, &nb, bytes, EU_MEM_HANDLE, 0)) return EULER_ENOMEM;
  if (keep) memcpy(nb, b->p, keep);
  if (b->p) CHECK(eu_mem_free_one(m, ops, b->p) == EULER_OK);
  b->p = nb; b->bytes = bytes;
  return EULER_OK;
}
static void grow_and_replace(void) {
  host_ctx h;
  ctx_init(&h, -1);
  eu_mem_ops ops = ops_of(&h);
  eu_mem m;
  memset(&m, 0, sizeof m);
  buf b = {NULL, 0};
  void* other = NULL;
  CHECK(!eu_mem_alloc(&m, &ops, &other, 50, EU_MEM_HANDLE, 0));
  CHECK(!reserve(&m, &ops, &b, 64, 0) && eu_mem_counted(&m) == 50 + 64 && m.n == 2);
  memset(b.p, 0x5c, 64);
  CHECK(!reserve(&m, &ops, &b, 32, 0) && b.bytes == 64 && m.n == 2);      /* grow-only */
  CHECK(!reserve(&m, &ops, &b, 128, 64) && eu_mem_counted(&m) == 50 + 128 && m.n == 2 && h.nlive == 2);
  for (int k = 0; k < 64; ++k) CHECK(((unsigned char*)b.p)[k] == 0x5c);      /* the records keep their bits */
  void* const old = b.p;
  h.fail_at = h.calls;      /* the next allocation fails */
  CHECK(reserve(&m, &ops, &b, 256, 128) == EULER_ENOMEM);
  CHECK(b.p == old && b.bytes == 128 && eu_mem_counted(&m) == 50 + 128 && m.n == 2 && h.nlive == 2);      /* the old block: still recorded, counted and readable */
  for (int k = 0; k < 64; ++k) CHECK(((unsigned char*)b.p)[k] == 0x5c);
  CHECK(!reserve(&m, &ops, &b, 256, 128) && eu_mem_counted(&m) == 50 + 256);      /* ... and the next attempt succeeds */
  eu_mem_free_all(&m, &ops);
  CHECK(h.nlive == 0 && h.bad_free == 0);
}

/* ---- the full table -------------------------------------------------------------------------------------------------------------------------- */
static void full_table(void) {
  host_ctx h;
  ctx_init(&h, -1);
  eu_mem_ops ops = ops_of(&h);
  eu_mem* m = (eu_mem*)calloc(1, sizeof(eu_mem));
  CHECK(m);
  void* p = NULL;
  for (int k = 0; k < EU_MEM_CAP; ++k) { CHECK(!eu_mem_full(m)); CHECK(!eu_mem_alloc(m, &ops, &p, 16, k % EU_MEM__GROUPS, 0)); }
  CHECK(eu_mem_full(m) && m->n == EU_MEM_CAP && eu_mem_counted(m) == (size_t)16 * EU_MEM_CAP);
  void* const last = p;
  const int calls = h.calls;
  void* q = &h;
  CHECK(eu_mem_alloc(m, &ops, &q, 16, EU_MEM_HANDLE, EU_MEM_ZERO) == EULER_ENOMEM);      /* refused before the allocator is asked: nothing to leak */
  CHECK(q == (void*)&h && h.calls == calls && h.nlive == EU_MEM_CAP && m->n == EU_MEM_CAP);
  CHECK(eu_mem_free_one(m, &ops, last) == EULER_OK && !eu_mem_full(m));
  CHECK(!eu_mem_alloc(m, &ops, &q, 16, EU_MEM_HANDLE, EU_MEM_ZERO) && all_zero(q, 16) && eu_mem_full(m));      /* room again */
  eu_mem_free_all(m, &ops);
  CHECK(m->n == 0 && h.nlive == 0 && h.bad_free == 0);
  free(m);
}

int main(void) {
  for (int k = -1; k < SEQ_N; ++k) creation_failing_at(k);      /* never, and at every k */
  free_one();
  free_group();
  grow_and_replace();
  full_table();
  printf("handle memory ledger: clean\n");
  return 0;
}
