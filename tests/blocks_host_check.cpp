// Host-only check of hyphy_amd/csrc/blocks.h (tests/test_blocks_cpu.py compiles and runs it): the owner of a shard's device and
// pinned blocks against a pool of its own.  The pool below is malloc-backed, keeps the set of live blocks, aborts on a free of a
// pointer it does not hold (unknown, or freed before), and can be told to fail the k-th allocation from now.  No GPU, no HIP call.
#include <stdio.h>
#include <stdlib.h>

#include <map>

#include "../hyphy_amd/csrc/blocks.h"

namespace {
struct Live { size_t bytes; bool pinned; };
std::map<void *, Live> g_live;
long g_calls = 0;       // pool calls of any kind
long g_fail_in = 0;     // > 0: the g_fail_in-th allocation from now fails
long g_sync_frees = 0;

hipError_t stub_alloc(void **p, size_t bytes, bool pinned) {
  g_calls++;
  if (g_fail_in > 0 && --g_fail_in == 0) {
    *p = nullptr;
    return hipErrorOutOfMemory;
  }
  *p = malloc(bytes ? bytes : 1);
  g_live[*p] = {bytes, pinned};
  return hipSuccess;
}
void stub_free(void *p, bool pinned) {
  g_calls++;
  if (!p) return;
  auto it = g_live.find(p);
  if (it == g_live.end() || it->second.pinned != pinned) {
    fprintf(stderr, "pool stub: free of a block that is not live (%p, %s)\n", p, pinned ? "pinned" : "device");
    abort();
  }
  g_live.erase(it);
  free(p);
}
size_t live_bytes(bool pinned) {
  size_t n = 0;
  for (const auto &kv : g_live)
    if (kv.second.pinned == pinned) n += kv.second.bytes;
  return n;
}

int g_failed = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      g_failed++;                                                     \
    }                                                                 \
  } while (0)
}  // namespace

namespace hyhip {
hipError_t pool_malloc(void **p, size_t bytes) { return stub_alloc(p, bytes, false); }
void pool_free(void *p) { stub_free(p, false); }
void pool_free_sync(void *p) { g_sync_frees++; stub_free(p, false); }
hipError_t pool_host_malloc(void **p, size_t bytes) { return stub_alloc(p, bytes, true); }
void pool_host_free(void *p) { stub_free(p, true); }
void pool_host_free_sync(void *p) { g_sync_frees++; stub_free(p, true); }
}  // namespace hyhip

using namespace hyhip;

namespace {

struct Fields {  // a shard in miniature: typed fields, a capacity, one owner
  double *a = nullptr, *b = nullptr;
  int *c = nullptr, *skipped = nullptr;
  char *h = nullptr;
  size_t cap = 0;
  BlockOwner own;
};
constexpr size_t kGroup = 4;  // blocks a group of `Fields` allocates (`skipped` asks for no bytes)
// the group at capacity n: 8 n + 8 n + 4 n device bytes, n pinned
size_t dev_bytes_at(size_t n) { return 20 * n; }
#define GROUP(f, n) {device_block((f).a, 8 * (n), "a"), device_block((f).b, 8 * (n), "b"), device_block((f).skipped, 0, "skipped"), \
                     device_block((f).c, 4 * (n), "c"), pinned_block((f).h, (n), "h")}
bool all_null(const Fields &f) { return !f.a && !f.b && !f.c && !f.h && !f.skipped; }
bool all_set(const Fields &f) { return f.a && f.b && f.c && f.h && !f.skipped; }

void check_group_get() {
  for (size_t k = 1; k <= kGroup; k++) {  // the k-th allocation of the group fails
    Fields f;
    double *other = nullptr;
    CHECK(f.own.get(device_block(other, 24)) == hipSuccess && other);
    const std::map<void *, Live> before = g_live;
    g_fail_in = (long)k;
    const BlockReq *failed = nullptr;
    const BlockReq g[] = GROUP(f, 10);
    CHECK(f.own.get_group(g, 5, &failed) == hipErrorOutOfMemory);
    static const char *const order[] = {"a", "b", "c", "h"};
    CHECK(failed && failed->name[0] == order[k - 1][0]);
    CHECK(all_null(f));
    CHECK(f.own.blocks() == 1 && f.own.device_bytes() == 24);
    CHECK(g_live.size() == before.size() && g_live.count(other) == 1);
    g_fail_in = 0;
  }
  Fields f;
  CHECK(f.own.get_group(GROUP(f, 10)) == hipSuccess);
  CHECK(all_set(f) && f.own.blocks() == kGroup && f.own.device_bytes() == dev_bytes_at(10));
  CHECK(live_bytes(false) == dev_bytes_at(10) && live_bytes(true) == 10);
  // a field that is set is not allocated over: the request is refused and the group stays as it was
  const size_t live = g_live.size();
  CHECK(f.own.get(device_block(f.a, 8)) != hipSuccess);
  CHECK(all_set(f) && g_live.size() == live && f.own.blocks() == kGroup);
  // a single get that fails
  double *one = nullptr;
  g_fail_in = 1;
  CHECK(f.own.get(device_block(one, 8)) == hipErrorOutOfMemory && !one && f.own.blocks() == kGroup);
  g_fail_in = 0;
}

void check_regrow() {
  for (size_t k = 1; k <= kGroup; k++) {
    Fields f;
    CHECK(f.own.regrow(GROUP(f, 4), f.cap, 3, 4, FreeMode::Sync) == hipSuccess);
    CHECK(all_set(f) && f.cap == 4 && f.own.device_bytes() == dev_bytes_at(4));
    g_fail_in = (long)k;
    CHECK(f.own.regrow(GROUP(f, 9), f.cap, 9, 9, FreeMode::Sync) == hipErrorOutOfMemory);
    g_fail_in = 0;
    CHECK(all_null(f) && f.cap == 0 && f.own.blocks() == 0 && f.own.device_bytes() == 0);
    CHECK(g_live.empty());
    // the next call allocates again, at the size it asks for — even one the lost capacity would have covered
    CHECK(f.own.regrow(GROUP(f, 2), f.cap, 2, 2, FreeMode::Sync) == hipSuccess);
    CHECK(all_set(f) && f.cap == 2 && f.own.device_bytes() == dev_bytes_at(2));
    CHECK(live_bytes(false) == dev_bytes_at(2) && live_bytes(true) == 2);
  }
  CHECK(g_live.empty());
  Fields f;
  CHECK(f.own.regrow(GROUP(f, 8), f.cap, 5, 8, FreeMode::NoSync) == hipSuccess && f.cap == 8);
  double *const a = f.a;
  const long calls = g_calls;
  for (size_t need = 0; need <= 8; need++) CHECK(f.own.regrow(GROUP(f, need), f.cap, need, need, FreeMode::Sync) == hipSuccess);
  CHECK(g_calls == calls && f.a == a && f.cap == 8);  // below capacity: the pool is not called
  const long syncs = g_sync_frees;
  CHECK(f.own.regrow(GROUP(f, 16), f.cap, 9, 16, FreeMode::Sync) == hipSuccess && f.cap == 16);
  CHECK(g_sync_frees == syncs + (long)kGroup);  // (the old blocks went back behind a synchronisation, as asked)
  CHECK(f.own.device_bytes() == dev_bytes_at(16) && live_bytes(false) == dev_bytes_at(16) && live_bytes(true) == 16);
}

void check_drop_and_release() {
  Fields f;
  const long calls = g_calls;
  f.own.drop(f.a, FreeMode::Sync);  // a null field: nothing
  f.own.drop(GROUP(f, 0), FreeMode::NoSync);
  CHECK(g_calls == calls && all_null(f));
  CHECK(f.own.get_group(GROUP(f, 6)) == hipSuccess);
  const long syncs = g_sync_frees;
  f.own.drop(f.b, FreeMode::NoSync);
  CHECK(!f.b && f.a && f.c && f.h && g_sync_frees == syncs);
  CHECK(f.own.blocks() == kGroup - 1 && f.own.device_bytes() == dev_bytes_at(6) - 48 && live_bytes(false) == dev_bytes_at(6) - 48);
  f.own.drop(f.h, FreeMode::Sync);
  CHECK(!f.h && g_sync_frees == syncs + 1 && live_bytes(true) == 0 && f.own.device_bytes() == dev_bytes_at(6) - 48);
  f.own.drop(f.b, FreeMode::Sync);  // again: nothing (the stub would abort on a second free)
  CHECK(f.own.get(device_block(f.b, 40)) == hipSuccess && f.own.device_bytes() == dev_bytes_at(6) - 8);
  f.own.release_all();  // each block exactly once: the stub aborts on a second free, and nothing stays live
  CHECK(g_live.empty() && f.own.blocks() == 0 && f.own.device_bytes() == 0);
  f.own.release_all();
  CHECK(g_live.empty());
}

void check_bytes_over_a_sequence() {
  Fields f;
  double *x = nullptr, *y = nullptr;
  size_t xcap = 0, want = 0;
  for (int step = 0; step < 40; step++) {  // get / drop / regrow in a fixed shuffle; the owner's figure follows the pool's live set
    switch (step % 5) {
      case 0: CHECK(f.own.regrow(GROUP(f, (size_t)step + 1), f.cap, (size_t)step + 1, (size_t)step + 1, FreeMode::Sync) == hipSuccess); break;
      case 1: if (!y) CHECK(f.own.get(device_block(y, 100 + (size_t)step)) == hipSuccess); break;
      case 2: CHECK(f.own.regrow({device_block(x, 8 * ((size_t)step + 3))}, xcap, (size_t)step, (size_t)step + 3, FreeMode::NoSync) == hipSuccess); break;
      case 3: f.own.drop(y, FreeMode::Sync); break;
      case 4: if (step % 2) { f.own.drop(GROUP(f, 0), FreeMode::Sync); f.cap = 0; } break;
    }
    want = live_bytes(false);
    CHECK(f.own.device_bytes() == want);
    CHECK(f.own.blocks() == g_live.size());
  }
  CHECK(want > 0);
  f.own.release_all();
  CHECK(f.own.device_bytes() == 0 && g_live.empty());
}

void check_move() {
  {
    BlockOwner dst;
    double *kept = nullptr;
    {
      Fields f;
      CHECK(f.own.get_group(GROUP(f, 3)) == hipSuccess);
      kept = f.a;
      Fields g = std::move(f);  // (what a vector of shards does when it grows)
      CHECK(f.own.blocks() == 0 && f.own.device_bytes() == 0 && g.own.blocks() == kGroup && g.a == kept);
      const long calls = g_calls;
      f.own.release_all();  // the source releases nothing ...
      CHECK(g_calls == calls && g_live.size() == kGroup);
      dst = std::move(g.own);
      CHECK(g.own.blocks() == 0 && dst.blocks() == kGroup);
    }                       // ... nor do the sources' destructors
    CHECK(g_live.size() == kGroup && g_live.count(kept) == 1 && dst.device_bytes() == dev_bytes_at(3));
    double *z = nullptr;
    BlockOwner other;
    CHECK(other.get(device_block(z, 8)) == hipSuccess);
    dst = std::move(other);  // move assignment releases what the target held
    CHECK(g_live.size() == 1 && g_live.count(z) == 1 && dst.blocks() == 1 && other.blocks() == 0);
  }  // an owner that goes away releases what it still holds
  CHECK(g_live.empty());
}

void check_call_scoped_blocks() {
  {
    Blocks blk;
    double *d = nullptr;
    int *i = nullptr;
    CHECK(blk.get(&d, 5) == hipSuccess && blk.get(&i, 0) == hipSuccess && d && i);
    CHECK(live_bytes(false) == 5 * sizeof(double) + sizeof(int));
    g_fail_in = 1;
    CHECK(blk.get(&d, 7) == hipErrorOutOfMemory && !d && blk.held.size() == 2);
    g_fail_in = 0;
  }
  CHECK(g_live.empty());
}

}  // namespace

int main() {
  check_group_get();
  CHECK(g_live.empty());
  check_regrow();
  CHECK(g_live.empty());
  check_drop_and_release();
  check_bytes_over_a_sequence();
  check_move();
  check_call_scoped_blocks();
  if (g_failed) {
    fprintf(stderr, "blocks_host_check: %d check(s) failed\n", g_failed);
    return 1;
  }
  printf("blocks_host_check: ok\n");
  return 0;
}
