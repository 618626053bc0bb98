// Who owns the library's device and pinned-host blocks.  Host only: nothing here needs device code or calls the HIP runtime (the
// pool does), so tests/blocks_host_check.cpp compiles it with the host compiler against a pool of its own.
//   Blocks      blocks of one call: back to the pool when the call returns, on every path
//   BlockOwner  blocks that live as long as a shard (Shard::own) or a partition: every allocation is recorded, one call releases them
#pragma once
#include <stddef.h>

#include <hip/hip_runtime_api.h>  // (hipError_t)

#include <algorithm>
#include <initializer_list>
#include <utility>
#include <vector>

namespace hyhip {

// Recycling allocator (pool.hip): analyses that create one likelihood function after another on the same tree (FEL: one per
// site) allocate the same ~45 device / pinned-host blocks and a stream over and over; hipMalloc / hipHostMalloc / hipFree /
// stream creation cost that life cycle more than its 50 evaluations.  Freed blocks go to a free list keyed by (device, size)
// and are handed out again on an exact size match.  pool_free / pool_host_free do NOT synchronise (hipFree does, implicitly):
// callers that free while work may be in flight use the _sync forms.  HYPHY_HIP_POOL_MB (default 1024; 0: off) caps the cached
// bytes per kind; blocks above 64 MiB are never cached.
hipError_t pool_malloc(void **p, size_t bytes);
void pool_free(void *p);
void pool_free_sync(void *p);
hipError_t pool_host_malloc(void **p, size_t bytes);
void pool_host_free(void *p);
void pool_host_free_sync(void *p);

// device blocks of one call: from the pool, back to it (behind a synchronisation) when the call returns, on every path
struct Blocks {
  std::vector<void *> held;
  Blocks() = default;
  Blocks(const Blocks &) = delete;
  Blocks &operator=(const Blocks &) = delete;
  ~Blocks() { release(); }
  void release() {
    for (void *b : held) pool_free_sync(b);
    held.clear();
  }
  template <typename T>
  hipError_t get(T **out, size_t n) {
    void *b = nullptr;
    const hipError_t e = pool_malloc(&b, std::max<size_t>(1, n) * sizeof(T));
    if (e == hipSuccess) held.push_back(b);
    *out = (T *)b;
    return e;
  }
};

// One block as a call site asks for it: the typed field that holds it, its size, where it lives, and the name an error message gives it.
struct BlockReq {
  void **field;
  size_t bytes;
  bool pinned;
  const char *name;
};
template <typename T>
inline BlockReq device_block(T *&field, size_t bytes, const char *name = "") { return {(void **)&field, bytes, false, name}; }
template <typename T>
inline BlockReq pinned_block(T *&field, size_t bytes, const char *name = "") { return {(void **)&field, bytes, true, name}; }

enum class FreeMode { NoSync, Sync };  // Sync: behind a device synchronisation (work that reads the block may be in flight)

// Every block a shard holds, as (pointer, requested bytes, device or pinned).  The fields stay where they are (Shard::codes, ...); they
// are set and nulled here alone, so a field is non-null exactly while its block is recorded.  Move-only: a copy could free twice.
class BlockOwner {
 public:
  BlockOwner() = default;
  BlockOwner(BlockOwner &&o) noexcept : held_(std::move(o.held_)) { o.held_.clear(); }
  BlockOwner &operator=(BlockOwner &&o) noexcept {
    if (this != &o) {
      release_all();
      held_ = std::move(o.held_);
      o.held_.clear();
    }
    return *this;
  }
  BlockOwner(const BlockOwner &) = delete;
  BlockOwner &operator=(const BlockOwner &) = delete;
  ~BlockOwner() { release_all(); }

  // Allocate into a field that is null.  On failure the field stays null and nothing is recorded.
  hipError_t get(const BlockReq &r) { return get_group(&r, 1); }
  // All or nothing: every listed field ends up set (a request of 0 bytes is skipped: its field stays null), or all are null, nothing is
  // recorded and `*failed` is the request that could not be served.
  hipError_t get_group(const BlockReq *g, size_t n, const BlockReq **failed = nullptr) {
    hipError_t e = hipSuccess;
    size_t k = 0;
    if (held_.empty()) held_.reserve(64);  // (a shard holds about fifty from creation on)
    for (; k < n && e == hipSuccess; k++) {
      if (g[k].bytes == 0) continue;
      void *b = nullptr;
      e = *g[k].field ? hipErrorInvalidValue : (g[k].pinned ? pool_host_malloc(&b, g[k].bytes) : pool_malloc(&b, g[k].bytes));
      if (e != hipSuccess) break;
      *g[k].field = b;
      held_.push_back({b, g[k].bytes, g[k].pinned});
    }
    if (e == hipSuccess) return e;
    if (failed) *failed = &g[k];
    drop(g, k, FreeMode::NoSync);  // (nothing has used them yet)
    return e;
  }
  hipError_t get_group(std::initializer_list<BlockReq> g, const BlockReq **failed = nullptr) { return get_group(g.begin(), g.size(), failed); }

  // Free the block of a field, remove its record and null the field.  A null field: nothing happens.
  void drop(const BlockReq *g, size_t n, FreeMode mode) {
    for (size_t k = 0; k < n; k++) {
      void *b = *g[k].field;
      if (!b) continue;
      *g[k].field = nullptr;
      for (size_t i = held_.size(); i-- > 0;)
        if (held_[i].ptr == b) {
          free_block(held_[i], mode);
          held_.erase(held_.begin() + (ptrdiff_t)i);
          break;
        }
    }
  }
  void drop(std::initializer_list<BlockReq> g, FreeMode mode) { drop(g.begin(), g.size(), mode); }
  template <typename T>
  void drop(T *&field, FreeMode mode) { drop({BlockReq{(void **)&field, 0, false, ""}}, mode); }

  // Grow-only buffers: nothing if `cap` covers `need`.  Otherwise drop the group, get it again at the sizes the caller worked out for
  // `new_cap`, and set `cap` last — after a failure every field is null and `cap` is 0, so the next call allocates again.
  hipError_t regrow(std::initializer_list<BlockReq> g, size_t &cap, size_t need, size_t new_cap, FreeMode mode) {
    if (cap >= need) return hipSuccess;
    drop(g, mode);
    cap = 0;
    const hipError_t e = get_group(g);
    if (e == hipSuccess) cap = new_cap;
    return e;
  }

  // Everything back to the pool, without a synchronisation (the caller has waited for the work that used the blocks), last block
  // first: the pool's free lists are stacks, so the next partition of the same shape finds each of its fields the block the field had
  // here.  The fields are not known here: the caller resets the object that holds them.
  void release_all() {
    for (size_t i = held_.size(); i-- > 0;) free_block(held_[i], FreeMode::NoSync);
    held_.clear();
  }

  size_t device_bytes() const {  // requested bytes of the device blocks held
    size_t n = 0;
    for (const Rec &r : held_)
      if (!r.pinned) n += r.bytes;
    return n;
  }
  size_t blocks() const { return held_.size(); }

 private:
  struct Rec {
    void *ptr;
    size_t bytes;
    bool pinned;
  };
  static void free_block(const Rec &r, FreeMode mode) {
    if (r.pinned) mode == FreeMode::Sync ? pool_host_free_sync(r.ptr) : pool_host_free(r.ptr);
    else mode == FreeMode::Sync ? pool_free_sync(r.ptr) : pool_free(r.ptr);
  }
  std::vector<Rec> held_;
};

}  // namespace hyhip
