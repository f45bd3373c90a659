// device_buffers.hpp -- who owns an engine's device memory.
//
//   DevPool      one per engine: every live block with its size, the byte ledger (gmb_resident_bytes) and release_all(),
//                the ONE place the blocks are freed when the engine goes
//   DevBuf<T>    pointer + element capacity of one block of a pool; converts to T*, so use sites read as with a bare pointer
//   ScopedBuf<T> a DevBuf that gives its block back at scope exit unless a DevBuf adopted it
//   RowGroup     the shared row count of several buffers that are only ever sized together
//   Budget       what a list of buffers and row groups takes, and what of it is still to be allocated: a call measures with it
//   Reserver     ... and then allocates, walking the same list
//
// No engine types, and no HIP beyond the two allocator hooks below: a program that defines GMB_DEVBUF_OWN_HOOKS supplies its own
// pair, which is how tools/device_buffers_check.cpp runs this very header on host memory under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <unordered_map>

#ifndef GMB_DEVBUF_OWN_HOOKS
#include <hip/hip_runtime.h>
#endif

namespace gmb {

// The allocator: devbuf_alloc returns nullptr, or why the block could not be had.  These are an engine's only hipMalloc / hipFree.
#ifdef GMB_DEVBUF_OWN_HOOKS
const char* devbuf_alloc(void** p, size_t bytes);
void devbuf_free(void* p);
#else
inline const char* devbuf_alloc(void** p, size_t bytes) {
  const hipError_t s = hipMalloc(p, bytes);
  return s == hipSuccess ? nullptr : hipGetErrorString(s);
}
inline void devbuf_free(void* p) { (void)hipFree(p); }
#endif

struct DevPool {
  // a refused allocation is reported to the owner (the engine: its error text), and what that returns is the status reserve /
  // renew hand on to their caller
  void* owner = nullptr;
  int (*refused)(void* owner, size_t bytes, const char* why) = nullptr;
  struct Block {
    size_t bytes;
    bool counted;
  };
  std::unordered_map<void*, Block> live;
  // the ledger: bytes of the live COUNTED blocks.  An uncounted block (the engine's scalar and status blocks, its launch plans:
  // fixed overhead the ledger never held) is freed with the rest and appears in neither number.
  int64_t bytes_resident = 0, bytes_peak = 0;

  int acquire(void** p, size_t bytes, bool counted) {
    *p = nullptr;
    if (const char* why = devbuf_alloc(p, bytes)) {
      *p = nullptr;
      return refused ? refused(owner, bytes, why) : -1;
    }
    live[*p] = Block{bytes, counted};
    if (counted) {
      bytes_resident += (int64_t)bytes;
      if (bytes_peak < bytes_resident) bytes_peak = bytes_resident;
    }
    return 0;
  }
  void release(void* p) {
    if (!p) return;
    auto it = live.find(p);
    if (it == live.end()) return;  // not ours: not ours to free
    if (it->second.counted) bytes_resident -= (int64_t)it->second.bytes;
    live.erase(it);
    devbuf_free(p);
  }
  void release_all() {
    for (auto& b : live) devbuf_free(b.first);
    live.clear();
    bytes_resident = 0;
  }
};

template <typename T>
struct DevBuf {
  T* p = nullptr;
  int64_t cap = 0;  // elements the block holds -- 0 while `stale`: the block is still there, the next reserve replaces it

  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;  // (`auto x = e->dA` would be a second owner)
  DevBuf& operator=(const DevBuf&) = delete;
  operator T*() const { return p; }

  // at least `need` elements: nothing when they are there (inline, two compares: gmb_set_theta comes through here on every
  // evaluation), else renew
  int reserve(DevPool& pool, int64_t need, bool counted = true) {
    if (cap >= need && p) return 0;
    return renew(pool, need, counted);
  }
  // a fresh block of exactly `need` elements (at least one): the old one is freed FIRST, so the two never coexist.  On failure
  // the buffer is empty.
  int renew(DevPool& pool, int64_t need, bool counted = true) {
    drop(pool);
    if (need < 1) need = 1;
    const int rc = pool.acquire(reinterpret_cast<void**>(&p), (size_t)need * sizeof(T), counted);
    if (!rc) cap = need;
    return rc;
  }
  // what the block holds is sized for something that is gone.  The block stays (and stays in the ledger) until the next
  // reserve frees it in exchange for one of the right size.
  void stale() { cap = 0; }
  void drop(DevPool& pool) {
    pool.release(p);
    p = nullptr;
    cap = 0;
  }
  // this buffer's block goes, `other`'s becomes this buffer's
  void adopt(DevPool& pool, DevBuf& other) {
    drop(pool);
    p = other.p;
    cap = other.cap;
    other.p = nullptr;
    other.cap = 0;
  }
};

// a temporary: whatever it still holds at scope exit -- an early return -- goes back to the pool
template <typename T>
struct ScopedBuf : DevBuf<T> {
  DevPool& pool;
  explicit ScopedBuf(DevPool& pl) : pool(pl) {}
  ~ScopedBuf() { this->drop(pool); }
};

// Buffers that are sized together by one row count (a prediction's workspaces, the prepared points, ...).  The count is claimed
// only after EVERY member has its block: a failure half-way leaves rows == 0, and the retry renews all of them.
struct RowGroup {
  int64_t rows = 0;
  void stale() { rows = 0; }
  template <typename RenewAll>  // int(): renew every member for `need` rows, stopping at the first failure
  int reserve_rows(int64_t need, RenewAll renew_all) {
    if (rows >= need) return 0;
    rows = 0;
    const int rc = renew_all();
    if (!rc) rows = need;
    return rc;
  }
};

// A call writes the list of its buffers once, as a function of a visitor, and walks it twice: with a Budget, to measure the request
// against the device BEFORE anything is touched, then with a Reserver.  Both answer "go on?".  In double: the element
// counts of a request that has to be refused can overflow int64_t.  A row group says what it takes through bytes(rows, args...)
// and held(args...) (workspaces.hpp).
struct Budget {
  double total = 0.0;  // bytes the listed buffers take at the sizes asked for
  double fresh = 0.0;  // bytes still to be allocated; a stale buffer or group holds nothing, so it counts in full
  template <typename T>
  bool buf(const DevBuf<T>& b, double need) {
    total += sizeof(T) * need;
    if ((double)b.cap < need) fresh += sizeof(T) * (need - (double)b.cap);
    return true;
  }
  template <typename Group, typename... Args>
  bool rows(Group& g, double need, Args... args) {
    const double have = (double)g.held(args...);
    total += g.bytes(need, args...);
    if (have < need) fresh += g.bytes(need, args...) - g.bytes(have, args...);
    return true;
  }
};
struct Reserver {
  DevPool& pool;
  int rc = 0;  // the first failure: the walk stops there
  template <typename T>
  bool buf(DevBuf<T>& b, double need) { return !(rc = b.reserve(pool, (int64_t)need)); }
  template <typename Group, typename... Args>
  bool rows(Group& g, double need, Args... args) { return !(rc = g.reserve(pool, (int64_t)need, args...)); }
};

}  // namespace gmb
