// Device memory of the engine behind one owning type (host-only: no HIP header, compiles with a plain C++17 compiler).
#pragma once
#include <cstddef>
#include <utility>

// The two hooks every allocation goes through.  The library defines them once (shared.hip: the HIP runtime's calls); the host test
// (tests/test_devmem_host.py) defines counting fakes, so that the failure paths -- which cannot be provoked on a GPU -- run on the CPU.
int rift_dev_alloc(void** p, size_t bytes);      // 0 on success (the library: the hipError_t)
void rift_dev_free(void* p);

// One device allocation of T elements: move-only, grows and never shrinks, freed by the destructor.
// Buffers that are sized together (l_S / l_cnt, cr_buf / cr_part, *_img / *_par) are one DevBuf each, every one with its own capacity:
// when the second of a pair fails to grow, the first stays usable at its true capacity and the second is empty, so the next call
// allocates exactly what is missing -- no capacity ever describes a block it does not belong to.
template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); cap_ = std::exchange(o.cap_, 0); }
    return *this;
  }
  ~DevBuf() { reset(); }
  T* get() const { return p_; }
  size_t cap() const { return cap_; }      // elements
  void reset() { if (p_) rift_dev_free(p_); p_ = nullptr; cap_ = 0; }

  // Room for `need` elements.  Enough already: nothing happens.  Else the old block is freed FIRST (whoever must wait for its readers
  // waits before the call), the buffer is empty, and max(need, grow_to) elements are allocated; on failure it stays empty and the
  // hook's error is returned.  *fresh: the buffer holds a new block (its contents are undefined).
  int reserve(size_t need, size_t grow_to = 0, bool* fresh = nullptr) {
    if (fresh) *fresh = false;
    if (need <= cap_) return 0;
    reset();
    const size_t n = need > grow_to ? need : grow_to;
    void* p = nullptr;
    const int rc = rift_dev_alloc(&p, n * sizeof(T));
    if (rc != 0) return rc;
    p_ = static_cast<T*>(p); cap_ = n;
    if (fresh) *fresh = true;
    return 0;
  }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};
