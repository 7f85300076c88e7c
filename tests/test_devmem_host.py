"""csrc/devmem.h on the CPU: the owning buffer type of the engine's device memory against counting fakes of its two allocation hooks.

The failure paths of a device allocation cannot be provoked on a GPU; the header is host-only, so they run here: a stand-alone program
(its own main, built by g++ with the address and undefined-behaviour sanitizers, run directly) defines the hooks as malloc / free with a
set of live addresses and a "fail the n-th allocation from now" knob.  The fake's free aborts on an address that is not live."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <unordered_map>
#include "devmem.h"

static std::set<void*> live;
static long allocs = 0, frees = 0, fail_in = 0;      // fail_in = n: the n-th allocation from now fails

int rift_dev_alloc(void** p, size_t bytes) {
  if (fail_in > 0 && --fail_in == 0) return 2;
  void* q = malloc(bytes ? bytes : 1);
  live.insert(q); ++allocs; *p = q;
  return 0;
}
void rift_dev_free(void* p) {
  if (!live.erase(p)) { fprintf(stderr, "free of an address that is not live\n"); abort(); }
  free(p); ++frees;
}

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #x, __PRETTY_FUNCTION__); exit(1); } } while (0)

template <class T> struct Image { DevBuf<T> bf, f32; int N = 0; };      // as PW: owning images held by value in a map

// the engine's way with two buffers sized together: one reserve each, the first error returned
template <class T> int grow_pair(DevBuf<T>& a, DevBuf<T>& b, size_t n) {
  if (int rc = a.reserve(n)) return rc;
  return b.reserve(n);
}

template <class T> void run() {
  const size_t base = live.size();
  {
    DevBuf<T> b;
    CHECK(b.get() == nullptr && b.cap() == 0);
    bool fresh = true;
    CHECK(b.reserve(0, 0, &fresh) == 0 && !fresh && allocs == frees && b.get() == nullptr);      // nothing needed: nothing allocated
    CHECK(b.reserve(10, 0, &fresh) == 0 && fresh && b.cap() == 10 && live.count(b.get()) == 1);
    for (size_t i = 0; i < 10; ++i) b.get()[i] = T(1);                                           // (the sanitizer checks the size)
    // below the capacity: no allocation, the same pointer, not fresh
    T* p = b.get(); long a0 = allocs, f0 = frees;
    fresh = true;
    CHECK(b.reserve(5, 0, &fresh) == 0 && !fresh && b.reserve(10, 64, &fresh) == 0 && !fresh);
    CHECK(allocs == a0 && frees == f0 && b.get() == p && b.cap() == 10);
    // growth: exactly the old block freed, grow_to honoured, fresh
    CHECK(b.reserve(20, 64, &fresh) == 0 && fresh);
    CHECK(allocs == a0 + 1 && frees == f0 + 1 && live.count(p) == 0 && live.count(b.get()) == 1 && b.cap() == 64 && live.size() == base + 1);
    for (size_t i = 0; i < 64; ++i) b.get()[i] = T(2);
    CHECK(b.reserve(100, 64, &fresh) == 0 && fresh && b.cap() == 100);                            // need beyond grow_to: need
    // a failed growth: empty, and the old, smaller size allocates again
    p = b.get(); a0 = allocs; f0 = frees;
    fail_in = 1;
    CHECK(b.reserve(1000, 0, &fresh) != 0 && !fresh);
    CHECK(b.get() == nullptr && b.cap() == 0 && live.count(p) == 0 && frees == f0 + 1 && allocs == a0 && live.size() == base);
    CHECK(b.reserve(100, 0, &fresh) == 0 && fresh && b.cap() == 100 && allocs == a0 + 1 && live.size() == base + 1);
    b.reset();
    CHECK(b.get() == nullptr && b.cap() == 0 && live.size() == base);
    b.reset();                                                                                    // (twice: nothing to free)
    CHECK(b.reserve(3) == 0);
  }                                                                                               // destructor of a full buffer
  CHECK(live.size() == base);
  {
    DevBuf<T> e;                                                                                  // destructor of a buffer left empty by a failure
    fail_in = 1;
    CHECK(e.reserve(4) != 0 && e.get() == nullptr && e.cap() == 0);
  }
  CHECK(live.size() == base && fail_in == 0);
  {  // moves transfer ownership; assignment frees the target's old block
    DevBuf<T> a;
    CHECK(a.reserve(8) == 0);
    T* p = a.get();
    DevBuf<T> b(std::move(a));
    CHECK(a.get() == nullptr && a.cap() == 0 && b.get() == p && b.cap() == 8 && live.size() == base + 1);
    DevBuf<T> c;
    CHECK(c.reserve(4) == 0);
    T* pc = c.get(); const long f0 = frees;
    c = std::move(b);
    CHECK(frees == f0 + 1 && live.count(pc) == 0 && c.get() == p && c.cap() == 8 && b.get() == nullptr && b.cap() == 0 && live.size() == base + 1);
    c = std::move(b);                                                                             // (from an empty one: the target is emptied)
    CHECK(c.get() == nullptr && c.cap() == 0 && live.size() == base);
  }
  CHECK(live.size() == base);
  {  // the paired rule: each buffer its own capacity, so a capacity never describes a block it does not belong to
    DevBuf<T> a, b;
    CHECK(grow_pair(a, b, 8) == 0 && a.cap() == 8 && b.cap() == 8);
    fail_in = 2;                                                                                  // the SECOND allocation of the growth fails
    CHECK(grow_pair(a, b, 16) != 0);
    CHECK(a.cap() == 16 && live.count(a.get()) == 1 && b.cap() == 0 && b.get() == nullptr && live.size() == base + 1);
    T* pa = a.get(); long a0 = allocs;
    CHECK(grow_pair(a, b, 8) == 0);                                                               // the next, smaller call: only what is missing
    CHECK(a.get() == pa && a.cap() == 16 && b.cap() == 8 && live.count(b.get()) == 1 && allocs == a0 + 1);
    for (size_t i = 0; i < 8; ++i) { a.get()[i] = T(3); b.get()[i] = T(4); }
    fail_in = 1;                                                                                  // the FIRST fails: the second is not touched
    T* pb = b.get();
    CHECK(grow_pair(a, b, 32) != 0 && a.get() == nullptr && a.cap() == 0 && b.get() == pb && b.cap() == 8 && live.size() == base + 1);
    CHECK(grow_pair(a, b, 32) == 0 && a.cap() == 32 && b.cap() == 32 && live.size() == base + 2);
  }
  CHECK(live.size() == base);
  {  // a map of owning images, as RiftCtx::pw: erase and clear() release everything
    std::unordered_map<std::string, Image<T>> pw;
    for (int i = 0; i < 7; ++i) {
      Image<T> w; w.N = i;
      CHECK(w.bf.reserve(16 + i) == 0 && w.f32.reserve(32) == 0);
      pw["layer." + std::to_string(i)] = std::move(w);
    }
    CHECK(live.size() == base + 14);
    {
      Image<T> w; w.N = 99;                                                                       // a key packed again: the old images go
      CHECK(w.bf.reserve(5) == 0 && w.f32.reserve(5) == 0);
      pw["layer.3"] = std::move(w);
    }
    CHECK(live.size() == base + 14 && pw["layer.3"].N == 99 && pw["layer.3"].bf.cap() == 5);
    const Image<T>& ref = pw["layer.2"];
    CHECK(ref.N == 2 && live.count(ref.bf.get()) == 1);
    pw.erase("layer.2");
    CHECK(live.size() == base + 12);
    pw.clear();
    CHECK(live.size() == base);
  }
}

int main() {
  run<float>();
  run<char>();
  CHECK(live.empty() && allocs == frees && allocs > 0);
  printf("ok %ld %ld\n", allocs, frees);
  return 0;
}
"""


def test_devbuf_ownership_growth_and_failure_paths(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    src = tmp_path / "devmem_host.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "devmem_host"
    subprocess.check_call([gxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(REPO, "rift_amd", "csrc"), str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    word, allocs, frees = r.stdout.split()
    assert word == "ok" and int(allocs) == int(frees) > 0
