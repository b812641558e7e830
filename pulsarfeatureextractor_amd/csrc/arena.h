// arena.h — bump allocator over one block of device scratch, with a measuring mode.
//
// A layout is one function that walks an Arena and returns a struct of typed pointers.  The
// walk on Arena{} (base 0) measures: bytes() is what the layout needs and the pointers mean
// nothing -- never branch on one, branch on the condition that decided whether to take it.
// The same walk on Arena{(uintptr_t)block} places: size and placement cannot disagree.
// Host-only, no HIP calls.  The block is 256-byte aligned (hipMalloc) and so is every region.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace pfe {

struct Arena {
  struct Region {
    const char* name;
    size_t off, bytes;
  };
  uintptr_t base = 0;  // 0: measure only
  size_t off = 0;
  std::vector<Region>* trace = nullptr;  // tests: every region taken, in order

  // a 256-aligned region of count * sizeof(T) bytes
  template <class T>
  T* take(size_t count, const char* name) {
    const size_t b = count * sizeof(T);
    if (trace) trace->push_back({name, off, b});
    T* p = reinterpret_cast<T*>(base + off);
    off += (b + 255) & ~(size_t)255;
    return p;
  }
  size_t bytes() const { return off; }  // extent so far (a multiple of 256)
};

}  // namespace pfe
