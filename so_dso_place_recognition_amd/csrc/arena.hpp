// arena.hpp — the layout rule of a handle's ONE scratch allocation: arithmetic alone, no HIP, so a host-only check
// (tests/native/arena_check.cpp) compiles it with a plain compiler.  handle_core.hpp includes it.
#pragma once
#include <cstddef>
#include <cstdint>

namespace pr {

// Offsets of the parts of one allocation, each on a 16-byte boundary: take() returns where a part starts, total is what to allocate.
struct Arena {
  size_t total = 0;
  size_t take(size_t bytes) { const size_t o = total; total += (bytes + 15) & ~(size_t)15; return o; }
};

// the part at `offset` of the allocation at `base`, typed
template <class T>
inline T* at(void* base, size_t offset) { return reinterpret_cast<T*>(static_cast<char*>(base) + offset); }

}  // namespace pr
