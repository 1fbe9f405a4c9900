// ngp_workspace.h -- how the ops of libngp_hip.so lay out the workspaces their callers allocate.  Plain C++, no HIP.
//
// The rule (DESIGN.md "Workspaces"): every op has ONE layout function, xx_layout(shape..., void* base), that carves its pieces with ngp_carver and
// returns their pointers plus `total`.  ngp_xx_workspace(shape...) is that function on a null base; the entry point calls it on the caller's pointer.
// Sizes and offsets are part of the C ABI.  (A layout carves inside a braced initialiser: its clauses are evaluated in the order written.)
#pragma once

#include <stddef.h>
#include <stdint.h>

static inline size_t ngp_align256(size_t n) { return (n + 255) & ~(size_t)255; }

// Bump allocator over a block that may not exist: with a null base it only counts.  It never reads or writes the block.
struct ngp_carver {
    unsigned char* base;
    size_t used = 0;
    explicit ngp_carver(void* b) : base(static_cast<unsigned char*>(b)) {}
    template <typename T>
    T* take(size_t count, size_t align = 256) {        // `count` elements of T at the next multiple of `align` (a power of two; 1 = right behind the piece before)
        used = (used + align - 1) & ~(align - 1);
        T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
        used += count * sizeof(T);
        return p;
    }
    size_t total(size_t align = 1) const { return (used + align - 1) & ~(align - 1); }     // bytes carved so far, rounded up to `align`
};

template <typename T> struct ngp_array_ws { T* p; size_t total; };                          // the layout of a buffer that is one array
template <typename T> static inline ngp_array_ws<T> ngp_array_layout(size_t count, void* base) { return {ngp_carver(base).take<T>(count, 1), count * sizeof(T)}; }

// whether a workspace of `bytes` bytes at `base` reaches the end of `piece_bytes` bytes at `piece` (for ops that run with a short workspace)
static inline bool ngp_ws_holds(const void* base, size_t bytes, const void* piece, size_t piece_bytes) {
    return (size_t)(static_cast<const unsigned char*>(piece) - static_cast<const unsigned char*>(base)) + piece_bytes <= bytes;
}
