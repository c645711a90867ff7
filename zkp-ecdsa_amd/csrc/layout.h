// Layouts of the host layer's device buffers.  A layout is a plain struct of pointers plus one function `size_t x_layout(X&, uint8_t* base, ...)` that takes
// its regions off a Carver in a fixed order and returns the bytes it needs; lay_out runs it twice -- on a null base for the size, then, the buffer reserved,
// on the real one.  Nothing here knows HIP: plain g++ compiles it (tests/host_arith/host_layout.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#define ZK_LAYOUT_ALIGN 256
#define ZK_LAYOUT_TAIL 256   // what every layout function adds to the Carver's offset: `return k.off + ZK_LAYOUT_TAIL`
struct Carver {
    uint8_t* base;   // nullptr: the size pass -- every region comes out nullptr
    size_t off = 0;
    explicit Carver(uint8_t* b) : base(b) {}
    void* take(size_t bytes) {
        off = (off + (ZK_LAYOUT_ALIGN - 1)) & ~(size_t)(ZK_LAYOUT_ALIGN - 1);
        void* p = base ? base + off : nullptr;
        off += bytes;
        return p;
    }
};
// layout(base) -> bytes; reserve(bytes, &base) -> 0 and the buffer's address, or the caller's error.  Returns that error, or 0 with the layout carved.
template <class Layout, class Reserve>
auto lay_out(Layout&& layout, Reserve&& reserve) -> decltype(reserve((size_t)0, (uint8_t**)nullptr)) {
    uint8_t* base = nullptr;
    const size_t need = layout(base);
    if (auto err = reserve(need, &base)) return err;
    layout(base);
    return {};
}
