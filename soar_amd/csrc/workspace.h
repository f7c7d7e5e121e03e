// workspace.h -- the one rule every caller-owned workspace follows, and the one check of it.  Blocks lie one after the other, each
// rounded up to 256 bytes; a sizing call (*_bytes) runs the same layout code on a NULL base, so that the size and the carving cannot
// disagree.  Every file that takes a workspace through the C ABI carves it with Carver and judges it with workspace_ok; only the
// rasterizer's state buffers (api.hip) have a layout of their own.
#pragma once

#include "soar_common.h"

namespace soar {

namespace {

// Blocks of a workspace.  With a NULL base (a _bytes query, or a layout that is computed once and added to a base later) take()
// answers NULL and only the offset advances: a NULL pointer takes no part in pointer arithmetic.
struct Carver {
    char *base;
    size_t off = 0;
    explicit Carver(void *workspace = nullptr) : base(static_cast<char *>(workspace)) {}
    // the byte offset of the next block, of count T's
    template <class T> size_t offset(size_t count)
    {
        const size_t o = off;
        off += align_up(count * sizeof(T));
        return o;
    }
    // the same in floats: the packed weights of the nets are indexed that way (64 floats = 256 bytes)
    size_t float_offset(size_t floats) { return offset<float>(floats) / sizeof(float); }
    template <class T> T *take(size_t count)
    {
        const size_t o = offset<T>(count);
        return base ? reinterpret_cast<T *>(base + o) : nullptr;
    }
    size_t bytes() const { return off; }
};

// sizing_call: the *_bytes function that answers `need`
inline bool workspace_ok(const char *what, const void *workspace, size_t have, size_t need, const char *sizing_call, size_t align = ALIGN)
{
    if (!workspace || ((uintptr_t)workspace & (align - 1))) {
        set_error("%s: NULL workspace or workspace not %zu-byte aligned", what, align);
        return false;
    }
    if (have < need) { set_error("%s: workspace of %zu bytes, need %zu (%s)", what, have, need, sizing_call); return false; }
    return true;
}

}  // namespace

}  // namespace soar
