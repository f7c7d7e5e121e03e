// net_weights.h -- where a network's tensors lie in its packed weight buffer, and the one packer (sam.hip, unet.hip, clip.hip).
// A network's plan derives from WeightPlan, add()s its tensors in the order its Python module lists them and keeps the indices it
// needs by name; *_weights_bytes answers align_up(total floats), *_pack_weights is pack_weights with the network's few special tensors.
#pragma once

#include "soar_common.h"

#include <vector>

namespace soar {
namespace {

struct WeightPlan {
    std::vector<size_t> off, n;        // floats: where a tensor starts in the packed buffer (a multiple of 4), how many the source holds
    std::vector<char> mat;             // the B operand of a matrix product: laid as 16-bit values where `half` asks for them
    size_t total = 0, floats = 0;      // floats of the packed buffer; of the sources
    bool half = false;                 // B operands take half the floats, their starts still 16-byte aligned
    // packed: floats the tensor takes in the buffer where that is not `count` (rows padded by the packer)
    int add(size_t count, size_t packed = 0, bool is_mat = false)
    {
        off.push_back(total); n.push_back(count); mat.push_back(is_mat); floats += count;
        if (!packed) packed = count;
        if (is_mat && half) packed = (packed + 1) / 2;
        total += (packed + 3) / 4 * 4;
        return (int)off.size() - 1;
    }
    int count() const { return (int)off.size(); }
};

constexpr int PACK_COPY = 2;           // special()'s answer for a tensor that is none of its own

// Checks the request against the plan (sizes NULL: the tensors' sizes are the caller's word), then lays tensor i at packed + off[i]:
// special(i, src, dst) answers 0 (laid), 1 (failed, the error set) or PACK_COPY, on which the n[i] floats are copied as they are.
template <class Special>
int pack_weights(const WeightPlan &P, const float *const *tensors, const int64_t *sizes, int count, void *packed, size_t packed_bytes,
                 hipStream_t stream, const char *me, Special special)
{
    if (!tensors || !packed || count != P.count() || packed_bytes < P.total * sizeof(float) || ((uintptr_t)packed & 255)) {
        set_error("%s: need %d tensors%s (got %d) and %zu bytes, 256-byte aligned (got %zu)", me, P.count(), sizes ? " with their sizes" : "",
                  count, P.total * sizeof(float), packed_bytes);
        return 1;
    }
    for (int i = 0; i < count; i++) {
        if (!tensors[i]) { set_error("%s: tensor %d is NULL", me, i); return 1; }
        if (sizes && sizes[i] != (int64_t)P.n[i]) { set_error("%s: tensor %d has %lld floats, the layout %zu", me, i, (long long)sizes[i], P.n[i]); return 1; }
    }
    float *base = static_cast<float *>(packed);
    for (int i = 0; i < count; i++) {
        const int rc = special(i, tensors[i], base + P.off[i]);
        if (rc == PACK_COPY) SOAR_HIP_OK(hipMemcpyAsync(base + P.off[i], tensors[i], P.n[i] * sizeof(float), hipMemcpyDeviceToDevice, stream));
        else if (rc) return 1;
    }
    return 0;
}

}  // namespace
}  // namespace soar
