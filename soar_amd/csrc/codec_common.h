// codec_common.h -- the host-side plumbing that the image codecs share (png.hip, video.hip, png_decode.hip, jpeg_decode.hip): the
// encoders' sizes -> offsets step (a scan over the pieces, then one offset per item) with its workspace blocks, and the argument
// checks the entry points have in common.  The kernels and the workspace layouts stay in the codecs' own files; the checksums of PNG
// are in png_common.h.  The carver and the workspace check come from workspace.h, the scans from scan_sort.h.  What launches or scans
// is a template so that it exists only in the files that use it.
#pragma once

#include "scan_sort.h"
#include "workspace.h"

namespace soar {
namespace {

// ---- the encoders: every piece's size, the exclusive scan of the sizes, one offset per item ---------------------------------------
struct SizeScan {
    int64_t *sizes, *offs;      // [n + 1] each; the measuring kernel writes sizes[n] = 0, so that offs[n] is the total
    void *temp;
    size_t temp_bytes;
};

inline void carve_size_scan(Carver &c, SizeScan &s, size_t cnt)
{
    s.sizes = c.take<int64_t>(cnt);
    s.offs = c.take<int64_t>(cnt);
    s.temp_bytes = scan_temp_bytes<int64_t>(cnt);
    s.temp = c.take<char>(s.temp_bytes);
}

template <int = 0>
__global__ void __launch_bounds__(256) item_offsets_kernel(int32_t B, int64_t per_item, const int64_t *__restrict__ offs, int64_t *__restrict__ out)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b <= B) out[b] = offs[(int64_t)b * per_item];
}

// the tail of a *_measure: B >= 1 items of per_item pieces each; out[b] = where item b begins, out[B] = the total
template <int = 0> inline int item_offsets(const char *what, const SizeScan &s, int32_t B, int64_t per_item, int64_t *out, hipStream_t stream)
{
    SOAR_HIP_OK(exclusive_scan_sum(s.temp, s.temp_bytes, s.sizes, s.offs, (size_t)(B * per_item) + 1, stream));
    hipLaunchKernelGGL(item_offsets_kernel<>, dim3((unsigned)(B + 256) / 256), dim3(256), 0, stream, B, per_item, s.offs, out);
    SOAR_LAUNCH_OK(what, stream, 0);
    return 0;
}

// a *_measure of no items: the offsets of nothing
inline int no_item_offsets(int64_t *out, hipStream_t stream)
{
    SOAR_HIP_OK(hipMemsetAsync(out, 0, sizeof(int64_t), stream));
    return 0;
}

// a *_measure's input: B items of item_bytes each, stride bytes apart.  many / one: "images" / "an image"
inline bool batch_ok(const char *me, int32_t B, const void *items, int64_t stride, int64_t item_bytes, const char *many, const char *one)
{
    if (B > 0 && (!items || (B > 1 && stride < item_bytes))) {
        set_error("%s: NULL %s, or %s stride of %lld bytes shorter than %s of %lld", me, many, one, (long long)stride, one, (long long)item_bytes);
        return false;
    }
    return true;
}

// a *_emit's output
inline bool emit_out_ok(const char *me, const uint8_t *out, int64_t capacity)
{
    if (capacity < 0 || (capacity > 0 && !out)) {
        set_error("%s: bad arguments (capacity=%lld with out %s)", me, (long long)capacity, out ? "given" : "NULL");
        return false;
    }
    return true;
}

// ---- the decoders: what a *_decode of B >= 1 files checks before it launches.  info: "segments" or "intervals" ----------------------
template <class Args>
inline bool decode_ok(const char *me, const Args &a, const void *out, const void *status, const void *info, const char *info_name,
                      const void *workspace, size_t have, size_t need, const char *sizing_call)
{
    if (!a.data || !a.offsets || !out || !status || !info) {
        set_error("%s: NULL data, offsets, out, status or %s", me, info_name);
        return false;
    }
    return workspace_ok(me, workspace, have, need, sizing_call);
}

// ---- a *_workspace_bytes: the file's plan_of without a workspace; never 0, so that there is always a block to allocate and pass ----
template <class Args, class Plan>
inline int workspace_bytes_of(const char *me, bool (*plan_of)(const char *, const Args *, void *, Plan &), const Args *args, size_t *bytes)
{
    Plan p;
    if (!bytes) { set_error("%s: NULL bytes", me); return 1; }
    if (!plan_of(me, args, nullptr, p)) return 1;
    *bytes = p.bytes > 0 ? p.bytes : ALIGN;
    return 0;
}

}  // namespace
}  // namespace soar
