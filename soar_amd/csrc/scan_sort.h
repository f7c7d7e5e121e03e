// scan_sort.h -- rocPRIM's scans and radix sorts as the mesh-export files and the codecs call them: the temporary-size queries
// (nothing runs, nothing is read) and the runs.  A run takes the carved size by value and checks it.  Everything is a template, so
// that rocPRIM's kernels exist only in the files that use them.
#pragma once

#include "soar_common.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace soar {

namespace {

template <class T> inline size_t scan_temp_bytes(size_t n, hipStream_t stream = 0)
{
    size_t bytes = 0;
    (void)rocprim::exclusive_scan((void *)nullptr, bytes, (T *)nullptr, (T *)nullptr, (T)0, n, rocprim::plus<T>(), stream);
    return bytes;
}

template <class K> inline size_t sort_keys_temp_bytes(size_t n, unsigned end_bit, hipStream_t stream = 0)
{
    size_t bytes = 0;
    (void)rocprim::radix_sort_keys((void *)nullptr, bytes, (K *)nullptr, (K *)nullptr, n, 0u, end_bit, stream);
    return bytes;
}

template <class K, class V> inline size_t sort_pairs_temp_bytes(size_t n, unsigned end_bit, hipStream_t stream = 0)
{
    size_t bytes = 0;
    (void)rocprim::radix_sort_pairs((void *)nullptr, bytes, (K *)nullptr, (K *)nullptr, (V *)nullptr, (V *)nullptr, n, 0u, end_bit, stream);
    return bytes;
}

template <class T> inline hipError_t exclusive_scan_sum(void *temp, size_t temp_bytes, T *in, T *out, size_t n, hipStream_t stream)
{
    return rocprim::exclusive_scan(temp, temp_bytes, in, out, (T)0, n, rocprim::plus<T>(), stream);
}

// stable, ascending, on the bits [0, end_bit)
template <class K> inline hipError_t sort_keys(void *temp, size_t temp_bytes, K *in, K *out, size_t n, unsigned end_bit, hipStream_t stream)
{
    return rocprim::radix_sort_keys(temp, temp_bytes, in, out, n, 0u, end_bit, stream);
}

template <class K, class V>
inline hipError_t sort_pairs(void *temp, size_t temp_bytes, K *keys, K *keys_out, V *vals, V *vals_out, size_t n, unsigned end_bit,
                             hipStream_t stream)
{
    return rocprim::radix_sort_pairs(temp, temp_bytes, keys, keys_out, vals, vals_out, n, 0u, end_bit, stream);
}

}  // namespace

}  // namespace soar
