// png_common.h -- the checksums that the PNG encoder (png.hip) and decoder (png_decode.hip) share: CRC-32 over a stretch of bytes by the
// 64 lanes of a wavefront, and the joining of Adler-32 values; and the integer sum over a wavefront that both count with.
#pragma once

#include "soar_common.h"

namespace soar {
namespace {

constexpr uint32_t ADLER_MOD = 65521u;
constexpr uint32_t CRC_POLY = 0xEDB88320u;

// over the 64 lanes of a wavefront; every lane gets the result
__device__ __forceinline__ int wave_sum_i(int x)
{
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
    return x;
}

// tab[256] in LDS, by one wavefront
__device__ __forceinline__ void crc_table(uint32_t *tab, int lane)
{
    for (int i = lane; i < 256; i += WAVE) {
        uint32_t c = (uint32_t)i;
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ CRC_POLY : c >> 1;
        tab[i] = c;
    }
}

__device__ __forceinline__ uint32_t crc_bytes(const uint32_t *tab, uint32_t c, const uint8_t *p, int64_t n)
{
    for (int64_t i = 0; i < n; i++) c = tab[(c ^ p[i]) & 255u] ^ (c >> 8);
    return c;
}

// a b modulo the CRC's polynomial, bit 31 being x^0
__device__ __forceinline__ uint32_t mulmod(uint32_t a, uint32_t b)
{
    uint32_t p = 0u;
    for (int i = 31; i >= 0; i--) {
        if ((a >> i) & 1u) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}

// x^(8 k)
__device__ __forceinline__ uint32_t x8n(int64_t k)
{
    uint32_t p = 0x80000000u, base = 0x00800000u;
    for (; k; k >>= 1) {
        if (k & 1) p = mulmod(p, base);
        base = mulmod(base, base);
    }
    return p;
}

// the CRC-32 of out[from, to), which this wavefront has written (or only reads): lane j runs over the j-th stretch (lane 0 from the
// all-ones start), the stretch's register is multiplied by x^(8 bytes behind it), and the XOR of all is the register at the end
__device__ __forceinline__ uint32_t crc_written(const uint32_t *tab, const uint8_t *out, int64_t from, int64_t to, int lane)
{
    __threadfence_block();
    __syncthreads();
    const int64_t m = to - from, q = (m + WAVE - 1) / WAVE;
    const int64_t s = min(m, lane * q), e = min(m, s + q);
    uint32_t c = crc_bytes(tab, lane == 0 ? 0xFFFFFFFFu : 0u, out + from + s, e - s);
    c = mulmod(c, x8n(m - e));
    for (int k = 32; k >= 1; k >>= 1) c ^= (uint32_t)__shfl_xor((int)c, k);
    return ~c;
}

// two Adler-32 values and the second's length -> the value of the two stretches one after the other
__device__ __forceinline__ uint32_t adler_join(uint32_t x, uint32_t y, uint32_t len2_mod)
{
    const uint32_t A1 = x & 0xFFFFu, B1 = x >> 16, A2 = y & 0xFFFFu, B2 = y >> 16;
    const uint32_t A = (A1 + A2 + ADLER_MOD - 1u) % ADLER_MOD;
    const uint32_t B = (uint32_t)((B1 + B2 + (unsigned long long)len2_mod * (A1 + ADLER_MOD - 1u)) % ADLER_MOD);
    return B << 16 | A;
}

}  // namespace
}  // namespace soar
