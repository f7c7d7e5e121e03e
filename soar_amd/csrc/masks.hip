// masks.hip -- mask clean-up of the preprocessing (soar_amd/masks.py): the union of a segmenter's K candidate masks,
// a 5 x 5 OPEN then CLOSE, and the largest 8-connected component, for N frames per call.  The reference does this per frame on the
// host with OpenCV (preproc/compute_kp_and_mask.py:68-75); here the candidates stay on the device and everything behind the read of
// the candidates works on bit-planes: bit b of word w of a row is pixel x = 32 w + b, ceil(W / 32) words a row.
//
//   masks_pack_morph_kernel  ONE launch for union, open and close: a workgroup packs a tile of 64 rows x 14 words with a halo of 8
//                            rows and one word (wave ballots over 64 consecutive pixels; uint8 rows of a multiple of 4
//                            pixels by 32-bit loads, 8 lanes a word), runs erode, dilate, dilate, erode as
//                            separable shifted AND / OR passes on two LDS planes, writes its part of the cleaned plane and adds
//                            its popcounts of the union and of the cleaned tile with one integer atomic each.
//                            Border rule (OpenCV's morphologyDefaultBorderValue): an erosion reads every position outside the
//                            image as set, a dilation as unset -- applied by EACH of the four operations to its own input, also to
//                            the rows of the halo that lie outside the image and to the padding bits of a row's last word.
//   ccl_init_kernel          a node per maximal run of set bits inside one word, named by the raster index y W + x of its first
//                            pixel; a run that comes in from the previous word starts out hooked to the first node of the row run
//   ccl_hook_kernel          per word: every node is united with the nodes of the row above that touch it (8-connectivity:
//                            also the diagonal neighbours across the word boundaries); atomicMin hooking as in mesh.hip, so a
//                            component's root is its smallest raster index whatever the order of the hooks
//   ccl_flatten_kernel       every node points at its root
//   ccl_count_kernel         integer adds at the root, one per wave and root (a row run inside a wave's 64 words is one add): a
//                            root r then holds r + area (so root <=> value > own index), every other node its root
//   ccl_winner_kernel        per root a 64-bit atomicMax of area << 32 | (0xFFFFFFFF - label): the largest area, the smallest label
//                            among equal areas; the number of roots with one atomic per workgroup
//   masks_emit_kernel        bytes 0 / 1 of the bit-plane, restricted to the nodes whose root is the winner
//
// Everything is integer arithmetic; the sums are integer atomics, so outputs and statistics are the same bits in every run.  The
// number of launches does not depend on the images, nothing is read back, nothing is allocated.
#include "workspace.h"

namespace soar {

namespace {

constexpr int MT_ROWS = 64, MT_WORDS = 14, MT_HALO = 8;       // output rows / words of a tile, halo rows (4 operations x radius 2)
constexpr int ML_ROWS = MT_ROWS + 2 * MT_HALO, ML_WORDS = MT_WORDS + 2;   // the LDS plane: 80 x 16 words
constexpr int MASK_THREADS = 256;
constexpr int DT_U8 = 0, DT_F32 = 1;

struct PackArgs {
    int N, K, H, W, WPR, dtype, morph;
    float thr;
    const void *cand;
    uint32_t *plane;         // [N][H][WPR]
    int32_t *stats;          // [N][4]
};

// the bits of word w of row y that are pixels of the image
__device__ __forceinline__ uint32_t valid_bits(int y, int w, int H, int W, int WPR)
{
    if (y < 0 || y >= H || w < 0 || w >= WPR) return 0u;
    return (w == WPR - 1 && (W & 31)) ? (1u << (W & 31)) - 1u : 0xFFFFFFFFu;
}

// 1 x 5 pass over the words of a row; the input of an operation gets that operation's border value wherever it is no pixel
template <bool ERODE>
__device__ __forceinline__ void morph_rows(const uint32_t *src, uint32_t *dst, int row0, int word0, int H, int W, int WPR)
{
    for (int i = threadIdx.x; i < ML_ROWS * ML_WORDS; i += MASK_THREADS) {
        const int r = i / ML_WORDS, c = i % ML_WORDS;
        uint32_t v = src[i], L = c > 0 ? src[i - 1] : 0u, R = c < ML_WORDS - 1 ? src[i + 1] : 0u;
        const uint32_t mv = valid_bits(row0 + r, word0 + c, H, W, WPR), mL = valid_bits(row0 + r, word0 + c - 1, H, W, WPR),
                       mR = valid_bits(row0 + r, word0 + c + 1, H, W, WPR);
        if (ERODE) { v |= ~mv; L |= ~mL; R |= ~mR; }
        else { v &= mv; L &= mL; R &= mR; }
        const uint32_t l1 = (v << 1) | (L >> 31), l2 = (v << 2) | (L >> 30), r1 = (v >> 1) | (R << 31), r2 = (v >> 2) | (R << 30);
        dst[i] = ERODE ? (v & l1 & l2 & r1 & r2) : (v | l1 | l2 | r1 | r2);
    }
}

// 5 x 1 pass; rows beyond the LDS plane are left out (what they would change lies inside the halo that is thrown away)
template <bool ERODE>
__device__ __forceinline__ void morph_cols(const uint32_t *src, uint32_t *dst)
{
    for (int i = threadIdx.x; i < ML_ROWS * ML_WORDS; i += MASK_THREADS) {
        const int r = i / ML_WORDS;
        uint32_t v = src[i];
#pragma unroll
        for (int d = -2; d <= 2; d++) {
            if (d == 0 || r + d < 0 || r + d >= ML_ROWS) continue;
            const uint32_t o = src[i + d * ML_WORDS];
            v = ERODE ? (v & o) : (v | o);
        }
        dst[i] = v;
    }
}

__device__ __forceinline__ int block_sum(int v, int *red)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

template <int DT, bool VEC>
__global__ void __launch_bounds__(MASK_THREADS) masks_pack_morph_kernel(PackArgs a)
{
    __shared__ uint32_t A[ML_ROWS * ML_WORDS], B[ML_ROWS * ML_WORDS];
    __shared__ int red[4];
    const int n = blockIdx.z, row0 = blockIdx.y * MT_ROWS - MT_HALO, word0 = blockIdx.x * MT_WORDS - 1;
    const int H = a.H, W = a.W, WPR = a.WPR, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t image = (size_t)H * W;

    // union of the K candidates
    if (VEC) {
        // uint8 rows of a multiple of 4 pixels: a lane reads 4 pixels, 8 lanes make a word, a wave 8 words
        for (int u = wave; u < ML_ROWS * (ML_WORDS / 8); u += MASK_THREADS / 64) {
            const int r = u / (ML_WORDS / 8), c = (u % (ML_WORDS / 8)) * 8 + (lane >> 3), y = row0 + r;
            const bool wanted = a.morph || (r >= MT_HALO && r < MT_HALO + MT_ROWS);
            uint32_t v = 0;
            if (wanted && y >= 0 && y < H) {                                                   // wave-uniform
                const int x = (word0 + c) * 32 + (lane & 7) * 4;
                if (x >= 0 && x < W) {
                    const size_t at = (size_t)n * a.K * image + (size_t)y * W + x;
                    uint32_t q = 0;
                    for (int k = 0; k < a.K; k++) {
                        const uint32_t b4 = *reinterpret_cast<const uint32_t *>(static_cast<const uint8_t *>(a.cand) + at + k * image);
                        uint32_t t = b4 | (b4 >> 4);         // within each byte: bits 0 .. 3 = low nibble | high nibble
                        t |= t >> 2;
                        t |= t >> 1;                         // bit 0 of every byte: the byte is non-zero (higher bits: mixed, dropped)
                        q |= t & 0x01010101u;
                    }
                    v = ((q & 1u) | ((q >> 7) & 2u) | ((q >> 14) & 4u) | ((q >> 21) & 8u)) << ((lane & 7) * 4);
                }
            }
            v |= (uint32_t)__shfl_xor((int)v, 1);
            v |= (uint32_t)__shfl_xor((int)v, 2);
            v |= (uint32_t)__shfl_xor((int)v, 4);
            if ((lane & 7) == 0) A[r * ML_WORDS + c] = v;
        }
    } else {
        // 64 consecutive pixels (two words) per ballot
        for (int u = wave; u < ML_ROWS * (ML_WORDS / 2); u += MASK_THREADS / 64) {
            const int r = u / (ML_WORDS / 2), c = (u % (ML_WORDS / 2)) * 2, y = row0 + r;
            const bool wanted = a.morph || (r >= MT_HALO && r < MT_HALO + MT_ROWS);
            uint64_t bits = 0;
            if (wanted && y >= 0 && y < H && word0 + c + 1 >= 0 && word0 + c < WPR) {          // wave-uniform
                const int x = (word0 + c) * 32 + lane;
                bool set = false;
                if (x >= 0 && x < W) {
                    const size_t at = (size_t)n * a.K * image + (size_t)y * W + x;
                    for (int k = 0; k < a.K; k++) {
                        if (DT == DT_U8) set |= static_cast<const uint8_t *>(a.cand)[at + k * image] != 0;
                        else set |= static_cast<const float *>(a.cand)[at + k * image] > a.thr;      // false for NaN, for -0.0 > 0.0
                    }
                }
                bits = __ballot(set);
            }
            if (lane == 0) {
                A[r * ML_WORDS + c] = (uint32_t)bits;
                A[r * ML_WORDS + c + 1] = (uint32_t)(bits >> 32);
            }
        }
    }
    __syncthreads();

    // this tile's own words: rows [MT_HALO, MT_HALO + MT_ROWS), words [1, 1 + MT_WORDS) of the LDS plane
    int uni = 0;
    for (int i = threadIdx.x; i < MT_ROWS * MT_WORDS; i += MASK_THREADS) {
        const int r = MT_HALO + i / MT_WORDS, c = 1 + i % MT_WORDS;
        uni += __popc(A[r * ML_WORDS + c]);              // nothing was loaded outside the image
    }
    if (a.morph) {
        morph_rows<true>(A, B, row0, word0, H, W, WPR);   __syncthreads();      // OPEN: erode ...
        morph_cols<true>(B, A);                                  __syncthreads();
        morph_rows<false>(A, B, row0, word0, H, W, WPR);  __syncthreads();      // ... dilate
        morph_cols<false>(B, A);                                 __syncthreads();
        morph_rows<false>(A, B, row0, word0, H, W, WPR);  __syncthreads();      // CLOSE: dilate ...
        morph_cols<false>(B, A);                                 __syncthreads();
        morph_rows<true>(A, B, row0, word0, H, W, WPR);   __syncthreads();      // ... erode
        morph_cols<true>(B, A);                                  __syncthreads();
    }
    int cleaned = 0;
    for (int i = threadIdx.x; i < MT_ROWS * MT_WORDS; i += MASK_THREADS) {
        const int r = MT_HALO + i / MT_WORDS, c = 1 + i % MT_WORDS, y = row0 + r, w = word0 + c;
        if (y < H && w < WPR) {                          // (y >= 0 and w >= 0 for a tile's own words)
            const uint32_t v = A[r * ML_WORDS + c] & valid_bits(y, w, H, W, WPR);       // padding bits leave as zeros
            a.plane[((size_t)n * H + y) * WPR + w] = v;
            cleaned += __popc(v);
        }
    }
    uni = block_sum(uni, red);
    cleaned = block_sum(cleaned, red);
    if (threadIdx.x == 0) {
        if (uni) atomicAdd(a.stats + 4 * n, uni);
        if (cleaned) atomicAdd(a.stats + 4 * n + 1, cleaned);
    }
}

// ---- connected components over the bit-plane -------------------------------------------------------------------------------------

struct CclArgs {
    int N, H, W, WPR;
    const uint32_t *plane;   // [N][H][WPR], padding bits zero
    int32_t *parent;         // [N][H W]: only the slots of run starts are used
    unsigned long long *key; // [N]
    int32_t *stats;          // [N][4]
    uint8_t *out;            // [N][H][W]
    int select;              // emit: 1 = the winner's nodes only, 0 = the plane as it is
};

__device__ __forceinline__ int uf_find(int32_t *parent, int x)
{
    for (;;) {
        const int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        x = p;
    }
}

// hook the larger root under the smaller one; when the larger one was hooked elsewhere in the meantime the union continues from
// that parent, so no link is lost and every component ends at its least id (mesh.hip's uf_union)
__device__ __forceinline__ void uf_union(int32_t *parent, int a, int b)
{
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + a, b);
        if (old == a) return;
        a = old;
    }
}

// the lowest run of ones of a non-zero word
__device__ __forceinline__ uint32_t lowest_run(uint32_t rest)
{
    return rest & ~(rest + (rest & (0u - rest)));
}

// first bit of the run of v that holds bit b (which is set)
__device__ __forceinline__ int run_start(uint32_t v, int b)
{
    const uint32_t below = ~v & ((1u << b) - 1u);
    return below ? 32 - __clz(below) : 0;
}

// word index of the launch -> frame, row, word; false past the end
__device__ __forceinline__ bool ccl_word(const CclArgs &a, int &n, int &y, int &w)
{
    const long long g = (long long)blockIdx.x * MASK_THREADS + threadIdx.x;
    n = blockIdx.y;
    if (g >= (long long)a.H * a.WPR) return false;
    y = (int)(g / a.WPR);
    w = (int)(g % a.WPR);
    return true;
}

__global__ void __launch_bounds__(MASK_THREADS) ccl_init_kernel(CclArgs a)
{
    int n, y, w;
    if (!ccl_word(a, n, y, w)) return;
    const uint32_t *row = a.plane + ((size_t)n * a.H + y) * a.WPR;
    int32_t *parent = a.parent + (size_t)n * a.H * a.W;
    uint32_t rest = row[w];
    const int base = y * a.W + 32 * w;
    while (rest) {
        const uint32_t seg = lowest_run(rest);
        rest &= ~seg;
        const int b = __ffs(seg) - 1;
        int p = base + b;
        if (b == 0 && w > 0 && (row[w - 1] >> 31)) {        // the run comes in from the left: walk to the word it starts in
            int ww = w - 1;
            uint32_t pv = row[ww];
            while (pv == 0xFFFFFFFFu && ww > 0 && (row[ww - 1] >> 31)) pv = row[--ww];
            p = y * a.W + 32 * ww + run_start(pv, 31);
        }
        parent[base + b] = p;
    }
}

__global__ void __launch_bounds__(MASK_THREADS) ccl_hook_kernel(CclArgs a)
{
    int n, y, w;
    if (!ccl_word(a, n, y, w) || y == 0) return;
    const uint32_t *row = a.plane + ((size_t)n * a.H + y) * a.WPR, *above = row - a.WPR;
    int32_t *parent = a.parent + (size_t)n * a.H * a.W;
    uint32_t rest = row[w];
    if (!rest) return;
    const uint32_t up = above[w], upL = w > 0 ? above[w - 1] : 0u, upR = w + 1 < a.WPR ? above[w + 1] : 0u;
    const int base = y * a.W + 32 * w, ubase = base - a.W;
    while (rest) {
        const uint32_t seg = lowest_run(rest);
        rest &= ~seg;
        const int s = base + __ffs(seg) - 1;
        uint32_t t = up & (seg | (seg << 1) | (seg >> 1));
        while (t) {                                       // every node of the word above that touches this one, once
            const int st = run_start(up, __ffs(t) - 1);
            const uint32_t x = up >> st;
            const uint32_t run = x == 0xFFFFFFFFu ? x : ((1u << (__ffs(~x) - 1)) - 1u) << st;
            t &= ~run;
            uf_union(parent, s, ubase + st);
        }
        if ((seg & 1u) && (upL >> 31)) uf_union(parent, s, ubase - 32 + run_start(upL, 31));
        if ((seg >> 31) && (upR & 1u)) uf_union(parent, s, ubase + 32);
    }
}

// after the hooks the forest is static: every node gets its root (a concurrent reader sees the old parent or the root, both ancestors)
__global__ void __launch_bounds__(MASK_THREADS) ccl_flatten_kernel(CclArgs a)
{
    int n, y, w;
    if (!ccl_word(a, n, y, w)) return;
    int32_t *parent = a.parent + (size_t)n * a.H * a.W;
    uint32_t rest = a.plane[((size_t)n * a.H + y) * a.WPR + w];
    const int base = y * a.W + 32 * w;
    while (rest) {
        const uint32_t seg = lowest_run(rest);
        rest &= ~seg;
        const int s = base + __ffs(seg) - 1, r = uf_find(parent, s);
        if (r != s) __hip_atomic_store(parent + s, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// a root is the least index of its component: after this pass slot r of a root holds r + area > r, every other node's slot its
// root < the node.  Indices and areas are below 2^31, their sum fits the unsigned word.
__global__ void __launch_bounds__(MASK_THREADS) ccl_count_kernel(CclArgs a)
{
    int n, y, w;
    const bool in = ccl_word(a, n, y, w);
    uint32_t *slot = reinterpret_cast<uint32_t *>(a.parent + (size_t)n * a.H * a.W);
    uint32_t rest = in ? a.plane[((size_t)n * a.H + y) * a.WPR + w] : 0u;
    const uint32_t base = in ? (uint32_t)(y * a.W + 32 * w) : 0u;
    const int lane = threadIdx.x & 63;
    while (__any(rest != 0u)) {                           // every lane's next node; the lanes that name the same root add once
        uint32_t cnt = 0, target = 0;
        if (rest) {
            const uint32_t seg = lowest_run(rest);
            rest &= ~seg;
            const uint32_t s = base + (uint32_t)(__ffs(seg) - 1);
            const uint32_t p = __hip_atomic_load(slot + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            target = p < s ? p : s;
            cnt = (uint32_t)__popc(seg);
        }
        unsigned long long todo = __ballot(cnt != 0u);
        while (todo) {
            const int leader = __ffsll(todo) - 1;
            const uint32_t t = (uint32_t)__shfl((int)target, leader);
            const bool mine = cnt != 0u && target == t;
            int v = mine ? (int)cnt : 0;
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if (lane == leader) atomicAdd(slot + t, (uint32_t)v);
            todo &= ~__ballot(mine);
        }
    }
}

__global__ void __launch_bounds__(MASK_THREADS) ccl_winner_kernel(CclArgs a)
{
    __shared__ int red[4];
    int n, y, w, roots = 0;
    if (ccl_word(a, n, y, w)) {
        const uint32_t *slot = reinterpret_cast<const uint32_t *>(a.parent + (size_t)n * a.H * a.W);
        uint32_t rest = a.plane[((size_t)n * a.H + y) * a.WPR + w];
        const uint32_t base = (uint32_t)(y * a.W + 32 * w);
        while (rest) {
            const uint32_t seg = lowest_run(rest);
            rest &= ~seg;
            const uint32_t s = base + (uint32_t)(__ffs(seg) - 1), p = slot[s];
            if (p > s) {
                roots++;
                atomicMax(a.key + n, ((unsigned long long)(p - s) << 32) | (0xFFFFFFFFu - s));
            }
        }
    }
    roots = block_sum(roots, red);
    if (threadIdx.x == 0 && roots) atomicAdd(a.stats + 4 * n + 2, roots);
}

__global__ void __launch_bounds__(MASK_THREADS) masks_emit_kernel(CclArgs a)
{
    __shared__ uint32_t keep[MASK_THREADS];
    int n, y, w;
    uint32_t k = 0;
    const bool in = ccl_word(a, n, y, w);
    if (in) {
        const uint32_t v = a.plane[((size_t)n * a.H + y) * a.WPR + w];
        if (!a.select) k = v;
        else {
            const unsigned long long key = a.key[n];
            const uint32_t win = 0xFFFFFFFFu - (uint32_t)key;               // no component: key = 0, and no word has a bit
            const uint32_t *slot = reinterpret_cast<const uint32_t *>(a.parent + (size_t)n * a.H * a.W);
            const uint32_t base = (uint32_t)(y * a.W + 32 * w);
            uint32_t rest = v;
            while (rest) {
                const uint32_t seg = lowest_run(rest);
                rest &= ~seg;
                const uint32_t s = base + (uint32_t)(__ffs(seg) - 1), p = slot[s];
                if ((p < s ? p : s) == win) k |= seg;
            }
            if (blockIdx.x == 0 && threadIdx.x == 0) a.stats[4 * n + 3] = (int32_t)(key >> 32);
        }
    }
    keep[threadIdx.x] = k;
    __syncthreads();
    // the bytes of this workgroup's 256 words, consecutive threads on consecutive pixels
    const long long words = (long long)a.H * a.WPR, first = (long long)blockIdx.x * MASK_THREADS;
    uint8_t *out = a.out + (size_t)n * a.H * a.W;
    for (int i = threadIdx.x; i < MASK_THREADS * 32; i += MASK_THREADS) {
        const long long g = first + (i >> 5);
        if (g >= words) break;
        const int yy = (int)(g / a.WPR), x = (int)(g % a.WPR) * 32 + (i & 31);
        if (x < a.W) out[(size_t)yy * a.W + x] = (uint8_t)((keep[i >> 5] >> (i & 31)) & 1u);
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------

constexpr int MASKS_MAX_FRAMES = 65535;               // the frame is a grid dimension
constexpr int MASKS_MAX_ROWS = 65535 * MT_ROWS;        // ... and so is the row of tiles

struct Layout {
    size_t key, plane, parent, total;
    int WPR;
};

bool masks_shape(const char *what, int N, int K, int H, int W)
{
    if (N < 1 || K < 1 || H < 1 || W < 1) { set_error("%s: need N, K, H, W >= 1 (N=%d, K=%d, H=%d, W=%d)", what, N, K, H, W); return false; }
    if (N > MASKS_MAX_FRAMES) { set_error("%s: at most %d frames per call (N=%d)", what, MASKS_MAX_FRAMES, N); return false; }
    if (H > MASKS_MAX_ROWS) { set_error("%s: at most %d rows (H=%d)", what, MASKS_MAX_ROWS, H); return false; }
    if ((long long)H * W >= (1ll << 31)) { set_error("%s: %d x %d pixels: H*W must stay below 2^31", what, H, W); return false; }
    return true;
}

Layout masks_layout(int N, int H, int W)
{
    Layout l;
    Carver c;
    l.WPR = (W + 31) / 32;
    l.key = c.offset<unsigned long long>((size_t)N);
    l.plane = c.offset<uint32_t>((size_t)N * H * l.WPR);
    l.parent = c.offset<int32_t>((size_t)N * H * W);
    l.total = c.bytes();
    return l;
}

int launch_pack(int N, int K, int H, int W, const void *cand, int dtype, float thr, int morph, const Layout &l, void *workspace,
                int32_t *stats, hipStream_t stream)
{
    char *ws = static_cast<char *>(workspace);
    SOAR_HIP_OK(hipMemsetAsync(stats, 0, (size_t)N * 4 * sizeof(int32_t), stream));
    SOAR_HIP_OK(hipMemsetAsync(ws + l.key, 0, (size_t)N * sizeof(unsigned long long), stream));
    PackArgs a{N, K, H, W, l.WPR, dtype, morph, thr, cand, reinterpret_cast<uint32_t *>(ws + l.plane), stats};
    const dim3 grid((unsigned)((l.WPR + MT_WORDS - 1) / MT_WORDS), (unsigned)((H + MT_ROWS - 1) / MT_ROWS), (unsigned)N);
    // uint8 rows that start on 4-byte boundaries are read 4 pixels a lane
    const bool vec = dtype == DT_U8 && W % 4 == 0 && reinterpret_cast<uintptr_t>(cand) % 4 == 0;
    if (vec) hipLaunchKernelGGL((masks_pack_morph_kernel<DT_U8, true>), grid, dim3(MASK_THREADS), 0, stream, a);
    else if (dtype == DT_U8) hipLaunchKernelGGL((masks_pack_morph_kernel<DT_U8, false>), grid, dim3(MASK_THREADS), 0, stream, a);
    else hipLaunchKernelGGL((masks_pack_morph_kernel<DT_F32, false>), grid, dim3(MASK_THREADS), 0, stream, a);
    SOAR_LAUNCH_OK("masks_pack_morph", stream, 0);
    return 0;
}

int launch_emit(int N, int H, int W, int select, const Layout &l, void *workspace, uint8_t *out, int32_t *stats, hipStream_t stream)
{
    char *ws = static_cast<char *>(workspace);
    CclArgs a{N, H, W, l.WPR, reinterpret_cast<uint32_t *>(ws + l.plane), reinterpret_cast<int32_t *>(ws + l.parent),
              reinterpret_cast<unsigned long long *>(ws + l.key), stats, out, select};
    const dim3 grid((unsigned)(((long long)H * l.WPR + MASK_THREADS - 1) / MASK_THREADS), (unsigned)N), block(MASK_THREADS);
    if (select) {
        hipLaunchKernelGGL(ccl_init_kernel, grid, block, 0, stream, a);
        SOAR_LAUNCH_OK("ccl_init", stream, 0);
        hipLaunchKernelGGL(ccl_hook_kernel, grid, block, 0, stream, a);
        SOAR_LAUNCH_OK("ccl_hook", stream, 0);
        hipLaunchKernelGGL(ccl_flatten_kernel, grid, block, 0, stream, a);
        SOAR_LAUNCH_OK("ccl_flatten", stream, 0);
        hipLaunchKernelGGL(ccl_count_kernel, grid, block, 0, stream, a);
        SOAR_LAUNCH_OK("ccl_count", stream, 0);
        hipLaunchKernelGGL(ccl_winner_kernel, grid, block, 0, stream, a);
        SOAR_LAUNCH_OK("ccl_winner", stream, 0);
    }
    hipLaunchKernelGGL(masks_emit_kernel, grid, block, 0, stream, a);
    SOAR_LAUNCH_OK("masks_emit", stream, 0);
    return 0;
}

int masks_run(const char *what, int N, int K, int H, int W, const void *cand, int dtype, float thr, int morph, int select, uint8_t *out,
              int32_t *stats, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (!masks_shape(what, N, K, H, W)) return 1;
    if (!cand || !out || !stats) { set_error("%s: NULL argument", what); return 1; }
    if (dtype != DT_U8 && dtype != DT_F32) { set_error("%s: unknown dtype code %d (0: uint8 / bool, 1: float32)", what, dtype); return 1; }
    const Layout l = masks_layout(N, H, W);
    if (!workspace_ok(what, workspace, workspace_bytes, l.total, "soar_masks_workspace_bytes")) return 1;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (launch_pack(N, K, H, W, cand, dtype, thr, morph, l, workspace, stats, stream)) return 1;
    return launch_emit(N, H, W, select, l, workspace, out, stats, stream);
}

}  // namespace
}  // namespace soar

using namespace soar;

extern "C" int soar_masks_workspace_bytes(int32_t N, int32_t H, int32_t W, size_t *bytes)
{
    if (!bytes) { set_error("soar_masks_workspace_bytes: NULL argument"); return 1; }
    if (!masks_shape("soar_masks_workspace_bytes", N, 1, H, W)) return 1;
    *bytes = masks_layout(N, H, W).total;
    return 0;
}

extern "C" int soar_masks_open_close(int32_t N, int32_t K, int32_t H, int32_t W, const void *cand, int32_t dtype, float threshold,
                                     uint8_t *out, int32_t *stats, void *workspace, size_t workspace_bytes, void *stream)
{
    return masks_run("soar_masks_open_close", N, K, H, W, cand, dtype, threshold, 1, 0, out, stats, workspace, workspace_bytes, stream);
}

extern "C" int soar_masks_largest_component(int32_t N, int32_t H, int32_t W, const uint8_t *mask, uint8_t *out, int32_t *stats,
                                            void *workspace, size_t workspace_bytes, void *stream)
{
    return masks_run("soar_masks_largest_component", N, 1, H, W, mask, DT_U8, 0.f, 0, 1, out, stats, workspace, workspace_bytes, stream);
}

extern "C" int soar_masks_clean(int32_t N, int32_t K, int32_t H, int32_t W, const void *cand, int32_t dtype, float threshold,
                                uint8_t *out, int32_t *stats, void *workspace, size_t workspace_bytes, void *stream)
{
    return masks_run("soar_masks_clean", N, K, H, W, cand, dtype, threshold, 1, 1, out, stats, workspace, workspace_bytes, stream);
}
