// fitviz.hip -- SMPLify fit inspection (soar_amd/fitviz.py): the image stage of the reference's
// SMPLify.visualize_params, so that only finished uint8 strips leave the device.
//   soar_fitviz_yaw_views   the fitted body and its copies turned about the camera's up axis through a pivot.  One thread per vertex.
//   soar_fitviz_strip       five panels per frame: keypoint discs (and, opt-in, limbs) over the photograph, the body's normal render
//                           over the photograph, and the normal renders of the yaw views.  One workgroup per 64 x 16 tile.
//   soar_fitviz_residuals   per frame the number of confident keypoints and the mean / largest pixel distance.  One wavefront per frame.
// Compiled with -ffp-contract=off.  Integer and un-contracted float32 arithmetic only, no atomics: the bits are reproducible, and a
// frame's output depends neither on N nor on its place.  tests/fitviz_ref.py restates all three from include/soar_hip.h.
#include "soar_common.h"

namespace soar {
namespace {

constexpr int YAW_THREADS = 256;
constexpr int MAX_VIEWS = 16;
constexpr int MAX_K = 512, MAX_L = 512;           // keypoints per set, limbs
constexpr int TILE_W = 64, TILE_H = 16;           // output pixels of a workgroup's tile
constexpr int STRIP_THREADS = 256;                // 16 lanes x 4 pixels a row, 16 rows
constexpr int ROW_WORDS = 50;                     // 48 dwords of the tile's row, one of the pixel behind it, one never read past
constexpr int COORD_LIMIT = 1 << 20;
constexpr int32_t NOT_DRAWN = INT32_MIN;
constexpr uint32_t LIMB_UNNAMED = 1u << 31;

// ---- yaw views -----------------------------------------------------------------------------------------------------------------
struct YawDev {
    int32_t N, V, n_views;
    const float *verts, *pivot, *R;
    int64_t sn, sv, sc;
    float *out;
};

__global__ void __launch_bounds__(YAW_THREADS) yaw_views_kernel(YawDev a)
{
    const int64_t idx = (int64_t)blockIdx.x * YAW_THREADS + threadIdx.x;
    if (idx >= (int64_t)a.N * a.V) return;
    const int n = (int)(idx / a.V), v = (int)(idx - (int64_t)n * a.V);
    const float *src = a.verts + n * a.sn + v * a.sv;
    const float x[3] = {src[0], src[a.sc], src[2 * a.sc]};
    const float p[3] = {a.pivot[n * 3], a.pivot[n * 3 + 1], a.pivot[n * 3 + 2]};
    float *dst = a.out + (((int64_t)n * a.n_views) * a.V + v) * 3;
    dst[0] = x[0]; dst[1] = x[1]; dst[2] = x[2];                      // view 0: the bits the objective saw
    const float d[3] = {x[0] - p[0], x[1] - p[1], x[2] - p[2]};
    for (int k = 1; k < a.n_views; k++) {
        const float *r = a.R + (k - 1) * 9;
        dst += (int64_t)a.V * 3;
        for (int i = 0; i < 3; i++)
            dst[i] = ((r[3 * i] * d[0] + r[3 * i + 1] * d[1]) + r[3 * i + 2] * d[2]) + p[i];
    }
}

// ---- the strip -----------------------------------------------------------------------------------------------------------------
struct StripDev {
    int32_t N, H, W, K, L, r2p1, radius, thickness, has_img, OH, RW;   // RW: pixels of an output row (5 W, or (5 W) / 2)
    const float *target_px, *fit_px;
    const uint8_t *kp_mask;
    const int32_t *limbs;
    const uint8_t *limb_rgb;
    const uint8_t *imgs;
    int64_t is_n, is_y, is_x, is_c;
    const float *prior;
    const uint8_t *mask;
    uint32_t target_rgb, fit_rgb;                   // r | g << 8 | b << 16
    uint8_t *out;
};

struct StripLds {
    int32_t cx[2][MAX_K], cy[2][MAX_K];             // the centres of the target set and of the fit set; cx = NOT_DRAWN: nothing to draw
    int32_t la[MAX_L], lb[MAX_L];                   // the limbs' keypoints
    uint32_t lrgb[MAX_L];
    uint16_t surv[2 * MAX_K + 2 * MAX_L];           // the primitives that can reach the tile, in drawing order
    int32_t wave_count[2][STRIP_THREADS / WAVE];
    uint32_t row[TILE_H][ROW_WORDS];                // the tile's bytes, as they go out
};

// 4 c^2 <= t2 L2 for |c| < 2^43, t2 <= 2^12, L2 < 2^43, without leaving int64: beyond 2^30 the left side is the larger
__device__ __forceinline__ bool within_band(int64_t c, int64_t t2, int64_t L2)
{
    const int64_t ac = c < 0 ? -c : c;
    return ac < (1ll << 30) && 4 * ac * ac <= t2 * L2;
}

// the limb rule of include/soar_hip.h; a = b is the disc of squared radius t2 / 4
__device__ __forceinline__ bool limb_covers(int px, int py, int ax, int ay, int bx, int by, int64_t t2)
{
    const int64_t dx = (int64_t)bx - ax, dy = (int64_t)by - ay, qx = (int64_t)px - ax, qy = (int64_t)py - ay;
    const int64_t L2 = dx * dx + dy * dy, s = qx * dx + qy * dy;
    if (s > 0 && s < L2) return within_band(qx * dy - qy * dx, t2, L2);
    const int64_t ex = s <= 0 ? qx : (int64_t)px - bx, ey = s <= 0 ? qy : (int64_t)py - by;
    return 4 * (ex * ex + ey * ey) <= t2;
}

// Primitive `idx` in drawing order: target limbs [0, L), target discs [L, L + K), fit limbs, fit discs.
struct Prim { int ax, ay, bx, by; uint32_t rgb; bool disc, drawn; };

__device__ __forceinline__ Prim primitive(const StripDev &a, const StripLds &s, int idx)
{
    const int half = a.L + a.K, set = idx >= half ? 1 : 0, q = idx - set * half;
    Prim p;
    if (q < a.L) {
        const int ia = s.la[q], ib = s.lb[q];
        p.ax = s.cx[set][ia]; p.ay = s.cy[set][ia]; p.bx = s.cx[set][ib]; p.by = s.cy[set][ib];
        p.rgb = s.lrgb[q];
        p.disc = false;
        p.drawn = p.ax != NOT_DRAWN && p.bx != NOT_DRAWN && !(p.rgb & LIMB_UNNAMED);
    } else {
        p.ax = p.bx = s.cx[set][q - a.L]; p.ay = p.by = s.cy[set][q - a.L];
        p.rgb = a.target_rgb ^ ((a.target_rgb ^ a.fit_rgb) & (0u - (uint32_t)set));      // (a select by mask: no table of two in scratch)
        p.disc = true;
        p.drawn = p.ax != NOT_DRAWN;
    }
    return p;
}

// whether the primitive can cover a pixel of [X0, X1] x [Y0, Y1]
__device__ __forceinline__ bool may_reach(const StripDev &a, const Prim &p, int X0, int X1, int Y0, int Y1)
{
    if (!p.drawn) return false;
    const int g = p.disc ? a.radius : (a.thickness + 1) / 2;
    const int lox = min(p.ax, p.bx) - g, hix = max(p.ax, p.bx) + g, loy = min(p.ay, p.by) - g, hiy = max(p.ay, p.by) + g;
    if (hix < X0 || lox > X1 || hiy < Y0 || loy > Y1) return false;
    if (p.disc || (p.ax == p.bx && p.ay == p.by)) return true;
    // a limb whose line passes the rectangle by more than half the thickness: the cross product is linear in the pixel, so its
    // smallest magnitude over the rectangle is at a corner when the four corners agree in sign
    const int64_t dx = (int64_t)p.bx - p.ax, dy = (int64_t)p.by - p.ay, L2 = dx * dx + dy * dy;
    int64_t lo = INT64_MAX, hi = INT64_MIN;
    for (int c = 0; c < 4; c++) {
        const int64_t qx = (int64_t)((c & 1) ? X1 : X0) - p.ax, qy = (int64_t)((c & 2) ? Y1 : Y0) - p.ay;
        const int64_t cr = qx * dy - qy * dx;
        lo = cr < lo ? cr : lo;
        hi = cr > hi ? cr : hi;
    }
    if (lo <= 0 && hi >= 0) return true;
    return within_band(lo > 0 ? lo : hi, (int64_t)a.thickness * a.thickness, L2);
}

__device__ __forceinline__ uint32_t blend_byte(uint32_t c, uint32_t img)
{
    const float v = rintf(0.6f * (float)c + 0.4f * (float)img);         // two products, one sum, half to even
    return (uint32_t)(int)fminf(fmaxf(v, 0.f), 255.f);
}

__device__ __forceinline__ uint32_t blend_rgb(const StripDev &a, uint32_t c, int n, int x, int y)
{
    const uint8_t *p = a.imgs + n * a.is_n + y * a.is_y + x * a.is_x;
    return blend_byte(c & 255u, p[0]) | blend_byte((c >> 8) & 255u, p[a.is_c]) << 8 | blend_byte((c >> 16) & 255u, p[2 * a.is_c]) << 16;
}

__device__ __forceinline__ uint32_t normal_byte(float v)
{
    const float s = (v * 0.5f + 0.5f) * 255.0f;
    return (uint32_t)(int)fminf(fmaxf(s, 0.f), 255.f);                  // truncated; NaN -> 0
}

// pixel (sx, sy) of the full strip, sx < 5 W, sy < H: r | g << 8 | b << 16
__device__ __forceinline__ uint32_t strip_pixel(const StripDev &a, const StripLds &s, int ns, int n, int sx, int sy)
{
    const int W = a.W;
    const int panel = (sx >= W) + (sx >= 2 * W) + (sx >= 3 * W) + (sx >= 4 * W), x = sx - panel * W;
    uint32_t c = 0;
    if (panel == 0) {
        const int64_t t2 = (int64_t)a.thickness * a.thickness;
        for (int i = ns - 1; i >= 0; i--) {                               // the last writer wins: the first hit from the end
            const Prim p = primitive(a, s, s.surv[i]);
            bool hit;
            if (p.disc) {
                const int dx = x - p.ax, dy = sy - p.ay;                  // (a survivor's centre is within the tile grown by the radius)
                hit = dx * dx + dy * dy <= a.r2p1;
            } else {
                hit = limb_covers(x, sy, p.ax, p.ay, p.bx, p.by, t2);
            }
            if (hit) { c = p.rgb; break; }
        }
    } else {
        const int k = panel < 2 ? 0 : panel - 2;
        const int64_t HW = (int64_t)a.H * W, body = (int64_t)n * 3 + k, at = (int64_t)sy * W + x;
        if (a.mask[body * 2 * HW + at]) {
            const float *pr = a.prior + body * 6 * HW + at;
            c = normal_byte(pr[0]) | normal_byte(pr[HW]) << 8 | normal_byte(pr[2 * HW]) << 16;
        }
        if (panel != 1) return c;
    }
    return a.has_img ? blend_rgb(a, c, n, x, sy) : c;
}

template <bool HALF>
__device__ __forceinline__ uint32_t out_pixel(const StripDev &a, const StripLds &s, int ns, int n, int ox, int oy)
{
    if constexpr (!HALF) {
        return strip_pixel(a, s, ns, n, ox, oy);
    } else {
        uint32_t sum[3] = {2u, 2u, 2u};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t c = strip_pixel(a, s, ns, n, 2 * ox + (j & 1), 2 * oy + (j >> 1));
            sum[0] += c & 255u; sum[1] += (c >> 8) & 255u; sum[2] += (c >> 16) & 255u;
        }
        return (sum[0] >> 2) | (sum[1] >> 2) << 8 | (sum[2] >> 2) << 16;
    }
}

// The grid: x = segment * tiles + tile (five panel-wide segments of a full strip, whose tiles start at the panel's column 0; one
// segment for a halved strip), y = rows of 16, z = frame.  A tile owns the aligned 4-byte words of the output whose first byte is one
// of its pixels'; the last of them may end in the pixel behind the tile (of the next tile, or of the next panel), which the tile
// computes as well.  Bytes are stored one by one only before the first word and behind the last word of an output row.
template <bool HALF>
__global__ void __launch_bounds__(STRIP_THREADS) strip_kernel(StripDev a, int tiles_per_seg, int seg_w)
{
    __shared__ StripLds s;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int n = blockIdx.z, seg = blockIdx.x / tiles_per_seg, x0 = (blockIdx.x - seg * tiles_per_seg) * TILE_W;
    const int ox0 = seg * seg_w + x0, oy0 = blockIdx.y * TILE_H;
    const int wt = min(TILE_W, seg_w - x0);                               // the tile's own columns
    // the part of panel 0 the tile's pixels (and the one behind them) are made of
    const int X0 = HALF ? 2 * ox0 : ox0, X1 = min(HALF ? 2 * (ox0 + TILE_W) + 1 : ox0 + TILE_W, a.W - 1);
    const int Y0 = HALF ? 2 * oy0 : oy0, Y1 = min(HALF ? 2 * oy0 + 2 * TILE_H - 1 : oy0 + TILE_H - 1, a.H - 1);
    int ns = 0;
    if (X0 < a.W) {                                                       // (uniform over the workgroup)
        for (int i = tid; i < 2 * a.K; i += STRIP_THREADS) {
            const int set = i >= a.K ? 1 : 0, k = i - set * a.K;
            const float *src = (set ? a.fit_px : a.target_px) + ((int64_t)n * a.K + k) * 2;
            const float x = src[0], y = src[1];
            bool ok = a.kp_mask[k] != 0 && fabsf(x) < (float)COORD_LIMIT && fabsf(y) < (float)COORD_LIMIT;   // (false for NaN)
            const int cx = ok ? (int)x : 0, cy = ok ? (int)y : 0;
            ok = ok && cx >= 1 && cy >= 1;
            s.cx[set][k] = ok ? cx : NOT_DRAWN;
            s.cy[set][k] = cy;
        }
        for (int i = tid; i < a.L; i += STRIP_THREADS) {
            const int ia = a.limbs[2 * i], ib = a.limbs[2 * i + 1];
            const bool named = (unsigned)ia < (unsigned)a.K && (unsigned)ib < (unsigned)a.K;      // (a limb of no keypoint draws nothing)
            s.la[i] = named ? ia : 0;
            s.lb[i] = named ? ib : 0;
            s.lrgb[i] = a.limb_rgb[3 * i] | a.limb_rgb[3 * i + 1] << 8 | a.limb_rgb[3 * i + 2] << 16 | (named ? 0u : LIMB_UNNAMED);
        }
        __syncthreads();
        // cull and compact in drawing order: a ballot and a prefix count per wavefront, the wavefronts' counts through LDS
        const int total = 2 * a.K + 2 * a.L;
        for (int base = 0, chunk = 0; base < total; base += STRIP_THREADS, chunk++) {
            const int idx = base + tid;
            const bool keep = idx < total && may_reach(a, primitive(a, s, idx), X0, X1, Y0, Y1);
            const unsigned long long m = __ballot(keep);
            if (lane == 0) s.wave_count[chunk & 1][wave] = __popcll(m);
            __syncthreads();
            int before = 0, all = 0;
            for (int w = 0; w < STRIP_THREADS / WAVE; w++) {
                const int c = s.wave_count[chunk & 1][w];
                before += w < wave ? c : 0;
                all += c;
            }
            if (keep) s.surv[ns + before + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = (uint16_t)idx;
            ns += all;
        }
        __syncthreads();
    }

    const int r = tid >> 4, i = tid & 15, oy = oy0 + r;
    const bool row_ok = oy < a.OH;
    auto pixel = [&](int j) -> uint32_t {                                   // (four copies, no array: nothing spills to scratch)
        const int ox = ox0 + 4 * i + j;
        return row_ok && ox < a.RW ? out_pixel<HALF>(a, s, ns, n, ox, oy) : 0u;
    };
    const uint32_t c0 = pixel(0), c1 = pixel(1), c2 = pixel(2), c3 = pixel(3);
    s.row[r][3 * i] = c0 | c1 << 24;                                      // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
    s.row[r][3 * i + 1] = c1 >> 8 | c2 << 16;
    s.row[r][3 * i + 2] = c2 >> 16 | c3 << 8;
    if (tid < TILE_H) {                                                   // the pixel behind the tile, one per row
        const int ox = ox0 + TILE_W, y = oy0 + tid;
        s.row[tid][48] = (ox < a.RW && y < a.OH) ? out_pixel<HALF>(a, s, ns, n, ox, y) : 0u;
        s.row[tid][49] = 0u;
    }
    __syncthreads();
    if (!row_ok) return;

    const int64_t at = (((int64_t)n * a.OH + oy) * a.RW + ox0) * 3;       // the tile's first byte of this row
    uint8_t *dst = a.out + at;
    const int h = (int)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3);   // bytes before the first aligned word
    const int own = 3 * wt, rem = 3 * (a.RW - ox0);                       // the tile's bytes; the bytes to the end of the row
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(s.row[r]);
    if (ox0 == 0 && i == 0)
        for (int b = 0; b < h; b++) dst[b] = bytes[b];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int m = 3 * i + j, first = h + 4 * m;
        if (first >= own) continue;
        if (first + 4 <= rem) {
            const uint64_t two = (uint64_t)s.row[r][m + 1] << 32 | s.row[r][m];
            *reinterpret_cast<uint32_t *>(dst + first) = (uint32_t)(two >> (8 * h));
        } else {
            for (int b = first; b < rem; b++) dst[b] = bytes[b];
        }
    }
}

// ---- residuals -----------------------------------------------------------------------------------------------------------------
struct ResidualDev {
    int32_t N, K;
    const float *fit_px, *target_px, *conf;
    const uint8_t *kp_mask;
    float thresh;
    float *out;
};

__global__ void __launch_bounds__(WAVE) residuals_kernel(ResidualDev a)
{
    const int n = blockIdx.x, lane = threadIdx.x;
    float sum = 0.f, mx = 0.f;
    int cnt = 0;
    for (int k = lane; k < a.K; k += WAVE) {
        const int64_t at = (int64_t)n * a.K + k;
        const float fx = a.fit_px[2 * at], fy = a.fit_px[2 * at + 1], tx = a.target_px[2 * at], ty = a.target_px[2 * at + 1];
        const bool ok = a.kp_mask[k] != 0 && a.conf[at] > a.thresh && isfinite(fx) && isfinite(fy) && isfinite(tx) && isfinite(ty);
        const float dx = fx - tx, dy = fy - ty;
        const float d = ok ? sqrtf(dx * dx + dy * dy) : 0.f;
        sum += d;
        mx = fmaxf(mx, d);
        cnt += ok ? 1 : 0;
    }
    for (int off = WAVE / 2; off >= 1; off >>= 1) {                       // a butterfly: every lane ends with the same sum
        sum += __shfl_xor(sum, off);
        mx = fmaxf(mx, __shfl_xor(mx, off));
        cnt += __shfl_xor(cnt, off);
    }
    if (lane == 0) {
        a.out[3 * n] = (float)cnt;
        a.out[3 * n + 1] = cnt ? sum / (float)cnt : 0.f;
        a.out[3 * n + 2] = cnt ? mx : 0.f;
    }
}

}  // namespace
}  // namespace soar

using namespace soar;

extern "C" {

int soar_fitviz_yaw_views(int32_t N, int32_t V, int32_t n_views, const float *verts, const int64_t *verts_stride, const float *pivot,
                          const float *R, float *out, void *stream_)
{
    const char *me = "soar_fitviz_yaw_views";
    if (N < 0 || V < 1 || n_views < 1 || n_views > MAX_VIEWS || (int64_t)N * V * n_views > (1ll << 30)) {
        set_error("%s: bad arguments (N=%d, V=%d, n_views=%d; need N >= 0, V >= 1, 1 <= n_views <= %d, N V n_views <= 2^30)", me, N, V,
                  n_views, MAX_VIEWS);
        return 1;
    }
    if (N == 0) return 0;
    if (!verts || !verts_stride || !pivot || !out || (n_views > 1 && !R)) {
        set_error("%s: NULL verts / verts_stride / pivot / R / out", me);
        return 1;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    YawDev d;
    d.N = N; d.V = V; d.n_views = n_views;
    d.verts = verts; d.pivot = pivot; d.R = R; d.out = out;
    d.sn = verts_stride[0]; d.sv = verts_stride[1]; d.sc = verts_stride[2];
    const unsigned blocks = (unsigned)(((int64_t)N * V + YAW_THREADS - 1) / YAW_THREADS);
    hipLaunchKernelGGL(yaw_views_kernel, dim3(blocks), dim3(YAW_THREADS), 0, stream, d);
    SOAR_LAUNCH_OK("fitviz_yaw_views", stream, 0);
    return 0;
}

int soar_fitviz_strip(const SoarFitvizStripArgs *args, void *stream_)
{
    const char *me = "soar_fitviz_strip";
    if (!args) { set_error("%s: NULL args", me); return 1; }
    const SoarFitvizStripArgs &a = *args;
    if (a.N < 0 || a.N > 65535 || a.H < 1 || a.W < 1 || a.H > 4096 || a.W > 4096 || a.K < 0 || a.L < 0) {
        set_error("%s: bad arguments (N=%d, H=%d, W=%d, K=%d, L=%d; need 0 <= N <= 65535, 1 <= H, W <= 4096, K, L >= 0)", me, a.N, a.H,
                  a.W, a.K, a.L);
        return 1;
    }
    if (a.K > MAX_K || a.L > MAX_L) {
        set_error("%s: K=%d keypoints and L=%d limbs; at most %d and %d are supported", me, a.K, a.L, MAX_K, MAX_L);
        return 1;
    }
    if (a.radius < 1 || a.radius > 8 || a.thickness < 1 || a.thickness > 64) {
        set_error("%s: radius=%d, thickness=%d; need 1 <= radius <= 8 and 1 <= thickness <= 64", me, a.radius, a.thickness);
        return 1;
    }
    if (a.half && (a.H < 2 || a.W < 1 || 5 * a.W < 2)) {
        set_error("%s: a halved strip needs H >= 2 (got H=%d, W=%d)", me, a.H, a.W);
        return 1;
    }
    if (a.N == 0) return 0;
    if (!a.prior || !a.mask || !a.out || (a.K > 0 && (!a.target_px || !a.fit_px || !a.kp_mask)) || (a.L > 0 && (!a.limbs || !a.limb_rgb))) {
        set_error("%s: NULL target_px / fit_px / kp_mask / limbs / limb_rgb / prior / mask / out (only imgs may be NULL)", me);
        return 1;
    }
    if (a.L > 0 && a.K == 0) { set_error("%s: limbs without keypoints", me); return 1; }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StripDev d;
    d.N = a.N; d.H = a.H; d.W = a.W; d.K = a.K; d.L = a.L;
    d.radius = a.radius; d.r2p1 = a.radius * a.radius + 1; d.thickness = a.thickness;
    d.has_img = a.imgs != nullptr;
    d.OH = a.half ? a.H / 2 : a.H;
    d.RW = a.half ? 5 * a.W / 2 : 5 * a.W;
    d.target_px = a.target_px; d.fit_px = a.fit_px; d.kp_mask = a.kp_mask; d.limbs = a.limbs; d.limb_rgb = a.limb_rgb;
    d.imgs = a.imgs;
    d.is_n = a.imgs_stride[0]; d.is_y = a.imgs_stride[1]; d.is_x = a.imgs_stride[2]; d.is_c = a.imgs_stride[3];
    d.prior = a.prior; d.mask = a.mask;
    d.target_rgb = a.target_rgb[0] | a.target_rgb[1] << 8 | a.target_rgb[2] << 16;
    d.fit_rgb = a.fit_rgb[0] | a.fit_rgb[1] << 8 | a.fit_rgb[2] << 16;
    d.out = a.out;
    const int seg_w = a.half ? d.RW : a.W, segs = a.half ? 1 : 5, tiles = (seg_w + TILE_W - 1) / TILE_W;
    const dim3 grid((unsigned)(segs * tiles), (unsigned)((d.OH + TILE_H - 1) / TILE_H), (unsigned)a.N);
    if (a.half)
        hipLaunchKernelGGL(strip_kernel<true>, grid, dim3(STRIP_THREADS), 0, stream, d, tiles, seg_w);
    else
        hipLaunchKernelGGL(strip_kernel<false>, grid, dim3(STRIP_THREADS), 0, stream, d, tiles, seg_w);
    SOAR_LAUNCH_OK("fitviz_strip", stream, 0);
    return 0;
}

int soar_fitviz_residuals(int32_t N, int32_t K, const float *fit_px, const float *target_px, const float *conf, const uint8_t *kp_mask,
                          float thresh, float *out, void *stream_)
{
    const char *me = "soar_fitviz_residuals";
    if (N < 0 || K < 0 || K > MAX_K || N > (1 << 24)) {
        set_error("%s: bad arguments (N=%d, K=%d; need 0 <= N <= 2^24, 0 <= K <= %d)", me, N, K, MAX_K);
        return 1;
    }
    if (N == 0) return 0;
    if (!out || (K > 0 && (!fit_px || !target_px || !conf || !kp_mask))) {
        set_error("%s: NULL fit_px / target_px / conf / kp_mask / out", me);
        return 1;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ResidualDev d;
    d.N = N; d.K = K; d.fit_px = fit_px; d.target_px = target_px; d.conf = conf; d.kp_mask = kp_mask; d.thresh = thresh; d.out = out;
    hipLaunchKernelGGL(residuals_kernel, dim3((unsigned)N), dim3(WAVE), 0, stream, d);
    SOAR_LAUNCH_OK("fitviz_residuals", stream, 0);
    return 0;
}

}  // extern "C"
