// pose_parts.hip -- hand and face keypoint detection of the preprocessing stage (soar_amd/pose_parts.py): the convolutional pose
// machine both networks are, the rectangles derived from the body keypoints, the crops and the maps' maxima, as include/soar_hip.h and
// DESIGN.md 9zb state them.  Forward only, float32.
//
//   (pose_common.h         the packer, the ingest, the 2 x 2 pool and the slice kernels, shared with pose.hip, and the bicubic rule)
//   (conv_gemm_kernel      conv_gemm.hip: every convolution.  1 x 1 and 3 x 3 in one launch with the ReLU in the epilogue; 7 x 7 as seven
//                          launches of seven taps, one per kernel row: the first with the bias, the later ones with res == y, which the
//                          epilogue reads and writes at the same index from the same thread, all with act = 0 because the epilogue
//                          applies the activation before it adds res)
//   cpm_relu_kernel        the ReLU of a 7 x 7 layer, in place behind its seventh launch
//   part_boxes_kernel      one thread per rectangle: left hand, right hand, face of a person
//   part_crop_kernel       one thread per crop pixel of both networks' inputs: bilinear, zeros outside, the left hand mirrored
//   part_keypoints_kernel  one workgroup per (crop, map): the source map in LDS, the x8 bicubic values on the fly, their maximum
//
// Compiled with -ffp-contract=off: the float32 expressions of the three part kernels evaluate as written (tests/pose_parts_ref.py
// restates them in NumPy, bit for bit).  No float atomics, no host synchronisation, no allocation; a crop's result does not depend on
// its batch.
#include "net_weights.h"
#include "pose_common.h"
#include "workspace.h"

namespace soar {

namespace {

constexpr int FRONT = SOAR_CPM_FRONT, MAX_LAYERS = SOAR_CPM_MAX_LAYERS;
constexpr int MAX_WIDTH = 4096;
constexpr int64_t MAX_PIX = int64_t(1) << 30;
constexpr int KP_THREADS = 1024, KP_MAX_CELLS = 12288;      // the source map in LDS: 48 KB

inline int pad8(int v) { return (v + 7) / 8 * 8; }
// layer i gives a stage's maps
inline bool is_maps(int i) { return i == FRONT + 1 || (i > FRONT + 1 && (i - FRONT - 2) % 7 == 6); }
// ... or reads (maps, features): a later stage's first
inline bool reads_row(int i) { return i > FRONT + 1 && (i - FRONT - 2) % 7 == 0; }

bool check_cfg(const char *me, const SoarCpmConfig *c)
{
    if (!c) { set_error("%s: NULL config", me); return false; }
    if (c->n_stages < 1 || c->n_stages > SOAR_CPM_MAX_STAGES || c->n_layers != 17 + 7 * (c->n_stages - 1)) {
        set_error("%s: need 1 .. %d stages and 17 + 7 (n_stages - 1) layers (n_stages=%d, n_layers=%d)", me, SOAR_CPM_MAX_STAGES, c->n_stages,
                  c->n_layers);
        return false;
    }
    if (c->n_maps < 2 || c->n_maps > MAX_WIDTH) {
        set_error("%s: n_maps must be 2 .. %d, the background among them (got %d)", me, MAX_WIDTH, c->n_maps);
        return false;
    }
    if (__builtin_popcount((unsigned)c->pool_mask) != 3 || (c->pool_mask >> (FRONT - 1))) {
        set_error("%s: pool_mask must hold three bits below %d: the maps are at 1/8 resolution (got %#x)", me, FRONT - 1, c->pool_mask);
        return false;
    }
    for (int i = 0; i < c->n_layers; i++) {
        const int w = c->width[i], s = c->side[i];
        if (is_maps(i) ? w != c->n_maps : (w < 8 || w % 8 || w > MAX_WIDTH)) {
            set_error("%s: layer %d: a width must be a multiple of 8 in 8 .. %d, the maps' n_maps = %d (got %d)", me, i, MAX_WIDTH, c->n_maps, w);
            return false;
        }
        if (s != 1 && s != 3 && s != 7) { set_error("%s: layer %d: a kernel side must be 1, 3 or 7 (got %d)", me, i, s); return false; }
    }
    return true;
}
bool check_size(const char *me, int32_t M, int32_t S)
{
    if (M < 0 || S < 8 || S % 8 || (int64_t)(M > 0 ? M : 1) * S * S > MAX_PIX) {
        set_error("%s: need M >= 0, S a multiple of 8, at least 8, and M S S <= 2^30 (M=%d, S=%d)", me, M, S);
        return false;
    }
    return true;
}

// ---- the layers, in the order of soar_amd.pose_parts.layer_keys ----
struct Layer {
    int cin, cout, side, cinp, coutp, nseg;
    Seg seg[2];
    int iw, ib;                                 // the plan's entries: weight, bias
};
struct Net {
    Layer L[MAX_LAYERS];
    int n, feat, mapsp;
    WeightPlan plan;
};
inline int stage_row(const Net &net) { return net.mapsp + net.feat; }      // [maps, padded | features]
Net build_net(const SoarCpmConfig &c)
{
    Net net;
    net.n = c.n_layers; net.feat = c.width[FRONT - 1]; net.mapsp = pad8(c.n_maps);
    const int F = net.feat, NM = c.n_maps, MP = net.mapsp;
    for (int i = 0; i < c.n_layers; i++) {
        Layer &l = net.L[i];
        l = Layer{};
        l.cout = c.width[i]; l.side = c.side[i]; l.coutp = pad8(l.cout);
        if (i == 0) { l.cin = 3; l.cinp = IMGP; l.seg[l.nseg++] = Seg{0, 0, 3}; }
        else if (reads_row(i)) {
            // the stage's input, as the weights order it -> as the row holds it
            l.cin = NM + F; l.cinp = MP + F;
            l.seg[l.nseg++] = c.maps_first ? Seg{0, 0, NM} : Seg{0, F, NM};
            l.seg[l.nseg++] = c.maps_first ? Seg{MP, NM, F} : Seg{MP, 0, F};
        } else {
            l.cin = i == FRONT ? F : c.width[i - 1]; l.cinp = l.cin;
            l.seg[l.nseg++] = Seg{0, 0, l.cin};
        }
        const size_t kk = (size_t)l.side * l.side;
        l.iw = net.plan.add((size_t)l.cout * l.cin * kk, (size_t)l.coutp * kk * l.cinp);
        l.ib = net.plan.add((size_t)l.cout, (size_t)l.coutp);
    }
    return net;
}

// ---- the workspace: floats ----
struct WsLayout {
    size_t in8, act[2], X, Y[2], total;
};
WsLayout ws_layout(const SoarCpmConfig &c, const Net &net, int M, int S)
{
    WsLayout L{};
    Carver ws;
    size_t pix = (size_t)M * S * S, act = 0;
    for (int i = 0; i < FRONT - 1; i++) {        // (the last front layer writes the features into the stage row)
        const size_t v = pix * net.L[i].coutp;
        act = v > act ? v : act;
        if ((c.pool_mask >> i) & 1) pix /= 4;
    }
    const size_t R = pix;
    size_t wide = 8;
    for (int i = FRONT; i < net.n; i++)
        if (!is_maps(i) && (size_t)net.L[i].coutp > wide) wide = net.L[i].coutp;
    L.in8 = ws.offset<float>((size_t)M * S * S * IMGP);
    for (int i = 0; i < 2; i++) L.act[i] = ws.offset<float>(act);
    L.X = ws.offset<float>(R * stage_row(net));
    for (int i = 0; i < 2; i++) L.Y[i] = ws.offset<float>(R * wide);
    L.total = ws.bytes() == 0 ? ALIGN : ws.bytes();
    return L;
}

// channels 0 .. C of rows ld apart, in place; thread = (row, channel quad)
__global__ void __launch_bounds__(256) cpm_relu_kernel(float *y, int64_t ld, int C, int64_t n4)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n4) return;
    const int c4 = C / 4;
    float4 *p = reinterpret_cast<float4 *>(y + (e / c4) * ld) + (int)(e % c4);
    float4 v = *p;
    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    *p = v;
}

// One convolution of side 1, 3 or 7 with zero padding: x's channels [0, Cin) of rows ldx apart -> y's [0, Cout) of rows ldy apart.
// w: [Cout][side side][Cin].  y must not overlap x.
int conv_layer(const float *x, int64_t ldx, float *y, int64_t ldy, int N, int H, int W, int Cin, int Cout, int side, const float *w,
               const float *bias, bool relu, hipStream_t stream)
{
    ConvGemm k{};
    k.x = x; k.ldx = ldx; k.xim = (int64_t)H * W;
    k.y = y; k.ldy = ldy; k.yim = (int64_t)H * W; k.Wout = W; k.os = 1;
    k.alpha = 1.f; k.bias = bias;
    k.N = N; k.Hg = H; k.Wg = W; k.Hin = H; k.Win = W; k.Cin = Cin; k.Cout = Cout;
    k.stride = 1; k.dil = 1; k.nph = 1;
    if (side <= 3) {
        k.act = relu ? ACT_RELU : ACT_NONE;
        square_taps(k.ph[0], w, (int64_t)side * side * Cin, side, -(side / 2));
        return launch_conv_gemm(k, stream);
    }
    // a kernel row per launch: the shared GEMM takes at most 9 taps.  The tile, and with it who computes which output, is the same
    // for all seven (conv_gemm_tile reads the rows, Cout and nph only)
    k.act = ACT_NONE;
    ConvTaps &t = k.ph[0];
    t.ldw = (int64_t)side * side * Cin; t.ntaps = side; t.py = t.px = 0;
    for (int r = 0; r < side; r++) {
        t.w = w + (size_t)r * side * Cin;
        for (int j = 0; j < side; j++) { t.dy[j] = (signed char)(r - side / 2); t.dx[j] = (signed char)(j - side / 2); }
        if (r == 1) { k.bias = nullptr; k.res = y; }
        if (launch_conv_gemm(k, stream)) return 1;
    }
    if (relu) {
        const int64_t n4 = (int64_t)N * H * W * (Cout / 4);
        hipLaunchKernelGGL(cpm_relu_kernel, dim3(blocks(n4)), dim3(256), 0, stream, y, ldy, Cout, n4);
        SOAR_LAUNCH_OK("cpm_relu", stream, 0);
    }
    return 0;
}

// ---- the rectangles ----
__device__ __forceinline__ float dist2(float ax, float ay, float bx, float by)
{
    const float dx = ax - bx, dy = ay - by;
    return sqrtf(dx * dx + dy * dy);
}
__global__ void __launch_bounds__(256) part_boxes_kernel(SoarPartBoxArgs k)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= k.B * k.part_people * 3) return;
    const int which = e % 3, q = (e / 3) % k.part_people, b = e / (3 * k.part_people);
    float x0 = 0.f, y0 = 0.f, side = 0.f;
    bool valid = false;
    if (q < min(k.n_people[b], k.max_people)) {
        const float *J = k.people + ((size_t)b * k.max_people + q) * SOAR_POSE_PARTS * 3;
        if (which < 2) {
            const float *sh = J + 3 * (which == 0 ? 5 : 2), *el = sh + 3, *wr = sh + 6;
            const float cx = wr[0] + 0.33f * (wr[0] - el[0]), cy = wr[1] + 0.33f * (wr[1] - el[1]);
            side = 1.5f * fmaxf(dist2(wr[0], wr[1], el[0], el[1]), 0.9f * dist2(el[0], el[1], sh[0], sh[1]));
            x0 = cx - side / 2.f;
            y0 = cy - side / 2.f;
            valid = sh[2] > k.hand_min_conf && el[2] > k.hand_min_conf && wr[2] > k.hand_min_conf && side > 1.f && side * side > k.min_hand_area;
        } else {
            const float *neck = J + 3, *nose = J, *rEye = J + 45, *lEye = J + 48, *rEar = J + 51, *lEar = J + 54;
            const float t = k.face_min_conf;
            const bool hNeck = neck[2] > t, hNose = nose[2] > t, hREye = rEye[2] > t, hLEye = lEye[2] > t, hREar = rEar[2] > t, hLEar = lEar[2] > t;
            float cx = 0.f, cy = 0.f, size = 0.f;
            int count = 0;
            if (hNeck && hNose) {
                const float nn = dist2(neck[0], neck[1], nose[0], nose[1]);
                if (hLEye == hLEar && hREye == hREar && hLEye != hREye) {
                    const float *eye = hLEye ? lEye : rEye, *ear = hLEye ? lEar : rEar;
                    cx = cx + ((eye[0] + ear[0]) + nose[0]) / 3.f;
                    cy = cy + ((eye[1] + ear[1]) + nose[1]) / 3.f;
                    size = size + 0.85f * ((dist2(nose[0], nose[1], eye[0], eye[1]) + dist2(nose[0], nose[1], ear[0], ear[1])) + nn);
                } else {
                    cx = cx + (neck[0] + nose[0]) / 2.f;
                    cy = cy + (neck[1] + nose[1]) / 2.f;
                    size = size + 2.f * nn;
                }
                count++;
            }
            if (hLEye && hREye) {
                cx = cx + (lEye[0] + rEye[0]) / 2.f;
                cy = cy + (lEye[1] + rEye[1]) / 2.f;
                size = size + 3.f * dist2(lEye[0], lEye[1], rEye[0], rEye[1]);
                count++;
            }
            if (hLEar && hREar) {
                cx = cx + (lEar[0] + rEar[0]) / 2.f;
                cy = cy + (lEar[1] + rEar[1]) / 2.f;
                size = size + 2.f * dist2(lEar[0], lEar[1], rEar[0], rEar[1]);
                count++;
            }
            if (count > 0) {
                cx = cx / (float)count; cy = cy / (float)count; size = size / (float)count;
                x0 = cx - size / 2.f;
                y0 = cy - size / 2.f;
                side = size;
            }
            valid = count > 0 && side * side > k.min_face_area;
        }
    }
    reinterpret_cast<float4 *>(k.boxes)[e] = valid ? make_float4(x0, y0, side, 1.f) : make_float4(0.f, 0.f, 0.f, 0.f);
}


// ---- the crops ----
struct CropK {
    const uint8_t *img;
    const float *boxes;
    float *hands, *faces;
    int H, W, S, P;
    int64_t n;                                  // B P 3 S S
};
__global__ void __launch_bounds__(256) part_crop_kernel(CropK k)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= k.n) return;
    const int S = k.S, u = (int)(e % S), v = (int)((e / S) % S);
    const int64_t j = e / ((int64_t)S * S);     // the rectangle: (frame, person, which)
    const int which = (int)(j % 3);
    const int64_t bp = j / 3;
    float *dst = which < 2 ? k.hands : k.faces;
    if (!dst) return;
    dst += ((which < 2 ? bp * 2 + which : bp) * 3 * S + v) * (int64_t)S + u;
    const float4 box = reinterpret_cast<const float4 *>(k.boxes)[j];
    float val[3] = {0.f, 0.f, 0.f};
    if (box.w != 0.f) {
        const float s = box.z / (float)S;
        const float x = box.x + (float)(which == 0 ? S - 1 - u : u) * s, y = box.y + (float)v * s;
        if (x > -1.f && x < (float)k.W && y > -1.f && y < (float)k.H) {
            const float fx = floorf(x), fy = floorf(y), ax = x - fx, ay = y - fy;
            const int ix = (int)fx, iy = (int)fy;               // -1 .. W - 1, -1 .. H - 1
            const bool l = ix >= 0, r = ix + 1 < k.W, t = iy >= 0, d = iy + 1 < k.H;
            const uint8_t *im = k.img + (size_t)(bp / k.P) * k.H * k.W * 3;
            const int64_t o00 = ((int64_t)iy * k.W + ix) * 3, o01 = o00 + 3, o10 = o00 + (int64_t)k.W * 3, o11 = o10 + 3;
#pragma unroll
            for (int c = 0; c < 3; c++) {       // BGR from RGB
                const float p00 = t && l ? (float)im[o00 + 2 - c] : 0.f, p01 = t && r ? (float)im[o01 + 2 - c] : 0.f;
                const float p10 = d && l ? (float)im[o10 + 2 - c] : 0.f, p11 = d && r ? (float)im[o11 + 2 - c] : 0.f;
                val[c] = (p00 * (1.f - ax) + p01 * ax) * (1.f - ay) + (p10 * (1.f - ax) + p11 * ax) * ay;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) dst[(int64_t)c * S * S] = val[c] / 256.f - 0.5f;
}

// ---- the maxima ----
struct KeypointsK {
    const float *heat, *boxes;
    float *out;
    int h, w, n_maps, which;
};
__global__ void __launch_bounds__(KP_THREADS) part_keypoints_kernel(KeypointsK k)
{
    extern __shared__ __attribute__((aligned(16))) float kp_lds[];
    __shared__ float best_v[KP_THREADS / 64];
    __shared__ int best_i[KP_THREADS / 64];
    const int tid = threadIdx.x, map = blockIdx.x, m = blockIdx.y;
    float *wt = kp_lds, *src = kp_lds + 32;                     // [8][4], [h][w]
    if (tid < 8) up_weights(tid, wt + 4 * tid);
    const float *heat = k.heat + (size_t)m * k.h * k.w * k.n_maps + map;
    for (int e = tid; e < k.h * k.w; e += KP_THREADS) src[e] = heat[(size_t)e * k.n_maps];
    __syncthreads();
    const int HH = 8 * k.h, WW = 8 * k.w;
    float best = -INFINITY;
    int at = 0x7fffffff;
    for (int e = tid; e < HH * WW; e += KP_THREADS) {           // (e ascends: a tie keeps the first)
        const int Y = e / WW, X = e - Y * WW;
        const int iy = up_cell(Y), ix = up_cell(X);
        const float *wy = wt + 4 * up_phase(Y), *wx = wt + 4 * up_phase(X);
        const int x0 = min(max(ix - 1, 0), k.w - 1), x1 = min(max(ix, 0), k.w - 1), x2 = min(max(ix + 1, 0), k.w - 1),
                  x3 = min(max(ix + 2, 0), k.w - 1);
        float row[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float *s = src + (size_t)min(max(iy - 1 + j, 0), k.h - 1) * k.w;
            row[j] = up_sum4(wx, s[x0], s[x1], s[x2], s[x3]);
        }
        const float v = up_sum4(wy, row[0], row[1], row[2], row[3]);
        if (v > best) { best = v; at = e; }
    }
#pragma unroll
    for (int lane = 32; lane >= 1; lane >>= 1) {
        const float ob = __shfl_xor(best, lane);
        const int oa = __shfl_xor(at, lane);
        if (ob > best || (ob == best && oa < at)) { best = ob; at = oa; }
    }
    if ((tid & 63) == 0) { best_v[tid >> 6] = best; best_i[tid >> 6] = at; }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < KP_THREADS / 64; i++)
            if (best_v[i] > best || (best_v[i] == best && best_i[i] < at)) { best = best_v[i]; at = best_i[i]; }
        const int hand = k.which == 0 ? m & 1 : 2;
        const float4 box = reinterpret_cast<const float4 *>(k.boxes)[(size_t)(k.which == 0 ? m >> 1 : m) * 3 + hand];
        float *o = k.out + ((size_t)m * (k.n_maps - 1) + map) * 3;
        if (best > 0.f && box.w != 0.f) {
            const int Y = at / WW, X = at - Y * WW;
            const float s = box.z / (float)WW;
            o[0] = box.x + (float)(hand == 0 ? WW - 1 - X : X) * s;
            o[1] = box.y + (float)Y * s;
            o[2] = best;
        } else {
            o[0] = o[1] = o[2] = 0.f;
        }
    }
}

}  // namespace
}  // namespace soar

using namespace soar;

extern "C" int soar_cpm_weights_size(const SoarCpmConfig *cfg, size_t *bytes, int32_t *count)
{
    const char *me = "soar_cpm_weights_size";
    if (!bytes) { set_error("%s: NULL bytes", me); return 1; }
    if (!check_cfg(me, cfg)) return 1;
    const Net net = build_net(*cfg);
    *bytes = align_up(net.plan.total * sizeof(float));
    if (count) *count = net.plan.count();
    return 0;
}

extern "C" int soar_cpm_workspace_size(const SoarCpmConfig *cfg, int32_t M, int32_t S, size_t *bytes)
{
    const char *me = "soar_cpm_workspace_size";
    if (!bytes) { set_error("%s: NULL bytes", me); return 1; }
    if (!check_cfg(me, cfg) || !check_size(me, M, S)) return 1;
    *bytes = ws_layout(*cfg, build_net(*cfg), M, S).total;
    return 0;
}

extern "C" int soar_cpm_pack_weights(const SoarCpmConfig *cfg, const float *const *tensors, const int64_t *sizes, int32_t count, void *packed,
                                     size_t packed_bytes, void *stream_)
{
    const char *me = "soar_cpm_pack_weights";
    if (!check_cfg(me, cfg)) return 1;
    if (!sizes) { set_error("%s: NULL sizes", me); return 1; }
    const Net net = build_net(*cfg);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    // entry 2 l is layer l's weight, entry 2 l + 1 its bias
    return pack_weights(net.plan, tensors, sizes, count, packed, packed_bytes, stream, me, [&](int i, const float *src, float *dst) {
        const Layer &l = net.L[i / 2];
        if (i % 2 == 0) {
            PackK k{};
            k.w = src; k.out = dst; k.cin = l.cin; k.cout = l.cout; k.kk = l.side * l.side; k.cinp = l.cinp; k.nseg = l.nseg;
            for (int s = 0; s < l.nseg; s++) k.seg[s] = l.seg[s];
            k.n = (int64_t)l.coutp * k.kk * l.cinp;
            hipLaunchKernelGGL(pose_pack_kernel, dim3(blocks(k.n)), dim3(256), 0, stream, k);
            SOAR_LAUNCH_OK("cpm_pack", stream, 0);
            return 0;
        }
        if (l.coutp == l.cout) return PACK_COPY;
        hipLaunchKernelGGL(pose_pad_kernel, dim3(blocks(l.coutp)), dim3(256), 0, stream, src, dst, l.cout, l.coutp);
        SOAR_LAUNCH_OK("cpm_pad", stream, 0);
        return 0;
    });
}

extern "C" int soar_cpm_forward(const SoarCpmConfig *cfg, const void *packed, const SoarCpmArgs *a, void *workspace, size_t workspace_bytes,
                                void *stream_)
{
    const char *me = "soar_cpm_forward";
    if (!check_cfg(me, cfg)) return 1;
    if (!a) { set_error("%s: NULL args", me); return 1; }
    if (!check_size(me, a->M, a->S)) return 1;
    if (a->M == 0) return 0;
    const SoarCpmConfig &c = *cfg;
    if (!packed || ((uintptr_t)packed & (ALIGN - 1)) || !a->x || !a->stage_out[c.n_stages - 1]) {
        set_error("%s: need the packed weights (256-byte aligned), x and the last stage's output", me);
        return 1;
    }
    const Net net = build_net(c);
    const WsLayout WL = ws_layout(c, net, a->M, a->S);
    if (!workspace_ok(me, workspace, workspace_bytes, WL.total, "soar_cpm_workspace_size")) return 1;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const float *P = static_cast<const float *>(packed);
    char *ws = static_cast<char *>(workspace);
    auto at = [&](size_t off) { return reinterpret_cast<float *>(ws + off); };
    float *in8 = at(WL.in8), *act[2] = {at(WL.act[0]), at(WL.act[1])}, *X = at(WL.X), *Y[2] = {at(WL.Y[0]), at(WL.Y[1])};
    const int M = a->M;
    int H = a->S, W = a->S;
    const int64_t npix = (int64_t)M * H * W;
    const int xrow = stage_row(net), F = net.feat, MP = net.mapsp;

    IngestK ik{};
    ik.x = a->x; ik.y = in8; ik.npix = npix; ik.H = H; ik.W = W;
    for (int j = 0; j < 4; j++) ik.xs[j] = a->x_stride[j];
    hipLaunchKernelGGL(pose_ingest_kernel, dim3(blocks(npix)), dim3(256), 0, stream, ik);
    SOAR_LAUNCH_OK("cpm_ingest", stream, 0);

    // one layer: x's channels [0, cinp) of rows ldx apart -> y's [0, coutp) of rows ldy apart (the columns behind cout: zero weights
    // and zero bias, so zeros)
    auto conv = [&](int li, const float *x, int64_t ldx, float *y, int64_t ldy) {
        const Layer &l = net.L[li];
        return conv_layer(x, ldx, y, ldy, M, H, W, l.cinp, l.coutp, l.side, P + net.plan.off[l.iw], P + net.plan.off[l.ib], !is_maps(li), stream);
    };
    // the front: the pools where the mask puts them, the last layer's output (the features) into the stage row
    const float *cur = in8;
    int cur_c = IMGP, side = 0;
    for (int li = 0; li < FRONT; li++) {
        const bool last = li == FRONT - 1;
        if (conv(li, cur, cur_c, last ? X + MP : act[side], last ? xrow : net.L[li].coutp)) return 1;
        cur = act[side]; cur_c = net.L[li].coutp; side ^= 1;
        if ((c.pool_mask >> li) & 1) {
            const int64_t n4 = (int64_t)M * (H / 2) * (W / 2) * (cur_c / 4);
            hipLaunchKernelGGL(pose_pool_kernel, dim3(blocks(n4)), dim3(256), 0, stream, cur, act[side], n4, H, W, cur_c);
            SOAR_LAUNCH_OK("cpm_pool", stream, 0);
            cur = act[side]; side ^= 1; H /= 2; W /= 2;
        }
    }
    const int64_t rows = (int64_t)M * H * W;
    auto slice = [&](int off, int C, float *dst) {
        if (!dst) return 0;
        hipLaunchKernelGGL(pose_slice_kernel, dim3(blocks(rows * C)), dim3(256), 0, stream, X, (int64_t)xrow, off, C, dst, rows * C);
        SOAR_LAUNCH_OK("cpm_slice", stream, 0);
        return 0;
    };
    if (slice(MP, F, a->features)) return 1;
    int li = FRONT;
    for (int s = 0; s < c.n_stages; s++) {
        // stage 1 reads the features, a later one the whole row; the layers ping-pong, the last writes the maps and their zero pad
        // channels into their segment of the row
        const int n = s == 0 ? 2 : 7;
        const float *x = s == 0 ? X + MP : X;
        int64_t ldx = xrow;
        for (int j = 0; j < n; j++, li++) {
            const bool last = j == n - 1;
            float *y = last ? X : Y[j & 1];
            const int64_t ldy = last ? xrow : net.L[li].coutp;
            if (conv(li, x, ldx, y, ldy)) return 1;
            x = y; ldx = ldy;
        }
        if (slice(0, c.n_maps, a->stage_out[s])) return 1;
    }
    return 0;
}

extern "C" int soar_part_boxes(const SoarPartBoxArgs *a, void *stream_)
{
    const char *me = "soar_part_boxes";
    if (!a) { set_error("%s: NULL args", me); return 1; }
    if (a->B < 0 || a->max_people < 1 || a->part_people < 1 || (int64_t)a->B * a->part_people > (1 << 24) ||
        (int64_t)(a->B > 0 ? a->B : 1) * a->max_people > (1 << 24)) {
        set_error("%s: need B >= 0, max_people, part_people >= 1 and B max_people, B part_people <= 2^24 (B=%d, max_people=%d, part_people=%d)", me,
                  a->B, a->max_people, a->part_people);
        return 1;
    }
    if (a->B == 0) return 0;
    if (!a->people || !a->n_people || !a->boxes || ((uintptr_t)a->boxes & 15)) {
        set_error("%s: NULL people / n_people / boxes, or boxes off 16 bytes", me);
        return 1;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(part_boxes_kernel, dim3(blocks((int64_t)a->B * a->part_people * 3)), dim3(256), 0, stream, *a);
    SOAR_LAUNCH_OK("part_boxes", stream, 0);
    return 0;
}

extern "C" int soar_part_crop(int32_t B, int32_t H, int32_t W, int32_t P, int32_t S, const uint8_t *images, const float *boxes, float *hands,
                              float *faces, void *stream_)
{
    const char *me = "soar_part_crop";
    if (B < 0 || H < 1 || W < 1 || P < 1 || S < 1 || (int64_t)(B > 0 ? B : 1) * H * W > MAX_PIX || (int64_t)(B > 0 ? B : 1) * P * 3 * S * S > MAX_PIX) {
        set_error("%s: need B >= 0, H, W, P, S >= 1, B H W <= 2^30 and 3 B P S S <= 2^30 (B=%d, H=%d, W=%d, P=%d, S=%d)", me, B, H, W, P, S);
        return 1;
    }
    if (B == 0) return 0;
    if (!images || !boxes || ((uintptr_t)boxes & 15) || (!hands && !faces)) {
        set_error("%s: NULL images / boxes, boxes off 16 bytes, or neither hands nor faces", me);
        return 1;
    }
    CropK k{};
    k.img = images; k.boxes = boxes; k.hands = hands; k.faces = faces; k.H = H; k.W = W; k.S = S; k.P = P;
    k.n = (int64_t)B * P * 3 * S * S;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(part_crop_kernel, dim3(blocks(k.n)), dim3(256), 0, stream, k);
    SOAR_LAUNCH_OK("part_crop", stream, 0);
    return 0;
}

extern "C" int soar_part_keypoints(int32_t M, int32_t h, int32_t w, int32_t n_maps, const float *heat, const float *boxes, int32_t which,
                                   float *out, void *stream_)
{
    const char *me = "soar_part_keypoints";
    if (M < 0 || M > 65535 || h < 1 || h != w || (int64_t)h * w > KP_MAX_CELLS || n_maps < 2 || n_maps > MAX_WIDTH || (which != 0 && which != 1) ||
        (which == 0 && M % 2)) {
        set_error("%s: need M in 0 .. 65535 (even for hands), h == w with h w <= %d, n_maps in 2 .. %d and which 0 (hands) or 1 (face) "
                  "(M=%d, h=%d, w=%d, n_maps=%d, which=%d)", me, KP_MAX_CELLS, MAX_WIDTH, M, h, w, n_maps, which);
        return 1;
    }
    if (M == 0) return 0;
    if (!heat || !boxes || !out || ((uintptr_t)boxes & 15)) { set_error("%s: NULL heat / boxes / out, or boxes off 16 bytes", me); return 1; }
    KeypointsK k{};
    k.heat = heat; k.boxes = boxes; k.out = out; k.h = h; k.w = w; k.n_maps = n_maps; k.which = which;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(part_keypoints_kernel, dim3((unsigned)(n_maps - 1), (unsigned)M), dim3(KP_THREADS), (32 + (size_t)h * w) * sizeof(float),
                       stream, k);
    SOAR_LAUNCH_OK("part_keypoints", stream, 0);
    return 0;
}
