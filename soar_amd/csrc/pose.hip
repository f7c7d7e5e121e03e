// pose.hip -- body keypoint detection of the preprocessing stage (soar_amd/pose.py): the BODY_25 network and the part-affinity
// post-processing, as include/soar_hip.h and DESIGN.md 9za state them.  Forward only, float32.
//
//   (pose_common.h, shared with pose_parts.hip: pose_pack_kernel, pose_pad_kernel, pose_ingest_kernel, pose_pool_kernel,
//                          pose_slice_kernel and the bicubic rule of the peaks, up_cell / up_phase / up_weights / up_sum4)
//   pose_pack_kernel       torch [Cout][Cin][kk] -> [Coutp][tap][Cinp]: up to three runs of input channels moved to where the padded
//                          activation row holds them, every other column and the rows behind Cout zeros
//   pose_preprocess_kernel uint8 RGB -> float32 BGR, v / 256 - 0.5
//   pose_ingest_kernel     the caller's strided [B][3][H][W] -> NHWC rows of 8 floats (3 values, 5 zeros)
//   (conv_gemm_kernel      conv_gemm.hip: every convolution, 3 x 3 and 1 x 1, with ReLU (act) or PReLU (slope) in its epilogue.  A layer
//                          reads a channel slice of its input's rows (ldx) and writes its slice of the buffer the next one reads (ldy):
//                          no concatenation is ever copied)
//   pose_pool_kernel       2 x 2 max pool, stride 2, NHWC
//   pose_slice_kernel      a channel slice of the rows -> a dense tensor (the stages' maps and the features, for the caller)
//   pose_peaks_kernel      one workgroup per (frame, part): the heat map upsampled by 8 (bicubic) strip by strip in LDS, strict 3 x 3
//                          maxima above the threshold as one ballot word per 64 pixels, read out in raster order, refined over 7 x 7
//   pose_assemble_kernel   one workgroup per frame, state in LDS: per limb the candidates' line integrals in parallel, the greedy choice
//                          by one wavefront, the persons' bookkeeping by one thread
//   pose_scale_kernel      net-input pixels -> image pixels
//
// Compiled with -ffp-contract=off: the post-processing's float32 expressions evaluate as written (tests/pose_ref.py restates them in
// NumPy, bit for bit).  No float atomics, no host synchronisation, no allocation; a frame's result does not depend on its batch.
#include "net_weights.h"
#include "pose_common.h"
#include "workspace.h"

namespace soar {

namespace {

constexpr int PAF = SOAR_POSE_PAF, HEAT = SOAR_POSE_HEAT, NPARTS = SOAR_POSE_PARTS, NPAIRS = SOAR_POSE_PAIRS;
constexpr int PAFP = 56, HEATP = 32;            // the maps' segments of a stage-input row, padded to multiples of 8
constexpr int MAXP = SOAR_POSE_MAX_PEAKS, MAX_PEOPLE = SOAR_POSE_MAX_PEOPLE;
constexpr int MAX_WIDTH = 4096;
constexpr int64_t MAX_PIX = int64_t(1) << 30;

bool check_cfg(const char *me, const SoarPoseConfig *c)
{
    if (!c) { set_error("%s: NULL config", me); return false; }
    const int v[10] = {c->c1, c->c2, c->c3, c->c4, c->cpm, c->feat, c->w0, c->w1, c->m0, c->m1};
    for (int i = 0; i < 10; i++)
        if (v[i] < 8 || v[i] % 8 || v[i] > MAX_WIDTH) {
            set_error("%s: every width must be a multiple of 8 in 8 .. %d (c1, c2, c3, c4, cpm, feat, w0, w1, m0, m1: entry %d is %d)", me,
                      MAX_WIDTH, i, v[i]);
            return false;
        }
    if (c->n_paf < 1 || c->n_paf > SOAR_POSE_MAX_STAGES || c->n_heat < 1 || c->n_heat > SOAR_POSE_MAX_STAGES) {
        set_error("%s: need 1 .. %d stages per branch (n_paf=%d, n_heat=%d)", me, SOAR_POSE_MAX_STAGES, c->n_paf, c->n_heat);
        return false;
    }
    return true;
}
bool check_size(const char *me, int32_t B, int32_t H, int32_t W)
{
    if (B < 0 || H < 16 || W < 16 || H % 16 || W % 16 || (int64_t)(B > 0 ? B : 1) * H * W > MAX_PIX) {
        set_error("%s: need B >= 0, H and W multiples of 16, at least 16, and B H W <= 2^30 (B=%d, H=%d, W=%d)", me, B, H, W);
        return false;
    }
    return true;
}

// ---- the layers, in the order of soar_amd.pose.layer_keys ----
struct Layer {
    int cin, cout, kk, cinp, coutp, nseg;
    bool prelu;
    Seg seg[3];
    int iw, ib, is;                             // the plan's entries: weight, bias, slopes (-1: none)
};
constexpr int N_VGG = 12;                       // then 17 per stage
inline int stage_row(const SoarPoseConfig &c) { return c.feat + PAFP + HEATP; }     // [features | PAF | heat maps]

struct Net {
    std::vector<Layer> L;
    WeightPlan plan;
};
Net build_net(const SoarPoseConfig &c)
{
    Net net;
    auto add = [&](int cin, int cout, int kk, bool prelu, int cinp, int coutp, std::initializer_list<Seg> segs) {
        Layer l{};
        l.cin = cin; l.cout = cout; l.kk = kk; l.cinp = cinp; l.coutp = coutp; l.prelu = prelu;
        for (const Seg &s : segs) l.seg[l.nseg++] = s;
        l.iw = net.plan.add((size_t)cout * cin * kk, (size_t)coutp * kk * cinp);
        l.ib = net.plan.add((size_t)cout, (size_t)coutp);
        l.is = prelu ? net.plan.add((size_t)cout, (size_t)coutp) : -1;
        net.L.push_back(l);
    };
    auto plain = [&](int cin, int cout, int kk, bool prelu) { add(cin, cout, kk, prelu, cin, cout, {Seg{0, 0, cin}}); };
    add(3, c.c1, 9, false, IMGP, c.c1, {Seg{0, 0, 3}});
    plain(c.c1, c.c1, 9, false);
    plain(c.c1, c.c2, 9, false); plain(c.c2, c.c2, 9, false);
    plain(c.c2, c.c3, 9, false); plain(c.c3, c.c3, 9, false); plain(c.c3, c.c3, 9, false); plain(c.c3, c.c3, 9, false);
    plain(c.c3, c.c4, 9, false);
    plain(c.c4, c.c4, 9, true); plain(c.c4, c.cpm, 9, true); plain(c.cpm, c.feat, 9, true);
    const int F = c.feat;
    for (int br = 0; br < 2; br++) {            // the PAF branch (L2) first
        const int ns = br == 0 ? c.n_paf : c.n_heat, maps = br == 0 ? PAF : HEAT, mapsp = br == 0 ? PAFP : HEATP;
        for (int s = 0; s < ns; s++) {
            const int w = s == 0 ? c.w0 : c.w1, m = s == 0 ? c.m0 : c.m1;
            for (int b = 0; b < 5; b++)
                for (int j = 0; j < 3; j++) {
                    if (b > 0 || j > 0) { plain(j == 0 ? 3 * w : w, w, 9, true); continue; }
                    // the stage's input, as the weights order it -> as the row holds it
                    if (br == 0 && s == 0) plain(F, w, 9, true);
                    else if (br == 0 || s == 0) add(F + PAF, w, 9, true, F + PAFP, w, {Seg{0, 0, F}, Seg{F, F, PAF}});
                    else add(F + HEAT + PAF, w, 9, true, F + PAFP + HEATP, w, {Seg{0, 0, F}, Seg{F + PAFP, F, HEAT}, Seg{F, F + HEAT, PAF}});
                }
            plain(3 * w, m, 1, true);
            add(m, maps, 1, false, m, mapsp, {Seg{0, 0, m}});
        }
    }
    return net;
}

// ---- the workspace: floats ----
struct WsLayout {
    size_t in8, act[2], X, Y[2], M, total;
};
WsLayout ws_layout(const SoarPoseConfig &c, int B, int H, int W)
{
    WsLayout L{};
    Carver ws;
    const size_t p0 = (size_t)B * H * W, R = p0 / 64;
    size_t act = p0 * c.c1;
    const size_t lv[3] = {(p0 / 4) * (size_t)(c.c1 > c.c2 ? c.c1 : c.c2), (p0 / 16) * (size_t)(c.c2 > c.c3 ? c.c2 : c.c3),
                          R * (size_t)(c.c3 > c.c4 ? (c.c3 > c.cpm ? c.c3 : c.cpm) : (c.c4 > c.cpm ? c.c4 : c.cpm))};
    for (size_t v : lv) act = v > act ? v : act;
    const size_t wmax = c.w0 > c.w1 ? c.w0 : c.w1, mmax = c.m0 > c.m1 ? c.m0 : c.m1;
    L.in8 = ws.offset<float>(p0 * IMGP);
    for (int i = 0; i < 2; i++) L.act[i] = ws.offset<float>(act);
    L.X = ws.offset<float>(R * stage_row(c));
    for (int i = 0; i < 2; i++) L.Y[i] = ws.offset<float>(R * 3 * wmax);
    L.M = ws.offset<float>(R * mmax);
    L.total = ws.bytes() == 0 ? ALIGN : ws.bytes();
    return L;
}

// ---- small image kernels ----
__global__ void __launch_bounds__(256) pose_preprocess_kernel(const uint8_t *rgb, float *bgr, int64_t npix)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
#pragma unroll
    for (int c = 0; c < 3; c++) bgr[p * 3 + c] = (float)rgb[p * 3 + (2 - c)] / 256.f - 0.5f;
}
ConvGemm conv_k(const float *x, int64_t ldx, float *y, int64_t ldy, int N, int H, int W, int Cin, int Cout, int kk, const float *w,
                const float *bias, const float *slope, int act)
{
    ConvGemm k{};
    k.x = x; k.ldx = ldx; k.xim = (int64_t)H * W;
    k.y = y; k.ldy = ldy; k.yim = (int64_t)H * W; k.Wout = W; k.os = 1;
    k.alpha = 1.f; k.bias = bias; k.slope = slope; k.act = act;
    k.N = N; k.Hg = H; k.Wg = W; k.Hin = H; k.Win = W; k.Cin = Cin; k.Cout = Cout;
    k.stride = 1; k.dil = 1; k.nph = 1;
    const int side = kk == 9 ? 3 : 1;
    square_taps(k.ph[0], w, (int64_t)kk * Cin, side, -(side / 2));
    return k;
}

// ---- the peaks ----
struct PeaksK {
    const float *heat;
    float *peaks;
    int32_t *counts;
    int h, w, P, max_peaks, R, NS;
    float thr;
};
constexpr int PEAK_THREADS = 1024;          // 25 workgroups a frame: each as wide as a workgroup gets
inline int peaks_src_rows(int R) { return (R + 8) / 8 + 5; }
inline size_t peaks_lds(int w, int R)
{
    const size_t Wp = 8 * (size_t)w + 8, nw = (8 * (size_t)w + 63) / 64;
    return ((size_t)(R + 8) * Wp + (size_t)peaks_src_rows(R) * w + 32) * sizeof(float) + (size_t)R * nw * sizeof(unsigned long long);
}
__global__ void __launch_bounds__(PEAK_THREADS) pose_peaks_kernel(PeaksK k)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ int new_y[MAXP], new_x[MAXP];
    __shared__ int count, n_new;
    const int tid = threadIdx.x, part = blockIdx.x, b = blockIdx.y;
    if (part == k.P - 1) {                       // the background map
        if (tid == 0) k.counts[(size_t)b * k.P + part] = 0;
        return;
    }
    const int HH = 8 * k.h, WW = 8 * k.w, Wp = WW + 8, nw = (WW + 63) / 64, R = k.R;
    unsigned long long *mask = reinterpret_cast<unsigned long long *>(lds_raw);           // [R][nw]
    float *wt = reinterpret_cast<float *>(mask + (size_t)R * nw);                          // [8][4]
    float *U = wt + 32;                                                                    // [R + 8][Wp]
    float *src = U + (size_t)(R + 8) * Wp;                                                 // [NS][w]
    if (tid < 8) up_weights(tid, wt + 4 * tid);
    if (tid == 0) count = 0;
    const float *heat = k.heat + (size_t)b * k.h * k.w * k.P + part;
    float *out = k.peaks + ((size_t)b * k.P + part) * k.max_peaks * 3;
    for (int Y0 = 0; Y0 < HH; Y0 += R) {
        const int iy_lo = up_cell(Y0 - 4) - 1;
        __syncthreads();
        for (int e = tid; e < k.NS * k.w; e += PEAK_THREADS) {
            const int r = e / k.w, x = e - r * k.w;
            const int iy = min(max(iy_lo + r, 0), k.h - 1);
            src[e] = heat[((size_t)iy * k.w + x) * k.P];
        }
        if (tid == 0) n_new = 0;
        __syncthreads();
        for (int e = tid; e < (R + 8) * Wp; e += PEAK_THREADS) {
            const int r = e / Wp, c = e - r * Wp;
            const int Y = Y0 - 4 + r, X = c - 4;
            float v = 0.f;
            if (Y >= 0 && Y < HH && X >= 0 && X < WW) {
                const int iy = up_cell(Y), ix = up_cell(X);
                const float *wy = wt + 4 * up_phase(Y), *wx = wt + 4 * up_phase(X);
                const int x0 = min(max(ix - 1, 0), k.w - 1), x1 = min(max(ix, 0), k.w - 1), x2 = min(max(ix + 1, 0), k.w - 1),
                          x3 = min(max(ix + 2, 0), k.w - 1);
                float row[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const float *s = src + (size_t)(iy - 1 + j - iy_lo) * k.w;
                    row[j] = up_sum4(wx, s[x0], s[x1], s[x2], s[x3]);
                }
                v = up_sum4(wy, row[0], row[1], row[2], row[3]);
            }
            U[e] = v;
        }
        __syncthreads();
        // 64 consecutive pixels of a row per wavefront: the ballot is the row's mask word
        bool found = false;
        for (int e = tid; e < R * nw * 64; e += PEAK_THREADS) {
            const int r = e / (nw * 64), X = e - r * (nw * 64), Y = Y0 + r;
            bool peak = false;
            if (Y >= 1 && Y <= HH - 2 && X >= 1 && X <= WW - 2) {
                const float *u = U + (size_t)(r + 4) * Wp + X + 4;
                const float v = u[0];
                peak = v > k.thr && v > u[-Wp - 1] && v > u[-Wp] && v > u[-Wp + 1] && v > u[-1] && v > u[1] && v > u[Wp - 1] && v > u[Wp] &&
                       v > u[Wp + 1];
            }
            const unsigned long long word = __ballot(peak);
            if ((tid & 63) == 0) mask[e >> 6] = word;
            found = found || peak;
        }
        if (__syncthreads_or(found) && tid == 0) {       // (most strips hold no peak: nothing to read out)
            int cnt = count, nn = 0;
            for (int wd = 0; wd < R * nw; wd++) {
                unsigned long long bits = mask[wd];
                if (cnt >= k.max_peaks) { cnt += __builtin_popcountll(bits); continue; }
                while (bits) {
                    if (cnt < k.max_peaks) { new_y[nn] = Y0 + wd / nw; new_x[nn] = (wd % nw) * 64 + (int)__builtin_ctzll(bits); nn++; }
                    cnt++;
                    bits &= bits - 1;
                }
            }
            n_new = nn;
            count = cnt;
        }
        __syncthreads();
        if (tid < n_new) {
            const int Y = new_y[tid], X = new_x[tid];
            float sx = 0.f, sy = 0.f, sw = 0.f;
            for (int yy = max(Y - 3, 0); yy <= min(Y + 3, HH - 1); yy++)
                for (int xx = max(X - 3, 0); xx <= min(X + 3, WW - 1); xx++) {
                    const float s = U[(size_t)(yy - Y0 + 4) * Wp + xx + 4];
                    if (s > 0.f) { sx = sx + (float)xx * s; sy = sy + (float)yy * s; sw = sw + s; }
                }
            float *o = out + (size_t)(min(count, k.max_peaks) - n_new + tid) * 3;
            o[0] = sx / sw + 0.5f;
            o[1] = sy / sw + 0.5f;
            o[2] = U[(size_t)(Y - Y0 + 4) * Wp + X + 4];
        }
    }
    __syncthreads();
    if (tid == 0) k.counts[(size_t)b * k.P + part] = count;
}

// ---- the assembly ----
constexpr int MAX_SUB = NPARTS * MAXP / 2;      // a new person takes two peaks nobody holds, and a peak is held once: never more
struct Person {
    signed char part[NPARTS + 3];               // the peak's index, -1: none
    float score;
    int n;                                      // parts; 0: merged into another
};
__global__ void __launch_bounds__(256) pose_assemble_kernel(SoarPoseAssembleArgs k)
{
    __shared__ float pk[NPARTS][MAXP][3];
    __shared__ int np[NPARTS];
    __shared__ float sc[MAXP * MAXP];
    __shared__ Person persons[MAX_SUB];
    __shared__ int conn_a[MAXP], conn_b[MAXP], n_conn, n_sub, kept[MAX_PEOPLE], n_kept;
    __shared__ float conn_s[MAXP];
    const int tid = threadIdx.x, b = blockIdx.x, P = HEAT;
    if (tid < NPARTS) np[tid] = min(max(k.counts[(size_t)b * P + tid], 0), k.max_peaks);
    if (tid == 0) n_sub = 0;
    __syncthreads();
    for (int e = tid; e < NPARTS * MAXP * 3; e += 256) {
        const int p = e / (MAXP * 3), r = e - p * (MAXP * 3), i = r / 3;
        if (i < np[p]) (&pk[0][0][0])[e] = k.peaks[(((size_t)b * P + p) * k.max_peaks + i) * 3 + (r - 3 * i)];
    }
    __syncthreads();
    const float *paf = k.paf + (size_t)b * k.h * k.w * PAF;
    for (int pr = 0; pr < NPAIRS; pr++) {
        const int pa = k.pair_a[pr], pb = k.pair_b[pr], na = np[pa], nb = np[pb];
        if (na == 0 || nb == 0) continue;       // (uniform over the workgroup)
        for (int e = tid; e < na * nb; e += 256) {
            const int ia = e / nb, ib = e - ia * nb;
            const float ax = pk[pa][ia][0], ay = pk[pa][ia][1];
            const float dx = pk[pb][ib][0] - ax, dy = pk[pb][ib][1] - ay;
            const float n = sqrtf(dx * dx + dy * dy);
            float score = -INFINITY;
            if (n >= 1e-6f) {
                const int m = min(max(5, (int)floorf(sqrtf(5.f * n) + 0.5f)), 25);
                const float ux = dx / n, uy = dy / n, den = (float)max(m - 1, 1);
                float sum = 0.f;
                int cnt = 0;
                for (int i = 0; i < m; i++) {
                    const float t = (float)i / den;
                    const float sx = ax + dx * t, sy = ay + dy * t;
                    const int cx = (int)fminf(fmaxf(floorf(sx * 0.125f), 0.f), (float)(k.w - 1));
                    const int cy = (int)fminf(fmaxf(floorf(sy * 0.125f), 0.f), (float)(k.h - 1));
                    const float *v = paf + ((size_t)cy * k.w + cx) * PAF;
                    const float s = v[k.paf_x[pr]] * ux + v[k.paf_y[pr]] * uy;
                    if (s > k.inter_threshold) { sum = sum + s; cnt++; }
                }
                if (cnt > 0 && (float)cnt / (float)m > k.min_above) score = sum / (float)cnt;
            }
            sc[e] = score;
        }
        __syncthreads();
        if (tid < 64) {
            // the best connection left, again and again: every lane ends up with the same answer and keeps the used ends itself
            unsigned used_a = 0u, used_b = 0u;
            int nc = 0;
            for (;;) {
                float best = -INFINITY;
                int at = 0x7fffffff;
                for (int e = tid; e < na * nb; e += 64) {
                    const int ia = e / nb, ib = e - ia * nb;
                    const float s = sc[e];
                    if (((used_a >> ia) | (used_b >> ib)) & 1u) continue;
                    if (s > best) { best = s; at = e; }          // (e ascends: a tie keeps the first)
                }
#pragma unroll
                for (int mlane = 32; mlane >= 1; mlane >>= 1) {
                    const float ob = __shfl_xor(best, mlane);
                    const int oa = __shfl_xor(at, mlane);
                    if (ob > best || (ob == best && oa < at)) { best = ob; at = oa; }
                }
                if (at == 0x7fffffff || !(best > -INFINITY)) break;
                const int ia = at / nb, ib = at - ia * nb;
                used_a |= 1u << ia; used_b |= 1u << ib;
                if (tid == 0) { conn_a[nc] = ia; conn_b[nc] = ib; conn_s[nc] = best; }
                nc++;
            }
            if (tid == 0) n_conn = nc;
        }
        __syncthreads();
        if (tid == 0) {
            int ns = n_sub;
            for (int c = 0; c < n_conn; c++) {
                const int ia = conn_a[c], ib = conn_b[c];
                const float cs = conn_s[c], sa = pk[pa][ia][2], sb = pk[pb][ib][2];
                int i = -1, j = -1;
                for (int q = 0; q < ns; q++) {
                    if (persons[q].n == 0) continue;
                    if (i < 0 && persons[q].part[pa] == ia) i = q;
                    if (j < 0 && persons[q].part[pb] == ib) j = q;
                }
                if (i >= 0 && j >= 0) {
                    if (i == j) continue;
                    bool disjoint = true;
                    for (int p = 0; p < NPARTS; p++) disjoint = disjoint && (persons[i].part[p] < 0 || persons[j].part[p] < 0);
                    if (!disjoint) continue;
                    for (int p = 0; p < NPARTS; p++)
                        if (persons[j].part[p] >= 0) persons[i].part[p] = persons[j].part[p];
                    persons[i].score = (persons[i].score + persons[j].score) + cs;
                    persons[i].n += persons[j].n;
                    persons[j].n = 0;
                } else if (i >= 0) {
                    if (persons[i].part[pb] < 0) { persons[i].part[pb] = (signed char)ib; persons[i].score = persons[i].score + (sb + cs); persons[i].n++; }
                } else if (j >= 0) {
                    if (persons[j].part[pa] < 0) { persons[j].part[pa] = (signed char)ia; persons[j].score = persons[j].score + (sa + cs); persons[j].n++; }
                } else if (ns < MAX_SUB) {
                    Person &q = persons[ns++];
                    for (int p = 0; p < NPARTS; p++) q.part[p] = -1;
                    q.part[pa] = (signed char)ia; q.part[pb] = (signed char)ib;
                    q.score = (sa + sb) + cs;
                    q.n = 2;
                }
            }
            n_sub = ns;
        }
        __syncthreads();
    }
    if (tid == 0) {
        int nk = 0;
        for (int q = 0; q < n_sub; q++) {
            const Person &p = persons[q];
            if (p.n == 0 || p.n < k.min_parts || p.score / (float)p.n < k.min_score) continue;
            if (nk < k.max_people) kept[nk] = q;
            nk++;
        }
        n_kept = nk;
        k.n_people[b] = nk;
    }
    __syncthreads();
    float *out = k.people + (size_t)b * k.max_people * NPARTS * 3;
    for (int e = tid; e < k.max_people * NPARTS; e += 256) {
        const int q = e / NPARTS, p = e - q * NPARTS;
        const int i = q < min(n_kept, k.max_people) ? persons[kept[q]].part[p] : -1;
        out[3 * e] = i >= 0 ? pk[p][i][0] : 0.f;
        out[3 * e + 1] = i >= 0 ? pk[p][i][1] : 0.f;
        out[3 * e + 2] = i >= 0 ? pk[p][i][2] : 0.f;
    }
}

__global__ void __launch_bounds__(256) pose_scale_kernel(float *people, int64_t n, float W, float net_w, float H, float net_h)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    people[3 * e] = people[3 * e] * W / net_w;
    people[3 * e + 1] = people[3 * e + 1] * H / net_h;
}

}  // namespace
}  // namespace soar

using namespace soar;

extern "C" int soar_pose_weights_size(const SoarPoseConfig *cfg, size_t *bytes, int32_t *count)
{
    const char *me = "soar_pose_weights_size";
    if (!bytes) { set_error("%s: NULL bytes", me); return 1; }
    if (!check_cfg(me, cfg)) return 1;
    const Net net = build_net(*cfg);
    *bytes = align_up(net.plan.total * sizeof(float));
    if (count) *count = net.plan.count();
    return 0;
}

extern "C" int soar_pose_workspace_size(const SoarPoseConfig *cfg, int32_t B, int32_t H, int32_t W, size_t *bytes)
{
    const char *me = "soar_pose_workspace_size";
    if (!bytes) { set_error("%s: NULL bytes", me); return 1; }
    if (!check_cfg(me, cfg) || !check_size(me, B, H, W)) return 1;
    *bytes = ws_layout(*cfg, B, H, W).total;
    return 0;
}

extern "C" int soar_pose_pack_weights(const SoarPoseConfig *cfg, const float *const *tensors, const int64_t *sizes, int32_t count, void *packed,
                                      size_t packed_bytes, void *stream_)
{
    const char *me = "soar_pose_pack_weights";
    if (!check_cfg(me, cfg)) return 1;
    if (!sizes) { set_error("%s: NULL sizes", me); return 1; }
    const Net net = build_net(*cfg);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    // entry -> its layer and role (0 weight, 1 bias, 2 slopes)
    std::vector<int> layer_of(net.plan.count()), role_of(net.plan.count());
    for (size_t l = 0; l < net.L.size(); l++) {
        layer_of[net.L[l].iw] = layer_of[net.L[l].ib] = (int)l; role_of[net.L[l].iw] = 0; role_of[net.L[l].ib] = 1;
        if (net.L[l].is >= 0) { layer_of[net.L[l].is] = (int)l; role_of[net.L[l].is] = 2; }
    }
    return pack_weights(net.plan, tensors, sizes, count, packed, packed_bytes, stream, me, [&](int i, const float *src, float *dst) {
        const Layer &l = net.L[layer_of[i]];
        if (role_of[i] == 0) {
            PackK k{};
            k.w = src; k.out = dst; k.cin = l.cin; k.cout = l.cout; k.kk = l.kk; k.cinp = l.cinp; k.nseg = l.nseg;
            for (int s = 0; s < l.nseg; s++) k.seg[s] = l.seg[s];
            k.n = (int64_t)l.coutp * l.kk * l.cinp;
            hipLaunchKernelGGL(pose_pack_kernel, dim3(blocks(k.n)), dim3(256), 0, stream, k);
            SOAR_LAUNCH_OK("pose_pack", stream, 0);
            return 0;
        }
        if (l.coutp == l.cout) return PACK_COPY;
        hipLaunchKernelGGL(pose_pad_kernel, dim3(blocks(l.coutp)), dim3(256), 0, stream, src, dst, l.cout, l.coutp);
        SOAR_LAUNCH_OK("pose_pad", stream, 0);
        return 0;
    });
}

extern "C" int soar_pose_preprocess(int32_t B, int32_t H, int32_t W, const uint8_t *rgb, float *bgr, void *stream_)
{
    if (B < 0 || H < 1 || W < 1 || (int64_t)(B > 0 ? B : 1) * H * W > MAX_PIX) {
        set_error("soar_pose_preprocess: need B >= 0, H, W >= 1 and B H W <= 2^30 (B=%d, H=%d, W=%d)", B, H, W);
        return 1;
    }
    if (B == 0) return 0;
    if (!rgb || !bgr) { set_error("soar_pose_preprocess: NULL %s", rgb ? "bgr" : "rgb"); return 1; }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int64_t npix = (int64_t)B * H * W;
    hipLaunchKernelGGL(pose_preprocess_kernel, dim3(blocks(npix)), dim3(256), 0, stream, rgb, bgr, npix);
    SOAR_LAUNCH_OK("pose_preprocess", stream, 0);
    return 0;
}

extern "C" int soar_pose_forward(const SoarPoseConfig *cfg, const void *packed, const SoarPoseNetArgs *a, void *workspace, size_t workspace_bytes,
                                 void *stream_)
{
    const char *me = "soar_pose_forward";
    if (!check_cfg(me, cfg)) return 1;
    if (!a) { set_error("%s: NULL args", me); return 1; }
    if (!check_size(me, a->B, a->H, a->W)) return 1;
    if (a->B == 0) return 0;
    const SoarPoseConfig &c = *cfg;
    const int n_stages = c.n_paf + c.n_heat;
    if (!packed || ((uintptr_t)packed & (ALIGN - 1)) || !a->x || !a->stage_out[c.n_paf - 1] || !a->stage_out[n_stages - 1]) {
        set_error("%s: need the packed weights (256-byte aligned), x and the last stage's output of either branch", me);
        return 1;
    }
    const WsLayout WL = ws_layout(c, a->B, a->H, a->W);
    if (!workspace_ok(me, workspace, workspace_bytes, WL.total, "soar_pose_workspace_size")) return 1;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const Net net = build_net(c);
    const float *P = static_cast<const float *>(packed);
    char *ws = static_cast<char *>(workspace);
    auto at = [&](size_t off) { return reinterpret_cast<float *>(ws + off); };
    float *in8 = at(WL.in8), *act[2] = {at(WL.act[0]), at(WL.act[1])}, *X = at(WL.X), *Y[2] = {at(WL.Y[0]), at(WL.Y[1])}, *M = at(WL.M);
    const int B = a->B;
    int H = a->H, W = a->W;
    const int64_t npix = (int64_t)B * H * W;
    const int xrow = stage_row(c), F = c.feat;

    IngestK ik{};
    ik.x = a->x; ik.y = in8; ik.npix = npix; ik.H = H; ik.W = W;
    for (int j = 0; j < 4; j++) ik.xs[j] = a->x_stride[j];
    hipLaunchKernelGGL(pose_ingest_kernel, dim3(blocks(npix)), dim3(256), 0, stream, ik);
    SOAR_LAUNCH_OK("pose_ingest", stream, 0);

    // one layer: x's channels [0, cinp) of rows ldx apart -> y's [0, cout) of rows ldy apart
    auto conv = [&](int li, const float *x, int64_t ldx, float *y, int64_t ldy, int act_) {
        const Layer &l = net.L[li];
        const ConvGemm k = conv_k(x, ldx, y, ldy, B, H, W, l.cinp, l.coutp, l.kk, P + net.plan.off[l.iw], P + net.plan.off[l.ib],
                                  l.is >= 0 ? P + net.plan.off[l.is] : nullptr, act_);
        return launch_conv_gemm(k, stream);
    };
    // the VGG front: ReLU up to conv4_1, pools behind conv1_2, conv2_2 and conv3_4
    const float *cur = in8;
    int cur_c = IMGP, side = 0, li = 0;
    for (; li < 9; li++) {
        if (conv(li, cur, cur_c, act[side], net.L[li].coutp, ACT_RELU)) return 1;
        cur = act[side]; cur_c = net.L[li].coutp; side ^= 1;
        if (li == 1 || li == 3 || li == 7) {
            const int64_t n4 = (int64_t)B * (H / 2) * (W / 2) * (cur_c / 4);
            hipLaunchKernelGGL(pose_pool_kernel, dim3(blocks(n4)), dim3(256), 0, stream, cur, act[side], n4, H, W, cur_c);
            SOAR_LAUNCH_OK("pose_pool", stream, 0);
            cur = act[side]; side ^= 1; H /= 2; W /= 2;
        }
    }
    for (; li < N_VGG; li++) {                   // conv4_2, conv4_3_CPM, conv4_4_CPM with their PReLUs; the last into the stage row
        const bool last = li == N_VGG - 1;
        if (conv(li, cur, cur_c, last ? X : act[side], last ? xrow : net.L[li].coutp, ACT_NONE)) return 1;
        cur = act[side]; cur_c = net.L[li].coutp; side ^= 1;
    }
    const int64_t rows = (int64_t)B * H * W;
    auto slice = [&](int off, int C, float *dst) {
        if (!dst) return 0;
        hipLaunchKernelGGL(pose_slice_kernel, dim3(blocks(rows * C)), dim3(256), 0, stream, X, (int64_t)xrow, off, C, dst, rows * C);
        SOAR_LAUNCH_OK("pose_slice", stream, 0);
        return 0;
    };
    if (slice(0, F, a->features)) return 1;
    for (int s = 0; s < n_stages; s++) {
        const bool paf = s < c.n_paf;
        const int w3 = 3 * net.L[li].coutp;
        for (int b = 0; b < 5; b++) {
            float *y = Y[b & 1];
            const float *x = b == 0 ? X : Y[(b & 1) ^ 1];
            const int64_t ldx = b == 0 ? xrow : w3;
            if (conv(li++, x, ldx, y, w3, ACT_NONE)) return 1;
            if (conv(li++, y, w3, y + w3 / 3, w3, ACT_NONE)) return 1;
            if (conv(li++, y + w3 / 3, w3, y + 2 * (w3 / 3), w3, ACT_NONE)) return 1;
        }
        const int m = net.L[li].coutp;
        if (conv(li++, Y[0], w3, M, m, ACT_NONE)) return 1;
        // the maps and their zero pad channels (zero rows of the packed matrix, zero bias) into their segment of the stage row
        const int off = paf ? F : F + PAFP;
        if (conv(li++, M, m, X + off, xrow, ACT_NONE)) return 1;
        if (slice(off, paf ? PAF : HEAT, a->stage_out[s])) return 1;
    }
    return 0;
}

extern "C" int soar_pose_peaks(int32_t B, int32_t h, int32_t w, const float *heat, float threshold, int32_t max_peaks, float *peaks,
                               int32_t *counts, void *stream_)
{
    const char *me = "soar_pose_peaks";
    if (B < 0 || B > 65535 || h < 1 || w < 1 || 8 * (int64_t)w > 1800 || h > (1 << 20) || max_peaks < 1 || max_peaks > MAXP || !(threshold >= 0.f)) {
        set_error("%s: need B in 0 .. 65535, h >= 1, 1 <= 8 w <= 1800, max_peaks in 1 .. %d and threshold >= 0 (B=%d, h=%d, w=%d, max_peaks=%d, "
                  "threshold=%g)", me, MAXP, B, h, w, max_peaks, (double)threshold);
        return 1;
    }
    if (B == 0) return 0;
    if (!heat || !peaks || !counts) { set_error("%s: NULL heat / peaks / counts", me); return 1; }
    PeaksK k{};
    k.heat = heat; k.peaks = peaks; k.counts = counts; k.h = h; k.w = w; k.P = HEAT; k.max_peaks = max_peaks; k.thr = threshold;
    k.R = 8;
    while (k.R > 1 && peaks_lds(w, k.R) > 60 * 1024) k.R /= 2;     // the strip's rows; a pixel's value does not depend on them
    k.NS = peaks_src_rows(k.R);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(pose_peaks_kernel, dim3(HEAT, (unsigned)B), dim3(PEAK_THREADS), peaks_lds(w, k.R), stream, k);
    SOAR_LAUNCH_OK("pose_peaks", stream, 0);
    return 0;
}

extern "C" int soar_pose_assemble(const SoarPoseAssembleArgs *a, void *stream_)
{
    const char *me = "soar_pose_assemble";
    if (!a) { set_error("%s: NULL args", me); return 1; }
    if (a->B < 0 || a->h < 1 || a->w < 1 || a->max_peaks < 1 || a->max_peaks > MAXP || a->max_people < 1 || a->max_people > MAX_PEOPLE) {
        set_error("%s: need B >= 0, h, w >= 1, max_peaks in 1 .. %d and max_people in 1 .. %d (B=%d, h=%d, w=%d, max_peaks=%d, max_people=%d)", me,
                  MAXP, MAX_PEOPLE, a->B, a->h, a->w, a->max_peaks, a->max_people);
        return 1;
    }
    for (int p = 0; p < NPAIRS; p++)
        if (a->pair_a[p] < 0 || a->pair_a[p] >= NPARTS || a->pair_b[p] < 0 || a->pair_b[p] >= NPARTS || a->pair_a[p] == a->pair_b[p] ||
            a->paf_x[p] < 0 || a->paf_x[p] >= PAF || a->paf_y[p] < 0 || a->paf_y[p] >= PAF) {
            set_error("%s: pair %d: parts must be two of 0 .. %d and the PAF channels in 0 .. %d", me, p, NPARTS - 1, PAF - 1);
            return 1;
        }
    if (a->B == 0) return 0;
    if (!a->peaks || !a->counts || !a->paf || !a->people || !a->n_people) { set_error("%s: NULL peaks / counts / paf / people / n_people", me); return 1; }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(pose_assemble_kernel, dim3((unsigned)a->B), dim3(256), 0, stream, *a);
    SOAR_LAUNCH_OK("pose_assemble", stream, 0);
    return 0;
}

extern "C" int soar_pose_scale(int64_t n, float *people, float W, float net_w, float H, float net_h, void *stream_)
{
    if (n < 0 || !(net_w > 0.f) || !(net_h > 0.f)) { set_error("soar_pose_scale: need n >= 0 and positive net sizes"); return 1; }
    if (n == 0) return 0;
    if (!people) { set_error("soar_pose_scale: NULL people"); return 1; }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(pose_scale_kernel, dim3(blocks(n)), dim3(256), 0, stream, people, n, W, net_w, H, net_h);
    SOAR_LAUNCH_OK("pose_scale", stream, 0);
    return 0;
}
