// unet_train.h - one training step of the reference's UNet (awesome/model/unet.py) on one image, fp32: the forward pass with batch
// statistics and the whole backward pass.  Same 18 convolutions + OutConv as unet.h (unet_plan), same products (gemm.h), and again the
// new kernels are what stands around them.
//
// Forward, per convolution i:  y_i [cout][hwp] = W_i [cout][Kp] . Col_i (weights packed per call WITHOUT a fold: unet_pack_kernel with
// gamma == nullptr), then one workgroup per channel reduces mean and biased variance over the P pixels in a fixed order and leaves
//     a = gamma / sqrt(var + eps),  b = beta - mean a,  mean,  1 / sqrt(var + eps)
// per layer (and updates the running statistics as torch does).  y_i stays as it left the product: a training-mode BatchNorm depends on
// y_i and cannot be folded, so every reader applies max(0, a y + b) per loaded value (unet_tgather_kernel, unet_tout_kernel).  All 18
// maps and their statistics survive until the backward, so the workspace has its own layout (no skip map is overwritten).
//
// Backward, i = 17 .. 0, from G_i = dL / d relu(bn(y_i)) (one buffer per convolution):
//   unet_bn_sums_kernel   g = G [a y + b > 0];  S1 = sum g (= dbeta),  S2 = sum g xhat (= dgamma): one workgroup per channel
//   unet_bn_dy_kernel     dy = a (g - S1 / P - xhat S2 / P) in place of G, zeros in the plane's padding columns
//   weight gradient       dW_i [cout][Kp] = dy . Col_i^T: Col_i gathered again strip by strip, the product cut into slices of
//                         UNET_TRAIN_DW_SLICE pixels (every slice its own partial), unet_dw_reduce_kernel adds the partials in pixel
//                         order and scatters into torch's [cout][cin][3][3] (column 9 cin: the bias gradient)
//   input gradient        D_i [cin][hwp] = Wt_i [cin][Kp'] . Col(dy): unet.h's direct gather on dy, Wt_i the flipped, transposed weights
//                         (unet_wt_pack_kernel; its column under the gather's row of ones is zero)
//   reader backward       gather form, a thread per destination element, no atomics.  Direct: the product writes G_{i-1} itself.
//                         Pool: unet_pool_bwd_kernel ADDS to the skip map's G (the Up block's concatenation wrote it first: its rows
//                         of D_i are produced straight into it).  Up: unet_up_bwd_kernel, the transpose of the interpolation.
// Strips are sized per layer from one Col budget.  Every reduction has a fixed order and whether a product is split depends on its
// shape only: two calls give the same bits.
#pragma once
#include "unet.h"

namespace {

constexpr int UNET_TCONVS = UNET_CONVS - 1;
constexpr long long UNET_TRAIN_COL_BUDGET = (long long)UNET_STRIP * 9232;   // floats of Col: what unet.h's default strip takes at base 64
constexpr int UNET_TRAIN_DW_SLICE = 2048;   // pixels per weight-gradient partial

struct UNetTrainPlan {
    UNetPlan p;                          // the convolutions and levels (its strip and workspace offsets are not used here)
    int strip[UNET_TCONVS];              // pixels per strip of Col_i (forward, weight gradient)
    int strip_b[UNET_TCONVS];            // ... of Col(dy_i) (input gradient)
    int kpt[UNET_TCONVS];                // Kp' = 9 cout + 1 rounded up to 16
    long long wt_off[UNET_TCONVS];       // Wt_i, floats from wt_base
    // workspace (floats from its base)
    long long y_off[UNET_TCONVS], g_off[UNET_TCONVS], stat_off[UNET_TCONVS];
    long long packed_off, wt_base, d_off, col_off, part_off, bytes;
    // the flat gradient buffer, parameters() order
    long long grad_w[UNET_CONVS], grad_b[UNET_CONVS], grad_gamma[UNET_TCONVS], grad_beta[UNET_TCONVS], param_count;
};

inline int unet_train_desc_rc(const InrUNetDesc* d) {
    const int rc = unet_desc_rc(d);
    if (rc) return rc;
    if ((d->height >> 4) * (d->width >> 4) < 2) return INR_EUNSUPPORTED;   // one value per channel at the bottom: no batch variance
    return INR_OK;
}

inline int unet_train_strip(const InrUNetDesc* d, int kp) {
    long long s = d->strip_points > 0 ? unet_round(d->strip_points, 128) : UNET_TRAIN_COL_BUDGET / kp / 128 * 128;
    if (s < 128) s = 128;
    if (s > (1 << 24)) s = 1 << 24;       // (a plane has at most 4096 x 4096 pixels)
    return (int)s;
}

// slices of the weight-gradient product over a plane of hw pixels cut into strips
inline int unet_train_dw_slices(int hw, int strip) {
    int n = 0;
    for (int p0 = 0; p0 < hw; p0 += strip) {
        const int n4 = unet_round(hw - p0 < strip ? hw - p0 : strip, 4);
        n += (n4 + UNET_TRAIN_DW_SLICE - 1) / UNET_TRAIN_DW_SLICE;
    }
    return n;
}

// (the descriptor has passed unet_train_desc_rc)
inline UNetTrainPlan unet_train_plan(const InrUNetDesc* d) {
    UNetTrainPlan t{};
    t.p = unet_plan(d);
    const UNetPlan& p = t.p;
    long long w = 0, wt = 0, gr = 0, col = 0, part = 1, dtmp = 1;
    auto take = [&](long long floats) { const long long at = w; w += (floats * 4 + 255) / 256 * 64; return at; };
    for (int i = 0; i < UNET_TCONVS; ++i) {
        const UNetConv& c = p.conv[i];
        const int hw = p.H[c.level] * p.W[c.level], hwp = p.hwp[c.level];
        t.kpt[i] = unet_kp(c.cout);
        t.strip[i] = unet_train_strip(d, c.kp);
        t.strip_b[i] = unet_train_strip(d, t.kpt[i]);
        t.wt_off[i] = wt;
        if (i > 0) wt += ((long long)c.cin * t.kpt[i] + 63) / 64 * 64;
        t.y_off[i] = take((long long)c.cout * hwp);
        t.g_off[i] = take((long long)c.cout * hwp);
        t.stat_off[i] = take(4ll * c.cout);
        t.grad_w[i] = gr; gr += 9ll * c.cin * c.cout;
        t.grad_b[i] = gr; gr += c.cout;
        t.grad_gamma[i] = gr; gr += c.cout;
        t.grad_beta[i] = gr; gr += c.cout;
        // Col of the forward / weight gradient and of the input gradient
        const long long ld = hwp < t.strip[i] ? hwp : t.strip[i], ldb = hwp < t.strip_b[i] ? hwp : t.strip_b[i];
        if (c.kp * ld > col) col = c.kp * ld;
        if (i > 0 && t.kpt[i] * ldb > col) col = t.kpt[i] * ldb;
        // split-K parts (forward; input gradient: at most cin rows per product) and weight-gradient partials
        if (unet_splitk(c.cout, hwp, c.kp, hwp <= t.strip[i]) && (long long)GEMM_SPLITK_MAX * c.cout * hwp > part)
            part = (long long)GEMM_SPLITK_MAX * c.cout * hwp;
        if (i > 0 && hwp <= t.strip_b[i] && (long long)GEMM_SPLITK_MAX * c.cin * hwp > part) part = (long long)GEMM_SPLITK_MAX * c.cin * hwp;
        const long long dw = (long long)unet_train_dw_slices(hw, t.strip[i]) * c.cout * c.kp;
        if (dw > part) part = dw;
        // the rows of D_i that do not go straight into a G
        const long long rows = c.src == UNET_SRC_POOL ? c.cin : (c.src == UNET_SRC_UP ? c.cin - c.cskip : 0);
        if (rows * hwp > dtmp) dtmp = rows * hwp;
    }
    t.grad_w[UNET_TCONVS] = gr; gr += (long long)d->out_chn * d->base_width;
    t.grad_b[UNET_TCONVS] = gr; gr += d->out_chn;
    t.param_count = gr;
    t.packed_off = take(p.packed_floats);
    t.wt_base = take(wt);
    t.d_off = take(dtmp);
    t.col_off = take(col);
    t.part_off = take(part);
    t.bytes = w * 4;
    return t;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
// unet.h's gather with the source's BatchNorm and ReLU applied to every loaded value: max(0, a[c] y + b[c])
struct UNetTGatherArgs {
    UNetGatherArgs g;
    const float* sa;       // a, b of the source (null: the network input, read as it is); UP: of the skip map
    const float* sb;
    const float* da;       // UP: of the deeper map
    const float* db;
};

__device__ __forceinline__ float unet_act(float a, float y, float b) { return fmaxf(fmaf(a, y, b), 0.f); }

template <int SRC>
__global__ __launch_bounds__(UNET_BLOCK) void unet_tgather_kernel(const UNetTGatherArgs t) {
    const UNetGatherArgs& a = t.g;
    const int col = blockIdx.x * UNET_BLOCK + threadIdx.x;
    if (col >= a.n4) return;
    const int groups = (a.cin + UNET_GATHER_CH - 1) / UNET_GATHER_CH;
    if ((int)blockIdx.y == groups) {                       // the row of ones and the zero rows behind it
        for (int k = 9 * a.cin; k < a.kp; ++k) a.col[(size_t)k * a.ld + col] = (k == 9 * a.cin && col < a.n) ? 1.f : 0.f;
        return;
    }
    const bool live = col < a.n;
    const int p = live ? a.p0 + col : a.p0;
    const int y = p / a.W, x = p - y * a.W;
    const int c0 = blockIdx.y * UNET_GATHER_CH, c1 = min(c0 + UNET_GATHER_CH, a.cin);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
        const bool in = live && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
        const int yc = min(max(yy, 0), a.H - 1), xc = min(max(xx, 0), a.W - 1);   // loads from clamped addresses, selected after
        float* out = a.col + ((size_t)c0 * 9 + tap) * a.ld + col;
        if (SRC == UNET_SRC_DIRECT) {
            const float* s = a.src + (size_t)c0 * a.src_ld + yc * a.W + xc;
            for (int c = c0; c < c1; ++c, s += a.src_ld, out += (size_t)9 * a.ld) {
                const float v = t.sa ? unet_act(t.sa[c], *s, t.sb[c]) : *s;
                *out = in ? v : 0.f;
            }
        } else if (SRC == UNET_SRC_POOL) {                 // (floor mode: 2 yc + 1 <= Hs - 1)
            const float* s = a.src + (size_t)c0 * a.src_ld + (2 * yc) * a.Ws + 2 * xc;
            for (int c = c0; c < c1; ++c, s += a.src_ld, out += (size_t)9 * a.ld) {
                const float ca = t.sa[c], cb = t.sb[c];
                const float v = fmaxf(fmaxf(unet_act(ca, s[0], cb), unet_act(ca, s[1], cb)),
                                      fmaxf(unet_act(ca, s[a.Ws], cb), unet_act(ca, s[a.Ws + 1], cb)));
                *out = in ? v : 0.f;
            }
        } else {                                           // (index and weight arithmetic: unet_gather_kernel)
            const int uy = yc - a.py0, ux = xc - a.px0;
            const bool inu = in && uy >= 0 && uy < 2 * a.Hd && ux >= 0 && ux < 2 * a.Wd;
            const float fy = a.sy * (float)min(max(uy, 0), 2 * a.Hd - 1), fx = a.sx * (float)min(max(ux, 0), 2 * a.Wd - 1);
            const int y0 = min((int)fy, a.Hd - 1), x0 = min((int)fx, a.Wd - 1);
            const int y1 = min(y0 + 1, a.Hd - 1), x1 = min(x0 + 1, a.Wd - 1);
            const float ly = fminf(fmaxf(fy - (float)y0, 0.f), 1.f), lx = fminf(fmaxf(fx - (float)x0, 0.f), 1.f);
            const float hy = 1.f - ly, hx = 1.f - lx;
            const int o00 = y0 * a.Wd + x0, o01 = y0 * a.Wd + x1, o10 = y1 * a.Wd + x0, o11 = y1 * a.Wd + x1;
            const int os = yc * a.W + xc;
            for (int c = c0; c < c1; ++c, out += (size_t)9 * a.ld) {
                float v;
                if (c < a.cskip) {                         // (uniform over the block)
                    v = in ? unet_act(t.sa[c], a.src[(size_t)c * a.src_ld + os], t.sb[c]) : 0.f;
                } else {
                    const float* s = a.deep + (size_t)(c - a.cskip) * a.deep_ld;
                    const float ca = t.da[c - a.cskip], cb = t.db[c - a.cskip];
                    const float v00 = unet_act(ca, s[o00], cb), v01 = unet_act(ca, s[o01], cb), v10 = unet_act(ca, s[o10], cb),
                                v11 = unet_act(ca, s[o11], cb);
                    v = inu ? hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11) : 0.f;
                }
                *out = v;
            }
        }
    }
}

// sum of v over the workgroup's 256 threads in a fixed order (a tree over LDS); every thread gets the result
__device__ __forceinline__ float unet_block_sum(float v, float* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = UNET_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// batch statistics of one channel per workgroup: stat = [a | b | mean | 1 / sigma] (cout floats each); running statistics in place
__global__ __launch_bounds__(UNET_BLOCK) void unet_stats_kernel(const float* __restrict__ y, int ld, int P, int cout,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                                float momentum, float* __restrict__ run_mean, float* __restrict__ run_var,
                                                                float* __restrict__ stat) {
    __shared__ float red[UNET_BLOCK];
    const int c = blockIdx.x;
    const float* row = y + (size_t)c * ld;
    float s = 0.f;
    for (int p = threadIdx.x; p < P; p += UNET_BLOCK) s += row[p];
    const float mean = unet_block_sum(s, red) / (float)P;
    float q = 0.f;
    for (int p = threadIdx.x; p < P; p += UNET_BLOCK) {
        const float dlt = row[p] - mean;
        q = fmaf(dlt, dlt, q);
    }
    const float var = unet_block_sum(q, red) / (float)P;
    if (threadIdx.x == 0) {
        const float istd = 1.f / sqrtf(var + eps);
        const float a = gamma[c] * istd;
        stat[c] = a;
        stat[cout + c] = beta[c] - mean * a;
        stat[2 * cout + c] = mean;
        stat[3 * cout + c] = istd;
        run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * mean;
        run_var[c] = (1.f - momentum) * run_var[c] + momentum * (var * ((float)P / (float)(P - 1)));
    }
}

// OutConv on the last map through its BatchNorm and ReLU: logits [oc][hw] = Wo [oc][kp] (act(x) | 1)
__global__ __launch_bounds__(UNET_BLOCK) void unet_tout_kernel(const float* __restrict__ x, int x_ld, int cin, const float* __restrict__ sa,
                                                               const float* __restrict__ sb, const float* __restrict__ Wo, int kp, int oc,
                                                               int hw, float* __restrict__ logits) {
    const int p = blockIdx.x * UNET_BLOCK + threadIdx.x;
    if (p >= hw) return;
    for (int o = 0; o < oc; ++o) {
        const float* w = Wo + (size_t)o * kp;
        float acc = w[cin];
        for (int c = 0; c < cin; ++c) acc = fmaf(w[c], unet_act(sa[c], x[(size_t)c * x_ld + p], sb[c]), acc);
        logits[(size_t)o * hw + p] = acc;
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------
// OutConv: G [cin][ld] = Wo^T dlogits (pixels < hw)
__global__ __launch_bounds__(UNET_BLOCK) void unet_out_bwd_kernel(const float* __restrict__ dlogits, const float* __restrict__ Wo, int kp,
                                                                  int oc, int cin, int hw, float* __restrict__ G, int ld) {
    const int p = blockIdx.x * UNET_BLOCK + threadIdx.x;
    if (p >= hw) return;
    for (int c = 0; c < cin; ++c) {
        float acc = 0.f;
        for (int o = 0; o < oc; ++o) acc = fmaf(Wo[(size_t)o * kp + c], dlogits[(size_t)o * hw + p], acc);
        G[(size_t)c * ld + p] = acc;
    }
}

// OutConv's weight and bias gradient: workgroup (c, o), c == cin the bias
__global__ __launch_bounds__(UNET_BLOCK) void unet_out_dw_kernel(const float* __restrict__ dlogits, const float* __restrict__ x, int x_ld,
                                                                 int cin, const float* __restrict__ sa, const float* __restrict__ sb, int hw,
                                                                 float* __restrict__ gw, float* __restrict__ gb) {
    __shared__ float red[UNET_BLOCK];
    const int c = blockIdx.x, o = blockIdx.y;
    const float* dl = dlogits + (size_t)o * hw;
    float s = 0.f;
    if (c < cin) {
        const float* row = x + (size_t)c * x_ld;
        const float ca = sa[c], cb = sb[c];
        for (int p = threadIdx.x; p < hw; p += UNET_BLOCK) s = fmaf(dl[p], unet_act(ca, row[p], cb), s);
    } else {
        for (int p = threadIdx.x; p < hw; p += UNET_BLOCK) s += dl[p];
    }
    s = unet_block_sum(s, red);
    if (threadIdx.x == 0) {
        if (c < cin) gw[(size_t)o * cin + c] = s;
        else gb[o] = s;
    }
}

// S1 = sum g -> dbeta, S2 = sum g xhat -> dgamma, g = G [a y + b > 0]; one channel per workgroup
__global__ __launch_bounds__(UNET_BLOCK) void unet_bn_sums_kernel(const float* __restrict__ G, const float* __restrict__ y, int ld, int P,
                                                                  int cout, const float* __restrict__ stat, float* __restrict__ dgamma,
                                                                  float* __restrict__ dbeta) {
    __shared__ float red[UNET_BLOCK];
    const int c = blockIdx.x;
    const float a = stat[c], b = stat[cout + c], mean = stat[2 * cout + c], istd = stat[3 * cout + c];
    const float* gr = G + (size_t)c * ld;
    const float* yr = y + (size_t)c * ld;
    float s1 = 0.f, s2 = 0.f;
    for (int p = threadIdx.x; p < P; p += UNET_BLOCK) {
        const float yv = yr[p];
        const float g = fmaf(a, yv, b) > 0.f ? gr[p] : 0.f;
        s1 += g;
        s2 = fmaf(g, (yv - mean) * istd, s2);
    }
    s1 = unet_block_sum(s1, red);
    s2 = unet_block_sum(s2, red);
    if (threadIdx.x == 0) {
        dbeta[c] = s1;
        dgamma[c] = s2;
    }
}

// dy = a (g - S1 / P - xhat S2 / P) in place of G; columns [P, ld) get zeros (the products contract over them)
__global__ __launch_bounds__(UNET_BLOCK) void unet_bn_dy_kernel(float* __restrict__ G, const float* __restrict__ y, int ld, int P, int cout,
                                                                const float* __restrict__ stat, const float* __restrict__ dgamma,
                                                                const float* __restrict__ dbeta) {
    const int p = blockIdx.x * UNET_BLOCK + threadIdx.x, c = blockIdx.y;
    if (p >= ld) return;
    const size_t at = (size_t)c * ld + p;
    if (p >= P) {
        G[at] = 0.f;
        return;
    }
    const float a = stat[c], b = stat[cout + c], mean = stat[2 * cout + c], istd = stat[3 * cout + c];
    const float inv = 1.f / (float)P;
    const float yv = y[at];
    const float g = fmaf(a, yv, b) > 0.f ? G[at] : 0.f;
    const float xh = (yv - mean) * istd;
    G[at] = a * (g - dbeta[c] * inv - xh * (dgamma[c] * inv));
}

// Wt [cin][kpt] from w [cout][cin][9]: Wt[i][(o, tap)] = w[o][i][8 - tap], zeros from column 9 cout on
__global__ __launch_bounds__(UNET_BLOCK) void unet_wt_pack_kernel(const float* __restrict__ w, int cout, int cin, int kpt,
                                                                  float* __restrict__ Wt) {
    const long long e = (long long)blockIdx.x * UNET_BLOCK + threadIdx.x;
    if (e >= (long long)cin * kpt) return;
    const int i = (int)(e / kpt), k = (int)(e - (long long)i * kpt);
    float v = 0.f;
    if (k < 9 * cout) {
        const int o = k / 9, tap = k - 9 * o;
        v = w[((size_t)o * cin + i) * 9 + (8 - tap)];
    }
    Wt[e] = v;
}

// dW [cout][kp] = the partials added in pixel order; columns < k go to gw [cout][k], column k to gb
__global__ __launch_bounds__(UNET_BLOCK) void unet_dw_reduce_kernel(const float* __restrict__ part, int slices, int cout, int k, int kp,
                                                                    float* __restrict__ gw, float* __restrict__ gb) {
    const long long e = (long long)blockIdx.x * UNET_BLOCK + threadIdx.x, mn = (long long)cout * kp;
    if (e >= mn) return;
    const int o = (int)(e / kp), c = (int)(e - (long long)o * kp);
    if (c > k) return;
    float v = 0.f;
    for (int z = 0; z < slices; ++z) v += part[(size_t)z * mn + e];
    if (c < k) gw[(size_t)o * k + c] = v;
    else gb[o] = v;
}

// max-pool reader: G [c][Hs x Ws] += D [c][H x W] of the pixel's window where the pixel is the window's first maximum (row-major
// order, over the ReLU'd values); rows / columns that floor mode drops get nothing
__global__ __launch_bounds__(UNET_BLOCK) void unet_pool_bwd_kernel(const float* __restrict__ D, int d_ld, int H, int W,
                                                                   const float* __restrict__ y, float* __restrict__ G, int ld, int Hs, int Ws,
                                                                   const float* __restrict__ sa, const float* __restrict__ sb) {
    const int p = blockIdx.x * UNET_BLOCK + threadIdx.x, c = blockIdx.y;
    if (p >= Hs * Ws) return;
    const int ys = p / Ws, xs = p - ys * Ws;
    const int wy = ys >> 1, wx = xs >> 1;
    if (wy >= H || wx >= W) return;
    const float* s = y + (size_t)c * ld + (2 * wy) * Ws + 2 * wx;
    const float ca = sa[c], cb = sb[c];
    const float v[4] = {unet_act(ca, s[0], cb), unet_act(ca, s[1], cb), unet_act(ca, s[Ws], cb), unet_act(ca, s[Ws + 1], cb)};
    int best = 0;
    float m = v[0];
#pragma unroll
    for (int j = 1; j < 4; ++j)
        if (v[j] > m) { m = v[j]; best = j; }
    const int own = (ys & 1) * 2 + (xs & 1);
    if (own == best) G[(size_t)c * ld + p] += D[(size_t)c * d_ld + wy * W + wx];
}

// Up reader, deeper map: G [c][Hd x Wd] = the transpose of the bilinear interpolation applied to D [c][H x W] (the rows of D behind the
// skip map's), each upsampled pixel's indices and weights computed as unet_gather_kernel computes them
__global__ __launch_bounds__(UNET_BLOCK) void unet_up_bwd_kernel(const float* __restrict__ D, int d_ld, int W, float* __restrict__ G, int ld,
                                                                 int Hd, int Wd, int py0, int px0, float sy, float sx) {
    const int p = blockIdx.x * UNET_BLOCK + threadIdx.x, c = blockIdx.y;
    if (p >= Hd * Wd) return;
    const int yd = p / Wd, xd = p - yd * Wd;
    // upsampled rows whose y0 or y1 can be yd: 2 yd - 3 .. 2 yd + 4 (a superset); the same for the columns
    float wy[8], wx[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int uy = 2 * yd - 3 + j, ux = 2 * xd - 3 + j;
        const float fy = sy * (float)min(max(uy, 0), 2 * Hd - 1), fx = sx * (float)min(max(ux, 0), 2 * Wd - 1);
        const int y0 = min((int)fy, Hd - 1), x0 = min((int)fx, Wd - 1);
        const int y1 = min(y0 + 1, Hd - 1), x1 = min(x0 + 1, Wd - 1);
        const float ly = fminf(fmaxf(fy - (float)y0, 0.f), 1.f), lx = fminf(fmaxf(fx - (float)x0, 0.f), 1.f);
        const bool iny = uy >= 0 && uy < 2 * Hd, inx = ux >= 0 && ux < 2 * Wd;
        wy[j] = iny ? (y0 == yd ? 1.f - ly : 0.f) + (y1 == yd ? ly : 0.f) : 0.f;
        wx[j] = inx ? (x0 == xd ? 1.f - lx : 0.f) + (x1 == xd ? lx : 0.f) : 0.f;
    }
    const float* d = D + (size_t)c * d_ld;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int uy = min(max(2 * yd - 3 + j, 0), 2 * Hd - 1);
        float r = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int ux = min(max(2 * xd - 3 + i, 0), 2 * Wd - 1);
            r = fmaf(wx[i], d[(uy + py0) * W + ux + px0], r);
        }
        acc = fmaf(wy[j], r, acc);
    }
    G[(size_t)c * ld + p] = acc;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
// index of the map a convolution reads (UP: its deeper map; the skip map is unet_train_skip); -1: the network input
inline int unet_train_src(int i) { return i - 1; }
inline int unet_train_skip(int i) { return UNET_TCONVS - 1 - i; }

// one strip of Col_i (forward and weight gradient)
inline void unet_train_gather(const UNetTrainPlan& t, int i, const float* input, int hw0, float* ws, int p0, int n, hipStream_t s) {
    const UNetPlan& p = t.p;
    const UNetConv& c = p.conv[i];
    const int l = c.level, hwp = p.hwp[l];
    UNetTGatherArgs a{};
    UNetGatherArgs& g = a.g;
    g.col = ws + t.col_off;
    g.cin = c.cin; g.cskip = c.cskip; g.kp = c.kp;
    g.H = p.H[l]; g.W = p.W[l];
    g.relu = i > 0;
    if (i == 0) {
        g.src = input; g.src_ld = hw0;
    } else {
        const int j = unet_train_src(i), lj = p.conv[j].level;
        const float* st = ws + t.stat_off[j];
        if (c.src == UNET_SRC_UP) {
            const int k = unet_train_skip(i);
            g.src = ws + t.y_off[k]; g.src_ld = hwp;
            a.sa = ws + t.stat_off[k]; a.sb = a.sa + p.conv[k].cout;
            g.deep = ws + t.y_off[j]; g.deep_ld = p.hwp[lj];
            a.da = st; a.db = st + p.conv[j].cout;
            g.Hd = p.H[lj]; g.Wd = p.W[lj];
            g.py0 = (g.H - 2 * g.Hd) / 2; g.px0 = (g.W - 2 * g.Wd) / 2;
            g.sy = g.Hd > 1 ? (float)(g.Hd - 1) / (float)(2 * g.Hd - 1) : 0.f;
            g.sx = g.Wd > 1 ? (float)(g.Wd - 1) / (float)(2 * g.Wd - 1) : 0.f;
        } else {
            g.src = ws + t.y_off[j]; g.src_ld = p.hwp[lj]; g.Ws = p.W[lj];
            a.sa = st; a.sb = st + p.conv[j].cout;
        }
    }
    g.ld = hwp < t.strip[i] ? hwp : t.strip[i];
    g.p0 = p0; g.n = n; g.n4 = unet_round(n, 4);
    const dim3 grid((g.n4 + UNET_BLOCK - 1) / UNET_BLOCK, (c.cin + UNET_GATHER_CH - 1) / UNET_GATHER_CH + 1);
    if (c.src == UNET_SRC_DIRECT) hipLaunchKernelGGL(unet_tgather_kernel<UNET_SRC_DIRECT>, grid, dim3(UNET_BLOCK), 0, s, a);
    else if (c.src == UNET_SRC_POOL) hipLaunchKernelGGL(unet_tgather_kernel<UNET_SRC_POOL>, grid, dim3(UNET_BLOCK), 0, s, a);
    else hipLaunchKernelGGL(unet_tgather_kernel<UNET_SRC_UP>, grid, dim3(UNET_BLOCK), 0, s, a);
}

inline int unet_train_forward(const InrUNetDesc* d, const UNetTrainPlan& t, const float* const* conv_w, const float* const* conv_b,
                              const float* const* gamma, const float* const* beta, float* const* run_mean, float* const* run_var,
                              float momentum, const float* input, float* logits, float* ws, hipStream_t s) {
    const UNetPlan& p = t.p;
    float* packed = ws + t.packed_off;
    float* col = ws + t.col_off;
    float* part = ws + t.part_off;
    const int hw0 = d->height * d->width;
    for (int i = 0; i < UNET_TCONVS; ++i) {                 // plain weights with the bias column: no fold
        const UNetConv& c = p.conv[i];
        const long long n = (long long)c.cout * c.kp;
        hipLaunchKernelGGL(unet_pack_kernel, dim3((unsigned)((n + UNET_BLOCK - 1) / UNET_BLOCK)), dim3(UNET_BLOCK), 0, s, conv_w[i], conv_b[i],
                           (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, 0.f, c.cout, 9 * c.cin,
                           c.kp, packed + c.w_off);
    }
    {
        const long long n = (long long)d->out_chn * p.out_kp;
        hipLaunchKernelGGL(unet_pack_kernel, dim3((unsigned)((n + UNET_BLOCK - 1) / UNET_BLOCK)), dim3(UNET_BLOCK), 0, s, conv_w[UNET_TCONVS],
                           conv_b[UNET_TCONVS], (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, 0.f,
                           d->out_chn, d->base_width, p.out_kp, packed + p.out_off);
    }
    for (int i = 0; i < UNET_TCONVS; ++i) {
        const UNetConv& c = p.conv[i];
        const int l = c.level, hw = p.H[l] * p.W[l], hwp = p.hwp[l], strip = t.strip[i];
        const int ld = hwp < strip ? hwp : strip;
        float* y = ws + t.y_off[i];
        for (int p0 = 0; p0 < hw; p0 += strip) {
            const int n = hw - p0 < strip ? hw - p0 : strip, n4 = unet_round(n, 4);
            unet_train_gather(t, i, input, hw0, ws, p0, n, s);
            int rc;
            if (unet_splitk(c.cout, hwp, c.kp, hwp <= strip))   // one strip = the whole plane: y is dense [cout][n4 = hwp]
                rc = gemm_rm_splitk(s, false, false, c.cout, n4, c.kp, packed + c.w_off, c.kp, col, ld, y, part);
            else
                rc = gemm_rm(s, false, false, c.cout, n4, c.kp, packed + c.w_off, c.kp, col, ld, y + p0, hwp);
            if (rc) return rc;
        }
        hipLaunchKernelGGL(unet_stats_kernel, dim3(c.cout), dim3(UNET_BLOCK), 0, s, (const float*)y, hwp, hw, c.cout, gamma[i], beta[i],
                           d->bn_eps, momentum, run_mean[i], run_var[i], ws + t.stat_off[i]);
    }
    const float* st = ws + t.stat_off[UNET_TCONVS - 1];
    hipLaunchKernelGGL(unet_tout_kernel, dim3((hw0 + UNET_BLOCK - 1) / UNET_BLOCK), dim3(UNET_BLOCK), 0, s,
                       (const float*)(ws + t.y_off[UNET_TCONVS - 1]), p.hwp[0], d->base_width, st, st + d->base_width,
                       (const float*)(packed + p.out_off), p.out_kp, d->out_chn, hw0, logits);
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

// D rows [r0, r0 + rows) of convolution i's input gradient into C [rows][hwp]: Wt_i . Col(dy_i), Col(dy_i) already in place for the strip
inline int unet_train_dgrad_rows(const UNetTrainPlan& t, int i, int r0, int rows, float* C, float* ws, int p0, int n4, int ldb,
                                 hipStream_t s) {
    const UNetPlan& p = t.p;
    const int hwp = p.hwp[p.conv[i].level], kpt = t.kpt[i];
    const float* Wt = ws + t.wt_base + t.wt_off[i] + (size_t)r0 * kpt;
    if (unet_splitk(rows, hwp, kpt, hwp <= t.strip_b[i]))
        return gemm_rm_splitk(s, false, false, rows, n4, kpt, Wt, kpt, ws + t.col_off, ldb, C, ws + t.part_off);
    return gemm_rm(s, false, false, rows, n4, kpt, Wt, kpt, ws + t.col_off, ldb, C + p0, hwp);
}

// reads what unet_train_forward left in ws (the maps y_i, their statistics, the packed weights)
inline int unet_train_backward(const InrUNetDesc* d, const UNetTrainPlan& t, const float* const* conv_w, const float* const* gamma,
                               const float* input, const float* dlogits, float* grads, float* ws, hipStream_t s) {
    (void)gamma;   // (a = gamma / sigma is in the statistics)
    const UNetPlan& p = t.p;
    float* col = ws + t.col_off;
    float* part = ws + t.part_off;
    float* Dt = ws + t.d_off;
    const int hw0 = d->height * d->width;
    for (int i = 1; i < UNET_TCONVS; ++i) {
        const UNetConv& c = p.conv[i];
        const long long n = (long long)c.cin * t.kpt[i];
        hipLaunchKernelGGL(unet_wt_pack_kernel, dim3((unsigned)((n + UNET_BLOCK - 1) / UNET_BLOCK)), dim3(UNET_BLOCK), 0, s, conv_w[i], c.cout,
                           c.cin, t.kpt[i], ws + t.wt_base + t.wt_off[i]);
    }
    {   // OutConv
        const int last = UNET_TCONVS - 1, b = d->base_width;
        const float* st = ws + t.stat_off[last];
        const float* Wo = ws + t.packed_off + p.out_off;
        hipLaunchKernelGGL(unet_out_dw_kernel, dim3(b + 1, d->out_chn), dim3(UNET_BLOCK), 0, s, dlogits, (const float*)(ws + t.y_off[last]),
                           p.hwp[0], b, st, st + b, hw0, grads + t.grad_w[UNET_TCONVS], grads + t.grad_b[UNET_TCONVS]);
        hipLaunchKernelGGL(unet_out_bwd_kernel, dim3((hw0 + UNET_BLOCK - 1) / UNET_BLOCK), dim3(UNET_BLOCK), 0, s, dlogits, Wo, p.out_kp,
                           d->out_chn, b, hw0, ws + t.g_off[last], p.hwp[0]);
    }
    for (int i = UNET_TCONVS - 1; i >= 0; --i) {
        const UNetConv& c = p.conv[i];
        const int l = c.level, hw = p.H[l] * p.W[l], hwp = p.hwp[l];
        float* G = ws + t.g_off[i];
        const float* y = ws + t.y_off[i];
        const float* st = ws + t.stat_off[i];
        float* dgamma = grads + t.grad_gamma[i];
        float* dbeta = grads + t.grad_beta[i];
        hipLaunchKernelGGL(unet_bn_sums_kernel, dim3(c.cout), dim3(UNET_BLOCK), 0, s, (const float*)G, y, hwp, hw, c.cout, st, dgamma, dbeta);
        hipLaunchKernelGGL(unet_bn_dy_kernel, dim3((hwp + UNET_BLOCK - 1) / UNET_BLOCK, c.cout), dim3(UNET_BLOCK), 0, s, G, y, hwp, hw, c.cout,
                           st, (const float*)dgamma, (const float*)dbeta);
        // weight (and bias) gradient
        {
            const int strip = t.strip[i], ld = hwp < strip ? hwp : strip;
            const long long mn = (long long)c.cout * c.kp;
            int slices = 0;
            for (int p0 = 0; p0 < hw; p0 += strip) {
                const int n = hw - p0 < strip ? hw - p0 : strip, n4 = unet_round(n, 4);
                unet_train_gather(t, i, input, hw0, ws, p0, n, s);
                GemmArgs g{};
                g.A = G + p0; g.B = col; g.C = part + (size_t)slices * mn;
                g.M = c.cout; g.N = c.kp; g.K = n4; g.lda = hwp; g.ldb = ld; g.ldc = c.kp;
                g.k_per_split = UNET_TRAIN_DW_SLICE;
                g.c_split_stride = mn;
                g.epi = GEMM_EPI_STORE;
                const int rc = gemm_launch(s, false, true, g);
                if (rc) return rc;
                slices += (n4 + UNET_TRAIN_DW_SLICE - 1) / UNET_TRAIN_DW_SLICE;
            }
            hipLaunchKernelGGL(unet_dw_reduce_kernel, dim3((unsigned)((mn + UNET_BLOCK - 1) / UNET_BLOCK)), dim3(UNET_BLOCK), 0, s,
                               (const float*)part, slices, c.cout, 9 * c.cin, c.kp, grads + t.grad_w[i], grads + t.grad_b[i]);
        }
        if (i == 0) break;
        // input gradient and reader backward
        const int j = unet_train_src(i), lj = p.conv[j].level;
        const int strip = t.strip_b[i], ldb = hwp < strip ? hwp : strip;
        UNetGatherArgs g{};
        g.src = G; g.src_ld = hwp;
        g.col = col; g.ld = ldb;
        g.cin = c.cout; g.kp = t.kpt[i];
        g.H = p.H[l]; g.W = p.W[l];
        g.relu = 0;
        for (int p0 = 0; p0 < hw; p0 += strip) {
            g.p0 = p0;
            g.n = hw - p0 < strip ? hw - p0 : strip;
            g.n4 = unet_round(g.n, 4);
            const dim3 grid((g.n4 + UNET_BLOCK - 1) / UNET_BLOCK, (c.cout + UNET_GATHER_CH - 1) / UNET_GATHER_CH + 1);
            hipLaunchKernelGGL(unet_gather_kernel<UNET_SRC_DIRECT>, grid, dim3(UNET_BLOCK), 0, s, g);
            int rc;
            if (c.src == UNET_SRC_DIRECT) {
                rc = unet_train_dgrad_rows(t, i, 0, c.cin, ws + t.g_off[j], ws, p0, g.n4, ldb, s);
            } else if (c.src == UNET_SRC_POOL) {
                rc = unet_train_dgrad_rows(t, i, 0, c.cin, Dt, ws, p0, g.n4, ldb, s);
            } else {
                rc = unet_train_dgrad_rows(t, i, 0, c.cskip, ws + t.g_off[unet_train_skip(i)], ws, p0, g.n4, ldb, s);
                if (!rc) rc = unet_train_dgrad_rows(t, i, c.cskip, c.cin - c.cskip, Dt, ws, p0, g.n4, ldb, s);
            }
            if (rc) return rc;
        }
        if (c.src == UNET_SRC_POOL) {
            const float* sj = ws + t.stat_off[j];
            const int Hs = p.H[lj], Ws = p.W[lj];
            hipLaunchKernelGGL(unet_pool_bwd_kernel, dim3((Hs * Ws + UNET_BLOCK - 1) / UNET_BLOCK, c.cin), dim3(UNET_BLOCK), 0, s,
                               (const float*)Dt, hwp, p.H[l], p.W[l], (const float*)(ws + t.y_off[j]), ws + t.g_off[j], p.hwp[lj], Hs, Ws, sj,
                               sj + p.conv[j].cout);
        } else if (c.src == UNET_SRC_UP) {
            const int Hd = p.H[lj], Wd = p.W[lj];
            const float sy = Hd > 1 ? (float)(Hd - 1) / (float)(2 * Hd - 1) : 0.f, sx = Wd > 1 ? (float)(Wd - 1) / (float)(2 * Wd - 1) : 0.f;
            hipLaunchKernelGGL(unet_up_bwd_kernel, dim3((Hd * Wd + UNET_BLOCK - 1) / UNET_BLOCK, c.cin - c.cskip), dim3(UNET_BLOCK), 0, s,
                               (const float*)Dt, hwp, p.W[l], ws + t.g_off[j], p.hwp[lj], Hd, Wd, (p.H[l] - 2 * Hd) / 2, (p.W[l] - 2 * Wd) / 2,
                               sy, sx);
        }
    }
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

}  // namespace
