// unet.h - the evaluation-mode forward pass of the reference's UNet (awesome/model/unet.py: InConv, 4 x Down, 4 x Up with bilinear
// upsampling, OutConv; channel widths base (1, 2, 4, 8, 8) going down and base (4, 2, 1, 1) coming up) on one image, fp32.
//
// Evaluation-mode BatchNorm is an affine map, so every Conv2d(3 x 3, padding 1) + BatchNorm2d pair is ONE matrix
//     Wp [C_out][Kp],  Kp = 9 C_in + 1 rounded up to a multiple of 16:   Wp[o][(i, tap)] = w[o][i][tap] scale[o],
//     Wp[o][9 C_in] = (b[o] - running_mean[o]) scale[o] + beta[o],  scale = gamma / sqrt(running_var + eps),  zeros behind
// (unet_pack_kernel, on the device, once per set of weights), and the convolution over planar maps [C][H W] is the product
//     Out [C_out][strip] = Wp . Col [Kp][strip]
// of gemm.h (gemm_rm; gemm_rm_splitk where the output has few tiles and the contraction is long), strip by strip over the pixels.
// The new kernels are what stands around those products:
//
//   unet_pack_kernel    the fold above (OutConv the same way without a BatchNorm: [out_chn][C + 1 -> 16 k]).
//   unet_gather_kernel  a strip of Col: row (i, tap) = input channel i shifted by the tap, zero outside the image; one row of ones
//                       (the bias column's partner); zero rows up to Kp.  It reads its input THROUGH what precedes the convolution -
//                       nothing, a 2 x 2 max-pool (floor mode), or the concatenation [skip map | bilinear x2 upsampling of the deeper
//                       map, align_corners, zero-padded to the skip map's size] - so none of those is ever written to memory.
//                       A thread owns one pixel of the strip and 8 channels: neighbouring lanes store neighbouring floats of a row.
//                       The tap loop is unrolled around the channel loop, index arithmetic once per tap; no per-lane array.
//   unet_out_kernel     the 1 x 1 OutConv, one thread per pixel.
//
// Convolution outputs are stored BEFORE their ReLU and every reader applies max(0, .) to each value it loads (per tap, before the
// pool's max and before interpolating); only the network input is read as it is.  That saves a pass per layer and leaves gemm.h
// without a new epilogue.  Every operand base is 16-byte aligned and every leading dimension a multiple of 4 floats (planes are
// padded to 4 pixels, strips start at multiples of 128), so the products run on gemm.h's 16-byte-load kernels.  Whether a product is
// split depends on its shape only: two calls give the same bits.
#pragma once
#include "gemm.h"

namespace {

constexpr int UNET_CONVS = 19;            // 18 3x3 convolutions (each with a BatchNorm) + OutConv
constexpr int UNET_LEVELS = 5;
constexpr int UNET_STRIP = 2048;          // default strip (pixels): Col of the widest layer (Kp 9232 at base 64) is 76 MB
constexpr int UNET_BLOCK = 256;
constexpr int UNET_GATHER_CH = 8;         // channels per gather block
constexpr int UNET_MAX_SIDE = 4096;
constexpr int UNET_SPLITK_TILES = 64;     // a product with at most this many 128 x 128 output tiles ...
constexpr int UNET_SPLITK_MIN_K = 2048;   // ... and a contraction at least this long is split (gemm_rm_splitk)

enum { UNET_SRC_DIRECT = 0, UNET_SRC_POOL = 1, UNET_SRC_UP = 2 };

inline int unet_round(int v, int m) { return (v + m - 1) / m * m; }
inline int unet_kp(int cin) { return unet_round(9 * cin + 1, 16); }

struct UNetConv {          // one 3x3 convolution of the network
    int cin, cout, level;  // output resolution: level 0 = the image, level l = l max-pools below
    int src;               // UNET_SRC_*
    int cskip;             // UP: channels of the skip map (the first cskip input channels)
    int kp;
    long long w_off;       // floats into the packed weights
};

struct UNetPlan {
    UNetConv conv[UNET_CONVS - 1];
    int H[UNET_LEVELS], W[UNET_LEVELS], hwp[UNET_LEVELS], chn[UNET_LEVELS];   // per level: size, plane stride (floats), widest map
    int strip;
    long long out_off, packed_floats;      // OutConv's matrix [out_chn][out_kp]
    int out_kp;
    // workspace (floats from its base): per level two maps [chn][hwp] (`mid`: first convolution of a block; `x`: the block's output -
    // the skip map on the way down, overwritten by the Up block's output once its first convolution has read it), Col, split-K parts
    long long mid_off[UNET_LEVELS], x_off[UNET_LEVELS], col_off, part_off, bytes;
};

inline bool unet_splitk(int M, int n4, int K, bool whole_plane) {
    const int tiles = ((M + GM_BM - 1) / GM_BM) * ((n4 + GM_BN - 1) / GM_BN);
    return whole_plane && tiles <= UNET_SPLITK_TILES && K >= UNET_SPLITK_MIN_K;
}

// (the descriptor has passed unet_desc_rc)
inline UNetPlan unet_plan(const InrUNetDesc* d) {
    UNetPlan p{};
    const int b = d->base_width;
    const int down[UNET_LEVELS] = {b, 2 * b, 4 * b, 8 * b, 8 * b}, up[4] = {4 * b, 2 * b, b, b};
    p.strip = d->strip_points > 0 ? unet_round(d->strip_points, 128) : UNET_STRIP;
    for (int l = 0; l < UNET_LEVELS; ++l) {
        p.H[l] = l ? p.H[l - 1] / 2 : d->height;
        p.W[l] = l ? p.W[l - 1] / 2 : d->width;
        p.hwp[l] = unet_round(p.H[l] * p.W[l], 4);
        p.chn[l] = down[l];
    }
    int n = 0;
    long long off = 0;
    auto add = [&](int cin, int cout, int level, int src, int cskip) {
        UNetConv& c = p.conv[n++];
        c.cin = cin; c.cout = cout; c.level = level; c.src = src; c.cskip = cskip;
        c.kp = unet_kp(cin);
        c.w_off = off;
        off += (long long)cout * c.kp;
    };
    add(d->in_chn, b, 0, UNET_SRC_DIRECT, 0);
    add(b, b, 0, UNET_SRC_DIRECT, 0);
    for (int l = 1; l < UNET_LEVELS; ++l) {
        add(down[l - 1], down[l], l, UNET_SRC_POOL, 0);
        add(down[l], down[l], l, UNET_SRC_DIRECT, 0);
    }
    int deep = down[4];
    for (int u = 0; u < 4; ++u) {
        const int l = 3 - u;
        add(down[l] + deep, up[u], l, UNET_SRC_UP, down[l]);
        add(up[u], up[u], l, UNET_SRC_DIRECT, 0);
        deep = up[u];
    }
    p.out_kp = unet_round(b + 1, 16);
    p.out_off = off;
    p.packed_floats = off + (long long)d->out_chn * p.out_kp;

    long long w = 0, col = 0, part = 0;
    auto take = [&](long long floats) { const long long at = w; w += (floats * 4 + 255) / 256 * 64; return at; };
    for (int l = 0; l < UNET_LEVELS; ++l) {
        p.mid_off[l] = take((long long)p.chn[l] * p.hwp[l]);
        p.x_off[l] = take((long long)p.chn[l] * p.hwp[l]);
    }
    for (int i = 0; i < UNET_CONVS - 1; ++i) {
        const UNetConv& c = p.conv[i];
        const int ld = p.hwp[c.level] < p.strip ? p.hwp[c.level] : p.strip;
        if ((long long)c.kp * ld > col) col = (long long)c.kp * ld;
        if (unet_splitk(c.cout, p.hwp[c.level], c.kp, p.hwp[c.level] <= p.strip)) {
            const long long need = (long long)GEMM_SPLITK_MAX * c.cout * p.hwp[c.level];
            if (need > part) part = need;
        }
    }
    p.col_off = take(col);
    p.part_off = take(part > 0 ? part : 1);
    p.bytes = w * 4;
    return p;
}

// INR_OK, or why the descriptor is refused
inline int unet_desc_rc(const InrUNetDesc* d) {
    if (!d) return INR_EINVAL;
    if (d->height < 16 || d->width < 16 || d->in_chn <= 0 || d->out_chn <= 0 || d->base_width <= 0 || d->strip_points < 0) return INR_EINVAL;
    if (!(d->bn_eps >= 0.f)) return INR_EINVAL;
    if ((d->base_width & 3) || d->base_width > 64 || d->out_chn > 8 || d->in_chn > 1024) return INR_EUNSUPPORTED;
    if (d->height > UNET_MAX_SIDE || d->width > UNET_MAX_SIDE || d->strip_points > (1 << 20)) return INR_EUNSUPPORTED;
    return INR_OK;
}

// ---- the fold ------------------------------------------------------------------------------------------------------------------------
// Wp [cout][kp] from w [cout][k] (k = 9 cin, or cin for OutConv), b [cout] and, with gamma != null, the BatchNorm's four vectors
__global__ __launch_bounds__(UNET_BLOCK) void unet_pack_kernel(const float* __restrict__ w, const float* __restrict__ b,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               const float* __restrict__ mean, const float* __restrict__ var, float eps,
                                                               int cout, int k, int kp, float* __restrict__ Wp) {
    const long long e = (long long)blockIdx.x * UNET_BLOCK + threadIdx.x;
    if (e >= (long long)cout * kp) return;
    const int o = (int)(e / kp), c = (int)(e - (long long)o * kp);
    float scale = 1.f, shift = 0.f, mu = 0.f;
    if (gamma) {
        scale = gamma[o] / sqrtf(var[o] + eps);
        shift = beta[o];
        mu = mean[o];
    }
    float v = 0.f;
    if (c < k) v = w[(size_t)o * k + c] * scale;
    else if (c == k) v = (b[o] - mu) * scale + shift;
    Wp[e] = v;
}

// ---- the column matrix -----------------------------------------------------------------------------------------------------------------
struct UNetGatherArgs {
    const float* src;      // DIRECT: [cin][src_ld] at H x W;  POOL: [cin][src_ld] at Hs x Ws (H = Hs / 2, W = Ws / 2);  UP: the skip map
    const float* deep;     // UP: [cin - cskip][deep_ld] at Hd x Wd
    float* col;            // [kp][ld]
    int src_ld, deep_ld, ld;
    int cin, cskip, kp;
    int H, W;              // the convolution's resolution
    int Ws;                // POOL: row length of the source
    int Hd, Wd, py0, px0;  // UP: size of the deeper map; rows / columns of zero padding in front of its upsampled image
    float sy, sx;          // UP: (Hd - 1) / (2 Hd - 1), (Wd - 1) / (2 Wd - 1)  (0 for a single row / column)
    int p0, n, n4;         // the strip: pixels [p0, p0 + n), columns [n, n4) of Col are zero
    int relu;              // the source holds pre-activation values (everything but the network input)
};

template <int SRC>
__global__ __launch_bounds__(UNET_BLOCK) void unet_gather_kernel(const UNetGatherArgs a) {
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
                const float v = a.relu ? fmaxf(*s, 0.f) : *s;
                *out = in ? v : 0.f;
            }
        } else if (SRC == UNET_SRC_POOL) {                 // (floor mode: 2 yc + 1 <= Hs - 1)
            const float* s = a.src + (size_t)c0 * a.src_ld + (2 * yc) * a.Ws + 2 * xc;
            for (int c = c0; c < c1; ++c, s += a.src_ld, out += (size_t)9 * a.ld) {
                const float v = fmaxf(fmaxf(fmaxf(s[0], 0.f), fmaxf(s[1], 0.f)), fmaxf(fmaxf(s[a.Ws], 0.f), fmaxf(s[a.Ws + 1], 0.f)));
                *out = in ? v : 0.f;
            }
        } else {
            // the upsampled map's pixel (uy, ux) = (yy - py0, xx - px0), zero outside 2 Hd x 2 Wd; torch's align_corners rule:
            // source coordinate = destination index * (in - 1) / (out - 1), upper neighbour clamped to the last row / column
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
                    v = in ? fmaxf(a.src[(size_t)c * a.src_ld + os], 0.f) : 0.f;
                } else {
                    const float* s = a.deep + (size_t)(c - a.cskip) * a.deep_ld;
                    const float v00 = fmaxf(s[o00], 0.f), v01 = fmaxf(s[o01], 0.f), v10 = fmaxf(s[o10], 0.f), v11 = fmaxf(s[o11], 0.f);
                    v = inu ? hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11) : 0.f;
                }
                *out = v;
            }
        }
    }
}

// ---- OutConv: logits [oc][hw] = Wo [oc][kp] (relu(x) | 1) ------------------------------------------------------------------------------
__global__ __launch_bounds__(UNET_BLOCK) void unet_out_kernel(const float* __restrict__ x, int x_ld, int cin, const float* __restrict__ Wo,
                                                              int kp, int oc, int hw, float* __restrict__ logits) {
    const int p = blockIdx.x * UNET_BLOCK + threadIdx.x;
    if (p >= hw) return;
    for (int o = 0; o < oc; ++o) {
        const float* w = Wo + (size_t)o * kp;
        float acc = w[cin];
        for (int c = 0; c < cin; ++c) acc = fmaf(w[c], fmaxf(x[(size_t)c * x_ld + p], 0.f), acc);
        logits[(size_t)o * hw + p] = acc;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
// conv_w / conv_b: 19 device pointers in state_dict order (inc, down1..4, up1..4: two each; outc); bn_*: the 18 BatchNorms behind them
inline int unet_pack(const InrUNetDesc* d, const UNetPlan& p, const float* const* conv_w, const float* const* conv_b,
                     const float* const* gamma, const float* const* beta, const float* const* mean, const float* const* var, float* packed,
                     hipStream_t s) {
    for (int i = 0; i < UNET_CONVS - 1; ++i) {
        const UNetConv& c = p.conv[i];
        const long long n = (long long)c.cout * c.kp;
        hipLaunchKernelGGL(unet_pack_kernel, dim3((unsigned)((n + UNET_BLOCK - 1) / UNET_BLOCK)), dim3(UNET_BLOCK), 0, s, conv_w[i], conv_b[i],
                           gamma[i], beta[i], mean[i], var[i], d->bn_eps, c.cout, 9 * c.cin, c.kp, packed + c.w_off);
    }
    const long long n = (long long)d->out_chn * p.out_kp;
    hipLaunchKernelGGL(unet_pack_kernel, dim3((unsigned)((n + UNET_BLOCK - 1) / UNET_BLOCK)), dim3(UNET_BLOCK), 0, s, conv_w[UNET_CONVS - 1],
                       conv_b[UNET_CONVS - 1], (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr,
                       0.f, d->out_chn, d->base_width, p.out_kp, packed + p.out_off);
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

inline int unet_forward(const InrUNetDesc* d, const UNetPlan& p, const float* packed, const float* input, float* logits, float* ws,
                        hipStream_t s) {
    float* col = ws + p.col_off;
    float* part = ws + p.part_off;
    const int hw0 = d->height * d->width;
    for (int i = 0; i < UNET_CONVS - 1; ++i) {
        const UNetConv& c = p.conv[i];
        const int l = c.level, hw = p.H[l] * p.W[l], hwp = p.hwp[l];
        const bool first_of_block = (i & 1) == 0;
        float* dst = ws + (first_of_block ? p.mid_off[l] : p.x_off[l]);
        UNetGatherArgs g{};
        g.col = col;
        g.cin = c.cin; g.cskip = c.cskip; g.kp = c.kp;
        g.H = p.H[l]; g.W = p.W[l];
        g.relu = i > 0;
        if (i == 0) {
            g.src = input; g.src_ld = hw0;
        } else if (c.src == UNET_SRC_DIRECT) {             // the second convolution of a block reads the first one's output
            g.src = ws + p.mid_off[l]; g.src_ld = hwp;
        } else if (c.src == UNET_SRC_POOL) {
            g.src = ws + p.x_off[l - 1]; g.src_ld = p.hwp[l - 1]; g.Ws = p.W[l - 1];
        } else {
            g.src = ws + p.x_off[l]; g.src_ld = hwp;
            g.deep = ws + p.x_off[l + 1]; g.deep_ld = p.hwp[l + 1];
            g.Hd = p.H[l + 1]; g.Wd = p.W[l + 1];
            g.py0 = (g.H - 2 * g.Hd) / 2; g.px0 = (g.W - 2 * g.Wd) / 2;
            g.sy = g.Hd > 1 ? (float)(g.Hd - 1) / (float)(2 * g.Hd - 1) : 0.f;
            g.sx = g.Wd > 1 ? (float)(g.Wd - 1) / (float)(2 * g.Wd - 1) : 0.f;
        }
        g.ld = hwp < p.strip ? hwp : p.strip;
        const int groups = (c.cin + UNET_GATHER_CH - 1) / UNET_GATHER_CH;
        for (int p0 = 0; p0 < hw; p0 += p.strip) {
            g.p0 = p0;
            g.n = hw - p0 < p.strip ? hw - p0 : p.strip;
            g.n4 = unet_round(g.n, 4);                     // (<= ld, and p0 + n4 <= hwp: the plane's padding takes the extra columns)
            const dim3 grid((g.n4 + UNET_BLOCK - 1) / UNET_BLOCK, groups + 1);
            if (c.src == UNET_SRC_DIRECT) hipLaunchKernelGGL(unet_gather_kernel<UNET_SRC_DIRECT>, grid, dim3(UNET_BLOCK), 0, s, g);
            else if (c.src == UNET_SRC_POOL) hipLaunchKernelGGL(unet_gather_kernel<UNET_SRC_POOL>, grid, dim3(UNET_BLOCK), 0, s, g);
            else hipLaunchKernelGGL(unet_gather_kernel<UNET_SRC_UP>, grid, dim3(UNET_BLOCK), 0, s, g);
            int rc;
            if (unet_splitk(c.cout, hwp, c.kp, hwp <= p.strip))   // one strip = the whole plane: dst is dense [cout][n4 = hwp]
                rc = gemm_rm_splitk(s, false, false, c.cout, g.n4, c.kp, packed + c.w_off, c.kp, col, g.ld, dst, part);
            else
                rc = gemm_rm(s, false, false, c.cout, g.n4, c.kp, packed + c.w_off, c.kp, col, g.ld, dst + p0, hwp);
            if (rc) return rc;
        }
    }
    hipLaunchKernelGGL(unet_out_kernel, dim3((hw0 + UNET_BLOCK - 1) / UNET_BLOCK), dim3(UNET_BLOCK), 0, s, (const float*)(ws + p.x_off[0]),
                       p.hwp[0], d->base_width, packed + p.out_off, p.out_kp, d->out_chn, hw0, logits);
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

}  // namespace
