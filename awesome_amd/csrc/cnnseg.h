// cnnseg.h - one training step of the convexity benchmark's segmentation network on the device: the reference's CNNNet
// (awesome/model/cnn_net.py: Conv3x3 C_in->W, LeakyReLU, depth x [Conv3x3 W->W, ReLU], Conv3x3 W->1, padding 1) trained with
// GradientPenaltyLoss(BCELoss) (awesome/measures/gradient_penalty_loss.py), whose penalty is a mean |d sum(s) / d input| and
// needs a double backward.  With f the logits, s = sigmoid(f) (or 1 - sigmoid(f)) and u = ds/df:
//
//   pass 1  forward             a_l = act_l(conv_l(a_{l-1}) + b_l), f                     (activations kept: they are the masks)
//   pass 2  backward of sum(s)  e_{L-1} = u, e_{l-1} = m_{l-1} . conv_l^T(e_l), g = conv_0^T(e_0)   -> penalty value
//   pass 3  tangent forward     q = dP/dg = coef sign(g) / count,  t_l = m_l . conv_l(t_{l-1}) (no bias), t_{L-1} at the output
//   pass 4  backward            d_f = dcrit/df + t_{L-1} du/df + dseg u,  d_{l-1} = m_{l-1} . conv_l^T(d_l)
//           dW_l = corr(a_{l-1}, d_l) + corr(t_{l-1}, e_l),   db_l = sum d_l
//
// (DESIGN.md section "CNNNet segmentation step" has the derivation.)  Maps are planar [C][H*W] fp32, batch 1.  Every convolution
// is one thread per pixel with all its output channels in registers; the weights are uniform loads.  The weight gradients are
// per-16x16-tile partial sums (slabs) added in tile order by one more kernel, every other reduction is a fixed-order tree over
// fixed blocks: the step is bit-reproducible.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int CNN_MAX_LAYERS = 5;     // depth <= 3 middle blocks
constexpr int CNN_MAX_IN = 8;
constexpr int CNN_WIDTH = 16;         // the compiled width (a template parameter of every kernel below)
constexpr int CNN_BLOCK = 256;
constexpr int CNN_TILE = 16;          // weight-gradient tile edge (256 pixels)
constexpr int CNN_STATS = 8;          // kept count, bce sum, |g| sums of the groups rgb / xy / feat, -, -, -

struct CnnConvArgs {
    const float* x0;      // input channels [0, c0)
    const float* x1;      // input channels [c0, ci)
    int c0, ci, co;
    const float* w;       // the layer's weight [co_layer][ci_layer][3][3] (torch layout); TRANSPOSED reads it as conv^T
    const float* b;       // bias or null
    int act;              // 0 none, 1 leaky relu (0.01), 2 relu
    const float* mask;    // null, or the activations whose sign is the mask: out *= (mask > 0 ? 1 : slope)
    float slope;
    float* out;
    int H, W;
};

// out[o][p] = sum_i sum_k w(o, i, k) x[i][p + d_k], zero padding.  Forward: w(o, i, k) = W[o][i][k]; transposed (the input gradient
// of a convolution): w(o, i, k) = W[i][o][8 - k].
template <int COMAX, bool TRANSPOSED>
__global__ void __launch_bounds__(CNN_BLOCK) cnn_conv_kernel(const CnnConvArgs a) {
    const int n = a.H * a.W;
    const int p = blockIdx.x * CNN_BLOCK + threadIdx.x;
    if (p >= n) return;
    const int y = p / a.W, x = p - y * a.W;
    float acc[COMAX];
#pragma unroll
    for (int o = 0; o < COMAX; ++o) acc[o] = 0.f;
    for (int i = 0; i < a.ci; ++i) {
        const float* __restrict__ xi = i < a.c0 ? a.x0 + (size_t)i * n : a.x1 + (size_t)(i - a.c0) * n;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
            const float v = (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) ? xi[yy * a.W + xx] : 0.f;
#pragma unroll
            for (int o = 0; o < COMAX; ++o) {
                if (o < a.co) {
                    const float w = TRANSPOSED ? a.w[(i * a.co + o) * 9 + (8 - k)] : a.w[(o * a.ci + i) * 9 + k];
                    acc[o] = fmaf(w, v, acc[o]);
                }
            }
        }
    }
#pragma unroll
    for (int o = 0; o < COMAX; ++o) {
        if (o < a.co) {
            float z = acc[o];
            if (a.b) z = z + a.b[o];
            if (a.act == 1) z = z > 0.f ? z : z * 0.01f;
            else if (a.act == 2) z = z <= 0.f ? 0.f : z;   // (torch's relu keeps a NaN)
            if (a.mask) z = a.mask[(size_t)o * n + p] > 0.f ? z : z * a.slope;
            a.out[(size_t)o * n + p] = z;
        }
    }
}

struct CnnPointArgs {
    const float* f;        // logits [n]
    const float* target;   // [n] or null
    float* seg;            // s [n]
    float* u;              // ds/df [n]
    float* g;              // pass 2's input gradient [C_in][n]; the stats kernel overwrites it with q
    float* stats_part;     // [blocks][CNN_STATS]
    float* f_out;          // the caller's copies of f and s, or null
    float* seg_out;
    int n, inversion, use_noneclass, cin, penalty;
    float noneclass;
    int group[CNN_MAX_IN];        // per input channel: 0 rgb, 1 xy, 2 feat, -1 no term
    float qscale[CNN_MAX_IN];     // g coef / count of the channel's group (0 = no term)
};

__device__ __forceinline__ float cnn_sigmoid(float f) { return 1.f / (1.f + expf(-f)); }

// s and u = ds/df as torch's sigmoid backward computes them ((1 - y) y, negated through 1 - y)
__global__ void __launch_bounds__(CNN_BLOCK) cnn_head_kernel(const CnnPointArgs a) {
    const int p = blockIdx.x * CNN_BLOCK + threadIdx.x;
    if (p >= a.n) return;
    const float sg = cnn_sigmoid(a.f[p]);
    const float d = (1.f - sg) * sg;
    const float s = a.inversion ? 1.f - sg : sg;
    a.seg[p] = s;
    a.u[p] = a.inversion ? -d : d;
    if (a.f_out) a.f_out[p] = a.f[p];
    if (a.seg_out) a.seg_out[p] = s;
}

// fixed-order block sum over CNN_BLOCK threads (tree in LDS)
__device__ __forceinline__ float cnn_block_sum(float v, float* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = CNN_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ float cnn_clamp_log(float l) { return l < -100.f ? -100.f : l; }   // std::max(l, -100): NaN stays NaN

__device__ __forceinline__ float cnn_bce(float s, float t) {   // torch's binary_cross_entropy, log clamped at -100
    const float li = cnn_clamp_log(logf(s)), l1 = cnn_clamp_log(log1pf(-s));
    return (t - 1.f) * l1 - t * li;
}

// per block: kept count, BCE sum and the |g| sums per group; g -> q = qscale sign(g) in place
__global__ void __launch_bounds__(CNN_BLOCK) cnn_stats_kernel(const CnnPointArgs a) {
    __shared__ float red[CNN_BLOCK];
    const int p = blockIdx.x * CNN_BLOCK + threadIdx.x;
    float kept = 0.f, bce = 0.f, g0 = 0.f, g1 = 0.f, g2 = 0.f;
    if (p < a.n) {
        if (a.target) {
            const float t = a.target[p];
            if (!a.use_noneclass || t != a.noneclass) {
                kept = 1.f;
                bce = cnn_bce(a.seg[p], t);
            }
        }
        if (a.penalty) {
            for (int c = 0; c < a.cin; ++c) {
                float* gp = a.g + (size_t)c * a.n + p;
                const float v = *gp;
                const int grp = a.group[c];
                const float av = fabsf(v);
                if (grp == 0) g0 = g0 + av;
                else if (grp == 1) g1 = g1 + av;
                else if (grp == 2) g2 = g2 + av;
                const float sgn = v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f);   // torch: sign(0) = 0 in the backward of abs
                *gp = grp >= 0 ? a.qscale[c] * sgn : 0.f;
            }
        }
    }
    float* out = a.stats_part + (size_t)blockIdx.x * CNN_STATS;
    const float v0 = cnn_block_sum(kept, red), v1 = cnn_block_sum(bce, red);
    const float v2 = cnn_block_sum(g0, red), v3 = cnn_block_sum(g1, red), v4 = cnn_block_sum(g2, red);
    if (threadIdx.x == 0) {
        out[0] = v0; out[1] = v1; out[2] = v2; out[3] = v3; out[4] = v4;
        out[5] = 0.f; out[6] = 0.f; out[7] = 0.f;
    }
}

struct CnnLossArgs {
    const float* stats_part;
    int blocks;
    float* stats;          // [CNN_STATS]: the sums, then [5] = the data seed's scale g / kept
    float* loss_out;       // [1] g (bce / kept + sum_grp coef_grp |g|_grp / count_grp)
    float* loss_user;      // the caller's copy, or null
    float gfac;
    float pen_scale[3];    // coef / count per group (0 = no term)
};

// one block: the stats partials in block order, then the loss value
__global__ void __launch_bounds__(CNN_BLOCK) cnn_loss_kernel(const CnnLossArgs a) {
    __shared__ float red[CNN_BLOCK];
    float tot[5];
    for (int j = 0; j < 5; ++j) {
        float acc = 0.f;
        for (int b = threadIdx.x; b < a.blocks; b += CNN_BLOCK) acc = acc + a.stats_part[(size_t)b * CNN_STATS + j];
        tot[j] = cnn_block_sum(acc, red);
    }
    if (threadIdx.x == 0) {
        for (int j = 0; j < 5; ++j) a.stats[j] = tot[j];
        float l = tot[1] / tot[0];
        for (int grp = 0; grp < 3; ++grp)
            if (a.pen_scale[grp] != 0.f) l = l + a.pen_scale[grp] * tot[2 + grp];
        a.stats[5] = a.gfac / tot[0];
        a.loss_out[0] = a.gfac * l;
        if (a.loss_user) a.loss_user[0] = a.gfac * l;
    }
}

struct CnnSeedArgs {
    const float* seg;
    const float* f;
    const float* target;
    const float* stats;    // [5] = g / kept
    const float* tout;     // t_{L-1} [n] or null (no penalty)
    const float* dseg;     // [n] or null
    float* df;
    int n, inversion, use_noneclass;
    float noneclass;
};

// d loss / d f at every pixel: the data term (torch's BCE backward through 1 - y and the sigmoid), the penalty's second-order term
// t_{L-1} du/df and the prior share's dseg u
__global__ void __launch_bounds__(CNN_BLOCK) cnn_seed_kernel(const CnnSeedArgs a) {
    const int p = blockIdx.x * CNN_BLOCK + threadIdx.x;
    if (p >= a.n) return;
    const float s = a.seg[p], t = a.target[p];
    const float sg = cnn_sigmoid(a.f[p]);
    const float d = (1.f - sg) * sg;
    float gs = 0.f;                                   // d loss / d s
    if (!a.use_noneclass || t != a.noneclass) gs = a.stats[5] * (s - t) / fmaxf((1.f - s) * s, 1e-12f);
    if (a.dseg) gs = gs + a.dseg[p];
    float df = (a.inversion ? -gs : gs) * d;
    if (a.tout) {
        const float du = d * (1.f - 2.f * sg);        // d/df of (1 - y) y
        df = df + a.tout[p] * (a.inversion ? -du : du);
    }
    a.df[p] = df;
}

struct CnnWgradArgs {
    const float* x0; const float* x1; int c0;   // the layer's input activations (forward term)
    const float* d;                             // the layer's output gradient (forward term) [co][n]
    const float* t;                             // tangent input [ci][n] (penalty term) or null
    const float* e;                             // pass 2's map at the layer's output [co][n]
    int ci, co, H, W, tiles_x;
    float* slab;                                // [tiles][P]; this layer's columns start at w_off (weights) / b_off (bias)
    int P, w_off, b_off;
};

// One 16x16 tile per block: thread = (o, i) pair, all 9 taps; dW[o][i][k] += sum_p D[o][p] X[i][p + d_k] over the tile's pixels in
// row-major order, the forward term then the penalty term; threads o < co also sum db[o].
template <int CMAX>
__global__ void __launch_bounds__(CNN_BLOCK) cnn_wgrad_kernel(const CnnWgradArgs a) {
    constexpr int E = CNN_TILE + 2;
    __shared__ float xs[CMAX][E * E];
    __shared__ float ds[CMAX][CNN_TILE * CNN_TILE];
    const int n = a.H * a.W;
    const int ty0 = (blockIdx.x / a.tiles_x) * CNN_TILE, tx0 = (blockIdx.x % a.tiles_x) * CNN_TILE;
    const int pair = threadIdx.x, o = pair / (a.ci > 0 ? a.ci : 1), i = pair - o * a.ci;
    const bool active = pair < a.ci * a.co;
    float acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.f;
    float bacc = 0.f;
    for (int phase = 0; phase < 2; ++phase) {
        if (phase == 1 && a.t == nullptr) break;
        const float* dsrc = phase == 0 ? a.d : a.e;
        __syncthreads();
        for (int j = threadIdx.x; j < a.ci * E * E; j += CNN_BLOCK) {
            const int c = j / (E * E), r = j - c * E * E, yy = ty0 + r / E - 1, xx = tx0 + r % E - 1;
            float v = 0.f;
            if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) {
                const size_t q = (size_t)yy * a.W + xx;
                v = phase == 1 ? a.t[(size_t)c * n + q] : (c < a.c0 ? a.x0[(size_t)c * n + q] : a.x1[(size_t)(c - a.c0) * n + q]);
            }
            xs[c][r] = v;
        }
        for (int j = threadIdx.x; j < a.co * CNN_TILE * CNN_TILE; j += CNN_BLOCK) {
            const int c = j / (CNN_TILE * CNN_TILE), r = j - c * CNN_TILE * CNN_TILE, yy = ty0 + r / CNN_TILE, xx = tx0 + r % CNN_TILE;
            ds[c][r] = (yy < a.H && xx < a.W) ? dsrc[(size_t)c * n + (size_t)yy * a.W + xx] : 0.f;
        }
        __syncthreads();
        if (active) {
            for (int py = 0; py < CNN_TILE; ++py) {
                for (int px = 0; px < CNN_TILE; ++px) {
                    const float dv = ds[o][py * CNN_TILE + px];
#pragma unroll
                    for (int k = 0; k < 9; ++k) acc[k] = fmaf(dv, xs[i][(py + k / 3) * E + px + k % 3], acc[k]);
                }
            }
        }
        if (phase == 0 && (int)threadIdx.x < a.co) {
            for (int r = 0; r < CNN_TILE * CNN_TILE; ++r) bacc = bacc + ds[threadIdx.x][r];
        }
    }
    float* row = a.slab + (size_t)blockIdx.x * a.P;
    if (active) {
#pragma unroll
        for (int k = 0; k < 9; ++k) row[a.w_off + pair * 9 + k] = acc[k];
    }
    if ((int)threadIdx.x < a.co) row[a.b_off + threadIdx.x] = bacc;
}

// grads[j] = sum over tiles in tile order; flags[block] = any non-finite gradient in this block
__global__ void __launch_bounds__(CNN_BLOCK) cnn_grad_reduce_kernel(const float* __restrict__ slab, int tiles, int P,
                                                                    float* __restrict__ grads, int32_t* __restrict__ flags) {
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    const int j = blockIdx.x * CNN_BLOCK + threadIdx.x;
    if (j < P) {
        float acc = 0.f;
        for (int t = 0; t < tiles; ++t) acc = acc + slab[(size_t)t * P + j];
        grads[j] = acc;
        if (!isfinite(acc)) atomicOr(&bad, 1);   // (an LDS flag: order-free)
    }
    __syncthreads();
    if (threadIdx.x == 0) flags[blockIdx.x] = bad;
}

// one block: a non-finite loss or gradient zeroes the gradient and sets *status (the optimizer then steps on a zero gradient)
__global__ void __launch_bounds__(CNN_BLOCK) cnn_finalize_kernel(const int32_t* __restrict__ flags, int nflags,
                                                                 const float* __restrict__ loss, float* __restrict__ grads, int P,
                                                                 int32_t* __restrict__ status, float* __restrict__ loss_user) {
    __shared__ int bad;
    if (threadIdx.x == 0) bad = isfinite(loss[0]) ? 0 : 1;
    __syncthreads();
    for (int b = threadIdx.x; b < nflags; b += CNN_BLOCK)
        if (flags[b]) atomicOr(&bad, 1);
    __syncthreads();
    if (bad)
        for (int j = threadIdx.x; j < P; j += CNN_BLOCK) grads[j] = 0.f;
    if (threadIdx.x == 0) {
        status[0] = bad;
        if (loss_user) loss_user[0] = loss[0];
    }
}

}  // namespace
