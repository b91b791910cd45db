// fcseg.h - one training step of the convexity benchmark's fully connected segmentation network on the device: the reference's
// FCNet (awesome/model/fc_net.py: Linear(F, 16), ReLU, depth x [Linear(16, 16), ReLU], Linear(16, 1)) on pixel rows (n, F), trained
// with a plain mean BCELoss on its first data_count rows, s = sigmoid(f) or 1 - sigmoid(f).
//
//   fc_rows_kernel   one row per lane: the forward through every layer with the activations in registers (all weights, < 1000
//                    floats, staged once per block in LDS and read as broadcasts), the BCE term, d loss / d f, and the backward
//                    delta_{l-1} = mask_{l-1} . W_l^T delta_l down to the first layer.  The weight gradients dW_l = sum_rows delta_l^T z_{l-1}
//                    contract over rows: the wave's 64 rows of delta_l and z_{l-1} go through LDS (row-major, stride 17) into the A / B
//                    operands of v_mfma_f32_16x16x4_f32 (4 rows per instruction, 16 instructions per layer and chunk), which sums
//                    over the lanes; the bias gradients sum_rows delta_l ride on a second accumulator tile whose B operand is a one in
//                    column l.  A block adds its 4 waves' tiles in wave order and writes one slab row [P + 1] (column P: its BCE sum).
//   fc_reduce_kernel one block: the slab rows in a fixed order -> grads, the loss; a non-finite loss or gradient zeroes grads and
//                    sets the status word.
//
// Blocks walk the rows in chunks of FC_BLOCK with a fixed stride, every sum has a fixed order, nothing is atomic in floats: two calls
// give the same bits.  (DESIGN.md section "FCNet segmentation step".)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int FC_WIDTH = 16;          // the compiled width: one MFMA tile
constexpr int FC_MAX_IN = 8;
constexpr int FC_MAX_DEPTH = 3;
constexpr int FC_MAX_LAYERS = FC_MAX_DEPTH + 2;
constexpr int FC_BLOCK = 256;
constexpr int FC_WAVES = FC_BLOCK / 64;
constexpr int FC_MAX_BLOCKS = 1024;   // slab rows: more rows than FC_BLOCK * FC_MAX_BLOCKS are walked with a grid stride
constexpr int FC_TS = FC_WIDTH + 1;   // row stride of the transpose buffers (floats)
constexpr int FC_REDUCE_BLOCK = 1024; // >= the largest parameter count + 1 (977 + 1)

typedef float fc_f32x4 __attribute__((ext_vector_type(4)));

struct FcArgs {
    const float* w[FC_MAX_LAYERS];    // torch Linear weights [out][in]
    const float* b[FC_MAX_LAYERS];
    const float* image;               // [n][ic]
    const float* feat;                // [n][F - ic] (null when ic == F)
    const float* target;              // [count] or null (no loss)
    const float* dseg;                // [n] or null
    float* logits;                    // [n] or null
    float* seg;                       // [n] or null
    float* slab;                      // [blocks][stride]; column P = the block's BCE sum
    long long n, count;               // rows; rows of the data term (the first `count`)
    int F, ic, inversion, P, stride;
    float seed_scale;                 // g / count
};

__device__ __forceinline__ float fc_sigmoid(float f) { return 1.f / (1.f + expf(-f)); }
__device__ __forceinline__ float fc_clamp_log(float l) { return l < -100.f ? -100.f : l; }   // std::max(l, -100): NaN stays NaN
__device__ __forceinline__ float fc_bce(float s, float t) {   // torch's binary_cross_entropy, log clamped at -100
    const float li = fc_clamp_log(logf(s)), l1 = fc_clamp_log(log1pf(-s));
    return (t - 1.f) * l1 - t * li;
}
__device__ __forceinline__ float fc_relu(float z) { return z <= 0.f ? 0.f : z; }   // (torch's relu keeps a NaN)

// LDS image of the weights: layer 0 zero-padded to [16][8], hidden layers [16][16], the output layer [16]; biases behind each
constexpr int FC_L0 = 0;                                         // W0p [16][8] | b0 [16]
constexpr int FC_LH = FC_WIDTH * FC_MAX_IN + FC_WIDTH;           // per hidden layer: W [16][16] | b [16]
constexpr int FC_LH_SIZE = FC_WIDTH * FC_WIDTH + FC_WIDTH;
template <int DEPTH> constexpr int fc_lout() { return FC_LH + DEPTH * FC_LH_SIZE; }   // w_out [16] | b_out | pad
template <int DEPTH> constexpr int fc_wfloats() { return fc_lout<DEPTH>() + FC_WIDTH + 4; }

// flat parameter offsets (parameters() order: w_0 | b_0 | w_1 | b_1 | ...)
__host__ __device__ __forceinline__ int fc_w_off(int F, int l) { return l == 0 ? 0 : (FC_WIDTH * F + FC_WIDTH) + (l - 1) * FC_LH_SIZE; }
__host__ __device__ __forceinline__ int fc_b_off(int F, int depth, int l) {
    return fc_w_off(F, l) + (l == 0 ? FC_WIDTH * F : (l == depth + 1 ? FC_WIDTH : FC_WIDTH * FC_WIDTH));
}

template <int DEPTH, bool BWD>
__global__ void __launch_bounds__(FC_BLOCK) fc_rows_kernel(const FcArgs a) {
    constexpr int L = DEPTH + 2;
    constexpr int WF = fc_wfloats<DEPTH>();
    constexpr int TBUF = FC_WAVES * 64 * FC_TS;                    // one transpose buffer, all waves
    constexpr int TILES = L + 1;                                   // dW tiles + the bias tile
    constexpr int SCR = BWD ? (2 * TBUF > FC_WAVES * TILES * 256 ? 2 * TBUF : FC_WAVES * TILES * 256) : FC_BLOCK;
    __shared__ __align__(16) float wl[WF];
    __shared__ __align__(16) float scr[SCR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int F = a.F;

    // ---- stage the weights ----
    for (int j = tid; j < FC_WIDTH * FC_MAX_IN; j += FC_BLOCK) {
        const int o = j / FC_MAX_IN, i = j - o * FC_MAX_IN;
        wl[FC_L0 + j] = i < F ? a.w[0][o * F + i] : 0.f;
    }
    if (tid < FC_WIDTH) wl[FC_L0 + FC_WIDTH * FC_MAX_IN + tid] = a.b[0][tid];
#pragma unroll
    for (int k = 0; k < DEPTH; ++k) {
        float* dst = wl + FC_LH + k * FC_LH_SIZE;
        for (int j = tid; j < FC_WIDTH * FC_WIDTH; j += FC_BLOCK) dst[j] = a.w[1 + k][j];
        if (tid < FC_WIDTH) dst[FC_WIDTH * FC_WIDTH + tid] = a.b[1 + k][tid];
    }
    if (tid < FC_WIDTH) wl[fc_lout<DEPTH>() + tid] = a.w[L - 1][tid];
    if (tid == 0) wl[fc_lout<DEPTH>() + FC_WIDTH] = a.b[L - 1][0];
    __syncthreads();

    fc_f32x4 acc[BWD ? TILES : 1];
#pragma unroll
    for (int t = 0; t < (BWD ? TILES : 1); ++t) acc[t] = fc_f32x4{0.f, 0.f, 0.f, 0.f};
    float bce_acc = 0.f;

    const long long chunks = (a.n + FC_BLOCK - 1) / FC_BLOCK;
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {   // (the same trip count for every thread of the block)
        const long long r = c * FC_BLOCK + tid;
        const bool live = r < a.n;
        float x[FC_MAX_IN];
#pragma unroll
        for (int i = 0; i < FC_MAX_IN; ++i) {
            float v = 0.f;
            if (live && i < F) v = i < a.ic ? a.image[(size_t)r * a.ic + i] : a.feat[(size_t)r * (F - a.ic) + (i - a.ic)];
            x[i] = v;
        }
        // ---- forward ----
        float z[DEPTH + 1][FC_WIDTH];
        {
            const float4* w4 = (const float4*)(wl + FC_L0);
            const float* b = wl + FC_L0 + FC_WIDTH * FC_MAX_IN;
#pragma unroll
            for (int o = 0; o < FC_WIDTH; ++o) {
                const float4 w0 = w4[o * 2], w1 = w4[o * 2 + 1];
                float s = b[o];
                s = fmaf(w0.x, x[0], s); s = fmaf(w0.y, x[1], s); s = fmaf(w0.z, x[2], s); s = fmaf(w0.w, x[3], s);
                s = fmaf(w1.x, x[4], s); s = fmaf(w1.y, x[5], s); s = fmaf(w1.z, x[6], s); s = fmaf(w1.w, x[7], s);
                z[0][o] = fc_relu(s);
            }
        }
#pragma unroll
        for (int k = 0; k < DEPTH; ++k) {
            const float4* w4 = (const float4*)(wl + FC_LH + k * FC_LH_SIZE);
            const float* b = wl + FC_LH + k * FC_LH_SIZE + FC_WIDTH * FC_WIDTH;
#pragma unroll
            for (int o = 0; o < FC_WIDTH; ++o) {
                float s = b[o];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 w = w4[o * 4 + q];
                    s = fmaf(w.x, z[k][4 * q], s); s = fmaf(w.y, z[k][4 * q + 1], s);
                    s = fmaf(w.z, z[k][4 * q + 2], s); s = fmaf(w.w, z[k][4 * q + 3], s);
                }
                z[k + 1][o] = fc_relu(s);
            }
        }
        float f = wl[fc_lout<DEPTH>() + FC_WIDTH];
        {
            const float4* w4 = (const float4*)(wl + fc_lout<DEPTH>());
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 w = w4[q];
                f = fmaf(w.x, z[DEPTH][4 * q], f); f = fmaf(w.y, z[DEPTH][4 * q + 1], f);
                f = fmaf(w.z, z[DEPTH][4 * q + 2], f); f = fmaf(w.w, z[DEPTH][4 * q + 3], f);
            }
        }
        const float sg = fc_sigmoid(f);
        const float s = a.inversion ? 1.f - sg : sg;
        if (live) {
            if (a.logits) a.logits[r] = f;
            if (a.seg) a.seg[r] = s;
        }
        const bool data = live && a.target != nullptr && r < a.count;
        float t = 0.f;
        if (data) {
            t = a.target[r];
            bce_acc = bce_acc + fc_bce(s, t);
        }
        if constexpr (BWD) {
            // ---- d loss / d f: torch's BCE backward through 1 - y and the sigmoid, plus the prior share's dseg ----
            const float dsig = (1.f - sg) * sg;
            float gs = 0.f;
            if (data) gs = a.seed_scale * (s - t) / fmaxf((1.f - s) * s, 1e-12f);
            if (live && a.dseg) gs = gs + a.dseg[r];
            const float df = live ? (a.inversion ? -gs : gs) * dsig : 0.f;

            float* ta = scr + wave * 64 * FC_TS;              // delta_l of the wave's 64 rows, [row][16]
            float* tb = scr + TBUF + wave * 64 * FC_TS;       // the layer's input, [row][16]
            const int mrow = lane >> 4, mcol = lane & 15;
            float d[FC_WIDTH];
#pragma unroll
            for (int o = 0; o < FC_WIDTH; ++o) d[o] = o == 0 ? df : 0.f;
#pragma unroll
            for (int l = L - 1; l >= 0; --l) {
                __syncthreads();                               // (the previous layer's reads are done)
#pragma unroll
                for (int o = 0; o < FC_WIDTH; ++o) {
                    ta[lane * FC_TS + o] = d[o];
                    tb[lane * FC_TS + o] = l == 0 ? (o < FC_MAX_IN ? x[o < FC_MAX_IN ? o : 0] : 0.f) : z[l > 0 ? l - 1 : 0][o];
                }
                __syncthreads();
                const float bsel = mcol == l ? 1.f : 0.f;
#pragma unroll
                for (int st = 0; st < 16; ++st) {
                    const float av = ta[(4 * st + mrow) * FC_TS + mcol];
                    const float bv = tb[(4 * st + mrow) * FC_TS + mcol];
                    acc[l] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[l], 0, 0, 0);
                    acc[L] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bsel, acc[L], 0, 0, 0);
                }
                if (l > 0) {                                   // delta_{l-1} = [z_{l-1} > 0] . W_l^T delta_l
                    float dp[FC_WIDTH];
                    if (l == L - 1) {
                        const float* w = wl + fc_lout<DEPTH>();
#pragma unroll
                        for (int i = 0; i < FC_WIDTH; ++i) dp[i] = w[i] * d[0];
                    } else {
                        const float4* w4 = (const float4*)(wl + FC_LH + (l - 1) * FC_LH_SIZE);
#pragma unroll
                        for (int i = 0; i < FC_WIDTH; ++i) dp[i] = 0.f;
#pragma unroll
                        for (int o = 0; o < FC_WIDTH; ++o) {
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                const float4 w = w4[o * 4 + q];
                                dp[4 * q] = fmaf(w.x, d[o], dp[4 * q]); dp[4 * q + 1] = fmaf(w.y, d[o], dp[4 * q + 1]);
                                dp[4 * q + 2] = fmaf(w.z, d[o], dp[4 * q + 2]); dp[4 * q + 3] = fmaf(w.w, d[o], dp[4 * q + 3]);
                            }
                        }
                    }
#pragma unroll
                    for (int i = 0; i < FC_WIDTH; ++i) d[i] = z[l > 0 ? l - 1 : 0][i] > 0.f ? dp[i] : 0.f;
                }
            }
        }
    }

    // ---- the block's slab row ----
    float* row = a.slab ? a.slab + (size_t)blockIdx.x * a.stride : nullptr;
    if constexpr (BWD) {
        __syncthreads();
        // C/D map of the 16x16 MFMA: register q of lane l is element [row 4 (l >> 4) + q][col l & 15]
#pragma unroll
        for (int t = 0; t < TILES; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) scr[(wave * TILES + t) * 256 + (4 * (lane >> 4) + q) * 16 + (lane & 15)] = acc[t][q];
        __syncthreads();
        const int o = tid >> 4, i = tid & 15;
#pragma unroll
        for (int t = 0; t < TILES; ++t) {
            float v = scr[t * 256 + tid];
#pragma unroll
            for (int w = 1; w < FC_WAVES; ++w) v = v + scr[(w * TILES + t) * 256 + tid];
            int j = -1;
            if (t == 0) { if (i < F) j = o * F + i; }
            else if (t < L - 1) j = fc_w_off(F, t) + tid;
            else if (t == L - 1) { if (o == 0) j = fc_w_off(F, t) + i; }
            else if (i < L && (i < L - 1 || o == 0)) j = fc_b_off(F, DEPTH, i) + o;     // the bias tile: [o][layer]
            if (j >= 0) row[j] = v;
        }
        __syncthreads();
    }
    if (a.target != nullptr && row != nullptr) {       // the block's BCE sum: a fixed tree over its threads
        float* red = scr;
        red[tid] = bce_acc;
        __syncthreads();
        for (int s = FC_BLOCK / 2; s > 0; s >>= 1) {
            if (tid < s) red[tid] = red[tid] + red[tid + s];
            __syncthreads();
        }
        if (tid == 0) row[a.P] = red[0];
    }
}

struct FcReduceArgs {
    const float* slab;     // [rows][stride]
    int rows, stride, P;   // P gradient columns (0: the loss only), column P of the slab = BCE sums
    float gfac, count;     // loss = gfac * (sum / count)
    float* grads;          // [P] or null
    int32_t* status;       // or null
    float* loss_out;       // the caller's float or null
    float* loss_ws;        // the workspace's copy (never null)
};

// one block: column j of the slab summed over the rows in a fixed order (four interleaved partial sums, then (0 + 1) + (2 + 3))
__global__ void __launch_bounds__(FC_REDUCE_BLOCK) fc_reduce_kernel(const FcReduceArgs a) {
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    const int j = threadIdx.x;
    const bool grad_col = a.grads != nullptr && j < a.P, loss_col = j == a.P;
    float v = 0.f;
    if (grad_col || loss_col) {
        float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
        int r = 0;
        for (; r + 3 < a.rows; r += 4) {
            p0 = p0 + a.slab[(size_t)r * a.stride + j];
            p1 = p1 + a.slab[(size_t)(r + 1) * a.stride + j];
            p2 = p2 + a.slab[(size_t)(r + 2) * a.stride + j];
            p3 = p3 + a.slab[(size_t)(r + 3) * a.stride + j];
        }
        for (; r < a.rows; ++r) p0 = p0 + a.slab[(size_t)r * a.stride + j];
        v = (p0 + p1) + (p2 + p3);
        if (loss_col) v = a.gfac * (v / a.count);
        if (!isfinite(v)) atomicOr(&bad, 1);   // (an LDS flag: order-free)
    }
    __syncthreads();
    if (grad_col) a.grads[j] = bad ? 0.f : v;
    if (loss_col) {
        a.loss_ws[0] = v;
        if (a.loss_out) a.loss_out[0] = v;
        if (a.status) a.status[0] = bad;
    }
}

}  // namespace
