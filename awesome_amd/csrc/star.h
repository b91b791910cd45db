// star.h - the star-shape prior of the teaser as a device-resident fit (notebooks/icml_teaser_code/star_shaped/
// star.ipynb cells 2-3).
//
//     x' = x + offset,  r = |x'|,  x^ = x' / (0.01 + r)
//     x_old = relu(W0 x^ + b0)                               [h]      a function of the direction alone
//     r_aug = relu(W1 x_old + b1 + W1_r r + b1_r)            [h]
//     out   = r (W2 x_old + b2 + W2_r r_aug + b2_r) - 1                W2_r >= 0, projected after every optimizer step
//     loss  = mean((sigmoid(out) - label)^2) over a minibatch of pixels; Adam over every parameter, `offset` from a given epoch on
//
// The read-out takes two layers at once (x_old AND r_aug) and the logit is scaled per point by r: neither is in the layer chain of the
// fused ICNN step kernels.  The notebook trains on 1000-pixel minibatches (500 background + 500 foreground pixels drawn per epoch),
// i.e. 1000 x h activations per layer - a launch-bound problem, not an MFMA-bound one.  It therefore runs layer by layer like wide.h:
// activations of the minibatch in HBM ([batch][h] row-major), the three h x h contractions as the fp32-MFMA GEMMs of csrc/gemm.h (the minibatch contraction in slices added in order), and
// everything else hand-written below: the polar split with layer 0, the epilogues, read-out + sigmoid + MSE + dL/dout, the relu masks
// of the backward pass, fixed-order column and point reductions, the gradient of the centre, torch's single-tensor Adam with the
// projection.  Twelve launches per optimizer step, none of them synchronises with the host; the minibatch indices of every epoch are an
// input ([steps][batch], drawn on the host side of the boundary like the notebook's torch.randperm).
//
// Parameters: ONE flat vector in the order of the notebook class's named_parameters():
//     offset[2] | W0.weight[h][2] | W0.bias[h] | W1.weight[h][h] | W1.bias[h] | W2.weight[h] | W2.bias | W1_r.weight[h] | W1_r.bias[h]
//     | W2_r.weight[h] | W2_r.bias                                                     P = h^2 + 8 h + 4
#pragma once
#include "wide.h"

namespace {

struct StarMap {
    int h, P;
    __host__ __device__ int p_off() const { return 0; }
    __host__ __device__ int p_w0() const { return 2; }
    __host__ __device__ int p_b0() const { return 2 + 2 * h; }
    __host__ __device__ int p_w1() const { return 2 + 3 * h; }
    __host__ __device__ int p_b1() const { return p_w1() + h * h; }
    __host__ __device__ int p_w2() const { return p_b1() + h; }
    __host__ __device__ int p_b2() const { return p_w2() + h; }
    __host__ __device__ int p_w1r() const { return p_b2() + 1; }
    __host__ __device__ int p_b1r() const { return p_w1r() + h; }
    __host__ __device__ int p_w2r() const { return p_b1r() + h; }
    __host__ __device__ int p_b2r() const { return p_w2r() + h; }
};
inline StarMap make_star_map(int h) {
    StarMap m{h, 0};
    m.P = m.p_b2r() + 1;
    return m;
}

constexpr int STAR_FEAT = 8;        // per point: x^0, x^1, r, x'0, x'1, 1 / (0.01 + r), -, -
constexpr int STAR_COLQ = 7;        // column sums per hidden unit: db1(=db1_r), dW1_r, dW2, dW2_r, db0, dW0[.][0], dW0[.][1]
constexpr int STAR_CHUNKS = 16;     // point chunks of the column sums (added in chunk order by the update kernel)

__device__ __forceinline__ float wave_sum(float v) {   // fixed butterfly order: reproducible
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// pixel number of minibatch entry p, clamped into the image (an index outside it must not become a fault)
__device__ __forceinline__ long long star_pixel(const int32_t* __restrict__ idx, const long long p, const long long n_pixels) {
    if (idx == nullptr) return p;
    const long long v = idx[p];
    return v < 0 ? 0 : (v >= n_pixels ? n_pixels - 1 : v);
}

// polar split + layer 0: thread = (point, unit).  idx: this epoch's minibatch (pixel numbers into coords / labels), or null = all points.
__global__ __launch_bounds__(256) void star_l0_kernel(const float* __restrict__ prm, const StarMap m, const float* __restrict__ coords,
                                                      const int32_t* __restrict__ idx, const long long n_pixels, const long long N,
                                                      float* __restrict__ feat, float* __restrict__ A0) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= N * m.h) return;
    const long long p = e / m.h;
    const int j = (int)(e - p * m.h);
    const long long pix = star_pixel(idx, p, n_pixels);
    const float x0 = coords[2 * pix] + prm[0], x1 = coords[2 * pix + 1] + prm[1];
    const float r = __fsqrt_rn(__fadd_rn(__fmul_rn(x0, x0), __fmul_rn(x1, x1)));
    const float den = __fadd_rn(0.01f, r);
    const float u0 = __fdiv_rn(x0, den), u1 = __fdiv_rn(x1, den);
    if (j == 0) {
        float* f = feat + p * STAR_FEAT;
        f[0] = u0; f[1] = u1; f[2] = r; f[3] = x0; f[4] = x1; f[5] = __fdiv_rn(1.f, den);
    }
    const float pre = fmaf(prm[m.p_w0() + 2 * j + 1], u1, fmaf(prm[m.p_w0() + 2 * j], u0, prm[m.p_b0() + j]));
    A0[e] = fmaxf(pre, 0.f);
}

// r_aug = relu((P1 + b1) + (W1_r r + b1_r)), in place over the GEMM's output
__global__ __launch_bounds__(256) void star_l1_kernel(const float* __restrict__ prm, const StarMap m, const float* __restrict__ feat,
                                                      const long long N, float* __restrict__ A1) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= N * m.h) return;
    const long long p = e / m.h;
    const int j = (int)(e - p * m.h);
    const float a = __fadd_rn(A1[e], prm[m.p_b1() + j]);
    const float b = fmaf(prm[m.p_w1r() + j], feat[p * STAR_FEAT + 2], prm[m.p_b1r() + j]);
    A1[e] = fmaxf(__fadd_rn(a, b), 0.f);
}

// read-out, sigmoid, squared error and dL/dout: one wave per point, four points per block.
// labels == null: forward only (logits out).  partial: [blocks][2] = (sum of squared errors, sum of ds) of the block's points.
// DENSE (the full-batch fits below): the criterion is the ICNN fits' data term (wide_data_term: SE / BCE on the sigmoid with the class
// coefficient coef[0] (target < 0.5) / coef[1], 'mean' normalisation included), labels / logits are this tile's rows, no index.
template <bool DENSE>
__global__ __launch_bounds__(256) void star_out_kernel(const float* __restrict__ prm, const StarMap m, const float* __restrict__ feat,
                                                       const float* __restrict__ A0, const float* __restrict__ A1,
                                                       const float* __restrict__ labels, const int32_t* __restrict__ idx,
                                                       const long long n_pixels, const long long N, float* __restrict__ logits, float* __restrict__ ds, float* __restrict__ drd,
                                                       float* __restrict__ partial, const float* __restrict__ coef = nullptr,
                                                       const int loss_kind = INR_LOSS_SE) {
    __shared__ float sh[4][2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long p = (long long)blockIdx.x * 4 + wv;
    float se = 0.f, sds = 0.f;
    if (p < N) {
        float sa = 0.f, sr = 0.f;
        for (int j = lane; j < m.h; j += 64) {
            sa = fmaf(prm[m.p_w2() + j], A0[p * m.h + j], sa);
            sr = fmaf(prm[m.p_w2r() + j], A1[p * m.h + j], sr);
        }
        sa = wave_sum(sa);
        sr = wave_sum(sr);
        const float r = feat[p * STAR_FEAT + 2];
        const float s = __fadd_rn(__fadd_rn(sa, prm[m.p_b2()]), __fadd_rn(sr, prm[m.p_b2r()]));
        const float out = __fsub_rn(__fmul_rn(r, s), 1.f);
        if (lane == 0) {
            if (logits) logits[p] = out;
            if (DENSE && labels) {
                float l = 0.f, dout = 0.f;
                wide_data_term<false>(labels, coef, loss_kind, WideJoint{}, p, out, l, dout);
                ds[p] = dout * r;
                drd[p] = dout * s;
                se = l;
                sds = dout * r;
            } else if (labels) {
                const float pr = 1.f / (1.f + expf(-out));
                const float er = pr - labels[star_pixel(idx, p, n_pixels)];
                const float dout = 2.f * er / (float)N * pr * (1.f - pr);
                ds[p] = dout * r;
                drd[p] = dout * s;
                se = er * er;
                sds = dout * r;
            }
        }
    }
    if (partial == nullptr) return;
    if (lane == 0) { sh[wv][0] = se; sh[wv][1] = sds; }
    __syncthreads();
    if (threadIdx.x < 2) partial[2 * blockIdx.x + threadIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

// D1 = ds W2_r (.) [r_aug > 0]
__global__ __launch_bounds__(256) void star_bwd1_kernel(const float* __restrict__ prm, const StarMap m, const float* __restrict__ ds,
                                                        const float* __restrict__ A1, const long long N, float* __restrict__ D1) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= N * m.h) return;
    const long long p = e / m.h;
    const int j = (int)(e - p * m.h);
    D1[e] = A1[e] > 0.f ? ds[p] * prm[m.p_w2r() + j] : 0.f;
}

// D0 = (D1 W1 + ds W2) (.) [x_old > 0], in place over the GEMM's output
__global__ __launch_bounds__(256) void star_bwd0_kernel(const float* __restrict__ prm, const StarMap m, const float* __restrict__ ds,
                                                        const float* __restrict__ A0, const long long N, float* __restrict__ D0) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= N * m.h) return;
    const long long p = e / m.h;
    const int j = (int)(e - p * m.h);
    D0[e] = A0[e] > 0.f ? fmaf(ds[p], prm[m.p_w2() + j], D0[e]) : 0.f;
}

// Column sums over the points of one chunk: grid (ceil(h / 32), CHUNKS), thread = (unit jj of 32, point group pg of 8).
// colp[chunk][q][h]; fixed order: a thread walks its points in order, the 8 groups are added in order.
// CHUNKS: STAR_CHUNKS for a minibatch; the dense fits cut a tile into STAR_DENSE_CHUNKS (a thread's walk is a chain of dependent
// loads: at 16 chunks of a 16384-point tile it is 128 steps long on 80 blocks; measured, a 256 x 256 step: 1081 -> 1056 us).
template <int CHUNKS>
__global__ __launch_bounds__(256) void star_col_kernel(const StarMap m, const float* __restrict__ feat, const float* __restrict__ ds,
                                                       const float* __restrict__ A0, const float* __restrict__ A1,
                                                       const float* __restrict__ D0, const float* __restrict__ D1, const long long N,
                                                       float* __restrict__ colp) {
    __shared__ float sh[8][STAR_COLQ][32];
    const int jj = threadIdx.x & 31, pg = threadIdx.x >> 5, j = blockIdx.x * 32 + jj, c = blockIdx.y;
    const long long cl = (N + CHUNKS - 1) / CHUNKS, p0 = c * cl, p1 = p0 + cl < N ? p0 + cl : N;
    float a[STAR_COLQ];
#pragma unroll
    for (int q = 0; q < STAR_COLQ; ++q) a[q] = 0.f;
    if (j < m.h) {
        for (long long p = p0 + pg; p < p1; p += 8) {
            const float d1 = D1[p * m.h + j], d0 = D0[p * m.h + j], s = ds[p];
            const float* f = feat + p * STAR_FEAT;
            a[0] += d1;
            a[1] = fmaf(d1, f[2], a[1]);
            a[2] = fmaf(s, A0[p * m.h + j], a[2]);
            a[3] = fmaf(s, A1[p * m.h + j], a[3]);
            a[4] += d0;
            a[5] = fmaf(d0, f[0], a[5]);
            a[6] = fmaf(d0, f[1], a[6]);
        }
    }
#pragma unroll
    for (int q = 0; q < STAR_COLQ; ++q) sh[pg][q][jj] = a[q];
    __syncthreads();
    for (int t = threadIdx.x; t < STAR_COLQ * 32; t += 256) {
        const int q = t >> 5, k = t & 31;
        if (blockIdx.x * 32 + k >= m.h) continue;
        float v = 0.f;
#pragma unroll
        for (int g = 0; g < 8; ++g) v += sh[g][q][k];
        colp[((size_t)c * STAR_COLQ + q) * m.h + blockIdx.x * 32 + k] = v;
    }
}

// Gradient of the centre: per point dx^ = D0 W0, dr = dout s + D1 . W1_r, chained through x^ = x' / (0.01 + r), r = |x'|
// (a pixel exactly at -offset has r = 0 and a NaN gradient, in torch as here).  One wave per point; offp[blocks][2].
// DENSE: on a full grid the centre can sit on a pixel; that pixel contributes nothing to the centre's gradient (include/inrfit.h).
template <bool DENSE>
__global__ __launch_bounds__(256) void star_point_kernel(const float* __restrict__ prm, const StarMap m, const float* __restrict__ feat,
                                                         const float* __restrict__ drd, const float* __restrict__ D0,
                                                         const float* __restrict__ D1, const long long N, float* __restrict__ offp) {
    __shared__ float sh[4][2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long p = (long long)blockIdx.x * 4 + wv;
    float g0 = 0.f, g1 = 0.f;
    if (p < N) {
        float du0 = 0.f, du1 = 0.f, drh = 0.f;
        for (int j = lane; j < m.h; j += 64) {
            const float d0 = D0[p * m.h + j];
            du0 = fmaf(d0, prm[m.p_w0() + 2 * j], du0);
            du1 = fmaf(d0, prm[m.p_w0() + 2 * j + 1], du1);
            drh = fmaf(D1[p * m.h + j], prm[m.p_w1r() + j], drh);
        }
        du0 = wave_sum(du0);
        du1 = wave_sum(du1);
        drh = wave_sum(drh);
        const float* f = feat + p * STAR_FEAT;
        const float r = f[2], x0 = f[3], x1 = f[4], q = f[5];
        const float dden = -(du0 * x0 + du1 * x1) * q * q;     // d / d(0.01 + r) of x' / (0.01 + r)
        const float dr = drd[p] + drh + dden;
        g0 = du0 * q + dr * x0 / r;                            // r = sqrt(x'0^2 + x'1^2): dr / dx' = x' / r
        g1 = du1 * q + dr * x1 / r;
        if (DENSE && r == 0.f) g0 = g1 = 0.f;
    }
    if (lane == 0) { sh[wv][0] = g0; sh[wv][1] = g1; }
    __syncthreads();
    if (threadIdx.x < 2) offp[2 * blockIdx.x + threadIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

// One block: the per-block partials of the read-out (loss, sum ds) and of the centre's gradient, each in a fixed order.
// scal[0] = loss, scal[1] = db2 (= db2_r), scal[2..3] = doffset
__global__ __launch_bounds__(256) void star_scalar_kernel(const float* __restrict__ partial, const float* __restrict__ offp, const int nb,
                                                          const long long N, float* __restrict__ scal, float* __restrict__ loss_hist,
                                                          const int hist_idx) {
    __shared__ float sm[4];
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int b = threadIdx.x; b < nb; b += 256) {
        v[0] += partial[2 * b];
        v[1] += partial[2 * b + 1];
        v[2] += offp[2 * b];
        v[3] += offp[2 * b + 1];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float t = block_sum256(v[k], sm);
        if (threadIdx.x == 0) {
            const float o = k == 0 ? t / (float)N : t;
            scal[k] = o;
            if (k == 0 && loss_hist) loss_hist[hist_idx] = o;
        }
    }
}

struct StarUpdArgs {
    float* prm;          // [P] in place
    float* opt;          // [2 P] exp_avg | exp_avg_sq
    const float* gW1;    // [h][h] from the GEMM
    const float* colp;   // [STAR_CHUNKS][STAR_COLQ][h]
    const float* scal;   // loss, db2, doffset[2]
    float* grads_out;    // [P] or null: the assembled gradient (mode 1: no optimizer step)
    StarMap m;
    float lr;
    OptConsts net, off;              // the network's / the centre's (its own step count; t = 0: it takes no step)
    int offset_on;                   // the centre takes this step
    int mode;                        // 0 = Adam + projection, 1 = gradients only
};

// Where the gradient of parameter i < P comes from: -1 = `g` (a scalar of `scal`, an element of the h x h product), else the column
// sum colq of hidden unit j - which each update kernel forms from what its backward pass left (chunk partials / the accumulated col).
__device__ __forceinline__ int star_grad_source(const StarMap& m, const int i, const float* __restrict__ scal, const float* __restrict__ gW1,
                                                float& g, int& j) {
    int colq = -1;
    if (i < m.p_w0()) g = scal[2 + i];
    else if (i < m.p_b0()) { j = (i - m.p_w0()) >> 1; colq = 5 + ((i - m.p_w0()) & 1); }
    else if (i < m.p_w1()) { j = i - m.p_b0(); colq = 4; }
    else if (i < m.p_b1()) g = gW1[i - m.p_w1()];
    else if (i < m.p_w2()) { j = i - m.p_b1(); colq = 0; }
    else if (i < m.p_b2()) { j = i - m.p_w2(); colq = 2; }
    else if (i < m.p_w1r()) g = scal[1];
    else if (i < m.p_b1r()) { j = i - m.p_w1r(); colq = 1; }
    else if (i < m.p_w2r()) { j = i - m.p_b1r(); colq = 0; }
    else if (i < m.p_b2r()) { j = i - m.p_w2r(); colq = 3; }
    else if (i < m.P) g = scal[1];
    return colq;
}
// W2_r.weight <- relu(W2_r.weight) behind the step
__device__ __forceinline__ float star_project(const StarMap& m, const int i, const float p) {
    return (i >= m.p_w2r() && i < m.p_b2r()) ? fmaxf(p, 0.f) : p;
}

// torch.optim.Adam, single-tensor arithmetic in torch's operation order (optim.h), then W2_r.weight <- relu(W2_r.weight)
__global__ __launch_bounds__(256) void star_update_kernel(const StarUpdArgs u) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const StarMap& m = u.m;
    if (i >= m.P) return;
    const int h = m.h;
    float g = 0.f;
    int j = 0;
    const int colq = star_grad_source(m, i, u.scal, u.gW1, g, j);
    if (colq >= 0) {
        g = 0.f;
#pragma unroll
        for (int c = 0; c < STAR_CHUNKS; ++c) g += u.colp[((size_t)c * STAR_COLQ + colq) * h + j];
    }
    if (u.grads_out) u.grads_out[i] = g;
    if (u.mode != 0) return;
    const bool is_off = i < m.p_w0();
    if (is_off && !u.offset_on) return;     // requires_grad = False: torch's Adam skips a parameter without a gradient
    float p = u.prm[i], mm = u.opt[i], v = u.opt[m.P + i];
    const OptConsts c = is_off ? u.off : u.net;
    p = star_project(m, i, adam_step(c, opt_step_size(u.lr, c.bc1), 0.f, g, p, mm, v));
    u.prm[i] = p;
    u.opt[i] = mm;
    u.opt[m.P + i] = v;
}

// ---- workspace ---------------------------------------------------------------------------------------------------------------------------
struct StarWs {
    float *feat, *A0, *A1, *D1, *D0, *ds, *drd, *partial, *offp, *colp, *gW1, *gpart, *scal;
    int nb4;           // blocks of the one-wave-per-point kernels
    long long bytes;
};
inline StarWs carve_star(int h, long long N, void* base) {
    StarWs w{};
    char* b = (char*)base;
    long long off = 0;
    auto take = [&](long long bytes) {
        float* p = (float*)(b + off);
        off += (bytes + 255) / 256 * 256;
        return p;
    };
    w.nb4 = (int)((N + 3) / 4);
    w.feat = take(N * STAR_FEAT * 4);
    w.A0 = take(N * h * 4);
    w.A1 = take(N * h * 4);
    w.D1 = take(N * h * 4);
    w.D0 = take(N * h * 4);
    w.ds = take(N * 4);
    w.drd = take(N * 4);
    w.partial = take((long long)w.nb4 * 2 * 4);
    w.offp = take((long long)w.nb4 * 2 * 4);
    w.colp = take((long long)STAR_CHUNKS * STAR_COLQ * h * 4);
    w.gW1 = take((long long)h * h * 4);
    w.gpart = take((long long)GEMM_SPLITK_MAX * h * h * 4);   // slices of the minibatch contraction (gemm_rm_splitk)
    w.scal = take(256);
    w.bytes = off;
    return w;
}

constexpr int STAR_MAX_HIDDEN = 1024;
constexpr long long STAR_MAX_BATCH = 1 << 16;   // the weight-gradient GEMM contracts over the minibatch in one call

inline dim3 star_elem_grid(long long N, int h) { return dim3((unsigned)((N * h + 255) / 256)); }

// forward of N points (idx: minibatch or null); labels != null also leaves dL/dout behind for the backward pass
inline int star_forward_pass(const StarMap& m, const StarWs& w, const float* prm, const float* coords, const int32_t* idx,
                             long long n_pixels, long long N, const float* labels, float* logits, hipStream_t s) {
    const int h = m.h;
    hipLaunchKernelGGL(star_l0_kernel, star_elem_grid(N, h), dim3(256), 0, s, prm, m, coords, idx, n_pixels, N, w.feat, w.A0);
    int rc = gemm_rm(s, false, true, (int)N, h, h, w.A0, h, prm + m.p_w1(), h, w.A1, h);      // P1 = x_old W1^T
    if (rc) return rc;
    hipLaunchKernelGGL(star_l1_kernel, star_elem_grid(N, h), dim3(256), 0, s, prm, m, (const float*)w.feat, N, w.A1);
    hipLaunchKernelGGL(star_out_kernel<false>, dim3(w.nb4), dim3(256), 0, s, prm, m, (const float*)w.feat, (const float*)w.A0, (const float*)w.A1,
                       labels, idx, n_pixels, N, logits, w.ds, w.drd, labels ? w.partial : nullptr);
    return INR_OK;
}

// backward of the pass above: every gradient into gW1 / colp / scal (assembled by star_update_kernel)
inline int star_backward_pass(const StarMap& m, const StarWs& w, const float* prm, long long N, float* loss_hist, int hist_idx,
                              hipStream_t s) {
    const int h = m.h;
    hipLaunchKernelGGL(star_bwd1_kernel, star_elem_grid(N, h), dim3(256), 0, s, prm, m, (const float*)w.ds, (const float*)w.A1, N, w.D1);
    int rc = gemm_rm(s, false, false, (int)N, h, h, w.D1, h, prm + m.p_w1(), h, w.D0, h);     // D1 W1
    if (rc) return rc;
    hipLaunchKernelGGL(star_bwd0_kernel, star_elem_grid(N, h), dim3(256), 0, s, prm, m, (const float*)w.ds, (const float*)w.A0, N, w.D0);
    if ((rc = gemm_rm_splitk(s, true, false, h, h, (int)N, w.D1, h, w.A0, h, w.gW1, w.gpart))) return rc;   // dW1 = D1^T x_old, slices added in order
    hipLaunchKernelGGL(star_col_kernel<STAR_CHUNKS>, dim3((h + 31) / 32, STAR_CHUNKS), dim3(256), 0, s, m, (const float*)w.feat, (const float*)w.ds,
                       (const float*)w.A0, (const float*)w.A1, (const float*)w.D0, (const float*)w.D1, N, w.colp);
    hipLaunchKernelGGL(star_point_kernel<false>, dim3(w.nb4), dim3(256), 0, s, prm, m, (const float*)w.feat, (const float*)w.drd,
                       (const float*)w.D0, (const float*)w.D1, N, w.offp);
    hipLaunchKernelGGL(star_scalar_kernel, dim3(1), dim3(256), 0, s, (const float*)w.partial, (const float*)w.offp, w.nb4, N, w.scal,
                       loss_hist, hist_idx);
    return INR_OK;
}

// ---- dense full-batch fits (inrfit_star_fit_dense / inrfit_star_loss_grad_dense) ------------------------------------------------------
// Every step sees ALL pixels of the image.  The grid is walked in tiles of STAR_DENSE_TILE points: the kernels above run on one tile
// at a time ([T][h] activations, whatever the image's size), and star_dense_acc_kernel adds the tile's gradient pieces - the h x h
// product (its split-K slices already added in slice order), the seven column sums (their STAR_DENSE_CHUNKS chunks added in chunk order), the
// loss, db2 and the centre's two components - onto the image's accumulators, tile after tile in stream order.  The tile size is a
// constant, not a property of the device: it fixes the order of every sum, so two runs give the same bits.
// Twelve launches per tile and one update launch per step; nothing synchronises with the host.
constexpr int STAR_DENSE_TILE = 16384;
constexpr int STAR_DENSE_CHUNKS = 128;   // point chunks of a tile's column sums (128 points each in a full tile)

// acc layout per call (images run one after another): gW1 [h][h] | col [STAR_COLQ][h] | scal [4] = loss, db2, doffset[2]
// grid: the elementwise blocks + ONE last block for the four scalars.  first: tile 0 stores, the others add.
__global__ __launch_bounds__(256) void star_dense_acc_kernel(const StarMap m, const float* __restrict__ gW1t, const float* __restrict__ colp,
                                                             const float* __restrict__ partial, const float* __restrict__ offp,
                                                             const int nb, const int first, float* __restrict__ gW1,
                                                             float* __restrict__ col, float* __restrict__ scal) {
    const int h = m.h;
    if (blockIdx.x == gridDim.x - 1) {
        __shared__ float sm[4];
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        for (int b = threadIdx.x; b < nb; b += 256) {
            v[0] += partial[2 * b];
            v[1] += partial[2 * b + 1];
            v[2] += offp[2 * b];
            v[3] += offp[2 * b + 1];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float t = block_sum256(v[k], sm);
            if (threadIdx.x == 0) scal[k] = first ? t : scal[k] + t;
        }
        return;
    }
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < h * h) {
        gW1[e] = first ? gW1t[e] : gW1[e] + gW1t[e];
    } else if (e < h * h + STAR_COLQ * h) {
        const int qj = e - h * h;   // = q * h + j
        float g = 0.f;
#pragma unroll
        for (int c = 0; c < STAR_DENSE_CHUNKS; ++c) g += colp[(size_t)c * STAR_COLQ * h + qj];
        col[qj] = first ? g : col[qj] + g;
    }
}

struct StarDenseUpdArgs {
    float* prm;          // [P] in place
    float* opt;          // [2 P + INR_OPT_HEADER_FLOATS]: exp_avg | exp_avg_sq or exp_inf | header (include/inrfit.h)
    const float* gW1;    // the accumulators of star_dense_acc_kernel
    const float* col;
    const float* scal;
    float* grads_out;    // mode 1: [P]
    float* loss_out;     // mode 1: [1]
    float* loss_hist;    // mode 0: this step's slot, or null
    int32_t* status;     // mode 0: this image's word
    StarMap m;
    InrOptDesc od;
    OptConsts net, off;              // the network's / the centre's (its own step count; t = 0: it takes no step)
    int offset_on;                   // the centre takes this step
    int t;                           // 1-based optimizer step index (selects the header's double-buffer slots)
    int mode;                        // 0 = optimizer step + projection + plateau, 1 = gradients and loss only
};

// Thread i < P: one parameter (torch's single-tensor Adam / Adamax in its operation order, then W2_r.weight <- relu(W2_r.weight));
// thread P: the loss, the "frozen by a non-finite loss" flag and ReduceLROnPlateau in the header (optim.h, shared with
// icnn_update_kernel): every thread derives "frozen" from the flag the previous step left and from THIS step's loss, so which
// parameters move does not depend on block timing.
__global__ __launch_bounds__(256) void star_dense_update_kernel(const StarDenseUpdArgs u) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const StarMap& m = u.m;
    if (i > m.P) return;
    const int h = m.h;
    const float loss = u.scal[0];
    float g = 0.f;
    int j = 0;
    const int colq = star_grad_source(m, i, u.scal, u.gW1, g, j);
    if (colq >= 0) g = u.col[colq * h + j];
    if (u.mode != 0) {
        if (i < m.P) u.grads_out[i] = g;
        else u.loss_out[0] = loss;
        return;
    }
    float* __restrict__ hdr = u.opt + 2 * (size_t)m.P;
    const bool bad_before = hdr[opt_hdr_frozen_before(u.t)] != 0.f;
    const float lr_now = hdr[opt_hdr_lr_of(u.t)];
    const bool frozen = bad_before || !isfinite(loss);
    if (i == m.P) {
        opt_header_step(hdr, u.od, u.t, loss, frozen, lr_now, u.loss_hist, u.status);
        return;
    }
    if (frozen) return;
    const bool is_off = i < m.p_w0();
    if (is_off && !u.offset_on) return;     // requires_grad = False: torch's optimizers skip a parameter without a gradient
    float p = u.prm[i], mm = u.opt[i], v = u.opt[m.P + i];
    const OptConsts c = is_off ? u.off : u.net;
    p = star_project(m, i, opt_step(u.od.kind, c, opt_step_size(lr_now, c.bc1), 0.f, g, p, mm, v));
    u.prm[i] = p;
    u.opt[i] = mm;
    u.opt[m.P + i] = v;
}

struct StarDenseWs {
    StarWs t;                        // one tile's buffers
    float *colp;                     // [STAR_DENSE_CHUNKS][STAR_COLQ][h] column sums of the tile's chunks
    float *gW1, *col, *scal, *coef;  // the image's accumulators; coef [n_images][2]
    long long bytes;
};
inline StarDenseWs carve_star_dense(int h, long long n_pixels, int n_images, void* base) {
    StarDenseWs w{};
    w.t = carve_star(h, n_pixels < STAR_DENSE_TILE ? n_pixels : STAR_DENSE_TILE, base);
    char* b = (char*)base;
    long long off = w.t.bytes;
    auto take = [&](long long bytes) {
        float* p = (float*)(b + off);
        off += (bytes + 255) / 256 * 256;
        return p;
    };
    w.colp = take((long long)STAR_DENSE_CHUNKS * STAR_COLQ * h * 4);
    w.gW1 = take((long long)h * h * 4);
    w.col = take((long long)STAR_COLQ * h * 4);
    w.scal = take(256);
    w.coef = take((long long)n_images * 2 * 4);
    w.bytes = off;
    return w;
}

// One pass over all N pixels of an image, tile by tile.  labels != null: the criterion; backward: every gradient onto the accumulators
// (complete after the last tile); logits != null: the forward's output [N].
inline int star_dense_pass(const StarMap& m, const StarDenseWs& w, const float* prm, const float* coords, const float* labels,
                           const float* coef, int loss_kind, long long N, float* logits, bool backward, hipStream_t s) {
    const int h = m.h;
    const StarWs& t = w.t;
    for (long long p0 = 0; p0 < N; p0 += STAR_DENSE_TILE) {
        const long long n = N - p0 < STAR_DENSE_TILE ? N - p0 : STAR_DENSE_TILE;
        const int nb4 = (int)((n + 3) / 4);
        hipLaunchKernelGGL(star_l0_kernel, star_elem_grid(n, h), dim3(256), 0, s, prm, m, coords + 2 * p0, (const int32_t*)nullptr, n, n,
                           t.feat, t.A0);
        int rc = gemm_rm(s, false, true, (int)n, h, h, t.A0, h, prm + m.p_w1(), h, t.A1, h);      // P1 = x_old W1^T
        if (rc) return rc;
        hipLaunchKernelGGL(star_l1_kernel, star_elem_grid(n, h), dim3(256), 0, s, prm, m, (const float*)t.feat, n, t.A1);
        hipLaunchKernelGGL(star_out_kernel<true>, dim3(nb4), dim3(256), 0, s, prm, m, (const float*)t.feat, (const float*)t.A0,
                           (const float*)t.A1, labels ? labels + p0 : nullptr, (const int32_t*)nullptr, n, n,
                           logits ? logits + p0 : nullptr, t.ds, t.drd, labels ? t.partial : nullptr, coef, loss_kind);
        if (!backward) continue;
        hipLaunchKernelGGL(star_bwd1_kernel, star_elem_grid(n, h), dim3(256), 0, s, prm, m, (const float*)t.ds, (const float*)t.A1, n, t.D1);
        if ((rc = gemm_rm(s, false, false, (int)n, h, h, t.D1, h, prm + m.p_w1(), h, t.D0, h))) return rc;     // D1 W1
        hipLaunchKernelGGL(star_bwd0_kernel, star_elem_grid(n, h), dim3(256), 0, s, prm, m, (const float*)t.ds, (const float*)t.A0, n, t.D0);
        if ((rc = gemm_rm_splitk(s, true, false, h, h, (int)n, t.D1, h, t.A0, h, t.gW1, t.gpart))) return rc;  // dW1 of the tile
        hipLaunchKernelGGL(star_col_kernel<STAR_DENSE_CHUNKS>, dim3((h + 31) / 32, STAR_DENSE_CHUNKS), dim3(256), 0, s, m, (const float*)t.feat,
                           (const float*)t.ds, (const float*)t.A0, (const float*)t.A1, (const float*)t.D0, (const float*)t.D1, n, w.colp);
        hipLaunchKernelGGL(star_point_kernel<true>, dim3(nb4), dim3(256), 0, s, prm, m, (const float*)t.feat, (const float*)t.drd,
                           (const float*)t.D0, (const float*)t.D1, n, t.offp);
        hipLaunchKernelGGL(star_dense_acc_kernel, dim3((h * h + STAR_COLQ * h + 255) / 256 + 1), dim3(256), 0, s, m, (const float*)t.gW1,
                           (const float*)w.colp, (const float*)t.partial, (const float*)t.offp, nb4, p0 == 0 ? 1 : 0, w.gW1, w.col, w.scal);
    }
    return INR_OK;
}

}  // namespace
