// wide.h - the layer-by-layer path for ICNN shapes the fused step kernels cannot hold (n_hidden > 130, or more than two hidden layers).
//
// The fused kernels (icnn_step.h, icnn_step2.h) keep the whole weight image of the network in LDS and every activation in registers;
// that is what makes them fast and what limits them to n_hidden <= 130 (77 KB per hidden layer for h = 130; 160 KB of LDS per CU) and
// L <= 2.  A `n_hidden: 256` or the 3 x 350 relu net of notebooks/imageRepresentationTest.ipynb cell 5 needs another shape of program:
// activations of a whole image in HBM (N x h floats per layer: 92 MB at 256x256 x 350 - nothing on a 288 GB part), one launch per
// layer and direction, and the h x h contractions as tiled fp32-MFMA GEMMs - csrc/gemm.h, hand-written for gfx950 (round 4; rounds
// 2-3 called rocBLAS here).  What used to be separate element-wise passes over the activations rides in the GEMMs' epilogues (bias +
// skip + relu of a hidden layer; the relu / periodic-activation mask of the backward pass) or in the one pass over Z_L that computes
// the output layer, the data term, dL/dlogit, dZ_L and the output layer's weight gradients (wide_out_kernel); the gradients of what the
// ext inputs (1, x) multiply - (db_k | dS_k), (db_in | dW_in) = dz^T (1, X) - are summed by the kernel that writes dz (wide_out_kernel
// for the last layer, the backward GEMM's epilogue for the others).  The contractions over the
// points (weight gradients, K = n_points) are split over blockIdx.z into chunks of WIDE_CHUNK points whose partial products
// wide_reduce_kernel adds in chunk order: no atomics, reproducible.  The optimizer step is icnn_update_kernel itself on a one-"slab"
// view of the gradient vector.
//
// Same arithmetic as the reference (awesome/model/convex_net.py:205-214): z0 = act0(W_in x + b_in); z_{k+1} = relu(W_k z_k + b_k + S_k x);
// y = w_o . z_L + b_o + s_o . x.  Layout: activations row-major [N][hs] (a point's h units, then the "ext" inputs (1, x), then zeros up
// to a multiple of 4 floats so that rows start on 16-byte boundaries), parameters in the flat order of include/inrfit.h (torch's
// row-major [out][in] Linear weights); the hidden layers' weight matrices are copied once per step into [L][h][hp] with zero padding
// (0.25 - 1.5 MB, by the last blocks of the layer-0 launch) so that every GEMM operand loads 16 bytes per lane.
#pragma once
#include "gemm.h"

namespace {

constexpr int WIDE_CHUNK = 512;      // points per split of the point-contractions (GEMM partials): at least; see wide_chunk
#ifndef INR_WIDE_OUT_CHUNK
#define INR_WIDE_OUT_CHUNK 128
#endif
constexpr int WIDE_OUT_CHUNK = INR_WIDE_OUT_CHUNK;  // points per block of wide_out_kernel / wide_extgrad_kernel (their partials)
// a weight gradient's contraction over the points: 512 points per slice up to 3 x 3 tiles of 128, 1024 from 4 x 4 on (the launch keeps >= 1024
// workgroups at 65 536 points; half the partial-product bytes to write and to add up: h = 512 L = 2 1 879 -> 1 849 us; at 3 x 3 tiles the 576
// workgroups of 1024-point slices were 1 % slower)
inline int wide_chunk(int h) {
    const int t = (h + GM_BM - 1) / GM_BM;
    return t >= 4 ? 2 * WIDE_CHUNK : WIDE_CHUNK;
}
inline int splitk_parts(long long N, int h) { return (int)((N + wide_chunk(h) - 1) / wide_chunk(h)); }
inline int out_parts(long long N) { return (int)((N + WIDE_OUT_CHUNK - 1) / WIDE_OUT_CHUNK); }

// ---- flat parameter offsets for any (h, C, L, F, O) ----------------------------------------------------------------------------------------
// F = n_features (the width of layer 0, the encode stage; h by default), O = n_out (output channels; 1 by default).  Layer k >= 1 and the
// output layer read h units, hidden layer 0 reads the F features; with L = 0 the output layer reads the features directly.  F = h, O = 1
// is the ICNN layout of include/inrfit.h.
struct WideMap {
    int h, C, L, P, F, O;
    __host__ __device__ int kin(int k) const { return k == 0 ? F : h; }      // input width of hidden layer k
    __host__ __device__ int hl() const { return L > 0 ? h : F; }             // width of the last activation (what the output layer reads)
    __host__ __device__ int p_win() const { return 0; }
    __host__ __device__ int p_bin() const { return F * C; }
    __host__ __device__ int p_w(int k) const { return F * C + F + (k > 0 ? (h * F + h + h * C) + (k - 1) * (h * h + h + h * C) : 0); }
    __host__ __device__ int p_b(int k) const { return p_w(k) + h * kin(k); }
    __host__ __device__ int p_s(int k) const { return p_b(k) + h; }
    __host__ __device__ int p_wo() const { return p_w(L); }
    __host__ __device__ int p_bo() const { return p_wo() + O * hl(); }
    __host__ __device__ int p_so() const { return p_bo() + O; }
    // a shape the ICNN kernels never served: its own feature width, several outputs or no hidden layer (the notebooks' encode nets) -
    // the layer-by-layer path with the multi-channel head (wide_head_kernel) and the output layer's gradient as a GEMM
    __host__ __device__ bool general() const { return F != h || O != 1 || L == 0; }
};
inline WideMap make_wide_map(int h, int C, int L, int F = 0, int O = 0) {
    WideMap m{h, C, L, 0, F > 0 ? F : h, O > 0 ? O : 1};
    m.P = m.p_so() + m.O * C;
    return m;
}
inline WideMap make_wide_map(const InrModelDesc* md) {
    return make_wide_map(md->n_hidden, md->in_features, md->n_layers, md->n_features, md->n_out);
}
// packed copies of the hidden layers' weights: layer 0 [hq][Fq], layer k >= 1 [hq][hq] (h, F rounded up to 16, zero padded)
inline __host__ __device__ int wide_q16(int n) { return (n + 15) / 16 * 16; }
inline __host__ __device__ long long wide_wp_off(const WideMap& m, int k) {
    const long long hq = wide_q16(m.h);
    return k == 0 ? 0 : hq * wide_q16(m.F) + (long long)(k - 1) * hq * hq;
}

constexpr int WIDE_MAX_HIDDEN = 1024, WIDE_MAX_LAYERS = 8;
constexpr int WIDE_MAX_HIDDEN_PAD = (WIDE_MAX_HIDDEN + 1 + 3 + 3) / 4 * 4;   // longest activation row (h + 1 + C, padded to 4 floats)

// ---- kernels ---------------------------------------------------------------------------------------------------------------------------
// Activations are stored [N][hs] with hs = h + 1 + C: the h units of the layer, then the "ext" inputs (1, x_0 .. x_{C-1}) - as in the
// fused kernels, bias and skip weights ride in the contractions: dW_ext [h x hs] = dz^T Z_ext holds dW, db and dS of a layer at once.

// z0[p][j] = act0(W_in[j] . x_p + b_in[j]) for j < h, the ext columns (1, x) for h <= j < h + 1 + C, zeros in the padding; pre0
// (optional, [N][hp]) keeps the pre-activation for the periodic activations' derivative.  Reads the coordinates from the grid descriptor.
constexpr int WIDE_L0_POINTS = 64, WIDE_L0_REP = 4;
template <int C>
__global__ __launch_bounds__(256) void wide_layer0_kernel(InrGridDesc gd, int img, const float* __restrict__ win, const float* __restrict__ bin,
                                                          long long N, int h, int hs, int hp, int act0, float omega, float* __restrict__ z0,
                                                          float* __restrict__ pre0, int pt_blocks, const float* __restrict__ params, WideMap pk,
                                                          float* __restrict__ wp) {
    // a thread writes four consecutive columns (hs is a multiple of 4: rows are cut into hs / 4 quads) of WIDE_L0_REP points'
    // rows, WIDE_L0_POINTS apart: its layer-0 weights are read once, the points' coordinates are all requested before the first
    // row is computed (32-bit index arithmetic inside the block)
    const int nq = hs >> 2;
    if ((int)blockIdx.x >= pt_blocks) {   // the launch's last blocks: hidden-layer weights -> [L][hq][hq], hq = h rounded up to 16, zero padded:
                                          // whatever a k-step reads past h of the other operand meets a zero here (gemm.h, GemmArgs::buf)
        // (layer 0 reads the F features: [hq][Fq], Fq = F rounded up to 16, first)
        const int hq = wide_q16(pk.h), fq = wide_q16(pk.F), e0 = hq * fq, per = hq * hq;
        const int e = (((int)blockIdx.x - pt_blocks) * gridDim.y + blockIdx.y) * 256 + threadIdx.x;
        if (pk.L > 0 && e < e0 + (pk.L - 1) * per) {
            const int k = e < e0 ? 0 : 1 + (e - e0) / per, r = e < e0 ? e : (e - e0) - (k - 1) * per;
            const int ld = k == 0 ? fq : hq, kin = pk.kin(k), i = r / ld, j = r - i * ld;
            wp[e] = i < pk.h && j < kin ? params[pk.p_w(k) + i * kin + j] : 0.f;
        }
        return;
    }
    const int idx = blockIdx.y * 256 + threadIdx.x;
    if (idx >= WIDE_L0_POINTS * nq) return;
    const int pl = idx / nq;
    const int j0 = 4 * (idx - pl * nq);
    const long long pb = (long long)blockIdx.x * (WIDE_L0_POINTS * WIDE_L0_REP) + pl;
    float x[WIDE_L0_REP][C];
#pragma unroll
    for (int r = 0; r < WIDE_L0_REP; ++r) {
        const long long pv = pb + r * WIDE_L0_POINTS, p = pv < N ? pv : N - 1;
        if (gd.mode == INR_GRID_SEPARABLE) {
            const unsigned pu = (unsigned)p, row = pu / (unsigned)gd.width;   // (an image of this path has < 2^32 points: 1 KB of activations each)
            x[r][0] = gd.xs[pu - row * (unsigned)gd.width];
            x[r][1] = gd.ys[row];
            if (C > 2) x[r][C - 1] = gd.ts ? gd.ts[img] : 0.f;
        } else {
            const float* cp = gd.coords + (size_t)img * gd.coords_image_stride;
#pragma unroll
            for (int c = 0; c < C; ++c) x[r][c] = cp[(size_t)c * N + p];
        }
    }
    float bq[4], wq[4][C];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = j0 + q < h ? j0 + q : h - 1;
        bq[q] = bin[j];
#pragma unroll
        for (int c = 0; c < C; ++c) wq[q][c] = win[j * C + c];
    }
#pragma unroll
    for (int r = 0; r < WIDE_L0_REP; ++r) {
        const long long p = pb + r * WIDE_L0_POINTS;
        if (p >= N) break;
        f32x4 out;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = j0 + q;
            float v;
            if (j >= h) {
                v = j == h ? 1.f : 0.f;
#pragma unroll
                for (int c = 0; c < C; ++c) v = (j == h + 1 + c) ? x[r][c] : v;
            } else {
                v = bq[q];
#pragma unroll
                for (int c = 0; c < C; ++c) v = fmaf(wq[q][c], x[r][c], v);
                if (pre0) pre0[p * hp + j] = v;
                v = act0 == INR_ACT_COS ? hw_cos(v) : (act0 == INR_ACT_SIN ? hw_sin(omega * v) : fmaxf(v, 0.f));
            }
            out[q] = v;
        }
        *(f32x4*)(z0 + (size_t)p * hs + j0) = out;
    }
}

// ONE pass over the last layer's activations Z_L [N][hs] (16 lanes per point, 16 points per iteration, WIDE_OUT_CHUNK points per block):
//   y = w_o . z_L + b_o + s_o . x  -> logits;   TRAIN: sigmoid, data term -> dy, the loss partial of the block;
//   dZ_L[p][j] = dy w_o[j] [z_L[p][j] > 0]  (the row is still in the cache);
//   and the block's share of the output layer's gradients (dw_o | db_o | ds_o)[j] = sum_p dy[p] Z_L,ext[p][j], summed over the block's
//   points in a fixed order -> part[block][hs_valid] (wide_reduce_kernel adds the blocks in order).
// The data term of a joint step (as in the fused step kernels' StepArgs, icnn_step.h; the host fills both from one DataTerm): the
// first data_count points carry the criterion against `target` (which holds data_count values; soft targets are FBMS's SE against seg with coefficient 1 / N), a
// target equal to `noneclass` drops the point, and from align_begin on a second term c_align (p - ind)^2 is added with
// ind = [seg > 0.5] (strict: a NaN in seg counts as 0) or seg itself (align_soft).  seg = null: no align term.
struct WideJoint {
    const float* seg;       // [N] or null
    float c_align;
    long long data_count, align_begin;
    int use_noneclass, align_soft;
    float noneclass;
};
// loss and dL/dlogit of ONE point from its logit: the output pass (wide_out_kernel) and the pass that rebuilds dL/dlogits from the
// logits for dL/dcoords (pcn_wide_dy_kernel) evaluate the same expressions.  JOINT = false: SE / BCE against target[p] with the
// class coefficient, or target[p] as dL/dlogit itself (INR_LOSS_EXTERNAL).
template <bool JOINT>
__device__ __forceinline__ void wide_data_term(const float* __restrict__ target, const float* __restrict__ coef, int loss_kind,
                                               const WideJoint& jn, long long p, float y, float& l, float& dy) {
    const float tg = target[JOINT ? (p < jn.data_count ? p : jn.data_count - 1) : p];   // (joint: never past the targets)
    if (!JOINT && loss_kind == INR_LOSS_EXTERNAL) {
        dy = tg;
        return;
    }
    const float pr = 1.f / (1.f + expf(-y));
    const float cw = tg < 0.5f ? coef[0] : coef[1];
    if (loss_kind == INR_LOSS_SE) {
        const float d = tg - pr;
        l = d * d * cw;
        dy = 2.f * (pr - tg) * pr * (1.f - pr) * cw;
    } else {
        const float lp = bce_log(pr), lq = bce_log(1.f - pr);   // clamped at -100, NaN kept (torch.nn.BCELoss)
        l = -(tg * lp + (1.f - tg) * lq) * cw;
        const float pq = pr * (1.f - pr);
        dy = (pr - tg) / fmaxf(pq, 1e-12f) * pq * cw;
    }
    if (JOINT) {
        if (p >= jn.data_count || (jn.use_noneclass && tg == jn.noneclass)) {   // a select: a NaN prior there stays out of the sum
            l = 0.f;
            dy = 0.f;
        }
        if (jn.seg != nullptr && p >= jn.align_begin) align_term(jn.seg + p, jn.c_align, jn.align_soft, pr, l, dy);
    }
}

struct WideOutArgs {
    const float* zl;        // [N][hs]
    const float* wo;        // [h]
    const float* sc;        // b_o, s_o[C]  (flat parameters at p_bo)
    const float* target;    // [N] or null
    const float* coef;      // c_fg, c_bg of this image
    float* logits;          // [N] or null
    float* dz;              // [N][hp] (train)
    float* part;            // [blocks][hsv + 1] output-layer gradient partials, then the block's loss partial (train)
    float* part_ext;        // [blocks][h][1 + C] partials of (db | dS) of the last hidden layer = dZ_L^T (1, X) (train, EXT instantiations)
    long long N;
    int h, C, hs, hp, hsv, loss_kind, train;
    WideJoint jn;           // JOINT instantiations only
};
constexpr int WIDE_OUT_MAXQ = (WIDE_MAX_HIDDEN_PAD + 63) / 64;   // f32x4 per lane and row
// 64-column slices a row may have (register budget of the instantiation); EXT: also dZ_L^T (1, X); JOINT: the data term of a joint step
template <int WIDE_OUT_NQ, bool EXT, bool JOINT = false>
__global__ __launch_bounds__(256) void wide_out_kernel(const WideOutArgs a) {
    __shared__ float sm[4];
    __shared__ float colw[4][5][64];        // per wave: the column sums of one 64-column slice (output layer; (1, x) sums)
    // JOINT: what only the data term and the logits' store read - the joint constants, the target / coefficient / logits pointers, the
    // loss kind - is read from LDS there: seventeen scalar registers less held across the point loop
    __shared__ WideJoint sjn;
    __shared__ const float* s_target;
    __shared__ const float* s_coef;
    __shared__ float* s_logits;
    __shared__ int s_kind;
    const int tid = threadIdx.x, l15 = tid & 15, rg = tid >> 4;      // 16 lanes per point, 16 row groups
    const long long p0 = (long long)blockIdx.x * WIDE_OUT_CHUNK;
    const int nq = (a.hs + 63) / 64;        // 64-column slices of a row (16 lanes x 4 floats)
    if (JOINT) {
        if (tid == 0) {
            sjn = a.jn;
            s_target = a.target;
            s_coef = a.coef;
            s_logits = a.logits;
            s_kind = a.loss_kind;
        }
        __syncthreads();
    }
    f32x4 gacc[WIDE_OUT_NQ];
    f32x4 eacc[EXT ? WIDE_OUT_NQ : 1][4];   // [slice][column of the lane's four] = sum_p dZ_L[p][j] (1, x_p)
#pragma unroll
    for (int q = 0; q < WIDE_OUT_NQ; ++q) gacc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < (EXT ? WIDE_OUT_NQ : 1); ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) eacc[q][e] = f32x4{0.f, 0.f, 0.f, 0.f};
    float lsum = 0.f;
    // the lane's columns: 4 l15 .. + 3 of every 64-column slice; their output weights once (0 past h), the rows of the NEXT 16 points
    // requested (unguarded, from clamped addresses) before this iteration's arithmetic
    f32x4 wq[WIDE_OUT_NQ];
    bool cq[WIDE_OUT_NQ];
#pragma unroll
    for (int q = 0; q < WIDE_OUT_NQ; ++q) {
        const int j = 64 * q + 4 * l15;
        cq[q] = q < nq && j < a.hs;
#pragma unroll
        for (int e = 0; e < 4; ++e) wq[q][e] = j + e < a.h ? a.wo[j + e] : 0.f;
    }
    auto load_row = [&](int it, f32x4 (&z)[WIDE_OUT_NQ]) {
        const long long p = p0 + it * 16 + rg;
        const float* zr = a.zl + (size_t)(p < a.N ? p : 0) * a.hs;
#pragma unroll
        for (int q = 0; q < WIDE_OUT_NQ; ++q) z[q] = *(const f32x4*)(zr + (cq[q] ? 64 * q + 4 * l15 : 0));
    };
    f32x4 zn[WIDE_OUT_NQ];
    load_row(0, zn);
    for (int it = 0; it < WIDE_OUT_CHUNK / 16; ++it) {
        const long long p = p0 + it * 16 + rg;
        const bool valid = p < a.N;
        const float* zr = a.zl + (size_t)(valid ? p : 0) * a.hs;
        f32x4 zq[WIDE_OUT_NQ];
        float ypart = 0.f;
#pragma unroll
        for (int q = 0; q < WIDE_OUT_NQ; ++q) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                zq[q][e] = cq[q] ? zn[q][e] : 0.f;
                ypart = fmaf(wq[q][e], zq[q][e], ypart);
            }
        }
        if (it + 1 < WIDE_OUT_CHUNK / 16) load_row(it + 1, zn);
        ypart = sum_over_points(ypart);     // over the 16 lanes of the point (one DPP row)
        float y = ypart + a.sc[0];
        f32x4 xe = f32x4{1.f, 0.f, 0.f, 0.f};   // the point's ext inputs (1, x)
        for (int c = 0; c < a.C; ++c) {
            xe[1 + c] = zr[a.h + 1 + c];
            y = fmaf(a.sc[1 + c], xe[1 + c], y);
        }
        if (JOINT) {
            if (valid && l15 == 0) s_logits[p] = y;   // (a joint step always writes its logits)
        } else if (a.logits && valid && l15 == 0) a.logits[p] = y;
        if (!JOINT && !a.train) continue;   // (a joint step always trains)
        float l = 0.f, dy = 0.f;
        if (valid) {
            if (JOINT) wide_data_term<true>(s_target, s_coef, s_kind, sjn, p, y, l, dy);
            else wide_data_term<false>(a.target, a.coef, a.loss_kind, a.jn, p, y, l, dy);
        }
        if (l15 == 0) lsum += l;
        float* dr = a.dz + (size_t)(valid ? p : 0) * a.hp;
#pragma unroll
        for (int q = 0; q < WIDE_OUT_NQ; ++q) {
            const int j = 64 * q + 4 * l15;
            if (q < nq && j < a.hs) {
#pragma unroll
                for (int e = 0; e < 4; ++e) gacc[q][e] = fmaf(dy, zq[q][e], gacc[q][e]);   // (dy = 0 for invalid points)
                if (valid && j < a.hp) {
                    f32x4 d;
#pragma unroll
                    for (int e = 0; e < 4; ++e) d[e] = zq[q][e] > 0.f ? dy * wq[q][e] : 0.f;   // (w_o = 0 past h)
                    *(f32x4*)(dr + j) = d;   // hp is a multiple of 4; the padding columns get zeros
                    if (EXT) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) eacc[q][e] += d[e] * xe;
                    }
                }
            }
        }
    }
    if (!JOINT && !a.train) return;
    {   // loss partial of the block: the 16 row groups in order
        const float v = sum_over_groups(sum_over_points(lsum));
        if ((tid & 63) == 0) sm[tid >> 6] = v;
        __syncthreads();
        if (tid == 0) a.part[(size_t)blockIdx.x * (a.hsv + 1) + a.hsv] = ((sm[0] + sm[1]) + sm[2]) + sm[3];   // one more column of the partials
    }
    // column sums over the block's 16 row groups: the four groups of a wave by lane exchange (every lane group then holds the wave's
    // totals; group g keeps column 4 l15 + g), the four waves through LDS, added in order
    const int wv = tid >> 6, gl = (tid >> 4) & 3;
    for (int q = 0; q < nq; ++q) {
        f32x4 gs = f32x4{0.f, 0.f, 0.f, 0.f}, es[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) es[e] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int qq = 0; qq < WIDE_OUT_NQ; ++qq)
            if (qq == q) {
                gs = gacc[qq];
                if (EXT) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) es[e] = eacc[EXT ? qq : 0][e];
                }
            }
        float mine[5] = {0.f, 0.f, 0.f, 0.f, 0.f};   // column 4 l15 + gl: the output-layer sum, then the (1, x) sums
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float t = sum_over_groups(gs[e]);
            mine[0] = gl == e ? t : mine[0];
            if (EXT) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float u = sum_over_groups(es[e][c]);
                    mine[1 + c] = gl == e ? u : mine[1 + c];
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < (EXT ? 5 : 1); ++c) colw[wv][c][4 * l15 + gl] = mine[c];
        __syncthreads();
        if (tid < 64) {
            const int j = 64 * q + tid;
            float t[5];
#pragma unroll
            for (int c = 0; c < (EXT ? 5 : 1); ++c) t[c] = ((colw[0][c][tid] + colw[1][c][tid]) + colw[2][c][tid]) + colw[3][c][tid];
            if (j < a.hsv) a.part[(size_t)blockIdx.x * (a.hsv + 1) + j] = t[0];
            if (EXT && j < a.h)
                for (int c = 0; c <= a.C; ++c) a.part_ext[((size_t)blockIdx.x * a.h + j) * (1 + a.C) + c] = t[1 + c];
        }
    }
}

// The output layer of the general shapes (WideMap::general: n_out <= 4 channels, its own feature width, or no hidden layer), one pass per
// WIDE_OUT_CHUNK points like wide_out_kernel, 16 lanes per point, 16 points per iteration:
//   y_c = w_o[c] . z_L + b_o[c] + s_o[c] . x   -> logits [O][N];   TRAIN: sigmoid, the data term of every channel -> dy [N][4], the
//   block's loss partial;  dZ_L[p][j] = (sum_c dy_c w_o[c][j]) (.) mask  with mask = [z_L > 0], or act0'(pre0) when the output layer reads
//   the periodic features directly (L = 0, PER).
// The row is walked twice (the dot products first, then dZ_L once dy is known; the second walk hits the cache) and the output weights sit
// in LDS, so the registers do not grow with O x the row length.  The output layer's own gradient (dw_o | db_o | ds_o) = dY^T (Z_L | 1 | X)
// is a small split-K GEMM over the points (wide_forward), the (1, x) sums of dZ_L are wide_extgrad_kernel's.
struct WideHeadArgs {
    const float* zl;        // [N][ls]: the hl units of the last activation, then (1, x), then zeros
    const float* wo;        // [O][hl]
    const float* sc;        // b_o [O], s_o [O][C]  (flat parameters at p_bo)
    const float* pre;       // PER: [N][lp] pre-activation of layer 0
    const float* target;    // [O][N] or null
    const float* coef;      // c_fg, c_bg of this image
    float* logits;          // [O][N] or null
    float* dy;              // [N][4] dL/dy_c, zeros past O (train)
    float* dz;              // [N][lp] (train)
    float* lpart;           // [blocks] the blocks' loss partials (train)
    long long N;
    int hl, C, ls, lp, loss_kind, train, act;
    float omega;
};
template <int O, bool PER>
__global__ __launch_bounds__(256) void wide_head_kernel(const WideHeadArgs a) {
    __shared__ __attribute__((aligned(16))) float sw[O][WIDE_OUT_MAXQ * 64];   // output weights, zeros past hl
    __shared__ float sm[4];
    const int tid = threadIdx.x, l15 = tid & 15, rg = tid >> 4;
    const long long p0 = (long long)blockIdx.x * WIDE_OUT_CHUNK;
    const int nq = (a.ls + 63) / 64, row = nq * 64;
    for (int i = tid; i < O * row; i += 256) {
        const int c = i / row, j = i - c * row;
        sw[c][j] = j < a.hl ? a.wo[c * a.hl + j] : 0.f;
    }
    float bo[O], so[O][3];
#pragma unroll
    for (int c = 0; c < O; ++c) {
        bo[c] = a.sc[c];
#pragma unroll
        for (int i = 0; i < 3; ++i) so[c][i] = i < a.C ? a.sc[O + c * a.C + i] : 0.f;
    }
    __syncthreads();
    float lsum = 0.f;
    for (int it = 0; it < WIDE_OUT_CHUNK / 16; ++it) {
        const long long p = p0 + it * 16 + rg;
        const bool valid = p < a.N;
        const float* zr = a.zl + (size_t)(valid ? p : 0) * a.ls;
        float yp[O];
#pragma unroll
        for (int c = 0; c < O; ++c) yp[c] = 0.f;
        for (int q = 0; q < nq; ++q) {
            const int j = 64 * q + 4 * l15;
            if (j < a.ls) {
                const f32x4 z = *(const f32x4*)(zr + j);   // (ls is a multiple of 4)
#pragma unroll
                for (int c = 0; c < O; ++c) {
                    const f32x4 w = *(const f32x4*)(&sw[c][j]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) yp[c] = fmaf(w[e], z[e], yp[c]);
                }
            }
        }
        float x[3] = {0.f, 0.f, 0.f};
        for (int i = 0; i < a.C; ++i) x[i] = zr[a.hl + 1 + i];
        float dyv[O], l = 0.f;
#pragma unroll
        for (int c = 0; c < O; ++c) {
            float y = sum_over_points(yp[c]) + bo[c];   // (over the 16 lanes of the point: every lane has it)
#pragma unroll
            for (int i = 0; i < 3; ++i) y = fmaf(so[c][i], x[i], y);   // (unused channels: 0 * x)
            if (a.logits && valid && l15 == 0) a.logits[(size_t)c * a.N + p] = y;
            float dy = 0.f;
            if (a.train && valid) {
                const float tg = a.target[(size_t)c * a.N + p];
                if (a.loss_kind == INR_LOSS_EXTERNAL) {
                    dy = tg;
                } else {
                    const float pr = 1.f / (1.f + expf(-y));
                    const float cw = tg < 0.5f ? a.coef[0] : a.coef[1];
                    if (a.loss_kind == INR_LOSS_SE) {
                        const float d = tg - pr;
                        l += d * d * cw;
                        dy = 2.f * (pr - tg) * pr * (1.f - pr) * cw;
                    } else {
                        const float lp = bce_log(pr), lq = bce_log(1.f - pr);   // clamped at -100, NaN kept (torch.nn.BCELoss)
                        l += -(tg * lp + (1.f - tg) * lq) * cw;
                        const float pq = pr * (1.f - pr);
                        dy = (pr - tg) / fmaxf(pq, 1e-12f) * pq * cw;
                    }
                }
            }
            dyv[c] = dy;
        }
        if (!a.train) continue;
        if (l15 == 0) lsum += l;
        if (!valid) continue;
        if (l15 == 0) {
            f32x4 d4 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < O; ++c) d4[c] = dyv[c];
            *(f32x4*)(a.dy + (size_t)p * 4) = d4;
        }
        float* dr = a.dz + (size_t)p * a.lp;
        const float* pr0 = PER ? a.pre + (size_t)p * a.lp : nullptr;
        for (int q = 0; q < nq; ++q) {
            const int j = 64 * q + 4 * l15;
            if (j >= a.lp) continue;   // (lp <= ls: the row holds every column of dZ_L)
            const f32x4 z = *(const f32x4*)(zr + j);
            f32x4 d;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = 0.f;
#pragma unroll
                for (int c = 0; c < O; ++c) v = fmaf(dyv[c], sw[c][j + e], v);
                if (PER) {
                    const float pz = j + e < a.hl ? pr0[j + e] : 0.f;   // (pre0's padding columns are never written)
                    v = j + e < a.hl ? v * (a.act == INR_ACT_COS ? -hw_sin(pz) : a.omega * hw_cos(a.omega * pz)) : 0.f;
                } else {
                    v = z[e] > 0.f ? v : 0.f;   // (w_o = 0 past hl: the padding columns get zeros)
                }
                d[e] = v;
            }
            *(f32x4*)(dr + j) = d;
        }
    }
    if (!a.train) return;
    const float v = sum_over_groups(sum_over_points(lsum));   // loss partial of the block: the 16 row groups in order
    if ((tid & 63) == 0) sm[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) a.lpart[blockIdx.x] = ((sm[0] + sm[1]) + sm[2]) + sm[3];
}

// dL/dcoords (an ICNN behind a learned deformation: convex_diffeomorphism_net.py:170-177): every pre-activation gradient dz [N][hp] the
// backward pass produces contributes dz . Wx with Wx [h][C] = the weights the coordinates enter that layer with (S_k of a hidden layer,
// W_in of layer 0); the output layer contributes s_o dL/dlogit (`init`: dx is started from it).  One pass over dz per layer, 16 lanes per
// point; dx is planar [C][N] like the fused kernels' (icnn_step.h, DX).  Only the autograd bridge asks for it.
__global__ __launch_bounds__(256) void wide_dx_kernel(const float* __restrict__ dz, int hp, const float* __restrict__ wx, int h, int C, long long N,
                                                      const float* __restrict__ dlogits, const float* __restrict__ so, float* __restrict__ dx,
                                                      int init, int O = 1) {   // O output channels: dlogits [O][N], s_o [O][C]
    const int l15 = threadIdx.x & 15;
    const long long p = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool valid = p < N;
    const float* row = dz + (size_t)(valid ? p : 0) * hp;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int j = 4 * l15; j < h; j += 64) {
        const f32x4 d = *(const f32x4*)(row + j);      // hp is a multiple of 4; the padding columns hold zeros
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (j + e < h)
                for (int c = 0; c < C; ++c) acc[c] = fmaf(d[e], wx[(j + e) * C + c], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = sum_over_points(acc[c]);
    if (valid && l15 < C) {
        const float a = l15 == 0 ? acc[0] : (l15 == 1 ? acc[1] : acc[2]);
        float* o = dx + (size_t)l15 * N + p;
        float b = init ? so[l15] * dlogits[p] : *o;
        for (int c = 1; init && c < O; ++c) b += so[c * C + l15] * dlogits[(size_t)c * N + p];
        *o = b + a;
    }
}

// gradients w.r.t. everything the "ext" inputs (1, x) multiply - (db_k | dS_k) of a hidden layer, (db_in | dW_in) of layer 0:
//   part[block][i][c] = sum over the block's WIDE_OUT_CHUNK points of dz[p][i] ext_c[p],  ext = (1, x_0 ..)
// A thread owns four consecutive units (one 16-byte load per point), 256 / (hp / 4) points are in flight per block and four loads per
// thread; the row groups are added in order through LDS.
__global__ __launch_bounds__(256) void wide_extgrad_kernel(const float* __restrict__ dz, int hp, const float* __restrict__ ext, int hs, long long N,
                                                           int h, int C, float* __restrict__ part) {
    __shared__ f32x4 red[256][4];
    const int nqc = hp / 4;                         // threads per point row
    const int RL = 256 / nqc > 0 ? 256 / nqc : 1;   // rows in flight (hp <= 1024: nqc <= 256)
    const int tid = threadIdx.x, q = tid % nqc, rl = tid / nqc;
    const long long p0 = (long long)blockIdx.x * WIDE_OUT_CHUNK;
    const long long p1 = p0 + WIDE_OUT_CHUNK < N ? p0 + WIDE_OUT_CHUNK : N;
    f32x4 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (rl < RL) {
#pragma unroll 4
        for (long long p = p0 + rl; p < p1; p += RL) {
            const f32x4 d = *(const f32x4*)(dz + (size_t)p * hp + 4 * q);
            const float* e = ext + (size_t)p * hs;
            acc[0] += d;
            for (int c = 0; c < C; ++c) acc[1 + c] += d * e[1 + c];
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) red[tid][c] = acc[c];
    __syncthreads();
    if (tid < nqc) {
        for (int c = 0; c <= C; ++c) {
            f32x4 t = red[tid][c];
            for (int r = 1; r < RL; ++r) t += red[r * nqc + tid][c];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = 4 * tid + e;
                if (i < h) part[((size_t)blockIdx.x * h + i) * (1 + C) + c] = t[e];
            }
        }
    }
}

// sum of the split-K partials [parts][a][b] in chunk order, scattered into the flat gradient vector:
//   mode 0 (hidden layer k): row i = unit, column j < h -> W_k[i][j]; j == h -> b_k[i]; j > h -> S_k[i][j - h - 1]
//   mode 1 (layer 0, B = the ext columns):           column 0 -> b_in[i]; j >= 1 -> W_in[i][j - 1]
//   mode 3 (hidden layer k, the ext columns only):   column 0 -> b_k[i];  j >= 1 -> S_k[i][j - 1]
//   mode 2 (output layer, a = 1, b = hsv + 1):       column j < h -> w_o[j]; j == h -> b_o; h < j <= h + C -> s_o[j - h - 1]; the last -> the loss
//   mode 4 (output layer of a general shape, a = O, b = hl + 1 + C): row c, column j < hl -> w_o[c][j]; j == hl -> b_o[c]; j > hl -> s_o[c][.]
//   mode 5 (the loss, a = b = 1)
// (mode 0 at layer k: the columns j < kin(k) are W_k - kin(0) = F)
// (one launch takes up to two such reductions - e.g. a layer's weight-gradient partials and the (db | dS) partials its backward GEMM
// left: the first j0.nblocks blocks serve the first)
struct WideRedJob {
    const float* part;
    int parts, a, b, mode, k, nblocks;
};
inline WideRedJob wide_red_job(const float* part, int parts, int a, int b, int mode, int k) {
    return WideRedJob{part, parts, a, b, mode, k, (a * b + 63) / 64};
}
__global__ __launch_bounds__(1024) void wide_reduce_kernel(const WideRedJob j0, const WideRedJob j1, WideMap m, float* __restrict__ grads) {
    // 64 consecutive elements per block, the partials in 16 contiguous ranges (one per wave) summed in order, ranges added in order
    __shared__ float sm[16][64];
    const bool first = (int)blockIdx.x < j0.nblocks;
    const WideRedJob& jb = first ? j0 : j1;
    const float* __restrict__ part = jb.part;
    const int parts = jb.parts, a = jb.a, b = jb.b, mode = jb.mode, k = jb.k;
    const int el = threadIdx.x & 63, pg = threadIdx.x >> 6;
    const int e = ((int)blockIdx.x - (first ? 0 : j0.nblocks)) * 64 + el;
    const int per = (parts + 15) / 16, q0 = pg * per, q1 = q0 + per < parts ? q0 + per : parts;
    float v = 0.f;
    if (e < a * b) {
#pragma unroll 8
        for (int q = q0; q < q1; ++q) v += part[(size_t)q * a * b + e];
    }
    sm[pg][el] = v;
    __syncthreads();
    if (pg != 0 || e >= a * b) return;
    v = sm[0][el];
#pragma unroll
    for (int r = 1; r < 16; ++r) v += sm[r][el];
    const int i = e / b, j = e - i * b;
    int dst;
    const int kin = m.kin(k), hl = m.hl();
    if (mode == 0) dst = j < kin ? m.p_w(k) + i * kin + j : (j == kin ? m.p_b(k) + i : m.p_s(k) + i * m.C + (j - kin - 1));
    else if (mode == 4) dst = j < hl ? m.p_wo() + i * hl + j : (j == hl ? m.p_bo() + i : m.p_so() + i * m.C + (j - hl - 1));
    else if (mode == 5) dst = m.P;
    else if (mode == 3) dst = j == 0 ? m.p_b(k) + i : m.p_s(k) + i * m.C + (j - 1);
    else if (mode == 1) dst = j == 0 ? m.p_bin() + i : m.p_win() + i * m.C + (j - 1);
    else dst = j < m.h ? m.p_wo() + j : (j == m.h ? m.p_bo() : (j <= m.h + m.C ? m.p_so() + (j - m.h - 1) : m.P));   // (last column: the loss)
    grads[dst] = v;
}
inline void wide_reduce(hipStream_t s, const WideMap& m, float* grads, WideRedJob j0, WideRedJob j1 = WideRedJob{nullptr, 0, 0, 0, 0, 0, 0}) {
    hipLaunchKernelGGL(wide_reduce_kernel, dim3((unsigned)(j0.nblocks + j1.nblocks)), dim3(1024), 0, s, j0, j1, m, grads);
}

// ---- workspace --------------------------------------------------------------------------------------------------------------------------
struct WideWs {
    float *z[WIDE_MAX_LAYERS + 1], *pre0, *dza, *dzb, *part, *part2, *grads, *coef, *wp, *dy, *lpart;
    int blocks;            // blocks of wide_out_kernel / wide_head_kernel (WIDE_OUT_CHUNK points each)
    int hs, hp, hsv;       // row length of the activations (multiple of 4), of the dz buffers (multiple of 4), h + 1 + C
    int fs, fp, fsv;       // the same for layer 0 (F features): z[0] rows, pre0 / dZ_0 rows, F + 1 + C  (= hs, hp, hsv when F = h)
    long long bytes;
};

inline long long wide_align(long long b) { return (b + 255) / 256 * 256; }

inline WideWs carve_wide(const WideMap& m, long long N, bool need_pre0, void* base) {
    WideWs w{};
    char* b = (char*)base;
    long long off = 0;
    auto take = [&](long long bytes) { float* p = (float*)(b + off); off += wide_align(bytes); return p; };
    auto mx = [](long long x, long long y) { return x > y ? x : y; };
    w.blocks = out_parts(N);
    w.hsv = m.h + 1 + m.C;
    w.hs = (w.hsv + 3) / 4 * 4;
    w.hp = (m.h + 3) / 4 * 4;
    w.fsv = m.F + 1 + m.C;
    w.fs = (w.fsv + 3) / 4 * 4;
    w.fp = (m.F + 3) / 4 * 4;
    for (int k = 0; k <= m.L; ++k) w.z[k] = take(N * (k == 0 ? w.fs : w.hs) * 4);
    w.pre0 = need_pre0 ? take(N * w.fp * 4) : nullptr;
    w.dza = take(N * mx(w.hp, w.fp) * 4);
    w.dzb = take(N * mx(w.hp, w.fp) * 4);
    long long part_gemm = m.L > 0 ? (long long)splitk_parts(N, m.h) * m.h * mx(m.h, m.F) : 0;
    long long part_out = (long long)w.blocks * (w.hsv + 1 > m.h * (1 + m.C) ? w.hsv + 1 : m.h * (1 + m.C));
    if (m.general()) part_out = (long long)splitk_parts(N, m.O) * m.O * (m.hl() + 1 + m.C);   // the output layer's GEMM partials
    w.part = take(mx(part_gemm, part_out) * 4);
    {   // (db | dS) partials: one [h][1 + C] block per wide_out_kernel block / per 128-row tile of the backward GEMM
        const long long tiles = (N + GM_BM - 1) / GM_BM;
        w.part2 = take(mx(w.blocks, tiles) * mx(m.h, m.F) * (1 + m.C) * 4);
    }
    w.grads = take(((long long)m.P + 1 + 31) / 32 * 32 * 4);
    w.wp = take(wide_wp_off(m, m.L) * 4);
    w.dy = m.general() ? take(N * 4 * 4) : nullptr;
    w.lpart = m.general() ? take((long long)w.blocks * 4) : nullptr;
    w.coef = nullptr;
    w.bytes = off;
    return w;
}

inline long long wide_total_bytes(const WideMap& m, long long N, bool pre0, int n_images) {   // + the per-image loss coefficients
    return carve_wide(m, N, pre0, nullptr).bytes + wide_align((long long)n_images * 2 * 4);
}

// the descriptor's own feature width / output count, 0 = today's meaning (F = h, O = 1)
inline int wide_desc_F(const InrModelDesc* md) { return md->n_features > 0 ? md->n_features : md->n_hidden; }
inline int wide_desc_O(const InrModelDesc* md) { return md->n_out > 0 ? md->n_out : 1; }
inline bool wide_desc_general(const InrModelDesc* md) {
    return wide_desc_F(md) != md->n_hidden || wide_desc_O(md) != 1 || md->n_layers == 0;
}
inline bool wide_shape_ok(const InrModelDesc* md) {
    if (!md || md->kind != INR_MODEL_ICNN || md->n_hidden < 1 || md->n_hidden > WIDE_MAX_HIDDEN || md->n_layers < 0 ||
        md->n_layers > WIDE_MAX_LAYERS || (md->in_features != 2 && md->in_features != 3))
        return false;
    if (md->n_features < 0 || md->n_features > WIDE_MAX_HIDDEN || md->n_out < 0 || md->n_out > 4) return false;
    // no hidden layer: only behind a periodic encode (the sine net's direct read-out); a relu layer 0 + read-out is not an ICNN shape
    return md->n_layers >= 1 || md->act0 == INR_ACT_COS || md->act0 == INR_ACT_SIN;
}

#define WIDE_EW(n) dim3((unsigned)(((n) + 255) / 256)), dim3(256), 0, s

// rows short enough for the wide_out_kernel instantiations that also sum dZ_L^T (1, X) (16 more accumulators per 64-column slice)
inline bool wide_out_has_ext(int hs) { return hs <= 9 * 64; }

// the output layer of a general shape: wide_head_kernel, and with `train` the output layer's gradient (a GEMM over the points), the
// (1, x) sums of dZ_L (the (db | dS) of the last hidden layer, or (db_in | dW_in) when the output layer reads the features) and the loss
inline int wide_head(const WideMap& m, const WideWs& w, const InrModelDesc* md, const float* params, long long N, const float* target,
                     int loss_kind, bool train, float* logits, hipStream_t s) {
    const int L = m.L, hl = m.hl(), C = m.C;
    const int ls = L > 0 ? w.hs : w.fs, lp = L > 0 ? w.hp : w.fp;
    WideHeadArgs a{};
    a.zl = w.z[L]; a.wo = params + m.p_wo(); a.sc = params + m.p_bo(); a.pre = w.pre0; a.target = target; a.coef = w.coef; a.logits = logits;
    a.dy = w.dy; a.dz = w.dza; a.lpart = w.lpart;
    a.N = N; a.hl = hl; a.C = C; a.ls = ls; a.lp = lp; a.loss_kind = loss_kind; a.train = train ? 1 : 0; a.act = md->act0; a.omega = md->act_omega;
#define WIDE_HEAD_GO(O_)                                                                                                   \
    do {                                                                                                                   \
        if (L == 0) hipLaunchKernelGGL((wide_head_kernel<O_, true>), dim3(w.blocks), dim3(256), 0, s, a);                  \
        else hipLaunchKernelGGL((wide_head_kernel<O_, false>), dim3(w.blocks), dim3(256), 0, s, a);                        \
    } while (0)
    if (m.O == 1) WIDE_HEAD_GO(1);
    else if (m.O == 2) WIDE_HEAD_GO(2);
    else if (m.O == 3) WIDE_HEAD_GO(3);
    else WIDE_HEAD_GO(4);
#undef WIDE_HEAD_GO
    if (!train) return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
    {   // (dw_o | db_o | ds_o) [O][hl + 1 + C] = dY^T (Z_L | 1 | X): dY [N][4] is the A operand stored along its free index (its fourth
        // column holds zeros), the rows of Z_L carry their ext columns; split over the points like the hidden layers' weight gradients
        GemmArgs g{};
        g.A = w.dy; g.lda = 4; g.B = w.z[L]; g.ldb = ls; g.C = w.part; g.ldc = hl + 1 + C;
        g.M = m.O; g.N = hl + 1 + C; g.K = (int)N; g.k_per_split = wide_chunk(m.O); g.c_split_stride = (long long)m.O * (hl + 1 + C);
        g.padA = g.padB = 1; g.buf = 1;
        if (const int rc = gemm_launch(s, true, false, g)) return rc;
    }
    hipLaunchKernelGGL(wide_extgrad_kernel, dim3(w.blocks), dim3(256), 0, s, (const float*)w.dza, lp, (const float*)(w.z[L] + hl), ls, N, hl, C, w.part2);
    const int parts = splitk_parts(N, m.O);
    wide_reduce(s, m, w.grads, wide_red_job(w.part, parts, m.O, hl + 1 + C, 4, 0),
                wide_red_job(w.part2, w.blocks, hl, 1 + C, L > 0 ? 3 : 1, L > 0 ? L - 1 : 0));
    wide_reduce(s, m, w.grads, wide_red_job(w.lpart, w.blocks, 1, 1, 5, 0));
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

// forward of ONE image; with `train`: also dZ_L (w.dza), the output layer's gradients and the loss (w.grads)
inline int wide_forward(const WideMap& m, const WideWs& w, const InrModelDesc* md, const float* params, const InrGridDesc* grid, int img,
                        const float* target, int loss_kind, bool train, float* logits, hipStream_t s, const WideJoint* jn = nullptr) {
    const long long N = grid->n_points;
    const int h = m.h, C = m.C, hs = w.hs;
    // layer 0 at width F (+ in the launch's last blocks: the padded copy of the hidden layers' weights)
    const int pt_blocks = (int)((N + WIDE_L0_POINTS * WIDE_L0_REP - 1) / (WIDE_L0_POINTS * WIDE_L0_REP));
    const unsigned l0y = (unsigned)((WIDE_L0_POINTS * (w.fs / 4) + 255) / 256);
    const int hq = wide_q16(h);   // row count of a packed weight matrix (and column count of layers k >= 1)
    const int pk_blocks = (int)((wide_wp_off(m, m.L) + 256ll * l0y - 1) / (256ll * l0y));
    const dim3 l0grid((unsigned)(pt_blocks + pk_blocks), l0y);
    if (C == 2) hipLaunchKernelGGL(wide_layer0_kernel<2>, l0grid, dim3(256), 0, s, *grid, img, params + m.p_win(), params + m.p_bin(), N, m.F, w.fs, w.fp, md->act0, md->act_omega, w.z[0], w.pre0, pt_blocks, params, m, w.wp);
    else hipLaunchKernelGGL(wide_layer0_kernel<3>, l0grid, dim3(256), 0, s, *grid, img, params + m.p_win(), params + m.p_bin(), N, m.F, w.fs, w.fp, md->act0, md->act_omega, w.z[0], w.pre0, pt_blocks, params, m, w.wp);
    for (int k = 0; k < m.L; ++k) {
        // z_{k+1} [N x h] = relu(z_k [N x kin] . W_k^T + b_k + S_k x)   (W_k stored [h_out][h_in]; bias, skip and relu in the GEMM's epilogue;
        // kin = F for k = 0)
        const int kin = m.kin(k), ks = k == 0 ? w.fs : hs;
        GemmArgs g{};
        g.A = w.z[k]; g.lda = ks; g.B = w.wp + wide_wp_off(m, k); g.ldb = k == 0 ? wide_q16(m.F) : hq; g.C = w.z[k + 1]; g.ldc = hs;
        g.M = (int)N; g.N = h; g.K = kin; g.padA = g.padB = 1; g.buf = 1;
        g.epi = GEMM_EPI_HIDDEN; g.bias = params + m.p_b(k); g.skip = params + m.p_s(k); g.ext = w.z[k] + kin; g.ext_ld = ks; g.C_in = C; g.ext_copy = hs - h;
        int rc = gemm_launch(s, false, true, g);
        if (rc) return rc;
    }
    if (m.general()) return wide_head(m, w, md, params, N, target, loss_kind, train, logits, s);
    WideOutArgs a{};
    a.zl = w.z[m.L]; a.wo = params + m.p_wo(); a.sc = params + m.p_bo(); a.target = target; a.coef = w.coef; a.logits = logits;
    a.dz = w.dza; a.part = w.part;
    a.N = N; a.h = h; a.C = C; a.hs = hs; a.hp = w.hp; a.hsv = w.hsv; a.loss_kind = loss_kind; a.train = train ? 1 : 0;
    a.part_ext = w.part2;
#define WIDE_OUT_GO(NQ_, EXT_)                                                                                              \
    do {                                                                                                                    \
        if (jn) hipLaunchKernelGGL((wide_out_kernel<NQ_, EXT_, true>), dim3(w.blocks), dim3(256), 0, s, a);                 \
        else hipLaunchKernelGGL((wide_out_kernel<NQ_, EXT_>), dim3(w.blocks), dim3(256), 0, s, a);                          \
    } while (0)
    if (jn) a.jn = *jn;   // (a joint step's data term: an ICNN-form shape in training)
    if (hs <= 5 * 64) WIDE_OUT_GO(5, true);
    else if (hs <= 6 * 64) WIDE_OUT_GO(6, true);   // (h = 350: no AGPR spills)
    else if (hs <= 7 * 64) WIDE_OUT_GO(7, true);
    else if (hs <= 9 * 64) WIDE_OUT_GO(9, true);
    else WIDE_OUT_GO(WIDE_OUT_MAXQ, false);
#undef WIDE_OUT_GO
    if (train) {
        // (dw_o | db_o | ds_o | loss), and (db | dS) of the last hidden layer = dZ_L^T (1, X) where the same pass summed it
        const WideRedJob jo = wide_red_job(w.part, w.blocks, 1, w.hsv + 1, 2, 0);
        if (wide_out_has_ext(hs)) wide_reduce(s, m, w.grads, jo, wide_red_job(w.part2, w.blocks, h, 1 + C, 3, m.L - 1));
        else wide_reduce(s, m, w.grads, jo);
    }
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

// backward of ONE image from dZ_L (w.dza, written by wide_forward): every remaining parameter gradient into w.grads (flat order).
// need_dz0 = false (general shapes only): dZ_0 and with it (db_in | dW_in) are not computed - the fit of frozen Fourier features.
inline int wide_backward(const WideMap& m, const WideWs& w, const InrModelDesc* md, const float* params, long long N, hipStream_t s,
                         const float* dlogits = nullptr, float* dcoords = nullptr,   // dcoords [C][N] (with dlogits = dL/dlogits): also dL/dcoords
                         bool need_dz0 = true) {
    const int h = m.h, C = m.C, hs = w.hs, hp = w.hp, parts = splitk_parts(N, h);
    const bool gen = m.general();
    float* gr = w.grads;
    int rc;
    float *dz = w.dza, *dzn = w.dzb;
    const int tiles = (int)((N + GM_BM - 1) / GM_BM), hq = wide_q16(h);
    const dim3 dxgrid((unsigned)((N + 15) / 16));
    if (dcoords) {   // s_o dL/dlogit + dZ_L . S_{L-1}  (L = 0: dZ_0 . W_in)
        if (m.L > 0)
            hipLaunchKernelGGL(wide_dx_kernel, dxgrid, dim3(256), 0, s, dz, hp, params + m.p_s(m.L - 1), h, C, N, dlogits, params + m.p_so(), dcoords, 1, m.O);
        else
            hipLaunchKernelGGL(wide_dx_kernel, dxgrid, dim3(256), 0, s, dz, w.fp, params + m.p_win(), m.F, C, N, dlogits, params + m.p_so(), dcoords, 1, m.O);
    }
    for (int k = m.L - 1; k >= 0; --k) {
        const int kin = m.kin(k), ks = k == 0 ? w.fs : hs, kp = k == 0 ? w.fp : hp;   // layer k's input width, its activation / dz rows
        {   // dW_k [h x kin] = dz^T Z_k: the contraction over the points, split into chunks of WIDE_CHUNK
            GemmArgs g{};
            g.A = dz; g.lda = hp; g.B = w.z[k]; g.ldb = ks; g.C = w.part; g.ldc = kin;
            g.M = h; g.N = kin; g.K = (int)N; g.k_per_split = wide_chunk(h); g.c_split_stride = (long long)h * kin; g.padA = g.padB = 1; g.buf = 1;
            if ((rc = gemm_launch(s, true, false, g))) return rc;   // (its partials are added up with the (1, x) sums below: one launch)
            // (db_k | dS_k) = dz^T (1, X): summed by the kernel that wrote dz (wide_out_kernel / wide_head for the last layer, the backward
            // GEMM's epilogue below for the others); only rows too long for wide_out_kernel's accumulators take a pass of their own
            if (!gen && k == m.L - 1 && !wide_out_has_ext(hs)) {
                hipLaunchKernelGGL(wide_extgrad_kernel, dim3(w.blocks), dim3(256), 0, s, dz, hp, w.z[k] + h, hs, N, h, C, w.part2);
                wide_reduce(s, m, gr, wide_red_job(w.part2, w.blocks, h, 1 + C, 3, k));
            }
        }
        if (k == 0 && gen && !need_dz0) {   // frozen input layer, no coordinate gradient: dW_0 is the last product
            wide_reduce(s, m, gr, wide_red_job(w.part, parts, h, kin, 0, k));
            break;
        }
        {   // dz_k = (dz W_k) (.) act'(layer k)     (the mask in the GEMM's epilogue, and dz_k^T (1, X) per 128-row tile)
            GemmArgs g{};
            g.A = dz; g.lda = hp; g.B = w.wp + wide_wp_off(m, k); g.ldb = k == 0 ? wide_q16(m.F) : hq; g.C = dzn; g.ldc = kp;   // (the weights wide_forward packed)
            g.M = (int)N; g.N = kin; g.K = h; g.padA = g.padB = 1; g.buf = 1; g.c_zero_to = kp;
            g.epi = GEMM_EPI_MASK;
            const int act = k == 0 ? md->act0 : INR_ACT_RELU;
            g.mask_act = act; g.omega = md->act_omega;
            if (act == INR_ACT_RELU) { g.mask = w.z[k]; g.mask_ld = ks; }
            else { g.mask = w.pre0; g.mask_ld = w.fp; }
            g.extsum = w.part2; g.ext = w.z[k] + kin; g.ext_ld = ks; g.C_in = C;
            if ((rc = gemm_launch(s, false, false, g))) return rc;
            // what the ext inputs multiply in the layer below: (db_{k-1} | dS_{k-1}), or (db_in | dW_in) of layer 0
            wide_reduce(s, m, gr, wide_red_job(w.part, parts, h, kin, 0, k), wide_red_job(w.part2, tiles, kin, 1 + C, k > 0 ? 3 : 1, k > 0 ? k - 1 : 0));
            if (dcoords)   // ... and what the coordinates multiply there: S_{k-1}, or W_in
                hipLaunchKernelGGL(wide_dx_kernel, dxgrid, dim3(256), 0, s, dzn, kp, params + (k > 0 ? m.p_s(k - 1) : m.p_win()), kin, C, N, dlogits,
                                   params + m.p_so(), dcoords, 0, m.O);
        }
        float* t = dz; dz = dzn; dzn = t;
    }
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

}  // namespace
