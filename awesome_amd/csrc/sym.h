// sym.h - the pose of the rotation / mirror-symmetry prior of the teaser as a deformation in front of the ICNN backbones (SURVEY.md §8
// f4; notebooks/icml_teaser_code/rotation_symmetric/rotation_symmetric.ipynb cells 2-3).
//
//     x' = x + offset,  r = |x'|,  n = x' / (eps + r)                    eps = 0.001 in the notebook
//     u  = n0 cos(th) - n1 sin(th),  v0 = n0 sin(th) + n1 cos(th),  v = mirror ? |v0| : v0
//     features (u, v, r) -> the network 3 -> h -> h -> 1
//
// The pose is three numbers per image, (offset0, offset1, orientation): the learned symmetry axis.  Three kernels, each a few
// operations per point: the features, the chain rule back to the pose as per-block partial sums, and the sums + torch's single-tensor
// Adam on the three parameters.  No atomics, every sum in a fixed order: the same bits on every run.  The backward pass recomputes
// the point's polar split from its two coordinates (8 bytes read) instead of keeping x', r and 1 / (eps + r) (16 bytes written and
// read); it is the same arithmetic on the same numbers as the forward pass, so it is the same values.
//
// Included by inrfit.hip behind star.h (wave_sum).  The "frozen" decision of a step is read from the flag the ICNN update has written
// into its header one launch earlier, as FlowDeform's separate update launch reads it.
#pragma once

namespace {

constexpr int SYM_POSE = 3;   // offset[2] | orientation

struct SymPoint {
    float x0, x1, r, q;   // x', |x'|, 1 / (eps + r)
    float c, s;           // cos / sin of the orientation
    float u, v0;
};

__device__ __forceinline__ void sym_load_coords(const InrGridDesc& gd, const int img, const long long N, const long long p, float& x0,
                                                float& x1) {
    if (gd.mode == INR_GRID_SEPARABLE) {
        const long long row = p / gd.width;
        x0 = gd.xs[p - row * gd.width];
        x1 = gd.ys[row];
    } else {
        const float* cp = gd.coords + (size_t)img * gd.coords_image_stride;
        x0 = cp[p];
        x1 = cp[(size_t)N + p];
    }
}

// the polar split and the rotation of one point: what the forward writes and the backward differentiates
__device__ __forceinline__ SymPoint sym_point(const float x0, const float x1, const float* __restrict__ pose, const float eps) {
    SymPoint t;
    t.x0 = __fadd_rn(x0, pose[0]);
    t.x1 = __fadd_rn(x1, pose[1]);
    t.r = __fsqrt_rn(__fadd_rn(__fmul_rn(t.x0, t.x0), __fmul_rn(t.x1, t.x1)));
    const float den = __fadd_rn(eps, t.r);
    t.q = __fdiv_rn(1.f, den);
    const float n0 = __fdiv_rn(t.x0, den), n1 = __fdiv_rn(t.x1, den);
    t.c = cosf(pose[2]);
    t.s = sinf(pose[2]);
    t.u = __fsub_rn(__fmul_rn(n0, t.c), __fmul_rn(n1, t.s));
    t.v0 = __fadd_rn(__fmul_rn(n0, t.s), __fmul_rn(n1, t.c));
    return t;
}

struct SymFwdArgs {
    InrGridDesc grid;    // the caller's 2-channel grid
    const float* pose;   // [n_images][3]
    float* xd;           // [n_images][3][N]: the backbone's explicit grid
    long long N;
    float eps;
    int mirror;
};

// thread = point; grid (ceil(N / 256), n_images)
__global__ __launch_bounds__(256) void sym_fwd_kernel(const SymFwdArgs a) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    const int img = blockIdx.y;
    if (p >= a.N) return;
    float x0, x1;
    sym_load_coords(a.grid, img, a.N, p, x0, x1);
    const SymPoint t = sym_point(x0, x1, a.pose + (size_t)img * SYM_POSE, a.eps);
    float* o = a.xd + (size_t)img * 3 * a.N;
    o[p] = t.u;
    o[(size_t)a.N + p] = a.mirror ? fabsf(t.v0) : t.v0;
    o[2 * (size_t)a.N + p] = t.r;
}

struct SymBwdArgs {
    InrGridDesc grid;
    const float* pose;   // [n_images][3]
    const float* dxd;    // [n_images][3][N]: dL / d(u, v, r) from the backbone
    float* part;         // [n_images][blocks][3]: (d offset0, d offset1, d orientation) of the block's points
    long long N;
    float eps;
    int mirror, blocks;
};

// thread = point; the block's three sums: butterfly inside a wave, the four waves in order
__global__ __launch_bounds__(256) void sym_bwd_kernel(const SymBwdArgs a) {
    __shared__ float sh[4][SYM_POSE];
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    const int img = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float g[SYM_POSE] = {0.f, 0.f, 0.f};
    if (p < a.N) {
        float x0, x1;
        sym_load_coords(a.grid, img, a.N, p, x0, x1);
        const SymPoint t = sym_point(x0, x1, a.pose + (size_t)img * SYM_POSE, a.eps);
        const float* d = a.dxd + (size_t)img * 3 * a.N;
        const float gu = d[p], gv = d[(size_t)a.N + p], gr = d[2 * (size_t)a.N + p];
        // torch's abs: sign(0) = 0
        const float gv0 = a.mirror ? (t.v0 > 0.f ? gv : (t.v0 < 0.f ? -gv : 0.f)) : gv;
        // a point at the centre (r == 0) has no direction: it contributes nothing (torch yields NaN there)
        if (t.r > 0.f) {
            g[2] = __fsub_rn(__fmul_rn(gv0, t.u), __fmul_rn(gu, t.v0));
            const float gn0 = __fadd_rn(__fmul_rn(gu, t.c), __fmul_rn(gv0, t.s));
            const float gn1 = __fsub_rn(__fmul_rn(gv0, t.c), __fmul_rn(gu, t.s));
            const float dot = __fadd_rn(__fmul_rn(gn0, t.x0), __fmul_rn(gn1, t.x1));
            // d / dx' of (n, r):  q gn  +  (gr - q^2 (gn . x')) x' / r
            const float k = __fdiv_rn(__fsub_rn(gr, __fmul_rn(__fmul_rn(t.q, t.q), dot)), t.r);
            g[0] = __fadd_rn(__fmul_rn(t.q, gn0), __fmul_rn(k, t.x0));
            g[1] = __fadd_rn(__fmul_rn(t.q, gn1), __fmul_rn(k, t.x1));
        }
    }
#pragma unroll
    for (int k = 0; k < SYM_POSE; ++k) {
        const float v = wave_sum(g[k]);
        if (lane == 0) sh[wv][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < SYM_POSE)
        a.part[((size_t)img * a.blocks + blockIdx.x) * SYM_POSE + threadIdx.x] =
            ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

struct SymUpdArgs {
    float* pose;            // [n_images][3] in place (mode 0)
    float* opt;             // [n_images][6] exp_avg[3] | exp_avg_sq[3] (mode 0)
    float* grads_out;       // [n_images][3] (mode 1)
    const float* part;      // [n_images][blocks][3]
    const float* lr_hdr;    // ICNN opt-state header of image 0: this step's lr and the "frozen" flag its update has written (optim.h)
    long long hdr_stride;
    const int32_t* status;  // per image, or null
    const float* gscale;    // [n_images] factor on the gradient (a joint step's detached clip factor), or null
    int blocks, t, mode;    // mode 0 = Adam step, 1 = gradients only
    OptConsts c;
    float wd;
};

// One wave per image; thread k < 3 owns pose parameter k: its block partials added in block order, then torch.optim.Adam's
// single-tensor step in torch's operation order (optim.h's adam_step).  An image the ICNN update of this step has frozen (a
// non-finite loss, now or earlier in the call) keeps its pose and its moments.
__global__ __launch_bounds__(64) void sym_update_kernel(const SymUpdArgs u) {
    const int img = blockIdx.x, k = threadIdx.x;
    if (k >= SYM_POSE) return;
    const float* q = u.part + (size_t)img * u.blocks * SYM_POSE + k;
    float g = 0.f;
    for (int b = 0; b < u.blocks; ++b) g += q[(size_t)b * SYM_POSE];
    if (u.mode == 1) {
        u.grads_out[(size_t)img * SYM_POSE + k] = g;
        return;
    }
    const float gmul = u.gscale != nullptr ? u.gscale[img] : 1.f;
    __builtin_assume(u.lr_hdr != nullptr);   // a pose never steps without the ICNN header: no null tests between the loads below
    if (deformation_frozen(gmul, nullptr, 0, 0, u.lr_hdr, u.hdr_stride, u.status, u.t, img, k)) return;   // (the ICNN update ran one launch earlier)
    const float lr = opt_hdr_lr(u.lr_hdr, u.hdr_stride, img, u.t, 0.f);
    float* pp = u.pose + (size_t)img * SYM_POSE + k;
    float* mp = u.opt + (size_t)img * 2 * SYM_POSE + k;
    float* vp = mp + SYM_POSE;
    float m = *mp, v = *vp;
    *pp = adam_step(u.c, opt_step_size(lr, u.c.bc1), u.wd, g * gmul, *pp, m, v);   // (x 1.0 is exact)
    *mp = m;
    *vp = v;
}

}  // namespace
