// optim.h - the ONE definition of an optimizer step and of the per-image optimizer header for every update kernel of the library
// (icnn_update_body, flow_update_body, rnvp_update_body, sym_update_kernel, star_update_kernel, star_dense_update_kernel).
//
//   * the header's slots by name (layout: include/inrfit.h, INR_OPT_HEADER_FLOATS) - nobody else indexes a header with a number;
//   * OptConsts / opt_consts(): what a step needs of (InrOptDesc, t), computed on the host in double like torch does;
//   * adam_step / adamax_step / opt_step: torch.optim.Adam / Adamax, single-tensor arithmetic in torch's operation order, on values
//     the caller has loaded (no loads, no stores: the callers keep the order of their own memory requests);
//   * opt_header_step: loss slot, "frozen" flag of the next step, ReduceLROnPlateau (torch semantics), the next step's learning rate;
//   * the "this image takes no step" decisions: frozen_in_launch (from the loss partials of THIS launch) and deformation_frozen
//     (what a deformation's or a pose's update asks behind or next to the ICNN update).
#pragma once
#include "icnn_step.h"

namespace {

// ---- header slots ---------------------------------------------------------------------------------------------------------------------
// The learning rate and the "frozen by a non-finite loss" flag are double buffers: step t (1-based) READS slot [t & 1] - what the step
// before it, or opt_init_kernel, left there - and WRITES the other one, so no block of a launch reads what another block of the same
// launch writes.
constexpr int OPT_HDR_LR = 2;        // current learning rate
constexpr int OPT_HDR_BEST = 3;      // plateau best
constexpr int OPT_HDR_NUM_BAD = 4;   // plateau num_bad (as float)
constexpr int OPT_HDR_LOSS = 5;      // last loss
__host__ __device__ constexpr int opt_hdr_lr_of(int t) { return t & 1; }                     // learning rate step t takes
__host__ __device__ constexpr int opt_hdr_lr_next(int t) { return (t + 1) & 1; }             // ... and the one it leaves for step t + 1
__host__ __device__ constexpr int opt_hdr_frozen_before(int t) { return 6 + (t & 1); }       // flag step t reads: frozen by an earlier step
__host__ __device__ constexpr int opt_hdr_frozen_next(int t) { return 6 + ((t + 1) & 1); }   // flag step t writes for step t + 1
// the same slot, read by an update that runs BEHIND the ICNN update of step t (one launch later on the stream): "frozen at step t"
__host__ __device__ constexpr int opt_hdr_frozen_by_update(int t) { return opt_hdr_frozen_next(t); }
// both flags: "frozen" is a property of one call, like `status`
__device__ __forceinline__ void opt_hdr_clear_frozen(float* hdr) { hdr[opt_hdr_frozen_before(0)] = hdr[opt_hdr_frozen_before(1)] = 0.f; }

// learning rate of step t of image img from the ICNN header (hdr0 = image 0's, hdr_stride floats per image), or `fallback` without one
__device__ __forceinline__ float opt_hdr_lr(const float* hdr0, const long long hdr_stride, const int img, const int t, const float fallback) {
    return hdr0 ? hdr0[(size_t)img * hdr_stride + opt_hdr_lr_of(t)] : fallback;
}

// ---- per-step constants ---------------------------------------------------------------------------------------------------------------
struct OptConsts {
    double bc1;        // 1 - beta1^t
    float bc2_sqrt;    // sqrt(1 - beta2^t)
    float one_minus_b1, one_minus_b2, beta2, eps;
};
// t: 1-based step count of the parameters this struct is for.  No descriptor or t == 0 (gradients only, effective weights only, a
// parameter that does not step yet): zeros, never used for a step.
inline OptConsts opt_consts(const InrOptDesc* opt, int t) {
    OptConsts c{};
    if (!opt || t <= 0) return c;
    c.bc1 = 1.0 - pow((double)opt->beta1, (double)t);
    c.bc2_sqrt = (float)sqrt(1.0 - pow((double)opt->beta2, (double)t));
    c.one_minus_b1 = (float)(1.0 - (double)opt->beta1);
    c.one_minus_b2 = (float)(1.0 - (double)opt->beta2);
    c.beta2 = opt->beta2;
    c.eps = opt->eps;
    return c;
}

// ---- the element step -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float opt_step_size(const float lr, const double bc1) { return (float)((double)lr / bc1); }

// torch.optim.Adam: returns the new parameter, m / v = exp_avg / exp_avg_sq in and out
__device__ __forceinline__ float adam_step(const OptConsts& c, const float step_size, const float wd, float g, const float p, float& m, float& v) {
    if (wd != 0.f) g = __fadd_rn(g, __fmul_rn(wd, p));
    m = __fadd_rn(m, __fmul_rn(c.one_minus_b1, __fsub_rn(g, m)));                                  // exp_avg.lerp_(grad, 1 - beta1)
    v = __fadd_rn(__fmul_rn(v, c.beta2), __fmul_rn(__fmul_rn(c.one_minus_b2, g), g));              // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1-beta2)
    const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), c.bc2_sqrt), c.eps);
    return __fadd_rn(p, __fdiv_rn(__fmul_rn(-step_size, m), denom));
}
// torch.optim.Adamax: v = exp_inf = max(beta2 exp_inf, |grad| + eps); p -= lr / bc1 * m / exp_inf
__device__ __forceinline__ float adamax_step(const OptConsts& c, const float step_size, const float wd, float g, const float p, float& m, float& v) {
    if (wd != 0.f) g = __fadd_rn(g, __fmul_rn(wd, p));
    m = __fadd_rn(m, __fmul_rn(c.one_minus_b1, __fsub_rn(g, m)));
    v = fmaxf(__fmul_rn(v, c.beta2), __fadd_rn(fabsf(g), c.eps));
    return __fadd_rn(p, __fdiv_rn(__fmul_rn(-step_size, m), v));
}
__device__ __forceinline__ float opt_step(const int kind, const OptConsts& c, const float step_size, const float wd, const float g, const float p,
                                          float& m, float& v) {
    return kind == INR_OPT_ADAM ? adam_step(c, step_size, wd, g, p, m, v) : adamax_step(c, step_size, wd, g, p, m, v);
}

// ---- the header's share of a step (one thread per image) ------------------------------------------------------------------------------
// Loss bookkeeping, the flag step t + 1 reads, ReduceLROnPlateau (torch semantics, mode 'min', relative threshold) and the learning
// rate of the NEXT step (the scheduler steps after the optimizer).  lr_now = hdr[opt_hdr_lr_of(t)], loaded by the caller.
__device__ __forceinline__ void opt_header_step(float* __restrict__ hdr, const InrOptDesc& opt, const int t, const float loss, const bool frozen,
                                                const float lr_now, float* loss_hist_slot, int32_t* status_slot) {
    if (loss_hist_slot) *loss_hist_slot = loss;
    float lr = lr_now;
    hdr[opt_hdr_frozen_next(t)] = frozen ? 1.f : 0.f;
    if (frozen) {
        if (status_slot) *status_slot = INR_STATUS_NONFINITE;
    } else if (opt.plateau) {
        float best = hdr[OPT_HDR_BEST];
        int num_bad = (int)hdr[OPT_HDR_NUM_BAD];
        if (loss < best * (1.f - opt.plateau_threshold)) {
            best = loss;
            num_bad = 0;
        } else {
            num_bad += 1;
        }
        if (num_bad > opt.plateau_patience) {
            const float nlr = fmaxf(lr * opt.plateau_factor, opt.plateau_min_lr);
            if (lr - nlr > opt.plateau_eps) lr = nlr;
            num_bad = 0;
        }
        hdr[OPT_HDR_BEST] = best;
        hdr[OPT_HDR_NUM_BAD] = (float)num_bad;
    }
    hdr[opt_hdr_lr_next(t)] = lr;
    hdr[OPT_HDR_LR] = lr;
    hdr[OPT_HDR_LOSS] = loss;
}

// ---- "this image takes no step" -------------------------------------------------------------------------------------------------------
// The loss of one image = the sum of its workgroups' loss partials, in the order icnn_update_kernel uses: 16 groups (group g takes the
// workgroups g, g + 16, ...), then the groups in order.  One definition for every kernel that needs the "non-finite loss" decision.
// `sl` = the partial of workgroup 0, `stride` = floats from one workgroup's partial to the next: 1 for the step kernels' dense copy
// (StepArgs::loss_part: 256 partials are 8 lines), the slab stride for a loss column read in place (the one-slab views of wide.h).
constexpr int LOSS_GROUPS = 16;
__device__ __forceinline__ float loss_column_group_sum(const float* __restrict__ sl, const int wgs, const size_t stride, const int grp) {
    float lp = 0.f;
    int w = grp;
    for (; w + 15 * LOSS_GROUPS < wgs; w += 16 * LOSS_GROUPS) {   // 256 slabs: one trip, 16 loads in flight
        float q[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) q[k] = sl[(size_t)(w + k * LOSS_GROUPS) * stride];
#pragma unroll
        for (int k = 0; k < 16; ++k) lp += q[k];
    }
    for (; w < wgs; w += LOSS_GROUPS) lp += sl[(size_t)w * stride];
    return lp;
}

// Exactly as the ICNN update of the same launch decides it: frozen by an earlier step (the flag the PREVIOUS launch wrote) or a
// non-finite loss now.  Called by the first 256 threads of a block.
__device__ __forceinline__ bool frozen_in_launch(const float* __restrict__ loss_part, const int wgs, const long long stride,
                                                 const float* __restrict__ hdr0, const long long hdr_stride, const int t, const int img,
                                                 const int tid) {
    __shared__ float redl[LOSS_GROUPS];
    if (tid < LOSS_GROUPS) redl[tid] = loss_column_group_sum(loss_part + (size_t)img * wgs * stride, wgs, (size_t)stride, tid);
    __syncthreads();
    float loss_now = 0.f;
#pragma unroll
    for (int k = 0; k < LOSS_GROUPS; ++k) loss_now += redl[k];
    const bool bad_before = hdr0 != nullptr && hdr0[(size_t)img * hdr_stride + opt_hdr_frozen_before(t)] != 0.f;
    return bad_before || !isfinite(loss_now);
}

// An image the ICNN update of step t has frozen takes no step of its deformation or pose either.  ONE source of truth with that
// update: the flag it has written for step t into the header's double buffer (one launch earlier on this stream; `status` may be
// NULL) - or, when it runs in THIS launch (loss_part != null: cdn_/pcn_update_kernel), the same decision from the same numbers.
// gmul: the joint step's detached clip factor, not finite when its composite loss was not (joint_step_finish_kernel).
__device__ __forceinline__ bool deformation_frozen(const float gmul, const float* loss_part, const int loss_wgs, const long long loss_stride,
                                                   const float* hdr0, const long long hdr_stride, const int32_t* status, const int t,
                                                   const int img, const int tid) {
    return !isfinite(gmul) ||
           (loss_part != nullptr
                ? frozen_in_launch(loss_part, loss_wgs, loss_stride, hdr0, hdr_stride, t, img, tid)
                : ((hdr0 != nullptr && hdr0[(size_t)img * hdr_stride + opt_hdr_frozen_by_update(t)] != 0.f) ||
                   (status != nullptr && status[img] != INR_STATUS_OK)));
}

}  // namespace
