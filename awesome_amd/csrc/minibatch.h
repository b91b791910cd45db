// Pixel-minibatch fits on the device (include/inrfit.h: inrfit_fit_minibatch, inrfit_cdn_fit_minibatch, inrfit_cdn_wide_fit_minibatch): the teaser notebooks' loops
// that train a coordinate net on a fresh random subset of the pixels at every optimizer step (convex.ipynb cell 3, repeating.ipynb
// cell 4, diffeo_convex.ipynb cells 9-11, the DataLoader loop of imageRepresentationTest.ipynb cell 6) as ONE enqueue of plain stream
// launches.  Step k is the pool gathered by row k of a device index table into a staging grid, the loss coefficients on the staging
// targets, and then fit_step - what inrfit_fit / inrfit_cdn_fit(steps = 1, step0 = step0 + k) launch for that explicit grid, on the
// same numbers - so a finite run ends bit for bit where the per-step host loop ends.  One kernel is new: the gather.
// inrfit_cdn_fit_minibatch keeps to the ICNN shapes with a fused kernel (it answers the others with INR_EUNSUPPORTED, as
// inrfit_cdn_joint_step does); inrfit_cdn_wide_fit_minibatch is the same call for the flow over a layer-by-layer ICNN (cdn_wide_shape).
//
// Included by inrfit.hip behind its fit skeletons (FusedIcnn, WideIcnn, NoDeform, FlowDeform, fit_step) and sequence.h (seq_grid).
#pragma once

#include <algorithm>

namespace {

// ---- gather -----------------------------------------------------------------------------------------------------------------------
// Unlike sequence.h's frame ids the pixel numbers are read from device memory (they are drawn there, thousands per step), so every
// one is clamped into the pool before use, as star.h does: a bad entry must not become a fault.
struct MbGatherArgs {
    const float* pool_coords;    // [C][n_pool]
    const float* pool_targets;   // [planes - C][n_pool]: [n_images][O][n_pool]
    const int32_t* row;          // index[k]: [count] used
    float* stage_coords;         // [C][count]: the explicit planar grid the step kernels read
    float* stage_targets;        // [n_images][O][count]
    long long n_pool;
    int count, C, planes;        // planes = C + n_images O
    int blocks;                  // blocks per plane
};

// one thread per (point, plane): plane z < C is channel z of the coordinates, plane C + q is target plane q = image O + o
__global__ __launch_bounds__(256) void mb_gather_kernel(const MbGatherArgs a) {
    const int z = blockIdx.x / a.blocks;
    const long long i = (long long)(blockIdx.x - z * a.blocks) * 256 + threadIdx.x;
    if (z >= a.planes || i >= a.count) return;
    long long id = a.row[i];
    id = id < 0 ? 0 : (id >= a.n_pool ? a.n_pool - 1 : id);
    if (z < a.C) a.stage_coords[(long long)z * a.count + i] = a.pool_coords[(long long)z * a.n_pool + id];
    else a.stage_targets[(long long)(z - a.C) * a.count + i] = a.pool_targets[(long long)(z - a.C) * a.n_pool + id];
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
struct MbLayout {
    float *stage_coords, *stage_targets;
    long long head_bytes;   // everything in front of the step's own workspace
};

static MbLayout mb_layout(int C, int O, long long batch, int n_images, void* base) {
    MbLayout l;
    char* b = (char*)base;
    long long off = 0;
    auto take = [&](long long bytes) { char* p = b + off; off += align256(bytes); return p; };
    l.stage_coords = (float*)take((long long)C * batch * 4);
    l.stage_targets = (float*)take((long long)n_images * O * batch * 4);
    l.head_bytes = off;
    return l;
}

// sizes the gather's launch and the step numbers can hold
static bool mb_sizes_ok(const InrModelDesc* model, long long n_pool, long long batch, int n_images, int steps, int step0) {
    if (n_pool <= 0 || batch <= 0 || batch > 0x7fffffffLL || n_images <= 0 || steps < 0 || step0 < 0) return false;
    if ((long long)steps + step0 > 0x7fffffffLL) return false;
    const long long planes = model->in_features + (long long)n_images * wide_desc_O(model);
    return (batch + 255) / 256 * planes <= 0x7fffffffLL;
}

// one batch size of a minibatch fit: the step's workspace carved for its point count (the launch shapes depend on it)
template <class B, class F>
struct MbCtx {
    InrGridDesc grid;
    B b;
    F f;
    MbCtx(const F& f0, long long count, float* stage_coords) : grid(seq_grid(stage_coords, count)), f(f0) {}
};

// `shape_ok` has been answered by the caller (INR_EUNSUPPORTED goes in front of the workspace's codes)
template <class B, class F>
int mb_run(const F& f0, const InrModelDesc* model, float* params, float* opt_state, const float* pool_coords, const float* pool_targets,
           long long n_pool, const int32_t* index, const int32_t* counts, long long batch, const InrLossDesc* loss, const InrOptDesc* opt,
           int n_images, int steps, int step0, float* loss_hist, int32_t* status, void* workspace, int64_t workspace_bytes, hipStream_t s) {
    if (!workspace) return INR_EINVAL;
    const int C = f0.in_channels(model), O = wide_desc_O(model);   // the pool's channels are the deformation's, not the backbone's
    const MbLayout l = mb_layout(C, O, batch, n_images, workspace);
    if (workspace_bytes < l.head_bytes) return INR_EWORKSPACE;
    void* ws = (char*)workspace + l.head_bytes;
    const int64_t ws_bytes = workspace_bytes - l.head_bytes;
    // the batch sizes of this call, each with its own carve of the one workspace
    std::vector<int32_t> sizes;
    if (counts) sizes.assign(counts, counts + steps);
    if (sizes.empty()) sizes.push_back((int32_t)batch);
    std::sort(sizes.begin(), sizes.end());
    sizes.erase(std::unique(sizes.begin(), sizes.end()), sizes.end());
    std::vector<MbCtx<B, F>> ctx;
    ctx.reserve(sizes.size());   // (the deformation keeps a pointer to its context's grid: no element moves)
    for (const int32_t c : sizes) {
        ctx.emplace_back(f0, (long long)c, l.stage_coords);
        MbCtx<B, F>& x = ctx.back();
        int rc = x.f.check(x.b, model, &x.grid, n_images, ws, ws_bytes, false);
        if (rc || (rc = x.b.loss_ok(loss))) return rc;
    }
    // every argument has been answered: the device's turn
    int rc = device_ready(ctx[0].b, ctx[0].f);
    if (rc) return rc;
    hipLaunchKernelGGL(opt_init_kernel, dim3(n_images), dim3(64), 0, s, opt_state, ctx[0].b.P(), *opt, step0);
    if (status && hipMemsetAsync(status, 0, sizeof(int32_t) * n_images, s) != hipSuccess) return INR_ELAUNCH;
    for (auto& x : ctx) x.b.begin_updates(params, opt_state, loss_hist, status, opt, steps);
    const bool from_targets = loss->weight_mode != INR_WEIGHT_NONE && loss->weight_mode != INR_WEIGHT_EXPLICIT;
    MbGatherArgs g{};
    g.pool_coords = pool_coords;
    g.pool_targets = pool_targets;
    g.stage_coords = l.stage_coords;
    g.stage_targets = l.stage_targets;
    g.n_pool = n_pool;
    g.C = C;
    g.planes = C + n_images * O;
    MbCtx<B, F>* prev = nullptr;
    for (int k = 0; k < steps; ++k) {
        const int32_t c = counts ? counts[k] : (int32_t)batch;
        MbCtx<B, F>& x = ctx[(size_t)(std::lower_bound(sizes.begin(), sizes.end(), c) - sizes.begin())];
        g.row = index + (size_t)k * (size_t)batch;
        g.count = c;
        g.blocks = (c + 255) / 256;
        hipLaunchKernelGGL(mb_gather_kernel, dim3((unsigned)(g.blocks * g.planes)), dim3(256), 0, s, g);
        // The batch sizes share one workspace.  Behind a step of its own size a context still holds its loss coefficients and the
        // parameter images its update kernels have kept in step, as in inrfit_fit; behind one of another size it takes them again.
        const bool same = prev == &x;
        if (!same || from_targets)
            hipLaunchKernelGGL(loss_coef_kernel, dim3(n_images), dim3(256), 0, s, (const float*)l.stage_targets, x.b.tstride(), *loss,
                               x.b.coef(), 1.f);
        if (!same) {
            if ((rc = x.b.pack(params, s))) return rc;
            x.f.begin(s);
        }
        TrainPass a{l.stage_targets, loss->kind};
        a.dxd = x.f.dxd;
        a.freeze_input = opt->freeze_input;
        if ((rc = fit_step(x.b, x.f, params, a, opt, step0 + k, k, same, s))) return rc;
        prev = &x;
    }
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

// what both entry points check of their shared arguments, in this order, before anything else
static int mb_check_args(const InrModelDesc* model, const float* pool_coords, const float* pool_targets, long long n_pool,
                         const int32_t* index, const int32_t* counts, long long batch, const InrLossDesc* loss, const InrOptDesc* opt,
                         int n_images, int steps, int step0, bool adam_only) {
    if (!model || !pool_coords || !pool_targets || !index || !opt) return INR_EINVAL;
    if (!mb_sizes_ok(model, n_pool, batch, n_images, steps, step0)) return INR_EINVAL;
    if (counts)
        for (int k = 0; k < steps; ++k)
            if (counts[k] < 1 || counts[k] > batch) return INR_EINVAL;
    return check_fit(opt, loss, adam_only);
}

}  // namespace

extern "C" {

int64_t inrfit_minibatch_workspace_bytes(const InrModelDesc* model, const InrFlowDesc* flow, int64_t batch, int n_images) {
    if (flow ? !flow_ok(flow) || !find_entry(model) || model->in_features != 2 : !find_entry(model) && !use_wide(model))
        return INR_EUNSUPPORTED;
    if (!mb_sizes_ok(model, 1, batch, n_images, 0, 0)) return INR_EINVAL;
    // the step's workspace is carved anew for every count: the largest over 1..batch (the layouts round per count)
    long long own = 0;
    InrGridDesc g = seq_grid(nullptr, 1);
    for (long long c = 1; c <= batch; ++c) {
        g.n_points = c;
        const long long o = flow ? inrfit_cdn_workspace_bytes(model, flow, &g, n_images) : inrfit_workspace_bytes(model, &g, n_images);
        if (o < 0) return o;
        if (o > own) own = o;
    }
    return mb_layout(model->in_features, wide_desc_O(model), batch, n_images, nullptr).head_bytes + align256(own);
}

int64_t inrfit_cdn_wide_minibatch_workspace_bytes(const InrModelDesc* model, const InrFlowDesc* flow, int64_t batch, int n_images) {
    if (!flow_ok(flow) || !cdn_wide_shape(model)) return INR_EUNSUPPORTED;
    if (!mb_sizes_ok(model, 1, batch, n_images, 0, 0)) return INR_EINVAL;
    long long own = 0;   // (as above: the largest carve over 1..batch)
    InrGridDesc g = seq_grid(nullptr, 1);
    for (long long c = 1; c <= batch; ++c) {
        g.n_points = c;
        const long long o = inrfit_cdn_workspace_bytes(model, flow, &g, n_images);
        if (o < 0) return o;
        if (o > own) own = o;
    }
    return mb_layout(model->in_features, wide_desc_O(model), batch, n_images, nullptr).head_bytes + align256(own);
}

int inrfit_fit_minibatch(const InrModelDesc* model, float* params, float* opt_state, const float* pool_coords,
                         const float* pool_targets, int64_t n_pool, const int32_t* index, const int32_t* counts, int64_t batch,
                         const InrLossDesc* loss, const InrOptDesc* opt, int n_images, int steps, int step0, float* loss_hist,
                         int32_t* status, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!params || !opt_state) return INR_EINVAL;
    if (const int rc = mb_check_args(model, pool_coords, pool_targets, n_pool, index, counts, batch, loss, opt, n_images, steps, step0, false))
        return rc;
    if (use_wide(model))
        return mb_run<WideIcnn>(NoDeform(), model, params, opt_state, pool_coords, pool_targets, n_pool, index, counts, batch, loss, opt,
                                n_images, steps, step0, loss_hist, status, workspace, workspace_bytes, (hipStream_t)stream);
    if (!find_entry(model)) return INR_EUNSUPPORTED;
    return mb_run<FusedIcnn>(NoDeform(), model, params, opt_state, pool_coords, pool_targets, n_pool, index, counts, batch, loss, opt,
                             n_images, steps, step0, loss_hist, status, workspace, workspace_bytes, (hipStream_t)stream);
}

int inrfit_cdn_fit_minibatch(const InrModelDesc* model, const InrFlowDesc* flow, float* icnn_params, float* flow_params,
                             float* icnn_opt_state, float* flow_opt_state, const float* pool_coords, const float* pool_targets,
                             int64_t n_pool, const int32_t* index, const int32_t* counts, int64_t batch, const InrLossDesc* loss,
                             const InrOptDesc* opt, float weight_decay_on_weight_g, int n_images, int steps, int step0,
                             float* loss_hist, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!icnn_params || !flow_params || !icnn_opt_state || !flow_opt_state) return INR_EINVAL;
    if (const int rc = mb_check_args(model, pool_coords, pool_targets, n_pool, index, counts, batch, loss, opt, n_images, steps, step0,
                                     true))   // the flow's optimizer step is Adam's only
        return rc;
    if (!flow_ok(flow) || !find_entry(model) || model->in_features != 2) return INR_EUNSUPPORTED;
    return mb_run<FusedIcnn>(FlowDeform(flow, flow_params, flow_opt_state, nullptr, weight_decay_on_weight_g), model, icnn_params,
                             icnn_opt_state, pool_coords, pool_targets, n_pool, index, counts, batch, loss, opt, n_images, steps, step0,
                             loss_hist, status, workspace, workspace_bytes, (hipStream_t)stream);
}

int inrfit_cdn_wide_fit_minibatch(const InrModelDesc* model, const InrFlowDesc* flow, float* icnn_params, float* flow_params,
                                  float* icnn_opt_state, float* flow_opt_state, const float* pool_coords, const float* pool_targets,
                                  int64_t n_pool, const int32_t* index, const int32_t* counts, int64_t batch, const InrLossDesc* loss,
                                  const InrOptDesc* opt, float weight_decay_on_weight_g, int n_images, int steps, int step0,
                                  float* loss_hist, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!icnn_params || !flow_params || !icnn_opt_state || !flow_opt_state) return INR_EINVAL;
    if (const int rc = mb_check_args(model, pool_coords, pool_targets, n_pool, index, counts, batch, loss, opt, n_images, steps, step0,
                                     true))   // the flow's optimizer step is Adam's only
        return rc;
    if (!flow_ok(flow) || !cdn_wide_shape(model)) return INR_EUNSUPPORTED;
    return mb_run<WideIcnn>(FlowDeform(flow, flow_params, flow_opt_state, nullptr, weight_decay_on_weight_g), model, icnn_params,
                            icnn_opt_state, pool_coords, pool_targets, n_pool, index, counts, batch, loss, opt, n_images, steps, step0,
                            loss_hist, status, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
