// Sequence pretraining on the device (include/inrfit.h: inrfit_pcn_fit_sequence, inrfit_rnvp_fit_identity_sequence): the mini-batch
// epochs of PathConnectedNet._non_prior_based_pretrain (awesome/model/path_connected_net.py:634-713) and of learn_flow_identity
// (:200-236) as ONE enqueue of plain stream launches.  A batch's step is what inrfit_pcn_fit(steps = 1) / inrfit_rnvp_fit_identity
// (steps = 1) launch for it - the same kernels with the same launch shapes on the same numbers - so a sequence fit ends bit for bit
// where the per-batch host loop ends.  Two kernels are new: the frame gather in front of every step and the epoch end behind the
// last batch of an epoch.
//
// Included by inrfit.hip behind its fit skeletons (FusedIcnn, RnvpDeform, PcnWs, the launch_* helpers).
#pragma once

namespace {

// ---- frame gather ---------------------------------------------------------------------------------------------------------------
// The frame ids travel as KERNEL ARGUMENTS: the host has validated every entry of `order` (a permutation of [0, T) per row) before
// the first launch, and the values a kernel sees are those very ints, by value - no id is ever read from device memory.
constexpr int SEQ_GATHER_FRAMES = 16;   // frames per gather launch (a larger batch takes several launches)
struct SeqGatherArgs {
    const float* frame_coords;    // [T][C][HW]
    const float* frame_targets;   // [T][HW] or null (identity pre-fit)
    float* stage_coords;          // [C][b HW]: the explicit planar grid the step kernels read
    float* stage_targets;         // [b HW]
    long long HW, bHW;            // points per frame, points of this batch (b HW)
    int C, n, slot0;              // channels, frames of this launch, staging slot of its first frame
    int ids[SEQ_GATHER_FRAMES];
};

// plane z < C: channel z of the coordinates, z == C: the targets.  VEC: HW % 4 == 0 and 16-byte aligned bases - every frame and
// every staging slot then starts on 16 bytes; otherwise (frame starts fall anywhere) element by element.
template <bool VEC>
__global__ __launch_bounds__(256) void seq_gather_kernel(const SeqGatherArgs a) {
    const int j = blockIdx.y, z = blockIdx.z;
    if (j >= a.n) return;
    const long long id = a.ids[j];
    const bool tgt = z == a.C;
    if (tgt && a.frame_targets == nullptr) return;
    const float* __restrict__ src = tgt ? a.frame_targets + id * a.HW : a.frame_coords + (id * a.C + z) * a.HW;
    float* __restrict__ dst = (tgt ? a.stage_targets : a.stage_coords + (long long)z * a.bHW) + (long long)(a.slot0 + j) * a.HW;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        if (4 * i < a.HW) *(f32x4*)(dst + 4 * i) = *(const f32x4*)(src + 4 * i);
    } else {
        if (i < a.HW) dst[i] = src[i];
    }
}

static void launch_seq_gather(const float* frame_coords, const float* frame_targets, float* stage_coords, float* stage_targets, int C,
                              long long HW, const int32_t* ids, int b, hipStream_t s) {
    const uintptr_t bases = (uintptr_t)frame_coords | (uintptr_t)frame_targets | (uintptr_t)stage_coords | (uintptr_t)stage_targets;
    const bool vec = HW % 4 == 0 && bases % 16 == 0;
    const long long per = vec ? HW / 4 : HW;
    for (int j0 = 0; j0 < b; j0 += SEQ_GATHER_FRAMES) {
        SeqGatherArgs a{};
        a.frame_coords = frame_coords;
        a.frame_targets = frame_targets;
        a.stage_coords = stage_coords;
        a.stage_targets = stage_targets;
        a.HW = HW;
        a.bHW = (long long)b * HW;
        a.C = C;
        a.n = b - j0 < SEQ_GATHER_FRAMES ? b - j0 : SEQ_GATHER_FRAMES;
        a.slot0 = j0;
        for (int j = 0; j < a.n; ++j) a.ids[j] = ids[j0 + j];
        const dim3 g((unsigned)((per + 255) / 256), (unsigned)a.n, (unsigned)(C + (frame_targets ? 1 : 0)));
        if (vec) hipLaunchKernelGGL(seq_gather_kernel<true>, g, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(seq_gather_kernel<false>, g, dim3(256), 0, s, a);
    }
}

// ---- epoch end ------------------------------------------------------------------------------------------------------------------
// The schedule state a Python loop keeps in doubles (torch's ReduceLROnPlateau: lr, best, num_bad), in the workspace.
struct SeqPlateau {
    double lr, best;
    long long num_bad;
};
// ... and its settings, as Python doubles (the caller's `schedule`, or InrOptDesc's floats widened)
struct SeqSchedule {
    double lr0, factor, threshold, min_lr, eps;
    int enabled, patience;
};

// the schedule state of a cold fit, in front of the first step.  (A sequence fit does not continue an earlier call: the header keeps
// `best` in fp32, so a continued scheduler would not be the uninterrupted one - inrfit_pcn_fit_sequence answers step0 != 0 with
// INR_EINVAL.)
__global__ void seq_begin_kernel(SeqPlateau* st, double lr0) {
    if (threadIdx.x != 0) return;
    st->lr = lr0;
    st->best = (double)INFINITY;
    st->num_bad = 0;
}

// One thread, fixed order, no atomics.  The epoch loss is summed as the host loop sums it - acc = acc + loss_b / n_batches in fp32,
// where torch divides a device scalar by a Python number as a product with the fp32 reciprocal - and the scheduler's decision is
// taken in double on (double)acc.  next_slot: header slot the NEXT optimizer step reads its learning rate from (opt_hdr_lr_of); the
// RealNVP half of the update reads the same slot.
__global__ void seq_epoch_end_kernel(const float* __restrict__ batch_loss, int n_batches, float* __restrict__ epoch_loss,
                                     float* __restrict__ hdr, int next_slot, SeqPlateau* __restrict__ st, const int32_t* __restrict__ status,
                                     const SeqSchedule sc) {
    if (threadIdx.x != 0) return;
    const float inv = 1.f / (float)n_batches;
    float acc = 0.f;
    for (int b = 0; b < n_batches; ++b) acc = __fadd_rn(acc, __fmul_rn(batch_loss[b], inv));
    *epoch_loss = acc;
    if (status[0] != INR_STATUS_OK) return;   // frozen by a non-finite loss: the schedule stands still like everything else
    if (!sc.enabled) return;
    const double el = (double)acc;
    double lr = st->lr, best = st->best;
    long long num_bad = st->num_bad;
    if (el < best * (1.0 - sc.threshold)) {
        best = el;
        num_bad = 0;
    } else {
        num_bad += 1;
    }
    if (num_bad > sc.patience) {
        const double nlr = fmax(lr * sc.factor, sc.min_lr);
        if (lr - nlr > sc.eps) lr = nlr;
        num_bad = 0;
    }
    st->lr = lr;
    st->best = best;
    st->num_bad = num_bad;
    hdr[next_slot] = (float)lr;
    hdr[OPT_HDR_LR] = (float)lr;
    hdr[OPT_HDR_BEST] = (float)best;
    hdr[OPT_HDR_NUM_BAD] = (float)num_bad;
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
struct SeqLayout {
    float *stage_coords, *stage_targets, *batch_loss;
    SeqPlateau* plateau;
    long long head_bytes;   // everything in front of the step's own workspace
};

static SeqLayout seq_layout(int C, long long HW, int batch, int n_batches, void* base) {
    SeqLayout l;
    char* b = (char*)base;
    long long off = 0;
    auto take = [&](long long bytes) { char* p = b + off; off += align256(bytes); return p; };
    l.stage_coords = (float*)take((long long)C * batch * HW * 4);
    l.stage_targets = (float*)take((long long)batch * HW * 4);
    l.batch_loss = (float*)take((long long)n_batches * 4);
    l.plateau = (SeqPlateau*)take(sizeof(SeqPlateau));
    l.head_bytes = off;
    return l;
}

static InrGridDesc seq_grid(const float* stage_coords, long long n_points) {
    InrGridDesc g{};
    g.mode = INR_GRID_EXPLICIT;
    g.n_points = n_points;
    g.coords = stage_coords;
    g.coords_image_stride = 0;
    return g;
}

// every entry in [0, T), every row a permutation
static bool seq_order_ok(const int32_t* order, int num_epochs, int T) {
    std::vector<char> seen((size_t)T);
    for (int e = 0; e < num_epochs; ++e) {
        std::fill(seen.begin(), seen.end(), 0);
        for (int i = 0; i < T; ++i) {
            const int32_t id = order[(size_t)e * T + i];
            if (id < 0 || id >= T || seen[(size_t)id]) return false;
            seen[(size_t)id] = 1;
        }
    }
    return true;
}

static bool seq_sizes_ok(int T, long long HW, int batch_size, int num_epochs, int step0) {
    if (T < 1 || HW < 1 || batch_size < 1 || num_epochs < 0 || step0 < 0) return false;
    const long long b = batch_size < T ? batch_size : T;
    return b * HW <= 0x7fffffffLL && (long long)num_epochs * ((T + b - 1) / b) + step0 <= 0x7fffffffLL;
}

// one batch shape of a sequence fit: the step's workspace carved for its point count (the launch shapes depend on it)
struct SeqPcnCtx {
    InrGridDesc grid;
    FusedIcnn b;
    RnvpDeform f;
    SeqPcnCtx(const RnvpDeform& f0) : f(f0) {}
};

}  // namespace

extern "C" {

int64_t inrfit_pcn_sequence_workspace_bytes(const InrModelDesc* model, const InrRnvpDesc* rnvp, int64_t HW, int T, int batch_size) {
    if (!rnvp_ok(rnvp)) return INR_EUNSUPPORTED;
    if (model && !find_entry(model)) return INR_EUNSUPPORTED;
    if (!seq_sizes_ok(T, HW, batch_size, 0, 0)) return INR_EINVAL;
    const int b = batch_size < T ? batch_size : T, r = T % b;
    const SeqLayout l = seq_layout(rnvp->channels, HW, b, (T + b - 1) / b, nullptr);
    InrGridDesc g = seq_grid(nullptr, (long long)b * HW);
    long long own = inrfit_pcn_workspace_bytes(model, rnvp, &g, 1);
    if (own < 0) return own;
    if (r) {
        g.n_points = (long long)r * HW;
        const long long o2 = inrfit_pcn_workspace_bytes(model, rnvp, &g, 1);
        if (o2 < 0) return o2;
        if (o2 > own) own = o2;
    }
    return l.head_bytes + align256(own);
}

int inrfit_pcn_fit_sequence(const InrModelDesc* model, const InrRnvpDesc* rnvp, float* icnn_params, float* flow_params,
                            float* icnn_opt_state, float* flow_opt_state, const float* frame_coords, const float* frame_targets,
                            const int32_t* order, int T, int64_t HW, int batch_size, int num_epochs, const InrLossDesc* loss,
                            const InrOptDesc* opt, const double* schedule, float flow_weight_decay, int step0, float* epoch_loss,
                            int32_t* status, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!icnn_params || !flow_params || !icnn_opt_state || !flow_opt_state || !frame_coords || !frame_targets || !order || !opt ||
        !epoch_loss || !status || !workspace)
        return INR_EINVAL;
    if (!seq_sizes_ok(T, HW, batch_size, num_epochs, step0) || step0 != 0) return INR_EINVAL;   // (a cold fit only: seq_begin_kernel)
    if (const int rc = check_fit(opt, loss, false)) return rc;
    if (!model || !rnvp_ok(rnvp) || !find_entry(model)) return INR_EUNSUPPORTED;   // the fused ICNN shapes only
    if (!seq_order_ok(order, num_epochs, T)) return INR_EINVAL;
    const int bs = batch_size < T ? batch_size : T, rem = T % bs, nb = (T + bs - 1) / bs, C = rnvp->channels;
    const SeqLayout l = seq_layout(C, HW, bs, nb, workspace);
    if (workspace_bytes < l.head_bytes) return INR_EWORKSPACE;
    void* ws = (char*)workspace + l.head_bytes;
    const int64_t ws_bytes = workspace_bytes - l.head_bytes;
    const RnvpDeform f0(rnvp, flow_params, flow_opt_state, nullptr, flow_weight_decay);
    SeqPcnCtx full(f0), last(f0);   // `last`: the short batch an epoch ends with when batch_size does not divide T
    full.grid = seq_grid(l.stage_coords, (long long)bs * HW);
    int rc = full.f.check(full.b, model, &full.grid, 1, ws, ws_bytes, false);
    if (rc || (rc = full.b.loss_ok(loss))) return rc;
    if (rem) {
        last.grid = seq_grid(l.stage_coords, (long long)rem * HW);
        if ((rc = last.f.check(last.b, model, &last.grid, 1, ws, ws_bytes, false))) return rc;
    }
    // every argument has been answered: the device's turn
    if ((rc = device_ready(full.b, full.f))) return rc;
    hipStream_t s = (hipStream_t)stream;
    SeqSchedule sc{(double)opt->lr, (double)opt->plateau_factor, (double)opt->plateau_threshold, (double)opt->plateau_min_lr,
                   (double)opt->plateau_eps, opt->plateau, opt->plateau_patience};
    if (schedule) {
        sc.lr0 = schedule[0];
        sc.factor = schedule[1];
        sc.threshold = schedule[2];
        sc.min_lr = schedule[3];
        sc.eps = schedule[4];
    }
    InrOptDesc o = *opt;   // the steps' own: one learning rate from the header, the scheduler is the epoch end's
    o.plateau = 0;
    o.lr = (float)sc.lr0;
    float* hdr = icnn_opt_state + 2 * (size_t)full.b.P();
    hipLaunchKernelGGL(opt_init_kernel, dim3(1), dim3(64), 0, s, icnn_opt_state, full.b.P(), o, step0);
    hipLaunchKernelGGL(seq_begin_kernel, dim3(1), dim3(64), 0, s, l.plateau, sc.lr0);
    if (hipMemsetAsync(status, 0, sizeof(int32_t), s) != hipSuccess) return INR_ELAUNCH;
    SeqPcnCtx* prev = nullptr;
    int k = step0;
    for (int e = 0; e < num_epochs; ++e) {
        const int32_t* row = order + (size_t)e * T;
        for (int j = 0; j < nb; ++j, ++k) {
            const int b = j == nb - 1 && rem ? rem : bs;
            SeqPcnCtx& c = b == bs ? full : last;
            launch_seq_gather(frame_coords, frame_targets, l.stage_coords, l.stage_targets, C, HW, row + (size_t)j * bs, b, s);
            hipLaunchKernelGGL(loss_coef_kernel, dim3(1), dim3(256), 0, s, (const float*)l.stage_targets, c.b.tstride(), *loss, c.b.coef(), 1.f);
            // the two shapes share one workspace: a step behind one of the other shape packs its parameter images again (behind one
            // of its own shape the update kernels have kept them in step, as in inrfit_pcn_fit)
            const bool packed = prev == &c;
            if (!packed && (rc = c.b.pack(icnn_params, s))) return rc;
            c.b.begin_updates(icnn_params, icnn_opt_state, l.batch_loss, status, &o, 1);
            c.b.set_step(k, &o, k + 1, j);
            TrainPass a{l.stage_targets, loss->kind};
            a.dxd = c.f.dxd;
            c.f.forward(true, packed, s);
            if ((rc = c.b.train(0, icnn_params, a, s))) return rc;
            c.f.update(c.b, true, s);
            prev = &c;
        }
        hipLaunchKernelGGL(seq_epoch_end_kernel, dim3(1), dim3(64), 0, s, (const float*)l.batch_loss, nb, epoch_loss + e, hdr, opt_hdr_lr_of(k + 1),
                           l.plateau, (const int32_t*)status, sc);
    }
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

int inrfit_rnvp_fit_identity_sequence(const InrRnvpDesc* rnvp, float* flow_params, float* flow_opt_state, const float* frame_coords,
                                      const int32_t* order, int T, int64_t HW, int batch_size, int num_epochs, const InrOptDesc* opt,
                                      int step0, float* loss_hist, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!flow_params || !flow_opt_state || !frame_coords || !order || !opt || !loss_hist || !workspace) return INR_EINVAL;
    if (!seq_sizes_ok(T, HW, batch_size, num_epochs, step0)) return INR_EINVAL;
    if (opt->kind != INR_OPT_ADAM && opt->kind != INR_OPT_ADAMAX) return INR_EINVAL;
    if (!rnvp_ok(rnvp)) return INR_EUNSUPPORTED;
    if (!seq_order_ok(order, num_epochs, T)) return INR_EINVAL;
    const int bs = batch_size < T ? batch_size : T, rem = T % bs, nb = (T + bs - 1) / bs, C = rnvp->channels;
    const SeqLayout l = seq_layout(C, HW, bs, nb, workspace);
    if (workspace_bytes < l.head_bytes) return INR_EWORKSPACE;
    void* ws = (char*)workspace + l.head_bytes;
    const int64_t ws_bytes = workspace_bytes - l.head_bytes;
    struct Ctx {
        InrGridDesc grid;
        PcnWs w;
    } full, last;
    full.grid = seq_grid(l.stage_coords, (long long)bs * HW);
    full.w = carve_pcn(rnvp, &full.grid, 1, ws);
    if (ws_bytes < full.w.bytes) return INR_EWORKSPACE;
    if (rem) {
        last.grid = seq_grid(l.stage_coords, (long long)rem * HW);
        last.w = carve_pcn(rnvp, &last.grid, 1, ws);
        if (ws_bytes < last.w.bytes) return INR_EWORKSPACE;
    }
    // every argument has been answered: the device's turn
    if (const int rc = rnvp_set_lds()) return rc;
    hipStream_t s = (hipStream_t)stream;
    Ctx* prev = nullptr;
    int k = step0;
    for (int e = 0; e < num_epochs; ++e) {
        const int32_t* row = order + (size_t)e * T;
        for (int j = 0; j < nb; ++j, ++k) {
            const int b = j == nb - 1 && rem ? rem : bs;
            Ctx& c = b == bs ? full : last;
            const PcnWs& w = c.w;
            launch_seq_gather(frame_coords, nullptr, l.stage_coords, l.stage_targets, C, HW, row + (size_t)j * bs, b, s);
            RnvpIdArgs ia{};
            ia.xd = w.xd;
            ia.dxd = w.dxd;
            ia.lossp = w.lossp;
            ia.grid = c.grid;
            ia.N = c.grid.n_points;
            const dim3 gl(w.blocksL, 1);
            launch_rnvp_fwd(w, flow_params, &c.grid, 1, w.xd, true, s, true, prev == &c);
            if (C == 2) hipLaunchKernelGGL(rnvp_identity_loss_kernel<2>, gl, dim3(256), 0, s, ia);
            else hipLaunchKernelGGL(rnvp_identity_loss_kernel<3>, gl, dim3(256), 0, s, ia);
            launch_rnvp_bwd(w, flow_params, &c.grid, 1, s);
            RnvpUpdArgs u = make_rnvp_upd_args(w, 1, 0, flow_params, flow_opt_state, nullptr, opt, opt->weight_decay, k + 1, nullptr, 0, nullptr);
            u.skip_linear = 1;
            u.RE = w.RE;
            u.unit_linear = 1;
            u.lossp = w.lossp;
            u.lossp_blocks = w.blocksL;
            u.loss_scale = 1.f / ((float)C * (float)c.grid.n_points);
            u.loss_hist = loss_hist + e;   // every batch of the epoch writes it: the last one's stays (path_connected_net.py:234)
            u.hist_idx = 0;
            u.hist_stride = 1;
            launch_rnvp_update_args(w, 1, u, s);
            prev = &c;
        }
    }
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

}  // extern "C"
