// libinrfit - MI355X (gfx950 / CDNA4) kernels for the per-image INR fit hot path.  C ABI: include/inrfit.h.
//
// What runs here (reference: jp-schneider/awesome, paths relative to its checkout):
//   icnn_step_kernel   fused  coords -> z0 = relu(W_in x + b_in) -> a1 = W1 z0 + b1 + S1 x (MFMA) -> z1 = relu(a1)
//                      -> y = w_o.z1 + b_o + s_o.x -> sigmoid -> SE/BCE data term -> backward (MFMA) -> per-workgroup
//                      gradient slab.  Replaces ConvexNextNet.forward + criterion + loss.backward()
//                      (awesome/model/convex_net.py:205-214, awesome/measures/weighted_loss.py:67-92,
//                      awesome/model/path_connected_net.py:941-948).
//                      The same kernel is the prior's share of the convexity losses' joint step (inrfit_joint_prior_step):
//                      a data-term mask (data_count, noneclass) and a hard / soft align term, all run-time StepArgs fields.
//   icnn_update_kernel fixed-order slab reduction + Adam/Adamax + enforce_convexity clamp + ReduceLROnPlateau
//                      (torch.optim.Adam/Adamax; convex_net.py:151-154,216-220; path_connected_net.py:949-951).
//
// Design (DESIGN.md has the full derivation):
//   * one workgroup = 4 waves (one per SIMD, up to 512 VGPRs each); a wave owns 16 points of a 64-point chunk;
//   * points live on the MFMA *column* (lane & 15), hidden units on the accumulator rows, so the D tile of one
//     v_mfma_f32_16x16x4_f32 is already the B operand of the next layer / of the backward product: activations never
//     leave registers between layers; weights are the A operand, read from one LDS image used by forward
//     (ds_read_b128 along a row) and backward (ds_read_b32 down a column);
//   * bias and the skip term ride in the GEMM as extra "ext" input rows (1, x, y[, t]) placed in the padding slots of
//     the last k-group, so b1/S1 gradients fall out of the dW product for free;
//   * dW1 = dZ1^T Z0ext contracts over points: the two operands are staged once through LDS (point-major rows,
//     float4 writes, conflict-free strides), the 9x9 output tiles are split over the 4 waves;
//   * fp32 everywhere (exact-f32 MFMA == fmaf chain), fixed-order reductions, no atomics: results are reproducible.
#include "icnn_step.h"
#include "icnn_step2.h"
#include "optim.h"
#include "flow.h"
#include "rnvp.h"
#include "joint_loss.h"
#include "wide.h"
#include "star.h"
#include "cnnseg.h"
#include "fcseg.h"
#include "unet.h"
#include "unet_train.h"

#include <type_traits>
#include <vector>

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// slab reduction + optimizer step
// ---------------------------------------------------------------------------------------------------------------------
constexpr int UPD_RANGES = WIDE_MAX_LAYERS + 1;   // hidden layers of the widest supported net + the output layer
struct UpdArgs {
    float* wimg;          // [n_images][img.floats] parameter images (kept in step with params)
    ImgMap img;
    float* params;        // [n_images][P]
    float* opt_state;     // [n_images][2P + HDR]
    const float* slabs;   // [n_images][wgs][PS]
    const float* loss_part;    // the workgroups' loss partials, [n_images][wgs] at stride loss_stride: the step kernels' dense copy
    long long loss_stride;     // (stride 1, Workspace::loss_part), or the loss column of a one-slab view in place (stride PS)
    float* loss_hist;     // [n_images][steps] or null
    float* grads_out;     // mode 1: [n_images][P]
    float* loss_out;      // mode 1: [n_images]
    int32_t* status;      // [n_images] or null
    InrOptDesc opt;
    int P, PS, wgs, n_images;   // P: parameters of the KERNEL's shape (slab column P = the loss); PS: slab stride in floats; the slab's
                                // column layout is img.sl_* (icnn_step.h, Cfg: gradient slab)
    int Pu, hu;                 // the CALLER's model: parameter count and n_hidden (hu == img.H: same shape; hu < img.H: the model runs
                                // zero-padded on the next compiled width, user_param_index below)
    int t;                // 1-based optimizer step index
    OptConsts c;          // ... and its constants
    int hist_idx, hist_stride;
    int mode;             // 0 = optimizer step, 1 = write reduced grads + loss only
    int clamp_lo[UPD_RANGES], clamp_hi[UPD_RANGES];    // flat ranges projected onto >= 0 (ln.weight of every hidden layer, out.ln.weight)
    int freeze_lo[UPD_RANGES], freeze_hi[UPD_RANGES];  // flat ranges that are never updated (the skip weights when opt.freeze_skips)
    int input_hi;                    // opt.freeze_input: flat range [0, input_hi) = input.weight | input.bias is never updated
    const float* gscale;             // [n_images] factor on the reduced gradient (device; the joint step's detached clip factor), or null
};

// A model whose n_hidden has no compiled kernel runs ZERO-PADDED on the next compiled width H (SURVEY 7 hard part 3): the padded
// hidden units have W_in = b_in = 0 rows, zero rows AND columns in every hidden layer and w_o = 0, so their activations, their relu
// masks (pre-activation 0 is "off") and every gradient that touches them are exactly 0 - the fit of the h real units is the same
// arithmetic with zeros added to the sums.  Nothing padded is ever stored: parameters, optimizer state and gradients keep the CALLER's
// flat layout (include/inrfit.h, with h), and the two kernels that touch it translate indices.
// Kernel-shape flat index j (layout with H = m.H) -> caller's flat index (layout with h), or -1 for a padded entry.
__host__ __device__ __forceinline__ int user_param_index(const ImgMap& m, int h, int j) {
    const int H = m.H, C = m.C;
    if (h == H) return j;
    if (j < m.p_bin) {                       // input.weight [H][C]
        const int i = j / C;
        return i < h ? j : -1;
    }
    if (j < m.p_w[0]) {                      // input.bias [H]
        const int i = j - m.p_bin;
        return i < h ? h * C + i : -1;
    }
    int base_u = h * C + h;                  // caller's offset of skip.0.ln.weight
    const int per_u = h * h + h + h * C;
    for (int k = 0; k < m.L; ++k, base_u += per_u) {
        if (j < m.p_b[k]) {                  // skip.k.ln.weight [H][H]
            const int q = j - m.p_w[k], o = q / H, i = q - o * H;
            return (o < h && i < h) ? base_u + o * h + i : -1;
        }
        if (j < m.p_s[k]) {                  // skip.k.ln.bias [H]
            const int o = j - m.p_b[k];
            return o < h ? base_u + h * h + o : -1;
        }
        if (j < m.p_s[k] + H * C) {          // skip.k.skp.weight [H][C]
            const int q = j - m.p_s[k], o = q / C;
            return o < h ? base_u + h * h + h + q : -1;
        }
    }
    if (j < m.p_bo) {                        // out.ln.weight [H]
        const int i = j - m.p_wo;
        return i < h ? base_u + i : -1;
    }
    return base_u + h + (j - m.p_bo);        // out.ln.bias, out.skp.weight [C]
}

constexpr int UPD_MAX_PARAMS = 256;  // most parameters per block
constexpr int UPD_GROUPS = 16;       // slab groups summed in parallel, then combined in fixed order

constexpr int UPD_LINE = 32;         // slab columns per 128-byte line (slab rows start on lines: carve)

// Which slab columns a block owns.  A CU pulls ~10 B/clock from memory whatever runs on it, so the reduction is as fast as its busiest
// CU, and what a CU pulls is whole lines: every block owns whole lines (its first column is a multiple of 32), so no line is taken in
// by two blocks - neighbours sit on different XCDs, which fetched a shared line twice - and a block takes in what it sums and nothing
// else.  One block per CU: the first n_wide blocks own ppb columns, the others one line less (the headline's 19 222 columns = 601
// lines -> 89 blocks of 96 + 167 of 64; DESIGN.md 4.3 lists the uniform splits, which INRFIT_UPD_LINES runs).  More than 8 lines per CU, or
// fewer lines than CUs: equal blocks of 8 lines / of one line.  x n_images blocks when there are many images.
// `reserve` = CUs left to other blocks of the same launch (the deformation's update in cdn_/pcn_update_kernel).
struct UpdSplit {
    int ppb;       // columns of a wide block (multiple of 32, <= UPD_MAX_PARAMS); blockDim.x = ppb / 4
    int n_wide;    // blocks [0, n_wide) own ppb columns, blocks [n_wide, blocks) ppb - 32
    int blocks;
};
inline UpdSplit upd_split(int cols, int reserve = 0) {   // cols = slab columns in use (P + 1 in the parameter-ordered layout)
    static const int forced = getenv("INRFIT_UPD_LINES") ? atoi(getenv("INRFIT_UPD_LINES")) : 0;   // measurement switch: equal blocks of n lines
    const int cus = 256 - reserve, lines = (cols + UPD_LINE - 1) / UPD_LINE, max_lpb = UPD_MAX_PARAMS / UPD_LINE;
    int lpb = forced > 0 ? forced : (lines + cus - 1) / cus;
    if (lpb < 1) lpb = 1;
    if (lpb > max_lpb) lpb = max_lpb;
    UpdSplit sp;
    sp.ppb = lpb * UPD_LINE;
    if (forced > 0 || lpb == 1 || lines >= lpb * cus) {
        sp.blocks = (lines + lpb - 1) / lpb;
        sp.n_wide = sp.blocks;
    } else {
        sp.blocks = cus;
        sp.n_wide = lines - (lpb - 1) * cus;
    }
    return sp;
}
inline dim3 upd_grid(int cols, int n_images, int reserve = 0) { return dim3(upd_split(cols, reserve).blocks, n_images); }
inline dim3 upd_block(int cols, int reserve = 0) { return dim3(upd_split(cols, reserve).ppb / 4, UPD_GROUPS); }

#if INR_STAMPS
__device__ unsigned long long g_updtimes[512][4];   // per block of the LAST update launch, s_memrealtime (100 MHz): entry, slab loads back, reduced, stores done
__device__ unsigned long long g_updissue[512];       // per block: entry -> the first slab load is about to issue (no wait in front)
#define UPD_STAMP_ISSUE()                                                                                     \
    if (threadIdx.x == 0 && threadIdx.y == 0 && img == 0 && bx < 512) g_updissue[bx] = __builtin_amdgcn_s_memrealtime()
#define UPD_STAMP(k)                                                                                          \
    if (threadIdx.x == 0 && threadIdx.y == 0 && img == 0 && bx < 512) {                                       \
        __builtin_amdgcn_s_waitcnt(0);                                                                        \
        g_updtimes[bx][k] = __builtin_amdgcn_s_memrealtime();                                                 \
    }
#else
#define UPD_STAMP(k)
#define UPD_STAMP_ISSUE()
#endif
// block = (blockDim.x lanes x float4 = the columns of a wide block) x 16 slab groups; bx = the block's index along the slab columns,
// n_wide = UpdSplit::n_wide (in a narrow block the last 8 lanes of every group have nothing to load)
static_assert(UPD_GROUPS == LOSS_GROUPS, "the loss column is summed in the update's group order");
__device__ __forceinline__ void icnn_update_body(const UpdArgs& u, const int bx, const int img, const int n_wide) {
    const int tx = threadIdx.x, grp = threadIdx.y;
    const int ppbw = 4 * blockDim.x;
    const int ppb = bx < n_wide ? ppbw : ppbw - UPD_LINE;                               // this block's columns ...
    const int col0 = bx < n_wide ? bx * ppbw : bx * (ppbw - UPD_LINE) + n_wide * UPD_LINE;   // ... and the first of them
    __shared__ float red[UPD_GROUPS][UPD_MAX_PARAMS];
    __shared__ float redl[UPD_GROUPS];     // this step's loss partials (every block sums them, from u.loss_part: see `frozen` below)
    UPD_STAMP(0);
    const int jl = grp * blockDim.x + tx;  // the first ppb threads finish one slab column = one parameter each
    // The kernel is one dependent chain (slabs -> LDS -> optimizer -> stores) and at one image it is latency, not bandwidth, that it
    // pays for.  The slab loads are therefore the block's FIRST memory instructions: their addresses are col0 + 4 tx plus row strides,
    // nothing else.  A quad of padding columns is read like any other (slab rows are padded to whole lines: in bounds) and never
    // consumed: only the threads with j >= 0 read their column of red[][] below.  Everything else the tail needs is requested behind
    // them, and whatever depends only on values known at entry is computed while they are in flight.
    const int j4 = col0 + 4 * tx;
    const bool takes = 4 * tx < ppb && j4 < u.PS;
    const float* __restrict__ sl = u.slabs + (size_t)img * u.wgs * u.PS + j4;
    const bool trip = takes && grp + 15 * UPD_GROUPS < u.wgs;   // 256 slabs: one trip, 16 loads in flight
    f32x4 q[16];
    auto request_slabs = [&]() {
        UPD_STAMP_ISSUE();
        if (trip) {
#pragma unroll
            for (int k = 0; k < 16; ++k) q[k] = *(const f32x4*)(sl + (size_t)(grp + k * UPD_GROUPS) * u.PS);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    request_slabs();
    // then the header
    float* __restrict__ st = u.opt_state + (size_t)img * (2 * (size_t)u.Pu + INR_OPT_HEADER_FLOATS);
    float* __restrict__ hdr = st + 2 * (size_t)u.Pu;
    float p_old = 0.f, m_old = 0.f, v_old = 0.f, lr_now = 0.f;
    bool bad_before = false;
    if (u.mode == 0 && jl < ppb) {   // (in every thread that may own a parameter: the index is not known yet)
        bad_before = hdr[opt_hdr_frozen_before(u.t)] != 0.f;   // written by the PREVIOUS step's launch (double buffer like the lr: no race)
        lr_now = hdr[opt_hdr_lr_of(u.t)];
    }
    __builtin_amdgcn_sched_barrier(0);
    const int j = jl < ppb ? slab_param_of_col(u.img, col0 + jl) : -1;   // flat parameter index (kernel shape), P = loss, -1 = none
    const int ju = (j >= 0 && j < u.P) ? user_param_index(u.img, u.hu, j) : -1;       // ... in the caller's layout; -1: padding (gradient exactly 0)
    if (u.mode == 0 && ju >= 0) {
        p_old = u.params[(size_t)img * u.Pu + ju];
        m_old = st[ju];
        v_old = st[u.Pu + ju];
    }
    // what the optimizer's tail needs of the index alone: the image slots, the range tests
    int slot[2] = {0, 0}, n_slots = 0;
    bool never_updated = false, clamped = false;
    if (u.mode == 0 && ju >= 0) {
        if (u.wimg != nullptr) n_slots = image_slots(u.img, j, slot);   // (the layer-by-layer path has no parameter image)
        if (u.opt.freeze_skips) {
#pragma unroll
            for (int k = 0; k < UPD_RANGES; ++k) never_updated = never_updated || (j >= u.freeze_lo[k] && j < u.freeze_hi[k]);
        }
        if (u.opt.freeze_input && j < u.input_hi) never_updated = true;
        if (u.opt.clamp) {
#pragma unroll
            for (int k = 0; k < UPD_RANGES; ++k) clamped = clamped || (j >= u.clamp_lo[k] && j < u.clamp_hi[k]);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    {
        f32x4 part = f32x4{0.f, 0.f, 0.f, 0.f};
        if (takes) {
            int w = grp;
            if (trip) {
#pragma unroll
                for (int k = 0; k < 16; ++k) part += q[k];
                w += 16 * UPD_GROUPS;
            }
            for (; w + 15 * UPD_GROUPS < u.wgs; w += 16 * UPD_GROUPS) {
                f32x4 r[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) r[k] = *(const f32x4*)(sl + (size_t)(w + k * UPD_GROUPS) * u.PS);
#pragma unroll
                for (int k = 0; k < 16; ++k) part += r[k];
            }
            for (; w < u.wgs; w += UPD_GROUPS) part += *(const f32x4*)(sl + (size_t)w * u.PS);
        }
        *(f32x4*)&red[grp][4 * tx] = part;
        if (u.mode == 0 && tx == 0) {   // the loss partials, summed in the same order as any parameter column
            redl[grp] = loss_column_group_sum(u.loss_part + (size_t)img * u.wgs * u.loss_stride, u.wgs, (size_t)u.loss_stride, grp);
        }
    }
    float step_size = 0.f;
    if (ju >= 0) step_size = opt_step_size(lr_now, u.c.bc1);
    UPD_STAMP(1);
    __syncthreads();
    if (j < 0) return;
    float gsum = 0.f;
#pragma unroll
    for (int k = 0; k < UPD_GROUPS; ++k) gsum += red[k][jl];  // fixed order: reproducible
    if (u.gscale != nullptr && j < u.P) gsum *= u.gscale[img];   // joint step: the prior's gradient is linear in the penalty coefficient

    UPD_STAMP(2);
    if (u.mode == 1) {
        if (ju >= 0) u.grads_out[(size_t)img * u.Pu + ju] = gsum;
        else if (j == u.P) u.loss_out[img] = gsum;
        return;
    }
    // A non-finite loss freezes the image: no parameter, optimizer state or schedule changes at this step or any later one of
    // this call (the reference raises ValueError("Loss is nan or inf!") before the backward pass, path_connected_net.py:232,374;
    // torch_agent.py:484-487).  Every block derives the decision from the slabs of THIS launch, so which parameters are updated
    // does not depend on block timing.
    float loss_now = 0.f;
#pragma unroll
    for (int k = 0; k < UPD_GROUPS; ++k) loss_now += redl[k];
    const bool frozen = bad_before || !isfinite(loss_now) || (u.gscale != nullptr && !isfinite(u.gscale[img]));
    if (j == u.P) {
        opt_header_step(hdr, u.opt, u.t, gsum, frozen, lr_now, u.loss_hist ? u.loss_hist + (size_t)img * u.hist_stride + u.hist_idx : nullptr,
                        u.status ? u.status + img : nullptr);
        return;
    }
    if (frozen || !isfinite(gsum) || ju < 0 || never_updated) return;

    float m = m_old, v = v_old;
    float p = opt_step(u.opt.kind, u.c, step_size, u.opt.weight_decay, gsum, p_old, m, v);
    if (clamped) p = fmaxf(p, 0.f);
    u.params[(size_t)img * u.Pu + ju] = p;
    if (n_slots > 0) {
        float* __restrict__ wi = u.wimg + (size_t)img * u.img.floats;
        wi[slot[0]] = p;
        if (n_slots > 1) wi[slot[1]] = p;
    }
    st[ju] = m;
    st[u.Pu + ju] = v;
    UPD_STAMP(3);
}

__global__ __launch_bounds__(UPD_MAX_PARAMS / 4 * UPD_GROUPS) void icnn_update_kernel(const UpdArgs u, const int n_wide) { icnn_update_body(u, blockIdx.x, blockIdx.y, n_wide); }

// Both optimizer updates of a composite step (ICNN + its deformation) in ONE launch.  They are independent - the ICNN update reads the
// step kernel's slabs, the deformation's update the unit / point slabs of its backward kernels - and each alone is a latency chain that
// leaves most of the chip idle (the flow / RealNVP update has 2K + 1 / F + 1 blocks): blocks [0, nbi) of a grid row are the ICNN
// update's, the rest the deformation's (its 256 threads = the first four waves of the block; the other waves leave at once, which
// s_barrier allows).  A CU holds one of these blocks (12 waves at up to 168 registers), so the ICNN update leaves the deformation's
// blocks their own CUs (`reserve` of upd_split): measured with 248 + 13 blocks the two parts ran one after the other.  Same arithmetic in the same order as the two separate kernels; the deformation's blocks take the "frozen by a
// non-finite loss" decision from the slabs themselves (frozen_in_launch) instead of the flag the ICNN update writes.
constexpr int UPD_UNION_MAX_THREADS = 768;   // 12 waves: three per SIMD, 168 registers each
__global__ __launch_bounds__(UPD_UNION_MAX_THREADS) void cdn_update_kernel(const UpdArgs ui, const FlowUpdArgs uf, const int nbi, const int n_wide) {
    if ((int)blockIdx.x < nbi) {
        icnn_update_body(ui, blockIdx.x, blockIdx.y, n_wide);
        return;
    }
    const int tid = threadIdx.y * blockDim.x + threadIdx.x;
    if (tid >= 256) return;
    flow_update_body<32>(uf, (int)blockIdx.x - nbi, blockIdx.y, tid);
}
template <int C>
__global__ __launch_bounds__(UPD_UNION_MAX_THREADS) void pcn_update_kernel(const UpdArgs ui, const RnvpUpdArgs ur, const int nbi, const int n_wide) {
    if ((int)blockIdx.x < nbi) {
        icnn_update_body(ui, blockIdx.x, blockIdx.y, n_wide);
        return;
    }
    const int tid = threadIdx.y * blockDim.x + threadIdx.x;
    if (tid >= 256) return;
    rnvp_update_body<C>(ur, (int)blockIdx.x - nbi, blockIdx.y, tid);
}
inline bool upd_union_ok(int cols, int reserve) {   // the ICNN update's block must hold the deformation update's 256 threads
    const dim3 b = upd_block(cols, reserve);
    const int n = (int)(b.x * b.y);
    static const bool off = getenv("INRFIT_SPLIT_UPDATES") != nullptr;   // measurement switch: the two launches of round 2
    return !off && n >= 256 && n <= UPD_UNION_MAX_THREADS;
}

// params -> parameter image: constant background (zeros, ext-input constants), then every parameter into its slot(s)
__global__ __launch_bounds__(256) void pack_image_kernel(float* __restrict__ wimg, const ImgMap m) {
    float* __restrict__ dst = wimg + (size_t)blockIdx.y * m.floats;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m.floats) return;
    float v = 0.f;
    const int e0 = m.ext[0] - m.HM;                                // k-group TM slot of the ext input "1"
    if (i == m.off_bin + e0) v = 1.f;
    if (i == m.off_floor + e0) v = -INFINITY;                      // no relu on ext inputs
    for (int c = 0; c < m.C; ++c) {
        const int ec = m.ext[1 + c] - m.HM;                        // ext input x_c
        if (i == m.off_win + c * 16 + ec) v = 1.f;
        if (i == m.off_floor + ec) v = -INFINITY;
    }
    dst[i] = v;
}

__global__ __launch_bounds__(256) void pack_params_kernel(const float* __restrict__ params, float* __restrict__ wimg,
                                                          const ImgMap m, int hu, int Pu) {
    const int img = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m.P) return;
    const int ju = user_param_index(m, hu, j);
    if (ju < 0) return;   // padded entry: stays 0 (pack_image_kernel's background)
    const float v = params[(size_t)img * Pu + ju];
    int slot[2];
    const int ns = image_slots(m, j, slot);
    float* __restrict__ wi = wimg + (size_t)img * m.floats;
    wi[slot[0]] = v;
    if (ns > 1) wi[slot[1]] = v;
}

// per-image loss coefficients (c_fg, c_bg): 'mean' normalisation x UnariesWeightedLoss class weight x `scale` (1, or the fused joint
// step's gamma alpha in the align mode).  `use_noneclass`: targets equal to `noneclass` leave before the criterion (weighted_loss.py
// :71-74), so N counts, and the class weight is taken over, only the others (inrfit_joint_prior_step; everyone else passes 0).
__global__ __launch_bounds__(256) void loss_coef_kernel(const float* __restrict__ targets, long long N, InrLossDesc loss,
                                                        float* __restrict__ coef, float scale, int use_noneclass = 0,
                                                        float noneclass = 0.f) {
    const int img = blockIdx.x;
    __shared__ unsigned long long cnt[4], cnt_nc[4];
    unsigned long long fg = 0, nc = 0;
    const bool weighted = loss.weight_mode != INR_WEIGHT_NONE && loss.weight_mode != INR_WEIGHT_EXPLICIT;
    if (weighted || use_noneclass) {
        const float* t = targets + (size_t)img * N;
        for (long long i = threadIdx.x; i < N; i += blockDim.x) {
            const bool drop = use_noneclass && t[i] == noneclass;
            fg += !drop && t[i] < 0.5f ? 1ull : 0ull;
            nc += drop ? 1ull : 0ull;
        }
        for (int o = 32; o > 0; o >>= 1) {
            fg += __shfl_xor(fg, o);
            nc += __shfl_xor(nc, o);
        }
        if ((threadIdx.x & 63) == 0) {
            cnt[threadIdx.x >> 6] = fg;
            cnt_nc[threadIdx.x >> 6] = nc;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        float cfg, cbg;
        if (use_noneclass) N -= (long long)(cnt_nc[0] + cnt_nc[1] + cnt_nc[2] + cnt_nc[3]);   // the valid points
        const float inv_n = 1.f / (float)N;
        if (loss.weight_mode == INR_WEIGHT_EXPLICIT) {
            cfg = loss.c_fg;
            cbg = loss.c_bg;
        } else if (loss.weight_mode == INR_WEIGHT_NONE) {
            cfg = cbg = inv_n;
        } else {
            const unsigned long long nfg = cnt[0] + cnt[1] + cnt[2] + cnt[3];
            const float cc = (float)(N - (long long)nfg) / (float)nfg;  // bg_count / fg_count
            float w;
            if (loss.weight_mode == INR_WEIGHT_EQUAL) w = cc;
            else if (loss.weight_mode == INR_WEIGHT_RATIO) w = (cc - 1.f) * loss.ratio + 1.f;
            else w = rintf(cc / 10.f) + 1.f;  // sssdms (torch.round = half-to-even)
            cfg = w * inv_n;
            cbg = inv_n;
        }
        coef[2 * img] = cfg * scale;
        coef[2 * img + 1] = cbg * scale;
    }
}

__global__ __launch_bounds__(256) void opt_init_kernel(float* opt_state, int P, InrOptDesc opt, int step0) {
    float* hdr = opt_state + (size_t)blockIdx.x * (2 * (size_t)P + INR_OPT_HEADER_FLOATS) + 2 * (size_t)P;
    if (threadIdx.x == 0) {
        float lr;
        if (step0 == 0) {
            lr = opt.lr;
            hdr[OPT_HDR_BEST] = INFINITY;
            hdr[OPT_HDR_NUM_BAD] = 0.f;
        } else {
            lr = hdr[OPT_HDR_LR];
        }
        hdr[OPT_HDR_LR] = lr;
        hdr[opt_hdr_lr_of(step0 + 1)] = lr;   // the first step of this call is t = step0 + 1
        opt_hdr_clear_frozen(hdr);
    }
}

// (value > threshold) (or its complement) as one bit per point, 64 points per word, LSB = lowest index: the PNG-ready mask
__global__ __launch_bounds__(256) void pack_masks_kernel(const float* __restrict__ values, long long N, float thr, int invert,
                                                         unsigned long long* __restrict__ bits) {
    const int img = blockIdx.y;
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    bool b = false;
    if (p < N) {
        b = values[(size_t)img * N + p] > thr;
        if (invert) b = !b;
    }
    const unsigned long long m = __ballot(b);
    const long long words = (N + 63) / 64;
    if ((threadIdx.x & 63) == 0 && p < N) bits[(size_t)img * words + (p >> 6)] = m;
}

__global__ __launch_bounds__(256) void miou_kernel(const float* __restrict__ out, const float* __restrict__ tgt, long long N,
                                                   float thr_out, float thr_tgt, int invert, float* __restrict__ iou) {
    const int img = blockIdx.x;
    const float* o = out + (size_t)img * N;
    const float* t = tgt + (size_t)img * N;
    unsigned long long inter = 0, uni = 0, tpos = 0;
    for (long long i = threadIdx.x; i < N; i += blockDim.x) {
        bool ob = o[i] > thr_out, tb = t[i] > thr_tgt;
        if (invert) {
            ob = !ob;
            tb = !tb;
        }
        inter += (ob && tb) ? 1ull : 0ull;
        uni += (ob || tb) ? 1ull : 0ull;
        tpos += tb ? 1ull : 0ull;
    }
    for (int s = 32; s > 0; s >>= 1) {
        inter += __shfl_xor(inter, s);
        uni += __shfl_xor(uni, s);
        tpos += __shfl_xor(tpos, s);
    }
    __shared__ unsigned long long sm[3][4];
    if ((threadIdx.x & 63) == 0) {
        sm[0][threadIdx.x >> 6] = inter;
        sm[1][threadIdx.x >> 6] = uni;
        sm[2][threadIdx.x >> 6] = tpos;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long I = sm[0][0] + sm[0][1] + sm[0][2] + sm[0][3];
        const unsigned long long U = sm[1][0] + sm[1][1] + sm[1][2] + sm[1][3];
        const unsigned long long T = sm[2][0] + sm[2][1] + sm[2][2] + sm[2][3];
        iou[img] = (T == 0 || U == 0) ? 0.f : (float)((double)I / (double)U);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
struct KernelEntry {
    int h, c, l;
    void (*train)(const StepArgs);
    void (*train_dx)(const StepArgs);  // also writes dL/dcoords
    void (*train_act[3])(const StepArgs);   // by layer-0 activation (INR_ACT_*): [0] == train
    void (*fwd_act[3])(const StepArgs);
    void (*fwd)(const StepArgs);
    int lds_bytes;
    int P;
    ImgMap img;
};

template <int H, int C>
KernelEntry make_entry() {
    using G = Cfg<H, C>;
    ImgMap m{};
    m.H = H; m.C = C; m.L = 1; m.HM = G::HM; m.S = G::S; m.PT = G::PT; m.floats = G::IMG_FLOATS;
    m.off_sc = G::OFF_SC; m.off_wine = G::OFF_WINE; m.off_win = G::OFF_WIN; m.off_bin = G::OFF_BIN;
    m.off_floor = G::OFF_FLOOR; m.off_wo = G::OFF_WO; m.off_wct[0] = G::OFF_WCT; m.off_w[0] = G::OFF_W;
    for (int e = 0; e < 4; ++e) m.ext[e] = e < G::NEXT ? G::ext_pos(e) : 0;
    m.p_bin = G::P_BIN; m.p_w[0] = G::P_W1; m.p_b[0] = G::P_B1; m.p_s[0] = G::P_S1; m.p_wo = G::P_WO; m.p_bo = G::P_BO;
    m.p_so = G::P_SO; m.P = G::P;
    m.sl_tile = G::SL_TILE; m.sl_cols = G::SL_COLS; m.KG = G::KG; m.kg_magic = 65536 / G::KG + 1;
    return KernelEntry{H, C, 1, icnn_step_kernel<H, C, true>, icnn_step_kernel<H, C, true, true>,
                       {icnn_step_kernel<H, C, true>, icnn_step_kernel<H, C, true, false, INR_ACT_COS>,
                        icnn_step_kernel<H, C, true, false, INR_ACT_SIN>},
                       {icnn_step_kernel<H, C, false>, icnn_step_kernel<H, C, false, false, INR_ACT_COS>,
                        icnn_step_kernel<H, C, false, false, INR_ACT_SIN>},
                       icnn_step_kernel<H, C, false>, G::LDS_BYTES, G::P, m};
}

template <int H, int C>
KernelEntry make_entry2() {
    using G = Cfg2<H, C>;
    ImgMap m{};
    m.H = H; m.C = C; m.L = 2; m.HM = G::HM; m.S = G::S; m.PT = G::PT; m.floats = G::IMG_FLOATS;
    m.off_sc = G::OFF_SC; m.off_wine = G::OFF_WINE; m.off_win = G::OFF_WIN; m.off_bin = G::OFF_BIN;
    m.off_floor = G::OFF_FLOOR; m.off_wo = G::OFF_WO; m.off_wct[0] = G::OFF_WCT0; m.off_wct[1] = G::OFF_WCT1;
    m.off_w[0] = G::OFF_W0; m.off_w[1] = G::OFF_W1;
    for (int e = 0; e < 4; ++e) m.ext[e] = e < G::NEXT ? G::ext_pos(e) : 0;
    m.p_bin = G::P_BIN; m.p_w[0] = G::P_W1; m.p_b[0] = G::P_B1; m.p_s[0] = G::P_S1; m.p_w[1] = G::P_W2; m.p_b[1] = G::P_B2;
    m.p_s[1] = G::P_S2; m.p_wo = G::P_WO; m.p_bo = G::P_BO; m.p_so = G::P_SO; m.P = G::P;
    m.sl_tile = G::SL_TILE; m.sl_cols = G::SL_COLS; m.KG = G::KG; m.kg_magic = 65536 / G::KG + 1;
    return KernelEntry{H, C, 2, icnn2_step_kernel<H, C, true>, icnn2_step_kernel<H, C, true, true>,
                       {icnn2_step_kernel<H, C, true>, icnn2_step_kernel<H, C, true, false, INR_ACT_COS>,
                        icnn2_step_kernel<H, C, true, false, INR_ACT_SIN>},
                       {icnn2_step_kernel<H, C, false>, icnn2_step_kernel<H, C, false, false, INR_ACT_COS>,
                        icnn2_step_kernel<H, C, false, false, INR_ACT_SIN>},
                       icnn2_step_kernel<H, C, false>, G::LDS_BYTES, G::P, m};
}

const KernelEntry kEntries[] = {
    make_entry<130, 2>(),  make_entry<130, 3>(),  make_entry<64, 2>(),  make_entry<64, 3>(),  make_entry<32, 2>(),
    make_entry<32, 3>(),   make_entry2<130, 2>(), make_entry2<130, 3>(), make_entry2<64, 2>(), make_entry2<64, 3>(),
};

// the kernel a model runs on: its own shape if compiled, else the smallest compiled width above it (zero-padded, user_param_index)
const KernelEntry* find_entry(const InrModelDesc* m) {
    if (!m || m->kind != INR_MODEL_ICNN || m->n_hidden < 1) return nullptr;
    if (m->n_features < 0 || m->n_out < 0 || wide_desc_general(m)) return nullptr;   // own feature width / several outputs / no hidden layer
    const KernelEntry* best = nullptr;
    for (const auto& e : kEntries)
        if (e.c == m->in_features && e.l == m->n_layers && e.h >= m->n_hidden && (!best || e.h < best->h)) best = &e;
    return best;
}

// Workgroups (= gradient slabs) per launch.  The chunk -> workgroup map fixes the order in which the points' gradient
// contributions are added up, so it must not depend on the box: this is the MI355X's CU count as a CONSTANT, not a device query
// (a partition with fewer CUs runs the same 256 workgroups in several rounds and gets the same bits).  It does depend on how
// many images share a launch (256 / n_images workgroups each): image k of a batch and the same image alone agree to rounding,
// not bit for bit (tests/test_gpu_determinism.py bounds it).
constexpr int INR_SLAB_BASE = 256;
int g_slab_base_override = 0;   // inrfit_debug_set_slab_base (tests / measurement only)

int wgs_per_image(long long n_points, int n_images) {
    const long long n_chunks = (n_points + SP - 1) / SP;
    long long w = (g_slab_base_override > 0 ? g_slab_base_override : INR_SLAB_BASE) / (n_images > 0 ? n_images : 1);
    if (w < 1) w = 1;
    if (w > n_chunks) w = n_chunks;
    return (int)w;
}

// what every path asks of a grid: a known mode with its pointers, width x height = n_points in (0, max_points], images; the callers
// add their own rules (check_grid, check_pcn)
bool grid_ok(const InrGridDesc* g, int n_images, long long max_points = 0x7fffffffLL) {
    if (!g || g->n_points <= 0 || g->n_points > max_points || n_images <= 0) return false;
    if (g->mode == INR_GRID_SEPARABLE) return g->xs && g->ys && (long long)g->width * g->height == g->n_points;
    return g->mode == INR_GRID_EXPLICIT && g->coords;
}

int check_grid(const InrGridDesc* g, const KernelEntry* e, int n_images) {
    if (!grid_ok(g, n_images)) return INR_EINVAL;
    if (g->mode == INR_GRID_SEPARABLE && (g->width <= 0 || g->height <= 0 || e->c > 3)) return INR_EINVAL;
    return INR_OK;
}

int set_lds(const KernelEntry* e) {
    // >64 KiB of dynamic LDS needs the opt-in attribute (idempotent, cheap)
    if (hipFuncSetAttribute((const void*)e->train, hipFuncAttributeMaxDynamicSharedMemorySize, e->lds_bytes) != hipSuccess)
        return INR_ELAUNCH;
    if (hipFuncSetAttribute((const void*)e->fwd, hipFuncAttributeMaxDynamicSharedMemorySize, e->lds_bytes) != hipSuccess)
        return INR_ELAUNCH;
    if (hipFuncSetAttribute((const void*)e->train_dx, hipFuncAttributeMaxDynamicSharedMemorySize, e->lds_bytes) != hipSuccess)
        return INR_ELAUNCH;
    for (int k = 1; k < 3; ++k) {
        if (hipFuncSetAttribute((const void*)e->train_act[k], hipFuncAttributeMaxDynamicSharedMemorySize, e->lds_bytes) != hipSuccess ||
            hipFuncSetAttribute((const void*)e->fwd_act[k], hipFuncAttributeMaxDynamicSharedMemorySize, e->lds_bytes) != hipSuccess)
            return INR_ELAUNCH;
    }
    return INR_OK;
}

// Gradient slab buffers an optimisation loop rotates through (step it uses buffer it % INR_SLAB_BUFFERS).  A step kernel that writes
// its slabs over the very lines the update kernel of the previous step has just read - lines that then sit, clean, in the L2s of all
// eight XCDs - runs 3.6 us longer than one that writes lines nobody has touched for a few launches (measured: DESIGN.md 6).
constexpr int INR_SLAB_BUFFERS = 4;

struct Workspace {
    float* coef;
    float* wimg;
    float* slabs;            // the buffer of the current step (set_step rotates it)
    float* loss_part;        // ... and its tail: the workgroups' loss partials once more, dense [n_images][wgs]
    float* slabs0;           // buffer 0
    long long slab_floats;   // floats per buffer (slabs + loss partials)
    long long loss_off;      // floats from a buffer's start to its loss partials
    int wgs, PS;
    long long bytes;
    void set_step(int it) {
        slabs = slabs0 + (size_t)(it % INR_SLAB_BUFFERS) * slab_floats;
        loss_part = slabs + loss_off;
    }
    int act0 = INR_ACT_RELU;     // layer-0 activation of the model this workspace was prepared for
    float act_omega = 0.f;
    int hu = 0, Pu = 0;          // the caller's n_hidden and parameter count (set_user; hu < e->h: zero-padded on the kernel's width)
    void set_user(const KernelEntry* e, const InrModelDesc* m) {
        hu = m ? m->n_hidden : e->h;
        const long long h = hu, c = e->c, l = e->l;
        Pu = (int)(h * c + h + l * (h * h + h + h * c) + h + 1 + c);
    }
};

Workspace carve(const KernelEntry* e, long long n_points, int n_images, void* base) {
    Workspace w;
    w.wgs = wgs_per_image(n_points, n_images);
    w.PS = (e->img.sl_cols + 31) / 32 * 32;   // slab rows start on 128-byte lines (the tile stores are whole lines then: -0.3 us)
    const long long coef_bytes = ((long long)n_images * 2 * 4 + 255) / 256 * 256;
    const long long img_bytes = ((long long)n_images * e->img.floats * 4 + 255) / 256 * 256;
    w.loss_off = ((long long)n_images * w.wgs * w.PS + 63) / 64 * 64;
    w.slab_floats = w.loss_off + ((long long)n_images * w.wgs + 63) / 64 * 64;
    const long long slab_bytes = w.slab_floats * 4 * INR_SLAB_BUFFERS;
    w.coef = (float*)base;
    w.wimg = (float*)((char*)base + coef_bytes);
    w.slabs0 = w.slabs = (float*)((char*)base + coef_bytes + img_bytes);
    w.loss_part = w.slabs + w.loss_off;
    w.bytes = coef_bytes + img_bytes + slab_bytes;
    return w;
}

}  // namespace

// Measurement only (bench.py): nothing but independent v_mfma_f32_16x16x4_f32 on every SIMD of the chip - what the matrix pipes
// sustain at the clock the chip holds under that load (tools/micro/mfma_rate.hip is the stand-alone version with LDS variants).
__global__ __launch_bounds__(256) void mfma_stream_kernel(float* __restrict__ sink, int iters) {
    f32x4 acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    // operands with the bit activity of real data (the clock the chip holds depends on it): 36 pseudo-random values in (-1, 1)
    f32x4 av[8], bv;
    unsigned h = (blockIdx.x * 256u + threadIdx.x) * 2654435761u + 12345u;
    auto rnd = [&]() { h = h * 1664525u + 1013904223u; return (float)(int)(h >> 8) * (1.f / 8388608.f) - 1.f; };
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) av[t][r] = rnd();
#pragma unroll
    for (int r = 0; r < 4; ++r) bv[r] = rnd();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int t = 0; t < 8; ++t) acc[t] = MFMA16(av[t][r], bv[r], acc[t]);
            __builtin_amdgcn_sched_barrier(0x7F6);
        }
    }
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t) s += acc[t][0] + acc[t][1] + acc[t][2] + acc[t][3];
    if (s == 12345.678f) sink[blockIdx.x * 256 + threadIdx.x] = s;   // never true: keeps the products alive
}


// ---------------------------------------------------------------------------------------------------------------------
// CNNNet segmentation step (csrc/cnnseg.h)
// ---------------------------------------------------------------------------------------------------------------------
namespace {

struct CnnWs {
    int n, L, Wd, cin, P, nb, tiles, tiles_x, rblocks;
    float *act, *f, *s, *u, *e, *g, *t, *tout, *df, *dl, *stats_part, *stats, *slab;
    int32_t* flags;
    long long bytes;
    float* map(float* base, int l) const { return base + (size_t)l * Wd * n; }
};

static bool cnn_desc_ok(const InrCnnSegDesc* d) {
    return d && d->kernel_size == 3 && d->width == CNN_WIDTH && d->depth >= 0 && d->depth <= CNN_MAX_LAYERS - 2 &&
           d->in_channels >= 1 && d->in_channels <= CNN_MAX_IN && d->image_channels >= 0 && d->image_channels <= d->in_channels &&
           d->height >= 1 && d->width_px >= 1 && (long long)d->height * d->width_px < (1LL << 30);
}

static long long cnn_param_count(const InrCnnSegDesc* d) {
    const long long W = d->width;
    return (W * d->in_channels * 9 + W) + (long long)d->depth * (W * W * 9 + W) + (W * 9 + 1);
}

static CnnWs cnn_layout(const InrCnnSegDesc* d, void* base) {
    CnnWs w{};
    w.n = d->height * d->width_px;
    w.L = d->depth + 2;
    w.Wd = d->width;
    w.cin = d->in_channels;
    w.P = (int)cnn_param_count(d);
    w.nb = (w.n + CNN_BLOCK - 1) / CNN_BLOCK;
    w.tiles_x = (d->width_px + CNN_TILE - 1) / CNN_TILE;
    w.tiles = w.tiles_x * ((d->height + CNN_TILE - 1) / CNN_TILE);
    w.rblocks = (w.P + CNN_BLOCK - 1) / CNN_BLOCK;
    char* p = (char*)base;
    long long off = 0;
    auto take = [&](long long floats) {
        float* r = (float*)(p + off);
        off += (floats * 4 + 255) / 256 * 256;
        return r;
    };
    const long long maps = (long long)(w.L - 1) * w.Wd * w.n;
    w.act = take(maps);
    w.f = take(w.n);
    w.s = take(w.n);
    w.u = take(w.n);
    w.e = take(maps);
    w.g = take((long long)w.cin * w.n);
    w.t = take(maps);
    w.tout = take(w.n);
    w.df = take(w.n);
    w.dl = take(maps);
    w.stats_part = take((long long)w.nb * CNN_STATS);
    w.stats = take(CNN_STATS);
    w.slab = take((long long)w.tiles * w.P);
    w.flags = (int32_t*)take(w.rblocks);
    w.bytes = off;
    return w;
}

static void cnn_conv(const CnnWs& w, const InrCnnSegDesc* d, bool transposed, const float* x0, const float* x1, int c0, int ci, int co,
                     const float* wt, const float* b, int act, const float* mask, float slope, float* out, hipStream_t s) {
    CnnConvArgs a{x0, x1, c0, ci, co, wt, b, act, mask, slope, out, d->height, d->width_px};
    const dim3 grid(w.nb), block(CNN_BLOCK);
    if (transposed) {
        if (co == 1) hipLaunchKernelGGL((cnn_conv_kernel<1, true>), grid, block, 0, s, a);
        else if (co <= CNN_MAX_IN) hipLaunchKernelGGL((cnn_conv_kernel<CNN_MAX_IN, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((cnn_conv_kernel<CNN_WIDTH, true>), grid, block, 0, s, a);
    } else {
        if (co == 1) hipLaunchKernelGGL((cnn_conv_kernel<1, false>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((cnn_conv_kernel<CNN_WIDTH, false>), grid, block, 0, s, a);
    }
}

// layer l: input channels / output channels
static inline int cnn_ci(const CnnWs& w, int l) { return l == 0 ? w.cin : w.Wd; }
static inline int cnn_co(const CnnWs& w, int l) { return l == w.L - 1 ? 1 : w.Wd; }
static inline float cnn_slope(int l) { return l == 0 ? 0.01f : 0.f; }   // the mask of activation l: LeakyReLU, then ReLU

static CnnPointArgs cnn_point_args(const CnnWs& w, const InrCnnSegDesc* d, const float* target) {
    CnnPointArgs a{};
    a.f = w.f;
    a.target = target;
    a.seg = w.s;
    a.u = w.u;
    a.g = w.g;
    a.stats_part = w.stats_part;
    a.n = w.n;
    a.inversion = d->inversion;
    a.use_noneclass = d->use_noneclass;
    a.noneclass = d->noneclass;
    a.cin = w.cin;
    a.penalty = d->penalty;
    int cnt[3] = {0, 0, 0};
    for (int c = 0; c < w.cin; ++c)
        if (d->channel_group[c] >= 0 && d->channel_group[c] < 3) cnt[d->channel_group[c]]++;
    for (int c = 0; c < CNN_MAX_IN; ++c) {
        const int grp = c < w.cin ? d->channel_group[c] : -1;
        const bool on = grp >= 0 && grp < 3 && d->coef[grp] != 0.f;
        a.group[c] = on ? grp : -1;
        a.qscale[c] = on ? (float)((double)d->g * d->coef[grp] / ((double)cnt[grp] * w.n)) : 0.f;
    }
    return a;
}

// pass 1 (+ pass 2 and the loss value with a target)
static int cnn_forward_passes(const CnnWs& w, const InrCnnSegDesc* d, const float* const* wts, const float* const* bs, const float* image,
                              const float* feat, const float* target, float* logits, float* seg, float* loss_out, hipStream_t s) {
    const int ic = d->image_channels;
    for (int l = 0; l < w.L; ++l) {
        const bool first = l == 0, last = l == w.L - 1;
        const float* x0 = first ? image : w.map(w.act, l - 1);
        const float* x1 = first ? feat : x0;
        cnn_conv(w, d, false, x0, x1, first ? ic : cnn_ci(w, l), cnn_ci(w, l), cnn_co(w, l), wts[l], bs[l], last ? 0 : (first ? 1 : 2),
                 nullptr, 0.f, last ? w.f : w.map(w.act, l), s);
    }
    CnnPointArgs pa = cnn_point_args(w, d, target);
    pa.f_out = logits;
    pa.seg_out = seg;
    hipLaunchKernelGGL(cnn_head_kernel, dim3(w.nb), dim3(CNN_BLOCK), 0, s, pa);
    if (!target) return INR_OK;
    if (d->penalty) {   // pass 2: e_{L-1} = u, e_{l-1} = m_{l-1} conv_l^T(e_l), g = conv_0^T(e_0)
        for (int l = w.L - 1; l >= 0; --l) {
            const float* src = l == w.L - 1 ? w.u : w.map(w.e, l);
            if (l > 0)
                cnn_conv(w, d, true, src, src, cnn_co(w, l), cnn_co(w, l), cnn_ci(w, l), wts[l], nullptr, 0, w.map(w.act, l - 1),
                         cnn_slope(l - 1), w.map(w.e, l - 1), s);
            else
                cnn_conv(w, d, true, src, src, cnn_co(w, 0), cnn_co(w, 0), w.cin, wts[0], nullptr, 0, nullptr, 0.f, w.g, s);
        }
    }
    hipLaunchKernelGGL(cnn_stats_kernel, dim3(w.nb), dim3(CNN_BLOCK), 0, s, pa);
    CnnLossArgs la{};
    la.stats_part = w.stats_part;
    la.blocks = w.nb;
    la.stats = w.stats;
    la.loss_out = w.stats + 6;
    la.loss_user = loss_out;
    la.gfac = d->g;
    int cnt[3] = {0, 0, 0};
    for (int c = 0; c < w.cin; ++c)
        if (d->channel_group[c] >= 0 && d->channel_group[c] < 3) cnt[d->channel_group[c]]++;
    for (int grp = 0; grp < 3; ++grp)
        la.pen_scale[grp] = (d->penalty && d->coef[grp] != 0.f && cnt[grp] > 0) ? (float)((double)d->coef[grp] / ((double)cnt[grp] * w.n)) : 0.f;
    hipLaunchKernelGGL(cnn_loss_kernel, dim3(1), dim3(CNN_BLOCK), 0, s, la);
    return INR_OK;
}

static int cnn_check(const InrCnnSegDesc* d, const float* const* wts, const float* const* bs, const float* image, const float* feat,
                     void* ws, long long ws_bytes, CnnWs* w) {
    if (!d || !wts || !bs || !image || !ws) return INR_EINVAL;
    if (!cnn_desc_ok(d)) return INR_EUNSUPPORTED;
    if (d->image_channels < d->in_channels && !feat) return INR_EINVAL;
    for (int l = 0; l < d->depth + 2; ++l)
        if (!wts[l] || !bs[l]) return INR_EINVAL;
    *w = cnn_layout(d, ws);
    if (ws_bytes < w->bytes) return INR_EWORKSPACE;
    return INR_OK;
}

}  // namespace

extern "C" {

int64_t inrfit_cnnseg_param_count(const InrCnnSegDesc* desc) { return cnn_desc_ok(desc) ? cnn_param_count(desc) : -1; }

int64_t inrfit_cnnseg_workspace_bytes(const InrCnnSegDesc* desc) {
    return cnn_desc_ok(desc) ? cnn_layout(desc, nullptr).bytes : -1;
}

int inrfit_cnnseg_forward(const InrCnnSegDesc* desc, const float* const* weights, const float* const* biases, const float* image,
                          const float* features, const float* target, float* logits, float* seg, float* loss_out, void* workspace,
                          int64_t workspace_bytes, void* stream) {
    CnnWs w;
    int rc = cnn_check(desc, weights, biases, image, features, workspace, workspace_bytes, &w);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = cnn_forward_passes(w, desc, weights, biases, image, features, target, logits, seg, loss_out, s))) return rc;
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

int inrfit_cnnseg_step(const InrCnnSegDesc* desc, const float* const* weights, const float* const* biases, const float* image,
                       const float* features, const float* target, const float* dseg, int reuse_forward, float* logits, float* seg,
                       float* loss_out, float* grads, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream) {
    CnnWs w;
    int rc = cnn_check(desc, weights, biases, image, features, workspace, workspace_bytes, &w);
    if (rc) return rc;
    if (!target || !grads || !status) return INR_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (!reuse_forward && (rc = cnn_forward_passes(w, desc, weights, biases, image, features, target, logits, seg, nullptr, s))) return rc;
    const bool pen = desc->penalty != 0;
    if (pen) {   // pass 3: t_l = m_l conv_l(t_{l-1}) from t_{-1} = q (in w.g), no biases
        for (int l = 0; l < w.L; ++l) {
            const bool last = l == w.L - 1;
            const float* x0 = l == 0 ? w.g : w.map(w.t, l - 1);
            cnn_conv(w, desc, false, x0, x0, cnn_ci(w, l), cnn_ci(w, l), cnn_co(w, l), weights[l], nullptr, 0,
                     last ? nullptr : w.map(w.act, l), cnn_slope(l), last ? w.tout : w.map(w.t, l), s);
        }
    }
    CnnSeedArgs sa{w.s, w.f, target, w.stats, pen ? w.tout : nullptr, dseg, w.df, w.n, desc->inversion, desc->use_noneclass,
                   desc->noneclass};
    hipLaunchKernelGGL(cnn_seed_kernel, dim3(w.nb), dim3(CNN_BLOCK), 0, s, sa);
    // pass 4: d_{l-1} = m_{l-1} conv_l^T(d_l)
    for (int l = w.L - 1; l > 0; --l) {
        const float* src = l == w.L - 1 ? w.df : w.map(w.dl, l);
        cnn_conv(w, desc, true, src, src, cnn_co(w, l), cnn_co(w, l), cnn_ci(w, l), weights[l], nullptr, 0, w.map(w.act, l - 1),
                 cnn_slope(l - 1), w.map(w.dl, l - 1), s);
    }
    int off = 0;
    for (int l = 0; l < w.L; ++l) {
        const int ci = cnn_ci(w, l), co = cnn_co(w, l);
        CnnWgradArgs a{};
        a.x0 = l == 0 ? image : w.map(w.act, l - 1);
        a.x1 = l == 0 ? features : a.x0;
        a.c0 = l == 0 ? desc->image_channels : ci;
        a.d = l == w.L - 1 ? w.df : w.map(w.dl, l);
        a.t = pen ? (l == 0 ? w.g : w.map(w.t, l - 1)) : nullptr;
        a.e = l == w.L - 1 ? w.u : w.map(w.e, l);
        a.ci = ci;
        a.co = co;
        a.H = desc->height;
        a.W = desc->width_px;
        a.tiles_x = w.tiles_x;
        a.slab = w.slab;
        a.P = w.P;
        a.w_off = off;
        a.b_off = off + co * ci * 9;
        off = a.b_off + co;
        hipLaunchKernelGGL(cnn_wgrad_kernel<CNN_WIDTH>, dim3(w.tiles), dim3(CNN_BLOCK), 0, s, a);
    }
    if (off != w.P) return INR_EINVAL;
    hipLaunchKernelGGL(cnn_grad_reduce_kernel, dim3(w.rblocks), dim3(CNN_BLOCK), 0, s, (const float*)w.slab, w.tiles, w.P, grads, w.flags);
    hipLaunchKernelGGL(cnn_finalize_kernel, dim3(1), dim3(CNN_BLOCK), 0, s, (const int32_t*)w.flags, w.rblocks,
                       (const float*)(w.stats + 6), grads, w.P, status, loss_out);
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

}  // extern "C"

extern "C" {

int inrfit_query(int* abi_version, int* max_hidden, int* lds_bytes) {
    if (abi_version) *abi_version = INRFIT_ABI_VERSION;
    if (max_hidden) *max_hidden = 130;
    if (lds_bytes) *lds_bytes = Cfg<130, 2>::LDS_BYTES;
    return INR_OK;
}

#define INRFIT_STR_(x) #x
#define INRFIT_STR(x) INRFIT_STR_(x)
#ifndef INRFIT_BUILD_FLAGS
#define INRFIT_BUILD_FLAGS "unknown (not built by awesome_amd/build.py)"
#endif
const char* inrfit_build_info(void) {
    return "libinrfit abi " INRFIT_STR(INRFIT_ABI_VERSION) "; gfx950; slab_base 256; " __VERSION__ "; flags: " INRFIT_BUILD_FLAGS;
}

int inrfit_debug_set_slab_base(int slab_base) {
    if (slab_base < 0 || slab_base > 4096) return INR_EINVAL;
    g_slab_base_override = slab_base;
    return INR_OK;
}

int inrfit_slabs_per_image(int64_t n_points, int n_images) {
    if (n_points <= 0 || n_images <= 0) return INR_EINVAL;
    return wgs_per_image(n_points, n_images);
}

int inrfit_supported(const InrModelDesc* model) { return (find_entry(model) || wide_shape_ok(model)) ? 1 : 0; }

int64_t inrfit_param_count(const InrModelDesc* m) {
    if (!m || m->kind != INR_MODEL_ICNN || m->n_hidden <= 0 || m->in_features <= 0 || m->n_layers < 0) return INR_EINVAL;
    if (m->n_features < 0 || m->n_features > WIDE_MAX_HIDDEN || m->n_out < 0 || m->n_out > 4) return INR_EINVAL;
    // W_in [F][C], b_in [F] | W_0 [h][F], b_0, S_0 | W_k [h][h], b_k, S_k (k >= 1) | W_o [O][h or F], b_o [O], S_o [O][C]
    const int64_t h = m->n_hidden, c = m->in_features, l = m->n_layers, f = wide_desc_F(m), o = wide_desc_O(m);
    const int64_t hidden = l > 0 ? (h * f + h + h * c) + (l - 1) * (h * h + h + h * c) : 0;
    return f * c + f + hidden + o * (l > 0 ? h : f) + o + o * c;
}

int64_t inrfit_opt_state_floats(const InrModelDesc* m) {
    const int64_t p = inrfit_param_count(m);
    return p < 0 ? p : 2 * p + INR_OPT_HEADER_FLOATS;
}

int64_t inrfit_workspace_bytes(const InrModelDesc* model, const InrGridDesc* grid, int n_images) {
    const KernelEntry* e = find_entry(model);
    if (!e && wide_shape_ok(model)) {
        if (!grid || grid->n_points <= 0 || n_images <= 0) return INR_EINVAL;
        return wide_total_bytes(make_wide_map(model), grid->n_points, model->act0 != INR_ACT_RELU, n_images);
    }
    if (!e) return INR_EUNSUPPORTED;
    if (!grid || grid->n_points <= 0 || n_images <= 0) return INR_EINVAL;
    return carve(e, grid->n_points, n_images, nullptr).bytes;
}

static int launch_pack(const KernelEntry* e, const Workspace& w, const float* params, int n_images, hipStream_t s) {
    hipLaunchKernelGGL(pack_image_kernel, dim3((e->img.floats + 255) / 256, n_images), dim3(256), 0, s, w.wimg, e->img);
    hipLaunchKernelGGL(pack_params_kernel, dim3((e->P + 255) / 256, n_images), dim3(256), 0, s, params, w.wimg, e->img, w.hu, w.Pu);
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

// What a joint step adds to the data term of a training pass: the align term against `seg` and the mask of the data term proper.
// One description for both backbones (the step kernel's StepArgs, wide.h's WideJoint); the default is what every other caller
// runs: no align term, all points.
struct DataTerm {
    const float* align_seg = nullptr;   // [N]: the align term's target, or null
    float c_align = 0.f;
    long long data_count = 0;           // 0 = all points
    int use_noneclass = 0;
    float noneclass = 0.f;
    int align_soft = 0;
    long long align_begin = 0;
};

static int launch_step(const KernelEntry* e, const Workspace& w, bool train, const InrGridDesc* grid, const float* targets,
                       int loss_kind, int n_images, float* logits, hipStream_t s, float* dcoords = nullptr,
                       const DataTerm& mask = DataTerm{}) {
    StepArgs a{};
    a.dcoords = dcoords;
    a.seg = mask.align_seg;
    a.c_align = mask.c_align;
    a.data_count = (int)(mask.data_count > 0 ? mask.data_count : grid->n_points);
    a.use_noneclass = mask.use_noneclass;
    a.noneclass = mask.noneclass;
    a.align_soft = mask.align_soft;
    a.align_begin = (int)mask.align_begin;
    a.wimg = w.wimg;
    a.targets = targets;
    a.coef = w.coef;
    a.slabs = w.slabs;
    a.loss_part = w.loss_part;
    a.logits = logits;
    a.grid = *grid;
    a.N = grid->n_points;
    a.n_images = n_images;
    a.wgs = w.wgs;
    a.PS = w.PS;
    a.loss_kind = loss_kind;
    a.act_omega = w.act_omega;
    if (dcoords && w.act0 != INR_ACT_RELU) return INR_EUNSUPPORTED;   // coordinate gradients: relu networks only
    hipLaunchKernelGGL(train ? (dcoords ? e->train_dx : e->train_act[w.act0]) : e->fwd_act[w.act0], dim3((unsigned)(n_images * w.wgs)),
                       dim3(WG_THREADS), e->lds_bytes, s, a);
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

// ---- measurement hook: HIP events around single step-kernel launches while it is armed (bench.py) -------------------------
struct StepTiming {
    bool on = false;
    int max_samples = 0;
    std::vector<hipEvent_t> ev;   // pairs (before, after) around step-kernel launches
    std::vector<hipEvent_t> evu;  // ... around update-kernel launches (inrfit_fit only)
};
static thread_local StepTiming g_timing;

static int launch_step_timed(const KernelEntry* e, const Workspace& w, const InrGridDesc* grid, const float* targets, int loss_kind,
                             int n_images, hipStream_t s, float* logits = nullptr) {
    if (!g_timing.on || (int)g_timing.ev.size() >= 2 * g_timing.max_samples)
        return launch_step(e, w, true, grid, targets, loss_kind, n_images, logits, s);
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return INR_ELAUNCH;
    (void)hipEventRecord(a, s);
    const int rc = launch_step(e, w, true, grid, targets, loss_kind, n_images, logits, s);
    (void)hipEventRecord(b, s);
    g_timing.ev.push_back(a);
    g_timing.ev.push_back(b);
    return rc;
}

static int check_loss(const InrLossDesc* l) {
    if (!l) return INR_EINVAL;
    if (l->kind != INR_LOSS_SE && l->kind != INR_LOSS_BCE && l->kind != INR_LOSS_EXTERNAL) return INR_EINVAL;
    if (l->weight_mode < INR_WEIGHT_NONE || l->weight_mode > INR_WEIGHT_EXPLICIT) return INR_EINVAL;
    return INR_OK;
}

// the ICNN update arguments shared by every fit loop (t, bias corrections and hist_idx are set per step)
static UpdArgs make_upd_args(const KernelEntry* e, const Workspace& w, float* params, float* opt_state, float* loss_hist,
                             int32_t* status, const InrOptDesc* opt, int n_images, int steps) {
    UpdArgs u{};
    u.wimg = w.wimg;
    u.img = e->img;
    u.params = params;
    u.opt_state = opt_state;
    u.slabs = w.slabs;
    u.loss_part = w.loss_part;
    u.loss_stride = 1;
    u.loss_hist = loss_hist;
    u.status = status;
    u.opt = *opt;
    u.P = e->P;
    u.Pu = w.Pu;
    u.hu = w.hu;
    u.PS = w.PS;
    u.wgs = w.wgs;
    u.n_images = n_images;
    u.hist_stride = steps;
    u.mode = 0;
    for (int k = 0; k < UPD_RANGES; ++k) u.clamp_lo[k] = u.clamp_hi[k] = 0;
    for (int k = 0; k < e->img.L; ++k) {
        u.clamp_lo[k] = e->img.p_w[k];
        u.clamp_hi[k] = e->img.p_w[k] + e->img.H * e->img.H;
    }
    u.clamp_lo[UPD_RANGES - 1] = e->img.p_wo;
    u.clamp_hi[UPD_RANGES - 1] = e->img.p_wo + e->img.H;
    for (int k = 0; k < UPD_RANGES; ++k) u.freeze_lo[k] = u.freeze_hi[k] = 0;
    for (int k = 0; k < e->img.L; ++k) {
        u.freeze_lo[k] = e->img.p_s[k];
        u.freeze_hi[k] = e->img.p_s[k] + e->img.H * e->img.C;
    }
    u.freeze_lo[UPD_RANGES - 1] = e->img.p_so;
    u.freeze_hi[UPD_RANGES - 1] = e->img.p_so + e->img.C;
    u.input_hi = e->img.p_w[0];
    return u;
}

// what changes from one optimizer step of a loop to the next (t is 1-based)
static void set_step_consts(UpdArgs& u, const InrOptDesc* opt, int t, int hist_idx = 0) {
    u.t = t;
    u.c = opt_consts(opt, t);
    u.hist_idx = hist_idx;
}

static void launch_icnn_update(const KernelEntry* e, const UpdArgs& u, hipStream_t s) {
    hipLaunchKernelGGL(icnn_update_kernel, upd_grid(e->img.sl_cols, u.n_images), upd_block(e->img.sl_cols), 0, s, u, upd_split(e->img.sl_cols).n_wide);
}

// the update-kernel half of bench.py's timing hook (launch_step_timed is the step kernel's)
static int launch_icnn_update_timed(const KernelEntry* e, const UpdArgs& u, hipStream_t s) {
    if (!g_timing.on || (int)g_timing.evu.size() >= 2 * g_timing.max_samples) {
        launch_icnn_update(e, u, s);
        return INR_OK;
    }
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return INR_ELAUNCH;
    (void)hipEventRecord(a, s);
    launch_icnn_update(e, u, s);
    (void)hipEventRecord(b, s);
    g_timing.evu.push_back(a);
    g_timing.evu.push_back(b);
    return INR_OK;
}

// common argument checks + workspace carve (every argument first: the device's turn is prepare's set_lds)
static int prepare_args(const InrModelDesc* model, const InrGridDesc* grid, int n_images, void* workspace, int64_t workspace_bytes,
                        const KernelEntry** e_out, Workspace* w_out) {
    const KernelEntry* e = find_entry(model);
    if (!e) return INR_EUNSUPPORTED;
    if (!workspace) return INR_EINVAL;
    int rc = check_grid(grid, e, n_images);
    if (rc) return rc;
    *w_out = carve(e, grid->n_points, n_images, workspace);
    w_out->set_user(e, model);
    if (workspace_bytes < w_out->bytes) return INR_EWORKSPACE;
    if (model->act0 < INR_ACT_RELU || model->act0 > INR_ACT_SIN) return INR_EINVAL;
    w_out->act0 = model->act0;
    w_out->act_omega = model->act_omega;
    *e_out = e;
    return INR_OK;
}
static int prepare(const InrModelDesc* model, const InrGridDesc* grid, int n_images, void* workspace, int64_t workspace_bytes,
                   const KernelEntry** e_out, Workspace* w_out) {
    if (const int rc = prepare_args(model, grid, n_images, workspace, workspace_bytes, e_out, w_out)) return rc;
    return set_lds(*e_out);
}

static void launch_reduce(const KernelEntry* e, const Workspace& w, int n_images, float* grads, float* loss_out, hipStream_t s) {
    UpdArgs u{};
    u.img = e->img;
    u.slabs = w.slabs;
    u.grads_out = grads;
    u.loss_out = loss_out;
    u.P = e->P;
    u.Pu = w.Pu;
    u.hu = w.hu;
    u.PS = w.PS;
    u.wgs = w.wgs;
    u.n_images = n_images;
    u.mode = 1;
    hipLaunchKernelGGL(icnn_update_kernel, upd_grid(e->img.sl_cols, n_images), upd_block(e->img.sl_cols), 0, s, u, upd_split(e->img.sl_cols).n_wide);
}


// ---------------------------------------------------------------------------------------------------------------------
// the layer-by-layer path (wide.h): shapes without a fused kernel - n_hidden > 130, more than two hidden layers, or a general shape
// (n_features != n_hidden, n_out > 1, no hidden layer)
// ---------------------------------------------------------------------------------------------------------------------
static bool use_wide(const InrModelDesc* m) { return find_entry(m) == nullptr && wide_shape_ok(m); }

// An ICNN-form shape of the layer-by-layer path: relu layer 0, one output, square layers.  What the RealNVP composite and the joint
// steps accept (the encode shapes stay refused there).
static bool pcn_wide_shape(const InrModelDesc* m) { return use_wide(m) && m->act0 == INR_ACT_RELU && !wide_desc_general(m); }

// ... and behind the coupling flow, which is 2-D only: every other shape keeps the answers of the fused route's checks
static bool cdn_wide_shape(const InrModelDesc* m) { return m && pcn_wide_shape(m) && m->in_features == 2; }

long long align256(long long b) { return (b + 255) / 256 * 256; }

// the layer-by-layer workspace behind a deformation's buffers (an ICNN-form shape): logits [N] | dL/dlogits [N] | ONE image's
// layer-by-layer workspace | the loss coefficients of every image
struct WideBehind {
    float *logit, *dy, *coef;
    WideWs w;
    long long bytes;
};
static WideBehind carve_wide_behind(const WideMap& m, long long N, int n_images, void* base) {
    WideBehind q;
    char* b = (char*)base;
    long long off = 0;
    q.logit = (float*)(b + off); off += align256(N * 4);
    q.dy = (float*)(b + off); off += align256(N * 4);
    q.w = carve_wide(m, N, false, b + off);
    off += q.w.bytes;
    q.coef = (float*)(b + off); off += wide_align((long long)n_images * 2 * 4);
    q.bytes = off;
    return q;
}

// the optimizer step of the layer-by-layer path = icnn_update_kernel on a one-"slab" view of the gradient vector (column = parameter,
// column P = the loss): the arguments every such loop shares (params, opt_state, loss_hist and status are set per image; t, the bias
// corrections and hist_idx per step)
static UpdArgs wide_upd_args(const WideMap& m, const float* grads, const InrOptDesc* opt, int steps) {
    UpdArgs u{};
    u.img.identity = 1;
    u.img.H = m.h; u.img.C = m.C; u.img.L = m.L; u.img.P = m.P; u.img.sl_cols = m.P + 1;
    u.opt = *opt;
    u.P = u.Pu = m.P;
    u.hu = m.h;
    u.PS = (m.P + 1 + 31) / 32 * 32;
    u.wgs = 1;
    u.n_images = 1;
    u.hist_stride = steps;
    u.slabs = grads;
    u.loss_part = grads + m.P;   // the one-slab view's loss column, in place
    u.loss_stride = u.PS;
    for (int k = 0; k < UPD_RANGES; ++k) u.clamp_lo[k] = u.clamp_hi[k] = u.freeze_lo[k] = u.freeze_hi[k] = 0;
    for (int k = 0; k < m.L; ++k) {
        u.clamp_lo[k] = m.p_w(k); u.clamp_hi[k] = m.p_w(k) + m.h * m.kin(k);
        u.freeze_lo[k] = m.p_s(k); u.freeze_hi[k] = m.p_s(k) + m.h * m.C;
    }
    u.clamp_lo[UPD_RANGES - 1] = m.p_wo(); u.clamp_hi[UPD_RANGES - 1] = m.p_wo() + m.O * m.hl();
    u.freeze_lo[UPD_RANGES - 1] = m.p_so(); u.freeze_hi[UPD_RANGES - 1] = m.p_so() + m.O * m.C;
    u.input_hi = m.p_w(0);   // input.weight | input.bias (L = 0: everything in front of the output layer)
    return u;
}
static void launch_wide_update(const WideMap& m, const UpdArgs& u, hipStream_t s) {
    hipLaunchKernelGGL(icnn_update_kernel, upd_grid(m.P + 1, 1), upd_block(m.P + 1), 0, s, u, upd_split(m.P + 1).n_wide);
}

int inrfit_step_only(const InrModelDesc* model, const float* params, const InrGridDesc* grid, const float* targets,
                     const InrLossDesc* loss, int n_images, int iters, void* workspace, int64_t workspace_bytes,
                     void* stream) {
    const KernelEntry* e;
    Workspace w;
    if (!params || !targets || iters < 0) return INR_EINVAL;
    int rc = check_loss(loss);
    if (rc) return rc;
    if ((rc = prepare(model, grid, n_images, workspace, workspace_bytes, &e, &w))) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(loss_coef_kernel, dim3(n_images), dim3(256), 0, s, targets, (long long)grid->n_points, *loss, w.coef, 1.f);
    if ((rc = launch_pack(e, w, params, n_images, s))) return rc;
    for (int it = 0; it < iters; ++it)
        if ((rc = launch_step_timed(e, w, grid, targets, loss->kind, n_images, s))) return rc;
    return INR_OK;
}

int inrfit_mfma_stream(int workgroups, int iters, double* flop, void* scratch, void* stream) {
    if (workgroups <= 0 || workgroups > 65535 || iters <= 0 || !scratch) return INR_EINVAL;
    hipLaunchKernelGGL(mfma_stream_kernel, dim3(workgroups), dim3(256), 0, (hipStream_t)stream, (float*)scratch, iters);
    if (flop) *flop = 2.0 * 16 * 16 * 4 * 32.0 * iters * 4.0 * workgroups;   // 32 products per iteration and wave, 4 waves
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

static void timing_clear() {
    for (hipEvent_t e : g_timing.ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : g_timing.evu) (void)hipEventDestroy(e);
    g_timing.ev.clear();
    g_timing.evu.clear();
}

static float timing_avg_us(const std::vector<hipEvent_t>& ev, int* n_out) {
    double sum = 0.0;
    int n = 0;
    for (size_t i = 0; i + 1 < ev.size(); i += 2) {
        float ms = 0.f;
        if (hipEventSynchronize(ev[i + 1]) == hipSuccess && hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) {
            sum += ms;
            ++n;
        }
    }
    if (n_out) *n_out = n;
    return n ? (float)(sum / n * 1e3) : 0.f;
}

int inrfit_timing_begin(int max_samples) {
    if (max_samples <= 0) return INR_EINVAL;
    timing_clear();
    g_timing.on = true;
    g_timing.max_samples = max_samples;
    return INR_OK;
}

int inrfit_timing_end(float* avg_step_bracket_us, float* avg_update_bracket_us, int* n_samples) {
    g_timing.on = false;
    int n = 0;
    const float su = timing_avg_us(g_timing.ev, &n), uu = timing_avg_us(g_timing.evu, nullptr);
    timing_clear();
    if (avg_step_bracket_us) *avg_step_bracket_us = su;
    if (avg_update_bracket_us) *avg_update_bracket_us = uu;
    if (n_samples) *n_samples = n;
    return INR_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// path-connected prior: ICNN(flow(Ax + b))
// ---------------------------------------------------------------------------------------------------------------------
namespace {

struct CdnWs {
    float *xd, *dxd, *FE, *ps, *slab1, *slab2;
    int blocks1, chunks, Wp, S1;   // blocks1 = blocks of the backward point kernel (rows of slab1)
    FlowShape sf, sb;              // launch shapes of the forward / backward point kernels (flow.h: flow_launch_shape)
    FlowMap fm;
    long long bytes;
    InrGridDesc dgrid;    // the deformed grid handed to the ICNN kernels
};

static bool flow_ok(const InrFlowDesc* f) {
    return f && f->width >= 1 && f->width <= 256 && (f->backbone == INR_FLOW_NORMAL_BLOCK || f->backbone == INR_FLOW_SIMPLE) &&
           (f->num_coupling == 2 || f->num_coupling == 4 || f->num_coupling == 6 || f->num_coupling == 8);
}

static CdnWs carve_cdn(const InrFlowDesc* f, const InrGridDesc* grid, int n_images, void* base) {
    CdnWs w;
    const long long N = grid->n_points;
    w.fm = make_flow_map(f->width, f->num_coupling, f->backbone == INR_FLOW_SIMPLE ? 0.f : LEAKY_SLOPE);
    w.sf = flow_launch_shape(N, n_images, false);
    w.sb = flow_launch_shape(N, n_images, true);
    w.blocks1 = w.sb.blocks;
    w.Wp = (f->width + 63) / 64 * 64;
    w.chunks = 64;   // x 2K nets x 4 waves: enough waves for 1024 SIMDs at one image
    while (w.chunks > 1 && N / w.chunks < 256) w.chunks /= 2;
    w.S1 = 3 * f->num_coupling + 6;
    char* b = (char*)base;
    long long off = 0;
    auto take = [&](long long bytes) { float* p = (float*)(b + off); off += align256(bytes); return p; };
    w.xd = take((long long)n_images * 2 * N * 4);
    w.dxd = take((long long)n_images * 2 * N * 4);
    w.FE = take((long long)n_images * w.fm.FE * 4);
    w.ps = take((long long)n_images * f->num_coupling * 3 * N * 4);
    w.slab1 = take((long long)n_images * w.blocks1 * w.S1 * 4);
    w.slab2 = take((long long)n_images * w.chunks * f->num_coupling * 2 * 3 * w.Wp * 4);
    w.dgrid = *grid;
    w.dgrid.mode = INR_GRID_EXPLICIT;
    w.dgrid.coords = w.xd;
    w.dgrid.coords_image_stride = 2 * N;
    w.bytes = off;
    return w;
}

FlowUpdArgs make_flow_upd_args(const CdnWs& w, int mode, float* FP, float* opt, float* grads_out, const InrOptDesc* od, float wd_g, int t,
                               const float* lr_hdr, long long hdr_stride, const int32_t* status = nullptr, const float* gscale = nullptr) {
    FlowUpdArgs u{};
    u.status = status;
    u.gscale = gscale;
    u.FP = FP;
    u.FE = w.FE;
    u.opt = opt;
    u.grads_out = grads_out;
    u.slab1 = w.slab1;
    u.slab2 = w.slab2;
    u.lr_hdr = lr_hdr;
    u.hdr_stride = hdr_stride;
    if (od) u.opt_desc = *od;
    u.m = w.fm;
    u.blocks1 = w.blocks1;
    u.S1 = w.S1;
    u.chunks = w.chunks;
    u.Wp = w.Wp;
    u.t = t;
    u.c = opt_consts(od, t);
    u.wd_g = wd_g;
    u.mode = mode;
    return u;
}

static void launch_flow_update_args(const InrFlowDesc* f, int n_images, const FlowUpdArgs& u, hipStream_t s) {
    hipLaunchKernelGGL(flow_update_kernel, dim3(2 * f->num_coupling + 1, n_images), dim3(256), 0, s, u);
}

// modes 1 (gradients only) and 2 (effective weights only)
void launch_flow_update(const CdnWs& w, const InrFlowDesc* f, int n_images, int mode, float* FP, float* grads_out, hipStream_t s) {
    launch_flow_update_args(f, n_images, make_flow_upd_args(w, mode, FP, nullptr, grads_out, nullptr, 0.f, 0, nullptr, 0), s);
}

// the ICNN update `ui` and the flow's optimizer step in one launch (cdn_update_kernel)
static void launch_cdn_update(const KernelEntry* e, const UpdArgs& ui, FlowUpdArgs uf, const InrFlowDesc* f, int n_images, hipStream_t s) {
    const int nbf = 2 * f->num_coupling + 1;
    const dim3 gi = upd_grid(e->img.sl_cols, n_images, nbf);
    uf.status = nullptr;
    uf.loss_part = ui.loss_part;
    uf.loss_wgs = ui.wgs;
    uf.loss_stride = ui.loss_stride;
    hipLaunchKernelGGL(cdn_update_kernel, dim3(gi.x + nbf, n_images), upd_block(e->img.sl_cols, nbf), 0, s, ui, uf, (int)gi.x,
                       upd_split(e->img.sl_cols, nbf).n_wide);
}

static void launch_flow_fwd(const CdnWs& w, const InrGridDesc* grid, int n_images, float* out, hipStream_t s) {
    FlowFwdArgs a{};
    a.FE = w.FE;
    a.xd = out;
    a.grid = *grid;
    a.N = grid->n_points;
    a.m = w.fm;
    const dim3 g(w.sf.blocks, n_images), b(w.sf.threads);
    const size_t lds = (w.fm.FE + 64) * sizeof(float);   // + slack: the pipelined unit loop reads one batch ahead
    if (w.sf.U == 1 && w.sf.Q == 2) hipLaunchKernelGGL((flow_fwd_kernel<2, 1>), g, b, lds, s, a);
    else if (w.sf.U == 4 && w.sf.Q == 2) hipLaunchKernelGGL((flow_fwd_kernel<2, 4>), g, b, lds, s, a);
    else if (w.sf.U == 4 && w.sf.Q == 4) hipLaunchKernelGGL((flow_fwd_kernel<4, 4>), g, b, lds, s, a);
    else if (w.sf.U == 2 && w.sf.Q == 2) hipLaunchKernelGGL((flow_fwd_kernel<2, 2>), g, b, lds, s, a);
    else if (w.sf.U == 4) hipLaunchKernelGGL((flow_fwd_kernel<1, 4>), g, b, lds, s, a);
    else if (w.sf.U == 2) hipLaunchKernelGGL((flow_fwd_kernel<1, 2>), g, b, lds, s, a);
    else hipLaunchKernelGGL((flow_fwd_kernel<1, 1>), g, b, lds, s, a);
}

static void launch_flow_bwd_points(const CdnWs& w, int K, int n_images, const FlowBwdArgs& a, hipStream_t s) {
    const dim3 g1(w.sb.blocks, n_images), b1(w.sb.threads);
    const size_t lds = (w.fm.FE + 64) * sizeof(float);
#define INR_FLOW_BWD(KK)                                                                                 \
    do {                                                                                                 \
        if (w.sb.U == 1 && w.sb.Q == 2) hipLaunchKernelGGL((flow_bwd_points_kernel<KK, 2, 1>), g1, b1, lds, s, a); \
        else if (w.sb.U == 4 && w.sb.Q == 2) hipLaunchKernelGGL((flow_bwd_points_kernel<KK, 2, 4>), g1, b1, lds, s, a); \
        else if (w.sb.U == 4) hipLaunchKernelGGL((flow_bwd_points_kernel<KK, 1, 4>), g1, b1, lds, s, a);     \
        else if (w.sb.U == 2) hipLaunchKernelGGL((flow_bwd_points_kernel<KK, 1, 2>), g1, b1, lds, s, a);     \
        else hipLaunchKernelGGL((flow_bwd_points_kernel<KK, 1, 1>), g1, b1, lds, s, a);                     \
    } while (0)
    switch (K) {
        case 2: INR_FLOW_BWD(2); break;
        case 4: INR_FLOW_BWD(4); break;
        case 6: INR_FLOW_BWD(6); break;
        default: INR_FLOW_BWD(8); break;
    }
#undef INR_FLOW_BWD
}

static void launch_flow_bwd(const CdnWs& w, const InrFlowDesc* f, const InrGridDesc* grid, int n_images, hipStream_t s) {
    FlowBwdArgs a{};
    a.FE = w.FE;
    a.dxd = w.dxd;
    a.ps = w.ps;
    a.slab1 = w.slab1;
    a.grid = *grid;
    a.N = grid->n_points;
    a.m = w.fm;
    a.S1 = w.S1;
    launch_flow_bwd_points(w, f->num_coupling, n_images, a, s);
    FlowUnitsArgs ua{};
    ua.FE = w.FE;
    ua.ps = w.ps;
    ua.slab2 = w.slab2;
    ua.N = grid->n_points;
    ua.m = w.fm;
    ua.chunks = w.chunks;
    ua.Wp = w.Wp;
    const dim3 g2(w.chunks, 2 * f->num_coupling, n_images);
    const int W = w.fm.W, rem = W % 64, full = W / 64;
    if (full >= 1 && full <= 3 && rem >= 1 && rem <= 4) {   // a few units past a multiple of 64 (W = 130): lane = point for those
#define INR_UNITS_REM(UU)                                                                                     \
    switch (rem) {                                                                                            \
        case 1: hipLaunchKernelGGL((flow_bwd_units_kernel<UU, 1>), g2, dim3(256), 0, s, ua); break;           \
        case 2: hipLaunchKernelGGL((flow_bwd_units_kernel<UU, 2>), g2, dim3(256), 0, s, ua); break;           \
        case 3: hipLaunchKernelGGL((flow_bwd_units_kernel<UU, 3>), g2, dim3(256), 0, s, ua); break;           \
        default: hipLaunchKernelGGL((flow_bwd_units_kernel<UU, 4>), g2, dim3(256), 0, s, ua); break;          \
    }
        if (full == 1) { INR_UNITS_REM(1) } else if (full == 2) { INR_UNITS_REM(2) } else { INR_UNITS_REM(3) }
#undef INR_UNITS_REM
        return;
    }
    switch (w.Wp / 64) {
        case 1: hipLaunchKernelGGL(flow_bwd_units_kernel<1>, g2, dim3(256), 0, s, ua); break;
        case 2: hipLaunchKernelGGL(flow_bwd_units_kernel<2>, g2, dim3(256), 0, s, ua); break;
        case 3: hipLaunchKernelGGL(flow_bwd_units_kernel<3>, g2, dim3(256), 0, s, ua); break;
        default: hipLaunchKernelGGL(flow_bwd_units_kernel<4>, g2, dim3(256), 0, s, ua); break;
    }
}

// the flow on its own (inrfit_flow_forward / _backward); in front of an ICNN: check_deformed
static int check_cdn(const InrFlowDesc* flow, const InrGridDesc* grid, int n_images, void* workspace, int64_t workspace_bytes,
                     CdnWs* w_out) {
    if (!flow_ok(flow)) return INR_EUNSUPPORTED;
    if (!workspace || !grid_ok(grid, n_images)) return INR_EINVAL;
    *w_out = carve_cdn(flow, grid, n_images, workspace);
    return workspace_bytes < w_out->bytes ? INR_EWORKSPACE : INR_OK;
}

}  // namespace

int64_t inrfit_flow_param_count(const InrFlowDesc* flow) {
    if (!flow_ok(flow)) return INR_EUNSUPPORTED;
    return make_flow_map(flow->width, flow->num_coupling).FP;
}

int64_t inrfit_cdn_workspace_bytes(const InrModelDesc* model, const InrFlowDesc* flow, const InrGridDesc* grid, int n_images) {
    if (!flow_ok(flow)) return INR_EUNSUPPORTED;
    if (!grid || grid->n_points <= 0 || n_images <= 0) return INR_EINVAL;
    const KernelEntry* e = model ? find_entry(model) : nullptr;
    const long long own = carve_cdn(flow, grid, n_images, nullptr).bytes;
    if (model && !e) {   // the layer-by-layer ICNN behind the flow
        if (!cdn_wide_shape(model)) return INR_EUNSUPPORTED;
        return own + carve_wide_behind(make_wide_map(model), grid->n_points, n_images, nullptr).bytes;
    }
    return own + (e ? align256(carve(e, grid->n_points, n_images, nullptr).bytes) : 0);
}

int inrfit_flow_forward(const InrFlowDesc* flow, const float* flow_params, const InrGridDesc* grid, int n_images,
                        float* out_coords, void* workspace, int64_t workspace_bytes, void* stream) {
    CdnWs w;
    if (!flow_params || !out_coords) return INR_EINVAL;
    int rc = check_cdn(flow, grid, n_images, workspace, workspace_bytes, &w);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    launch_flow_update(w, flow, n_images, 2, (float*)flow_params, nullptr, s);
    launch_flow_fwd(w, grid, n_images, out_coords, s);
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

int inrfit_flow_backward(const InrFlowDesc* flow, const float* flow_params, const InrGridDesc* grid, const float* dout_coords,
                         int n_images, float* flow_grads, void* workspace, int64_t workspace_bytes, void* stream) {
    CdnWs w;
    if (!flow_params || !dout_coords || !flow_grads) return INR_EINVAL;
    int rc = check_cdn(flow, grid, n_images, workspace, workspace_bytes, &w);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    launch_flow_update(w, flow, n_images, 2, (float*)flow_params, nullptr, s);
    if (hipMemcpyAsync(w.dxd, dout_coords, sizeof(float) * 2 * (size_t)grid->n_points * n_images, hipMemcpyDeviceToDevice, s) != hipSuccess)
        return INR_ELAUNCH;
    launch_flow_bwd(w, flow, grid, n_images, s);   // recomputes the forward from the grid, walks the couplings backwards
    launch_flow_update(w, flow, n_images, 1, (float*)flow_params, flow_grads, s);
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

// ---------------------------------------------------------------------------------------------------------------------
// path-connected prior with the normflows RealNVP deformation: ICNN(minmax^-1(RealNVP(minmax(a (.) x + b))))
// ---------------------------------------------------------------------------------------------------------------------
namespace {

struct PcnWs {
    float *xd, *dxd, *zs, *ps, *slab1, *slab2, *RE, *lossp;
    int blocksL;
    int blocks1, chunks, S1;      // blocks1 = blocks of the backward point kernel (rows of slab1)
    FlowShape sf, sb;             // launch shapes of the forward / backward point kernels (flow.h: flow_launch_shape)
    RnvpMap rm;
    long long bytes;
    InrGridDesc dgrid;
};

static bool rnvp_ok(const InrRnvpDesc* r) {
    if (!r || (r->channels != 2 && r->channels != 3)) return false;
    if (r->hidden_units < 1 || r->hidden_units > 256 || r->n_flows < 1 || r->n_flows > INR_RNVP_MAX_FLOWS) return false;
    if (r->output_fn != 0 && r->output_fn != 1) return false;
    for (int f = 0; f < r->n_flows; ++f)
        if (r->masks[f] < 1u || r->masks[f] > (1u << r->channels) - 2u) return false;   // at least one input and one output
    for (int c = 0; c < r->channels; ++c)
        if (!(r->vmax[c] > r->vmin[c])) return false;
    if (!(r->new_max > r->new_min)) return false;
    const int ldsf = RNVP_HDR + r->n_flows * (r->hidden_units * RNVP_REC + RNVP_TAIL);
    return (ldsf + 4 * (r->n_flows * 4 * r->channels + 2 * r->channels)) * 4 <= 160 * 1024;   // all flows' records live in LDS
}

static RnvpMap make_rnvp_map(const InrRnvpDesc* r) {
    RnvpMap m{};
    m.C = r->channels;
    m.HID = r->hidden_units;
    m.F = r->n_flows;
    m.net = 2 * m.HID * m.C + m.HID + m.C;
    m.pf = 2 * m.net + 2 * m.C;
    m.RP = 2 * m.C + m.F * m.pf;
    m.fl = m.HID * RNVP_REC + RNVP_TAIL;
    m.LDSF = RNVP_HDR + m.F * m.fl;
    m.HIDp = (m.HID + 63) / 64 * 64;
    m.A = 2 * (m.C - 1);
    m.out_fn = r->output_fn;
    m.out_scale = r->output_fn ? (r->output_scale != 0.f ? r->output_scale : 1.f) : 1.f;
    for (int c = 0; c < 3; ++c) {
        m.vmin[c] = c < m.C ? r->vmin[c] : 0.f;
        m.vmax[c] = c < m.C ? r->vmax[c] : 1.f;
    }
    m.nmin = r->new_min;
    m.nmax = r->new_max;
    for (int f = 0; f < RNVP_MAX_FLOWS; ++f) m.masks[f] = f < m.F ? r->masks[f] : 1u;
    return m;
}

static PcnWs carve_pcn(const InrRnvpDesc* r, const InrGridDesc* grid, int n_images, void* base) {
    PcnWs w;
    const long long N = grid->n_points;
    w.rm = make_rnvp_map(r);
    const int C = w.rm.C, F = w.rm.F;
    // The RealNVP point kernels (32 hidden units per flow: the per-flow scalar work, evaluated by every lane of a point, is as large as
    // the unit loop).  Small launches at C = 2: the FORWARD cuts the unit loop over 2 lanes (flow.h: U lanes per point; 16.8 -> 14.7 us at
    // 256x256, U = 4: 15.9); the backward stays at one lane per point (U = 2: 26.8 vs 26.3 us, U = 4: 30.5, and twice / four times the
    // partial-sum blocks for the update).  INR_RNVP_SHAPE = U forces both (measurement / test switch).
    {
        const char* fe = getenv("INR_RNVP_SHAPE");
        const bool small = C == 2 && N * n_images <= 98304;
        int uf = fe ? atoi(fe) : (small ? 2 : 1), ub = fe ? atoi(fe) : 1;
        if ((uf != 1 && uf != 2 && uf != 4) || C != 2) uf = 1;
        if ((ub != 1 && ub != 2 && ub != 4) || C != 2) ub = 1;
        w.sf = FlowShape{1, uf, 256, (int)((N * uf + 255) / 256)};
        w.sb = FlowShape{1, ub, 256, (int)((N * ub + 255) / 256)};
        // Large launches (several waves per SIMD anyway): Q = 2 points per lane - every record read serves two points, half the
        // LDS instructions and half the partial-sum blocks.  configs[3] (262 144 points, C = 3): forward Q = 1 51.7 | 2 44.2 | 4 48.5 us
        // (bit-identical), backward over points 89.8 | 82.0 us, the update behind it 24.7 -> 21.3 us.  (Round 2 had measured Q > 1
        // slower - on unit loops that hipcc had not unrolled, profiles/NOTES.md.)  C = 2, 16 images of 256x256 per launch: 2501 -> 2444 us
        // per step.  INR_RNVP_QF / _QB force a shape.
        const char* qf = getenv("INR_RNVP_QF");
        const char* qb = getenv("INR_RNVP_QB");
        const bool large = N * n_images >= 196608;
        int QF = qf ? atoi(qf) : 2, QB = qb ? atoi(qb) : 2;
        if (!large || (QF != 1 && QF != 2 && QF != 4)) QF = 1;
        if (!large || (QB != 1 && QB != 2)) QB = 1;
        if (QF > 1) w.sf = FlowShape{QF, 1, 256, (int)((N + 256 * QF - 1) / (256 * QF))};
        if (QB > 1) w.sb = FlowShape{QB, 1, 256, (int)((N + 256 * QB - 1) / (256 * QB))};
    }
    w.blocks1 = w.sb.blocks;
    w.chunks = 64;   // x F flows x 4 waves: enough waves for the 1024 SIMDs
    while (w.chunks > 1 && N / w.chunks < 1024) w.chunks /= 2;
    w.S1 = F * 4 * C + 2 * C;
    char* b = (char*)base;
    long long off = 0;
    auto take = [&](long long bytes) { float* p = (float*)(b + off); off += align256(bytes); return p; };
    w.xd = take((long long)n_images * C * N * 4);
    w.dxd = take((long long)n_images * C * N * 4);
    w.zs = take((long long)n_images * F * C * N * 4);
    w.ps = take((long long)n_images * F * w.rm.A * N * 4);
    w.slab1 = take((long long)n_images * w.blocks1 * w.S1 * 4);
    w.slab2 = take((long long)n_images * w.chunks * F * 2 * (2 * C + 1) * w.rm.HIDp * 4);
    w.RE = take((long long)n_images * w.rm.LDSF * 4);
    w.blocksL = (int)((N + 255) / 256);
    w.lossp = take((long long)n_images * w.blocksL * 4);
    w.dgrid = *grid;
    w.dgrid.mode = INR_GRID_EXPLICIT;
    w.dgrid.coords = w.xd;
    w.dgrid.coords_image_stride = (long long)C * N;
    w.bytes = off;
    return w;
}

// the point kernels keep every flow's records in LDS: allow more than the default 64 KB of dynamic LDS (once per process)
static int rnvp_set_lds() {
    static int rc = -1;
    if (rc >= 0) return rc;
    const int lim = 160 * 1024;
    bool ok = true;
    ok &= hipFuncSetAttribute((const void*)rnvp_fwd_kernel<2, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, lim) == hipSuccess;
    ok &= hipFuncSetAttribute((const void*)rnvp_fwd_kernel<3, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, lim) == hipSuccess;
    ok &= hipFuncSetAttribute((const void*)rnvp_fwd_kernel<3, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, lim) == hipSuccess;
    ok &= hipFuncSetAttribute((const void*)rnvp_fwd_kernel<3, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, lim) == hipSuccess;
    ok &= hipFuncSetAttribute((const void*)rnvp_fwd_kernel<2, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, lim) == hipSuccess;
    ok &= hipFuncSetAttribute((const void*)rnvp_fwd_kernel<2, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, lim) == hipSuccess;
    ok &= hipFuncSetAttribute((const void*)rnvp_bwd_points_kernel<3, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, lim) == hipSuccess;
    ok &= hipFuncSetAttribute((const void*)rnvp_bwd_points_kernel<2, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, lim) == hipSuccess;
    ok &= hipFuncSetAttribute((const void*)rnvp_bwd_points_kernel<2, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, lim) == hipSuccess;
    ok &= hipFuncSetAttribute((const void*)rnvp_bwd_points_kernel<3, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, lim) == hipSuccess;
    ok &= hipFuncSetAttribute((const void*)rnvp_fwd_kernel<2, 1, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, lim) == hipSuccess;
    ok &= hipFuncSetAttribute((const void*)rnvp_fwd_kernel<2, 1, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, lim) == hipSuccess;
    ok &= hipFuncSetAttribute((const void*)rnvp_bwd_points_kernel<2, 1, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, lim) == hipSuccess;
    ok &= hipFuncSetAttribute((const void*)rnvp_bwd_points_kernel<2, 1, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, lim) == hipSuccess;
    ok &= hipFuncSetAttribute((const void*)rnvp_bwd_points_kernel<2, 1, 1, RnvpBwdDinArgs>, hipFuncAttributeMaxDynamicSharedMemorySize, lim) == hipSuccess;
    ok &= hipFuncSetAttribute((const void*)rnvp_bwd_points_kernel<2, 2, 1, RnvpBwdDinArgs>, hipFuncAttributeMaxDynamicSharedMemorySize, lim) == hipSuccess;
    ok &= hipFuncSetAttribute((const void*)rnvp_bwd_points_kernel<3, 1, 1, RnvpBwdDinArgs>, hipFuncAttributeMaxDynamicSharedMemorySize, lim) == hipSuccess;
    ok &= hipFuncSetAttribute((const void*)rnvp_bwd_points_kernel<3, 2, 1, RnvpBwdDinArgs>, hipFuncAttributeMaxDynamicSharedMemorySize, lim) == hipSuccess;
    ok &= hipFuncSetAttribute((const void*)rnvp_inverse_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, lim) == hipSuccess;
    ok &= hipFuncSetAttribute((const void*)rnvp_inverse_kernel<3>, hipFuncAttributeMaxDynamicSharedMemorySize, lim) == hipSuccess;
    rc = ok ? INR_OK : INR_ENODEVICE;
    return rc;
}

// the RealNVP on its own (inrfit_rnvp_*); in front of an ICNN: check_deformed
static int check_pcn(const InrRnvpDesc* r, const InrGridDesc* grid, int n_images, void* workspace, int64_t workspace_bytes, PcnWs* w_out) {
    if (!rnvp_ok(r)) return INR_EUNSUPPORTED;
    if (!workspace || !grid_ok(grid, n_images)) return INR_EINVAL;
    if (grid->mode == INR_GRID_SEPARABLE && r->channels == 3 && !grid->ts) return INR_EINVAL;   // the separable grid's t axis
    *w_out = carve_pcn(r, grid, n_images, workspace);
    if (workspace_bytes < w_out->bytes) return INR_EWORKSPACE;
    return rnvp_set_lds();   // flow records of wide MLPs exceed the default 64 KB of dynamic LDS
}

// parameters -> packed image; once per parameter set, in front of the forward
static void launch_rnvp_pack(const PcnWs& w, const float* rp, int n_images, hipStream_t s, bool unit_linear = false) {
    RnvpPackArgs a{};
    a.RP = rp;
    a.RE = w.RE;
    a.m = w.rm;
    a.unit_linear = unit_linear ? 1 : 0;
    const dim3 g(w.rm.F, n_images);
    if (w.rm.C == 2) hipLaunchKernelGGL(rnvp_pack_kernel<2>, g, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(rnvp_pack_kernel<3>, g, dim3(256), 0, s, a);
}

void launch_rnvp_fwd(const PcnWs& w, const float* rp, const InrGridDesc* grid, int n_images, float* out, bool keep, hipStream_t s,
                     bool unit_linear = false, bool packed = false) {
    if (!packed) launch_rnvp_pack(w, rp, n_images, s, unit_linear);   // (in the fit loops the update kernel refreshes the image)
    RnvpFwdArgs a{};
    a.RE = w.RE;
    a.xd = out;
    a.zs = keep ? w.zs : nullptr;
    a.grid = *grid;
    a.N = grid->n_points;
    a.m = w.rm;
    const dim3 g(w.sf.blocks, n_images), b(w.sf.threads);
    const size_t lds = (size_t)(w.rm.LDSF + 64) * sizeof(float);   // + slack: the pipelined unit loop reads one batch ahead
    if (w.rm.C == 2) {
        if (w.sf.Q == 2) hipLaunchKernelGGL((rnvp_fwd_kernel<2, 2>), g, b, lds, s, a);
        else if (w.sf.Q == 4) hipLaunchKernelGGL((rnvp_fwd_kernel<2, 4>), g, b, lds, s, a);
        else if (w.sf.U == 2) hipLaunchKernelGGL((rnvp_fwd_kernel<2, 1, 2>), g, b, lds, s, a);
        else if (w.sf.U == 4) hipLaunchKernelGGL((rnvp_fwd_kernel<2, 1, 4>), g, b, lds, s, a);
        else hipLaunchKernelGGL((rnvp_fwd_kernel<2, 1>), g, b, lds, s, a);   // (Q > 1: measured slower, flow.h)
    } else {
        if (w.sf.Q == 2) hipLaunchKernelGGL((rnvp_fwd_kernel<3, 2>), g, b, lds, s, a);
        else if (w.sf.Q == 4) hipLaunchKernelGGL((rnvp_fwd_kernel<3, 4>), g, b, lds, s, a);
        else hipLaunchKernelGGL((rnvp_fwd_kernel<3, 1>), g, b, lds, s, a);
    }
}

// seed: the gradient at the deformed coordinates when it is not the ICNN's (w.dxd); din: also d / d input coordinates (both:
// inrfit_rnvp_backward, whose workspace has one lane per point in the backward walk - w.sb.U == 1)
static void launch_rnvp_bwd(const PcnWs& w, const float* rp, const InrGridDesc* grid, int n_images, hipStream_t s,
                            const float* seed = nullptr, float* din = nullptr) {
    RnvpBwdArgs a{};
    a.RE = w.RE;   // packed by the forward of this step
    a.dxd = seed ? seed : w.dxd;
    a.zs = w.zs;
    a.ps = w.ps;
    a.slab1 = w.slab1;
    a.grid = *grid;
    a.N = grid->n_points;
    a.m = w.rm;
    a.S1 = w.S1;
    const dim3 g1(w.sb.blocks, n_images), b1(w.sb.threads);
    const size_t lds = (size_t)(w.rm.LDSF + 4 * w.S1) * sizeof(float);
    if (din != nullptr) {
        RnvpBwdDinArgs da{};
        static_cast<RnvpBwdArgs&>(da) = a;
        da.din = din;
        if (w.rm.C == 2) {
            if (w.sb.Q == 2) hipLaunchKernelGGL((rnvp_bwd_points_kernel<2, 2, 1, RnvpBwdDinArgs>), g1, b1, lds, s, da);
            else hipLaunchKernelGGL((rnvp_bwd_points_kernel<2, 1, 1, RnvpBwdDinArgs>), g1, b1, lds, s, da);
        } else {
            if (w.sb.Q == 2) hipLaunchKernelGGL((rnvp_bwd_points_kernel<3, 2, 1, RnvpBwdDinArgs>), g1, b1, lds, s, da);
            else hipLaunchKernelGGL((rnvp_bwd_points_kernel<3, 1, 1, RnvpBwdDinArgs>), g1, b1, lds, s, da);
        }
    } else if (w.rm.C == 2) {
        if (w.sb.Q == 2) hipLaunchKernelGGL((rnvp_bwd_points_kernel<2, 2>), g1, b1, lds, s, a);
        else if (w.sb.U == 2) hipLaunchKernelGGL((rnvp_bwd_points_kernel<2, 1, 2>), g1, b1, lds, s, a);
        else if (w.sb.U == 4) hipLaunchKernelGGL((rnvp_bwd_points_kernel<2, 1, 4>), g1, b1, lds, s, a);
        else hipLaunchKernelGGL((rnvp_bwd_points_kernel<2, 1>), g1, b1, lds, s, a);
    } else {
        if (w.sb.Q == 2) hipLaunchKernelGGL((rnvp_bwd_points_kernel<3, 2>), g1, b1, lds, s, a);
        else hipLaunchKernelGGL((rnvp_bwd_points_kernel<3, 1>), g1, b1, lds, s, a);
    }
    RnvpUnitsArgs ua{};
    ua.RP = rp;
    ua.zs = w.zs;
    ua.ps = w.ps;
    ua.slab2 = w.slab2;
    ua.N = grid->n_points;
    ua.m = w.rm;
    ua.chunks = w.chunks;
    // hidden units in blocks of 32 (8 per wave) - or 64 (16 per wave) when that needs no second block
    // (16 units per wave at HID = 32 - two waves per block, the per-point loads amortised over twice the units - was measured slower:
    // 114 vs 62.7 us at configs[3] (267 registers: one wave per SIMD), 14.4 vs 12.5 us at 256x256)
    const int upw = (w.rm.HID > 32 && w.rm.HID <= 64) ? 16 : 8;
    const dim3 g2(w.chunks, w.rm.F * ((w.rm.HID + 4 * upw - 1) / (4 * upw)), n_images);
    const size_t lds2 = (size_t)(RNVP_HDR + w.rm.fl) * sizeof(float);
    // waves that own units: a block of 4 waves covers 4 upw units; with fewer units than that the idle waves are not launched
    const int waves = (w.rm.HID + upw - 1) / upw < 4 ? (w.rm.HID + upw - 1) / upw : 4;
    const dim3 b2(64 * waves);
    if (w.rm.C == 2) {
        if (upw == 8) hipLaunchKernelGGL((rnvp_bwd_units_kernel<2, 8>), g2, b2, lds2, s, ua);
        else hipLaunchKernelGGL((rnvp_bwd_units_kernel<2, 16>), g2, b2, lds2, s, ua);
    } else {
        if (upw == 8) hipLaunchKernelGGL((rnvp_bwd_units_kernel<3, 8>), g2, b2, lds2, s, ua);
        else hipLaunchKernelGGL((rnvp_bwd_units_kernel<3, 16>), g2, b2, lds2, s, ua);
    }
}

RnvpUpdArgs make_rnvp_upd_args(const PcnWs& w, int n_images, int mode, float* rp, float* opt, float* grads_out, const InrOptDesc* od,
                               float wd_flow, int t, const float* lr_hdr, long long hdr_stride, const int32_t* status) {
    RnvpUpdArgs u{};
    u.RP = rp;
    u.opt = opt;
    u.grads_out = grads_out;
    u.slab1 = w.slab1;
    u.slab2 = w.slab2;
    u.lr_hdr = lr_hdr;
    u.hdr_stride = hdr_stride;
    u.status = status;
    if (od) u.opt_desc = *od;
    u.m = w.rm;
    u.blocks1 = w.blocks1;
    u.S1 = w.S1;
    u.chunks = w.chunks;
    u.t = t;
    u.c = opt_consts(od, t);
    u.wd_flow = wd_flow;
    u.mode = mode;
    return u;
}

// the ICNN update `ui` and the RealNVP's optimizer step in one launch (pcn_update_kernel)
static void launch_pcn_update(const KernelEntry* e, const PcnWs& w, const UpdArgs& ui, RnvpUpdArgs ur, int n_images, hipStream_t s) {
    const int nbf = w.rm.F + 1;
    const dim3 gi = upd_grid(e->img.sl_cols, n_images, nbf), g(gi.x + nbf, n_images), b = upd_block(e->img.sl_cols, nbf);
    ur.status = nullptr;
    ur.loss_part = ui.loss_part;
    ur.loss_wgs = ui.wgs;
    ur.loss_stride = ui.loss_stride;
    const int n_wide = upd_split(e->img.sl_cols, nbf).n_wide;
    if (w.rm.C == 2) hipLaunchKernelGGL(pcn_update_kernel<2>, g, b, 0, s, ui, ur, (int)gi.x, n_wide);
    else hipLaunchKernelGGL(pcn_update_kernel<3>, g, b, 0, s, ui, ur, (int)gi.x, n_wide);
}

static void launch_rnvp_update_args(const PcnWs& w, int n_images, const RnvpUpdArgs& u, hipStream_t s) {
    const dim3 g(w.rm.F + 1, n_images);
    if (w.rm.C == 2) hipLaunchKernelGGL(rnvp_update_kernel<2>, g, dim3(256), 0, s, u);
    else hipLaunchKernelGGL(rnvp_update_kernel<3>, g, dim3(256), 0, s, u);
}

// mode 1: gradients only
void launch_rnvp_grads(const PcnWs& w, int n_images, float* rp, float* grads_out, hipStream_t s) {
    launch_rnvp_update_args(w, n_images, make_rnvp_upd_args(w, n_images, 1, rp, nullptr, grads_out, nullptr, 0.f, 0, nullptr, 0, nullptr), s);
}

}  // namespace

int64_t inrfit_rnvp_param_count(const InrRnvpDesc* rnvp) {
    if (!rnvp_ok(rnvp)) return INR_EUNSUPPORTED;
    return make_rnvp_map(rnvp).RP;
}

int64_t inrfit_pcn_workspace_bytes(const InrModelDesc* model, const InrRnvpDesc* rnvp, const InrGridDesc* grid, int n_images) {
    if (!rnvp_ok(rnvp)) return INR_EUNSUPPORTED;
    if (!grid || grid->n_points <= 0 || n_images <= 0) return INR_EINVAL;
    const KernelEntry* e = model ? find_entry(model) : nullptr;
    const long long own = carve_pcn(rnvp, grid, n_images, nullptr).bytes;
    if (model && !e) {   // the layer-by-layer ICNN behind the RealNVP
        if (!pcn_wide_shape(model)) return INR_EUNSUPPORTED;
        return own + carve_wide_behind(make_wide_map(model), grid->n_points, n_images, nullptr).bytes;
    }
    return own + (e ? align256(carve(e, grid->n_points, n_images, nullptr).bytes) : 0);
}

int inrfit_rnvp_actnorm_init(const InrRnvpDesc* rnvp, float* flow_params, const InrGridDesc* grid, int n_images, void* workspace,
                             int64_t workspace_bytes, void* stream) {
    PcnWs w;
    if (!flow_params) return INR_EINVAL;
    int rc = check_pcn(rnvp, grid, n_images, workspace, workspace_bytes, &w);
    if (rc) return rc;
    RnvpInitArgs a{};
    a.RP = flow_params;
    a.z = w.xd;
    a.grid = *grid;
    a.N = grid->n_points;
    a.m = w.rm;
    const size_t lds = (size_t)(RNVP_HDR + w.rm.fl + 64) * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    const long long N = grid->n_points;
    if (N >= 16384) {
        // large grids: 2 F + 1 launches over all points instead of one block per image (13 ms at 128x128x16, F = 18)
        RnvpInitParArgs pa{};
        pa.b = a;
        pa.nb = (int)((N + 1023) / 1024);
        if (pa.nb > 256) pa.nb = 256;
        pa.part = (double*)w.dxd;   // [n_images][2][nb][C] doubles: 48 KB at most per image, dxd has C N floats
        const dim3 g((unsigned)pa.nb, (unsigned)n_images);
        for (int f = 0; f <= w.rm.F; ++f) {
            pa.f = f;
            if (w.rm.C == 2) hipLaunchKernelGGL(rnvp_init_couple_kernel<2>, g, dim3(256), lds, s, pa);
            else hipLaunchKernelGGL(rnvp_init_couple_kernel<3>, g, dim3(256), lds, s, pa);
            if (f < w.rm.F) {
                if (w.rm.C == 2) hipLaunchKernelGGL(rnvp_init_var_kernel<2>, g, dim3(256), 0, s, pa);
                else hipLaunchKernelGGL(rnvp_init_var_kernel<3>, g, dim3(256), 0, s, pa);
            }
        }
        return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
    }
    if (w.rm.C == 2) hipLaunchKernelGGL(rnvp_actnorm_init_kernel<2>, dim3(n_images), dim3(1024), lds, s, a);
    else hipLaunchKernelGGL(rnvp_actnorm_init_kernel<3>, dim3(n_images), dim3(1024), lds, s, a);
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

int inrfit_rnvp_forward(const InrRnvpDesc* rnvp, const float* flow_params, const InrGridDesc* grid, int n_images,
                        float* out_coords, void* workspace, int64_t workspace_bytes, void* stream) {
    PcnWs w;
    if (!flow_params || !out_coords) return INR_EINVAL;
    int rc = check_pcn(rnvp, grid, n_images, workspace, workspace_bytes, &w);
    if (rc) return rc;
    launch_rnvp_fwd(w, flow_params, grid, n_images, out_coords, false, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

int inrfit_rnvp_backward(const InrRnvpDesc* rnvp, const float* flow_params, const InrGridDesc* grid, const float* dout_coords,
                         int n_images, float* flow_grads, float* din_coords, void* workspace, int64_t workspace_bytes, void* stream) {
    PcnWs w;
    if (!flow_params || !dout_coords || !flow_grads) return INR_EINVAL;
    int rc = check_pcn(rnvp, grid, n_images, workspace, workspace_bytes, &w);
    if (rc) return rc;
    if (w.sb.U != 1) {   // (a forced U-lanes-per-point shape: the seeded walk runs one lane per point; fewer slab rows than carved)
        w.sb = FlowShape{1, 1, 256, (int)((grid->n_points + 255) / 256)};
        w.blocks1 = w.sb.blocks;
    }
    hipStream_t s = (hipStream_t)stream;
    launch_rnvp_fwd(w, flow_params, grid, n_images, w.xd, true, s);   // the forward is recomputed: the state in front of every flow
    launch_rnvp_bwd(w, flow_params, grid, n_images, s, dout_coords, din_coords);
    launch_rnvp_grads(w, n_images, const_cast<float*>(flow_params), flow_grads, s);
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

int inrfit_rnvp_inverse(const InrRnvpDesc* rnvp, const float* flow_params, const float* in_coords, int64_t in_image_stride,
                        int64_t n_points, int n_images, float* out_coords, void* workspace, int64_t workspace_bytes, void* stream) {
    PcnWs w;
    if (!flow_params || !in_coords || !out_coords || n_points <= 0) return INR_EINVAL;
    InrGridDesc g{};
    g.mode = INR_GRID_EXPLICIT;
    g.n_points = n_points;
    g.coords = in_coords;
    g.coords_image_stride = in_image_stride;
    int rc = check_pcn(rnvp, &g, n_images, workspace, workspace_bytes, &w);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    launch_rnvp_pack(w, flow_params, n_images, s);
    RnvpInvArgs a{};
    a.RE = w.RE;
    a.in = in_coords;
    a.out = out_coords;
    a.N = n_points;
    a.in_image_stride = in_image_stride;
    a.m = w.rm;
    const dim3 gr((unsigned)((n_points + 255) / 256), n_images);
    const size_t lds = (size_t)(w.rm.LDSF + 64) * sizeof(float);   // + slack: the pipelined unit loop reads one batch ahead
    if (w.rm.C == 2) hipLaunchKernelGGL(rnvp_inverse_kernel<2>, gr, dim3(256), lds, s, a);
    else hipLaunchKernelGGL(rnvp_inverse_kernel<3>, gr, dim3(256), lds, s, a);
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

int inrfit_rnvp_fit_identity(const InrRnvpDesc* rnvp, float* flow_params, float* flow_opt_state, const InrGridDesc* grid,
                             const InrOptDesc* opt, int n_images, int steps, int step0, float* loss_hist, void* workspace,
                             int64_t workspace_bytes, void* stream) {
    PcnWs w;
    if (!flow_params || !flow_opt_state || !opt || steps < 0 || step0 < 0) return INR_EINVAL;
    if (opt->kind != INR_OPT_ADAM && opt->kind != INR_OPT_ADAMAX) return INR_EINVAL;
    int rc = check_pcn(rnvp, grid, n_images, workspace, workspace_bytes, &w);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int C = w.rm.C;
    RnvpIdArgs ia{};
    ia.xd = w.xd;
    ia.dxd = w.dxd;
    ia.lossp = w.lossp;
    ia.grid = *grid;
    ia.N = grid->n_points;
    const dim3 gl(w.blocksL, n_images);
    for (int it = 0; it < steps; ++it) {
        launch_rnvp_fwd(w, flow_params, grid, n_images, w.xd, true, s, true, it > 0);
        if (C == 2) hipLaunchKernelGGL(rnvp_identity_loss_kernel<2>, gl, dim3(256), 0, s, ia);
        else hipLaunchKernelGGL(rnvp_identity_loss_kernel<3>, gl, dim3(256), 0, s, ia);
        launch_rnvp_bwd(w, flow_params, grid, n_images, s);
        RnvpUpdArgs u = make_rnvp_upd_args(w, n_images, 0, flow_params, flow_opt_state, nullptr, opt, opt->weight_decay,
                                           step0 + it + 1, nullptr, 0, nullptr);
        u.skip_linear = 1;
        u.RE = w.RE;
        u.unit_linear = 1;
        u.lossp = w.lossp;
        u.lossp_blocks = w.blocksL;
        u.loss_scale = 1.f / ((float)C * (float)grid->n_points);
        u.loss_hist = loss_hist;
        u.hist_idx = it;
        u.hist_stride = steps;
        launch_rnvp_update_args(w, n_images, u, s);
    }
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

int64_t inrfit_joint_loss_workspace_bytes(int64_t n_elems) {
    if (n_elems <= 0) return INR_EINVAL;
    return (int64_t)(JL_MAX_BLOCKS * JL_PART + JL_RES + 8) * 4;
}

namespace {

static int check_joint_desc(const InrJointLossDesc* d) {
    if (!d) return INR_EINVAL;
    if (d->kind != INR_LOSS_SE && d->kind != INR_LOSS_BCE) return INR_EINVAL;
    if (d->weight_mode < INR_WEIGHT_NONE || d->weight_mode > INR_WEIGHT_SSSDMS) return INR_EINVAL;
    if (d->form < INR_JOINT_FBMS || d->form > INR_JOINT_AWESOME_PIXEL) return INR_EINVAL;
    if (d->target_rule != 0 && d->target_rule != 1) return INR_EINVAL;
    if (d->form == INR_JOINT_AWESOME_IMAGE) {
        if (d->prior_kind != INR_LOSS_SE && d->prior_kind != INR_LOSS_BCE) return INR_EINVAL;
        if (d->prior_weight_mode < INR_WEIGHT_NONE || d->prior_weight_mode > INR_WEIGHT_SSSDMS) return INR_EINVAL;
    }
    return INR_OK;
}

// kernel arguments of the composite loss for `batch` items of `n` pixels (see joint_loss.h for the three layouts)
int make_joint_args(const float* output, const float* target, int batch, long long n, const InrJointLossDesc* desc, float* doutput,
                    void* workspace, JointLossArgs* out) {
    JointLossArgs a{};
    a.output = output;
    a.target = target;
    a.doutput = doutput;
    a.part = (float*)workspace;
    a.res = a.part + JL_MAX_BLOCKS * JL_PART;
    a.n = n;
    a.batch = batch;
    a.total = (long long)batch * n;
    a.d = *desc;
    if (desc->form == INR_JOINT_AWESOME_PIXEL) {
        a.es = 2; a.cs = 1; a.bs = 2 * n;
        a.n_data = desc->n_scribble > 0 ? desc->n_scribble : n;
        if (a.n_data > n) return INR_EINVAL;
        a.pen_lo = n - a.n_data;                       // awesome_loss.py:58-59 slices [random:], random = n - n_scribble
        a.pen_on = desc->extra_penalty && a.n_data < n;
        a.d.prior_kind = desc->kind;                   // one criterion for both terms
        a.d.prior_weight_mode = desc->weight_mode;
        a.d.prior_ratio = desc->ratio;
    } else {
        a.es = 1; a.cs = n; a.bs = 2 * n;
        a.n_data = n;
        a.pen_lo = 0;
        a.pen_on = desc->form == INR_JOINT_FBMS ? 1 : (desc->extra_penalty ? 1 : 0);
    }
    const long long want = (a.total + 1023) / 1024;   // >= 4 pixels per thread
    a.blocks = (int)(want < 1 ? 1 : (want > JL_MAX_BLOCKS ? JL_MAX_BLOCKS : want));
    *out = a;
    return INR_OK;
}

}  // namespace

int inrfit_joint_loss(const float* output, const float* target, int batch, int64_t hw, const InrJointLossDesc* desc,
                      float* loss_out, float* doutput, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!output || !target || !loss_out || !workspace || batch <= 0 || hw <= 0) return INR_EINVAL;
    int rc = check_joint_desc(desc);
    if (rc) return rc;
    if (workspace_bytes < inrfit_joint_loss_workspace_bytes((int64_t)batch * hw)) return INR_EWORKSPACE;
    JointLossArgs a;
    if ((rc = make_joint_args(output, target, batch, hw, desc, doutput, workspace, &a))) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(joint_loss_partial_kernel<true>, dim3(a.blocks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(joint_loss_finish_kernel, dim3(1), dim3(256), 0, s, a);
    if (doutput) hipLaunchKernelGGL(joint_loss_grad_kernel<false>, dim3(a.blocks), dim3(256), 0, s, a, (const float*)nullptr, (float*)nullptr);
    if (hipMemcpyAsync(loss_out, a.res, 4 * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) return INR_ELAUNCH;
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

// ---------------------------------------------------------------------------------------------------------------------
// fused joint step (one image): composite loss + prior forward/backward + optimizer, no host round trip
// ---------------------------------------------------------------------------------------------------------------------
namespace {

// one thread: this step's learning rate into the ICNN header's double buffer (the update kernels read hdr[t & 1]), the
// "frozen" flags cleared (every joint step stands alone), and the data-term coefficients of the prior's step kernel:
// FBMS: the penalty beta mean((prior - seg)^2) as the SE term against the soft target `seg` with the UNCLIPPED, unscaled
// coefficient 1/n (joint_step_finish_kernel turns the kernel's own loss column into the clip factor);
// AWESOME_IMAGE: left to loss_coef_kernel (class weights of the prior criterion from the targets; x gamma alpha with the extra
// penalty on, where the step kernel's align mode adds the second data term).
__global__ void joint_prep_kernel(float* hdr, float lr, int t, float* coef, float c, int write_coef) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        hdr[opt_hdr_lr_of(t)] = lr;
        hdr[OPT_HDR_LR] = lr;
        opt_hdr_clear_frozen(hdr);
        if (write_coef) coef[0] = coef[1] = c;
    }
}

struct JointFinArgs {
    JointLossArgs jl;       // part = the segmentation-side partial sums (joint_loss_partial_kernel<false>)
    const float* slabs;     // the step kernel's gradient slabs of this step [wgs][PS]
    int wgs, PS, loss_col;
    float* gscale;          // [1] -> the update kernels
    float* loss_out;        // [4] or null
};

__global__ __launch_bounds__(256) void joint_step_finish_kernel(const JointFinArgs f) {
    __shared__ float sm[4];
    const JointLossArgs& a = f.jl;
    constexpr int SLOT[5] = {0, 1, 2, 6, 7};   // seg loss over fg / the rest, fg count, valid pixels, bg count
    float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int b = threadIdx.x; b < a.blocks; b += 256)
#pragma unroll
        for (int k = 0; k < 5; ++k) v[k] += a.part[JL_PART * b + SLOT[k]];
    float tot[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 5; ++k) tot[SLOT[k]] = jl_block_sum(v[k], sm);
    // the prior's share, as the step kernel summed it: FBMS mean((prior - seg)^2); AWESOME_IMAGE mean(w' pcrit), with the extra
    // penalty on gamma alpha mean(w' pcrit) + beta mean((prior - [seg > 0.5])^2) (the align mode)
    float lc = 0.f;
    for (int w = threadIdx.x; w < f.wgs; w += 256) lc += f.slabs[(size_t)w * f.PS + f.loss_col];
    const float prior_term = jl_block_sum(lc, sm);
    const bool align = a.d.form == INR_JOINT_AWESOME_IMAGE && a.pen_on;
    float pen_sum = 0.f;   // the align term alone (joint_align_partial_kernel), for loss_out[2]
    if (align) {
        float v3 = 0.f;
        for (int b = threadIdx.x; b < a.blocks; b += 256) v3 += a.part[JL_PART * b + 3];
        pen_sum = jl_block_sum(v3, sm);
    }
    if (threadIdx.x != 0) return;
    float gs;
    if (a.d.form == INR_JOINT_FBMS) {
        jl_finish(a, tot, prior_term * (float)a.total);     // jl_finish divides the penalty sum by n again
        gs = a.res[3] * a.d.beta;                           // d penalty / d theta = clip * beta * d mean((p - s)^2) / d theta
    } else if (align) {
        const float nd = tot[6], nfg = tot[2], g = a.d.gamma;
        const float w = jl_class_weight(a.d.weight_mode, a.d.ratio, nfg, tot[7]);
        const float seg_raw = (w * tot[0] + tot[1]) / nd;
        a.res[0] = g * seg_raw + prior_term;
        a.res[1] = seg_raw;
        a.res[2] = pen_sum / (float)a.total;
        a.res[3] = 1.f;
        a.res[4] = g * w / nd;
        a.res[5] = g / nd;
        a.res[6] = 0.f;                                     // the indicator carries no gradient to seg
        a.res[7] = nfg;
        gs = 1.f;                                           // gamma alpha and beta sit in the step kernel's coefficients
    } else {
        const float nd = tot[6], nfg = tot[2];
        const float w = jl_class_weight(a.d.weight_mode, a.d.ratio, nfg, tot[7]);
        const float seg_raw = (w * tot[0] + tot[1]) / nd;
        a.res[0] = seg_raw + a.d.alpha * prior_term;
        a.res[1] = seg_raw;
        a.res[2] = 0.f;
        a.res[3] = 1.f;
        a.res[4] = w / nd;
        a.res[5] = 1.f / nd;
        a.res[6] = 0.f;
        a.res[7] = nfg;
        gs = a.d.alpha;
    }
    // a non-finite COMPOSITE loss freezes the row: the update kernels read a non-finite gradient scale as "no step" (a NaN in
    // `seg` does not reach the prior's own loss column in the AWESOME_IMAGE form; it reaches res[0] through seg_raw)
    f.gscale[0] = isfinite(a.res[0]) ? gs : __builtin_nanf("");
    if (f.loss_out) {
#pragma unroll
        for (int k = 0; k < 4; ++k) f.loss_out[k] = a.res[k];
    }
}

// what the three joint-step entry points share, before and after the prior's own kernels
struct JointCtx {
    JointLossArgs jl;
    float* gscale;
    float* logits;
    InrLossDesc prior_loss;   // the data term the prior's step kernel evaluates
    const float* prior_targets;
    DataTerm term;            // AWESOME_IMAGE with the extra penalty: the pass's align mode (seg, beta / n, hard, every point), else none
};

// the loss, optimizer and step arguments of a joint step
int check_joint_step(const InrJointLossDesc* desc, const InrOptDesc* opt, int step) {
    if (const int rc = check_joint_desc(desc)) return rc;
    if (!opt || (opt->kind != INR_OPT_ADAM && opt->kind != INR_OPT_ADAMAX) || step < 1) return INR_EINVAL;
    if (desc->form == INR_JOINT_AWESOME_PIXEL) return INR_EUNSUPPORTED;            // pixel mode has no dense-grid prior pass
    // the AWESOME_IMAGE prior term runs inside the step kernel, which reads unaries (fg < 0.5) and has no pixel mask
    if (desc->form == INR_JOINT_AWESOME_IMAGE && (desc->target_rule != 0 || desc->use_noneclass)) return INR_EUNSUPPORTED;
    return INR_OK;
}

int joint_begin(const InrJointLossDesc* desc, const InrOptDesc* opt, const float* seg, const float* target, long long N, int step,
                float* prior_logits, float* jws, float* icnn_hdr, float* coef, hipStream_t s, JointCtx* c) {
    int rc = check_joint_step(desc, opt, step);
    if (rc) return rc;
    // seg-side sums over the single image: output = seg (channel stride unused), PRIOR = false
    if ((rc = make_joint_args(seg, target, 1, N, desc, nullptr, jws, &c->jl))) return rc;
    c->gscale = c->jl.res + JL_RES;
    c->logits = prior_logits;
    c->term = DataTerm{};
    hipLaunchKernelGGL(joint_loss_partial_kernel<false>, dim3(c->jl.blocks), dim3(256), 0, s, c->jl);
    const bool fbms = desc->form == INR_JOINT_FBMS;
    hipLaunchKernelGGL(joint_prep_kernel, dim3(1), dim3(64), 0, s, icnn_hdr, opt->lr, step, coef, 1.f / (float)N, fbms ? 1 : 0);
    if (fbms) {
        c->prior_loss = InrLossDesc{INR_LOSS_SE, INR_WEIGHT_EXPLICIT, 1.f, 1.f / (float)N, 1.f / (float)N};
        c->prior_targets = seg;
    } else {
        c->prior_loss = InrLossDesc{desc->prior_kind, desc->prior_weight_mode, desc->prior_ratio, 0.f, 0.f};
        c->prior_targets = target;
        float scale = 1.f;
        if (c->jl.pen_on) {   // loss = gamma (crit(seg) + alpha pcrit(prior)) + beta align: both prior terms in the step kernel
            scale = desc->gamma * desc->alpha;
            c->term.align_seg = seg;
            c->term.c_align = desc->beta / (float)N;
        }
        hipLaunchKernelGGL(loss_coef_kernel, dim3(1), dim3(256), 0, s, target, N, c->prior_loss, coef, scale);
    }
    return INR_OK;
}

// where a training pass left the prior's loss: column `col` of `wgs` rows of PS floats - the step kernel's gradient slabs, or the
// layer-by-layer path's one-slab gradient vector (wgs = 1, col = P)
struct LossColumn {
    const float* slabs;
    int wgs, PS, col;
};

static void joint_finish(const JointCtx& c, const LossColumn& lc, float* loss_out, hipStream_t s) {
    JointFinArgs f{};
    f.jl = c.jl;
    f.slabs = lc.slabs;
    f.wgs = lc.wgs;
    f.PS = lc.PS;
    f.loss_col = lc.col;
    f.gscale = c.gscale;
    f.loss_out = loss_out;
    if (c.term.align_seg) hipLaunchKernelGGL(joint_align_partial_kernel, dim3(c.jl.blocks), dim3(256), 0, s, c.jl, (const float*)c.logits);
    hipLaunchKernelGGL(joint_step_finish_kernel, dim3(1), dim3(256), 0, s, f);
}

static void joint_dseg(const JointCtx& c, float* dseg, hipStream_t s) {
    hipLaunchKernelGGL(joint_loss_grad_kernel<true>, dim3(c.jl.blocks), dim3(256), 0, s, c.jl, (const float*)c.logits, dseg);
}

long long joint_ws_bytes(long long N) { return align256(inrfit_joint_loss_workspace_bytes(N)) + align256(N * 4); }

}  // namespace

int64_t inrfit_joint_step_workspace_bytes(const InrModelDesc* model, const InrGridDesc* grid) {
    const int64_t b = inrfit_workspace_bytes(model, grid, 1);
    if (b < 0) return b;
    return align256(b) + joint_ws_bytes(grid->n_points);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// the host driver: one skeleton per operation (forward, loss + gradients, fit, fused joint step, joint prior step) over two policies
// ---------------------------------------------------------------------------------------------------------------------
// A BACKBONE B is the ICNN on a grid.  FusedIcnn runs the hand-written step kernel (KernelEntry + Workspace): one launch covers
// every image.  WideIcnn runs the layer-by-layer path (WideMap + WideWs): one image at a time through one gradient buffer.  Both give
//   fused, max_points             whether one launch covers all images; the most points a grid may have
//   check(...)                    on the caller's grid: shape, arguments and workspace carve (icnn_form: ICNN-form shapes only)
//   find(model, icnn_form), carve_behind(model, dgrid, n, base)
//                                 behind a deformation (check_deformed): the shape alone, then the carve at `base` on the deformed grid
//   loss_ok(loss), device()       the shape's own loss rule; the device's turn (set_lds) once every argument has passed
//   bytes, P(), coef(), tstride() workspace bytes, parameters per image, loss coefficients, target / logit floats per image
//   pack(params, s), infer(params, logits, s)
//                                 parameters into the step kernel's image (nothing layer by layer); the inference pass -> logits
//   begin_updates(...), set_step(buf, opt, t, hist_idx), u, hdr(), opt_stride(), status()
//                                 the optimizer step's arguments of this call and of step t; image 0's header, the stride to the next
//   units()                       gradient buffers walked in turn: 1 (fused), n_images (layer by layer)
//   train(k, params, pass, s)     the training pass of unit k -> gradients and loss in the unit's buffer (loss_column())
//   grads_out(k, grads, loss, s)  ... out to the caller
//   update(k, s)                  ... into the optimizer step.  Layer by layer it sits inside the unit loop: the buffer is one image's.
// A DEFORMATION F is what runs in front of the backbone: NoDeform, FlowDeform (the coupling flow) or RnvpDeform.  It gives
//   none, dxd, bytes              whether it is NoDeform; where the pass writes dL/dcoords (null: none); bytes of the whole workspace
//   check(b, ...), device()       every argument check and both carves (check_deformed); its set_lds
//   begin(s)                      once per call, in front of the first forward
//   forward(train, packed, s)     the coordinates the backbone sees (train: keep what the backward reads)
//   gradients(s)                  loss_grad: its backward and its gradients (mode 1)
//   update(b, fit, s)             its backward seeded from dxd and its optimizer step, which reads this step's learning rate and the
//                                 frozen flag from the ICNN headers and b.u's status and gscale.  Over the fused backbone it owns the
//                                 ICNN's update too (the skeletons skip b.update): where upd_union_ok allows, the backward and one
//                                 combined launch, else icnn_update_kernel, the backward, its own update.
namespace {

// dL/dlogit of the data term from the logits wide_out_kernel wrote (wide_data_term, the expressions of its own dy, which it keeps in
// registers): what wide_dx_kernel starts dL/dcoords from (s_o dL/dlogit).  JOINT: the data term of a joint step.
template <bool JOINT>
__global__ __launch_bounds__(256) void pcn_wide_dy_kernel(const float* __restrict__ logit, const float* __restrict__ target,
                                                          const float* __restrict__ coef, int loss_kind, long long N,
                                                          float* __restrict__ dy, const WideJoint jn) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    float l = 0.f, d = 0.f;
    wide_data_term<JOINT>(target, coef, loss_kind, jn, p, logit[p], l, d);
    dy[p] = d;
}

// one training pass, as a skeleton asks a backbone for it
struct TrainPass {
    const float* targets;             // [n_images][tstride]; INR_LOSS_EXTERNAL: dL/dlogits
    int loss_kind;
    float* logits = nullptr;          // [n_images][tstride]: the pass leaves its logits here as well, or null
    float* dxd = nullptr;             // [n_images][C][N]: dL/dcoords as well, or null
    const DataTerm* term = nullptr;   // a joint step's data term, or null
    int freeze_input = 0;             // the fit's opt->freeze_input: a general shape then skips dZ_0
};

struct FusedIcnn {
    static constexpr bool fused = true;
    static constexpr long long max_points = 0x7fffffffLL;
    const KernelEntry* e = nullptr;
    Workspace w;
    InrGridDesc grid;   // the grid the step kernel reads: the caller's, or the deformation's
    int n_images = 0;
    long long bytes = 0;
    bool timed = false;   // bench.py's timing hooks (inrfit_timing_*) bracket the launches: the plain fit only
    UpdArgs u;

    int check(const InrModelDesc* model, const InrGridDesc* g, int n, void* ws, int64_t ws_bytes, bool) {
        if (const int rc = prepare_args(model, g, n, ws, ws_bytes, &e, &w)) return rc;
        grid = *g;
        n_images = n;
        bytes = w.bytes;
        return INR_OK;
    }
    bool find(const InrModelDesc* model, bool) { return (e = find_entry(model)) != nullptr; }
    long long carve_behind(const InrModelDesc* model, const InrGridDesc& dgrid, int n, void* base) {
        w = carve(e, dgrid.n_points, n, base);
        w.set_user(e, model);
        grid = dgrid;
        n_images = n;
        return align256(w.bytes);
    }
    int loss_ok(const InrLossDesc*) const { return INR_OK; }
    int device() { return set_lds(e); }
    int P() const { return w.Pu; }
    float* coef() const { return w.coef; }
    long long tstride() const { return grid.n_points; }
    bool coef_for(int) const { return true; }
    int units() const { return 1; }
    int pack(const float* params, hipStream_t s) { return launch_pack(e, w, params, n_images, s); }
    int infer(const float*, float* logits, hipStream_t s) { return launch_step(e, w, false, &grid, nullptr, 0, n_images, logits, s); }
    void begin_updates(float* params, float* opt_state, float* loss_hist, int32_t* status, const InrOptDesc* opt, int steps) {
        u = make_upd_args(e, w, params, opt_state, loss_hist, status, opt, n_images, steps);
    }
    void set_step(int buf, const InrOptDesc* opt, int t, int hist_idx) {
        w.set_step(buf);
        u.slabs = w.slabs;
        u.loss_part = w.loss_part;
        set_step_consts(u, opt, t, hist_idx);
    }
    float* hdr() const { return u.opt_state + 2 * (size_t)u.Pu; }
    long long opt_stride() const { return 2 * (long long)u.Pu + INR_OPT_HEADER_FLOATS; }
    int32_t* status() const { return u.status; }
    int train(int, const float*, const TrainPass& a, hipStream_t s) {
        if (timed) return launch_step_timed(e, w, &grid, a.targets, a.loss_kind, n_images, s, a.logits);
        return launch_step(e, w, true, &grid, a.targets, a.loss_kind, n_images, a.logits, s, a.dxd, a.term ? *a.term : DataTerm{});
    }
    LossColumn loss_column() const { return LossColumn{w.slabs, w.wgs, w.PS, e->img.sl_cols - 1}; }
    int grads_out(int, float* grads, float* loss_out, hipStream_t s) {
        launch_reduce(e, w, n_images, grads, loss_out, s);
        return INR_OK;
    }
    int update(int, hipStream_t s) {
        if (timed) return launch_icnn_update_timed(e, u, s);
        launch_icnn_update(e, u, s);
        return INR_OK;
    }
};

struct WideIcnn {
    static constexpr bool fused = false;
    static constexpr long long max_points = 0x7fffffffLL / WIDE_MAX_HIDDEN * 64;
    const InrModelDesc* model = nullptr;
    WideMap m;
    WideWs w;
    float *coef_all = nullptr, *logit = nullptr, *dy = nullptr;   // logit, dy [N]: behind a deformation only
    InrGridDesc grid;
    int n_images = 0;
    long long bytes = 0;
    UpdArgs u;   // the one-slab view of w.grads; its per-image pointers are update's, from:
    float *params0 = nullptr, *opt0 = nullptr, *hist0 = nullptr;
    int32_t* status0 = nullptr;

    bool find(const InrModelDesc* md, bool icnn_form) {
        model = md;
        return icnn_form ? pcn_wide_shape(md) : use_wide(md);
    }
    int check(const InrModelDesc* md, const InrGridDesc* g, int n, void* ws, int64_t ws_bytes, bool icnn_form) {
        if (!find(md, icnn_form)) return INR_EUNSUPPORTED;
        if (!ws || !grid_ok(g, n, max_points)) return INR_EINVAL;
        if (md->act0 < INR_ACT_RELU || md->act0 > INR_ACT_SIN) return INR_EINVAL;
        m = make_wide_map(md);
        const bool pre0 = md->act0 != INR_ACT_RELU;
        bytes = wide_total_bytes(m, g->n_points, pre0, n);
        if (ws_bytes < bytes) return INR_EWORKSPACE;
        w = carve_wide(m, g->n_points, pre0, ws);
        coef_all = (float*)((char*)ws + w.bytes);
        grid = *g;
        n_images = n;
        return INR_OK;
    }
    long long carve_behind(const InrModelDesc* md, const InrGridDesc& dgrid, int n, void* base) {
        m = make_wide_map(md);
        const WideBehind q = carve_wide_behind(m, dgrid.n_points, n, base);
        w = q.w;
        coef_all = q.coef;
        logit = q.logit;
        dy = q.dy;
        grid = dgrid;
        n_images = n;
        return q.bytes;
    }
    // several outputs: 'mean' over the O x N elements (torch's MSELoss on (N, O)), no class weights from the targets
    int loss_ok(const InrLossDesc* l) const {
        return m.O > 1 && l->weight_mode != INR_WEIGHT_NONE && l->weight_mode != INR_WEIGHT_EXPLICIT ? INR_EINVAL : INR_OK;
    }
    int device() { return INR_OK; }
    int P() const { return m.P; }
    float* coef() const { return coef_all; }
    long long tstride() const { return (long long)m.O * grid.n_points; }
    bool coef_for(int loss_kind) const { return loss_kind != INR_LOSS_EXTERNAL; }   // (targets = dL/dlogits: nothing to weigh)
    int units() const { return n_images; }
    int pack(const float*, hipStream_t) { return INR_OK; }   // (wide_forward's layer-0 launch packs the weights)
    int infer(const float* params, float* logits, hipStream_t s) {
        for (int img = 0; img < n_images; ++img)
            if (const int rc = wide_forward(m, w, model, params + (size_t)img * m.P, &grid, img, nullptr, 0, false,
                                            logits + (size_t)img * tstride(), s))
                return rc;
        return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
    }
    void begin_updates(float* params, float* opt_state, float* loss_hist, int32_t* status, const InrOptDesc* opt, int steps) {
        u = wide_upd_args(m, w.grads, opt, steps);
        params0 = params;
        opt0 = opt_state;
        hist0 = loss_hist;
        status0 = status;
    }
    void set_step(int, const InrOptDesc* opt, int t, int hist_idx) { set_step_consts(u, opt, t, hist_idx); }
    float* hdr() const { return opt0 + 2 * (size_t)m.P; }
    long long opt_stride() const { return 2 * (long long)m.P + INR_OPT_HEADER_FLOATS; }
    int32_t* status() const { return status0; }
    // forward + backward of image k: gradients and the loss into w.grads.  With dxd, dL/dlogits (dy) comes from the logits of the
    // output pass, which a fit or loss_grad keeps in the scratch row `logit` (and copies out where asked) and a joint step writes to the
    // caller's row.
    int train(int k, const float* params, const TrainPass& a, hipStream_t s) {
        const long long N = grid.n_points, ON = tstride();
        const bool ext = a.loss_kind == INR_LOSS_EXTERNAL, need_dy = a.dxd && !ext;
        const float* p = params + (size_t)k * m.P;
        const float* tg = a.targets + (size_t)k * ON;
        float* out = a.logits ? a.logits + (size_t)k * ON : nullptr;
        float* lg = need_dy && !a.term ? logit : out;
        WideJoint jn{};
        if (a.term) {
            jn.seg = a.term->align_seg;
            jn.c_align = a.term->c_align;
            jn.data_count = a.term->data_count > 0 ? a.term->data_count : N;
            jn.align_begin = a.term->align_begin;
            jn.use_noneclass = a.term->use_noneclass;
            jn.align_soft = a.term->align_soft;
            jn.noneclass = a.term->noneclass;
        }
        w.coef = coef_all + 2 * k;
        int rc = wide_forward(m, w, model, p, &grid, k, tg, a.loss_kind, true, ext ? nullptr : lg, s, a.term ? &jn : nullptr);
        if (rc) return rc;
        if (need_dy) {
            const dim3 dygrid((unsigned)((N + 255) / 256));
            if (a.term)
                hipLaunchKernelGGL(pcn_wide_dy_kernel<true>, dygrid, dim3(256), 0, s, (const float*)lg, tg, (const float*)w.coef, a.loss_kind, N,
                                   dy, jn);
            else
                hipLaunchKernelGGL(pcn_wide_dy_kernel<false>, dygrid, dim3(256), 0, s, (const float*)lg, tg, (const float*)w.coef, a.loss_kind,
                                   N, dy, jn);
        }
        if ((rc = wide_backward(m, w, model, p, N, s, need_dy ? dy : tg, a.dxd ? a.dxd + (size_t)k * m.C * N : nullptr,
                                !(m.general() && a.freeze_input))))   // frozen features: dZ_0 has no use
            return rc;
        if (lg != out && out && hipMemcpyAsync(out, lg, sizeof(float) * N, hipMemcpyDeviceToDevice, s) != hipSuccess) return INR_ELAUNCH;
        return INR_OK;
    }
    LossColumn loss_column() const { return LossColumn{w.grads, 1, u.PS, m.P}; }
    int grads_out(int k, float* grads, float* loss_out, hipStream_t s) {
        if (hipMemcpyAsync(grads + (size_t)k * m.P, w.grads, sizeof(float) * m.P, hipMemcpyDeviceToDevice, s) != hipSuccess) return INR_ELAUNCH;
        if (loss_out && hipMemcpyAsync(loss_out + k, w.grads + m.P, sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) return INR_ELAUNCH;
        return INR_OK;
    }
    // icnn_update_kernel on the one-slab view (it writes the next learning rate and the "frozen" flag into the image's header)
    int update(int k, hipStream_t s) {
        u.params = params0 + (size_t)k * m.P;
        u.opt_state = opt0 + (size_t)k * opt_stride();
        u.loss_hist = hist0 ? hist0 + (size_t)k * u.hist_stride : nullptr;
        u.status = status0 ? status0 + k : nullptr;
        launch_wide_update(m, u, s);
        return INR_OK;
    }
};

// The checks of a deformed prior, every argument and no device call: the deformation's description and the backbone's shape, the
// channels, the workspace pointer and the grid, then the carve: the deformation's buffers | the backbone's on the deformed grid.
template <class F, class B>
int check_deformed(F& f, B& b, const InrModelDesc* model, const InrGridDesc* grid, int n_images, void* ws, int64_t ws_bytes) {
    if (!f.desc_ok() || !b.find(model, true)) return INR_EUNSUPPORTED;
    if (const int rc = f.channels_ok(model->in_features)) return rc;
    if (!ws || !grid_ok(grid, n_images, B::max_points) || !f.grid_rule(grid)) return INR_EINVAL;
    f.carve(grid, n_images, ws);
    f.bytes += b.carve_behind(model, f.dgrid, n_images, (char*)ws + f.bytes);
    return ws_bytes < f.bytes ? INR_EWORKSPACE : INR_OK;
}

struct NoDeform {   // ConvexNet / ConvexNextNet: the ICNN on the caller's grid
    static constexpr bool none = true;
    float* dxd = nullptr;
    long long bytes = 0;
    template <class B>
    int check(B& b, const InrModelDesc* model, const InrGridDesc* grid, int n, void* ws, int64_t ws_bytes, bool icnn_form) {
        const int rc = b.check(model, grid, n, ws, ws_bytes, icnn_form);
        bytes = b.bytes;
        return rc;
    }
    int in_channels(const InrModelDesc* model) const { return model->in_features; }   // channels of the caller's grid
    int device() { return INR_OK; }
    void begin(hipStream_t) {}
    void step(int) {}
    void forward(bool, bool, hipStream_t) {}
    void gradients(hipStream_t) {}
    template <class B>
    void update(B&, bool, hipStream_t) {}
};

struct FlowDeform : CdnWs {   // ConvexDiffeomorphismNet: the ICNN behind the weight-normed coupling flow
    static constexpr bool none = false;
    const InrFlowDesc* flow;
    float *params, *opt_state, *grads;   // the flow's (opt_state: fit and joint step; grads: loss_grad)
    float wd_g;                          // weight decay on weight_g
    const InrGridDesc* grid = nullptr;   // the caller's
    int n_images = 0;
    FlowDeform(const InrFlowDesc* f, const float* p, float* o = nullptr, float* g = nullptr, float wd = 0.f)
        : flow(f), params(const_cast<float*>(p)), opt_state(o), grads(g), wd_g(wd) {}
    bool desc_ok() const { return flow_ok(flow); }
    int channels_ok(int c) const { return c == 2 ? INR_OK : INR_EUNSUPPORTED; }   // the reference flow is 2-D only (diffeomorphism_net.py:288)
    bool grid_rule(const InrGridDesc*) const { return true; }
    void carve(const InrGridDesc* g, int n, void* ws) {
        static_cast<CdnWs&>(*this) = carve_cdn(flow, g, n, ws);
        grid = g;
        n_images = n;
    }
    template <class B>
    int check(B& b, const InrModelDesc* model, const InrGridDesc* g, int n, void* ws, int64_t ws_bytes, bool) {
        return check_deformed(*this, b, model, g, n, ws, ws_bytes);
    }
    int in_channels(const InrModelDesc* model) const { return model->in_features; }
    int device() { return INR_OK; }
    // the flow's effective weights (mode 2): once per call; in the fit, the update kernel rebuilds them after every step
    void begin(hipStream_t s) { launch_flow_update(*this, flow, n_images, 2, params, nullptr, s); }
    void step(int) {}
    void forward(bool, bool, hipStream_t s) { launch_flow_fwd(*this, grid, n_images, xd, s); }
    void gradients(hipStream_t s) {
        launch_flow_bwd(*this, flow, grid, n_images, s);
        launch_flow_update(*this, flow, n_images, 1, params, grads, s);
    }
    template <class B>
    void update(B& b, bool, hipStream_t s) {
        // the learning rate of THIS step sits in the ICNN header's [t & 1] (the plateau thread writes the next one into the other slot)
        const UpdArgs& u = b.u;
        const FlowUpdArgs uf = make_flow_upd_args(*this, 0, params, opt_state, nullptr, &u.opt, wd_g, u.t, b.hdr(), b.opt_stride(),
                                                  b.status(), u.gscale);
        if constexpr (B::fused) {
            if (upd_union_ok(b.e->img.sl_cols, 2 * flow->num_coupling + 1)) {
                launch_flow_bwd(*this, flow, grid, n_images, s);
                launch_cdn_update(b.e, u, uf, flow, n_images, s);   // (the ICNN half writes `status`: the flow half gets none)
                return;
            }
            launch_icnn_update(b.e, u, s);
        }
        // (layer by layer the unit loop has stepped every image's ICNN: its header holds the frozen flag of this step)
        launch_flow_bwd(*this, flow, grid, n_images, s);
        launch_flow_update_args(flow, n_images, uf, s);
    }
};

struct RnvpDeform : PcnWs {   // PathConnectedNet: the ICNN behind the normflows RealNVP
    static constexpr bool none = false;
    const InrRnvpDesc* rnvp;
    float *params, *opt_state, *grads;   // the RealNVP's (opt_state: fit and joint step; grads: loss_grad)
    float wd;                            // its weight decay
    const InrGridDesc* grid = nullptr;   // the caller's
    int n_images = 0;
    RnvpDeform(const InrRnvpDesc* r, const float* p, float* o = nullptr, float* g = nullptr, float w = 0.f)
        : rnvp(r), params(const_cast<float*>(p)), opt_state(o), grads(g), wd(w) {}
    bool desc_ok() const { return rnvp_ok(rnvp); }
    int channels_ok(int c) const { return c == rnvp->channels ? INR_OK : INR_EINVAL; }
    bool grid_rule(const InrGridDesc* g) const { return !(g->mode == INR_GRID_SEPARABLE && rnvp->channels == 3 && !g->ts); }   // the t axis
    void carve(const InrGridDesc* g, int n, void* ws) {
        static_cast<PcnWs&>(*this) = carve_pcn(rnvp, g, n, ws);
        grid = g;
        n_images = n;
    }
    template <class B>
    int check(B& b, const InrModelDesc* model, const InrGridDesc* g, int n, void* ws, int64_t ws_bytes, bool) {
        return check_deformed(*this, b, model, g, n, ws, ws_bytes);
    }
    int in_channels(const InrModelDesc* model) const { return model->in_features; }
    int device() { return rnvp_set_lds(); }   // flow records of wide MLPs exceed the default 64 KB of dynamic LDS
    void begin(hipStream_t) {}
    void step(int) {}
    // the parameters are packed into RE in front of the forward - except in the fit after its first step (`packed`), where the update
    // kernel has refreshed RE (update with fit = true)
    void forward(bool train, bool packed, hipStream_t s) { launch_rnvp_fwd(*this, params, grid, n_images, xd, train, s, false, packed); }
    void gradients(hipStream_t s) {
        launch_rnvp_bwd(*this, params, grid, n_images, s);
        launch_rnvp_grads(*this, n_images, params, grads, s);
    }
    template <class B>
    void update(B& b, bool fit, hipStream_t s) {
        // the learning rate of THIS step sits in the ICNN header's [t & 1] (the plateau thread writes the next one into the other slot)
        const UpdArgs& u = b.u;
        RnvpUpdArgs ru = make_rnvp_upd_args(*this, n_images, 0, params, opt_state, nullptr, &u.opt, wd, u.t, b.hdr(), b.opt_stride(),
                                            b.status());
        ru.gscale = u.gscale;
        if (fit) ru.RE = RE;   // the next step's forward reuses it (`packed`)
        if constexpr (B::fused) {
            if (upd_union_ok(b.e->img.sl_cols, rm.F + 1)) {
                launch_rnvp_bwd(*this, params, grid, n_images, s);
                launch_pcn_update(b.e, *this, u, ru, n_images, s);   // (the ICNN half writes `status`: the RealNVP half gets none)
                return;
            }
            launch_icnn_update(b.e, u, s);
        }
        launch_rnvp_bwd(*this, params, grid, n_images, s);
        launch_rnvp_update_args(*this, n_images, ru, s);
    }
};

// whether F::update runs the backbone's optimizer step too (else the skeletons call b.update in the unit loop)
template <class B, class F>
constexpr bool update_merged = B::fused && !F::none;

template <class B, class F>
int device_ready(B& b, F& f) {
    const int rc = f.device();
    return rc ? rc : b.device();
}

// the optimizer and loss rules of the fits (a fit evaluates its own loss: no INR_LOSS_EXTERNAL)
static int check_fit(const InrOptDesc* opt, const InrLossDesc* loss, bool adam_only) {
    if (opt->kind != INR_OPT_ADAM && (adam_only || opt->kind != INR_OPT_ADAMAX)) return INR_EINVAL;
    if (const int rc = check_loss(loss)) return rc;
    return loss->kind == INR_LOSS_EXTERNAL ? INR_EINVAL : INR_OK;
}

template <class B, class F>
int forward_run(B b, F f, const InrModelDesc* model, const float* params, const InrGridDesc* grid, int n_images, float* logits,
                void* workspace, int64_t workspace_bytes, hipStream_t s) {
    int rc = f.check(b, model, grid, n_images, workspace, workspace_bytes, false);
    if (rc || (rc = device_ready(b, f))) return rc;
    f.begin(s);
    f.forward(false, false, s);
    if ((rc = b.pack(params, s))) return rc;
    return b.infer(params, logits, s);
}

// loss + gradients of every image (loss->kind may be INR_LOSS_EXTERNAL: `targets` = dL/dlogits, and on the plain layer-by-layer path
// loss_out may be null); dcoords: NoDeform only, dL/dcoords as well (inrfit_backward)
template <class B, class F>
int loss_grad_run(B b, F f, const InrModelDesc* model, const float* params, const InrGridDesc* grid, const float* targets,
                  const InrLossDesc* loss, int n_images, float* loss_out, float* grads, void* workspace, int64_t workspace_bytes,
                  hipStream_t s, float* dcoords = nullptr) {
    int rc = f.check(b, model, grid, n_images, workspace, workspace_bytes, false);
    if (rc || (rc = b.loss_ok(loss)) || (rc = device_ready(b, f))) return rc;
    f.begin(s);
    f.forward(true, false, s);
    if (b.coef_for(loss->kind)) hipLaunchKernelGGL(loss_coef_kernel, dim3(n_images), dim3(256), 0, s, targets, b.tstride(), *loss, b.coef(), 1.f);
    if ((rc = b.pack(params, s))) return rc;
    TrainPass a{targets, loss->kind};
    a.dxd = F::none ? dcoords : f.dxd;
    for (int k = 0; k < b.units(); ++k)
        if ((rc = b.train(k, params, a, s)) || (rc = b.grads_out(k, grads, loss_out, s))) return rc;
    f.gradients(s);
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

// One optimizer step: the deformation's forward (all images) | per unit: the training pass, then (unless F::update owns it) the ICNN's
// update | the deformation's backward seeded from dxd and its update.  `step`: the 0-based number of the step (t = step + 1);
// `packed`: the update of the step in front has left the deformation's packed parameters in this workspace.
template <class B, class F>
int fit_step(B& b, F& f, float* params, const TrainPass& a, const InrOptDesc* opt, int step, int hist_idx, bool packed, hipStream_t s) {
    b.set_step(step, opt, step + 1, hist_idx);
    f.step(step);   // (a deformation whose forward depends on the step number: PoseDeform's mirror switch)
    f.forward(true, packed, s);
    for (int k = 0; k < b.units(); ++k) {
        if (const int rc = b.train(k, params, a, s)) return rc;
        if constexpr (!update_merged<B, F>)
            if (const int rc = b.update(k, s)) return rc;
    }
    f.update(b, true, s);
    return INR_OK;
}

template <class B, class F>
int fit_run(B b, F f, const InrModelDesc* model, float* params, float* opt_state, const InrGridDesc* grid, const float* targets,
            const InrLossDesc* loss, const InrOptDesc* opt, int n_images, int steps, int step0, float* loss_hist, float* final_logits,
            int32_t* status, void* workspace, int64_t workspace_bytes, hipStream_t s) {
    int rc = f.check(b, model, grid, n_images, workspace, workspace_bytes, false);
    if (rc || (rc = b.loss_ok(loss)) || (rc = device_ready(b, f))) return rc;
    hipLaunchKernelGGL(loss_coef_kernel, dim3(n_images), dim3(256), 0, s, targets, b.tstride(), *loss, b.coef(), 1.f);
    hipLaunchKernelGGL(opt_init_kernel, dim3(n_images), dim3(64), 0, s, opt_state, b.P(), *opt, step0);
    if (status && hipMemsetAsync(status, 0, sizeof(int32_t) * n_images, s) != hipSuccess) return INR_ELAUNCH;
    if ((rc = b.pack(params, s))) return rc;
    f.begin(s);
    b.begin_updates(params, opt_state, loss_hist, status, opt, steps);
    // bench.py's timing hooks bracket the plain fused fit's launches only: events elsewhere would change what is launched and measured
    if constexpr (B::fused && F::none) b.timed = true;
    // opt->logits_at_last_forward: final_logits = the output of the LAST training forward (parameters before the last optimizer
    // step) - what the reference's IoU gate looks at (path_connected_net.py:939-972) - written by that step's pass itself
    const bool gate_logits = final_logits && opt->logits_at_last_forward && steps > 0;
    TrainPass a{targets, loss->kind};
    a.dxd = f.dxd;
    a.freeze_input = opt->freeze_input;
    for (int it = 0; it < steps; ++it) {
        a.logits = gate_logits && it == steps - 1 ? final_logits : nullptr;
        if ((rc = fit_step(b, f, params, a, opt, step0 + it, it, it > 0, s))) return rc;
    }
    if (hipGetLastError() != hipSuccess) return INR_ELAUNCH;
    if (final_logits && !gate_logits) {
        f.forward(false, false, s);
        return b.infer(params, final_logits, s);
    }
    return INR_OK;
}

// A frozen step hands a layer-by-layer backbone's caller a zero gradient: d loss / d seg of a non-finite loss has no meaning, and the
// kernels that write it (joint_loss_grad_kernel<true>, joint_prior_dseg_kernel) do not look at the status.  gscale is the finish
// kernel's: NaN = frozen.  (The fused joint steps do not launch it.)
__global__ __launch_bounds__(256) void joint_dseg_gate_kernel(const float* __restrict__ gscale, long long N, float* __restrict__ dseg) {
    if (isfinite(gscale[0])) return;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < N; e += (long long)gridDim.x * 256) dseg[e] = 0.f;
}
static void joint_dseg_gate(const float* gscale, long long N, float* dseg, int blocks, hipStream_t s) {
    hipLaunchKernelGGL(joint_dseg_gate_kernel, dim3(blocks), dim3(256), 0, s, gscale, N, dseg);
}

// the ICNN update of a joint step: one optimizer step per call, so no plateau scheduler; the reduced gradient is scaled by the finish
// kernel's `gscale`
template <class B>
void joint_begin_update(B& b, float* params, float* opt_state, int32_t* status, const InrOptDesc* opt, int step, const float* gscale) {
    InrOptDesc o = *opt;
    o.plateau = 0;
    b.begin_updates(params, opt_state, nullptr, status, &o, 1);
    b.u.gscale = gscale;
    b.set_step(step, &o, step, 0);
}

// The fused joint step: joint_begin | the deformation's forward | the training pass with the joint data term (its loss column = the
// prior's whole share, with the UNCLIPPED coefficient; dxd unscaled) | the finish kernel (gscale), in front of both updates: they read
// it | the ICNN's update x gscale | the deformation's backward seeded from dxd and its update x gscale | d loss / d seg.  Nothing is
// read on the host.
template <class B, class F>
int joint_step_run(B b, F f, const InrModelDesc* model, float* params, float* opt_state, const InrGridDesc* grid, const float* seg,
                   const float* target, const InrJointLossDesc* desc, const InrOptDesc* opt, int step, float* loss_out, float* dseg,
                   float* prior_logits, int32_t* status, void* workspace, int64_t workspace_bytes, hipStream_t s) {
    int rc = f.check(b, model, grid, 1, workspace, workspace_bytes, true);
    if (rc) return rc;
    const long long N = grid->n_points;
    if (workspace_bytes < align256(f.bytes) + joint_ws_bytes(N)) return INR_EWORKSPACE;
    if ((rc = check_joint_step(desc, opt, step)) || (rc = device_ready(b, f))) return rc;   // (every argument first, then the device)
    float* jws = (float*)((char*)workspace + align256(f.bytes));
    float* logits = prior_logits ? prior_logits : (float*)((char*)jws + align256(inrfit_joint_loss_workspace_bytes(N)));
    JointCtx c;
    if ((rc = joint_begin(desc, opt, seg, target, N, step, logits, jws, opt_state + 2 * (size_t)b.P(), b.coef(), s, &c))) return rc;
    if (status && hipMemsetAsync(status, 0, sizeof(int32_t), s) != hipSuccess) return INR_ELAUNCH;
    if ((rc = b.pack(params, s))) return rc;
    joint_begin_update(b, params, opt_state, status, opt, step, c.gscale);
    f.begin(s);
    f.forward(true, false, s);
    TrainPass a{c.prior_targets, c.prior_loss.kind};
    a.logits = logits;
    a.dxd = f.dxd;
    a.term = &c.term;
    if ((rc = b.train(0, params, a, s))) return rc;
    joint_finish(c, b.loss_column(), loss_out, s);
    if constexpr (!update_merged<B, F>)
        if ((rc = b.update(0, s))) return rc;   // (layer by layer: writes the frozen flag of this step into the header)
    f.update(b, false, s);
    joint_dseg(c, dseg, s);
    if constexpr (!B::fused) joint_dseg_gate(c.gscale, N, dseg, c.jl.blocks, s);
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

}  // namespace

#include "sequence.h"
#include "minibatch.h"
#include "sym.h"

// ---- the rotation / mirror-symmetry prior: the pose as one more deformation (csrc/sym.h) ------------------------------------------------
namespace {

struct SymWs {
    float *xd, *dxd, *part;
    int blocks;          // blocks of the point kernels = rows of `part` per image
    long long bytes;
    InrGridDesc dgrid;   // the 3-channel feature grid handed to the backbone
};

static SymWs carve_sym(const InrGridDesc* grid, int n_images, void* base) {
    SymWs w;
    const long long N = grid->n_points;
    w.blocks = (int)((N + 255) / 256);
    char* b = (char*)base;
    long long off = 0;
    auto take = [&](long long bytes) { float* p = (float*)(b + off); off += align256(bytes); return p; };
    w.xd = take((long long)n_images * 3 * N * 4);
    w.dxd = take((long long)n_images * 3 * N * 4);
    w.part = take((long long)n_images * w.blocks * SYM_POSE * 4);
    w.dgrid = *grid;
    w.dgrid.mode = INR_GRID_EXPLICIT;
    w.dgrid.coords = w.xd;
    w.dgrid.coords_image_stride = 3 * N;
    w.bytes = off;
    return w;
}

static bool sym_ok(const InrSymDesc* d) { return d && d->r_eps > 0.f && d->r_eps < INFINITY; }

// RotationSymmetricNet: the network 3 -> h -> h -> 1 behind the pose (offset, orientation).  It reads a 2-channel grid and hands the
// backbone 3 channels; its three parameters take the step FlowDeform's separate update launch takes: the learning rate and the
// "frozen" flag from the ICNN headers, b.u's status and gscale.
struct PoseDeform : SymWs {
    static constexpr bool none = false;
    const InrSymDesc* sym;
    float *pose, *opt_state, *grads;     // [n][3]; opt_state [n][6]: fit; grads [n][3]: loss_grad
    int mirror;                          // this pass mirrors (a fit sets it per step: step)
    bool by_step;
    const InrGridDesc* grid = nullptr;   // the caller's
    int n_images = 0;
    // mirror_flag < 0: a fit, the switch of sym->symmetry_from_step
    PoseDeform(const InrSymDesc* d, const float* p, int mirror_flag, float* o = nullptr, float* g = nullptr)
        : sym(d), pose(const_cast<float*>(p)), opt_state(o), grads(g), mirror(mirror_flag > 0), by_step(mirror_flag < 0) {}
    bool desc_ok() const { return sym_ok(sym); }
    int channels_ok(int c) const { return c == 3 ? INR_OK : INR_EUNSUPPORTED; }   // the backbone reads (u, v, r)
    int in_channels(const InrModelDesc*) const { return 2; }
    bool grid_rule(const InrGridDesc*) const { return true; }
    void carve(const InrGridDesc* g, int n, void* ws) {
        static_cast<SymWs&>(*this) = carve_sym(g, n, ws);
        grid = g;
        n_images = n;
    }
    template <class B>
    int check(B& b, const InrModelDesc* model, const InrGridDesc* g, int n, void* ws, int64_t ws_bytes, bool) {
        return check_deformed(*this, b, model, g, n, ws, ws_bytes);
    }
    int device() { return INR_OK; }
    void begin(hipStream_t) {}
    void step(int k) {
        if (by_step) mirror = sym->symmetry_from_step >= 0 && k >= sym->symmetry_from_step;
    }
    dim3 point_grid() const { return dim3((unsigned)blocks, (unsigned)n_images); }
    void forward(bool, bool, hipStream_t s) {
        SymFwdArgs a{};
        a.grid = *grid;
        a.pose = pose;
        a.xd = xd;
        a.N = grid->n_points;
        a.eps = sym->r_eps;
        a.mirror = mirror;
        hipLaunchKernelGGL(sym_fwd_kernel, point_grid(), dim3(256), 0, s, a);
    }
    void backward(hipStream_t s) {
        SymBwdArgs a{};
        a.grid = *grid;
        a.pose = pose;
        a.dxd = dxd;
        a.part = part;
        a.N = grid->n_points;
        a.eps = sym->r_eps;
        a.mirror = mirror;
        a.blocks = blocks;
        hipLaunchKernelGGL(sym_bwd_kernel, point_grid(), dim3(256), 0, s, a);
    }
    void gradients(hipStream_t s) {
        backward(s);
        SymUpdArgs u{};
        u.grads_out = grads;
        u.part = part;
        u.blocks = blocks;
        u.mode = 1;
        hipLaunchKernelGGL(sym_update_kernel, dim3(n_images), dim3(64), 0, s, u);
    }
    // ICNN update (over the fused backbone: this owns it) | pose backward | pose update
    template <class B>
    void update(B& b, bool, hipStream_t s) {
        const UpdArgs& bu = b.u;
        if constexpr (B::fused) launch_icnn_update(b.e, bu, s);
        backward(s);
        SymUpdArgs u{};
        u.pose = pose;
        u.opt = opt_state;
        u.part = part;
        u.lr_hdr = b.hdr();   // the learning rate of THIS step sits in the ICNN header's [t & 1]
        u.hdr_stride = b.opt_stride();
        u.status = b.status();
        u.gscale = bu.gscale;
        u.blocks = blocks;
        u.t = bu.t;
        u.mode = 0;
        u.c = opt_consts(&bu.opt, bu.t);
        u.wd = bu.opt.weight_decay;
        hipLaunchKernelGGL(sym_update_kernel, dim3(n_images), dim3(64), 0, s, u);
    }
};

// the shape of the network behind the pose: a fused kernel (C = 3) or the layer-by-layer ICNN form
static bool sym_shape_ok(const InrModelDesc* model) {
    return model && model->in_features == 3 && (find_entry(model) || pcn_wide_shape(model));
}

}  // namespace

extern "C" {

int64_t inrfit_sym_workspace_bytes(const InrModelDesc* model, const InrGridDesc* grid, int n_images) {
    if (!sym_shape_ok(model)) return INR_EUNSUPPORTED;
    if (!grid || grid->n_points <= 0 || n_images <= 0) return INR_EINVAL;
    const long long own = carve_sym(grid, n_images, nullptr).bytes;
    if (const KernelEntry* e = find_entry(model)) return own + align256(carve(e, grid->n_points, n_images, nullptr).bytes);
    return own + carve_wide_behind(make_wide_map(model), grid->n_points, n_images, nullptr).bytes;
}

int64_t inrfit_sym_minibatch_workspace_bytes(const InrModelDesc* model, int64_t batch, int n_images) {
    if (!sym_shape_ok(model)) return INR_EUNSUPPORTED;
    if (!mb_sizes_ok(model, 1, batch, n_images, 0, 0)) return INR_EINVAL;
    // the step's workspace is carved anew for every count: the largest over 1..batch (the layouts round per count)
    long long own = 0;
    InrGridDesc g = seq_grid(nullptr, 1);
    for (long long c = 1; c <= batch; ++c) {
        g.n_points = c;
        const long long o = inrfit_sym_workspace_bytes(model, &g, n_images);
        if (o < 0) return o;
        if (o > own) own = o;
    }
    return mb_layout(2, 1, batch, n_images, nullptr).head_bytes + align256(own);
}

int inrfit_sym_forward(const InrModelDesc* model, const InrSymDesc* sym, const float* params, const float* pose_params,
                       const InrGridDesc* grid, int n_images, int mirror, float* logits, void* workspace, int64_t workspace_bytes,
                       void* stream) {
    if (!params || !pose_params || !logits || !sym_ok(sym)) return INR_EINVAL;
    const PoseDeform f(sym, pose_params, mirror ? 1 : 0);
    if (pcn_wide_shape(model))
        return forward_run(WideIcnn(), f, model, params, grid, n_images, logits, workspace, workspace_bytes, (hipStream_t)stream);
    return forward_run(FusedIcnn(), f, model, params, grid, n_images, logits, workspace, workspace_bytes, (hipStream_t)stream);
}

int inrfit_sym_loss_grad(const InrModelDesc* model, const InrSymDesc* sym, const float* params, const float* pose_params,
                         const InrGridDesc* grid, const float* targets, const InrLossDesc* loss, int n_images, int mirror,
                         float* loss_out, float* grads, float* pose_grads, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!params || !pose_params || !targets || !loss_out || !grads || !pose_grads || !sym_ok(sym)) return INR_EINVAL;
    if (const int rc = check_loss(loss)) return rc;
    if (loss->kind == INR_LOSS_EXTERNAL) return INR_EINVAL;
    const PoseDeform f(sym, pose_params, mirror ? 1 : 0, nullptr, pose_grads);
    if (pcn_wide_shape(model))
        return loss_grad_run(WideIcnn(), f, model, params, grid, targets, loss, n_images, loss_out, grads, workspace, workspace_bytes,
                             (hipStream_t)stream);
    return loss_grad_run(FusedIcnn(), f, model, params, grid, targets, loss, n_images, loss_out, grads, workspace, workspace_bytes,
                         (hipStream_t)stream);
}

int inrfit_sym_fit(const InrModelDesc* model, const InrSymDesc* sym, float* params, float* pose_params, float* opt_state,
                   float* pose_opt_state, const InrGridDesc* grid, const float* targets, const InrLossDesc* loss, const InrOptDesc* opt,
                   int n_images, int steps, int step0, float* loss_hist, int32_t* status, void* workspace, int64_t workspace_bytes,
                   void* stream) {
    if (!params || !pose_params || !opt_state || !pose_opt_state || !targets || !opt || !sym_ok(sym) || steps < 0 || step0 < 0)
        return INR_EINVAL;
    if ((long long)steps + step0 > 0x7fffffffLL) return INR_EINVAL;
    if (const int rc = check_fit(opt, loss, true)) return rc;   // the pose's optimizer step is Adam's only
    const PoseDeform f(sym, pose_params, -1, pose_opt_state);
    if (pcn_wide_shape(model))
        return fit_run(WideIcnn(), f, model, params, opt_state, grid, targets, loss, opt, n_images, steps, step0, loss_hist, nullptr, status,
                       workspace, workspace_bytes, (hipStream_t)stream);
    return fit_run(FusedIcnn(), f, model, params, opt_state, grid, targets, loss, opt, n_images, steps, step0, loss_hist, nullptr, status,
                   workspace, workspace_bytes, (hipStream_t)stream);
}

int inrfit_sym_fit_minibatch(const InrModelDesc* model, const InrSymDesc* sym, float* params, float* pose_params, float* opt_state,
                             float* pose_opt_state, const float* pool_coords, const float* pool_targets, int64_t n_pool,
                             const int32_t* index, const int32_t* counts, int64_t batch, const InrLossDesc* loss, const InrOptDesc* opt,
                             int n_images, int steps, int step0, float* loss_hist, int32_t* status, void* workspace,
                             int64_t workspace_bytes, void* stream) {
    if (!params || !pose_params || !opt_state || !pose_opt_state || !sym_ok(sym)) return INR_EINVAL;
    if (const int rc = mb_check_args(model, pool_coords, pool_targets, n_pool, index, counts, batch, loss, opt, n_images, steps, step0,
                                     true))   // the pose's optimizer step is Adam's only
        return rc;
    if (!sym_shape_ok(model)) return INR_EUNSUPPORTED;
    const PoseDeform f(sym, pose_params, -1, pose_opt_state);
    if (pcn_wide_shape(model))
        return mb_run<WideIcnn>(f, model, params, opt_state, pool_coords, pool_targets, n_pool, index, counts, batch, loss, opt, n_images,
                                steps, step0, loss_hist, status, workspace, workspace_bytes, (hipStream_t)stream);
    return mb_run<FusedIcnn>(f, model, params, opt_state, pool_coords, pool_targets, n_pool, index, counts, batch, loss, opt, n_images,
                             steps, step0, loss_hist, status, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"

extern "C" {

int64_t inrfit_wide_joint_step_workspace_bytes(const InrModelDesc* model, const InrGridDesc* grid) {
    if (!pcn_wide_shape(model)) return INR_EUNSUPPORTED;
    if (!grid || grid->n_points <= 0) return INR_EINVAL;
    return align256(wide_total_bytes(make_wide_map(model), grid->n_points, false, 1)) + joint_ws_bytes(grid->n_points);
}

int64_t inrfit_pcn_wide_joint_step_workspace_bytes(const InrModelDesc* model, const InrRnvpDesc* rnvp, const InrGridDesc* grid) {
    if (!rnvp_ok(rnvp) || !pcn_wide_shape(model)) return INR_EUNSUPPORTED;
    if (!grid || grid->n_points <= 0) return INR_EINVAL;
    return align256(inrfit_pcn_workspace_bytes(model, rnvp, grid, 1)) + joint_ws_bytes(grid->n_points);
}

int64_t inrfit_cdn_wide_joint_step_workspace_bytes(const InrModelDesc* model, const InrFlowDesc* flow, const InrGridDesc* grid) {
    if (!flow_ok(flow) || !cdn_wide_shape(model)) return INR_EUNSUPPORTED;
    if (!grid || grid->n_points <= 0) return INR_EINVAL;
    return align256(inrfit_cdn_workspace_bytes(model, flow, grid, 1)) + joint_ws_bytes(grid->n_points);
}

int inrfit_wide_joint_step(const InrModelDesc* model, float* params, float* opt_state, const InrGridDesc* grid, const float* seg,
                           const float* target, const InrJointLossDesc* desc, const InrOptDesc* opt, int step, float* loss_out,
                           float* dseg, float* prior_logits, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!params || !opt_state || !seg || !target || !dseg) return INR_EINVAL;
    return joint_step_run(WideIcnn(), NoDeform(), model, params, opt_state, grid, seg, target, desc, opt, step, loss_out, dseg, prior_logits,
                          status, workspace, workspace_bytes, (hipStream_t)stream);
}

int inrfit_pcn_wide_joint_step(const InrModelDesc* model, const InrRnvpDesc* rnvp, float* icnn_params, float* flow_params,
                               float* icnn_opt_state, float* flow_opt_state, const InrGridDesc* grid, const float* seg,
                               const float* target, const InrJointLossDesc* desc, const InrOptDesc* opt, float flow_weight_decay,
                               int step, float* loss_out, float* dseg, float* prior_logits, int32_t* status, void* workspace,
                               int64_t workspace_bytes, void* stream) {
    if (!icnn_params || !flow_params || !icnn_opt_state || !flow_opt_state || !seg || !target || !dseg) return INR_EINVAL;
    return joint_step_run(WideIcnn(), RnvpDeform(rnvp, flow_params, flow_opt_state, nullptr, flow_weight_decay), model, icnn_params,
                          icnn_opt_state, grid, seg, target, desc, opt, step, loss_out, dseg, prior_logits, status, workspace,
                          workspace_bytes, (hipStream_t)stream);
}

int inrfit_cdn_wide_joint_step(const InrModelDesc* model, const InrFlowDesc* flow, float* icnn_params, float* flow_params,
                               float* icnn_opt_state, float* flow_opt_state, const InrGridDesc* grid, const float* seg,
                               const float* target, const InrJointLossDesc* desc, const InrOptDesc* opt, float wd_on_weight_g,
                               int step, float* loss_out, float* dseg, float* prior_logits, int32_t* status, void* workspace,
                               int64_t workspace_bytes, void* stream) {
    if (!icnn_params || !flow_params || !icnn_opt_state || !flow_opt_state || !seg || !target || !dseg) return INR_EINVAL;
    if (!opt || opt->kind != INR_OPT_ADAM) return INR_EINVAL;   // the flow's optimizer step is Adam's only (checked before the model)
    return joint_step_run(WideIcnn(), FlowDeform(flow, flow_params, flow_opt_state, nullptr, wd_on_weight_g), model, icnn_params,
                          icnn_opt_state, grid, seg, target, desc, opt, step, loss_out, dseg, prior_logits, status, workspace,
                          workspace_bytes, (hipStream_t)stream);
}

int inrfit_forward(const InrModelDesc* model, const float* params, const InrGridDesc* grid, int n_images, float* logits,
                   void* workspace, int64_t workspace_bytes, void* stream) {
    if (!params || !logits) return INR_EINVAL;
    if (use_wide(model))
        return forward_run(WideIcnn(), NoDeform(), model, params, grid, n_images, logits, workspace, workspace_bytes, (hipStream_t)stream);
    return forward_run(FusedIcnn(), NoDeform(), model, params, grid, n_images, logits, workspace, workspace_bytes, (hipStream_t)stream);
}

int inrfit_cdn_forward(const InrModelDesc* model, const InrFlowDesc* flow, const float* icnn_params, const float* flow_params,
                       const InrGridDesc* grid, int n_images, float* logits, void* workspace, int64_t workspace_bytes,
                       void* stream) {
    if (!icnn_params || !flow_params || !logits) return INR_EINVAL;
    if (cdn_wide_shape(model))
        return forward_run(WideIcnn(), FlowDeform(flow, flow_params), model, icnn_params, grid, n_images, logits, workspace, workspace_bytes,
                           (hipStream_t)stream);
    return forward_run(FusedIcnn(), FlowDeform(flow, flow_params), model, icnn_params, grid, n_images, logits, workspace, workspace_bytes,
                       (hipStream_t)stream);
}

int inrfit_pcn_forward(const InrModelDesc* model, const InrRnvpDesc* rnvp, const float* icnn_params, const float* flow_params,
                       const InrGridDesc* grid, int n_images, float* logits, void* workspace, int64_t workspace_bytes,
                       void* stream) {
    if (!icnn_params || !flow_params || !logits) return INR_EINVAL;
    if (pcn_wide_shape(model))
        return forward_run(WideIcnn(), RnvpDeform(rnvp, flow_params), model, icnn_params, grid, n_images, logits, workspace, workspace_bytes,
                           (hipStream_t)stream);
    return forward_run(FusedIcnn(), RnvpDeform(rnvp, flow_params), model, icnn_params, grid, n_images, logits, workspace, workspace_bytes,
                       (hipStream_t)stream);
}

int inrfit_loss_grad(const InrModelDesc* model, const float* params, const InrGridDesc* grid, const float* targets,
                     const InrLossDesc* loss, int n_images, float* loss_out, float* grads, void* workspace,
                     int64_t workspace_bytes, void* stream) {
    if (!params || !targets || !loss_out || !grads) return INR_EINVAL;
    if (const int rc = check_loss(loss)) return rc;
    if (use_wide(model))
        return loss_grad_run(WideIcnn(), NoDeform(), model, params, grid, targets, loss, n_images, loss_out, grads, workspace, workspace_bytes,
                             (hipStream_t)stream);
    return loss_grad_run(FusedIcnn(), NoDeform(), model, params, grid, targets, loss, n_images, loss_out, grads, workspace, workspace_bytes,
                         (hipStream_t)stream);
}

int inrfit_backward(const InrModelDesc* model, const float* params, const InrGridDesc* grid, const float* dlogits,
                    int n_images, float* grads, float* dcoords, void* workspace, int64_t workspace_bytes, void* stream) {
    const KernelEntry* e;
    Workspace w;
    if (!params || !dlogits || !grads) return INR_EINVAL;
    if (use_wide(model)) {
        const InrLossDesc ext{INR_LOSS_EXTERNAL, INR_WEIGHT_NONE, 1.f, 0.f, 0.f};
        return loss_grad_run(WideIcnn(), NoDeform(), model, params, grid, dlogits, &ext, n_images, nullptr, grads, workspace, workspace_bytes,
                             (hipStream_t)stream, dcoords);
    }
    int rc = prepare(model, grid, n_images, workspace, workspace_bytes, &e, &w);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = launch_pack(e, w, params, n_images, s))) return rc;
    if ((rc = launch_step(e, w, true, grid, dlogits, INR_LOSS_EXTERNAL, n_images, nullptr, s, dcoords))) return rc;
    launch_reduce(e, w, n_images, grads, w.coef /* scratch: the loss slot is unused in this mode */, s);
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

int inrfit_cdn_loss_grad(const InrModelDesc* model, const InrFlowDesc* flow, const float* icnn_params,
                         const float* flow_params, const InrGridDesc* grid, const float* targets, const InrLossDesc* loss,
                         int n_images, float* loss_out, float* icnn_grads, float* flow_grads, void* workspace,
                         int64_t workspace_bytes, void* stream) {
    if (!icnn_params || !flow_params || !targets || !loss_out || !icnn_grads || !flow_grads) return INR_EINVAL;
    if (const int rc = check_loss(loss)) return rc;
    const FlowDeform f(flow, flow_params, nullptr, flow_grads);
    if (cdn_wide_shape(model))
        return loss_grad_run(WideIcnn(), f, model, icnn_params, grid, targets, loss, n_images, loss_out, icnn_grads, workspace,
                             workspace_bytes, (hipStream_t)stream);
    return loss_grad_run(FusedIcnn(), f, model, icnn_params, grid, targets, loss, n_images, loss_out, icnn_grads, workspace,
                         workspace_bytes, (hipStream_t)stream);
}

int inrfit_pcn_loss_grad(const InrModelDesc* model, const InrRnvpDesc* rnvp, const float* icnn_params,
                         const float* flow_params, const InrGridDesc* grid, const float* targets, const InrLossDesc* loss,
                         int n_images, float* loss_out, float* icnn_grads, float* flow_grads, void* workspace,
                         int64_t workspace_bytes, void* stream) {
    if (!icnn_params || !flow_params || !targets || !loss_out || !icnn_grads || !flow_grads) return INR_EINVAL;
    if (const int rc = check_loss(loss)) return rc;
    const RnvpDeform f(rnvp, flow_params, nullptr, flow_grads);
    if (pcn_wide_shape(model))
        return loss_grad_run(WideIcnn(), f, model, icnn_params, grid, targets, loss, n_images, loss_out, icnn_grads, workspace,
                             workspace_bytes, (hipStream_t)stream);
    return loss_grad_run(FusedIcnn(), f, model, icnn_params, grid, targets, loss, n_images, loss_out, icnn_grads, workspace,
                         workspace_bytes, (hipStream_t)stream);
}

int inrfit_fit(const InrModelDesc* model, float* params, float* opt_state, const InrGridDesc* grid, const float* targets,
               const InrLossDesc* loss, const InrOptDesc* opt, int n_images, int steps, int step0, float* loss_hist,
               float* final_logits, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!params || !opt_state || !targets || !opt || steps < 0 || step0 < 0) return INR_EINVAL;
    if (const int rc = check_fit(opt, loss, false)) return rc;
    if (use_wide(model))
        return fit_run(WideIcnn(), NoDeform(), model, params, opt_state, grid, targets, loss, opt, n_images, steps, step0, loss_hist,
                       final_logits, status, workspace, workspace_bytes, (hipStream_t)stream);
    return fit_run(FusedIcnn(), NoDeform(), model, params, opt_state, grid, targets, loss, opt, n_images, steps, step0, loss_hist,
                   final_logits, status, workspace, workspace_bytes, (hipStream_t)stream);
}

int inrfit_cdn_fit(const InrModelDesc* model, const InrFlowDesc* flow, float* icnn_params, float* flow_params,
                   float* icnn_opt_state, float* flow_opt_state, const InrGridDesc* grid, const float* targets,
                   const InrLossDesc* loss, const InrOptDesc* opt, float wd_on_weight_g, int n_images, int steps, int step0,
                   float* loss_hist, float* final_logits, int32_t* status, void* workspace, int64_t workspace_bytes,
                   void* stream) {
    if (!icnn_params || !flow_params || !icnn_opt_state || !flow_opt_state || !targets || !opt || steps < 0 || step0 < 0)
        return INR_EINVAL;
    if (const int rc = check_fit(opt, loss, true)) return rc;   // the flow's optimizer step is Adam's only
    const FlowDeform f(flow, flow_params, flow_opt_state, nullptr, wd_on_weight_g);
    if (cdn_wide_shape(model))
        return fit_run(WideIcnn(), f, model, icnn_params, icnn_opt_state, grid, targets, loss, opt, n_images, steps, step0, loss_hist,
                       final_logits, status, workspace, workspace_bytes, (hipStream_t)stream);
    return fit_run(FusedIcnn(), f, model, icnn_params, icnn_opt_state, grid, targets, loss, opt, n_images, steps, step0, loss_hist,
                   final_logits, status, workspace, workspace_bytes, (hipStream_t)stream);
}

int inrfit_pcn_fit(const InrModelDesc* model, const InrRnvpDesc* rnvp, float* icnn_params, float* flow_params,
                   float* icnn_opt_state, float* flow_opt_state, const InrGridDesc* grid, const float* targets,
                   const InrLossDesc* loss, const InrOptDesc* opt, float flow_weight_decay, int n_images, int steps, int step0,
                   float* loss_hist, float* final_logits, int32_t* status, void* workspace, int64_t workspace_bytes,
                   void* stream) {
    if (!icnn_params || !flow_params || !icnn_opt_state || !flow_opt_state || !targets || !opt || steps < 0 || step0 < 0)
        return INR_EINVAL;
    if (const int rc = check_fit(opt, loss, false)) return rc;
    const RnvpDeform f(rnvp, flow_params, flow_opt_state, nullptr, flow_weight_decay);
    if (pcn_wide_shape(model))
        return fit_run(WideIcnn(), f, model, icnn_params, icnn_opt_state, grid, targets, loss, opt, n_images, steps, step0, loss_hist,
                       final_logits, status, workspace, workspace_bytes, (hipStream_t)stream);
    return fit_run(FusedIcnn(), f, model, icnn_params, icnn_opt_state, grid, targets, loss, opt, n_images, steps, step0, loss_hist,
                   final_logits, status, workspace, workspace_bytes, (hipStream_t)stream);
}

int inrfit_joint_step(const InrModelDesc* model, float* params, float* opt_state, const InrGridDesc* grid, const float* seg,
                      const float* target, const InrJointLossDesc* desc, const InrOptDesc* opt, int step, float* loss_out,
                      float* dseg, float* prior_logits, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!params || !opt_state || !seg || !target || !dseg) return INR_EINVAL;
    return joint_step_run(FusedIcnn(), NoDeform(), model, params, opt_state, grid, seg, target, desc, opt, step, loss_out, dseg, prior_logits,
                          status, workspace, workspace_bytes, (hipStream_t)stream);
}

int inrfit_pcn_joint_step(const InrModelDesc* model, const InrRnvpDesc* rnvp, float* icnn_params, float* flow_params,
                          float* icnn_opt_state, float* flow_opt_state, const InrGridDesc* grid, const float* seg,
                          const float* target, const InrJointLossDesc* desc, const InrOptDesc* opt, float flow_weight_decay,
                          int step, float* loss_out, float* dseg, float* prior_logits, int32_t* status, void* workspace,
                          int64_t workspace_bytes, void* stream) {
    if (!icnn_params || !flow_params || !icnn_opt_state || !flow_opt_state || !seg || !target || !dseg) return INR_EINVAL;
    return joint_step_run(FusedIcnn(), RnvpDeform(rnvp, flow_params, flow_opt_state, nullptr, flow_weight_decay), model, icnn_params,
                          icnn_opt_state, grid, seg, target, desc, opt, step, loss_out, dseg, prior_logits, status, workspace,
                          workspace_bytes, (hipStream_t)stream);
}

int inrfit_cdn_joint_step(const InrModelDesc* model, const InrFlowDesc* flow, float* icnn_params, float* flow_params,
                          float* icnn_opt_state, float* flow_opt_state, const InrGridDesc* grid, const float* seg,
                          const float* target, const InrJointLossDesc* desc, const InrOptDesc* opt, float wd_on_weight_g,
                          int step, float* loss_out, float* dseg, float* prior_logits, int32_t* status, void* workspace,
                          int64_t workspace_bytes, void* stream) {
    if (!icnn_params || !flow_params || !icnn_opt_state || !flow_opt_state || !seg || !target || !dseg) return INR_EINVAL;
    if (!opt || opt->kind != INR_OPT_ADAM) return INR_EINVAL;   // the flow's optimizer step is Adam's only (checked before the model)
    return joint_step_run(FusedIcnn(), FlowDeform(flow, flow_params, flow_opt_state, nullptr, wd_on_weight_g), model, icnn_params,
                          icnn_opt_state, grid, seg, target, desc, opt, step, loss_out, dseg, prior_logits, status, workspace,
                          workspace_bytes, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// the prior's share of a joint step (include/inrfit.h: inrfit_joint_prior_step); the segmentation share stays with the caller
// ---------------------------------------------------------------------------------------------------------------------
namespace {

struct PriorShareArgs {
    const float* logits;    // the step kernel's pre-sigmoid output of this step
    const float* seg;
    const float* targets;   // [data_count]
    const float* coef;      // c_fg, c_bg (loss_coef_kernel: c_data / n_valid x class weight)
    long long N, data_count, align_begin;
    int kind, use_noneclass, align_rule;
    float noneclass;
    float* part;            // [blocks][2]: data term, raw align sum
    int blocks;
};

// loss_out[1] and [2] on their own (the step kernel's loss column holds them mixed), per block, for the finish kernel to combine in
// fixed order.  The data term repeats the step kernel's arithmetic on its logits; masked points are skipped, not multiplied by 0.
__global__ __launch_bounds__(256) void joint_prior_partial_kernel(const PriorShareArgs a) {
    __shared__ float sm[4];
    float ld = 0.f, la = 0.f;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < a.N; e += (long long)a.blocks * 256) {
        const float p = 1.f / (1.f + expf(-a.logits[e]));
        if (e < a.data_count) {
            const float t = a.targets[e];
            if (!(a.use_noneclass && t == a.noneclass)) {
                const float cw = t < 0.5f ? a.coef[0] : a.coef[1];
                if (a.kind == INR_LOSS_SE) {
                    const float d = t - p;
                    ld += d * d * cw;
                } else {
                    ld += -(t * bce_log(p) + (1.f - t) * bce_log(1.f - p)) * cw;
                }
            }
        }
        if (a.align_rule != INR_ALIGN_NONE && e >= a.align_begin) {
            const float s = a.seg[e];
            const float d = p - (a.align_rule == INR_ALIGN_SOFT ? s : (s > 0.5f ? 1.f : 0.f));
            la = fmaf(d, d, la);
        }
    }
    const float r0 = jl_block_sum(ld, sm);
    const float r1 = jl_block_sum(la, sm);
    if (threadIdx.x == 0) {
        a.part[2 * blockIdx.x] = r0;
        a.part[2 * blockIdx.x + 1] = r1;
    }
}

struct PriorFinArgs {
    const float* part;
    int blocks;
    const float* slabs;     // the step kernel's gradient slabs of this step [wgs][PS]
    int wgs, PS, loss_col;
    const float* seg_term;  // [1] or null
    float n_align;          // 0 without an align term
    float* gscale;          // [1] -> the update kernel
    float* loss_out;        // [4] or null
};

__global__ __launch_bounds__(256) void joint_prior_finish_kernel(const PriorFinArgs f) {
    __shared__ float sm[4];
    float v0 = 0.f, v1 = 0.f, lc = 0.f;
    for (int b = threadIdx.x; b < f.blocks; b += 256) {
        v0 += f.part[2 * b];
        v1 += f.part[2 * b + 1];
    }
    for (int w = threadIdx.x; w < f.wgs; w += 256) lc += f.slabs[(size_t)w * f.PS + f.loss_col];
    const float data = jl_block_sum(v0, sm);
    const float align = jl_block_sum(v1, sm);
    const float prior_term = jl_block_sum(lc, sm);   // the prior's whole share, as the step kernel summed it
    if (threadIdx.x != 0) return;
    const float total = (f.seg_term ? f.seg_term[0] : 0.f) + prior_term;
    // a non-finite COMPOSITE loss freezes the row: the update kernel reads a non-finite gradient scale as "no step"
    const float gs = isfinite(total) ? 1.f : __builtin_nanf("");
    f.gscale[0] = gs;
    if (f.loss_out) {
        f.loss_out[0] = total;
        f.loss_out[1] = data;
        f.loss_out[2] = f.n_align > 0.f ? align / f.n_align : 0.f;
        f.loss_out[3] = gs;
    }
}

// d(prior's share) / d seg: the soft align's -2 beta (p - s) / n_align on [align_begin, N), 0 everywhere else
__global__ __launch_bounds__(256) void joint_prior_dseg_kernel(const float* __restrict__ logits, const float* __restrict__ seg, long long N,
                                                               long long align_begin, int soft, float c, float* __restrict__ dseg) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < N; e += (long long)gridDim.x * 256) {
        float d = 0.f;
        if (soft && e >= align_begin) d = c * (1.f / (1.f + expf(-logits[e])) - seg[e]);
        dseg[e] = d;
    }
}

}  // namespace

namespace {

// argument checks of inrfit_joint_prior_step / inrfit_wide_joint_prior_step in front of the shape's own
static int check_joint_prior(const InrJointPriorDesc* desc, const InrOptDesc* opt, int step) {
    if (!opt || (opt->kind != INR_OPT_ADAM && opt->kind != INR_OPT_ADAMAX) || step < 1) return INR_EINVAL;
    if (desc->kind != INR_LOSS_SE && desc->kind != INR_LOSS_BCE) return INR_EINVAL;
    if (desc->weight_mode < INR_WEIGHT_NONE || desc->weight_mode > INR_WEIGHT_SSSDMS) return INR_EINVAL;
    if (desc->align_rule < INR_ALIGN_NONE || desc->align_rule > INR_ALIGN_SOFT) return INR_EINVAL;
    return INR_OK;
}

// the ranges of the two terms over the N points
struct PriorRanges {
    long long data_count, align_begin, n_align;
    bool align;
};
static int prior_ranges(const InrJointPriorDesc* desc, long long N, PriorRanges* r) {
    r->data_count = desc->data_count > 0 ? desc->data_count : N;
    if (desc->data_count < 0 || r->data_count > N) return INR_EINVAL;
    r->align = desc->align_rule != INR_ALIGN_NONE;
    if (r->align && (desc->align_begin < 0 || desc->align_begin >= N)) return INR_EINVAL;
    r->align_begin = r->align ? desc->align_begin : 0;
    r->n_align = r->align ? N - desc->align_begin : 0;
    return INR_OK;
}

// header, class coefficients and status in front of the prior's pass
static int joint_prior_begin(const InrJointPriorDesc* desc, const PriorRanges& r, const InrOptDesc* opt, int step, const float* target,
                             float* hdr, float* coef, int32_t* status, hipStream_t s) {
    hipLaunchKernelGGL(joint_prep_kernel, dim3(1), dim3(64), 0, s, hdr, opt->lr, step, coef, 0.f, 0);
    const InrLossDesc pl{desc->kind, desc->weight_mode, desc->ratio, 0.f, 0.f};
    hipLaunchKernelGGL(loss_coef_kernel, dim3(1), dim3(256), 0, s, target, r.data_count, pl, coef, desc->c_data, desc->use_noneclass,
                       desc->noneclass);
    if (status && hipMemsetAsync(status, 0, sizeof(int32_t), s) != hipSuccess) return INR_ELAUNCH;
    return INR_OK;
}

// behind the prior's pass: loss_out[1] and [2] on their own, then the finish kernel (gscale) on the pass's loss column; -> the blocks
// of the point-wise launches
static int joint_prior_finish(const InrJointPriorDesc* desc, const PriorRanges& r, const float* logits, const float* seg, const float* target,
                              const float* coef, long long N, float* jws, const LossColumn& lc, const float* seg_term, float* gscale,
                              float* loss_out, hipStream_t s) {
    PriorShareArgs pa{};
    pa.logits = logits;
    pa.seg = seg;
    pa.targets = target;
    pa.coef = coef;
    pa.N = N;
    pa.data_count = r.data_count;
    pa.align_begin = r.align_begin;
    pa.kind = desc->kind;
    pa.use_noneclass = desc->use_noneclass ? 1 : 0;
    pa.align_rule = desc->align_rule;
    pa.noneclass = desc->noneclass;
    pa.part = jws;
    const long long want = (N + 1023) / 1024;
    pa.blocks = (int)(want < 1 ? 1 : (want > JL_MAX_BLOCKS ? JL_MAX_BLOCKS : want));   // 2 x blocks <= the JL_PART x JL_MAX_BLOCKS floats
    hipLaunchKernelGGL(joint_prior_partial_kernel, dim3(pa.blocks), dim3(256), 0, s, pa);
    PriorFinArgs f{};
    f.part = jws;
    f.blocks = pa.blocks;
    f.slabs = lc.slabs;
    f.wgs = lc.wgs;
    f.PS = lc.PS;
    f.loss_col = lc.col;
    f.seg_term = seg_term;
    f.n_align = (float)r.n_align;
    f.gscale = gscale;
    f.loss_out = loss_out;
    hipLaunchKernelGGL(joint_prior_finish_kernel, dim3(1), dim3(256), 0, s, f);
    return pa.blocks;
}

static void joint_prior_dseg(const InrJointPriorDesc* desc, const PriorRanges& r, int blocks, const float* logits, const float* seg,
                             long long N, float* dseg, hipStream_t s) {
    const bool soft = desc->align_rule == INR_ALIGN_SOFT;
    hipLaunchKernelGGL(joint_prior_dseg_kernel, dim3(blocks), dim3(256), 0, s, logits, seg, N, r.align_begin, soft ? 1 : 0,
                       soft ? -2.f * desc->beta / (float)r.n_align : 0.f, dseg);
}

}  // namespace

}  // extern "C"

namespace {

// header, coefficients and status | the training pass with the masked data term and the align term | loss_out and gscale | the ICNN's
// update x gscale | d loss / d seg (layer by layer: zeroed on a frozen step)
template <class B>
int joint_prior_step_run(B b, const InrModelDesc* model, float* params, float* opt_state, const InrGridDesc* grid, const float* seg,
                         const float* target, const InrJointPriorDesc* desc, const float* seg_term, const InrOptDesc* opt, int step,
                         float* loss_out, float* dseg, float* prior_logits, int32_t* status, void* workspace, int64_t workspace_bytes,
                         hipStream_t s) {
    if (!params || !opt_state || !seg || !target || !dseg || !desc || !grid) return INR_EINVAL;
    int rc = check_joint_prior(desc, opt, step);
    if (rc) return rc;
    // (a shape of the other backbone, or an encode shape: INR_EUNSUPPORTED)
    if ((rc = b.check(model, grid, 1, workspace, workspace_bytes, true))) return rc;
    const long long N = grid->n_points;
    if (workspace_bytes < align256(b.bytes) + joint_ws_bytes(N)) return INR_EWORKSPACE;
    PriorRanges r;
    if ((rc = prior_ranges(desc, N, &r)) || (rc = b.device())) return rc;
    float* jws = (float*)((char*)workspace + align256(b.bytes));
    float* logits = prior_logits ? prior_logits : (float*)((char*)jws + align256(inrfit_joint_loss_workspace_bytes(N)));
    float* gscale = jws + JL_MAX_BLOCKS * JL_PART + JL_RES;
    if ((rc = joint_prior_begin(desc, r, opt, step, target, opt_state + 2 * (size_t)b.P(), b.coef(), status, s))) return rc;
    if ((rc = b.pack(params, s))) return rc;
    joint_begin_update(b, params, opt_state, status, opt, step, gscale);
    DataTerm t;
    t.align_seg = r.align ? seg : nullptr;
    t.c_align = r.align ? desc->beta / (float)r.n_align : 0.f;
    t.data_count = r.data_count;
    t.use_noneclass = desc->use_noneclass ? 1 : 0;
    t.noneclass = desc->noneclass;
    t.align_soft = desc->align_rule == INR_ALIGN_SOFT ? 1 : 0;
    t.align_begin = r.align_begin;
    TrainPass a{target, desc->kind};
    a.logits = logits;
    a.term = &t;
    if ((rc = b.train(0, params, a, s))) return rc;
    const int blocks = joint_prior_finish(desc, r, logits, seg, target, b.coef(), N, jws, b.loss_column(), seg_term, gscale, loss_out, s);
    if ((rc = b.update(0, s))) return rc;
    joint_prior_dseg(desc, r, blocks, logits, seg, N, dseg, s);
    if constexpr (!B::fused) joint_dseg_gate(gscale, N, dseg, blocks, s);
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

}  // namespace

extern "C" {

int inrfit_joint_prior_step(const InrModelDesc* model, float* params, float* opt_state, const InrGridDesc* grid, const float* seg,
                            const float* target, const InrJointPriorDesc* desc, const float* seg_term, const InrOptDesc* opt,
                            int step, float* loss_out, float* dseg, float* prior_logits, int32_t* status, void* workspace,
                            int64_t workspace_bytes, void* stream) {
    return joint_prior_step_run(FusedIcnn(), model, params, opt_state, grid, seg, target, desc, seg_term, opt, step, loss_out, dseg,
                                prior_logits, status, workspace, workspace_bytes, (hipStream_t)stream);
}

int inrfit_wide_joint_prior_step(const InrModelDesc* model, float* params, float* opt_state, const InrGridDesc* grid, const float* seg,
                                 const float* target, const InrJointPriorDesc* desc, const float* seg_term, const InrOptDesc* opt,
                                 int step, float* loss_out, float* dseg, float* prior_logits, int32_t* status, void* workspace,
                                 int64_t workspace_bytes, void* stream) {
    return joint_prior_step_run(WideIcnn(), model, params, opt_state, grid, seg, target, desc, seg_term, opt, step, loss_out, dseg,
                                prior_logits, status, workspace, workspace_bytes, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// star-shape prior of the teaser (csrc/star.h)
// ---------------------------------------------------------------------------------------------------------------------
static int check_star(const InrStarDesc* star, int64_t n_points, void* workspace, int64_t workspace_bytes, StarMap* m, StarWs* w) {
    if (!star || star->n_hidden < 1 || star->n_hidden > STAR_MAX_HIDDEN) return INR_EUNSUPPORTED;
    if (n_points <= 0 || n_points * (int64_t)star->n_hidden > (int64_t)1 << 31) return INR_EINVAL;
    if (!workspace) return INR_EINVAL;
    *m = make_star_map(star->n_hidden);
    *w = carve_star(star->n_hidden, n_points, workspace);
    if (workspace_bytes < w->bytes) return INR_EWORKSPACE;
    return INR_OK;
}

int64_t inrfit_star_param_count(const InrStarDesc* star) {
    if (!star || star->n_hidden < 1 || star->n_hidden > STAR_MAX_HIDDEN) return INR_EUNSUPPORTED;
    return make_star_map(star->n_hidden).P;
}

int64_t inrfit_star_workspace_bytes(const InrStarDesc* star, int64_t n_points) {
    if (!star || star->n_hidden < 1 || star->n_hidden > STAR_MAX_HIDDEN) return INR_EUNSUPPORTED;
    if (n_points <= 0 || n_points * (int64_t)star->n_hidden > (int64_t)1 << 31) return INR_EINVAL;
    return carve_star(star->n_hidden, n_points, nullptr).bytes;
}

int inrfit_star_forward(const InrStarDesc* star, const float* params, const float* coords, int64_t n_points, float* logits,
                        void* workspace, int64_t workspace_bytes, void* stream) {
    StarMap m;
    StarWs w;
    if (!params || !coords || !logits) return INR_EINVAL;
    int rc = check_star(star, n_points, workspace, workspace_bytes, &m, &w);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = star_forward_pass(m, w, params, coords, nullptr, n_points, n_points, nullptr, logits, s))) return rc;
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

// the centre's own step count at epoch ep (0: it takes no step yet)
static int star_offset_step(int ep, int offset_first_step) {
    return offset_first_step >= 0 && ep >= offset_first_step ? ep - offset_first_step + 1 : 0;
}

int inrfit_star_loss_grad(const InrStarDesc* star, const float* params, const float* coords, const float* labels, int64_t n_pixels,
                          const int32_t* index, int64_t batch, float* loss, float* grads, void* workspace, int64_t workspace_bytes,
                          void* stream) {
    StarMap m;
    StarWs w;
    if (!params || !coords || !labels || !grads || n_pixels <= 0 || batch > STAR_MAX_BATCH) return INR_EINVAL;
    if (!index && batch > n_pixels) return INR_EINVAL;
    int rc = check_star(star, batch, workspace, workspace_bytes, &m, &w);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = star_forward_pass(m, w, params, coords, index, n_pixels, batch, labels, nullptr, s))) return rc;
    if ((rc = star_backward_pass(m, w, params, batch, loss, 0, s))) return rc;
    StarUpdArgs u{};
    u.prm = nullptr;
    u.gW1 = w.gW1;
    u.colp = w.colp;
    u.scal = w.scal;
    u.grads_out = grads;
    u.m = m;
    u.mode = 1;
    hipLaunchKernelGGL(star_update_kernel, dim3((m.P + 255) / 256), dim3(256), 0, s, u);
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

int inrfit_star_fit(const InrStarDesc* star, float* params, float* opt_state, const float* coords, const float* labels,
                    int64_t n_pixels, const int32_t* batch_index, int64_t batch, const InrOptDesc* opt, int32_t steps, int32_t step0,
                    int32_t offset_first_step, float* loss_hist, void* workspace, int64_t workspace_bytes, void* stream) {
    StarMap m;
    StarWs w;
    if (!params || !opt_state || !coords || !labels || !batch_index || !opt || steps < 0 || step0 < 0 || n_pixels <= 0) return INR_EINVAL;
    if (opt->kind != INR_OPT_ADAM || batch > STAR_MAX_BATCH) return INR_EINVAL;
    int rc = check_star(star, batch, workspace, workspace_bytes, &m, &w);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    StarUpdArgs u{};
    u.prm = params;
    u.opt = opt_state;
    u.gW1 = w.gW1;
    u.colp = w.colp;
    u.scal = w.scal;
    u.m = m;
    u.lr = opt->lr;
    u.mode = 0;
    for (int it = 0; it < steps; ++it) {
        const int ep = step0 + it;
        const int32_t* idx = batch_index + (size_t)it * batch;
        if ((rc = star_forward_pass(m, w, params, coords, idx, n_pixels, batch, labels, nullptr, s))) return rc;
        if ((rc = star_backward_pass(m, w, params, batch, loss_hist, it, s))) return rc;
        const int t_off = star_offset_step(ep, offset_first_step);
        u.net = opt_consts(opt, ep + 1);
        u.off = opt_consts(opt, t_off);
        u.offset_on = t_off > 0;
        hipLaunchKernelGGL(star_update_kernel, dim3((m.P + 255) / 256), dim3(256), 0, s, u);
    }
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

// ---- the dense full-batch form (csrc/star.h: tiles of STAR_DENSE_TILE points, accumulated in tile order) ------------------------------
int32_t inrfit_star_dense_tile_points(void) { return STAR_DENSE_TILE; }

int64_t inrfit_star_opt_state_floats(const InrStarDesc* star) {
    if (!star || star->n_hidden < 1 || star->n_hidden > STAR_MAX_HIDDEN) return INR_EUNSUPPORTED;
    return 2 * (int64_t)make_star_map(star->n_hidden).P + INR_OPT_HEADER_FLOATS;
}

int64_t inrfit_star_dense_workspace_bytes(const InrStarDesc* star, int64_t n_pixels, int32_t n_images) {
    if (!star || star->n_hidden < 1 || star->n_hidden > STAR_MAX_HIDDEN) return INR_EUNSUPPORTED;
    if (n_pixels <= 0 || n_images <= 0) return INR_EINVAL;
    return carve_star_dense(star->n_hidden, n_pixels, n_images, nullptr).bytes;
}

// everything the two dense entry points share in front of their first HIP call
static int check_star_dense(const InrStarDesc* star, const float* params, const float* coords, int64_t coords_image_stride,
                            const float* targets, const InrLossDesc* loss, int64_t n_pixels, int32_t n_images, void* workspace,
                            int64_t workspace_bytes, StarMap* m, StarDenseWs* w) {
    if (!star || star->n_hidden < 1 || star->n_hidden > STAR_MAX_HIDDEN) return INR_EUNSUPPORTED;
    if (!params || !coords || !targets || !loss || !workspace || n_pixels <= 0 || n_images <= 0) return INR_EINVAL;
    if (coords_image_stride != 0 && coords_image_stride < 2 * n_pixels) return INR_EINVAL;
    if (loss->kind != INR_LOSS_SE && loss->kind != INR_LOSS_BCE) return INR_EINVAL;
    if (loss->weight_mode < INR_WEIGHT_NONE || loss->weight_mode > INR_WEIGHT_EXPLICIT) return INR_EINVAL;
    *m = make_star_map(star->n_hidden);
    *w = carve_star_dense(star->n_hidden, n_pixels, n_images, workspace);
    if (workspace_bytes < w->bytes) return INR_EWORKSPACE;
    return INR_OK;
}

int inrfit_star_loss_grad_dense(const InrStarDesc* star, const float* params, const float* coords, int64_t coords_image_stride,
                                const float* targets, const InrLossDesc* loss, int64_t n_pixels, int32_t n_images, float* loss_out,
                                float* grads, void* workspace, int64_t workspace_bytes, void* stream) {
    StarMap m;
    StarDenseWs w;
    if (!loss_out || !grads) return INR_EINVAL;
    int rc = check_star_dense(star, params, coords, coords_image_stride, targets, loss, n_pixels, n_images, workspace, workspace_bytes, &m, &w);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(loss_coef_kernel, dim3(n_images), dim3(256), 0, s, targets, (long long)n_pixels, *loss, w.coef, 1.f);
    StarDenseUpdArgs u{};
    u.gW1 = w.gW1;
    u.col = w.col;
    u.scal = w.scal;
    u.m = m;
    u.mode = 1;
    for (int img = 0; img < n_images; ++img) {
        const float* prm = params + (size_t)img * m.P;
        if ((rc = star_dense_pass(m, w, prm, coords + (size_t)img * coords_image_stride, targets + (size_t)img * n_pixels, w.coef + 2 * img,
                                  loss->kind, n_pixels, nullptr, true, s)))
            return rc;
        u.grads_out = grads + (size_t)img * m.P;
        u.loss_out = loss_out + img;
        hipLaunchKernelGGL(star_dense_update_kernel, dim3((m.P + 1 + 255) / 256), dim3(256), 0, s, u);
    }
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

int inrfit_star_fit_dense(const InrStarDesc* star, float* params, float* opt_state, const float* coords, int64_t coords_image_stride,
                          const float* targets, const InrLossDesc* loss, const InrOptDesc* opt, int64_t n_pixels, int32_t n_images,
                          int32_t steps, int32_t step0, int32_t offset_first_step, float* loss_hist, float* final_logits, int32_t* status,
                          void* workspace, int64_t workspace_bytes, void* stream) {
    StarMap m;
    StarDenseWs w;
    if (!opt_state || !opt || !status || steps < 0 || step0 < 0) return INR_EINVAL;
    if (opt->kind != INR_OPT_ADAM && opt->kind != INR_OPT_ADAMAX) return INR_EINVAL;
    if (opt->weight_decay != 0.f || opt->clamp || opt->freeze_skips || opt->freeze_input) return INR_EINVAL;   // not part of this prior
    int rc = check_star_dense(star, params, coords, coords_image_stride, targets, loss, n_pixels, n_images, workspace, workspace_bytes, &m, &w);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, sizeof(int32_t) * n_images, s) != hipSuccess) return INR_ELAUNCH;
    hipLaunchKernelGGL(opt_init_kernel, dim3(n_images), dim3(32), 0, s, opt_state, m.P, *opt, (int)step0);
    hipLaunchKernelGGL(loss_coef_kernel, dim3(n_images), dim3(256), 0, s, targets, (long long)n_pixels, *loss, w.coef, 1.f);
    StarDenseUpdArgs u{};
    u.gW1 = w.gW1;
    u.col = w.col;
    u.scal = w.scal;
    u.m = m;
    u.od = *opt;
    u.mode = 0;
    for (int img = 0; img < n_images; ++img) {
        float* prm = params + (size_t)img * m.P;
        const float* xy = coords + (size_t)img * coords_image_stride;
        const float* tg = targets + (size_t)img * n_pixels;
        float* lg = final_logits ? final_logits + (size_t)img * n_pixels : nullptr;
        u.prm = prm;
        u.opt = opt_state + (size_t)img * (2 * (size_t)m.P + INR_OPT_HEADER_FLOATS);
        u.status = status + img;
        for (int it = 0; it < steps; ++it) {
            const int ep = step0 + it;
            const bool gate = lg && opt->logits_at_last_forward && it == steps - 1;
            if ((rc = star_dense_pass(m, w, prm, xy, tg, w.coef + 2 * img, loss->kind, n_pixels, gate ? lg : nullptr, true, s))) return rc;
            const int t_off = star_offset_step(ep, offset_first_step);
            u.t = ep + 1;
            u.net = opt_consts(opt, u.t);
            u.off = opt_consts(opt, t_off);
            u.offset_on = t_off > 0;
            u.loss_hist = loss_hist ? loss_hist + (size_t)img * steps + it : nullptr;
            hipLaunchKernelGGL(star_dense_update_kernel, dim3((m.P + 1 + 255) / 256), dim3(256), 0, s, u);
        }
        if (lg && (!opt->logits_at_last_forward || steps == 0)) {   // the logits at the final parameters: one more forward
            if ((rc = star_dense_pass(m, w, prm, xy, nullptr, nullptr, loss->kind, n_pixels, lg, false, s))) return rc;
        }
    }
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

__global__ __launch_bounds__(256) void debug_tanh_exp_kernel(const float* __restrict__ x, long long n, float* __restrict__ th,
                                                              float* __restrict__ ex) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        th[i] = fast_tanh(x[i]);
        ex[i] = fast_exp(x[i]);
    }
}

int inrfit_debug_tanh_exp(const float* x, int64_t n, float* tanh_out, float* exp_out, void* stream) {
    if (!x || !tanh_out || !exp_out || n <= 0) return INR_EINVAL;
    hipLaunchKernelGGL(debug_tanh_exp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, (long long)n,
                       tanh_out, exp_out);
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

int inrfit_miou(const float* out, const float* tgt, int n_images, int64_t n_points, float thr_out, float thr_tgt, int invert,
                float* iou, void* stream) {
    if (!out || !tgt || !iou || n_images <= 0 || n_points <= 0) return INR_EINVAL;
    hipLaunchKernelGGL(miou_kernel, dim3(n_images), dim3(256), 0, (hipStream_t)stream, out, tgt, (long long)n_points, thr_out,
                       thr_tgt, invert, iou);
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

int inrfit_pack_masks(const float* values, int n_images, int64_t n_points, float threshold, int invert, uint64_t* bits,
                      void* stream) {
    if (!values || !bits || n_images <= 0 || n_points <= 0) return INR_EINVAL;
    const long long words = (n_points + 63) / 64;
    hipLaunchKernelGGL(pack_masks_kernel, dim3((unsigned)((words + 3) / 4), n_images), dim3(256), 0, (hipStream_t)stream, values,
                       (long long)n_points, threshold, invert, (unsigned long long*)bits);
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

#if INR_STAMPS
#pragma GCC visibility push(default)   // diagnostic readers, not in include/inrfit.h: tools/stamps*.py find them by name
int inrfit_debug_updtimes(unsigned long long* host_out) {   // [512][4] of the last update launch
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_updtimes), sizeof(unsigned long long) * 2048) == hipSuccess ? 0 : -4;
}
int inrfit_debug_updissue(unsigned long long* host_out) {   // [512] of the last update launch (absolute, like updtimes[][0])
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_updissue), sizeof(unsigned long long) * 512) == hipSuccess ? 0 : -4;
}
int inrfit_debug_wgfirst(unsigned long long* host_out) {   // [1024] of the last step launch (relative to the workgroup's entry)
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_wgfirst), sizeof(unsigned long long) * 1024) == hipSuccess ? 0 : -4;
}
int inrfit_debug_stamps2(unsigned long long* host_out) {
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_stamps2), sizeof(unsigned long long) * 16) == hipSuccess ? 0 : -4;
}
int inrfit_debug_stamps(unsigned long long* host_out) {
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 16) == hipSuccess ? 0 : -4;
}
int inrfit_debug_wgtimes(unsigned long long* host_out) {   // [1024][4], then cleared for the next launch
    if (hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_wgtimes), sizeof(unsigned long long) * 4096) != hipSuccess) return -4;
    static unsigned long long zeros[4096];
    return hipMemcpyToSymbol(HIP_SYMBOL(g_wgtimes), zeros, sizeof(zeros)) == hipSuccess ? 0 : -4;
}
#pragma GCC visibility pop
#endif

const char* inrfit_strerror(int code) {
    switch (code) {
        case INR_OK: return "ok";
        case INR_EINVAL: return "invalid argument";
        case INR_EUNSUPPORTED: return "model shape has no compiled kernel";
        case INR_EWORKSPACE: return "workspace too small";
        case INR_ELAUNCH: return "HIP launch failed";
        case INR_ENODEVICE: return "no gfx950 device";
        default: return "unknown error";
    }
}

}  // extern "C"


// ---------------------------------------------------------------------------------------------------------------------
// FCNet segmentation step (csrc/fcseg.h)
// ---------------------------------------------------------------------------------------------------------------------
namespace {

struct FcWs {
    int P, blocks;
    long long count;
    float *slab, *loss;
    long long bytes;
};

static bool fc_desc_ok(const InrFcSegDesc* d) {
    return d && d->width == FC_WIDTH && d->depth >= 0 && d->depth <= FC_MAX_DEPTH && d->in_channels >= 1 && d->in_channels <= FC_MAX_IN &&
           d->image_channels >= 0 && d->image_channels <= d->in_channels && d->n_rows >= 1 && d->n_rows < (1LL << 40) &&
           d->data_count >= 0 && d->data_count <= d->n_rows;
}

static long long fc_param_count(const InrFcSegDesc* d) {
    return (long long)fc_b_off(d->in_channels, d->depth, d->depth + 1) + 1;
}

static FcWs fc_layout(const InrFcSegDesc* d, void* base) {
    FcWs w{};
    w.P = (int)fc_param_count(d);
    const long long chunks = (d->n_rows + FC_BLOCK - 1) / FC_BLOCK;
    w.blocks = (int)(chunks < FC_MAX_BLOCKS ? chunks : FC_MAX_BLOCKS);
    w.count = d->data_count > 0 ? d->data_count : d->n_rows;
    w.slab = (float*)base;
    const long long slab_bytes = ((long long)w.blocks * (w.P + 1) * 4 + 255) / 256 * 256;
    w.loss = (float*)((char*)base + slab_bytes);
    w.bytes = slab_bytes + 256;
    return w;
}

static int fc_check(const InrFcSegDesc* d, const float* const* wts, const float* const* bs, const float* image, const float* feat,
                    void* ws, long long ws_bytes, FcWs* w) {
    if (!d || !wts || !bs || !ws) return INR_EINVAL;
    if (!fc_desc_ok(d)) return INR_EUNSUPPORTED;
    if ((d->image_channels > 0 && !image) || (d->image_channels < d->in_channels && !feat)) return INR_EINVAL;
    for (int l = 0; l < d->depth + 2; ++l)
        if (!wts[l] || !bs[l]) return INR_EINVAL;
    *w = fc_layout(d, ws);
    if (ws_bytes < w->bytes) return INR_EWORKSPACE;
    return INR_OK;
}

template <bool BWD>
static void fc_launch_rows(int depth, int blocks, hipStream_t s, const FcArgs& a) {
    const dim3 grid(blocks), block(FC_BLOCK);
    switch (depth) {
        case 0: hipLaunchKernelGGL((fc_rows_kernel<0, BWD>), grid, block, 0, s, a); break;
        case 1: hipLaunchKernelGGL((fc_rows_kernel<1, BWD>), grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL((fc_rows_kernel<2, BWD>), grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL((fc_rows_kernel<3, BWD>), grid, block, 0, s, a); break;
    }
}

static FcArgs fc_args(const FcWs& w, const InrFcSegDesc* d, const float* const* wts, const float* const* bs, const float* image,
                      const float* feat, const float* target, const float* dseg, float* logits, float* seg) {
    FcArgs a{};
    for (int l = 0; l < d->depth + 2; ++l) {
        a.w[l] = wts[l];
        a.b[l] = bs[l];
    }
    a.image = image;
    a.feat = feat;
    a.target = target;
    a.dseg = dseg;
    a.logits = logits;
    a.seg = seg;
    a.slab = w.slab;
    a.n = d->n_rows;
    a.count = w.count;
    a.F = d->in_channels;
    a.ic = d->image_channels;
    a.inversion = d->inversion;
    a.P = w.P;
    a.seed_scale = (float)((double)d->g / (double)w.count);
    return a;
}

}  // namespace

extern "C" {

int64_t inrfit_fcseg_param_count(const InrFcSegDesc* desc) {
    InrFcSegDesc d;
    if (!desc) return -1;
    d = *desc;
    if (d.n_rows < 1) d.n_rows = 1;       // (the count does not depend on the rows)
    if (d.data_count < 0 || d.data_count > d.n_rows) d.data_count = 0;
    return fc_desc_ok(&d) ? fc_param_count(&d) : -1;
}

int64_t inrfit_fcseg_workspace_bytes(const InrFcSegDesc* desc) { return fc_desc_ok(desc) ? fc_layout(desc, nullptr).bytes : -1; }

int inrfit_fcseg_forward(const InrFcSegDesc* desc, const float* const* weights, const float* const* biases, const float* image_rows,
                         const float* feature_rows, const float* target, float* logits, float* seg, float* loss_out, void* workspace,
                         int64_t workspace_bytes, void* stream) {
    FcWs w;
    int rc = fc_check(desc, weights, biases, image_rows, feature_rows, workspace, workspace_bytes, &w);
    if (rc) return rc;
    if (target && !loss_out) return INR_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    FcArgs a = fc_args(w, desc, weights, biases, image_rows, feature_rows, target, nullptr, logits, seg);
    a.P = 0;            // forward: the slab holds the BCE sums only
    a.stride = 1;
    fc_launch_rows<false>(desc->depth, w.blocks, s, a);
    if (target) {
        FcReduceArgs r{w.slab, w.blocks, 1, 0, desc->g, (float)w.count, nullptr, nullptr, loss_out, w.loss};
        hipLaunchKernelGGL(fc_reduce_kernel, dim3(1), dim3(FC_REDUCE_BLOCK), 0, s, r);
    }
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

int inrfit_fcseg_step(const InrFcSegDesc* desc, const float* const* weights, const float* const* biases, const float* image_rows,
                      const float* feature_rows, const float* target, const float* dseg, int reuse_forward, float* logits, float* seg,
                      float* loss_out, float* grads, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream) {
    FcWs w;
    int rc = fc_check(desc, weights, biases, image_rows, feature_rows, workspace, workspace_bytes, &w);
    if (rc) return rc;
    if (!target || !grads || !status) return INR_EINVAL;
    (void)reuse_forward;   // the rows' forward is part of the one step launch either way (include/inrfit.h)
    hipStream_t s = (hipStream_t)stream;
    FcArgs a = fc_args(w, desc, weights, biases, image_rows, feature_rows, target, dseg, logits, seg);
    a.stride = w.P + 1;
    fc_launch_rows<true>(desc->depth, w.blocks, s, a);
    FcReduceArgs r{w.slab, w.blocks, w.P + 1, w.P, desc->g, (float)w.count, grads, status, loss_out, w.loss};
    hipLaunchKernelGGL(fc_reduce_kernel, dim3(1), dim3(FC_REDUCE_BLOCK), 0, s, r);
    return hipGetLastError() == hipSuccess ? INR_OK : INR_ELAUNCH;
}

}  // extern "C"

// ---- the UNet backbone's evaluation pass (csrc/unet.h) ---------------------------------------------------------------------------------
extern "C" {

int64_t inrfit_unet_packed_floats(const InrUNetDesc* desc) {
    const int rc = unet_desc_rc(desc);
    return rc ? rc : unet_plan(desc).packed_floats;
}

int64_t inrfit_unet_workspace_bytes(const InrUNetDesc* desc) {
    const int rc = unet_desc_rc(desc);
    return rc ? rc : unet_plan(desc).bytes;
}

int inrfit_unet_pack(const InrUNetDesc* desc, const float* const* conv_w, const float* const* conv_b, const float* const* bn_gamma,
                     const float* const* bn_beta, const float* const* bn_mean, const float* const* bn_var, float* packed, void* stream) {
    if (!desc || !conv_w || !conv_b || !bn_gamma || !bn_beta || !bn_mean || !bn_var || !packed) return INR_EINVAL;
    for (int i = 0; i < UNET_CONVS; ++i)
        if (!conv_w[i] || !conv_b[i]) return INR_EINVAL;
    for (int i = 0; i < UNET_CONVS - 1; ++i)
        if (!bn_gamma[i] || !bn_beta[i] || !bn_mean[i] || !bn_var[i]) return INR_EINVAL;
    if (((uintptr_t)packed) & 15) return INR_EINVAL;
    const int rc = unet_desc_rc(desc);
    if (rc) return rc;
    return unet_pack(desc, unet_plan(desc), conv_w, conv_b, bn_gamma, bn_beta, bn_mean, bn_var, packed, (hipStream_t)stream);
}

int inrfit_unet_forward(const InrUNetDesc* desc, const float* packed, const float* input, float* logits, void* workspace,
                        int64_t workspace_bytes, void* stream) {
    if (!desc || !packed || !input || !logits || !workspace) return INR_EINVAL;
    if ((((uintptr_t)packed) | ((uintptr_t)workspace)) & 15) return INR_EINVAL;
    const int rc = unet_desc_rc(desc);
    if (rc) return rc;
    const UNetPlan p = unet_plan(desc);
    if (workspace_bytes < p.bytes) return INR_EWORKSPACE;
    return unet_forward(desc, p, packed, input, logits, (float*)workspace, (hipStream_t)stream);
}

}  // extern "C"

// ---- the UNet backbone's training step (csrc/unet_train.h) ------------------------------------------------------------------------------
extern "C" {

int64_t inrfit_unet_param_count(const InrUNetDesc* desc) {
    const int rc = unet_desc_rc(desc);
    return rc ? rc : unet_train_plan(desc).param_count;
}

int64_t inrfit_unet_train_workspace_bytes(const InrUNetDesc* desc) {
    const int rc = unet_train_desc_rc(desc);
    return rc ? rc : unet_train_plan(desc).bytes;
}

int inrfit_unet_train_forward(const InrUNetDesc* desc, const float* const* conv_w, const float* const* conv_b, const float* const* bn_gamma,
                              const float* const* bn_beta, float* const* running_mean, float* const* running_var, float momentum,
                              const float* input, float* logits, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!desc || !conv_w || !conv_b || !bn_gamma || !bn_beta || !running_mean || !running_var || !input || !logits || !workspace)
        return INR_EINVAL;
    for (int i = 0; i < UNET_CONVS; ++i)
        if (!conv_w[i] || !conv_b[i]) return INR_EINVAL;
    for (int i = 0; i < UNET_CONVS - 1; ++i)
        if (!bn_gamma[i] || !bn_beta[i] || !running_mean[i] || !running_var[i]) return INR_EINVAL;
    if (((uintptr_t)workspace) & 15) return INR_EINVAL;
    if (!(momentum >= 0.f && momentum <= 1.f)) return INR_EINVAL;
    const int rc = unet_train_desc_rc(desc);
    if (rc) return rc;
    const UNetTrainPlan t = unet_train_plan(desc);
    if (workspace_bytes < t.bytes) return INR_EWORKSPACE;
    return unet_train_forward(desc, t, conv_w, conv_b, bn_gamma, bn_beta, running_mean, running_var, momentum, input, logits,
                              (float*)workspace, (hipStream_t)stream);
}

int inrfit_unet_train_backward(const InrUNetDesc* desc, const float* const* conv_w, const float* const* conv_b, const float* const* bn_gamma,
                               const float* const* bn_beta, const float* input, const float* dlogits, float* grads, void* workspace,
                               int64_t workspace_bytes, void* stream) {
    if (!desc || !conv_w || !conv_b || !bn_gamma || !bn_beta || !input || !dlogits || !grads || !workspace) return INR_EINVAL;
    for (int i = 0; i < UNET_CONVS; ++i)
        if (!conv_w[i] || !conv_b[i]) return INR_EINVAL;
    for (int i = 0; i < UNET_CONVS - 1; ++i)
        if (!bn_gamma[i] || !bn_beta[i]) return INR_EINVAL;
    if (((uintptr_t)workspace) & 15) return INR_EINVAL;
    const int rc = unet_train_desc_rc(desc);
    if (rc) return rc;
    const UNetTrainPlan t = unet_train_plan(desc);
    if (workspace_bytes < t.bytes) return INR_EWORKSPACE;
    return unet_train_backward(desc, t, conv_w, bn_gamma, input, dlogits, grads, (float*)workspace, (hipStream_t)stream);
}

}  // extern "C"
