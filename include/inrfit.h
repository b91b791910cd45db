/*
 * inrfit.h - C ABI of libinrfit.so: the MI355X (gfx950) implementation of the per-image INR fit hot path of
 * jp-schneider/awesome (dense-grid input-convex coordinate MLP: forward, loss, backward, Adam/Adamax, convexity clamp).
 *
 * The reference has no FFI: its hot path is Python/PyTorch.  Each entry point below states the reference
 * code it replaces (paths relative to the reference checkout).  The binding a maintainer would add on the reference side
 * is a ctypes stub; this repo's own host side is awesome_amd/_lib.py.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (torch tensors' data_ptr()), unless marked "host";
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous w.r.t. the host;
 *   - return value: 0 on success, negative INR_E* for argument/launch errors (synchronous);
 *     per-image numerical failures (NaN/Inf loss) are reported in the `status` device array of inrfit_fit;
 *   - no global mutable state: thread-safe for distinct streams; one process per GPU;
 *   - all arithmetic is fp32 (the reference's AwesomeConfig.dtype default, awesome/run/awesome_config.py:193).
 *
 * Flat parameter vector of the ICNN (ConvexNet == ConvexNextNet(L=1), awesome/model/convex_net.py:10-40,177-220),
 * h = n_hidden, C = in_features, L = n_layers; row-major like the torch state_dict tensors:
 *     input.weight [h][C] | input.bias [h] |
 *     for k in 0..L-1: skip.k.ln.weight [h][h] | skip.k.ln.bias [h] | skip.k.skp.weight [h][C] |
 *     out.ln.weight [h] | out.ln.bias [1] | out.skp.weight [C]
 *   P = h*C + h + L*(h*h + h + h*C) + h + 1 + C            (17813 for h=130, C=2, L=1)
 * General form (ABI 8), F = n_features or h, O = n_out or 1 - the coordinate MLPs of the notebooks (an encode stage of F features, L relu
 * layers of h units, O outputs):
 *     input.weight [F][C] | input.bias [F] | skip.0.ln.weight [h][F] | skip.0.ln.bias [h] | skip.0.skp.weight [h][C] |
 *     for k in 1..L-1: skip.k.ln.weight [h][h] | skip.k.ln.bias [h] | skip.k.skp.weight [h][C] |
 *     out.ln.weight [O][h] | out.ln.bias [O] | out.skp.weight [O][C]          (L = 0: out.ln.weight [O][F], read from the features)
 *   P = F*C + F + (L > 0 ? (h*F + h + h*C) + (L-1)*(h*h + h + h*C) : 0) + O*(L > 0 ? h : F) + O + O*C   (256269 for h=350, C=2, L=3, F=20, O=3)
 * With F = h and O = 1 this is the layout above.  Support: 1 <= F <= 1024, 1 <= O <= 4; L = 0 only with a periodic layer 0 (INR_ACT_COS /
 * INR_ACT_SIN).  A shape with F != h, O > 1 or L = 0 runs on the layer-by-layer path only; the composite priors (cdn_*, pcn_*), the joint
 * steps and inrfit_step_only return INR_EUNSUPPORTED for it.  With O > 1, logits, targets and dlogits are [n_images][O][n_points]
 * (channel-planar like the coordinates); the data term is averaged over O * n_points (torch's MSELoss on (N, O)) and takes weight_mode
 * INR_WEIGHT_NONE or INR_WEIGHT_EXPLICIT only (others: INR_EINVAL).
 */
#ifndef INRFIT_H
#define INRFIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: exactly the declarations between this push and the pop at the end of the file are
 * exported (nm -D shows the inrfit_* entry points and nothing else of the library's own). */
#pragma GCC visibility push(default)

#define INRFIT_ABI_VERSION 8

enum {
    INR_OK = 0,
    INR_EINVAL = -1,      /* bad argument (null pointer, non-positive size, unknown enum) */
    INR_EUNSUPPORTED = -2,/* model shape not built into this library (see inrfit_query / inrfit_supported) */
    INR_EWORKSPACE = -3,  /* workspace too small */
    INR_ELAUNCH = -4,     /* HIP launch failure (hipGetLastError) */
    INR_ENODEVICE = -5    /* no gfx950 device / wrong architecture */
};

enum { INR_MODEL_ICNN = 1 };
enum { INR_GRID_SEPARABLE = 0, INR_GRID_EXPLICIT = 1 };
enum { INR_LOSS_SE = 0, INR_LOSS_BCE = 1, INR_LOSS_EXTERNAL = 2 /* inrfit_backward only: dL/dlogit supplied */ };
enum { INR_WEIGHT_NONE = 0, INR_WEIGHT_EQUAL = 1, INR_WEIGHT_RATIO = 2, INR_WEIGHT_SSSDMS = 3, INR_WEIGHT_EXPLICIT = 4 };
enum { INR_OPT_ADAM = 0, INR_OPT_ADAMAX = 1 };
enum { INR_STATUS_OK = 0, INR_STATUS_NONFINITE = 1 };

/* Activation of layer 0 = the ENCODE stage of the coordinate network (the hidden skip layers are always relu):
 *   INR_ACT_RELU  z0 = relu(W_in x + b_in)                  the packaged models (convex_net.py:205-214; FCNet)
 *   INR_ACT_COS   z0 = cos(W_in x + b_in)                   random Fourier features cos(x @ A + b) with W_in = A^T, b_in = b
 *                                                           frozen (InrOptDesc.freeze_input) - notebooks/imageRepresentationTest.ipynb
 *                                                           cell 5, `ourSimpleNetwork` (features -> relu layers -> sigmoid)
 *   INR_ACT_SIN   z0 = sin(act_omega (W_in x + b_in))       learnable sine layer, act_omega = 10 pi in
 *                                                           notebooks/icml_teaser_code/repeating/repeating.ipynb cell 3 (`myNet`)
 * Evaluated in registers where relu is (the D tile of the layer-0 MFMA); sin / cos are v_sin_f32 / v_cos_f32 after a v_fract_f32
 * range reduction (|argument| <~ 1e3: absolute error <~ 1e-5).  The coordinate-gradient (DX) kernels exist for relu only. */
enum { INR_ACT_RELU = 0, INR_ACT_COS = 1, INR_ACT_SIN = 2 };

/* awesome/model/convex_net.py:177-203 constructor arguments (n_hidden, in_features, n_hidden_layers). */
typedef struct InrModelDesc {
    int32_t kind;        /* INR_MODEL_ICNN */
    int32_t n_hidden;    /* h */
    int32_t in_features; /* C: 2 (x,y) or 3 (x,y,t) */
    int32_t n_layers;    /* L hidden skip layers (ConvexNet: 1) */
    int32_t act0;        /* INR_ACT_* (0 = relu: a zero-initialised tail keeps old callers' meaning) */
    float act_omega;     /* INR_ACT_SIN only */
    int32_t n_features;  /* F: width of layer 0 (the encode stage), 1..1024; 0 = n_hidden (ABI 8; zero tail = ABI 7 meaning) */
    int32_t n_out;       /* O: output channels, 1..4; 0 = 1 (ABI 8) */
} InrModelDesc;

/* The dense coordinate grid every image is evaluated on.
 * SEPARABLE: point p = row*width + col has coords (xs[col], ys[row][, ts[image]]) - the layout produced by
 *            Transformator.get_positional_matrices (awesome/dataset/transformator.py:25-61) and the how-to grid
 *            (notebooks/how_to/convexity.ipynb cell 7); xs/ys are tiny 1-D arrays so their values are exactly the
 *            caller's (torch.linspace / arange/n), nothing is re-derived in the kernel.
 * EXPLICIT:  coords is channel-planar [C][n_points] per image (the (B,C,H,W) tensor the reference feeds through
 *            @pixelize, awesome/util/pixelize.py:31-33); image i starts at coords + i*coords_image_stride
 *            (stride 0 = one grid shared by all images). */
typedef struct InrGridDesc {
    int32_t mode;
    int32_t width, height;
    int64_t n_points; /* width*height for SEPARABLE */
    const float* xs;  /* [width]  */
    const float* ys;  /* [height] */
    const float* ts;  /* [n_images] or NULL (C == 2) */
    const float* coords;
    int64_t coords_image_stride; /* in floats */
} InrGridDesc;

/* Data term on sigmoid(logit) vs. unaries: SE (awesome/measures/se.py:21-23) or BCE (torch.nn.BCELoss), 'mean'
 * reduction, optionally re-weighted per class as UnariesWeightedLoss._compute_weight does
 * (awesome/measures/unaries_weighted_loss.py:35-69; weight applies to target < 0.5).
 * EXPLICIT: per-element coefficient is c_fg (target < 0.5) or c_bg, normalisation included - expresses the how-to
 * loop's (1-w)*mean_bg + w*mean_fg (notebooks/how_to/convexity.ipynb cell 9). */
typedef struct InrLossDesc {
    int32_t kind;
    int32_t weight_mode;
    float ratio;
    float c_fg, c_bg;
} InrLossDesc;

/* torch.optim.Adam / Adamax defaults (awesome/run/awesome_config.py:34-41; path_connected_net.py:924-929),
 * enforce_convexity after every step (convex_net.py:216-220; hook awesome/run/awesome_runner.py:294-297),
 * ReduceLROnPlateau(mode='min', rel threshold) stepped with the loss every step (path_connected_net.py:932-933,951). */
typedef struct InrOptDesc {
    int32_t kind;
    float lr, beta1, beta2, eps, weight_decay;
    int32_t clamp;
    int32_t plateau;
    int32_t plateau_patience;
    float plateau_factor, plateau_threshold, plateau_min_lr, plateau_eps;
    int32_t freeze_skips; /* 1: no skp.weight (incl. out.skp) is ever updated.  With zero skips and clamp = 0 the ICNN is the plain
                             relu MLP Linear(C,h) [Linear(h,h)]xL Linear(h,1) = FCNet(in_type='xy') (awesome/model/fc_net.py:10-59),
                             the "no prior" coordinate network of configs[0]. */
    int32_t freeze_input; /* 1: input.weight / input.bias are never updated: fixed random Fourier features (buffers A, b of
                             `ourSimpleNetwork`, imageRepresentationTest.ipynb cell 5). */
    int32_t logits_at_last_forward; /* 1: `final_logits` of the fit calls = the output of the LAST training forward, i.e. at the
                             parameters before the last optimizer step - the tensor the reference's IoU gate reads
                             (device_prior_output, path_connected_net.py:939-972; convex_diffeomorphism_net.py:405-438) - written
                             by that step's launch (no extra forward launch).  0: logits at the final parameters. */
} InrOptDesc;

/* Per-image optimizer state, `opt_state` = n_images * inrfit_opt_state_floats(model) floats:
 *   exp_avg [P] | exp_avg_sq or exp_inf [P] | header [INR_OPT_HEADER_FLOATS]
 * header: [0],[1] lr of odd/even steps (double buffer, internal), [2] current lr, [3] plateau best,
 *         [4] plateau num_bad (as float), [5] last loss, [6],[7] "frozen by a non-finite loss" flag of odd/even steps
 *         (double buffer, internal; cleared at the start of every fit call, like `status`).
 * Zero-initialise for a cold fit (step0 == 0 takes lr from InrOptDesc and resets the plateau state;
 * step0 > 0 continues from header[2..4]). */
#define INR_OPT_HEADER_FLOATS 8

/* Capabilities. max_hidden: largest n_hidden any built kernel supports; lds_bytes: LDS used by the h=130 kernel. */
int inrfit_query(int* abi_version, int* max_hidden, int* lds_bytes);
/* Static, host string: ABI version, target, the slab base and the compiler + code-generation flags this binary was built
 * with (awesome_amd/build.py passes them in).  The fit is a chaotic iteration: two builds whose VALU arithmetic rounds
 * differently (e.g. another fused-multiply-add contraction) end a 2000-step fit a few mask pixels apart, so bench.py prints
 * this string next to the parameter checksum.  The library is built with -ffp-contract=off: every fma is an explicit fmaf. */
const char* inrfit_build_info(void);
/* Gradient slabs (= workgroups) one image gets in a launch of n_images images over n_points points: min(256 / n_images, chunks),
 * at least 1.  A constant of the library (NOT the device's CU count), because it fixes the summation order of the gradients. */
int inrfit_slabs_per_image(int64_t n_points, int n_images);
/* Test / measurement hook: replace the 256 above (0 = default).  Process-global; not for production use - it changes the
 * rounding of every gradient sum and therefore the trajectory of a fit (tests/test_gpu_determinism.py bounds by how much). */
int inrfit_debug_set_slab_base(int slab_base);
/* 1 if (h, C, L) has a compiled kernel, else 0. */
int inrfit_supported(const InrModelDesc* model);
int64_t inrfit_param_count(const InrModelDesc* model);
int64_t inrfit_opt_state_floats(const InrModelDesc* model);
/* Scratch every compute call needs (parameter images in LDS layout, per-workgroup gradient slabs each followed by the workgroups'
 * loss partials as a dense array, loss coefficients). */
int64_t inrfit_workspace_bytes(const InrModelDesc* model, const InrGridDesc* grid, int n_images);

/* logits[n_images][n_points] = f_theta(grid).  Replaces ConvexNet/ConvexNextNet.forward
 * (awesome/model/convex_net.py:26-35, 205-214) incl. the @pixelize reshapes, for n_images parameter sets at once
 * (the PriorCache axis, awesome/util/prior_cache.py:49-59). */
int inrfit_forward(const InrModelDesc* model, const float* params, const InrGridDesc* grid, int n_images,
                   float* logits, void* workspace, int64_t workspace_bytes, void* stream);

/* loss_out[n_images], grads[n_images][P] (same flat order as params) of the data term at `params`.
 * Replaces one forward + criterion + loss.backward() of the hot loop (awesome/model/path_connected_net.py:941-948;
 * awesome/agent/torch_agent.py:470-491) - used by the autograd.Function bridge so the stock training loop still works. */
int inrfit_loss_grad(const InrModelDesc* model, const float* params, const InrGridDesc* grid, const float* targets,
                     const InrLossDesc* loss, int n_images, float* loss_out, float* grads, void* workspace,
                     int64_t workspace_bytes, void* stream);

/* grads[n_images][P] = sum_p dlogits[image][p] * d logit_p / d params: the vector-Jacobian product of the forward
 * (forward is recomputed, nothing is saved).  Replaces autograd's backward through ConvexNextNet.forward for an
 * arbitrary downstream criterion (AwesomeImageLoss, FBMSJointLoss, ... - awesome/agent/torch_agent.py:478-491).
 * dcoords (optional, may be NULL) [n_images][C][n_points]: dlogits[p] * d logit_p / d coords_p - the gradient that flows
 * on into a learned deformation of the grid (ConvexDiffeomorphismNet.forward, awesome/model/convex_diffeomorphism_net.py:
 * 173-178: ICNN(flow(Ax+b))).  Shapes with a fused kernel: relu layer 0 only; the layer-by-layer shapes (n_hidden > 130 or more than
 * two hidden layers): any layer-0 activation. */
int inrfit_backward(const InrModelDesc* model, const float* params, const InrGridDesc* grid, const float* dlogits,
                    int n_images, float* grads, float* dcoords, void* workspace, int64_t workspace_bytes, void* stream);

/* `steps` full-batch optimisation steps of n_images independent fits, entirely on device:
 *   E x { forward, loss, backward, Adam/Adamax step, clamp, plateau.step(loss) }
 * Replaces the inner loops of _prior_based_pretrain (awesome/model/path_connected_net.py:937-962), the how-to loop
 * (notebooks/how_to/convexity.ipynb cell 9) and learn_convex_net (path_connected_net.py:364-379).
 * params/opt_state are updated in place; step0 = number of optimizer steps already taken (bias correction);
 * loss_hist (optional) [n_images][steps]: loss at the parameters BEFORE each step, as the reference logs it;
 * final_logits (optional) [n_images][n_points]: logits at the final parameters; status [n_images] int32. */
int inrfit_fit(const InrModelDesc* model, float* params, float* opt_state, const InrGridDesc* grid, const float* targets,
               const InrLossDesc* loss, const InrOptDesc* opt, int n_images, int steps, int step0, float* loss_hist,
               float* final_logits, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);

/* iou[n_images]: binary Jaccard of the class selected by `invert` between (out > thr_out) and (tgt > thr_tgt);
 * 0 if the target has no member of that class.  Replaces MIOU(invert=True, average='binary')
 * (awesome/measures/miou.py:29-48) and the IoU gate of the fit loop (path_connected_net.py:964-972). */
int inrfit_miou(const float* out, const float* tgt, int n_images, int64_t n_points, float thr_out, float thr_tgt, int invert,
                float* iou, void* stream);

/* bits[n_images][ceil(n_points/64)]: (values > threshold) - or its complement with `invert` - one bit per point, LSB = lowest
 * index.  The on-device form of the mask export after evaluation (awesome/run/functions.py:2315-2361 save_result_mask writes
 * `prior > 0.5` as an image): 8 KB instead of 256 KB leave the device per 256x256 mask. */
int inrfit_pack_masks(const float* values, int n_images, int64_t n_points, float threshold, int invert, uint64_t* bits,
                      void* stream);

/* ---- path-connected prior: ICNN(flow(Ax + b)), ConvexDiffeomorphismNet (awesome/model/convex_diffeomorphism_net.py:130-188)
 * with the weight-normalised coupling flow NormalizingFlow1D(backbone='normal_block') of awesome/model/diffeomorphism_net.py:
 * 169-302 (2-D grids only, like the reference).  Flat flow parameter vector (W = width, K = num_coupling):
 *     linear.weight [2][2] | linear.bias [2] |
 *     for i in 0..K-1, for net in (s, t):  in_linear weight_v [W] | weight_g | bias [W] | out_linear weight_v [W] | weight_g | bias
 *     for i in 0..K-1 (WNScale):  weight | scale.bias | scale.weight_g | scale.weight_v
 *   FP = 6 + 2K(3W + 3) + 4K.   flow_opt_state = n_images * 2 * FP floats (exp_avg | exp_avg_sq), zero for a cold fit.
 * The ICNN behind the flow: a shape with a fused kernel, or an ICNN-form shape of the layer-by-layer path (relu layer 0, one output,
 * n_features = n_hidden, n_hidden <= 1024, n_layers <= 8) with in_features = 2 - inrfit_cdn_workspace_bytes / _forward / _loss_grad /
 * _fit take both under the same names and semantics (the flow's kernels run all images in one launch, a layer-by-layer ICNN one image
 * after the other in one image's workspace).  inrfit_cdn_joint_step and inrfit_cdn_fit_minibatch take the fused shapes only; the
 * others go to inrfit_cdn_wide_joint_step and inrfit_cdn_wide_fit_minibatch. */
enum { INR_FLOW_NORMAL_BLOCK = 0, /* NormalBlock: tanh(WN2 leaky_relu(WN1 u)), keys in_linear / out_linear (diffeomorphism_net.py:169-192;
                                     backbone 'normal_block' / 'residual_block' - every reference config) */
       INR_FLOW_SIMPLE = 1        /* SimpleBackbone: tanh(WN2 relu(WN1 u)), keys linear1 / linear2 (:83-104; NormalizingFlow1D's
                                     'default' backbone, i.e. what ConvexDiffeomorphismNet() builds without diffeo_args) */ };
typedef struct InrFlowDesc {
    int32_t width;        /* W <= 256 */
    int32_t num_coupling; /* K in {2, 4, 6, 8} */
    int32_t backbone;     /* INR_FLOW_NORMAL_BLOCK | INR_FLOW_SIMPLE: same flat parameter layout, the hidden activation differs */
} InrFlowDesc;

int64_t inrfit_flow_param_count(const InrFlowDesc* flow);
int64_t inrfit_cdn_workspace_bytes(const InrModelDesc* model, const InrFlowDesc* flow, const InrGridDesc* grid, int n_images);
/* out_coords[n_images][2][n_points] = flow(A x + b): ConvexDiffeomorphismNet.get_deformation (:179-184). */
int inrfit_flow_forward(const InrFlowDesc* flow, const float* flow_params, const InrGridDesc* grid, int n_images,
                        float* out_coords, void* workspace, int64_t workspace_bytes, void* stream);
/* flow_grads[n_images][FP] = sum_p dout_coords[image][c][p] * d out_coords / d flow_params: the vector-Jacobian product of
 * inrfit_flow_forward (autograd's backward through NormalizingFlow1D.forward o Linear, diffeomorphism_net.py:286-300; the forward
 * is recomputed from the grid, nothing is saved).  dout_coords [n_images][2][n_points]. */
int inrfit_flow_backward(const InrFlowDesc* flow, const float* flow_params, const InrGridDesc* grid, const float* dout_coords,
                         int n_images, float* flow_grads, void* workspace, int64_t workspace_bytes, void* stream);
/* logits[n_images][n_points] = ICNN(flow(A x + b)): ConvexDiffeomorphismNet.forward (:173-178). */
int inrfit_cdn_forward(const InrModelDesc* model, const InrFlowDesc* flow, const float* icnn_params, const float* flow_params,
                       const InrGridDesc* grid, int n_images, float* logits, void* workspace, int64_t workspace_bytes,
                       void* stream);
/* loss and the gradient w.r.t. every parameter (ICNN flat order, flow flat order) of the data term. */
int inrfit_cdn_loss_grad(const InrModelDesc* model, const InrFlowDesc* flow, const float* icnn_params,
                         const float* flow_params, const InrGridDesc* grid, const float* targets, const InrLossDesc* loss,
                         int n_images, float* loss_out, float* icnn_grads, float* flow_grads, void* workspace,
                         int64_t workspace_bytes, void* stream);
/* `steps` full-batch steps of ConvexDiffeomorphismNet.pretrain's inner loop (:405-430): forward, criterion, backward,
 * Adam over the parameter groups of get_weight_normalized_param_groups (awesome/util/torch.py:19-35: weight decay
 * `wd_on_weight_g` on every *weight_g, none elsewhere; opt->kind must be INR_OPT_ADAM), ReduceLROnPlateau, enforce_convexity. */
int inrfit_cdn_fit(const InrModelDesc* model, const InrFlowDesc* flow, float* icnn_params, float* flow_params,
                   float* icnn_opt_state, float* flow_opt_state, const InrGridDesc* grid, const float* targets,
                   const InrLossDesc* loss, const InrOptDesc* opt, float wd_on_weight_g, int n_images, int steps, int step0,
                   float* loss_hist, float* final_logits, int32_t* status, void* workspace, int64_t workspace_bytes,
                   void* stream);

/* ---- path-connected prior with the RealNVP deformation: PathConnectedNet.forward (awesome/model/path_connected_net.py:79-85)
 * as built by real_nvp_path_connected_net (awesome/model/net_factory.py:124-175):
 *     ICNN( MinMax^-1( RealNVP( MinMax( a (.) x + b ) ) ) ),   C = 2 (x, y) or 3 (x, y, t)
 * RealNVP = n_flows x [ MaskedAffineFlow(mask_f, t = MLP[C, hid, C], s = MLP[C, hid, C]), ActNorm(C) ] from the third-party
 * package normflows==1.7.3 (net_factory.py:70-114), which is NOT in the reference checkout: the kernels restate its published
 * definitions (awesome_amd/csrc/rnvp.h) - parity for this variant is UNPINNED.
 * masks[f]: bit c set = channel c passes through flow f unchanged and feeds its MLPs (net_factory.py:86-99 counts 1 .. 2^C-2
 * in binary, LSB = channel 0).  vmin/vmax/new_min/new_max: the fitted MinMax buffers (awesome/transforms/min_max.py:22-58).
 * Flat flow parameter vector (C, hid = hidden_units, F = n_flows):
 *     linear.weight [C] | linear.bias [C] |
 *     for f in 0..F-1:  for net in (s, t):  net.0.weight [hid][C] | net.0.bias [hid] | net.2.weight [C][hid] | net.2.bias [C]
 *                       then ActNorm  s [C] | t [C]
 *   RP = 2C + F (2 (2 hid C + hid + C) + 2C).   flow_opt_state = n_images * 2 * RP floats, zero for a cold fit. */
#define INR_RNVP_MAX_FLOWS 32
typedef struct InrRnvpDesc {
    int32_t channels;      /* C in {2, 3}; equals the ICNN's in_features */
    int32_t hidden_units;  /* hid <= 256 (and F * (8 hid + 12) floats must fit the 160 KB of LDS) */
    int32_t n_flows;       /* F <= 32 */
    int32_t output_fn;     /* 0 = none, 1 = tanh (flow_output_fn) */
    float output_scale;    /* flow_output_scale; 0 or 1 = none */
    float vmin[3], vmax[3];
    float new_min, new_max;
    uint32_t masks[INR_RNVP_MAX_FLOWS];
} InrRnvpDesc;

int64_t inrfit_rnvp_param_count(const InrRnvpDesc* rnvp);
int64_t inrfit_pcn_workspace_bytes(const InrModelDesc* model, const InrRnvpDesc* rnvp, const InrGridDesc* grid, int n_images);
/* ActNorm's data-dependent initialisation (first forward of nf.flows.ActNorm): flow after flow, s = -log(std + 1e-6),
 * t = -mean * exp(s) over all points of the image; writes the ActNorm entries of flow_params in place. */
int inrfit_rnvp_actnorm_init(const InrRnvpDesc* rnvp, float* flow_params, const InrGridDesc* grid, int n_images,
                             void* workspace, int64_t workspace_bytes, void* stream);
/* out_coords[n_images][C][n_points]: PathConnectedNet.get_deformation (path_connected_net.py:124-128). */
int inrfit_rnvp_forward(const InrRnvpDesc* rnvp, const float* flow_params, const InrGridDesc* grid, int n_images,
                        float* out_coords, void* workspace, int64_t workspace_bytes, void* stream);
/* The vector-Jacobian product of inrfit_rnvp_forward (the forward is recomputed inside, as inrfit_backward does for the ICNN):
 * dout_coords [n_images][C][n_points], planar like out_coords -> flow_grads [n_images][RP] in the flat flow layout (linear.weight /
 * linear.bias included) and, when din_coords is not NULL, d / d input coordinates [n_images][C][n_points] (through MinMax and the
 * 1x1 linear).  With inrfit_backward(dcoords) this is the autograd bridge of get_deformation -> ConvexNextNet compositions.
 * Workspace: inrfit_pcn_workspace_bytes(NULL, rnvp, grid, n_images). */
int inrfit_rnvp_backward(const InrRnvpDesc* rnvp, const float* flow_params, const InrGridDesc* grid, const float* dout_coords,
                         int n_images, float* flow_grads, float* din_coords, void* workspace, int64_t workspace_bytes, void* stream);
/* out_coords[n_images][C][n_points] = linear^-1(flow_net^-1(in_coords)): PathConnectedNet.inverse (path_connected_net.py:87-122).
 * in_coords is channel-planar [C][n_points] per image; in_image_stride (floats) = 0 shares one input among all images. */
int inrfit_rnvp_inverse(const InrRnvpDesc* rnvp, const float* flow_params, const float* in_coords, int64_t in_image_stride,
                        int64_t n_points, int n_images, float* out_coords, void* workspace, int64_t workspace_bytes, void* stream);
/* `steps` steps of PathConnectedNet.learn_flow_identity (path_connected_net.py:155-250): Adamax/Adam on the flow_net parameters
 * only (weight decay opt->weight_decay, constant lr; the 1x1 linear is not part of this model) for the loss
 * SE('mean')(flow_net(x), x) on the grid x.  loss_hist (optional) [n_images][steps]. */
int inrfit_rnvp_fit_identity(const InrRnvpDesc* rnvp, float* flow_params, float* flow_opt_state, const InrGridDesc* grid,
                             const InrOptDesc* opt, int n_images, int steps, int step0, float* loss_hist, void* workspace,
                             int64_t workspace_bytes, void* stream);
/* logits[n_images][n_points]: PathConnectedNet.forward (:79-85).
 * ICNN shapes of inrfit_pcn_forward / _loss_grad / _fit / _workspace_bytes: every shape with a fused kernel, and every ICNN-form
 * shape of the layer-by-layer path (n_hidden > 130 or more than two hidden layers; relu layer 0, one output, n_features = n_hidden):
 * there one optimizer step is the RealNVP forward, the layer-by-layer forward / backward on the deformed coordinates (which also
 * returns dL/dcoords), the ICNN update, the RealNVP backward seeded from dL/dcoords and the RealNVP update - all on the stream, same
 * semantics (one learning rate from the ICNN header, a non-finite loss freezes both halves of the image).  The encode shapes and
 * n_hidden > 1024 stay INR_EUNSUPPORTED; inrfit_pcn_joint_step takes the fused shapes only (the others: inrfit_pcn_wide_joint_step). */
int inrfit_pcn_forward(const InrModelDesc* model, const InrRnvpDesc* rnvp, const float* icnn_params, const float* flow_params,
                       const InrGridDesc* grid, int n_images, float* logits, void* workspace, int64_t workspace_bytes,
                       void* stream);
int inrfit_pcn_loss_grad(const InrModelDesc* model, const InrRnvpDesc* rnvp, const float* icnn_params,
                         const float* flow_params, const InrGridDesc* grid, const float* targets, const InrLossDesc* loss,
                         int n_images, float* loss_out, float* icnn_grads, float* flow_grads, void* workspace,
                         int64_t workspace_bytes, void* stream);
/* `steps` full-batch steps of _prior_based_pretrain's inner loop (path_connected_net.py:937-962) for PathConnectedNet:
 * Adamax (or Adam) over the groups of :922-929 - `flow_weight_decay` on every flow_net parameter, none on the ICNN and the
 * 1x1 linear - ReduceLROnPlateau on the loss, enforce_convexity. */
int inrfit_pcn_fit(const InrModelDesc* model, const InrRnvpDesc* rnvp, float* icnn_params, float* flow_params,
                   float* icnn_opt_state, float* flow_opt_state, const InrGridDesc* grid, const float* targets,
                   const InrLossDesc* loss, const InrOptDesc* opt, float flow_weight_decay, int n_images, int steps, int step0,
                   float* loss_hist, float* final_logits, int32_t* status, void* workspace, int64_t workspace_bytes,
                   void* stream);

/* ---- sequence pretraining: ONE network over the T frames of a sequence, trained in mini-batches of `batch_size` frames
 * (PathConnectedNet._non_prior_based_pretrain, awesome/model/path_connected_net.py:634-713, and the mini-batched learn_flow_identity,
 * :200-236), all epochs in one call: plain stream launches, nothing is read on the host in between.
 * frame_coords [T][C][HW] (channel-planar per frame), frame_targets [T][HW]; order: HOST array [num_epochs][T] of int32 frame ids, one
 * permutation of 0..T-1 per epoch (torch's DataLoader order).  It is validated on the host before the first launch - an entry outside
 * [0, T) or a row that is no permutation: INR_EINVAL - and the ids reach the gather kernel as launch arguments, never through memory.
 * Epoch e takes the batches order[e][0:b], order[e][b:2b], ... (b = min(batch_size, T); the last one may be shorter: its step runs on
 * its own points and its mean loss is over them).  Per batch: the frames are gathered into a staging grid [C][b HW] and staging
 * targets, then exactly what inrfit_pcn_fit(steps = 1, step0 = number of steps so far) launches for that explicit grid.  Per epoch:
 * epoch_loss[e] (device, [num_epochs]) = sum over the batches, in batch order, of loss_b / n_batches in fp32, and - with opt->plateau -
 * torch's ReduceLROnPlateau(mode 'min', relative threshold) stepped with it, comparisons and learning rate in double; the learning
 * rate goes to the ICNN header ([2] and the slot of the next step), which both halves of the update read.  schedule: NULL, or a HOST
 * array of 5 doubles {lr, factor, threshold, min_lr, eps} that replaces opt's float fields in the scheduler's arithmetic (a Python
 * loop carries them as doubles: 0.1 is not a float), lr being the learning rate the fit starts with.  step0 must be 0 (else INR_EINVAL): a sequence fit is a cold
 * fit - the header keeps the scheduler's `best` in fp32, so a continued call would not be the uninterrupted one; opt_state is left as
 * inrfit_pcn_fit leaves it.  inrfit_rnvp_fit_identity_sequence has no scheduler and continues with step0 = steps taken so far.
 * A non-finite batch loss freezes the network at the parameters in front of that step for the rest of the call and sets status[0].
 * ICNN shapes: those with a fused kernel (the layer-by-layer shapes: INR_EUNSUPPORTED).  model = NULL in the size query: the
 * workspace of inrfit_rnvp_fit_identity_sequence. */
int64_t inrfit_pcn_sequence_workspace_bytes(const InrModelDesc* model, const InrRnvpDesc* rnvp, int64_t HW, int T, int batch_size);
int inrfit_pcn_fit_sequence(const InrModelDesc* model, const InrRnvpDesc* rnvp, float* icnn_params, float* flow_params,
                            float* icnn_opt_state, float* flow_opt_state, const float* frame_coords, const float* frame_targets,
                            const int32_t* order, int T, int64_t HW, int batch_size, int num_epochs, const InrLossDesc* loss,
                            const InrOptDesc* opt, const double* schedule, float flow_weight_decay, int step0, float* epoch_loss,
                            int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);
/* The same skeleton over inrfit_rnvp_fit_identity's step (flow parameters only, constant learning rate opt->lr, weight decay
 * opt->weight_decay): learn_flow_identity over DataLoader(TensorDataset(x, x), batch_size, shuffle) with x = frame_coords.
 * loss_hist [num_epochs] (device): the LAST batch's loss of every epoch, as the reference records it (:234). */
int inrfit_rnvp_fit_identity_sequence(const InrRnvpDesc* rnvp, float* flow_params, float* flow_opt_state, const float* frame_coords,
                                      const int32_t* order, int T, int64_t HW, int batch_size, int num_epochs, const InrOptDesc* opt,
                                      int step0, float* loss_hist, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- pixel-minibatch fits: a coordinate net trained on a fresh subset of a pixel pool at every optimizer step (the teaser notebooks'
 * loops: convex.ipynb cell 3, repeating.ipynb cell 4, diffeo_convex.ipynb cells 9-11, the DataLoader loop of
 * imageRepresentationTest.ipynb cell 6), all steps in one call: plain stream launches, nothing is read on the host in between and no
 * call synchronises.
 * pool_coords [C][n_pool] (channel-planar) and the index table are shared by all n_images nets; pool_targets [n_images][O][n_pool].
 * index: DEVICE array [steps][batch] of int32 pixel numbers (drawn on the device; thousands per step, so they do not travel as launch
 * arguments).  Every entry is clamped into [0, n_pool) before use.  counts: HOST array [steps], the points of step k (1..batch: the
 * DataLoader's short last batch takes the first counts[k] entries of its row), or NULL: every step takes `batch`.
 * Step k: the pool is gathered by index[k][0:counts[k]] into a staging grid [C][counts[k]] and staging targets
 * [n_images][O][counts[k]]; the loss coefficients are taken on the staging targets; then exactly what inrfit_fit(steps = 1, step0 =
 * step0 + k) - inrfit_cdn_fit for the flow variant - launches for that explicit grid: the same kernels, launch shapes and slab counts.
 * The optimizer header (learning-rate double buffer, plateau state), the parameters and the "frozen" flag carry over a change of
 * count, so a finite run ends bit for bit where the per-step host loop ends.  A non-finite batch loss freezes the net at the
 * parameters in front of that step for the rest of the call and sets status (loss_hist[k] keeps the non-finite value): inrfit_fit's
 * semantics inside one call.  loss_hist [n_images][steps] or NULL.  There are no final logits: inference over all pixels is
 * inrfit_forward / inrfit_cdn_forward.  Shapes: everything inrfit_fit / inrfit_cdn_fit take.  The workspace holds the staging buffers
 * and the step's own workspace for every count in 1..batch (a host computation; flow = NULL: inrfit_fit_minibatch's).
 * Checks, every one before the first HIP call: INR_EINVAL (a null pointer, n_pool / batch / n_images <= 0, steps / step0 < 0, a count
 * outside 1..batch, the optimizer, the loss, INR_LOSS_EXTERNAL), then INR_EUNSUPPORTED (the shape), then INR_EWORKSPACE. */
int64_t inrfit_minibatch_workspace_bytes(const InrModelDesc* model, const InrFlowDesc* flow, int64_t batch, int n_images);
int inrfit_fit_minibatch(const InrModelDesc* model, float* params, float* opt_state, const float* pool_coords,
                         const float* pool_targets, int64_t n_pool, const int32_t* index, const int32_t* counts, int64_t batch,
                         const InrLossDesc* loss, const InrOptDesc* opt, int n_images, int steps, int step0, float* loss_hist,
                         int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);
int inrfit_cdn_fit_minibatch(const InrModelDesc* model, const InrFlowDesc* flow, float* icnn_params, float* flow_params,
                             float* icnn_opt_state, float* flow_opt_state, const float* pool_coords, const float* pool_targets,
                             int64_t n_pool, const int32_t* index, const int32_t* counts, int64_t batch, const InrLossDesc* loss,
                             const InrOptDesc* opt, float weight_decay_on_weight_g, int n_images, int steps, int step0,
                             float* loss_hist, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);
/* inrfit_cdn_fit_minibatch takes the ICNN shapes with a fused kernel.  The pair below is the same call, with the same checks in the
 * same order, for the flow over an ICNN of the layer-by-layer path (ICNN-form, no fused kernel, in_features = 2: the shapes
 * inrfit_cdn_fit takes beyond the fused ones); every other shape: INR_EUNSUPPORTED. */
int64_t inrfit_cdn_wide_minibatch_workspace_bytes(const InrModelDesc* model, const InrFlowDesc* flow, int64_t batch, int n_images);
int inrfit_cdn_wide_fit_minibatch(const InrModelDesc* model, const InrFlowDesc* flow, float* icnn_params, float* flow_params,
                                  float* icnn_opt_state, float* flow_opt_state, const float* pool_coords, const float* pool_targets,
                                  int64_t n_pool, const int32_t* index, const int32_t* counts, int64_t batch, const InrLossDesc* loss,
                                  const InrOptDesc* opt, float weight_decay_on_weight_g, int n_images, int steps, int step0,
                                  float* loss_hist, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- rotation / mirror-symmetry prior of the teaser: pose and network trained together (csrc/sym.h) --------------------------------
 * Replaces: `myNet` of notebooks/icml_teaser_code/rotation_symmetric/rotation_symmetric.ipynb cell 2 and the loop of cell 3 (one Adam
 * over pose and network, the `symmetry_prior` switch flipped once training has started).  Per point, with the pose (o0, o1, th):
 *     x' = x + o,  r = |x'|,  n = x' / (r_eps + r),  u = n0 cos th - n1 sin th,  v0 = n0 sin th + n1 cos th,  v = mirror ? |v0| : v0
 * and the network `model` (in_features = 3: a fused kernel, or the layer-by-layer ICNN form such as the notebook's h = 150) on the
 * features (u, v, r).  pose_params [n_images][3] = offset[2] | orientation; pose_opt_state [n_images][6] = exp_avg[3] | exp_avg_sq[3]
 * (zero it before step 0); pose_grads [n_images][3].  grid: the caller's 2-channel grid, shared or per image as everywhere.
 * The pose takes torch's single-tensor Adam step with the learning rate of the network's step (the ICNN header's double buffer) and
 * opt->weight_decay; a step the network's update freezes (a non-finite loss) leaves the pose and its moments untouched.  A point with
 * r == 0 contributes nothing to the pose's gradient (torch yields NaN there).  Every sum has a fixed order: two calls give the same
 * bits.  Callers of the notebook's net pass opt->clamp = 0, opt->freeze_skips = 1 (an unconstrained MLP); the optimizer is Adam.
 * symmetry_from_step: the step with 0-based number step0 + k mirrors iff it is >= symmetry_from_step (negative: never, 0: always).
 * Checks, every one before the first HIP call: INR_EINVAL (a null pointer, r_eps not in (0, inf), steps / step0 < 0, the optimizer, the
 * loss, INR_LOSS_EXTERNAL; the minibatch fit: inrfit_fit_minibatch's), then INR_EUNSUPPORTED (in_features != 3, no kernel and no
 * layer-by-layer form of the shape), then INR_EINVAL (workspace pointer, grid, n_images), then INR_EWORKSPACE. */
typedef struct InrSymDesc {
    int32_t symmetry_from_step;
    float r_eps;   /* the notebook: 0.001 */
} InrSymDesc;

int64_t inrfit_sym_workspace_bytes(const InrModelDesc* model, const InrGridDesc* grid, int n_images);
/* staging buffers (2 coordinate planes, the targets) + inrfit_sym_workspace_bytes for every count in 1..batch */
int64_t inrfit_sym_minibatch_workspace_bytes(const InrModelDesc* model, int64_t batch, int n_images);
/* logits [n_images][n_points] of pose + network; mirror != 0: with the prior */
int inrfit_sym_forward(const InrModelDesc* model, const InrSymDesc* sym, const float* params, const float* pose_params,
                       const InrGridDesc* grid, int n_images, int mirror, float* logits, void* workspace, int64_t workspace_bytes,
                       void* stream);
/* loss_out [n_images], grads [n_images][P] (inrfit_loss_grad's) and pose_grads [n_images][3] */
int inrfit_sym_loss_grad(const InrModelDesc* model, const InrSymDesc* sym, const float* params, const float* pose_params,
                         const InrGridDesc* grid, const float* targets, const InrLossDesc* loss, int n_images, int mirror,
                         float* loss_out, float* grads, float* pose_grads, void* workspace, int64_t workspace_bytes, void* stream);
/* inrfit_fit's full-batch steps with the pose beside the network (params, pose_params, both optimizer states IN PLACE); there are no
 * final logits (inrfit_sym_forward) */
int inrfit_sym_fit(const InrModelDesc* model, const InrSymDesc* sym, float* params, float* pose_params, float* opt_state,
                   float* pose_opt_state, const InrGridDesc* grid, const float* targets, const InrLossDesc* loss, const InrOptDesc* opt,
                   int n_images, int steps, int step0, float* loss_hist, int32_t* status, void* workspace, int64_t workspace_bytes,
                   void* stream);
/* inrfit_fit_minibatch's contract (pool_coords [2][n_pool], the shared index table, counts, the index clamp, step0, loss_hist, status):
 * step k launches exactly what inrfit_sym_fit(steps = 1, step0 = step0 + k) launches on the gathered rows. */
int inrfit_sym_fit_minibatch(const InrModelDesc* model, const InrSymDesc* sym, float* params, float* pose_params, float* opt_state,
                             float* pose_opt_state, const float* pool_coords, const float* pool_targets, int64_t n_pool,
                             const int32_t* index, const int32_t* counts, int64_t batch, const InrLossDesc* loss, const InrOptDesc* opt,
                             int n_images, int steps, int step0, float* loss_hist, int32_t* status, void* workspace,
                             int64_t workspace_bytes, void* stream);

/* ---- joint segmentation + prior training: the composite losses on the device (row a12).
 * INR_JOINT_FBMS - FBMSJointLoss (awesome/measures/fbms_joint_loss.py:35-59).  output [batch][2][hw] = [seg, prior] probabilities (the
 * WrapperModule's output, image mode), target [batch][hw]:
 *     loss = alpha * mean(w (.) crit(seg, target)) + clip(beta * mean((seg - prior)^2))
 * crit = kind (INR_LOSS_SE | INR_LOSS_BCE = torch.nn.BCELoss), w = UnariesWeightedLoss weights by weight_mode / ratio with the
 * fg/bg counts taken over the whole batch (unaries_weighted_loss.py:35-69), clip: the penalty is rescaled to the segmentation
 * loss when it exceeds it (factor detached).  The reference takes that decision on the host - one sync per training step; here
 * nothing leaves the device.
 * INR_JOINT_AWESOME_IMAGE - AwesomeImageLoss (awesome/measures/awesome_image_loss.py:34-53), same layout:
 *     loss = mean(w crit(seg, t)) + alpha * mean(w' pcrit(prior, t));   extra_penalty (the runner's hook, awesome_runner.py:351-371):
 *     loss = gamma * loss + beta * mean((prior - (seg > 0.5))^2)
 * pcrit / w' = prior_kind / prior_weight_mode / prior_ratio.
 * INR_JOINT_AWESOME_PIXEL - AwesomeLoss (awesome/measures/awesome_loss.py:45-65), pixel mode: output [batch][hw][2] = (seg, prior) per
 * pixel, the first n_scribble pixels carry targets [batch][n_scribble], the others are random pixels of the align term:
 *     loss = mean(w crit(seg_s, t)) + alpha * mean(w crit(prior_s, t));   extra_penalty and n_scribble < hw:
 *     loss = gamma * loss + beta * mean((prior_r - (seg_r > 0.5))^2) over pixels [hw - n_scribble, hw)   (the reference's slice, :58-59;
 *     its constants are gamma = 0.1, beta = 100; prior_kind / prior_weight_mode are taken equal to kind / weight_mode).
 * loss_out [4] (device): loss, mean weighted crit(seg) (before alpha / gamma), mean penalty (before beta), FBMS's clip factor.
 * doutput (optional), laid out like output: d loss / d output, BOTH channels. */
enum { INR_JOINT_FBMS = 0, INR_JOINT_AWESOME_IMAGE = 1, INR_JOINT_AWESOME_PIXEL = 2 };
typedef struct InrJointLossDesc {
    int32_t kind;
    int32_t weight_mode;
    float ratio;
    float alpha, beta;
    int32_t clip_penalty;     /* INR_JOINT_FBMS */
    int32_t form;             /* INR_JOINT_* (0 = FBMS: a zero-initialised tail keeps ABI v4 callers' meaning) */
    int32_t prior_kind;       /* INR_JOINT_AWESOME_IMAGE: criterion / weights of the prior term */
    int32_t prior_weight_mode;
    float prior_ratio;
    float gamma;              /* AWESOME_*: factor on the data terms once extra_penalty is on */
    int32_t extra_penalty;
    int64_t n_scribble;       /* INR_JOINT_AWESOME_PIXEL: leading pixels with targets (0 = all) */
    /* ABI v7 - the targets' meaning for the data terms (a zero-initialised tail keeps the v6 meaning):
     * target_rule 0: unaries, UnariesWeightedLoss (awesome/measures/unaries_weighted_loss.py:35-69): fg = target < 0.5, bg = the rest;
     * target_rule 1: class labels, WeightedLoss (awesome/measures/weighted_loss.py:38-62): fg = target == 0, bg = target == 1 (the
     *                counts behind the class weight), any other value takes weight 1;
     * use_noneclass: pixels whose target equals `noneclass` leave the data terms altogether - sums, counts and the mean's
     *                denominator (weighted_loss.py:71-74; 2 in the reference's FBMS configs).  The penalty / align term has no
     *                targets and keeps every pixel. */
    int32_t target_rule;
    int32_t use_noneclass;
    float noneclass;
} InrJointLossDesc;
int64_t inrfit_joint_loss_workspace_bytes(int64_t n_elems);
int inrfit_joint_loss(const float* output, const float* target, int batch, int64_t hw, const InrJointLossDesc* desc,
                      float* loss_out, float* doutput, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- ONE fused training step of the joint segmentation + prior optimisation for one image:
 * TorchAgent._perform_step (awesome/agent/torch_agent.py:428-551) with the PriorManager swap (awesome/dataset/prior_dataset.py:96-110)
 * reduced to "which parameter row".  The segmentation network stays a torch module; everything behind its output runs here:
 *     prior forward (this image's parameters) -> sigmoid -> composite loss (value + d loss / d seg) -> prior backward FROM THE
 *     ACTIVATIONS OF THAT SAME PASS (the fused step kernel; no second forward) -> Adam / Adamax on the row in place -> enforce_convexity
 * seg [n_points]: the segmentation module's probabilities of this image (output channel 0 of the WrapperModule, after its sigmoid /
 * inversion, wrapper_module.py:230-273); target [n_points].  dseg [n_points] (out) = d loss / d seg for the torch backbone's own
 * backward.  prior_logits [n_points] (out, optional): the prior's pre-sigmoid output of this step's forward.  loss_out [4] as in
 * inrfit_joint_loss.  params / opt_state: ONE row (inrfit_param_count / inrfit_opt_state_floats floats); the reference keeps ONE
 * optimizer state for the single prior model whose VALUES are swapped per image (torch_agent.py:812-839), so a caller reproduces it
 * by passing the same opt_state with every row and `step` = the global step count; a state per row with its own count is the
 * per-image variant.  `step` >= 1 is torch's state['step'] after this step (bias corrections); the learning rate is opt->lr (host
 * schedulers stay on the host), opt->plateau is ignored.  A non-finite loss leaves the row untouched and sets *status (optional).
 * Forms: INR_JOINT_FBMS (any target rule / noneclass: the prior's term has no targets), and INR_JOINT_AWESOME_IMAGE with
 * extra_penalty off or on, on unaries without a noneclass (its prior terms are evaluated by the step kernel, which reads unaries:
 * with the penalty on, the class-weighted criterion against the targets AND the align term against [seg > 0.5] in the same pass);
 * otherwise INR_EUNSUPPORTED (INR_JOINT_AWESOME_PIXEL always).  With the penalty on, loss_out[2] is the mean align term before
 * beta and loss_out[3] = 1, as inrfit_joint_loss gives them.
 * A non-finite COMPOSITE loss (a NaN in `seg` as much as in the prior) freezes the row.
 * How the clip stays on the device with a single prior pass: the prior's gradient is linear in the penalty's coefficient, so the step
 * kernel runs with the unclipped coefficient, its own loss column gives the penalty, and the update kernel multiplies the reduced
 * gradient by the (detached) clip factor. */
int64_t inrfit_joint_step_workspace_bytes(const InrModelDesc* model, const InrGridDesc* grid);
int inrfit_joint_step(const InrModelDesc* model, float* params, float* opt_state, const InrGridDesc* grid, const float* seg,
                      const float* target, const InrJointLossDesc* desc, const InrOptDesc* opt, int step, float* loss_out,
                      float* dseg, float* prior_logits, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);
/* The same step with the path-connected priors (ICNN behind a learned deformation of the grid): PathConnectedNet with the RealNVP
 * flow (optimizer over ICNN + flow_net + 1x1 linear, `flow_weight_decay` on the flow_net parameters) and ConvexDiffeomorphismNet
 * (weight decay `wd_on_weight_g` on every *weight_g; opt->kind must be INR_OPT_ADAM).  Workspace: inrfit_pcn_workspace_bytes /
 * inrfit_cdn_workspace_bytes (n_images = 1) + inrfit_joint_loss_workspace_bytes(n_points). */
int inrfit_pcn_joint_step(const InrModelDesc* model, const InrRnvpDesc* rnvp, float* icnn_params, float* flow_params,
                          float* icnn_opt_state, float* flow_opt_state, const InrGridDesc* grid, const float* seg,
                          const float* target, const InrJointLossDesc* desc, const InrOptDesc* opt, float flow_weight_decay,
                          int step, float* loss_out, float* dseg, float* prior_logits, int32_t* status, void* workspace,
                          int64_t workspace_bytes, void* stream);
int inrfit_cdn_joint_step(const InrModelDesc* model, const InrFlowDesc* flow, float* icnn_params, float* flow_params,
                          float* icnn_opt_state, float* flow_opt_state, const InrGridDesc* grid, const float* seg,
                          const float* target, const InrJointLossDesc* desc, const InrOptDesc* opt, float wd_on_weight_g,
                          int step, float* loss_out, float* dseg, float* prior_logits, int32_t* status, void* workspace,
                          int64_t workspace_bytes, void* stream);


/* The PRIOR's share of a joint step, for losses whose segmentation share stays with the caller (the convexity benchmark's
 * AwesomeImageLoss / AwesomeImageLossJoint / AwesomeLoss / AwesomeLossJoint, whose segmentation criterion may need second-order
 * autograd through the segmentation network).  Every one of them splits into
 *     loss = seg_term                                       (the caller's, e.g. gamma crit(seg, t), evaluated in torch)
 *          + c_data  pcrit_masked(prior[p < data_count], t)  (the prior's data term: 'mean' over the valid points)
 *          + beta    mean_{p >= align_begin}((prior - A(seg))^2),   A = [seg > 0.5] (INR_ALIGN_HARD) or seg (INR_ALIGN_SOFT)
 * and this call evaluates the last two in the step kernel: prior forward, loss, backward, Adam / Adamax + enforce_convexity on the
 * row in place, as inrfit_joint_step.  `target` holds data_count values: target[p] is the target of point p.  Points whose target
 * equals `noneclass` (use_noneclass) contribute nothing and are not counted; the class weight (weight_mode) is taken over the rest.
 * ICNN priors with a fused kernel only (a layer-by-layer shape: INR_EUNSUPPORTED; inrfit_wide_joint_prior_step takes those). */
enum { INR_ALIGN_NONE = 0, INR_ALIGN_HARD = 1, INR_ALIGN_SOFT = 2 };
typedef struct InrJointPriorDesc {
    int32_t kind;             /* the prior's data term: INR_LOSS_SE or INR_LOSS_BCE */
    int32_t weight_mode;      /* INR_WEIGHT_NONE .. INR_WEIGHT_SSSDMS on unaries (fg = target < 0.5) */
    float ratio;              /* INR_WEIGHT_RATIO */
    int32_t use_noneclass;
    float noneclass;
    int64_t data_count;       /* points with a data term: [0, data_count); 0 = all points */
    float c_data;             /* the data term's factor (gamma alpha) */
    int32_t align_rule;       /* INR_ALIGN_* */
    float beta;               /* the align term's factor; the mean runs over n_points - align_begin points */
    int64_t align_begin;
} InrJointPriorDesc;
/* Arguments as inrfit_joint_step (same workspace, inrfit_joint_step_workspace_bytes), plus `seg_term`: null or ONE device float,
 * the caller's segmentation share, read on the device after the caller's own work on `stream`.  loss_out [4]: the composite loss
 * (*seg_term + the prior's share), the data term (c_data included), the mean align term before beta, the gradient scale (1; NaN =
 * frozen).  dseg [n_points] = d(prior's share) / d seg: 0 for INR_ALIGN_NONE / HARD, -2 beta (prior - seg) / n_align on the align
 * range for INR_ALIGN_SOFT.  A non-finite composite loss (a NaN in *seg_term as much as in the prior's share) leaves the row and its
 * moments untouched and sets *status; a NaN in seg counts as 0 under INR_ALIGN_HARD (torch's nan > 0.5). */
int inrfit_joint_prior_step(const InrModelDesc* model, float* params, float* opt_state, const InrGridDesc* grid, const float* seg,
                            const float* target, const InrJointPriorDesc* desc, const float* seg_term, const InrOptDesc* opt,
                            int step, float* loss_out, float* dseg, float* prior_logits, int32_t* status, void* workspace,
                            int64_t workspace_bytes, void* stream);

/* ---- the fused joint step for ICNN shapes of the layer-by-layer path (n_hidden > 130 or more than two hidden layers).
 * inrfit_joint_step, inrfit_pcn_joint_step and inrfit_joint_prior_step keep returning INR_EUNSUPPORTED for these shapes; the three
 * calls below take the same argument lists with the same semantics (one image per call, the row updated in place, `step` = torch's
 * state['step'] after the step, opt->plateau ignored, loss_out [4], dseg, optional prior_logits; a non-finite composite loss leaves
 * the row - for the path-connected prior also the flow parameters - and every moment untouched and sets *status; nothing is read
 * on the host) for exactly the ICNN-form shapes without a fused kernel: relu layer 0, one output, n_features = n_hidden,
 * in_features 2 or 3, n_hidden <= 1024, n_layers <= 8.  A shape WITH a fused kernel and the encode shapes: INR_EUNSUPPORTED.
 * One step = the layer-by-layer forward, whose output pass evaluates the joint step's data term (soft targets, the masked data
 * term, the hard / soft align term) into the loss column of its gradient vector, the layer-by-layer backward, the finish kernel
 * (clip factor / gradient scale), the optimizer step on the gradient vector times that scale, d loss / d seg - and for the
 * path-connected prior the RealNVP's forward in front and its backward and update (same scale, learning rate and frozen flag from
 * the ICNN's header) behind.  Forms of inrfit_wide_joint_step / inrfit_pcn_wide_joint_step: as inrfit_joint_step.
 * One addition to the fused calls' semantics: when the composite loss is not finite (*status = 1), dseg is all zeros - a frozen step
 * hands the backbone no gradient.
 * Workspace: the two calls below (inrfit_wide_joint_prior_step: inrfit_wide_joint_step_workspace_bytes). */
int64_t inrfit_wide_joint_step_workspace_bytes(const InrModelDesc* model, const InrGridDesc* grid);
int64_t inrfit_pcn_wide_joint_step_workspace_bytes(const InrModelDesc* model, const InrRnvpDesc* rnvp, const InrGridDesc* grid);
int inrfit_wide_joint_step(const InrModelDesc* model, float* params, float* opt_state, const InrGridDesc* grid, const float* seg,
                           const float* target, const InrJointLossDesc* desc, const InrOptDesc* opt, int step, float* loss_out,
                           float* dseg, float* prior_logits, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);
int inrfit_pcn_wide_joint_step(const InrModelDesc* model, const InrRnvpDesc* rnvp, float* icnn_params, float* flow_params,
                               float* icnn_opt_state, float* flow_opt_state, const InrGridDesc* grid, const float* seg,
                               const float* target, const InrJointLossDesc* desc, const InrOptDesc* opt, float flow_weight_decay,
                               int step, float* loss_out, float* dseg, float* prior_logits, int32_t* status, void* workspace,
                               int64_t workspace_bytes, void* stream);
int inrfit_wide_joint_prior_step(const InrModelDesc* model, float* params, float* opt_state, const InrGridDesc* grid, const float* seg,
                                 const float* target, const InrJointPriorDesc* desc, const float* seg_term, const InrOptDesc* opt,
                                 int step, float* loss_out, float* dseg, float* prior_logits, int32_t* status, void* workspace,
                                 int64_t workspace_bytes, void* stream);

/* The same step for ConvexDiffeomorphismNet over such an ICNN: the twin of inrfit_pcn_wide_joint_step behind the weight-normed coupling
 * flow, with the argument list and semantics of inrfit_cdn_joint_step (Adam only: any other optimizer is INR_EINVAL, answered before
 * the model is looked at; wd_on_weight_g as in inrfit_cdn_fit).  It takes exactly the shapes inrfit_cdn_joint_step refuses -
 * ICNN-form, no fused kernel, in_features = 2 - and refuses the others (fused shapes, encode shapes: INR_EUNSUPPORTED).  One step =
 * the flow's forward | the layer-by-layer forward and backward, whose dL/dcoords lands planar [2][n_points] in the flow's buffer | the
 * finish kernel | the ICNN's optimizer step | the flow's backward and its Adam step with the same gradient scale, this step's
 * learning rate and the frozen flag from the ICNN's header | d loss / d seg (all zeros when *status = 1).
 * The other inrfit_cdn_* calls (workspace_bytes, forward, loss_grad, fit, fit_minibatch) take these shapes under their own names. */
int64_t inrfit_cdn_wide_joint_step_workspace_bytes(const InrModelDesc* model, const InrFlowDesc* flow, const InrGridDesc* grid);
int inrfit_cdn_wide_joint_step(const InrModelDesc* model, const InrFlowDesc* flow, float* icnn_params, float* flow_params,
                               float* icnn_opt_state, float* flow_opt_state, const InrGridDesc* grid, const float* seg,
                               const float* target, const InrJointLossDesc* desc, const InrOptDesc* opt, float wd_on_weight_g,
                               int step, float* loss_out, float* dseg, float* prior_logits, int32_t* status, void* workspace,
                               int64_t workspace_bytes, void* stream);

/* Measurement hook (bench.py, rocprof): launch ONLY the fused forward+loss+backward step kernel `iters` times
 * back-to-back on `stream` (no optimizer step), so its average duration can be bracketed with events. */
int inrfit_step_only(const InrModelDesc* model, const float* params, const InrGridDesc* grid, const float* targets,
                     const InrLossDesc* loss, int n_images, int iters, void* workspace, int64_t workspace_bytes,
                     void* stream);

/* Measurement hook (bench.py): one launch of `workgroups` x 4 waves that issue nothing but independent fp32 16x16x4 MFMAs
 * (32 * iters per wave); *flop = the products' flops.  Timed by the caller, it gives the matrix-pipe rate the chip sustains at
 * the clock it holds under full MFMA load - the practical ceiling next to the nominal peak.  `scratch`: any device buffer of
 * >= workgroups * 1 KiB (never written in practice). */
int inrfit_mfma_stream(int workgroups, int iters, double* flop, void* scratch, void* stream);

/* Measurement hook (bench.py): between begin and end, inrfit_fit and inrfit_step_only calls of this thread bracket each of
 * their (first max_samples) step-kernel launches - inrfit_fit also its update-kernel launches - with a pair of HIP events on
 * the launch stream; end waits for them and returns the average elapsed time of a bracket in microseconds (0 if none).
 * A bracket = the kernel + what the two event packets add to the sequence; bench.py removes that excess by comparing the sum
 * of the two brackets with the un-instrumented time per optimizer step. */
int inrfit_timing_begin(int max_samples);
int inrfit_timing_end(float* avg_step_bracket_us, float* avg_update_bracket_us, int* n_samples);

/* Test hook (tests/test_gpu_rnvp.py): the kernels' own tanh / exp of the coupling outputs (awesome_amd/csrc/rnvp.h fast_tanh /
 * fast_exp) evaluated on x [n] -> tanh_out [n], exp_out [n], so their error bounds are asserted against float64 on the device
 * that runs them. */
int inrfit_debug_tanh_exp(const float* x, int64_t n, float* tanh_out, float* exp_out, void* stream);

/* ---- star-shape prior of the teaser ----------------------------------------------------------------------
 * Replaces: `myNet` of notebooks/icml_teaser_code/star_shaped/star.ipynb cell 2 (forward) and the training loop of cell 3 (minibatch of
 * pixels -> sigmoid -> nn.MSELoss -> torch.optim.Adam(net.parameters(), lr) -> W2_r.weight <- relu(W2_r.weight); `offset` joins the
 * optimizer at a given epoch).  out = r (W2 x_old + W2_r relu(W1 x_old + W1_r r)) - 1, x_old = relu(W0 x / (0.01 + r)), r = |x + offset|.
 * params: ONE flat vector in the order of the class's named_parameters():
 *   offset[2] | W0.weight[h][2] | W0.bias[h] | W1.weight[h][h] | W1.bias[h] | W2.weight[h] | W2.bias | W1_r.weight[h] | W1_r.bias[h] |
 *   W2_r.weight[h] | W2_r.bias                                                      (inrfit_star_param_count = h^2 + 8 h + 4)
 * coords: [n_pixels][2] row-major (the notebook's pixel_info), labels [n_pixels]; 1 <= n_hidden <= 1024.  Layer-by-layer kernels with
 * the hand-written fp32-MFMA GEMMs of csrc/gemm.h for the h x h contractions (csrc/star.h); results reproducible run to run. */
typedef struct InrStarDesc {
    int32_t n_hidden;
} InrStarDesc;

int64_t inrfit_star_param_count(const InrStarDesc* star);
/* workspace for n_points points evaluated at once (the minibatch size for _fit / _loss_grad, all pixels for _forward) */
int64_t inrfit_star_workspace_bytes(const InrStarDesc* star, int64_t n_points);
/* logits[n_points] = net(coords) (star.ipynb cell 4 / 6: inference on every pixel) */
int inrfit_star_forward(const InrStarDesc* star, const float* params, const float* coords, int64_t n_points, float* logits,
                        void* workspace, int64_t workspace_bytes, void* stream);
/* One minibatch (index[batch] pixel numbers, or NULL = the first `batch` pixels): loss[1] = MSE(sigmoid(net), labels) and its gradient
 * with respect to every parameter, the centre included, in the parameter layout (grads[P]); batch <= 65536. */
int inrfit_star_loss_grad(const InrStarDesc* star, const float* params, const float* coords, const float* labels, int64_t n_pixels,
                          const int32_t* index, int64_t batch, float* loss, float* grads, void* workspace, int64_t workspace_bytes,
                          void* stream);
/* The training loop of cell 3 on the device: for epoch = step0 .. step0 + steps - 1: minibatch batch_index[epoch - step0][batch]
 * (values clamped into [0, n_pixels)), forward, MSE, backward, Adam (opt->lr, beta1, beta2, eps; kind must be INR_OPT_ADAM) on params
 * IN PLACE with opt_state [2 P] (exp_avg | exp_avg_sq; zero it before epoch 0), then W2_r.weight <- max(W2_r.weight, 0).  `offset`
 * takes its first step at epoch `offset_first_step` with its own step count, as torch's Adam treats a parameter that starts to
 * receive gradients (the notebook sets requires_grad after the forward pass of epoch 1000: offset_first_step = 1001; < 0: never).
 * loss_hist [steps] or NULL.  Nothing synchronises with the host. */
int inrfit_star_fit(const InrStarDesc* star, float* params, float* opt_state, const float* coords, const float* labels,
                    int64_t n_pixels, const int32_t* batch_index, int64_t batch, const InrOptDesc* opt, int32_t steps, int32_t step0,
                    int32_t offset_first_step, float* loss_hist, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- the star-shape prior as a dense, full-batch, many-image fit (what `pretrain` runs for every other prior family) -----------------
 * Every step sees ALL n_pixels pixels of an image: forward, the criterion of the ICNN fits on sigmoid(out) against the unaries
 * (InrLossDesc: SE / BCE, BCE's log clamped at -100 with a NaN kept a NaN; weight modes none / equal / ratio / sssdms / explicit with
 * target < 0.5 as foreground, the class counts taken once before the loop), backward, INR_OPT_ADAM or INR_OPT_ADAMAX in torch's
 * single-tensor operation order on params IN PLACE, W2_r.weight <- max(W2_r.weight, 0), ReduceLROnPlateau (InrOptDesc.plateau*).
 * The images run one after another inside the call; nothing synchronises with the host.
 *   params [n_images][P]; opt_state [n_images][inrfit_star_opt_state_floats] = exp_avg [P] | exp_avg_sq or exp_inf [P] | header
 *   [INR_OPT_HEADER_FLOATS], the header as documented for the ICNN fits above (step0 == 0 takes lr from InrOptDesc and resets the
 *   plateau state, step0 > 0 continues from the header; zero-initialise for a cold fit);
 *   coords [n_pixels][2] row-major, image i at coords + i * coords_image_stride floats (0 = one grid for all images, else >= 2 n_pixels);
 *   targets [n_images][n_pixels]; loss_hist [n_images][steps] or NULL: the loss BEFORE each step; final_logits [n_images][n_pixels] or
 *   NULL: the output of the last training forward (opt->logits_at_last_forward = 1, what the IoU gate reads) or the logits at the
 *   final parameters (0; one more forward); status [n_images].
 * The centre takes its first step at epoch `offset_first_step` with its own step count, as in inrfit_star_fit (< 0: never).
 * A non-finite loss freezes that image alone: its parameters and moments stay as they were before that step, status =
 * INR_STATUS_NONFINITE.  opt->weight_decay != 0, clamp, freeze_skips, freeze_input: INR_EINVAL (not part of this prior).
 * Point tiles: the grid is walked in tiles of inrfit_star_dense_tile_points() points - a constant of the library, NOT derived from the
 * device, because it fixes the order of the sums - so the workspace holds [T][h] activations whatever n_pixels is, and no 65536 limit
 * applies.  Every gradient is accumulated over the tiles in tile order (the h x h product's split-K slices in slice order inside a tile,
 * the seven column sums, the centre's and the read-out bias's scalars): two runs give the same bits.
 * Centre on a pixel: a pixel exactly at -offset has r = 0, where x'/r is 0/0 - torch (and the minibatch entry points above) give the
 * centre a NaN gradient.  On a dense grid that is a live case, so here such a pixel contributes NOTHING to the centre's gradient; every
 * other gradient of that pixel is finite as it is (out = -1 there). */
int32_t inrfit_star_dense_tile_points(void);
int64_t inrfit_star_opt_state_floats(const InrStarDesc* star);
int64_t inrfit_star_dense_workspace_bytes(const InrStarDesc* star, int64_t n_pixels, int32_t n_images);
int inrfit_star_fit_dense(const InrStarDesc* star, float* params, float* opt_state, const float* coords, int64_t coords_image_stride,
                          const float* targets, const InrLossDesc* loss, const InrOptDesc* opt, int64_t n_pixels, int32_t n_images,
                          int32_t steps, int32_t step0, int32_t offset_first_step, float* loss_hist, float* final_logits, int32_t* status,
                          void* workspace, int64_t workspace_bytes, void* stream);
/* loss_out [n_images], grads [n_images][P] of the same criterion at `params`, with the same tiling and the same r = 0 convention; no
 * optimizer.  (The gradient surface beyond one tile, and beyond inrfit_star_loss_grad's 65536 points.) */
int inrfit_star_loss_grad_dense(const InrStarDesc* star, const float* params, const float* coords, int64_t coords_image_stride,
                                const float* targets, const InrLossDesc* loss, int64_t n_pixels, int32_t n_images, float* loss_out,
                                float* grads, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- the convexity benchmark's segmentation network (awesome/model/cnn_net.py CNNNet, csrc/cnnseg.h) --------------------------------
 * Conv3x3 in_channels -> width, LeakyReLU(0.01), depth x [Conv3x3 width -> width, ReLU], Conv3x3 width -> 1, all with padding 1, batch 1,
 * fp32; the input is the channel concatenation of `image` [image_channels][H][W] and `features` [in_channels - image_channels][H][W].
 * s = sigmoid(f), or 1 - sigmoid(f) with `inversion`.  The share of the joint loss it is trained with (GradientPenaltyLoss(BCELoss) or
 * BCELoss, times g):
 *     loss = g ( mean_{t != noneclass} BCE(s, t) + sum_grp coef[grp] mean_{channels of grp, pixels} |d sum(s) / d input| )
 * channel_group[c] names the group of input channel c (0 rgb, 1 xy, 2 feat, -1 none); coef[grp] = 0: no term; penalty = 0: no
 * penalty at all.  Supported: kernel_size 3, width 16, depth <= 3, 1 <= in_channels <= 8, any H x W (INR_EUNSUPPORTED otherwise).
 * weights / biases: host arrays of depth + 2 device pointers, the layers' torch tensors ([co][ci][3][3] and [co]). */
typedef struct InrCnnSegDesc {
    int32_t in_channels;
    int32_t image_channels;
    int32_t width;
    int32_t depth;
    int32_t kernel_size;
    int32_t height;
    int32_t width_px;
    int32_t inversion;
    int32_t use_noneclass;
    float noneclass;
    float g;
    int32_t penalty;
    float coef[3];
    int32_t channel_group[8];
} InrCnnSegDesc;

/* gradient layout: the module's parameters() order, w_0 | b_0 | w_1 | b_1 | ... */
int64_t inrfit_cnnseg_param_count(const InrCnnSegDesc* desc);
int64_t inrfit_cnnseg_workspace_bytes(const InrCnnSegDesc* desc);
/* Forward: logits [H W] = f, seg [H W] = s.  With `target` [H W] (else null) also the loss above into loss_out[0] (one device float,
 * the seg_term inrfit_joint_prior_step can take) and everything inrfit_cnnseg_step needs from the forward, kept in `workspace`. */
int inrfit_cnnseg_forward(const InrCnnSegDesc* desc, const float* const* weights, const float* const* biases, const float* image,
                          const float* features, const float* target, float* logits, float* seg, float* loss_out, void* workspace,
                          int64_t workspace_bytes, void* stream);
/* One step: the forward above (skipped with reuse_forward = 1 when inrfit_cnnseg_forward ran with the same arguments on the same
 * workspace), then grads [param_count] = d (loss + sum_p dseg[p] s[p]) / d parameters; dseg [H W] or null.  A non-finite loss or gradient
 * zeroes grads and sets *status = 1 (else 0).  Reductions are fixed-order: results are bit-reproducible.  No host sync. */
int inrfit_cnnseg_step(const InrCnnSegDesc* desc, const float* const* weights, const float* const* biases, const float* image,
                       const float* features, const float* target, const float* dseg, int reuse_forward, float* logits, float* seg,
                       float* loss_out, float* grads, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- the convexity benchmark's fully connected segmentation network (awesome/model/fc_net.py FCNet, csrc/fcseg.h) -------------------
 * Linear(in_channels, width), ReLU, depth x [Linear(width, width), ReLU], Linear(width, 1) on n_rows pixel rows, fp32.  A row's input is
 * the concatenation [image_rows[r][0 .. image_channels) | feature_rows[r][0 .. in_channels - image_channels)], read from the two
 * row-major tensors as they are.  s = sigmoid(f), or 1 - sigmoid(f) with `inversion`.  The share of the joint loss it is trained with
 * (a plain mean BCELoss on the first data_count rows, log clamped at -100, times g):
 *     loss = g mean_{r < data_count} BCE(s_r, target_r)                    (data_count = 0: all n_rows)
 * Supported: width 16, 0 <= depth <= 3, 1 <= in_channels <= 8, any n_rows >= 1 (INR_EUNSUPPORTED otherwise).
 * weights / biases: host arrays of depth + 2 device pointers, the layers' torch tensors ([out][in] and [out]). */
typedef struct InrFcSegDesc {
    int32_t in_channels;
    int32_t image_channels;
    int32_t width;
    int32_t depth;
    int32_t inversion;
    float g;
    int64_t n_rows;
    int64_t data_count;
} InrFcSegDesc;

/* gradient layout: the module's parameters() order, w_0 | b_0 | w_1 | b_1 | ...; the count does not depend on n_rows */
int64_t inrfit_fcseg_param_count(const InrFcSegDesc* desc);
int64_t inrfit_fcseg_workspace_bytes(const InrFcSegDesc* desc);
/* Forward: logits [n_rows] = f, seg [n_rows] = s (either may be null).  With `target` [data_count or n_rows] (else null) also the loss
 * above into loss_out[0] (one device float, the seg_term inrfit_joint_prior_step can take).  With target = null this is the evaluation
 * forward over a whole image's rows: one launch. */
int inrfit_fcseg_forward(const InrFcSegDesc* desc, const float* const* weights, const float* const* biases, const float* image_rows,
                         const float* feature_rows, const float* target, float* logits, float* seg, float* loss_out, void* workspace,
                         int64_t workspace_bytes, void* stream);
/* One step, two launches: grads [param_count] = d (loss + sum_r dseg[r] s[r]) / d parameters, dseg [n_rows] or null; loss_out, logits,
 * seg as above (each may be null).  The rows' forward is recomputed inside the step's one launch over the rows (its activations never
 * leave registers: that is cheaper than reading them back), so reuse_forward changes nothing but documents, as for
 * inrfit_cnnseg_step, that inrfit_fcseg_forward ran with the same arguments and logits / seg are not needed again.  A non-finite loss
 * or gradient zeroes grads and sets *status = 1 (else 0).  Reductions are fixed-order: results are bit-reproducible.  No host sync. */
int inrfit_fcseg_step(const InrFcSegDesc* desc, const float* const* weights, const float* const* biases, const float* image_rows,
                      const float* feature_rows, const float* target, const float* dseg, int reuse_forward, float* logits, float* seg,
                      float* loss_out, float* grads, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- the UNet segmentation backbone in evaluation mode (awesome/model/unet.py UNet, csrc/unet.h) ------------------------------------
 * InConv, 4 x Down (2 x 2 max-pool + two 3 x 3 convolutions), 4 x Up (bilinear x2 upsampling with align_corners, zero-padded to the skip
 * map's size and concatenated behind it, two 3 x 3 convolutions), OutConv (1 x 1); every 3 x 3 convolution is followed by a BatchNorm2d
 * in evaluation mode (running statistics) and a ReLU.  Channel widths base_width (1, 2, 4, 8, 8) going down and base_width (4, 2, 1, 1)
 * coming up (the reference: base_width 64).  fp32, one image per call, planar maps [channels][height * width].
 * inrfit_unet_pack folds every convolution + BatchNorm pair into one matrix (done once per set of weights, on the device);
 * inrfit_unet_forward runs the network from the packed weights: per convolution a gather kernel and a product of csrc/gemm.h, strip
 * by strip over the pixels (strip_points pixels, rounded up to a multiple of 128; 0: the default of 2048).  Results do not depend on
 * anything but the arguments: two calls give the same bits.
 * Argument errors are answered before the first HIP call: null pointers (table entries included), height or width < 16, non-positive
 * channel counts: INR_EINVAL; base_width not a multiple of 4 or above 64, out_chn above 8, in_chn above 1024, a side above 4096:
 * INR_EUNSUPPORTED; workspace too small: INR_EWORKSPACE. */
typedef struct InrUNetDesc {
    int32_t in_chn;
    int32_t out_chn;
    int32_t base_width;
    int32_t height;
    int32_t width;
    int32_t strip_points;   /* 0: default */
    float bn_eps;
} InrUNetDesc;

/* floats of the packed weights / bytes of the workspace; negative: the error code of the descriptor */
int64_t inrfit_unet_packed_floats(const InrUNetDesc* desc);
int64_t inrfit_unet_workspace_bytes(const InrUNetDesc* desc);
/* conv_w / conv_b: host arrays of 19 device pointers, the convolutions' torch tensors in state_dict order (inc.conv.conv.{0,3},
 * down1..4.mpconv.1.conv.{0,3}, up1..4.conv.conv.{0,3}, outc.conv); bn_gamma / bn_beta / bn_mean / bn_var: host arrays of 18 device
 * pointers, the BatchNorms behind the first 18 (weight, bias, running_mean, running_var).  packed: [inrfit_unet_packed_floats] device
 * floats, 16-byte aligned.  The packed weights do not depend on height, width or strip_points. */
int inrfit_unet_pack(const InrUNetDesc* desc, const float* const* conv_w, const float* const* conv_b, const float* const* bn_gamma,
                     const float* const* bn_beta, const float* const* bn_mean, const float* const* bn_var, float* packed, void* stream);
/* input [in_chn][height * width] -> logits [out_chn][height * width]; workspace 16-byte aligned.  No host sync. */
int inrfit_unet_forward(const InrUNetDesc* desc, const float* packed, const float* input, float* logits, void* workspace,
                        int64_t workspace_bytes, void* stream);

/* ---- the UNet backbone's training step (csrc/unet_train.h) ---------------------------------------------------------------------------
 * The same network on one image in training mode: every BatchNorm normalises with the mean and biased variance of its own input over
 * the image's pixels, and the backward pass yields the gradient of every parameter.  Pointer tables as for inrfit_unet_pack (19
 * convolutions, 18 BatchNorms: weight = gamma, bias = beta).  Strips of the column matrices are sized per layer from one budget;
 * strip_points > 0 forces one size.  Every reduction has a fixed order: two calls give the same bits.  No host sync.
 * Errors as for inrfit_unet_forward; in addition (height >> 4) * (width >> 4) < 2 is INR_EUNSUPPORTED (a single value per channel at
 * the bottom level has no batch variance) and a momentum outside [0, 1] is INR_EINVAL. */
/* number of parameters = floats of the gradient buffer, in torch's parameters() order: per convolution weight [cout][cin][3][3], bias,
 * gamma, beta; then OutConv's weight and bias.  Does not depend on height, width or strip_points. */
int64_t inrfit_unet_param_count(const InrUNetDesc* desc);
int64_t inrfit_unet_train_workspace_bytes(const InrUNetDesc* desc);
/* input [in_chn][height * width] -> logits [out_chn][height * width].  running_mean / running_var are updated in place as torch does:
 * running = (1 - momentum) running + momentum stat, with the unbiased variance.  The workspace keeps what the backward needs. */
int inrfit_unet_train_forward(const InrUNetDesc* desc, const float* const* conv_w, const float* const* conv_b, const float* const* bn_gamma,
                              const float* const* bn_beta, float* const* running_mean, float* const* running_var, float momentum,
                              const float* input, float* logits, void* workspace, int64_t workspace_bytes, void* stream);
/* dlogits [out_chn][height * width] -> grads [inrfit_unet_param_count], every element written.  workspace: as inrfit_unet_train_forward
 * left it for the same descriptor, weights and input. */
int inrfit_unet_train_backward(const InrUNetDesc* desc, const float* const* conv_w, const float* const* conv_b, const float* const* bn_gamma,
                               const float* const* bn_beta, const float* input, const float* dlogits, float* grads, void* workspace,
                               int64_t workspace_bytes, void* stream);

const char* inrfit_strerror(int code);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif
#endif /* INRFIT_H */
