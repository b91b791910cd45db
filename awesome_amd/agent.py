"""The slice of the reference's TorchAgent that the hot path touches (awesome/agent/torch_agent.py).

    PretrainAgent._pretrain          <- TorchAgent._pretrain (:553-627): load `pretrain_state.pth` if present, else call
                                        model.pretrain(train_set, test_set, device, agent, use_progress_bar, **pretrain_args) and
                                        save the returned state
    PretrainAgent._decompose_training_item  <- :380-426
    JointTrainer.perform_step        <- TorchAgent._perform_step (:428-551): per-image prior swap, forward through the
                                        WrapperModule, criterion(output, labels), backward, optimizer.step, enforce_convexity
                                        (the batch_processed hook of awesome/run/awesome_runner.py:294-297)

The reference keeps every image's prior state in a CPU PriorCache and swaps it in and out with load_state_dict / deepcopy
around every step (dataset/prior_dataset.py:96-110), then pulls loss and outputs back to the host (:501-504).  Here the priors
live in one device-resident table (awesome_amd.PriorBank), the swap re-points parameter views, and nothing syncs with the host
unless the caller reads a value.  Everything else the reference agent does (tracker, tensorboard, events, checkpoint objects) is
control plane and out of scope."""
from __future__ import annotations

import inspect
import logging
import os
from typing import Any, Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import torch

from .model.pretrainable_module import PretrainableModule, decompose_training_item
from .prior_bank import PriorBank


def _cpu_state(state: Any) -> Any:
    if isinstance(state, torch.Tensor):
        return state.detach().cpu()
    if isinstance(state, dict):
        return {k: _cpu_state(v) for k, v in state.items()}
    if isinstance(state, (list, tuple)):
        return type(state)(_cpu_state(v) for v in state)
    return state


class PretrainAgent:
    def __init__(self, training_dataset, device="cuda:0", agent_folder: str = "runs/agent", pretrain_args: Optional[Dict[str, Any]] = None,
                 do_pretraining: Optional[bool] = True, force_pretrain: Optional[bool] = False,
                 pretrain_state_path: Optional[str] = None, logger=None):
        self.training_dataset = training_dataset
        self.device = torch.device(device)
        self.agent_folder = agent_folder
        self.pretrain_args = dict(pretrain_args or {})
        self.do_pretraining, self.force_pretrain = do_pretraining, force_pretrain
        self.pretrain_state_path = pretrain_state_path
        self.logger = logger

    def _decompose_training_item(self, item: Any):
        return decompose_training_item(item, self.training_dataset)

    def _pretrain(self, model: torch.nn.Module, train_set, test_set=None, use_progress_bar: bool = True, **kwargs) -> Optional[Any]:
        """TorchAgent._pretrain (:553-627).  Returns the pretrain state (the PriorCache state for prior datasets)."""
        if not (self.do_pretraining is True or (self.do_pretraining is None and kwargs.get("do_pretraining", False))):
            return None
        if not isinstance(model, PretrainableModule):
            raise ValueError("Model is not pretrainable!")
        pre = dict(self.pretrain_args)
        pre.update(kwargs.get("pretrain_args", {}))
        state, loaded = None, False
        if self.pretrain_state_path is not None:
            if os.path.exists(self.pretrain_state_path):
                try:
                    state = torch.load(self.pretrain_state_path, map_location="cpu", weights_only=False)
                    model.pretrain_load_state(train_set=train_set, test_set=test_set, device=self.device, agent=self,
                                              use_progress_bar=use_progress_bar, state=state, **pre)
                    loaded = True
                    logging.info(f"Pretrain state loaded from {self.pretrain_state_path}")
                except Exception as err:   # noqa: BLE001 (the reference logs and pretrains instead)
                    logging.error(f"Error loading pretrain state: {err}")
        else:
            self.pretrain_state_path = os.path.join(self.agent_folder, "pretrain_state.pth")
        force = self.force_pretrain is True or (self.force_pretrain is None and kwargs.get("force_pretrain", False))
        if not loaded or force:
            logging.info("Starting pretraining...")
            state = model.pretrain(train_set=train_set, test_set=test_set, device=self.device, agent=self,
                                   use_progress_bar=use_progress_bar, **pre)
            if state is not None:
                os.makedirs(os.path.dirname(self.pretrain_state_path) or ".", exist_ok=True)
                tmp = self.pretrain_state_path + ".tmp"
                torch.save(_cpu_state(state), tmp)
                os.replace(tmp, self.pretrain_state_path)
                logging.info(f"Pretrain state saved to {self.pretrain_state_path}")
            else:
                logging.info("No pretrain state returned, not saving...")
        logging.info("Pretraining done!")
        return state


def _loss_takes_input(loss: Callable) -> bool:
    """TorchAgent.forward_additional_loss_args (torch_agent.py:150-164): a loss whose `__call__` (for an nn.Module: whose `forward`)
    names `_input` or `kwargs` also receives `_input=device_inputs`."""
    try:
        spec = inspect.signature(loss.__call__).parameters
    except (TypeError, ValueError):
        return False
    if "_input" in spec or "kwargs" in spec:
        if isinstance(loss, torch.nn.Module):
            spec = inspect.signature(loss.forward).parameters
            return "_input" in spec or "kwargs" in spec
        return True
    return False


def _normalise_item(inputs: Sequence[Any], input_mode: str = "image", prior_arg_mode: Optional[str] = None):
    """One training item at batch size 1, as the fused routes take it: (xi, ai, n, pixel), or None for what they refuse.
    image: xi (1, C, H, W), every tensor of ai 4-d, n = H W.  pixel (WrapperModule._forward_pixels): `inputs[0]` is (1, n, F) or
    (n, F) and xi its (n, F) rows, ai the other inputs' rows; the prior's coordinates are xi's first two features
    ('xy_c_preattached') or the clean-xy rows, the third input ('param_clean_grid')."""
    if input_mode == "pixel":
        if prior_arg_mode not in ("xy_c_preattached", "param_clean_grid"):
            return None
        if prior_arg_mode == "param_clean_grid" and (len(inputs) < 3 or not isinstance(inputs[2], torch.Tensor)):
            return None
        x0, rest = inputs[0], tuple(inputs[1:])
        if x0.dim() == 2:
            x0 = x0[None]
            rest = tuple(a[None] if isinstance(a, torch.Tensor) and a.dim() == 2 else a for a in rest)
        if x0.dim() != 3 or x0.shape[0] != 1:
            return None
        xi, ai = x0[0], tuple(a[0] if isinstance(a, torch.Tensor) else a for a in rest)
        return xi, ai, xi.shape[0], True
    xi = inputs[0] if inputs[0].dim() == 4 else inputs[0][None]
    if xi.shape[0] != 1:
        return None
    ai = tuple(a if not isinstance(a, torch.Tensor) or a.dim() == 4 else a[None] for a in inputs[1:])
    return xi, ai, xi.shape[-2] * xi.shape[-1], False


def _layer_by_layer_joint(ispec) -> bool:
    """An ICNN shape the layer-by-layer joint steps take (inrfit_wide_joint_step and its kin): the library serves it, it has no
    fused kernel, and it is an ICNN-form shape (relu layer 0, one output, n_features = n_hidden) - not an encode net's."""
    return ispec.supported() and not ispec.fused() and not ispec.general and ispec.act0 == "relu"


def _fused_prior_family(prior, kind: str, fused_layer_by_layer: bool, fused_cdn_layer_by_layer: bool = False):
    """Which fused joint step serves `prior` under optimizer `kind`: (family, ispec, dspec, wide), or None = the autograd step.
    Host logic only (no device), so the routing of a model class can be checked anywhere."""
    from .model.star_net import StarShapedNet
    if isinstance(prior, StarShapedNet):
        # its `spec` describes the ICNN calls of the autograd bridge, NOT its parameter vector (awesome_amd/star.py PARAM_ORDER): the
        # fused ICNN step would run over another layout.  No fused joint step for the star prior: autograd through its forward.
        return None
    if hasattr(prior, "_specs"):
        try:
            ispec, dspec = prior._specs()
        except NotImplementedError:   # no fused form of this composite at all ('resnet' flow backbone): autograd step
            return None
        family = "pcn" if type(dspec).__name__ == "RnvpSpec" else "cdn"
        wide = not ispec.fused()
        # its ICNN runs layer by layer: the composite's autograd step - unless asked for: fused_layer_by_layer for a
        # PathConnectedNet (inrfit_pcn_wide_joint_step), fused_cdn_layer_by_layer on top of it for a ConvexDiffeomorphismNet
        # (inrfit_cdn_wide_joint_step; a switch of its own, so that the first one alone keeps routing as it did)
        asked = fused_layer_by_layer and (family == "pcn" or fused_cdn_layer_by_layer)
        if wide and not (asked and _layer_by_layer_joint(ispec)):
            return None
        if kind != "adam" and family == "cdn":
            return None
    elif hasattr(prior, "spec"):
        ispec, dspec, family = prior.spec, None, "icnn"
        wide = not ispec.fused()
        # n_hidden > 130 or L > 2: inrfit_joint_step has no kernel (INR_EUNSUPPORTED); autograd step - unless asked
        # for (fused_layer_by_layer: inrfit_wide_joint_step / inrfit_wide_joint_prior_step)
        if wide and not (fused_layer_by_layer and _layer_by_layer_joint(ispec)):
            return None
        if getattr(prior, "fit_options", None):   # FCNet / encode nets: frozen ranges, no clamp - not part of the joint configs
            return None
    else:
        return None
    return family, ispec, dspec, wide


def _prior_grid(prior_args, pixel: bool):
    """The prior's coordinates (WrapperModule.get_prior_args) as the kernels' explicit grid, (2, n) float32."""
    from . import icnn as K
    coords = prior_args[0]
    if pixel:
        coords = coords.reshape(-1, coords.shape[-1]).t()                  # (n, 2) -> (2, n)
    else:
        coords = coords[0] if coords.dim() == 4 else coords
        coords = coords.reshape(coords.shape[0], -1)                       # (2, H, W) -> (2, H W)
    return K.Grid.explicit(coords.to(torch.float32).contiguous())


# The segmentation share of the convexity route, g crit(seg, t): two implementations of the same two operations.
#   forward() -> (seg, seg_term)           seg: image (1, H, W) / pixel (n, 1); seg_term: the share's device scalar
#   backward(seg, seg_term, dseg, check)   the gradient of seg_term + sum(dseg * seg) into the network's .grad.  `check(status)` is
#                                          JointTrainer._check_finite: called once, with the share's status word (None: it has
#                                          none), before anything reaches .grad
class _TorchSegShare:
    """In torch, for any network and criterion: the class's own view of the segmentation channel (convexity_seg_share), one backward
    through the network for both shares."""

    def __init__(self, trainer: "JointTrainer", form, xi, ai, labels, kw):
        self.trainer, self.form, self.xi, self.ai, self.labels, self.kw = trainer, form, xi, ai, labels, kw

    def forward(self):
        from .measures.losses import convexity_seg_share
        seg = self.trainer.wrapper.segmentation_output(self.xi, self.ai)     # autograd attached
        return seg, convexity_seg_share(self.trainer.criterion, self.form, seg[None], self.labels, **self.kw)

    def backward(self, seg, seg_term, dseg, check) -> None:
        check(None)
        roots, grads = [], []
        if seg_term.requires_grad:
            roots.append(seg_term)
            grads.append(None)
        if dseg is not None and seg.requires_grad:
            roots.append(seg)
            grads.append(dseg.view_as(seg))
        if roots:
            torch.autograd.backward(roots, grads)


class _HipSegShare:
    """In HIP (fused_segmentation), `CS` = awesome_amd.cnnseg for a CNNNet on the image or awesome_amd.fcseg for an FCNet on pixel
    rows: CS.forward (s and the share, penalties included) now, CS.step(reuse_forward=True) for the network's gradient of both shares
    into the trainer's flat buffer after the prior's step.  `plan`: what JointTrainer._cnnseg_plan / _fcseg_plan returned."""

    def __init__(self, trainer: "JointTrainer", CS, plan, labels, pixel: bool):
        self.trainer, self.CS, self.labels = trainer, CS, labels
        self.net, self.desc, self.image, self.feat = plan
        self.seg_shape = (-1, 1) if pixel else (1, self.desc.height, self.desc.width_px)

    def forward(self):
        from .measures.losses import AwesomeImageLossJoint, AwesomeLossJoint
        fwd = self.CS.forward(self.net, self.desc, self.image, self.feat, self.labels)
        crit = self.trainer.criterion
        if isinstance(crit, (AwesomeImageLossJoint, AwesomeLossJoint)):       # what convexity_seg_share (the class's __call__)
            crit.criterion.apply_gradient_penalty = True                      # leaves behind
        return fwd.seg.view(self.seg_shape), fwd.loss

    def backward(self, seg, seg_term, dseg, check) -> None:
        CS = self.CS
        grads = self.trainer._seg_grad_buffer(CS.param_count(self.desc), self.image.device)
        out = CS.step(self.net, self.desc, self.image, self.feat, self.labels, dseg=dseg, reuse_forward=True, grads=grads)
        # a non-finite loss or gradient: the network's gradient is zero (the optimizer still steps its moments, as torch would
        # on a zero gradient) and the failure is latched like the prior's
        check(out.status)
        CS.assign_grads(self.net, grads)


class JointTrainer:
    """One optimisation step of the joint segmentation + prior training (TorchAgent._perform_step, :428-551) on device-resident
    priors.  `wrapper` is a WrapperModule(segmentation_module, prior_module); `bank` holds one parameter row per image of the
    prior module; `criterion(output, labels)` e.g. FBMSJointLoss.  `optimizer`: ONE torch optimizer over the segmentation module's
    parameters and the prior module's Parameter objects, as the reference builds it (torch_agent.py:812-839).

    `perform_step` tries these routes in this order, each at batch size 1 (what a PriorManager swap implies):

    joint      takes  image items; FBMSJointLoss, or AwesomeImageLoss on unaries targets without a noneclass (with its extra
                      penalty on only under `fused_extra_penalty`: the step kernel then evaluates both data terms, the weighted
                      criterion against the targets and the align term against [seg > 0.5], in one pass); an ICNN,
                      PathConnectedNet or ConvexDiffeomorphismNet prior (these two without weight decay)
               calls  the segmentation module in torch, then ONE entry point for everything behind its output - prior forward on
                      the image's bank row, sigmoid, the composite loss, d loss / d seg, the prior's backward, Adam / Adamax and
                      enforce_convexity in place: inrfit_joint_step / inrfit_pcn_joint_step / inrfit_cdn_joint_step
                      (awesome_amd.joint); seg.backward(dseg)
                      (an ICNN of the layer-by-layer path - n_hidden > 130 or more than two hidden layers - alone or behind a
                      PathConnectedNet's RealNVP: only under `fused_layer_by_layer`, then inrfit_wide_joint_step /
                      inrfit_pcn_wide_joint_step, and inrfit_wide_joint_prior_step on the `convexity` route; behind a
                      ConvexDiffeomorphismNet's coupling flow only with `fused_cdn_layer_by_layer` as well, then
                      inrfit_cdn_wide_joint_step; else `autograd`)
               else   `convexity` where that applies and the criterion has no such desc; `autograd` for everything else it
                      refuses: batch > 1, the step that initialises ActNorm
    convexity  takes  (`fused_convexity_losses`) AwesomeImageLoss, AwesomeImageLossJoint, AwesomeLoss, AwesomeLossJoint on an ICNN
                      prior, in every phase, with ANY segmentation criterion; image items, and pixel items (input_mode='pixel')
                      under prior_arg_mode 'xy_c_preattached' / 'param_clean_grid'
               calls  the segmentation share g crit(seg, t) (one of the two below), inrfit_joint_prior_step (the prior's masked
                      data term and hard / soft align term, the row's step, d(prior's share) / d seg:
                      measures.losses.convexity_joint_form), the share's backward
               else   `autograd`: batch > 1, a prior criterion without a kernel form, a step without scribble pixels
      torch share     any network and criterion: segmentation_output, convexity_seg_share (the class's own evaluation,
                      GradientPenaltyLoss's second-order penalty included), torch.autograd.backward([seg_term, seg], [None, dseg])
      HIP share       (`fused_segmentation`) image items: a CNNNet awesome_amd.cnnseg supports (3x3, width 16, depth <= 3, 'rgbxy',
                      one output) with BCELoss or GradientPenaltyLoss(BCELoss, mean): inrfit_cnnseg_forward, the prior's step,
                      inrfit_cnnseg_step.  Pixel items: an FCNet awesome_amd.fcseg supports (width 16, depth <= 3, 'rgb' / 'rgbxy'
                      rows of at most 8 channels, one output) with a plain mean BCELoss: inrfit_fcseg_forward, the prior's step,
                      inrfit_fcseg_step.  Either network's gradient of both shares lands in one flat .grad buffer.  Any other
                      network or criterion: the torch share
    autograd   takes  any item, criterion and optimizer
               calls  WrapperModule forward -> criterion -> loss.backward() through the HIP autograd bridges -> optimizer.step()
                      -> enforce_convexity()

    `joint` and `convexity` are the fused implementation (`fused`, the default whenever `_plan_fused` finds one: Adam or Adamax
    without amsgrad, one param group for the prior, a prior with a fused device form, a criterion one of the two routes knows).
    After their call the torch optimizer steps the segmentation parameters only (the prior's Parameters never receive a .grad,
    which torch.optim skips); the prior's hyper-parameters are read from their param group every step, so host LR schedulers keep
    working.  The criterion's desc is read every step too, so the runner's extra-penalty hook takes effect at once.

    The reference shares ONE optimizer state over all images' priors (it has one prior model whose VALUES are swapped): that is
    `shared_prior_moments=True`, the default; False keeps Adam moments and step counts per image (fused routes only)."""

    def __init__(self, wrapper: torch.nn.Module, bank: PriorBank, criterion: Callable, optimizer: torch.optim.Optimizer,
                 fused: Optional[bool] = None, shared_prior_moments: bool = True, check_finite: str = "epoch",
                 fused_extra_penalty: bool = False, fused_convexity_losses: bool = False, fused_segmentation: bool = False,
                 fused_layer_by_layer: bool = False, fused_cdn_layer_by_layer: bool = False):
        if fused_segmentation and not fused_convexity_losses:
            raise ValueError("fused_segmentation runs inside the convexity losses' fused step: it needs fused_convexity_losses=True")
        if fused_cdn_layer_by_layer and not fused_layer_by_layer:
            raise ValueError("fused_cdn_layer_by_layer extends the layer-by-layer fused steps to ConvexDiffeomorphismNet: it needs "
                             "fused_layer_by_layer=True")
        if check_finite not in ("step", "epoch"):
            raise ValueError("check_finite: 'step' (raise before backward like the reference, one host sync per step) or 'epoch' "
                             "(device flag, the caller polls raise_if_failed())")
        self.check_finite = check_finite
        self.wrapper, self.bank, self.criterion, self.optimizer = wrapper, bank, criterion, optimizer
        self.forward_additional_loss_args = _loss_takes_input(criterion)
        self.shared_prior_moments = bool(shared_prior_moments)
        self.fused_extra_penalty = bool(fused_extra_penalty)
        self.fused_convexity_losses = bool(fused_convexity_losses)
        self.fused_segmentation = bool(fused_segmentation)
        self.fused_layer_by_layer = bool(fused_layer_by_layer)
        self.fused_cdn_layer_by_layer = bool(fused_cdn_layer_by_layer)
        # (both names date from the CNNNet share; they serve the FCNet share, inrfit_fcseg_step, as well)
        self._cnn_grads: Optional[torch.Tensor] = None     # the segmentation network's flat gradient (fused_segmentation)
        self.cnnseg_status: Optional[torch.Tensor] = None   # status word of the last inrfit_cnnseg_step / inrfit_fcseg_step
        self._fused_plan = self._plan_fused()
        if fused and self._fused_plan is None:
            raise ValueError("this combination of prior module / criterion / optimizer has no fused joint step")
        self.fused = (self._fused_plan is not None) if fused is None else bool(fused)
        self._t: Dict[Any, int] = {}
        self._opt_state: Dict[Any, Tuple[torch.Tensor, Optional[torch.Tensor]]] = {}
        self.last_status: Optional[torch.Tensor] = None
        self.failed = torch.zeros((), dtype=torch.bool, device=bank.device)   # any step so far had a non-finite loss (device flag)
        self._path: Optional[str] = None       # which implementation took the previous step ("fused" / "autograd")

    # -- ONE optimizer state for the prior, whichever implementation steps it -----------------------------------------------
    # The reference has one torch optimizer for the whole run (torch_agent.py:812-839).  The fused step keeps the prior's moments
    # in its own flat buffers; when a step has to take the other implementation (AwesomeImageLoss once the runner's hook has set
    # `extra_penalty`, unless fused_extra_penalty; a batch of more than one image; the step that initialises ActNorm) the moments
    # and the step count move with it, so the trajectory is the single-optimizer one.  Per-image moments
    # (shared_prior_moments=False) exist in the fused buffers only and are not carried over.
    def _prior_params(self):
        from .prior_bank import _ordered_parameters
        return list(_ordered_parameters(self.wrapper.prior_module))

    def _moment_keys(self) -> Tuple[str, str]:
        return ("exp_avg", "exp_inf") if self._fused_plan["kind"] == "adamax" else ("exp_avg", "exp_avg_sq")

    def _flat_moment_views(self, plan):
        """[(parameter, first-moment view, second-moment view)] into the fused buffers, in bank-row order."""
        iopt, fopt = self._state_for(None, plan)
        P = plan["ispec"].n_params
        Pd = 0 if plan["dspec"] is None else plan["dspec"].n_params
        out, off = [], 0
        for p in self._prior_params():
            n = p.numel()
            if off < P:
                m, v = iopt[off:off + n], iopt[P + off:P + off + n]
            else:
                o = off - P
                m, v = fopt[o:o + n], fopt[Pd + o:Pd + o + n]
            out.append((p, m, v))
            off += n
        assert off == P + Pd, (off, P, Pd)
        return out

    def _hand_over(self, to: str) -> None:
        plan = self._fused_plan
        if plan is None or not self.shared_prior_moments or self._path in (None, to):
            self._path = to
            return
        k1, k2 = self._moment_keys()
        views = self._flat_moment_views(plan)
        if to == "autograd":      # fused buffers -> torch.optim state
            t = self._t.get(None, 0)
            if t > 0:
                for p, m, v in views:
                    st = self.optimizer.state[p]
                    st["step"] = torch.tensor(float(t), dtype=torch.float32)
                    st[k1], st[k2] = m.detach().clone().view_as(p), v.detach().clone().view_as(p)
        else:                     # torch.optim state -> fused buffers
            steps = [float(self.optimizer.state[p]["step"]) for p, _, _ in views if "step" in self.optimizer.state.get(p, {})]
            if steps:
                for p, m, v in views:
                    st = self.optimizer.state.get(p, {})
                    if k1 in st:
                        m.copy_(st[k1].reshape(-1))
                        v.copy_(st[k2].reshape(-1))
                self._t[None] = int(max(steps))
        self._path = to

    # -- fused path ----------------------------------------------------------------------------------------------------------
    def _plan_fused(self) -> Optional[Dict[str, Any]]:
        prior = getattr(self.wrapper, "prior_module", None)
        if prior is None or self.bank.device.type != "cuda":
            return None
        if not getattr(self.wrapper, "use_prior_sigmoid", True) or not getattr(self.wrapper, "evaluate_prior", True):
            return None
        opt = self.optimizer
        if isinstance(opt, torch.optim.Adam) and not isinstance(opt, torch.optim.AdamW):
            kind = "adam"
        elif isinstance(opt, torch.optim.Adamax):
            kind = "adamax"
        else:
            return None
        from .prior_bank import _ordered_parameters
        pids = {id(p) for p in _ordered_parameters(prior)}
        groups = [g for g in opt.param_groups if any(id(p) in pids for p in g["params"])]
        if len(groups) != 1 or groups[0].get("amsgrad", False) or groups[0].get("maximize", False):
            return None
        if not pids <= {id(p) for p in groups[0]["params"]}:
            return None
        fam = _fused_prior_family(prior, kind, self.fused_layer_by_layer, getattr(self, "fused_cdn_layer_by_layer", False))
        if fam is None:
            return None
        family, ispec, dspec, wide = fam
        if not hasattr(self.criterion, "joint_desc") or self.criterion.joint_desc() is None:
            if not self._convexity_applies(family):
                return None
        return dict(kind=kind, group=groups[0], family=family, ispec=ispec, dspec=dspec, wide=wide)

    def _convexity_applies(self, family: str) -> bool:
        """fused_convexity_losses: one of the convexity benchmark's losses on an ICNN prior (inrfit_joint_prior_step)."""
        from .measures.losses import CONVEXITY_LOSSES
        return self.fused_convexity_losses and family == "icnn" and isinstance(self.criterion, CONVEXITY_LOSSES)

    def _state_for(self, key: Any, plan) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        k = None if self.shared_prior_moments else key
        st = self._opt_state.get(k)
        if st is None:
            from . import _lib as L
            P = plan["ispec"].n_params
            dev = self.bank.device
            iopt = torch.zeros(2 * P + L.INR_OPT_HEADER_FLOATS, dtype=torch.float32, device=dev)
            fopt = None if plan["dspec"] is None else torch.zeros(2 * plan["dspec"].n_params, dtype=torch.float32, device=dev)
            st = self._opt_state[k] = (iopt, fopt)
        return st

    # -- the stages the fused routes share ---------------------------------------------------------------------------------------
    def _step_state(self, key: Any):
        """Bump the step count of `key` (of everything under shared_prior_moments) -> (t, ICNN moments, flow moments, the prior's
        hyper-parameters).  Read from the param group every step: host LR schedulers change them between steps."""
        plan, g = self._fused_plan, self._fused_plan["group"]
        kc = None if self.shared_prior_moments else key
        t = self._t[kc] = self._t.get(kc, 0) + 1
        iopt, fopt = self._state_for(key, plan)
        hp = dict(lr=float(g["lr"]), betas=tuple(g.get("betas", (0.9, 0.999))), eps=float(g.get("eps", 1e-8)),
                  weight_decay=float(g.get("weight_decay", 0.0)))
        return t, iopt, fopt, hp

    def _latch(self, res) -> None:
        """A non-finite loss froze the prior's row on the device.  The reference raises ValueError('Loss is nan or inf!') before
        backward (torch_agent.py:484-487), which needs the loss on the host: check_finite="step" does exactly that (one 4-byte
        read per step, _check_finite).  The default keeps the step free of host syncs: the failure is latched in `failed`, the
        caller polls it (scripts/run.py: once per epoch) and raises then - the run is over either way, and a backbone that has
        produced a NaN cannot be stepped meaningfully (its own backward multiplies any gradient by NaN)."""
        self.last_status = res.status
        self.failed |= res.status.reshape(-1)[0] != 0

    def _check_finite(self, seg_status: Optional[torch.Tensor] = None) -> None:
        """Latch the HIP segmentation share's status word, if this step has one, then raise under check_finite == 'step'."""
        if seg_status is not None:
            self.cnnseg_status = seg_status
            self.failed |= seg_status.reshape(-1)[0] != 0
        if self.check_finite == "step":
            self.raise_if_failed()

    def _finish(self, res, seg: torch.Tensor, pixel: bool):
        """The torch optimizer's step (segmentation parameters only) and the step's (loss, output): [seg, sigmoid(prior)] along the
        channel axis, image (1, 2, H, W) / pixel (1, n, 2)."""
        self.optimizer.step()
        out = torch.cat([seg.detach(), torch.sigmoid(res.prior_logits).view_as(seg)], dim=-1 if pixel else 0)[None]
        return res.loss[0], out

    # -- route `joint` -----------------------------------------------------------------------------------------------------------
    def _perform_step_fused(self, key: Any, inputs: Sequence[torch.Tensor], labels: torch.Tensor):
        from . import joint as J
        plan, w = self._fused_plan, self.wrapper
        desc = self.criterion.joint_desc() if hasattr(self.criterion, "joint_desc") else None
        if not self._joint_desc_fusable(desc, plan):
            if self._convexity_applies(plan["family"]):
                return self._perform_step_prior_share(key, inputs, labels)
            return None
        item = _normalise_item(inputs)
        if item is None:
            return None
        if plan["family"] == "pcn" and not all(float(b) > 0 for n, b in w.prior_module.named_buffers() if n.endswith("data_dep_init_done")):
            return None   # ActNorm's data-dependent initialisation happens in the module's first forward: take the autograd step once
        xi, ai, _, _ = item
        self._hand_over("fused")
        self.optimizer.zero_grad()
        seg = w.segmentation_output(xi, ai)                                   # (1, H, W), autograd attached
        grid = _prior_grid(w.get_prior_args(xi, *ai, segm=seg)[0], False)
        row = self.bank.row(key)
        P = plan["ispec"].n_params
        t, iopt, fopt, hp = self._step_state(key)
        segd = seg.detach().reshape(-1).to(torch.float32).contiguous()
        tgt = labels.detach().reshape(-1).to(torch.float32).contiguous()
        if plan["family"] == "icnn":
            step_fn = J.wide_joint_step if plan["wide"] else J.joint_step
            res = step_fn(plan["ispec"], row, iopt, grid, segd, tgt, desc, step=t, optimizer=plan["kind"], clamp=True, **hp)
        else:
            del hp["weight_decay"]      # zero (_joint_desc_fusable): torch would also apply it to their 1x1 / linear layer
            if plan["family"] == "pcn":
                step_fn = J.pcn_wide_joint_step if plan["wide"] else J.pcn_joint_step
                res = step_fn(plan["ispec"], plan["dspec"], row[:P], row[P:], iopt, fopt, grid, segd, tgt, desc,
                              step=t, optimizer=plan["kind"], flow_weight_decay=0.0, **hp)
            else:
                step_fn = J.cdn_wide_joint_step if plan["wide"] else J.cdn_joint_step
                res = step_fn(plan["ispec"], plan["dspec"], row[:P], row[P:], iopt, fopt, grid, segd, tgt, desc,
                              step=t, weight_decay_on_weight_g=0.0, **hp)
        self._latch(res)
        self._check_finite()
        if seg.requires_grad:
            seg.backward(res.dseg.view_as(seg))
        return self._finish(res, seg, False)

    def _joint_desc_fusable(self, desc, plan) -> bool:
        """Whether inrfit_joint_step (and its path-connected variants) take this step's composite loss."""
        if desc is None or (plan["family"] != "icnn" and float(plan["group"].get("weight_decay", 0.0)) != 0.0):
            return False
        if desc.form != 0 and (desc.form != 1 or desc.target_rule or desc.use_noneclass):
            return False  # the pixel form; AwesomeImageLoss on class labels or with a noneclass (inrfit_joint_step: INR_EUNSUPPORTED)
        if desc.form == 1 and desc.extra_penalty and not self.fused_extra_penalty:
            return False  # AwesomeImageLoss with its extra penalty on: the autograd step unless asked for (the desc is read every
                          # step, so gamma / alpha / beta and the hook's switch take effect at once)
        return True

    # -- route `convexity` -------------------------------------------------------------------------------------------------------
    def _perform_step_prior_share(self, key: Any, inputs: Sequence[torch.Tensor], labels: torch.Tensor):
        """fused_convexity_losses: the segmentation share (torch or HIP) + inrfit_joint_prior_step for the prior's share, one
        backward through the segmentation network for both.  None -> the autograd step."""
        from . import _lib as L
        from . import joint as J
        from .measures.losses import convexity_joint_form
        plan, w = self._fused_plan, self.wrapper
        item = _normalise_item(inputs, getattr(w, "input_mode", "image"), getattr(w, "prior_arg_mode", None))
        if item is None:
            return None
        xi, ai, n, pixel = item
        form = convexity_joint_form(self.criterion, n)
        if form is None or form.pixel != pixel or labels.numel() != (form.data_count or n):
            return None
        kw = {"_input": list(inputs)} if self.forward_additional_loss_args else {}
        share = self._seg_share(form, xi, ai, labels, pixel, kw)
        self._hand_over("fused")
        self.optimizer.zero_grad()
        seg, seg_term = share.forward()
        grid = _prior_grid(w.get_prior_args(xi, *ai, segm=seg)[0], pixel)
        row = self.bank.row(key)
        t, iopt, _, hp = self._step_state(key)
        segd = seg.detach().reshape(-1).to(torch.float32).contiguous()
        tgt = labels.detach().reshape(-1).to(torch.float32).contiguous()
        st = seg_term.detach().reshape(1).to(torch.float32).contiguous()
        step_fn = J.wide_joint_prior_step if plan["wide"] else J.joint_prior_step
        res = step_fn(plan["ispec"], row, iopt, grid, segd, tgt, form.prior_desc(), step=t, seg_term=st,
                      optimizer=plan["kind"], clamp=True, **hp)
        self._latch(res)
        dseg = res.dseg if form.align_rule == L.ALIGN_SOFT else None          # hard / none: d(prior's share) / d seg = 0
        share.backward(seg, seg_term, dseg, self._check_finite)
        return self._finish(res, seg, pixel)

    def _seg_share(self, form, xi, ai, labels, pixel: bool, kw):
        """The HIP share where fused_segmentation is on and _cnnseg_plan (image items) / _fcseg_plan (pixel items) accepts the
        step's network and criterion, else the torch share.  `kw`: the criterion's `_input` keyword, if it takes one."""
        if self.fused_segmentation:
            if pixel:
                from . import fcseg as CS
                hip = self._fcseg_plan(form, xi, ai, labels)
            else:
                from . import cnnseg as CS
                hip = self._cnnseg_plan(form, xi, ai, labels, kw)
            if hip is not None:
                return _HipSegShare(self, CS, hip, labels, pixel)
        return _TorchSegShare(self, form, xi, ai, labels, kw)

    def _seg_grad_buffer(self, n_params: int, device) -> torch.Tensor:
        """The HIP share's flat gradient buffer, kept across steps (the parameters' .grad are views of it)."""
        if self._cnn_grads is None or self._cnn_grads.numel() != n_params or self._cnn_grads.device != device:
            self._cnn_grads = torch.empty(n_params, dtype=torch.float32, device=device)
        return self._cnn_grads

    def _cnnseg_plan(self, form, xi, ai, labels, kw):
        """fused_segmentation: (net, InrCnnSegDesc, image, features) when this image-mode step's segmentation share has a HIP form
        (awesome_amd.cnnseg), else None (the torch share)."""
        from . import cnnseg as CS
        from .measures.losses import AwesomeImageLoss, AwesomeImageLossJoint, _criterion_kwargs
        w, crit = self.wrapper, self.criterion
        net = getattr(w, "segmentation_module", None)
        if not getattr(w, "use_segmentation_sigmoid", True) or not CS.net_supported(net):
            return None
        if isinstance(crit, AwesomeImageLoss):
            ckw = _criterion_kwargs(crit.criterion, crit.forward_kwargs_criterion, kw)
        elif isinstance(crit, AwesomeImageLossJoint):
            ckw = _criterion_kwargs(crit.criterion, True, kw)
        else:
            return None
        seg_in, seg_args, _ = w.get_segmentation_module_args(xi, ai, {})
        if len(seg_args) < 1 or not isinstance(seg_in, torch.Tensor) or not isinstance(seg_args[0], torch.Tensor):
            return None
        image, feat = seg_in, seg_args[0]
        if image.dim() != 4 or feat.dim() != 4 or image.shape[0] != 1 or feat.shape[0] != 1 or image.shape[-2:] != feat.shape[-2:]:
            return None
        if image.dtype != torch.float32 or not image.is_cuda or image.shape[1] + feat.shape[1] != net.in_chn:
            return None
        H, W = image.shape[-2], image.shape[-1]
        if labels.numel() != H * W:
            return None
        sform = CS.criterion_form(crit.criterion, ckw, image.shape[1], net.in_chn)
        if sform is None:
            return None
        desc = CS.make_desc(net, image.shape[1], H, W, sform, inversion=bool(getattr(w, "use_segmentation_output_inversion", False)),
                            g=form.g)
        return net, desc, image, feat

    def _fcseg_plan(self, form, xi, ai, labels):
        """fused_segmentation: (net, InrFcSegDesc, image rows, feature rows) when this pixel-mode step's segmentation share has a HIP
        form (awesome_amd.fcseg), else None (the torch share)."""
        from . import fcseg as FS
        from .measures.losses import AwesomeLoss, AwesomeLossJoint
        w, crit = self.wrapper, self.criterion
        net = getattr(w, "segmentation_module", None)
        if not getattr(w, "use_segmentation_sigmoid", True) or not FS.net_supported(net):
            return None
        if not isinstance(crit, (AwesomeLoss, AwesomeLossJoint)) or FS.criterion_form(crit.criterion) is None:
            return None
        image, seg_args, _ = w.get_segmentation_module_args(xi, ai, {})
        if not isinstance(image, torch.Tensor) or image.dim() != 2 or image.dtype != torch.float32 or not image.is_cuda:
            return None
        n = image.shape[0]
        feat = None
        if net.in_type == "rgbxy":
            if len(seg_args) < 1 or not isinstance(seg_args[0], torch.Tensor):
                return None
            feat = seg_args[0]
            if feat.dim() != 2 or feat.shape[0] != n or not feat.is_cuda:
                return None
        if n < 2 or image.shape[1] + (0 if feat is None else feat.shape[1]) != net.in_chn:
            return None       # (one row: process_segmentation_output drops the dimension, the torch path's shapes differ)
        desc = FS.make_desc(net, image.shape[1], n, data_count=form.data_count,
                            inversion=bool(getattr(w, "use_segmentation_output_inversion", False)), g=form.g)
        return net, desc, image, feat

    # -- the step ------------------------------------------------------------------------------------------------------------
    def perform_step(self, key: Any, inputs: Sequence[torch.Tensor], labels: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (loss, output) as device tensors (no host sync)."""
        if self.fused and self._fused_plan is not None:
            done = self._perform_step_fused(key, inputs, labels)
            if done is not None:
                return done
        self._hand_over("autograd")
        self.optimizer.zero_grad()
        with self.bank.manager(self.wrapper.prior_module, key):
            out = self.wrapper(*inputs)
            loss = self.criterion(out, labels, _input=list(inputs)) if self.forward_additional_loss_args else self.criterion(out, labels)
            self.failed |= ~torch.isfinite(loss.detach())
            if self.check_finite == "step":
                self.raise_if_failed()
            loss.backward()
            self.optimizer.step()
            self.wrapper.enforce_convexity()   # batch_processed hook (awesome_runner.py:294-297)
        return loss.detach(), out.detach()

    def raise_if_failed(self) -> None:
        """One host sync: the reference's `ValueError("Loss is nan or inf!")` (torch_agent.py:484-487), checked when the caller asks."""
        if bool(self.failed):
            raise ValueError("Loss is nan or inf!")
