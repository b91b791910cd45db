"""Host-side logic of the fused joint step for the convexity benchmark's losses (no GPU): the prior criterion's kernel form, the split
each loss produces at each of its switches (measures.losses.convexity_joint_form -> InrJointPriorDesc), the segmentation share as the
class computes it, and JointTrainer's opt-in keyword."""
import pytest
import torch

from awesome_amd import _lib as L
from awesome_amd.measures import (AwesomeImageLoss, AwesomeImageLossJoint, AwesomeLoss, AwesomeLossJoint, GradientPenaltyLoss, SE,
                                  UnariesWeightedLoss, WeightedLoss)
from awesome_amd.measures.losses import convexity_joint_form, convexity_seg_share, joint_prior_criterion_form


def _gpl(**kw):
    return GradientPenaltyLoss(torch.nn.BCELoss(), apply_gradient_penalty=True, xygrad=0.01, rgbgrad=0.01, noneclass=2.0, **kw)


def test_prior_criterion_form():
    assert joint_prior_criterion_form(torch.nn.BCELoss()) == ("bce", "none", 1.0, None)       # targets of 2 included, as in torch
    assert joint_prior_criterion_form(_gpl()) == ("bce", "none", 1.0, 2.0)                      # penalty off: inner + noneclass mask
    assert joint_prior_criterion_form(GradientPenaltyLoss(SE("mean"))) == ("se", "none", 1.0, None)
    assert joint_prior_criterion_form(UnariesWeightedLoss(torch.nn.BCELoss(), mode="sssdms", noneclass=2.0)) == ("bce", "sssdms", 1.0, 2.0)
    with pytest.raises(TypeError):   # class labels (target_rule 1): the autograd step
        joint_prior_criterion_form(WeightedLoss(torch.nn.BCELoss(), mode="sssdms"))
    with pytest.raises(TypeError):
        joint_prior_criterion_form(GradientPenaltyLoss(UnariesWeightedLoss(torch.nn.BCELoss(), noneclass=3.0), noneclass=2.0))
    with pytest.raises(TypeError):
        joint_prior_criterion_form(torch.nn.MSELoss())


def _desc_tuple(form):
    d = form.prior_desc()
    return (d.kind, d.weight_mode, d.use_noneclass, d.noneclass, d.data_count, pytest.approx(d.c_data), d.align_rule,
            pytest.approx(d.beta), d.align_begin)


def test_awesome_image_loss_split():
    crit = AwesomeImageLoss(criterion=_gpl(), alpha=0.7, beta=100.0, gamma=0.1)
    f = convexity_joint_form(crit, 400)
    assert not f.pixel and f.g == 1.0
    assert _desc_tuple(f) == (L.INR_LOSS_BCE, L.INR_WEIGHT_NONE, 0, 0.0, 0, 0.7, L.ALIGN_NONE, 0.0, 0)
    crit.extra_penalty = True
    f = convexity_joint_form(crit, 400)
    assert f.g == pytest.approx(0.1)
    assert _desc_tuple(f) == (L.INR_LOSS_BCE, L.INR_WEIGHT_NONE, 0, 0.0, 0, 0.07, L.ALIGN_HARD, 100.0, 0)
    # a prior criterion the class would call with its penalty on has no form (the class itself raises there)
    assert convexity_joint_form(AwesomeImageLoss(prior_criterion=_gpl()), 400) is None
    assert convexity_joint_form(AwesomeImageLoss(prior_criterion=WeightedLoss(torch.nn.BCELoss())), 400) is None


def test_awesome_image_loss_joint_split():
    crit = AwesomeImageLossJoint(criterion=_gpl(), alpha=0.5, beta=2.0, gamma=0.3)
    f = convexity_joint_form(crit, 100)
    assert _desc_tuple(f) == (L.INR_LOSS_BCE, L.INR_WEIGHT_NONE, 1, 2.0, 0, 0.5, L.ALIGN_NONE, 0.0, 0)
    crit.map_initially_on_segmentation = True
    assert _desc_tuple(convexity_joint_form(crit, 100)) == (L.INR_LOSS_BCE, L.INR_WEIGHT_NONE, 1, 2.0, 0, 0.15, L.ALIGN_HARD, 2.0, 0)
    crit.extra_penalty = True   # wins over map_initially_on_segmentation
    assert _desc_tuple(convexity_joint_form(crit, 100)) == (L.INR_LOSS_BCE, L.INR_WEIGHT_NONE, 1, 2.0, 0, 0.15, L.ALIGN_SOFT, 2.0, 0)


@pytest.mark.parametrize("n", [1000, 1003, 17])
def test_pixel_losses_split(n):
    n_scr = int(n * 0.8 // 1)
    crit = AwesomeLoss(alpha=0.6, scribble_percentage=0.8)
    assert _desc_tuple(convexity_joint_form(crit, n)) == (L.INR_LOSS_BCE, 0, 0, 0.0, n_scr, 0.6, L.ALIGN_NONE, 0.0, 0)
    crit.extra_penalty = True
    f = convexity_joint_form(crit, n)
    assert f.pixel and f.g == pytest.approx(0.1)
    assert _desc_tuple(f) == (L.INR_LOSS_BCE, 0, 0, 0.0, n_scr, 0.06, L.ALIGN_HARD, 100.0, n - n_scr)
    crit = AwesomeLossJoint(alpha=0.6, beta=3.0, gamma=0.2, scribble_percentage=0.8)
    crit.extra_penalty = True
    assert _desc_tuple(convexity_joint_form(crit, n)) == (L.INR_LOSS_BCE, 0, 0, 0.0, n_scr, 0.12, L.ALIGN_SOFT, 3.0, n - n_scr)
    # all pixels are scribbles: no align term even with the penalty on (the classes' `n_rand > 0`)
    crit = AwesomeLossJoint(alpha=0.6, beta=3.0, gamma=0.2, scribble_percentage=1.0)
    crit.extra_penalty = True
    assert _desc_tuple(convexity_joint_form(crit, n)) == (L.INR_LOSS_BCE, 0, 0, 0.0, n, 0.6, L.ALIGN_NONE, 0.0, 0)
    # no scribble pixel at all: the autograd step
    assert convexity_joint_form(AwesomeLoss(scribble_percentage=0.0), n) is None


def test_other_losses_have_no_split():
    from awesome_amd.measures import FBMSJointLoss
    assert convexity_joint_form(FBMSJointLoss(), 100) is None


def _composite(crit, seg_out, prior_out, target, **kw):
    """The class's own __call__ on the (seg, prior) output, and the split: seg share + the prior's share computed here in torch."""
    f = convexity_joint_form(crit, prior_out.shape[-2] if f_pixel(crit) else prior_out.numel())
    if f_pixel(crit):
        out = torch.cat([seg_out, prior_out], dim=-1)
    else:
        out = torch.cat([seg_out, prior_out], dim=1)
    inner = getattr(crit, "criterion", None)
    flag = getattr(inner, "apply_gradient_penalty", None)
    ref = crit(out, target, **kw)
    if flag is not None:
        inner.apply_gradient_penalty = flag    # the split replaces the call: it starts from the same switch
    share = convexity_seg_share(crit, f, seg_out, target, **kw)
    s, p, t = seg_out.reshape(-1), prior_out.reshape(-1), target.reshape(-1)
    kind, mode, ratio, nc = f.prior_form
    pd, td = p[: t.numel()], t
    keep = torch.ones_like(td, dtype=torch.bool) if nc is None else td != nc
    assert kind == "bce" and mode == "none"
    data = torch.nn.functional.binary_cross_entropy(pd[keep], td[keep])
    total = share + f.g * f.alpha * data
    if f.align_rule != L.ALIGN_NONE:
        a = s if f.align_rule == L.ALIGN_SOFT else (s > 0.5).float()
        total = total + f.beta * torch.mean((p[f.align_begin:] - a[f.align_begin:]) ** 2)
    return ref, total


def f_pixel(crit):
    return isinstance(crit, (AwesomeLoss, AwesomeLossJoint))


@pytest.mark.parametrize("which,phase", [(w, p) for w in ("image", "image_joint", "pixel", "pixel_joint") for p in ("before", "after")]
                         + [("image_joint", "map")])
def test_split_recomposes_the_class_loss(which, phase):
    """CPU: seg share + prior share (the formula inrfit_joint_prior_step evaluates) == the class's __call__, every phase."""
    g = torch.Generator().manual_seed(3)
    if which.startswith("image"):
        seg = torch.rand(1, 1, 6, 7, generator=g) * 0.9 + 0.05
        prior = torch.rand(1, 1, 6, 7, generator=g) * 0.9 + 0.05
        target = torch.randint(0, 3, (1, 1, 6, 7), generator=g).float()    # 0 / 1 and the noneclass 2
        inner = GradientPenaltyLoss(torch.nn.BCELoss(), apply_gradient_penalty=False, noneclass=2.0)
        # (torch's BCELoss refuses targets outside [0, 1]: the prior criterion masks the 2s here too)
        crit = (AwesomeImageLoss(criterion=inner, prior_criterion=GradientPenaltyLoss(torch.nn.BCELoss(), noneclass=2.0), alpha=0.7,
                                 beta=100.0, gamma=0.1) if which == "image"
                else AwesomeImageLossJoint(criterion=inner, alpha=0.7, beta=3.0, gamma=0.2))
    else:
        n = 43
        n_scr = int(n * 0.8 // 1)
        seg = torch.rand(1, n, 1, generator=g) * 0.9 + 0.05
        prior = torch.rand(1, n, 1, generator=g) * 0.9 + 0.05
        target = (torch.rand(1, n_scr, 1, generator=g) > 0.5).float()
        crit = (AwesomeLoss(alpha=0.7, scribble_percentage=0.8) if which == "pixel"
                else AwesomeLossJoint(alpha=0.7, beta=3.0, gamma=0.2, scribble_percentage=0.8))
    if phase == "after":
        crit.extra_penalty = True
    elif phase == "map":        # AwesomeImageLossJoint only
        crit.map_initially_on_segmentation = True
    ref, total = _composite(crit, seg, prior, target)
    assert float(total) == pytest.approx(float(ref), rel=1e-5)


def test_seg_share_leaves_the_gradient_penalty_switch_as_the_class_does():
    inner = GradientPenaltyLoss(torch.nn.BCELoss(), apply_gradient_penalty=False)
    crit = AwesomeImageLossJoint(criterion=inner)
    seg = torch.full((1, 1, 2, 2), 0.3)
    convexity_seg_share(crit, convexity_joint_form(crit, 4), seg, torch.ones(1, 1, 2, 2))
    assert inner.apply_gradient_penalty is True     # AwesomeImageLossJoint.__call__ leaves it on after its prior call


def test_joint_trainer_fused_convexity_losses_argument():
    """The opt-in keyword, off by default; no fused plan without a device."""
    from awesome_amd.agent import JointTrainer
    from awesome_amd.model import ConvexNet, WrapperModule
    from awesome_amd.prior_bank import PriorBank, _ordered_parameters
    factory = lambda: ConvexNet(n_hidden=8, in_features=2)   # noqa: E731
    wrapper = WrapperModule(torch.nn.Conv2d(1, 1, 3, padding=1), factory())
    bank = PriorBank(factory, n_images=1, device="cpu")
    opt = torch.optim.Adam(list(wrapper.segmentation_module.parameters()) + list(_ordered_parameters(wrapper.prior_module)), lr=1e-3)
    assert JointTrainer(wrapper, bank, AwesomeImageLossJoint(), opt).fused_convexity_losses is False
    tr = JointTrainer(wrapper, bank, AwesomeImageLossJoint(), opt, fused_convexity_losses=True)
    assert tr.fused_convexity_losses is True and tr._fused_plan is None and not tr.fused
    assert tr._convexity_applies("icnn") and not tr._convexity_applies("pcn")
    tr2 = JointTrainer(wrapper, bank, AwesomeImageLossJoint(), opt)
    assert not tr2._convexity_applies("icnn")
