"""Mutual information of an image pair on the device: the label-free criterion for a multimodal registration, where
registration_ssim says nothing because the intensities of the two images are related by a non-linear or inverted map.

joint_histogram() counts the pairs (fixed value, moving value) of all voxels into bins_a x bins_b cells in one streaming pass
(cvx_joint_hist_f32, include/convexadam_sim.h); with `disp` the moving image is sampled through the field inside that pass -- the arithmetic
of warp_device, bit for bit, without the warped volume.  value_range() is the pass that finds the range the bins are laid over; both chain
on the stream.  The counts are integers and exact: the same bytes on every run.  entropies(), mutual_information() and
normalized_mutual_information() turn a histogram into numbers with torch, in float64, wherever the histogram lives; registration_mi() is
the multimodal twin of registration_ssim.

Tensors must live on the HIP device; there is no CPU path.  Not built: Parzen-window or partial-volume weights (every voxel counts once, in
one cell), local MI maps, gradients of MI with respect to the field, and MI as a registration cost."""
import collections

import torch

from . import _lib
from ._lib import call, f32c, field_operand, ptr, require_device_tensor

STATS = ("kept", "masked", "non_finite", "outside", "clamped")


def _bins(bins):
    ba, bb = (bins, bins) if isinstance(bins, int) else bins
    return int(ba), int(bb)


def _operands(fixed, moving, disp, mask, who):
    """The checked operands of both entry points -> (fixed, moving, field arguments, mask, shape)."""
    fixed = require_device_tensor(fixed, "fixed")
    moving = require_device_tensor(moving, "moving")
    if fixed.dim() != 3 or fixed.shape != moving.shape:
        raise ValueError("%s expects two (H, W, D) volumes of equal shape, got %s and %s" % (who, tuple(fixed.shape), tuple(moving.shape)))
    shape = tuple(int(s) for s in fixed.shape)
    a = f32c(fixed)
    b = f32c(moving.to(a.device))
    u, field = None, (ptr(None), 0, 0, 0)
    if disp is not None:
        disp = require_device_tensor(disp, "disp")
        u, _, cs, vs, f64 = field_operand(disp.to(a.device), grid=shape, name="disp")
        field = (ptr(u), f64, cs, vs)
    m = None
    if mask is not None:
        mask = require_device_tensor(mask, "mask")
        if tuple(mask.shape) != shape:
            raise ValueError("%s: mask must be %s, got %s" % (who, shape, tuple(mask.shape)))
        m = (mask if mask.dtype == torch.uint8 else (mask != 0).to(torch.uint8)).to(a.device).contiguous()
    _lib.sim_lib()
    return a, b, u, field, m, shape


def value_range(fixed, moving, disp=None, mask=None, drop_outside=False, return_info=False):
    """(lo_a, hi_a, lo_b, hi_b) of the voxels joint_histogram would keep -> (4,) float32 device tensor; (+Inf, -Inf, +Inf, -Inf) when
    there are none.  return_info: also the (5,) int64 device tensor of STATS."""
    a, b, u, field, m, shape = _operands(fixed, moving, disp, mask, "value_range")
    rng = torch.empty(4, dtype=torch.float32, device=a.device)
    stats = torch.empty(len(STATS), dtype=torch.int64, device=a.device)
    call(a.device, "cvx_sim_range_f32", ptr(a), ptr(b), *field, ptr(m), *shape, int(bool(drop_outside)), ptr(rng), ptr(stats))
    return (rng, stats) if return_info else rng


def joint_histogram(fixed, moving, bins=32, disp=None, mask=None, value_range=None, drop_outside=False, return_info=False):  # noqa: A002
    """Joint histogram of two (H, W, D) device volumes -> (bins_a, bins_b) int64 device tensor, index a the fixed image.

    bins          an int or a pair, each 2 .. 256
    disp          None, or a displacement field (3, H, W, D) / (H, W, D, 3) in voxels, float32 or float64, read where it lies: the moving
                  value of a voxel is then the one warp_device(moving, disp) would hold there
    mask          None, or (H, W, D): a voxel takes part where the mask is non-zero
    value_range   None: the range of the kept voxels, found by a pass of its own on the same stream; or (lo_a, hi_a, lo_b, hi_b) as a
                  (4,) device tensor (what value_range() returns) or four numbers.  Values outside are counted in the end bins.
    drop_outside  with a field: a voxel whose sampling point lies outside the volume is dropped (and counted) instead of sampling 0
    return_info   also dict(stats=(5,) int64 device tensor in the order of STATS, range=(4,) float32 device tensor): no host round trip
    A voxel with a NaN or an Inf in either image or in its field is never counted in the histogram."""
    ba, bb = _bins(bins)
    a, b, u, field, m, shape = _operands(fixed, moving, disp, mask, "joint_histogram")
    drop = int(bool(drop_outside))
    if value_range is None:
        rng = torch.empty(4, dtype=torch.float32, device=a.device)
        scratch_stats = torch.empty(len(STATS), dtype=torch.int64, device=a.device)
        call(a.device, "cvx_sim_range_f32", ptr(a), ptr(b), *field, ptr(m), *shape, drop, ptr(rng), ptr(scratch_stats))
    else:
        rng = torch.as_tensor(value_range, dtype=torch.float32).to(a.device).contiguous()
        if tuple(rng.shape) != (4,):
            raise ValueError("joint_histogram: value_range must hold (lo_a, hi_a, lo_b, hi_b), got shape %s" % (tuple(rng.shape),))
    hist = torch.empty((ba, bb), dtype=torch.int64, device=a.device)
    stats = torch.empty(len(STATS), dtype=torch.int64, device=a.device)
    call(a.device, "cvx_joint_hist_f32", ptr(a), ptr(b), *field, ptr(m), *shape, ba, bb, ptr(rng), drop, ptr(hist), ptr(stats))
    return (hist, dict(stats=stats, range=rng)) if return_info else hist


def _entropy(counts, n):
    c = counts.to(torch.float64)
    p = c / n
    zero = torch.zeros((), dtype=torch.float64, device=c.device)
    return -torch.where(c > 0, p * torch.log(p), zero).sum()


def entropies(hist):
    """(H_a, H_b, H_ab) in nats, 0-d float64 tensors on the histogram's device: -sum p ln p over the non-zero bins of the two marginals
    and of the joint histogram.  An empty histogram gives NaN."""
    if not isinstance(hist, torch.Tensor) or hist.dim() != 2 or hist.dtype.is_floating_point:
        raise ValueError("entropies expects the (bins_a, bins_b) integer tensor of joint_histogram")
    n = hist.sum().to(torch.float64)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=hist.device)
    return tuple(torch.where(n > 0, _entropy(c, n), nan) for c in (hist.sum(1), hist.sum(0), hist.reshape(-1)))


def _hist_of(fixed_or_hist, moving, kwargs):
    if moving is None:
        if kwargs:
            raise TypeError("a histogram takes no further arguments: %s" % sorted(kwargs))
        return fixed_or_hist
    return joint_histogram(fixed_or_hist, moving, **kwargs)


def mutual_information(fixed_or_hist, moving=None, **kwargs):
    """H_a + H_b - H_ab of a joint histogram, or of two volumes with joint_histogram's arguments -> 0-d float64 tensor."""
    ha, hb, hab = entropies(_hist_of(fixed_or_hist, moving, kwargs))
    return ha + hb - hab


def normalized_mutual_information(fixed_or_hist, moving=None, **kwargs):
    """(H_a + H_b) / H_ab (Studholme's normalisation: 1 for independent images, 2 for a one-to-one relation); NaN where H_ab = 0."""
    ha, hb, hab = entropies(_hist_of(fixed_or_hist, moving, kwargs))
    nan = torch.full((), float("nan"), dtype=torch.float64, device=hab.device)
    return torch.where(hab == 0, nan, (ha + hb) / hab)


RegistrationMI = collections.namedtuple("RegistrationMI", "mi_before mi_after nmi_before nmi_after")


def registration_mi(fixed, moving, disp, bins=32, mask=None, drop_outside=True):
    """Mutual information and its normalised form of (fixed, moving) and of (fixed, moving warped by disp), on ONE range, that of the
    unwarped pair: the multimodal twin of registration_ssim.  Device in, 0-d device tensors out; the warped volume is never written.
    fixed, moving (H, W, D); disp as for joint_histogram -> RegistrationMI(mi_before, mi_after, nmi_before, nmi_after)"""
    rng = value_range(fixed, moving, mask=mask)
    before = joint_histogram(fixed, moving, bins, mask=mask, value_range=rng)
    after = joint_histogram(fixed, moving, bins, disp=disp, mask=mask, value_range=rng, drop_outside=drop_outside)
    return RegistrationMI(mutual_information(before), mutual_information(after), normalized_mutual_information(before),
                          normalized_mutual_information(after))
