"""Cost-volume confidence: the soft reading of the convex stage's cost volume on top of libconvexadam_hip.so.

correlate() and coupled_convex() keep hard argmins of the (2 hw + 1)^3 x h x w x d volume; soft_stats() reads the same volume as a
Boltzmann distribution per coarse cell, p_k ~ exp(-beta e_k), and returns its mean displacement, 3 x 3 covariance, partition sum and mean
excess energy in one call (cvx_soft_stats_f32, include/convexadam_soft.h): a sharp minimum has a small covariance, an edge a covariance
that is long in one direction (the aperture problem), homogeneous tissue a flat distribution with high entropy.  The helpers below unpack
the twelve channels; convex_confidence() runs the reference's convex stage and reads its volume around the regularised field.

Tensors must live on the HIP device; there is no CPU path.  Not built: a cell_mask variant, the certified (unscaled) volume
(correlate(mode="certified") holds 729 x the mean cost: divide beta by 729 to read it), feeding confidences into the rigid or affine
fits, and any default for beta."""
import torch

from . import _lib
from ._lib import call, f32c, ptr, require_device_tensor, scratch

CHANNELS = 12


def soft_stats(ssd, disp_hw, beta, field=None, coupling=0.0, return_info=False):
    """Soft statistics of a cost volume -> (12, h, w, d) float32 device tensor.

    ssd       (n^3, h, w, d) float32 or float16 device tensor, n = 2 disp_hw + 1, as correlate() returns it (read where it lies)
    beta      inverse temperature in units of 1 / cost, > 0.  It has no default because the scale of the costs depends on the features:
              channel 11 of the result is each cell's minimum cost and channel 9 the partition sum Z, whose reciprocal is the weight of
              the best displacement.  A beta around 1 / (typical spread of the costs above the minimum) gives Z well between 1 (the
              best displacement takes everything: beta too large to say anything about uncertainty) and n^3 (all displacements alike:
              beta too small); try one, look at the median of Z, and scale beta accordingly.
    field     None, or a (3, h, w, d) / (1, 3, h, w, d) field in coarse voxels (what coupled_convex returns): the statistics are then those
              of the coupled energy e_k + coupling * |delta_k - field|^2, coupling >= 0
    Channels  0..2 mean displacement (the order of disp_mesh: component 0 runs fastest in k), 3..8 covariance (00, 01, 02, 11, 12, 22),
              9 Z, 10 mean excess energy sum_k p_k (e_k - min), 11 min_k e_k.  A cell whose column holds a NaN or a -Inf, or nothing
              but +Inf, is NaN in all channels; +Inf entries beside finite ones weigh nothing.
    return_info   also dict(non_finite=number of such cells) (one device-to-host copy)"""
    ssd = require_device_tensor(ssd, "ssd")
    if ssd.dim() != 4:
        raise ValueError("soft_stats: ssd must be (n^3, h, w, d), got %s" % (tuple(ssd.shape),))
    hw = int(disp_hw)
    K, h, w, d = (int(s) for s in ssd.shape)
    if K != (2 * hw + 1) ** 3:
        raise ValueError("soft_stats: ssd holds %d displacements, disp_hw = %d needs %d" % (K, hw, (2 * hw + 1) ** 3))
    half = ssd.dtype == torch.float16
    s = ssd.detach().contiguous() if half else f32c(ssd)
    u = None
    if field is not None:
        field = require_device_tensor(field, "field")
        if tuple(field.shape) not in ((3, h, w, d), (1, 3, h, w, d)):
            raise ValueError("soft_stats: field must be (3, %d, %d, %d), got %s" % (h, w, d, tuple(field.shape)))
        u = f32c(field.to(s.device))
    elif float(coupling) != 0.0:
        raise ValueError("soft_stats: a coupling of %g needs a field" % float(coupling))
    _lib.soft_lib()
    out = torch.empty((CHANNELS, h, w, d), dtype=torch.float32, device=s.device)
    bad = torch.empty(1, dtype=torch.int64, device=s.device)
    call(s.device, "cvx_soft_stats_f32", ptr(s), int(half), ptr(u), float(coupling), float(beta), h, w, d, hw, ptr(out), ptr(bad),
         *scratch(s.device, "cvx_soft_stats_workspace_bytes", h, w, d, hw, required=True,
                  otherwise="cvx_soft_stats: bad extent (%dx%dx%d), disp_hw %d, or a volume of 2^31 entries or more" % (h, w, d, hw)))
    if return_info:
        return out, dict(non_finite=int(bad.item()))
    return out


def _stats(stats):
    if not isinstance(stats, torch.Tensor) or stats.dim() != 4 or stats.shape[0] != CHANNELS:
        raise ValueError("expected the (12, h, w, d) tensor of soft_stats")
    return stats


def soft_displacement(stats):
    """The mean displacement as a field, (1, 3, h, w, d) in coarse voxels: the soft counterpart of coupled_convex's result."""
    return _stats(stats)[0:3].unsqueeze(0)


def soft_covariance(stats):
    """(h, w, d, 3, 3), symmetric: the covariance of the displacement per cell, in coarse voxels squared."""
    s = _stats(stats)
    return s[[3, 4, 5, 4, 6, 7, 5, 7, 8]].permute(1, 2, 3, 0).reshape(tuple(s.shape[1:]) + (3, 3))


def soft_entropy(stats, beta):
    """(h, w, d) float64: the entropy ln Z + beta E / Z of the weights in nats, between 0 (one displacement) and ln n^3 (all alike).
    `beta` is the one given to soft_stats (it is read as float32, like there)."""
    s = _stats(stats)
    b = float(torch.tensor(float(beta), dtype=torch.float32))
    return torch.log(s[9].to(torch.float64)) + b * s[10].to(torch.float64)


def soft_sigma(stats, grid_sp):
    """(h, w, d): sqrt(trace cov) * grid_sp, the standard deviation of the displacement in voxels of the image grid."""
    s = _stats(stats)
    return torch.sqrt(s[3] + s[6] + s[8]) * float(grid_sp)


class Confidence:
    """What convex_confidence returns: `field` (1, 3, h, w, d) the convex stage's coarse field in coarse voxels, `stats` the (12, h, w, d)
    soft statistics around it, `beta`, `grid_sp`, and with full_res `sigma` / `entropy` (H, W, D) on the image grid (None otherwise)."""

    def __init__(self, field, stats, beta, grid_sp, sigma=None, entropy=None):
        self.field, self.stats, self.beta, self.grid_sp, self.sigma, self.entropy = field, stats, beta, grid_sp, sigma, entropy

    def displacement(self):
        return soft_displacement(self.stats)

    def covariance(self):
        return soft_covariance(self.stats)


def convex_confidence(img_fixed, img_moving, beta, mind_r=1, mind_d=2, grid_sp=6, disp_hw=4, coupling=1.0, full_res=True):
    """The reference's convex stage on two (H, W, D) device images and the soft reading of its cost volume: MIND-SSC features, pooling by
    grid_sp, the exact float32 cost volume, coupled_convex, then soft_stats of the coupled energy around that field (`coupling`: the last
    coefficient of the reference's schedule, 1.0; 0 reads the data term alone).  Every step is a device operator of this package; nothing
    returns to the host.  full_res: sigma and entropy up-sampled to the image grid by resize_trilinear.  -> Confidence"""
    from .convex_adam_MIND import extract_features
    from .convex_adam_utils import avg_pool, correlate, coupled_convex, disp_mesh_t, resize_trilinear
    img_fixed = require_device_tensor(img_fixed, "img_fixed")
    img_moving = require_device_tensor(img_moving, "img_moving")
    if img_fixed.dim() != 3 or img_fixed.shape != img_moving.shape:
        raise ValueError("convex_confidence expects two (H, W, D) volumes of equal shape")
    dev = img_fixed.device
    H, W, D = (int(s) for s in img_fixed.shape)
    ff, fm = extract_features(img_fixed, img_moving, mind_r, mind_d, False, None, None, device=dev, dtype=torch.float32)
    ff, fm = avg_pool(ff, grid_sp), avg_pool(fm, grid_sp)
    ssd, am = correlate(ff, fm, disp_hw, grid_sp, (H, W, D), int(ff.shape[1]))
    field = coupled_convex(ssd, am, disp_mesh_t(disp_hw, dev), grid_sp, (H, W, D))
    stats = soft_stats(ssd, disp_hw, beta, field=field, coupling=coupling)
    sigma = entropy = None
    if full_res:
        both = torch.stack([soft_sigma(stats, grid_sp), soft_entropy(stats, beta).to(torch.float32)]).unsqueeze(0)
        up = resize_trilinear(both, (H, W, D))
        sigma, entropy = up[0, 0], up[0, 1]
    return Confidence(field, stats, float(beta), int(grid_sp), sigma, entropy)
