"""3-D structural similarity on the HIP device: the reference tests' acceptance criterion (tests/helper_functions.py:102-145,
used as `ssim3D(warped, expected) > 0.95` by tests/test_convex_adam_mind.py:45-85) as one fused kernel (csrc/ssim.hip).

    gaussian(window_size, sigma), create_window_3D(window_size, channel)   the reference's window builders (tensors, any device)
    ssim3D(img1, img2, window_size=11, size_average=True)                  0-d device tensor, or (N, D) for size_average=False
    ssim3D_map(img1, img2, window_size=11)                                 the (N, C, H, W, D) map
    registration_ssim(fixed, moving, disp, window_size=11)                 ssim3D(fixed, moving warped by disp), all on the device

Inputs are (N, C, H, W, D) device tensors; every (n, c) volume is filtered on its own (the reference's groups=channel).  The window is
the outer product of a 1-D Gaussian (sigma 1.5), so the kernel filters the five moments x, y, xx, yy, xy along D, W and H in turn; padding
is zeros and the border is not renormalised, exactly as F.conv3d(padding=window_size // 2).  window_size must be odd and at most 11: an
even window makes the reference's output one voxel larger per axis, a larger one adds taps below 1e-6; both raise, nothing is routed to
another implementation.  Nothing here synchronises with the host.
"""
import torch

from ._lib import call, f32c, ptr, require_device_tensor, scratch

# (shortest H chunk, W tile, D tile) of csrc/ssim.hip: SSIM_MIN_HCHUNK, SSIM_TW, SSIM_TD.  A workgroup owns a W x D tile and walks a chunk
# of H; results do not depend on any of the three (tests/test_gpu_ssim.py walks the extents around them)
TILE = (16, 16, 32)


def gaussian(window_size, sigma):
    """helper_functions.py:102-105, operation for operation (float32)."""
    x = torch.arange(window_size, dtype=torch.float32) - window_size // 2
    gauss = torch.exp(-x ** 2 / (2 * sigma ** 2))
    return gauss / gauss.sum()


def create_window_3D(window_size, channel):  # noqa: N802  (the reference's name)
    """helper_functions.py:107-112: the (channel, 1, ws, ws, ws) float32 window the reference convolves with.  The kernel does not read
    it (it filters with the 1-D weights, computed in float64 and rounded once); it is here for code written against the helper file."""
    w1 = gaussian(window_size, 1.5).unsqueeze(1)
    w2 = w1.mm(w1.t())
    w3 = w1.mm(w2.reshape(1, -1)).reshape(window_size, window_size, window_size).float().unsqueeze(0).unsqueeze(0)
    return w3.expand(channel, 1, window_size, window_size, window_size).contiguous()


def _pair(img1, img2):
    require_device_tensor(img1, "img1")
    require_device_tensor(img2, "img2")
    if img1.dim() != 5 or img1.shape != img2.shape:
        raise ValueError("ssim3D expects two (N, C, H, W, D) tensors of equal shape, got %s and %s" % (tuple(img1.shape), tuple(img2.shape)))
    if img1.device != img2.device:
        raise ValueError("ssim3D: img1 on %s, img2 on %s" % (img1.device, img2.device))
    return f32c(img1), f32c(img2)


def _run(img1, img2, window_size, want_map=False, want_mean=False, want_slices=False):
    a, b = _pair(img1, img2)
    dev = a.device
    n, c, h, w, d = [int(v) for v in a.shape]
    ws = int(window_size)
    out_map = torch.empty_like(a) if want_map else None
    mean = torch.empty((), dtype=torch.float32, device=dev) if want_mean else None
    slices = torch.empty((n, d), dtype=torch.float32, device=dev) if want_slices else None
    # (only the means need scratch; a refused window answers 0 and the call says why)
    buf = scratch(dev, "cvx_ssim3d_workspace_bytes", n, c, h, w, d, ws) if (want_mean or want_slices) else (None, 0)
    call(dev, "cvx_ssim3d_f32", ptr(a), ptr(b), n, c, h, w, d, ws, ptr(out_map), ptr(mean), ptr(slices), *buf)
    return out_map, mean, slices


def ssim3D(img1, img2, window_size=11, size_average=True):  # noqa: N802  (the reference's name)
    """helper_functions.py:137-145.  size_average=True: the mean of the map over everything, a 0-d device tensor.
    size_average=False: the reference evaluates `ssim_map.mean(1).mean(1).mean(1)` on the 5-D map, which removes C, H and W and
    leaves shape (N, D) -- the mean over channel, H and W for every index of the LAST axis, not one value per sample.  That is what
    the reference returns, so that is what this returns.  Both are float64 sums added in a fixed order: the same bits on every run."""
    _, mean, slices = _run(img1, img2, window_size, want_mean=bool(size_average), want_slices=not size_average)
    return mean if size_average else slices


def ssim3D_map(img1, img2, window_size=11):  # noqa: N802
    """The (N, C, H, W, D) ssim map (`ssim_map` of helper_functions.py:130)."""
    return _run(img1, img2, window_size, want_map=True)[0]


def warp_device(moving, disp):
    """apply_convex(disp, moving) without the host: moving (H, W, D) device tensor, disp (3, H, W, D) as register_pair_device returns it
    or (H, W, D, 3) as convex_adam_pt does (voxels) -> the warped volume, float32, on the device.  The interpolation is apply_convex's
    own kernel and runs in float64 like scipy's map_coordinates."""
    require_device_tensor(moving, "moving")
    require_device_tensor(disp, "disp")
    if moving.dim() != 3:
        raise ValueError("warp_device: moving must be (H, W, D)")
    shape = tuple(moving.shape)
    if disp.dim() == 4 and tuple(disp.shape) == shape + (3,):
        field = disp
    elif disp.dim() == 4 and tuple(disp.shape) == (3,) + shape:
        field = disp.permute(1, 2, 3, 0)
    else:
        raise ValueError("warp_device: disp must be (3, H, W, D) or (H, W, D, 3) matching moving %s, got %s" % (shape, tuple(disp.shape)))
    dev = moving.device
    m = moving.detach().to(torch.float64).contiguous()
    f = field.detach().to(dev, torch.float64).contiguous()
    out = torch.empty_like(m)
    call(dev, "cvx_map_coordinates_linear_f64", ptr(m), ptr(f), shape[0], shape[1], shape[2], ptr(out))
    return out.to(torch.float32)


def registration_ssim(fixed, moving, disp, window_size=11):
    """ssim3D(fixed, moving warped by disp): the reference test's criterion for a finished registration, device in, 0-d device tensor
    out, no host round trip.  fixed, moving (H, W, D); disp as for warp_device."""
    require_device_tensor(fixed, "fixed")
    if fixed.dim() != 3 or fixed.shape != moving.shape:
        raise ValueError("registration_ssim expects two (H, W, D) volumes of equal shape")
    return ssim3D(fixed[None, None], warp_device(moving, disp)[None, None], window_size=window_size)
