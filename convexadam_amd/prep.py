"""The nnU-Net preprocessing helpers of the reference under its names (src/convexAdam/convex_adam_utils.py:15-21, 142-170, 196-265;
again in self_configuring/convexAdam_hyper_util.py:295-420), on the kernels of csrc/prep.hip (include/convexadam_prep.h):

    nnUNetNorm, nnUNetNormProps, nnUNetCTnorm       convex_adam_utils.py:142-170   statistics + one elementwise kernel, nothing leaves the device
    create_nonzero_mask, get_bbox_from_mask         :240-259                       mask, hole filling by line sweeps, box by integer atomics
    crop_to_bbox                                    :262-265                       a slice (no kernel)
    compute_steps_for_sliding_window, get_gaussian  :196-237                       host tables
    pdist_squared                                   :15-21                         the torch operators of the reference, on x's device
    normalise_and_crop                              mask -> box -> crop -> normalisation of the crop in one call

The normalisers and the mask take tensors on the HIP device only: there is no CPU path.  float32 is the pinned dtype; other floating
dtypes are converted and the result is cast back, as MINDSSC does."""
import ctypes as C

import numpy as np
import torch

from ._lib import CVX_PREP_CLAMP, CVX_PREP_POSITIVE, call, f32c, ptr, require_device_tensor, scratch


def _volume(img, name):
    img = require_device_tensor(img, name)
    if not img.dtype.is_floating_point:
        raise TypeError("%s must be a floating-point tensor, got %s" % (name, img.dtype))
    return f32c(img)


def _stats(x, flags=0, clamp=(0.0, 0.0), quantiles=None, moments=False):
    """x: float32 contiguous device tensor.  -> the parameter block {mean, std, lo, hi} (4 float32 on the device) [, {count, mean, ss}
    as 3 float64 on the device]; nothing is downloaded."""
    n = x.numel()
    params = torch.empty(4, dtype=torch.float32, device=x.device)
    mom = torch.empty(3, dtype=torch.float64, device=x.device) if moments else None
    q = quantiles or (0.0, 0.0)
    call(x.device, "cvx_prep_stats_f32", ptr(x), n, flags, float(clamp[0]), float(clamp[1]), 2 if quantiles else 0, float(q[0]), float(q[1]),
         ptr(params), ptr(mom), *scratch(x.device, "cvx_prep_stats_workspace_bytes", n, required=True))
    return (params, mom) if moments else params


def _normalise(x, mode, params=None, host=None, out=None):
    """out: a contiguous float32 tensor of x's size to write into (a new one by default)"""
    if out is None:
        out = torch.empty_like(x)
    hp = (C.c_float * 4)(*host) if host is not None else None
    call(x.device, "cvx_prep_normalise_f32", ptr(x), x.numel(), ptr(params), hp, mode, ptr(out))
    return out


def _like(out, img):
    out = out.view(img.shape)
    return out if img.dtype == torch.float32 else out.to(img.dtype)


def _norm_positive(x, out=None):
    return _normalise(x, 1, params=_stats(x, CVX_PREP_POSITIVE), out=out)


def _norm_ct(x, out=None):
    return _normalise(x, 0, params=_stats(x, CVX_PREP_CLAMP, (-1000.0, 1500.0), (0.005, 0.995)), out=out)


def nnUNetNorm(img):
    """(img - mean) / (std + 1e-8) with the mean and standard deviation of the voxels > 0, zero elsewhere.  (convex_adam_utils.py:142-148)
    Device tensor of any shape in, a new tensor out.  No positive voxel: all zero; exactly one: NaN there (its std is NaN, as in torch)."""
    return _like(_norm_positive(_volume(img, "img")), img)


def nnUNetNormProps(img, props):
    """(clamp(img, percentile_00_5, percentile_99_5) - mean) / sd with the four numbers of `props`.  (convex_adam_utils.py:151-159)"""
    x = _volume(img, "img")
    host = [float(props['mean']), float(props['sd']), float(props['percentile_00_5']), float(props['percentile_99_5'])]
    return _like(_normalise(x, 0, host=host), img)


def nnUNetCTnorm(img):
    """clamp to [-1000, 1500]; mean, std and the 0.005 / 0.995 quantiles of that; clamp to the quantiles; (x - mean) / std.
    (convex_adam_utils.py:162-170)  The volume is read four times and written once, and no number leaves the device in between.
    The one extension: more than 2^24 elements are accepted, where the reference's torch.quantile raises -- the rank is then
    float64(float32(q)) * (n - 1) in float64 and the interpolation weight is rounded to float32 (below that size the rank is
    torch's float32(q) * float32(n - 1))."""
    return _like(_norm_ct(_volume(img, "img")), img)


# ---- mask, box, crop --------------------------------------------------------------------------------------------------------------
def _nonzero_mask(data):
    """data (C, X, Y, Z) / (C, X, Y) device tensor -> (bool mask, int32[6] box on the device, rounds of the hole filling)."""
    data = require_device_tensor(data, "data")
    if data.dtype != torch.float32:                 # `!= 0` is decided in data's own dtype (a float64 1e-60 is not zero)
        data = (data != 0).to(torch.float32)
    x = data.detach().contiguous()
    shape = tuple(int(s) for s in x.shape[1:])
    ndim = len(shape)
    H, W, D = ((1,) + shape) if ndim == 2 else shape
    mask = torch.empty(shape, dtype=torch.uint8, device=x.device)
    box = torch.empty(6, dtype=torch.int32, device=x.device)
    rounds = C.c_int(0)
    call(x.device, "cvx_prep_nonzero_mask_u8", ptr(x), int(x.shape[0]), H, W, D, ndim, ptr(mask), ptr(box), None, C.byref(rounds),
         *scratch(x.device, "cvx_prep_nonzero_mask_workspace_bytes", H, W, D, required=True))
    return mask.view(torch.bool), box, int(rounds.value)


def create_nonzero_mask(data):
    """OR over the channels of data[c] != 0 with its holes filled (scipy.ndimage.binary_fill_holes' result).  (convex_adam_utils.py:240-248)
    numpy in -> numpy bool out (through the device), device tensor in -> device bool tensor out."""
    assert len(data.shape) == 4 or len(data.shape) == 3, "data must have shape (C, X, Y, Z) or shape (C, X, Y)"
    if isinstance(data, np.ndarray):
        return _nonzero_mask(torch.from_numpy(np.ascontiguousarray(data != 0).astype(np.float32)).to("cuda"))[0].cpu().numpy()
    return _nonzero_mask(data)[0]


def _box_list(box6):
    b = [int(v) for v in box6.cpu().tolist()]           # 24 bytes
    if b[1] == 0:
        raise ValueError("zero-size array to reduction operation minimum which has no identity")      # np.min of no coordinates
    return [[b[0], b[1]], [b[2], b[3]], [b[4], b[5]]]


def get_bbox_from_mask(mask, outside_value=0):
    """[[lo, hi], [lo, hi], [lo, hi]]: per axis the smallest index with mask != outside_value and the largest plus 1, as Python ints.
    (convex_adam_utils.py:251-259)  A device tensor is reduced on the device and 24 bytes are downloaded; an empty mask raises
    ValueError, as np.min of an empty array does."""
    if isinstance(mask, np.ndarray):
        c = np.where(mask != outside_value)
        return [[int(np.min(c[a])), int(np.max(c[a])) + 1] for a in range(3)]
    mask = require_device_tensor(mask, "mask")
    if mask.dim() != 3:
        raise ValueError("get_bbox_from_mask expects a 3-d mask, got %s" % (tuple(mask.shape),))
    if mask.dtype == torch.bool and outside_value == 0 and mask.is_contiguous():
        m = mask.view(torch.uint8)                  # a bool tensor's bytes are the mask already
    else:
        m = (mask != outside_value).to(torch.uint8).contiguous()
    box = torch.empty(6, dtype=torch.int32, device=m.device)
    H, W, D = [int(s) for s in m.shape]
    call(m.device, "cvx_prep_mask_bbox_i32", ptr(m), H, W, D, ptr(box), None)
    return _box_list(box)


def crop_to_bbox(image, bbox):
    """The part of a 3-d numpy array or tensor inside bbox = [[lo, hi]] * 3 (a view).  (convex_adam_utils.py:262-265)"""
    assert len(image.shape) == 3, "crop_to_bbox only supports 3d images, got shape %s" % (tuple(image.shape),)
    (z0, z1), (y0, y1), (x0, x1) = bbox
    return image[z0:z1, y0:y1, x0:x1]


def normalise_and_crop(img, kind='ct'):
    """Non-zero mask -> box -> crop -> normalisation of the crop: img (X, Y, Z) or (C, X, Y, Z) on the device -> (normalised crop, bbox).
    kind 'ct' = nnUNetCTnorm, 'nonzero' = nnUNetNorm, per channel.  Between the steps only the six box integers leave the device; a
    channel's crop is gathered once and its normalisation is written straight into the result."""
    if kind not in ('ct', 'nonzero'):
        raise ValueError("normalise_and_crop: kind must be 'ct' or 'nonzero', got %r" % (kind,))
    img = require_device_tensor(img, "img")
    if img.dim() not in (3, 4):
        raise ValueError("normalise_and_crop expects (X, Y, Z) or (C, X, Y, Z), got %s" % (tuple(img.shape),))
    data = img if img.dim() == 4 else img.unsqueeze(0)
    bbox = _box_list(_nonzero_mask(data)[1])
    norm = _norm_ct if kind == 'ct' else _norm_positive
    out = torch.empty((int(data.shape[0]),) + tuple(hi - lo for lo, hi in bbox), dtype=torch.float32, device=data.device)
    for c in range(data.shape[0]):
        norm(_volume(crop_to_bbox(data[c], bbox), "img"), out=out[c])
    if img.dtype != torch.float32:
        out = out.to(img.dtype)
    return (out if img.dim() == 4 else out[0]), bbox


# ---- host tables ------------------------------------------------------------------------------------------------------------------
def compute_steps_for_sliding_window(patch_size, image_size, step_size=.5):
    """Start coordinates of the sliding windows, one list per axis.  (convex_adam_utils.py:196-221)  Per axis: the last window starts at
    room = image - patch; windows = ceil(room / (patch * step_size)) + 1, so that neighbours are at most patch * step_size apart; the
    starts are round(i * room / (windows - 1)) with numpy's rounding (half to even); one window starts at 0.  Host integers."""
    starts = []
    for patch, size in zip(patch_size, image_size):
        room = size - patch
        windows = int(np.ceil(room / (patch * step_size))) + 1
        stride = room / (windows - 1) if windows > 1 else 0.0
        starts.append([int(np.round(stride * i)) for i in range(windows)])
    return starts


def gaussian_kernel1d(sigma, n):
    """The 1-d kernel scipy.ndimage.gaussian_filter applies (order 0, truncate 4) to a unit impulse at n // 2 of a line of n zeros
    (mode 'constant'): exp(-0.5 / sigma^2 x^2) / sum over x = -r .. r, r = int(4 sigma + 0.5), cut to the line."""
    radius = int(4.0 * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    line = np.zeros(n)
    c = n // 2
    for i in range(n):
        if abs(i - c) <= radius:
            line[i] = phi[i - c + radius]
    return line


def get_gaussian(patch_size, sigma_scale=1. / 8, device='cuda'):
    """The Gaussian importance map of a patch, (1, 1, *patch_size) half.  (convex_adam_utils.py:224-237)  Bit for bit the reference's table:
    the float64 products fl(fl(k0[i] k1[j]) k2[k]) of the 1-d kernels, divided by the maximum, cast to float32, zeros replaced by the
    smallest non-zero value, cast to half (which underflows the far tail back to zero, as in the reference).  A table built once per run
    on the host; device='cpu' is allowed."""
    ks = [gaussian_kernel1d(n * sigma_scale, n) for n in patch_size]
    g = ks[0]
    for k in ks[1:]:
        g = g[..., None] * k
    table = (g / g.max()).astype(np.float32)
    nonzero = table > 0
    table = np.where(nonzero, table, table[nonzero].min())                 # a weight of zero would divide by zero downstream
    return torch.from_numpy(table).to(torch.float16).reshape((1, 1) + table.shape).to(device)


def pdist_squared(x):
    """Pairwise squared distances of the N columns of x (B, C, N) -> (B, N, N), as |a|^2 + |b|^2 - 2 a.b with NaN entries set to 0 and
    negative ones (cancellation) to 0.  (convex_adam_utils.py:15-21)  Torch operators on whatever device x is on."""
    norms = x.pow(2).sum(dim=1)                                             # (B, N)
    gram = torch.bmm(x.transpose(1, 2), x)                                  # (B, N, N)
    dist = norms[:, :, None] + norms[:, None, :] - 2.0 * gram
    dist = torch.where(torch.isnan(dist), torch.zeros_like(dist), dist)
    return dist.clamp_min(0.0)
