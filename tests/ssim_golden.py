"""Cases of tests/golden/ssim.npz (captured from the reference's tests/helper_functions.py::ssim3D by golden/make_golden_ssim.py).

The fixture stores the reference's results, not the inputs: those are regenerated here from seeds with convexadam_amd.phantom and
torch's CPU generator, which give the same volumes on every host."""
import torch

from convexadam_amd.phantom import phantom

# (case name, window sizes)
CASES = [("phantom", (11,)), ("unit", (11, 7)), ("cancel", (11,)), ("tiny", (11, 3)), ("long", (11,)), ("batch", (11, 1))]


def _pair(shape, seed, noise_a, noise_b):
    x = phantom(shape, seed, noise_a)
    y = torch.roll(phantom(shape, seed, noise_b), shifts=(1, 0, -1), dims=(0, 1, 2))
    return x[None, None].contiguous(), y[None, None].contiguous()


def inputs(name):
    """(img1, img2), float32 CPU tensors (N, C, H, W, D)."""
    if name == "phantom":                      # a phantom against its second noise realisation, rolled by (1, 0, -1)
        return _pair((24, 20, 28), 1, 10, 11)
    if name == "unit":                         # the same pair rescaled to [0, 1]: the range C1 and C2 are meant for
        x, y = _pair((24, 20, 28), 1, 10, 11)
        lo, hi = torch.minimum(x.min(), y.min()), torch.maximum(x.max(), y.max())
        return ((x - lo) / (hi - lo)).contiguous(), ((y - lo) / (hi - lo)).contiguous()
    if name == "cancel":                       # large offset: G*(xx) - mu mu cancels seven digits
        x, y = _pair((24, 20, 28), 1, 10, 11)
        return (50.0 * x + 1000.0).contiguous(), (50.0 * y + 1000.0).contiguous()
    if name == "tiny":                         # smaller than the window on every axis
        return _pair((5, 4, 3), 2, 20, 21)
    if name == "long":                         # more than one tile along W and D
        return _pair((12, 33, 65), 3, 30, 31)
    if name == "batch":
        g = torch.Generator().manual_seed(6)
        x = torch.rand(2, 3, 9, 10, 13, generator=g)
        return x.contiguous(), (x + 0.1 * torch.randn(2, 3, 9, 10, 13, generator=g)).contiguous()
    raise KeyError(name)


def key(name, ws, field):
    return "%s_ws%d_%s" % (name, ws, field)
