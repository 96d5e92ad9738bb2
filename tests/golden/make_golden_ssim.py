"""Captures tests/golden/ssim.npz from the upstream reference (build container only, like make_golden.py):

    python tests/golden/make_golden_ssim.py

Runs the reference's own tests/helper_functions.py::ssim3D on the cases of tests/ssim_golden.py, in float32 and -- on .double() inputs --
in float64, and stores per (case, window size):
    r32, r64        the two means (size_average=True)
    s32, s64        the two slice means (size_average=False), shape (N, D)
    m64             the float64 map (the reference's expression, re-evaluated with the reference's own window: the function returns no map)
    E_map, E_mean, E_slice   the reference's own float32 distance from its float64 result: max |m32 - m64|, |r32 - r64|, max |s32 - s64|
The inputs are not stored (tests/ssim_golden.py regenerates them from seeds).  Before the file is written, a float32 SEPARABLE evaluation
(conv3d along D, then W, then H with the 1-D window) must meet the bounds tests/test_gpu_ssim.py holds the kernel to: they are
attainable by the kernel's kind of arithmetic before a device sees them."""
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ssim_golden  # noqa: E402
from _ref_import import REF_ROOT  # noqa: E402


def reference_helpers():
    if "SimpleITK" not in sys.modules:
        sys.modules["SimpleITK"] = types.ModuleType("SimpleITK")
    if not hasattr(sys.modules["SimpleITK"], "Image"):
        sys.modules["SimpleITK"].Image = type("Image", (), {})
    sys.path.insert(0, os.path.join(REF_ROOT, "tests"))
    return importlib.import_module("helper_functions")


def separable_f32(ref, x, y, ws):
    """float32, three 1-D passes (D, W, H) per moment with the reference's 1-D window."""
    c = x.shape[1]
    g = ref.gaussian(ws, 1.5)

    def filt(v):
        v = F.conv3d(v, g.view(1, 1, 1, 1, ws).expand(c, 1, 1, 1, ws).contiguous(), padding=(0, 0, ws // 2), groups=c)
        v = F.conv3d(v, g.view(1, 1, 1, ws, 1).expand(c, 1, 1, ws, 1).contiguous(), padding=(0, ws // 2, 0), groups=c)
        return F.conv3d(v, g.view(1, 1, ws, 1, 1).expand(c, 1, ws, 1, 1).contiguous(), padding=(ws // 2, 0, 0), groups=c)

    mu1, mu2 = filt(x), filt(y)
    m11, m22, m12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = filt(x * x) - m11, filt(y * y) - m22, filt(x * y) - m12
    c1, c2 = np.float32(0.01 ** 2), np.float32(0.03 ** 2)
    m = ((2 * m12 + c1) * (2 * s12 + c2)) / ((m11 + m22 + c1) * (s1 + s2 + c2))
    md = m.double()
    return md.numpy(), float(md.mean().float()), md.mean(1).mean(1).mean(1).float().numpy()


def ref_map(ref, x, y, ws):
    """_ssim_3D's map (helper_functions.py:115-130) with the reference's own window builder, in the dtype of x."""
    c = x.shape[1]
    win = ref.create_window_3D(ws, c).type_as(x)
    conv = lambda v: F.conv3d(v, win, padding=ws // 2, groups=c)      # noqa: E731
    mu1, mu2 = conv(x), conv(y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1, s2, s12 = conv(x * x) - mu1_sq, conv(y * y) - mu2_sq, conv(x * y) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2                                     # noqa: N806
    return ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))


def main():
    torch.set_num_threads(8)
    ref = reference_helpers()
    out = {}
    for name, wss in ssim_golden.CASES:
        x, y = ssim_golden.inputs(name)
        for ws in wss:
            r32, s32 = ref.ssim3D(x, y, ws, True), ref.ssim3D(x, y, ws, False)
            r64, s64 = ref.ssim3D(x.double(), y.double(), ws, True), ref.ssim3D(x.double(), y.double(), ws, False)
            m32, m64 = ref_map(ref, x, y, ws), ref_map(ref, x.double(), y.double(), ws)
            assert m32.mean() == r32 and m64.mean() == r64, "the map restatement is not the reference's map"
            e_map = float((m32.double() - m64).abs().max())
            e_mean = abs(float(r32) - float(r64))
            e_slice = float((s32.double() - s64).abs().max())
            sm, sr, ss = separable_f32(ref, x, y, ws)
            d_map, d_mean, d_slice = np.abs(sm - m64.numpy()).max(), abs(sr - float(r64)), np.abs(ss.astype(np.float64) - s64.numpy()).max()
            print("%-8s ws %2d  r64 %.9f  E_map %.3g E_mean %.3g E_slice %.3g | separable float32: %.3g %.3g %.3g" % (
                name, ws, float(r64), e_map, e_mean, e_slice, d_map, d_mean, d_slice))
            assert d_map <= e_map + 2.0 ** -20 and d_mean <= e_mean + 2.0 ** -22 and d_slice <= e_slice + 2.0 ** -22, "bounds not attainable"
            k = lambda f: ssim_golden.key(name, ws, f)                # noqa: E731
            out[k("r32")], out[k("r64")] = np.float32(r32), np.float64(r64)
            out[k("s32")], out[k("s64")] = s32.numpy(), s64.numpy()
            out[k("m64")] = m64.numpy()
            out[k("E_map")], out[k("E_mean")], out[k("E_slice")] = np.float64(e_map), np.float64(e_mean), np.float64(e_slice)
    path = os.path.join(HERE, "ssim.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
