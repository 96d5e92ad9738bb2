"""Multi-channel (label / nnUNet feature) variant, mirror of the reference's
`convexAdam.convex_adam_nnUNet` (src/convexAdam/convex_adam_nnUNet.py): extract_features (:19-38) and
convex_adam (:41-159).  The weighted one-hot features are built by HIP kernels (label histogram,
expansion) and the registration itself is the same C-ABI pipeline with C = number of labels present;
the registration entries write only the features' two stride poolings, straight from the label maps.
The reference stores features in fp16; this engine keeps float32 throughout.
"""
import ctypes as C
import os
import time

import numpy as np
import torch

from ._lib import call, f32c, lib, ptr, require_device_tensor
from .convex_adam_MIND import _register_device, _require_hip, register_pair_device  # noqa: F401  (register_pair_device: the feature entry, re-exported)


def _label_channels(pred_fixed, pred_moving, device):
    """Two label maps -> (lf, lm, present_d, weights_d, C): the maps as float32 device tensors, the labels present in either map
    (ascending, int32) and their weights w_c = (n_c_fix + n_c_mov + eps)^-0.3 normalised to mean 1 (convex_adam_nnUNet.py:24-33):
    histograms on the device, the weights by cvx_label_weights_host."""
    device = torch.device(device if device is not None else "cuda")
    lf = require_device_tensor(f32c(pred_fixed.to(device)), "pred_fixed")
    lm = require_device_tensor(f32c(pred_moving.to(device)), "pred_moving")
    max_label = int(max(float(lf.max()), float(lm.max())))
    hist = torch.zeros((2, max_label + 1), dtype=torch.int64, device=device)
    for lab, h in ((lf, hist[0]), (lm, hist[1])):
        call(device, "cvx_label_histogram_i64", ptr(lab), lab.numel(), max_label, ptr(h))
    h_host = hist.cpu().numpy()
    present = np.zeros(max_label + 1, np.int32)
    weights = np.zeros(max_label + 1, np.float32)
    Cn = lib().cvx_label_weights_host(h_host[0].ctypes.data_as(C.c_void_p), h_host[1].ctypes.data_as(C.c_void_p), max_label,
                                      present.ctypes.data_as(C.c_void_p), weights.ctypes.data_as(C.c_void_p))
    present_d = torch.from_numpy(present[:Cn].copy()).to(device)
    weights_d = torch.from_numpy(weights[:Cn].copy()).to(device)
    return lf, lm, present_d, weights_d, Cn


def extract_features(pred_fixed, pred_moving, mult=10.0, device=None):
    """Label maps (H,W,D) -> weighted one-hot features (1,C,H,W,D) x 2; C = labels present in either map,
    w_c = (n_c_fix + n_c_mov + eps)^-0.3 normalised to mean 1, features = mult * w_c * onehot.
    (convex_adam_nnUNet.py:19-38; `mult` = 10 there, a parameter in self_configuring/convexAdam_hyper_util.py:64-83)"""
    lf, lm, present_d, weights_d, Cn = _label_channels(pred_fixed, pred_moving, device)
    device = lf.device
    H, W, D = [int(s) for s in lf.shape[-3:]]
    V = H * W * D
    ff = torch.empty((1, Cn, H, W, D), dtype=torch.float32, device=device)
    fm = torch.empty_like(ff)
    for lab, out in ((lf, ff), (lm, fm)):
        call(device, "cvx_label_features_f32", ptr(lab), V, Cn, ptr(present_d), ptr(weights_d), float(mult), ptr(out))
    return ff, fm


def label_features_pooled(pred_fixed, pred_moving, g1, g2=0, mult=10.0, device=None):
    """avg_pool3d(extract_features(...), g, stride=g) for the window g1 and, g2 > 0, for g2 as well, without the one-hot volumes
    (cvx_label_features_pooled_f32; the same bits): ((f1, m1), (f2, m2) or None), each (C, H//g, W//g, D//g) float32."""
    lf, lm, present_d, weights_d, Cn = _label_channels(pred_fixed, pred_moving, device)
    device = lf.device
    H, W, D = [int(s) for s in lf.shape[-3:]]
    g1, g2 = int(g1), int(g2)
    if g1 < 1 or g2 < 0:
        raise ValueError("label_features_pooled: pooling windows must be g1 >= 1 and g2 >= 0 (0: no second output)")
    shape = lambda g: (Cn, H // g, W // g, D // g)
    res = []
    for lab in (lf, lm):
        o1 = torch.empty(shape(g1), dtype=torch.float32, device=device)
        o2 = torch.empty(shape(g2), dtype=torch.float32, device=device) if g2 > 0 else None
        call(device, "cvx_label_features_pooled_f32", ptr(lab), H, W, D, Cn, ptr(present_d), ptr(weights_d), float(mult), g1, ptr(o1), g2, ptr(o2))
        res.append((o1, o2))
    return (res[0][0], res[1][0]), ((res[0][1], res[1][1]) if g2 > 0 else None)


def register_labels_device(pred_fixed, pred_moving, mult=10.0, lambda_weight=1.25, grid_sp=6, disp_hw=4, selected_niter=80, selected_smooth=0,
                           grid_sp_adam=2, ic=True, cost_scale=12.0, out=None, profile=None, cost="ssd", n_box=2, n_spline_pools=3,
                           corr_mode="exact", storage="fp32", adam_mode=None):
    """One registration from two (H,W,D) label maps, device out: the field register_pair_device(feat_fixed=, feat_moving=) returns for
    extract_features(pred_fixed, pred_moving, mult), bit for bit and with the same options, through cvx_register_label_pair_f32 -- the
    pooled features are written straight from the maps, the (C,H,W,D) one-hot volumes never exist."""
    if pred_fixed.dim() < 3 or pred_fixed.shape != pred_moving.shape or pred_fixed.numel() != pred_fixed.shape[-3:].numel():
        raise ValueError("register_labels_device expects two (H,W,D) label maps of equal shape")
    lf, lm, present_d, weights_d, Cn = _label_channels(pred_fixed, pred_moving, pred_fixed.device if pred_fixed.device.type == "cuda" else None)
    H, W, D = [int(s) for s in lf.shape[-3:]]
    _require_hip(lf.device)
    return _register_device(
        "cvx_register_label_pair", (ptr(lf), ptr(lm), ptr(present_d), ptr(weights_d), float(mult)),
        lambda smooth, out_: register_labels_device(lf, lm, mult, lambda_weight, grid_sp, disp_hw, selected_niter, smooth, grid_sp_adam, ic, cost_scale,
                                                    out_, profile, cost, n_box, n_spline_pools, corr_mode, storage, adam_mode),
        Cn, H, W, D, lf.device, 1, 2, lambda_weight, grid_sp, disp_hw, selected_niter, selected_smooth, grid_sp_adam, ic, cost_scale, out, profile,
        cost, n_box, n_spline_pools, corr_mode, storage, adam_mode)


def convex_adam_pt(pred_fixed, pred_moving, lambda_weight, grid_sp, disp_hw, selected_niter, selected_smooth,
                   grid_sp_adam=2, ic=True, device="cuda"):
    """Tensor-level entry: label maps in, np.ndarray (H,W,D,3) float64 out (values quantised through fp16
    like the reference's `.cpu().half()` at :151-154)."""
    smooth = selected_smooth if selected_smooth in (3, 5) else 0       # only 3 and 5 act in the reference (:136-144)
    # the packaged nnUNet path keeps the MIND cost scale 12 even when C != 12 (:127)
    disp = register_labels_device(pred_fixed.to(device), pred_moving.to(device), lambda_weight=lambda_weight, grid_sp=grid_sp,
                                  disp_hw=disp_hw, selected_niter=selected_niter, selected_smooth=smooth,
                                  grid_sp_adam=grid_sp_adam, ic=ic, cost_scale=12.0)
    return disp.permute(1, 2, 3, 0).half().cpu().numpy().astype(float)


def convex_adam(path_pred_fixed, path_pred_moving, lambda_weight, grid_sp, disp_hw, selected_niter, selected_smooth,
                grid_sp_adam=2, ic=True, result_path='./'):
    """File wrapper (convex_adam_nnUNet.py:41-159): NIfTI label maps in, `disp.nii.gz` out."""
    from .nifti_io import load_affine, load_fdata, save_image      # nibabel when installed, else the built-in NIfTI-1 reader / writer
    pred_fixed = torch.from_numpy(load_fdata(path_pred_fixed)).float()
    pred_moving = torch.from_numpy(load_fdata(path_pred_moving)).float()
    torch.cuda.synchronize()
    t0 = time.time()
    displacements = convex_adam_pt(pred_fixed, pred_moving, lambda_weight, grid_sp, disp_hw, selected_niter, selected_smooth,
                                   grid_sp_adam, ic)
    torch.cuda.synchronize()
    print('case time: ', time.time() - t0)
    save_image(displacements, load_affine(path_pred_fixed), os.path.join(result_path, 'disp.nii.gz'))
