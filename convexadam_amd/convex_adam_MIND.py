"""Pipeline-level mirror of the reference's `convexAdam.convex_adam_MIND`
(src/convexAdam/convex_adam_MIND.py): extract_features (:22-61), convex_adam_pt (:64-202),
convex_adam (:205-248).  Same keyword arguments, same output: np.ndarray (H,W,D,3) float64,
channel a = displacement along array axis a in voxels, fixed(x) ~ moving(x + u(x)).

The whole pair runs inside one C-ABI call (cvx_register_pair_f32): MIND-SSC -> pooling ->
correlation -> coupled convex (-> reverse direction -> inverse consistency) -> Adam instance
optimisation -> up-sampling, all on the current HIP stream, with no host round trips (the
reference's `.cpu()` hop at :156 and `.item()` syncs at convex_adam_utils.py:61 do not exist here).
"""
import ctypes as C
import os
import time
import warnings
from pathlib import Path
from typing import Optional, Union

import numpy as np
import torch

from ._lib import PairParams, call, f32c, lib, ptr, scratch
from .convex_adam_utils import MINDSSC, validate_image

_DEFAULT_DEVICE = torch.device("cuda" if torch.cuda.is_available() else "cpu")

# Mode of the Adam loop when a caller does not name one: "exact" -- every operator in the reference's evaluation order, bit-identical to
# oracle/cvx_oracle.c -- unless CONVEXADAM_ADAM_MODE=fast or set_default_adam_mode("fast").  (Round 4 shipped "fast" as the default on the
# strength of ONE full-size capture of the reference; round 5 captured three more and the mode does not meet the 80-iteration criteria
# on all of them -- tests/test_oracle_vs_golden.py::test_fast_adam_mode_against_four_reference_captures, DESIGN.md section 11 -- so the
# throughput arithmetic is opt-in: adam_mode="fast".)  A defaulted call falls back to "exact" where the fast loop does not exist
# (two-pool spline); an explicit adam_mode="fast" there raises.
_default_adam_mode = os.environ.get("CONVEXADAM_ADAM_MODE", "exact")
if _default_adam_mode not in ("exact", "fast", "fast_all"):
    raise ValueError("CONVEXADAM_ADAM_MODE must be 'exact', 'fast' or 'fast_all', not %r" % (_default_adam_mode,))


def set_default_adam_mode(mode):
    """'fast' or 'exact'; returns the previous default."""
    global _default_adam_mode
    if mode not in ("exact", "fast", "fast_all"):
        raise ValueError("adam mode must be 'exact', 'fast' or 'fast_all'")
    prev, _default_adam_mode = _default_adam_mode, mode
    return prev


def default_adam_mode():
    return _default_adam_mode


def _resolve_adam_mode(adam_mode, n_spline_pools=3, storage="fp32"):
    if adam_mode is None:
        return _default_adam_mode if n_spline_pools != 2 else "exact"
    return adam_mode


def _require_hip(device):
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("convexadam_amd runs only on a HIP device (torch device 'cuda'); got %s. "
                           "There is no CPU fallback -- use the upstream reference for CPU runs." % device)
    return device


def _load_mask(path):
    from .nifti_io import load_fdata   # nib.load(path).get_fdata() (:94-95); built-in NIfTI-1 reader when nibabel is absent
    return torch.from_numpy(load_fdata(path)).float()


def feature_transform(obj):
    """Device counterpart of scipy.ndimage.distance_transform_edt(obj, return_indices=True)[1] for a (H,W,D) device tensor:
    (3,H,W,D) int32 coordinates of the nearest ZERO voxel, scipy's tie-breaking included (csrc/edt.hip)."""
    o = f32c(obj)
    H, W, D = [int(s) for s in o.shape[-3:]]
    feat = torch.empty((3, H, W, D), dtype=torch.int32, device=o.device)
    call(o.device, "cvx_feature_transform_i32", ptr(o), H, W, D, ptr(feat), *scratch(o.device, "cvx_feature_transform_workspace_bytes", H, W, D))
    return feat


def _replicate_fill(img, mask, device):
    """Masked 'replicate fill' of convex_adam_MIND.py:40-51: outside the eroded mask the image takes the value of the
    nearest in-mask voxel (found at half resolution with the Euclidean feature transform, tie-breaking as scipy's, which
    the reference calls on the host), tri-linearly up-sampled; inside it keeps its own values.  Everything runs in HIP
    kernels: erosion, feature transform, index expression of :45, gather, up-sampling, merge."""
    from .convex_adam_utils import resize_trilinear
    H, W, D = [int(s) for s in img.shape[-3:]]
    if H % 2 or W % 2 or D % 2:
        raise ValueError("masked feature extraction needs even extents (the reference's index expression at "
                         "convex_adam_MIND.py:45 and its x2 up-sampling only line up for even H, W, D)")
    im = f32c(img.to(device)).reshape(H, W, D)
    mk = f32c(mask.to(device)).reshape(H, W, D)
    m = torch.empty_like(mk)
    call(device, "cvx_mask_erode_f32", ptr(mk), H, W, D, 0.9, ptr(m))
    if float(m[::2, ::2, ::2].max()) == 0.0:
        raise ValueError("masked feature extraction: the eroded mask is empty at half resolution (no voxel to replicate from)")
    # edt((m[::2,::2,::2] == 0), return_indices=True): the "objects" are the voxels OUTSIDE the eroded mask
    outside = (m[::2, ::2, ::2] == 0).to(torch.float32).contiguous()
    feat = feature_transform(outside)
    h2, w2, d2 = [int(s) for s in outside.shape]
    lin_d = torch.empty((h2, w2, d2), dtype=torch.int64, device=device)
    call(device, "cvx_feature_flat_index_i64", ptr(feat), h2, w2, d2, W, D, ptr(lin_d))   # same expression as :45
    half_src = im[::2, ::2, ::2].contiguous()
    half = torch.empty((1, 1) + tuple(half_src.shape), dtype=torch.float32, device=device)
    filled = torch.empty((1, 1, H, W, D), dtype=torch.float32, device=device)
    call(device, "cvx_gather_f32", ptr(half_src), ptr(lin_d), lin_d.numel(), ptr(half))
    up = resize_trilinear(half, (H, W, D))                              # F.interpolate(scale_factor=2, trilinear)
    call(device, "cvx_select_f32", ptr(m), ptr(im), ptr(up), im.numel(), ptr(filled))
    return filled


def extract_features(img_fixed: torch.Tensor, img_moving: torch.Tensor, mind_r: int, mind_d: int, use_mask: bool,
                     mask_fixed: torch.Tensor, mask_moving: torch.Tensor, device: torch.device = torch.device("cuda"),
                     dtype: torch.dtype = torch.float16):
    """MIND-SSC features of both images, (1,12,H,W,D) each in `dtype`.  (convex_adam_MIND.py:22-61)"""
    device = _require_hip(device)
    if use_mask:
        fixed_r = _replicate_fill(img_fixed, mask_fixed, device)
        moving_r = _replicate_fill(img_moving, mask_moving, device)
    else:
        fixed_r = img_fixed.unsqueeze(0).unsqueeze(0).to(device)
        moving_r = img_moving.unsqueeze(0).unsqueeze(0).to(device)
    features_fix = MINDSSC(fixed_r, mind_r, mind_d, device=device).to(dtype)
    features_mov = MINDSSC(moving_r, mind_r, mind_d, device=device).to(dtype)
    return features_fix, features_mov


# ---- what the three device entry points share ----------------------------------------------------------------------------------------
def _unpack_pair(img_fixed, img_moving, feat_fixed, feat_moving, shape_error=None):
    """Two (H,W,D) images or two (C,H,W,D) feature volumes -> (a, b, ff, fm, n_feat, H, W, D, dev); the pair not given is None.  `shape_error`:
    text of the ValueError for images that are not two 3-D volumes of equal shape (None: not checked here)."""
    if feat_fixed is not None:
        ff, fm = f32c(feat_fixed), f32c(feat_moving)
        n_feat = int(ff.shape[0])
        H, W, D = [int(s) for s in ff.shape[1:]]
        return None, None, ff, fm, n_feat, H, W, D, ff.device
    a, b = f32c(img_fixed), f32c(img_moving)
    if shape_error is not None and (a.dim() != 3 or a.shape != b.shape):
        raise ValueError(shape_error)
    H, W, D = [int(s) for s in a.shape]
    return a, b, None, None, 0, H, W, D, a.device


def _pair_params(adam_mode, cost="ssd", corr_mode="exact", storage="fp32", **fields):
    """struct cvx_pair_params, every field by name; a field left out stays 0, which the library reads as its default."""
    fields = {k: float(v) if k in ("lambda_weight", "cost_scale") else int(v) for k, v in fields.items()}
    return PairParams(cost=1 if cost == "sad" else 0, corr_fast=1 if corr_mode == "fast" else 0, fp16_storage=1 if storage == "fp16" else 0,
                      adam_fast={"exact": 0, "fast": 1, "fast_all": 2}[adam_mode], **fields)


def _field_shape(H, W, D, grid_sp, ic, lambda_weight):
    """Full resolution, or the coarse grid for the reference's ic=False & lambda_weight<=0 case."""
    return (3, H, W, D) if ic or lambda_weight > 0 else (3, H // grid_sp, W // grid_sp, D // grid_sp)


def _register_device(entry, head, again, n_feat, H, W, D, dev, mind_r, mind_d, lambda_weight, grid_sp, disp_hw, selected_niter, selected_smooth,
                     grid_sp_adam, ic, cost_scale, out, profile, cost, n_box, n_spline_pools, corr_mode, storage, adam_mode):
    """What the single-pair device entries share (register_pair_device here, convex_adam_nnUNet.register_labels_device): the reference's
    behaviour for option values it does not handle, struct cvx_pair_params, workspace and output, the call.  `entry`: the entry point is
    entry_f32, its workspace query entry_workspace_bytes; `head`: the arguments in front of the parameter struct;
    `again(selected_smooth, out)`: the same public call with these two arguments replaced.  (The caller has checked that `dev` is a HIP device.)"""
    if lambda_weight > 0 and selected_niter < 1:
        # the reference reads `disp_sample` after a loop that never ran (:181)
        raise UnboundLocalError("local variable 'disp_sample' referenced before assignment "
                                "(selected_niter=0 with lambda_weight>0, convex_adam_MIND.py:181)")
    if selected_smooth > 0 and selected_smooth % 2 == 0:
        # The reference announces "+1" for an even kernel and then overwrites its own fix (:185-189): three avg_pool3d(k, stride 1,
        # padding k//2) that each make every axis one voxel longer -- it returns (H+3, W+3, D+3, 3).  Restated as it behaves: the pair
        # without smoothing, then the three growing pools (cvx_box_grow_f32).  With lambda_weight <= 0 the block is never reached (:155).
        from .convex_adam_utils import box_smooth
        if out is not None and lambda_weight > 0:
            raise ValueError("register_pair_device: an even selected_smooth returns a (3,H+3,W+3,D+3) field; `out` is not supported")
        disp = again(0, out)
        return box_smooth(disp[None], int(selected_smooth), 3)[0] if lambda_weight > 0 else disp
    adam_mode = _resolve_adam_mode(adam_mode, n_spline_pools, storage)
    if cost not in ("ssd", "sad") or corr_mode not in ("exact", "fast") or storage not in ("fp32", "fp16") or adam_mode not in ("exact", "fast", "fast_all"):
        raise ValueError("cost must be 'ssd' or 'sad', corr_mode 'exact' or 'fast', adam_mode 'exact', 'fast' or 'fast_all', storage 'fp32' or 'fp16'")
    p = _pair_params(adam_mode, cost, corr_mode, storage, H=H, W=W, D=D, mind_r=mind_r, mind_d=mind_d, lambda_weight=lambda_weight, grid_sp=grid_sp,
                     disp_hw=disp_hw, selected_niter=selected_niter, selected_smooth=selected_smooth, grid_sp_adam=grid_sp_adam, ic=bool(ic),
                     n_feat=n_feat, cost_scale=cost_scale, n_box=n_box, n_spline_pools=n_spline_pools)
    ws = scratch(dev, entry + "_workspace_bytes", C.byref(p), required=True)
    oshape = _field_shape(H, W, D, grid_sp, ic, lambda_weight)
    if out is None:
        out = torch.empty(oshape, dtype=torch.float32, device=dev)
    dims = (C.c_int * 3)()
    if profile is not None:
        lib().cvx_set_profiling(int(profile))
    call(dev, entry + "_f32", *head, C.byref(p), ptr(out), C.cast(dims, C.c_void_p), *ws)
    assert tuple(dims) == tuple(oshape[1:]), (tuple(dims), oshape)
    return out


def register_pair_device(img_fixed=None, img_moving=None, feat_fixed=None, feat_moving=None, mind_r=1, mind_d=2,
                         lambda_weight=1.25, grid_sp=6, disp_hw=4, selected_niter=80, selected_smooth=0, grid_sp_adam=2,
                         ic=True, cost_scale=12.0, out=None, profile=None, cost="ssd", n_box=2, n_spline_pools=3, corr_mode="exact",
                         storage="fp32", adam_mode=None):
    """One registration, device in / device out: returns the displacement field as a (3,H',W',D') float32
    device tensor (full resolution, or the coarse grid for the reference's ic=False & lambda_weight<=0 case).
    Either two (H,W,D) images (MIND-SSC features are computed) or two (C,H,W,D) feature volumes.
    Variants of the challenge scripts: cost="sad" (l2r_2021 task 3 :54), n_box=1 (task 2 :60), n_spline_pools=2
    (task 3 :191); corr_mode="fast" = FMA / separable correlation sums; storage="fp16" = pooled features and cost volume rounded to
    half precision with float32 accumulation (the reference's GPU default dtype, convex_adam_MIND.py:79); adam_mode="fast" = the
    Adam loop in throughput arithmetic (cvx_adam_run_fast_f32; same mathematics, graded by end-point error, not by bits)."""
    a, b, ff, fm, n_feat, H, W, D, dev = _unpack_pair(img_fixed, img_moving, feat_fixed, feat_moving,
                                                      "register_pair_device expects two (H,W,D) volumes of equal shape")
    _require_hip(dev)
    return _register_device(
        "cvx_register_pair", (ptr(a), ptr(b), ptr(ff), ptr(fm)),
        lambda smooth, out_: register_pair_device(img_fixed, img_moving, feat_fixed, feat_moving, mind_r, mind_d, lambda_weight, grid_sp, disp_hw,
                                                  selected_niter, smooth, grid_sp_adam, ic, cost_scale, out_, profile, cost, n_box, n_spline_pools,
                                                  corr_mode, storage, adam_mode),
        n_feat, H, W, D, dev, mind_r, mind_d, lambda_weight, grid_sp, disp_hw, selected_niter, selected_smooth, grid_sp_adam, ic, cost_scale, out,
        profile, cost, n_box, n_spline_pools, corr_mode, storage, adam_mode)


def register_pair_snapshots_device(img_fixed=None, img_moving=None, feat_fixed=None, feat_moving=None, snapshot_iters=(40, 60, 80),
                                   smooths=(0, 3, 5), mind_r=1, mind_d=2, lambda_weight=1.25, grid_sp=6, disp_hw=4, grid_sp_adam=2, ic=True,
                                   cost_scale=12.0, n_spline_pools=3, adam_mode=None):
    """One Adam run, several results: the up-sampled `disp_sample` after each iteration of `snapshot_iters`
    (1-based), once per entry of `smooths` (0 = as is, k = three k^3 mean filters) -> (n_snap, n_smooth, 3, H, W, D) device tensor.
    The default is the 9-field variant of self_configuring/convex_adam_MIND.py:115-139; the sweep's stage 2 evaluates iterations
    60 / 80 / 100 / 120 of one 120-iteration run the same way (adam_run_withconfig_shiftSpline.py:234-246)."""
    a, b, ff, fm, n_feat, H, W, D, dev = _unpack_pair(img_fixed, img_moving, feat_fixed, feat_moving)
    _require_hip(dev)
    its = [int(v) for v in snapshot_iters]
    sms = [int(v) for v in smooths]
    p = _pair_params(_resolve_adam_mode(adam_mode, n_spline_pools), H=H, W=W, D=D, mind_r=mind_r, mind_d=mind_d, lambda_weight=lambda_weight,
                     grid_sp=grid_sp, disp_hw=disp_hw, selected_niter=its[-1], grid_sp_adam=grid_sp_adam, ic=bool(ic), n_feat=n_feat,
                     cost_scale=cost_scale, n_spline_pools=n_spline_pools)
    it_arr = (C.c_int * len(its))(*its)
    sm_arr = (C.c_int * len(sms))(*sms)
    ws = scratch(dev, "cvx_register_pair_snapshots_workspace_bytes", C.byref(p), len(its), C.cast(sm_arr, C.c_void_p), len(sms),
                 required=True, otherwise="bad snapshot arguments")
    out = torch.empty((len(its), len(sms), 3, H, W, D), dtype=torch.float32, device=dev)
    call(dev, "cvx_register_pair_snapshots_f32", ptr(a), ptr(b), ptr(ff), ptr(fm), C.byref(p), C.cast(it_arr, C.c_void_p), len(its),
         C.cast(sm_arr, C.c_void_p), len(sms), ptr(out), *ws)
    return out


def register_pairs_device(imgs_fixed, imgs_moving, outs=None, n_streams=2, mind_r=1, mind_d=2, lambda_weight=1.25, grid_sp=6,
                          disp_hw=4, selected_niter=80, selected_smooth=0, grid_sp_adam=2, ic=True, cost_scale=12.0, adam_mode=None):
    """Several independent pairs (lists of (H,W,D) device tensors, equal shapes) in one call: the library deals them
    onto `n_streams` internal HIP streams so that independent pairs fill each other's idle issue slots
    (cvx_register_pairs_f32).  Returns the list of (3,H,W,D) fields."""
    n = len(imgs_fixed)
    fx = [f32c(t) for t in imgs_fixed]
    mv = [f32c(t) for t in imgs_moving]
    H, W, D = [int(s) for s in fx[0].shape]
    dev = fx[0].device
    _require_hip(dev)
    if lambda_weight > 0 and selected_niter < 1:
        raise UnboundLocalError("local variable 'disp_sample' referenced before assignment (convex_adam_MIND.py:181)")
    p = _pair_params(_resolve_adam_mode(adam_mode), H=H, W=W, D=D, mind_r=mind_r, mind_d=mind_d, lambda_weight=lambda_weight, grid_sp=grid_sp,
                     disp_hw=disp_hw, selected_niter=selected_niter, selected_smooth=selected_smooth, grid_sp_adam=grid_sp_adam, ic=bool(ic),
                     cost_scale=cost_scale)
    n_streams = max(1, min(int(n_streams), n, 8))
    ws = scratch(dev, "cvx_register_pair_workspace_bytes", C.byref(p), required=True,
                 size=lambda per: (per + 4095) // 4096 * 4096 * n_streams)          # one 4 KiB-rounded slot per internal stream
    if outs is None:
        outs = [torch.empty(_field_shape(H, W, D, grid_sp, ic, lambda_weight), dtype=torch.float32, device=dev) for _ in range(n)]
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    dims = (C.c_int * 3)()
    call(dev, "cvx_register_pairs_f32", n, C.cast(arr(fx), C.c_void_p), C.cast(arr(mv), C.c_void_p), None, None, C.byref(p),
         C.cast(arr(outs), C.c_void_p), C.cast(dims, C.c_void_p), *ws, n_streams)
    return outs


# ---- host <-> device hand-over of the drop-in API ---------------------------------------------------------------
# convex_adam_pt takes host images and returns a host array.  The field is packed on the DEVICE into the reference's output format
# ((H,W,D,3) float64 after the `dtype` round trip, convex_adam_MIND.py:198-202) and written by the packing kernel straight into pinned
# host memory (cvx_pack_field_f64): no permuted device copy, no pageable download, no single-threaded astype(float) of 165 MB.
# Pinned buffers are pooled (hipHostMalloc of 165 MB costs tens of milliseconds): a buffer returns to the pool when the array handed to
# the caller -- and every view of it -- has been garbage-collected.
import threading
import weakref

_QUANT = {torch.float32: 0, torch.float16: 1}


_BUSY = object()                              # pool entry taken, the ndarray that will own it does not exist yet


class _PinnedPool:
    """Thread-safe: an entry is marked _BUSY inside the lock by take() and stays so until give() installs the weak reference to the
    array handed to the caller (pack_field_to_host releases the GIL in synchronize() between the two -- ADVICE round 4)."""

    def __init__(self):
        self._entries = []                    # [tensor, _BUSY | weakref to the ndarray handed out | None (free)]
        self._lock = threading.Lock()

    @staticmethod
    def _free(ref):
        return ref is None or (ref is not _BUSY and ref() is None)

    def take(self, shape, dtype):
        n = 1
        for v in shape:
            n *= int(v)
        with self._lock:
            for e in self._entries:
                t, ref = e
                if t is not None and t.dtype == dtype and t.numel() >= n and self._free(ref):
                    e[1] = _BUSY
                    return e, t.view(-1)[:n].view(shape)
            e = [None, _BUSY]
            self._entries.append(e)
            if len(self._entries) > 8:        # drop the oldest free buffer
                for i, (_, ref) in enumerate(self._entries):
                    if self._entries[i] is not e and self._free(ref):
                        del self._entries[i]
                        break
        try:
            e[0] = torch.empty(n, dtype=dtype, pin_memory=True)      # (outside the lock: hipHostMalloc of 165 MB takes tens of ms)
        except BaseException:
            self.give(e, None)
            with self._lock:
                if e in self._entries:
                    self._entries.remove(e)
            raise
        return e, e[0].view(shape)

    def give(self, e, arr):
        """arr = the ndarray handed to the caller (the entry is free again once it is garbage-collected), or None = free now."""
        with self._lock:
            e[1] = weakref.ref(arr) if arr is not None else None

    def clear(self):
        with self._lock:
            self._entries = [e for e in self._entries if e[1] is _BUSY]


_out_pool = _PinnedPool()


_tls = threading.local()


def _stage_pins():
    """The calling thread's four pinned input-staging slots of convex_adam_pt_many (re-used across calls; a slot is re-allocated when the
    image shape changes)."""
    if not hasattr(_tls, "pins"):
        _tls.pins = [None] * 4
        _tls.pin_free = [None] * 4                       # the event behind the last upload FROM a slot: lives with the slot, not with a generator
    return _tls.pins


def upload_image(img, device):
    """Host image -> float32 device tensor (torch's own upload: 27.5 MB in 0.56 ms on the round-4 boxes, as fast as a copy from pinned
    memory).  NB: this path deliberately runs NO multi-threaded host work -- a 128-thread torch CPU copy into a pinned staging buffer
    exhausted the container's CPU quota (16 cores of 256 visible) and the cgroup throttling stalled every third call for 70-100 ms."""
    t = img if isinstance(img, torch.Tensor) else validate_image(img)
    return t.float().to(device).contiguous()


def pack_field_to_host(disp, dtype=torch.float32, sync=True, staging=None):
    """(3,H,W,D) float32 device field -> np.ndarray (H,W,D,3) float64 in pinned host memory, every value passed through `dtype`
    (float16 / float32) first: the device-side equivalent of convex_adam_MIND.py:198-202.
    staging = None: the packing kernel writes the host array itself (3.0 ms for 165 MB, the fastest single call).  staging = a (H,W,D,3)
    float64 DEVICE tensor: the kernel packs into it (0.05 ms) and a copy engine moves it to the host -- measured beside a registration on
    another stream: 5.95 ms for both, against 9.05 ms when the kernel writes across PCIe (its stalled wavefronts hold the compute
    units); this is what convex_adam_pt_many uses."""
    if dtype not in _QUANT:
        field = disp.permute(1, 2, 3, 0).to(dtype)
        return field.cpu().numpy().astype(float)
    f = f32c(disp)
    _, H, W, D = [int(v) for v in f.shape]
    e, buf = _out_pool.take((H, W, D, 3), torch.float64)
    try:
        call(f.device, "cvx_pack_field_f64", ptr(f), H, W, D, _QUANT[dtype], ptr(buf if staging is None else staging))
        if staging is not None:
            buf.copy_(staging, non_blocking=True)
        if sync:
            torch.cuda.current_stream(f.device).synchronize()
        arr = buf.numpy()
    except BaseException:
        _out_pool.give(e, None)
        raise
    _out_pool.give(e, arr)
    return arr


def set_profiling(mode: int):
    """0 = off, 1 = keep the stage timings of the last call, 2 = accumulate over calls (hipEvents on the launch stream)."""
    lib().cvx_set_profiling(int(mode))


def last_profile(max_intervals=4096):
    """[(stage, milliseconds)] recorded since profiling was switched on (waits for the last event)."""
    names = (C.c_char_p * max_intervals)()
    ms = (C.c_float * max_intervals)()
    n = lib().cvx_last_pair_profile(C.cast(names, C.c_void_p), C.cast(ms, C.c_void_p), max_intervals)
    return [(names[i].decode(), float(ms[i])) for i in range(n)]


def convex_adam_pt(
    img_fixed,
    img_moving,
    mind_r: int = 1,
    mind_d: int = 2,
    lambda_weight: float = 1.25,
    grid_sp: int = 6,
    disp_hw: int = 4,
    selected_niter: int = 80,
    selected_smooth: int = 0,
    grid_sp_adam: int = 2,
    ic: bool = True,
    use_mask: bool = False,
    path_fixed_mask: Optional[Union[Path, str]] = None,
    path_moving_mask: Optional[Union[Path, str]] = None,
    dtype: torch.dtype = torch.float16,
    verbose: bool = False,
    device: torch.device = _DEFAULT_DEVICE,
    adam_mode: Optional[str] = None,
) -> np.ndarray:
    """Coupled convex optimisation with Adam instance optimisation.  (convex_adam_MIND.py:64-202)
    adam_mode (not in the reference): "exact" = the Adam loop in the reference's evaluation order (bit-identical to the CPU oracle),
    "fast" = the same loop in throughput arithmetic (cvx_adam_run_fast_f32; ~1.3x faster per pair, graded by end-point error);
    None = the package default (set_default_adam_mode / CONVEXADAM_ADAM_MODE, "exact" out of the box).

    Computes in float32 on the HIP device whatever `dtype` says; `dtype` only quantises the returned
    field the way the reference's `.cpu().to(dtype)` does (:198-200) -- pass torch.float32 for
    full-precision output.  Returns np.ndarray (H,W,D,3) float64."""
    device = _require_hip(device)
    img_fixed = validate_image(img_fixed).float()
    img_moving = validate_image(img_moving).float()
    if selected_smooth > 0 and selected_smooth % 2 == 0:
        print('selected_smooth should be an odd number, adding 1')       # the reference's message (:187); its fix is overwritten at :189,
                                                                         # so the field grows to (H+3, W+3, D+3, 3) -- restated in register_pair_device
    H, W, D = img_fixed.shape
    t0 = time.time()
    if use_mask:
        mask_fixed = _load_mask(path_fixed_mask)
        mask_moving = _load_mask(path_moving_mask)
        ff, fm = extract_features(img_fixed, img_moving, mind_r, mind_d, True, mask_fixed, mask_moving, device, torch.float32)
        disp = register_pair_device(feat_fixed=ff[0], feat_moving=fm[0], lambda_weight=lambda_weight, grid_sp=grid_sp,
                                    disp_hw=disp_hw, selected_niter=selected_niter, selected_smooth=selected_smooth,
                                    grid_sp_adam=grid_sp_adam, ic=ic, adam_mode=adam_mode)
    else:
        disp = register_pair_device(upload_image(img_fixed, device), upload_image(img_moving, device), mind_r=mind_r, mind_d=mind_d,
                                    lambda_weight=lambda_weight, grid_sp=grid_sp, disp_hw=disp_hw,
                                    selected_niter=selected_niter, selected_smooth=selected_smooth,
                                    grid_sp_adam=grid_sp_adam, ic=ic, adam_mode=adam_mode)
    # (H,W,D,3) float64 after the dtype round trip (:198-201), packed on the device into pinned host memory
    displacements = pack_field_to_host(disp, dtype)
    if verbose:
        print(f'case time: {time.time() - t0}')
    return displacements


def convex_adam_pt_many(pairs, dtype: torch.dtype = torch.float16, device: torch.device = _DEFAULT_DEVICE, **kw):
    """Generator over an iterable of (img_fixed, img_moving) host images: yields convex_adam_pt's result for each pair -- what a sweep
    over pairs (self_configuring/convex_run_withconfig.py:85) needs from the drop-in API -- with the transfers hidden behind the
    registrations (measured: 6.95 instead of 10.2 ms per pair at the benchmark size, engine 5.8):
      * the images of pair i + 1 are copied into pinned staging buffers (single-threaded memcpy: a 128-thread torch copy runs into the
        container's CPU quota) and uploaded asynchronously on their own stream WHILE pair i registers -- a pageable `.to(device)` beside
        a running download blocked for 9 ms;
      * the field of pair i is packed into a DEVICE buffer (0.05 ms) and moved to pooled pinned memory by a copy engine on a side stream
        -- the packing kernel writing across PCIe itself would hold the compute units with stalled wavefronts (9.05 instead of 5.95 ms
        for a registration + a download side by side).
    Keyword arguments as convex_adam_pt (no masks)."""
    device = _require_hip(device)
    main = torch.cuda.current_stream(device)
    side = torch.cuda.Stream(device)
    up = torch.cuda.Stream(device)
    bufs = [None, None, None]                            # rotating device fields: pair i's is read by the side stream while pair i + 1 registers
    stage = [None, None]                                 # packed fields on the device
    # pinned staging for two pairs in flight + the events that free them; the buffers outlive the call (per thread: hipHostMalloc of
    # 4 x 27.5 MB cost ~10 ms per generator, 1.2 ms per pair of an 8-pair sweep)
    # (the events that free the slots are thread-local like the slots: two generators interleaved on one thread, or a new one started
    # after an abandoned one, wait for each other's uploads before they overwrite a slot -- ADVICE round 5)
    pins = _stage_pins()
    pin_free = _tls.pin_free

    def upload(k, img_fixed, img_moving):
        out = []
        for j, img in enumerate((img_fixed, img_moving)):
            t = validate_image(img).float().contiguous()
            slot = 2 * (k % 2) + j
            if pin_free[slot] is not None:
                pin_free[slot].synchronize()
            if pins[slot] is None or pins[slot].shape != t.shape:
                pins[slot] = torch.empty(t.shape, dtype=torch.float32, pin_memory=True)
            np.copyto(pins[slot].numpy(), t.numpy())
            with torch.cuda.stream(up):
                d = pins[slot].to(device, non_blocking=True)
                pin_free[slot] = torch.cuda.Event()
                pin_free[slot].record(up)
            d.record_stream(main)
            out.append(d)
        ev = torch.cuda.Event()
        ev.record(up)
        return out[0], out[1], ev

    it = iter(pairs)
    try:
        nxt = upload(0, *next(it))
    except StopIteration:
        return
    pending = None
    i = 0
    while nxt is not None:
        fd, md, ev = nxt
        main.wait_event(ev)
        b = bufs[i % 3]
        if b is not None and tuple(b.shape[1:]) != tuple(fd.shape):
            b = None
        disp = register_pair_device(fd, md, out=b, **kw)
        bufs[i % 3] = disp if tuple(disp.shape[1:]) == tuple(fd.shape) else None
        if bufs[i % 3] is None:
            disp.record_stream(side)                     # (even selected_smooth: a fresh (H+3, ..) field the side stream still reads)
        ready = torch.cuda.Event()
        ready.record(main)
        try:                                             # the NEXT pair's upload is enqueued before this pair's download exists
            nxt = upload(i + 1, *next(it))
        except StopIteration:
            nxt = None
        with torch.cuda.stream(side):
            side.wait_event(ready)
            st = stage[i % 2]
            if dtype in _QUANT and (st is None or tuple(st.shape[:3]) != tuple(disp.shape[1:])):
                st = stage[i % 2] = torch.empty(tuple(disp.shape[1:]) + (3,), dtype=torch.float64, device=device)
            arr = pack_field_to_host(disp, dtype, sync=False, staging=st if dtype in _QUANT else None)
            done = torch.cuda.Event()
            done.record(side)
        if pending is not None:
            pending[1].synchronize()
            yield pending[0]
        pending = (arr, done)
        i += 1
    if pending is not None:
        pending[1].synchronize()
        yield pending[0]
    main.wait_stream(side)


def convex_adam(
    path_img_fixed: Union[Path, str],
    path_img_moving: Union[Path, str],
    mind_r: int = 1,
    mind_d: int = 2,
    lambda_weight: float = 1.25,
    grid_sp: int = 6,
    disp_hw: int = 4,
    selected_niter: int = 80,
    selected_smooth: int = 0,
    grid_sp_adam: int = 2,
    ic: bool = True,
    use_mask: bool = False,
    path_fixed_mask: Optional[Union[Path, str]] = None,
    path_moving_mask: Optional[Union[Path, str]] = None,
    result_path: Union[Path, str] = './',
    verbose: bool = False,
) -> None:
    """File wrapper: reads two NIfTI images, writes `disp.nii.gz` with the fixed image's affine.
    (convex_adam_MIND.py:205-248; through nibabel when it is installed, else the built-in NIfTI-1 reader / writer of nifti_io.py)"""
    from .nifti_io import load_affine, load_fdata, save_image
    img_fixed = torch.from_numpy(load_fdata(path_img_fixed)).float()
    img_moving = torch.from_numpy(load_fdata(path_img_moving)).float()
    displacements = convex_adam_pt(img_fixed=img_fixed, img_moving=img_moving, mind_r=mind_r, mind_d=mind_d,
                                   lambda_weight=lambda_weight, grid_sp=grid_sp, disp_hw=disp_hw,
                                   selected_niter=selected_niter, selected_smooth=selected_smooth,
                                   grid_sp_adam=grid_sp_adam, ic=ic, use_mask=use_mask, path_fixed_mask=path_fixed_mask,
                                   path_moving_mask=path_moving_mask, verbose=verbose)
    save_image(displacements, load_affine(path_img_fixed), os.path.join(result_path, 'disp.nii.gz'))


if __name__ == "__main__":
    import argparse
    parser = argparse.ArgumentParser()
    parser.add_argument("-f", "--path_img_fixed", type=str, required=True)
    parser.add_argument("-m", '--path_img_moving', type=str, required=True)
    parser.add_argument('--mind_r', type=int, default=1)
    parser.add_argument('--mind_d', type=int, default=2)
    parser.add_argument('--lambda_weight', type=float, default=1.25)
    parser.add_argument('--grid_sp', type=int, default=6)
    parser.add_argument('--disp_hw', type=int, default=4)
    parser.add_argument('--selected_niter', type=int, default=80)
    parser.add_argument('--selected_smooth', type=int, default=0)
    parser.add_argument('--grid_sp_adam', type=int, default=2)
    parser.add_argument('--ic', choices=('True', 'False'), default='True')
    parser.add_argument('--use_mask', choices=('True', 'False'), default='False')
    parser.add_argument('--path_mask_fixed', type=str, default=None)
    parser.add_argument('--path_mask_moving', type=str, default=None)
    parser.add_argument('--result_path', type=str, default='./')
    a = parser.parse_args()
    convex_adam(a.path_img_fixed, a.path_img_moving, a.mind_r, a.mind_d, a.lambda_weight, a.grid_sp, a.disp_hw,
                a.selected_niter, a.selected_smooth, a.grid_sp_adam, a.ic == 'True', a.use_mask == 'True',
                a.path_mask_fixed, a.path_mask_moving, a.result_path)
