"""GPU tests of the label entries: pooled weighted one-hot features straight from the label maps (cvx_label_features_pooled_f32) and the
pair pipeline on top of them (cvx_register_label_pair_f32, register_labels_device).  The one-hot volumes are never written; every result
is BIT-IDENTICAL (np.array_equal) to the path that writes them -- cvx_label_features_f32 + cvx_avgpool_f32 (+ cvx_register_pair_f32 on the
feature volumes) -- to the CPU oracle's restatement of the reference, and to the reference's own capture."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def N():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from convexadam_amd import convex_adam_nnUNet
    return convex_adam_nnUNet


@pytest.fixture(scope="module")
def M():
    from convexadam_amd import convex_adam_MIND
    return convex_adam_MIND


@pytest.fixture(scope="module")
def U():
    from convexadam_amd import convex_adam_utils
    return convex_adam_utils


# ---- 1. the operator ---------------------------------------------------------------------------------------------------------------
def uniform_cells(rng, labs, shape, g):
    """A map of whole uniform g^3 cells (remainder voxels continue the last cell's pattern): k = g^3 in every pooled cell."""
    coarse = rng.choice(labs, [-(-s // g) for s in shape])
    fine = coarse.repeat(g, 0).repeat(g, 1).repeat(g, 2)
    return fine[:shape[0], :shape[1], :shape[2]]


def label_sets(shape, g1, g2):
    """(name, fixed map, moving map): one channel; 9 labels; the three sets of test_label_features_many_and_large_labels (41 labels,
    labels up to 304 with gaps and labels of one map only, disjoint even / odd maps); whole uniform cells of either window."""
    rng = np.random.default_rng(shape[0] * 10000 + shape[1] * 100 + shape[2] + g1)
    yield "one_channel", np.full(shape, 3), np.full(shape, 3)
    yield "9_labels", rng.choice(np.arange(9), shape), rng.choice(np.arange(9), shape)
    yield "41_labels", rng.choice(np.arange(41), shape), rng.choice(np.arange(41), shape)
    labs = np.array([0, 1, 2, 5, 17, 64, 128, 255, 256, 257, 299, 300, 301] + list(range(100, 140, 3)))
    lf, lm = rng.choice(labs, shape), rng.choice(labs, shape)
    lf[0, 0, :3] = [303, 302, 280]                                     # only in the fixed map
    lm[-1, -1, -2:] = [290, 304]                                       # only in the moving map
    yield "max_label_300", lf, lm
    yield "one_map_only", rng.choice(np.arange(0, 70, 2), shape), rng.choice(np.arange(1, 71, 2), shape)
    if shape == (12, 18, 13):
        yield "70_labels", rng.choice(np.arange(70), shape), rng.choice(np.arange(70), shape)
    for g in sorted({g1, g2} - {0, 1}):
        yield "uniform_cells_%d" % g, uniform_cells(rng, np.arange(9), shape, g), uniform_cells(rng, np.arange(9), shape, g)


def pooled_with_guards(N, lab, present_d, weights_d, Cn, mult, g1, g2):
    """cvx_label_features_pooled_f32 into buffers with one guard float on either side of each output."""
    from convexadam_amd import _lib
    H, W, D = lab.shape
    bufs, outs = [], []
    for g in (g1, g2):
        if g == 0:
            bufs.append(None)
            continue
        n = Cn * (H // g) * (W // g) * (D // g)
        bufs.append(torch.full((n + 2,), 7.0, dtype=torch.float32, device=DEV))
    ptr = lambda b: C.c_void_p(b.data_ptr() + 4) if b is not None else None
    _lib.check(_lib.lib().cvx_label_features_pooled_f32(C.c_void_p(lab.data_ptr()), H, W, D, Cn, C.c_void_p(present_d.data_ptr()),
                                                        C.c_void_p(weights_d.data_ptr()), float(mult), g1, ptr(bufs[0]), g2, ptr(bufs[1]),
                                                        _lib.stream_ptr(DEV)))
    for g, b in zip((g1, g2), bufs):
        if b is None:
            outs.append(None)
            continue
        got = host(b)
        assert got[0] == 7.0 and got[-1] == 7.0, "guard float overwritten (window %d)" % g
        outs.append(got[1:-1].reshape(Cn, H // g, W // g, D // g))
    return outs


# the issue's six geometries; then two more, one per remaining path of the launcher: a row longer than one tile (windows 5 and 2 share
# tiles of 10 x 10 x 320 voxels: two tiles along D) and windows without a common tile in the LDS budget (7 and 5: the direct kernel)
GEOMETRIES = [((12, 14, 16), 4, 2), ((13, 11, 17), 3, 2), ((12, 18, 13), 6, 2), ((10, 10, 10), 5, 2), ((8, 8, 8), 4, 1), ((4, 4, 4), 2, 0),
              ((10, 10, 334), 5, 2), ((14, 15, 36), 7, 5)]


@pytest.mark.parametrize("shape,g1,g2", GEOMETRIES)
def test_pooled_label_features_vs_onehot_path_and_oracle(N, U, orc, shape, g1, g2):
    for name, lf, lm in label_sets(shape, g1, g2):
        lf, lm = lf.astype(np.float32), lm.astype(np.float32)
        lf_d, lm_d, present_d, weights_d, Cn = N._label_channels(dev(lf), dev(lm), DEV)
        for mult in (10.0, 0.37):
            ff, fm = N.extract_features(lf_d, lm_d, mult=mult, device=DEV)          # the path that writes the one-hot volumes
            rf, rm, pres = orc.label_features(lf, lm, mult)
            assert Cn == len(pres) == ff.shape[1], name
            for lab_d, feat, ref in ((lf_d, ff, rf), (lm_d, fm, rm)):
                got = pooled_with_guards(N, lab_d, present_d, weights_d, Cn, mult, g1, g2)
                for g, out in zip((g1, g2), got):
                    if g == 0:
                        assert out is None
                        continue
                    assert np.array_equal(out, host(U.avg_pool(feat, g))[0]), (name, mult, g)
                    assert np.array_equal(out, orc.avgpool_stride(ref, g)), (name, mult, g)
                    if name.startswith("uniform_cells_%d" % g):                     # every cell full: k = g^3 for one channel, 0 for the rest
                        assert ((out != 0).sum(0) == 1).all(), (name, g)
        # the Python operator: the same tensors, for both maps
        (f1, m1), second = N.label_features_pooled(lf_d, lm_d, g1, g2, mult=0.37, device=DEV)
        a, b = pooled_with_guards(N, lf_d, present_d, weights_d, Cn, 0.37, g1, g2), pooled_with_guards(N, lm_d, present_d, weights_d, Cn, 0.37, g1, g2)
        assert np.array_equal(host(f1), a[0]) and np.array_equal(host(m1), b[0]), name
        if g2 == 0:
            assert second is None
        else:
            assert np.array_equal(host(second[0]), a[1]) and np.array_equal(host(second[1]), b[1]), name


def test_unlisted_and_out_of_table_labels(N, U):
    """A voxel whose label equals no present[c] contributes to no channel; labels beyond the label -> channel table (>= 8192) and negative
    ones are matched like any other: against cvx_label_features_f32 + cvx_avgpool_f32 with the same channel list."""
    from convexadam_amd import _lib
    rng = np.random.default_rng(5)
    shape, g1, g2 = (8, 12, 10), 4, 2
    lab = rng.choice(np.array([0, 1, 4, 7, 9000, 70000, -3, 8191, 8192]), shape).astype(np.float32)
    lab[:4, :4, :4] = rng.choice(np.array([0, 4, 9000]), (4, 4, 4))    # a coarse cell of unlisted labels only
    present = np.array([1, 7, 8191, 8192, 70000, -3], np.int32)        # 0, 4 and 9000 are not listed
    weights = np.array([0.5, 1.25, 3.0, 0.75, 1.5, 2.0], np.float32)
    lab_d, present_d, weights_d = dev(lab), dev(present), dev(weights)
    feat = torch.empty((1, present.size) + shape, dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().cvx_label_features_f32(C.c_void_p(lab_d.data_ptr()), lab.size, present.size, C.c_void_p(present_d.data_ptr()),
                                                 C.c_void_p(weights_d.data_ptr()), 10.0, C.c_void_p(feat.data_ptr()), _lib.stream_ptr(DEV)))
    got = pooled_with_guards(N, lab_d, present_d, weights_d, present.size, 10.0, g1, g2)
    for g, out in zip((g1, g2), got):
        assert np.array_equal(out, host(U.avg_pool(feat, g))[0]), g
    assert (got[0][:, 0, 0, 0] == 0).all() and (got[1][:, :2, :2, :2] == 0).all()


# ---- 2. the pair entry against the feature entry -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def labels_pair(N, golden):
    g = golden("labels")
    lf, lm = dev(g["lab_fix"].astype(np.float32)), dev(g["lab_mov"].astype(np.float32))
    ff, fm = N.extract_features(lf, lm, device=DEV)
    return lf, lm, ff, fm


PAIR_VARIANTS = [dict(lambda_weight=0, ic=False), dict(lambda_weight=0, ic=True),
                 dict(lambda_weight=1.25, selected_niter=5, ic=True, selected_smooth=0), dict(lambda_weight=1.25, selected_niter=5, ic=True, selected_smooth=3),
                 dict(lambda_weight=1.25, selected_niter=5, ic=True, storage="fp16"), dict(lambda_weight=1.25, selected_niter=5, ic=True, cost="sad", n_box=1),
                 dict(lambda_weight=1.25, selected_niter=5, ic=True, n_spline_pools=2)]


@pytest.mark.parametrize("kw", PAIR_VARIANTS, ids=lambda kw: "-".join("%s=%s" % kv for kv in kw.items()))
def test_label_pair_equals_feature_pair(N, M, labels_pair, kw):
    lf, lm, ff, fm = labels_pair
    want = M.register_pair_device(feat_fixed=ff[0], feat_moving=fm[0], grid_sp=4, disp_hw=2, **kw)
    got = N.register_labels_device(lf, lm, grid_sp=4, disp_hw=2, **kw)
    coarse = not kw["ic"] and kw["lambda_weight"] <= 0
    assert tuple(got.shape) == tuple(want.shape) == ((3, 6, 5, 7) if coarse else (3, 24, 20, 28))
    assert np.array_equal(host(got), host(want))
    assert np.isfinite(host(got)).all() and np.abs(host(got)).max() > 0


def test_label_pair_with_windows_that_do_not_divide(N, M):
    """grid_sp 5 with grid_sp_adam 2 on a (20, 25, 30) pair of random 9-label maps."""
    rng = np.random.default_rng(11)
    lf, lm = dev(rng.integers(0, 9, (20, 25, 30)).astype(np.float32)), dev(rng.integers(0, 9, (20, 25, 30)).astype(np.float32))
    ff, fm = N.extract_features(lf, lm, device=DEV)
    kw = dict(lambda_weight=1.25, selected_niter=5, grid_sp=5, disp_hw=2, grid_sp_adam=2, ic=True)
    want = M.register_pair_device(feat_fixed=ff[0], feat_moving=fm[0], **kw)
    got = N.register_labels_device(lf, lm, **kw)
    assert got.shape == (3, 20, 25, 30) and np.array_equal(host(got), host(want))


def test_label_pair_options_errors_and_profile(N, M, labels_pair):
    """The label entry treats option values like the feature entry (same exceptions), accepts `mult` and `out`, and records the stage
    interval "label_features" where the MIND path records "mind"."""
    lf, lm, ff, fm = labels_pair
    with pytest.raises(UnboundLocalError):
        N.register_labels_device(lf, lm, grid_sp=4, disp_hw=2, selected_niter=0)
    with pytest.raises(ValueError, match="cost must be"):
        N.register_labels_device(lf, lm, grid_sp=4, disp_hw=2, selected_niter=2, cost="ncc")
    with pytest.raises(ValueError, match="equal shape"):
        N.register_labels_device(lf, lm[:, :, :-1], grid_sp=4, disp_hw=2, selected_niter=2)
    even = N.register_labels_device(lf, lm, grid_sp=4, disp_hw=2, selected_niter=2, selected_smooth=2)       # the reference's growing pools
    assert even.shape == (3, 27, 23, 31)
    assert np.array_equal(host(even), host(M.register_pair_device(feat_fixed=ff[0], feat_moving=fm[0], grid_sp=4, disp_hw=2, selected_niter=2, selected_smooth=2)))
    f2, m2 = N.extract_features(lf, lm, mult=0.37, device=DEV)
    out = torch.full((3, 24, 20, 28), 7.0, dtype=torch.float32, device=DEV)
    got = N.register_labels_device(lf, lm, mult=0.37, grid_sp=4, disp_hw=2, selected_niter=2, out=out, profile=1)
    stages = [name for name, _ in M.last_profile()]
    M.set_profiling(0)
    assert got is out and "label_features" in stages and "mind" not in stages and "adam" in stages
    assert np.array_equal(host(out), host(M.register_pair_device(feat_fixed=f2[0], feat_moving=m2[0], grid_sp=4, disp_hw=2, selected_niter=2)))


# ---- 3. against the reference's capture -----------------------------------------------------------------------------------------------
def test_label_pair_vs_reference_golden(N, orc, golden, nnunet):
    """BASELINE configs[3] (tests/golden/nnunet.npz): from the reference's label maps the label entry is bit-identical to the reference at
    the convex stage and to the oracle's float32 restatement after 1, 5 and 20 Adam iterations -- the assertions
    test_nnunet_pipeline_vs_reference_golden makes for the feature entry."""
    g = golden("nnunet")
    gs, hw, gsa = (int(v) for v in g["cfg"])
    lf, lm, ff, fm = nnunet.features(g)
    kw = dict(grid_sp=gs, disp_hw=hw, grid_sp_adam=gsa, ic=True, cost_scale=12.0)
    field = lambda t: np.moveaxis(host(t), 0, -1)
    lf_d, lm_d = dev(lf), dev(lm)
    nnunet.field_checks(g, "convex", field(N.register_labels_device(lf_d, lm_d, lambda_weight=0, **kw)), exact=True)
    for niter in (1, 5, 20):
        out = field(N.register_labels_device(lf_d, lm_d, lambda_weight=1.25, selected_niter=niter, **kw))
        want = orc.convex_adam_pipeline(None, None, lambda_weight=1.25, selected_niter=niter, grid_sp=gs, disp_hw=hw, grid_sp_adam=gsa, features=(ff, fm))
        assert np.array_equal(out, want.astype(np.float32)), niter


# ---- 4. the tensor really is gone ---------------------------------------------------------------------------------------------------
def test_label_pair_allocates_no_onehot_volume(N):
    """(48, 48, 48), 40 labels, device-resident maps: across a call the allocator's peak rises by at most workspace + field + 1 MB, which is
    below ONE (C, H, W, D) float32 volume (tests/test_label_pooled_abi.py checks that part without a GPU); the feature entry holds two."""
    from convexadam_amd import _lib
    from convexadam_amd._lib import PairParams
    shape, Cn = (48, 48, 48), 40
    rng = np.random.default_rng(3)
    lf, lm = dev(rng.integers(0, Cn, shape).astype(np.float32)), dev(rng.integers(0, Cn, shape).astype(np.float32))
    kw = dict(grid_sp=4, disp_hw=2, grid_sp_adam=2, selected_niter=2)
    _lib.release_workspaces()
    N.register_labels_device(lf, lm, **kw)                             # warm-up: code objects, the histogram's first launch
    _lib.release_workspaces()                                          # the measured call allocates its workspace itself
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = N.register_labels_device(lf, lm, **kw)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    p = PairParams(48, 48, 48, 1, 2, 1.25, 4, 2, 2, 0, 2, 1, Cn, 12.0)
    nws = _lib.lib().cvx_register_label_pair_workspace_bytes(C.byref(p))
    bound = nws + out.numel() * 4 + (1 << 20)
    print("allocator peak rise %d B, workspace query %d B, bound %d B, one one-hot volume %d B" % (rise, nws, bound, Cn * 48 ** 3 * 4))
    assert rise <= bound < Cn * 48 ** 3 * 4
    assert out.shape == (3, 48, 48, 48) and bool(torch.isfinite(out).all())


@pytest.mark.parametrize("lam,ic", [(1.25, 1), (0.0, 1), (1.25, 0), (0.0, 0)])
def test_label_pair_workspace_contract(N, labels_pair, lam, ic):
    """cvx_register_label_pair_f32 with EXACTLY the queried workspace, cut from the front of a buffer whose tail holds a pattern: the same
    bits as through the grow-only Python workspace, the tail intact; one byte less is refused and the output stays untouched."""
    from convexadam_amd import _lib
    from convexadam_amd._lib import PairParams
    lf, lm, _, _ = labels_pair
    L = _lib.lib()
    _, _, present_d, weights_d, Cn = N._label_channels(lf, lm, DEV)
    par = PairParams(24, 20, 28, 1, 2, lam, 4, 2, 3, 0, 2, ic, Cn, 12.0)
    need = L.cvx_register_label_pair_workspace_bytes(C.byref(par))
    assert need > 0
    tail = 8192
    buf = torch.full((need + tail,), 0xA5, dtype=torch.uint8, device=DEV)
    want = N.register_labels_device(lf, lm, lambda_weight=lam, grid_sp=4, disp_hw=2, selected_niter=3, ic=bool(ic))
    out = torch.full(tuple(want.shape), 7.0, dtype=torch.float32, device=DEV)
    vp = lambda t: C.c_void_p(t.data_ptr())
    call = lambda nbytes: L.cvx_register_label_pair_f32(vp(lf), vp(lm), vp(present_d), vp(weights_d), 10.0, C.byref(par), vp(out), None, vp(buf), nbytes,
                                                       _lib.stream_ptr(DEV))
    assert call(need - 1) == _lib.CVX_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call(need) == 0
    torch.cuda.synchronize()
    assert np.array_equal(host(out), host(want))
    assert bool((buf[need:] == 0xA5).all())
