"""The device pieces of the CuRIOUS rigid registration (l2r_2020_convexAdam_CuRIOUS.py) on the GPU, every comparison bit for bit:

  mask       threshold_pool_mask = torch's CPU F.avg_pool3d((img > t).float(), g, stride=g) > .5                          (:328,330)
  masked     coupled_convex(..., cell_mask=m) = the oracle's coupled_convex on ssd * m, with the plain argmin of the UNMASKED volume as the
             seed (:336-338), `ssd` untouched, and nothing read from the columns of masked-out cells
  centroids  label_centroids' integer sums = numpy int64 sums; landmark_tre = the float64 restatement of :312-319.  The script's own
             float32 `mesh[:, idx].mean(1)` is compared with the exact centroid as a statement about the SCRIPT: for a label of N <= 10^5
             voxels it lies within 1.01 N 2^-24 max|coordinate| (first-order worst case of any summation order of N float32 terms plus the
             division, 1 % for the higher-order terms at that N); the kernel's sums are exact and carry no tolerance.
  stage      convex_stage = the composition of the single operators with ssd.mul_(mask) (small and at the script's size 256 x 256 x 288,
             C = 24, half-width 6), = the CPU oracle's operators, = the reference script's own results (tests/golden/curious.npz)
  samples    rigid_samples(coarse) = _field_samples(resize_trilinear(coarse)) rows, cells on every face, edge and corner, g = 1..7, full size
  whole call convex_adam_rigid(...).T = least_trimmed_rigid on the rows sampled from the stage's field, bit for bit; T of the golden's rows
             by the criterion of test_gpu_rigid.py; a known motion is recovered (a check of wiring and direction convention, printed)
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"


# ---- mask ----------------------------------------------------------------------------------------------------------------------------
def mask_ref(img, t, g):
    return (F.avg_pool3d((img > t).float()[None, None], g, stride=g) > .5)[0, 0]


@pytest.mark.parametrize("g", range(1, 9))
def test_mask_kernel_equals_torch_for_every_grid_spacing(g):
    from convexadam_amd.rigid import threshold_pool_mask
    gen = torch.Generator().manual_seed(100 + g)
    for ext in ((4 * g, 3 * g, 5 * g), (4 * g + g // 2, 3 * g + (g - 1), 2 * g + 1 if g > 1 else 3), (g, g, g), (g, 2 * g, 7 * g + g - 1)):
        # integer-valued data so that thresholds AT data values occur; smooth enough that cells near count = g^3 / 2 occur
        img = torch.round(8 * F.interpolate(torch.randn(1, 1, 3, 3, 3, generator=gen), size=ext, mode="trilinear", align_corners=False)[0, 0]
                          + 2 * torch.randn(ext, generator=gen)).contiguous()
        for t in (0.0, float(img.median()), float(img.flatten()[7 % img.numel()]), 10.0, -1e30, 1e30):
            got = threshold_pool_mask(img.to(DEV), t, g)
            assert got.dtype == torch.bool and tuple(got.shape) == tuple(s // g for s in ext)
            assert torch.equal(got.cpu(), mask_ref(img, t, g)), (g, ext, t)
        nan = img.clone()
        nan.view(-1)[torch.randperm(nan.numel(), generator=gen)[:max(1, nan.numel() // 5)]] = float("nan")
        assert torch.equal(threshold_pool_mask(nan.to(DEV), -5.0, g).cpu(), mask_ref(nan, -5.0, g)), (g, ext, "nan")
        assert torch.equal(threshold_pool_mask(nan.to(DEV)[None, None], 0.0, g).cpu(), mask_ref(nan, 0.0, g))


def test_mask_kernel_hits_every_count_of_a_cell():
    """Every count 0..g^3 of voxels above the threshold in one cell: the rule 2 * count > g^3 against torch's float expression."""
    from convexadam_amd.rigid import threshold_pool_mask
    for g in range(1, 9):
        n = g ** 3
        img = torch.zeros(n + 1, n, dtype=torch.float32)
        for c in range(n + 1):
            img[c, :c] = 20.0
        gen = torch.Generator().manual_seed(g)
        img = torch.stack([row[torch.randperm(n, generator=gen)] for row in img])                 # which voxels of the cell: any
        vol = img.reshape(n + 1, g, g, g).permute(1, 0, 2, 3).reshape(g, (n + 1) * g, g)           # cells side by side along W
        vol = vol.contiguous()
        assert torch.equal(threshold_pool_mask(vol.to(DEV), 10.0, g).cpu(), mask_ref(vol, 10.0, g)), g


# ---- masked coupled convex -----------------------------------------------------------------------------------------------------------
def run_masked(ssd, am, hw, mask):
    from convexadam_amd.convex_adam_utils import coupled_convex, disp_mesh_t
    K, h, w, d = ssd.shape
    s = torch.from_numpy(ssd).to(DEV)
    keep = s.clone()
    out = coupled_convex(s, torch.from_numpy(am).to(DEV), disp_mesh_t(hw, DEV), 1, (h, w, d),
                         cell_mask=None if mask is None else torch.from_numpy(mask).to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(s.view(torch.int32), keep.view(torch.int32)), "the cost volume was written"
    return out[0].cpu().numpy()


def check_masked(orc, ssd, hw, mask, am=None):
    ssd = np.ascontiguousarray(ssd, np.float32)
    am = np.argmin(ssd, 0).astype(np.int64) if am is None else am         # of the UNMASKED volume, as the script passes it
    want = orc.coupled_convex(ssd * mask[None].astype(np.float32), am, orc.disp_mesh(hw), hw)
    got = run_masked(ssd, am, hw, mask)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), "masked coupled convex differs from the oracle on ssd * mask"
    return got


def random_volume(rng, hw, ext, smooth=True):
    """A cost volume with structure: a paraboloid around a per-cell random displacement plus noise (plain noise has no basin)."""
    n = 2 * hw + 1
    h, w, d = ext
    g = np.stack(np.meshgrid(*[np.arange(n) - hw] * 3, indexing="ij")).reshape(3, -1, 1, 1, 1).astype(np.float32)
    c = rng.uniform(-hw, hw, (3, 1, h, w, d)).astype(np.float32)
    ssd = ((g - c) ** 2).sum(0) * np.float32(1.5) + rng.random((n ** 3, h, w, d), dtype=np.float32) * np.float32(0.3 if smooth else 3.0)
    return np.ascontiguousarray(ssd, np.float32)


@pytest.mark.parametrize("hw", range(1, 9))
def test_masked_coupled_convex_equals_oracle_on_the_product(orc, hw):
    rng = np.random.default_rng(40 + hw)
    ext = (7, 6, 9) if hw <= 4 else (5, 4, 6)               # v = 378 (v % 4 == 2), 120
    ssd = random_volume(rng, hw, ext)
    v = int(np.prod(ext))
    ones, zeros = np.ones(ext, np.uint8), np.zeros(ext, np.uint8)
    one_kept, one_dropped = zeros.copy(), ones.copy()
    one_kept.reshape(-1)[v // 3] = 1
    one_dropped.reshape(-1)[v // 2] = 0
    full = check_masked(orc, ssd, hw, ones)
    assert np.array_equal(full.view(np.int32), run_masked(ssd, np.argmin(ssd, 0).astype(np.int64), hw, None).view(np.int32))
    for m in (zeros, one_kept, one_dropped, (rng.random(ext) < 0.85).astype(np.uint8), (rng.random(ext) < 0.15).astype(np.uint8)):
        check_masked(orc, ssd, hw, m)
    half = check_masked(orc, ssd, hw, (rng.random(ext) < 0.5).astype(np.uint8))
    assert not np.array_equal(half, full), "a half-empty mask left the field unchanged: the case tests nothing"


@pytest.mark.parametrize("ext", [(1, 1, 1), (1, 5, 1), (2, 1, 7), (1, 2, 2), (2, 2, 2), (3, 5, 7), (4, 4, 4), (1, 1, 9), (6, 1, 2)])
def test_masked_coupled_convex_on_thin_and_odd_extents(orc, ext):
    rng = np.random.default_rng(sum(ext) * 7 + ext[0])
    for hw in (2, 3):
        ssd = random_volume(rng, hw, ext, smooth=False)
        for p in (0.0, 0.5, 1.0):
            check_masked(orc, ssd, hw, (rng.random(ext) < p).astype(np.uint8))


def test_masked_coupled_convex_with_ties_at_the_minimum_in_kept_cells(orc):
    rng = np.random.default_rng(5)
    hw, ext = 3, (6, 7, 5)
    ssd = np.round(random_volume(rng, hw, ext) * 4) / 4                     # coarse values: many equal entries per column
    ssd[:, 2:4] = np.minimum(ssd[:, 2:4], np.float32(0.25))                 # whole plateaus at the minimum
    ssd[:, 0, 0] = 0.0                                                      # kept all-zero columns beside masked-out ones
    ssd = ssd.astype(np.float32)
    for p in (1.0, 0.6, 0.3):
        m = (rng.random(ext) < p).astype(np.uint8)
        m[0, 0, :3] = 1
        check_masked(orc, ssd, hw, m)


def test_masked_coupled_convex_streams_and_prunes_to_the_same_bits(orc):
    """Both pass implementations (branch and bound, streaming scans) read the mask: option no_prune."""
    from convexadam_amd import _lib
    rng = np.random.default_rng(9)
    hw, ext = 3, (8, 6, 10)                                                 # v % 4 == 0: the four-voxel streaming kernel
    ssd = random_volume(rng, hw, ext)
    m = (rng.random(ext) < 0.5).astype(np.uint8)
    L = _lib.lib()
    for name, val in ((b"no_prune", 1), (b"prune_stream_above", 0)):
        old = L.cvx_get_option(name)
        assert L.cvx_set_option(name, val) == 0
        try:
            check_masked(orc, ssd, hw, m)
            check_masked(orc, np.ascontiguousarray(ssd[:, :7, :, :9]), hw, np.ascontiguousarray(m[:7, :, :9]))       # v % 4 != 0
        finally:
            assert L.cvx_set_option(name, old) == 0


def test_masked_coupled_convex_on_the_zero_background_pair(orc):
    """Features of a skull-stripped pair: flat zero columns in kept cells beside the masked-out ones, and a mask from the mask kernel."""
    from convexadam_amd.phantom import zero_background_pair
    from convexadam_amd.rigid import threshold_pool_mask
    shape, g, hw = (40, 36, 44), 4, 3
    fix, mov = zero_background_pair(shape)
    ff = orc.avgpool_stride(orc.mindssc(fix.numpy(), 1, 2), g)
    fm = orc.avgpool_stride(orc.mindssc(mov.numpy(), 1, 2), g)
    ssd, am = orc.correlate(ff, fm, hw)
    for img in (fix, mov):
        m = threshold_pool_mask((img != 0).float().to(DEV), 0.5, g).cpu().numpy().astype(np.uint8)
        assert 0.05 < m.mean() < 0.95
        check_masked(orc, ssd, hw, m, am)


def test_non_finite_values_in_masked_out_columns_do_not_reach_the_result(orc):
    rng = np.random.default_rng(21)
    hw, ext = 2, (6, 5, 7)
    ssd = random_volume(rng, hw, ext)
    m = (rng.random(ext) < 0.5).astype(np.uint8)
    am = np.argmin(ssd, 0).astype(np.int64)
    clean = run_masked(ssd, am, hw, m)
    dirty = ssd.copy()
    zs, ys, xs = np.nonzero(m == 0)
    for i, bad in zip(range(0, len(zs), 3), [np.nan, np.inf, -np.inf] * len(zs)):
        dirty[rng.integers(0, ssd.shape[0]), zs[i], ys[i], xs[i]] = bad
    dirty[:, zs[1], ys[1], xs[1]] = np.nan
    assert np.array_equal(run_masked(dirty, am, hw, m).view(np.int32), clean.view(np.int32))
    assert np.array_equal(clean.view(np.int32), orc.coupled_convex(ssd * m[None], am, orc.disp_mesh(hw), hw).view(np.int32))


def test_a_nan_in_a_kept_column_follows_the_unmasked_rule(orc):
    rng = np.random.default_rng(22)
    hw, ext = 2, (5, 6, 4)
    ssd = random_volume(rng, hw, ext)
    m = (rng.random(ext) < 0.6).astype(np.uint8)
    zs, ys, xs = np.nonzero(m)
    ssd[17, zs[0], ys[0], xs[0]] = np.nan
    ssd[3, zs[-1], ys[-1], xs[-1]] = np.nan
    with np.errstate(invalid="ignore"):
        am = np.argmin(ssd, 0).astype(np.int64)
        check_masked(orc, ssd, hw, m, am)


# ---- centroids -----------------------------------------------------------------------------------------------------------------------
def sums_ref(seg, max_label):
    seg = np.asarray(seg)
    lab = seg.astype(np.int64).reshape(-1)
    ok = (lab >= 0) & (lab <= max_label)
    acc = np.zeros((max_label + 1, 4), np.int64)
    coords = np.stack(np.meshgrid(*[np.arange(s) for s in seg.shape], indexing="ij")).reshape(3, -1)
    acc[:, 0] = np.bincount(lab[ok], minlength=max_label + 1)
    for a in range(3):                                                   # float64 weights: exact, the sums stay far below 2^53
        acc[:, 1 + a] = np.bincount(lab[ok], weights=coords[a][ok].astype(np.float64), minlength=max_label + 1).astype(np.int64)
    return acc


def device_sums(seg, max_label):
    from convexadam_amd.rigid import label_centroids
    cent, counts = label_centroids(torch.as_tensor(seg).to(DEV), max_label, return_counts=True)
    return cent.numpy(), counts.numpy()


@pytest.mark.parametrize("case", ["random255", "blobs", "absent", "full", "one_row", "out_of_range"])
def test_label_centroid_sums_are_the_integer_sums(case):
    rng = np.random.default_rng(3)
    if case == "random255":
        seg, ml = rng.integers(0, 256, (37, 29, 50)).astype(np.float32), 255
    elif case == "blobs":
        from convexadam_amd.phantom import label_phantom
        seg, ml = label_phantom((48, 40, 70), 12, 4).numpy(), 11
    elif case == "absent":
        seg, ml = rng.integers(0, 5, (20, 21, 22)).astype(np.float32) * 3, 14
    elif case == "full":
        seg, ml = np.full((33, 17, 65), 7, np.float32), 9
    elif case == "one_row":
        seg, ml = rng.integers(0, 3, (1, 1, 131)).astype(np.float32), 2
    else:
        seg, ml = rng.integers(-3, 40, (16, 18, 20)).astype(np.float32), 20
        seg[0, 0, :4] = [np.nan, 1e30, -1e30, 20.75]                  # NaN / huge: no label; 20.75 truncates to 20 like .short()
    acc = sums_ref(np.nan_to_num(seg, nan=-5.0, posinf=-5.0, neginf=-5.0).clip(-5, 1e6), ml)
    cent, counts = device_sums(seg, ml)
    assert np.array_equal(counts, acc[:, 0])
    with np.errstate(invalid="ignore", divide="ignore"):
        want = acc[:, 1:].astype(np.float64) / acc[:, :1].astype(np.float64)
    assert np.array_equal(np.isnan(cent), np.isnan(want)) and np.array_equal(np.nan_to_num(cent), np.nan_to_num(want))
    assert np.array_equal(np.isnan(cent[:, 0]), acc[:, 0] == 0)


def test_label_centroids_at_the_script_size_and_against_its_float32_mean():
    """256 x 256 x 288 with 15 landmark spheres (the script's volumes) + one large label; exact sums, and the script's float32
    expression within the summation-error bound of the docstring."""
    H, W, D = 256, 256, 288
    rng = np.random.default_rng(8)
    seg = np.zeros((H, W, D), np.float32)
    zz, yy, xx = np.ogrid[:H, :W, :D]
    for l in range(1, 16):
        c = rng.uniform(30, 220, 3)
        r = rng.uniform(2.0, 9.0) if l < 15 else 28.0
        seg[(zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 <= r * r] = l
    ml = 16                                                             # label 16 absent
    cent, counts = device_sums(seg, ml)
    lab = seg.astype(np.int64).reshape(-1)
    assert np.array_equal(counts, np.bincount(lab, minlength=ml + 1))
    mesh = torch.stack(torch.meshgrid(torch.arange(H), torch.arange(W), torch.arange(D), indexing="ij")).reshape(3, -1).float()
    worst = 0.0
    for l in range(1, ml + 1):
        idx = np.nonzero(lab == l)[0]
        if l == 16:
            assert idx.size == 0 and np.isnan(cent[l]).all()
            continue
        z, y, x = np.unravel_index(idx, (H, W, D))
        exact = np.array([z.sum(), y.sum(), x.sum()], np.int64).astype(np.float64) / idx.size
        assert np.array_equal(cent[l], exact), l
        if idx.size <= 100000:
            script = mesh[:, torch.from_numpy(idx)].mean(1).double().numpy()
            bound = 1.01 * idx.size * 2.0 ** -24 * max(z.max(), y.max(), x.max())
            err = np.abs(script - exact).max()
            worst = max(worst, err / bound)
            assert err <= bound, (l, idx.size, err, bound)
    print("script float32 centroid vs exact: largest error / bound = %.3g" % worst)


def test_landmark_tre_is_the_scripts_expression():
    from convexadam_amd.rigid import landmark_tre
    rng = np.random.default_rng(12)
    shape = (40, 44, 36)
    a = np.zeros(shape, np.float32)
    b = np.zeros(shape, np.float32)
    for l in range(1, 7):
        p = rng.integers(4, 30, 3)
        a[p[0]:p[0] + 3, p[1]:p[1] + 2, p[2]:p[2] + 4] = l
        if l != 4:                                                      # label 4 absent from b: NaN, like the script's empty mean
            q = p + rng.integers(-3, 4, 3)
            b[q[0]:q[0] + 3, q[1]:q[1] + 3, q[2]:q[2] + 2] = l
    b[0, 0, 0] = 6
    tre = landmark_tre(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)).numpy()
    assert tre.shape == (6,)
    mesh = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")).reshape(3, -1).astype(np.float64)
    for l in range(1, 7):
        ia, ib = np.nonzero(a.reshape(-1) == l)[0], np.nonzero(b.reshape(-1) == l)[0]
        if l == 4:
            assert np.isnan(tre[l - 1])
            continue
        want = np.sqrt(((mesh[:, ia].mean(1) - mesh[:, ib].mean(1)) ** 2).sum())
        assert abs(tre[l - 1] - want) <= 1e-12 * max(1.0, want)
    assert np.array_equal(np.nan_to_num(landmark_tre(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), max_label=6).numpy()),
                          np.nan_to_num(tre))


# ---- the convex stage in one call ----------------------------------------------------------------------------------------------------
def phantom_case(shape, g):
    """Zero-background fixed image (40 x + 100 inside the ellipsoid), a rigidly moved copy, a second modality of it and the matrix A."""
    from convexadam_amd.phantom import ellipsoid_mask, zero_background_pair
    fix, _ = zero_background_pair(shape)
    fixed = ((40.0 * fix + 100.0) * ellipsoid_mask(shape, 0.42)).contiguous()
    ang = np.deg2rad(4.0)
    A = torch.tensor([[np.cos(ang), -np.sin(ang), 0.0, 0.15], [np.sin(ang), np.cos(ang), 0.0, -0.16], [0.0, 0.0, 1.0, 0.14]], dtype=torch.float32)
    grid = F.affine_grid(A[None], (1, 1) + tuple(shape), align_corners=False)
    moving = F.grid_sample(fixed[None, None], grid, mode="bilinear", padding_mode="zeros", align_corners=False)[0, 0].contiguous()
    moving2 = torch.where(moving > 0, 300.0 - 0.004 * (moving - 100.0) ** 2 - moving, torch.zeros(())).clamp_min(0.0).contiguous()   # non-linear map
    return fixed, moving, moving2, A


def stage_features(fixed, movs, g, r=3, dil=3):
    from convexadam_amd.convex_adam_utils import mind_pooled
    ff = mind_pooled(fixed.to(DEV)[None, None], r, dil, g)
    return torch.cat([ff] * len(movs), 1), torch.cat([mind_pooled(m.to(DEV)[None, None], r, dil, g) for m in movs], 1)


def compose_stage(ff, fm, g, hw, shape, mf, mm, it):
    """What a user writes from the single operators, with the read-modify-write of the cost volume the stage avoids."""
    from convexadam_amd.convex_adam_utils import correlate, coupled_convex, disp_mesh_t, inverse_consistency, resize_trilinear
    mesh = disp_mesh_t(hw, DEV)
    Cn = int(ff.shape[1])

    def direction(a, b, m):
        ssd, am = correlate(a, b, hw, g, shape, ch=Cn)
        if m is not None:
            ssd.mul_(m.to(DEV).float())
        out = coupled_convex(ssd, am, mesh, g, shape)
        del ssd
        return out

    soft = direction(ff, fm, mf)
    if it == 0:
        return soft, resize_trilinear(soft * g, shape), soft, None
    soft_ = direction(fm, ff, mm)
    h, w, d = [int(s) for s in soft.shape[2:]]
    scale = torch.tensor([h - 1, w - 1, d - 1], dtype=torch.float32, device=DEV).view(1, 3, 1, 1, 1) / 2
    ice, _ = inverse_consistency((soft / scale).flip(1), (soft_ / scale).flip(1), iter=it)
    coarse = ice.flip(1) * scale * g
    return coarse, resize_trilinear(coarse, shape), soft, soft_


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("it", [0, 5])
def test_convex_stage_equals_the_operator_composition_and_the_oracle(orc, it):
    from convexadam_amd import _lib
    from convexadam_amd.rigid import convex_stage, threshold_pool_mask
    shape, g, hw = (48, 42, 54), 6, 3
    fixed, moving, moving2, _ = phantom_case(shape, g)
    ff, fm = stage_features(fixed, [moving, moving2], g)
    mf, mm = threshold_pool_mask(fixed.to(DEV), 10.0, g), threshold_pool_mask(moving.to(DEV), 10.0, g)
    for m in (mf, mm):
        assert 0.25 < float(m.float().mean()) < 0.75
    coarse, hr = convex_stage(ff, fm, g, hw, shape, mf, mm, it)
    want_c, want_hr, soft, soft_ = compose_stage(ff, fm, g, hw, shape, mf, mm, it)
    assert bits_equal(coarse, want_c) and bits_equal(hr, want_hr)
    assert float(coarse.abs().max()) > 0, "an all-zero field tests nothing"
    plain_c, _ = convex_stage(ff, fm, g, hw, shape, None, None, it, full_res=False)
    assert not bits_equal(plain_c, coarse), "the masks changed nothing: the case cannot fail with the mask ignored"
    assert bits_equal(plain_c, compose_stage(ff, fm, g, hw, shape, None, None, it)[0])
    # a second call in the same workspace, and one in a fresh workspace
    again_c, again_hr = convex_stage(ff, fm, g, hw, shape, mf, mm, it)
    assert bits_equal(again_c, coarse) and bits_equal(again_hr, hr)
    _lib.release_workspaces()
    fresh_c, fresh_hr = convex_stage(ff, fm, g, hw, shape, mf, mm, it)
    assert bits_equal(fresh_c, coarse) and bits_equal(fresh_hr, hr)
    # the CPU oracle's operators on ssd * mask, from the same features
    F_, M_ = ff[0].cpu().numpy(), fm[0].cpu().numpy()
    mesh = orc.disp_mesh(hw)

    def direction(a, b, m):
        ssd, am = orc.correlate(a, b, hw)
        return orc.coupled_convex(ssd * m.cpu().numpy()[None].astype(np.float32), am, mesh, hw)

    s1 = direction(F_, M_, mf)
    if it == 0:
        o_c = s1
        o_hr = orc.resize_trilinear(s1 * np.float32(g), shape)
    else:
        s2 = direction(M_, F_, mm)
        scale = (np.array(s1.shape[1:], np.float32) - 1).reshape(3, 1, 1, 1) / np.float32(2)
        ice, _ = orc.inverse_consistency((s1 / scale)[::-1], (s2 / scale)[::-1], it)
        o_c = ice[::-1] * scale * np.float32(g)
        o_hr = orc.resize_trilinear(o_c, shape)
        assert np.array_equal(soft_[0].cpu().numpy().view(np.int32), s2.view(np.int32))
    assert np.array_equal(soft[0].cpu().numpy().view(np.int32), s1.view(np.int32))
    assert np.array_equal(coarse[0].cpu().numpy().view(np.int32), np.ascontiguousarray(o_c, np.float32).view(np.int32))
    assert np.array_equal(hr[0].cpu().numpy().view(np.int32), o_hr.view(np.int32))


@pytest.mark.parametrize("it", [0, 5])
def test_convex_stage_at_the_script_size(it):
    """256 x 256 x 288, C = 24, grid 6, search half-width 6 (2197 x 42 x 42 x 48 cost volume), ellipsoid masks."""
    from convexadam_amd.phantom import ellipsoid_mask, phantom
    from convexadam_amd.rigid import convex_stage, threshold_pool_mask
    shape, g, hw = (256, 256, 288), 6, 6
    fixed = phantom(shape, 3, 30)
    moving = torch.roll(phantom(shape, 3, 31), (7, -5, 9), (0, 1, 2)).contiguous()
    ff, fm = stage_features(fixed, [moving, (moving * moving).contiguous()], g)
    mf = threshold_pool_mask(ellipsoid_mask(shape, 0.40).to(DEV), 0.5, g)
    mm = threshold_pool_mask(ellipsoid_mask(shape, 0.38, shift=(5, -4, 6)).to(DEV), 0.5, g)
    coarse, hr = convex_stage(ff, fm, g, hw, shape, mf, mm, it)
    want_c, want_hr, _, _ = compose_stage(ff, fm, g, hw, shape, mf, mm, it)
    assert bits_equal(coarse, want_c) and bits_equal(hr, want_hr)
    assert float(coarse.abs().max()) > 0
    again_c, again_hr = convex_stage(ff, fm, g, hw, shape, mf, mm, it)
    assert bits_equal(again_c, coarse) and bits_equal(again_hr, hr)


# ---- the whole call ------------------------------------------------------------------------------------------------------------------
def test_nearest_label_warp_uses_the_scripts_coordinates():
    """tre_deformable goes through warp_labels_nearest, whose grid is grid0 + disp.flip / ((size - 1) / 2); the script's (:356-357,376) is
    affine + disp / (size - 1) * 2 -- equal, halving a divisor doubles the quotient exactly.  Checked against torch on the CPU."""
    from convexadam_amd.convexAdam_hyper_util import warp_labels_nearest
    from convexadam_amd.phantom import label_phantom
    shape = (30, 33, 28)
    seg = label_phantom(shape, 9, 2)
    gen = torch.Generator().manual_seed(4)
    disp = 5 * F.interpolate(torch.randn(1, 3, 4, 4, 4, generator=gen), size=shape, mode="trilinear", align_corners=False)
    affine = F.affine_grid(torch.eye(3, 4)[None], (1, 1) + shape, align_corners=False)
    disp0 = (disp.permute(0, 2, 3, 4, 1) / torch.tensor([shape[0] - 1, shape[1] - 1, shape[2] - 1]).view(1, 1, 1, 1, 3) * 2).flip(4)
    want = F.grid_sample(seg[None, None], affine + disp0, align_corners=False, mode="nearest")[0, 0]
    got = warp_labels_nearest(seg.to(DEV), disp.to(DEV)).cpu()
    assert torch.equal(got, want)


def cell_distance(Ta, Tb, pts, shape):
    """Mean distance in voxels between the images of the kept cells under two (4, 4) transforms of normalised (x, y, z, 1) rows."""
    half = torch.tensor([shape[2] - 1, shape[1] - 1, shape[0] - 1], dtype=torch.float64) / 2
    a, b = pts.double() @ Ta.double().t(), pts.double() @ Tb.double().t()
    return float((((a - b)[:, :3] * half) ** 2).sum(1).sqrt().mean())


def test_convex_adam_rigid_is_its_parts_and_recovers_a_known_motion():
    """Wiring and direction convention (the bit comparisons above grade the arithmetic): moving = fixed pulled through affine_grid(A),
    A = 4 degrees + about 7-8 voxels per axis; T must lie closer to inverse(A) than the identity does."""
    from convexadam_amd.rigid import _field_samples, convex_adam_rigid, convex_stage, least_trimmed_rigid, threshold_pool_mask
    shape, g, hw = (96, 90, 108), 6, 4
    fixed, moving, moving2, A = phantom_case(shape, g)
    res = convex_adam_rigid(fixed.to(DEV), [moving.to(DEV), moving2.to(DEV)], grid_sp=g, disp_hw=hw)
    assert res.disp_hr is None and res.tre_rigid is None and tuple(res.T.shape) == (4, 4)
    mf, mm = threshold_pool_mask(fixed.to(DEV), 10.0, g), threshold_pool_mask(moving.to(DEV), 10.0, g)
    assert torch.equal(res.mask_fix, mf) and torch.equal(res.mask_mov, mm)
    ff, fm = stage_features(fixed, [moving, moving2], g)
    _, hr = convex_stage(ff, fm, g, hw, shape, mf, mm, 5)
    T1, T2 = _field_samples(hr, mf, g)
    assert bits_equal(res.T, least_trimmed_rigid(T1, T2, 15))
    with_field = convex_adam_rigid(fixed.to(DEV), [moving.to(DEV), moving2.to(DEV)], grid_sp=g, disp_hw=hw, return_field=True)
    assert bits_equal(with_field.T, res.T) and bits_equal(with_field.disp_hr, hr)
    A4 = torch.eye(4, dtype=torch.float64)
    A4[:3] = A.double()
    Ainv = torch.linalg.inv(A4)
    before = cell_distance(torch.eye(4), Ainv, T1.cpu(), shape)
    after = cell_distance(res.T.cpu(), Ainv, T1.cpu(), shape)
    print("known motion: mean distance of the kept cells to inverse(A): identity %.2f voxels, T %.2f voxels; masks keep %.0f %% / %.0f %%"
          % (before, after, 100 * float(mf.float().mean()), 100 * float(mm.float().mean())))
    assert after < before
    # landmarks: label blobs inside the fixed image, moved with the same A
    seg = torch.zeros(shape)
    rng = np.random.default_rng(2)
    for l in range(1, 9):
        c = [int(rng.integers(s // 3, 2 * s // 3)) for s in shape]
        seg[c[0] - 2:c[0] + 3, c[1] - 2:c[1] + 3, c[2] - 2:c[2] + 3] = l
    seg_m = F.grid_sample(seg[None, None], F.affine_grid(A[None], (1, 1) + tuple(shape), align_corners=False), mode="nearest", align_corners=False)[0, 0]
    scored = convex_adam_rigid(fixed.to(DEV), [moving.to(DEV), moving2.to(DEV)], grid_sp=g, disp_hw=hw, seg_fixed=seg.to(DEV), seg_moving=seg_m.to(DEV))
    assert bits_equal(scored.T, res.T) and scored.disp_hr is not None
    for t in (scored.tre_before, scored.tre_deformable, scored.tre_rigid):
        assert t.dtype == torch.float64 and tuple(t.shape) == (int(seg_m.max()),)
    print("landmark TRE (mean over labels present): before %.2f, deformable %.2f, rigid %.2f voxels"
          % tuple(float(np.nanmean(t.numpy())) for t in (scored.tre_before, scored.tre_deformable, scored.tre_rigid)))
    from convexadam_amd.rigid import affine_warp, landmark_tre
    assert torch.equal(torch.nan_to_num(scored.tre_rigid),
                       torch.nan_to_num(landmark_tre(seg.to(DEV), affine_warp(seg_m.to(DEV)[None], res.T, mode="nearest")[0], int(seg_m.max()))))


def test_convex_adam_rigid_names_the_threshold_when_nothing_is_kept():
    from convexadam_amd.rigid import convex_adam_rigid
    img = torch.rand(24, 24, 24).to(DEV)
    with pytest.raises(ValueError, match="mask_thresh"):
        convex_adam_rigid(img, img, grid_sp=6, disp_hw=2, mask_thresh=10.0)


# ---- the reference script's own results (tests/golden/curious.npz) -------------------------------------------------------------------
def test_convex_stage_reproduces_the_reference_script(golden):
    from convexadam_amd.rigid import _field_samples, convex_stage, least_trimmed_rigid, rigid_from_field
    from test_gpu_rigid import lts64
    G = golden("curious")
    g, hw, it, lts = int(G["grid_sp"]), int(G["disp_hw"]), int(G["ic_iters"]), int(G["lts_iters"])
    shape = tuple(int(s) for s in G["shape"])
    ff, fm = torch.from_numpy(G["feat_fix"]).to(DEV)[None], torch.from_numpy(G["feat_mov"]).to(DEV)[None]
    mf, mm = torch.from_numpy(G["mask_fix"]).to(DEV), torch.from_numpy(G["mask_mov"]).to(DEV)

    def same(t, key):
        return np.array_equal(t.cpu().numpy().view(np.int32), np.ascontiguousarray(G[key]).view(np.int32))

    assert same(convex_stage(ff, fm, g, hw, shape, mf, None, 0, full_res=False)[0][0], "soft_fwd")
    assert same(convex_stage(fm, ff, g, hw, shape, mm, None, 0, full_res=False)[0][0], "soft_rev")
    assert same(convex_stage(ff, fm, g, hw, shape, None, None, 0, full_res=False)[0][0], "soft_fwd_plain")
    coarse, hr = convex_stage(ff, fm, g, hw, shape, mf, mm, it)
    assert same(coarse[0], "coarse") and same(hr[0, :, ::3].contiguous(), "disp_hr_z3")
    assert int(hr.contiguous().view(torch.int32).long().sum()) == int(G["disp_hr_bitsum"])
    T1, T2 = _field_samples(hr, mf, g)
    assert same(T1, "T1") and same(T2, "T2")
    T = rigid_from_field(hr, mf, g, lts).cpu().numpy().astype(np.float64)
    assert np.array_equal(T, least_trimmed_rigid(T1, T2, lts).cpu().numpy().astype(np.float64))
    T64 = lts64(G["T1"].astype(np.float64), G["T2"].astype(np.float64), lts)
    ref_err, err = np.abs(G["R"].astype(np.float64) - T64).max(), np.abs(T - T64).max()
    print("T against the float64 restatement: library %.3g, reference float32 %.3g" % (err, ref_err))
    assert err <= 4 * ref_err + 2e-6


# ---- rigid-fit rows straight from the coarse field -----------------------------------------------------------------------------------
def faces_mask(hwd, rng, p):
    """Random cells plus cells on every face, edge and corner of the grid (their sample points have corners outside the volume or
    clamped interpolation taps)."""
    m = rng.random(hwd) < p
    m[0, :, ::2] = True; m[-1, ::2, :] = True; m[:, 0, ::3] = True; m[::2, -1, :] = True; m[:, ::2, 0] = True; m[::3, :, -1] = True
    for z in (0, -1):
        for y in (0, -1):
            for x in (0, -1):
                m[z, y, x] = True
    return torch.from_numpy(m)


@pytest.mark.parametrize("shape,g", [((48, 42, 54), 6), ((40, 36, 44), 4), ((33, 29, 41), 5), ((30, 31, 32), 3), ((24, 20, 28), 1), ((25, 14, 9), 7),
                                     ((256, 256, 288), 6)])
def test_rigid_samples_from_the_coarse_field_are_the_rows_of_the_upsampled_field(shape, g):
    from convexadam_amd.convex_adam_utils import resize_trilinear
    from convexadam_amd.rigid import _field_samples, rigid_samples
    rng = np.random.default_rng(shape[0] * 3 + g)
    hwd = tuple(s // g for s in shape)
    gen = torch.Generator().manual_seed(shape[2] + g)
    coarse = (6.0 * F.interpolate(torch.randn(1, 3, 3, 3, 3, generator=gen), size=hwd, mode="trilinear", align_corners=False)
              + 0.5 * torch.randn(1, 3, *hwd, generator=gen)).to(DEV)
    hr = resize_trilinear(coarse, shape)
    for p in (0.3, 1.0):
        mask = faces_mask(hwd, rng, p)
        T1, T2 = rigid_samples(coarse, mask.to(DEV), g, shape)
        W1, W2 = _field_samples(hr, mask, g)
        assert tuple(T1.shape) == (int(mask.sum()), 4)
        assert bits_equal(T1, W1) and bits_equal(T2, W2)
    assert bits_equal(rigid_samples(coarse[0], mask[None, None].to(DEV).float(), g, shape)[1], W2)


def test_rigid_samples_on_the_golden_and_inside_the_whole_call(golden):
    from convexadam_amd import rigid
    G = golden("curious")
    g, shape = int(G["grid_sp"]), tuple(int(s) for s in G["shape"])
    T1, T2 = rigid.rigid_samples(torch.from_numpy(G["coarse"]).to(DEV), torch.from_numpy(G["mask_fix"]).to(DEV), g, shape)
    assert np.array_equal(T1.cpu().numpy().view(np.int32), G["T1"].view(np.int32)) and np.array_equal(T2.cpu().numpy().view(np.int32), G["T2"].view(np.int32))
    fixed, moving, moving2, _ = phantom_case((48, 42, 54), 6)
    args = (fixed.to(DEV), [moving.to(DEV), moving2.to(DEV)])
    for it in (0, 5):
        got = rigid.convex_adam_rigid(*args, grid_sp=6, disp_hw=3, ic_iters=it).T
        assert rigid.SAMPLE_FROM_COARSE
        rigid.SAMPLE_FROM_COARSE = False
        try:
            want = rigid.convex_adam_rigid(*args, grid_sp=6, disp_hw=3, ic_iters=it).T
        finally:
            rigid.SAMPLE_FROM_COARSE = True
        assert bits_equal(got, want)


def test_rigid_samples_needs_two_cells():
    from convexadam_amd.rigid import rigid_samples
    coarse = torch.zeros(1, 3, 4, 5, 6, device=DEV)
    mask = torch.zeros(4, 5, 6)
    mask[1, 2, 3] = 1
    with pytest.raises(ValueError, match="at least 2"):
        rigid_samples(coarse, mask, 2, (8, 10, 12))
