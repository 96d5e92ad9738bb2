"""Anchors the oracle's generic volume operators on plain torch CPU, at the small edge shapes where the HIP kernels switch code
paths (tests/test_gpu_operators.py grades those kernels against the oracle bit for bit):
  * box_zero   = F.avg_pool3d(k, stride 1, padding k // 2)  (count_include_pad; for extents < k, which avg_pool3d refuses, the same
                 window sum written as an explicit zero F.pad + avg_pool3d without padding: an out-of-range tap adds +0.0, which leaves a
                 sum that starts from +0.0 unchanged);
  * smooth     = the sweep's smoothers: a 5-tap Gaussian as replicate F.pad + F.conv3d along H, then W, then D on a (B*C, 1, ...) view,
                 and the Kovesi box chains as chains of avg_pool3d; the adjoint is torch autograd through the same composition;
  * grid_sample = 5-D F.grid_sample(bilinear, zeros, align_corners=False), including non-finite, huge and lattice-centre coordinates
                 and non-finite volume values.
  * coupled_convex on cost volumes with +Inf entries and the float32 -> half rounding table: the oracle side of
                 tests/test_gpu_fp16_edges.py (inputs in tests/fp16_edge_cases.py).
Everything is bit-exact (np.array_equal with equal_nan and the same NaN positions).  CPU only.

Which ATen convolution kernel runs depends on the thread count and the input size: with one thread a multi-channel adjoint, and at
any thread count a volume of a single voxel, take kernels that round differently.  The oracle restates the kernel every other case
takes, so these tests run torch with at least two threads and anchor the Gaussian on volumes of more than one voxel (the GPU tests
still grade the single voxel against the oracle)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp16_edge_cases as E  # noqa: E402


@pytest.fixture(autouse=True)
def _torch_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(max(n, 2))
    yield
    torch.set_num_threads(n)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.isnan(a), np.isnan(b))


def spiked(shape, seed):
    """Standard normals with +inf, -inf, NaN and -0.0 on the borders and inside (channel 0 only when there are several channels,
    so that the other channels stay finite after a chain of filters)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape).astype(np.float32)
    c0 = x[0]
    c0[0, 0, 0] = np.inf
    c0[-1, -1, -1] = -np.inf
    c0[tuple(s // 2 for s in c0.shape)] = np.nan
    c0[0, -1, 0] = -0.0
    c0.reshape(-1)[rng.integers(0, c0.size, 2)] = -0.0
    return x


def box_torch(x, k):
    """One zero-padded box filter of size k (odd) on (C, H, W, D) float32, torch CPU."""
    t = torch.from_numpy(np.ascontiguousarray(x))[None]
    p = k // 2
    if min(x.shape[1:]) >= k:
        return F.avg_pool3d(t, k, stride=1, padding=p)[0]
    return F.avg_pool3d(F.pad(t, (p,) * 6), k, stride=1, padding=0)[0]


def gauss_weights(sigma):
    """The 5 taps of the sweep's GaussianSmoothing (torch float32 arithmetic of the reference's definition)."""
    s = torch.tensor([sigma])
    n = torch.ceil(s * 3.0 / 2.0).long().item() * 2 + 1
    assert n == 5
    w = torch.exp(-torch.pow(torch.linspace(-(n // 2), n // 2, n), 2) / (2 * torch.pow(s, 2)))
    return w / w.sum()


def gauss_torch(x, w):
    """Separable replicate-padded 5-tap convolution along H, W, D on a (B*C, 1, H, W, D) view."""
    C, H, W, D = x.shape
    y = x.reshape(C, 1, H, W, D)
    for axis in range(3):
        pad = [0] * 6
        pad[2 * (2 - axis)] = pad[2 * (2 - axis) + 1] = 2           # F.pad lists the last axis first
        shape = [1, 1, 1, 1, 1]
        shape[2 + axis] = 5
        y = F.conv3d(F.pad(y, pad, mode="replicate"), w.reshape(shape))
    return y.reshape(C, H, W, D)


def chain_torch(x, sizes):
    y = x[None]
    for k in sizes:
        y = F.avg_pool3d(y, k, stride=1, padding=k // 2)
    return y[0]


def forward_and_adjoint(fn, x, go):
    xt = torch.from_numpy(np.ascontiguousarray(x)).requires_grad_(True)
    y = fn(xt)
    y.backward(torch.from_numpy(np.ascontiguousarray(go)))
    return y.detach().numpy(), xt.grad.numpy()


# ---- box_zero ----------------------------------------------------------------------------------------------------------------
BOX_SHAPES = [(1, 1, 1, 1), (1, 1, 5, 4), (2, 1, 1, 8), (1, 2, 3, 4), (3, 1, 2, 4), (5, 3, 2, 12), (2, 6, 5, 260), (4, 9, 1, 8),
              (3, 10, 11, 12), (3, 10, 11, 13), (1, 7, 2, 16), (2, 40, 48, 56)]


@pytest.mark.parametrize("k", [1, 3, 5, 7, 9])
@pytest.mark.parametrize("shape", BOX_SHAPES)
def test_box_zero_vs_avg_pool3d(orc, shape, k):
    x = spiked(shape, sum(shape) * 10 + k)
    assert same(orc.box_zero(x, k), box_torch(x, k).numpy())
    z = np.zeros(shape, np.float32)
    assert same(orc.box_zero(z, k), box_torch(z, k).numpy())


@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("shape", [(1, 1, 3, 4), (2, 5, 2, 8), (3, 10, 11, 12), (1, 7, 7, 7)])
def test_box_zero_chains_vs_avg_pool3d(orc, shape, k):
    """Three passes in a row (the pipeline's final smoothing); non-finite values spread through the chain."""
    x = spiked(shape, k)
    r, t = x, torch.from_numpy(x)
    for _ in range(3):
        r, t = orc.box_zero(r, k), box_torch(t.numpy(), k)
    assert same(r, t.numpy())


# ---- sweep smoothers ---------------------------------------------------------------------------------------------------------
SMOOTH_SHAPES = [(1, 1, 6, 7), (2, 2, 6, 7), (3, 3, 6, 7), (4, 4, 6, 7), (1, 5, 6, 7), (2, 6, 1, 7), (3, 6, 2, 7),
                 (1, 6, 3, 7), (4, 6, 4, 7), (2, 6, 5, 7), (1, 6, 7, 1), (5, 6, 7, 2), (1, 6, 7, 3), (3, 6, 7, 4), (2, 6, 7, 5),
                 (1, 2, 3, 301), (3, 8, 5, 12), (2, 1, 1, 1), (1, 1, 2, 1)]


@pytest.mark.parametrize("sigma", [0.7, 1.0])
@pytest.mark.parametrize("shape", SMOOTH_SHAPES)
def test_gaussian_smoother_vs_torch_conv3d(orc, shape, sigma):
    """Forward and adjoint; C = 1 is the single-image convolution whose adjoint rounds the products (the oracle's unfused path),
    axes of length 1 .. 5 are shorter than / as long as the stencil (the replicate-padding ranges of the adjoint overlap)."""
    w = gauss_weights(sigma)
    rng = np.random.default_rng(len(shape) * 100 + sum(shape))
    x = rng.standard_normal(shape).astype(np.float32)
    go = rng.standard_normal(shape).astype(np.float32)
    sm = orc.make_smoother(gauss_w=w.numpy())
    fwd, adj = forward_and_adjoint(lambda t: gauss_torch(t, w), x, go)
    assert same(orc.smooth(x, sm), fwd)
    assert same(orc.smooth(go, sm, backward=True), adj)


@pytest.mark.parametrize("sizes", [[3, 3, 3], [3, 3, 3, 3], [3, 3, 3, 5], [3, 3, 5, 5], [3, 5, 5, 5], [5, 5, 5, 5]])
@pytest.mark.parametrize("shape", [(1, 5, 6, 7), (3, 5, 6, 8), (2, 8, 5, 12), (1, 6, 7, 20)])
def test_box_chain_smoother_vs_torch_avg_pool3d(orc, shape, sizes):
    rng = np.random.default_rng(sum(sizes) + sum(shape))
    x = rng.standard_normal(shape).astype(np.float32)
    go = rng.standard_normal(shape).astype(np.float32)
    sm = orc.make_smoother(sizes)
    fwd, adj = forward_and_adjoint(lambda t: chain_torch(t, sizes), x, go)
    assert same(orc.smooth(x, sm), fwd)
    assert same(orc.smooth(go, sm, backward=True), adj)


# ---- grid_sample -------------------------------------------------------------------------------------------------------------
def special_coords(S):
    """Normalised coordinates along an axis of S voxels that hit the sampler's edges."""
    f = np.float32
    on = [(2 * i + 1) / S - 1 for i in (0, S // 2, S - 1)]               # voxel centres (exact for power-of-two S)
    near_clamp = [2e9 / S, -2e9 / S, 2.000001e9 / S, -2.000001e9 / S, 1e9, -1e9, 1.00001e9, -1.00001e9]
    return np.array(on + [1.0, -1.0, 1 + 1 / S, -1 - 1 / S, 0.0, -0.0, np.nan, np.inf, -np.inf, 3e9, -3e9] + near_clamp, f)


def special_grid(h, w, d, n, seed):
    """(n, 1, 1, 3) grid: each coordinate is a special value or uniform in [-1.2, 1.2]."""
    rng = np.random.default_rng(seed)
    g = (rng.random((n, 3)) * 2.4 - 1.2).astype(np.float32)
    for a, S in enumerate((d, w, h)):                                   # grid = (x, y, z) <-> (d, w, h)
        sp = special_coords(S)
        pick = rng.random(n) < 0.5
        g[pick, a] = sp[rng.integers(0, sp.size, int(pick.sum()))]
    g[0] = np.float32(-0.0)
    g[1] = [1.0, 1.0, 1.0]
    g[2] = [-1.0, -1.0, -1.0]
    return g.reshape(n, 1, 1, 3)


def grid_sample_torch(vol, grid):
    return F.grid_sample(torch.from_numpy(vol)[None], torch.from_numpy(grid)[None], mode="bilinear", padding_mode="zeros",
                         align_corners=False)[0].numpy()


@pytest.mark.parametrize("C,vshape", [(1, (1, 1, 1)), (3, (1, 5, 7)), (2, (6, 1, 5)), (12, (4, 6, 1)), (5, (4, 8, 16)), (1, (9, 10, 11))])
def test_grid_sample_vs_torch(orc, C, vshape):
    rng = np.random.default_rng(C * 100 + sum(vshape))
    vol = rng.standard_normal((C,) + vshape).astype(np.float32)
    grid = special_grid(*vshape, 600, C + sum(vshape))
    assert same(orc.grid_sample(vol, grid), grid_sample_torch(vol, grid))
    vol.reshape(C, -1)[:, rng.integers(0, vol[0].size, 2)] = np.inf    # non-finite volume values: +inf * 0 weight is NaN
    vol.reshape(C, -1)[:, -1] = np.nan
    assert same(orc.grid_sample(vol, grid), grid_sample_torch(vol, grid))


def test_grid_sample_lattice_centres_with_non_finite_neighbours(orc):
    """Coordinates exactly on voxel centres: the upper corner along each axis has weight 0, and a +inf / NaN there still makes the
    sample NaN (0 * inf), as in ATen; the same voxel two taps away does not touch the sample."""
    h, w, d = 4, 8, 16
    vol = np.random.default_rng(5).standard_normal((2, h, w, d)).astype(np.float32)
    vol[0, 1, 2, 4] = np.inf
    vol[1, 2, 5, 9] = np.nan
    zz, yy, xx = np.meshgrid(np.arange(h), np.arange(w), np.arange(d), indexing="ij")
    grid = np.stack([(2 * xx + 1) / d - 1, (2 * yy + 1) / w - 1, (2 * zz + 1) / h - 1], -1).astype(np.float32)
    ix = ((grid[..., 0] + np.float32(1)) * np.float32(d) - np.float32(1)) / np.float32(2)
    assert np.array_equal(ix, xx.astype(np.float32))                    # the centres are exact: the weights below are exactly 0 / 1
    got = orc.grid_sample(vol, grid)
    assert same(got, grid_sample_torch(vol, grid))
    assert got[0, 1, 2, 4] == np.inf and np.isnan(got[1, 2, 5, 9])                                     # the voxel itself (weight 1)
    assert np.isnan(got[0, 0, 1, 3]) and np.isnan(got[0, 1, 1, 4]) and np.isnan(got[1, 1, 4, 8])       # 0-weight taps: 0 * inf, 0 * NaN
    assert np.isfinite(got[0, 1, 2, 5]) and np.isfinite(got[0, 1, 3, 4])                               # beyond the upper corner: untouched
    assert np.array_equal(got[:, 3, :, :], vol[:, 3, :, :])                                            # no non-finite value nearby: exact copy


# ---- half precision and +Inf costs: the references of tests/test_gpu_fp16_edges.py -------------------------------------------------
def test_half_table_numpy_vs_torch():
    """numpy's float32 -> float16 cast (the expected value of the GPU rounding tests) equals torch's at every boundary: all finite
    halves, the midpoints to their successors (ties to even, 65520 -> Inf, 2^-25 -> 0) and the float32 neighbours of the midpoints."""
    t = E.half_boundary_table()
    assert t.dtype == np.float32 and t.size >= 4 * 63488 + 7
    want = torch.from_numpy(t).half().numpy()
    got = E.to_half(t)
    nan = np.isnan(t)
    assert nan.sum() == 1 and np.array_equal(np.isnan(got), nan) and np.array_equal(np.isnan(want), nan)
    assert np.array_equal(got[~nan].view(np.uint16), want[~nan].view(np.uint16))
    assert E.same(got.astype(np.float32), torch.from_numpy(t).half().float().numpy())
    # the table reaches what it is there for: both results of a tie, the overflow boundary, the subnormal range, signed zeros
    h = got.astype(np.float32)
    assert np.isposinf(h[t == np.float32(65520.0)]).all() and (h[t == np.float32(65519.996)] == 65504).all()
    assert (h[t == np.float32(2.0 ** -25)] == 0).all() and (h[t == np.nextafter(np.float32(2.0 ** -25), np.float32(1))] == np.float32(2.0 ** -24)).all()
    assert np.signbit(h[(t == 0) & np.signbit(t)]).all() and not np.signbit(h[(t == 0) & ~np.signbit(t)]).any()
    finite = np.isfinite(t)
    assert (np.isinf(h) & finite).sum() > 4 and ((h == 0) & (t != 0)).sum() > 2


@pytest.mark.parametrize("C,shape,hw", E.GEOMETRIES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("kind", E.KINDS)
def test_half_volume_generators_reach_their_case(orc, C, shape, hw, kind):
    """The feature pairs of the GPU tests give, on the oracle's volume rounded to half: subnormals only / mass ties / +Inf entries
    on both sides of 65504 / all-Inf columns beside finite ones -- from a finite float32 volume."""
    f, m = E.feature_pair(C, shape, hw, kind)
    assert np.isfinite(f).all() and np.isfinite(m).all() and max(np.abs(f).max(), np.abs(m).max()) < 65504
    ref, _ = orc.correlate(f, m, hw)
    p = E.volume_property(kind, ref)
    assert E.property_holds(kind, ref.shape[0], p), p


def _inf_inputs():
    out = []
    for hw in (2, 3):
        for kind in E.INF_KINDS:
            for foreign in (False, True):
                out.append(pytest.param(kind, hw, foreign, id="%s-hw%d-%s" % (kind, hw, "foreign" if foreign else "true")))
    return out


@pytest.mark.parametrize("kind,hw,foreign", _inf_inputs())
def test_coupled_convex_with_infinite_costs_vs_torch(orc, kind, hw, foreign):
    """+Inf costs follow torch.argmin (an all-Inf column, penalised or not, gives index 0): the oracle against the operator written in
    plain torch, with the true argmin and with one foreign displacement for every voxel."""
    ssd = E.inf_volume(kind, hw)
    assert np.isposinf(ssd).any() and not np.isnan(ssd).any() and np.isfinite(ssd).any()
    if kind != "scattered":
        assert np.isposinf(ssd).reshape(ssd.shape[0], -1).all(0).any()
    am = E.foreign_constant_argmin(hw) if foreign else E.first_minimum(ssd)
    mesh = orc.disp_mesh(hw)
    assert E.same(orc.coupled_convex(ssd, am, mesh, hw), E.coupled_convex_torch(ssd, am, mesh))


def test_coupled_convex_lattice_sheet_vs_torch(orc):
    """An all-Inf sheet between uniform winners at (1, 1, 1): the first smoothing step puts the sheet's interior exactly on the lattice
    point (0, 0, 0), and every pass still returns index 0 = (-2, -2, -2) there, as torch.argmin does for a column of equal costs."""
    ssd, am, hw, x0 = E.lattice_sheet_volume()
    mesh = orc.disp_mesh(hw)
    assert np.array_equal(mesh[:, 93], [1, 1, 1]) and np.array_equal(mesh[:, 0], [-2, -2, -2]) and np.array_equal(mesh[:, 62], [0, 0, 0])
    assert (am[:, :, x0] == 0).all() and (np.delete(am, x0, 2) == 93).all()
    u0 = orc.box_zero(mesh[:, am.reshape(-1)].reshape((3,) + am.shape), 3)
    assert E.same(u0[:, 1:-1, 1:-1, x0], np.zeros((3,) + tuple(s - 2 for s in am.shape[:2]), np.float32))
    assert E.same(orc.coupled_convex(ssd, am, mesh, hw), E.coupled_convex_torch(ssd, am, mesh))


@pytest.mark.parametrize("kind", ["overflow", "block"])
def test_coupled_convex_on_overflowing_half_volume_vs_torch(orc, kind):
    C, shape, hw = E.GEOMETRIES[0]
    f, m = E.feature_pair(C, shape, hw, kind)
    vol = E.widen(orc.correlate(f, m, hw)[0])
    assert np.isposinf(vol).any()
    mesh = orc.disp_mesh(hw)
    for am in (E.first_minimum(vol), E.foreign_constant_argmin(hw, shape)):
        assert E.same(orc.coupled_convex(vol, am, mesh, hw), E.coupled_convex_torch(vol, am, mesh))
