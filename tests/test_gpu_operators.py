"""GPU tests of the generic volume operators of pool.hip at every kernel branch their launchers choose (run on the MI355X box with
`-m gpu`): the forward box filter (k_box_walk in all six instances and the k_box_zero fallback), the sweep's smoothers forward and
adjoint (k_gauss1d, box chains) and inside the exact Adam loop, grid_sample at the sampler's edges, and the masked-feature and
label-feature helpers.  Every comparison is bit-exact against the CPU oracle and, where torch defines the operator on the CPU, against
torch too (tests/test_oracle_operators.py pins the oracle to torch at the small edge shapes)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.isnan(a), np.isnan(b))


def cdiv(a, b):
    return -(-a // b)


@pytest.fixture(scope="module")
def U():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from convexadam_amd import convex_adam_utils
    return convex_adam_utils


@pytest.fixture(scope="module")
def HU():
    from convexadam_amd import convexAdam_hyper_util
    return convexAdam_hyper_util


@pytest.fixture(scope="module")
def L():
    from convexadam_amd import _lib
    return _lib.lib()


class option:
    """Sets a library option for the duration of a with-block and restores the previous value."""

    def __init__(self, L, name, value):
        self.L, self.name, self.value = L, name.encode(), value

    def __enter__(self):
        self.old = self.L.cvx_get_option(self.name)
        assert self.L.cvx_set_option(self.name, self.value) == 0

    def __exit__(self, *exc):
        self.L.cvx_set_option(self.name, self.old)


# ---- (a) the forward box filter at every launch choice --------------------------------------------------------------------------
def walk_choice(C, H, W, D, k, aligned=True, box_walk=1):
    """Restates the forward branch of launch_box_zero and launch_box_walk_r (convexadam_amd/csrc/pool.hip, the two functions after
    k_box_walk): None when k_box_zero<false> runs, else (R, CPT, L) of the k_box_walk<R, CPT> launch with segments of L planes."""
    if not (aligned and D % 4 == 0 and box_walk != 0):          # (in != out: always, the callers ping-pong)
        return None
    if k not in (3, 5, 7):
        return None
    R = k // 2
    quads4 = C * W * (D // 4)
    cpt2 = quads4 * H < (1 << 22)
    cpt = 2 if cpt2 else 4
    nq = D // cpt
    items = C * W * nq
    L = 16
    while L > 4 and items * cdiv(H, L) < 256 * 256 * 6:
        L -= 4
    return R, cpt, L


FULL = (3, 160, 192, 224)           # the benchmark resolution: the pipeline's final smoothing (three passes of k = 3 or 5)

# (shape, k, passes, how): how = "" (random input with non-finite values), "zeros", "misaligned" (input and output 4 bytes off a
# 16-byte boundary), "box_walk=0" (the option that disables the walk)
BOX_CASES = [
    # two columns per thread: partial last segment, full last segment (H % L == 0), H < L, H = 1, rows of > 64 quads, W = 1, W < R
    ((3, 10, 11, 12), 3, (1, 2, 3), ""), ((3, 10, 11, 12), 5, (1, 2, 3), ""), ((3, 10, 11, 12), 7, (1, 2, 3), ""),
    ((2, 8, 5, 8), 3, (1, 2), ""), ((2, 8, 5, 8), 5, (1, 3), ""), ((2, 8, 5, 8), 7, (1, 2), ""),
    ((2, 3, 7, 12), 5, (1, 3), ""), ((1, 1, 6, 16), 3, (1, 2), ""), ((1, 1, 6, 16), 7, (1,), ""),
    ((2, 6, 5, 260), 3, (1, 2, 3), ""), ((2, 6, 5, 260), 5, (1, 2), ""), ((2, 6, 5, 260), 7, (1,), ""),
    ((3, 5, 1, 8), 3, (1, 2), ""), ((3, 5, 1, 8), 7, (1,), ""), ((2, 7, 2, 12), 7, (1, 3), ""), ((2, 7, 2, 12), 5, (2,), ""),
    ((1, 9, 3, 4), 5, (1, 3), ""), ((4, 21, 9, 36), 3, (3,), ""),
    ((3, 10, 11, 12), 3, (2,), "zeros"), ((2, 6, 5, 260), 7, (1,), "zeros"),
    # four columns per thread (C * W * D/4 * H >= 2^22): full last segment with rows of 128 quads, partial last segment with k = 7,
    # rows of a single quad, and the benchmark resolution
    ((1, 128, 256, 512), 3, (1,), ""), ((1, 128, 256, 512), 5, (1,), ""), ((1, 132, 256, 512), 7, (1,), ""),
    ((16, 256, 1024, 4), 3, (1,), ""), ((16, 256, 1024, 4), 5, (1,), ""),
    (FULL, 3, (3,), ""), (FULL, 5, (3,), ""),
    # k_box_zero<false>: D % 4 != 0, misaligned pointers, k outside {3, 5, 7}, the option off
    ((3, 10, 11, 13), 3, (1, 3), ""), ((3, 10, 11, 13), 5, (2,), ""), ((2, 6, 5, 258), 7, (1,), ""),
    ((3, 10, 11, 12), 3, (1, 2, 3), "misaligned"), ((3, 10, 11, 12), 5, (2,), "misaligned"), ((2, 6, 5, 260), 7, (1,), "misaligned"),
    ((3, 10, 11, 12), 1, (1, 2), ""), ((3, 10, 11, 12), 9, (1, 2), ""), ((2, 4, 3, 8), 9, (1,), ""),
    ((3, 10, 11, 12), 3, (1, 3), "box_walk=0"), ((2, 6, 5, 260), 7, (2,), "box_walk=0"),
]


def _box_params():
    out = []
    for shape, k, passes, how in BOX_CASES:
        for p in passes:
            marks = [pytest.mark.timeout(900)] if shape == FULL else []
            out.append(pytest.param(shape, k, p, how, marks=marks, id="%s-k%d-p%d%s" % ("x".join(map(str, shape)), k, p, "-" + how if how else "")))
    return out


def _choice(shape, k, how):
    return walk_choice(*shape, k, aligned=how != "misaligned", box_walk=0 if how == "box_walk=0" else 1)


def test_box_cases_cover_every_launch_choice():
    """The parametrisation below reaches all six k_box_walk instances, full and partial last z segments for both column counts,
    H < L and H = 1, rows of one quad and rows longer than a wavefront of quads (lanes 0 and 63 mid-row), W = 1 and W < R, and
    k_box_zero<false> for each reason the walk is not taken."""
    inst, seg, short, nq, narrow, fallback = set(), set(), set(), set(), set(), set()
    for shape, k, passes, how in BOX_CASES:
        C_, H, W, D = shape
        ch = _choice(shape, k, how)
        if ch is None:
            fallback.add("D%4" if D % 4 else "misaligned" if how == "misaligned" else "box_walk=0" if how == "box_walk=0" else "k=%d" % k)
            continue
        R, cpt, Ls = ch
        inst.add((R, cpt))
        if H > Ls:
            seg.add((cpt, "full" if H % Ls == 0 else "partial"))
        if H < Ls:
            short.add("H<L")
        if H == 1:
            short.add("H=1")
        nq.add("nq=1" if D // cpt == 1 else "nq>64" if D // cpt > 64 else "")
        if W == 1:
            narrow.add("W=1")
        if W < R:
            narrow.add("W<R")
    assert inst == {(r, c) for r in (1, 2, 3) for c in (2, 4)}
    assert seg == {(c, s) for c in (2, 4) for s in ("full", "partial")}
    assert short == {"H<L", "H=1"}
    assert {"nq=1", "nq>64"} <= nq
    assert narrow == {"W=1", "W<R"}
    assert fallback == {"D%4", "misaligned", "k=1", "k=9", "box_walk=0"}
    assert _choice(FULL, 3, "") == (1, 4, 12) and _choice(FULL, 5, "") == (2, 4, 12)         # the pipeline's final smoothing


def spiked(shape, seed):
    """Standard normals with +inf and -inf in channel 0, NaN and -0.0 in the last channel, on the borders and inside (more of them in
    large volumes)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape, dtype=np.float32)
    c0, cl = x[0], x[-1]
    c0[0, 0, 0] = np.inf
    c0[-1, -1, -1] = -np.inf
    c0[0, -1, c0.shape[2] // 2] = np.inf
    cl[tuple(s // 2 for s in cl.shape)] = np.nan
    cl[-1, 0, 0] = -0.0
    extra = max(1, c0.size // 2_000_000)
    for c, v in ((c0, np.inf), (c0, -np.inf), (cl, np.nan), (cl, -0.0), (c0, -0.0)):
        c.reshape(-1)[rng.integers(0, c.size, extra)] = v
    return x


def box_smooth_misaligned(L, x, k, passes):
    """cvx_box_smooth_f32 with the input and the output 4 bytes past a 16-byte boundary inside larger buffers (the walk needs both
    16-byte aligned); the guard elements around the output must stay untouched."""
    from convexadam_amd import _lib
    C_, H, W, D = x.shape
    n = x.size
    src = torch.zeros(n + 8, dtype=torch.float32, device=DEV)
    src[1:1 + n] = dev(x).reshape(-1)
    dst = torch.full((n + 8,), 7.0, dtype=torch.float32, device=DEV)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    nws = L.cvx_box_smooth_workspace_bytes(C_, H, W, D, passes)
    ws = torch.empty(max(nws, 256), dtype=torch.uint8, device=DEV)
    _lib.check(L.cvx_box_smooth_f32(C.c_void_p(src.data_ptr() + 4), C_, H, W, D, k, passes, C.c_void_p(dst.data_ptr() + 4),
                                    C.c_void_p(ws.data_ptr()), nws, _lib.stream_ptr(DEV)))
    out = host(dst)
    assert out[0] == 7.0 and np.all(out[1 + n:] == 7.0)
    return out[1:1 + n].reshape(x.shape)


@pytest.mark.parametrize("shape,k,passes,how", _box_params())
def test_box_smooth_every_launch_choice(U, L, orc, shape, k, passes, how):
    """`passes` x avg_pool3d(k, stride 1, padding k // 2): bit-identical to the oracle's chain of box_zero and, where every extent is
    >= k (avg_pool3d refuses smaller ones), to torch's CPU avg_pool3d; non-finite values propagate exactly (+inf / 27 is +inf)."""
    x = np.zeros(shape, np.float32) if how == "zeros" else spiked(shape, sum(shape) * 16 + k)
    if how == "misaligned":
        got = box_smooth_misaligned(L, x, k, passes)
    elif how == "box_walk=0":
        with option(L, "box_walk", 0):
            got = host(U.box_smooth(dev(x)[None], k, passes))[0]
    else:
        got = host(U.box_smooth(dev(x)[None], k, passes))[0]
    ref = x
    for _ in range(passes):
        ref = orc.box_zero(ref, k)
    assert same(got, ref), "max |diff| %g, NaN %d vs %d" % (np.nanmax(np.abs(got - ref)), np.isnan(got).sum(), np.isnan(ref).sum())
    if min(shape[1:]) >= k:
        t = torch.from_numpy(x)[None]
        for _ in range(passes):
            t = F.avg_pool3d(t, k, stride=1, padding=k // 2)
        assert same(got, t[0].numpy())


def test_box_walk_keeps_infinite_sums_infinite(U, L, orc):
    """Regression: the walk divided its sums by k^3 with div_exact, which turns +-inf into NaN (fma(-27, inf, inf)); avg_pool3d and
    k_box_zero give +-inf.  One +inf and one -inf voxel, far apart, in every launch variant of the walk."""
    for shape, k in (((2, 10, 11, 12), 3), ((2, 10, 11, 12), 5), ((2, 10, 11, 12), 7), ((1, 128, 256, 512), 3), ((1, 132, 256, 512), 7)):
        assert _choice(shape, k, "") is not None
        x = np.zeros(shape, np.float32)
        x[0, 1, 2, 4] = np.inf
        x[-1, -2, -3, -5] = -np.inf
        got = host(U.box_smooth(dev(x)[None], k, 1))[0]
        ref = orc.box_zero(x, k)
        assert same(got, ref) and not np.isnan(got).any(), (shape, k)
        assert np.isposinf(got).sum() == np.isposinf(ref).sum() > 0 and np.isneginf(got).sum() == np.isneginf(ref).sum() > 0


# ---- (b) the sweep's smoothers, forward and adjoint, and inside the exact Adam loop --------------------------------------------
SMOOTHERS = {"gauss07": ("g", 0.7), "gauss10": ("g", 1.0), "kov13": ("k", 1.3), "kov16": ("k", 1.6), "kov19": ("k", 1.9),
             "kov22": ("k", 2.2), "kov25": ("k", 2.5), "kov28": ("k", 2.8)}


def make_pair(HU, orc, name):
    kind, sigma = SMOOTHERS[name]
    if kind == "g":
        mod = HU.GaussianSmoothing(sigma)
        return mod, orc.make_smoother(gauss_w=np.array(list(mod.spec.gauss_w), np.float32))
    mod = HU.kovesi_spline(sigma, 4)
    return mod, orc.make_smoother(mod.sizes)


# C = 1 (the unfused Gaussian adjoint), 2, 3, 5; each axis in turn of length 1 .. 5; a line of 301 voxels; D % 4 == 0 (the box
# chains on the walk) and D % 4 != 0
SMOOTH_SHAPES = [(1, 1, 1, 1), (1, 6, 7, 9), (2, 6, 7, 9), (3, 6, 7, 9), (5, 6, 7, 9),
                 (1, 1, 7, 9), (2, 2, 7, 9), (3, 3, 7, 9), (1, 4, 7, 9), (5, 5, 7, 9),
                 (2, 6, 1, 9), (1, 6, 2, 9), (3, 6, 3, 9), (2, 6, 4, 9), (1, 6, 5, 9),
                 (3, 6, 7, 1), (1, 6, 7, 2), (2, 6, 7, 3), (5, 6, 7, 4), (1, 6, 7, 5),
                 (1, 2, 3, 301), (2, 301, 2, 3),
                 (3, 8, 6, 12), (1, 5, 7, 16), (2, 9, 5, 132), (3, 20, 24, 28), (1, 13, 11, 10)]


def test_smoother_shapes_reach_the_walk_and_the_fallback():
    walk = [s for s in SMOOTH_SHAPES if walk_choice(*s, 3) is not None and walk_choice(*s, 5) is not None]
    assert len(walk) >= 4 and any(s[3] % 4 for s in SMOOTH_SHAPES if min(s[1:]) >= 5)
    assert {s[0] for s in SMOOTH_SHAPES} >= {1, 2, 3, 5}
    for a in range(3):
        assert {s[1 + a] for s in SMOOTH_SHAPES} >= {1, 2, 3, 4, 5}
    assert max(max(s[1:]) for s in SMOOTH_SHAPES) >= 300


@pytest.mark.parametrize("name", list(SMOOTHERS))
@pytest.mark.parametrize("shape", SMOOTH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sweep_smoother_forward_and_adjoint(HU, orc, name, shape):
    mod, sm = make_pair(HU, orc, name)
    rng = np.random.default_rng(sum(shape) * 7 + len(name))
    x = rng.standard_normal(shape, dtype=np.float32)
    go = rng.standard_normal(shape, dtype=np.float32)
    xd = dev(x)[None].requires_grad_(True)
    y = mod(xd)
    y.backward(dev(go)[None])
    assert same(host(y)[0], orc.smooth(x, sm)), (name, shape)
    assert same(host(xd.grad)[0], orc.smooth(go, sm, backward=True)), (name, shape)


@pytest.mark.parametrize("name", ["gauss10", "kov19", "kov28"])
@pytest.mark.parametrize("grid", [(20, 24, 28), (80, 96, 112)], ids=lambda s: "x".join(map(str, s)))
def test_exact_adam_loop_with_sweep_smoother_on_walk_grids(U, HU, orc, name, grid):
    """The exact Adam loop with a sweep smoother on control grids whose rows are multiples of 4 voxels, so that the box chains run on
    the walk; (80, 96, 112) is the sweep's own grid at grid_sp_adam = 2 for a 160 x 192 x 224 pair.  U, G, P, m, v bit for bit."""
    mod, sm = make_pair(HU, orc, name)
    if SMOOTHERS[name][0] == "k":
        assert all(walk_choice(3, *grid, k) is not None for k in mod.sizes)
    rng = np.random.default_rng(sum(grid) + len(name))
    C_ = 12
    F2 = rng.random((C_,) + grid, dtype=np.float32)
    M2 = rng.random((C_,) + grid, dtype=np.float32)
    P0 = (0.7 * rng.standard_normal((3,) + grid)).astype(np.float32)
    niter = 3 if grid == (20, 24, 28) else 2
    Ud, st = U.adam_run(dev(F2)[None], dev(M2)[None], dev(P0)[None], 0.8, niter, smoother=mod, return_state=True)
    r = orc.adam_run(F2, M2, P0, 0.8, niter, want_grad=True, smoother=sm)
    assert np.array_equal(host(Ud)[0], r["U"])
    assert np.array_equal(host(st["G"])[0], r["G"])
    assert np.array_equal(host(st["P"])[0], r["P"])
    assert np.array_equal(host(st["m"])[0], r["m"]) and np.array_equal(host(st["v"])[0], r["v"])


# ---- (c) grid_sample ----------------------------------------------------------------------------------------------------------
def special_coords(S):
    """Normalised coordinates along an axis of S voxels that hit the sampler's edges: voxel centres, +-1 and just outside, +-0,
    non-finite values, and magnitudes around the +-1e9 clamp of tri_setup (in voxel units) and beyond."""
    on = [(2 * i + 1) / S - 1 for i in (0, S // 2, S - 1)]
    near_clamp = [2e9 / S, -2e9 / S, 2.000001e9 / S, -2.000001e9 / S, 1.9999e9 / S, 1e9, -1e9, 1.00001e9, -1.00001e9]
    return np.array(on + [1.0, -1.0, 1 + 1 / S, -1 - 1 / S, 0.0, -0.0, np.nan, np.inf, -np.inf, 3e9, -3e9] + near_clamp, np.float32)


def special_grid(h, w, d, out, seed):
    rng = np.random.default_rng(seed)
    n = int(np.prod(out))
    g = (rng.random((n, 3)) * 2.4 - 1.2).astype(np.float32)
    for a, S in enumerate((d, w, h)):                                   # grid = (x, y, z) <-> (d, w, h)
        sp = special_coords(S)
        pick = rng.random(n) < 0.4
        g[pick, a] = sp[rng.integers(0, sp.size, int(pick.sum()))]
    g[0] = np.float32(-0.0)
    if n > 2:
        g[1] = 1.0
        g[2] = -1.0
    return g.reshape(tuple(out) + (3,))


def grid_sample_torch(vol, grid):
    return F.grid_sample(torch.from_numpy(vol)[None], torch.from_numpy(grid)[None], mode="bilinear", padding_mode="zeros",
                         align_corners=False)[0].numpy()


@pytest.mark.parametrize("C_,vshape,out", [(1, (1, 1, 1), (1, 1, 1)), (3, (1, 5, 7), (3, 5, 17)), (2, (6, 1, 5), (1, 1, 257)),
                                            (12, (4, 6, 1), (5, 3, 17)), (5, (4, 8, 16), (60, 70, 72)), (1, (9, 10, 11), (1, 1, 257)),
                                            (12, (5, 6, 7), (1, 1, 255)), (3, (1, 1, 9), (2, 3, 43)), (2, (16, 8, 4), (3, 5, 17))])
def test_grid_sample_edges_vs_oracle_and_torch(U, orc, C_, vshape, out):
    """Channel counts 1 .. 12, axes of length 1, output counts of 1, 255, 257 and ~300 k, and edge coordinates: bit-identical to
    the oracle and to torch's CPU grid_sample, also with +inf / NaN volume values."""
    rng = np.random.default_rng(C_ * 100 + sum(vshape))
    vol = rng.standard_normal((C_,) + vshape, dtype=np.float32)
    grid = special_grid(*vshape, out, C_ + sum(out))
    for _ in range(2):
        got = host(U.grid_sample(dev(vol)[None], dev(grid)[None]))[0]
        assert same(got, orc.grid_sample(vol, grid))
        assert same(got, grid_sample_torch(vol, grid))
        vol.reshape(C_, -1)[:, rng.integers(0, vol[0].size, 2)] = np.inf
        vol.reshape(C_, -1)[:, -1] = np.nan


def test_grid_sample_lattice_centres_with_non_finite_neighbours(U, orc):
    """Coordinates exactly on voxel centres: the upper corner along each axis has weight 0, and +inf / NaN there must still make the
    sample NaN (0 * inf), as in ATen; the tap-selecting form of tri_sample may not drop it."""
    h, w, d = 4, 8, 16
    vol = np.random.default_rng(5).standard_normal((3, h, w, d), dtype=np.float32)
    vol[0, 1, 2, 4] = np.inf
    vol[1, 2, 5, 9] = np.nan
    vol[2, 3, 7, 15] = -np.inf                                          # on the far corner: its 0-weight neighbours are outside
    zz, yy, xx = np.meshgrid(np.arange(h), np.arange(w), np.arange(d), indexing="ij")
    grid = np.stack([(2 * xx + 1) / d - 1, (2 * yy + 1) / w - 1, (2 * zz + 1) / h - 1], -1).astype(np.float32)
    got = host(U.grid_sample(dev(vol)[None], dev(grid)[None]))[0]
    assert same(got, orc.grid_sample(vol, grid))
    assert same(got, grid_sample_torch(vol, grid))
    assert got[0, 1, 2, 4] == np.inf and np.isnan(got[0, 0, 1, 3]) and np.isnan(got[1, 1, 4, 8]) and got[2, 3, 7, 15] == -np.inf


# ---- (d) masked-feature helpers and label features ------------------------------------------------------------------------------
def _masks(shape, rng):
    H, W, D = shape
    full = np.ones(shape, np.float32)
    rand = (rng.random(shape) < 0.75).astype(np.float32)
    border = np.zeros(shape, np.float32)                                # touches all six faces
    border[0], border[-1], border[:, 0], border[:, -1], border[:, :, 0], border[:, :, -1] = 1, 1, 1, 1, 1, 1
    border[H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1, :] = 1
    return [full, rand, border]


@pytest.mark.parametrize("shape", [(2, 8, 6), (6, 2, 10), (8, 10, 2), (4, 6, 8), (10, 12, 14)])
def test_replicate_fill_vs_oracle(orc, shape):
    from convexadam_amd import convex_adam_MIND as M
    rng = np.random.default_rng(sum(shape))
    img = rng.standard_normal(shape, dtype=np.float32)
    masks = _masks(shape, rng)
    if min(shape) >= 4:                                                 # a 3^3 block at an even corner: its erosion leaves one half-resolution voxel
        one = np.zeros(shape, np.float32)
        one[1:4, 1:4, 1:4] = 1
        assert (orc.box3_replicate(one) > np.float32(0.9))[::2, ::2, ::2].sum() == 1
        masks.append(one)
    ran = 0
    for mask in masks:
        if not (orc.box3_replicate(mask) > np.float32(0.9))[::2, ::2, ::2].any():
            continue                                                    # (an empty eroded mask is an error, tested elsewhere)
        got = host(M._replicate_fill(torch.from_numpy(img), torch.from_numpy(mask), torch.device(DEV)))[0, 0]
        want, _ = orc.replicate_fill(img, mask)
        assert np.array_equal(got, want)
        ran += 1
    assert ran >= 2


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 3, 5), (3, 1, 7), (5, 7, 1), (2, 1, 3), (9, 11, 13), (3, 3, 3)])
def test_mask_erode_vs_torch(L, orc, shape):
    """(ReplicationPad3d(1) + avg_pool3d(3))(mask) > 0.9 at odd and one-voxel extents, where the clamp folds several taps onto one
    voxel: against the same composition in torch on the CPU and the oracle's box3_replicate."""
    from convexadam_amd import _lib
    rng = np.random.default_rng(sum(shape))
    for mask in [np.ones(shape, np.float32), (rng.random(shape) < 0.8).astype(np.float32), (rng.random(shape) < 0.95).astype(np.float32)]:
        m = dev(mask)
        out = torch.full((mask.size + 2,), 7.0, dtype=torch.float32, device=DEV)
        _lib.check(L.cvx_mask_erode_f32(C.c_void_p(m.data_ptr()), *shape, 0.9, C.c_void_p(out.data_ptr() + 4), _lib.stream_ptr(DEV)))
        got = host(out)
        assert got[0] == 7.0 and got[-1] == 7.0
        got = got[1:-1].reshape(shape)
        t = F.avg_pool3d(torch.nn.ReplicationPad3d(1)(torch.from_numpy(mask)[None, None]), 3, stride=1)[0, 0]
        want = (t > 0.9).to(torch.float32).numpy()
        assert np.array_equal(got, want)
        assert np.array_equal(got, (orc.box3_replicate(mask) > np.float32(0.9)).astype(np.float32))


@pytest.mark.parametrize("case", ["40_labels", "max_label_300", "one_map_only"])
def test_label_features_many_and_large_labels(orc, case):
    """>= 32 present labels (the weights' Sleef block of 32 elements), max_label around 300 (several strides of the histogram's LDS
    clear loop) with gaps, labels present in only one of the two maps."""
    from convexadam_amd import convex_adam_nnUNet as N
    rng = np.random.default_rng(len(case))
    shape = (12, 14, 16)
    if case == "40_labels":
        labs = np.arange(41)
        lf, lm = rng.choice(labs, shape), rng.choice(labs, shape)
    elif case == "max_label_300":
        labs = np.array([0, 1, 2, 5, 17, 64, 128, 255, 256, 257, 299, 300, 301] + list(range(100, 140, 3)))
        lf, lm = rng.choice(labs, shape), rng.choice(labs, shape)
        lf[0, 0, :3] = [303, 302, 280]                                  # only in the fixed map
        lm[-1, -1, -2:] = [290, 304]                                    # only in the moving map
    else:
        lf = rng.choice(np.arange(0, 70, 2), shape)                     # even labels in one map, odd in the other
        lm = rng.choice(np.arange(1, 71, 2), shape)
    lf, lm = lf.astype(np.float32), lm.astype(np.float32)
    ff, fm = N.extract_features(dev(lf), dev(lm), device=DEV)
    rf, rm, pres = orc.label_features(lf, lm, 10.0)
    assert len(pres) >= 32 and len(pres) == len(set(np.unique(lf)) | set(np.unique(lm)))
    assert np.array_equal(host(ff)[0], rf) and np.array_equal(host(fm)[0], rm)
