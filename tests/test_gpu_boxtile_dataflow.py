"""The three-box tiles of the exact Adam loop (boxtile.hip) across their hand-over and tap options, bit for bit against the CPU oracle:
  box_tile_sync  1 = the passes hand over through per-row readiness flags in LDS, 0 = two workgroup barriers;
  box_prediv     1 = k_warp_grad stores gU / 27 and the adjoint tiles load divided taps, 0 = the tiles divide every tap they load.
P, m, v, U and grad_out (G of the last iteration) must equal the oracle's for every combination, and no flag wait may have run into its
spin bound (cvx_box_tile_sync_errors).  Run the file once more with the race-stress library (python -m convexadam_amd.csrc.build --jitter,
CONVEXADAM_HIP_LIB=<.../libconvexadam_hip_jitter.so>): the waits then take random detours and must still be bit-identical.

Signed zeros: the adjoint's taps keep the sign of a zero gU (prep and k_warp_grad<.., PREDIV> both store `g == 0 ? g : g / 27`).  The warp
kernel itself never produces -0.0: its sums start from +0.0 and a round-to-nearest sum is -0.0 only when both terms are, so a zero gradient
is +0.0; test_zero_gradient_input runs an input whose gradient is mostly exact zeros."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OPTS = ("box_fwd_tile", "box_bwd_tile", "box_tile_sync", "box_prediv")
SYNC_PREDIV = [(1, 1), (1, 0), (0, 1), (0, 0)]
_REF = {}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from convexadam_amd import _lib
    lib = _lib.lib()
    assert lib.cvx_box_tile_sync_errors(1) >= 0
    return lib


def inputs(shape, C, seed, kind="random"):
    rng = np.random.default_rng(seed)
    F2 = rng.random((C,) + shape, dtype=np.float32)
    if kind == "zero":                      # identical features, zero displacement
        return F2, F2.copy(), np.zeros((3,) + shape, np.float32)
    M2 = rng.random((C,) + shape, dtype=np.float32)
    P0 = (0.7 * rng.standard_normal((3,) + shape)).astype(np.float32)
    return F2, M2, P0


def oracle(orc, key, F2, M2, P0, niter):
    if key not in _REF:
        _REF[key] = orc.adam_run(F2, M2, P0, 1.25, niter, want_grad=True)
    return _REF[key]


def run_and_check(L, orc, key, F2, M2, P0, niter, variant, sync, prediv):
    from convexadam_amd import convex_adam_utils as U
    r = oracle(orc, key, F2, M2, P0, niter)
    old = [L.cvx_get_option(n.encode()) for n in OPTS]
    for n, val in zip(OPTS, (variant, variant, sync, prediv)):
        assert L.cvx_set_option(n.encode(), val) == 0, n
    try:
        Ud, st = U.adam_run(dev(F2)[None], dev(M2)[None], dev(P0)[None], 1.25, niter, return_state=True)
        torch.cuda.synchronize()
    finally:
        for n, val in zip(OPTS, old):
            L.cvx_set_option(n.encode(), val)
    assert L.cvx_box_tile_sync_errors(1) == 0, "a readiness-flag wait ran into its spin bound"
    for name, got in (("U", Ud), ("G", st["G"]), ("P", st["P"]), ("m", st["m"]), ("v", st["v"])):
        a, b = host(got)[0], r[name]
        assert np.array_equal(a, b), "%s differs: %d elements, max |diff| %g" % (name, int((a != b).sum()), float(np.abs(a - b).max()))
        assert np.array_equal(np.signbit(a), np.signbit(b)), name


@pytest.mark.parametrize("sync,prediv", SYNC_PREDIV)
def test_benchmark_grid(L, orc, sync, prediv):
    """80 x 96 x 112 with 12 channels, the benchmark's control grid: the automatic choice (12 x 16 x 56 tiles, default segments)."""
    shape = (80, 96, 112)
    F2, M2, P0 = inputs(shape, 12, 7)
    run_and_check(L, orc, ("bench",), F2, M2, P0, 2, -1, sync, prediv)


# ragged tiles in all three directions (d % 4 == 0), rows longer than the marching kernel's 126 voxels, grids smaller than one tile
SHAPES = [(25, 17, 60), (30, 37, 116), (14, 20, 132), (13, 9, 252), (5, 3, 4), (2, 2, 8), (11, 15, 52)]
# both tile kinds with their default segments, one segment per row in every pass, and planes / 2 segments (16 / 14 / 12 planes)
VARIANTS = [2000, 1000, 2111, 2876, 1111, 1876, 2999]


@pytest.mark.parametrize("sync,prediv", SYNC_PREDIV)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_and_segments(L, orc, shape, variant, sync, prediv):
    F2, M2, P0 = inputs(shape, 5, sum(shape))
    run_and_check(L, orc, ("shape", shape), F2, M2, P0, 3, variant, sync, prediv)


@pytest.mark.parametrize("sync,prediv", SYNC_PREDIV)
def test_zero_gradient_input(L, orc, sync, prediv):
    """Identical features and a zero field: a gradient made mostly of exact zeros, so most taps take the `g == 0` branch."""
    shape = (24, 20, 60)
    F2, M2, P0 = inputs(shape, 4, 5, kind="zero")
    run_and_check(L, orc, ("zero",), F2, M2, P0, 3, 2000, sync, prediv)


def test_options_default_and_roundtrip(L):
    assert L.cvx_get_option(b"box_tile_sync") in (0, 1) and L.cvx_get_option(b"box_prediv") in (0, 1)
    assert L.cvx_get_option(b"tile_census_ptr") == 0
