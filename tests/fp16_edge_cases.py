"""Inputs of tests/test_gpu_fp16_edges.py and of its oracle-side companion in tests/test_oracle_operators.py: the places where half
precision differs from float32 (rounding boundaries, subnormals, mass ties, overflow to +Inf) and cost volumes with +Inf entries.
Host code only (numpy / torch CPU); every generator is deterministic.  Each `*_property` function returns the figure a test asserts
on the ORACLE's volume before it looks at a kernel, so that a quiet change of a generator cannot empty a case."""
import numpy as np
import torch
import torch.nn.functional as F

INF = np.float32(np.inf)


def same(a, b):
    """Equal shape, equal values, equal NaN pattern, and equal signs wherever the value is not NaN (so -0.0 != +0.0 here)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or not np.array_equal(a, b, equal_nan=True) or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return bool(np.array_equal(np.signbit(a[ok]), np.signbit(b[ok])))


def to_half(x):
    """float32 -> float16, round to nearest even, overflow to +-Inf (numpy; test_half_table_numpy_vs_torch pins it to torch)."""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float32).astype(np.float16)


def widen(x):
    """float32 -> half -> float32: the values a half-precision buffer holds."""
    return to_half(x).astype(np.float32)


# ---- (1) every rounding boundary of float32 -> half --------------------------------------------------------------------------------
def half_boundary_table():
    """float32 values: for every finite half h (63 488 bit patterns) h itself, the midpoint between h and the next half away from zero
    (65520 for h = 65504: the midpoint to 2^16, where round-to-nearest-even overflows), and the two float32 neighbours of that
    midpoint; then NaN, +-Inf, +-0, 65519.996, 65520, 2^-25 (half of the smallest subnormal: ties to zero) and its float32 successor.
    Shuffled with a fixed seed, so that every prefix holds normals, subnormals and both signs."""
    bits = np.arange(1 << 16, dtype=np.uint32)
    bits = bits[(bits & 0x7C00) != 0x7C00].astype(np.uint16)
    assert bits.size == 63488
    h = bits.view(np.float16).astype(np.float64)
    nxt = (bits + np.uint16(1)).view(np.float16).astype(np.float64)
    nxt = np.where(np.isinf(nxt), np.sign(nxt) * 65536.0, nxt)
    mid = ((h + nxt) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (h + nxt) / 2)                  # 12 significant bits: exact in float32
    lo, hi = np.nextafter(mid, -INF), np.nextafter(mid, INF)
    tiny = np.float32(2.0 ** -25)
    extra = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 65519.996, 65520.0, tiny, np.nextafter(tiny, INF)], np.float32)
    t = np.concatenate([h.astype(np.float32), mid, lo, hi, extra])
    return t[np.random.default_rng(16).permutation(t.size)].copy()


# ---- (2) feature pairs whose half cost volume is subnormal / tied / overflowing / all-Inf in places ----------------------------
# (C, coarse shape, hw): one group of 5 with d % 4 = 3; groups 4 + 3 with d % 4 = 2; one displacement, run-time channel loop; the
# cascade channel sum on full quads only; hw > 8 with d % 4 = 1; a y-tiled plane
GEOMETRIES = [(12, (5, 6, 7), 2), (12, (6, 7, 10), 3), (5, (4, 5, 11), 0), (20, (4, 5, 8), 1), (12, (3, 4, 5), 10), (12, (5, 40, 37), 2)]
KINDS = ["sub", "tiny", "overflow", "block"]
# overflow: uniform [0, 1) features times s give costs of C s^2 / 6 on average; s is scaled per C so that the costs straddle 65504
# (181 for C = 12; at C = 20 it would put nearly every entry at +Inf, 140 keeps both sides).  With hw 0 the only displacement's cost
# is a mean over 5^3 voxels and hardly spreads: 5 * 181^2 / 6 = 27 000 never overflows, 360 does on the interior voxels and not on
# the zero-padded border
OVERFLOW_SCALE = {5: 360.0, 12: 181.0, 20: 140.0}
# block: the bright block of the fixed features, [:, z0:z1, y0:y1, x0:x1]; shrunk per geometry until between 10 % and 90 % of the
# columns are all-Inf (the two 3^3 boxes spread a block voxel over a 5^3 neighbourhood; with hw 10 the window exceeds the volume)
BLOCKS = {(5, 6, 7): (slice(None), slice(None), slice(0, 2)), (6, 7, 10): (slice(None), slice(None), slice(0, 3)),
          (4, 5, 11): (slice(None), slice(None), slice(0, 3)), (4, 5, 8): (slice(None), slice(None), slice(0, 2)),
          (3, 4, 5): (slice(0, 1), slice(0, 1), slice(0, 1)), (5, 40, 37): (slice(None), slice(0, 14), slice(None))}


def feature_pair(C, shape, hw, kind):
    rng = np.random.default_rng(1000 * C + 10 * sum(shape) + hw)
    f = rng.random((C,) + shape, dtype=np.float32)
    m = rng.random((C,) + shape, dtype=np.float32)
    if kind == "sub":
        s = 2.0 ** -9
    elif kind == "tiny":
        s = 2.0 ** -12
    elif kind == "overflow":
        s = OVERFLOW_SCALE[C]
    else:
        s = 16.0
    f, m = f * np.float32(s), m * np.float32(s)
    if kind == "block":
        f[(slice(None),) + BLOCKS[shape]] += np.float32(2000.0)
    return f, m


def tied_columns(vol):
    """share of the columns of a (K, ...) volume whose minimum is attained more than once"""
    col = vol.reshape(vol.shape[0], -1)
    return float(((col == col.min(0)).sum(0) > 1).mean())


def volume_property(kind, ref32):
    """The figure the `kind` case is there for, measured on the oracle's float32 volume `ref32` (which must be finite)."""
    assert np.isfinite(ref32).all()
    h = to_half(ref32)
    if kind == "sub":                       # more than 90 % of the stored values are half subnormals (exact zeros do not count)
        return float(((h != 0) & (np.abs(h.astype(np.float32)) < np.float32(2.0 ** -14))).mean())
    if kind == "tiny":                      # more than 50 % of the columns have a tied minimum (where K > 1)
        return tied_columns(h.astype(np.float32))
    if kind == "overflow":                  # between 5 % and 95 % of the entries are +Inf
        return float(np.isposinf(h).mean())
    return float(np.isposinf(h).reshape(h.shape[0], -1).all(0).mean())      # block: all-Inf columns, 10 % .. 90 % of the voxels


def property_holds(kind, K, p):
    if kind == "sub":
        return p > 0.9
    if kind == "tiny":
        return p > 0.5 or K == 1
    if kind == "overflow":
        return 0.05 < p < 0.95
    return 0.1 < p < 0.9


def first_minimum(vol32):
    """torch.argmin(vol, 0) for a volume without NaN: the first index of the column minimum (+Inf columns: index 0)."""
    return vol32.reshape(vol32.shape[0], -1).argmin(0).reshape(vol32.shape[1:]).astype(np.int64)


# ---- (3) cost volumes for the coupled passes ---------------------------------------------------------------------------------------
PRUNING_KINDS = ["foreign_argmin", "flat", "plateaus", "hw0", "zero_columns", "zero_columns_foreign", "signed_zero_columns"]


def pruning_volume(kind, tiny=6e-8):
    """The inputs of test_coupled_convex_pruning_edge_cases (tests/test_gpu_parity.py) with the tiny entry of the zero_columns kinds as
    a parameter (1e-30 there; 6e-8 rounds to the smallest half subnormal): (ssd float32, argmin, hw)."""
    rng = np.random.default_rng(7)
    shape, hw = (6, 8, 12), 3
    if kind == "hw0":
        hw = 0
    K = (2 * hw + 1) ** 3
    if kind == "flat":
        ssd = np.full((K,) + shape, 0.75, np.float32)
    elif kind == "plateaus":
        ssd = (rng.integers(0, 3, (K,) + shape) * 0.5).astype(np.float32)
    else:
        ssd = rng.random((K,) + shape, dtype=np.float32)
    if kind.startswith("zero_columns") or kind == "signed_zero_columns":
        ssd[:, :, :5, :] = 0.0
        ssd[:, 2:4, 5:, 3:7] = 0.0
        ssd[K // 3, 1, 2, :] = tiny
        if kind == "signed_zero_columns":
            ssd[::7, :, 1, :] = -0.0
    am = first_minimum(ssd)
    if kind in ("foreign_argmin", "zero_columns_foreign"):
        am = rng.integers(0, K, shape).astype(np.int64)
    return ssd, am, hw


def worst_case_volume():
    """The input of test_coupled_convex_bounded_worst_case: (ssd float32, argmin, hw)."""
    rng = np.random.default_rng(3)
    shape, hw = (10, 12, 16), 4
    K = (2 * hw + 1) ** 3
    ssd = rng.random((K,) + shape, dtype=np.float32)
    ssd[:, :, :7, :] = 0.25
    return ssd, first_minimum(ssd), hw


INF_KINDS = ["scattered", "columns", "plane", "block"]
INF_SHAPE = (6, 8, 12)


def inf_volume(kind, hw):
    """Uniform [0, 1) costs on INF_SHAPE with +Inf entries: 40 % scattered; isolated all-Inf columns in the interior, on faces and in a
    corner; an all-Inf plane one voxel thick; an all-Inf block three voxels thick.  Every value is a half value already."""
    K = (2 * hw + 1) ** 3
    rng = np.random.default_rng(31 + hw + len(kind))
    ssd = widen(rng.random((K,) + INF_SHAPE, dtype=np.float32))
    if kind == "scattered":
        ssd[rng.random(ssd.shape) < 0.4] = INF
    elif kind == "columns":
        for z, y, x in ((2, 3, 5), (3, 4, 7), (0, 4, 6), (3, 0, 2), (2, 5, 11), (5, 7, 11), (0, 0, 0)):
            ssd[:, z, y, x] = INF
    elif kind == "plane":
        ssd[:, :, 4, :] = INF
    else:
        ssd[:, 1:4, 2:7, 3:9] = INF
    return ssd


def foreign_constant_argmin(hw, shape=INF_SHAPE):
    """One displacement other than mesh[0] for every voxel: the first smoothing step lands exactly on it in the interior."""
    K = (2 * hw + 1) ** 3
    return np.full(shape, K // 2 + 1, np.int64)


def lattice_sheet_volume():
    """hw 2: every finite column has its minimum at displacement (1, 1, 1) (index 93); the plane x = 6 is all +Inf, so its argmin is
    index 0 = (-2, -2, -2).  On the sheet's interior the first smoothing step is (9 (-2) + 18 (+1)) / 27 = 0 in every component: u
    sits exactly on the lattice point (0, 0, 0), whose column entry is +Inf like every other.  -> (ssd, argmin, hw, sheet x)"""
    hw, x0 = 2, 6
    rng = np.random.default_rng(93)
    ssd = widen(np.float32(1) + rng.random((125,) + INF_SHAPE, dtype=np.float32))
    ssd[93] = np.float32(0.125)
    ssd[:, :, :, x0] = INF
    return ssd, first_minimum(ssd), hw, x0


def coupled_convex_torch(ssd, argmin, mesh):
    """The operator in plain torch float32 on the CPU, written from its definition: u = 3^3 box mean (zero padding, / 27) of the
    winners' displacements; then six passes with coef = 0.003 .. 1: winner = argmin_k(cost[k] + coef |mesh[k] - u|^2), u = box mean of
    the new winners' displacements.  ssd (K, h, w, d), argmin (h, w, d), mesh (3, K) -> (3, h, w, d)."""
    cost = torch.from_numpy(np.ascontiguousarray(ssd, np.float32))
    K, h, w, d = cost.shape
    mesh_t = torch.from_numpy(np.ascontiguousarray(mesh, np.float32))

    def box_mean(winners):
        return F.avg_pool3d(mesh_t[:, winners.reshape(-1)].reshape(1, 3, h, w, d), 3, stride=1, padding=1)[0]

    u = box_mean(torch.from_numpy(np.ascontiguousarray(argmin, np.int64)))
    for coef in torch.tensor([0.003, 0.01, 0.03, 0.1, 0.3, 1.0]):
        dist = (mesh_t.reshape(3, K, 1) - u.reshape(3, 1, -1)).pow(2).sum(0)
        u = box_mean(torch.argmin(cost.reshape(K, -1) + coef * dist, 0))
    return u.numpy()
