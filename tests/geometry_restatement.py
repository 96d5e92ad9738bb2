"""numpy float64 restatement of the arithmetic contract of csrc/geometry.hip, the shared geometries of the geometry
tests, and their error bounds.  Test infrastructure only: the product never imports it.

The restatement computes the source coordinate element-wise as written in the contract, ((M0 i + M1 j) + M2 k) + t, and interpolates
with scipy.ndimage.map_coordinates(order=1, mode='nearest') on the clipped coordinate plus the inside rule -- the same eight-tap sum as
the kernels.  The parent's host functions (imageio.resample, rescale_displacement_field, apply_convex_original_moving) compute the
coordinate through a BLAS matrix product instead; tests/test_geometry_reference.py pins the two to each other within the bounds below.
"""
import numpy as np
from scipy.ndimage import map_coordinates

from convexadam_amd.geometry import Grid, field_frame, grid_of, index_map, resampled_grid
from convexadam_amd.imageio import Image

EPS = 2.0 ** -52
NEAR = 1e-9                      # a reference coordinate this close to an inside/outside boundary (and not on it) is left out
MAX_LEFT_OUT = 1e-3              # ... for at most 0.1 % of a case's voxels


def _cs(a):
    """cos, sin with the zeros of a quarter turn exact (cos(pi / 2) is 6e-17 in float64): an image header's direction cosines for such
    a turn are 0 and +-1, and an entry of 6e-17 would put coordinates one ulp beside an inside/outside boundary instead of on it"""
    c, s = np.cos(a), np.sin(a)
    return (0.0 if abs(c) < 1e-15 else c), (0.0 if abs(s) < 1e-15 else s)


def rot_x(a):
    c, s = _cs(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float64)


def rot_y(a):
    c, s = _cs(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float64)


def rot_z(a):
    c, s = _cs(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64)


# (fixed (z, y, x), fixed spacing, fixed direction, moving (z, y, x), moving spacing, moving direction, moving origin); fixed origin 0
CASES = {
    1: ((10, 12, 14), (1.0, 1.0, 2.0), np.eye(3), (8, 20, 18), (0.5, 0.5, 2.5), rot_z(np.pi / 2), (6.0, 0.0, 0.0)),
    2: ((9, 16, 15), (0.8, 0.8, 3.0), rot_z(0.2), (7, 19, 21), (0.6, 0.7, 3.3), rot_z(0.2) @ rot_x(0.15), (1.5, -2.0, 0.7)),
    3: ((6, 30, 28), (0.5, 0.5, 3.6), rot_y(-0.1), (5, 31, 17), (0.9, 0.4, 4.0), rot_z(np.pi / 4), (2.0, 3.0, -1.0)),
}


def smooth_noise(shape, seed, amp=1.0, channels=None):
    """trilinearly up-sampled 3^3 noise of amplitude `amp` on (z, y, x) = shape (float64; `channels` adds a LAST axis)"""
    rng = np.random.default_rng(seed)
    coarse = amp * (2.0 * rng.random((channels or 1, 3, 3, 3)) - 1.0)
    zz, yy, xx = np.meshgrid(*[np.linspace(0.0, 2.0, n) if n > 1 else np.zeros(1) for n in shape], indexing="ij")
    out = np.stack([map_coordinates(c, [zz, yy, xx], order=1, mode="nearest") for c in coarse], -1)
    return out if channels else out[..., 0]


def make_case(n, dtype=np.float64):
    """Case n of the table: fixed and moving Image (smooth noise + white noise), the fixed image at 1 mm by the resample_img rule
    (grid only), and a field of trilinearly up-sampled 3^3 noise of amplitude 2 on that grid, (H, W, D, 3) float64."""
    fs, fsp, fd, ms, msp, md, mo = CASES[n]
    rng = np.random.default_rng(100 + n)
    fixed = Image((smooth_noise(fs, 10 + n) + 0.1 * rng.random(fs)).astype(dtype), fsp, (0.0, 0.0, 0.0), fd.reshape(-1))
    moving = Image((smooth_noise(ms, 20 + n) + 0.1 * rng.random(ms)).astype(dtype), msp, mo, md.reshape(-1))
    gr = resampled_grid(grid_of(fixed), (1.0, 1.0, 1.0))
    field = smooth_noise(gr.size[::-1], 30 + n, amp=2.0, channels=3)
    return fixed, moving, gr, field


def grid_image(grid, array=None):
    """an Image on `grid` (zeros unless `array`): what CopyInformation needs on the host path"""
    arr = np.zeros(tuple(grid.size)[::-1], np.float64) if array is None else array
    return Image(arr, grid.spacing, grid.origin, grid.direction)


def source_coordinates(M, t, out_size):
    """ci (3, nz, ny, nx) in x, y, z order: ((M[a][0] i + M[a][1] j) + M[a][2] k) + t[a], element-wise, i = x, j = y, k = z"""
    nx, ny, nz = out_size
    k, j, i = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    return np.stack([((M[a, 0] * i + M[a, 1] * j) + M[a, 2] * k) + t[a] for a in range(3)], 0)


def interpolate_itk(src, ci, default=0.0):
    """src (z, y, x) any dtype -> float64 values at ci (x, y, z order): inside means -0.5 <= ci <= n - 0.5 on all axes, clamped taps"""
    lim = np.array(src.shape[::-1], np.float64).reshape(3, 1, 1, 1)
    inside = np.all((ci >= -0.5) & (ci <= lim - 0.5), axis=0)
    cic = np.clip(np.where(np.isfinite(ci), ci, 0.0), 0.0, lim - 1.0)
    vals = map_coordinates(np.asarray(src, np.float64), cic[::-1], order=1, mode="nearest")
    return np.where(inside, vals, float(default))


def resample(src, src_grid, out_grid, default=0.0, out_dtype=None):
    """restatement of cvx_resample_linear_f64 -> (array in out_dtype (default: src's), ci)"""
    M, t = index_map(src_grid, out_grid)
    ci = source_coordinates(M, t, grid_of(out_grid).size)
    vals = interpolate_itk(src, ci, default)
    dt = np.dtype(out_dtype or src.dtype)
    return (vals.astype(dt) if np.issubdtype(dt, np.floating) else np.rint(vals).astype(dt)), ci


def carry_field(field, moving_grid, fixed_grid, fixed_resampled_grid):
    """restatement of the carried field of cvx_field_to_grid_f64: field (H, W, D, 3) -> ((mz, my, mx, 3) float64, ci)"""
    M, t = index_map(fixed_resampled_grid, moving_grid)
    ci = source_coordinates(M, t, grid_of(moving_grid).size)
    vz, vy, vx = [interpolate_itk(field[..., c], ci, 0.0) for c in range(3)]
    R, ratio = field_frame(moving_grid, fixed_grid, fixed_resampled_grid)
    s = [((vx * R[0, b] + vy * R[1, b]) + vz * R[2, b]) * ratio[b] for b in range(3)]
    return np.stack([s[2], s[1], s[0]], -1), ci


def warp_coordinates(carried):
    """(z + s_z, y + s_y, x + s_x): the coordinates apply_convex samples the moving image at, (3, mz, my, mx) in z, y, x order"""
    ident = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in carried.shape[:3]], indexing="ij")
    return np.stack([carried[..., a] + ident[a] for a in range(3)], 0)


def warp(moving, carried):
    """restatement of the warped output (float64): map_coordinates(order=1, mode='constant') semantics, 0 unless 0 <= c <= n - 1"""
    c = warp_coordinates(carried)
    lim = np.array(moving.shape, np.float64).reshape(3, 1, 1, 1)
    inside = np.all((c >= 0.0) & (c <= lim - 1.0), axis=0)
    cc = np.clip(np.where(np.isfinite(c), c, 0.0), 0.0, lim - 1.0)
    return np.where(inside, map_coordinates(np.asarray(moving, np.float64), cc, order=1, mode="nearest"), 0.0)


# ---- bounds ------------------------------------------------------------------------------------------------------------------------
def value_range(a):
    a = np.asarray(a, np.float64)
    return float(a.max() - a.min())


def bound_interp(ci, source):
    """B_i = 64 eps max(|ci|, 1) 3 range(source): the two evaluations of ci differ by a few ulps of their magnitude, and the interpolant
    moves at most range(source) per index unit and axis"""
    return 64 * EPS * max(float(np.abs(ci).max()), 1.0) * 3 * value_range(source)


def bound_carried(ci, field, ratio):
    """B_c = (3 B_i + 8 eps max|field|) max(ratio): three components through an orthonormal rotation in another summation order"""
    return (3 * bound_interp(ci, field) + 8 * EPS * float(np.abs(field).max())) * float(np.max(ratio))


def bound_warped(b_c, moving):
    """B_w = 3 B_c range(moving) + 64 eps max|moving|"""
    return 3 * b_c * value_range(moving) + 64 * EPS * float(np.abs(np.asarray(moving, np.float64)).max())


def near_boundary(c, lows, highs):
    """voxels where a coordinate lies within NEAR of an inside/outside boundary without being exactly on it; c (3, ...), per-axis bounds"""
    out = np.zeros(c.shape[1:], bool)
    for a in range(3):
        for b in (lows[a], highs[a]):
            d = np.abs(c[a] - b)
            out |= (d < NEAR) & (d != 0.0)
    return out
