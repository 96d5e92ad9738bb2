"""numpy restatement of cvx_crop_field_half_f32 (include/convexadam_hip.h), element-wise in the contract's operation order:
float64 multiplies, adds and divisions one at a time (numpy fuses nothing), one rounding to float32, then ATen's float32 halving.  The
kernel is held to it bit for bit (tests/test_gpu_cropfield.py), and it to the reference's own output within a derived bound
(tests/test_cropfield_reference.py).  A helper module, not a test file.

Fields are numpy float32 arrays (H, W, D, 3) here, whatever layout the kernel reads them in."""
import numpy as np

F32, F64 = np.float32, np.float64
U32 = 2.0 ** -24          # unit roundoff of float32


def halve(d):
    """F.interpolate(scale_factor=0.5, mode='trilinear', align_corners=False) of float32 (..., S0, S1, S2): per axis the taps 2 o and
    min(2 o + 1, S - 1), weights 0.5 and 0.5, combined in float32 last axis first (ATen's order)."""
    d = np.asarray(d)
    assert d.dtype == F32
    h = F32(0.5)
    for axis in (-1, -2, -3):
        S = d.shape[axis]
        o = np.arange(S // 2)
        a, b = np.take(d, 2 * o, axis=axis), np.take(d, np.minimum(2 * o + 1, S - 1), axis=axis)
        d = a * h + b * h
        assert d.dtype == F32
    return d


def axis_taps(geom, a, S, n):
    """for every source index x = 0 .. S - 1 of axis a: x, g, the two clamped taps and their weights (float64 / int arrays of length S)"""
    g3 = np.asarray(geom, F64).reshape(9, 3)
    x = np.arange(S, dtype=F64)
    with np.errstate(invalid="ignore", over="ignore"):
        g = g3[0, a] * (x - g3[1, a])
        c = np.where(g > 0.0, g, 0.0)
        c = np.where(c > F64(n - 1), F64(n - 1), c)
    f = np.floor(c)
    t = c - f
    i0 = f.astype(np.int64)
    i1 = np.minimum(i0 + 1, n - 1)
    return x, g, (i0, i1), (1.0 - t, 1.0 - (1.0 - t))


def chain(field, geom, full, voxels=False):
    """d = m - x on the original fixed grid before the flips: float64 (S0, S1, S2, 3)"""
    field = np.asarray(field)
    assert field.dtype == F32 and field.ndim == 4 and field.shape[3] == 3
    n = field.shape[:3]
    g3 = np.asarray(geom, F64).reshape(9, 3)
    nfsp, nmsp, ms, mlo, pfs, pms = g3[2], g3[3], g3[4], g3[5], g3[6], g3[7]
    ax = [axis_taps(geom, a, full[a], n[a]) for a in range(3)]
    shape = [(-1, 1, 1), (1, -1, 1), (1, 1, -1)]
    d = np.empty(tuple(full) + (3,), F64)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            p = np.zeros(tuple(full), F64)
            for i in range(2):
                for j in range(2):
                    for k in range(2):
                        y = [ax[0][2][i].reshape(shape[0]), ax[1][2][j].reshape(shape[1]), ax[2][2][k].reshape(shape[2])]
                        v = field[y[0], y[1], y[2], a]
                        if voxels:                                 # the reference's float32 disp_p at the tap, every operation rounded to float32
                            ya = y[a].astype(F32)
                            v = (ya + v) * F32(pms[a]) - ya * F32(pfs[a])
                            assert v.dtype == F32
                        v = v.astype(F64)
                        p = p + ((v * ax[0][3][i].reshape(shape[0])) * ax[1][3][j].reshape(shape[1])) * ax[2][3][k].reshape(shape[2])
            g, x = ax[a][1].reshape(shape[a]), ax[a][0].reshape(shape[a])
            m = ((g * nfsp[a] + p) / nmsp[a]) / ms[a] + mlo[a]
            d[..., a] = m - x
    return d


def flip_field(d, flip_mask):
    """output index i along a flipped axis reads source index S - 1 - i, and that axis's component changes sign: (S0, S1, S2, 3)"""
    d = np.array(d)
    for a in range(3):
        if (flip_mask >> a) & 1:
            d = np.flip(d, axis=a).copy()
            d[..., a] = -d[..., a]
    return d


def crop_field_half(field, geom, full, flip_mask=3, voxels=False, identity=False, out_dtype=F32):
    """the restatement of one launch: (3, S0 // 2, S1 // 2, S2 // 2) in out_dtype (np.float32 or np.float16)"""
    if identity:
        field = np.asarray(field)
        assert field.dtype == F32 and tuple(field.shape[:3]) == tuple(full)
        d = field
    else:
        d = chain(field, geom, full, voxels)
    with np.errstate(over="ignore", invalid="ignore"):
        d32 = flip_field(d, flip_mask).astype(F32)
        out = halve(np.moveaxis(d32, 3, 0))
        return np.ascontiguousarray(out if out_dtype == F32 else out.astype(np.float16))


def physical(disp, pre_fix_spacing, pre_mov_spacing):
    """task1:390-397 in float32, as the reference (and convexadam_amd.cropfield.physical_displacement) forms it: (H, W, D, 3) voxel field
    -> (H, W, D, 3) millimetres"""
    disp = np.asarray(disp, F32)
    grid = np.stack(np.meshgrid(*[np.arange(n, dtype=F32) for n in disp.shape[:3]], indexing="ij"), axis=3)
    return (grid + disp) * np.asarray(pre_mov_spacing, F32) - grid * np.asarray(pre_fix_spacing, F32)


def ulp16(r):
    """spacing of float16 at |r| (2^-24 below the smallest normal)"""
    a = np.abs(np.asarray(r, F64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (e - 10)


def reference_bound(field_p, geom, full):
    """E (3,): a bound on |reference's float32 value before its float16 cast - restatement| for a physical field (H, W, D, 3), per
    component, from the magnitudes of the reference's float32 intermediates (u = 2^-24; derivation: DESIGN.md 27):
        dg  = 8 u (|fs| X + |fs lo|)                        the inverted affine's two entries (3 u each) and the matmul's roundings
        ds  = dg + u (4 G + n)                               normalising by n - 1 to [-1, 1] and back inside grid_sample
        dp  = sum_b L_b ds_b + 12 u P                        the interpolant moves by at most its steepest tap difference per voxel of
                                                             coordinate error; its own weights, products and 7 additions round 12 times
        dm  = (((dg + u G) |nfsp| + dp + u Q) / |nmsp| + u Q / |nmsp|) / |ms| + 2 u Q / |nmsp ms| + u M
        E   = dm + u (M + X) + 7 u (M + X)                   the subtraction; three float32 averaging steps on either side and the
                                                             restatement's one rounding to float32
    with X = S - 1, G = max |g|, P = max |disp_p|, L_b = the largest difference of that component between neighbours along axis b,
    Q = G |nfsp| + P, M = Q / |nmsp ms| + |mlo|."""
    field_p = np.asarray(field_p, F64)
    n = field_p.shape[:3]
    g3 = np.asarray(geom, F64).reshape(9, 3)
    fs, lo, nfsp, nmsp, ms, mlo = (np.abs(g3[i]) for i in range(6))
    X = np.array(full, F64) - 1.0
    G = np.maximum(np.abs(g3[0] * (0.0 - g3[1])), np.abs(g3[0] * (X - g3[1])))
    dg = 8 * U32 * (fs * X + fs * lo)
    ds = dg + U32 * (4 * G + np.array(n, F64))
    E = np.zeros(3)
    for c in range(3):
        P = np.abs(field_p[..., c]).max()
        L = [np.abs(np.diff(field_p[..., c], axis=b)).max() if n[b] > 1 else 0.0 for b in range(3)]
        dp = sum(L[b] * ds[b] for b in range(3)) + 12 * U32 * P
        Q = G[c] * nfsp[c] + P
        M = Q / (nmsp[c] * ms[c]) + mlo[c]
        dm = (((dg[c] + U32 * G[c]) * nfsp[c] + dp + U32 * Q) / nmsp[c] + U32 * Q / nmsp[c]) / ms[c] + 2 * U32 * Q / (nmsp[c] * ms[c]) + U32 * M
        E[c] = dm + 8 * U32 * (M + X[c])
    return E
