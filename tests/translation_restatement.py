"""numpy float64 restatement of the arithmetic contract of csrc/fieldmean.hip: which voxels count, the float16 round
trip, and the ORDER of the additions.  Test infrastructure only: the product never imports it.

The order (K = 16, S = 256 K):
    voxel v = (z W + y) D + x; block b owns [b S, (b + 1) S); thread t adds voxels b S + k 256 + t, k = 0 .. K - 1, in that order from 0.0;
    the 256 accumulators of a block are combined by acc[t] += acc[t + s], t < s, for s = 128, 64, .., 1;
    the finish lets thread t add block partials t, t + 256, .. in order from 0.0 and runs the same tree.
An excluded voxel (and the padding behind the last voxel or the last partial) adds nothing in the kernel.  Here it adds +0.0, which gives
the same bits: an accumulator starts at +0.0 and a sum of two floats is -0.0 only if both are -0.0, so no accumulator is ever -0.0, and
x + 0.0 == x bit for bit for every other x, NaN payloads aside (the tests compare NaN-ness, not payloads).
"""
import math

import numpy as np

import geometry_restatement as G

THREADS, K = 256, 16
S = THREADS * K


def quantize_f16(values):
    """convex_adam_pt's default dtype round trip: float32 -> float16 (nearest even; beyond 65504 -> inf) -> float64"""
    values = np.asarray(values)
    assert values.dtype == np.float32, "the round trip is defined for a float32 field"
    with np.errstate(over="ignore"):
        return values.astype(np.float16).astype(np.float64)


def field_values(field, layout):
    """(V, 3) view of a field: layout 'last' = (H, W, D, 3), 'first' = (3, H, W, D); components z, y, x"""
    field = np.asarray(field)
    return field.reshape(-1, 3) if layout == "last" else field.reshape(3, -1).T


def _tree(acc):
    """acc (..., 256) -> (...): acc[t] += acc[t + s] for s = 128 .. 1"""
    acc = acc.copy()
    s = THREADS // 2
    while s >= 1:
        acc[..., :s] += acc[..., s:2 * s]
        s //= 2
    return acc[..., 0]


def n_blocks(V):
    return -(-V // S)


def field_sums(values, include=None):
    """values (V, 3) float64 (already through quantize_f16 if that applies), include (V,) bool or None -> (sums float64[3], count)"""
    values = np.asarray(values, np.float64)
    V = values.shape[0]
    include = np.ones(V, bool) if include is None else np.asarray(include, bool).reshape(-1)
    nb = n_blocks(V)
    padded = np.zeros((nb * S, 3), np.float64)
    padded[:V] = np.where(include[:, None], values, 0.0)
    per_thread = padded.reshape(nb, K, THREADS, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        acc = np.zeros((nb, THREADS, 3), np.float64)
        for k in range(K):                                         # thread t of block b: voxels b S + k 256 + t in the order of k
            acc += per_thread[:, k]
        partial = _tree(np.moveaxis(acc, 1, -1))                    # (nb, 3)
        rounds = -(-nb // THREADS)
        padded_partials = np.zeros((rounds * THREADS, 3), np.float64)
        padded_partials[:nb] = partial
        padded_partials = padded_partials.reshape(rounds, THREADS, 3)
        acc = np.zeros((THREADS, 3), np.float64)
        for r in range(rounds):                                     # thread t: partials t, t + 256, ..
            acc += padded_partials[r]
        sums = _tree(acc.T)
    return sums, int(include.sum())


def added_at_most(V):
    """L: no value passes through more than K + 8 + ceil(nblocks / 256) + 8 additions"""
    return K + 8 + -(-n_blocks(V) // THREADS) + 8


def fsum_bound(values, include=None):
    """(exact sums by math.fsum, bound): |sum - fsum| <= L 2^-53 sum|v| (1 + 1e-3) per component.  Every addition rounds by at most
    2^-53 of its result, a partial sum of at most sum|v| (1 + L 2^-53); a value passes through at most L of them."""
    values = np.asarray(values, np.float64)
    inc = np.ones(values.shape[0], bool) if include is None else np.asarray(include, bool).reshape(-1)
    v = values[inc]
    exact = np.array([math.fsum(v[:, c].tolist()) for c in range(3)])
    bound = np.array([added_at_most(values.shape[0]) * 2.0 ** -53 * math.fsum(np.abs(v[:, c]).tolist()) * (1 + 1e-3) for c in range(3)])
    return exact, bound


def seg_mask(seg, seg_grid, field_grid):
    """the mask of the two-step path, resample(seg) > 0: the resampling restatement of geometry_restatement, the cast of the source's
    dtype (float64 as it is, float32 rounded, integers by rint, half to even), then > 0 -> (H, W, D) bool"""
    resampled, _ = G.resample(np.asarray(seg), G.grid_of(seg_grid), G.grid_of(field_grid))
    return resampled > 0


def field_mean(field, layout, include=None, quantize=False):
    """(sums, count) of a field array as the device call sees it"""
    v = field_values(field, layout)
    return field_sums(quantize_f16(v) if quantize else v.astype(np.float64), include)
