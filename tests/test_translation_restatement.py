"""The restatement of the field-mean contract (tests/translation_restatement.py) against exact arithmetic and against the host path of
convex_adam_translation.  No GPU.

Against math.fsum the bound is derived, not observed: no value passes through more than L = K + 8 + ceil(nblocks / 256) + 8 additions
(K per thread, 8 tree steps, the finish's per-thread adds and its 8 tree steps), each of which rounds by at most 2^-53 of a partial sum
that is itself at most sum|v| (1 + L 2^-53); hence |sum - fsum| <= L 2^-53 sum|v| (1 + 1e-3).
Against field_to_translation the whole-voxel translation must be the same; the test first asserts that the host's value before rounding
lies at least 0.25 from a half-integer, a condition on the chosen inputs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import translation_restatement as R  # noqa: E402

SIZES = (1, 63, 64, 65, 255, 256, 257, R.S - 1, R.S, R.S + 1, 3 * R.S + 77, 256 * R.S, 256 * R.S + 1)


def test_constants_match_the_kernel():
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "convexadam_amd", "csrc", "fieldmean.hip")).read()
    val = lambda name: int(re.search(r"constexpr int %s\s*=\s*(\d+)" % name, src).group(1))      # noqa: E731
    assert (val("FM_THREADS"), val("FM_K")) == (R.THREADS, R.K) and R.S == R.THREADS * R.K


@pytest.mark.parametrize("V", SIZES)
def test_restatement_against_fsum(V):
    rng = np.random.default_rng(V)
    v32 = (rng.standard_normal((V, 3)) * np.array([3.0, 40.0, 0.01]) + np.array([2.5, -0.3, 0.0])).astype(np.float32)
    mask = rng.random(V) < 0.4
    for values in (v32.astype(np.float64), R.quantize_f16(v32), rng.standard_normal((V, 3)) * 1e6):
        for inc in (None, mask):
            sums, count = R.field_sums(values, inc)
            exact, bound = R.fsum_bound(values, inc)
            assert count == (V if inc is None else int(mask.sum()))
            assert np.all(np.abs(sums - exact) <= bound), (V, sums - exact, bound)
    assert R.added_at_most(V) == R.K + 8 + -(-R.n_blocks(V) // 256) + 8


def test_restatement_edges():
    V = R.S + 5
    zero = R.field_sums(np.full((V, 3), 7.0), np.zeros(V, bool))
    assert zero[1] == 0 and np.array_equal(zero[0], np.zeros(3)) and not np.signbit(zero[0]).any()
    v = np.ones((V, 3))
    v[R.S + 1, 1] = np.nan
    v[17, 2] = np.inf
    sums, count = R.field_sums(v)
    assert count == V and sums[0] == V and np.isnan(sums[1]) and sums[2] == np.inf
    inc = np.ones(V, bool)
    inc[[17, R.S + 1]] = False
    sums, count = R.field_sums(v, inc)
    assert count == V - 2 and np.array_equal(sums, np.full(3, V - 2.0))
    # the float16 round trip: ties to even, subnormals, overflow
    q = R.quantize_f16(np.array([2049.0, 2051.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 65504.0, 65519.9, 65520.0,
                                 -70000.0], np.float32))
    assert np.array_equal(q, [2048.0, 2052.0, 1.0, 1 + 2.0 ** -9, 2.0 ** -24, 0.0, 2.0 ** -23, 65504.0, 65504.0, np.inf, -np.inf])
    # both layouts name the same values
    f = np.arange(2 * 3 * 4 * 3, dtype=np.float64).reshape(2, 3, 4, 3)
    assert np.array_equal(R.field_values(f, "last"), R.field_values(np.ascontiguousarray(np.moveaxis(f, 3, 0)), "first"))


@pytest.mark.parametrize("spacing_xyz", [(1.0, 1.0, 1.0), (1.0, 1.0, 2.0), (1.1, 1.3, 2.0)])
def test_same_whole_voxel_translation_as_the_host_path(spacing_xyz):
    from convexadam_amd.convex_adam_translation import field_to_translation, mean_to_translation
    rng = np.random.default_rng(11)
    shape = (21, 26, 31)                                                  # 16926 voxels: five blocks, the last one partial
    f32 = (rng.standard_normal(shape + (3,)) * 0.8 + np.array([4.2, -0.1, -2.2])).astype(np.float32)
    field = f32.astype(np.float16).astype(np.float64)                     # what convex_adam_pt returns
    zz, yy, xx = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    mask = ((zz - 10) / 8.0) ** 2 + ((yy - 13) / 9.0) ** 2 + ((xx - 15) / 12.0) ** 2 <= 1.0
    for m in (None, mask):
        host_mean = np.mean(field[m], axis=0) if m is not None else np.mean(field, axis=(0, 1, 2))
        pre = host_mean / np.array(spacing_xyz[::-1])
        assert np.all(np.abs(pre - np.floor(pre) - 0.5) >= 0.25), pre     # a condition on the inputs above, not a tolerance of the code
        sums, count = R.field_mean(f32, "last", None if m is None else m.reshape(-1), quantize=True)
        assert count == (field.size // 3 if m is None else int(m.sum()))
        assert mean_to_translation(sums / count, spacing_xyz) == field_to_translation(field, spacing_xyz, m)
