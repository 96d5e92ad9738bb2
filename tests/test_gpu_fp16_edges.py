"""storage="fp16" and +Inf costs where half precision differs from float32 (run on the MI355X box with `-m gpu`).

The parity suite grades the half-precision paths on uniform [0, 1) features: costs of 0.5 .. 3, normal halves, hardly a tie.  Here:
  (1) the two rounding kernels (cvx_round_f16_f32, cvx_pack_field_f64 with quantize = 1) at every boundary of float32 -> half;
  (2) the half cost volume as corrfused.hip stores it -- subnormal values, mass ties, overflow to +Inf, all-Inf columns -- on geometries
      that reach each store path of the kernel (partial quads with d % 4 = 1, 2, 3, one displacement, hw > 8, y tiles);
  (3) the plain argmin and the six coupled passes (pruned and streaming) on such half volumes, on the pruning edge cases cast to half,
      on NaN columns, and on float32 / half volumes with +Inf entries: +Inf costs follow torch.argmin, an all-Inf column gives index 0;
  (4) the Adam loop on half-precision feature records with 1, 4 and 7 channels in all three modes, and the whole pair.
Every comparison is exact (np.array_equal; NaN patterns and signs included where they can occur) against the CPU oracle, which
tests/test_oracle_operators.py pins to plain torch on the same inputs (tests/fp16_edge_cases.py)."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp16_edge_cases as E  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).to(DEV)           # (a copy: the shared references are read-only)


def host(t):
    return t.detach().cpu().numpy()


def gid(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module")
def U():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from convexadam_amd import convex_adam_utils
    return convex_adam_utils


@pytest.fixture(scope="module")
def L():
    from convexadam_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def M():
    from convexadam_amd import convex_adam_MIND
    return convex_adam_MIND


@pytest.fixture(scope="module")
def table():
    t = E.half_boundary_table()
    t.setflags(write=False)
    return t


# ---- (1) rounding to half, at every boundary ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ["all", 1, 255, 256, 257])
def test_round_f16_in_place_at_every_boundary(L, table, n):
    """cvx_round_f16_f32 on a prefix of the table that starts one float past a 16-byte boundary: ties to even, the subnormal range,
    65520 -> +Inf, 2^-25 -> +0, signed zeros, NaN; the floats around the prefix stay untouched (the kernel's tail)."""
    from convexadam_amd import _lib
    n = table.size if n == "all" else n
    buf = torch.full((n + 4,), 7.0, dtype=torch.float32, device=DEV)
    buf[1:1 + n] = dev(table[:n])
    assert buf.data_ptr() % 16 == 0
    _lib.check(L.cvx_round_f16_f32(C.c_void_p(buf.data_ptr() + 4), n, _lib.stream_ptr(DEV)))
    got = host(buf)
    assert got[0] == 7.0 and np.all(got[1 + n:] == 7.0)
    assert E.same(got[1:1 + n], E.widen(table[:n]))


PACK_SHAPES = [(1, 1, 1), (3, 5, 17), (1, 1, 257), (44, 45, 43)]           # V = 1, 255, 257 and 85 140 (the whole table, > 3 * 256)


@pytest.mark.parametrize("where", ["device", "pinned"])
@pytest.mark.parametrize("shape", PACK_SHAPES, ids=gid)
def test_pack_field_quantises_at_every_boundary(L, table, shape, where):
    """cvx_pack_field_f64: [3][H][W][D] float32 -> [H][W][D][3] float64 through half (quantize = 1) or as it is (quantize = 0), into
    device memory and into pinned host memory; a partial last workgroup, a single voxel, and the whole table."""
    from convexadam_amd import _lib
    V = shape[0] * shape[1] * shape[2]
    assert 3 * V >= table.size or V <= 257
    x = np.resize(table, 3 * V).reshape((3,) + shape)
    xd = dev(x)
    for quantize in (1, 0):
        if where == "device":
            out = torch.full((3 * V + 2,), 7.0, dtype=torch.float64, device=DEV)
        else:
            out = torch.full((3 * V + 2,), 7.0, dtype=torch.float64).pin_memory()
        _lib.check(L.cvx_pack_field_f64(C.c_void_p(xd.data_ptr()), *shape, quantize, C.c_void_p(out.data_ptr() + 8), _lib.stream_ptr(DEV)))
        torch.cuda.synchronize()
        got = host(out)
        assert got[0] == 7.0 and got[-1] == 7.0
        moved = np.moveaxis(x, 0, -1)
        want = E.to_half(moved).astype(np.float64) if quantize else moved.astype(np.float64)
        assert E.same(got[1:-1].reshape(shape + (3,)), want), quantize


def test_pack_field_to_host_through_half(M, table):
    shape = PACK_SHAPES[-1]
    x = np.resize(table, 3 * shape[0] * shape[1] * shape[2]).reshape((3,) + shape)
    got = M.pack_field_to_host(dev(x), dtype=torch.float16)
    assert got.dtype == np.float64 and got.shape == shape + (3,)
    assert E.same(got, E.to_half(np.moveaxis(x, 0, -1)).astype(np.float64))
    assert E.same(M.pack_field_to_host(dev(x), dtype=torch.float32), np.moveaxis(x, 0, -1).astype(np.float64))


# ---- (2) the half cost volume as the kernel stores it ------------------------------------------------------------------------------
_oracle_volumes = {}


def oracle_volume(orc, C_, shape, hw, kind):
    """(f, m, the oracle's float32 volume) of a case, computed once and left unchanged; the case's property is asserted here, on the
    oracle's side, before any kernel runs."""
    key = (C_, shape, hw, kind)
    if key not in _oracle_volumes:
        f, m = E.feature_pair(C_, shape, hw, kind)
        ref, _ = orc.correlate(f, m, hw)
        for a in (f, m, ref):
            a.setflags(write=False)
        _oracle_volumes[key] = (f, m, ref)
    f, m, ref = _oracle_volumes[key]
    p = E.volume_property(kind, ref)                # (asserts that the float32 volume is finite)
    assert E.property_holds(kind, ref.shape[0], p), "%s case of %s: %g" % (kind, key, p)
    return f, m, ref


def same_half(got, want):
    """two float16 arrays: equal bits but for NaN payloads"""
    nan = np.isnan(want)
    return got.dtype == want.dtype == np.float16 and got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got[~nan].view(np.uint16), want[~nan].view(np.uint16))


@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("C_,shape,hw", E.GEOMETRIES, ids=gid)
def test_half_volume_bits_and_first_minimum(U, orc, C_, shape, hw, kind):
    """correlate(storage="fp16") = the oracle's float32 volume rounded once to half -- same bits, same +Inf pattern -- and its argmin is
    the FIRST minimum of the widened stored values: index 0 for a column of equal costs, all zeros and all +Inf included."""
    f, m, ref = oracle_volume(orc, C_, shape, hw, kind)
    ssd, am = U.correlate(dev(f)[None], dev(m)[None], hw, 1, shape, C_, storage="fp16")
    assert ssd.dtype == torch.float16 and ssd.element_size() == 2
    want = E.to_half(ref)
    assert not np.isnan(want).any()
    got = host(ssd)
    assert same_half(got, want), "%d of %d stored values differ" % (int((got.view(np.uint16) != want.view(np.uint16)).sum()), want.size)
    assert np.array_equal(np.isposinf(got), np.isposinf(want))
    assert np.array_equal(host(am), E.first_minimum(want.astype(np.float32)))


@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("C_,shape,hw", E.GEOMETRIES[:2], ids=gid)
def test_half_values_in_a_float32_buffer(U, L, orc, C_, shape, hw, kind):
    """cvx_corr_opts.f16 = 1: the values of the half volume in a float32 buffer, and the same argmin."""
    from convexadam_amd import _lib
    f, m, ref = oracle_volume(orc, C_, shape, hw, kind)
    ssd16, am16 = U.correlate(dev(f)[None], dev(m)[None], hw, 1, shape, C_, storage="fp16")
    K = (2 * hw + 1) ** 3
    fd, md = dev(f), dev(m)
    ssd = torch.full((K,) + shape, 7.0, dtype=torch.float32, device=DEV)
    am = torch.full(shape, -1, dtype=torch.int64, device=DEV)
    nws = L.cvx_correlate_workspace_bytes(C_, *shape, hw)
    ws = _lib.workspace(nws, torch.device(DEV))
    opts = _lib.CorrOpts(0, 2, 0, 1)
    _lib.check(L.cvx_correlate_ex_f32(_lib.ptr(fd), _lib.ptr(md), C_, *shape, hw, C.byref(opts), _lib.ptr(ssd), _lib.ptr(am), _lib.ptr(ws), nws,
                                      _lib.stream_ptr(DEV)))
    assert E.same(host(ssd), host(ssd16).astype(np.float32))
    assert E.same(host(ssd), E.widen(ref))
    assert np.array_equal(host(am), host(am16))


# ---- (3) argmin and coupled passes on half volumes and on +Inf costs -----------------------------------------------------------
# The passes three ways: streaming (no_prune), the default (pruned; a pass whose listed boxes exceed a chunk budget streams instead, and
# the scan then also overwrites what the voxel kernel settled -- on volumes of a few hundred voxels with flat columns that is every
# pass), and pruned with an unreachable budget, so that cand_box decides every voxel of every pass.
PASS_MODES = [("no_prune", 1), ("no_prune", 0), ("prune_stream_above", 1 << 30)]


@contextlib.contextmanager
def option(L, name, value):
    """Sets a library option for the duration of a with-block and restores the previous value."""
    old = L.cvx_get_option(name.encode())
    assert L.cvx_set_option(name.encode(), value) == 0
    try:
        yield
    finally:
        L.cvx_set_option(name.encode(), old)


def check_coupled(U, L, orc, vol, am, hw, half):
    """U.coupled_convex on `vol` (float32; cast to half on the host first if `half`) in each of PASS_MODES against the oracle on the
    values the kernels see."""
    shape = vol.shape[1:]
    mesh = orc.disp_mesh(hw)
    seen = E.widen(vol) if half else vol
    want = orc.coupled_convex(seen, am, mesh, hw)
    vd = dev(E.to_half(vol)) if half else dev(vol)
    assert vd.dtype == (torch.float16 if half else torch.float32)
    for name, value in PASS_MODES:
        with option(L, name, value):
            out = host(U.coupled_convex(vd, dev(am), dev(mesh)[:, :, None], 1, shape))[0]
        bad = ~((out == want) | (np.isnan(out) & np.isnan(want)))
        assert E.same(out, want), "%s = %d: %d of %d values differ from the oracle's, first at %s" % (
            name, value, int(bad.sum()), want.size, tuple(np.argwhere(bad)[0]) if bad.any() else None)
    return want


@pytest.mark.parametrize("kind", E.PRUNING_KINDS)
def test_pruning_edge_cases_on_half(U, L, orc, kind):
    """The inputs of test_coupled_convex_pruning_edge_cases as a half volume (__half instances of k_argmin_voxel / k_argmin_wave /
    k_argmin4_stream and of cand_box; cvx_coupled_convex_f16 takes its lower bound from its own minimum pass)."""
    ssd, am, hw = E.pruning_volume(kind, tiny=6e-8)
    seen = E.widen(ssd)
    if "zero_columns" in kind:
        K = ssd.shape[0]
        assert (seen[K // 3, 1, 2, :] == np.float32(2.0 ** -24)).all()          # the entry survives as the smallest half subnormal
        assert (seen[:, 1, 2, :] != 0).sum() == ssd.shape[3]
    if kind == "signed_zero_columns":
        assert np.signbit(seen[::7, :, 1, :]).all()
    if kind not in ("foreign_argmin", "zero_columns_foreign"):
        am = E.first_minimum(seen)                                              # (rounding can add ties in front of the float32 winner)
    check_coupled(U, L, orc, ssd, am, hw, half=True)


def test_bounded_worst_case_on_half(U, L, orc):
    """The input of test_coupled_convex_bounded_worst_case as a half volume: every pass streams (k_argmin4_stream on __half)."""
    ssd, _, hw = E.worst_case_volume()
    seen = E.widen(ssd)
    assert (seen[:, :, :7, :] == np.float32(0.25)).all()
    check_coupled(U, L, orc, ssd, E.first_minimum(seen), hw, half=True)


@pytest.mark.parametrize("seed", ["true_argmin", "foreign_argmin"])
@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("C_,shape,hw", E.GEOMETRIES[:2], ids=gid)
def test_coupled_passes_on_half_volumes(U, L, orc, C_, shape, hw, kind, seed):
    """Subnormal, mass-tied, overflowing and partly all-Inf half volumes through the six passes; (5, 6, 7) has v % 4 != 0 (k_argmin),
    (6, 7, 10) v % 4 == 0 (k_argmin4)."""
    assert (5 * 6 * 7) % 4 != 0 and (6 * 7 * 10) % 4 == 0 and shape in ((5, 6, 7), (6, 7, 10))
    _, _, ref = oracle_volume(orc, C_, shape, hw, kind)
    vol = E.widen(ref)
    am = E.first_minimum(vol)
    if seed == "foreign_argmin":
        am = np.random.default_rng(hw).integers(0, vol.shape[0], shape).astype(np.int64)
    check_coupled(U, L, orc, vol, am, hw, half=True)


@pytest.mark.parametrize("case", [0, 3, 4])
def test_nan_columns_on_half(U, L, orc, case):
    """The three inputs of test_nan_in_the_cost_volume: the coupled passes on the HALF volume keep the first NaN of a column."""
    rng = np.random.default_rng(case)
    shape, hw = (5, 6, 7), 2
    f = rng.random((12,) + shape, dtype=np.float32)
    m = rng.random((12,) + shape, dtype=np.float32)
    if case == 0:
        m[3, 2, 3, 4] = np.nan
    elif case == 3:
        f[:, 2, 2, 2] = np.nan
    else:
        m[0, 0, 0, 0] = np.nan
        m[5, 4, 5, 6] = np.nan
        f[2, 1, 4, 3] = np.nan
    ref = E.to_half(orc.correlate(f, m, hw)[0])
    assert np.isnan(ref).any()
    ssd, am = U.correlate(dev(f)[None], dev(m)[None], hw, 1, shape, 12, storage="fp16")
    assert same_half(host(ssd), ref)
    col = ref.astype(np.float32).reshape(ref.shape[0], -1)
    first = np.where(np.isnan(col).any(0), np.isnan(col).argmax(0), np.where(np.isnan(col), np.inf, col).argmin(0)).reshape(shape)
    assert np.array_equal(host(am), first)
    check_coupled(U, L, orc, ref.astype(np.float32), first.astype(np.int64), hw, half=True)
    other = (first + 7) % ref.shape[0]                                         # a caller's argmin that is not the first NaN
    check_coupled(U, L, orc, ref.astype(np.float32), other.astype(np.int64), hw, half=True)


@pytest.mark.parametrize("half", [False, True], ids=["float32", "half"])
@pytest.mark.parametrize("seed", ["true_argmin", "foreign_argmin"])
@pytest.mark.parametrize("hw", [2, 3])
@pytest.mark.parametrize("kind", E.INF_KINDS)
def test_coupled_passes_with_infinite_costs(U, L, orc, kind, hw, seed, half):
    """+Inf entries: scattered, whole columns (interior, faces, a corner), a plane, a block.  An all-Inf column has no usable bound
    (Inf - Inf); its argmin is index 0 in every pass, also where the smoothed field sits exactly on another lattice point -- which
    one foreign displacement for every voxel produces throughout the interior."""
    ssd = E.inf_volume(kind, hw)
    assert np.isposinf(ssd).any() and not np.isnan(ssd).any() and E.same(ssd, E.widen(ssd))
    if kind == "scattered":
        assert 0.35 < np.isposinf(ssd).mean() < 0.45
    else:
        assert np.isposinf(ssd).reshape(ssd.shape[0], -1).all(0).any()
    am = E.foreign_constant_argmin(hw) if seed == "foreign_argmin" else E.first_minimum(ssd)
    check_coupled(U, L, orc, ssd, am, hw, half)


@pytest.mark.parametrize("half", [False, True], ids=["float32", "half"])
def test_coupled_passes_with_u_on_a_lattice_point_of_an_all_inf_column(U, L, orc, half):
    """An all-Inf sheet one voxel thick between winners at (1, 1, 1): the first smoothing step is exactly (0, 0, 0) on the sheet
    (asserted on the oracle's side), a lattice point other than mesh[0]; the sheet's winner stays index 0."""
    ssd, am, hw, x0 = E.lattice_sheet_volume()
    mesh = orc.disp_mesh(hw)
    assert np.array_equal(mesh[:, 0], [-2, -2, -2]) and np.array_equal(mesh[:, 93], [1, 1, 1])
    assert np.isposinf(ssd[:, :, :, x0]).all() and np.isfinite(np.delete(ssd, x0, 3)).all()
    u0 = orc.box_zero(mesh[:, am.reshape(-1)].reshape((3,) + am.shape), 3)
    assert (u0[:, 1:-1, 1:-1, x0] == 0).all() and u0[:, 1:-1, 1:-1, x0].size > 0
    check_coupled(U, L, orc, ssd, am, hw, half)


# ---- (4) Adam loop on half records, and the whole pair ---------------------------------------------------------------------------
@pytest.mark.parametrize("feat", ["subnormal", "large"])
@pytest.mark.parametrize("mode", ["exact", "fast", "fast_all"])
@pytest.mark.parametrize("C_", [1, 4, 7])
def test_adam_on_half_records(U, orc, C_, mode, feat):
    """adam_run(storage="fp16") with 1, 4 and 7 channels (less than, exactly and more than one four-channel record) on features whose
    half records are subnormal (s = 2^-16) or reach +-60000: U, P and G equal the oracle's loop on numpy-rounded features.  No entry point refuses one of these channel counts
    (the loop's only refusals are control grids of about 2^31 bytes and box chains outside the separable kernel's range)."""
    grid = (10, 12, 14)
    rng = np.random.default_rng(C_ + len(mode) + len(feat))
    if feat == "subnormal":
        F2 = rng.random((C_,) + grid, dtype=np.float32) * np.float32(2.0 ** -16)
        M2 = rng.random((C_,) + grid, dtype=np.float32) * np.float32(2.0 ** -16)
        assert (np.abs(E.widen(F2)) < 2.0 ** -14).all() and (E.widen(F2) != F2).any()
    else:
        F2 = ((rng.random((C_,) + grid, dtype=np.float32) * 2 - 1) * np.float32(60000.0)).astype(np.float32)
        M2 = ((rng.random((C_,) + grid, dtype=np.float32) * 2 - 1) * np.float32(60000.0)).astype(np.float32)
        assert np.isfinite(E.widen(F2)).all() and np.isfinite(E.widen(M2)).all() and np.abs(F2).max() > 50000
    P0 = (0.5 * rng.standard_normal((3,) + grid)).astype(np.float32)
    Ud, st = U.adam_run(dev(F2)[None], dev(M2)[None], dev(P0)[None], 1.25, 3, return_state=True, storage="fp16", mode=mode)
    r = orc.adam_run(E.widen(F2), E.widen(M2), P0, 1.25, 3, want_grad=True, mode=mode)
    assert E.same(host(Ud)[0], r["U"])
    assert E.same(host(st["P"])[0], r["P"])
    assert E.same(host(st["G"])[0], r["G"])


def pair_features(kind):
    rng = np.random.default_rng(len(kind))
    C_, shape = 12, (24, 32, 28)
    f = rng.random((C_,) + shape, dtype=np.float32)
    if kind == "zero_background":            # exact zeros and ties
        m = np.roll(f, (1, -1, 2), (1, 2, 3)).copy()
        f[:, :, :14] = 0
        m[:, :, :15] = 0
    elif kind == "subnormal_costs":
        f = f * np.float32(2.0 ** -9)
        m = rng.random((C_,) + shape, dtype=np.float32) * np.float32(2.0 ** -9)
    else:                                    # a bright block whose costs overflow; the features themselves stay far below 65504
        f = f * np.float32(16)
        m = rng.random((C_,) + shape, dtype=np.float32) * np.float32(16)
        f[:, 6:16, 8:20, 10:20] += np.float32(2000)
    return f, m


@pytest.mark.parametrize("kind", ["zero_background", "subnormal_costs", "overflowing_block"])
def test_pair_with_half_storage(M, L, orc, kind):
    """register_pair_device(storage="fp16") on features: both cost volumes, their argmins, twelve coupled passes, inverse consistency
    and two Adam iterations on half records against the oracle's pipeline, with the coupled passes in each of PASS_MODES."""
    f, m = pair_features(kind)
    assert max(np.abs(f).max(), np.abs(m).max()) < 65504
    kw = dict(lambda_weight=1.25, grid_sp=2, disp_hw=3, selected_niter=2, grid_sp_adam=2, ic=True, storage="fp16", adam_mode="exact")
    ref, st = orc.convex_adam_pipeline(None, None, features=(f, m), return_stages=True, **kw)
    vol = E.to_half(orc.correlate(st["fs"], st["ms"], 3)[0])
    if kind == "zero_background":
        assert (vol == 0).mean() > 0.1 and E.tied_columns(vol.astype(np.float32)) > 0.3
    elif kind == "subnormal_costs":
        assert (np.abs(vol.astype(np.float32)) < 2.0 ** -14).mean() > 0.9
    else:
        allinf = np.isposinf(vol).reshape(vol.shape[0], -1).all(0).mean()
        assert 0.05 < allinf < 0.9 and np.isfinite(orc.correlate(st["fs"], st["ms"], 3)[0]).all()
    for name, value in PASS_MODES:
        with option(L, name, value):
            out = host(M.register_pair_device(feat_fixed=dev(f), feat_moving=dev(m), **kw))
        assert E.same(np.moveaxis(out, 0, -1).astype(np.float64), ref), (name, value)
