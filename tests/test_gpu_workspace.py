"""Workspace contract of every entry point that takes a caller-provided workspace (run on the MI355X box with `-m gpu`).

For each operator, shape and layout-changing option: a call with EXACTLY the queried size -- cut from the front of a larger buffer whose
tail holds a byte pattern -- succeeds, leaves the pattern intact and produces the same bits as a call with a generous workspace; a call
with one byte less is refused with CVX_ERR_WORKSPACE and leaves the outputs untouched.  Every input is a real allocation.

The two workspaces also differ in what they hold when the call starts: zeros in the generous one, 0xFF bytes in the exact one.  The
package's workspace is grow-only and shared by every operator of a thread and stream, so a call always finds another kernel's leftovers;
equal outputs say that no entry point reads a workspace word before it has written it."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TAIL = 8192


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from convexadam_amd import _lib
    return _lib.lib()


class option:
    def __init__(self, L, **kv):
        self.L, self.kv, self.old = L, kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = self.L.cvx_get_option(k.encode())
            assert self.L.cvx_set_option(k.encode(), v) == 0
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.L.cvx_set_option(k.encode(), v)


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rnd(shape, seed, lo=0.0, hi=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (lo + (hi - lo) * torch.rand(shape, generator=g)).to(dtype).to(DEV)


def as_bytes(t):
    return t.contiguous().view(torch.uint8)


def check_workspace(L, need, call, outs, prep=lambda: None):
    """need: the size query's value; call(ws, nbytes) -> rc; outs: every buffer the call writes; prep(): resets in/out buffers."""
    def run(ws, nbytes, stale=None):
        for o in outs:
            as_bytes(o).fill_(0xA5)
        if stale is not None:
            stale[0].fill_(stale[1])            # what another operator might have left in the shared, grow-only workspace
        prep()
        torch.cuda.synchronize()
        before = [o.clone() for o in outs]
        rc = call(ws, nbytes)
        torch.cuda.synchronize()
        return rc, before

    big = torch.empty(need + (1 << 20), dtype=torch.uint8, device=DEV)
    rc, _ = run(p(big), big.numel(), (big, 0x00))
    assert rc == 0, L.cvx_last_error()
    ref = [o.clone() for o in outs]
    buf = torch.empty(need + TAIL, dtype=torch.uint8, device=DEV)
    buf[need:].fill_(0x5A)
    # stale contents: zeros in the generous run, 0xFF bytes here (NaN as floats, -1 as counters, tickets and flags; DESIGN.md section 29 lists
    # who initialises each such word) -- equal outputs then also say that no entry point depends on what its workspace held
    rc, _ = run(p(buf), need, (buf[:need], 0xFF))
    assert rc == 0, L.cvx_last_error()
    assert bool((buf[need:] == 0x5A).all()), "the call wrote behind its queried workspace"
    for o, r in zip(outs, ref):
        assert torch.equal(as_bytes(o), as_bytes(r)), "outputs differ between the exact and a generous workspace"
    if need > 0:
        rc, before = run(p(buf), need - 1)
        assert rc == -2, "one byte short: rc %d" % rc
        for o, b in zip(outs, before):
            assert torch.equal(as_bytes(o), as_bytes(b)), "a refused call touched its outputs"


SHAPES = [(7, 9, 11), (24, 20, 16)]
BIG = (36, 32, 32)          # > 32768 voxels: the reference-bits mean runs its two-pass cascade (several chunks, slots cleared first)


@pytest.mark.parametrize("shape", SHAPES + [BIG])
@pytest.mark.parametrize("mean_threads", [0, 8])
def test_mindssc(L, shape, mean_threads):
    H, W, D = shape
    img = rnd(shape, 1)
    out = torch.empty((12,) + shape, device=DEV)
    with option(L, mind_mean_threads=mean_threads):
        need = L.cvx_mindssc_workspace_bytes(H, W, D, 1, 2)
        check_workspace(L, need, lambda ws, n: L.cvx_mindssc_f32(p(img), H, W, D, 1, 2, p(out), ws, n, stream()), [out])


@pytest.mark.parametrize("shape", [(12, 12, 20), (24, 20, 16), BIG])
@pytest.mark.parametrize("single", [0, 1])
@pytest.mark.parametrize("mean_threads", [0, 8])
def test_mindssc_pooled(L, shape, single, mean_threads):
    H, W, D = shape
    img = rnd(shape, 2)
    o1 = torch.empty((12, H // 4, W // 4, D // 4), device=DEV)
    o2 = torch.empty((12, H // 2, W // 2, D // 2), device=DEV)
    rep = C.c_int(0)
    with option(L, mind_single=single, mind_mean_threads=mean_threads):
        need = L.cvx_mindssc_workspace_bytes(H, W, D, 1, 2)
        nscr = L.cvx_mindssc_pooled_scratch_bytes(H, W, D, 1, 2, 4, 2)
        scr = torch.empty(max(nscr, 1), dtype=torch.uint8, device=DEV)
        check_workspace(L, need, lambda ws, n: L.cvx_mindssc_pooled_f32(p(img), H, W, D, 1, 2, 4, p(o1), 2, p(o2), p(scr) if nscr else None, nscr,
                                                                         ws, n, C.byref(rep), stream()), [o1, o2, scr])


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("passes", [1, 2, 3])
def test_box_smooth(L, shape, passes):
    H, W, D = shape
    x = rnd((3,) + shape, 3)
    out = torch.empty_like(x)
    need = L.cvx_box_smooth_workspace_bytes(3, H, W, D, passes)
    assert (need == 0) == (passes == 1)
    check_workspace(L, need, lambda ws, n: L.cvx_box_smooth_f32(p(x), 3, H, W, D, 3, passes, p(out), ws, n, stream()), [out])


@pytest.mark.parametrize("shape", SHAPES)
def test_smooth(L, shape):
    from convexadam_amd._lib import Smoother
    H, W, D = shape
    x = rnd((3,) + shape, 4)
    out = torch.empty_like(x)
    sm = Smoother(0, 2, (C.c_int * 4)(3, 5, 0, 0), (C.c_float * 5)(0, 0, 0, 0, 0))
    need = L.cvx_smooth_workspace_bytes(3, H, W, D)
    check_workspace(L, need, lambda ws, n: L.cvx_smooth_f32(p(x), 3, H, W, D, C.byref(sm), 0, p(out), ws, n, stream()), [out])


CORR_SHAPES = [(5, 6, 7), (12, 10, 14)]


@pytest.mark.parametrize("shape", CORR_SHAPES)
@pytest.mark.parametrize("C_", [12, 16])
@pytest.mark.parametrize("fast", [0, 1, 2])
@pytest.mark.parametrize("opts", [{}, {"corr_unfused": 1}, {"corr_fused_all": 1}, {"corr_cert": 2}, {"cert_unfused": 2}])
def test_correlate(L, shape, C_, fast, opts):
    from convexadam_amd._lib import CorrOpts
    h, w, d = shape
    hw = 2
    K, v = (2 * hw + 1) ** 3, h * w * d
    fix, mov = rnd((C_,) + shape, 5), rnd((C_,) + shape, 6)
    ssd = torch.empty(K * v, device=DEV)
    am = torch.empty(v, dtype=torch.int64, device=DEV)
    co = CorrOpts(0, 2, fast, 0)
    with option(L, **opts):
        need = L.cvx_correlate_workspace_bytes(C_, h, w, d, hw)
        big = torch.empty(need + (1 << 20), dtype=torch.uint8, device=DEV)
        rc = L.cvx_correlate_ex_f32(p(fix), p(mov), C_, h, w, d, hw, C.byref(co), p(ssd), p(am), p(big), big.numel(), stream())
        torch.cuda.synchronize()
        if fast == 1 and opts.get("corr_unfused"):           # the fast variant exists only in the fused kernel, which the option turns off
            assert rc == -4, L.cvx_last_error()
            return
        check_workspace(L, need, lambda ws, n: L.cvx_correlate_ex_f32(p(fix), p(mov), C_, h, w, d, hw, C.byref(co), p(ssd), p(am), ws, n, stream()),
                        [ssd, am])


@pytest.mark.parametrize("shape", CORR_SHAPES)
@pytest.mark.parametrize("cf_map", [0, 1])
def test_correlate_census_hw5(L, shape, cf_map):
    """hw = 5 is the one search width at which the co-located launch of the fused kernel (option cf_map = 1, 512 workgroups) has more
    workgroups than items (11 * 11 * 3 = 363): with option cf_census every workgroup that passes the pair test -- up to number 376 --
    writes its four census words.  The census is the last carve of the fused kernel's part of the workspace; behind it lie the 256 bytes
    of slack that every size query adds and then the argmin keys (8 bytes per voxel), which the argmin pass arms after the kernel.  A
    carve of items + 8 slots ended 192 bytes short of the last record's end: the overhang stayed inside that slack, so neither the keys
    nor the tail pattern could show it; the carve now holds a slot per workgroup.  This test therefore could not have failed on the old carve:
    what it pins is that the census, at the one width where it has more writers than items, changes neither the volume nor the argmin
    and keeps the workspace contract."""
    h, w, d = shape
    hw, C_ = 5, 12
    K, v = (2 * hw + 1) ** 3, h * w * d
    fix, mov = rnd((C_,) + shape, 31), rnd((C_,) + shape, 32)
    ssd = torch.empty(K * v, device=DEV)
    am = torch.empty(v, dtype=torch.int64, device=DEV)
    with option(L, cf_map=cf_map):
        need = L.cvx_correlate_workspace_bytes(C_, h, w, d, hw)
        plain = torch.empty(need, dtype=torch.uint8, device=DEV)
        assert L.cvx_correlate_f32(p(fix), p(mov), C_, h, w, d, hw, p(ssd), p(am), p(plain), need, stream()) == 0, L.cvx_last_error()
        torch.cuda.synchronize()
        want = [ssd.clone(), am.clone()]
        with option(L, cf_census=1):
            assert L.cvx_correlate_workspace_bytes(C_, h, w, d, hw) == need           # the census is always carved
            check_workspace(L, need, lambda ws, n: L.cvx_correlate_f32(p(fix), p(mov), C_, h, w, d, hw, p(ssd), p(am), ws, n, stream()), [ssd, am])
            assert L.cvx_correlate_f32(p(fix), p(mov), C_, h, w, d, hw, p(ssd), p(am), p(plain), need, stream()) == 0, L.cvx_last_error()
            torch.cuda.synchronize()
    assert torch.equal(ssd, want[0]) and torch.equal(am, want[1]), "the census changed the volume or the argmin"


@pytest.mark.parametrize("shape", CORR_SHAPES)
@pytest.mark.parametrize("opts", [{}, {"corr_unfused": 1}])
def test_correlate_plain(L, shape, opts):
    h, w, d = shape
    hw, C_ = 3, 12
    fix, mov = rnd((C_,) + shape, 27), rnd((C_,) + shape, 28)
    ssd = torch.empty((2 * hw + 1) ** 3 * h * w * d, device=DEV)
    am = torch.empty(h * w * d, dtype=torch.int64, device=DEV)
    with option(L, **opts):
        need = L.cvx_correlate_workspace_bytes(C_, h, w, d, hw)
        check_workspace(L, need, lambda ws, n: L.cvx_correlate_f32(p(fix), p(mov), C_, h, w, d, hw, p(ssd), p(am), ws, n, stream()), [ssd, am])


def _volume(L, C_, shape, hw, seed):
    h, w, d = shape
    K, v = (2 * hw + 1) ** 3, h * w * d
    fix, mov = rnd((C_,) + shape, seed), rnd((C_,) + shape, seed + 1)
    ssd = torch.empty(K * v, device=DEV)
    am = torch.empty(v, dtype=torch.int64, device=DEV)
    need = L.cvx_correlate_workspace_bytes(C_, h, w, d, hw)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert L.cvx_correlate_f32(p(fix), p(mov), C_, h, w, d, hw, p(ssd), p(am), p(ws), need, stream()) == 0
    mesh = torch.empty(3 * K, device=DEV)
    assert L.cvx_disp_mesh_f32(hw, p(mesh), stream()) == 0
    return ssd, am, mesh


@pytest.mark.parametrize("shape", CORR_SHAPES)
@pytest.mark.parametrize("no_prune", [0, 1])
@pytest.mark.parametrize("f16", [0, 1])
def test_coupled_convex(L, shape, no_prune, f16):
    h, w, d = shape
    hw = 2
    ssd, am, mesh = _volume(L, 12, shape, hw, 7)
    if f16:
        ssd = ssd.half()
    fn = L.cvx_coupled_convex_f16 if f16 else L.cvx_coupled_convex_f32
    out = torch.empty(3 * h * w * d, device=DEV)
    with option(L, no_prune=no_prune):
        need = L.cvx_coupled_convex_workspace_bytes(h, w, d, hw)
        check_workspace(L, need, lambda ws, n: fn(p(ssd), p(am), p(mesh), h, w, d, hw, p(out), ws, n, stream()), [out])


def _bases(L, shape):
    bs = []
    for n in shape:
        b = torch.empty(n, device=DEV)
        assert L.cvx_affine_base_f32(n, p(b), stream()) == 0
        bs.append(b)
    return bs


@pytest.mark.parametrize("shape", CORR_SHAPES)
@pytest.mark.parametrize("ic_fused", [0, 1])
def test_inverse_consistency(L, shape, ic_fused):
    h, w, d = shape
    f1, f2 = rnd((3,) + shape, 8, -0.05, 0.05), rnd((3,) + shape, 9, -0.05, 0.05)
    o1, o2 = torch.empty_like(f1), torch.empty_like(f2)
    bh, bw, bd = _bases(L, shape)
    with option(L, ic_fused=ic_fused):
        need = L.cvx_inverse_consistency_workspace_bytes(h, w, d)
        check_workspace(L, need, lambda ws, n: L.cvx_inverse_consistency_f32(p(f1), p(f2), h, w, d, 4, p(bh), p(bw), p(bd), p(o1), p(o2), ws, n,
                                                                              stream()), [o1, o2])


# every Adam entry point; the box chain {3, 5} takes the generic smoother path, which uses the two temporaries of the layout
ADAM = {
    "run": lambda L, a, sm: L.cvx_adam_run_f32(*a),
    "fast": lambda L, a, sm: L.cvx_adam_run_fast_f32(*a),
    "fast_all": lambda L, a, sm: L.cvx_adam_run_fast_all_f32(*a),
    "smoother_chain": lambda L, a, sm: L.cvx_adam_run_smoother_f32(*a[:-3], sm, *a[-3:]),
    "ex_chain_f16": lambda L, a, sm: L.cvx_adam_run_ex_f32(*a[:-3], sm, 1, *a[-3:]),
    "mode_fast_chain": lambda L, a, sm: L.cvx_adam_run_mode_f32(*a[:-3], sm, 1, *a[-3:]),
    "mode_fast_all_chain_f16": lambda L, a, sm: L.cvx_adam_run_mode_f32(*a[:-3], sm, 2 | 16, *a[-3:]),
}


@pytest.mark.parametrize("shape", [(5, 6, 7), (12, 10, 14)])
@pytest.mark.parametrize("entry", sorted(ADAM))
def test_adam(L, shape, entry):
    from convexadam_amd._lib import Smoother
    h, w, d = shape
    C_ = 12
    F2, M2 = rnd((C_,) + shape, 10), rnd((C_,) + shape, 11)
    P0 = rnd((3,) + shape, 12, -0.5, 0.5)
    P, m, v, U = torch.empty_like(P0), torch.empty_like(P0), torch.empty_like(P0), torch.empty_like(P0)
    bh, bw, bd = _bases(L, shape)
    sm = C.byref(Smoother(0, 2, (C.c_int * 4)(3, 5, 0, 0), (C.c_float * 5)(0, 0, 0, 0, 0)))

    def prep():
        P.copy_(P0); m.zero_(); v.zero_()

    def call(ws, n):
        a = (p(F2), p(M2), C_, h, w, d, p(P), p(m), p(v), 1.25, 3, 0, 1.0, p(bh), p(bw), p(bd), p(U), None, None, 0, None, ws, n, stream())
        return ADAM[entry](L, a, sm)
    need = L.cvx_adam_workspace_bytes(C_, h, w, d)
    check_workspace(L, need, call, [P, m, v, U], prep)


@pytest.mark.parametrize("shape", SHAPES)
def test_feature_transform_and_edt(L, shape):
    H, W, D = shape
    obj = (rnd(shape, 13) > 0.7).float()
    feat = torch.empty((3,) + shape, dtype=torch.int32, device=DEV)
    need = L.cvx_feature_transform_workspace_bytes(H, W, D)
    check_workspace(L, need, lambda ws, n: L.cvx_feature_transform_i32(p(obj), H, W, D, p(feat), ws, n, stream()), [feat])
    objs = (rnd((2,) + shape, 14) > 0.6).float()
    d2 = torch.empty((2,) + shape, dtype=torch.int32, device=DEV)
    need = L.cvx_edt_squared_workspace_bytes(2, H, W, D)
    check_workspace(L, need, lambda ws, n: L.cvx_edt_squared_i32(p(objs), 2, H, W, D, p(d2), ws, n, stream()), [d2])
    seg = (rnd(shape, 29) * 4).floor()
    labs = (C.c_int * 3)(1, 2, 3)
    d2l = torch.empty((6,) + shape, dtype=torch.int32, device=DEV)           # two volumes per label
    need = L.cvx_edt_squared_workspace_bytes(6, H, W, D)
    check_workspace(L, need, lambda ws, n: L.cvx_edt_squared_labels_i32(p(seg), H, W, D, C.cast(labs, C.c_void_p), 3, p(d2l), ws, n, stream()), [d2l])


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nl", [1, 13])
def test_surface_distance_bits(L, shape, nl):
    H, W, D = shape
    segs = [(rnd(shape, 15 + i) * (nl + 1)).floor().clamp(max=nl) for i in range(2)]
    bits = []
    for sgm in segs:
        b = torch.empty(int(L.cvx_label_bits_bytes(H, W, D, nl)) // 8, dtype=torch.int64, device=DEV)
        assert L.cvx_label_bits_u64(p(sgm), H, W, D, nl, p(b), stream()) == 0
        bits.append(b)
    nbins = (H - 1) ** 2 + (W - 1) ** 2 + (D - 1) ** 2 + 2
    hist = torch.empty((nl, nbins), dtype=torch.int64, device=DEV)
    over = torch.empty(nl, dtype=torch.int32, device=DEV)
    act4 = (C.c_uint64 * 4)(*[(1 << 64) - 1] * 4)

    def prep():
        hist.zero_(); over.zero_()
    need = L.cvx_surface_distance_hist_bits_workspace_bytes(H, W, D, nl)
    check_workspace(L, need, lambda ws, n: L.cvx_surface_distance_hist_bits_i64(p(bits[0]), p(bits[1]), H, W, D, nl, C.cast(act4, C.c_void_p), nbins,
                                                                                p(hist), nbins, p(over), 1, 0, ws, n, stream()), [hist, over], prep)


@pytest.mark.parametrize("n,nrhs", [(5, 1), (37, 3)])
def test_tps_fit(L, n, nrhs):
    c = rnd((n, 3), 17, 0.0, 30.0)
    f = rnd((n, nrhs), 18, -2.0, 2.0)
    theta = torch.empty((n + 4, nrhs), device=DEV)
    need = L.cvx_tps_fit_workspace_bytes(n, nrhs)
    check_workspace(L, need, lambda ws, nb: L.cvx_tps_fit_f32(p(c), p(f), n, nrhs, 0.0, p(theta), ws, nb, stream()), [theta])


@pytest.mark.parametrize("n", [7, 301])
def test_rigid_lts(L, n):
    f = rnd((n, 4), 19, -20.0, 20.0)
    f[:, 3] = 1.0
    m = (f + rnd((n, 4), 20, -0.1, 0.1)).contiguous()
    m[:, 3] = 1.0
    T = torch.empty((4, 4), device=DEV)
    mask = torch.empty(n, dtype=torch.uint8, device=DEV)
    need = L.cvx_rigid_lts_workspace_bytes(n)
    check_workspace(L, need, lambda ws, nb: L.cvx_rigid_lts_f32(p(f), 4, p(m), 4, n, 5, p(T), p(mask), ws, nb, stream()), [T, mask])


PAIR_SHAPES = [(24, 28, 20), (26, 22, 30)]


def _pair(H, W, D, ic, lam, nf):
    from convexadam_amd._lib import PairParams
    return PairParams(H, W, D, 1, 2, lam, 2, 2, 3, 0, 2, ic, nf, 1.0, 0, 2, 0, 0, 0)


@pytest.mark.parametrize("shape", PAIR_SHAPES)
@pytest.mark.parametrize("ic", [0, 1])
@pytest.mark.parametrize("lam", [0.0, 1.25])
@pytest.mark.parametrize("nf", [0, 12])
@pytest.mark.parametrize("opts", [{}, {"corr_cert": 0}, {"corr_cert": 2}, {"corr_cert": 0, "corr_dual": 1}, {"mind_single": 1}, {"no_prune": 1},
                                  {"mind_mean_threads": 8}])
def test_register_pair(L, shape, ic, lam, nf, opts):
    H, W, D = shape
    pp = _pair(H, W, D, ic, lam, nf)
    a, b = rnd(shape, 21), rnd(shape, 22)
    ff, fm = (rnd((nf,) + shape, 23), rnd((nf,) + shape, 24)) if nf else (None, None)
    out = torch.empty((3,) + shape, device=DEV)
    with option(L, **opts):
        need = L.cvx_register_pair_workspace_bytes(C.byref(pp))
        assert need > 0
        check_workspace(L, need, lambda ws, n: L.cvx_register_pair_f32(p(a), p(b), p(ff), p(fm), C.byref(pp), p(out), None, ws, n, stream()), [out])


@pytest.mark.parametrize("shape", PAIR_SHAPES)
@pytest.mark.parametrize("ic", [0, 1])
def test_register_pair_snapshots(L, shape, ic):
    H, W, D = shape
    pp = _pair(H, W, D, ic, 1.25, 0)
    its, sms = (C.c_int * 2)(1, 3), (C.c_int * 2)(0, 3)
    a, b = rnd(shape, 25), rnd(shape, 26)
    out = torch.empty((2, 2, 3) + shape, device=DEV)
    need = L.cvx_register_pair_snapshots_workspace_bytes(C.byref(pp), 2, C.cast(sms, C.c_void_p), 2)
    assert need > 0
    check_workspace(L, need, lambda ws, n: L.cvx_register_pair_snapshots_f32(p(a), p(b), None, None, C.byref(pp), C.cast(its, C.c_void_p), 2,
                                                                             C.cast(sms, C.c_void_p), 2, p(out), ws, n, stream()), [out])


@pytest.mark.parametrize("n_streams", [1, 2])
def test_register_pairs(L, n_streams):
    H, W, D = PAIR_SHAPES[1]
    pp = _pair(H, W, D, 1, 1.25, 0)
    imgs = [rnd(PAIR_SHAPES[1], 30 + i) for i in range(6)]
    outs = [torch.empty((3, H, W, D), device=DEV) for _ in range(3)]
    fix, mov = (C.c_void_p * 3)(*[i.data_ptr() for i in imgs[:3]]), (C.c_void_p * 3)(*[i.data_ptr() for i in imgs[3:]])
    dst = (C.c_void_p * 3)(*[o.data_ptr() for o in outs])
    per = L.cvx_register_pair_workspace_bytes(C.byref(pp))
    need = -(-per // 4096) * 4096 * n_streams          # n_streams slices of the pair's workspace, each rounded up to 4 KiB (include/convexadam_hip.h)
    check_workspace(L, need, lambda ws, n: L.cvx_register_pairs_f32(3, C.cast(fix, C.c_void_p), C.cast(mov, C.c_void_p), None, None, C.byref(pp),
                                                                  C.cast(dst, C.c_void_p), None, ws, n, n_streams, stream()), outs)
