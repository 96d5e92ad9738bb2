"""The cost volumes of tests/coupled_range_cases.py on the CPU: the table is the one it claims to be, the reference alone meets the conditions
the cases are there for, and the oracle's coupled_convex equals the reference's on every case and both seeds -- against its captures
(tests/golden/coupled_range.npz, made by tests/golden/make_golden_coupled_range.py) everywhere, live against the upstream function where
its tree is present (skipped elsewhere), and against a plain torch composition written from the operator's definition everywhere.  Never
part of the `-m gpu` selection.

What the reference does at the edges: nothing special.  torch.argmin returns the first NaN of a column, otherwise the
first minimum under `<`; -Inf + penalty = -Inf, so the first -Inf of a column wins every pass whatever the penalty, a column with a NaN
keeps its first NaN, and a cost beyond +-2^24 absorbs the penalty in its rounding: where every coupled cost of a column rounds to the same
value index 0 wins.  Nothing overflows inside the passes (the penalty is at most 3 (2 hw)^2), so a bound B - smin = +Inf exists only
in a branch-and-bound restatement, not upstream."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import coupled_range_cases as CC  # noqa: E402

SMALL = [c for c in CC.CASES if not c.large]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def torch_passes(c, which, costs_of_pass=None):
    """The operator in plain torch float32 on the CPU, from its definition: u = 3^3 box mean (zero padding, / 27) of the winners'
    displacements, then six passes winner = argmin_k(cost[k] + coef |mesh[k] - u|^2), u = box mean of the new winners' displacements.
    -> (first smoothing step [3, h, w, d], the six passes' winners [6, h, w, d], final field, the float32 coupled costs [K, v] and
    u [3, v] of pass `costs_of_pass` or None)"""
    from oracle import oracle
    cost = torch.from_numpy(np.array(c.seen())).reshape(c.K, -1)
    mesh = torch.from_numpy(oracle.disp_mesh(c.hw))

    def box_mean(winners):
        return F.avg_pool3d(mesh[:, winners.reshape(-1)].reshape((1, 3) + c.shape), 3, padding=1, stride=1)[0]

    u = first = box_mean(torch.from_numpy(np.array(c.seed(which))))
    winners, kept = [], None
    for j, coef in enumerate(torch.tensor(CC.COEFFS)):
        coupled = cost + coef * (mesh.reshape(3, c.K, 1) - u.reshape(3, 1, -1)).pow(2).sum(0)
        if j == costs_of_pass:
            kept = coupled.numpy(), u.reshape(3, -1).numpy()
        winners.append(torch.argmin(coupled, 0))
        u = box_mean(winners[-1])
    return first.numpy(), torch.stack(winners).reshape((6,) + c.shape).numpy(), u.numpy(), kept


@pytest.fixture(scope="module")
def fields(orc):
    """(case name, seed) -> the oracle's field, computed once and left unchanged"""
    out = {}
    for c in CC.CASES:
        for which in CC.SEEDS:
            f = orc.coupled_convex(np.array(c.seen()), np.array(c.seed(which)), orc.disp_mesh(c.hw), c.hw)
            f.setflags(write=False)
            out[c.name, which] = f
    return out


@pytest.fixture(scope="module")
def passes():
    """(case name, seed) -> torch_passes(...)[:3], computed once"""
    return {(c.name, which): torch_passes(c, which)[:3] for c in CC.CASES for which in CC.SEEDS}


# ---- the table is the one the issue asks for ------------------------------------------------------------------------------------------------
def test_the_list_is_the_matrix_of_the_issue():
    assert len(set(CC.NAMES)) == len(CC.NAMES)
    assert [(s, hw) for s, hw, _ in CC.GEOMETRIES] == [((5, 6, 7), 2), ((4, 6, 8), 2), ((5, 6, 7), 1), ((4, 5, 6), 4)] and CC.LARGE[:2] == ((16, 20, 16), 2)
    assert (5 * 6 * 7) % 4 != 0 and (4 * 6 * 8) % 4 == 0 and (4 * 5 * 6) % 4 == 0 and 9 ** 3 > 2 * 256
    # every displacement its own slice at 27 and 125 displacements; slices of two at 16x20x16 -- and at 4x5x6, hw 4, whose 729 displacements
    # exceed the 512 slices a single block of columns is cut into
    assert [CC.k_slices(np.prod(s), (2 * hw + 1) ** 3)[0] for s, hw, _ in CC.GEOMETRIES] == [1, 1, 1, 2]
    assert CC.k_slices(np.prod(CC.LARGE[0]), 125)[0] >= 2
    assert CC.k_slices(210, 125, aligned=False) == (1, 125) and CC.k_slices(30784, 729) == (43, 17)          # (the benchmark pair: 31 blocks, 17 slices of 43)
    kinds = ["noise@2^%d" % e for e in (-140, -126, -100, -30, 10, 17, 24, 60, 100, 127)] + ["realmin@2^%d" % e for e in (-100, 14, 40, 120)] + \
        ["2^14+r", "2^17+64r", "-2^17+8r", "2^24+r", "2^30+r", "-2^30+r"] + ["%s@2^%d" % (k, e) for k in ("signed", "negative") for e in (0, 20, 100)] + \
        ["wide@1e30", "3e38_and_-3e38", "neginf_scattered10", "neginf_scattered40", "neginf_columns", "neginf_with_posinf", "neginf_with_nan",
         "neginf_plane", "zeros_late_negative", "zeros_everywhere"] + ["masked:" + k for k in CC.MASKED_KINDS]
    assert len(kinds) == 39
    for shape, hw, _ in CC.GEOMETRIES:
        assert [c.kind for c in CC.CASES if (c.shape, c.hw) == (shape, hw)] and \
            sorted(c.kind for c in CC.CASES if (c.shape, c.hw) == (shape, hw)) == sorted(kinds), (shape, hw)
    assert sorted(c.kind for c in CC.CASES if c.large) == sorted(["noise@2^17", "noise@2^127", "realmin@2^14", "2^14+r", "signed@2^20"])
    assert len(CC.CASES) == 4 * 39 + 5
    count = {cls: sum(c.cls == cls for c in SMALL) // 4 for cls in CC.CLASSES}
    assert count == {"scaled_noise": 10, "real_minimum": 4, "offset_spread": 4, "absorbed": 2, "signed": 6, "wide_spread": 1, "overflow_bound": 1,
                     "neg_inf": 6, "signed_zeros": 2, "masked": 3}
    assert {c.cls for c in CC.CASES if c.large} == {"scaled_noise", "real_minimum", "offset_spread", "signed"}


def test_the_volumes_are_what_their_names_claim():
    f32 = np.finfo(np.float32)
    for c in CC.CASES:
        ssd, seen = c.ssd(), c.seen()
        K = c.K
        assert ssd.shape == (K,) + c.shape and ssd.dtype == np.float32 and ssd.flags.c_contiguous and not ssd.flags.writeable, c.name
        assert (c.mask is not None) == (c.cls == "masked") == c.masked, c.name
        kind = c.kind
        col = seen.reshape(K, -1)
        true, foreign = c.seed("true").reshape(-1), c.seed("foreign").reshape(-1)
        assert true.dtype == foreign.dtype == np.int64 and 0 <= foreign.min() and foreign.max() < K and (foreign != true).mean() > 0.9, c.name
        # torch.argmin itself on the values the passes see
        assert np.array_equal(true, torch.argmin(torch.from_numpy(np.array(col)), 0).numpy()), c.name
        if c.cls in ("scaled_noise", "real_minimum", "offset_spread", "absorbed", "signed", "wide_spread", "overflow_bound"):
            assert np.isfinite(ssd).all(), c.name
        if kind == "noise@2^-140":
            assert (np.abs(ssd) < f32.tiny).all() and (ssd != 0).mean() > 0.99, c.name                 # all entries denormal
        if kind == "noise@2^127":
            assert ssd.max() > 2.0 ** 126 and np.isfinite(ssd.max()), c.name
        if kind.startswith("noise@"):
            e = int(kind.split("^")[1])
            assert (ssd >= 0).all() and 2.0 ** (e - 1) < ssd.max() <= 2.0 ** e, c.name          # (= 2^e only where a denormal rounds up to it)
        if kind.startswith("realmin@"):
            base = CC.realmin_base(c.shape, c.hw).astype(np.float64)
            assert np.array_equal(ssd.astype(np.float64), base * 2.0 ** int(kind.split("^")[1])), c.name    # an exact multiple
        if kind == "2^24+r":
            assert set(np.unique(ssd)) == {np.float32(2.0 ** 24), np.float32(2.0 ** 24 + 1)}, c.name       # (2^24 + r rounds to 2^24 + 1 never to + 2)
        if c.cls == "absorbed":
            assert (np.abs(ssd) == np.float32(2.0 ** 30)).all() and len(np.unique(ssd)) == 1, c.name
        if kind.startswith("signed@") or kind == "wide@1e30":
            assert 0.4 < (ssd < 0).mean() < 0.6, c.name
        if kind.startswith("negative@"):
            assert (ssd <= 0).all() and (ssd < 0).mean() > 0.99, c.name
        if kind == "wide@1e30":
            a = np.abs(ssd.reshape(K, -1).astype(np.float64))
            assert (np.log10(a.max(0) / a.min(0)) > 40).all(), c.name
        if c.cls == "overflow_bound":
            both = (col == np.float32(3e38)).any(0) & (col == np.float32(-3e38)).any(0)
            assert 0.3 < both.mean() < 0.7, c.name
            with np.errstate(over="ignore"):
                assert np.isposinf(np.float32(3e38) - col.min(0)[both]).all(), c.name                     # B - smin = +Inf in float32
        if c.cls == "neg_inf":
            assert np.isneginf(ssd).any() and bool(np.isnan(ssd).any()) == (kind == "neginf_with_nan"), c.name
        if kind in ("neginf_scattered10", "neginf_scattered40"):
            share = float(kind[-2:]) / 100
            assert abs(np.isneginf(ssd).mean() - share) < 0.02, c.name
        if kind in CC.WHOLE_NEGINF_COLUMNS:
            whole = np.isneginf(col).all(0).reshape(c.shape)
            assert whole.sum() == (len(set(CC.marked_columns(c.shape))) if kind == "neginf_columns" else c.shape[0] * c.shape[2]), c.name
            if kind == "neginf_columns":                  # interior, faces and corners
                h, w, d = c.shape
                assert whole[1:-1, 1:-1, 1:-1].any() and whole[0, 1:-1, 1:-1].any() and whole[0, 0, 0] and whole[-1, -1, -1], c.name
        if kind == "neginf_with_posinf":
            shared = np.isneginf(col).any(0) & np.isposinf(col).any(0)
            first_neg, first_pos = np.isneginf(col).argmax(0)[shared], np.isposinf(col).argmax(0)[shared]
            assert shared.sum() == len(set(CC.marked_columns(c.shape))) and (first_neg < first_pos).any() and (first_neg > first_pos).any(), c.name
        if kind == "neginf_with_nan":
            shared = np.isneginf(col).any(0) & np.isnan(col).any(0)
            first_neg, first_nan = np.isneginf(col).argmax(0)[shared], np.isnan(col).argmax(0)[shared]
            assert shared.sum() == len(set(CC.marked_columns(c.shape))) == np.isnan(col).sum(), c.name
            assert (first_nan < first_neg).any() and (first_nan > first_neg).any() and np.array_equal(true[shared], first_nan), c.name
        if c.cls == "signed_zeros":
            zero = (col == 0).all(0)
            neg = np.signbit(col) & zero[None]
            allneg = neg.all(0)
            assert allneg.sum() == 1 and zero.sum() >= (col.shape[1] if kind == "zeros_everywhere" else 0.15 * col.shape[1]), c.name
            mixed = zero & ~allneg
            assert neg[:, mixed].any(0).all() and not neg[0, mixed].any() and (true[zero] == 0).all(), c.name   # -0.0 only behind the first +0.0
        if c.masked:
            out = c.mask.reshape(-1) == 0
            assert 0.45 < 1 - out.mean() < 0.75 and out.sum() >= 3, c.name
            poison = ssd.reshape(K, -1)[:, out]
            assert np.isnan(poison[:, 0::3]).all() and np.isneginf(poison[:, 1::3]).all() and (poison[:, 2::3] == np.float32(3e38)).all(), c.name
            assert (col[:, out] == 0).all() and not np.signbit(col[:, out]).any() and np.array_equal(col[:, ~out], ssd.reshape(K, -1)[:, ~out], equal_nan=True), c.name
        if c.half_ok():
            assert same(CC.widen(ssd), np.array(ssd)) and np.array_equal(np.signbit(CC.widen(ssd)), np.signbit(ssd)), c.name
    halves = {c.kind for c in CC.CASES if c.half_ok()}
    assert halves == {"signed@2^0", "negative@2^0", "zeros_late_negative", "zeros_everywhere"} | {k for k, cls, _ in CC.KINDS if cls == "neg_inf"}


# ---- the conditions the cases are there for, on the reference alone ---------------------------------------------------------------------------
def pass_one_shares(c, which):
    """(share of columns with two or more displacements tied at the float32 minimum of pass 1, share of columns whose first-index float32
    winner is not the argmin of the same expression in float64)"""
    from oracle import oracle
    (coupled, u), mesh = torch_passes(c, which, costs_of_pass=0)[3], oracle.disp_mesh(c.hw).astype(np.float64)
    q = ((mesh[:, :, None] - u.astype(np.float64)[:, None, :]) ** 2).sum(0)
    exact = c.seen().reshape(c.K, -1).astype(np.float64) + float(np.float32(CC.COEFFS[0])) * q
    return float(((coupled == coupled.min(0)).sum(0) >= 2).mean()), float((coupled.argmin(0) != exact.argmin(0)).mean())


@pytest.mark.parametrize("kind", CC.TIE_KINDS)
def test_rounding_creates_ties_and_moves_winners_in_pass_one(kind):
    """Pass 1 (coef 0.003) of the reference, at every geometry: in at least 1 % of the columns two or more displacements tie at the float32
    minimum, and in at least 1 % the first-index float32 winner is not the argmin of the same expression in float64.  Held on the FOREIGN
    seed -- u is then a random point of the 1/27 lattice, the setting of the model that proposed the volumes.  The true seed's shares are
    printed beside them and DESIGN 40 lists both: they are of the same size, but a geometry has 120 to 210 columns, 1 % of them is one or
    two, and one cell (2^14+r at 4x5x6-hw4: 4 of 120 columns tied, no winner moved) falls below it; other spreads of the family only move
    that cell elsewhere (2^14 + r/2 under its own seed: 2 of 210 at 5x6x7-hw1), so the volumes stay as proposed."""
    n = 0
    for c in CC.CASES:
        if c.kind == kind:
            tied, moved = pass_one_shares(c, "foreign")
            print("%s: foreign seed tied %.4f, moved %.4f; true seed tied %.4f, moved %.4f" % ((c.name, tied, moved) + pass_one_shares(c, "true")))
            assert tied >= 0.01 and moved >= 0.01, (c.name, tied, moved)
            n += 1
    assert n == len(CC.GEOMETRIES) + (kind in CC.LARGE_KINDS)


def test_absorbed_penalty_leaves_index_zero(passes):
    for c in CC.CASES:
        if c.cls == "absorbed":
            for which in CC.SEEDS:
                assert (passes[c.name, which][1] == 0).all(), (c.name, which)


def test_the_passes_move_a_real_minimum(passes):
    """The final field differs from the first smoothing step at more than half of the voxels: on the foreign seed at every scale, on the true
    seed where the penalty can compete with the cost differences (2^-100).  From 2^14 up the true seed is a fixed point of the passes --
    a cost gap of 2^14 * 0.01 against a penalty of at most 3 (2 hw)^2 -- which is the reference's behaviour, and is held here too."""
    for c in CC.CASES:
        if c.cls == "real_minimum":
            first, winners, final = passes[c.name, "foreign"]
            assert float((first != final).any(0).mean()) > 0.5 and float((winners[-1] != c.seed("foreign")).mean()) > 0.5, c.name
            first, winners, final = passes[c.name, "true"]
            if c.kind == "realmin@2^-100":
                assert float((first != final).any(0).mean()) > 0.5 and float((winners[-1] != c.seed("true")).mean()) > 0.5, c.name
            else:
                assert float((winners[-1] != c.seed("true")).mean()) < 0.01, c.name


def test_a_whole_neginf_column_keeps_its_first_entry(passes):
    n = 0
    for c in CC.CASES:
        if c.kind in CC.WHOLE_NEGINF_COLUMNS:
            whole = np.isneginf(c.seen()).all(0)
            for which in CC.SEEDS:
                assert (passes[c.name, which][1][:, whole] == 0).all(), (c.name, which)
                n += 1
        if c.kind == "neginf_with_posinf":                   # (more than the issue asks: the first -Inf of a mixed column wins as well)
            col = np.isneginf(c.seen()).reshape(c.K, -1)
            has = col.any(0).reshape(c.shape)
            for which in CC.SEEDS:
                assert np.array_equal(passes[c.name, which][1][:, has], np.broadcast_to(col.argmax(0).reshape(c.shape)[has], (6, int(has.sum())))), c.name
    assert n == 2 * 2 * len(CC.GEOMETRIES)


# ---- the oracle against the reference ---------------------------------------------------------------------------------------------------------
def test_oracle_equals_the_torch_composition(fields, passes):
    bad = [(c.name, which) for c in CC.CASES for which in CC.SEEDS if not same(np.array(fields[c.name, which]), passes[c.name, which][2])]
    assert not bad, bad


def test_oracle_equals_the_captures(golden, fields):
    ref = golden("coupled_range")
    want = {"%s:%s" % (c.name, which) for c in CC.CASES for which in CC.SEEDS}
    assert set(ref) == want, "tests/golden/coupled_range.npz was made for another list: run make_golden_coupled_range.py"   # (the large geometry included)
    bad = [key for key in sorted(ref) if not same(ref[key], np.array(fields[tuple(key.rsplit(":", 1))]))]
    assert not bad, bad
    assert all(v.dtype == np.float32 and v.ndim == 4 and v.shape[0] == 3 for v in ref.values())         # recorded outputs only
    assert os.path.getsize(os.path.join(HERE, "golden", "coupled_range.npz")) < os.path.getsize(os.path.join(HERE, "golden", "mind_range.npz"))


@pytest.fixture(scope="module")
def upstream():
    try:
        from _ref_import import import_reference, reference_available
    except ImportError:
        pytest.skip("the import harness of the upstream reference is not on this host")
    if not reference_available():
        pytest.skip("the upstream reference tree is not on this host")
    # the repository's own `convexAdam` package (the drop-in front end of the device operators) may be imported already: the reference's
    # package of the same name is imported in its place and both the module table and the path are put back
    # the harness also stands empty `nibabel` / `SimpleITK` modules in for the ones the reference only names: they are taken out again, so
    # that a later test's `import nibabel` finds what this host really has (this file runs before tests/test_host_logic.py)
    mine = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "convexAdam" or k.startswith("convexAdam.")}
    stubs = {m: sys.modules.get(m) for m in ("nibabel", "SimpleITK")}
    path = list(sys.path)
    try:
        utils = import_reference()[0]
        assert not utils.__file__.startswith(os.path.dirname(HERE)), utils.__file__
    finally:
        for k in [k for k in sys.modules if k == "convexAdam" or k.startswith("convexAdam.")]:
            del sys.modules[k]
        sys.modules.update(mine)
        for m, was in stubs.items():
            if was is None:
                sys.modules.pop(m, None)
            else:
                sys.modules[m] = was
        sys.path[:] = path
    return utils.coupled_convex


def test_oracle_equals_the_live_reference(upstream, fields):
    from make_golden_coupled_range import reference_field
    bad = [(c.name, which) for c in CC.CASES for which in CC.SEEDS if not same(reference_field(upstream, c, which), np.array(fields[c.name, which]))]
    assert not bad, bad
