"""tests/golden/curious.npz (the reference's CuRIOUS script functions on the CPU, make_golden_curious.py) against the oracle's operators
composed the way the script composes them: correlate -> ssd * mask -> coupled_convex (seeded by the argmin of the UNMASKED volume) in both
directions -> inverse_consistency on (disp_soft / scale).flip(1) -> .flip(1) * scale * grid_sp -> trilinear up-sampling.  Bit for bit;
this is the statement the GPU tests lean on when they compare the library with the oracle on ssd * mask.  No GPU."""
import numpy as np


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def test_oracle_composition_reproduces_the_curious_golden(golden, orc):
    G = golden("curious")
    hw, g, it = int(G["disp_hw"]), int(G["grid_sp"]), int(G["ic_iters"])
    shape = tuple(int(s) for s in G["shape"])
    mesh = orc.disp_mesh(hw)
    assert 0.25 < G["mask_fix"].mean() < 0.75 and 0.25 < G["mask_mov"].mean() < 0.75

    def direction(a, b, m):
        ssd, am = orc.correlate(a, b, hw)
        plain = orc.coupled_convex(ssd, am, mesh, hw)
        return orc.coupled_convex(ssd * m[None].astype(np.float32), am, mesh, hw), plain

    s1, plain = direction(G["feat_fix"], G["feat_mov"], G["mask_fix"])
    s2, _ = direction(G["feat_mov"], G["feat_fix"], G["mask_mov"])
    assert np.array_equal(bits(plain), bits(G["soft_fwd_plain"]))
    assert np.array_equal(bits(s1), bits(G["soft_fwd"])) and np.array_equal(bits(s2), bits(G["soft_rev"]))
    assert not np.array_equal(G["soft_fwd"], G["soft_fwd_plain"]), "the fixture would pass with the mask ignored"
    scale = (np.array(s1.shape[1:], np.float32) - 1).reshape(3, 1, 1, 1) / np.float32(2)
    ice, _ = orc.inverse_consistency((s1 / scale)[::-1], (s2 / scale)[::-1], it)
    assert np.array_equal(bits(ice), bits(G["disp_ice"]))
    coarse = ice[::-1] * scale * np.float32(g)
    assert np.array_equal(bits(coarse), bits(G["coarse"])) and np.abs(coarse).max() > 0
    hr = orc.resize_trilinear(coarse, shape)
    assert np.array_equal(bits(hr[:, ::3]), bits(G["disp_hr_z3"]))
    assert int(bits(hr).astype(np.int64).sum()) == int(G["disp_hr_bitsum"])
