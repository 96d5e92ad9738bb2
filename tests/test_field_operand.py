"""CPU checks of _lib.field_operand, the one reading of a displacement-field argument that fieldops.py, geometry.py, affine.py and
cropfield.py share: layout, strides, element type and every refusal.  Metadata only -- no library, no device."""
import pytest
import torch

from convexadam_amd._lib import field_operand

GRID = (5, 4, 7)
V = 5 * 4 * 7


def test_both_layouts_with_and_without_a_grid():
    inter, planar = torch.zeros(GRID + (3,)), torch.zeros((3,) + GRID)
    for grid in (None, GRID, list(GRID), torch.Size(GRID)):
        t, shape, cs, vs, f64 = field_operand(inter, grid)
        assert (t.data_ptr(), shape, cs, vs, f64) == (inter.data_ptr(), GRID, 1, 3, 0)
        t, shape, cs, vs, f64 = field_operand(planar, grid)
        assert (t.data_ptr(), shape, cs, vs, f64) == (planar.data_ptr(), GRID, V, 1, 0)
    for strict in (False, True):
        assert field_operand(inter, strict=strict)[1:4] == (GRID, 1, 3)
        assert field_operand(planar, strict=strict)[1:4] == (GRID, V, 1)


def test_the_ambiguous_shape():
    t = torch.zeros((3, 3, 3, 3))
    assert field_operand(t)[1:4] == ((3, 3, 3), 1, 3)                    # as convex_adam_pt returns it: (H, W, D, 3)
    assert field_operand(t, (3, 3, 3))[1:4] == ((3, 3, 3), 1, 3)
    assert field_operand(t, (3, 3, 3), strict=True)[1:4] == ((3, 3, 3), 1, 3)
    assert field_operand(t, (3, 3, 3), planar=True)[1:4] == ((3, 3, 3), 27, 1)
    assert field_operand(t, (3, 3, 3), planar=False)[1:4] == ((3, 3, 3), 1, 3)
    with pytest.raises(ValueError, match=r"a field of shape \(3, 3, 3, 3\) does not say which of its layouts it is: pass field_grid"):
        field_operand(t, strict=True)


@pytest.mark.parametrize("dtype, want, f64", [(torch.int32, torch.float64, 1), (torch.float16, torch.float64, 1), (torch.uint8, torch.float64, 1),
                                              (torch.float32, torch.float32, 0), (torch.float64, torch.float64, 1)])
def test_element_types(dtype, want, f64):
    src = (torch.arange(3 * V) % 50).reshape((3,) + GRID).to(dtype)
    t, _, _, _, flag = field_operand(src)
    assert t.dtype == want and flag == f64 and torch.equal(t, src.to(want))
    assert (t.data_ptr() == src.data_ptr()) == (dtype == want)           # float32 and float64 are read in place
    t32, _, _, _, flag = field_operand(src, f32=True)                    # cropfield's rule
    assert t32.dtype == torch.float32 and flag == 0 and torch.equal(t32, src.to(torch.float32))


def test_a_view_is_made_contiguous_and_keeps_its_values():
    base = torch.arange(3 * V, dtype=torch.float32).reshape((3,) + GRID)
    view = base.permute(1, 2, 3, 0)                                      # (H, W, D, 3), strides of the planar tensor
    assert not view.is_contiguous()
    t, shape, cs, vs, _ = field_operand(view, GRID)
    assert t.is_contiguous() and (shape, cs, vs) == (GRID, 1, 3) and torch.equal(t, view)
    t, shape, cs, vs, _ = field_operand(base[:, ::2])
    assert t.is_contiguous() and (shape, cs, vs) == ((3, 4, 7), 84, 1) and torch.equal(t, base[:, ::2])
    grad = torch.zeros(GRID + (3,), requires_grad=True)
    assert not field_operand(grad)[0].requires_grad


def test_refusals():
    with pytest.raises(ValueError, match=r"^disp must be \(H, W, D, 3\) or \(3, H, W, D\), got \(5, 4, 7\)$"):
        field_operand(torch.zeros(GRID), name="disp")
    with pytest.raises(ValueError, match=r"^first must be \(H, W, D, 3\) or \(3, H, W, D\), got \(2, 5, 4, 7\)$"):
        field_operand(torch.zeros((2,) + GRID), name="first")
    with pytest.raises(ValueError, match=r"^field must be \(H, W, D, 3\) or \(3, H, W, D\), got \(1, 3, 5, 4, 7\)$"):
        field_operand(torch.zeros((1, 3) + GRID), GRID, strict=True)
    with pytest.raises(ValueError, match=r"^a field of shape \(2, 5, 4, 7\) does not say which of its layouts it is: pass field_grid$"):
        field_operand(torch.zeros((2,) + GRID), strict=True)
    on_grid = r"^field must be \(H, W, D, 3\) or \(3, H, W, D\) on the grid \(z, y, x\) = \(5, 4, 7\), got %s$"
    with pytest.raises(ValueError, match=on_grid % r"\(5, 4, 8, 3\)"):
        field_operand(torch.zeros((5, 4, 8, 3)), GRID)
    with pytest.raises(ValueError, match=on_grid % r"\(3, 7, 4, 5\)"):
        field_operand(torch.zeros((3, 7, 4, 5)), GRID, strict=True)
    with pytest.raises(ValueError, match=on_grid % r"\(1, 3, 5, 4, 7\)"):
        field_operand(torch.zeros((1, 3) + GRID), GRID)
    with pytest.raises(ValueError, match=on_grid % r"\(3, 5, 4, 7\)"):
        field_operand(torch.zeros((3,) + GRID), GRID, planar=False)
    with pytest.raises(ValueError, match=on_grid % r"\(5, 4, 7, 3\)"):
        field_operand(torch.zeros(GRID + (3,)), GRID, planar=True)
