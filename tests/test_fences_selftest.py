"""CPU: tests/fences.py can fail.  Fake operators, written with torch ops on the fenced views, that misbehave in the four ways the fence
exists for are each reported by check_fences; the well-behaved one is not.  Without this a green tests/test_gpu_fences.py proves nothing.

The fake operators reach outside their operand through the view's storage, as a kernel does through its pointer.  On a plain allocation
(storage offset 0, nothing behind the last element) the stray access has nowhere to go and is skipped: there it would land in the
allocator's slack, which is exactly why the plain run cannot see it.

The second half does the same for fenced(.., shift=) and check_unaligned(): a shifted payload sits where it should, the moat checks still
catch a store one element before and one element behind it, and a refusal is accepted only from an operator with the right to refuse.
(check_side_stream needs a device: tests/test_gpu_placement_selftest.py.)"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fences  # noqa: E402
from fences import IN, INOUT, OUT, SCRATCH, check_fences, check_unaligned, fenced  # noqa: E402

DEV = "cpu"


def outside(t, k):
    """The element k places after the view's last one (k >= 1) or -k places before its first (k <= -1), or None on a plain allocation."""
    off = t.storage_offset() + (t.numel() - 1 + k if k > 0 else k)
    room = t.untyped_storage().nbytes() // t.element_size()
    if t.storage_offset() == 0 or not 0 <= off < room:
        return None
    return torch.as_strided(t, (1,), (1,), off)


def op_good(t):
    t["y"].copy_(2 * t["x"] + t["idx"].to(torch.float32))
    t["state"].add_(1)
    t["ws"].fill_(7)


def op_store_before(t):
    op_good(t)
    e = outside(t["y"], -1)
    if e is not None:
        e.fill_(1.0)


def op_store_after(t):
    op_good(t)
    e = outside(t["y"], 1)
    if e is not None:
        e.fill_(1.0)


def op_read_past_input(t):
    op_good(t)
    e = outside(t["x"], 1)
    if e is not None:
        t["y"].view(-1)[-1:] += 0 * e          # a tap with a zero weight


def operands():
    g = torch.Generator().manual_seed(3)
    x = torch.rand((3, 5, 7), generator=g)
    idx = torch.randint(0, 4, (3, 5, 7), generator=g, dtype=torch.int32)
    return {"x": IN(x), "idx": IN(idx, loud=3), "y": OUT((3, 5, 7)), "state": INOUT(torch.rand((3, 5, 7), generator=g)), "ws": SCRATCH(100)}


def op_skips_one(t):
    good = 2 * t["x"] + t["idx"].to(torch.float32)
    y = t["y"].view(-1)
    y[:5] = good.view(-1)[:5]
    y[6:] = good.view(-1)[6:]                   # element 5 keeps what the buffer held
    t["state"].add_(1)


def op_store_before_inout(t):
    op_good(t)
    e = outside(t["state"], -1)
    if e is not None:
        e.fill_(0.0)


def op_writes_input(t):
    op_good(t)
    t["x"].view(-1)[0] = 0.5


def test_layout():
    v = fenced((3, 5, 7), torch.float32, DEV, float("nan"))
    f = v.fence
    assert v.shape == (3, 5, 7) and v.is_contiguous()
    assert f.lo % 256 == 0 and f.lo >= 64 * 1024 and f.raw.numel() == 2 * f.lo + 512 and f.nbytes == 420
    assert (v.data_ptr() - f.raw.data_ptr()) == f.lo
    whole = f.raw.view(torch.float32)
    assert bool(torch.isnan(whole[:f.lo // 4]).all()) and bool(torch.isnan(whole[(f.lo + 420) // 4:]).all())
    big = fenced((2, 300, 300), torch.float32, DEV, 0)
    assert big.fence.lo == 4 * 300 * 300 * 4 and big.fence.lo % 256 == 0          # four planes > 64 KiB
    assert fences.moat_bytes((7, 9, 11), torch.float64) == 64 * 1024
    o = fenced((10,), torch.int32, DEV, None)
    assert bool((o.fence.raw == 0xA5).all())
    lab = fenced((4, 4), torch.int64, DEV, 2)
    assert bool((lab.fence.raw.view(torch.int64)[:8] == 2).all())


def test_well_behaved_operator_passes():
    plain = check_fences(operands(), op_good, DEV)
    ops = operands()
    assert torch.equal(plain["y"], 2 * ops["x"].data + ops["idx"].data.float())


@pytest.mark.parametrize("op,needle", [
    (op_store_before, "before its payload"),
    (op_store_after, "behind its payload"),
    (op_store_before_inout, "inout operand 'state'"),
    (op_read_past_input, "loud-moat fenced run differs from the plain run in out 'y'"),
    (op_skips_one, "fenced run differs from the plain run in out 'y': first at byte 20"),
    (op_writes_input, "input 'x' was modified"),
])
def test_misbehaving_operator_is_reported(op, needle):
    with pytest.raises(AssertionError) as e:
        check_fences(operands(), op, DEV)
    assert needle in str(e.value), str(e.value)


def test_failed_call_is_reported():
    with pytest.raises(AssertionError, match="returned -2"):
        check_fences(operands(), lambda t: -2, DEV)


# ---- shifted payloads (check_unaligned) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,n", [(torch.float32, 4), (torch.float32, 12), (torch.float64, 8), (torch.int64, 24), (torch.float16, 2), (torch.float16, 18),
                                     (torch.uint8, 1), (torch.uint8, 17), (torch.float32, 0)])
def test_shifted_layout(dtype, n):
    plain = fenced((3, 5, 7), dtype, DEV, None)
    v = fenced((3, 5, 7), dtype, DEV, None, shift=n)
    f, f0 = v.fence, plain.fence
    assert v.shape == (3, 5, 7) and v.is_contiguous()
    assert f.lo == f0.lo + n and f.nbytes == f0.nbytes and (v.data_ptr() - f.raw.data_ptr()) == f.lo
    assert f.lo % 256 == n and f.lo % 16 == n % 16
    assert f.raw.numel() % 256 == 0 and f.raw.numel() - f.lo - f.nbytes >= f0.lo          # both moats as large as without the shift
    v.fill_(1)
    assert int((f.raw != 0xA5).sum()) == f.nbytes and bool((f.payload() != 0xA5).all())


def test_shifted_layout_keeps_the_typed_moat_fill():
    v = fenced((5, 3), torch.float32, DEV, float("nan"), shift=4)
    whole = v.fence.raw.view(torch.float32)
    assert bool(torch.isnan(whole).all())
    v.fill_(0.0)
    assert int((~torch.isnan(whole)).sum()) == 15
    with pytest.raises(AssertionError, match="whole elements"):
        fenced((5, 3), torch.float32, DEV, 0, shift=2)
    with pytest.raises(AssertionError, match="whole elements"):
        fenced((5, 3), torch.uint8, DEV, 0, shift=256)


ALL = ("x", "idx", "y", "state")


def test_well_behaved_operator_passes_unaligned():
    for which in (ALL, ("x",), ("y",), ("state",), ()):
        ts, how = check_unaligned(operands(), op_good, DEV, which)
        assert how == "ran"
        for k in ALL:
            assert ts[k].fence.lo % 256 == (4 if k in which else 0)


@pytest.mark.parametrize("op,which,needle", [
    (op_store_before, ALL, "of out operand 'y' changed, the first 4 byte(s) before its payload"),
    (op_store_after, ALL, "of out operand 'y' changed, the first 1 byte(s) behind its payload"),
    (op_store_before, ("y",), "before its payload"),
    (op_store_before_inout, ALL, "inout operand 'state'"),
    (op_read_past_input, ALL, "differs from the aligned plain run in out 'y'"),
    (op_skips_one, ALL, "differs from the aligned plain run in out 'y': first at byte 20"),
    (op_writes_input, ALL, "input 'x' was modified"),
])
def test_misbehaving_operator_is_reported_unaligned(op, which, needle):
    with pytest.raises(AssertionError) as e:
        check_unaligned(operands(), op, DEV, which)
    assert needle in str(e.value), str(e.value)


def op_takes_a_wide_path_blindly(t):
    """what an unguarded 16-byte kernel does to a misaligned output in the worst case: it rounds the address down"""
    op_good(t)
    if t["y"].data_ptr() % 16:
        e = outside(t["y"], -1)
        if e is not None:
            e.copy_(t["y"].view(-1)[:1])


def test_rounded_down_address_is_reported():
    check_fences(operands(), op_takes_a_wide_path_blindly, DEV)                 # aligned payloads: nothing to see
    with pytest.raises(AssertionError, match="before its payload"):
        check_unaligned(operands(), op_takes_a_wide_path_blindly, DEV, ("y",))


def test_refusal_is_accepted_only_with_the_right_to_refuse():
    def refuses(t):
        return -1 if t["x"].data_ptr() % 16 else (op_good(t) or 0)
    with pytest.raises(AssertionError, match="the call returned -1"):
        check_unaligned(operands(), refuses, DEV, ALL)
    ts, how = check_unaligned(operands(), refuses, DEV, ALL, refusal=(-1, lambda: "x is not aligned to 16 bytes"))
    assert how == "refused"
    with pytest.raises(AssertionError, match="does not name the alignment"):
        check_unaligned(operands(), refuses, DEV, ALL, refusal=(-1, lambda: "bad argument"))

    def refuses_late(t):
        op_good(t)
        return -1 if t["x"].data_ptr() % 16 else 0
    with pytest.raises(AssertionError, match="a refused call wrote output 'y'"):
        check_unaligned(operands(), refuses_late, DEV, ALL, refusal=(-1, lambda: "not aligned"))


def test_scratch_is_never_shifted():
    with pytest.raises(AssertionError, match="never shifted"):
        check_unaligned(operands(), op_good, DEV, ("ws",))
