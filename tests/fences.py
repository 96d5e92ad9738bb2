"""Fences for operator tests: every operand of a call sits between two moats, and the call is run three ways.

A plain module that test files import (like geometry_restatement.py).  It works on any torch device: tests/test_fences_selftest.py runs it
on the CPU with fake operators, tests/test_gpu_fences.py on the HIP kernels.

fenced(shape, dtype, device, moat_fill) makes ONE uint8 allocation [moat | payload rounded up to 256 bytes | moat] and returns a view of
the payload.  MOAT is a multiple of 256 bytes (the payload keeps the alignment of a fresh allocation), at least 64 KiB and at least four
planes of the operand's slowest axis, so that every byte a misbehaving kernel could plausibly touch belongs to the test.

  inputs      moat = the LOUD fill (quiet NaN for floating types; for integer types a valid value of the operand that differs from the
              quiet one, chosen by the caller -- never an out-of-range index) or the QUIET fill (zeros)
  outputs,    moats AND payload start as 0xA5 bytes
  in/out      moats 0xA5, payload = the caller's data
  scratch     like an output; only its moats are checked (a workspace's contents are the kernel's business)

check_fences() runs one call (a) on plain allocations, (b) fenced with loud input moats, (c) fenced with quiet input moats, and asserts
  * every moat byte of every operand is intact after (b) and (c)           -- a store outside an output, or any store next to an input
  * output payloads of (b), (c) and (a) are byte-identical                   -- a read outside an input that reaches arithmetic (0 * NaN),
                                                                                and an element the call leaves unwritten ((a)'s outputs
                                                                                start as 0x3C bytes, the fenced ones as 0xA5)
  * input payloads are unchanged.
What it cannot see: a read outside an operand whose value never reaches arithmetic or a store (a load that is masked away afterwards)."""
import math

import torch

MOAT_MIN = 64 * 1024
ALIGN = 256
OUT_BYTE = 0xA5          # fenced outputs, in/out moats, scratch
PLAIN_OUT_BYTE = 0x3C    # outputs of the plain run: differs, so that an unwritten element shows in the comparison


def _round_up(n, a):
    return -(-n // a) * a


def moat_bytes(shape, dtype):
    item = torch.empty((), dtype=dtype).element_size()
    plane = item * int(math.prod(shape[1:])) if len(shape) > 1 else item
    return _round_up(max(MOAT_MIN, 4 * plane), ALIGN)


class Fence:
    """The allocation behind a fenced view: raw uint8 buffer, payload range [lo, lo + nbytes), and a snapshot of the initial bytes."""

    def __init__(self, raw, lo, nbytes):
        self.raw, self.lo, self.nbytes = raw, lo, nbytes
        self.initial = None

    def snapshot(self):
        self.initial = self.raw.clone()

    def moats_intact(self):
        """None, or (side, distance in bytes of the first changed moat byte from the payload, count of changed bytes)."""
        lo, hi = self.lo, self.lo + self.nbytes
        diff = self.raw != self.initial
        diff[lo:hi] = False
        n = int(diff.sum())
        if n == 0:
            return None
        first = int(diff.nonzero()[0])
        return ("before", lo - first, n) if first < lo else ("behind", first - hi + 1, n)

    def payload(self):
        return self.raw[self.lo:self.lo + self.nbytes]


def fenced(shape, dtype, device, moat_fill):
    """A contiguous view of `shape` between two moats.  moat_fill: a number of `dtype` (NaN, 0, a label ...) that fills both moats and the
    payload's rounding, or None: 0xA5 bytes everywhere, the payload included.  The Fence is the view's attribute `.fence`."""
    shape = tuple(int(s) for s in shape)
    item = torch.empty((), dtype=dtype).element_size()
    nbytes = item * int(math.prod(shape))
    moat = moat_bytes(shape, dtype)
    total = moat + _round_up(max(nbytes, 1), ALIGN) + moat
    raw = torch.empty(total, dtype=torch.uint8, device=device)
    assert raw.data_ptr() % ALIGN == 0 or raw.device.type == "cpu", "a fresh allocation is expected to be 256-byte aligned"
    if moat_fill is None:
        raw.fill_(OUT_BYTE)
    elif dtype == torch.uint8:
        raw.fill_(int(moat_fill))
    else:
        raw.view(dtype).fill_(moat_fill)
    view = raw[moat:moat + nbytes].view(dtype).view(shape)
    view.fence = Fence(raw, moat, nbytes)
    return view


class Operand:
    """kind: 'in' | 'out' | 'inout' | 'scratch'.  data: the tensor (in, inout) or None; shape / dtype for out and scratch.
    loud: the loud moat value of an integer input (floating inputs get NaN)."""

    def __init__(self, kind, data=None, shape=None, dtype=None, loud=None):
        assert kind in ("in", "out", "inout", "scratch")
        self.kind, self.data, self.loud = kind, data, loud
        self.shape = tuple(data.shape) if data is not None else tuple(shape)
        self.dtype = data.dtype if data is not None else dtype
        if kind in ("in", "inout"):
            assert data is not None
        if kind == "in" and not self.dtype.is_floating_point:
            assert loud is not None, "an integer input needs a loud moat value that is valid for the operand"


def IN(data, loud=None):
    return Operand("in", data, loud=loud)


def OUT(shape, dtype=torch.float32):
    return Operand("out", shape=shape, dtype=dtype)


def INOUT(data):
    return Operand("inout", data)


def SCRATCH(nbytes):
    return Operand("scratch", shape=(int(nbytes),), dtype=torch.uint8)


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8)


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def _first_diff(a, b):
    d = (a != b).nonzero()
    return int(d[0]), int(d.numel())


def _plain(op, device):
    if op.kind in ("in", "inout"):
        return op.data.detach().clone().contiguous().to(device)
    t = torch.empty(op.shape, dtype=op.dtype, device=device)
    _bytes(t).fill_(PLAIN_OUT_BYTE)
    return t


def _fenced(op, device, loud):
    if op.kind == "in":
        fill = (float("nan") if op.dtype.is_floating_point else op.loud) if loud else 0
        t = fenced(op.shape, op.dtype, device, fill)
        t.copy_(op.data)
    else:
        t = fenced(op.shape, op.dtype, device, None)
        if op.kind == "inout":
            t.copy_(op.data)
    t.fence.snapshot()
    return t


def check_fences(operands, call, device):
    """operands: {name: Operand}; call(tensors: {name: tensor}) runs the operator once (return value None or 0).
    Returns the plain run's tensors, (a), for a further comparison with an oracle."""
    runs = {}
    for mode in ("plain", "loud", "quiet"):
        ts = {k: (_plain(op, device) if mode == "plain" else _fenced(op, device, mode == "loud")) for k, op in operands.items()}
        _sync(device)
        rc = call(ts)
        _sync(device)
        assert rc in (None, 0), "%s run: the call returned %r" % (mode, rc)
        runs[mode] = ts
    for mode in ("loud", "quiet"):
        for k, op in operands.items():
            hit = runs[mode][k].fence.moats_intact()
            assert hit is None, ("%s run: %d moat byte(s) of %s operand %r changed, the first %d byte(s) %s its payload"
                                 % (mode, hit[2], op.kind, k, hit[1], hit[0]))
    for k, op in operands.items():
        a = _bytes(runs["plain"][k])
        if op.kind == "in":
            want = _bytes(op.data.detach().contiguous().to(device))
            for mode in ("plain", "loud", "quiet"):
                got = _bytes(runs[mode][k])
                assert torch.equal(got, want), "%s run: input %r was modified (first at byte %d, %d bytes)" % ((mode, k) + _first_diff(got, want))
        elif op.kind in ("out", "inout"):
            for mode in ("loud", "quiet"):
                got = _bytes(runs[mode][k])
                assert torch.equal(got, a), ("%s-moat fenced run differs from the plain run in %s %r: first at byte %d of the payload, %d bytes"
                                             % ((mode, op.kind, k) + _first_diff(got, a)))
    return runs["plain"]
