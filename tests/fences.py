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
What it cannot see: a read outside an operand whose value never reaches arithmetic or a store (a load that is masked away afterwards).

Two more modes run the same (operands, call) pair where check_fences always stands on torch's default stream with 256-byte aligned payloads
(DESIGN.md section 33):
  check_side_stream()  on a fresh stream, behind a bounded delay, with operands that become valid only on that stream and snapshots taken
                       on it: work that lands on another queue, or that is never joined back, changes the snapshot
  check_unaligned()    fenced(.., shift=) puts the named payloads one element behind the boundary: the call runs with the same bits and
                       intact moats, or refuses where the header gives it the right to."""
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


def fenced(shape, dtype, device, moat_fill, shift=0):
    """A contiguous view of `shape` between two moats.  moat_fill: a number of `dtype` (NaN, 0, a label ...) that fills both moats and the
    payload's rounding, or None: 0xA5 bytes everywhere, the payload included.  The Fence is the view's attribute `.fence`.
    shift: the payload starts that many bytes behind the 256-byte boundary (a multiple of the element size, below 256); both moats keep
    at least their size."""
    shape = tuple(int(s) for s in shape)
    item = torch.empty((), dtype=dtype).element_size()
    assert 0 <= shift < ALIGN and shift % item == 0, "shift %r: whole elements, less than one boundary" % (shift,)
    nbytes = item * int(math.prod(shape))
    moat = moat_bytes(shape, dtype)
    total = moat + _round_up(max(nbytes, 1) + shift, ALIGN) + moat
    raw = torch.empty(total, dtype=torch.uint8, device=device)
    assert raw.data_ptr() % ALIGN == 0 or raw.device.type == "cpu", "a fresh allocation is expected to be 256-byte aligned"
    if moat_fill is None:
        raw.fill_(OUT_BYTE)
    elif dtype == torch.uint8:
        raw.fill_(int(moat_fill))
    else:
        raw.view(dtype).fill_(moat_fill)
    view = raw[moat + shift:moat + shift + nbytes].view(dtype).view(shape)
    view.fence = Fence(raw, moat + shift, nbytes)
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


def _fenced(op, device, loud, shift=0):
    if op.kind == "in":
        fill = (float("nan") if op.dtype.is_floating_point else op.loud) if loud else 0
        t = fenced(op.shape, op.dtype, device, fill, shift)
        t.copy_(op.data)
    else:
        t = fenced(op.shape, op.dtype, device, None, shift)
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


# ---- two more run modes: the same (operands, call) pair on a side stream behind a delay, and at unaligned addresses -------------------------
def plain_run(operands, call, device):
    """The plain run of check_fences on the current stream: (tensors, seconds the host spent inside `call`).  The reference of both modes."""
    import time
    ts = {k: _plain(op, device) for k, op in operands.items()}
    _sync(device)
    t0 = time.perf_counter()
    rc = call(ts)
    host = time.perf_counter() - t0
    _sync(device)
    assert rc in (None, 0), "plain run: the call returned %r" % (rc,)
    return ts, host


class Delay:
    """Bounded, ordinary work that keeps a stream busy: `reps` fills of one tensor of fixed size.  No kernel of it waits on anything.
    unit_ms: one fill on the device (events, median); enqueue_ms: what the host spends to enqueue one; launch_ms: host-to-completion of a
    one-element fill on an idle stream (median of 20).  floor_ms = 100 * launch_ms; a row's delay is max(floor, 3 * the host time of its
    plain call), capped at cap_ms."""
    NBYTES = 256 << 20
    CAP_MS = 200.0

    def __init__(self, device):
        import time
        self.buf = torch.empty(self.NBYTES, dtype=torch.uint8, device=device)
        self._one = one = torch.empty(1, dtype=torch.float32, device=device)
        self._apart = {}
        s = torch.cuda.Stream(device)
        with torch.cuda.stream(s):
            for _ in range(3):
                self.buf.fill_(1)
                one.fill_(1.0)
            s.synchronize()
            lat = []
            for _ in range(20):
                t0 = time.perf_counter()
                one.fill_(1.0)
                s.synchronize()
                lat.append(time.perf_counter() - t0)
            units, enq = [], []
            for _ in range(5):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                t0 = time.perf_counter()
                for _ in range(8):
                    self.buf.fill_(1)
                enq.append((time.perf_counter() - t0) / 8)
                b.record()
                s.synchronize()
                units.append(a.elapsed_time(b) / 8)
        self.launch_ms = 1e3 * sorted(lat)[len(lat) // 2]
        self.unit_ms = sorted(units)[len(units) // 2]
        self.enqueue_ms = 1e3 * sorted(enq)[len(enq) // 2]
        self.floor_ms = 100.0 * self.launch_ms
        self.cap_ms = self.CAP_MS
        # the host must enqueue fills faster than the device retires them, or no backlog ever forms in front of the call
        assert self.unit_ms > 3.0 * self.enqueue_ms, "delay unit %.3f ms is not well above its enqueue cost %.3f ms" % (self.unit_ms, self.enqueue_ms)

    def independent(self, a, b):
        """True if work on stream `b` completes while stream `a` is still held back by the delay.  Streams are dealt onto a few hardware
        queues (4 by default); two streams on one queue run in the order of their enqueues, so work misplaced from `a` onto `b` would look
        well placed.  Probed once per pair of streams with one floor's worth of delay; nothing here waits longer than that delay runs."""
        key = (a.cuda_stream, b.cuda_stream)
        if key not in self._apart:
            torch.cuda.synchronize()
            held, done = torch.cuda.Event(), torch.cuda.Event()
            with torch.cuda.stream(a):
                self.enqueue(self.floor_ms)
                held.record()
            with torch.cuda.stream(b):
                self._one.fill_(1.0)
                done.record()
            apart = False
            while not held.query():
                if done.query():
                    apart = not held.query()
                    break
            torch.cuda.synchronize()
            self._apart[key] = apart
        return self._apart[key]

    def side_stream(self, device, apart_from=()):
        """A torch.cuda.Stream (the next of torch's pool) that shares a hardware queue neither with torch's default stream nor with any
        stream in `apart_from`.  A pair of streams seen for the first time is probed, which synchronises the device: not for use inside
        a call under check_side_stream."""
        others = [torch.cuda.default_stream(device)] + list(apart_from)
        for _ in range(64):
            s = torch.cuda.Stream(device)
            if all(s.cuda_stream != o.cuda_stream and self.independent(s, o) and self.independent(o, s) for o in others):
                return s
        raise AssertionError("no stream of torch's pool runs beside %d given stream(s): are all hardware queues taken?" % len(others))

    def ms_for(self, host_seconds):
        return min(self.cap_ms, max(self.floor_ms, 3e3 * host_seconds))

    def enqueue(self, ms):
        """on the current stream"""
        for _ in range(int(math.ceil(ms / self.unit_ms))):
            self.buf.fill_(1)


def _stale(op, device):
    """What an operand of the side-stream run holds until the staged data is copied in on that stream."""
    if op.kind in ("out", "scratch"):
        t = torch.empty(op.shape, dtype=op.dtype, device=device)
        _bytes(t).fill_(PLAIN_OUT_BYTE)
    elif op.dtype.is_floating_point:
        t = torch.full(op.shape, float("nan"), dtype=op.dtype, device=device)
    elif op.kind == "in":
        t = torch.full(op.shape, op.loud, dtype=op.dtype, device=device)
    else:
        t = torch.zeros(op.shape, dtype=op.dtype, device=device)
    return t


def check_side_stream(operands, call, device, delay, reference=None, delay_ms=None, stream=None):
    """Runs `call` on a fresh side stream whose operands become valid only on that stream, behind `delay` (a Delay):

      inputs and in/out payloads start stale (quiet NaN; integers: the operand's loud value, in/out integers zeros), outputs as 0x3C bytes;
      the data waits in staging tensors; everything is synchronised;
      on a fresh torch.cuda.Stream: the delay, the copies staging -> operands, `call`, copies of the outputs and in/out buffers into snapshots;
      that stream alone is synchronised and the snapshots are read, then the device is synchronised.

    The snapshots must be byte-identical to the outputs of the default-stream plain run (`reference` = plain_run(..), made here if None) and the
    inputs unchanged.  A piece of the call on another queue reads stale data or writes after the snapshot; a missing join leaves 0x3C bytes.
    Returns (snapshots, armed): armed says that the delay was still running when `call` had returned to the host, i.e. that the whole call
    was enqueued behind it.  Where it is False the check holds only up to the call's first synchronisation -- or the host was held up while
    it enqueued: delay_ms asks for a longer delay than the row's own.
    The side stream is one that does not share a hardware queue with torch's default stream (Delay.side_stream): on a shared queue work
    misplaced onto the default stream would run in enqueue order and look well placed.  The library's internal streams cannot be chosen
    that way; a misplacement among them is seen whenever they sit on another queue than the caller's.  stream: the side stream to use
    (the self-test's fakes need to know it beforehand, to pick their own second stream on another queue)."""
    assert torch.device(device).type == "cuda", "a side stream needs a device"
    if reference is None:
        reference = plain_run(operands, call, device)
    ref, host = reference
    ts = {k: _stale(op, device) for k, op in operands.items()}
    staged = {k: op.data.detach().clone().contiguous().to(device) for k, op in operands.items() if op.kind in ("in", "inout")}
    snaps = {k: torch.zeros(op.shape, dtype=op.dtype, device=device) for k, op in operands.items() if op.kind in ("out", "inout")}
    torch.cuda.synchronize()
    s = stream or delay.side_stream(device)              # fresh, and on another hardware queue than the default stream
    gate = torch.cuda.Event()
    with torch.cuda.stream(s):
        delay.enqueue(delay.ms_for(host) if delay_ms is None else delay_ms)
        gate.record()
        for k, v in staged.items():
            ts[k].copy_(v)
        rc = call(ts)
        armed = not gate.query()
        for k, v in snaps.items():
            v.copy_(ts[k])
        s.synchronize()
        got = {k: _bytes(v).cpu() for k, v in snaps.items()}
    torch.cuda.synchronize()
    assert rc in (None, 0), "side-stream run: the call returned %r" % (rc,)
    for k, op in operands.items():
        if op.kind == "in":
            assert torch.equal(_bytes(ts[k]), _bytes(staged[k])), "side-stream run: input %r was modified" % k
        elif op.kind in ("out", "inout"):
            want = _bytes(ref[k]).cpu()
            assert torch.equal(got[k], want), ("side-stream run: the snapshot of %s %r, taken on the call's stream, differs from the default-stream run: "
                                               "first at byte %d, %d bytes" % ((op.kind, k) + _first_diff(got[k], want)))
    return snaps, armed


ELEMENT_SHIFT = {torch.float32: 4, torch.int32: 4, torch.float64: 8, torch.int64: 8, torch.float16: 2, torch.uint8: 1}


def check_unaligned(operands, call, device, which, reference=None, refusal=None, bits_may_differ=False):
    """The loud-moat fenced run with the operands named in `which` one element behind the 256-byte boundary (scratch operands never move: a
    workspace's carves assume an aligned base).  Accepted: the call returns 0, every moat is intact, inputs are unchanged and the outputs are
    byte-identical to the aligned plain run (`reference`); or, with refusal = (error code, last_error function): the call returns that code,
    the outputs keep their 0xA5 bytes and the error text names the alignment.  bits_may_differ: the comparison with the aligned run is left
    to the caller (who compares the returned tensors with the oracle).  Returns (tensors, "ran" | "refused")."""
    if reference is None:
        reference = plain_run(operands, call, device)
    ref = reference[0]
    for k in which:
        assert operands[k].kind != "scratch", "scratch operand %r is never shifted" % k
    ts = {k: _fenced(op, device, True, ELEMENT_SHIFT[op.dtype] if k in which else 0) for k, op in operands.items()}
    for k in which:
        assert ts[k].data_ptr() % ALIGN == ELEMENT_SHIFT[operands[k].dtype] or torch.device(device).type == "cpu"
    _sync(device)
    rc = call(ts)
    _sync(device)
    for k, op in operands.items():
        hit = ts[k].fence.moats_intact()
        assert hit is None, ("unaligned run (%s shifted): %d moat byte(s) of %s operand %r changed, the first %d byte(s) %s its payload"
                             % (",".join(sorted(which)), hit[2], op.kind, k, hit[1], hit[0]))
        if op.kind == "in":
            got, want = _bytes(ts[k]), _bytes(op.data.detach().contiguous().to(device))
            assert torch.equal(got, want), "unaligned run: input %r was modified (first at byte %d, %d bytes)" % ((k,) + _first_diff(got, want))
    if rc not in (None, 0):
        assert refusal is not None and rc == refusal[0], "unaligned run (%s shifted): the call returned %r" % (",".join(sorted(which)), rc)
        msg = refusal[1]()
        assert "align" in str(msg), "the refusal does not name the alignment: %r" % (msg,)
        for k, op in operands.items():
            if op.kind == "out":
                assert bool((_bytes(ts[k]) == OUT_BYTE).all()), "a refused call wrote output %r" % k
            elif op.kind == "inout":
                assert torch.equal(_bytes(ts[k]), _bytes(op.data.detach().contiguous().to(device))), "a refused call changed in/out %r" % k
        return ts, "refused"
    if not bits_may_differ:
        for k, op in operands.items():
            if op.kind in ("out", "inout"):
                got, want = _bytes(ts[k]), _bytes(ref[k])
                assert torch.equal(got, want), ("unaligned run (%s shifted) differs from the aligned plain run in %s %r: first at byte %d of the payload, "
                                                "%d bytes" % ((",".join(sorted(which)), op.kind, k) + _first_diff(got, want)))
    return ts, "ran"
