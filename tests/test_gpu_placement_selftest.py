"""fences.check_side_stream can fail (run on the MI355X box with `-m gpu`).  Fake operators, written with torch ops, that put their work on the
wrong queue in the four ways the check exists for are each reported; the well-behaved one is not.  Without this a green
tests/test_gpu_placement.py proves nothing.

The fakes are data races on the test's own tensors and nothing else: every access stays inside the operands, nothing waits on memory or on
another workgroup, and the harness synchronises the device before it compares.

Streams are dealt onto a few hardware queues, and two streams on one queue run in enqueue order: work misplaced between them looks well
placed.  So the harness takes a side stream on another queue than the default stream's, and the fakes that use a second stream take one on
another queue than the caller's (Delay.side_stream probes that, before the run); test_streams_on_one_queue_are_told_apart pins the probe itself."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fences import IN, INOUT, OUT, Delay, check_side_stream  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPE = (32, 64, 64)


@pytest.fixture(scope="module")
def delay():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return Delay(DEV)


def operands():
    g = torch.Generator().manual_seed(5)
    x = torch.rand(SHAPE, generator=g)
    idx = torch.randint(0, 4, SHAPE, generator=g, dtype=torch.int32)
    return {"x": IN(x), "idx": IN(idx, loud=3), "y": OUT(SHAPE), "state": INOUT(torch.rand(SHAPE, generator=g))}


def work(t):
    t["y"].copy_(2 * t["x"] + t["idx"].to(torch.float32))
    t["state"].add_(1)


def op_good(t):
    work(t)


def op_forks_and_joins(t):
    """an internal stream used correctly: forked from the caller's stream by an event, joined back by another"""
    cur, side = torch.cuda.current_stream(), torch.cuda.Stream(DEV)
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        work(t)
    cur.wait_stream(side)


def op_default_stream(t):
    with torch.cuda.stream(torch.cuda.default_stream()):
        work(t)


def make_op_second_stream_no_event(other):
    def op(t):
        with torch.cuda.stream(other):
            work(t)
    return op


def make_op_never_joins(delay, other):
    def op(t):
        other.wait_stream(torch.cuda.current_stream())   # the fork is right: the inputs are valid when the work starts
        with torch.cuda.stream(other):
            delay.enqueue(delay.floor_ms)
            work(t)
    return op


def make_op_zeroes_here_accumulates_elsewhere(other):
    def op(t):
        t["y"].zero_()
        t["state"].add_(1)
        with torch.cuda.stream(other):
            t["y"].add_(2 * t["x"] + t["idx"].to(torch.float32))
    return op


def test_delay_outlasts_its_own_enqueue(delay):
    assert delay.unit_ms > 3 * delay.enqueue_ms and delay.floor_ms == 100 * delay.launch_ms and delay.floor_ms < delay.cap_ms
    s = torch.cuda.Stream(DEV)
    gate = torch.cuda.Event()
    with torch.cuda.stream(s):
        delay.enqueue(delay.floor_ms)
        gate.record()
        assert not gate.query(), "the delay had drained before its last fill was enqueued"
    s.synchronize()
    assert gate.query()


@pytest.mark.parametrize("op", [op_good, op_forks_and_joins], ids=["plain", "forks_and_joins"])
def test_well_behaved_operator_passes(delay, op):
    snaps, armed = check_side_stream(operands(), op, DEV, delay)
    ops = operands()
    assert armed
    assert torch.equal(snaps["y"].cpu(), 2 * ops["x"].data + ops["idx"].data.float()) and torch.equal(snaps["state"].cpu(), ops["state"].data + 1)


@pytest.mark.parametrize("name", ["default_stream", "second_stream_no_event", "never_joins", "zeroes_here_accumulates_elsewhere"])
def test_misplaced_work_is_reported(delay, name):
    from fences import plain_run
    s = delay.side_stream(DEV)                           # the harness's stream, and a second one on another queue than it: chosen before the run
    other = delay.side_stream(DEV, apart_from=[s])
    op = {"default_stream": op_default_stream, "second_stream_no_event": make_op_second_stream_no_event(other), "never_joins": make_op_never_joins(delay, other),
          "zeroes_here_accumulates_elsewhere": make_op_zeroes_here_accumulates_elsewhere(other)}[name]
    want = plain_run(operands(), op_good, DEV)           # (a fake that races on the default stream as well has no reference of its own)
    with pytest.raises(AssertionError) as e:
        check_side_stream(operands(), op, DEV, delay, reference=want, stream=s)
    assert "snapshot of out 'y', taken on the call's stream, differs from the default-stream run" in str(e.value), str(e.value)
    torch.cuda.synchronize()


def test_failed_call_is_reported(delay):
    calls = []

    def fails_on_the_side_stream(t):
        calls.append(1)
        work(t)
        return 0 if len(calls) == 1 else -3
    with pytest.raises(AssertionError, match="side-stream run: the call returned -3"):
        check_side_stream(operands(), fails_on_the_side_stream, DEV, delay)


def test_streams_on_one_queue_are_told_apart(delay):
    """the probe behind Delay.side_stream: a stream is not independent of itself, the chosen side stream runs beside the default stream in
    both directions, and a second one beside both"""
    d = torch.cuda.default_stream(DEV)
    s = delay.side_stream(DEV)
    assert not delay.independent(s, s) and not delay.independent(d, d)
    assert delay.independent(s, d) and delay.independent(d, s)
    u = delay.side_stream(DEV, apart_from=[s])
    assert u.cuda_stream not in (s.cuda_stream, d.cuda_stream) and delay.independent(s, u) and delay.independent(u, s) and delay.independent(u, d)
