"""Every fenced operator once more on a side stream and at unaligned addresses (run on the MI355X box with `-m gpu`).

The fence tables (tests/test_gpu_fences.py, tests/test_gpu_prep_fences.py, tests/test_gpu_fieldops_fences.py) run every row on torch's
default stream with 256-byte aligned payloads.  Here the same rows, with the same ids and options, run

  * under fences.check_side_stream: on a fresh stream, behind a delay, with operands that become valid only on that stream and snapshots of
    the outputs taken on it.  A launch, memset or copy that forgets its stream argument, or an internal stream that is not forked from /
    joined to the caller's, changes a snapshot.
  * under fences.check_unaligned with every non-scratch operand one element behind the 256-byte boundary: what trips every pointer guard of
    a launcher at once
  * the same with each operand shifted alone, for the first default-option row of every entry point: what meets a guard that looks at the
    wrong pointer.
All three in one test item per row, test_row[<the row's id>]: they share the row's operands and its plain run.

Two things the tables cannot express have tests of their own: cvx_register_pairs_f32 (its operands travel through host pointer tables and it
runs on an internal stream pool) and the pair pipeline with option mind_overlap = 1.  The last tests need no device: every row id of the three
tables is run in both modes or excused in writing, and no table names what the libraries do not export."""
import ctypes as C
import os
import re
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_fences as F  # noqa: E402
import test_gpu_fieldops_fences as FF  # noqa: E402
import test_gpu_prep_fences as PF  # noqa: E402
from fences import IN, OUT, SCRATCH, Delay, check_side_stream, check_unaligned, plain_run  # noqa: E402
from test_gpu_workspace import PAIR_SHAPES, _pair, option, p, rnd, stream  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class PRow:
    """One row of one of the three tables: build(libs, orc) -> (operands, call, verify or None)."""

    def __init__(self, table, id, entry, opts, build):
        self.table, self.id, self.entry, self.opts, self.build = table, id, entry, opts, build


TABLE = [PRow("main", r.id, r.entry, r.opts, (lambda libs, orc, r=r: r.build(libs["main"], orc))) for r in F.ROWS] + \
        [PRow("prep", "%s-%s" % (r[0][4:], r[1]), r[0], {}, (lambda libs, orc, r=r: r[2](libs["prep"]))) for r in PF.ROWS] + \
        [PRow("field", "%s-%s" % (r[0][4:], r[1]), r[0], {}, (lambda libs, orc, r=r: r[2](libs["field"]))) for r in FF.ROWS]
IDS = [r.id for r in TABLE]

# ---- the exclusion tables (row id or entry point -> reason) ----------------------------------------------------------------------------
# rows that are not run under a mode at all
EXCLUDED_SIDE_STREAM = {}
EXCLUDED_UNALIGNED = {}

# Entry points whose call synchronises its stream before it returns (a `_host` result), or whose row's closure does: the delay has drained
# by then, so the side-stream check is sound only up to the first synchronisation.  They still run; the others must return to the host
# while the delay is still executing (check_side_stream's `armed`).
UP_TO_FIRST_SYNC = {
    "cvx_rigid_samples_f32": "the number of kept cells is a host result (count_host): the call synchronises its stream to deliver it, and the row's closure "
                             "synchronises the device to blank the unwritten rows; the check is sound only up to that first synchronisation",
    "cvx_tps_fit_f32": "the blocked LU reports a singular system through a device flag that the call reads back before it returns (tps.hip: copy to the host, then "
                       "a synchronisation of its stream); the factorisation and the solve run in front of it, so the check is sound only up to that first synchronisation",
    "cvx_rigid_lts_f32": "the fit's status word (degenerate sample sets) is read back by the call before it returns (rigid.hip: copy to the host, then a "
                         "synchronisation of its stream); the check is sound only up to that first synchronisation",
    "cvx_prep_nonzero_mask_u8": "the hole filling sweeps until nothing changes and reads its `changed` flag back after every round (prep.hip: copy to the host, then a "
                                "synchronisation of its stream); the check is sound only up to that first synchronisation, that of the first round",
    "cvx_surface_hist_batch_i64": "the row's closure uploads the pointer table from pageable host memory (a synchronous copy in front of the call) and synchronises "
                                  "the device behind it so that the table outlives the kernel; the check is sound only up to that first synchronisation",
}

# Entry points with the right to refuse a misaligned operand: (error code, the header sentence that gives it).  A row of such an entry
# point may return that code under check_unaligned (outputs untouched, cvx_last_error() names the alignment) or run with the same bits.
CVX_ERR_WORKSPACE = -2
REFUSES_UNALIGNED = {
    "cvx_mindssc_pooled_f32": (CVX_ERR_WORKSPACE,
                               "an image that is not 16-byte aligned always takes the two passes and needs their scratch whatever the query said"),
}

# Rows whose unaligned run may differ in bits from the aligned one: a different but documented evaluation order of the scalar path; the
# row's own comparison with the oracle must then pass on the unaligned run.
DIFFERENT_BITS = {}


def _excused(table, r):
    return table.get(r.id) or table.get(r.entry)


SIDE_ROWS = [r for r in TABLE if not _excused(EXCLUDED_SIDE_STREAM, r)]
UNALIGNED_ROWS = [r for r in TABLE if not _excused(EXCLUDED_UNALIGNED, r)]
# the first default-option row of every entry point
SINGLE_ROWS = list({r.entry: r for r in reversed(UNALIGNED_ROWS) if not r.opts}.values())[::-1]


@pytest.fixture(scope="module")
def libs():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from convexadam_amd import _field, _lib, _prep
    return {"main": _lib.lib(), "prep": _prep.lib(), "field": _field.lib()}


@pytest.fixture(scope="module")
def delay(libs):
    d = Delay(DEV)
    print("\n[placement] delay unit %.4f ms (256 MiB fill), enqueue %.4f ms, one-element fill to completion %.4f ms, floor %.3f ms, cap %.0f ms"
          % (d.unit_ms, d.enqueue_ms, d.launch_ms, d.floor_ms, d.cap_ms))
    return d


def _side_stream(operands, call, delay, synchronises=False, reference=None):
    """check_side_stream; a call that does not synchronise and still was not armed (the host was held up while it enqueued) runs once more
    behind the longest delay, so that what passes is a run whose every launch sat behind the delay"""
    snaps, armed = check_side_stream(operands, call, DEV, delay, reference=reference)
    if not armed and not synchronises:
        snaps, armed = check_side_stream(operands, call, DEV, delay, reference=reference, delay_ms=delay.cap_ms)
    return snaps, armed


def _movable(operands):
    return [k for k, op in operands.items() if op.kind != "scratch"]


def _refusal(libs, r):
    if r.entry not in REFUSES_UNALIGNED:
        return None
    return REFUSES_UNALIGNED[r.entry][0], libs["main"].cvx_last_error


def _unaligned(libs, r, operands, call, verify, which, ref):
    loose = r.id in DIFFERENT_BITS
    ts, how = check_unaligned(operands, call, DEV, which, reference=ref, refusal=_refusal(libs, r), bits_may_differ=loose)
    if loose and how == "ran":
        assert verify is not None, "a row in DIFFERENT_BITS needs its own comparison with the oracle"
        verify(ts)


@pytest.mark.gpu
@pytest.mark.parametrize("r", TABLE, ids=IDS)
def test_row(libs, orc, delay, r):
    """One row under both modes (one test item per row, not one per row and mode: the modes share the row's operands and its plain run, and
    the suite's list of items stays short; every assertion names its mode)."""
    with option(libs["main"], **r.opts):
        operands, call, verify = r.build(libs, orc)
        ref = plain_run(operands, call, DEV)
        if r in SIDE_ROWS:
            synchronises = r.entry in UP_TO_FIRST_SYNC
            _, armed = _side_stream(operands, call, delay, synchronises, ref)
            assert armed or synchronises, ("side-stream run: the call returned to the host only after the delay had drained (it synchronises, or its enqueue "
                                           "outlasts the cap of %.0f ms): list the entry point in UP_TO_FIRST_SYNC" % delay.cap_ms)
            assert not (armed and synchronises), "listed in UP_TO_FIRST_SYNC, but the whole call was enqueued behind the delay: take it off the table"
        if r in UNALIGNED_ROWS:
            _unaligned(libs, r, operands, call, verify, _movable(operands), ref)         # every operand at once: what trips every guard
            if r in SINGLE_ROWS:                                                          # each alone: what meets a guard that looks at the wrong pointer
                for k in _movable(operands):
                    _unaligned(libs, r, operands, call, verify, [k], ref)


# ---- what the tables cannot express ----------------------------------------------------------------------------------------------------
def _pairs_case():
    """three small pairs: (images fixed, images moving, params) of PAIR_SHAPES[0]"""
    shape = PAIR_SHAPES[0]
    pp = _pair(*shape, 1, 1.25, 0)
    return shape, pp, [rnd(shape, 90 + i, 0.0, 100.0) for i in range(3)], [rnd(shape, 93 + i, 0.0, 100.0) for i in range(3)]


@pytest.mark.gpu
def test_register_pairs_from_a_side_stream(libs, delay):
    """cvx_register_pairs_f32 on two internal streams, called from a side stream whose inputs arrive late: byte-identical to three
    cvx_register_pair_f32 calls on the default stream; then once more from a DIFFERENT side stream (the thread-local pool's events are reused)."""
    L = libs["main"]
    shape, pp, fixs, movs = _pairs_case()
    per = L.cvx_register_pair_workspace_bytes(C.byref(pp))
    ws1 = torch.empty(per, dtype=torch.uint8, device=DEV)
    want = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for f, m in zip(fixs, movs):
        out = torch.empty((3,) + shape, device=DEV)
        assert L.cvx_register_pair_f32(p(f), p(m), None, None, C.byref(pp), p(out), None, p(ws1), per, stream()) == 0, L.cvx_last_error()
        want.append(out)
    host = time.perf_counter() - t0                    # what the host spends to enqueue three pairs
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(w).all()) for w in want)
    n_streams = 2
    need = -(-per // 4096) * 4096 * n_streams
    used = []
    for attempt in range(2):                             # a different stream each time
        ins = [torch.full(shape, float("nan"), device=DEV) for _ in range(6)]
        outs = [torch.empty((3,) + shape, device=DEV) for _ in range(3)]
        for o in outs:
            o.view(-1).view(torch.uint8).fill_(0x3C)
        snaps = [torch.zeros((3,) + shape, device=DEV) for _ in range(3)]
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        fix, mov = (C.c_void_p * 3)(*[t.data_ptr() for t in ins[:3]]), (C.c_void_p * 3)(*[t.data_ptr() for t in ins[3:]])
        dst = (C.c_void_p * 3)(*[o.data_ptr() for o in outs])
        torch.cuda.synchronize()
        s = delay.side_stream(DEV, apart_from=used)
        used.append(s)
        gate = torch.cuda.Event()
        with torch.cuda.stream(s):
            delay.enqueue(min(delay.cap_ms, 10 * delay.ms_for(host)))      # (ten times the rows' rule: one call enqueues three pairs)
            gate.record()
            for t, v in zip(ins, fixs + movs):
                t.copy_(v)
            rc = L.cvx_register_pairs_f32(3, C.cast(fix, C.c_void_p), C.cast(mov, C.c_void_p), None, None, C.byref(pp), C.cast(dst, C.c_void_p), None, p(ws), need,
                                          n_streams, stream())
            armed = not gate.query()
            for sn, o in zip(snaps, outs):
                sn.copy_(o)
            s.synchronize()
            got = [sn.cpu() for sn in snaps]
        torch.cuda.synchronize()
        assert rc == 0, L.cvx_last_error()
        assert armed, "attempt %d: the three pairs' enqueue outlasted the delay" % attempt
        for i in range(3):
            assert torch.equal(got[i].view(torch.int32), want[i].cpu().view(torch.int32)), \
                "attempt %d, pair %d: the snapshot taken on the caller's stream differs from cvx_register_pair_f32 on the default stream" % (attempt, i)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", PAIR_SHAPES, ids=["x".join(map(str, s)) for s in PAIR_SHAPES])
def test_register_pair_mind_overlap_on_a_side_stream(libs, delay, shape):
    """option mind_overlap = 1 (the moving image's descriptor pass on the library's own side stream) under check_side_stream: no row carries it"""
    L = libs["main"]
    assert not any("mind_overlap" in r.opts for r in TABLE)
    H, W, D = shape
    pp = _pair(H, W, D, 1, 1.25, 0)
    a, b = rnd(shape, 43, 0.0, 100.0), rnd(shape, 44, 0.0, 100.0)
    ops = {"a": IN(a), "b": IN(b), "out": OUT((3,) + shape), "ws": SCRATCH(L.cvx_register_pair_workspace_bytes(C.byref(pp)))}

    def call(t):
        return L.cvx_register_pair_f32(p(t["a"]), p(t["b"]), None, None, C.byref(pp), p(t["out"]), None, p(t["ws"]), t["ws"].numel(), stream())
    in_order = plain_run(ops, call, DEV)
    with option(L, mind_overlap=1):
        snaps, armed = _side_stream(ops, call, delay)
        assert armed, "the pair's enqueue outlasted the longest delay"
    assert torch.equal(snaps["out"].view(torch.int32), in_order[0]["out"].view(torch.int32)), "mind_overlap = 1 changes the result"


@pytest.mark.gpu
@pytest.mark.parametrize("rid", ["adam_run_ex_f32-exact-f32-C12-5x3x8", "adam_run_ex_f32-exact-f32-C5-%s" % "x".join(map(str, F.ADAM_TILE_SHAPES[2]))])
def test_unaligned_lds_boxes(libs, orc, rid):
    """k_box3x3 (adam.hip) runs the exact boxes where the marching kernel does not reach: rows beyond 126 voxels, which no table holds, or
    option box_tiled = 1.  Rows of whole quads with P, m, v one element off: its 16-byte staging loads must give way to the element-wise ones."""
    r = next(r for r in TABLE if r.id == rid)
    assert not r.opts
    with option(libs["main"], box_tiled=1):
        operands, call, verify = r.build(libs, orc)
        assert operands["P"].shape[-1] % 4 == 0
        ref = plain_run(operands, call, DEV)
        verify(ref[0])
        check_unaligned(operands, call, DEV, _movable(operands), reference=ref)
        check_unaligned(operands, call, DEV, ["P"], reference=ref)


# ---- coverage (no device) --------------------------------------------------------------------------------------------------------------
def _exports():
    from convexadam_amd._field import FIELD_SIGNATURES
    from convexadam_amd._lib import SIGNATURES
    from convexadam_amd._prep import PREP_SIGNATURES
    return set(SIGNATURES) | set(PREP_SIGNATURES) | set(FIELD_SIGNATURES)


def test_every_row_runs_in_both_modes_or_is_excused():
    assert len(set(IDS)) == len(IDS) == len(F.ROWS) + len(PF.ROWS) + len(FF.ROWS), "row ids collide between the tables"
    side, unal = {r.id for r in SIDE_ROWS}, {r.id for r in UNALIGNED_ROWS}
    for r in TABLE:
        assert r.id in side or _excused(EXCLUDED_SIDE_STREAM, r), "%s runs on no side stream and is not excused" % r.id
        assert r.id in unal or _excused(EXCLUDED_UNALIGNED, r), "%s runs at no unaligned address and is not excused" % r.id
    fenced_entries = {r.entry for r in TABLE}
    single = {r.entry for r in SINGLE_ROWS}
    for e in fenced_entries:
        assert e in single or e in EXCLUDED_UNALIGNED, "%s has no default-option row for the single-operand shifts" % e
    assert all(not r.opts for r in SINGLE_ROWS) and len(single) == len(SINGLE_ROWS)
    for table in (EXCLUDED_SIDE_STREAM, EXCLUDED_UNALIGNED, UP_TO_FIRST_SYNC, DIFFERENT_BITS):
        assert all(isinstance(v, str) and len(v) > 60 for v in table.values()), "a reason longer than a phrase, please"
    assert "ic_fused" not in {k for r in TABLE for k in r.opts}        # the fused IC kernel rounds differently by design


def test_tables_name_exported_entry_points_only():
    names = _exports()
    ids = set(IDS)
    for table in (EXCLUDED_SIDE_STREAM, EXCLUDED_UNALIGNED, DIFFERENT_BITS):
        stray = {k for k in table if k not in ids and k not in names}
        assert not stray, "neither a row id nor an export: %s" % sorted(stray)
    for table in (UP_TO_FIRST_SYNC, REFUSES_UNALIGNED):
        assert not set(table) - names, "not exported: %s" % sorted(set(table) - names)
        assert not set(table) - {r.entry for r in TABLE}, "no row runs %s" % sorted(set(table) - {r.entry for r in TABLE})
    assert not {r.entry for r in TABLE} - names


def test_refusals_quote_the_header():
    text = ""
    for h in ("convexadam_hip.h", "convexadam_prep.h", "convexadam_field.h"):
        with open(os.path.join(ROOT, "include", h)) as f:
            text += re.sub(r"[\s*/]+", " ", f.read())
    for entry, (code, sentence) in REFUSES_UNALIGNED.items():
        assert code < 0 and re.sub(r"\s+", " ", sentence) in text, "%s: the header does not say %r" % (entry, sentence)
