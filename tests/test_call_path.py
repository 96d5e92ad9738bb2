"""CPU checks of the one call path from the Python layer into the library (convexadam_amd/_lib.py: call, scratch, lib) against a stub
handle: no library is loaded and no device is touched.  The stand-in for a device is torch.device("cpu") -- it names no index, so call()
takes no guard, and workspace() allocates host memory -- with _lib.stream_ptr replaced by a fixed handle."""
import ctypes as C
import threading

import pytest
import torch

from convexadam_amd import _lib

CPU = torch.device("cpu")
STREAM = 0x5150
TABLES = ("SIGNATURES", "PREP_SIGNATURES", "FIELD_SIGNATURES", "AFFINE_SIGNATURES")


class Stub:
    """A handle with every entry point of the four tables (minus `lacking`); each records its arguments and answers what `answers` says
    for its name (0 otherwise).  cvx_last_error answers `message`."""

    def __init__(self, lacking=(), answers=None, message=b""):
        self.calls, self.message = [], message
        answers = dict(answers or {}, cvx_version=_lib.ABI_VERSION)
        for table in TABLES:
            for name in getattr(_lib, table):
                if name not in lacking:
                    setattr(self, name, self._entry(name, answers.get(name, 0)))
        self.cvx_last_error = lambda: self.message

    def _entry(self, name, answer):
        def entry(*args):
            self.calls.append((name, args))
            return answer
        return entry


@pytest.fixture
def stub(monkeypatch):
    def install(**kw):
        s = Stub(**kw)
        monkeypatch.setattr(_lib, "_lib", s)
        return s
    monkeypatch.setattr(_lib, "stream_ptr", lambda device=None: C.c_void_p(STREAM))
    monkeypatch.setattr(_lib, "_tls", threading.local())
    return install


def test_call_appends_the_stream_last_and_checks_the_status(stub):
    s = stub(answers={"cvx_box3_fast_f32": _lib.CVX_ERR_LAUNCH}, message=b"box3: launch failed")
    assert _lib.call(CPU, "cvx_avgpool_f32", 1, 2.5, None) is None
    (name, args), = s.calls
    assert name == "cvx_avgpool_f32" and args[:-1] == (1, 2.5, None)
    assert isinstance(args[-1], C.c_void_p) and args[-1].value == STREAM
    with pytest.raises(_lib.CvxError, match="box3: launch failed") as e:
        _lib.call(CPU, "cvx_box3_fast_f32", 7)
    assert e.value.code == _lib.CVX_ERR_LAUNCH
    assert s.calls[-1][1][0] == 7 and s.calls[-1][1][-1].value == STREAM


def test_required_scratch_refuses_a_zero_answer(stub):
    s = stub(message=b"cvx_register_pair: bad extent")
    with pytest.raises(_lib.CvxError, match="bad extent") as e:
        _lib.scratch(CPU, "cvx_register_pair_workspace_bytes", 3, required=True, otherwise="not this")
    assert e.value.code == _lib.CVX_ERR_INVALID_ARG and "not this" not in str(e.value)
    assert s.calls == [("cvx_register_pair_workspace_bytes", (3,))]
    s.message = b""
    with pytest.raises(_lib.CvxError, match="bad snapshot arguments") as e:
        _lib.scratch(CPU, "cvx_register_pair_snapshots_workspace_bytes", required=True, otherwise="bad snapshot arguments")
    assert e.value.code == _lib.CVX_ERR_INVALID_ARG


def test_scratch_passes_a_zero_answer_on_with_a_buffer(stub):
    stub()
    p, n = _lib.scratch(CPU, "cvx_box_smooth_workspace_bytes", 3, 4, 4, 4, 1)
    assert n == 0 and isinstance(p, C.c_void_p) and p.value


def test_scratch_returns_the_query_value_and_the_stream_buffer(stub):
    stub(answers={"cvx_adam_workspace_bytes": 10000, "cvx_register_pair_workspace_bytes": 5000})
    p, n = _lib.scratch(CPU, "cvx_adam_workspace_bytes", 12, 4, 4, 4)
    (key, buf), = _lib._tls.workspaces.items()
    assert n == 10000 and p.value == buf.data_ptr() and buf.numel() >= n and key == (str(CPU), STREAM)
    assert _lib.scratch(CPU, "cvx_adam_workspace_bytes", 12, 4, 4, 4, required=True)[0].value == p.value          # grow-only: reused
    p3, n3 = _lib.scratch(CPU, "cvx_register_pair_workspace_bytes", None, required=True, size=lambda per: 3 * (per + 3192))
    assert n3 == 3 * 8192 and _lib._tls.workspaces[key].numel() >= n3 and p3.value == _lib._tls.workspaces[key].data_ptr()


@pytest.mark.parametrize("table", TABLES)
def test_a_library_that_lacks_a_declared_entry_point_fails_at_load(monkeypatch, table):
    name = sorted(getattr(_lib, table))[-1]
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", __file__)
    monkeypatch.setattr(C, "CDLL", lambda path: Stub(lacking=(name,)))
    with pytest.raises(RuntimeError, match="lacks the entry point %s: rebuild with" % name):
        _lib.lib()
    assert _lib._lib is None
    monkeypatch.setattr(C, "CDLL", lambda path: Stub())
    assert _lib.lib() is _lib.lib() and isinstance(_lib.lib(), Stub)
