"""The binding of include/convexadam_spline.h: the table lives in _lib.py beside the other six; lib() here is _lib.spline_lib(), which types
it on the handle the first time it is asked.  tests/test_spline_abi.py and the GPU suites name this module."""
from ._lib import SPLINE_SIGNATURES, spline_lib as lib  # noqa: F401
