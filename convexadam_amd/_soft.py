"""The binding of include/convexadam_soft.h: the table lives in _lib.py beside the other four; lib() here is _lib.soft_lib(), which types
it on the handle the first time it is asked.  tests/test_softstats_abi.py and the GPU suites name this module."""
from ._lib import SOFT_SIGNATURES, soft_lib as lib  # noqa: F401
