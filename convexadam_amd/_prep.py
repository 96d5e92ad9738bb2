"""The preprocessing binding (include/convexadam_prep.h) under its earlier module name: the table, the flags and the handle all live in
_lib.py, and lib() types every table when it loads the library.  tests/test_prep_abi.py and the GPU suites name this module."""
from ._lib import CVX_PREP_CLAMP, CVX_PREP_POSITIVE, PREP_SIGNATURES, lib  # noqa: F401
