"""The field-operator binding (include/convexadam_field.h) under its earlier module name: the table and the handle live in _lib.py, and
lib() types every table when it loads the library.  tests/test_fieldops_abi.py and the GPU suites name this module."""
from ._lib import FIELD_SIGNATURES, lib  # noqa: F401
