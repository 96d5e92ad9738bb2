"""The binding of include/convexadam_sim.h: the table lives in _lib.py beside the other five; lib() here is _lib.sim_lib(), which types
it on the handle the first time it is asked.  tests/test_simhist_abi.py and the GPU suites name this module."""
from ._lib import SIM_SIGNATURES, sim_lib as lib  # noqa: F401
