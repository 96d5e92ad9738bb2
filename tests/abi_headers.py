"""What a public header under include/ declares, read as text: shared by test_abi.py, test_prep_abi.py, test_fieldops_abi.py and
test_affine_abi.py, each of which holds its own header against its own binding table."""
import re


def header_source(path):
    """the header without its block comments"""
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def header_functions(path):
    """the sorted names of the cvx_* functions the header declares"""
    return sorted(set(re.findall(r"\b(cvx_[a-z0-9_]+)\s*\(", header_source(path))))
