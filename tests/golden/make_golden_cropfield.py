"""Goldens for the crop-field conversion of the abdomen MR-CT script, captured by EXECUTING the reference's own function definitions
(run ONLY where the reference tree is present):

    python tests/golden/make_golden_cropfield.py        # -> tests/golden/cropfield.npz

l2r_2021_convexAdam_task1_docker.py runs the whole challenge at import time, so it cannot be imported; its `util_kpts_pt` (:29-37) and
`convert_crop_field` (:38-105) FunctionDef nodes are lifted out of the parsed file with `ast`, compiled as they stand and called on the
CPU: `torch.Tensor.cuda` is the identity for the duration, and `pd.read_csv` is a stand-in that returns one in-memory row with the
three pandas accessors the function uses (df['Id'] == case, df.loc[mask], df[column].values[0]).  No reference text is stored.

Stored per case: the row's strings, the float32 field (1, H, W, D, 3) in millimetres and the float16 array the function returned.
  small   fixed 11 x 9 x 7, a field of a few millimetres on 5 x 5 x 9
  far     fixed 13 x 10 x 9, displacements of tens of millimetres, where float16 resolves 1/32 to 1/16 mm
"""
import ast
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ref_import import REF_ROOT  # noqa: E402

SCRIPT = "l2r_2021_convexAdam_task1_docker.py"
COLUMNS = ("FixShape", "FixSpacing", "FixCrop", "MovShape", "MovSpacing", "MovCrop")


class Column:
    def __init__(self, values):
        self.values = values

    def __eq__(self, other):
        return [v == other for v in self.values]


class Frame:
    """the three accessors of a pandas DataFrame that convert_crop_field touches"""
    def __init__(self, rows):
        self.rows = rows
        self.loc = self

    def __getitem__(self, key):
        if isinstance(key, str):
            return Column([r[key] for r in self.rows])
        return Frame([r for r, keep in zip(self.rows, key) if keep])


def lift(names, **globs):
    tree = ast.parse(open(os.path.join(REF_ROOT, SCRIPT)).read())
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(f.name for f in fns) == sorted(names)
    ns = dict(torch=torch, F=F, np=np, **globs)
    exec(compile(ast.Module(body=fns, type_ignores=[]), SCRIPT, "exec"), ns)
    return ns


def brackets(values):
    return "[" + " ".join("%g" % v for v in values) + "]"


CASES = {
    # tag: (row, field shape, offset and spread of the field in mm)
    "small": (dict(FixShape=(11, 9, 7), FixSpacing=(1.5, 1.5, 3.0), FixCrop=(2, 9, 1, 8, 0, 6), MovShape=(12, 13, 9), MovSpacing=(1.2, 1.2, 2.5),
                   MovCrop=(1, 9, 2, 11, 1, 7)), (5, 5, 9), 0.0, 2.0),
    "far": (dict(FixShape=(13, 10, 9), FixSpacing=(0.9, 1.1, 2.5), FixCrop=(1, 12, 0, 9, 1, 8), MovShape=(15, 12, 10), MovSpacing=(1.0, 0.8, 3.0),
                 MovCrop=(2, 14, 1, 11, 0, 9)), (5, 5, 9), 35.0, 12.0),
}


def main():
    rng = np.random.default_rng(2021)
    out = {}
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        for tag, (row, shape, offset, spread) in CASES.items():
            strings = {k: brackets(row[k]) for k in COLUMNS}
            frame = Frame([dict(Id=tag, **strings), dict(Id="another", **strings)])
            ns = lift(("util_kpts_pt", "convert_crop_field"), pd=type("pd", (), {"read_csv": staticmethod(lambda path: frame)}))
            sign = np.where(rng.random((1,) + shape + (3,)) < 0.5, -1.0, 1.0)
            field = (sign * offset + spread * rng.standard_normal((1,) + shape + (3,))).astype(np.float32)
            got = ns["convert_crop_field"](tag, torch.from_numpy(field.copy()))
            assert got.dtype == np.float16 and got.shape == (3,) + tuple(s // 2 for s in row["FixShape"]), (got.dtype, got.shape)
            out[tag + "_field"] = field
            out[tag + "_out"] = got
            for k in COLUMNS:
                out[tag + "_" + k] = np.array(strings[k])
    finally:
        torch.Tensor.cuda = cuda
    path = os.path.join(HERE, "cropfield.npz")
    np.savez_compressed(path, **out)
    print("wrote cropfield.npz %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
