"""Golden for the least-trimmed affine fit, captured by EXECUTING the reference's own function definition (run ONLY in the build container):

    python tests/golden/make_golden_affine.py        # -> tests/golden/affine_lts.npz

l2r_2020_convexAdam_CuRIOUS.py runs a whole challenge case at import time, so it cannot be imported; its `least_trimmed_squares`
FunctionDef node (:272-278) is lifted out of the parsed file with `ast`, compiled as it stands and called with this script's globals, as
make_golden_variants.py does.  No reference text is stored.  The function calls torch.solve(B, A), which current torch no longer has; it
is supplied as (torch.linalg.solve(A, B), None) -- the same equation A X = B and the same return shape.

Per tag and iteration count k the file holds the points (float32), the reference's own float32 result `<tag>_ref<k>`, and `<tag>_f64_<k>`:
the SAME function run on the float64 copies of the points, i.e. a float64 evaluation of the same equation and the same selection.
"""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("CONVEXADAM_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
import affine_restatement as R  # noqa: E402

CASES = (("clean", dict(n=600, seed=11, noise=0.0, outliers=0.4), (1, 2, 5)), ("noisy", dict(n=501, seed=12, noise=1e-2, outliers=0.0), (1,)))


class _Torch:
    """torch with the removed torch.solve(B, A) -> (solution of A X = B, LU) put back"""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def solve(B, A):
        return torch.linalg.solve(A, B), None


def lift(script, name):
    tree = ast.parse(open(os.path.join(REF, script)).read())
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name)
    ns = dict(torch=_Torch())
    exec(compile(ast.Module(body=[fn], type_ignores=[]), script, "exec"), ns)
    return ns[name]


def main():
    fn = lift("l2r_2020_convexAdam_CuRIOUS.py", "least_trimmed_squares")
    out = {}
    for tag, kw, ks in CASES:
        f, m, _ = R.points(**kw)
        out[tag + "_fixed"], out[tag + "_moving"] = f, m
        for k in ks:
            out["%s_ref%d" % (tag, k)] = fn(torch.from_numpy(f.copy()), torch.from_numpy(m.copy()), k).numpy()
            out["%s_f64_%d" % (tag, k)] = fn(torch.from_numpy(f.copy()).double(), torch.from_numpy(m.copy()).double(), k).numpy()
    path = os.path.join(HERE, "affine_lts.npz")
    np.savez_compressed(path, **out)
    print("wrote affine_lts.npz %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
