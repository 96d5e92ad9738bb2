"""CPU checks of the affine entry points (include/convexadam_affine.h): the header and the binding table list the same names, the library
exports them, none of them leaked into the main header or table, the ABI version is unchanged, the workspace query, and every bad argument
is refused with a message before anything touches a device (the pointers below are not memory: a launch would fault)."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "convexadam_affine.h")
NAMES = ["cvx_affine_field_f64", "cvx_affine_lts_f32", "cvx_affine_lts_workspace_bytes"]
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from abi_headers import header_functions, header_source  # noqa: E402


@pytest.fixture(scope="module")
def L():
    from convexadam_amd.csrc import build
    build.build()
    from convexadam_amd import _affine
    return _affine.lib()


def test_header_and_table_list_the_same_names(L):
    from convexadam_amd import _affine, _field, _lib, _prep
    names = header_functions(HEADER)
    assert names == NAMES and names == sorted(_affine.AFFINE_SIGNATURES)
    for table in (_lib.SIGNATURES, _prep.PREP_SIGNATURES, _field.FIELD_SIGNATURES):
        assert not set(names) & set(table), "the affine entry points have a table of their own"
    main = open(os.path.join(ROOT, "include", "convexadam_hip.h")).read()
    src = header_source(HEADER)
    for n in names:
        assert hasattr(L, n), "libconvexadam_hip.so does not export %s" % n
        assert n not in main
        assert getattr(L, n).restype is _affine.AFFINE_SIGNATURES[n][0]
        args = re.search(r"\b%s\s*\(([^)]*)\)" % n, src).group(1)
        assert len(args.split(",")) == len(_affine.AFFINE_SIGNATURES[n][1]), n


def test_version_is_unchanged(L):
    from convexadam_amd import _lib
    assert L.cvx_version() == 2 == _lib.ABI_VERSION


def test_python_names_are_reexported():
    from convexadam_amd import affine, convex_adam_utils
    for n in ("find_affine_3d", "least_trimmed_affine", "least_trimmed_squares", "affine_from_field", "convex_adam_affine", "affine_to_field",
              "register_with_affine"):
        assert getattr(convex_adam_utils, n) is getattr(affine, n)


def test_affine_module_imports_on_its_own():
    """convexadam_amd.affine imported FIRST in a fresh interpreter (tools/time_affine.py does that): affine_to_field then pulls in fieldops and
    convex_adam_utils, which import each other; a host tensor must get as far as the device check"""
    import subprocess
    import sys
    code = ("import torch\nfrom convexadam_amd.affine import affine_to_field\n"
            "try:\n    affine_to_field(torch.eye(4), (2, 3, 4))\nexcept RuntimeError as e:\n    assert 'no CPU path' in str(e), e\n    print('refused')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "refused", r.stderr[-2000:]


def test_build_lists_the_source_and_the_header():
    from convexadam_amd.csrc import build
    assert "affine.hip" in build.SOURCES
    for f in ("affine.hip", "affine_core.h", "lts_common.h"):
        assert os.path.exists(os.path.join(build.HERE, f)), f


def test_workspace_query(L):
    q = L.cvx_affine_lts_workspace_bytes
    for n in (-1, 0, 3, (1 << 28) + 1):
        assert q(n) == 0
    # pattern words, selection bytes and the status word, each carve on a 256-byte boundary, 256 bytes of slack behind the last
    up = lambda v: -(-v // 256) * 256  # noqa: E731
    for n in (4, 8, 63, 64, 65, 1025, 70001, 1 << 28):
        assert q(n) == up(up(4 * n) + n) + 4 + 256, n
    assert all(q(n + 1) >= q(n) for n in range(4, 3000))


F, M, X, INL, WS = (C.c_void_p(k << 32) for k in (1, 2, 3, 4, 5))


def test_fit_refuses_bad_arguments_without_a_launch(L):
    n = 1000
    ok = dict(f=F, ldf=4, m=M, ldm=4, n=n, iters=5, normal=0, X=X, inl=INL, ws=WS, wsb=L.cvx_affine_lts_workspace_bytes(n))

    def call(**kw):
        a = dict(ok, **kw)
        return L.cvx_affine_lts_f32(a["f"], a["ldf"], a["m"], a["ldm"], a["n"], a["iters"], a["normal"], a["X"], a["inl"], a["ws"], a["wsb"], None)

    def refused(word, code=-1, **kw):
        assert call(**kw) == code, kw
        assert word in L.cvx_last_error(), (kw, L.cvx_last_error())

    for k in ("f", "m", "X", "ws"):
        refused(b"null", **{k: None})
    for bad in (-1, 0, 3, (1 << 28) + 1):
        refused(b"outside", n=bad)
    for bad in (4, 7):
        refused(b"n >= 8", n=bad)                                # two fits need n / 2 >= 4 points
    refused(b"iters", iters=0)
    refused(b"iters", iters=-2)
    for bad in (-1, 2):
        refused(b"normal", normal=bad)
    refused(b"ld", ldf=3)                                        # three columns: a single least-squares fit only
    refused(b"ld", ldm=3)
    refused(b"ld", ldf=3, ldm=3, iters=1, normal=1)
    refused(b"ld", ldf=2, ldm=3, iters=1)
    refused(b"ld", ldf=(1 << 20) + 1)
    refused(b"aligned", f=C.c_void_p((1 << 32) + 2))
    refused(b"aligned", X=C.c_void_p((3 << 32) + 1))
    refused(b"X overlaps", X=F)
    refused(b"X overlaps", X=C.c_void_p((2 << 32) + 16 * n - 4))
    refused(b"inliers overlaps", inl=C.c_void_p((1 << 32) + 16 * n - 1))
    refused(b"inliers overlaps", inl=C.c_void_p((3 << 32) + 63))
    refused(b"workspace", code=-2, wsb=ok["wsb"] - 1)
    refused(b"workspace", code=-2, wsb=0)


def test_field_refuses_bad_arguments_without_a_launch(L):
    H, W, D = 6, 5, 7
    V = H * W * D
    TH, U, O = F, M, X
    ok = dict(th=TH, H=H, W=W, D=D, u=U, u64=0, ucs=1, uvs=3, out=O, o64=1, ocs=V, ovs=1)

    def call(**kw):
        a = dict(ok, **kw)
        return L.cvx_affine_field_f64(a["th"], a["H"], a["W"], a["D"], a["u"], a["u64"], a["ucs"], a["uvs"], a["out"], a["o64"], a["ocs"], a["ovs"], None)

    def refused(word, **kw):
        assert call(**kw) == -1, kw
        assert word in L.cvx_last_error(), (kw, L.cvx_last_error())

    refused(b"null", th=None)
    refused(b"null", out=None)
    for axis in "HWD":
        refused(b"extent", **{axis: 0})
        refused(b"extent", **{axis: -3})
    refused(b"2^31", H=2048, W=2048, D=512)
    refused(b"2^31", H=1 << 16, W=1 << 16, D=1)
    refused(b"strides of u", ucs=1, uvs=2)                       # components fold onto the next voxel
    refused(b"strides of u", ucs=V - 1, uvs=1)                   # planes fold onto each other
    refused(b"strides of u", ucs=0)
    refused(b"strides of out", ocs=1, ovs=1)
    refused(b"strides of out", ovs=-1)
    refused(b"aligned", th=C.c_void_p((1 << 32) + 2))
    refused(b"aligned", u=C.c_void_p((2 << 32) + 2))
    refused(b"aligned", u=C.c_void_p((2 << 32) + 4), u64=1)
    refused(b"aligned", out=C.c_void_p((3 << 32) + 4))
    refused(b"overlaps", out=U)
    refused(b"overlaps", out=C.c_void_p((2 << 32) + 4 * 3 * V - 8))
    refused(b"overlaps", out=C.c_void_p((1 << 32) + 40))
    # strides of an absent u are not looked at
    assert call(u=None, ucs=0, uvs=0, out=None) == -1 and b"null" in L.cvx_last_error()
