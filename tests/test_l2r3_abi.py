"""CPU checks of the rank-sum entry points (csrc/ranksum.hip): header, binding and export agree, the ABI version is unchanged, every
refusal returns its status code and message before anything is launched, and the Python layer answers bad arguments from tensor metadata
before it asks for a device.  No kernel is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def L():
    from convexadam_amd.csrc import build
    build.build()
    from convexadam_amd import _lib
    return _lib.lib()


def test_header_and_binding_declare_the_symbols(L):
    from convexadam_amd import _lib
    text = open(os.path.join(ROOT, "include", "convexadam_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in (("cvx_ranksum_critical_u2", 3), ("cvx_ranksum_better_f64", 11)):
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, src)
        assert decl, "%s is not declared in the header" % name
        assert name in _lib.SIGNATURES and hasattr(L, name)
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(decl.group(1).split(",")) == n_args
    assert _lib.SIGNATURES["cvx_ranksum_better_f64"][1][-1] is C.c_void_p                       # the stream
    assert _lib.SIGNATURES["cvx_ranksum_better_f64"][1][2:4] == [C.c_double, C.c_double]        # scale, sign
    assert re.search(r"#define\s+CVX_ABI_VERSION\s+2\b", src)
    assert L.cvx_version() == 2 == _lib.ABI_VERSION
    assert "ranksum.hip" in __import__("convexadam_amd.csrc.build", fromlist=["SOURCES"]).SOURCES
    block = text[text.index("csrc/ranksum.hip"):text.index("int cvx_ranksum_critical_u2")]
    for stated in ("U2 = 2 #{a > b} + #{a == b}", "s = U2 / 2 + S (S + 1) / 2", "z = (s - S (2 S + 1) / 2) / sqrt(S S (2 S + 1) / 12)",
                   "erfc(|z| / sqrt(2))", "x = sign * ((double) mean_i + scale * samples[r][i][k])", "[U2(r, i, j) >= u2_crit]"):
        assert stated in block, stated                              # the arithmetic is written out where the symbols are declared


def test_critical_u2_refusals(L):
    out = C.c_int(0)
    for S, p, word in ((0, 0.05, b"sample count"), (-3, 0.05, b"sample count"), (4097, 0.05, b"sample count"), (18, 0.0, b"p threshold"),
                       (18, 1.0, b"p threshold"), (18, -0.1, b"p threshold"), (18, 1.5, b"p threshold"), (18, NAN, b"p threshold"),
                       (18, INF, b"p threshold")):
        assert L.cvx_ranksum_critical_u2(S, p, C.byref(out)) == -1 and word in L.cvx_last_error(), (S, p, L.cvx_last_error())
    assert L.cvx_ranksum_critical_u2(18, 0.05, None) == -1 and b"null" in L.cvx_last_error()
    assert L.cvx_ranksum_critical_u2(1, 0.05, C.byref(out)) == 0 and out.value == 3              # "never" = 2 S^2 + 1
    assert L.cvx_ranksum_critical_u2(2, 0.05, C.byref(out)) == 0 and out.value == 9
    assert L.cvx_ranksum_critical_u2(4096, 0.05, C.byref(out)) == 0


def test_better_refusals(L):
    x, m, sc, u = C.c_void_p(1 << 24), C.c_void_p(2 << 24), C.c_void_p(3 << 24), C.c_void_p(4 << 24)
    R, N, S = 3, 5, 7

    def call(samples=x, means=m, scale=0.1, sign=1.0, ext=(R, N, S), crit=60, scores=sc, u2=u):
        return L.cvx_ranksum_better_f64(samples, means, scale, sign, *ext, crit, scores, u2, None)

    def refused(word, **kw):
        rc = call(**kw)
        msg = L.cvx_last_error()
        assert rc == -1 and word in msg, (kw, rc, msg)

    refused(b"null", samples=None)
    refused(b"null", scores=None)
    refused(b"null", samples=None, means=None, u2=None)
    for i in range(3):
        for bad in (0, -1):
            ext = [R, N, S]
            ext[i] = bad
            refused(b"extent", ext=tuple(ext))
    refused(b"extent", ext=(1, 4097, 7))
    refused(b"extent", ext=(1, 5, 4097))
    refused(b"2^31", ext=(129, 4096, 4096))                         # R N S = 2^31 + 2^24
    refused(b"2^31", ext=(128, 4096, 4096))                         # 2^31 exactly: one more than an int holds
    refused(b"2^31", ext=(129, 4096, 1))                            # R N N alone, with u2
    for crit in (-1, 2 * S * S + 2, 1 << 30):
        refused(b"threshold", crit=crit)
    for bad in (NAN, INF, -INF):
        refused(b"non-finite", scale=bad)
        refused(b"non-finite", sign=bad)
    refused(b"aligned", samples=C.c_void_p((1 << 24) + 4))
    refused(b"aligned", means=C.c_void_p((2 << 24) + 2))
    refused(b"aligned", scores=C.c_void_p((3 << 24) + 1))
    refused(b"aligned", u2=C.c_void_p((4 << 24) + 2))
    sbytes, obytes, ubytes = R * N * S * 8, R * N * 4, R * N * N * 4
    refused(b"overlap", scores=x)
    refused(b"overlap", scores=C.c_void_p((1 << 24) + sbytes - 4))                               # on the samples' last bytes
    refused(b"overlap", samples=C.c_void_p((3 << 24) + obytes - 4))                              # on the last score
    refused(b"overlap", u2=x)
    refused(b"overlap", u2=C.c_void_p((1 << 24) + sbytes - 4))
    refused(b"overlap", u2=sc)
    refused(b"overlap", scores=C.c_void_p((4 << 24) + ubytes - 4))                               # on u2's last element
    refused(b"overlap", scores=m)
    refused(b"overlap", u2=C.c_void_p((2 << 24) + N * 4 - 4))                                    # on the last mean
    # what is accepted never reaches this point without a device: the checks above are all there is before the launch


def test_python_layer_refuses_bad_arguments_before_the_device_check(L):
    from convexadam_amd import l2r3
    Z = torch.zeros
    bad = {
        "two_dims": lambda: l2r3.ranksum_better(Z(5, 7)),
        "four_dims": lambda: l2r3.ranksum_better(Z(1, 2, 5, 7)),
        "empty_axis": lambda: l2r3.ranksum_better(Z(2, 0, 7)),
        "too_many_teams": lambda: l2r3.ranksum_better(torch.empty(1, 4097, 1, device="meta")),
        "too_many_samples": lambda: l2r3.ranksum_better(torch.empty(1, 2, 4097, device="meta")),
        "too_many_elements": lambda: l2r3.ranksum_better(torch.empty(128, 4096, 4096, device="meta")),
        "too_many_u2": lambda: l2r3.ranksum_better(torch.empty(129, 4096, 1, device="meta"), return_u2=True),
        "means_shape": lambda: l2r3.ranksum_better(Z(2, 5, 7), means=Z(7)),
        "means_2d": lambda: l2r3.ranksum_better(Z(2, 5, 7), means=Z(5, 1)),
        "scale_nan": lambda: l2r3.ranksum_better(Z(2, 5, 7), means=Z(5), scale=NAN),
        "sign_inf": lambda: l2r3.ranksum_better(Z(2, 5, 7), means=Z(5), sign=INF),
        "p_zero": lambda: l2r3.ranksum_better(Z(2, 5, 7), p_threshold=0.0),
        "p_nan": lambda: l2r3.ranksum_better(Z(2, 5, 7), p_threshold=NAN),
        "critical_s": lambda: l2r3.critical_u2(0),
        "critical_s_large": lambda: l2r3.critical_u2(4097),
        "critical_p": lambda: l2r3.critical_u2(18, 1.0),
        "scores_better_3d": lambda: l2r3.scores_better(Z(1, 5, 7)),
        "rank_no_teams": lambda: l2r3.rank_experiments({"metrics": {"sim1": "DSC", "smooth": "LogJacDetStd"}}),
        "rank_noise_shape": lambda: l2r3.rank_experiments(_tiny_data(), noise=np.zeros((4, 50, 3, 2))),
        "rank_repeats": lambda: l2r3.rank_experiments(_tiny_data(), repeats=0),
        "configure_no_pairs": lambda: l2r3.self_configure([], (32, 40, 48)),
        "configure_sim2": lambda: l2r3.self_configure([{}], (32, 40, 48), sim2="NCC"),
        "configure_pair_keys": lambda: l2r3.self_configure([{"fixed": Z(4, 4, 4)}], (32, 40, 48)),
    }
    for name in sorted(bad):
        with pytest.raises(ValueError):
            bad[name]()
            pytest.fail("%s was accepted" % name)
    with pytest.raises(TypeError):
        l2r3.ranksum_better(np.zeros((2, 5, 7)))
    with pytest.raises(TypeError):
        l2r3.ranksum_better(Z(2, 5, 7), means=[0.0] * 5)
    # valid arguments on the CPU reach the device check: there is no CPU path
    for ok in (lambda: l2r3.ranksum_better(Z(2, 5, 7)), lambda: l2r3.ranksum_better(Z(2, 5, 7), means=Z(5), return_u2=True),
               lambda: l2r3.scores_better(Z(5, 7))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            ok()


def _tiny_data():
    team = {"time": 1.0, "sim1": {"mean": 0.5, "std": 0.0, "30": 0.4}, "smooth": {"mean": 0.1, "std": 0.0, "30": 0.1}}
    return {"metrics": {"sim1": "DSC", "smooth": "LogJacDetStd", "sim2": None}, "MIND; a": team, "MIND; b": team, "nnUNet; c": team}
