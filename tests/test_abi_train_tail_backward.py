"""CPU suite: the tail's routed and fused backward are declared in include/mms_train_tail_backward.h (valid C), exported
by the built library with the declared argument lists and bound by mms_answer_selection_amd/train_tail_backward.py;
include/mms.h, capi.py, include/mms_train_tail.h's declaration set and the ABI version are as they were; the refusals are
mms_train_tail_backward_f32's, in its order, on both new calls, without a GPU -- nothing is enqueued on any of these
paths; the workspace queries; and the plan of csrc/train_tail_backward_plans.h, swept by a host program under
AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import test_abi_train_tail as A
import train_tail_backward_cases as B
import train_tail_reference as R
from conftest import ROOT

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 3
NEW = ["mms_train_tail_backward_routed_f32", "mms_train_tail_backward_fused_f32"]
OLD = "mms_train_tail_backward_f32"
QUERIES = ["mms_train_tail_backward_workspace_bytes", "mms_train_tail_backward_fused_workspace_bytes"]
BWD, BWD_OUTPUTS, BIG, WS = A.BWD, A.BWD_OUTPUTS, A.BIG, A.WS
_shape, _distinct, bwd = A._shape, A._distinct, A.bwd


@pytest.fixture(scope="module")
def tb(hiplib):
    from mms_answer_selection_amd import train_tail, train_tail_backward
    train_tail.lib()
    train_tail_backward.lib()
    return train_tail_backward


@pytest.fixture(scope="module")
def tail(tb):
    from mms_answer_selection_amd import train_tail
    return train_tail


def _declarations(name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    out = {}
    for ret, fn, params in re.findall(r"\b(int|size_t)\s+(mms_\w+)\s*\(([^)]*)\)\s*;", txt):
        out[fn] = [re.sub(r"\s*\w+$", "", " ".join(p.split())) for p in params.split(",")]
    return out


def test_every_declared_name_is_exported_with_the_declared_argument_list(tb, tail, hiplib):
    decl = _declarations("mms_train_tail_backward.h")
    assert sorted(decl) == sorted(NEW + QUERIES + ["mms_train_tail_backward_route"])
    assert sorted(tb.EXPORTED_SYMBOLS) == sorted(decl)
    so = open(os.path.join(ROOT, "mms_answer_selection_amd", "libmms_hip.so"), "rb").read()
    ctype = {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t}
    for n, params in decl.items():
        assert hasattr(hiplib, n) and n.encode() in so, n
        bound = getattr(tb.lib(), n).argtypes
        assert len(bound) == len(params), n
        for b, p in zip(bound, params):
            if p == "const mms_score_tail_shape*":
                assert b is C.POINTER(tail.TrainTailShape), (n, p)
            elif p.endswith("*"):
                assert b is C.c_void_p, (n, p)
            else:
                assert b is ctype[p], (n, p)
    old = _declarations("mms_train_tail.h")[OLD]
    for n in NEW:
        assert decl[n] == old, n


def test_header_is_c():
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I",
                           os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "train_tail_backward_abi_is_c.c")])


def test_the_frozen_surface_is_untouched(tb, tail, hiplib):
    from mms_answer_selection_amd import capi
    assert "mms_train_tail_" not in open(os.path.join(ROOT, "include", "mms.h")).read()
    assert not [n for n in dir(capi) if "train_tail" in n]
    assert not [n for n in capi.EXPORTED_SYMBOLS if "train_tail" in n]
    assert hiplib.mms_version() == 212 and capi.MMS_VERSION == 212
    assert sorted(_declarations("mms_train_tail.h")) == sorted(A.FORWARDS + A.BACKWARDS + A.QUERIES + ["mms_train_tail_route"])
    assert sorted(tail.EXPORTED_SYMBOLS) == sorted(_declarations("mms_train_tail.h"))
    assert not [n for n in tail.EXPORTED_SYMBOLS if n in tb.EXPORTED_SYMBOLS]


def test_refusals_are_the_existing_calls_in_its_order(tb, tail, hiplib):
    """Every refused shape, the phase, the dropout ratio, a NULL input, no output, two arrays at one address and the
    workspace: each new call returns what mms_train_tail_backward_f32 returns."""
    for shape, code in A._refused(tail):
        sp = C.byref(shape)
        assert hiplib.mms_train_tail_backward_route(sp) == tail.ROUTE_NONE
        assert all(getattr(hiplib, q)(sp) == 0 for q in QUERIES)
        for n in NEW:
            assert bwd(hiplib, n, sp, [None] * len(BWD), None, 0) == code == bwd(hiplib, OLD, sp, [None] * len(BWD), None, 0)
            assert bwd(hiplib, n, sp, _distinct(BWD)) == code, n
    assert hiplib.mms_train_tail_backward_route(None) == tail.ROUTE_NONE
    sp = C.byref(_shape(tail))
    for n in NEW:
        assert bwd(hiplib, n, None, _distinct(BWD)) == INVALID
        for kw in (dict(phase=A.TEST), dict(phase=2), dict(ratio=0.0), dict(ratio=1.0)):
            assert bwd(hiplib, n, sp, _distinct(BWD), **kw) == INVALID, (n, kw)
            assert bwd(hiplib, n, sp, [None] * len(BWD), None, 0, **kw) == INVALID, (n, kw)
    for t, pool in A.TAILS + ((R.v4(256), R.MAX), (R.small(65), R.MAX)):
        sp = C.byref(_shape(tail, t, pool))
        for n, query in zip(NEW, QUERIES):
            need = getattr(hiplib, query)(sp)
            reached = hiplib.mms_train_tail_backward_fused_workspace_bytes(sp) > 0
            for k in BWD[:16]:
                a = _distinct(BWD)
                a[BWD.index(k)] = None
                if k == "shift" and pool == R.AVE:
                    continue                           # a valid call: not made without a GPU
                assert bwd(hiplib, n, sp, a) == INVALID == bwd(hiplib, OLD, sp, a), (n, k)
                assert bwd(hiplib, n, sp, a, None, 0) == INVALID, (n, k)          # before UNSUPPORTED and the workspace
            a = _distinct(BWD)
            for k in BWD_OUTPUTS:
                a[BWD.index(k)] = None
            assert bwd(hiplib, n, sp, a) == INVALID, n                            # no output at all
            for i in range(len(BWD)):
                for j in range(i):
                    a = _distinct(BWD)
                    a[i] = a[j]
                    assert bwd(hiplib, n, sp, a) == INVALID, (n, BWD[i], BWD[j])
                a = _distinct(BWD)
                assert bwd(hiplib, n, sp, a, a[i], BIG) == INVALID, (n, BWD[i])
            a = _distinct(BWD)
            if n.endswith("fused_f32") and not reached:
                assert need == 0 and bwd(hiplib, n, sp, a, None, 0) == UNSUPPORTED == bwd(hiplib, n, sp, a, WS, BIG)
                continue
            assert need > 0
            assert bwd(hiplib, n, sp, a, None, need) == WORKSPACE
            assert bwd(hiplib, n, sp, a, WS, need - 1) == WORKSPACE
    for t in (R.v4(0), R.small(0)):
        for n in NEW:
            assert bwd(hiplib, n, C.byref(_shape(tail, t)), [None] * len(BWD), None, 0) == OK


def test_workspace_queries_and_reach(tb, tail, hiplib):
    """The routed query never falls below mms_train_tail_workspace_bytes; the fused query is 0 exactly where the forced
    call says MMS_ERR_UNSUPPORTED; every FUSED answer of the route is a shape the fused launches reach."""
    tails = R.GPU_TAILS + B.PARITY_TAILS + [B.PAST_N, R.v4(100), R.v4(256), R.v4(257), R.v4(400), R.v5(256), R.v5(1517),
                                            R.Tail(R.v4(50).stage, 2, 65, 2), R.Tail(R.v4(50).stage, 65, 32, 2)]
    reached = 0
    for pool in R.POOLS:
        for t in tails:
            shape = _shape(tail, t, pool)
            sp = C.byref(shape)
            step, routed = tail.train_tail_workspace_bytes(shape), tb.train_tail_backward_workspace_bytes(shape)
            fused = tb.train_tail_backward_workspace_bytes(shape, "fused")
            assert routed >= step > 0, (t, pool)
            rc = bwd(hiplib, NEW[1], sp, _distinct(BWD), None, 0)
            assert (fused == 0) == (rc == UNSUPPORTED) and rc in (UNSUPPORTED, WORKSPACE), (t, pool, fused, rc)
            route = tb.train_tail_backward_route(shape)
            assert route in (tb.ROUTE_SEQUENCE, tb.ROUTE_FUSED)
            if route == tb.ROUTE_FUSED:
                assert fused > 0 and routed >= fused, (t, pool)
            else:
                assert routed == step, (t, pool)
            s = t.stage.conv
            within = (1 <= s.N <= 256 and s.stride == 1 and s.pad == 0 and t.H <= 64 and s.K + t.F1 <= 128)
            assert (fused > 0) == within, (t, pool)
            reached += fused > 0
    assert reached > 20


def test_binding_refuses_before_the_library(tb):
    import torch
    from mms_answer_selection_amd import capi
    x, w, k = torch.zeros(3, 2, 3, 3), torch.zeros(3, 2, 2, 2), torch.zeros(3)
    args = [x, w, 2, tb.POOL_AVE, torch.zeros(3, 3, 2, 2), torch.zeros(3, 3), torch.zeros(3, 3), k, k, k, k, torch.zeros(3, 2),
            torch.zeros(4, 5), torch.zeros(2, 4), torch.zeros(3, 4, dtype=torch.int32), torch.zeros(3, 4), torch.zeros(3, 2),
            torch.zeros(3)]
    with pytest.raises(capi.MMSArgumentError):
        tb.train_tail_backward_routed(*args)                                       # no output
    with pytest.raises(capi.MMSArgumentError):
        tb.train_tail_backward_routed(*args, bottom_diff=torch.zeros(3, 2, 3, 2))
    with pytest.raises(capi.MMSArgumentError):
        tb.train_tail_backward_routed(*args, bottom_diff=torch.zeros_like(x), route="sequence")
    with pytest.raises(capi.MMSError):
        tb.train_tail_backward_fused(*args, bottom_diff=torch.zeros_like(x))       # host tensors: there is no CPU path


# ---- the plan, from the C++ --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plans_host(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is part of the image"
    exe = tmp_path_factory.mktemp("ttb_plans") / "train_tail_backward_plans_host"
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "mms_answer_selection_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "train_tail_backward_plans_host.cpp"), "-o", str(exe)])
    return str(exe)


def run_host(exe, args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "every plan holds its invariants" in out.stdout
    return out.stdout


def test_the_plan_holds_its_invariants_over_the_sweep(plans_host):
    out = run_host(plans_host, ["--sweep"])
    n = {k: int(v) for k, v in re.findall(r"count (\w+)=(\d+)", out)}
    assert n["shapes"] > 100000
    for branch in ("reached", "reached_not_routed", "past_n", "past_head", "past_channels", "past_image", "several_slabs", "long_slabs",
                   "chunked"):
        assert n.get(branch, 0) > 0, (branch, n)


def test_the_listed_tails_take_the_plans_the_gpu_suite_counts_on(plans_host, tb, tail):
    """TWO_CHUNKS is cut into two chunks of input channels by the bottom_diff plan; one image per workgroup; N = 256 is
    64 slabs of four units; the library's fused query is the plan's bytes less the head's part."""
    args = lambda t: [getattr(t.stage.conv, k) for k in ("N", "C", "H", "W", "K", "kh", "kw")] + [t.F1, t.H, t.C]  # noqa: E731
    tails = [B.TWO_CHUNKS, R.v4(50), R.small(256), R.small(65), B.PAST_N, R.PAST_H]
    out = run_host(plans_host, [v for t in tails for v in args(t)])
    plans = [dict(kv.split("=") for kv in line.split()[1:]) for line in out.splitlines() if line.startswith("plan ")]
    assert len(plans) == len(tails)
    p = dict(zip(("two", "v4", "s256", "s65", "past_n", "past_h"), plans))
    assert p["two"]["ok"] == "1" and p["two"]["chunks"] == "2"
    assert p["v4"]["ok"] == "1" and int(p["v4"]["chunks"]) > 2 and p["v4"]["slabs"] == "50" and p["v4"]["ups"] == "1"
    assert p["s256"]["slabs"] == "64" and p["s256"]["ups"] == "4" and p["s65"]["slabs"] == "33" and p["s65"]["ups"] == "2"
    assert p["past_n"]["ok"] == "0" and p["past_h"]["ok"] == "0"
    for key in ("two", "v4", "s256", "s65"):
        assert p[key]["bottom_G"] == p[key]["wdiff_G"] == "1"
    from mms_answer_selection_amd import head
    r16 = lambda v: (v + 15) // 16 * 16                                             # noqa: E731
    for t, key in ((B.TWO_CHUNKS, "two"), (R.v4(50), "v4"), (R.small(256), "s256")):
        hb = head.head_workspace_bytes(head.head_shape(*R.head_shape(t), phase=head.TRAIN))
        want = int(p[key]["bytes"]) + r16(hb)
        assert tb.train_tail_backward_workspace_bytes(_shape(tail, t, R.AVE), "fused") == want, key
