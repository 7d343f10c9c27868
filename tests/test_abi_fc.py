"""CPU suite: the InnerProduct, Softmax, SoftmaxWithLoss and Concat calls are declared in include/mms_fc.h (valid C),
exported by the built library and bound by mms_answer_selection_amd/fc.py; include/mms.h, capi.py and the ABI version
are as they were; every row of the header's refusal table holds without a GPU -- nothing is enqueued on any of these
paths, the arrays are NULL or addresses that are never touched; the workspace queries are the model's and 0 for refused
shapes; and the plan header (csrc/fc_plans.h) holds its invariants in a host program built with AddressSanitizer and
UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import fc_reference as R
from conftest import ROOT

OK, INVALID, UNSUPPORTED, WORKSPACE = R.OK, R.INVALID, R.UNSUPPORTED, R.WORKSPACE
BASE = 1 << 30                            # stands for arrays that are never touched: every call here returns first
GAP = 1 << 26                             # between two of them: more than any array of these shapes
A = [BASE + i * GAP for i in range(12)]
INT_MAX = 2 ** 31 - 1
BIG = 1 << 40
SIZES = [("f32", 4), ("f64", 8)]


@pytest.fixture(scope="module")
def fc(hiplib):
    from mms_answer_selection_amd import fc
    fc.lib()
    return fc


def _header():
    return open(os.path.join(ROOT, "include", "mms_fc.h")).read()


def _declared():
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return sorted(set(re.findall(r"\b(mms_\w+)\s*\(", txt)))


PREFIXES = ("mms_inner_product_", "mms_softmax_", "mms_concat_")


def test_every_declared_name_is_exported_and_bound(fc, hiplib):
    names = _declared()
    assert len(names) == 23 and all(n.startswith(PREFIXES) for n in names), names
    assert sorted(fc.EXPORTED_SYMBOLS) == names
    so = open(os.path.join(ROOT, "mms_answer_selection_amd", "libmms_hip.so"), "rb").read()
    for n in names:
        assert hasattr(hiplib, n) and n.encode() in so, n
        assert getattr(fc.lib(), n).argtypes is not None, n
    for stem in ("inner_product", "softmax", "softmax_loss", "concat"):
        for f in (stem + "_forward", stem + "_backward", stem + "_forward_f64", stem + "_backward_f64"):
            assert callable(getattr(fc, f)), f


def test_header_is_c():
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I",
                           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "fc_abi_is_c.c")])


def test_the_frozen_surface_is_untouched(fc, hiplib):
    from mms_answer_selection_amd import capi
    mms_h = open(os.path.join(ROOT, "include", "mms.h")).read()
    for word in PREFIXES + ("MMS_FC_", "MMS_LOSS_NORM", "MMS_CONCAT"):
        assert word not in mms_h, word
    assert not [n for n in capi.EXPORTED_SYMBOLS if n.startswith(PREFIXES)]
    assert not [n for n in dir(capi) if n.startswith(("inner_product", "softmax_", "concat_"))]
    assert hiplib.mms_version() == 212 and capi.MMS_VERSION == 212


def test_the_constants_are_the_headers(fc):
    defs = {k: int(v.strip("()")) for k, v in re.findall(r"#define\s+(MMS_\w+)\s+(\(?-?\d+\)?)", _header())}
    assert defs == dict(MMS_FC_PASS_FORWARD=fc.PASS_FORWARD, MMS_FC_PASS_BACKWARD=fc.PASS_BACKWARD, MMS_FC_ROUTE_NONE=fc.ROUTE_NONE, MMS_FC_ROUTE_GENERIC=fc.ROUTE_GENERIC, MMS_FC_ROUTE_FAST=fc.ROUTE_FAST,
                        MMS_LOSS_NORM_FULL=fc.NORM_FULL, MMS_LOSS_NORM_VALID=fc.NORM_VALID,
                        MMS_LOSS_NORM_BATCH_SIZE=fc.NORM_BATCH_SIZE, MMS_LOSS_NORM_NONE=fc.NORM_NONE,
                        MMS_CONCAT_MAX_BOTTOMS=fc.CONCAT_MAX_BOTTOMS)
    head = {k: int(v) for k, v in re.findall(r"#define\s+(MMS_HEAD_NORM_\w+)\s+(\d+)",
                                             open(os.path.join(ROOT, "include", "mms_head.h")).read())}
    assert head == {k.replace("LOSS", "HEAD"): v for k, v in defs.items() if k.startswith("MMS_LOSS_NORM")}
    assert (R.FULL, R.VALID, R.BATCH_SIZE, R.NONE) == (fc.NORM_FULL, fc.NORM_VALID, fc.NORM_BATCH_SIZE, fc.NORM_NONE)
    assert R.MAX_BOTTOMS == fc.CONCAT_MAX_BOTTOMS


# ---- InnerProduct ----------------------------------------------------------------------------------------------------
def ips(fc, M=50, K=66, N=32, transpose=0, bias=1):
    return fc.InnerProductShape(M, K, N, transpose, bias)


BAD_IP = [dict(M=-1), dict(K=0), dict(K=-3), dict(N=0), dict(N=-1), dict(transpose=2), dict(transpose=-1), dict(bias=2),
          dict(M=46341, K=46341), dict(M=46341, N=46341), dict(K=46341, N=46341), dict(M=INT_MAX, K=2, N=1)]


def test_inner_product_queries(fc, hiplib):
    for M, K, N in [(50, 66, 32), (1, 1, 1), (129, 3, 2), (8193, 2, 2), (1517, 205, 64)]:
        sp = C.byref(ips(fc, M, K, N))
        assert hiplib.mms_inner_product_workspace_bytes(sp) == R.ip_workspace_bytes(M, K, N, 4)
        assert hiplib.mms_inner_product_workspace_bytes_f64(sp) == R.ip_workspace_bytes(M, K, N, 8)
        for p in (R.FORWARD, R.BACKWARD):
            assert hiplib.mms_inner_product_route(sp, p) == R.ip_route(M, K, N, p), (M, K, N, p)
    for bad in BAD_IP + [dict(M=0)]:
        sp = C.byref(ips(fc, **bad))
        assert hiplib.mms_inner_product_workspace_bytes(sp) == 0, bad
        assert hiplib.mms_inner_product_workspace_bytes_f64(sp) == 0, bad
    for bad in BAD_IP:
        assert hiplib.mms_inner_product_route(C.byref(ips(fc, **bad)), R.FORWARD) == R.ROUTE_NONE, bad
        assert hiplib.mms_inner_product_route(C.byref(ips(fc, **bad)), R.BACKWARD) == R.ROUTE_NONE, bad
    assert hiplib.mms_inner_product_workspace_bytes(None) == 0 and hiplib.mms_inner_product_route(None, R.FORWARD) == R.ROUTE_NONE
    route = lambda M, K, N, p: hiplib.mms_inner_product_route(C.byref(ips(fc, M, K, N)), p)
    assert route(32, 32, 2, R.FORWARD) == R.ROUTE_FAST and route(31, 32, 2, R.FORWARD) == R.ROUTE_GENERIC      # multiply-adds
    assert route(50, 128, 32, R.FORWARD) == R.ROUTE_FAST and route(50, 127, 32, R.FORWARD) == R.ROUTE_GENERIC  # a wide top: K
    assert route(50, 66, 16, R.FORWARD) == R.ROUTE_FAST and route(50, 66, 17, R.FORWARD) == R.ROUTE_GENERIC    # the narrow tile
    assert route(129, 66, 32, R.BACKWARD) == R.ROUTE_FAST and route(128, 66, 32, R.BACKWARD) == R.ROUTE_GENERIC  # slabs
    assert route(129, 3, 5, R.BACKWARD) == R.ROUTE_GENERIC                                                      # multiply-adds
    for p in (-1, 2):
        assert route(50, 66, 32, p) == R.ROUTE_NONE


@pytest.mark.parametrize("name,size", [("mms_inner_product_forward_f32", 4), ("mms_inner_product_forward_f64", 8),
                                       ("mms_inner_product_forward_generic_f32", 4)])
def test_inner_product_forward_refusals(fc, hiplib, name, size):
    fn = getattr(hiplib, name)
    x, w, b, top = A[:4]
    for bad in BAD_IP:
        assert fn(C.byref(ips(fc, **bad)), x, w, b, top, None) == INVALID, bad
    assert fn(None, x, w, b, top, None) == INVALID
    sp = C.byref(ips(fc))
    for ptrs in ((None, w, b, top), (x, None, b, top), (x, w, None, top), (x, w, b, None)):
        assert fn(sp, *ptrs, None) == INVALID, ptrs
    assert fn(C.byref(ips(fc, M=0)), None, None, None, None, None) == OK
    assert fn(C.byref(ips(fc, M=0, K=0)), None, None, None, None, None) == INVALID
    nx, nw, nt = 50 * 66 * size, 66 * 32 * size, 50 * 32 * size
    for t in (x, x + nx - size, x - nt + size, w, w + nw - size, b, b + 31 * size, b - nt + size):
        assert fn(sp, x, w, b, t, None) == INVALID, t - BASE
    # without a bias term b is not looked at
    assert fn(C.byref(ips(fc, M=0, bias=0)), None, None, None, None, None) == OK


@pytest.mark.parametrize("name,size", [("mms_inner_product_backward_f32", 4), ("mms_inner_product_backward_f64", 8),
                                       ("mms_inner_product_backward_generic_f32", 4)])
def test_inner_product_backward_refusals(fc, hiplib, name, size):
    fn = getattr(hiplib, name)
    x, w, td, dw, db, dx, ws = A[:7]
    for bad in BAD_IP:
        assert fn(C.byref(ips(fc, **bad)), x, w, td, dw, db, dx, ws, BIG, None) == INVALID, bad
    assert fn(None, x, w, td, dw, db, dx, ws, BIG, None) == INVALID
    sp = C.byref(ips(fc))
    need = R.ip_workspace_bytes(50, 66, 32, size)
    assert fn(sp, x, w, None, dw, db, dx, ws, BIG, None) == INVALID
    assert fn(sp, None, w, td, dw, db, dx, ws, BIG, None) == INVALID               # w_diff needs x
    assert fn(sp, x, None, td, dw, db, dx, ws, BIG, None) == INVALID               # bottom_diff needs w
    assert fn(sp, x, w, td, None, None, None, ws, BIG, None) == INVALID            # no output at all
    assert fn(C.byref(ips(fc, bias=0)), x, w, td, dw, db, dx, ws, BIG, None) == INVALID    # b_diff without a bias term
    assert fn(C.byref(ips(fc, M=0)), None, None, None, None, None, None, None, 0, None) == OK
    # the workspace: needed for w_diff and b_diff only
    assert fn(sp, x, w, td, dw, db, dx, None, BIG, None) == WORKSPACE
    assert fn(sp, x, w, td, dw, db, dx, ws, need - 1, None) == WORKSPACE
    assert fn(sp, x, w, td, None, db, None, ws, need - 1, None) == WORKSPACE
    assert fn(sp, x, w, td, dw, None, None, ws, 0, None) == WORKSPACE
    # outputs over inputs and over each other
    nx, nw, nt = 50 * 66 * size, 66 * 32 * size, 50 * 32 * size
    assert fn(sp, x, w, td, x, db, dx, ws, BIG, None) == INVALID
    assert fn(sp, x, w, td, dw, db, dw + nw - size, ws, BIG, None) == INVALID
    assert fn(sp, x, w, td, dw, dw + size, dx, ws, BIG, None) == INVALID
    assert fn(sp, x, w, td, dw, db, td - nx + size, ws, BIG, None) == INVALID
    assert fn(sp, x, w, td, dw, db, w, ws, BIG, None) == INVALID
    assert fn(sp, x, w, td, dw, db, dx, dx + nx - size, BIG, None) == INVALID      # the workspace over bottom_diff
    assert fn(sp, x, w, td, dw, db, dx, td + nt - size, BIG, None) == INVALID      # ... over top_diff


# ---- Softmax, SoftmaxWithLoss ----------------------------------------------------------------------------------------
BAD_SM = [(-1, 3, 1), (4, 0, 1), (4, -2, 1), (4, 3, 0), (4, 3, -1), (46341, 1, 46341), (2 ** 20, 2 ** 11, 1),
          (2 ** 16, 3, 2 ** 16)]


@pytest.mark.parametrize("suffix,size", SIZES)
def test_softmax_refusals(fc, hiplib, suffix, size):
    fwd, bwd = getattr(hiplib, "mms_softmax_forward_" + suffix), getattr(hiplib, "mms_softmax_backward_" + suffix)
    x, y, z = A[:3]
    for bad in BAD_SM:
        sp = C.byref(fc.SoftmaxShape(*bad))
        assert fwd(sp, x, y, None) == INVALID and bwd(sp, x, y, z, None) == INVALID, bad
    assert fwd(None, x, y, None) == INVALID and bwd(None, x, y, z, None) == INVALID
    sp, n = C.byref(fc.SoftmaxShape(4, 3, 5)), 60 * size
    zero = C.byref(fc.SoftmaxShape(0, 3, 5))
    assert fwd(zero, None, None, None) == OK and bwd(zero, None, None, None, None) == OK
    assert fwd(sp, None, y, None) == INVALID and fwd(sp, x, None, None) == INVALID
    for ptrs in ((None, y, z), (x, None, z), (x, y, None)):
        assert bwd(sp, *ptrs, None) == INVALID
    for d in (0, size, n - size, -size, -n + size):
        assert fwd(sp, x, x + d, None) == INVALID, d
        assert bwd(sp, x, y, x + d, None) == INVALID, d                            # bottom_diff over top
        assert bwd(sp, x, x + d, z, None) == INVALID, d                            # top_diff over top
        if d:
            assert bwd(sp, x, y, y + d, None) == INVALID, d                        # partly over top_diff


def sls(fc, outer=50, channels=3, inner=2, norm=R.VALID, has_ignore=0, ignore=0):
    return fc.SoftmaxLossShape(outer, channels, inner, norm, has_ignore, ignore)


@pytest.mark.parametrize("suffix,size", SIZES)
def test_softmax_loss_refusals_and_queries(fc, hiplib, suffix, size):
    fwd = getattr(hiplib, "mms_softmax_loss_forward_" + suffix)
    bwd = getattr(hiplib, "mms_softmax_loss_backward_" + suffix)
    query = getattr(hiplib, "mms_softmax_loss_workspace_bytes" + ("" if size == 4 else "_f64"))
    x, lab, prob, loss, ws = A[:5]
    lw = C.c_float(1.0) if size == 4 else C.c_double(1.0)
    bad_shapes = [sls(fc, *b) for b in BAD_SM] + [sls(fc, norm=4), sls(fc, norm=-1)]
    for s in bad_shapes:
        assert fwd(C.byref(s), x, lab, prob, loss, ws, BIG, None) == INVALID
        assert bwd(C.byref(s), prob, lab, lw, x, ws, BIG, None) == INVALID
        assert query(C.byref(s)) == 0
    assert fwd(None, x, lab, prob, loss, ws, BIG, None) == INVALID and query(None) == 0
    assert bwd(None, prob, lab, lw, x, ws, BIG, None) == INVALID
    for outer, inner in [(50, 2), (1, 1), (64, 1), (65, 1), (1517, 1), (300, 70)]:
        assert query(C.byref(sls(fc, outer, 3, inner))) == R.loss_workspace_bytes(outer * inner, size)
    zero = C.byref(sls(fc, outer=0))
    assert query(zero) == 0 and fwd(zero, None, None, None, None, None, 0, None) == OK
    assert bwd(zero, None, None, lw, None, None, 0, None) == OK
    sp, need = C.byref(sls(fc)), R.loss_workspace_bytes(100, size)
    for ptrs in ((None, lab, prob, loss), (x, None, prob, loss), (x, lab, None, loss), (x, lab, prob, None)):
        assert fwd(sp, *ptrs, ws, BIG, None) == INVALID
    assert bwd(sp, None, lab, lw, x, ws, BIG, None) == INVALID and bwd(sp, prob, None, lw, x, ws, BIG, None) == INVALID
    assert bwd(sp, prob, lab, lw, None, ws, BIG, None) == INVALID
    assert fwd(sp, x, lab, prob, loss, None, BIG, None) == WORKSPACE
    assert fwd(sp, x, lab, prob, loss, ws, need - 1, None) == WORKSPACE
    assert bwd(sp, prob, lab, lw, x, None, BIG, None) == WORKSPACE
    assert bwd(sp, prob, lab, lw, x, ws, need - 1, None) == WORKSPACE
    n = 300 * size
    assert fwd(sp, x, lab, x, loss, ws, BIG, None) == INVALID
    assert fwd(sp, x, lab, x + n - size, loss, ws, BIG, None) == INVALID
    assert fwd(sp, x, lab, prob, lab, ws, BIG, None) == INVALID
    assert fwd(sp, x, lab, prob, prob + size, ws, BIG, None) == INVALID
    assert fwd(sp, x, lab, prob, loss, prob + n - size, BIG, None) == INVALID
    assert bwd(sp, prob, lab, lw, prob, ws, BIG, None) == INVALID
    assert bwd(sp, prob, lab, lw, lab - n + size, ws, BIG, None) == INVALID
    assert bwd(sp, prob, lab, lw, x, x + n - size, BIG, None) == INVALID


# ---- Concat ----------------------------------------------------------------------------------------------------------
def ccs(fc, num_concats=7, inner=5, ext=(1, 3, 4, 64)):
    return fc.ConcatShape(num_concats, inner, len(ext), (C.c_int * 8)(*ext[:8]))


def ptr_array(ptrs):
    return (C.c_void_p * max(len(ptrs), 1))(*ptrs)


@pytest.mark.parametrize("suffix,size", SIZES)
def test_concat_refusals(fc, hiplib, suffix, size):
    fwd, bwd = getattr(hiplib, "mms_concat_forward_" + suffix), getattr(hiplib, "mms_concat_backward_" + suffix)
    top = A[9]
    four = ptr_array(A[:4])
    bad = [ccs(fc, num_concats=-1), ccs(fc, inner=0), ccs(fc, inner=-1), ccs(fc, ext=()), ccs(fc, ext=(1, -1, 3)),
           ccs(fc, ext=(0, 0)), ccs(fc, num_concats=2 ** 20, inner=2 ** 11), ccs(fc, ext=(INT_MAX, 1)),
           ccs(fc, num_concats=1, inner=2 ** 16, ext=(2 ** 15,))]
    nine = fc.ConcatShape(7, 5, 9, (C.c_int * 8)(1, 1, 1, 1, 1, 1, 1, 1))
    for s in bad + [nine]:
        assert fwd(C.byref(s), ptr_array(A[:8]), top, None) == INVALID
        assert bwd(C.byref(s), top, ptr_array(A[:8]), None) == INVALID
    assert fwd(None, four, top, None) == INVALID and bwd(None, top, four, None) == INVALID
    sp = C.byref(ccs(fc))
    assert fwd(sp, None, top, None) == INVALID and fwd(sp, four, None, None) == INVALID
    assert bwd(sp, None, four, None) == INVALID and bwd(sp, top, None, None) == INVALID
    zero = C.byref(ccs(fc, num_concats=0))
    assert fwd(zero, None, None, None) == OK and bwd(zero, None, None, None) == OK
    assert fwd(sp, ptr_array([A[0], None, A[2], A[3]]), top, None) == INVALID      # a NULL bottom of extent 3
    assert bwd(sp, top, ptr_array([None] * 4), None) == INVALID                    # a backward with no diff
    # a bottom that aliases top: at its start, at its end, the smallest bottom on its last element
    nt = 7 * 72 * 5 * size
    for i, nbot in enumerate((1, 3, 4, 64)):
        nb = 7 * nbot * 5 * size
        for alias in (top, top + nt - size, top - nb + size):
            ptrs = list(A[:4])
            ptrs[i] = alias
            assert fwd(sp, ptr_array(ptrs), top, None) == INVALID, (i, alias - top)
            assert bwd(sp, top, ptr_array(ptrs), None) == INVALID, (i, alias - top)
    # two bottom diffs overlapping; two bottoms may be one array (they are only read)
    assert bwd(sp, top, ptr_array([A[0], A[0], A[2], A[3]]), None) == INVALID
    assert bwd(sp, top, ptr_array([A[0], A[1], A[2], A[2] + 7 * 4 * 5 * size - size]), None) == INVALID
    # an extent of 0 is not looked at
    s0 = C.byref(ccs(fc, num_concats=0, ext=(2, 0, 3)))
    assert fwd(s0, None, None, None) == OK


def test_binding_refuses_before_the_library(fc):
    import torch
    from mms_answer_selection_amd import capi
    x, w = torch.zeros(4, 3), torch.zeros(2, 3)
    with pytest.raises(capi.MMSError, match="GPU memory"):
        fc.inner_product_forward(x, w)                                             # host tensors: there is no CPU path
    with pytest.raises(capi.MMSArgumentError):
        fc.inner_product_forward(x.half(), w.half())
    with pytest.raises(capi.MMSArgumentError):
        fc.inner_product_forward(x, torch.zeros(2, 4))
    with pytest.raises(capi.MMSArgumentError):
        fc.inner_product_forward(x, w, torch.zeros(3))
    with pytest.raises(capi.MMSArgumentError):
        fc.inner_product_forward(x, w, route="fast")
    with pytest.raises(capi.MMSArgumentError):
        fc.inner_product_backward(x, w, torch.zeros(4, 2))
    with pytest.raises(capi.MMSArgumentError):
        fc.inner_product_backward(x, w, torch.zeros(4, 2), w_diff=torch.zeros(3, 2))
    with pytest.raises(capi.MMSArgumentError):
        fc.softmax_forward(x, axis=2)
    with pytest.raises(capi.MMSArgumentError):
        fc.softmax_forward(x, out=torch.zeros(3, 4))
    with pytest.raises(capi.MMSError, match="GPU memory"):
        fc.softmax_forward(x)
    with pytest.raises(capi.MMSArgumentError):
        fc.softmax_loss_forward(x, torch.zeros(3))
    with pytest.raises(capi.MMSArgumentError):
        fc.concat_forward([])
    with pytest.raises(capi.MMSArgumentError):
        fc.concat_forward([x] * 9)
    with pytest.raises(capi.MMSArgumentError):
        fc.concat_forward([x, torch.zeros(5, 3)])
    with pytest.raises(capi.MMSArgumentError):
        fc.concat_backward(torch.zeros(4, 6), [(4, 3), (4, 2)])
    with pytest.raises(capi.MMSError, match="GPU memory"):
        fc.concat_forward([x, x])


# ---- the plans, from the C++ -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plans_host(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is part of the image"
    exe = tmp_path_factory.mktemp("fc_plans") / "fc_plans_host"
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "mms_answer_selection_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "fc_plans_host.cpp"), "-o", str(exe)])
    return str(exe)


def run_host(exe, args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "every plan holds its invariants" in out.stdout
    return out.stdout


def test_the_plans_hold_their_invariants_over_the_sweep(plans_host):
    out = run_host(plans_host, ["--sweep"])
    n = {k: int(v) for k, v in re.findall(r"count (\w+)=(\d+)", out)}
    assert n["shapes"] > 40000
    for branch in ("fwd_fast", "fwd_generic", "bwd_fast", "bwd_generic", "tiled", "tiles_outnumber_waves", "several_slabs", "long_slabs",
                   "ip_refused", "ip_empty", "loss_slabs", "loss_long_slabs", "concat"):
        assert n.get(branch, 0) > 0, (branch, n)


def test_the_listed_shapes_take_the_branches_the_model_names(plans_host):
    shapes = [(50, 66, 32), (50, 32, 2), (1517, 205, 64), (31, 32, 2), (32, 32, 2), (8193, 3, 2), (17, 17, 17), (17, 16, 17),
              (50, 127, 32), (50, 128, 32), (128, 66, 32), (129, 66, 32), (1517, 66, 32), (50, 203, 64)]
    out = run_host(plans_host, [v for s in shapes for v in s])
    plans = [dict(kv.split("=") for kv in line.split()[1:]) for line in out.splitlines() if line.startswith("plan ")]
    assert len(plans) == len(shapes)
    for (M, K, N), p in zip(shapes, plans):
        assert int(p["fwd_route"]) == R.ip_route(M, K, N, R.FORWARD) and int(p["slabs"]) == R.slabs(M), (M, K, N, p)
        assert int(p["bwd_route"]) == R.ip_route(M, K, N, R.BACKWARD), (M, K, N, p)
        assert int(p["slab_rows"]) == R.slab_rows(M) and int(p["ws_elems"]) * 4 == R.ip_workspace_bytes(M, K, N, 4)
        assert p["fwd"] == ("tiled" if int(p["fwd_route"]) == R.ROUTE_FAST else "-"), (M, K, N, p)
        assert p["wdiff"] == p["bottom"] == ("tiled" if int(p["bwd_route"]) == R.ROUTE_FAST else "-"), (M, K, N, p)
