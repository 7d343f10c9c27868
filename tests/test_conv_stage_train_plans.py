"""The launch plans of the TRAIN stage's fused forward, read from the C++ itself, and what the large shapes of
tests/test_gpu_conv_stage_train.py rest on.  tests/native/conv_stage_train_plans_host.cpp includes
csrc/conv_stage_train_plans.h (train_plan, train_route, fused_bytes, train_finish_grid), prints the plans of the shapes it
is given and holds every plan to what the two launches rely on -- partial sums of 2 K groups words with one slot per
workgroup, the convolution's own chunk of input channels, bands of whole windows that cover the map, the LDS, and chunks
of launch 2 that cover a channel's pooled elements exactly once, at most 64 unless they are of the least size.  No GPU:
the program is host code, built with AddressSanitizer and UBSan like tests/native/conv_plans_host.cpp.

  * every shape of conv_stage_train_reference.LARGE_STAGES reaches what it is listed for (LARGE_PLANS), and the library's
    route call says what the list says of the main call;
  * the invariants hold over conv_plans_host's sweep of shapes times the windows that divide the map;
  * the first draw of forward_conditioned_inputs passes at every large shape, the exact probe's sums stay below 2^24;
  * float32 arithmetic alone, on the fused route's order of sums, meets the project's float32 bar at every large shape:
    the bar the GPU tests hold the kernels to is not fitted to them."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import conv_stage_train_reference as R
from pooled_stage_suite import BAR, _cshape
from util import SEED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [R.stage_id(st) for st in R.LARGE_STAGES]
LINES = ("shape", "plan", "finish", "route")


@pytest.fixture(scope="module")
def plans_host(tmp_path_factory):
    """mms_common.h pulls in the HIP runtime header, so hipcc compiles it -- the host side only."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path_factory.mktemp("conv_stage_train_plans") / "conv_stage_train_plans_host"
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "mms_answer_selection_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "conv_stage_train_plans_host.cpp"), "-o", str(exe)])
    return str(exe)


def run_host(exe, args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "every plan holds its invariants" in out.stdout
    return out.stdout


def fields(line):
    return {k: int(v) for k, v in (w.split("=") for w in line.split()[1:])}


def host_args(st):
    return list(st.conv[:7]) + list(st.pool)


def plans_of(exe, stages):
    """-> [{"shape" | "plan" | "finish" | "route": fields}] per stage, in order"""
    out, got = run_host(exe, [v for st in stages for v in host_args(st)]), []
    for line in out.splitlines():
        word = line.split()[0]
        if word == "shape":
            got.append({})
        if word in LINES:
            got[-1][word] = fields(line)
    assert len(got) == len(stages) and all(sorted(g) == sorted(LINES) for g in got)
    return got


@pytest.fixture(scope="module")
def listed(plans_host):
    return dict(zip(R.LARGE_STAGES, plans_of(plans_host, R.LARGE_STAGES)))


@pytest.fixture(scope="module")
def stage(hiplib):
    from mms_answer_selection_amd import conv_stage_train
    conv_stage_train.lib()
    return conv_stage_train


def test_every_large_shape_is_plain_and_has_its_claim():
    """The program takes stride 1, pad 0, group 1 and a window that tiles the map."""
    assert sorted(R.LARGE_PLANS) == sorted(R.LARGE_STAGES) and len(set(R.LARGE_STAGES)) == len(R.LARGE_STAGES)
    for st in R.LARGE_STAGES:
        s = st.conv
        assert (R.CR.pair(s.stride), R.CR.pair(s.pad), s.group) == ((1, 1), (0, 0), 1)
        OH, OW = R.CR.output_dims(s)
        assert OH % st.pool[0] == 0 and OW % st.pool[1] == 0
        assert s.N * s.K * OH * OW <= 1100000              # seconds per test: about a million elements of y at most


@pytest.mark.parametrize("st", R.LARGE_STAGES, ids=IDS)
def test_large_shape_reaches_what_it_claims(st, listed, stage, hiplib):
    from mms_answer_selection_amd import conv
    got, want, s = listed[st], R.LARGE_PLANS[st], st.conv
    OH, OW = R.CR.output_dims(s)
    assert (got["shape"]["OH"], got["shape"]["OW"], got["shape"]["PP"]) == (OH, OW, OH * OW // (st.pool[0] * st.pool[1]))
    assert got["plan"]["ok"] == 1
    for line in ("plan", "finish"):
        assert {k: got[line][k] for k in want[line]} == want[line], line
    assert got["plan"]["partial_bytes"] == 2 * s.K * want["plan"]["groups"] * 4
    assert got["finish"]["windows"] == s.N * got["shape"]["PP"]
    names = {stage.ROUTE_SEQUENCE: R.SEQ, stage.ROUTE_FUSED: R.FUSED}
    for method in R.METHODS:
        assert names[got["route"][method]] == want["route"][method], method
        assert names[stage.conv_stage_train_route(_cshape(conv, st), st.pool, method)] == want["route"][method], method


def test_the_large_shapes_reach_what_the_parent_lists_do_not(plans_host, listed):
    """Each regime by the rule that defines it, over the whole list -- the statement of LARGE_PLANS without its figures --
    and why LARGE_STAGES exists: no shape of GPU_STAGES reaches any of them."""
    L = list(listed.values())
    fold = R.FOLD_THREADS
    assert any(p["finish"]["chunks"] > 1 and p["finish"]["last"] == 1 for p in L)                  # a chunk of one
    assert any(p["finish"]["chunks"] > 2 and 1 < p["finish"]["last"] < p["finish"]["wpc"] for p in L)
    assert any(p["finish"]["wpc"] > 1024 and p["finish"]["chunks"] == 64 and p["finish"]["last"] < p["finish"]["wpc"] for p in L)
    assert any(fold < p["plan"]["groups"] < 2 * fold and p["plan"]["last_images"] < p["plan"]["G"] for p in L)
    assert any(p["plan"]["groups"] > 5 * fold and p["plan"]["groups"] % fold and p["plan"]["bands"] == 2 for p in L)
    assert any(p["plan"]["kind"] == 1 and p["plan"]["last_rows"] < p["plan"]["R"] and p["plan"]["groups"] > fold for p in L)
    for m in ("ave", "max"):
        assert any(p["route"][m] == 1 for p in L) and any(p["route"][m] == 0 and p["plan"]["kind"] == 1 for p in L)
    small = [st for st in R.FUSED_STAGES]
    for p in plans_of(plans_host, small):
        assert p["plan"]["ok"] == 1
        assert p["finish"]["chunks"] == 1 and p["plan"]["groups"] <= fold and p["route"] == dict(ave=0, max=0)


def test_invariants_hold_over_the_sweep(plans_host):
    out = run_host(plans_host, ["--sweep"])
    n = {k: int(v) for k, v in (line.split()[1].split("=") for line in out.splitlines() if line.startswith("sweep "))}
    # conv_plans_host's shapes: N x C x K x (H, W, kernel) with the kernel inside the image, 2 * 5 * 5 * 356
    assert n["shapes"] == 17800 and n["plans"] > 6 * n["shapes"] and n["ok"] > n["plans"] // 2
    assert n["finish_grids"] == 17 * 9
    for branch in ("kind_images", "kind_row_band", "kind_one_image", "band_higher_than_the_convolutions",
                   "band_halved_for_the_chunk", "several_chunks", "tile_row_padded", "ragged_last_band",
                   "refused_by_the_convolution", "refused_by_the_window", "refused_by_the_chunk", "fused_max",
                   "finish_one_chunk", "finish_least_chunks", "finish_capped_chunks", "finish_ragged_last_chunk"):
        assert n.get(branch, 0) > 0, branch


def test_route_table_and_workspace_of_the_large_shapes(stage, hiplib):
    """The main call's workspace query where the forward is fused: max(the partial sums, the backward's carve); the
    forced fused query is never below the partial sums."""
    from mms_answer_selection_amd import conv
    for st in R.LARGE_STAGES:
        sp, s = C.byref(_cshape(conv, st)), st.conv
        partials = 2 * s.K * R.LARGE_PLANS[st]["plan"]["groups"] * 4
        for pool, method in enumerate(R.METHODS):
            auto = hiplib.mms_conv_stage_train_workspace_bytes(sp, *st.pool, pool)
            seq = hiplib.mms_conv_stage_train_sequence_workspace_bytes(sp, *st.pool, pool)
            fused = hiplib.mms_conv_stage_train_fused_workspace_bytes(sp, *st.pool, pool)
            assert fused >= partials and seq > 0
            assert auto == (fused if R.LARGE_PLANS[st]["route"][method] == R.FUSED else seq)


# ---- inputs, and what float32 alone achieves -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def large_inputs(st):
    return R.forward_conditioned_inputs(st, np.float32, SEED)


@pytest.mark.parametrize("st", R.LARGE_STAGES, ids=IDS)
def test_the_first_draw_is_forward_conditioned(st):
    first = R._draw(st, np.float32, SEED)
    var, scale, gap = R.conditions(st, first)
    print("least variance %.3g, least |scale| %.3g (least top-two gap %.3g: not a condition here)" % (var, scale, gap))
    assert var >= R.MIN_VAR > 1e6 * R.VAR_EPS and scale >= R.MIN_SCALE
    assert first["scale"][0] > 0 > first["scale"][1]
    inp = large_inputs(st)
    for k, v in first.items():
        assert (v is None and inp[k] is None) or (v == inp[k]).all(), k


@pytest.mark.parametrize("st", R.LARGE_STAGES, ids=IDS)
def test_large_probe_sums_are_exact_in_float(st):
    inp = R.integer_probe(st, SEED)
    y, s0, s1 = R.probe_sums(st, inp)                                          # asserts the 2^24 bounds
    print("largest sum |y| %d, largest sum y*y %d of 2^24 = %d" % (np.abs(y).sum(axis=(0, 2, 3)).max(), s1.max(), 2 ** 24))
    assert (y.astype(np.float32).astype(np.int64) == y).all()
    assert inp["scale"][R.ZERO_CHANNEL] == 0 and inp["scale"][R.NEGATIVE_CHANNEL] < 0 < inp["scale"][R.POSITIVE_CHANNEL]
    # the restated fold is the identity on exact sums: the statistics are those of the int64 sums, to the word
    p = R.LARGE_PLANS[st]["plan"]
    tot = R.fold_partials(R.fused_partials(y.astype(np.float32), p["G"], p["R"], p["bands"]))
    assert (tot[:, 0].astype(np.int64) == s0).all() and (tot[:, 1].astype(np.int64) == s1).all()


@pytest.mark.parametrize("st", R.LARGE_STAGES, ids=IDS)
def test_float32_on_the_fused_order_of_sums_meets_the_bar(st):
    """save_mean, save_std and the running blobs from float32 partial sums per launch-1 workgroup, folded as launch 2
    folds them, against the float64 model in assert_close's metric: inside BAR[float32], the bar of the GPU tests."""
    inp, p = large_inputs(st), R.LARGE_PLANS[st]["plan"]
    got = R.fused_statistics_f32(st, inp, p["G"], p["R"], p["bands"])
    want = R.model_forward(st, R.AVE, inp)                                     # the statistics do not depend on the method
    worst = 0.0
    for k in sorted(got):
        scale = max(1.0, float(np.max(np.abs(want[k]))))
        ratio = float(np.max(np.abs(got[k].astype(np.float64) - want[k]))) / (BAR[np.float32] * scale)
        print("%-13s %.3g of the bar" % (k, ratio))
        worst = max(worst, ratio)
    assert sorted(got) == ["running_mean", "running_var", "save_mean", "save_std"] and worst <= 1.0
