"""The launch plans of the fast convolution route, read from the C++ itself: tests/native/conv_plans_host.cpp includes
csrc/conv_plans.h (conv_wdiff_plan, conv_generic_slabs) and csrc/conv_tile.h (conv_prod_plan), prints the plans of the
shapes it is given and holds every plan to what the kernels rely on -- the LDS, the pixel tile, bands that cover the map,
a chunk of 1 .. Cin channels, at most 64 slabs that cover the units.  No GPU: the program is host code, built with
AddressSanitizer and UBSan like tests/native/bx3_waits_host.cpp.

  * every shape of conv_reference.PLAN_CASES takes the branch it is listed for (PLANS below: the fields that say so);
  * the invariants hold over a sweep of 17 800 shapes, and the sweep reaches every branch of both plans;
  * the workspace of each listed shape is the value written next to it (tests/test_gpu_conv_plans.py compares the
    library's answer with the same value)."""
import os
import shutil
import subprocess

import pytest

import conv_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Per listed shape, what its comment in conv_reference.PLAN_CASES claims, as fields of the printed plans.  G0, R0: the
# geometry before the plan shrank it to the LDS.  A pass that is not named is only held to the routes.
PLANS = {
    (3, 4, 12, 12, 17, 11, 11): dict(
        forward=dict(G0=64, R0=2, G=1, R=1, bands=2, Cin=4, CC=3, MT=2),
        param_diff=dict(G0=64, G=23, R=2, bands=1, groups=8, MT=2)),
    (2, 33, 9, 9, 5, 9, 9): dict(
        forward=dict(G0=256, G=32, R=1, bands=1, Cin=33, CC=4, MT=1),
        bottom_diff=dict(G0=3, R0=9, G=1, R=1, bands=9, Cin=5, CC=3, MT=4),
        param_diff=dict(G0=256, G=6, groups=42)),
    (3, 1, 9, 9, 1, 9, 9): dict(
        forward=dict(G0=256, G=128, R=1, bands=1, Cin=1, CC=1, Kpad=84, MT=1),
        bottom_diff=dict(G0=3, G=3, R=9, bands=1, Cin=1, CC=1, Kpad=84),
        param_diff=dict(G0=256, G=166, groups=2)),
    (1, 1, 3, 258, 1, 3, 3): dict(
        forward=dict(G=1, R=1, bands=1, BW=258),
        param_diff=dict(G=1, R=1, bands=1, PP=257, slabs=1)),
    (2, 3, 6, 40, 33, 1, 1): dict(
        param_diff=dict(G0=1, R0=6, G=1, R=5, bands=2, MT=4, units=4, ups=1, slabs=4)),
    (2, 64, 9, 14, 33, 1, 1): dict(
        forward=dict(G0=2, G=2, R=9, Cin=64, CC=51, MT=4),
        bottom_diff=dict(G=2, R=9, bands=1, Cin=33, CC=33, MT=4),
        param_diff=dict(G0=2, R0=9, G=1, R=8, bands=2, MT=4)),
    (2, 40, 3, 130, 1, 3, 1): dict(
        forward=dict(G=1, R=1, bands=1, Cin=40, CC=37),
        bottom_diff=dict(G=1, R=1, bands=3, MT=4)),
    (5, 1, 14, 130, 1, 1, 1): dict(
        param_diff=dict(G=1, R=1, bands=14, units=70, ups=2, slabs=35)),
    (2, 8, 20, 40, 1, 11, 11): dict(
        forward=dict(G=1, R0=5, R=5, bands=2, Cin=8, CC=6),
        param_diff=dict(bands=2, groups=16)),
    (9, 4, 12, 12, 33, 7, 7): dict(
        forward=dict(G0=7, G=4, R=6, bands=1, Cin=4, CC=4, MT=4)),
}
PASSES = ("forward", "bottom_diff", "param_diff")


@pytest.fixture(scope="module")
def plans_host(tmp_path_factory):
    """mms_common.h pulls in the HIP runtime header, so hipcc compiles it -- the host side only."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path_factory.mktemp("conv_plans") / "conv_plans_host"
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "mms_answer_selection_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "conv_plans_host.cpp"), "-o", str(exe)])
    return str(exe)


def run_host(exe, args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "every plan holds its invariants" in out.stdout
    return out.stdout


def fields(line):
    return {k: int(v) for k, v in (w.split("=") for w in line.split()[1:])}


@pytest.fixture(scope="module")
def listed(plans_host):
    """-> {shape[:7]: {"forward" | "bottom_diff" | "param_diff" | "generic_slabs" | "workspace": fields}}"""
    out = run_host(plans_host, [v for s in R.PLAN_SHAPES for v in s[:7]])
    plans, cur = {}, None
    for line in out.splitlines():
        word = line.split()[0]
        if word == "shape":
            f = fields(line)
            cur = plans.setdefault(tuple(f[k] for k in ("N", "C", "H", "W", "K", "kh", "kw")), {})
            cur["shape"] = f
        elif word in PASSES + ("generic_slabs", "workspace"):
            cur[word] = fields(line)
    assert list(plans) == [tuple(s[:7]) for s in R.PLAN_SHAPES]
    return plans


def test_every_listed_shape_is_plain(plans_host):
    """The program takes stride 1, pad 0, group 1: the listed shapes are of that kind, and each has its PLANS entry."""
    for s in R.PLAN_SHAPES:
        assert (R.pair(s.stride), R.pair(s.pad), s.group) == ((1, 1), (0, 0), 1)
    assert sorted(PLANS) == sorted(tuple(s[:7]) for s in R.PLAN_SHAPES)


@pytest.mark.parametrize("case", R.PLAN_CASES, ids=["-".join(str(v) for v in c[0][:7]) for c in R.PLAN_CASES])
def test_listed_shape_takes_its_branch(case, listed):
    s, routes, workspace = case
    got = listed[tuple(s[:7])]
    assert (got["shape"]["OH"], got["shape"]["OW"]) == R.output_dims(s)
    assert "".join("GF"[got[p]["ok"]] for p in PASSES) == routes
    for p, want in PLANS[tuple(s[:7])].items():
        assert got[p]["ok"] == 1
        assert {k: got[p][k] for k in want} == want, p
    fast = got["param_diff"]["slabs"] if got["param_diff"]["ok"] else 0
    assert got["workspace"]["slabs"] == max(got["generic_slabs"]["slabs"], fast)
    assert got["workspace"]["bytes"] == got["workspace"]["slabs"] * (s.K * s.C * s.kh * s.kw + s.K) * 4 == workspace


def test_the_listed_shapes_reach_what_the_parent_list_does_not(listed):
    """Each branch by the rule that defines it, over the whole list (the transcription-free statement of PLANS)."""
    P = list(listed.values())
    prod = [p[k] for p in P for k in ("forward", "bottom_diff") if p[k]["ok"]]
    wd = [p["param_diff"] for p in P if p["param_diff"]["ok"]]
    assert any(a["G"] < a["G0"] and a["G"] == 1 and a["R"] < a["R0"] and a["CC"] < min(4, a["Cin"]) for a in prod)
    assert any(a["G"] < a["G0"] and a["G"] > 1 for a in prod)
    assert any(p["bottom_diff"]["ok"] and p["bottom_diff"]["MT"] == 4 for p in P)
    assert any(p["forward"]["ok"] and p["forward"]["CC"] < p["forward"]["Cin"] and p["forward"]["bands"] > 1 for p in P)
    assert any(a["R"] < a["R0"] and a["G0"] == 1 for a in wd) and any(a["R"] < a["R0"] and a["G0"] > 1 for a in wd)
    assert any(a["ups"] > 1 and a["bands"] > 1 for a in wd)
    assert any(a["G0"] == 256 for a in prod) and any(p["shape"]["OW"] == 256 and p["forward"]["ok"] for p in P)
    assert any(p["forward"]["ok"] and not p["bottom_diff"]["ok"] and p["shape"]["W"] > 256 for p in P)
    assert any(p["forward"]["ok"] and p["bottom_diff"]["ok"] and not p["param_diff"]["ok"] for p in P)
    assert any(p["param_diff"]["ok"] and p["param_diff"]["slabs"] != p["generic_slabs"]["slabs"] for p in P)


def test_the_parent_list_leaves_on_the_first_pass(plans_host):
    """Why PLAN_CASES exists: no fast shape of GPU_SHAPES takes a fallback branch of conv_prod_plan."""
    plain = [s for s in R.GPU_SHAPES if (R.pair(s.stride), R.pair(s.pad), s.group) == ((1, 1), (0, 0), 1)]
    out = run_host(plans_host, [v for s in plain for v in s[:7]])
    seen = 0
    for line in out.splitlines():
        if line.split()[0] in ("forward", "bottom_diff"):
            a = fields(line)
            if a["ok"]:
                seen += 1
                assert (a["G"], a["R"]) == (a["G0"], a["R0"]) and a["CC"] >= min(4, a["Cin"]), line
    assert seen >= 2 * len(R.V4_SHAPES)


def test_a_kernel_whose_weights_alone_exceed_the_lds_is_refused(plans_host):
    """conv_prod_plan's last branch: 64 output channels of a 16 x 16 kernel are 16 640 floats of weights and offsets
    with one input channel, so the forward is generic; the bottom_diff (one output channel) is fast."""
    out = run_host(plans_host, [1, 1, 16, 16, 64, 16, 16])
    got = {line.split()[0]: fields(line) for line in out.splitlines() if line.split()[0] in PASSES}
    assert got["forward"]["ok"] == 0 and got["forward"]["G0"] == 256
    assert got["bottom_diff"]["ok"] == 1 and got["bottom_diff"]["CC"] == 3 < min(4, got["bottom_diff"]["Cin"])


def test_invariants_hold_over_the_sweep(plans_host):
    out = run_host(plans_host, ["--sweep"])
    n = {k: int(v) for k, v in (line.split()[1].split("=") for line in out.splitlines() if line.startswith("sweep "))}
    # N x C x K x (H, W, kernel) with the kernel inside the image: 2 * 5 * 5 * 356
    assert n["shapes"] == 17800 and n["wdiff_plans"] == n["shapes"] and n["prod_plans"] > 4 * n["shapes"]
    for branch in ("prod_first_pass", "prod_G_halved", "prod_G_halved_above_one", "prod_R_halved", "prod_few_channels",
                   "prod_chunks_and_bands", "prod_MT4_bottom_diff", "prod_refused_by_tile", "wdiff_first_pass",
                   "wdiff_G_decremented", "wdiff_R_decremented", "wdiff_refused_by_lds", "wdiff_refused_by_tile",
                   "wdiff_slab_inside_image", "slab_counts_differ", "forward_fast_param_diff_generic",
                   "forward_fast_bottom_diff_generic"):
        assert n.get(branch, 0) > 0, branch
