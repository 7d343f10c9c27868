"""GPU suite: the Convolution kernels at the launch plans the shapes of tests/test_gpu_conv.py never take -- the fallback
branches of conv_prod_plan (fewer images, then fewer rows per workgroup; a chunk of fewer than four channels) and of
conv_wdiff_plan (G and R one less at a time; the refusal), MT = 4 in the bottom_diff direction, chunks x bands, slab
boundaries inside an image, 1 x 1 maps, OW = 256, and the three passes on different routes.  The shapes and what each is
listed for: conv_reference.PLAN_CASES; that a shape takes its branch is tests/test_conv_plans.py's, from the C++.
The checks are tests/test_gpu_conv.py's own (run, probe, model, Guarded): equality with the int64 reference on the
integer probe -- which a wrong band height, chunk remainder or slab boundary fails whatever the order of a sum -- and the
float64 model at the project's bars on the conditioned inputs."""
import numpy as np
import pytest
import torch

import conv_reference as R
import test_gpu_conv as V
from util import assert_close

pytestmark = pytest.mark.gpu

CASE_IDS = ["-".join(str(v) for v in c[0][:7]) for c in R.PLAN_CASES]
MODES = {"f32": (np.float32, "auto"), "f32-generic": (np.float32, "generic"), "f64": (np.float64, "auto")}
MIXED = [c[0] for c in R.PLAN_CASES if c[1] != "FFF"]
WS_GUARD = 4096         # bytes, a multiple of 16


class GuardedWorkspace:
    """What conv_backward takes as `ws`: exactly the bytes asked for, every word a NaN, between two zones of sentinel
    bytes -- a launch that writes more slabs than mms_conv_workspace_bytes counted leaves its mark."""

    def __init__(self):
        self.buf, self.n = None, 0

    def get(self, nbytes, device):
        assert self.buf is None, "one call per workspace"
        if nbytes == 0:
            return None, 0
        assert nbytes % 4 == 0
        self.n = int(nbytes)
        self.buf = torch.full((2 * WS_GUARD + self.n,), 0x5A, dtype=torch.uint8, device=device)
        self.buf[WS_GUARD:WS_GUARD + self.n].view(torch.float32).fill_(float("nan"))
        return self.buf.data_ptr() + WS_GUARD, self.n

    def check(self, nbytes):
        assert self.n == nbytes
        b = V.host(self.buf)
        assert (b[:WS_GUARD] == 0x5A).all() and (b[WS_GUARD + self.n:] == 0x5A).all(), "workspace: guard overwritten"


@pytest.mark.parametrize("mode", list(MODES), ids=list(MODES))
@pytest.mark.parametrize("case", R.PLAN_CASES, ids=CASE_IDS)
def test_probe_parity_and_determinism_at_the_plan(case, mode, hiplib):
    """Per shape, on the automatic route in float32, on the generic route in float32 and in float64: (1) the integer probe
    equals the int64 reference word for word in all four outputs, on top of non-zero initial diffs; (2) the conditioned
    inputs against the float64 model at the bar; (3) a second run with a NaN-filled workspace of exactly the size asked
    for between guard zones, every operand one element off a 16-byte boundary, gives the same words."""
    from mms_answer_selection_amd import conv
    s, dtype, route = case[0], *MODES[mode]
    assert R.probe_bound(s) < 2 ** 24
    pin, pwant = V.probe(s)
    got = V.run(s, pin, dtype, route=route)
    assert sorted(got) == sorted(pwant)
    for k, v in pwant.items():
        V.assert_words_equal(got[k], v.astype(dtype), "integer probe, " + k)
    inp = V.inputs(s, dtype)
    first = V.run(s, inp, dtype, route=route)
    want = V.model(s, dtype)
    for k in sorted(want):
        assert first[k].dtype == dtype and not np.isnan(first[k]).any(), k
        scale = max(1.0, float(np.max(np.abs(want[k]))))
        print("%-12s %.3e" % (k, float(np.max(np.abs(first[k].astype(np.float64) - want[k]))) / scale))
    for k in sorted(want):
        assert_close(first[k], want[k], V.BAR[dtype], k)
    ws = GuardedWorkspace()
    second = V.run(s, inp, dtype, shift=1, ws=ws, route=route)
    ws.check((conv.conv_workspace_bytes if dtype == np.float32 else conv.conv_workspace_bytes_f64)(V.cshape(s)))
    for k in first:
        V.assert_words_equal(second[k], first[k], k + ", second run: NaN workspace, operands off by one element")
    pws = GuardedWorkspace()
    again = V.run(s, pin, dtype, shift=1, ws=pws, route=route)
    pws.check(ws.n)
    for k in got:
        V.assert_words_equal(again[k], got[k], k + ", integer probe, second run")


@pytest.mark.parametrize("case", R.PLAN_CASES, ids=CASE_IDS)
def test_routes_and_workspace_are_the_recorded_ones(case, hiplib):
    """The three passes take the routes of the list -- the mixed rows are the point -- and mms_conv_workspace_bytes is
    the value tests/test_conv_plans.py read from the plans: max(generic slabs, fast slabs) * (K C kh kw + K) * 4."""
    from mms_answer_selection_amd import conv
    s, routes, workspace = case
    name = {conv.ROUTE_FAST: "F", conv.ROUTE_GENERIC: "G"}
    got = "".join(name[conv.conv_route(V.cshape(s), p)]
                  for p in (conv.PASS_FORWARD, conv.PASS_BOTTOM_DIFF, conv.PASS_PARAM_DIFF))
    assert got == routes
    assert conv.conv_workspace_bytes(V.cshape(s)) == workspace


@pytest.mark.parametrize("dtype", V.DTYPES, ids=V.IDS)
@pytest.mark.parametrize("s", MIXED, ids=["-".join(str(v) for v in s[:7]) for s in MIXED])
def test_optional_backward_outputs_on_mixed_routes(s, dtype, hiplib):
    """tests/test_gpu_conv.py's own body where the backward's two halves take different routes: bottom_diff, weight_diff
    and bias_diff left out alone and in pairs have the words of the full run, and what was not asked for is untouched."""
    V.test_optional_backward_outputs(s, dtype, hiplib)


def test_a_workgroup_of_several_images_keeps_them_apart(hiplib):
    """S(9, 4, 12, 12, 33, 7, 7): the forward takes 4 images per workgroup after halving G = 7, so the batch runs as
    groups of 4, 4 and 1.  The whole batch against the same batch as three calls of 4, 4 and 1 images: top and
    bottom_diff are the concatenation word for word (conditioned inputs and probe), and on the probe weight_diff and
    bias_diff equal the three calls accumulated into the same diffs."""
    s = R.PLAN_SHAPES[-1]
    assert tuple(s[:7]) == (9, 4, 12, 12, 33, 7, 7)
    parts = ((0, 4), (4, 8), (8, 9))
    for name, inp in (("conditioned", V.inputs(s, np.float32)), ("probe", V.probe(s)[0])):
        whole = V.run(s, inp, np.float32)
        dw, db = inp["weight_diff0"], inp["bias_diff0"]
        tops, dxs = [], []
        for a, b in parts:
            sub = dict(inp, x=inp["x"][a:b], top_diff=inp["top_diff"][a:b], weight_diff0=dw, bias_diff0=db)
            got = V.run(s._replace(N=b - a), sub, np.float32)
            tops.append(got["top"])
            dxs.append(got["bottom_diff"])
            dw, db = got["weight_diff"], got["bias_diff"]
        V.assert_words_equal(whole["top"], np.concatenate(tops), name + ": top, whole batch against 4 + 4 + 1")
        V.assert_words_equal(whole["bottom_diff"], np.concatenate(dxs), name + ": bottom_diff, whole against 4 + 4 + 1")
        if name == "probe":
            V.assert_words_equal(whole["weight_diff"], dw, "probe: weight_diff, whole batch against 4 + 4 + 1 accumulated")
            V.assert_words_equal(whole["bias_diff"], db, "probe: bias_diff, whole batch against 4 + 4 + 1 accumulated")
