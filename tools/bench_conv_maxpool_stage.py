"""Times the TEST-phase stage Convolution -> BN -> MaxPool -> TanH (include/mms_conv_maxpool_stage.h) on the five
stages of network_v3 and network_v5, float, in one process and alternating pass by pass:

    fused     mms_conv_maxpool_stage_forward_fused_f32: one launch, the map never stored -- whether or not
              mms_conv_maxpool_stage_route sends the shape there (its rules rest on this table)
    sequence  mms_conv_maxpool_stage_forward_sequence_f32: mms_conv_forward_f32 into the workspace, then
              mms_bn_maxpool_tanh_forward_f32 (TEST) from it -- what a host had before this call
    torch     conv2d + eval-mode batch_norm + max_pool2d + tanh on the same tensors (scale's signs are mixed, so this is
              the same work, not the same numbers)

Protocol (tools/bench_conv.py's): every call of a pass takes the next of a ring of operand sets (x, top, save_pool)
that together exceed the 256-MB Infinity Cache (at least two sets), so no operand is cache-warm from the call before;
the sequence's workspace is one buffer, as a host would keep it; a pass is `iters` calls between two HIP events on one
stream; two untimed warm-up passes, then seven timed ones; the table gives the median pass and the range, in us per
call, the ratio sequence / fused of the medians, whether the two ranges are apart, and the bytes each form moves through
device memory.

    python tools/bench_conv_maxpool_stage.py [stage:N[:ab] ...]      default: every stage at N = 50 and N = 1517

`:ab` leaves torch out (the points between the two batch sizes that place a routing threshold).  A few (stage, N) per
invocation let a job script put each step under a time limit of its own.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench_conv import measure
from mms_answer_selection_amd import capi, conv, conv_maxpool_stage

RING_BYTES = 320 << 20
# C, H, W, K, kernel (stride 1, pad 0), window
STAGES = {
    "v3a": (1, 40, 40, 64, 5, 4),                # network_v3: 36 x 36 map, bands of 4 rows
    "v3b": (64, 9, 9, 64, 5, 5),                 # 5 x 5 map, one window, ten images per workgroup
    "v5a": (2, 40, 40, 32, 3, 2),                # network_v5: 38 x 38 map, bands of 6 rows (the last of 2)
    "v5b": (32, 19, 19, 32, 4, 2),               # 16 x 16 map, one image per workgroup
    "v5c": (32, 8, 8, 32, 3, 6),                 # 6 x 6 map, one window, seven images per workgroup
}
TILE_PIXELS, LDS_FLOATS = 256, 16384             # csrc/conv_tile.h: kConvTilePixels, kConvLdsFloats


def fused_plan(C, H, W, K, k, p):
    """-> (images per workgroup, bands per image) of the fused launch: csrc/conv_tile.h's conv_prod_plan(d, FORWARD,
    rq = p) restated for a k x k kernel, stride 1, no padding, one group.  The library does not export its plan;
    tests/test_abi_conv_maxpool_stage.py holds this restatement to the counts at which mms_conv_maxpool_stage_route
    changes its answer, so a change of the plan that this function misses fails there."""
    OH, OW = H - k + 1, W - k + 1
    assert OW <= TILE_PIXELS and C <= 64 and K <= 64, "the fused launch does not reach this shape"
    if OH * OW <= TILE_PIXELS // 2:
        G, R, bands = TILE_PIXELS // (OH * OW), OH, 1
    else:
        upb = TILE_PIXELS // OW // p
        assert upb >= 1, "the fused launch does not reach this shape"
        units = OH // p
        nb = -(-units // upb)
        G, R = 1, -(-units // nb) * p
        bands = -(-OH // R)
    mpad = 16 * (1 if K <= 16 else 2 if K <= 32 else 4)
    while True:                                  # fewer images, then fewer rows, until four input channels fit the LDS
        plane = (R + k - 1) * W
        cc = next((c for c in range(C, 0, -1) if G * c * plane + (mpad + 1) * ((c * k * k + 3) & ~3) <= LDS_FLOATS), 0)
        if cc >= min(C, 4):
            return G, bands
        if G > 1:
            G = (G + 1) // 2
        elif R > p:
            R = (R // p + 1) // 2 * p
            bands = -(-OH // R)
        else:
            assert cc >= 1, "the fused launch does not reach this shape"
            return G, bands


def bench(name, N, with_torch=True):
    C, H, W, K, k, p = STAGES[name]
    G, bands = fused_plan(C, H, W, K, k, p)
    OH, OW = H - k + 1, W - k + 1
    pooled = N * K * (OH // p) * (OW // p)
    per_set = 4 * (N * C * H * W + 2 * pooled)
    nsets = max(2, -(-RING_BYTES // per_set))
    g = torch.Generator(device="cuda").manual_seed(1701)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    sets = [dict(x=rnd(N, C, H, W) * 0.5, top=torch.empty(N, K, OH // p, OW // p, device="cuda"),
                 sp=torch.empty(N, K, OH // p, OW // p, device="cuda")) for _ in range(nsets)]
    w, b = rnd(K, C, k, k) * (C * k * k) ** -0.5, rnd(K) * 0.1
    mean, var = rnd(K) * 0.5, torch.rand(K, device="cuda", generator=g) + 0.5
    scale, shift = (torch.rand(K, device="cuda", generator=g) + 0.5) * torch.sign(rnd(K)), rnd(K) * 0.5
    ws = capi.Workspace()
    s = lambda i: sets[i % nsets]
    ours = lambda route: (lambda i: conv_maxpool_stage.conv_maxpool_stage_forward(
        s(i)["x"], w, b, p, mean, var, scale, shift, s(i)["top"], s(i)["sp"], ws=ws, route=route))

    def torch_f(i):
        with torch.no_grad():
            y = torch.nn.functional.conv2d(s(i)["x"], w, b)
            y = torch.nn.functional.batch_norm(y, mean, var, scale, shift, training=False, eps=1e-9)
            torch.tanh(torch.nn.functional.max_pool2d(y, p))

    shape = conv.conv_shape(N, C, H, W, K, k)
    route = conv_maxpool_stage.conv_maxpool_stage_route(shape, p)
    fns = {"fused": ours("fused"), "sequence": ours("sequence")}
    if with_torch:
        fns["torch"] = torch_f
    iters = 20 if N <= 100 else 3
    small = 4 * (N * C * H * W + K * C * k * k + 5 * K + 2 * pooled)
    moved = {"fused": small, "sequence": small + 8 * N * K * OH * OW}
    print("%s N=%d (%d,%d,%d)->%d %dx%d, window %dx%d: %d operand sets of %.1f MB, %d calls per pass, %d workgroups, "
          "mms_conv_maxpool_stage_route = %d" % (name, N, C, H, W, K, k, k, p, p, nsets, per_set / 1e6, iters,
                                                 -(-N // G) * bands, route))
    res = measure(fns, iters)
    for key, v in res.items():
        if isinstance(v, str):
            print("  %-9s not measured (%s)" % (key, v))
            continue
        extra = "  %7.1f MB moved" % (moved[key] / 1e6) if key in moved else ""
        if key == "fused" and not isinstance(res["sequence"], str):
            q = res["sequence"]
            apart = "fused faster" if v[2] < q[1] else "sequence faster" if q[2] < v[1] else "ranges overlap"
            extra += "  sequence / fused = %.2f  (%s)" % (q[0] / v[0], apart)
        print("  %-9s median %10.1f us  range %10.1f .. %10.1f%s" % (key, v[0], v[1], v[2], extra))
    del sets
    torch.cuda.empty_cache()


if __name__ == "__main__":
    steps = sys.argv[1:] or ["%s:%d" % (name, n) for n in (50, 1517) for name in STAGES]
    print("device: %s; torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    for step in steps:
        name, n, *rest = step.split(":")
        bench(name, int(n), with_torch=rest != ["ab"])
