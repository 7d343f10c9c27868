"""Times the TEST-phase stage Convolution -> BN -> AvePool -> TanH (include/mms_conv_stage.h) on network_v4's two
stages at N = 50 (the driver's training batch) and N = 1517 (the test split), float, in one process and alternating pass
by pass:

    fused     mms_conv_stage_forward_fused_f32: one launch, the map never stored -- whether or not
              mms_conv_stage_route sends the shape there (its rules rest on this table)
    sequence  mms_conv_stage_forward_sequence_f32: mms_conv_forward_f32 into the workspace, then
              mms_bn_pool_tanh_forward_f32 (TEST) from it -- what a host had before this call
    torch     conv2d + eval-mode batch_norm + avg_pool2d + tanh on the same tensors

Protocol (tools/bench_conv.py's): every call of a pass takes the next of a ring of operand sets (x, top, save_pool)
that together exceed the 256-MB Infinity Cache (at least two sets), so no operand is cache-warm from the call before;
the sequence's workspace is one buffer, as a host would keep it; a pass is `iters` calls between two HIP events on one
stream; two untimed warm-up passes, then seven timed ones; the table gives the median pass and the range, in us per
call, the ratio sequence / fused of the medians, and the bytes each form moves through device memory.

    python tools/bench_conv_stage.py [stage:N[:ab] ...]        default: conv0:50 conv1:50 conv0:1517 conv1:1517

`:ab` leaves torch out (the points between the two batch sizes that place a routing threshold).  One (stage, N) per
invocation lets a job script put each step under a time limit of its own.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench_conv import measure
from mms_answer_selection_amd import capi, conv, conv_stage

RING_BYTES = 320 << 20
STAGES = {"conv0": (4, 40, 40, 32, 4), "conv1": (32, 9, 9, 64, 5)}      # C, H, W, K (5 x 5, stride 1, pad 0), window


def bench(name, N, with_torch=True):
    C, H, W, K, p = STAGES[name]
    OH, OW = H - 4, W - 4
    pooled = N * K * (OH // p) * (OW // p)
    per_set = 4 * (N * C * H * W + 2 * pooled)
    nsets = max(2, -(-RING_BYTES // per_set))
    g = torch.Generator(device="cuda").manual_seed(1701)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    sets = [dict(x=rnd(N, C, H, W) * 0.5, top=torch.empty(N, K, OH // p, OW // p, device="cuda"),
                 sp=torch.empty(N, K, OH // p, OW // p, device="cuda")) for _ in range(nsets)]
    w, b = rnd(K, C, 5, 5) * (C * 25) ** -0.5, rnd(K) * 0.1
    mean, var = rnd(K) * 0.5, torch.rand(K, device="cuda", generator=g) + 0.5
    scale, shift = torch.rand(K, device="cuda", generator=g) + 0.5, rnd(K) * 0.5
    ws = capi.Workspace()
    s = lambda i: sets[i % nsets]
    ours = lambda route: (lambda i: conv_stage.conv_stage_forward(s(i)["x"], w, b, p, mean, var, scale, shift, s(i)["top"],
                                                                  s(i)["sp"], ws=ws, route=route))

    def torch_f(i):
        with torch.no_grad():
            y = torch.nn.functional.conv2d(s(i)["x"], w, b)
            y = torch.nn.functional.batch_norm(y, mean, var, scale, shift, training=False, eps=1e-9)
            torch.tanh(torch.nn.functional.avg_pool2d(y, p))

    shape = conv.conv_shape(N, C, H, W, K, 5)
    route = conv_stage.conv_stage_route(shape, p)
    fns = {"fused": ours("fused"), "sequence": ours("sequence")}
    if with_torch:
        fns["torch"] = torch_f
    iters = 20 if N <= 100 else 3
    small = 4 * (N * C * H * W + K * C * 25 + 5 * K + 2 * pooled)
    moved = {"fused": small, "sequence": small + 8 * N * K * OH * OW}
    G, bands = (1, 9) if name == "conv0" else (10, 1)          # csrc/conv_tile.h: images per workgroup, bands per image
    print("%s N=%d (%d,%d,%d)->%d 5x5, window %dx%d: %d operand sets of %.1f MB, %d calls per pass, %d workgroups, "
          "mms_conv_stage_route = %d" % (name, N, C, H, W, K, p, p, nsets, per_set / 1e6, iters, -(-N // G) * bands, route))
    res = measure(fns, iters)
    for k, v in res.items():
        if isinstance(v, str):
            print("  %-9s not measured (%s)" % (k, v))
            continue
        extra = "  %7.1f MB moved" % (moved[k] / 1e6) if k in moved else ""
        if k == "fused" and not isinstance(res["sequence"], str):
            extra += "  sequence / fused = %.2f" % (res["sequence"][0] / v[0])
        print("  %-9s median %10.1f us  range %10.1f .. %10.1f%s" % (k, v[0], v[1], v[2], extra))
    del sets
    torch.cuda.empty_cache()


if __name__ == "__main__":
    steps = sys.argv[1:] or ["conv0:50", "conv1:50", "conv0:1517", "conv1:1517"]
    print("device: %s; torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    for step in steps:
        name, n, *rest = step.split(":")
        bench(name, int(n), with_torch=rest != ["ab"])
