"""Times the TRAIN-phase forward of the stage Convolution -> BN -> Pool -> TanH (include/mms_conv_stage_train.h), float,
in one process and alternating pass by pass:

    fused     mms_conv_stage_train_forward_fused_f32: two launches -- whether or not mms_conv_stage_train_route sends
              the shape there (its rule rests on this table)
    sequence  the two public calls a host had before this one, issued here: mms_conv_forward_f32, then
              mms_bn_pool_tanh_forward_f32 / mms_bn_maxpool_tanh_forward_f32 with phase 0 (three launches at the
              training batch)
    one-call  mms_conv_stage_train_forward_sequence_f32: the same two calls behind the new entry point

Stages: network_v4's two (AVE) and the MAX stages of network_v3 / network_v5 (tools/bench_conv_maxpool_stage.py's table).
Protocol (tools/bench_conv.py's): every call of a pass takes the next of a ring of operand sets (x, y, top, save_pool)
that together exceed the 256-MB Infinity Cache (at least two sets); a pass is `iters` calls between two HIP events on
one stream; two untimed warm-up passes, then seven timed ones; the table gives the median pass and the range, in us per
call, and the ratio sequence / fused of the medians.

    python tools/bench_conv_stage_train.py stage:N [stage:N ...]       stage: conv0 conv1 v3a v3b v5a v5b v5c

One (stage, N) per invocation gives each point a process of its own.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench_conv import measure
from bench_conv_maxpool_stage import STAGES as MAX_STAGES, fused_plan
from mms_answer_selection_amd import bn_maxpool, capi, conv, conv_stage_train

RING_BYTES = 320 << 20
# C, H, W, K, kernel, window, pooling method
STAGES = {"conv0": (4, 40, 40, 32, 5, 4, "ave"), "conv1": (32, 9, 9, 64, 5, 5, "ave")}
STAGES.update({k: v + ("max",) for k, v in MAX_STAGES.items()})


def bench(name, N):
    C, H, W, K, k, p, method = STAGES[name]
    OH, OW = H - k + 1, W - k + 1
    pooled = (N, K, OH // p, OW // p)
    per_set = 4 * (N * C * H * W + N * K * OH * OW + 2 * pooled[0] * pooled[1] * pooled[2] * pooled[3])
    nsets = max(2, -(-RING_BYTES // per_set))
    g = torch.Generator(device="cuda").manual_seed(1701)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    new = lambda *s: torch.empty(*s, device="cuda")
    sets = [dict(x=rnd(N, C, H, W) * 0.5, y=new(N, K, OH, OW), top=new(*pooled), sp=new(*pooled)) for _ in range(nsets)]
    w, b = rnd(K, C, k, k) * (C * k * k) ** -0.5, rnd(K) * 0.1
    scale, shift = torch.rand(K, device="cuda", generator=g) + 0.5, rnd(K) * 0.5
    rm, rv, sm, ss = rnd(K) * 0.5, torch.rand(K, device="cuda", generator=g) + 0.5, new(K), new(K)
    ws = capi.Workspace()
    s = lambda i: sets[i % nsets]
    bn = capi.bn_pool_tanh_forward if method == "ave" else bn_maxpool.bn_maxpool_tanh_forward

    def stage(route):
        return lambda i: conv_stage_train.conv_stage_train_forward(
            s(i)["x"], w, b, p, method, scale, shift, rm, rv, s(i)["y"], s(i)["top"], s(i)["sp"], sm, ss, ws=ws,
            route=route)

    def two_calls(i):
        conv.conv_forward(s(i)["x"], w, b, s(i)["y"])
        bn(s(i)["y"], p, scale, shift, rm, rv, s(i)["top"], s(i)["sp"], sm, ss, phase=0, ws=ws)

    G, bands = fused_plan(C, H, W, K, k, p)
    shape = conv.conv_shape(N, C, H, W, K, k)
    iters = 20 if N <= 200 else 3
    print("%s N=%d %s (%d,%d,%d)->%d %dx%d, window %dx%d: %d operand sets of %.1f MB, %d calls per pass, %d workgroups "
          "(%d image(s) x 1/%d), mms_conv_stage_train_route = %d"
          % (name, N, method, C, H, W, K, k, k, p, p, nsets, per_set / 1e6, iters, -(-N // G) * bands, G, bands,
             conv_stage_train.conv_stage_train_route(shape, p, method)))
    res = measure({"fused": stage("fused"), "sequence": two_calls, "one-call": stage("sequence")}, iters)
    for key, v in res.items():
        if isinstance(v, str):
            print("  %-9s not measured (%s)" % (key, v))
            continue
        extra = ""
        if key == "fused" and not isinstance(res["sequence"], str):
            extra = "  sequence / fused = %.3f  ranges %s" % (
                res["sequence"][0] / v[0], "apart" if v[2] < res["sequence"][1] or res["sequence"][2] < v[1] else "overlap")
        print("  %-9s median %10.1f us  range %10.1f .. %10.1f%s" % (key, v[0], v[1], v[2], extra))
    del sets
    torch.cuda.empty_cache()


if __name__ == "__main__":
    print("device: %s; torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    for step in sys.argv[1:] or ["conv0:50", "conv1:50"]:
        name, n = step.split(":")
        bench(name, int(n))
