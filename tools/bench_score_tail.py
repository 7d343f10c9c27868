"""Times the scoring tail Convolution -> BN -> Pool -> TanH -> head -> prob (include/mms_score_tail.h) at the tails of
the driver's nets, float, in one process and alternating pass by pass:

    fused      mms_score_tail_forward_fused_f32: one launch -- whether or not mms_score_tail_route sends the shape there
               (its rules rest on this table)
    sequence   mms_score_tail_forward_sequence_f32: mms_conv_stage_forward_f32 (MAX: mms_conv_maxpool_stage_forward_f32)
               into flt, then mms_head_forward_f32 from it -- what a host had before this call
    two calls  the same two public calls issued from here, with the host's own flt and h: the baseline itself, and a
               check that the sequence adds nothing to it

Protocol (tools/bench_conv.py's): every call of a pass takes the next of a ring of operand sets (x, overlap, prob, and
for the two calls flt and h) that together exceed the 256-MB Infinity Cache (at least two sets), so no operand is
cache-warm from the call before; the workspace is one buffer, as a host would keep it; a pass is `iters` calls between
two HIP events on one stream; two untimed warm-up passes, then seven timed ones; the table gives the median pass and the
range, in us per call, and the ratio sequence / fused of the medians.  No label: the scoring pass has no loss.

    python tools/bench_score_tail.py [net:N ...]        default: v4:50 v4:100 v4:400 v4:1517 v5:50 v5:1517

One (net, N) per invocation gives each point a fresh process, and lets a job script put each under a time limit.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench_conv import measure
from mms_answer_selection_amd import capi, conv, conv_maxpool_stage, conv_stage, head, score_tail

RING_BYTES = 320 << 20
# C, H, W, K, kernel, window, pool, F1, hidden units, classes: network_v4's tail; network_v5's last stage with
# network_v4_2's head behind it
NETS = {"v4": (32, 9, 9, 64, 5, 5, score_tail.POOL_AVE, 2, 32, 2),
        "v5": (32, 8, 8, 32, 3, 6, score_tail.POOL_MAX, 2, 64, 2)}


def bench(name, N):
    C, H, W, K, k, p, pool, F1, HID, CLS = NETS[name]
    for m in (score_tail, head, conv_stage, conv_maxpool_stage):
        m.lib()                # every family's signatures are on the handle: head_forward without a label applies none
    per_set = 4 * N * (C * H * W + F1 + CLS + K + HID)
    nsets = max(2, -(-RING_BYTES // per_set))
    g = torch.Generator(device="cuda").manual_seed(1701)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    uni = lambda *s: torch.rand(*s, device="cuda", generator=g)
    sets = [dict(x=rnd(N, C, H, W) * 0.5, ov=uni(N, F1), prob=torch.empty(N, CLS, device="cuda"),
                 flt=torch.empty(N, K, device="cuda"), h=torch.empty(N, HID, device="cuda")) for _ in range(nsets)]
    w, b = rnd(K, C, k, k) * (C * k * k) ** -0.5, rnd(K) * 0.1
    mean, var = rnd(K) * 0.5, uni(K) + 0.5
    scale, shift = uni(K) + 0.5, rnd(K) * 0.5
    w1, b1 = (uni(HID, K + F1) * 2 - 1) * (3.0 / (K + F1)) ** 0.5, rnd(HID) * 0.1
    w2, b2 = (uni(CLS, HID) * 2 - 1) * (6.0 / HID) ** 0.5, rnd(CLS) * 0.1
    ws, ws2 = capi.Workspace(), capi.Workspace()
    s = lambda i: sets[i % nsets]
    ours = lambda route: (lambda i: score_tail.score_tail_forward(
        s(i)["x"], w, b, p, pool, mean, var, scale, shift, s(i)["ov"], w1, b1, w2, b2, prob=s(i)["prob"], ws=ws,
        route=route))
    stage = conv_maxpool_stage.conv_maxpool_stage_forward if pool == score_tail.POOL_MAX else conv_stage.conv_stage_forward

    def two_calls(i):
        stage(s(i)["x"], w, b, p, mean, var, scale, shift, s(i)["flt"].view(N, K, 1, 1), ws=ws2)
        head.head_forward(s(i)["flt"], s(i)["ov"], w1, b1, None, w2, b2, None, s(i)["h"], s(i)["prob"], phase=head.TEST)

    shape = score_tail.score_tail_shape(conv.conv_shape(N, C, H, W, K, k), p, pool, F1, HID, CLS)
    fns = {"fused": ours("fused"), "sequence": ours("sequence"), "two calls": two_calls}
    iters = 20 if N <= 100 else 5
    print("%s N=%d (%d,%d,%d)->%d %dx%d, %s window %dx%d, head %d+%d -> %d -> %d: %d operand sets of %.2f MB, %d calls "
          "per pass, mms_score_tail_route = %d" % (name, N, C, H, W, K, k, k, "MAX" if pool else "AVE", p, p, K, F1, HID,
                                                   CLS, nsets, per_set / 1e6, iters, score_tail.score_tail_route(shape)))
    res = measure(fns, iters)
    for key, v in res.items():
        if isinstance(v, str):
            print("  %-9s not measured (%s)" % (key, v))
            continue
        extra = ""
        if key == "fused" and not isinstance(res["sequence"], str):
            extra = "  sequence / fused = %.2f" % (res["sequence"][0] / v[0])
        print("  %-9s median %10.1f us  range %10.1f .. %10.1f%s" % (key, v[0], v[1], v[2], extra))
    del sets
    torch.cuda.empty_cache()


if __name__ == "__main__":
    steps = sys.argv[1:] or ["v4:50", "v4:100", "v4:400", "v4:1517", "v5:50", "v5:1517"]
    print("device: %s; torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    for step in steps:
        name, n = step.split(":")
        bench(name, int(n))
