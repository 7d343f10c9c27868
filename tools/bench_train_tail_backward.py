"""Times the backward of the TRAIN-phase tail Convolution -> BN -> Pool -> TanH -> head at the tails of the driver's
nets, float, every output asked for, in one process and alternating pass by pass:

    fused      mms_train_tail_backward_fused_f32 (include/mms_train_tail_backward.h): the head's backward, the
               coefficients, bottom_diff and the parameter diffs with top_diff formed in their loaders, the reduce --
               whether or not mms_train_tail_backward_route sends the shape there (its rule rests on this table)
    sequence   mms_train_tail_backward_f32: mms_head_backward_f32, then mms_conv_stage_train_backward_f32

Protocol (tools/bench_conv.py's): every call of a pass takes the next of a ring of operand sets (x, y, overlap, mask and
every per-sample array) that together exceed the 256-MB Infinity Cache (at least two sets), so no operand is cache-warm
from the call before; the workspace is one buffer, as a host would keep it; a pass is `iters` calls between two HIP
events on one stream; two untimed warm-up passes, then seven timed ones; the table gives the median pass and the range,
in us per call, and the ratio sequence / fused of the medians.  What the backward reads is a forward's, in every set.

    python tools/bench_train_tail_backward.py [net:N ...]     default: every net at N = 50, 100, 256, 400

N = 400 is past the fused launches' reach (256 samples): its row says so.  One (net, N) per invocation gives each point
a fresh process.  The images of a workgroup (kTrainTailBackwardImages, csrc/train_tail_backward.hip) are a build's:
builds that differ in the constant only are measured by running this tool on each.  The accumulated parameter diffs are
not reset between calls: no timing depends on their values.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench_conv import measure
from mms_answer_selection_amd import capi, conv, conv_stage_train, head, train_tail, train_tail_backward

RING_BYTES = 320 << 20
# C, H, W, K, kernel, window, pool, F1, hidden units, classes: the last stage of network_v4, network_v3 and network_v5
# with the head behind it
NETS = {"v4": (32, 9, 9, 64, 5, 5, train_tail.POOL_AVE, 2, 32, 2),
        "v3": (64, 9, 9, 64, 5, 5, train_tail.POOL_MAX, 2, 64, 2),
        "v5": (32, 8, 8, 32, 3, 6, train_tail.POOL_MAX, 2, 32, 2)}
BATCHES = (50, 100, 256, 400)


def bench(name, N):
    C, H, W, K, k, p, pool, F1, HID, CLS = NETS[name]
    for m in (train_tail_backward, train_tail, head, conv_stage_train, conv):
        m.lib()                # every family's signatures are on the handle before a call goes through it
    OH = H - k + 1
    per_set = 4 * N * (C * H * W + K * OH * OH + 2 * K + F1 + 2 * HID + CLS)
    nsets = max(2, -(-RING_BYTES // per_set))
    g = torch.Generator(device="cuda").manual_seed(1701)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    uni = lambda *s: torch.rand(*s, device="cuda", generator=g)
    new = lambda *s: torch.empty(*s, device="cuda")
    sets = [dict(x=rnd(N, C, H, W) * 0.5, ov=uni(N, F1), mask=(uni(N, HID) >= 0.5).to(torch.int32), y=new(N, K, OH, OH),
                 flt=new(N, K), sp=new(N, K), h=new(N, HID), prob=new(N, CLS), dx=new(N, C, H, W), dov=new(N, F1))
            for _ in range(nsets)]
    w, b = rnd(K, C, k, k) * (C * k * k) ** -0.5, rnd(K) * 0.1
    scale, shift = uni(K) + 0.5, rnd(K) * 0.5
    rm, rv, sm, ss = rnd(K) * 0.5, uni(K) + 0.5, new(K), new(K)
    w1, b1 = (uni(HID, K + F1) * 2 - 1) * (3.0 / (K + F1)) ** 0.5, rnd(HID) * 0.1
    w2, b2 = (uni(CLS, HID) * 2 - 1) * (6.0 / HID) ** 0.5, rnd(CLS) * 0.1
    label, loss = (uni(N) >= 0.5).float(), new(1)
    dw, db, dsc, dsh = torch.zeros_like(w), torch.zeros_like(b), new(K), new(K)
    dw1, db1, dw2, db2 = torch.zeros_like(w1), torch.zeros_like(b1), torch.zeros_like(w2), torch.zeros_like(b2)
    ws = capi.Workspace()
    s = lambda i: sets[i % nsets]

    def forward(route):
        return lambda i: train_tail.train_tail_forward(
            s(i)["x"], w, b, p, pool, scale, shift, rm, rv, s(i)["ov"], w1, b1, s(i)["mask"], w2, b2, label, s(i)["y"],
            s(i)["flt"], s(i)["sp"], sm, ss, s(i)["h"], s(i)["prob"], loss, ws=ws, route=route)

    def backward(call, **kw):
        return lambda i: call(s(i)["x"], w, p, pool, s(i)["y"], s(i)["flt"], s(i)["sp"], scale, shift, sm, ss, s(i)["ov"],
                              w1, w2, s(i)["mask"], s(i)["h"], s(i)["prob"], label, 1.0, s(i)["dx"], dw, db, dsc, dsh,
                              s(i)["dov"], dw1, db1, dw2, db2, ws=ws, **kw)

    for i in range(nsets):     # what the backward reads is a forward's, in every set
        forward("sequence")(i)
    shape = train_tail.train_tail_shape(conv.conv_shape(N, C, H, W, K, k), p, pool, F1, HID, CLS)
    fns = {"fused": backward(train_tail_backward.train_tail_backward_routed, route="fused"),
           "sequence": backward(train_tail.train_tail_backward)}
    iters = 20 if N <= 100 else 5
    print("%s N=%d (%d,%d,%d)->%d %dx%d, %s window %dx%d, head %d+%d -> %d -> %d: %d operand sets of %.2f MB, %d calls "
          "per pass, mms_train_tail_backward_route = %d" % (
              name, N, C, H, W, K, k, k, "MAX" if pool else "AVE", p, p, K, F1, HID, CLS, nsets, per_set / 1e6, iters,
              train_tail_backward.train_tail_backward_route(shape)))
    res = measure(fns, iters)
    for key, v in res.items():
        if isinstance(v, str):
            print("  %-9s not measured (%s)" % (key, v))
            continue
        extra = ""
        if key == "fused" and not isinstance(res["sequence"], str):
            seq = res["sequence"]
            apart = v[2] < seq[1] or seq[2] < v[1]
            extra = "  sequence / fused = %.2f, ranges %s" % (seq[0] / v[0], "apart" if apart else "overlap")
        print("  %-9s median %10.1f us  range %10.1f .. %10.1f%s" % (key, v[0], v[1], v[2], extra))
    del sets
    torch.cuda.empty_cache()


if __name__ == "__main__":
    steps = sys.argv[1:] or ["%s:%d" % (n, N) for n in NETS for N in BATCHES]
    print("device: %s; torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    for step in steps:
        name, n = step.split(":")
        bench(name, int(n))
