"""Times the classifier-head calls (include/mms_head.h) on network_v4's head (64 + 2 features, 32 hidden units, 2
classes, TRAIN, ratio 0.5), forward (with the loss) and backward (all six diffs), at N = 50 (the training batch),
N = 1517 (the test split) and N = 65536: float on the route mms_head_route picks (fast) and on the generic route, double
(generic).  Next to them, in the same process and alternating pass by pass, the sequence a host would issue in torch
without this feature: cat, F.linear, tanh, mask multiply, F.linear, log_softmax + nll_loss, and autograd's backward of
that graph (its forward is recorded outside the timed region).

Protocol: every call of a pass takes the next of a ring of operand sets that together exceed the 256-MB Infinity Cache
(at least two sets), and the ring position carries on from pass to pass and from candidate to candidate, so no operand
is cache-warm from an earlier call; a pass is `iters` calls between two HIP events on one stream; two untimed warm-up
passes, then seven timed ones; the table gives the median pass and the range, in us per call, the ratio torch / ours of
the medians, and the launches per call of each of our routes.  For medians over fresh processes run it several times;
the committed profile is three runs.

    python tools/bench_head.py [N ...]        default: 50 1517 65536
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from mms_answer_selection_amd import capi, head

PASSES, WARMUP, RING_BYTES, MAX_SETS = 7, 2, 320 << 20, 8192
F0, F1, H, C = 64, 2, 32, 2
SINGLE = 256                    # csrc/head.hip: kHeadSingleSamples


def launches(route, N, f64):
    """Launches per (forward with a loss, backward with parameter diffs), from csrc/head.hip's host code."""
    if route == "auto" and not f64:
        return (1, 1) if N <= SINGLE else (2, 2)
    return 3, 4


def one_pass(fn, base, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(base, base + iters):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / iters


def measure(fns, iters, prepare=None):
    us = {k: [] for k in fns}
    base = 0
    for p in range(WARMUP + PASSES):
        for k, f in fns.items():
            if prepare and k in prepare:
                prepare[k](base, iters)
            t = one_pass(f, base, iters)
            base += iters
            if p >= WARMUP:
                us[k].append(t)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in us.items()}


def bench(N, dtype):
    f64 = dtype == torch.float64
    size = 8 if f64 else 4
    per_set = size * N * (2 * (F0 + F1) + 2 * H + 2 * C + 1) + 4 * N * H
    nsets = min(MAX_SETS, max(2, -(-RING_BYTES // per_set)))
    g = torch.Generator(device="cuda").manual_seed(1701)
    rnd = lambda *s: torch.rand(*s, device="cuda", dtype=dtype, generator=g) * 2 - 1
    new = lambda *s: torch.empty(*s, device="cuda", dtype=dtype)
    sets = []
    for _ in range(nsets):
        mask = (torch.rand(N, H, device="cuda", generator=g) >= 0.5)
        sets.append(dict(x0=rnd(N, F0), x1=rnd(N, F1).abs(), mask=mask.to(torch.int32), maskf=mask.to(dtype) * 2,
                         label=torch.randint(0, C, (N,), device="cuda", generator=g).to(dtype), h=new(N, H), prob=new(N, C),
                         dx0=new(N, F0), dx1=new(N, F1)))
    for s in sets:
        s["labeli"] = s["label"].long()
    w1, b1 = rnd(H, F0 + F1) * (3.0 / (F0 + F1)) ** 0.5, rnd(H) * 0.2
    w2, b2 = rnd(C, H) * (6.0 / H) ** 0.5, rnd(C) * 0.2
    dw1, db1, dw2, db2 = (torch.zeros_like(t) for t in (w1, b1, w2, b2))
    loss = new(1)
    ws = capi.Workspace()
    fwd, bwd = (head.head_forward_f64, head.head_backward_f64) if f64 else (head.head_forward, head.head_backward)
    s = lambda i: sets[i % nsets]
    for d in sets:                                    # the backward's saved blobs
        fwd(d["x0"], d["x1"], w1, b1, d["mask"], w2, b2, d["label"], d["h"], d["prob"], loss, ws=ws)
    ours_f = lambda route: (lambda i: fwd(s(i)["x0"], s(i)["x1"], w1, b1, s(i)["mask"], w2, b2, s(i)["label"], s(i)["h"],
                                          s(i)["prob"], loss, ws=ws, route=route))
    ours_b = lambda route: (lambda i: bwd(s(i)["x0"], s(i)["x1"], w1, w2, s(i)["mask"], s(i)["h"], s(i)["prob"],
                                          s(i)["label"], 1.0, s(i)["dx0"], s(i)["dx1"], dw1, db1, dw2, db2, ws=ws,
                                          route=route))

    def graph(d, x0, x1, pw1, pb1, pw2, pb2):
        hh = torch.tanh(F.linear(torch.cat([x0, x1], dim=1), pw1, pb1))
        return F.nll_loss(F.log_softmax(F.linear(hh * d["maskf"], pw2, pb2), dim=1), d["labeli"])

    def torch_f(i):
        with torch.no_grad():
            graph(s(i), s(i)["x0"], s(i)["x1"], w1, b1, w2, b2)

    recorded = {}

    def record(base, iters):                          # autograd graphs for one pass, built outside the timed region
        recorded.clear()
        for i in range(base, base + iters):
            leaves = [t.detach().requires_grad_() for t in (s(i)["x0"], s(i)["x1"], w1, b1, w2, b2)]
            recorded[i] = (graph(s(i), *leaves), leaves)
        torch.cuda.synchronize()

    def torch_b(i):
        out, leaves = recorded[i]
        torch.autograd.grad(out, leaves)

    routes = ["generic"] if f64 else ["auto", "generic"]
    iters = 20 if N <= 2000 else 3
    label = {"auto": "fast", "generic": "generic"}
    fns_f = {label[r]: ours_f(r) for r in routes}
    fns_b = {label[r]: ours_b(r) for r in routes}
    fns_f["torch"], fns_b["torch"] = torch_f, torch_b
    shape = head.head_shape(N, F0, F1, H, C)
    picked = [head.head_route(shape, p) for p in range(2)]
    print("head N=%d (%d+%d)->%d->%d %s: %d operand sets of %.3f MB, %d calls per pass, mms_head_route (fwd, bwd) = %s"
          % (N, F0, F1, H, C, "f64" if f64 else "f32", nsets, per_set / 1e6, iters, picked))
    for k, (what, fns, prep) in enumerate((("forward", fns_f, None), ("backward", fns_b, {"torch": record}))):
        res = measure(fns, iters, prep)
        for name, v in res.items():
            extra = ""
            if name != "torch":
                route = "auto" if name == "fast" else "generic"
                extra = "  torch / this = %.2f  launches %d" % (res["torch"][0] / v[0], launches(route, N, f64)[k])
            print("  %-9s %-8s median %10.1f us  range %10.1f .. %10.1f%s" % (what, name, v[0], v[1], v[2], extra))
    del sets, recorded
    torch.cuda.empty_cache()


if __name__ == "__main__":
    batches = [int(v) for v in sys.argv[1:]] or [50, 1517, 65536]
    print("device: %s; torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    for N in batches:
        for dtype in (torch.float32, torch.float64):
            bench(N, dtype)
