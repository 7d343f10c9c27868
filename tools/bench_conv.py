"""Times the Convolution calls (include/mms_conv.h) on network_v4's two layers, forward and backward (bottom_diff,
weight_diff and bias_diff in one call), at N = 50 (the driver's training batch) and N = 1517 (the test split): float on
the route mms_conv_route picks (fast) and on the generic route, double (generic).  Next to them, in the same process and
alternating pass by pass, what a host would call without this feature: torch.nn.functional.conv2d and
aten.convolution_backward on the same tensors, float and double.

Protocol: every call of a pass takes the next of a ring of operand sets that together exceed the 256-MB Infinity Cache
(at least two sets), so no operand is cache-warm from the call before; a pass is `iters` calls between two HIP events
on one stream; two untimed warm-up passes, then seven timed ones; the table gives the median pass and the range, in us
per call, and the ratio torch / ours of the medians.

    python tools/bench_conv.py [N ...]        default: 50 1517
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mms_answer_selection_amd import capi, conv

PASSES, WARMUP, RING_BYTES = 7, 2, 320 << 20
LAYERS = [("conv0", 4, 40, 40, 32), ("conv1", 32, 9, 9, 64)]       # (name, C, H, W, K), 5 x 5, stride 1, pad 0


def one_pass(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / iters


def measure(fns, iters):
    """fns: {name: f(i)}.  The candidates take turns, pass by pass.  -> {name: (median, min, max) us per call}, or an
    error string for a candidate that raised."""
    us, failed = {k: [] for k in fns}, {}
    for p in range(WARMUP + PASSES):
        for k, f in fns.items():
            if k in failed:
                continue
            try:
                t = one_pass(f, iters)
            except Exception as e:                       # torch without a convolution backend for this dtype
                failed[k] = "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:80])
                continue
            if p >= WARMUP:
                us[k].append(t)
    return {k: failed.get(k) or (statistics.median(v), min(v), max(v)) for k, v in us.items()}


def bench(name, N, C, H, W, K, dtype):
    f64 = dtype == torch.float64
    size = 8 if f64 else 4
    OH, OW = H - 4, W - 4
    per_set = size * N * (2 * C * H * W + 2 * K * OH * OW)
    nsets = max(2, -(-RING_BYTES // per_set))
    g = torch.Generator(device="cuda").manual_seed(1701)
    rnd = lambda *s: torch.randn(*s, device="cuda", dtype=dtype, generator=g)
    sets = [dict(x=rnd(N, C, H, W) * 0.5, dy=rnd(N, K, OH, OW) * 0.1, top=torch.empty(N, K, OH, OW, device="cuda", dtype=dtype),
                 dx=torch.empty(N, C, H, W, device="cuda", dtype=dtype)) for _ in range(nsets)]
    w, b = rnd(K, C, 5, 5) * (C * 25) ** -0.5, rnd(K) * 0.1
    dw, db = torch.zeros_like(w), torch.zeros_like(b)
    ws = capi.Workspace()
    fwd, bwd = (conv.conv_forward_f64, conv.conv_backward_f64) if f64 else (conv.conv_forward, conv.conv_backward)
    s = lambda i: sets[i % nsets]
    ours_f = lambda route: (lambda i: fwd(s(i)["x"], w, b, s(i)["top"], route=route))
    ours_b = lambda route: (lambda i: bwd(s(i)["x"], w, s(i)["dy"], s(i)["dx"], dw, db, ws=ws, route=route))

    def torch_f(i):
        with torch.no_grad():
            torch.nn.functional.conv2d(s(i)["x"], w, b)

    def torch_b(i):
        torch.ops.aten.convolution_backward(s(i)["dy"], s(i)["x"], w, [K], [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
                                            [True, True, True])

    routes = ["generic"] if f64 else ["auto", "generic"]
    iters = 20 if N <= 100 else 3
    label = {"auto": "fast", "generic": "generic"}
    fns_f = {label[r]: ours_f(r) for r in routes}
    fns_b = {label[r]: ours_b(r) for r in routes}
    fns_f["torch"], fns_b["torch"] = torch_f, torch_b
    shape = conv.conv_shape(N, C, H, W, K, 5)
    picked = [conv.conv_route(shape, p) for p in range(3)]
    print("%s N=%d (%d,%d,%d)->%d 5x5 %s: %d operand sets of %.1f MB, %d calls per pass, mms_conv_route (fwd, bottom, param) = %s"
          % (name, N, C, H, W, K, "f64" if f64 else "f32", nsets, per_set / 1e6, iters, picked))
    gflop = 2.0 * N * K * OH * OW * C * 25 / 1e9
    for what, fns, mult in (("forward", fns_f, 1), ("backward", fns_b, 2)):
        res = measure(fns, iters)
        for k, v in res.items():
            if isinstance(v, str):
                print("  %-9s %-8s not measured (%s)" % (what, k, v))
                continue
            ratio = ""
            if k != "torch" and not isinstance(res["torch"], str):
                ratio = "  torch / this = %.2f" % (res["torch"][0] / v[0])
            print("  %-9s %-8s median %10.1f us  range %10.1f .. %10.1f  %7.2f TFLOP/s%s"
                  % (what, k, v[0], v[1], v[2], mult * gflop / v[0] * 1e3, ratio))
    del sets
    torch.cuda.empty_cache()


if __name__ == "__main__":
    batches = [int(v) for v in sys.argv[1:]] or [50, 1517]
    print("device: %s; torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    for N in batches:
        for (name, C, H, W, K) in LAYERS:
            for dtype in (torch.float32, torch.float64):
                bench(name, N, C, H, W, K, dtype)
