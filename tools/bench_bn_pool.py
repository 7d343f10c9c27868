"""Times the fused BN -> AvePool -> TanH calls (mms_bn_pool_tanh_forward_f32 TRAIN and TEST, mms_bn_pool_tanh_backward_f32)
by the protocol of tools/bench_bn.py: HBM-cold rotation over distinct buffer sets (together larger
than the 256-MB Infinity Cache), 200 calls captured in one hipGraph and timed between two events, median of 5 replays.
Beside each, in the same process and with the replays ALTERNATING (fused, layered, BN alone, fused, ...):

  layered   what a host did before the fused call: mms_bn_forward_f32, then torch's avg_pool2d and an in-place tanh;
            backward: torch's tanh_backward and avg_pool2d_backward, then mms_bn_backward_f32
  BN alone  mms_bn_forward_f32 / mms_bn_backward_f32 on the same x, nothing after it

Prints us per call and, for the fused call, the fraction of 8 TB/s on its COMPULSORY bytes (s = 4, P = pooled elements
per map): forward N C (H W + 2 P) s (read x, write save_pool and top), backward N C (2 H W + 3 P) s (read x, write
bottom_diff; read top, top_diff, save_pool).

    python tools/bench_bn_pool.py [N C H W kh kw ...] > profiles/bn_pool_bench.txt
    default: network_v4's four shapes, 50 / 1517 x 32 x 36 x 36 with 4 x 4 windows, 50 / 1517 x 64 x 5 x 5 with 5 x 5
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mms_answer_selection_amd import capi

ITERS, REPLAYS, ROTATE_BYTES, PEAK = 200, 5, 768 << 20, 8e12
aten = torch.ops.aten


def timed_alternating(stream, launches):
    """launches: {name: launch(i)}; -> {name: median us per call over REPLAYS replays of a graph of ITERS calls}, the
    graphs replayed in turn within each round."""
    graphs = {}
    with torch.cuda.stream(stream):
        for name, launch in launches.items():
            for i in range(3):
                launch(i)
            stream.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream):
                for i in range(ITERS):
                    launch(i)
            g.replay()
            stream.synchronize()
            graphs[name] = g
        us = {name: [] for name in graphs}
        for _ in range(REPLAYS):
            for name, g in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                g.replay()
                e1.record(stream)
                stream.synchronize()
                us[name].append(e0.elapsed_time(e1) * 1000.0 / ITERS)
    return {name: statistics.median(v) for name, v in us.items()}


def bench(N, C, H, W, kh, kw, stream):
    n, k = N * C * H * W, (kh, kw)
    pooled = (N, C, H // kh, W // kw)
    p = n // (kh * kw)
    nsets = max(4, -(-ROTATE_BYTES // (2 * 4 * n)))
    dev = dict(device="cuda")
    sets = []
    for _ in range(nsets):
        sets.append(dict(x=torch.randn(N, C, H, W, **dev) * 0.8 + 0.3, dx=torch.empty(N, C, H, W, **dev),
                         bn_top=torch.empty(N, C, H, W, **dev), top=torch.empty(pooled, **dev),
                         save_pool=torch.empty(pooled, **dev), top_diff=torch.randn(pooled, **dev)))
    scale, shift = torch.rand(C, **dev) + 0.5, torch.randn(C, **dev)
    rm, rv = torch.zeros(C, **dev), torch.ones(C, **dev)
    mean, std = torch.empty(C, **dev), torch.empty(C, **dev)
    dscale, dshift = torch.empty(C, **dev), torch.empty(C, **dev)
    ws = capi.Workspace()
    s = lambda i: sets[i % nsets]

    def fused_fwd(phase):
        return lambda i: capi.bn_pool_tanh_forward(s(i)["x"], k, scale, shift, rm, rv, s(i)["top"], s(i)["save_pool"],
                                                   mean, std, phase=phase, ws=ws)

    def bn_fwd(phase):
        return lambda i: capi.bn_forward(s(i)["x"], scale, shift, rm, rv, s(i)["bn_top"], mean, std, phase=phase, ws=ws)

    def layered_fwd(phase):
        def f(i):
            bn_fwd(phase)(i)
            torch.nn.functional.avg_pool2d(s(i)["bn_top"], k).tanh_()
        return f

    def fused_bwd(i):
        capi.bn_pool_tanh_backward(s(i)["x"], k, s(i)["top"], s(i)["top_diff"], s(i)["save_pool"], scale, mean, std,
                                   s(i)["dx"], dscale, dshift, ws=ws)

    def bn_bwd(i, dy=None):
        capi.bn_backward(s(i)["x"], s(i)["bn_top"] if dy is None else dy, scale, mean, std, s(i)["dx"], dscale, dshift,
                         ws=ws)

    def layered_bwd(i):
        g = aten.tanh_backward(s(i)["top_diff"], s(i)["top"])
        bn_bwd(i, aten.avg_pool2d_backward(g, s(i)["bn_top"], list(k), list(k), [0, 0], False, True, None))

    torch.cuda.synchronize()
    out = {}
    for title, phase in (("forward TRAIN", 0), ("forward TEST", 1)):
        out[title] = timed_alternating(stream, {"fused": fused_fwd(phase), "layered": layered_fwd(phase),
                                                "BN alone": bn_fwd(phase)})
    with torch.cuda.stream(stream):
        for i in range(nsets):                   # the backward reads batch statistics and every set's own top / save_pool
            fused_fwd(0)(i)
    out["backward"] = timed_alternating(stream, {"fused": fused_bwd, "layered": layered_bwd, "BN alone": bn_bwd})
    null = timed_alternating(stream, {"null": lambda i: capi.null_launch(256)})["null"]
    wsb = capi.bn_pool_tanh_workspace_bytes(N, C, H, W, kh, kw)
    route = "one launch per pass (one workgroup per channel)" if wsb == 0 else \
        "two launches per pass (TEST forward: one), %d chunks per channel" % (wsb // (C * 16))
    print("BN+pool+tanh %d x %d x %d x %d, %d x %d windows, f32, %.2f MB of x, %d buffer sets, %s, mms_null_launch %.2f us"
          % (N, C, H, W, kh, kw, 4 * n / 1e6, nsets, route, null))
    need = {"forward TRAIN": 4 * (n + 2 * p), "forward TEST": 4 * (n + 2 * p), "backward": 4 * (2 * n + 3 * p)}
    for title, t in out.items():
        b = need[title]
        print("  %-14s fused %8.2f us  (%7.2f MB compulsory, %.3f of 8 TB/s)   layered %8.2f us  (x %.2f)   "
              "BN alone %8.2f us  (x %.2f)" % (title, t["fused"], b / 1e6, b / (t["fused"] * 1e-6) / PEAK, t["layered"],
                                               t["layered"] / t["fused"], t["BN alone"], t["BN alone"] / t["fused"]))
    sys.stdout.flush()


if __name__ == "__main__":
    a = [int(v) for v in sys.argv[1:]]
    shapes = [tuple(a[i:i + 6]) for i in range(0, len(a), 6)] or [(50, 32, 36, 36, 4, 4), (50, 64, 5, 5, 5, 5),
                                                                  (1517, 32, 36, 36, 4, 4), (1517, 64, 5, 5, 5, 5)]
    st = torch.cuda.Stream()
    for shape in shapes:
        bench(*shape, st)
