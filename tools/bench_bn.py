"""Times the BN calls (mms_bn_forward_f32 TRAIN and TEST, mms_bn_backward_f32) by the protocol of DESIGN.md section 6:
HBM-cold rotation over distinct buffer sets (together larger than the 256-MB Infinity Cache), 200 calls captured in one
hipGraph and timed between two events, median of 5 replays.  Prints us per call and the fraction of 8 TB/s on the
COMPULSORY bytes B_fwd = 2 s NCS (read x, write top) and B_bwd = 3 s NCS (read x and top_diff, write bottom_diff); the
kernels move 3 and 5 (one more read of x for the statistics, of x and top_diff for the backward sums), which the L2 /
Infinity Cache serves when a channel's share fits.  mms_null_launch is timed the same way beside them (the launch floor).

As a yardstick only, torch.nn.functional.batch_norm (training) forward + backward on the same tensors in the same
process: eager, 50 iterations between two events after 5 warm-up iterations -- at the two small shapes that is a
measurement of its launches, not of its kernels.

    python tools/bench_bn.py [N C S ...]      default: 50 32 1296, 50 64 25, 1517 32 1296, 1517 64 25
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mms_answer_selection_amd import capi

ITERS, REPLAYS, ROTATE_BYTES, PEAK = 200, 5, 768 << 20, 8e12
TORCH_ITERS, TORCH_WARMUP = 50, 5


def timed(stream, launch):
    """launch(i) enqueues call i; -> median us per call over REPLAYS replays of a graph of ITERS calls."""
    with torch.cuda.stream(stream):
        for i in range(3):
            launch(i)
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            for i in range(ITERS):
                launch(i)
        g.replay()
        stream.synchronize()
        us = []
        for _ in range(REPLAYS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            g.replay()
            e1.record(stream)
            stream.synchronize()
            us.append(e0.elapsed_time(e1) * 1000.0 / ITERS)
    return statistics.median(us)


def torch_yardstick(sets):
    """F.batch_norm(training=True) forward + backward (x, weight and bias gradients), eager; -> us per fwd + bwd."""
    C = sets[0]["x"].shape[1]
    w = torch.ones(C, device="cuda", requires_grad=True)
    b = torch.zeros(C, device="cuda", requires_grad=True)
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")

    def step(i):
        s = sets[i % len(sets)]
        x = s["x"].detach().requires_grad_(True)
        y = torch.nn.functional.batch_norm(x, rm, rv, w, b, True, 0.1, 1e-9)
        y.backward(s["dy"])
        w.grad = b.grad = None

    for i in range(TORCH_WARMUP):
        step(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(TORCH_ITERS):
        step(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / TORCH_ITERS


def bench(N, C, S, stream):
    n = N * C * S
    nsets = max(4, -(-ROTATE_BYTES // (2 * 4 * n)))
    sets = []
    for _ in range(nsets):
        sets.append(dict(x=torch.randn(N, C, S, device="cuda") * 0.8 + 0.3, dy=torch.randn(N, C, S, device="cuda"),
                         top=torch.empty(N, C, S, device="cuda"), dx=torch.empty(N, C, S, device="cuda")))
    scale, shift = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda")
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    mean, std = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    dscale, dshift = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    ws = capi.Workspace()
    torch.cuda.synchronize()
    s = lambda i: sets[i % nsets]
    fwd = lambda phase: (lambda i: capi.bn_forward(s(i)["x"], scale, shift, rm, rv, s(i)["top"], mean, std, phase=phase,
                                                   ws=ws))
    train = timed(stream, fwd(0))
    test = timed(stream, fwd(1))
    with torch.cuda.stream(stream):
        fwd(0)(0)                                # the backward below reads batch statistics, not the TEST phase's
    bwd = timed(stream, lambda i: capi.bn_backward(s(i)["x"], s(i)["dy"], scale, mean, std, s(i)["dx"], dscale, dshift,
                                                   ws=ws))
    null = timed(stream, lambda i: capi.null_launch(256))
    yard = torch_yardstick(sets)
    wsb = capi.bn_workspace_bytes(N, C, S)
    route = "one launch per pass (one workgroup per channel)" if wsb == 0 else \
        "two launches per pass, %d chunks per channel" % (wsb // (C * 16))
    print("BN %d x %d x %d f32, %.2f MB per tensor, %d buffer sets, %s, mms_null_launch %.2f us"
          % (N, C, S, 4 * n / 1e6, nsets, route, null))
    for name, us, b in (("forward TRAIN", train, 2 * 4 * n), ("backward", bwd, 3 * 4 * n),
                        ("forward TRAIN + backward", train + bwd, 5 * 4 * n), ("forward TEST", test, 2 * 4 * n)):
        print("  %-28s %9.2f us/call  %8.2f MB compulsory  %.3f of 8 TB/s" % (name, us, b / 1e6, b / (us * 1e-6) / PEAK))
    print("  %-28s %9.2f us      (yardstick: eager, launches included)" % ("torch batch_norm fwd + bwd", yard))


if __name__ == "__main__":
    a = [int(v) for v in sys.argv[1:]]
    shapes = [tuple(a[i:i + 3]) for i in range(0, len(a), 3)] or [(50, 32, 1296), (50, 64, 25), (1517, 32, 1296),
                                                                  (1517, 64, 25)]
    st = torch.cuda.Stream()
    for shape in shapes:
        bench(*shape, st)
