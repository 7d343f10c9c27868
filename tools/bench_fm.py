"""Times the FM calls (mms_fm_forward_f32 / _backward_f32 / _forward_backward_f32) by the protocol of DESIGN.md section 6:
HBM-cold rotation over distinct buffer sets (together larger than the 256-MB Infinity Cache), 200 launches captured in
one hipGraph and timed between two events, median of 5 replays.  Prints us per call and the fraction of 8 TB/s on the
algorithmic bytes B_fwd = s (N C dim + N), B_bwd = s (2 N C dim + N), B_fused = s (2 N C dim + 2 N), with
mms_null_launch timed the same way beside them (the launch floor).

    python tools/bench_fm.py [N C dim ...]        default: 4096 2 301 and 4096 80 51
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mms_answer_selection_amd import capi

ITERS, REPLAYS, ROTATE_BYTES, PEAK = 200, 5, 768 << 20, 8e12


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


def bench(N, C, dim, stream):
    n = N * C * dim
    nsets = max(4, -(-ROTATE_BYTES // (2 * 4 * n)))
    sets = []
    for _ in range(nsets):
        sets.append(dict(x=torch.randn(N, C, dim, device="cuda") * 0.4, g=torch.randn(N, device="cuda"),
                         top=torch.empty(N, device="cuda"), bd=torch.empty(N, C, dim, device="cuda"),
                         db=torch.empty(1, device="cuda")))
    bias = torch.full((1,), 0.25, device="cuda")
    torch.cuda.synchronize()
    s = lambda i: sets[i % nsets]
    fwd = timed(stream, lambda i: capi.fm_forward(s(i)["x"], s(i)["top"], bias=bias))
    bwd = timed(stream, lambda i: capi.fm_backward(s(i)["x"], s(i)["g"], s(i)["bd"], s(i)["db"]))
    bwd_nobias = timed(stream, lambda i: capi.fm_backward(s(i)["x"], s(i)["g"], s(i)["bd"], None))
    fused = timed(stream, lambda i: capi.fm_forward_backward(s(i)["x"], s(i)["g"], s(i)["top"], s(i)["bd"], bias=bias,
                                                             bias_diff=s(i)["db"]))
    null = timed(stream, lambda i: capi.null_launch(256))
    chain = (dim - 1) * (C + 1) + C + 1
    print("FM %d x %d x %d f32, %d buffer sets of %.1f MB, chain %d adds per sample, mms_null_launch %.2f us"
          % (N, C, dim, nsets, 2 * 4 * n / 1e6, chain, null))
    for name, us, b in (("forward", fwd, 4 * (n + N)), ("backward", bwd, 4 * (2 * n + N)),
                        ("backward, bias_diff = NULL", bwd_nobias, 4 * (2 * n + N)),
                        ("fused", fused, 4 * (2 * n + 2 * N))):
        print("  %-28s %8.2f us/call  %7.2f MB  %.3f of 8 TB/s" % (name, us, b / 1e6, b / (us * 1e-6) / PEAK))


if __name__ == "__main__":
    a = [int(v) for v in sys.argv[1:]]
    shapes = [tuple(a[i:i + 3]) for i in range(0, len(a), 3)] or [(4096, 2, 301), (4096, 80, 51)]
    st = torch.cuda.Stream()
    for shape in shapes:
        bench(*shape, st)
