"""Times Dropout (include/mms_dropout.h: mms_dropout_forward_f32 / _backward_f32, the mask regenerated in the backward,
nothing stored) at network_v4's sim_drop shapes -- the SimCross top, N x 4 x 40 x 40, ratio 0.1, at the driver's train
batch (N = 50, do_trec_qa_clean.py:66) and at N = 1517 -- and next to it, in the same process and alternating pass by
pass, what a host without these calls would run:

  torch fwd        torch.nn.functional.dropout(x, 0.1, training=True) under no_grad
  torch fwd+bwd    the same with autograd, then torch.autograd.grad(y, x, dy): its backward reads the mask it stored

Protocol: every call of a pass takes the next of a ring of operand sets (x, y, dy, dx); the ring is sized so that the
two arrays one direction touches exceed the 256-MB Infinity Cache over the ring on their own (at least two sets), and
the ring position carries on from pass to pass and from candidate to candidate; a
pass is `iters` calls between two HIP events on one stream; two untimed warm-up passes, then seven timed ones; the table
gives the median pass and the range in us per call, the ratio torch / this of the medians, and the bytes per second a
call of this library achieves on its compulsory traffic (one array read, one written, per direction).  `sequence`
advances with every call, as a host's iteration counter would.  torch allocates its outputs itself; so that its
allocator cannot hand the same, cache-warm block back on every call, the results of the last `nsets` torch calls are
kept alive in a ring of their own: torch's written arrays rotate through as many distinct blocks as this library's.

    python tools/bench_dropout.py [--batch N ...] [--out profiles/dropout_bench.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from mms_answer_selection_amd import dropout

PASSES, WARMUP, RING_BYTES = 7, 2, 320 << 20
RATIO, SEED = 0.1, 1701


def one_pass(fn, base, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(base, base + iters):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / iters


def measure(fns, iters):
    us = {k: [] for k in fns}
    base = 0
    for p in range(WARMUP + PASSES):
        for k, f in fns.items():
            t = one_pass(f, base, iters)
            base += iters
            if p >= WARMUP:
                us[k].append(t)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in us.items()}


def bench(N, dtype, out):
    size = 8 if dtype == torch.float64 else 4
    shape = (N, 4, 40, 40)
    n = N * 4 * 40 * 40
    per_set = 4 * size * n
    nsets = max(2, -(-RING_BYTES // (per_set // 2)))      # a forward-only candidate touches half of every set
    gen = torch.Generator(device="cuda").manual_seed(1701)
    rnd = lambda: torch.randn(shape, device="cuda", dtype=dtype, generator=gen)
    sets = [(rnd(), torch.empty(shape, device="cuda", dtype=dtype), rnd(), torch.empty(shape, device="cuda", dtype=dtype))
            for _ in range(nsets)]
    leaves = [s[0].clone().requires_grad_() for s in sets]
    held = [None] * nsets                                      # torch's outputs of the last nsets calls, kept alive

    def this_fwd(i):
        x, y, _, _ = sets[i % nsets]
        dropout.dropout_forward(x, RATIO, SEED, i, out=y)

    def this_bwd(i):
        _, _, dy, dx = sets[i % nsets]
        dropout.dropout_backward(dy, RATIO, SEED, i, out=dx)

    def this_both(i):
        this_fwd(i)
        this_bwd(i)

    def torch_fwd(i):
        with torch.no_grad():
            held[i % nsets] = F.dropout(sets[i % nsets][0], RATIO, training=True)

    def torch_both(i):
        x = leaves[i % nsets]
        y = F.dropout(x, RATIO, training=True)
        held[i % nsets] = (y.detach(), torch.autograd.grad(y, x, sets[i % nsets][2]))

    fns = {"this fwd": this_fwd, "this bwd": this_bwd, "this fwd+bwd": this_both, "torch fwd": torch_fwd,
           "torch fwd+bwd": torch_both}
    iters = max(20, min(200, int(2e9 // per_set)))
    out("dropout %s: %d x 4 x 40 x 40 = %d elements, ratio %.1f, %.2f MB per operand set, %d sets, %d calls per pass"
        % ("f64" if size == 8 else "f32", N, n, RATIO, per_set / 1e6, nsets, iters))
    res = measure(fns, iters)
    for name, v in res.items():
        if name.startswith("this"):
            arrays = 4 if name.endswith("fwd+bwd") else 2
            extra = "  %7.1f GB/s on %d bytes per element" % (arrays * size * n / v[0] / 1e3, arrays * size)
        else:
            ours = res["this fwd" if name == "torch fwd" else "this fwd+bwd"][0]
            extra = "  torch / this = %.2f" % (v[0] / ours)
        out("  %-14s median %8.1f us  range %8.1f .. %8.1f%s" % (name, v[0], v[1], v[2], extra))
    del sets, leaves, held
    torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="*", default=[50, 1517])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "dropout_bench.txt"))
    a = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out("tools/bench_dropout.py (us per call between two HIP events around the Python calls; torch / this: ratio of the "
        "medians)")
    out("device: %s; torch %s; %d lanes per workgroup, at most %d workgroups per launch"
        % (torch.cuda.get_device_name(0), torch.__version__, dropout.THREADS, dropout.MAX_BLOCKS))
    out("note: the times include the host side of every call (ctypes for this library, the dispatcher and autograd for "
        "torch), which is what a small shape mostly measures")
    for N in a.batch:
        for dtype in (torch.float32, torch.float64):
            bench(N, dtype, out)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
