"""Times the solver update (include/mms_solver.h: mms_solver_step_f32, AdaDelta with network_v4's hyper-parameters,
MMS_SOLVER_DIFF_ZERO, no clipping: one launch) on network_v4's 20 learnable blobs, and next to it, in the same process,
on tensors of the same sizes and alternating pass by pass:

  torch per blob   a torch restatement of the reference's per-blob GPU sequence: the regularizer's axpy, the AdaDelta
                   update expression (one fused kernel in the reference, ten elementwise torch calls here), Blob::Update's
                   axpy, and the memset of Net::ClearParamDiffs
  torch foreach    torch.optim.Adadelta(foreach=True).step() + zero_grad(set_to_none=False)

and the same call with clipping on (three launches) and in double.

The blob list (do_trec_qa_clean.py): the word table V x 50 and its bias, SimCross 4 x 50 x 50 and its bias, conv0
3200 + 32, BN 4 x 32, conv1 51200 + 64, BN 4 x 64, fc1 32 x 66 + 32, fc2 2 x 32 + 2.  V is a flag: the driver's
vocabulary is not part of this repository, so the V used is an ASSUMPTION that the output records.

Protocol: every call of a pass takes the next of a ring of blob sets that together exceed the 256-MB Infinity Cache
(at least two sets), the ring position carrying on from pass to pass and from candidate to candidate; a pass is `iters`
calls between two HIP events on one stream; two untimed warm-up passes, then seven timed ones; the table gives the
median pass and the range in us per call, the ratio torch / ours of the medians, and the bytes per second the call
achieves on its compulsory traffic (32 bytes per element in float: four arrays read, four written).

Not live gradients: every candidate zeroes the diffs it is handed (DIFF_ZERO, zero_grad, g.zero_()) and nothing
refills them, so from a blob set's second use on its diffs are all zero, and the clipping candidate's norm is 0.  The
kernels take no value-dependent branch, so the times are of the same work; the output says so next to the figures.

    python tools/bench_solver.py [--vocab V ...] [--out profiles/solver_bench.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mms_answer_selection_amd import capi, solver

PASSES, WARMUP, RING_BYTES = 7, 2, 320 << 20
MOMENTUM, DELTA, WEIGHT_DECAY, RATE = 0.95, 5e-7, 5e-4, 1.0


def blob_sizes(V):
    return ([V * 50, 50, 4 * 50 * 50, 4, 3200, 32] + [32] * 4 + [51200, 64] + [64] * 4 + [32 * 66, 32, 2 * 32, 2])


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


def torch_per_blob(blobs):
    """The reference's GPU sequence, blob by blob, as torch calls (sgd_solver.cpp:175-191, adadelta_solver.cu,
    blob.cpp:161, net.cpp:923)."""
    om = 1.0 - MOMENTUM
    for w, g, h, h2 in blobs:
        g.add_(w, alpha=WEIGHT_DECAY)
        h.mul_(MOMENTUM).addcmul_(g, g, value=om)
        u = h2.add(DELTA).div_(h.add(DELTA)).sqrt_()
        g.mul_(u)
        h2.mul_(MOMENTUM).addcmul_(g, g, value=om)
        g.mul_(RATE)
        w.sub_(g)
        g.zero_()


def bench(V, dtype, out):
    size = 8 if dtype == torch.float64 else 4
    sizes = blob_sizes(V)
    total = sum(sizes)
    per_set = 4 * size * total
    nsets = max(2, -(-RING_BYTES // per_set))
    gen = torch.Generator(device="cuda").manual_seed(1701)
    rnd = lambda n: torch.rand(n, device="cuda", dtype=dtype, generator=gen) * 2 - 1
    sets, tables, optims = [], [], []
    for _ in range(nsets):
        blobs = [(rnd(n), rnd(n), rnd(n).abs(), rnd(n).abs() * 1e-3) for n in sizes]
        sets.append(blobs)
        tables.append(solver.solver_blobs([b + (1.0, 1.0) for b in blobs]))
        params = [b[0].requires_grad_() for b in blobs]
        for b in blobs:
            b[0].grad = b[1]
        opt = torch.optim.Adadelta(params, lr=RATE, rho=MOMENTUM, eps=DELTA, weight_decay=WEIGHT_DECAY, foreach=True)
        opt.step()                                    # creates its state (of the same size as ours)
        optims.append(opt)
    hyper = dict(momentum=MOMENTUM, delta=DELTA, weight_decay=WEIGHT_DECAY, diff_out=solver.DIFF_ZERO)
    plain, clipped = solver.solver_param(**hyper), solver.solver_param(clip_gradients=1e30, **hyper)
    step = solver.solver_step_f64 if dtype == torch.float64 else solver.solver_step
    ws = capi.Workspace()

    def torch_blobs(i):
        with torch.no_grad():
            torch_per_blob(sets[i % nsets])

    def torch_foreach(i):
        optims[i % nsets].step()
        optims[i % nsets].zero_grad(set_to_none=False)

    fns = {"this, 1 launch": lambda i: step(plain, tables[i % nsets], RATE),
           "this, clip, 3": lambda i: step(clipped, tables[i % nsets], RATE, ws=ws),
           "torch per blob": torch_blobs, "torch foreach": torch_foreach}
    iters = max(4, min(20, nsets))
    out("solver AdaDelta %s: V = %d (assumed), %d blobs, %d elements, %.1f MB per blob set, %d sets, %d calls per pass"
        % ("f64" if size == 8 else "f32", V, len(sizes), total, per_set / 1e6, nsets, iters))
    res = measure(fns, iters)
    ours = res["this, 1 launch"][0]
    for name, v in res.items():
        extra = ""
        if name.startswith("this"):
            extra = "  %7.1f GB/s on %d bytes per element" % (2 * per_set / v[0] / 1e3, 8 * size)
        else:
            extra = "  torch / this = %.2f" % (v[0] / ours)
        out("  %-15s median %9.1f us  range %9.1f .. %9.1f%s" % (name, v[0], v[1], v[2], extra))
    del sets, tables, optims
    torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, nargs="*", default=[20000, 100000])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "solver_bench.txt"))
    a = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out("tools/bench_solver.py (us per call between two HIP events around the Python calls; torch / this: ratio of the "
        "medians)")
    out("device: %s; torch %s; CHUNK %d, BLOBS_PER_LAUNCH %d" % (torch.cuda.get_device_name(0), torch.__version__,
                                                              solver.CHUNK, solver.BLOBS_PER_LAUNCH))
    out("note: every candidate zeroes the diffs it is handed and nothing refills them, so after a blob set's first use "
        "its diffs are all zero (the clipping candidate's norm is then 0 and nothing is scaled): the times are of the "
        "same streaming code over the same bytes, not of steps on live gradients")
    for V in a.vocab:
        for dtype in (torch.float32, torch.float64):
            bench(V, dtype, out)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
