"""Times the double Embed / ranking-metric calls next to their float twins, in one process, by the protocol of DESIGN.md
section 6: HBM-cold rotation over distinct buffer sets (together larger than the 256-MB Infinity Cache where the
shape allows; at least 4 sets), 200 launches captured in one hipGraph and timed between two events, median of 5
replays, mms_null_launch timed the same way in the same run (the launch floor).  Shapes are cfg 4's: 1,517 candidates
in 68 groups for MAP + MRR and AUC, 50 x 80 and 121,360 indices x 50 columns for the Embed backward.

    python tools/bench_f64_embed_rank.py > profiles/f64_embed_rank.txt
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mms_answer_selection_amd import capi

ITERS, REPLAYS, ROTATE_BYTES, MAX_SETS = 200, 5, 768 << 20, 64


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


def nsets(bytes_per_set):
    return int(min(MAX_SETS, max(4, -(-ROTATE_BYTES // max(1, bytes_per_set)))))


def check(rc, what):
    capi.check(rc, what)


def bench_rank(n, groups, stream):
    r = np.random.default_rng(4)
    lib, s = capi.lib(), stream.cuda_stream
    for dt, sfx, wsb in ((torch.float32, "f32", lib.mms_rank_workspace_bytes(n)),
                         (torch.float64, "f64", lib.mms_rank_workspace_bytes_f64(n))):
        k = nsets(4 * n * dt.itemsize)
        sets = []
        for _ in range(k):
            prob = torch.from_numpy(r.standard_normal((n, 2))).to(dt).cuda()
            label = torch.from_numpy((r.uniform(size=n) < 0.1).astype(np.float64)).to(dt).cuda()
            group = torch.from_numpy(np.sort(r.integers(0, groups, n)).astype(np.float64)).to(dt).cuda()
            sets.append((prob, label, group, torch.empty(3, dtype=dt, device="cuda"),
                         torch.empty(1, dtype=torch.int32, device="cuda")))
        ws = torch.empty(int(wsb), dtype=torch.uint8, device="cuda")
        mm, auc = getattr(lib, "mms_rank_map_mrr_" + sfx), getattr(lib, "mms_rank_auc_" + sfx)
        e = dt.itemsize

        def run_mm(i):
            p, l, g, o, eff = sets[i % k]
            check(mm(n, 1, p.data_ptr(), l.data_ptr(), g.data_ptr(), o.data_ptr(), o.data_ptr() + e, eff.data_ptr(),
                     ws.data_ptr(), ws.numel(), s), "map_mrr")

        def run_auc(i):
            p, l, g, o, eff = sets[i % k]
            check(auc(n, 2, 1, p.data_ptr(), l.data_ptr(), 0, 0, o.data_ptr() + 2 * e, ws.data_ptr(), ws.numel(), s), "auc")

        print("  %s  MAP + MRR %8.2f us/call   AUC %8.2f us/call   (%d candidates, %d groups, %d buffer sets)"
              % (sfx, timed(stream, run_mm), timed(stream, run_auc), n, groups, k))


def bench_embed_backward(M, N, K, stream):
    r = np.random.default_rng(5)
    lib, s = capi.lib(), stream.cuda_stream
    for dt, sfx, wsb in ((torch.float32, "f32", lib.mms_embed_workspace_bytes(M, N)),
                         (torch.float64, "f64", lib.mms_embed_workspace_bytes_f64(M, N))):
        k = nsets((M * N + M) * dt.itemsize)
        idx = r.integers(0, K, M)
        idx[r.uniform(size=M) < 0.6] = 0                 # the zero-pad id owns most of a TREC-QA batch
        sets = [(torch.from_numpy(idx.astype(np.float64)).to(dt).cuda(),
                 torch.randn(M, N, device="cuda", dtype=dt)) for _ in range(k)]
        wd = torch.zeros(K, N, dtype=dt, device="cuda")
        bd = torch.zeros(N, dtype=dt, device="cuda")
        ws = torch.empty(int(wsb), dtype=torch.uint8, device="cuda")
        fn = getattr(lib, "mms_embed_backward_" + sfx)

        def run(i):
            ix, dT = sets[i % k]
            check(fn(M, N, K, ix.data_ptr(), dT.data_ptr(), wd.data_ptr(), bd.data_ptr(), ws.data_ptr(), ws.numel(), s),
                  "embed_backward")

        print("  %s  Embed backward %9.2f us/call   (%d indices x %d, vocabulary %d, 60 %% zero-pad id, %d buffer sets)"
              % (sfx, timed(stream, run), M, N, K, k))


if __name__ == "__main__":
    st = torch.cuda.Stream()
    print("mms_null_launch(256): %.2f us/call" % timed(st, lambda i: capi.null_launch(256)))
    print("ranking metrics, cfg 4")
    bench_rank(1517, 68, st)
    print("Embed backward, cfg 4")
    bench_embed_backward(50 * 80, 50, 20000, st)
    bench_embed_backward(121360, 50, 20000, st)
