"""tools/triplet_cosine_probe.py -- dev-only: the fused cosine (q, a+, a-) step against the Euclid step and against
the seven-launch unfused cosine chain.  One process, per batch size: an HBM-cold ring of distinct operands (>= 1 GiB
of q / a+ / a- / gradients, so no step finds its rows in the 256 MB last-level cache), every variant captured into
hipGraphs over the same ring, the variants timed ALTERNATELY (a, b, c, a, b, c, ...), median and spread of the
repeats.  us per step; the fraction of 8 TB/s is over the 6*N*D*4 bytes the fused step has to move.

  python tools/triplet_cosine_probe.py [--out FILE] [--repeats 9] [--finish inlaunch|launch]
"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mms_answer_selection_amd import capi

PEAK_BPS = 8.0e12
D, G, MARGIN = 300, 16, 0.9


def probe(N, repeats, say):
    slot_bytes = 6 * N * D * 4
    ring = -(-(1 << 30) // slot_bytes)
    ring = -(-ring // G) * G                                   # whole graphs
    gen = torch.Generator(device="cuda").manual_seed(1)
    mk = lambda *s: torch.randn(*s, device="cuda", generator=gen) * 0.4
    q, an = mk(ring, N, 1, D), mk(ring, N, 1, D)
    ap = q + 0.5 * mk(ring, N, 1, D)
    y = (torch.rand(ring, N, 1, device="cuda", generator=gen) < 0.8).float()
    dq, dp, dn = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    tq = [torch.empty_like(q), torch.empty_like(q)]            # the unfused chain's two dq branches, per slot
    col = lambda: torch.empty(ring, N, 1, device="cuda")
    sp, sn, n0p, n1p, n0n, n1n, o, s, gp, gn = (col() for _ in range(10))
    loss = torch.empty(ring, 1, device="cuda")
    ws = capi.TripletWorkspace()
    lib = capi.lib()
    split_args = [(C.c_void_p * 2)(tq[0][i].data_ptr(), tq[1][i].data_ptr()) for i in range(ring)]

    def cosine(i):
        capi.triplet_cosine_step(q[i], ap[i], an[i], y[i], sp[i], sn[i], loss[i], dq[i], dp[i], dn[i], margin=MARGIN,
                                 norms=(n0p[i].view(N), n1p[i].view(N), n1n[i].view(N)), ws=ws)

    def euclid(i):
        capi.triplet_euclid_step(q[i], ap[i], an[i], y[i], sp[i], sn[i], loss[i], dq[i], dp[i], dn[i], margin=MARGIN, ws=ws)

    def chain(i):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        tp, tn = sp[i].view(N, 1, 1, 1), sn[i].view(N, 1, 1, 1)
        capi.simcross_forward(0, q[i], ap[i], tp, norm0=n0p[i], norm1=n1p[i])
        capi.simcross_forward(0, q[i], an[i], tn, norm0=n0n[i], norm1=n1n[i])
        capi.pairrank_forward(sp[i], sn[i], y[i], o[i], s[i], loss[i], margin=MARGIN)
        capi.pairrank_backward(y[i], o[i], s[i], gp[i], gn[i])
        capi.simcross_backward(0, q[i], ap[i], tp, gp[i].view(N, 1, 1, 1), tq[0][i], dp[i], norm0=n0p[i], norm1=n1p[i])
        capi.simcross_backward(0, q[i], an[i], tn, gn[i].view(N, 1, 1, 1), tq[1][i], dn[i], norm0=n0n[i], norm1=n1n[i])
        capi.check(lib.mms_split_backward_f32(N * D, 2, split_args[i], dq[i].data_ptr(), st), "split")

    variants = [("a fused cosine step", cosine), ("b fused euclid step", euclid), ("c unfused cosine chain, 7 launches", chain)]
    graphs = {}
    for name, step in variants:
        for i in range(ring):
            step(i)                                            # warm-up: every slot, eager
        torch.cuda.synchronize()
        cap = torch.cuda.Stream()
        cap.wait_stream(torch.cuda.current_stream())
        gs = []
        with torch.cuda.stream(cap):
            for g0 in range(0, ring, G):
                gph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gph, stream=cap):
                    for i in range(g0, g0 + G):
                        step(i)
                gs.append(gph)
        torch.cuda.current_stream().wait_stream(cap)
        for gph in gs:
            gph.replay()
        torch.cuda.synchronize()
        graphs[name] = gs
    laps = max(4, 1024 // ring)                                # >= 1000 steps per timed window
    ts = {name: [] for name, _ in variants}
    for rep in range(repeats):
        for name, _ in variants:                               # alternate the variants inside every repeat
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(laps):
                for gph in graphs[name]:
                    gph.replay()
            e1.record()
            torch.cuda.synchronize()
            ts[name].append(e0.elapsed_time(e1) * 1e3 / (laps * ring))
    say("N = %d, D = %d: ring of %d slots (%.2f GiB of operands and gradients), %d steps per window, %d repeats"
        % (N, D, ring, ring * slot_bytes / 2.0 ** 30, laps * ring, repeats))
    med = {}
    for name, _ in variants:
        v = sorted(ts[name])
        med[name] = v[len(v) // 2]
        say("  %-36s median %7.2f us   min %7.2f   max %7.2f   (spread %.2f)   %5.1f%% of 8 TB/s on 6*N*D*4 = %.1f MB"
            % (name, med[name], v[0], v[-1], v[-1] - v[0], 100.0 * slot_bytes / (med[name] * 1e-6) / PEAK_BPS, slot_bytes / 1e6))
    a, b, c = (med[name] for name, _ in variants)
    say("  a / c = %.2f   a - b = %+.2f us" % (a / c, a - b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--finish", default="inlaunch", choices=["inlaunch", "launch"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("triplet_cosine_probe: no GPU (there is no CPU fallback)")
    capi.set_triplet_finish_mode(args.finish)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("triplet_cosine_probe: %s, loss finish mode %s" % (torch.cuda.get_device_name(0), args.finish))
    for N in (4096, 16384):
        probe(N, args.repeats, say)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
