"""tools/embed_f16_timing.py -- dev-only: the fp16-storage Embed calls against the fp32 ones on the same ids, in one process.
HIP events around one pass over a ring of operand sets larger than the last-level cache (every call reads its operands from
HBM), the variants alternating, REPS passes each; prints median, min and max per call in us.

Two batches, N = 50, a 100000-row table, 40 % of the ids on the zero-pad word (one long segment) and the rest uniform:
  M0 = M1 = 2000 (network_v4's training batch): the inverted index is built beside the pair forward, the backward is the INDEXED call;
  M0 = M1 = 60680 (M = 121,360): past the one-workgroup index, the backward is the pair call with the device-wide sort.
Backward variants: (a) the _f16 call on half gradient blobs; (b) what a host had to do before: a torch .float() of both blobs, then the
fp32 call; (c) the fp32 call alone on pre-widened blobs.  Forward variants: (a) embed_forward_pair_f16 from a half table; (b) the fp32
pair forward, then a torch .half() of both tops; (c) the fp32 pair forward alone.

  python tools/embed_f16_timing.py [--reps 7] [--out FILE]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mms_answer_selection_amd import capi

RING_BYTES = 768 << 20          # three times the 256 MB last-level cache
K, N = 100000, 50
BATCHES = [(2000, 2000), (60680, 60680)]


def operand_sets(M0, M1, n_sets):
    g = torch.Generator(device="cuda").manual_seed(17)

    def ids(M):
        i = torch.randint(0, K, (M,), device="cuda", generator=g)
        i[torch.rand(M, device="cuda", generator=g) < 0.4] = 0
        return i.float()

    sets = []
    for _ in range(n_sets):
        table = (torch.randn(K, N, device="cuda", generator=g) * 0.4).half()
        d0, d1 = torch.randn(M0, N, device="cuda", generator=g).half(), torch.randn(M1, N, device="cuda", generator=g).half()
        s = dict(i0=ids(M0), i1=ids(M1), table16=table, table32=table.float(), bias=torch.randn(N, device="cuda", generator=g) * 0.1,
                 d0h=d0, d1h=d1, d0f=d0.float(), d1f=d1.float(), wd=torch.zeros(K, N, device="cuda"), bd=torch.zeros(N, device="cuda"),
                 t0h=torch.empty(M0, N, dtype=torch.float16, device="cuda"), t1h=torch.empty(M1, N, dtype=torch.float16, device="cuda"),
                 t0f=torch.empty(M0, N, device="cuda"), t1f=torch.empty(M1, N, device="cuda"), index=capi.EmbedPairIndex())
        s["indexed"] = capi.embed_forward_pair_f16(s["i0"], s["i1"], table, s["t0h"], s["t1h"], bias=s["bias"], index=s["index"])
        sets.append(s)
    return sets


def set_bytes(M0, M1):
    return 2 * K * N * 4 + (M0 + M1) * N * 6          # the gradient table read and written; a blob in either format


def backward(variant, s, ws):
    d0, d1 = (s["d0h"], s["d1h"]) if variant != "c" else (s["d0f"], s["d1f"])
    if variant == "b":
        d0, d1 = d0.float(), d1.float()
    if s["indexed"]:
        f = capi.embed_backward_pair_indexed_f16 if variant == "a" else capi.embed_backward_pair_indexed
        f(s["i0"], s["i1"], d0, d1, s["wd"], s["index"], bias_diff=s["bd"])
    else:
        f = capi.embed_backward_pair_f16 if variant == "a" else capi.embed_backward_pair
        f(s["i0"], s["i1"], d0, d1, s["wd"], bias_diff=s["bd"], ws=ws)


def forward(variant, s, ws):
    if variant == "a":
        capi.embed_forward_pair_f16(s["i0"], s["i1"], s["table16"], s["t0h"], s["t1h"], bias=s["bias"], index=s["index"])
    else:
        capi.embed_forward_pair(s["i0"], s["i1"], s["table32"], s["t0f"], s["t1f"], bias=s["bias"], index=s["index"])
        if variant == "b":
            s["t0f"].half(), s["t1f"].half()


def one_pass(call, variant, sets, ws):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for s in sets:
        call(variant, s, ws)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / len(sets)


LABELS = {("bwd", "a"): "(a) _f16 call on half blobs", ("bwd", "b"): "(b) .float() of both blobs + fp32 call",
          ("bwd", "c"): "(c) fp32 call, blobs pre-widened", ("fwd", "a"): "(a) _f16 pair forward, half table",
          ("fwd", "b"): "(b) fp32 pair forward + .half() of both tops", ("fwd", "c"): "(c) fp32 pair forward"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = ["%s, %d passes per variant, ring of operand sets >= %d MB, K = %d, N = %d" % (
        torch.cuda.get_device_name(0), args.reps, RING_BYTES >> 20, K, N)]
    ws = capi.Workspace()
    for M0, M1 in BATCHES:
        sets = operand_sets(M0, M1, max(4, min(64, -(-RING_BYTES // set_bytes(M0, M1)))))
        for kind, call in (("bwd", backward), ("fwd", forward)):
            for v in "abc":
                one_pass(call, v, sets, ws)            # warm-up pass (workspace and torch's cache are filled here)
            ts = {v: [] for v in "abc"}
            for _ in range(args.reps):
                for v in "abc":
                    ts[v].append(one_pass(call, v, sets, ws))
            for v in "abc":
                t = sorted(ts[v])
                lines.append("%s M0=M1=%-6d %-7s %-46s median %8.2f us   min %8.2f   max %8.2f   (%d sets)" % (
                    kind, M0, "indexed" if (kind == "bwd" and sets[0]["indexed"]) else "", LABELS[kind, v], t[len(t) // 2], t[0], t[-1],
                    len(sets)))
            print("\n".join(lines[-3:]), flush=True)
        del sets
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
