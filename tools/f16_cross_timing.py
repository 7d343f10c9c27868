"""tools/f16_cross_timing.py -- dev-only: the fp16-storage word-grid calls against the fp32 entry points on the same shapes, the
inputs widened.  HIP events around one pass over a ring of operand sets larger than the last-level cache (every call reads its
operands from HBM), both variants in one process, alternating, REPS passes each; prints median, min and max per call in us.

The bilinear rows (dist_mode 2, M = 4 with bias; mms_simcross_bilinear_*_f16, mms_embed_simcross_bilinear_forward_f16) time the scoring
forward from grids and from word ids (a 100000-row table) at the test split's 1517 candidates, and forward + backward at a training batch.
The embed rows (dist_mode 1 and 0 from word ids and the same 100000-row table, with the Embed bias) time mms_embed_simcross_forward_f16
against mms_embed_simcross_forward_f32 at those 1517 candidates.

  python tools/f16_cross_timing.py [--reps 7] [--out FILE] [--only elementwise|bilinear|embed]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mms_answer_selection_amd import capi

RING_BYTES = 768 << 20          # per variant: three times the 256 MB last-level cache


def operand_sets(shape, half, n_sets):
    N, W1, W2, D = shape
    g = torch.Generator(device="cuda").manual_seed(7)
    sets = []
    for _ in range(n_sets):
        q = (torch.randn(N, W1, D, device="cuda", generator=g) * 0.4).half()
        a = (torch.randn(N, W2, D, device="cuda", generator=g) * 0.4).half()
        if not half:
            q, a = q.float(), a.float()
        sets.append(dict(q=q, a=a, dT=torch.randn(N, 1, W1, W2, device="cuda", generator=g), top=torch.empty(N, 1, W1, W2, device="cuda"),
                         n0=torch.empty(N, W1, device="cuda"), n1=torch.empty(N, W2, device="cuda"), dq=torch.empty_like(q), da=torch.empty_like(a)))
    return sets


def set_bytes(shape, half):
    N, W1, W2, D = shape
    e = 2 if half else 4
    return 2 * N * (W1 + W2) * D * e + 2 * N * W1 * W2 * 4


def call(kind, mode, half, s):
    n = dict(norm0=s["n0"], norm1=s["n1"]) if mode == 0 else {}
    if kind == "fwd":
        (capi.simcross_forward_f16 if half else capi.simcross_forward)(mode, s["q"], s["a"], s["top"], **n)
    elif kind == "bwd":
        (capi.simcross_backward_f16 if half else capi.simcross_backward)(mode, s["q"], s["a"], s["top"], s["dT"], s["dq"], s["da"], **n)
    else:
        (capi.simcross_forward_backward_f16 if half else capi.simcross_forward_backward)(mode, s["q"], s["a"], s["dT"], s["top"], s["dq"], s["da"], **n)


def one_pass(kind, mode, half, sets):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for s in sets:
        call(kind, mode, half, s)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / len(sets)


CASES = [("fwd", 1, "fp32", (1517, 40, 40, 50)), ("fwd", 0, "fp32", (1517, 40, 40, 50)), ("bwd", 1, "fp32", (1517, 40, 40, 50)),
         ("bwd", 1, "reference", (1517, 40, 40, 50)), ("fwdbwd", 1, "fp32", (64, 40, 40, 300)), ("fwdbwd", 0, "fp32", (64, 40, 40, 300))]


BILINEAR_M, BILINEAR_K = 4, 100000
BILINEAR_CASES = [("fwd", (1517, 40, 40, 50)), ("fwd_ids", (1517, 40, 40, 50)), ("fwdbwd", (50, 40, 40, 50))]


def bilinear_sets(kind, shape, half, n_sets):
    N, W1, W2, D = shape
    M = BILINEAR_M
    g = torch.Generator(device="cuda").manual_seed(11)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    sets, ws = [], capi.Workspace()                 # one workspace per variant: its calls follow each other on one stream
    for _ in range(n_sets):
        s = dict(W=rnd(M, D, D) * 0.08, bias=rnd(M, W1, W2), top=torch.empty(N, M, W1, W2, device="cuda"), ws=ws)
        if kind == "fwd_ids":
            table = (rnd(BILINEAR_K, D) * 0.4).half()
            s.update(table=table if half else table.float(), iq=torch.randint(0, BILINEAR_K, (N, W1), device="cuda", generator=g).float(),
                     ia=torch.randint(0, BILINEAR_K, (N, W2), device="cuda", generator=g).float())
        else:
            q, a = (rnd(N, W1, D) * 0.4).half(), (rnd(N, W2, D) * 0.4).half()
            s.update(q=q if half else q.float(), a=a if half else a.float())
        if kind == "fwdbwd":
            s.update(dT=rnd(N, M, W1, W2), dq=torch.empty_like(s["q"]), da=torch.empty_like(s["a"]), dW=torch.empty_like(s["W"]),
                     dbias=torch.zeros(M, W1, W2, device="cuda"))
        sets.append(s)
    return sets


def bilinear_set_bytes(kind, shape, half):
    N, W1, W2, D = shape
    e = 2 if half else 4
    if kind == "fwd_ids":
        return BILINEAR_K * D * e + N * BILINEAR_M * W1 * W2 * 4
    return (2 if kind == "fwdbwd" else 1) * (N * (W1 + W2) * D * e + N * BILINEAR_M * W1 * W2 * 4)


def bilinear_call(kind, half, s):
    if kind == "fwd":
        if half:
            capi.simcross_bilinear_forward_f16(s["q"], s["a"], s["W"], s["bias"], s["top"], ws=s["ws"])
        else:
            capi.simcross_forward(2, s["q"], s["a"], s["top"], W=s["W"], bias=s["bias"], ws=s["ws"])
    elif kind == "fwd_ids":
        (capi.embed_simcross_bilinear_forward_f16 if half else capi.embed_simcross_bilinear_forward)(s["iq"], s["ia"], s["table"], s["W"], s["bias"],
                                                                                                     s["top"])
    elif half:
        capi.simcross_bilinear_forward_backward_f16(s["q"], s["a"], s["W"], s["bias"], s["dT"], s["top"], s["dq"], s["da"], s["dW"], s["dbias"],
                                                    ws=s["ws"])
    else:
        capi.simcross_forward_backward(2, s["q"], s["a"], s["dT"], s["top"], s["dq"], s["da"], W=s["W"], bias=s["bias"], dW=s["dW"],
                                       dbias=s["dbias"], ws=s["ws"])


def bilinear_pass(kind, half, sets):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for s in sets:
        bilinear_call(kind, half, s)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / len(sets)


def bilinear_rows(reps, lines):
    for kind, shape in BILINEAR_CASES:
        sets = {half: bilinear_sets(kind, shape, half, max(4, min(256, -(-RING_BYTES // bilinear_set_bytes(kind, shape, half))))) for half in (False, True)}
        for half in (False, True):
            bilinear_pass(kind, half, sets[half])   # warm-up pass (the workspaces are allocated here)
        ts = {False: [], True: []}
        for _ in range(reps):
            for half in (False, True):
                ts[half].append(bilinear_pass(kind, half, sets[half]))
        what = "%-7s bilinear M=%d bias  %s" % (kind, BILINEAR_M, "x".join(map(str, shape)))
        for half in (False, True):
            v = sorted(ts[half])
            lines.append("%-44s %-4s median %8.2f us   min %8.2f   max %8.2f   (%d sets)" % (what, "f16" if half else "fp32", v[len(v) // 2], v[0], v[-1],
                                                                                            len(sets[half])))
        print("\n".join(lines[-2:]), flush=True)
        del sets
        torch.cuda.empty_cache()


EMBED_CASES = [(1, (1517, 40, 40, 50)), (0, (1517, 40, 40, 50))]


def embed_sets(shape, half, n_sets):
    N, W1, W2, D = shape
    g = torch.Generator(device="cuda").manual_seed(13)
    sets = []
    for _ in range(n_sets):
        table = (torch.randn(BILINEAR_K, D, device="cuda", generator=g) * 0.4).half()
        sets.append(dict(table=table if half else table.float(), ebias=torch.randn(D, device="cuda", generator=g) * 0.1,
                         iq=torch.randint(0, BILINEAR_K, (N, W1), device="cuda", generator=g).float(),
                         ia=torch.randint(0, BILINEAR_K, (N, W2), device="cuda", generator=g).float(),
                         top=torch.empty(N, 1, W1, W2, device="cuda"), n0=torch.empty(N, W1, device="cuda"), n1=torch.empty(N, W2, device="cuda")))
    return sets


def embed_pass(mode, half, sets):
    f = capi.embed_simcross_forward_f16 if half else capi.embed_simcross_forward
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for s in sets:
        n = dict(norm0=s["n0"], norm1=s["n1"]) if mode == 0 else {}
        f(mode, s["iq"], s["ia"], s["table"], s["top"], embed_bias=s["ebias"], **n)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / len(sets)


def embed_rows(reps, lines):
    for mode, shape in EMBED_CASES:
        N, W1, W2, D = shape
        nbytes = lambda half: BILINEAR_K * D * (2 if half else 4) + N * (W1 + W2) * 4 + N * W1 * W2 * 4
        sets = {half: embed_sets(shape, half, max(4, min(256, -(-RING_BYTES // nbytes(half))))) for half in (False, True)}
        for half in (False, True):
            embed_pass(mode, half, sets[half])      # warm-up pass
        ts = {False: [], True: []}
        for _ in range(reps):
            for half in (False, True):
                ts[half].append(embed_pass(mode, half, sets[half]))
        what = "fwd_ids %s embed bias  %s" % (("cosine", "euclid")[mode], "x".join(map(str, shape)))
        for half in (False, True):
            v = sorted(ts[half])
            lines.append("%-44s %-4s median %8.2f us   min %8.2f   max %8.2f   (%d sets)" % (what, "f16" if half else "fp32", v[len(v) // 2], v[0], v[-1],
                                                                                            len(sets[half])))
        print("\n".join(lines[-2:]), flush=True)
        del sets
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("elementwise", "bilinear", "embed"), default=None)
    args = ap.parse_args()
    lines = ["%s, %d passes per variant, ring of operand sets >= %d MB per variant" % (torch.cuda.get_device_name(0), args.reps, RING_BYTES >> 20)]
    for kind, mode, bwd_mode, shape in (CASES if args.only in (None, "elementwise") else []):
        capi.set_euclid_backward_mode(bwd_mode)
        sets = {half: operand_sets(shape, half, max(4, min(256, -(-RING_BYTES // set_bytes(shape, half))))) for half in (False, True)}
        for half in (False, True):                   # the backward reads a forward's top (and norms)
            for s in sets[half]:
                call("fwd", mode, half, s)
            one_pass(kind, mode, half, sets[half])   # warm-up pass
        ts = {False: [], True: []}
        for _ in range(args.reps):
            for half in (False, True):
                ts[half].append(one_pass(kind, mode, half, sets[half]))
        what = "%-6s %s %-9s %s" % (kind, ("cosine", "euclid")[mode], bwd_mode if (mode == 1 and kind != "fwd") else "", "x".join(map(str, shape)))
        for half in (False, True):
            v = sorted(ts[half])
            lines.append("%-44s %-4s median %8.2f us   min %8.2f   max %8.2f   (%d sets)" % (what, "f16" if half else "fp32", v[len(v) // 2], v[0], v[-1],
                                                                                            len(sets[half])))
        print("\n".join(lines[-2:]), flush=True)
        del sets
        torch.cuda.empty_cache()
    capi.set_euclid_backward_mode("fp32")
    if args.only in (None, "bilinear"):
        bilinear_rows(args.reps, lines)
    if args.only in (None, "embed"):
        embed_rows(args.reps, lines)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
