#!/usr/bin/env python3
"""tools/elementwise_routes.py -- one call per row of DESIGN.md 4.4b's routing table, and the listing that pins it.

  run (on the GPU, by itself under the profiler, no counters and no other tracing):
      rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 tools/elementwise_routes.py --labels LABELS \
          [--lib LIBMMS_HIP.SO]
    calls every elementwise entry point once per route, printing `== label` before each call.  --lib loads another
    build of the library (the parent commit's, say) through the same binding.
  listing:
      python3 tools/elementwise_routes.py --listing OUT --labels LABELS > profiles/elementwise_routes.txt
    prints, per label, the (kernel, workgroups, workgroup size, LDS bytes) of every launch the call made.  Two builds
    route alike exactly when their listings are equal line for line.

A one-element torch add precedes every call; in the trace it separates one call's launches from the next's."""
import argparse
import csv
import glob
import re
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--lib")
ap.add_argument("--listing")
ap.add_argument("--labels", help="file the run writes its labels to, and the listing reads them from")
args = ap.parse_args()

ROUTES = []   # (label, function of no arguments), in call order


def build_routes():
    import torch
    from mms_answer_selection_amd import capi
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(7)

    def rnd(*shape, dtype=torch.float32, off=0):
        """off: elements by which the tensor's base is moved off its (16-byte aligned) allocation"""
        n = 1
        for s in shape:
            n *= s
        base = torch.randn(n + off, generator=g).to(dev).to(dtype)
        return base[off:].view(*shape)

    def sim(mode, N, W1, W2, D, off=0):
        q, a = rnd(N, W1, D, off=off), rnd(N, W2, D, off=off)
        top, td = torch.empty(N, 1, W1, W2, device=dev), rnd(N, 1, W1, W2)
        n0, n1 = torch.empty(N * W1, device=dev), torch.empty(N * W2, device=dev)
        dq, da = torch.empty_like(q), torch.empty_like(a)
        return q, a, top, td, n0, n1, dq, da

    def three(tag, mode, N, W1, W2, D, off=0, bwd_modes=("fp32",)):
        shape = "%dx%dx%dx%d%s" % (N, W1, W2, D, " +%dB" % (4 * off) if off else "")
        q, a, top, td, n0, n1, dq, da = sim(mode, N, W1, W2, D, off)
        ROUTES.append(("forward mode %d %s %s" % (mode, tag, shape),
                       lambda: capi.simcross_forward(mode, q, a, top, norm0=n0, norm1=n1)))
        for bm in bwd_modes:
            sfx = " bwd=%s" % bm if len(bwd_modes) > 1 else ""

            def bwd(bm=bm):
                capi.set_euclid_backward_mode(bm)
                capi.simcross_backward(mode, q, a, top, td, dq, da, norm0=n0, norm1=n1)
                capi.set_euclid_backward_mode("fp32")

            def fused(bm=bm):
                capi.set_euclid_backward_mode(bm)
                capi.simcross_forward_backward(mode, q, a, td, top, dq, da, norm0=n0, norm1=n1)
                capi.set_euclid_backward_mode("fp32")
            ROUTES.append(("backward mode %d %s %s%s" % (mode, tag, shape, sfx), bwd))
            ROUTES.append(("forward_backward mode %d %s %s%s" % (mode, tag, shape, sfx), fused))

    both = ("fp32", "reference")
    # Euclid, W1 = W2 = 1
    three("rows pair32", 1, 33, 1, 1, 300, bwd_modes=both)
    three("rows wave 2/wave", 1, 33, 1, 1, 400)
    three("rows wave 1/wave", 1, 33, 1, 1, 404)
    three("rows wave 1/wave widest", 1, 5, 1, 1, 1024)
    three("rows generic (width)", 1, 9, 1, 1, 1028)
    three("rows generic (D % 4)", 1, 9, 1, 1, 30)
    three("rows generic (alignment)", 1, 9, 1, 1, 300, off=2)
    three("rows beyond the generic kernel's LDS", 1, 2, 1, 1, 16388)
    # cosine, W1 = W2 = 1
    three("rows pair32", 0, 33, 1, 1, 300)
    three("rows vec4", 0, 9, 1, 1, 64)
    three("rows scalar (D % 4)", 0, 9, 1, 1, 30)
    three("rows scalar (alignment)", 0, 9, 1, 1, 64, off=2)
    # word grids
    for mode in (1, 0):
        three("grid tiles, tiled backward", mode, 3, 5, 7, 20, bwd_modes=both if mode == 1 else ("fp32",))
        three("grid image, lane backward (Euclid)", mode, 1024, 8, 8, 50, bwd_modes=both if mode == 1 else ("fp32",))
        three("grid plain backward", mode, 2, 64, 65, 8)

    # fp16 storage
    for dist in ("ordered", "tree"):
        for N, D in ((33, 304), (9, 1024)):
            q, a = rnd(N, 1, D, dtype=torch.float16), rnd(N, 1, D, dtype=torch.float16)
            top, td = torch.empty(N, device=dev), rnd(N)
            n0, n1 = torch.empty(N, device=dev), torch.empty(N, device=dev)
            dq, da = torch.empty_like(q), torch.empty_like(a)

            def with_dist(fn, dist=dist):
                def run():
                    capi.set_f16_distance_mode(dist)
                    fn()
                    capi.set_f16_distance_mode("ordered")
                return run
            tag = "%dx%d distance=%s" % (N, D, dist)
            ROUTES.append(("f16 euclid forward " + tag,
                           with_dist(lambda q=q, a=a, top=top: capi.simcross_euclid_forward_f16(q, a, top))))
            ROUTES.append(("f16 euclid forward_backward " + tag, with_dist(
                lambda q=q, a=a, top=top, td=td, dq=dq, da=da: capi.simcross_euclid_forward_backward_f16(q, a, td, top, dq, da))))
            ROUTES.append(("f16 cosine forward " + tag, with_dist(
                lambda q=q, a=a, top=top, n0=n0, n1=n1: capi.simcross_cosine_forward_f16(q, a, top, n0, n1))))
            ROUTES.append(("f16 cosine forward_backward " + tag, with_dist(
                lambda q=q, a=a, top=top, td=td, dq=dq, da=da, n0=n0, n1=n1:
                capi.simcross_cosine_forward_backward_f16(q, a, td, top, dq, da, n0, n1))))

    # Embed fused into the forward
    for mode in (1, 0):
        for N, W1, W2, D in ((3, 5, 7, 20), (1024, 8, 8, 50)):
            K = 97
            iq = torch.randint(0, K, (N, W1), generator=g).float().to(dev)
            ia = torch.randint(0, K, (N, W2), generator=g).float().to(dev)
            w, top = rnd(K, D), torch.empty(N, 1, W1, W2, device=dev)
            n0, n1 = torch.empty(N * W1, device=dev), torch.empty(N * W2, device=dev)
            ROUTES.append(("embed forward mode %d %dx%dx%dx%d" % (mode, N, W1, W2, D),
                           lambda mode=mode, iq=iq, ia=ia, w=w, top=top, n0=n0, n1=n1:
                           capi.embed_simcross_forward(mode, iq, ia, w, top, n0, n1)))

    # fused (q, a+, a-) steps
    for name, step in (("euclid", capi.triplet_euclid_step), ("cosine", capi.triplet_cosine_step)):
        for tag, N, D, off in (("pair32", 33, 300, 0), ("wave 2/wave", 33, 400, 0), ("wave 1/wave", 33, 404, 0),
                               ("generic (width)", 9, 1028, 0), ("generic (D % 4)", 9, 30, 0),
                               ("gradients off alignment", 33, 300, 2)):
            q, p, m = rnd(N, 1, D), rnd(N, 1, D), rnd(N, 1, D)
            y = torch.ones(N, device=dev)
            sp, sn, loss = torch.empty(N, device=dev), torch.empty(N, device=dev), torch.empty(1, device=dev)
            dq, dp, dm = (rnd(N, 1, D, off=off) for _ in range(3))
            ROUTES.append(("triplet %s step %s %dx%d" % (name, tag, N, D),
                           lambda step=step, q=q, p=p, m=m, y=y, sp=sp, sn=sn, loss=loss, dq=dq, dp=dp, dm=dm:
                           step(q, p, m, y, sp, sn, loss, dq, dp, dm)))
    return torch, capi


def run(build=build_routes):
    """build: fills ROUTES (tools/learned_metric_routes.py passes its own)"""
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from mms_answer_selection_amd import capi
    if args.lib:
        capi.LIB_PATH = os.path.abspath(args.lib)
    torch, _ = build()
    sep = torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    if args.labels:
        open(args.labels, "w").write("".join(label + "\n" for label, _ in ROUTES))
    for label, fn in ROUTES:
        print("== " + label, flush=True)
        sep.add_(1)
        fn()
        torch.cuda.synchronize()
    sep.add_(1)
    torch.cuda.synchronize()
    print("%d calls" % len(ROUTES))


def listing(out_dir, ignore=None, grid3=False):
    """ignore: regex of foreign kernels that neither belong to a call nor end it (the runtime's own fill kernel, which
    a hipMemsetAsync inside a call launches); grid3: workgroups as X x Y x Z (the GEMM kernels' grids), not X alone"""
    labels = open(args.labels).read().splitlines()
    f = glob.glob(out_dir + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    groups, cur = [], None
    for r in rows:                                   # a run of the library's kernels between two foreign ones = a call
        if ignore and re.search(ignore, r["Kernel_Name"]):
            continue
        if re.search(r"\bmms::|_ZN3mms", r["Kernel_Name"]):
            if cur is None:
                cur = []
                groups.append(cur)
            wg = int(r["Workgroup_Size_X"])
            grid = "%d" % (int(r["Grid_Size_X"]) // wg)
            if grid3:
                grid += " x %d x %d" % tuple(int(r["Grid_Size_" + d]) // int(r["Workgroup_Size_" + d]) for d in "YZ")
            cur.append("    %s  grid %s  workgroup %d  lds %s" % (r["Kernel_Name"], grid, wg, r.get("LDS_Block_Size", "?")))
        else:
            cur = None
    if len(groups) != len(labels):
        sys.exit("%s: %d labelled calls but %d groups of launches" % (sys.argv[0], len(labels), len(groups)))
    for label, grp in zip(labels, groups):
        print(label)
        print("\n".join(grp))


if __name__ == "__main__":
    listing(args.listing) if args.listing else run()
