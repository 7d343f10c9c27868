"""Times the Pooling and TanH calls (include/mms_pool.h) against torch's max_pool2d / avg_pool2d (ceil_mode=True) and
tanh in the same process, alternating pass by pass, float and double, forward and backward:

    v4pool0    (N, 32, 36, 36), 4 x 4 stride 4, AVE      network_v4's first pooling; in float also the fused
               mms_bn_pool_tanh_forward_f32 in TEST phase, which reads the same map and does more arithmetic
    v5pool0    (N, 32, 38, 38), 2 x 2 stride 2, MAX      network_v5's first pooling
    over_max   (N, 32, 36, 36), 3 x 3 stride 2, MAX      overlapping windows, the last ones clipped
    over_ave   the same, AVE
    whole      (N, 64, 5, 5), 5 x 5                      pool1 of all three nets: a window that is the whole map, AVE
    tanh       N * 32 * 81 elements                      the TanH behind network_v4's pool0

Protocol (tools/bench_conv.py's): every call of a pass takes the next of a ring of operand sets that together exceed the
256-MB Infinity Cache (at least two sets), so no operand is cache-warm from the call before; a pass is `iters` calls
between two HIP events on one stream; two untimed warm-up passes, then seven timed ones; the table gives the median pass
and the range, in us per call, the fraction of 8 TB/s on the bytes the call must move (every array once), and the ratio
torch / this of the medians.  torch's backward is autograd's on a graph kept from a forward outside the timed region.

    python tools/bench_pool.py [point:N:dtype ...]      default: every point at N = 50 and 1517, f32 and f64

One point per invocation gives each a fresh process, and lets a job script put each under a time limit.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from bench_conv import measure
from mms_answer_selection_amd import capi, pool

RING_BYTES = 320 << 20
PEAK = 8e12
# C, H, W, kernel, stride, method
POINTS = {"v4pool0": (32, 36, 36, 4, 4, "ave"), "v5pool0": (32, 38, 38, 2, 2, "max"), "over_max": (32, 36, 36, 3, 2, "max"),
          "over_ave": (32, 36, 36, 3, 2, "ave"), "whole": (64, 5, 5, 5, 1, "ave")}
BATCHES = (50, 1517)
DTYPES = {"f32": torch.float32, "f64": torch.float64}


def report(res, nbytes, base="this"):
    for key, v in res.items():
        if isinstance(v, str):
            print("  %-14s not measured (%s)" % (key, v))
            continue
        extra = ""
        if key in nbytes:
            extra = "  %5.1f %% of 8 TB/s on %.2f MB" % (100 * nbytes[key] / (v[0] * 1e-6) / PEAK, nbytes[key] / 1e6)
        twin = key.replace("torch", base)
        if key.startswith("torch") and not isinstance(res.get(twin), str):
            extra += "  torch / this = %.2f" % (v[0] / res[twin][0])
        if key == "fused bn_pool_tanh":
            t = res["this fwd"]
            slack = (t[2] - t[1]) + (v[2] - v[1])
            extra += "  this fwd - fused = %+.1f us, the two ranges together %.1f us: %s" % (
                t[0] - v[0], slack, "not slower" if t[0] - v[0] <= slack else "SLOWER")
        print("  %-14s median %9.1f us  range %9.1f .. %9.1f%s" % (key, v[0], v[1], v[2], extra))


def bench_pool(name, N, dname):
    C, H, W, k, st, method = POINTS[name]
    dtype, size = DTYPES[dname], 4 if dname == "f32" else 8
    PH, PW = pool.pool_output_dims((N, C, H, W), method, k, st)
    nb, nt = N * C * H * W, N * C * PH * PW
    is_max = method == "max"
    per_set = size * (2 * nb + 3 * nt) + 4 * nt
    nsets = max(2, -(-RING_BYTES // per_set))
    g = torch.Generator(device="cuda").manual_seed(1701)
    rnd = lambda *s: torch.randn(*s, device="cuda", dtype=dtype, generator=g)
    new = lambda *s, dt=dtype: torch.empty(*s, device="cuda", dtype=dt)
    sets = []
    for _ in range(nsets):
        d = dict(x=rnd(N, C, H, W).requires_grad_(True), dy=rnd(N, C, PH, PW), top=new(N, C, PH, PW), dx=new(N, C, H, W),
                 mask=new(N, C, PH, PW, dt=torch.int32) if is_max else None, sp=new(N, C, PH, PW))
        d["ty"] = (F.max_pool2d(d["x"], k, st, 0, ceil_mode=True) if is_max else
                   F.avg_pool2d(d["x"], k, st, 0, ceil_mode=True, count_include_pad=True))
        d["xd"] = d["x"].detach()
        sets.append(d)
    s = lambda i: sets[i % nsets]
    fns = {
        "this fwd": lambda i: pool.pool_forward(s(i)["xd"], method, k, st, mask=s(i)["mask"], out=s(i)["top"]),
        "this bwd": lambda i: pool.pool_backward(s(i)["dy"], (N, C, H, W), method, k, st, mask=s(i)["mask"], out=s(i)["dx"]),
    }

    def torch_fwd(i):
        with torch.no_grad():
            if is_max:
                F.max_pool2d(s(i)["xd"], k, st, 0, ceil_mode=True, return_indices=True)
            else:
                F.avg_pool2d(s(i)["xd"], k, st, 0, ceil_mode=True, count_include_pad=True)

    fns["torch fwd"] = torch_fwd
    fns["torch bwd"] = lambda i: torch.autograd.grad(s(i)["ty"], s(i)["x"], s(i)["dy"], retain_graph=True)
    if name == "v4pool0" and dname == "f32":
        scale, shift, rm, rv = rnd(C).abs() + 0.5, rnd(C), rnd(C) * 0.1, rnd(C).abs() + 0.5
        sm, ss, ws = new(C), new(C), capi.Workspace()
        fns["fused bn_pool_tanh"] = lambda i: capi.bn_pool_tanh_forward(s(i)["xd"], (k, k), scale, shift, rm, rv, s(i)["top"],
                                                                        s(i)["sp"], sm, ss, phase=1, ws=ws)
    for i in range(nsets):                 # the backward reads a forward's mask, in every set
        fns["this fwd"](i)
    iters = 50 if N <= 100 else 10
    print("%s %s N=%d: (%d,%d,%d,%d) %s %dx%d stride %d -> %dx%d, %d operand sets of %.2f MB, %d calls per pass"
          % (name, dname, N, N, C, H, W, method.upper(), k, k, st, PH, PW, nsets, per_set / 1e6, iters))
    moved_f = size * (nb + nt) + (4 * nt if is_max else 0)
    moved_b = size * (nb + nt) + (4 * nt if is_max else 0)
    report(measure(fns, iters), {"this fwd": moved_f, "this bwd": moved_b, "fused bn_pool_tanh": size * (nb + 2 * nt)})
    del sets
    torch.cuda.empty_cache()


def bench_tanh(N, dname):
    dtype, size = DTYPES[dname], 4 if dname == "f32" else 8
    n = N * 32 * 81
    nsets = max(2, -(-RING_BYTES // (4 * n * size)))
    g = torch.Generator(device="cuda").manual_seed(1701)
    sets = []
    for _ in range(nsets):
        x = torch.randn(n, device="cuda", dtype=dtype, generator=g).requires_grad_(True)
        ty = torch.tanh(x)
        sets.append(dict(x=x, xd=x.detach(), ty=ty, y=ty.detach().clone(), dy=torch.randn(n, device="cuda", dtype=dtype, generator=g),
                         out=torch.empty(n, device="cuda", dtype=dtype)))
    s = lambda i: sets[i % nsets]

    def torch_fwd(i):
        with torch.no_grad():
            torch.tanh(s(i)["xd"], out=s(i)["out"])

    fns = {"this fwd": lambda i: pool.tanh_forward(s(i)["xd"], out=s(i)["out"]),
           "this bwd": lambda i: pool.tanh_backward(s(i)["y"], s(i)["dy"], out=s(i)["out"]),
           "torch fwd": torch_fwd,
           "torch bwd": lambda i: torch.autograd.grad(s(i)["ty"], s(i)["x"], s(i)["dy"], retain_graph=True)}
    iters = 50 if N <= 100 else 10
    print("tanh %s N=%d: %d elements, %d operand sets, %d calls per pass" % (dname, N, n, nsets, iters))
    report(measure(fns, iters), {"this fwd": 2 * n * size, "this bwd": 3 * n * size})


if __name__ == "__main__":
    steps = sys.argv[1:] or ["%s:%d:%s" % (p, N, d) for p in list(POINTS) + ["tanh"] for N in BATCHES for d in DTYPES]
    print("device: %s; torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    pool.lib()
    for step in steps:
        name, n, d = step.split(":")
        if name == "tanh":
            bench_tanh(int(n), d)
        else:
            bench_pool(name, int(n), d)
