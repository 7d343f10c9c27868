"""Times the InnerProduct, Softmax and SoftmaxWithLoss calls (include/mms_fc.h) against torch.nn.functional.linear /
softmax / cross_entropy and their autograd backward in the same process, alternating pass by pass, float and double, and
the per-layer chain Concat -> InnerProduct -> TanH -> Dropout -> InnerProduct -> SoftmaxWithLoss against the fused
mms_head_forward_f32 / mms_head_backward_f32:

    v4fc1      K = 66 (F0 + F1 = 64 + 2, tools/bench_head.py's), N_out = 32      network_v4's fc1
    v4fc2      K = 32, N_out = 2                                                   network_v4's fc2
    simfc1     K = 100 + 100 + 1 + 2 = 203, N_out = 64                            the SimMatrix net's fc1
    softmax    (M, 2, 1)                 loss: the same with labels
    concat     the SimMatrix net's four bottoms (100, 100, 1, 2) against torch.cat and the split's four copies
    chain      network_v4's head, float: six forward and six backward calls against one each

Protocol (tools/bench_conv.py's measure): a pass is `iters` calls between two HIP events on one stream; two untimed
warm-up passes, then seven timed ones; the candidates take turns pass by pass; the table gives the median pass and the
range in us per call.  The operands are a few KB to a MB: a ring of 16 operand sets keeps a call from re-reading the
lines its predecessor wrote, but every set is cache-resident, as it is in a net, where the layer before has just written
it.  These are launch-bound calls: the figures compare launch counts and latencies, not bandwidth.  "this" is the
route mms_inner_product_route picks for the pass (printed), "generic" the *_generic_f32 calls -- the same kernels where
the pick is generic, so the fast route is timed only at the shapes routed to it; torch's backward is autograd's on a graph kept
from a forward outside the timed region and, like this backward, gives all three gradients.

    python tools/bench_fc.py [point:M:dtype ...]      default: every point at M = 50 and 1517, f32 and f64
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from bench_conv import measure
from mms_answer_selection_amd import capi, dropout, fc, head, pool

F0, F1, H, C = 64, 2, 32, 2                                        # tools/bench_head.py's
IP_POINTS = {"v4fc1": (F0 + F1, H), "v4fc2": (H, C), "simfc1": (100 + 100 + 1 + F1, 64)}
BATCHES = (50, 1517)
DTYPES = {"f32": torch.float32, "f64": torch.float64}
NSETS = 16
ROUTES = {fc.ROUTE_FAST: "fast", fc.ROUTE_GENERIC: "generic"}


def report(res):
    for key, v in res.items():
        if isinstance(v, str):
            print("  %-14s not measured (%s)" % (key, v))
            continue
        extra = ""
        for other in ("torch", "generic", "head"):
            twin = key.replace("this", other)
            if key.startswith("this") and twin in res and not isinstance(res[twin], str):
                extra += "  %s / this = %.2f" % (other, res[twin][0] / v[0])
        print("  %-14s median %8.1f us  range %8.1f .. %8.1f%s" % (key, v[0], v[1], v[2], extra))


def rnd_maker(dtype):
    g = torch.Generator(device="cuda").manual_seed(1701)
    return lambda *s: torch.randn(*s, device="cuda", dtype=dtype, generator=g)


def bench_ip(name, M, dname):
    K, N = IP_POINTS[name]
    dtype = DTYPES[dname]
    rnd = rnd_maker(dtype)
    w, b = (rnd(N, K) * (3.0 / K) ** 0.5).requires_grad_(True), (rnd(N) * 0.2).requires_grad_(True)
    wd, bd = w.detach(), b.detach()
    dw, db, ws = torch.zeros_like(wd), torch.zeros_like(bd), capi.Workspace()
    sets = []
    for _ in range(NSETS):
        x = rnd(M, K).requires_grad_(True)
        sets.append(dict(x=x, xd=x.detach(), ty=F.linear(x, w, b), top=torch.empty(M, N, device="cuda", dtype=dtype),
                         dy=rnd(M, N), dx=torch.empty(M, K, device="cuda", dtype=dtype)))
    s = lambda i: sets[i % NSETS]

    def torch_fwd(i):
        with torch.no_grad():
            F.linear(s(i)["xd"], wd, bd)

    fns = {"this fwd": lambda i: fc.inner_product_forward(s(i)["xd"], wd, bd, out=s(i)["top"]),
           "this bwd": lambda i: fc.inner_product_backward(s(i)["xd"], wd, s(i)["dy"], dw, db, s(i)["dx"], ws=ws),
           "torch fwd": torch_fwd,
           "torch bwd": lambda i: torch.autograd.grad(s(i)["ty"], (s(i)["x"], w, b), s(i)["dy"], retain_graph=True)}
    if dname == "f32":
        fns["generic fwd"] = lambda i: fc.inner_product_forward(s(i)["xd"], wd, bd, out=s(i)["top"], route="generic")
        fns["generic bwd"] = lambda i: fc.inner_product_backward(s(i)["xd"], wd, s(i)["dy"], dw, db, s(i)["dx"], ws=ws,
                                                                 route="generic")
    shape = fc.inner_product_shape(M, K, N)
    route = "generic" if dname == "f64" else "fwd %s, bwd %s" % tuple(ROUTES[fc.inner_product_route(shape, p)]
                                                                   for p in (fc.PASS_FORWARD, fc.PASS_BACKWARD))
    iters = 200 if M <= 100 else 100
    print("%s %s M=%d: K=%d N_out=%d, route %s, %d calls per pass" % (name, dname, M, K, N, route, iters))
    report(measure(fns, iters))


def bench_softmax(M, dname):
    dtype = DTYPES[dname]
    rnd = rnd_maker(dtype)
    sets = []
    for _ in range(NSETS):
        x = rnd(M, C).requires_grad_(True)
        label = torch.randint(0, C, (M,), device="cuda")
        sets.append(dict(x=x, xd=x.detach(), ty=F.softmax(x, dim=1), tl=F.cross_entropy(x, label), label=label,
                         labelf=label.to(dtype), dy=rnd(M, C), out=torch.empty(M, C, device="cuda", dtype=dtype),
                         prob=torch.empty(M, C, device="cuda", dtype=dtype), loss=torch.empty(1, device="cuda", dtype=dtype)))
    for d in sets:
        d["top"] = d["ty"].detach().clone()
    s, ws = (lambda i: sets[i % NSETS]), capi.Workspace()

    def torch_fwd(i):
        with torch.no_grad():
            F.softmax(s(i)["xd"], dim=1)

    def torch_loss_fwd(i):
        with torch.no_grad():
            F.cross_entropy(s(i)["xd"], s(i)["label"])

    iters = 200 if M <= 100 else 100
    print("softmax %s M=%d: (%d, %d, 1), %d calls per pass" % (dname, M, M, C, iters))
    report(measure({"this fwd": lambda i: fc.softmax_forward(s(i)["xd"], out=s(i)["out"]),
                    "this bwd": lambda i: fc.softmax_backward(s(i)["top"], s(i)["dy"], out=s(i)["out"]),
                    "torch fwd": torch_fwd,
                    "torch bwd": lambda i: torch.autograd.grad(s(i)["ty"], s(i)["x"], s(i)["dy"], retain_graph=True)}, iters))
    print("loss %s M=%d: (%d, %d, 1), VALID, %d calls per pass" % (dname, M, M, C, iters))
    report(measure({"this fwd": lambda i: fc.softmax_loss_forward(s(i)["xd"], s(i)["labelf"], s(i)["prob"], s(i)["loss"], ws=ws),
                    "this bwd": lambda i: fc.softmax_loss_backward(s(i)["top"], s(i)["labelf"], 1.0, out=s(i)["out"], ws=ws),
                    "torch fwd": torch_loss_fwd,
                    "torch bwd": lambda i: torch.autograd.grad(s(i)["tl"], s(i)["x"], retain_graph=True)}, iters))


def bench_concat(M, dname):
    dtype, ext = DTYPES[dname], (100, 100, 1, F1)
    rnd = rnd_maker(dtype)
    sets = [dict(b=[rnd(M, e) for e in ext], top=torch.empty(M, sum(ext), device="cuda", dtype=dtype),
                 d=[torch.empty(M, e, device="cuda", dtype=dtype) for e in ext]) for _ in range(NSETS)]
    s = lambda i: sets[i % NSETS]
    shapes = [(M, e) for e in ext]

    def torch_bwd(i):
        for dst, src in zip(s(i)["d"], torch.split(s(i)["top"], list(ext), dim=1)):
            dst.copy_(src)

    iters = 200 if M <= 100 else 100
    print("concat %s M=%d: bottoms %s, %d calls per pass" % (dname, M, ext, iters))
    report(measure({"this fwd": lambda i: fc.concat_forward(s(i)["b"], out=s(i)["top"]),
                    "this bwd": lambda i: fc.concat_backward(s(i)["top"], shapes, s(i)["d"]),
                    "torch fwd": lambda i: torch.cat(s(i)["b"], dim=1, out=s(i)["top"]),
                    "torch bwd": torch_bwd}, iters))


def bench_chain(M):
    """float, TRAIN phase: the chain's dropout regenerates its mask, the head reads the one mms_dropout_mask_u32 wrote"""
    dtype, ratio, seed, seq = torch.float32, 0.5, 1234, 7
    rnd = rnd_maker(dtype)
    new = lambda *s: torch.empty(*s, device="cuda", dtype=dtype)
    w1, b1 = rnd(H, F0 + F1) * (3.0 / (F0 + F1)) ** 0.5, rnd(H) * 0.2
    w2, b2 = rnd(C, H) * (6.0 / H) ** 0.5, rnd(C) * 0.2
    dw1, db1, dw2, db2 = (torch.zeros_like(t) for t in (w1, b1, w2, b2))
    mask = dropout.dropout_mask((M, H), ratio, seed, seq)
    sets = [dict(x0=rnd(M, F0), x1=rnd(M, F1).abs(), label=torch.randint(0, C, (M,), device="cuda").to(dtype), feat=new(M, F0 + F1),
                 h=new(M, H), d=new(M, H), z2=new(M, C), prob=new(M, C), loss=new(1), dz2=new(M, C), dd=new(M, H),
                 dfeat=new(M, F0 + F1), dx0=new(M, F0), dx1=new(M, F1)) for _ in range(NSETS)]
    s, ws, hws = (lambda i: sets[i % NSETS]), capi.Workspace(), capi.Workspace()

    def chain_fwd(i):
        t = s(i)
        fc.concat_forward([t["x0"], t["x1"]], out=t["feat"])
        fc.inner_product_forward(t["feat"], w1, b1, out=t["h"])
        pool.tanh_forward(t["h"], out=t["h"])
        dropout.dropout_forward(t["h"], ratio, seed, seq, out=t["d"])
        fc.inner_product_forward(t["d"], w2, b2, out=t["z2"])
        fc.softmax_loss_forward(t["z2"], t["label"], t["prob"], t["loss"], ws=ws)

    def chain_bwd(i):
        t = s(i)
        fc.softmax_loss_backward(t["prob"], t["label"], 1.0, out=t["dz2"], ws=ws)
        fc.inner_product_backward(t["d"], w2, t["dz2"], dw2, db2, t["dd"], ws=ws)
        dropout.dropout_backward(t["dd"], ratio, seed, seq, out=t["dd"])
        pool.tanh_backward(t["h"], t["dd"], out=t["dd"])
        fc.inner_product_backward(t["feat"], w1, t["dd"], dw1, db1, t["dfeat"], ws=ws)
        fc.concat_backward(t["dfeat"], [(M, F0), (M, F1)], [t["dx0"], t["dx1"]])

    def head_fwd(i):
        t = s(i)
        head.head_forward(t["x0"], t["x1"], w1, b1, mask, w2, b2, t["label"], t["h"], t["prob"], t["loss"], ws=hws)

    def head_bwd(i):
        t = s(i)
        head.head_backward(t["x0"], t["x1"], w1, w2, mask, t["h"], t["prob"], t["label"], 1.0, t["dx0"], t["dx1"], dw1, db1,
                           dw2, db2, ws=hws)

    for i in range(NSETS):
        chain_fwd(i)
    iters = 100
    print("chain f32 M=%d: network_v4's head, TRAIN, six calls a pass against one, %d passes' calls per pass" % (M, iters))
    report(measure({"this fwd": chain_fwd, "this bwd": chain_bwd, "head fwd": head_fwd, "head bwd": head_bwd}, iters))


if __name__ == "__main__":
    steps = sys.argv[1:] or (["%s:%d:%s" % (p, M, d) for p in list(IP_POINTS) + ["softmax", "concat"] for M in BATCHES for d in DTYPES]
                             + ["chain:%d:f32" % M for M in BATCHES])
    print("device: %s; torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    fc.lib()
    for step in steps:
        name, m, d = step.split(":")
        if name == "softmax":
            bench_softmax(int(m), d)
        elif name == "concat":
            bench_concat(int(m), d)
        elif name == "chain":
            bench_chain(int(m))
        else:
            bench_ip(name, int(m), d)
