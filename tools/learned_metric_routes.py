#!/usr/bin/env python3
"""tools/learned_metric_routes.py -- one call per launch sequence of the learned-metric sources (csrc/bilinear.hip,
csrc/simmatrix.hip, over csrc/gemm32.hip), and the listing that pins which launch serves which call.

Driven and listed exactly like tools/elementwise_routes.py, whose command line, run loop and listing it uses:
  run (on the GPU, by itself under the profiler, no counters and no other tracing):
      rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 tools/learned_metric_routes.py --labels LABELS \
          [--lib LIBMMS_HIP.SO]
  listing:
      python3 tools/learned_metric_routes.py --listing OUT --labels LABELS > profiles/learned_metric_routes.txt

Shapes are those of the tests that hold these routes to their bars: the route table of
tests/test_gpu_bilinear_grid_accuracy.py (every row), the shape lists of tests/test_gpu_matrix_pipe_accuracy.py,
tests/test_gpu_simmatrix_flags.py and tests/test_gpu_triplet_simmatrix_fused.py, the Embed-fused cases of
tests/test_gpu_embed.py.  Calls that clear a buffer with hipMemsetAsync (the SimMatrix alias's dW, the fused step's ones) make the runtime launch its fill kernel between the
library's own; the listing leaves it out."""
import elementwise_routes as er          # parses the command line: the two scripts share it

FILL = r"fillBuffer"                     # the HIP runtime's memset kernel

BILINEAR = [                             # (N, W1, W2, D, M, bias_term): tests/test_gpu_bilinear_grid_accuracy.py SHAPES
    (512, 48, 5, 52, 1, 1), (512, 3, 48, 53, 2, 0), (513, 17, 40, 64, 3, 1),
    (1, 40, 40, 52, 1, 1), (2, 40, 3, 50, 1, 0), (8, 41, 7, 52, 2, 1), (9, 5, 40, 53, 1, 0), (32, 48, 48, 64, 1, 1),
    (33, 16, 33, 64, 4, 1), (256, 2, 3, 8, 2, 1),
    (257, 3, 2, 8, 1, 1), (511, 2, 2, 6, 2, 0),
    (3, 49, 4, 52, 1, 1), (2, 4, 49, 52, 2, 1), (5, 7, 6, 65, 2, 1), (3, 5, 4, 66, 1, 1), (40, 9, 5, 68, 1, 0),
    (5, 40, 40, 68, 1, 1), (400, 8, 8, 72, 4, 1), (5600, 8, 8, 68, 1, 0),
    (16385, 2, 1, 68, 4, 1), (256, 2, 2, 4, 256, 1),
    (300, 1, 1, 24, 3, 1),
]
ALIAS = [(2304, 300), (2304, 64), (130, 33)]          # W1 = W2 = M = 1: (N, D); the last one below the bf16 pipe's rows
EMBED = [(1517, 40, 40, 50, 4, 20000, 1), (600, 16, 24, 64, 2, 300, 0), (50, 40, 40, 50, 4, 1000, 1), (7, 9, 13, 33, 3, 40, 1)]
PIPE = [(2049, 300, 300), (2125, 52, 304), (2049, 64, 160), (2048, 24, 8), (2125, 96, 128), (2085, 200, 72)]
FLAGS = [(130, 33, 18), (700, 64, 48), (2048, 24, 8), (2049, 33, 18), (6144, 64, 48)]
HALF = [(2049, 304, 304), (2125, 64, 160), (2048, 24, 8), (2125, 96, 128), (2085, 200, 72)]
# The fused route needs N >= 6081 (96 panels of 64 rows) and N % 4 == 0: (2125, 300, 300), (2049, 64, 160), (130, 33, 18) and
# (6080, 300, 300) run the layers one by one; the others are the shapes of tests/test_gpu_triplet_simmatrix_fused.py
TRIPLET = [(2125, 300, 300), (2049, 64, 160), (6144, 64, 48), (130, 33, 18),
           (6084, 4, 4), (6084, 36, 68), (6084, 112, 64), (6148, 116, 112), (6144, 100, 200), (6084, 208, 212),
           (6084, 300, 300), (6148, 304, 304), (6080, 300, 300)]
MODES = ("bf16x3", "fp32")


def build_routes():
    import torch
    from mms_answer_selection_amd import capi
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(11)
    add = er.ROUTES.append

    def rnd(*shape, dtype=torch.float32):
        return torch.randn(*shape, generator=g).to(dev).to(dtype)

    def in_mode(mode, fn):
        def run():
            capi.set_matrix_mode(mode)
            fn()
            capi.set_matrix_mode("bf16x3")
        return run

    def bilinear(tag, N, W1, W2, D, M, bias_term, mode=None):
        q, a, W = rnd(N, W1, D), rnd(N, W2, D), rnd(M, D, D)
        bias = rnd(M, W1, W2) if bias_term else None
        top, td = torch.empty(N, M, W1, W2, device=dev), rnd(N, M, W1, W2)
        dq, da, dW = torch.empty_like(q), torch.empty_like(a), torch.empty_like(W)
        dbias = torch.zeros(M, W1, W2, device=dev) if bias_term else None
        shape = "%dx%dx%dx%d M=%d bias=%d%s" % (N, W1, W2, D, M, bias_term, " %s" % mode if mode else "")
        wrap = (lambda fn: in_mode(mode, fn)) if mode else (lambda fn: fn)
        add(("bilinear forward %s %s" % (tag, shape), wrap(lambda: capi.simcross_forward(2, q, a, top, W=W, bias=bias))))
        add(("bilinear backward %s %s" % (tag, shape), wrap(lambda: capi.simcross_backward(
            2, q, a, top, td, dq, da, W=W, bias_term=bool(bias_term), dW=dW, dbias=dbias))))

    for s in BILINEAR:
        bilinear("grid", *s)
    for mode in MODES:
        for N, D in ALIAS:
            for bias_term in (0, 1):
                bilinear("as SimMatrix", N, 1, 1, D, 1, bias_term, mode)
    for N, W1, W2, D, M, K, bias_term in EMBED:
        iq = torch.randint(0, K, (N, W1), generator=g).float().to(dev)
        ia = torch.randint(0, K, (N, W2), generator=g).float().to(dev)
        table, W, top = rnd(K, D), rnd(M, D, D), torch.empty(N, M, W1, W2, device=dev)
        bias = rnd(M, W1, W2) if bias_term else None
        add(("bilinear embed forward %dx%dx%dx%d M=%d bias=%d" % (N, W1, W2, D, M, bias_term),
             lambda iq=iq, ia=ia, table=table, W=W, bias=bias, top=top:
             capi.embed_simcross_bilinear_forward(iq, ia, table, W, bias, top)))

    def simmatrix(N, K1, K2):
        q, a, W, td = rnd(N, K1), rnd(N, K2), rnd(K1, K2), rnd(N, 1)
        top, qw = torch.empty(N, 1, device=dev), torch.empty(N, K2, device=dev)
        dq, da, dW = torch.empty_like(q), torch.empty_like(a), torch.zeros_like(W)
        return q, a, W, td, top, qw, dq, da, dW

    for shape in sorted(set(PIPE + FLAGS)):
        q, a, W, td, top, qw, dq, da, dW = simmatrix(*shape)
        tag = "%dx%dx%d" % shape
        add(("simmatrix forward no workspace %s" % tag,
             lambda q=q, a=a, W=W, top=top, qw=qw: capi.simmatrix_forward(q, a, W, top, qw, use_workspace=False)))
        for mode in MODES:
            add(("simmatrix forward %s %s" % (tag, mode),
                 in_mode(mode, lambda q=q, a=a, W=W, top=top, qw=qw: capi.simmatrix_forward(q, a, W, top, qw))))
            # all flags on, with and without the forward's Q.W; then each flag off once (with Q.W, and without for da)
            for cached, ppd, pd0, pd1 in ((1, 1, 1, 1), (0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (0, 0, 1, 1),
                                          (0, 1, 0, 1)):
                add(("simmatrix backward %s %s qw=%d ppd=%d pd0=%d pd1=%d" % (tag, mode, cached, ppd, pd0, pd1),
                     in_mode(mode, lambda q=q, a=a, W=W, td=td, dq=dq, da=da, dW=dW, qw=qw, cached=cached, ppd=ppd, pd0=pd0,
                             pd1=pd1: capi.simmatrix_backward(q, a, W, td, dq, da, dW, param_propagate_down=bool(ppd),
                                                              propagate_down=(bool(pd0), bool(pd1)),
                                                              qw=qw if cached else None))))

    h = torch.float16
    for N, K1, K2 in HALF:
        q, a, W, td = rnd(N, K1, dtype=h), rnd(N, K2, dtype=h), rnd(K1, K2), rnd(N, 1)
        top, qw = torch.empty(N, 1, device=dev), torch.empty(N, K2, device=dev)
        dq, da, dW = torch.empty_like(q), torch.empty_like(a), torch.zeros_like(W)
        tag = "%dx%dx%d" % (N, K1, K2)
        add(("f16 simmatrix forward %s" % tag, lambda q=q, a=a, W=W, top=top: capi.simmatrix_forward_f16(q, a, W, top)))
        add(("f16 simmatrix forward_train %s" % tag,
             lambda q=q, a=a, W=W, top=top, qw=qw: capi.simmatrix_forward_train_f16(q, a, W, top, qw)))
        add(("f16 simmatrix backward %s" % tag, lambda q=q, a=a, W=W, qw=qw, td=td, dq=dq, da=da, dW=dW:
             capi.simmatrix_backward_f16(q, a, W, qw, td, dq, da, dW)))
        add(("f16 simmatrix backward dW only %s" % tag, lambda q=q, a=a, W=W, td=td, dW=dW:
             capi.simmatrix_backward_f16(q, a, W, None, td, None, None, dW)))

    for N, K1, K2 in TRIPLET:
        q, p, m, W = rnd(N, K1), rnd(N, K2), rnd(N, K2), rnd(K1, K2)
        y = torch.ones(N, 1, device=dev)
        sp, sn, loss = torch.empty(N, 1, device=dev), torch.empty(N, 1, device=dev), torch.empty(1, device=dev)
        dq, dp, dm, dW = torch.empty_like(q), torch.empty_like(p), torch.empty_like(m), torch.zeros_like(W)
        for mode in MODES:
            add(("triplet simmatrix step %dx%dx%d %s" % (N, K1, K2, mode),
                 in_mode(mode, lambda q=q, p=p, m=m, y=y, W=W, sp=sp, sn=sn, loss=loss, dq=dq, dp=dp, dm=dm, dW=dW:
                         capi.triplet_simmatrix_step(q, p, m, y, W, sp, sn, loss, dq, dp, dm, dW))))
    return torch, capi


if __name__ == "__main__":
    er.listing(er.args.listing, ignore=FILL, grid3=True) if er.args.listing else er.run(build_routes)
