"""Times the fused BN -> MaxPool -> TanH calls (mms_bn_maxpool_tanh_forward_f32 TRAIN and TEST,
mms_bn_maxpool_tanh_backward_f32) by the protocol of tools/bench_bn_pool.py: HBM-cold rotation over
distinct buffer sets, 200 calls captured in one hipGraph and timed between two events, median of 5 replays, the replays
ALTERNATING (fused, layered, AVE, fused, ...).  Beside each:

  layered   what a host of network_v3 / network_v5 has without the call: mms_bn_forward_f32, then torch's max_pool2d
            (with indices) and an in-place tanh; backward: torch's tanh_backward and max_pool2d_with_indices_backward,
            then mms_bn_backward_f32
  AVE       mms_bn_pool_tanh_* at the same shape: the same sweep with a sum in place of the compare

Prints us per call and, for the fused call, the fraction of 8 TB/s on its COMPULSORY bytes (those of
tools/bench_bn_pool.py: the MAX form stores no mask).

    python tools/bench_bn_maxpool.py [N C H W kh kw ...] > profiles/bn_maxpool_bench.txt
    default: the BN shapes of network_v3 (32 x 36 x 36 with 4 x 4, 64 x 5 x 5 with 5 x 5) and network_v5 (32 x 38 x 38
    and 64 x 16 x 16 with 2 x 2, 64 x 6 x 6 with 6 x 6), each at N = 50 and N = 1517
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench_bn_pool import PEAK, ROTATE_BYTES, timed_alternating
from mms_answer_selection_amd import bn_maxpool, capi

aten = torch.ops.aten


def bench(N, C, H, W, kh, kw, stream):
    n, k = N * C * H * W, (kh, kw)
    pooled = (N, C, H // kh, W // kw)
    p = n // (kh * kw)
    nsets = max(4, -(-ROTATE_BYTES // (2 * 4 * n)))
    dev = dict(device="cuda")
    sets = []
    for _ in range(nsets):
        sets.append(dict(x=torch.randn(N, C, H, W, **dev) * 0.8 + 0.3, dx=torch.empty(N, C, H, W, **dev),
                         bn_top=torch.empty(N, C, H, W, **dev), top=torch.empty(pooled, **dev),
                         save_pool=torch.empty(pooled, **dev), top_diff=torch.randn(pooled, **dev),
                         idx=torch.zeros(pooled, dtype=torch.int64, **dev)))
    scale, shift = torch.rand(C, **dev) + 0.5, torch.randn(C, **dev)
    scale[1::2] *= -1
    rm, rv = torch.zeros(C, **dev), torch.ones(C, **dev)
    mean, std = torch.empty(C, **dev), torch.empty(C, **dev)
    dscale, dshift = torch.empty(C, **dev), torch.empty(C, **dev)
    ws = capi.Workspace()
    s = lambda i: sets[i % nsets]

    def fused_fwd(phase, call=bn_maxpool.bn_maxpool_tanh_forward):
        return lambda i: call(s(i)["x"], k, scale, shift, rm, rv, s(i)["top"], s(i)["save_pool"], mean, std, phase=phase,
                              ws=ws)

    def layered_fwd(phase):
        def f(i):
            capi.bn_forward(s(i)["x"], scale, shift, rm, rv, s(i)["bn_top"], mean, std, phase=phase, ws=ws)
            top, idx = aten.max_pool2d_with_indices(s(i)["bn_top"], list(k), list(k))
            s(i)["top"].copy_(top.tanh_())
            s(i)["idx"].copy_(idx)
        return f

    def fused_bwd(i):
        bn_maxpool.bn_maxpool_tanh_backward(s(i)["x"], k, s(i)["top"], s(i)["top_diff"], s(i)["save_pool"], scale, shift,
                                            mean, std, s(i)["dx"], dscale, dshift, ws=ws)

    def ave_bwd(i):
        capi.bn_pool_tanh_backward(s(i)["x"], k, s(i)["top"], s(i)["top_diff"], s(i)["save_pool"], scale, mean, std,
                                   s(i)["dx"], dscale, dshift, ws=ws)

    def layered_bwd(i):
        g = aten.tanh_backward(s(i)["top_diff"], s(i)["top"])
        dy = aten.max_pool2d_with_indices_backward(g, s(i)["bn_top"], list(k), list(k), [0, 0], [1, 1], False, s(i)["idx"])
        capi.bn_backward(s(i)["x"], dy, scale, mean, std, s(i)["dx"], dscale, dshift, ws=ws)

    torch.cuda.synchronize()
    out = {}
    for title, phase in (("forward TRAIN", 0), ("forward TEST", 1)):
        out[title] = timed_alternating(stream, {"fused": fused_fwd(phase), "layered": layered_fwd(phase),
                                                "AVE": fused_fwd(phase, capi.bn_pool_tanh_forward)})
    with torch.cuda.stream(stream):
        for i in range(nsets):                   # the backward reads batch statistics, every set's own top / save_pool
            layered_fwd(0)(i)                    # ... and, layered, its indices
            fused_fwd(0)(i)
    out["backward"] = timed_alternating(stream, {"fused": fused_bwd, "layered": layered_bwd, "AVE": ave_bwd})
    wsb = bn_maxpool.bn_maxpool_tanh_workspace_bytes(N, C, H, W, kh, kw)
    route = "one launch per pass (one workgroup per channel)" if wsb == 0 else \
        "two launches per pass (TEST forward: one), %d chunks per channel" % (wsb // (C * 16))
    print("BN+maxpool+tanh %d x %d x %d x %d, %d x %d windows, f32, %.2f MB of x, %d buffer sets, %s"
          % (N, C, H, W, kh, kw, 4 * n / 1e6, nsets, route))
    need = {"forward TRAIN": 4 * (n + 2 * p), "forward TEST": 4 * (n + 2 * p), "backward": 4 * (2 * n + 3 * p)}
    for title, t in out.items():
        b = need[title]
        print("  %-14s fused %8.2f us  (%7.2f MB compulsory, %.3f of 8 TB/s)   layered %8.2f us  (x %.2f)   "
              "AVE call %8.2f us  (MAX / AVE %.2f)" % (title, t["fused"], b / 1e6, b / (t["fused"] * 1e-6) / PEAK,
                                                      t["layered"], t["layered"] / t["fused"], t["AVE"],
                                                      t["fused"] / t["AVE"]))
    sys.stdout.flush()


if __name__ == "__main__":
    a = [int(v) for v in sys.argv[1:]]
    v3_v5 = [(32, 36, 36, 4, 4), (64, 5, 5, 5, 5), (32, 38, 38, 2, 2), (64, 16, 16, 2, 2), (64, 6, 6, 6, 6)]
    shapes = [tuple(a[i:i + 6]) for i in range(0, len(a), 6)] or [(N,) + g for N in (50, 1517) for g in v3_v5]
    st = torch.cuda.Stream()
    for shape in shapes:
        bench(*shape, st)
