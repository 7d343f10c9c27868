"""SimMatrix backward under every subset of its three propagate flags, and the layer-by-layer fallback of the fused
learned-metric triplet step.

The parity suites hold each route of mms_simmatrix_backward(_cached)_f32 to the oracle with all flags on (and one
partial combination).  Which launches a call makes depends on the flags -- the dW reduction's launch builds the dq
product's weight operand only when dq follows, da rides in the dq launch only when both are asked for -- so every
subset is pinned here: an output whose flag is off is not touched, and one whose flag is on carries the bits of the
all-flags-on call.
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from util import assert_bitexact, rng

pytestmark = pytest.mark.gpu

# each the smallest shape that reaches its route
SHAPES = [
    (130, 33, 18),     # gemm32 everywhere; K2 % 4 != 0: cached da takes the scalar row-scale
    (700, 64, 48),     # every multiple-of-4 test of the panel kernel holds, its size test (96 workgroups) does not: gemm32,
                       # with the vector row-scale for cached da
    (2048, 24, 8),     # the bf16 pipe at its row threshold, with the side job's 8-column minimum (fp32 mode: gemm32)
    (2049, 33, 18),    # above the threshold with K2 % 4 != 0: no side job; dW on the bf16 pipe (mode 0), dq and da on gemm32
    # The panel kernel takes a product only from 96 workgroups up: 64-row blocks times the split of the pairs.  For dq that
    # is N >= 6081 rows, and for dW (one row block, one slab per 64 pairs) as well, so this is the smallest round size at
    # which fp32 mode reaches the panel's split-K dW, W^T written by its reduction (or by the transpose launch when dW is
    # off) and the panel's da side job.  It is the one shape above 2 049 rows: no smaller one runs that route.
    (6144, 64, 48),
]
FLAGS = list(itertools.product((False, True), repeat=3))      # (param_propagate_down, propagate_down0, propagate_down1)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def nan_like(shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


_cases = {}


def _case(capi, shape, mode, cached):
    """Inputs on the device, the forward's Q.W when cached, and the all-flags-on outputs: made once per
    (shape, mode, cached) and left unchanged."""
    key = (shape, mode, cached)
    if key not in _cases:
        N, K1, K2 = shape
        r = rng(sum(shape) + 3)
        q = dev((r.standard_normal((N, K1)) * 0.4).astype(np.float32))
        a = dev((r.standard_normal((N, K2)) * 0.4).astype(np.float32))
        W = dev(r.uniform(-0.08, 0.08, (K1, K2)).astype(np.float32))
        dT = dev(r.standard_normal((N, 1)).astype(np.float32))
        dW0 = r.standard_normal((K1, K2)).astype(np.float32)
        qw = None
        if cached:
            qw = nan_like((N, K2))
            capi.simmatrix_forward(q, a, W, nan_like((N, 1)), qw)
        gq, ga, gW = nan_like((N, K1)), nan_like((N, K2)), dev(dW0)
        capi.simmatrix_backward(q, a, W, dT, gq, ga, gW, qw=qw)        # the default workspace, all flags on
        full = (host(gW), host(gq), host(ga))
        assert not any(np.isnan(x).any() for x in full), "the all-flags-on call left an output unwritten"
        _cases[key] = (q, a, W, dT, dW0, qw, full)
    return _cases[key]


@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: "".join("1" if x else "0" for x in f))
@pytest.mark.parametrize("cached", [True, False], ids=["cached", "uncached"])
@pytest.mark.parametrize("mode", ["bf16x3", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_backward_flag_subsets(shape, mode, cached, flags, hiplib):
    from mms_answer_selection_amd import capi
    capi.set_matrix_mode(mode)
    try:
        q, a, W, dT, dW0, qw, (fW, fq, fa) = _case(capi, shape, mode, cached)
        ppd, pd0, pd1 = flags
        N, K1, K2 = shape
        gq, ga, gW = nan_like((N, K1)), nan_like((N, K2)), dev(dW0)
        capi.simmatrix_backward(q, a, W, dT, gq, ga, gW, param_propagate_down=ppd, propagate_down=(pd0, pd1), qw=qw)
        what = "%s %s %s flags %s: " % (shape, mode, "cached" if cached else "uncached", flags)
        # every combination is bit-equal to the all-flags-on call: the reductions of dW share one ordered sum, the forms
        # of da one product and one scaling
        assert_bitexact(host(gW), fW if ppd else dW0, what + ("dW" if ppd else "dW untouched"))
        if pd0:
            assert_bitexact(host(gq), fq, what + "dq")
        else:
            assert np.isnan(host(gq)).all(), what + "dq touched"
        if pd1:
            assert_bitexact(host(ga), fa, what + "da")
        else:
            assert np.isnan(host(ga)).all(), what + "da touched"
    finally:
        capi.set_matrix_mode("bf16x3")


def test_triplet_fallback_matches_layers(hiplib):
    """mms_triplet_simmatrix_step_f32 at a shape its fused route refuses (K2 = 18 is no multiple of 4: the panel kernel
    takes none of the three products) against the same seven calls made one by one: every output bit for bit."""
    from mms_answer_selection_amd import capi
    N, K1, K2 = 130, 33, 18
    margin, lw = 0.3, 0.7
    r = rng(N + K1 + 7 * K2)
    q = dev((r.standard_normal((N, K1)) * 0.4).astype(np.float32))
    ap = dev((r.standard_normal((N, K2)) * 0.4).astype(np.float32))
    an = dev((r.standard_normal((N, K2)) * 0.4).astype(np.float32))
    W = dev(r.uniform(-0.08, 0.08, (K1, K2)).astype(np.float32))
    y = dev((r.uniform(size=(N, 1)) < 0.8).astype(np.float32))
    dW0 = r.standard_normal((K1, K2)).astype(np.float32)

    out = dict(s_pos=nan_like((N, 1)), s_neg=nan_like((N, 1)), loss=nan_like((1,)), dq=nan_like((N, K1)),
               da_pos=nan_like((N, K2)), da_neg=nan_like((N, K2)), dW=dev(dW0))
    capi.triplet_simmatrix_step(q, ap, an, y, W, margin=margin, loss_weight=lw, **out)

    ref = dict(s_pos=nan_like((N, 1)), s_neg=nan_like((N, 1)), loss=nan_like((1,)), dq=nan_like((N, K1)),
               da_pos=nan_like((N, K2)), da_neg=nan_like((N, K2)), dW=dev(dW0))
    qwp, qwn = nan_like((N, K2)), nan_like((N, K2))
    capi.simmatrix_forward(q, ap, W, ref["s_pos"], qwp, use_workspace=False)
    capi.simmatrix_forward(q, an, W, ref["s_neg"], qwn, use_workspace=False)
    o, s, gp, gn = (nan_like((N, 1)) for _ in range(4))
    capi.pairrank_forward(ref["s_pos"], ref["s_neg"], y, o, s, ref["loss"], margin=margin)
    capi.pairrank_backward(y, o, s, gp, gn, top_diff=lw)
    dq2 = nan_like((N, K1))
    capi.simmatrix_backward(q, ap, W, gp, ref["dq"], ref["da_pos"], ref["dW"], qw=qwp)
    capi.simmatrix_backward(q, an, W, gn, dq2, ref["da_neg"], ref["dW"], qw=qwn)
    two = (C.c_void_p * 2)(ref["dq"].data_ptr(), dq2.data_ptr())            # Split: pos + neg, in place on pos
    capi.check(capi.lib().mms_split_backward_f32(N * K1, 2, two, ref["dq"].data_ptr(),
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)), "split")
    torch.cuda.synchronize()
    for k in ("s_pos", "s_neg", "loss", "dq", "da_pos", "da_neg", "dW"):
        got = host(out[k])
        assert not np.isnan(got).any(), k + " not written"
        assert_bitexact(got, host(ref[k]), k)
