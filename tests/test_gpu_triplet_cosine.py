"""GPU: the fused cosine (q, a+, a-) step, mms_triplet_cosine_step_f32 (include/mms.h), against

  * the CPU oracle's chain -- two SimCross layers with dist_mode 0 sharing q (sim_cross_layer.cpp:112-139, 226-250),
    PairRankLoss (pair_rank_loss_layer.cpp:26-84), Split sum of dq -- at the project's 1e-5 (the reference's dot
    products are cblas_sdot: no defined order), and
  * the unfused calls on the device (mms_simcross_forward_f32 x2, mms_pairrank_forward_f32 / _backward_f32,
    mms_simcross_backward_f32 x2, mms_split_backward_f32) BIT FOR BIT: scores, norms and gradients.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from util import TOL, assert_bitexact, assert_close, qa, rng

pytestmark = pytest.mark.gpu

SHAPES = [(8, 300), (4096, 300), (4091, 300), (1, 300), (77, 301), (5, 4), (19, 1024), (7, 400), (33, 200), (9, 100),
          (1000, 100), (13, 50), (2050, 304)]
MARGIN, LW = 0.9, 1.0
KINK = 4e-5     # twice the two scores' combined 1e-5 allowance


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def nan_like(shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def inputs(N, D):
    r = rng(3 * N + D)
    q, ap = qa(r, N, 1, 1, D)
    _, an = qa(r, N, 1, 1, D)
    ap = (q + 0.5 * ap).astype(np.float32)           # positive cosine near 0.89, negative near 0
    y = (r.uniform(size=(N, 1)) < 0.8).astype(np.float32)
    return q, ap, an, y


def outputs(N, D):
    shape = (N, 1, D)
    return dict(s_pos=nan_like((N, 1)), s_neg=nan_like((N, 1)), loss=nan_like((1,)), dq=nan_like(shape),
                da_pos=nan_like(shape), da_neg=nan_like(shape)), tuple(nan_like((N,)) for _ in range(3))


def fused(capi, q, ap, an, y, out, norms, finish="inlaunch", margin=MARGIN, ws=None):
    capi.set_triplet_finish_mode(finish)
    try:
        capi.triplet_cosine_step(q, ap, an, y, margin=margin, loss_weight=LW, norms=norms, ws=ws, **out)
    finally:
        capi.set_triplet_finish_mode("inlaunch")


def unfused(capi, q, ap, an, y, mk=nan_like, margin=MARGIN):
    """The seven-launch chain on the device; `mk(shape)` allocates every output and temporary."""
    N, _, D = q.shape
    r = {}
    for br, a in (("pos", ap), ("neg", an)):
        r["s_" + br], r["n0_" + br], r["n1_" + br] = mk((N, 1, 1, 1)), mk((N, 1)), mk((N, 1))
        capi.simcross_forward(0, q, a, r["s_" + br], norm0=r["n0_" + br], norm1=r["n1_" + br])
    o, s, r["loss"] = mk((N, 1)), mk((N, 1)), nan_like((1,))
    capi.pairrank_forward(r["s_pos"].view(N, 1), r["s_neg"].view(N, 1), y, o, s, r["loss"], margin=margin)
    gp, gn = mk((N, 1)), mk((N, 1))
    capi.pairrank_backward(y, o, s, gp, gn, top_diff=LW)
    tmp = {}
    for br, a, g in (("pos", ap, gp), ("neg", an, gn)):
        tmp[br], r["da_" + br] = mk((N, 1, D)), mk((N, 1, D))
        capi.simcross_backward(0, q, a, r["s_" + br], g.view(N, 1, 1, 1), tmp[br], r["da_" + br],
                               norm0=r["n0_" + br], norm1=r["n1_" + br])
    r["dq"] = mk((N, 1, D))
    arr = (C.c_void_p * 2)(tmp["pos"].data_ptr(), tmp["neg"].data_ptr())          # Split: pos + neg, in that order
    capi.check(capi.lib().mms_split_backward_f32(N * D, 2, arr, r["dq"].data_ptr(),
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)), "split")
    torch.cuda.synchronize()
    return r


def assert_same_as_unfused(out, norms, ref, what):
    assert_bitexact(host(out["s_pos"]).ravel(), host(ref["s_pos"]).ravel(), what + " s_pos")
    assert_bitexact(host(out["s_neg"]).ravel(), host(ref["s_neg"]).ravel(), what + " s_neg")
    assert_bitexact(host(norms[0]).ravel(), host(ref["n0_pos"]).ravel(), what + " norm_q (pos layer's norm0)")
    assert_bitexact(host(norms[0]).ravel(), host(ref["n0_neg"]).ravel(), what + " norm_q (neg layer's norm0)")
    assert_bitexact(host(norms[1]).ravel(), host(ref["n1_pos"]).ravel(), what + " norm_pos")
    assert_bitexact(host(norms[2]).ravel(), host(ref["n1_neg"]).ravel(), what + " norm_neg")
    assert_bitexact(host(out["dq"]), host(ref["dq"]), what + " dq")
    assert_bitexact(host(out["da_pos"]), host(ref["da_pos"]), what + " da_pos")
    assert_bitexact(host(out["da_neg"]), host(ref["da_neg"]), what + " da_neg")


# --------------------------------------------------------------------------- #
# 1. parity with the oracle
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("cfg", SHAPES)
@pytest.mark.parametrize("finish", ["inlaunch", "launch"])
def test_triplet_cosine_step_against_the_oracle(cfg, finish, oracle, hiplib):
    from mms_answer_selection_amd import capi
    N, D = cfg
    q, ap, an, y = inputs(N, D)
    sp, nq, npos = oracle.simcross_forward(0, q, ap)
    sn, _, nneg = oracle.simcross_forward(0, q, an)
    loss_ref, o, s = oracle.pairrank_forward(sp.reshape(N, 1), sn.reshape(N, 1), y, MARGIN)
    gsp, gsn = oracle.pairrank_backward(y, o, s, top_diff=LW)

    out, norms = outputs(N, D)
    fused(capi, dev(q), dev(ap), dev(an), dev(y), out, norms, finish)
    g = {k: host(v) for k, v in out.items()}
    assert_close(g["s_pos"].ravel(), sp.ravel(), TOL, "s_pos")
    assert_close(g["s_neg"].ravel(), sn.ravel(), TOL, "s_neg")
    assert_close(host(norms[0]).ravel(), nq.ravel(), TOL, "norm_q")
    assert_close(host(norms[1]).ravel(), npos.ravel(), TOL, "norm_pos")
    assert_close(host(norms[2]).ravel(), nneg.ravel(), TOL, "norm_neg")
    assert_close(g["loss"][0], loss_ref, TOL, "loss")

    # gradients: the oracle chain evaluated at the GPU's own scores (test_triplet_simmatrix_step's rule)
    loss2, o2, s2 = oracle.pairrank_forward(g["s_pos"], g["s_neg"], y, MARGIN)
    g2p, g2n = oracle.pairrank_backward(y, o2, s2, top_diff=LW)
    assert_close(g["loss"][0], loss2, TOL, "loss at the GPU's scores")
    dq_p, dap2, _, _ = oracle.simcross_backward(0, q, ap, g["s_pos"].reshape(sp.shape), g2p.reshape(sp.shape),
                                                norm0=nq, norm1=npos)
    dq_n, dan2, _, _ = oracle.simcross_backward(0, q, an, g["s_neg"].reshape(sn.shape), g2n.reshape(sn.shape),
                                                norm0=nq, norm1=nneg)
    assert_close(g["da_pos"], dap2, TOL, "da_pos")
    assert_close(g["da_neg"], dan2, TOL, "da_neg")
    assert_close(g["dq"], dq_p + dq_n, TOL, "dq")

    # hinge decisions: a row may decide differently from the oracle's scores only within KINK of the kink
    flipped = ((g2p != gsp) | (g2n != gsn)).ravel()
    near = (np.abs(o.astype(np.float64)) <= KINK).ravel()
    print("N=%d D=%d %s: rows near the kink %d, rows that decide differently %d, active hinges %.0f%%"
          % (N, D, finish, int(near.sum()), int(flipped.sum()), 100.0 * float((o > 0).mean())))
    assert not (flipped & ~near).any(), "%d rows away from the kink decide the hinge differently" % int((flipped & ~near).sum())
    assert int(near.sum()) <= max(2, N // 500), "%d rows sit within %g of the kink" % (int(near.sum()), KINK)


# --------------------------------------------------------------------------- #
# 2. bitwise equality with the unfused chain on the device
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("cfg", SHAPES)
def test_triplet_cosine_step_equals_the_unfused_chain_bitwise(cfg, hiplib):
    from mms_answer_selection_amd import capi
    N, D = cfg
    q, ap, an, y = inputs(N, D)
    qd, apd, andv, yd = dev(q), dev(ap), dev(an), dev(y)
    ref = unfused(capi, qd, apd, andv, yd)
    for finish in ("inlaunch", "launch"):
        out, norms = outputs(N, D)
        fused(capi, qd, apd, andv, yd, out, norms, finish)
        assert_same_as_unfused(out, norms, ref, "%s %s" % (cfg, finish))
        assert_close(host(out["loss"])[0], host(ref["loss"])[0], TOL, "loss")


@pytest.mark.parametrize("cfg", [(19, 300), (6, 100), (11, 304), (9, 52)])
def test_triplet_cosine_step_zero_rows_have_the_chains_nan_ness(cfg, hiplib):
    """A zero q row and a zero answer row: the reference's 0/0, NaN exactly where the unfused chain has NaN."""
    from mms_answer_selection_amd import capi
    N, D = cfg
    q, ap, an, y = inputs(N, D)
    q[1] = 0.0
    ap[2] = 0.0
    an[4] = 0.0
    y[1] = y[2] = 1.0
    qd, apd, andv, yd = dev(q), dev(ap), dev(an), dev(y)
    ref = unfused(capi, qd, apd, andv, yd)
    out, norms = outputs(N, D)
    fused(capi, qd, apd, andv, yd, out, norms)
    assert_same_as_unfused(out, norms, ref, "zero rows %s" % (cfg,))
    sp = host(out["s_pos"]).ravel()
    assert np.isnan(sp[1]) and np.isnan(sp[2]) and np.isfinite(sp[0])
    assert np.isnan(host(out["da_pos"])[2]).all() and np.isfinite(host(out["da_pos"])[0]).all()
    assert np.isnan(host(out["loss"])[0]) and np.isnan(host(ref["loss"])[0])


@pytest.mark.parametrize("cfg", [(19, 300, "all"), (19, 300, "out"), (21, 304, "all"), (21, 304, "out"), (37, 301, "all"),
                                 (5, 2048, "none")])
def test_triplet_cosine_step_unaligned_views(cfg, hiplib):
    """Arrays that are not 16-byte aligned: the unfused calls fall to their scalar kernels (another sum order when
    the inputs are unaligned, the written-out backward when only the gradients are) and the step follows them."""
    from mms_answer_selection_amd import capi
    N, D, which = cfg
    q, ap, an, y = inputs(N, D)

    def shifted(shape):
        buf = torch.full((int(np.prod(shape)) + 1,), float("nan"), dtype=torch.float32, device="cuda")
        v = buf[1:].view(shape)
        assert v.data_ptr() % 16 != 0
        return v

    def place(x):
        if which != "all":
            return dev(x)
        v = shifted(x.shape)
        v.copy_(torch.from_numpy(x))
        return v

    qd, apd, andv, yd = place(q), place(ap), place(an), dev(y)
    mk = nan_like if which == "none" else shifted
    ref = unfused(capi, qd, apd, andv, yd, mk=mk)
    out = dict(s_pos=nan_like((N, 1)), s_neg=nan_like((N, 1)), loss=nan_like((1,)), dq=mk((N, 1, D)),
               da_pos=mk((N, 1, D)), da_neg=mk((N, 1, D)))
    norms = tuple(nan_like((N,)) for _ in range(3))
    fused(capi, qd, apd, andv, yd, out, norms)
    assert_same_as_unfused(out, norms, ref, "unaligned %s" % (cfg,))


# --------------------------------------------------------------------------- #
# 3. loss = NULL, the reference-order loss sum, determinism
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("cfg", [(4095, 300), (77, 52), (33, 304)])
def test_triplet_cosine_step_without_the_loss_scalar_or_norms(cfg, hiplib):
    from mms_answer_selection_amd import capi
    N, D = cfg
    q, ap, an, y = (dev(x) for x in inputs(N, D))
    a, na = outputs(N, D)
    fused(capi, q, ap, an, y, a, na)
    b, _ = outputs(N, D)
    b["loss"] = None
    fused(capi, q, ap, an, y, b, None)
    c, nc = outputs(N, D)
    fused(capi, q, ap, an, y, c, (None, nc[1], None))
    for k in a:
        if k != "loss":
            assert_bitexact(host(b[k]), host(a[k]), "loss=None: " + k)
        assert_bitexact(host(c[k]), host(a[k]), "norm_q=norm_neg=None: " + k)
    assert_bitexact(host(nc[1]), host(na[1]), "norm_pos alone")
    assert np.isnan(host(nc[0])).all() and np.isnan(host(nc[2])).all()


@pytest.mark.parametrize("cfg", [(4096, 300), (8193, 100), (77, 301), (1, 300), (130, 304)])
def test_triplet_cosine_step_reference_loss_sum_is_bit_identical(cfg, oracle, hiplib):
    """MMS_LOSS_SUM_REFERENCE: Forward_cpu's running fp32 sum (pair_rank_loss_layer.cpp:41-49) of the terms formed
    from the GPU's own scores, bit for bit."""
    from mms_answer_selection_amd import capi
    N, D = cfg
    q, ap, an, y = inputs(N, D)
    out, norms = outputs(N, D)
    capi.set_loss_sum_mode("reference")
    try:
        fused(capi, dev(q), dev(ap), dev(an), dev(y), out, norms)
    finally:
        capi.set_loss_sum_mode("fast")
    lref, _, _ = oracle.pairrank_forward(host(out["s_pos"]), host(out["s_neg"]), y, MARGIN)
    assert_bitexact(host(out["loss"]), np.array([lref], np.float32), "loss, reference sum")


@pytest.mark.parametrize("cfg", [(4091, 300), (1000, 100), (77, 301), (19, 1024)])
def test_triplet_cosine_step_is_deterministic(cfg, hiplib):
    from mms_answer_selection_amd import capi
    N, D = cfg
    q, ap, an, y = (dev(x) for x in inputs(N, D))
    a, na = outputs(N, D)
    b, nb = outputs(N, D)
    fused(capi, q, ap, an, y, a, na)
    fused(capi, q, ap, an, y, b, nb)
    for k in a:
        assert_bitexact(host(b[k]), host(a[k]), k)
    for u, v in zip(na, nb):
        assert_bitexact(host(u), host(v), "norms")


# --------------------------------------------------------------------------- #
# 4. launch and buffer behaviour
# --------------------------------------------------------------------------- #
def test_triplet_cosine_step_many_launches_and_graph_replay(hiplib):
    """The arrival words are handed back zeroed by every launch: hundreds of launches on one workspace and replays
    of a captured graph all return the first launch's bits."""
    from mms_answer_selection_amd import capi
    N, D = 4096, 300
    q, ap, an, y = (dev(x) for x in inputs(N, D))
    ws = capi.TripletWorkspace()
    two, _ = outputs(N, D)
    fused(capi, q, ap, an, y, two, None, "launch", ws=ws)
    first, nfirst = outputs(N, D)
    fused(capi, q, ap, an, y, first, nfirst, ws=ws)
    torch.cuda.synchronize()
    ref = host(first["loss"]).copy()
    assert np.isfinite(ref).all()
    assert_close(ref[0], host(two["loss"])[0], TOL, "in-launch loss vs two-launch loss")
    assert_bitexact(host(first["dq"]), host(two["dq"]))
    out, nout = outputs(N, D)
    for i in range(400):
        fused(capi, q, ap, an, y, out, nout, ws=ws)
        if i % 100 == 0:
            assert_bitexact(host(out["loss"]), ref, "launch %d" % i)
    assert_bitexact(host(out["loss"]), ref)
    assert_bitexact(host(out["dq"]), host(first["dq"]))
    cap = torch.cuda.Stream()
    cap.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cap):
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph, stream=cap):
            for _ in range(4):
                fused(capi, q, ap, an, y, out, nout, ws=ws)
    torch.cuda.current_stream().wait_stream(cap)
    for rep in range(5):
        for v in list(out.values()) + list(nout):
            v.fill_(float("nan"))
        gph.replay()
        torch.cuda.synchronize()
        for k in out:
            assert_bitexact(host(out[k]), host(first[k]), "graph replay %d: %s" % (rep, k))
        for u, v in zip(nout, nfirst):
            assert_bitexact(host(u), host(v), "graph replay %d: norms" % rep)


@pytest.mark.parametrize("cfg", [(13, 50), (77, 301), (9, 1100), (1, 7), (8, 50), (4096, 300), (19, 1024), (33, 200),
                                 (9, 100), (1, 300)])
def test_triplet_cosine_step_stays_inside_its_buffers(cfg, hiplib):
    """Every output and the workspace at EXACTLY the ABI's size inside one arena, canary words between and after
    them, across the kernel families (D = 100/200/300, D % 4 == 0 up to 1024, everything else)."""
    from mms_answer_selection_amd import capi
    N, D = cfg
    q, ap, an, y = (dev(x) for x in inputs(N, D))
    want, nwant = outputs(N, D)
    fused(capi, q, ap, an, y, want, nwant)
    wsb = hiplib.mms_triplet_workspace_bytes(N)
    assert wsb % 4 == 0
    sizes = dict(ws=wsb // 4, s_pos=N, s_neg=N, norm_q=N, norm_pos=N, norm_neg=N, loss=1, dq=N * D, da_pos=N * D,
                 da_neg=N * D)
    CAN = 64                                                   # canary floats after every buffer (256 B keeps 16-B alignment)
    total = sum(((n + 3) // 4 * 4) + CAN for n in sizes.values())
    arena = torch.full((total,), -777.25, dtype=torch.float32, device="cuda")
    off, view = 0, {}
    for k, n in sizes.items():
        view[k] = arena[off:off + n]
        off += (n + 3) // 4 * 4 + CAN
    lib = capi.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    capi.check(lib.mms_triplet_workspace_init(view["ws"].data_ptr(), wsb, st), "init")
    p = lambda k: view[k].data_ptr()
    for finish in ("inlaunch", "launch"):
        capi.set_triplet_finish_mode(finish)
        try:
            capi.check(lib.mms_triplet_cosine_step_f32(
                N, D, MARGIN, LW, q.data_ptr(), ap.data_ptr(), an.data_ptr(), y.data_ptr(), p("s_pos"), p("s_neg"),
                p("norm_q"), p("norm_pos"), p("norm_neg"), p("loss"), p("dq"), p("da_pos"), p("da_neg"), p("ws"), wsb,
                st), "step")
        finally:
            capi.set_triplet_finish_mode("inlaunch")
        torch.cuda.synchronize()
        h = arena.cpu().numpy()
        mask = np.ones(total, bool)
        off = 0
        for k, n in sizes.items():
            mask[off:off + n] = False
            off += (n + 3) // 4 * 4 + CAN
        assert (h[mask] == np.float32(-777.25)).all(), "a canary word was overwritten (%s, finish=%s)" % (cfg, finish)
        for k in ("s_pos", "s_neg", "dq", "da_pos", "da_neg"):
            assert_bitexact(host(view[k]).ravel(), host(want[k]).ravel(), k)
        for k, v in zip(("norm_q", "norm_pos", "norm_neg"), nwant):
            assert_bitexact(host(view[k]), host(v), k)
        assert_close(host(view["loss"])[0], host(want["loss"])[0], TOL, "loss")
        words = view["ws"][:1056 * 2].view(torch.int32)
        assert int(words.abs().max().item()) == 0, "arrival words not reset"
        for k in ("s_pos", "s_neg", "norm_q", "norm_pos", "norm_neg", "loss", "dq", "da_pos", "da_neg"):
            view[k].fill_(-777.25)


def test_triplet_cosine_step_argument_checks(hiplib):
    from mms_answer_selection_amd import capi
    N, D = 64, 300
    q, ap, an, y = (dev(x) for x in inputs(N, D))
    out, norms = outputs(N, D)
    lib = capi.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    wsb = hiplib.mms_triplet_workspace_bytes(N)
    ws = torch.zeros(wsb, dtype=torch.uint8, device="cuda")
    args = lambda n, w, nbytes, qp=q.data_ptr(): (
        n, D, MARGIN, LW, qp, ap.data_ptr(), an.data_ptr(), y.data_ptr(), out["s_pos"].data_ptr(),
        out["s_neg"].data_ptr(), None, None, None, out["loss"].data_ptr(), out["dq"].data_ptr(),
        out["da_pos"].data_ptr(), out["da_neg"].data_ptr(), w, nbytes, st)
    assert lib.mms_triplet_cosine_step_f32(*args(N, ws.data_ptr(), wsb - 4)) == 3      # MMS_ERR_WORKSPACE: too small
    assert lib.mms_triplet_cosine_step_f32(*args(N, None, wsb)) == 3
    assert lib.mms_triplet_cosine_step_f32(*args(N, ws.data_ptr() + 4, wsb)) == 3      # not 8-byte aligned
    assert lib.mms_triplet_cosine_step_f32(*args(N, ws.data_ptr(), wsb, None)) == 1    # MMS_ERR_INVALID_ARG: q == NULL
    assert lib.mms_triplet_cosine_step_f32(*args(-1, ws.data_ptr(), wsb)) == 1
    assert lib.mms_triplet_cosine_step_f32(*args(0, None, 0)) == 0                     # N == 0: a no-op
    torch.cuda.synchronize()
    for v in out.values():
        assert np.isnan(host(v)).all(), "a refused or empty call wrote something"
    assert lib.mms_triplet_cosine_step_f32(*args(N, ws.data_ptr(), wsb)) == 0
    torch.cuda.synchronize()
    assert np.isfinite(host(out["loss"])).all() and np.isfinite(host(out["dq"])).all()
    with pytest.raises(TypeError):
        capi.triplet_cosine_step(q, ap, an, y, ws=capi.Workspace(), **out)
