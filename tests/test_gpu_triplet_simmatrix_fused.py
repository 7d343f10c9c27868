"""The FUSED route of mms_triplet_simmatrix_step_f32 (csrc/simmatrix.hip: tripsim_fused; the `p.Y2` epilogue of
panel_gemm_kernel<NT, true> in csrc/panel_gemm.h), at the shapes that reach it.

tripsim_fused serves a call only if panel_eligible(Q W), panel_eligible(B W^T) and panel_dw_eligible(Q^T B) all hold: 96 or more
panels of 64 rows (N >= 6081) and, because the dW product contracts over the N triplets (pg_mult4(p.K)), N % 4 == 0 -- so N >= 6084.
Everything else runs the layers one by one inside the call.  Until this module the suite ran the fused route at ONE shape,
(8192, 100, 200), on dense data at 1e-5 of the largest output, in the default matrix mode.  Here, in both matrix modes:

  1. exact probes of the whole step -- small-integer inputs for which every intermediate is exact in fp32 in any summation order
     (asserted on the CPU from the fp64 reference: every bound on a partial sum < 2^24 half-units), planted rows on every
     PairRankLoss decision edge, every output compared BIT FOR BIT (apart from the sign of a zero) with numpy's fp64, the loss too;
  2. single-product probes (tests/matrix_pipe_model.py) of dq, dW, Q W and the scores at the bar 2^-20, with the probe values in
     a+, in a-, and in both; the epilogue's row dot within gamma_K2 of the fp64 dot of the kernel's own row of Q W;
  3. dense data -- after redrawing the rows within 1e-4 of a decision edge, ZERO rows may decide differently from the fp64
     scores; s+-, da+-, dq, dW within twice the CPU oracle's own componentwise error; loss at 1e-5; two calls give the same bits.

Route table: (N, K1, K2) -> forward | backward in "bf16x3" mode | backward in "fp32" mode, read off tripsim_fused, panel_eligible,
panel_launch, panel_pick_ksplit, bx3_eligible, bx3_tn_eligible, bx3_tn_pick_chunks and bx3_ntw.  panel<NT, T/F> =
panel_gemm_kernel<NT, A_KC>, NT = 4 / 7 / 13 / 19 for a width <= 64 / <= 112 / <= 208 / <= 304 (forward: K2, dq: K1, dW: K2);
tn(c x p) = bx3_tn_kernel<false> with NO k-scale (only this route passes none), c chunks of p pairs; bx3<NTW> = bx3_kernel;
every forward is followed by loss_finish_kernel, every tn by splitk_reduce_split_kernel, every panel<., F> by
splitk_reduce_transpose_kernel (and preceded by the runtime's fill of the `ones` k-scale).  bx3_eligible and bx3_tn_eligible take
every shape of this list, the 4 x 4 one included: in "bf16x3" mode the backward is always on the bf16 pipe.
profiles/learned_metric_routes.txt records the kernels a trace saw per shape and mode.

  (6084,   4,   4)  panel<4,T>: one partial 32-deep k-tile, no full one; 96 panels, the last of 4 rows
                    | tn(96 x 64, last chunk 4 pairs), bx3<1>  | panel<4,F> ksplit 96 x 64 (1 row block), panel<4,T>
  (6144,  64,  48)  panel<4,T>: full k-tiles only, no ragged panel
                    | tn(96 x 64), bx3<2>                      | panel<4,F> ksplit 96 x 64, panel<4,T>
  (6084,  36,  68)  panel<7,T>: NC = 17, ONE float4 in the second lane group (c4 < NC masks the other 15 lanes)
                    | tn(96 x 64), bx3<2>                      | panel<7,F> ksplit 96 x 64, panel<4,T>
  (6084, 112,  64)  panel<4,T> upper edge
                    | tn(96 x 64), bx3<4>                      | panel<4,F> ksplit 96 x 64 (2 row blocks), panel<7,T> upper edge
  (6148, 116, 112)  panel<7,T> upper edge; 97 panels
                    | tn(97 x 64, last chunk 4 pairs), bx3<4>  | panel<7,F> ksplit 97 x 64, panel<13,T> lower edge
  (6144, 100, 200)  panel<13,T>, k tail 4
                    | tn(96 x 64, 2 quadrants), bx3<4>         | panel<13,F> ksplit 96 x 64, panel<7,T>, k tail 8
  (6084, 208, 212)  panel<19,T> lower edge
                    | tn(64 x 96, 4 quadrants), two-group bx3<4> | panel<19,F> ksplit 64 x 96 (4 row blocks), panel<13,T> upper edge
  (6084, 300, 300)  panel<19,T>, k tail 12: cfg 3's widths
                    | tn(64 x 96, 4 quadrants), two-group bx3<5> | panel<19,F> ksplit 48 x 128 (5 row blocks), panel<19,T>
  (6148, 304, 304)  panel<19,T>: the widest the kernel takes
                    | tn(49 x 128, last chunk 4 pairs), two-group bx3<5> | panel<19,F> ksplit 39 x 160, panel<19,T>
  (6080, 300, 300)  NOT fused (95 panels): SimMatrix x 2 -> PairRankLoss -> SimMatrix backward x 2 -> split_sum; held to the same
                    checks as far as they apply (the exact probes, the dense rule).

One-line mutations of the fused route, each tried once on a scratch build (none changes an address or a bound), and the tests of
this module that fail: Y2's registers loaded from Y -- all three; trip_s0 / trip_s1 swapped -- all three; trip_hinge_ge forced to
0 -- the exact probe under the "gpu" hinge mode (18 cases); B = g+ a+ + g+ a- -- all three (probes "a-" and "both"); the `ones`
fill set to 2.0 -- all three in "fp32" mode; pair_grad's `> 0` on `similar` made `>= 0` -- every exact probe; a non-null k-scale
handed to bx3_tn_kernel -- all three in "bf16x3" mode.  The module runs in about 15 s on an MI355X (114 cases).
"""
import functools

import numpy as np
import pytest
import torch

import matrix_pipe_model as mp
from matrix_pipe_model import check_probe, diag_of
from util import rng

pytestmark = pytest.mark.gpu

FUSED = [(6084, 4, 4), (6144, 64, 48), (6084, 36, 68), (6084, 112, 64), (6148, 116, 112), (6144, 100, 200), (6084, 208, 212),
         (6084, 300, 300), (6148, 304, 304)]
FALLBACK = (6080, 300, 300)
SHAPES = FUSED + [FALLBACK]
OUTPUTS = ("s_pos", "s_neg", "loss", "dq", "da_pos", "da_neg", "dW")
GUARD = 64          # floats: 256 bytes, keeps an output's 16-byte alignment
DEVICE = "cuda"


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEVICE)


def host(t):
    return t.detach().cpu().numpy()


MODES = ["bf16x3", "fp32"]


@pytest.fixture
def in_matrix_mode(request, hiplib):
    """Selects the test's `matrix_mode` parameter around it.  (The mode is a parameter, not a fixture's, and the outermost mark: it
    then varies fastest and both modes of a shape share one cached CPU reference.)"""
    from mms_answer_selection_amd import capi
    capi.set_matrix_mode(request.node.callspec.params["matrix_mode"])
    yield
    capi.set_matrix_mode("bf16x3")


class Guarded:
    """An output that starts as NaN between two NaN guard words of GUARD floats each (init: its starting values instead)."""

    def __init__(self, shape, init=None):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEVICE)
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        assert self.t.data_ptr() % 16 == 0 and self.t.is_contiguous()
        if init is not None:
            self.t.copy_(dev(init))

    def guards_intact(self):
        return bool(torch.isnan(self.buf[:GUARD]).all()) and bool(torch.isnan(self.buf[-GUARD:]).all())

    def bits(self):
        return self.buf.view(torch.int32).clone()


class Step:
    """One problem on the device; run() makes one call into fresh guarded outputs and returns them as host arrays."""

    def __init__(self, q, ap, an, y, W, margin, lw):
        self.h = dict(q=q, a_pos=ap, a_neg=an, y=y, W=W)
        self.d = {k: dev(v) for k, v in self.h.items()}
        self.N, self.K1, self.K2 = q.shape[0], q.shape[1], ap.shape[1]
        self.margin, self.lw = margin, lw

    def fresh(self, dW0):
        N, K1, K2 = self.N, self.K1, self.K2
        return dict(s_pos=Guarded((N, 1)), s_neg=Guarded((N, 1)), loss=Guarded((1,)), dq=Guarded((N, K1)),
                    da_pos=Guarded((N, K2)), da_neg=Guarded((N, K2)), dW=Guarded((K1, K2), dW0))

    def call(self, out, with_loss=True):
        from mms_answer_selection_amd import capi
        d = self.d
        args = {k: (v.t if with_loss or k != "loss" else None) for k, v in out.items()}
        capi.triplet_simmatrix_step(d["q"], d["a_pos"], d["a_neg"], d["y"], d["W"], margin=self.margin, loss_weight=self.lw, **args)
        torch.cuda.synchronize()
        for k, v in out.items():
            assert v.guards_intact(), "%s: a store outside the output" % k
        for k, v in self.h.items():
            assert np.array_equal(host(self.d[k]).view(np.uint32), v.view(np.uint32)), "the call changed its input %s" % k

    def run(self, dW0=None):
        out = self.fresh(np.zeros((self.K1, self.K2), np.float32) if dW0 is None else dW0)
        self.call(out)
        g = {k: host(v.t) for k, v in out.items()}
        for k, v in g.items():
            assert np.isfinite(v).all(), "%s: %d elements not written (or not finite)" % (k, int((~np.isfinite(v)).sum()))
        return g, out


def pairrank_at(oracle, s_pos, s_neg, y, margin, lw, hinge="cpu"):
    """(g+, g-, terms) of PairRankLoss at the given fp32 scores, by the project's statement of the reference
    (oracle/mms_oracle_impl.h).  hinge "gpu": the .cu file's `ordered >= 0` -- it differs from `>` at ordered == 0 only, where a
    positive stand-in for `ordered` makes the oracle's strict test let the term through."""
    _, o, s = oracle.pairrank_forward(s_pos, s_neg, y, margin)
    terms = np.maximum(o.astype(np.float64), 0.0) + np.abs((1.0 - y.astype(np.float64)) * s.astype(np.float64))
    og = np.where(o == 0, np.float32(1.0), o) if hinge == "gpu" else o
    gp, gn = oracle.pairrank_backward(y, og, s, top_diff=lw)
    return gp, gn, terms, o, s


# ----------------------------------------------------------------------------------------------------------------------
# 1. exact probes of the whole step
# ----------------------------------------------------------------------------------------------------------------------
MARGIN_X = 2.0
# (label, y, s+, s-, kind).  kind "hot": q = e_k, a+ = u e_j, a- = v e_j' with |W[k, j]| = |W[k, j']| = 1 and u, v chosen so that the
# scores are exactly (s+, s-); "same": a+ == a- (one-hot): B and dq's row are exactly zero; the dense kinds copy random rows.
# ordered = margin - y (s+ - s-), similar = s+ - s-, inner = [ordered > 0] y - ((1 - y) similar > 0 ? 1 : -1) (1 - y).
CASES = [
    ("ordered == 0, y = 1", 1.0, 1, -1, "hot"),
    ("ordered = +1", 1.0, 2, 1, "hot"),
    ("ordered = -1", 1.0, 2, -1, "hot"),
    ("y = 0, similar == 0: the > 0 test gives -1", 0.0, 1, 1, "hot"),
    ("y = 0, similar > 0", 0.0, 2, 1, "hot"),
    ("y = 0, similar < 0", 0.0, 1, 2, "hot"),
    ("y = 0.5, ordered == 0", 0.5, 2, -2, "hot"),
    ("y = 0.5, inner 0", 0.5, 1, -1, "hot"),
    ("y = 0.5, inner 1", 0.5, -1, 1, "hot"),
    ("y = 2, ordered == 0, inner -1", 2.0, 2, 1, "hot"),
    ("y = 2, inner 3", 2.0, 1, 2, "hot"),
    ("y = 2, inner 1", 2.0, 1, 1, "hot"),
    ("y = 2, ordered < 0", 2.0, 1, -1, "hot"),
    ("ordered == 0 with a- = 0: Y's registers alone", 1.0, 2, 0, "hot"),
    ("ordered == 0 with a+ = 0: Y2's registers alone", 1.0, 0, -2, "hot"),
    ("a+ == a-, y = 1", 1.0, 1, 1, "same"),
    ("a+ == a-, y = 0", 0.0, 2, 2, "same"),
    ("dense a+ == a-", 1.0, None, None, "dense same"),
    ("dense, a- = 0, y = 1", 1.0, None, None, "dense an0"),
    ("dense, a+ = 0, y = 1", 1.0, None, None, "dense ap0"),
    ("dense, a- = 0, y = 0", 0.0, None, None, "dense an0"),
    ("dense, a+ = 0, y = 0", 0.0, None, None, "dense ap0"),
]


def planted_rows(N, shape_index):
    """{row: case}.  Panel 0, an interior panel and the last full panel are planted whole (64 rows: every row position g + 4 rr of
    every wave's block), case = (position + rotation) % len(CASES); the rows of the ragged last panel (4 rows at N = 6084, 6148)
    take "ordered == 0, y = 1" first and then cases that rotate with the shape."""
    nc, plan = len(CASES), {}
    panels = (N + 63) // 64
    last_full = N // 64 - 1
    for t, pnl in enumerate((0, panels // 2, last_full)):
        for pos in range(64):
            plan[pnl * 64 + pos] = (pos + 7 * t + 3 * shape_index) % nc
    for j, row in enumerate(range(64 * (N // 64), N)):
        plan[row] = 0 if j == 0 else (j + 3 * shape_index) % nc
    return plan


@functools.lru_cache(maxsize=2)
def exact_problem(shape):
    """Inputs and their fp64 products for the exact probe.  Everything is a small integer; the bounds that make the GPU's fp32
    arithmetic exact in ANY order are asserted in exact_expected()."""
    N, K1, K2 = shape
    r = rng(17 * N + 3 * K1 + K2)
    vals = np.array([-2, -1, 1, 2, -2, -1, 1, 2, 0], np.float32)            # mostly nonzero

    def draw(*s):
        return vals[r.integers(0, vals.size, s)]

    q, ap, an, W, dW0 = draw(N, K1), draw(N, K2), draw(N, K2), draw(K1, K2), draw(K1, K2)
    y = (r.uniform(size=(N, 1)) < 0.7).astype(np.float32)
    k = np.arange(K1)
    W[k, k % K2] = np.where(r.integers(0, 2, K1) == 0, -1.0, 1.0)           # two unit entries per row of W: the planted scores
    W[k, (k + 1) % K2] = np.where(r.integers(0, 2, K1) == 0, -1.0, 1.0)
    plan = planted_rows(N, SHAPES.index(shape))
    for row, c in plan.items():
        _, yy, sp, sn, kind = CASES[c]
        y[row, 0] = yy
        if kind.startswith("dense"):
            if kind == "dense same":
                an[row] = ap[row]
            elif kind == "dense an0":
                an[row] = 0
            else:
                ap[row] = 0
            continue
        kk = row % K1
        j, j2 = kk % K2, (kk + 1) % K2
        q[row], ap[row], an[row] = 0, 0, 0
        q[row, kk] = 1
        if kind == "same":
            ap[row, j] = an[row, j] = sp * W[kk, j]
        else:
            ap[row, j], an[row, j2] = sp * W[kk, j], sn * W[kk, j2]
    q64, ap64, an64, W64 = (x.astype(np.float64) for x in (q, ap, an, W))
    P = q64 @ W64
    sp, sn = np.sum(P * ap64, axis=1, keepdims=True), np.sum(P * an64, axis=1, keepdims=True)
    for row, c in plan.items():
        if CASES[c][2] is not None:
            assert (sp[row, 0], sn[row, 0]) == (CASES[c][2], CASES[c][3]), "planted scores of row %d" % row
    for x in (q, ap, an, W, dW0):
        assert np.abs(x).max() <= 2
    return dict(q=q, ap=ap, an=an, W=W, dW0=dW0, y=y, P=P, sp=sp, sn=sn, plan=plan)


def exact_expected(pr, oracle, hinge):
    """fp64 expectations of every output, and the proof that they are what ANY fp32 summation order gives: all values are multiples
    of 1/2 and every sum of absolute values that bounds a partial sum is below 2^23 (so: < 2^24 half-units)."""
    q, ap, an, W, dW0, y, P = (pr[k].astype(np.float64) for k in ("q", "ap", "an", "W", "dW0", "y", "P"))
    N = q.shape[0]
    sp32, sn32 = pr["sp"].astype(np.float32), pr["sn"].astype(np.float32)
    assert (sp32 == pr["sp"]).all() and (sn32 == pr["sn"]).all()
    gp, gn, terms, o, s = pairrank_at(oracle, sp32, sn32, pr["y"], MARGIN_X, float(N), hinge)       # scale = N / N = 1
    gp, gn = gp.astype(np.float64), gn.astype(np.float64)
    B = gp * ap + gn * an
    e = dict(s_pos=pr["sp"], s_neg=pr["sn"], da_pos=gp * P, da_neg=gn * P, dq=B @ W.T, dW=dW0 + q.T @ B, dW2=dW0 + 2.0 * (q.T @ B))
    S = terms.sum()
    Pb = np.abs(q) @ np.abs(W)
    Bb = np.abs(gp) * np.abs(ap) + np.abs(gn) * np.abs(an)
    bounds = dict(P=Pb, s_pos=np.sum(Pb * np.abs(ap), axis=1), s_neg=np.sum(Pb * np.abs(an), axis=1), da=np.maximum(np.abs(gp), np.abs(gn)) * Pb,
                  B=Bb, dq=Bb @ np.abs(W).T, dW=np.abs(dW0) + 2.0 * (np.abs(q).T @ Bb), loss=np.abs(terms).sum())
    for name, b in bounds.items():
        assert 2.0 * np.max(b) < 2.0 ** 24, "%s: a partial sum could leave fp32's exact integers (bound %g)" % (name, np.max(b))
    for name, v in list(e.items()) + [("terms", terms), ("B", B), ("g+", gp), ("g-", gn)]:
        assert (np.round(2.0 * v) == 2.0 * v).all(), "%s: not a multiple of 1/2" % name
        assert (v.astype(np.float32).astype(np.float64) == v).all(), name
    # loss_finish_kernel ends as the reference does (pair_rank_loss_layer.cpp:49): ONE fp32 division of the sum by the count.  The
    # sum of the terms is exact, so the loss is that correctly rounded quotient: bit equality, not 2 ulp.
    e["loss"] = np.array([np.float32(S) / np.float32(N)], np.float32).astype(np.float64)
    assert np.float64(np.float32(S)) == S
    return e, dict(o=o, s=s, gp=gp, gn=gn)


def assert_exact(got, want, what):
    """Bit for bit apart from the sign of a zero: `want` is fp64 and exactly representable, so numeric equality says it."""
    g = np.asarray(got, dtype=np.float64)
    assert g.shape == want.shape, (what, g.shape, want.shape)
    bad = g != want
    assert not bad.any(), "%s: %d of %d elements differ, first at %s: got %r, exact %r" % (
        what, int(bad.sum()), bad.size, tuple(int(v) for v in np.argwhere(bad)[0]), g[bad][0], want[bad][0])


@pytest.mark.parametrize("matrix_mode", MODES)
@pytest.mark.parametrize("hinge", ["cpu", "gpu"])
@pytest.mark.parametrize("shape", SHAPES)
def test_exact_probe_of_the_whole_step(shape, hinge, matrix_mode, oracle, in_matrix_mode):
    """Every output of the step, bit for bit (apart from the sign of a zero) against fp64, on integer inputs with planted decision
    edges; outputs start as NaN between NaN guards; inputs are compared with their host copies afterwards; a second call with
    loss = NULL changes no bit of any other output and accumulates dW again, exactly.  The loss is held to bit equality with
    float32(sum) / float32(N): the sum is exact and loss_finish_kernel ends with the reference's one division."""
    from mms_answer_selection_amd import capi
    pr = exact_problem(shape)
    want, _ = exact_expected(pr, oracle, hinge)
    N = shape[0]
    st = Step(pr["q"], pr["ap"], pr["an"], pr["y"], pr["W"], MARGIN_X, float(N))
    capi.set_pairrank_hinge_mode(hinge)
    try:
        g, out = st.run(pr["dW0"])
        what = "%s %s hinge %s: " % (shape, matrix_mode, hinge)
        for k in OUTPUTS:
            assert_exact(g[k], want[k], what + k)
        first = {k: v.bits() for k, v in out.items()}
        st.call(out, with_loss=False)
        for k in OUTPUTS:
            if k != "dW":
                assert torch.equal(out[k].bits(), first[k]), what + "the second call (loss = NULL) changed " + k
        assert_exact(host(out["dW"].t), want["dW2"], what + "dW accumulated twice")
    finally:
        capi.set_pairrank_hinge_mode("cpu")


# ----------------------------------------------------------------------------------------------------------------------
# 2. single-product probes at the fused shapes
# ----------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24


def gamma(n):
    """The bound of an fp32 sum of n products taken in any order: |fl(sum x_j y_j) - sum x_j y_j| <= gamma_n sum |x_j y_j|."""
    return n * U / (1.0 - n * U)


@pytest.mark.parametrize("matrix_mode", MODES)
@pytest.mark.parametrize("probe", ["a+", "a-", "both"])
@pytest.mark.parametrize("shape", FUSED)
def test_probe_fused_step(shape, probe, matrix_mode, oracle, in_matrix_mode):
    """The construction of test_gpu_matrix_pipe_accuracy.py::test_probe_triplet_simmatrix_step at the shapes that fuse: y = 1,
    loss_weight = N and a margin no score reaches make g+ = -1 and g- = +1 (asserted from PairRankLoss at the GPU's own scores).
      "a+":   a- = 0, so B = g+ a+ -- the probe as it was;  "a-": mirrored, a+ = 0: the second answer's half of B;
      "both": both answers are populated on DISJOINT columns, so each element of B is still one exact value.  For dq, W is a
              checkerboard (W[k, j] = 0 for k + j odd) and the answers are one-hot at columns of opposite parity: every dq element
              stays ONE product, from a+ for half of the k and from a- for the other half.
    Three calls: (A) dq = B W^T;  (B) dW += Q^T B onto a nonzero dW, q with one nonzero per column;  (C) one-hot q and answers: the
    scores are triple products and da+- / g+- is the row of Q W, single products -- the forward instantiation at the bar.
    In every call da+- = g+- P for ONE common row P, bit for bit, and the epilogue's dots agree with the fp64 dot of that P with the
    answers within gamma_K2 sum |P_j a_j| (a derived bound: any summation order of K2 fp32 products)."""
    N, K1, K2 = shape
    r = rng(5 * N + K1 + 3 * K2 + len(probe))
    margin, lw = 1.0e6, float(N)
    y = np.ones((N, 1), np.float32)
    i = np.arange(N)
    what = "%s %s probe %s: " % (shape, matrix_mode, probe)
    zeros = np.zeros((N, K2), np.float32)

    def step(q, ap, an, W, dW0=None):
        g, _ = Step(q, ap, an, y, W, margin, lw).run(dW0)
        gp, gn, _, _, _ = pairrank_at(oracle, g["s_pos"], g["s_neg"], y, margin, lw)
        assert (gp == -1.0).all() and (gn == 1.0).all(), "the probe needs g+ = -1, g- = +1 on every row"
        # da+- = g+- times ONE row P: with g+ = -1, g- = +1 that is da- == -da+ numerically; P = da+ / g+ exactly
        assert (g["da_neg"].astype(np.float64) == -g["da_pos"].astype(np.float64)).all(), what + "da_neg != -da_pos"
        P = -g["da_pos"].astype(np.float64)
        for name, a in (("s_pos", ap), ("s_neg", an)):
            a64 = a.astype(np.float64)
            d64, dabs = np.sum(P * a64, axis=1, keepdims=True), np.sum(np.abs(P * a64), axis=1, keepdims=True)
            err = np.abs(g[name].astype(np.float64) - d64)
            bad = err > gamma(K2) * dabs
            assert not bad.any(), what + "%s: the epilogue's dot is %.3g from the fp64 dot of its own P row at row %d (bound %.3g)" % (
                name, err[bad][0], int(np.argwhere(bad)[0][0]), (gamma(K2) * dabs)[bad][0])
        return g, gp, gn, P

    Wd = mp.probe_values(r, (K1, K2))[0]
    # (A) dq
    v1, v2 = mp.probe_values(r, (N,))[0], mp.probe_values(r, (N,))[0]
    q = mp.probe_values(r, (N, K1))[0]
    if probe == "both":
        W = (Wd * ((np.arange(K1)[:, None] + np.arange(K2)[None, :]) % 2 == 0)).astype(np.float32)
        ap, an = mp.one_per_row(v1, K2), mp.one_per_row(v2, K2, offset=1)
    else:
        W = Wd
        ap, an = (mp.one_per_row(v1, K2), zeros) if probe == "a+" else (zeros, mp.one_per_row(v1, K2))
    g, gp, gn, _ = step(q, ap, an, W)
    B = (gp * ap + gn * an).astype(np.float32)                              # exact: disjoint support, g = +-1
    bcol = np.where(W[:, i % K2].T != 0, diag_of(B, K2)[:, None], diag_of(B, K2, 1)[:, None]) if probe == "both" else diag_of(B, K2)[:, None]
    wcol = np.where(W[:, i % K2].T != 0, W[:, i % K2].T, W[:, (i + 1) % K2].T) if probe == "both" else W[:, i % K2].T
    check_probe(what + "dq", g["dq"], B, W.T, single=(bcol, wcol))
    # (B) dW, accumulated onto a nonzero dW of 1/8 of the product's magnitude (few bits: one rounding, in the bar's budget)
    rows = mp.tn_rows(N, K1)
    qc = mp.one_per_column(mp.probe_values(r, (K1,))[0], N)
    d1, d2 = mp.probe_values(r, (N, K2))[0], mp.probe_values(r, (N, K2))[0]
    if probe == "both":
        even = (np.arange(K2) % 2 == 0)[None, :]
        ap, an = (d1 * even).astype(np.float32), (d2 * ~even).astype(np.float32)
    else:
        ap, an = (d1, zeros) if probe == "a+" else (zeros, d1)
    dW0 = (0.125 * r.integers(-4, 5, (K1, K2)) / 4.0).astype(np.float32)
    g, gp, gn, _ = step(qc, ap, an, Wd, dW0)
    B = (gp * ap + gn * an).astype(np.float32)
    check_probe(what + "dW", g["dW"], qc.T, B, extra=dW0, single=(qc[rows, np.arange(K1)][:, None], B[rows, :]))
    # (C) the forward: Q W (read back as da+- / g+-) and both scores
    q = mp.one_per_row(mp.probe_values(r, (N,))[0] * mp.pow2(r, (N,), -8, 8, signed=False), K1)
    s1 = mp.probe_values(r, (N,))[0] * mp.pow2(r, (N,), -8, 8, signed=False)
    s2 = mp.probe_values(r, (N,))[0] * mp.pow2(r, (N,), -8, 8, signed=False)
    if probe == "both":
        ap, an = mp.one_per_row(s1, K2, offset=3), mp.one_per_row(s2, K2, offset=2)
    else:
        ap, an = (mp.one_per_row(s1, K2, offset=3), zeros) if probe == "a+" else (zeros, mp.one_per_row(s1, K2, offset=3))
    g, gp, gn, P = step(q, ap, an, Wd)
    check_probe(what + "Q.W (da_pos / g+)", P, q, Wd, single=(diag_of(q, K1)[:, None], Wd[i % K1, :]))
    qw64, D = mp.reference(q, Wd)
    for name, a, off in (("s_pos", ap, 3), ("s_neg", an, 2 if probe == "both" else 3)):
        a64 = a.astype(np.float64)
        t64, tD = np.sum(qw64 * a64, axis=1, keepdims=True), np.sum(D * np.abs(a64), axis=1, keepdims=True)
        e, idx = mp.componentwise_error(g[name], t64, tD, what + name)
        print(what + "%s: e = %.3g" % (name, e))
        av = diag_of(a, K2, off)
        hint = ""
        if e > mp.BAR:
            hint = mp.name_lost_term(diag_of(q, K1), Wd[i % K1, (i + off) % K2], g[name][:, 0].astype(np.float64) / np.where(av != 0, av, 1.0))
        assert e <= mp.BAR, what + "%s: componentwise error %.3g > %.3g at row %d; %s" % (name, e, mp.BAR, idx[0], hint)


# ----------------------------------------------------------------------------------------------------------------------
# 3. dense data
# ----------------------------------------------------------------------------------------------------------------------
MARGIN_D, LW_D, EDGE = 0.3, 1.0, 1.0e-4


def decisions64(sp, sn, y, margin):
    """(inner, ordered, similar, near) in fp64 (pairrank_math.h on exact scores).  near: a row within EDGE of an edge -- |ordered|
    (where y != 0: at y = 0 `ordered` is the margin itself) or |(1 - y) similar| (where y != 1: at y = 1 the factor 1 - y removes
    `similar` from the result) below EDGE (|s+| + |s-| + margin)."""
    similar = sp - sn
    ordered = margin - y * similar
    inner = (ordered > 0) * y - np.where((1.0 - y) * similar > 0, 1.0, -1.0) * (1.0 - y)
    thr = EDGE * (np.abs(sp) + np.abs(sn) + margin)
    near = ((y != 0) & (np.abs(ordered) < thr)) | ((y != 1) & (np.abs((1.0 - y) * similar) < thr))
    return inner, ordered, similar, near


def dense_inputs_redrawn(shape):
    """The suite's usual data (matrix_pipe_model.dense_inputs, y from {0, 1}) with the rows near a decision edge redrawn, and its
    fp64 scores and decisions.  Asserts that the redraw terminates and took fewer than 1 % of the rows."""
    N, K1, K2 = shape
    r = rng(N + 5 * K1 + 11 * K2)
    q, ap, W, _ = mp.dense_inputs(r, N, K1, K2)
    an = (r.standard_normal((N, K2)) * 0.4).astype(np.float32)
    y = (r.uniform(size=(N, 1)) < 0.8).astype(np.float32)
    W64, y64 = W.astype(np.float64), y.astype(np.float64)
    redrawn = 0
    for rounds in range(20):
        P64 = q.astype(np.float64) @ W64
        sp = np.sum(P64 * ap.astype(np.float64), axis=1, keepdims=True)
        sn = np.sum(P64 * an.astype(np.float64), axis=1, keepdims=True)
        inner, ordered, similar, near = decisions64(sp, sn, y64, MARGIN_D)
        rows = np.flatnonzero(near[:, 0])
        if rows.size == 0:
            break
        redrawn += rows.size
        q[rows] = (r.standard_normal((rows.size, K1)) * 0.4).astype(np.float32)
        ap[rows] = (r.standard_normal((rows.size, K2)) * 0.4).astype(np.float32)
        an[rows] = (r.standard_normal((rows.size, K2)) * 0.4).astype(np.float32)
    else:
        raise AssertionError("the redraw of rows near a decision edge did not terminate")
    assert redrawn < 0.01 * N, "%d of %d rows had to be redrawn" % (redrawn, N)
    return q, ap, an, y, W, P64, sp, sn, inner, redrawn


@functools.lru_cache(maxsize=2)
def dense_problem(shape, oracle):
    """dense_inputs_redrawn, the fp64 reference of every output and the CPU oracle's chain on the same inputs."""
    N, K1, K2 = shape
    q, ap, an, y, W, P64, sp, sn, inner, redrawn = dense_inputs_redrawn(shape)
    W64 = W.astype(np.float64)
    scale = np.float64(np.float32(LW_D) / np.float32(N))                    # pair_rank_loss_layer.cpp:64, formed in fp32
    gp64, gn64 = -scale * inner, scale * inner
    q64, ap64, an64 = (x.astype(np.float64) for x in (q, ap, an))
    PD = np.abs(q64) @ np.abs(W64)
    B64 = gp64 * ap64 + gn64 * an64
    BD = np.abs(gp64) * np.abs(ap64) + np.abs(gn64) * np.abs(an64)
    refs = dict(s_pos=(sp, np.sum(PD * np.abs(ap64), axis=1, keepdims=True)), s_neg=(sn, np.sum(PD * np.abs(an64), axis=1, keepdims=True)),
                da_pos=(gp64 * P64, np.abs(gp64) * PD), da_neg=(gn64 * P64, np.abs(gn64) * PD),
                dq=(B64 @ W64.T, BD @ np.abs(W64).T), dW=(q64.T @ B64, np.abs(q64).T @ BD))
    # the CPU oracle's chain on the same inputs
    osp, _ = oracle.simmatrix_forward(q, ap, W)
    osn, _ = oracle.simmatrix_forward(q, an, W)
    oloss, oo, os_ = oracle.pairrank_forward(osp, osn, y, MARGIN_D)
    ogp, ogn = oracle.pairrank_backward(y, oo, os_, top_diff=LW_D)
    assert (ogp.astype(np.float64) == gp64).all() and (ogn.astype(np.float64) == gn64).all(), "the oracle's own scores decide as fp64 does"
    zero = np.zeros((K1, K2), np.float32)
    odq_p, odap, odW1 = oracle.simmatrix_backward(q, ap, W, ogp, dW_in=zero)
    odq_n, odan, odW = oracle.simmatrix_backward(q, an, W, ogn, dW_in=odW1)
    orc = dict(s_pos=osp, s_neg=osn, da_pos=odap, da_neg=odan, dq=odq_p + odq_n, dW=odW)
    e_oracle = {k: mp.componentwise_error(orc[k], refs[k][0], refs[k][1], "oracle " + k)[0] for k in refs}
    return dict(q=q, ap=ap, an=an, y=y, W=W, refs=refs, e_oracle=e_oracle, loss=float(oloss), gp=gp64, gn=gn64, redrawn=redrawn)


@pytest.mark.parametrize("matrix_mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_dense_decisions_errors_and_determinism(shape, matrix_mode, oracle, in_matrix_mode):
    """Dense data whose rows are all at least 1e-4 (relative to |s+| + |s-| + margin) from a decision edge: no fp32-accurate score
    can change a decision, so ZERO rows may decide differently from the fp64 scores; s+-, da+-, dq and dW (onto a zero dW) within
    twice the CPU oracle's own componentwise error against fp64, + 2^-24 (test_dense_error_within_twice_the_references' rule); the
    loss within 1e-5 of the oracle's; a second call gives the same bits everywhere."""
    N, K1, K2 = shape
    pr = dense_problem(shape, oracle)
    st = Step(pr["q"], pr["ap"], pr["an"], pr["y"], pr["W"], MARGIN_D, LW_D)
    g, out = st.run()
    what = "%s %s: " % (shape, matrix_mode)
    gp, gn, _, _, _ = pairrank_at(oracle, g["s_pos"], g["s_neg"], pr["y"], MARGIN_D, LW_D)
    flips = int(((gp.astype(np.float64) != pr["gp"]) | (gn.astype(np.float64) != pr["gn"])).sum())
    assert flips == 0, what + "%d rows decide differently from the fp64 scores (%d rows were redrawn)" % (flips, pr["redrawn"])
    fails = []
    for k, (C64, D) in pr["refs"].items():
        e, idx = mp.componentwise_error(g[k], C64, D, what + k)
        msg = what + "%s: e = %.3g at %s, e(oracle) = %.3g" % (k, e, idx, pr["e_oracle"][k])
        print(msg)
        if not e <= 2.0 * pr["e_oracle"][k] + 2.0 ** -24:
            fails.append(msg)
    assert not fails, "; ".join(fails)
    print(what + "loss %.9g, oracle %.9g" % (g["loss"][0], pr["loss"]))
    assert abs(float(g["loss"][0]) - pr["loss"]) <= 1e-5 * abs(pr["loss"]), what + "loss %.9g, oracle %.9g" % (g["loss"][0], pr["loss"])
    _, out2 = st.run()
    for k in OUTPUTS:
        assert torch.equal(out2[k].bits(), out[k].bits()), what + "a second call gives other bits in " + k
