"""The fp64 paths of csrc/f64_paths.hip held to what double can give (tests/f64_gemm_model.py has the routes, the probes and
the bar): every matrix-pipe product, on both kernels and through every feature of its parameter block, returns the int64
reference BIT FOR BIT on exact-sum probes; scaling the operands by powers of two changes no bit; dense data stays within the
derived gamma_n bar (the only tolerance in this file); batch counts and row counts beyond one launch's grid are sliced; the
cosine and Euclid double kernels give the double oracle's bits on every geometry, on edge rows and on misaligned rows.

Every buffer a call sees lies in one arena with a guard band of a sentinel value after it; outputs are pre-filled with NaN."""
import numpy as np
import pytest
import torch

import f64_gemm_model as gm
from mms_answer_selection_amd import capi

pytestmark = pytest.mark.gpu
GUARD = 32                                    # doubles after every buffer (256 B keeps the 16-byte alignment)
SENT = -777.25


class Arena:
    """Named float64 buffers in ONE device allocation, GUARD sentinel doubles after each (and `lead` before the first, which
    also shifts every buffer by that many doubles: lead = 1 makes every base 8- but not 16-byte aligned).  An entry is an
    array (an input, or an output with incoming contents) or a shape (an output: NaN)."""

    def __init__(self, lead=0, **entries):
        self.span, off = {}, lead
        for k, v in entries.items():
            shape = v.shape if isinstance(v, np.ndarray) else tuple(v)
            n = int(np.prod(shape))
            self.span[k] = (off, n, shape)
            off += (n + 1) // 2 * 2 + GUARD
        host = np.full(off, SENT)
        for k, v in entries.items():
            o, n, _ = self.span[k]
            host[o:o + n] = v.ravel() if isinstance(v, np.ndarray) else np.nan
        self.buf = torch.from_numpy(host).cuda()

    def __getitem__(self, k):
        o, n, shape = self.span[k]
        return self.buf[o:o + n].view(shape)

    def host(self, k):
        return self[k].cpu().numpy()

    def check(self):
        """Every sentinel still holds its bits."""
        torch.cuda.synchronize()
        keep = torch.ones(self.buf.numel(), dtype=torch.bool, device="cuda")
        for o, n, _ in self.span.values():
            keep[o:o + n] = False
        guard = self.buf[keep]
        assert bool((guard.view(torch.int64) == torch.full_like(guard, SENT).view(torch.int64)).all()), "a guard band was written"


def same_bits(x, y):
    """Two device tensors hold the same bytes (NaN included)."""
    return bool((x.contiguous().view(torch.int64) == y.contiguous().view(torch.int64)).all())


def all_nan(x):
    return bool(torch.isnan(x).all())


# ----------------------------------------------------------------------------------------------------------------------
# exact probes
# ----------------------------------------------------------------------------------------------------------------------
def run_simmatrix(p, ref, what, flags=True, scale=None):
    """Forward, backward with every flag, then the flag subsets; every output bit for bit `ref` (times 2^scale[name])."""
    N, K1 = p["q"].shape
    K2 = p["a"].shape[1]
    want = lambda k: ref[(k, False)] if scale is None else np.ldexp(ref[(k, False)].astype(np.float64), scale[k])
    A = Arena(q=p["q"], a=p["a"], W=p["W"], dT=p["dT"], top=(N, 1), scratch=(N, K2), dq=(N, K1), da=(N, K2), dW=p["dW_in"])
    capi.simmatrix_forward_f64(A["q"], A["a"], A["W"], A["top"], A["scratch"])
    capi.simmatrix_backward_f64(A["q"], A["a"], A["W"], A["dT"], A["dq"], A["da"], A["dW"])
    A.check()
    for k in ("top", "scratch", "dq", "da", "dW"):
        gm.assert_bits(A.host(k), want(k), "%s %s" % (k, what))
    if not flags:
        return
    for ppd, pd0, pd1 in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1)):
        O = Arena(dq=(N, K1), da=(N, K2), dW=p["dW_in"])
        capi.simmatrix_backward_f64(A["q"], A["a"], A["W"], A["dT"], O["dq"], O["da"], O["dW"], param_propagate_down=bool(ppd),
                                    propagate_down=(bool(pd0), bool(pd1)))
        O.check()
        fl = "%s flags %d%d%d" % (what, ppd, pd0, pd1)
        assert same_bits(O["dq"], A["dq"]) if pd0 else all_nan(O["dq"]), "dq " + fl
        assert same_bits(O["da"], A["da"]) if pd1 else all_nan(O["da"]), "da " + fl
        if ppd:
            assert same_bits(O["dW"], A["dW"]), "dW " + fl
        else:
            gm.assert_bits(O.host("dW"), p["dW_in"], "untouched dW " + fl)


def run_bilinear(p, ref, bias, what, scale=None):
    """Forward and backward of dist_mode 2; top, dq, da, dW (and dbias, accumulated) bit for bit `ref` (times 2^scale[name])."""
    N, W1, D = p["q"].shape
    M, W2 = p["W"].shape[0], p["a"].shape[1]
    want = lambda k: ref[(k, bias)] if scale is None else np.ldexp(ref[(k, bias)].astype(np.float64), scale[k])
    A = Arena(q=p["q"], a=p["a"], W=p["W"], bias=p["bias"], dT=p["dT"], top=(N, M, W1, W2), dq=(N, W1, D), da=(N, W2, D),
              dW=(M, D, D), dbias=p["dbias_in"])
    capi.simcross_forward_f64(2, A["q"], A["a"], A["top"], W=A["W"], bias=A["bias"] if bias else None)
    gm.assert_bits(A.host("top"), want("top"), "top " + what)
    capi.simcross_backward_f64(2, A["q"], A["a"], A["top"], A["dT"], A["dq"], A["da"], W=A["W"], bias_term=bias, dW=A["dW"],
                               dbias=A["dbias"] if bias else None)
    A.check()
    for k in ("dq", "da", "dW"):
        gm.assert_bits(A.host(k), want(k), "%s %s" % (k, what))
    gm.assert_bits(A.host("dbias"), want("dbias") if bias else p["dbias_in"], "dbias " + what)


@pytest.mark.parametrize("shape", gm.SIMMATRIX, ids=gm.shape_id)
def test_probe_simmatrix(shape, hiplib):
    p, ref = gm.probe_case("simmatrix", shape)
    run_simmatrix(p, ref, str(shape))


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", gm.BILINEAR, ids=gm.shape_id)
def test_probe_bilinear(shape, bias, hiplib):
    p, ref = gm.probe_case("bilinear", shape)
    run_bilinear(p, ref, bias, "%s bias %d" % (shape, bias))


# q x 2^200, W x 2^-180, a x 2^-40, dT x 2^90; what is added to a product carries the product's power
EQ, EW, EA, EG = 200, -180, -40, 90


def _scaled(p, exps):
    return {k: np.ldexp(v, exps[k]) for k, v in p.items()}


# SimMatrix: tiled; tallk (dW tiled).  Bilinear: tiled everywhere; forward and t2 on tallk; dq and da on tallk
@pytest.mark.parametrize("shape", [(37, 24, 19), (70, 1030, 1100), (5, 2, 70, 65, 67), (1, 2, 3, 5, 1028), (2, 2, 516, 515, 5)],
                         ids=gm.shape_id)
def test_power_of_two_scaling_changes_no_bit(shape, hiplib):
    """Any fp32 or bf16 staging of an operand overflows or flushes here; double only moves the exponent."""
    if len(shape) == 3:
        p, ref = gm.probe_case("simmatrix", shape)
        ps = _scaled(p, dict(q=EQ, a=EA, W=EW, dT=EG, dW_in=EG + EQ + EA))
        run_simmatrix(ps, ref, "scaled %s" % (shape,), flags=False,
                      scale=dict(scratch=EQ + EW, top=EQ + EW + EA, dq=EG + EA + EW, da=EG + EQ + EW, dW=EG + EQ + EA))
    else:
        p, ref = gm.probe_case("bilinear", shape)
        ps = _scaled(p, dict(q=EQ, a=EA, W=EW, dT=EG, bias=EQ + EW + EA, dbias_in=EG))
        run_bilinear(ps, ref, True, "scaled %s" % (shape,),
                     scale=dict(top=EQ + EW + EA, dq=EG + EW + EA, da=EG + EQ + EW, dW=EQ + EG + EA, dbias=EG))


# ----------------------------------------------------------------------------------------------------------------------
# dense data: the derived bar
# ----------------------------------------------------------------------------------------------------------------------
def dense_simmatrix(shape):
    v, E, S = gm.dense_case("simmatrix", shape)
    N, K1, K2 = shape
    n = gm.simmatrix_n(shape)
    A = Arena(q=v["q"], a=v["a"], W=v["W"], dT=v["dT"], top=(N, 1), scratch=(N, K2), dq=(N, K1), da=(N, K2), dW=v["dW_in"])
    capi.simmatrix_forward_f64(A["q"], A["a"], A["W"], A["top"], A["scratch"])
    capi.simmatrix_backward_f64(A["q"], A["a"], A["W"], A["dT"], A["dq"], A["da"], A["dW"])
    A.check()
    for k in ("top", "scratch", "dq", "da", "dW"):
        gm.check_dense("%s %s" % (k, shape), A.host(k), *E[k], S[k], n[k])


def dense_bilinear(shape):
    v, E, S = gm.dense_case("bilinear", shape)
    N, M, W1, W2, D = shape
    n = gm.bilinear_n(shape, True)
    A = Arena(q=v["q"], a=v["a"], W=v["W"], bias=v["bias"], dT=v["dT"], top=(N, M, W1, W2), dq=(N, W1, D), da=(N, W2, D),
              dW=(M, D, D), dbias=v["dbias_in"])
    capi.simcross_forward_f64(2, A["q"], A["a"], A["top"], W=A["W"], bias=A["bias"])
    capi.simcross_backward_f64(2, A["q"], A["a"], A["top"], A["dT"], A["dq"], A["da"], W=A["W"], bias_term=True, dW=A["dW"],
                               dbias=A["dbias"])
    A.check()
    for k in ("top", "dq", "da", "dW", "dbias"):
        gm.check_dense("%s %s" % (k, shape), A.host(k), *E[k], S[k], n[k])


@pytest.mark.parametrize("shape", gm.SIMMATRIX_DENSE + gm.BILINEAR_DENSE, ids=gm.shape_id)
def test_dense_within_derived_bar(shape, hiplib):
    """|got - exact| <= gamma_n S on every element of every output (f64_gemm_model has n per product)."""
    (dense_simmatrix if len(shape) == 3 else dense_bilinear)(shape)


# ----------------------------------------------------------------------------------------------------------------------
# more batches or rows than one launch's grid holds
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", gm.BILINEAR_LARGE + gm.SIMMATRIX_LARGE, ids=gm.shape_id)
def test_large_batch_counts_are_sliced(shape, hiplib):
    """Bilinear: N M = 65538 (two slices, 21845 pairs and 1) and exactly 65535 (one launch).  SimMatrix: 65537 row tiles, so
    forward, dq and da take two launches (65535 tiles and 2) and dW runs on the long-K kernel over 4 M rows.  Every element of
    forward and backward, bit for bit."""
    if len(shape) == 3:
        return large_simmatrix(shape)
    N, M = shape[:2]
    assert [x["launches"] for x in gm.routes("simcross_forward", shape)] == ([2, 2] if N * M > gm.GRID_MAX else [1, 1])
    p = gm.bilinear_probe(shape)
    ref = {(k, True): v for k, v in gm.bilinear_ref(p, True).items()}
    run_bilinear(gm.f64(p), ref, True, str(shape))


def large_simmatrix(shape):
    assert gm.routes("simmatrix_forward", shape)[0]["launches"] == 2
    p = gm.simmatrix_probe(shape)
    ref = {(k, False): v for k, v in gm.simmatrix_ref(p).items()}
    run_simmatrix(gm.f64(p), ref, str(shape), flags=False)


# ----------------------------------------------------------------------------------------------------------------------
# cosine and Euclid in double: geometry and edge rows
# ----------------------------------------------------------------------------------------------------------------------
COSINE = [(1, 1, 1, 1), (5, 1, 1, 3), (6, 1, 1, 63), (7, 1, 1, 64), (9, 1, 1, 65), (3, 1, 1, 300), (3, 5, 7, 9), (2, 1, 4, 16)]


def nan_blind_bits(got, ref, what):
    """Bit patterns equal, up to the payload (and sign) of a NaN."""
    got, ref = np.asarray(got), np.asarray(ref).reshape(np.shape(got))
    both_nan = np.isnan(got) & np.isnan(ref)
    bad = np.flatnonzero(((gm.bits(got) != gm.bits(ref)) & ~both_nan).ravel())
    assert bad.size == 0, "%s: %d of %d elements differ, first at %s: got %r, oracle %r" % (
        what, bad.size, got.size, np.unravel_index(int(bad[0]), got.shape), got.ravel()[bad[0]], ref.ravel()[bad[0]])


def cosine_inputs(shape):
    N, W1, W2, D = shape
    r = np.random.default_rng(1701 + gm.shape_seed(shape))
    ints = lambda s: (r.integers(1, 5, s) * np.where(r.integers(0, 2, s) == 0, -1, 1)).astype(np.float64)
    dT = r.choice(np.array([1.0, 3.0, 5.0]), (N, 1, W1, W2)) * np.ldexp(1.0, r.integers(-4, 5, (N, 1, W1, W2)))
    return ints((N, W1, D)), ints((N, W2, D)), dT * np.where(r.integers(0, 2, dT.shape) == 0, -1.0, 1.0)


def run_cosine(q, a, dT, oracle, what):
    N, W1, D = q.shape
    W2 = a.shape[1]
    with np.errstate(all="ignore"):
        top_o, n0_o, n1_o = oracle.simcross_forward(0, q, a)
        dq_o, da_o, _, _ = oracle.simcross_backward(0, q, a, top_o, dT, norm0=n0_o, norm1=n1_o)
    A = Arena(q=q, a=a, dT=dT, top=(N, 1, W1, W2), n0=(N, W1), n1=(N, W2), dq=(N, W1, D), da=(N, W2, D))
    capi.simcross_forward_f64(0, A["q"], A["a"], A["top"], norm0=A["n0"], norm1=A["n1"])
    capi.simcross_backward_f64(0, A["q"], A["a"], A["top"], A["dT"], A["dq"], A["da"], norm0=A["n0"], norm1=A["n1"])
    A.check()
    out = {k: A.host(k) for k in ("top", "n0", "n1", "dq", "da")}
    for k, o in (("top", top_o), ("n0", n0_o), ("n1", n1_o), ("dq", dq_o), ("da", da_o)):
        nan_blind_bits(out[k], o, "%s %s" % (k, what))
    return out


@pytest.mark.parametrize("shape", COSINE, ids=gm.shape_id)
def test_cosine_f64_bit_for_bit_on_probes_and_edge_rows(shape, oracle, hiplib):
    """Integers in [-4, 4]: the three dot products are exact in any order, so top, norm0 and norm1 are the oracle's bits, and
    the backward (d_cross_bwd<0>: the reference's expression in the reference's order) is too.  Then one all-zero q row, one
    all-zero a row, one +inf and one NaN, each in a pair of its own while pairs last: the oracle's bits up to NaN payload,
    and the last pair, which holds no edge, keeps every bit of the clean run."""
    N, W1, W2, D = shape
    q, a, dT = cosine_inputs(shape)
    clean = run_cosine(q, a, dT, oracle, "%s clean" % (shape,))
    assert all(np.isfinite(v).all() for v in clean.values())
    if N < 2:
        return
    qe, ae = q.copy(), a.copy()
    edges = [(qe, 1 % W1, "zero"), (ae, 2 % W2, "zero"), (qe, 0, "inf"), (ae, 3 % W2, "nan")]
    for i, (x, w, kind) in enumerate(edges):
        n = i % (N - 1)                                         # pair N - 1 stays clean
        if kind == "zero":
            x[n, w] = 0.0
        else:
            x[n, w, (2 * i + n) % D] = np.inf if kind == "inf" else np.nan
    got = run_cosine(qe, ae, dT, oracle, "%s edges" % (shape,))
    assert np.isnan(got["top"]).any() and np.isinf(got["n0"]).any()
    if N >= 5 or W1 > 1:                                        # the zero rows are rows of their own
        assert (got["n0"] == 0).any() and (got["n1"] == 0).any()
    for k in got:
        assert (gm.bits(got[k][N - 1]) == gm.bits(clean[k][N - 1])).all(), "%s: the clean pair changed" % k
    if N >= 5:                                                  # one edge per pair: pairs 4 .. N - 1 are all clean
        for k in got:
            assert (gm.bits(got[k][4:]) == gm.bits(clean[k][4:])).all(), k


@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "offset8"])
@pytest.mark.parametrize("D", [15, 16, 17, 31, 32, 33, 48, 300])
def test_euclid_rows_f64_on_misaligned_bases(D, lead, oracle, hiplib):
    """d_euclid_rows_fwd takes its 16-byte loads only where both rows are 16-byte aligned: on a base that is 8-byte but not
    16-byte aligned every row of an even D (every other row of an odd one) falls to the scalar loop.  The d-ascending sum is
    the oracle's either way, more than one block of 64 pairs."""
    N = 67
    r = np.random.default_rng(1701 + 13 * D)
    q, a = r.standard_normal((N, 1, D)) * 0.4, r.standard_normal((N, 1, D)) * 0.4
    top_o, _, _ = oracle.simcross_forward(1, q, a)
    A = Arena(lead=lead, q=q, a=a, top=(N, 1, 1, 1))
    assert A["q"].data_ptr() % 16 == 8 * lead and A["a"].data_ptr() % 16 == 8 * lead
    capi.simcross_forward_f64(1, A["q"], A["a"], A["top"])
    A.check()
    gm.assert_bits(A.host("top"), top_o, "top D %d lead %d" % (D, lead))
