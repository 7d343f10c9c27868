"""tests/f64_gemm_model.py proved on the CPU: the shape lists reach every product x kernel x feature cell the launchers of
csrc/f64_paths.hip can produce, every probe chain stays an exact integer below 2^53, the int64 reference is the double CPU
oracle's result bit for bit, and the double oracle itself lies within the derived gamma_n bar on dense data."""
import numpy as np
import pytest

import f64_gemm_model as gm

# the oracle's products are scalar loops: the shapes it is run on here stay below 3e8 multiply-adds per call
def _bil_work(s):
    N, M, W1, W2, D = s
    return N * M * (2 * W1 * D * D + 2 * D * D * W2 + 4 * W1 * W2 * D)


def _sm_work(s):
    N, K1, K2 = s
    return 3 * N * K1 * K2


BIL_SMALL = [s for s in gm.BILINEAR if _bil_work(s) <= 300_000_000]
SM_SMALL = [s for s in gm.SIMMATRIX if _sm_work(s) <= 300_000_000]


def test_oracle_runs_on_almost_every_listed_shape():
    assert BIL_SMALL == gm.BILINEAR
    assert set(gm.SIMMATRIX) - set(SM_SMALL) == {(4096, 64, 1024), (4097, 64, 1024)}


def test_routes_named_in_the_shape_lists():
    """The routes the shape lists were chosen for, read off the model."""
    def r(call, shape, product):
        return next(x for x in gm.routes(call, shape, bias=True) if x["product"] == product)
    s = (1, 2, 3, 5, 1028)
    assert r("simcross_forward", s, "bil_QW")["kernel"] == r("simcross_forward", s, "bil_top")["kernel"] == "tallk"
    assert r("simcross_forward", s, "bil_top")["bias"] and r("simcross_backward", s, "bil_t2")["kernel"] == "tallk"
    s = (1, 2, 1030, 520, 6)
    t1, da, dq, dW = (r("simcross_backward", s, "bil_" + k) for k in ("t1", "da", "dq", "dW"))
    assert t1["kernel"] == "tallk" and not t1["a_kfast"]
    assert da["kernel"] == dq["kernel"] == "tallk" and da["seg"] and dq["seg"] and not da["a_kfast"]
    assert dW["kernel"] == "tiled" and not dW["seg"]
    s = (3, 2, 5, 7, 1028)
    assert r("simcross_forward", s, "bil_QW")["kernel"] == "tiled" and r("simcross_forward", s, "bil_top")["kernel"] == "tallk"
    s = (70, 1030, 1100)
    assert r("simmatrix_forward", s, "sm_fwd")["kernel"] == "tallk"
    assert [x["kernel"] for x in gm.routes("simmatrix_backward", s)] == ["tiled", "tallk", "tallk"]
    # the two sides of both thresholds
    assert r("simmatrix_backward", (1023, 8, 8), "sm_dW")["kernel"] == "tiled"
    assert r("simmatrix_backward", (1024, 8, 8), "sm_dW")["kernel"] == "tallk"
    assert r("simmatrix_backward", (4096, 64, 1024), "sm_dq")["kernel"] == "tallk"
    assert r("simmatrix_backward", (4097, 64, 1024), "sm_dq")["kernel"] == "tiled"
    # L below one MFMA k-step
    assert {r("simcross_backward", s, "bil_dq")["L"] for s in gm.BILINEAR} >= {1}
    assert {x["L"] for s in gm.BILINEAR for x in gm.routes("simcross_backward", s) + gm.routes("simcross_forward", s)} >= {1, 2, 3}


def test_every_reachable_cell_is_hit():
    """Every product reaches every kernel, and on each kernel every value of every feature its launcher can produce there."""
    seen = gm.all_routes()
    missing = []
    for product, kernels in gm.REQUIRED.items():
        for kernel, feats in kernels.items():
            rows = [x for x in seen if x["product"] == product and x["kernel"] == kernel]
            if not rows:
                missing.append((product, kernel))
            for f, values in feats.items():
                for v in values:
                    if not any(x[f] == v for x in rows):
                        missing.append((product, kernel, f, v))
    for kernel, feats in gm.REQUIRED_TILES.items():
        rows = [x for x in seen if x["kernel"] == kernel]
        for f, values in feats.items():
            for v in values:
                if not any(x[f] == v for x in rows):
                    missing.append((kernel, f, v))
    assert not missing, missing
    # every feature of the parameter block is seen on BOTH kernels by some product
    for f in ("a_kfast", "b_nfast", "seg", "nb0", "nb1", "kscale", "rowscale", "bias", "beta"):
        for kernel in ("tiled", "tallk"):
            for v in (True, False):
                assert any(x["kernel"] == kernel and x[f] == v for x in seen), (f, kernel, v)
    # segmented K together with a batch, and a straddled segment boundary, on tallk
    assert any(x["kernel"] == "tallk" and x["seg"] and x["nb0"] for x in seen)
    assert any(x["straddle"] for x in seen) and any(x["kernel"] == "tallk" and x["seg"] and not x["straddle"] for x in seen)


def test_slicing_restated():
    """One launch up to 65535 batches or row tiles; 65538 = 3 x 21846 falls into two slices of unequal size; the route of a
    product does not depend on it."""
    top = gm.routes("simcross_forward", (13107, 5, 2, 1, 3))[1]
    assert top["launches"] == 1 and top["n_b0"] * top["n_b1"] == 65535
    sl = gm.slices(1, 21846, 3, 64)
    assert [(b, nb) for b, nb, _, _ in sl] == [(0, 21845), (21845, 1)]
    assert all(x["launches"] == 2 for x in gm.routes("simcross_forward", (21846, 3, 1, 1, 4)))
    N = 64 * 65535 + 65
    fwd = gm.routes("simmatrix_forward", (N, 2, 2))[0]
    assert fwd["kernel"] == "tiled" and fwd["launches"] == 2
    assert gm.slices(N, 1, 1, 64) == [(0, 1, 0, 64 * 65535), (0, 1, 64 * 65535, 65)]
    dW = gm.routes("simmatrix_backward", (N, 2, 2))[0]
    assert dW["kernel"] == "tallk" and dW["launches"] == 1
    for s in gm.BILINEAR + gm.BILINEAR_DENSE:
        assert all(x["launches"] == 1 for x in gm.routes("simcross_backward", s))


@pytest.mark.parametrize("shape", gm.BILINEAR + gm.BILINEAR_LARGE, ids=gm.shape_id)
def test_bilinear_probe_chains_stay_below_2_53(shape):
    bound = gm.bilinear_bound(shape)
    print("%s: bound 2^%.1f" % (shape, np.log2(bound)))
    assert bound < 2 ** 53
    if shape in gm.BILINEAR_LARGE:
        return
    p = gm.bilinear_probe(shape)
    assert all(np.abs(v).max() <= gm.B for v in p.values())
    for k in ("W", "bias", "dT", "dbias_in"):
        assert (p[k] != 0).all()
    N, M, W1, W2, D = shape
    nzq, nza = (p["q"] != 0).sum(-1).ravel(), (p["a"] != 0).sum(-1).ravel()
    assert set(np.unique(nzq)) <= {1, D} and set(np.unique(nza)) <= {1, D}
    if N * W1 > 2 and D > 1:
        assert (nzq == 1).any() and (nzq == D).any()
    _, ref = gm.probe_case("bilinear", shape)
    for (name, b), v in ref.items():
        assert v.dtype == np.int64 and int(np.abs(v).max()) <= bound, name
    if D >= 50:
        assert int(np.abs(ref[("top", True)]).max()) > 2 ** 30 and (ref[("top", True)] % 2 == 1).any()


@pytest.mark.parametrize("shape", gm.SIMMATRIX + gm.SIMMATRIX_LARGE, ids=gm.shape_id)
def test_simmatrix_probe_chains_stay_below_2_53(shape):
    bound = gm.simmatrix_bound(shape)
    print("%s: bound 2^%.1f" % (shape, np.log2(bound)))
    assert bound < 2 ** 53
    if shape in gm.SIMMATRIX_LARGE or shape not in SM_SMALL:
        return
    _, ref = gm.probe_case("simmatrix", shape)
    for (name, _b), v in ref.items():
        assert v.dtype == np.int64 and int(np.abs(v).max()) <= bound, name
    if shape[0] >= 37:                                          # beyond what an fp32 accumulator holds, with odd low bits
        big = np.concatenate([v.ravel() for v in ref.values()])
        assert ((np.abs(big) > 2 ** 24) & (big % 2 == 1)).any()
    if shape[1] * shape[2] >= 2 ** 13:
        assert int(np.abs(ref[("top", False)]).max()) > 2 ** 30


@pytest.mark.parametrize("shape", BIL_SMALL, ids=gm.shape_id)
def test_oracle_is_the_integer_reference_bilinear(shape, oracle):
    p, ref = gm.probe_case("bilinear", shape)
    for b in (False, True):
        top, _, _ = oracle.simcross_forward(2, p["q"], p["a"], p["W"], p["bias"] if b else None)
        gm.assert_bits(top, ref[("top", b)], "top %s bias %d" % (shape, b))
        dq, da, dW, db = oracle.simcross_backward(2, p["q"], p["a"], top, p["dT"], W=p["W"], bias_term=b,
                                                  dbias_in=p["dbias_in"] if b else None)
        for name, got in (("dq", dq), ("da", da), ("dW", dW)) + ((("dbias", db),) if b else ()):
            gm.assert_bits(got, ref[(name, b)], "%s %s bias %d" % (name, shape, b))


@pytest.mark.parametrize("shape", SM_SMALL, ids=gm.shape_id)
def test_oracle_is_the_integer_reference_simmatrix(shape, oracle):
    p, ref = gm.probe_case("simmatrix", shape)
    top, scr = oracle.simmatrix_forward(p["q"], p["a"], p["W"])
    dq, da, dW = oracle.simmatrix_backward(p["q"], p["a"], p["W"], p["dT"], dW_in=p["dW_in"])
    for name, got in (("top", top), ("scratch", scr), ("dq", dq), ("da", da), ("dW", dW)):
        gm.assert_bits(got, ref[(name, False)], "%s %s" % (name, shape))


def test_a_wrong_element_or_a_narrower_type_changes_the_bits():
    """What the probes are for: one dropped term, or one pass through fp32, is visible in the bits of an output."""
    p, ref = gm.probe_case("simmatrix", (37, 24, 19))
    want = ref[("scratch", False)].astype(np.float64)
    q2 = p["q"].copy()
    q2[4, 23] = 0                                               # row 4 is dense
    assert (np.matmul(q2, p["W"]) != want)[4].all() and (np.matmul(q2, p["W"]) == want)[:4].all()
    for name in ("top", "dq", "da", "dW"):                      # three factors each: beyond 2^24 with odd low bits
        v = ref[(name, False)].astype(np.float64)
        assert (v.astype(np.float32).astype(np.float64) != v).any(), name


@pytest.mark.parametrize("shape", gm.BILINEAR_DENSE, ids=gm.shape_id)
def test_double_oracle_within_the_derived_bar_bilinear(shape, oracle):
    v, E, S = gm.dense_case("bilinear", shape)
    n = gm.bilinear_n(shape, True)
    top, _, _ = oracle.simcross_forward(2, v["q"], v["a"], v["W"], v["bias"])
    dq, da, dW, db = oracle.simcross_backward(2, v["q"], v["a"], top, v["dT"], W=v["W"], bias_term=True, dbias_in=v["dbias_in"])
    for name, got in (("top", top), ("dq", dq), ("da", da), ("dW", dW), ("dbias", db)):
        gm.check_dense("oracle %s %s" % (name, shape), got, *E[name], S[name], n[name])


@pytest.mark.parametrize("shape", gm.SIMMATRIX_DENSE, ids=gm.shape_id)
def test_double_oracle_within_the_derived_bar_simmatrix(shape, oracle):
    v, E, S = gm.dense_case("simmatrix", shape)
    n = gm.simmatrix_n(shape)
    top, scr = oracle.simmatrix_forward(v["q"], v["a"], v["W"])
    dq, da, dW = oracle.simmatrix_backward(v["q"], v["a"], v["W"], v["dT"], dW_in=v["dW_in"])
    for name, got in (("top", top), ("scratch", scr), ("dq", dq), ("da", da), ("dW", dW)):
        gm.check_dense("oracle %s %s" % (name, shape), got, *E[name], S[name], n[name])


def test_dense_check_is_exact_and_tight():
    """dense_error resolves a unit in the last place of a value beyond 2^53 2^-s, and the longest chain's bar is a quarter of 1e-12
    of the sum of the absolute values of an element's own terms."""
    E = np.array([(1 << 70) + 12345, -(1 << 40) + 1, 0], dtype=object)
    got = np.array([float((1 << 70) + 12345) * 2.0 ** -60, (-(1 << 40) + 1) * 2.0 ** -60, 0.0])
    err = gm.dense_error(got, E, 60)
    assert err[1] == 0 and err[2] == 0 and 0 < err[0] <= 2.0 ** 17 * 2.0 ** -60
    assert gm.dense_error(np.nextafter(got, np.inf), E, 60)[1] == np.nextafter(got[1], np.inf) - got[1]
    assert gm.gamma(2 * 1030 + 2) < 2.3e-13                     # the longest chain of the dense shapes, relative to S
