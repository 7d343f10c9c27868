"""CPU side of tests/test_gpu_triplet_simmatrix_fused.py: the preconditions of its exact probe and of its dense test, checked
without a GPU (the GPU tests assert the same things again through the functions they share with this file)."""
import numpy as np

import test_gpu_triplet_simmatrix_fused as tf
from test_gpu_triplet_simmatrix_fused import CASES, SHAPES, exact_expected, exact_problem


def test_exact_problem_covers_every_edge(oracle):
    """Every case sits in the first panel, in an
    interior one and in the last rows; all 64 row positions of a panel are planted; the two hinge modes expect different gradients
    exactly on the rows with ordered == 0, of which every shape has some in each of those places."""
    for shape in SHAPES:
        N = shape[0]
        pr = exact_problem(shape)
        plan = pr["plan"]
        panels = (N + 63) // 64
        where = {"first": range(0, 64), "interior": range(64 * (panels // 2), 64 * (panels // 2) + 64), "last": range(64 * (N // 64 - 1), N)}
        for name, rows in where.items():
            assert {plan[i] for i in rows} == set(range(len(CASES))), "%s panel of %s lacks a case" % (name, shape)
        assert {i % 64 for i in plan} == set(range(64))
        if N % 64:
            assert plan[64 * (N // 64)] == 0, "the ragged panel's first row is the `ordered == 0` case"
        e_cpu, d_cpu = exact_expected(pr, oracle, "cpu")
        e_gpu, d_gpu = exact_expected(pr, oracle, "gpu")
        zero = (d_cpu["o"] == 0)[:, 0] & (pr["y"] != 0)[:, 0]
        differ = (d_cpu["gp"] != d_gpu["gp"])[:, 0]
        assert (differ == zero).all() and zero.sum() >= 9
        for name, rows in where.items():
            assert zero[list(rows)].any(), name
        for c, (label, _, _, _, kind) in enumerate(CASES):
            rows = [i for i, cc in plan.items() if cc == c]
            if "same" in kind:
                assert (e_cpu["dq"][rows] == 0).all(), label          # B is exactly zero there


def test_dense_redraw_terminates_and_is_rare():
    """Rows within 1e-4 of a decision edge are redrawn: the loop ends (it raises otherwise) and touches fewer than 1 % of the rows;
    afterwards no row is near an edge."""
    for shape in SHAPES:
        q, ap, an, y, W, P64, sp, sn, inner, redrawn = tf.dense_inputs_redrawn(shape)
        assert redrawn < 0.01 * shape[0]
        assert not tf.decisions64(sp, sn, y.astype(np.float64), tf.MARGIN_D)[3].any()
        print(shape, "rows redrawn:", redrawn)
