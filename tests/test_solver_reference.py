"""CPU suite: the numpy model of the solver update (tests/solver_reference.py) is pinned by torch.optim on the CPU in
float64, and its branches (clip, L1, iter_size, lr_mult = 0, DIFF_ZERO) by direct formulas.

torch's Adadelta and the reference's are the same formula up to rounding: torch takes sqrt(a) / sqrt(b) where the
reference takes sqrt(a / b), groups (1 - rho) * g * g from the left, and may fuse a product into a sum.  So the bound is
not a chosen number but the count of roundings on either path, all data being POSITIVE so that no sum cancels and
relative errors simply add (sqrt halves one).  With u = 2^-53, per step and from the same state, relative to the exact
value, each path stays within:

    g' = g + wd w                       2u
    h' = om g'^2 + m h                  g'^2: 2 * 2u + u; om: + u; m h: u; the sum: + u          ->  7u
    delta                               ours:  (h2 + d) / (h' + d): u + 8u + u, sqrt: 5u + u, times g': + 2u + u  ->  9u
                                        torch: sqrt(h' + d): 4u + u, sqrt(h2 + d): u / 2 + u, /: + u, times g'   -> 10.5u
    h2' = om delta^2 + m h2             2 * 10.5u + u, om: + u, the sum: + u                     -> 24u
    w'  = w - lr delta                  (10.5u + u) |lr delta| + u |w'|

The two paths differ by at most the sum of their bounds; gamma(k) = k u / (1 - k u) covers the second-order terms.
"""
import numpy as np
import pytest
import torch

import solver_reference as R

U = 2.0 ** -53


def gamma(k):
    return k * U / (1 - k * U)


# dyadic hyper-parameters: they are float fields of the proto, and torch takes them as doubles
RHO, EPS, WD, LR = 0.9375, 2.0 ** -20, 2.0 ** -11, 0.5
SHAPES = [(1,), (7,), (3, 5), (4, 50, 50)]


def _positive(rng, shape, lo, hi):
    return rng.uniform(lo, hi, size=shape)


def _blobs_of(params, state_of, ada):
    out = []
    for p in params:
        s = state_of(p)
        out.append(R.Blob(p.detach().numpy().reshape(-1).copy(), p.grad.numpy().reshape(-1).copy(), s[0], s[1] if ada else None))
    return out


def test_adadelta_is_torch_adadelta_within_the_operation_count():
    rng = np.random.default_rng(11)
    params = [torch.tensor(_positive(rng, s, 0.5, 2.0), requires_grad=True) for s in SHAPES]
    opt = torch.optim.Adadelta(params, lr=LR, rho=RHO, eps=EPS, weight_decay=WD, foreach=False)
    p = R.param(R.ADADELTA, momentum=RHO, delta=EPS, weight_decay=WD)
    for it in range(3):
        for q in params:
            q.grad = torch.tensor(_positive(rng, tuple(q.shape), 0.01, 1.0))

        def state(q):
            s = opt.state.get(q, {})
            if "square_avg" not in s:
                return np.zeros(q.numel()), np.zeros(q.numel())
            return s["square_avg"].numpy().reshape(-1).copy(), s["acc_delta"].numpy().reshape(-1).copy()
        before = _blobs_of(params, state, True)
        model, _, _ = R.step(np.float64, p, before, LR)
        opt.step()
        for q, b in zip(params, model):
            w = q.detach().numpy().reshape(-1)
            h = opt.state[q]["square_avg"].numpy().reshape(-1)
            h2 = opt.state[q]["acc_delta"].numpy().reshape(-1)
            upd = np.abs(b.g)                                        # lr * delta: the diff holds the applied update
            assert np.all(upd > 0) and np.all(b.h > 0) and np.all(b.w > 0), it
            assert np.all(np.abs(b.h - h) <= gamma(14) * h), it
            assert np.all(np.abs(b.h2 - h2) <= gamma(48) * h2), it
            assert np.all(np.abs(b.w - w) <= gamma(21.5) * upd + gamma(2) * np.abs(w)), it


def test_sgd_is_torch_sgd_within_the_operation_count():
    """torch keeps buf with p -= lr buf, the reference h = lr buf; lr is a power of two, so the change of variable is
    exact.  g' = g + wd w: 2u; m buf: u; the sum: + u -> 3u on either path; w' = w - h': 3u |h'| + u |w'|."""
    rng = np.random.default_rng(12)
    params = [torch.tensor(_positive(rng, s, 0.5, 2.0), requires_grad=True) for s in SHAPES]
    opt = torch.optim.SGD(params, lr=LR, momentum=RHO, weight_decay=WD, foreach=False)
    p = R.param(R.SGD, momentum=RHO, weight_decay=WD)
    for it in range(3):
        for q in params:
            q.grad = torch.tensor(_positive(rng, tuple(q.shape), 0.01, 1.0))

        def state(q):
            buf = opt.state.get(q, {}).get("momentum_buffer")
            return (np.zeros(q.numel()) if buf is None else LR * buf.numpy().reshape(-1), None)
        before = _blobs_of(params, state, False)
        model, _, _ = R.step(np.float64, p, before, LR)
        opt.step()
        for q, b in zip(params, model):
            h = LR * opt.state[q]["momentum_buffer"].numpy().reshape(-1)
            w = q.detach().numpy().reshape(-1)
            assert np.all(h > 0), it
            assert np.all(np.abs(b.h - h) <= gamma(6) * h), it
            assert np.array_equal(b.g, b.h), it
            assert np.all(np.abs(b.w - w) <= gamma(6) * h + gamma(2) * np.abs(w)), it


def _one(dt, n=37, seed=5, **kw):
    rng = np.random.default_rng(seed)
    mk = lambda: rng.standard_normal(n).astype(dt)
    return R.Blob(mk(), mk(), np.abs(mk()), np.abs(mk()), **kw)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_branches_against_direct_formulas(dt):
    b = _one(dt, lr_mult=0.5, decay_mult=2.0)
    b.w[3], b.w[4] = dt(0.0), dt(-0.0)
    m, wd, rate = dt(np.float32(0.9)), dt(np.float32(5e-4)), dt(0.25)
    lr, ld = dt(rate * dt(0.5)), dt(wd * dt(2.0))
    # SGD, L1, iter_size 3
    p = R.param(R.SGD, R.L1, 3, R.DIFF_UPDATE, momentum=0.9, weight_decay=5e-4)
    (o,), norm, scale = R.step(dt, p, [b], 0.25)
    accum = dt(dt(1) / dt(3))
    sign = ((b.w > 0).astype(dt) - (b.w < 0).astype(dt))
    g = b.g * accum + ld * sign
    h = lr * g + m * b.h
    assert norm is None and scale is None
    assert np.array_equal(o.h, h) and np.array_equal(o.g, h) and np.array_equal(o.w, b.w - h)
    assert o.h2 is not None and np.array_equal(o.h2, b.h2)            # SGD leaves it alone
    # L2, iter_size 1, DIFF_ZERO
    p = R.param(R.SGD, R.L2, 1, R.DIFF_ZERO, momentum=0.9, weight_decay=5e-4)
    (o,), _, _ = R.step(dt, p, [b], 0.25)
    h = lr * (b.g + ld * b.w) + m * b.h
    assert np.array_equal(o.h, h) and np.array_equal(o.w, b.w - h)
    assert np.array_equal(o.g, np.zeros_like(b.g)) and not np.signbit(o.g).any()
    # decay_mult 0 skips the regularizer: -0 stays -0 where adding +0 would make it +0
    for decay_mult in (0.0, 1.0):
        z = R.Blob(np.zeros_like(b.w), np.full_like(b.g, -0.0), np.full_like(b.h, -0.0), None, 1.0, decay_mult)
        (o,), _, _ = R.step(dt, R.param(R.SGD, momentum=0.0, weight_decay=5e-4), [z], 1.0)
        assert np.signbit(o.h).all() == (decay_mult == 0.0) and np.signbit(o.h).any() == (decay_mult == 0.0)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_adadelta_formula_lr_mult_zero_and_clip(dt):
    m, d = dt(np.float32(0.95)), dt(np.float32(5e-7))
    om = dt(dt(1) - m)
    frozen = _one(dt, lr_mult=0.0, decay_mult=0.0)
    p = R.param(R.ADADELTA, momentum=0.95, delta=5e-7, weight_decay=5e-4)
    (o,), _, _ = R.step(dt, p, [frozen], 1.0)
    h = om * (frozen.g * frozen.g) + m * frozen.h
    dx = frozen.g * np.sqrt((d + frozen.h2) / (d + h))
    h2 = om * (dx * dx) + m * frozen.h2
    assert np.array_equal(o.h, h) and np.array_equal(o.h2, h2)        # the histories move
    assert np.array_equal(o.w, frozen.w) and not o.g.any()            # the data does not: the update is 0 * dx
    assert not np.array_equal(o.h, frozen.h) and not np.array_equal(o.h2, frozen.h2)
    # clip: diffs (3, 4) and (12,) -> norm 13; thresholds above, equal and below
    a = R.Blob(np.ones(2, dt), np.array([3, 4], dt), np.zeros(2, dt), np.zeros(2, dt))
    c = R.Blob(np.ones(1, dt), np.array([12], dt), np.zeros(1, dt), np.zeros(1, dt))
    for clip, want in ((20.0, 1.0), (13.0, 1.0), (6.5, 0.5)):
        pc = R.param(R.SGD, momentum=0.0, clip_gradients=clip)
        out, norm, scale = R.step(dt, pc, [a, c], 1.0)
        assert norm == 13 and scale == want
        assert np.array_equal(out[0].g, a.g * dt(want)) and np.array_equal(out[1].w, c.w - c.g * dt(want))
        again, _, _ = R.step(dt, pc, [a, c], 1.0, scale=scale)        # the scale handed in
        assert all(np.array_equal(x.w, y.w) for x, y in zip(out, again))
    assert R.step(dt, R.param(R.SGD), [a], 1.0)[1] is None            # clip_gradients -1: off
