"""GPU suite: mms_solver_step_f32 / _f64 (include/mms_solver.h) against the numpy model of tests/solver_reference.py.

The comparison is word-for-word equality of data, diff, hist_grad and hist_update: the model rounds once per line of
the header's table and so does the kernel.  The one tolerance of the file is the bar on the gradient norm of dense
data, gamma(n + 2) |g|: n - 1 additions and one rounded square per element is gamma(n) on the sum of squares in any
order, the square root halves it and adds one rounding.

Shapes come from the header's constants (solver.CHUNK, solver.BLOBS_PER_LAUNCH): around one chunk, several chunks, and
one blob more than a launch takes.  Every array sits between guard zones, at a 16-byte aligned address or one element
past it (the scalar path)."""
import fractions
import math

import numpy as np
import pytest
import torch

import solver_reference as R

pytestmark = pytest.mark.gpu

GUARD = 8                                  # elements on either side of every array: 32 or 64 bytes, so 16-byte aligned
SENTINEL = 7.25
DTYPES = [np.float32, np.float64]
TYPES = [R.ADADELTA, R.SGD]
HYPER = {R.ADADELTA: dict(momentum=0.95, delta=5e-7, weight_decay=5e-4),      # do_trec_qa_clean.py:322-348
         R.SGD: dict(momentum=0.9, weight_decay=5e-4)}
RATE = {R.ADADELTA: 1.0, R.SGD: 0.01}


@pytest.fixture(scope="module")
def solver(hiplib):
    from mms_answer_selection_amd import solver
    solver.lib()
    return solver


def counts_of(solver):
    c = solver.CHUNK
    return [1, 2, 3, 4, 5, 7, c - 1, c, c + 1, 3 * c + 7]


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_words(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def make_blobs(dt, counts, seed, ada, lr_mults=None, decay_mults=None):
    rng = np.random.default_rng(seed)
    out = []
    for k, n in enumerate(counts):
        w, g = rng.standard_normal(n).astype(dt), rng.standard_normal(n).astype(dt)
        h, h2 = np.abs(rng.standard_normal(n)).astype(dt), np.abs(rng.standard_normal(n)).astype(dt) * dt(1e-3)
        if n >= 3:                                  # zeros and +-0 in g; a parameter at +-0 (L1's sign)
            g[n // 2], g[n - 1], w[0], w[n // 3] = dt(0.0), dt(-0.0), dt(-0.0), dt(0.0)
        if n >= 7:                                  # an element that has never moved
            g[1], h[1], h2[1] = dt(0.0), dt(0.0), dt(0.0)
        out.append(R.Blob(w, g, h, h2 if ada else None,
                          1.0 if lr_mults is None else lr_mults[k % len(lr_mults)],
                          1.0 if decay_mults is None else decay_mults[k % len(decay_mults)]))
    return out


class Device:
    """The blobs on the device, every array between guard zones; offset: elements past the aligned address."""

    def __init__(self, solver, blobs, offset=0):
        self.solver, self.n, self.bufs, entries = solver, [len(b.w) for b in blobs], [], []
        for b in blobs:
            views = []
            for a in (b.w, b.g, b.h, b.h2):
                if a is None:
                    views.append(None)
                    self.bufs.append(None)
                    continue
                host = np.full(GUARD + offset + len(a) + GUARD, SENTINEL, a.dtype)
                host[GUARD + offset:GUARD + offset + len(a)] = a
                buf = torch.from_numpy(host).cuda()
                assert buf.data_ptr() % 16 == 0
                self.bufs.append(buf)
                views.append(buf[GUARD + offset:GUARD + offset + len(a)])
            entries.append(tuple(views) + (b.lr_mult, b.decay_mult))
        self.lo = GUARD + offset
        self.blobs = solver.solver_blobs(entries)
        self.like = blobs

    def read(self):
        """-> the blobs as they are now; asserts every guard zone"""
        torch.cuda.synchronize()
        out, it = [], iter(self.bufs)
        for b, n in zip(self.like, self.n):
            arrays = []
            for _ in range(4):
                buf = next(it)
                if buf is None:
                    arrays.append(None)
                    continue
                host = buf.cpu().numpy()
                assert (host[:self.lo] == SENTINEL).all() and (host[self.lo + n:] == SENTINEL).all(), "guard zone"
                arrays.append(host[self.lo:self.lo + n].copy())
            out.append(R.Blob(*arrays, b.lr_mult, b.decay_mult))
        return out


def stepper(solver, dt):
    return solver.solver_step if dt == np.float32 else solver.solver_step_f64


def assert_blobs(got, want, what):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        for name in ("w", "g", "h", "h2"):
            x, y = getattr(a, name), getattr(b, name)
            assert (x is None) == (y is None), (what, k, name)
            if x is not None:
                assert same_words(x, y), (what, k, name, len(x), int((bits(x) != bits(y)).sum()))


def run(solver, dt, p, blobs, rate, offset=0, **kw):
    dev = Device(solver, blobs, offset)
    stepper(solver, dt)(solver.solver_param(**p._asdict()), dev.blobs, rate, **kw)
    return dev.read()


def configs(t):
    for reg in (R.L2, R.L1):
        for iter_size in (1, 3):
            for diff_out in (R.DIFF_UPDATE, R.DIFF_ZERO):
                yield R.param(t, reg, iter_size, diff_out, **HYPER[t])


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("dt", DTYPES)
def test_one_call_over_every_count_and_a_count_zero_blob(solver, dt, t):
    """All counts in one launch with an empty blob among them; lr_mult 0 and 1, decay_mult 0 next to 1; every
    regularization, iter_size and diff_out; the aligned and the scalar path give the model's words."""
    counts = counts_of(solver)
    counts.insert(4, 0)
    blobs = make_blobs(dt, counts, 1, t == R.ADADELTA, lr_mults=[1.0, 0.0, 0.5], decay_mults=[1.0, 0.0])
    for p in configs(t):
        want, _, _ = R.step(dt, p, blobs, RATE[t])
        for offset in (0, 1):
            assert_blobs(run(solver, dt, p, blobs, RATE[t], offset), want, (p, offset))


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("dt", DTYPES)
def test_each_count_alone(solver, dt, t):
    p = R.param(t, **HYPER[t])
    for n in counts_of(solver):
        blobs = make_blobs(dt, [n], 100 + n, t == R.ADADELTA)
        want, _, _ = R.step(dt, p, blobs, RATE[t])
        for offset in (0, 1):
            assert_blobs(run(solver, dt, p, blobs, RATE[t], offset), want, (n, offset))


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("dt", DTYPES)
def test_one_blob_more_than_a_launch_takes(solver, dt, t):
    counts = [1 + k % 7 for k in range(solver.BLOBS_PER_LAUNCH + 1)]
    counts[3] = 0                                                     # skipped blobs do not count towards a launch
    counts.append(9)
    blobs = make_blobs(dt, counts, 2, t == R.ADADELTA, lr_mults=[1.0, 2.0], decay_mults=[1.0, 0.0, 1.0])
    p = R.param(t, R.L2, 1, R.DIFF_ZERO, **HYPER[t])
    want, _, _ = R.step(dt, p, blobs, RATE[t])
    for offset in (0, 1):
        assert_blobs(run(solver, dt, p, blobs, RATE[t], offset), want, offset)


@pytest.mark.parametrize("dt", DTYPES)
def test_lr_mult_zero_moves_the_histories_only(solver, dt):
    blobs = make_blobs(dt, [solver.CHUNK + 5, 6], 3, True, lr_mults=[0.0])
    for b in blobs:
        b.w[b.w == 0] = dt(1.5)        # a parameter at -0 minus an update of -0 is +0 in IEEE arithmetic: another word
    p = R.param(R.ADADELTA, **HYPER[R.ADADELTA])
    got = run(solver, dt, p, blobs, 1.0)
    assert_blobs(got, R.step(dt, p, blobs, 1.0)[0], "lr_mult 0")
    for a, b in zip(got, blobs):
        assert same_words(a.w, b.w)
        assert (a.h != b.h).sum() > len(b.h) // 2 and (a.h2 != b.h2).sum() > len(b.h2) // 2


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("dt", DTYPES)
def test_two_consecutive_steps_carry_the_state_in_the_tensors(solver, dt, t):
    blobs = make_blobs(dt, [5, solver.CHUNK + 1, 2], 4, t == R.ADADELTA, decay_mults=[1.0, 0.0])
    p = R.param(t, **HYPER[t])
    dev = Device(solver, blobs)
    sp = solver.solver_param(**p._asdict())
    rng = np.random.default_rng(44)
    fresh = [rng.standard_normal(len(b.w)).astype(dt) for b in blobs]     # the second backward's gradients
    stepper(solver, dt)(sp, dev.blobs, RATE[t])
    for k, g in enumerate(fresh):
        dev.bufs[4 * k + 1][dev.lo:dev.lo + len(g)].copy_(torch.from_numpy(g))
    stepper(solver, dt)(sp, dev.blobs, RATE[t] / 2)
    mid, _, _ = R.step(dt, p, blobs, RATE[t])
    for b, g in zip(mid, fresh):
        b.g = g
    want, _, _ = R.step(dt, p, mid, RATE[t] / 2)
    assert_blobs(dev.read(), want, "two steps")


def _dyadic(dt, solver, ada):
    """Diffs that are small integers / 8 and whose sum of squares is S^2 / 64 for an integer S: every partial sum is
    exact in either element type and the norm is S / 8."""
    c = solver.CHUNK
    blobs = make_blobs(dt, [5, c + 1, 3 * c + 7], 5, ada, decay_mults=[1.0, 0.0])
    rng = np.random.default_rng(55)
    total = 0
    for b in blobs:
        ints = rng.integers(-3, 4, size=len(b.g))
        total += int((ints * ints).sum())
        b.g = (ints / 8.0).astype(dt)
    S = math.isqrt(total) + 1
    fix = S * S - total                                               # 1 .. 2 S
    last = make_blobs(dt, [fix], 6, ada)[0]
    last.g = np.where(np.arange(fix) % 2 == 0, 0.125, -0.125).astype(dt)
    assert S * S < 2 ** 24 and fix > 0
    return blobs + [last], S / 8.0


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("dt", DTYPES)
def test_clipping_on_dyadic_probes_is_exact(solver, dt, t):
    blobs, norm = _dyadic(dt, solver, t == R.ADADELTA)
    # above the threshold (scale exactly 1/2, and one that rounds), below it, and equal: `>` does not clip
    for clip, scale in ((norm / 2, dt(0.5)), (1.0, dt(dt(1.0) / dt(norm))), (2 * norm, dt(1)), (norm, dt(1))):
        assert float(np.float32(clip)) == clip
        p = R.param(t, clip_gradients=clip, **HYPER[t])
        want, mnorm, mscale = R.step(dt, p, blobs, RATE[t])
        assert mnorm == dt(norm) and same_words(np.array([mscale]), np.array([scale]))
        for offset in (0, 1):
            info = torch.full((2,), float("nan"), dtype=torch.from_numpy(np.zeros(1, dt)).dtype, device="cuda")
            got = run(solver, dt, p, blobs, RATE[t], offset, clip_info=info)
            assert same_words(info.cpu().numpy(), np.array([norm, scale], dt)), (clip, offset)
            assert_blobs(got, want, (clip, offset))


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("dt", DTYPES)
def test_clipping_over_more_blobs_than_a_launch_takes(solver, dt, t):
    """The norm's running sum crosses from the first table's launches to the second's through the workspace, and the
    second table's chunk sums lie behind the first's: BLOBS_PER_LAUNCH + 1 non-empty blobs (one of two chunks, an empty
    one among them), dyadic diffs with sum of squares S^2 / 64, a workspace full of NaN, both alignments."""
    from mms_answer_selection_amd import capi
    ada = t == R.ADADELTA
    counts = [1 + k % 7 for k in range(solver.BLOBS_PER_LAUNCH)]
    counts[2] = solver.CHUNK + 3
    counts.insert(5, 0)
    blobs = make_blobs(dt, counts, 9, ada, lr_mults=[1.0, 0.5], decay_mults=[1.0, 0.0])
    rng = np.random.default_rng(99)
    total = 0
    for b in blobs:
        ints = rng.integers(-3, 4, size=len(b.g))
        total += int((ints * ints).sum())
        b.g = (ints / 8.0).astype(dt)
    S = math.isqrt(total) + 1
    last = make_blobs(dt, [S * S - total], 10, ada)[0]                # the blob of the second table
    last.g = np.where(np.arange(len(last.g)) % 2 == 0, 0.125, -0.125).astype(dt)
    blobs.append(last)
    assert sum(1 for b in blobs if len(b.g)) == solver.BLOBS_PER_LAUNCH + 1 and len(last.g) > 0
    norm = S / 8.0
    tdt = torch.float32 if dt == np.float32 else torch.float64
    for clip, scale in ((norm / 2, dt(0.5)), (norm, dt(1))):
        p = R.param(t, clip_gradients=clip, **HYPER[t])
        want, mnorm, mscale = R.step(dt, p, blobs, RATE[t])
        assert mnorm == dt(norm) and mscale == scale
        for offset in (0, 1):
            dev = Device(solver, blobs, offset)
            sp = solver.solver_param(**p._asdict())
            need = (solver.solver_workspace_bytes if dt == np.float32 else solver.solver_workspace_bytes_f64)(
                sp, dev.blobs)
            ws = capi.Workspace()
            ws.get(need, dev.blobs.device)
            ws.buf.view(tdt).fill_(float("nan"))
            info = torch.full((2,), float("nan"), dtype=tdt, device="cuda")
            stepper(solver, dt)(sp, dev.blobs, RATE[t], clip_info=info, ws=ws)
            assert same_words(info.cpu().numpy(), np.array([norm, scale], dt)), (clip, offset)
            assert_blobs(dev.read(), want, (clip, offset))


def test_the_binding_refuses_device_tensors_that_do_not_fit(solver):
    from mms_answer_selection_amd import capi
    z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device="cuda")
    for bad in ((z(4), z(4, torch.float64), z(4), z(4)),             # diff of another dtype
                (z(4), z(4), z(4, torch.float16), z(4)),
                (z(4), z(5), z(4), z(4)),                            # unequal sizes
                (z(4), z(4), z(4), z(3)),
                (z(4), z(8)[::2], z(4), z(4)),                       # not contiguous
                (z(8)[::2], z(4), z(4), z(4)),
                (z(4), z(4).cpu(), z(4), z(4)),                      # host memory
                (z(4, torch.float16), z(4, torch.float16), z(4, torch.float16), None)):
        with pytest.raises(capi.MMSArgumentError):
            solver.solver_blobs([(z(4), z(4), z(4), z(4), 1.0, 1.0), bad + (1.0, 1.0)])
    with pytest.raises(capi.MMSArgumentError):                       # the second blob's dtype is not the first's
        solver.solver_blobs([(z(4), z(4), z(4), z(4), 1.0, 1.0),
                             tuple(z(4, torch.float64) for _ in range(4)) + (1.0, 1.0)])
    blobs = solver.solver_blobs([(z(4), z(4), z(4), z(4), 1.0, 1.0)])
    p = solver.solver_param(clip_gradients=1.0)
    with pytest.raises(capi.MMSArgumentError):
        solver.solver_step_f64(p, blobs, 1.0)                        # float blobs at the double call
    for info in (z(3), z(2, torch.float64), z(4)[::2], z(2).cpu()):
        with pytest.raises(capi.MMSArgumentError):
            solver.solver_step(p, blobs, 1.0, clip_info=info)
    solver.solver_step(p, blobs, 1.0, clip_info=z(2))                # and what fits is taken
    torch.cuda.synchronize()


def _exact_norm(blobs):
    total = fractions.Fraction(0)
    for b in blobs:
        total += sum(fractions.Fraction(float(x)) ** 2 for x in b.g)
    return math.sqrt(total)                                           # correctly rounded to double, then one sqrt


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("dt", DTYPES)
def test_clipping_on_dense_data_and_determinism(solver, dt, t):
    from mms_answer_selection_amd import capi
    c = solver.CHUNK
    blobs = make_blobs(dt, [3, c - 1, 0, 2 * c + 9, 4], 7, t == R.ADADELTA, decay_mults=[1.0, 0.0])
    n = sum(len(b.g) for b in blobs)
    exact = _exact_norm(blobs)
    u = 2.0 ** -24 if dt == np.float32 else 2.0 ** -53
    bar = (n + 2) * u / (1 - (n + 2) * u) * exact
    tdt = torch.float32 if dt == np.float32 else torch.float64
    for factor in (0.5, 2.0):                                         # the norm is 100 % / 50 % away from the threshold
        clip = float(np.float32(exact * factor))
        assert abs(clip - exact) > 0.01 * exact
        p = R.param(t, clip_gradients=clip, **HYPER[t])
        sp = solver.solver_param(**p._asdict())
        info = torch.zeros(2, dtype=tdt, device="cuda")
        got = run(solver, dt, p, blobs, RATE[t], 0, clip_info=info)
        norm, scale = info.cpu().numpy()
        print("dense clip: dtype %s n %d exact %.17g returned %.17g |diff| %.3g bar %.3g scale %.17g"
              % (np.dtype(dt).name, n, exact, norm, abs(float(norm) - exact), bar, scale))
        assert abs(float(norm) - exact) <= bar
        assert same_words(np.array([scale]), np.array([R.clip_scale(dt, norm, clip)]))
        assert (scale < 1) == (factor < 1)
        want, _, _ = R.step(dt, p, blobs, RATE[t], scale=scale)
        assert_blobs(got, want, factor)
        # the same words from a workspace full of NaN, from shifted arrays, and without clip_info
        ws = capi.Workspace()
        need = (solver.solver_workspace_bytes if dt == np.float32 else solver.solver_workspace_bytes_f64)(
            sp, Device(solver, blobs).blobs)
        assert need > 0
        ws.get(need, torch.device("cuda", torch.cuda.current_device()))
        ws.buf.view(tdt).fill_(float("nan"))
        info2 = torch.zeros(2, dtype=tdt, device="cuda")
        assert_blobs(run(solver, dt, p, blobs, RATE[t], 1, clip_info=info2, ws=ws), want, "shifted, NaN workspace")
        assert same_words(info2.cpu().numpy(), info.cpu().numpy())
        assert_blobs(run(solver, dt, p, blobs, RATE[t], 0), want, "no clip_info")


@pytest.mark.parametrize("dt", DTYPES)
def test_a_refused_call_writes_nothing(solver, dt):
    import ctypes as C
    from mms_answer_selection_amd import capi
    blobs = make_blobs(dt, [9, solver.CHUNK + 3], 8, True)
    step = stepper(solver, dt)
    name = "mms_solver_step_f32" if dt == np.float32 else "mms_solver_step_f64"

    def untouched(dev):
        assert_blobs(dev.read(), blobs, "refused")

    dev = Device(solver, blobs)
    for bad in (dict(type=3), dict(iter_size=0), dict(regularization=7), dict(diff_out=5)):
        with pytest.raises(capi.MMSError):
            step(solver.solver_param(**dict(HYPER[R.ADADELTA], **bad)), dev.blobs, 1.0)
        untouched(dev)
    # clipping without a workspace, straight at the library (the binding would bring one)
    sp = solver.solver_param(clip_gradients=1.0, **HYPER[R.ADADELTA])
    rc = getattr(solver.lib(), name)(C.byref(sp), dev.blobs.array, len(dev.blobs), 1.0, None, None, 0, None)
    assert rc == 3
    untouched(dev)
    # the second blob's diff is the first blob's data; then a NULL hist_update for AdaDelta
    keep = dev.blobs.array[1].diff
    dev.blobs.array[1].diff = dev.blobs.array[0].data
    with pytest.raises(capi.MMSError):
        step(solver.solver_param(**HYPER[R.ADADELTA]), dev.blobs, 1.0)
    dev.blobs.array[1].diff = keep
    keep = dev.blobs.array[0].hist_update
    dev.blobs.array[0].hist_update = None
    with pytest.raises(capi.MMSError):
        step(solver.solver_param(**HYPER[R.ADADELTA]), dev.blobs, 1.0)
    dev.blobs.array[0].hist_update = keep
    untouched(dev)
    # the same table is good once it is whole again
    step(solver.solver_param(**HYPER[R.ADADELTA]), dev.blobs, 1.0)
    assert_blobs(dev.read(), R.step(dt, R.param(R.ADADELTA, **HYPER[R.ADADELTA]), blobs, 1.0)[0], "after refusals")
    # and SGD takes a table with a hist_update NULL, leaving the other blob's hist_update alone (on arrays of its own:
    # a momentum buffer is signed and no E[g^2] for AdaDelta)
    sgd = Device(solver, blobs)
    sgd.blobs.array[0].hist_update = None
    step(solver.solver_param(type=R.SGD, **HYPER[R.SGD]), sgd.blobs, 0.01)
    assert_blobs(sgd.read(), R.step(dt, R.param(R.SGD, **HYPER[R.SGD]), blobs, 0.01)[0], "SGD with a NULL hist_update")
