"""Whose setting is it?  include/mms.h gives six arithmetic switches to the CALLING THREAD (a Caffe host drives one GPU
per thread) and one, the matrix pipe, to the process; a thread that never set the Euclidean mode takes MMS_EUCLID_BWD
from the environment.  tests/test_gpu_mode_matrix.py runs every combination on one thread, which a process-wide
variable passes just as well: these tests use two.

The getter / setter tests need no GPU (libmms_hip.so loads without one) and are not marked; the last test runs
kernels under two threads' different settings."""
import contextlib
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from util import TOL, assert_bitexact, assert_close, qa, rng

HERE = os.path.dirname(os.path.abspath(__file__))
WAIT = 120.0            # seconds; only ever runs out when something is already broken

# The six per-thread switches: (stem of mms_set_<stem>_mode / mms_get_<stem>_mode, default value).  include/mms.h:
# MMS_PAIRRANK_HINGE_CPU, MMS_LOSS_SUM_FAST, MMS_F16_DISTANCE_ORDERED, MMS_RANK_TIES_INPUT_ORDER = 0,
# MMS_TRIPLET_FINISH_INLAUNCH = 1; the Euclidean default is the process's (None here, see euclid_process_default).
PER_THREAD = [("euclid_backward", None), ("pairrank_hinge", 0), ("loss_sum", 0), ("f16_distance", 0),
              ("triplet_finish", 1), ("rank_tie", 0)]
PROCESS_WIDE = "matrix"                         # default 0 (bf16x3)


def euclid_mode_of(value):
    """csrc/simcross_rows.hip, euclid_backward_mode(): "reference", "exact" and "1" select MMS_EUCLID_BWD_REFERENCE (1),
    anything else, or no variable, MMS_EUCLID_BWD_FP32 (0)."""
    return 1 if value in ("reference", "exact", "1") else 0


def defaults():
    return [euclid_mode_of(os.environ.get("MMS_EUCLID_BWD")) if d is None else d for _, d in PER_THREAD]


def get_one(lib, stem):
    return getattr(lib, "mms_get_%s_mode" % stem)()


def set_one(lib, stem, value):
    return getattr(lib, "mms_set_%s_mode" % stem)(value)


def get_all(lib):
    return [get_one(lib, stem) for stem, _ in PER_THREAD]


def set_all(lib, values):
    for (stem, _), v in zip(PER_THREAD, values):
        assert set_one(lib, stem, v) == 0, stem


@contextlib.contextmanager
def preserved(lib):
    """The calling thread's six modes and the process's matrix mode are put back on the way out."""
    mine, matrix = get_all(lib), get_one(lib, PROCESS_WIDE)
    try:
        yield
    finally:
        set_all(lib, mine)
        set_one(lib, PROCESS_WIDE, matrix)


class Worker(threading.Thread):
    """A thread whose exception is re-raised by finish(); on an exception it sets `release`, so that nobody waits for
    a signal that will not come."""

    def __init__(self, fn, release=()):
        super().__init__()
        self.fn, self.release, self.error, self.value = fn, release, None, None

    def run(self):
        try:
            self.value = self.fn()
        except BaseException as e:      # noqa: B902 -- handed to the test thread
            self.error = e
            for ev in self.release:
                ev.set()

    def finish(self):
        self.join(WAIT)
        assert not self.is_alive(), "worker thread did not finish"
        if self.error is not None:
            raise self.error
        return self.value


def in_thread(fn):
    w = Worker(fn)
    w.start()
    return w.finish()


def test_a_fresh_thread_starts_at_the_defaults(hiplib):
    lib, want = hiplib, defaults()
    with preserved(lib):
        set_all(lib, [1 - d for d in want])
        assert get_all(lib) == [1 - d for d in want]
        assert in_thread(lambda: get_all(lib)) == want, [stem for stem, _ in PER_THREAD]


def test_a_threads_settings_are_its_own(hiplib):
    lib, base = hiplib, defaults()
    theirs = [1 - d for d in base]
    worker_has_set, main_has_set = threading.Event(), threading.Event()

    def work():
        set_all(lib, theirs)
        first = get_all(lib)
        worker_has_set.set()
        assert main_has_set.wait(WAIT)
        return first, get_all(lib)

    with preserved(lib):
        set_all(lib, base)
        w = Worker(work, release=(worker_has_set,))
        w.start()
        try:
            assert worker_has_set.wait(WAIT)
            assert get_all(lib) == base, "another thread's setters changed this thread's modes"
            set_all(lib, base)
        finally:
            main_has_set.set()
        first, later = w.finish()
        assert first == theirs
        assert later == theirs, "this thread's setters changed the other thread's modes"
        assert get_all(lib) == base


def test_matrix_mode_is_process_wide(hiplib):
    lib = hiplib
    with preserved(lib):
        assert set_one(lib, PROCESS_WIDE, 0) == 0
        assert in_thread(lambda: (set_one(lib, PROCESS_WIDE, 1), get_one(lib, PROCESS_WIDE))) == (0, 1)
        assert get_one(lib, PROCESS_WIDE) == 1, "mms_set_matrix_mode on another thread is not visible here"
        assert in_thread(lambda: get_one(lib, PROCESS_WIDE)) == 1
        assert set_one(lib, PROCESS_WIDE, 0) == 0


def test_invalid_values_are_refused_on_a_worker_thread(hiplib):
    lib = hiplib

    def work():
        for stem in [s for s, _ in PER_THREAD] + [PROCESS_WIDE]:
            before = get_one(lib, stem)
            for bad in (-1, 2, 7, 2 ** 31 - 1):
                assert set_one(lib, stem, bad) == 1, "%s accepted %d" % (stem, bad)      # MMS_ERR_INVALID_ARG
                assert get_one(lib, stem) == before, "%s changed by a refused value" % stem
        return get_all(lib)

    with preserved(lib):
        assert in_thread(work) == defaults()


ENV_CASES = [(None, 0), ("fp32", 0), ("reference", 1), ("exact", 1), ("1", 1), ("0", 0), ("nonsense", 0)]


@pytest.mark.parametrize("main_sets_opposite", [False, True], ids=["untouched", "main-sets-opposite"])
@pytest.mark.parametrize("value,want", ENV_CASES, ids=[str(v) for v, _ in ENV_CASES])
def test_environment_gives_the_process_default(value, want, main_sets_opposite, hiplib):
    """A fresh process per setting (the library reads the variable once).  With the main thread's own setting the
    opposite of the environment's, a new thread still starts from the environment's."""
    assert euclid_mode_of(value) == want
    env = dict(os.environ)
    env.pop("MMS_EUCLID_BWD", None)
    if value is not None:
        env["MMS_EUCLID_BWD"] = value
    cmd = [sys.executable, os.path.join(HERE, "mode_env_worker.py")]
    if main_sets_opposite:
        cmd += ["--main-sets", str(1 - want)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=WAIT)
    assert p.returncode == 0, p.stderr
    seen = dict(line.split() for line in p.stdout.splitlines() if line.split()[:1] in (["main"], ["thread"]))
    assert seen == {"main": str(1 - want if main_sets_opposite else want), "thread": str(want)}, p.stdout


@pytest.mark.gpu
def test_two_threads_compute_under_their_own_modes(oracle, hiplib):
    """The test thread: Euclid "reference", loss_sum "reference", hinge "cpu" -- the oracle's bits in dq, loss and
    da.  A worker: Euclid "fp32", loss_sum "fast", hinge "gpu".  Their calls alternate, three rounds each; every
    round each thread gets what ITS modes promise."""
    import torch
    from mms_answer_selection_amd import capi
    lib = hiplib
    r = rng(2024)
    N, D = 96, 300                                                        # the mode-matrix case
    q, a = qa(r, N, 1, 1, D)
    dT = r.standard_normal((N, 1, 1, 1)).astype(np.float32)
    top_ref, _, _ = oracle.simcross_forward(1, q, a)
    dq_ref, da_ref, _, _ = oracle.simcross_backward(1, q, a, top_ref, dT)
    sa = r.standard_normal((257, 1)).astype(np.float32)                   # ties at the hinge
    sb = sa.copy(); sb[::3] -= 0.5; sb[1::3] += 0.25
    y = (r.uniform(size=(257, 1)) < 0.7).astype(np.float32)
    loss_ref, o_ref, s_ref = oracle.pairrank_forward(sa, sb, y, 0.5)
    ga_ref, gb_ref = oracle.pairrank_backward(y, o_ref, s_ref, top_diff=1.0)
    tie = (o_ref == 0) & (y == 1)
    assert tie.sum() >= 8 and (ga_ref[tie] == 0).all()                    # Backward_cpu's `>` stops the hinge term there
    at_tie = -(np.float32(1.0) / np.float32(257))                         # the .cu kernel's `>=` lets it through: -y / count

    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    nan = lambda shape: torch.full(tuple(shape), float("nan"), device="cuda")
    qd, ad, topd, dTd, sad, sbd, yd = (up(x) for x in (q, a, top_ref, dT, sa, sb, y))

    def one_round():
        gq, ga = nan(q.shape), nan(a.shape)
        capi.simcross_backward(1, qd, ad, topd, dTd, gq, ga)
        po, ps, pl = nan(sa.shape), nan(sa.shape), nan((1,))
        capi.pairrank_forward(sad, sbd, yd, po, ps, pl, margin=0.5)
        pa, pb = nan(sa.shape), nan(sa.shape)
        capi.pairrank_backward(yd, po, ps, pa, pb)
        torch.cuda.synchronize()
        return dict(dq=gq.cpu().numpy(), loss=pl.cpu().numpy(), da=pa.cpu().numpy(), modes=get_all(lib))

    my_turn, their_turn = threading.Event(), threading.Event()
    stop = []

    def work():
        capi.set_euclid_backward_mode("fp32")
        capi.set_loss_sum_mode("fast")
        capi.set_pairrank_hinge_mode("gpu")
        rounds = []
        for _ in range(3):
            assert their_turn.wait(WAIT)
            their_turn.clear()
            if stop:
                break
            rounds.append(one_round())
            my_turn.set()
        return rounds

    with preserved(lib):
        # what the worker's modes give on ONE thread: the kernels are deterministic, so the worker must get these bits
        capi.set_euclid_backward_mode("fp32")
        capi.set_loss_sum_mode("fast")
        capi.set_pairrank_hinge_mode("gpu")
        alone = one_round()
        capi.set_euclid_backward_mode("reference")
        capi.set_loss_sum_mode("reference")
        capi.set_pairrank_hinge_mode("cpu")
        w = Worker(work, release=(my_turn,))
        w.start()
        mine = []
        try:
            for _ in range(3):
                mine.append(one_round())
                their_turn.set()
                assert my_turn.wait(WAIT)
                my_turn.clear()
                if w.error is not None:
                    break
        finally:
            stop.append(True)
            their_turn.set()
        theirs = w.finish()
    assert len(mine) == 3 and len(theirs) == 3
    for i, m in enumerate(mine):
        assert m["modes"][:3] == [1, 0, 1], "test thread's euclid / hinge / loss_sum modes in round %d" % i
        assert_bitexact(m["dq"], dq_ref, "test thread, round %d: dq, reference mode" % i)
        assert_bitexact(m["loss"], np.array([loss_ref], np.float32), "test thread, round %d: loss, reference sum" % i)
        assert_bitexact(m["da"], ga_ref, "test thread, round %d: da, Backward_cpu comparison" % i)
    for i, t in enumerate(theirs):
        assert t["modes"][:3] == [0, 1, 0], "worker's euclid / hinge / loss_sum modes in round %d" % i
        assert_close(t["dq"], dq_ref, TOL, "worker, round %d: dq, fp32 mode" % i)
        assert_bitexact(t["dq"], alone["dq"], "worker, round %d: dq is what fp32 mode gives on one thread" % i)
        assert_close(t["loss"][0], loss_ref, TOL, "worker, round %d: loss" % i)
        assert_bitexact(t["loss"], alone["loss"], "worker, round %d: loss is what the fast sum gives on one thread" % i)
        assert_bitexact(t["da"][tie], np.full(int(tie.sum()), at_tie, np.float32), "worker, round %d: hinge rows" % i)
        assert_bitexact(t["da"][~tie], ga_ref[~tie], "worker, round %d: rows off the tie" % i)
