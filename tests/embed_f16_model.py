"""Inputs that pin the ordered scatter-add of the fp16-storage Embed backward (mms_embed_backward*_f16) -- plain numpy,
no GPU.  The segment lengths and the witness come from tests/embed_segments.py; the values do not.

es.telescoping_diff rounded to half does NOT pin the order: with half-valued addends of size ~1 on an fp32 accumulator
of size ~1 nearly every add is exact (a half has 11 significant bits, the accumulator 24), and an adjacent swap then
changes no word of the result.  Here the accumulator is LARGE instead:

  top_diff  N(0, 1) rounded to half (numpy's astype(float16) rounds to nearest even), and
  wd0       +-(8192 + U[0, 4096)) in fp32 on every table row,

so the accumulator's ulp, 2^-10, exceeds the granularity of the addends below 1 (a half in [0.5, 1) is a multiple of
2^-11, a smaller one of a finer grid) and close to half of all adds round, all along every chain.  A running sum of up
to 769 N(0, 1) rows moves the accumulator by ~30: it stays inside [4096, 16384), ulp 2^-11 at the smallest."""
import functools

import numpy as np

import embed_segments as es

H, F = np.float16, np.float32
LENGTHS = es.FLOAT_LENGTHS      # the half instantiation keeps kSegChunk = 256 rows: the float path boundaries
CH = 256
K = es.K


def widen(x):
    """half -> float, exactly"""
    assert x.dtype == H
    return x.astype(F)


def large_accumulator_inputs(index, N, K, seed):
    """-> (top_diff (M, N) half, wd0 (K, N) fp32, bd0 (N) fp32) for the id vector `index`"""
    r = np.random.default_rng(seed)
    top_diff = r.standard_normal((np.asarray(index).size, N)).astype(H)
    sign = np.where(r.uniform(size=(K, N)) < 0.5, -1.0, 1.0)
    wd0 = (sign * (8192.0 + r.uniform(0.0, 4096.0, (K, N)))).astype(F)
    bd0 = r.standard_normal(N).astype(F)
    return top_diff, wd0, bd0


# ---- the cases tests/test_gpu_embed_f16.py runs: name -> (M, N, seed); K = 600, planted lengths es.FLOAT_LENGTHS -----
# The seeds are held to the conditions of tests/test_embed_f16_model.py.  Measured smallest es.order_witness per case on
# the widened values (swap / drop_last / add_twice, words of 300):
#   f16-M4000-N300  13 / 299 / 299     f16-M4500-N300  8 / 299 / 299
CASES = {
    "f16-M4000-N300": (4000, 300, 5101),       # one-workgroup index
    "f16-M4500-N300": (4500, 300, 5102),       # device-wide sort
    "f16-M4000-N51": (4000, 51, 5103),         # odd N: every other row of top_diff is only 2-byte aligned
}
WITNESS_CASES = tuple(n for n, c in CASES.items() if c[1] == 300)


@functools.lru_cache(maxsize=None)
def make_case(name):
    """The inputs of one case (treat as read-only)."""
    M, N, seed = CASES[name]
    index, planted = es.planted_index(LENGTHS, M, K, seed)
    top_diff, wd0, bd0 = large_accumulator_inputs(index, N, K, seed + 50)
    c = {"name": name, "M": M, "N": N, "K": K, "lengths": tuple(LENGTHS), "index": index, "planted": planted,
         "top_diff": top_diff, "wd0": wd0, "bd0": bd0}
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c
