"""Inputs that pin the ordered scatter-add of the Embed backward (csrc/embed.hip) -- plain numpy, no GPU.

weight_diff[id, :] receives the rows of top_diff that carry `id` one by one, n ascending, on top of the value already
there (embed_layer.cpp:155-180), and the library promises those bits.  HOW a segment (the rows of one id) is summed
depends on its length R; `length_class` names the paths.  Two things make the promise testable:

  planted_index     an id vector with segments of exactly the wanted lengths, every boundary between two paths among
                    them, scattered over the batch;
  telescoping_diff  a top_diff whose running sum per destination row stays O(1).  With plain N(0, 1) rows the sum grows
                    like sqrt(R), the low bits of two neighbouring addends are then lost the same way in either order,
                    and an adjacent swap inside a long segment changes NO word of the result: bit equality would not
                    see a locally wrong order.  With a telescoping sum every addend keeps meeting an accumulator of
                    its own size.

`order_witness` measures, with the reference chain alone, how many words of a destination row one adjacent swap (or a
dropped / doubled last row) changes: the condition tests/test_embed_segments.py puts on the inputs."""
import functools

import numpy as np

FLOAT_LENGTHS = (1, 2, 7, 8, 9, 31, 32, 33, 34, 255, 256, 257, 264, 511, 512, 513, 769)      # 3494 rows
DOUBLE_LENGTHS = (1, 8, 9, 32, 33, 127, 128, 129, 136, 255, 256, 257, 385)                   # 1756 rows
K = 600
PAIR_CUT = 1777                 # M0 of the pair calls: layer 0 = rows [0, 1777), layer 1 = the rest
PREP_MAX = 4096                 # kPrepMax: the one-workgroup inverted index up to here, the device-wide sort above
CLASSES = ("1..8", "9..32", "33..CH", "CH+1..2CH", ">2CH")


def seg_chunk(dtype):
    """kSegChunk<T> of csrc/embed.hip"""
    return 256 if np.dtype(dtype) == np.float32 else 128


def length_class(R, CH):
    if R <= 8:
        return "1..8"              # embed_bwd_short_kernel, 8-load branch
    if R <= 32:
        return "9..32"             # embed_bwd_short_kernel, 32-load branch
    if R <= CH:
        return "33..CH"            # embed_bwd_seg_kernel, one chunk
    if R <= 2 * CH:
        return "CH+1..2CH"         # two chunks: stage_rows(1, CH) runs
    return ">2CH"                  # the in-loop stage_rows, double-buffered gather


def segment_lengths(index):
    """id -> number of rows that carry it"""
    ids, counts = np.unique(np.asarray(index).astype(np.int64), return_counts=True)
    return dict(zip(ids.tolist(), counts.tolist()))


def class_histogram(index, CH):
    hist = dict.fromkeys(CLASSES, 0)
    for R in segment_lengths(index).values():
        hist[length_class(R, CH)] += 1
    return hist


def planted_index(lengths, M, K, seed):
    """-> (index (M,) int64, planted ids (len(lengths),)): planted id i owns exactly lengths[i] rows, no other id more
    than 8, all of it shuffled over the batch."""
    r = np.random.default_rng(seed)
    lengths = np.asarray(lengths, np.int64)
    rest = M - int(lengths.sum())
    ids = r.permutation(K)
    planted, others = ids[:lengths.size], ids[lengths.size:]
    assert lengths.size <= K and 0 <= rest <= 8 * others.size, (M, K, rest)
    filler = r.permutation(np.repeat(others, 8))[:rest]           # without replacement: at most 8 of each
    index = r.permutation(np.concatenate([np.repeat(planted, lengths), filler]))
    return index.astype(np.int64), planted.astype(np.int64)


def telescoping_diff(index, N, dtype, seed):
    """-> (top_diff (M, N), ids, y0 (len(ids), N)).  For every id, with its rows n_1 < n_2 < ... in batch order,
    top_diff[n_t] = y_t - y_(t-1), y ~ N(0, 1) per column in `dtype`; weight_diff[ids[i]] must start at y0[i].  The
    running sum after t rows is then y_t up to rounding, whatever the segment's length."""
    r = np.random.default_rng(seed)
    index = np.asarray(index).astype(np.int64)
    order = np.argsort(index, kind="stable")                       # segments side by side, n ascending inside
    sid = index[order]
    head = np.r_[True, sid[1:] != sid[:-1]]
    ids = sid[head]
    y = r.standard_normal((index.size, N)).astype(dtype)
    y0 = r.standard_normal((ids.size, N)).astype(dtype)
    prev = np.empty_like(y)
    prev[1:] = y[:-1]
    prev[head] = y0
    top_diff = np.empty_like(y)
    top_diff[order] = y - prev
    return top_diff, ids, y0


def _words(x):
    x = np.ascontiguousarray(x)
    return x.view("u%d" % x.dtype.itemsize)


def reference_prefix(X, a0):
    """P[t] = the accumulator before row t is added, P[R] = the result: acc = 1 * X[t] + acc in X's dtype."""
    P = np.empty((X.shape[0] + 1, X.shape[1]), X.dtype)
    P[0] = a0
    for t in range(X.shape[0]):
        P[t + 1] = X[t] + P[t]
    return P


def swapped_chains(X, P, swaps):
    """Results (len(swaps), N) of the chain with rows s and s + 1 exchanged, s in `swaps` (ascending).  Chain s is the
    reference up to row s, so it joins the (swaps, N) accumulator there; every row is stepped once per later t."""
    R = X.shape[0]
    swaps = np.asarray(swaps, np.int64)
    at = {int(s): k for k, s in enumerate(swaps)}
    A = np.empty((swaps.size, X.shape[1]), X.dtype)
    for t in range(R):
        n = int(np.searchsorted(swaps, t - 1, "left"))             # chains with s + 1 < t: past their swap
        A[:n] += X[t]
        k = at.get(t - 1)
        if k is not None:
            A[k] = X[t - 1] + A[k]
        k = at.get(t)
        if k is not None:
            A[k] = X[t + 1] + P[t]
    return A


def swaps_to_check(R, CH):
    """Every adjacent swap for R <= 800; beyond that the ones at the chunk boundaries and 64 evenly spaced others."""
    if R <= 800:
        return np.arange(R - 1)
    edge = [s for b in range(CH, R, CH) for s in (b - 2, b - 1, b) if 0 <= s < R - 1]
    return np.unique(np.r_[edge, np.linspace(0, R - 2, 64).astype(np.int64), R - 2]).astype(np.int64)


def order_witness(index, top_diff, wd0, planted_ids):
    """Per planted segment, from the reference chain alone: the SMALLEST number of words of the destination row that
    one adjacent swap of its rows changes ("swap", None for R = 1), and the number changed by leaving the last row out
    ("drop_last") and by adding it twice ("add_twice")."""
    index = np.asarray(index).astype(np.int64)
    CH = seg_chunk(top_diff.dtype)
    out = []
    for i in planted_ids:
        X = top_diff[np.flatnonzero(index == i)]
        R = X.shape[0]
        P = reference_prefix(X, wd0[i])
        final = _words(P[R])
        w = {"id": int(i), "R": R, "swap": None,
             "drop_last": int((_words(P[R - 1]) != final).sum()),
             "add_twice": int((_words(X[R - 1] + P[R]) != final).sum())}
        if R >= 2:
            A = swapped_chains(X, P, swaps_to_check(R, CH))
            w["swap"] = int((_words(A) != final).sum(axis=1).min())
        out.append(w)
    return out


# ---- the cases tests/test_gpu_embed_segments.py runs: name -> (dtype, M, N, planted lengths, seed) -----------------
# K = 600 throughout; N = 300 is five column slices, the last one 44 wide.  The seeds are held to the conditions of
# tests/test_embed_segments.py (exact histogram, every length class, a segment across the pair cut, order_witness >= 1
# at N = 300).  Measured smallest order_witness per case (swap / drop_last / add_twice, words of 300):
#   f32-M4000-N300  4 / 300 / 300     f32-M4500-N300  5 / 300 / 300
#   f64-M2200-N300  6 / 300 / 300     f64-M4200-N300  4 / 300 / 300
CASES = {
    "f32-M4000-N300": (np.float32, 4000, 300, FLOAT_LENGTHS, 4101),      # one-workgroup index
    "f32-M4500-N300": (np.float32, 4500, 300, FLOAT_LENGTHS, 4102),      # device-wide sort
    "f32-M4000-N50": (np.float32, 4000, 50, FLOAT_LENGTHS, 4103),        # narrow: one partial column slice
    "f64-M2200-N300": (np.float64, 2200, 300, DOUBLE_LENGTHS, 4104),     # one-workgroup index
    "f64-M4200-N300": (np.float64, 4200, 300, DOUBLE_LENGTHS, 4105),     # device-wide sort
}
FLOAT_CASES = tuple(n for n, c in CASES.items() if c[0] == np.float32)
DOUBLE_CASES = tuple(n for n, c in CASES.items() if c[0] == np.float64)
WITNESS_CASES = tuple(n for n, c in CASES.items() if c[2] == 300)


@functools.lru_cache(maxsize=None)
def make_case(name):
    """The inputs of one case (treat as read-only): weight_diff starts at the telescoping y0 on every row a segment
    lands on and at random values elsewhere, bias_diff at random values."""
    dtype, M, N, lengths, seed = CASES[name]
    index, planted = planted_index(lengths, M, K, seed)
    top_diff, ids, y0 = telescoping_diff(index, N, dtype, seed + 50)
    r = np.random.default_rng(seed + 100)
    wd0 = r.standard_normal((K, N)).astype(dtype)
    wd0[ids] = y0
    bd0 = r.standard_normal(N).astype(dtype)
    c = {"name": name, "dtype": dtype, "M": M, "N": N, "K": K, "lengths": tuple(lengths), "index": index,
         "planted": planted, "top_diff": top_diff, "wd0": wd0, "bd0": bd0}
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def straddlers(index, planted, cut):
    """planted ids with rows on both sides of `cut`"""
    index = np.asarray(index)
    return [int(i) for i in planted if (index[:cut] == i).any() and (index[cut:] == i).any()]
