"""A numpy restatement of include/mms_dropout.h, word for word: Philox4x32-10 in uint64 arithmetic, the word of a global
element index, thr and scale per element type in numpy's float32 / float64 arithmetic, and forward / backward / mask.
Not a test file: tests/test_dropout_model.py pins it against the published known answers, tests/test_abi_dropout.py and
tests/test_gpu_dropout.py compare the library with it."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
TRAIN, TEST = 0, 1

_U = np.uint64
_LOW = _U(0xFFFFFFFF)
_32 = _U(32)

KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(ctr, key):
    """ctr: four 32-bit words (scalars or equally shaped arrays), key: two scalars -> the four output words, uint64
    arrays holding 32-bit values.  Every product is of two values below 2^32, so uint64 holds it exactly."""
    c = [np.asarray(v, dtype=_U) & _LOW for v in ctr]
    k0, k1 = (_U(int(v) & 0xFFFFFFFF) for v in key)
    for _ in range(10):
        p0, p1 = _U(M0) * c[0], _U(M1) * c[2]
        c = [(p1 >> _32) ^ c[1] ^ k0, p1 & _LOW, (p0 >> _32) ^ c[3] ^ k1, p0 & _LOW]
        k0, k1 = (k0 + _U(W0)) & _LOW, (k1 + _U(W1)) & _LOW
    return c


def words(seed, sequence, offset, count):
    """word(g) for g = offset .. offset + count - 1 as a uint32 array; Python integers carry the 64-bit g."""
    seed, sequence, offset, count = int(seed), int(sequence), int(offset), int(count)
    assert 0 <= offset and offset + count <= 1 << 64
    if count == 0:
        return np.zeros(0, np.uint32)
    first, last = offset >> 2, (offset + count - 1) >> 2
    groups = _U(first) + np.arange(last - first + 1, dtype=_U)      # uint64 + uint64: no detour through float64
    out = philox4x32_10((groups & _LOW, groups >> _32, sequence & 0xFFFFFFFF, sequence >> 32),
                        (seed & 0xFFFFFFFF, seed >> 32))
    flat = np.stack(out, axis=1).reshape(-1).astype(np.uint32)
    lead = offset & 3
    return flat[lead:lead + count]


def word(seed, sequence, g):
    return int(words(seed, sequence, g, 1)[0])


def threshold(ratio, dtype):
    """(thr, scale) as DropoutLayer::LayerSetUp computes them with Dtype = dtype; None for a ratio the calls refuse."""
    T = np.dtype(dtype).type
    r = T(ratio)
    if not (r > T(0) and r < T(1)):
        return None
    t = T(2 ** 32 - 1) * r                       # float32(UINT_MAX) is 2^32; one product in T
    if not t < T(4294967296.0):
        return None
    return int(t), T(1.0 / (1.0 - float(r)))     # float(r) is exact; the quotient is double arithmetic, then narrowed


def mask(count, ratio, seed, sequence, offset=0, dtype=np.float32):
    thr, _ = threshold(ratio, dtype)
    return (words(seed, sequence, offset, count) > np.uint32(thr)).astype(np.uint32)


def forward(x, ratio, seed, sequence, offset=0, phase=TRAIN):
    """x: a float32 or float64 array -> (x * Dtype(keep)) * scale, two roundings, in x's dtype."""
    x = np.asarray(x)
    if phase == TEST:
        return x.copy()
    _, scale = threshold(ratio, x.dtype)
    keep = mask(x.size, ratio, seed, sequence, offset, x.dtype).reshape(x.shape).astype(x.dtype)
    with np.errstate(invalid="ignore"):
        return (x * keep) * scale


backward = forward                                # the same map on the diffs
