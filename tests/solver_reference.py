"""The solver update of include/mms_solver.h as a numpy model: the reference's CPU path (SGDSolver::ApplyUpdate),
one numpy operation per rounding, in float32 or float64.  Every array operation below is elementwise and rounds once in
the array's dtype, which is what the table in the header states; the cited lines are the reference's.

Restated, not copied (the header says the same): caffe_powx(x, 2) as x * x, caffe_powx(x, 0.5) as sqrt(x), and
caffe_cpu_axpby / caffe_axpy as rounded products and a rounded sum.
"""
import collections

import numpy as np

SGD, ADADELTA = 0, 1
L2, L1 = 0, 1
DIFF_UPDATE, DIFF_ZERO = 0, 1

# SolverParameter; the four numbers are float fields of the proto, so they pass through float32 on their way to Dtype
Param = collections.namedtuple("Param", "type regularization iter_size diff_out momentum delta weight_decay clip_gradients")


def param(type=ADADELTA, regularization=L2, iter_size=1, diff_out=DIFF_UPDATE, momentum=0.0, delta=1e-8,
          weight_decay=0.0, clip_gradients=-1.0):
    return Param(type, regularization, iter_size, diff_out, momentum, delta, weight_decay, clip_gradients)


class Blob:
    """One learnable parameter and its solver state: w = data, g = diff, h = history_[i], h2 = history_[P + i]."""

    def __init__(self, w, g, h, h2, lr_mult=1.0, decay_mult=1.0):
        self.w, self.g, self.h, self.h2, self.lr_mult, self.decay_mult = w, g, h, h2, lr_mult, decay_mult

    def copy(self):
        return Blob(self.w.copy(), self.g.copy(), self.h.copy(), None if self.h2 is None else self.h2.copy(),
                    self.lr_mult, self.decay_mult)


def _field(dt, v):
    return dt(np.float32(v))


def l2norm(dt, blobs):
    """sgd_solver.cpp:85-89: sqrt of the sum over blobs of sumsq(diff), in Dtype.  The order of a blob's own sum is
    BLAS's there and a fixed tree in the library: this one (numpy's) is a third, so it is EXACT only on data whose
    every partial sum is exact, and that is all it is used for."""
    total = dt(0)
    for b in blobs:
        total = dt(total + dt(np.sum(b.g * b.g, dtype=dt)))
    return dt(np.sqrt(total))


def clip_scale(dt, norm, clip_gradients):
    """sgd_solver.cpp:90-91: the scale, or 1 where the reference does not scale."""
    clip = _field(dt, clip_gradients)
    return dt(clip / dt(norm)) if dt(norm) > clip else dt(1)


def step(dt, p, blobs, rate, scale=None):
    """One ApplyUpdate + Net::Update on copies of `blobs` -> (new blobs, l2norm or None, scale or None).  With clipping
    on, `scale` is the scale to apply (as the library returned it); None: the model's own l2norm() and clip_scale()."""
    dt = np.dtype(dt).type
    m = _field(dt, p.momentum)
    om = dt(dt(1) - m)
    d = _field(dt, p.delta)
    wd = _field(dt, p.weight_decay)
    rate = dt(rate)
    norm = None
    if p.clip_gradients >= 0 and scale is None:                        # sgd_solver.cpp:81-99
        norm = l2norm(dt, blobs)
        scale = clip_scale(dt, norm, p.clip_gradients)
    out = []
    with np.errstate(all="ignore"):
        for b in blobs:
            b = b.copy()
            w, g, h, h2 = b.w, b.g, b.h, b.h2
            assert all(a is None or a.dtype == dt for a in (w, g, h, h2))
            if p.clip_gradients >= 0 and dt(scale) != dt(1):           # :90-97, scale_diff
                g = g * dt(scale)
            if p.iter_size != 1:                                       # :119-127
                accum = dt(dt(1) / dt(p.iter_size))
                g = g * accum
            ld = dt(wd * dt(np.float32(b.decay_mult)))                 # :151
            if ld != 0:                                                # :154
                r = w if p.regularization == L2 else np.sign(w).astype(dt)    # :155-168; caffe_cpu_sign
                if p.regularization == L1:
                    r = np.where(np.isnan(w), dt(0), r).astype(dt)     # (0 < NaN) - (NaN < 0) = 0
                t = ld * r
                g = g + t
            lr = dt(rate * dt(np.float32(b.lr_mult)))                  # sgd_solver.cpp:217, adadelta_solver.cpp:31
            if p.type == ADADELTA:
                u = g * g                                              # adadelta_solver.cpp:36-38
                a = om * u                                             # :41-43
                c = m * h
                h = a + c
                u = d + h2                                             # :49-52
                t = d + h                                              # :54-57
                u = u / t                                              # :60-63
                u = np.sqrt(u)                                         # :66-68
                g = g * u                                              # :71-74
                u = g * g                                              # :77-79
                a = om * u                                             # :82-84
                c = m * h2
                h2 = a + c
                g = lr * g                                             # :87-89
            elif p.type == SGD:
                a = lr * g                                             # sgd_solver.cpp:221-223
                c = m * h
                h = a + c
                g = h.copy()                                           # :224-226
            else:
                raise ValueError("solver type %r" % (p.type,))
            w = w - g                                                  # blob.cpp:161
            if p.diff_out == DIFF_ZERO:                                # net.cpp:923
                g = np.zeros_like(g)
            b.w, b.g, b.h, b.h2 = (x if x is None else x.astype(dt, copy=False) for x in (w, g, h, h2))
            out.append(b)
    return out, norm, scale
