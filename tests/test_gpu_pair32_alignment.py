"""euclid_pair32_kernel's line-aligned lane map (simcross_rows.hip, SHIFT): lane j, slot `it` of a half-wave holds
float4 j + 32*it - u of its row, u = the row's offset within a 128-byte line in float4s.  The map serves a launch
whose arrays are congruent mod 128; any other launch keeps the unshifted map.  Both must give the oracle's bits.

Operands are carved from ONE flat buffer at chosen offsets within a line (k float4s, k = 0..7): with row r at
u = (k + 3r) mod 8 (D = 100 / 300) every peel occurs at every k, the largest (7 idle lanes of 32 at D = 100, where
32 - 7 lanes are exactly the row) included.  N = 37: odd (the last wave misses a half), more than 16 (several
workgroups).  Each output sits between 64-float guard bands that must stay untouched: idle lanes store nothing.

Forward-only and fused launches run in this process.  The library serves a backward-only launch with the
workgroup-dense kernel; MMS_EUCLID_LAYOUT_BWD=pair (read once per process) routes it to euclid_pair32_kernel, so
those cases run in one child process: this file run as a script."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N = 37
WIDTHS = (100, 200, 300)
GUARD = 64
SENTINEL = np.float32(-7717.25)
# k (float4s into a 128-byte line) of q, a, dq, da: the eight congruent placements, then placements whose arrays
# disagree (all four; only the gradients; only q against a, which a forward-only launch sees too)
PLACEMENTS = [(k, k, k, k) for k in range(8)] + [(1, 3, 6, 0), (5, 5, 2, 5), (0, 7, 7, 7)]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


class Arena:
    """One flat device buffer full of SENTINEL; take() returns a view of n floats that starts k float4s into a
    128-byte line and keeps GUARD floats clear on both sides."""

    def __init__(self, floats):
        self.buf = torch.full((floats,), float(SENTINEL), dtype=torch.float32, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.cursor = 0
        self.outputs = []

    def take(self, n, k, output=False):
        off = self.cursor + GUARD
        while (self.buf.data_ptr() // 4 + off) % 32 != 4 * k:
            off += 1
        v = self.buf[off:off + n]
        assert v.data_ptr() % 128 == 16 * k
        self.cursor = off + n + GUARD
        assert self.cursor <= self.buf.numel()
        if output:
            self.outputs.append((off, n))
        return v

    def check_untouched(self, what):
        """Everything outside the outputs -- the guard bands and the inputs -- holds what it held before."""
        now = self.buf.cpu().numpy()
        keep = np.ones(now.size, dtype=bool)
        for off, n in self.outputs:
            keep[off:off + n] = False
            for lo in (off - GUARD, off + n):
                band = now[lo:lo + GUARD]
                assert (_bits(band) == _bits(SENTINEL)).all(), "%s: guard band at %d written" % (what, lo)
        assert (_bits(now[keep]) == _bits(self.before[keep])).all(), "%s: bytes outside the outputs changed" % what

    def freeze(self):
        self.before = self.buf.cpu().numpy().copy()


_cases = {}


def case(D, oracle):
    """Inputs and the oracle's outputs for width D: computed once, shared, never written."""
    if D not in _cases:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from util import qa, rng
        r = rng(37 * D)
        q, a = qa(r, N, 1, 1, D)
        a[1, 0] = q[1, 0]                           # degenerate pair: T = 1, divisor 1e-9
        a[2, 0, : D // 2] = q[2, 0, : D // 2]
        dT = r.standard_normal((N, 1, 1, 1)).astype(np.float32)
        top, _, _ = oracle.simcross_forward(1, q, a)
        dq, da, _, _ = oracle.simcross_backward(1, q, a, top, dT)
        for x in (q, a, dT, top, dq, da):
            x.setflags(write=False)
        _cases[D] = (q, a, dT, top, dq, da)
    return _cases[D]


def assert_grad(got, ref, what, mode):
    """reference mode: the reference's bits.  fp32 mode: one term per element, within 2 ulp of the reference's
    (normal numbers) and inside the 1e-5 bar (tests/test_gpu_parity.py: _assert_grad)."""
    if mode == "reference":
        assert (_bits(got) == _bits(ref)).all(), "%s: %d words differ" % (what, int((_bits(got) != _bits(ref)).sum()))
        return
    normal = np.abs(ref) >= np.float32(1.2e-38)
    ulps = np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    assert not normal.any() or ulps[normal].max() <= 2, "%s: %d ulp from the reference" % (what, ulps[normal].max())
    if (~normal).any():
        assert np.abs(got[~normal].astype(np.float64) - ref[~normal]).max() <= 1e-37, what
    err = np.abs(got.astype(np.float64) - ref).max()
    assert err <= 1e-5 * max(1.0, float(np.abs(ref).max())), "%s: max abs err %.3e" % (what, err)


def run_launch(capi, oracle, kind, D, place, mode):
    """One launch of `kind` (forward / fused / backward) at width D with q, a, dq, da placed at `place`."""
    q, a, dT, top_ref, dq_ref, da_ref = case(D, oracle)
    kq, ka, kdq, kda = place
    ar = Arena(4 * N * D + 3 * N + 16 * (GUARD + 32))
    qd, ad = ar.take(N * D, kq).view(N, 1, D), ar.take(N * D, ka).view(N, 1, D)
    dTd = ar.take(N, 0).view(N, 1, 1, 1)
    top = ar.take(N, 2, output=(kind != "backward")).view(N, 1, 1, 1)
    qd.copy_(torch.from_numpy(q))
    ad.copy_(torch.from_numpy(a))
    dTd.copy_(torch.from_numpy(dT))
    what = "%s D=%d k=%s %s" % (kind, D, place, mode)
    if kind == "backward":
        top.copy_(torch.from_numpy(top_ref))
    else:
        top.fill_(float("nan"))
    if kind != "forward":
        gq = ar.take(N * D, kdq, output=True).view(N, 1, D)
        ga = ar.take(N * D, kda, output=True).view(N, 1, D)
        gq.fill_(float("nan"))
        ga.fill_(float("nan"))
    ar.freeze()
    if kind == "forward":
        capi.simcross_forward(1, qd, ad, top)
    elif kind == "fused":
        capi.simcross_forward_backward(1, qd, ad, dTd, top, gq, ga)
    else:
        capi.simcross_backward(1, qd, ad, top, dTd, gq, ga)
    torch.cuda.synchronize()
    ar.check_untouched(what)
    if kind != "backward":
        got = top.cpu().numpy()
        assert (_bits(got) == _bits(top_ref)).all(), "%s: top differs from the oracle" % what
    if kind != "forward":
        assert_grad(gq.cpu().numpy(), dq_ref, what + " dq", mode)
        assert_grad(ga.cpu().numpy(), da_ref, what + " da", mode)


@pytest.mark.gpu
@pytest.mark.parametrize("bwd_mode", ["reference", "fp32"])
@pytest.mark.parametrize("D", WIDTHS)
def test_forward_and_fused_launches_at_every_line_offset(D, bwd_mode, oracle, hiplib):
    from mms_answer_selection_amd import capi
    capi.set_euclid_backward_mode(bwd_mode)          # (the autouse fixture restores the default afterwards)
    for place in PLACEMENTS:
        if bwd_mode == "reference":                  # a forward has no backward term: once is enough
            run_launch(capi, oracle, "forward", D, place, bwd_mode)
        run_launch(capi, oracle, "fused", D, place, bwd_mode)


@pytest.mark.gpu
def test_backward_only_pair_launch_at_every_line_offset(hiplib, oracle):
    env = dict(os.environ, MMS_EUCLID_LAYOUT_BWD="pair")
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "backward-only pair launches ok: %d" % (len(WIDTHS) * len(PLACEMENTS) * 2) in out.stdout


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from oracle import cpu_oracle
    from mms_answer_selection_amd import capi
    assert os.environ.get("MMS_EUCLID_LAYOUT_BWD") == "pair"
    cpu_oracle.build()
    done = 0
    for bwd_mode in ("reference", "fp32"):
        capi.set_euclid_backward_mode(bwd_mode)
        for D in WIDTHS:
            for place in PLACEMENTS:
                run_launch(capi, cpu_oracle, "backward", D, place, bwd_mode)
                done += 1
    print("backward-only pair launches ok: %d" % done)
