"""The two routes of the backward-only Euclid launch at the GloVe widths (simcross_rows.hip: launch_pair32 ->
euclid_block_kernel<.., FULL>).  A workgroup owns 16 consecutive pairs.  N a multiple of 16 takes the whole-batch
instantiation (no end-of-batch clamps, unmasked stores, coefficients formed ahead of the operands); any other N
takes the clamped instantiation, whose last workgroup is partly filled.  Both must give the oracle's gradients --
the reference's bits in the reference arithmetic, the 1e-5 relative bar of tests/test_gpu_bwd_modes.py in the
default fp32 arithmetic -- and must write nothing outside dq / da.

Pairs are independent, so one oracle run per width on 48 pairs serves every N (the first N pairs); `top` comes from
the library's own Forward launch.  q, a, dq and da are carved from flat buffers so that their base pointers sit 0,
16 or 48 bytes past a 128-byte boundary; dq / da have one guard row on either side holding a sentinel bit pattern.

propagate_down: mms_simcross_backward_f32 (mms_abi.hip) looks at the two flags only to tell "neither" (two memsets,
no kernel) from "at least one"; with one flag off it still launches this kernel, which writes both gradients.  There
is no route that leaves one buffer untouched, so that case of the issue has nothing to check here and is left out.
"""
import numpy as np
import pytest
import torch

from mms_answer_selection_amd import capi

pytestmark = pytest.mark.gpu

NMAX = 48
WIDTHS = (100, 200, 300)
N_FULL = (16, 32, 48)              # every workgroup inside the batch
N_CLAMPED = (1, 15, 17, 33)        # one partly filled last workgroup
OFFSETS = (0, 16, 48)              # bytes past a 128-byte boundary
SENTINEL = np.uint32(0xFFC5A5A5)   # a NaN payload no gradient can carry


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


_cases = {}


def case(D, oracle):
    """NMAX pairs of width D in the benchmark's distribution and the oracle's outputs: computed once, never written."""
    if D not in _cases:
        r = np.random.default_rng(4096 + D)
        q = (r.standard_normal((NMAX, 1, D)) * 0.4).astype(np.float32)
        a = (r.standard_normal((NMAX, 1, D)) * 0.4).astype(np.float32)
        dT = r.standard_normal((NMAX, 1, 1, 1)).astype(np.float32)
        top, _, _ = oracle.simcross_forward(1, q, a)
        dq, da, _, _ = oracle.simcross_backward(1, q, a, top, dT)
        for x in (q, a, dT, top, dq, da):
            x.setflags(write=False)
        _cases[D] = (q, a, dT, top, dq, da)
    return _cases[D]


def carve(rows, D, offset, guard):
    """A (rows, 1, D) device view whose first byte sits `offset` bytes past a 128-byte boundary, with `guard` rows of
    SENTINEL words before and after it.  Returns (whole flat buffer, index of the view's first float, view)."""
    total = (rows + 2 * guard) * D + 64
    flat = torch.from_numpy(np.full(total, SENTINEL, dtype=np.uint32).view(np.float32).copy()).cuda()
    start = guard * D
    while (flat.data_ptr() + 4 * start) % 128 != offset:
        start += 1
    view = flat[start:start + rows * D].view(rows, 1, D)
    assert view.data_ptr() % 128 == offset
    return flat, start, view


def backward(oracle, D, N, offset, mode):
    """One backward-only launch on the first N pairs; checks the guards, returns (dq, da) as numpy arrays."""
    q, a, dT, top_ref, _, _ = case(D, oracle)
    _, _, qd = carve(N, D, offset, 0)
    _, _, ad = carve(N, D, offset, 0)
    qd.copy_(torch.from_numpy(q[:N].copy()))
    ad.copy_(torch.from_numpy(a[:N].copy()))
    dTd = torch.from_numpy(dT[:N].copy()).cuda()
    top = torch.empty(N, 1, 1, 1, device="cuda")
    capi.simcross_forward(1, qd, ad, top)
    assert (_bits(top.cpu().numpy()) == _bits(top_ref[:N])).all()
    out = []
    for _ in range(2):
        out.append(carve(N, D, offset, 1))
    capi.simcross_backward(1, qd, ad, top, dTd, out[0][2], out[1][2])
    torch.cuda.synchronize()
    what = "D=%d N=%d offset=%d %s" % (D, N, offset, mode)
    for name, (flat, start, view) in zip(("dq", "da"), out):
        host = _bits(flat.cpu().numpy())
        assert (host[:start] == SENTINEL).all(), "%s: words before %s written" % (what, name)
        assert (host[start + N * D:] == SENTINEL).all(), "%s: words after %s written" % (what, name)
    return out[0][2].cpu().numpy(), out[1][2].cpu().numpy()


def check_grad(got, ref, what, mode):
    if mode == "reference":
        assert (_bits(got) == _bits(ref)).all(), "%s: %d words differ" % (what, int((_bits(got) != _bits(ref)).sum()))
    else:
        nz = ref != 0                                         # (an exact zero has no relative error to print)
        print("%s: max relative error %.3e" % (what, float(np.max(np.abs(got[nz] - ref[nz]) / np.abs(ref[nz])))))
        np.testing.assert_allclose(got, ref, rtol=1e-5, atol=0, err_msg=what)


@pytest.fixture
def bwd_mode(request):
    before = capi.get_euclid_backward_mode()
    capi.set_euclid_backward_mode(request.param)
    assert capi.get_euclid_backward_mode() == request.param
    yield request.param
    capi.set_euclid_backward_mode(before)


@pytest.mark.parametrize("bwd_mode", ["reference", "fp32"], indirect=True)
@pytest.mark.parametrize("D", WIDTHS)
def test_both_routes_match_the_oracle_and_write_nothing_else(D, bwd_mode, oracle, hiplib):
    _, _, _, _, dq_ref, da_ref = case(D, oracle)
    for N in N_FULL + N_CLAMPED:
        for offset in OFFSETS:
            dq, da = backward(oracle, D, N, offset, bwd_mode)
            what = "D=%d N=%d offset=%d %s" % (D, N, offset, bwd_mode)
            check_grad(dq, dq_ref[:N], what + " dq", bwd_mode)
            check_grad(da, da_ref[:N], what + " da", bwd_mode)


@pytest.mark.parametrize("bwd_mode", ["reference", "fp32"], indirect=True)
@pytest.mark.parametrize("D", WIDTHS)
def test_routes_agree_on_shared_pairs(D, bwd_mode, oracle, hiplib):
    """N = 33 (clamped route, three workgroups) then N = 32 (whole-batch route) on the same first 32 pairs: pairs are
    independent, so rows 0-31 carry the same 32-bit words in both arithmetic modes."""
    dq33, da33 = backward(oracle, D, 33, 0, bwd_mode)
    dq32, da32 = backward(oracle, D, 32, 0, bwd_mode)
    assert (_bits(dq33[:32]) == _bits(dq32)).all()
    assert (_bits(da33[:32]) == _bits(da32)).all()
