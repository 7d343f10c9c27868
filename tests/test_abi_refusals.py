"""CPU suite: the host-side argument rules of the launching entry points include/mms.h declares and csrc/mms_abi.hip
defines, as tables of (arguments, returned code) -- which of INVALID_ARG / UNSUPPORTED / WORKSPACE wins included.

Nothing is enqueued on any of these paths: every row is refused by a host-side rule or returns at an empty-batch
early-out, so the arrays are NULL or addresses that are never touched.  A row names only what differs from its form's
defaults; the defaults themselves (a valid call) are never sent.  The calls with refusal suites of their own (BN,
BN -> pool, FM, the f64 Embed / ranking calls, the fp16 Embed and bilinear-f16 calls) are pinned there."""
import ctypes as C

import pytest

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 3
P = 4096                                  # stands for arrays that are never touched: every call here returns first
AMPLE = 1 << 40                           # a workspace size no query exceeds


class Form:
    """The argument list of an entry point without its trailing stream: `name=value` scalars, `name*` arrays."""

    def __init__(self, spec):
        self.defaults, self.arrays = {}, []
        for k, tok in enumerate(spec.split()):
            if tok.endswith("*"):
                self.defaults[tok[:-1]] = P + 64 * k
                self.arrays.append(tok[:-1])
            else:
                name, value = tok.split("=")
                self.defaults[name] = float(value) if "." in value else int(value)

    def nulls(self, **more):
        return dict({a: None for a in self.arrays}, **more)

    def args(self, row):
        assert row and not set(row) - set(self.defaults), row      # the defaults alone would launch
        return dict(self.defaults, **row)


def each_null(names, code, **more):
    return [(dict({n: None}, **more), code) for n in names.split()]


def run(lib, symbol, form, table):
    fn = getattr(lib, symbol)
    for row, code in table:
        assert fn(*form.args(row).values(), None) == code, (symbol, row)


# ---- dist_mode, N, W1, W2, D (and M): the leading arguments of the SimCross families ----------------------------
MODE_RANGE = [({"dist_mode": -1}, INVALID), ({"dist_mode": 3}, INVALID)]
GRID_DIMS = [
    ({"N": -1}, INVALID), ({"W1": 0}, INVALID), ({"W1": -1}, INVALID), ({"W2": 0}, INVALID), ({"W2": -1}, INVALID),
    ({"D": 0}, INVALID), ({"D": -1}, INVALID),
    ({"N": 1, "W1": 2, "W2": 1, "D": 2 ** 30}, INVALID),           # N*W1*D alone passes INT_MAX
    ({"N": 1, "W1": 1, "W2": 2, "D": 2 ** 30}, INVALID),           # N*W2*D alone
    ({"N": 1, "W1": 2 ** 16, "W2": 2 ** 15, "D": 1}, INVALID),     # N*M*W1*W2 alone
    ({"N": 0, "D": 0}, INVALID),                                   # the sizes are judged before the empty batch
]
M_RANGE = [({"M": 0}, INVALID), ({"M": -1}, INVALID)]
M_NEEDS_BILINEAR = [({"dist_mode": 0, "M": 2}, INVALID), ({"dist_mode": 1, "M": 2}, INVALID),
                    ({"dist_mode": 2, "N": 1, "W1": 2 ** 10, "W2": 2 ** 10, "D": 1, "M": 2 ** 11}, INVALID)]
SIMCROSS_DIMS = MODE_RANGE + GRID_DIMS + M_RANGE + M_NEEDS_BILINEAR

SIMCROSS_FORWARD = Form("dist_mode=1 N=3 W1=2 W2=5 D=4 M=1 q* a* W* bias* top* norm0* norm1* workspace* workspace_bytes=0")
SIMCROSS_FORWARD_ROWS = SIMCROSS_DIMS + [
    (SIMCROSS_FORWARD.nulls(N=0), OK), (SIMCROSS_FORWARD.nulls(N=0, dist_mode=0), OK),
    (SIMCROSS_FORWARD.nulls(N=0, dist_mode=2, M=3), OK), ({"N": 0}, OK),
    (SIMCROSS_FORWARD.nulls(N=0, dist_mode=3), INVALID),
] + each_null("q a top", INVALID) + each_null("q a top norm0 norm1", INVALID, dist_mode=0) + \
    each_null("q a top W", INVALID, dist_mode=2, M=2) + [
    ({"dist_mode": 2, "W": None, "workspace": None}, INVALID),     # the arguments are judged before the workspace
    (SIMCROSS_FORWARD.nulls(), INVALID), (SIMCROSS_FORWARD.nulls(N=-1), INVALID),
]

SIMCROSS_BACKWARD = Form("dist_mode=1 N=3 W1=2 W2=5 D=4 M=1 q* a* W* bias_term=0 top* top_diff* norm0* norm1* "
                         "propagate_down0=1 propagate_down1=1 dq* da* dW* dbias* workspace* workspace_bytes=0")
SIMCROSS_BACKWARD_ROWS = SIMCROSS_DIMS + [
    (SIMCROSS_BACKWARD.nulls(N=0), OK), (SIMCROSS_BACKWARD.nulls(N=0, dist_mode=0), OK),
    (SIMCROSS_BACKWARD.nulls(N=0, dist_mode=2, M=3, bias_term=1), OK), ({"N": 0}, OK),
    (SIMCROSS_BACKWARD.nulls(N=0, M=0), INVALID),
] + each_null("q a top top_diff dq da", INVALID) + \
    each_null("dq da", INVALID, propagate_down0=0, propagate_down1=0) + \
    each_null("q top_diff da norm0 norm1", INVALID, dist_mode=0) + \
    each_null("a top dq W dW", INVALID, dist_mode=2, M=2) + \
    each_null("W dW dbias", INVALID, dist_mode=2, M=2, bias_term=1) + [
    ({"dist_mode": 2, "dW": None, "workspace": None}, INVALID),    # the arguments are judged before the workspace
    (SIMCROSS_BACKWARD.nulls(), INVALID),
]

SIMCROSS_FORWARD_BACKWARD = Form("dist_mode=1 N=3 W1=2 W2=5 D=4 M=1 q* a* W* bias* top_diff* top* norm0* norm1* dq* da* "
                                 "dW* dbias* workspace* workspace_bytes=0")
SIMCROSS_FORWARD_BACKWARD_ROWS = SIMCROSS_DIMS + [
    (SIMCROSS_FORWARD_BACKWARD.nulls(N=0), OK), (SIMCROSS_FORWARD_BACKWARD.nulls(N=0, dist_mode=2, M=3), OK),
    (SIMCROSS_FORWARD_BACKWARD.nulls(N=0, dist_mode=-1), INVALID),
] + each_null("q a top top_diff dq da", INVALID) + each_null("q top norm0 norm1", INVALID, dist_mode=0) + \
    each_null("q a top top_diff dq da W", INVALID, dist_mode=2, M=2) + [
    ({"dist_mode": 2, "W": None, "dW": None, "workspace": None}, INVALID),
    (SIMCROSS_FORWARD_BACKWARD.nulls(), INVALID),
]


@pytest.mark.parametrize("symbol", ["mms_simcross_forward_f32", "mms_simcross_forward_f64"])
def test_simcross_forward(hiplib, symbol):
    run(hiplib, symbol, SIMCROSS_FORWARD, SIMCROSS_FORWARD_ROWS)


@pytest.mark.parametrize("symbol", ["mms_simcross_backward_f32", "mms_simcross_backward_f64"])
def test_simcross_backward(hiplib, symbol):
    run(hiplib, symbol, SIMCROSS_BACKWARD, SIMCROSS_BACKWARD_ROWS)


def test_simcross_forward_backward(hiplib):
    run(hiplib, "mms_simcross_forward_backward_f32", SIMCROSS_FORWARD_BACKWARD, SIMCROSS_FORWARD_BACKWARD_ROWS)


@pytest.mark.parametrize("symbol, form, table", [
    ("mms_simcross_forward_block_f32", SIMCROSS_FORWARD, SIMCROSS_FORWARD_ROWS),
    ("mms_simcross_backward_block_f32", SIMCROSS_BACKWARD, SIMCROSS_BACKWARD_ROWS)], ids=["forward", "backward"])
def test_simcross_block_calls_judge_as_the_argument_lists_do(hiplib, symbol, form, table):
    from mms_answer_selection_amd import capi
    fn = getattr(hiplib, symbol)
    assert fn(None, None) == INVALID
    for row, code in table:
        block = capi.SimCrossArgs(**form.args(row))
        assert fn(C.addressof(block), None) == code, (symbol, row)


def test_simcross_workspace_queries_refuse_with_zero(hiplib):
    for row, code in SIMCROSS_DIMS:
        dims = list(SIMCROSS_FORWARD.args(row).values())[:6]
        assert code == INVALID
        assert hiplib.mms_simcross_workspace_bytes(*dims) == 0, row
        assert hiplib.mms_simcross_workspace_bytes_f64(*dims) == 0, row


# ---- fp16 storage, sentence-vector pairs (W1 == W2 == 1) ---------------------------------------------------------
ROWS_DIMS = [({"N": -1}, INVALID), ({"D": 0}, INVALID), ({"D": -1}, INVALID), ({"N": 2, "D": 2 ** 30}, INVALID),
             ({"N": 0, "D": 0}, INVALID), ({"N": 0}, OK)]
ROWS_F16 = {
    "mms_simcross_euclid_forward_f16": (Form("N=3 D=8 q_f16* a_f16* top*"), "q_f16 a_f16 top"),
    "mms_simcross_cosine_forward_f16": (Form("N=3 D=8 q_f16* a_f16* top* norm0* norm1*"), "q_f16 a_f16 top"),
    "mms_simcross_cosine_forward_backward_f16": (Form("N=3 D=8 q_f16* a_f16* top_diff* top* norm0* norm1* dq_f16* da_f16*"),
                                                 "q_f16 a_f16 top_diff top dq_f16 da_f16"),
    "mms_simcross_euclid_forward_backward_f16": (Form("N=3 D=8 q_f16* a_f16* top_diff* top* dq_f16* da_f16*"),
                                                 "q_f16 a_f16 top_diff top dq_f16 da_f16"),
}


@pytest.mark.parametrize("symbol", sorted(ROWS_F16))
def test_rows_f16(hiplib, symbol):
    form, required = ROWS_F16[symbol]
    run(hiplib, symbol, form, ROWS_DIMS + [(form.nulls(N=0), OK), (form.nulls(), INVALID), (form.nulls(N=-1), INVALID)] +
        each_null(required, INVALID))


# ---- fp16 storage, word grids, dist_mode 0 / 1 -------------------------------------------------------------------
GRID_F16 = {
    "mms_simcross_forward_f16": (Form("dist_mode=1 N=3 W1=2 W2=5 D=4 q_f16* a_f16* top* norm0* norm1*"), "q_f16 a_f16 top"),
    "mms_simcross_backward_f16": (Form("dist_mode=1 N=3 W1=2 W2=5 D=4 q_f16* a_f16* top* top_diff* norm0* norm1* dq_f16* "
                                       "da_f16*"), "q_f16 a_f16 top top_diff dq_f16 da_f16"),
    "mms_simcross_forward_backward_f16": (Form("dist_mode=1 N=3 W1=2 W2=5 D=4 q_f16* a_f16* top_diff* top* norm0* norm1* "
                                               "dq_f16* da_f16*"), "q_f16 a_f16 top_diff top dq_f16 da_f16"),
}


@pytest.mark.parametrize("symbol", sorted(GRID_F16))
def test_grid_f16(hiplib, symbol):
    form, required = GRID_F16[symbol]
    run(hiplib, symbol, form, MODE_RANGE + GRID_DIMS + [
        ({"dist_mode": 2}, UNSUPPORTED), ({"W1": 1, "W2": 1}, UNSUPPORTED), ({"dist_mode": 0, "W1": 1, "W2": 1}, UNSUPPORTED),
        ({"dist_mode": 2, "N": 0}, UNSUPPORTED), ({"W1": 1, "W2": 1, "N": 0}, UNSUPPORTED),
        (form.nulls(dist_mode=2), UNSUPPORTED), (form.nulls(W1=1, W2=1), UNSUPPORTED),
        ({"dist_mode": 2, "N": -1}, INVALID), ({"dist_mode": 2, "D": 0}, INVALID),        # INVALID before UNSUPPORTED
        ({"W1": 1, "W2": 1, "D": 0}, INVALID), ({"W1": 1, "W2": 1, "N": -1}, INVALID),
        ({"dist_mode": 3, "W1": 1, "W2": 1}, INVALID),
        ({"N": 0}, OK), (form.nulls(N=0), OK), (form.nulls(N=0, dist_mode=0), OK), (form.nulls(), INVALID),
    ] + each_null(required, INVALID) + each_null(required + " norm0 norm1", INVALID, dist_mode=0))


# ---- Embed-fused SimCross scoring --------------------------------------------------------------------------------
K_RULES = [({"K": 0}, INVALID), ({"K": -1}, INVALID), ({"K": 2 ** 16, "D": 2 ** 15}, INVALID)]      # K*D passes INT_MAX
EMBED_SIMCROSS = Form("dist_mode=1 N=3 W1=2 W2=5 D=4 K=7 index_q* index_a* table* embed_bias* top* norm0* norm1*")
EMBED_BILINEAR = Form("N=3 W1=2 W2=5 D=4 M=2 K=7 index_q* index_a* table* embed_bias* W* bias* top*")


@pytest.mark.parametrize("symbol", ["mms_embed_simcross_forward_f32", "mms_embed_simcross_forward_f16"])
def test_embed_simcross(hiplib, symbol):
    form = EMBED_SIMCROSS
    run(hiplib, symbol, form, GRID_DIMS + K_RULES + [
        ({"dist_mode": 2}, UNSUPPORTED), ({"dist_mode": 3}, UNSUPPORTED), ({"dist_mode": -1}, UNSUPPORTED),
        ({"dist_mode": 2, "N": -1}, UNSUPPORTED), ({"dist_mode": 2, "K": 0}, UNSUPPORTED),  # UNSUPPORTED before INVALID
        (form.nulls(dist_mode=2), UNSUPPORTED), ({"dist_mode": 2, "N": 0}, UNSUPPORTED),
        ({"N": 0}, OK), (form.nulls(N=0), OK), (form.nulls(N=0, dist_mode=0), OK), ({"N": 0, "K": 0}, INVALID),
        (form.nulls(), INVALID),
    ] + each_null("index_q index_a table top", INVALID) +
        each_null("index_q index_a table top norm0 norm1", INVALID, dist_mode=0))


@pytest.mark.parametrize("symbol", ["mms_embed_simcross_bilinear_forward_f32", "mms_embed_simcross_bilinear_forward_f16"])
def test_embed_bilinear(hiplib, symbol):
    form = EMBED_BILINEAR
    run(hiplib, symbol, form, GRID_DIMS + M_RANGE + K_RULES + [
        ({"N": 1, "W1": 2 ** 10, "W2": 2 ** 10, "D": 1, "M": 2 ** 11}, INVALID),
        ({"N": 0}, OK), (form.nulls(N=0), OK), ({"N": 0, "K": 0}, INVALID), ({"N": 0, "M": 0}, INVALID),
        (form.nulls(), INVALID),
    ] + each_null("index_q index_a table W top", INVALID))


# ---- SimMatrix ---------------------------------------------------------------------------------------------------
SIMMATRIX_DIMS = [({"N": -1}, INVALID), ({"K1": 0}, INVALID), ({"K1": -1}, INVALID), ({"K2": 0}, INVALID),
                  ({"K2": -1}, INVALID), ({"N": 0, "K1": 0}, INVALID), ({"N": 0, "K2": -1}, INVALID), ({"N": 0}, OK)]
_SM = "N=3 K1=4 K2=5 "
_WS = " workspace* workspace_bytes=%d" % AMPLE
_FLAGS = " param_propagate_down=1 propagate_down0=1 propagate_down1=1 dq* da* dW*"
SIMMATRIX = {
    "mms_simmatrix_forward_f32": (Form(_SM + "q* a* W* top* qw_scratch*"), "q a W top qw_scratch"),
    "mms_simmatrix_forward_f64": (Form(_SM + "q* a* W* top* qw_scratch*"), "q a W top qw_scratch"),
    "mms_simmatrix_forward_ws_f32": (Form(_SM + "q* a* W* top* qw_scratch*" + _WS), "q a W top qw_scratch"),
    "mms_simmatrix_forward_f16": (Form(_SM + "q_f16* a_f16* W* top*" + _WS), "q_f16 a_f16 W top"),
    "mms_simmatrix_forward_train_f16": (Form(_SM + "q_f16* a_f16* W* top* qw_scratch*" + _WS),
                                        "q_f16 a_f16 W top qw_scratch"),
    "mms_simmatrix_backward_f16": (Form(_SM + "q_f16* a_f16* W* qw* top_diff* dq_f16* da_f16* dW*" + _WS),
                                   "q_f16 a_f16 W top_diff"),
    "mms_simmatrix_backward_f32": (Form(_SM + "q* a* W* top_diff*" + _FLAGS + _WS), "q a W top_diff"),
    "mms_simmatrix_backward_cached_f32": (Form(_SM + "q* a* W* qw* top_diff*" + _FLAGS + _WS), "q a W qw top_diff"),
    "mms_simmatrix_backward_f64": (Form(_SM + "q* a* W* top_diff*" + _FLAGS), "q a W top_diff"),
}
PROPAGATE_DOWN = [
    ({"dW": None}, INVALID), ({"dq": None}, INVALID), ({"da": None}, INVALID),
    ({"param_propagate_down": 0, "dW": None, "dq": None}, INVALID),        # each flag asks for its own array only
    ({"propagate_down0": 0, "dq": None, "da": None}, INVALID),
    ({"propagate_down1": 0, "da": None, "dW": None}, INVALID),
    ({"param_propagate_down": 0, "propagate_down0": 0, "propagate_down1": 0, "q": None}, INVALID),
]


@pytest.mark.parametrize("symbol", sorted(SIMMATRIX))
def test_simmatrix(hiplib, symbol):
    form, required = SIMMATRIX[symbol]
    table = SIMMATRIX_DIMS + [(form.nulls(N=0), OK), (form.nulls(), INVALID), (form.nulls(N=-1), INVALID)] + \
        each_null(required, INVALID)
    if "param_propagate_down" in form.defaults:
        table = table + PROPAGATE_DOWN
    run(hiplib, symbol, form, table)


def test_simmatrix_workspace_rules(hiplib):
    form = SIMMATRIX["mms_simmatrix_forward_ws_f32"][0]
    need = hiplib.mms_simmatrix_workspace_bytes(3, 4, 5)
    assert need > 1
    run(hiplib, "mms_simmatrix_forward_ws_f32", form, [
        ({"workspace": None}, WORKSPACE), ({"workspace_bytes": need - 1}, WORKSPACE), ({"workspace_bytes": 0}, WORKSPACE),
        ({"workspace": None, "workspace_bytes": 0}, WORKSPACE),
        ({"workspace": None, "q": None}, INVALID), ({"workspace_bytes": need - 1, "qw_scratch": None}, INVALID),
        ({"workspace": None, "N": -1}, INVALID), ({"workspace": None, "K2": 0}, INVALID),   # INVALID before WORKSPACE
        ({"workspace": None, "workspace_bytes": 0, "N": 0}, OK),                           # the empty batch needs none
    ])
    for dims in ((-1, 4, 5), (3, 0, 5), (3, 4, -1)):
        assert hiplib.mms_simmatrix_workspace_bytes(*dims) == 0, dims
        assert hiplib.mms_triplet_simmatrix_workspace_bytes(*dims) == 0, dims
    assert hiplib.mms_triplet_simmatrix_workspace_bytes(0, 4, 5) == 0


# ---- PairRank ----------------------------------------------------------------------------------------------------
PAIRRANK_FORWARD = {
    "mms_pairrank_forward_f32": Form("count=4 margin=1.0 a* b* y* ordered* similar* loss*" + _WS),
    "mms_pairrank_forward_f64": Form("count=4 margin=1.0 a* b* y* ordered* similar* loss*"),
}
PAIRRANK_BACKWARD = Form("count=4 top_diff=1.0 y* ordered* similar* propagate_down0=1 propagate_down1=1 da* db*")


@pytest.mark.parametrize("symbol", sorted(PAIRRANK_FORWARD))
def test_pairrank_forward(hiplib, symbol):
    form = PAIRRANK_FORWARD[symbol]
    run(hiplib, symbol, form, [({"count": 0}, INVALID), ({"count": -1}, INVALID), (form.nulls(count=0), INVALID),
                               (form.nulls(), INVALID)] + each_null("a b y ordered similar loss", INVALID))


@pytest.mark.parametrize("symbol", ["mms_pairrank_backward_f32", "mms_pairrank_backward_f64"])
def test_pairrank_backward(hiplib, symbol):
    form = PAIRRANK_BACKWARD
    run(hiplib, symbol, form, [
        ({"count": 0}, INVALID), ({"count": -1}, INVALID), (form.nulls(count=0), INVALID), (form.nulls(), INVALID),
        ({"da": None}, INVALID), ({"db": None}, INVALID),
        ({"propagate_down0": 0, "da": None, "db": None}, INVALID), ({"propagate_down1": 0, "da": None, "db": None}, INVALID),
        ({"propagate_down0": 0, "propagate_down1": 0, "y": None}, INVALID),
    ] + each_null("y ordered similar", INVALID))


# ---- the fused triplet steps -------------------------------------------------------------------------------------
TRIPLET_SIMMATRIX = Form("N=3 K1=4 K2=5 margin=1.0 loss_weight=1.0 q* a_pos* a_neg* y* W* s_pos* s_neg* loss* dq* da_pos* "
                         "da_neg* dW*" + _WS)
TRIPLET_EUCLID = Form("N=3 D=8 margin=1.0 loss_weight=1.0 q* a_pos* a_neg* y* s_pos* s_neg* loss* dq* da_pos* da_neg*" + _WS)
TRIPLET_COSINE = Form("N=3 D=8 margin=1.0 loss_weight=1.0 q* a_pos* a_neg* y* s_pos* s_neg* norm_q* norm_pos* norm_neg* "
                      "loss* dq* da_pos* da_neg*" + _WS)
TRIPLET_ROWS_DIMS = [({"N": -1}, INVALID), ({"D": 0}, INVALID), ({"D": -1}, INVALID), ({"N": 2, "D": 2 ** 30}, INVALID)]
TRIPLET_REQUIRED = "q a_pos a_neg y s_pos s_neg dq da_pos da_neg"


def test_triplet_simmatrix_step(hiplib):
    form = TRIPLET_SIMMATRIX
    need = hiplib.mms_triplet_simmatrix_workspace_bytes(3, 4, 5)
    assert need > 1
    run(hiplib, "mms_triplet_simmatrix_step_f32", form, [
        ({"N": 0}, INVALID), (form.nulls(N=0), INVALID), ({"N": -1}, INVALID), ({"K1": 0}, INVALID), ({"K1": -1}, INVALID),
        ({"K2": 0}, INVALID), ({"K2": -1}, INVALID),
        ({"N": 2 ** 16, "K1": 2 ** 15, "K2": 1}, INVALID),            # N*K1 alone passes INT_MAX
        ({"N": 2 ** 16, "K1": 1, "K2": 2 ** 15}, INVALID),            # N*K2 alone
        (form.nulls(), INVALID),
        ({"workspace": None}, WORKSPACE), ({"workspace_bytes": need - 1}, WORKSPACE), ({"workspace_bytes": 0}, WORKSPACE),
        ({"loss": None, "workspace": None}, WORKSPACE),               # loss may be NULL
        ({"workspace": None, "q": None}, INVALID), ({"workspace_bytes": need - 1, "dW": None}, INVALID),
        ({"workspace": None, "N": 0}, INVALID), ({"workspace": None, "K1": 0}, INVALID),     # INVALID before WORKSPACE
    ] + each_null(TRIPLET_REQUIRED + " W dW", INVALID))


def test_triplet_euclid_step(hiplib):
    form = TRIPLET_EUCLID
    need = hiplib.mms_triplet_workspace_bytes(3)
    assert need == 1056 * 8 + 3 * 4
    run(hiplib, "mms_triplet_euclid_step_f32", form, TRIPLET_ROWS_DIMS + [
        ({"N": 0}, INVALID), (form.nulls(N=0), INVALID), (form.nulls(), INVALID),
        ({"workspace": None}, WORKSPACE), ({"workspace_bytes": need - 1}, WORKSPACE), ({"workspace_bytes": 0}, WORKSPACE),
        ({"workspace": P + 4}, WORKSPACE),                            # the arrival words are 8-byte words
        ({"loss": None, "workspace": None}, WORKSPACE),               # loss may be NULL
        ({"workspace": None, "q": None}, INVALID), ({"workspace": None, "D": 0}, INVALID),   # INVALID before WORKSPACE
    ] + each_null(TRIPLET_REQUIRED, INVALID))


def test_triplet_cosine_step(hiplib):
    form = TRIPLET_COSINE
    need = hiplib.mms_triplet_workspace_bytes(3)
    run(hiplib, "mms_triplet_cosine_step_f32", form, TRIPLET_ROWS_DIMS + [
        ({"N": 0}, OK), (form.nulls(N=0), OK), (form.nulls(N=0, workspace_bytes=0), OK), ({"N": 0, "D": 0}, INVALID),
        (form.nulls(), INVALID),
        ({"workspace": None}, WORKSPACE), ({"workspace_bytes": need - 1}, WORKSPACE), ({"workspace": P + 4}, WORKSPACE),
        ({"loss": None, "norm_q": None, "norm_pos": None, "norm_neg": None, "workspace": None}, WORKSPACE),   # optional
        ({"workspace": None, "dq": None}, INVALID), ({"workspace": None, "N": -1}, INVALID),  # INVALID before WORKSPACE
    ] + each_null(TRIPLET_REQUIRED, INVALID))


def test_triplet_workspace_init(hiplib):
    init = hiplib.mms_triplet_workspace_init
    for ws, nbytes in ((None, 0), (None, AMPLE), (P, 1056 * 8 - 1), (P, 0), (P + 4, AMPLE)):
        assert init(ws, nbytes, None) == WORKSPACE, (ws, nbytes)
    for n in (0, -1):
        assert hiplib.mms_triplet_workspace_bytes(n) == 0 and hiplib.mms_pairrank_workspace_bytes(n) == 0
        assert hiplib.mms_rank_workspace_bytes(n) == 0


# ---- ranking metrics (f32; the _f64 twins: tests/test_abi_f64_embed_rank.py) -------------------------------------
RANK = {
    "mms_rank_map_mrr_f32": (Form("n=5 fixed_axis=0 prob* label* group* map_out* mrr_out* effective_out*" + _WS), [
        ({"n": 0}, INVALID), ({"n": -1}, INVALID), ({"fixed_axis": -1}, INVALID),
        ({"n": 2 ** 16, "fixed_axis": 2 ** 15 - 1}, INVALID),         # n*(fixed_axis+1) passes INT_MAX
    ] + each_null("prob label group", INVALID)),
    "mms_rank_auc_f32": (Form("n=5 dim=3 fixed_axis=1 prob* label* has_ignore_label=0 ignore_label=0 auc_out*" + _WS), [
        ({"n": 0}, INVALID), ({"n": -1}, INVALID), ({"dim": 0}, INVALID), ({"dim": -1}, INVALID),
        ({"fixed_axis": -1}, INVALID), ({"fixed_axis": 3}, INVALID), ({"fixed_axis": 4}, INVALID),
        ({"n": 2 ** 16, "dim": 2 ** 15}, INVALID),
    ] + each_null("prob label auc_out", INVALID)),
    "mms_rank_auc_nd_f32": (Form("outer=2 channels=3 inner=2 fixed_axis=1 prob* label* has_ignore_label=0 ignore_label=0 "
                                 "auc_out*" + _WS), [
        ({"outer": 0}, INVALID), ({"outer": -1}, INVALID), ({"channels": 0}, INVALID), ({"channels": -1}, INVALID),
        ({"inner": 0}, INVALID), ({"inner": -1}, INVALID), ({"fixed_axis": -1}, INVALID), ({"fixed_axis": 3}, INVALID),
        ({"outer": 2 ** 11, "channels": 2 ** 10, "inner": 2 ** 10}, INVALID),
    ] + each_null("prob label auc_out", INVALID)),
    "mms_rank_accuracy_f32": (Form("count=4 a* b* label* acc_out*" + _WS), [
        ({"count": 0}, INVALID), ({"count": -1}, INVALID)] + each_null("a b label acc_out", INVALID)),
}


@pytest.mark.parametrize("symbol", sorted(RANK))
def test_rank(hiplib, symbol):
    form, table = RANK[symbol]
    first = next(iter(form.defaults))
    run(hiplib, symbol, form, table + [(form.nulls(), INVALID), (form.nulls(**{first: 0}), INVALID)])


# ---- Embed (f32; the _f64 and _f16 twins have suites of their own) -----------------------------------------------
EMBED_DIMS = [({"M": -1}, INVALID), ({"N": 0}, INVALID), ({"N": -1}, INVALID), ({"K": 0}, INVALID), ({"K": -1}, INVALID),
              ({"M": 2 ** 16, "N": 2 ** 15}, INVALID), ({"M": 0, "K": 0}, INVALID), ({"M": 0}, OK)]
EMBED_FORWARD = Form("M=6 N=2 K=7 index* weight* bias* top*")
EMBED_BACKWARD = Form("M=6 N=2 K=7 index* top_diff* weight_diff* bias_diff*" + _WS)
PAIR_DIMS = [({"M0": 0}, INVALID), ({"M0": -1}, INVALID), ({"M1": 0}, INVALID), ({"M1": -1}, INVALID), ({"N": 0}, INVALID),
             ({"N": -1}, INVALID), ({"K": 0}, INVALID), ({"K": -1}, INVALID),
             ({"M0": 2 ** 30, "M1": 2 ** 30, "N": 1}, INVALID),       # (M0+M1)*N passes INT_MAX
             ({"M0": 2 ** 15, "M1": 2 ** 15, "N": 2 ** 15}, INVALID)]
EMBED_FORWARD_PAIR = Form("M0=3 M1=4 N=2 K=7 index0* index1* weight* bias* top0* top1* index_workspace* "
                          "index_workspace_bytes=%d" % AMPLE)
EMBED_BACKWARD_PAIR = Form("M0=3 M1=4 N=2 K=7 index0* top_diff0* index1* top_diff1* weight_diff* bias_diff*" + _WS)
NO_OUTPUT = {"weight_diff": None, "bias_diff": None}


def test_embed_forward(hiplib):
    form = EMBED_FORWARD
    run(hiplib, "mms_embed_forward_f32", form, EMBED_DIMS + [(form.nulls(M=0), OK), (form.nulls(), INVALID)] +
        each_null("index weight top", INVALID))


def test_embed_backward(hiplib):
    form = EMBED_BACKWARD
    run(hiplib, "mms_embed_backward_f32", form, EMBED_DIMS + [
        (form.nulls(M=0), OK), (NO_OUTPUT, OK), (form.nulls(), OK),                # no gradient asked for: nothing to do
        (dict(NO_OUTPUT, N=0), INVALID), (dict(NO_OUTPUT, M=-1), INVALID),
        ({"weight_diff": None, "index": None}, INVALID), ({"bias_diff": None, "top_diff": None}, INVALID),
    ] + each_null("index top_diff", INVALID))


def test_embed_forward_pair(hiplib):
    form = EMBED_FORWARD_PAIR
    run(hiplib, "mms_embed_forward_pair_f32", form, PAIR_DIMS + [(form.nulls(), INVALID)] +
        each_null("index0 index1 weight top0 top1", INVALID))


@pytest.mark.parametrize("symbol", ["mms_embed_backward_pair_f32", "mms_embed_backward_pair_indexed_f32"])
def test_embed_backward_pair(hiplib, symbol):
    form = EMBED_BACKWARD_PAIR
    beyond_the_index = {"M0": 4096, "M1": 1}                      # what mms_embed_pair_index_supported rejects
    assert hiplib.mms_embed_pair_index_supported(4096, 1, 7) == 0
    assert hiplib.mms_embed_pair_index_supported(4095, 1, 7) == 1
    assert hiplib.mms_embed_pair_index_supported(0, 1, 7) == 0 and hiplib.mms_embed_pair_index_supported(3, 4, 0) == 0
    indexed = symbol.endswith("indexed_f32")
    table = PAIR_DIMS + [(NO_OUTPUT, OK), (dict(NO_OUTPUT, K=0), INVALID), (dict(NO_OUTPUT, index0=None), INVALID),
                         (form.nulls(), INVALID), (dict(beyond_the_index, top_diff1=None), INVALID),
                         (dict(beyond_the_index, M1=2 ** 30, N=2), INVALID)] + \
        each_null("index0 top_diff0 index1 top_diff1", INVALID)
    if indexed:
        table = table + [(beyond_the_index, UNSUPPORTED), (dict(beyond_the_index, **NO_OUTPUT), UNSUPPORTED)]
    else:
        table = table + [(dict(beyond_the_index, **NO_OUTPUT), OK)]
    run(hiplib, symbol, form, table)


# ---- Net glue ----------------------------------------------------------------------------------------------------
def test_feed_gather_rows(hiplib):
    form = Form("rows=3 row_elems=4 src_rows=10 src* perm* first=2 dst*")
    run(hiplib, "mms_feed_gather_rows_f32", form, [
        ({"rows": -1}, INVALID), ({"row_elems": 0}, INVALID), ({"row_elems": -1}, INVALID), ({"src_rows": 0}, INVALID),
        ({"src_rows": -1}, INVALID), ({"first": -1}, INVALID),
        ({"rows": 2 ** 16, "row_elems": 2 ** 15, "src_rows": 2 ** 17}, INVALID),              # rows*row_elems
        ({"first": 8}, INVALID), ({"first": 10, "rows": 1}, INVALID),                         # first+rows > src_rows
        ({"first": 2 ** 31 - 1, "rows": 1, "src_rows": 2 ** 31 - 1}, INVALID),                # ... beyond an int
        ({"rows": 0}, OK), (form.nulls(rows=0), OK), (form.nulls(rows=0, first=10), OK),
        (form.nulls(rows=0, first=11), INVALID), (form.nulls(rows=0, row_elems=0), INVALID),
        (form.nulls(), INVALID), ({"src": None}, INVALID), ({"dst": None}, INVALID),
        ({"perm": None, "dst": None}, INVALID),                                               # perm may be NULL
    ])


def test_split_backward(hiplib):
    fn = hiplib.mms_split_backward_f32
    tops = (C.c_void_p * 3)(P, P + 64, P + 128)
    hole = (C.c_void_p * 3)(P, None, P + 128)
    last = (C.c_void_p * 9)(*([P] * 8 + [None]))
    for args, code in [
            ((-1, 3, tops, P + 256), INVALID), ((5, 0, tops, P + 256), INVALID), ((5, -1, tops, P + 256), INVALID),
            ((5, 3, None, P + 256), INVALID), ((0, 3, None, None), INVALID), ((5, 3, tops, None), INVALID),
            ((5, 3, hole, P + 256), INVALID), ((5, 9, last, P + 256), INVALID), ((5, 3, hole, None), INVALID),
            ((0, 3, tops, P + 256), OK), ((0, 3, tops, None), OK), ((0, 3, hole, None), OK), ((0, 0, tops, None), INVALID)]:
        assert fn(*args, None) == code, args


@pytest.mark.parametrize("symbol", ["mms_dot_f32", "mms_dot_f64"])
def test_dot(hiplib, symbol):
    fn = getattr(hiplib, symbol)
    for args in [(-1, P, P + 64, P + 128), (5, P, P + 64, None), (0, None, None, None), (5, None, P + 64, P + 128),
                 (5, P, None, P + 128), (5, None, None, None), (-1, None, None, None)]:
        assert fn(*args, None) == INVALID, args


def test_null_launch(hiplib):
    assert hiplib.mms_null_launch(0, None) == INVALID and hiplib.mms_null_launch(-1, None) == INVALID


# ---- the mode setters: a value outside the range is refused and the mode stays ------------------------------------
@pytest.mark.parametrize("stem", ["matrix", "euclid_backward", "pairrank_hinge", "triplet_finish", "loss_sum", "rank_tie",
                                  "f16_distance"])
def test_mode_setters(hiplib, stem):
    setter, getter = getattr(hiplib, "mms_set_%s_mode" % stem), getattr(hiplib, "mms_get_%s_mode" % stem)
    before = getter()
    assert before in (0, 1)
    try:
        for held in (0, 1):
            assert setter(held) == OK and getter() == held
            for outside in (-1, 2, 7, -2 ** 31):
                assert setter(outside) == INVALID and getter() == held, (held, outside)
    finally:
        assert setter(before) == OK and getter() == before
