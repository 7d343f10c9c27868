"""Layer<double> of Embed, MRR, AUC and RankAccuracy in the C++ mirror (MAP stays float-only there: an earlier test
pins it as the unregistered type): each created by type string from its
prototxt, driven end to end by mms_layer_run_f64 (SetUp / Forward / Backward over Blob<double>) at one small shape, and
compared word for word with the C-ABI call it binds."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(hiplib):
    from mms_answer_selection_amd import layers
    layers.lib()
    layers.set_mode_gpu()
    return layers


@pytest.fixture(scope="module")
def capi(hiplib):
    from mms_answer_selection_amd import capi
    return capi


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float64)).cuda()


def words(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64).ravel()


def metric_inputs(n=90, groups=6, seed=5):
    r = np.random.default_rng(seed)
    prob = r.standard_normal((n, 2))
    prob[:, 1] = r.permutation(n) / float(n)
    label = (r.uniform(size=n) < 0.3).astype(np.float64)
    group = r.integers(0, groups, n).astype(np.float64)
    return prob, label, group


def test_embed_double_layer(L, capi):
    r = np.random.default_rng(41)
    K, N = 11, 6
    index = r.integers(0, K, (7, 5)).astype(np.float64)
    weight, bias = r.standard_normal((K, N)), r.standard_normal(N)
    dT = r.standard_normal((7, 5, N))
    wd0, bd0 = r.standard_normal((K, N)), r.standard_normal(N)
    proto = ('layer { name: "e" type: "Embed" bottom: "i" top: "t" '
             'embed_param { num_output: %d input_dim: %d bias_term: true } }' % (N, K))
    top, _, (wd, bd) = L.run_layer_f64(proto, [index], top_diff=dT, params=[weight, bias], param_diffs=[wd0, bd0],
                                       propagate_down=[False])
    assert top.shape == (7, 5, N)
    t = torch.empty((35, N), dtype=torch.float64, device="cuda")
    capi.embed_forward_f64(dev(index), dev(weight), t, bias=dev(bias))
    assert (words(top) == words(t.cpu().numpy())).all()
    wd_abi, bd_abi = dev(wd0), dev(bd0)
    capi.embed_backward_f64(dev(index), dev(dT), wd_abi, bd_abi)
    assert (words(wd) == words(wd_abi.cpu().numpy())).all()          # both parameter diffs come back, accumulated
    assert (words(bd) == words(bd_abi.cpu().numpy())).all()
    assert not (words(wd) == words(wd0)).all() and not (words(bd) == words(bd0)).all()


def test_mrr_double_layer(L, capi):
    prob, label, group = metric_inputs()
    proto = 'layer { name: "m" type: "MRR" bottom: "p" bottom: "l" bottom: "g" top: "t" }'
    top, _, _ = L.run_layer_f64(proto, [prob, label, group], propagate_down=[False, False, False])
    assert top.shape == ()                                             # a zero-axis top
    _, rr, _ = capi.rank_map_mrr_f64(dev(prob), dev(label), dev(group), 1)
    assert words(top)[0] == words(rr)[0]


def test_auc_double_layer_with_two_tops(L, capi):
    prob, label, _ = metric_inputs(seed=6)
    proto = 'layer { name: "a" type: "AUC" bottom: "p" bottom: "l" top: "auc" top: "extra" }'
    top, _, _ = L.run_layer_f64(proto, [prob, label], propagate_down=[False, False])
    assert top.size == 1
    assert words(top)[0] == words(capi.rank_auc_f64(dev(prob), dev(label), 1))[0]


def test_rank_accuracy_double_layer(L, capi):
    r = np.random.default_rng(43)
    a, b = r.standard_normal((77, 1)), r.standard_normal((77, 1))
    y = r.choice(np.array([-1.0, 0.0, 1.0]), (77, 1))
    proto = 'layer { name: "r" type: "RankAccuracy" bottom: "a" bottom: "b" bottom: "y" top: "t" }'
    top, _, _ = L.run_layer_f64(proto, [a, b, y], propagate_down=[False, False, False])
    assert words(top)[0] == words(capi.rank_accuracy_f64(dev(a), dev(b), dev(y)))[0]


def test_float_registry_is_unchanged(L):
    assert sorted(L.registered_layer_types()) == ["AUC", "Embed", "HDF5Data", "MAP", "MRR", "PairRankLoss", "RankAccuracy", "SimCross",
                                  "SimMatrix"]
