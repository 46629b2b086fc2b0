"""The numpy restatement of ops.wide_bn_act (tests/_wide_bn_ref.py) held to fp64
torch.nn.BatchNorm1d + relu under autograd on the live rows, and the recorded conditions of the
reference fixtures nsbn_regnn_* (tests/golden/make_golden_bn.py). No GPU."""
import numpy as np
import pytest
import torch

import _golden as G
import _wide_bn_ref as R

TOL = 1e-12
STATE = [123, 2, 0, 9, 0, 0, 0, 0]


def _case(n, H, seed):
    rng = np.random.default_rng(seed)
    mu, sd = rng.uniform(-8, 8, H), rng.uniform(0.5, 2, H)
    x = rng.standard_normal((n, H)) * sd + mu
    rs = rng.uniform(0.5, 1.5, n)
    bias = rng.standard_normal(H) * 0.1
    res = rng.standard_normal((n, H))
    gamma = rng.uniform(0.5, 1.5, H) * rng.choice([-1.0, 1.0], H)
    beta = rng.standard_normal(H) * 0.3
    gy = rng.standard_normal((n, H))
    return x, rs, bias, res, gamma, beta, gy


def _close(tag, got, want):
    err = float(np.abs(np.asarray(got) - np.asarray(want)).max())
    scale = max(1.0, float(np.abs(np.asarray(want)).max()))
    assert err <= TOL * scale, f"{tag}: {err:.3e}"


@pytest.mark.parametrize("n,live,H", [(300, 300, 8), (300, 137, 36), (300, 2, 16), (50, 31, 64)])
@pytest.mark.parametrize("opt", [True, False])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_restatement_matches_torch_batchnorm(n, live, H, opt, p):
    """forward, every gradient and the three buffers against fp64 BatchNorm1d (training mode) +
    relu + the mask under autograd on the first `live` rows; zeros past them"""
    x, rs, bias, res, gamma, beta, gy = _case(n, H, 1000 * H + live)
    if not opt:
        rs = bias = res = None
    w = R.drop_weight(STATE, 1, n, H, p)
    rm0, rv0 = np.linspace(-1, 1, H), np.linspace(0.5, 2, H)
    y, c = R.forward(x, gamma, beta, live, rs, bias, res, w)
    g = R.backward(gy, c)
    rm, rv, nbt = R.buffers(c, rm0, rv0, 5)

    bn = torch.nn.BatchNorm1d(H).double()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma))
        bn.bias.copy_(torch.from_numpy(beta))
        bn.running_mean.copy_(torch.from_numpy(rm0))
        bn.running_var.copy_(torch.from_numpy(rv0))
        bn.num_batches_tracked.fill_(5)
    bn.train()
    tx = torch.from_numpy(x[:live].copy()).requires_grad_()
    tb = torch.from_numpy(np.zeros(H) if bias is None else bias.copy()).requires_grad_()
    tr = torch.from_numpy(np.zeros((live, H)) if res is None else res[:live].copy()).requires_grad_()
    a = tx * (1.0 if rs is None else torch.from_numpy(rs[:live, None])) + tb + tr
    ty = torch.relu(bn(a)) * torch.from_numpy(w[:live])
    ty.backward(torch.from_numpy(gy[:live]))
    _close("y", y[:live], ty.detach().numpy())
    assert not y[live:].any() and not g["gx"][live:].any() and not g["gres"][live:].any()
    _close("gx", g["gx"][:live], tx.grad.numpy())
    _close("gres", g["gres"][:live], tr.grad.numpy())
    _close("g_gamma", g["g_gamma"], bn.weight.grad.numpy())
    _close("g_beta", g["g_beta"], bn.bias.grad.numpy())
    # the conv bias's gradient: 0 in the restatement, rounding noise of a cancelling sum in torch
    assert not g["g_bias"].any()
    assert float(tb.grad.abs().max()) <= 1e-10 * max(1.0, float(np.abs(gy).sum(0).max()))
    _close("running_mean", rm, bn.running_mean.numpy())
    _close("running_var", rv, bn.running_var.numpy())
    assert nbt == int(bn.num_batches_tracked) == 6


def test_restatement_fewer_than_two_rows():
    """live = 1 and 0: variance 0, finite outputs, the buffers untouched"""
    x, rs, bias, res, gamma, beta, gy = _case(20, 8, 3)
    for live in (1, 0):
        y, c = R.forward(x, gamma, beta, live, rs, bias, res)
        g = R.backward(gy, c)
        assert np.isfinite(y).all() and all(np.isfinite(v).all() for v in g.values())
        assert not y[live:].any() and not g["gx"].any()      # one row: ga = 0
        rm, rv, nbt = R.buffers(c, np.ones(8), np.full(8, 2.0), 4)
        assert (rm == 1).all() and (rv == 2).all() and nbt == 4
    y, _ = R.forward(x, gamma, beta, 1, rs, bias, res)
    np.testing.assert_allclose(y[0], np.maximum(beta, 0), atol=1e-15)


def test_mask_is_the_step_spec():
    """drop_weight is the fused step's hash mask of (state, layer): 0 or 1 / keep, keyed on both"""
    w = R.drop_weight(STATE, 1, 64, 16, 0.5)
    assert set(np.unique(w)) == {0.0, 2.0}
    assert not np.array_equal(w, R.drop_weight(STATE, 0, 64, 16, 0.5))
    assert np.array_equal(R.drop_weight(STATE, 1, 64, 16, 0.0), np.ones((64, 16)))


def test_separate_moves_inputs_off_the_corner():
    x, rs, bias, res, gamma, beta, _ = _case(300, 16, 9)
    x = x.astype(np.float32)
    R.separate(x, gamma, beta, 137, rs, bias, res)
    _, c = R.forward(x, gamma, beta, 137, rs, bias, res)
    assert np.abs(c["pre"]).min() >= 1e-3


@pytest.mark.parametrize("name", ["nsbn_regnn_h64_res1", "nsbn_regnn_h128_res0"])
def test_fixture_conditions(name):
    """the recorded conditions: training-mode 'bn', every layer's live targets >= 2, the outer
    block has padded rows on the device sampler, the parameter names are mag.REGNN's, the conv
    BatchNorms stepped once and the model-level one (unused in the forward) not at all"""
    from regnn_hip import mag
    d = G.load(name)
    m = d["meta"]
    assert m["use_norm"] == "bn" and m["training"] and m["dropout"] == 0.0
    assert m["residual"] == name.endswith("res1")
    B = len(d["batch"])
    assert B == 32 and m["sizes"] == [25, 20] and m["classes"] == 7
    live = [int(d[f"adj{h}_size"][1]) for h in range(2)]
    assert live == m["live"] and all(v >= 2 for v in live)
    assert live[0] < B * (m["sizes"][0] + 1) and live[1] == B
    assert sum(m["counts"]) == 354
    counts, K = m["counts"], m["in_channels"]
    model = mag.REGNN(K, m["hidden"], m["classes"], m["num_layers"], m["scaling_factor"], 0.0,
                      {t: K for t in range(4)}, m["num_edge_types"], residual=m["residual"],
                      use_norm="bn", self_loop_type=2, feats_type=m["feats_type"],
                      num_nodes_dict={t: counts[t] for t in range(4)}, target_node_type=0)
    assert {n for n, _ in model.named_parameters()} == set(G.sub(d, "p_"))
    bufs = G.sub(d, "buf_")
    assert {n for n, _ in model.named_buffers()} == set(bufs)
    for i in range(2):
        assert int(bufs[f"convs.{i}.norm.num_batches_tracked"]) == 1
        assert np.abs(bufs[f"convs.{i}.norm.running_var"] - 1).max() > 0
    assert int(bufs["norm.num_batches_tracked"]) == 0
