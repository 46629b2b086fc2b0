"""ops.wide_bn_act (regnn_wide_bn_fwd / _bwd: BatchNorm1d in training mode over the live rows of a
capacity-sized block, then relu and the hash dropout) against its fp64 restatement
(tests/_wide_bn_ref.py, itself held to torch.nn.BatchNorm1d by test_cpu_wide_bn.py):

1. every width tier (the generic one at 8, 16, 36) x live in {n, 137, 2}, with and without
   rs / bias / res, p in {0, 0.5}; one case of 40 000 rows (past one grid pass of the statistics
   launch: the grid stride and a full 512-row slab merge); 1e-5 x max(1, max|ref|) (G.close);
2. live = 1; 3. bitwise reproducibility; 4. a captured graph replayed with a new device count;
5. the dropout mask is wide_ln_act's; 6. refusals."""
import functools

import numpy as np
import pytest
import torch

import _golden as G
import _wide_bn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5
STATE = [123, 2, 0, 9, 0, 0, 0, 0]
WIDTHS = [8, 16, 36, 64, 128, 256, 512, 1024]


@functools.lru_cache(maxsize=None)
def _inputs(n, H, live, opt):
    """fp32 inputs (numpy), column means in [-8, 8] and standard deviations in [0.5, 2], moved off
    the relu's corner for this live count (R.separate)"""
    rng = np.random.default_rng(7919 * H + 31 * live + n + int(opt))
    mu, sd = rng.uniform(-8, 8, H), rng.uniform(0.5, 2, H)
    d = dict(x=(rng.standard_normal((n, H)) * sd + mu).astype(np.float32),
             gamma=(rng.uniform(0.5, 1.5, H) * rng.choice([-1.0, 1.0], H)).astype(np.float32),
             beta=rng.uniform(-0.3, 0.3, H).astype(np.float32),
             gy=rng.standard_normal((n, H)).astype(np.float32),
             rm=rng.uniform(-1, 1, H).astype(np.float32),
             rv=rng.uniform(0.5, 2, H).astype(np.float32), rs=None, bias=None, res=None)
    if opt:
        d.update(rs=rng.uniform(0.5, 1.5, n).astype(np.float32),
                 bias=(rng.standard_normal(H) * 0.1).astype(np.float32),
                 res=rng.standard_normal((n, H)).astype(np.float32))
    R.separate(d["x"], d["gamma"], d["beta"], live, d["rs"], d["bias"], d["res"])
    return d


def _bn(d, H, momentum=0.1, eps=1e-5):
    bn = torch.nn.BatchNorm1d(H, eps=eps, momentum=momentum).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(d["gamma"]))
        bn.bias.copy_(torch.from_numpy(d["beta"]))
        bn.running_mean.copy_(torch.from_numpy(d["rm"]))
        bn.running_var.copy_(torch.from_numpy(d["rv"]))
        bn.num_batches_tracked.fill_(5)
    return bn.train()


def _t(a, grad=False):
    return None if a is None else torch.from_numpy(a).to(DEV).requires_grad_(grad)


def _run(d, H, live, p, n=None, live_t=None):
    """one forward + backward on the device -> dict of tensors, the BatchNorm module"""
    from regnn_hip import ops
    bn = _bn(d, H)
    x, bias, res = _t(d["x"], True), _t(d["bias"], True), _t(d["res"], True)
    state = torch.tensor(STATE, dtype=torch.int64, device=DEV)
    lv = live_t if live_t is not None else \
        (None if live is None else torch.tensor([live], dtype=torch.int32, device=DEV))
    assert ops.wide_bn_ok(x, bn, bias)
    y = ops.wide_bn_act(x, bias, bn, p, state, 1, rs=_t(d["rs"]), res=res, live=lv)
    y.backward(_t(d["gy"]))
    out = dict(y=y.detach(), gx=x.grad, g_gamma=bn.weight.grad, g_beta=bn.bias.grad,
               running_mean=bn.running_mean, running_var=bn.running_var)
    if res is not None:
        out["gres"] = res.grad
    if bias is not None:
        out["g_bias"] = bias.grad
    return out, bn


def _ref(d, H, live, p):
    n = d["x"].shape[0]
    w = R.drop_weight(STATE, 1, n, H, p)
    y, c = R.forward(d["x"], d["gamma"], d["beta"], live, d["rs"], d["bias"], d["res"], w)
    want = R.backward(d["gy"], c)
    want["y"] = y
    want["running_mean"], want["running_var"], want["nbt"] = R.buffers(c, d["rm"], d["rv"], 5)
    return want


def _compare(got, bn, want, live):
    for k, v in got.items():
        if k == "g_bias":
            assert not v.any(), "g_bias must be exactly 0"
            continue
        ok, err = G.close(v.double().cpu().numpy(), want[k], TOL)
        print(f"{k}: rel err {err:.3e}")
        assert ok, f"{k}: rel err {err:.3e}"
    for k in ("y", "gx", "gres"):
        if k in got:
            assert not got[k][live:].any(), f"{k} past the live rows"
    assert int(bn.num_batches_tracked) == want["nbt"]


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("opt", [True, False])
@pytest.mark.parametrize("live", [300, 137, 2])
@pytest.mark.parametrize("H", WIDTHS)
def test_wide_bn_matches_restatement(H, live, opt, p):
    d = _inputs(300, H, live, opt)
    got, bn = _run(d, H, live, p)
    want = _ref(d, H, live, p)
    assert want["nbt"] == 6
    _compare(got, bn, want, live)


def test_wide_bn_null_live_is_every_row():
    d = _inputs(300, 36, 300, True)
    got, bn = _run(d, 36, None, 0.5)
    _compare(got, bn, _ref(d, 36, 300, 0.5), 300)


def test_wide_bn_many_rows():
    """40 000 rows of 64 (16 rows per block: 2500 blocks' worth on the 512-block statistics
    launch, so its grid strides and all 512 slab rows merge), 33 333 live"""
    n, live, H = 40000, 33333, 64
    d = _inputs(n, H, live, True)
    got, bn = _run(d, H, live, 0.5)
    _compare(got, bn, _ref(d, H, live, 0.5), live)


@pytest.mark.parametrize("H", [16, 512])
def test_wide_bn_one_live_row(H):
    """live = 1: variance 0 by definition, finite outputs, the three buffers untouched"""
    d = _inputs(300, H, 2, True)
    got, bn = _run(d, H, 1, 0.0)
    for k, v in got.items():
        assert torch.isfinite(v).all(), k
    assert not got["y"][1:].any() and not got["gx"].any()
    assert torch.equal(bn.running_mean.cpu(), torch.from_numpy(d["rm"]))
    assert torch.equal(bn.running_var.cpu(), torch.from_numpy(d["rv"]))
    assert int(bn.num_batches_tracked) == 5
    want = _ref(d, H, 1, 0.0)
    ok, err = G.close(got["y"].double().cpu().numpy(), want["y"], TOL)
    assert ok, err


@pytest.mark.parametrize("H,n,live", [(36, 300, 137), (1024, 300, 300), (64, 40000, 33333)])
def test_wide_bn_bitwise_reproducible(H, n, live):
    d = _inputs(n, H, live, True)
    a, _ = _run(d, H, live, 0.5)
    b, _ = _run(d, H, live, 0.5)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_wide_bn_graph_replay_with_new_count():
    """forward + backward captured once at live = 137; the count tensor rewritten to 211 and the
    graph replayed equals an eager call at 211 (every launch reads the count on the device)"""
    from regnn_hip import ops
    H, n = 128, 300
    d = _inputs(n, H, 137, True)
    bn = _bn(d, H)
    x, bias, res = _t(d["x"], True), _t(d["bias"], True), _t(d["res"], True)
    rs, gy = _t(d["rs"]), _t(d["gy"])
    state = torch.tensor(STATE, dtype=torch.int64, device=DEV)
    live = torch.tensor([137], dtype=torch.int32, device=DEV)
    ins = [x, bias, res, bn.weight, bn.bias]

    def body():
        y = ops.wide_bn_act(x, bias, bn, 0.5, state, 1, rs=rs, res=res, live=live)
        return (y,) + torch.autograd.grad(y, ins, gy)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = body()
    live.fill_(211)
    with torch.no_grad():
        bn.running_mean.copy_(torch.from_numpy(d["rm"]))
        bn.running_var.copy_(torch.from_numpy(d["rv"]))
        bn.num_batches_tracked.fill_(5)
    g.replay()
    torch.cuda.synchronize()
    got, bn2 = _run(d, H, 211, 0.5)
    for a, k in zip(outs, ["y", "gx", "g_bias", "gres", "g_gamma", "g_beta"]):
        assert torch.equal(a, got[k]), k
    assert not outs[0][211:].any() and outs[0][137:211].any()
    assert torch.equal(bn.running_mean, bn2.running_mean)
    assert torch.equal(bn.running_var, bn2.running_var)
    assert int(bn.num_batches_tracked) == int(bn2.num_batches_tracked) == 6


def test_wide_bn_dropout_mask_is_wide_ln_acts():
    """p = 0.5: the zero pattern equals wide_ln_act's for the same (state, layer), compared where
    both undropped activations are positive"""
    from regnn_hip import ops
    H, n = 64, 300
    d = _inputs(n, H, 300, False)
    state = torch.tensor(STATE, dtype=torch.int64, device=DEV)
    x = _t(d["x"])
    ln = torch.nn.LayerNorm(H).to(DEV)
    ys = {}
    for p in (0.0, 0.5):
        ys["bn", p] = ops.wide_bn_act(x, None, _bn(d, H), p, state, 3)
        ys["ln", p] = ops.wide_ln_act(x, None, ln, p, state, 3).detach()
    both = (ys["bn", 0.0] > 0) & (ys["ln", 0.0] > 0)
    assert int(both.sum()) > 1000
    zb, zl = (ys["bn", 0.5] == 0)[both], (ys["ln", 0.5] == 0)[both]
    assert torch.equal(zb, zl)
    assert zb.any() and not zb.all()
    w = torch.from_numpy(R.drop_weight(STATE, 3, n, H, 0.5)).to(DEV)
    assert torch.equal(zb, (w == 0)[both])


def test_wide_bn_refusals():
    from regnn_hip import _lib as L
    from regnn_hip import ops
    for H in (6, 1028):
        x = torch.zeros(8, H, device=DEV)
        bn = torch.nn.BatchNorm1d(H).to(DEV)
        assert not ops.wide_bn_ok(x, bn)
        with pytest.raises(ValueError, match="width"):
            ops.wide_bn_act(x, None, bn)
        a, y, st = torch.empty_like(x), torch.empty_like(x), torch.empty(2, H, device=DEV)
        slab = torch.empty(512, 3 * H, device=DEV)
        sums = torch.empty(2, H, device=DEV)
        p = lambda t: L.ptr(t)                                   # noqa: E731
        s = torch.cuda.current_stream().cuda_stream
        rc = L._so.regnn_wide_bn_fwd(8, H, p(x), None, None, None, p(bn.weight), p(bn.bias), None,
                                     0, 0.0, p(a), p(st), p(y), p(slab), None, p(bn.running_mean),
                                     p(bn.running_var), p(bn.num_batches_tracked), 1e-5, 0.1, 1, s)
        assert rc == 2                                           # REGNN_EUNSUPPORTED
        rc = L._so.regnn_wide_bn_bwd(8, H, p(y), p(a), p(st), None, p(bn.weight), p(bn.bias), None,
                                     0, 0.0, p(x), None, p(slab), p(sums), None, 1, s)
        assert rc == 2
        assert int(bn.num_batches_tracked) == 0
    x = torch.zeros(8, 16, device=DEV)
    assert ops.wide_bn_ok(x, torch.nn.BatchNorm1d(16).to(DEV))
    for kw in (dict(momentum=None), dict(affine=False), dict(track_running_stats=False)):
        bn = torch.nn.BatchNorm1d(16, **kw).to(DEV)
        assert not ops.wide_bn_ok(x, bn), kw
        with pytest.raises(ValueError):
            ops.wide_bn_act(x, None, bn)
    with pytest.raises(ValueError, match="training"):
        ops.wide_bn_act(x, None, torch.nn.BatchNorm1d(16).to(DEV).eval())
