"""GPU checks of NS REGATv2 training on device-sampled blocks (regnn_ns_gatv2_fwd / _bwd,
ops.ns_gatv2, mag.REGATv2Conv on an NSBlock and NSTrainer(device_blocks=True) with
mag.GATV2_BLOCKS on):

1. per-element fp64 parity of ops.ns_gatv2, forward and backward, on the padded ladder block
   (rows of 1 .. 65 entries in a 64-row block of 40 live rows) under _attention_ref.rel_err <=
   TOL_F32, over the six shapes x two recipes and one shape per further register tier of the
   backward (_ns_gatv2_blocks.WIDTH_SHAPES); out past the live rows and g_xs past the live
   sources exactly zero;
2. mag.REGATv2Conv on the padded block of the mag_regatv2conv_* fixtures against the fixture
   arrays and against the conv's own exact-size call, 1e-5;
3. two forward runs give the same bits (out and a), two backward runs the same g_xd, g_att, g_tab;
4. one NSTrainer(device_blocks=True) step against NeighborSampler + mag.train_step on the same
   batch (loss and every parameter gradient, 1e-5), also with a batch shorter than its capacity;
5. capture() succeeds (a host sync inside a capture raises) and six replays track six eager steps;
6. the configurations the blocks do not cover are refused with ValueError / TypeError;
7. with the knob off the conv still refuses a block (NotImplementedError) and the trainer the
   model (ValueError).
"""
import numpy as np
import pytest
import torch

import _attention_ref as R
import _golden as G
import _ns_gat_blocks as B
import _ns_gatv2_blocks as V
import test_gpu_ns_gat as T        # its _mag / _model / _trainer recipe (the graph is built once)

pytestmark = pytest.mark.gpu
DEV = "cuda"

_DEVBLK = {}


@pytest.fixture
def knob_on(monkeypatch):
    from regnn_hip import mag
    monkeypatch.setitem(mag.GATV2_BLOCKS, "mode", "on")


def _ladder():
    if not _DEVBLK:
        _DEVBLK["blk"] = V.ladder_block().to(DEV)
    return _DEVBLK["blk"]


def _leaves(recipe, H, C):
    xs, xd, att, tab, gy, slope = V.ladder_case(recipe, H, C)
    return [t.to(DEV).requires_grad_(True) for t in (xs, xd, att, tab)], gy.to(DEV), slope


CASES = [(r, H, C) for H, C in V.SHAPES for r in V.RECIPES] + \
        [("unit", H, C) for H, C in V.WIDTH_SHAPES]


@pytest.mark.parametrize("recipe,H,C", CASES)
def test_ns_gatv2_matches_fp64_per_element(recipe, H, C):
    from regnn_hip import ops
    c = B.LADDER
    want, scale = V.ladder_ref(recipe, H, C)
    leaves, gy, slope = _leaves(recipe, H, C)
    out = ops.ns_gatv2(_ladder(), *leaves, slope)
    out.backward(gy)
    got = dict(zip(V.KEYS, [out] + [t.grad for t in leaves]))
    errs = {}
    for k in V.KEYS:
        g = got[k].detach().cpu()
        assert bool(torch.isfinite(g).all()), k
        errs[k] = R.rel_err(g, want[k], scale[k])
    print(f"ns_gatv2 {recipe} H={H} C={C}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert not out[c["live_dst"]:].any()
    assert not got["g_xs"][c["live_src"]:].any()
    for k, v in errs.items():
        assert v <= R.TOL_F32, f"{k}: {v:.3e}"


def _fixture_conv(d):
    from regnn_hip import mag
    m = d["meta"]
    H, C = m["heads"], m["out_channels"]
    conv = mag.REGATv2Conv(H * C, C, m["num_node_types"], m["num_edge_types"], heads=H,
                           scaling_factor=m["scaling_factor"], residual=m["residual"],
                           use_norm=m["use_norm"], self_loop_type=2)
    P = G.sub(d, "p_", np.float32)
    with torch.no_grad():
        for n, p in conv.named_parameters():
            p.copy_(torch.from_numpy(P[n]))
    return conv.to(DEV)


@pytest.mark.parametrize("name", V.FIXTURES)
def test_regatv2conv_on_padded_block_matches_fixture_and_exact_path(name, knob_on):
    d = G.load(name)
    m = d["meta"]
    n_src, n_dst = m["n_src"], m["n_dst"]
    blk = B.fixture_block(d).to(DEV)
    conv = _fixture_conv(d)
    x = torch.full((blk.n_src, d["x"].shape[1]), 1e3, device=DEV)
    x[:n_src] = torch.from_numpy(d["x"]).to(DEV)
    x.requires_grad_(True)
    out = conv((x, x[:blk.n_dst]), blk)
    gout = torch.zeros(blk.n_dst, out.shape[1], device=DEV)
    gout[:n_dst] = torch.from_numpy(d["gout"]).to(DEV)
    out.backward(gout)
    got = {"out": out[:n_dst].detach(), "x": x.grad[:n_src].clone()}
    got.update({n: p.grad.clone() for n, p in conv.named_parameters()})
    assert not x.grad[n_src:].any()
    want = {"out": d["out"], **G.sub(d, "grad_")}
    assert set(want) == set(got)
    # the exact-size call on the same fixture (the path the block replaces)
    conv.zero_grad()
    x2 = torch.from_numpy(d["x"]).to(DEV).requires_grad_(True)
    ei = torch.from_numpy(np.stack([d["src"], d["dst"]])).to(DEV)
    out2 = conv((x2, x2[:n_dst]), ei, torch.from_numpy(d["edge_type"]).to(DEV),
                torch.from_numpy(d["target_node_type"]).to(DEV))
    out2.backward(torch.from_numpy(d["gout"]).to(DEV))
    exact = {"out": out2.detach(), "x": x2.grad}
    exact.update({n: p.grad for n, p in conv.named_parameters()})
    for k in want:
        g = got[k].float().cpu().numpy()
        ok, err = G.close(g, want[k], 1e-5)
        ok2, err2 = G.close(g, exact[k].float().cpu().numpy(), 1e-5)
        print(f"{name} {k}: fixture {err:.2e} exact path {err2:.2e}")
        assert ok, f"{k} vs fixture: rel err {err:.3e}"
        assert ok2, f"{k} vs exact-size path: rel err {err2:.3e}"


def test_forward_and_backward_bitwise_reproducible():
    from regnn_hip import ops
    dev = _ladder()
    E = dev.E
    runs = []
    for _ in range(2):
        leaves, gy, slope = _leaves("unit", 8, 64)
        out, a = ops.ns_gatv2(dev, *leaves, slope, return_attn=True)
        out.backward(gy)
        runs.append((out.detach(), a[:E], leaves[1].grad, leaves[2].grad, leaves[3].grad))
    (o1, a1, *g1), (o2, a2, *g2) = runs
    assert torch.equal(o1, o2) and torch.equal(a1, a2)
    assert not a1.requires_grad
    assert bool(torch.isfinite(a1).all()) and float(a1.max()) <= 1.0
    for name, x, y in zip(("g_xd", "g_att", "g_tab"), g1, g2):
        assert torch.equal(x, y), name


@pytest.mark.parametrize("n_train", [None, 37])
def test_trainer_device_blocks_match_pyg_path(n_train, knob_on):
    """n_train = 37: the batch holds fewer targets than its capacity (sizes[0] < B)"""
    from regnn_hip import mag
    from regnn_hip.sampler import NeighborSampler
    d = T._mag()
    idx = torch.arange(d["n_paper"] if n_train is None else n_train, device=DEV)
    m_api, m_eng = T._model(d, model="regatv2"), T._model(d, model="regatv2")
    m_api.train(); m_eng.train()
    smp = NeighborSampler(d["rg"], idx, [6, 4], batch_size=64, shuffle=True, seed=3)
    batch = next(iter(smp))
    loss_api = mag.train_step(m_api, torch.optim.SGD(m_api.parameters(), lr=0.0), batch,
                              d["x_dict"], d["edge_type"], d["node_type"], d["local"], d["y"], 1)
    tr = T._trainer(d, m_eng, train_idx=idx, device_blocks=True)
    assert tr._gat_blocks and tr.fused is None and tr.pipelined
    assert tr.ahead == 1 and len(tr.slots) == 2
    tr._forward_backward()
    torch.cuda.synchronize()
    la = float(loss_api.detach())
    print(f"loss {float(tr.loss):.7f} against {la:.7f}")
    assert abs(float(tr.loss) - la) <= 1e-5 * max(1.0, abs(la))
    assert int(tr.sampler.sizes[0]) == (64 if n_train is None else n_train)
    gp = dict(m_api.named_parameters())
    for n, p in m_eng.named_parameters():
        if gp[n].grad is None:                 # declared, unused in forward (REGNN.norm)
            assert not p.grad.any(), n
            continue
        ok, err = G.close(p.grad.cpu().numpy(), gp[n].grad.cpu().numpy().astype(np.float64), 1e-5)
        print(f"{n}: rel err {err:.2e}")
        assert ok, f"{n}: rel err {err:.3e}"


def test_trainer_device_blocks_capture_and_replay(knob_on):
    d = T._mag()
    tr_e = T._trainer(d, T._model(d, model="regatv2"), device_blocks=True)
    tr_g = T._trainer(d, T._model(d, model="regatv2"), device_blocks=True)
    tr_g.capture(warmup=1)                     # a host sync inside the capture would raise
    assert not tr_g.graph_groups               # one-step graphs only
    le, lg = [], []
    for _ in range(6):
        tr_e.step()
        le.append(float(tr_e.loss))
        tr_g.replay()
        lg.append(float(tr_g.loss))
    print("eager", le, "replayed", lg)
    assert np.all(np.isfinite(lg))
    assert np.allclose(le, lg, rtol=1e-4, atol=1e-5), (le, lg)
    assert tr_g.edges_total() > 0


@pytest.mark.parametrize("kw", [dict(use_norm="bn"), dict(self_loop_type=1)])
def test_device_blocks_refusals(kw, knob_on):
    d = T._mag()
    with pytest.raises(ValueError):
        T._trainer(d, T._model(d, model="regatv2", **kw), device_blocks=True)


def test_device_blocks_refuse_bf16_tables(knob_on):
    d = dict(T._mag())
    d["x_dict"] = {k: v.bfloat16() for k, v in d["x_dict"].items()}
    with pytest.raises(ValueError):
        T._trainer(d, T._model(d, model="regatv2"), device_blocks=True)


def test_conv_refuses_return_weights_on_a_block(knob_on):
    d = G.load(V.FIXTURES[0])
    blk = B.fixture_block(d).to(DEV)
    conv = _fixture_conv(d)
    x = torch.zeros(blk.n_src, d["x"].shape[1], device=DEV)
    with pytest.raises(ValueError):
        conv((x, x[:blk.n_dst]), blk, return_weights=True)


def test_ops_refuses_other_dtypes_and_strided_blocks():
    from regnn_hip import ops
    dev = _ladder()
    (xs, xd, att, tab), _gy, slope = _leaves("unit", 2, 32)
    with pytest.raises(TypeError):
        ops.ns_gatv2(dev, xs.detach().bfloat16(), xd, att, tab, slope)
    strided = dev.to(DEV)
    strided.strided_rows = (None, 7)
    with pytest.raises(ValueError):
        ops.ns_gatv2(strided, xs, xd, att, tab, slope)


def test_knob_off_keeps_the_refusals(monkeypatch):
    from regnn_hip import mag
    monkeypatch.setitem(mag.GATV2_BLOCKS, "mode", "off")
    d = G.load(V.FIXTURES[0])
    blk = B.fixture_block(d).to(DEV)
    conv = _fixture_conv(d)
    x = torch.zeros(blk.n_src, d["x"].shape[1], device=DEV)
    with pytest.raises(NotImplementedError):
        conv((x, x[:blk.n_dst]), blk)
    g = T._mag()
    with pytest.raises(ValueError):
        T._trainer(g, T._model(g, model="regatv2"), device_blocks=True)
