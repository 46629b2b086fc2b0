"""GPU checks of NS REGAT training on device-sampled blocks (regnn_ns_gat_fwd / _bwd, ops.ns_gat,
mag.REGATConv on an NSBlock, NSTrainer(device_blocks=True)):

1. per-element fp64 parity of ops.ns_gat, forward and backward, on a padded ladder block (rows of
   1 .. 65 entries in a 64-row block of 40 live rows) under _attention_ref.rel_err <= TOL_F32;
2. mag.REGATConv on the padded block of the mag_regatconv_* fixtures against the fixture arrays
   and against the exact-size conv call, 1e-5;
3. two forward runs give the same bits (out and a);
4. one NSTrainer(device_blocks=True) step against NeighborSampler + mag.train_step on the same
   batch (loss and every parameter gradient, 1e-5), also with a batch shorter than its capacity;
5. capture() succeeds (a host sync inside a capture raises) and six replays track six eager steps;
6. the configurations the blocks do not cover are refused with ValueError.
"""
import numpy as np
import pytest
import torch

import _attention_ref as R
import _golden as G
import _ns_gat_blocks as B

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURES = ["mag_regatconv_h2_res1", "mag_regatconv_h4_res0"]
SHAPES = [(1, 64), (2, 32), (4, 16), (8, 64), (8, 8), (3, 8)]

_LADDER = {}


def _ladder():
    """the ladder block, built once: (CPU block, device block)"""
    if not _LADDER:
        blk = B.ladder_block()
        _LADDER["blk"] = (blk, blk.to(DEV))
    return _LADDER["blk"]


def _ladder_case(recipe, H, C):
    c = B.LADDER
    ft, el, er, tab, gy, slope = R.gat_inputs(recipe, c["cap_src"], H, C, c["n_rel"],
                                              seed=100 + 7 * H + C)
    er, gy = er[:c["cap_dst"]].clone(), gy[:c["cap_dst"]].clone()
    gy[c["live_dst"]:] = 0.0                                  # no gradient into the padded rows
    return ft, el, er, tab, gy, slope


@pytest.mark.parametrize("recipe", ["unit", "wide"])
@pytest.mark.parametrize("H,C", SHAPES)
def test_ns_gat_matches_fp64_per_element(recipe, H, C):
    from regnn_hip import ops
    c = B.LADDER
    cpu, dev = _ladder()
    ft, el, er, tab, gy, slope = _ladder_case(recipe, H, C)
    ptr, idx, rel = cpu.live()
    want, scale = R.gat_case_ref(ptr, idx, rel, el, er, tab, ft, gy, slope,
                                 global_max="detached")
    leaves = [t.to(DEV).requires_grad_(True) for t in (el, er, tab, ft)]
    out = ops.ns_gat(dev, *leaves, slope)
    out.backward(gy.to(DEV))
    got = {"out": out, "g_el": leaves[0].grad, "g_er": leaves[1].grad, "g_tab": leaves[2].grad,
           "g_ft": leaves[3].grad}
    errs = {}
    for k in ("out", "g_ft", "g_el", "g_er", "g_tab"):
        g = got[k].detach().cpu()
        assert bool(torch.isfinite(g).all()), k
        errs[k] = R.rel_err(g, want[k], scale[k])
    print(f"ns_gat {recipe} H={H} C={C}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert not out[c["live_dst"]:].any()
    assert not got["g_ft"][c["live_src"]:].any() and not got["g_el"][c["live_src"]:].any()
    for k, v in errs.items():
        assert v <= R.TOL_F32, f"{k}: {v:.3e}"


def _fixture_conv(d):
    from regnn_hip import mag
    m = d["meta"]
    H, C = m["heads"], m["out_channels"]
    conv = mag.REGATConv(H * C, C, m["num_node_types"], m["num_edge_types"], heads=H,
                         scaling_factor=m["scaling_factor"], residual=m["residual"],
                         use_norm=m["use_norm"], self_loop_type=2)
    P = G.sub(d, "p_", np.float32)
    with torch.no_grad():
        for n, p in conv.named_parameters():
            p.copy_(torch.from_numpy(P[n]))
    return conv.to(DEV)


@pytest.mark.parametrize("name", FIXTURES)
def test_regatconv_on_padded_block_matches_fixture_and_exact_path(name):
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


def test_block_refusals_of_the_convs():
    from regnn_hip import mag
    d = G.load(FIXTURES[0])
    blk = B.fixture_block(d).to(DEV)
    conv = _fixture_conv(d)
    x = torch.zeros(blk.n_src, d["x"].shape[1], device=DEV)
    with pytest.raises(ValueError):
        conv((x, x[:blk.n_dst]), blk, return_weights=True)
    m = d["meta"]
    v2 = mag.REGATv2Conv(64, m["out_channels"], 4, 7, heads=m["heads"], self_loop_type=2).to(DEV)
    with pytest.raises(NotImplementedError):
        v2((x, x[:blk.n_dst]), blk)


def test_forward_bitwise_reproducible():
    from regnn_hip import ops
    _, dev = _ladder()
    ft, el, er, tab, _gy, slope = [t.to(DEV) if torch.is_tensor(t) else t
                                   for t in _ladder_case("unit", 8, 64)]
    with torch.no_grad():
        o1, a1 = ops.ns_gat(dev, el, er, tab, ft, slope, return_attn=True)
        o2, a2 = ops.ns_gat(dev, el, er, tab, ft, slope, return_attn=True)
    E = dev.E
    assert torch.equal(o1, o2) and torch.equal(a1[:E], a2[:E])
    assert bool(torch.isfinite(a1[:E]).all()) and float(a1[:E].max()) <= 1.0


def test_ops_refuses_other_dtypes_and_strided_blocks():
    from regnn_hip import ops
    _, dev = _ladder()
    ft, el, er, tab, _gy, slope = [t.to(DEV) if torch.is_tensor(t) else t
                                   for t in _ladder_case("unit", 2, 32)]
    with pytest.raises(TypeError):
        ops.ns_gat(dev, el, er, tab, ft.bfloat16(), slope)
    strided = dev.to(DEV)
    strided.strided_rows = (None, 7)
    with pytest.raises(ValueError):
        ops.ns_gat(strided, el, er, tab, ft, slope)


# ---- the trainer --------------------------------------------------------------------------------
_MAG = {}


def _mag():
    """synth.mag_like(0.003, seed=1) as test_gpu_ns_engine._mag builds it, once"""
    if _MAG:
        return _MAG
    from regnn_hip import synth
    from regnn_hip.graph import RelGraph
    gd = synth.mag_like(0.003, seed=1, device=DEV)
    keep = gd["rel"] <= 7
    rg = RelGraph(gd["src"][keep], gd["dst"][keep], gd["N"], DEV)
    edge_type = gd["rel"][keep].to(torch.int64) - 1
    node_type = gd["ntype"]
    offs = torch.tensor([gd["type_offsets"][t] for t in synth.NTYPES], device=DEV)
    local = torch.arange(gd["N"], device=DEV) - offs[node_type]
    feats = synth.type_features(gd["counts"], {t: 16 for t in synth.NTYPES}, seed=1, device=DEV)
    x_dict = {k: f for k, f in enumerate(feats)}
    n_paper = gd["counts"]["paper"]
    y = torch.full((gd["N"], 1), -1, dtype=torch.int64, device=DEV)
    y[:n_paper, 0] = (torch.arange(n_paper, device=DEV) * 7) % 5
    _MAG.update(rg=rg, edge_type=edge_type, node_type=node_type, local=local, x_dict=x_dict, y=y,
                n_paper=n_paper)
    return _MAG


def _model(d, model="regat", **kw):
    from regnn_hip import mag
    torch.manual_seed(0)
    kw = {"use_norm": "ln", "self_loop_type": 2, **kw}
    return mag.REGNN(16, 8, 5, 2, 10.0, 0.0, {k: 16 for k in d["x_dict"]}, 7, model=model,
                     heads=2, **kw).to(DEV)


def _trainer(d, model, train_idx=None, **kw):
    from regnn_hip.ns import NSTrainer
    opt = torch.optim.Adam(model.parameters(), lr=1e-2, capturable=True)
    idx = torch.arange(d["n_paper"], device=DEV) if train_idx is None else train_idx
    return NSTrainer(model, opt, d["rg"], [6, 4], 64, idx, d["x_dict"], d["edge_type"],
                     d["node_type"], d["local"], d["y"], 7, seed=3, **kw)


@pytest.mark.parametrize("n_train", [None, 37])
def test_trainer_device_blocks_match_pyg_path(n_train):
    """n_train = 37: the batch holds fewer targets than its capacity (sizes[0] < B)"""
    from regnn_hip import mag
    from regnn_hip.sampler import NeighborSampler
    d = _mag()
    idx = torch.arange(d["n_paper"] if n_train is None else n_train, device=DEV)
    m_api, m_eng = _model(d), _model(d)
    m_api.train(); m_eng.train()
    smp = NeighborSampler(d["rg"], idx, [6, 4], batch_size=64, shuffle=True, seed=3)
    batch = next(iter(smp))
    loss_api = mag.train_step(m_api, torch.optim.SGD(m_api.parameters(), lr=0.0), batch,
                              d["x_dict"], d["edge_type"], d["node_type"], d["local"], d["y"], 1)
    tr = _trainer(d, m_eng, train_idx=idx, device_blocks=True)
    assert tr.fused is None and tr.pipelined and tr.ahead == 1 and len(tr.slots) == 2
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


def test_trainer_device_blocks_capture_and_replay():
    d = _mag()
    tr_e = _trainer(d, _model(d), device_blocks=True)
    tr_g = _trainer(d, _model(d), device_blocks=True)
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


@pytest.mark.parametrize("kw", [dict(model="regatv2"), dict(use_norm="bn"),
                                dict(self_loop_type=1)])
def test_device_blocks_refusals(kw):
    d = _mag()
    with pytest.raises(ValueError):
        _trainer(d, _model(d, **kw), device_blocks=True)


def test_device_blocks_flag_changes_nothing_for_regcn():
    d = _mag()
    a = _trainer(d, _model(d, model="regcn"), device_blocks=True)
    b = _trainer(d, _model(d, model="regcn"))
    assert (a.fused is None) == (b.fused is None) and a.ahead == b.ahead
    assert len(a.slots) == len(b.slots) and not a._gat_blocks
