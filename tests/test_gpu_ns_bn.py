"""NSTrainer on 'regcn' models with use_norm 'bn': the capacity-sized blocks' BatchNorm takes its
statistics over the live rows (ops.wide_bn_act), never over the padded ones.

7. loss, every gradient and every BatchNorm buffer against the reference's own REGNN class in
   training mode (tests/golden/make_golden_bn.py), 1e-5 x max(1, max|ref|);
8. one module step against NeighborSampler + mag.train_step (exact-size blocks, torch's
   BatchNorm1d) on the same batch, also with fewer targets than the batch capacity;
9. captured and replayed steps track eager ones, running buffers included;
10. no silent fall-back: a width the operator does not cover, and engine="fused", raise.

Before ops.wide_bn_act existed tests 7 and 8 failed: the module path ran torch's BatchNorm1d over
every row of the capacity-sized blocks."""
import numpy as np
import pytest
import torch

import _golden as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5


def _check(tag, got, want, tol=TOL):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    ok, err = G.close(got, np.asarray(want, np.float64), tol)
    print(f"{tag}: rel err {err:.3e}")
    assert ok, f"{tag}: rel err {err:.3e}"


# ---- 7. the reference's REGNN with batch norm ---------------------------------------------------
def _golden_model(d):
    from regnn_hip import mag
    m = d["meta"]
    counts, K = m["counts"], m["in_channels"]
    model = mag.REGNN(K, m["hidden"], m["classes"], m["num_layers"], m["scaling_factor"], 0.0,
                      {t: K for t in range(4)}, m["num_edge_types"], residual=m["residual"],
                      use_norm="bn", self_loop_type=2, feats_type=m["feats_type"],
                      num_nodes_dict={t: counts[t] for t in range(4)}, target_node_type=0)
    P = G.sub(d, "p_", np.float32)
    assert {n for n, _ in model.named_parameters()} == set(P)
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(torch.from_numpy(P[n]))
    return model.to(DEV)


@pytest.mark.parametrize("name", ["nsbn_regnn_h64_res1", "nsbn_regnn_h128_res0"])
def test_bn_module_step_vs_reference(name):
    """the device sampler reproduces the fixture's batch; NSTrainer(engine="module") on it, with
    the default knobs, gives the reference's loss, gradients and BatchNorm buffers"""
    from regnn_hip.graph import RelGraph
    from regnn_hip.ns import NSTrainer
    d = G.load(name)
    m = d["meta"]
    N = int(sum(m["counts"]))
    rg = RelGraph(torch.from_numpy(d["src"]), torch.from_numpy(d["dst"]), N, DEV)
    model = _golden_model(d)
    model.train()
    x_dict = {t: torch.from_numpy(d[f"x{t}"]).to(DEV) for t in range(4)}
    nt, loc = torch.from_numpy(d["ntype"]).to(DEV), torch.from_numpy(d["local"]).to(DEV)
    batch = torch.from_numpy(d["batch"]).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2, capturable=True)
    tr = NSTrainer(model, opt, rg, m["sizes"], len(d["batch"]), batch, x_dict,
                   torch.from_numpy(d["edge_type"]).to(DEV), nt, loc,
                   torch.from_numpy(d["y"]).to(DEV).view(-1, 1), m["num_edge_types"],
                   seed=m["seed"], shuffle=False, engine="module", pipeline=False)
    assert tr.fused is None and tr._blocks_ok
    s = tr.slots[0]
    # the fixture's batch, as NSTrainer._sample draws one (its own batch index instead of the
    # epoch's next)
    s.set_seed(m["seed"], m["epoch"], m["batch_idx"])
    s.set_targets(batch)
    s.run_hops(meta_only=tr._module_lean, strided=False)
    L_ = len(m["sizes"])
    for h in range(L_):                  # hop h's block = the fixture's adjs, outermost first
        n_dst = int(d[f"adj{L_ - 1 - h}_size"][1])
        assert int(s.sizes[h]) == n_dst
        assert s.blocks[h].live_rows is not None
    assert int(s.sizes[L_ - 1]) < s.blocks[L_ - 1].n_dst          # the outer block has padding
    tr._module_step(s)
    torch.cuda.synchronize()
    _check("loss", tr.loss, d["loss"])
    got = {n: p.grad for n, p in model.named_parameters()}
    for k, v in G.sub(d, "grad_").items():
        _check(k, got[k], v)
    bufs = dict(model.named_buffers())
    want = G.sub(d, "buf_")
    assert set(want) == set(bufs)
    for k, v in want.items():
        if k.endswith("num_batches_tracked"):
            assert int(bufs[k]) == int(v), k
        else:
            _check(k, bufs[k], v)


# ---- 8.-10. a synthetic ogbn-mag-like graph -----------------------------------------------------
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


def _model(d, hidden=16, residual=False, dropout=0.0, **kw):
    from regnn_hip import mag
    torch.manual_seed(0)
    kw = {"use_norm": "bn", "self_loop_type": 2, **kw}
    m = mag.REGNN(16, hidden, 5, 2, 10.0, dropout, {k: 16 for k in d["x_dict"]}, 7, model="regcn",
                  residual=residual, **kw).to(DEV)
    with torch.no_grad():
        for conv in m.convs:
            conv.bias.normal_(0, 0.1)
            if kw["use_norm"] == "bn":
                conv.norm.weight.normal_(1, 0.2)
                conv.norm.bias.normal_(0, 0.2)
    return m


def _trainer(d, model, train_idx=None, **kw):
    from regnn_hip.ns import NSTrainer
    opt = torch.optim.Adam(model.parameters(), lr=1e-2, capturable=True)
    idx = torch.arange(d["n_paper"], device=DEV) if train_idx is None else train_idx
    return NSTrainer(model, opt, d["rg"], [6, 4], 64, idx, d["x_dict"], d["edge_type"],
                     d["node_type"], d["local"], d["y"], 7, seed=3, **kw)


@pytest.mark.parametrize("n_train", [None, 37])
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("hidden", [16, 64])
def test_bn_module_step_matches_exact_size_path(hidden, residual, n_train):
    """n_train = 37: the batch holds fewer targets than its capacity (sizes[0] < B), so the last
    layer's block has padded rows too"""
    from regnn_hip import mag
    from regnn_hip.sampler import NeighborSampler
    d = _mag()
    idx = torch.arange(d["n_paper"] if n_train is None else n_train, device=DEV)
    m_api, m_eng = _model(d, hidden, residual), _model(d, hidden, residual)
    m_api.train(); m_eng.train()
    smp = NeighborSampler(d["rg"], idx, [6, 4], batch_size=64, shuffle=True, seed=3)
    batch = next(iter(smp))
    loss_api = mag.train_step(m_api, torch.optim.SGD(m_api.parameters(), lr=0.0), batch,
                              d["x_dict"], d["edge_type"], d["node_type"], d["local"], d["y"], 1)
    tr = _trainer(d, m_eng, train_idx=idx, engine="module")
    assert tr.fused is None and tr._blocks_ok
    tr._forward_backward()
    torch.cuda.synchronize()
    la = float(loss_api.detach())
    print(f"loss {float(tr.loss):.7f} against {la:.7f}")
    assert abs(float(tr.loss) - la) <= TOL * max(1.0, abs(la))
    assert int(tr.sampler.sizes[0]) == (64 if n_train is None else n_train)
    assert int(tr.sampler.sizes[1]) < tr.sampler.blocks[1].n_dst
    gp = dict(m_api.named_parameters())
    for n, p in m_eng.named_parameters():
        if gp[n].grad is None:                 # declared, unused in forward (REGNN.norm)
            assert not p.grad.any(), n
            continue
        _check(n, p.grad, gp[n].grad.cpu().numpy())
    ba = dict(m_api.named_buffers())
    for n, b in m_eng.named_buffers():
        if n.endswith("num_batches_tracked"):
            assert int(b) == int(ba[n]) == (1 if n.startswith("convs.") else 0), n
        else:
            _check(n, b, ba[n].cpu().numpy())


def test_bn_capture_and_replay_tracks_eager():
    d = _mag()
    m_e, m_g = _model(d, 64, True, dropout=0.5), _model(d, 64, True, dropout=0.5)
    m_e.train(); m_g.train()
    tr_e = _trainer(d, m_e, engine="module")
    tr_g = _trainer(d, m_g, engine="module")
    tr_g.capture(warmup=1)                     # a host sync inside the capture would raise
    le, lg = [], []
    for _ in range(6):
        tr_e.step()
        le.append(float(tr_e.loss))
        tr_g.replay()
        lg.append(float(tr_g.loss))
    print("eager", le, "replayed", lg)
    assert np.all(np.isfinite(lg))
    assert np.allclose(le, lg, rtol=1e-4, atol=1e-5), (le, lg)
    be = dict(m_e.named_buffers())
    for n, b in m_g.named_buffers():
        if n.endswith("num_batches_tracked"):
            assert int(b) == int(be[n]) == (6 if n.startswith("convs.") else 0), n
        else:
            assert torch.allclose(b, be[n], rtol=1e-4, atol=1e-5), n


def test_bn_no_silent_fallback():
    d = _mag()
    with pytest.raises(ValueError, match="use_norm 'bn'"):
        _trainer(d, _model(d, hidden=6), engine="module")
    m = _model(d, hidden=16)
    m.convs[1].norm = torch.nn.BatchNorm1d(16, momentum=None).to(DEV)
    with pytest.raises(ValueError, match="momentum"):
        _trainer(d, m)
    with pytest.raises(ValueError, match="fused"):
        _trainer(d, _model(d, hidden=64), engine="fused")
    # a covered width builds, on the module engine ("auto" falls to it: the fused step has no bn)
    tr = _trainer(d, _model(d, hidden=16))
    assert tr.fused is None and tr._blocks_ok
