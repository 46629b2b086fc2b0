"""The fused two-layer NS step with residual convs (regnn_nsm_params.residual: each conv adds
x_target @ W before its LayerNorm, mag/regnn_layers.py:101-107,131-132):

* loss and every gradient against the reference's own REGNN class with residual=True
  (tests/golden/make_golden_residual.py: relation slots with the meta-only and the full last hop,
  and the edge pass), 1e-5 x max(1, max|ref|);
* against the mag.REGNN autograd path on one sampled batch over the step's modes (relation
  slots, the sampler's layer-0 sums, strided blocks, dropout);
* bitwise reproducibility of the step;
* NSTrainer: the pipelined, captured trainer with the fused Adam against eager unpipelined
  steps, and the fall-back to the module path where the two-layer form does not apply.

Self-contained: the small helpers are copies of those in test_gpu_regnn_golden.py /
test_gpu_ns_engine.py."""
import functools

import numpy as np
import pytest
import torch

import _golden as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5


def _check(tag, got, want, tol=TOL):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    ok, err = G.close(got, want, tol)
    print(f"{tag}: rel err {err:.3e}")
    assert ok, f"{tag}: rel err {err:.3e}"


# ---------------------------------------------------------------------------------------------
# 1. the reference's REGNN with residual
# ---------------------------------------------------------------------------------------------
def _golden_model(d):
    from regnn_hip import mag
    m = d["meta"]
    counts, K = m["counts"], m["in_channels"]
    model = mag.REGNN(K, m["hidden"], m["classes"], m["num_layers"], m["scaling_factor"], 0.0,
                      {t: K for t in range(4)}, m["num_edge_types"], residual=m["residual"],
                      use_norm="ln", self_loop_type=2, feats_type=m["feats_type"],
                      num_nodes_dict={t: counts[t] for t in range(4)}, target_node_type=0)
    P = G.sub(d, "p_", np.float32)
    assert {n for n, _ in model.named_parameters()} == set(P)
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(torch.from_numpy(P[n]))
    return model.to(DEV)


@pytest.mark.parametrize("name,lean", [("nsres_regnn_schema", "on"), ("nsres_regnn_schema", "off"),
                                       ("nsres_regnn_ft3", "off")])
def test_residual_fused_step_vs_reference(monkeypatch, name, lean):
    """regnn_ns_hop reproduces the fixture's sampled batch; regnn_nsm_step's loss and every
    gradient match the reference REGNN's with residual=True. nsres_regnn_schema: relation slots,
    a hub row of the transposed index among the batch targets, rows with 1 and 26 entries;
    nsres_regnn_ft3: the edge pass. (Before the residual mode existed FusedStep raised
    ValueError here.)"""
    from regnn_hip import ns
    from regnn_hip.graph import RelGraph
    from regnn_hip.ns import DeviceSampler, FusedStep
    monkeypatch.setitem(ns.LEAN_LAST_HOP, "mode", lean)
    d = G.load(name)
    m = d["meta"]
    assert m["residual"] is True
    N = int(sum(m["counts"]))
    rg = RelGraph(torch.from_numpy(d["src"]), torch.from_numpy(d["dst"]), N, DEV)
    ds = DeviceSampler(rg, m["sizes"], len(d["batch"]), etype=torch.from_numpy(d["edge_type"]),
                       ntype=torch.from_numpy(d["ntype"]), num_edge_types=m["num_edge_types"])
    model = _golden_model(d)
    model.eval()
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    x_dict = {t: torch.from_numpy(d[f"x{t}"]).to(DEV) for t in range(4)}
    nt, loc = torch.from_numpy(d["ntype"]).to(DEV), torch.from_numpy(d["local"]).to(DEV)
    if m.get("y_global"):
        y_flat = torch.from_numpy(d["y"])
    else:
        y_flat = torch.full((N,), -1, dtype=torch.int64)
        y_flat[:m["counts"][0]] = torch.from_numpy(d["y"])
    loss = torch.zeros((), device=DEV)
    fs = FusedStep(model, ds, x_dict, nt, loc, y_flat, loss)
    assert fs.two_layer and fs.P.two_layer == 1
    assert fs.P.residual == 1
    assert fs.P.rel_slots == (1 if m.get("schema") == "ogbn-mag" else 0)
    L_ = len(m["sizes"])
    assert ds.meta_only[L_ - 1] == (lean == "on")
    ds.set_seed(m["seed"], m["epoch"], m["batch_idx"])
    ds.set_targets(torch.from_numpy(d["batch"]).to(DEV))
    ds.run_hops()
    for h in range(L_):                  # hop h's block = the fixture's adjs, outermost first
        n_src, n_dst = (int(v) for v in d[f"adj{L_ - 1 - h}_size"])
        assert int(ds.sizes[h]) == n_dst
        assert int(ds.sizes[8 + h]) == d[f"adj{L_ - 1 - h}_src"].size + n_dst   # + self loops
    n_chk = int(ds.sizes[L_ if lean == "off" else L_ - 1])
    assert ds.n_id[:n_chk].cpu().numpy().tolist() == d["n_id"][:n_chk].tolist()
    fs.step()
    torch.cuda.synchronize()
    _check("loss", loss, d["loss"])
    got = {n: p.grad for n, p in model.named_parameters()}
    for k, v in G.sub(d, "grad_").items():
        _check(k, got[k], v)


# ---------------------------------------------------------------------------------------------
# 2.-5. a synthetic ogbn-mag-like graph
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mag_graph(scale, seed, F):
    from regnn_hip import synth
    from regnn_hip.graph import RelGraph
    gd = synth.mag_like(scale, seed=seed, device=DEV)
    keep = gd["rel"] <= 7
    rg = RelGraph(gd["src"][keep], gd["dst"][keep], gd["N"], DEV)
    edge_type = gd["rel"][keep].to(torch.int64) - 1
    node_type = gd["ntype"]
    offs = torch.tensor([gd["type_offsets"][t] for t in synth.NTYPES], device=DEV)
    local = torch.arange(gd["N"], device=DEV) - offs[node_type]
    feats = synth.type_features(gd["counts"], {t: F for t in synth.NTYPES}, seed=1, device=DEV)
    return dict(gd=gd, rg=rg, edge_type=edge_type, node_type=node_type, local=local,
                x_dict={k: f for k, f in enumerate(feats)}, n_paper=gd["counts"]["paper"])


def _mag(scale, seed=0, F=128, hidden=64, classes=37, dropout=0.0, layers=2, residual=True):
    from regnn_hip import mag
    d = dict(_mag_graph(scale, seed, F))
    n_paper, N = d["n_paper"], d["gd"]["N"]
    y = torch.full((N, 1), -1, dtype=torch.int64, device=DEV)
    y[:n_paper, 0] = (torch.arange(n_paper, device=DEV) * 7) % classes
    x_dict = d["x_dict"]

    def model(seed=0):
        torch.manual_seed(seed)
        m = mag.REGNN(F, hidden, classes, layers, 10.0, dropout, {k: F for k in x_dict}, 7,
                      residual=residual, use_norm="ln", self_loop_type=2).to(DEV)
        with torch.no_grad():
            for conv in m.convs:
                conv.relation_weight.copy_(torch.linspace(0.02, 0.12, 11, device=DEV))
                conv.bias.normal_(0, 0.1)
        return m

    d.update(y=y, model=model)
    return d


def _trainer(d, model, batch=96, sizes=(7, 5), seed=3, lr=1e-2, opt="torch", **kw):
    from regnn_hip.ns import NSTrainer
    o = torch.optim.Adam(model.parameters(), lr=lr, capturable=True) if opt == "torch" else None
    return NSTrainer(model, o, d["rg"], list(sizes), batch,
                     torch.arange(d["n_paper"], device=DEV), d["x_dict"], d["edge_type"],
                     d["node_type"], d["local"], d["y"], 7, seed=seed, **kw)


def _nsm_seed(st, layer):
    """the fused step's dropout seed of `layer` (include/regnn_hip.h, regnn_nsm_step)."""
    from regnn_hip.sampler import _mix
    M = (1 << 64) - 1
    return _mix((st[0] & M) ^ _mix(((st[1] << 40) ^ (st[3] << 8) ^ (layer + 0x51ED27)) & M))


# PRE_SUMS "on" takes effect only with relation slots over strided blocks (FusedStep leaves
# pre_sums 0 otherwise and runs what "off" runs): those combinations are left out
MODES = [(rs, pre, st, 128) for rs in ("auto", "off") for st in ("on", "off")
         for pre in ("on", "off") if pre == "off" or (rs == "auto" and st == "on")]
# 64-wide inputs with relation slots: layer 0's general kernel (the 128-wide rows have their own;
# the 64-wide edge pass is nsres_regnn_ft3's)
MODES.append(("auto", "off", "on", 64))


@pytest.mark.parametrize("dropout", [0.0, 0.5])
@pytest.mark.parametrize("rel_slots,pre_sums,strided,width", MODES)
def test_residual_fused_step_matches_module_path(monkeypatch, rel_slots, pre_sums, strided, width,
                                                 dropout):
    """regnn_nsm_step with residual against the mag.REGNN autograd path (agg + x_target before
    the conv's GEMM) on the same sampled batch: loss and every parameter gradient at 1e-5. With
    dropout the module path gets the fused step's hash masks in place of torch's RNG."""
    from oracle import regnn_oracle as O
    from regnn_hip import ns
    monkeypatch.setitem(ns.REL_SLOTS, "mode", rel_slots)
    monkeypatch.setitem(ns.PRE_SUMS, "mode", pre_sums)
    monkeypatch.setitem(ns.STRIDED, "mode", strided)
    d = _mag(0.003, seed=6, F=width, dropout=dropout)
    m_mod, m_fus = d["model"](1), d["model"](1)
    m_mod.train(); m_fus.train()
    tr_m = _trainer(d, m_mod, engine="module")
    assert tr_m.fused is None
    tr_f = _trainer(d, m_fus)
    assert tr_f.fused is not None and tr_f.fused.two_layer
    for fs in tr_f.fused_slots:
        assert fs.P.residual == 1
        assert fs.P.rel_slots == (1 if rel_slots == "auto" else 0)
        assert fs.W.pre_sums == (1 if pre_sums == "on" else 0)
        assert bool(fs.W.stride[0]) == (strided == "on")
    tr_f._forward_backward()
    torch.cuda.synchronize()
    st = tr_f.sampler.state.cpu().tolist()
    calls = []
    if dropout > 0:
        keep16 = int(round((1 - dropout) * 65536))

        def hash_dropout(x, p=0.5, training=True, inplace=False):
            layer = len(calls)
            calls.append(layer)
            mask = O.dropout_mask(_nsm_seed(st, layer), x.shape[0], x.shape[1], 4, keep16)
            return x * torch.from_numpy(mask).to(x.device, x.dtype) / (keep16 / 65536)
        monkeypatch.setattr(torch.nn.functional, "dropout", hash_dropout)
    tr_m._forward_backward()
    torch.cuda.synchronize()
    if dropout > 0:
        assert calls == [0, 1]
    n0 = int(tr_f.sampler.sizes[1])
    assert torch.equal(tr_m.sampler.sizes[8:10], tr_f.sampler.sizes[8:10])
    assert torch.equal(tr_m.sampler.n_id[:n0], tr_f.sampler.n_id[:n0])
    lm, lf = float(tr_m.loss), float(tr_f.loss)
    print(f"loss module {lm:.7f} fused {lf:.7f}")
    assert abs(lm - lf) <= 1e-5 * max(1.0, abs(lm)), (lm, lf)
    gm = dict(m_mod.named_parameters())
    for n, p in m_fus.named_parameters():
        _check(n, p.grad, gm[n].grad.cpu().numpy().astype(np.float64))


@pytest.mark.parametrize("rel_slots", ["auto", "off"])
def test_residual_step_bitwise_reproducible(monkeypatch, rel_slots):
    """the residual step run twice on the same batch (dropout on): loss and every gradient
    bitwise equal (the residual terms ride in the step's exact / fixed-order sums)."""
    from regnn_hip import ns
    monkeypatch.setitem(ns.REL_SLOTS, "mode", rel_slots)
    d = _mag(0.003, seed=6, dropout=0.5)
    m = d["model"](1)
    m.train()
    tr = _trainer(d, m, pipeline=False)
    fs = tr.fused
    assert fs is not None and fs.P.residual == 1 and not tr.adam_fused
    assert fs.P.rel_slots == (1 if rel_slots == "auto" else 0)
    tr._forward_backward()
    torch.cuda.synchronize()
    g1, l1 = tr.flat.clone(), tr.loss.clone()
    assert np.isfinite(float(l1)) and float(g1.abs().max()) > 0
    tr.flat.zero_()
    fs.step()
    torch.cuda.synchronize()
    assert torch.equal(tr.loss, l1)
    assert torch.equal(tr.flat, g1)


def test_residual_trainer_pipelined_captured_matches_eager():
    """engine="auto" takes the fused step for a residual model (FlatAdam inside its last launch);
    4 steps pipelined and captured (lookahead groups) train the same batches to the same
    parameters as 4 eager unpipelined steps."""
    d = _mag(0.002, seed=8, classes=13, dropout=0.4)

    def make(pipe):
        return _trainer(d, d["model"](5), batch=100, sizes=(6, 4), seed=9, opt=None,
                        adam=dict(lr=1e-2), engine="auto", pipeline=pipe)
    tr_p, tr_u = make(True), make(False)
    assert tr_p.fused is not None and tr_u.fused is not None
    assert tr_p.pipelined and not tr_u.pipelined
    assert tr_p.adam_fused and tr_u.adam_fused
    assert all(fs.P.residual == 1 and fs.two_layer for fs in tr_p.fused_slots)
    tr_p.capture(warmup=2)                              # warm-up steps undone by capture()
    tr_p.run_steps(4)
    for _ in range(4):
        tr_u.step()
    torch.cuda.synchronize()
    assert torch.equal(tr_p.sampler.n_id[:int(tr_p.sampler.sizes[0])],
                       tr_u.sampler.n_id[:int(tr_u.sampler.sizes[0])])
    lp, lu = float(tr_p.loss), float(tr_u.loss)
    assert np.isfinite(lp) and np.allclose(lp, lu, rtol=1e-6, atol=1e-7), (lp, lu)
    pp, pu = tr_p.param_vector().cpu().numpy(), tr_u.param_vector().cpu().numpy()
    assert np.all(np.isfinite(pp))
    assert np.allclose(pp, pu, rtol=1e-6, atol=1e-7), float(np.abs(pp - pu).max())


def test_residual_falls_back_outside_two_layer_form():
    """a hop-0 block past the transposed index (1300 x 26 = 33,800 > 32,768 entries) or a third
    layer: the composed-map form has no residual, so engine="auto" trains on the module path
    (every slot) and engine="fused" / FusedStep raise ValueError before any launch."""
    from regnn_hip.ns import DeviceSampler, FusedStep
    d = _mag(0.003, seed=6)
    tr = _trainer(d, d["model"](1), batch=1300, sizes=(25, 20), engine="auto")
    assert tr.fused is None and not hasattr(tr, "fused_slots")
    tr.step()
    torch.cuda.synchronize()
    assert np.isfinite(float(tr.loss))
    with pytest.raises(ValueError, match="two-layer"):
        _trainer(d, d["model"](1), batch=1300, sizes=(25, 20), engine="fused")
    ds = DeviceSampler(d["rg"], [25, 20], 1300, etype=d["edge_type"], ntype=d["node_type"],
                       num_edge_types=7)
    m = d["model"](1)
    for p in m.parameters():
        p.grad = torch.zeros_like(p)
    with pytest.raises(ValueError, match="two-layer"):
        FusedStep(m, ds, d["x_dict"], d["node_type"], d["local"], d["y"].reshape(-1),
                  torch.zeros((), device=DEV))
    assert ds.edge_meta[1] is None                      # refused before the sampler was touched
    d3 = _mag(0.003, seed=6, layers=3)
    tr3 = _trainer(d3, d3["model"](1), batch=64, sizes=(5, 4, 3), engine="auto")
    assert tr3.fused is None
    tr3.step()
    torch.cuda.synchronize()
    assert np.isfinite(float(tr3.loss))
    with pytest.raises(ValueError, match="two-layer"):
        _trainer(d3, d3["model"](1), batch=64, sizes=(5, 4, 3), engine="fused")
