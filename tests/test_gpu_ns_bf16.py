"""bf16 input feature tables in the NS sampler's sums launch (regnn_ns_hop_typed_sums_dt). bf16 ->
fp32 is a 16-bit shift, so a bf16 table must give bit for bit what the fp32 kernels give on
x.bfloat16().float():

* the sums launch alone on the hand-built typed graph (32 / 64 lanes per row, one and two rounds,
  with and without the type layout), every output bitwise;
* the fused two-layer step: loss and the gradient bucket bitwise;
* FusedStep against the fp64 oracle evaluated on the rounded inputs;
* the module engine (hidden 128) through the sampler's input sums;
* the captured, pipelined trainer against eager steps;
* the refusals, and ShardedInference's chunked widening.

Self-contained: the helpers import from the test files whose recipes they follow."""
import numpy as np
import pytest
import torch

import _golden as G
from test_ns_type_layout import SEED, hand_graph

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5
NAMES = ("s_agg", "s_w", "u_self", "u_rel", "scnt", "inv")


def _widen(x_dict):
    return {k: v.float() for k, v in x_dict.items()}


def _bf16(x_dict):
    return {k: v.bfloat16().contiguous() for k, v in x_dict.items()}


def _check(tag, got, want, tol=TOL):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    ok, err = G.close(got, want, tol)
    print(f"{tag}: rel err {err:.3e}")
    assert ok, f"{tag}: rel err {err:.3e}"


# ---------------------------------------------------------------------------------------------
# 1. the sums launch, bitwise
# ---------------------------------------------------------------------------------------------
def _special(tab):
    """a few elements of a bf16 table overwritten in place with -0.0, bf16 subnormals and +-2^60:
    a widening that is not the pure shift (a conversion that flushes or rounds) would show."""
    bits = tab.view(torch.int16)
    pats = [-0x8000, 0x0001, 0x007F, -0x8000 + 0x0001, -0x8000 + 0x007F, 0x5D80, -0x8000 + 0x5D80]
    n, K = tab.shape
    for i, p in enumerate(pats):
        for r in {0, n // 2, n - 1}:
            bits[r, (5 * i + 3 * r) % K] = p
            bits[r, (4 * i + 64) % K] = p
    return tab


@pytest.mark.parametrize("layout", [True, False])
@pytest.mark.parametrize("sizes", [(3, 3), (3, 20), (3, 33)])
def test_sums_launch_bitwise(sizes, layout):
    """(3, 3): 32 lanes per row, one round; (3, 20): 32 lanes, 21 entries (two rounds); (3, 33):
    64 lanes and the Floyd path (node 0 has 40 in-edges, node 36 exactly 33). layout False: the
    permuted graph, whose launch reads the lookup tables (the other DERIVE instantiation)."""
    import test_gpu_ns_type_layout as TL
    g = hand_graph() if layout else TL._permuted(hand_graph())
    c = TL._case(g)
    xb = {t: _special(v.bfloat16().contiguous()) for t, v in c["x"].items()}
    res = {}
    for mode, x in (("bf16", xb), ("fp32", _widen(xb))):
        tr, _ = TL._trainer(dict(c, x=x), sizes)
        s = tr.sampler
        ts = s.typed_sums[1]
        assert (ts["layout"] is not None) == layout
        assert ts["dtype"] == (1 if mode == "bf16" else 0)
        s.set_seed(SEED, 0, 0)
        s.set_targets(torch.arange(g["N"], device=DEV))
        s.run_hops()
        torch.cuda.synchronize()
        assert s.sums_fresh[1]
        bufs, n1 = TL._sums(tr)
        res[mode] = (bufs, s.n_id[:n1].clone(), n1)
    (a, ida, n1), (b, idb, _) = res["bf16"], res["fp32"]
    assert n1 >= g["N"] and torch.equal(ida, idb)
    for name, p, q in zip(NAMES, a, b):
        assert torch.equal(p, q), name
    assert bool(a[0].any()) and int(a[4].max()) == min(sizes[1], 40)
    # the self rows are the table rows shifted up 16 bits, nothing else
    nt, loc = c["ntype"][ida.long()], c["local"][ida.long()]
    want = torch.empty(n1, 128, dtype=torch.int32, device=a[2].device)
    for t, tab in xb.items():
        m = nt == t
        want[m] = tab.view(torch.int16)[loc[m].long()].int() << 16
    assert torch.equal(a[2].view(torch.int32), want)


# ---------------------------------------------------------------------------------------------
# 2. the fused step, bitwise
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("dropout", [0.0, 0.5])
def test_fused_step_bitwise(dropout, residual):
    from test_gpu_ns_residual import _mag, _trainer
    d = _mag(0.003, seed=6, dropout=dropout, residual=residual)
    xb = _bf16(d["x_dict"])
    res = {}
    for mode, x in (("bf16", xb), ("fp32", _widen(xb))):
        m = d["model"](1)
        m.train()
        tr = _trainer(dict(d, x_dict=x), m, pipeline=False)
        fs = tr.fused
        assert fs is not None and fs.two_layer and fs.W.pre_sums == 1
        assert fs.P.residual == int(residual)
        tr._forward_backward()
        torch.cuda.synchronize()
        res[mode] = (tr.loss.clone(), tr.flat.clone())
    (la, ga), (lb, gb) = res["bf16"], res["fp32"]
    assert torch.isfinite(la) and float(ga.abs().max()) > 0
    assert torch.equal(la, lb)
    assert torch.equal(ga, gb)


# ---------------------------------------------------------------------------------------------
# 3. against the reference (the fp64 oracle pinned to it), on rounded inputs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mag_regnn_schema", "nsres_regnn_schema"])
def test_fused_step_vs_oracle_on_rounded_inputs(name):
    """FusedStep over DeviceSampler on the fixture's batch with x_dict in bf16: loss and every
    gradient against oracle.regnn_oracle.mag_regnn_model on x.bfloat16().double() at 1e-5. (Not
    against the fixtures' stored fp32 gradients: rounding the inputs moves nsres_regnn_schema's
    convs.1.weight gradient by 0.18 of its largest element.)"""
    from oracle import regnn_oracle as O
    from regnn_hip import mag
    from regnn_hip.graph import RelGraph
    from regnn_hip.ns import DeviceSampler, FusedStep
    d = G.load(name)
    m = d["meta"]
    residual = bool(m.get("residual", False))
    N = int(sum(m["counts"]))
    rg = RelGraph(torch.from_numpy(d["src"]), torch.from_numpy(d["dst"]), N, DEV)
    ds = DeviceSampler(rg, m["sizes"], len(d["batch"]), etype=torch.from_numpy(d["edge_type"]),
                       ntype=torch.from_numpy(d["ntype"]), num_edge_types=m["num_edge_types"])
    counts, K = m["counts"], m["in_channels"]
    model = mag.REGNN(K, m["hidden"], m["classes"], m["num_layers"], m["scaling_factor"], 0.0,
                      {t: K for t in range(4)}, m["num_edge_types"], residual=residual,
                      use_norm="ln", self_loop_type=2, feats_type=m["feats_type"],
                      num_nodes_dict={t: counts[t] for t in range(4)}, target_node_type=0)
    P32 = G.sub(d, "p_", np.float32)
    assert {n for n, _ in model.named_parameters()} == set(P32)
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(torch.from_numpy(P32[n]))
    model = model.to(DEV).eval()
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    xb = {t: torch.from_numpy(d[f"x{t}"]).bfloat16().to(DEV) for t in range(4)}
    nt, loc = torch.from_numpy(d["ntype"]).to(DEV), torch.from_numpy(d["local"]).to(DEV)
    assert m.get("y_global")
    loss = torch.zeros((), device=DEV)
    fs = FusedStep(model, ds, xb, nt, loc, torch.from_numpy(d["y"]), loss)
    assert fs.two_layer and fs.P.rel_slots == 1 and fs.W.pre_sums == 1
    assert fs.P.residual == int(residual)
    ds.set_seed(m["seed"], m["epoch"], m["batch_idx"])
    ds.set_targets(torch.from_numpy(d["batch"]).to(DEV))
    ds.run_hops()
    L_ = len(m["sizes"])
    for h in range(L_):                  # the fixture's batch (adjs outermost first)
        assert int(ds.sizes[h]) == int(d[f"adj{L_ - 1 - h}_size"][1])
    fs.step()
    torch.cuda.synchronize()
    adjs = [(d[f"adj{h}_src"], d[f"adj{h}_dst"], d[f"adj{h}_eid"],
             tuple(int(v) for v in d[f"adj{h}_size"])) for h in range(L_)]
    x64 = {t: v.double().cpu().numpy() for t, v in xb.items()}
    _, ref_loss, ref = O.mag_regnn_model(x64, d["ntype"], d["local"], d["n_id"], adjs,
                                         d["edge_type"], G.sub(d, "p_"), d["y"][d["batch"]],
                                         feats_type=m["feats_type"], residual=residual)
    _check("loss", loss, np.asarray(ref_loss))
    got = {n: p.grad for n, p in model.named_parameters()}
    assert set(ref) == set(G.sub(d, "grad_")) and set(ref) <= set(got)
    for k, v in ref.items():
        _check(k, got[k], v)


# ---------------------------------------------------------------------------------------------
# 4. the module engine
# ---------------------------------------------------------------------------------------------
def test_module_engine_reads_the_sums():
    from test_gpu_ns_residual import _mag, _trainer
    d = _mag(0.003, seed=6, hidden=128, residual=False)
    xb = _bf16(d["x_dict"])
    res = {}
    for mode, x in (("bf16", xb), ("fp32", _widen(xb))):
        m = d["model"](1)
        m.train()
        tr = _trainer(dict(d, x_dict=x), m, engine="module", pipeline=False)
        assert tr.fused is None
        tr._forward_backward()
        torch.cuda.synchronize()
        s = tr.sampler
        pre = s.blocks[-1].pre_sums
        assert pre is not None and s.typed_sums[-1]["dtype"] == (1 if mode == "bf16" else 0)
        n1 = int(s.sizes[1])
        res[mode] = (float(tr.loss), {n: p.grad.clone() for n, p in m.named_parameters()},
                     [t[:n1].clone() for t in pre])
    (la, ga, pa), (lb, gb, pb) = res["bf16"], res["fp32"]
    for name, p, q in zip(("U", "cnt", "x_self", "u_rel"), pa, pb):
        assert torch.equal(p, q), name
    assert bool(pa[0].any())
    # (zero in exact arithmetic: the bound absorbs a GEMM algorithm choice that may differ per run)
    assert np.isfinite(la) and abs(la - lb) <= TOL * max(1.0, abs(lb)), (la, lb)
    for n, g in ga.items():
        _check(n, g, gb[n].double().cpu().numpy())


# ---------------------------------------------------------------------------------------------
# 5. captured and pipelined
# ---------------------------------------------------------------------------------------------
def test_trainer_pipelined_captured_matches_eager():
    """4 steps pipelined and captured on bf16 tables train to the parameters of 4 eager
    unpipelined steps, bitwise (test_residual_trainer_pipelined_captured_matches_eager's recipe)."""
    from test_gpu_ns_residual import _mag, _trainer
    d = _mag(0.002, seed=8, classes=13, dropout=0.4)
    d = dict(d, x_dict=_bf16(d["x_dict"]))

    def make(pipe):
        return _trainer(d, d["model"](5), batch=100, sizes=(6, 4), seed=9, opt=None,
                        adam=dict(lr=1e-2), engine="auto", pipeline=pipe)
    tr_p, tr_u = make(True), make(False)
    assert tr_p.fused is not None and tr_u.fused is not None
    assert tr_p.pipelined and not tr_u.pipelined
    assert tr_p.adam_fused and tr_u.adam_fused
    assert all(fs.W.pre_sums == 1 for fs in tr_p.fused_slots)
    assert all(s.typed_sums[1]["dtype"] == 1 for s in tr_p.slots)
    tr_p.capture(warmup=2)                              # warm-up steps undone by capture()
    tr_p.run_steps(4)
    for _ in range(4):
        tr_u.step()
    torch.cuda.synchronize()
    assert torch.equal(tr_p.sampler.n_id[:int(tr_p.sampler.sizes[0])],
                       tr_u.sampler.n_id[:int(tr_u.sampler.sizes[0])])
    lp, lu = float(tr_p.loss), float(tr_u.loss)
    assert np.isfinite(lp) and np.allclose(lp, lu, rtol=1e-6, atol=1e-7), (lp, lu)
    pp, pu = tr_p.param_vector(), tr_u.param_vector()
    assert bool(torch.isfinite(pp).all())
    assert torch.equal(pp, pu)


# ---------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------
def test_refusals_name_the_cause(monkeypatch):
    from regnn_hip import mag, ns
    from regnn_hip.ns import DeviceSampler, FusedStep
    from test_gpu_ns_residual import _mag, _trainer
    d = _mag(0.003, seed=6, residual=False)
    xb = _bf16(d["x_dict"])
    # FusedStep without the sampler's input sums: agg0 would read the bf16 rows as fp32
    monkeypatch.setitem(ns.PRE_SUMS, "mode", "off")
    ds = DeviceSampler(d["rg"], [7, 5], 96, etype=d["edge_type"], ntype=d["node_type"],
                       num_edge_types=7)
    m = d["model"](1)
    for p in m.parameters():
        p.grad = torch.zeros_like(p)
    with pytest.raises(ValueError, match="PRE_SUMS"):
        FusedStep(m, ds, xb, d["node_type"], d["local"], d["y"].reshape(-1),
                  torch.zeros((), device=DEV))
    assert ds.edge_meta[1] is None                      # refused before the sampler was touched
    monkeypatch.setitem(ns.PRE_SUMS, "mode", "on")
    # the module path at K = 64: no sums launch for that width
    d64 = _mag(0.003, seed=6, F=64, hidden=128, residual=False)
    with pytest.raises(ValueError, match="128"):
        _trainer(dict(d64, x_dict=_bf16(d64["x_dict"])), d64["model"](1), engine="module")
    # tables that learn stay fp32
    n_paper = d["n_paper"]
    counts = {k: int(v.shape[0]) for k, v in d["x_dict"].items()}
    m2 = mag.REGNN(128, 64, 37, 2, 10.0, 0.0, {k: 128 for k in range(4)}, 7, use_norm="ln",
                   self_loop_type=2, feats_type=2, num_nodes_dict=counts,
                   target_node_type=0).to(DEV)
    with pytest.raises(ValueError, match="feats_type"):
        ns.NSTrainer(m2, None, d["rg"], [7, 5], 96, torch.arange(n_paper, device=DEV),
                     {0: xb[0]}, d["edge_type"], d["node_type"], d["local"], d["y"], 7)


# ---------------------------------------------------------------------------------------------
# 7. inference
# ---------------------------------------------------------------------------------------------
def test_sharded_inference_widens_in_chunks(monkeypatch):
    from regnn_hip import inference
    from test_gpu_ns import _setup
    gd, rg, edge_type, node_type, local, x_dict, model = _setup(scale=0.002, seed=2)
    model.eval()
    xb = _bf16(x_dict)
    inf = inference.ShardedInference(model, rg, edge_type, node_type, local)
    want = inf.run(_widen(xb), gather=None)
    rows = min(int(v.shape[0]) for v in xb.values())
    chunk = max(1, (rows + 2) // 3 + (1 if rows % 3 == 0 else 0))
    monkeypatch.setattr(inference, "BF16_CHUNK_ROWS", chunk)
    # the smallest type spans three chunks, the last one partial
    assert 2 * chunk < rows < 3 * chunk
    got = inf.run(xb, gather=None)
    torch.cuda.synchronize()
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    _check("logits", got, want.double().cpu().numpy())
