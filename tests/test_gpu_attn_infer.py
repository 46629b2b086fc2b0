"""GPU checks of the forward-only fused attention (regnn_mag_attn_fwd + regnn_mag_attn_epilogue,
ops.mag_attn_*) and of the full-neighbour inference of the mag 'regat' / 'regatv2' models on it:

1. operator, per element against fp64 under _attention_ref.rel_err with the `out` scale
   sum_e a_e |x_u| <= TOL_F32: the ladder graph (N = 320, in-degrees 0 .. 300) in the three
   PLAN_FORMS, the recipes unit / wide / deep, six (H, D) and the kinds GAT-el, GAT-attn_l and
   GATv2 (message rows = score rows); rows of in-degree 0 exactly 0;
2. the fused form against the chain of existing operators on `unit`, 2e-5 under that metric;
3. two calls return equal bits (also in the `tree` form);
4. the inference-path layer over the mag_regat*conv fixtures' edges (bias, residual, LayerNorm)
   against the reference-generated outputs, _golden.close at 1e-5;
5. model.inference for 'regat' / 'regatv2' on mag_like(0.002) against the fp64 restatement and
   against the model's own eval forward on full-neighbour batches (NeighborSampler [-1, -1]);
6. three ranks in lockstep with gmax = the maximum of the three against one rank, and
   gather='argmax' against the logits' argmax.

Measured maxima of 1. on an MI355X over the 162 cases (unit / wide / deep): GAT-el 4.1e-7 /
9.3e-7 / 6.7e-7, GAT-attn_l 6.8e-7 / 2.2e-6 / 2.2e-6, GATv2 3.5e-7 / 1.7e-6 / 1.2e-6.
"""
import types

import numpy as np
import pytest
import torch

import _attention_ref as R
import _attn_infer_ref as A
import _golden as G
import _ns_gat_blocks as B

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURES = ["mag_regatconv_h4_res0", "mag_regatconv_h2_res1", "mag_regatv2conv_h4_res0",
            "mag_regatv2conv_h2_res1"]

_GRAPHS, _REFS = {}, {}


def _graph(form):
    """the ladder graph in one plan form, once: (row-block view on the device, CPU CSR, rg, pack)"""
    if form not in _GRAPHS:
        rg, e_feat = R.ladder_graph(form, DEV)
        pack = rg.rel_pack(e_feat)
        blk = types.SimpleNamespace(csr_ptr=rg.csr_ptr, csr_idx=rg.csr_idx, csr_plan=rg.csr_plan,
                                    n_dst=rg.n_dst, n_src=rg.n_src, E=rg.E, pack=pack)
        csr = (rg.csr_ptr.cpu(), rg.csr_idx.cpu().long(), pack.rel_csr.cpu().long())
        _GRAPHS[form] = (blk, csr, rg, pack)
    return _GRAPHS[form]


def _reference(kind, recipe, H, D):
    """inputs, fp64 reference and scale of a case, once for the three plan forms (whose CSRs
    hold the same rows in the same order)"""
    key = (kind, recipe, H, D)
    if key not in _REFS:
        c = A.operator_inputs(kind, recipe, 320, H, D, R.N_REL, seed=300 + 7 * H + D)
        want, scale, _ = A.operator_reference(kind, c, *_graph("noplan")[1])
        _REFS[key] = (c, want, scale)
    return _REFS[key]


def _fused(blk, kind, c):
    """the operator: regnn_mag_attn_fwd, gmax on the device, regnn_mag_attn_epilogue (no tail)"""
    from regnn_hip import ops
    d = {k: v.to(DEV) for k, v in c.items() if torch.is_tensor(v)}
    if kind == "gat_el":
        kw = dict(el=d["el"], er=d["er"])
    elif kind == "gat_attn":
        kw = dict(att=d["al"], er=d["er"])
    else:
        kw = dict(att=d["att"], xd=d["xd"])
    acc, rmax, rsum = ops.mag_attn_fwd(blk, d["x"], "gatv2" if kind == "gatv2" else "gat",
                                       d["tab"], c["slope"], **kw)
    gmax = rmax.amax().reshape(1)
    y = ops.mag_attn_epilogue(acc, rmax, rsum, gmax)
    return y.view(acc.shape), (acc, rmax, rsum)


@pytest.mark.parametrize("form", list(R.PLAN_FORMS))
@pytest.mark.parametrize("recipe", A.RECIPES)
@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("H,D", A.SHAPES)
def test_operator_matches_fp64_per_element(kind, recipe, H, D, form):
    blk, csr, _rg, _pack = _graph(form)
    for a, b in zip(csr, _graph("noplan")[1]):
        assert torch.equal(a, b)                       # one reference serves the three forms
    c, want, scale = _reference(kind, recipe, H, D)
    out, (acc, rmax, rsum) = _fused(blk, kind, c)
    err = R.rel_err(out.cpu(), want, scale)
    print(f"mag_attn {kind} {recipe} H={H} D={D} {form}: {err:.2e}")
    empty = (csr[0][1:] == csr[0][:-1]).to(DEV)
    assert int(empty.sum()) > 0
    assert not out[empty].any() and not acc[empty].any() and not rsum[empty].any()
    assert bool((rmax[empty] == -torch.inf).all())
    assert err <= R.TOL_F32, f"{err:.3e}"


@pytest.mark.parametrize("form", ["default", "tree"])
@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("H,D", [s for s in A.SHAPES if s[0] & (s[0] - 1) == 0])
def test_fused_agrees_with_the_chain_of_existing_operators(kind, H, D, form):
    """(the chain's edge softmax takes H a power of two only: 3 heads run on the fused form alone)"""
    from regnn_hip import ops
    blk, _csr, rg, pack = _graph(form)
    c, want, scale = _reference(kind, "unit", H, D)
    d = {k: v.to(DEV) for k, v in c.items() if torch.is_tensor(v)}
    out, _ = _fused(blk, kind, c)
    with torch.no_grad():
        if kind == "gatv2":
            s = ops.gatv2_scores(rg, d["x"], d["xd"], d["att"], c["slope"])
            a = ops.edge_softmax_logits(rg, s, d["tab"], pack, global_max=True)
        else:
            el = d["el"] if kind == "gat_el" else (d["x"] * d["al"]).sum(-1)
            a = ops.gat_attention(rg, el, d["er"], d["tab"], pack, c["slope"], global_max=True)
        chain = ops.head_spmm(rg, a, d["x"])
    err = float(((out - chain).abs().double().cpu() / (scale + R.FLOOR)).max())
    print(f"mag_attn {kind} H={H} D={D} {form}: fused against chain {err:.2e}")
    assert err <= 2e-5
    # ops' own chain form (the fallback for shapes the kernel refuses) is that chain (GATv2 here:
    # the GAT kinds' inputs carry er, not att_dst; test_inference_layer_matches_fixture has both)
    if kind == "gatv2":
        y = ops.mag_attn_infer(blk, d["x"], d["xd"], "gatv2", d["tab"], c["slope"], att=d["att"],
                               form="chain")
        assert float(((y.view_as(chain) - chain).abs().double().cpu() / (scale + R.FLOOR)).max()) \
            <= 2e-5


@pytest.mark.parametrize("form", ["default", "tree"])
@pytest.mark.parametrize("kind", A.KINDS)
def test_two_calls_return_equal_bits(kind, form):
    blk = _graph(form)[0]
    c, _want, _scale = _reference(kind, "wide", 8, 64)
    o1, t1 = _fused(blk, kind, c)
    o2, t2 = _fused(blk, kind, c)
    assert torch.equal(o1, o2)
    for a, b in zip(t1, t2):
        assert torch.equal(a, b)


def test_epilogue_zero_terms_and_tail():
    """rsum = 0 and a gmax - rmax beyond the exponential's range give a zero attention term (no
    NaN); bias, residual, LayerNorm and relu against torch"""
    from regnn_hip import ops
    g = torch.Generator().manual_seed(0)
    n, H, D = 37, 3, 8
    acc = torch.randn(n, H, D, generator=g)
    rmax = torch.randn(n, H, generator=g)
    rsum = torch.rand(n, H, generator=g) + 1.0
    rsum[0], rmax[0], acc[0] = 0.0, -torch.inf, 0.0
    rmax[1] = -1e4                                     # exp(gmax - rmax) overflows fp64 too
    bias, res = torch.randn(H * D, generator=g), torch.randn(n, H * D, generator=g)
    lw, lb = torch.randn(H * D, generator=g), torch.randn(H * D, generator=g)
    gmax = torch.tensor([40.0])
    den = rsum.double() + 1e-16 * torch.exp(gmax.double() - rmax.double())
    att = acc.double() / den[:, :, None]
    att[0] = 0.0
    assert not att[1].any()
    want = att.reshape(n, H * D) + bias.double() + res.double()
    want_ln = torch.relu(torch.nn.functional.layer_norm(want, (H * D,), lw.double(), lb.double(),
                                                        1e-5))
    dv = lambda t: t.to(DEV)                            # noqa: E731
    y = ops.mag_attn_epilogue(dv(acc), dv(rmax), dv(rsum), dv(gmax), dv(bias), dv(res))
    y_ln = ops.mag_attn_epilogue(dv(acc), dv(rmax), dv(rsum), dv(gmax), dv(bias), dv(res),
                                 (dv(lw), dv(lb), 1e-5), relu=True)
    y0 = ops.mag_attn_epilogue(dv(acc), dv(rmax), dv(rsum), dv(gmax))
    assert bool(torch.isfinite(y).all()) and not y0[:2].any()
    for got, ref in ((y, want), (y_ln, want_ln)):
        ok, err = G.close(got.cpu().numpy(), ref.numpy(), 1e-5)
        assert ok, f"{err:.3e}"


def test_refused_rows_fall_back_to_the_chain_on_the_device():
    """bf16 rows are outside the fused kernel's range: form=None takes the chain of existing
    operators (never the host), form='fused' raises; the chain's result is the fused one of the
    widened rows up to the bf16 store of the aggregate"""
    from regnn_hip import ops
    blk = _graph("default")[0]
    H, D = 4, 16
    g = torch.Generator().manual_seed(5)
    x = torch.randn(320, H, D, generator=g).bfloat16().to(DEV)
    att_s, att_d = (torch.randn(1, H, D, generator=g).to(DEV) / D ** 0.5 for _ in range(2))
    tab = (torch.randn(R.N_REL, H, generator=g) * 0.5).to(DEV)
    assert not ops.mag_attn_fused_ok("gat", H, D, x) and ops.mag_attn_fused_ok("gat", H, D, x.float())
    with pytest.raises(ValueError):
        ops.mag_attn_scores(blk, x, x, "gat", tab, 0.2, att_s, att_d, form="fused")
    st = ops.mag_attn_scores(blk, x, x, "gat", tab, 0.2, att_s, att_d)
    assert st.form == "chain"
    got = st.finish().float()
    want = ops.mag_attn_infer(blk, x.float(), x.float(), "gat", tab, 0.2, att_s, att_d)
    assert got.is_cuda and got.shape == want.shape
    # each within TOL_F32 x scale of the exact result, scale = sum a |x| <= max |x|; + the store
    slack = 2 * R.TOL_F32 * float(x.float().abs().max())
    assert bool(((got - want).abs() <= R.BF16_REL * want.abs() + slack).all())


# ---- the layer over the fixtures -----------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_inference_layer_matches_fixture(name):
    from regnn_hip import ops
    d = G.load(name)
    m = d["meta"]
    H, C, n_dst, n_src = m["heads"], m["out_channels"], m["n_dst"], m["n_src"]
    v2 = "v2" in m["layer"].lower()
    b = B.fixture_block(d, cap_dst=n_dst, cap_src=n_src)
    ptr, idx, rel = b.live()
    blk = A.RowCsr(ptr, idx, rel, DEV)
    blk.n_src = n_src
    P = {k: torch.from_numpy(v).to(DEV) for k, v in G.sub(d, "p_", np.float32).items()}
    xs = (torch.from_numpy(d["x"]).to(DEV) @ P["lin_src.weight"].t()).view(-1, H, C)
    tab = torch.nn.functional.leaky_relu(P["relation_weight"] * m["scaling_factor"])
    kw = dict(att=P["att"]) if v2 else dict(att_src=P["att_src"], att_dst=P["att_dst"])
    res = xs[:n_dst].reshape(n_dst, H * C) if m["residual"] else None
    assert m["use_norm"] == "ln"
    for form in ("fused", "chain"):
        y = ops.mag_attn_infer(blk, xs, xs[:n_dst], "gatv2" if v2 else "gat", tab,
                               m["negative_slope"], bias=P["bias"], residual=res,
                               ln=(P["norm.weight"], P["norm.bias"], 1e-5), form=form, **kw)
        ok, err = G.close(y.cpu().numpy(), d["out"], 1e-5)
        print(f"{name} {form}: rel err {err:.2e}")
        assert ok, f"{form}: rel err {err:.3e}"


# ---- the model -----------------------------------------------------------------------------------
_MAG = {}


def _mag():
    """synth.mag_like(0.002, seed=1) set up as test_gpu_ns_gat._mag does, once"""
    if _MAG:
        return _MAG
    from regnn_hip import synth
    from regnn_hip.graph import RelGraph
    gd = synth.mag_like(0.002, seed=1, device=DEV)
    keep = gd["rel"] <= 7
    rg = RelGraph(gd["src"][keep], gd["dst"][keep], gd["N"], DEV)
    edge_type = gd["rel"][keep].to(torch.int64) - 1
    node_type = gd["ntype"]
    offs = torch.tensor([gd["type_offsets"][t] for t in synth.NTYPES], device=DEV)
    local = torch.arange(gd["N"], device=DEV) - offs[node_type]
    feats = synth.type_features(gd["counts"], {t: 16 for t in synth.NTYPES}, seed=1, device=DEV)
    x_dict = {k: f for k, f in enumerate(feats)}
    _MAG.update(rg=rg, edge_type=edge_type, node_type=node_type, local=local, x_dict=x_dict,
                n_paper=gd["counts"]["paper"],
                csr=A.full_csr_with_loops(rg, edge_type, node_type, 7))
    return _MAG


def _model(d, model, **kw):
    from regnn_hip import mag
    torch.manual_seed(0)
    kw = {"use_norm": "ln", "self_loop_type": 2, **kw}
    return mag.REGNN(16, 8, 5, 2, 10.0, 0.0, {k: 16 for k in d["x_dict"]}, 7, model=model,
                     heads=2, **kw).to(DEV).eval()


def _restated(d, m, key):
    if key not in d:
        d[key] = A.model_restated(m, d["csr"], d["node_type"], d["local"], d["x_dict"]).numpy()
    return d[key]


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("model", ["regat", "regatv2"])
def test_model_inference_matches_restatement_and_exact_size_path(model, residual):
    from regnn_hip.sampler import NeighborSampler
    d = _mag()
    m = _model(d, model, residual=residual)
    loader = NeighborSampler(d["rg"], None, [-1], batch_size=4096, shuffle=False)
    out = m.inference(d["x_dict"], loader, d["edge_type"], d["node_type"], d["local"], DEV)
    ref = _restated(d, m, ("ref", model, residual))
    assert out.shape == ref.shape
    ok, err = G.close(out.cpu().numpy(), ref, 1e-5)
    print(f"{model} residual={residual}: inference against fp64 restatement {err:.2e}")
    assert ok, f"inference rel err {err:.3e}"
    # the model's own exact-size path on full-neighbour batches: the same logits for the targets
    idx = torch.arange(0, d["n_paper"], 7, device=DEV)
    smp = NeighborSampler(d["rg"], idx, [-1, -1], batch_size=64, shuffle=False)
    seen = 0
    with torch.no_grad():
        for k, (bs, n_id, adjs) in enumerate(smp):
            if k == 2:
                break
            z = m(n_id, d["x_dict"], adjs, d["edge_type"], d["node_type"], d["local"], logits=True)
            ok, err = G.close(out[n_id[:bs]].cpu().numpy(), z.cpu().numpy().astype(np.float64),
                              1e-5)
            print(f"{model} residual={residual} batch {k}: against the exact-size path {err:.2e}")
            assert ok, f"batch {k}: rel err {err:.3e}"
            seen += bs
    assert seen > 0


@pytest.mark.parametrize("model", ["regat", "regatv2"])
def test_sharded_lockstep_equals_one_rank_and_argmax(model):
    from regnn_hip.inference import ShardedInference, shard_bounds
    d = _mag()
    m = _model(d, model, residual=True)
    args = (m, d["rg"], d["edge_type"], d["node_type"], d["local"])
    W = 3
    bounds = shard_bounds(d["rg"].csr_ptr, W)
    ranks = [ShardedInference(*args, r, W, bounds) for r in range(W)]
    xs = [s.input(d["x_dict"], 0)[1] for s in ranks]
    for layer in range(m.num_layers):
        xs_all = torch.cat(xs, 0)                        # what exchange_rows returns
        st = [s.attention_scores(layer, xs_all, xr) for s, xr in zip(ranks, xs)]
        gmax = torch.stack([t.gmax for t in st]).amax(0)  # the MAX all-reduce
        xl = [s.attention_finish(layer, t, xr, gmax=gmax) for s, t, xr in zip(ranks, st, xs)]
        if layer + 1 < m.num_layers:
            xs = [s.project(layer + 1, x) for s, x in zip(ranks, xl)]
    out = torch.cat([s.head(x) for s, x in zip(ranks, xl)], 0)
    one_rank = ShardedInference(*args)
    one = one_rank.run(d["x_dict"])
    ok, err = G.close(out.cpu().numpy(), one.cpu().numpy().astype(np.float64), 1e-5)
    print(f"{model}: three ranks against one {err:.2e}")
    assert ok, f"sharded rel err {err:.3e}"
    ref = _restated(d, m, ("ref", model, True))
    ok, err = G.close(out.cpu().numpy(), ref, 1e-5)
    assert ok, f"sharded against the restatement: rel err {err:.3e}"
    am = one_rank.run(d["x_dict"], gather="argmax").cpu().numpy()
    z = one.cpu().numpy()
    top2 = np.sort(z, 1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 1e-4
    assert am.dtype == np.int64 and am.shape == (z.shape[0],)
    assert np.array_equal(am[clear], z.argmax(1)[clear])
    assert clear.mean() > 0.9
