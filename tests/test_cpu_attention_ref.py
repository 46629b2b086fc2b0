"""The inputs of the per-element attention parity tests are well conditioned: for every input
recipe of _attention_ref.py and every fp32 (H, D) of the parity matrix, an fp32 torch run of the
fp64 restatement stays at or below 2.5e-6 under the per-element metric, a quarter of the
kernels' bound of 1e-5 (worst measured 1.0e-6). What a kernel may add on top is the rest:
__expf's argument scaling and its own summation orders. The fp32 run of the global-max softmax
holds the one maximum constant, as the kernels' backward does (_attention_ref._softmax); the
fp64 reference differentiates it. The same guard covers what test_gpu_attention_matrix.py adds:
the bf16-representable inputs, GATv2 with one shared leaf, the per-edge tensors under the scale
|reference| and the score operator alone. Also pins the ladder graph's degrees and plans and the
shape predicates of ops.py against the dispatch tables. No GPU; no kernel is launched."""
import pytest
import torch

import _attention_ref as R

N = 320
SHAPES, WIDE = R.SHAPES, R.WIDE     # the matrix's shapes: one table for this file and the GPU's


@pytest.fixture(scope="module")
def graph():
    rg, e_feat = R.ladder_graph("default", "cpu", N)
    return rg, rg.rel_pack(e_feat, num_rel=R.N_REL).rel_csr


def _fp32(fn, inputs, gy, names):
    leaves = [None if t is None else t.detach().float().clone().requires_grad_(True)
              for t in inputs]
    out = fn(*leaves)
    out.backward(gy.float())
    got = {"out": out.detach()}
    got.update({k: t.grad for k, t in zip(names, leaves) if t is not None})
    return got


def _check(got, want, scale):
    for k in want:
        err = R.rel_err(got[k], want[k], scale[k])
        assert err <= R.TOL_GUARD, f"{k}: fp32 restatement err {err:.3e}"


def test_ladder_graph_forms():
    src, dst, rel = R.ladder_edges(N)
    assert 3000 <= src.size <= 4000 and rel.min() == 1 and rel.max() == R.N_REL
    for form in R.PLAN_FORMS:
        rg, _ = R.ladder_graph(form, "cpu", N)
        deg = (rg.csr_ptr[1:] - rg.csr_ptr[:-1]).tolist()
        assert deg[:len(R.IN_DEGREES)] == R.IN_DEGREES
        out = (rg.csc_ptr[1:] - rg.csc_ptr[:-1]).tolist()
        assert out[len(R.IN_DEGREES):len(R.IN_DEGREES) + len(R.OUT_DEGREES)] == R.OUT_DEGREES
    rg, _ = R.ladder_graph("tree", "cpu", N)
    assert rg.csr_plan.n_levels >= 2 and rg.csc_plan.n_levels >= 2


def test_shape_predicates_mirror_the_dispatch_tables():
    """ops.heads_ok / gatv2_scores_ok / edge_softmax_ok against the tier tables of dispatch_heads
    and launch_gatv2 and sm_log2, restated here: a row of nvec 16-byte vectors takes the first
    (lanes, vectors per lane) tier that holds it and whose lanes hold one head's vph vectors,
    vph a power of two. (Imports the Python side of the library; nothing is launched.)"""
    from regnn_hip import ops
    tiers = [(16, 1), (16, 2), (16, 4), (64, 2), (64, 4), (64, 8)]

    def takes(table, H, D, ev):
        if D % ev:
            return False
        nvec, vph = H * D // ev, D // ev
        return vph & (vph - 1) == 0 and any(nvec <= l * n and vph <= l for l, n in table)
    for H in list(range(1, 40)) + [64, 65, 128, 512, 513]:
        for D in list(range(1, 70)) + [96, 128, 256, 260, 512]:
            assert ops.heads_ok(H, D, torch.float32) == takes(tiers, H, D, 4), (H, D)
            assert ops.heads_ok(H, D, torch.bfloat16) == takes(tiers, H, D, 8), (H, D)
            assert ops.gatv2_scores_ok(H, D) == takes(tiers[:5], H, D, 4), (H, D)
    assert [h for h in range(0, 70) if ops.edge_softmax_ok(h)] == [1, 2, 4, 8, 16, 32]
    for H, D in R.POW2_SHAPES:
        assert ops.heads_ok(H, D) and ops.gat_fused_ok(H) and ops.edge_softmax_ok(H)
    assert all(ops.gatv2_scores_ok(H, D) for H, D in R.V2_SHAPES + [(3, 8)])
    assert all(ops.heads_ok(H, D, torch.bfloat16) for H, D in R.BF16_SHAPES)
    with pytest.raises(ValueError, match=r"ops\.head_spmm: unsupported shape \(H=4, D=12, float32"):
        ops.head_spmm(None, None, torch.zeros(2, 4, 12))


@pytest.mark.parametrize("global_max", [False, True])
@pytest.mark.parametrize("recipe,H,D", [("unit", H, D) for H, D in SHAPES] +
                         [("wide", H, D) for H, D in WIDE])
def test_gat_recipe_conditioned(graph, recipe, H, D, global_max):
    rg, rel = graph
    ft, el, er, tab, gy, slope = R.gat_inputs(recipe, N, H, D, R.N_REL, seed=H * 1000 + D)
    want, scale = R.gat_case_ref(rg.csr_ptr, rg.csr_idx, rel, el, er, tab, ft, gy, slope,
                                 global_max)
    got = _fp32(lambda el_, er_, tab_, ft_: R.gat_reference(rg.csr_ptr, rg.csr_idx, rel, el_, er_,
                                                            tab_, ft_, slope,
                                                            global_max and "detached"),
                [el, er, tab, ft], gy, ["g_el", "g_er", "g_tab", "g_ft"])
    _check(got, want, scale)


@pytest.mark.parametrize("H,D", SHAPES)
def test_gat_attn_recipe_conditioned(graph, H, D):
    rg, rel = graph
    ft, al, ar, tab, gy, slope = R.gat_attn_inputs(N, H, D, R.N_REL, seed=H * 1000 + D)
    want, scale = R.gat_attn_case_ref(rg.csr_ptr, rg.csr_idx, rel, al, ar, tab, ft, gy, slope)

    def fn(al_, ar_, tab_, ft_):
        return R.gat_reference(rg.csr_ptr, rg.csr_idx, rel, (ft_ * al_).sum(-1),
                               (ft_ * ar_).sum(-1), tab_, ft_, slope)
    _check(_fp32(fn, [al, ar, tab, ft], gy, ["g_al", "g_ar", "g_tab", "g_ft"]), want, scale)


@pytest.mark.parametrize("global_max", [False, True])
@pytest.mark.parametrize("recipe,H,D", [("unit", H, D) for H, D in SHAPES if H & (H - 1) == 0] +
                         [("wide", H, D) for H, D in WIDE if H & (H - 1) == 0])
def test_gatv2_recipe_conditioned(graph, recipe, H, D, global_max):
    rg, rel = graph
    fs, fd, att, tab, ft, gy, slope = R.gatv2_inputs(recipe, N, H, D, R.N_REL, seed=H * 1000 + D)
    want, scale = R.gatv2_case_ref(rg.csr_ptr, rg.csr_idx, rel, fs, fd, att, tab, ft, gy, slope,
                                   global_max)
    got = _fp32(lambda *t: R.gatv2_reference(rg.csr_ptr, rg.csr_idx, rel, *t, slope,
                                             global_max and "detached"),
                [fs, fd, att, tab, ft], gy, ["g_fs", "g_fd", "g_att", "g_tab", "g_ft"])
    _check(got, want, scale)


@pytest.mark.parametrize("H,D", R.BF16_SHAPES)
def test_gat_bf16_recipe_conditioned(graph, H, D):
    """the bf16-row cases: ft and gy bf16-representable (the reference takes the same values, so
    the guard is on fp32 arithmetic alone; the kernels' bf16 stores are rel_err's bf16_store)"""
    rg, rel = graph
    ft, el, er, tab, gy, slope = R.gat_inputs("unit", N, H, D, R.N_REL, seed=H * 1000 + D,
                                              bf16=True)
    assert torch.equal(ft, ft.bfloat16().float()) and torch.equal(gy, gy.bfloat16().float())
    want, scale = R.gat_case_ref(rg.csr_ptr, rg.csr_idx, rel, el, er, tab, ft, gy, slope)
    got = _fp32(lambda el_, er_, tab_, ft_: R.gat_reference(rg.csr_ptr, rg.csr_idx, rel, el_, er_,
                                                            tab_, ft_, slope),
                [el, er, tab, ft], gy, ["g_el", "g_er", "g_tab", "g_ft"])
    _check(got, want, scale)


@pytest.mark.parametrize("global_max", [False, True])
@pytest.mark.parametrize("H,D", R.SHARED_SHAPES)
def test_gatv2_shared_leaf_conditioned(graph, H, D, global_max):
    """GATv2 with fs, fd and ft one leaf: its gradient against the sum of the three scales"""
    rg, rel = graph
    x, att, tab, gy, slope = R.gatv2_shared_inputs(N, H, D, R.N_REL, seed=H * 1000 + D)
    want, scale = R.gatv2_shared_case_ref(rg.csr_ptr, rg.csr_idx, rel, x, att, tab, gy, slope,
                                          global_max)
    got = _fp32(lambda x_, att_, tab_: R.gatv2_reference(rg.csr_ptr, rg.csr_idx, rel, x_, x_, att_,
                                                         tab_, x_, slope,
                                                         global_max and "detached"),
                [x, att, tab], gy, ["g_x", "g_att", "g_tab"])
    _check(got, want, scale)


@pytest.mark.parametrize("H,D", R.DIRECT_SHAPES)
def test_direct_per_edge_conditioned(graph, H, D):
    """the per-edge tensors under the scale |reference|: the attention a of GAT and of GATv2
    (both recipes, both softmax forms, with and without the table) and the GATv2 score of `wide`,
    which fp32 forms exactly. The `unit` score is left out of this scale: see DIRECT_SHAPES."""
    rg, rel = graph
    ptr, idx = rg.csr_ptr, rg.csr_idx
    f64 = lambda t: None if t is None else t.double()   # noqa: E731
    for recipe in ("unit", "wide"):
        ft, el, er, tab, gy, slope = R.gat_inputs(recipe, N, H, D, R.N_REL, seed=H * 1000 + D)
        fs, fd, att, tab2, _, _, slope2 = R.gatv2_inputs(recipe, N, H, D, R.N_REL,
                                                         seed=H * 1000 + D)
        for global_max in (False, True):
            for t, t2 in ((tab, tab2), (None, None)):
                ref = R.gat_attention_ref(ptr, idx, rel, el.double(), er.double(), f64(t), slope,
                                          global_max)
                got = R.gat_attention_ref(ptr, idx, rel, el, er, t, slope,
                                          global_max and "detached")
                err = R.rel_err(got, ref, ref.abs())
                assert err <= R.TOL_GUARD, f"gat a {recipe} gmax={global_max}: {err:.3e}"
                ref = R.gatv2_attention_ref(ptr, idx, rel, fs.double(), fd.double(), att.double(),
                                            f64(t2), slope2, global_max)
                got = R.gatv2_attention_ref(ptr, idx, rel, fs, fd, att, t2, slope2,
                                            global_max and "detached")
                err = R.rel_err(got, ref, ref.abs())
                assert err <= R.TOL_GUARD, f"gatv2 a {recipe} gmax={global_max}: {err:.3e}"
        if recipe == "wide":
            ref = R.gatv2_score_ref(ptr, idx, fs.double(), fd.double(), att.double(), slope2)
            assert torch.equal(R.gatv2_score_ref(ptr, idx, fs, fd, att, slope2).double(), ref)


@pytest.mark.parametrize("H,D", R.SCORE_SHAPES)
def test_gatv2_score_alone_conditioned(graph, H, D):
    """the score operator alone (`unit`), s and its three gradients under the scale of their
    terms; (3, 8) is the boundary shape it takes while the edge softmax refuses H = 3"""
    rg, rel = graph
    fs, fd, att, _, _, _, slope = R.gatv2_inputs("unit", N, H, D, R.N_REL, seed=H * 1000 + D)
    gs = R.score_grad(rg.E, H, seed=H * 1000 + D)
    want, scale = R.gatv2_score_case_ref(rg.csr_ptr, rg.csr_idx, fs, fd, att, gs, slope)
    leaves = [t.clone().requires_grad_(True) for t in (fs, fd, att)]
    s = R.gatv2_score_ref(rg.csr_ptr, rg.csr_idx, *leaves, slope)
    s.backward(gs)
    got = {"s": s.detach(), "g_fs": leaves[0].grad, "g_fd": leaves[1].grad,
           "g_att": leaves[2].grad}
    _check(got, want, scale)
