"""The inputs of the per-element attention parity tests are well conditioned: for every input
recipe of _attention_ref.py and every fp32 (H, D) of the parity matrix, an fp32 torch run of the
fp64 restatement stays at or below 2.5e-6 under the per-element metric, a quarter of the
kernels' bound of 1e-5 (worst measured 1.0e-6). What a kernel may add on top is the rest:
__expf's argument scaling and its own summation orders. The fp32 run of the global-max softmax
holds the one maximum constant, as the kernels' backward does (_attention_ref._softmax); the
fp64 reference differentiates it. Also pins the ladder graph's degrees and plans. No GPU, no
HIP library."""
import pytest
import torch

import _attention_ref as R

N = 320
# every fp32 (H, D) of the issue's matrix: one per dispatch tier, H = 16 / 32, generic head counts
SHAPES = [(1, 4), (4, 16), (8, 16), (1, 128), (16, 16), (32, 8), (8, 64), (2, 256), (16, 64),
          (32, 64), (3, 4), (6, 8), (12, 16), (64, 4)]
WIDE = [(4, 16), (32, 8), (3, 4)]


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
