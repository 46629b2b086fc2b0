"""The inputs of the per-element SpMM parity tests are well conditioned, and the metric bites.

Conditioning: for every fp32 width of _spmm_ref.WIDTHS, an fp32 torch run of the fp64
restatement (spmm_reference, fused_ref) stays at or below 2.5e-6 under the per-element metric, a
quarter of the kernels' bound of 1e-5, on the ladder graph and on the bipartite ladder. The
restatement reads the CSR edge list only, which is the same in every plan form (asserted), so one
fp32 run stands for the three forms. What a kernel may add on top is its own summation order.

The metric bites: four single-edge perturbations of the fp64 reference each exceed ten times the
kernels' bound. Also pins the bipartite ladder's degrees. No GPU, no HIP library."""
import pytest
import torch

import _spmm_ref as R

N = 320
F32_WIDTHS = [R.width(nv) for nv in R.WIDTHS]
NAMES = ["x", "tab", "pre", "post", "bias", "edge_w"]


@pytest.fixture(scope="module")
def graphs():
    """kind -> (ptr, idx, rel_csr, n_src, csr_eid) of the default form; the other forms hold the
    same CSR."""
    out = {}
    for kind, make in (("ladder", R.ladder_graph), ("bipartite", R.ladder_bipartite)):
        forms = {}
        for form in R.PLAN_FORMS:
            rg, e_feat = make(form, "cpu", N)
            forms[form] = (rg, rg.rel_pack(e_feat, num_rel=R.N_REL).rel_csr)
        rg, rel = forms["default"]
        for form, (other, orel) in forms.items():
            assert torch.equal(other.csr_ptr, rg.csr_ptr) and torch.equal(other.csr_idx, rg.csr_idx)
            assert torch.equal(orel, rel) and torch.equal(other.csr_eid, rg.csr_eid), form
        out[kind] = (rg.csr_ptr, rg.csr_idx, rel, rg.n_src, rg.csr_eid)
    return out


def _fp32(ptr, idx, rel, t, gy, same):
    """an fp32 torch run of the restatement: y and the gradients of the given inputs"""
    leaves = {k: v.detach().float().clone().requires_grad_(True) for k, v in t.items()
              if v is not None}
    if same:
        leaves["post"] = leaves["pre"]
    y = R.spmm_reference(ptr, idx, rel, leaves["x"], *(leaves.get(k) for k in NAMES[1:]))
    y.backward(gy.float())
    got = {"y": y.detach()}
    for k, v in leaves.items():
        if not (same and k == "post"):
            got["g_ew" if k == "edge_w" else "g_" + k] = v.grad
    return got


@pytest.mark.parametrize("F", F32_WIDTHS)
@pytest.mark.parametrize("kind", ["ladder", "bipartite"])
def test_spmm_recipe_conditioned(graphs, kind, F):
    """ladder: the matrix's case (table, pre is post, bias) and the per-edge-weight case;
    bipartite: distinct pre [n_src] and post [n_dst] with table, edge weights and bias."""
    ptr, idx, rel, n_src, eid = graphs[kind]
    d = R.spmm_inputs(F, n_src, N, R.N_REL, seed=F, n_edge=idx.numel())
    ew = d["edge_w"][eid]
    if kind == "ladder":
        cases = [({"x": d["x"], "tab": d["tab"], "pre": d["pre"], "post": d["pre"],
                   "bias": d["bias"]}, True),
                 ({"x": d["x"], "edge_w": ew}, False)]
    else:
        cases = [({"x": d["x"], "tab": d["tab"], "pre": d["pre"], "post": d["post"],
                   "bias": d["bias"], "edge_w": ew}, False)]
    for t, same in cases:
        args = [t.get(k) for k in NAMES]
        want, scale = R.spmm_case_ref(ptr, idx, rel, args[0], args[1], args[2],
                                      args[2] if same else args[3], args[4], d["gy"], n_src,
                                      edge_w=args[5])
        got = _fp32(ptr, idx, rel, t, d["gy"], same)
        assert sorted(got) == sorted(want)
        for k in want:
            err = R.rel_err(got[k], want[k], scale[k])
            assert err <= R.TOL_GUARD, f"{k}: fp32 restatement err {err:.3e}"


@pytest.mark.parametrize("F", F32_WIDTHS)
def test_fused_recipe_conditioned(graphs, F):
    """an fp32 run of fused_ref's arithmetic (LayerNorm after the aggregation) under its row
    metric; the pre-LN deviation of every row that is not constant is >= 0.1, so the LayerNorm
    amplifies the aggregation's rounding by at most ten."""
    ptr, idx, rel, n_src, _ = graphs["ladder"]
    d = e = R.fused_inputs(F, n_src, N, R.N_REL, seed=F)
    for bias, res in ((d["bias"], e["residual"]), (None, None), (d["bias"], None)):
        ln = (e["ln_w"], e["ln_b"], 1e-5)
        ref, den, min_std = R.fused_ref(ptr, idx, rel, d["x"], d["tab"], d["post"], bias, res, ln,
                                        relu=True)
        print(f"F={F} bias={bias is not None} res={res is not None}: min std {min_std:.3f}")
        assert min_std >= 0.1, min_std
        v = R.spmm_reference(ptr, idx, rel, d["x"], d["tab"], None, d["post"], bias)
        if res is not None:
            v = v + res
        got = torch.relu(torch.nn.functional.layer_norm(v, (F,), ln[0], ln[1], ln[2]))
        err = R.fused_err(got, ref, den)
        assert err <= R.TOL_GUARD, f"fp32 fused restatement err {err:.3e} (min std {min_std:.3f})"
        if bias is None and res is None:
            # row 0 has no edges: constant, and exactly relu(ln_b)
            assert torch.equal(ref[0], e["ln_b"].double().clamp(min=0.0))


# ---- the metric bites --------------------------------------------------------------------------
def _edit(ptr, idx, rel, row, k, op):
    """the CSR with edge k of `row` dropped / doubled / given another relation id"""
    p = int(ptr[row]) + k
    assert p < int(ptr[row + 1])
    ptr, idx, rel = ptr.clone(), idx.clone(), rel.clone()
    if op == "drop":
        keep = torch.ones(idx.numel(), dtype=torch.bool)
        keep[p] = False
        idx, rel = idx[keep], rel[keep]
        ptr[row + 1:] -= 1
    elif op == "twice":
        idx, rel = torch.cat([idx[:p + 1], idx[p:]]), torch.cat([rel[:p + 1], rel[p:]])
        ptr[row + 1:] += 1
    else:
        rel[p] = (rel[p] + 1) % R.N_REL
    return ptr, idx, rel


@pytest.mark.parametrize("op,row,F", [("drop", 24, 64), ("swap", 3, 64), ("zero_vec", 5, 36),
                                      ("twice", 20, 64)])
def test_metric_bites(graphs, op, row, F):
    """drop one edge of the 300-edge row; swap the relation id of one edge of the 3-edge row;
    zero the last 16-byte vector of one row at a ragged width; add one edge's term twice (the
    129-edge row). Each must exceed 10 x the kernels' bound on y."""
    ptr, idx, rel, n_src, _ = graphs["ladder"]
    assert int(ptr[row + 1] - ptr[row]) == R.IN_DEGREES[row]
    d = R.spmm_inputs(F, n_src, N, R.N_REL, seed=F)
    want, scale = R.spmm_case_ref(ptr, idx, rel, d["x"], d["tab"], d["pre"], d["pre"], d["bias"],
                                  d["gy"], n_src)
    dd = {k: v.double() for k, v in d.items()}
    if op == "zero_vec":
        y = want["y"].clone()
        y[row, -4:] = 0.0
    else:
        y = R.spmm_reference(*_edit(ptr, idx, rel, row, 1, op), dd["x"], dd["tab"], dd["pre"],
                             dd["pre"], dd["bias"])
    other = torch.ones(N, dtype=torch.bool)
    other[row] = False
    assert torch.equal(y[other], want["y"][other])
    err = R.rel_err(y, want["y"], scale["y"])
    print(f"{op}: {err:.3e}")
    assert err > 10 * R.TOL_F32, f"{op} measures only {err:.3e}"


def test_bipartite_ladder_degrees():
    src, dst, rel = R.bipartite_edges(N)
    assert 3000 <= src.size <= 4000 and rel.min() == 1 and rel.max() == R.N_REL
    assert src.max() == N + R.N_EXTRA - 1 and dst.max() < N
    for form in R.PLAN_FORMS:
        rg, _ = R.ladder_bipartite(form, "cpu", N)
        assert (rg.n_src, rg.n_dst) == (N + R.N_EXTRA, N)
        deg = (rg.csr_ptr[1:] - rg.csr_ptr[:-1]).tolist()
        assert len(deg) == N and deg[:len(R.IN_DEGREES)] == R.IN_DEGREES
        out = (rg.csc_ptr[1:] - rg.csc_ptr[:-1]).tolist()
        assert len(out) == N + R.N_EXTRA and min(out[N:]) >= 1 and sum(out[N:]) == 200
        assert out[len(R.IN_DEGREES):len(R.IN_DEGREES) + len(R.OUT_DEGREES)] == R.OUT_DEGREES
        if form != "noplan":
            assert rg.csr_plan.n_long > 0 and rg.csc_plan.n_long > 0
        else:
            assert rg.csr_plan.n_long == 0 and rg.csc_plan.n_long == 0
