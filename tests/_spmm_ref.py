"""fp64 references of the relation SpMM (re_spmm.hip: ops.re_spmm, ops.edge_spmm, the raw
regnn_spmm_bwd, ops.re_spmm_fused) with a per-element error scale, the input recipes, the width
ladder and the bipartite ladder graph of the SpMM parity tests (test_cpu_spmm_ref.py,
test_gpu_spmm_tiers.py). A plain helper: no test lives here. The metric, the bounds and the
ladder graph are _attention_ref's.

The operation, over the CSR edge list (ptr, idx, rel_csr), every factor optional:
  y[v] = post[v] * sum_{e: u->v} tab[rel_e] * ew_e * pre[u] * x[u] + bias
`spmm_reference` is the torch restatement with autograd, run in the dtype of its inputs: fp64 is
the reference, fp32 the yardstick of what the arithmetic alone costs (test_cpu_spmm_ref.py).

The error of a tensor is  max |got - ref| / (scale + 2^-100)  elementwise (_attention_ref.rel_err),
`scale` being the same reduction with every product replaced by its absolute value
(a_e = |tab_e| |ew_e|, T_e = sum_d |post_v gy_v| |pre_u x_u|):
  y[v]      |post_v| sum_e a_e |pre_u| |x_u| + |bias|     g_x[u]   |pre_u| sum_e a_e |post_v| |gy_v|
  g_tab[r]  sum_{rel_e = r} |ew_e| T_e                    g_ew[e]  |tab_e| T_e
  g_pre[u]  sum_{e from u} a_e T_e / |pre_u|              g_post[v] sum_{e into v} a_e T_e / |post_v|
  g_bias    sum_v |gy_v|
so an error confined to a short row, or one dropped edge of a 300-edge row, is measured against
that row's own magnitude; an element whose scale is 0 (a row without edges) must be exactly 0.
When `pre is post` (the same_scale case of ops._ReSpmm) the one leaf's gradient and its scale are
the sums of the two."""
import numpy as np
import torch

from _attention_ref import (BF16_REL, FLOOR, IN_DEGREES, N_REL, OUT_DEGREES,  # noqa: F401
                            PLAN_FORMS, TOL_F32, TOL_GUARD, _edges, ladder_edges, ladder_graph,
                            rel_err)

# the nvec ladder: 16-byte vectors per row -> the (LPR, NV) branch of dispatch<T>() it lands in
# (re_spmm.hip); one ragged (a row that does not fill LPR * NV vectors) and one full width each.
# F = 4 nvec floats (fp32) or 8 nvec (bf16).
WIDTHS = {
    1: "LPR=4 NV=1 ragged",
    3: "LPR=4 NV=1 ragged",
    4: "LPR=4 NV=1 full",
    5: "LPR=8 NV=1 ragged",
    8: "LPR=8 NV=1 full",
    9: "LPR=16 NV=1 ragged",
    15: "LPR=16 NV=1 ragged",
    16: "LPR=16 NV=1 FULL (launch_f16v, rows in flight by regnn_tune key 2)",
    17: "LPR=16 NV=2 ragged",
    32: "LPR=16 NV=2 full",
    33: "LPR=16 NV=3 ragged",
    48: "LPR=16 NV=3 full",
    49: "LPR=16 NV=4 ragged",
    64: "LPR=16 NV=4 full",
    65: "LPR=64 NV=2 ragged",
    128: "LPR=64 NV=2 full",
    129: "LPR=64 NV=4 ragged",
    256: "LPR=64 NV=4 full",
}
N_EXTRA = 40                   # source-only nodes of the bipartite ladder


def width(nvec, bf16=False):
    return nvec * (8 if bf16 else 4)


# ---- the restatement ---------------------------------------------------------------------------
def _edge_coef(rel_csr, tab, edge_w):
    """tab[rel_e] * ew_e per CSR edge, or None when both are absent"""
    c = None
    if tab is not None:
        c = tab.reshape(-1)[rel_csr.long()]
    if edge_w is not None:
        c = edge_w.reshape(-1) if c is None else c * edge_w.reshape(-1)
    return c


def spmm_reference(ptr, idx, rel_csr, x, tab=None, pre=None, post=None, bias=None, edge_w=None):
    """y of the module docstring in the dtype of x; edge_w in CSR edge order."""
    src, dst, n_dst = _edges(ptr, idx)
    m = x if pre is None else x * pre[:, None]
    m = m[src]
    c = _edge_coef(rel_csr, tab, edge_w)
    if c is not None:
        m = m * c[:, None]
    y = torch.zeros(n_dst, x.shape[1], dtype=x.dtype, device=x.device).index_add(0, dst, m)
    if post is not None:
        y = y * post[:, None]
    if bias is not None:
        y = y + bias
    return y


def _leaf(t):
    return None if t is None else t.detach().double().clone().requires_grad_(True)


def spmm_case_ref(ptr, idx, rel_csr, x, tab, pre, post, bias, gy, n_src, edge_w=None):
    """fp64 reference and scale of every output of one SpMM case: dicts over y, g_x and
    whichever of g_tab, g_pre, g_post, g_bias, g_ew exist. `pre is post`: g_pre alone, combined."""
    same = pre is not None and pre is post
    assert x.shape[0] == n_src
    x_, tab_, pre_, bias_, ew_ = (_leaf(t) for t in (x, tab, pre, bias, edge_w))
    post_ = pre_ if same else _leaf(post)
    gy = gy.detach().double()
    y = spmm_reference(ptr, idx, rel_csr, x_, tab_, pre_, post_, bias_, ew_)
    y.backward(gy)
    want = {"y": y.detach(), "g_x": x_.grad}
    for k, t in (("g_tab", tab_), ("g_pre", pre_), ("g_bias", bias_), ("g_ew", ew_)):
        if t is not None:
            want[k] = t.grad
    if post_ is not None and not same:
        want["g_post"] = post_.grad

    src, dst, n_dst = _edges(ptr, idx)
    F = x.shape[1]
    with torch.no_grad():
        z = lambda *s: torch.zeros(*s, dtype=torch.float64)          # noqa: E731
        one = torch.ones((), dtype=torch.float64)
        P = one.expand(n_src) if pre_ is None else pre_.abs()
        Q = one.expand(n_dst) if post_ is None else post_.abs()
        at = one.expand(src.numel()) if tab_ is None else tab_.reshape(-1)[rel_csr.long()].abs()
        aw = one.expand(src.numel()) if ew_ is None else ew_.reshape(-1).abs()
        a = at * aw
        xs, gs = x_.abs() * P[:, None], gy.abs() * Q[:, None]       # |pre x|, |post gy|
        scale = {"y": z(n_dst, F).index_add(0, dst, a[:, None] * xs[src]) * Q[:, None],
                 "g_x": z(n_src, F).index_add(0, src, a[:, None] * gs[dst]) * P[:, None]}
        if bias_ is not None:
            scale["y"] = scale["y"] + bias_.abs()
            scale["g_bias"] = gy.abs().sum(0)
        T = (gs[dst] * xs[src]).sum(1)
        if tab_ is not None:
            scale["g_tab"] = z(tab_.numel()).index_add(0, rel_csr.long(), aw * T).view_as(tab_)
        if ew_ is not None:
            scale["g_ew"] = (at * T).view_as(ew_)
        s_pre = z(n_src).index_add(0, src, a * T) / P
        s_post = z(n_dst).index_add(0, dst, a * T) / Q
        if same:
            assert n_src == n_dst
            scale["g_pre"] = s_pre + s_post
        else:
            if pre_ is not None:
                scale["g_pre"] = s_pre
            if post_ is not None:
                scale["g_post"] = s_post
    assert sorted(want) == sorted(scale)
    return want, scale


# ---- the fused forward epilogue ----------------------------------------------------------------
def fused_ref(ptr, idx, rel_csr, x, tab=None, post=None, bias=None, residual=None, ln=None,
              relu=False):
    """act(LayerNorm(post * agg + bias + residual)) of ops.re_spmm_fused in fp64 (the dtype of
    its inputs after .double()), every piece optional; ln = (weight, bias, eps) or None.
    Returns (ref, den, min_std): den [n_dst, 1] = max(1, max |ref| over the row), the divisor of
    fused_err, and min_std the smallest pre-LN standard deviation over the rows that are not
    constant (inf without LN). A constant row normalises to exactly ln_b."""
    d = lambda t: None if t is None else t.detach().double()         # noqa: E731
    v = spmm_reference(ptr, idx, rel_csr, d(x), d(tab), None, d(post), d(bias))
    if residual is not None:
        v = v + d(residual)
    min_std = float("inf")
    if ln is not None:
        w, b, eps = ln
        mean = v.mean(1, keepdim=True)
        c = v - mean
        var = (c * c).mean(1, keepdim=True)
        std = var.sqrt().flatten()
        varied = (v != v[:, :1]).any(1)
        if bool(varied.any()):
            min_std = float(std[varied].min())
        v = c / (var + eps).sqrt()
        if w is not None:
            v = v * d(w)
        if b is not None:
            v = v + d(b)
    if relu:
        v = v.clamp(min=0.0)
    den = v.abs().amax(1, keepdim=True).clamp(min=1.0)
    return v, den, min_std


def fused_err(got, ref, den, bf16_store=False):
    """max |got - ref| / max(1, max |ref| over the row); bf16_store as rel_err's."""
    got = got.detach().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "NaN / inf in a kernel output"
    err = (got - ref).abs()
    if bf16_store:
        err = (err - BF16_REL * ref.abs()).clamp(min=0.0)
    return float((err / den).max().item())


# ---- input recipe ------------------------------------------------------------------------------
def spmm_inputs(F, n_src, n_dst, n_rel, seed, bf16=False, n_edge=None):
    """fp32 CPU tensors of one case, a dict: x [n_src, F], gy [n_dst, F] randn (bf16-representable
    when bf16); tab [n_rel] randn * 0.5, signs mixed as a LeakyReLU'd relation table's are; pre
    [n_src], post [n_dst] uniform in [0.5, 1.5] (degree norms are positive); bias [F] randn;
    edge_w [n_edge] randn when n_edge is given (the caller's edge order)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)    # noqa: E731
    u = lambda n: torch.rand(n, generator=g, dtype=torch.float32) + 0.5  # noqa: E731
    d = {"x": r(n_src, F), "gy": r(n_dst, F), "tab": r(n_rel) * 0.5, "pre": u(n_src),
         "post": u(n_dst), "bias": r(F)}
    if n_edge is not None:
        d["edge_w"] = r(n_edge)
    if bf16:
        d["x"], d["gy"] = d["x"].bfloat16().float(), d["gy"].bfloat16().float()
    return d


def fused_inputs(F, n_src, n_dst, n_rel, seed, bf16=False):
    """spmm_inputs for the fused epilogue, kept away from rows that a LayerNorm would blow up:
    |tab| >= 0.5 (signs still mixed) and the columns of x offset by +2, -2, +2, ..., so a row
    with a single edge, without bias and residual, still deviates by more than 0.1 (the callers
    assert it). Adds residual [n_dst, F] randn, ln_w = 1 + 0.1 randn, ln_b = 0.1 randn."""
    d = spmm_inputs(F, n_src, n_dst, n_rel, seed)
    g = torch.Generator().manual_seed(seed + 7919)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)    # noqa: E731
    d["tab"] = torch.where(d["tab"] >= 0, 1.0, -1.0) * (0.5 + d["tab"].abs())
    d["x"] = d["x"] + 2.0 * (1.0 - 2.0 * (torch.arange(F) % 2))
    d.update(residual=r(n_dst, F), ln_w=1.0 + 0.1 * r(F), ln_b=0.1 * r(F))
    if bf16:
        d["x"], d["residual"] = d["x"].bfloat16().float(), d["residual"].bfloat16().float()
    return d


# ---- the bipartite ladder ----------------------------------------------------------------------
def bipartite_edges(N=320, seed=13):
    """ladder_edges(N) plus N_EXTRA source-only nodes N .. N+39 with 200 more edges from them
    into the plain nodes (so IN_DEGREES of nodes 0..24 stay); (src, dst, rel) int64."""
    src, dst, rel = ladder_edges(N)
    first = len(IN_DEGREES) + len(OUT_DEGREES)               # the first plain node
    rng = np.random.default_rng(seed)
    s = rng.integers(N, N + N_EXTRA, 200)
    s[:N_EXTRA] = np.arange(N, N + N_EXTRA)                 # every extra node has an out-edge
    d = rng.integers(first, N, 200)
    r = rng.integers(1, N_REL + 1, 200)
    perm = rng.permutation(src.size + 200)                   # edge ids unrelated to the rows
    return (np.concatenate([src, s])[perm].astype(np.int64),
            np.concatenate([dst, d])[perm].astype(np.int64),
            np.concatenate([rel, r])[perm].astype(np.int64))


def ladder_bipartite(form="default", device="cpu", N=320):
    """(RelGraph, e_feat) with n_src = N + 40 sources and n_dst = N destinations."""
    from regnn_hip.graph import RelGraph
    src, dst, rel = bipartite_edges(N)
    split, chunk = PLAN_FORMS[form]
    rg = RelGraph(src, dst, N + N_EXTRA, device, num_dst=N, split=split, chunk=chunk)
    return rg, torch.from_numpy(rel).to(device)
