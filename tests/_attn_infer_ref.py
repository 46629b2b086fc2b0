"""References and inputs of the forward-only attention tests (test_cpu_attn_infer.py,
test_gpu_attn_infer.py: regnn_mag_attn_fwd / _epilogue, ops.mag_attn_*, the attention models in
regnn_hip.inference). A plain helper: no test lives here, and nothing here needs a GPU.

* the `deep` input recipe: _attention_ref's `wide` recipe with 128 subtracted from er[::3] (GAT)
  or from fd[::3] in every column (GATv2, slope 0.25). A third of the rows then lie 30 .. 50
  below the one global maximum, where the 1e-16 of the ogbn-mag softmax (mag/utils.py:45-57)
  is a visible to dominant share of the denominator: with `wide` alone that share is <= 3e-8 and
  a missing correction term could not be seen.
* operator_case: inputs, fp64 reference and the `out` scale (sum_e a_e |x_u|) of one operator
  case, for the kinds "gat_el", "gat_attn" and "gatv2" (message rows = score rows).
* online_reference: the identity the kernels rest on, as plain torch in any dtype -- per-row
  maximum m, S = sum exp(s - m), acc = sum exp(s - m) x, then acc / (S + eps exp(gmax - m)).
* conv_restated / model_restated: the layer-wise inference of the two attention models over
  the full CSR with self loops (_ns_gat_blocks.conv_restated's arithmetic, the attention by
  _attention_ref.gat_reference / gatv2_reference(global_max=True)), then relu, then out_lin.
"""
import numpy as np
import torch
import torch.nn.functional as F

import _attention_ref as R

KINDS = ("gat_el", "gat_attn", "gatv2")
RECIPES = ("unit", "wide", "deep")
SHAPES = [(1, 64), (2, 32), (4, 16), (8, 8), (8, 64), (3, 8)]
DEEP_SHIFT = 128.0


class RowCsr:
    """what ops.mag_attn_scores reads of a row block: csr_ptr / csr_idx / csr_plan, n_dst, E and
    pack.rel_csr (0-based relation ids, uint8)"""

    def __init__(self, ptr, idx, rel, device="cpu", split=256, chunk=256):
        from regnn_hip.graph import SegPlan
        self.csr_ptr = torch.as_tensor(ptr).to(torch.int32).to(device).contiguous()
        self.csr_idx = torch.as_tensor(idx).to(torch.int32).to(device).contiguous()
        self.n_dst, self.E = self.csr_ptr.numel() - 1, int(self.csr_idx.numel())
        self.csr_plan = SegPlan(self.csr_ptr, split, chunk)
        self.pack = type("RowPack", (), {})()
        self.pack.rel_csr = torch.as_tensor(rel).to(torch.uint8).to(device).contiguous()
        self.device = device

    def live(self):
        return self.csr_ptr.cpu(), self.csr_idx.cpu().long(), self.pack.rel_csr.cpu().long()


def csr_of(src, dst, rel, n_dst):
    """(ptr, idx, rel) int64 arrays: the edges stably sorted by destination"""
    order = np.argsort(dst, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n_dst))]).astype(np.int64)
    return ptr, np.asarray(src)[order].astype(np.int64), np.asarray(rel)[order].astype(np.int64)


def ladder_csr(self_loops=False, N=320):
    """the ladder graph (_attention_ref.ladder_edges) as a CSR with 0-based relation ids;
    self_loops: every row's own loop last, relation N_REL + v % 4 (as the row blocks carry)"""
    src, dst, rel = R.ladder_edges(N)
    rel = rel - 1
    if self_loops:
        loop = np.arange(N)
        src, dst = np.concatenate([src, loop]), np.concatenate([dst, loop])
        rel = np.concatenate([rel, R.N_REL + loop % 4])
    return csr_of(src, dst, rel, N)


N_REL_LOOPS = R.N_REL + 4


# ---- operator cases ----------------------------------------------------------------------------
def operator_inputs(kind, recipe, N, H, D, n_rel, seed):
    """fp32 CPU tensors of one operator case, by name. Every kind: x [N, H, D] (the gathered and
    aggregated rows), tab [n_rel, H], slope. gat_el: el, er [N, H]. gat_attn: al [1, H, D] and
    er; el = <x, al> is the kernel's to form (wide / deep: x multiples of 2^-4 plus per-source
    offsets in {-8, 0, 8} and al = 1 / D, so el is exact in fp32 in any order and spans +-9).
    gatv2: xd [N, H, D] (the destinations' rows) and att [1, H, D]."""
    base = "wide" if recipe == "deep" else recipe
    if recipe not in RECIPES:
        raise ValueError(recipe)
    if kind == "gat_el":
        ft, el, er, tab, _gy, slope = R.gat_inputs(base, N, H, D, n_rel, seed)
        c = dict(x=ft, el=el, er=er, tab=tab, slope=slope)
    elif kind == "gat_attn":
        if base == "unit":
            ft, al, ar, tab, _gy, slope = R.gat_attn_inputs(N, H, D, n_rel, seed)
            er = (ft * ar).sum(-1)
        else:
            fs, _fd, _att, tab, _ft, _gy, slope = R.gatv2_inputs("wide", N, H, D, n_rel, seed)
            _f, _el, er, _t, _g, _s = R.gat_inputs("wide", N, H, D, n_rel, seed + 1)
            ft, al = fs, torch.full((1, H, D), 1.0 / D)
        c = dict(x=ft, al=al, er=er, tab=tab, slope=slope)
    elif kind == "gatv2":
        fs, fd, att, tab, _ft, _gy, slope = R.gatv2_inputs(base, N, H, D, n_rel, seed)
        c = dict(x=fs, xd=fd, att=att, tab=tab, slope=slope)
    else:
        raise ValueError(kind)
    if recipe == "deep":
        key = "xd" if kind == "gatv2" else "er"
        c[key] = c[key].clone()
        c[key][::3] -= DEEP_SHIFT
    return c


def scores(kind, c, ptr, idx, rel, dtype=torch.float64):
    """s [E, H] of a case in dtype, CSR order, and (src, dst, n_dst)"""
    src, dst, n_dst = R._edges(ptr, idx)
    t = {k: v.to(dtype) for k, v in c.items() if torch.is_tensor(v)}
    if kind == "gatv2":
        s = (F.leaky_relu(t["x"][src] + t["xd"][dst], c["slope"]) * t["att"]).sum(-1)
        s = s + t["tab"][rel.long()]
    else:
        el = t["el"] if kind == "gat_el" else (t["x"] * t["al"]).sum(-1)
        s = F.leaky_relu(el[src] + t["er"][dst] + t["tab"][rel.long()], c["slope"])
    return s, (src, dst, n_dst)


def operator_reference(kind, c, ptr, idx, rel, dtype=torch.float64, eps=1e-16, gmax=None):
    """(out [n_dst, H, D], scale, eps share [n_dst, H]) of the ogbn-mag softmax + aggregation in
    dtype, through _attention_ref's restatements; gmax: another maximum than the case's own"""
    t = {k: v.to(dtype) for k, v in c.items() if torch.is_tensor(v)}
    if kind == "gatv2":
        out = R.gatv2_reference(ptr, idx, rel, t["x"], t["xd"], t["att"], t["tab"], t["x"],
                                c["slope"], global_max=True)
        a = R.gatv2_attention_ref(ptr, idx, rel, t["x"], t["xd"], t["att"], t["tab"], c["slope"],
                                  global_max=True)
    else:
        el = t["el"] if kind == "gat_el" else (t["x"] * t["al"]).sum(-1)
        out = R.gat_reference(ptr, idx, rel, el, t["er"], t["tab"], t["x"], c["slope"],
                              global_max=True)
        a = R.gat_attention_ref(ptr, idx, rel, el, t["er"], t["tab"], c["slope"],
                                global_max=True)
    src, dst, n_dst = R._edges(ptr, idx)
    scale = R._aggregate(a, t["x"].abs(), src, dst, n_dst)
    s, _ = scores(kind, c, ptr, idx, rel, dtype)
    H = s.shape[1]
    den = torch.zeros(n_dst, H, dtype=dtype).index_add(0, dst, torch.exp(s - s.max()))
    share = eps / (den + eps)
    share[den == 0] = 0.0                               # rows without entries
    return out, scale, share


def online_reference(kind, c, ptr, idx, rel, dtype=torch.float64, eps=1e-16, correct=True):
    """the same quantity in the kernels' form: per-row maximum m, S = sum exp(s - m),
    acc = sum exp(s - m) x, gmax = max m, out = acc / (S + eps exp(gmax - m)).
    correct=False drops the eps term (what a plain per-row softmax would return)."""
    s, (src, dst, n_dst) = scores(kind, c, ptr, idx, rel, dtype)
    H = s.shape[1]
    x = c["x"].to(dtype)
    m = torch.full((n_dst, H), -torch.inf, dtype=dtype)
    m = m.scatter_reduce(0, dst[:, None].expand(-1, H), s, reduce="amax", include_self=True)
    ex = torch.exp(s - m[dst])
    S = torch.zeros(n_dst, H, dtype=dtype).index_add(0, dst, ex)
    acc = torch.zeros(n_dst, H, x.shape[2], dtype=dtype).index_add(0, dst, ex[:, :, None] * x[src])
    gmax = m.max()
    den = S + (eps * torch.exp(gmax - m) if correct else 0.0)
    out = acc / den[:, :, None]
    out[(S == 0)[:, :, None].expand_as(out)] = 0.0
    return out


# ---- the layers and the model ------------------------------------------------------------------
def conv_restated(P, meta, ptr, idx, rel, x, n_dst, v2):
    """mag REGATConv / REGATv2Conv over a CSR whose rows are the first n_dst sources
    (mag/regnn_layers.py:253-325, 394-436): P = the conv's parameters by name, in x's dtype."""
    H, C = meta["heads"], meta["out_channels"]
    xs = (x @ P["lin_src.weight"].t()).view(-1, H, C)
    xd = xs[:n_dst]                                            # lin_dst is lin_src
    tab = F.leaky_relu(P["relation_weight"] * meta["scaling_factor"])
    if v2:
        out = R.gatv2_reference(ptr, idx, rel, xs, xd, P["att"], tab, xs, meta["negative_slope"],
                                global_max=True)
    else:
        a_s = (xs * P["att_src"]).sum(-1)
        a_d = (xd * P["att_dst"]).sum(-1)
        out = R.gat_reference(ptr, idx, rel, a_s, a_d, tab, xs, meta["negative_slope"],
                              global_max=True)
    out = out.reshape(-1, H * C) + P["bias"]
    if meta["residual"]:
        out = out + xd.reshape(-1, H * C)
    if meta["use_norm"] == "ln":
        out = F.layer_norm(out, (H * C,), P["norm.weight"], P["norm.bias"])
    return out


def full_csr_with_loops(rg, edge_type, node_type, num_edge_types):
    """(ptr, idx, rel) CPU tensors of the whole graph with every node's self loop (relation
    num_edge_types + node type), as the full-neighbour inference reads it"""
    N = rg.n_dst
    ptr = rg.csr_ptr.cpu().numpy().astype(np.int64)
    src = rg.csr_idx.cpu().numpy().astype(np.int64)
    dst = np.repeat(np.arange(N), np.diff(ptr))
    et = edge_type.cpu().numpy()[rg.csr_eid.cpu().numpy()]
    loop = np.arange(N)
    p, i, r = csr_of(np.concatenate([src, loop]), np.concatenate([dst, loop]),
                     np.concatenate([et, node_type.cpu().numpy() + num_edge_types]), N)
    return torch.from_numpy(p), torch.from_numpy(i), torch.from_numpy(r)


def model_restated(model, csr, node_type, local, x_dict, dtype=torch.float64):
    """logits [N, classes] of mag.REGNN's layer-wise inference ('regat' / 'regatv2', feats_type
    != 2) restated on the CPU in dtype"""
    P = {n: p.detach().cpu().to(dtype) for n, p in model.named_parameters()}
    nt, loc = node_type.cpu(), local.cpu()
    N = nt.numel()
    x = torch.zeros(N, model.hidden_dim, dtype=dtype)
    for k, xf in x_dict.items():
        m = nt == k
        x[m] = xf.cpu().to(dtype)[loc[m]] @ P[f"lins.{k}.weight"].t() + P[f"lins.{k}.bias"]
    ptr, idx, rel = csr
    for i, conv in enumerate(model.convs):
        pc = {k[len(f"convs.{i}."):]: v for k, v in P.items() if k.startswith(f"convs.{i}.")}
        meta = dict(heads=conv.heads, out_channels=conv.out_channels,
                    scaling_factor=conv.scaling_factor, negative_slope=conv.negative_slope,
                    residual=conv.residual, use_norm=conv.use_norm)
        x = F.relu(conv_restated(pc, meta, ptr, idx, rel, x, N, conv.v2))
    return x @ P["out_lin.weight"].t() + P["out_lin.bias"]
