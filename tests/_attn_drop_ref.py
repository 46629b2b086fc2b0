"""fp64 restatement of the fused GAT attention dropout (regnn_gat_fused_fwd_drop /
regnn_spmm_heads_bwd_drop, ops.gat_fused(attn_drop=p)) on top of _attention_ref.py, which it
imports and does not change. A plain helper: no test lives here.

  out[v,h,:] = sum_{e: u->v} w[e,h] a[e,h] ft[u,h,:],   w = mask / keep,  keep = 1 - p
a = the UNDROPPED edge softmax of layer/REGATConv.py:80-88 (gat_attention_ref) and mask the
project's hash mask over (CSR edge position, head): oracle.regnn_oracle.dropout_mask(seed, E, Hq, 4,
keep16)[:, :H] with Hq = max(4, H rounded up to a multiple of 4). Gradients by autograd.

The error scales are _attention_scales' with the factor w carried wherever the reference carries
it (a = the attention, x = ft, gy = the incoming gradient):
  out[v,h,:]   sum_e w_e a_e |x_u|               g_ft[u,h,:]   sum_e w_e a_e |gy_v|
  T_e = w_e sum_d |gy_v x_u|,   gs[e,h] = a_e (T_e + sum_e' a_e' T_e')
  g_el / g_er / g_tab   the source / destination / relation sums of gs
An element whose scale is 0 (a row without in-edges, or one whose entries are all dropped in that
head) must be exactly 0: rel_err's floor of 2^-100 admits nothing else, and exact_zeros says so
outright."""
import torch

import _attention_ref as AR
from oracle import regnn_oracle as O

PS = (0.5, 0.2, 0.6)                     # p = 0.5: 8-bit draws; 0.2 and 0.6: 16-bit draws
# the seeds of the GPU parity tests, picked in test_cpu_attn_drop.py (input fairness)
SEEDS = {0.5: 0x1234_5678_9ABC_DEF1, 0.2: 0x0FED_CBA9_8765_4322, 0.6: 0x2468_ACE0_1357_9BDF}
SHAPES = [(1, 64), (2, 32), (4, 16), (8, 8), (8, 64), (32, 4)]


def keep16_of(p):
    return int(round((1.0 - float(p)) * 65536))


def head_cols(H):
    return max(4, (H + 3) // 4 * 4)


def attn_mask(seed, E, H, keep16):
    """0/1 keep mask [E, H] (float64) over (CSR edge position, head)"""
    m = O.dropout_mask(int(seed), int(E), head_cols(H), 4, int(keep16))
    return torch.from_numpy(m[:, :H].copy())


def drop_weight(seed, E, H, p):
    """w = mask / keep (float64); p = 0 would be the undropped operator and has no mask"""
    return attn_mask(seed, E, H, keep16_of(p)) / (1.0 - float(p))


def gat_drop_reference(ptr, idx, rel_csr, el, er, tab, ft, slope, w):
    """gat_reference with a * w ahead of the aggregation; runs in the dtype of its inputs"""
    src, dst, n_dst = AR._edges(ptr, idx)
    a = AR.gat_attention_ref(ptr, idx, rel_csr, el, er, tab, slope)
    return AR._aggregate(a * w.to(a.dtype).to(a.device), ft, src, dst, n_dst)


def _drop_scales(a, w, ft, gy, src, dst, n_dst, n_src, rel, n_rel):
    """_attention_scales with w carried: out / g_ft on a * w, T = w * sum_d |gy x|"""
    H = a.shape[1]
    z = lambda *s: torch.zeros(*s, dtype=a.dtype, device=a.device)   # noqa: E731
    x, g = ft[src], gy[dst]
    aw = a * w
    sc = {"out": z(n_dst, H, ft.shape[2]).index_add(0, dst, aw[:, :, None] * x.abs()),
          "g_ft": z(n_src, H, ft.shape[2]).index_add(0, src, aw[:, :, None] * g.abs())}
    T = w * (g * x).abs().sum(-1)
    gs = a * (T + z(n_dst, H).index_add(0, dst, a * T)[dst])
    sc["gs"] = gs
    sc["g_src"] = z(n_src, H).index_add(0, src, gs)
    sc["g_dst"] = z(n_dst, H).index_add(0, dst, gs)
    if rel is not None:
        assert rel.numel() == 0 or int(rel.max()) < n_rel
        sc["g_tab"] = z(n_rel, H).index_add(0, rel.long(), gs)
    return sc


def gat_drop_case_ref(ptr, idx, rel_csr, el, er, tab, ft, gy, slope, w):
    """fp64 reference and scale of out, g_ft, g_el, g_er[, g_tab] (el given)"""
    el, er, tab, ft = AR._leaves([el, er, tab, ft])
    gy, w = gy.detach().double(), w.double().to(ft.device)
    out = gat_drop_reference(ptr, idx, rel_csr, el, er, tab, ft, slope, w)
    out.backward(gy)
    want = {"out": out.detach(), "g_ft": ft.grad, "g_el": el.grad, "g_er": er.grad}
    src, dst, n_dst = AR._edges(ptr, idx)
    with torch.no_grad():
        a = AR.gat_attention_ref(ptr, idx, rel_csr, el, er, tab, slope)
        s = _drop_scales(a, w, ft, gy, src, dst, n_dst, ft.shape[0],
                         *((None, 0) if tab is None else (rel_csr, tab.shape[0])))
    scale = {"out": s["out"], "g_ft": s["g_ft"], "g_el": s["g_src"], "g_er": s["g_dst"]}
    if tab is not None:
        want["g_tab"], scale["g_tab"] = tab.grad, s["g_tab"]
    return want, scale


def exact_zeros(got, scale):
    """every element whose scale is 0 is exactly 0 (and there may be none)"""
    return bool((got.detach()[(scale == 0).to(got.device)] == 0).all())


def fairness(ptr, mask, p):
    """the three conditions on a mask [E, H] over the ladder graph's CSR (test_cpu_attn_drop.py):
    (a row of degree >= 2 fully dropped in some head, a row of degree >= 256 with kept and dropped
    entries in every head, |keep rate - keep16 / 65536| in sigmas)"""
    ptr = ptr.long().tolist()
    full = mixed = False
    for v in range(len(ptr) - 1):
        rows = mask[ptr[v]:ptr[v + 1]]
        if rows.shape[0] >= 2 and bool((rows.sum(0) == 0).any()):
            full = True
        if rows.shape[0] >= 256:
            k = rows.sum(0)
            mixed = mixed or bool(((k > 0) & (k < rows.shape[0])).all())
    q = keep16_of(p) / 65536.0
    sigma = (q * (1 - q) / mask.numel()) ** 0.5
    return full, mixed, abs(float(mask.mean()) - q) / sigma
