"""fp64 references of the GAT / GATv2 attention kernels (re_gat.hip, re_gatv2.hip) with a
per-element error scale, the input recipes and the ladder graph of the attention parity tests
(test_cpu_attention_ref.py, test_gpu_gat_fused.py, test_gpu_attention_matrix.py) and the table of
the matrix's shapes. A plain helper: no test lives here.

The restatements are torch code with autograd over the CSR edge list (ptr, idx, rel_csr):
  gat_reference    layer/REGATConv.py:80-92     (global_max: the softmax of mag/utils.py:45-57)
  gatv2_reference  layer/REGATv2Conv.py:139-163 (likewise)
They run in whatever dtype their inputs have: fp64 is the reference, fp32 the yardstick of what
the arithmetic alone costs (test_cpu_attention_ref.py).

The error of a tensor is  max |got - ref| / (scale + 2^-100)  elementwise, where `scale` is the
same reduction as the tensor's with every product replaced by its absolute value, down to the
per-edge level (a = the attention, x = ft, gy = the incoming gradient, T_e = sum_d |gy_v x_u|):
  out[v,h,:]   sum_e a_e |x_u|                   g_ft[u,h,:]   sum_e a_e |gy_v|
  gs[e,h]      a_e (T_e + sum_e' a_e' T_e')      (d loss / d logit of edge e)
  g_el / g_er / g_tab                            the source / destination / relation sums of gs
  g_att[h,d]   sum_e gs_e |LeakyReLU(fs_u + fd_v)|
  g_fs / g_fd  the source / destination sums of gs_e |att| LeakyReLU'(fs_u + fd_v)
  g_al, g_ar   sum_n g_el[n,h] |ft[n,h,:]| (g_er likewise); g_ft gains g_el |al| + g_er |ar|
so an error confined to a short row is measured against that row's own magnitude and not against
a hub row's. The floor 2^-100 absorbs the fp32 underflow of attention weights below 1e-38; a
tensor element whose scale is 0 (a row without edges) must be exactly 0."""
import numpy as np
import torch
import torch.nn.functional as F

FLOOR = 2.0 ** -100
TOL_F32 = 1e-5                 # the kernels' bound under the metric above
TOL_GUARD = 2.5e-6             # fp32 torch run of the restatement: a quarter of it
BF16_REL = 2.0 ** -8           # round-to-nearest-even of a bf16 store, x2 for ties


# ---- edge list ---------------------------------------------------------------------------------
def _edges(ptr, idx):
    ptr = ptr.long()
    n_dst = ptr.numel() - 1
    dst = torch.repeat_interleave(torch.arange(n_dst, device=ptr.device), ptr[1:] - ptr[:-1])
    return idx.long(), dst, n_dst


def _softmax(s, dst, n_dst, global_max):
    """global_max == "detached": the one maximum as a constant. Its own gradient is
    -a * 1e-16 / (den + 1e-16) per edge, which the kernels' backward drops as documented
    (ops.gat_attention); autograd sums it over EVERY edge onto the one arg-max logit, in fp32
    a sum of E * H rounding errors on a single element (the fp32 yardstick's, not the inputs')."""
    H = s.shape[1]
    if global_max:
        ex = torch.exp(s - (s.max().detach() if global_max == "detached" else s.max()))
        den = torch.zeros(n_dst, H, dtype=s.dtype, device=s.device).index_add(0, dst, ex)
        return ex / (den[dst] + 1e-16)
    m = torch.full((n_dst, H), -torch.inf, dtype=s.dtype, device=s.device)
    m = m.scatter_reduce(0, dst[:, None].expand(-1, H), s, reduce="amax", include_self=True)
    ex = torch.exp(s - m[dst])
    den = torch.zeros(n_dst, H, dtype=s.dtype, device=s.device).index_add(0, dst, ex)
    return ex / den[dst]


def _aggregate(a, ft, src, dst, n_dst):
    out = torch.zeros(n_dst, a.shape[1], ft.shape[2], dtype=a.dtype, device=a.device)
    return out.index_add(0, dst, a[:, :, None] * ft[src])


def gat_attention_ref(ptr, idx, rel_csr, el, er, tab, slope, global_max=False):
    """a[e,h] of layer/REGATConv.py:80-88 in CSR edge order."""
    src, dst, n_dst = _edges(ptr, idx)
    s = el[src] + er[dst] + (tab[rel_csr.long()] if tab is not None else 0.0)
    return _softmax(F.leaky_relu(s, slope), dst, n_dst, global_max)


def gat_reference(ptr, idx, rel_csr, el, er, tab, ft, slope, global_max=False):
    """torch restatement of layer/REGATConv.py:80-92 over the CSR edge list."""
    src, dst, n_dst = _edges(ptr, idx)
    a = gat_attention_ref(ptr, idx, rel_csr, el, er, tab, slope, global_max)
    return _aggregate(a, ft, src, dst, n_dst)


def gatv2_attention_ref(ptr, idx, rel_csr, fs, fd, att, tab, slope, global_max=False):
    src, dst, n_dst = _edges(ptr, idx)
    e = F.leaky_relu(fs[src] + fd[dst], slope)                               # [E, H, D]
    s = (e * att).sum(-1)
    if tab is not None:
        s = s + tab[rel_csr.long()]
    return _softmax(s, dst, n_dst, global_max)


def gatv2_reference(ptr, idx, rel_csr, fs, fd, att, tab, ft, slope, global_max=False):
    """torch restatement of layer/REGATv2Conv.py:139-163 (GATv2 score, relation bias,
    per-destination softmax; global_max: mag/utils.py:45-57) and the per-head aggregation."""
    src, dst, n_dst = _edges(ptr, idx)
    a = gatv2_attention_ref(ptr, idx, rel_csr, fs, fd, att, tab, slope, global_max)
    return _aggregate(a, ft, src, dst, n_dst)


# ---- scales ------------------------------------------------------------------------------------
def _attention_scales(a, ft, gy, src, dst, n_dst, n_src, rel, n_rel):
    """scales of out, g_ft and the per-edge gs, and gs's source / destination / relation sums"""
    H = a.shape[1]
    z = lambda *s: torch.zeros(*s, dtype=a.dtype, device=a.device)   # noqa: E731
    x, g = ft[src], gy[dst]
    sc = {"out": z(n_dst, H, ft.shape[2]).index_add(0, dst, a[:, :, None] * x.abs()),
          "g_ft": z(n_src, H, ft.shape[2]).index_add(0, src, a[:, :, None] * g.abs())}
    T = (g * x).abs().sum(-1)
    gs = a * (T + z(n_dst, H).index_add(0, dst, a * T)[dst])
    sc["gs"] = gs
    sc["g_src"] = z(n_src, H).index_add(0, src, gs)
    sc["g_dst"] = z(n_dst, H).index_add(0, dst, gs)
    if rel is not None:
        assert rel.numel() == 0 or int(rel.max()) < n_rel
        sc["g_tab"] = z(n_rel, H).index_add(0, rel.long(), gs)
    return sc


def _leaves(ts):
    return [None if t is None else t.detach().double().clone().requires_grad_(True) for t in ts]


def gat_case_ref(ptr, idx, rel_csr, el, er, tab, ft, gy, slope, global_max=False, n_src=None):
    """fp64 reference and scale of every output of the GAT kinds (el given):
    dicts over out, g_ft, g_el, g_er[, g_tab]."""
    el, er, tab, ft = _leaves([el, er, tab, ft])
    gy = gy.detach().double()
    out = gat_reference(ptr, idx, rel_csr, el, er, tab, ft, slope, global_max)
    out.backward(gy)
    want = {"out": out.detach(), "g_ft": ft.grad, "g_el": el.grad, "g_er": er.grad}
    src, dst, n_dst = _edges(ptr, idx)
    with torch.no_grad():
        a = gat_attention_ref(ptr, idx, rel_csr, el, er, tab, slope, global_max)
        s = _attention_scales(a, ft, gy, src, dst, n_dst, ft.shape[0],
                              *((None, 0) if tab is None else (rel_csr, tab.shape[0])))
    scale = {"out": s["out"], "g_ft": s["g_ft"], "g_el": s["g_src"], "g_er": s["g_dst"]}
    if tab is not None:
        want["g_tab"], scale["g_tab"] = tab.grad, s["g_tab"]
    return want, scale


def gat_attn_case_ref(ptr, idx, rel_csr, al, ar, tab, ft, gy, slope):
    """the same with el / er = the dots of ft with attn_l / attn_r (layer/REGATConv.py:68-69):
    out, g_ft, g_al, g_ar[, g_tab]."""
    al, ar, tab, ft = _leaves([al, ar, tab, ft])
    gy = gy.detach().double()
    el, er = (ft * al).sum(-1), (ft * ar).sum(-1)
    out = gat_reference(ptr, idx, rel_csr, el, er, tab, ft, slope)
    out.backward(gy)
    want = {"out": out.detach(), "g_ft": ft.grad, "g_al": al.grad, "g_ar": ar.grad}
    src, dst, n_dst = _edges(ptr, idx)
    with torch.no_grad():
        a = gat_attention_ref(ptr, idx, rel_csr, el, er, tab, slope)
        s = _attention_scales(a, ft, gy, src, dst, n_dst, ft.shape[0],
                              *((None, 0) if tab is None else (rel_csr, tab.shape[0])))
        gel, ger = s["g_src"][:, :, None], s["g_dst"][:, :, None]
        scale = {"out": s["out"], "g_ft": s["g_ft"] + gel * al.abs() + ger * ar.abs(),
                 "g_al": (gel * ft.abs()).sum(0, keepdim=True),
                 "g_ar": (ger * ft.abs()).sum(0, keepdim=True)}
    if tab is not None:
        want["g_tab"], scale["g_tab"] = tab.grad, s["g_tab"]
    return want, scale


def gatv2_case_ref(ptr, idx, rel_csr, fs, fd, att, tab, ft, gy, slope, global_max=False):
    """fp64 reference and scale of the GATv2 kinds: out, g_fs, g_fd, g_att, g_ft[, g_tab]."""
    fs, fd, att, tab, ft = _leaves([fs, fd, att, tab, ft])
    gy = gy.detach().double()
    out = gatv2_reference(ptr, idx, rel_csr, fs, fd, att, tab, ft, slope, global_max)
    out.backward(gy)
    want = {"out": out.detach(), "g_fs": fs.grad, "g_fd": fd.grad, "g_att": att.grad,
            "g_ft": ft.grad}
    src, dst, n_dst = _edges(ptr, idx)
    with torch.no_grad():
        a = gatv2_attention_ref(ptr, idx, rel_csr, fs, fd, att, tab, slope, global_max)
        s = _attention_scales(a, ft, gy, src, dst, n_dst, ft.shape[0],
                              *((None, 0) if tab is None else (rel_csr, tab.shape[0])))
        pre = fs[src] + fd[dst]
        gs = s["gs"][:, :, None]
        through = gs * att.abs() * torch.where(pre > 0, 1.0, slope)
        scale = {"out": s["out"], "g_ft": s["g_ft"],
                 "g_att": (gs * F.leaky_relu(pre, slope).abs()).sum(0, keepdim=True),
                 "g_fs": torch.zeros_like(fs).index_add(0, src, through),
                 "g_fd": torch.zeros_like(fd).index_add(0, dst, through)}
    if tab is not None:
        want["g_tab"], scale["g_tab"] = tab.grad, s["g_tab"]
    return want, scale


def gatv2_shared_case_ref(ptr, idx, rel_csr, x, att, tab, gy, slope, global_max=False):
    """the GATv2 kinds with fs, fd and ft ONE leaf x (layer/REGATv2Conv.py share_weights=True on
    a graph whose sources are its destinations): out, g_x, g_att[, g_tab]. g_x is the sum of the
    three partial gradients, so its scale is the sum of their scales."""
    x, att, tab = _leaves([x, att, tab])
    gy = gy.detach().double()
    out = gatv2_reference(ptr, idx, rel_csr, x, x, att, tab, x, slope, global_max)
    out.backward(gy)
    want = {"out": out.detach(), "g_x": x.grad, "g_att": att.grad}
    _, part = gatv2_case_ref(ptr, idx, rel_csr, x, x, att, tab, x, gy, slope, global_max)
    scale = {"out": part["out"], "g_x": part["g_fs"] + part["g_fd"] + part["g_ft"],
             "g_att": part["g_att"]}
    if tab is not None:
        want["g_tab"], scale["g_tab"] = tab.grad, part["g_tab"]
    return want, scale


def gatv2_score_ref(ptr, idx, fs, fd, att, slope):
    """s[e,h] = <att[h], LeakyReLU(fs[u,h] + fd[v,h])> in CSR edge order, in the inputs' dtype"""
    src, dst, _ = _edges(ptr, idx)
    return (F.leaky_relu(fs[src] + fd[dst], slope) * att).sum(-1)


def gatv2_score_case_ref(ptr, idx, fs, fd, att, gs, slope):
    """fp64 reference and scale of the score operator alone (loss = sum gs * s): s, g_fs, g_fd,
    g_att. s[e,h] is measured against sum_d |att LeakyReLU(fs_u + fd_v)|, the gradients against
    the sums of |gs| |att| LeakyReLU' and |gs| |LeakyReLU|."""
    fs, fd, att = _leaves([fs, fd, att])
    gs = gs.detach().double()
    s = gatv2_score_ref(ptr, idx, fs, fd, att, slope)
    s.backward(gs)
    want = {"s": s.detach(), "g_fs": fs.grad, "g_fd": fd.grad, "g_att": att.grad}
    src, dst, _ = _edges(ptr, idx)
    with torch.no_grad():
        pre = fs[src] + fd[dst]
        act = F.leaky_relu(pre, slope).abs()
        through = gs.abs()[:, :, None] * att.abs() * torch.where(pre > 0, 1.0, slope)
        scale = {"s": (act * att.abs()).sum(-1),
                 "g_fs": torch.zeros_like(fs).index_add(0, src, through),
                 "g_fd": torch.zeros_like(fd).index_add(0, dst, through),
                 "g_att": (gs.abs()[:, :, None] * act).sum(0, keepdim=True)}
    return want, scale


# ---- the metric --------------------------------------------------------------------------------
def rel_err(got, ref, scale, bf16_store=False):
    """max |got - ref| / (scale + 2^-100); bf16_store: |got - ref| less the rounding of a bf16
    store, 2^-8 |ref|. NaN / inf in got fails."""
    got = got.detach().double()
    assert got.shape == ref.shape == scale.shape, (got.shape, ref.shape, scale.shape)
    assert bool(torch.isfinite(got).all()), "NaN / inf in a kernel output"
    if got.numel() == 0:
        return 0.0
    err = (got - ref).abs()
    if bf16_store:
        err = (err - BF16_REL * ref.abs()).clamp(min=0.0)
    return float((err / (scale + FLOOR)).max().item())


# ---- input recipes -----------------------------------------------------------------------------
def _grid(x, bits, lim):
    return (x.clamp(-lim, lim) * 2.0 ** bits).round() / 2.0 ** bits


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def gat_inputs(recipe, N, H, D, n_rel, seed, bf16=False):
    """fp32 CPU tensors (ft, el, er, tab, gy, slope) of the GAT kinds with el given.
    unit: randn (tab * 0.5), slope 0.2; bf16: ft and gy bf16-representable.
    wide: el, er, tab multiples of 2^-8 with |el| <= 2, |er|, |tab| <= 1, per-source offsets in
    {-8, 0, 8} on el and per-destination offsets in {-4, 0, 4} on er, slope 0.25: every score,
    maximum and difference is exact in fp32, |score| <= 16 and the online-softmax rescale factors
    reach e^+-20."""
    g = torch.Generator().manual_seed(seed)
    ft, gy = _randn(g, N, H, D), _randn(g, N, H, D)
    el, er, tab = _randn(g, N, H), _randn(g, N, H), _randn(g, n_rel, H) * 0.5
    slope = 0.2
    if recipe == "wide":
        so = torch.randint(-1, 2, (N, 1), generator=g).float() * 8.0
        do = torch.randint(-1, 2, (N, 1), generator=g).float() * 4.0
        el, er, tab = _grid(el, 8, 2.0) + so, _grid(er * 0.5, 8, 1.0) + do, _grid(tab, 8, 1.0)
        slope = 0.25
    elif recipe != "unit":
        raise ValueError(recipe)
    if bf16:
        ft, gy = ft.bfloat16().float(), gy.bfloat16().float()
    return ft, el, er, tab, gy, slope


def gat_attn_inputs(N, H, D, n_rel, seed):
    """(ft, attn_l, attn_r, tab, gy, slope) of the attn_l kind: attn_* randn / sqrt(D), so el and
    er are O(1) at every D and their own fp32 rounding stays far inside the bound."""
    g = torch.Generator().manual_seed(seed)
    ft, gy = _randn(g, N, H, D), _randn(g, N, H, D)
    al, ar = _randn(g, 1, H, D) / D ** 0.5, _randn(g, 1, H, D) / D ** 0.5
    return ft, al, ar, _randn(g, n_rel, H) * 0.5, gy, 0.2


def gatv2_inputs(recipe, N, H, D, n_rel, seed):
    """(fs, fd, att, tab, ft, gy, slope) of the GATv2 kinds.
    unit: fs, fd randn * 0.5, att randn / sqrt(D) (scores O(1) at every D), tab randn * 0.5.
    wide: fs, fd multiples of 2^-4 in [-1, 1] plus per-source offsets in {-8, 0, 8} and
    per-destination offsets in {-4, 0, 4}, att = 1 / D with one entry per head negated, tab
    multiples of 2^-8 in [-1, 1], slope 0.25: every term of a score is a multiple of 2^-12 and
    every partial sum below 2^4, so the scores are exact in fp32 in any summation order and lie
    in about [-4, 15], as GAT's wide scores do. (Scores further below the one global maximum
    would make the 1e-16 of the global-max softmax visible: at exp(-30) its share of the
    denominator, which the kernels' backward drops as documented, is 1e-3.)"""
    g = torch.Generator().manual_seed(seed)
    ft, gy = _randn(g, N, H, D), _randn(g, N, H, D)
    fs, fd = _randn(g, N, H, D) * 0.5, _randn(g, N, H, D) * 0.5
    att, tab = _randn(g, 1, H, D) / D ** 0.5, _randn(g, n_rel, H) * 0.5
    slope = 0.2
    if recipe == "wide":
        assert D & (D - 1) == 0 and D <= 64
        so = torch.randint(-1, 2, (N, 1, 1), generator=g).float() * 8.0
        do = torch.randint(-1, 2, (N, 1, 1), generator=g).float() * 4.0
        fs, fd = _grid(fs, 4, 1.0) + so, _grid(fd, 4, 1.0) + do
        att = torch.full((1, H, D), 1.0 / D)
        att[0, torch.arange(H), torch.arange(H) % D] *= -1.0
        tab = _grid(tab, 8, 1.0)
        slope = 0.25
    elif recipe != "unit":
        raise ValueError(recipe)
    return fs, fd, att, tab, ft, gy, slope


def gatv2_shared_inputs(N, H, D, n_rel, seed):
    """(x, att, tab, gy, slope) of the shared-leaf GATv2 case: gatv2_inputs' `unit` tensors with
    x = its fs (randn * 0.5: x + x keeps the scores O(1))."""
    fs, _, att, tab, _, gy, slope = gatv2_inputs("unit", N, H, D, n_rel, seed)
    return fs, att, tab, gy, slope


def score_grad(E, H, seed):
    """gs [E, H], the incoming gradient of the score operator's own case"""
    return _randn(torch.Generator().manual_seed(seed + 77), E, H)


# ---- the shapes of the parity matrix (test_cpu_attention_ref.py guards every one of them,
# test_gpu_attention_matrix.py / test_gpu_gat_fused.py run them) ---------------------------------
# every fp32 (H, D): one or two per dispatch tier, H = 16 / 32, generic head counts
SHAPES = [(1, 4), (4, 16), (8, 16), (1, 128), (16, 16), (32, 8), (8, 64), (2, 256), (16, 64),
          (32, 64), (3, 4), (6, 8), (12, 16), (64, 4)]
WIDE = [(4, 16), (32, 8), (3, 4)]                     # shapes that also run the `wide` recipe
POW2_SHAPES = [(H, D) for H, D in SHAPES if H & (H - 1) == 0 and H <= 32]
V2_SHAPES = [(H, D) for H, D in POW2_SHAPES if H * D <= 1024]
# bf16 rows (8 elements per vector): the tiers (16,1) (16,1) (16,2) (16,4) (64,2) (64,4) (64,8)
BF16_SHAPES = [(1, 8), (8, 16), (16, 16), (8, 64), (16, 64), (32, 64), (32, 128)]
SHARED_SHAPES = [(4, 16), (8, 64)]                    # GATv2 with fs, fd, ft one leaf
# the direct per-edge checks, scale |reference|: the attention a of both recipes, the GATv2 score
# s of `wide` alone (exact in fp32). s of `unit` is a dot with cancellation: under |reference| its
# fp32 restatement is off by 3.7e-5 .. 1.5e-3 on these shapes, far past TOL_GUARD, so it is left
# out of that scale and runs under the scale of its terms instead (gatv2_score_case_ref).
DIRECT_SHAPES = [(1, 4), (8, 64), (32, 8)]
# the boundary shape the score operator takes on its own (H = 3: the edge softmax refuses it)
SCORE_SHAPES = DIRECT_SHAPES + [(3, 8)]


# ---- the ladder graph --------------------------------------------------------------------------
IN_DEGREES = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255,
              256, 257, 300]
OUT_DEGREES = [9, 17, 33, 65, 129, 257, 300, 8, 16, 64]
PLAN_FORMS = {"default": (256, 256),     # row 257: a 256-edge chunk and a one-edge chunk
              "tree": (8, 4),            # the 300-edge rows: 75 chunks > FANIN, two tree levels
              "noplan": (1 << 20, 256)}  # a split above every degree: no plan
N_REL = 7


def ladder_edges(N=320, seed=11):
    """(src, dst, rel) int64 arrays, deterministic. Nodes 0..24 are destinations with the
    in-degrees IN_DEGREES (their sources drawn from the plain nodes), nodes 25..34 sources with
    the out-degrees OUT_DEGREES into the plain nodes 35..N-1, and ~800 more edges run among the
    plain nodes (some of which keep in-degree 0). No self loops; duplicate edges occur; relation
    ids in [1, 7]."""
    nd, ns = len(IN_DEGREES), len(OUT_DEGREES)
    first = nd + ns
    assert N > first + 2
    rng = np.random.default_rng(seed)
    src, dst = [], []
    for v, k in enumerate(IN_DEGREES):
        src.append(rng.integers(first, N, k)); dst.append(np.full(k, v))
    for i, k in enumerate(OUT_DEGREES):
        src.append(np.full(k, nd + i)); dst.append(rng.integers(first, N, k))
    s = rng.integers(first, N, 800)
    d = rng.integers(first, N - 1, 800)
    d = np.where(d >= s, d + 1, d)                       # d != s, uniform over the others
    src.append(s); dst.append(d)
    src, dst = np.concatenate(src).astype(np.int64), np.concatenate(dst).astype(np.int64)
    perm = rng.permutation(src.size)                     # edge ids unrelated to the rows
    src, dst = src[perm], dst[perm]
    rel = rng.integers(1, N_REL + 1, src.size).astype(np.int64)
    assert not (src == dst).any()
    assert np.bincount(dst, minlength=N)[:nd].tolist() == IN_DEGREES
    assert np.bincount(src, minlength=N)[nd:first].tolist() == OUT_DEGREES
    return src, dst, rel


def ladder_graph(form="default", device="cpu", N=320):
    """(RelGraph, e_feat) of the ladder graph in one of PLAN_FORMS."""
    from regnn_hip.graph import RelGraph
    src, dst, rel = ladder_edges(N)
    split, chunk = PLAN_FORMS[form]
    rg = RelGraph(src, dst, N, device, split=split, chunk=chunk)
    for plan in (rg.csr_plan, rg.csc_plan):
        if form == "default":
            assert plan.n_long == 2 and plan.n_chunk == 4 and plan.n_levels == 1
        elif form == "tree":
            assert plan.n_levels >= 2, "raise the hub degree: the tree needs > FANIN chunks"
        else:
            assert plan.n_long == 0
    return rg, torch.from_numpy(rel).to(device)
