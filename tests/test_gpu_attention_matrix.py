"""The full-graph attention kernels (re_gat.hip, re_gat_fused.h, re_gatv2.hip) against the fp64
restatements of _attention_ref.py under its per-element metric, over every dispatch tier.

Graph: the ladder graph (N = 320, in-degrees 0 .. 300) in its three plan forms; the reference is
built once per case (the CSR is the same in every form), NaN-filled blocks of the outputs' sizes
go back to the allocator before each run, rows without in-edges must come out exactly 0.
Bound: AR.TOL_F32 = 1e-5 on every tensor (bf16-stored ones with bf16_store=True);
test_cpu_attention_ref.py shows that the restatement's own fp32 arithmetic costs at most a quarter
of it on every (recipe, shape, kind) used here. Each case prints its maxima (-s).

Shapes: AR.POW2_SHAPES, one or two per (lanes per row, vectors per lane) tier of REGNN_GATF /
REGNN_HEADS / REGNN_V2; each test asserts the tier its shape lands in from the tables below.
Kinds:
  a fused-el    ops.gat_fused, el given                       d unfused, global max
  b fused-elx   attn_l passed (ft as two leaves, and as one)  e GATv2 chain, both softmax forms,
  c unfused     head_spmm(gat_attention)                        and with fs, fd, ft one leaf
  f bf16 rows of a and c                                      g a and s directly, per edge
then the grid stride (N = 45000), bitwise repeats, and the shapes outside the tiers, which the
operators refuse with a ValueError before anything is launched."""
import pytest
import torch

import _attention_ref as AR
import _attn_drop_ref as DR

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 320

# ---- the dispatch tiers, spelled out: (lanes per row, vectors per lane), in dispatch order ----
TIERS = [(16, 1), (16, 2), (16, 4), (64, 2), (64, 4), (64, 8)]     # REGNN_GATF, REGNN_HEADS
V2_TIERS = TIERS[:5]                                               # REGNN_V2
# the tier every shape of the matrix lands in. The fused forward takes the first tier that holds
# the row's vectors; the per-head SpMM and the GATv2 scores also need a head's vectors inside one
# group of lanes, which moves (1, 128) from (16, 2) to (64, 2).
GATF_F32 = {(1, 4): (16, 1), (4, 16): (16, 1), (8, 16): (16, 2), (1, 128): (16, 2),
            (16, 16): (16, 4), (32, 8): (16, 4), (8, 64): (64, 2), (2, 256): (64, 2),
            (16, 64): (64, 4), (32, 64): (64, 8)}
HEADS_F32 = {**GATF_F32, (1, 128): (64, 2)}
V2_F32 = {k: v for k, v in HEADS_F32.items() if k != (32, 64)}
ROWS_BF16 = {(1, 8): (16, 1), (8, 16): (16, 1), (16, 16): (16, 2), (8, 64): (16, 4),
             (16, 64): (64, 2), (32, 64): (64, 4), (32, 128): (64, 8)}


def _tier(table, H, D, ev, head_in_group):
    nvec, vph = H * D // ev, D // ev
    for lpr, nv in table:
        if nvec <= lpr * nv and (vph <= lpr or not head_in_group):
            return lpr, nv
    return None


def _assert_tiers(H, D, gatf=None, heads=None, v2=None, ev=4):
    if gatf is not None:
        assert _tier(TIERS, H, D, ev, False) == gatf[(H, D)], "fused forward tier"
    if heads is not None:
        assert _tier(TIERS, H, D, ev, True) == heads[(H, D)], "per-head SpMM tier"
    if v2 is not None:
        assert _tier(V2_TIERS, H, D, 4, True) == v2[(H, D)], "GATv2 score tier"


def test_every_tier_has_a_case():
    assert sorted(GATF_F32) == sorted(AR.POW2_SHAPES) and sorted(V2_F32) == sorted(AR.V2_SHAPES)
    assert sorted(ROWS_BF16) == sorted(AR.BF16_SHAPES)
    for table in (GATF_F32, HEADS_F32, ROWS_BF16):
        assert set(table.values()) == set(TIERS)
    assert set(V2_F32.values()) == set(V2_TIERS)


# ---- graphs, inputs, runs ------------------------------------------------------------------------
def _forms(n):
    out = {}
    for form in AR.PLAN_FORMS:
        rg, e_feat = AR.ladder_graph(form, DEV, n)
        out[form] = (rg, rg.rel_pack(e_feat, num_rel=AR.N_REL))
    return out


@pytest.fixture(scope="module")
def graphs():
    return _forms(N)


def _dev(inp):
    return tuple(t.to(DEV) if torch.is_tensor(t) else t for t in inp)


def _seed(H, D):
    return 1000 * H + D


def _poison(rg, H, D):
    """NaN-filled blocks of the outputs' sizes go back to the allocator: a skipped store is likely
    to surface as NaN instead of a stale correct value"""
    n = rg.n_dst
    junk = [torch.full(sh, float("nan"), device=DEV) for sh in
            [(n, H, D)] * 3 + [(rg.E, H)] * 3 + [(n, H)] * 2]
    junk += [torch.full((n, H, D), float("nan"), device=DEV, dtype=torch.bfloat16)] * 2
    del junk


def _leaf(t, bf16=False):
    if t is None:
        return None
    return (t.bfloat16() if bf16 else t.clone()).requires_grad_(True)


def _no_tab(inp, at=3):
    return inp[:at] + (None,) + inp[at + 1:]


def _run_gat(kind, rg, pack, inp, bf16=False):
    """kinds a / c / d: (ft, el, er, tab, gy, slope) -> out, g_ft, g_el, g_er[, g_tab]"""
    from regnn_hip import ops
    ft0, el0, er0, tab0, gy, slope = inp
    _poison(rg, *ft0.shape[1:])
    ft, el, er, tab = _leaf(ft0, bf16), _leaf(el0), _leaf(er0), _leaf(tab0)
    pk = pack if tab is not None else None
    if kind == "fused":
        y = ops.gat_fused(rg, el, er, ft, tab, pk, slope)
    else:
        a = ops.gat_attention(rg, el, er, tab, pk, slope, global_max=kind == "gmax")
        y = ops.head_spmm(rg, a, ft)
    y.backward(gy.to(ft.dtype))
    got = {"out": y.detach(), "g_ft": ft.grad, "g_el": el.grad, "g_er": er.grad}
    if tab is not None:
        got["g_tab"] = tab.grad
    return got


def _run_elx(rg, pack, inp):
    """kind b, ft as two leaves of equal values (one under attn_dots, one under gat_fused): the
    tensors of kind a, and the fp32 (el, er) the reference then takes as its inputs"""
    from regnn_hip import ops
    ft0, al, ar, tab0, gy, slope = inp
    _poison(rg, *ft0.shape[1:])
    ft, tab = _leaf(ft0), _leaf(tab0)
    el, er = ops.attn_dots(ft0.clone().requires_grad_(True), al, ar)
    el.retain_grad(); er.retain_grad()
    y = ops.gat_fused(rg, el, er, ft, tab, pack if tab is not None else None, slope, attn_l=al)
    y.backward(gy)
    got = {"out": y.detach(), "g_ft": ft.grad, "g_el": el.grad, "g_er": er.grad}
    if tab is not None:
        got["g_tab"] = tab.grad
    return got, (el.detach(), er.detach())


def _run_attn(rg, pack, inp):
    """kind b, ft one leaf under attn_dots and gat_fused: out, g_ft, g_al, g_ar, g_tab"""
    from regnn_hip import ops
    ft0, al0, ar0, tab0, gy, slope = inp
    _poison(rg, *ft0.shape[1:])
    ft, al, ar, tab = _leaf(ft0), _leaf(al0), _leaf(ar0), _leaf(tab0)
    el, er = ops.attn_dots(ft, al, ar)
    y = ops.gat_fused(rg, el, er, ft, tab, pack, slope, attn_l=al)
    y.backward(gy)
    return {"out": y.detach(), "g_ft": ft.grad, "g_al": al.grad, "g_ar": ar.grad,
            "g_tab": tab.grad}


def _v2_chain(rg, pack, fs, fd, att, tab, ft, slope, global_max):
    from regnn_hip import ops
    s = ops.gatv2_scores(rg, fs, fd, att, slope)
    a = ops.edge_softmax_logits(rg, s, tab, pack if tab is not None else None, global_max)
    return ops.head_spmm(rg, a, ft)


def _run_v2(rg, pack, inp, global_max):
    """kind e: (fs, fd, att, tab, ft, gy, slope) -> out, g_fs, g_fd, g_att, g_ft[, g_tab]"""
    fs0, fd0, att0, tab0, ft0, gy, slope = inp
    _poison(rg, *ft0.shape[1:])
    fs, fd, att, tab, ft = (_leaf(t) for t in (fs0, fd0, att0, tab0, ft0))
    y = _v2_chain(rg, pack, fs, fd, att, tab, ft, slope, global_max)
    y.backward(gy)
    got = {"out": y.detach(), "g_fs": fs.grad, "g_fd": fd.grad, "g_att": att.grad,
           "g_ft": ft.grad}
    if tab is not None:
        got["g_tab"] = tab.grad
    return got


def _run_v2_shared(rg, pack, inp, global_max):
    """kind e with fs, fd and ft ONE leaf: (x, att, tab, gy, slope) -> out, g_x, g_att, g_tab"""
    x0, att0, tab0, gy, slope = inp
    _poison(rg, *x0.shape[1:])
    x, att, tab = _leaf(x0), _leaf(att0), _leaf(tab0)
    y = _v2_chain(rg, pack, x, x, att, tab, x, slope, global_max)
    y.backward(gy)
    return {"out": y.detach(), "g_x": x.grad, "g_att": att.grad, "g_tab": tab.grad}


def _compare(tag, got, want, scale, fails, worst, bf16=False):
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for name in sorted(want):
        stored = bf16 and name in ("out", "g_ft")
        if stored:
            assert got[name].dtype == torch.bfloat16
        err = AR.rel_err(got[name], want[name], scale[name], bf16_store=stored)
        worst[name] = max(worst.get(name, 0.0), err)
        if not err <= AR.TOL_F32:
            fails.append(f"{tag} {name}: err {err:.3e}")
        if not DR.exact_zeros(got[name], scale[name]):
            fails.append(f"{tag} {name}: non-zero where the scale is 0")


def _report(title, worst, fails):
    print(f"{title}: " + " ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())))
    assert not fails, "; ".join(fails)


def _recipes(H, D):
    return ("unit", "wide") if (H, D) in AR.WIDE else ("unit",)


def _gat_matrix(graphs, kind, H, D, bf16=False):
    fails, worst = [], {}
    for recipe in (("unit",) if bf16 else _recipes(H, D)):
        inp = _dev(AR.gat_inputs(recipe, N, H, D, AR.N_REL, _seed(H, D), bf16=bf16))
        for use_tab in (True, False):
            inp_t = inp if use_tab else _no_tab(inp)
            want = scale = None
            for form, (rg, pack) in graphs.items():
                got = _run_gat(kind, rg, pack, inp_t, bf16=bf16)
                if want is None:                      # the CSR is the same in every form
                    ft, el, er, tab, gy, slope = inp_t
                    want, scale = AR.gat_case_ref(rg.csr_ptr, rg.csr_idx, pack.rel_csr, el, er,
                                                  tab, ft, gy, slope, global_max=kind == "gmax")
                    assert bool((scale["out"] == 0).any())
                _compare(f"{recipe} tab={use_tab} {form}", got, want, scale, fails, worst, bf16)
    _report(f"attention matrix {kind}{' bf16' if bf16 else ''} H={H} D={D}", worst, fails)


# ---- a, c, d: el given ---------------------------------------------------------------------------
@pytest.mark.parametrize("H,D", AR.POW2_SHAPES)
def test_fused_el_vs_fp64(graphs, H, D):
    """a: ops.gat_fused with el given (gat_fused_fwd_kernel; backward gat_attn_lse,
    spmm_heads BWD, gat_softmax_bwd_group, segment_sum), with and without the relation table"""
    _assert_tiers(H, D, gatf=GATF_F32, heads=HEADS_F32)
    _gat_matrix(graphs, "fused", H, D)


@pytest.mark.parametrize("global_max", [False, True])
@pytest.mark.parametrize("H,D", AR.POW2_SHAPES)
def test_unfused_vs_fp64(graphs, H, D, global_max):
    """c / d: head_spmm(gat_attention) per destination (gat_softmax_fwd/bwd_group) and with the one
    global maximum (gat_scores + edge_softmax_fwd), whose own gradient the backward drops"""
    _assert_tiers(H, D, heads=HEADS_F32)
    _gat_matrix(graphs, "gmax" if global_max else "unfused", H, D)


# ---- b: attn_l passed ----------------------------------------------------------------------------
@pytest.mark.parametrize("H,D", AR.POW2_SHAPES)
def test_fused_elx_vs_fp64(graphs, H, D):
    """b: attn_l passed, so the forward re-forms el from the rows it gathers where D / 4 lanes fit
    its group; at (1, 128) on tier (16, 2) they do not and the launcher reads el. Two leaves for
    ft: the five tensors of kind a against the restatement on the fp32 el / er; one leaf: g_ft
    with the dots' share, g_al and g_ar against gat_attn_case_ref."""
    _assert_tiers(H, D, gatf=GATF_F32, heads=HEADS_F32)
    lpr = GATF_F32[(H, D)][0]
    assert (D // 4 > lpr) == ((H, D) == (1, 128)), "the one shape that falls back to reading el"
    inp = _dev(AR.gat_attn_inputs(N, H, D, AR.N_REL, _seed(H, D)))
    fails, worst = [], {}
    for use_tab in (True, False):
        inp_t = inp if use_tab else _no_tab(inp)
        want = scale = None
        for form, (rg, pack) in graphs.items():
            got, (el, er) = _run_elx(rg, pack, inp_t)
            if want is None:
                want, scale = AR.gat_case_ref(rg.csr_ptr, rg.csr_idx, pack.rel_csr, el, er,
                                              inp_t[3], inp_t[0], inp_t[4], inp_t[5])
            _compare(f"two leaves tab={use_tab} {form}", got, want, scale, fails, worst)
    want = scale = None
    for form, (rg, pack) in graphs.items():
        got = _run_attn(rg, pack, inp)
        if want is None:
            want, scale = AR.gat_attn_case_ref(rg.csr_ptr, rg.csr_idx, pack.rel_csr, inp[1],
                                               inp[2], inp[3], inp[0], inp[4], inp[5])
        _compare(f"one leaf {form}", got, want, scale, fails, worst)
    _report(f"attention matrix elx H={H} D={D}", worst, fails)


# ---- e: GATv2 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("global_max", [False, True])
@pytest.mark.parametrize("H,D", AR.V2_SHAPES)
def test_gatv2_vs_fp64(graphs, H, D, global_max):
    """e: gatv2_scores -> edge_softmax_logits -> head_spmm, the chain of layer/REGATv2Conv.py and
    mag.REGATv2Conv on full graphs. At (1, 128) the score launches size their grids for 16 lanes
    a row and run 64: the grid-stride loop has to reach every row."""
    _assert_tiers(H, D, heads=HEADS_F32, v2=V2_F32)
    fails, worst = [], {}
    for recipe in _recipes(H, D):
        inp = _dev(AR.gatv2_inputs(recipe, N, H, D, AR.N_REL, _seed(H, D)))
        for use_tab in (True, False):
            inp_t = inp if use_tab else _no_tab(inp)
            want = scale = None
            for form, (rg, pack) in graphs.items():
                got = _run_v2(rg, pack, inp_t, global_max)
                if want is None:
                    want, scale = AR.gatv2_case_ref(rg.csr_ptr, rg.csr_idx, pack.rel_csr,
                                                    *inp_t, global_max)
                    assert bool((scale["out"] == 0).any())
                _compare(f"{recipe} tab={use_tab} {form}", got, want, scale, fails, worst)
    _report(f"attention matrix gatv2 gmax={global_max} H={H} D={D}", worst, fails)


@pytest.mark.parametrize("global_max", [False, True])
@pytest.mark.parametrize("H,D", AR.SHARED_SHAPES)
def test_gatv2_shared_leaf_vs_fp64(graphs, H, D, global_max):
    """e with fs, fd and ft one leaf (the layer's share_weights=True): the three partial gradients
    accumulate into one tensor, measured against the sum of their scales"""
    _assert_tiers(H, D, heads=HEADS_F32, v2=V2_F32)
    inp = _dev(AR.gatv2_shared_inputs(N, H, D, AR.N_REL, _seed(H, D)))
    fails, worst = [], {}
    want = scale = None
    for form, (rg, pack) in graphs.items():
        got = _run_v2_shared(rg, pack, inp, global_max)
        if want is None:
            want, scale = AR.gatv2_shared_case_ref(rg.csr_ptr, rg.csr_idx, pack.rel_csr, *inp,
                                                   global_max)
        _compare(form, got, want, scale, fails, worst)
    _report(f"attention matrix gatv2 shared gmax={global_max} H={H} D={D}", worst, fails)


# ---- f: bf16 rows --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fused", "unfused"])
@pytest.mark.parametrize("H,D", AR.BF16_SHAPES)
def test_bf16_rows_vs_fp64(graphs, H, D, kind):
    """f: ft and gy in bf16 (8 elements a vector, so other tier boundaries); out and g_ft are
    stored in bf16, the other gradients in fp32"""
    _assert_tiers(H, D, gatf=ROWS_BF16 if kind == "fused" else None, heads=ROWS_BF16, ev=8)
    _gat_matrix(graphs, kind, H, D, bf16=True)


# ---- g: per edge ---------------------------------------------------------------------------------
@pytest.mark.parametrize("H,D", AR.DIRECT_SHAPES)
def test_attention_per_edge_vs_fp64(graphs, H, D):
    """g: the attention itself, |a - ref| <= 1e-5 |ref| per (edge, head): an error in a can partly
    cancel inside the aggregation. gat_attention and gatv2_scores -> edge_softmax_logits, both
    recipes, both softmax forms, with and without the table; the GATv2 score s under the same
    scale on `wide` only (there fp32 forms it exactly; `unit` is kept out, AR.DIRECT_SHAPES)."""
    from regnn_hip import ops
    f64 = lambda t: None if t is None else t.double()   # noqa: E731
    fails, worst = [], {}

    def check(tag, name, got, ref):
        err = AR.rel_err(got, ref, ref.abs())
        worst[name] = max(worst.get(name, 0.0), err)
        if not err <= AR.TOL_F32:
            fails.append(f"{tag} {name}: err {err:.3e}")

    rg0, pack0 = graphs["default"]
    ptr, idx, rel = rg0.csr_ptr, rg0.csr_idx, pack0.rel_csr
    for recipe in ("unit", "wide"):
        _, el, er, tab, _, slope = _dev(AR.gat_inputs(recipe, N, H, D, AR.N_REL, _seed(H, D)))
        fs, fd, att, tab2, _, _, slope2 = _dev(AR.gatv2_inputs(recipe, N, H, D, AR.N_REL,
                                                               _seed(H, D)))
        s_ref = AR.gatv2_score_ref(ptr, idx, fs.double(), fd.double(), att.double(), slope2)
        for global_max in (False, True):
            for t, t2 in ((tab, tab2), (None, None)):
                a_ref = AR.gat_attention_ref(ptr, idx, rel, el.double(), er.double(), f64(t),
                                             slope, global_max)
                a2_ref = AR.gatv2_attention_ref(ptr, idx, rel, fs.double(), fd.double(),
                                                att.double(), f64(t2), slope2, global_max)
                for form, (rg, pack) in graphs.items():
                    tag = f"{recipe} gmax={global_max} tab={t is not None} {form}"
                    pk = pack if t is not None else None
                    _poison(rg, H, D)
                    with torch.no_grad():
                        a = ops.gat_attention(rg, el, er, t, pk, slope, global_max=global_max)
                        s = ops.gatv2_scores(rg, fs, fd, att, slope2)
                        a2 = ops.edge_softmax_logits(rg, s, t2, pk, global_max)
                    check(tag, "gat_a", a, a_ref)
                    check(tag, "gatv2_a", a2, a2_ref)
                    if recipe == "wide":
                        check(tag, "gatv2_s", s, s_ref)
    _report(f"attention per edge H={H} D={D}", worst, fails)


@pytest.mark.parametrize("H,D", AR.SCORE_SHAPES)
def test_gatv2_scores_alone_vs_fp64(graphs, H, D):
    """the score operator on its own (`unit`): s and its three gradients, each under the scale of
    its terms. (3, 8) is a head count the score kernels take although the edge softmax, and with
    it the GATv2 chain, refuses it."""
    from regnn_hip import ops
    fs0, fd0, att0, _, _, _, slope = _dev(AR.gatv2_inputs("unit", N, H, D, AR.N_REL, _seed(H, D)))
    fails, worst = [], {}
    want = scale = None
    for form, (rg, _) in graphs.items():
        gs = AR.score_grad(rg.E, H, _seed(H, D)).to(DEV)
        _poison(rg, H, D)
        fs, fd, att = _leaf(fs0), _leaf(fd0), _leaf(att0)
        s = ops.gatv2_scores(rg, fs, fd, att, slope)
        s.backward(gs)
        got = {"s": s.detach(), "g_fs": fs.grad, "g_fd": fd.grad, "g_att": att.grad}
        if want is None:
            want, scale = AR.gatv2_score_case_ref(rg.csr_ptr, rg.csr_idx, fs0, fd0, att0, gs,
                                                  slope)
        _compare(form, got, want, scale, fails, worst)
    _report(f"gatv2 scores alone H={H} D={D}", worst, fails)


# ---- the grid stride -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["unfused", "gatv2"])
def test_grid_stride_vs_fp64(kind):
    """c and e at (4, 16) on a ladder graph with more rows than the capped grids hold groups: the
    16-lane score and SpMM kernels, the 32-lane softmax kernels and the segment sum all stride"""
    from regnn_hip import _lib as L
    H, D, n = 4, 16, 45000
    k_max_grid = L.slab_rows() // 2
    assert n > k_max_grid * 16
    big = _forms(n)
    fails, worst = [], {}
    want = scale = None
    if kind == "unfused":
        inp = _dev(AR.gat_inputs("unit", n, H, D, AR.N_REL, _seed(H, D)))
    else:
        inp = _dev(AR.gatv2_inputs("unit", n, H, D, AR.N_REL, _seed(H, D)))
    for form, (rg, pack) in big.items():
        if kind == "unfused":
            got = _run_gat("unfused", rg, pack, inp)
            if want is None:
                ft, el, er, tab, gy, slope = inp
                want, scale = AR.gat_case_ref(rg.csr_ptr, rg.csr_idx, pack.rel_csr, el, er, tab,
                                              ft, gy, slope)
        else:
            got = _run_v2(rg, pack, inp, False)
            if want is None:
                want, scale = AR.gatv2_case_ref(rg.csr_ptr, rg.csr_idx, pack.rel_csr, *inp)
        _compare(form, got, want, scale, fails, worst)
    _report(f"attention grid stride {kind} N={n}", worst, fails)


# ---- bitwise repeats -----------------------------------------------------------------------------
def _repeat_runs(H, D):
    gat = lambda bf16=False: _dev(AR.gat_inputs("unit", N, H, D, AR.N_REL, _seed(H, D),   # noqa
                                                bf16=bf16))
    elx = lambda: _dev(AR.gat_attn_inputs(N, H, D, AR.N_REL, _seed(H, D)))               # noqa
    v2 = lambda: _dev(AR.gatv2_inputs("unit", N, H, D, AR.N_REL, _seed(H, D)))           # noqa
    sh = lambda: _dev(AR.gatv2_shared_inputs(N, H, D, AR.N_REL, _seed(H, D)))            # noqa
    return {
        "fused-el": (gat, lambda rg, pk, i: _run_gat("fused", rg, pk, i)),
        "fused-elx": (elx, lambda rg, pk, i: _run_elx(rg, pk, i)[0]),
        "fused-elx one leaf": (elx, _run_attn),
        "unfused": (gat, lambda rg, pk, i: _run_gat("unfused", rg, pk, i)),
        "unfused gmax": (gat, lambda rg, pk, i: _run_gat("gmax", rg, pk, i)),
        "gatv2": (v2, lambda rg, pk, i: _run_v2(rg, pk, i, False)),
        "gatv2 gmax": (v2, lambda rg, pk, i: _run_v2(rg, pk, i, True)),
        "gatv2 shared": (sh, lambda rg, pk, i: _run_v2_shared(rg, pk, i, False)),
        "bf16 fused-el": (lambda: gat(True), lambda rg, pk, i: _run_gat("fused", rg, pk, i, True)),
        "bf16 unfused": (lambda: gat(True), lambda rg, pk, i: _run_gat("unfused", rg, pk, i, True)),
    }


REPEAT_KINDS = ["fused-el", "fused-elx", "fused-elx one leaf", "unfused", "unfused gmax", "gatv2",
                "gatv2 gmax", "gatv2 shared", "bf16 fused-el", "bf16 unfused"]


@pytest.mark.parametrize("kind", REPEAT_KINDS)
def test_repeat_is_bitwise(graphs, kind):
    """fixed-order reductions and no atomics: two runs of a kind on the `tree` form (chunks, two
    tree levels) at (8, 64) return the same bits, output and every gradient"""
    make, run = _repeat_runs(8, 64)[kind]
    rg, pack = graphs["tree"]
    inp = make()
    first, second = run(rg, pack, inp), run(rg, pack, inp)
    assert sorted(first) == sorted(second)
    for name in first:
        assert torch.equal(first[name], second[name]), f"{kind} {name}"


# ---- shapes outside the tiers --------------------------------------------------------------------
# (kind, bf16, H, D, the operator that refuses). Every one of them is refused: D / vector is no
# power of two ((4, 12), (2, 96): 3 and 24 vectors a head; bf16 (4, 12)), D is no multiple of the
# vector ((4, 6); bf16 (4, 4)), the edge softmax takes powers of two <= 32 heads ((3, 8), H = 64)
# and the score kernels rows of at most 1024 elements ((32, 64)). None is met by the bound instead.
BOUNDARY = [("fused", False, 4, 12, "gat_fused"), ("fused", False, 2, 96, "gat_fused"),
            ("fused", False, 4, 6, "gat_fused"), ("fused", True, 4, 4, "gat_fused"),
            ("fused", True, 4, 12, "gat_fused"),
            ("unfused", False, 4, 12, "head_spmm"), ("unfused", False, 2, 96, "head_spmm"),
            ("unfused", False, 4, 6, "head_spmm"), ("unfused", True, 4, 4, "head_spmm"),
            ("unfused", True, 4, 12, "head_spmm"),
            ("gatv2", False, 4, 12, "gatv2_scores"), ("gatv2", False, 3, 8, "edge_softmax_logits"),
            ("gatv2", False, 32, 64, "gatv2_scores")]


@pytest.mark.parametrize("kind,bf16,H,D,op", BOUNDARY)
def test_shape_outside_the_tiers_is_refused_in_forward(graphs, kind, bf16, H, D, op):
    """a shape some kernel of the chain does not take raises ValueError from the forward call,
    naming the operator and the shape, before anything is launched: never a forward result whose
    backward then fails (what ops.gat_fused did at D = 12, 24, 96: dispatch_gat_fused takes any
    D % 4 == 0, dispatch_heads in its backward does not)"""
    rg, pack = graphs["default"]
    with pytest.raises(ValueError) as ei:
        if kind == "gatv2":
            _run_v2(rg, pack, _dev(AR.gatv2_inputs("unit", N, H, D, AR.N_REL, _seed(H, D))), False)
        else:
            _run_gat(kind, rg, pack, _dev(AR.gat_inputs("unit", N, H, D, AR.N_REL, _seed(H, D),
                                                        bf16=bf16)), bf16=bf16)
    msg = str(ei.value)
    assert f"ops.{op}:" in msg and f"H={H}" in msg, msg
    assert op == "edge_softmax_logits" or f"D={D}" in msg, msg
    assert ("bfloat16" in msg) == bf16, msg


def test_edge_softmax_refuses_64_heads(graphs):
    from regnn_hip import ops
    rg, pack = graphs["default"]
    s = torch.randn(rg.E, 64, device=DEV, requires_grad=True)
    with pytest.raises(ValueError, match=r"ops\.edge_softmax_logits: .*H=64"):
        ops.edge_softmax_logits(rg, s, None, None, False)
