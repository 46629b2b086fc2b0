"""Relation SpMM (re_spmm.hip) against the fp64 restatement of _spmm_ref.py under the per-element
metric, over every width tier of dispatch<T>(), every compile-time mode, the three plan forms of
the 320-node ladder graph (chunks, a two-level tree, no plan), both storage types and both
pre-scale policies. Every graph is built once per module and every fp64 reference once per
(case kind, width, dtype); a case is a handful of launches.

Which parametrisation reaches what (all against spmm_case_ref unless noted):
  dispatch branch (LPR, NV)            nvec of WIDTHS (F = 4 nvec fp32, 8 nvec bf16)
    (4,1) 1 3 4   (8,1) 5 8   (16,1) 9 15   (16,1,FULL; launch_f16v) 16   (16,2) 17 32
    (16,3) 33 48  (16,4) 49 64  (64,2) 65 128  (64,4) 129 256   ragged first, full last
  spmm_main only                       form "noplan"
  spmm_chunks + spmm_fixup             form "default" (rows 257 and 300: two chunks each, one
                                       partial_reduce level), form "tree" (split 8, chunk 4:
                                       two levels); every nvec of test_matrix in each form
  kFwd                                 every forward; bias in the kernel: no_post, emit, fused
  kBwd                                 test_argument_shapes copy_u / tab_nograd
  kBwdSlab                             test_matrix (+ node gradient, ng_a / ng_b with PRESCALE
                                       off), test_argument_shapes no_pre / no_post / bipartite
  kBwdEdge                             test_argument_shapes edge (ops.edge_spmm)
  kBwdBoth                             test_bwd_both_c_abi (raw regnn_spmm_bwd; not reachable
                                       from the operators)
  in-kernel in_scale, d0 = s0 * os     PRESCALE off (test_matrix, bipartite_off)
  regnn_row_scale (+ dot)              PRESCALE auto; its U = 2 / 4 forms in test_tune_row_pass
  epilogue_fused                       test_fused_forward vs fused_ref (row metric)
  regnn_spmm_fwd_next                  test_emit
  grid-stride loops                    test_tune_grid_cap (two blocks)

Bounds. fp32: rel_err <= TOL_F32 = 1e-5 (test_cpu_spmm_ref.py: the arithmetic alone costs at
most a quarter of it). bf16: TOL_F32 + m * BF16_REL, with rel_err(bf16_store=True) for a tensor
the kernel stores in bf16; m from BF16_M below. Where re_spmm adds the bias outside the kernel
(a differentiable post) the bf16 rows' y is fp32 = bf16(post * agg) + bias: see _check; the
matrix also runs that forward with the bias in the kernel, under the plain bound. Forward y bits do not depend on regnn_tune key 2
(test_tune_rows_in_flight says why)."""
import contextlib

import pytest
import torch

import _spmm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 320
FORMS = list(R.PLAN_FORMS)
# one ragged and one full width per LPR family
FAMILY_NVEC = [3, 4, 5, 8, 9, 16, 33, 64, 65, 256]
ONE_PER_FAMILY = [3, 5, 16, 33, 129]
FUSED_NVEC = [1, 3, 9, 16, 33, 49, 65, 129, 256]

# bf16-rounded intermediates on an output's path, keyed by (output, PRESCALE mode and bwd).
# The roundings:
#   A  pre * x written in x's dtype by regnn_row_scale (ops.py:277, re_spmm.hip:886), auto only
#   B  post * gy written likewise in backward (ops.py:361), auto only
#   C  the stored y that the node gradient's <gy, y> / post reads: by regnn_row_scale's dot
#      (ops.py:362, re_spmm.hip:874) under auto, as ng_b (ops.py:366, re_spmm.hip:306) under off
# y: A. g_x: B. g_tab (dots <post gy, x> of re_spmm.hip:216): B. The combined node gradient
# g_pre = <x, acc> + <gy, y> / post: the first term reads B, the second C and, through y, A;
# counted per additive term (the terms' scales add up), so 2 under auto and 1 (C) under off.
# g_post alone: C and A. g_bias is torch's column sum of gy: none.
BF16_M = {("y", "auto"): 1, ("y", "off"): 0,
          ("g_x", "auto"): 1, ("g_x", "off"): 0,
          ("g_tab", "auto"): 1, ("g_tab", "off"): 0,
          ("g_pre", "auto"): 2, ("g_pre", "off"): 1,
          ("g_post", "auto"): 2, ("g_post", "off"): 1,
          ("g_bias", "auto"): 0, ("g_bias", "off"): 0}

_REF = {}          # (kind, F, bf16, n_rel) -> (inputs, want, scale), computed once on the CPU
WORST = {}         # (test, dtype, output) -> worst error seen (printed; read off one run)


def _note(test, bf16, name, err):
    key = (test, "bf16" if bf16 else "fp32", name)
    WORST[key] = max(WORST.get(key, 0.0), err)
    print(f"ERR {key[0]} {key[1]} {name} {err:.3e}")


# ---- graphs, once per module -------------------------------------------------------------------
def _rel_ids(E, n_rel, seed=5):
    g = torch.Generator().manual_seed(seed + n_rel)
    r = torch.randint(1, n_rel + 1, (E,), generator=g)
    r[:n_rel] = torch.arange(1, n_rel + 1)              # every id occurs, the last one included
    return r


@pytest.fixture(scope="module")
def ladder():
    """form -> (rg, {n_rel: pack}); n_rel 7: the ladder's own ids, 1 / 64 / 65: drawn here"""
    out = {}
    for form in FORMS:
        rg, e_feat = R.ladder_graph(form, DEV, N)
        packs = {R.N_REL: rg.rel_pack(e_feat, num_rel=R.N_REL)}
        for n_rel in (1, 64, 65):
            packs[n_rel] = rg.rel_pack(_rel_ids(rg.E, n_rel).to(DEV), num_rel=n_rel)
        long_rows = form != "noplan"
        assert (rg.csr_plan.n_long > 0) == long_rows and (rg.csc_plan.n_long > 0) == long_rows
        out[form] = (rg, packs)
    return out


@pytest.fixture(scope="module")
def bipartite():
    out = {}
    for form in FORMS:
        rg, e_feat = R.ladder_bipartite(form, DEV, N)
        long_rows = form != "noplan"
        assert (rg.csr_plan.n_long > 0) == long_rows and (rg.csc_plan.n_long > 0) == long_rows
        assert rg.n_src == N + R.N_EXTRA and rg.n_dst == N
        out[form] = (rg, {R.N_REL: rg.rel_pack(e_feat, num_rel=R.N_REL)})
    return out


def _poison(*shapes):
    """NaN-filled blocks of the outputs' sizes go back to the allocator: a skipped store is
    likely to surface as NaN instead of a stale correct row"""
    junk = [torch.full(s, float("nan"), device=DEV) for s in shapes]
    del junk


def _dev(t, bf16=False, grad=False):
    if t is None:
        return None
    t = t.to(DEV, torch.bfloat16 if bf16 else t.dtype)
    return t.requires_grad_(True) if grad else t


def _csr(rg, pack):
    return rg.csr_ptr.cpu(), rg.csr_idx.cpu(), pack.rel_csr.cpu()


# ---- references, once per (kind, F, dtype, n_rel) ----------------------------------------------
# kind -> (tab, pre, post, bias, edge_w) of the reference; "same": post is pre
KINDS = {"matrix": ("tab", "pre", "same", "bias", None),
         "copy_u": (None, "pre", "same", None, None),
         "no_pre": ("tab", None, "post", "bias", None),
         "no_post": ("tab", "pre", None, "bias", None),
         "bipartite": ("tab", "pre", "post", "bias", None),
         "edge": (None, None, None, None, "edge_w"),
         "both": ("tab", "pre", "post", None, "edge_w"),      # the C-ABI case, and
         "both_noew": ("tab", "pre", "post", None, None)}     # its relation bins (no ew)


def _reference(kind, rg, pack, F, bf16, n_rel=R.N_REL):
    key = (kind, F, bf16, n_rel)
    if key not in _REF:
        seed = 100003 * n_rel + 2 * F + int(bf16)
        d = R.spmm_inputs(F, rg.n_src, rg.n_dst, n_rel, seed, bf16, n_edge=rg.E)
        d["edge_w_csr"] = d["edge_w"][rg.csr_eid.cpu()]
        tab, pre, post, bias, ew = KINDS[kind]
        args = {"tab": d["tab"] if tab else None, "pre": d["pre"] if pre else None,
                "bias": d["bias"] if bias else None, "ew": d["edge_w_csr"] if ew else None}
        args["post"] = args["pre"] if post == "same" else (d["post"] if post else None)
        ptr, idx, rel = _csr(rg, pack)
        want, scale = R.spmm_case_ref(ptr, idx, rel, d["x"], args["tab"], args["pre"],
                                      args["post"], args["bias"], d["gy"], rg.n_src,
                                      edge_w=args["ew"])
        _REF[key] = (d, want, scale)
    return _REF[key]


def _check(test, got, want, scale, bf16, prescale="auto", bias_outside=False):
    """every output of `got` under its bound; returns the failures. bias_outside: y is the
    kernel's bf16 rows plus a bias added by torch in fp32 (ops.py:431, a differentiable post),
    so the store's rounding is relative to |y - bias| <= scale and not to |y|: one more
    BF16_REL on the scale in place of rel_err's 2^-8 |ref|."""
    fails = []
    for name in sorted(got):
        g = got[name]
        assert g is not None, name
        bound, stored = R.TOL_F32, False
        if bf16:
            stored = g.dtype == torch.bfloat16
            m = BF16_M[(name, prescale)]
            if name == "y" and bias_outside:
                assert not stored
                m += 1
            bound = R.TOL_F32 + m * R.BF16_REL
        err = R.rel_err(g.cpu(), want[name], scale[name], bf16_store=stored)
        _note(test, bf16, name, err)
        if not err <= bound:
            fails.append(f"{name}: err {err:.3e} > {bound:.3e}")
    return fails


# ---- a. the matrix -----------------------------------------------------------------------------
def _matrix_run(rg, pack, d, bf16):
    from regnn_hip import ops
    F = d["x"].shape[1]
    x = _dev(d["x"], bf16, True)
    tab, norm, bias = _dev(d["tab"], grad=True), _dev(d["pre"], grad=True), _dev(d["bias"], grad=True)
    _poison((N, F), (N, F), (N, F), (N,))
    y = ops.re_spmm(rg, x, tab, pack, pre=norm, post=norm, bias=bias)
    y.backward(_dev(d["gy"]).to(y.dtype))
    return {"y": y.detach(), "g_x": x.grad, "g_tab": tab.grad, "g_pre": norm.grad,
            "g_bias": bias.grad}


def _matrix_case(test, ladder, form, nvec, bf16, prescale, monkeypatch, n_rel=R.N_REL):
    from regnn_hip import ops
    if prescale == "off":
        monkeypatch.setitem(ops.PRESCALE, "mode", "off")
        monkeypatch.setitem(ops.PRESCALE, "bwd", "off")
    rg, packs = ladder[form]
    F = R.width(nvec, bf16)
    d, want, scale = _reference("matrix", rg, packs[n_rel], F, bf16, n_rel)
    got = _matrix_run(rg, packs[n_rel], d, bf16)
    assert got["g_x"].dtype == (torch.bfloat16 if bf16 else torch.float32)
    fails = _check(test, got, want, scale, bf16, prescale, bias_outside=True)
    if bf16:
        # the same forward with no input requiring grad: the bias is added in the kernel, y is
        # stored in bf16 once, after it, and holds the plain bound (m = 0 with PRESCALE off)
        x, tab, norm, bias = _dev(d["x"], True), _dev(d["tab"]), _dev(d["pre"]), _dev(d["bias"])
        _poison((N, F))
        y = ops.re_spmm(rg, x, tab, packs[n_rel], pre=norm, post=norm, bias=bias)
        assert y.dtype == torch.bfloat16
        fails += _check(test + "_bias_in_kernel", {"y": y}, want, scale, True, prescale)
    assert not fails, f"nvec={nvec} ({R.WIDTHS.get(nvec)}) {form} {prescale}: " + "; ".join(fails)
    return got


@pytest.mark.parametrize("prescale", ["auto", "off"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("nvec", list(R.WIDTHS))
def test_matrix(ladder, monkeypatch, nvec, bf16, form, prescale):
    """ops.re_spmm with a relation table, pre is post (same-scale), bias, every input requiring
    grad: y, g_x, g_tab, the combined node gradient and g_bias."""
    _matrix_case("matrix", ladder, form, nvec, bf16, prescale, monkeypatch)


# ---- b. argument shapes ------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["copy_u", "tab_nograd", "no_pre", "no_post", "bipartite",
                                     "bipartite_off", "edge"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nvec", FAMILY_NVEC)
def test_argument_shapes(ladder, bipartite, monkeypatch, nvec, form, variant):
    from regnn_hip import ops
    F = R.width(nvec)
    prescale = "off" if variant.endswith("_off") else "auto"
    if prescale == "off":
        monkeypatch.setitem(ops.PRESCALE, "mode", "off")
        monkeypatch.setitem(ops.PRESCALE, "bwd", "off")
    kind = {"tab_nograd": "matrix", "bipartite_off": "bipartite"}.get(variant, variant)
    rg, packs = (bipartite if kind == "bipartite" else ladder)[form]
    pack = packs[R.N_REL]
    d, want, scale = _reference(kind, rg, pack, F, False)
    x = _dev(d["x"], grad=True)
    gy = _dev(d["gy"])
    _poison((rg.n_dst, F), (rg.n_src, F), (rg.n_src,), (rg.E,))
    if variant == "copy_u":
        norm = _dev(d["pre"], grad=True)
        y = ops.re_spmm(rg, x, pre=norm, post=norm)
        y.backward(gy)
        got = {"y": y, "g_x": x.grad, "g_pre": norm.grad}
    elif variant == "tab_nograd":
        norm, bias = _dev(d["pre"], grad=True), _dev(d["bias"], grad=True)
        y = ops.re_spmm(rg, x, _dev(d["tab"]), pack, pre=norm, post=norm, bias=bias)
        y.backward(gy)
        got = {"y": y, "g_x": x.grad, "g_pre": norm.grad, "g_bias": bias.grad}
    elif variant == "no_pre":
        tab, post, bias = (_dev(d[k], grad=True) for k in ("tab", "post", "bias"))
        y = ops.re_spmm(rg, x, tab, pack, post=post, bias=bias)
        y.backward(gy)
        got = {"y": y, "g_x": x.grad, "g_tab": tab.grad, "g_post": post.grad, "g_bias": bias.grad}
    elif variant == "no_post":
        tab, pre, bias = (_dev(d[k], grad=True) for k in ("tab", "pre", "bias"))
        y = ops.re_spmm(rg, x, tab, pack, pre=pre, bias=bias)        # bias in the kernel
        y.backward(gy)
        got = {"y": y, "g_x": x.grad, "g_tab": tab.grad, "g_pre": pre.grad, "g_bias": bias.grad}
    elif kind == "bipartite":
        tab, pre, post, bias = (_dev(d[k], grad=True) for k in ("tab", "pre", "post", "bias"))
        assert pre.numel() == N + R.N_EXTRA and post.numel() == N
        y = ops.re_spmm(rg, x, tab, pack, pre=pre, post=post, bias=bias)
        y.backward(gy)
        got = {"y": y, "g_x": x.grad, "g_tab": tab.grad, "g_pre": pre.grad, "g_post": post.grad,
               "g_bias": bias.grad}
    else:
        ew = _dev(d["edge_w"], grad=True)                            # the caller's edge order
        y = ops.edge_spmm(rg, x, ew)
        y.backward(gy)
        got = {"y": y, "g_x": x.grad, "g_ew": ew.grad[rg.csr_eid]}   # -> CSR order
    got["y"] = got["y"].detach()
    assert sorted(got) == sorted(k for k in want if not (variant == "tab_nograd" and k == "g_tab"))
    fails = _check("shapes_" + variant, got, want, scale, False)
    assert not fails, f"nvec={nvec} {form} {variant}: " + "; ".join(fails)


# ---- c. kBwdBoth through the C ABI -------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nvec", ONE_PER_FAMILY)
def test_bwd_both_c_abi(bipartite, nvec, form):
    """One raw regnn_spmm_bwd with a slab AND edge_grad (kBwdBoth), relation table, edge weights,
    in_scale and out_scale all present, on the bipartite ladder; arguments as _ReSpmm.backward
    and _EdgeSpmm.backward form them. The kernel's per-edge value is <g_v, x_u> * in_scale *
    out_scale without tab and ew (comment above accumulate): times tab[rel_e] it is d loss /
    d ew_e, and its relation bins are d loss / d tab of the same inputs without edge weights."""
    from regnn_hip import _lib as L, ops
    rg, packs = bipartite[form]
    pack = packs[R.N_REL]
    F = R.width(nvec)
    d, want, scale = _reference("both", rg, pack, F, False)
    _, want_t, scale_t = _reference("both_noew", rg, pack, F, False)
    assert torch.equal(d["x"], _REF[("both_noew", F, False, R.N_REL)][0]["x"])   # same inputs
    x, gy, tab, pre, post = (_dev(d[k]) for k in ("x", "gy", "tab", "pre", "post"))
    w_csc = _dev(d["edge_w"])[rg.csc_eid].contiguous()
    n_rel = tab.numel()
    _poison((rg.n_src, F), (rg.E,), (rg.n_src,))
    gx = torch.empty(rg.n_src, F, device=DEV)
    eg = torch.empty(rg.E, device=DEV)
    node = torch.empty(rg.n_src, device=DEV)
    slab = ops._slab(n_rel, DEV)
    plan_args, part = ops._plan_args(rg.csc_plan, F, DEV)
    L.call("regnn_spmm_bwd", L.ptr(rg.csc_ptr), L.ptr(rg.csc_idx), L.ptr(pack.rel_csc),
           L.ptr(tab), L.ptr(w_csc), L.ptr(post), L.ptr(pre), L.ptr(gy), L.ptr(x), None,
           L.ptr(gx), L.ptr(slab), n_rel, L.ptr(eg), L.ptr(node), rg.n_src, F, L.dtype_code(x),
           *plan_args, L.stream())
    g_tab = ops._reduce(slab, n_rel)
    torch.cuda.synchronize()
    del part
    # CSC position -> CSR position; d loss / d ew_e = tab[rel_e] * the kernel's per-edge value
    g_ew = torch.empty(rg.E, dtype=torch.float64)
    g_ew[rg.csc2csr.cpu().long()] = eg.cpu().double() * d["tab"].double()[pack.rel_csc.cpu().long()]
    got = {"g_x": gx, "g_pre": node, "g_ew": g_ew}
    fails = _check("bwd_both", got, want, scale, False)
    fails += _check("bwd_both", {"g_tab": g_tab}, want_t, scale_t, False)
    assert not fails, f"nvec={nvec} {form}: " + "; ".join(fails)


# ---- d. fused forward --------------------------------------------------------------------------
# (LN, residual, ReLU, bias); LN "plain": no weight and no bias
FUSED_COMBOS = [("affine", True, True, True), ("affine", False, True, False),
                (None, True, False, True), ("plain", False, False, True),
                (None, False, True, False)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("nvec", FUSED_NVEC)
def test_fused_forward(ladder, nvec, bf16, form):
    """ops.re_spmm_fused (residual + LayerNorm + ReLU epilogue, group_sum<LPR> over a possibly
    ragged row) against fused_ref: |got - ref| / max(1, max |ref| of the row) <= 1e-5, in bf16
    less the rounding of the one store (the epilogue computes in fp32 from exact inputs: m = 0).
    Every row that is not constant deviates by >= 0.1 before the LayerNorm. Row 0 has no edges:
    without bias and residual it must be exactly relu(ln_b)."""
    from regnn_hip import ops
    rg, packs = ladder[form]
    pack = packs[R.N_REL]
    F = R.width(nvec, bf16)
    key = ("fused", F, bf16)
    if key not in _REF:
        d = R.fused_inputs(F, N, N, R.N_REL, 7 * F + int(bf16), bf16)
        refs = []
        for ln, res, relu, bias in FUSED_COMBOS:
            lnt = None if ln is None else ((d["ln_w"], d["ln_b"], 1e-5) if ln == "affine"
                                           else (None, None, 1e-5))
            refs.append(R.fused_ref(*_csr(rg, pack), d["x"], d["tab"], d["post"],
                                    d["bias"] if bias else None, d["residual"] if res else None,
                                    lnt, relu))
        _REF[key] = (d, refs)
    d, refs = _REF[key]
    x, tab, post, bias, res, lw, lb = (_dev(d[k], bf16 and k in ("x", "residual")) for k in
                                       ("x", "tab", "post", "bias", "residual", "ln_w", "ln_b"))
    fails = []
    for (ln, use_res, relu, use_bias), (ref, den, min_std) in zip(FUSED_COMBOS, refs):
        assert min_std >= 0.1, min_std
        _poison((N, F))
        lnt = None if ln is None else ((lw, lb, 1e-5) if ln == "affine" else (None, None, 1e-5))
        with torch.no_grad():
            y = ops.re_spmm_fused(rg, x, tab, pack, post=post, bias=bias if use_bias else None,
                                  residual=res if use_res else None, ln=lnt, relu=relu)
        assert y.dtype == x.dtype
        err = R.fused_err(y.cpu(), ref, den, bf16_store=bf16)
        _note("fused", bf16, "y", err)
        if not err <= R.TOL_F32:
            fails.append(f"{(ln, use_res, relu, use_bias)}: err {err:.3e} (min std {min_std:.2f})")
        if ln == "affine" and not use_res and not use_bias:
            want0 = d["ln_b"].clamp(min=0.0)
            if bf16:
                want0 = want0.bfloat16()
            assert torch.equal(y[0].cpu(), want0), "the empty row is not exactly relu(ln_b)"
    assert not fails, f"nvec={nvec} {form}: " + "; ".join(fails)


# ---- e. emit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("nvec", FUSED_NVEC)
def test_emit(ladder, nvec, bf16, form):
    """ops.re_spmm(..., emit=(scale, None)): the consumer's pre-scaled rows scale * y leave from
    the same epilogue (regnn_spmm_fwd_next). fp32: against scale * y under the y scale times
    |scale|; bf16: exactly the bf16 rounding of scale * bf16(y), which the kernel forms from the
    stored values."""
    from regnn_hip import ops
    rg, packs = ladder[form]
    pack = packs[R.N_REL]
    F = R.width(nvec, bf16)
    d, want, scale = _reference("matrix", rg, pack, F, bf16)
    x, tab, norm, bias = _dev(d["x"], bf16), _dev(d["tab"]), _dev(d["pre"]), _dev(d["bias"])
    nscale = _dev(d["post"])
    _poison((N, F), (N, F))
    y, xs = ops.re_spmm(rg, x, tab, pack, pre=norm, post=norm, bias=bias, emit=(nscale, None))
    assert xs is not None and xs.dtype == x.dtype and y.dtype == x.dtype
    fails = _check("emit", {"y": y}, want, scale, bf16)
    if bf16:
        assert torch.equal(xs, (y.float() * nscale[:, None]).bfloat16())
    else:
        s = d["post"].double()[:, None]
        err = R.rel_err(xs.cpu(), want["y"] * s, scale["y"] * s.abs())
        _note("emit", bf16, "xs", err)
        if not err <= R.TOL_F32:
            fails.append(f"xs: err {err:.3e}")
    assert not fails, f"nvec={nvec} {form}: " + "; ".join(fails)


# ---- f. edges of the argument checks -----------------------------------------------------------
@pytest.mark.parametrize("prescale", ["auto", "off"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nvec", [16, 65])
@pytest.mark.parametrize("n_rel", [1, 64])
def test_relation_count_limits(ladder, monkeypatch, n_rel, nvec, form, prescale):
    """n_rel = 1, and n_rel = 64: exactly 64 KiB of lane-private LDS bins, the limit."""
    _matrix_case(f"n_rel{n_rel}", ladder, form, nvec, False, prescale, monkeypatch, n_rel=n_rel)


def test_relation_count_over_limit(ladder):
    from regnn_hip import ops
    rg, packs = ladder["default"]
    d = R.spmm_inputs(64, N, N, 65, 1)
    x, tab = _dev(d["x"], grad=True), _dev(d["tab"], grad=True)
    y = ops.re_spmm(rg, x, tab, packs[65])
    with pytest.raises(RuntimeError, match="invalid argument"):
        y.backward(_dev(d["gy"]))


@pytest.mark.parametrize("F,bf16", [(1028, False), (2056, True), (6, False), (12, True)])
def test_unsupported_width(ladder, F, bf16):
    """rows past 256 vectors and rows that are no whole number of 16-byte vectors: the forward
    and the backward refuse and leave the caller's output untouched"""
    from regnn_hip import _lib as L, ops
    rg, _ = ladder["default"]
    dt = torch.bfloat16 if bf16 else torch.float32
    x = torch.ones(N, F, dtype=dt, device=DEV)
    out = torch.full((N, F), float("nan"), dtype=dt, device=DEV)
    plan_args, part = ops._plan_args(rg.csr_plan, F, DEV)
    with pytest.raises(RuntimeError, match="unsupported shape/dtype"):
        L.call("regnn_spmm_fwd", L.ptr(rg.csr_ptr), L.ptr(rg.csr_idx), None, None, None, None,
               None, None, L.ptr(x), L.ptr(out), N, F, L.dtype_code(x), *plan_args, L.stream())
    plan_args, part2 = ops._plan_args(rg.csc_plan, F, DEV)
    with pytest.raises(RuntimeError, match="unsupported shape/dtype"):
        L.call("regnn_spmm_bwd", L.ptr(rg.csc_ptr), L.ptr(rg.csc_idx), None, None, None, None,
               None, L.ptr(x), L.ptr(x), None, L.ptr(out), None, 0, None, None, N, F,
               L.dtype_code(x), *plan_args, L.stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


@contextlib.contextmanager
def _tune(key, value):
    """regnn_tune(key, value) for a block; the old value is restored in a finally"""
    from regnn_hip import _lib as L
    old = L._so.regnn_tune(key, value)
    try:
        yield
    finally:
        L._so.regnn_tune(key, old)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("un", [4, 16])
def test_tune_rows_in_flight(ladder, monkeypatch, un, bf16, form):
    """regnn_tune(2, 4 / 16) at 16 vectors per row (F = 64 fp32, 128 bf16): the matrix's
    assertions, and the same bits as the default. launch_f16v only changes UNT, the number of
    rows whose loads are issued before any is consumed; accumulate() still folds edge
    e0 + k + u into acc in ascending order with one fmaf each, and an edge slot past the batch's
    end adds fmaf(0, v, acc) = acc and a dot scaled by 0 whatever UN is. So y, g_x and the
    relation bins must not change by a bit."""
    base = _matrix_case("tune_un", ladder, form, 16, bf16, "auto", monkeypatch)
    with _tune(2, un):
        got = _matrix_case("tune_un", ladder, form, 16, bf16, "auto", monkeypatch)
    for k in ("y", "g_x", "g_tab", "g_pre"):
        assert torch.equal(got[k], base[k]), f"{k} changed with {un} rows in flight"


@pytest.mark.parametrize("prescale", ["auto", "off"])
@pytest.mark.parametrize("nvec", ONE_PER_FAMILY)
def test_tune_grid_cap(ladder, monkeypatch, nvec, prescale):
    """a grid of two blocks: every block strides over many segments, chunks and rows"""
    with _tune(1, 2):
        _matrix_case("grid_cap", ladder, "tree", nvec, False, prescale, monkeypatch)


@pytest.mark.parametrize("rows", [2, 4])
@pytest.mark.parametrize("nvec", ONE_PER_FAMILY)
def test_tune_row_pass(ladder, monkeypatch, nvec, rows):
    """regnn_row_scale with 2 / 4 rows per lane group and step (PRESCALE auto). With 320 rows the
    groups of the first step cover every row, so the further rows of each group fall past the
    end and the ok[u] guards decide every store."""
    with _tune(4, rows):
        _matrix_case("row_pass", ladder, "tree", nvec, False, "auto", monkeypatch)
        _matrix_case("row_pass", ladder, "tree", nvec, True, "auto", monkeypatch)


# ---- g. determinism ----------------------------------------------------------------------------
@pytest.mark.parametrize("nvec", ONE_PER_FAMILY)
def test_two_runs_equal(ladder, monkeypatch, nvec):
    a = _matrix_case("determinism", ladder, "tree", nvec, False, "auto", monkeypatch)
    b = _matrix_case("determinism", ladder, "tree", nvec, False, "auto", monkeypatch)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k} differs between two runs"


@pytest.fixture(scope="module", autouse=True)
def _worst_report():
    """after the module: the worst error per (test, dtype, output) of this run (pytest -s)"""
    yield
    for key in sorted(WORST):
        print("WORST", *key, f"{WORST[key]:.3e}")
