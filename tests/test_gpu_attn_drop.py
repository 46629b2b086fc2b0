"""The fused GAT attention dropout on the GPU: ops.gat_fused(attn_drop=p) (regnn_gat_fused_fwd_drop
and, in the backward, regnn_spmm_heads_bwd_drop) against the masked fp64 restatement of
_attn_drop_ref.py under the per-element metric of _attention_ref.py, the layer and model wiring,
and what the mask may depend on (the seed in device memory, the CSR edge position and the head:
not the plan form).

Parity matrix: the ladder graph (N = 320, in-degrees 0 .. 300) in its three plan forms, (H, D) in
_attn_drop_ref.SHAPES, p in {0.5 (8-bit draws), 0.2, 0.6 (16-bit draws)}, with and without the
relation table, in two score forms:
  el-reading   el given; recipes `unit` and `wide` (_attention_ref.gat_inputs)
  ELX          attn_l passed, so the kernel re-forms el from the rows it gathers. el must then BE
               attn_dots(ft, attn_l): the inputs are gat_attn_inputs' (the `wide` recipe's el is
               no dot of ft). ft enters as two leaves of equal values, one under attn_dots and
               one under gat_fused, so g_ft is the aggregation's alone and g_el / g_er are read
               off the dots' outputs: the same five tensors as the el-reading form, against the
               same restatement with the fp32 el / er as its inputs.
Bound: out, g_ft, g_el, g_er, g_tab <= TOL_F32 = 1e-5; bf16 rows (el-reading) with
rel_err(bf16_store=True) on the tensors stored in bf16. test_cpu_attn_drop.py shows that the
arithmetic of the restatement alone costs at most a quarter of the bound on these inputs and
that the masks are fair. Each case prints its maxima (-s); DESIGN.md section 8 records them."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _attention_ref as AR
import _attn_drop_ref as DR
import _golden as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 320
NAMES = ["out", "g_ft", "g_el", "g_er", "g_tab"]


@pytest.fixture(scope="module")
def graphs():
    out = {}
    for form in AR.PLAN_FORMS:
        rg, e_feat = AR.ladder_graph(form, DEV, N)
        out[form] = (rg, rg.rel_pack(e_feat, num_rel=AR.N_REL))
    return out


@pytest.fixture
def fused_mode():
    """ops.ATTN_DROP["mode"] = "fused" for one test (the default is by measurement: "torch")"""
    from regnn_hip import ops
    old = ops.ATTN_DROP["mode"]
    ops.ATTN_DROP["mode"] = "fused"
    yield
    ops.ATTN_DROP["mode"] = old


def _seed(s):
    return torch.tensor([s], dtype=torch.int64, device=DEV)


def _poison(rg, H, D):
    """NaN-filled blocks of the outputs' sizes go back to the allocator: a skipped store is likely
    to surface as NaN instead of a stale correct value"""
    junk = [torch.full(sh, float("nan"), device=DEV) for sh in
            [(N, H, D)] * 2 + [(rg.E, H)] * 3 + [(N, H)] * 2]
    del junk


def _run(rg, pack, inp, p, seed, elx=False, bf16=False, drop=None):
    """one forward + backward of ops.gat_fused: dict over NAMES. inp: (ft, el, er, tab, gy, slope)
    or, elx, (ft, al, ar, tab, gy, slope) on the device; tab None: no relation table."""
    from regnn_hip import ops
    ft0, a0, b0, tab0, gy, slope = inp
    H, D = ft0.shape[1:]
    _poison(rg, H, D)
    ft = (ft0.bfloat16() if bf16 else ft0.clone()).requires_grad_(True)
    tab = None if tab0 is None else tab0.clone().requires_grad_(True)
    if elx:
        el, er = ops.attn_dots(ft0.clone().requires_grad_(True), a0, b0)
        el.retain_grad(); er.retain_grad()
        al = a0
    else:
        el, er, al = a0.clone().requires_grad_(True), b0.clone().requires_grad_(True), None
    if drop is not None:              # a raw (seed, keep16, scale) request
        y = ops._GatFused.apply(el, er, tab, ft, rg, pack if tab is not None else None, slope, al,
                                drop)
    else:
        y = ops.gat_fused(rg, el, er, ft, tab, pack if tab is not None else None, slope,
                          attn_l=al, attn_drop=p, drop_seed=seed)
    y.backward(gy.to(ft.dtype))
    got = {"out": y.detach(), "g_ft": ft.grad, "g_el": el.grad, "g_er": er.grad}
    if tab is not None:
        got["g_tab"] = tab.grad
    return got, (el.detach(), er.detach())


def _inputs(kind, H, D, bf16=False):
    if kind == "elx":
        inp = AR.gat_attn_inputs(N, H, D, AR.N_REL, 1000 * H + D)
    else:
        inp = AR.gat_inputs(kind, N, H, D, AR.N_REL, 1000 * H + D, bf16=bf16)
    return tuple(t.to(DEV) if torch.is_tensor(t) else t for t in inp)


def _compare(tag, got, want, scale, fails, worst, bf16=False, tol=AR.TOL_F32):
    for name in sorted(want):
        stored = bf16 and name in ("out", "g_ft")
        err = AR.rel_err(got[name], want[name], scale[name], bf16_store=stored)
        worst[name] = max(worst.get(name, 0.0), err)
        if not err <= tol:
            fails.append(f"{tag} {name}: err {err:.3e}")
        if not DR.exact_zeros(got[name], scale[name]):
            fails.append(f"{tag} {name}: non-zero where the scale is 0")


@pytest.mark.parametrize("p", DR.PS)
@pytest.mark.parametrize("H,D", DR.SHAPES)
def test_parity_vs_fp64(graphs, H, D, p):
    """1: forward and every gradient against the masked fp64 restatement, every plan form, both
    score forms, with and without the relation table"""
    w = DR.drop_weight(DR.SEEDS[p], graphs["default"][0].E, H, p).to(DEV)
    seed = _seed(DR.SEEDS[p])
    fails, worst = [], {}
    for kind in ("unit", "wide", "elx"):
        inp = _inputs(kind, H, D)
        for use_tab in (True, False):
            inp_t = inp if use_tab else inp[:3] + (None,) + inp[4:]
            want = scale = None
            for form, (rg, pack) in graphs.items():
                got, (el, er) = _run(rg, pack, inp_t, p, seed, elx=kind == "elx")
                if want is None:                  # the CSR is the same in every form
                    want, scale = DR.gat_drop_case_ref(
                        rg.csr_ptr, rg.csr_idx, pack.rel_csr, el, er, inp_t[3], inp_t[0], inp_t[4],
                        inp_t[5], w)
                    assert bool((scale["out"] == 0).any())
                _compare(f"{kind} tab={use_tab} {form}", got, want, scale, fails, worst)
    print(f"attn_drop parity H={H} D={D} p={p}: " +
          " ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())))
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("p", DR.PS)
def test_parity_bf16_rows(graphs, p):
    """1, bf16 rows: the el-reading form (the ELX form is fp32 only), H = 8, D = 64"""
    H, D = 8, 64
    w = DR.drop_weight(DR.SEEDS[p], graphs["default"][0].E, H, p).to(DEV)
    inp = _inputs("unit", H, D, bf16=True)
    fails, worst = [], {}
    want = scale = None
    for form, (rg, pack) in graphs.items():
        got, (el, er) = _run(rg, pack, inp, p, _seed(DR.SEEDS[p]), bf16=True)
        assert got["out"].dtype == got["g_ft"].dtype == torch.bfloat16
        if want is None:
            want, scale = DR.gat_drop_case_ref(rg.csr_ptr, rg.csr_idx, pack.rel_csr, el, er,
                                               inp[3], inp[0], inp[4], inp[5], w)
        _compare(f"bf16 {form}", got, want, scale, fails, worst, bf16=True)
    print(f"attn_drop parity bf16 rows p={p}: " +
          " ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())))
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("H,D", [(8, 64), (2, 32)])
def test_keep_everything_is_the_undropped_operator(graphs, H, D):
    """2: keep16 = 65536 keeps every edge with a scale of 1.0: bitwise ops.gat_fused without
    dropout, output and every gradient, in both score forms"""
    for kind in ("unit", "elx"):
        inp = _inputs(kind, H, D)
        for form, (rg, pack) in graphs.items():
            plain, _ = _run(rg, pack, inp, 0.0, None, elx=kind == "elx")
            kept, _ = _run(rg, pack, inp, None, None, elx=kind == "elx",
                           drop=(_seed(DR.SEEDS[0.5]), 65536, 1.0))
            for name in NAMES:
                assert torch.equal(plain[name], kept[name]), f"{kind} {form} {name}"


def test_seed_is_read_on_the_device(graphs):
    """3: the seed tensor overwritten in place draws another mask; each run matches the
    restatement of its own seed; two runs on one seed return the same bits"""
    H, D, p = 8, 64, 0.6
    rg, pack = graphs["default"]
    inp = _inputs("elx", H, D)
    s1, s2 = DR.SEEDS[0.6], DR.SEEDS[0.2]
    seed = _seed(s1)
    runs = [_run(rg, pack, inp, p, seed, elx=True)]
    seed.fill_(s2)
    runs.append(_run(rg, pack, inp, p, seed, elx=True))
    runs.append(_run(rg, pack, inp, p, seed, elx=True))
    assert not torch.equal(runs[0][0]["out"], runs[1][0]["out"])
    for name in NAMES:
        assert torch.equal(runs[1][0][name], runs[2][0][name]), name
    fails = []
    for s, (got, (el, er)) in zip((s1, s2), runs):
        w = DR.drop_weight(s, rg.E, H, p).to(DEV)
        want, scale = DR.gat_drop_case_ref(rg.csr_ptr, rg.csr_idx, pack.rel_csr, el, er, inp[3],
                                           inp[0], inp[4], inp[5], w)
        _compare(f"seed {s:#x}", got, want, scale, fails, {})
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("H,D", [(8, 64), (2, 32), (32, 4)])
def test_mask_does_not_depend_on_the_plan(graphs, H, D):
    """4: one seed in the three plan forms: the same mask, so the outputs differ by the summation
    order alone, <= 2e-5 of each other under the metric (two kernels' bounds)"""
    p = 0.6
    inp = _inputs("unit", H, D)
    w = DR.drop_weight(DR.SEEDS[p], graphs["default"][0].E, H, p).to(DEV)
    outs, scale = {}, None
    for form, (rg, pack) in graphs.items():
        outs[form], (el, er) = _run(rg, pack, inp, p, _seed(DR.SEEDS[p]))
        if scale is None:
            _, scale = DR.gat_drop_case_ref(rg.csr_ptr, rg.csr_idx, pack.rel_csr, el, er, inp[3],
                                            inp[0], inp[4], inp[5], w)
    for a, b in (("default", "tree"), ("default", "noplan"), ("tree", "noplan")):
        for name in NAMES:
            err = AR.rel_err(outs[a][name], outs[b][name].double(), scale[name])
            assert err <= 2e-5, f"{a} vs {b} {name}: {err:.3e}"


# ---- layer ---------------------------------------------------------------------------------------
def _layer(name, attn_drop):
    import dgl
    from layer import REGATConv
    d = G.load(name)
    m = d["meta"]
    g = dgl.DGLGraph((d["g_src"], d["g_dst"]), num_nodes=int(d["g_N"])).to(DEV)
    mod = REGATConv(int(d["g_R"]), m["alpha"], m["in_feats"], m["out_feats"], m["num_heads"], 0.0,
                    attn_drop, m["negative_slope"], m["residual"],
                    F.elu if m["activation"] else None, use_weight=m["use_weight"])
    P = G.sub(d, "p_", np.float32)
    with torch.no_grad():
        for n, q in mod.named_parameters():
            q.copy_(torch.from_numpy(P[n]))
    return d, m, g, mod.to(DEV), torch.from_numpy(d["g_rel"]).to(DEV)


def _layer_ref(d, m, rg, rel_csr, w, mod):
    """fp64 restatement of REGATConv.forward in train mode with the attention weights w"""
    P = {n: q.detach().double().clone().requires_grad_(True) for n, q in mod.named_parameters()}
    x = torch.from_numpy(d["feat"]).to(DEV).double().requires_grad_(True)
    H, D = m["num_heads"], m["out_feats"]
    ft = (x @ P["fc.weight"].T).view(-1, H, D)
    el, er = (ft * P["attn_l"]).sum(-1), (ft * P["attn_r"]).sum(-1)
    tab = F.leaky_relu(P["edge_weight"] * m["alpha"], 0.01)
    out = DR.gat_drop_reference(rg.csr_ptr, rg.csr_idx, rel_csr, el, er, tab, ft,
                                m["negative_slope"], w)
    if m["residual"]:
        out = out + (x @ P["res_fc.weight"].T).view(-1, H, D)
    if m["activation"]:
        out = F.elu(out)
    out.backward(torch.from_numpy(d["gout"]).to(DEV).double())
    return out.detach(), x.grad, {n: q.grad for n, q in P.items()}


@pytest.mark.parametrize("name", ["regatconv_h4_ee", "regatconv_h8_d64_ee_res_elu"])
def test_layer_train_mode_matches_masked_restatement(fused_mode, name):
    """5: layer.REGATConv in train() with attn_drop = 0.6 and the knob at "fused" draws the mask of
    seed base + 1, base as drop_request draws it; output, input and parameter gradients <= 1e-5 (G.close)"""
    from regnn_hip import ops
    p = 0.6
    d, m, g, mod, e_feat = _layer(name, p)
    ops._DROP_CTR.clear()
    torch.manual_seed(5)
    base = int(torch.randint(1, 2 ** 62, (1,)).item())
    ops._DROP_CTR.clear()
    torch.manual_seed(5)
    mod.train()
    x = torch.from_numpy(d["feat"]).to(DEV).requires_grad_(True)
    y = mod(g, x, e_feat)
    y.backward(torch.from_numpy(d["gout"]).to(DEV))
    rg = g.relgraph(DEV)
    pack = rg.rel_pack(e_feat, num_rel=int(d["g_R"]))
    w = DR.drop_weight(base + 1, rg.E, m["num_heads"], p).to(DEV)
    want, want_gx, want_gp = _layer_ref(d, m, rg, pack.rel_csr, w, mod)
    pairs = [("out", y, want), ("grad_feat", x.grad, want_gx)]
    pairs += [(n, q.grad, want_gp[n]) for n, q in mod.named_parameters()]
    for tag, a, b in pairs:
        ok, err = G.close(a.detach().cpu().numpy(), b.cpu().numpy(), 1e-5)
        assert ok, f"{tag}: rel err {err:.3e}"
    assert not torch.equal(y, mod(g, x, e_feat))             # a fresh mask per call


def test_layer_eval_and_torch_mode_unchanged(fused_mode):
    """5: eval() is ops.gat_fused without dropout, bitwise; ATTN_DROP "fused" does not run the
    unfused attention and "torch" takes the gat_attention -> nn.Dropout -> head_spmm path"""
    from regnn_hip import ops
    d, m, g, mod, e_feat = _layer("regatconv_h4_ee", 0.6)
    x = torch.from_numpy(d["feat"]).to(DEV)
    rg = g.relgraph(DEV)
    pack = rg.rel_pack(e_feat, num_rel=int(d["g_R"]))
    mod.eval()
    with torch.no_grad():
        ft = mod.fc(x).view(-1, m["num_heads"], m["out_feats"])
        el, er = ops.attn_dots(ft, mod.attn_l, mod.attn_r)
        tab = F.leaky_relu(mod.edge_weight * m["alpha"], 0.01)
        want = ops.gat_fused(rg, el, er, ft, tab, pack, m["negative_slope"], attn_l=mod.attn_l)
        assert torch.equal(mod(g, x, e_feat), want)
    mod.train()
    calls = []
    orig = ops.gat_attention
    ops.gat_attention = lambda *a, **k: calls.append(1) or orig(*a, **k)
    try:
        mod(g, x, e_feat)
        assert not calls, "the fused mode ran the unfused attention"
        ops.ATTN_DROP["mode"] = "torch"
        y = mod(g, x, e_feat)
        assert calls == [1] and bool(torch.isfinite(y).all())
    finally:
        ops.gat_attention = orig
        ops.ATTN_DROP["mode"] = "fused"       # the fixture restores the default


# ---- model ---------------------------------------------------------------------------------------
def test_model_training_step_repeats_from_its_seeds(fused_mode):
    """6: nets.REGAT (heads [2, 2, 1], hidden 8) in train() with attn_drop = 0.5, fused, on a
    mag-shaped graph of a few thousand nodes: two passes under identical seeds give the same bits,
    loss and every gradient"""
    import dgl
    from regnn_hip import nets, ops, synth
    gd = synth.mag_like(0.002, seed=0, device=DEV)
    g = dgl.DGLGraph((gd["src"], gd["dst"]), num_nodes=gd["N"])
    e_feat = gd["rel"].to(torch.int64)
    gen = torch.Generator(device=DEV).manual_seed(1)
    dims = [16, 8, 8, 8][:len(gd["counts"])]
    feats = [torch.randn(n, k, generator=gen, device=DEV)
             for n, k in zip(gd["counts"].values(), dims)]
    labels = torch.randint(0, 4, (gd["N"],), generator=gen, device=DEV)
    torch.manual_seed(0)
    net = nets.REGAT(g, gd["R"], 100.0, 2, 8, 8, 4, [2, 2, 1], F.elu, 0.0, 0.5, 0.01, False,
                     dims).to(DEV).train()
    runs = []
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        ops._DROP_CTR.clear()
        torch.manual_seed(7)
        logits, _ = net(feats, e_feat)
        loss = F.cross_entropy(logits, labels)
        loss.backward()
        runs.append((loss.detach().clone(),
                     {n: q.grad.clone() for n, q in net.named_parameters()}))
    assert bool(torch.isfinite(runs[0][0]))
    assert torch.equal(runs[0][0], runs[1][0])
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n
    net.zero_grad(set_to_none=True)
    logits, _ = net(feats, e_feat)                    # the counter moved on: another mask
    assert not torch.equal(F.cross_entropy(logits, labels), runs[0][0])


# ---- generic head counts -------------------------------------------------------------------------
def test_generic_head_count_runs_the_unfused_path(graphs):
    """7: H = 3 is no shape of the fused kernels: ops.gat_fused(attn_drop > 0) runs
    head_spmm(dropout(gat_attention)) on torch's stream, without an error"""
    from regnn_hip import ops
    rg, pack = graphs["default"]
    ft, el, er, tab, gy, slope = _inputs("unit", 3, 4)
    torch.manual_seed(3)
    y = ops.gat_fused(rg, el, er, ft, tab, pack, slope, attn_drop=0.5)
    torch.manual_seed(3)
    a = ops.gat_attention(rg, el, er, tab, pack, slope)
    want = ops.head_spmm(rg, F.dropout(a, 0.5, True), ft)
    assert torch.equal(y, want)
    assert not torch.equal(y, ops.gat_fused(rg, el, er, ft, tab, pack, slope))
