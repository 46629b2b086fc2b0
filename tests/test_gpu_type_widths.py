"""One input width per node type (feats_type 5 of mag/regnn_ns.py:185-194: paper rows 256 wide,
the other types 128) on the module path's device blocks:

1. ops.ns_typed_agg over mixed widths (regnn_ns_typed_agg_kt / _bwd) per element against fp64
   sums on a hand-built padded block, both hop forms, ext on and off;
2. the _kt entries at equal widths against regnn_ns_typed_agg (the same bits forward);
3. ops.typed_linear over mixed widths (regnn_typed_linear_fwd_kt / _wgrad_kt) against fp64 and,
   per type, against the equal-width launch on that type alone (the same bits);
4. one NSTrainer(engine="module") step through the typed first layer against the reference order
   (group_input first) on the same batch;
5. the step pipelined and captured against eager unpipelined steps, bitwise;
6. the reference-generated fixture mag_regnn_ft5_h128 now runs the typed first layer over a
   meta-only hop.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _golden as G  # noqa: E402
import _ns_gat_blocks as B  # noqa: E402

DEV = "cuda"
# row lengths around the 16 / 32 / 64 lanes-per-row groups of the three widths, one row longer than
# two 64-entry passes, an EMPTY live row first; capacity rows (empty) follow
LENS = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130]
ROW_ONE_TYPE, ROWS_ALL_TYPES = 3, (5, 12)
CAP_DST, CAP_SRC, LIVE_SRC, N_REL = 24, 320, 120, 11
COUNTS = [90, 70, 60, 50]                      # nodes per type
WIDTHS = [(256, 128, 128, 128), (64, 256, 128), (128, 64), (256, 256)]


@functools.lru_cache(maxsize=None)
def _block(T, seed=5):
    """a padded block (tests/_ns_gat_blocks.py's layout) over T node types with its own n_id /
    node type / local row tables, and the same edges' per-edge source type / table row."""
    rng = np.random.default_rng(seed)
    counts = COUNTS[:T]
    ntype = np.concatenate([np.full(c, t, dtype=np.int64) for t, c in enumerate(counts)])
    local = np.concatenate([np.arange(c, dtype=np.int64) for c in counts])
    n_id = rng.permutation(ntype.size)[:LIVE_SRC]
    src_type = ntype[n_id]
    by_type = [np.flatnonzero(src_type == t) for t in range(T)]
    assert all(len(b) > 0 for b in by_type)
    idx, rel = [], []
    for v, n in enumerate(LENS):
        row = rng.integers(0, LIVE_SRC, n)
        if v == ROW_ONE_TYPE:
            row = rng.choice(by_type[T - 1], n)
        if v in ROWS_ALL_TYPES:
            row[:T] = [b[v % len(b)] for b in by_type]
        idx += row.tolist()
        rel += rng.integers(0, N_REL, n).tolist()
    ptr = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    idx, rel = np.asarray(idx, dtype=np.int64), np.asarray(rel, dtype=np.int64)
    assert len(set(src_type[idx[ptr[ROW_ONE_TYPE]:ptr[ROW_ONE_TYPE + 1]]])) == 1
    for v in ROWS_ALL_TYPES:
        assert len(set(src_type[idx[ptr[v]:ptr[v + 1]]])) == T
    blk = B._pad(ptr, idx, rel, CAP_DST, CAP_SRC)
    cap_e = blk.csr_idx.numel()
    e_type = np.zeros(cap_e, dtype=np.int32)
    e_off = np.zeros(cap_e, dtype=np.int64)
    e_type[:idx.size] = src_type[idx]
    e_off[:idx.size] = local[n_id[idx]]
    nid = np.zeros(CAP_SRC, dtype=np.int64)
    nid[:LIVE_SRC] = n_id
    return dict(blk=blk, ptr=ptr, idx=idx, rel=rel, n_id=nid, ntype=ntype, local=local,
                e_type=e_type, e_off=e_off, counts=counts)


def _dev_block(b, meta):
    blk = b["blk"].to(DEV)
    if meta:
        blk.edge_meta = (torch.from_numpy(b["e_type"]).to(DEV), torch.from_numpy(b["e_off"]).to(DEV))
    return blk


@functools.lru_cache(maxsize=None)
def _tables(widths):
    g = torch.Generator().manual_seed(sum(widths) + len(widths))
    return tuple(torch.randn(c, k, generator=g) for c, k in zip(COUNTS, widths))


@functools.lru_cache(maxsize=None)
def _agg_case(widths):
    """(gS, gw, S64, w64, d rw in fp64) of one width set: the fp64 sums over the block's live
    rows and autograd's relation-weight gradient, formed once."""
    T, SK = len(widths), sum(widths)
    b = _block(T)
    g = torch.Generator().manual_seed(17)
    gS = torch.randn(CAP_DST, SK, generator=g)
    gw = torch.randn(CAP_DST, T, generator=g)
    n = len(LENS)
    rw64 = _rw().double().requires_grad_(True)
    tab64 = torch.nn.functional.leaky_relu(rw64 * 10.0)
    dst = torch.from_numpy(np.repeat(np.arange(n), LENS))
    gsrc = b["n_id"][b["idx"]]
    e_t = torch.from_numpy(b["ntype"][gsrc])
    e_row = torch.from_numpy(b["local"][gsrc])
    wt = tab64[torch.from_numpy(b["rel"])]
    parts, wparts = [], []
    for t, K in enumerate(widths):
        m = e_t == t
        X = _tables(widths)[t].double()[e_row[m]]
        parts.append(torch.zeros(n, K, dtype=torch.float64).index_add(0, dst[m], wt[m, None] * X))
        wparts.append(torch.zeros(n, dtype=torch.float64).index_add(0, dst[m], wt[m]))
    S64, w64 = torch.cat(parts, 1), torch.stack(wparts, 1)
    ((S64 * gS[:n].double()).sum() + (w64 * gw[:n].double()).sum()).backward()
    return gS, gw, S64.detach().numpy(), w64.detach().numpy(), rw64.grad.numpy()


def _rw():
    return torch.linspace(-0.05, 0.2, N_REL)


def _run_agg(widths, meta, ext):
    """ops.ns_typed_agg and its relation-weight gradient: (S, w, pad columns or None, d rw)"""
    from regnn_hip import ops
    T, SK = len(widths), sum(widths)
    b = _block(T)
    gS, gw = _agg_case(widths)[:2]
    tables = [t.to(DEV) for t in _tables(widths)]
    assert ops.ns_typed_agg_ok(tables)
    rw = _rw().to(DEV).requires_grad_(True)
    tab = torch.nn.functional.leaky_relu(rw * 10.0)
    out = ops.ns_typed_agg(_dev_block(b, meta), tab, torch.from_numpy(b["n_id"]).to(DEV), tables,
                           torch.from_numpy(b["ntype"]).to(DEV),
                           torch.from_numpy(b["local"]).to(DEV), ext=ext)
    if ext:
        Tp = (T + 3) // 4 * 4
        assert out.shape == (CAP_DST, SK + Tp)
        g = torch.cat([gS, gw, torch.randn(CAP_DST, Tp - T)], 1).to(DEV)   # the pad's gradient
        (out * g).sum().backward()                                         # reaches nothing
        S, w, pad = out[:, :SK], out[:, SK:SK + T], out[:, SK + T:]
    else:
        S, w = out
        assert S.shape == (CAP_DST, SK) and w.shape == (CAP_DST, T)
        ((S * gS.to(DEV)).sum() + (w * gw.to(DEV)).sum()).backward()
        pad = None
    torch.cuda.synchronize()
    return S.detach(), w.detach(), pad, rw.grad.clone()


# ---------------------------------------------------------------------------------------------
# 1. ns_typed_agg at mixed widths, per element against fp64
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: "x".join(map(str, w)))
def test_typed_agg_mixed_widths_against_fp64(widths):
    _, _, S64, w64, g64 = _agg_case(widths)
    n = len(LENS)
    S, w, _, g = _run_agg(widths, meta=False, ext=False)
    for tag, got, want in [("S", S[:n], S64), ("w", w[:n], w64), ("d rel weight", g, g64)]:
        ok, err = G.close(got.cpu().numpy(), want, 1e-5)
        print(f"{widths} {tag}: rel err {err:.3e}")
        assert ok, f"{tag}: rel err {err:.3e}"
    assert g.abs().max() > 0
    # empty rows (the live row of length 0 and the capacity rows) are exact zeros
    assert not S[0].any() and not w[0].any() and not S[n:].any() and not w[n:].any()
    for meta in (False, True):
        for ext in (False, True):
            if not meta and not ext:
                continue
            S2, w2, pad, g2 = _run_agg(widths, meta=meta, ext=ext)
            assert torch.equal(S2, S) and torch.equal(w2, w), (meta, ext)
            assert torch.equal(g2, g), (meta, ext)
            if ext:
                assert pad.shape[1] == (-len(widths)) % 4 and not pad.any()


def test_typed_agg_ok_on_device_tables():
    """ops.ns_typed_agg_ok with device tables (its shape half runs without a GPU in
    tests/test_cpu_type_widths.py)"""
    from regnn_hip import ops
    mk = lambda ws, dt=torch.float32: [torch.zeros(8, k, dtype=dt, device=DEV) for k in ws]  # noqa: E731
    for ws in ((256, 128, 128, 128), (64, 256, 128), (128, 64)):
        assert ops.ns_typed_agg_ok(mk(ws)) and ops.ns_typed_agg_ok(mk(ws), pre_sums=True)
    for ws in ((256, 96, 128, 128), (512, 128)):
        assert not ops.ns_typed_agg_ok(mk(ws))
    bf = torch.bfloat16
    assert not ops.ns_typed_agg_ok(mk((256, 128, 128, 128), bf), pre_sums=True)
    assert ops.ns_typed_agg_ok(mk((128,) * 4, bf), pre_sums=True)
    assert not ops.ns_typed_agg_ok(mk((256,)) + mk((128,), bf), pre_sums=True)
    assert not ops.ns_typed_agg_ok([t[:, 4:] for t in mk((260, 132))])       # not contiguous


# ---------------------------------------------------------------------------------------------
# 2. equal widths through the _kt entries
# ---------------------------------------------------------------------------------------------
def _c_agg(kt, b, meta, tables, K, tab, gS=None, gw=None):
    """regnn_ns_typed_agg(_kt) or, with gS / gw, its backward (reduced), called directly."""
    from regnn_hip import _lib as L, ops
    T = len(tables)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, torch.int32)  # noqa: E731
    blk = b["blk"].to(DEV)
    keep = [i32(b["n_id"]), i32(b["ntype"]), torch.from_numpy(b["local"]).to(DEV),
            i32(b["e_type"]), torch.from_numpy(b["e_off"]).to(DEV)]
    hop = ([None, None, None, L.ptr(keep[3]), L.ptr(keep[4])] if meta else
           [L.ptr(keep[0]), L.ptr(keep[1]), L.ptr(keep[2]), None, None])
    idx = None if meta else L.ptr(blk.csr_idx)
    arr = ops._ptr_array([L.ptr(t) for t in tables])
    width = (ctypes.c_int32 * T)(*[K] * T) if kt else K
    sfx = "_kt" if kt else ""
    if gS is None:
        S = torch.full((CAP_DST, T * K), 7.0, device=DEV)
        w = torch.full((CAP_DST, T), 7.0, device=DEV)
        L.call("regnn_ns_typed_agg" + sfx, L.ptr(blk.csr_ptr), idx, L.ptr(blk.rel), L.ptr(tab),
               *hop, arr, T, width, CAP_DST, L.ptr(S), L.ptr(w), T * K, T, L.stream())
        torch.cuda.synchronize()
        return S, w
    rows = L.slab_rows()
    slab = torch.empty(rows, N_REL, device=DEV)
    L.call(f"regnn_ns_typed_agg{sfx}_bwd", L.ptr(blk.csr_ptr), idx, L.ptr(blk.rel), *hop, arr, T,
           width, CAP_DST, L.ptr(gS), L.ptr(gw), T * K, T, L.ptr(slab), N_REL, rows, L.stream())
    out = ops._reduce(slab, N_REL)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("K", [64, 128])
def test_kt_entry_at_equal_widths_gives_the_equal_width_bits(K):
    T = 4
    b = _block(T)
    tables = [t.to(DEV) for t in _tables((K,) * T)]
    tab = torch.nn.functional.leaky_relu(_rw() * 10.0).to(DEV)
    g = torch.Generator().manual_seed(K)
    gS = torch.randn(CAP_DST, T * K, generator=g).to(DEV)
    gw = torch.randn(CAP_DST, T, generator=g).to(DEV)
    for meta in (False, True):
        S0, w0 = _c_agg(False, b, meta, tables, K, tab)
        S1, w1 = _c_agg(True, b, meta, tables, K, tab)
        assert torch.equal(S1, S0) and torch.equal(w1, w0), meta
        assert S0[1:len(LENS)].abs().max() > 0
        g0 = _c_agg(False, b, meta, tables, K, tab, gS, gw)
        g1 = _c_agg(True, b, meta, tables, K, tab, gS, gw)
        g2 = _c_agg(True, b, meta, tables, K, tab, gS, gw)
        ok, err = G.close(g1.cpu().numpy(), g0.cpu().numpy(), 1e-5)
        print(f"K {K} meta {meta} bwd vs equal-width entry: rel err {err:.3e}")
        assert ok, err
        assert torch.equal(g1, g2)


# ---------------------------------------------------------------------------------------------
# 3. typed_linear at mixed widths
# ---------------------------------------------------------------------------------------------
def _close(a, b, tol):
    """tests/test_gpu_typed.py's bound: max |a - b| within tol of max(1, max |b|)"""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err = (a - b).abs().max().item() / max(1.0, b.abs().max().item())
    assert err <= tol, f"rel err {err:.3e} > {tol}"


# picked rows per type: none; one forward chunk and a row (65 at width 256, whose chunks hold 64
# rows; 129 at the others' 128); a run across a 1024-row wgrad chunk
@pytest.mark.parametrize("O", [64, 128])
@pytest.mark.parametrize("widths,picks", [((256, 128, 128, 128), (65, 129, 1025, 0)),
                                          ((64, 256, 128), (0, 1025, 129))],
                         ids=["256x128x128x128", "64x256x128"])
def test_typed_linear_mixed_widths(widths, picks, O):
    from regnn_hip import ops
    T = len(widths)
    torch.manual_seed(sum(widths) + O)
    counts = [max(p, 1) + 40 for p in picks]
    ntype = torch.cat([torch.full((c,), t, dtype=torch.int64) for t, c in enumerate(counts)])
    local = torch.cat([torch.arange(c, dtype=torch.int64) for c in counts])
    offs = np.concatenate([[0], np.cumsum(counts)])
    ids = torch.cat([int(offs[t]) + torch.randperm(counts[t])[:p] for t, p in enumerate(picks)])
    n_id = ids[torch.randperm(ids.numel())].to(DEV)
    ntype, local = ntype.to(DEV), local.to(DEV)
    tabs = [torch.randn(c, k, device=DEV) for c, k in zip(counts, widths)]
    Ws = [torch.randn(O, k, device=DEV, requires_grad=True) for k in widths]
    bs = [torch.randn(O, device=DEV, requires_grad=True) for _ in widths]
    assert ops.typed_linear_fusable(tabs, Ws, bs)
    gy = torch.randn(n_id.numel(), O, device=DEV)
    runs = []
    for _ in range(2):
        for p in Ws + bs:
            p.grad = None
        y = ops.typed_linear(tabs, Ws, bs, ntype, local, n_id)
        y.backward(gy)
        runs.append([y.detach().clone()] + [p.grad.clone() for p in Ws + bs])
    for a, c in zip(*runs):
        assert torch.equal(a, c)
    y = runs[0][0]
    nt, li = ntype[n_id].cpu(), local[n_id].cpu()
    for t in range(T):
        m = nt == t
        assert int(m.sum()) == picks[t]
        X = tabs[t].cpu().double()[li[m]]
        Gm = gy.cpu().double()[m]
        _close(Ws[t].grad, Gm.T @ X, 1e-5)                # (a type without rows: zeros)
        _close(bs[t].grad, Gm.sum(0), 1e-5)
        if not picks[t]:
            continue
        _close(y[m.to(DEV)], X @ Ws[t].detach().cpu().double().T + bs[t].detach().cpu().double(),
               1e-5)
        # the equal-width launch over this type's rows alone: the same bits per row
        one = ops.typed_linear([tabs[t]], [Ws[t].detach()], [bs[t].detach()],
                               torch.zeros_like(ntype), local, n_id[m.to(DEV)])
        assert torch.equal(y[m.to(DEV)], one)


# ---------------------------------------------------------------------------------------------
# 4. / 5. the model on the module path
# ---------------------------------------------------------------------------------------------
MAG_WIDTHS = (256, 128, 128, 128)


@functools.lru_cache(maxsize=None)
def _mag_widths(scale=0.003, seed=2):
    from regnn_hip import synth
    from test_gpu_ns_engine import _mag
    d = _mag(scale, seed=seed, F=128, classes=13)
    feats = synth.type_features(d["gd"]["counts"], dict(zip(synth.NTYPES, MAG_WIDTHS)), seed=1,
                                device=DEV)
    return dict(d, x_dict={k: f for k, f in enumerate(feats)})


def _model(hidden, residual, dropout=0.0, seed=7):
    from regnn_hip import mag
    torch.manual_seed(seed)
    m = mag.REGNN(128, hidden, 13, 2, 10.0, dropout, dict(enumerate(MAG_WIDTHS)), 7,
                  use_norm="ln", self_loop_type=2, residual=residual).to(DEV)
    with torch.no_grad():
        for conv in m.convs:
            conv.relation_weight.copy_(torch.linspace(-0.02, 0.12, conv.relation_weight.numel(),
                                                        device=DEV))
            conv.bias.normal_(0, 0.1)
    return m.train()


def _trainer(d, m, opt, **kw):
    from regnn_hip.ns import NSTrainer
    return NSTrainer(m, opt, d["rg"], [6, 4], 96, torch.arange(d["n_paper"], device=DEV),
                     d["x_dict"], d["edge_type"], d["node_type"], d["local"], d["y"], 7, **kw)


def _grads_one_step(d, hidden, residual, typed):
    """tests/test_gpu_ns_typed.py's recipe: one module-engine step with mag.TYPED_AGG "auto"
    (the typed first layer) or "off" (group_input over every sampled row, then the convs)."""
    from regnn_hip import mag, ops
    old, old_csc = mag.TYPED_AGG["mode"], ops.NS_CSC["mode"]
    mag.TYPED_AGG["mode"] = ops.NS_CSC["mode"] = "auto" if typed else "off"
    try:
        m = _model(hidden, residual)
        tr = _trainer(d, m, torch.optim.SGD(m.parameters(), lr=0.0), seed=3, engine="module")
        assert tr.fused is None and tr._module_lean == typed
        seen = []
        orig = m._typed_first_layer

        def spy(*a, **k):
            out = orig(*a, **k)
            seen.append(out is not None)
            return out
        m._typed_first_layer = spy
        tr._forward_backward()
        torch.cuda.synchronize()
        assert seen == [typed]
        return float(tr.loss), {n: p.grad.detach().double().cpu().numpy().copy()
                                for n, p in m.named_parameters()}
    finally:
        mag.TYPED_AGG["mode"], ops.NS_CSC["mode"] = old, old_csc


@pytest.mark.parametrize("hidden,residual", [(128, True), (512, False)])
def test_typed_first_layer_mixed_widths_matches_reference_order(hidden, residual):
    d = _mag_widths()
    la, ga = _grads_one_step(d, hidden, residual, True)
    lb, gb = _grads_one_step(d, hidden, residual, False)
    print(f"hidden {hidden}: loss {la!r} vs {lb!r}")
    assert abs(la - lb) <= 1e-5 * max(1.0, abs(lb)), (la, lb)
    for n in gb:
        ok, err = G.close(ga[n], gb[n], 1e-5)
        print(f"hidden {hidden} grad {n}: rel err {err:.3e}")
        assert ok, f"{n}: rel err {err:.3e}"
    assert np.abs(ga["convs.0.relation_weight"]).max() > 0


@functools.lru_cache(maxsize=None)
def _captured_and_eager():
    """one pipelined trainer captured and replayed for 4 steps and one eager unpipelined trainer
    stepped 4 times from the same seed (tests/test_gpu_ns_bf16.py's recipe), run once for the two
    tests below. Hidden 128 with residual; ops.SMALL_BLAS is switched off for the run, so the
    small products take the x6 GEMM and not hipBLASLt, which may pick another algorithm under
    capture (tests/test_gpu_ns_engine.py); a sampling lookahead of 1 keeps the capture short."""
    from regnn_hip import ns, ops
    knobs = [(ops.SMALL_BLAS, "mode", "off"), (ns.MODULE_PIPELINE, "mode", "on"),
             (ns.MODULE_AHEAD, "n", 1)]
    old = [(d_, k, d_[k]) for d_, k, _ in knobs]
    for d_, k, v in knobs:
        d_[k] = v
    try:
        d = _mag_widths()

        def make(pipe):
            return _trainer(d, _model(128, True, seed=5), None, seed=9, adam=dict(lr=1e-2),
                            engine="module", pipeline=pipe)
        tr_p, tr_u = make(True), make(False)
        assert tr_p.fused is None and tr_p._module_lean and tr_u._module_lean
        assert tr_p.pipelined and not tr_u.pipelined
        tr_p.capture(warmup=2)                          # warm-up steps undone by capture()
        tr_p.run_steps(4)
        for _ in range(4):
            tr_u.step()
        torch.cuda.synchronize()
        same_batch = torch.equal(tr_p.sampler.n_id[:int(tr_p.sampler.sizes[0])],
                                 tr_u.sampler.n_id[:int(tr_u.sampler.sizes[0])])
        return (same_batch, float(tr_p.loss), float(tr_u.loss), tr_p.param_vector().clone(),
                tr_u.param_vector().clone())
    finally:
        for d_, k, v in old:
            d_[k] = v


def test_mixed_widths_step_captures_and_tracks_eager():
    """no host sync on the step: capture() succeeds (on the mask loop it raised), the replays
    train the eager trainer's batches, and the loss after 4 steps agrees within the bound
    tests/test_gpu_ns_engine.py::test_pipelined_trainer_matches_unpipelined holds the module
    path to (5e-5: ulp-level differences of the step that Adam carries forward)."""
    same_batch, lp, lu, pp, pu = _captured_and_eager()
    assert same_batch
    print(f"loss captured {lp!r} eager {lu!r}; max |d param| {float((pp - pu).abs().max()):.3e}")
    assert np.isfinite(lp) and np.allclose(lp, lu, rtol=5e-5, atol=5e-6), (lp, lu)
    assert bool(torch.isfinite(pp).all())


def test_mixed_widths_pipelined_captured_matches_eager():
    """4 replayed pipelined steps end at the parameters of 4 eager unpipelined steps, BITWISE.

    This needs the module path's step to give the same bits on every run of a batch. It did not,
    with equal widths either: hop 0's transposed index places a source's entries in the order an
    integer atomic cursor hands out, and the last layer's backward (regnn_ns_spmm_bwd_csc) sums
    floats in entry order, so two eager trainers from one seed differed in the last bits of
    lins.*, convs.0.* and convs.1.relation_weight (~1e-7 relative after one forward / backward,
    ~1e-6 in the parameters after four Adam steps). The sampler now sorts every segment of that
    index (regnn_ns_csc_sort, test_csc_sort_orders_every_segment)."""
    same_batch, lp, lu, pp, pu = _captured_and_eager()
    assert same_batch
    print(f"loss captured {lp!r} eager {lu!r}; max |d param| {float((pp - pu).abs().max()):.3e}")
    assert np.isfinite(lp) and np.allclose(lp, lu, rtol=1e-6, atol=1e-7), (lp, lu)
    assert bool(torch.isfinite(pp).all())
    assert torch.equal(pp, pu)


def test_csc_sort_orders_every_segment():
    """regnn_ns_csc_sort against torch.sort per segment: segments of 0, 1, 2, 63, 64, 65 and 700
    entries (the shuffle form up to 64, the pass form above), duplicates, a live count below the
    capacity (sources past it untouched)."""
    from regnn_hip import _lib as L
    g = torch.Generator().manual_seed(3)
    lens = [0, 1, 2, 63, 64, 65, 700, 5, 0, 17]
    live = len(lens) - 1                                      # the last segment is not live
    ptr = torch.tensor([0] + np.cumsum(lens).tolist(), dtype=torch.int32)
    E = int(ptr[-1])
    ent = torch.randint(0, 1 << 20, (E,), generator=g, dtype=torch.int32)
    ent[200:260] = ent[200]                                   # equal entries
    sizes = torch.zeros(16, dtype=torch.int32)
    sizes[1] = live
    cap_src = len(lens) + 3
    ptr_d = torch.cat([ptr, torch.full((3,), -7, dtype=torch.int32)]).to(DEV)   # stale tail
    out = torch.full((E,), -1, dtype=torch.int32, device=DEV)
    ent_d = ent.to(DEV)
    L.call("regnn_ns_csc_sort", L.ptr(sizes.to(DEV)), 1, L.ptr(ptr_d), L.ptr(ent_d), L.ptr(out),
           cap_src, E, L.stream())
    torch.cuda.synchronize()
    assert torch.equal(ent_d.cpu(), ent)                      # the source is left alone
    got = out.cpu()
    for u, n in enumerate(lens):
        seg = slice(int(ptr[u]), int(ptr[u + 1]))
        want = torch.sort(ent[seg]).values if u < live else torch.full((n,), -1, dtype=torch.int32)
        assert torch.equal(got[seg], want), u


# ---------------------------------------------------------------------------------------------
# 6. the reference fixture takes the new path
# ---------------------------------------------------------------------------------------------
def test_ft5_fixture_runs_the_typed_first_layer():
    """tests/test_gpu_regnn_golden.py::test_regnn_module_step_ft5_vs_reference[on] checks this
    trainer's loss and gradients against the reference's: with unequal widths on the device path
    it does so through the typed first layer over a meta-only last hop."""
    from regnn_hip.graph import RelGraph
    from regnn_hip.ns import NSTrainer
    from test_gpu_regnn_golden import _inputs, _model as golden_model
    d = G.load("mag_regnn_ft5_h128")
    m = d["meta"]
    assert len(set(m["feature_dims"])) > 1
    rg = RelGraph(torch.from_numpy(d["src"]), torch.from_numpy(d["dst"]), int(sum(m["counts"])),
                  DEV)
    model = golden_model(d)
    x_dict, _, et, nt, loc = _inputs(d)
    batch = torch.from_numpy(d["batch"]).to(DEV)
    tr = NSTrainer(model, None, rg, m["sizes"], batch.numel(), batch, x_dict, et, nt, loc,
                   torch.from_numpy(d["y"]).to(DEV).reshape(-1, 1), m["num_edge_types"],
                   seed=m["seed"], engine="auto", pipeline=False)
    assert tr.fused is None and tr._module_lean is True
    assert tr.slots[0].blocks[-1].meta_only and tr.slots[0].blocks[-1].edge_meta is not None
    assert getattr(tr.slots[0].blocks[-1], "pre_sums", None) is None     # no sums at mixed widths
