"""bf16 input tables on every model path (ops.BF16_ROWS "on"): the gather-fused per-type Linear and
layer 0's typed aggregation read bf16 rows through the `_dt` entries. The contract is the sums
launch's: widening bf16 to fp32 is exact and nothing after the load differs, so every result is
the fp32 result on the widened tables -- torch.equal for the two operators, and for whole steps
the TOL of tests/test_gpu_ns_bf16.py (zero in exact arithmetic: the bound absorbs a hipBLASLt
algorithm choice that may differ per run). The reference is always the same call on
{k: v.float()}.

1. ops.typed_linear: Y and every weight / bias gradient, bitwise;
2. ops.ns_typed_agg on a padded block: S, w and the relation-table gradient, bitwise;
3. knob off: the refusals of today;
4. NSTrainer's regcn module path with residual convs, and at a fan-out above 63 (64);
5. regat / regatv2 on device blocks, one step and captured replays;
6. the exact-size path (mag.train_step);
7. what stays refused with the knob on.
"""
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
TOL = 1e-5                                     # tests/test_gpu_ns_bf16.py


def _widen(x):
    if isinstance(x, dict):
        return {k: v.float() for k, v in x.items()}
    return [v.float() for v in x]


def _bf16(x_dict):
    return {k: v.bfloat16().contiguous() for k, v in x_dict.items()}


@pytest.fixture
def knob_on(monkeypatch):
    from regnn_hip import ops
    monkeypatch.setitem(ops.BF16_ROWS, "mode", "on")


def _check(tag, got, want, tol=TOL):
    got = got.detach().double().cpu().numpy()
    want = want.detach().double().cpu().numpy()
    ok, err = G.close(got, want, tol)
    print(f"{tag}: rel err {err:.3e}")
    assert ok, f"{tag}: rel err {err:.3e}"


# ---------------------------------------------------------------------------------------------
# 1. typed_linear
# ---------------------------------------------------------------------------------------------
ROWS = 50                                      # rows per table: the sampled rows repeat
# type runs: empty; below one 16-row MFMA tile; a partial forward chunk (128 rows, 64 at width
# 256); past the 1024-row wgrad chunk with its last 32-row step partial (1100 = 1024 + 2 * 32 + 12)
RUNS = (100, 1100, 7, 0)


def _linear_case(widths, O, use_n_id, wgroup=None):
    """ops.typed_linear forward + backward on bf16 tables and on the widened ones"""
    from regnn_hip import ops
    T = len(widths)
    g = torch.Generator().manual_seed(sum(widths) + O + 2 * use_n_id)
    tabs = [torch.randn(ROWS, k, generator=g).bfloat16().to(DEV) for k in widths]
    ntype = torch.arange(T).repeat_interleave(ROWS)                  # per global node
    local = torch.arange(ROWS).repeat(T)
    ids = torch.cat([t * ROWS + torch.randint(0, ROWS, (n,), generator=g)
                     for t, n in enumerate(RUNS[:T])])
    ids = ids[torch.randperm(ids.numel(), generator=g)]
    if use_n_id:
        nt, li, n_id = ntype.to(DEV), local.to(DEV), ids.to(DEV)
    else:
        nt, li, n_id = ntype[ids].to(DEV), local[ids].to(DEV), None   # one entry per row
    wg = list(range(T)) if wgroup is None else wgroup
    gk = {}
    for t, grp in enumerate(wg):
        gk[grp] = widths[t]
    Ws0 = [torch.randn(O, gk[i], generator=g) for i in range(len(gk))]
    bs0 = [torch.randn(O, generator=g) for _ in range(len(gk))]
    gy = torch.randn(ids.numel(), O, generator=g).to(DEV)
    out = []
    for tables in (tabs, _widen(tabs)):
        Ws = [w.clone().to(DEV).requires_grad_(True) for w in Ws0]
        bs = [b.clone().to(DEV).requires_grad_(True) for b in bs0]
        assert ops.typed_linear_fusable(tables, Ws, bs)
        y = ops.typed_linear(tables, Ws, bs, nt, li, n_id, wgroup=wgroup)
        y.backward(gy)
        out.append((y.detach(), [w.grad for w in Ws], [b.grad for b in bs]))
    torch.cuda.synchronize()
    return out


def _assert_linear_equal(out):
    (y, gW, gb), (y0, gW0, gb0) = out
    assert y.shape == (sum(RUNS), y.shape[1]) and bool(y.any())
    assert torch.equal(y, y0)
    for i, (a, b) in enumerate(zip(gW, gW0)):
        assert torch.equal(a, b), f"W[{i}].grad"
    for i, (a, b) in enumerate(zip(gb, gb0)):
        assert torch.equal(a, b), f"bias[{i}].grad"
    # (the last type has no rows: its group's gradients are zeros)
    assert all(bool(a.any()) for a in gW[:-1] + gb[:-1])
    assert not bool(gW[-1].any()) and not bool(gb[-1].any())


@pytest.mark.parametrize("use_n_id", [True, False], ids=["n_id", "rows"])
@pytest.mark.parametrize("O", [64, 128])
@pytest.mark.parametrize("widths", [(128, 128, 128, 128), (256, 128, 64, 128)],
                         ids=lambda w: "x".join(map(str, w)))
def test_typed_linear_bf16_rows_bitwise(knob_on, widths, O, use_n_id):
    _assert_linear_equal(_linear_case(widths, O, use_n_id))


def test_typed_linear_bf16_rows_shared_weight_group(knob_on):
    """types 1 and 2 share one weight and bias: their runs' chunks sum into one gradient"""
    out = _linear_case((128, 128, 128, 128), 64, True, wgroup=[0, 1, 1, 2])
    assert len(out[0][1]) == 3
    _assert_linear_equal(out)


# ---------------------------------------------------------------------------------------------
# 2. ns_typed_agg
# ---------------------------------------------------------------------------------------------
# row degrees 0, 1, LPR - 1, LPR, LPR + 1 and 2 LPR + 3 for LPR = K_max / 4 in {16, 32, 64}: one
# block for every width set; capacity rows (empty) follow
LENS = [0, 1, 15, 16, 17, 35, 31, 32, 33, 67, 63, 64, 65, 131]
CAP_DST, CAP_SRC, LIVE_SRC, N_REL = 24, 320, 160, 11
AGG_WIDTHS = [(128, 128, 128, 128), (256, 128, 128, 64), (64,) * 8]


@functools.lru_cache(maxsize=None)
def _block(T, seed=11):
    """tests/test_gpu_type_widths.py's padded block (tests/_ns_gat_blocks.py's layout) over T
    node types of 40 nodes each: sources drawn from all types (mixed within a row), in both the
    idx / n_id / node type / local row form and the per-edge source type / table row form."""
    rng = np.random.default_rng(seed)
    counts = [40] * T
    ntype = np.repeat(np.arange(T, dtype=np.int64), counts)
    local = np.concatenate([np.arange(c, dtype=np.int64) for c in counts])
    n_id = rng.permutation(ntype.size)[:LIVE_SRC]
    idx = rng.integers(0, LIVE_SRC, sum(LENS)).astype(np.int64)
    rel = rng.integers(0, N_REL, sum(LENS)).astype(np.int64)
    ptr = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    for v in (5, 9, 13):                                 # the long rows hold several types
        assert len(set(ntype[n_id[idx[ptr[v]:ptr[v + 1]]]])) > 1
    blk = B._pad(ptr, idx, rel, CAP_DST, CAP_SRC)
    cap_e = blk.csr_idx.numel()
    e_type, e_off = np.zeros(cap_e, dtype=np.int32), np.zeros(cap_e, dtype=np.int64)
    e_type[:idx.size] = ntype[n_id[idx]]
    e_off[:idx.size] = local[n_id[idx]]
    nid = np.zeros(CAP_SRC, dtype=np.int64)
    nid[:LIVE_SRC] = n_id
    return dict(blk=blk, n_id=nid, ntype=ntype, local=local, e_type=e_type, e_off=e_off)


def _run_agg(b, tables, meta, ext, g_out):
    from regnn_hip import ops
    blk = b["blk"].to(DEV)
    if meta:
        blk.edge_meta = (torch.from_numpy(b["e_type"]).to(DEV),
                         torch.from_numpy(b["e_off"]).to(DEV))
    rw = torch.linspace(-0.05, 0.2, N_REL).to(DEV).requires_grad_(True)
    tab = torch.nn.functional.leaky_relu(rw * 10.0)
    out = ops.ns_typed_agg(blk, tab, torch.from_numpy(b["n_id"]).to(DEV), tables,
                           torch.from_numpy(b["ntype"]).to(DEV),
                           torch.from_numpy(b["local"]).to(DEV), ext=ext)
    outs = (out,) if ext else out
    sum((o * g.view_as(o)).sum() for o, g in zip(outs, g_out)).backward()
    torch.cuda.synchronize()
    return [o.detach() for o in outs], rw.grad.clone()


@pytest.mark.parametrize("ext", [False, True], ids=["S_w", "ext"])
@pytest.mark.parametrize("meta", [False, True], ids=["n_id", "edge_meta"])
@pytest.mark.parametrize("widths", AGG_WIDTHS, ids=lambda w: "x".join(map(str, w)))
def test_ns_typed_agg_bf16_rows_bitwise(knob_on, widths, meta, ext):
    from regnn_hip import ops
    T, SK = len(widths), sum(widths)
    b = _block(T)
    g = torch.Generator().manual_seed(SK + T)
    tabs = [torch.randn(40, k, generator=g).bfloat16().to(DEV) for k in widths]
    assert ops.ns_typed_agg_ok(tabs)
    if ext:
        g_out = [torch.randn(CAP_DST, SK + (T + 3) // 4 * 4, generator=g).to(DEV)]
    else:
        g_out = [torch.randn(CAP_DST, SK, generator=g).to(DEV),
                 torch.randn(CAP_DST, T, generator=g).to(DEV)]
    got, g_rw = _run_agg(b, tabs, meta, ext, g_out)
    want, g_rw0 = _run_agg(b, _widen(tabs), meta, ext, g_out)
    for name, a, c in zip(("S", "w"), got, want):
        assert a.shape == c.shape and torch.equal(a, c), name
    n = len(LENS)
    assert bool(got[0][1:n].any()) and not bool(got[0][n:].any()) and not bool(got[0][0].any())
    assert torch.equal(g_rw, g_rw0) and bool(g_rw.any())


# ---------------------------------------------------------------------------------------------
# 3. knob off: today's refusals
# ---------------------------------------------------------------------------------------------
def test_knob_off_refuses_as_before(monkeypatch):
    from regnn_hip import ops
    from test_gpu_ns_residual import _mag
    monkeypatch.setitem(ops.BF16_ROWS, "mode", "off")
    d = _mag(0.003, seed=6, hidden=128, residual=False)
    xb = _bf16(d["x_dict"])
    m = d["model"](1)
    with pytest.raises(ValueError, match="group_input needs fp32 tables"):
        m.group_input(xb, d["node_type"], d["local"], torch.arange(32, device=DEV))
    tabs = [xb[k] for k in range(4)]
    assert not ops.ns_typed_agg_ok(tabs)
    assert ops.ns_typed_agg_ok(tabs, pre_sums=True)
    Ws = [m.lins[str(k)].weight for k in range(4)]
    bs = [m.lins[str(k)].bias for k in range(4)]
    assert not ops.typed_linear_fusable(tabs, Ws, bs)
    assert ops.typed_linear_fusable(_widen(tabs), Ws, bs)


# ---------------------------------------------------------------------------------------------
# 4. the trainer's regcn module path
# ---------------------------------------------------------------------------------------------
def _one_step(d, x_dict, **kw):
    from test_gpu_ns_residual import _trainer
    m = d["model"](1)
    m.train()
    tr = _trainer(dict(d, x_dict=x_dict), m, engine="module", pipeline=False, **kw)
    assert tr.fused is None
    tr._forward_backward()
    torch.cuda.synchronize()
    s = tr.sampler
    n_all = int(s.sizes[len(s.sizes_k)])
    return (float(tr.loss), {n: p.grad.clone() for n, p in m.named_parameters()},
            s.n_id[:n_all].clone(), getattr(s.blocks[-1], "pre_sums", None) is not None)


@pytest.mark.parametrize("residual,sizes", [(True, (7, 5)), (False, (5, 64))],
                         ids=["residual", "fanout64"])
def test_trainer_module_path_bf16_rows(knob_on, residual, sizes):
    """residual convs project the raw rows of the targets (group_input); at a fan-out above 63
    the sampler's sums launch does not apply and layer 0 gathers the bf16 rows itself (with the
    knob off: "a fan-out above 63"). The fan-out is 64, the one value above 63 the device sampler
    takes (DeviceSampler refuses fan-outs outside [1, 64] whatever the tables' dtype)."""
    from test_gpu_ns_residual import _mag
    d = _mag(0.003, seed=6, hidden=128, residual=residual)
    xb = _bf16(d["x_dict"])
    la, ga, na, pre_a = _one_step(d, xb, sizes=sizes)
    lb, gb, nb, pre_b = _one_step(d, _widen(xb), sizes=sizes)
    assert torch.equal(na, nb) and na.numel() > 96
    assert pre_a == pre_b == (max(sizes) <= 63)
    print(f"loss {la!r} against {lb!r}")
    assert np.isfinite(la) and abs(la - lb) <= TOL * max(1.0, abs(lb)), (la, lb)
    for n, g in ga.items():
        _check(n, g, gb[n])
    assert bool(ga["lins.0.weight"].any()) and bool(ga["convs.0.relation_weight"].any())


# ---------------------------------------------------------------------------------------------
# 5. regat / regatv2 on device blocks
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gat_data():
    """tests/test_gpu_ns_gat.py's graph with input tables 64 wide in bf16: its own are 16 wide,
    which the gather-fused Linear takes in no dtype (widths 64 / 128 / 256)."""
    from test_gpu_ns_gat import _mag
    d = dict(_mag())
    g = torch.Generator().manual_seed(4)
    d["x_dict"] = {k: torch.randn(v.shape[0], 64, generator=g).bfloat16().to(DEV)
                   for k, v in d["x_dict"].items()}
    return d


def _gat_model(d, kind):
    """test_gpu_ns_gat._model at the tables' width: 2 heads x 32 (the Linear's output a multiple
    of 64)"""
    from regnn_hip import mag
    torch.manual_seed(0)
    return mag.REGNN(64, 32, 5, 2, 10.0, 0.0, {k: 64 for k in d["x_dict"]}, 7, model=kind,
                     heads=2, use_norm="ln", self_loop_type=2).to(DEV).train()


@pytest.fixture
def gat_knobs(knob_on, monkeypatch):
    from regnn_hip import mag, ops
    monkeypatch.setitem(ops.NS_GAT_SRC, "mode", "gather")     # no float atomics in the backward
    monkeypatch.setitem(mag.GATV2_BLOCKS, "mode", "on")


@pytest.mark.parametrize("kind", ["regat", "regatv2"])
def test_gat_device_blocks_bf16_rows_one_step(gat_knobs, kind):
    from test_gpu_ns_gat import _trainer
    d = _gat_data()
    res = []
    for x in (d["x_dict"], _widen(d["x_dict"])):
        m = _gat_model(d, kind)
        tr = _trainer(dict(d, x_dict=x), m, device_blocks=True)
        assert tr.fused is None and tr._gat_blocks
        tr._forward_backward()
        torch.cuda.synchronize()
        res.append((float(tr.loss), {n: p.grad.clone() for n, p in m.named_parameters()}))
    (la, ga), (lb, gb) = res
    print(f"{kind}: loss {la!r} against {lb!r}")
    assert np.isfinite(la) and abs(la - lb) <= TOL * max(1.0, abs(lb)), (la, lb)
    for n, g in ga.items():
        _check(f"{kind} {n}", g, gb[n])
    assert bool(ga["lins.0.weight"].any())


@pytest.mark.parametrize("kind", ["regat", "regatv2"])
def test_gat_device_blocks_bf16_rows_capture_and_replay(gat_knobs, kind):
    from test_gpu_ns_gat import _trainer
    d = _gat_data()
    tr_e = _trainer(d, _gat_model(d, kind), device_blocks=True)
    tr_g = _trainer(d, _gat_model(d, kind), device_blocks=True)
    tr_g.capture(warmup=1)                     # a host sync inside the capture would raise
    le, lg = [], []
    for _ in range(3):
        tr_e.step()
        le.append(float(tr_e.loss))
        tr_g.replay()
        lg.append(float(tr_g.loss))
    print(kind, "eager", le, "replayed", lg)
    assert np.all(np.isfinite(lg))
    assert np.allclose(le, lg, rtol=1e-4, atol=1e-5), (le, lg)


# ---------------------------------------------------------------------------------------------
# 6. the exact-size path
# ---------------------------------------------------------------------------------------------
def test_exact_size_train_step_bf16_rows(knob_on):
    from regnn_hip import mag
    from regnn_hip.sampler import NeighborSampler
    d = _gat_data()
    idx = torch.arange(d["n_paper"], device=DEV)
    smp = NeighborSampler(d["rg"], idx, [6, 4], batch_size=64, shuffle=True, seed=3)
    batch = next(iter(smp))
    res = []
    for x in (d["x_dict"], _widen(d["x_dict"])):
        m = _gat_model(d, "regat")
        loss = mag.train_step(m, torch.optim.SGD(m.parameters(), lr=0.0), batch, x,
                              d["edge_type"], d["node_type"], d["local"], d["y"], 1)
        torch.cuda.synchronize()
        res.append((float(loss.detach()), {n: p.grad.clone() for n, p in m.named_parameters()
                                           if p.grad is not None}))
    (la, ga), (lb, gb) = res
    print(f"loss {la!r} against {lb!r}")
    assert np.isfinite(la) and abs(la - lb) <= TOL * max(1.0, abs(lb)), (la, lb)
    assert set(ga) == set(gb) and "lins.0.weight" in ga
    for n, g in ga.items():
        _check(n, g, gb[n])


# ---------------------------------------------------------------------------------------------
# 7. still refused with the knob on
# ---------------------------------------------------------------------------------------------
def test_still_refused_with_the_knob_on(knob_on, monkeypatch):
    from regnn_hip import mag, ns
    from test_gpu_ns_residual import _mag, _trainer
    d = _mag(0.003, seed=6, residual=False)                  # hidden 64: the fused step's model
    xb = _bf16(d["x_dict"])
    # the fused step reads bf16 rows through the sampler's sums only
    monkeypatch.setitem(ns.PRE_SUMS, "mode", "off")
    with pytest.raises(ValueError, match="PRE_SUMS"):
        _trainer(dict(d, x_dict=xb), d["model"](1), engine="fused")
    monkeypatch.setitem(ns.PRE_SUMS, "mode", "on")
    # one fp32 table among bf16 ones
    mixed = dict(xb)
    mixed[1] = mixed[1].float()
    with pytest.raises(ValueError, match="one dtype"):
        _trainer(dict(d, x_dict=mixed), d["model"](1), engine="module")
    with pytest.raises(ValueError, match="fp32 tables"):
        d["model"](1).group_input(mixed, d["node_type"], d["local"],
                                  torch.arange(32, device=DEV))
    # tables that learn stay fp32
    counts = {k: int(v.shape[0]) for k, v in d["x_dict"].items()}
    m2 = mag.REGNN(128, 64, 37, 2, 10.0, 0.0, {k: 128 for k in range(4)}, 7, use_norm="ln",
                   self_loop_type=2, feats_type=2, num_nodes_dict=counts,
                   target_node_type=0).to(DEV)
    with pytest.raises(ValueError, match="feats_type"):
        ns.NSTrainer(m2, None, d["rg"], [7, 5], 96, torch.arange(d["n_paper"], device=DEV),
                     {0: xb[0]}, d["edge_type"], d["node_type"], d["local"], d["y"], 7)
    # a width the typed kernels have no instantiation for
    g = torch.Generator().manual_seed(1)
    x96 = {k: torch.randn(v.shape[0], 96, generator=g).bfloat16().to(DEV) for k, v in xb.items()}
    m96 = mag.REGNN(96, 128, 37, 2, 10.0, 0.0, {k: 96 for k in range(4)}, 7, use_norm="ln",
                    self_loop_type=2).to(DEV)
    with pytest.raises(ValueError, match="96"):
        _trainer(dict(d, x_dict=x96), m96, engine="module")
