"""The sampler's sums launch at one input width per node type (regnn_ns_hop_typed_sums_kt) and its
layer-0 consumer (regnn_ns_slot_agg_kt / _bwd_kt), behind ops.NS_SUMS_KT:

1. the launch on the hand-built typed graph against an fp64 restatement over the sampler oracle's
   draws (tests/_ns_sums_kt_ref.py), five width sets x three fan-outs x both DERIVE instantiations;
2. every width 128: regnn_ns_hop_typed_sums_dt's bits, fp32 and bf16 tables;
3. bf16 tables: the bits of the fp32 call on the widened tables;
4. the slot kernels on a padded block, forward and backward;
5. the module-engine trainer on fp32 tables, knob on against knob off, and the reference's fixture;
6. bf16 tables of mixed widths; 7. captured and pipelined; 8. sharded inference.

Floats against fp64 or across code paths: _golden.close at 1e-5, the project's bound (an fp32
restatement of these sums measures ~4e-7 under that metric). Integers and copies: exact."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import _golden as G
import _ns_sums_kt_ref as R
from test_ns_type_layout import SEED, hand_graph

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5
NAMES = ("s_agg", "s_w", "u_self", "u_rel", "scnt", "inv")
T = 4


def _close(tag, got, want, tol=TOL):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = want.detach().double().cpu().numpy() if torch.is_tensor(want) else np.asarray(want)
    ok, err = G.close(got, want, tol)
    print(f"{tag}: rel err {err:.3e}")
    assert ok, f"{tag}: rel err {err:.3e}"


@functools.lru_cache(maxsize=None)
def _graph(layout):
    """the hand-built typed graph on the device (layout False: its ids permuted, so the launch
    reads the lookup tables: the other DERIVE instantiation) and its CSR by target on the host."""
    import test_gpu_ns_type_layout as TL
    g = hand_graph() if layout else TL._permuted(hand_graph())
    c = TL._case(g)
    rg = c["rg"]
    c["csr"] = tuple(t.cpu().numpy() for t in (rg.csr_ptr, rg.csr_idx, rg.csr_eid))
    return c


def _tables(widths, seed=5, dtype=torch.float32):
    gen = torch.Generator().manual_seed(seed)
    counts = hand_graph()["counts"]
    return {t: torch.randn(c, widths[t], generator=gen).to(DEV).to(dtype).contiguous()
            for t, c in enumerate(counts)}


def _sampler(c, sizes, x, widths):
    """a DeviceSampler whose outer hop runs as the sums launch over the tables x -- the _kt entry
    for `widths`, regnn_ns_hop_typed_sums_dt for None -- into NaN-filled output buffers."""
    from regnn_hip import _lib as L
    from regnn_hip.ns import DeviceSampler, sampler_type_layout
    g = c["g"]
    s = DeviceSampler(c["rg"], list(sizes), g["N"], etype=c["etype"], ntype=c["ntype"],
                      num_edge_types=g["R"])
    s.enable_edge_meta(c["local"], 1)
    s.meta_only[1], s.hop_strided[1] = True, True
    cap = s.caps[1]
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)  # noqa: E731
    if widths is None:
        U, xs = nan(cap, T, 128), nan(cap, 128)
    else:
        U, xs = nan(cap, sum(widths)), nan(cap, max(widths))
    tabs = [x[t] for t in range(T)]
    ts = dict(tables=(ctypes.c_void_p * T)(*[t.data_ptr() for t in tabs]),
              dtype=L.dtype_code(tabs[0]), T=T, K=128, s_agg=U, s_w=nan(cap, T), u_self=xs,
              u_rel=torch.full((cap, T + 1), -9, dtype=torch.int32, device=DEV), keep=tabs,
              layout=sampler_type_layout(s, T), meta_unread=True)
    if widths is not None:
        ts["widths"] = (ctypes.c_int32 * T)(*widths)
    s.typed_sums[1] = ts
    return s


def _run(c, sizes, x, widths, layout):
    s = _sampler(c, sizes, x, widths)
    ts = s.typed_sums[1]
    assert (ts["layout"] is not None) == layout
    s.set_seed(SEED, 0, 0)
    s.set_targets(torch.arange(c["g"]["N"], device=DEV))
    s.run_hops()
    torch.cuda.synchronize()
    assert s.sums_fresh[1]
    n1 = int(s.sizes[1])
    cap = s.caps[1]
    U = ts["s_agg"].reshape(cap, -1)
    assert n1 < cap and bool(torch.isnan(U[n1:]).all())        # rows past the batch: untouched
    bufs = [U[:n1].clone(), ts["s_w"][:n1].clone(), ts["u_self"][:n1].clone(),
            ts["u_rel"][:n1].clone(), s.hop_bufs[1]["scnt"].clone(), s.blocks[1].inv.clone()]
    return s, bufs, n1


# ---------------------------------------------------------------------------------------------
# 1. against the fp64 restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [True, False], ids=["layout", "tables"])
@pytest.mark.parametrize("sizes", R.FANOUTS, ids=lambda s: f"k{s[1]}")
@pytest.mark.parametrize("widths", R.WIDTH_SETS, ids=lambda w: "x".join(map(str, w)))
def test_sums_kt_against_fp64(widths, sizes, layout):
    c = _graph(layout)
    x = _tables(widths)
    s, got, n1 = _run(c, sizes, x, widths, layout)
    x64 = {t: v.double().cpu().numpy() for t, v in x.items()}
    n_id, ref = R.oracle_sums(c["g"], c["csr"], x64, widths, *sizes, SEED)
    assert n1 == len(n_id) and s.n_id[:n1].cpu().tolist() == n_id
    assert int(ref["scnt"].max()) == min(sizes[1], 40)
    for name, t in zip(NAMES, got):
        a = t[:n1].cpu().numpy()
        assert np.isfinite(a).all(), name
        if name in ("s_agg", "u_self", "inv"):
            _close(name, a, ref[name])
        else:                                  # counts, slot relations: exact
            assert np.array_equal(a.astype(np.int64), ref[name].astype(np.int64)), name
    # the self rows are copies, and exactly zero past their own width
    us = got[2].cpu().numpy()
    assert np.array_equal(us, ref["u_self"].astype(np.float32))
    kself = np.array([widths[int(c["g"]["ntype"][t])] for t in n_id])
    past = np.arange(max(widths))[None, :] >= kself[:, None]
    assert not us[past].any() and not np.signbit(us[past]).any()
    # rows past the batch: in-count 0, scale 1
    assert not got[4][n1:].any() and bool((got[5][n1:] == 1).all())


# ---------------------------------------------------------------------------------------------
# 2. / 3. bitwise: all widths 128 against the equal-width entry; bf16 against widened fp32
# ---------------------------------------------------------------------------------------------
def _state(s):
    """what the sampling leaves besides the sums: the per-slot meta, the hop's sizes, the edge
    total in the state."""
    et, eo = s.edge_meta[1]
    return [s.blocks[1].rel.clone(), et.clone(), eo.clone(), s.sizes.clone(), s.state[5:6].clone()]


@pytest.mark.parametrize("layout", [True, False], ids=["layout", "tables"])
@pytest.mark.parametrize("sizes", R.FANOUTS, ids=lambda s: f"k{s[1]}")
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_all_128_gives_the_equal_width_bits(dtype, sizes, layout):
    c = _graph(layout)
    x = _tables((128,) * 4, dtype=dtype)
    sa, a, n1 = _run(c, sizes, x, (128,) * 4, layout)
    sb, b, n1b = _run(c, sizes, x, None, layout)
    assert n1 == n1b and torch.equal(sa.n_id[:n1], sb.n_id[:n1])
    for name, p, q in zip(NAMES, a, b):
        assert torch.equal(p, q), name
    for p, q in zip(_state(sa), _state(sb)):
        assert torch.equal(p, q)
    assert bool(a[0].any()) and int(a[4].max()) == min(sizes[1], 40)


@pytest.mark.parametrize("layout", [True, False], ids=["layout", "tables"])
@pytest.mark.parametrize("sizes", R.FANOUTS, ids=lambda s: f"k{s[1]}")
@pytest.mark.parametrize("widths", [(256, 128, 128, 128), (64, 256, 128, 64)],
                         ids=lambda w: "x".join(map(str, w)))
def test_bf16_tables_give_the_widened_fp32_bits(widths, sizes, layout):
    from test_gpu_ns_bf16 import _special
    c = _graph(layout)
    xb = {t: _special(v) for t, v in _tables(widths, dtype=torch.bfloat16).items()}
    sa, a, n1 = _run(c, sizes, xb, widths, layout)
    sb, b, _ = _run(c, sizes, {t: v.float() for t, v in xb.items()}, widths, layout)
    assert sa.typed_sums[1]["dtype"] == 1 and sb.typed_sums[1]["dtype"] == 0
    for name, p, q in zip(NAMES, a, b):
        assert torch.equal(p, q), name
    for p, q in zip(_state(sa), _state(sb)):
        assert torch.equal(p, q)
    # the self rows are the table rows' bits shifted up by 16, zeros after them, nothing else
    ida = sa.n_id[:n1].long()
    nt, loc = c["ntype"][ida], c["local"][ida]
    want = torch.zeros(n1, max(widths), dtype=torch.int32, device=DEV)
    for t, tab in xb.items():
        m = nt == t
        want[m, :widths[t]] = tab.view(torch.int16)[loc[m].long()].int() << 16
    assert torch.equal(a[2].view(torch.int32), want)


def test_meta_is_optional(monkeypatch):
    """the all-NULL meta triple (ns.SUMS_META "off" on a graph with the layout): the same sums,
    the per-slot meta left alone."""
    from regnn_hip import ns
    c = _graph(True)
    widths, sizes = (256, 128, 128, 128), (3, 20)
    x = _tables(widths)
    sa, a, _ = _run(c, sizes, x, widths, True)
    monkeypatch.setitem(ns.SUMS_META, "mode", "off")
    sb, b, _ = _run(c, sizes, x, widths, True)
    assert sa.meta_fresh[1] and not sb.meta_fresh[1]
    for name, p, q in zip(NAMES, a, b):
        assert torch.equal(p, q), name
    assert bool(sa.blocks[1].rel.any()) and not bool(sb.blocks[1].rel.any())


# ---------------------------------------------------------------------------------------------
# 4. the slot kernels
# ---------------------------------------------------------------------------------------------
def _slot_case(widths, sizes=(3, 20)):
    c = _graph(True)
    x = _tables(widths)
    s, bufs, n1 = _run(c, sizes, x, widths, True)
    ts = s.typed_sums[1]
    R_ = c["g"]["R"]
    gen = torch.Generator().manual_seed(2)
    tab = (torch.randn(R_ + T, generator=gen) * 0.5).to(DEV)
    cap = s.caps[1]
    assert n1 == 48 and cap == 192             # live rows below the capacity, and below 128
    return c, x, s, ts, tab, n1, cap, R_


def _slot_fwd_c(ts, sizes_t, tab, widths, n_et, cap, fill=float("nan")):
    from regnn_hip import _lib as L
    ld = (sum(widths) if widths else T * 128) + 4
    out = torch.full((cap, ld), fill, device=DEV)
    wd = 128 if widths is None else (ctypes.c_int32 * T)(*widths)
    L.call("regnn_ns_slot_agg" if widths is None else "regnn_ns_slot_agg_kt", L.ptr(sizes_t), 1,
           L.ptr(ts["s_agg"]), L.ptr(ts["s_w"]), L.ptr(ts["u_self"]), L.ptr(ts["u_rel"]),
           L.ptr(tab), n_et, T, wd, cap, L.ptr(out), ld, L.stream())
    torch.cuda.synchronize()
    return out


def _blk(s, ts, widths):
    b = types.SimpleNamespace(pre_sums=(ts["s_agg"], ts["s_w"], ts["u_self"], ts["u_rel"]),
                              live_rows=s.sizes[1:2])
    if widths is not None:
        b.pre_widths = tuple(widths)
    return b


def _slot_autograd(s, ts, tab, widths, n_et, g):
    from regnn_hip import ops
    t = tab.clone().requires_grad_(True)
    out = ops.ns_slot_agg(_blk(s, ts, widths), t, n_et)
    out.backward(g)
    torch.cuda.synchronize()
    return out.detach(), t.grad.clone()


@pytest.mark.parametrize("widths", R.WIDTH_SETS, ids=lambda w: "x".join(map(str, w)))
def test_slot_agg_kt_against_fp64(widths):
    c, x, s, ts, tab, n1, cap, n_et = _slot_case(widths)
    SK = sum(widths)
    out = _slot_fwd_c(ts, s.sizes, tab, widths, n_et, cap)
    U, cnt, xs, ur = (t[:n1].double().cpu().numpy() for t in
                      (ts["s_agg"], ts["s_w"], ts["u_self"], ts["u_rel"]))
    tab64 = tab.double().cpu().numpy()
    S, w = R.slot_fwd(U, cnt, xs, ur.astype(np.int64), tab64, n_et, widths)
    _close("S", out[:n1, :SK], S)
    _close("w", out[:n1, SK:SK + T], w)
    # the row rule: zeros in [n, next multiple of 128), later rows untouched
    assert not bool(out[n1:128].any()) and bool(torch.isnan(out[128:]).all())
    # backward, through ops.ns_slot_agg, on every live row's gradient
    gen = torch.Generator().manual_seed(4)
    g = torch.randn(cap, SK + 4, generator=gen).to(DEV)
    o1, d1 = _slot_autograd(s, ts, tab, widths, n_et, g)
    o2, d2 = _slot_autograd(s, ts, tab, widths, n_et, g)
    assert torch.equal(o1[:128], out[:128]) and torch.equal(o1[:128], o2[:128])
    assert torch.equal(d1, d2)                 # the same bits on every run
    g64 = g[:n1].double().cpu().numpy()
    want = R.slot_bwd(U, cnt, xs, ur.astype(np.int64), g64[:, :SK], g64[:, SK:SK + T], n_et,
                      widths, tab.numel())
    assert np.abs(want).max() > 0
    _close("d tab", d1, want)


def test_slot_agg_kt_at_128_gives_the_equal_width_bits():
    widths = (128,) * 4
    c, x, s, ts, tab, n1, cap, n_et = _slot_case(widths)
    a = _slot_fwd_c(ts, s.sizes, tab, widths, n_et, cap, fill=7.0)
    b = _slot_fwd_c(ts, s.sizes, tab, None, n_et, cap, fill=7.0)
    assert torch.equal(a, b) and bool((a[128:] == 7.0).all())
    gen = torch.Generator().manual_seed(4)
    g = torch.randn(cap, 4 * 128 + 4, generator=gen).to(DEV)
    _, da = _slot_autograd(s, ts, tab, widths, n_et, g)
    ts3 = dict(ts, s_agg=ts["s_agg"].view(cap, T, 128))
    _, db = _slot_autograd(s, ts3, tab, None, n_et, g)
    assert torch.equal(da, db) and bool(da.any())


@pytest.mark.parametrize("widths", [(256, 128, 128, 128), (64, 256, 128, 64)],
                         ids=lambda w: "x".join(map(str, w)))
def test_slot_agg_kt_against_the_typed_gather(widths):
    """the same batch sampled in full (CSR blocks), layer 0's operand gathered from the raw rows
    (ops.ns_typed_agg, ext): the sums' route gives the same [S | w | 0] and the same d tab."""
    from regnn_hip import ops
    from regnn_hip.ns import DeviceSampler
    c, x, s, ts, tab, n1, cap, n_et = _slot_case(widths)
    g_ = c["g"]
    s2 = DeviceSampler(c["rg"], [3, 20], g_["N"], etype=c["etype"], ntype=c["ntype"],
                       num_edge_types=n_et)
    s2.set_seed(SEED, 0, 0)
    s2.set_targets(torch.arange(g_["N"], device=DEV))
    s2.run_hops(meta_only=False)
    torch.cuda.synchronize()
    assert int(s2.sizes[1]) == n1 and torch.equal(s2.n_id[:n1], s.n_id[:n1])
    gen = torch.Generator().manual_seed(4)
    g = torch.randn(cap, sum(widths) + 4, generator=gen).to(DEV)
    g[n1:] = 0                                 # (the gather's rows past the batch have no edges)
    t2 = tab.clone().requires_grad_(True)
    ref = ops.ns_typed_agg(s2.blocks[1], t2, s2.n_id, [x[t] for t in range(T)], c["ntype"],
                           c["local"], ext=True)
    ref.backward(g[:ref.shape[0]])
    got, d = _slot_autograd(s, ts, tab, widths, n_et, g)
    _close("[S | w | 0]", got[:n1], ref[:n1])
    _close("d tab", d, t2.grad)


# ---------------------------------------------------------------------------------------------
# 5. the trainer on fp32 tables
# ---------------------------------------------------------------------------------------------
def _one_step(d, hidden, residual, knob, x_dict=None):
    from regnn_hip import ops
    from test_gpu_type_widths import _model, _trainer
    old = ops.NS_SUMS_KT["mode"]
    ops.NS_SUMS_KT["mode"] = knob
    try:
        m = _model(hidden, residual)
        d = d if x_dict is None else dict(d, x_dict=x_dict)
        tr = _trainer(d, m, torch.optim.SGD(m.parameters(), lr=0.0), seed=3, engine="module")
        assert tr.fused is None and tr._module_lean
        pre = getattr(tr.slots[0].blocks[-1], "pre_sums", None)
        assert (pre is not None) == (knob == "on")
        tr._forward_backward()
        torch.cuda.synchronize()
        n1 = int(tr.sampler.sizes[1])
        return (float(tr.loss), {n: p.grad.detach().double().cpu().numpy().copy()
                                 for n, p in m.named_parameters()},
                None if pre is None else [t[:n1].clone() for t in pre])
    finally:
        ops.NS_SUMS_KT["mode"] = old


@pytest.mark.parametrize("hidden,residual", [(128, True), (512, False)])
def test_trainer_fp32_knob_on_matches_knob_off(hidden, residual):
    from test_gpu_type_widths import _mag_widths
    d = _mag_widths()
    la, ga, pre = _one_step(d, hidden, residual, "on")
    lb, gb, _ = _one_step(d, hidden, residual, "off")
    assert pre[0].dim() == 2 and pre[0].shape[1] == 640 and pre[2].shape[1] == 256
    print(f"hidden {hidden}: loss {la!r} vs {lb!r}")
    assert np.isfinite(la) and abs(la - lb) <= TOL * max(1.0, abs(lb)), (la, lb)
    for n in gb:
        _close(f"hidden {hidden} grad {n}", ga[n], gb[n])
    assert np.abs(ga["convs.0.relation_weight"]).max() > 0


def test_ft5_fixture_with_the_sums(monkeypatch):
    """tests/test_gpu_regnn_golden.py::test_regnn_module_step_ft5_vs_reference with the knob on:
    the reference's loss and every gradient at 1e-5, layer 0 reading the sampler's sums."""
    from regnn_hip import ops
    from regnn_hip.graph import RelGraph
    from regnn_hip.ns import NSTrainer
    from test_gpu_regnn_golden import _inputs, _model as golden_model
    monkeypatch.setitem(ops.NS_SUMS_KT, "mode", "on")
    d = G.load("mag_regnn_ft5_h128")
    m = d["meta"]
    rg = RelGraph(torch.from_numpy(d["src"]), torch.from_numpy(d["dst"]), int(sum(m["counts"])),
                  DEV)
    model = golden_model(d)
    model.eval()
    x_dict, _, et, nt, loc = _inputs(d)
    y = torch.from_numpy(d["y"]).to(DEV).reshape(-1, 1)
    batch = torch.from_numpy(d["batch"]).to(DEV)
    tr = NSTrainer(model, None, rg, m["sizes"], batch.numel(), batch, x_dict, et, nt, loc, y,
                   m["num_edge_types"], seed=m["seed"], engine="auto", pipeline=False)
    assert tr.fused is None and tr._module_lean is True
    s = tr.slots[0]
    pre = getattr(s.blocks[-1], "pre_sums", None)
    assert pre is not None
    assert s.blocks[-1].pre_widths == tuple(int(x_dict[t].shape[1]) for t in sorted(x_dict))
    assert len(set(s.blocks[-1].pre_widths)) > 1
    s.set_seed(m["seed"], m["epoch"], m["batch_idx"])
    s.set_targets(batch)
    s.run_hops(meta_only=True, strided=False)
    L_ = len(m["sizes"])
    n_chk = int(s.sizes[L_ - 1])
    assert s.sums_fresh[-1]
    assert s.n_id[:n_chk].cpu().numpy().tolist() == d["n_id"][:n_chk].tolist()
    tr._module_step(s)
    torch.cuda.synchronize()
    _close("loss", tr.loss, d["loss"])
    got = {n: p.grad for n, p in model.named_parameters()}
    for k, v in G.sub(d, "grad_").items():
        _close(k, got[k], v)


# ---------------------------------------------------------------------------------------------
# 6. bf16 tables of mixed widths
# ---------------------------------------------------------------------------------------------
def _bf16(x_dict):
    return {k: v.bfloat16().contiguous() for k, v in x_dict.items()}


def test_trainer_bf16_mixed_widths():
    from test_gpu_type_widths import _mag_widths, _model, _trainer
    d = _mag_widths()
    xb = _bf16(d["x_dict"])
    la, ga, pa = _one_step(d, 128, False, "on", x_dict=xb)
    lb, gb, pb = _one_step(d, 128, False, "on", x_dict={k: v.float() for k, v in xb.items()})
    for name, p, q in zip(("U", "cnt", "x_self", "u_rel"), pa, pb):
        assert torch.equal(p, q), name
    assert bool(pa[0].any())
    # (zero in exact arithmetic: the bound absorbs a GEMM algorithm choice that may differ per run)
    assert np.isfinite(la) and abs(la - lb) <= TOL * max(1.0, abs(lb)), (la, lb)
    for n in gb:
        _close(f"grad {n}", ga[n], gb[n])
    # the knob off: refused as before, and the message names the knob
    m = _model(128, False)
    with pytest.raises(ValueError, match="REGNN_NS_SUMS_KT"):
        _trainer(dict(d, x_dict=xb), m, torch.optim.SGD(m.parameters(), lr=0.0), seed=3,
                 engine="module")


# ---------------------------------------------------------------------------------------------
# 7. captured and pipelined
# ---------------------------------------------------------------------------------------------
def test_bf16_mixed_widths_pipelined_captured_matches_eager():
    """tests/test_gpu_type_widths.py::_captured_and_eager's recipe on bf16 tables of mixed widths
    (so without residual convs), the knob on: 4 replayed pipelined steps end at the parameters of
    4 eager unpipelined steps, bitwise."""
    from regnn_hip import ns, ops
    from test_gpu_type_widths import _mag_widths, _model, _trainer
    knobs = [(ops.SMALL_BLAS, "mode", "off"), (ns.MODULE_PIPELINE, "mode", "on"),
             (ns.MODULE_AHEAD, "n", 1), (ops.NS_SUMS_KT, "mode", "on")]
    old = [(d_, k, d_[k]) for d_, k, _ in knobs]
    for d_, k, v in knobs:
        d_[k] = v
    try:
        d = _mag_widths()
        d = dict(d, x_dict=_bf16(d["x_dict"]))

        def make(pipe):
            return _trainer(d, _model(128, False, seed=5), None, seed=9, adam=dict(lr=1e-2),
                            engine="module", pipeline=pipe)
        tr_p, tr_u = make(True), make(False)
        assert tr_p.fused is None and tr_p._module_lean and tr_u._module_lean
        assert tr_p.pipelined and not tr_u.pipelined
        for s in tr_p.slots + tr_u.slots:
            assert s.typed_sums[-1]["dtype"] == 1 and "widths" in s.typed_sums[-1]
        tr_p.capture(warmup=2)                          # warm-up steps undone by capture()
        tr_p.run_steps(4)
        for _ in range(4):
            tr_u.step()
        torch.cuda.synchronize()
        assert torch.equal(tr_p.sampler.n_id[:int(tr_p.sampler.sizes[0])],
                           tr_u.sampler.n_id[:int(tr_u.sampler.sizes[0])])
        lp, lu = float(tr_p.loss), float(tr_u.loss)
        pp, pu = tr_p.param_vector(), tr_u.param_vector()
        print(f"loss captured {lp!r} eager {lu!r}; max |d param| {float((pp - pu).abs().max()):.3e}")
        assert np.isfinite(lp) and bool(torch.isfinite(pp).all())
        assert torch.equal(pp, pu)
    finally:
        for d_, k, v in old:
            d_[k] = v


# ---------------------------------------------------------------------------------------------
# 8. sharded inference
# ---------------------------------------------------------------------------------------------
def test_sharded_inference_on_bf16_mixed_widths():
    from test_gpu_type_widths import _mag_widths, _model
    d = _mag_widths()
    xb = _bf16(d["x_dict"])
    m = _model(128, False).eval()
    args = (d["rg"], d["edge_type"], d["node_type"], d["local"], 0, 1)
    want = m.inference_sharded({k: v.float() for k, v in xb.items()}, *args, gather=None)
    got = m.inference_sharded(xb, *args, gather=None)
    torch.cuda.synchronize()
    assert got.shape == want.shape and bool(torch.isfinite(got).all()) and bool(got.any())
    assert torch.equal(got, want)
