"""GPU checks of the gather form of the device-block attention backwards (regnn_ns_block_tidx,
regnn_ns_gat_bwd_gather / regnn_ns_gatv2_bwd_gather, ops.NS_GAT_SRC = "gather",
NSTrainer(device_blocks=True) with the knob on):

1. the index: t_ptr, t_pos[:n], t_row[:n] and the piece list are exactly _ns_gat_src's numpy
   restatement on the ladder, hub and boundary blocks; a second build into buffers pre-filled with
   0x7f bytes gives the same bits;
2. per-element fp64 parity of ops.ns_gat / ops.ns_gatv2 with the knob on, forward and backward,
   under _attention_ref.rel_err <= TOL_F32: the ladder block (the existing tests' shapes, and one
   per register tier of the v2 row pass) and the hub block;
3. the same row pass: g_er, g_tab (GAT) and g_xd, g_att, g_tab (v2) are torch.equal to atomic
   mode's; g_ft / g_el / g_xs agree with it within 2 TOL_F32 of the scale;
4. every row written, once: the C entries called with NaN-filled g_ft / g_el / g_xs leave no NaN,
   rows past the live sources and rows nothing names are exact zeros;
5. two backward runs give the same bits of g_ft, g_el, g_xs (the second after an unrelated
   launch);
6. the trainer with the knob on: one step against NeighborSampler + mag.train_step, also with a
   short batch; capture and six replays against six eager steps; the freshness guard; for regat
   and for regatv2 (mag.GATV2_BLOCKS on);
7. two identically seeded trainers give torch.equal flat gradient buckets after one eager step.
"""
import numpy as np
import pytest
import torch

import _attention_ref as R
import _golden as G
import _ns_gat_blocks as B
import _ns_gat_src as S
import _ns_gatv2_blocks as V
import test_gpu_ns_gat as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
BLOCKS = ["ladder", "hub"]

_DEV = {}


def _chunk():
    from regnn_hip import ops
    return ops.NS_TIDX_CHUNK


def _block(name):
    """(CPU block, device block, dims), moved once"""
    if name not in _DEV:
        if name == "boundary":
            cpu = S.boundary_block(_chunk())
            dims = dict(S.HUB, cap_dst=cpu.n_dst, live_dst=2 * _chunk() + 1, live_src=905)
        else:
            cpu, dims = S.block_of(name, _chunk())
        _DEV[name] = (cpu, cpu.to(DEV), dims)
    return _DEV[name]


@pytest.fixture
def gather(monkeypatch):
    from regnn_hip import ops
    monkeypatch.setitem(ops.NS_GAT_SRC, "mode", "gather")


# ---- 1. the index ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ladder", "hub", "boundary"])
def test_index_is_exactly_the_canonical_one(name):
    from regnn_hip import ops
    cpu, dev, _ = _block(name)
    t_ptr, t_pos, t_row = S.tidx_reference(cpu)
    n = int(t_ptr[-1])
    t = ops.ns_block_tidx(dev)
    assert t.fresh and t.fits(dev)
    assert np.array_equal(t.t_ptr.cpu().numpy(), t_ptr)
    assert np.array_equal(t.t_pos[:n].cpu().numpy(), t_pos)
    assert np.array_equal(t.t_row[:n].cpu().numpy(), t_row)
    want = S.pieces_reference(t_ptr, _chunk())
    head = t.t_long[:4].tolist()
    assert head == [len(want), len({p[0] for p in want}), _chunk(), 0]
    assert t.pieces() == want
    # a second build into other buffers, pre-filled: every slot a reader takes is rewritten
    t2 = ops.NsTidx(dev.n_dst, dev.n_src, dev.csr_idx.numel(), DEV)
    for buf in (t2.t_ptr, t2.t_pos, t2.t_row, t2.t_long, t2.work):
        buf.view(torch.uint8).fill_(0x7f)
    assert ops.ns_block_tidx(dev, out=t2) is t2
    assert torch.equal(t2.t_ptr, t.t_ptr) and torch.equal(t2.t_pos[:n], t.t_pos[:n])
    assert torch.equal(t2.t_row[:n], t.t_row[:n])
    assert torch.equal(t2.t_long[:4 + 4 * len(want)], t.t_long[:4 + 4 * len(want)])
    # and a rebuild in place (the counters are cleared by the build itself)
    ops.ns_block_tidx(dev, out=t2)
    assert torch.equal(t2.t_ptr, t.t_ptr) and torch.equal(t2.t_pos[:n], t.t_pos[:n])
    assert torch.equal(t2.t_row[:n], t.t_row[:n])


def test_index_refuses_other_buffers_and_strided_blocks():
    from regnn_hip import ops
    _, dev, _ = _block("ladder")
    with pytest.raises(ValueError):
        ops.ns_block_tidx(dev, out=ops.NsTidx(dev.n_dst, dev.n_src + 1, dev.csr_idx.numel(), DEV))
    strided = dev.to(DEV)
    strided.strided_rows = (None, 7)
    with pytest.raises(ValueError):
        ops.ns_block_tidx(strided)


# ---- the operators --------------------------------------------------------------------------------
def _run_gat(name, recipe, H, C):
    """ops.ns_gat forward + backward on a block under the current knob: dict over GAT_KEYS"""
    from regnn_hip import ops
    _, dev, dims = _block(name)
    ft, el, er, tab, gy, slope = S.gat_case(dims, recipe, H, C)
    leaves = [t.to(DEV).requires_grad_(True) for t in (el, er, tab, ft)]
    out = ops.ns_gat(dev, *leaves, slope)
    out.backward(gy.to(DEV))
    return {"out": out.detach(), "g_el": leaves[0].grad, "g_er": leaves[1].grad,
            "g_tab": leaves[2].grad, "g_ft": leaves[3].grad}


def _run_gatv2(name, recipe, H, C):
    from regnn_hip import ops
    _, dev, dims = _block(name)
    xs, xd, att, tab, gy, slope = S.gatv2_case(dims, recipe, H, C)
    leaves = [t.to(DEV).requires_grad_(True) for t in (xs, xd, att, tab)]
    out = ops.ns_gatv2(dev, *leaves, slope)
    out.backward(gy.to(DEV))
    return {"out": out.detach(), "g_xs": leaves[0].grad, "g_xd": leaves[1].grad,
            "g_att": leaves[2].grad, "g_tab": leaves[3].grad}


def _check(tag, got, want, scale, keys, dims, src_keys):
    errs = {}
    for k in keys:
        g = got[k].detach().cpu()
        assert bool(torch.isfinite(g).all()), k
        errs[k] = R.rel_err(g, want[k], scale[k])
    print(f"{tag}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert not got["out"][dims["live_dst"]:].any()
    for k in src_keys:
        assert not got[k][dims["live_src"]:].any(), k
    for k, v in errs.items():
        assert v <= R.TOL_F32, f"{k}: {v:.3e}"


GAT_CASES = [("ladder", r, H, C) for H, C in T.SHAPES for r in S.RECIPES] + \
            [("hub", r, H, C) for H, C in S.HUB_SHAPES for r in S.RECIPES]
GATV2_CASES = [("ladder", r, H, C) for H, C in V.SHAPES for r in S.RECIPES] + \
              [("ladder", "unit", H, C) for H, C in V.WIDTH_SHAPES] + \
              [("hub", r, H, C) for H, C in S.HUB_SHAPES for r in S.RECIPES]


# ---- 2. parity -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,recipe,H,C", GAT_CASES)
def test_ns_gat_gather_matches_fp64_per_element(gather, name, recipe, H, C):
    want, scale = S.gat_ref(name, _chunk(), recipe, H, C)
    got = _run_gat(name, recipe, H, C)
    _check(f"ns_gat gather {name} {recipe} H={H} C={C}", got, want, scale, S.GAT_KEYS,
           _block(name)[2], ("g_ft", "g_el"))


@pytest.mark.parametrize("name,recipe,H,C", GATV2_CASES)
def test_ns_gatv2_gather_matches_fp64_per_element(gather, name, recipe, H, C):
    want, scale = S.gatv2_ref(name, _chunk(), recipe, H, C)
    got = _run_gatv2(name, recipe, H, C)
    _check(f"ns_gatv2 gather {name} {recipe} H={H} C={C}", got, want, scale, S.GATV2_KEYS,
           _block(name)[2], ("g_xs",))


# ---- 3. the same row pass ------------------------------------------------------------------------
@pytest.mark.parametrize("name", BLOCKS + ["boundary"])
@pytest.mark.parametrize("H,C", S.HUB_SHAPES)
def test_row_pass_outputs_equal_atomic_mode(monkeypatch, name, H, C):
    from regnn_hip import ops
    monkeypatch.setitem(ops.NS_GAT_SRC, "mode", "atomic")
    a1, a2 = _run_gat(name, "unit", H, C), _run_gatv2(name, "unit", H, C)
    monkeypatch.setitem(ops.NS_GAT_SRC, "mode", "gather")
    g1, g2 = _run_gat(name, "unit", H, C), _run_gatv2(name, "unit", H, C)
    for k in ("out", "g_er", "g_tab"):
        assert torch.equal(a1[k], g1[k]), f"gat {k}"
    for k in ("out", "g_xd", "g_att", "g_tab"):
        assert torch.equal(a2[k], g2[k]), f"gatv2 {k}"
    if name == "boundary":
        # no fp64 reference is kept for this block: the scale is the atomic form's own magnitude
        # (sum |terms| >= |sum|), so this arm is the weaker one -- the exact piece boundaries'
        for k, a, g in (("g_ft", a1, g1), ("g_el", a1, g1), ("g_xs", a2, g2)):
            d = float((a[k] - g[k]).abs().max())
            print(f"boundary H={H} C={C} {k}: max |gather - atomic| {d:.2e}")
            assert d <= 2 * R.TOL_F32 * max(1.0, float(a[k].abs().max())), k
        return
    _, s1 = S.gat_ref(name, _chunk(), "unit", H, C)
    _, s2 = S.gatv2_ref(name, _chunk(), "unit", H, C)
    for k, a, g, s in (("g_ft", a1, g1, s1), ("g_el", a1, g1, s1), ("g_xs", a2, g2, s2)):
        err = R.rel_err(g[k].cpu(), a[k].cpu().double(), s[k])
        print(f"{name} H={H} C={C} {k}: gather against atomic {err:.2e}")
        assert err <= 2 * R.TOL_F32, f"{k}: {err:.3e}"


# ---- 4. / 5. the C entries directly --------------------------------------------------------------
def _direct(name, kind, H, C, fill=float("nan")):
    """(g_ft, g_el) or (g_xs,) of the gather entry called directly, its outputs pre-filled"""
    from regnn_hip import _lib as L, ops
    _, dev, dims = _block(name)
    t = ops.ns_block_tidx(dev)
    cap_e = dev.csr_idx.numel()
    z = lambda *s: torch.empty(*s, device=DEV)                      # noqa: E731
    ent = z(cap_e, H)
    n_work = int(L._so.regnn_ns_gat_src_work_floats(cap_e, H * C))
    work = z(n_work)
    rows = 16
    index = (L.ptr(t.t_ptr), L.ptr(t.t_pos), L.ptr(t.t_row), L.ptr(t.t_long), dev.n_src,
             dev.n_src, cap_e, L.ptr(ent), L.ptr(work), n_work)
    if kind == "gat":
        ft, el, er, tab, gy, slope = [x.to(DEV) if torch.is_tensor(x) else x
                                      for x in S.gat_case(dims, "unit", H, C)]
        with torch.no_grad():
            _, a = ops.ns_gat(dev, el, er, tab, ft, slope, return_attn=True)
        g_ft, g_el = torch.full_like(ft, fill), torch.full_like(el, fill)
        g_er, slab = torch.empty_like(er), z(rows, tab.shape[0] * H)
        L.call("regnn_ns_gat_bwd_gather", L.ptr(dev.csr_ptr), L.ptr(dev.csr_idx), L.ptr(dev.rel),
               L.ptr(el), L.ptr(er), L.ptr(tab), L.ptr(ft), L.ptr(a), L.ptr(gy), slope, dev.n_dst,
               dev.n_src, H, C, tab.shape[0], L.ptr(g_ft), L.ptr(g_el), L.ptr(g_er), L.ptr(slab),
               rows, *index, L.stream())
        return g_ft, g_el
    xs, xd, att, tab, gy, slope = [x.to(DEV) if torch.is_tensor(x) else x
                                   for x in S.gatv2_case(dims, "unit", H, C)]
    att = att.contiguous()
    with torch.no_grad():
        _, a = ops.ns_gatv2(dev, xs, xd, att, tab, slope, return_attn=True)
    g_xs, g_xd = torch.full_like(xs, fill), torch.empty_like(xd)
    att_slab, tab_slab = z(rows, H * C), z(rows, tab.shape[0] * H)
    L.call("regnn_ns_gatv2_bwd_gather", L.ptr(dev.csr_ptr), L.ptr(dev.csr_idx), L.ptr(dev.rel),
           L.ptr(xs), L.ptr(xd), L.ptr(att), L.ptr(tab), L.ptr(a), L.ptr(gy), slope, dev.n_dst,
           dev.n_src, H, C, tab.shape[0], L.ptr(g_xs), L.ptr(g_xd), L.ptr(att_slab),
           L.ptr(tab_slab), rows, *index, L.stream())
    return (g_xs,)


@pytest.mark.parametrize("name", BLOCKS + ["boundary"])
@pytest.mark.parametrize("kind", ["gat", "gatv2"])
def test_every_source_row_written_once(name, kind):
    cpu, _, dims = _block(name)
    t_ptr, _, _ = S.tidx_reference(cpu)
    unnamed = torch.from_numpy(np.flatnonzero(np.diff(t_ptr) == 0)).to(DEV)
    assert unnamed.numel() >= cpu.n_src - dims["live_src"]
    for H, C in S.HUB_SHAPES:
        for g in _direct(name, kind, H, C):
            assert not torch.isnan(g).any(), (H, C)
            assert not g[dims["live_src"]:].any(), (H, C)
            assert not g[unnamed].any(), (H, C)
            assert g[:dims["live_src"]].any()


@pytest.mark.parametrize("H,C", S.HUB_SHAPES)
def test_backward_bitwise_reproducible_on_the_hub_block(H, C):
    first = _direct("hub", "gat", H, C) + _direct("hub", "gatv2", H, C)
    noise = torch.zeros(64 << 20, device=DEV)                  # an unrelated launch in between
    second = _direct("hub", "gat", H, C, fill=1.0) + _direct("hub", "gatv2", H, C, fill=1.0)
    assert not noise.any()
    for k, x, y in zip(("g_ft", "g_el", "g_xs"), first, second):
        assert torch.equal(x, y), k


def test_junk_knob_raises_at_first_use(monkeypatch):
    from regnn_hip import ops
    monkeypatch.setitem(ops.NS_GAT_SRC, "mode", "scatter")
    _, dev, dims = _block("ladder")
    ft, el, er, tab, gy, slope = S.gat_case(dims, "unit", 2, 32)
    leaves = [t.to(DEV).requires_grad_(True) for t in (el, er, tab, ft)]
    out = ops.ns_gat(dev, *leaves, slope)
    with pytest.raises(ValueError):
        out.backward(gy.to(DEV))


# ---- 6. the trainer -------------------------------------------------------------------------------
@pytest.fixture(params=["regat", "regatv2"])
def model_kind(request, monkeypatch):
    from regnn_hip import mag, ops
    monkeypatch.setitem(ops.NS_GAT_SRC, "mode", "gather")
    if request.param == "regatv2":
        monkeypatch.setitem(mag.GATV2_BLOCKS, "mode", "on")
    return request.param


@pytest.mark.parametrize("n_train", [None, 37])
def test_trainer_gather_matches_pyg_path(model_kind, n_train):
    """n_train = 37: the batch holds fewer targets than its capacity (sizes[0] < B)"""
    from regnn_hip import mag
    from regnn_hip.sampler import NeighborSampler
    d = T._mag()
    idx = torch.arange(d["n_paper"] if n_train is None else n_train, device=DEV)
    m_api, m_eng = T._model(d, model=model_kind), T._model(d, model=model_kind)
    m_api.train(); m_eng.train()
    smp = NeighborSampler(d["rg"], idx, [6, 4], batch_size=64, shuffle=True, seed=3)
    batch = next(iter(smp))
    loss_api = mag.train_step(m_api, torch.optim.SGD(m_api.parameters(), lr=0.0), batch,
                              d["x_dict"], d["edge_type"], d["node_type"], d["local"], d["y"], 1)
    tr = T._trainer(d, m_eng, train_idx=idx, device_blocks=True)
    assert tr._gat_blocks and tr._gat_src_gather
    assert tr.fused is None and tr.pipelined and tr.ahead == 1 and len(tr.slots) == 2
    assert all(b.tidx is s.tidx[h] for s in tr.slots for h, b in enumerate(s.blocks))
    tr._forward_backward()
    torch.cuda.synchronize()
    la = float(loss_api.detach())
    print(f"{model_kind} loss {float(tr.loss):.7f} against {la:.7f}")
    assert abs(float(tr.loss) - la) <= 1e-5 * max(1.0, abs(la))
    assert int(tr.sampler.sizes[0]) == (64 if n_train is None else n_train)
    gp = dict(m_api.named_parameters())
    for n, p in m_eng.named_parameters():
        if gp[n].grad is None:                 # declared, unused in forward (REGNN.norm)
            assert not p.grad.any(), n
            continue
        ok, err = G.close(p.grad.cpu().numpy(), gp[n].grad.cpu().numpy().astype(np.float64), 1e-5)
        print(f"{n}: rel err {err:.2e}")
        assert ok, f"{n}: rel err {err:.3e}"


def test_trainer_gather_capture_and_replay(model_kind):
    d = T._mag()
    tr_e = T._trainer(d, T._model(d, model=model_kind), device_blocks=True)
    tr_g = T._trainer(d, T._model(d, model=model_kind), device_blocks=True)
    tr_g.capture(warmup=1)                     # a host sync inside the capture would raise
    assert not tr_g.graph_groups               # one-step graphs only
    le, lg = [], []
    for _ in range(6):
        tr_e.step()
        le.append(float(tr_e.loss))
        tr_g.replay()
        lg.append(float(tr_g.loss))
    print(model_kind, "eager", le, "replayed", lg)
    assert np.all(np.isfinite(lg))
    assert np.allclose(le, lg, rtol=1e-4, atol=1e-5), (le, lg)
    assert tr_g.edges_total() > 0


def test_trainer_refuses_a_stale_index(model_kind):
    d = T._mag()
    tr = T._trainer(d, T._model(d, model=model_kind), device_blocks=True)
    tr._forward_backward()                     # slot 0 trained, slot 1 sampled with its index
    s = tr.slots[tr.cur]
    assert all(t.fresh for t in s.tidx)
    s.run_hops(meta_only=tr._module_lean, strided=False)       # resampled, the index not rebuilt
    assert not any(t.fresh for t in s.tidx)
    with pytest.raises(RuntimeError, match="older than their batch"):
        tr._module_step(s)


def test_knob_off_leaves_the_trainer_without_an_index():
    d = T._mag()
    tr = T._trainer(d, T._model(d), device_blocks=True)
    assert tr._gat_blocks and not tr._gat_src_gather
    assert all(t is None for s in tr.slots for t in s.tidx)
    assert not any(hasattr(b, "tidx") for s in tr.slots for b in s.blocks)


# ---- 7. step reproducibility ----------------------------------------------------------------------
def test_two_seeded_trainers_give_the_same_gradient_bits(model_kind, monkeypatch):
    from regnn_hip import ops
    monkeypatch.setitem(ops.SMALL_BLAS, "mode", "off")         # the deterministic x6 GEMM
    d = T._mag()
    flats = []
    for _ in range(2):
        tr = T._trainer(d, T._model(d, model=model_kind), device_blocks=True)
        tr._forward_backward()
        torch.cuda.synchronize()
        flats.append((float(tr.loss), tr.flat.clone()))
        torch.zeros(16 << 20, device=DEV)      # an unrelated launch between the two runs
    assert flats[0][1].any()
    assert flats[0][0] == flats[1][0]
    assert torch.equal(flats[0][1], flats[1][1])
