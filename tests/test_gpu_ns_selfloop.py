"""GPU checks of mag self_loop_type 1 / 3 on device-sampled blocks and in inference
(regnn_ns_hop_noloop, DeviceSampler(self_loops=False), the convs on loop-less NSBlocks,
NSTrainer(device_blocks=True) and ShardedInference for models of those types):

1. the loop-less sampler against oracle.sampler_oracle, bit for bit (n_id, sizes, every block
   array), two consecutive batches on one sampler, a batch of one zero-in-degree target (E = 0);
2. a default sampler's block with its loop entries removed equals the loop-less block;
3. each conv class on a loop-less block: the mag_noloop_*conv_sl3 fixtures and the exact-size call
   (1e-5), the per-element attention metric on a padded ladder block with rows of 0 entries
   (_attention_ref.rel_err <= TOL_F32), both mismatch refusals;
4. NSTrainer(device_blocks=True), (regcn, regat, regatv2) x (1, 3): one step against the
   nssl_regnn_* fixtures and against NeighborSampler + mag.train_step on the same batch (also a
   batch shorter than its capacity); regcn with use_norm 'bn', and at hidden 128 (the typed first
   layer's plain form and the one-launch LayerNorm epilogue), against the exact-size path;
   NS_GAT_SRC "gather": two runs of one batch give the same gradient bits;
5. capture: six replays track six eager steps (regcn and regat, type 3);
6. inference for each model and type: REGNN.inference against REGNN.forward in eval mode over
   full-neighbour adjs, inference_sharded's steps driven in lockstep for 2 ranks against 1, a node
   without in-edges among the rows for type 3 (1e-5, as test_gpu_infer / test_gpu_attn_infer);
7. engine="fused", bf16 tables, strided=True / enable_csc on a loop-less sampler raise ValueError;
   with mag.NOLOOP_BLOCKS off (the default) the trainer and the inference refuse types 1 / 3 as
   they did before the path existed.
"""
import numpy as np
import pytest
import torch

import _attention_ref as R
import _golden as G
import _ns_gat_blocks as B
from oracle import sampler_oracle as SO

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5
KINDS = ["regcn", "regat", "regatv2"]
CONV_FIXTURES = {k: f"mag_noloop_{k}conv_sl3" for k in KINDS}


@pytest.fixture(autouse=True)
def _knobs_on(monkeypatch):
    """the path is opt-in: mag.NOLOOP_BLOCKS (and, for regatv2 on blocks, mag.GATV2_BLOCKS)"""
    from regnn_hip import mag
    monkeypatch.setitem(mag.GATV2_BLOCKS, "mode", "on")
    monkeypatch.setitem(mag.NOLOOP_BLOCKS, "mode", "on")


def _check(tag, got, want, tol=TOL):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = want.detach().double().cpu().numpy() if torch.is_tensor(want) else \
        np.asarray(want, np.float64)
    ok, err = G.close(got, want, tol)
    print(f"{tag}: rel err {err:.3e}")
    assert ok, f"{tag}: rel err {err:.3e}"


# ---------------------------------------------------------------------------------------------
# 1. / 2. the sampler
# ---------------------------------------------------------------------------------------------
_SG = {}
N_NODES, K_FAN = 300, 5


def _sampler_graph():
    """300 nodes; among the 37 targets (nodes 0 .. 36): in-degree 0 (nodes 0 .. 3), < k, = k
    (node 5), > k and a hub (node 6, 150 in-edges); edges dst-major, so edge ids are CSR
    positions"""
    if _SG:
        return _SG
    from regnn_hip.graph import RelGraph
    rng = np.random.default_rng(41)
    deg = rng.integers(1, 12, N_NODES)
    deg[:4], deg[4], deg[5], deg[6], deg[7] = 0, 2, K_FAN, 150, 64
    deg[8], deg[9] = 65, 3
    dst = np.repeat(np.arange(N_NODES), deg).astype(np.int64)
    src = rng.integers(0, N_NODES, dst.size).astype(np.int64)
    et = rng.integers(0, 7, dst.size).astype(np.int64)
    nt = rng.integers(0, 4, N_NODES).astype(np.int64)
    rg = RelGraph(torch.from_numpy(src), torch.from_numpy(dst), N_NODES, DEV)
    assert np.array_equal(rg.csr_eid.cpu().numpy(), np.arange(dst.size))
    _SG.update(rg=rg, src=src, dst=dst, et=et, nt=nt, deg=deg,
               ptr=rg.csr_ptr.cpu().numpy().astype(np.int64))
    return _SG


def _sampler(g, sizes, cap=64, **kw):
    from regnn_hip.ns import DeviceSampler
    return DeviceSampler(g["rg"], sizes, cap, etype=torch.from_numpy(g["et"]),
                         ntype=torch.from_numpy(g["nt"]), num_edge_types=7, **kw)


def _run(ds, batch, seed, bi):
    ds.set_seed(seed, 1, bi)
    ds.set_targets(torch.as_tensor(batch).to(DEV))
    e0 = int(ds.state[5])
    ds.run_hops()
    torch.cuda.synchronize()
    return e0


def _assert_block_is_oracle(g, ds, batch, sizes, seed, bi, e0):
    L_ = len(sizes)
    _, rn_id, radjs = SO.neighbor_sample(g["ptr"], g["src"], list(batch), sizes, seed, epoch=1,
                                         batch_idx=bi)
    sz = ds.sizes.cpu().numpy()
    total = 0
    for h in range(L_):
        s, d, e, (n_src, n_dst) = radjs[L_ - 1 - h]
        s, d, e = (np.asarray(v, np.int64) for v in (s, d, e))
        blk, cap = ds.blocks[h], ds.caps[h]
        assert blk.self_loops is False
        assert sz[h] == n_dst and sz[h + 1] == n_src and sz[8 + h] == s.size
        cnt = np.bincount(d, minlength=n_dst)
        ptr = np.concatenate([[0], np.cumsum(cnt)])
        got_ptr = blk.csr_ptr.cpu().numpy()
        assert np.array_equal(got_ptr[:n_dst + 1], ptr)
        assert np.all(got_ptr[n_dst:cap + 1] == s.size)         # the padded rows are empty
        E = s.size
        assert np.array_equal(blk.csr_idx[:E].cpu().numpy(), s)
        assert np.array_equal(blk.row[:E].cpu().numpy(), d)
        assert np.array_equal(blk.pos[:E].cpu().numpy(), e)      # ascending CSR positions
        assert np.array_equal(blk.rel[:E].cpu().numpy(), g["et"][e])
        assert np.array_equal(ds.hop_bufs[h]["gsrc"][:E].cpu().numpy(), g["src"][e])
        inv = blk.inv.cpu().numpy()
        want_inv = np.ones(cap, np.float32)
        want_inv[:n_dst] = np.float32(1.0) / np.maximum(cnt, 1).astype(np.float32)
        assert np.array_equal(inv, want_inv)
        total += E
    assert ds.n_id[:sz[L_]].cpu().tolist() == list(rn_id)
    assert int(ds.state[5]) - e0 == total
    return radjs


@pytest.mark.parametrize("sizes", [[5, 3], [64]])
def test_loopless_sampler_is_the_oracle_bit_for_bit(sizes):
    g = _sampler_graph()
    ds = _sampler(g, sizes, self_loops=False)
    rng = np.random.default_rng(2)
    first = np.arange(37)
    second = np.concatenate([[6, 0, 7], rng.permutation(np.arange(10, N_NODES))[:34]])
    for bi, batch in enumerate([first, second]):         # two batches: the stamps advance
        e0 = _run(ds, batch, 17, bi)
        radjs = _assert_block_is_oracle(g, ds, batch.tolist(), sizes, 17, bi, e0)
        if bi == 0:                                       # the degree classes are all there
            cnt = np.bincount(np.asarray(radjs[-1][1]), minlength=37)
            k = sizes[0]
            assert (cnt[:4] == 0).all() and cnt[6] == k and (cnt < k).any() and (cnt == k).any()
            assert g["deg"][5] == K_FAN and g["deg"][6] > 64
    assert int(ds.sizes[0]) == 37 < ds.caps[0]
    # one zero-in-degree target: a valid block without any entry
    e0 = _run(ds, np.array([2]), 17, 2)
    _assert_block_is_oracle(g, ds, [2], sizes, 17, 2, e0)
    sz = ds.sizes.cpu().tolist()
    assert sz[0] == 1 and sz[1] == 1 and sz[8] == 0
    assert not ds.blocks[0].csr_ptr.any()


@pytest.mark.parametrize("sizes", [[5, 3], [64]])
def test_default_sampler_minus_its_loops_is_the_loopless_block(sizes):
    g = _sampler_graph()
    a, b = _sampler(g, sizes), _sampler(g, sizes, self_loops=False)
    batch = np.arange(37)
    for ds in (a, b):
        _run(ds, batch, 23, 4)
    assert a.blocks[0].self_loops is True
    sa, sb = a.sizes.cpu().tolist(), b.sizes.cpu().tolist()
    for h in range(len(sizes)):
        assert sa[h] == sb[h] and sa[h + 1] == sb[h + 1] and sa[8 + h] == sb[8 + h] + sa[h]
        Ea, Eb = sa[8 + h], sb[8 + h]
        x, y = a.blocks[h], b.blocks[h]
        keep = x.pos[:Ea] >= 0
        assert int(keep.sum()) == Eb
        for name in ("csr_idx", "rel", "pos", "row"):
            assert torch.equal(getattr(x, name)[:Ea][keep], getattr(y, name)[:Eb]), name
        n = sa[h]
        pa, pb = x.csr_ptr[:n + 1].long(), y.csr_ptr[:n + 1].long()
        assert torch.equal(pa - torch.arange(n + 1, device=DEV), pb)
    assert a.n_id[:sa[len(sizes)]].tolist() == b.n_id[:sb[len(sizes)]].tolist()


# ---------------------------------------------------------------------------------------------
# 3. the convs on loop-less blocks
# ---------------------------------------------------------------------------------------------
def _noloop_fixture_block(d, cap_dst=B.CAP_DST, cap_src=B.CAP_SRC):
    """the fixture's edges as a padded loop-less block (stable sort by dst, nothing appended)"""
    m = d["meta"]
    order = np.argsort(d["dst"], kind="stable")
    cnt = np.bincount(d["dst"], minlength=m["n_dst"])
    ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    blk = B._pad(ptr, d["src"][order], d["edge_type"][order], cap_dst, cap_src)
    return _as_nsblock(blk, cnt, cap_dst)


def _as_nsblock(blk, cnt, cap_dst, self_loops=False):
    inv = np.ones(cap_dst, np.float32)
    inv[:len(cnt)] = 1.0 / np.maximum(cnt, 1)
    blk = blk.to(DEV)
    blk.inv = torch.from_numpy(inv).to(DEV)
    blk.self_loops = self_loops
    return blk


def _conv(kind, d, self_loop_type=3):
    from regnn_hip import mag
    m = d["meta"]
    H, C = m["heads"], m["out_channels"]
    if kind == "regcn":
        conv = mag.REGCNConv(64, 64, m["num_node_types"], m["num_edge_types"],
                             m["scaling_factor"], residual=m["residual"], use_norm=m["use_norm"],
                             self_loop_type=self_loop_type)
    else:
        cls = mag.REGATv2Conv if kind == "regatv2" else mag.REGATConv
        conv = cls(H * C, C, m["num_node_types"], m["num_edge_types"], heads=H,
                   scaling_factor=m["scaling_factor"], residual=m["residual"],
                   use_norm=m["use_norm"], self_loop_type=self_loop_type)
    if self_loop_type != 2:                  # (type 2: num_node_types more relation weights)
        P = G.sub(d, "p_", np.float32)
        assert {n for n, _ in conv.named_parameters()} == set(P)
        with torch.no_grad():
            for n, p in conv.named_parameters():
                p.copy_(torch.from_numpy(P[n]))
    return conv.to(DEV)


@pytest.mark.parametrize("kind", KINDS)
def test_conv_on_loopless_block_matches_fixture_and_exact_path(kind):
    d = G.load(CONV_FIXTURES[kind])
    m = d["meta"]
    assert m["self_loop_type"] == 3 and d["empty"].size >= 3
    n_src, n_dst = m["n_src"], m["n_dst"]
    blk = _noloop_fixture_block(d)
    conv = _conv(kind, d)
    assert conv.relation_weight.shape[0] == m["num_edge_types"]
    x = torch.full((blk.n_src, d["x"].shape[1]), 1e3, device=DEV)
    x[:n_src] = torch.from_numpy(d["x"]).to(DEV)
    x.requires_grad_(True)
    out = conv((x, x[:blk.n_dst]), blk)
    gout = torch.zeros(blk.n_dst, out.shape[1], device=DEV)
    gout[:n_dst] = torch.from_numpy(d["gout"]).to(DEV)
    out.backward(gout)
    got = {"out": out[:n_dst].detach(), "x": x.grad[:n_src].clone()}
    got.update({n: p.grad.clone() for n, p in conv.named_parameters()})
    assert not x.grad[n_src:].any()
    want = {"out": d["out"], **G.sub(d, "grad_")}
    assert set(want) == set(got)
    conv.zero_grad()
    x2 = torch.from_numpy(d["x"]).to(DEV).requires_grad_(True)
    ei = torch.from_numpy(np.stack([d["src"], d["dst"]])).to(DEV)
    out2 = conv((x2, x2[:n_dst]), ei, torch.from_numpy(d["edge_type"]).to(DEV),
                torch.from_numpy(d["target_node_type"]).to(DEV))
    out2.backward(torch.from_numpy(d["gout"]).to(DEV))
    exact = {"out": out2.detach(), "x": x2.grad}
    exact.update({n: p.grad for n, p in conv.named_parameters()})
    for k in want:
        _check(f"{kind} {k} vs fixture", got[k], want[k])
        _check(f"{kind} {k} vs exact-size path", got[k], exact[k])


# the loop-less ladder: _ns_gat_blocks' lengths and rows of 0 entries (first, in the middle, last)
NL_LENGTHS = [0] + B.LADDER_LENGTHS + [0]
_NL = {}


def _noloop_ladder():
    if _NL:
        return _NL["cpu"], _NL["dev"]
    c = B.LADDER
    rng = np.random.default_rng(9)
    lens = [NL_LENGTHS[v % len(NL_LENGTHS)] for v in range(c["live_dst"])]
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    E = int(ptr[-1])
    idx = rng.integers(0, c["live_src"], E).astype(np.int64)
    rel = rng.integers(0, c["n_edge_types"], E).astype(np.int64)
    cpu = B._pad(ptr, idx, rel, c["cap_dst"], c["cap_src"])
    _NL["cpu"], _NL["dev"] = cpu, _as_nsblock(cpu, np.asarray(lens), c["cap_dst"])
    _NL["empty"] = [v for v, n in enumerate(lens) if n == 0]
    return _NL["cpu"], _NL["dev"]


@pytest.mark.parametrize("H,C", [(2, 32), (8, 64), (3, 8)])
def test_ns_gat_on_loopless_ladder_matches_fp64_per_element(H, C):
    from regnn_hip import ops
    c = B.LADDER
    cpu, dev = _noloop_ladder()
    ft, el, er, tab, gy, slope = R.gat_inputs("unit", c["cap_src"], H, C, c["n_edge_types"],
                                              seed=300 + 7 * H + C)
    er, gy = er[:c["cap_dst"]].clone(), gy[:c["cap_dst"]].clone()
    gy[c["live_dst"]:] = 0.0
    ptr, idx, rel = cpu.live()
    want, scale = R.gat_case_ref(ptr, idx, rel, el, er, tab, ft, gy, slope,
                                 global_max="detached")
    leaves = [t.to(DEV).requires_grad_(True) for t in (el, er, tab, ft)]
    out = ops.ns_gat(dev, *leaves, slope)
    out.backward(gy.to(DEV))
    got = {"out": out, "g_el": leaves[0].grad, "g_er": leaves[1].grad, "g_tab": leaves[2].grad,
           "g_ft": leaves[3].grad}
    assert len(_NL["empty"]) >= 3 and not out[_NL["empty"]].any()    # the zero attention term
    assert not out[c["live_dst"]:].any() and not got["g_er"][_NL["empty"]].any()
    for k in ("out", "g_ft", "g_el", "g_er", "g_tab"):
        err = R.rel_err(got[k].detach().cpu(), want[k], scale[k])
        print(f"ns_gat loop-less H={H} C={C} {k}: {err:.2e}")
        assert err <= R.TOL_F32, f"{k}: {err:.3e}"


@pytest.mark.parametrize("H,C", [(2, 32), (8, 64), (3, 8)])
def test_ns_gatv2_on_loopless_ladder_matches_fp64_per_element(H, C):
    from regnn_hip import ops
    c = B.LADDER
    cpu, dev = _noloop_ladder()
    fs, fd, att, tab, _ft, gy, slope = R.gatv2_inputs("unit", c["cap_src"], H, C,
                                                      c["n_edge_types"], seed=400 + 7 * H + C)
    xd, gy = fd[:c["cap_dst"]].clone(), gy[:c["cap_dst"]].clone()
    gy[c["live_dst"]:] = 0.0
    ptr, idx, rel = cpu.live()
    w, s = R.gatv2_case_ref(ptr, idx, rel, fs, xd, att, tab, fs, gy, slope,
                            global_max="detached")
    want = {"out": w["out"], "g_xs": w["g_fs"] + w["g_ft"], "g_xd": w["g_fd"],
            "g_att": w["g_att"], "g_tab": w["g_tab"]}
    scale = {"out": s["out"], "g_xs": s["g_fs"] + s["g_ft"], "g_xd": s["g_fd"],
             "g_att": s["g_att"], "g_tab": s["g_tab"]}
    leaves = [t.to(DEV).requires_grad_(True) for t in (fs, xd, att, tab)]
    out = ops.ns_gatv2(dev, *leaves, slope)
    out.backward(gy.to(DEV))
    got = dict(zip(("out", "g_xs", "g_xd", "g_att", "g_tab"), [out] + [t.grad for t in leaves]))
    assert not out[_NL["empty"]].any() and not out[c["live_dst"]:].any()
    assert not got["g_xd"][_NL["empty"]].any()
    for k, v in got.items():
        err = R.rel_err(v.detach().cpu(), want[k], scale[k])
        print(f"ns_gatv2 loop-less H={H} C={C} {k}: {err:.2e}")
        assert err <= R.TOL_F32, f"{k}: {err:.3e}"


@pytest.mark.parametrize("kind", KINDS)
def test_convs_refuse_a_block_of_the_other_form(kind):
    d = G.load(CONV_FIXTURES[kind])
    blk = _noloop_fixture_block(d)
    x = torch.zeros(blk.n_src, d["x"].shape[1], device=DEV)
    with pytest.raises(ValueError, match="self_loop_type 2.*self_loops=False"):
        _conv(kind, d, self_loop_type=2)((x, x[:blk.n_dst]), blk)
    looped = _noloop_fixture_block(d)
    looped.self_loops = True                 # (only the flag: the conv refuses before any launch)
    for slt in (1, 3):
        with pytest.raises(ValueError, match=f"self_loop_type {slt}.*self_loops=True"):
            _conv(kind, d, self_loop_type=slt)((x, x[:blk.n_dst]), looped)


# ---------------------------------------------------------------------------------------------
# 4. / 5. the trainer
# ---------------------------------------------------------------------------------------------
_FX = {}


def _fx(kind, slt):
    """an nssl_regnn_* fixture on the device, loaded once"""
    key = (kind, slt)
    if key not in _FX:
        from regnn_hip.graph import RelGraph
        d = G.load(f"nssl_regnn_{kind}_sl{slt}")
        m = d["meta"]
        N = int(sum(m["counts"]))
        d["rg"] = RelGraph(torch.from_numpy(d["src"]), torch.from_numpy(d["dst"]), N, DEV)
        d["x_dict"] = {t: torch.from_numpy(d[f"x{t}"]).to(DEV) for t in range(4)}
        d["nt"] = torch.from_numpy(d["ntype"]).to(DEV)
        d["loc"] = torch.from_numpy(d["local"]).to(DEV)
        d["et"] = torch.from_numpy(d["edge_type"]).to(DEV)
        d["N"] = N
        _FX[key] = d
    return _FX[key]


def _fx_model(d, use_norm="ln", hidden=None):
    """the fixture's model with its parameters; another norm or width: a seeded model"""
    from regnn_hip import mag
    m = d["meta"]
    K = m["in_channels"]
    torch.manual_seed(0)
    model = mag.REGNN(K, hidden or m["hidden"], m["classes"], m["num_layers"], m["scaling_factor"], 0.0,
                      {t: K for t in range(4)}, m["num_edge_types"], residual=m["residual"],
                      use_norm=use_norm, self_loop_type=m["self_loop_type"], model=m["kind"],
                      heads=m["heads"], feats_type=m["feats_type"])
    if use_norm == "ln" and hidden is None:
        P = G.sub(d, "p_", np.float32)
        assert {n for n, _ in model.named_parameters()} == set(P)
        with torch.no_grad():
            for n, p in model.named_parameters():
                p.copy_(torch.from_numpy(P[n]))
    return model.to(DEV)


def _fx_trainer(d, model, **kw):
    from regnn_hip.ns import NSTrainer
    m = d["meta"]
    batch = torch.from_numpy(d["batch"]).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2, capturable=True)
    return NSTrainer(model, opt, d["rg"], m["sizes"], len(d["batch"]), batch, d["x_dict"],
                     d["et"], d["nt"], d["loc"], torch.from_numpy(d["y"]).to(DEV).view(-1, 1),
                     m["num_edge_types"], seed=m["seed"], shuffle=False, device_blocks=True, **kw)


@pytest.mark.parametrize("slt", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_trainer_step_on_loopless_blocks_vs_reference(kind, slt):
    """the loop-less sampler reproduces the fixture's batch; one NSTrainer(device_blocks=True)
    module step on it gives the reference REGNN's loss and every gradient"""
    d = _fx(kind, slt)
    m = d["meta"]
    assert m["self_loop_type"] == slt and m["num_edge_types"] == (11 if slt == 1 else 7)
    model = _fx_model(d)
    model.eval()                                     # dropout 0, LayerNorm: as the fixture ran
    tr = _fx_trainer(d, model)
    assert tr.fused is None and tr._blocks_ok and tr._noloop and tr.pipelined
    assert tr.ahead == 1 and len(tr.slots) == 2
    assert all(not s.self_loops and not s.strided and s.csc[0] is None for s in tr.slots)
    s = tr.slots[0]
    s.set_seed(m["seed"], m["epoch"], m["batch_idx"])
    s.set_targets(torch.from_numpy(d["batch"]).to(DEV))
    e0 = tr.edges_total()
    tr._run_hops(0)
    L_ = len(m["sizes"])
    for h in range(L_):                              # hop h's block = the fixture's adjs
        n_src, n_dst = (int(v) for v in d[f"adj{L_ - 1 - h}_size"])
        assert int(s.sizes[h]) == n_dst and int(s.sizes[h + 1]) == n_src
        assert int(s.sizes[8 + h]) == d[f"adj{L_ - 1 - h}_src"].size
        blk = s.blocks[h]
        assert blk.self_loops is False and blk.live_rows is not None
        if slt == 3:                                 # a live target without a sampled in-edge
            p = blk.csr_ptr[:n_dst + 1].cpu().numpy()
            empty = np.nonzero(np.diff(p) == 0)[0]
            assert np.array_equal(empty, d[f"empty{L_ - 1 - h}"]) and empty.size >= 1
    assert s.n_id[:int(s.sizes[L_])].cpu().tolist() == d["n_id"].tolist()
    assert tr.edges_total() - e0 == sum(d[f"adj{h}_src"].size for h in range(L_))
    tr._module_step(s)
    torch.cuda.synchronize()
    _check(f"{kind} sl{slt} loss", tr.loss, d["loss"])
    got = {n: p.grad for n, p in model.named_parameters()}
    for k, v in G.sub(d, "grad_").items():
        _check(f"{kind} sl{slt} {k}", got[k], v)


_MAG = {}


def _mag(slt):
    """test_gpu_ns_gat._mag's graph; type 1: with its self-loop relations (num_edge_types 11)"""
    if slt in _MAG:
        return _MAG[slt]
    import test_gpu_ns_gat as T
    from regnn_hip import mag
    from regnn_hip.graph import RelGraph
    d = dict(T._mag())
    d["n_et"] = 7
    if slt == 1:
        rg = d["rg"]
        # the caller-order edge list back from the CSR (edge csr_eid[p] sits at position p)
        eid = rg.csr_eid.long()
        ptr = rg.csr_ptr.long()
        ei = torch.empty(2, rg.E, dtype=torch.int64, device=DEV)
        ei[0, eid] = rg.csr_idx.long()
        ei[1, eid] = torch.repeat_interleave(torch.arange(ptr.numel() - 1, device=DEV),
                                             ptr[1:] - ptr[:-1])
        ei, et, n_et = mag.add_self_loop_relations(ei, d["edge_type"], d["node_type"], 7)
        assert n_et == 11 and ei.shape[1] == rg.E + d["node_type"].numel()
        d.update(rg=RelGraph(ei[0], ei[1], d["node_type"].numel(), DEV), edge_type=et, n_et=n_et)
    _MAG[slt] = d
    return d


def _mag_model(d, kind, slt, **kw):
    from regnn_hip import mag
    torch.manual_seed(0)
    kw = {"use_norm": "ln", "residual": True, **kw}
    return mag.REGNN(16, 8, 5, 2, 10.0, 0.0, {k: 16 for k in d["x_dict"]}, d["n_et"], model=kind,
                     heads=2, self_loop_type=slt, **kw).to(DEV)


def _mag_trainer(d, model, train_idx=None, **kw):
    from regnn_hip.ns import NSTrainer
    opt = torch.optim.Adam(model.parameters(), lr=1e-2, capturable=True)
    idx = torch.arange(d["n_paper"], device=DEV) if train_idx is None else train_idx
    return NSTrainer(model, opt, d["rg"], [6, 4], 64, idx, d["x_dict"], d["edge_type"],
                     d["node_type"], d["local"], d["y"], d["n_et"], seed=3, **kw)


def _step_vs_exact_path(d, kind, slt, n_train, **model_kw):
    from regnn_hip import mag
    from regnn_hip.sampler import NeighborSampler
    idx = torch.arange(d["n_paper"] if n_train is None else n_train, device=DEV)
    m_api, m_eng = _mag_model(d, kind, slt, **model_kw), _mag_model(d, kind, slt, **model_kw)
    m_api.train(); m_eng.train()
    smp = NeighborSampler(d["rg"], idx, [6, 4], batch_size=64, shuffle=True, seed=3)
    batch = next(iter(smp))
    assert getattr(batch[2][0], "block", None) is None         # the exact-size path
    loss_api = mag.train_step(m_api, torch.optim.SGD(m_api.parameters(), lr=0.0), batch,
                              d["x_dict"], d["edge_type"], d["node_type"], d["local"], d["y"], 1)
    tr = _mag_trainer(d, m_eng, train_idx=idx, device_blocks=True)
    assert tr._noloop and tr.fused is None and tr.pipelined and len(tr.slots) == 2
    tr._forward_backward()
    torch.cuda.synchronize()
    tag = f"{kind} sl{slt} n_train={n_train} {model_kw}"
    _check(f"{tag} loss", tr.loss, loss_api.detach())
    assert int(tr.sampler.sizes[0]) == (64 if n_train is None else n_train)
    gp = dict(m_api.named_parameters())
    for n, p in m_eng.named_parameters():
        if gp[n].grad is None:                 # declared, unused in forward (REGNN.norm)
            assert not p.grad.any(), n
            continue
        _check(f"{tag} {n}", p.grad, gp[n].grad)


@pytest.mark.parametrize("n_train", [None, 37])
@pytest.mark.parametrize("slt", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_trainer_loopless_blocks_match_exact_size_path(kind, slt, n_train):
    _step_vs_exact_path(_mag(slt), kind, slt, n_train)


@pytest.mark.parametrize("slt", [1, 3])
def test_trainer_loopless_regcn_with_batch_norm_matches_exact_size_path(slt):
    _step_vs_exact_path(_mag(slt), "regcn", slt, 37, use_norm="bn")


@pytest.mark.parametrize("slt", [1, 3])
def test_trainer_loopless_regcn_wide_epilogue_matches_exact_size_path(slt):
    """hidden 128 on 64-wide tables: the typed first layer in its plain form (ops.ns_typed_agg by
    n_id) and the one-launch LayerNorm epilogue (ops.wide_ln_act) on loop-less blocks, against the
    exact-size path on the same batch of the fixture's graph (for type 3 with an empty row)"""
    from regnn_hip import mag
    from regnn_hip.sampler import NeighborSampler
    d = _fx("regcn", slt)
    m = d["meta"]
    m_api, m_eng = _fx_model(d, hidden=128), _fx_model(d, hidden=128)
    m_api.train(); m_eng.train()
    idx = torch.from_numpy(d["batch"]).to(DEV)
    y = torch.from_numpy(d["y"]).to(DEV).view(-1, 1)
    smp = NeighborSampler(d["rg"], idx, m["sizes"], batch_size=len(d["batch"]), shuffle=False,
                          seed=m["seed"])
    batch = next(iter(smp))
    loss_api = mag.train_step(m_api, torch.optim.SGD(m_api.parameters(), lr=0.0), batch,
                              d["x_dict"], d["et"], d["nt"], d["loc"], y, 1)
    tr = _fx_trainer(d, m_eng)
    assert tr._noloop and tr.fused is None
    blk0 = tr.slots[0].model_blocks()[0]
    assert m_eng._wide_epi(blk0) is not None                   # the wide epilogue is what runs
    tr._forward_backward()
    torch.cuda.synchronize()
    assert tr.sampler.n_id[:int(tr.sampler.sizes[2])].tolist() == batch[1].tolist()
    _check(f"regcn sl{slt} hidden 128 loss", tr.loss, loss_api.detach())
    gp = dict(m_api.named_parameters())
    for n, p in m_eng.named_parameters():
        if gp[n].grad is None:
            assert not p.grad.any(), n
            continue
        _check(f"regcn sl{slt} hidden 128 {n}", p.grad, gp[n].grad)


@pytest.mark.parametrize("slt", [1, 3])
@pytest.mark.parametrize("kind", ["regat", "regatv2"])
def test_gather_backward_gives_the_same_bits_on_loopless_blocks(kind, slt, monkeypatch):
    from regnn_hip import ops
    monkeypatch.setitem(ops.NS_GAT_SRC, "mode", "gather")
    monkeypatch.setitem(ops.SMALL_BLAS, "mode", "off")         # the deterministic x6 GEMM
    d = _mag(slt)
    flats = []
    for _ in range(2):
        tr = _mag_trainer(d, _mag_model(d, kind, slt), device_blocks=True)
        assert tr._gat_src_gather and all(t is not None for s in tr.slots for t in s.tidx)
        tr._forward_backward()
        torch.cuda.synchronize()
        flats.append((float(tr.loss), tr.flat.clone()))
    assert flats[0][1].any() and bool(torch.isfinite(flats[0][1]).all())
    assert flats[0][0] == flats[1][0]
    assert torch.equal(flats[0][1], flats[1][1])


@pytest.mark.parametrize("kind", ["regcn", "regat"])
def test_trainer_loopless_capture_and_replay(kind):
    d = _mag(3)
    tr_e = _mag_trainer(d, _mag_model(d, kind, 3), device_blocks=True)
    tr_g = _mag_trainer(d, _mag_model(d, kind, 3), device_blocks=True)
    tr_g.capture(warmup=1)                     # a host sync inside the capture would raise
    assert not tr_g.graph_groups               # one-step graphs only
    le, lg = [], []
    for _ in range(6):
        tr_e.step()
        le.append(float(tr_e.loss))
        tr_g.replay()
        lg.append(float(tr_g.loss))
    print(kind, "eager", le, "replayed", lg)
    assert np.all(np.isfinite(lg))
    assert np.allclose(le, lg, rtol=1e-4, atol=1e-5), (le, lg)
    assert tr_g.edges_total() > 0


def test_without_device_blocks_the_model_keeps_the_exact_size_path():
    d = _mag(3)
    tr = _mag_trainer(d, _mag_model(d, "regcn", 3))
    assert not tr._blocks_ok and not tr._noloop and tr.slots[0].self_loops


# ---------------------------------------------------------------------------------------------
# 6. inference
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slt", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_inference_matches_forward_over_full_neighbour_adjs(kind, slt):
    from regnn_hip.sampler import NeighborSampler
    d = _fx(kind, slt)
    model = _fx_model(d).eval()
    loader = NeighborSampler(d["rg"], None, [-1], batch_size=4096, shuffle=False)
    out = model.inference(d["x_dict"], loader, d["et"], d["nt"], d["loc"], DEV)
    assert out.shape == (d["N"], d["meta"]["classes"]) and bool(torch.isfinite(out).all())
    deg = np.diff(d["rg"].csr_ptr.cpu().numpy())
    idx = torch.from_numpy(d["batch"]).to(DEV)
    if slt == 3:                                     # a node without in-edges among the rows
        assert (deg[d["batch"]] == 0).any()
    else:
        assert deg.min() >= 1                        # type 1: every node has its loop edge
    smp = NeighborSampler(d["rg"], idx, [-1, -1], batch_size=16, shuffle=False)
    seen = 0
    with torch.no_grad():
        for k, (bs, n_id, adjs) in enumerate(smp):
            z = model(n_id, d["x_dict"], adjs, d["et"], d["nt"], d["loc"], logits=True)
            _check(f"{kind} sl{slt} batch {k}", out[n_id[:bs]], z)
            seen += bs
    assert seen == idx.numel()


@pytest.mark.parametrize("slt", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_sharded_inference_two_ranks_in_lockstep_equal_one(kind, slt):
    from regnn_hip.inference import ShardedInference, shard_bounds
    d = _fx(kind, slt)
    model = _fx_model(d).eval()
    args = (model, d["rg"], d["et"], d["nt"], d["loc"])
    W = 2
    bounds = shard_bounds(d["rg"].csr_ptr, W)
    ranks = [ShardedInference(*args, r, W, bounds) for r in range(W)]
    assert all(r.block.self_loops is False for r in ranks)
    xs = [s.input(d["x_dict"], 0)[1] for s in ranks]
    for layer in range(model.num_layers):
        xs_all = torch.cat(xs, 0)                        # what exchange_rows returns
        if kind == "regcn":
            xl = [s.aggregate(layer, xs_all, xr) for s, xr in zip(ranks, xs)]
        else:
            st = [s.attention_scores(layer, xs_all, xr) for s, xr in zip(ranks, xs)]
            gmax = torch.stack([t.gmax for t in st]).amax(0)  # the MAX all-reduce
            xl = [s.attention_finish(layer, t, xr, gmax=gmax) for s, t, xr in zip(ranks, st, xs)]
        if layer + 1 < model.num_layers:
            xs = [s.project(layer + 1, x) for s, x in zip(ranks, xl)]
    out = torch.cat([s.head(x) for s, x in zip(ranks, xl)], 0)
    one = ShardedInference(*args).run(d["x_dict"])
    assert bool(torch.isfinite(one).all())
    _check(f"{kind} sl{slt}: two ranks against one", out, one)


# ---------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------
def test_fused_engine_and_bf16_tables_are_refused_with_a_reason():
    d = _mag(3)
    with pytest.raises(ValueError, match="fused"):
        _mag_trainer(d, _mag_model(d, "regcn", 3), device_blocks=True, engine="fused")
    b = dict(d)
    b["x_dict"] = {k: v.bfloat16() for k, v in d["x_dict"].items()}
    for kind in KINDS:
        with pytest.raises(ValueError, match="fp32 input tables"):
            _mag_trainer(b, _mag_model(b, kind, 3), device_blocks=True)


@pytest.mark.parametrize("slt", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_knob_off_keeps_the_refusals(kind, slt, monkeypatch):
    from regnn_hip import mag
    from regnn_hip.inference import ShardedInference
    monkeypatch.setitem(mag.NOLOOP_BLOCKS, "mode", "off")
    d = _mag(3)                                  # (type 1's model on 7 relations: refused first)
    with pytest.raises(ValueError, match="device_blocks=True does not cover"):
        _mag_trainer(d, _mag_model(d, kind, slt), device_blocks=True)
    tr = _mag_trainer(d, _mag_model(d, kind, slt))           # the exact-size path as before
    assert not tr._blocks_ok and not tr._noloop and tr.slots[0].self_loops
    f = _fx(kind, slt)
    with pytest.raises(NotImplementedError, match="REGNN_NOLOOP_BLOCKS"):
        ShardedInference(_fx_model(f), f["rg"], f["et"], f["nt"], f["loc"])
    monkeypatch.setitem(mag.NOLOOP_BLOCKS, "mode", "maybe")
    with pytest.raises(ValueError, match="'on' or 'off'"):
        _mag_trainer(d, _mag_model(d, kind, slt), device_blocks=True)


def test_loopless_sampler_refuses_what_it_does_not_write():
    g = _sampler_graph()
    ds = _sampler(g, [5, 3], self_loops=False)
    ds.set_seed(1, 0, 0)
    ds.set_targets(torch.arange(8, device=DEV))
    with pytest.raises(ValueError, match="fixed-stride"):
        ds.run_hops(strided=True)
    with pytest.raises(ValueError, match="transposed index"):
        ds.enable_csc(0)
    with pytest.raises(ValueError, match="edge meta"):
        ds.enable_edge_meta(torch.arange(N_NODES), 1)
    ds.hop_strided[0] = True
    with pytest.raises(ValueError, match="fixed-stride"):
        ds.run_hops()
    ds.hop_strided[0] = None
    ds.typed_sums[1] = {}
    with pytest.raises(ValueError, match="input sums"):
        ds.run_hops()
