"""The sampler's sums launch with the type layout (regnn_ns_type_layout: a slot's source type,
table row and relation computed from its node id) on a hand-built typed graph of 48 nodes
(test_ns_type_layout.hand_graph): bitwise against the table-reading launch, and against numpy
fp64 sums over the edges the sampler oracle draws; and the fall-back to the tables on graphs
without the layout."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _golden as G  # noqa: E402
from oracle import sampler_oracle as SO  # noqa: E402
from test_ns_type_layout import SEED, hand_graph  # noqa: E402

DEV = "cuda:0"
K = 128
FANOUTS = [(3, 3), (3, 33)]                    # the outer hop: 32 lanes per row / 64 lanes


def _case(g):
    """the graph on the device, its tables (one per type, fixed values) and a REGNN-2 model."""
    from regnn_hip.graph import RelGraph
    rg = RelGraph(g["src"], g["dst"], g["N"], DEV)
    gen = torch.Generator().manual_seed(5)
    x = {t: torch.randn(c, K, generator=gen).to(DEV) for t, c in enumerate(g["counts"])}
    y = torch.full((g["N"], 1), -1, dtype=torch.int64, device=DEV)
    n0 = g["counts"][0]
    y[:n0, 0] = (torch.arange(n0, device=DEV) * 7) % 5
    if "y_of" in g:                            # (permuted ids: the labels follow their nodes)
        y = y[torch.from_numpy(g["y_of"]).to(DEV)]
    return dict(g=g, rg=rg, x=x, y=y, etype=torch.from_numpy(g["etype"]).to(DEV),
                ntype=torch.from_numpy(g["ntype"]).to(DEV),
                local=torch.from_numpy(g["local"]).to(DEV))


def _trainer(c, sizes, seed_model=3):
    from regnn_hip import mag
    from regnn_hip.ns import NSTrainer
    g = c["g"]
    torch.manual_seed(seed_model)
    m = mag.REGNN(K, 64, 5, 2, 10.0, 0.5, {t: K for t in c["x"]}, g["R"], use_norm="ln",
                  self_loop_type=2).to(DEV)
    with torch.no_grad():
        for conv in m.convs:
            conv.relation_weight.copy_(torch.linspace(0.02, 0.12, g["R"] + 4, device=DEV))
            conv.bias.normal_(0, 0.1)
    m.train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-2, capturable=True)
    # every node a target of the one batch (labels: the type-0 nodes), in id order
    tr = NSTrainer(m, opt, c["rg"], list(sizes), g["N"], torch.arange(g["N"], device=DEV), c["x"],
                   c["etype"], c["ntype"], c["local"], c["y"], g["R"], seed=SEED, shuffle=False,
                   pipeline=False)
    assert tr.fused is not None and tr.fused.W.pre_sums
    return tr, m


def _sums(tr):
    W = tr.fused.W
    n1 = int(tr.sampler.sizes[1])
    s = tr.sampler
    out = [tr.fused._buf(a)[:n1].clone() for a in (W.s_agg, W.s_w, W.u_self, W.u_rel)]
    return out + [s.hop_bufs[1]["scnt"][:n1].clone(), s.blocks[1].inv[:n1].clone()], n1


NAMES = ("s_agg", "s_w", "u_self", "u_rel", "scnt", "inv")


def _oracle_sums(c, k0, k1):
    """hop 0's n_id and, per row of the outer hop, the fp64 per-type sums, counts, self row, slot
    relations, in-count and 1/(in-count + 1) over the edges the sampler oracle draws."""
    g, rg = c["g"], c["rg"]
    ptr, idx, eid = (t.cpu().numpy() for t in (rg.csr_ptr, rg.csr_idx, rg.csr_eid))
    n_id, _, _, _ = SO.sample_hop(ptr, idx, list(range(g["N"])), k0, SO.hop_seed(SEED, 0, 0, 0))
    seed = SO.hop_seed(SEED, 0, 0, 1)
    x = {t: v.double().cpu().numpy() for t, v in c["x"].items()}
    n1, T, R = len(n_id), 4, g["R"]
    S, w = np.zeros((n1, T, K)), np.zeros((n1, T))
    xs, ur = np.zeros((n1, K)), np.full((n1, T + 1), -1, dtype=np.int64)
    cnt = np.zeros(n1, dtype=np.int64)
    degs = set()
    for i, t in enumerate(n_id):
        srcs, pos = SO.sample_row(ptr, idx, int(t), k1, seed)
        d = int(ptr[t + 1] - ptr[t])
        degs.add(0 if d == 0 else 1 if d < k1 else 2 if d == k1 else 3)
        cnt[i] = len(srcs)
        for u, p in zip(srcs, pos):
            tt = int(g["ntype"][u])
            S[i, tt] += x[tt][int(g["local"][u])]
            w[i, tt] += 1
            r = int(g["etype"][eid[p]])
            assert ur[i, tt] in (-1, r)
            ur[i, tt] = r
        tt = int(g["ntype"][t])
        xs[i] = x[tt][int(g["local"][t])]
        ur[i, T] = R + tt
    assert degs == {0, 1, 2, 3}               # in-degree 0, < k, = k, > k (the Floyd path)
    return n_id, dict(s_agg=S, s_w=w, u_self=xs, u_rel=ur, scnt=cnt, inv=1.0 / (cnt + 1.0))


def _check_oracle(c, sizes, want_layout, monkeypatch):
    """set_seed / set_targets / run_hops on the trainer's sampler against _oracle_sums."""
    from regnn_hip import ns
    monkeypatch.setitem(ns.SUMS_META, "mode", "off")   # where it applies: no per-slot meta
    tr, _ = _trainer(c, sizes)
    s = tr.sampler
    assert (s.typed_sums[1]["layout"] is not None) == want_layout
    s.set_seed(SEED, 0, 0)
    s.set_targets(torch.arange(c["g"]["N"], device=DEV))
    s.run_hops()
    torch.cuda.synchronize()
    assert s.sums_fresh[1] and s.meta_fresh[1] == (not want_layout)
    got, n1 = _sums(tr)
    n_id, ref = _oracle_sums(c, *sizes)
    assert n1 == len(n_id) and s.n_id[:n1].cpu().tolist() == n_id
    for name, t in zip(NAMES, got):
        a = t.cpu().numpy()
        if name in ("s_agg", "u_self", "inv"):
            ok, err = G.close(a, ref[name], 1e-5)
            assert ok, f"{name}: rel err {err:.3e}"
        else:                                  # counts, slot relations: exact
            assert np.array_equal(a.astype(np.int64), ref[name].astype(np.int64)), name
    # the self rows are copies: exact
    assert np.array_equal(got[2].cpu().numpy(), ref["u_self"].astype(np.float32))
    return tr


@pytest.mark.parametrize("sizes", FANOUTS)
@pytest.mark.parametrize("meta", ["auto", "off"])
def test_type_layout_bitwise_equals_tables(monkeypatch, sizes, meta):
    """(a) the derived launch against the table-reading one on the same batch: sums, counts, self
    rows, slot relations, in-counts, 1/in-counts, the loss and every gradient bitwise equal
    (meta "off": the derived launch also leaves the per-slot meta out)."""
    from regnn_hip import ns
    c = _case(hand_graph())
    monkeypatch.setitem(ns.SUMS_META, "mode", meta)
    res = {}
    for mode in ("on", "off"):
        monkeypatch.setitem(ns.TYPE_LAYOUT, "mode", mode)
        tr, m = _trainer(c, sizes)
        assert (tr.sampler.typed_sums[1]["layout"] is not None) == (mode == "on")
        tr._forward_backward()
        torch.cuda.synchronize()
        assert tr.sampler.meta_fresh[1] == (not (mode == "on" and meta == "off"))
        bufs, n1 = _sums(tr)
        assert n1 >= c["g"]["N"]
        res[mode] = (tr.loss.clone(), [p.grad.clone() for p in m.parameters()], bufs)
    (la, ga, ba), (lb, gb, bb) = res["on"], res["off"]
    for name, x, y in zip(NAMES, ba, bb):
        assert torch.equal(x, y), name
    assert torch.equal(la, lb) and torch.isfinite(la)
    for x, y in zip(ga, gb):
        assert torch.equal(x, y)
    assert any(bool(x.any()) for x in ga)


@pytest.mark.parametrize("sizes", FANOUTS)
def test_type_layout_against_oracle(monkeypatch, sizes):
    """(b) independently of both kernels: the oracle's draws, numpy fp64 sums."""
    _check_oracle(_case(hand_graph()), sizes, True, monkeypatch)


def _permuted(g):
    perm = np.random.default_rng(0).permutation(g["N"])
    p = dict(g, src=perm[g["src"]], dst=perm[g["dst"]])
    for k in ("ntype", "local"):
        p[k] = np.empty_like(g[k])
        p[k][perm] = g[k]
    p["y_of"] = np.argsort(perm)              # new id -> old id
    return p


def _reversed_rows(g):
    w = dict(g, local=g["local"].copy())
    f = g["ntype"] == 2
    w["local"][f] = w["local"][f][::-1]
    return w


@pytest.mark.parametrize("variant", [_permuted, _reversed_rows])
@pytest.mark.parametrize("sizes", FANOUTS)
def test_no_layout_falls_back_to_tables(monkeypatch, sizes, variant):
    """node ids permuted (types interleave), or one type's table rows reversed: the setup function
    finds no layout, the launch reads the tables (and writes its meta), and the sums still equal
    the oracle's."""
    tr = _check_oracle(_case(variant(hand_graph())), sizes, False, monkeypatch)
    tr.fused.step()                            # the tables' meta is there for whoever reads it
    torch.cuda.synchronize()
    assert torch.isfinite(tr.loss)


def test_sums_grid_rounds_match_in_kernel_gather(monkeypatch):
    """more row groups than the GPU holds blocks at once (1024 x 17 = 17408 rows = 2176 groups
    against 1024 resident blocks on 256 CUs): the sums launch then runs 726 blocks of three rounds
    of row groups each. Sums, counts, self rows, slot relations, the loss and every gradient stay
    bitwise those of agg0's own gather (PRE_SUMS off) on the same batch."""
    from regnn_hip import ns
    from test_gpu_ns_engine import _mag, _setup_trainer
    d = _mag(0.3, seed=9, F=128, hidden=64, classes=29, dropout=0.5)
    res = {}
    for mode in ("on", "off"):
        monkeypatch.setitem(ns.PRE_SUMS, "mode", mode)
        m = d["model"](4)
        m.train()
        tr, _ = _setup_trainer(d, m, batch=1024, sizes=(16, 4))
        assert tr.sampler.caps[1] == 17408 and bool(tr.fused.W.pre_sums) == (mode == "on")
        tr._forward_backward()
        torch.cuda.synchronize()
        fs = tr.fused_slots[tr._trained] if tr.pipelined else tr.fused
        n1 = int(tr.sampler.sizes[1])
        W = fs.W
        res[mode] = (float(tr.loss), [p.grad.clone() for p in m.parameters()],
                     [fs._buf(a)[:n1].clone() for a in (W.s_agg, W.s_w, W.u_self, W.u_rel)])
    (la, ga, ba), (lb, gb, bb) = res["on"], res["off"]
    assert n1 > 726 * 8, n1                    # rows of the second round are live
    for x, y in zip(ba, bb):
        assert torch.equal(x, y)
    assert la == lb
    for x, y in zip(ga, gb):
        assert torch.equal(x, y)


def test_step_refuses_stale_sums(monkeypatch):
    """a batch sampled without the sums launch (run_hops(meta_only=False)) must not train on the
    previous batch's sums, with or without the per-slot meta."""
    from regnn_hip import ns
    monkeypatch.setitem(ns.SUMS_META, "mode", "off")
    tr, _ = _trainer(_case(hand_graph()), (3, 3))
    tr._forward_backward()
    s = tr.sampler
    assert not s.meta_fresh[1]
    s.set_seed(SEED, 0, 1)
    s.set_targets(torch.arange(48, device=DEV))
    s.run_hops(meta_only=False)
    with pytest.raises(RuntimeError, match="input sums"):
        tr.fused.step()
    torch.cuda.synchronize()
