"""GPU checks of the strided transposed index's split build (regnn_ns_hop csc_rank, ABI 48: counts
+ ranks in one launch, every workgroup's own scan and placement in a second) and of its second
half deferred into the two-layer step's head launch (regnn_nsm_work csc_pending):

* a hub graph on a standalone sampler: segments, csc_ptr, the hub list and the piece table
  against oracle/sampler_oracle.py, over several batches of one sampler with a CSR batch between;
* nearly empty blocks (37 targets and one target on a 300-target sampler);
* two fused trainers that differ only in the deferral: losses, gradients, indices, parameters;
* the guard between the step's csc_pending and what the sampler's latest batch did.
"""
import numpy as np
import pytest
import torch

from oracle import sampler_oracle as SO
from test_gpu_ns_engine import _mag, _oracle_csr, _setup_trainer

pytestmark = pytest.mark.gpu
DEV = "cuda"
K0, CAP = 12, 300
PIECE = 1024


def _hub_graph(seed):
    from regnn_hip.graph import RelGraph
    from regnn_hip.ns import DeviceSampler
    rng = np.random.default_rng(seed)
    N, E = 2000, 80000
    dst = rng.integers(0, N, E)
    r = rng.random(E)
    src = np.where(r < 0.70, 0,
                   np.where(r < 0.85, rng.integers(1, 4, E), rng.integers(0, N, E)))
    et, nt = rng.integers(0, 7, E), rng.integers(0, 4, N)
    rg = RelGraph(src, dst, N, DEV)
    ds = DeviceSampler(rg, [K0, 5], CAP, etype=torch.from_numpy(et), ntype=torch.from_numpy(nt),
                       num_edge_types=7)
    ds.enable_csc(0)
    return dict(rng=rng, N=N, rg=rg, ds=ds, et=et, nt=nt, csr=_oracle_csr(rg))


def _want_index(g, targets, batch_idx):
    """hop 0's block transposed on the CPU (oracle/sampler_oracle.py): per local source the
    sorted entries (target row << 8 | relation), self loops included."""
    ptr, idx, eid = g["csr"]
    n_id, s, d, e = SO.sample_hop(ptr, idx, [int(t) for t in targets], K0,
                                  SO.hop_seed(5, 0, batch_idx, 0))
    want = [[] for _ in n_id]
    for u, v, p in zip(s, d, e):
        want[u].append((v << 8) | int(g["et"][eid[p]]))
    for v, t in enumerate(targets):
        want[v].append((v << 8) | (7 + int(g["nt"][int(t)])))
    return [sorted(w) for w in want]


def _compare_index(ds, want):
    from regnn_hip import ns
    _, cptr, cent, clong = ds.csc[0]
    sz = ds.sizes.cpu().tolist()
    n_src, slots = sz[1], sz[8]
    cnt = np.array([len(w) for w in want])
    assert n_src == len(want) and slots == cnt.sum()
    cp = cptr[:n_src + 1].cpu().numpy()
    assert np.array_equal(cp, np.concatenate([[0], np.cumsum(cnt)])) and cp[-1] == sz[8]
    ce = cent[:slots].cpu().numpy().astype(np.int64)
    for u in range(n_src):
        assert sorted(ce[cp[u]:cp[u + 1]].tolist()) == want[u], u
    cl = clong.cpu().numpy()
    hubs = np.nonzero(cnt > 16)[0]
    assert cl[0] == hubs.size and np.array_equal(cl[1:1 + hubs.size], hubs)
    npiece_at = ns._LONG_CAP + 1
    tab_at = (npiece_at + 1 + 3) // 4 * 4
    npc = -(-cnt[hubs] // PIECE)
    assert cl[npiece_at] == npc.sum()
    tab = cl[tab_at:tab_at + 4 * int(npc.sum())].reshape(-1, 4)
    at = 0
    for li, (u, m) in enumerate(zip(hubs.tolist(), npc.tolist())):
        for k in range(m):                 # a row's pieces: consecutive, in order, tiling it
            row, first, ents, word = tab[at + k].tolist()
            assert row == u and first == cp[u] + k * PIECE
            assert ents == min(PIECE, cnt[u] - k * PIECE) and 0 < ents <= PIECE
            assert word == (li << 16) | (k << 8) | m
        assert cp[u] + sum(tab[at:at + m, 2]) == cp[u + 1]
        at += m
    return cnt


def _batch(g, it, n_targets, strided):
    ds = g["ds"]
    targets = g["rng"].permutation(g["N"])[:n_targets]
    ds.set_seed(5, 0, it)
    ds.set_targets(torch.from_numpy(targets).to(DEV))
    ds.run_hops(strided=strided)
    return _compare_index(ds, _want_index(g, targets, it))


@pytest.mark.parametrize("seed", [21, 22, 23])
def test_split_index_hub_graph(seed):
    """placement 1 (both launches in regnn_ns_hop): one source of ~2,500 entries (three pieces),
    a few between 17 and 1,024, ~700 short ones; 3,900 slots = four placing workgroups, the last
    partial. Strided batches one after another on one sampler (the counters and ranks are
    reused), a CSR-layout batch between them."""
    g = _hub_graph(seed)
    for it, strided in enumerate([True, True, False, True], start=1):
        cnt = _batch(g, it, CAP, strided)
        assert not g["ds"].csc_deferred[0]
        if it == 1:                        # the shape this test is about
            assert cnt.max() > PIECE
            assert np.count_nonzero((cnt > 16) & (cnt <= PIECE)) >= 2
            assert cnt.sum() == CAP * (K0 + 1) > 3 * 1024


@pytest.mark.parametrize("n_targets", [37, 1])
def test_split_index_sparse_block(n_targets):
    """most slots empty: placing workgroups with no live slot, and a single target"""
    g = _hub_graph(21)
    _batch(g, 1, CAP, True)
    _batch(g, 2, n_targets, True)


def _fused_pair(monkeypatch):
    from regnn_hip import ns
    d = _mag(0.003, seed=10, F=128, hidden=64, classes=19, dropout=0.5)
    trs, models = [], []
    for mode in ("on", "off"):
        monkeypatch.setitem(ns.CSC_DEFER, "mode", mode)
        m = d["model"](6)
        m.train()
        tr, _ = _setup_trainer(d, m, batch=120, sizes=(9, 7))
        assert tr.fused is not None and tr.fused.two_layer and tr.sampler.strided
        assert bool(tr.fused.W.csc_pending) == (mode == "on")
        trs.append(tr)
        models.append(m)
    return trs, models


def test_deferred_index_matches_sampler_queue(monkeypatch):
    """the index finished by the head launch's extra workgroups against both launches on the
    sampler's queue: bitwise the same loss, gradients and (sorted per source) index over eager
    steps, and the same parameters after captured steps"""
    from regnn_hip import ns
    (a, b), models = _fused_pair(monkeypatch)
    for _ in range(3):
        a._forward_backward()
        b._forward_backward()
        torch.cuda.synchronize()
        sa, sb = a.sampler, b.sampler
        assert sa.csc_deferred[0] and not sb.csc_deferred[0]
        assert torch.equal(sa.sizes, sb.sizes)
        assert float(a.loss) == float(b.loss)
        for pa, pb in zip(models[0].parameters(), models[1].parameters()):
            assert torch.equal(pa.grad, pb.grad)
        n0, E0 = int(sa.sizes[1]), int(sa.sizes[8])
        ca, cb = sa.csc[0], sb.csc[0]
        assert E0 > 0 and torch.equal(ca[1][:n0 + 1], cb[1][:n0 + 1])
        la, lb = ca[3].cpu().numpy(), cb[3].cpu().numpy()
        npiece_at = ns._LONG_CAP + 1
        tab_at = (npiece_at + 1 + 3) // 4 * 4
        assert np.array_equal(la[:1 + la[0]], lb[:1 + lb[0]])        # hub list
        assert la[npiece_at] == lb[npiece_at] and np.array_equal(
            la[tab_at:tab_at + 4 * la[npiece_at]], lb[tab_at:tab_at + 4 * lb[npiece_at]])
        cp = ca[1][:n0 + 1].cpu().numpy()
        ea, eb = ca[2][:E0].cpu().numpy(), cb[2][:E0].cpu().numpy()
        for u in range(n0):
            assert np.array_equal(np.sort(ea[cp[u]:cp[u + 1]]), np.sort(eb[cp[u]:cp[u + 1]])), u
    for tr in (a, b):
        tr.capture(warmup=1)
        tr.run_steps(4)
    torch.cuda.synchronize()
    assert torch.equal(a.param_vector(), b.param_vector())


def test_deferral_refused_when_index_row_is_wider_than_head(monkeypatch):
    """a hop-0 fan-out of 64: 128 targets x 65 slots need 9 placing workgroups, the head has 8.
    The index's grid row may not widen the head's (extra head workgroups would write past the
    slab), so the trainer keeps both launches on the sampler's queue; at fan-out 63 the two
    counts are equal and the deferral applies."""
    from regnn_hip import ns
    monkeypatch.setitem(ns.CSC_DEFER, "mode", "on")
    d = _mag(0.003, seed=10, F=128, hidden=64, classes=19, dropout=0.5)
    for k0, want in ((64, False), (63, True)):
        m = d["model"](6)
        m.train()
        tr, _ = _setup_trainer(d, m, batch=128, sizes=(k0, 7))
        assert tr.fused is not None and tr.fused.two_layer and tr.sampler.strided
        ce = tr.sampler.blocks[0].csr_idx.numel()
        assert (-(-ce // 1024) > -(-128 // 16)) == (not want)
        for fs in tr.fused_slots:
            assert bool(fs.W.csc_pending) == want and fs.sampler.csc_defer[0] == want
    # fan-out 63: the index's row as wide as the head's (8 and 8) against the sampler's queue
    monkeypatch.setitem(ns.CSC_DEFER, "mode", "off")
    m2 = d["model"](6)
    m2.train()
    ref, _ = _setup_trainer(d, m2, batch=128, sizes=(63, 7))
    assert not ref.fused.W.csc_pending
    for _ in range(2):
        tr._forward_backward()
        ref._forward_backward()
        torch.cuda.synchronize()
        assert float(tr.loss) == float(ref.loss)
        for pa, pb in zip(m.parameters(), m2.parameters()):
            assert torch.equal(pa.grad, pb.grad)
        n0 = int(tr.sampler.sizes[1])
        assert torch.equal(tr.sampler.csc[0][1][:n0 + 1], ref.sampler.csc[0][1][:n0 + 1])


def test_pending_bit_guard(monkeypatch):
    """FusedStep.step refuses a step whose csc_pending disagrees with what the sampler's latest
    batch on that slot did (as it does for stale input sums)"""
    (a, _), _ = _fused_pair(monkeypatch)
    a._prime()
    fs, s = a.fused_slots[a.cur], a.slots[a.cur]
    assert fs.W.csc_pending == 1 and s.csc_deferred[0]
    s.csc_defer[0] = False                 # told pending, the batch built its index in full
    a._sample(a.cur)
    assert not s.csc_deferred[0]
    with pytest.raises(RuntimeError, match="transposed index"):
        fs.step()
    s.csc_defer[0] = True                  # not told, the index is pending
    a._sample(a.cur)
    fs.W.csc_pending = 0
    with pytest.raises(RuntimeError, match="transposed index"):
        fs.step()
    fs.W.csc_pending = 1
    fs.step()
    torch.cuda.synchronize()
    assert np.isfinite(float(a.loss))
