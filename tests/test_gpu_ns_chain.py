"""GPU checks of the sampler chain's rank ride (ABI 50): a strided hop 0's counts + ranks run in
leading workgroups of the outer hop's sums launch (regnn_ns_csc_job),
its placement after that launch (regnn_ns_hop strided = 5) or in the head launch (CSC_DEFER):

* twin fused trainers that differ only in the knob (REGNN_NS_CSC_RIDE): sizes, losses, gradients,
  the index, the sums launch's outputs, and the parameters after captured steps -- bitwise;
* a hub graph on a standalone sampler whose outer hop is the sums launch in its table-reading
  form (ungrouped node types): the index against oracle/sampler_oracle.py over strided, strided,
  CSR, strided batches, then nearly empty blocks after a full one (stale ranks and counters);
* the 64-lane instantiations (a hop-1 and a hop-0 fan-out of 40).
"""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_ns_csc_split as S
from test_gpu_ns_engine import _mag, _setup_trainer

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _twins(monkeypatch, sizes=(9, 7), defer="off"):
    from regnn_hip import ns
    monkeypatch.setitem(ns.CSC_DEFER, "mode", defer)
    d = _mag(0.003, seed=10, F=128, hidden=64, classes=19, dropout=0.5)
    trs, models = [], []
    for mode in ("on", "off"):
        monkeypatch.setitem(ns.CSC_RIDE, "mode", mode)
        m = d["model"](6)
        m.train()
        tr, _ = _setup_trainer(d, m, batch=120, sizes=sizes)
        assert tr.fused is not None and tr.fused.two_layer and tr.sampler.strided
        assert all(s.csc_ride == (mode == "on") for s in tr.slots)
        assert bool(tr.fused.W.csc_pending) == (defer == "on")
        trs.append(tr)
        models.append(m)
    return trs, models


def _same_batch(a, b, models):
    """everything the sampler and the step wrote for the latest batch of trainers a (ride) and b"""
    from regnn_hip import ns
    sa, sb = a.sampler, b.sampler
    assert (0, True) in sa._csc_jobs and not sb._csc_jobs      # a's ranks rode the sums launch
    assert sa.csc_deferred[0] == sb.csc_deferred[0] == bool(a.fused.W.csc_pending)
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
    assert np.array_equal(la[:1 + la[0]], lb[:1 + lb[0]])            # hub list
    assert la[npiece_at] == lb[npiece_at] and np.array_equal(        # piece table
        la[tab_at:tab_at + 4 * la[npiece_at]], lb[tab_at:tab_at + 4 * lb[npiece_at]])
    cp = ca[1][:n0 + 1].cpu().numpy()
    ea, eb = ca[2][:E0].cpu().numpy(), cb[2][:E0].cpu().numpy()
    for u in range(n0):
        assert np.array_equal(np.sort(ea[cp[u]:cp[u + 1]]), np.sort(eb[cp[u]:cp[u + 1]])), u
    ta, tb = sa.typed_sums[1], sb.typed_sums[1]
    n1 = int(sa.sizes[1])
    for key in ("s_agg", "s_w", "u_self", "u_rel"):                  # the sums launch's rows
        assert torch.equal(ta[key][:n1], tb[key][:n1]), key
    assert torch.equal(sa.n_id[:int(sa.sizes[2])], sb.n_id[:int(sb.sizes[2])])
    assert torch.equal(sa.hop_bufs[0]["scnt"], sb.hop_bufs[0]["scnt"])
    assert torch.equal(sa.blocks[0].csr_idx, sb.blocks[0].csr_idx)   # local source ids
    assert torch.equal(sa.blocks[0].inv, sb.blocks[0].inv)


@pytest.mark.parametrize("defer", ["off", "on"])
def test_rank_ride_twin_trainers(monkeypatch, defer):
    """the knob changes which launch writes counts and ranks and where the placement runs, and
    nothing else: three eager steps and five captured ones, bitwise (entries per source sorted:
    their order inside a segment is the atomics', as before)"""
    (a, b), models = _twins(monkeypatch, defer=defer)
    for _ in range(3):
        a._forward_backward()
        b._forward_backward()
        torch.cuda.synchronize()
        _same_batch(a, b, models)
    for tr in (a, b):
        tr.capture(warmup=1)
        tr.run_steps(5)
    torch.cuda.synchronize()
    assert torch.equal(a.param_vector(), b.param_vector())


@pytest.mark.parametrize("sizes", [(9, 40), (40, 7)])
def test_rank_ride_wide_fanouts(monkeypatch, sizes):
    """a hop-1 fan-out of 40: the sums launch's 64-lane instantiation carries the rank job; a
    hop-0 fan-out of 40: 120 x 41 = 4,920 slots = 20 job workgroups, the last partial"""
    (a, b), models = _twins(monkeypatch, sizes=sizes)
    for _ in range(2):
        a._forward_backward()
        b._forward_backward()
        torch.cuda.synchronize()
        _same_batch(a, b, models)


def _hub_with_sums(seed, k1):
    """test_gpu_ns_csc_split's hub graph on a sampler whose outer hop (fan-out k1) is the sums
    launch: node types are not grouped by id, so it reads its lookup tables (no layout)"""
    from regnn_hip.ns import DeviceSampler
    g = S._hub_graph(seed)
    nt, N = g["nt"], g["N"]
    ds = DeviceSampler(g["rg"], [S.K0, k1], S.CAP, etype=torch.from_numpy(g["et"]),
                       ntype=torch.from_numpy(nt), num_edge_types=7)
    ds.enable_csc(0)
    local = np.zeros(N, dtype=np.int64)
    for t in range(4):
        local[nt == t] = np.arange(np.count_nonzero(nt == t))
    ds.enable_edge_meta(torch.from_numpy(local), 1)
    ds.meta_only[1] = True
    gen = torch.Generator().manual_seed(seed)
    tabs = [torch.randn(max(1, int(np.count_nonzero(nt == t))), 128, generator=gen).to(DEV)
            for t in range(4)]
    cap, T, K = ds.caps[1], 4, 128
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=DEV)  # noqa: E731
    ds.typed_sums[1] = dict(
        tables=(ctypes.c_void_p * T)(*[t.data_ptr() for t in tabs]), T=T, K=K, keep=tabs,
        s_agg=z(cap, T, K), s_w=z(cap, T), u_self=z(cap, K),
        u_rel=torch.full((cap, T + 1), -1, dtype=torch.int32, device=DEV), layout=None)
    g["ds"] = ds
    return g


def _hub_batch(g, it, n_targets, strided):
    ds = g["ds"]
    cnt = S._batch(g, it, n_targets, strided)
    assert not ds.csc_deferred[0]
    assert ds.sums_fresh[1] == bool(strided)
    if strided:                                # hop 1's sampled counts: every live row has one
        n1 = int(ds.sizes[1])
        assert int(ds.sizes[2]) == n1 and torch.all(ds.blocks[1].inv[:n1] > 0)
    return cnt


@pytest.mark.parametrize("k1", [5, 40])
def test_rank_ride_hub_graph(k1):
    """one source of ~2,500 entries in three pieces, ranks written by the sums launch's job
    workgroups (16 of them for 3,900 slots, the last partial): strided batches on one sampler
    with a CSR-layout batch between, then 37 targets and one target, whose counters and ranks
    from the full batch before are stale"""
    g = _hub_with_sums(21, k1)
    assert g["ds"].csc_ride
    for it, strided in enumerate([True, True, False, True], start=1):
        cnt = _hub_batch(g, it, S.CAP, strided)
        if it == 1:
            assert (0, True) in g["ds"]._csc_jobs
            assert cnt.max() > S.PIECE and cnt.sum() == S.CAP * (S.K0 + 1) > 3 * 1024
    _hub_batch(g, 5, 37, True)
    _hub_batch(g, 6, S.CAP, True)
    _hub_batch(g, 7, 1, True)


def test_default_defers_placement_where_ranks_ride(monkeypatch):
    """CSC_DEFER "auto": the head launch finishes the index exactly where hop 0's ranks ride the
    sums launch; with the ride off both halves stay on the sampler's queue, as before"""
    from regnn_hip import ns
    monkeypatch.setitem(ns.CSC_DEFER, "mode", "auto")
    d = _mag(0.003, seed=10, F=128, hidden=64, classes=19, dropout=0.5)
    for ride in ("on", "off"):
        monkeypatch.setitem(ns.CSC_RIDE, "mode", ride)
        m = d["model"](6)
        m.train()
        tr, _ = _setup_trainer(d, m, batch=120, sizes=(9, 7))
        assert tr.fused is not None and tr.fused.two_layer and tr.sampler.strided
        for fs in tr.fused_slots:
            assert bool(fs.W.csc_pending) == fs.sampler.csc_defer[0] == (ride == "on")
        tr._forward_backward()
        torch.cuda.synchronize()
        s = tr.sampler
        assert s.csc_deferred[0] == (ride == "on")
        assert ((0, True) in s._csc_jobs) == (ride == "on")
        assert np.isfinite(float(tr.loss))
