"""The sampler's type layout (regnn_hip.ns.type_layout -> regnn_ns_type_layout): node ids grouped
by type, table row = id - the type's first id, one relation per (target type, source type) pair.
CPU checks of the setup function on plain tensors, of the C entry's argument validation, and of
the hand-built graph the GPU test (test_gpu_ns_type_layout.py) samples: the sampler oracle alone
must hit every degree class and draw every type boundary on it."""
import ctypes
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import sampler_oracle as SO  # noqa: E402

SEED = 11                                     # the GPU test's base seed (epoch 0, batch 0)


# ---- the hand-built typed graph ---------------------------------------------------------------
def hand_graph():
    """48 nodes, T = 4, ids grouped by type: type 0 = 0..19, type 1 = 20 (one node: its first id
    is its last), type 2 = 21..35, type 3 = 36..47. In-degrees cover 0, < k, = k, > k for k = 3
    and for k = 33 (node 36: exactly 33, node 0: 40). The rows whose whole neighbourhood is drawn
    at either fan-out (47, 21, 20: degree <= 3) hold every type's first and last node as sources.
    One relation per (target type, source type) pair, numbered in sorted pair order."""
    counts = [20, 1, 15, 12]
    off = np.concatenate([[0], np.cumsum(counts)])
    N = int(off[-1])
    ntype = np.repeat(np.arange(4), counts)
    ins = {i: set() for i in range(N)}
    ins[0] = set(range(1, 41))                # 40 in-edges, every source type
    ins[36] = set(range(0, 33))               # exactly 33
    ins[47] = {0, 19, 20}                     # = 3: type 0's first / last, type 1's only node
    ins[21] = {35, 36, 47}                    # = 3: type 2's last, type 3's first / last
    ins[20] = {21, 5}                         # 2: type 2's first
    ins[35] = {1, 2, 3, 4, 22}                # 5 (> 3)
    ins[19] = set()                           # no in-edge: the self loop alone
    for i in range(1, 19):                    # type-0 rows, degrees 0..4
        ins[i] = {(i * 7 + j * 5) % N for j in range(i % 5)} - {i}
    src, dst = [], []
    for d in range(N):
        for s in sorted(ins[d]):
            src.append(s)
            dst.append(d)
    src, dst = np.array(src), np.array(dst)
    pairs = sorted({(int(ntype[d]), int(ntype[s])) for s, d in zip(src, dst)})
    rel_of = {p: r for r, p in enumerate(pairs)}
    etype = np.array([rel_of[(int(ntype[d]), int(ntype[s]))] for s, d in zip(src, dst)])
    local = np.arange(N) - off[ntype]
    return dict(src=src, dst=dst, etype=etype, ntype=ntype, local=local, N=N, off=off,
                counts=counts, R=len(pairs), pairs=rel_of)


def csr_by_target(g):
    """(ptr, idx, eid): the graph's CSR by target, edges of a row in input order."""
    order = np.argsort(g["dst"], kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(g["dst"], minlength=g["N"]))])
    return ptr, g["src"][order], order


def test_oracle_covers_the_hand_graph():
    g = hand_graph()
    ptr, idx, _ = csr_by_target(g)
    deg = np.diff(ptr)
    bounds = {int(g["off"][t]) for t in range(4)} | {int(g["off"][t + 1]) - 1 for t in range(4)}
    assert len(bounds) == 7                   # type 1: first == last
    for k in (3, 33):
        assert (deg == 0).any() and ((deg > 0) & (deg < k)).any()
        assert (deg == k).any() and (deg > k).any()
        seed = SO.hop_seed(SEED, 0, 0, 1)
        drawn = set()
        for t in range(g["N"]):               # every node is a target row of the outer hop
            srcs, pos = SO.sample_row(ptr, idx, t, k, seed)
            assert len(srcs) == min(int(deg[t]), k) and len(set(pos)) == len(pos)
            drawn.update(srcs)
        assert bounds <= drawn, bounds - drawn


# ---- the setup function -----------------------------------------------------------------------
def _mag_cpu(scale=0.003):
    from regnn_hip import synth
    gd = synth.mag_like(scale, seed=0, device="cpu")
    keep = gd["rel"] <= 7
    src, dst = gd["src"][keep].numpy(), gd["dst"][keep].numpy()
    g = dict(src=src, dst=dst, etype=gd["rel"][keep].numpy().astype(np.int64) - 1,
             ntype=gd["ntype"].numpy(), N=gd["N"])
    off = np.array([gd["type_offsets"][t] for t in synth.NTYPES] + [gd["N"]])
    g["local"] = np.arange(g["N"]) - off[g["ntype"]]
    return g, off, synth


def _layout(g, T=4):
    from regnn_hip import ns
    ptr, idx, eid = csr_by_target(g)
    return ns.type_layout(torch.from_numpy(g["ntype"]), torch.from_numpy(g["local"]),
                          torch.from_numpy(ptr), torch.from_numpy(idx),
                          torch.from_numpy(g["etype"][eid]).to(torch.uint8), T)


def test_layout_accepted_for_mag_like():
    g, off, synth = _mag_cpu()
    lay = _layout(g)
    assert lay is not None and lay["T"] == 4
    assert lay["type_off"] == off.tolist()
    tid = {t: k for k, t in enumerate(synth.NTYPES)}
    # synth.mag_like's relations (0-based): 0..3 the forward MAG_EDGES (paper-paper both ways as
    # one), 4..6 the reverses of affiliated_with, writes, has_topic
    want = [[-1] * 4 for _ in range(4)]
    for r, (st, dt, _c) in enumerate(synth.MAG_EDGES):
        want[tid[dt]][tid[st]] = r
    for j, i in enumerate((0, 1, 3)):
        st, dt, _c = synth.MAG_EDGES[i]
        want[tid[st]][tid[dt]] = 4 + j
    assert sum(v >= 0 for row in want for v in row) == 7
    assert lay["pair_rel"] == want


def test_layout_of_the_hand_graph():
    g = hand_graph()
    lay = _layout(g)
    assert lay["type_off"] == g["off"].tolist()
    for (dt, st), r in g["pairs"].items():
        assert lay["pair_rel"][dt][st] == r
    assert sum(v >= 0 for row in lay["pair_rel"] for v in row) == g["R"]


def test_layout_refused():
    g = hand_graph()
    # interleaved types: the ids permuted, every per-node array following its node
    perm = np.random.default_rng(0).permutation(g["N"])
    p = dict(g, src=perm[g["src"]], dst=perm[g["dst"]])
    p["ntype"], p["local"] = np.empty_like(g["ntype"]), np.empty_like(g["local"])
    p["ntype"][perm], p["local"][perm] = g["ntype"], g["local"]
    assert _layout(p) is None
    # a wrong table row: the rows of one type reversed
    w = dict(g, local=g["local"].copy())
    f = g["ntype"] == 2
    w["local"][f] = w["local"][f][::-1]
    assert _layout(w) is None
    # five types
    five = dict(g, ntype=g["ntype"].copy())
    five["ntype"][-1] = 4
    assert _layout(five, T=5) is None
    # two relations on one (target type, source type) pair
    two = dict(g, etype=g["etype"].copy())
    e = int(np.nonzero(g["dst"] == 0)[0][0])
    two["etype"][e] = (two["etype"][e] + 1) % g["R"]
    assert _layout(two) is None


def test_layout_accepts_a_type_without_nodes():
    """pinned: a type with zero nodes is accepted (equal offsets: no id falls between them, so
    the kernel's compares skip the type)."""
    g = hand_graph()
    nt = g["ntype"].copy()
    nt[nt == 1] = 2                            # type 1 loses its only node to type 2
    off = np.array([0, 20, 20, 36, 48])
    e = dict(g, ntype=nt, local=np.arange(g["N"]) - off[nt])
    pairs = sorted({(int(nt[d]), int(nt[s])) for s, d in zip(g["src"], g["dst"])})
    e["etype"] = np.array([pairs.index((int(nt[d]), int(nt[s])))
                           for s, d in zip(g["src"], g["dst"])])
    lay = _layout(e)
    assert lay is not None and lay["type_off"] == off.tolist()
    assert all(v == -1 for v in lay["pair_rel"][1]) and all(r[1] == -1 for r in lay["pair_rel"])


# ---- the C entry's validation (no GPU: before any launch) ---------------------------------------
def _sums_call(lay, n_et=7, T=4, meta=(1 << 24, 1 << 25, 1 << 26)):
    from regnn_hip import _lib, ns
    tabs = (ctypes.c_void_p * 4)(*[(1 << 30) + 4096 * t for t in range(4)])
    s = ns.layout_struct(lay)
    f = 1 << 20                                # never dereferenced: validation comes first
    return _lib._so.regnn_ns_hop_typed_sums(
        f, f, None, None, n_et, 3, 1, f, f, f, 64, f, meta[0], f, None, meta[1], meta[2], tabs, T,
        128, 1 << 27, f, 1 << 28, f, None, ctypes.addressof(s), None)


def test_c_entry_rejects_bad_layouts_without_gpu():
    good = dict(T=4, type_off=[0, 20, 21, 36, 48],
                pair_rel=[[0, 1, 2, 3], [4, -1, 5, -1], [6, -1, -1, -1], [-1] * 4])
    assert _sums_call(dict(good, type_off=[0, 20, 19, 36, 48])) == 1     # decreasing offsets
    assert _sums_call(dict(good, type_off=[1, 20, 21, 36, 48])) == 1     # not from 0
    bad = [row[:] for row in good["pair_rel"]]
    bad[1][2] = 7
    assert _sums_call(dict(good, pair_rel=bad)) == 1                     # relation >= n_et
    bad[1][2] = -2
    assert _sums_call(dict(good, pair_rel=bad)) == 1                     # relation < -1
    assert _sums_call(dict(good, T=3), T=4) == 1                         # another type count
    assert _sums_call(good, meta=(1 << 24, None, 1 << 26)) == 1          # meta: all or none
    # without a layout the lookup tables are required
    from regnn_hip import _lib
    f = 1 << 20
    tabs = (ctypes.c_void_p * 4)(*[(1 << 30) + 4096 * t for t in range(4)])
    assert _lib._so.regnn_ns_hop_typed_sums(
        f, f, None, None, 7, 3, 1, f, f, f, 64, f, f, f, None, f, f, tabs, 4, 128, 1 << 27, f,
        1 << 28, f, None, None, None) == 1
