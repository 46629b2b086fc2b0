"""Golden vectors of self_loop_type 1 and 3: the REFERENCE's own REGNN class (mag/regnn_ns.py:216-346)
and conv classes (mag/regnn_layers.py) where the conv appends no self loop
(mag/regnn_layers.py:54-57, 86-99: relation_weight has num_edge_types entries), run in float64.

    python tests/golden/make_golden_selfloop.py
        (writes tests/golden/nssl_regnn_*.npz and tests/golden/mag_noloop_*conv_sl3.npz)

Like make_golden_bn.py this imports the reference at generation time only and no test runs it; the
helpers come from make_golden.py and the graph from make_golden_residual._schema_graph, both of
which stay as they are. No file name starts with a prefix an existing test globs (mag_regnn_,
mag_regcnconv_, mag_regatconv_, mag_regatv2conv_, nsres_, nsbn_). Running it again rewrites the
same bytes.

nssl_regnn_{regcn,regat,regatv2}_sl{1,3}: the ogbn-mag-schema graph of make_golden_residual (354
nodes, graph seed 5), K = 64, hidden width 64 (regcn: 64 channels; the attention models: 2 heads
x 32), residual, use_norm 'ln', dropout 0, 7 classes, fan-out [5, 3], a batch of 32 papers drawn
by oracle.sampler_oracle, eval mode (dropout 0, LayerNorm: the same function as training mode),
the loss and every gradient as make_golden_residual._store stores them.
  * self_loop_type 1: the four self-loop relations are edges of the graph (mag/regnn_ns.py:107-119:
    author, field_of_study, institution, paper -> relations 7..10, num_edge_types 11), appended
    after the 7-relation graph's edges and the whole re-sorted dst-major (stable), so edge ids are
    CSR positions again. base_src / base_dst / base_edge_type hold the 7-relation graph.
  * self_loop_type 3: no self loops. Asserted before saving: every block has a live target without
    a sampled in-edge (paper ISO of the schema graph has no edge at all); `empty0` / `empty1` hold
    those targets' rows, outermost block first.

mag_noloop_{regcn,regat,regatv2}conv_sl3: one conv call each on gen_mag / gen_mag_gat's random
bipartite block recipe with self_loop_type 3 (residual, 'ln'), a few targets without in-edges.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
import make_golden_residual as MR  # noqa: E402

COUNTS = [170, 40, 14, 130]                        # author, field_of_study, institution, paper
SIZES, K, CLASSES, GRAPH_SEED = [5, 3], 64, 7, 5
MODELS = {"regcn": (64, 1), "regat": (32, 2), "regatv2": (32, 2)}    # (hidden channels, heads)


def _with_loops(src, dst, et, N, ntype, n_et):
    """self_loop_type 1's graph: one (v, v) edge per node, relation n_et + node type (the schema
    graph numbers its node types in the reference's edge_index_dict order), dst-major again"""
    loop = np.arange(N, dtype=np.int64)
    s = np.concatenate([src, loop])
    d = np.concatenate([dst, loop])
    t = np.concatenate([et, n_et + ntype.astype(np.int64)])
    o = np.argsort(d, kind="stable")
    return s[o], d[o], t[o]


def gen_regnn(kind, slt, model_seed):
    regnn_layers, SO = MR._setup()
    rng = np.random.default_rng(GRAPH_SEED)
    src, dst, edge_type, ntype, local, p0, batch = MR._schema_graph(rng, COUNTS)
    N = int(sum(COUNTS))
    n_et = 7
    st = {}
    if slt == 1:
        st.update(base_src=src, base_dst=dst, base_edge_type=edge_type)
        src, dst, edge_type = _with_loops(src, dst, edge_type, N, ntype, n_et)
        n_et += 4
    ptr = MR._csr_ptr(dst, N)
    batch = (p0 + batch).astype(np.int64)
    seed, epoch, batch_idx = 91, 0, 3
    _, n_id, adjs = SO.neighbor_sample(ptr, src, batch.tolist(), SIZES, seed, epoch, batch_idx)
    live = [int(sz[1]) for _s, _d, _e, sz in adjs]            # outermost hop first
    assert live[-1] == batch.size
    if slt == 3:
        for h, (_s, d_, _e, sz) in enumerate(adjs):
            cnt = np.bincount(np.asarray(d_, np.int64), minlength=int(sz[1]))
            empty = np.nonzero(cnt == 0)[0]
            assert empty.size >= 1, f"block {h}: every live target has a sampled in-edge"
            st[f"empty{h}"] = empty.astype(np.int64)
    y = np.full(N, -1, np.int64)
    y[p0:] = rng.integers(0, CLASSES, COUNTS[3])
    hidden, heads = MODELS[kind]
    args = SimpleNamespace(model=kind, feats_type=3, self_loop_type=slt, no_re=False)
    REGNN = MG._reference_regnn_class(args, {t: COUNTS[t] for t in range(4)}, 3, regnn_layers)
    torch.manual_seed(model_seed)
    model = REGNN(K, hidden, CLASSES, heads, 2, 10.0, 0.0, {t: K for t in range(4)}, n_et, True,
                  False, use_norm="ln")
    MG._set_params(model, rng, ew_alpha=10.0)
    model.eval()
    assert all(int(c.relation_weight.shape[0]) == n_et for c in model.convs)
    x_dict = {t: torch.from_numpy((MG.f32(rng, COUNTS[t], K) if t == 3 else
                                   rng.uniform(-0.5, 0.5, (COUNTS[t], K)).astype(np.float32))
                                  .astype(np.float64)) for t in range(4)}
    out, loss = MR._run(model, x_dict, n_id, adjs, edge_type, ntype, local, y[batch])
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(g).all())
                                              for g in MG._grads(model).values())
    st.update(src=src, dst=dst, edge_type=edge_type, ntype=ntype, local=local, y=y, batch=batch,
              n_id=np.asarray(n_id, np.int64), logp=out, loss=loss.detach())
    MR._store(st, x_dict, adjs, model)
    MG.save(f"nssl_regnn_{kind}_sl{slt}",
            dict(model="mag.REGNN", kind=kind, feats_type=3, in_channels=K, hidden=hidden,
                 heads=heads, hidden_dim=hidden * heads, classes=CLASSES, num_layers=2,
                 scaling_factor=10.0, num_edge_types=n_et, counts=COUNTS, target_type=3,
                 target_offset=p0, y_global=True, sizes=SIZES, seed=seed, epoch=epoch,
                 batch_idx=batch_idx, use_norm="ln", self_loop_type=slt, dropout=0.0,
                 schema="ogbn-mag", residual=True, live=live, graph_seed=GRAPH_SEED), st)


def gen_convs():
    """gen_mag / gen_mag_gat's block recipe with self_loop_type 3: nothing appended, targets 3, 17
    and 42 without any in-edge (they come out bias + residual / the zero attention term)."""
    regnn_layers, _SO = MR._setup()
    rng = np.random.default_rng(60)
    n_src, n_dst, E = 240, 80, 900
    num_node_types, num_edge_types = 4, 7
    src = rng.integers(0, n_src, size=E).astype(np.int64)
    dst = rng.integers(0, n_dst, size=E).astype(np.int64)
    dst[np.isin(dst, [3, 17, 42])] = 5
    edge_type = rng.integers(0, num_edge_types, size=E).astype(np.int64)
    tnt = rng.integers(0, num_node_types, size=n_dst).astype(np.int64)
    empty = np.nonzero(np.bincount(dst, minlength=n_dst) == 0)[0]
    assert set(empty.tolist()) >= {3, 17, 42}
    for tag, cls, H, C in (("regcn", "REGCNConv", 1, 64), ("regat", "REGATConv", 2, 32),
                           ("regatv2", "REGATv2Conv", 2, 32)):
        torch.manual_seed(10)
        if tag == "regcn":
            conv = regnn_layers.REGCNConv(64, 64, num_node_types, num_edge_types, 10.0,
                                          residual=True, use_norm="ln", self_loop_type=3)
        else:
            conv = getattr(regnn_layers, cls)(H * C, C, num_node_types, num_edge_types, heads=H,
                                              scaling_factor=10.0, residual=True, use_norm="ln",
                                              self_loop_type=3)
        MG._set_params(conv, rng, ew_alpha=10.0)
        assert int(conv.relation_weight.shape[0]) == num_edge_types
        x = torch.from_numpy(MG.f32(rng, n_src, H * C).astype(np.float64)).requires_grad_(True)
        ei = torch.from_numpy(np.stack([src, dst]))
        out = conv((x, x[:n_dst]), ei, torch.from_numpy(edge_type), torch.from_numpy(tnt))
        gout = MG.f32(rng, *out.shape)
        out.backward(torch.from_numpy(gout.astype(np.float64)))
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(x.grad).all())
        st = dict(src=src, dst=dst, edge_type=edge_type, target_node_type=tnt, empty=empty,
                  x=x.detach().numpy().astype(np.float32), gout=gout, out=out, grad_x=x.grad)
        MG._pack("p_", MG._params(conv), st)
        MG._pack("grad_", MG._grads(conv), st)
        MG.save(f"mag_noloop_{tag}conv_sl3",
                dict(layer=f"mag.{cls}", n_src=n_src, n_dst=n_dst, num_node_types=num_node_types,
                     num_edge_types=num_edge_types, heads=H, out_channels=C, scaling_factor=10.0,
                     residual=True, use_norm="ln", self_loop_type=3, negative_slope=0.2), st)


if __name__ == "__main__":
    torch.set_default_dtype(torch.float64)
    which = sys.argv[1:] or ["regnn", "convs"]
    if "regnn" in which:
        for i, kind in enumerate(MODELS):
            for slt in (1, 3):
                gen_regnn(kind, slt, 30 + 2 * i + (slt == 3))
    if "convs" in which:
        gen_convs()
