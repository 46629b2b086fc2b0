"""Golden vectors of the fused NS step's residual mode: the REFERENCE's own REGNN class
(mag/regnn_ns.py:216-346) with residual=True, use_norm 'ln', self_loop_type 2, dropout 0, run in
float64 on a sampled batch, as make_golden.gen_regnn / gen_regnn_schema / gen_regnn_ft5 do.

    python tests/golden/make_golden_residual.py     (writes tests/golden/nsres_regnn_*.npz)

Like make_golden.py this imports the reference at generation time only and no test runs it; its
helpers come from make_golden.py, which stays as it is. The file names do not start with
mag_regnn_, so no existing test's fixture glob picks them up. Running it again rewrites the same
bytes.

* nsres_regnn_schema: an ogbn-mag-schema graph (one relation per type pair: the fused step's
  relation slots apply), K = 128, hidden 64, 349 classes, fan-out [25, 20], built here so that the
  innermost block (the batch's; `adj1_*`, the fused step's hop 0) holds
    (a) a batch target that is the source of more than 16 entries, self loop included (a hub row
        of the transposed index: the residual term meets the piece path there),
    (b) a batch target whose only transposed entry is its own self loop,
    (c) batch targets with exactly 1 in-entry (the self loop) and with 26 (full fan-out + self),
    (d) at least three node types among the layer-0 targets (the block's sources);
  asserted from the oracle sampler's adjs before saving.
* nsres_regnn_ft3: gen_regnn's random-relation graph (no relation slots: the edge pass), K = 64,
  5 classes, fan-out [4, 3].
"""
import importlib
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

_PURGE = ["dgl", "layer", "model", "utils", "regnn_layers", "torch_geometric", "torch_scatter",
          "torch_sparse", "ogb", "texttable"]


def _setup():
    MG._purge(_PURGE)
    MG._use_paths([MG.SHIM, os.path.join(MG.REF, "mag")])
    regnn_layers = importlib.import_module("regnn_layers")
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle import sampler_oracle as SO
    return regnn_layers, SO


def _csr_ptr(dst, N):
    ptr = np.zeros(N + 1, np.int64)
    np.add.at(ptr, dst + 1, 1)
    return np.cumsum(ptr)


def _run(model, x_dict, n_id, adjs, edge_type, ntype, local, yb):
    t_adjs = [(torch.tensor([s_, d_], dtype=torch.int64), torch.tensor(e_, dtype=torch.int64), sz)
              for s_, d_, e_, sz in adjs]
    out = model(torch.tensor(n_id), x_dict, t_adjs, torch.from_numpy(edge_type),
                torch.from_numpy(ntype), torch.from_numpy(local))
    loss = torch.nn.functional.nll_loss(out, torch.from_numpy(yb))
    loss.backward()
    return out, loss


def _store(st, x_dict, adjs, model):
    for t, x in x_dict.items():
        st[f"x{t}"] = x.numpy().astype(np.float32)
    for h, (s_, d_, e_, sz) in enumerate(adjs):
        st[f"adj{h}_src"], st[f"adj{h}_dst"] = np.asarray(s_), np.asarray(d_)
        st[f"adj{h}_eid"] = np.asarray(e_)
        st[f"adj{h}_size"] = np.asarray(sz)
    MG._pack("p_", MG._params(model), st)
    MG._pack("grad_", MG._grads(model), st)


# the batch's papers (local ids): 0..2 the graph's hub papers (rows past the fan-out), HUB the
# paper the other batch papers cite (a hub row of the transposed index), ISO a paper without any
# edge (1 in-entry; its only transposed entry its own self loop)
HUB, ISO, N_CITERS, BATCH = 5, 6, 18, 32


def _schema_graph(rng, counts):
    """ogbn-mag's schema as make_golden._mag_schema_graph builds it (the 4 raw relations in the
    dataset's order, the 3 reverse relations appended, cites undirected and coalesced, global ids
    type by type, edge ids = positions of the dst-major CSR), plus the cases of this fixture: no
    edge touches paper ISO, and N_CITERS of the batch's papers cite paper HUB. Returns the graph
    and the batch (local paper ids)."""
    A, Fd, I, P = 0, 1, 2, 3
    off = np.concatenate([[0], np.cumsum(counts)[:-1]])

    def rnd(st, dt, n, hub_dst=None, hub_frac=0.0):
        s = rng.integers(0, counts[st], n)
        d = rng.integers(0, counts[dt], n)
        if hub_dst is not None:                       # a few hub targets: rows past the fan-out
            m = rng.random(n) < hub_frac
            d[m] = rng.integers(0, hub_dst, int(m.sum()))
        return np.stack([s, d])

    aff = rnd(A, I, 260)
    writes = rnd(A, P, 700, hub_dst=3, hub_frac=0.12)
    cites = rnd(P, P, 500, hub_dst=2, hub_frac=0.1)
    topic = rnd(P, Fd, 420, hub_dst=2, hub_frac=0.15)
    writes = writes[:, writes[1] != ISO]
    cites = cites[:, (cites[0] != ISO) & (cites[1] != ISO) & (cites[0] != cites[1])]
    topic = topic[:, topic[0] != ISO]
    # the batch: the hub papers, HUB, ISO and papers whose in-degree (writes + undirected cites +
    # topics' reverse, one more for the cite added below) stays <= 25, so the fan-out of 25 keeps
    # every in-edge of theirs, the one from HUB included
    und = np.unique(np.concatenate([cites[0] * counts[P] + cites[1],
                                    cites[1] * counts[P] + cites[0]]))
    deg = (np.bincount(writes[1], minlength=counts[P]) +
           np.bincount(und % counts[P], minlength=counts[P]) +
           np.bincount(topic[0], minlength=counts[P]))
    fixed = [0, 1, 2, HUB, ISO]
    cand = [p for p in range(counts[P]) if p not in fixed and deg[p] + 1 <= 25]
    rest = rng.choice(np.asarray(cand), BATCH - len(fixed), replace=False).astype(np.int64)
    batch = np.concatenate([np.asarray(fixed, np.int64), rest])
    citers = rest[:N_CITERS]
    cites = np.concatenate([cites, np.stack([citers, np.full(N_CITERS, HUB)])], 1)

    rels = {}
    rels[("author", "affiliated_with", "institution")] = (A, I, aff)
    rels[("author", "writes", "paper")] = (A, P, writes)
    rels[("paper", "has_topic", "field_of_study")] = (P, Fd, topic)
    rels[("institution", "to", "author")] = (I, A, aff[::-1])
    rels[("paper", "to", "author")] = (P, A, writes[::-1])
    rels[("field_of_study", "to", "paper")] = (Fd, P, topic[::-1])
    ei = np.concatenate([cites, cites[::-1]], 1)
    ei = np.unique(ei[0] * counts[P] + ei[1])
    rels[("paper", "cites", "paper")] = (P, P, np.stack([ei // counts[P], ei % counts[P]]))
    order = [("author", "affiliated_with", "institution"), ("author", "writes", "paper"),
             ("paper", "cites", "paper"), ("paper", "has_topic", "field_of_study"),
             ("institution", "to", "author"), ("paper", "to", "author"),
             ("field_of_study", "to", "paper")]
    src, dst, et = [], [], []
    for i, key in enumerate(order):
        st, dt, e = rels[key]
        src.append(e[0] + off[st])
        dst.append(e[1] + off[dt])
        et.append(np.full(e.shape[1], i))
    src, dst, et = (np.concatenate(v).astype(np.int64) for v in (src, dst, et))
    o = np.argsort(dst, kind="stable")             # edge ids = CSR positions (dst-major, stable)
    ntype = np.repeat(np.arange(4), counts).astype(np.int64)
    local = np.concatenate([np.arange(c) for c in counts]).astype(np.int64)
    return src[o], dst[o], et[o], ntype, local, int(off[P]), batch


def check_cases(adj_in_src, adj_in_dst, n_batch, n_id, ntype):
    """conditions (a)-(d) of the schema fixture, from the innermost block's (the batch's) local
    source / target ids; the self loops are not in the adjs (the model appends one per target)."""
    s, d = np.asarray(adj_in_src), np.asarray(adj_in_dst)
    out_cnt = np.bincount(s[s < n_batch], minlength=n_batch) + 1      # transposed entries + self
    in_cnt = np.bincount(d, minlength=n_batch) + 1                    # in-entries + self
    assert (out_cnt > 16).any(), "(a) no batch target is a hub row of the transposed index"
    assert (out_cnt == 1).any(), "(b) no batch target with its self loop as only transposed entry"
    assert (in_cnt == 1).any() and (in_cnt == 26).any(), "(c) in-entry counts 1 and 26"
    src_types = np.unique(np.asarray(ntype)[np.asarray(n_id)[np.unique(np.concatenate(
        [s, np.arange(n_batch)]))]])
    assert src_types.size >= 3, "(d) fewer than three node types among the layer-0 targets"


def gen_schema():
    regnn_layers, SO = _setup()
    rng = np.random.default_rng(177)
    counts = [170, 40, 14, 130]                    # author, field_of_study, institution, paper
    src, dst, edge_type, ntype, local, p0, batch = _schema_graph(rng, counts)
    N = int(sum(counts))
    ptr = _csr_ptr(dst, N)
    batch = (p0 + batch).astype(np.int64)
    sizes, seed, epoch, batch_idx = [25, 20], 321, 0, 4
    _, n_id, adjs = SO.neighbor_sample(ptr, src, batch.tolist(), sizes, seed, epoch, batch_idx)
    check_cases(adjs[-1][0], adjs[-1][1], batch.size, n_id, ntype)
    K, H, C = 128, 64, 349
    y = np.full(N, -1, np.int64)
    y[p0:] = rng.integers(0, C, counts[3])
    args = SimpleNamespace(model="regcn", feats_type=3, self_loop_type=2, no_re=False)
    REGNN = MG._reference_regnn_class(args, {t: counts[t] for t in range(4)}, 3, regnn_layers)
    torch.manual_seed(14)
    model = REGNN(K, H, C, 1, 2, 10.0, 0.0, {t: K for t in range(4)}, 7, True, False,
                  use_norm="ln")
    MG._set_params(model, rng, ew_alpha=10.0)
    model.eval()
    x_dict = {t: torch.from_numpy((MG.f32(rng, counts[t], K) if t == 3 else
                                   rng.uniform(-0.5, 0.5, (counts[t], K)).astype(np.float32))
                                  .astype(np.float64)) for t in range(4)}
    out, loss = _run(model, x_dict, n_id, adjs, edge_type, ntype, local, y[batch])
    st = dict(src=src, dst=dst, edge_type=edge_type, ntype=ntype, local=local, y=y, batch=batch,
              n_id=np.asarray(n_id, np.int64), logp=out, loss=loss.detach())
    _store(st, x_dict, adjs, model)
    MG.save("nsres_regnn_schema",
            dict(model="mag.REGNN", feats_type=3, in_channels=K, hidden=H, classes=C,
                 num_layers=2, scaling_factor=10.0, num_edge_types=7, counts=counts,
                 target_type=3, target_offset=p0, y_global=True, sizes=sizes, seed=seed,
                 epoch=epoch, batch_idx=batch_idx, use_norm="ln", self_loop_type=2, dropout=0.0,
                 schema="ogbn-mag", residual=True), st)


def gen_ft3():
    """make_golden.gen_regnn's graph and batch recipe (relations drawn at random: the edge pass),
    feats_type 3, with residual."""
    regnn_layers, SO = _setup()
    rng = np.random.default_rng(150)
    counts = [40, 50, 8, 12]                       # paper (target), author, institution, field
    N = sum(counts)
    ntype = np.repeat(np.arange(4), counts)
    local = np.concatenate([np.arange(c) for c in counts])
    E = 900
    src = rng.integers(0, N, E)
    dst = rng.integers(0, N, E)
    dst[:40] = rng.integers(0, 3, 40)              # a few hub targets (rows longer than the fan-out)
    order = np.argsort(dst, kind="stable")         # edge ids = CSR positions of the dst-major CSR
    src, dst = src[order].astype(np.int64), dst[order].astype(np.int64)
    edge_type = rng.integers(0, 7, E).astype(np.int64)
    ptr = _csr_ptr(dst, N)
    batch = rng.choice(counts[0], 12, replace=False).astype(np.int64)
    sizes, seed, epoch, batch_idx = [4, 3], 9, 1, 3
    _, n_id, adjs = SO.neighbor_sample(ptr, src, batch.tolist(), sizes, seed, epoch, batch_idx)
    K, H, C = 64, 64, 5
    y = rng.integers(0, C, counts[0]).astype(np.int64)
    args = SimpleNamespace(model="regcn", feats_type=3, self_loop_type=2, no_re=False)
    REGNN = MG._reference_regnn_class(args, {t: counts[t] for t in range(4)}, 0, regnn_layers)
    torch.manual_seed(15)
    model = REGNN(K, H, C, 1, 2, 10.0, 0.0, {t: K for t in range(4)}, 7, True, False,
                  use_norm="ln")
    MG._set_params(model, rng, ew_alpha=10.0)
    model.eval()
    x_dict = {t: torch.from_numpy(MG.f32(rng, counts[t], K).astype(np.float64)) for t in range(4)}
    out, loss = _run(model, x_dict, n_id, adjs, edge_type, ntype, local, y[batch])
    st = dict(src=src, dst=dst, edge_type=edge_type, ntype=ntype, local=local, y=y, batch=batch,
              n_id=np.asarray(n_id, np.int64), logp=out, loss=loss.detach())
    _store(st, x_dict, adjs, model)
    MG.save("nsres_regnn_ft3",
            dict(model="mag.REGNN", feats_type=3, in_channels=K, hidden=H, classes=C,
                 num_layers=2, scaling_factor=10.0, num_edge_types=7, counts=counts, sizes=sizes,
                 seed=seed, epoch=epoch, batch_idx=batch_idx, use_norm="ln", self_loop_type=2,
                 dropout=0.0, residual=True), st)


if __name__ == "__main__":
    torch.set_default_dtype(torch.float64)
    which = sys.argv[1:] or ["schema", "ft3"]
    if "schema" in which:
        gen_schema()
    if "ft3" in which:
        gen_ft3()
