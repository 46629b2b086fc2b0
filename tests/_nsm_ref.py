"""fp64 reference, case builder and error metric for the fused NS step (regnn_nsm_step:
re_nsm.hip + re_nsm2.hip) over its whole envelope -- helper of tests/test_cpu_nsm_ref.py and
tests/test_gpu_nsm_matrix.py, no tests in it.

Reference: oracle/cpu_ns.REGNNCPU over oracle/cpu_ns.Sampler's batch (bit-identical to the device
sampler; e_id = CSR positions), run in fp64. The same restatement in fp32 is the yardstick of what
fp32 arithmetic alone costs. RefModel adds what the step has and REGNNCPU lacks: the residual
(mag/regnn_layers.py:101-107,131-132), this build's hash dropout masks, and the retained
intermediates of the per-relation scale below.

Metric: own_scale_error = max|got - ref| / max|ref| of that tensor -- no floor of 1: the loss is a
mean over the batch, so every gradient is far below 1 and a floor hides errors of a fraction of a
percent of a tensor's largest element. An element whose reference is exactly zero (the lins.t
gradients of a type absent from the batch, a relation without a sampled edge) must be exactly zero.
Each relation-table gradient is also measured per element (a rare relation's entry lies far below
a common one's) against the sum that forms it with every product replaced by its absolute value
(the scheme of _attention_ref.py):

    d loss / d rw_r = alpha LeakyReLU'(alpha rw_r) sum_{e in r} inv_v sum_d (x_u W)_d g_{v,d}
    scale[r]        = alpha |LeakyReLU'(alpha rw_r)| sum_{e in r} inv_v sum_d |(x_u W)_d| |g_{v,d}|

with g the gradient at the conv's mean-aggregated rows, e over the block's entries (self loops
included), inv_v = 1 / entries of row v.

Bound: TOL = 1e-5 (the project's fp32 figure), now on each tensor's own maximum; the fp32
yardstick stays below TOL_GUARD = TOL / 4 on every case (a condition on the inputs)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import cpu_ns as CN
from oracle import regnn_oracle as O
from oracle.sampler_oracle import _mix

TOL = 1e-5
TOL_GUARD = 2.5e-6
HIDDEN = 64
ALPHA = 10.0
M64 = (1 << 64) - 1


def nsm_seed(st, layer):
    """the fused step's dropout seed of `layer` (include/regnn_hip.h, regnn_nsm_step): seed
    word, epoch and global batch of the step's sampler state."""
    return _mix((st[0] & M64) ^ _mix(((st[1] << 40) ^ (st[3] << 8) ^ (layer + 0x51ED27)) & M64))


# ---------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------
class RefModel(CN.REGNNCPU):
    """REGNNCPU + residual convs + hash dropout; keeps each conv's projected source rows and
    mean-aggregated rows (with their gradient) for the per-relation scale. conv follows
    REGNNCPU.conv line by line (its dead degree norm left out) with three differences: the
    residual, the retained intermediates, and the two reductions of _layer_norm's docstring.
    tests/test_cpu_nsm_ref.py pins it to the fixtures REGNNCPU is pinned to."""

    def __init__(self, *a, residual=False, **kw):
        super().__init__(*a, **kw)
        self.residual = bool(residual)
        self.trace = []

    def conv(self, c, x, x_t, src, dst, etype, tgt_type):
        n_t = tgt_type.numel()
        loop = torch.arange(n_t)
        src = torch.cat([src, loop])
        dst = torch.cat([dst, loop])
        et = torch.cat([etype, tgt_type + self.ne])
        e_feat = torch.zeros(et.numel(), self.ne + self.T, dtype=x.dtype).scatter_(
            1, et.view(-1, 1), 1.0)
        xs = x @ c.weight
        # (e_feat @ rw as a broadcast product + torch.sum: the gradient of rw is then a cascade
        # sum over the block's entries, not a matrix product's running sum -- see _layer_norm)
        ew = (e_feat * F.leaky_relu(c.relation_weight * self.alpha)).sum(1)
        s = torch.zeros(n_t, xs.shape[1], dtype=x.dtype).index_add_(0, dst, ew.view(-1, 1) * xs[src])
        cnt = torch.zeros(n_t, dtype=x.dtype).index_add_(0, dst, torch.ones_like(ew))
        agg = s / cnt.clamp(min=1).view(-1, 1)
        if agg.requires_grad:
            agg.retain_grad()
        out = agg + c.bias
        if self.residual:                              # regnn_layers.py:101-107,131-132
            out = out + x_t @ c.weight
        self.trace.append(dict(xs=xs.detach(), agg=agg, src=src, dst=dst, et=et, inv=1.0 / cnt))
        return _layer_norm(out, c.norm)

    def forward(self, n_id, x_dict, adjs, edge_type, node_type, local_idx, seeds=None):
        """seeds: per layer the 64-bit seed of its dropout mask (None: no dropout)."""
        self.trace = []
        x = self.group_input(x_dict, node_type[n_id], local_idx[n_id])
        nt = node_type[n_id]
        keep16 = int(round((1 - self.dropout) * 65536))
        for i, (src, dst, e_id, size) in enumerate(adjs):
            x_t = x[:size[1]]
            nt = nt[:size[1]]
            x = F.relu(self.conv(self.convs[i], x, x_t, src, dst, edge_type[e_id], nt))
            if seeds is not None:
                mask = O.dropout_mask(seeds[i], x.shape[0], x.shape[1], 4, keep16)
                x = x * torch.from_numpy(mask).to(x.dtype) / (keep16 / 65536)
        return self.out_lin(x).log_softmax(dim=-1)


def _layer_norm(x, ln):
    """torch.nn.LayerNorm written out in elementwise ops and torch.sum. The gradients of its
    weight and bias are column sums over every row of the block; F.layer_norm's CPU backward adds
    those rows one after another (in fp32 a rounding walk of ~eps sqrt(rows / 3): 3e-6 at 35,000
    rows on one thread, less on several), while autograd of the broadcast multiply and add
    reduces with torch.sum's cascade summation, whose error does not grow with the row count or
    change materially with the thread count. The same function in fp64 (golden pins)."""
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    return (x - mu) / torch.sqrt(var + ln.eps) * ln.weight + ln.bias


def masked_nll(logp, y):
    """mean nll over the targets with a label >= 0 (regnn_nsm_params.loss); with none, 0 and so
    a zero gradient (the step's finalize: nvalid > 0 ? sum / nvalid : 0)."""
    n = int((y >= 0).sum())
    return F.nll_loss(logp, y, ignore_index=-1, reduction="sum") / max(n, 1)


def sample(case):
    """oracle/cpu_ns.Sampler over the case's CSR -> (n_id, adjs as tensors, outermost first)."""
    smp = CN.Sampler(case["ptr"], case["idx"], case["N"])
    n_id, adjs = smp.sample(case["batch"], case["sizes"], case["seed"], case["epoch"],
                            case["batch_idx"])
    return n_id, [(torch.from_numpy(s), torch.from_numpy(d), torch.from_numpy(p), sz)
                  for s, d, p, sz in adjs]


def build_model(case, dtype):
    m = RefModel(case["k_in"], case.get("hidden", HIDDEN), case["C"], case["L"], ALPHA,
                 case["dropout"], case["T"], case["n_et"], residual=case["residual"]).to(dtype)
    assert {n for n, _ in m.named_parameters()} == set(case["params"])
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_(torch.from_numpy(case["params"][n]))
    return m


def run_model(model, case, dtype, n_id, adjs, state=None):
    """forward + masked nll + backward of `model` on the sampled batch -> dict(loss, logp, grads
    (fp64 arrays by parameter name; a parameter outside the graph -- REGNN.norm -- is left out),
    rel_scale (per convs.l.relation_weight), nvalid)."""
    x_dict = {t: torch.from_numpy(x).to(dtype) for t, x in enumerate(case["x"])}
    seeds = None
    if case["dropout"] > 0:
        st = state if state is not None else [case["seed"], case["epoch"], 0, case["batch_idx"]]
        seeds = [nsm_seed(st, l) for l in range(case["L"])]
    model.zero_grad()
    logp = model(torch.from_numpy(n_id), x_dict, adjs, torch.from_numpy(case["etype"]),
                 torch.from_numpy(case["ntype"]), torch.from_numpy(case["local"]), seeds=seeds)
    y = torch.from_numpy(case["labels"][case["batch"]])
    loss = masked_nll(logp, y)
    loss.backward()
    grads = {n: p.grad.detach().double().numpy() for n, p in model.named_parameters()
             if p.grad is not None}
    rel_scale = {}
    for l, (c, tr) in enumerate(zip(model.convs, model.trace)):
        g = tr["agg"].grad.double()
        term = tr["inv"].double()[tr["dst"]] * (tr["xs"].double()[tr["src"]].abs()
                                                 * g[tr["dst"]].abs()).sum(1)
        per = torch.zeros(c.relation_weight.numel(), dtype=torch.float64).index_add_(
            0, tr["et"], term)
        rwa = c.relation_weight.detach().double() * ALPHA
        slope = torch.where(rwa >= 0, torch.ones_like(rwa), torch.full_like(rwa, 0.01))
        rel_scale[f"convs.{l}.relation_weight"] = (ALPHA * slope * per).numpy()
    return dict(loss=float(loss.detach()), logp=logp.detach().double().numpy(), grads=grads,
                rel_scale=rel_scale, nvalid=int((y >= 0).sum()))


def run_reference(case, dtype=torch.float64, state=None, threads=1):
    """loss, log-probabilities and every parameter gradient of the case in `dtype` (fp64: the
    reference; fp32: the yardstick), plus the sampled n_id and block sizes. state: the step's
    sampler state words (dropout seeds); None: the case's own seed / epoch / batch index.
    threads: torch's CPU threads during the run (restored after), so a figure repeats."""
    n_id, adjs = sample(case)
    prev = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        out = run_model(build_model(case, dtype), case, dtype, n_id, adjs, state)
    finally:
        torch.set_num_threads(prev)
    out.update(n_id=n_id, sizes=[tuple(sz) for *_, sz in adjs],
               edges=[int(s.numel()) for s, *_ in adjs])
    return out


# ---------------------------------------------------------------------------------------------
# the metric
# ---------------------------------------------------------------------------------------------
def own_scale_error(got, ref, scale=None):
    """max |got - ref| / scale. scale None: max|ref| of the tensor (no floor); an array: per
    element. Where the reference (or an element's scale) is exactly zero, got must be exactly
    zero: inf otherwise."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.all(np.isfinite(got)):
        return float("inf")
    if np.any((ref == 0) & (got != 0)):
        return float("inf")
    if scale is None:
        s = float(np.abs(ref).max()) if ref.size else 0.0
        return float(np.abs(got - ref).max() / s) if s > 0 else 0.0
    scale = np.asarray(scale, np.float64)
    assert scale.shape == ref.shape
    if np.any((scale == 0) & ((ref != 0) | (got != 0))):
        return float("inf")
    live = scale > 0
    return float((np.abs(got - ref)[live] / scale[live]).max()) if live.any() else 0.0


def compare(got_loss, got_grads, ref):
    """every figure of one run against the reference `ref` (run_reference's dict): {name: own-scale
    error}, the relation tables also as "<name>[per-element]". got_grads must hold every
    gradient of the reference."""
    errs = {"loss": own_scale_error(got_loss, ref["loss"])}
    for n, r in ref["grads"].items():
        errs[n] = own_scale_error(got_grads[n], r)
        if n in ref["rel_scale"]:
            errs[n + "[per-element]"] = own_scale_error(got_grads[n], r, ref["rel_scale"][n])
    return errs


# ---------------------------------------------------------------------------------------------
# the case builder
# ---------------------------------------------------------------------------------------------
def _pair_table(rng, T, n_et, src_ok, dst_ok):
    """"slots" schema: n_et (target type, source type) pairs, one relation each; (0, 0) and a
    second source type for type 0 first, then one pair per other target type, then at random."""
    first = [(0, 0)]
    others = [b for b in range(1, T) if src_ok[b]]
    if others:
        first.append((0, others[int(rng.integers(len(others)))]))
    srcs = [b for b in range(T) if src_ok[b]]
    for a in range(1, T):
        if dst_ok[a]:
            first.append((a, srcs[int(rng.integers(len(srcs)))]))
    rest = [(a, b) for a in range(T) for b in range(T)
            if dst_ok[a] and src_ok[b] and (a, b) not in first]
    rest = [rest[i] for i in rng.permutation(len(rest))]
    pairs = (first + rest)[:n_et]
    rel = rng.permutation(n_et)[:len(pairs)]           # (fewer pairs than n_et: unused relations)
    return {p: int(r) for p, r in zip(pairs, rel)}


def make_case(T, k_in, L, C, n_edge_types, B, sizes, schema, *, residual=False, dropout=0.0,
              unlabelled=None, absent_type=None, empty_type=None, n_nodes=3000, deg=12,
              min_deg=0, seed=0, name="", hidden=HIDDEN, hub_fanin=18):
    """A small typed graph (numpy only), one batch and a model's parameters.

    Node ids grouped by type, local = id - type offset, labels -1 outside type 0; relations per
    edge under schema "slots" (one relation per (target type, source type) pair) or "random"
    (drawn at random: several per pair). absent_type: a type with nodes that are nobody's source;
    empty_type: a type without nodes (its input table keeps one unread row: a table needs an
    address). unlabelled: None, "quarter" or "all" of the batch targets get label -1.

    The batch opens with a target without in-edges, a hub (an in-neighbour of itself twice and of
    the low-degree targets below: with its self loop, its row of hop 0's transposed index holds
    17+ entries from B = 17 on, where 14 of them are other targets), a target with more in-edges
    than any fan-out, then up to hub_fanin (18) low-degree targets (<= 3 in-edges + the hub); the
    rest is drawn at random from type 0. min_deg: a floor under every other node's in-degree. What
    B allows of this is asserted below and recorded in case["edges"]. hidden: the model's width
    (64: the fused step's); it shapes the parameters only, so at 64 and hub_fanin 18 every array
    is the one the builder always drew (tests/test_cpu_nsmod_ref.py pins their hashes)."""
    assert schema in ("slots", "random") and len(sizes) == L
    rng = np.random.default_rng(1000 + seed)
    n_et = int(n_edge_types)
    # -- nodes ---------------------------------------------------------------------------------
    w = np.array([0.0 if t == empty_type else (2.0 if t == 0 else 1.0) for t in range(T)])
    counts = np.floor(n_nodes * w / w.sum()).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(counts)])
    N = int(off[-1])
    ntype = np.repeat(np.arange(T), counts).astype(np.int64)
    local = np.arange(N) - off[ntype]
    src_ok = [counts[t] > 0 and t != absent_type for t in range(T)]
    dst_ok = [counts[t] > 0 for t in range(T)]
    # -- degrees and the batch -----------------------------------------------------------------
    kmax = max(sizes)
    d = rng.integers(1, 2 * deg, N)
    heavy = rng.random(N) < 0.05
    d[heavy] = rng.integers(3 * deg, 4 * deg + 1, int(heavy.sum()))
    d = np.maximum(d, min_deg)                         # (the special targets below keep theirs)
    n_low = max(0, min(int(hub_fanin), B - 3))
    z, hub, hi = 0, 1, 2
    low = np.arange(3, 3 + n_low)
    # (the hub's and the low targets' rows stay below the first fan-out: every edge is sampled)
    d[z], d[hub], d[hi], d[low] = 0, 1, max(4 * deg, kmax + 5), max(1, min(3, sizes[0] - 2))
    special = 3 + n_low
    if B == 1:
        batch = np.array([hi])
    else:
        rest = special + rng.permutation(counts[0] - special)[:max(0, B - special)]
        batch = np.concatenate([[z, hub, hi], low, rest])[:B]
    # -- edges ---------------------------------------------------------------------------------
    dst = np.repeat(np.arange(N), d)
    dst = np.concatenate([dst, [hub, hub], low])       # the hub's own edges
    forced = np.zeros(dst.size, bool)
    forced[dst.size - 2 - n_low:] = True
    dt = ntype[dst]
    src = np.empty(dst.size, np.int64)
    rel = np.empty(dst.size, np.int64)
    pairs = None
    if schema == "slots":
        pairs = _pair_table(rng, T, n_et, src_ok, dst_ok)
        keep = np.ones(dst.size, bool)
        for a in range(T):
            m = np.nonzero(dt == a)[0]
            opts = [(b, r) for (aa, b), r in pairs.items() if aa == a]
            if not opts:                               # a target type without a pair: no in-edges
                keep[m] = False
                continue
            pick = rng.integers(len(opts), size=m.size)
            bs = np.array([o[0] for o in opts])[pick]
            src[m] = off[bs] + np.floor(rng.random(m.size) * counts[bs]).astype(np.int64)
            rel[m] = np.array([o[1] for o in opts])[pick]
        src[forced], rel[forced] = hub, pairs[(0, 0)]
        src, dst, rel = src[keep], dst[keep], rel[keep]
    else:
        pool = np.nonzero(np.array(src_ok)[ntype])[0]
        src[:] = pool[rng.integers(pool.size, size=dst.size)]
        rel[:] = rng.integers(n_et, size=dst.size)
        src[forced] = hub
    order = np.argsort(dst, kind="stable")
    src, dst, rel = src[order], dst[order], rel[order]
    ptr = np.zeros(N + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(dst, minlength=N))
    # -- labels, inputs, parameters -------------------------------------------------------------
    labels = np.full(N, -1, np.int64)
    labels[:counts[0]] = rng.integers(C, size=counts[0])
    if unlabelled == "quarter":
        labels[batch[2::4]] = -1
    elif unlabelled == "all":
        labels[batch] = -1
    x = [rng.standard_normal((max(int(c), 1), k_in)).astype(np.float32) for c in counts]
    with torch.random.fork_rng():                      # (the caller's torch RNG stays as it was)
        torch.manual_seed(seed)
        m = RefModel(k_in, hidden, C, L, ALPHA, dropout, T, n_et, residual=residual)
    n_rel = n_et + T
    with torch.no_grad():
        for c in m.convs:
            mag = rng.uniform(0.03, 0.15, n_rel)
            sign = np.where(rng.random(n_rel) < 0.3, -1.0, 1.0)
            sign[0], sign[-1] = 1.0, -1.0              # both LeakyReLU slopes, whatever the draw
            c.relation_weight.copy_(torch.from_numpy(mag * sign))
            c.bias.copy_(torch.from_numpy(rng.normal(0, 0.1, hidden)))
            c.norm.weight.copy_(torch.from_numpy(1 + rng.normal(0, 0.2, hidden)))
            c.norm.bias.copy_(torch.from_numpy(rng.normal(0, 0.1, hidden)))
    params = {n: p.detach().numpy().copy() for n, p in m.named_parameters()}
    case = dict(name=name, T=T, k_in=k_in, L=L, C=C, n_et=n_et, B=B, sizes=list(sizes),
                schema=schema, residual=residual, dropout=dropout, unlabelled=unlabelled,
                absent_type=absent_type, empty_type=empty_type, N=N, counts=counts, off=off,
                ntype=ntype, local=local, src=src, dst=dst, etype=rel, ptr=ptr, idx=src,
                labels=labels, batch=batch.astype(np.int64), x=x, params=params,
                seed=4242 + seed, epoch=1, batch_idx=3, pairs=pairs, hidden=int(hidden),
                hub_fanin=int(hub_fanin))
    case["edges"] = _check_edges(case)
    return case


def case_from_fixture(d):
    """a golden REGNN fixture (tests/golden/mag_regnn_*, nsres_regnn_*) as a case: its graph as the
    dst-major CSR (stable in edge order, as RelGraph builds it), relations per CSR position."""
    m = d["meta"]
    counts = np.asarray(m["counts"], np.int64)
    N = int(counts.sum())
    order = np.argsort(d["dst"], kind="stable")
    src, dst = d["src"][order], d["dst"][order]
    ptr = np.zeros(N + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(dst, minlength=N))
    if m.get("y_global"):
        labels = d["y"].astype(np.int64)
    else:
        labels = np.full(N, -1, np.int64)
        labels[:counts[0]] = d["y"]
    params = {k[2:]: v.astype(np.float32) for k, v in d.items() if k.startswith("p_")}
    return dict(name="fixture", T=4, k_in=m["in_channels"], L=m["num_layers"], C=m["classes"],
                n_et=m["num_edge_types"], B=int(d["batch"].size), sizes=list(m["sizes"]),
                residual=bool(m.get("residual", False)), dropout=0.0, N=N, counts=counts,
                ntype=d["ntype"], local=d["local"], src=src, dst=dst, etype=d["edge_type"][order],
                ptr=ptr, idx=src, labels=labels, batch=d["batch"].astype(np.int64),
                x=[d[f"x{t}"] for t in range(4)], params=params, seed=m["seed"],
                epoch=m["epoch"], batch_idx=m["batch_idx"])


def slots_eligible(case):
    """every (target type, source type) pair of the graph has at most one relation
    (regnn_hip.ns.relation_slots_ok's condition, on the CPU)."""
    key = (case["ntype"][case["dst"]] * case["T"] + case["ntype"][case["src"]]) * 256 + case["etype"]
    pair = np.unique(key) // 256
    return np.unique(pair).size == pair.size


def _check_edges(case):
    """the builder's own asserts: the edges the case declares are present in its sampled batch."""
    B, sizes, batch = case["B"], case["sizes"], case["batch"]
    deg = np.diff(case["ptr"])
    n_id, adjs = sample(case)
    s0, d0, _, _ = adjs[-1]                             # hop 0: the batch targets' block
    e = dict(B=B, n_id=int(n_id.size))
    assert batch.size == B and np.unique(batch).size == B
    assert np.all(case["ntype"][batch] == 0)
    assert np.all(np.diff(case["ntype"]) >= 0)
    assert np.array_equal(case["local"], np.arange(case["N"]) - case["off"][case["ntype"]])
    assert np.all(case["labels"][case["ntype"] != 0] == -1)
    e["zero_in"] = bool((deg[batch] == 0).any())
    e["more"] = bool((deg[batch] > sizes[0]).any())
    e["fewer"] = bool(((deg[batch] < sizes[0]) & (deg[batch] > 0)).any())
    hub_row = int((s0 == 1).sum()) + 1 if B > 1 else 0  # + the hub's self loop (it is target 1)
    e["long_row"] = hub_row
    e["B_odd"] = B % 16 != 0
    if B >= 17:
        assert e["zero_in"] and e["more"] and e["fewer"] and hub_row >= 17, e
    elif B == 1:
        assert e["more"], e                            # one target: the one edge that fits
    assert e["B_odd"], e
    present = np.unique(case["ntype"][n_id])
    e["types_present"] = present.tolist()
    if case["absent_type"] is not None:
        assert case["counts"][case["absent_type"]] > 0
        assert case["absent_type"] not in present
    if case["empty_type"] is not None:
        assert case["counts"][case["empty_type"]] == 0
    e["slots"] = slots_eligible(case)
    assert e["slots"] == (case["schema"] == "slots"), e
    rws = [case["params"][f"convs.{l}.relation_weight"] for l in range(case["L"])]
    for l, rw in enumerate(rws):
        assert (rw > 0).any() and (rw < 0).any() and np.unique(rw).size == rw.size
        assert all(not np.array_equal(rw, o) for o in rws[:l])
        for nm in ("bias", "norm.weight", "norm.bias"):
            assert np.all(case["params"][f"convs.{l}.{nm}"] != 0)
        assert np.any(case["params"][f"convs.{l}.norm.weight"] != 1)
    y = case["labels"][batch]
    e["unlabelled"] = int((y < 0).sum())
    want = {None: 0, "quarter": len(batch[2::4]), "all": B}[case["unlabelled"]]
    assert e["unlabelled"] == want, e
    for xt in case["x"]:
        assert xt.dtype == np.float32
    return e


# ---------------------------------------------------------------------------------------------
# the matrix (tests/test_gpu_nsm_matrix.py runs it; tests/test_cpu_nsm_ref.py guards its inputs)
# ---------------------------------------------------------------------------------------------
def _spec(id, form, rel_slots, pre_sums, **kw):
    return dict(id=id, form=form, rel_slots=rel_slots, pre_sums=pre_sums, kw=kw)


# form: "two" (re_nsm2.hip) / "composed" (re_nsm.hip); rel_slots / pre_sums: what FusedStep must
# report with every knob at its default. kw: make_case's arguments
MATRIX = [
    _spec("01-t4-k64-slots", "two", 1, 0, T=4, k_in=64, L=2, C=37, n_edge_types=7, B=97,
          sizes=(7, 5), schema="slots"),
    _spec("01-t4-k64-slots-drop", "two", 1, 0, T=4, k_in=64, L=2, C=37, n_edge_types=7, B=97,
          sizes=(7, 5), schema="slots", dropout=0.5),
    _spec("02-t4-k64-random", "two", 0, 0, T=4, k_in=64, L=2, C=37, n_edge_types=7, B=97,
          sizes=(7, 5), schema="random"),
    _spec("03-t1-k64-random", "two", 0, 0, T=1, k_in=64, L=2, C=5, n_edge_types=3, B=17,
          sizes=(6, 4), schema="random"),
    _spec("04-t1-k128-one-target", "two", 1, 1, T=1, k_in=128, L=2, C=1, n_edge_types=1, B=1,
          sizes=(25, 20), schema="slots"),
    _spec("05-t3-k128-rel64-c384", "two", 0, 0, T=3, k_in=128, L=2, C=384, n_edge_types=61, B=50,
          sizes=(9, 7), schema="random"),
    _spec("06-t5-k64-c349", "two", 1, 0, T=5, k_in=64, L=2, C=349, n_edge_types=12, B=97,
          sizes=(7, 5), schema="slots"),
    _spec("07-t8-k64-slots", "two", 1, 0, T=8, k_in=64, L=2, C=37, n_edge_types=20, B=33,
          sizes=(6, 4), schema="slots", absent_type=5, empty_type=6),
    _spec("07-t8-k64-random", "two", 0, 0, T=8, k_in=64, L=2, C=37, n_edge_types=20, B=33,
          sizes=(6, 4), schema="random", absent_type=5, empty_type=6),
    _spec("08-t4-k64-residual-drop", "two", 1, 0, T=4, k_in=64, L=2, C=37, n_edge_types=7, B=97,
          sizes=(7, 5), schema="slots", residual=True, dropout=0.5),
    _spec("09-t4-k128-quarter-unlabelled", "two", 1, 1, T=4, k_in=128, L=2, C=37, n_edge_types=7,
          B=97, sizes=(7, 5), schema="slots", unlabelled="quarter"),
    _spec("09-t4-k128-all-unlabelled", "two", 1, 1, T=4, k_in=128, L=2, C=37, n_edge_types=7,
          B=97, sizes=(7, 5), schema="slots", unlabelled="all"),
    _spec("10-t4-k128-modes", "two", 1, 1, T=4, k_in=128, L=2, C=37, n_edge_types=7, B=97,
          sizes=(7, 5), schema="slots"),
    _spec("11-composed-c385", "composed", 1, 0, T=4, k_in=128, L=2, C=385, n_edge_types=7, B=50,
          sizes=(7, 5), schema="slots"),
    _spec("11-composed-c448", "composed", 1, 0, T=4, k_in=128, L=2, C=448, n_edge_types=7, B=50,
          sizes=(7, 5), schema="slots"),
    _spec("12-composed-k64-c448-random", "composed", 0, 0, T=4, k_in=64, L=2, C=448,
          n_edge_types=7, B=50, sizes=(7, 5), schema="random"),
    _spec("13-composed-l3-slots", "composed", 1, 0, T=4, k_in=128, L=3, C=37, n_edge_types=7,
          B=50, sizes=(5, 4, 3), schema="slots"),
    _spec("13-composed-l3-slots-drop", "composed", 1, 0, T=4, k_in=128, L=3, C=37,
          n_edge_types=7, B=50, sizes=(5, 4, 3), schema="slots", dropout=0.5),
    _spec("13-composed-l3-random", "composed", 0, 0, T=4, k_in=128, L=3, C=37, n_edge_types=7,
          B=50, sizes=(5, 4, 3), schema="random"),
    _spec("13-composed-l3-random-drop", "composed", 0, 0, T=4, k_in=128, L=3, C=37,
          n_edge_types=7, B=50, sizes=(5, 4, 3), schema="random", dropout=0.5),
    _spec("14-composed-t5-l3", "composed", 0, 0, T=5, k_in=64, L=3, C=37, n_edge_types=9, B=50,
          sizes=(5, 4, 3), schema="random"),
    _spec("15-composed-t8-l4-c448-rel64", "composed", 0, 0, T=8, k_in=64, L=4, C=448,
          n_edge_types=56, B=33, sizes=(4, 3, 3, 2), schema="random"),
    _spec("16-composed-t2-l4", "composed", 1, 0, T=2, k_in=128, L=4, C=19, n_edge_types=4, B=20,
          sizes=(3, 3, 2, 2), schema="slots"),
    # both grid clamps loop: live layer-0 target rows > 2048 x 16, live layer-1 target rows >
    # 1024 x 16 (asserted by both test files)
    # B (20 + 1) > 16,384 needs B >= 781 before any two targets share a neighbour; every node
    # has more in-edges than the first fan-out (min_deg), and on 100,000 nodes the shared
    # neighbours cost about a seventh: 931 targets reach 16,909 and 35,377 rows. (Seed: of the
    # draws 300..307 two trip the guard by 1e-3 and 9e-6 in lins.t.weight of a rare type -- a
    # ReLU input within an fp32 rounding of 0 among 2 M -- and four miss the layer-1 clamp)
    _spec("17-composed-clamps", "composed", 1, 0, T=4, k_in=64, L=3, C=19, n_edge_types=7, B=931,
          sizes=(20, 2, 1), schema="slots", n_nodes=100_000, deg=16, min_deg=21, seed=302),
    # case 04 again with three classes: C = 1 leaves its loss and every gradient exactly zero,
    # so only this one puts figures on the T = 1, k_in = 128, one-target path
    _spec("04-t1-k128-one-target-c3", "two", 1, 1, T=1, k_in=128, L=2, C=3, n_edge_types=1, B=1,
          sizes=(25, 20), schema="slots", seed=400),
]
SPECS = {s["id"]: s for s in MATRIX}
# per MATRIX position, so two cases of one shape do not share a graph
for _i, _s in enumerate(MATRIX):
    _s["kw"].setdefault("seed", _i)
CLAMP_ID = "17-composed-clamps"
CLAMP_ROWS0, CLAMP_ROWS1 = 2048 * 16, 1024 * 16


@functools.lru_cache(maxsize=None)
def case_of(id):
    return make_case(name=id, **SPECS[id]["kw"])


@functools.lru_cache(maxsize=None)
def reference_of(id, dtype=torch.float64):
    """the case's reference, computed once and shared (callers leave it unchanged)."""
    return run_reference(case_of(id), dtype)
