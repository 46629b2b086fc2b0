"""Padded sampled blocks for the device-block attention tests (test_cpu_ns_gat.py,
test_gpu_ns_gat.py), in the layout regnn_ns_hop leaves (regnn_hip.ns.NSBlock, CSR form): ptr
[cap_dst + 1], idx / rel [cap_e], row v's self loop last with relation num_edge_types + node
type, the rows past the live ones empty, the entries past the last live one unread. A plain
helper: no test lives here, and nothing here needs a GPU.

* fixture_block  the block of a mag_regatconv_* golden fixture, padded to capacity
* ladder_block   40 live rows of lengths 1 .. 65 in a 64-row block over 200 of 320 sources
* conv_restated  mag REGATConv over such a block as plain torch (any dtype), the attention by
                 _attention_ref.gat_reference
"""
import numpy as np
import torch
import torch.nn.functional as F

import _attention_ref as R

CAP_DST, CAP_SRC = 128, 320          # > the fixtures' 90 targets / 260 sources
LADDER_LENGTHS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65]
LADDER = dict(cap_dst=64, live_dst=40, cap_src=320, live_src=200, n_edge_types=7, n_rel=11)


class Block:
    """what ops.ns_gat and mag.REGATConv read of an NSBlock"""

    is_ns_block = True

    def __init__(self, ptr, idx, rel, n_dst, n_src, E, device="cpu"):
        self.csr_ptr = torch.as_tensor(ptr, dtype=torch.int32).to(device)
        self.csr_idx = torch.as_tensor(idx, dtype=torch.int32).to(device)
        self.rel = torch.as_tensor(rel, dtype=torch.uint8).to(device)
        self.pos = self.row = self.inv = None
        self.n_dst, self.n_src, self.E = int(n_dst), int(n_src), int(E)   # capacities; live E
        self.device = device

    def __iter__(self):
        return iter((self, None, (self.n_src, self.n_dst)))

    def to(self, device):
        return Block(self.csr_ptr, self.csr_idx, self.rel, self.n_dst, self.n_src, self.E, device)

    def live(self):
        """(ptr, idx[:E], rel[:E]) as CPU tensors, for the references"""
        return (self.csr_ptr.cpu(), self.csr_idx[:self.E].cpu().long(),
                self.rel[:self.E].cpu().long())


def _pad(ptr, idx, rel, cap_dst, cap_src, slack=96):
    """capacity rows (empty) after the live ones, and unread entries after the last live one"""
    n_live, E = len(ptr) - 1, int(ptr[-1])
    assert n_live <= cap_dst
    ptr = np.concatenate([ptr, np.full(cap_dst - n_live, E, dtype=np.int64)])
    idx = np.concatenate([idx, np.zeros(slack, dtype=np.int64)])
    rel = np.concatenate([rel, np.zeros(slack, dtype=np.int64)])
    return Block(ptr, idx, rel, cap_dst, cap_src, E)


def fixture_block(d, cap_dst=CAP_DST, cap_src=CAP_SRC):
    """the fixture's (src, dst, edge_type, target_node_type) as a padded block: a stable sort by
    dst, then each target's self loop last in its row (relation num_edge_types + node type)."""
    m = d["meta"]
    n_dst, n_et = m["n_dst"], m["num_edge_types"]
    src, dst, et = d["src"], d["dst"], d["edge_type"]
    order = np.argsort(dst, kind="stable")
    src, dst, et = src[order], dst[order], et[order]
    cnt = np.bincount(dst, minlength=n_dst) + 1
    ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    E = int(ptr[-1])
    idx, rel = np.empty(E, dtype=np.int64), np.empty(E, dtype=np.int64)
    fill = ptr[:-1].copy()
    for s, v, r in zip(src, dst, et):
        idx[fill[v]], rel[fill[v]] = s, r
        fill[v] += 1
    loop = ptr[1:] - 1
    assert np.array_equal(fill, loop)
    idx[loop] = np.arange(n_dst)
    rel[loop] = d["target_node_type"] + n_et
    return _pad(ptr, idx, rel, cap_dst, cap_src)


def ladder_block(seed=5):
    """live rows of the lengths LADDER_LENGTHS (cycled): length 1 is the self loop alone, 64 / 65
    straddle a wave; sources drawn from the live ones with repeats, relations 0 .. 6 and the self
    loops' 7 + v % 4."""
    c = LADDER
    rng = np.random.default_rng(seed)
    lens = [LADDER_LENGTHS[v % len(LADDER_LENGTHS)] for v in range(c["live_dst"])]
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx, rel = [], []
    for v, n in enumerate(lens):
        idx += rng.integers(0, c["live_src"], n - 1).tolist() + [v]
        rel += rng.integers(0, c["n_edge_types"], n - 1).tolist() + [c["n_edge_types"] + v % 4]
    return _pad(ptr, np.asarray(idx, dtype=np.int64), np.asarray(rel, dtype=np.int64),
                c["cap_dst"], c["cap_src"])


def conv_restated(P, meta, blk, x, global_max=True):
    """mag.REGATConv.forward((x, x[:cap_dst]), blk) restated in torch over the block's live
    entries (mag/regnn_layers.py:253-325): P = the conv's parameters by name, in x's dtype."""
    H, C = meta["heads"], meta["out_channels"]
    ptr, idx, rel = blk.live()
    xs = (x @ P["lin_src.weight"].t()).view(-1, H, C)
    xd = xs[:blk.n_dst]                                       # lin_dst is lin_src
    a_s = (xs * P["att_src"]).sum(-1)
    a_d = (xd * P["att_dst"]).sum(-1)
    tab = F.leaky_relu(P["relation_weight"] * meta["scaling_factor"])
    out = R.gat_reference(ptr, idx, rel, a_s, a_d, tab, xs, meta["negative_slope"],
                          global_max=global_max)
    out = out.reshape(-1, H * C) + P["bias"]
    if meta["residual"]:
        out = out + xd.reshape(-1, H * C)
    if meta["use_norm"] == "ln":
        out = F.layer_norm(out, (H * C,), P["norm.weight"], P["norm.bias"])
    return out
