"""What the tests of the gather form of the device-block attention backwards share
(test_cpu_ns_gat_src.py, test_gpu_ns_gat_src.py; regnn_ns_block_tidx, regnn_ns_gat_bwd_gather,
regnn_ns_gatv2_bwd_gather, ops.NS_GAT_SRC). A plain helper: no test lives here, and nothing here
needs a GPU.

* tidx_reference  the canonical transposed index of a padded block in numpy: the stable sort of
                  the live entries by source
* pieces_reference  the long segments' piece list the index contract defines, from t_ptr
* hub_block       a block whose hub sources have chunk - 1, chunk, chunk + 1, 2 chunk + 3 and
                  2 chunk + 8 .. entries, with garbage in the unread tail of idx
* boundary_block  a block without random draws whose hub segments have exactly chunk - 1, chunk,
                  chunk + 1, 2 chunk and 2 chunk + 1 entries
* gat_case / gatv2_case, gat_ref / gatv2_ref  inputs and fp64 references of one (block, recipe,
                  H, C), the references computed once and left unchanged
"""
import numpy as np
import torch

import _attention_ref as R
import _ns_gat_blocks as B

HUB = dict(cap_src=1024, live_src=800, n_edge_types=7, n_rel=11)
HUB_SOURCES = (700, 701, 702, 703, 704)
HUB_SHAPES = [(8, 64), (3, 8)]
GUARD_SHAPES = [(8, 64), (3, 8), (1, 64), (4, 16)]
RECIPES = ["unit", "wide"]

_CACHE = {}


def live_entries(blk):
    """(positions e, rows v, sources u) of the block's live entries, e ascending: e in
    [ptr[v], ptr[v + 1]) for a row v < cap_dst and 0 <= idx[e] < n_src"""
    ptr = blk.csr_ptr.cpu().numpy().astype(np.int64)
    idx = blk.csr_idx.cpu().numpy().astype(np.int64)
    cnt = ptr[1:] - ptr[:-1]
    row = np.repeat(np.arange(blk.n_dst), cnt)
    pos = np.concatenate([np.arange(ptr[v], ptr[v + 1]) for v in range(blk.n_dst)] or
                         [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    src = idx[pos]
    ok = (src >= 0) & (src < blk.n_src)
    return pos[ok], row[ok], src[ok]


def tidx_reference(blk):
    """(t_ptr [cap_src + 1], t_pos [n], t_row [n]) int64, n = the live entries"""
    pos, row, src = live_entries(blk)
    order = np.argsort(src, kind="stable")
    t_ptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=blk.n_src))])
    return t_ptr.astype(np.int64), pos[order], row[order]


def pieces_reference(t_ptr, chunk):
    """[(source, first slot, count, piece, pieces of the row)]: sources ascending, the pieces of
    a row of more than `chunk` entries consecutive"""
    out = []
    for u in range(len(t_ptr) - 1):
        n = int(t_ptr[u + 1] - t_ptr[u])
        if n <= chunk:
            continue
        k = -(-n // chunk)
        out += [(u, int(t_ptr[u]) + i * chunk, min(chunk, n - i * chunk), i, k) for i in range(k)]
    return out


def hub_dims(chunk):
    return dict(HUB, cap_dst=2 * chunk + 64, live_dst=2 * chunk + 8)


def hub_block(chunk):
    """live_dst = 2 chunk + 8 rows of cap_dst = 2 chunk + 64. Row v holds, in this order: the hub
    sources (700: every live row, 701: rows < chunk + 1, 702: rows < chunk, 703: rows < chunk - 1,
    704: rows < 2 chunk + 3), [0, 1, 2, 4, 8, 16, 21][v % 7] random sources from [0, 800) with
    relations in [0, 7), and its self loop v last with relation 7 + v % 4. The unread tail of idx
    holds out-of-range and in-range garbage."""
    key = ("hub", chunk)
    if key in _CACHE:
        return _CACHE[key]
    c = hub_dims(chunk)
    rng = np.random.default_rng(9)
    upto = {700: c["live_dst"], 701: chunk + 1, 702: chunk, 703: chunk - 1, 704: 2 * chunk + 3}
    ptr, idx, rel = [0], [], []
    for v in range(c["live_dst"]):
        hubs = [u for u in HUB_SOURCES if v < upto[u]]
        k = [0, 1, 2, 4, 8, 16, 21][v % 7]
        idx += hubs + rng.integers(0, c["live_src"], k).tolist() + [v]
        rel += rng.integers(0, c["n_edge_types"], len(hubs) + k).tolist() + \
            [c["n_edge_types"] + v % 4]
        ptr.append(len(idx))
    blk = B._pad(np.asarray(ptr, dtype=np.int64), np.asarray(idx, dtype=np.int64),
                 np.asarray(rel, dtype=np.int64), c["cap_dst"], c["cap_src"])
    tail = blk.csr_idx.numel() - blk.E
    garbage = np.resize(np.asarray([-1, c["cap_src"], 5, 700, 2 ** 31 - 1, -2 ** 31, 0, 799]), tail)
    blk.csr_idx[blk.E:] = torch.as_tensor(garbage, dtype=torch.int32)
    _CACHE[key] = blk
    return blk


BOUNDARY_SOURCES = (900, 901, 902, 903, 904)


def boundary_block(chunk):
    """2 chunk + 1 live rows of 2 chunk + 8: row v holds the sources 900 (rows < chunk - 1), 901
    (rows < chunk), 902 (rows < chunk + 1), 903 (rows < 2 chunk), 904 (every row) and its self
    loop v -- no random draw, so the segments of 900 .. 904 have exactly chunk - 1, chunk,
    chunk + 1, 2 chunk and 2 chunk + 1 entries; the same garbage in the tail of idx."""
    key = ("boundary", chunk)
    if key in _CACHE:
        return _CACHE[key]
    live = 2 * chunk + 1
    upto = {900: chunk - 1, 901: chunk, 902: chunk + 1, 903: 2 * chunk, 904: live}
    ptr, idx, rel = [0], [], []
    for v in range(live):
        hubs = [u for u in BOUNDARY_SOURCES if v < upto[u]]
        idx += hubs + [v]
        rel += [(v + i) % 7 for i in range(len(hubs))] + [7 + v % 4]
        ptr.append(len(idx))
    blk = B._pad(np.asarray(ptr, dtype=np.int64), np.asarray(idx, dtype=np.int64),
                 np.asarray(rel, dtype=np.int64), 2 * chunk + 8, HUB["cap_src"])
    tail = blk.csr_idx.numel() - blk.E
    garbage = np.resize(np.asarray([-1, HUB["cap_src"], 5, 904, 2 ** 31 - 1, -2 ** 31]), tail)
    blk.csr_idx[blk.E:] = torch.as_tensor(garbage, dtype=torch.int32)
    _CACHE[key] = blk
    return blk


def ladder_block():
    if "ladder" not in _CACHE:
        _CACHE["ladder"] = B.ladder_block()
    return _CACHE["ladder"]


def block_of(name, chunk):
    """(block, its dims) of "ladder" or "hub" """
    return (ladder_block(), B.LADDER) if name == "ladder" else (hub_block(chunk), hub_dims(chunk))


def gat_case(dims, recipe, H, C):
    """(ft, el, er, tab, gy, slope), fp32 CPU tensors: gy zero past the live rows"""
    ft, el, er, tab, gy, slope = R.gat_inputs(recipe, dims["cap_src"], H, C, dims["n_rel"],
                                              seed=100 + 7 * H + C)
    er, gy = er[:dims["cap_dst"]].clone(), gy[:dims["cap_dst"]].clone()
    gy[dims["live_dst"]:] = 0.0
    return ft, el, er, tab, gy, slope


def gatv2_case(dims, recipe, H, C):
    """(xs, xd, att, tab, gy, slope), fp32 CPU tensors: xs is score operand and message"""
    fs, fd, att, tab, _ft, gy, slope = R.gatv2_inputs(recipe, dims["cap_src"], H, C,
                                                      dims["n_rel"], seed=200 + 7 * H + C)
    xd, gy = fd[:dims["cap_dst"]].clone(), gy[:dims["cap_dst"]].clone()
    gy[dims["live_dst"]:] = 0.0
    return fs, xd, att, tab, gy, slope


GAT_KEYS = ("out", "g_ft", "g_el", "g_er", "g_tab")
GATV2_KEYS = ("out", "g_xs", "g_xd", "g_att", "g_tab")


def gat_ref(name, chunk, recipe, H, C):
    """(want, scale) over GAT_KEYS, fp64"""
    key = ("gat", name, chunk, recipe, H, C)
    if key not in _CACHE:
        blk, dims = block_of(name, chunk)
        ft, el, er, tab, gy, slope = gat_case(dims, recipe, H, C)
        ptr, idx, rel = blk.live()
        _CACHE[key] = R.gat_case_ref(ptr, idx, rel, el, er, tab, ft, gy, slope,
                                     global_max="detached")
    return _CACHE[key]


def gatv2_ref(name, chunk, recipe, H, C):
    """(want, scale) over GATV2_KEYS, fp64, in ops.ns_gatv2's terms: g_xs = g_fs + g_ft"""
    key = ("gatv2", name, chunk, recipe, H, C)
    if key not in _CACHE:
        blk, dims = block_of(name, chunk)
        xs, xd, att, tab, gy, slope = gatv2_case(dims, recipe, H, C)
        ptr, idx, rel = blk.live()
        w, s = R.gatv2_case_ref(ptr, idx, rel, xs, xd, att, tab, xs, gy, slope,
                                global_max="detached")
        fold = lambda d: {"out": d["out"], "g_xs": d["g_fs"] + d["g_ft"],      # noqa: E731
                          "g_xd": d["g_fd"], "g_att": d["g_att"], "g_tab": d["g_tab"]}
        _CACHE[key] = (fold(w), fold(s))
    return _CACHE[key]
