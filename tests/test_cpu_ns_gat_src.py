"""The gather form of the device-block attention backwards (regnn_ns_block_tidx,
regnn_ns_gat_bwd_gather, regnn_ns_gatv2_bwd_gather, ops.NS_GAT_SRC) without a GPU:

* _ns_gat_src.tidx_reference (what the GPU test holds the index to, exactly) against a brute-force
  loop over the sources, on the ladder block and on the hub block: dead rows and the garbage in
  the unread tail of idx contribute nothing, every segment ascends, and the hub segments have
  the lengths the piece list is meant to meet (one entry under a piece, a piece exactly full, one
  entry over, three pieces) -- on the boundary block exactly, which no random draw touches;
* input fairness on the hub block: the torch restatement of both operators run in fp32 stays
  within _attention_ref.TOL_GUARD (a quarter of the kernels' bound) of the fp64 reference under
  the per-element metric -- hub sources sum several hundred terms, so this is the guard that the
  inputs, not the kernels, are well conditioned;
* every new entry point's refusals, returned before any launch (fake non-NULL pointers do), the
  ABI number, which these additive symbols leave at 51, and the symbols themselves;
* the knob: "atomic" by default, a junk value raises at first use.
"""
import numpy as np
import pytest
import torch

import _attention_ref as R
import _ns_gat_src as S

EINVAL, EUNSUPPORTED = 1, 2
F = 0x10000                                   # a fake non-NULL pointer: nothing may launch


def _chunk():
    from regnn_hip import ops
    return ops.NS_TIDX_CHUNK


@pytest.mark.parametrize("name", ["ladder", "hub"])
def test_tidx_reference_against_brute_force(name):
    blk, dims = S.block_of(name, _chunk())
    t_ptr, t_pos, t_row = S.tidx_reference(blk)
    ptr = blk.csr_ptr.numpy()
    idx = blk.csr_idx.numpy()
    assert ptr[dims["live_dst"]] == ptr[-1] == blk.E < idx.size     # dead rows, an unread tail
    segs = {u: [] for u in range(blk.n_src)}       # per source, by a walk over the rows in order
    for v in range(blk.n_dst):
        for e in range(ptr[v], ptr[v + 1]):
            if 0 <= idx[e] < blk.n_src:
                segs[int(idx[e])].append((e, v))
    at = 0
    for u in range(blk.n_src):
        seg = segs[u]
        assert t_ptr[u] == at and t_ptr[u + 1] == at + len(seg), u
        assert [int(e) for e in t_pos[at:at + len(seg)]] == [e for e, _ in seg], u
        assert [int(v) for v in t_row[at:at + len(seg)]] == [v for _, v in seg], u
        assert all(a < b for a, b in zip(seg, seg[1:])), u          # ascending positions
        at += len(seg)
    # every entry of the live rows names a source in range here; none of the tail is counted
    assert at == t_ptr[-1] == blk.E == len(t_pos) == len(t_row)
    assert (np.diff(t_ptr[dims["live_src"]:]) == 0).all()          # sources nothing names


def test_hub_block_meets_the_piece_boundaries():
    c = _chunk()
    blk = S.hub_block(c)
    assert c != 256 or blk.E == 6172
    tail = blk.csr_idx[blk.E:].tolist()
    assert -1 in tail and blk.n_src in tail and 5 in tail          # out of range and in range
    idx = blk.csr_idx[:blk.E].numpy()
    rng_hits = {u: int((idx == u).sum()) for u in S.HUB_SOURCES}
    t_ptr, _, _ = S.tidx_reference(blk)
    lens = {u: int(t_ptr[u + 1] - t_ptr[u]) for u in S.HUB_SOURCES}
    assert lens == rng_hits
    # the construction's own counts (a random draw may add to them): at least these
    floor = {700: 2 * c + 8, 701: c + 1, 702: c, 703: c - 1, 704: 2 * c + 3}
    assert all(lens[u] >= floor[u] for u in floor)
    pieces = S.pieces_reference(t_ptr, c)
    per_row = {}
    for u, first, n, i, k in pieces:
        assert 1 <= n <= c and 0 <= i < k
        per_row.setdefault(u, []).append((first, n, i, k))
    assert sorted(per_row) == list(per_row)                         # sources ascending
    for u, ps in per_row.items():
        assert [p[2] for p in ps] == list(range(ps[0][3]))          # consecutive, numbered
        assert sum(p[1] for p in ps) == lens.get(u, sum(p[1] for p in ps)) > c
    assert max(k for *_x, k in pieces) >= 3
    print("hub segments", lens, "pieces", len(pieces))


def test_boundary_block_has_the_exact_piece_boundaries():
    c = _chunk()
    blk = S.boundary_block(c)
    t_ptr, t_pos, _ = S.tidx_reference(blk)
    lens = [int(t_ptr[u + 1] - t_ptr[u]) for u in S.BOUNDARY_SOURCES]
    assert lens == [c - 1, c, c + 1, 2 * c, 2 * c + 1]
    pieces = S.pieces_reference(t_ptr, c)
    # c - 1 and c are short; c + 1: a full piece and one entry; 2c: two full; 2c + 1: three
    assert [(u, n, i, k) for u, _f, n, i, k in pieces] == [
        (902, c, 0, 2), (902, 1, 1, 2), (903, c, 0, 2), (903, c, 1, 2),
        (904, c, 0, 3), (904, c, 1, 3), (904, 1, 2, 3)]


@pytest.mark.parametrize("recipe", S.RECIPES)
@pytest.mark.parametrize("H,C", S.GUARD_SHAPES)
def test_fp32_gat_restatement_inside_the_guard_on_the_hub_block(recipe, H, C):
    c = _chunk()
    blk, dims = S.block_of("hub", c)
    want, scale = S.gat_ref("hub", c, recipe, H, C)
    ft, el, er, tab, gy, slope = S.gat_case(dims, recipe, H, C)
    ptr, idx, rel = blk.live()
    el, er, tab, ft = [t.clone().requires_grad_(True) for t in (el, er, tab, ft)]
    out = R.gat_reference(ptr, idx, rel, el, er, tab, ft, slope, global_max="detached")
    out.backward(gy)
    got = {"out": out.detach(), "g_ft": ft.grad, "g_el": el.grad, "g_er": er.grad,
           "g_tab": tab.grad}
    errs = {k: R.rel_err(got[k], want[k], scale[k]) for k in S.GAT_KEYS}
    print(f"fp32 gat restatement, hub, {recipe} H={H} C={C}: " +
          " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= R.TOL_GUARD, f"{k}: {v:.3e}"


@pytest.mark.parametrize("recipe", S.RECIPES)
@pytest.mark.parametrize("H,C", S.GUARD_SHAPES)
def test_fp32_gatv2_restatement_inside_the_guard_on_the_hub_block(recipe, H, C):
    c = _chunk()
    blk, dims = S.block_of("hub", c)
    want, scale = S.gatv2_ref("hub", c, recipe, H, C)
    xs, xd, att, tab, gy, slope = S.gatv2_case(dims, recipe, H, C)
    ptr, idx, rel = blk.live()
    fs, ft, xd, att, tab = [t.clone().requires_grad_(True) for t in (xs, xs, xd, att, tab)]
    out = R.gatv2_reference(ptr, idx, rel, fs, xd, att, tab, ft, slope, global_max="detached")
    out.backward(gy)
    got = {"out": out.detach(), "g_xs": fs.grad + ft.grad, "g_xd": xd.grad, "g_att": att.grad,
           "g_tab": tab.grad}
    errs = {k: R.rel_err(got[k], want[k], scale[k]) for k in S.GATV2_KEYS}
    print(f"fp32 gatv2 restatement, hub, {recipe} H={H} C={C}: " +
          " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= R.TOL_GUARD, f"{k}: {v:.3e}"


# ---- the entry points' refusals ------------------------------------------------------------------
CAP_DST, CAP_SRC, CAP_E = 64, 320, 4096


def _tidx(cap_dst=CAP_DST, n_src=CAP_SRC, cap_src=CAP_SRC, cap_e=CAP_E, long_ints=None,
          work_ints=None, **null):
    from regnn_hip import _lib
    so = _lib._so
    p = dict.fromkeys(("ptr", "idx", "t_ptr", "t_pos", "t_row", "t_long", "work"), F)
    p.update(null)
    if long_ints is None:
        long_ints = so.regnn_ns_tidx_long_ints(max(cap_e, 0))
    if work_ints is None:
        work_ints = so.regnn_ns_tidx_work_ints(max(cap_src, 0), max(cap_e, 0))
    return so.regnn_ns_block_tidx(p["ptr"], p["idx"], cap_dst, n_src, cap_src, cap_e, p["t_ptr"],
                                  p["t_pos"], p["t_row"], p["t_long"], long_ints, p["work"],
                                  work_ints, None)


def _work(H, C):
    from regnn_hip import _lib
    return _lib._so.regnn_ns_gat_src_work_floats(CAP_E, max(H, 0) * max(C, 0))


_INDEX = ("t_ptr", "t_pos", "t_row", "t_long", "ent", "piece_work")


def _gat(H=8, C=64, n_rel=11, rows=16, work=None, cap_e=CAP_E, n_out=CAP_SRC, **null):
    from regnn_hip import _lib
    p = dict.fromkeys(("ptr", "idx", "rel", "el", "er", "tab", "ft", "a", "gy", "g_ft", "g_el",
                       "g_er", "slab") + _INDEX, F)
    p.update(null)
    return _lib._so.regnn_ns_gat_bwd_gather(
        p["ptr"], p["idx"], p["rel"], p["el"], p["er"], p["tab"], p["ft"], p["a"], p["gy"], 0.2,
        CAP_DST, CAP_SRC, H, C, n_rel, p["g_ft"], p["g_el"], p["g_er"], p["slab"], rows,
        p["t_ptr"], p["t_pos"], p["t_row"], p["t_long"], CAP_SRC, n_out, cap_e, p["ent"],
        p["piece_work"], _work(H, C) if work is None else work, None)


def _gatv2(H=8, C=64, n_rel=11, rows=16, work=None, cap_e=CAP_E, n_out=CAP_SRC, **null):
    from regnn_hip import _lib
    p = dict.fromkeys(("ptr", "idx", "rel", "xs", "xd", "att", "tab", "a", "gy", "g_xs", "g_xd",
                       "att_slab", "tab_slab") + _INDEX, F)
    p.update(null)
    return _lib._so.regnn_ns_gatv2_bwd_gather(
        p["ptr"], p["idx"], p["rel"], p["xs"], p["xd"], p["att"], p["tab"], p["a"], p["gy"], 0.2,
        CAP_DST, CAP_SRC, H, C, n_rel, p["g_xs"], p["g_xd"], p["att_slab"], p["tab_slab"], rows,
        p["t_ptr"], p["t_pos"], p["t_row"], p["t_long"], CAP_SRC, n_out, cap_e, p["ent"],
        p["piece_work"], _work(H, C) if work is None else work, None)


def test_null_pointers_and_negative_sizes_are_invalid_arguments():
    for name in ("ptr", "idx", "t_ptr", "t_pos", "t_row", "t_long", "work"):
        assert _tidx(**{name: None}) == EINVAL, name
    for kw in (dict(cap_dst=-1), dict(n_src=-1), dict(cap_src=-1), dict(cap_e=-1),
               dict(long_ints=-1), dict(work_ints=-1), dict(n_src=CAP_SRC + 1)):
        assert _tidx(**kw) == EINVAL, kw
    for name in ("ptr", "idx", "el", "er", "ft", "a", "gy", "g_ft", "g_el", "g_er") + _INDEX:
        assert _gat(**{name: None}) == EINVAL, name
    assert _gat(rel=None) == EINVAL                             # a table without relation ids
    assert _gat(tab=None) == EINVAL                             # a relation slab without a table
    assert _gat(rows=0) == EINVAL
    assert _gat(cap_e=-1) == EINVAL and _gat(n_out=-1) == EINVAL and _gat(work=-1) == EINVAL
    for name in ("ptr", "idx", "xs", "xd", "att", "a", "gy", "g_xs", "g_xd") + _INDEX:
        assert _gatv2(**{name: None}) == EINVAL, name
    assert _gatv2(rel=None) == EINVAL
    assert _gatv2(tab=None) == EINVAL
    assert _gatv2(rows=0) == EINVAL
    assert _gatv2(cap_e=-1) == EINVAL and _gatv2(n_out=-1) == EINVAL and _gatv2(work=-1) == EINVAL


# the unsupported (H, C) list of test_cpu_ns_gatv2.py; (16, 256) = 4096 columns is GATv2's alone
@pytest.mark.parametrize("H,C", [(17, 64), (0, 64), (8, 6), (8, 516), (8, 0), (16, 256)])
def test_unsupported_shapes_are_refused_before_any_launch(H, C):
    assert _gatv2(H=H, C=C) == EUNSUPPORTED
    if (H, C) != (16, 256):
        assert _gat(H=H, C=C) == EUNSUPPORTED


def test_budgets_exceeded_are_unsupported():
    from regnn_hip import _lib, ops
    so = _lib._so
    # the piece list and the build's scratch: sized by the capacities, checked before any launch
    assert so.regnn_ns_tidx_long_ints(CAP_E) == 4 + 4 * (2 * (CAP_E // ops.NS_TIDX_CHUNK) + 2)
    assert _tidx(long_ints=so.regnn_ns_tidx_long_ints(CAP_E) - 1) == EUNSUPPORTED
    assert _tidx(work_ints=so.regnn_ns_tidx_work_ints(CAP_SRC, CAP_E) - 1) == EUNSUPPORTED
    # capacities beyond the packed fields (int32 slots, 16-bit piece numbers)
    assert _tidx(cap_e=2 ** 31 - 1, long_ints=2 ** 40, work_ints=2 ** 40) == EUNSUPPORTED
    assert _tidx(cap_src=2 ** 31 - 1, long_ints=2 ** 40, work_ints=2 ** 40) == EUNSUPPORTED
    assert _tidx(cap_e=65535 * ops.NS_TIDX_CHUNK, long_ints=2 ** 40,
                 work_ints=2 ** 40) == EUNSUPPORTED
    # the piece workspace and the slabs
    assert so.regnn_ns_gat_src_work_floats(CAP_E, 512) >= (CAP_E // ops.NS_TIDX_CHUNK + 1) * 512
    assert _gat(work=_work(8, 64) - 1) == EUNSUPPORTED
    assert _gatv2(work=_work(8, 64) - 1) == EUNSUPPORTED
    assert _gat(H=16, C=64, n_rel=65) == EUNSUPPORTED          # 16 x 65 > REGNN_NS_GAT_MAX_BINS
    assert _gatv2(H=16, C=64, n_rel=65) == EUNSUPPORTED
    assert _gat(rows=2049) == EUNSUPPORTED                     # > REGNN_NS_GAT_WORK_FLOATS
    assert _gatv2(rows=2049) == EUNSUPPORTED


def test_abi_number_unchanged_and_symbols_declared():
    from regnn_hip import _lib, build
    assert _lib._so.regnn_abi_version() == _lib.ABI_VERSION == build.header_abi() == 51
    assert {"regnn_ns_block_tidx", "regnn_ns_tidx_long_ints", "regnn_ns_tidx_work_ints",
            "regnn_ns_gat_src_work_floats", "regnn_ns_gat_bwd_gather",
            "regnn_ns_gatv2_bwd_gather"} <= set(_lib.EXPORTED)


def test_chunk_constant_mirrors_the_header():
    import os
    import re
    from regnn_hip import build, ops
    with open(os.path.join(build.INCLUDE, "regnn_hip.h")) as f:
        m = re.search(r"#define REGNN_NS_TIDX_CHUNK (\d+)", f.read())
    assert m and int(m.group(1)) == ops.NS_TIDX_CHUNK


def test_knob_defaults_to_atomic_and_refuses_junk(monkeypatch):
    import os
    from regnn_hip import ops
    if "REGNN_NS_GAT_SRC" not in os.environ:
        assert ops.NS_GAT_SRC["mode"] == "atomic"
        assert ops.ns_gat_src_mode() == "atomic"
    monkeypatch.setitem(ops.NS_GAT_SRC, "mode", "gather")
    assert ops.ns_gat_src_mode() == "gather"
    monkeypatch.setitem(ops.NS_GAT_SRC, "mode", "scatter")
    with pytest.raises(ValueError):
        ops.ns_gat_src_mode()
    # first use inside the operator: the backward of a block attention (no GPU: the mode is
    # checked before any tensor is touched)
    with pytest.raises(ValueError):
        ops._NsGat.backward(None, torch.zeros(1), None)
    with pytest.raises(ValueError):
        ops._NsGatv2.backward(None, torch.zeros(1), None)
