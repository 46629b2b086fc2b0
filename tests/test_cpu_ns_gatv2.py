"""The device-block GATv2 attention (regnn_ns_gatv2_fwd / _bwd, ops.ns_gatv2, mag.GATV2_BLOCKS)
without a GPU:

* the padded-block restatement the GPU tests compare against (_ns_gatv2_blocks.conv_restated,
  the attention by _attention_ref.gatv2_reference(global_max=True) with xs as score operand and
  message) reproduces the committed mag_regatv2conv_* fixtures in fp64 -- out[:90], grad_x[:260]
  and every parameter gradient at 1e-5 (_golden.close), with rows grad_x[260:] exactly 0 although
  the padded x rows hold 1e3;
* input fairness: on the ladder block the same restatement run in fp32 torch stays within
  _attention_ref.TOL_GUARD (a quarter of the kernels' bound) of the fp64 reference under the
  per-element metric, for both recipes and all six shapes of the GPU parity test and for its
  further widths (_ns_gatv2_blocks.WIDTH_SHAPES) -- so the inputs leave the kernels three
  quarters of their bound;
* the entry points' refusals, returned before any launch (fake non-NULL pointers do), the ABI
  number, which these additive symbols leave at 51, and the symbols themselves;
* the knob's host side: ns.gat_blocks_unsupported on a 'regatv2' model with it off, on, and on
  with heads x width past 2048.
"""
import numpy as np
import pytest
import torch

import _attention_ref as R
import _golden as G
import _ns_gat_blocks as B
import _ns_gatv2_blocks as V

EINVAL, EUNSUPPORTED = 1, 2


@pytest.mark.parametrize("name", V.FIXTURES)
def test_padded_block_restatement_reproduces_fixture(name):
    d = G.load(name)
    m = d["meta"]
    n_src, n_dst = m["n_src"], m["n_dst"]
    blk = B.fixture_block(d)
    assert blk.n_dst == 128 > n_dst and blk.n_src == 320 > n_src
    P = {k: torch.from_numpy(v).double().requires_grad_(True)
         for k, v in G.sub(d, "p_", np.float64).items()}
    x = torch.full((blk.n_src, d["x"].shape[1]), 1e3, dtype=torch.float64)
    x[:n_src] = torch.from_numpy(d["x"]).double()
    x.requires_grad_(True)
    out = V.conv_restated(P, m, blk, x)
    gout = torch.zeros(blk.n_dst, out.shape[1], dtype=torch.float64)
    gout[:n_dst] = torch.from_numpy(d["gout"]).double()
    out.backward(gout)
    for tag, got, want in [("out", out[:n_dst], d["out"]), ("grad_x", x.grad[:n_src], d["grad_x"])]:
        ok, err = G.close(got.detach().numpy(), want, 1e-5)
        print(f"{name} {tag}: rel err {err:.3e}")
        assert ok, f"{tag}: rel err {err:.3e}"
    assert not x.grad[n_src:].any()
    want = {k: v for k, v in G.sub(d, "grad_").items() if k != "x"}
    assert set(want) == set(P)
    for k, v in want.items():
        ok, err = G.close(P[k].grad.numpy(), v, 1e-5)
        print(f"{name} grad {k}: rel err {err:.3e}")
        assert ok, f"grad {k}: rel err {err:.3e}"


CASES = [(r, H, C) for H, C in V.SHAPES for r in V.RECIPES] + \
        [("unit", H, C) for H, C in V.WIDTH_SHAPES]


@pytest.mark.parametrize("recipe,H,C", CASES)
def test_fp32_restatement_stays_inside_the_guard(recipe, H, C):
    want, scale = V.ladder_ref(recipe, H, C)
    xs, xd, att, tab, gy, slope = V.ladder_case(recipe, H, C)
    ptr, idx, rel = V.ladder_block().live()
    fs, ft, xd, att, tab = [t.clone().requires_grad_(True) for t in (xs, xs, xd, att, tab)]
    out = R.gatv2_reference(ptr, idx, rel, fs, xd, att, tab, ft, slope, global_max="detached")
    out.backward(gy)
    got = {"out": out.detach(), "g_xs": fs.grad + ft.grad, "g_xd": xd.grad, "g_att": att.grad,
           "g_tab": tab.grad}
    errs = {k: R.rel_err(got[k], want[k], scale[k]) for k in V.KEYS}
    print(f"fp32 restatement {recipe} H={H} C={C}: " +
          " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= R.TOL_GUARD, f"{k}: {v:.3e}"


def _fwd(H=8, C=64, **null):
    from regnn_hip import _lib
    f = 0x10000
    p = dict.fromkeys(("ptr", "idx", "rel", "xs", "xd", "att", "tab", "a", "out", "work"), f)
    p.update(null)
    return _lib._so.regnn_ns_gatv2_fwd(p["ptr"], p["idx"], p["rel"], p["xs"], p["xd"], p["att"],
                                       p["tab"], 0.2, 64, 320, H, C, p["a"], p["out"], p["work"],
                                       None)


def _bwd(H=8, C=64, n_rel=11, rows=16, **null):
    from regnn_hip import _lib
    f = 0x10000
    p = dict.fromkeys(("ptr", "idx", "rel", "xs", "xd", "att", "tab", "a", "gy", "g_xs", "g_xd",
                       "att_slab", "tab_slab"), f)
    p.update(null)
    return _lib._so.regnn_ns_gatv2_bwd(p["ptr"], p["idx"], p["rel"], p["xs"], p["xd"], p["att"],
                                       p["tab"], p["a"], p["gy"], 0.2, 64, 320, H, C, n_rel,
                                       p["g_xs"], p["g_xd"], p["att_slab"], p["tab_slab"], rows,
                                       None)


def test_null_pointers_are_invalid_arguments():
    for name in ("ptr", "idx", "xs", "xd", "att", "a", "out", "work"):
        assert _fwd(**{name: None}) == EINVAL, name
    assert _fwd(rel=None) == EINVAL                            # a table without relation ids
    for name in ("ptr", "idx", "xs", "xd", "att", "a", "gy", "g_xs", "g_xd"):
        assert _bwd(**{name: None}) == EINVAL, name
    assert _bwd(rel=None) == EINVAL
    assert _bwd(tab=None) == EINVAL                            # a relation slab without a table
    assert _bwd(rows=0) == EINVAL                              # slabs without rows to write


@pytest.mark.parametrize("H,C", [(17, 64), (0, 64), (8, 6), (8, 516), (8, 0), (16, 256)])
def test_unsupported_shapes_are_refused_before_any_launch(H, C):
    assert _fwd(H=H, C=C) == EUNSUPPORTED
    assert _bwd(H=H, C=C) == EUNSUPPORTED


def test_slabs_beyond_their_budgets_are_unsupported():
    assert _bwd(H=16, C=64, n_rel=65) == EUNSUPPORTED          # 16 x 65 > REGNN_NS_GAT_MAX_BINS
    assert _bwd(rows=2049) == EUNSUPPORTED                     # > REGNN_NS_GAT_WORK_FLOATS


def test_abi_number_unchanged_and_symbols_declared():
    from regnn_hip import _lib, build
    assert _lib._so.regnn_abi_version() == _lib.ABI_VERSION == build.header_abi() == 51
    assert {"regnn_ns_gatv2_fwd", "regnn_ns_gatv2_bwd"} <= set(_lib.EXPORTED)


def _regatv2(hidden=8, heads=2):
    from regnn_hip import mag
    return mag.REGNN(16, hidden, 5, 2, 10.0, 0.0, {k: 16 for k in range(4)}, 7, model="regatv2",
                     heads=heads, use_norm="ln", self_loop_type=2)


def test_knob_gates_the_trainer_check(monkeypatch):
    from regnn_hip import mag, ns
    x_dict = {k: torch.zeros(1, 16) for k in range(4)}
    model = _regatv2()
    monkeypatch.setitem(mag.GATV2_BLOCKS, "mode", "off")
    why = ns.gat_blocks_unsupported(model, x_dict)
    assert why is not None and why.startswith("regatv2: GATv2 scores have no device-block "
                                              "operator")
    monkeypatch.setitem(mag.GATV2_BLOCKS, "mode", "on")
    assert ns.gat_blocks_unsupported(model, x_dict) is None
    wide = _regatv2(hidden=260, heads=8)                       # 8 x 260 = 2080 > 2048
    why = ns.gat_blocks_unsupported(wide, x_dict)
    assert why is not None and "2048" in why
    assert ns.gat_blocks_unsupported(_regatv2(hidden=256, heads=8), x_dict) is None
    bf16 = {k: v.bfloat16() for k, v in x_dict.items()}
    assert ns.gat_blocks_unsupported(model, bf16) is not None


def test_knob_is_off_by_default():
    import os
    from regnn_hip import mag
    if "REGNN_GATV2_BLOCKS" not in os.environ:
        assert mag.GATV2_BLOCKS["mode"] == "off"
