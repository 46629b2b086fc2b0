"""The device-block attention (regnn_ns_gat_fwd / _bwd, ops.ns_gat) without a GPU:

* the padded-block restatement the GPU tests compare against (_ns_gat_blocks.conv_restated, the
  attention by _attention_ref.gat_reference(global_max=True)) reproduces the committed
  mag_regatconv_* fixtures in fp64 -- out[:90], grad_x[:260] and every parameter gradient at
  1e-5 (_golden.close), with rows grad_x[260:] exactly 0 although the padded x rows hold 1e3.
  (The fixtures hold duplicate (src, dst) pairs, sampled self edges, rows of the self loop alone
  and a longest row of 57.)
* the entry points' refusals, returned before any launch (fake non-NULL pointers do), and the
  ABI number, which these additive symbols leave at 51.
"""
import numpy as np
import pytest
import torch

import _golden as G
import _ns_gat_blocks as B

EINVAL, EUNSUPPORTED = 1, 2
FIXTURES = ["mag_regatconv_h2_res1", "mag_regatconv_h4_res0"]


@pytest.mark.parametrize("name", FIXTURES)
def test_padded_block_restatement_reproduces_fixture(name):
    d = G.load(name)
    m = d["meta"]
    n_src, n_dst = m["n_src"], m["n_dst"]
    blk = B.fixture_block(d)
    assert blk.n_dst == 128 > n_dst and blk.n_src == 320 > n_src
    ptr = blk.csr_ptr.numpy()
    lens = np.diff(ptr)
    assert np.all(lens[n_dst:] == 0) and lens[:n_dst].min() == 1 and lens.max() == 57
    assert int((lens[:n_dst] == 1).sum()) == 2                 # rows of the self loop alone
    P = {k: torch.from_numpy(v).double().requires_grad_(True)
         for k, v in G.sub(d, "p_", np.float64).items()}
    x = torch.full((blk.n_src, d["x"].shape[1]), 1e3, dtype=torch.float64)
    x[:n_src] = torch.from_numpy(d["x"]).double()
    x.requires_grad_(True)
    out = B.conv_restated(P, m, blk, x)
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


def _fwd(H=8, C=64, **null):
    from regnn_hip import _lib
    f = 0x10000
    p = dict.fromkeys(("ptr", "idx", "rel", "el", "er", "tab", "ft", "a", "out", "work"), f)
    p.update(null)
    return _lib._so.regnn_ns_gat_fwd(p["ptr"], p["idx"], p["rel"], p["el"], p["er"], p["tab"],
                                     p["ft"], 0.2, 64, 320, H, C, p["a"], p["out"], p["work"],
                                     None)


def _bwd(H=8, C=64, n_rel=11, **null):
    from regnn_hip import _lib
    f = 0x10000
    p = dict.fromkeys(("ptr", "idx", "rel", "el", "er", "tab", "ft", "a", "gy", "g_ft", "g_el",
                       "g_er", "slab"), f)
    p.update(null)
    return _lib._so.regnn_ns_gat_bwd(p["ptr"], p["idx"], p["rel"], p["el"], p["er"], p["tab"],
                                     p["ft"], p["a"], p["gy"], 0.2, 64, 320, H, C, n_rel,
                                     p["g_ft"], p["g_el"], p["g_er"], p["slab"], 16, None)


def test_null_pointers_are_invalid_arguments():
    for name in ("ptr", "idx", "el", "er", "ft", "a", "out", "work"):
        assert _fwd(**{name: None}) == EINVAL, name
    assert _fwd(rel=None) == EINVAL                            # a table without relation ids
    for name in ("ptr", "idx", "el", "er", "ft", "a", "gy", "g_ft", "g_el", "g_er"):
        assert _bwd(**{name: None}) == EINVAL, name
    assert _bwd(rel=None) == EINVAL
    assert _bwd(tab=None) == EINVAL                            # a slab without a table


@pytest.mark.parametrize("H,C", [(17, 64), (0, 64), (8, 6), (8, 516), (8, 0)])
def test_unsupported_shapes_are_refused_before_any_launch(H, C):
    assert _fwd(H=H, C=C) == EUNSUPPORTED
    assert _bwd(H=H, C=C) == EUNSUPPORTED


def test_relation_bins_beyond_the_lds_budget_are_unsupported():
    assert _bwd(H=16, n_rel=65) == EUNSUPPORTED                # 16 x 65 > REGNN_NS_GAT_MAX_BINS


def test_abi_number_unchanged_and_symbols_declared():
    from regnn_hip import _lib, build
    assert _lib._so.regnn_abi_version() == _lib.ABI_VERSION == build.header_abi() == 51
    assert {"regnn_ns_gat_fwd", "regnn_ns_gat_bwd"} <= set(_lib.EXPORTED)
