"""The sampler's sums launch and its layer-0 consumer at one input width per node type, CPU side:
the three C entries' refusals (regnn_ns_hop_typed_sums_kt, regnn_ns_slot_agg_kt / _bwd_kt: all
returned before any launch, so no GPU is needed), the host gate ops.typed_agg_layout_ok under
ops.NS_SUMS_KT, and the fp64 restatement the GPU tests compare against (tests/_ns_sums_kt_ref.py)
at all-128 against the equal-width restatement of tests/test_gpu_ns_type_layout.py."""
import ctypes
import types

import numpy as np
import pytest
import torch

import _ns_sums_kt_ref as R
from test_ns_type_layout import SEED, csr_by_target, hand_graph

EINVAL, EUNSUPPORTED = 1, 2
F32, BF16 = 0, 1
FAKE = 0x10000                                 # never dereferenced: validation comes first


def _widths(*w):
    return (ctypes.c_int32 * len(w))(*w)


def _sums_call(dtype=F32, table=FAKE, widths=(256, 128, 128, 128), k=5, T=4,
               meta=(FAKE, FAKE, FAKE)):
    from regnn_hip import _lib
    tabs = (ctypes.c_void_p * 8)(FAKE, FAKE, table, FAKE, FAKE, FAKE, FAKE, FAKE)
    wd = None if widths is None else _widths(*widths)
    return _lib._so.regnn_ns_hop_typed_sums_kt(
        FAKE, FAKE, FAKE, FAKE, 7, k, 1, FAKE, FAKE, FAKE, 64, FAKE, meta[0], FAKE, FAKE, meta[1],
        meta[2], tabs, dtype, T, wd, FAKE, FAKE, FAKE, FAKE, None, None, None)


def test_symbols_and_abi():
    from regnn_hip import _lib, build
    for name in ("regnn_ns_hop_typed_sums_kt", "regnn_ns_slot_agg_kt", "regnn_ns_slot_agg_bwd_kt"):
        assert hasattr(_lib._so, name) and name in _lib.EXPORTED
    # the _dt / slot parameters in their order, a pointer (widths) where K stood
    P = ctypes.c_void_p
    for new, old, at in (("regnn_ns_hop_typed_sums_kt", "regnn_ns_hop_typed_sums_dt", 20),
                         ("regnn_ns_slot_agg_kt", "regnn_ns_slot_agg", 9),
                         ("regnn_ns_slot_agg_bwd_kt", "regnn_ns_slot_agg_bwd", 10)):
        a, ret = _lib._SIG[new]
        b, _ = _lib._SIG[old]
        assert b[at] is ctypes.c_int32
        assert a == b[:at] + [P] + b[at + 1:] and ret is ctypes.c_int
    assert _lib._so.regnn_abi_version() == _lib.ABI_VERSION == build.header_abi() == 51


def test_sums_kt_refusals_come_before_any_launch():
    assert _sums_call(widths=None) == EINVAL                       # NULL widths
    assert _sums_call(dtype=2) == EINVAL                            # no such dtype
    assert _sums_call(dtype=-1) == EINVAL
    assert _sums_call(meta=(FAKE, None, FAKE)) == EINVAL            # the meta triple: all or none
    assert _sums_call(meta=(None, FAKE, None)) == EINVAL
    for dt in (F32, BF16):
        assert _sums_call(dt, table=None) == EINVAL                 # a NULL table
        assert _sums_call(dt, table=FAKE + 8) == EINVAL             # off the 16-byte grid
        for bad in (0, 32, 96, 192, 512, -128):
            assert _sums_call(dt, widths=(256, 128, bad, 128)) == EUNSUPPORTED
        assert _sums_call(dt, T=5, widths=(128,) * 5) == EUNSUPPORTED
        assert _sums_call(dt, T=0, widths=(128,)) == EUNSUPPORTED
        assert _sums_call(dt, k=64) == EUNSUPPORTED
        assert _sums_call(dt, k=0) == EUNSUPPORTED


def _slot_call(bwd, widths=(256, 128, 128, 128), T=4, ld=None, U=FAKE, out=FAKE):
    from regnn_hip import _lib
    wd = None if widths is None else _widths(*widths)
    if ld is None:
        ld = sum(widths or ()) + 4
    if bwd:
        return _lib._so.regnn_ns_slot_agg_bwd_kt(FAKE, 1, U, FAKE, FAKE, FAKE, out, ld, 7, T, wd,
                                                 FAKE, 11, 8, None)
    return _lib._so.regnn_ns_slot_agg_kt(FAKE, 1, U, FAKE, FAKE, FAKE, FAKE, 7, T, wd, 64, out, ld,
                                         None)


@pytest.mark.parametrize("bwd", [False, True])
def test_slot_kt_refusals_come_before_any_launch(bwd):
    assert _slot_call(bwd, widths=None, ld=644) == EINVAL           # NULL widths
    assert _slot_call(bwd, U=None) == EINVAL
    assert _slot_call(bwd, U=FAKE + 4) == EINVAL                    # off the 16-byte grid
    assert _slot_call(bwd, out=FAKE + 8) == EINVAL
    assert _slot_call(bwd, ld=640) == EINVAL                        # ld < sum K_t + T
    assert _slot_call(bwd, ld=646) == EINVAL                        # not a multiple of 4
    for bad in (0, 32, 96, 512):
        assert _slot_call(bwd, widths=(128, bad, 128, 128), ld=2048) == EUNSUPPORTED
    assert _slot_call(bwd, T=5, widths=(128,) * 5) == EUNSUPPORTED


def test_layout_gate_follows_the_knob(monkeypatch):
    from regnn_hip import ops
    bf, f32 = torch.bfloat16, torch.float32

    def tabs(widths, dt):
        return [torch.zeros(3, K, dtype=dt) for K in widths]
    mixed, eq = (256, 128, 128, 128), (128,) * 4
    for mode in ("off", "on"):
        monkeypatch.setitem(ops.NS_SUMS_KT, "mode", mode)
        on = mode == "on"
        assert ops.typed_agg_layout_ok(tabs(eq, bf), pre_sums=True)
        assert ops.typed_agg_layout_ok(tabs(mixed, bf), pre_sums=True) == on
        assert ops.typed_agg_layout_ok(tabs((64, 256, 128, 64), bf), pre_sums=True) == on
        assert ops.typed_agg_layout_ok(tabs((64,) * 4, bf), pre_sums=True) == on
        # never: without the sums, five tables, another width, mixed dtypes
        assert not ops.typed_agg_layout_ok(tabs(mixed, bf))
        assert not ops.typed_agg_layout_ok(tabs((128,) * 5, bf), pre_sums=True)
        assert not ops.typed_agg_layout_ok(tabs((256, 96, 128, 128), bf), pre_sums=True)
        assert not ops.typed_agg_layout_ok(tabs(mixed, bf)[:3] + tabs((128,), f32), pre_sums=True)
        # fp32 tables: what they were, whatever the knob says
        assert ops.typed_agg_layout_ok(tabs(mixed, f32))
        assert ops.typed_agg_layout_ok(tabs((128,) * 8, f32), pre_sums=True)
        assert not ops.typed_agg_layout_ok(tabs((256, 96), f32))
    monkeypatch.setitem(ops.NS_SUMS_KT, "mode", "yes")
    with pytest.raises(ValueError, match="REGNN_NS_SUMS_KT"):
        ops.typed_agg_layout_ok(tabs(mixed, bf), pre_sums=True)


@pytest.mark.parametrize("sizes", [(3, 3), (3, 33)])
def test_restatement_at_128_is_the_equal_width_one(sizes):
    """the per-type-width restatement with every width 128 against the arrays
    tests/test_gpu_ns_type_layout.py::_oracle_sums gives (on the CPU: its graph as a namespace of
    CPU tensors) -- equal, not close: the same fp64 additions in the same order."""
    import test_gpu_ns_type_layout as TL
    g = hand_graph()
    ptr, idx, eid = csr_by_target(g)
    gen = torch.Generator().manual_seed(5)
    x = {t: torch.randn(c, 128, generator=gen) for t, c in enumerate(g["counts"])}
    rg = types.SimpleNamespace(csr_ptr=torch.from_numpy(ptr), csr_idx=torch.from_numpy(idx),
                               csr_eid=torch.from_numpy(eid))
    assert SEED == TL.SEED
    n_id, want = TL._oracle_sums(dict(g=g, rg=rg, x=x), *sizes)
    x64 = {t: v.double().numpy() for t, v in x.items()}
    n_id2, got = R.oracle_sums(g, (ptr, idx, eid), x64, (128,) * 4, *sizes, SEED)
    assert n_id == n_id2
    assert np.array_equal(got["s_agg"].reshape(want["s_agg"].shape), want["s_agg"])
    for name in ("s_w", "u_self", "u_rel", "scnt", "inv"):
        assert np.array_equal(got[name], want[name]), name


def test_restatement_layouts_and_slot_formulas():
    """mixed widths: type t's sum sits at column sum_{u<t} K_u, the self row is zero past its own
    width; the slot formulas against a direct evaluation on one hand-made row."""
    g = hand_graph()
    csr = csr_by_target(g)
    widths = (64, 256, 128, 64)
    rng = np.random.default_rng(0)
    x64 = {t: rng.standard_normal((c, widths[t])) for t, c in enumerate(g["counts"])}
    n_id, ref = R.oracle_sums(g, csr, x64, widths, 3, 20, SEED)
    c = R.cols(widths)
    assert c.tolist() == [0, 64, 320, 448, 512] and ref["s_agg"].shape[1] == 512
    assert ref["u_self"].shape[1] == 256
    for i, t in enumerate(n_id):
        tt = int(g["ntype"][t])
        assert not ref["u_self"][i, widths[tt]:].any()
        assert np.array_equal(ref["u_self"][i, :widths[tt]], x64[tt][int(g["local"][t])])
        for q in range(4):
            if ref["s_w"][i, q] == 0:
                assert not ref["s_agg"][i, c[q]:c[q + 1]].any() and ref["u_rel"][i, q] == -1
    # one row: slot 1 (relation 2, two entries), self loop of type 3 (relation 7 + 3)
    U, cnt = rng.standard_normal((1, 512)), np.array([[0.0, 2.0, 0.0, 0.0]])
    xs = np.zeros((1, 256))
    xs[0, :64] = rng.standard_normal(64)
    ur = np.array([[-1, 2, -1, -1, 10]])
    tab = rng.standard_normal(11)
    S, w = R.slot_fwd(U, cnt, xs, ur, tab, 7, widths)
    assert np.allclose(S[0, 64:320], tab[2] * U[0, 64:320]) and not S[0, :64].any()
    assert np.allclose(S[0, 448:], tab[10] * xs[0, :64]) and not S[0, 320:448].any()
    assert np.allclose(w[0], [0, 2 * tab[2], 0, tab[10]])
    gS, gw = rng.standard_normal((1, 512)), rng.standard_normal((1, 4))
    d = R.slot_bwd(U, cnt, xs, ur, gS, gw, 7, widths, 11)
    want = np.zeros(11)
    want[2] = U[0, 64:320] @ gS[0, 64:320] + 2 * gw[0, 1]
    want[10] = xs[0, :64] @ gS[0, 448:] + gw[0, 3]
    assert np.allclose(d, want)
