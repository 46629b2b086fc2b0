"""One input width per node type (feats_type 5: paper rows 256 wide, the others 128) without a
GPU: the four `_kt` entries exist under the unchanged ABI number, each of their refusals comes
back before any launch (null stream, fake non-NULL pointers, as tests/test_cpu_ns_gat.py), and the
host predicates take the widths they should. ops.ns_typed_agg_ok itself also asks for device
tables; its shape / dtype half, ops.typed_agg_layout_ok, is what runs here (on meta tensors), the
device half in tests/test_gpu_type_widths.py."""
import ctypes

import pytest
import torch

EINVAL, EUNSUPPORTED = 1, 2
F = 0x10000                                  # a fake, 16-byte aligned, non-NULL pointer
NEW = ("regnn_ns_typed_agg_kt", "regnn_ns_typed_agg_kt_bwd", "regnn_typed_linear_fwd_kt",
       "regnn_typed_linear_wgrad_kt")


def _i32(vals):
    return (ctypes.c_int32 * len(vals))(*vals)


def _ptrs(vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def _agg(widths=(256, 128, 128, 128), meta=True, tables=None, ld_s=None, S=F, T=None, K_t=True,
         bwd=False, n_rel=11, **null):
    """regnn_ns_typed_agg_kt (or _bwd) over fake pointers; meta: the e_type / e_off hop form."""
    from regnn_hip import _lib
    T = len(widths) if T is None else T
    p = dict.fromkeys(("ptr", "rel", "tab", "w", "slab"), F)
    hop = dict(idx=None, n_id=None, ntype=None, local=None, e_type=F, e_off=F) if meta else \
        dict(idx=F, n_id=F, ntype=F, local=F, e_type=None, e_off=None)
    p.update(hop)
    p.update(null)
    tabs = _ptrs([F] * len(widths) if tables is None else tables)
    kt = _i32(widths) if K_t else None
    ld = sum(widths) + 4 if ld_s is None else ld_s
    if bwd:
        return _lib._so.regnn_ns_typed_agg_kt_bwd(
            p["ptr"], p["idx"], p["rel"], p["n_id"], p["ntype"], p["local"], p["e_type"],
            p["e_off"], tabs, T, kt, 64, S, p["w"], ld, ld, p["slab"], n_rel, 16, None)
    return _lib._so.regnn_ns_typed_agg_kt(
        p["ptr"], p["idx"], p["rel"], p["tab"], p["n_id"], p["ntype"], p["local"], p["e_type"],
        p["e_off"], tabs, T, kt, 64, S, p["w"], ld, ld, None)


def _lin(widths=(256, 128, 128, 128), O=64, wgroup=None, G=None, wgrad=False, tab=None, T=None,
         K_t=True, Y=F):
    from regnn_hip import _lib
    n = len(widths)
    T = n if T is None else T
    tabs = _ptrs([F] * n if tab is None else tab)
    kt = _i32(widths) if K_t else None
    if wgrad:
        wg = list(range(n)) if wgroup is None else wgroup
        G = max(wg) + 1 if G is None else G
        return _lib._so.regnn_typed_linear_wgrad_kt(F, F, F, 100, T, tabs, _i32(wg), G, kt, O, Y,
                                                    F, _ptrs([F] * n), _ptrs([F] * n), None)
    return _lib._so.regnn_typed_linear_fwd_kt(F, F, F, 100, T, tabs, _ptrs([F] * n),
                                              _ptrs([F] * n), kt, O, Y, None)


def test_new_symbols_under_the_unchanged_abi_number():
    from regnn_hip import _lib, build
    assert _lib._so.regnn_abi_version() == _lib.ABI_VERSION == build.header_abi() == 51
    assert set(NEW) <= set(_lib.EXPORTED)
    for name in NEW:
        assert hasattr(_lib._so, name), name


@pytest.mark.parametrize("bwd", [False, True])
def test_typed_agg_kt_refusals_before_any_launch(bwd):
    for bad in (96, 512, 0, 32):
        assert _agg(widths=(256, bad, 128, 128), bwd=bwd) == EUNSUPPORTED, bad
    for T in (0, 9, -1):
        assert _agg(T=T, bwd=bwd) == EINVAL, T
    assert _agg(K_t=False, bwd=bwd) == EINVAL
    assert _agg(tables=[F, F, None, F], bwd=bwd) == EINVAL             # a null table
    assert _agg(tables=[F, F + 4, F, F], bwd=bwd) == EINVAL            # a misaligned table
    assert _agg(S=F + 4, bwd=bwd) == EINVAL                            # misaligned S / gS
    assert _agg(ld_s=256 + 3 * 128 - 4, bwd=bwd) == EINVAL             # ld_s < sum K_t
    assert _agg(ld_s=256 + 3 * 128 + 2, bwd=bwd) == EINVAL             # not a multiple of 4
    for meta in (True, False):                                         # either hop form, whole
        names = ("e_type", "e_off") if meta else ("idx", "n_id", "ntype", "local")
        for name in names:
            assert _agg(meta=meta, bwd=bwd, **{name: None}) == EINVAL, name
    for name in ("ptr", "rel", "w"):
        assert _agg(bwd=bwd, **{name: None}) == EINVAL, name
    if bwd:
        assert _agg(bwd=True, n_rel=257) == EINVAL
        assert _agg(bwd=True, slab=None) == EINVAL
    else:
        assert _agg(tab=None) == EINVAL


@pytest.mark.parametrize("wgrad", [False, True])
def test_typed_linear_kt_refusals_before_any_launch(wgrad):
    for bad in (96, 512, 0):
        assert _lin(widths=(64, bad, 128), wgrad=wgrad) == EUNSUPPORTED, bad
    for T in (0, 9):
        assert _lin(T=T, wgrad=wgrad) == EINVAL, T
    assert _lin(K_t=False, wgrad=wgrad) == EINVAL
    assert _lin(tab=[F, F + 8, F, F], wgrad=wgrad) == EINVAL
    assert _lin(Y=F + 4, wgrad=wgrad) == EINVAL
    assert _lin(O=72, wgrad=wgrad) == EUNSUPPORTED
    if wgrad:
        assert _lin(O=80, wgrad=True) == EUNSUPPORTED                  # wgrad: O % 64
        # a weight group may only join types of one width
        assert _lin(wgroup=[0, 1, 1, 0], wgrad=True) == EINVAL
        assert _lin(wgroup=[0, 1, 1, 2], G=4, wgrad=True) == EINVAL    # a group without a type


def _meta(widths, dtype=torch.float32):
    return [torch.empty(10, k, dtype=dtype, device="meta") for k in widths]


def test_typed_agg_layout_takes_mixed_fp32_widths_only():
    from regnn_hip import ops
    for widths in ((256, 128, 128, 128), (64, 256, 128), (128, 64), (128, 128), (256, 256)):
        assert ops.typed_agg_layout_ok(_meta(widths)), widths
        assert ops.typed_agg_layout_ok(_meta(widths), pre_sums=True), widths
    for widths in ((256, 96, 128, 128), (512, 128), (96,), (128, 512, 64)):
        assert not ops.typed_agg_layout_ok(_meta(widths)), widths
    # bf16: equal width 128 through the sums launch only
    bf = torch.bfloat16
    assert ops.typed_agg_layout_ok(_meta((128,) * 4, bf), pre_sums=True)
    assert not ops.typed_agg_layout_ok(_meta((128,) * 4, bf))
    assert not ops.typed_agg_layout_ok(_meta((256, 128, 128, 128), bf), pre_sums=True)
    assert not ops.typed_agg_layout_ok(_meta((128, 64), bf), pre_sums=True)
    # mixed dtypes
    mixed = _meta((256,)) + _meta((128,), bf)
    assert not ops.typed_agg_layout_ok(mixed) and not ops.typed_agg_layout_ok(mixed, True)
    assert not ops.typed_agg_layout_ok(_meta((128,), bf) + _meta((128,)), pre_sums=True)
    assert not ops.typed_agg_layout_ok([]) and not ops.typed_agg_layout_ok(_meta((128,) * 9))
    # the operand contract also asks for device tables
    assert not ops.ns_typed_agg_ok([torch.zeros(4, k) for k in (256, 128)])


def test_mixed_widths_still_refused_by_the_fused_step():
    from regnn_hip import mag, ns
    dims = {0: 256, 1: 128, 2: 128, 3: 128}
    m = mag.REGNN(128, 64, 13, 2, 10.0, 0.0, dims, 7, use_norm="ln", self_loop_type=2)
    x = {k: torch.zeros(4, d) for k, d in dims.items()}
    assert "equal" in ns.fused_unsupported(m, x)
    same = {k: torch.zeros(4, 128) for k in dims}
    m = mag.REGNN(128, 64, 13, 2, 10.0, 0.0, {k: 128 for k in dims}, 7, use_norm="ln",
                  self_loop_type=2)
    assert ns.fused_unsupported(m, same) is None


def test_csc_sort_symbol_and_refusals():
    """regnn_ns_csc_sort (the canonical order of hop 0's transposed index, what makes the module
    path's step reproducible bit for bit): declared, and its refusals come before any launch."""
    from regnn_hip import _lib
    f = _lib._so.regnn_ns_csc_sort
    assert "regnn_ns_csc_sort" in _lib.EXPORTED
    assert f(None, 1, F, F, F + 64, 8, 8, None) == EINVAL
    assert f(F, 1, None, F, F + 64, 8, 8, None) == EINVAL
    assert f(F, 1, F, None, F + 64, 8, 8, None) == EINVAL
    assert f(F, 1, F, F, None, 8, 8, None) == EINVAL
    assert f(F, 1, F, F + 64, F + 64, 8, 8, None) == EINVAL          # in place
    assert f(F, -1, F, F, F + 64, 8, 8, None) == EINVAL
    assert f(F, 1, F, F, F + 64, -1, 8, None) == EINVAL
    assert f(F, 1, F, F, F + 64, 0, 8, None) == 0                    # nothing to sort
