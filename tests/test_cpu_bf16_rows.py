"""bf16 input tables on the model side (ops.BF16_ROWS) without a GPU: the four `_dt` entries exist
under the unchanged ABI number, each of their refusals comes back before any launch for both
storage types (null stream, fake non-NULL pointers, as tests/test_cpu_type_widths.py), the knob
defaults to off, and the shape / dtype predicate takes bf16 tables with the knob on only (on meta
tensors; the device half runs in tests/test_gpu_bf16_rows.py)."""
import ctypes

import pytest
import torch

EINVAL, EUNSUPPORTED = 1, 2
F32, BF16 = 0, 1
F = 0x10000                                  # a fake, 16-byte aligned, non-NULL pointer
NEW = ("regnn_typed_linear_fwd_dt", "regnn_typed_linear_wgrad_dt", "regnn_ns_typed_agg_dt",
       "regnn_ns_typed_agg_dt_bwd")
BOTH = pytest.mark.parametrize("dtype", [F32, BF16])


def _i32(vals):
    return (ctypes.c_int32 * len(vals))(*vals)


def _ptrs(vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def _agg(dtype, widths=(256, 128, 128, 128), meta=True, tables=None, ld_s=None, S=F, T=None,
         K_t=True, bwd=False, n_rel=11, no_tables=False, **null):
    """regnn_ns_typed_agg_dt (or _dt_bwd) over fake pointers; meta: the e_type / e_off hop form."""
    from regnn_hip import _lib
    T = len(widths) if T is None else T
    p = dict.fromkeys(("ptr", "rel", "tab", "w", "slab"), F)
    hop = dict(idx=None, n_id=None, ntype=None, local=None, e_type=F, e_off=F) if meta else \
        dict(idx=F, n_id=F, ntype=F, local=F, e_type=None, e_off=None)
    p.update(hop)
    p.update(null)
    tabs = None if no_tables else _ptrs([F] * len(widths) if tables is None else tables)
    kt = _i32(widths) if K_t else None
    ld = sum(widths) + 4 if ld_s is None else ld_s
    if bwd:
        return _lib._so.regnn_ns_typed_agg_dt_bwd(
            p["ptr"], p["idx"], p["rel"], p["n_id"], p["ntype"], p["local"], p["e_type"],
            p["e_off"], tabs, dtype, T, kt, 64, S, p["w"], ld, ld, p["slab"], n_rel, 16, None)
    return _lib._so.regnn_ns_typed_agg_dt(
        p["ptr"], p["idx"], p["rel"], p["tab"], p["n_id"], p["ntype"], p["local"], p["e_type"],
        p["e_off"], tabs, dtype, T, kt, 64, S, p["w"], ld, ld, None)


def _lin(dtype, widths=(256, 128, 128, 128), O=64, wgroup=None, G=None, wgrad=False, tab=None,
         T=None, K_t=True, Y=F, no_tables=False):
    from regnn_hip import _lib
    n = len(widths)
    T = n if T is None else T
    tabs = None if no_tables else _ptrs([F] * n if tab is None else tab)
    kt = _i32(widths) if K_t else None
    if wgrad:
        wg = list(range(n)) if wgroup is None else wgroup
        G = max(wg) + 1 if G is None else G
        return _lib._so.regnn_typed_linear_wgrad_dt(F, F, F, 100, T, tabs, dtype, _i32(wg), G, kt,
                                                    O, Y, F, _ptrs([F] * n), _ptrs([F] * n), None)
    return _lib._so.regnn_typed_linear_fwd_dt(F, F, F, 100, T, tabs, dtype, _ptrs([F] * n),
                                              _ptrs([F] * n), kt, O, Y, None)


def test_dt_symbols_under_the_unchanged_abi_number():
    from regnn_hip import _lib, build
    assert _lib._so.regnn_abi_version() == _lib.ABI_VERSION == build.header_abi() == 51
    assert set(NEW) <= set(_lib.EXPORTED)
    for name in NEW:
        assert hasattr(_lib._so, name), name


@pytest.mark.parametrize("bwd", [False, True])
def test_typed_agg_dt_refuses_a_dtype_other_than_the_two(bwd):
    for bad in (2, -1):
        assert _agg(bad, bwd=bwd) == EINVAL, bad


@BOTH
@pytest.mark.parametrize("bwd", [False, True])
def test_typed_agg_dt_refusals_before_any_launch(dtype, bwd):
    for bad in (96, 512, 0):
        assert _agg(dtype, widths=(256, bad, 128, 128), bwd=bwd) == EUNSUPPORTED, bad
    for T in (0, 9):
        assert _agg(dtype, T=T, bwd=bwd) == EINVAL, T
    assert _agg(dtype, K_t=False, bwd=bwd) == EINVAL
    assert _agg(dtype, no_tables=True, bwd=bwd) == EINVAL
    assert _agg(dtype, tables=[F, F, None, F], bwd=bwd) == EINVAL      # a null table
    assert _agg(dtype, tables=[F, F + 8, F, F], bwd=bwd) == EINVAL     # a misaligned table
    # ... and everything the _kt entry refuses
    assert _agg(dtype, S=F + 4, bwd=bwd) == EINVAL                     # misaligned S / gS
    assert _agg(dtype, ld_s=256 + 3 * 128 - 4, bwd=bwd) == EINVAL      # ld_s < sum K_t
    assert _agg(dtype, ld_s=256 + 3 * 128 + 2, bwd=bwd) == EINVAL      # not a multiple of 4
    for meta in (True, False):
        names = ("e_type", "e_off") if meta else ("idx", "n_id", "ntype", "local")
        for name in names:
            assert _agg(dtype, meta=meta, bwd=bwd, **{name: None}) == EINVAL, name
    for name in ("ptr", "rel", "w"):
        assert _agg(dtype, bwd=bwd, **{name: None}) == EINVAL, name
    if bwd:
        assert _agg(dtype, bwd=True, n_rel=257) == EINVAL
        assert _agg(dtype, bwd=True, slab=None) == EINVAL
    else:
        assert _agg(dtype, tab=None) == EINVAL


@pytest.mark.parametrize("wgrad", [False, True])
def test_typed_linear_dt_refuses_a_dtype_other_than_the_two(wgrad):
    for bad in (2, -1):
        assert _lin(bad, wgrad=wgrad) == EINVAL, bad


@BOTH
@pytest.mark.parametrize("wgrad", [False, True])
def test_typed_linear_dt_refusals_before_any_launch(dtype, wgrad):
    for bad in (96, 512, 0):
        assert _lin(dtype, widths=(64, bad, 128), wgrad=wgrad) == EUNSUPPORTED, bad
    for T in (0, 9):
        assert _lin(dtype, T=T, wgrad=wgrad) == EINVAL, T
    assert _lin(dtype, K_t=False, wgrad=wgrad) == EINVAL
    assert _lin(dtype, no_tables=True, wgrad=wgrad) == EINVAL
    assert _lin(dtype, tab=[F, None, F, F], wgrad=wgrad) == EINVAL     # a null table
    assert _lin(dtype, tab=[F, F + 8, F, F], wgrad=wgrad) == EINVAL    # a misaligned table
    assert _lin(dtype, Y=F + 4, wgrad=wgrad) == EINVAL                 # misaligned Y / gY
    assert _lin(dtype, O=72, wgrad=wgrad) == EUNSUPPORTED
    if wgrad:
        assert _lin(dtype, O=80, wgrad=True) == EUNSUPPORTED           # wgrad: O % 64
        # a weight group may only join types of one width
        assert _lin(dtype, wgroup=[0, 1, 1, 0], wgrad=True) == EINVAL
        assert _lin(dtype, wgroup=[0, 1, 1, 2], G=4, wgrad=True) == EINVAL   # no type in a group


def test_knob_defaults_to_off_and_checks_its_value(monkeypatch):
    import os
    from regnn_hip import ops
    if "REGNN_BF16_ROWS" not in os.environ:
        assert ops.BF16_ROWS["mode"] == "off"
    assert ops.BF16_ROWS["mode"] == os.environ.get("REGNN_BF16_ROWS", "off")
    monkeypatch.setitem(ops.BF16_ROWS, "mode", "yes")
    with pytest.raises(ValueError, match="BF16_ROWS"):
        ops.bf16_rows_on()


def _meta(widths, dtype=torch.bfloat16):
    return [torch.empty(10, k, dtype=dtype, device="meta") for k in widths]


SHAPES_OK = ((256, 128, 128, 128), (64,), (128,) * 8)
SHAPES_BAD = ((128,) * 9, (128, 96))


def test_layout_predicate_knob_off_refuses_bf16_rows(monkeypatch):
    from regnn_hip import ops
    monkeypatch.setitem(ops.BF16_ROWS, "mode", "off")
    for widths in SHAPES_OK + SHAPES_BAD:
        assert not ops.typed_agg_layout_ok(_meta(widths)), widths
        assert not ops.typed_agg_layout_ok(_meta(widths), pre_sums=False), widths


def test_layout_predicate_knob_on_takes_bf16_rows(monkeypatch):
    from regnn_hip import ops
    monkeypatch.setitem(ops.BF16_ROWS, "mode", "on")
    for widths in SHAPES_OK:
        assert ops.typed_agg_layout_ok(_meta(widths)), widths
    for widths in SHAPES_BAD:
        assert not ops.typed_agg_layout_ok(_meta(widths)), widths
    # one fp32 table among bf16 ones, either way round
    assert not ops.typed_agg_layout_ok(_meta((128, 128)) + _meta((128,), torch.float32))
    assert not ops.typed_agg_layout_ok(_meta((128,), torch.float32) + _meta((128, 128)))
    # fp32 tables: as ever
    assert ops.typed_agg_layout_ok(_meta((256, 128, 64), torch.float32))
    # the operand contract also asks for device tables
    assert not ops.ns_typed_agg_ok([torch.zeros(4, 128).bfloat16()])


def test_pre_sums_answers_do_not_depend_on_the_knob(monkeypatch):
    from regnn_hip import ops
    cases = [_meta(w) for w in SHAPES_OK + SHAPES_BAD + ((128,) * 4, (128, 64), (128,) * 5)]
    cases += [_meta((128,) * 4, torch.float32), _meta((256, 128), torch.float32),
              _meta((128,)) + _meta((128,), torch.float32)]
    answers = {}
    for mode in ("off", "on"):
        monkeypatch.setitem(ops.BF16_ROWS, "mode", mode)
        answers[mode] = [ops.typed_agg_layout_ok(t, pre_sums=True) for t in cases]
    assert answers["off"] == answers["on"]
    assert answers["off"][5] and not answers["off"][7]     # (128,) * 4 yes, five tables no
