"""bf16 input feature tables in the NS sampler's sums launch, CPU side: the host gate
(ns.fused_unsupported), the new C entry (regnn_ns_hop_typed_sums_dt: a symbol added under ABI 50)
and its refusals, all returned before any launch (no GPU needed)."""
import ctypes

EINVAL, EUNSUPPORTED = 1, 2
F32, BF16 = 0, 1


def _model(T, K, residual=False):
    from regnn_hip import mag
    return mag.REGNN(K, 64, 11, 2, 10.0, 0.0, {k: K for k in range(T)}, 7, residual=residual,
                     use_norm="ln", self_loop_type=2)


def _gate(T, K, dtypes, residual=False):
    import torch
    from regnn_hip import ns
    x = {k: torch.zeros(3, K, dtype=dtypes[k % len(dtypes)]) for k in range(T)}
    return ns.fused_unsupported(_model(T, K, residual), x)


def test_gate_accepts_bf16_tables_at_the_sums_launch_shapes():
    import torch
    bf, f32 = torch.bfloat16, torch.float32
    assert _gate(4, 128, [bf]) is None
    assert _gate(4, 128, [bf], residual=True) is None
    why = _gate(4, 128, [f32, bf])
    assert why is not None and "one dtype" in why
    for why in (_gate(4, 64, [bf]), _gate(5, 128, [bf]), _gate(8, 64, [bf])):
        assert why is not None and "bf16" in why
    assert _gate(4, 128, [torch.float16]) is not None


def test_fp32_gate_cases_give_what_they_gave():
    """the cases of tests/test_cpu_host.py and tests/test_cpu_ns_residual.py"""
    import torch
    f32 = [torch.float32]
    assert _gate(4, 128, f32) is None
    assert _gate(8, 64, f32) is None
    assert _gate(5, 128, f32) is not None
    assert _gate(2, 96, f32) is not None
    assert _gate(4, 128, f32, residual=True) is None


def test_symbol_and_abi():
    from regnn_hip import _lib, build
    assert hasattr(_lib._so, "regnn_ns_hop_typed_sums_dt")
    assert "regnn_ns_hop_typed_sums_dt" in _lib.EXPORTED
    args, ret = _lib._SIG["regnn_ns_hop_typed_sums_dt"]
    old, _ = _lib._SIG["regnn_ns_hop_typed_sums"]
    # the fp32 entry's parameters in its order, with dtype right after tables (position 17)
    assert args == old[:18] + [ctypes.c_int32] + old[18:] and ret is ctypes.c_int
    assert _lib._so.regnn_abi_version() == _lib.ABI_VERSION == build.header_abi() == 51
    assert (_lib.F32_CODE, _lib.BF16_CODE) == (F32, BF16)


def _sums_call(dtype, table=0x10000, K=128, k=5, T=4):
    """regnn_ns_hop_typed_sums_dt with valid-looking arguments (never dereferenced on the host
    except the table array), no index job, no type layout"""
    from regnn_hip import _lib
    fake = 0x10000
    tabs = (ctypes.c_void_p * 4)(fake, fake, table, fake)
    return _lib._so.regnn_ns_hop_typed_sums_dt(
        fake, fake, fake, fake, 7, k, 1, fake, fake, fake, 64, fake, fake, fake, fake, fake,
        fake, tabs, dtype, T, K, fake, fake, fake, fake, None, None, None)


def test_dt_entry_refusals_come_before_any_launch():
    assert _sums_call(2) == EINVAL                          # no such dtype
    assert _sums_call(-1) == EINVAL
    for dt in (F32, BF16):
        assert _sums_call(dt, table=0x10008) == EINVAL      # a table base off the 16-byte grid
        assert _sums_call(dt, table=None) == EINVAL         # a NULL table
        assert _sums_call(dt, K=64) == EUNSUPPORTED
        assert _sums_call(dt, k=64) == EUNSUPPORTED
        assert _sums_call(dt, k=0) == EUNSUPPORTED
        assert _sums_call(dt, T=5) == EUNSUPPORTED
