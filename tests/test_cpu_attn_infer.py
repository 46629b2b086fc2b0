"""The forward-only attention of the full-neighbour inference (regnn_mag_attn_fwd,
regnn_mag_attn_epilogue, regnn_hip.inference for 'regat' / 'regatv2') without a GPU:

* both symbols exist, the ABI number stays 51, and bad arguments / unsupported shapes are refused
  with the documented codes before any launch (fake non-NULL pointers do);
* the `deep` inputs are fair: on the ladder graph, with and without self loops, the fp64
  reference has at least 50 rows whose 1e-16 share of the softmax denominator lies in [1e-3, 1],
  dropping the term is an error of at least 100 x TOL_F32, and the fp32 torch run of the restatement stays within
  TOL_GUARD of the fp64 one under the attention metric;
* the identity the kernels rest on holds in fp64: the online form with the corrected denominator
  exp(s - m) / (S + eps exp(gmax - m)) equals the global-max softmax to 1e-12;
* ShardedInference still refuses self_loop_type 1 for the attention models.
"""
import pytest
import torch

import _attention_ref as R
import _attn_infer_ref as A

EINVAL, EUNSUPPORTED = 1, 2
GAT, GATV2 = 0, 1
SHAPES = [(1, 64), (4, 16), (8, 8)]


def _fwd(kind=GAT, H=8, D=64, **null):
    from regnn_hip import _lib
    f = 0x10000
    p = dict.fromkeys(("ptr", "idx", "rel", "tab", "el", "er", "att", "x", "xd", "acc", "rmax",
                       "rsum"), f)
    p.update(null)
    return _lib._so.regnn_mag_attn_fwd(p["ptr"], p["idx"], p["rel"], p["tab"], kind, p["el"],
                                       p["er"], p["att"], p["x"], p["xd"], p["acc"], p["rmax"],
                                       p["rsum"], 64, H, D, 0.2, None, None)


def _epi(H=8, D=64, flags=3, eps=1e-16, **null):
    from regnn_hip import _lib
    f = 0x10000
    p = dict.fromkeys(("acc", "rmax", "rsum", "gmax", "bias", "res", "lw", "lb", "y"), f)
    p.update(null)
    return _lib._so.regnn_mag_attn_epilogue(p["acc"], p["rmax"], p["rsum"], p["gmax"], eps,
                                            p["bias"], p["res"], p["lw"], p["lb"], 1e-5, flags,
                                            64, H, D, p["y"], None)


def test_symbols_declared_and_abi_number_unchanged():
    from regnn_hip import _lib, build
    assert _lib._so.regnn_abi_version() == _lib.ABI_VERSION == build.header_abi() == 51
    assert {"regnn_mag_attn_fwd", "regnn_mag_attn_epilogue"} <= set(_lib.EXPORTED)


def test_null_pointers_and_unknown_kinds_are_invalid_arguments():
    for name in ("ptr", "idx", "x", "acc", "rmax", "rsum"):
        assert _fwd(GAT, **{name: None}) == EINVAL, name
        assert _fwd(GATV2, **{name: None}) == EINVAL, name
    assert _fwd(GAT, rel=None) == EINVAL                       # a table without relation ids
    assert _fwd(GAT, er=None) == EINVAL
    assert _fwd(GAT, el=None, att=None) == EINVAL              # neither el nor attn_l
    assert _fwd(GATV2, att=None) == EINVAL
    assert _fwd(GATV2, xd=None) == EINVAL
    assert _fwd(2) == EINVAL and _fwd(-1) == EINVAL
    for name in ("acc", "rmax", "rsum", "gmax", "y"):
        assert _epi(**{name: None}) == EINVAL, name
    assert _epi(flags=4) == EINVAL
    assert _epi(eps=-1.0) == EINVAL


@pytest.mark.parametrize("H,D", [(0, 64), (8, 0), (8, 6), (33, 64), (1, 2052)])
def test_unsupported_shapes_are_refused_before_any_launch(H, D):
    """H * D beyond the lane layout's 2048 columns, D no multiple of 4"""
    assert _fwd(GAT, H=H, D=D) == EUNSUPPORTED
    assert _fwd(GAT, H=H, D=D, el=None) == EUNSUPPORTED
    assert _fwd(GATV2, H=H, D=D) == EUNSUPPORTED
    if D % 4 == 0:
        assert _epi(H=H, D=D) == EUNSUPPORTED


@pytest.mark.parametrize("D", [12, 24, 512])
def test_head_dots_need_a_power_of_two_vector_count(D):
    """D / 4 not a power of two (or above 64): the el-given kind alone takes it"""
    assert _fwd(GAT, H=2, D=D, el=None) == EUNSUPPORTED
    assert _fwd(GATV2, H=2, D=D) == EUNSUPPORTED
    from regnn_hip import ops
    assert not ops.mag_attn_fused_ok("gatv2", 2, D) and ops.mag_attn_fused_ok("gat", 2, D)


_CSR = {}


def _csr(loops):
    if loops not in _CSR:
        _CSR[loops] = tuple(torch.from_numpy(a) for a in A.ladder_csr(self_loops=loops))
    return _CSR[loops]


def _case(kind, recipe, H, D, loops):
    n_rel = A.N_REL_LOOPS if loops else R.N_REL
    return A.operator_inputs(kind, recipe, 320, H, D, n_rel, seed=300 + 7 * H + D)


@pytest.mark.parametrize("loops", [True, False])
@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("H,D", SHAPES)
def test_deep_inputs_make_the_eps_term_visible_and_stay_fair(kind, H, D, loops):
    ptr, idx, rel = _csr(loops)
    c = _case(kind, "deep", H, D, loops)
    want, scale, share = A.operator_reference(kind, c, ptr, idx, rel)
    rows = int(((share >= 1e-3) & (share <= 1.0)).any(1).sum())
    guard = R.rel_err(A.operator_reference(kind, c, ptr, idx, rel, torch.float32)[0], want, scale)
    dropped = R.rel_err(A.online_reference(kind, c, ptr, idx, rel, correct=False), want, scale)
    wide = A.operator_reference(kind, _case(kind, "wide", H, D, loops), ptr, idx, rel)[2]
    print(f"{kind} H={H} D={D} loops={loops}: {rows} rows with eps share >= 1e-3 (max "
          f"{float(share.max()):.3f}), fp32 restatement {guard:.2e}, eps dropped {dropped:.2e}, "
          f"wide's share {float(wide.max()):.1e}")
    assert rows >= 50
    assert guard <= R.TOL_GUARD
    # without the term a row's weights grow by share / (1 - share) >= share: with shares up to
    # ~1 the error is far above 100 x the kernels' bound (a one-entry row has |out| = scale)
    assert dropped >= 100 * R.TOL_F32
    assert float(wide.max()) <= 1e-6


@pytest.mark.parametrize("recipe", A.RECIPES)
@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("H,D", SHAPES)
def test_online_form_with_corrected_denominator_is_the_global_max_softmax(kind, recipe, H, D):
    ptr, idx, rel = _csr(True)
    c = _case(kind, recipe, H, D, True)
    want, scale, _ = A.operator_reference(kind, c, ptr, idx, rel)
    err = R.rel_err(A.online_reference(kind, c, ptr, idx, rel), want, scale)
    print(f"{kind} {recipe} H={H} D={D}: {err:.2e}")
    assert err <= 1e-12


@pytest.mark.parametrize("model", ["regat", "regatv2"])
def test_sharded_inference_refuses_other_self_loop_types(model):
    from regnn_hip import mag
    from regnn_hip.inference import ShardedInference
    m = mag.REGNN(16, 8, 5, 2, 10.0, 0.0, {k: 16 for k in range(4)}, 7, model=model, heads=2,
                  self_loop_type=1)
    with pytest.raises(NotImplementedError):
        ShardedInference(m, None, None, None, None)
