"""CPU side of the fused GAT attention dropout (regnn_gat_fused_fwd_drop,
regnn_spmm_heads_bwd_drop): the two symbols are declared, bound and exported under ABI 51 and
refuse a NULL seed / a keep threshold above 2^16 before any launch; the masked fp64 restatement of
_attn_drop_ref.py is well conditioned on the GPU tests' inputs (an fp32 torch run of it stays at
a quarter of the kernels' bound); and the masks the GPU tests draw are fair inputs: a short row
fully dropped, a chunked row with kept and dropped entries in every head, the keep rate within
three sigmas. No GPU."""
import os
import re
import subprocess

import pytest
import torch

import _attention_ref as AR
import _attn_drop_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 320
NEW = ("regnn_gat_fused_fwd_drop", "regnn_spmm_heads_bwd_drop")


def test_symbols_declared_bound_exported():
    from regnn_hip import _lib
    src = open(os.path.join(ROOT, "include", "regnn_hip.h")).read()
    decl = set(re.findall(r"^\s*(?:int|int64_t)\s+(regnn_\w+)\s*\(", src, re.M))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB], capture_output=True,
                         text=True).stdout
    syms = set(re.findall(r"\bT (regnn_\w+)", out))
    for name in NEW:
        assert name in decl and name in _lib.EXPORTED and name in syms, name
    assert _lib.ABI_VERSION == 51 and _lib._so.regnn_abi_version() == 51


def test_drop_entries_refuse_bad_seed_and_threshold_without_gpu():
    """EINVAL (1) for a NULL seed and for keep16 = 65537, every other argument plausible; H = 3
    is REGNN_EUNSUPPORTED (2). All before any launch: no GPU is present here."""
    from regnn_hip import _lib
    A = [1 << 20, 1 << 21, 1 << 22, 1 << 23, 1 << 24, 1 << 25, 1 << 26, 1 << 27, 1 << 28]
    seed = 1 << 29
    fwd = _lib._so.regnn_gat_fused_fwd_drop

    def f(H, seed_, keep16):
        return fwd(*A, 10, H, 16, 0.2, 0, None, None, seed_, keep16, 2.0, None)
    assert f(8, None, 32768) == 1
    assert f(8, seed, 65537) == 1
    assert f(3, seed, 32768) == 2
    bwd = _lib._so.regnn_spmm_heads_bwd_drop

    def b(H, seed_, keep16):
        return bwd(*A[:8], 10, H, 16, 0, None, seed_, keep16, 2.0, None)
    assert b(8, None, 32768) == 1
    assert b(8, seed, 65537) == 1
    assert b(3, seed, 32768) == 2
    assert fwd(*A, 0, 8, 16, 0.2, 0, None, None, seed, 65536, 1.0, None) == 0     # no rows: OK
    assert bwd(*A[:8], 0, 8, 16, 0, None, seed, 65536, 1.0, None) == 0


def test_knob_and_fused_head_counts():
    """the layer's knob names one of its two paths; ops.gat_fused fuses powers of two <= 32"""
    from regnn_hip import ops
    assert ops.ATTN_DROP["mode"] in ("torch", "fused")
    assert [h for h in range(0, 70) if ops.gat_fused_ok(h)] == [1, 2, 4, 8, 16, 32]


def test_mask_is_the_oracle_mask_on_padded_heads():
    """the [E, Hq] indexing: H <= 4 reads the first columns of one 4-wide vector per edge, H = 8
    two vectors; 8-bit draws iff keep16 % 256 == 0; keep16 = 65536 keeps everything."""
    from oracle import regnn_oracle as O
    E = 1000
    m4 = DR.attn_mask(7, E, 4, 26214)
    for H in (1, 2):
        assert torch.equal(DR.attn_mask(7, E, H, 26214), m4[:, :H])
    assert torch.equal(DR.attn_mask(7, E, 8, 26214),
                       torch.from_numpy(O.dropout_mask(7, E, 8, 4, 26214)))
    assert DR.head_cols(1) == 4 and DR.head_cols(8) == 8 and DR.head_cols(32) == 32
    assert bool(DR.attn_mask(7, E, 32, 65536).all())
    assert DR.keep16_of(0.5) % 256 == 0 and DR.keep16_of(0.6) == 26214 and 26214 % 256


@pytest.fixture(scope="module")
def graph():
    rg, e_feat = AR.ladder_graph("default", "cpu", N)
    return rg, rg.rel_pack(e_feat, num_rel=AR.N_REL).rel_csr


@pytest.mark.parametrize("p", DR.PS)
@pytest.mark.parametrize("H,D", [(1, 64), (2, 32), (8, 8), (32, 4)])
@pytest.mark.parametrize("recipe", ["unit", "wide"])
def test_masked_restatement_conditioned(graph, recipe, H, D, p):
    """an fp32 torch run of the masked restatement against the fp64 one under the per-element
    metric: <= TOL_GUARD, a quarter of the kernels' bound. The inputs, not the kernels."""
    rg, rel = graph
    ft, el, er, tab, gy, slope = AR.gat_inputs(recipe, N, H, D, AR.N_REL, seed=H * 1000 + D)
    w = DR.drop_weight(DR.SEEDS[p], rg.E, H, p)
    want, scale = DR.gat_drop_case_ref(rg.csr_ptr, rg.csr_idx, rel, el, er, tab, ft, gy, slope, w)
    leaves = [t.detach().float().clone().requires_grad_(True) for t in (el, er, tab, ft)]
    out = DR.gat_drop_reference(rg.csr_ptr, rg.csr_idx, rel, *leaves, slope, w)
    out.backward(gy.float())
    got = {"out": out.detach()}
    got.update({k: t.grad for k, t in zip(["g_el", "g_er", "g_tab", "g_ft"], leaves)})
    for k in want:
        err = AR.rel_err(got[k], want[k], scale[k])
        assert err <= AR.TOL_GUARD, f"{k}: fp32 restatement err {err:.3e}"
        assert DR.exact_zeros(got[k], scale[k]), k
    assert bool((scale["out"] == 0).any())


@pytest.mark.parametrize("p", DR.PS)
@pytest.mark.parametrize("H", sorted({h for h, _ in DR.SHAPES}))
def test_gpu_masks_are_fair_inputs(graph, H, p):
    """a condition on the GPU tests' inputs, not a measurement: see fairness()"""
    rg, _ = graph
    mask = DR.attn_mask(DR.SEEDS[p], rg.E, H, DR.keep16_of(p))
    full, mixed, sigmas = DR.fairness(rg.csr_ptr, mask, p)
    assert full, "no row of degree >= 2 is fully dropped in any head"
    assert mixed, "no chunked row has kept and dropped entries in every head"
    assert sigmas <= 3.0, f"keep rate {sigmas:.2f} sigmas off"
