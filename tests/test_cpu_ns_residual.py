"""The fused NS step's residual mode, CPU side: the host gate (ns.fused_unsupported), the two
residual fixtures (tests/golden/make_golden_residual.py) against the CPU oracle, the cases the
schema fixture must contain, and the regnn_nsm_params layout / ABI number."""
import ctypes
import os
import re

import numpy as np
import pytest

import _golden as G
from oracle import regnn_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2e-6              # tests/test_oracle.py: fp64 results stored as fp32 -> ~1e-7 rounding
FIXTURES = ["nsres_regnn_schema", "nsres_regnn_ft3"]


def _check(tag, got, want, tol=TOL):
    ok, err = G.close(got, want, tol)
    assert ok, f"{tag}: rel err {err:.3e}"


def test_gate_accepts_two_layer_residual_only():
    import torch
    from regnn_hip import mag, ns

    def model(T, K, layers=2, classes=11, residual=True):
        return mag.REGNN(K, 64, classes, layers, 10.0, 0.0, {k: K for k in range(T)}, 7,
                         residual=residual, use_norm="ln", self_loop_type=2)

    def gate(m, T, K):
        return ns.fused_unsupported(m, {k: torch.zeros(3, K) for k in range(T)})

    assert gate(model(4, 128), 4, 128) is None
    assert gate(model(4, 128, classes=ns.TWO_LAYER_MAX_CLASSES), 4, 128) is None
    for why in (gate(model(4, 128, layers=3), 4, 128), gate(model(4, 128, layers=4), 4, 128),
                gate(model(4, 128, classes=400), 4, 128)):
        assert why is not None and "two-layer" in why
    mixed = model(4, 128)
    mixed.convs[1].residual = False
    why = gate(mixed, 4, 128)
    assert why is not None and "mixed" in why
    # without residual: three layers and 400 classes stay covered (the composed-map form)
    assert gate(model(4, 128, layers=3, residual=False), 4, 128) is None
    assert gate(model(4, 128, classes=400, residual=False), 4, 128) is None
    # the existing gate cases (tests/test_cpu_host.py) give what they gave
    assert gate(model(4, 128, residual=False), 4, 128) is None
    assert gate(model(8, 64, residual=False), 8, 64) is None
    assert gate(model(5, 128, residual=False), 5, 128) is not None
    assert gate(model(2, 96, residual=False), 2, 96) is not None


def _regnn_adjs(d):
    return [(d[f"adj{h}_src"], d[f"adj{h}_dst"], d[f"adj{h}_eid"],
             tuple(int(v) for v in d[f"adj{h}_size"])) for h in range(d["meta"]["num_layers"])]


@pytest.mark.parametrize("name", FIXTURES)
def test_residual_fixture_matches_oracle(name):
    """the oracle's REGNN composition with residual against the reference's own REGNN class
    (as tests/test_oracle.py::test_mag_regnn_model pins the mag_regnn_* fixtures)."""
    d = G.load(name)
    m = d["meta"]
    assert m["residual"] is True and m["use_norm"] == "ln" and m["self_loop_type"] == 2
    assert m["dropout"] == 0.0 and m["hidden"] == 64 and m["num_layers"] == 2
    P = G.sub(d, "p_")
    x_dict = {t: d[f"x{t}"].astype(np.float64) for t in range(4) if f"x{t}" in d}
    logp, loss, gr = O.mag_regnn_model(x_dict, d["ntype"], d["local"], d["n_id"], _regnn_adjs(d),
                                       d["edge_type"], P, d["y"][d["batch"]],
                                       feats_type=m["feats_type"],
                                       residual=m.get("residual", False))
    _check("logp", logp, d["logp"])
    _check("loss", np.asarray(loss), d["loss"])
    want = G.sub(d, "grad_")
    assert set(want) == set(gr), set(want) ^ set(gr)
    for k, v in want.items():
        _check(k, gr[k], v)


def test_fixture_names_stay_out_of_existing_globs():
    assert not [n for n in G.names("mag_regnn_") if "nsres" in n]
    assert set(FIXTURES) <= set(G.names("nsres_regnn_"))


def test_schema_fixture_structure():
    """the cases the residual kernels must meet, read from the fixture's innermost block (the
    batch's: adjs are stored outermost first, so adj1 is the fused step's hop 0); every target
    row gets one self loop on top of the stored edges."""
    d = G.load("nsres_regnn_schema")
    m = d["meta"]
    assert (m["in_channels"], m["classes"], m["sizes"], m["schema"]) == (128, 349, [25, 20], "ogbn-mag")
    assert m["y_global"] is True
    B = d["batch"].size
    s, t = d["adj1_src"], d["adj1_dst"]
    n_src, n_dst = (int(v) for v in d["adj1_size"])
    assert n_dst == B and d["n_id"][:B].tolist() == d["batch"].tolist()
    out_cnt = np.bincount(s[s < B], minlength=B) + 1      # transposed entries, self loop included
    in_cnt = np.bincount(t, minlength=B) + 1
    assert (out_cnt > 16).any()                           # (a) a hub row of the transposed index
    assert (out_cnt == 1).any()                           # (b) only its own self loop
    assert (in_cnt == 1).any() and (in_cnt == 26).any()   # (c) self loop only; fan-out + self
    assert in_cnt.max() == 26
    layer0_targets = d["n_id"][:n_src]                    # hop 0's sources = layer 0's rows
    assert np.unique(d["ntype"][layer0_targets]).size >= 3          # (d)
    # one relation per (source type, target type) pair: the relation-slot mode applies
    pair = d["ntype"][d["src"]] * 4 + d["ntype"][d["dst"]]
    for p in np.unique(pair):
        assert np.unique(d["edge_type"][pair == p]).size == 1
    assert os.path.getsize(os.path.join(G.GOLDEN, "nsres_regnn_schema.npz")) < 1536 * 1024


def test_ft3_fixture_takes_the_edge_pass():
    d = G.load("nsres_regnn_ft3")
    m = d["meta"]
    assert (m["in_channels"], m["classes"], m["sizes"]) == (64, 5, [4, 3])
    pair = d["ntype"][d["src"]] * 4 + d["ntype"][d["dst"]]
    assert any(np.unique(d["edge_type"][pair == p]).size > 1 for p in np.unique(pair))


def test_params_struct_and_abi():
    """`residual` is the last member of regnn_nsm_params, an int32 right after two_layer, in the
    header and in the ctypes mirror; the ABI number moved in the header, the library and _lib."""
    from regnn_hip import _lib, build, ns
    fields = ns._NsmParams._fields_
    assert fields[-1] == ("residual", ctypes.c_int32)
    assert fields[-2][0] == "two_layer"
    off = ns._NsmParams.residual.offset
    assert off == ns._NsmParams.two_layer.offset + 4
    # one int32 more than the struct that ended with two_layer (up to the pointer alignment)
    assert ctypes.sizeof(ns._NsmParams) == (off + 4 + 7) // 8 * 8
    src = open(os.path.join(ROOT, "include", "regnn_hip.h")).read()
    body = re.search(r"typedef struct regnn_nsm_params \{(.*?)\} regnn_nsm_params;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [s.strip() for s in body.split(";") if s.strip()]
    assert members[-1] == "int32_t residual" and members[-2] == "int32_t two_layer"
    assert _lib._so.regnn_abi_version() == _lib.ABI_VERSION == build.header_abi()
    assert _lib.ABI_VERSION >= 49


def test_composed_map_form_refuses_residual():
    """regnn_nsm_slab_floats / regnn_nsm_step with residual outside the two-layer form: refused
    before anything is launched (no GPU needed: REGNN_EUNSUPPORTED = 2)."""
    from regnn_hip import _lib, ns
    P = ns._NsmParams()
    P.n_types, P.k_in, P.n_layers, P.n_classes = 4, 128, 3, 11
    P.p_drop = 0.0
    for l in range(3):
        P.n_rel[l] = 11
    P.n_edge_types, P.residual, P.two_layer = 7, 1, 0
    W = ns._NsmWork()
    slab = _lib._so.regnn_nsm_slab_floats
    assert slab(ctypes.addressof(P), 64) == -2
    assert _lib._so.regnn_nsm_step(ctypes.addressof(P), ctypes.addressof(W), None) == 2
    P.n_layers, P.two_layer = 2, 0                 # two layers, but the composed-map form
    assert slab(ctypes.addressof(P), 64) == -2
    assert _lib._so.regnn_nsm_step(ctypes.addressof(P), ctypes.addressof(W), None) == 2
    P.two_layer = 1
    assert slab(ctypes.addressof(P), 64) > 0
    P.residual, P.two_layer, P.n_layers = 0, 0, 3
    assert slab(ctypes.addressof(P), 64) > 0
