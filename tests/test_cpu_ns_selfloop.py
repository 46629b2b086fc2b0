"""CPU checks of the self_loop_type 1 / 3 fixtures and host-side rules (no GPU):

* the nssl_regnn_* and mag_noloop_*conv_sl3 fixtures (tests/golden/make_golden_selfloop.py) load
  and their meta is consistent: relation_weight of 7 (type 3) / 11 (type 1) entries, finite loss
  and gradients, for type 3 a live target without a sampled in-edge in every block;
* mag.add_self_loop_relations reproduces the type-1 graph stored in the fixture from its
  7-relation graph;
* the convs refuse a block of the other form before any launch, both directions;
* gat_blocks_unsupported covers the three models at types 1 / 3 with mag.NOLOOP_BLOCKS on and
  refuses bf16 tables there; with the knob off (the default) it and ShardedInference refuse
  types 1 / 3 as before.

oracle/cpu_ns.py restates self_loop_type 2 only (it takes no self_loop_type), so the exact-size
restatement is not compared with these fixtures here; tests/test_gpu_ns_selfloop.py compares the
exact-size path on the GPU.
"""
import numpy as np
import pytest
import torch

import _golden as G

KINDS = ["regcn", "regat", "regatv2"]


@pytest.mark.parametrize("slt", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_regnn_fixture_meta_is_consistent(kind, slt):
    d = G.load(f"nssl_regnn_{kind}_sl{slt}")
    m = d["meta"]
    n_et = 11 if slt == 1 else 7
    assert m["self_loop_type"] == slt and m["kind"] == kind and m["num_edge_types"] == n_et
    assert m["sizes"] == [5, 3] and len(d["batch"]) == 32 and int(sum(m["counts"])) == 354
    assert m["hidden"] * m["heads"] == 64 and m["in_channels"] == 64 and m["residual"] is True
    P, Gr = G.sub(d, "p_"), G.sub(d, "grad_")
    for i in range(m["num_layers"]):
        assert P[f"convs.{i}.relation_weight"].shape[0] == n_et
    assert np.isfinite(d["loss"]) and all(np.isfinite(v).all() for v in Gr.values())
    assert set(Gr) <= set(P) and any(np.abs(v).max() > 0 for v in Gr.values())
    assert int(d["edge_type"].max()) == n_et - 1
    assert np.all(np.diff(d["dst"]) >= 0)                # dst-major: edge ids are CSR positions
    L_ = m["num_layers"]
    for h in range(L_):
        n_src, n_dst = (int(v) for v in d[f"adj{h}_size"])
        assert n_dst == m["live"][h] and d[f"adj{h}_src"].max() < n_src
        cnt = np.bincount(d[f"adj{h}_dst"], minlength=n_dst)
        assert cnt.max() <= m["sizes"][L_ - 1 - h]
        if slt == 3:                                     # the empty-row assertion
            empty = np.nonzero(cnt == 0)[0]
            assert empty.size >= 1 and np.array_equal(empty, d[f"empty{h}"])
        else:                                            # every node has its loop edge to sample
            assert cnt.min() >= 1
    assert m["live"][-1] == 32


@pytest.mark.parametrize("kind", KINDS)
def test_add_self_loop_relations_reproduces_the_type1_graph(kind):
    from regnn_hip import mag
    d = G.load(f"nssl_regnn_{kind}_sl1")
    ei = torch.from_numpy(np.stack([d["base_src"], d["base_dst"]]))
    ei2, et2, n_et = mag.add_self_loop_relations(ei, torch.from_numpy(d["base_edge_type"]),
                                                 torch.from_numpy(d["ntype"]), 7)
    assert n_et == 11 == d["meta"]["num_edge_types"]
    N = d["ntype"].size
    assert ei2.shape[1] == ei.shape[1] + N and torch.equal(ei2[:, :ei.shape[1]], ei)
    o = np.argsort(ei2[1].numpy(), kind="stable")        # the fixture's dst-major edge order
    assert np.array_equal(ei2[0].numpy()[o], d["src"])
    assert np.array_equal(ei2[1].numpy()[o], d["dst"])
    assert np.array_equal(et2.numpy()[o], d["edge_type"])
    # the reference's order (author, field_of_study, institution, paper) under another numbering
    # of the node types: paper = 0, author = 1, institution = 2, field_of_study = 3
    nt = torch.tensor([0, 1, 2, 3, 3])
    _, et3, n3 = mag.add_self_loop_relations(torch.zeros(2, 0, dtype=torch.int64),
                                             torch.zeros(0, dtype=torch.int64), nt, 7,
                                             rel_of_type=[3, 0, 2, 1])
    assert n3 == 11 and et3.tolist() == [10, 7, 9, 8, 8]


@pytest.mark.parametrize("kind", KINDS)
def test_conv_fixture_meta_is_consistent(kind):
    d = G.load(f"mag_noloop_{kind}conv_sl3")
    m = d["meta"]
    assert m["self_loop_type"] == 3 and m["heads"] * m["out_channels"] == 64
    assert G.sub(d, "p_")["relation_weight"].shape[0] == m["num_edge_types"] == 7
    cnt = np.bincount(d["dst"], minlength=m["n_dst"])
    assert np.array_equal(np.nonzero(cnt == 0)[0], d["empty"]) and d["empty"].size >= 3
    assert np.isfinite(d["out"]).all() and np.isfinite(d["grad_x"]).all()


class _FakeBlock:
    is_ns_block = True

    def __init__(self, self_loops):
        self.self_loops = self_loops
        self.n_dst = 4


@pytest.mark.parametrize("kind", KINDS)
def test_convs_refuse_the_other_block_form_before_any_launch(kind, monkeypatch):
    from regnn_hip import mag
    monkeypatch.setitem(mag.GATV2_BLOCKS, "mode", "on")
    x = torch.zeros(6, 8)

    def conv(slt):
        if kind == "regcn":
            return mag.REGCNConv(8, 8, 4, 7, self_loop_type=slt)
        cls = mag.REGATv2Conv if kind == "regatv2" else mag.REGATConv
        return cls(8, 4, 4, 7, heads=2, self_loop_type=slt)

    with pytest.raises(ValueError, match="self_loop_type 2.*self_loops=False"):
        conv(2)((x, x[:4]), _FakeBlock(False))
    for slt in (1, 3):
        with pytest.raises(ValueError, match=f"self_loop_type {slt}.*self_loops=True"):
            conv(slt)((x, x[:4]), _FakeBlock(True))
    assert mag.block_matches(_FakeBlock(True), 2) and mag.block_matches(_FakeBlock(False), 3)
    assert not mag.block_matches(_FakeBlock(False), 2)


def test_gat_blocks_unsupported_covers_types_1_and_3(monkeypatch):
    from regnn_hip import mag
    from regnn_hip.inference import ShardedInference
    from regnn_hip.ns import gat_blocks_unsupported
    x = {k: torch.zeros(3, 16) for k in range(4)}
    xb = {k: v.bfloat16() for k, v in x.items()}

    def model(kind, slt, **kw):
        return mag.REGNN(16, 8, 5, 2, 10.0, 0.0, {k: 16 for k in range(4)}, 7, model=kind,
                         heads=2, self_loop_type=slt, **kw)

    monkeypatch.setitem(mag.GATV2_BLOCKS, "mode", "on")
    monkeypatch.setitem(mag.NOLOOP_BLOCKS, "mode", "off")    # the default: opt-in
    for slt in (1, 3):
        for kind in KINDS:
            assert gat_blocks_unsupported(model(kind, slt), x) is not None
            with pytest.raises(NotImplementedError, match="REGNN_NOLOOP_BLOCKS"):
                ShardedInference(model(kind, slt), None, None, None, None)
    monkeypatch.setitem(mag.NOLOOP_BLOCKS, "mode", "on")
    for slt in (1, 3):
        for kind in KINDS:
            assert gat_blocks_unsupported(model(kind, slt), x) is None
            assert "fp32 input tables" in gat_blocks_unsupported(model(kind, slt), xb)
        assert "bn" in gat_blocks_unsupported(model("regat", slt, use_norm="bn"), x)
        assert gat_blocks_unsupported(model("regcn", slt, use_norm="bn"), x) is None
        assert model("regcn", slt).typed_first_layer_ok(x) is False
    monkeypatch.setitem(mag.GATV2_BLOCKS, "mode", "off")
    assert "regatv2" in gat_blocks_unsupported(model("regatv2", 3), x)
    # type 2 as before: 'regcn' is not this function's to cover
    assert "regcn" in gat_blocks_unsupported(model("regcn", 2), x)
