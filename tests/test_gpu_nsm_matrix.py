"""regnn_nsm_step (re_nsm.hip + re_nsm2.hip) against the fp64 reference of tests/_nsm_ref.py over
its envelope: input widths 64 and 128, 1..8 node types, 2..4 layers, up to 448 classes and 64
relations, relation slots and the edge pass, residual, dropout, unlabelled targets, a type absent
from the batch, every sampler / agg0 mode, and the composed form's grid clamps (_nsm_ref.MATRIX).

Per case: the device sampler's batch equals the CPU sampler's, the step took the form the case
is there for (two-layer / composed, relation slots, the sampler's input sums), and the loss and
every parameter gradient lie within TOL = 1e-5 of the reference on the tensor's own maximum --
the relation tables also per element, structural zeros exactly. Two-layer cases run twice and
must repeat bitwise (the composed form sums with float atomics and is not asked to).
tests/test_cpu_nsm_ref.py holds the fp32 yardstick to TOL / 4 on the same inputs."""
import numpy as np
import pytest
import torch

import _nsm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _setup(case):
    """RelGraph, DeviceSampler and mag.REGNN (the case's parameters by name, zeroed .grad)."""
    from regnn_hip import mag
    from regnn_hip.graph import RelGraph
    from regnn_hip.ns import DeviceSampler
    T, K, L = case["T"], case["k_in"], case["L"]
    rg = RelGraph(torch.from_numpy(case["src"]), torch.from_numpy(case["dst"]), case["N"], DEV)
    # the CPU sampler's CSR is the device's: positions are edge ids
    assert torch.equal(rg.csr_eid.cpu(), torch.arange(case["src"].size))
    assert torch.equal(rg.csr_ptr.cpu().long(), torch.from_numpy(case["ptr"]))
    ds = DeviceSampler(rg, case["sizes"], case["B"], etype=torch.from_numpy(case["etype"]),
                       ntype=torch.from_numpy(case["ntype"]), num_edge_types=case["n_et"])
    model = mag.REGNN(K, case.get("hidden", R.HIDDEN), case["C"], L, R.ALPHA, case["dropout"],
                      {t: K for t in range(T)}, case["n_et"], residual=case["residual"],
                      use_norm="ln", self_loop_type=2)
    assert {n for n, _ in model.named_parameters()} == set(case["params"])
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(torch.from_numpy(case["params"][n]))
    model = model.to(DEV)
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    model.train(case["dropout"] > 0)
    x_dict = {t: torch.from_numpy(x).to(DEV) for t, x in enumerate(case["x"])}
    return rg, ds, model, x_dict


def _untouched(ds):
    return (all(m is None for m in ds.edge_meta) and all(c is None for c in ds.csc) and
            all(t is None for t in ds.typed_sums) and not ds.strided and not any(ds.meta_only)
            and ds.local is None)


def _run(id, strided=True, lean=True, pre_sums=None):
    """one step of case `id` with every assert of the module docstring; returns the figures."""
    from regnn_hip.ns import FusedStep
    spec, case = R.SPECS[id], R.case_of(id)
    L, B = case["L"], case["B"]
    rg, ds, model, x_dict = _setup(case)
    loss = torch.full((), 7.0, device=DEV)
    fs = FusedStep(model, ds, x_dict, torch.from_numpy(case["ntype"]).to(DEV),
                   torch.from_numpy(case["local"]).to(DEV), torch.from_numpy(case["labels"]), loss)
    # -- the form taken --------------------------------------------------------------------------
    two = spec["form"] == "two"
    assert fs.two_layer == two and fs.P.two_layer == int(two)
    assert fs.P.rel_slots == spec["rel_slots"]
    assert fs.P.k_in == case["k_in"] and fs.P.n_types == case["T"]
    assert fs.P.n_layers == L and fs.P.n_classes == case["C"]
    assert fs.P.residual == int(case["residual"])
    assert all(fs.P.n_rel[l] == case["n_et"] + case["T"] for l in range(L))
    want_pre = spec["pre_sums"] if pre_sums is None else pre_sums
    assert fs.W.pre_sums == want_pre
    assert ds.strided == (two and strided) and bool(fs.W.stride[0]) == (two and strided)
    assert ds.meta_only[L - 1] == lean
    ks = fs.kernels()
    assert ks[:2] == (["agg0", "head"] if two else ["prep", "agg0"])
    assert ks.count("agg") == (0 if two else L - 2) and ("rel0" in ks) == (not spec["rel_slots"])
    # -- the batch -------------------------------------------------------------------------------
    ds.set_seed(case["seed"], case["epoch"], case["batch_idx"])
    ds.set_targets(torch.from_numpy(case["batch"]).to(DEV))
    ds.run_hops()
    st = ds.state.cpu().tolist()
    assert (st[0], st[1], st[3]) == (case["seed"], case["epoch"], case["batch_idx"])
    ref = (R.run_reference(case, state=st) if case["dropout"] > 0 else R.reference_of(id))
    sz = ds.sizes.cpu().tolist()
    for h in range(L):                          # hop h's block = the reference's adjs[L - 1 - h]
        n_src, n_dst = ref["sizes"][L - 1 - h]
        assert sz[h] == n_dst
        assert sz[8 + h] == ref["edges"][L - 1 - h] + n_dst        # + one self loop per row
    n_chk = sz[L - 1] if lean else sz[L]        # the meta-only last hop appends nothing to n_id
    assert n_chk == (ref["sizes"][0][1] if lean else ref["n_id"].size)
    assert ds.n_id[:n_chk].cpu().tolist() == ref["n_id"][:n_chk].tolist()
    if id == R.CLAMP_ID:                        # both grid clamps loop
        assert sz[L - 1] > R.CLAMP_ROWS0 and -(-ds.caps[L - 1] // 16) > 2048
        assert sz[L - 2] > R.CLAMP_ROWS1 and -(-ds.caps[L - 2] // 16) > 1024
    # -- the step --------------------------------------------------------------------------------
    fs.step()
    torch.cuda.synchronize()
    got_loss = float(loss)
    got = {n: p.grad.detach().cpu().double().numpy() for n, p in model.named_parameters()}
    for n in set(got) - set(ref["grads"]):      # REGNN.norm: declared, never read
        assert n.startswith("norm.") and not got[n].any(), n
    errs = R.compare(got_loss, got, ref)
    nz = [float(np.abs(g).max()) for g in ref["grads"].values() if g.any()]
    worst = max(errs, key=errs.get)
    for n, e in errs.items():
        print(f"{id} {n}: {e:.3e}")
    print(f"NSM_MATRIX {id} worst {errs[worst]:.2e} ({worst}) smallest max|ref| "
          f"{min(nz) if nz else 0.0:.2e} loss {got_loss:.6f} ref {ref['loss']:.6f}")
    # -- bitwise repeat (two-layer form) ---------------------------------------------------------
    if two:
        fs.step()
        torch.cuda.synchronize()
        assert float(loss) == got_loss or (np.isnan(got_loss) and np.isnan(float(loss)))
        for n, p in model.named_parameters():
            assert np.array_equal(p.grad.cpu().double().numpy(), got[n]), n
    bad = {n: e for n, e in errs.items() if not e <= R.TOL}
    assert not bad, f"{id}: own-scale error past {R.TOL:g}: {bad}"
    return dict(loss=got_loss, ref=ref, errs=errs)


PLAIN = [s["id"] for s in R.MATRIX if not s["id"].startswith(("09-", "10-"))]


@pytest.mark.parametrize("id", PLAIN)
def test_nsm_step_matches_fp64_reference(id):
    _run(id)


def test_nsm_step_quarter_unlabelled():
    """the loss and every gradient are means over the 73 labelled of 97 targets."""
    out = _run("09-t4-k128-quarter-unlabelled")
    assert out["ref"]["nvalid"] == 73


def test_nsm_step_no_labelled_target():
    """include/regnn_hip.h, regnn_nsm_params.loss: no labelled target in the batch -> loss 0 and
    every gradient exactly 0 (not torch's NaN mean over nothing)."""
    out = _run("09-t4-k128-all-unlabelled")
    assert out["ref"]["nvalid"] == 0 and out["loss"] == 0.0


@pytest.mark.parametrize("mode", ["default", "strided_off", "lean_off", "pre_sums_off"])
def test_nsm_step_modes(monkeypatch, mode):
    """the two-layer step's sampler layouts and agg0 forms on one batch: CSR blocks, the full
    last hop and agg0's own gather (each turns the sampler's input sums off)."""
    from regnn_hip import ns
    if mode == "strided_off":
        monkeypatch.setitem(ns.STRIDED, "mode", "off")
    if mode == "lean_off":
        monkeypatch.setitem(ns.LEAN_LAST_HOP, "mode", "off")
    if mode == "pre_sums_off":
        monkeypatch.setitem(ns.PRE_SUMS, "mode", "off")
    _run("10-t4-k128-modes", strided=mode != "strided_off", lean=mode != "lean_off",
         pre_sums=int(mode == "default"))


# make_case's arguments and the reason FusedStep must give (fused_unsupported's wording)
REFUSED = {
    "t5-k128": (dict(T=5, k_in=128, L=2, C=37, n_edge_types=9),        # 5 x 129 > 600
                r"5 node types x input width 128 exceed the fused step's tables"),
    "c449": (dict(T=4, k_in=64, L=2, C=449, n_edge_types=7), r"out_lin must be 64 -> <= 448"),
    "rel65": (dict(T=4, k_in=64, L=2, C=37, n_edge_types=61), r"relation table > 64"),
    "k96": (dict(T=4, k_in=96, L=2, C=37, n_edge_types=7),
            r"input widths must be equal, 64 or 128"),
    "residual-l3": (dict(T=4, k_in=64, L=3, C=37, n_edge_types=7, residual=True),
                    r"residual convs run in the fused step's two-layer form only"),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_nsm_step_refuses_outside_envelope(what):
    """outside the header's envelope FusedStep raises, for the reason the case is named after,
    before any launch and before it changes anything of the sampler."""
    from regnn_hip.ns import FusedStep
    kw, why = dict(REFUSED[what][0]), REFUSED[what][1]
    L = kw["L"]
    case = R.make_case(B=33, sizes=(5, 4, 3)[:L], schema="random", n_nodes=600, seed=50, **kw)
    rg, ds, model, x_dict = _setup(case)
    assert _untouched(ds)
    loss = torch.full((), 7.0, device=DEV)
    with pytest.raises(ValueError, match="regnn_nsm_step does not cover this model: " + why):
        FusedStep(model, ds, x_dict, torch.from_numpy(case["ntype"]).to(DEV),
                  torch.from_numpy(case["local"]).to(DEV), torch.from_numpy(case["labels"]), loss)
    assert _untouched(ds)
    torch.cuda.synchronize()
    assert float(loss) == 7.0 and all(not p.grad.any() for p in model.parameters())
