"""The fused NS step's fp64 reference (tests/_nsm_ref.py) checked on the CPU, before
tests/test_gpu_nsm_matrix.py measures regnn_nsm_step against it:

* golden pin: the helper's sampler + restatement reproduce the reference REGNN's own vectors
  (mag_regnn_schema, mag_regnn_ft3; with the residual subclass nsres_regnn_*) at the tolerance of
  tests/test_oracle.py;
* the unlabelled-target mean against torch's nll_loss(ignore_index=-1);
* the fp32 yardstick guard: on every case of the GPU matrix, the same restatement in fp32 stays
  within TOL_GUARD = TOL / 4 of the fp64 one under the own-scale metric, the per-element
  relation metric included, at 1 thread and, for the largest case and the two with the least
  margin, at 2, 4 and 16 -- a condition on the inputs (never another bound);
* the builder's declared edges, case by case;
* the metric's exact-zero rule."""
import numpy as np
import pytest
import torch

import _golden as G
import _nsm_ref as R

GOLDEN_TOL = 2e-6          # tests/test_oracle.py: fp64 results stored as fp32


@pytest.mark.parametrize("name", ["mag_regnn_schema", "mag_regnn_ft3", "nsres_regnn_schema",
                                  "nsres_regnn_ft3"])
def test_reference_reproduces_golden(name):
    d = G.load(name)
    case = R.case_from_fixture(d)
    assert case["residual"] == name.startswith("nsres")
    assert R.slots_eligible(case) == (d["meta"].get("schema") == "ogbn-mag")
    ref = R.run_reference(case)
    assert ref["n_id"].tolist() == d["n_id"].tolist()
    L = case["L"]
    for h in range(L):
        assert ref["sizes"][h] == tuple(int(v) for v in d[f"adj{h}_size"])
        assert ref["edges"][h] == d[f"adj{h}_src"].size
    for tag, got, want in (("logp", ref["logp"], d["logp"]), ("loss", ref["loss"], d["loss"])):
        ok, err = G.close(got, want, GOLDEN_TOL)
        assert ok, f"{tag}: rel err {err:.3e}"
    want = G.sub(d, "grad_")
    assert set(want) == set(ref["grads"]), set(want) ^ set(ref["grads"])
    for k, v in want.items():
        ok, err = G.close(ref["grads"][k], v, GOLDEN_TOL)
        assert ok, f"{k}: rel err {err:.3e}"
        # the fixtures hold fp32 roundings of fp64 results: 2^-24 of the tensor's own maximum
        assert R.own_scale_error(ref["grads"][k], v) <= 2e-7, k


def test_unlabelled_mean_matches_torch_ignore_index():
    id = "09-t4-k128-quarter-unlabelled"
    case, ref = R.case_of(id), R.reference_of(id)
    y = torch.from_numpy(case["labels"][case["batch"]])
    assert 0 < int((y < 0).sum()) < y.numel() and ref["nvalid"] == int((y >= 0).sum())
    logp = torch.from_numpy(ref["logp"])
    want = torch.nn.functional.nll_loss(logp, y, ignore_index=-1)
    assert abs(ref["loss"] - float(want)) <= 1e-14 * abs(float(want))
    # the gradient too: the same model under torch's own mean
    n_id, adjs = R.sample(case)
    m = R.build_model(case, torch.float64)
    x_dict = {t: torch.from_numpy(x).double() for t, x in enumerate(case["x"])}
    out = m(torch.from_numpy(n_id), x_dict, adjs, torch.from_numpy(case["etype"]),
            torch.from_numpy(case["ntype"]), torch.from_numpy(case["local"]))
    torch.nn.functional.nll_loss(out, y, ignore_index=-1).backward()
    for n, p in m.named_parameters():
        if p.grad is not None:
            assert R.own_scale_error(ref["grads"][n], p.grad.numpy()) <= 1e-12, n
    # no labelled target: loss 0 and every gradient exactly 0 (the step's contract; torch's mean
    # over nothing is NaN)
    ref0 = R.reference_of("09-t4-k128-all-unlabelled")
    assert ref0["nvalid"] == 0 and ref0["loss"] == 0.0
    assert all(not g.any() for g in ref0["grads"].values())


def _yardstick(id, threads):
    case, ref = R.case_of(id), R.reference_of(id)
    y32 = R.run_reference(case, torch.float32, threads=threads)
    assert y32["n_id"].tolist() == ref["n_id"].tolist()
    errs = R.compare(y32["loss"], y32["grads"], ref)
    worst = max(errs, key=errs.get)
    print(f"{id}: fp32 yardstick, {threads} thread(s): worst {errs[worst]:.2e} ({worst})")
    assert set(ref["rel_scale"]) == {f"convs.{l}.relation_weight" for l in range(case["L"])}
    for n, e in errs.items():
        assert e <= R.TOL_GUARD, f"{id} {n}: fp32 yardstick {e:.3e} at {threads} thread(s)"


@pytest.mark.parametrize("id", [s["id"] for s in R.MATRIX])
def test_fp32_yardstick_guard(id):
    """fp32 arithmetic alone costs at most TOL / 4 on this case's inputs, so TOL = 1e-5 on the
    kernel needs no floor. run_reference pins torch's thread count, so the figure repeats."""
    _yardstick(id, 1)


@pytest.mark.parametrize("threads", [2, 4, 16])
@pytest.mark.parametrize("id", [R.CLAMP_ID, "13-composed-l3-slots", "06-t5-k64-c349"])
def test_fp32_yardstick_guard_any_thread_count(id, threads):
    """the guard does not hang on one summation order: the largest case (35,000 rows) and the two
    with the least margin hold it at other thread counts too. (The restatement reduces over a
    block's rows and entries with torch.sum's cascade summation, _nsm_ref._layer_norm.)"""
    _yardstick(id, threads)


@pytest.mark.parametrize("id", [s["id"] for s in R.MATRIX])
def test_case_carries_its_edges(id):
    spec, case, ref = R.SPECS[id], R.case_of(id), R.reference_of(id)
    e, kw = case["edges"], spec["kw"]
    B, L = kw["B"], kw["L"]
    assert e["B_odd"] and ref["sizes"][-1][1] == B
    assert e["slots"] == (kw["schema"] == "slots") == bool(spec["rel_slots"])
    assert kw["T"] * (kw["k_in"] + 1) <= 600 and kw["n_edge_types"] + kw["T"] <= 64
    two = L == 2 and kw["C"] <= 384 and B * (kw["sizes"][0] + 1) <= 32768
    assert spec["form"] == ("two" if two else "composed")
    if B >= 17:
        assert e["zero_in"] and e["more"] and e["fewer"] and e["long_row"] >= 17
    else:
        assert B == 1 and e["more"]
    # the zero-in-degree target's row holds its self loop only
    if B >= 17:
        assert not (R.sample(case)[1][-1][1] == 0).any()
    want_unl = {None: 0, "quarter": len(case["batch"][2::4]), "all": B}[kw.get("unlabelled")]
    assert e["unlabelled"] == want_unl == B - ref["nvalid"]
    if "absent_type" in kw:
        a, z = kw["absent_type"], kw["empty_type"]
        assert case["counts"][a] > 0 and a not in e["types_present"]
        assert case["counts"][z] == 0 and z not in e["types_present"]
    # (a sparse pair table may keep a further type out of a batch: the same rule holds for it)
    for t in range(kw["T"]):                   # absent: exactly zero in the reference
        gone = t not in e["types_present"]
        assert bool(ref["grads"][f"lins.{t}.weight"].any()) == (not gone and ref["nvalid"] > 0
                                                                and kw["C"] > 1)
    if kw["T"] > 1:
        assert len(e["types_present"]) >= 2
    if id == R.CLAMP_ID:
        # live layer-0 / layer-1 target rows past agg0's 2048 and agg's 1024 blocks of 16 rows
        assert ref["sizes"][0][1] > R.CLAMP_ROWS0 and ref["sizes"][1][1] > R.CLAMP_ROWS1
    if kw["n_edge_types"] + kw["T"] == 64:
        assert all(case["params"][f"convs.{l}.relation_weight"].size == 64 for l in range(L))
    if kw["L"] == 4 and kw["T"] == 8:
        assert 6 + L + 4 * (L - 1) + kw["T"] == 30     # finalize's longest job list (of 32)


def test_some_relation_has_no_sampled_edge():
    """the exact-zero rule has a live instance: a relation of the 64-entry tables without a
    sampled edge in some layer (scale 0, reference 0)."""
    ref = R.reference_of("05-t3-k128-rel64-c384")
    sc, g = ref["rel_scale"]["convs.1.relation_weight"], ref["grads"]["convs.1.relation_weight"]
    assert (sc == 0).any() and not g[sc == 0].any() and g[sc > 0].all()


def test_own_scale_metric_catches_a_dropped_row():
    """what the floor of 1 let through: in the gradient of the batch's rarest type's lins.t.weight
    (max|ref| 4e-6: below 1e-5 x 1) a dropped last row -- the whole tensor zeroed, even -- passes
    _golden.close at 1e-5; under the own-scale metric both fail by orders of magnitude."""
    id = "01-t4-k64-slots"
    ref = R.reference_of(id)
    got = {n: g.copy() for n, g in R.run_reference(R.case_of(id), torch.float32)["grads"].items()}
    assert max(R.compare(ref["loss"], got, ref).values()) <= R.TOL_GUARD
    n = min((f"lins.{t}.weight" for t in range(4)), key=lambda k: np.abs(ref["grads"][k]).max())
    assert 0 < np.abs(ref["grads"][n]).max() < 1e-5
    for rows in (slice(-1, None), slice(None)):
        bad = dict(got)
        bad[n] = got[n].copy()
        bad[n][rows] = 0.0
        ok, _ = G.close(bad[n], ref["grads"][n], 1e-5)
        assert ok                                           # the old yardstick: passes
        err = R.compare(ref["loss"], bad, ref)[n]
        assert err > 100 * R.TOL, (n, err)


def test_own_scale_error_rules():
    ref = np.array([0.0, 2e-3, -4e-3])
    assert R.own_scale_error(ref, ref) == 0.0
    assert R.own_scale_error(ref + np.array([0, 4e-8, 0]), ref) == pytest.approx(1e-5)
    assert R.own_scale_error(ref + np.array([1e-30, 0, 0]), ref) == float("inf")   # exact zero
    assert R.own_scale_error(np.zeros(3), np.zeros(3)) == 0.0
    assert R.own_scale_error(np.array([0, 0, 1e-30]), np.zeros(3)) == float("inf")
    # per element: a small entry is held to its own scale, not to the tensor's maximum
    sc = np.array([0.0, 1.0, 1e-4])
    got = ref + np.array([0, 0, 1e-8])
    assert R.own_scale_error(got, ref) == pytest.approx(2.5e-6)
    assert R.own_scale_error(got, ref, sc) == pytest.approx(1e-4)
    assert R.own_scale_error(np.array([np.nan, 0, 0]), ref) == float("inf")
