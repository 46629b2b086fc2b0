"""The module-path matrix's inputs and reference (tests/_nsmod_ref.py) checked on the CPU, before
tests/test_gpu_nsmod_matrix.py measures the NS module path against them:

* the case builder still draws every array of the fused-step matrix it always drew (hashes taken
  before make_case learnt `hidden` and `hub_fanin`);
* the fp32 yardstick guard per module case: the same restatement in fp32 stays within TOL_GUARD =
  TOL / 4 of the fp64 one at 1 and 4 threads -- a condition on the inputs, never another bound;
* no ReLU input of a case lies within an fp32 rounding of zero (KINK_MARGIN);
* the builder's own asserts per case: the hub's row against the gather's chunk size, the row
  counts of the two grid cases, the live counts of the short batches, the types present;
* RefModel at hidden 512 against oracle.cpu_ns.REGNNCPU where both apply;
* two faults the floor of 1 let through and the own-scale metric catches."""
import hashlib

import numpy as np
import pytest
import torch

import _golden as G
import _nsm_ref as R
import _nsmod_ref as M

# sha256 (first 16 hex digits) over params, x, src, etype, batch and labels of every fused-step
# case, taken from make_case before it had `hidden` and `hub_fanin`
CASE_HASH = {
    "01-t4-k64-slots": "75099f9e0d5e4903", "01-t4-k64-slots-drop": "627f0a306f0ea0c3",
    "02-t4-k64-random": "80dae347c035d695", "03-t1-k64-random": "f29638848a02daaf",
    "04-t1-k128-one-target": "02bd83392c0e08da", "05-t3-k128-rel64-c384": "ec01f4502d4a0cb5",
    "06-t5-k64-c349": "e939617e6a993828", "07-t8-k64-slots": "6d91f5e75cfd0d2b",
    "07-t8-k64-random": "f5b10958cc43b89d", "08-t4-k64-residual-drop": "ef8699de4fa03ac7",
    "09-t4-k128-quarter-unlabelled": "f159a4c590bc7a80",
    "09-t4-k128-all-unlabelled": "a96f58f6aea87cf3", "10-t4-k128-modes": "61d9b98949f2694f",
    "11-composed-c385": "7c8403e63d9b361d", "11-composed-c448": "ff550add6d1407e4",
    "12-composed-k64-c448-random": "0ceda94659f18d61", "13-composed-l3-slots": "be638f8f3bf2a42d",
    "13-composed-l3-slots-drop": "4f8f4a6c462c12fc", "13-composed-l3-random": "2c66a1784dbf332e",
    "13-composed-l3-random-drop": "7991b6535d17ca49", "14-composed-t5-l3": "a2cbf89bd8593947",
    "15-composed-t8-l4-c448-rel64": "eb1803cdeec4791b", "16-composed-t2-l4": "3ccde2e3aaced60b",
    "17-composed-clamps": "ac3b0d1776664b1e", "04-t1-k128-one-target-c3": "35fe984491d8e443",
}


def case_hash(case):
    h = hashlib.sha256()
    for n in sorted(case["params"]):
        h.update(n.encode())
        h.update(np.ascontiguousarray(case["params"][n]).tobytes())
    for x in case["x"]:
        h.update(np.ascontiguousarray(x).tobytes())
    for k in ("src", "etype", "batch", "labels"):
        a = np.ascontiguousarray(case[k])
        h.update(str(a.dtype).encode())
        h.update(a.tobytes())
    return h.hexdigest()[:16]


def test_every_fused_step_case_is_pinned():
    assert set(CASE_HASH) == {s["id"] for s in R.MATRIX}


@pytest.mark.parametrize("id", sorted(CASE_HASH))
def test_fused_step_cases_keep_their_arrays(id):
    case = R.case_of(id)
    assert case["hidden"] == R.HIDDEN == 64 and case["hub_fanin"] == 18
    assert case_hash(case) == CASE_HASH[id]


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("id", M.IDS)
def test_fp32_yardstick_guard(id, threads):
    case, ref = M.case_of(id), M.reference_of(id)
    y32 = R.run_reference(case, torch.float32, threads=threads)
    assert y32["n_id"].tolist() == ref["n_id"].tolist()
    errs = R.compare(y32["loss"], y32["grads"], ref)
    worst = max(errs, key=errs.get)
    print(f"{id}: fp32 yardstick, {threads} thread(s): worst {errs[worst]:.2e} ({worst})")
    for n, e in errs.items():
        assert e <= R.TOL_GUARD, f"{id} {n}: fp32 yardstick {e:.3e} at {threads} thread(s)"


@pytest.mark.parametrize("id", M.IDS)
def test_no_relu_input_within_a_rounding_of_zero(id):
    """_nsmod_ref.KINK_MARGIN: a condition on the inputs, like the guard (m03's first draw held an
    element at 1.1e-7, and the hipBLASLt route of the GEMM_X6 "off" twin flipped it)."""
    assert M.kink_margin(M.case_of(id)) >= M.KINK_MARGIN


@pytest.mark.parametrize("id", M.IDS)
def test_case_carries_what_it_is_there_for(id):
    spec, case, ref = M.SPECS[id], M.case_of(id), M.reference_of(id)
    e, kw, cap = case["edges"], spec["kw"], M.capacity(id)
    B, L, H = case["B"], case["L"], case["hidden"]
    assert H == kw["hidden"] and case["params"]["convs.0.weight"].shape == (H, H)
    assert case["params"]["lins.0.weight"].shape == (H, kw["k_in"])
    assert cap % 16 != 0 and ref["sizes"][-1][1] == B <= cap
    if B >= 17:         # the batch opens with the zero-in-edge target, the hub, the over-fan-out one
        assert e["zero_in"] and e["more"] and e["fewer"] and e["long_row"] >= 17
        assert case["batch"][:3].tolist() == [0, 1, 2]
    else:
        assert B == 1 and e["more"]
    # the hub's row of hop 0's transposed index against the gather's chunk
    chunk = M.hub_chunk(H)
    assert H == 192 or chunk == {64: 128, 128: 64}.get(H, 32)   # (192: no gather width)
    if id.startswith("m18"):
        assert H == 256 and e["long_row"] > 2 * chunk          # 3 or more chunks of 32
    elif id.startswith("m19"):
        assert H == 128 and e["long_row"] > chunk              # 2 or more chunks of 64
    elif B > 1:
        assert e["long_row"] < 32
    # the row counts the two grid cases need, the edge capacity of hop 0's transposed index
    if id == M.LN_CLAMP_ID:
        assert ref["sizes"][0][1] > M.LN_CLAMP_ROWS == 512 * (256 // 64)
    elif H >= 256:
        assert ref["sizes"][0][1] <= M.LN_CLAMP_ROWS
    assert (cap * (kw["sizes"][0] + 1) > M.INDEX_MAX_EDGES) == (id == M.NO_INDEX_ID)
    assert spec["form"]["csc"] == (id != M.NO_INDEX_ID)
    # short batches
    if id.startswith("m16"):
        assert (B, cap) == (61, 97)
    if id.startswith("m17"):
        assert (B, cap) == (1, 33)
    # labels: -1 in the reference, -100 on the device, the same targets
    y, yd = case["labels"][case["batch"]], M.device_labels(case)[case["batch"]]
    assert np.array_equal(y < 0, yd == -100) and np.array_equal(y[y >= 0], yd[y >= 0])
    assert ref["nvalid"] == int((y >= 0).sum())
    if id.startswith("m15"):
        assert (B, ref["nvalid"]) == (97, 73)
    # types: an absent or empty one has exactly zero lins gradients in the reference
    if kw.get("absent_type") is not None:
        assert kw["absent_type"] not in e["types_present"]
        assert kw["empty_type"] not in e["types_present"]
    for t in range(kw["T"]):
        assert bool(ref["grads"][f"lins.{t}.weight"].any()) == (t in e["types_present"])
    # what decides the form: relation slots and <= 4 types of width 128 for the input sums
    slots = e["slots"] and kw["T"] <= 4 and kw["k_in"] == 128
    assert spec["form"]["pre_sums"] == slots
    assert spec["form"]["epi"] == (H in (128, 256, 512, 1024))
    assert spec["form"]["live"] == (spec["form"]["epi"] and not kw.get("residual", False))
    assert spec["form"]["strided0"] == (spec["form"]["csc"] and H in (64, 128, 256, 512, 1024, 2048))
    assert L <= 4                              # rel_tabs' kTabsMax


def test_refmodel_h512_matches_regnncpu():
    """RefModel at the module path's width against the pinned oracle where both apply (no
    residual, no dropout, every target labelled): loss, log-probabilities and every gradient at
    the golden pins' 2e-6."""
    from oracle import cpu_ns as CN
    id = "m03-h512"
    case, ref = M.case_of(id), M.reference_of(id)
    assert case["hidden"] == 512 and not case["residual"] and case["dropout"] == 0
    m = CN.REGNNCPU(case["k_in"], 512, case["C"], case["L"], R.ALPHA, 0.0, case["T"],
                    case["n_et"]).double()
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_(torch.from_numpy(case["params"][n]))
    n_id, adjs = R.sample(case)
    x_dict = {t: torch.from_numpy(x).double() for t, x in enumerate(case["x"])}
    logp = m(torch.from_numpy(n_id), x_dict, adjs, torch.from_numpy(case["etype"]),
             torch.from_numpy(case["ntype"]), torch.from_numpy(case["local"]))
    y = torch.from_numpy(case["labels"][case["batch"]])
    assert (y >= 0).all()
    loss = torch.nn.functional.nll_loss(logp, y)
    loss.backward()
    for tag, got, want in (("loss", ref["loss"], float(loss.detach())),
                           ("logp", ref["logp"], logp.detach().numpy())):
        ok, err = G.close(got, want, 2e-6)
        assert ok, f"{tag}: rel err {err:.3e}"
    for n, p in m.named_parameters():
        if p.grad is None:
            assert n not in ref["grads"]
            continue
        ok, err = G.close(ref["grads"][n], p.grad.numpy(), 2e-6)
        assert ok, f"{n}: rel err {err:.3e}"
        assert R.own_scale_error(ref["grads"][n], p.grad.numpy()) <= 2e-6, n


def test_own_scale_metric_catches_dropped_rows_at_h512():
    """the last 3 rows of one lins.t.weight gradient dropped (a ragged tail of the [512, 128]
    product lost), in the batch's rarest type (max|ref| 9e-7): passes _golden.close at 1e-5 and
    fails compare on the m03 reference by orders of magnitude; no other figure moves."""
    ref = M.reference_of("m03-h512")
    got = {n: g.copy() for n, g in ref["grads"].items()}
    n = min((k for k in (f"lins.{t}.weight" for t in range(4)) if ref["grads"][k].any()),
            key=lambda k: np.abs(ref["grads"][k]).max())
    assert got[n].shape == (512, 128) and np.abs(got[n][-3:]).max() > 0
    got[n][-3:] = 0.0
    ok, err = G.close(got[n], ref["grads"][n], 1e-5)
    print(f"{n}: last 3 rows dropped: _golden.close {ok} ({err:.2e}), max|ref| "
          f"{np.abs(ref['grads'][n]).max():.2e}")
    assert ok                                               # the old yardstick: passes
    errs = R.compare(ref["loss"], got, ref)
    assert errs[n] > 100 * R.TOL and all(e == 0 for k, e in errs.items() if k != n), errs[n]


def test_own_scale_metric_catches_a_single_pass_clamp(monkeypatch):
    """a LayerNorm weight gradient summed over the first 2048 rows of its layer only -- what
    ln_bwd_kernel's clamped grid gives without its row loop -- fails compare. It is taken where a
    layer has more than 2048 rows: convs.0.norm.weight of the clamp case (the issue names
    convs.1.norm.weight on m03, whose layers hold 531 and 97 rows: nothing to drop there).
    _golden.close's verdict is printed, not asserted: the issue expected it to pass, but the 613
    lost rows carry 3.6e-3 of a gradient of 1e-2 in size, which the floor of 1 rejects as well."""
    id = M.LN_CLAMP_ID
    case, ref = M.case_of(id), M.reference_of(id)
    kept = []

    def layer_norm(x, ln):
        mu = x.mean(1, keepdim=True)
        xhat = (x - mu) / torch.sqrt(((x - mu) ** 2).mean(1, keepdim=True) + ln.eps)
        out = xhat * ln.weight + ln.bias
        out.retain_grad()
        kept.append((xhat.detach(), out))
        return out
    monkeypatch.setattr(R, "_layer_norm", layer_norm)
    again = R.run_reference(case)
    n = "convs.0.norm.weight"
    xhat, out = kept[0]
    assert xhat.shape[0] == ref["sizes"][0][1] > M.LN_CLAMP_ROWS
    terms = (out.grad * xhat).numpy()
    assert R.own_scale_error(terms.sum(0), ref["grads"][n]) <= 1e-12
    assert R.own_scale_error(again["grads"][n], ref["grads"][n]) <= 1e-12
    got = {k: g.copy() for k, g in ref["grads"].items()}
    got[n] = terms[:M.LN_CLAMP_ROWS].sum(0)
    ok, err = G.close(got[n], ref["grads"][n], 1e-5)
    print(f"{n}: first {M.LN_CLAMP_ROWS} rows only: _golden.close {ok} ({err:.2e})")
    assert R.compare(ref["loss"], got, ref)[n] > 100 * R.TOL
