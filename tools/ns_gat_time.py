"""Per-step time of NS 'regat' / 'regatv2' training on the device-sampled blocks against the
default exact-size path, in one process (bench.py times the 'regcn' step only):

    python tools/ns_gat_time.py [--model regat] [--scale 1] [--batch 512] [--steps 20]
                                [--rounds 7] [--kernel-steps 0] [--src atomic] [--out FILE]
                                [--tables fp32|bf16]

One graph -- mag_like(scale), 128-d inputs, REGNN 'regat' hidden 64 x 8 heads, 349 classes,
fan-out [25, 20], dropout 0.5, FlatAdam -- and two trainers over it:

  A  NSTrainer(...)                       the default: exact-size adjs (a host read of the
                                          sampler's sizes per step), mag.make_block and the
                                          gat_scores / amax / edge_softmax / head SpMM chain, eager
  B  NSTrainer(..., device_blocks=True)   the capacity-sized blocks through ops.ns_gat, the next
                                          batch sampled on a second stream, captured (one-step
                                          graphs), run_steps

--model regatv2: the same two paths for REGATv2Conv; B switches mag.GATV2_BLOCKS on (the blocks
through ops.ns_gatv2), A is the gatv2_scores / amax / edge_softmax / head SpMM chain.
--kernel-steps K > 0: after the windows, K more eager steps of B under ops' event timers; the
attention operator's device time per step (both layers) goes into "kernel_us_per_step".

--src gather: a third trainer C, path B with ops.NS_GAT_SRC = "gather" (the backwards' per-source
sums by a gather over each block's transposed index, built on the sampler's stream: no float
atomics), captured as B is; the windows then alternate A, B, C, so gather is timed against the
atomic form in the same process. Its peak memory is measured as B's is, and --kernel-steps times
both forms ("kernel_us_per_step" for B, "kernel_us_per_step_gather" for C, the latter with the
index build, ns_block_tidx, on the sampler's stream).

--tables bf16: a further trainer D, path B on bf16 copies of the input tables (x.bfloat16(), with
ops.BF16_ROWS "on": group_input's gather-fused Linear reads the bf16 rows), captured as B is and
timed in the same alternating windows; the JSON line then carries both tables' bytes and D's peak.

After warm-up runs of both, `rounds` timed windows of `steps` steps each, alternating A and B; a
window is a host clock around the steps ending in a device synchronise. Prints (and with --out
writes) one JSON line: each path's per-step median, min and max over the rounds (us), B's peak
device memory after capture and warm-up (torch.cuda.max_memory_allocated over B's construction,
capture and warm-up; A's tensors made earlier are included in the figure's base and listed apart).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "re-gnn_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--dropout", type=float, default=0.5)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--model", choices=["regat", "regatv2"], default="regat")
    ap.add_argument("--kernel-steps", type=int, default=0)
    ap.add_argument("--src", choices=["atomic", "gather"], default="atomic")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tables", choices=["fp32", "bf16"], default="fp32")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ns_gat_time: needs the GPU (no CPU timing)")
    from regnn_hip import mag, ops, synth
    from regnn_hip.graph import RelGraph
    from regnn_hip.ns import NSTrainer
    dev = "cuda"
    gd = synth.mag_like(args.scale, seed=0, device=dev, zipf_s=1.1)
    keep = gd["rel"] <= 7
    rg = RelGraph(gd["src"][keep], gd["dst"][keep], gd["N"], dev)
    edge_type = gd["rel"][keep].to(torch.int64) - 1
    del keep, gd["src"], gd["dst"], gd["rel"]
    node_type = gd["ntype"]
    offs = torch.tensor([gd["type_offsets"][t] for t in synth.NTYPES], device=dev)
    local = torch.arange(gd["N"], device=dev) - offs[node_type]
    feats = synth.type_features(gd["counts"], {t: 128 for t in synth.NTYPES}, seed=1, device=dev)
    x_dict = {k: f for k, f in enumerate(feats)}
    n_paper = gd["counts"]["paper"]
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    y = torch.full((gd["N"], 1), -1, dtype=torch.int64, device=dev)
    y[:n_paper, 0] = torch.randint(0, 349, (n_paper,), generator=gen, device=dev)

    def trainer(x_dict=x_dict, **kw):
        torch.manual_seed(3)
        model = mag.REGNN(128, args.hidden, 349, 2, 10.0, args.dropout,
                          {k: 128 for k in x_dict}, 7, use_norm="ln", self_loop_type=2,
                          model=args.model, heads=args.heads).to(dev)
        model.train()
        return NSTrainer(model, None, rg, [25, 20], args.batch,
                         torch.arange(n_paper, device=dev), x_dict, edge_type, node_type, local,
                         y, 7, seed=123, adam=dict(lr=1e-3), **kw)

    def run_a(tr, k):
        for _ in range(k):
            tr.step()

    tr_a = trainer()
    assert tr_a.fused is None and not tr_a._blocks_ok
    run_a(tr_a, args.warmup)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    if args.model == "regatv2":
        mag.GATV2_BLOCKS["mode"] = "on"        # path B only: A was built and warmed before
    tr_b = trainer(device_blocks=True)
    assert tr_b._gat_blocks and tr_b.pipelined and tr_b.ahead == 1
    tr_b.capture(warmup=2)
    tr_b.run_steps(args.warmup)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    runs = {"exact_eager": lambda k: run_a(tr_a, k), "device_blocks_captured": tr_b.run_steps}
    trainers = {"exact_eager": tr_a, "device_blocks_captured": tr_b}
    peak_c = base_c = None
    if args.src == "gather":
        base_c = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        ops.NS_GAT_SRC["mode"] = "gather"      # read when C is built and when it is captured
        tr_c = trainer(device_blocks=True)
        assert tr_c._gat_src_gather and tr_c.pipelined and tr_c.ahead == 1
        tr_c.capture(warmup=2)
        tr_c.run_steps(args.warmup)
        torch.cuda.synchronize()
        peak_c = torch.cuda.max_memory_allocated()
        ops.NS_GAT_SRC["mode"] = "atomic"
        runs["device_blocks_gather_captured"] = tr_c.run_steps
        trainers["device_blocks_gather_captured"] = tr_c
    peak_d = base_d = None
    if args.tables == "bf16":
        xb = {k: v.bfloat16().contiguous() for k, v in x_dict.items()}
        torch.cuda.synchronize()
        base_d = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        ops.BF16_ROWS["mode"] = "on"
        tr_d = trainer(x_dict=xb, device_blocks=True)
        assert tr_d._gat_blocks and tr_d.pipelined and tr_d.ahead == 1
        tr_d.capture(warmup=2)
        tr_d.run_steps(args.warmup)
        torch.cuda.synchronize()
        peak_d = torch.cuda.max_memory_allocated()
        runs["device_blocks_bf16_tables_captured"] = tr_d.run_steps
        trainers["device_blocks_bf16_tables_captured"] = tr_d
    us = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, run in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(args.steps)
            torch.cuda.synchronize()
            us[k].append((time.perf_counter() - t0) / args.steps * 1e6)
    out = {"workload": f"mag_like({args.scale:g}) NS step, {args.model} hidden {args.hidden} x "
                       f"{args.heads} heads, batch {args.batch}, fan-out [25, 20], dropout "
                       f"{args.dropout}, FlatAdam",
           "steps_per_window": args.steps, "rounds": args.rounds,
           "device_blocks_peak_bytes": int(peak), "allocated_before_device_blocks_bytes": int(base)}
    for k, v in us.items():
        out[k] = {"us_per_step_median": round(statistics.median(v), 1),
                  "min": round(min(v), 1), "max": round(max(v), 1),
                  "final_loss": float(trainers[k].loss)}
    if peak_c is not None:
        out["device_blocks_gather_peak_bytes"] = int(peak_c)
        out["allocated_before_device_blocks_gather_bytes"] = int(base_c)
    if peak_d is not None:
        nbytes = lambda d: sum(t.numel() * t.element_size() for t in d.values())  # noqa: E731
        out["table_bytes"] = {"fp32": nbytes(x_dict), "bf16": nbytes(xb)}
        # (D's peak and base both hold the fp32 tables and the earlier trainers)
        out["device_blocks_bf16_tables_peak_bytes"] = int(peak_d)
        out["allocated_before_device_blocks_bf16_tables_bytes"] = int(base_d)
    if args.kernel_steps > 0:
        from regnn_hip import profile
        forms = [("kernel_us_per_step", tr_b, "atomic")]
        if args.src == "gather":
            forms.append(("kernel_us_per_step_gather", tr_c, "gather"))
        for key, tr, mode in forms:
            ops.NS_GAT_SRC["mode"] = mode      # eager steps read it at every backward
            profile.enable()
            for _ in range(args.kernel_steps):
                tr.step()
            torch.cuda.synchronize()
            out[key] = {
                k: round(v[2] * 1e3 / args.kernel_steps, 1)
                for k, v in sorted(profile.summary().items())
                if k.startswith("ns_gat") or k == "ns_block_tidx"}
            profile.enable(False)
        ops.NS_GAT_SRC["mode"] = "atomic"
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
