"""Per-step time of the NS step on bf16 input feature tables against fp32 tables, in one process:

    python tools/ns_bf16_time.py [--scale 10] [--batch 512] [--steps 160] [--rounds 7]
                                 [--hidden 64|512] [--first fp32|bf16] [--only fp32|bf16]
                                 [--residual] [--rows off|on] [--out FILE]

bench.py's NS workload twice over one graph -- mag_like(scale), 128-d inputs, 349 classes, fan-out
[25, 20], dropout 0.5, FlatAdam, pipelined and captured (NSTrainer.capture / run_steps) -- once
on the fp32 tables and once on their bf16 copies (x.bfloat16(): the sampler's sums launch reads
256-byte rows, regnn_ns_hop_typed_sums_dt). --hidden 64: the fused two-layer step; --hidden 512:
the module path. After warm-up runs of both, `rounds` timed windows of `steps` steps each,
alternating the two trainers; a window is a host clock around run_steps() ending in a device
synchronise. Prints every round's us per step and one JSON line with each variant's median, min
and max, the table bytes, the memory each trainer holds on top of the graph and the tables, and
the process's peak allocated memory after capture() (--only: with that dtype's tables alone). No
step is retried.

--rows on: ops.BF16_ROWS "on" -- the model's own readers of raw rows (group_input's gather-fused
Linear, layer 0's typed aggregation) take the bf16 tables too; --residual: residual convs (module
path only: they project the targets' raw rows, which on bf16 tables needs --rows on). --out FILE:
the JSON line is also written there.
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
    ap.add_argument("--scale", type=float, default=10.0)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=160)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--dropout", type=float, default=0.5)
    ap.add_argument("--first", choices=["fp32", "bf16"], default="fp32",
                    help="the variant whose trainer is built first and leads every round")
    ap.add_argument("--only", choices=["fp32", "bf16"], default=None,
                    help="build and time this variant alone (its tables only: the process's "
                         "peak allocated memory is then that of a user of this dtype)")
    ap.add_argument("--residual", action="store_true", help="residual convs (--hidden 512)")
    ap.add_argument("--rows", choices=["off", "on"], default="off", help="ops.BF16_ROWS")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ns_bf16_time: needs the GPU (no CPU timing)")
    from regnn_hip import mag, ops, synth
    ops.BF16_ROWS["mode"] = args.rows
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
    n_paper = gd["counts"]["paper"]
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    y = torch.full((gd["N"], 1), -1, dtype=torch.int64, device=dev)
    y[:n_paper, 0] = torch.randint(0, 349, (n_paper,), generator=gen, device=dev)
    feats = list(synth.type_features(gd["counts"], {t: 128 for t in synth.NTYPES}, seed=1,
                                     device=dev))
    tables = {}
    if args.only != "bf16":
        tables["fp32"] = {k: f for k, f in enumerate(feats)}
    if args.only != "fp32":
        # (a type at a time: with --only bf16 the fp32 rows of a type go as its copy is made)
        tables["bf16"] = {}
        for k in range(len(feats)):
            tables["bf16"][k] = feats[k].bfloat16().contiguous()
            if args.only == "bf16":
                feats[k] = None
    del feats
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    table_bytes = {k: sum(t.numel() * t.element_size() for t in v.values())
                   for k, v in tables.items()}

    def trainer(x_dict):
        torch.manual_seed(3)
        model = mag.REGNN(128, args.hidden, 349, 2, 10.0, args.dropout, {k: 128 for k in x_dict},
                          7, use_norm="ln", self_loop_type=2, residual=args.residual).to(dev)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        tr = NSTrainer(model, None, rg, [25, 20], args.batch, torch.arange(n_paper, device=dev),
                       x_dict, edge_type, node_type, local, y, 7, seed=123, adam=dict(lr=1e-3),
                       engine="fused" if args.hidden == 64 else "module")
        if args.hidden == 64:
            assert tr.fused.two_layer and tr.fused.W.pre_sums == 1 and tr.adam_fused
        else:
            assert tr.fused is None and tr.slots[0].blocks[-1].pre_sums is not None
        tr.capture(warmup=2)
        torch.cuda.synchronize()
        return tr, torch.cuda.memory_allocated() - base

    trs, added = {}, {}
    for k in (args.first, "bf16" if args.first == "fp32" else "fp32"):
        if k in tables:
            trs[k], added[k] = trainer(tables[k])
    peak = torch.cuda.max_memory_allocated()      # graph + tables + trainer(s), after capture()
    for tr in trs.values():
        tr.run_steps(args.warmup)
    torch.cuda.synchronize()
    us = {k: [] for k in trs}
    for r in range(args.rounds):
        for k, tr in trs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.run_steps(args.steps)
            torch.cuda.synchronize()
            us[k].append((time.perf_counter() - t0) / args.steps * 1e6)
            print(f"round {r} {k}: {us[k][-1]:.2f} us/step", flush=True)
    engine = "fused two-layer step" if args.hidden == 64 else "module path"
    if args.residual:
        engine += ", residual"
    out = {"workload": f"mag_like({args.scale:g}) NS step, batch {args.batch}, fan-out [25, 20], "
                       f"hidden {args.hidden} ({engine}), dropout {args.dropout}, FlatAdam, "
                       "captured",
           "steps_per_window": args.steps, "rounds": args.rounds, "first": args.first,
           "bf16_rows": args.rows,
           "peak_allocated_bytes_after_capture": int(peak)}
    if args.only is None:
        out["every_bf16_round_below_every_fp32_round"] = max(us["bf16"]) < min(us["fp32"])
    for k, v in us.items():
        out[k] = {"us_per_step_median": round(statistics.median(v), 2),
                  "min": round(min(v), 2), "max": round(max(v), 2),
                  "rounds_us": [round(t, 2) for t in v],
                  "table_bytes": table_bytes[k], "trainer_added_bytes": int(added[k]),
                  "final_loss": float(trs[k].loss)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
