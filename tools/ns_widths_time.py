"""Per-step time of NS 'regcn' training on the module engine with one input width per node type
(feats_type 5's shape: paper rows 256 wide, the other types 128), in one process:

    python tools/ns_widths_time.py [--scale 1] [--batch 512] [--hidden 512] [--steps 20]
                                   [--rounds 7] [--widths 256,128,128,128]
                                   [--legs eager,captured] [--kernel-steps 0] [--out FILE]

One graph -- mag_like(scale), REGNN 'regcn' hidden 512, LayerNorm, 349 classes, fan-out [25, 20],
dropout 0.5, FlatAdam -- and two trainers over it, built through NSTrainer's public arguments only
(so the same file runs on a checkout of an earlier commit):

  eager     NSTrainer(engine="module", pipeline=False), one step() per step;
  captured  NSTrainer(engine="module") pipelined, capture() and run_steps(). Where the step cannot
            be captured (a host synchronisation in it: group_input's mask per type, the only form
            unequal widths had before ops.typed_linear / ops.ns_typed_agg took them), the leg is
            reported as {"error": ...} and left out of the windows.

After warm-up runs, `rounds` timed windows of `steps` steps each, alternating the legs; a window is
a host clock around the steps ending in a device synchronise. Prints (and with --out writes) one
JSON line: each leg's per-step median, min and max over the rounds (us), and whether the trainer
ran the typed first layer over a meta-only last hop (module_lean).
--kernel-steps K > 0: after the windows, K more eager steps under regnn_hip.profile's event timers;
the device time per step of the typed layer-0 operators (ns_typed_agg, ns_typed_agg_bwd,
typed_linear, typed_wgrad) and of the sampler's sums route (ns_typed_sums, ns_slot_agg,
ns_slot_agg_bwd) goes into "kernel_us_per_step". A label the step never launched is
absent (with the sampler's pre-sums on, equal widths never launch ns_typed_agg).

--sums-kt off[,on[,on-bf16]]: the legs are captured pipelined trainers instead, one per entry, under
ops.NS_SUMS_KT "off" / "on" / "on" with the tables stored in bf16 (the sampler's sums launch at one
width per type); the windows alternate between them, "kernel_us_per_step" is per entry (an eager
trainer each), and every leg reports the device memory its trainer added at its peak
(trainer_peak_mb, on top of what was allocated before it was built; tables_mb: its input tables).
A tree without the knob runs "--sums-kt off" only: the parent's leg of an A/B.
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
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--dropout", type=float, default=0.5)
    ap.add_argument("--widths", default="256,128,128,128")
    ap.add_argument("--legs", default="eager,captured")
    ap.add_argument("--kernel-steps", type=int, default=0)
    ap.add_argument("--sums-kt", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ns_widths_time: needs the GPU (no CPU timing)")
    from regnn_hip import mag, synth
    from regnn_hip.graph import RelGraph
    from regnn_hip.ns import NSTrainer
    dev = "cuda"
    widths = [int(w) for w in args.widths.split(",")]
    gd = synth.mag_like(args.scale, seed=0, device=dev, zipf_s=1.1)
    keep = gd["rel"] <= 7
    rg = RelGraph(gd["src"][keep], gd["dst"][keep], gd["N"], dev)
    edge_type = gd["rel"][keep].to(torch.int64) - 1
    del keep, gd["src"], gd["dst"], gd["rel"]
    node_type = gd["ntype"]
    offs = torch.tensor([gd["type_offsets"][t] for t in synth.NTYPES], device=dev)
    local = torch.arange(gd["N"], device=dev) - offs[node_type]
    feats = synth.type_features(gd["counts"], dict(zip(synth.NTYPES, widths)), seed=1, device=dev)
    x_dict = {k: f for k, f in enumerate(feats)}
    n_paper = gd["counts"]["paper"]
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    y = torch.full((gd["N"], 1), -1, dtype=torch.int64, device=dev)
    y[:n_paper, 0] = torch.randint(0, 349, (n_paper,), generator=gen, device=dev)

    def knob(entry):
        """ops.NS_SUMS_KT for a --sums-kt entry (None: left alone) and the entry's tables"""
        if entry is None:
            return x_dict
        from regnn_hip import ops
        if hasattr(ops, "NS_SUMS_KT"):
            ops.NS_SUMS_KT["mode"] = "off" if entry == "off" else "on"
        elif entry != "off":
            sys.exit("ns_widths_time: this tree has no ops.NS_SUMS_KT (--sums-kt off only)")
        return x_bf16 if entry == "on-bf16" else x_dict

    entries = args.sums_kt.split(",") if args.sums_kt else []
    if any(e not in ("off", "on", "on-bf16") for e in entries):
        sys.exit("ns_widths_time: --sums-kt takes off, on, on-bf16")
    x_bf16 = ({k: v.bfloat16().contiguous() for k, v in x_dict.items()}
              if "on-bf16" in entries else None)

    def trainer(pipeline, entry=None):
        x_dict = knob(entry)
        torch.manual_seed(3)
        model = mag.REGNN(widths[0], args.hidden, 349, 2, 10.0, args.dropout,
                          dict(enumerate(widths)), 7, use_norm="ln", self_loop_type=2).to(dev)
        model.train()
        tr = NSTrainer(model, None, rg, [25, 20], args.batch,
                       torch.arange(n_paper, device=dev), x_dict, edge_type, node_type, local,
                       y, 7, seed=123, adam=dict(lr=1e-3), engine="module", pipeline=pipeline)
        assert tr.fused is None
        return tr

    legs, errors, mem = {}, {}, {}
    mb = lambda b: round(b / 2 ** 20, 1)          # noqa: E731
    for e in entries:
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        tr = trainer(True, e)
        tr.capture(warmup=2)
        tr.run_steps(args.warmup)
        torch.cuda.synchronize()
        tabs = x_bf16 if e == "on-bf16" else x_dict
        mem["kt_" + e] = {"trainer_peak_mb": mb(torch.cuda.max_memory_allocated() - base),
                          "tables_mb": mb(sum(t.numel() * t.element_size()
                                              for t in tabs.values())),
                          "pre_sums": getattr(tr.slots[0].blocks[-1], "pre_sums", None)
                          is not None}
        legs["kt_" + e] = (tr, tr.run_steps)
    tr_e = None
    if not entries:
        tr_e = trainer(False)
        for _ in range(args.warmup):
            tr_e.step()
        torch.cuda.synchronize()
        legs["eager"] = (tr_e, lambda k: [tr_e.step() for _ in range(k)])
    try:
        if "captured" not in args.legs.split(",") or entries:
            raise RuntimeError("leg not asked for (--legs)")
        tr_c = trainer(True)
        tr_c.capture(warmup=2)
        tr_c.run_steps(args.warmup)
        torch.cuda.synchronize()
        legs["captured"] = (tr_c, tr_c.run_steps)
    except Exception as e:                      # noqa: BLE001 (the step cannot be captured)
        torch.cuda.synchronize()
        if not entries:
            errors["captured"] = f"{type(e).__name__}: {e}".splitlines()[0][:200]
    us = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, (_tr, run) in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(args.steps)
            torch.cuda.synchronize()
            us[k].append((time.perf_counter() - t0) / args.steps * 1e6)
    out = {"workload": f"mag_like({args.scale:g}) NS step, regcn hidden {args.hidden}, LayerNorm, "
                       f"input widths {widths}, batch {args.batch}, fan-out [25, 20], dropout "
                       f"{args.dropout}, FlatAdam, module engine",
           "steps_per_window": args.steps, "rounds": args.rounds}
    for k, v in us.items():
        tr = legs[k][0]
        out[k] = {"us_per_step_median": round(statistics.median(v), 1),
                  "min": round(min(v), 1), "max": round(max(v), 1),
                  "final_loss": float(tr.loss),
                  "module_lean": bool(getattr(tr, "_module_lean", False))}
        out[k].update(mem.get(k, {}))
    for k, e in errors.items():
        out[k] = {"error": e}
    labels = ("ns_typed_agg", "ns_typed_agg_bwd", "typed_linear", "typed_wgrad", "ns_typed_sums",
              "ns_slot_agg", "ns_slot_agg_bwd")

    def kernel_us(tr):
        """device time per step of the layer-0 operators over kernel_steps eager steps"""
        from regnn_hip import profile
        profile.enable()
        for _ in range(args.kernel_steps):
            tr.step()
        torch.cuda.synchronize()
        res = {k: round(v[2] * 1e3 / args.kernel_steps, 1)
               for k, v in sorted(profile.summary().items()) if k in labels}
        profile.enable(False)
        return res

    if args.kernel_steps > 0 and tr_e is not None:
        out["kernel_us_per_step"] = kernel_us(tr_e)
    for e in entries if args.kernel_steps > 0 else []:
        tr = trainer(False, e)
        for _ in range(args.warmup):
            tr.step()
        torch.cuda.synchronize()
        out["kt_" + e]["kernel_us_per_step"] = kernel_us(tr)
        del tr
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
