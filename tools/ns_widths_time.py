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
typed_linear, typed_wgrad) goes into "kernel_us_per_step". A label the step never launched is
absent (with the sampler's pre-sums on, equal widths never launch ns_typed_agg).
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

    def trainer(pipeline):
        torch.manual_seed(3)
        model = mag.REGNN(widths[0], args.hidden, 349, 2, 10.0, args.dropout,
                          dict(enumerate(widths)), 7, use_norm="ln", self_loop_type=2).to(dev)
        model.train()
        tr = NSTrainer(model, None, rg, [25, 20], args.batch,
                       torch.arange(n_paper, device=dev), x_dict, edge_type, node_type, local,
                       y, 7, seed=123, adam=dict(lr=1e-3), engine="module", pipeline=pipeline)
        assert tr.fused is None
        return tr

    legs, errors = {}, {}
    tr_e = trainer(False)
    for _ in range(args.warmup):
        tr_e.step()
    torch.cuda.synchronize()
    legs["eager"] = (tr_e, lambda k: [tr_e.step() for _ in range(k)])
    try:
        if "captured" not in args.legs.split(","):
            raise RuntimeError("leg not asked for (--legs)")
        tr_c = trainer(True)
        tr_c.capture(warmup=2)
        tr_c.run_steps(args.warmup)
        torch.cuda.synchronize()
        legs["captured"] = (tr_c, tr_c.run_steps)
    except Exception as e:                      # noqa: BLE001 (the step cannot be captured)
        torch.cuda.synchronize()
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
    for k, e in errors.items():
        out[k] = {"error": e}
    if args.kernel_steps > 0:
        from regnn_hip import profile
        profile.enable()
        for _ in range(args.kernel_steps):
            tr_e.step()
        torch.cuda.synchronize()
        out["kernel_us_per_step"] = {
            k: round(v[2] * 1e3 / args.kernel_steps, 1)
            for k, v in sorted(profile.summary().items())
            if k in ("ns_typed_agg", "ns_typed_agg_bwd", "typed_linear", "typed_wgrad")}
        profile.enable(False)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
