#!/usr/bin/env python3
"""A/B of the train step with `compile("sgd")` / `compile("adagrad")` (K7s / K7g: native sweep, fused L2 term, marked
gradients, graph replay) against the stock path the same strings took before (a torch.optim.SGD / Adagrad OBJECT handed
to compile: eager launches, K6 value pass, table-sized L2 gradients, zero-filled dense table gradients).

BASELINE config 2's model (bench.py criteo_c2), B = 4096, at the mid (1e5 rows per field) and the Criteo-card
vocabularies.  Both models live in one process and are timed in alternating blocks, every step ending in a device
synchronise, after a warm-up that goes past the graph capture.  Prints one table row per (vocabulary, optimizer):
ms/step of both paths, their ratio, the sweep kernel's bytes per second by the byte model of DESIGN.md (K7s / K7g),
and launches per step (graph nodes for the replayed step; kernels seen by torch.profiler for the eager one).

    python tools/optim_probe.py [--steps 200] [--vocab mid,criteo-card] [--optimizers sgd,adagrad] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "xdeepfm-pytorch_amd"))

import torch                                     # noqa: E402

import bench                                     # noqa: E402


def build(cfg, vocab, dev, optimizer, stock):
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    cols = [SparseFeat("C%d" % (i + 1), v, cfg["emb_dim"]) for i, v in enumerate(vocab)]
    cols += [DenseFeat("I%d" % (i + 1), 1) for i in range(cfg["n_dense"])]
    model = xDeepFM(cols, cols, dnn_hidden_units=cfg["dnn"], cin_layer_size=cfg["cin"], l2_reg_dnn=1e-5, device=dev)
    if stock:
        opt = torch.optim.SGD(model.parameters(), lr=0.01) if optimizer == "sgd" else torch.optim.Adagrad(model.parameters())
        model.compile(opt, "binary_crossentropy", metrics=[])
    else:
        model.compile(optimizer, "binary_crossentropy", metrics=[])
    for pg in model.optim.param_groups:          # a rate at which a sum-reduced loss over 4096 rows stays finite
        pg["lr"] = 1e-5 if optimizer == "sgd" else 1e-3
    model.train()
    return model


def timed(model, batches, steps, k0):
    t0 = time.perf_counter()
    for k in range(steps):
        xb, yb = batches[(k0 + k) % len(batches)]
        model.train_on_batch(xb, yb)
        torch.cuda.synchronize()
    return time.perf_counter() - t0


def eager_launches(model, batches):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for k in range(3):
                model.train_on_batch(*batches[k % len(batches)])
            torch.cuda.synchronize()
        n = sum(e.count for e in prof.key_averages() if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower())
        return round(n / 3.0, 1)
    except Exception as exc:      # noqa: BLE001 -- a figure for the table, not a check
        return "n/a (%s)" % type(exc).__name__


def kernel_rate(model, batches, optimizer):
    """(bytes by the byte model, seconds) of the sweep kernel per step, from HIP events around its launches (eager steps)."""
    from xdfm_amd import ops
    ops.PROFILE = []
    try:
        for k in range(10):
            model.train_on_batch(*batches[k % len(batches)])
        torch.cuda.synchronize()
        rows = [(w, e0.elapsed_time(e1) * 1e-3) for name, w, e0, e1 in ops.PROFILE if name.startswith(optimizer + "_step")]
    finally:
        ops.PROFILE = None
    rows = rows[len(rows) // 2:]
    return sum(w for w, _ in rows) / len(rows), sum(t for _, t in rows) / len(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--block", type=int, default=50, help="steps per alternating block")
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--vocab", default="mid,criteo-card")
    ap.add_argument("--optimizers", default="sgd,adagrad")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = bench.WORKLOADS["criteo_c2"]
    B = cfg["batch"]
    results = []
    for preset in args.vocab.split(","):
        vocab = bench.preset_vocab(preset, cfg["n_sparse"])
        batches = [(torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev))
                   for X, y in bench.synthetic_batches(8, B, vocab, cfg["n_dense"], seed=2025)]
        for optimizer in args.optimizers.split(","):
            new = build(cfg, vocab, dev, optimizer, stock=False)
            old = build(cfg, vocab, dev, optimizer, stock=True)
            for m in (new, old):
                timed(m, batches, args.warmup, 0)
            n_table = sum(t.numel() for t in new._gather_tables())
            t_new = t_old = 0.0
            done = 0
            while done < args.steps:
                n = min(args.block, args.steps - done)
                t_new += timed(new, batches, n, done)
                t_old += timed(old, batches, n, done)
                done += n
            step = new.__dict__["_graphed_step"]
            nodes = [e.nodes for e in step.entries.values() if e.graph is not None]
            launches_old = eager_launches(old, batches)
            nbytes, secs = kernel_rate(new, batches, optimizer)
            row = dict(vocab=preset, table_params=n_table, optimizer=optimizer, steps=args.steps,
                       ms_new=round(t_new / args.steps * 1e3, 4), ms_stock=round(t_old / args.steps * 1e3, 4),
                       speedup=round(t_old / t_new, 3), replays=step.replays, graph_nodes=nodes[0] if nodes else None,
                       launches_stock=launches_old, sweep_bytes=int(nbytes), sweep_us=round(secs * 1e6, 2),
                       sweep_TBps=round(nbytes / secs / 1e12, 3))
            print(json.dumps(row), flush=True)
            results.append(row)
            del new, old, step
            torch.cuda.empty_cache()
    print("| vocabulary | optimizer | new ms/step | stock ms/step | stock / new | sweep us | sweep TB/s | launches new (graph nodes) | launches stock |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in results:
        print("| %s (%.0f M table parameters) | %s | %.3f | %.3f | %.2f | %.1f | %.2f | 1 (%s) | %s |" % (
            r["vocab"], r["table_params"] / 1e6, r["optimizer"], r["ms_new"], r["ms_stock"], r["speedup"], r["sweep_us"],
            r["sweep_TBps"], r["graph_nodes"], r["launches_stock"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
