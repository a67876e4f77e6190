#!/usr/bin/env python3
"""A/B of the train step with `compile("sgd")` / `compile("adagrad")` / `compile("rmsprop")` (K7s / K7g / K7r; K7m with --momentum: native sweep,
fused L2 term, marked gradients, graph replay) against the stock path the same strings took before (a torch.optim.SGD /
Adagrad / RMSprop OBJECT handed
to compile: eager launches, K6 value pass, table-sized L2 gradients, zero-filled dense table gradients).

BASELINE config 2's model (bench.py criteo_c2), B = 4096, at the mid (1e5 rows per field) and the Criteo-card
vocabularies.  Both models live in one process and are timed in alternating blocks, every step ending in a device
synchronise, after a warm-up that goes past the graph capture.  Prints one table row per (vocabulary, optimizer):
ms/step of both paths, their ratio, the sweep kernel's bytes per second by the byte model of DESIGN.md (K7s / K7g),
and launches per step (graph nodes for the replayed step; kernels seen by torch.profiler for the eager one).

A third arm, `deferred`, is the native step with the deferred (exact) table update (K7sd / K7gd / K7rd, `deferred=True`) beside
the native sweep (`deferred=False`).  Its timed blocks end with a flush inside the timed region, and a block is longer than
the flush period, so every deferred update is paid for inside the time reported.  For that arm the tool also prints the
flush (ms per flush, and amortised over the period) and the catch-up launch (us), from HIP events around them.

With `--momentum MU` (and `--nesterov`), `sgd` is SGD with momentum (K7m / K7md): every arm builds
xdfm_amd.optim.TableSGD(momentum=MU) and hands the object to compile; `sweep` and `deferred` run with XDFM_SGD_MOMENTUM_NATIVE on,
`stock` with it off -- the fallback the class took before (flush, the L2 term by hand, torch.optim.SGD.step over dense
gradients).  The switch is a module attribute that is set in front of every block.

`--optimizer ftrl` is xdfm_amd.optim.TableFTRL (K7f): `sweep` is its kernel, `stock` the same class on its torch-op step; it
has no deferred arm.  Its two configurations: the model's default L2 on the tables (every element is updated, 24 B per
parameter), and `--no_table_l2` (l2_reg_embedding = l2_reg_linear = 0 with FTRL's own l2: the step reads the marks and the
batch's rows).  `--optimizers ftrl,adagrad` puts the native Adagrad step on the same model beside it.

`--optimizer rowwise_adagrad` is xdfm_amd.optim.TableRowwiseAdagrad (K7w for the tables, K7g for the rest): `sweep` is its
kernels, `stock` the same class on its torch-op step, and a further arm, `adagrad`, is the native Adagrad step
(compile("adagrad")) at its own best path -- deferred where "auto" chooses it -- timed in the same alternating blocks.  No
deferred arm.  With the model's default L2 on the tables every row is updated (8 + 8 / D bytes per parameter); with
`--no_table_l2` the step reads the marks and the batch's rows.  Every row also reports the bytes of optimizer state.

    python tools/optim_probe.py [--steps 256] [--vocab mid,criteo-card] [--optimizers sgd,adagrad,rmsprop,ftrl,rowwise_adagrad] [--arms sweep,deferred,stock,adagrad]
                                [--momentum 0.9 [--nesterov]] [--no_table_l2] [--out FILE.json]
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


def route(model):
    """The route a model of this probe takes through TableSGD with a momentum: set in front of everything that steps it."""
    from xdfm_amd import optim
    optim.SGD_MOMENTUM_NATIVE = getattr(model, "_probe_native", True)


def build(cfg, vocab, dev, optimizer, stock, deferred=False, momentum=0.0, nesterov=False, no_table_l2=False, auto=False):
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    cols = [SparseFeat("C%d" % (i + 1), v, cfg["emb_dim"]) for i, v in enumerate(vocab)]
    cols += [DenseFeat("I%d" % (i + 1), 1) for i in range(cfg["n_dense"])]
    l2_kw = dict(l2_reg_embedding=0.0, l2_reg_linear=0.0) if no_table_l2 else {}
    model = xDeepFM(cols, cols, dnn_hidden_units=cfg["dnn"], cin_layer_size=cfg["cin"], l2_reg_dnn=1e-5, device=dev, **l2_kw)
    if optimizer == "ftrl":
        # `sweep`: K7f; `stock`: the same class sent down its torch-op step.  With --no_table_l2 FTRL's own (proximal) l2 stands
        # in for the model's L2 on the tables: the recommended configuration, whose cost follows the batch
        from xdfm_amd.optim import TableFTRL
        opt = TableFTRL(model.parameters(), lr=1e-3, l2=1e-3 if no_table_l2 else 0.0)
        model.compile(opt, "binary_crossentropy", metrics=[])
        if stock:
            opt._native = lambda: False
    elif optimizer == "rowwise_adagrad":
        # `sweep`: K7w + K7g; `stock`: the same class sent down its torch-op step
        model.compile("rowwise_adagrad", "binary_crossentropy", metrics=[])
        if stock:
            model.optim._native = lambda: False
    elif optimizer == "sgd" and momentum:
        from xdfm_amd.optim import TableSGD
        opt = TableSGD(model.parameters(), lr=0.01, momentum=momentum, nesterov=nesterov, deferred=bool(deferred))
        model.compile(opt, "binary_crossentropy", metrics=[])
        model._probe_native = not stock
    elif stock:
        opt = {"sgd": lambda p: torch.optim.SGD(p, lr=0.01), "adagrad": torch.optim.Adagrad,
               "rmsprop": torch.optim.RMSprop}[optimizer](model.parameters())
        model.compile(opt, "binary_crossentropy", metrics=[])
    else:
        model.compile(optimizer, "binary_crossentropy", metrics=[])
        if not auto:                             # (auto: the class's own choice, "auto" unless the environment says otherwise)
            model.optim.deferred = bool(deferred)
    for pg in model.optim.param_groups:          # a rate at which a sum-reduced loss over 4096 rows stays finite
        pg["lr"] = {"sgd": 1e-5 * (1.0 - momentum), "adagrad": 1e-3, "rmsprop": 1e-4, "ftrl": 1e-3, "rowwise_adagrad": 1e-3}[optimizer]
    model.train()
    return model


def timed(model, batches, steps, k0):
    route(model)
    t0 = time.perf_counter()
    for k in range(steps):
        xb, yb = batches[(k0 + k) % len(batches)]
        model.train_on_batch(xb, yb)
        torch.cuda.synchronize()
    if hasattr(model.optim, "flush"):            # deferred arm: what the block still owes is paid inside it
        model.optim.flush()
        torch.cuda.synchronize()
    return time.perf_counter() - t0


def deferred_parts(model, batches, reps=3):
    """(ms per flush after a full period of steps, us per catch-up launch) of a model on the deferred path, by HIP events."""
    route(model)
    opt = model.optim
    plan = model._gather_plan()
    flush_ms, catch_us = [], []
    k = 0
    for _ in range(reps):
        opt.flush()
        while opt._since < opt.flush_every:
            model.train_on_batch(*batches[k % len(batches)])
            k += 1
            if opt._since == opt.flush_every // 2:          # rows of a fresh batch, half a period behind
                X, emb, lin = plan.last_gather
                Xn = batches[(k + 3) % len(batches)][0]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                opt._catchup(plan, Xn, emb, lin)
                e1.record()
                torch.cuda.synchronize()
                catch_us.append(e0.elapsed_time(e1) * 1e3)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        opt.flush()
        e1.record()
        torch.cuda.synchronize()
        flush_ms.append(e0.elapsed_time(e1))
    return sorted(flush_ms)[len(flush_ms) // 2], sorted(catch_us)[len(catch_us) // 2]


def eager_launches(model, batches):
    route(model)
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
    route(model)
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
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--block", type=int, default=128, help="steps per alternating block (longer than the flush period)")
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--vocab", default="mid,criteo-card")
    ap.add_argument("--optimizers", "--optimizer", dest="optimizers", default="sgd,adagrad,rmsprop")
    ap.add_argument("--momentum", type=float, default=0.0, help="sgd only: SGD with this momentum, in (0, 1) (K7m)")
    ap.add_argument("--nesterov", action="store_true", help="with --momentum: Nesterov momentum")
    ap.add_argument("--arms", default="sweep,deferred,stock")
    ap.add_argument("--no_table_l2", action="store_true",
                    help="build the models with l2_reg_embedding = l2_reg_linear = 0 (ftrl: its own l2 = 1e-3 in their place)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if (args.momentum or args.nesterov) and args.optimizers != "sgd":
        ap.error("--momentum / --nesterov need --optimizer sgd")
    if not 0.0 <= args.momentum < 1.0 or (args.nesterov and not args.momentum):
        ap.error("--momentum must be in [0, 1), and --nesterov needs one above 0")
    dev = torch.device("cuda:0")
    cfg = bench.WORKLOADS["criteo_c2"]
    B = cfg["batch"]
    arms = args.arms.split(",")
    results = []
    for preset in args.vocab.split(","):
        vocab = bench.preset_vocab(preset, cfg["n_sparse"])
        batches = [(torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev))
                   for X, y in bench.synthetic_batches(8, B, vocab, cfg["n_dense"], seed=2025)]
        for optimizer in args.optimizers.split(","):
            # FTRL and row-wise Adagrad have no deferred form; the `adagrad` arm stands beside row-wise Adagrad only
            arms = [a for a in args.arms.split(",") if not (optimizer in ("ftrl", "rowwise_adagrad") and a == "deferred")
                    and not (optimizer != "rowwise_adagrad" and a == "adagrad")]
            models = {a: build(cfg, vocab, dev, "adagrad" if a == "adagrad" else optimizer, stock=a == "stock",
                               deferred=a == "deferred", momentum=args.momentum, nesterov=args.nesterov,
                               no_table_l2=args.no_table_l2, auto=a == "adagrad") for a in arms}
            kernel = "sgdm" if optimizer == "sgd" and args.momentum else "rowwise" if optimizer == "rowwise_adagrad" else optimizer
            for m in models.values():
                timed(m, batches, args.warmup, 0)
            native = models.get("sweep", models.get("deferred"))
            n_table = sum(t.numel() for t in native._gather_tables()) if native is not None else 0
            secs = {a: 0.0 for a in arms}
            blocks = {a: [] for a in arms}
            done = 0
            while done < args.steps:
                n = min(args.block, args.steps - done)
                for a in arms:
                    dt = timed(models[a], batches, n, done)
                    secs[a] += dt
                    blocks[a].append(round(dt / n * 1e3, 4))
                done += n
            row = dict(vocab=preset, table_params=n_table, optimizer=optimizer, steps=args.steps, block=args.block,
                       table_l2=not args.no_table_l2)
            if args.momentum:
                row.update(momentum=args.momentum, nesterov=args.nesterov)
            for a in arms:
                row["ms_" + a] = round(secs[a] / args.steps * 1e3, 4)
                row["ms_blocks_" + a] = blocks[a]            # per alternating block: the spread
            if "sweep" in models:
                step = models["sweep"].__dict__["_graphed_step"]
                nodes = [e.nodes for e in step.entries.values() if e.graph is not None]
                if "stock" in models and args.momentum:
                    st = models["stock"].__dict__.get("_graphed_step")
                    row["graph_nodes_stock"] = ([e.nodes for e in st.entries.values() if e.graph is not None] or [None])[0] if st else None
                    row["replays_stock"] = st.replays if st else 0
                nbytes, ksecs = kernel_rate(models["sweep"], batches, kernel)
                row.update(replays=step.replays, graph_nodes=nodes[0] if nodes else None, sweep_bytes=int(nbytes),
                           sweep_us=round(ksecs * 1e6, 2), sweep_TBps=round(nbytes / ksecs / 1e12, 3))
            for a in arms:                               # bytes of optimizer state (after the steps that created it)
                if a != "stock":
                    row["state_bytes_" + a] = sum(v.numel() * v.element_size() for st in models[a].optim.state.values()
                                                  for v in st.values() if torch.is_tensor(v) and v.is_cuda)
            if "adagrad" in models:
                opt = models["adagrad"].optim
                row["adagrad_deferred_steps"] = opt.path_counts["scan"]
                nbytes, ksecs = kernel_rate(models["adagrad"], batches, "adagrad")
                row.update(adagrad_step_bytes=int(nbytes), adagrad_step_us=round(ksecs * 1e6, 2))
                opt.flush()
            if "stock" in models:
                row["launches_stock"] = eager_launches(models["stock"], batches)
                if "sweep" in models:
                    row["speedup"] = round(secs["stock"] / secs["sweep"], 3)
            if "deferred" in models:
                opt = models["deferred"].optim
                flush_ms, catch_us = deferred_parts(models["deferred"], batches)
                nbytes, ksecs = kernel_rate(models["deferred"], batches, kernel)
                opt.flush()
                row.update(flush_every=opt.flush_every, deferred_steps=opt.path_counts["scan"], flush_ms=round(flush_ms, 3),
                           flush_ms_per_step=round(flush_ms / opt.flush_every, 4), catchup_us=round(catch_us, 1),
                           scan_us=round(ksecs * 1e6, 2))
            print(json.dumps(row), flush=True)
            results.append(row)
            del models, native
            torch.cuda.empty_cache()
    g = lambda r, k, f="%.3f": (f % r[k]) if isinstance(r.get(k), (int, float)) else "-"
    print("| vocabulary | optimizer | sweep ms/step | deferred ms/step | stock ms/step | stock / sweep | flush ms | flush ms/step | catch-up us | step scan us | sweep us | sweep TB/s | launches sweep (graph nodes) | launches stock |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in results:
        print("| %s (%.0f M table parameters) | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s | 1 (%s) | %s |" % (
            r["vocab"], r["table_params"] / 1e6, r["optimizer"], g(r, "ms_sweep"), g(r, "ms_deferred"), g(r, "ms_stock"),
            g(r, "speedup", "%.2f"), g(r, "flush_ms"), g(r, "flush_ms_per_step"), g(r, "catchup_us", "%.1f"), g(r, "scan_us", "%.1f"),
            g(r, "sweep_us", "%.1f"), g(r, "sweep_TBps", "%.2f"), r.get("graph_nodes", "-"), r.get("launches_stock", "-")))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
