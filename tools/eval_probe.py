"""A/B of the native route of `evaluate` (K14s: csrc/eval_metrics.hip, ops.eval_metrics) against the host route (predictions
copied to the host, numpy's log_loss / roc_auc_score / mean_squared_error / accuracy there), in one process on one GPU
(profiles/eval_probe.md).  bench.py's criteo_c2 model (mid vocabulary), batch_size 8192, N = 2^18 and 2^22 rows, metrics
["binary_crossentropy", "auc", "mse", "acc"]:

  (1) `evaluate` end to end, ops.EVAL_NATIVE on against off in alternating blocks: a host clock from a synchronise before the
      call to its return (both routes end in a host read).  On a tree without ops.eval_metrics (the parent commit) only the off
      arm exists and is what is timed.
  (2) the metrics stage alone, on the predictions of (1) kept on the device, each from a synchronise to the host values:
        native   one ops.eval_metrics call and its read-back
        device   the float64 ATen compositions of xdfm_amd/metrics.py (logloss, auc, mse; there is no device accuracy) and
                 their read-back
        host     the copy of the predictions to the host, the widening to float64 and the four numpy functions: what
                 `evaluate` does after the batch loop on the host route
      in alternating order, and the native call's device time between two events.
  The values of the two routes are compared before anything is timed: AUC and accuracy bit for bit.

  python tools/eval_probe.py [--rows 262144,4194304] [--reps 5]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xdeepfm-pytorch_amd"))
sys.path.insert(0, ROOT)

import numpy as np
import torch
from xdfm_amd import ops
from xdfm_amd import metrics as M

dev = torch.device("cuda:0")
NAMES = ["binary_crossentropy", "auc", "mse", "acc"]
BATCH = 8192
HAS_NATIVE = hasattr(ops, "eval_metrics")


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_max_ms": [round(min(ms), 3), round(max(ms), 3)],
            "spread_ms": round(max(ms) - min(ms), 3), "n": len(ms)}


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def alternating(arms, reps):
    """arms: {name: fn}; every block runs each arm once, the order reversed from block to block.  {name: [ms]}."""
    t = {k: [] for k in arms}
    order = list(arms)
    for blk in range(reps):
        for k in (order if blk % 2 == 0 else order[::-1]):
            t[k].append(clocked(arms[k])[0])
    return t


def probe(rows, reps):
    import bench
    cfg = dict(bench.WORKLOADS["criteo_c2"])
    vocab = bench.preset_vocab("mid", cfg["n_sparse"])
    Xf, yf = bench.synthetic_batches(1, rows, vocab, cfg["n_dense"], seed=77)[0]
    torch.manual_seed(0)
    model = bench.build_model(cfg, vocab, dev)
    model.compile("adam", "binary_crossentropy", metrics=NAMES)
    data = {n: Xf[:, i] for i, n in enumerate(model.feature_index.keys())}
    y = np.asarray(yf, np.float32).reshape(-1, 1)

    def evaluate(native):
        def run():
            if HAS_NATIVE:
                ops.EVAL_NATIVE = native
            return model.evaluate(data, y, BATCH)
        return run

    # ---- (1) evaluate end to end; one untimed call per arm first (code objects, the workspace, the allocator's blocks)
    arms = {"off": evaluate(False)}
    if HAS_NATIVE:
        arms["on"] = evaluate(True)
    vals = {k: fn() for k, fn in arms.items()}
    if HAS_NATIVE:
        for k in ("auc", "acc"):
            assert np.float64(vals["on"][k]).tobytes() == np.float64(vals["off"][k]).tobytes(), (k, vals)
        for k in ("binary_crossentropy", "mse"):
            assert abs(vals["on"][k] - vals["off"][k]) <= 2.0 ** -44 * vals["off"][k], (k, vals)
    t = alternating(arms, reps)
    row = {"what": "evaluate end to end, criteo_c2 (mid vocabulary), batch_size %d, N = %d, metrics %s: ms per call, arms alternating"
                   % (BATCH, rows, "+".join(NAMES)), "values_off": vals["off"]}
    for k in t:
        row["EVAL_NATIVE_" + k] = stats(t[k])
    if HAS_NATIVE:
        row["off_minus_on_median_ms"] = round(statistics.median(t["off"]) - statistics.median(t["on"]), 3)
    print(json.dumps(row), flush=True)

    # ---- (2) the metrics stage alone
    model.eval()
    Xd = torch.from_numpy(np.ascontiguousarray(Xf)).float().to(dev)
    with torch.no_grad():
        pred = torch.cat([model(Xd[s:s + BATCH]) for s in range(0, rows, BATCH)])
    del Xd
    yd = torch.from_numpy(y.reshape(-1)).to(dev)
    p1 = pred.reshape(-1)

    def host():
        ph = pred.cpu().data.numpy().astype("float64")
        return [M.log_loss(y, ph), M.roc_auc_score(y, ph), M.mean_squared_error(y, ph), M.accuracy_score(y, np.where(ph > 0.5, 1, 0))]

    def device():
        return torch.stack([M.log_loss_device(yd, p1), M.roc_auc_score_device(yd, p1), M.mean_squared_error_device(yd, p1)]).tolist()

    stage = {"host": host, "device": device}
    if HAS_NATIVE:
        stage["native"] = lambda: ops.eval_metrics(yd, p1, 15).tolist()
    for fn in stage.values():
        fn()
    t = alternating(stage, reps)
    row = {"what": "metrics stage alone, N = %d: ms from a synchronise to the host values (host: copy + widen + 4 numpy functions; "
                   "device: 3 float64 ATen compositions, no accuracy; native: one xdfm_eval_metrics call for all 4)" % rows}
    for k in t:
        row[k] = stats(t[k])
    if HAS_NATIVE:
        ev = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.eval_metrics(yd, p1, 15)
            e1.record()
            torch.cuda.synchronize()
            ev.append(e0.elapsed_time(e1))
        row["native_device_events"] = stats(ev)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="262144,4194304")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    saved = getattr(ops, "EVAL_NATIVE", None)
    try:
        for n in (int(v) for v in args.rows.split(",")):
            probe(n, args.reps)
    finally:
        if saved is not None:
            ops.EVAL_NATIVE = saved
