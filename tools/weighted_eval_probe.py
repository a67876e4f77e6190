"""What the weighted metrics (K14w: csrc/eval_metrics_w.hip, ops.eval_metrics_w, compile(weighted_metrics=...)) cost, in one
process on one GPU (profiles/weighted_eval_probe.md).  bench.py's criteo_c2 model (mid vocabulary); every comparison with its
arms alternating, median [min, max] per arm, one JSON line each:

  (1) kernel   xdfm_eval_metrics_w with unit weights against xdfm_eval_metrics on the same rows, all four metrics, between
               device events: the cost of the payload in the sort and of the `cum` scan.  N = 4096, 2^18, 2^22.  The four
               values of the two calls are compared bit for bit first.
  (2) evaluate `evaluate(sample_weight=)` on a model compiled with metrics and weighted_metrics of the same four names,
               ops.EVAL_W_NATIVE on against off: a host clock from a synchronise before the call to its return.  2^18 and 2^22
               rows, batch_size 8192.
  (3) fit      ms per step of fit(verbose=2, sample_weight=...), batch_size 4096, metrics [logloss, auc]: (a) alone, (b) with
               weighted_metrics of the same names, (c) as (b) with ops.EVAL_W_NATIVE off.

  python tools/weighted_eval_probe.py [--reps 7] [--skip kernel,evaluate,fit]"""
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

dev = torch.device("cuda:0")
NAMES = ["binary_crossentropy", "auc", "mse", "acc"]


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_max_ms": [round(min(ms), 4), round(max(ms), 4)],
            "spread_ms": round(max(ms) - min(ms), 4), "n": len(ms)}


def alternating(arms, reps, timer):
    """arms: {name: fn}; every block runs each arm once, the order reversed from block to block.  {name: [ms]}."""
    t = {k: [] for k in arms}
    order = list(arms)
    for blk in range(reps):
        for k in (order if blk % 2 == 0 else order[::-1]):
            t[k].append(timer(arms[k]))
    return t


def by_events(fn, inner=5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def by_clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def kernel(reps):
    for N in (4096, 1 << 18, 1 << 22):
        rng = np.random.default_rng(N)
        y = torch.from_numpy((rng.random(N) < 0.3).astype(np.float32)).to(dev)
        p = torch.from_numpy(rng.random(N).astype(np.float32)).to(dev)
        w = torch.ones(N, dtype=torch.float32, device=dev)
        arms = {"eval_metrics": lambda: ops.eval_metrics(y, p, 15), "eval_metrics_w": lambda: ops.eval_metrics_w(y, p, w, 15)}
        a, b = (fn().cpu().numpy() for fn in arms.values())
        assert a.tobytes() == b.tobytes(), (N, a, b)
        t = alternating(arms, reps, by_events)
        row = {"what": "kernel: all four metrics of N = %d rows, unit weights, ms per call between device events (5 calls per "
                       "sample), arms alternating" % N, "values": a.tolist()}
        row.update({k: stats(v) for k, v in t.items()})
        row["w_over_unweighted"] = round(statistics.median(t["eval_metrics_w"]) / statistics.median(t["eval_metrics"]), 3)
        print(json.dumps(row), flush=True)


def _criteo(rows, seed):
    import bench
    cfg = dict(bench.WORKLOADS["criteo_c2"])
    vocab = bench.preset_vocab("mid", cfg["n_sparse"])
    Xf, yf = bench.synthetic_batches(1, rows, vocab, cfg["n_dense"], seed=seed)[0]
    torch.manual_seed(0)
    model = bench.build_model(cfg, vocab, dev)
    data = {n: Xf[:, i] for i, n in enumerate(model.feature_index.keys())}
    y = np.asarray(yf, np.float32).reshape(-1, 1)
    w = (np.random.default_rng(seed).integers(1, 17, rows) / 4.0).astype(np.float32)
    return model, data, y, w


def evaluate(reps):
    for rows in (1 << 18, 1 << 22):
        model, data, y, w = _criteo(rows, 77)
        model.compile("adam", "binary_crossentropy", metrics=NAMES, weighted_metrics=NAMES)

        def arm(native):
            def run():
                ops.EVAL_W_NATIVE = native
                return model.evaluate(data, y, 8192, sample_weight=w)
            return run
        arms = {"off": arm(False), "on": arm(True)}
        vals = {k: fn() for k, fn in arms.items()}
        for k in ("weighted_auc", "weighted_acc"):
            assert np.float64(vals["on"][k]).tobytes() == np.float64(vals["off"][k]).tobytes(), (k, vals)
        t = alternating(arms, reps, by_clock)
        row = {"what": "evaluate(sample_weight=) end to end, criteo_c2 (mid vocabulary), batch_size 8192, N = %d, metrics and "
                       "weighted_metrics %s: ms per call, arms alternating" % (rows, "+".join(NAMES)), "values_on": vals["on"]}
        row.update({"EVAL_W_NATIVE_" + k: stats(v) for k, v in t.items()})
        row["off_minus_on_median_ms"] = round(statistics.median(t["off"]) - statistics.median(t["on"]), 3)
        print(json.dumps(row), flush=True)
        del model


def fit(reps):
    rows, batch = 1 << 17, 4096
    steps = rows // batch
    model, data, y, w = _criteo(rows, 78)
    names = ["binary_crossentropy", "auc"]

    def epoch():
        model.fit(data, y, batch_size=batch, epochs=1, verbose=2, shuffle=False, sample_weight=w)
    # one model, compiled anew for every sample (compile makes a new optimizer), one untimed epoch after each compile
    order = [("a_metrics_alone", None, True), ("b_weighted_native", names, True), ("c_weighted_host", names, False)]
    t = {k: [] for k, _, _ in order}
    for blk in range(reps):
        for k, weighted, native in (order if blk % 2 == 0 else order[::-1]):
            model.compile("adam", "binary_crossentropy", metrics=names, weighted_metrics=weighted)
            ops.EVAL_W_NATIVE = native
            epoch()
            t[k].append(by_clock(epoch) / steps)
    row = {"what": "fit(verbose=2, sample_weight=), criteo_c2 (mid vocabulary), batch_size %d, %d steps per epoch, metrics %s: ms per "
                   "step of one epoch (host clock, epoch-end reads included), arms alternating; (b) and (c) add weighted_metrics of "
                   "the same names" % (batch, steps, "+".join(names))}
    row.update({k: stats(v) for k, v in t.items()})
    row["b_minus_a_median_ms"] = round(statistics.median(t["b_weighted_native"]) - statistics.median(t["a_metrics_alone"]), 4)
    row["c_minus_a_median_ms"] = round(statistics.median(t["c_weighted_host"]) - statistics.median(t["a_metrics_alone"]), 4)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip", default="")
    args = ap.parse_args()
    saved = ops.EVAL_W_NATIVE
    try:
        for name, fn in (("kernel", kernel), ("evaluate", evaluate), ("fit", fit)):
            if name not in args.skip.split(","):
                fn(args.reps)
    finally:
        ops.EVAL_W_NATIVE = saved
