"""A/B of the native batch metrics (K14: csrc/metrics.hip, ops.batch_metrics) against the float64 device compositions of
xdfm_amd/metrics.py (*_device) that `fit(verbose > 0)` ran per step before, in one process on one GPU
(profiles/metrics_probe.md):

  python tools/metrics_probe.py           (1) one call for LOGLOSS | AUC and for all four metrics at B = 4096 and B = 32768, each
                                              arm captured into a HIP graph of CALLS back-to-back calls (kernel time, no host
                                              launch gaps), the arms' graphs replayed in alternating blocks between device
                                              events; the stock arm has no device accuracy, so its "all four" is its three
                                          (2) the launches of one call of each arm: the nodes of a graph that holds one call
                                          (3) `fit` on bench.py's criteo_c2 model (1e5 rows per field) with
                                              metrics=["binary_crossentropy", "auc"], verbose=2, 64 steps per epoch: one fit
                                              call whose epochs alternate ops.METRICS_NATIVE on / off (the loop reads the switch
                                              every step), a host clock from a synchronise at the epoch's start to one after
                                              its read-back
                                          (4) the same fit with metrics=[]: the floor
  python tools/metrics_probe.py --no-fit  (1) and (2) only"""
import contextlib
import io
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
from xdfm_amd import graphstep, ops
from xdfm_amd import metrics as M
from xdfm_amd.callbacks import Callback

dev = torch.device("cuda:0")
CALLS, BLOCKS, REPLAYS = 20, 10, 10
EPOCH_PAIRS, STEPS_PER_EPOCH = 8, 64
STOCK = {1: M.log_loss_device, 2: M.roc_auc_score_device, 4: M.mean_squared_error_device}


def graph_of(fn, calls, keep=False):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True) if keep else torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    return g


def us_per_call(g):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPLAYS):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (REPLAYS * CALLS)


def summary(t, unit, nd=2):
    return {"native_median_" + unit: round(statistics.median(t[True]), nd), "stock_median_" + unit: round(statistics.median(t[False]), nd),
            "native_min_max_" + unit: [round(min(t[True]), nd), round(max(t[True]), nd)],
            "stock_min_max_" + unit: [round(min(t[False]), nd), round(max(t[False]), nd)],
            "spread_" + unit: round(max(max(v) - min(v) for v in t.values()), nd)}


def call_arm(native, y, p, which, log):
    """One step's metrics as `fit` forms them: into a row of a float64 log, nothing read back."""
    if native:
        return lambda: ops.batch_metrics(y, p, which, log[0])

    def stock():
        for k, bit in enumerate((1, 2, 4)):
            if which & bit:
                log[0, k:k + 1].copy_(STOCK[bit](y, p).reshape(1))
    return stock


def calls_ab():
    rng = np.random.default_rng(0)
    for B in (4096, 32768):
        y = torch.from_numpy((rng.random(B) < 0.25).astype(np.float32)).to(dev).reshape(B, 1)
        p = torch.from_numpy(rng.random(B).astype(np.float32)).to(dev)
        log = torch.zeros((2, 4), dtype=torch.float64, device=dev)
        for which, label in ((3, "logloss | auc"), (15, "all four (stock arm: logloss, auc, mse; it has no device accuracy)")):
            graphs = {n: graph_of(call_arm(n, y, p, which, log), CALLS) for n in (True, False)}
            launches = {n: graphstep.census(graph_of(call_arm(n, y, p, which, log), 1, keep=True)) for n in (True, False)}
            t = {True: [], False: []}
            for blk in range(BLOCKS):
                for n in ((True, False) if blk % 2 == 0 else (False, True)):
                    t[n].append(us_per_call(graphs[n]))
            row = {"what": "one call, B = %d, %s" % (B, label)}
            row.update(summary(t, "us"))
            row["launches (memset nodes)"] = {"native": "%d (%d)" % launches[True][:2], "stock": "%d (%d)" % launches[False][:2]}
            print(json.dumps(row), flush=True)


class EpochClock(Callback):
    """Sets ops.METRICS_NATIVE for the epoch (arms[epoch]; None leaves it) and times it between two synchronises."""

    def __init__(self, arms):
        super().__init__()
        self.arms, self.times = arms, []

    def on_epoch_begin(self, epoch, logs=None):
        if self.arms[epoch] is not None:
            ops.METRICS_NATIVE = self.arms[epoch]
        torch.cuda.synchronize()
        self.t0 = time.perf_counter()

    def on_epoch_end(self, epoch, logs=None):
        torch.cuda.synchronize()
        self.times.append((self.arms[epoch], time.perf_counter() - self.t0))


def fit_ab():
    import bench
    cfg = dict(bench.WORKLOADS["criteo_c2"])
    B = cfg["batch"]
    vocab = bench.preset_vocab("mid", cfg["n_sparse"])
    Xf, yf = bench.synthetic_batches(1, STEPS_PER_EPOCH * B, vocab, cfg["n_dense"], seed=77)[0]

    def epochs_of(metrics, arms):
        torch.manual_seed(0)
        model = bench.build_model(cfg, vocab, dev)
        model.compile("adam", "binary_crossentropy", metrics=metrics)
        data = {n: Xf[:, i] for i, n in enumerate(model.feature_index.keys())}
        clock = EpochClock(arms)
        with contextlib.redirect_stdout(io.StringIO()):
            model.fit(data, yf, batch_size=B, epochs=len(arms), verbose=2, shuffle=False, callbacks=[clock])
        return clock.times[2:]                                # the first two epochs (eager steps, the capture) are warm-up

    arms = [True, False] + [a for k in range(EPOCH_PAIRS) for a in ((True, False) if k % 2 == 0 else (False, True))]
    times = epochs_of(["binary_crossentropy", "auc"], arms)
    t = {n: [1e3 * s / STEPS_PER_EPOCH for a, s in times if a is n] for n in (True, False)}
    row = {"what": "fit, criteo_c2 (1e5-row tables), batch %d, %d steps per epoch, metrics logloss + auc, verbose=2: ms per step, "
                   "epochs alternating" % (B, STEPS_PER_EPOCH)}
    row.update(summary(t, "ms", 4))
    print(json.dumps(row), flush=True)
    floor = [1e3 * s / STEPS_PER_EPOCH for _, s in epochs_of([], [None] * (2 + EPOCH_PAIRS))]
    print(json.dumps({"what": "the same fit with metrics=[] (the floor): ms per step", "median_ms": round(statistics.median(floor), 3),
                      "min_max_ms": [round(min(floor), 3), round(max(floor), 3)]}), flush=True)


saved = ops.METRICS_NATIVE
try:
    calls_ab()
    if "--no-fit" not in sys.argv:
        fit_ab()
finally:
    ops.METRICS_NATIVE = saved
