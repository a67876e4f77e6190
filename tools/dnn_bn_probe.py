"""A/B of the native batch norm of the DNN tower (csrc/bn.hip, ops.bn_act) against the stock sequence (nn.BatchNorm1d + torch.relu),
in one process on one GPU, with ops.DNN_BN_NATIVE flipped between the arms:

  python tools/dnn_bn_probe.py            one layer forward + backward (ops.dense -> batch norm -> relu, through autograd) at the two
                                          layers of the flagship tower, batch 4096: 429 -> 256 and 256 -> 256 -- time and launches;
                                          then bench.py's criteo_c2 train step with dnn_use_bn=True, replayed from its captured
                                          graph -- time and node count (profiles/dnn_bn_probe.md)
  python tools/dnn_bn_probe.py --rows N   another batch size

Time: every layer arm is captured into a HIP graph of CALLS back-to-back passes (kernel time, no host launch gaps); the arms'
graphs are replayed in alternating blocks between device events.  Launches: the nodes of a graph that holds one pass."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xdeepfm-pytorch_amd"))
sys.path.insert(0, ROOT)

import torch
from xdfm_amd import graphstep, ops

dev = torch.device("cuda:0")
ROWS = int(sys.argv[sys.argv.index("--rows") + 1]) if "--rows" in sys.argv else 4096
LAYERS = [(429, 256), (256, 256)]
CALLS, BLOCKS, REPLAYS, STEPS = 20, 10, 10, 20


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


def layer_pass(x, lin, bn, g, native):
    ops.DNN_BN_NATIVE = native
    a = x.detach().requires_grad_(True)
    for p in list(lin.parameters()) + list(bn.parameters()):
        p.grad = None
    z = ops.dense(a, lin.weight, lin.bias)
    if native:
        assert ops.bn_native(z, bn)
    ops.bn_act(z, bn, "relu", True).backward(g)


def summary(t):
    return {"native_median_us": round(statistics.median(t[True]), 2), "stock_median_us": round(statistics.median(t[False]), 2),
            "native_min_max_us": [round(min(t[True]), 2), round(max(t[True]), 2)],
            "stock_min_max_us": [round(min(t[False]), 2), round(max(t[False]), 2)],
            "spread_us": round(max(max(v) - min(v) for v in t.values()), 2)}


def step_model(native):
    """bench.py's criteo_c2 model (1e5 rows per table: the tower does not see the tables) with dnn_use_bn=True, its train step
    captured with ops.DNN_BN_NATIVE = native."""
    import bench
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    cfg = dict(bench.WORKLOADS["criteo_c2"])
    vocab = bench.preset_vocab("mid", cfg["n_sparse"])
    cols = [SparseFeat("C%d" % (i + 1), v, cfg["emb_dim"]) for i, v in enumerate(vocab)]
    cols += [DenseFeat("I%d" % (i + 1), 1) for i in range(cfg["n_dense"])]
    torch.manual_seed(0)
    model = xDeepFM(cols, cols, dnn_hidden_units=cfg["dnn"], cin_layer_size=cfg["cin"], l2_reg_dnn=1e-5, dnn_use_bn=True, device=dev)
    model.compile("adam", "binary_crossentropy", metrics=[])
    model.train()
    step = model.__dict__["_graphed_step"] = graphstep.GraphedStep(model)
    batches = [(torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev))
               for X, y in bench.synthetic_batches(4, ROWS, vocab, cfg["n_dense"], seed=1)]
    ops.DNN_BN_NATIVE = native
    for i in range(5):                                   # two eager steps, the capture, two replays
        model.train_on_batch(*batches[i % len(batches)])
    torch.cuda.synchronize()
    nodes = [e.nodes for e in step.entries.values() if e.graph is not None]
    assert step.replays >= 2 and not step.disabled and len(nodes) == 1, (step.replays, step.disabled, nodes)
    return model, batches, nodes[0]


saved = ops.DNN_BN_NATIVE
try:
    torch.manual_seed(0)
    for k, out in LAYERS:
        x = torch.randn(ROWS, k, device=dev)
        lin = torch.nn.Linear(k, out).to(dev)
        bn = torch.nn.BatchNorm1d(out).to(dev).train()
        g = torch.randn(ROWS, out, device=dev)
        graphs = {native: graph_of(lambda native=native: layer_pass(x, lin, bn, g, native), CALLS) for native in (True, False)}
        launches = {native: graphstep.census(graph_of(lambda native=native: layer_pass(x, lin, bn, g, native), 1, keep=True))
                    for native in (True, False)}
        t = {True: [], False: []}
        for blk in range(BLOCKS):
            for native in ((True, False) if blk % 2 == 0 else (False, True)):
                t[native].append(us_per_call(graphs[native]))
        row = {"what": "dense + batch norm + relu, layer forward + backward %d x %d -> %d" % (ROWS, k, out)}
        row.update(summary(t))
        row["launches (memset nodes)"] = {"native": "%d (%d)" % launches[True][:2], "stock": "%d (%d)" % launches[False][:2]}
        print(json.dumps(row), flush=True)
    arms = {native: step_model(native) for native in (True, False)}
    t = {True: [], False: []}
    for blk in range(BLOCKS):
        for native in ((True, False) if blk % 2 == 0 else (False, True)):
            model, batches, _ = arms[native]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(STEPS):
                model.train_on_batch(*batches[i % len(batches)])
            e1.record()
            torch.cuda.synchronize()
            t[native].append(e0.elapsed_time(e1) * 1e3 / STEPS)
    row = {"what": "train step (criteo_c2, 1e5-row tables, batch %d), dnn_use_bn=True, replayed from the captured graph" % ROWS}
    row.update({k: (round(v, 1) if isinstance(v, float) else [round(q, 1) for q in v]) for k, v in summary(t).items()})
    row["graph_nodes"] = {"native": arms[True][2], "stock": arms[False][2]}
    print(json.dumps(row), flush=True)
finally:
    ops.DNN_BN_NATIVE = saved
