"""A/B/C of dnn_activation='prelu' in the DNN tower, in one process on one GPU, the arms alternated in blocks:

  fused     ops.DensePReLU: the dense + PReLU kernels of csrc/dnn.hip (XDFM_DNN_PRELU_NATIVE=1)
  unfused   ops.dense (library GEMMs forward, native dX / dW) + the elementwise kernels of csrc/prelu.hip (XDFM_DNN_PRELU_NATIVE=0)
  stock     F.linear + F.prelu under autograd, eager (its backward holds a memset: it is not what a captured step may contain)

  python tools/dnn_prelu_probe.py            one layer forward + backward at the two layers of the flagship tower, batch 4096:
                                             429 -> 256 and 256 -> 256 -- time and launches; then bench.py's criteo_c2 train step with
                                             dnn_activation='prelu' on both settings of the switch, replayed from its captured graph --
                                             time and node count (profiles/dnn_prelu_probe.md)
  python tools/dnn_prelu_probe.py --rows N   another batch size

Time.  "graph": the fused and unfused arms captured into a HIP graph of CALLS back-to-back passes (kernel time, no host launch
gaps), the graphs replayed in alternating blocks between device events.  "eager": all three arms launched from Python, CALLS
passes between two device events (launch gaps included: the only way the stock arm can be timed).  Launches: the nodes of a
graph that holds one pass."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xdeepfm-pytorch_amd"))
sys.path.insert(0, ROOT)

import torch
import torch.nn.functional as F
from xdfm_amd import graphstep, ops

dev = torch.device("cuda:0")
ROWS = int(sys.argv[sys.argv.index("--rows") + 1]) if "--rows" in sys.argv else 4096
LAYERS = [(429, 256), (256, 256)]
CALLS, BLOCKS, REPLAYS, STEPS = 20, 10, 10, 20
ARMS = ("fused", "unfused", "stock")


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


def us_per_call_eager(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / CALLS


def layer_pass(x, lin, alpha, g, arm):
    ops.DNN_PRELU_NATIVE = arm == "fused"
    a = x.detach().requires_grad_(True)
    for p in list(lin.parameters()) + [alpha]:
        p.grad = None
    if arm == "stock":
        y = F.prelu(F.linear(a, lin.weight, lin.bias), alpha)
    else:
        assert ops.dense_prelu_native(a, lin.weight, lin.bias, alpha) == (arm == "fused")
        y = ops.dense_prelu(a, lin.weight, lin.bias, alpha)
    y.backward(g)


def summary(t):
    out = {}
    for arm, v in t.items():
        out[arm + "_median_us"] = round(statistics.median(v), 2)
        out[arm + "_min_max_us"] = [round(min(v), 2), round(max(v), 2)]
    out["spread_us"] = round(max(max(v) - min(v) for v in t.values()), 2)
    return out


def alternate(arms, blk):
    return arms if blk % 2 == 0 else tuple(reversed(arms))


def step_model(fused):
    """bench.py's criteo_c2 model (1e5 rows per table: the tower does not see the tables) with dnn_activation='prelu', its train
    step captured with ops.DNN_PRELU_NATIVE = fused."""
    import bench
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    cfg = dict(bench.WORKLOADS["criteo_c2"])
    vocab = bench.preset_vocab("mid", cfg["n_sparse"])
    cols = [SparseFeat("C%d" % (i + 1), v, cfg["emb_dim"]) for i, v in enumerate(vocab)]
    cols += [DenseFeat("I%d" % (i + 1), 1) for i in range(cfg["n_dense"])]
    torch.manual_seed(0)
    model = xDeepFM(cols, cols, dnn_hidden_units=cfg["dnn"], cin_layer_size=cfg["cin"], l2_reg_dnn=1e-5, dnn_activation="prelu", device=dev)
    model.compile("adam", "binary_crossentropy", metrics=[])
    model.train()
    step = model.__dict__["_graphed_step"] = graphstep.GraphedStep(model)
    batches = [(torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev))
               for X, y in bench.synthetic_batches(4, ROWS, vocab, cfg["n_dense"], seed=1)]
    ops.DNN_PRELU_NATIVE = fused
    for i in range(5):                                   # two eager steps, the capture, two replays
        model.train_on_batch(*batches[i % len(batches)])
    torch.cuda.synchronize()
    nodes = [(e.nodes,) + tuple(graphstep.census(e.graph)[1:]) for e in step.entries.values() if e.graph is not None]
    assert step.replays >= 2 and not step.disabled and len(nodes) == 1, (step.replays, step.disabled, nodes)
    return model, batches, nodes[0]


saved = ops.DNN_PRELU_NATIVE
try:
    torch.manual_seed(0)
    for k, out in LAYERS:
        x = torch.randn(ROWS, k, device=dev)
        lin = torch.nn.Linear(k, out).to(dev)
        alpha = torch.nn.Parameter(torch.full((1,), 0.25, device=dev))
        g = torch.randn(ROWS, out, device=dev)
        fn = {arm: (lambda arm=arm: layer_pass(x, lin, alpha, g, arm)) for arm in ARMS}
        graphs = {arm: graph_of(fn[arm], CALLS) for arm in ARMS[:2]}
        launches = {arm: graphstep.census(graph_of(fn[arm], 1, keep=True)) for arm in ARMS}
        t, te = {arm: [] for arm in ARMS[:2]}, {arm: [] for arm in ARMS}
        for blk in range(BLOCKS):
            for arm in alternate(ARMS[:2], blk):
                t[arm].append(us_per_call(graphs[arm]))
        for arm in ARMS:
            us_per_call_eager(fn[arm])                   # warm
        for blk in range(BLOCKS):
            for arm in alternate(ARMS, blk):
                te[arm].append(us_per_call_eager(fn[arm]))
        what = "dense + prelu, layer forward + backward %d x %d -> %d" % (ROWS, k, out)
        row = {"what": what + ", graph of %d passes" % CALLS}
        row.update(summary(t))
        row["launches (memset nodes)"] = {arm: "%d (%d)" % launches[arm][:2] for arm in ARMS}
        print(json.dumps(row), flush=True)
        row = {"what": what + ", eager"}
        row.update(summary(te))
        print(json.dumps(row), flush=True)
    arms = {fused: step_model(fused) for fused in (True, False)}
    t = {"fused": [], "unfused": []}
    for blk in range(BLOCKS):
        for arm in alternate(("fused", "unfused"), blk):
            model, batches, _ = arms[arm == "fused"]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(STEPS):
                model.train_on_batch(*batches[i % len(batches)])
            e1.record()
            torch.cuda.synchronize()
            t[arm].append(e0.elapsed_time(e1) * 1e3 / STEPS)
    row = {"what": "train step (criteo_c2, 1e5-row tables, batch %d), dnn_activation='prelu', replayed from the captured graph" % ROWS}
    row.update({k: (round(v, 1) if isinstance(v, float) else [round(q, 1) for q in v]) for k, v in summary(t).items()})
    row["graph_nodes (memset, other)"] = {"fused": "%d (%d, %d)" % arms[True][2], "unfused": "%d (%d, %d)" % arms[False][2]}
    print(json.dumps(row), flush=True)
finally:
    ops.DNN_PRELU_NATIVE = saved
