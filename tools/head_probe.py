"""A/B of the native output head (ops.Head: csrc/reg.hip, K8) against the stock tail it replaces (two nn.Linear(K, 1)
products, the logit adds, PredictionLayer, F.binary_cross_entropy / F.mse_loss / F.l1_loss(reduction='sum') and their
autograd), for each of the five (link, loss) pairs, in one process on one GPU, alternating blocks of the two arms on the
same tensors:

  python tools/head_probe.py              forward + backward at B 4096, Ku 384, Kv 256, then the node count of one
                                          captured train step of a small xDeepFM per (task, loss), native against stock
                                          (stock: _fused_head patched to return None; that graph is counted, not replayed)
  python tools/head_probe.py --weights    the head with one weight per example (xdfm_head_fwd_w / _bwd_w) against the head
                                          without: forward + backward of each pair replayed from a graph of 20 passes (kernel
                                          time), the node counts of a captured train step with and without a weight vector,
                                          and bench.py's criteo_c2 step (1e5 rows per table) replayed with and without one

Time: device events around blocks of eager forward + backward passes (launch gaps included: that is what the tail costs an
eager step).  No pass / fail bar rests on these numbers."""
import gc
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

assert torch.cuda.is_available(), "head_probe.py measures on a GPU; there is no CPU arm"
dev = torch.device("cuda:0")
B, KU, KV = 4096, 384, 256
PAIRS = [("binary", "binary_crossentropy", F.binary_cross_entropy), ("binary", "mse", F.mse_loss), ("binary", "mae", F.l1_loss),
         ("regression", "mse", F.mse_loss), ("regression", "mae", F.l1_loss)]

torch.manual_seed(0)
u = torch.randn(B, KU, device=dev, requires_grad=True)
v = torch.randn(B, KV, device=dev, requires_grad=True)
lin = torch.randn(B, 1, device=dev, requires_grad=True)
wu = (torch.randn(1, KU, device=dev) / (KU + KV) ** 0.5).requires_grad_(True)
wv = (torch.randn(1, KV, device=dev) / (KU + KV) ** 0.5).requires_grad_(True)
bias = torch.zeros(1, device=dev, requires_grad=True)
LEAVES = [u, v, lin, wu, wv, bias]
Y = {"binary": (torch.rand(B, 1, device=dev) < 0.3).float(), "regression": 3.0 + 1.5 * torch.randn(B, 1, device=dev)}


def native_pass(task, fn):
    for t in LEAVES:
        t.grad = None
    pred, loss = ops.Head.apply(Y[task], bias, lin, u, wu, v, wv, *ops.head_mode(task, fn))
    loss.backward()
    return pred, loss


def stock_pass(task, fn):
    for t in LEAVES:
        t.grad = None
    z = lin + F.linear(u, wu) + F.linear(v, wv) + bias
    pred = (torch.sigmoid(z) if task == "binary" else z).squeeze()
    loss = fn(pred, Y[task].squeeze(), reduction="sum")
    loss.backward()
    return pred, loss


WEIGHTS = "--weights" in sys.argv[1:]
W = torch.rand(B, device=dev) * 4.0


def weighted_pass(task, fn):
    for t in LEAVES:
        t.grad = None
    pred, loss = ops.Head.apply(Y[task], bias, lin, u, wu, v, wv, *ops.head_mode(task, fn), W)
    loss.backward()
    return pred, loss


def event_timer(run, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def graph_of(run, passes=20):
    """`passes` forward + backward passes captured in one HIP graph: replayed, they cost kernel time without launch gaps."""
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for _ in range(passes):
            run()
    return g


def stats(t):
    return {"median_us": round(statistics.median(t), 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2), "blocks": len(t)}


def alternate(arms, per_block, blocks=10):
    """arms: name -> callable; blocks of `per_block` calls between device events, the arms alternating -> us per call."""
    times = {k: [] for k in arms}
    order = list(arms)
    for blk in range(blocks):
        for k in (order if blk % 2 == 0 else order[::-1]):
            times[k].append(1e3 * event_timer(arms[k], per_block) / per_block)
    return times


def weights_main():
    passes = 20
    for task, name, fn in PAIRS:
        graphs = {"unweighted": graph_of(lambda: native_pass(task, fn), passes), "weighted": graph_of(lambda: weighted_pass(task, fn), passes)}
        t = alternate({k: g.replay for k, g in graphs.items()}, 10)
        row = {"what": "K8 forward + backward, %s / %s, B %d Ku %d Kv %d, graph of %d passes, us per pass" % (task, name, B, KU, KV, passes)}
        for k, v in t.items():
            row[k] = stats([x / passes for x in v])
        row["weighted_minus_unweighted_us"] = round(row["weighted"]["median_us"] - row["unweighted"]["median_us"], 2)
        row["spread_us"] = round(max(r["max_us"] - r["min_us"] for r in (row["weighted"], row["unweighted"])), 2)
        print(json.dumps(row), flush=True)
    # node counts of the captured step of the small model, as GraphedStep captures it
    for task, name, _ in PAIRS:
        counts = {}
        for arm in ("unweighted", "weighted"):
            model, x, y = small_model(task, name)
            sw = torch.rand(x.shape[0], device=dev) * 4.0 if arm == "weighted" else None
            for _ in range(graphstep.EAGER_STEPS_BEFORE_CAPTURE + 2):
                model.train_on_batch(x, y, sw)
            ents = [e for e in model.__dict__["_graphed_step"].entries.values() if e.graph is not None]
            counts[arm] = graphstep.census(ents[0].graph) if ents else None
        print(json.dumps({"what": "nodes of one captured train step (nodes, memset, other), %s / %s, B 256" % (task, name), **counts}), flush=True)
    # the flagship step: bench.py's criteo_c2 model at 1e5 rows per table, replayed with and without a weight vector
    import bench
    cfg = bench.WORKLOADS["criteo_c2"]
    vocab = bench.preset_vocab("mid", cfg["n_sparse"])
    batches = [(torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)) for X, y in bench.synthetic_batches(4, cfg["batch"], vocab, cfg["n_dense"], seed=7)]
    sw = torch.rand(cfg["batch"], device=dev) * 4.0
    model = bench.build_model(cfg, vocab, dev)
    model.train()
    state = {"i": 0}

    def step(weighted):
        xb, yb = batches[state["i"] % len(batches)]
        state["i"] += 1
        model.train_on_batch(xb, yb, sw if weighted else None)
    for _ in range(6):
        step(False)
        step(True)
    ents = {("weighted" if e.sw is not None else "unweighted"): e for e in model.__dict__["_graphed_step"].entries.values() if e.graph is not None}
    t = alternate({"unweighted": lambda: step(False), "weighted": lambda: step(True)}, 20)
    row = {"what": "train step (criteo_c2, 1e5-row tables, batch %d), replayed from the captured graph, us per step" % cfg["batch"],
           "graph_nodes": {k: e.nodes for k, e in ents.items()}}
    for k, v in t.items():
        row[k] = stats(v)
    row["weighted_minus_unweighted_us"] = round(row["weighted"]["median_us"] - row["unweighted"]["median_us"], 1)
    row["spread_us"] = round(max(r["max_us"] - r["min_us"] for r in (row["weighted"], row["unweighted"])), 1)
    print(json.dumps(row), flush=True)


def small_model(task, name):
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    from oracle import xdeepfm_oracle as orc
    vocab, nd, D = [50, 31, 77, 12, 9, 40], 3, 8
    cols = [SparseFeat("C%d" % (i + 1), n, D) for i, n in enumerate(vocab)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(nd)]
    model = xDeepFM(cols, cols, dnn_hidden_units=(32, 16), cin_layer_size=(16, 8), l2_reg_dnn=1e-5, task=task, device=dev)
    model.compile("adam", name, metrics=[])
    model.train()
    Xn, yn = orc.synthetic_batch(256, vocab, nd, seed=100)
    x, y = torch.from_numpy(Xn).to(dev), torch.from_numpy(yn).to(dev)
    if task == "regression":
        y = 3.0 + 1.5 * torch.randn_like(y)
    model.train_on_batch(x, y)                      # creates the model's GraphedStep
    return model, x, y


if WEIGHTS:
    weights_main()
    sys.exit(0)


for task, name, fn in PAIRS:
    arms = {"native": lambda: native_pass(task, fn), "stock": lambda: stock_pass(task, fn)}
    for run in arms.values():
        for _ in range(20):
            run()
    pa, la = native_pass(task, fn)
    ga = [t.grad.clone() for t in LEAVES]
    pb, lb = stock_pass(task, fn)
    gb = [t.grad.clone() for t in LEAVES]
    times = {k: [] for k in arms}
    for blk in range(10):
        for k in (("native", "stock") if blk % 2 == 0 else ("stock", "native")):
            times[k].append(event_timer(arms[k], 100) / 100)
    row = {"what": "head forward + backward, %s / %s, B %d Ku %d Kv %d (device events, eager launches)" % (task, name, B, KU, KV),
           "pred_max_abs_diff": float((pa.detach() - pb.detach()).abs().max()),
           "loss_rel_diff": abs(la.item() - lb.item()) / abs(lb.item()),
           "grad_max_rel_diff": max(float((x - y).abs().max() / y.abs().max().clamp_min(1e-30)) for x, y in zip(ga, gb))}
    for k, t in times.items():
        row[k] = {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4), "blocks": len(t)}
    row["stock_over_native"] = round(row["stock"]["median_ms"] / row["native"]["median_ms"], 2)
    print(json.dumps(row), flush=True)


def captured_nodes(task, name, native):
    """(nodes, memset nodes, other nodes) of one captured train step (the capture of graphstep.GraphedStep, without its
    refusal of memset nodes: the graph is only counted)."""
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    from oracle import xdeepfm_oracle as orc
    vocab, nd, D = [50, 31, 77, 12, 9, 40], 3, 8
    cols = [SparseFeat("C%d" % (i + 1), n, D) for i, n in enumerate(vocab)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(nd)]
    model = xDeepFM(cols, cols, dnn_hidden_units=(32, 16), cin_layer_size=(16, 8), l2_reg_dnn=1e-5, task=task, device=dev)
    model.compile("adam", name, metrics=[])
    model.train()
    if not native:
        model._fused_head = lambda x, y: None
    step = model.__dict__["_graphed_step"] = graphstep.GraphedStep(model)
    Xn, yn = orc.synthetic_batch(256, vocab, nd, seed=100)
    x, y = torch.from_numpy(Xn).to(dev), torch.from_numpy(yn).to(dev)
    if task == "regression":
        y = 3.0 + 1.5 * torch.randn_like(y)
    if hasattr(model.optim, "sync_lr"):
        model.optim.sync_lr()
    for _ in range(graphstep.EAGER_STEPS_BEFORE_CAPTURE):
        step._eager_on_side_stream(x, y)
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()
    try:
        sx, sy = x.clone(), y.clone()
        torch.cuda.current_stream().synchronize()
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph, stream=step.stream):
            model._train_step_eager(sx, sy)
        return graphstep.census(graph)
    finally:
        gc.enable()


for task, name, _ in PAIRS:
    n_nat, n_stock = captured_nodes(task, name, True), captured_nodes(task, name, False)
    print(json.dumps({"what": "nodes of one captured train step (nodes, memset, other), %s / %s, B 256" % (task, name),
                      "native": n_nat, "stock": n_stock}), flush=True)
