"""A/B of the native output head (ops.Head: csrc/reg.hip, K8) against the stock tail it replaces (two nn.Linear(K, 1)
products, the logit adds, PredictionLayer, F.binary_cross_entropy / F.mse_loss / F.l1_loss(reduction='sum') and their
autograd), for each of the five (link, loss) pairs, in one process on one GPU, alternating blocks of the two arms on the
same tensors:

  python tools/head_probe.py              forward + backward at B 4096, Ku 384, Kv 256, then the node count of one
                                          captured train step of a small xDeepFM per (task, loss), native against stock
                                          (stock: _fused_head patched to return None; that graph is counted, not replayed)

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


def event_timer(run, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


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
