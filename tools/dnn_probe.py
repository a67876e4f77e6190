"""A/B of the native dense-layer kernels (csrc/dnn.hip) against their library counterparts, in one process on one GPU, at
the two layers of the flagship DNN tower (batch 4096: 429 -> 256 and 256 -> 256, ReLU):

  python tools/dnn_probe.py            per operation: forward, input gradient, weight + bias gradient; then a whole layer
                                       forward + backward through ops.dense_relu with ops.DNN_NATIVE on and off
  python tools/dnn_probe.py --rows N   another batch size
  python tools/dnn_probe.py --dropout P   the native dropout (ops.dense_relu_dropout) against ops.dense_relu + nn.Dropout: one
                                       layer forward + backward at both shapes, then the flagship train step with
                                       dnn_dropout = P under both settings of ops.DNN_DROPOUT_NATIVE (profiles/dnn_dropout_probe.md)

Library arm of an operation = what runs with XDFM_DNN_NATIVE=0: torch._addmm_activation; gz.mm(W); xdfm_relu_bwd_colsum
(mask pass + bias gradient, once per layer, booked with the weight gradient) + gz.t().mm(x).
Time: every arm is captured into a HIP graph of CALLS back-to-back calls (kernel time, no host launch gaps) and the two
graphs are replayed in alternating blocks between device events; reported per call in microseconds."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xdeepfm-pytorch_amd"))
sys.path.insert(0, ROOT)

import torch
from xdfm_amd import _lib, ops

dev = torch.device("cuda:0")
ROWS = int(sys.argv[sys.argv.index("--rows") + 1]) if "--rows" in sys.argv else 4096
LAYERS = [(429, 256), (256, 256)]
CALLS, BLOCKS, REPLAYS = 20, 10, 10
lib = _lib.load()


def graph_of(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS):
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


def ab(what, native_fn, library_fn):
    graphs = {"native": graph_of(native_fn), "library": graph_of(library_fn)}
    times = {"native": [], "library": []}
    for b in range(BLOCKS):
        for arm in (("native", "library") if b % 2 == 0 else ("library", "native")):
            times[arm].append(us_per_call(graphs[arm]))
    row = {"what": what}
    for arm, v in times.items():
        row[arm] = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
    row["library_over_native"] = round(row["library"]["median_us"] / row["native"]["median_us"], 2)
    print(json.dumps(row), flush=True)
    return row


def library_mask_and_dw(g, y, x, ws, gz, db):
    _lib.check(lib.xdfm_relu_bwd_colsum(ops._ptr(g), ops._ptr(y), g.shape[0], g.shape[1], g.stride(0), y.stride(0), ops._ptr(ws),
                                        ops._ptr(gz), ops._ptr(db), ops._stream()), "relu_bwd_colsum")
    return gz.t().mm(x)


def layer_pass(x, W, b, g):
    a = [x.detach().requires_grad_(True), W.detach().requires_grad_(True), b.detach().requires_grad_(True)]
    ops.dense_relu(*a).backward(g)


def set_arm(native):
    ops.DNN_NATIVE = native


def dropout_layer_pass(x, W, b, g, p, native, drop):
    a = [x.detach().requires_grad_(True), W.detach().requires_grad_(True), b.detach().requires_grad_(True)]
    if native:
        ops.dense_relu_dropout(a[0], a[1], a[2], p, ops.draw_dropout_seed(x.device), 0).backward(g)      # the seed draw is part of the arm
    else:
        drop(ops.dense_relu(*a)).backward(g)


def flagship_step_model(p, native):
    """bench.py's criteo_c2 model (1e5 rows per table: the tower does not see the tables) with dnn_dropout = p, its train
    step captured with ops.DNN_DROPOUT_NATIVE = native."""
    import bench
    from xdfm_amd import graphstep
    cfg = dict(bench.WORKLOADS["criteo_c2"])
    vocab = bench.preset_vocab("mid", cfg["n_sparse"])
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    cols = [SparseFeat("C%d" % (i + 1), v, cfg["emb_dim"]) for i, v in enumerate(vocab)]
    cols += [DenseFeat("I%d" % (i + 1), 1) for i in range(cfg["n_dense"])]
    torch.manual_seed(0)
    model = xDeepFM(cols, cols, dnn_hidden_units=cfg["dnn"], cin_layer_size=cfg["cin"], l2_reg_dnn=1e-5, dnn_dropout=p, device=dev)
    model.compile("adam", "binary_crossentropy", metrics=[])
    model.train()
    step = model.__dict__["_graphed_step"] = graphstep.GraphedStep(model)
    batches = [(torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev))
               for X, y in bench.synthetic_batches(4, ROWS, vocab, cfg["n_dense"], seed=1)]
    ops.DNN_DROPOUT_NATIVE = native
    for i in range(5):                                   # two eager steps, the capture, two replays
        model.train_on_batch(*batches[i % len(batches)])
    torch.cuda.synchronize()
    ops.DNN_DROPOUT_NATIVE = True
    nodes = [e.nodes for e in step.entries.values() if e.graph is not None]
    assert step.replays >= 2 and not step.disabled and len(nodes) == 1, (step.replays, step.disabled, nodes)
    return model, batches, nodes[0]


def dropout_probe(p):
    """--dropout P: (a) one layer forward + backward through ops.dense_relu_dropout against ops.dense_relu + nn.Dropout at both
    flagship layers; (b) the flagship train step with dnn_dropout = P under both settings of ops.DNN_DROPOUT_NATIVE.  Alternating
    blocks in one process; `spread_us` is the largest (max - min) over an arm's blocks."""
    torch.manual_seed(0)
    drop = torch.nn.Dropout(p).train()
    for k, out in LAYERS:
        x = torch.randn(ROWS, k, device=dev)
        W = torch.randn(out, k, device=dev) / k ** 0.5
        b = torch.randn(out, device=dev)
        g = torch.randn(ROWS, out, device=dev)
        assert ops.dense_dropout_native(x, W, b, p)
        graphs = {native: graph_of(lambda native=native: dropout_layer_pass(x, W, b, g, p, native, drop)) for native in (True, False)}
        t = {True: [], False: []}
        for blk in range(BLOCKS):
            for native in ((True, False) if blk % 2 == 0 else (False, True)):
                t[native].append(us_per_call(graphs[native]))
        print(json.dumps({"what": "dropout %g, layer forward + backward %d x %d -> %d" % (p, ROWS, k, out),
                          "native_median_us": round(statistics.median(t[True]), 2), "stock_median_us": round(statistics.median(t[False]), 2),
                          "native_min_max_us": [round(min(t[True]), 2), round(max(t[True]), 2)],
                          "stock_min_max_us": [round(min(t[False]), 2), round(max(t[False]), 2)],
                          "spread_us": round(max(max(v) - min(v) for v in t.values()), 2)}), flush=True)
    arms = {native: flagship_step_model(p, native) for native in (True, False)}
    STEPS = 20
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
    print(json.dumps({"what": "flagship train step (criteo_c2, 1e5-row tables, batch %d), dnn_dropout %g" % (ROWS, p),
                      "native_median_us": round(statistics.median(t[True]), 1), "stock_median_us": round(statistics.median(t[False]), 1),
                      "native_min_max_us": [round(min(t[True]), 1), round(max(t[True]), 1)],
                      "stock_min_max_us": [round(min(t[False]), 1), round(max(t[False]), 1)],
                      "spread_us": round(max(max(v) - min(v) for v in t.values()), 1),
                      "graph_nodes": {"native": arms[True][2], "stock": arms[False][2]}}), flush=True)


if "--dropout" in sys.argv:
    dropout_probe(float(sys.argv[sys.argv.index("--dropout") + 1]))
    sys.exit(0)

torch.manual_seed(0)
total = {"native": 0.0, "library": 0.0}
for k, out in LAYERS:
    x = torch.randn(ROWS, k, device=dev)
    W = torch.randn(out, k, device=dev) / k ** 0.5
    b = torch.randn(out, device=dev)
    g = torch.randn(ROWS, out, device=dev)
    assert ops.dense_native(x, W, b)
    y = ops._dense_fwd_native(x, W, b, ops.ACT_CODES["relu"])
    gz = torch.where(y > 0, g, torch.zeros_like(g))
    ws = torch.empty(lib.xdfm_colsum_ws_elems(out), device=dev)
    gz_buf, db_buf = torch.empty_like(g), torch.empty(out, device=dev)
    shape = "%d x %d -> %d" % (ROWS, k, out)
    rows = [
        ab("forward " + shape, lambda: ops._dense_fwd_native(x, W, b, 1), lambda: torch._addmm_activation(b, x, W.t(), use_gelu=False)),
        ab("input gradient " + shape, lambda: ops._dense_bwd_native(g, y, x, W, True, False, False), lambda: gz.mm(W)),
        ab("weight + bias gradient (library: + mask pass) " + shape, lambda: ops._dense_bwd_native(g, y, x, W, False, True, True),
           lambda: library_mask_and_dw(g, y, x, ws, gz_buf, db_buf)),
    ]
    for r in rows:
        for arm in total:
            total[arm] += r[arm]["median_us"]
    layer = {}
    for native in (True, False):
        set_arm(native)
        layer[native] = graph_of(lambda: layer_pass(x, W, b, g))
    set_arm(True)
    t = {True: [], False: []}
    for blk in range(BLOCKS):
        for native in ((True, False) if blk % 2 == 0 else (False, True)):
            t[native].append(us_per_call(layer[native]))
    print(json.dumps({"what": "ops.dense_relu forward + backward " + shape,
                      "native_median_us": round(statistics.median(t[True]), 2), "library_median_us": round(statistics.median(t[False]), 2)}),
          flush=True)
print(json.dumps({"what": "tower: sum of the six operations' medians, rows %d" % ROWS, "native_us": round(total["native"], 1),
                  "library_us": round(total["library"], 1), "fp32_mfma_floor_us": round(
                      sum(6.0 * ROWS * k * out for k, out in LAYERS) / 157.3e12 * 1e6, 1)}))
