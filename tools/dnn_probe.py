"""A/B of the native dense-layer kernels (csrc/dnn.hip) against their library counterparts, in one process on one GPU, at
the two layers of the flagship DNN tower (batch 4096: 429 -> 256 and 256 -> 256, ReLU):

  python tools/dnn_probe.py            per operation: forward, input gradient, weight + bias gradient; then a whole layer
                                       forward + backward through ops.dense_relu with ops.DNN_NATIVE on and off
  python tools/dnn_probe.py --rows N   another batch size

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
