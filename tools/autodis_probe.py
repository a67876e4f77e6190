"""A/B of the native AutoDis op (csrc/autodis.hip) against the stock per-field torch loop (XDFM_AUTODIS_NATIVE=0), in one
process on one GPU, alternating blocks of the two arms on the same tensors:

  python tools/autodis_probe.py                       layer alone (B 4096, F 13, K 16, D 16) and the xDeepFMPro train step
  python tools/autodis_probe.py --trace native|stock  a few layer forward + backward passes of one arm and nothing else, to
                                                      run under `rocprofv3 --kernel-trace --stats -d DIR -- python ...`
  python tools/autodis_probe.py --count DIR [passes]  kernel launches per pass from that trace's CSV

Layer time: device events around blocks of eager forward + backward passes (launch gaps included: that is what the
layer costs a step).  Step time: host clock around blocks of train_on_batch ending in a synchronise."""
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xdeepfm-pytorch_amd"))
sys.path.insert(0, ROOT)

TRACE_PASSES = 10


def count(trace_dir, passes):
    f = sorted(glob.glob(trace_dir + "/**/*kernel_trace.csv", recursive=True))[0]
    names = {}
    for r in csv.DictReader(open(f)):
        names[r["Kernel_Name"]] = names.get(r["Kernel_Name"], 0) + 1
    total = sum(names.values())
    ours = sum(n for k, n in names.items() if "autodis" in k)
    print(json.dumps({"trace": trace_dir, "passes": passes, "launches_per_pass": total / passes,
                      "autodis_kernel_launches_per_pass": ours / passes, "distinct_kernels": len(names)}))


if "--count" in sys.argv:
    i = sys.argv.index("--count")
    count(sys.argv[i + 1], int(sys.argv[i + 2]) if len(sys.argv) > i + 2 else TRACE_PASSES)
    sys.exit(0)

import torch
import bench
from deepctr.inputs import DenseFeat, SparseFeat
from deepctr.xdeepfm_pro import xDeepFMPro
from deepctr.xdeepfm_pro.autodis import AutoDisLayer
from xdfm_amd import ops

dev = torch.device("cuda:0")
B, F, K, D = 4096, 13, 16, 16


def arm(native):
    os.environ["XDFM_AUTODIS_NATIVE"] = "1" if native else "0"


def layer_pass(layer, cols, g):
    layer.zero_grad(set_to_none=True)
    flat, _ = layer(cols)
    torch.autograd.backward(flat, g)
    return flat


def layer_setup():
    torch.manual_seed(0)
    layer = AutoDisLayer(F, K, D, device=dev)
    x = torch.rand(B, F, device=dev)
    cols = [x[:, i:i + 1] for i in range(F)]
    g = torch.randn(B, F * D, device=dev)
    return layer, cols, g


if "--trace" in sys.argv:
    native = sys.argv[sys.argv.index("--trace") + 1] == "native"
    arm(native)
    layer, cols, g = layer_setup()
    torch.cuda.synchronize()
    for _ in range(TRACE_PASSES):
        layer_pass(layer, cols, g)
    torch.cuda.synchronize()
    print("traced %d passes, native=%s, ops.AutoDis.calls=%d" % (TRACE_PASSES, native, ops.AutoDis.calls))
    sys.exit(0)


def ab(run, blocks, per_block, timer):
    """alternate the arms block by block; per-pass times (ms) of every block, per arm"""
    times = {True: [], False: []}
    for b in range(blocks):
        for native in ((True, False) if b % 2 == 0 else (False, True)):
            arm(native)
            times[native].append(timer(run, per_block) / per_block)
    return times


def event_timer(run, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def host_timer(run, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(what, times):
    row = {"what": what}
    for native, name in ((True, "native"), (False, "stock")):
        v = times[native]
        row[name] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "blocks": len(v)}
    row["stock_over_native"] = round(row["stock"]["median_ms"] / row["native"]["median_ms"], 2)
    row["stock_over_native_range"] = [round(row["stock"]["min_ms"] / row["native"]["max_ms"], 2),
                                      round(row["stock"]["max_ms"] / row["native"]["min_ms"], 2)]
    print(json.dumps(row), flush=True)


# ---- the layer alone
layer, cols, g = layer_setup()
for native in (True, False):
    arm(native)
    for _ in range(20):
        layer_pass(layer, cols, g)
calls = ops.AutoDis.calls
arm(True)
a = layer_pass(layer, cols, g).detach().clone()
assert ops.AutoDis.calls == calls + 1, "the native arm did not reach ops.AutoDis"
arm(False)
b = layer_pass(layer, cols, g).detach()
assert ops.AutoDis.calls == calls + 1, "the stock arm reached ops.AutoDis"
print(json.dumps({"what": "layer outputs, native against stock", "max_abs_diff": float((a - b).abs().max()), "max_abs": float(b.abs().max())}))
summary("AutoDisLayer forward + backward, B %d F %d K %d D %d (device events, eager launches)" % (B, F, K, D),
        ab(lambda: layer_pass(layer, cols, g), blocks=10, per_block=200, timer=event_timer))

# ---- inside the xDeepFMPro train step at the criteo_pro shape
cfg = bench.WORKLOADS["criteo_pro"]
vocab = bench.preset_vocab("mid", cfg["n_sparse"])
fcols = [SparseFeat("C%d" % (i + 1), v, cfg["emb_dim"]) for i, v in enumerate(vocab)] + \
        [DenseFeat("I%d" % (i + 1), 1) for i in range(cfg["n_dense"])]
model = xDeepFMPro(fcols, fcols, cin_layer_size=cfg["cin"], dnn_hidden_units=cfg["dnn"], l2_reg_dnn=1e-5, device=dev,
                   use_autodis=True, autodis_buckets=16)
model.compile("adam", "binary_crossentropy", metrics=[])
model.train()
batches = [(torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev))
           for X, y in bench.synthetic_batches(4, cfg["batch"], vocab, cfg["n_dense"], seed=5)]
state = {"s": 0}


def step():
    model.train_on_batch(*batches[state["s"] % 4])
    state["s"] += 1


for native in (True, False):
    arm(native)
    for _ in range(6):
        step()
summary("xDeepFMPro(use_autodis=True) train step, criteo_pro shape, batch %d (host clock, synchronised blocks)" % cfg["batch"],
        ab(step, blocks=8, per_block=25, timer=host_timer))
