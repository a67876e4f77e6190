"""A/B of the native pooled variable-length lookup (ops.VarLenPool: csrc/varlen.hip) against torch's composition of the
same arithmetic (index, mask, pool, autograd -- what deepctr/inputs.py:141-155 + deepctr/layers/sequence.py:49-77 launch),
in one process on one GPU, alternating blocks of the two arms on the same tensors:

  python tools/varlen_probe.py                        forward + backward at B 4096, F 3 (mean / sum / max), maxlen 20, D 16
  python tools/varlen_probe.py --trace native|torch   a few passes of one arm and nothing else, to run under
                                                      `rocprofv3 --kernel-trace --stats -d DIR -- python ...`
  python tools/varlen_probe.py --count DIR [passes]   kernel launches per pass from that trace's CSV

Time: device events around blocks of eager forward + backward passes (launch gaps included: that is what the stage costs
an eager step).  Launches of the native arm are also counted without a profiler, from ops.PROFILE and the chunking rule of
K2 (one launch per 4096 positions and call)."""
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xdeepfm-pytorch_amd"))
sys.path.insert(0, ROOT)

TRACE_PASSES = 10


def count(trace_dir, passes):
    f = sorted(glob.glob(trace_dir + "/**/*kernel_trace.csv", recursive=True))[0]
    names = {}
    for r in csv.DictReader(open(f)):
        names[r["Kernel_Name"]] = names.get(r["Kernel_Name"], 0) + 1
    print(json.dumps({"trace": trace_dir, "passes": passes, "launches_per_pass": sum(names.values()) / passes,
                      "distinct_kernels": len(names)}))


if "--count" in sys.argv:
    i = sys.argv.index("--count")
    count(sys.argv[i + 1], int(sys.argv[i + 2]) if len(sys.argv) > i + 2 else TRACE_PASSES)
    sys.exit(0)

import torch
from xdfm_amd import ops

dev = torch.device("cuda:0")
B, F, T, D, V = 4096, 3, 20, 16, 1000
COMBINERS = ("mean", "sum", "max")

torch.manual_seed(0)
ids = torch.randint(1, V, (B, F, T))
lengths = torch.randint(1, T + 1, (B, F))
ids[torch.arange(T)[None, None, :] >= lengths[:, :, None]] = 0          # zero mask: padding behind the valid items
X = ids.reshape(B, F * T).float().to(dev)
tables = [torch.randn(V, D, device=dev, requires_grad=True) for _ in range(F)]
lins = [torch.randn(V, 1, device=dev, requires_grad=True) for _ in range(F)]
g_emb = torch.randn(F, B * D, device=dev)
g_lin = torch.randn(B, 1, device=dev)
plan = ops.VarLenPlan([f * T for f in range(F)], [T] * F, [None] * F, COMBINERS, [V] * F, D, 0, 0)


def native_pass():
    for t in tables + lins:
        t.grad = None
    emb = torch.empty((F, B * D), device=dev)
    dnn = torch.empty((B, F * D), device=dev)
    lin = torch.zeros((B, 1), device=dev)
    emb, dnn, lin = ops.VarLenPool.apply(X, emb, dnn, lin, plan, F, *tables, *lins)
    torch.autograd.backward([emb, lin], [g_emb, g_lin])
    return emb, lin


def torch_pool(rows, mask, mode):
    m = mask.unsqueeze(2).float()
    if mode == "max":
        return (rows - (1 - m) * 1e9).max(dim=1)[0]
    s = (rows * m).sum(dim=1)
    return s / (mask.float().sum(1, keepdim=True) + 1e-8) if mode == "mean" else s


def torch_pass():
    for t in tables + lins:
        t.grad = None
    embs, lin = [], torch.zeros((B, 1), device=dev)
    for f in range(F):
        idx = X[:, f * T:(f + 1) * T].long()
        mask = idx != 0
        embs.append(torch_pool(tables[f][idx], mask, COMBINERS[f]))
        lin = lin + torch_pool(lins[f][idx], mask, COMBINERS[f])
    emb = torch.stack(embs).reshape(F, B * D)
    torch.autograd.backward([emb, lin], [g_emb, g_lin])
    return emb, lin


ARMS = {"native": native_pass, "torch": torch_pass}

if "--trace" in sys.argv:
    arm = sys.argv[sys.argv.index("--trace") + 1]
    torch.cuda.synchronize()
    for _ in range(TRACE_PASSES):
        ARMS[arm]()
    torch.cuda.synchronize()
    print("traced %d passes of the %s arm" % (TRACE_PASSES, arm))
    sys.exit(0)


def event_timer(run, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


for run in ARMS.values():
    for _ in range(20):
        run()
a, la = native_pass()
ga = [t.grad.clone() for t in tables + lins]
b, lb = torch_pass()
gb = [t.grad.clone() for t in tables + lins]
a, la, b, lb = a.detach(), la.detach(), b.detach(), lb.detach()
print(json.dumps({"what": "native against torch", "pooled_max_abs_diff": float((a - b).abs().max()),
                  "linear_max_abs_diff": float((la - lb).abs().max()),
                  "grad_max_abs_diff": max(float((x - y).abs().max()) for x, y in zip(ga, gb)),
                  "grad_max_abs": max(float(y.abs().max()) for y in gb)}))
# launches of the native arm: the forward, the expand kernel, and K2's reduce once per 4096 positions for the [V, D] and
# once more for the [V, 1] tables (+ one zero fill of the gradient buffer by torch)
ops.PROFILE = []
native_pass()
calls = [p[0] for p in ops.PROFILE]
ops.PROFILE = None
chunks = (B * T + 4095) // 4096
print(json.dumps({"what": "native launches per pass", "library_calls": calls, "kernel_launches": 1 + 1 + 2 * chunks, "fills": 1}))

times = {k: [] for k in ARMS}
for blk in range(10):
    for k in (("native", "torch") if blk % 2 == 0 else ("torch", "native")):
        times[k].append(event_timer(ARMS[k], 100) / 100)
row = {"what": "pooled lookup forward + backward, B %d F %d maxlen %d D %d V %d (device events, eager launches)" % (B, F, T, D, V)}
for k, v in times.items():
    row[k] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "blocks": len(v)}
row["torch_over_native"] = round(row["torch"]["median_ms"] / row["native"]["median_ms"], 2)
print(json.dumps(row), flush=True)
