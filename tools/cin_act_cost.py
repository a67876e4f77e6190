"""What the full-output CIN path costs: device time of one CINStack forward + backward at the bench shape (m = 26, D = 16,
B = 4096, layers (256, 128, 128), sum pooling) for three arms

    relu-lean   relu, the default path (hidden rows + 1-bit sign mask, dX forms dOut itself)
    relu-full   relu with XDFM_CIN_LEAN=0 XDFM_CIN_NODOUT=0 (full fp32 outputs, dOut materialised)
    sigmoid     sigmoid, which always takes the full-output path (ops.cin_lean_allowed)

    python tools/cin_act_cost.py [--blocks 9] [--iters 20]

Each arm is warmed up, then timed in blocks of `iters` forward + backward passes between two device events; the arms
alternate block by block, and the median over the blocks of each arm is printed in microseconds per pass, with the spread
(min .. max) of its blocks.  A machine without a GPU is an error."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xdeepfm-pytorch_amd"))
from deepctr.layers import CIN  # noqa: E402

ARMS = [("relu-lean", "relu", {}), ("relu-full", "relu", {"XDFM_CIN_LEAN": "0", "XDFM_CIN_NODOUT": "0"}), ("sigmoid", "sigmoid", {})]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cin_act_cost: needs a GPU")
    dev = torch.device("cuda:0")
    m, D, ls, B = 26, 16, (256, 128, 128), 4096
    torch.manual_seed(0)
    x = (torch.randn(B, m, D, device=dev) * 0.5).requires_grad_(True)
    layers = {}
    for name, act, _ in ARMS:
        torch.manual_seed(1)
        layers[name] = CIN(m, ls, act, True, 0.0, 1024, device="cpu").to(dev)

    def one_pass(name, env):
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            layer = layers[name]
            layer.zero_grad()
            x.grad = None
            layer(x).sum().backward()
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v

    for name, _, env in ARMS:
        for _ in range(5):
            one_pass(name, env)
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in ARMS}
    for _ in range(a.blocks):
        for name, _, env in ARMS:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                one_pass(name, env)
            t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1) * 1e3 / a.iters)
    for name, _, _ in ARMS:
        v = sorted(times[name])
        print("%-10s median %8.1f us per forward + backward   (%d blocks of %d: %.1f .. %.1f)" % (
            name, v[len(v) // 2], a.blocks, a.iters, v[0], v[-1]), flush=True)


if __name__ == "__main__":
    main()
