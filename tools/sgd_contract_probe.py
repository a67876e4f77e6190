#!/usr/bin/env python3
"""Which of torch.optim.SGD's momentum lines contract on this device: one bitwise comparison of torch's GPU step (foreach on
and off, plain and Nesterov, one step from a given buffer over 2^20 elements) with the eight fp32 spellings of
buf = mu buf + g, d = g + mu buf, p = p - lr d -- each line as one fma or as a rounded product and a rounded sum, emulated in
numpy.  What csrc/opt_math.h (OPT_SGDM) says about ATen's rounding rests on this; profiles/sgdm_probe.md records a run.

    python tools/sgd_contract_probe.py
"""
import itertools
import sys

import numpy as np
import torch

F32 = np.float32


def fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def two(a, b, c):
    return ((np.asarray(a, F32) * np.asarray(b, F32)).astype(F32) + np.asarray(c, F32)).astype(F32)


def main():
    dev = torch.device("cuda:0")
    n = 1 << 20
    rng = np.random.RandomState(1)
    p0 = (rng.randn(n) * 0.05).astype(F32)
    b0 = (rng.randn(n) * 0.02).astype(F32)
    g = (rng.randn(n) * 0.1).astype(F32)
    lr, mu = 0.01, 0.9
    for nesterov in (False, True):
        for foreach in (False, True):
            p = torch.nn.Parameter(torch.from_numpy(p0).to(dev))
            opt = torch.optim.SGD([p], lr=lr, momentum=mu, nesterov=nesterov, foreach=foreach)
            opt.state[p]["momentum_buffer"] = torch.from_numpy(b0).to(dev)
            p.grad = torch.from_numpy(g).to(dev)
            opt.step()
            torch.cuda.synchronize()
            gp, gb = p.detach().cpu().numpy(), opt.state[p]["momentum_buffer"].cpu().numpy()
            for kb, kd, kp in itertools.product((fma, two), repeat=3):
                buf = kb(F32(mu), b0, g)
                d = kd(F32(mu), buf, g) if nesterov else buf
                pp = kp(-F32(lr), d, p0)
                print("nesterov=%d foreach=%d buf=%s d=%s p=%s: buf mismatches %d, p mismatches %d of %d" % (
                    nesterov, foreach, kb.__name__, kd.__name__ if nesterov else "-", kp.__name__,
                    int((buf.view(np.uint32) != gb.view(np.uint32)).sum()), int((pp.view(np.uint32) != gp.view(np.uint32)).sum()), n))
    return 0


if __name__ == "__main__":
    sys.exit(main())
