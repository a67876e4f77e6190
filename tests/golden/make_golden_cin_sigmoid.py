#!/usr/bin/env python3
"""Generate the sigmoid-CIN goldens by RUNNING THE REFERENCE (deepctr/layers/activation.py:57-84 as used at
deepctr/layers/interaction.py:185,226-229):

  tests/golden/cin_sigmoid_split.npz            CIN, B = 3, m = 4, D = 4, layer_size (6, 4), split_half
  tests/golden/cin_sigmoid_nosplit.npz          CIN, same input sizes, layer_size (5, 3), no split (odd H)
  tests/golden/sigmoid/model_sigmoid_small.npz  xDeepFM at model_sum_small's size with cin_activation="sigmoid"

make_golden.py's import recipe and its recipes for the two families are reused unchanged, so the keys are those of the
relu goldens: the CIN files hold x, out, gout, dx, w<i>, b<i>, dw<i>, db<i>, layer_size, split_half, activation; the model
file holds what model_sum_small holds plus `cin_activation`.  The files are data only.

The model file lives one directory down: tests/test_oracle_golden.py and tests/test_gpu_parity.py run every
tests/golden/model_*.npz through a relu model, and a sigmoid golden is none of theirs.  The two CIN files carry their
activation like cin_linear_act does, so the CIN golden tests of both files pick them up as further cases.

Usage:  python tests/golden/make_golden_cin_sigmoid.py
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg                      # noqa: E402  (registers the reference's deepctr package)
from deepctr.models.xdeepfm import xDeepFM    # noqa: E402

CIN_CASES = [
    # name,                 B, m, D, layer_size, split, act
    ("cin_sigmoid_split",   3, 4, 4, (6, 4),     True,  "sigmoid"),
    ("cin_sigmoid_nosplit", 3, 4, 4, (5, 3),     False, "sigmoid"),
]
MODEL_DIR = "sigmoid"
MODEL_CASES = [
    # model_sum_small's row of make_golden.MODEL_CASES with the activation
    (MODEL_DIR + "/model_sigmoid_small", xDeepFM, [7, 5, 11, 3, 9, 4], 3, 4, (8, 6), (16, 8), 32, dict(cin_activation="sigmoid")),
]


def main():
    torch.set_num_threads(4)
    mg.CIN_CASES = CIN_CASES
    mg.gen_cin()
    os.makedirs(os.path.join(HERE, MODEL_DIR), exist_ok=True)
    mg.MODEL_CASES = MODEL_CASES
    # kw_keys / kw_vals carry the integer constructor arguments of the attention models (none here); the activation is a
    # string and gets a key of its own
    save = mg._save

    def save_model(name, **arrays):
        assert arrays["kw_keys"].tolist() == ["cin_activation"]
        arrays["kw_keys"], arrays["kw_vals"] = np.array([]), np.array([])      # as model_sum_small stores its empty kw
        arrays["cin_activation"] = np.array("sigmoid")
        save(name, **arrays)

    mg._save = save_model
    try:
        mg.gen_models()
    finally:
        mg._save = save


if __name__ == "__main__":
    main()
