"""The fixed list of cases behind test_gpu_head_ex.py::test_ticketed_finish_matches_two_launch_finish_bit_for_bit: the
head's (identity, mse) and (sigmoid, mae) instantiations on a 17-row case and on one a row short
of a grid stride, each twice in a row, through the C ABI.

As a program (python ticket_child_ex.py OUT.npz, started by the test with XDFM_TICKETS=1 in a fresh process) it registers
the ticket board first and writes every output, and the board read after every case, to OUT.npz; imported by the test,
run_cases runs the same calls on the two-launch path.  The board is registered once per process and changes every later
launch, which is why the ticketed half never runs inside the pytest process (as tests/ticket_child.py)."""
import os
import sys

import numpy as np

if __name__ == "__main__":          # as a program: the paths conftest.py sets for the tests (its own directory is there already)
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_ROOT, os.path.join(_ROOT, "xdeepfm-pytorch_amd")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import head_ex_drivers as DX  # noqa: E402
import head_ex_ref as X  # noqa: E402

MODES = [(X.LINK_IDENTITY, X.LOSS_MSE), (X.LINK_SIGMOID, X.LOSS_MAE)]
CASES = ["c1111", "k4_k68_b2047"]


def run_cases(dev):
    import torch
    from xdfm_amd import _lib
    out = {}
    for mode in MODES:
        for name in CASES:
            c = X.make_ex_case(name, mode[0])
            tag = "%s/%s" % (X.mode_id(mode), name)
            for rep in (0, 1):
                for k, v in DX.run_head_ex(c, mode, dev).items():
                    out["head/%s/%d/%s" % (tag, rep, k)] = np.asarray(v)
            torch.cuda.synchronize()
            if 0 in _lib._BOARDS:
                out["board/" + tag] = _lib._BOARDS[0].cpu().numpy().copy()
    out["meta/board_registered"] = np.array(int(0 in _lib._BOARDS))
    return out


def main(path):
    import torch
    from xdfm_amd import _lib
    assert os.environ.get("XDFM_TICKETS") == "1", "start this program with XDFM_TICKETS=1"
    dev = torch.device("cuda:0")
    _lib.ticket_board(dev)
    assert 0 in _lib._BOARDS, "no ticket board was registered"
    out = run_cases(dev)
    np.savez(path, **out)
    print("ticket_child_ex: %d arrays, %d board readings" % (len(out), sum(k.startswith("board/") for k in out)))


if __name__ == "__main__":
    main(sys.argv[1])
