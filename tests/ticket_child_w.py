"""The fixed list of cases behind test_gpu_head_w_abi.py::test_ticketed_finish_matches_two_launch_finish_bit_for_bit: the
weighted head's (sigmoid, bce), (identity, mse) and (sigmoid, mae) instantiations on a vectorised and on a scalar case that
run more than one sweep, each twice in a row, through xdfm_head_fwd_w / xdfm_head_bwd_w.

As a program (python ticket_child_w.py OUT.npz, started by the test with XDFM_TICKETS=1 in a fresh process) it registers
the ticket board first and writes every output, and the board read after every case, to OUT.npz; imported by the test,
run_cases runs the same calls on the two-launch path.  The board is registered once per process and changes every later
launch, which is why the ticketed half never runs inside the pytest process (as tests/ticket_child_ex.py)."""
import os
import sys

import numpy as np

if __name__ == "__main__":          # as a program: the paths conftest.py sets for the tests (its own directory is there already)
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_ROOT, os.path.join(_ROOT, "xdeepfm-pytorch_amd")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import head_ex_ref as X  # noqa: E402
import head_w_drivers as DW  # noqa: E402
import head_w_ref as W  # noqa: E402

MODES = [(X.LINK_SIGMOID, X.LOSS_BCE), (X.LINK_IDENTITY, X.LOSS_MSE), (X.LINK_SIGMOID, X.LOSS_MAE)]
CASES = [(2049, 8, 32, True), (513, 7, 0, False)]


def run_cases(dev):
    import torch
    from xdfm_amd import _lib
    out = {}
    for mode in MODES:
        for case in CASES:
            c, w = W.make_w_case(case, mode[0])
            tag = "%s/%s" % (W.mode_id(mode), W.w_case_id(case))
            for rep in (0, 1):
                for k, v in DW.run_head_w(c, mode, dev, w).items():
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
    print("ticket_child_w: %d arrays, %d board readings" % (len(out), sum(k.startswith("board/") for k in out)))


if __name__ == "__main__":
    main(sys.argv[1])
