"""CPU: the helpers of the dense-layer GPU tests (tests/dnn_ref.py) -- the float64 reference against torch.autograd, the
split-plan mirror against the library's workspace query and the case table's claims, and the bound that makes the integer
inputs' sums exact in fp32."""
import pytest
import torch

import dnn_ref as R


@pytest.mark.parametrize("rows,k,out,relu,bias", [(5, 7, 32, True, True), (33, 13, 64, False, True), (9, 1, 96, True, False)])
def test_reference_matches_autograd_in_float64(rows, k, out, relu, bias):
    """Both sides are float64 and differ only in summation order: 1e-12 relative to each output's largest magnitude."""
    x, W, b, g = R.normal_inputs(rows, k, out, seed=rows + k + out)
    b = b if bias else None
    leaves = [t.double().requires_grad_(True) for t in (x, W)] + ([b.double().requires_grad_(True)] if bias else [])
    z = torch.nn.functional.linear(*leaves)
    y = torch.relu(z) if relu else z
    y.backward(g.double())
    y_ref = R.dense_ref(x, W, b, relu)
    dx, dW, db = R.dense_bwd_ref(g, y_ref.float() if relu else None, x, W)
    pairs = [("y", y_ref, y.detach()), ("dx", dx, leaves[0].grad), ("dW", dW, leaves[1].grad)]
    if bias:
        pairs.append(("db", db, leaves[2].grad))
    for name, got, want in pairs:
        assert got.dtype == torch.float64 and got.shape == want.shape, name
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), name


def test_negative_zero_negative_and_zero_close_the_mask():
    g = torch.tensor([[1.0, 2.0, 3.0, 4.0, 5.0, 6.0]])
    y = torch.tensor([[-0.0, -1.0, 0.0, 1.1754944e-38, 1.0, float("nan")]])
    x, W = torch.tensor([[2.0]]), torch.ones(6, 1)
    dx, dW, db = R.dense_bwd_ref(g, y, x, W)
    assert db.tolist() == [0.0, 0.0, 0.0, 4.0, 5.0, 0.0]
    assert dW[:, 0].tolist() == [0.0, 0.0, 0.0, 8.0, 10.0, 0.0] and dx.tolist() == [[9.0]]
    assert R.dense_bwd_ref(g, None, x, W)[2].tolist() == g[0].tolist()
    for v in R.MASK_CLOSED:
        assert not torch.tensor(v) > 0
    for v in R.MASK_OPEN:
        assert torch.tensor(v) > 0 and torch.tensor(v).item() >= 1.1754943508222875e-38          # normal: no flush can close it


def test_reference_zeros_are_positive():
    """An all-(-0.0) sum: the reference reports +0.0, what a sum that starts from +0.0 gives."""
    y = R.dense_ref(torch.tensor([[0.0]]), torch.tensor([[-3.0]] * 32), None, False)
    assert R.bits(y.float()).eq(0).all()
    for t in R.dense_bwd_ref(torch.zeros(1, 32), None, torch.tensor([[-3.0]]), torch.tensor([[-3.0]] * 32)):
        assert R.bits(t.float()).eq(0).all()


def test_split_plan_table():
    for rows, want in [(256, (1, 256, 1, 256)), (257, (2, 160, 2, 97)), (1100, (5, 224, 5, 204)), (2049, (9, 256, 9, 1)),
                       (4096, (16, 256, 16, 256)), (8225, (32, 288, 29, 161)), (9000, (32, 288, 32, 72)),
                       (8193, (32, 288, 29, 129)), (1, (1, 32, 1, 1))]:
        assert R.split_plan(rows) == want, rows


@pytest.mark.parametrize("name", list(R.ABI_CASES))
def test_each_case_exercises_what_its_name_says(name):
    from xdfm_amd import _lib
    lib = _lib.load()
    rows, k, out = R.ABI_CASES[name]
    want, kper, nsplit, last = R.split_plan(rows)
    assert (want, kper, nsplit, last) == R.ABI_PLANS[name]
    assert lib.xdfm_dense_supported(rows, k, out) == 1
    assert want * (out * k + out) == lib.xdfm_dense_bwd_w_ws_elems(rows, k, out)
    assert kper % R.DN_K == 0 and 1 <= nsplit <= want and 1 <= last <= kper and (nsplit - 1) * kper + last == rows
    #  the claims of the table's third column
    stages_dx = out // R.DN_K
    claims = {
        "E1": k == 1 and rows == 1 and kper == R.DN_K,
        "E2": rows % 64 == 0 and k % 64 == 0 and out % 64 == 0,
        "E3": rows % 64 == 1 and k % 64 == 1 and out % 64 == 32 and stages_dx == 3,
        "E4": rows % 64 == 63 and k % 32 == 31 and out % 64 == 32 and stages_dx == 5,
        "E5a": nsplit == 1 and R.split_plan(rows + 1)[2] == 2,
        "E5b": nsplit == 2 and R.split_plan(rows - 1)[2] == 1,
        "E6": nsplit == 5,                                   # 4 + 1: one unrolled round, a one-term tail
        "E7": nsplit == 9 and last == 1,
        "E8": nsplit == 16 and rows == 4096 and last == kper,
        "E9": rows > 8192 and kper == 288 > R.DN_SPLIT_ROWS and kper // R.DN_K == 9 and nsplit == 29 < want == 32 and out % 64 == 32,
        "E10": nsplit == 32 == want and kper == 288,
    }
    assert claims[name]
    if rows * out >= 64:
        y = R.mask_pattern(rows, out, seed=rows + out)
        is_open = y > 0
        for dim in (0, 1):
            assert bool(is_open.any(dim).all()) and bool((~is_open).any(dim).all()), "every row and column: open and closed cells"
        assert 0.4 < float(is_open.float().mean()) < 0.6


def test_integer_inputs_are_exact_in_fp32_at_the_largest_case():
    rows, k, out = max(R.ABI_CASES.values(), key=lambda c: c[0] * c[1] * c[2])
    assert (rows, k, out) == R.ABI_CASES["E9"]
    for r_, k_, o_ in R.ABI_CASES.values():
        assert r_ <= 9000 and R.exact_sum_bound(r_, k_, o_) < 2 ** 24
    assert R.exact_sum_bound(9000, 65, 160) == 81000
    x, W, b, g = R.int_inputs(rows, k, out, seed=9)
    for t in (x, W, b, g):
        assert t.dtype == torch.float32 and float(t.abs().max()) == 3.0 and bool((t == t.round()).all())
        assert sorted(t.unique().tolist()) == [-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0]
    y_mask = R.mask_pattern(rows, out, seed=10)
    y6 = R.dense_ref(x, W, b, False)
    dx6, dW6, db6 = R.dense_bwd_ref(g, y_mask, x, W)
    for t in (y6, dx6, dW6, db6):
        assert float(t.abs().max()) <= R.exact_sum_bound(rows, k, out) and bool((t == t.round()).all())
    #  an fp32 product on the CPU, whatever its order of additions, reproduces float64 exactly
    gz = torch.where(y_mask > 0, g, torch.zeros_like(g))
    for got, want in ((torch.mm(x, W.t()) + b, y6), (torch.mm(gz, W), dx6), (torch.mm(gz.t(), x), dW6), (gz.sum(0), db6)):
        assert got.dtype == torch.float32 and R.first_difference(got + 0.0, want.float()) is None


def test_first_difference_names_the_cell_and_its_tile():
    a = torch.zeros(130, 70)
    b = a.clone()
    assert R.first_difference(a, b) is None
    b[129, 65] = 1.0
    msg = R.first_difference(a, b)
    assert "(row 129, column 65)" in msg and "tile (2, 1), cell (1, 1)" in msg
    assert R.first_difference(torch.tensor([0.0]), torch.tensor([-0.0])) is not None
    nan = torch.tensor([float("nan")])
    assert R.first_difference(nan, nan.clone()) is None
