"""GPU tests (-m gpu) of every f16x3 / bf16 template instance of the CIN contraction kernels, driven one level at a time
through the C ABI and compared with a float64 contraction computed by torch on the device:

  forward  xdfm_cin_fwd_pack + xdfm_cin_level_fwd         cin_fwd_x3_kernel<MT, M, NW, .., NT, SYM>   relu(W @ Z + b)
  dX       xdfm_cin_bwd_pack + xdfm_cin_level_bwd_x_ex    cin_bwd_x3_kernel<HBT, NW, NT>,
                                                           cin_bwd_x3_sym_kernel<HBT, NW, NT, M>       autograd of W @ Z
  dW       xdfm_cin_level_bwd_w, and xdfm_cin_bwd_prep +
           xdfm_cin_level_bwd_w_prepared                   cin_bwd_w_x3_kernel<4, NW, NT, SYM>         dOut @ Z^T

with Z[(i, j)][n] = x_prev[i][n] * x0[j][n] (deepctr/layers/interaction.py:218-229).  Each SWEEP row names the instance the
host must pick in each direction, and the probes last_fwd_inst / last_bwx_inst / last_bww_inst (include/xdfm.h) must
report exactly that one; tests/test_cin_coverage.py checks on the CPU that the rows reach every instance the sources build
and that every claim follows from the host rules.

Two input families per row:

exact   W in [-4, 4], x0 / x_prev / dOut in [-3, 3], bias in [-8, 8], dX prefill in [-5, 5], all integers.  Every operand a
        kernel forms is exact in its narrow format.  f16x3 range-fits by powers of two (|W| sW < 2^15; x columns or rows
        < 2^7; dOut < 2^15), so W sW, the x_prev x0 products (< 2^14, at most 4 significant bits) and dOut sD are fp16
        values with a zero lo half; bf16 holds every integer up to 256 (|W| <= 4, |x_prev x0| <= 9, |dOut| <= 3).  Every
        partial sum is an integer multiple of the scales' product, below 2^24 of it: forward <= Hp m 4 9 + 8 <= 1600 * 36
        + 8, dZ <= 256 * 4 * 3, dX <= 40 * 3072 * 3 + 5, dW <= N * 27 < 16640 * 27.  The fp32 accumulation is then exact in
        any order, the scales come off exactly, and the kernels must reproduce the float64 result bit for bit: a dropped,
        doubled or mispaired term changes an integer.
normal  Gaussian inputs.  Every element must satisfy |got - ref| <= K * mag + 2^-24 |ref| (the rounding of the stored
        fp32 value), mag = the same contraction on |W|, |b|, |x|, |dOut| in float64: the bar is scaled per element, not by
        the tensor's maximum.  K is the smallest power of two at least 4x the worst (|got - ref| - 2^-24 |ref|) / mag
        measured on the healthy kernels over the whole sweep (MI355X): cin_math 1 K = 2^-18, worst 4.8e-7 (the fp32-MFMA
        forward at m = 50; the f16x3 kernels themselves 1.9e-7: dx0 at m = 22, H = 240); cin_math 2 K = 2^-6, worst
        3.8e-3 (the bf16 forward at m = 12, H = 225; dX 1.7e-3, dW 6.5e-4).

Every dX and dW call runs twice and must repeat its bits; the folded dW must be exactly symmetric.  dX runs with
XDFM_BWX_SET_DXP | XDFM_BWX_SET_DX0 and accumulating, on outputs filled with non-zero values beforehand.
"""
import contextlib
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

F, B = 1, 2          # cin_math: f16x3, bf16
K = {F: 2.0 ** -18, B: 2.0 ** -6}

# Instance codes (the probe values): T * 1000 + waves * 100 + MFMA terms * 10 + folded, T = MT (forward), HBT (dX) or 4 (dW),
# terms 3 = f16x3, 1 = bf16; 0 = the call ran the fp32-MFMA kernel.  fold: 0 = x_prev is a tensor of its own; 1 = level 0
# (x_prev IS x0) with option x3_sym 1 -- the folded kernels where they are built (m = 22, 26), the full grid elsewhere;
# 2 = level 0 with x3_sym 0.  N = 16384 is the 8-wave threshold.
#   m, H, Hp, N, cin_math, x3_waves, fold, other options, forward, dX, dW
SWEEP = [
    # every even field count: f16x3 MT 2 / MT 4 / MT 8 with 4 and 8 waves, bf16 MT 4 / MT 8 with 4 and 8 waves
    (8, 33, 17, 1000, F, 0, 0, {}, 2430, 4430, 0),
    (8, 100, 13, 2048, F, 0, 0, {}, 4430, 8430, 4830),
    (8, 129, 13, 16420, F, 0, 0, {}, 4830, 16830, 4830),
    (8, 225, 9, 16383, F, 0, 0, {}, 8430, 16430, 0),
    (8, 256, 11, 16384, F, 0, 0, {}, 8830, 16830, 4830),
    (8, 65, 21, 3000, B, 0, 0, {}, 4410, 8410, 4810),
    (8, 240, 9, 4100, B, 0, 0, {}, 8410, 16410, 4810),
    (8, 256, 10, 16500, B, 0, 0, {}, 8810, 16810, 4810),
    (10, 40, 21, 16384, F, 0, 0, {}, 2430, 4830, 0),
    (10, 160, 9, 16384, F, 4, 0, {}, 4430, 16430, 4430),
    (10, 80, 5, 16388, F, 0, 0, {}, 4830, 8830, 4830),
    (10, 240, 13, 2500, F, 0, 0, {}, 8430, 16430, 4830),
    (10, 225, 3, 16420, F, 0, 0, {}, 8830, 16830, 4830),
    (10, 100, 7, 16384, B, 0, 0, {}, 4410, 8810, 4810),
    (10, 225, 17, 777, B, 0, 0, {}, 8410, 16410, 0),
    (10, 240, 5, 16384, B, 0, 0, {}, 8810, 16810, 4810),
    (12, 47, 13, 777, F, 0, 0, {}, 2430, 4430, 0),
    (12, 129, 19, 3001, F, 0, 0, {}, 4430, 16430, 0),
    (12, 200, 4, 16500, F, 0, 0, {}, 4830, 16830, 4830),
    (12, 256, 9, 1028, F, 0, 0, {}, 8430, 16430, 4830),
    (12, 240, 5, 16416, F, 0, 0, {}, 8830, 16830, 4830),
    (12, 150, 11, 16388, B, 4, 0, {}, 4410, 16410, 4410),
    (12, 256, 6, 2052, B, 0, 0, {}, 8410, 16410, 4810),
    (12, 225, 3, 16640, B, 0, 0, {}, 8810, 16810, 4810),
    (14, 52, 9, 16420, F, 0, 0, {}, 2430, 4830, 0),
    (14, 65, 17, 4096, F, 0, 0, {}, 4430, 8430, 4830),
    (14, 224, 3, 16384, F, 0, 0, {}, 4830, 16830, 4830),
    (14, 225, 7, 16384, F, 4, 0, {}, 8430, 16430, 4430),
    (14, 256, 4, 16448, F, 0, 0, {}, 8830, 16830, 4830),
    (14, 200, 13, 1500, B, 0, 0, {}, 4410, 16410, 4810),
    (14, 240, 7, 16384, B, 4, 0, {}, 8410, 16410, 4410),
    (14, 256, 5, 16420, B, 0, 0, {}, 8810, 16810, 4810),
    (16, 64, 25, 96, F, 0, 0, {}, 2430, 4430, 0),
    (16, 200, 11, 3000, F, 0, 0, {}, 4430, 16430, 4830),
    (16, 96, 6, 16400, F, 0, 0, {}, 4830, 8830, 4830),
    (16, 240, 13, 2000, F, 0, 0, {}, 8430, 16430, 4830),
    (16, 256, 3, 16420, F, 0, 0, {"bww_nsplit": 1}, 8830, 16830, 4830),
    (16, 80, 9, 16416, B, 0, 0, {}, 4410, 8810, 4810),
    (16, 225, 11, 3000, B, 0, 0, {}, 8410, 16410, 4810),
    (16, 240, 3, 16384, B, 0, 0, {}, 8810, 16810, 4810),
    (18, 36, 11, 16500, F, 0, 0, {}, 2430, 4830, 0),
    (18, 224, 17, 2500, F, 0, 0, {}, 4430, 16430, 4830),
    (18, 256, 9, 16384, F, 0, 0, {"x3_fwd_mt": 4}, 4830, 16830, 4830),
    (18, 225, 5, 132, F, 0, 0, {}, 8430, 16430, 4830),
    (18, 240, 4, 16420, F, 0, 0, {}, 8830, 16830, 4830),
    (18, 129, 7, 2048, B, 0, 0, {}, 4410, 16410, 4810),
    (18, 256, 9, 16383, B, 0, 0, {}, 8410, 16410, 0),
    (18, 225, 5, 16388, B, 0, 0, {}, 8810, 16810, 4810),
    (20, 58, 19, 4100, F, 0, 0, {}, 2430, 4430, 0),
    (20, 96, 5, 16384, F, 4, 0, {}, 4430, 8430, 4430),
    (20, 150, 3, 16640, F, 0, 0, {}, 4830, 16830, 4830),
    (20, 256, 11, 3076, F, 0, 0, {}, 8430, 16430, 4830),
    (20, 225, 4, 16500, F, 0, 0, {}, 8830, 16830, 4830),
    (20, 224, 9, 16384, B, 0, 0, {}, 4410, 16810, 4810),
    (20, 240, 13, 1000, B, 0, 0, {}, 8410, 16410, 4810),
    (20, 256, 3, 16416, B, 0, 0, {}, 8810, 16810, 4810),
    (22, 45, 27, 1537, F, 0, 0, {}, 2430, 4430, 0),
    (22, 129, 9, 2000, F, 0, 0, {}, 4430, 16430, 4830),
    (22, 100, 5, 16420, F, 0, 0, {}, 4830, 8830, 4830),
    (22, 256, 7, 4096, F, 0, 0, {}, 8430, 16430, 4830),
    (22, 240, 3, 16384, F, 0, 0, {}, 8830, 16830, 4830),
    (22, 160, 9, 3000, B, 0, 0, {}, 4410, 16410, 4810),
    (22, 225, 7, 2500, B, 0, 0, {}, 8410, 16410, 4810),
    (22, 240, 4, 16500, B, 0, 0, {}, 8810, 16810, 4810),
    (24, 61, 7, 16388, F, 0, 0, {}, 2430, 4830, 0),
    (24, 65, 15, 2052, F, 0, 0, {}, 4430, 8430, 4830),
    (24, 224, 4, 16384, F, 0, 0, {}, 4830, 16830, 4830),
    (24, 225, 9, 1000, F, 0, 0, {}, 8430, 16430, 4830),
    (24, 256, 3, 16640, F, 0, 0, {}, 8830, 16830, 4830),
    (24, 100, 11, 2500, B, 0, 0, {}, 4410, 8410, 4810),
    (24, 256, 5, 16384, B, 4, 0, {}, 8410, 16410, 4410),
    (24, 225, 3, 16420, B, 0, 0, {}, 8810, 16810, 4810),
    (26, 33, 23, 3000, F, 0, 0, {}, 2430, 4430, 0),
    (26, 80, 13, 2500, F, 0, 0, {}, 4430, 8430, 4830),
    (26, 200, 5, 16416, F, 0, 0, {}, 4830, 16830, 4830),
    (26, 240, 9, 16383, F, 0, 0, {}, 8430, 16430, 0),
    (26, 256, 5, 16384, F, 0, 0, {}, 8830, 16830, 4830),
    (26, 129, 9, 16384, B, 0, 0, {}, 4410, 16810, 4810),
    (26, 256, 7, 4000, B, 0, 0, {}, 8410, 16410, 4810),
    (26, 240, 3, 16448, B, 0, 0, {}, 8810, 16810, 4810),
    (28, 40, 15, 16416, F, 0, 0, {}, 2430, 4830, 0),
    (28, 100, 6, 16420, F, 4, 0, {}, 4430, 8430, 4430),
    (28, 180, 4, 16420, F, 0, 0, {"bww_nsplit": 3}, 4830, 16830, 4830),
    (28, 240, 7, 2048, F, 0, 0, {}, 8430, 16430, 4830),
    (28, 225, 3, 16384, F, 0, 0, {}, 8830, 16830, 4830),
    (28, 65, 9, 16384, B, 0, 0, {}, 4410, 8810, 4810),
    (28, 240, 5, 3076, B, 0, 0, {}, 8410, 16410, 4810),
    (28, 256, 4, 16384, B, 0, 0, {}, 8810, 16810, 4810),
    (30, 47, 5, 2500, F, 0, 0, {}, 2430, 4430, 0),
    (30, 129, 12, 1060, F, 0, 0, {}, 4430, 16430, 4830),
    (30, 72, 6, 16388, F, 0, 0, {}, 4830, 8830, 4830),
    (30, 256, 5, 16383, F, 0, 0, {}, 8430, 16430, 0),
    (30, 240, 3, 16500, F, 0, 0, {}, 8830, 16830, 4830),
    (30, 200, 7, 16384, B, 0, 0, {}, 4410, 16810, 4810),
    (30, 225, 9, 2500, B, 0, 0, {}, 8410, 16410, 4810),
    (30, 256, 3, 16384, B, 0, 0, {}, 8810, 16810, 4810),
    (32, 52, 29, 130, F, 0, 0, {}, 2430, 4430, 0),
    (32, 160, 8, 3000, F, 0, 0, {}, 4430, 16430, 4830),
    (32, 140, 3, 16384, F, 0, 0, {}, 4830, 16830, 4830),
    (32, 225, 5, 16388, F, 4, 0, {}, 8430, 16430, 4430),
    (32, 256, 4, 16420, F, 0, 0, {}, 8830, 16830, 4830),
    (32, 96, 13, 2000, B, 0, 0, {}, 4410, 8410, 4810),
    (32, 256, 7, 1028, B, 0, 0, {}, 8410, 16410, 4810),
    (32, 240, 3, 16420, B, 0, 0, {}, 8810, 16810, 4810),
    (34, 64, 9, 16384, F, 0, 0, {}, 2430, 4830, 0),
    (34, 200, 14, 2048, F, 0, 0, {}, 4430, 16430, 4830),
    (34, 224, 3, 16420, F, 0, 0, {}, 4830, 16830, 4830),
    (34, 240, 5, 2500, F, 0, 0, {}, 8430, 16430, 4830),
    (34, 256, 2, 16384, F, 0, 0, {}, 8830, 16830, 4830),
    (34, 150, 5, 16500, B, 0, 0, {}, 4410, 16810, 4810),
    (34, 225, 9, 4000, B, 0, 0, {}, 8410, 16410, 4810),
    (34, 256, 3, 16388, B, 0, 0, {}, 8810, 16810, 4810),
    (36, 36, 10, 2500, F, 0, 0, {}, 2430, 4430, 0),
    (36, 90, 9, 2052, F, 0, 0, {}, 4430, 8430, 4830),
    (36, 224, 2, 16448, F, 0, 0, {}, 4830, 16830, 4830),
    (36, 256, 7, 16384, F, 4, 0, {}, 8430, 16430, 4430),
    (36, 225, 4, 16416, F, 0, 0, {}, 8830, 16830, 4830),
    (36, 110, 9, 2048, B, 0, 0, {}, 4410, 8410, 4810),
    (36, 240, 3, 16384, B, 4, 0, {}, 8410, 16410, 4410),
    (36, 225, 5, 16384, B, 0, 0, {}, 8810, 16810, 4810),
    (38, 58, 11, 16400, F, 0, 0, {}, 2430, 4830, 0),
    (38, 224, 10, 1537, F, 0, 0, {}, 4430, 16430, 0),
    (38, 160, 3, 16384, F, 0, 0, {}, 4830, 16830, 4830),
    (38, 225, 6, 3000, F, 0, 0, {}, 8430, 16430, 4830),
    (38, 240, 3, 16420, F, 0, 0, {}, 8830, 16830, 4830),
    (38, 200, 6, 16420, B, 0, 0, {}, 4410, 16810, 4810),
    (38, 256, 5, 2500, B, 0, 0, {}, 8410, 16410, 4810),
    (38, 225, 3, 16500, B, 0, 0, {}, 8810, 16810, 4810),
    (40, 64, 33, 2052, F, 0, 0, {}, 2430, 4430, 0),
    (40, 150, 9, 1000, F, 0, 0, {}, 4430, 16430, 4830),
    (40, 128, 4, 16384, F, 0, 0, {}, 4830, 8830, 4830),
    (40, 256, 5, 16383, F, 0, 0, {}, 8430, 16430, 0),
    (40, 256, 3, 16420, F, 0, 0, {}, 8830, 16830, 4830),
    (40, 65, 13, 16384, B, 0, 0, {}, 4410, 8810, 4810),
    (40, 240, 7, 3000, B, 0, 0, {}, 8410, 16410, 4810),
    (40, 256, 3, 16384, B, 0, 0, {}, 8810, 16810, 4810),
    # level 0 over the folded pair list (m = 22, 26): every tile and wave count of the three folded kernels
    (22, 48, 22, 3000, F, 0, 1, {}, 2431, 4431, 0),
    (22, 40, 22, 16384, F, 0, 1, {}, 2431, 4831, 0),
    (22, 20, 22, 2000, F, 0, 1, {}, 0, 2431, 0),
    (22, 100, 22, 2500, F, 0, 1, {}, 4431, 8431, 4831),
    (22, 120, 22, 16420, F, 0, 1, {}, 4831, 8831, 4831),
    (22, 200, 22, 16384, F, 4, 1, {}, 4431, 16431, 4431),
    (22, 240, 22, 4100, F, 0, 1, {}, 8431, 16431, 4831),
    (22, 256, 22, 16500, F, 0, 1, {}, 8831, 16831, 4831),
    (22, 64, 22, 16384, B, 0, 1, {}, 0, 4411, 0),
    (22, 100, 22, 3000, B, 0, 1, {}, 4411, 8411, 4811),
    (22, 128, 22, 16384, B, 0, 1, {}, 4411, 8811, 4811),
    (22, 225, 22, 2000, B, 4, 1, {}, 8411, 16411, 4411),
    (22, 256, 22, 16420, B, 0, 1, {}, 8811, 16811, 4811),
    (26, 33, 26, 1000, F, 0, 1, {}, 2431, 4431, 0),
    (26, 64, 26, 16388, F, 0, 1, {}, 2431, 4831, 0),
    (26, 32, 26, 16384, F, 0, 1, {}, 0, 2431, 0),
    (26, 65, 26, 3000, F, 0, 1, {}, 4431, 8431, 4831),
    (26, 100, 26, 16384, F, 0, 1, {}, 4831, 8831, 4831),
    (26, 224, 26, 16384, F, 0, 1, {"bww_nsplit": 7}, 4831, 16831, 4831),
    (26, 128, 26, 16416, F, 4, 1, {}, 4431, 8431, 4431),
    (26, 256, 26, 2052, F, 0, 1, {}, 8431, 16431, 4831),
    (26, 225, 26, 16420, F, 0, 1, {}, 8831, 16831, 4831),
    (26, 48, 26, 3000, B, 0, 1, {}, 0, 4411, 0),
    (26, 160, 26, 2500, B, 0, 1, {}, 4411, 16411, 4811),
    (26, 100, 26, 16420, B, 0, 1, {}, 4411, 8811, 4811),
    (26, 128, 26, 3000, B, 4, 1, {}, 4411, 8411, 4411),
    (26, 240, 26, 16384, B, 4, 1, {}, 8411, 16411, 4411),
    (26, 256, 26, 16384, B, 0, 1, {}, 8811, 16811, 4811),
    # level 0 on the full (i, j) grid: x3_sym 0, or a field count without folded kernels (x_prev is x0 in the plain kernels)
    (22, 100, 22, 16384, F, 0, 2, {}, 4830, 8830, 4830),
    (26, 256, 26, 3000, B, 0, 2, {}, 8410, 16410, 4810),
    (8, 100, 8, 16384, F, 0, 1, {}, 4830, 8830, 4830),
    (40, 64, 40, 2000, F, 0, 1, {}, 2430, 4430, 0),
    (18, 225, 18, 16420, B, 0, 1, {}, 8810, 16810, 4810),
    # instances only dX has, boundaries, options, and the fallbacks (probe 0) that must stay correct
    (8, 20, 13, 3000, F, 0, 0, {}, 0, 2430, 0),              # H <= 32: fp32 forward, dX HBT 2
    (30, 32, 9, 16384, F, 0, 0, {}, 0, 2430, 0),             # HBT 2 has 4 waves only
    (12, 64, 17, 2048, B, 0, 0, {}, 0, 4410, 0),             # bf16 H = 64: fp32 forward and dW
    (12, 65, 17, 2048, B, 0, 0, {}, 4410, 8410, 4810),       # bf16 H = 65
    (20, 48, 7, 16384, B, 0, 0, {}, 0, 4410, 0),             # bf16 HBT 4 has 4 waves only
    (4, 100, 9, 3000, F, 0, 0, {}, 0, 8430, 4830),           # m < 8: fp32 forward
    (6, 200, 5, 16384, B, 0, 0, {}, 0, 16810, 4810),
    (6, 40, 6, 2000, F, 0, 1, {}, 0, 4430, 0),
    (10, 100, 7, 28, F, 0, 0, {}, 4430, 8430, 0),            # N < 32: fp32 dW
    (20, 100, 5, 20, B, 0, 0, {}, 4410, 8410, 0),
    (25, 100, 7, 3000, F, 0, 0, {}, 0, 8430, 4830),          # odd m: fp32 forward, the dX kernel's odd last tile
    (13, 130, 11, 16384, B, 0, 0, {}, 0, 16810, 4810),
    (50, 200, 3, 16384, F, 0, 0, {}, 0, 16430, 4830),        # m > 48: the 8-wave dX does not fit LDS
    (66, 150, 2, 16384, B, 0, 0, {}, 0, 16410, 4810),        # bf16: m > 64
    (34, 200, 7, 3000, F, 0, 0, {"x3_fwd_mt": 2}, 2430, 16430, 4830),
]


def _row_id(r):
    opts = "".join("-%s%d" % (k, v) for k, v in sorted(r[7].items()))
    return "m%d-H%d-Hp%d-N%d-%s-w%d-l0%d%s" % (r[0], r[1], r[2], r[3], {F: "f16x3", B: "bf16"}[r[4]], r[5], r[6], opts)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _p(t):
    return None if t is None else t.data_ptr()


@contextlib.contextmanager
def _options(**kv):
    """library options for one test; every one is restored afterwards"""
    from xdfm_amd import _lib
    old = {k: _lib.get_option(k) for k in kv}
    try:
        for k, v in kv.items():
            _lib.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            _lib.set_option(k, v)


def _inputs(m, H, Hp, N, fold, family, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)

    def ints(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g, device=dev).float()

    def normal(scale, *shape):
        return torch.randn(shape, generator=g, device=dev) * scale

    if family == "exact":
        W, bias, x0, dOut = ints(-4, 4, H, Hp * m), ints(-8, 8, H), ints(-3, 3, m, N), ints(-3, 3, H, N)
        xp = x0 if fold else ints(-3, 3, Hp, N)
    else:
        W, bias, x0, dOut = normal(0.1, H, Hp * m), normal(0.1, H), normal(1.0, m, N), normal(1.0, H, N)
        xp = x0 if fold else normal(1.0, Hp, N)
    return W, bias, xp, x0, dOut, ints(-5, 5, Hp, N), ints(-5, 5, m, N)


def _contraction(W, bias, xp, x0, dOut):
    """float64: pre-activation W @ Z + b, dX of (W @ Z) . dOut by autograd (x_prev and x0 as separate leaves, also when
    x_prev is x0), dW = dOut @ Z^T"""
    xpd = xp.double().requires_grad_(True)
    x0d = x0.double().requires_grad_(True)
    Z = (xpd[:, None, :] * x0d[None, :, :]).reshape(xp.shape[0] * x0.shape[0], -1)
    pre = W.double() @ Z
    (pre * dOut.double()).sum().backward()
    return pre.detach() + bias.double()[:, None], xpd.grad, x0d.grad, dOut.double() @ Z.detach().t()


def _compare(got, want, mag, family, k, what):
    """exact: bit for bit; normal: |got - want| <= k * mag + 2^-24 |want| per element.  Returns the worst
    (|got - want| - 2^-24 |want|) / mag: the error beyond the rounding of the stored value, per unit of mag."""
    got = got.double()
    assert bool(torch.isfinite(got).all()), what + ": not finite"
    err = (got - want).abs()
    if family == "exact":
        bad = err != 0
        if bool(bad.any()):
            i = int(bad.flatten().nonzero()[0])
            raise AssertionError("%s: %d of %d elements differ from the exact result (first: flat %d, %r != %r)" % (
                what, int(bad.sum()), bad.numel(), i, float(got.flatten()[i]), float(want.flatten()[i])))
        return 0.0
    excess = err - 2.0 ** -24 * want.abs()
    over = excess > k * mag + 1e-30
    ratio = float((excess / (mag + 1e-300)).max())
    assert not bool(over.any()), "%s: %d elements over the bar, worst |got - ref| / mag = %.3g (K = %.3g)" % (
        what, int(over.sum()), ratio, k)
    return ratio


def _same_bits(a, b, what):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what + ": a second call gave other bits"


def run_row(row, family, k=None):
    """All three directions of one SWEEP row; returns {tensor: max |got - ref| / mag} (normal family)."""
    from xdfm_amd import _lib
    lib = _lib.load()
    dev = _dev()
    st = torch.cuda.current_stream().cuda_stream
    m, H, Hp, N, math, waves, fold, opts, want_fwd, want_bwx, want_bww = row
    k = K[math] if k is None else k
    seed = ((m * 1009 + H) * 1009 + Hp) * 100003 + N * 3 + fold + 17 * math
    W, bias, xp, x0, dOut, pre_p, pre_0 = _inputs(m, H, Hp, N, fold, family, seed, dev)
    out_r, dxp_r, dx0_r, dW_r = _contraction(W, bias, xp, x0, dOut)
    if family == "normal":
        out_m, dxp_m, dx0_m, dW_m = _contraction(W.abs(), bias.abs(), xp.abs(), x0.abs(), dOut.abs())
    else:
        out_m = dxp_m = dx0_m = dW_m = None
    ratios = {}
    with _options(cin_math=math, x3_waves=waves, x3_sym=0 if fold == 2 else 1, last_fwd_inst=-1, last_bwx_inst=-1,
                  last_bww_inst=-1, **opts):
        # ---- forward (ReLU)
        pack = torch.empty(lib.xdfm_cin_fwd_pack_elems(H, Hp, m), dtype=torch.float32, device=dev)
        _lib.check(lib.xdfm_cin_fwd_pack(_p(W), H, Hp, m, _p(pack), st), "cin_fwd_pack")
        out = torch.full((H, N), 7.0, device=dev)
        _lib.check(lib.xdfm_cin_level_fwd(_p(xp), _p(x0), _p(pack), _p(bias), H, Hp, m, N, 1, _p(out), st), "cin_level_fwd")
        assert (_lib.get_option("last_fwd_inst"), _lib.get_option("last_fwd_kernel")) == (want_fwd, math if want_fwd else 0)
        ratios["out"] = _compare(out, torch.relu(out_r), out_m, family, k, "out")

        # ---- dX: stored (flags 3) and accumulated (flags 0) onto non-zero prefills, each twice
        wz = torch.empty(lib.xdfm_cin_bwd_pack_elems(H, Hp, m), dtype=torch.float32, device=dev)
        _lib.check(lib.xdfm_cin_bwd_pack(_p(W), H, Hp, m, _p(wz), st), "cin_bwd_pack")

        def bwx(flags):
            dxp, dx0 = pre_p.clone(), pre_0.clone()
            _lib.check(lib.xdfm_cin_level_bwd_x_ex(_p(dOut), _p(xp), _p(x0), _p(wz), H, Hp, m, N, _p(dxp), _p(dx0), flags, st),
                       "cin_level_bwd_x")
            return dxp, dx0

        for flags in (3, 0):
            (dxp, dx0), (dxp2, dx02) = bwx(flags), bwx(flags)
            _same_bits(dxp, dxp2, "dxp")
            _same_bits(dx0, dx02, "dx0")
            base_p, base_0 = (0.0, 0.0) if flags else (pre_p.double(), pre_0.double())
            what = "flags %d: " % flags
            if want_bwx % 10 == 1:
                # folded level 0: the whole gradient in dx0, dxp zero-filled when it is set, untouched otherwise
                assert torch.equal(dxp, torch.zeros_like(dxp) if flags else pre_p), what + "dxp of the folded kernel"
                ratios["dx0"] = _compare(dx0, base_0 + dxp_r + dx0_r, None if dxp_m is None else dxp_m + dx0_m, family, k,
                                         what + "dx0 (folded)")
            else:
                ratios["dxp"] = _compare(dxp, base_p + dxp_r, dxp_m, family, k, what + "dxp")
                ratios["dx0"] = _compare(dx0, base_0 + dx0_r, dx0_m, family, k, what + "dx0")
        assert (_lib.get_option("last_bwx_inst"), _lib.get_option("last_bwx_kernel")) == (want_bwx, math if want_bwx else 0)

        # ---- dW: the stand-alone entry point, each twice
        ws = torch.empty(max(lib.xdfm_cin_bwd_w_ws_elems(H, Hp, m, N), 1), dtype=torch.float32, device=dev)

        def bww():
            dW = torch.full((H, Hp * m), 7.0, device=dev)
            _lib.check(lib.xdfm_cin_level_bwd_w(_p(dOut), _p(xp), _p(x0), H, Hp, m, N, _p(ws), _p(dW), st), "cin_level_bwd_w")
            return dW

        dW, dW2 = bww(), bww()
        _same_bits(dW, dW2, "dW")
        assert (_lib.get_option("last_bww_inst"), _lib.get_option("last_bww_kernel")) == (want_bww, math if want_bww else 0)
        ratios["dW"] = _compare(dW, dW_r, dW_m, family, k, "dW")
        if want_bww % 10 == 1:
            d3 = dW.view(H, m, m)
            assert torch.equal(d3, d3.transpose(1, 2)), "folded dW is not exactly symmetric"
        if want_bww:
            # the prepared path: a linear level whose dOut is its hidden gradient (dOut = dHid), formed by xdfm_cin_bwd_prep
            # together with the dW kernel's fp16 planes and per-n-split scales
            D = 4
            ws2 = torch.empty(lib.xdfm_cin_bwd_w_ws_elems(H, Hp, m, N), dtype=torch.float32, device=dev)
            dws = torch.empty(lib.xdfm_cin_bwd_prep_ws_elems(H, Hp, m, N // D, D), dtype=torch.float32, device=dev)

            def prepared():
                dO2, dbias, flag = torch.empty((H, N), device=dev), torch.empty(H, device=dev), ctypes.c_int(0)
                _lib.check(lib.xdfm_cin_bwd_prep(_p(dOut), None, 0, H, N // D, D, 0, _p(dOut), 0, H, None, 0, 0, 0, 0, 0, _p(dO2),
                                                 _p(dbias), _p(dws), _p(xp), _p(x0), Hp, m, _p(ws2), ctypes.byref(flag), st),
                           "cin_bwd_prep")
                assert flag.value == 1, "the fused dOut pass did not prepare the dW operands"
                dW = torch.full((H, Hp * m), 7.0, device=dev)
                _lib.check(lib.xdfm_cin_level_bwd_w_prepared(_p(dO2), _p(xp), _p(x0), H, Hp, m, N, _p(ws2), _p(dW), st),
                           "cin_level_bwd_w_prepared")
                return dW

            dWp, dWp2 = prepared(), prepared()
            _same_bits(dWp, dWp2, "dW (prepared)")
            assert _lib.get_option("last_bww_inst") == want_bww
            ratios["dW prepared"] = _compare(dWp, dW_r, dW_m, family, k, "dW (prepared)")
            if want_bww % 10 == 1:
                d3 = dWp.view(H, m, m)
                assert torch.equal(d3, d3.transpose(1, 2)), "folded dW (prepared) is not exactly symmetric"
    return ratios


@pytest.mark.parametrize("family", ["exact", "normal"])
@pytest.mark.parametrize("row", SWEEP, ids=[_row_id(r) for r in SWEEP])
def test_cin_instance_vs_float64(row, family):
    run_row(row, family)


@pytest.mark.parametrize("math", [F, B], ids=["f16x3", "bf16"])
@pytest.mark.parametrize("m,H,Hp,N,last", [(8, 272, 13, 3000, {F: 0, B: 0}), (26, 300, 9, 16384, {F: 4830, B: 4410})])
def test_dx_of_more_than_256_rows_is_split_across_calls(m, H, Hp, N, last, math):
    """dX takes at most 256 rows of the contraction per call; the layer walks H in calls of 256 (xdfm_amd/ops.py), the first
    storing, the others adding.  The last call's rows (16 or 44) decide its kernel: 16 rows fall back to the fp32-MFMA
    kernel in both arithmetics, 44 run HBT 4.  Exact inputs: the sum of the calls is the float64 result bit for bit."""
    from xdfm_amd import _lib
    lib = _lib.load()
    dev = _dev()
    st = torch.cuda.current_stream().cuda_stream
    W, bias, xp, x0, dOut, _, _ = _inputs(m, H, Hp, N, 0, "exact", H + m, dev)
    _, dxp_r, dx0_r, _ = _contraction(W, bias, xp, x0, dOut)
    dxp, dx0 = torch.full((Hp, N), 3.0, device=dev), torch.full((m, N), 5.0, device=dev)
    with _options(cin_math=math, last_bwx_inst=-1):
        for h0 in range(0, H, 256):
            hc = min(256, H - h0)
            Wc, dOc = W[h0:h0 + hc].contiguous(), dOut[h0:h0 + hc].contiguous()
            wz = torch.empty(lib.xdfm_cin_bwd_pack_elems(hc, Hp, m), dtype=torch.float32, device=dev)
            _lib.check(lib.xdfm_cin_bwd_pack(_p(Wc), hc, Hp, m, _p(wz), st), "cin_bwd_pack")
            _lib.check(lib.xdfm_cin_level_bwd_x_ex(_p(dOc), _p(xp), _p(x0), _p(wz), hc, Hp, m, N, _p(dxp), _p(dx0),
                                                   3 if h0 == 0 else 0, st), "cin_level_bwd_x")
        assert _lib.get_option("last_bwx_inst") == last[math]
        assert _lib.get_option("last_bwx_kernel") == (math if last[math] else 0)
    _compare(dxp, dxp_r, None, "exact", 0.0, "dxp")
    _compare(dx0, dx0_r, None, "exact", 0.0, "dx0")


@pytest.mark.parametrize("math", [F, B], ids=["f16x3", "bf16"])
@pytest.mark.parametrize("m,D,waves", [(8, 4, 0), (8, 16, 4), (18, 8, 0), (18, 32, 4), (40, 32, 0), (40, 16, 4)])
def test_cin_layer_rows_vs_oracle_at_8_waves(m, D, waves, math):
    """deepctr.layers.CIN (256, 96) at B * D >= 16384 -- the fused path the model runs: xdfm_cin_pack_all, the forward's
    epilogues (direct-connect sums at D, ReLU sign bits), xdfm_cin_bwd_prep, the dX kernel forming dOut itself and the
    prepared dW -- at field counts other than BASELINE's, with 8 waves (x3_waves 0) and 4 (x3_waves 4).  As in
    test_full_size_cin_rows_vs_oracle_subset: 48 rows of the full launch against the oracle run on those rows, gradients
    through a gout that is zero elsewhere.  f16x3 (ReLU) at that test's fp32 bars; bf16 (linear) at the bars of
    test_cin_bf16_mfma_path_vs_fp32_oracle."""
    import numpy as np
    from deepctr.layers import CIN
    from oracle import xdeepfm_oracle as orc
    from xdfm_amd import _lib
    dev = _dev()
    Bn = 16384 // D + 3
    act = "relu" if math == F else "linear"
    torch.manual_seed(m * 100 + D)
    layer = CIN(m, (256, 96), act, True, 0.0, 1024, device="cpu")
    x = torch.randn(Bn, m, D) * 0.5
    rows = torch.randperm(Bn)[:48]
    W = [c.weight.detach().clone().requires_grad_(True) for c in layer.conv1ds]
    Bs = [c.bias.detach().clone().requires_grad_(True) for c in layer.conv1ds]
    xs = x[rows].clone().requires_grad_(True)
    want = orc.cin_forward(xs, W, Bs, True, act)
    gsub = torch.randn(want.shape)
    (want * gsub).sum().backward()
    layer = layer.to(dev)
    xg = x.to(dev).requires_grad_(True)
    nt = 3 if math == F else 1
    nw = 4 if waves == 4 else 8
    with _options(cin_math=math, x3_waves=waves, last_fwd_inst=-1, last_bwx_inst=-1, last_bww_inst=-1):
        out = layer(xg)
        # the last forward launch is level 1 (H 96: MT 4), the last dX and dW launches level 0 (H 256: HBT 16, dW)
        assert _lib.get_option("last_fwd_inst") == (4000 + 10 * nt + 100 * (nw if nt == 3 else 4))
        gout = torch.zeros(Bn, want.shape[1])
        gout[rows] = gsub
        (out * gout.to(dev)).sum().backward()
        assert _lib.get_option("last_bwx_inst") == 16000 + 100 * nw + 10 * nt
        assert _lib.get_option("last_bww_inst") == 4000 + 100 * nw + 10 * nt
    r = rows.to(dev)
    pairs = [("dx rows", xg.grad[r], xs.grad)] + [("dw%d" % i, c.weight.grad, W[i].grad) for i, c in enumerate(layer.conv1ds)] + \
        [("db%d" % i, c.bias.grad, Bs[i].grad) for i, c in enumerate(layer.conv1ds)]
    mask = torch.ones(Bn, dtype=torch.bool)
    mask[rows] = False
    assert float(xg.grad[mask.to(dev)].abs().max()) == 0.0      # untouched examples get exactly zero
    if math == F:
        np.testing.assert_allclose(out[r].detach().cpu().numpy(), want.detach().numpy(), rtol=2e-5, atol=2e-6, err_msg="out rows")
        for what, got, w in pairs:
            w = w.detach().numpy()
            np.testing.assert_allclose(got.detach().cpu().numpy(), w, rtol=2e-4, atol=2e-5 * float(np.abs(w).max()) + 1e-9,
                                       err_msg=what)
        return

    def rel(got, w):
        w = w.detach().numpy()
        return float(np.abs(got.detach().cpu().numpy() - w).max() / np.abs(w).max())

    def cos(got, w):
        a, b = got.detach().cpu().numpy().ravel().astype(np.float64), w.detach().numpy().ravel().astype(np.float64)
        return float(a @ b / np.sqrt((a @ a) * (b @ b)))

    assert rel(out[r], want) < 2e-2, rel(out[r], want)
    for what, got, w in pairs:
        assert cos(got, w) > 0.998 and rel(got, w) < 4e-2, (what, cos(got, w), rel(got, w))
