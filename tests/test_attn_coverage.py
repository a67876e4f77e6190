"""CPU: every kernel instance K5 (csrc/attn.hip) builds is in the GPU sweep of tests/test_gpu_attention.py, so that a
new instance cannot be added without a test."""
import os
import re

from conftest import ROOT


def _dispatch_instances():
    src = open(os.path.join(ROOT, "xdeepfm-pytorch_amd", "csrc", "attn.hip")).read()
    body = src[src.index("#define ATTN_DISPATCH"):]
    body = body[:body.index("default:")]
    found = re.findall(r"case\s+(\d+)\s*\*\s*16\s*\+\s*(\d+)\s*:\s*return\s+FN<\s*(\d+)\s*,\s*(\d+)\s*>", body)
    assert len(found) == body.count("case "), "unparsed case line in ATTN_DISPATCH"
    out = set()
    for d, nh, td, tnh in found:
        assert (d, nh) == (td, tnh), "ATTN_DISPATCH case %s * 16 + %s calls FN<%s, %s>" % (d, nh, td, tnh)
        out.add((int(d), int(nh)))
    return out


def test_every_attention_instance_is_in_the_gpu_sweep():
    from test_gpu_attention import ENVELOPE, SWEEP
    built = _dispatch_instances()
    assert len(built) >= 15
    assert set(ENVELOPE) == built, "ENVELOPE of test_gpu_attention.py != ATTN_DISPATCH instances"
    swept = {(c[0], c[1]) for c in SWEEP}
    assert swept == built, "missing from the sweep: %s; not built: %s" % (sorted(built - swept), sorted(swept - built))
    for inst in sorted(built):
        cases = [c for c in SWEEP if (c[0], c[1]) == inst]
        fwd_max, train1, train2 = ENVELOPE[inst]
        # the 512-thread variant with a key-block tail (S % 8 != 0), trained
        assert any(c[2] <= 512 and c[2] % 8 and c[7] for c in cases), inst
        # the 1024-thread variant: trained where the backward fits past 512 tokens, else its forward where that fits
        if max(train1, train2) > 512:
            assert any(c[2] > 512 and c[7] for c in cases), inst
        elif fwd_max > 512:
            assert any(c[2] > 512 for c in cases), inst
        for c in cases:
            limit = train1 if c[4] == 1 else train2
            assert c[2] <= (limit if c[7] else fwd_max), c
