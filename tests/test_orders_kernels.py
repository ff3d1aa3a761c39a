"""CPU: the order-stream kernels in the built code object (no GPU) - they exist once per book tile, keep four market-waves per SIMD (<= 128 VGPRs) and spill no
more VGPRs than the one-order hooks they replace (k_place_order / k_tape_place_order of the same tile, same build), whose matching code they inline."""
import os
import shutil

import pytest

from test_kernel_resources import OBJDUMP, READELF, _kernels

needs_tools = pytest.mark.skipif(not (os.path.exists(READELF) and os.path.exists(OBJDUMP) and shutil.which(os.environ.get("HIPCC", "hipcc"))),
                                 reason="needs hipcc and the ROCm LLVM tools")


def _one(ks, cap, stem, but=None):
    inst = {n: v for n, v in ks.items() if cap in n and stem in n and (but is None or but not in n)}
    assert len(inst) == 1, (cap, stem, sorted(inst))
    return next(iter(inst.items()))


@needs_tools
def test_order_stream_kernels_exist_once_per_tile_and_fit_the_hooks_budget():
    ks, bodies = _kernels()
    assert len([n for n in ks if "order_stream" in n]) == 4, sorted(n for n in ks if "order_stream" in n)
    for cap in ("cap256", "cap512"):
        for stream, hook in (("14k_order_stream", "13k_place_order"), ("19k_tape_order_stream", "18k_tape_place_order")):
            n, v = _one(ks, cap, stream)
            _, h = _one(ks, cap, hook)
            assert v["vgpr_count"] <= 128, (n, v)
            assert v["vgpr_spill_count"] <= h["vgpr_spill_count"], (n, v["vgpr_spill_count"], h["vgpr_spill_count"])
            body = bodies[n]
            # the chunk's results (and the summary): 16-byte vector stores; the chunk's messages: 16-byte vector loads
            assert sum("global_store_dwordx4" in l for l in body) >= 2 and sum("global_load_dwordx4" in l for l in body) >= 2, n
            if "tape" in stream:
                assert sum("global_store_dwordx4" in l for l in body) >= 4, n         # ... and the fill's record: two more
    # the names leave every stem the other kernel tests count alone
    for stem in ("k_tape_place_order", "k_place_order", "k_tape_run", "k_tstepILb", "k_stepILb"):
        assert not any(stem in n for n in ks if "order_stream" in n), stem
