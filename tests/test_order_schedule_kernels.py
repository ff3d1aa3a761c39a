"""CPU: the order-schedule kernels in the built code object (no GPU) - they exist once per book tile, keep four market-waves per SIMD (<= 128 VGPRs) and spill no
more VGPRs than the one-order hooks whose matching code they inline (k_place_order / k_tape_place_order of the same tile, same build); the order-stream kernels
beside them are still four."""
import os
import shutil

import pytest

from test_kernel_resources import OBJDUMP, READELF, _kernels

needs_tools = pytest.mark.skipif(not (os.path.exists(READELF) and os.path.exists(OBJDUMP) and shutil.which(os.environ.get("HIPCC", "hipcc"))),
                                 reason="needs hipcc and the ROCm LLVM tools")


def _one(ks, cap, stem):
    inst = {n: v for n, v in ks.items() if cap in n and stem in n}
    assert len(inst) == 1, (cap, stem, sorted(inst))
    return next(iter(inst.items()))


@needs_tools
def test_schedule_kernels_exist_once_per_tile_and_fit_the_hooks_budget():
    ks, bodies = _kernels()
    sched = sorted(n for n in ks if "sched_orders" in n)
    assert len(sched) == 4, sched
    assert len([n for n in ks if "order_stream" in n]) == 4
    for cap in ("cap256", "cap512"):
        for kern, hook in (("14k_sched_orders", "13k_place_order"), ("15k_tsched_orders", "18k_tape_place_order")):
            n, v = _one(ks, cap, kern)
            _, h = _one(ks, cap, hook)
            assert v["vgpr_count"] <= 128, (n, v)
            assert v["vgpr_spill_count"] <= h["vgpr_spill_count"], (n, v["vgpr_spill_count"], h["vgpr_spill_count"])
            body = bodies[n]
            # the chunk's messages: 16-byte vector loads; the counters' row: 8-byte vector accesses, a load and a store
            assert sum("global_load_dwordx4" in l for l in body) >= 2, n
            assert any("global_load_dwordx2" in l for l in body) and any("global_store_dwordx2" in l for l in body), n
    # the names leave every stem the other kernel tests count alone
    for stem in ("order_stream", "k_tape_", "k_stepILb", "k_tstepILb", "k_policy_step", "k_place_order"):
        assert not any(stem in n for n in sched), stem
