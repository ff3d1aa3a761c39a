"""CPU: register budget of the tape-writing step kernels, read from the built code object (no GPU) - the rule tests/test_kernel_resources.py applies to k_step:
four market-waves per SIMD (<= 128 VGPRs) and a hot body whose only scratch instructions sit by the cold calls of the kernel's tail."""
import os
import shutil

import pytest

from test_kernel_resources import OBJDUMP, READELF, _kernels

needs_tools = pytest.mark.skipif(not (os.path.exists(READELF) and os.path.exists(OBJDUMP) and shutil.which(os.environ.get("HIPCC", "hipcc"))),
                                 reason="needs hipcc and the ROCm LLVM tools")


@needs_tools
def test_tape_step_kernels_keep_four_waves_per_simd_and_a_scratch_free_hot_body():
    ks, bodies = _kernels()
    steps = {n: v for n, v in ks.items() if "k_tstepILb" in n}
    assert len(steps) == 4, sorted(ks)                     # two book tiles x with / without info tensors (the tallies are decided at run time)
    for n, v in steps.items():
        assert v["vgpr_count"] <= 128, (n, v)
        body = bodies[n]
        scratch = [i for i, l in enumerate(body) if "scratch_" in l]
        calls = [i for i, l in enumerate(body) if "s_swappc" in l]
        assert len(scratch) <= 6, (n, len(scratch))
        for i in scratch:
            assert min(abs(i - c) for c in calls) <= 24 and i > len(body) - 200, (n, i, len(body), body[i])
        # the record: 16-byte vector stores (two per fill)
        assert sum("global_store_dwordx4" in l for l in body) >= 2, n
    for cap in ("cap256", "cap512"):
        assert len([n for n in bodies if cap in n and "slow_tstep" in n]) == 2


@needs_tools
def test_the_other_tape_writers_exist_once_per_tile_and_fit():
    ks, _ = _kernels()
    for stem in ("k_tape_run", "k_tape_place_order"):
        inst = {n: v for n, v in ks.items() if stem in n}
        assert len(inst) == 2, (stem, sorted(inst))
        for n, v in inst.items():
            assert v["vgpr_count"] <= 128 and v["vgpr_spill_count"] <= 32, (n, v)      # (k_run_random's bound: the episode kernel keeps more state live)
    for stem in ("k_tape_offsets", "k_tape_pack", "k_tape_last", "k_tape_counts", "k_tape_episode", "k_tape_partial"):
        inst = [v for n, v in ks.items() if stem in n]
        assert len(inst) == 1 and inst[0]["vgpr_spill_count"] == 0 and inst[0]["private_segment_fixed_size"] == 0, (stem, inst)

