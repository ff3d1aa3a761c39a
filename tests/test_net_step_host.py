"""CPU: the k_net_step family (csrc/cda_kernels.inc: the one-launch rollout step of every network but the default one) as built - its instance count, its register
budget (k_policy_step's: four market-waves per SIMD), its MFMA count (the activation is chosen in the epilogues, never around the MFMA layers), its names against the
stems other host tests count - and the C-ABI of include/cda.h cda_net_step_* without a device."""
import ctypes as C
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_kernel_resources as KR  # noqa: E402

STEM = "k_net_step"
# stems that the other host tests count or exclude kernels by: no instance of the new family may carry one
FOREIGN_STEMS = ("k_policy_step", "k_stepILb", "k_tstepILb", "k_tape_", "k_script_actions", "k_script_label", "order_stream", "sched_orders", "k_place_order",
                 "k_run_random", "k_reset", "k_mlp_")
# layer 1's k-steps per compiled history depth (KX / 16: test_kernel_resources.py)
DEPTH_K1 = {"k_net_stepI": 11, "k_net_step_h1I": 3, "k_net_step_h2I": 6, "k_net_step_h3I": 8, "k_net_step_h6I": 16, "k_net_step_h7I": 19, "k_net_step_h8I": 21}


@pytest.mark.skipif(not (os.path.exists(KR.READELF) and os.path.exists(KR.OBJDUMP) and shutil.which(os.environ.get("HIPCC", "hipcc"))),
                    reason="needs hipcc and the ROCm LLVM tools")
def test_net_step_instances_keep_the_policy_steps_budget():
    ks, bodies = KR._kernels()
    net = {n: v for n, v in ks.items() if STEM in n}
    assert len(net) == 14, sorted(net)                           # one per compiled history depth x with / without the tallies - NOT one per (activation, trunk) pair
    seen = set()
    for n, v in net.items():
        assert not any(stem in n for stem in FOREIGN_STEMS), n
        assert v["vgpr_count"] <= 128 and v["vgpr_spill_count"] <= 2, (n, v)
        body = bodies[n]
        key = [k for k in DEPTH_K1 if k in n]
        assert len(key) == 1, n
        seen.add(key[0])
        assert sum("v_mfma_f32_32x32x16_bf16" in l for l in body) <= DEPTH_K1[key[0]] + 32, n        # layer 1, layer 2, heads: once each, whatever the activation
        scratch = [i for i, l in enumerate(body) if "scratch_" in l]
        calls = [i for i, l in enumerate(body) if "s_swappc" in l]
        assert len(scratch) <= 6 and all(min(abs(i - c) for c in calls) <= 24 and i > len(body) - 200 for i in scratch), (n, len(scratch))
    assert seen == set(DEPTH_K1)
    # what the other tests count is what it was: 14 policy-step instances, the general build twice per tile
    assert sum("k_policy_step" in n for n in ks) == 14
    for cap in ("cap256", "cap512"):
        assert len([n for n in bodies if cap in n and "slow_step" in n]) == 2


@pytest.fixture(scope="module")
def hip_lib():
    import __graft_entry__ as g
    g.build_hip()
    from gym_continuousdoubleauction_amd import _lib
    return _lib.lib()


def test_the_four_symbols_load_and_refuse_without_a_device(hip_lib):
    L = hip_lib
    INVALID = -1
    for name in ("cda_net_step_supported", "cda_net_step_advised", "cda_net_step_range", "cda_policy_step_launch_count"):
        assert hasattr(L, name), name
    one = C.c_void_p(64)                                         # non-NULL, never dereferenced: validation fails first
    tail = (0, 8, one, one, one, 1, one, 0, *([one] * 5), *([one] * 5), *([one] * 4), None, 0, None, None, None)
    assert len(L.cda_net_step_range.argtypes) == len(L.cda_policy_step_range.argtypes) + 2
    for act, vfs in ((1, 0), (0, 1), (3, 1), (0, 0)):
        assert L.cda_net_step_range(None, act, vfs, *tail) == INVALID                 # no env
        assert L.cda_net_step_supported(None, act, vfs) == 0 and L.cda_net_step_advised(None, act, vfs) == 0
    for act, vfs in ((4, 0), (-1, 0), (0, 2), (1, -1)):
        assert L.cda_net_step_range(None, act, vfs, *tail) == INVALID
        assert L.cda_net_step_range(one, act, vfs, *tail) == INVALID                  # the codes are checked before the env is looked at
        assert L.cda_net_step_supported(None, act, vfs) == INVALID and L.cda_net_step_advised(None, act, vfs) == INVALID
    assert L.cda_policy_step_launch_count(None) == 0
