"""CPU: the network kernels' instance table (tests/mlp_variants.py) is the set of objects the build compiles, every object exports its OWN copy of every entry
point of include/cda_mlp.h and mlp.Layout.fn reaches exactly that copy, the layout constants follow their closed forms at every depth - and the conditions the GPU
walk (tests/test_hip_mlp_variants.py) relies on hold on the float64 statement alone, at every variant's seed.  Nothing here launches a kernel."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mlp_variants as V      # noqa: E402


@pytest.fixture(scope="module")
def hip_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build_hip()
    from gym_continuousdoubleauction_amd import _lib
    return _lib.lib(), _lib


def _addr(fn):
    return C.cast(fn, C.c_void_p).value


def test_the_table_is_the_set_of_objects_the_build_compiles():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    from gym_continuousdoubleauction_amd import _lib, mlp
    assert len(V.VARIANTS) == 56 == len(set(V.VARIANTS)) == len(set(V.IDS))
    assert len(V.VARIANTS) == len(mlp.HIST_VARIANTS) * len(mlp.ACTIVATIONS) * 2
    built = [name for name, _ in G.mlp_variant_objects()] + ["cda_mlp"]          # (the default variant: compiled from the source on the link line)
    assert len(built) == len(set(built)) == 56
    assert set(built) == {V.object_name(*v) for v in V.VARIANTS}
    flags = dict(G.mlp_variant_objects())
    for h, act, vfs in V.VARIANTS:                                                # ... each with the flags of ITS variant
        name = V.object_name(h, act, vfs)
        if name == "cda_mlp":
            continue
        want = [f"-DCDA_MLP_HIST={h}"] + ([f"-DCDA_MLP_ACT={mlp.ACTIVATIONS.index(act)}"] if act != "tanh" else []) + (["-DCDA_MLP_VFS=1"] if vfs else [])
        assert flags[name] == want, name
    # the loader binds the same set: the unsuffixed names + mlp_variant_suffixes()
    assert {"cda_mlp" + s for s in [""] + _lib.mlp_variant_suffixes()} == set(built)
    assert V.IDS[0] == "h1-tanh" and "h6-elu-vfs" in V.IDS and "h4-linear-vfs" in V.IDS


def test_every_variant_resolves_every_entry_point_to_a_copy_of_its_own(hip_lib):
    """the dispatch check: Layout(h, act, vfs).fn(name) is the symbol <name> + this variant's suffix, and the 56 addresses of one name are pairwise distinct - two
    variants sharing an address means a suffix collapsed (e.g. _vfs dropped behind an activation's suffix)"""
    L, _lib = hip_lib
    from gym_continuousdoubleauction_amd import mlp
    raw = C.CDLL(_lib.LIB_PATH)                                                    # (a second handle: symbols looked up by the name this file forms)
    assert len(_lib.MLP_SYMBOLS) == 23
    for name in _lib.MLP_SYMBOLS:
        addrs = {}
        for h, act, vfs in V.VARIANTS:
            lay = mlp.Layout(h, act, vfs)
            a = _addr(lay.fn(name))
            assert a, (name, h, act, vfs)
            assert a == _addr(getattr(raw, name + V.object_name(h, act, vfs)[len("cda_mlp"):])), (name, h, act, vfs)
            assert a == _addr(mlp.layout(h, act, vfs).fn(name))
            addrs.setdefault(a, []).append(V.variant_id((h, act, vfs)))
        shared = {hex(a): ids for a, ids in addrs.items() if len(ids) > 1}
        assert not shared and len(addrs) == 56, (name, shared)


def test_learner_entry_points_resolve_to_one_address_from_every_layout(hip_lib):
    L, _lib = hip_lib
    from gym_continuousdoubleauction_amd import mlp
    net = {_addr(mlp.layout(*v).fn(n)) for v in V.VARIANTS for n in _lib.MLP_SYMBOLS}
    for name in _lib.LEARNER_SYMBOLS:
        addrs = {_addr(mlp.Layout(*v).fn(name)) for v in V.VARIANTS}
        assert len(addrs) == 1 and addrs == {_addr(getattr(L, name))} and not addrs & net, name


#: the padded observation width per depth: whole 32-wide operand tiles at depths 2, 3, 6, a half tile at the end at 1, 4, 7, 8
KX_OF = {1: 48, 2: 96, 3: 128, 4: 176, 6: 256, 7: 304, 8: 336}
PAD_OF = {1: 6, 2: 12, 3: 2, 4: 8, 6: 4, 7: 10, 8: 0}


def test_layout_constants_follow_their_closed_forms_at_every_depth():
    from gym_continuousdoubleauction_amd import mlp
    assert tuple(sorted(KX_OF)) == tuple(mlp.HIST_VARIANTS)
    params = {}
    for h in mlp.HIST_VARIANTS:
        for act in mlp.ACTIVATIONS:
            for vfs in (False, True):
                L = mlp.Layout(h, act, vfs)
                obs = 42 * h
                assert (L.hist, L.OBS, L.KX, L.KX - L.OBS) == (h, obs, KX_OF[h], PAD_OF[h]) and L.KX % 16 == 0
                assert L.XT == -(-L.KX // 32) and (L.KX % 32 == 0) == (h in (2, 3, 6))
                assert L.PARAMS == 512 * obs + 512 + 2 * 256 * 256 + 512 + 32 * 256 + 32 + 2 == 512 * obs + 140322
                assert L.WB_ELEMS == 512 * L.KX + 4 * 256 * 256 + 4 * 32 * 256
                assert L.SLAB == 512 * 32 * L.XT + 2 * 256 * 256 + 32 * 512
                assert (L.OFF_W1, L.OFF_B1, L.OFF_W2, L.OFF_B2, L.OFF_WO, L.OFF_BO, L.OFF_LS) == (
                    0, 512 * obs, 512 * obs + 512, 512 * obs + 512 + 131072, 512 * obs + 1024 + 131072, 512 * obs + 1024 + 131072 + 8192, L.PARAMS - 2)
                assert L.suffix == V.object_name(h, act, vfs)[len("cda_mlp"):]
        params[h] = L.PARAMS
        assert mlp.layout_of_params(L.PARAMS).hist == h
    assert len(set(params.values())) == len(params)                               # unambiguous: no two depths share a parameter count
    assert sum(1 for hh in mlp.HIST_VARIANTS if mlp.layout(hh).PARAMS == params[6]) == 1


# ---- what the suite compared with the float64 statement before the walk: the parametrize lists of the four files, as literals -------------------------------------
COVERED_BEFORE = (
    [(4, "tanh", False)]                                                                        # tests/test_hip_mlp.py: the unsuffixed default
    + [(h, "tanh", False) for h in (1, 2, 3, 6, 7, 8)]                                          # tests/test_hip_hist.py DEPTHS
    + [(h, a, False) for h in (1, 4, 8) for a in ("relu", "elu", "linear")]                     # tests/test_hip_activation.py
    + [(h, a, True) for h in (1, 4, 8) for a in ("tanh", "elu", "relu")]                        # tests/test_hip_vf_share.py (forward: tanh / elu, backward: tanh / relu)
    + [(4, "tanh", False), (1, "relu", False), (8, "tanh", True), (4, "relu", True), (4, "tanh", False), (8, "relu", False), (1, "tanh", True)])   # test_hip_sampler.py STEP_CASES


def test_print_the_variants_no_earlier_numeric_test_names():
    covered = set(COVERED_BEFORE)
    assert covered <= set(V.VARIANTS)
    uncovered = [v for v in V.VARIANTS if v not in covered]
    print("\n[mlp variants] not compared with the float64 statement before tests/test_hip_mlp_variants.py (%d of %d): %s"
          % (len(uncovered), len(V.VARIANTS), " ".join(V.variant_id(v) for v in uncovered)))
    mid = [v for v in uncovered if v[0] in (2, 3, 6, 7)]
    assert len([v for v in mid if v[1] != "tanh"]) == 24 and [v for v in mid if v[1] == "tanh"] == [(h, "tanh", True) for h in (2, 3, 6, 7)]
    assert [v for v in uncovered if v[0] not in (2, 3, 6, 7)] == [(h, "linear", True) for h in (1, 4, 8)]
    assert len(uncovered) == 31


@pytest.mark.parametrize("h", [h for h in KX_OF])
def test_the_reference_alone_meets_the_conditions_the_walk_relies_on(h):
    """at every variant's seed and input, on the float64 statement: a relu network's stored h1 is zero in more than a fifth of its entries; a non-tanh network's
    outputs differ from the tanh network's of the same parameters by far more than 1e-2 + both kernels' error bounds; a shared trunk's value column differs from
    the separate network's; the head setting alternates over every axis"""
    from gym_continuousdoubleauction_amd import mlp
    x = V.obs(V.N_FWD, h)
    for vfs in (False, True):
        refs = {}
        for act in mlp.ACTIVATIONS:
            sd = V.head_on(h, act, vfs)
            th = V.theta(h, vfs, V.seed_of(h), 2.0, sd)
            assert mlp.has_log_std_head(th) == sd
            out, _, h1, h2 = mlp.reference_outputs(th, x, keep=True, activation=act, vf_share_layers=vfs)
            tanh_out = mlp.reference_outputs(th, x, activation="tanh", vf_share_layers=vfs)
            refs[act] = out
            hmax = max(1.0, float(h1.abs().max()), float(h2.abs().max()))
            bound = 2e-2 * max(1.0, float(h2.abs().max())) if vfs else 3e-3 * max(1.0, float(out.abs().max())) * hmax
            tanh_bound = 2e-2 if vfs else 3e-3 * max(1.0, float(tanh_out.abs().max()))
            if act != "tanh":
                diff = float((out[:, :25] - tanh_out[:, :25]).abs().max())
                print(f"\n[mlp variants] {V.variant_id((h, act, vfs))}: differs from tanh by {diff:.3g} (kernel bounds {bound:.3g} + {tanh_bound:.3g})")
                assert diff > 1e-2 + bound + tanh_bound, (act, vfs, diff)
            if act == "relu":
                share = float((h1[:, :V.H] == 0).double().mean())
                assert share > 0.25 and bool((h1 >= 0).all()), share                    # (0.2 asserted of the kernel's image, whose flipped share is < 0.02)
            if vfs:
                sep = mlp.reference_outputs(th, x, activation=act)
                d24 = float((sep[:, 24] - out[:, 24]).abs().max())
                assert d24 > 1e-2 + bound, (act, d24)
            if not sd:
                assert bool((out[:, 25:] == 0).all())
            else:
                assert float(out[:, 25:27].abs().max()) > 0 and bool((out[:, 27:] == 0).all())
    heads = [V.head_on(*v) for v in V.VARIANTS]
    for axis, values in ((0, mlp.HIST_VARIANTS), (1, mlp.ACTIVATIONS), (2, (False, True))):
        for val in values:
            assert {hd for v, hd in zip(V.VARIANTS, heads) if v[axis] == val} == {False, True}, (axis, val)
