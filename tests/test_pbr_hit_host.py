"""The oracle's per-hit material of the textured metallic-roughness model (oracle_integrator.cpp applyPbrTextures) against the float64
statement of the rule in tests/pbr_hit_domain.py, class by class.  No GPU: the oracle names the hit (mesh, triangle, bu, bv, t) and
the reference computes everything else from the scene as given to the C ABI.

Three things are held: the branch outcomes of unguarded rows agree; no class leaves more than 2 % of its rows out as too near a
threshold; and the oracle's largest difference from the reference per class is no larger than the committed ORACLE_MEASURED, from
which tests/test_gpu_pbr_hit.py derives the device's bounds.
"""
import numpy as np
import pytest

import oracle_lib as ol
import pbr_hit_domain as D

_results = {}
_oracles = {}


def oracle_of(sc):
    if id(sc) not in _oracles:
        _oracles[id(sc)] = ol.OracleScene(sc)
    return _oracles[id(sc)]


def run(name):
    """(scene, rows, the oracle's rows, the reference at the oracle's hits, their differences) of a class, computed once."""
    if name not in _results:
        sc, rows = D.class_rows(name)
        got = oracle_of(sc).pbr_hits(rows)
        ref = D.reference(sc, rows, got)
        _results[name] = (sc, rows, got, ref, D.differences(ref, got))
    return _results[name]


ALL = list(D.CLASSES)


def test_every_class_is_in_a_group_and_has_a_measured_entry():
    grouped = [c for g in D.GROUPS.values() for c in g]
    assert sorted(grouped) == sorted(ALL)
    assert sorted(D.ORACLE_MEASURED) == sorted(ALL)


@pytest.mark.parametrize("name", ALL)
def test_rows_hit_and_few_are_guarded(name):
    sc, rows, got, ref, d = run(name)
    assert rows.shape == (D.ROWS, 20)
    assert d["rows"] >= D.ROWS * 3 // 4, "rays that miss their patch"
    if name == "material/not-pbr":
        assert d["textured"] == 0 and not (got["textured"] > 0).any()
        return
    assert d["textured"] == d["rows"]
    # the 2 % condition, on the reference alone
    assert d["guarded"] <= 0.02 * d["textured"], {k: int((ref["guards"][k] < v).sum()) for k, v in D.GUARD.items()}


@pytest.mark.parametrize("name", ALL)
def test_branch_outcomes_agree(name):
    sc, rows, got, ref, d = run(name)
    bad = d["branch_mismatches"]
    assert len(bad) == 0, (len(bad), bad[:8], ref["basis"][bad[:8]], got["basis"][bad[:8]], ref["discard"][bad[:8]], got["discard"][bad[:8]])
    # what the surface record reports, which the reference restates as well
    hit = got["hit"] > 0
    use = hit & (ref["guards"]["front"] >= D.GUARD["front"]) & (ref["guards"]["hit_flip"] >= D.GUARD["hit_flip"])
    assert np.array_equal(ref["front_face"][use], got["front_face"][use] > 0)
    # (the patches lie up to 250 units from the origin with edges of 1 .. 2: a float32 edge vector carries 250 x 2^-23 = 3e-5)
    assert D.angle(ref["geometric_normal"][use], got["geometric_normal"][use]).max() < 1e-4
    assert D.angle(ref["hit_normal"][use], got["hit_normal"][use]).max() < 1e-4


@pytest.mark.parametrize("name", ALL)
def test_oracle_within_committed_measure(name):
    sc, rows, got, ref, d = run(name)
    committed = D.ORACLE_MEASURED[name]
    print(name, {k: d[k] for k in ("colour", "scalar", "normal")}, "compared", d["compared"], "guarded", d["guarded"])
    for k in ("colour", "scalar", "normal"):
        assert d[k] <= committed[k], (k, d[k], committed[k])
        assert np.isfinite(d[k])


def _of_material(rows, *names):
    wanted = rows.view(np.uint32)[:, 9]
    return np.isin(wanted, [D.MAT[n] for n in names])


def test_classes_take_the_paths_they_are_named_for():
    """Each class is only worth its name if its rows decide the way the name says: asserted on the reference's outcomes."""
    basis = lambda name: run(name)[3]["basis"][run(name)[2]["hit"] > 0]
    assert set(basis("tangent/vertex") & 3) == {1}
    assert set(basis("tangent/none-at-all") & 3) == {2}
    sc, rows, got, ref, d = run("tangent/none")
    hit = got["hit"] > 0
    assert [set(ref["basis"][hit & (got["mesh"] == m)] & 3) for m in range(4)] == [{2}, {1}, {3}, {1}]   # meshes 2, 3: no uv set at all
    sc, rows, got, ref, d = run("tangent/untrusted")
    hit = got["hit"] > 0
    assert set(ref["basis"][hit & (got["mesh"] == 0)] & 3) == {2}                  # w = 0: never trusted
    assert set(ref["basis"][hit & (got["mesh"] == 1)] & 3) == {1, 2}               # |tsign| on both sides of 0.5
    # a tangent 1e-4 .. 1e-2 rad from the normal keeps its own basis (the reference's rule)
    for a in D.PARALLEL:
        assert set(basis("tangent/parallel-%.1e" % a) & 3) == {1}, a
    sc, rows, got, ref, d = run("tangent/degenerate-uv")
    hit = got["hit"] > 0
    assert set(ref["basis"][hit & (got["mesh"] < 4)] & 3) == {3} and set(ref["basis"][hit & (got["mesh"] == 4)] & 3) == {2}
    flat = hit & ((got["mesh"] == 2) | (got["mesh"] == 3))
    assert (np.abs(ref["hit_normal"][flat][:, 2]) > 0.999).all() and (np.abs(ref["hit_normal"][hit & (got["mesh"] < 2)][:, 2]) < 0.999).all()
    for name in ("transform/mirrored", "transform/sheared"):
        assert set(basis(name) & 3) == {1, 2}
    # from behind, the mapped normal stays on the viewer's side: it is turned only where the map tips it below the surface
    for name in ("side/back", "transform/mirrored", "normal/zero"):
        sc, rows, got, ref, d = run(name)
        keep = (got["hit"] > 0) & ~ref["discard"]
        back = keep & ~ref["front_face"]
        assert back.sum() > 500
        facing = np.where(ref["front_face"][:, None], ref["geometric_normal"], -ref["geometric_normal"])
        assert (np.sum(ref["normal"] * facing, axis=1)[keep] >= 0.0).all()
        assert ((ref["basis"][back] & 4) != 0).mean() < 0.25, name
    assert set(basis("normal/zero") & 3) == {1, 2, 3}
    sc, rows, got, ref, d = run("bary/edges")
    hit = got["hit"] > 0
    w = np.stack([1.0 - got["bu"] - got["bv"], got["bu"], got["bv"]], axis=1)[hit]
    assert (w.min(axis=1) < 0.0).sum() > 100 and (w.min(axis=1) == 0.0).sum() > 100 and (w.max(axis=1) > 0.999999).sum() > 100
    # the normal-scale switch sits between 1e-4 and 1.0001e-4
    sc, rows, got, ref, d = run("material/normal-scale")
    hit = got["hit"] > 0
    for i, on in enumerate((False, False, True, True, True, False)):
        b = ref["basis"][hit & _of_material(rows, "nscale%d" % i)]
        assert len(b) > 100 and ((b != 0).all() if on else (b == 0).all()), i
    # the 33x7 and 16x16 chains are read on every level
    sc, rows, got, ref, d = run("footprint")
    hit = (got["hit"] > 0) & (got["mesh"] == 0)
    for column, levels in ((0, 5), (1, 6)):
        lods = ref["lods"][hit][:, column]
        assert set(np.floor(lods).astype(int)) == set(range(levels)) and (lods == levels - 1).any() and (lods == 0).any()
    assert (ref["lods"][(got["hit"] > 0) & (got["mesh"] == 1)] == 0.0).all()       # uv-per-world 0
    cos = np.abs(np.sum(ref["geometric_normal"] * D._unit(rows[:, 3:6].astype(np.float64)), axis=1))[got["hit"] > 0]
    assert (cos < 1e-3).sum() > 50 and (cos > 0.9).sum() > 50


def test_gradient_rows_are_rarely_guarded():
    """grad/given runs on the device only (the oracle has no gradient path), but its 2 % condition is the reference's alone: at the
    oracle's hits, which do not depend on the instantiation."""
    sc, rows = D.gradient_class_rows()
    ref = D.reference(sc, rows, oracle_of(sc).pbr_hits(rows))
    near = {k: int((ref["guards"][k] < v).sum()) for k, v in D.GUARD.items()}
    assert D.guarded(ref).sum() <= 0.02 * D.ROWS, near
    # gradient samples with their tap count decided, and the variance term inside and outside its window
    assert np.isfinite(ref["guards"]["aniso_ceil"]).sum() > D.ROWS // 4 and np.isfinite(ref["guards"]["grad_window"]).sum() > D.ROWS // 8
    valid = rows.view(np.uint32)[:, 19]
    assert set(valid) == {1, 2, 3} and (rows.view(np.uint32)[:, 10] == 1).all()


def test_python_mirrors_the_probe_header():
    """include/ptr_debug_pbr.h has a signature table of its own: the tables of ptr_abi.h and ptr_debug.h keep their sizes."""
    import ctypes as C
    import os
    import re

    text = open(os.path.join(ol.ROOT, "include", "ptr_debug_pbr.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = {name: params.count(",") + 1 for name, params in re.findall(r"\b(ptr_[a-z_]+)\s*\(([^()]*)\)\s*;", text)}
    assert set(declared) == set(D.pt.PBR_HIT_SYMBOLS) == {"ptr_debug_pbr_hits"}
    assert not set(D.pt.PBR_HIT_SYMBOLS) & (set(D.pt.ABI_SYMBOLS) | set(D.pt.DEBUG_SYMBOLS))
    lib = D.pt.load_library()
    for name, count in declared.items():
        fn = getattr(lib, name)
        assert len(fn.argtypes) == count and fn.restype is C.c_int


def test_alpha_modes_draw_as_the_rule_says():
    """BLEND draws exactly once, every other mode not at all; MASK discards on both sides of the cutoff."""
    sc, rows, got, ref, d = run("material/alpha")
    hit = got["hit"] > 0
    before = rows.view(np.uint32)[:, 8]
    once, _ = D.rng_next(before)
    blend = hit & _of_material(rows, "blend")
    assert np.array_equal(got["state"][blend], once[blend]) and (once[blend] != before[blend]).all()
    assert np.array_equal(got["state"][hit & ~blend], before[hit & ~blend])
    for name in ("mask", "mask_factor", "blend"):
        m = hit & _of_material(rows, name)
        assert 0.1 < (got["discard"][m] > 0).mean() < 0.9, name
    assert not (got["discard"][hit & _of_material(rows, "opaque")] > 0).any()
    for name in D.CLASSES:
        if name != "material/alpha":
            r = run(name)
            h = r[2]["hit"] > 0
            assert np.array_equal(r[2]["state"][h], r[1].view(np.uint32)[:, 8][h]), name


def test_out_of_range_inputs_are_clamped_not_refused():
    """Factors outside [0, 1] and texture indices past the count reach the device as given: the results stay in range."""
    sc, rows, got, ref, d = run("material/factors")
    keep = (got["hit"] > 0) & ~(got["discard"] > 0)
    for f in ("roughness", "metallic", "transmission"):
        assert (got[f][keep] >= 0.0).all() and (got[f][keep] <= 1.0).all()
    a = keep & _of_material(rows, "factors_a")
    assert (got["metallic"][a] > 0.0).any() and (got["base_color"][a][:, 0] > 1.0).any()
    sc, rows, got, ref, d = run("material/texture-index")
    keep = got["hit"] > 0
    assert (got["basis"][keep] == 0).all() and (got["occlusion"][keep] == 1.0).all()
    assert np.allclose(got["base_color"][keep], [0.9, 0.8, 0.7], rtol=0, atol=1e-7)
