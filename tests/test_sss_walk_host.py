"""The float64 restatement of the random-walk subsurface path (tests/sss_walk_ref.py) against the oracle's sssWalkBegin / sssWalkStep and
its whole walk, on the input sets test_gpu_sss_walk.py puts to the device (tests/sss_walk_cases.py).  No GPU.  This is where the input sets
are shown to be fair: the share of near-tie rows of every group comes from the reference alone and stays under 2 %, and every outcome
and every branch of the two functions is taken by at least 5 % of the rows of some group."""
import os
import re

import numpy as np
import pytest

import oracle_lib as ol
import sss_walk_cases as K
import sss_walk_ref as R

pt = ol.pt

NEAR_TIE_CAP = 0.02
# test_gpu_parity.test_sample_bsdf_matches_oracle (the subsurface materials): direction atol 2e-4; weight, pdf, throughput rtol 3e-3, atol 1e-5
DIR_ATOL, RTOL, ATOL = 2e-4, 3e-3, 1e-5


def test_the_header_and_its_signature_table_agree():
    """include/ptr_debug_sss.h has a signature table of its own: the tables of ptr_abi.h and ptr_debug.h keep their sizes."""
    text = open(os.path.join(ol.ROOT, "include", "ptr_debug_sss.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = dict(re.findall(r"\bint\s+(ptr_\w+)\s*\(([^;]*)\)\s*;", text))
    assert set(declared) == set(pt.SSS_WALK_SYMBOLS) == {"ptr_debug_sss_walk_begin", "ptr_debug_sss_walk_step", "ptr_debug_sss_walks"}
    for name, args in declared.items():
        assert len(args.split(",")) == len(pt._SSS_WALK_SIGNATURES[name][1]), name
    lib = pt.load_library()
    assert all(hasattr(lib, s) for s in pt.SSS_WALK_SYMBOLS)
    assert not set(pt.SSS_WALK_SYMBOLS) & (set(pt.ABI_SYMBOLS) | set(pt.DEBUG_SYMBOLS))


def test_the_probes_refuse_before_any_launch():
    """a NULL argument, n == 0 and sssMaxSteps > 64 are refused on the host: no device is needed to be told so"""
    import ctypes as C
    lib = pt.load_library()
    material, s = K.begin_materials()["skin"], K.settings()
    rows, states = np.zeros((4, 20), np.float32), np.ones(4, np.uint32)
    out, out_states = np.zeros((4, 24), np.float32), np.zeros(4, np.uint32)
    fp, up = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)), lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    err = C.create_string_buffer(256)
    too_many = K.settings(65)
    for fn in (lib.ptr_debug_sss_walk_begin, lib.ptr_debug_sss_walk_step):
        good = (C.byref(material), C.byref(s), fp(rows), up(states), 4, fp(out), up(out_states))
        for position, value in ((0, None), (1, None), (2, None), (3, None), (4, 0), (5, None), (6, None), (1, C.byref(too_many))):
            args = list(good)
            args[position] = value
            assert fn(*args, err, len(err)) != 0, (fn.__name__, position)
            assert err.value
    xys = np.zeros((4, 3), np.uint32)
    good = (C.c_void_p(1), C.byref(s), up(xys), 4, 8, fp(out), fp(out))   # (refused before the handle is looked at)
    for position, value in ((0, None), (1, None), (2, None), (3, 0), (4, 0), (4, 65), (5, None), (6, None), (1, C.byref(too_many))):
        args = list(good)
        args[position] = value
        assert lib.ptr_debug_sss_walks(*args, err, len(err)) != 0, position


@pytest.fixture(scope="module")
def begin_results():
    """group -> (inputs, states, reference, oracle rows, oracle states), computed once"""
    s = K.settings()
    out = {}
    for group, material in K.begin_materials().items():
        inputs, states = K.begin_inputs(group)
        ref = R.begin(material, s, inputs, states)
        rows, ostates = ol.sss_walk_begin(material, s, inputs, states)
        out[group] = (material, inputs, states, ref, rows, ostates)
    return out


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    """the steps the oracle's whole walks of the sphere scene took: what the step groups draw their states from on this side"""
    host, _ = K.scene("sphere", tmp_path_factory.mktemp("sss_host"))
    steps, _ = ol.OracleScene(host).sss_walks(K.walk_settings(host), K.all_pixels(), 32)
    rows, states = K.recorded_steps(steps)
    assert len(rows) > 2000
    return rows, states


@pytest.fixture(scope="module")
def step_results(recorded):
    out = {}
    for group, (material, limit, _) in K.step_groups().items():
        rows, states, kind = K.step_inputs(group, recorded)
        ref = R.step(material, limit, rows, states)
        orows, ostates = ol.sss_walk_step(material, K.settings(limit), rows, states)
        out[group] = (material, limit, rows, states, kind, ref, orows, ostates)
    return out


def test_begin_matches_the_oracle(begin_results):
    s = K.settings()
    shares = {}
    for group, (material, inputs, states, ref, rows, ostates) in begin_results.items():
        near = R.near_ties(ref)
        assert near.mean() <= NEAR_TIE_CAP, (group, near.mean())
        ok = ~near
        got = pt.sss_fields(rows, pt.SSS_BEGIN_FIELDS)
        assert np.array_equal(got["outcome"][ok], ref["outcome"][ok]), (group, np.flatnonzero(got["outcome"] != ref["outcome"])[:8])
        assert np.array_equal(ostates[ok], ref["states"][ok]), group
        outside, excluded = K.assert_begin_values(group, got, ref, ok, material, s, inputs, states)
        assert (near | outside).mean() <= NEAR_TIE_CAP, (group, near.mean(), outside.mean())
        assert excluded.mean() <= K.EXCLUDED_CAP.get(group, 0.0), (group, excluded.mean())
        if excluded.any():
            print("%s: excluded %.4f" % (group, excluded.mean()))
        shares[group] = (float(near.mean()), float(outside.mean()), float(excluded.mean()))
        # what an outcome does not define reads 0
        assert np.all(rows[got["outcome"] == 0, 1:] == 0.0) and np.all(rows[got["outcome"] == 1, 9:] == 0.0)
    print("begin: group -> (near ties, outside the strict bound, excluded): %s" % shares)
    # the additions the one-ulp rule derives are the reference's own: they are what sss_walk_cases.DERIVED records
    assert set(K.SENSITIVITY_SEEN) == set(K.DERIVED) == set(K.SENSITIVE_BEGIN)
    for group, seen in K.SENSITIVITY_SEEN.items():
        for f, value in seen.items():
            assert abs(value - K.DERIVED[group][f]) <= 1e-4 * K.DERIVED[group][f], (group, f, value)


def test_step_matches_the_oracle(step_results):
    for group, (material, limit, rows, states, kind, ref, orows, ostates) in step_results.items():
        near = R.near_ties(ref)
        assert near.mean() <= NEAR_TIE_CAP, (group, near.mean())
        ok = ~near
        got = pt.sss_fields(orows, pt.SSS_STEP_FIELDS)
        bad = np.flatnonzero((got["outcome"] != ref["outcome"]) & ok)
        assert bad.size == 0, (group, bad[:8], kind[bad[:8]])
        assert np.array_equal(ostates[ok], ref["states"][ok]), group
        outside, excluded = K.assert_step_values(group, got, ref, ok, material, limit, rows, states)
        assert (near | outside).mean() <= NEAR_TIE_CAP, (group, near.mean(), outside.mean())
        assert excluded.mean() <= K.EXCLUDED_CAP.get(group, 0.0), (group, excluded.mean())
        if excluded.any():
            print("%s: excluded %.4f" % (group, excluded.mean()))


def test_the_draws_each_event_takes(step_results, begin_results):
    """A miss takes exactly one draw, a scatter three, a boundary event one (a scatter cut off before its direction: one); the coat lobe
    three, the refraction into the medium one.  Counted on the oracle's states: the reference's own counts are what they are held to."""
    for group, (material, limit, rows, states, kind, ref, orows, ostates) in step_results.items():
        ok = ~R.near_ties(ref)
        one, three = R.lr.rng_draw(states, 1)[1], R.lr.rng_draw(states, 3)[1]
        cut = ref["margins"]["cutoff"] < 0.0
        for event, want in ((0, one), (2, one)):
            rows_of = ok & (ref["event"] == event)
            assert np.array_equal(ostates[rows_of], want[rows_of]), (group, event)
        scattered = ok & (ref["event"] == 1)
        assert np.array_equal(ostates[scattered & ~cut], three[scattered & ~cut]) and np.array_equal(ostates[scattered & cut], one[scattered & cut]), group
        assert np.array_equal(ref["draws"], np.where((ref["event"] == 1) & ~cut, 3, 1))
    for group, (material, inputs, states, ref, rows, ostates) in begin_results.items():
        one, three = R.lr.rng_draw(states, 1)[1], R.lr.rng_draw(states, 3)[1]
        coat = ref["margins"]["lobe"] > 0.0
        assert np.array_equal(ostates, np.where(coat, three, one)), group


def test_every_outcome_and_branch_is_occupied(begin_results, step_results):
    """... by at least 5 % of the rows of at least one group; the share is the reference's."""
    best = {}
    for results, at in ((begin_results, 3), (step_results, 5)):
        for group, entry in results.items():
            ref = entry[at]
            shares = {("outcome", o): float((ref["outcome"] == o).mean()) for o in (R.FALLBACK, R.SAMPLE, R.WALKING)}
            shares.update({k: float(v.mean()) for k, v in R.branches(ref).items()})
            if "event" in ref:
                shares.update({("event", e): float((ref["event"] == e).mean()) for e in (0, 1, 2)})
                shares["step_limit"] = float((ref["step"].astype(np.int64) >= max(entry[1], 1)).mean())
            for k, v in shares.items():
                best[k] = max(best.get(k, 0.0), v)
    # Three of the coat's five rejections cannot be the first to fire anywhere: the VNDF half vector has dot(wh, n) >= 0 by construction
    # (its z is clamped at 0) and wo.wh > 0 wherever wo is above the surface, so dot(wi, wh) = dot(wo, wh) and ggx_pdf's cosines are
    # positive there; below the surface cosThetaO <= 0 rejects first.  Their conditions do hold in rows the earlier ones reject (that is
    # what `branches` counts), which is as occupied as the shader lets them be; dot(wh, n) <= 0 holds only at a rounded zero.
    unreachable_alone = {"coat_wh_rejects"}
    thin = {k: v for k, v in best.items() if v < 0.05 and k not in unreachable_alone}
    assert not thin, thin


def test_the_whole_walk_matches_the_float64_walk(tmp_path):
    """The oracle's walk (its own BVH and intersectors) against the float64 walk over analytic hits: the sequence of outcomes and the
    final record agree for at least 98 % of the walks of every scene - the condition test_gpu_sss_walk.py puts to the device."""
    for name in K.SCENES:
        host, twin = K.scene(name, tmp_path)
        s = K.walk_settings(host)
        xys = K.all_pixels()
        steps, final = ol.OracleScene(host).sss_walks(s, xys, 32)
        cam, cam_states = ol.camera_rays(s, xys)
        ref = K.reference_walks(host, twin, s, cam, cam_states)
        same = K.walks_agree(steps, final, ref)
        assert np.array_equal(final["first_hit"] != 0, ref["first_hit"]), name
        assert np.array_equal(final["started"] != 0, ref["started"]), name
        assert same.mean() >= 0.98, (name, same.mean(), np.flatnonzero(~same)[:16])
        if name != "cube_inward":   # (an inward cube shows the camera its back faces: no walk starts, which is what is checked there)
            assert ref["started"].mean() > 0.1 and (ref["queries"] > 3).mean() > 0.02, name
        else:
            assert not ref["started"].any()
