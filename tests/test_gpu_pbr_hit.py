"""GPU tests of the per-hit material of the textured metallic-roughness model (csrc/kernels/wavefront.hip applyPbrTextures with
csrc/kernels/texture.h, and the upload's triUv / triTangent rows) through ptr_debug_pbr_hits, on the input classes of
tests/pbr_hit_domain.py.

The device is held to the float64 reference on the rows the reference does not guard: branch outcomes (discard, basis of the normal
map, the flip to the geometric side, two-sidedness) and random states equal, values within 4 x the oracle's own largest difference
from the reference in that class (ORACLE_MEASURED, re-derived by tests/test_pbr_hit_host.py), and no less than 4 float32 ulps of the
output's range.  The margin is for what separates the device from the oracle: log2f, rsqrt and division, and nothing else.  The
device is also held to the oracle row by row: the same hit, random state and decisions, values within DEVICE_ORACLE_ULPS ulps, and
where a class was measured bit-equal (DEVICE_EQUALS_ORACLE) it must stay so.

The gradient classes run instantiation 1 (applyPbrTextures<true>), which the oracle does not have: without valid bits it must
reproduce instantiation 0 bit for bit in every class; with gradients it is held to the reference's statement of the tap rule of
texture.h and of the variance term.  Its bound is the largest of the bounds of the material classes that read textures away from
[0, 1] (GRADIENT_BOUND_FROM): a gradient sample is the mean of up to eight level samples at coordinates that far out, at a level of
detail computed as the cone's is, so it carries the level sample's error and no other.
"""
import numpy as np
import pytest

import oracle_lib as ol
import pbr_hit_domain as D

pytestmark = pytest.mark.gpu

# classes in which the device's rows were measured bit-equal to the oracle's on an MI355X (every output word of every row)
DEVICE_EQUALS_ORACLE = ("material/texture-index", "material/not-pbr")
DEVICE_ORACLE_ULPS = 8
GRADIENT_BOUND_FROM = ("material/slots", "material/transforms", "material/wraps", "material/nearest", "material/uv-sets")

_oracles = {}


def _oracle(sc):
    if id(sc) not in _oracles:
        _oracles[id(sc)] = ol.OracleScene(sc)
    return _oracles[id(sc)]


def _against_reference(name, sc, rows, got, limit):
    ref = D.reference(sc, rows, got)
    d = D.differences(ref, got)
    bad = d["branch_mismatches"]
    print("%s: rows %d guarded %d compared %d  device - reference: colour %.3g scalar %.3g normal %.3g  (bounds %.3g %.3g %.3g)"
          % (name, d["rows"], d["guarded"], d["compared"], d["colour"], d["scalar"], d["normal"], limit(d)["colour"], limit(d)["scalar"],
             limit(d)["normal"]))
    assert len(bad) == 0, (name, len(bad), bad[:8], ref["basis"][bad[:8]], got["basis"][bad[:8]])
    assert d["guarded"] <= 0.02 * max(d["textured"], 1)
    for k in ("colour", "scalar", "normal"):
        assert d[k] <= limit(d)[k], (name, k, d[k], limit(d)[k])
    # the surface record the kernel reports, which the reference restates as well
    use = (got["hit"] > 0) & (ref["guards"]["front"] >= D.GUARD["front"]) & (ref["guards"]["hit_flip"] >= D.GUARD["hit_flip"])
    assert np.array_equal(ref["front_face"][use], got["front_face"][use] > 0)
    # (the patches lie up to 250 units from the origin with edges of 1 .. 2: a float32 edge vector carries 250 x 2^-23 = 3e-5)
    assert D.angle(ref["geometric_normal"][use], got["geometric_normal"][use]).max() < 1e-4
    assert D.angle(ref["hit_normal"][use], got["hit_normal"][use]).max() < 1e-4
    return d, ref


@pytest.mark.parametrize("group", list(D.GROUPS))
def test_device_matches_reference_and_oracle(group):
    for name in D.GROUPS[group]:
        sc, rows = D.class_rows(name)
        got = sc.dev.pbr_hits(rows)
        assert (got["hit"] > 0).sum() >= D.ROWS * 3 // 4
        _, ref = _against_reference(name, sc, rows, got, lambda d: D.bounds(name, d["range"]))
        # ... and the oracle, row by row
        ora = _oracle(sc).pbr_hits(rows)
        same_hit = (got["hit"] > 0) & (ora["hit"] > 0) & (got["mesh"] == ora["mesh"]) & (got["triangle"] == ora["triangle"])
        if name != "bary/edges":   # (a ray aimed at an edge two triangles share may report either of them)
            assert same_hit.sum() >= 0.999 * (got["hit"] > 0).sum()
        assert same_hit.sum() >= 0.99 * (got["hit"] > 0).sum()
        assert np.array_equal(got["state"][same_hit], ora["state"][same_hit])
        assert np.array_equal(got["textured"][same_hit], ora["textured"][same_hit])
        # the decisions: equal wherever the reference finds the row clear of every threshold
        clear = same_hit & ~D.guarded(ref)
        assert np.array_equal(got["discard"][clear], ora["discard"][clear]) and np.array_equal(got["basis"][clear], ora["basis"][clear])
        both = same_hit & (got["discard"] == ora["discard"]) & (got["basis"] == ora["basis"])
        print("%s: device and oracle decide differently on %d guarded rows" % (name, int((same_hit & ~both).sum())))
        # the values (bu .. discard): device and oracle run the same float32 statements in the same order and differ in log2f, rsqrt
        # and division, an ulp each, which the bilinear and trilinear weights pass on: DEVICE_ORACLE_ULPS float32 ulps of the largest value
        # in the class (at least 1), against a largest measured 3.3e-7 where that value is 1.5
        worst = float(np.abs(got["raw"][both][:, 4:29].astype(np.float64) - ora["raw"][both][:, 4:29]).max())
        scale = max(1.0, float(np.abs(ora["raw"][both][:, 4:29]).max()))
        equal = np.array_equal(got["raw"].view(np.uint32), ora["raw"].view(np.uint32))
        print("%s: device - oracle: largest difference %.3g over %d rows (bound %.3g), bit-equal: %s"
              % (name, worst, int(both.sum()), DEVICE_ORACLE_ULPS * D.EPS32 * scale, equal))
        assert worst <= DEVICE_ORACLE_ULPS * D.EPS32 * scale, (name, worst)
        if name in DEVICE_EQUALS_ORACLE:
            assert equal, name


@pytest.mark.parametrize("group", list(D.GROUPS))
def test_instantiation_with_no_valid_gradients_is_the_plain_one(group):
    """grad/none: applyPbrTextures<true> with the valid bits 0 gives every output word of applyPbrTextures<false>."""
    for name in D.GROUPS[group]:
        sc, rows = D.class_rows(name)
        plain = sc.dev.pbr_hits(rows)["raw"]
        with_rd = rows.copy()
        with_rd.view(np.uint32)[:, 10] = 1
        with_rd[:, 11:19] = np.random.default_rng(5).uniform(-1.0, 1.0, size=(rows.shape[0], 8)).astype(np.float32)   # ignored: no valid bit
        assert np.array_equal(sc.dev.pbr_hits(with_rd)["raw"].view(np.uint32), plain.view(np.uint32)), name


def test_instantiation_with_gradients_matches_reference():
    """grad/given: isotropic, anisotropic, zero and oversized gradients, one set valid or both, through a rotated texture transform and
    on NEAREST textures."""
    sc, rows = D.gradient_class_rows()
    got = sc.dev.pbr_hits(rows)

    def limit(d):
        limits = [D.bounds(c, d["range"]) for c in GRADIENT_BOUND_FROM]
        return {k: max(b[k] for b in limits) for k in ("colour", "scalar", "normal")}

    d, ref = _against_reference("grad/given", sc, rows, got, limit)
    # the class runs what it is named for: gradient samples of 1 .. 8 taps, the variance term inside and outside its window
    assert np.isfinite(ref["guards"]["aniso_ceil"]).sum() > D.ROWS // 4 and np.isfinite(ref["guards"]["grad_window"]).sum() > D.ROWS // 8
    plain = sc.dev.pbr_hits(np.where(np.arange(20) >= 10, 0.0, rows).astype(np.float32))
    keep = (got["hit"] > 0) & ~(got["discard"] > 0) & ~(plain["discard"] > 0)
    assert (got["roughness"][keep] > plain["roughness"][keep] + 1e-4).sum() > 100          # the variance term widened lobes
    assert (np.abs(got["base_color"][keep] - plain["base_color"][keep]).max(axis=1) > 1e-3).sum() > 500
