"""The path state of the wavefront integrator on the device (csrc/kernels/wavefront.hip shadeSlot: the medium stack and its packing, the
flags word, Russian roulette, lastPdf / lastDelta / specDepth, and when a finished item is published), read out of the pool after every
iteration of the production loop by ptr_debug_path_states (include/ptr_debug_path.h) and held, vertex by vertex,
  (a, b) to the float64 bookkeeping of tests/path_state_ref.py given the device's own BSDF sample of that vertex, which the existing probes
         reproduce from the recorded ray, random state, material and front face;
  (c)    to the oracle's per-vertex recorder;
  (d)    to the count of 511 vertices between two mirrors;
  (e, f) to the production render, and to itself under another batch.
The groups are those of tests/path_state_cases.py, which tests/test_path_state_host.py shows fair."""
import numpy as np
import pytest

import oracle_lib as ol
import path_state_cases as K
import path_state_ref as R

pt = ol.pt
pytestmark = pytest.mark.gpu

MISS = 0xFFFFFFFF
F = np.float32


def _normalize32(a):
    """vec.h normalize, operation for operation in float32: a x (1 / sqrt((x x + y y) + z z))"""
    a = np.asarray(a, F)
    d = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        return a * (F(1.0) / np.sqrt(d))[:, None]


def device_vertices(dev, host, settings, pixels, cap):
    """The device's vertices of the pixels as the table path_state_cases.check_vertices takes: the snapshots of ptr_debug_path_states,
    and for every vertex the hit and the BSDF sample the probes give for the recorded ray and random state.  Asserts on the way what
    ties the probes to the snapshots to the bit: t, the next origin, the sampled direction, its pdf."""
    tables = K.scene_tables(host)
    snap, ran, items = dev.path_states(settings, pixels, 0, cap + 2)
    V, n = snap["flags"].shape
    fl = R.decode_flags(snap["flags"])
    cam, cam_rng = pt.debug_camera_rays(settings, K.xys_of(settings, pixels))
    origin = np.concatenate([cam[None, :, 0:3], snap["origin"][:-1]])
    direction = np.concatenate([cam[None, :, 3:6], snap["direction"][:-1]])
    rng_before = np.concatenate([cam_rng[None], snap["rng"][:-1]])
    reached = np.concatenate([np.ones((1, n), bool), fl["alive"][:-1] != 0])
    goes = fl["alive"] != 0
    kk, ii = np.nonzero(reached)
    m = len(kk)
    o, d = origin[kk, ii], direction[kk, ii]
    rays = np.concatenate([o, np.full((m, 1), 1e-4, F), d, np.full((m, 1), np.inf, F)], axis=1).astype(F)
    hits, _ = dev.extend_rays(rays)
    miss = snap["hit_word"][kk, ii] == MISS
    assert np.array_equal(hits["primType"][~miss] <= 2, np.ones((~miss).sum(), bool)) and np.array_equal(hits["t"][~miss].view(np.uint32), snap["t"][kk, ii][~miss].view(np.uint32))
    surf = dev.surface_hits(np.concatenate([o, d, snap["direction"][kk, ii]], axis=1))
    assert np.array_equal(surf[:, 0] != 0, ~miss)
    index = hits["primIndex"].astype(np.int64)
    lookup = lambda table: np.concatenate([table, [0]])[np.clip(index, 0, max(len(table) - 1, 0))]   # (an empty table reads 0: never selected)
    material = np.where(hits["primType"] == 1, lookup(tables["sphere_material"]), lookup(tables["rect_material"]))
    material = np.minimum(np.where(miss, 0, material), tables["count"] - 1)
    mtype = tables["type"][material]
    front = surf[:, 11] != 0
    normal, shading = surf[:, 5:8], surf[:, 8:11].copy()
    zero = np.einsum("ij,ij->i", shading, shading) <= 0
    shading[zero] = normal[zero]
    face = bool(settings.metalSemantics & pt.PTR_METAL_FACE_NORMAL)
    glass_n = np.where((face & ~front)[:, None], -normal, normal)
    nrm = _normalize32(np.where((mtype == 2)[:, None], glass_n, shading))
    wo = -_normalize32(d)
    took = ~miss & (mtype != 3)
    # under a rectangle light a surface that is not a delta one draws the three numbers of its light sample first, whatever comes of it
    rng_in = rng_before[kk, ii].copy()
    sampled_light = took & ~tables["delta"][material] & (tables["lights"] > 0)
    rng_in[sampled_light] = R.lr.rng_draw(rng_in[sampled_light], 3)[1]
    rng_rect = rng_in.copy()
    sampled_env = took & ~tables["delta"][material] & tables["env"]   # ... and three more under a sampled environment
    rng_in[sampled_env] = R.lr.rng_draw(rng_in[sampled_env], 3)[1]
    sample, rng_bsdf = np.zeros((m, 8), F), rng_in.copy()
    for mat in np.unique(material[took]):
        rows = np.flatnonzero(took & (material == mat))
        inputs = np.concatenate([surf[rows, 2:5], nrm[rows], wo[rows]], axis=1)
        sample[rows], rng_bsdf[rows] = pt.debug_sample_bsdf(host.desc.materials[int(mat)], settings, inputs, front[rows].astype(np.uint32), rng_in[rows])
    valid = took & (sample[:, 6] > 0) & (np.einsum("ij,ij->i", sample[:, 0:3], sample[:, 0:3]) > 0) & np.isfinite(sample[:, 3:6]).all(axis=1)
    on = goes[kk, ii]
    # (b) the probe's direction and pdf are the next snapshot's to the bit, and the next ray starts where offsetOrigin puts it
    assert not (on & ~valid).any()
    bits = lambda a: np.ascontiguousarray(a, F).view(np.uint32)
    assert np.array_equal(bits(sample[on, 0:3]), bits(snap["direction"][kk, ii][on])), "the probe's direction is not the recorded one"
    assert np.array_equal(bits(sample[on, 6]), bits(snap["last_pdf"][kk, ii][on])), "the probe's pdf is not the recorded lastPdf"
    assert np.array_equal(bits(surf[on, 12:15]), bits(snap["origin"][kk, ii][on])), "the next origin is not offsetOrigin's"
    media = bool(settings.metalSemantics & pt.PTR_METAL_MEDIA)
    thin = tables["thin"][material] & bool(settings.metalSemantics & pt.PTR_METAL_THIN)
    event = R.medium_event((mtype == 2) & ~thin, sample[:, 0:3], normal, front) if media else np.zeros(m, np.int64)

    def table(values, dtype=None):
        out = np.zeros((V, n) + values.shape[1:], dtype or values.dtype)
        out[kk, ii] = values
        return out
    v = dict(exists=table(took), valid=table(valid), initial_rng=cam_rng, t=table(hits["t"]), material=table(material), rng_bsdf=table(rng_bsdf),
             weight=table(sample[:, 3:6]), pdf=table(sample[:, 6]), is_delta=table(sample[:, 7] != 0), medium_event=table(event),
             direction=table(sample[:, 0:3]), throughput=snap["throughput"], last_pdf=snap["last_pdf"], last_delta=fl["last_delta"] != 0,
             spec_depth=fl["spec_depth"], medium_depth=fl["medium_depth"], stack=R.unpack_stack(snap["medium"]), rng_after=snap["rng"],
             ended=~goes, reached=reached, miss=table(miss), prim_type=table(hits["primType"]), prim_index=table(hits["primIndex"]),
             origin_in=origin, direction_in=direction, rng_before=rng_before, rng_rect=table(rng_rect), sampled_light=table(sampled_light),
             front=table(front), hit_t=table(hits["t"]),
             queued=np.where((((fl["pending"][:, :, None] >> np.arange(R.REC_SLOTS, dtype=np.uint32)) & 1) != 0)[..., None],
                             snap["record_value"].reshape(V, n, R.REC_SLOTS, 3), F(0.0)).sum(axis=2),   # (a slot that is not pending holds whatever was there)
             thr_before=np.concatenate([np.ones((1, n, 3), F), snap["throughput"][:-1]]), last_delta_before=np.concatenate([np.ones((1, n), bool), fl["last_delta"][:-1] != 0]))
    return v, snap, fl, ran, items, tables


def oracle_agreement(name, settings, v, items, ov, ot, oradiance, pixels):
    """(c): the paths whose whole sequence of (primitive, discrete state, random state) and whose radiance are the oracle's"""
    V = min(v["reached"].shape[0], ot["valid"].shape[0])
    o_reached = ot["valid"][:V] != 0
    same = (v["reached"][:V] == o_reached).all(axis=0) & ~v["reached"][V:].any(axis=0)
    both = v["reached"][:V] & o_reached
    o_miss = ot["hit"][:V] == 0
    same &= np.where(both, v["miss"][:V] == o_miss, True).all(axis=0)
    hit = both & ~v["miss"][:V] & ~o_miss
    for mine, theirs in (("prim_type", "prim_type"), ("prim_index", "prim_index")):
        same &= np.where(hit, v[mine][:V] == ot[theirs][:V], True).all(axis=0)
    on = hit & ~v["ended"][:V] & (ot["ended"][:V] == 0)
    same &= np.where(hit, v["ended"][:V] == (ot["ended"][:V] != 0), True).all(axis=0)
    theirs = dict(spec_depth=ot["spec_depth"][:V], medium_depth=ot["medium_depth"][:V], rng_after=ot["rng_after"][:V], last_delta=ot["last_delta"][:V] != 0)
    for f, other in theirs.items():
        same &= np.where(on, np.asarray(v[f][:V], np.int64) == np.asarray(other, np.int64), True).all(axis=0)
    live = np.arange(R.MAX_STACK)[None, None, :] < np.asarray(v["medium_depth"][:V], np.int64)[:, :, None]
    same &= np.where(on[:, :, None] & live, v["stack"][:V] == ot["stack"][:V], True).all(axis=(0, 2))
    close = lambda a, b, rtol, atol: np.abs(a.astype(np.float64) - b) <= atol + rtol * np.abs(b)
    same &= close(items[:, :3], oradiance, K.RTOL, K.ATOL).all(axis=1)
    # per-vertex floats of the agreeing paths at the project's bounds against the oracle
    sel = on & same[None, :]
    assert close(v["direction"][:V][sel], ot["direction"][:V][sel], 0.0, K.DIR_ATOL).all(), name
    for mine, theirs in (("weight", "weight"), ("pdf", "pdf"), ("throughput", "throughput")):
        assert close(v[mine][:V][sel], ot[theirs][:V][sel], K.RTOL, K.ATOL).all(), (name, mine)
    # what each vertex queued, as it landed, against the oracle's queued radiance of that vertex
    near = (ot["near"] != 0).any(axis=0)
    held = both & (same & ~near)[None, :]
    assert close(v["queued"][:V][held], ot["queued"][:V][held], K.RTOL, K.ATOL).all(), (name, "queued")
    listed = [(int(p % settings.width), int(p // settings.width)) for p in pixels[~same]]
    return same, near, listed


def check_queued_against_the_probes(name, dev, settings, snap, fl, v):
    """What a vertex queues, against the probes on the recorded vertex.  The rectangle-light sample: ptr_debug_rect_light_nee with the
    recorded ray, throughput and random state queues exactly when the pending bit says so, advances the random state as the vertex did,
    and its contribution is the record's, bit for bit, unless k_connect found the shadow ray occluded and zeroed it (vertices inside an
    absorbing medium are left out: the probe takes the throughput after Beer-Lambert, which the snapshots do not hold).  A settled
    specular connection (kind 3): ptr_debug_light_connection along the next ray with the probe's BSDF sample and the throughput before it
    gives the record's value within 1e-5 relative (the record's origin is offsetOrigin of the normalised direction, the next ray's of the
    direction as sampled: a last-bit difference of the origin)."""
    V, n = fl["alive"].shape
    rec = snap["record_value"].reshape(V, n, R.REC_SLOTS, 3)
    depth_before = np.concatenate([np.zeros((1, n), np.int64), np.asarray(fl["medium_depth"][:-1], np.int64)])
    kk, ii = np.nonzero(v["sampled_light"] & (depth_before == 0))
    rays = np.concatenate([v["origin_in"][kk, ii], v["direction_in"][kk, ii]], axis=1)
    out, states = dev.rect_light_nee(settings, rays, v["thr_before"][kk, ii], v["rng_before"][kk, ii])
    assert np.array_equal(states, v["rng_rect"][kk, ii]), (name, "the light sample's draws")
    queued = (fl["pending"][kk, ii] & 1) != 0
    assert np.array_equal(out[:, 1] != 0, queued), (name, "queued", int((out[:, 1] != 0).sum()), int(queued.sum()))
    value = rec[kk, ii, 0]
    lit = queued & (value != 0).any(axis=1)
    assert np.array_equal(np.ascontiguousarray(out[lit, 9:12]).view(np.uint32), np.ascontiguousarray(value[lit]).view(np.uint32)), (name, "contribution")
    assert queued.sum() >= 100 and lit.sum() >= 50, (name, int(queued.sum()), int(lit.sum()))
    # settled specular connections
    # (of paths that go on: the snapshot holds the next ray only then)
    kk3, ii3 = np.nonzero(((fl["pending"] >> 3) & 1 != 0) & (snap["record_kind"][..., 3] == 3) & (depth_before == 0) & (fl["alive"] != 0))
    if len(kk3):
        inputs = np.concatenate([snap["origin"][kk3, ii3], snap["direction"][kk3, ii3], v["weight"][kk3, ii3], v["pdf"][kk3, ii3][:, None],
                                 v["thr_before"][kk3, ii3], np.zeros((len(kk3), 1), F)], axis=1)
        conn, info = dev.light_connection(settings, inputs)
        got, want = rec[kk3, ii3, 3].astype(np.float64), conn[:, 5:8].astype(np.float64)
        seen = (got != 0).any(axis=1)   # (k_connect zeroes an occluded one)
        assert info["settles"] and np.all(conn[:, 0] != 0), name
        assert np.all(np.abs(got[seen] - want[seen]) <= 1e-5 * np.abs(want[seen])), (name, "settled connection")
    assert len(kk3) >= 3 or name not in ("lit/spec", "lit/mnee"), (name, len(kk3))
    return int(queued.sum()), int(lit.sum()), len(kk3)


def check_accum_schedule(name, dev, settings, tables, snap, fl, items, v):
    """When radiance arrives (path_state_ref.accum_schedule, stated on the snapshots to the bit): the connections a visit queues - the
    pending bits of the flags, the records as k_connect left them - are added to `accum` at the slot's next visit, in slot order; a path
    that ends with connections outstanding keeps its sum, is flagged, and is published one visit later with them; one that ends with
    none is published at once, and `accum` reads 0 from then on.  Only surface vertices queue, and they add nothing at once."""
    V, n = fl["alive"].shape
    rec = snap["record_value"].reshape(V, n, R.REC_SLOTS, 3)
    alive, flush, pending = fl["alive"] != 0, fl["flush"] != 0, fl["pending"]
    assert not (flush & alive).any() and not (flush & (pending == 0)).any(), name
    # the kind of a queued record by its slot: any-hit (0) for the light sample; a settled (3) or traced (1) specular connection; the chain (2)
    for slot, kinds in ((0, (0,)), (3, (1, 3)), (4, (2,))):
        queued = ((pending >> slot) & 1) != 0
        assert np.isin(snap["record_kind"][..., slot][queued], kinds).all(), (name, slot)
    for slot in (1, 2):   # a sampled environment's: any-hit records
        queued = ((pending >> slot) & 1) != 0
        assert np.all(snap["record_kind"][..., slot][queued] == 0) and (queued.any() == bool(tables["env"])), (name, slot)
    if name == "lit/traced":
        assert (snap["record_kind"][..., 3][((pending >> 3) & 1) != 0] == 1).all() and (((pending >> 3) & 1) != 0).sum() >= 20, name
    landed_by_slot = [int((((pending >> k) & 1) != 0).sum()) for k in range(R.REC_SLOTS)]
    at_once = flushed = escaped = weighted_escapes = emitters = weighted_emitters = 0
    worst = 0.0
    for k in range(V):
        acc = snap["accum"][k - 1].copy() if k else np.zeros((n, 3), F)
        for slot in range(R.REC_SLOTS if k else 0):
            on = ((pending[k - 1] >> slot) & 1) != 0
            acc = np.where(on[:, None], (acc + rec[k - 1][:, slot]).astype(F), acc)
        alive_before, was_flush = (alive[k - 1], flush[k - 1]) if k else (np.ones(n, bool), np.zeros(n, bool))
        went_on = alive_before & alive[k]
        ended_waiting = alive_before & ~alive[k] & flush[k]
        bits = lambda a: np.ascontiguousarray(a, F).view(np.uint32)
        for rows in (went_on, ended_waiting):
            assert np.array_equal(bits(snap["accum"][k][rows]), bits(acc[rows])), (name, k)
        assert np.array_equal(snap["flush_item"][k][ended_waiting], snap["item"][k][ended_waiting]), (name, k)
        # a flagged item: published now with what just landed, and the slot is done
        assert np.array_equal(bits(items[was_flush, :3]), bits(acc[was_flush])) and not snap["accum"][k][was_flush].any(), (name, k)
        assert np.all(snap["flags"][k][was_flush] == 2), (name, k)
        # ended with nothing outstanding: published at once - the sum so far plus what the last vertex adds at once (an escaped ray's
        # background, an emitter's radiance) - and accum handed on
        ended_now = alive_before & ~alive[k] & ~flush[k]
        assert not snap["accum"][k][ended_now].any() and np.all(snap["flags"][k][ended_now] == 2), (name, k)
        # ... held to float64 with its MIS weight: the environment's pdf along the escaped ray (ptr_debug_env_eval), the light's for the
        # emitter hit (ptr_debug_light_connection), the recorded lastPdf and lastDelta
        rows = np.flatnonzero(ended_now & (v["miss"][k] | ~v["exists"][k]))
        if rows.size:
            miss = v["miss"][k][rows]
            o, d = v["origin_in"][k][rows], v["direction_in"][k][rows]
            env = dev.env_eval(settings, d) if tables["env"] else None
            light_pdf, front = np.zeros(rows.size), v["front"][k][rows]
            if tables["lights"]:
                conn, _ = dev.light_connection(settings, np.concatenate([o, d, np.ones((rows.size, 7), F), np.zeros((rows.size, 1), F)], axis=1))
                light_pdf = conn[:, 8].astype(np.float64)
            want, bound = K.immediate_radiance(settings, tables, v, k, rows, miss, front, v["material"][k][rows], v["hit_t"][k][rows].astype(np.float64), env, light_pdf)
            got = items[rows, :3].astype(np.float64) - acc[rows]
            slack = bound[:, None] * np.abs(want) + 2.0 ** -24 * np.abs(items[rows, :3])
            assert np.all(np.abs(got - want) <= slack), (name, k, rows[(np.abs(got - want) > slack).any(axis=1)][:8])
            worst = max(worst, float((np.abs(got - want) / np.maximum(slack, 1e-300)).max()))
            before = K.state_before(v, k)
            uses = (~before["last_delta"][rows]) | bool(settings.enableSpecularNee) | bool(settings.enableMnee)
            escaped += int(miss.sum())
            weighted_escapes += int((miss & uses & tables["env"]).sum())
            emitters += int((~miss).sum())
            weighted_emitters += int((~miss & uses & (light_pdf > 0)).sum())
        assert np.array_equal(ended_now & ~v["miss"][k] & ~v["exists"][k], ended_now & ~v["miss"][k] & (tables["type"][v["material"][k]] == 3)), (name, k)
        at_once += int(ended_now.sum())
        flushed += int(was_flush.sum())
    assert at_once + flushed == n and flushed >= 10 and at_once >= 50, (name, at_once, flushed)
    assert weighted_escapes >= 50 or not tables["env"], (name, weighted_escapes)
    assert weighted_emitters >= 50 or not tables["lights"], (name, weighted_emitters)
    return landed_by_slot, at_once, flushed, escaped, weighted_escapes, emitters, weighted_emitters, worst


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("path_state_gpu")
    made = {}
    for name, (build, make, cap) in K.groups().items():
        if build not in made:
            host = build(tmp)
            made[build] = (host, pt.DeviceScene(host.desc, 0, keepalive=host))
    return made


@pytest.mark.parametrize("name", list(K.groups()))
def test_every_vertex_against_float64_and_the_oracle(name, scenes):
    build, make, cap = K.groups()[name]
    host, dev = scenes[build]
    settings = make(host)
    pixels = K.pixels_of(settings)
    v, snap, fl, ran, items, tables = device_vertices(dev, host, settings, pixels, cap)
    V, n = fl["alive"].shape
    # (a) the flags word field by field: alive paths count their depth, nothing else moves; a path that ended reads as the reset state
    # (lastDelta alone), published at once (no light: no record is ever pending, no flush), and its slot is not written again
    goes = fl["alive"] != 0
    assert np.array_equal(fl["depth"][goes], (np.arange(V)[:, None] + np.ones((1, n), np.int64))[goes]), name
    assert np.array_equal(snap["item"], np.broadcast_to(np.arange(n, dtype=np.uint32), (V, n))), name
    assert not fl["walk"].any() and not fl["spare"].any(), name
    if tables["lights"] or tables["env"]:
        schedule = check_accum_schedule(name, dev, settings, tables, snap, fl, items, v)
        if tables["lights"]:
            print("%s: light samples held to the probe bit for bit: %d queued, %d of them unoccluded; settled connections held to the probe: %d"
                  % ((name,) + check_queued_against_the_probes(name, dev, settings, snap, fl, v)))
    else:
        for f in ("flush", "pending"):
            assert not fl[f].any(), (name, f)
        assert np.all(snap["flags"][~goes & v["reached"]] == 2) and not snap["accum"].any(), name
    dead = ~(goes | (fl["flush"] != 0) | (fl["pending"] != 0))[:-1]
    assert np.array_equal(snap["raw"][1:][dead].view(np.uint32)[:, :8], snap["raw"][:-1][dead].view(np.uint32)[:, :8]), name   # rays and flags
    assert np.array_equal(snap["raw"][1:][dead].view(np.uint32)[:, 10:24], snap["raw"][:-1][dead].view(np.uint32)[:, 10:24]), name
    assert not goes[-1].any() and ran >= int(v["reached"].sum(axis=0).max()), name
    # (a, b) the bookkeeping in float64 from the device's own samples: discrete state and random state exactly, throughput within its bound
    counts = K.check_vertices(settings, tables, v, name)
    # the radiance of a path is what its escaping vertex adds: background x throughput through the clamp, with weight 1
    last = v["reached"].sum(axis=0) - 1
    idx = np.arange(n)
    escaped = v["miss"][last, idx]
    state = dict(throughput=v["thr_before"][last, idx].astype(np.float64), last_delta=v["last_delta_before"][last, idx], last_pdf=np.ones(n))
    want = np.where(escaped[:, None], R.escaped(settings, state, np.array(K.BACKGROUND, F).astype(np.float64)), 0.0)
    if not (tables["lights"] or tables["env"]):   # (under a light or a sampled environment the schedule above has said what is published)
        assert np.all(np.abs(items[:, :3] - want) <= 4.0 * 2.0 ** -24 * np.abs(want)), name
    else:
        print("%s: connections landed %s by record slot; items published at once %d, flushed one visit later %d; escaped rays %d (MIS-weighted "
              "%d), emitter hits %d (MIS-weighted %d), worst %.3f of the bound" % ((name,) + schedule))
    # (c) against the oracle's recorder
    ov, ot, oradiance, _, _ = K.oracle_vertices(host, settings, cap, ol)
    same, near, listed = oracle_agreement(name, settings, v, items, ov, ot, oradiance, pixels)
    print("%s: paths %d, vertices %d, near ties %.4f, paths that differ from the oracle's %.4f: %s; largest deviation from float64 %.3f of its "
          "bound; what it leaves for expf: %.2f ulp; pushes at 8: %d, pops at 0: %d, clamp engaged: %d, roulette kills %d, spares %d"
          % (name, n, counts["vertices"], near.mean(), 1.0 - same.mean(), listed[:24], counts["worst"], counts["expf_ulp"], counts["push_at_8"],
             counts["pop_at_0"], counts["clamped"], sum(counts["killed"].values()), sum(counts["spared"].values())))
    assert same.mean() >= 0.98, (name, same.mean(), listed[:32])
    assert near.mean() <= K.NEAR_TIE_CAP


def test_deep_counts_to_511(scenes):
    """(d) Depth and specDepth count 1 .. 510 between the mirrors with no other field of the flags word moving, and the path ends at
    vertex 510 by depth >= maxDepth.  fillRenderParams clamps maxDepth to 511, the width of the counters - the oracle has no such clamp -
    so at maxDepth 600 the device stops after the same vertex and publishes: the snapshots are those of maxDepth 511, bit for bit."""
    build, make, cap = K.groups()["deep"]
    host, dev = scenes[build]
    s = make(host)
    pixels = K.pixels_of(s)
    snap, ran, items = dev.path_states(s, pixels, 0, 520)
    fl = R.decode_flags(snap["flags"])
    V, n = fl["alive"].shape
    assert V >= 512 and np.all(fl["alive"][:510] == 1) and not fl["alive"][510:].any()
    count = np.arange(1, 511, dtype=np.uint32)[:, None]
    assert np.array_equal(fl["depth"][:510], np.broadcast_to(count, (510, n))) and np.array_equal(fl["spec_depth"][:510], np.broadcast_to(count, (510, n)))
    assert np.all(snap["flags"][:510] == (1 | 2 | (count << 8) | (count << 17))) and np.all(snap["flags"][510:] == 2)
    deeper = s.copy()
    deeper.maxDepth = 600
    snap600, ran600, items600 = dev.path_states(deeper, pixels, 0, 520)
    assert ran600 == ran and np.array_equal(snap600["raw"].view(np.uint32), snap["raw"].view(np.uint32)) and np.array_equal(items600, items)
    assert not items[:, :3].any()   # (the paths never leave: what is published is 0, and it is published)


@pytest.mark.parametrize("knobs", [{}, {"PTR_TAIL_BELOW": "0"}, {"PTR_TAIL_BELOW": "1000000"}, {"PTR_POOL_SLOTS": "256", "PTR_POOL_GROUPS": "1"}],
                         ids=["default", "no_tail", "tail_at_once", "small_pool"])
def test_the_wavefront_renders_what_the_probe_steps(knobs, tmp_path, monkeypatch):
    """(e) render_image is the probe's itemAccum bit for bit: through the dense k_shade (default), the listed one (no tail),
    k_tail_run (the tail as soon as the queue is dry), and a pool smaller than the frame, whose slots are reused - a stale `medium`
    word or flags field of the slot's previous item would show here."""
    for knob, value in knobs.items():   # the knobs are read when the scene is uploaded
        monkeypatch.setenv(knob, value)
    for name in ("nested/through/5", "nested/inside/7", "mixed/5", "mixed/0", "lit/spec", "lit/mnee", "lit/traced", "env"):
        build, make, cap = K.groups()[name]
        host = build(tmp_path)
        dev = pt.DeviceScene(host.desc, 0, keepalive=host)
        s = make(host)
        # (two samples per pixel: 1536 work items, more than the 1024 slots the smallest pool has; k_resolve adds a pixel's samples in
        # their order and halves the sum, which is exact)
        image, _ = dev.render_image(s, 2)
        first, second = (dev.path_states(s, K.pixels_of(s), sample, 4)[2][:, :3] for sample in (0, 1))
        want = (((np.zeros_like(first) + first) + second) * F(0.5)).reshape(s.height, s.width, 3)
        off = (image.view(np.uint32) != want.view(np.uint32)).any(axis=2)
        assert not off.any(), (name, knobs, [(int(x), int(y)) for y, x in zip(*np.nonzero(off))][:16])
        dev.close()


def _comparable(snap):
    """the words of the snapshots that do not depend on what ran on the scene before: rays, flags, hit, throughput, random state, radiance,
    and the stack entries below the depth (what lies above it, like the records of a path that queues none, is whatever was there)"""
    words = snap["raw"].view(np.uint32)
    depth = R.decode_flags(snap["flags"])["medium_depth"].astype(np.int64)
    live = np.arange(R.MAX_STACK)[None, None, :] < depth[:, :, None]
    return np.concatenate([words[:, :, 0:17], np.where(live, R.unpack_stack(snap["medium"]), 0)], axis=2)


def test_the_snapshots_do_not_depend_on_the_batch(scenes):
    """(f) the same pixels reversed, and one pixel alone: bit for bit"""
    for name in ("nested/through/5", "mixed/5"):
        build, make, cap = K.groups()[name]
        host, dev = scenes[build]
        s = make(host)
        pixels = K.pixels_of(s)[5:5 + 517]   # (not a multiple of a wave)
        snap, ran, items = dev.path_states(s, pixels, 0, cap + 2)
        back, ran_back, items_back = dev.path_states(s, pixels[::-1], 0, cap + 2)
        a, b = _comparable(snap), _comparable(back)[:, ::-1]
        assert ran == ran_back and np.array_equal(a, b) and np.array_equal(items[:, :3], items_back[::-1, :3]), name
        for i in (0, 63, 64, 516):
            one, _, item = dev.path_states(s, pixels[i:i + 1], 0, cap + 2)
            c = _comparable(one)
            k = min(c.shape[0], a.shape[0])
            assert np.array_equal(c[:k, 0], a[:k, i]) and np.array_equal(item[0, :3], items[i, :3]), (name, i)
            # (the batch runs until its longest path ends: this pixel's slot is not written again once its own has)
            assert np.array_equal(a[k:, i], np.broadcast_to(a[k - 1, i], a[k:, i].shape)), (name, i)
