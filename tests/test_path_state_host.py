"""The oracle's per-vertex recorder (oracle_path_states: the render loop's own body with a sink) against the float64 bookkeeping of
tests/path_state_ref.py, on the groups test_gpu_path_state.py puts to the device (tests/path_state_cases.py).  No GPU.  This is where the
groups are shown fair: near ties stay under the project's cap of 2 % of the paths of every group, and the branches the device test is
about are taken - the stack reaches 8, pushes find it full, pops find it empty, roulette kills and spares at depths 5, 6 and 8 and
beyond, the deep paths reach vertex 510.  The figures are printed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as ol
import path_state_cases as K
import path_state_ref as R

pt = ol.pt


def test_the_header_and_its_signature_table_agree():
    """include/ptr_debug_path.h has a signature table of its own: the tables of ptr_abi.h and ptr_debug.h keep their sizes."""
    text = open(os.path.join(ol.ROOT, "include", "ptr_debug_path.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = dict(re.findall(r"\bint\s+(ptr_\w+)\s*\(([^;]*)\)\s*;", text))
    assert set(declared) == set(pt.PATH_STATE_SYMBOLS) == {"ptr_debug_path_states"}
    for name, args in declared.items():
        assert len(args.split(",")) == len(pt._PATH_STATE_SIGNATURES[name][1]), name
    lib = pt.load_library()
    assert all(hasattr(lib, s) for s in pt.PATH_STATE_SYMBOLS)
    assert not set(pt.PATH_STATE_SYMBOLS) & (set(pt.ABI_SYMBOLS) | set(pt.DEBUG_SYMBOLS))
    assert pt.PATH_STATE_WORDS == int(re.search(r"#define PTR_PATH_STATE_WORDS (\d+)u", open(os.path.join(ol.ROOT, "include", "ptr_debug_path.h")).read()).group(1))


def test_the_probe_refuses_before_any_launch(tmp_path):
    """a NULL argument, no pixel, no iteration and a pixel outside the image are refused on the host"""
    lib = pt.load_library()
    s = K.groups()["deep"][1](K.deep_scene(tmp_path))
    pixels, states, items, ran = np.zeros(4, np.uint32), np.zeros((2, 4, 48), np.uint32), np.zeros((4, 4), np.float32), C.c_uint32(0)
    fp, up = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)), lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    outside = np.array([0, 1, s.width * s.height, 2], np.uint32)
    err = C.create_string_buffer(256)
    good = (C.c_void_p(1), C.byref(s), up(pixels), 4, 0, 2, up(states), C.byref(ran), fp(items))   # (refused before the handle is looked at)
    for position, value in ((0, None), (1, None), (2, None), (3, 0), (3, (1 << 20) + 1), (5, 0), (6, None), (7, None), (8, None), (2, up(outside))):
        args = list(good)
        args[position] = value
        assert lib.ptr_debug_path_states(*args, err, len(err)) != 0, position
        assert err.value


def test_the_packing_round_trips():
    """the 16-bit packing as a pure function of the eight ids: every position, the ids at the edges of a byte and of the half-word"""
    edge = (0, 1, 255, 256, 0xFFFE, 0xFFFF)
    for position in range(R.MAX_STACK):
        for value in edge:
            for rest in edge:
                ids = np.full(R.MAX_STACK, rest, np.uint32)
                ids[position] = value
                words = R.pack_stack(ids)
                assert words.dtype == np.uint32 and np.array_equal(R.unpack_stack(words), ids)
                # the word and the half the entry lies in, said once more without the function
                assert (int(words[position // 2]) >> (16 * (position % 2))) & 0xFFFF == value
    rng = np.random.default_rng(3)
    ids = rng.integers(0, 65536, (1000, 8)).astype(np.uint32)
    assert np.array_equal(R.unpack_stack(R.pack_stack(ids)), ids)
    fields = dict(alive=1, last_delta=0, flush=1, walk=0, medium_depth=8, depth=511, spec_depth=510, pending=0b10101, spare=0)
    word = R.encode_flags(**fields)
    assert {k: int(v) for k, v in R.decode_flags(word).items()} == fields
    assert int(word) == 1 | 4 | (8 << 4) | (511 << 8) | (510 << 17) | (0b10101 << 26)
    for name, shift, bits in R._FIELDS:   # each field alone reads back alone
        only = R.decode_flags(np.uint32(((1 << bits) - 1) << shift))
        assert all(int(v) == ((1 << bits) - 1 if k == name else 0) for k, v in only.items()), name


def test_the_reference_draws_the_oracles_stream():
    for state in (1, 0x9e3779b9, 0xFFFFFFFF, 12345):
        want, after = ol.rng_floats(state, 3)
        got, got_after = R.lr.rng_draw(np.array([state], np.uint32), 3)
        assert np.array_equal(got[0], want.astype(np.float64)) and int(got_after[0]) == after


def check_immediate(name, host, settings, tables, v, t):
    """The radiance the oracle's vertices add at once against float64: an escaped ray's background and an emitter's emission, each with
    its MIS weight (1.0 unless a non-delta bounce or specular NEE or MNEE; its clamp) from the recorded lastBsdfPdf and the oracle's
    own light pdf along the recorded ray."""
    osc = ol.OracleScene(host)
    rgba = np.ctypeslib.as_array(host.desc.envRgba, shape=(host.desc.envHeight, host.desc.envWidth, 4)).copy() if tables["env"] else None
    escaped = weighted_escapes = emitters = weighted_emitters = 0
    worst = 0.0
    for k in range(t["valid"].shape[0]):
        material = np.minimum(t["material"][k], tables["count"] - 1)
        miss = (t["valid"][k] != 0) & (t["hit"][k] == 0)
        emitter = (t["valid"][k] != 0) & (t["hit"][k] != 0) & (tables["type"][material] == 3)
        rows = np.flatnonzero(miss | emitter)
        if rows.size == 0:
            continue
        o, d = t["ray_origin"][k][rows], t["ray_direction"][k][rows]
        env = ol.env_eval(rgba, settings.environmentRotation, settings.environmentIntensity, d)[1] if tables["env"] else None
        inputs = np.concatenate([o, d, np.ones((rows.size, 3), np.float32), np.ones((rows.size, 1), np.float32), np.ones((rows.size, 3), np.float32),
                                 np.zeros((rows.size, 1), np.float32)], axis=1)
        light_pdf = osc.light_connection(settings, inputs)["pdf"].astype(np.float64)
        want, bound = K.immediate_radiance(settings, tables, v, k, rows, miss[rows], t["front"][k][rows] != 0, material[rows], t["t"][k][rows].astype(np.float64),
                                           env, light_pdf)
        got = t["immediate"][k][rows].astype(np.float64)
        ratio = np.abs(got - want) / np.maximum(np.abs(want), 1e-300) / bound[:, None]
        assert np.all((ratio <= 1.0) | (got == want)), (name, k, float(ratio.max()))
        worst = max(worst, float(ratio.max()))
        before = K.state_before(v, k)
        uses = (~before["last_delta"][rows]) | bool(settings.enableSpecularNee) | bool(settings.enableMnee)
        escaped += int(miss[rows].sum())
        weighted_escapes += int((miss[rows] & uses & tables["env"]).sum())
        emitters += int(emitter[rows].sum())
        weighted_emitters += int((emitter[rows] & uses & (tables["lights"] > 0) & (light_pdf > 0)).sum())
    if tables["env"]:
        assert weighted_escapes >= 50, (name, weighted_escapes)
    if tables["lights"]:
        assert weighted_emitters >= 50, (name, weighted_emitters)
    return escaped, weighted_escapes, emitters, weighted_emitters, worst


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("path_state_host")
    out = {}
    for name, (build, make, cap) in K.groups().items():
        host = build(tmp)
        settings = make(host)
        out[name] = (host, settings, cap) + K.oracle_vertices(host, settings, cap, ol)
    return out


def test_the_recorder_matches_the_float64_bookkeeping(recorded):
    total = {}
    for name, (host, settings, cap, v, t, radiance, cam, cam_states) in recorded.items():
        tables = K.scene_tables(host)
        near = (t["near"] != 0).any(axis=0)
        assert near.mean() <= K.NEAR_TIE_CAP, (name, near.mean())
        # the first vertex is the camera ray's, with the random state the camera left
        assert np.array_equal(t["rng_entry"][0], cam_states) and np.array_equal(t["ray_direction"][0], cam[:, 3:6]), name
        # nothing but the BSDF sample and roulette draws - and, under a rectangle light, the three numbers of its sample, drawn at every
        # surface that is not a delta one whatever comes of the sample; no group has a sampled environment
        lit = (tables["lights"] > 0) & v["exists"] & ~tables["delta"][np.minimum(t["material"], tables["count"] - 1)]
        three = R.lr.rng_draw(t["rng_entry"].reshape(-1), 3)[1].reshape(t["rng_entry"].shape)
        assert np.array_equal(t["rng_rect"], np.where(lit, three, t["rng_entry"])), name
        # ... and under a sampled environment three more, at the same surfaces
        under_env = tables["env"] & v["exists"] & ~tables["delta"][np.minimum(t["material"], tables["count"] - 1)]
        three = R.lr.rng_draw(t["rng_rect"].reshape(-1), 3)[1].reshape(t["rng_rect"].shape)
        assert np.array_equal(t["rng_env"], np.where(under_env, three, t["rng_rect"])), name
        counts_immediate = check_immediate(name, host, settings, tables, v, t)
        # the medium event is the rule the device test infers it by
        took = v["exists"] & v["valid"]
        dielectric = (tables["type"][np.minimum(t["material"], tables["count"] - 1)] == 2)
        thin = tables["thin"][np.minimum(t["material"], tables["count"] - 1)] & bool(settings.metalSemantics & pt.PTR_METAL_THIN)
        # (asked only where the event is read: with the medium stack on, which every group here pairs with the face-normal rule; without
        # that rule a dielectric hit from the back refracts about a normal that points along the ray, and the rule does not describe it)
        for k in range(cap if settings.metalSemantics & pt.PTR_METAL_MEDIA else 0):
            rows = np.flatnonzero(took[k])
            inferred = R.medium_event((dielectric & ~thin)[k][rows], t["direction"][k][rows], t["normal"][k][rows], t["front"][k][rows] != 0)
            assert np.array_equal(inferred, v["medium_event"][k][rows]), (name, k)
        counts = K.check_vertices(settings, tables, v, name)
        # a path's radiance is the sum of what its vertices added, in their order
        added = np.zeros((len(radiance), 3), np.float32)
        for k in range(cap):
            added = ((added + t["immediate"][k]).astype(np.float32) + t["queued"][k]).astype(np.float32)
        # (to the bit where a vertex adds one term; a vertex that queues several connections adds them one by one, the recorder their sum)
        assert np.array_equal(added, radiance) if tables["lights"] == 0 else np.allclose(added, radiance, rtol=1e-6, atol=0.0), name
        counts["slots"] = [int(((t["queued_mask"] >> k) & 1).sum()) for k in range(R.REC_SLOTS)]
        counts["flushed"] = flushed = int(((t["ended"] != 0) & (t["queued_mask"] != 0)).sum())
        kills = {k: n for k, n in counts["killed"].items() if n}
        spares = {k: n for k, n in counts["spared"].items() if n}
        print("%s: escaped rays %d (MIS-weighted %d), emitter hits %d (MIS-weighted %d), worst %.3f of the bound" % ((name,) + counts_immediate))
        print("%s: paths %d, vertices %d, near ties %.4f, stack at 8: %d, pushes at 8: %d, pops at 0: %d, throughput clamp engaged: %d, roulette "
              "kills by depth %s, spares by depth %s, published at once / flushed: %d / %d, deepest vertex %d, worst throughput deviation %.3f of "
              "its bound, record slots used %s" % (name, len(radiance), counts["vertices"], near.mean(), counts["depth8"], counts["push_at_8"], counts["pop_at_0"],
                             counts["clamped"], kills, spares, len(radiance) - flushed, flushed, counts["max_depth_seen"], counts["worst"], counts["slots"]))
        total[name] = counts
    nested = [c for g, c in total.items() if g.startswith("nested")]
    assert all(c["depth8"] > 0 for g, c in total.items() if g.startswith("nested/through"))
    assert min(c["push_at_8"] for g, c in total.items() if g.startswith("nested/through")) >= 100
    assert all(c["pop_at_0"] > 0 for g, c in total.items() if g.startswith("nested/inside"))
    assert nested
    for g, c in total.items():
        if g.startswith("mixed") or g.startswith("lit") or g == "env":
            for what in ("killed", "spared"):
                by = c[what]
                assert sum(by.values()) >= 50 and by.get(5, 0) > 0 and by.get(6, 0) > 0 and sum(n for k, n in by.items() if k >= 8) > 0, (g, what, by)
            assert not any(n for k, n in c["killed"].items() if k < R.ROULETTE_FROM)
    # the throughput clamp engages: the loader's defaults have it on, and a refraction out of glass weighs more than 1
    assert all(c["clamped"] >= 100 for g, c in total.items() if g.startswith("nested"))
    # record slots 0, 3 and 4 are used under the light (1 and 2 are a sampled environment's), and both ways of publishing occur
    assert total["lit/nee"]["slots"][0] >= 100 and total["lit/spec"]["slots"][3] >= 20 and total["lit/mnee"]["slots"][4] >= 5, [total[g]["slots"] for g in total if g.startswith("lit")]
    assert total["lit/traced"]["slots"][3] >= 20
    assert total["env"]["slots"][1] >= 100 and total["env"]["slots"][2] >= 20, total["env"]["slots"]   # (every one of the five slots is used)
    assert all(50 <= total[g]["flushed"] <= 718 for g in total if g.startswith("lit")) and 10 <= total["env"]["flushed"] <= 718
    assert total["deep"]["max_depth_seen"] == 510


def test_the_thresholds_fall_on_both_sides_of_the_clamp(recorded):
    """roulette's threshold is clamp(maxComp, 0.05, 0.95): in `mixed` paths arrive with maxComp under 0.05, between, and over 0.95"""
    for name in ("mixed/0", "mixed/5"):
        t = recorded[name][4]
        taken = t["roulette"] != 0
        thr = t["roulette_threshold"][taken]
        assert (thr == np.float32(0.05)).sum() >= 10 and (thr == np.float32(0.95)).sum() >= 10 and ((thr > 0.05) & (thr < 0.95)).sum() >= 10, \
            (name, (thr == np.float32(0.05)).sum(), (thr == np.float32(0.95)).sum())


def test_the_accum_schedule():
    """what the device test holds `accum` to, on a path made up here: immediate terms at once, queued terms one visit later, publication
    at the last vertex or, with connections outstanding, one visit after it"""
    imm = np.array([[1.0, 0, 0], [0, 0, 0], [0, 2.0, 0]])
    que = np.array([[0, 0, 4.0], [0, 0, 0], [0, 0, 0]])
    accum, at, flushed, total = R.accum_schedule(imm, que, 2)
    assert at == 2 and not flushed and np.array_equal(total, [1, 2, 4])
    assert np.array_equal(accum[0], [1, 0, 0]) and np.array_equal(accum[1], [1, 0, 4]) and np.array_equal(accum[2], [0, 0, 0])
    que[2] = [8.0, 0, 0]
    accum, at, flushed, total = R.accum_schedule(imm, que, 2)
    assert at == 3 and flushed and np.array_equal(accum[2], [1, 2, 4]) and np.array_equal(total, [9, 2, 4]) and np.array_equal(accum[3], [0, 0, 0])


def test_a_material_table_the_stack_cannot_address_is_refused_at_upload():
    """The medium stack holds 16-bit material ids while the oracle's holds full indices: more than 65536 materials are refused when the
    scene is uploaded, with a message, before a device is looked for (so this needs none); 65536 pass that check."""
    lib = pt.load_library()
    materials = (pt.PtrMaterial * 65537)()
    desc = pt.PtrSceneDesc()
    desc.materials, desc.materialCount = materials, 65537
    handle, err = C.c_void_p(), C.create_string_buffer(512)
    assert lib.ptr_scene_upload(C.byref(desc), 0, C.byref(handle), err, len(err)) != 0 and not handle.value
    message = err.value.decode()
    assert "65537 materials" in message and "at most 65536" in message and "16-bit" in message, message
    desc.materialCount = 65536
    if pt.device_count() == 0:   # (with a device the scene, which has nothing in it, is simply uploaded)
        assert lib.ptr_scene_upload(C.byref(desc), 0, C.byref(handle), err, len(err)) != 0
        assert "materials" not in err.value.decode()
