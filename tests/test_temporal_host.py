"""CPU tests of temporal accumulation (include/ptr_temporal.h): the exported surface and its ctypes mirror, the parameter check, and the
numpy restatement the GPU tests compare the kernels with (tests/temporal_ref.py) on cases worked by hand.  No GPU.

The test_reference_* tests below check the restatement itself, against arithmetic done by hand, and use nothing of the library: they
are what makes tests/test_gpu_temporal.py's bit-for-bit comparisons mean something, and they would pass on a tree without the feature
but for the line under the imports, which ties the module to the surface it belongs to."""
import ctypes as C
import importlib
import math
import os
import re
import subprocess

import numpy as np

import temporal_cases as tc
import temporal_ref as ref

pt = importlib.import_module("metal-pathtracer-arm64_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
assert "ptr_temporal_step" in pt.TEMPORAL_SYMBOLS   # the restatement is of this surface: no surface, no module


# --------------------------------------------------------------------------- the surface
def test_library_exports_every_function_of_the_temporal_header(tmp_path):
    text = open(os.path.join(ROOT, "include", "ptr_temporal.h")).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    found = {name: (kind, 0 if args.strip() in ("", "void") else args.count(",") + 1)
             for kind, name, args in re.findall(r"\b(int|void)\s+(ptr_[a-z_]+)\s*\(([^()]*)\)\s*;", text)}
    assert found == {"ptr_temporal_default_params": ("void", 1), "ptr_temporal_check_params": ("int", 3), "ptr_temporal_create": ("int", 7),
                     "ptr_temporal_release": ("void", 1), "ptr_temporal_reset": ("int", 1), "ptr_temporal_step_device": ("int", 11),
                     "ptr_temporal_step": ("int", 10), "ptr_debug_temporal_accumulate": ("int", 16), "ptr_debug_temporal_records": ("int", 6),
                     "ptr_debug_temporal_camera": ("int", 2)}
    assert set(found) == set(pt.TEMPORAL_SYMBOLS) and len(pt.TEMPORAL_SYMBOLS) == 10
    lib = pt.load_library()
    for name, (kind, count) in found.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == count and fn.restype is (C.c_int if kind == "int" else None), name
    others = [pt.ABI_SYMBOLS, pt.DEBUG_SYMBOLS, pt.POST_SYMBOLS, pt.STATS_SYMBOLS, pt.ADAPTIVE_SYMBOLS, pt.MULTI_SYMBOLS, pt.FRAME_SYMBOLS,
              pt.MULTI_FRAME_SYMBOLS, pt.DYNAMIC_SYMBOLS, pt.DEFORM_SYMBOLS, pt.DEFORM_DEVICE_SYMBOLS, pt.BACKGROUND_SYMBOLS]
    assert not set(pt.TEMPORAL_SYMBOLS) & set().union(*others)
    # the probes of this header live in this header's list alone
    assert [s for s in pt.TEMPORAL_SYMBOLS if s.startswith("ptr_debug_")] == ["ptr_debug_temporal_accumulate", "ptr_debug_temporal_records",
                                                                             "ptr_debug_temporal_camera"]
    # sizeof and offsetof of the two structs against a compiled program
    members = [("PtrTemporalParams", f) for f, _ in pt.PtrTemporalParams._fields_] + [("PtrTemporalInfo", f) for f, _ in pt.PtrTemporalInfo._fields_]
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "ptr_temporal.h"\nint main() { std::printf("%zu %zu' + " %zu" * len(members) +
                   '\\n", sizeof(PtrTemporalParams), sizeof(PtrTemporalInfo)' + "".join(", offsetof(%s, %s)" % m for m in members) + "); }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(s) for s in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    mirror = [C.sizeof(pt.PtrTemporalParams), C.sizeof(pt.PtrTemporalInfo)] + [getattr(getattr(pt, s), f).offset for s, f in members]
    assert got == mirror == [16, 32, 0, 4, 8, 12, 0, 4, 8, 16, 24]


def test_default_params():
    p = pt.PtrTemporalParams(9, 9.0, 9.0, 9)
    pt.load_library().ptr_temporal_default_params(C.byref(p))
    assert (p.maxHistory, p.normalCos, p.planeTolerance, p.flags) == (32, F(0.9), F(0.01), 0)
    q = pt.PtrTemporalParams.defaults(maxHistory=4)
    assert (q.maxHistory, q.normalCos, q.flags) == (4, F(0.9), 0)
    pt.load_library().ptr_temporal_default_params(None)   # (ignored)


def test_check_params_refuses_each_bad_value_by_name():
    lib = pt.load_library()
    err = C.create_string_buffer(256)
    assert lib.ptr_temporal_check_params(C.byref(pt.PtrTemporalParams.defaults()), err, len(err)) == 0
    for good in (dict(maxHistory=1), dict(maxHistory=65535), dict(normalCos=-1.0), dict(normalCos=1.0), dict(planeTolerance=1e-30)):
        assert lib.ptr_temporal_check_params(C.byref(pt.PtrTemporalParams.defaults(**good)), err, len(err)) == 0, good
    bad = [(dict(maxHistory=0), "maxHistory"), (dict(maxHistory=65536), "maxHistory"), (dict(normalCos=1.5), "normalCos"),
           (dict(normalCos=math.nan), "normalCos"), (dict(planeTolerance=0.0), "planeTolerance"), (dict(planeTolerance=-1.0), "planeTolerance"),
           (dict(planeTolerance=math.nan), "planeTolerance"), (dict(flags=1), "flag")]
    for override, word in bad:
        err.value = b""
        assert lib.ptr_temporal_check_params(C.byref(pt.PtrTemporalParams.defaults(**override)), err, len(err)) == 1, override
        assert err.value.decode().startswith("ptr_temporal_check_params: ") and word in err.value.decode(), (override, err.value)
    assert lib.ptr_temporal_check_params(None, err, len(err)) == 1 and b"null argument" in err.value


def test_entry_points_refuse_null_arguments_without_a_device():
    lib = pt.load_library()
    err = C.create_string_buffer(256)
    out = C.c_void_p()
    assert lib.ptr_temporal_create(None, 4, 4, None, C.byref(out), err, len(err)) == 1 and b"null argument" in err.value and not out.value
    s = pt.PtrSettings()
    assert lib.ptr_temporal_step(None, C.byref(s), None, None, None, None, None, None, err, len(err)) == 1 and b"null argument" in err.value
    assert lib.ptr_temporal_step_device(None, C.byref(s), None, None, None, None, None, None, None, err, len(err)) == 1
    assert err.value == b"ptr_temporal_step_device: null argument"
    assert lib.ptr_temporal_reset(None) == 1
    assert lib.ptr_debug_temporal_records(None, None, None, None, err, len(err)) == 1 and b"null argument" in err.value
    assert lib.ptr_debug_temporal_camera(None, None) == 1
    lib.ptr_temporal_release(None)


def test_camera_probe_is_the_camera_the_rays_come_from():
    """ptr_debug_temporal_camera needs no device; the rays of ptr_debug_camera_rays do (test_gpu_temporal.py compares them).  Here: the
    geometry buildCamera promises - horizontal and vertical perpendicular, the viewport centred on the axis to the target."""
    s = pt.PtrSettings()
    s.width, s.height = 96, 64
    s.cameraVerticalFov, s.cameraDistance, s.cameraYaw, s.cameraPitch = 40.0, 5.0, 0.3, 0.2
    s.cameraTarget[:] = [0.5, 1.0, -0.25]
    o, ll, h, w = pt.debug_temporal_camera(s).astype(np.float64)
    assert abs(h @ w) < 1e-5 and abs(np.linalg.norm(h) / np.linalg.norm(w) - 1.5) < 1e-5
    centre = ll + 0.5 * h + 0.5 * w
    axis = (centre - o) / np.linalg.norm(centre - o)
    to_target = np.array([0.5, 1.0, -0.25]) - o
    assert np.allclose(axis, to_target / np.linalg.norm(to_target), atol=1e-5) and abs(np.linalg.norm(to_target) - 5.0) < 1e-4


# --------------------------------------------------------------------------- the restatement, on cases worked by hand
W, H = 16, 8


def run(rgb, cur, prev, history, cam_prev=None, **kw):
    cam = tc.camera(W, H)
    return ref.accumulate(rgb, cur, prev, history, cam, cam if cam_prev is None else cam_prev, **kw)


def test_reference_zero_motion_is_the_sequential_running_mean():
    rng = np.random.default_rng(1)
    frames = rng.random((6, H, W, 3)).astype(F)
    cur, prev = tc.plane_records(W, H)
    out, length, history = run(frames[0], cur, prev, np.zeros((H, W, 4), F), has_history=False)
    assert np.array_equal(out, frames[0]) and (length == 1).all() and np.array_equal(history, tc.history_of(frames[0], 1.0))
    mean = frames[0]
    for k in range(2, 7):
        out, length, history = run(frames[k - 1], cur, prev, history)
        mean = mean + (frames[k - 1] - mean) * (F(1) / F(k))
        assert out.dtype == F and np.array_equal(out, mean) and (length == k).all(), k
        assert np.array_equal(history, tc.history_of(mean, float(k)))
    assert np.allclose(out, frames.mean(axis=0), atol=1e-6)


def test_reference_integer_shift_takes_the_history_of_the_shifted_pixel():
    rng = np.random.default_rng(2)
    c, hist = rng.random((H, W, 3)).astype(F), rng.random((H, W, 3)).astype(F)
    cur, prev = tc.plane_records(W, H, shift=(3, -2))
    out, length, _ = run(c, cur, prev, tc.history_of(hist, 3.0))
    for y in range(H):
        for x in range(W):
            if 0 <= x + 3 < W and 0 <= y - 2 < H:
                h = hist[y - 2, x + 3]
                assert length[y, x] == 4 and np.array_equal(out[y, x], h + (c[y, x] - h) * F(0.25)), (x, y)
            else:   # the source lies outside the image
                assert length[y, x] == 1 and np.array_equal(out[y, x], c[y, x]), (x, y)


def test_reference_half_pixel_shift_is_four_taps_of_a_quarter():
    rng = np.random.default_rng(3)
    c, hist = rng.random((H, W, 3)).astype(F), rng.random((H, W, 3)).astype(F)
    lengths = rng.integers(1, 5, (H, W)).astype(F)
    cur, prev = tc.plane_records(W, H, shift=(0.5, 0.5))
    out, length, _ = run(c, cur, prev, tc.history_of(hist, lengths))
    q = F(0.25)
    for y, x in ((0, 0), (3, 7), (H - 2, W - 2)):
        taps = [(y, x), (y, x + 1), (y + 1, x), (y + 1, x + 1)]
        big_b, sc, sn = F(0), np.zeros(3, F), F(0)
        for t in taps:
            big_b, sc, sn = big_b + q, sc + q * hist[t], sn + q * lengths[t]
        assert big_b == 1
        n = min(sn / big_b + F(1), F(32))
        assert length[y, x] == n and np.array_equal(out[y, x], sc + (c[y, x] - sc) * (F(1) / n))
    # the last column and row have two taps outside: the two inside renormalise
    y, x = 2, W - 1
    sc = (q * hist[y, x] + q * hist[y + 1, x]) / F(0.5)
    n = (q * lengths[y, x] + q * lengths[y + 1, x]) / F(0.5) + F(1)
    assert length[y, x] == n and np.array_equal(out[y, x], sc + (c[y, x] - sc) * (F(1) / n))


def test_reference_drops_a_tap_for_each_reason_and_renormalises():
    rng = np.random.default_rng(4)
    c, hist = rng.random((H, W, 3)).astype(F), rng.random((H, W, 3)).astype(F)
    y, x = 3, 5   # the pixel looked at; its taps are (3, 5) (3, 6) (4, 5) (4, 6); the one spoiled is tap 1
    q = F(0.25)

    def spoiled(what):
        cur, prev = tc.plane_records(W, H, shift=(0.5, 0.5))
        history = tc.history_of(hist, 2.0)
        if what == "id":
            prev[0][y, x + 1, 3] = tc.bits([6])[0]
        elif what == "normal":
            prev[1][y, x + 1, :3] = [0.6, 0.0, 0.8]   # cosine 0.8 < 0.9; the plane test alone would pass (distance 0)
        elif what == "plane":
            prev[0][y, x + 1, 2] += F(0.125)          # 0.125 off the plane > 0.01 * |Xprev - o| ~ 0.01
        elif what == "length":
            history[y, x + 1, 3] = 0
        elif what == "colour":
            history[y, x + 1, 1] = np.inf
        return run(c, cur, prev, history)

    full = spoiled(None)
    assert full[1][y, x] == 3
    for what in ("id", "normal", "plane", "length", "colour"):
        out, length, _ = spoiled(what)
        sc = ((q * hist[y, x] + q * hist[y + 1, x]) + q * hist[y + 1, x + 1]) / F(0.75)
        assert length[y, x] == 3 and np.array_equal(out[y, x], sc + (c[y, x] - sc) * (F(1) / F(3))), what
        assert not np.array_equal(out[y, x], full[0][y, x]), what
        untouched = np.ones((H, W), bool)
        untouched[y - 1:y + 1, x:x + 2] = False   # the four pixels that have the spoiled pixel among their taps
        assert np.array_equal(out[untouched], full[0][untouched]), what


def test_reference_max_history_turns_the_mean_into_a_fixed_blend():
    rng = np.random.default_rng(5)
    frames = rng.random((7, H, W, 3)).astype(F)
    cur, prev = tc.plane_records(W, H)
    out, length, history = run(frames[0], cur, prev, np.zeros((H, W, 4), F), has_history=False, max_history=4)
    for k in range(2, 8):
        before = history[..., :3]
        out, length, history = run(frames[k - 1], cur, prev, history, max_history=4)
        a = F(1) / F(min(k, 4))
        assert (length == min(k, 4)).all() and np.array_equal(out, before + (frames[k - 1] - before) * a), k
    # maxHistory 1: a = 1, the frame itself up to the rounding of hist + (c - hist)
    before = history[..., :3]
    out1, length1, _ = run(frames[1], cur, prev, history, max_history=1)
    assert np.array_equal(out1, before + (frames[1] - before)) and np.allclose(out1, frames[1], atol=2e-7) and (length1 == 1).all()


def test_reference_copies_miss_and_nan_pixels_through_with_length_zero():
    rng = np.random.default_rng(6)
    c, hist = rng.random((H, W, 3)).astype(F), rng.random((H, W, 3)).astype(F)
    cur, prev = tc.plane_records(W, H)
    cur[2][1, 2, 3] = tc.MISS_BITS
    c[4, 9, 0] = np.nan
    c[5, 3, 2] = -np.inf
    for has_history in (True, False):
        out, length, history = run(c, cur, prev, tc.history_of(hist, 5.0), has_history=has_history)
        for y, x in ((1, 2), (4, 9), (5, 3)):
            assert length[y, x] == 0 and history[y, x, 3] == 0 and np.array_equal(out[y, x], c[y, x], equal_nan=True), (y, x)
            assert np.array_equal(history[y, x, :3], c[y, x], equal_nan=True)
        others = np.ones((H, W), bool)
        others[[1, 4, 5], [2, 9, 3]] = False
        assert (length[others] == (6 if has_history else 1)).all() and np.isfinite(out[others]).all()
    # as a tap, a pixel stored with length 0 gives nothing: the following frame resets there and nowhere else
    out2, length2, _ = run(hist, *tc.plane_records(W, H), history)
    assert length2[1, 2] == 1 and length2[4, 9] == 1 and length2[0, 0] == 2


def test_reference_resets_a_point_behind_the_previous_camera():
    rng = np.random.default_rng(7)
    c, hist = rng.random((H, W, 3)).astype(F), rng.random((H, W, 3)).astype(F)
    cur, prev = tc.plane_records(W, H)
    behind = tc.camera(W, H, origin=(0.0, 0.0, -2.0))   # the plane z = -1 lies behind a camera at z = -2 looking down -z
    out, length, _ = run(c, cur, prev, tc.history_of(hist, 9.0), cam_prev=behind)
    assert (length == 1).all() and np.array_equal(out, c)
    in_plane = tc.camera(W, H, origin=(0.0, 0.0, -1.0))   # ... and in the plane of one at z = -1: den = 0
    out, length, _ = run(c, cur, prev, tc.history_of(hist, 9.0), cam_prev=in_plane)
    assert (length == 1).all() and np.array_equal(out, c)
    out, length, _ = run(c, cur, prev, tc.history_of(hist, 9.0))
    assert (length == 10).all()
