"""CPU tests of temporal accumulation that carries covariance (include/ptr_temporal_cov.h): the exported surface and its ctypes mirror, the
parameter check, and the numpy restatement the GPU tests compare the kernel with (tests/temporal_cov_ref.py) on cases worked by hand, on
the exact-projection camera of tests/temporal_cases.py.  No GPU.

The test_reference_* tests use nothing of the library; the line under the imports ties the module to the surface it belongs to."""
import ctypes as C
import importlib
import math
import os
import re
import subprocess

import numpy as np

import temporal_cases as tc
import temporal_cov_ref as cref
import temporal_ref as ref

pt = importlib.import_module("metal-pathtracer-arm64_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
assert "ptr_temporal_step_cov" in pt.TEMPORAL_COV_SYMBOLS   # the restatement is of this surface: no surface, no module


# --------------------------------------------------------------------------- the surface
def test_library_exports_every_function_of_the_temporal_cov_header(tmp_path):
    text = open(os.path.join(ROOT, "include", "ptr_temporal_cov.h")).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    found = {name: (kind, 0 if args.strip() in ("", "void") else args.count(",") + 1)
             for kind, name, args in re.findall(r"\b(int|void)\s+(ptr_[a-z_]+)\s*\(([^()]*)\)\s*;", text)}
    assert found == {"ptr_temporal_cov_default_params": ("void", 1), "ptr_temporal_cov_check_params": ("int", 3),
                     "ptr_temporal_create_cov": ("int", 8), "ptr_temporal_step_cov_device": ("int", 13), "ptr_temporal_step_cov": ("int", 12),
                     "ptr_debug_temporal_accumulate_cov": ("int", 21)}
    assert set(found) == set(pt.TEMPORAL_COV_SYMBOLS) and len(pt.TEMPORAL_COV_SYMBOLS) == 6
    lib = pt.load_library()
    for name, (kind, count) in found.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == count and fn.restype is (C.c_int if kind == "int" else None), name
    others = [pt.ABI_SYMBOLS, pt.DEBUG_SYMBOLS, pt.POST_SYMBOLS, pt.STATS_SYMBOLS, pt.ADAPTIVE_SYMBOLS, pt.MULTI_SYMBOLS, pt.FRAME_SYMBOLS,
              pt.MULTI_FRAME_SYMBOLS, pt.DYNAMIC_SYMBOLS, pt.DEFORM_SYMBOLS, pt.DEFORM_DEVICE_SYMBOLS, pt.BACKGROUND_SYMBOLS, pt.TEMPORAL_SYMBOLS,
              pt.PBR_HIT_SYMBOLS, pt.SSS_WALK_SYMBOLS, pt.PATH_STATE_SYMBOLS]
    assert not set(pt.TEMPORAL_COV_SYMBOLS) & set().union(*others)
    assert len(pt.TEMPORAL_SYMBOLS) == 10, "ptr_temporal.h keeps its ten"
    assert [s for s in pt.TEMPORAL_COV_SYMBOLS if s.startswith("ptr_debug_")] == ["ptr_debug_temporal_accumulate_cov"]
    # sizeof and offsetof of the struct against a compiled program
    members = [f for f, _ in pt.PtrTemporalCovParams._fields_]
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "ptr_temporal_cov.h"\nint main() { std::printf("%zu' + " %zu" * len(members) +
                   '\\n", sizeof(PtrTemporalCovParams)' + "".join(", offsetof(PtrTemporalCovParams, %s)" % m for m in members) + "); }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(s) for s in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    mirror = [C.sizeof(pt.PtrTemporalCovParams)] + [getattr(pt.PtrTemporalCovParams, f).offset for f in members]
    assert got == mirror == [8, 0, 4]


def test_default_params():
    p = pt.PtrTemporalCovParams(9.0, 9)
    pt.load_library().ptr_temporal_cov_default_params(C.byref(p))
    assert (p.rejectSigma, p.flags) == (3.0, 0)
    q = pt.PtrTemporalCovParams.defaults(rejectSigma=0.5)
    assert (q.rejectSigma, q.flags) == (0.5, 0)
    pt.load_library().ptr_temporal_cov_default_params(None)   # (ignored)


def test_check_params_refuses_each_bad_value_by_name():
    lib = pt.load_library()
    err = C.create_string_buffer(256)
    for good in ({}, dict(rejectSigma=0.0), dict(rejectSigma=1e-30), dict(rejectSigma=1e30)):
        assert lib.ptr_temporal_cov_check_params(C.byref(pt.PtrTemporalCovParams.defaults(**good)), err, len(err)) == 0, good
    bad = [(dict(rejectSigma=-1.0), "rejectSigma"), (dict(rejectSigma=-1e-30), "rejectSigma"), (dict(rejectSigma=math.nan), "rejectSigma"),
           (dict(rejectSigma=math.inf), "rejectSigma"), (dict(rejectSigma=-math.inf), "rejectSigma"), (dict(flags=1), "flag")]
    for override, word in bad:
        err.value = b""
        assert lib.ptr_temporal_cov_check_params(C.byref(pt.PtrTemporalCovParams.defaults(**override)), err, len(err)) == 1, override
        assert err.value.decode().startswith("ptr_temporal_cov_check_params: ") and word in err.value.decode(), (override, err.value)
    assert lib.ptr_temporal_cov_check_params(None, err, len(err)) == 1 and err.value == b"ptr_temporal_cov_check_params: null argument"


def test_entry_points_refuse_null_arguments_without_a_device():
    lib = pt.load_library()
    err = C.create_string_buffer(256)
    out = C.c_void_p()
    assert lib.ptr_temporal_create_cov(None, 4, 4, None, None, C.byref(out), err, len(err)) == 1 and not out.value
    assert err.value == b"ptr_temporal_create_cov: null argument"
    s = pt.PtrSettings()
    assert lib.ptr_temporal_step_cov(None, C.byref(s), None, None, None, None, None, None, None, None, err, len(err)) == 1
    assert err.value == b"ptr_temporal_step_cov: null argument"
    assert lib.ptr_temporal_step_cov_device(None, C.byref(s), None, None, None, None, None, None, None, None, None, err, len(err)) == 1
    assert err.value == b"ptr_temporal_step_cov_device: null argument"
    a = np.zeros(64, F)
    fp = a.ctypes.data_as(C.POINTER(C.c_float))
    p, cp = pt.PtrTemporalParams.defaults(), pt.PtrTemporalCovParams.defaults()
    args = [1, 1, C.byref(p), C.byref(cp), 1] + [fp] * 8 + [0] + [fp] * 5
    for hole in (2, 3, 6, 10, 15, 18):   # params, cov_params, cov, cov_history, out_cov, out_cov_history
        holed = list(args)
        holed[hole] = None
        err.value = b""
        assert lib.ptr_debug_temporal_accumulate_cov(*holed, err, len(err)) == 1 and err.value == b"ptr_debug_temporal_accumulate_cov: null argument", hole
    # and a bad value is named before any device is looked for
    assert lib.ptr_debug_temporal_accumulate_cov(*(args[:3] + [C.byref(pt.PtrTemporalCovParams.defaults(rejectSigma=-1.0))] + args[4:]), err, len(err)) == 1
    assert b"rejectSigma" in err.value


# --------------------------------------------------------------------------- the restatement, on cases worked by hand
W, H = 16, 8
ZERO4, ZERO6 = np.zeros((H, W, 4), F), np.zeros((H, W, 6), F)


def run(rgb, cov, cur, prev, history, cov_history, cam_prev=None, **kw):
    cam = tc.camera(W, H)
    return cref.accumulate_cov(rgb, cov, cur, prev, history, cov_history, cam, cam if cam_prev is None else cam_prev, **kw)


def diag(value):
    c = np.zeros((H, W, 6), F)
    c[..., :3] = value
    return c


def test_reference_luminance_projections():
    k = np.array([0.2126, 0.7152, 0.0722])
    assert cref.lum(np.array([[1.0, 1.0, 1.0]], F))[0] == F(F(F(0.2126) + F(0.7152)) + F(0.0722))
    c6 = np.array([[2.0, 3.0, 5.0, 0.5, -0.25, 0.125]], F)
    full = np.array([[2.0, 0.5, -0.25], [0.5, 3.0, 0.125], [-0.25, 0.125, 5.0]])
    assert abs(float(cref.lumvar(c6)[0]) - k @ full @ k) < 1e-6
    for bad in ([-1.0, 0, 0, 0, 0, 0], [np.nan, 1, 1, 0, 0, 0], [np.inf, 1, 1, 0, 0, 0], [1, 1, 1, -np.inf, 0, 0], [0, 0, 0, 0, 0, 0]):
        with np.errstate(all="ignore"):
            assert cref.lumvar(np.array([bad], F))[0] == 0, bad


def test_reference_zero_motion_is_the_covariance_of_the_running_mean():
    """N = 1..8 frames: colour, length and colour history are temporal_ref.accumulate's, exactly; the covariance is (sum of the frames'
    covariances) / N^2.  cov_N = ((N-1)/N)^2 cov_{N-1} + C_N / N^2 has at most five roundings a step; a float32 simulation of 2,000 random
    sequences had a worst relative error of 3.1e-7, so rtol 1e-5 leaves a thirty-fold margin."""
    rng = np.random.default_rng(11)
    frames, covs = rng.random((8, H, W, 3)).astype(F), (rng.random((8, H, W, 6)) * 1e-2).astype(F)
    cur, prev = tc.plane_records(W, H)
    got = run(frames[0], covs[0], cur, prev, ZERO4, ZERO6, has_history=False, reject_sigma=0.0)
    want = ref.accumulate(frames[0], cur, prev, ZERO4, tc.camera(W, H), tc.camera(W, H), has_history=False)
    assert all(np.array_equal(g, x) for g, x in zip(got[:3], want)) and np.array_equal(got[3], covs[0]) and np.array_equal(got[4], covs[0])
    for n in range(2, 9):
        want = ref.accumulate(frames[n - 1], cur, prev, want[2], tc.camera(W, H), tc.camera(W, H))
        got = run(frames[n - 1], covs[n - 1], cur, prev, got[2], got[4], reject_sigma=0.0)
        assert all(g.dtype == F for g in got) and all(np.array_equal(g, x) for g, x in zip(got[:3], want)), n
        assert (got[1] == n).all() and np.array_equal(got[3], got[4])
        exact = covs[:n].astype(np.float64).sum(axis=0) / (n * n)
        assert np.allclose(got[3], exact, rtol=1e-5, atol=0), (n, float(np.abs(got[3] / exact - 1).max()))


def test_reference_max_history_settles_at_a_over_two_minus_a():
    """maxHistory 4: a = 1/4 for good, and 40 frames of one covariance C end at C * a / (2 - a) = C / 7 (the fixed point of
    v = (1 - a)^2 v + a^2 C), approached by a factor 9/16 a frame."""
    rng = np.random.default_rng(12)
    c = (rng.random((H, W, 6)) * 1e-2 + 1e-4).astype(F)
    cur, prev = tc.plane_records(W, H)
    frame = np.full((H, W, 3), 0.5, F)
    got = run(frame, c, cur, prev, ZERO4, ZERO6, has_history=False, max_history=4, reject_sigma=0.0)
    for _ in range(39):
        got = run(frame, c, cur, prev, got[2], got[4], max_history=4, reject_sigma=0.0)
    assert (got[1] == 4).all()
    assert np.allclose(got[3], c.astype(np.float64) / 7.0, rtol=1e-5, atol=0), float(np.abs(got[3] / (c.astype(np.float64) / 7.0) - 1).max())


def test_reference_half_pixel_shift_takes_the_mean_of_the_four_taps():
    rng = np.random.default_rng(13)
    c, hist = rng.random((H, W, 3)).astype(F), rng.random((H, W, 3)).astype(F)
    cc, hv = (rng.random((H, W, 6)) * 1e-2).astype(F), (rng.random((H, W, 6)) * 1e-2).astype(F)
    lengths = rng.integers(1, 5, (H, W)).astype(F)
    cur, prev = tc.plane_records(W, H, shift=(0.5, 0.5))
    out, length, _, out_cov, stored = run(c, cc, cur, prev, tc.history_of(hist, lengths), hv, reject_sigma=0.0)
    q = F(0.25)
    for y, x in ((0, 0), (3, 7), (H - 2, W - 2)):
        sv = np.zeros(6, F)
        for t in ((y, x), (y, x + 1), (y + 1, x), (y + 1, x + 1)):
            sv = sv + q * hv[t]
        a = F(1) / length[y, x]
        k = F(1) - a
        assert np.array_equal(out_cov[y, x], (k * k) * sv + (a * a) * cc[y, x]) and np.array_equal(stored[y, x], out_cov[y, x]), (y, x)
        assert np.allclose(sv, hv[y:y + 2, x:x + 2].reshape(4, 6).mean(axis=0), rtol=1e-6)
    # the last column has two taps outside: the two inside renormalise
    y, x = 2, W - 1
    sv = (q * hv[y, x] + q * hv[y + 1, x]) / F(0.5)
    a = F(1) / length[y, x]
    k = F(1) - a
    assert np.array_equal(out_cov[y, x], (k * k) * sv + (a * a) * cc[y, x])


def test_reference_drops_a_tap_from_the_covariance_for_each_reason():
    rng = np.random.default_rng(14)
    c, hist = rng.random((H, W, 3)).astype(F), rng.random((H, W, 3)).astype(F)
    cc, hv = (rng.random((H, W, 6)) * 1e-2).astype(F), (rng.random((H, W, 6)) * 1e-2).astype(F)
    y, x = 3, 5   # the pixel looked at; its taps are (3, 5) (3, 6) (4, 5) (4, 6); the one spoiled is tap 1
    q = F(0.25)

    def spoiled(what):
        cur, prev = tc.plane_records(W, H, shift=(0.5, 0.5))
        history = tc.history_of(hist, 2.0)
        if what == "id":
            prev[0][y, x + 1, 3] = tc.bits([6])[0]
        elif what == "normal":
            prev[1][y, x + 1, :3] = [0.6, 0.0, 0.8]
        elif what == "plane":
            prev[0][y, x + 1, 2] += F(0.125)
        elif what == "length":
            history[y, x + 1, 3] = 0
        elif what == "colour":
            history[y, x + 1, 1] = np.inf
        return run(c, cc, cur, prev, history, hv, reject_sigma=0.0)

    full = spoiled(None)
    a = F(1) / F(3)
    k = F(1) - a
    for what in ("id", "normal", "plane", "length", "colour"):
        out, length, _, out_cov, _ = spoiled(what)
        sv = ((q * hv[y, x] + q * hv[y + 1, x]) + q * hv[y + 1, x + 1]) / F(0.75)
        assert length[y, x] == 3 and np.array_equal(out_cov[y, x], (k * k) * sv + (a * a) * cc[y, x]), what
        assert not np.array_equal(out_cov[y, x], full[3][y, x]), what
        untouched = np.ones((H, W), bool)
        untouched[y - 1:y + 1, x:x + 2] = False
        assert np.array_equal(out_cov[untouched], full[3][untouched]), what


def test_reference_miss_and_non_finite_colours_have_no_covariance():
    rng = np.random.default_rng(15)
    c, hist = rng.random((H, W, 3)).astype(F), rng.random((H, W, 3)).astype(F)
    cc, hv = (rng.random((H, W, 6)) * 1e-2 + 1e-4).astype(F), (rng.random((H, W, 6)) * 1e-2).astype(F)
    cur, prev = tc.plane_records(W, H)
    cur[2][1, 2, 3] = tc.MISS_BITS
    c[4, 9, 0] = np.nan
    c[5, 3, 2] = -np.inf
    for has_history in (True, False):
        out, length, history, out_cov, stored = run(c, cc, cur, prev, tc.history_of(hist, 5.0), hv, has_history=has_history, reject_sigma=0.0)
        for y, x in ((1, 2), (4, 9), (5, 3)):
            assert length[y, x] == 0 and (out_cov[y, x] == 0).all() and (stored[y, x] == 0).all(), (y, x)
        others = np.ones((H, W), bool)
        others[[1, 4, 5], [2, 9, 3]] = False
        assert (out_cov[others] != 0).all()


def test_reference_non_finite_input_covariance_counts_as_zero():
    rng = np.random.default_rng(16)
    c, hist = rng.random((H, W, 3)).astype(F), rng.random((H, W, 3)).astype(F)
    cc, hv = (rng.random((H, W, 6)) * 1e-2).astype(F), (rng.random((H, W, 6)) * 1e-2).astype(F)
    cur, prev = tc.plane_records(W, H)
    spoiled, cleaned = cc.copy(), cc.copy()
    for (y, x, j), value in zip(((1, 1, 0), (2, 5, 3), (6, 11, 5)), (np.nan, np.inf, -np.inf)):
        spoiled[y, x, j] = value
        cleaned[y, x, j] = 0
    for has_history in (True, False):
        for sigma in (0.0, 3.0):
            got = run(c, spoiled, cur, prev, tc.history_of(hist, 3.0), hv, has_history=has_history, reject_sigma=sigma)
            want = run(c, cleaned, cur, prev, tc.history_of(hist, 3.0), hv, has_history=has_history, reject_sigma=sigma)
            assert all(np.array_equal(g, x) for g, x in zip(got, want)) and np.isfinite(got[3]).all()
    first = run(c, spoiled, cur, prev, ZERO4, ZERO6, has_history=False)
    assert np.array_equal(first[3], cleaned)


def test_reference_max_history_one_with_an_infinite_history_covariance_gives_cc():
    """a = 1, k = 0: 0 * inf is NaN, and the final replacement puts Cc there; a finite history covariance gives 0 * H + 1 * Cc = Cc too."""
    rng = np.random.default_rng(17)
    c, hist = rng.random((H, W, 3)).astype(F), rng.random((H, W, 3)).astype(F)
    cc = (rng.random((H, W, 6)) * 1e-2).astype(F)
    hv = np.full((H, W, 6), np.inf, F)
    hv[:, ::2] = 1.0
    cur, prev = tc.plane_records(W, H)
    out, length, _, out_cov, stored = run(c, cc, cur, prev, tc.history_of(hist, 7.0), hv, max_history=1, reject_sigma=0.0)
    assert (length == 1).all() and np.array_equal(out_cov, cc) and np.array_equal(stored, cc)
    assert np.array_equal(out, hist + (c - hist)), "the colour was blended (a = 1), not reset"


def test_reference_resets_the_covariance_behind_the_previous_camera():
    rng = np.random.default_rng(18)
    c, hist = rng.random((H, W, 3)).astype(F), rng.random((H, W, 3)).astype(F)
    cc, hv = (rng.random((H, W, 6)) * 1e-2).astype(F), (rng.random((H, W, 6)) * 1e-2).astype(F)
    cur, prev = tc.plane_records(W, H)
    for origin in ((0.0, 0.0, -2.0), (0.0, 0.0, -1.0)):   # the plane z = -1 behind the previous camera, and in its plane
        out, length, _, out_cov, _ = run(c, cc, cur, prev, tc.history_of(hist, 9.0), hv, cam_prev=tc.camera(W, H, origin=origin), reject_sigma=0.0)
        assert (length == 1).all() and np.array_equal(out, c) and np.array_equal(out_cov, cc)
    out, length, _, out_cov, _ = run(c, cc, cur, prev, tc.history_of(hist, 9.0), hv, reject_sigma=0.0)
    assert (length == 10).all() and not np.array_equal(out_cov, cc)


def test_reference_rejects_a_frame_its_history_cannot_explain():
    """Grey history 1.0 of covariance diag(1e-4) against grey frames of covariance diag(1e-4): lumvar of either is
    1e-4 * (0.2126^2 + 0.7152^2 + 0.0722^2) = 5.619e-5, V = 1.1238e-4, and with sigma 3 the threshold is 9 V = 1.011e-3.  A frame of 2.0
    (d^2 = 1) is rejected, one of 1.01 (d^2 = 1e-4) is kept; sigma 0 keeps both.  The rule makes lumvar finite always, so V is infinite
    only by overflow: a frame covariance diag(3e38) has lumvar 1.69e38, and 9 V is +inf, which no d^2 exceeds: both are kept."""
    cur, prev = tc.plane_records(W, H)
    history, hv, cc = tc.history_of(np.ones((H, W, 3), F), 4.0), diag(1e-4), diag(1e-4)
    v = cref.lumvar(cc)[0, 0] + cref.lumvar(hv)[0, 0]
    assert abs(float(F(9) * v) - 1.011e-3) < 1e-6
    far, near = np.full((H, W, 3), 2.0, F), np.full((H, W, 3), 1.01, F)
    plain = lambda frame: ref.accumulate(frame, cur, prev, history, tc.camera(W, H), tc.camera(W, H))
    # rejected: length 1, out = c, covariance Cc
    out, length, stored, out_cov, _ = run(far, cc, cur, prev, history, hv, reject_sigma=3.0)
    assert (length == 1).all() and np.array_equal(out, far) and np.array_equal(out_cov, cc) and np.array_equal(stored, tc.history_of(far, 1.0))
    # kept: the blend of ptr_temporal.h and the blended covariance
    a = F(1) / F(5)
    k = F(1) - a
    blended = (k * k) * hv + (a * a) * cc
    out, length, _, out_cov, _ = run(near, cc, cur, prev, history, hv, reject_sigma=3.0)
    assert (length == 5).all() and np.array_equal(out, plain(near)[0]) and np.array_equal(out_cov, blended)
    for frame in (far, near):
        out, length, _, out_cov, _ = run(frame, cc, cur, prev, history, hv, reject_sigma=0.0)
        assert (length == 5).all() and np.array_equal(out, plain(frame)[0]) and np.array_equal(out_cov, blended), "sigma 0 never rejects"
        huge = diag(3e38)
        assert np.isfinite(cref.lumvar(huge)).all() and (cref.lumvar(huge) > 1e38).all()
        out, length, _, out_cov, _ = run(frame, huge, cur, prev, history, hv, reject_sigma=3.0)
        assert (length == 5).all() and np.array_equal(out, plain(frame)[0]), "an infinite threshold never rejects"
    # one pixel apart from the rest: only it resets
    mixed = near.copy()
    mixed[2, 3] = 2.0
    out, length, _, out_cov, _ = run(mixed, cc, cur, prev, history, hv, reject_sigma=3.0)
    assert length[2, 3] == 1 and (np.delete(length.ravel(), 2 * W + 3) == 5).all() and np.array_equal(out_cov[2, 3], cc[2, 3])
