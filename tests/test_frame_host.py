"""CPU tests of the resumable-frame surface (include/ptr_frame.h): the exported functions and their ctypes table, the argument checks, the
CLI's --snapshots flag, and the numpy restatement the GPU tests compare the frame with (tests/frame_ref.py) on synthetic samples.

Two refusals - a non-uniform frame given to accumulate, a pixel below 2 samples given to refine - need a frame that exists, and a frame
is created on a device only: tests/test_gpu_frame.py::test_what_a_frame_refuses holds them."""
import ctypes as C
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_ref
import frame_ref

pt = importlib.import_module("metal-pathtracer-arm64_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SIZES = [(1, 1), (5, 3), (67, 45)]


def thresholds(samples):
    """The median and the 0.25 quantile of the dilated error after the first four samples."""
    first = adaptive_ref.adaptive_ref(samples[:4], adaptive_ref.params(4, 4, 4, 0.0))
    return float(np.median(first.E[0])), float(np.quantile(first.E[0], 0.25))


# --------------------------------------------------------------------------- the surface
def test_library_exports_every_function_of_the_frame_header():
    text = open(os.path.join(ROOT, "include", "ptr_frame.h")).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    found = {}
    for ret, name, args in re.findall(r"\b(int|void)\s+(ptr_[a-z_]+)\s*\(([^()]*)\)\s*;", text):
        found[name] = (ret, 0 if args.strip() in ("", "void") else args.count(",") + 1)
    assert set(found) == set(pt.FRAME_SYMBOLS) and len(found) == len(pt.FRAME_SYMBOLS) == 11
    assert found == {"ptr_frame_create": ("int", 5), "ptr_frame_release": ("void", 1), "ptr_frame_reset": ("int", 4),
                     "ptr_frame_accumulate": ("int", 6), "ptr_frame_refine": ("int", 7), "ptr_frame_resolve_device": ("int", 7),
                     "ptr_frame_resolve": ("int", 6), "ptr_frame_info": ("int", 2), "ptr_frame_export": ("int", 8),
                     "ptr_frame_import": ("int", 8), "ptr_frame_debug_create": ("int", 8)}
    lib = pt.load_library()
    for name, (ret, count) in found.items():
        assert hasattr(lib, name), name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == count, name
        assert fn.restype is (C.c_int if ret == "int" else None), name
    others = set(pt.ABI_SYMBOLS) | set(pt.DEBUG_SYMBOLS) | set(pt.POST_SYMBOLS) | set(pt.STATS_SYMBOLS) | set(pt.ADAPTIVE_SYMBOLS) | set(pt.MULTI_SYMBOLS)
    assert not set(pt.FRAME_SYMBOLS) & others


def test_ctypes_mirrors_have_the_headers_sizes():
    assert C.sizeof(pt.PtrFrameInfo) == 32 and pt.PtrFrameInfo.totalSamples.offset == 16 and pt.PtrFrameInfo.uniform.offset == 24
    assert C.sizeof(pt.PtrAdaptiveParams) == 16 and C.sizeof(pt.PtrAdaptiveInfo) == 16 + 4 * 32
    assert [k for k, _, _ in pt.FRAME_STATE] == list(adaptive_ref.zero_state(1))


# --------------------------------------------------------------------------- bad arguments
def _call(name, *args):
    err = C.create_string_buffer(256)
    rc = getattr(pt.load_library(), name)(*args, err, len(err))
    return rc, err.value.decode()


def _refused(name, *args):
    rc, message = _call(name, *args)
    assert rc == 1 and message.startswith(name + ":"), (name, rc, message)
    return message


def test_bad_arguments_are_refused_by_name():
    """`frame` and `scene` are made-up handles: a bad argument must be refused before anything looks behind them."""
    frame, scene = C.c_void_p(0x1000), C.c_void_p(0x1000)
    settings = pt.PtrSettings()
    settings.width, settings.height, settings.maxDepth = 8, 8, 2
    no_width, no_height, huge = settings.copy(), settings.copy(), settings.copy()
    no_width.width, no_height.height = 0, 0
    huge.width = huge.height = 0x10000
    out = C.c_void_p()
    for args in ((None, C.byref(settings), C.byref(out)), (scene, None, C.byref(out)), (scene, C.byref(settings), None),
                 (scene, C.byref(no_width), C.byref(out)), (scene, C.byref(no_height), C.byref(out)), (scene, C.byref(huge), C.byref(out))):
        _refused("ptr_frame_create", *args)
    assert not out.value
    samples = np.ones((2, 8, 8, 4), np.float32)
    sp = samples.ctypes.data_as(C.POINTER(C.c_float))
    for args in ((8, 8, None, 2, 0, C.byref(out)), (8, 8, sp, 2, 0, None), (0, 8, sp, 2, 0, C.byref(out)), (8, 0, sp, 2, 0, C.byref(out)),
                 (8, 8, sp, 0, 0, C.byref(out)), (0x10000, 0x10000, sp, 2, 0, C.byref(out))):
        _refused("ptr_frame_debug_create", *args)
    assert not out.value
    _refused("ptr_frame_reset", None, C.byref(settings))
    _refused("ptr_frame_accumulate", None, 4, None, None)
    assert "spp" in _refused("ptr_frame_accumulate", frame, 0, None, None)
    good = pt.PtrAdaptiveParams(4, 16, 4, 0.1)
    _refused("ptr_frame_refine", None, C.byref(good), None, None, None)
    _refused("ptr_frame_refine", frame, None, None, None, None)
    rgb = np.full((8, 8, 3), 7.0, np.float32)
    fp = rgb.ctypes.data_as(C.POINTER(C.c_float))
    _refused("ptr_frame_resolve", None, fp, None, None)
    _refused("ptr_frame_resolve", frame, None, None, None)
    _refused("ptr_frame_resolve_device", None, C.c_void_p(rgb.ctypes.data), None, None, None)
    _refused("ptr_frame_resolve_device", frame, None, None, None, None)
    st = adaptive_ref.zero_state(64)
    f = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    u = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    full = [frame, f(st["sum"]), f(st["mean"]), f(st["m"]), u(st["n"]), f(st["e"])]
    for name in ("ptr_frame_export", "ptr_frame_import"):
        for drop in range(6):
            args = list(full)
            args[drop] = None
            _refused(name, *args)
    info = pt.PtrFrameInfo()
    assert pt.load_library().ptr_frame_info(None, C.byref(info)) == 1 and pt.load_library().ptr_frame_info(frame, None) == 1
    assert (rgb == 7.0).all()


def test_bad_refine_parameters_are_refused_by_name():
    """Behind a handle that is never dereferenced: the parameters are checked before the frame is looked at."""
    bad = [pt.PtrAdaptiveParams(1, 16, 4, 0.1), pt.PtrAdaptiveParams(0, 16, 4, 0.1), pt.PtrAdaptiveParams(8, 7, 4, 0.1),
           pt.PtrAdaptiveParams(4, 16, 0, 0.1), pt.PtrAdaptiveParams(4, 16, 4, -0.5), pt.PtrAdaptiveParams(4, 16, 4, math.nan),
           pt.PtrAdaptiveParams(4, 16, 4, math.inf)]
    for p in bad:
        _refused("ptr_frame_refine", C.c_void_p(0x1000), C.byref(p), None, None, None)
    assert "minSpp" in _refused("ptr_frame_refine", C.c_void_p(0x1000), C.byref(bad[0]), None, None, None)


def test_frames_fail_loudly_without_gpu():
    if pt.device_count() > 0:
        pytest.skip("a GPU is present")
    settings = pt.PtrSettings()
    settings.width, settings.height, settings.maxDepth = 8, 8, 2
    out = C.c_void_p()
    rc, message = _call("ptr_frame_create", C.c_void_p(0x1000), C.byref(settings), C.byref(out))
    assert rc == 2 and message.startswith("ptr_frame_create:") and "no CPU fallback" in message and not out.value
    samples = np.ones((2, 8, 8, 4), np.float32)
    rc, message = _call("ptr_frame_debug_create", 8, 8, samples.ctypes.data_as(C.POINTER(C.c_float)), 2, 0, C.byref(out))
    assert rc == 2 and message.startswith("ptr_frame_debug_create:") and "no CPU fallback" in message and not out.value
    with pytest.raises(pt.PtrError, match="no CPU fallback"):
        pt.debug_frame(samples)


def test_cli_documents_and_checks_the_snapshots_flag():
    helped = subprocess.run([pt.CLI_PATH, "--help"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert helped.returncode == 0 and "--snapshots=<n1,n2,...>" in helped.stdout
    scene = os.path.join(GOLDEN, "smoke.scene")
    run = lambda *flags: subprocess.run([pt.CLI_PATH, "--scene=" + scene, "--sppTotal=16", *flags], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                        text=True)
    for flags in (("--snapshots=4,8", "--adaptive"), ("--snapshots=4,8", "--devices=2"), ("--snapshots=4,8", "--devices=0"), ("--snapshots=8,4",),
                  ("--snapshots=4,4",), ("--snapshots=1,4",), ("--snapshots=4,16",), ("--snapshots=4,x",), ("--snapshots=",), ("--snapshots=4,,8",)):
        res = run(*flags)
        assert res.returncode == 1 and "--snapshots" in res.stdout, (flags, res.stdout)
        assert "HIP" not in res.stdout, flags                          # refused with a message, before any device call


# --------------------------------------------------------------------------- the sanitizer program
def test_the_stand_alone_host_check_builds_and_runs_clean(tmp_path):
    """tools/frame_host_check.cpp with -fsanitize=address,undefined: a stand-alone program on the CPU with its own main and the
    sanitizers' runtimes linked in.  It walks the per-element bodies of csrc/kernels/frame.h over every image size 1x1 .. 130x70 and
    holds the frames' table of pixels per count (csrc/host/frame_classes.h) against the histogram of the counts after every move."""
    csrc = os.path.join(ROOT, "metal-pathtracer-arm64_amd", "csrc")
    exe = tmp_path / "frame_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(csrc, "host"), "-I", os.path.join(csrc, "kernels"),
                    os.path.join(ROOT, "tools", "frame_host_check.cpp"), "-o", str(exe)], check=True)
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout
    m = re.fullmatch(r"frame host check: (\d+) entries visited, (\d+) in their round's class, (\d+) kept, (\d+) dropped, (\d+) class moves, no finding",
                     res.stdout.strip())
    assert m, res.stdout
    visited, in_class, kept, dropped, moves = (int(v) for v in m.groups())
    assert visited == kept + dropped and 0 < in_class < visited and kept > 0 and dropped > 0
    assert moves >= 130 * 70      # at least one move per image size
    assert "runtime error" not in res.stdout and "AddressSanitizer" not in res.stdout


# --------------------------------------------------------------------------- the restatement's own laws
def uniform_state(x, n):
    """The state of a uniform frame of n samples, through adaptive_ref alone."""
    h, w = x.shape[1:3]
    order = adaptive_ref.pixel_order(w, h)
    st, _, _ = adaptive_ref.round_ref(w, h, adaptive_ref.params(2, n, 1, 0.0), 0, x[:n].reshape(n, h * w, 3)[:, order], order,
                                      adaptive_ref.zero_state(h * w))
    return st


@pytest.mark.parametrize("w,h", SIZES)
def test_a_frame_continued_is_the_adaptive_frame_and_every_pixel_is_uniform(w, h):
    x = adaptive_ref.synthetic_samples(24, h, w)
    thr, thr2 = thresholds(x)
    fr = frame_ref.FrameRef(x)
    fr.accumulate(3)
    fr.accumulate(1)
    fr.refine(adaptive_ref.params(4, 16, 4, thr))
    want = adaptive_ref.adaptive_ref(x[:16], adaptive_ref.params(4, 16, 4, thr))
    rgb, cov, count = fr.resolve()
    assert np.array_equal(count, want.count)
    assert np.array_equal(rgb, want.rgb, equal_nan=True) and np.array_equal(cov, want.cov, equal_nan=True)
    # ... and an empty frame refined is that frame with its rounds
    whole = frame_ref.FrameRef(x)
    info = whole.refine(adaptive_ref.params(4, 16, 4, thr))
    assert info.rounds == want.rounds and info.active_after == want.active_after and info.total_samples == int(want.count.sum())
    assert all(np.array_equal(whole.state[k], fr.state[k], equal_nan=True) for k in fr.state)
    assert all(n_s == n_l_before for (_, n_s, _), n_l_before in zip(whole.log, want.active_after))      # S = L in every round
    # a second refine: every pixel is the uniform pixel of its count
    before = fr.state["n"].copy()
    info = fr.refine(adaptive_ref.params(4, 24, 4, thr2))
    assert info.total_samples == int((fr.state["n"] - before).sum())
    assert info.pixels_at_max == int((fr.state["n"] == 24).sum())
    for n in np.unique(fr.state["n"]):
        u = uniform_state(x, int(n))
        sel = fr.state["n"] == n
        for k in ("sum", "mean", "m", "e"):
            assert np.array_equal(fr.state[k][sel], u[k][sel], equal_nan=True), (k, int(n))


def test_the_second_refine_mixes_classes():
    """Conditions on the input at 67x45, from the restatement alone."""
    w, h = 67, 45
    x = adaptive_ref.synthetic_samples(24, h, w)
    thr, thr2 = thresholds(x)
    assert abs(thr - 0.7363) < 5e-5 and abs(thr2 - 0.6003) < 5e-5
    fr = frame_ref.FrameRef(x)
    fr.refine(adaptive_ref.params(4, 16, 4, thr))
    first = fr.state["n"].copy()
    start = len(fr.log)
    info = fr.refine(adaptive_ref.params(4, 24, 4, thr2))
    log = fr.log[start:]
    # |L| before each round: the start list (every pixel of it gets samples before the loop ends), then the lengths after
    before = [int((fr.state["n"] > first).sum())] + [n_l for _, _, n_l in log[:-1]]
    mixed = sum(1 for (_, n_s, _), n_l in zip(log, before) if n_s < n_l)      # rounds in which S is a strict subset of L
    resumed = int(((first == 4) & (fr.state["n"] > 4)).sum())
    counts = sorted(int(v) for v in np.unique(fr.state["n"]))
    print("rounds %d of which %d mixed; %d pixels resumed from 4 samples; counts %s; log %s" % (info.rounds, mixed, resumed, counts, log))
    assert info.rounds == len(log) and mixed >= 2 and resumed >= 100 and len(counts) >= 4
    assert (info.rounds, mixed, resumed, counts) == (5, 3, 800, [4, 8, 12, 16, 20, 24])
